"""CPU: the trainers' random stream as tests/train_random_ref.py states it (the generator's known answers, the
statistics of the mask and of the shifts), and the argument errors of the seeded trainers, which must come before any
GPU call."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import train_random_ref as R  # noqa: E402


def test_known_answers():
    for counter, key, words in R.KNOWN:
        got = R.philox4x32([counter], [key])[0]
        assert tuple(int(w) for w in got) == words, [hex(int(w)) for w in got]
    counters = np.array([k[0] for k in R.KNOWN], np.uint32)
    keys = np.array([k[1] for k in R.KNOWN], np.uint32)
    assert np.array_equal(R.philox4x32(counters, keys), np.array([k[2] for k in R.KNOWN], np.uint32))


def test_words_are_counted_by_element_site_and_epoch():
    w = R.words(2 ** 63 + 5, 7, R.SITE_SHIFT, 10)
    for i in (0, 3, 4, 9):
        ref = R.philox4x32([(i // 4, R.SITE_SHIFT, 7, 0)], [(5, 2 ** 31)])[0][i % 4]
        assert w[i] == ref
    assert not np.array_equal(w, R.words(2 ** 63 + 5, 8, R.SITE_SHIFT, 10))
    assert not np.array_equal(w, R.words(2 ** 63 + 5, 7, R.SITE_DROPOUT, 10))


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_kept_fraction(p):
    n = 10 ** 6
    mask = R.dropout_mask(12345, 3, 1000, 1000, p)
    kept = int(np.count_nonzero(mask))
    sd = np.sqrt(n * p * (1 - p))
    print(f"p = {p}: kept {kept} of {n}, expected {n * (1 - p):.0f}, {abs(kept - n * (1 - p)) / sd:.2f} standard deviations")
    assert abs(kept - n * (1 - p)) <= 5 * sd
    assert set(np.unique(mask)) == {np.float32(0.0), np.float32(1.0 / (1.0 - p))}
    assert R.threshold(p) == int(p * 2 ** 32) and R.threshold(0.0) == 0
    assert np.all(R.dropout_mask(1, 0, 3, 5, 0.0) == 1.0)


@pytest.mark.parametrize("m", [1, 3, 16])
def test_shifts_cover_their_range(m):
    s = R.shifts(99, 2, 4000, m)
    assert s.dtype == np.int32 and s.min() == -m and s.max() == m
    assert set(np.unique(s)) == set(range(-m, m + 1))
    assert np.all(R.shifts(99, 2, 50, 0) == 0)


def test_reference_windows_are_a_gather():
    audio, onsets, _y = R.synthetic_hits(1, 5, 3, 16, 4)
    starts = onsets.min(1) - 2
    sh, win = R.shifted_windows(audio, starts, 16, 6, 1, 4, 2)
    assert win.shape == (10, 3, 16) and sh.shape == (10,)
    for j in (0, 4, 5, 9):
        s0 = starts[j % 5] + sh[j]
        assert np.array_equal(win[j], audio[s0:s0 + 16].T)


def test_argument_errors_come_before_any_gpu_call(monkeypatch):
    from onset_fingerprinting_amd import _lib, data, model

    def no_gpu(*a, **k):
        raise AssertionError("a GPU call was made before the arguments were checked")

    monkeypatch.setattr(_lib, "require_gpu", no_gpu)
    monkeypatch.setattr(_lib, "lib", no_gpu)
    x, y = torch.zeros(8, 3, 32), torch.zeros(8, 2)
    cases = [(model.fit_cnn, model.cnn_loss_and_grads_device, lambda p: model.CNN(32, 2, dropout_rate=p)),
             (model.fit_lcccnn, model.cccnn_loss_and_grads_device, lambda p: model.LCCCNN(32, 2, dropout_rate=p))]
    audio = np.zeros((400, 3), np.float32)
    onsets = np.array([[50, 52, 51], [150, 151, 153], [250, 250, 250]])
    for fit, grads, make in cases:
        # without a seed the class default of 0.5 is refused as before, and the text says how to opt in
        with pytest.raises(ValueError, match="dropout_rate=0.0"):
            fit(make(0.5), x, y)
        with pytest.raises(ValueError, match="or pass seed= for this package's own dropout stream"):
            fit(make(0.5), x, y)
        with pytest.raises(ValueError, match="dropout_rate=0.0"):
            grads(make(0.5), x, y)
        for bad in (-1, 2 ** 64, 1.5, "7", True):
            with pytest.raises(ValueError, match="seed"):
                fit(make(0.5), x, y, seed=bad)
            with pytest.raises(ValueError, match="seed"):
                grads(make(0.0), x, y, seed=bad)
        m = make(0.5)
        (m.dropout if fit is model.fit_cnn else m.model.dropout).p = 1.0
        with pytest.raises(ValueError, match="dropout_rate < 1"):
            fit(m, x, y, seed=1)
        with pytest.raises(ValueError, match="dropout_rate < 1"):
            grads(m, x, y, seed=1)
        src = data.ShiftedWindows(audio, onsets, 32, pre_samples=4, max_shift=3, n_extractions=2)
        assert (src.n, src.n_onsets, src.channels, src.frame_length) == (6, 3, 3, 32)
        with pytest.raises(ValueError, match="x_val"):
            fit(make(0.0), x, y, x_val=src, y_val=torch.zeros(3, 2), seed=1)
        with pytest.raises(ValueError, match="one row per onset"):
            fit(make(0.0), src, torch.zeros(6, 2), seed=1)
        with pytest.raises(ValueError, match="needs seed="):
            fit(make(0.0), src, torch.zeros(3, 2))
        with pytest.raises(ValueError, match="epoch"):
            grads(make(0.5), x, y, seed=1, epoch=-1)
    with pytest.raises(ValueError, match="1024"):  # the batch limit counts the extractions
        big = data.ShiftedWindows(np.zeros((40000, 3), np.float32), 40 + 60 * np.arange(600), 32, n_extractions=2)
        model.fit_cnn(model.CNN(32, 2, dropout_rate=0.0), big, torch.zeros(600, 2))
    with pytest.raises(ValueError, match="seed"):
        model.dropout_mask_device(-1, 0, 4, 4, 0.5)
    with pytest.raises(ValueError, match="0 <= p < 1"):
        model.dropout_mask_device(1, 0, 4, 4, 1.0)
    with pytest.raises(IndexError):
        data.ShiftedWindows(audio, onsets, 32, pre_samples=48, max_shift=3)
    with pytest.raises(IndexError):
        data.ShiftedWindows(audio, np.array([390]), 32)
    with pytest.raises(ValueError):
        data.ShiftedWindows(audio, onsets, 32, n_extractions=0)
