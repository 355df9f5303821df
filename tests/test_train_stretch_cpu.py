"""CPU: site 2 of the trainers' random stream as tests/train_stretch_ref.py states it, against an explicit enumeration
of the values the reference's randint(1, S) * choice((-1, 1)) can give, and the construction of data.StretchedWindows,
which touches no GPU."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import train_stretch_ref as S  # noqa: E402

from onset_fingerprinting_amd import data  # noqa: E402


@pytest.mark.parametrize("span", [2, 3, 8])
def test_every_stretch_occurs_and_no_other(span):
    allowed = sorted(set(range(-(span - 1), 0)) | set(range(1, span)))
    got = S.stretches(2 ** 63 + 5, 3, 4096, span)
    assert got.dtype == np.int32 and got.shape == (4096,)
    values, counts = np.unique(got, return_counts=True)
    print(f"span {span}: values {values.tolist()} counts {counts.tolist()}")
    assert values.tolist() == allowed
    assert 0 not in values and span not in values and -span not in values


@pytest.mark.parametrize("span", [2, 3, 8])
def test_the_ends_of_the_word_range(span):
    got = S.stretch_of_words(np.array([0, 2 ** 32 - 1], np.uint32), span)
    assert got.tolist() == [-(span - 1), span - 1]


@pytest.mark.parametrize("span", [2, 3, 8])
def test_the_rule_by_exhaustion_of_v(span):
    """Every value v = (word * 2 (S - 1)) >> 32 can take, by the smallest word that gives it: v counts through the
    allowed stretches in ascending order."""
    m = 2 * (span - 1)
    firsts = np.array([-((-v * 2 ** 32) // m) for v in range(m)], np.uint64).astype(np.uint32)
    assert ((firsts.astype(np.uint64) * np.uint64(m)) >> np.uint64(32)).tolist() == list(range(m))
    allowed = sorted(set(range(-(span - 1), 0)) | set(range(1, span)))
    assert S.stretch_of_words(firsts, span).tolist() == allowed


def test_stretches_are_site_2_words():
    import train_random_ref as R
    w = R.words(77, 5, S.SITE_STRETCH, 10)
    assert np.array_equal(S.stretches(77, 5, 10, 8), S.stretch_of_words(w, 8))
    assert not np.array_equal(w, R.words(77, 5, R.SITE_SHIFT, 10))
    assert not np.array_equal(S.stretches(77, 5, 64, 8), S.stretches(77, 6, 64, 8))
    # the shifts of a stretching source are those of site 1
    sh, _sd = S.draws(77, 5, 10, 3, 8)
    assert np.array_equal(sh, R.shifts(77, 5, 10, 3))


def test_span_arithmetic():
    audio = np.zeros((4000, 2), np.float32)
    assert int(31 * 0.1) == 3 and int(256 * 0.03) == 7
    assert data.StretchedWindows(audio, [100, 900], 31, max_stretch=0.1).stretch_span == 3
    assert data.StretchedWindows(audio, [100, 900], 256).stretch_span == 7
    off = data.StretchedWindows(audio, [100, 900], 256, max_stretch=0)
    assert off.stretch_span == 0 and isinstance(off, data.ShiftedWindows)
    src = data.StretchedWindows(audio, np.array([[100, 120], [900, 880]]), 31, pre_samples=2, max_stretch=0.1,
                                max_shift=3, n_extractions=4)
    assert (src.n, src.n_onsets, src.channels, src.max_shift) == (8, 2, 2, 3)
    assert src.starts.tolist() == [98, 878]


def test_a_span_of_one_is_refused():
    audio = np.zeros((4000, 2), np.float32)
    with pytest.raises(ValueError, match=r"randint\(1, 1\)"):
        data.StretchedWindows(audio, [100], 31, max_stretch=0.04)  # int(1.24) == 1
    with pytest.raises(ValueError, match=r"randint\(1, 1\)"):
        data.StretchedWindows(audio, [100], 256, max_stretch=0.005)
    with pytest.raises(ValueError):
        data.StretchedWindows(audio, [100], 31, max_stretch=-0.1)


def test_the_longest_window_must_end_inside_the_audio():
    W, span, m, N = 31, 3, 2, 500
    audio = np.zeros((N, 2), np.float32)
    last = N - (m + W + span - 1)  # the start whose longest, furthest shifted window ends at row N
    data.StretchedWindows(audio, [m, last], W, max_stretch=0.1, max_shift=m)
    with pytest.raises(IndexError):
        data.StretchedWindows(audio, [m, last + 1], W, max_stretch=0.1, max_shift=m)
    with pytest.raises(IndexError):
        data.StretchedWindows(audio, [m - 1, last], W, max_stretch=0.1, max_shift=m)
    # without a stretch the limit is ShiftedWindows'
    data.StretchedWindows(audio, [m, N - (m + W)], W, max_stretch=0, max_shift=m)
    with pytest.raises(IndexError):
        data.StretchedWindows(audio, [m, N - (m + W) + 1], W, max_stretch=0, max_shift=m)
