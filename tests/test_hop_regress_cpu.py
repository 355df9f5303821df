"""CPU-only checks of the window regressor inside the hop (realtime.HopSession(regressor=...)): argument errors are
raised before any GPU call, the numpy restatement the GPU tests compare against is find_onset_groups made online, the
constructor's bounds hold on random streams, and the committed fixture g25 gives the GPU tests something to check."""
import numpy as np
import pytest

import oracle
from tests.conftest import load_golden
from tests.test_gpu_hop_regress import B, D, EDGES, F, PRE, SESSION, SESSION_CASE, SESSION_RING_ROWS, online_hits


@pytest.fixture
def no_gpu_calls(monkeypatch):
    """Any use of the library or of torch's device fails the test."""
    import torch

    from onset_fingerprinting_amd import _lib

    def refuse(*a, **k):
        raise AssertionError("a GPU call was made before the arguments were checked")

    monkeypatch.setattr(_lib, "lib", refuse)
    monkeypatch.setattr(_lib, "require_gpu", refuse)
    monkeypatch.setattr(torch.cuda, "device", refuse)


def cnn(*a, **kw):
    from onset_fingerprinting_amd import model
    return model.CNN(*a, **kw)


def hop_session(*a, **kw):
    from onset_fingerprinting_amd import realtime
    return realtime.HopSession(*a, sr=96000, n_fft=256, **kw)


def test_backtrack_is_refused(no_gpu_calls):
    with pytest.raises(ValueError, match="backtrack"):
        hop_session(3, 128, regressor=cnn(256, 2, 3), backtrack=True)


def test_max_distance_must_cover_a_hop(no_gpu_calls):
    with pytest.raises(ValueError, match="max_distance"):
        hop_session(3, 128, regressor=cnn(256, 2, 3), max_distance=127)


def test_channels_and_frame_length_must_be_the_models(no_gpu_calls):
    with pytest.raises(ValueError, match="channels"):
        hop_session(4, 128, regressor=cnn(256, 2, 3))
    with pytest.raises(ValueError, match="frame_length"):
        hop_session(3, 128, regressor=cnn(256, 2, 3), frame_length=128)


@pytest.mark.parametrize("min_channels", [0, 4])
def test_min_channels_must_lie_in_1_to_n_signals(min_channels, no_gpu_calls):
    with pytest.raises(ValueError, match="min_channels"):
        hop_session(3, 128, regressor=cnn(256, 2, 3), min_channels=min_channels)


def test_ring_must_hold_a_pending_window_and_a_hop(no_gpu_calls):
    from onset_fingerprinting_amd import realtime
    need = realtime.regress_ring_rows(128, 256, 32, 1000)
    assert need == 1000 + 32 + 10 * 128  # K = ceil(1224 / 128) - 1 = 9 hops of waiting, and the hop being written
    with pytest.raises(ValueError, match="ring"):
        hop_session(3, 128, regressor=cnn(256, 2, 3), pre_samples=32, ring_seconds=(need - 1) / 96000)
    with pytest.raises(AssertionError, match="GPU call"):  # one row more passes every check
        hop_session(3, 128, regressor=cnn(256, 2, 3), pre_samples=32, ring_seconds=need / 96000)


def test_more_pending_groups_than_the_queue_holds(no_gpu_calls):
    from onset_fingerprinting_amd import _lib, realtime
    # 4096-sample windows of groups 129 samples apart: a group waits 32 hops while one more closes every other hop
    assert realtime.regress_pending_bound(128, 4096, 0, 128) > _lib.REG_QUEUE
    with pytest.raises(ValueError, match="pending"):
        hop_session(3, 128, regressor=cnn(4096, 2, 3, layer_sizes=[1]), max_distance=128)
    assert realtime.regress_pending_bound(128, 256, 0, 1000) <= 3


def test_models_outside_the_envelope(no_gpu_calls):
    from onset_fingerprinting_amd import model
    with pytest.raises(ValueError, match="RNN"):
        hop_session(3, 128, regressor=model.RNN(256, 2, 3))
    with pytest.raises(ValueError, match="CNNRNN"):
        hop_session(3, 128, regressor=model.CNNRNN(256, 2, 3))
    with pytest.raises(ValueError, match="CNN, CCCNN or LCCCNN"):
        import torch
        hop_session(3, 128, regressor=torch.nn.Linear(2, 2))
    with pytest.raises(ValueError, match="outputs"):
        hop_session(3, 128, regressor=cnn(256, 65, 3))
    with pytest.raises(ValueError, match="channels"):
        hop_session(9, 128, regressor=cnn(256, 2, 9))
    with pytest.raises(ValueError, match="input_size"):
        hop_session(3, 128, regressor=cnn(4097, 2, 3, layer_sizes=[1]))
    with pytest.raises(ValueError, match="conv layers"):
        hop_session(3, 128, regressor=cnn(64, 2, 3, layer_sizes=[1] * 9))


def test_without_a_regressor_the_checks_do_not_run(no_gpu_calls):
    with pytest.raises(AssertionError, match="GPU call"):  # straight to the library, as before
        hop_session(3, 128, backtrack=True, max_distance=1)


def test_replay_checks_its_arguments_first(no_gpu_calls):
    from onset_fingerprinting_amd import realtime
    audio = np.zeros((1024, 3), np.float32)
    with pytest.raises(ValueError, match="channels"):
        realtime.regress_stream_device(cnn(256, 2, 2), audio, [0], [10], 128)
    with pytest.raises(ValueError, match="min_channels"):
        realtime.regress_stream_device(cnn(256, 2, 3), audio, [0], [10], 128, min_channels=4)
    with pytest.raises(ValueError, match="onsets"):
        realtime.regress_stream_device(cnn(256, 2, 3), audio, [0, 1], [10], 128)


def test_flags_are_never_silent():
    from onset_fingerprinting_amd import _lib, realtime
    realtime.check_regress_flags(0, "test")
    with pytest.raises(_lib.OnsetFPError, match="overflow"):
        realtime.check_regress_flags(_lib.REGF_QUEUE, "test")
    with pytest.raises(_lib.OnsetFPError, match="refused"):
        realtime.check_regress_flags(_lib.REGF_BAD_ONSET, "test")


# ---- the restatement ----------------------------------------------------------------------------------------------

def random_stream(rng, n_hops, Bk, C, rate):
    """Bursts of onsets (hits) and stray single onsets, unsorted within a hop as the detector's records can be."""
    N = n_hops * Bk
    onsets, channels = [], []
    t = int(rng.integers(0, 400))
    while t < N:
        if rng.random() < 0.8:
            for c in rng.permutation(C)[: int(rng.integers(1, C + 1))]:
                s = t + int(rng.integers(0, 120))
                if s < N:
                    onsets.append(s), channels.append(int(c))
            if rng.random() < 0.3:  # a channel fires again
                s = t + int(rng.integers(60, 200))
                if s < N:
                    onsets.append(s), channels.append(int(rng.integers(0, C)))
        else:
            onsets.append(t), channels.append(int(rng.integers(0, C)))
        t += int(rng.integers(1, rate))
    order = np.argsort(np.asarray(onsets) // Bk, kind="stable")  # hop by hop, any order within a hop
    return np.asarray(channels)[order], np.asarray(onsets)[order]


@pytest.mark.parametrize("seed", range(12))
def test_restatement_on_random_streams(seed):
    from onset_fingerprinting_amd import _lib, realtime
    rng = np.random.default_rng(seed)
    for _ in range(200):  # a parameter set the constructor admits
        Bk = int(rng.choice([32, 64, 128, 256]))
        Fk = int(rng.choice([16, 64, 256, 1024, 4096]))
        pre = int(rng.integers(0, 2 * Fk))
        Dk = int(rng.integers(Bk, 12 * Bk))
        if realtime.regress_pending_bound(Bk, Fk, pre, Dk) <= _lib.REG_QUEUE:
            break
    else:
        pytest.fail("no admissible parameter set drawn")
    C, minc, n_hops = 4, int(rng.integers(1, 5)), 600
    ch, on = random_stream(rng, n_hops, Bk, C, rate=int(rng.integers(Dk // 2 + 2, 3 * Dk + 3)))
    hits, pending, groups = online_hits(ch, on, n_hops, Bk, C, Fk, pre, Dk, minc)
    # the groups are the offline function's on the whole list, in feed order
    order = np.argsort(on, kind="stable")
    closed = [s for s in on if s + Dk < n_hops * Bk]  # (the offline function also closes the stream's last group)
    want = oracle.find_onset_groups(on[order], ch[order], Dk, minc, width=C)
    want = [] if want is None else list(want)
    assert len(groups) in (len(want), len(want) - 1) and len(closed) > 0
    assert all(np.array_equal(a, b) for a, b in zip(groups, want))
    # every kept group whose window the stream completes is evaluated exactly once, in order, at the first hop
    # that holds its last row and lies after the evaluation before it
    evaluated = [h for h in hits if h is not None]
    assert all(np.array_equal(e[1], g) for e, g in zip(evaluated, groups))
    assert len(evaluated) >= len([g for g in groups if g[g >= 0].min() - pre + Fk <= (n_hops - realtime.regress_hold_hops(Bk, Fk, pre, Dk) - 1) * Bk])
    starts = [e[0] for e in evaluated]
    assert starts == sorted(set(starts))  # strictly increasing: the head is always the earliest due
    last = -1
    for h, e in enumerate(hits):
        if e is not None:
            assert (h + 1) * Bk >= e[0] + Fk and h > last
            last = h
    # the bounds the constructor relies on
    assert max(pending) <= realtime.regress_pending_bound(Bk, Fk, pre, Dk) <= _lib.REG_QUEUE
    K = realtime.regress_hold_hops(Bk, Fk, pre, Dk)
    rows = realtime.regress_ring_rows(Bk, Fk, pre, Dk)
    for h, e in enumerate(hits):
        if e is not None:
            assert (h + 1) * Bk - e[0] <= rows, (h, e, K)


def test_edge_cases_show_what_they_are_named_for():
    for name, (onsets, minc, shows) in EDGES.items():
        hits, pend, _ = online_hits([c for c, _ in onsets], [s for _, s in onsets], 20, B, 3, F, PRE, D, minc)
        assert shows is None or shows(hits, pend), name
    # the window that ends with hop 10 is evaluated no later than the one that ends a sample after it
    a = online_hits(*zip(*EDGES["window_ends_with_the_hop"][0]), 20, B, 3, F, PRE, D, 3)[0]
    b = online_hits(*zip(*EDGES["window_ends_one_sample_later"][0]), 20, B, 3, F, PRE, D, 3)[0]
    assert [h is not None for h in a].index(True) <= [h is not None for h in b].index(True)


def test_fixture_gives_the_session_tests_hits_and_a_wrapped_window():
    from onset_fingerprinting_amd import realtime
    g = load_golden("g25_hoplocate")
    audio = g[f"{SESSION_CASE}/audio"]
    ch, on = [], []
    for k in range(len(g[f"{SESSION_CASE}/hops"])):
        n = int(g[f"{SESSION_CASE}/n_onsets"][k])
        ch += [int(c) for c in g[f"{SESSION_CASE}/channels"][k, :n]]
        on += [int(s) for s in g[f"{SESSION_CASE}/onsets"][k, :n]]
    p = SESSION
    hits, pending, _ = online_hits(ch, on, len(audio) // 128, 128, 3, p["frame_length"], p["pre_samples"],
                                   p["max_distance"], p["min_channels"])
    starts = [h[0] for h in hits if h is not None]
    assert len(starts) >= 10
    assert SESSION_RING_ROWS == realtime.regress_ring_rows(128, p["frame_length"], p["pre_samples"], p["max_distance"])
    assert any(s % SESSION_RING_ROWS + p["frame_length"] > SESSION_RING_ROWS for s in starts)
    assert sum(h is not None for h in hits[:450]) >= 3 and sum(h is not None for h in hits[:300]) >= 1
