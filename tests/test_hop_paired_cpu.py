"""CPU-only checks of the voting locator inside the hop (realtime.HopSession(locator=MultilateratePaired(...))):
argument errors are raised before any GPU call, the restatement the GPU tests compare against is find_onset_groups plus
the oracle's windows_ref, and the synthetic streams of tests/test_gpu_hop_paired.py give those tests something to
check: every vote branch, sums that do not depend on their order, nothing left out."""
import numpy as np
import pytest
import torch

import oracle
from oracle import locate_kernels as K
from tests.test_gpu_hop_paired import B, CASES, NO_GROUP, SESSION, first_of, restate, tables, window_rows
from tests.test_gpu_hop_regress import SESSION_RING_ROWS, online_hits
from tests.test_hop_regress_cpu import no_gpu_calls, random_stream  # noqa: F401 (a fixture)


def host_locator(S=3, side=9):
    """A MultilateratePaired with nothing but the host attributes the checks read."""
    from onset_fingerprinting_amd import multilateration as ml
    m = object.__new__(ml.MultilateratePaired)
    m.sensor_locs = [(0.0, 0.0)] * S
    m.side, m.radius, m.device = side, 4, torch.device("cuda", 0)
    return m


def hop_session(*a, **kw):
    from onset_fingerprinting_amd import realtime
    return realtime.HopSession(*a, sr=96000, n_fft=256, **kw)


# ---- argument errors ------------------------------------------------------------------------------------------------

def test_the_check_that_it_is_missing_has_gone(no_gpu_calls):
    with pytest.raises(AssertionError, match="GPU call"):  # every check passes: straight to the library
        hop_session(3, 128, locator=host_locator())


@pytest.mark.parametrize("kw,match", [
    (dict(n=4), "sensors"),
    (dict(device=1), "device 1"),
    (dict(tol=-0.5), "tol"),
    (dict(left=-1), "left"),
    (dict(right=0), "right"),
    (dict(left=1, right=1024), "window cap"),
    (dict(backtrack=True), "backtrack"),
    (dict(max_distance=127), "max_distance"),
    (dict(min_channels=0), "min_channels"),
    (dict(min_channels=4), "min_channels"),
    (dict(right=1024, max_distance=128), "pending"),
    (dict(regressor=object()), "regressor"),
])
def test_argument_errors_come_before_any_gpu_call(kw, match, no_gpu_calls):
    kw = dict(kw)
    n = kw.pop("n", 3)
    with pytest.raises(ValueError, match=match):
        hop_session(n, 128, locator=host_locator(), **kw)


def test_nine_sensors_are_outside_the_grouping_state(no_gpu_calls):
    with pytest.raises(ValueError, match="sensors"):
        hop_session(9, 128, locator=host_locator(S=9))


def test_window_cap_and_envelope_to_the_sample(no_gpu_calls):
    from onset_fingerprinting_amd import _lib
    with pytest.raises(AssertionError, match="GPU call"):  # the cap itself is inside
        hop_session(3, 128, locator=host_locator(), left=0, right=1024)
    # side 857: a bitmap of 22 952 words; 32 + 12 w + 91 808 <= 98 304 holds up to w = 538
    assert _lib.paired_lds_bytes(538, 857) <= _lib.PAIR_LDS_ENVELOPE < _lib.paired_lds_bytes(539, 857)
    with pytest.raises(ValueError, match="LDS"):
        hop_session(3, 128, locator=host_locator(side=857), left=0, right=539)
    with pytest.raises(AssertionError, match="GPU call"):  # one sample of window less
        hop_session(3, 128, locator=host_locator(side=857), left=0, right=538)
    assert _lib.paired_lds_bytes(256, 357) == 32 + 3072 + 15932  # the default locator: about 19 KiB


def test_ring_must_hold_a_pending_window_and_a_hop(no_gpu_calls):
    from onset_fingerprinting_amd import realtime
    need = realtime.regress_ring_rows(128, SESSION["left"] + SESSION["right"], SESSION["left"], SESSION["max_distance"])
    assert need == SESSION_RING_ROWS
    with pytest.raises(ValueError, match="ring"):
        hop_session(3, 128, locator=host_locator(), ring_seconds=(need - 1) / 96000, **SESSION)
    with pytest.raises(AssertionError, match="GPU call"):  # one row more passes every check
        hop_session(3, 128, locator=host_locator(), ring_seconds=need / 96000, **SESSION)


def test_replay_checks_its_arguments_first(no_gpu_calls):
    m = host_locator()
    audio = np.zeros((1024, 3), np.float32)
    with pytest.raises(ValueError, match="sensors"):
        m.locate_cc_stream_device(audio[:, :2], [0], [10], 128)
    with pytest.raises(ValueError, match="window cap"):
        m.locate_cc_stream_device(audio, [0], [10], 128, right=1025)
    with pytest.raises(ValueError, match="onsets"):
        m.locate_cc_stream_device(audio, [0, 1], [10], 128)


def test_a_mixed_group_is_refused(no_gpu_calls):
    from onset_fingerprinting_amd import realtime

    def member(paired):
        s = object.__new__(realtime.HopSession)
        s.handle, s._group, s._paired = 1, None, paired
        s.close = lambda: None
        return s

    with pytest.raises(ValueError, match="voting locator"):
        realtime.HopSessionGroup([member(True), member(False)])
    with pytest.raises(AssertionError, match="GPU call"):  # all or none
        realtime.HopSessionGroup([member(True), member(True)])


# ---- the restatement ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", range(8))
def test_restatement_is_find_onset_groups_and_windows_ref(seed):
    """online_hits with F = left + right, pre = left, then first / onset from the row: the groups are the offline
    function's, and first, onset and the status of a window below 0 are ofp_paired_windows' on the same rows."""
    rng = np.random.default_rng(seed)
    C, n_hops = int(rng.choice([3, 4])), 400
    left, right = int(rng.integers(0, 200)), int(rng.integers(1, 400))
    D, minc = int(rng.integers(B, 8 * B)), int(rng.integers(1, C + 1))
    ch, on = random_stream(rng, n_hops, B, C, rate=int(rng.integers(D // 2 + 2, 3 * D + 3)))
    hits, _, groups = online_hits(ch, on, n_hops, B, C, left + right, left, D, minc)
    order = np.argsort(on, kind="stable")
    want = oracle.find_onset_groups(on[order], ch[order], D, minc, width=C)
    want = [] if want is None else list(want)
    assert len(groups) in (len(want), len(want) - 1) and len(groups) >= 5
    assert all(np.array_equal(a, b) for a, b in zip(groups, want))
    rows = np.stack(groups)[None]
    N = n_hops * B
    a_off, b_off, ln, first, status = K.windows_ref(1, N, C, C, left, right, groups=rows)
    evaluated = [h for h in hits if h is not None]
    assert len(evaluated) >= 5 and any(s < 0 for s, _ in evaluated) == any(status == K.PAIRED_NEG_WINDOW)
    for k, (start, row) in enumerate(evaluated):
        assert np.array_equal(row, groups[k])
        f, onset = first_of(row)
        assert f == first[k] and start == onset - left
        assert (status[k] == K.PAIRED_NEG_WINDOW) == (start < 0)
        if start >= 0:  # the window is complete when it is evaluated: the same rows, never clipped
            assert status[k] == K.PAIRED_OK and ln[k, 0] == left + right
            assert a_off[k, 0] == start * C + f
            assert list(b_off[k]) == [start * C + (f - 1) % C, start * C + (f + 1) % C]


# ---- the GPU cases have something to check --------------------------------------------------------------------------

@pytest.fixture(scope="module")
def restated():
    return {name: (make(), ) for name, make in CASES.items()}


def test_cases_reach_every_vote_branch_with_exact_sums(restated):
    kinds, firsts, neg, left_out = set(), set(), 0, 0
    for name, (case, ) in restated.items():
        p, slots = tables(case["model"])
        want, _ = restate(case)
        hits = [e for e in want if e is not None]
        assert bool(hits) == (name not in NO_GROUP), name
        samples = case["audio"][np.isfinite(case["audio"])] * 256
        assert np.array_equal(samples, np.rint(samples)) and np.abs(samples).max(initial=0) <= 227, name
        for e in hits:
            if e["status"] != K.PAIRED_OK:
                neg += 1
                continue
            a, b0, b1 = window_rows(case["audio"], p.S, e["first"], e["onset"], case["left"], case["right"])
            if not (K.order_independent(a, b0) and K.order_independent(a, b1)):
                left_out += 1
            kinds.add(K.vote_kind(slots, p.S, e["first"], e["lags"], case["tol"]))
            firsts.add((p.S, e["first"]))
    assert kinds == {"overlap", "disjoint", "one_empty", "both_empty", "single"}
    assert left_out == 0  # a condition, not a tolerance
    assert neg >= 1
    assert {(3, 0), (3, 2), (4, 0), (4, 3), (2, 0), (2, 1)} <= firsts  # the neighbour wrap on both sides


def test_cases_named_for_an_edge_show_it(restated):
    def lags(name):
        return [e["lags"] for e in restate(restated[name][0])[0] if e is not None and e["lags"] is not None]

    assert all(list(l) == [-255, -255] for l in lags("flat_zero"))       # every lag ties: the first maximum
    assert all(list(l) == [0, 0] for l in lags("flat_constant"))
    assert lags("length_1")[0].tolist() == [0, 0]
    nan = restated["nan_sample"][0]
    assert np.isnan(nan["audio"]).sum() == 4
    p, _ = tables("default")
    assert p.side == 357 and (p.side * p.side) % 32 != 0  # the last bitmap word is partial
    for name in ("length_255", "length_256", "length_257", "length_1024"):
        assert len(lags(name)) >= 3, name
    # the impulses put the correlation's peak where the pick wants it
    case = restated["vote_p3_tol2"][0]
    assert len({tuple(l) for l in lags("vote_p3_tol2")}) >= 5
