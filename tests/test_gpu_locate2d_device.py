"""GPU parity of the planar locator's device forms (csrc/ofp_locate_dev.h: the planar instantiation of loc_feed): the
replay entry ``Multilaterate.locate_stream_device`` against the reference's trace (golden g23, m2d/m3 and m2d/m4air),
the host state machine call for call and a stream with negative lags, ``locate_groups_device`` with a
``Multilaterate`` against a per-row replay of the host functions, and ``realtime.HopSession(locator=Multilaterate)``
-- both graph forms, and in a group next to a 3-D member -- against detect_hits replayed on the host.

Tolerances: ROOT_TOL for roots and polar tuples against the golden or a separately launched solve, bit equality where
both sides run the same device arithmetic, integers exact."""
import numpy as np
import pytest
import torch

from tests import locate2d_cases as lc

pytestmark = pytest.mark.gpu

ROOT_TOL = 1e-6


def m2d(name):
    from onset_fingerprinting_amd import multilateration as ml
    return ml.Multilaterate(**lc.layout_args(name))


def plain(ongoing):
    return [(list(s), list(o)) for s, o in ongoing]


def shared(ongoing):
    """Where an entry is the same object as the one before it."""
    return [k for k in range(1, len(ongoing)) if ongoing[k] is ongoing[k - 1]]


# ---- 1: the stream against the golden trace -------------------------------------------------------------------

@pytest.mark.parametrize("name", lc.LAYOUTS)
def test_stream_matches_the_reference_trace_call_for_call(name):
    m = m2d(name)
    sens, ons, want = lc.trace(name)
    found, rphi, _ = m.locate_stream_device(sens, ons)
    assert m.ongoing == []  # untouched
    assert found.dtype == bool and rphi.dtype == np.float64 and rphi.shape == (len(sens), 2)
    assert np.array_equal(found, want[:, 0] == 1), np.flatnonzero(found != (want[:, 0] == 1))[:10]
    assert found.sum() >= 20
    assert np.abs(rphi[found] - want[found, 1:]).max() < ROOT_TOL
    assert np.isnan(rphi[~found]).all()


# ---- 2: the state call for call ---------------------------------------------------------------------------------

@pytest.mark.parametrize("name", lc.LAYOUTS)
def test_state_equals_the_host_state_machine_at_every_prefix(name):
    m = m2d(name)
    sens, ons, want = lc.trace(name)
    K = len(sens)
    first = int(np.flatnonzero(want[:, 0])[0])
    host = {}
    for k, (s, o) in enumerate(zip(sens, ons)):  # one fresh object; its state after K' calls is the K'-prefix's
        r = m.locate(int(s), int(o))
        assert (r is not None) == bool(want[k, 0]), k
        host[k + 1] = (plain(m.ongoing), shared(m.ongoing))
    # the first calls, the call after the first located one, mid-stream, all calls
    prefixes = {1, 2, 3, first + 2, K // 2, K}
    if name == "m4air":  # and a state that carries a group beyond three members
        prefixes.add(min(kp for kp, (groups, _) in host.items() if any(len(g[0]) >= 4 for g in groups)))
    prefixes = sorted(prefixes)
    aliased = 0
    for kp in prefixes:
        found, _, ongoing = m.locate_stream_device(sens[:kp], ons[:kp])
        assert np.array_equal(found, want[:kp, 0] == 1), kp
        assert plain(ongoing) == host[kp][0], kp  # duplicates included
        assert shared(ongoing) == host[kp][1], kp
        aliased += len(shared(ongoing))
    assert aliased >= 1


def test_a_negative_lag_is_taken_as_it_is_never_swapped():
    """Each row's two earliest arrivals exchanged (lc.swapped_stream): the planar routine tests the negative lag with
    is_legal and extends the group in the order fed, where the 3-D routine would swap the two onsets first.  Expected
    values: the host ``Multilaterate.locate``, call for call on a fresh object."""
    sens, ons = lc.swapped_stream("m3")
    m_dev, m = m2d("m3"), m2d("m3")
    want = [m.locate(int(s), int(o)) for s, o in zip(sens, ons)]
    hit = np.array([w is not None for w in want])
    found, rphi, ongoing = m_dev.locate_stream_device(sens, ons)
    assert np.array_equal(found, hit), np.flatnonzero(found != hit)[:10]
    assert found.sum() >= 1
    assert plain(ongoing) == plain(m.ongoing)  # duplicates included
    assert shared(ongoing) == shared(m.ongoing)
    assert np.abs(rphi[found] - np.array([w for w in want if w is not None], np.float64)).max() < ROOT_TOL
    assert np.isnan(rphi[~found]).all()


# ---- 3: batched rows ----------------------------------------------------------------------------------------

def replay_row(ml, m, row, used):
    """One row through the host functions, in the order locate applies them: (status is 1, a code or 'no root',
    guess, root or None, (sensors, onsets))."""
    nan2 = (np.nan, np.nan)
    if not used:
        return ml.LOCATE_UNUSED, nan2, None, None
    order = sorted((int(v), k) for k, v in enumerate(row) if v >= 0)[:3]
    if len(order) < 3:
        return ml.LOCATE_FEW_CHANNELS, nan2, None, None
    sens, ons = [k for _, k in order], [v for v, _ in order]
    if not (m.is_legal(sens[0], sens[1], ons[1] - ons[0]) and m.is_legal(sens[0], sens[2], ons[2] - ons[0])):
        return ml.LOCATE_ILLEGAL_LAG, nan2, None, (sens, ons)
    cell = m.is_legal_3d((sens, ons))
    if cell == (0, 0):
        return ml.LOCATE_NO_CELL, nan2, None, (sens, ons)
    guess = np.array(cell) - m.radius
    c = ml.speed_of_sound(100, medium=m.medium)
    root = ml.solve_trilateration(m.sensor_locs[sens[1]], m.sensor_locs[sens[2]], m.sensor_locs[sens[0]],
                                  (ons[1] - ons[0]) * c / m.sr, (ons[2] - ons[0]) * c / m.sr, guess, device=m.device)
    return (1 if root is not None else "no root"), tuple(guess), root, (sens, ons)


@pytest.mark.parametrize("name", lc.LAYOUTS)
def test_batched_rows_equal_the_row_replay(name):
    from onset_fingerprinting_amd import multilateration as ml
    m = m2d(name)
    groups, n_groups = lc.group_rows(name)
    gd, nd = torch.from_numpy(np.array(groups)).to(m.device), torch.from_numpy(n_groups).to(m.device)
    xy, status, guess = (t.cpu().numpy() for t in ml.locate_groups_device(gd, nd, m, return_guess=True))
    assert xy.shape == (2, lc.CAP, 2) and status.shape == (2, lc.CAP) and status.dtype == np.int32
    seen, unreordered = set(), 0
    c = ml.speed_of_sound(100, medium=m.medium)
    for clip in range(2):
        for r in range(lc.CAP):
            want, wguess, root, group = replay_row(ml, m, groups[clip, r], r < n_groups[clip])
            ctx = (clip, r, groups[clip, r])
            if want == "no root":
                assert status[clip, r] > 1, ctx  # fsolve's other ier values: the reference drops them
            else:
                assert status[clip, r] == want, ctx
            seen.add(int(status[clip, r]))
            assert np.array_equal(guess[clip, r], wguess, equal_nan=True), ctx
            if root is None:
                assert want == "no root" or np.isnan(xy[clip, r]).all(), ctx
                continue
            assert np.abs(xy[clip, r] - np.array(root, np.float64)).max() < ROOT_TOL, ctx
            sens, ons = group
            if sens[1] == 1 and sens[2] != 0:
                # Multilaterate3D.trilaterate would solve for (origin, 0, 1) with the two later onsets exchanged: another
                # geometry.  The planar class keeps (origin, 1, b), which is what the replay above solved.
                other = ml.solve_trilateration(m.sensor_locs[0], m.sensor_locs[1], m.sensor_locs[sens[0]],
                                               (ons[2] - ons[0]) * c / m.sr, (ons[1] - ons[0]) * c / m.sr,
                                               np.array(wguess), device=m.device)
                assert other is None or np.abs(xy[clip, r] - np.array(other, np.float64)).max() > 1e-3, ctx
                unreordered += 1
    assert {1, ml.LOCATE_UNUSED, ml.LOCATE_FEW_CHANNELS, ml.LOCATE_ILLEGAL_LAG, ml.LOCATE_NO_CELL} <= seen, seen
    assert unreordered >= 1
    # the polar form of a located row is the reference's tuple
    clip, r = np.argwhere(status == 1)[0]
    rphi = ml.cartesian_to_polar(*xy[clip, r], m.radius)
    assert 0 <= rphi[0] < 1.2 and 0 <= rphi[1] < 360
    # n_groups = None: every row is used
    _, status_all = ml.locate_groups_device(gd, None, m)
    assert (status_all.cpu().numpy() != ml.LOCATE_UNUSED).all()


# ---- 4: one row alone against a batch ---------------------------------------------------------------------------

@pytest.mark.parametrize("name", lc.LAYOUTS)
def test_a_row_gives_the_same_bits_alone_and_inside_a_batch(name):
    from onset_fingerprinting_amd import multilateration as ml
    m = m2d(name)
    groups, _ = lc.group_rows(name)
    S = groups.shape[2]
    flat = groups.reshape(-1, S)
    N, at = 4099, 2050  # not a multiple of the solve kernel's 64 lanes
    big = np.ascontiguousarray(flat[np.arange(N) % len(flat)])[None]
    located = 0
    for k in (8, 9, 5):  # two hits of the trace and the row without a common cell
        big[0, at] = flat[k]
        one = np.array(flat[k])[None, None]
        a = ml.locate_groups_device(torch.from_numpy(one).to(m.device), None, m, return_guess=True)
        b = ml.locate_groups_device(torch.from_numpy(big).to(m.device), None, m, return_guess=True)
        for x, y in zip(a, b):
            x, y = x.cpu().numpy()[0, 0], y.cpu().numpy()[0, at]
            assert x.tobytes() == y.tobytes(), (k, x, y)
        located += int(a[1].cpu()[0, 0]) == 1
    assert located >= 1 and int(a[1].cpu()[0, 0]) == ml.LOCATE_NO_CELL


# ---- 5: the hop graph -------------------------------------------------------------------------------------------

def hop_session(m, locator=True):
    from onset_fingerprinting_amd import realtime
    return realtime.HopSession(len(m.sensor_locs), lc.HOP, sr=lc.SR, n_fft=2048, ring_seconds=0.5,
                               locator=m if locator else None, **lc.DETECTOR)


def host_driven(m, q):
    """detect_hits on the host: a hop's onsets, sorted, through Multilaterate.locate until one returns."""
    seen = []
    solve = m.trilaterate
    m.trilaterate = lambda group, guess: (seen.append(group), solve(group, guess))[1]
    res, fed = None, 0
    try:
        for i in np.argsort(q["onsets"], kind="stable"):
            fed += 1
            res = m.locate(int(q["channels"][i]), int(q["onsets"][i]))
            if res is not None:
                break
    finally:
        del m.trilaterate
    group = (list(seen[-1][0]), list(seen[-1][1])) if res is not None else None
    return res, group, fed, len(q["onsets"]) - fed


@pytest.mark.parametrize("form", ["fused", "nodes"])
def test_session_matches_the_host_driven_path(form, monkeypatch):
    monkeypatch.setenv("OFP_HOP_GRAPH", form)
    plan = lc.hop_plan("m3")  # the CPU's view of the stream: the oracle's detector and the numpy model
    assert sum(res == "located" for _, res in plan) >= 5 and sum(res is None for _, res in plan) >= 1
    audio = lc.head_stream("m3")
    m_dev, m = m2d("m3"), m2d("m3")
    a, b = hop_session(m_dev), hop_session(m, locator=False)
    located = idle = 0
    onset_hops = []
    for h in range(len(audio) // lc.HOP):
        hop = audio[h * lc.HOP:(h + 1) * lc.HOP]
        r, q = a(hop), b(hop)
        assert np.array_equal(r["onsets"], q["onsets"]) and np.array_equal(r["channels"], q["channels"]), h
        if len(q["onsets"]) == 0:
            assert r["location"] is None and r["located_group"] is None and (r["fed"], r["dropped"]) == (0, 0), h
            continue
        onset_hops.append(h)
        res, group, fed, dropped = host_driven(m, q)
        assert (r["location"] is not None) == (res is not None), h
        if res is not None:
            assert np.abs(np.array(r["location"], np.float64) - np.array(res, np.float64)).max() < ROOT_TOL, h
            located += 1
        else:
            idle += 1
        assert r["located_group"] == group, h
        assert (r["fed"], r["dropped"]) == (fed, dropped), h
        assert plain(a.ongoing) == plain(m.ongoing), h
    assert located >= 5 and idle >= 1
    assert onset_hops == [h for h, _ in plan]  # the hops the oracle's detector found onsets in
    assert plain(a.ongoing) == plain(m.ongoing)
    assert m_dev.ongoing == []  # the locator's own state is not touched
    a.reset()
    assert a.ongoing == []
    a.close()
    b.close()


def test_a_group_of_a_planar_and_a_3d_member_equals_the_members_alone():
    from onset_fingerprinting_amd import realtime
    from tests.test_gpu_hop_group import assert_same
    from tests.test_gpu_hop_locate import session
    audio2 = lc.head_stream("m3")
    m = m2d("m3")
    member3, _, audio3, B = session("rt3_fast3")
    twin3, _, _, _ = session("rt3_fast3")
    assert B == lc.HOP
    member2, twin2 = hop_session(m), hop_session(m)
    group = realtime.HopSessionGroup([member2, member3])
    n = min(len(audio2), len(audio3)) // B
    located = [0, 0]
    for h in range(n):
        hops = [audio2[h * B:(h + 1) * B], audio3[h * B:(h + 1) * B]]
        got = group(hops)
        for s, twin in enumerate((twin2, twin3)):
            assert_same(got[s], twin(hops[s]), (s, h))
            located[s] += got[s]["location"] is not None
    assert located[0] >= 5 and located[1] >= 5
    assert plain(member2.ongoing) == plain(twin2.ongoing) and plain(member3.ongoing) == plain(twin3.ongoing)
    group.close()
    for t in (member2, member3, twin2, twin3):
        t.close()


# ---- 6: refusals, with the device usable afterwards ---------------------------------------------------------

def test_refusals_are_reported_and_leave_the_device_usable():
    from onset_fingerprinting_amd import _lib
    m = m2d("m3")
    sens, ons, want = lc.trace("m3")

    def still_works():
        found, rphi, _ = m.locate_stream_device(sens, ons)
        assert np.array_equal(found, want[:, 0] == 1)
        assert np.abs(rphi[found] - want[found, 1:]).max() < ROOT_TOL

    with pytest.raises(_lib.OnsetFPError, match="refused"):  # a sensor the locator does not have
        m.locate_stream_device([0, 3], [5000, 5100])
    still_works()
    with pytest.raises(_lib.OnsetFPError, match="refused"):
        m.locate_stream_device([0, -1], [5000, 5100])
    # 70 onsets of one sensor at one sample: no call extends a group (the sensor is in every one), each keeps all
    # earlier groups (lag 0) and adds a seed, so the 65th call needs a 65th group
    K = 70
    s70, o70 = np.zeros(K, np.int32), np.full(K, 5000, np.int64)
    found, _, ongoing = m.locate_stream_device(s70[:64], o70[:64])
    assert not found.any() and len(ongoing) == 64  # exactly full is not an overflow
    with pytest.raises(_lib.OnsetFPError, match="overflow"):
        m.locate_stream_device(s70, o70)
    still_works()
    found, rphi, ongoing = m.locate_stream_device([], [])  # an empty stream is an empty state
    assert found.shape == (0,) and rphi.shape == (0, 2) and ongoing == []
