"""realtime.HopSessionGroup on the GPU: S sessions' hops in ONE graph launch (k_hop_fused_group, grid (C + 1 + strength, S)).

The bar is equality, not a tolerance: a member runs the device code a stand-alone session runs, on its own state, and
nothing is summed across members -- every output of a group call is bit for bit what a twin ``HopSession`` with the same
arguments, fed the same hops, returns.  Where a CPU reference exists (the oracle detector, the reference's golden
realtime trace g25) the members are held to it as the stand-alone sessions are.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch  # noqa: F401  (before the package, as in the other GPU test modules: both bring a HIP runtime)

import oracle
from onset_fingerprinting_amd import synth
from tests.test_gpu_hop_locate import g25, golden_ongoing, plain, same_location, session

pytestmark = pytest.mark.gpu

SR = 48000


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_same(r, q, ctx):
    """Two result dicts of HopSession.collect, bit for bit."""
    assert r.keys() == q.keys(), ctx
    for k in r:
        a, b = r[k], q[k]
        if a is None or b is None:
            assert a is None and b is None, (k, ctx)
        elif k in ("rel", "mel", "logits", "strength", "tempogram"):
            assert a.shape == b.shape and np.array_equal(bits(a), bits(b)), (k, ctx)
        elif k in ("channels", "onsets"):
            assert np.array_equal(a, b), (k, ctx)
        elif k == "location":
            assert np.array_equal(np.array(a, np.float64).view(np.uint64), np.array(b, np.float64).view(np.uint64)), ctx
        else:  # located_group, fed, dropped
            assert a == b, (k, ctx)


def hops_of(x, B, i):
    return np.ascontiguousarray(x[i * B:(i + 1) * B])


@functools.lru_cache(maxsize=None)
def stream(seed, period, seconds=0.5, C=2):
    x = synth.drum_hits(C, seconds, SR, seed=seed, period=period)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def quiet_stream(seconds=0.5, C=2):
    x = (1e-3 * np.random.default_rng(5).standard_normal((int(seconds * SR), C))).astype(np.float32)
    x.setflags(write=False)
    return x


def close_all(*things):
    for t in things:
        t.close()


# ---- 1: heterogeneous members against twins and the oracle -------------------------------------------------

def test_group_equals_twins_and_the_oracle_with_heterogeneous_members():
    """Three members that differ in detector arguments, stream and classifier; members 0 and 1 find their onsets in
    different hops and member 2 never does, so one launch holds both sides of the count branch."""
    from onset_fingerprinting_amd import realtime
    from onset_fingerprinting_amd.pipeline import seeded_fcnn
    C, B, F = 2, 64, 256
    rt = dict(realtime.REALTIME_DETECTOR_KWARGS)
    specs = [(dict(), stream(11, 0.05), seeded_fcnn(40, 8, seed=1)),
             (rt, stream(12, 0.07), seeded_fcnn(40, 8, seed=2)),
             (dict(), quiet_stream(), None)]

    def make(kw, clf):
        return realtime.HopSession(C, B, sr=SR, n_fft=F, classifier=clf, want_rel=True, ring_seconds=0.1, **kw)

    members = [make(kw, clf) for kw, _, clf in specs]
    twins = [make(kw, clf) for kw, _, clf in specs]
    odets = [oracle.OracleDetector(C, B, sr=SR, **kw) for kw, _, _ in specs]
    for m, t, o, (_, x, _) in zip(members, twins, odets, specs):
        warm = x[: int(0.1 * SR)]
        m.init_minmax_tracker(warm)   # members join warmed up
        t.init_minmax_tracker(warm)
        o.init_minmax_tracker(warm)
    group = realtime.HopSessionGroup(members)
    assert len(group) == 3 and group.sessions == tuple(members)
    nb = int(0.5 * SR) // B
    assert nb == 375
    n_on = [0, 0, 0]
    onset_hops = [[], [], []]
    for i in range(nb):
        hops = np.stack([hops_of(x, B, i) for _, x, _ in specs])
        got = group(hops) if i % 2 else group([h for h in hops])  # both input forms
        for s in range(3):
            assert_same(got[s], twins[s](hops[s]), (s, i))
            ch, d, rel = odets[s](hops[s])
            assert [int(v) for v in got[s]["channels"]] == [int(v) for v in ch], (s, i)
            assert [int(v) for v in got[s]["onsets"]] == [i * B + int(v) for v in d], (s, i)
            assert np.array_equal(bits(got[s]["rel"]), bits(rel)), (s, i)
            n_on[s] += len(ch)
            if len(ch):
                onset_hops[s].append(i)
    assert n_on[0] >= 8 and n_on[1] >= 8 and n_on[2] == 0, n_on
    assert set(onset_hops[0]) != set(onset_hops[1])
    for m, t in zip(members, twins):
        assert m.current_index == t.current_index == nb * B
        assert np.array_equal(bits(m.audio(m.ring_samples)), bits(t.audio(t.ring_samples)))
    close_all(group, *members, *twins)


# ---- 2: locators against the reference's golden realtime trace -------------------------------------------

@pytest.mark.parametrize("with_audio", [True, False])
def test_grouped_locators_match_the_reference_hop_by_hop(with_audio):
    g = g25()
    mode = "audio" if with_audio else "plain"
    cases = ["rt3_fast3", "rt3_realtime"]
    built = [session(c, with_audio=with_audio) for c in cases]
    from onset_fingerprinting_amd import realtime
    group = realtime.HopSessionGroup([b[0] for b in built])
    audios, B = [b[2] for b in built], built[0][3]
    n_hops = [len(a) // B for a in audios]
    assert n_hops == [750, 1250] and all(b[3] == B for b in built)
    hop_rows = [{int(h): k for k, h in enumerate(g[f"{c}/hops"])} for c in cases]
    zeros = np.zeros((B, 3), np.float32)
    located = [0, 0]
    for h in range(max(n_hops)):
        res = group([a[h * B:(h + 1) * B] if h < n else zeros for a, n in zip(audios, n_hops)])
        for s, case in enumerate(cases):
            if h >= n_hops[s]:
                continue  # member 0 runs on zeros once its recording has ended
            r, k = res[s], hop_rows[s].get(h)
            if k is None:
                assert len(r["onsets"]) == 0 and r["location"] is None and r["fed"] == 0 and r["dropped"] == 0, (s, h)
                continue
            n = int(g[f"{case}/n_onsets"][k])
            assert np.array_equal(r["channels"], g[f"{case}/channels"][k, :n]), (s, h)
            assert np.array_equal(r["onsets"], g[f"{case}/onsets"][k, :n]), (s, h)
            same_location(r["location"], g[f"{case}/{mode}/res"][k], (s, h))
            assert r["fed"] == g[f"{case}/{mode}/fed"][k] and r["dropped"] == g[f"{case}/{mode}/dropped"][k], (s, h)
            assert plain(built[s][0].ongoing) == golden_ongoing(g, case, mode, k), (s, h)
            located[s] += r["location"] is not None
    for s, case in enumerate(cases):
        assert located[s] == int(g[f"{case}/{mode}/res"][:, 0].sum()) >= 10, (case, located)
    close_all(group, *[b[0] for b in built])


# ---- 3: onset strength and tempogram: grid.x = C + 2 -----------------------------------------------------------

def test_grouped_onset_strength_and_tempogram_equal_the_twins():
    from onset_fingerprinting_amd import realtime
    C, B, F = 2, 64, 256
    xs = [stream(11, 0.05), stream(12, 0.07)]

    def make():
        return realtime.HopSession(C, B, sr=SR, n_fft=F, ring_seconds=0.05,
                                   onset_strength=dict(max_length=5, avg_length=7, tg_win_length=16))

    members, twins = [make(), make()], [make(), make()]
    group = realtime.HopSessionGroup(members)
    differ = False
    for i in range(200):
        hops = np.stack([hops_of(x, B, i) for x in xs])
        got = group(hops)
        for s in range(2):
            assert got[s]["strength"].shape == (4,) and got[s]["tempogram"].shape == (16,)
            assert_same(got[s], twins[s](hops[s]), (s, i))
        differ |= not np.array_equal(bits(got[0]["strength"]), bits(got[1]["strength"]))
    assert differ
    close_all(group, *members, *twins)


# ---- 4: more workgroups than the device has compute units ---------------------------------------------------

def test_a_grid_larger_than_the_device_queues_and_every_member_is_exact():
    from onset_fingerprinting_amd import realtime
    S, C, B, F, nb = 96, 2, 32, 256, 40   # 96 x 3 = 288 workgroups, 256 compute units
    periods = (0.004, 0.005, 0.006, 0.007)
    xs = [synth.drum_hits(C, 0.3, SR, seed=20 + k, period=p)[: nb * B] for k, p in enumerate(periods)]

    def make():
        return realtime.HopSession(C, B, sr=SR, n_fft=F, ring_seconds=8 * B / SR, want_rel=True)

    members = [make() for _ in range(S)]
    twins = [make() for _ in range(4)]
    assert members[0].ring_samples == 8 * B
    group = realtime.HopSessionGroup(members)
    n_on = [0] * 4
    for i in range(nb):
        want = [twins[k](hops_of(xs[k], B, i)) for k in range(4)]
        got = group(np.stack([hops_of(xs[s % 4], B, i) for s in range(S)]))
        for s in range(S):
            assert_same(got[s], want[s % 4], (s, i))
        for k in range(4):
            n_on[k] += len(want[k]["onsets"])
    assert len(set(bits(want[k]["mel"]).tobytes() for k in range(4))) == 4  # (the four streams do differ)
    assert sum(n_on) > 0
    ring = [t.audio(8 * B) for t in twins]
    for s in (0, 1, 2, 3, 50, 95):
        assert np.array_equal(bits(members[s].audio(8 * B)), bits(ring[s % 4]))
    close_all(group, *members, *twins)


# ---- 5: ring seam, joining mid-stream, reset and warm-up inside a group, release ----------------------------

def test_members_join_mid_stream_reset_in_the_group_and_leave_it():
    from onset_fingerprinting_amd import realtime
    from onset_fingerprinting_amd.pipeline import seeded_fcnn
    C, B, F = 2, 64, 256
    R = 5 * B + 17   # not a multiple of the hop: writes straddle the end of the ring
    xs = [stream(11, 0.05), stream(12, 0.07)]
    clf = seeded_fcnn(40, 8, seed=3)

    def make():
        return realtime.HopSession(C, B, sr=SR, n_fft=F, ring_seconds=R / SR, want_rel=True, classifier=clf)

    members, twins = [make(), make()], [make(), make()]
    assert members[0].ring_samples == R
    pos = [0, 0]  # next hop of each stream

    def step(group):
        hops = [hops_of(xs[s], B, pos[s]) for s in range(2)]
        got = group(hops) if group is not None else [members[s](hops[s]) for s in range(2)]
        for s in range(2):
            assert_same(got[s], twins[s](hops[s]), (s, pos[s]))
            pos[s] += 1

    for _ in range(20):
        step(None)
    group = realtime.HopSessionGroup(members)   # both join 20 hops into their streams, rings wrapped
    for _ in range(20):
        step(group)
    members[1].reset()                           # inside the group; its stream starts again, warmed up
    twins[1].reset()
    warm = xs[1][:2000]
    members[1].init_minmax_tracker(warm)
    twins[1].init_minmax_tracker(warm)
    pos[1] = 0
    assert members[1].current_index == 0
    for _ in range(10):
        step(group)
    group.close()
    assert all(m._group is None for m in members)
    for _ in range(20):
        step(None)
    assert pos == [70, 30]
    for m, t in zip(members, twins):
        assert m.current_index == t.current_index
        assert np.array_equal(bits(m.audio(R)), bits(t.audio(R)))
    close_all(*members, *twins)


# ---- 6: refusals -------------------------------------------------------------------------------------------

def test_refusals_leave_the_sessions_usable(monkeypatch):
    from onset_fingerprinting_amd import realtime
    from onset_fingerprinting_amd._lib import OnsetFPError
    C, B, F = 2, 64, 256
    x = stream(11, 0.05)

    def make(C=C, F=F, **kw):
        return realtime.HopSession(C, B, sr=SR, n_fft=F, ring_seconds=0.05, **kw)

    a, b, twin_a, twin_b = make(), make(), make(), make()
    with pytest.raises(ValueError):
        realtime.HopSessionGroup([])
    with pytest.raises(ValueError):
        realtime.HopSessionGroup([a, a])
    odd = [make(F=512), make(C=3), make(onset_strength=dict(max_length=5, avg_length=7))]
    monkeypatch.setenv("OFP_HOP_GRAPH", "nodes")
    odd.append(make())
    monkeypatch.delenv("OFP_HOP_GRAPH")
    for other, what in zip(odd, ("n_fft", "channels", "onset strength", "five-node")):
        with pytest.raises(OnsetFPError, match=what):
            realtime.HopSessionGroup([a, other])
    loc, _, _, _ = session("rt3_fast3")
    noloc, _, _, _ = session("rt3_fast3", locator=False)
    with pytest.raises(OnsetFPError, match="locator"):
        realtime.HopSessionGroup([loc, noloc])
    hop = hops_of(x, B, 0)
    b.submit(hop)
    with pytest.raises(OnsetFPError, match="in flight"):
        realtime.HopSessionGroup([a, b])
    assert_same(b.collect(), twin_b(hop), "b")
    assert a._group is None and b._group is None
    # a real group: what its members and the group refuse
    group = realtime.HopSessionGroup([a, b])
    with pytest.raises(ValueError):
        realtime.HopSessionGroup([a])            # already in a group
    with pytest.raises(OnsetFPError, match="group"):
        a(hop)                                   # a member's hops go through the group
    with pytest.raises(OnsetFPError, match="group"):
        a.push_raw(hop)
    with pytest.raises(ctypes.ArgumentError):
        group(np.zeros((2, B, C), np.float64))
    with pytest.raises(ctypes.ArgumentError):
        group([hop, hop.astype(np.float64)])
    with pytest.raises(ValueError):
        group(np.zeros((2, B - 1, C), np.float32))
    with pytest.raises(ValueError):
        group([hop, hop[:-1]])
    with pytest.raises(ValueError):
        group([hop])
    group.submit([hop, hop])
    with pytest.raises(OnsetFPError, match="not been collected"):
        group.submit([hop, hop])
    got = group.collect()
    assert_same(got[0], twin_a(hop), "a in the group")
    twin_b(hop)
    group.close()
    with pytest.raises(ValueError):
        group([hop, hop])                        # closed
    # after all of it every session still works alone and none has lost or gained a hop
    for i in range(1, 6):
        h = hops_of(x, B, i)
        assert_same(a(h), twin_a(h), i)
        assert_same(b(h), twin_b(h), i)
    for s in odd + [loc, noloc]:
        r = s(np.zeros((s.block_size, s.n_signals), np.float32))
        assert len(r["onsets"]) == 0 and s.current_index == s.block_size
    close_all(a, b, twin_a, twin_b, loc, noloc, *odd)


# ---- 7: a group of one ---------------------------------------------------------------------------------------

def test_a_group_of_one_is_the_plain_session():
    from onset_fingerprinting_amd import realtime
    from onset_fingerprinting_amd.pipeline import seeded_fcnn
    C, B, F = 2, 64, 256
    x = stream(11, 0.05)
    clf = seeded_fcnn(40, 8, seed=1)
    member, twin = (realtime.HopSession(C, B, sr=SR, n_fft=F, ring_seconds=0.05, want_rel=True, classifier=clf)
                    for _ in range(2))
    group = realtime.HopSessionGroup([member])
    n_on = 0
    for i in range(100):
        hop = hops_of(x, B, i)
        want = twin(hop)
        if i % 2:
            assert_same(group(hop[None])[0], want, i)
        else:  # the path the latency tool times: counts only, outputs in the member's host arrays
            assert group.push_raw(hop[None]) == [len(want["onsets"])]
            assert np.array_equal(bits(member._mel), bits(want["mel"])) and np.array_equal(bits(member._rel), bits(want["rel"]))
        n_on += len(want["onsets"])
    assert n_on > 0 and member.current_index == twin.current_index == 100 * B
    close_all(group, member, twin)
