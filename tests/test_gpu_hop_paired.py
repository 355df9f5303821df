"""The voting locator of a stream ("The voting locator in the hop"): the replay entry
``MultilateratePaired.locate_cc_stream_device`` and ``realtime.HopSession(locator=MultilateratePaired(...))`` against a
numpy restatement -- ``online_hits`` with F = left + right, pre = left, then first / onset from the row, the oracle's
``find_ref`` on the window rows and ``vote_ref`` on the locator's slot maps -- and against the batched
``locate_cc_device`` / ``locate_cc_groups_device``.  Everything is equal; the coordinates are bit-equal (one device
function forms them).  The synthetic streams hold integers in -127..127 times 1/256, so every sum of the correlation
is exact whatever its order (tests/test_hop_paired_cpu.py shows that, and that the cases reach every vote branch)."""
import functools
import json

import numpy as np
import pytest

from oracle import locate_kernels as K
from tests.conftest import load_golden
from tests.test_gpu_hop_regress import EDGES, SESSION_CASE, SESSION_RING_ROWS, online_hits

B = 128
UNIT = K.UNIT
NEG = K.PAIRED_NEG_WINDOW

# the oracle's small models (S = 2, 3, 5), one of four sensors and the default grid: 14-inch head, scale 10, side 357
# (127 449 cells: the last bitmap word is partial)
S4 = ([[0.9, 0], [0.95, 90], [0.9, 180], [1.0, 270]], 8, 1, 48000)
DEFAULT = ([[0.9, 0], [0.9, 120], [0.9, 240]], 14 * 2.54, 10, 96000)
MODELS = {"p2": K.PAIRED_MODELS[0], "p3": K.PAIRED_MODELS[1], "p5": K.PAIRED_MODELS[2], "p4": S4, "default": DEFAULT}


@functools.lru_cache(None)
def tables(name):
    """The oracle's tables of a model and its slot maps."""
    p = K.Paired(*MODELS[name])
    return p, [p.slot_map(s) for s in range(2 * p.S)]


# ---- the semantics, restated (no GPU) -------------------------------------------------------------------------------

def first_of(row):
    """(first, onset) of a group row: the earliest channel present, ties by channel (k_paired_windows)."""
    onset, first = min((int(v), k) for k, v in enumerate(row) if v >= 0)
    return first, onset


def window_rows(audio, S, first, onset, left, right):
    """The three rows locate_cc correlates: the first channel, (first - 1) % S and (first + 1) % S."""
    w = audio[onset - left:onset + right]
    assert len(w) == left + right  # never clipped: the stage waits for the last row
    return w[:, first], w[:, (first - 1) % S], w[:, (first + 1) % S]


def restate(case):
    """Per hop None or a dict(status, onset, first, group, lags, cell); and the FIFO's length per hop."""
    p, slots = tables(case["model"])
    audio, left, right = case["audio"], case["left"], case["right"]
    ch, on = [c for c, _ in case["onsets"]], [s for _, s in case["onsets"]]
    hits, pending, _ = online_hits(ch, on, len(audio) // B, B, p.S, left + right, left, case["D"], case["minc"])
    out = []
    for h in hits:
        if h is None:
            out.append(None)
            continue
        start, row = h
        first, onset = first_of(row)
        assert start == onset - left
        e = dict(status=K.PAIRED_OK, onset=onset, first=first, group=row, lags=None, cell=-1)
        if start < 0:
            e["status"] = NEG
        else:
            a, b0, b1 = window_rows(audio, p.S, first, onset, left, right)
            e["lags"] = np.array([K.find_ref(a, b0, 0)[0], K.find_ref(a, b1, 0)[0]], np.int32)
            e["cell"] = K.vote_ref(slots, p.S, first, e["lags"], case["tol"])[1]
        out.append(e)
    return out, pending


# ---- the synthetic streams ------------------------------------------------------------------------------------------

def int_noise(n, C, seed, amp=3):
    return (np.random.default_rng(seed).integers(-amp, amp + 1, (n, C)) * UNIT).astype(np.float32)


def picks_for(name, seed, reach):
    """(first, lag0, lag1) from the oracle's vote_hits -- real cells, two different cells, the extremes of the maps and
    beyond them -- plus one pair beyond both maps, as far as an impulse pair `reach` samples apart can show them."""
    p, slots = tables(name)
    first, lags = K.vote_hits(slots, p.S, seed)
    out = [(int(f), int(l[0]), int(l[1])) for f, l in zip(first, lags.astype(np.int64))]
    for i in range(p.S):
        out.append((i, int(np.nanmin(slots[2 * i])) - 3, int(np.nanmax(slots[2 * i + 1])) + 3))
    keep = [q for q in out if abs(q[1]) < reach and abs(q[2]) < reach]
    keep = [q for k, q in enumerate(keep) if q not in keep[:k]]
    rank = [sum(r[0] == q[0] for r in keep[:k]) for k, q in enumerate(keep)]  # sensor by sensor in turn, so that a
    return [q for _, _, q in sorted(zip(rank, range(len(keep)), keep))]         # short stream meets every first sensor


def impulse_stream(name, left, right, tol, seed, D=300, minc=None, limit=18):
    """One group per pick, 2 D + window apart: the first channel fires at `onset`, the others 5, 9, ... samples later;
    impulses in the window make the correlation peak at the pick's lags (channel (first - 1) % S leads by lag0,
    (first + 1) % S by lag1; with S == 2 they are one channel and lag1 is dropped)."""
    p, _ = tables(name)
    S, w = p.S, left + right
    picks = picks_for(name, seed, max(w // 2 - 1, 1))[:limit]
    gap = 2 * D + w
    n = -(-(left + 64 + gap * (len(picks) + 1)) // B) * B
    audio = int_noise(n, S, seed)
    onsets = []
    for k, (first, lag0, lag1) in enumerate(picks):
        onset = left + 64 + gap * k
        at = onset - left + w // 2
        audio[onset - left:onset + right] = int_noise(w, S, seed + k + 1, amp=1)
        audio[at, first] = 127 * UNIT
        audio[at - lag0, (first - 1) % S] += 100 * UNIT
        if S > 2:
            audio[at - lag1, (first + 1) % S] += 100 * UNIT
        onsets += [((first + j) % S, onset + (0, 5, 9, 11, 13)[j]) for j in range(S)]
    return dict(model=name, audio=audio, onsets=onsets, left=left, right=right, tol=tol, D=D,
                minc=S if minc is None else minc)


def edge_case(name):
    """The state-machine edges of the regress stage's tests with F = 64 = left + right, pre = 16 = left."""
    onsets, minc, _ = EDGES[name]
    return dict(model="p3", audio=int_noise(20 * B, 3, 3, amp=127), onsets=onsets, left=16, right=48, tol=2, D=300,
                minc=minc)


def length_case(w):
    """Window lengths on both sides of 256 threads (2 w - 1 lags) and of two passes, 1 and the cap."""
    if w < 64:
        return dict(model="p3", audio=int_noise(12 * B, 3, w, amp=127), onsets=[(1, 300), (2, 303), (0, 310)], left=0,
                    right=w, tol=2, D=300, minc=3)
    return impulse_stream("p3", 0, w, 2, seed=w, limit=4)


def flat_case(value):
    """A constant window: 0 makes every lag tie (the first maximum, lag -(w - 1)); a constant gives a triangle."""
    audio = np.full((16 * B, 3), value * UNIT, np.float32)
    return dict(model="p3", audio=audio, onsets=[(2, 400), (0, 404), (1, 409), (0, 1200), (1, 1201), (2, 1202)], left=16,
                right=240, tol=2, D=300, minc=3)


def nan_case():
    c = impulse_stream("p3", 16, 240, 2, seed=77, limit=4)
    on = sorted(s for _, s in c["onsets"])
    c["audio"][on[0] + 40, 1] = np.nan   # in the first group's window, on one channel
    c["audio"][on[3] + 7, :] = np.nan    # in the second group's window, on every channel
    return c


CASES = {f"edge_{n}": functools.partial(edge_case, n) for n in sorted(EDGES)}
NO_GROUP = {"edge_onset_one_past_anchor_plus_distance"}  # the edge is that no group with three channels forms
for _name, _left in (("p2", 0), ("p3", 16), ("p5", 0), ("p4", 16)):
    for _tol in (0, 0.5, 2, 2.5):
        CASES[f"vote_{_name}_tol{_tol}"] = functools.partial(impulse_stream, _name, _left, 256 - _left, _tol, seed=5)
for _w in (1, 255, 256, 257, 1024):
    CASES[f"length_{_w}"] = functools.partial(length_case, _w)
CASES["flat_zero"] = functools.partial(flat_case, 0)
CASES["flat_constant"] = functools.partial(flat_case, 64)
CASES["nan_sample"] = nan_case
CASES["default_grid"] = functools.partial(impulse_stream, "default", 0, 256, 2, seed=9, limit=10)
CASES["default_grid_tol0"] = functools.partial(impulse_stream, "default", 16, 240, 0, seed=9, limit=3)


# ---- (a) the replay against the restatement --------------------------------------------------------------------------

def ml():
    from onset_fingerprinting_amd import multilateration
    return multilateration


@functools.lru_cache(None)
def locator(name):
    loc, d, scale, sr = MODELS[name]
    m = ml().MultilateratePaired(loc, drum_diameter=d, scale=scale, sr=sr)
    p, _ = tables(name)
    assert (m.side, m.radius, m.n_buckets) == (p.side, p.radius, p.n_buckets)
    return m


def replay(m, case):
    return m.locate_cc_stream_device(case["audio"], [c for c, _ in case["onsets"]], [s for _, s in case["onsets"]], B,
                                     tol=case["tol"], left=case["left"], right=case["right"], max_distance=case["D"],
                                     min_channels=case["minc"])


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def batched_rphi(m, audio, want, tol, left, right):
    """locate_cc_device on the evaluated hits -> rphi float64 [n, 2], cell, status."""
    import torch
    on = torch.tensor([e["onset"] for e in want], dtype=torch.int64, device=m.device)
    first = torch.tensor([e["first"] for e in want], dtype=torch.int32, device=m.device)
    x = torch.from_numpy(np.ascontiguousarray(audio)).to(m.device)
    rphi, cell, status = m.locate_cc_device(x, on, first, tol=tol, left=left, right=right)
    return rphi.cpu().numpy(), cell.cpu().numpy(), status.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_replay_against_the_restatement(name):
    case = CASES[name]()
    m = locator(case["model"])
    want, pending = restate(case)
    got = replay(m, case)
    assert np.array_equal(got["hit"], [e is not None for e in want]), (np.flatnonzero(got["hit"]), want)
    assert np.array_equal(got["pending"], pending)
    hops = [h for h, e in enumerate(want) if e is not None]
    assert bool(hops) == (name not in NO_GROUP)
    if not hops:
        return
    for key in ("status", "onset", "first"):
        assert np.array_equal(got[key][hops], [want[h][key] for h in hops]), key
    assert np.array_equal(got["group"][hops], np.stack([want[h]["group"] for h in hops]))
    ok = [h for h in hops if want[h]["status"] == K.PAIRED_OK]
    for h in hops:
        if want[h]["status"] != K.PAIRED_OK:  # refused as the batched form refuses it: no position
            assert got["cell"][h] == -1 and np.isnan(got["rphi"][h]).all()
    assert np.isnan(got["rphi"][~got["hit"]]).all()
    if not ok:
        return
    assert np.array_equal(got["lags"][ok], np.stack([want[h]["lags"] for h in ok])), (got["lags"][ok], [want[h]["lags"] for h in ok])
    assert np.array_equal(got["cell"][ok], [want[h]["cell"] for h in ok])
    rphi, cell, status = batched_rphi(m, case["audio"], [want[h] for h in ok], case["tol"], case["left"], case["right"])
    assert not status.any() and np.array_equal(cell, got["cell"][ok])
    assert np.array_equal(bits(got["rphi"][ok]), bits(rphi))


@pytest.mark.gpu
def test_replay_reports_an_overflowing_queue_and_a_refused_onset():
    """The replay takes parameters a session's constructor refuses: twelve groups 20 samples apart with windows of the
    cap are all pending before the first is due.  The flags are raised, never silent."""
    from onset_fingerprinting_amd import _lib
    m = locator("p3")
    audio = int_noise(24 * B, 3, 1, amp=127)
    onsets = [(c, 200 + 20 * k + c) for k in range(12) for c in range(3)]
    with pytest.raises(_lib.OnsetFPError, match="overflow"):
        m.locate_cc_stream_device(audio, [c for c, _ in onsets], [s for _, s in onsets], B, right=1024, max_distance=10)
    with pytest.raises(_lib.OnsetFPError, match="refused"):
        m.locate_cc_stream_device(audio, [0, 5, 1], [300, 301, 302], B)
    few = dict(model="p3", audio=audio, onsets=onsets[:9], left=0, right=1024, tol=2, D=10, minc=3)
    got, (want, pending) = replay(m, few), restate(few)
    assert np.array_equal(got["hit"], [e is not None for e in want]) and got["hit"].sum() == 3 and max(pending) == 3


# ---- (b) the session ----------------------------------------------------------------------------------------------------

SESSION = dict(tol=2, left=32, right=224, max_distance=1000, min_channels=3)  # the regress tests' windows: F 256, pre 32


def stream():
    g = load_golden("g25_hoplocate")
    args = json.loads(str(g[f"{SESSION_CASE}/args"]))
    det = {k: (tuple(v) if isinstance(v, list) else v) for k, v in args["detector"].items()}
    audio = g[f"{SESSION_CASE}/audio"]
    assert (audio.shape[1], args["hop"], args["sr"]) == (3, 128, 96000)
    return audio, det


def session(det, ring_rows=SESSION_RING_ROWS, **kw):
    from onset_fingerprinting_amd import realtime
    return realtime.HopSession(3, 128, sr=96000, n_fft=256, ring_seconds=ring_rows / 96000, **det, **kw)


def play(sess, audio, n_hops=None):
    n_hops = len(audio) // 128 if n_hops is None else n_hops
    return [sess(audio[h * 128:(h + 1) * 128]) for h in range(n_hops)]


def same_hit(a, b, where):
    assert (a is None) == (b is None), where
    if a is not None:
        assert set(a) == set(b)
        for k in a:
            assert np.array_equal(a[k], b[k]), (where, k, a[k], b[k])


def same_location(a, b, where):
    assert (a is None) == (b is None), where
    if a is not None:
        assert np.array_equal(bits(a), bits(b)), (where, a, b)


def assert_session(results, m, audio, p):
    """A session's dicts against the replay fed the session's own onsets, and against the batched form on the whole
    recording with the same rows.  -> the evaluated hops."""
    import torch
    ch = np.concatenate([r["channels"] for r in results])
    on = np.concatenate([r["onsets"] for r in results])
    n = len(results)
    rep = m.locate_cc_stream_device(audio[:n * 128], ch, on, 128, **p)
    hops = np.flatnonzero(rep["hit"])
    for h, r in enumerate(results):
        if not rep["hit"][h]:
            assert r["cc_hit"] is None and r["location"] is None, h
            continue
        want = dict(status=int(rep["status"][h]), onset=int(rep["onset"][h]), first=int(rep["first"][h]),
                    group=rep["group"][h], lags=rep["lags"][h], cell=int(rep["cell"][h]))
        same_hit(r["cc_hit"], want, h)
        same_location(r["location"], tuple(rep["rphi"][h]) if want["status"] == K.PAIRED_OK else None, h)
    ok = [h for h in hops if rep["status"][h] == K.PAIRED_OK]
    x = torch.from_numpy(np.ascontiguousarray(audio)).to(m.device)
    groups = torch.from_numpy(rep["group"][ok]).to(m.device).unsqueeze(0)
    rphi, cell, status = ml().locate_cc_groups_device(x, groups, None, m, tol=p["tol"], left=p["left"], right=p["right"])
    assert not status.cpu().numpy().any()  # these windows are complete: the batched form clips none of them
    assert np.array_equal(cell.cpu().numpy()[0], rep["cell"][ok])
    assert np.array_equal(bits(rphi.cpu().numpy()[0]), bits(rep["rphi"][ok]))
    lags = m._vote(x.unsqueeze(0), None, (groups, None), p["tol"], p["left"], p["right"])[3]  # (the batched form's own)
    assert np.array_equal(lags.cpu().numpy(), rep["lags"][ok])
    _, slots = tables("p3")
    for h in ok:  # and the cell is the oracle's vote for the device's lags
        assert rep["cell"][h] == K.vote_ref(slots, 3, int(rep["first"][h]), rep["lags"][h], p["tol"])[1], h
    return hops


def same_but(a, b):
    for k in a:
        if isinstance(a[k], np.ndarray):
            assert np.array_equal(a[k].view(np.uint32) if a[k].dtype == np.float32 else a[k],
                                  b[k].view(np.uint32) if b[k].dtype == np.float32 else b[k]), k
        else:
            assert a[k] == b[k] or (a[k] is None and b[k] is None), k


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["fused", "nodes"])
def test_session_on_a_ring_the_windows_wrap_around(form, monkeypatch):
    monkeypatch.setenv("OFP_HOP_GRAPH", form)
    audio, det = stream()
    m = locator("p3")
    res_before = m.res.copy()
    sess = session(det, locator=m, **SESSION)
    assert sess.ring_samples == SESSION_RING_ROWS
    first = play(sess, audio)
    hops = assert_session(first, m, audio, SESSION)
    assert len(hops) >= 10
    starts = [first[h]["cc_hit"]["onset"] - SESSION["left"] for h in hops]
    assert any(s % SESSION_RING_ROWS + 256 > SESSION_RING_ROWS for s in starts)  # a window across the ring's wrap
    assert np.array_equal(m.res, res_before)  # the session writes no vote grid
    plain = play(session(det), audio, 300)  # the other outputs are the plain session's, bit for bit
    assert sum(len(r["onsets"]) for r in plain) >= 9
    for a, b in zip(plain, first):
        same_but(a, b)
        assert set(b) == set(a) | {"location", "cc_hit"}
    sess.reset()  # the state is cleared: the same stream gives the same answers
    again = play(sess, audio, 300)
    for h, (a, b) in enumerate(zip(first, again)):
        same_hit(a["cc_hit"], b["cc_hit"], h)
        same_location(a["location"], b["location"], h)
    sess.close()


@pytest.mark.gpu
def test_group_of_three_locators_is_the_members_alone():
    from onset_fingerprinting_amd import realtime
    audio, det = stream()
    loc = MODELS["p3"][0]
    ms = [ml().MultilateratePaired(loc, drum_diameter=d, scale=1, sr=48000) for d in (8, 10, 12)]
    assert len({m.radius for m in ms}) == 3
    params = [SESSION, dict(tol=0.5, left=0, right=256, max_distance=1000, min_channels=3),
              dict(tol=2.5, left=16, right=100, max_distance=600, min_channels=2)]
    n = 450
    alone = [play(session(det, locator=m, **p), audio, n) for m, p in zip(ms, params)]
    members = [session(det, locator=m, **p) for m, p in zip(ms, params)]
    group = realtime.HopSessionGroup(members)
    hops = np.stack([audio] * 3)
    for h in range(n):
        out = group(np.ascontiguousarray(hops[:, h * 128:(h + 1) * 128]))
        for i in range(3):
            same_hit(alone[i][h]["cc_hit"], out[i]["cc_hit"], (i, h))
            same_location(alone[i][h]["location"], out[i]["location"], (i, h))
            same_but({k: v for k, v in alone[i][h].items() if k not in ("cc_hit", "location")}, out[i])
    for i in range(3):
        assert sum(r["cc_hit"] is not None for r in alone[i]) >= 3
    group.close()
    for s in members:
        s.close()


@pytest.mark.gpu
def test_refused_at_construction():
    from onset_fingerprinting_amd import model
    _, det = stream()
    m = locator("p3")
    with pytest.raises(ValueError, match="regressor"):
        session(det, locator=m, regressor=model.CNN(256, 2, 3), **SESSION)
    with pytest.raises(ValueError, match="window cap"):
        session(det, 8000, locator=m, **dict(SESSION, right=1024))
    with pytest.raises(ValueError, match="ring"):
        session(det, SESSION_RING_ROWS - 1, locator=m, **SESSION)
    session(det, 8000, locator=m, **dict(SESSION, left=0, right=1024)).close()  # the cap itself is inside
