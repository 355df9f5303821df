"""The window regressor of a stream ("The window regressor in the hop"): the replay entry
``realtime.regress_stream_device`` and ``realtime.HopSession(regressor=...)`` against a numpy restatement of the
stage's semantics (``online_hits`` below), ``oracle.group_windows``-style extraction and the batched ``model(x)``.
Hit hops, rows and starts are equal and the positions are bit-equal: the stage forms every output by the batched
kernels' own sequence of floating-point operations (csrc/ofp_nn_dev.h)."""
import json

import numpy as np
import pytest
import torch

from tests.conftest import load_golden


# ---- the semantics, restated (no GPU; tests/test_hop_regress_cpu.py checks this function against the oracle) ----

def online_hits(channels, onsets, n_hops, B, C, F, pre, D, min_channels):
    """-> (hits: per hop None or (start, row int64 [C]); pending: the FIFO's length before each hop's evaluation;
    groups: every kept row in closing order).  Feed order: sorted by sample, stable; hop h (from 1) takes the onsets
    below h * B."""
    order = np.argsort(np.asarray(onsets, np.int64), kind="stable")
    feed = [(int(onsets[i]), int(channels[i])) for i in order]
    cur, fifo, groups, k = [], [], [], 0
    hits, pending = [None] * n_hops, [0] * n_hops

    def close():
        if len({c for _, c in cur}) >= min_channels:
            row = np.full(C, -1, np.int64)
            for s, c in cur:
                row[c] = s  # the last onset of a channel wins
            fifo.append((int(row[row >= 0].min()) - pre, row))
            groups.append(row)

    for h in range(1, n_hops + 1):
        end = h * B
        while k < len(feed) and feed[k][0] < end:
            s, c = feed[k]
            k += 1
            if cur and s - cur[0][0] > D:
                close()
                cur = []
            cur.append((s, c))
        if cur and end > cur[0][0] + D:  # no later onset can join
            close()
            cur = []
        pending[h - 1] = len(fifo)
        if fifo and end >= fifo[0][0] + F:  # the head's last row has arrived; one group per hop
            hits[h - 1] = fifo.pop(0)
    return hits, pending, groups


def window(audio, start, F):
    """[C, F] from row `start`; rows before sample 0 are zeros."""
    out = np.zeros((audio.shape[1], F), np.float32)
    lo = max(start, 0)
    out[:, lo - start:] = audio[lo:start + F].T
    return out


# the parameters of the session tests on the golden g25 stream (3 channels x 128 samples at 96 kHz); the CPU test
# file checks that they yield hits and windows across the ring's wrap on the committed onsets
SESSION = dict(frame_length=256, pre_samples=32, max_distance=1000, min_channels=3)
SESSION_CASE = "rt3_fast3"
SESSION_RING_ROWS = 2312  # realtime.regress_ring_rows(128, 256, 32, 1000): the shortest ring the constructor admits


# ---- models -----------------------------------------------------------------------------------------------------

def randomise(model, seed):
    """Non-trivial norm layers: running statistics and affine parameters away from their initial 0 / 1."""
    g = torch.Generator().manual_seed(seed)
    for m in model.modules():
        if isinstance(m, torch.nn.BatchNorm1d):
            m.running_mean.copy_(torch.randn(m.num_features, generator=g) * 0.3)
            m.running_var.copy_(torch.rand(m.num_features, generator=g) + 0.5)
        if isinstance(m, (torch.nn.BatchNorm1d, torch.nn.GroupNorm)):
            with torch.no_grad():
                m.weight.copy_(torch.rand(m.weight.shape, generator=g) + 0.5)
                m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.2)
    return model.eval()


def make(cls, *a, seed=0, **kw):
    from onset_fingerprinting_amd import model
    torch.manual_seed(seed)
    return randomise(getattr(model, cls)(*a, **kw), seed + 1)


def batched(model, audio, hits, F):
    """The existing batched forward on the hits' windows -> float32 [n, n_out]."""
    x = np.stack([window(audio, s, F) for s, _ in hits])
    with torch.no_grad():
        return model(torch.from_numpy(x).cuda()).cpu().numpy()


def assert_replay(model, audio, channels, onsets, B, F, pre, D, minc):
    """The replay against the restatement and the batched forward; -> (expected hits per hop, pending per hop)."""
    from onset_fingerprinting_amd import realtime
    import oracle
    H, C = len(audio) // B, audio.shape[1]
    want, pending, _ = online_hits(channels, onsets, H, B, C, F, pre, D, minc)
    got = realtime.regress_stream_device(model, audio, channels, onsets, B, F, pre, D, minc)
    assert np.array_equal(got["hit"], [w is not None for w in want]), (np.flatnonzero(got["hit"]), want)
    assert np.array_equal(got["pending"], pending)
    hops = [h for h, w in enumerate(want) if w is not None]
    hits = [want[h] for h in hops]
    if not hits:
        return want, pending
    assert np.array_equal(got["start"][hops], [s for s, _ in hits])
    assert np.array_equal(got["group"][hops], np.stack([r for _, r in hits]))
    for s, r in hits:  # where every channel is present and the clip holds the window this is oracle.group_windows
        if (r >= 0).all():
            assert np.array_equal(window(audio, s, F), oracle.group_windows(audio, r[None], F, pre)[0])
    ref = batched(model, audio, hits, F)
    assert np.array_equal(got["position"][hops].view(np.uint32), ref.view(np.uint32)), \
        np.abs(got["position"][hops] - ref).max()
    assert np.isfinite(ref).all() and np.abs(ref).max() > 0
    return want, pending


def noise(n, C, seed=3):
    return np.random.default_rng(seed).standard_normal((n, C)).astype(np.float32)


# ---- (a) the replay entry at the edges of the state machine -------------------------------------------------------
B, F, PRE, D = 128, 64, 16, 300  # hop 10 ends at 1280, hop 12 at 1536


def trio(a, d1=5, d2=9):
    return [(0, a), (1, a + d1), (2, a + d2)]


EDGES = {
    # name: (onsets as (channel, sample), min_channels, what the restatement must show)
    "start_before_sample_0": (trio(5), 3, lambda hits, pend: hits[[h is not None for h in hits].index(True)][0] == -11),
    # start + F == h * B exactly: anchor 1280 - 64 + 16 -> evaluated in the hop that closes it or later, never earlier
    "window_ends_with_the_hop": (trio(1280 - F + PRE), 3, None),
    "window_ends_one_sample_later": (trio(1280 - F + PRE + 1), 3, None),
    "hop_ends_at_anchor_plus_distance": (trio(1280 - D), 3, lambda hits, pend: pend[9] == 0 and pend[10] == 1),
    "hop_ends_one_past_anchor_plus_distance": (trio(1280 - D - 1), 3, lambda hits, pend: pend[9] == 1),
    "onset_at_anchor_plus_distance": ([(0, 700), (1, 705), (2, 700 + D)], 3,
                                      lambda hits, pend: sum(h is not None for h in hits) == 1),
    "onset_one_past_anchor_plus_distance": ([(0, 700), (1, 705), (2, 700 + D + 1)], 3,
                                            lambda hits, pend: sum(h is not None for h in hits) == 0),
    "channel_fires_twice": ([(0, 700), (1, 705), (0, 760), (2, 770)], 3,
                            lambda hits, pend: [h for h in hits if h is not None][0][1][0] == 760),
    "the_anchor_channel_fires_again": ([(0, 700), (0, 760), (1, 770), (2, 780)], 3,
                                       lambda hits, pend: [h for h in hits if h is not None][0][0] == 760 - PRE),
    "below_min_channels": ([(0, 700), (1, 705)] + trio(1500), 3,
                           lambda hits, pend: sum(h is not None for h in hits) == 1),
    "missing_channel": ([(0, 700), (2, 705)], 2, lambda hits, pend: [h for h in hits if h is not None][0][1][1] == -1),
    "ties_keep_list_order": ([(2, 700), (0, 700), (1, 700)], 3, None),
}


@pytest.fixture(scope="module")
def edge_model():
    return make("CNN", F, 2, 3, layer_sizes=[3, 5])


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(EDGES))
def test_replay_at_the_edges_of_the_state_machine(name, edge_model):
    onsets, minc, shows = EDGES[name]
    audio = noise(20 * B, 3)
    want, pend = assert_replay(edge_model, audio, [c for c, _ in onsets], [s for _, s in onsets], B, F, PRE, D, minc)
    assert shows is None or shows(want, pend), (want, pend)


@pytest.mark.gpu
def test_replay_with_groups_queueing():
    """A long window after short groups: three groups pending at once, and two due in the same hop (the second is
    evaluated one hop later)."""
    Fq, Dq = 1024, 128
    m = make("CNN", Fq, 2, 3, layer_sizes=[2, 2], pool=True)
    # the first group's row is rewritten 100 samples after its anchor: its start lies 29 samples before the next one's
    onsets = [(0, 1000), (0, 1100), (1, 1100), (2, 1110)] + trio(1129) + trio(1300) + trio(1500) + trio(3000)
    audio = noise(40 * B, 3)
    want, pend = assert_replay(m, audio, [c for c, _ in onsets], [s for _, s in onsets], B, Fq, 0, Dq, 3)
    assert max(pend) >= 3
    hops = [h for h, w in enumerate(want) if w is not None]
    assert len(hops) == 5
    s0, s1 = want[hops[0]][0], want[hops[1]][0]
    assert -(-(s0 + Fq) // B) == -(-(s1 + Fq) // B) == hops[0] + 1 and hops[1] == hops[0] + 1  # both due in one hop


@pytest.mark.gpu
@pytest.mark.parametrize("anchor,hit_hop", [(1024, 16), (1025, 17)])
def test_the_due_condition_decides_the_hop(anchor, hit_hop):
    """h * B == start + frame_length exactly, and one sample short of it, where nothing but the due condition decides:
    with max_distance = B = 128 the group closes at the end of hop 10, long before its 1024-sample window is complete.
    Start 1024 ends its window with hop 16 (16 * 128 == 1024 + 1024) and is evaluated there; start 1025 is one sample
    short at that hop end and is evaluated in hop 17."""
    Fq, Dq = 1024, 128
    m = make("CNN", Fq, 2, 3, layer_sizes=[2, 2], pool=True)
    onsets = trio(anchor)
    audio = noise(24 * B, 3)
    want, pend = assert_replay(m, audio, [c for c, _ in onsets], [s for _, s in onsets], B, Fq, 0, Dq, 3)
    assert pend[9] == 1 and pend[8] == 0  # closed at the end of hop 10
    assert [h + 1 for h, w in enumerate(want) if w is not None] == [hit_hop]
    assert want[hit_hop - 1][0] == anchor  # (assert_replay has compared the device's hit hops with `want`)


@pytest.mark.gpu
def test_replay_with_groups_shorter_than_a_hop():
    """The replay has no max_distance >= block_size condition: several groups close in one hop."""
    onsets = trio(300, 2, 4) + trio(350, 2, 4) + trio(400, 2, 4) + trio(900, 1, 2)
    m = make("CNN", F, 2, 3, layer_sizes=[3, 5])
    want, pend = assert_replay(m, noise(16 * B, 3), [c for c, _ in onsets], [s for _, s in onsets], B, F, PRE, 40, 3)
    assert max(pend) >= 2 and sum(w is not None for w in want) == 4  # (two groups close in hop 4)


@pytest.mark.gpu
def test_replay_reports_an_overflowing_queue_and_a_refused_onset():
    """The replay takes parameters a session's constructor refuses: 4096-sample windows of groups 129 samples apart
    fill the queue of 8 before the first is due.  The flag is raised, never silent, and the device stays usable."""
    from onset_fingerprinting_amd import _lib, realtime
    m = make("CNN", 4096, 2, 3, layer_sizes=[1])
    assert realtime.regress_pending_bound(B, 4096, 0, 128) > _lib.REG_QUEUE
    onsets = [o for k in range(12) for o in trio(200 + 129 * k, 1, 2)]
    audio = noise(48 * B, 3)
    with pytest.raises(_lib.OnsetFPError, match="overflow"):
        realtime.regress_stream_device(m, audio, [c for c, _ in onsets], [s for _, s in onsets], B, 4096, 0, 128, 3)
    with pytest.raises(_lib.OnsetFPError, match="refused"):
        realtime.regress_stream_device(m, audio, [0, 5, 1], [300, 301, 302], B, 4096, 0, 128, 3)
    few = onsets[:9]  # three groups: within the queue
    assert_replay(m, audio, [c for c, _ in few], [s for _, s in few], B, 4096, 0, 128, 3)


# ---- (b) small models at the tile edges -------------------------------------------------------------------------
ONSETS_B = trio(300) + trio(900, 0, 0) + [(0, 1500), (1, 1510)]  # the last group has no third channel


def cnn23(**kw):
    return dict(cls="CNN", args=(23, kw.pop("output_size", 2)), kw=dict(channels=2, layer_sizes=[3, 5], **kw))


def cccnn20(**kw):
    return dict(cls="CCCNN", args=(20, 2), kw=dict(channels=3, layer_sizes=[2, 3], kernel_sizes=[3, 5], strides=[1, 2], **kw))


SMALL = {
    "cnn": cnn23(),  # fc has 5 * 23 = 115 inputs: not a multiple of the MFMA's 4
    "cnn_17_outputs": cnn23(output_size=17),
    "cnn_bn": cnn23(batch_norm=True),
    "cnn_pool": cnn23(pool=True),
    "cnn_bn_pool_17": cnn23(batch_norm=True, pool=True, output_size=17),
    "cnn_dilation": cnn23(dilation=2),
    "cnn_dilation_bn_pool": cnn23(dilation=2, batch_norm=True, pool=True),
    # (Conv1d needs groups to divide both channel counts: the grouped variant takes layer_sizes [4, 6], fc 6 * 23 = 138)
    "cnn_groups": dict(cls="CNN", args=(23, 2), kw=dict(channels=2, layer_sizes=[4, 6], groups=2)),
    "cnn_groups_bn_pool_17": dict(cls="CNN", args=(23, 17), kw=dict(channels=2, layer_sizes=[4, 6], groups=2, batch_norm=True,
                                                                    pool=True)),
    "cnn_relu": cnn23(activation=torch.nn.ReLU),
    "cccnn": cccnn20(),
    "cccnn_gn": cccnn20(batch_norm=True),
    "cccnn_pool": cccnn20(pool=True),
    "cccnn_gn_pool": cccnn20(batch_norm=True, pool=True),
    "cccnn_grouped": cccnn20(group=True),
    "cccnn_grouped_gn": cccnn20(group=True, batch_norm=True),
    "cccnn_grouped_pool": cccnn20(group=True, pool=True),
    "cccnn_grouped_gn_pool": cccnn20(group=True, batch_norm=True, pool=True),
    "lcccnn_gn_pool": dict(cls="LCCCNN", args=(20, 2), kw=dict(channels=3, layer_sizes=[2, 3], kernel_sizes=[3, 5],
                                                               strides=[1, 2], batch_norm=True, pool=True)),
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(SMALL))
def test_small_models_at_the_tile_edges(name):
    spec = SMALL[name]
    m = make(spec["cls"], *spec["args"], seed=7, **spec["kw"])
    C = spec["kw"]["channels"]
    onsets = [(c, s) for c, s in ONSETS_B if c < C]
    audio = noise(16 * B, C, seed=11)
    want, _ = assert_replay(m, audio, [c for c, _ in onsets], [s for _, s in onsets], B, spec["args"][0], 4, D, 2)
    assert sum(w is not None for w in want) == 3


def workspace_floats(model, F):
    import ctypes

    from onset_fingerprinting_amd import _lib
    from onset_fingerprinting_amd import model as mdl
    r, keep = mdl.hop_regressor_struct(model, 0, F, 0, 1000, 3)
    return int(_lib.lib().ofp_regress_workspace_floats(ctypes.byref(r)))


@pytest.mark.gpu
@pytest.mark.parametrize("width,in_lds", [(47, True), (48, False)])
def test_both_sides_of_the_lds_switch(width, in_lds):
    """Activations stay in LDS while both buffers fit 96 KiB: 2 x 47 x 256 floats do, 2 x 48 x 256 do not."""
    m = make("CNN", 256, 2, 3, layer_sizes=[width, 4], seed=5)
    ws = workspace_floats(m, 256)
    assert (ws == 0) == in_lds and (in_lds or ws == width * 256)
    onsets = trio(300) + trio(1700)
    assert_replay(m, noise(24 * B, 3, seed=13), [c for c, _ in onsets], [s for _, s in onsets], B, 256, 32, 1000, 3)


# ---- (c) the session ----------------------------------------------------------------------------------------------

def stream():
    g = load_golden("g25_hoplocate")
    args = json.loads(str(g[f"{SESSION_CASE}/args"]))
    det = {k: (tuple(v) if isinstance(v, list) else v) for k, v in args["detector"].items()}
    audio = g[f"{SESSION_CASE}/audio"]
    assert (audio.shape[1], args["hop"], args["sr"]) == (3, 128, 96000)
    return audio, det, args


def session(det, ring_rows=SESSION_RING_ROWS, **kw):
    from onset_fingerprinting_amd import realtime
    return realtime.HopSession(3, 128, sr=96000, n_fft=256, ring_seconds=ring_rows / 96000, **det, **kw)


def play(sess, audio, n_hops=None):
    n_hops = len(audio) // 128 if n_hops is None else n_hops
    return [sess(audio[h * 128:(h + 1) * 128]) for h in range(n_hops)]


def assert_session(results, model, audio, p):
    """A session's hits against the restatement fed the session's own onsets, and the batched forward."""
    ch = np.concatenate([r["channels"] for r in results])
    on = np.concatenate([r["onsets"] for r in results])
    want, _, _ = online_hits(ch, on, len(results), 128, 3, p["frame_length"], p["pre_samples"], p["max_distance"],
                             p["min_channels"])
    assert [r["hit"] is not None for r in results] == [w is not None for w in want]
    hops = [h for h, w in enumerate(want) if w is not None]
    hits = [want[h] for h in hops]
    ref = batched(model, audio, hits, p["frame_length"])
    for k, h in enumerate(hops):
        got = results[h]["hit"]
        assert got["start"] == hits[k][0] and np.array_equal(got["group"], hits[k][1]), h
        assert np.array_equal(got["position"].view(np.uint32), ref[k].view(np.uint32)), (h, got["position"], ref[k])
    return hits


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["fused", "nodes"])
@pytest.mark.parametrize("kind", ["cnn", "lcccnn"])
def test_session_on_a_ring_the_windows_wrap_around(kind, form, monkeypatch):
    monkeypatch.setenv("OFP_HOP_GRAPH", form)
    audio, det, _ = stream()
    m = (make("CNN", 256, 2, 3) if kind == "cnn" else
         make("LCCCNN", 256, 2, 3, layer_sizes=[4, 8], kernel_sizes=[5, 3], strides=[2, 1], batch_norm=True, pool=True))
    sess = session(det, regressor=m, **SESSION)
    assert sess.ring_samples == SESSION_RING_ROWS
    first = play(sess, audio)
    hits = assert_session(first, m, audio, SESSION)
    assert len(hits) >= 10
    assert any(s % SESSION_RING_ROWS + 256 > SESSION_RING_ROWS for s, _ in hits)  # a window across the ring's wrap
    sess.reset()  # the state is cleared: the same stream gives the same answers
    again = play(sess, audio, 300)
    for a, b in zip(first, again):
        assert (a["hit"] is None) == (b["hit"] is None)
        if a["hit"] is not None:
            assert np.array_equal(a["hit"]["position"].view(np.uint32), b["hit"]["position"].view(np.uint32))
    sess.close()


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["fused", "nodes"])
def test_session_with_activations_in_the_workspace(form, monkeypatch):
    """A model past the LDS switch in a session: its activations live in the device workspace the session owns."""
    monkeypatch.setenv("OFP_HOP_GRAPH", form)
    audio, det, _ = stream()
    m = make("CNN", 256, 2, 3, layer_sizes=[48, 4], seed=5)
    assert workspace_floats(m, 256) == 48 * 256
    sess = session(det, regressor=m, **SESSION)
    results = play(sess, audio, 450)
    assert len(assert_session(results, m, audio, SESSION)) >= 3
    sess.close()


def same_but(a, b, skip):
    for k in a:
        if k in skip:
            continue
        if isinstance(a[k], np.ndarray):
            assert np.array_equal(a[k].view(np.uint32) if a[k].dtype == np.float32 else a[k],
                                  b[k].view(np.uint32) if b[k].dtype == np.float32 else b[k]), k
        elif isinstance(a[k], dict):
            same_but(a[k], b[k], ())
        else:
            assert a[k] == b[k] or (a[k] is None and b[k] is None), k


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["fused", "nodes"])
def test_locator_and_regressor_together_are_each_alone(form, monkeypatch):
    from onset_fingerprinting_amd import multilateration as ml
    monkeypatch.setenv("OFP_HOP_GRAPH", form)
    audio, det, args = stream()
    m = make("CNN", 256, 2, 3)
    n = 450
    loc = lambda: ml.Multilaterate3D(**args["layout"])
    both = play(session(det, 96000, locator=loc(), regressor=m, **SESSION), audio, n)
    only_loc = play(session(det, 96000, locator=loc()), audio, n)
    only_reg = play(session(det, 96000, regressor=m, **SESSION), audio, n)
    assert sum(r["hit"] is not None for r in both) >= 3 and sum(r["location"] is not None for r in both) >= 3
    for b, l, r in zip(both, only_loc, only_reg):
        same_but(l, b, ())          # everything the locator-only session returns, bit for bit
        same_but(r, b, ())          # and everything the regressor-only session returns
        assert set(b) == set(l) | set(r)


@pytest.mark.gpu
def test_group_of_three_architectures_is_the_members_alone():
    from onset_fingerprinting_amd import realtime
    audio, det, _ = stream()
    models = [make("CNN", 256, 2, 3), make("CNN", 128, 3, 3, layer_sizes=[4, 4], batch_norm=True, pool=True),
              make("LCCCNN", 64, 2, 3, layer_sizes=[2, 3], kernel_sizes=[3, 5], strides=[1, 2], group=True)]
    params = [dict(SESSION, frame_length=m_.input_size if hasattr(m_, "input_size") else m_.model.input_size)
              for m_ in models]
    n = 450
    alone = [play(session(det, regressor=m_, **p), audio, n) for m_, p in zip(models, params)]
    members = [session(det, regressor=m_, **p) for m_, p in zip(models, params)]
    group = realtime.HopSessionGroup(members)
    hops = np.stack([audio] * 3)
    for h in range(n):
        out = group(np.ascontiguousarray(hops[:, h * 128:(h + 1) * 128]))
        for i in range(3):
            same_but(alone[i][h], out[i], ())
    for i in range(3):
        assert sum(r["hit"] is not None for r in alone[i]) >= 3
    group.close()
    # a group must agree on having a regressor
    with pytest.raises(Exception, match="regressor"):
        realtime.HopSessionGroup([members[0], session(det)])
    for s in members:
        s.close()


@pytest.mark.gpu
def test_group_with_locator_and_regressor_is_the_members_alone():
    """The group launch of members that run both stages after the detector (models of different weights)."""
    from onset_fingerprinting_amd import multilateration as ml
    from onset_fingerprinting_amd import realtime
    audio, det, args = stream()
    models = [make("CNN", 256, 2, 3), make("CNN", 256, 2, 3, seed=4)]
    both = lambda m_: session(det, 96000, locator=ml.Multilaterate3D(**args["layout"]), regressor=m_, **SESSION)
    n = 450
    alone = [play(both(m_), audio, n) for m_ in models]
    members = [both(m_) for m_ in models]
    group = realtime.HopSessionGroup(members)
    hops = np.stack([audio] * 2)
    for h in range(n):
        out = group(np.ascontiguousarray(hops[:, h * 128:(h + 1) * 128]))
        for i in range(2):
            same_but(alone[i][h], out[i], ())
            assert set(out[i]) == set(alone[i][h])
    for i in range(2):
        assert sum(r["hit"] is not None for r in alone[i]) >= 3
        assert sum(r["location"] is not None for r in alone[i]) >= 3
    first = [next(r["hit"]["position"] for r in a if r["hit"] is not None) for a in alone]
    assert not np.array_equal(first[0], first[1])  # (each member's answers are its own model's)
    group.close()
    for s in members:
        s.close()


# ---- (d) a session without a regressor --------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("form", ["fused", "nodes"])
def test_a_session_without_a_regressor_is_unchanged(form, monkeypatch):
    monkeypatch.setenv("OFP_HOP_GRAPH", form)
    audio, det, _ = stream()
    plain = play(session(det), audio, 300)
    with_reg = play(session(det, regressor=make("CNN", 256, 2, 3), **SESSION), audio, 300)
    assert all("hit" not in r for r in plain)
    assert sum(len(r["onsets"]) for r in plain) >= 9
    for a, b in zip(plain, with_reg):
        same_but(a, b, ())  # every key of the plain session, bit for bit; the regressor only adds `hit`
        assert set(b) == set(a) | {"hit"}
