"""CPU-only: what tests/test_gpu_seq_train_random.py rests on, checked on the reference alone
(tests/seq_train_random_ref.py): the replay is each trainer's recipe and its masked forward is the plain one when nothing
is dropped; every trajectory case's comparable prefix reaches MIN_PREFIX of EPOCHS, so that the GPU test compares
something; the stretched source draws all four stretches over the epochs used; and the case tables cross the slab,
chunk and workgroup edges they name."""
import copy
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import seq_train_random_ref as Q  # noqa: E402
import test_gpu_cnnrnn_train as GC  # noqa: E402  (helpers only; its tests are collected from its own file)
import test_gpu_rnn_train as GR  # noqa: E402
import train_random_ref as R  # noqa: E402
import train_stretch_ref as S  # noqa: E402
from test_gpu_train_random import EPOCHS, MIN_PREFIX  # noqa: E402

f32, f64 = np.float32, np.float64
# restated from csrc/ofp_seq_train.h, csrc/ofp_rnn_train.hip and csrc/ofp_train_chain.h: rows per slab of the dense
# layers' weight gradient, rows per slab of the input projection's, samples per chunk of the Linear head, sequences per
# workgroup of the GRU at hidden 8
DENSE_SLAB, INPROJ_SLAB, HEAD_CHUNK, GRU_GROUP = 256, 2048, 64, 32
ANCHOR_EPOCHS = (0, 1, 5)


def cdiv(a, b):
    return -(-a // b)


# ---- the replay -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["rnn", "cnnrnn"])
def test_replay_without_dropout_is_the_recipe_of_the_trainers_own_test(kind):
    """p = 0 on one static batch: the curve of torch_epochs of the trainer's own GPU test, to the bit."""
    c = Q.CASES[Q.MAIN[kind]]
    m = Q.make_model(c, 0.0)
    x, y = Q.cpu_batches(c, 1, 1)[0], Q.labels(c)
    xt, yt = torch.from_numpy(x), torch.from_numpy(y)
    for dtype in (torch.float32, torch.float64):
        ours, _flat = Q.replay(kind, m, lambda e: x, y, 3, None, 0.0, dtype)
        want, _val = (GR if kind == "rnn" else GC).torch_epochs(m, xt, yt, xt[:4], yt[:4], 3, dtype)
        print(f"{kind} {dtype}: {ours.tolist()} against {want.tolist()}")
        assert np.array_equal(ours, want) and ours[2] < ours[0]


@pytest.mark.parametrize("name", ["rnn_p0.5_stretched", "rnn_three_layers", "rnn_one_layer", "cnnrnn_p0.5_stretched",
                                  "cnnrnn_bn_p0.5_stretched"])
def test_masked_forward_with_nothing_dropped_is_the_plain_forward(name):
    """At p = 1e-12 the threshold is 0 and float32(1 / (1 - p)) is 1: masks of ones.  The masked formulas (for the
    CNNRNN behind its conv stack, through the RNN's helper) then give the modules' own forward; at p = 0.5 another."""
    c = Q.CASES[name]
    net = copy.deepcopy(Q.make_model(c)).double().train()
    net.attention.dropout = 0.0  # the plain forward runs torch's module, whose own dropout must stay off
    if c.kind == "rnn":
        net.rnn.dropout = 0.0
    x = torch.from_numpy(Q.cpu_batches(c, 1, 1)[0]).double()
    assert R.threshold(1e-12) == 0 and R.scale(1e-12) == f32(1)
    with torch.no_grad():
        plain = Q.forward(c.kind, net, x, 5, 2, 0.0).numpy()
        ones = Q.forward(c.kind, net, x, 5, 2, 1e-12).numpy()
        half = Q.forward(c.kind, net, x, 5, 2, 0.5).numpy()
        again = Q.forward(c.kind, net, x, 5, 3, 0.5).numpy()
    err, top = float(np.max(np.abs(ones - plain))), float(np.max(np.abs(plain)))
    print(f"{name}: max |masked with ones - plain| {err:.3e} of {top:.3e}; at p = 0.5 {np.max(np.abs(half - plain)):.3e}")
    assert err <= 1e-12 * top
    assert np.max(np.abs(half - plain)) > 1e-3 * top and not np.array_equal(half, again)


# ---- the comparable prefix ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", Q.TRAJ)
def test_comparable_prefix(name):
    torch.set_num_threads(1)
    c = Q.CASES[name]
    ref = Q.replays(c.kind, Q.make_model(c), Q.cpu_batches(c, Q.SEED, EPOCHS), Q.labels(c), Q.SEED, c.p)
    prefix, spread = R.comparable_prefix(ref["ref32"], ref["pert"])
    print(f"{name}: comparable prefix {prefix} of {EPOCHS}; loss {ref['ref32'][0]:.6g} -> {ref['ref32'][-1]:.6g}; "
          f"largest spread / loss {np.max(spread / ref['ref32']):.3e}")
    assert ref["pert"].shape == (8, EPOCHS) and np.isfinite(ref["ref64"]).all()
    assert prefix >= MIN_PREFIX
    assert ref["ref32"][-1] < ref["ref32"][0]
    assert np.any(ref["pert"] != ref["ref32"][None, :]), "the disturbed replays are the replay itself"


# ---- the draws ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("onsets", sorted({c.onsets for c in Q.CASES.values()}))
def test_stretch_draws(onsets):
    n = onsets * Q.REPS
    per_epoch = {e: S.draws(Q.SEED, e, n, Q.MAX_SHIFT, Q.SPAN) for e in range(EPOCHS)}
    for what, epochs in (("the anchor's epochs", ANCHOR_EPOCHS), ("the trajectory's epochs", range(EPOCHS))):
        stretches = {int(v) for e in epochs for v in per_epoch[e][1]}
        shifts = {int(v) for e in epochs for v in per_epoch[e][0]}
        print(f"{n} items, {what}: stretches {sorted(stretches)}, shifts {sorted(shifts)}")
        assert stretches == {-2, -1, 1, 2}
        assert shifts == set(range(-Q.MAX_SHIFT, Q.MAX_SHIFT + 1))
    for a, b in ((0, 1), (1, 5)):
        assert not np.array_equal(per_epoch[a][0], per_epoch[b][0])
        assert not np.array_equal(per_epoch[a][1], per_epoch[b][1])


# ---- the case tables ------------------------------------------------------------------------------------------------
def test_case_tables_cross_the_edges():
    from onset_fingerprinting_amd import model
    cases = Q.CASES
    for kind in ("rnn", "cnnrnn"):
        mine = {k: c for k, c in cases.items() if c.kind == kind}
        traj = [c for c in mine.values() if c.traj]
        assert sorted((c.p, c.source) for c in traj) == [(0.1, "shifted"), (0.1, "stretched"), (0.5, "shifted"),
                                                         (0.5, "stretched")]
        assert all((c.channels, c.width, c.onsets) == (3, 32, Q.ONSETS) for c in traj)
        edges = [c for c in mine.values() if not c.traj]
        assert all((c.p, c.source) == (0.5, "stretched") for c in edges)
        assert {c.channels for c in mine.values()} == {1, 3, 8}
        assert Q.CASES[Q.MAIN[kind]].p == 0.5 and Q.CASES[Q.MAIN[kind]].source == "stretched"
    assert model.RNN_TRAIN_MAX_CHANNELS == 8
    assert {c.kw.get("num_layers", 2) for c in cases.values() if c.kind == "rnn"} == {1, 2, 3}
    assert {bool(c.kw.get("batch_norm")) for c in cases.values() if c.kind == "cnnrnn" and c.traj} == {False, True}
    w31 = cases["rnn_width_31"]
    assert w31.width % 2 == 1 and w31.width % 4 != 0
    assert {int(c.width * Q.MAX_STRETCH) for c in cases.values()} == {Q.SPAN} and Q.SPAN == 3

    # the usual batch stays inside one head chunk and one input-projection slab ...
    n = Q.ONSETS * Q.REPS
    assert n == 42 and cdiv(n, HEAD_CHUNK) == 1 and cdiv(n * 32, INPROJ_SLAB) == 1
    # ... the large one crosses all four
    big, cbig = cases["rnn_66_windows"], cases["cnnrnn_66_windows"]
    n = big.onsets * Q.REPS
    rows = n * Q.steps_of(big)
    assert (n, rows) == (66, 2112) and cbig.onsets == big.onsets
    assert cdiv(n, HEAD_CHUNK) == 2 and cdiv(n, GRU_GROUP) == 3
    assert cdiv(rows, DENSE_SLAB) == 9 and cdiv(rows, INPROJ_SLAB) == 2
    assert Q.steps_of(cbig) == 6 and cdiv(n * 6, DENSE_SLAB) == 2
    # the validation batch is the larger one, and past one head chunk itself
    assert Q.N_VAL == 70 > Q.ONSETS * Q.REPS and cdiv(Q.N_VAL, HEAD_CHUNK) == 2

    # every case is a model the trainer takes, with the GRU's time steps the table counts rows by
    for name, c in cases.items():
        m = Q.make_model(c)
        if c.kind == "rnn":
            cfg = model._rnn_arch(m, seed=Q.SEED)
            assert (cfg.channels, cfg.hidden, cfg.heads, cfg.permute_input) == (c.channels, 8, 2, 1), name
            assert 256 // cfg.hidden == GRU_GROUP
        else:
            cfg, convs, bns = model._cnnrnn_arch(m, c.width, seed=Q.SEED)
            assert (cfg.cnn.channels[0], cfg.hidden, convs[-1].out_channels) == (c.channels, 8, Q.steps_of(c)), name
            assert bool(bns) == bool(c.kw.get("batch_norm")) and 256 // cfg.hidden == GRU_GROUP
        audio, onsets, y = Q.hits(c)
        assert audio.shape[1] == c.channels and y.shape == (c.onsets, 2)
        # room for the longest, furthest shifted window of the last hit
        assert onsets.min(1).max() - Q.PRE + Q.MAX_SHIFT + c.width + Q.SPAN - 1 <= len(audio), name
        assert onsets.min(1).min() - Q.PRE - Q.MAX_SHIFT >= 0, name
