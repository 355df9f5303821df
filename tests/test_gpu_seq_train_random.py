"""GPU: the two sequence trainers (model.fit_rnn, model.fit_cnnrnn; `kind`) under the trainers' random stream through
whole epochs -- window sources (sites 1 and 2) together with the dropout sites 0, 3 and 4 --, against
tests/seq_train_random_ref.py, whose table says what each case straddles.

  anchor        for every case and e in {0, 1, 5}: *_loss_and_grads_device(model after e epochs, src.windows(seed, e),
                y, seed=seed, epoch=e) is train_loss[e] of a fit of 6 epochs, bit for bit (fits are prefixes of each
                other, also asserted); and so that this cannot hold emptily: the windows of epochs 0 and 1 differ, the
                same quantity on epoch 0's windows or under epoch 0's masks is another loss, another seed another
                train_loss[0]
  trajectory    the rule and constants of test_gpu_train_random.py::test_trajectory_over_the_comparable_prefix against
                the CPU replay of the trainer's recipe on src.windows(seed, e) under the numpy masks: |ours - ref32| <=
                max(4 x running max(spread of eight float32 replays with one batch element moved by one ulp, |ref32 -
                ref64|), 2^-22 x loss) over the comparable prefix (at least MIN_PREFIX epochs); where that is all 40
                epochs the end parameters within max(4 x spread, 2^-23 x max |p|)
  the epoch     two fits as a replayed graph and one with OFP_RNN_GRAPH / OFP_CNNRNN_GRAPH = nodes (plain launches, in a
                fresh child process as the trainers' own determinism tests run them) give the same losses and state
  off           StretchedWindows(max_stretch=0) is the ShiftedWindows; ShiftedWindows(max_shift=0, n_extractions=1) is
                the tensor of its frames; p = 0 with a seed is p = 0 without: bit for bit on losses and state
  validation    with dropout and a validation batch larger than the training batch the last val_loss is the eval-mode
                L1 loss of the returned module: of its torch layers in float64 and of its own (inference) forward,
                within 2^-20 relative
The refusals of the two entries are in tests/test_gpu_train_stretch.py::test_refusals.  Every figure is printed before it
is asserted (run with -s to see them)."""
import copy
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, str(Path(__file__).resolve().parent))
import seq_train_random_ref as Q  # noqa: E402
import test_gpu_cnnrnn_train as GC  # noqa: E402  (helpers only; its tests are collected from its own file)
import test_gpu_rnn_train as GR  # noqa: E402
import test_gpu_train_random as T  # noqa: E402
import train_random_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

REPO = Path(__file__).resolve().parents[1]
U20, U22, U23 = T.U20, T.U22, T.U23
f32, f64 = np.float32, np.float64
KINDS = ["rnn", "cnnrnn"]
ENV = {"rnn": "OFP_RNN_GRAPH", "cnnrnn": "OFP_CNNRNN_GRAPH"}


def fit_fn(kind):
    from onset_fingerprinting_amd import model
    return model.fit_rnn if kind == "rnn" else model.fit_cnnrnn


def grads_fn(kind):
    from onset_fingerprinting_amd import model
    return model.rnn_loss_and_grads_device if kind == "rnn" else model.cnnrnn_loss_and_grads_device


def targets(c):
    """y of the case's onsets [O, 2] on the GPU; the fit tiles it over the extractions."""
    return torch.from_numpy(Q.hits(c)[2]).cuda()


def state_of(m):
    return torch.cat([t.detach().reshape(-1).float() for t in m.state_dict().values()])


def run_fit(c, x, epochs, p=None, **kw):
    """A fit of the case's module from its start state -> (module, record)."""
    m = Q.make_model(c, p).cuda()
    fit = fit_fn(c.kind)(m, x, targets(c), max_epochs=epochs, **kw)
    assert fit.epochs == epochs
    return m, fit


def same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


# ---- a. the epoch trains on that epoch's windows under that epoch's masks ------------------------------------------
@pytest.mark.parametrize("name", list(Q.CASES))
def test_the_epoch_trains_on_its_windows_under_its_masks(name):
    c = Q.CASES[name]
    seed, grads = Q.SEED, grads_fn(c.kind)
    src = Q.make_source(c)
    y = targets(c).repeat(Q.REPS, 1)
    assert (src.n, src.channels, src.frame_length) == (c.onsets * Q.REPS, c.channels, c.width)
    assert getattr(src, "stretch_span", 0) == (Q.SPAN if c.source == "stretched" else 0)
    _m6, long = run_fit(c, src, 6, seed=seed)
    curve = long.train_loss
    assert bool(torch.isfinite(curve).all())
    win = {e: src.windows(seed, e) for e in (0, 1, 5)}
    assert not torch.equal(win[0], win[1]), "epochs 0 and 1 cut the same windows"
    after = {0: Q.make_model(c).cuda()}
    for e in (1, 5):
        after[e], short = run_fit(c, src, e, seed=seed)
        assert same_bits(short.train_loss, curve[:e]), f"the fit of {e} epochs is no prefix of the fit of 6"
    for e in (0, 1, 5):
        loss, _g = grads(after[e], win[e], y, seed=seed, epoch=e)
        print(f"{name} epoch {e}: the fit's loss {float(curve[e]):.9g}, loss of the model after {e} epochs on "
              f"windows({seed}, {e}) under the masks of epoch {e} {float(loss):.9g}")
        assert float(loss) == float(curve[e]), (name, e)
    stale_windows, _g = grads(after[1], win[0], y, seed=seed, epoch=1)
    stale_masks, _g = grads(after[1], win[1], y, seed=seed, epoch=0)
    _m, other = run_fit(c, src, 1, seed=seed + 1)
    print(f"{name}: train_loss[1] {float(curve[1]):.9g}; on epoch 0's windows {float(stale_windows):.9g}, under epoch "
          f"0's masks {float(stale_masks):.9g}; train_loss[0] {float(curve[0]):.9g}, with seed {seed + 1} "
          f"{float(other.train_loss[0]):.9g}")
    assert float(stale_windows) != float(curve[1]), "epoch 1 trained on the windows of epoch 0"
    assert float(stale_masks) != float(curve[1]), "epoch 1 trained under the masks of epoch 0"
    assert float(other.train_loss[0]) != float(curve[0]), "two seeds gave the same first loss"


# ---- b. trajectory --------------------------------------------------------------------------------------------------
_refs = {}


def reference(name):
    """(the case's source, the replays on its batches); the replays once per case and session."""
    c = Q.CASES[name]
    src = Q.make_source(c)
    if name not in _refs:
        torch.set_num_threads(1)
        # the batches the epoch graph trains on, held to the resampler's bits by test_gpu_train_stretch.py
        batches = [src.windows(Q.SEED, e).cpu().numpy() for e in range(T.EPOCHS)]
        assert not np.array_equal(batches[0], batches[1])
        _refs[name] = Q.replays(c.kind, Q.make_model(c), batches, Q.labels(c), Q.SEED, c.p)
    return src, _refs[name]


@pytest.mark.parametrize("name", Q.TRAJ)
def test_trajectory_over_the_comparable_prefix(name):
    c = Q.CASES[name]
    src, ref = reference(name)
    ref32, ref64 = ref["ref32"], ref["ref64"]
    prefix, spread = R.comparable_prefix(ref32, ref["pert"])
    print(f"{name}: comparable prefix {prefix} of {T.EPOCHS}; loss {ref32[0]:.6g} -> {ref32[-1]:.6g}")
    assert prefix >= T.MIN_PREFIX
    m, fit = run_fit(c, src, T.EPOCHS, seed=Q.SEED)
    ours = fit.train_loss.cpu().numpy().astype(f64)
    assert fit.seed == Q.SEED and np.isfinite(ours).all()
    own = np.maximum(spread[:prefix], np.abs(ref32[:prefix] - ref64[:prefix]))
    bound = np.maximum(4 * np.maximum.accumulate(own), U22 * ref32[:prefix])
    diff = np.abs(ours[:prefix] - ref32[:prefix].astype(f32).astype(f64))
    worst = int(np.argmax(diff / bound))
    print(f"{name}: worst epoch {worst}: |ours - ref32| {diff[worst]:.3e} bound {bound[worst]:.3e} error / bound "
          f"{diff[worst] / bound[worst]:.3g} (spread {spread[worst]:.3e}, |ref32 - ref64| "
          f"{abs(ref32[worst] - ref64[worst]):.3e}, loss {ref32[worst]:.6g}); last epoch of the prefix: "
          f"{diff[prefix - 1]:.3e} against {bound[prefix - 1]:.3e}")
    assert np.all(diff <= bound), (name, worst, diff[worst], bound[worst])
    if prefix == T.EPOCHS:
        mine = torch.cat([q.detach().reshape(-1) for q in m.parameters()]).cpu().numpy().astype(f64)
        rec = ref["flat"]
        sp = np.max(np.abs(rec[1:] - rec[0]))
        err = np.max(np.abs(mine - rec[0]))
        b = max(4 * sp, U23 * np.max(np.abs(rec[0])))
        print(f"{name}: parameters max |ours - ref32| {err:.3e}, spread of the disturbed runs {sp:.3e}, bound {b:.3e} "
              f"error / bound {err / b:.3g}")
        assert err <= b, (err, b)


# ---- c. graph, plain launches, determinism --------------------------------------------------------------------------
def twelve_epochs(kind):
    """12 epochs at p = 0.5 from the stretched source -> (train_loss, state) as numpy."""
    c = Q.CASES[Q.MAIN[kind]]
    m, fit = run_fit(c, Q.make_source(c), 12, seed=7)
    return fit.train_loss.cpu().numpy(), state_of(m).cpu().numpy()


@pytest.mark.parametrize("kind", KINDS)
def test_two_fits_and_plain_launches_give_the_same_bits(kind, tmp_path):
    a, b = twelve_epochs(kind), twelve_epochs(kind)
    assert np.isfinite(a[0]).all()
    for u, v in zip(a, b):
        assert np.array_equal(u.view(np.uint32), v.view(np.uint32)), "two fits with one seed differ"
    out = tmp_path / "nodes.npz"
    code = ("import sys, numpy as np; sys.path[:0] = [sys.argv[1], sys.argv[2]]; import test_gpu_seq_train_random as t; "
            "tl, flat = t.twelve_epochs(sys.argv[4]); np.savez(sys.argv[3], tl=tl, flat=flat)")
    env = dict(os.environ)
    env[ENV[kind]] = "nodes"
    done = subprocess.run([sys.executable, "-c", code, str(REPO), str(REPO / "tests"), str(out), kind], env=env,
                          timeout=300, capture_output=True, text=True)
    assert done.returncode == 0, done.stderr[-2000:]
    nodes = np.load(out)
    for u, v in zip(a, (nodes["tl"], nodes["flat"])):
        assert np.array_equal(u.view(np.uint32), v.view(np.uint32)), "graph replay and plain launches differ"


# ---- d. off means off -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_off_means_off(kind):
    c = Q.CASES[Q.MAIN[kind]]
    audio, onsets, _y = Q.hits(c)

    def run(x, p, **kw):
        m, fit = run_fit(c, x, 10, p, **kw)
        return fit.train_loss, state_of(m)

    def same(what, got, want):
        assert same_bits(got[0], want[0]) and torch.equal(got[1], want[1]), (kind, what)

    # no stretch is the shifted source, without and with dropout
    for p in (0.0, 0.5):
        shifted = run(Q.make_source(c, "shifted"), p, seed=9)
        assert bool(torch.isfinite(shifted[0]).all())
        same(f"StretchedWindows(max_stretch=0) at p = {p}", run(Q.make_source(c, "stretched", max_stretch=0), p, seed=9),
             shifted)
    # no shift and one extraction is the tensor of the frames; p = 0 with a seed is p = 0 without
    frames = torch.from_numpy(R.shifted_windows(audio, onsets.min(1) - Q.PRE, c.width, 0, 0, 0, 1)[1]).cuda()
    base = run(frames, 0.0)
    assert bool(torch.isfinite(base[0]).all())
    still = Q.make_source(c, "shifted", max_shift=0, n_extractions=1)
    for what, got in (("p = 0 with a seed", run(frames, 0.0, seed=9)),
                      ("ShiftedWindows(max_shift=0, n_extractions=1)", run(still, 0.0)),
                      ("that source and a seed", run(still, 0.0, seed=9))):
        same(what, got, base)
    # and on is on: the same fit with p = 0.5 is another
    assert not same_bits(run(frames, 0.5, seed=9)[0], base[0])


# ---- e. validation is eval ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_validation_is_eval(kind):
    c = Q.CASES[Q.MAIN[kind]]
    va, vo, vy = R.synthetic_hits(9, Q.N_VAL, c.channels, c.width, 0)
    xv = torch.from_numpy(R.shifted_windows(va, vo.min(1) - Q.PRE, c.width, 0, 0, 0, 1)[1])
    yv = torch.from_numpy(vy)
    src = Q.make_source(c)
    assert len(xv) == Q.N_VAL > src.n
    m, fit = run_fit(c, src, 10, seed=3, x_val=xv.cuda(), y_val=yv.cuda())
    assert not m.training and bool(torch.isfinite(fit.val_loss).all())
    last = float(fit.val_loss[fit.epochs - 1])
    net = copy.deepcopy(m).cpu().double().eval()
    with torch.no_grad():
        layers = float(F.l1_loss((GR if kind == "rnn" else GC).torch_forward(net, xv.double()), yv.double()))
        own = float(F.l1_loss(m(xv.cuda()), yv.cuda()))
    for what, again in (("its torch layers in float64", layers), ("its own forward", own)):
        rel = abs(again - last) / abs(again)
        print(f"{kind}: last validation loss {last:.9g}, eval-mode L1 of the trained module by {what} {again:.9g}, rel "
              f"{rel:.3e}, bound {U20:.3e}, error / bound {rel / U20:.3g}")
        assert rel <= U20, (kind, what)
