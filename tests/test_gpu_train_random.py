"""GPU: the trainers' random stream (csrc/ofp_train_random.h): dropout in front of the Linear head and per-epoch shift
augmentation inside the epoch graph of model.fit_cnn / model.fit_lcccnn, against tests/train_random_ref.py.

  stream        ofp_philox4x32, the dropout mask and the shifted windows are bitwise equal to the numpy reference;
                outputs go into NaN-filled buffers with a guard tail
  gradients     under a mask, per tensor max |ours - g64| <= max(4 x max |g32 - g64|, 2^-23 x max |g64|) against torch
                autograd on the CPU with the reference mask multiplied in before fc; the loss within 2 n 2^-24 relative
  trajectories  against a CPU torch replay of the same recipe with the reference's masks and shifts, in float64, in
                float32 and as eight float32 runs with one input value moved by one ulp: over the comparable prefix
                (the disturbed runs within 1e-5 relative) |ours - ref32| <= max(4 x running max of (spread, |ref32 -
                ref64|), 2^-22 x loss); where the whole run is comparable the end parameters agree within max(4 x
                spread, 2^-23 x max |p|).  The prefix must be at least 24 epochs.
  the epoch     graph and plain launches give the same bits, so do two runs with one seed; two seeds differ
  off           p = 0 and an unshifted window source give the bits of a fit without them
Batches: 21 windows (n F is then no multiple of 4 at the widths used); a window source of 21 onsets and 2 extractions
gives 42.  Every figure is printed before it is asserted (run with -s to see them)."""
import copy
import ctypes
import sys
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

sys.path.insert(0, str(Path(__file__).resolve().parent))
import train_random_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

U24, U23, U22, U20 = 2.0 ** -24, 2.0 ** -23, 2.0 ** -22, 2.0 ** -20
GUARD = 64
f32, f64 = np.float32, np.float64
N = 21
EPOCHS = 40
MIN_PREFIX = 24


def guarded(shape, dtype=torch.float32):
    numel = int(np.prod(shape))
    if dtype == torch.float32:
        buf = torch.full((numel + GUARD,), float("nan"), dtype=dtype, device="cuda")
    else:
        buf = torch.full((numel + GUARD,), -12345, dtype=dtype, device="cuda")
    return buf[:numel].view(*shape), buf


def guard_intact(buf):
    tail = buf[-GUARD:]
    return bool(torch.isnan(tail).all()) if buf.dtype == torch.float32 else bool((tail == -12345).all())


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


# ---- 1. the generator -----------------------------------------------------------------------------------------------
def test_generator():
    from onset_fingerprinting_amd import _lib
    from onset_fingerprinting_amd._lib import check
    rng = np.random.default_rng(1)
    counters = np.concatenate([np.array([k[0] for k in R.KNOWN], np.uint32),
                               rng.integers(0, 2 ** 32, (4096, 4), dtype=np.uint64).astype(np.uint32)])
    keys = np.concatenate([np.array([k[1] for k in R.KNOWN], np.uint32),
                           rng.integers(0, 2 ** 32, (4096, 2), dtype=np.uint64).astype(np.uint32)])
    n = len(counters)
    out, buf = guarded((n, 4), torch.int32)
    c = torch.from_numpy(counters.view(np.int32)).cuda()
    k = torch.from_numpy(keys.view(np.int32)).cuda()
    check(_lib.lib().ofp_philox4x32(c.data_ptr(), k.data_ptr(), n, out.data_ptr(), stream()), "ofp_philox4x32")
    torch.cuda.synchronize()
    got = out.cpu().numpy().view(np.uint32)
    assert guard_intact(buf)
    for i, (_c, _k, words) in enumerate(R.KNOWN):
        assert tuple(int(w) for w in got[i]) == words, (i, [hex(int(w)) for w in got[i]])
    assert np.array_equal(got, R.philox4x32(counters, keys))


# ---- 2. the mask ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1), (3, 5), (7, 65), (21, 186), (2, 2049)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_mask(shape):
    from onset_fingerprinting_amd import model
    n, F_ = shape
    for p in (0.1, 0.5, 0.999):
        for epoch in (0, 1, 257):
            for seed in (0, 1, 2 ** 63 + 5):
                out, buf = guarded((n, F_))
                got = model.dropout_mask_device(seed, epoch, n, F_, p, out=out)
                torch.cuda.synchronize()
                assert got.data_ptr() == out.data_ptr() and guard_intact(buf), (p, epoch, seed)
                ref = R.dropout_mask(seed, epoch, n, F_, p)
                assert np.array_equal(got.cpu().numpy().view(np.uint32), ref.view(np.uint32)), (p, epoch, seed)


def test_mask_at_an_unaligned_address():
    """A mask that starts 4 bytes past a 16-byte boundary takes the single-element path: the same values."""
    from onset_fingerprinting_amd import model
    n, F_ = 7, 65
    buf = torch.full((1 + n * F_ + GUARD,), float("nan"), dtype=torch.float32, device="cuda")
    out = buf[1:1 + n * F_].view(n, F_)
    assert out.data_ptr() % 16 == 4
    model.dropout_mask_device(3, 2, n, F_, 0.5, out=out)
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf[0])) and guard_intact(buf)
    assert np.array_equal(out.cpu().numpy().view(np.uint32), R.dropout_mask(3, 2, n, F_, 0.5).view(np.uint32))


# ---- 3. the windows -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [1, 3, 4, 5])
@pytest.mark.parametrize("W", [1, 31, 256])
def test_windows(C, W):
    from onset_fingerprinting_amd import _lib
    from onset_fingerprinting_amd._lib import check
    rng = np.random.default_rng([C, W])
    O = 9
    for m in (0, 1, 16):
        for reps in (1, 3):
            gap = W + 2 * m + 3
            audio = rng.standard_normal((gap * (O + 1), C)).astype(f32)
            starts = (m + gap * np.arange(O) + rng.integers(0, 3, O)).astype(np.int64)
            seed, epoch = 77 + m, 3 * reps
            n = O * reps
            (win, bw), (sh, bs) = guarded((n, C, W)), guarded((n,), torch.int32)
            a, s = torch.from_numpy(audio).cuda(), torch.from_numpy(starts).cuda()
            check(_lib.lib().ofp_shift_windows(seed, epoch, a.data_ptr(), audio.shape[0], C, s.data_ptr(), O, reps, m, W,
                                               sh.data_ptr(), win.data_ptr(), stream()), "ofp_shift_windows")
            torch.cuda.synchronize()
            assert guard_intact(bw) and guard_intact(bs), (m, reps)
            ref_sh, ref_win = R.shifted_windows(audio, starts, W, seed, epoch, m, reps)
            assert np.array_equal(sh.cpu().numpy(), ref_sh), (m, reps)
            assert np.array_equal(win.cpu().numpy().view(np.uint32), ref_win.view(np.uint32)), (m, reps)


def test_shifted_windows_class():
    from onset_fingerprinting_amd import data
    audio, onsets, _y = R.synthetic_hits(4, 6, 3, 31, 16)
    src = data.ShiftedWindows(audio, onsets, 31, pre_samples=2, max_shift=16, n_extractions=3)
    assert (src.n, src.n_onsets, src.channels) == (18, 6, 3)
    ref_sh, ref_win = R.shifted_windows(audio, onsets.min(1) - 2, 31, 9, 5, 16, 3)
    assert np.array_equal(src.shifts(9, 5).cpu().numpy(), ref_sh)
    assert np.array_equal(src.windows(9, 5).cpu().numpy(), ref_win)
    one = data.ShiftedWindows(audio[:, 0], onsets[:, 0], 31, max_shift=1)
    assert tuple(one.windows(1, 0).shape) == (6, 31)
    with pytest.raises(ValueError, match="seed"):
        src.windows()
    with pytest.raises(IndexError):
        data.ShiftedWindows(audio, onsets, 31, pre_samples=int(onsets.min()) - 15, max_shift=16)


# ---- models and data ------------------------------------------------------------------------------------------------
def cnn_model(p, **kw):
    from onset_fingerprinting_amd import model
    torch.manual_seed(5)
    args = dict(layer_sizes=[5, 6], kernel_size=3, padding=1, lr=0.003)
    args.update(kw)
    return model.CNN(31, 2, channels=3, dropout_rate=p, **args)  # F = 6 * 31 = 186 (42 with the pool)


def lcccnn_model(p, **kw):
    """GroupNorm's initial weights are scaled by 0.2 so that the head's softmax is not saturated (asserted where it
    matters), as tests/test_gpu_cccnn_train.py does."""
    from onset_fingerprinting_amd import model
    torch.manual_seed(6)
    args = dict(layer_sizes=[3, 2], batch_norm=True, lr=0.001)
    args.update(kw)
    m = model.LCCCNN(31, 2, channels=3, dropout_rate=p, **args)  # F = 3 * 61 = 183
    with torch.no_grad():
        for mod in m.model.conv_layers:
            if isinstance(mod, nn.GroupNorm):
                mod.weight.mul_(0.2)
    return m


MODELS = {
    "cnn_plain": lambda p: cnn_model(p),
    "cnn_bn": lambda p: cnn_model(p, batch_norm=True),
    "cnn_pool": lambda p: cnn_model(p, pool=True),
    "lcccnn_shared": lambda p: lcccnn_model(p, group=False),
    "lcccnn_grouped": lambda p: lcccnn_model(p, group=True),
}


def is_cnn(name):
    return name.startswith("cnn")


def hits(max_shift=3):
    return R.synthetic_hits(8, N, 3, 31, max_shift)


def static_batch():
    audio, onsets, y = hits()
    return R.shifted_windows(audio, onsets.min(1) - 2, 31, 0, 0, 0, 1)[1], y


def gradient_batch():
    """Normal deviates for x and y, as the gradient tests of tests/test_gpu_cnn_train.py and
    tests/test_gpu_cccnn_train.py draw them: the rule compares with torch's own float32 error, which says something
    only where every tensor's gradient is well above the rounding of the values it is summed from.  (On the windows of
    synthetic_hits one tensor of one case, bn1.bias of lcccnn_shared at p = 0.5, a sum of 8e-3 at most, missed it with
    1.17e-9 against 4 x torch's 2.4e-10 while torch's own error of the same tensor at p = 0.1 was 1.6e-9.)"""
    gen = torch.Generator().manual_seed(21)
    return torch.randn(N, 3, 31, generator=gen), torch.randn(N, 2, generator=gen)


# ---- 4. gradients under a mask --------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("name", list(MODELS))
def test_gradients_under_a_mask(name, p):
    from onset_fingerprinting_amd import model
    m = MODELS[name](p)
    x, y = gradient_batch()
    seed, epoch = 1234567, 3
    feats, nfeat = R.features_of(m), R.head_of(m).in_features
    assert (N * nfeat) % 4 != 0
    mask = R.dropout_mask(seed, epoch, N, nfeat, p)
    ref = {}
    for dtype in (torch.float32, torch.float64):
        net = copy.deepcopy(m).to(dtype).train()
        h = feats(net, x.to(dtype))
        if not is_cnn(name) and dtype == torch.float64:
            print(f"{name}: largest p of the head {float(h.detach().max()):.4f}")
            assert float(h.detach().max()) < 0.9, "the softmax of the head is saturated"
        v = m.loss(R.head_of(net)(h * torch.from_numpy(mask).to(dtype)), y.to(dtype))
        v.backward()
        ref[dtype] = ({k: q.grad.numpy() for k, q in net.named_parameters()}, float(v.detach()))
    fn = model.cnn_loss_and_grads_device if is_cnn(name) else model.cccnn_loss_and_grads_device
    loss, grads = fn(m, x.cuda(), y.cuda(), seed=seed, epoch=epoch)
    (g32, _l32), (g64, loss64) = ref[torch.float32], ref[torch.float64]
    assert sorted(grads) == sorted(g64)
    label = f"{name} p={p}"
    for k, r64 in g64.items():
        mine = grads[k].detach().cpu().numpy().astype(f64)
        r64 = r64.astype(f64)
        err, err32 = np.max(np.abs(mine - r64)), np.max(np.abs(g32[k].astype(f64) - r64))
        bound = max(4 * err32, U23 * np.max(np.abs(r64)))
        print(f"{label} {k}: |ours - g64| {err:.3e}  |g32 - g64| {err32:.3e}  bound {bound:.3e}")
        assert err <= bound, (label, k, err, bound)
    rel = abs(float(loss) - loss64) / loss64
    print(f"{label} loss: ours {float(loss):.9g} ref64 {loss64:.9g} rel {rel:.3e} bound {2 * N * U24:.3e}")
    assert rel <= 2 * N * U24
    # another epoch is another mask: another loss
    loss1, _g = fn(m, x.cuda(), y.cuda(), seed=seed, epoch=epoch + 1)
    assert float(loss1) != float(loss)


# ---- 5. trajectories ------------------------------------------------------------------------------------------------
# what is trained: MSE + Tanh is the smooth case the comparable prefix was checked on; L1 + SiLU + BatchNorm the
# reference's own kind of network
TRAJ = {
    "cnn_mse_tanh_p0.1": ("cnn", 0.1, dict(loss=F.mse_loss, activation=nn.Tanh)),
    "cnn_l1_silu_bn_p0.5": ("cnn", 0.5, dict(loss=F.l1_loss, activation=nn.SiLU, batch_norm=True)),
    "lcccnn_mse_tanh_p0.1": ("lcccnn", 0.1, dict(loss=F.mse_loss, activation=nn.Tanh, group=False)),
    "lcccnn_grouped_mse_tanh_p0.5": ("lcccnn", 0.5, dict(loss=F.mse_loss, activation=nn.Tanh, group=True)),
}
TRAJ_SEED = 2024


def traj_setup(case, shifted):
    """-> (module, fit arguments (x or source, y), replay arguments)."""
    from onset_fingerprinting_amd import data
    kind, p, kw = TRAJ[case]
    m = (cnn_model if kind == "cnn" else lcccnn_model)(p, **kw)
    audio, onsets, y = hits()
    starts = onsets.min(1) - 2
    if shifted:
        src = data.ShiftedWindows(audio, onsets, 31, pre_samples=2, max_shift=3, n_extractions=2)
        return m, p, (src, torch.from_numpy(y)), dict(data=audio, y=np.tile(y, (2, 1)), source=(starts, 31, 3, 2))
    x = R.shifted_windows(audio, starts, 31, 0, 0, 0, 1)[1]
    return m, p, (torch.from_numpy(x), torch.from_numpy(y)), dict(data=x, y=y, source=None)


def traj_reference(case, shifted):
    m, p, _fit, rep = traj_setup(case, shifted)
    return R.replays(m, rep["data"], rep["y"], EPOCHS, TRAJ_SEED, p, rep["source"])


@pytest.mark.parametrize("shifted", [False, True], ids=["dropout", "dropout_and_shifts"])
@pytest.mark.parametrize("case", list(TRAJ))
def test_trajectory_over_the_comparable_prefix(case, shifted):
    from onset_fingerprinting_amd import model
    torch.set_num_threads(1)
    ref = traj_reference(case, shifted)
    ref32, ref64 = ref["ref32"], ref["ref64"]
    prefix, spread = R.comparable_prefix(ref32, ref["pert"])
    print(f"{case}: comparable prefix {prefix} of {EPOCHS}; loss {ref32[0]:.6g} -> {ref32[-1]:.6g}")
    assert prefix >= MIN_PREFIX
    m, _p, (x, y), _rep = traj_setup(case, shifted)
    m = m.cuda()
    fit = (model.fit_cnn if TRAJ[case][0] == "cnn" else model.fit_lcccnn)(
        m, x if shifted else x.cuda(), y.cuda(), max_epochs=EPOCHS, seed=TRAJ_SEED)
    ours = fit.train_loss.cpu().numpy().astype(f64)
    assert fit.epochs == EPOCHS and fit.seed == TRAJ_SEED and np.isfinite(ours).all()
    own = np.maximum(spread[:prefix], np.abs(ref32[:prefix] - ref64[:prefix]))
    bound = np.maximum(4 * np.maximum.accumulate(own), U22 * ref32[:prefix])
    diff = np.abs(ours[:prefix] - ref32[:prefix].astype(f32).astype(f64))
    worst = int(np.argmax(diff / bound))
    print(f"{case}: worst epoch {worst}: |ours - ref32| {diff[worst]:.3e} bound {bound[worst]:.3e} (spread "
          f"{spread[worst]:.3e}, |ref32 - ref64| {abs(ref32[worst] - ref64[worst]):.3e}, loss {ref32[worst]:.6g}); "
          f"last epoch of the prefix: {diff[prefix - 1]:.3e} against {bound[prefix - 1]:.3e}")
    assert np.all(diff <= bound), (case, worst, diff[worst], bound[worst])
    if prefix == EPOCHS:
        mine = torch.cat([q.detach().reshape(-1) for q in m.parameters()]).cpu().numpy().astype(f64)
        rec = ref["flat"]
        sp = np.max(np.abs(rec[1:] - rec[0]))
        err = np.max(np.abs(mine - rec[0]))
        b = max(4 * sp, U23 * np.max(np.abs(rec[0])))
        print(f"{case}: parameters max |ours - ref32| {err:.3e}, spread of the disturbed runs {sp:.3e}, bound {b:.3e}")
        assert err <= b, (err, b)


# ---- 6. the epoch reaches the stream --------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["cnn", "lcccnn"])
def test_the_epoch_reaches_the_stream(kind, monkeypatch):
    from onset_fingerprinting_amd import model
    case = "cnn_l1_silu_bn_p0.5" if kind == "cnn" else "lcccnn_grouped_mse_tanh_p0.5"
    fit_fn = model.fit_cnn if kind == "cnn" else model.fit_lcccnn
    env = "OFP_CNN_GRAPH" if kind == "cnn" else "OFP_CCCNN_GRAPH"

    def run(seed, mode=None):
        if mode:
            monkeypatch.setenv(env, mode)
        m, _p, (src, y), _rep = traj_setup(case, True)
        m = m.cuda()
        fit = fit_fn(m, src, y.cuda(), max_epochs=12, seed=seed)
        monkeypatch.delenv(env, raising=False)
        return fit.train_loss, torch.cat([t.detach().reshape(-1).float() for t in m.state_dict().values()])

    (la, pa), (lb, pb), (lc, pc), (ld, _pd) = run(7), run(7), run(7, "nodes"), run(8)
    assert bool(torch.isfinite(la).all())
    assert torch.equal(la.view(torch.int32), lb.view(torch.int32)) and torch.equal(pa, pb)
    assert torch.equal(la.view(torch.int32), lc.view(torch.int32)) and torch.equal(pa, pc)
    assert float(la[0]) != float(ld[0]), "two seeds gave the same first loss"
    nfeat = R.head_of(traj_setup(case, False)[0]).in_features
    m0, m1 = (model.dropout_mask_device(7, e, 2 * N, nfeat, 0.5) for e in (0, 1))
    assert not torch.equal(m0, m1)


# ---- 7. off means off -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["cnn", "lcccnn"])
def test_off_means_off(kind):
    from onset_fingerprinting_amd import data, model
    fit_fn = model.fit_cnn if kind == "cnn" else model.fit_lcccnn
    make = (lambda: cnn_model(0.0, batch_norm=True)) if kind == "cnn" else (lambda: lcccnn_model(0.0))
    audio, onsets, y = hits()
    frames = data.FastFrameExtractor(audio, onsets, 31, 2, device=0).frames
    y = torch.from_numpy(y).cuda()

    def run(x, **kw):
        m = make().cuda()
        fit = fit_fn(m, x, y, max_epochs=10, **kw)
        return fit.train_loss, torch.cat([t.detach().reshape(-1).float() for t in m.state_dict().values()])

    base_l, base_p = run(frames)
    assert bool(torch.isfinite(base_l).all())
    source = data.ShiftedWindows(audio, onsets, 31, pre_samples=2, max_shift=0, n_extractions=1)
    for what, (l, q) in (("p = 0 with a seed", run(frames, seed=9)), ("p = 0 without a seed", run(frames, seed=None)),
                         ("unshifted windows", run(source)), ("unshifted windows and a seed", run(source, seed=9))):
        assert torch.equal(l.view(torch.int32), base_l.view(torch.int32)) and torch.equal(q, base_p), what


# ---- 8. validation is eval ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["cnn", "lcccnn"])
def test_validation_is_eval(kind):
    from onset_fingerprinting_amd import model
    case = "cnn_l1_silu_bn_p0.5" if kind == "cnn" else "lcccnn_grouped_mse_tanh_p0.5"
    m, _p, (src, y), _rep = traj_setup(case, True)
    m = m.cuda()
    xv, yv = static_batch()
    xv, yv = torch.from_numpy(xv[:8]).cuda(), torch.from_numpy(yv[:8]).cuda()
    fit = (model.fit_cnn if kind == "cnn" else model.fit_lcccnn)(m, src, y.cuda(), x_val=xv, y_val=yv, max_epochs=10,
                                                                 seed=3)
    assert fit.epochs == 10 and not m.training
    with torch.no_grad():
        again = float(F.l1_loss(m(xv), yv))
    last = float(fit.val_loss[fit.epochs - 1])
    rel = abs(again - last) / abs(again)
    print(f"{kind}: last validation loss {last:.9g}, forward of the trained module {again:.9g}, rel {rel:.3e}, bound "
          f"{U20:.3e}")
    assert rel <= U20
