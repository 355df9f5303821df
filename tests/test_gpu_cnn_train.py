"""GPU: training model.CNN (csrc/ofp_cnn_train.hip, model.fit_cnn) against float64 references and the reference's
recorded runs (tests/golden/g26_cnn_train.npz, made by make_golden_cnn_train.py).

  kernels     the convolution's three gradients, BatchNorm in training mode, the Linear head with its loss (forward
              and backward, on both sides of its chunk of 64 samples and its 256-thread strides) and the NAdam step,
              called directly, element-wise against float64 with the derived bounds of tests/cnn_train_ref.py;
              outputs go into NaN-filled buffers with a guard tail
  gradients   per tensor, max |ours - g64| <= 4 x max |g32 - g64|, floored at 2^-23 x max |g64|; up to the limit of
              1 024 windows, so that whole chains cross slabs and chunks
  epoch       with more validation than training windows: the first losses against the start and against torch in
              float64, graph and plain launches bit for bit
  trajectory  over the comparable prefix (the epochs before the 8 disturbed reference curves first stray more than
              1e-5 relative): |ours_e - ref_e| <= 4 x the largest, up to e, of the disturbed runs' spread and of
              |ref32 - ref64|, floored at 2^-22 x loss_e
  outcome     of the chaotic cases: final and best loss at most the largest of the nine reference runs plus the width
              of their range (not less than the curve's own wobble)
Every figure is printed before it is asserted (run with -s to see them)."""
import copy
import json
import sys
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

sys.path.insert(0, str(Path(__file__).resolve().parent))
import cnn_train_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = ["l1_silu_bn", "l1_silu_pool", "mse_tanh_dil_bn"]
STOP = "l1_silu_bn_stop"
U24, U23, U22, U20 = 2.0 ** -24, 2.0 ** -23, 2.0 ** -22, 2.0 ** -20
GUARD = 64
f32, f64 = np.float32, np.float64


@pytest.fixture(scope="module")
def g(golden):
    return golden("g26_cnn_train")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, f32)).cuda()


def guarded(*shape):
    numel = int(np.prod(shape))
    buf = torch.full((numel + GUARD,), float("nan"), dtype=torch.float32, device="cuda")
    return buf[:numel].view(*shape), buf


def within(name, got, ref, bound, ctx, buf=None):
    """Element-wise |got - ref| <= bound (NaN fails); the guard tail behind the output is untouched."""
    if buf is not None:
        assert bool(torch.isnan(buf[-GUARD:]).all()), (name, ctx, "store past the end of the output")
    got = got.detach().cpu().numpy().astype(f64)
    assert got.shape == ref.shape, (name, ctx, got.shape, ref.shape)
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = float(np.max(np.where(np.isnan(err) | ((bound == 0) & (err > 0)), np.inf,
                                      np.where(bound > 0, err / bound, 0.0)))) if err.size else 0.0
    print(f"{ctx} {name}: largest error / bound {ratio:.3g}, largest error {float(np.nanmax(err)) if err.size else 0:.3e}")
    assert bool((err <= bound).all()), (name, ctx, f"error / bound = {ratio:.3g}")


def load_case(g, case):
    from onset_fingerprinting_amd import model
    cfg = json.loads(str(g[f"{case}/cfg"]))
    kw = dict(cfg["kwargs"])
    kw["activation"], kw["loss"] = getattr(nn, kw["activation"]), getattr(F, kw["loss"])
    m = model.CNN(cfg["width"], 2, channels=cfg["channels"], dropout_rate=0.0, lr=cfg["lr"], **kw)
    pre = f"{case}/sd0/"
    m.load_state_dict({k[len(pre):]: torch.from_numpy(g[k]) for k in g.files if k.startswith(pre)})
    x, y = torch.from_numpy(g[f"{case}/x"]), torch.from_numpy(g[f"{case}/y"])
    val = (torch.from_numpy(g[f"{case}/x_val"]), torch.from_numpy(g[f"{case}/y_val"])) if "n_val" in cfg else None
    return cfg, m, x, y, val


_runs = {}


def our_run(g, case):
    """fit_cnn on the golden's inputs and start, on the GPU; once per case and session."""
    from onset_fingerprinting_amd import model
    if case not in _runs:
        cfg, m, x, y, val = load_case(g, case)
        m = m.cuda()
        kw = dict(x_val=val[0].cuda(), y_val=val[1].cuda(), patience=cfg["patience"]) if val else {}
        fit = model.fit_cnn(m, x.cuda(), y.cuda(), max_epochs=cfg["epochs"], **kw)
        _runs[case] = (m, fit)
    return _runs[case]


def comparable_prefix(ref, pert):
    n = len(ref)
    with np.errstate(invalid="ignore"):
        spread = np.max(np.abs(pert[:, :n].astype(f64) - ref.astype(f64)), axis=0)
    bad = np.isnan(spread) | (spread > 1e-5 * ref)
    return (int(np.argmax(bad)) if bad.any() else n), spread


# ---- the convolution's gradients ------------------------------------------------------------------------------------
# (k, dilation, padding, groups, cin, cout, width, n)
CONV_CASES = [
    (1, 1, 0, 1, 5, 6, 1, 3), (1, 1, 0, 1, 6, 5, 7, 2), (2, 1, 0, 1, 5, 6, 2, 3), (2, 2, 1, 2, 6, 4, 7, 3),
    (2, 3, 1, 1, 5, 6, 64, 2), (3, 1, 0, 1, 5, 6, 7, 3), (3, 1, 1, 1, 6, 5, 1, 4), (3, 1, 2, 2, 6, 10, 2, 3),
    (3, 2, 1, 6, 6, 12, 64, 2), (3, 3, 2, 1, 5, 6, 7, 3), (3, 3, 1, 1, 5, 6, 257, 2), (5, 1, 0, 1, 6, 5, 7, 3),
    (5, 1, 2, 2, 6, 4, 64, 3), (5, 1, 4, 6, 6, 6, 2, 3), (5, 2, 2, 1, 5, 6, 257, 2), (5, 3, 4, 1, 5, 6, 64, 2),
    (5, 2, 4, 3, 6, 6, 7, 5),
]


def check_conv_backward(k, dil, pad, groups, cin, cout, w, n, need_dx=True):
    from onset_fingerprinting_amd import model
    wc = w + 2 * pad - dil * (k - 1)
    assert wc >= 1
    rng = np.random.default_rng([k, dil, pad, groups, cin, cout, w, n])
    x = rng.standard_normal((n, cin, w)).astype(f32)
    wt = rng.standard_normal((cout, cin // groups, k)).astype(f32)
    dz = rng.standard_normal((n, cout, wc)).astype(f32)
    ref = R.conv1d_backward_ref(x, wt, dz, pad, dil, groups)
    (dx, bx), (dw, bw), (db, bb) = guarded(n, cin, w), guarded(cout, cin // groups, k), guarded(cout)
    model.conv1d_backward(dev(x), dev(wt), dev(dz), pad, dil, groups, dx=dx, dw=dw, db=db, need_dx=need_dx)
    torch.cuda.synchronize()
    ctx = f"k{k} d{dil} p{pad} g{groups} {cin}->{cout} w{w} n{n}"
    if need_dx:
        within("dx", dx, *ref["dx"], ctx, bx)
    else:
        assert bool(torch.isnan(bx).all()), "dx was written although it was not asked for"
    within("dw", dw, *ref["dw"], ctx, bw)
    within("db", db, *ref["db"], ctx, bb)


@pytest.mark.parametrize("case", CONV_CASES, ids=lambda c: "k{}d{}p{}g{}_{}to{}_w{}n{}".format(*c))
def test_conv_backward(case):
    check_conv_backward(*case)


def test_conv_backward_over_several_slabs():
    """n * wc spans three slabs of the reducer and is no multiple of the slab; once more without dx."""
    from onset_fingerprinting_amd import _lib
    slab = int(_lib.lib().ofp_cnn_train_slab())
    w = 257
    n = (2 * slab + slab // 3) // w + 1
    assert 2 * slab < n * w < 3 * slab and (n * w) % slab
    check_conv_backward(3, 1, 1, 1, 5, 6, w, n)
    check_conv_backward(3, 1, 1, 2, 4, 6, w, n, need_dx=False)


# ---- BatchNorm in training mode -------------------------------------------------------------------------------------
def bn_shapes():
    from onset_fingerprinting_amd import _lib
    slab = int(_lib.lib().ofp_cnn_train_slab())
    n = (2 * slab + 5) // 131 + 1
    assert n * 131 > 2 * slab and (n * 131) % slab
    return [(3, 5, 7), (2, 3, 1), (n, 4, 131)]  # n * w odd; n * w = 2; several slabs


@pytest.mark.parametrize("which", [0, 1, 2], ids=["odd", "two", "slabs"])
def test_batchnorm_training(which):
    from onset_fingerprinting_amd import model
    n, C, w = bn_shapes()[which]
    rng = np.random.default_rng(40 + which)
    x = (rng.standard_normal((n, C, w)) * 1.5 + 0.3).astype(f32)
    ga, be = rng.uniform(0.5, 1.5, C).astype(f32), rng.standard_normal(C).astype(f32)
    rm, rv = rng.standard_normal(C).astype(f32), rng.uniform(0.5, 2, C).astype(f32)
    dy = rng.standard_normal((n, C, w)).astype(f32)
    eps, mom = 1e-5, 0.1
    fwd = R.batchnorm_train_forward_ref(x, ga, be, rm, rv, eps, mom)
    bwd = R.batchnorm_train_backward_ref(x, ga, dy, eps)
    ctx = f"bn n{n} C{C} w{w}"
    xd, gd, rmd, rvd = dev(x), dev(ga), dev(rm), dev(rv)
    y, by = guarded(n, C, w)
    _y, mean, rstd = model.batchnorm_train_forward(xd, gd, dev(be), rmd, rvd, eps, mom, out=y)
    torch.cuda.synchronize()
    within("y", y, *fwd["y"], ctx, by)
    within("mean", mean, *fwd["mean"], ctx)
    within("rstd", rstd, *fwd["rstd"], ctx)
    within("running_mean", rmd, *fwd["running_mean"], ctx)
    within("running_var", rvd, *fwd["running_var"], ctx)
    dx, bx = guarded(n, C, w)
    _dx, dgamma, dbeta = model.batchnorm_train_backward(xd, gd, mean, rstd, dev(dy), out=dx)
    torch.cuda.synchronize()
    within("dx", dx, *bwd["dx"], ctx, bx)
    within("dgamma", dgamma, *bwd["dgamma"], ctx)
    within("dbeta", dbeta, *bwd["dbeta"], ctx)


# ---- NAdam ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("step", [0, 7, 251])
def test_nadam_step(step):
    from onset_fingerprinting_amd import model
    fac = model.cnn_step_factors(model.cnn_rate_table(0.01, 300))[step]
    rng = np.random.default_rng(step)
    n = 1000
    p, gr = rng.standard_normal(n).astype(f32), rng.standard_normal(n).astype(f32)
    m = (gr * rng.uniform(0.1, 1.0, n)).astype(f32)
    v = (gr.astype(f64) ** 2 * rng.uniform(0.1, 1.0, n)).astype(f32)
    row = np.zeros(4, f32)
    row[:3] = fac
    p1, m1, v1, upd = R.nadam_step_ref(p, gr, m, v, row[:3].astype(f64))
    (pd, bp), md, vd = guarded(n), dev(m), dev(v)
    pd.copy_(dev(p))
    model.nadam_step(pd, dev(gr), md, vd, dev(row))
    torch.cuda.synchronize()
    ctx = f"nadam step {step}"
    within("p", pd, p1, 8 * U24 * np.abs(upd) + U24 * np.abs(p1), ctx, bp)
    within("exp_avg", md, m1, 3 * U24 * (np.abs(m) + np.abs(gr)), ctx)
    within("exp_avg_sq", vd, v1, 4 * U24 * np.abs(v1), ctx)


# ---- the Linear head with its loss ----------------------------------------------------------------------------------
_head = {}


def head_case(shape, loss):
    """Inputs and float64 reference of one shape and loss; computed once."""
    if (shape, loss) not in _head:
        inputs = R.linear_head_inputs(*shape)
        _head[shape, loss] = (inputs, R.linear_head_ref(*inputs, loss))
    return _head[shape, loss]


def check_head(shape, loss, label=""):
    from onset_fingerprinting_amd import model
    (h, w, b, y), ref = head_case(shape, loss)
    n, Fe, O = shape
    sizes = {"out": (n, O), "dy": (n, O), "loss": (1,), "dw": (O, Fe), "db": (O,), "dh": (n, Fe)}
    bufs = {k: guarded(*s) for k, s in sizes.items()}
    model.linear_head_train(dev(h), dev(w), dev(b), dev(y), loss, out=bufs["out"][0], dy=bufs["dy"][0],
                            loss_out=bufs["loss"][0], dw=bufs["dw"][0], db=bufs["db"][0], dh=bufs["dh"][0])
    torch.cuda.synchronize()
    ctx = f"head{label} n{n} F{Fe} O{O} {'mse' if loss else 'l1'}"
    for k in sizes:
        within(k, bufs[k][0], *ref[k], ctx, bufs[k][1])


@pytest.mark.parametrize("loss", [0, 1], ids=["l1", "mse"])
@pytest.mark.parametrize("shape", R.HEAD_SHAPES, ids=lambda s: "n{}_F{}_O{}".format(*s))
def test_linear_head(shape, loss):
    """ofp_linear_head_train, the launches both trainers' epochs make, element-wise against float64 on either side of
    the chunk of 64 samples, the 256-thread strides over samples and features and the odd output tail."""
    check_head(shape, loss)


def test_linear_head_refusals():
    """n = 0, n = 1025, O = 17, F = 0 and a NULL pointer: OFP_ERR_INVALID, nothing written, the device usable."""
    from onset_fingerprinting_amd import _lib, model
    L, INVALID = _lib.lib(), 1  # OFP_ERR_INVALID of include/onsetfp.h
    n, Fe, O = 4, 5, 3
    src = torch.ones(1025 * 17, dtype=torch.float32, device="cuda")
    outs = [torch.full((1025 * 17,), float("nan"), dtype=torch.float32, device="cuda") for _ in range(6)]
    ws = torch.full((1 << 16,), float("nan"), dtype=torch.float32, device="cuda")
    p, o = src.data_ptr(), [t.data_ptr() for t in outs]

    def call(n, Fe, O, h=p, dw=o[3]):
        return L.ofp_linear_head_train(h, n, Fe, p, O, p, p, 0, o[0], o[1], o[2], dw, o[4], o[5], ws.data_ptr(),
                                       ws.numel() * 4, None)

    for args in ((0, Fe, O), (1025, Fe, O), (n, Fe, 17), (n, 0, O)):
        assert L.ofp_linear_head_train_workspace_bytes(*args) == -1
        assert call(*args) == INVALID, args
        assert b"ofp_linear_head_train" in L.ofp_last_error()
    assert call(n, Fe, O, h=None) == INVALID and call(n, Fe, O, dw=None) == INVALID
    assert L.ofp_linear_head_train(p, n, Fe, p, O, p, p, 2, *o, ws.data_ptr(), ws.numel() * 4, None) == INVALID
    assert L.ofp_linear_head_train(p, n, Fe, p, O, p, p, 0, *o, ws.data_ptr(), 8, None) != 0  # work space too small
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(t).all()) for t in outs + [ws]), "a refused call wrote something"
    with pytest.raises(ValueError, match="limits"):
        model.linear_head_train(src[:1025 * 2].view(1025, 2), src[:4].view(2, 2), src[:2], src[:2050].view(1025, 2))
    check_head((65, 257, 3), 1, " after the refusals")


# ---- gradients at the start -----------------------------------------------------------------------------------------
def autograd_reference(model, x, y):
    """Loss and gradients of torch autograd on the CPU over the model's own torch layers, in float32 and float64."""
    out = {}
    for dtype in (torch.float32, torch.float64):
        net = copy.deepcopy(model).cpu().to(dtype).train()
        v = model.loss(net.fc(torch.flatten(net.conv_layers(x.to(dtype)), start_dim=1)), y.to(dtype))
        v.backward()
        out[dtype] = ({k: p.grad.numpy() for k, p in net.named_parameters()}, float(v.detach()))
    return out


def check_grads(ours, loss_ours, g32, g64, loss64, n, label):
    assert sorted(ours) == sorted(g64)
    for k, ref64 in g64.items():
        mine = ours[k].detach().cpu().numpy().astype(f64)
        ref64 = ref64.astype(f64)
        err = np.max(np.abs(mine - ref64))
        err32 = np.max(np.abs(g32[k].astype(f64) - ref64))
        bound = max(4 * err32, U23 * np.max(np.abs(ref64)))
        print(f"{label} {k}: |ours - g64| {err:.3e}  |g32 - g64| {err32:.3e}  bound {bound:.3e}  error / bound "
              f"{err / bound:.3g}")
        assert err <= bound, (label, k, err, bound)
    rel = abs(float(loss_ours) - loss64) / loss64
    print(f"{label} loss: ours {float(loss_ours):.9g} ref64 {loss64:.9g} rel {rel:.3e} bound {n * U24:.3e}  error / "
          f"bound {rel / (n * U24):.3g}")
    assert rel <= n * U24


ACTS = [nn.Identity, nn.ReLU, nn.SiLU, nn.LeakyReLU, nn.ELU, nn.Tanh]
ARCH = [dict(activation=a, batch_norm=bn) for a in ACTS for bn in (False, True)] + [
    dict(pool=True, width=32), dict(pool=True, width=33, batch_norm=True), dict(pool=True, width=35, kernel_size=5,
                                                                                padding=2),
    dict(layer_sizes=[5]), dict(layer_sizes=[4, 6, 5], batch_norm=True, pool=True, width=37),
    dict(groups=2, channels=4, layer_sizes=[6, 4], batch_norm=True), dict(groups=2, channels=4, layer_sizes=[4],
                                                                          dilation=2, loss=F.mse_loss),
    dict(loss=F.mse_loss, batch_norm=True, activation=nn.Tanh),
]


def arch_id(a):
    return "-".join(f"{k}={getattr(v, '__name__', v)}" for k, v in a.items())


@pytest.mark.parametrize("arch", ARCH, ids=arch_id)
def test_gradients_of_the_architecture_matrix(arch):
    from onset_fingerprinting_amd import model
    kw = dict(arch)
    width, channels = kw.pop("width", 30), kw.pop("channels", 3)
    torch.manual_seed(len(arch_id(arch)))
    m = model.CNN(width, 2, channels=channels, dropout_rate=0.0, **{"layer_sizes": [5, 6], **kw})
    n = 21
    x, y = torch.randn(n, channels, width), torch.randn(n, 2)
    loss, grads = model.cnn_loss_and_grads_device(m, x.cuda(), y.cuda())
    ref = autograd_reference(m, x, y)
    check_grads(grads, loss, ref[torch.float32][0], ref[torch.float64][0], ref[torch.float64][1], 2 * n, arch_id(arch))


# Whole networks at the batch sizes of the workload.  Width 32, kernel 3, padding 1: 32 (sample, position) pairs per
# sample, so n = 64 is exactly one slab of the reducer and one chunk of the Linear head's weight gradient, n = 65 adds
# a slab of 32 pairs and a chunk of one sample, n = 1024 (the limit) has 16 of each; 129 and 257 lie past two chunks
# and past the 256-thread stride of the loss kernel.  Smooth activations, so that the float32 reference is not itself
# at a kink; one ReLU case with a pool.
BIG = [dict(n=n, batch_norm=bn, activation=nn.Tanh if bn else nn.SiLU) for n in (64, 65, 129, 257, 1024)
       for bn in (False, True)] + [
    dict(n=65, output_size=1), dict(n=65, output_size=3, batch_norm=True), dict(n=65, output_size=16),
    dict(n=65, pool=True, width=33, batch_norm=True, activation=nn.ReLU),
    dict(n=65, groups=2, channels=4, layer_sizes=[6, 4], batch_norm=True), dict(n=65, loss=F.mse_loss, activation=nn.Tanh),
]


def big_model(arch):
    from onset_fingerprinting_amd import model
    kw = dict(arch)
    n, width, channels, out = kw.pop("n"), kw.pop("width", 32), kw.pop("channels", 3), kw.pop("output_size", 2)
    torch.manual_seed(len(arch_id(arch)))
    m = model.CNN(width, out, channels=channels, dropout_rate=0.0, **{"layer_sizes": [5, 6], **kw})
    return m, torch.randn(n, channels, width), torch.randn(n, out)


@pytest.mark.parametrize("arch", BIG, ids=arch_id)
def test_gradients_past_one_slab_and_one_chunk(arch):
    from onset_fingerprinting_amd import _lib, model
    m, x, y = big_model(arch)
    n, wc = len(x), x.shape[2]
    if "width" not in arch:
        slab = int(_lib.lib().ofp_cnn_train_slab())
        assert wc * 64 == slab and (n == 64 or n * wc > slab)
    loss, grads = model.cnn_loss_and_grads_device(m, x.cuda(), y.cuda())
    ref = autograd_reference(m, x, y)
    check_grads(grads, loss, ref[torch.float32][0], ref[torch.float64][0], ref[torch.float64][1], y.numel(),
                arch_id(arch))


@pytest.mark.parametrize("case", CASES + [STOP])
def test_gradients_at_the_start(g, case):
    from onset_fingerprinting_amd import model
    cfg, m, x, y, _val = load_case(g, case)
    loss, grads = model.cnn_loss_and_grads_device(m, x.cuda(), y.cuda())
    pre32, pre64 = f"{case}/g32/", f"{case}/g64/"
    g32 = {k[len(pre32):]: g[k] for k in g.files if k.startswith(pre32)}
    g64 = {k[len(pre64):]: g[k] for k in g.files if k.startswith(pre64)}
    check_grads(grads, loss, g32, g64, float(g[f"{case}/loss64"]), 2 * len(x), case)


# ---- training runs --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES + [STOP])
def test_trajectory_over_the_comparable_prefix(g, case):
    ref, ref64 = g[f"{case}/errors"], g[f"{case}/errors64"]
    prefix, spread = comparable_prefix(ref, g[f"{case}/pert_errors"])
    assert prefix >= min(24, len(ref))
    m, fit = our_run(g, case)
    ours = fit.train_loss.cpu().numpy()
    assert fit.epochs >= prefix and np.isfinite(ours[:fit.epochs]).all()
    own = np.maximum(spread[:prefix], np.abs(ref[:prefix].astype(f64) - ref64[:prefix]))
    bound = np.maximum(4 * np.maximum.accumulate(own), U22 * ref[:prefix])
    diff = np.abs(ours[:prefix].astype(f64) - ref[:prefix])
    worst = int(np.argmax(diff / bound))
    print(f"{case}: prefix {prefix} of {len(ref)}; worst epoch {worst}: |ours - ref| {diff[worst]:.3e} bound "
          f"{bound[worst]:.3e} (spread {spread[worst]:.3e}, loss {ref[worst]:.6g}); last epoch of the prefix: "
          f"{diff[prefix - 1]:.3e} against {bound[prefix - 1]:.3e}")
    assert np.all(diff <= bound), (case, worst, diff[worst], bound[worst])
    if prefix == len(ref) and "stop" not in case:  # comparable over its whole length: the end state too
        assert fit.epochs == len(ref)
        ps = torch.cat([p.detach().reshape(-1) for p in m.parameters()]).cpu().numpy().astype(f64)
        st = [b.detach().reshape(-1) for k, b in m.named_buffers() if "running" in k]
        st = torch.cat(st).cpu().numpy().astype(f64) if st else np.zeros(0)
        for what, mine, rec in (("parameters", ps, g[f"{case}/flat"]), ("running statistics", st, g[f"{case}/stats"])):
            rec = rec.astype(f64)
            if rec.shape[1] == 0:
                continue
            sp = np.max(np.abs(rec[1:] - rec[0]))
            err = np.max(np.abs(mine - rec[0]))
            b = max(4 * sp, U23 * np.max(np.abs(rec[0])))
            print(f"{case}: {what} max |ours - ref| {err:.3e}, spread of the disturbed runs {sp:.3e}, bound {b:.3e}")
            assert err <= b, (what, err, b)


def test_a_case_is_comparable_over_its_whole_length(g):
    assert any(comparable_prefix(g[f"{c}/errors"], g[f"{c}/pert_errors"])[0] == len(g[f"{c}/errors"]) for c in CASES)


@pytest.mark.parametrize("case", [c for c in CASES if c != "mse_tanh_dil_bn"])
def test_outcome_of_the_chaotic_cases(g, case):
    ref, pert = g[f"{case}/errors"], g[f"{case}/pert_errors"]
    prefix, _s = comparable_prefix(ref, pert)
    assert prefix < len(ref), "not a chaotic case"
    curves = [ref] + [pert[k] for k in range(len(pert))]
    finals = np.array([c[-1] for c in curves], f64)
    bests = np.array([c.min() for c in curves], f64)
    wobble = float(np.max(np.abs(np.diff(ref[-51:].astype(f64)))))
    _m, fit = our_run(g, case)
    ours = fit.train_loss.cpu().numpy()[:fit.epochs]
    w_final = max(finals.max() - finals.min(), wobble)
    w_best = max(bests.max() - bests.min(), wobble)
    msg = (f"{case}: reference finals {finals.tolist()} bests {bests.tolist()} wobble {wobble:.4g}; ours final "
           f"{ours[-1]:.8g} best {ours.min():.8g} epochs {fit.epochs}")
    print(msg)
    assert fit.epochs == len(ref), msg
    assert ours[-1] <= finals.max() + w_final, msg
    assert ours.min() <= bests.max() + w_best, msg


def test_early_stop(g):
    from onset_fingerprinting_amd import model
    cfg, start, x, y, val = load_case(g, STOP)
    stop = int(g[f"{STOP}/stop"])
    m, fit = our_run(g, STOP)
    tl, vl = fit.train_loss.cpu().numpy(), fit.val_loss.cpu().numpy()
    ref_val = g[f"{STOP}/val"]
    print(f"{STOP}: reference stops after {stop} epochs, ours after {fit.epochs}; last validation loss ours "
          f"{vl[fit.epochs - 1]:.7g} reference {ref_val[-1]:.7g}")
    assert fit.epochs == stop
    assert tl.shape == vl.shape == (cfg["epochs"],) and len(fit.lrs) == stop
    assert np.isfinite(tl[:stop]).all() and np.isfinite(vl[:stop]).all()
    assert np.isnan(tl[stop:]).all() and np.isnan(vl[stop:]).all()
    assert not m.training
    for mod in m.conv_layers:
        if isinstance(mod, nn.BatchNorm1d):
            assert int(mod.num_batches_tracked) == stop
    later = stop + 7
    m2 = copy.deepcopy(start).cuda()
    fit2 = model.fit_cnn(m2, x.cuda(), y.cuda(), x_val=val[0].cuda(), y_val=val[1].cuda(), max_epochs=cfg["epochs"],
                         min_epochs=later, patience=cfg["patience"])
    assert fit2.epochs == later and bool(torch.isnan(fit2.val_loss[later:]).all())
    assert torch.equal(fit2.train_loss[:stop].view(torch.int32), fit.train_loss[:stop].view(torch.int32))


def test_consistency_with_inference(g):
    """The trainer's last validation loss against the existing HIP forward of the trained module: one chain of
    float32 sums against another."""
    _cfg, _s, _x, _y, val = load_case(g, STOP)
    m, fit = our_run(g, STOP)
    with torch.no_grad():
        again = float(F.l1_loss(m(val[0].cuda()), val[1].cuda()))
    last = float(fit.val_loss[fit.epochs - 1])
    rel = abs(again - last) / abs(again)
    print(f"last validation loss {last:.9g}, forward of the trained module {again:.9g}, rel {rel:.3e}, bound {U20:.3e}")
    assert rel <= U20


def test_determinism_and_graph_against_plain_launches(g, monkeypatch):
    from onset_fingerprinting_amd import model
    cfg, start, x, y, val = load_case(g, STOP)
    results = []
    for mode in (None, None, "nodes"):
        if mode:
            monkeypatch.setenv("OFP_CNN_GRAPH", mode)
        m = copy.deepcopy(start).cuda()
        fit = model.fit_cnn(m, x.cuda(), y.cuda(), x_val=val[0].cuda(), y_val=val[1].cuda(), max_epochs=90)
        results.append((fit, torch.cat([t.detach().reshape(-1).float() for t in m.state_dict().values()])))
    monkeypatch.delenv("OFP_CNN_GRAPH", raising=False)
    (a, pa) = results[0]
    assert a.epochs == 90 and bool(torch.isfinite(a.train_loss).all())
    for b, pb in results[1:]:
        assert b.epochs == a.epochs and torch.equal(pa, pb)
        assert torch.equal(a.train_loss.view(torch.int32), b.train_loss.view(torch.int32))
        assert torch.equal(a.val_loss.view(torch.int32), b.val_loss.view(torch.int32))


_five = {}


@pytest.mark.parametrize("E", [1, 2])
def test_a_short_run_is_the_start_of_a_longer_one(g, E):
    """The epoch driver's short paths: max_epochs = 1 captures no graph at all, max_epochs = 2 captures one and replays
    it once.  The rate of epoch e depends on e alone (model.cnn_rate_table), not on max_epochs, so the losses of
    either run are the first of a 5-epoch run, bit for bit."""
    from onset_fingerprinting_amd import model
    _cfg, start, x, y, val = load_case(g, STOP)

    def run(epochs):
        fit = model.fit_cnn(copy.deepcopy(start).cuda(), x.cuda(), y.cuda(), x_val=val[0].cuda(),
                            y_val=val[1].cuda(), max_epochs=epochs)
        assert fit.epochs == epochs
        return fit

    if not _five:
        _five["fit"] = run(5)
    long, short = _five["fit"], run(E)
    assert torch.equal(short.train_loss[:E].view(torch.int32), long.train_loss[:E].view(torch.int32))
    assert torch.equal(short.val_loss[:E].view(torch.int32), long.val_loss[:E].view(torch.int32))


def test_in_place_semantics(g):
    from onset_fingerprinting_amd import model
    cfg, m, x, y, _val = load_case(g, "l1_silu_bn")
    before = {k: v.clone() for k, v in m.state_dict().items()}
    fit = model.fit_cnn(m, x, y, max_epochs=40)  # module and data on the CPU
    assert fit.epochs == 40 and fit.val_loss is None and not m.training
    after = m.state_dict()
    assert all(not v.is_cuda for v in after.values())
    assert all(not torch.equal(before[k], after[k]) for k in before)
    assert int(m.conv_layers.bn1.num_batches_tracked) == 40
    # the same 40 epochs on a GPU copy of the start give the same bits
    m_gpu = load_case(g, "l1_silu_bn")[1].cuda()
    fit_gpu = model.fit_cnn(m_gpu, x.cuda(), y.cuda(), max_epochs=40)
    assert all(torch.equal(after[k], v.cpu()) for k, v in m_gpu.state_dict().items())
    assert torch.equal(fit.train_loss.view(torch.int32), fit_gpu.train_loss.view(torch.int32))
    # a second call continues from the new parameters: its first loss is the loss of the module as it stands
    loss_now, _g = model.cnn_loss_and_grads_device(m, x, y)
    again = model.fit_cnn(m, x, y, max_epochs=5)
    assert float(again.train_loss[0]) == float(loss_now)
    assert float(again.train_loss[0]) < float(fit.train_loss[0])
    assert int(m.conv_layers.bn1.num_batches_tracked) == 45


# ---- the epoch past one slab, one chunk and 256 validation windows --------------------------------------------------
def epoch_start():
    """Width 32 with BatchNorm, n = 130 (three slabs, three chunks), n_val = 300 > n and > the loss kernel's 256
    threads: the work space is sized by the validation batch."""
    from onset_fingerprinting_amd import model
    torch.manual_seed(130)
    m = model.CNN(32, 2, channels=3, dropout_rate=0.0, layer_sizes=[5, 6], batch_norm=True)
    return m, torch.randn(130, 3, 32), torch.randn(130, 2), torch.randn(300, 3, 32), torch.randn(300, 2)


def test_one_epoch_with_a_validation_batch_larger_than_the_training_batch():
    from onset_fingerprinting_amd import model
    m, x, y, xv, yv = epoch_start()
    m = m.cuda()
    loss0, _g = model.cnn_loss_and_grads_device(m, x.cuda(), y.cuda())
    fit = model.fit_cnn(m, x.cuda(), y.cuda(), x_val=xv.cuda(), y_val=yv.cuda(), max_epochs=1)
    assert fit.epochs == 1
    assert float(fit.train_loss[0]) == float(loss0)
    ref = {}
    for dtype in (torch.float32, torch.float64):
        net = copy.deepcopy(m).cpu().to(dtype).eval()
        with torch.no_grad():
            ref[dtype] = float(F.l1_loss(net.fc(torch.flatten(net.conv_layers(xv.to(dtype)), start_dim=1)),
                                         yv.to(dtype)))
    ours, l32, l64 = float(fit.val_loss[0]), ref[torch.float32], ref[torch.float64]
    bound = max(4 * abs(l32 - l64), U22 * l64)
    print(f"validation loss after one epoch: ours {ours:.9g} torch float32 {l32:.9g} float64 {l64:.9g}; |ours - l64| "
          f"{abs(ours - l64):.3e} bound {bound:.3e}  error / bound {abs(ours - l64) / bound:.3g}")
    assert abs(ours - l64) <= bound


def test_determinism_past_one_slab_and_one_chunk(monkeypatch):
    """Five epochs twice as a graph and once as plain launches: the same bits in both curves and in the final state."""
    from onset_fingerprinting_amd import model
    start, x, y, xv, yv = epoch_start()
    results = []
    for mode in (None, None, "nodes"):
        if mode:
            monkeypatch.setenv("OFP_CNN_GRAPH", mode)
        m = copy.deepcopy(start).cuda()
        fit = model.fit_cnn(m, x.cuda(), y.cuda(), x_val=xv.cuda(), y_val=yv.cuda(), max_epochs=5)
        results.append((fit, torch.cat([t.detach().reshape(-1).float() for t in m.state_dict().values()])))
    monkeypatch.delenv("OFP_CNN_GRAPH", raising=False)
    (a, pa) = results[0]
    assert a.epochs == 5 and bool(torch.isfinite(a.train_loss).all()) and bool(torch.isfinite(a.val_loss).all())
    for b, pb in results[1:]:
        assert b.epochs == 5 and torch.equal(pa, pb)
        assert torch.equal(a.train_loss.view(torch.int32), b.train_loss.view(torch.int32))
        assert torch.equal(a.val_loss.view(torch.int32), b.val_loss.view(torch.int32))
