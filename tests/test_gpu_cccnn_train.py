"""GPU: training model.LCCCNN (csrc/ofp_cccnn_train.hip, model.fit_lcccnn) against float64 references and the
reference's recorded runs (tests/golden/g27_cccnn_train.npz, made by make_golden_cccnn_train.py).

  kernels     the strided convolution's three gradients, GroupNorm(1) in training mode, the correlation head's
              backward and the SGD step, called directly, element-wise against float64 with the derived bounds of
              tests/cccnn_train_ref.py; outputs go into NaN-filled buffers with a guard tail
  gradients   per tensor, max |ours - g64| <= 4 x max |g32 - g64|, floored at 2^-23 x max |g64|; the inputs or
              GroupNorm's weights are scaled so that the softmax of the head is not saturated (asserted); up to the
              limit of 4 096 (window, sensor) pairs, so that whole chains cross slabs and chunks
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

from oracle import nn_kernels as K

sys.path.insert(0, str(Path(__file__).resolve().parent))
import cccnn_train_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = ["shared_gn_l1_silu", "grouped_strided_l1", "shared_gn_pool_mse_tanh_dil"]
WHOLE = "shared_gn_pool_mse_tanh_dil"
STOP = "shared_gn_l1_silu_stop"
U24, U23, U22, U20 = 2.0 ** -24, 2.0 ** -23, 2.0 ** -22, 2.0 ** -20
GUARD = 64
f32, f64 = np.float32, np.float64


@pytest.fixture(scope="module")
def g(golden):
    return golden("g27_cccnn_train")


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
    bound = np.broadcast_to(bound, err.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = float(np.max(np.where(np.isnan(err) | ((bound == 0) & (err > 0)), np.inf,
                                      np.where(bound > 0, err / bound, 0.0)))) if err.size else 0.0
    print(f"{ctx} {name}: largest error / bound {ratio:.3g}, largest error {float(np.nanmax(err)) if err.size else 0:.3e}")
    assert bool((err <= bound).all()), (name, ctx, f"error / bound = {ratio:.3g}")


# ---- the convolution's gradients ------------------------------------------------------------------------------------
# (k, stride, dilation, padding, groups, cin, cout, width, n)
CONV_CASES = [
    (1, 1, 1, 0, 1, 1, 5, 7, 3), (9, 1, 1, 1, 1, 1, 3, 32, 4), (33, 1, 1, 1, 1, 5, 5, 40, 3),
    (64, 1, 1, 1, 1, 5, 5, 70, 2),  # 321 outputs per channel
    (64, 1, 1, 0, 1, 1, 2, 64, 2),  # one column is left
    (5, 2, 1, 1, 4, 4, 8, 33, 3), (3, 3, 2, 2, 1, 2, 3, 34, 2),  # the stride does not divide
    (4, 4, 1, 0, 2, 4, 4, 19, 3),
    (3, 2, 1, 1, 1, 1, 2, 257, 40),  # n * wc = 5160 spans three slabs
] + R.WGRAD_LANE_CASES  # both sides of every change of the lanes per output (tests/test_cccnn_train_cpu.py)


def check_conv_backward(k, stride, dil, pad, groups, cin, cout, w, n, need_dx=True):
    from onset_fingerprinting_amd import model
    wc = R.conv_width(w, k, pad, dil, stride)
    assert wc >= 1
    rng = np.random.default_rng([k, stride, dil, pad, groups, cin, cout, w, n])
    x = rng.standard_normal((n, cin, w)).astype(f32)
    wt = rng.standard_normal((cout, cin // groups, k)).astype(f32)
    dz = rng.standard_normal((n, cout, wc)).astype(f32)
    ref = R.conv1d_backward_strided_ref(x, wt, dz, pad, dil, groups, stride)
    (dx, bx), (dw, bw), (db, bb) = guarded(n, cin, w), guarded(cout, cin // groups, k), guarded(cout)
    model.conv1d_backward_strided(dev(x), dev(wt), dev(dz), pad, dil, groups, stride, dx=dx, dw=dw, db=db,
                                  need_dx=need_dx)
    torch.cuda.synchronize()
    ctx = f"k{k} s{stride} d{dil} p{pad} g{groups} {cin}->{cout} w{w} n{n}"
    if need_dx:
        within("dx", dx, *ref["dx"], ctx, bx)
    else:
        assert bool(torch.isnan(bx).all()), "dx was written although it was not asked for"
    within("dw", dw, *ref["dw"], ctx, bw)
    within("db", db, *ref["db"], ctx, bb)


@pytest.mark.parametrize("case", CONV_CASES, ids=lambda c: "k{}s{}d{}p{}g{}_{}to{}_w{}n{}".format(*c))
def test_conv_backward_strided(case):
    from onset_fingerprinting_amd import _lib
    k, stride, dil, pad, groups, cin, cout, w, n = case
    if w == 257:
        slab = int(_lib.lib().ofp_cnn_train_slab())
        assert 2 * slab < n * R.conv_width(w, k, pad, dil, stride) < 3 * slab
    check_conv_backward(*case)


def test_conv_backward_strided_without_dx():
    check_conv_backward(5, 2, 1, 1, 4, 4, 8, 33, 3, need_dx=False)


def test_conv_backward_strided_equals_the_stride_1_entry():
    """At stride 1 the two entries run the same kernels: the same bits."""
    from onset_fingerprinting_amd import model
    rng = np.random.default_rng(77)
    x, wt, dz = (dev(rng.standard_normal(s)) for s in ((3, 4, 21), (6, 2, 5), (3, 6, 19)))
    a = model.conv1d_backward(x, wt, dz, 1, 1, 2)
    b = model.conv1d_backward_strided(x, wt, dz, 1, 1, 2, 1)
    assert all(torch.equal(p.view(torch.int32), q.view(torch.int32)) for p, q in zip(a, b))


# ---- GroupNorm(1) in training mode ----------------------------------------------------------------------------------
# (K, V, items, pool, offset)
GN_CASES = [(1, 1, 2, False, 0.0), (5, 7, 3, False, 0.0), (5, 7, 3, True, 0.0), (2, 257, 3, False, 0.0),
            (2, 257, 3, True, 0.0), (6, 33, 130, False, 0.0), (6, 33, 130, True, 0.0), (2, 257, 3, False, 1000.0)]


@pytest.mark.parametrize("case", GN_CASES, ids=lambda c: "K{}V{}n{}{}{}".format(c[0], c[1], c[2], "_pool" if c[3] else "",
                                                                                 "_mean1000" if c[4] else ""))
def test_groupnorm_training(case):
    from onset_fingerprinting_amd import _lib, model
    Kc, V, items, pool, offset = case
    if items == 130:
        assert items * V > 2 * int(_lib.lib().ofp_cnn_train_slab())  # several slabs, the last one partial
    rng = np.random.default_rng([Kc, V, items, int(pool)])
    x = (rng.standard_normal((items, Kc, V)) * 1.5 + 0.3 + offset).astype(f32)
    ga = (rng.uniform(0.5, 1.5, Kc) * rng.choice([-1, 1], Kc)).astype(f32)
    be = rng.standard_normal(Kc).astype(f32)
    Vo = V // 2 if pool else V
    dy = rng.standard_normal((items, Kc, Vo)).astype(f32)
    eps = 1e-5
    fwd = R.groupnorm1_train_forward_ref(x, ga, be, eps, pool)
    bwd = R.groupnorm1_train_backward_ref(x, ga, be, dy, eps, pool)
    ctx = f"gn K{Kc} V{V} items{items} pool{int(pool)} offset{offset:g}"
    xd, gd, bd = dev(x), dev(ga), dev(be)
    y, by = guarded(items, Kc, Vo)
    _y, mean, rstd = model.groupnorm1_train_forward(xd, gd, bd, eps, pool, out=y)
    torch.cuda.synchronize()
    within("y", y, *fwd["y"], ctx, by)
    within("mean", mean, *fwd["mean"], ctx)
    within("rstd", rstd, *fwd["rstd"], ctx)
    dx, bx = guarded(items, Kc, V)
    _dx, dgamma, dbeta = model.groupnorm1_train_backward(xd, gd, bd, mean, rstd, dev(dy), pool, out=dx)
    torch.cuda.synchronize()
    within("dx", dx, *bwd["dx"], ctx, bx)
    within("dgamma", dgamma, *bwd["dgamma"], ctx)
    within("dbeta", dbeta, *bwd["dbeta"], ctx)


# ---- the correlation head's backward --------------------------------------------------------------------------------
def check_head_backward(Kc, V, n, C, O, scale=None, ctx=""):
    from onset_fingerprinting_amd import model
    rng = np.random.default_rng([Kc, V, n, C, O])
    scale = 1.0 / np.sqrt(Kc * V) if scale is None else scale  # cc of order 1: the softmax is spread out
    f = (rng.standard_normal((n * C, Kc, V)) * scale).astype(f32)
    dout = rng.standard_normal((n, O)).astype(f32)
    wfc = rng.standard_normal((O, C * (2 * V - 1))).astype(f32)
    fd = dev(f)
    probs = model.autocorr_softmax(fd)
    p_ref, e_p = K.autocorr_softmax_ref(f)
    ref, bound = R.autocorr_softmax_backward_ref(f, dout, wfc, C, e_p=e_p)
    df, buf = guarded(n * C, Kc, V)
    model.autocorr_softmax_backward(fd, probs, dev(dout), dev(wfc), C, out=df)
    torch.cuda.synchronize()
    ctx = ctx or f"head K{Kc} V{V} items{n * C} O{O} scale {scale:.3g}"
    print(f"{ctx}: largest p {p_ref.max():.6f}, largest |df| {np.abs(ref).max():.3e}")
    within("df", df, ref, bound, ctx, buf)
    return df, p_ref


@pytest.mark.parametrize("Kc,V,n,C,O", [(1, 1, 2, 1, 2), (1, 2, 1, 3, 2), (5, 7, 2, 2, 2), (2, 129, 1, 2, 3),
                                        (5, 133, 2, 4, 2)], ids=lambda v: str(v))
def test_head_backward(Kc, V, n, C, O):
    """(K, V, items, O) = (1,1,2,2), (1,2,3,2), (5,7,4,2), (2,129,2,3) -- 257 lags cross the workgroup's stride --
    and (5,133,8,2), the head of the reference's training configuration."""
    df, _p = check_head_backward(Kc, V, n, C, O)
    if V == 1:
        assert bool((df == 0).all()), "one lag: p = 1 and the gradient is exactly zero"


def test_head_backward_saturated():
    """Inputs x 30: the lag 0 takes everything; the gradient stays finite and inside the bound."""
    df, p = check_head_backward(5, 7, 2, 2, 2, scale=30.0 / np.sqrt(35))
    assert np.all(p[:, 6] > 1 - 1e-6) and bool(torch.isfinite(df).all())


def test_head_backward_beyond_64_kib_of_lds():
    from onset_fingerprinting_amd import model
    Kc, V = K.AUTOCORR_BIG_LDS
    assert 65536 < model.cccnn_head_lds_bytes(Kc, V) <= model.CCCNN_TRAIN_MAX_LDS
    check_head_backward(Kc, V, 1, 2, 2)
    check_head_backward(1, 63, 1, 2, 2, ctx="after the large launch")  # a small launch after the attribute was raised


# ---- SGD ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("step", [0, 1, 100])
def test_sgd_step(step):
    from onset_fingerprinting_amd import model
    rate = np.asarray(model.lcccnn_rates(0.003, 101), f32)[step]
    assert (rate == 0) == (step == 100)
    rng = np.random.default_rng(step)
    n = 1000
    p, gr = rng.standard_normal(n).astype(f32), (rng.standard_normal(n) * 0.05).astype(f32)
    b0 = (rng.standard_normal(n) * 0.05).astype(f32)
    mom, wd = f32(model.LCCCNN_MOMENTUM), f32(model.LCCCNN_WEIGHT_DECAY)
    ref = R.sgd_step_ref(p, gr, b0, rate, step == 0, mom, wd)
    (pd, bp), bd = guarded(n), dev(b0)
    pd.copy_(dev(p))
    model.sgd_step(pd, dev(gr), bd, dev(np.array([rate], f32)), step == 0)
    torch.cuda.synchronize()
    ctx = f"sgd step {step}, rate {rate:.6g}"
    within("p", pd, *ref["p"], ctx, bp)
    within("momentum buffer", bd, *ref["buf"], ctx)
    if step == 100:
        assert np.array_equal(pd.cpu().numpy(), p), "the parameter changed at a rate of 0"


# ---- gradients of whole networks ------------------------------------------------------------------------------------
def torch_forward(net, x):
    """model.py:513-538 over the torch layers of a CCCNN (training-mode semantics; no dropout): -> (out, probs)."""
    B, C, W = x.shape
    h = net.conv_layers(x if net.group else x.reshape(B * C, 1, W))
    V = h.shape[-1]
    f = h.reshape(B * C, -1, V)
    BC, Kc, _ = f.shape
    cc_raw = F.conv1d(f.reshape(1, BC * Kc, V), f.reshape(BC * Kc, 1, V), groups=BC * Kc, padding=V - 1)
    probs = torch.flatten(F.softmax(cc_raw.view(BC, Kc, -1).sum(dim=1), dim=-1).view(B, C, -1), start_dim=1)
    return net.fc(probs), probs


def autograd_reference(model, x, y):
    """Loss and gradients of torch autograd on the CPU over the model's own torch layers, in float32 and float64."""
    out = {}
    for dtype in (torch.float32, torch.float64):
        net = copy.deepcopy(model).cpu().to(dtype).train()
        o, probs = torch_forward(net.model, x.to(dtype))
        v = model.loss(o, y.to(dtype))
        v.backward()
        out[dtype] = ({k: p.grad.numpy() for k, p in net.named_parameters()}, float(v.detach()),
                      float(probs.detach().max()))
    return out


def check_grads(ours, loss_ours, g32, g64, loss64, n, label):
    assert sorted(ours) == sorted(g64)
    top = max(np.max(np.abs(v)) for v in g64.values())
    for k, ref64 in g64.items():
        mine = ours[k].detach().cpu().numpy().astype(f64)
        ref64 = ref64.astype(f64)
        err = np.max(np.abs(mine - ref64))
        err32 = np.max(np.abs(g32[k].astype(f64) - ref64))
        bound = max(4 * err32, U23 * np.max(np.abs(ref64)))
        print(f"{label} {k}: |ours - g64| {err:.3e}  |g32 - g64| {err32:.3e}  bound {bound:.3e}  max |g64| "
              f"{np.max(np.abs(ref64)):.3e} ({np.max(np.abs(ref64)) / top:.2g} of the largest)  error / bound "
              f"{err / bound:.3g}")
        assert err <= bound, (label, k, err, bound)
    rel = abs(float(loss_ours) - loss64) / loss64
    print(f"{label} loss: ours {float(loss_ours):.9g} ref64 {loss64:.9g} rel {rel:.3e} bound {n * U24:.3e}  error / "
          f"bound {rel / (n * U24):.3g}")
    assert rel <= n * U24


ACTS = [nn.Identity, nn.ReLU, nn.SiLU, nn.LeakyReLU, nn.ELU, nn.Tanh]
ARCH = [dict(activation=a, batch_norm=bn, group=gr) for a in ACTS for bn in (False, True) for gr in (False, True)] + [
    dict(pool=True, width=32), dict(pool=True, width=33, batch_norm=True), dict(pool=True, width=35, group=True,
                                                                                batch_norm=True),
    dict(kernel_sizes=[9, 1]), dict(kernel_sizes=[9, 1], batch_norm=True, group=True),
    dict(strides=[2, 1]), dict(strides=[2, 1], batch_norm=True, kernel_sizes=[5, 3], group=True),
    dict(layer_sizes=[2] * 7, kernel_sizes=[1, 5, 8, 3, 3, 3, 1], width=48, batch_norm=True),
    dict(layer_sizes=[2] * 7, kernel_sizes=[1, 5, 8, 3, 3, 3, 1], width=48),
    dict(loss=F.mse_loss, batch_norm=True, activation=nn.Tanh, dilation=2, padding=2),
]


def arch_id(a):
    return "-".join(f"{k}={getattr(v, '__name__', v)}" for k, v in a.items()).replace(" ", "")


def arch_model(arch):
    """The module and batch of one row of ARCH.  GroupNorm's initial weights are scaled by 0.2, and without a norm the
    inputs by 0.5, so that the head's softmax is not saturated and every tensor's gradient is well above rounding."""
    from onset_fingerprinting_amd import model
    kw = dict(arch)
    width, channels = kw.pop("width", 30), kw.pop("channels", 3)
    torch.manual_seed(len(arch_id(arch)))
    m = model.LCCCNN(width, 2, channels=channels, dropout_rate=0.0, **{"layer_sizes": [3, 2], **kw})
    with torch.no_grad():
        for mod in m.model.conv_layers:
            if isinstance(mod, nn.GroupNorm):
                mod.weight.mul_(0.2)
    n = 7
    x, y = torch.randn(n, channels, width) * (1.0 if kw.get("batch_norm") else 0.5), torch.randn(n, 2)
    return m, x, y


@pytest.mark.parametrize("arch", ARCH, ids=arch_id)
def test_gradients_of_the_architecture_matrix(arch):
    from onset_fingerprinting_amd import model
    m, x, y = arch_model(arch)
    ref = autograd_reference(m, x, y)
    pmax = ref[torch.float64][2]
    print(f"{arch_id(arch)}: largest p of the head {pmax:.4f}")
    assert pmax < 0.9, "the softmax of the head is saturated: the float32 gradients would be noise"
    loss, grads = model.cccnn_loss_and_grads_device(m, x.cuda(), y.cuda())
    check_grads(grads, loss, ref[torch.float32][0], ref[torch.float64][0], ref[torch.float64][1], 2 * len(x),
                arch_id(arch))


# Whole networks at the batch sizes of the workload.  Width 30, 3 sensors: n = 65 windows are 195 items when the stack
# is shared (5850 pairs, three slabs of the reducer) and two chunks of the Linear's weight gradient; n = 257 lies past
# the 256-thread stride of the loss kernel; n = 1024 with 4 sensors is the limit of both, 4096 items.  Smooth
# activations (SiLU by default, Tanh), so that the float32 reference is not itself at a kink.
BIG = [dict(n=n, batch_norm=bn, group=gr, activation=nn.Tanh if gr else nn.SiLU) for n in (65, 257)
       for bn in (False, True) for gr in (False, True)] + [
    dict(n=65, output_size=1, batch_norm=True), dict(n=65, output_size=3), dict(n=65, output_size=16, batch_norm=True),
    dict(n=65, strides=[2, 1], pool=True, batch_norm=True),
    dict(n=1024, channels=4, batch_norm=True),
]


def big_model(arch):
    """arch_model at a batch size and output count of its own: the same scaling of GroupNorm's weights and inputs."""
    from onset_fingerprinting_amd import model
    kw = dict(arch)
    n, channels, out = kw.pop("n"), kw.pop("channels", 3), kw.pop("output_size", 2)
    torch.manual_seed(len(arch_id(arch)))
    m = model.LCCCNN(30, out, channels=channels, dropout_rate=0.0, **{"layer_sizes": [3, 2], **kw})
    with torch.no_grad():
        for mod in m.model.conv_layers:
            if isinstance(mod, nn.GroupNorm):
                mod.weight.mul_(0.2)
    x, y = torch.randn(n, channels, 30) * (1.0 if kw.get("batch_norm") else 0.5), torch.randn(n, out)
    return m, x, y


@pytest.mark.parametrize("arch", BIG, ids=arch_id)
def test_gradients_past_one_slab_and_one_chunk(arch):
    from onset_fingerprinting_amd import _lib, model
    m, x, y = big_model(arch)
    n, C = x.shape[:2]
    items = n if arch.get("group") else n * C
    wc = R.conv_width(30, 3, 1, 1, arch.get("strides", [1])[0])  # of the first layer
    # two chunks at least; several slabs too, unless the windows themselves are the items (65 x 30 pairs are one slab)
    assert n > 64 and (items * wc > int(_lib.lib().ofp_cnn_train_slab()) or (arch.get("group") and n == 65))
    assert n * C <= model.CCCNN_TRAIN_MAX_ITEMS and n <= model.CCCNN_TRAIN_MAX_BATCH
    ref = autograd_reference(m, x, y)
    pmax = ref[torch.float64][2]
    print(f"{arch_id(arch)}: largest p of the head {pmax:.4f}")
    assert pmax < 0.9, "the softmax of the head is saturated: the float32 gradients would be noise"
    loss, grads = model.cccnn_loss_and_grads_device(m, x.cuda(), y.cuda())
    check_grads(grads, loss, ref[torch.float32][0], ref[torch.float64][0], ref[torch.float64][1], y.numel(),
                arch_id(arch))


def test_the_reference_training_architecture():
    """train.py's own network at its own width (7 layers of 5 maps, kernels 1, 33, 64, 15, 15, 15, 1, GroupNorm, 4
    sensors, 256 samples; head of 5 x 133), 6 windows: loss and gradients against float64 autograd, then 3 epochs.

    Measured on an MI355X: every tensor is inside the rule, most with an error below torch's own float32 error (e.g.
    conv7.bias 6.6e-10 against 1.2e-9, fc.weight 3.6e-8 against 3.1e-7).  While the head's cc was still rounded to
    float32 before the softmax, conv7.bias missed it with 6.2e-9 against a bound of 4.8e-9; csrc/ofp_cccnn_train.hip
    (k_head_fwd) says why."""
    from onset_fingerprinting_amd import model
    torch.manual_seed(11)
    m = model.LCCCNN(256, 2, 4, layer_sizes=[5] * 7, kernel_sizes=[1, 33, 64, 15, 15, 15, 1], dropout_rate=0.0,
                     batch_norm=True, loss=F.l1_loss, lr=0.001, group=False)
    with torch.no_grad():
        for mod in m.model.conv_layers:
            if isinstance(mod, nn.GroupNorm):
                mod.weight.mul_(0.2)
    x, y = torch.randn(6, 4, 256), torch.randn(6, 2)
    ref = autograd_reference(m, x, y)
    print(f"largest p of the head {ref[torch.float64][2]:.4f}")
    assert ref[torch.float64][2] < 0.9
    loss, grads = model.cccnn_loss_and_grads_device(m, x.cuda(), y.cuda())
    check_grads(grads, loss, ref[torch.float32][0], ref[torch.float64][0], ref[torch.float64][1], 12, "train.py")
    fit = model.fit_lcccnn(m, x, y, max_epochs=3)
    tl = fit.train_loss.cpu().numpy()
    print(f"3 epochs: {tl.tolist()}, rates {fit.lrs.tolist()}")
    assert fit.epochs == 3 and np.isfinite(tl).all() and float(tl[0]) == float(loss)
    assert all(bool(torch.isfinite(p).all()) for p in m.parameters())


# ---- the recorded runs ----------------------------------------------------------------------------------------------
def load_case(g, case):
    from onset_fingerprinting_amd import model
    cfg = json.loads(str(g[f"{case}/cfg"]))
    kw = dict(cfg["kwargs"])
    kw["activation"], kw["loss"] = getattr(nn, kw["activation"]), getattr(F, kw["loss"])
    m = model.LCCCNN(cfg["width"], 2, channels=cfg["channels"], dropout_rate=0.0, lr=cfg["lr"], **kw)
    pre = f"{case}/sd0/"
    m.load_state_dict({k[len(pre):]: torch.from_numpy(g[k]) for k in g.files if k.startswith(pre)})
    x, y = torch.from_numpy(g[f"{case}/x"]), torch.from_numpy(g[f"{case}/y"])
    val = (torch.from_numpy(g[f"{case}/x_val"]), torch.from_numpy(g[f"{case}/y_val"])) if "n_val" in cfg else None
    return cfg, m, x, y, val


_runs = {}


def our_run(g, case):
    """fit_lcccnn on the golden's inputs and start, on the GPU; once per case and session."""
    from onset_fingerprinting_amd import model
    if case not in _runs:
        cfg, m, x, y, val = load_case(g, case)
        m = m.cuda()
        kw = dict(x_val=val[0].cuda(), y_val=val[1].cuda(), patience=cfg["patience"]) if val else {}
        fit = model.fit_lcccnn(m, x.cuda(), y.cuda(), max_epochs=cfg["epochs"], **kw)
        _runs[case] = (m, fit)
    return _runs[case]


def comparable_prefix(ref, pert):
    n = len(ref)
    with np.errstate(invalid="ignore"):
        spread = np.max(np.abs(pert[:, :n].astype(f64) - ref.astype(f64)), axis=0)
    bad = np.isnan(spread) | (spread > 1e-5 * ref)
    return (int(np.argmax(bad)) if bad.any() else n), spread


@pytest.mark.parametrize("case", CASES + [STOP])
def test_gradients_at_the_start(g, case):
    from onset_fingerprinting_amd import model
    cfg, m, x, y, _val = load_case(g, case)
    loss, grads = model.cccnn_loss_and_grads_device(m, x.cuda(), y.cuda())
    pre32, pre64 = f"{case}/g32/", f"{case}/g64/"
    g32 = {k[len(pre32):]: g[k] for k in g.files if k.startswith(pre32)}
    g64 = {k[len(pre64):]: g[k] for k in g.files if k.startswith(pre64)}
    check_grads(grads, loss, g32, g64, float(g[f"{case}/loss64"]), 2 * len(x), case)


@pytest.mark.parametrize("case", CASES + [STOP])
def test_trajectory_over_the_comparable_prefix(g, case):
    ref, ref64 = g[f"{case}/errors"], g[f"{case}/errors64"]
    prefix, spread = comparable_prefix(ref, g[f"{case}/pert_errors"])
    assert prefix >= (len(ref) if case == WHOLE else min(16, len(ref)))
    m, fit = our_run(g, case)
    ours = fit.train_loss.cpu().numpy()
    assert fit.epochs >= prefix and np.isfinite(ours[:fit.epochs]).all()
    assert np.array_equal(fit.lrs, g[f"{case}/rates"][:fit.epochs])
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
        mine = torch.cat([p.detach().reshape(-1) for p in m.parameters()]).cpu().numpy().astype(f64)
        rec = g[f"{case}/flat"].astype(f64)
        sp = np.max(np.abs(rec[1:] - rec[0]))
        err = np.max(np.abs(mine - rec[0]))
        b = max(4 * sp, U23 * np.max(np.abs(rec[0])))
        print(f"{case}: parameters max |ours - ref| {err:.3e}, spread of the disturbed runs {sp:.3e}, bound {b:.3e}")
        assert err <= b, (err, b)


def test_a_case_is_comparable_over_its_whole_length(g):
    assert comparable_prefix(g[f"{WHOLE}/errors"], g[f"{WHOLE}/pert_errors"])[0] == len(g[f"{WHOLE}/errors"])


@pytest.mark.parametrize("case", [c for c in CASES if c != WHOLE])
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
    later = stop + 7
    m2 = copy.deepcopy(start).cuda()
    fit2 = model.fit_lcccnn(m2, x.cuda(), y.cuda(), x_val=val[0].cuda(), y_val=val[1].cuda(),
                            max_epochs=cfg["epochs"], min_epochs=later, patience=cfg["patience"])
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
            monkeypatch.setenv("OFP_CCCNN_GRAPH", mode)
        m = copy.deepcopy(start).cuda()
        fit = model.fit_lcccnn(m, x.cuda(), y.cuda(), x_val=val[0].cuda(), y_val=val[1].cuda(), max_epochs=90)
        results.append((fit, torch.cat([t.detach().reshape(-1).float() for t in m.state_dict().values()])))
    monkeypatch.delenv("OFP_CCCNN_GRAPH", raising=False)
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
    it once.  The rate of epoch e depends on e alone (model.lcccnn_rates), not on max_epochs, so the losses of
    either run are the first of a 5-epoch run, bit for bit."""
    from onset_fingerprinting_amd import model
    _cfg, start, x, y, val = load_case(g, STOP)

    def run(epochs):
        fit = model.fit_lcccnn(copy.deepcopy(start).cuda(), x.cuda(), y.cuda(), x_val=val[0].cuda(),
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
    case = CASES[0]
    cfg, m, x, y, _val = load_case(g, case)
    before = {k: v.clone() for k, v in m.state_dict().items()}
    fit = model.fit_lcccnn(m, x, y, max_epochs=40)  # module and data on the CPU
    assert fit.epochs == 40 and fit.val_loss is None and not m.training
    assert fit.train_loss.shape == (40,) and bool(torch.isfinite(fit.train_loss).all())
    after = m.state_dict()
    assert all(not v.is_cuda for v in after.values())
    assert all(not torch.equal(before[k], after[k]) for k in before)
    # the same 40 epochs on a GPU copy of the start give the same bits
    m_gpu = load_case(g, case)[1].cuda()
    fit_gpu = model.fit_lcccnn(m_gpu, x.cuda(), y.cuda(), max_epochs=40)
    assert all(torch.equal(after[k], v.cpu()) for k, v in m_gpu.state_dict().items())
    assert torch.equal(fit.train_loss.view(torch.int32), fit_gpu.train_loss.view(torch.int32))
    # a second call continues from the new parameters: its first loss is the loss of the module as it stands
    loss_now, _g = model.cccnn_loss_and_grads_device(m, x, y)
    again = model.fit_lcccnn(m, x, y, max_epochs=5)
    assert float(again.train_loss[0]) == float(loss_now)
    assert float(again.train_loss[0]) < float(fit.train_loss[0])
    # NaN beyond the epochs run
    short = model.fit_lcccnn(load_case(g, case)[1], x, y, max_epochs=12, min_epochs=3)
    assert short.epochs == 12 and bool(torch.isfinite(short.train_loss).all())


# ---- the epoch past one slab, one chunk and 256 validation windows --------------------------------------------------
def epoch_start():
    """Width 30 with GroupNorm, 3 sensors, n = 130 (390 items, six slabs; three chunks), n_val = 300 > n and > the
    loss kernel's 256 threads: the work space is sized by the validation batch."""
    from onset_fingerprinting_amd import model
    torch.manual_seed(130)
    m = model.LCCCNN(30, 2, channels=3, dropout_rate=0.0, layer_sizes=[3, 2], batch_norm=True)
    with torch.no_grad():
        for mod in m.model.conv_layers:
            if isinstance(mod, nn.GroupNorm):
                mod.weight.mul_(0.2)
    return m, torch.randn(130, 3, 30), torch.randn(130, 2), torch.randn(300, 3, 30), torch.randn(300, 2)


def test_one_epoch_with_a_validation_batch_larger_than_the_training_batch():
    from onset_fingerprinting_amd import model
    m, x, y, xv, yv = epoch_start()
    m = m.cuda()
    loss0, _g = model.cccnn_loss_and_grads_device(m, x.cuda(), y.cuda())
    fit = model.fit_lcccnn(m, x.cuda(), y.cuda(), x_val=xv.cuda(), y_val=yv.cuda(), max_epochs=1)
    assert fit.epochs == 1
    assert float(fit.train_loss[0]) == float(loss0)
    ref = {}
    for dtype in (torch.float32, torch.float64):
        net = copy.deepcopy(m).cpu().to(dtype).eval()
        with torch.no_grad():
            out, probs = torch_forward(net.model, xv.to(dtype))
            ref[dtype] = float(F.l1_loss(out, yv.to(dtype)))
        assert float(probs.max()) < 0.9
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
            monkeypatch.setenv("OFP_CCCNN_GRAPH", mode)
        m = copy.deepcopy(start).cuda()
        fit = model.fit_lcccnn(m, x.cuda(), y.cuda(), x_val=xv.cuda(), y_val=yv.cuda(), max_epochs=5)
        results.append((fit, torch.cat([t.detach().reshape(-1).float() for t in m.state_dict().values()])))
    monkeypatch.delenv("OFP_CCCNN_GRAPH", raising=False)
    (a, pa) = results[0]
    assert a.epochs == 5 and bool(torch.isfinite(a.train_loss).all()) and bool(torch.isfinite(a.val_loss).all())
    for b, pb in results[1:]:
        assert b.epochs == 5 and torch.equal(pa, pb)
        assert torch.equal(a.train_loss.view(torch.int32), b.train_loss.view(torch.int32))
        assert torch.equal(a.val_loss.view(torch.int32), b.val_loss.view(torch.int32))
