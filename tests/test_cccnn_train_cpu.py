"""CPU-only: the host side of fit_lcccnn (model.py) and the float64 references of tests/cccnn_train_ref.py.

  references   equal torch autograd in float64 (F.conv1d with stride, F.group_norm (+ max_pool1d), the head written
               with F.conv1d as the reference writes it, torch.optim.SGD over 5 steps)
  bounds       a numpy float32 emulation of each kernel's arithmetic lies inside its bound, and a planted fault
               (a dropped last tap, stride ignored, the lag-0 factor 1 instead of 2, s2 left out, weight decay
               skipped) lies outside
  host side    lcccnn_rates against a real SGD + CosineAnnealingLR(100) run, configure_optimizers, every ValueError
               of the limits raised before any GPU call, the g27_cccnn_train fixture's own conditions"""
import json
import sys
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

sys.path.insert(0, str(Path(__file__).resolve().parent))
import cccnn_train_ref as R  # noqa: E402

f32, f64 = np.float32, np.float64
CASES = ["shared_gn_l1_silu", "grouped_strided_l1", "shared_gn_pool_mse_tanh_dil", "shared_gn_l1_silu_stop"]
T64 = lambda a, grad=False: torch.tensor(np.asarray(a, f64), dtype=torch.float64, requires_grad=grad)


def close(a, b, tol=1e-10):
    return np.max(np.abs(a - b)) <= tol * max(1.0, np.max(np.abs(b))) if np.size(a) else True


def inside(got, ref_bound):
    ref, bound = ref_bound
    return bool(np.all(np.abs(np.asarray(got, f64) - ref) <= bound))


# ---- the references against autograd ---------------------------------------------------------------------------------
CONV = [(3, 1, 1, 1, 1, 2, 3, 9, 3), (5, 2, 1, 1, 4, 4, 8, 33, 2), (3, 3, 2, 2, 1, 2, 3, 34, 2), (4, 4, 1, 0, 2, 4, 4, 19, 3),
        (64, 1, 1, 0, 1, 1, 2, 64, 2), (1, 1, 1, 0, 1, 1, 5, 7, 3)]


def conv_data(k, stride, dil, pad, groups, cin, cout, w, n):
    rng = np.random.default_rng([k, stride, dil, pad, groups, cin, cout, w, n])
    wc = R.conv_width(w, k, pad, dil, stride)
    return (rng.standard_normal((n, cin, w)).astype(f32), rng.standard_normal((cout, cin // groups, k)).astype(f32),
            rng.standard_normal((n, cout, wc)).astype(f32))


@pytest.mark.parametrize("case", CONV, ids=str)
def test_conv_reference_against_autograd(case):
    k, stride, dil, pad, groups, cin, cout, w, n = case
    x, wt, dz = conv_data(*case)
    ref = R.conv1d_backward_strided_ref(x, wt, dz, pad, dil, groups, stride)
    xt, wtt, b = T64(x, True), T64(wt, True), torch.zeros(cout, dtype=torch.float64, requires_grad=True)
    F.conv1d(xt, wtt, b, stride=stride, padding=pad, dilation=dil, groups=groups).backward(T64(dz))
    for name, t in (("dx", xt), ("dw", wtt), ("db", b)):
        val, bound = ref[name]
        assert val.shape == tuple(t.shape) == bound.shape and np.all(bound >= 0)
        assert close(val, t.grad.numpy(), 1e-12), name


def gn_data(K, V, items, pool, offset=0.0):
    rng = np.random.default_rng([K, V, items, int(pool)])
    x = (rng.standard_normal((items, K, V)) * 1.5 + 0.3 + offset).astype(f32)
    ga, be = rng.uniform(0.5, 1.5, K).astype(f32) * rng.choice([-1, 1], K).astype(f32), rng.standard_normal(K).astype(f32)
    dy = rng.standard_normal((items, K, V // 2 if pool else V)).astype(f32)
    return x, ga, be, dy


@pytest.mark.parametrize("K,V,items,pool", [(5, 7, 3, False), (5, 7, 3, True), (1, 1, 2, False), (2, 8, 4, True)])
def test_groupnorm_reference_against_autograd(K, V, items, pool):
    x, ga, be, dy = gn_data(K, V, items, pool)
    fwd = R.groupnorm1_train_forward_ref(x, ga, be, 1e-5, pool)
    bwd = R.groupnorm1_train_backward_ref(x, ga, be, dy, 1e-5, pool)
    xt, gt, bt = T64(x, True), T64(ga, True), T64(be, True)
    y = F.group_norm(xt, 1, gt, bt, 1e-5)
    if pool:
        y = F.max_pool1d(y, 2, 2)
    y.backward(T64(dy))
    assert close(fwd["y"][0], y.detach().numpy())
    assert close(fwd["mean"][0], x.astype(f64).mean((1, 2)))
    assert close(fwd["rstd"][0], 1 / np.sqrt(x.astype(f64).var((1, 2)) + 1e-5))
    assert close(bwd["dx"][0], xt.grad.numpy(), 1e-9) and close(bwd["dgamma"][0], gt.grad.numpy(), 1e-9)
    assert close(bwd["dbeta"][0], bt.grad.numpy(), 1e-9)
    for d in (fwd, bwd):
        for val, bound in d.values():
            assert bound.shape == val.shape and np.all(bound >= 0)


def head_data(K, V, n, C, O, scale=None):
    rng = np.random.default_rng([K, V, n, C, O])
    scale = 1.0 / np.sqrt(K * V) if scale is None else scale  # cc of order 1: the softmax is spread out
    f = (rng.standard_normal((n * C, K, V)) * scale).astype(f32)
    dout = rng.standard_normal((n, O)).astype(f32)
    wfc = rng.standard_normal((O, C * (2 * V - 1))).astype(f32)
    return f, dout, wfc


def head_torch(f, wfc, n, C):
    """model.py:524-538 on maps f [n * C, K, V] (float64 tensors): -> out [n, O] without the bias."""
    BC, K, V = f.shape
    cc_raw = F.conv1d(f.reshape(1, BC * K, V), f.reshape(BC * K, 1, V), groups=BC * K, padding=V - 1)
    cc = cc_raw.view(BC, K, -1).sum(dim=1)
    probs = torch.flatten(F.softmax(cc, dim=-1).view(n, C, -1), start_dim=1)
    return probs @ wfc.t(), probs


@pytest.mark.parametrize("K,V,n,C,O", [(1, 1, 2, 1, 2), (1, 2, 1, 3, 2), (5, 7, 2, 2, 2), (2, 9, 1, 2, 3)])
def test_head_reference_against_autograd(K, V, n, C, O):
    f, dout, wfc = head_data(K, V, n, C, O)
    df, bound = R.autocorr_softmax_backward_ref(f, dout, wfc, C)
    ft = T64(f, True)
    out, probs = head_torch(ft, T64(wfc), n, C)
    out.backward(T64(dout))
    assert close(R.autocorr_softmax_f64(f)[1], probs.detach().numpy().reshape(n * C, -1), 1e-12)
    assert close(df, ft.grad.numpy(), 1e-11) and bound.shape == df.shape and np.all(bound >= 0)
    if V == 1:
        assert np.all(df == 0)  # one lag: p = 1 whatever the maps are


def test_sgd_reference_against_torch():
    """Five steps of torch.optim.SGD(momentum 0.8, weight decay 1e-3) in float64, the first included, at the rates of
    the schedule; and lcccnn_rates against a real SGD + CosineAnnealingLR(100) run over 250 steps."""
    from onset_fingerprinting_amd import model
    steps, lr = 250, 0.0017
    rates = model.lcccnn_rates(lr, steps)
    assert rates.dtype == np.float64 and rates.shape == (steps,)
    torch.manual_seed(2)
    p = nn.Parameter(torch.randn(40, dtype=torch.float64))
    q, buf = p.detach().numpy().copy(), np.zeros(40)
    opt = torch.optim.SGD([p], lr=lr * 100, momentum=0.8, weight_decay=1e-3)
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, 100)
    for e in range(steps):
        assert opt.param_groups[0]["lr"] == rates[e], e
        if e < 5:
            grad = torch.randn(40, dtype=torch.float64)
            p.grad = grad.clone()
            opt.step()
            out = R.sgd_step_ref(q, grad.numpy(), buf, rates[e], e == 0, 0.8, 1e-3)
            q, buf = out["p"][0], out["buf"][0]
            assert close(q, p.detach().numpy(), 1e-14), e
            assert close(buf, opt.state[p]["momentum_buffer"].numpy(), 1e-14), e
        else:
            opt.step()
        sched.step()
    assert rates[0] == lr * 100 and rates[100] == 0.0 and rates[101] > 0 and abs(rates[200] - lr * 100) < 1e-12
    assert (model.LCCCNN_MOMENTUM, model.LCCCNN_WEIGHT_DECAY) == (0.8, 1e-3)


def lanes_per_output(outputs):
    """csrc/ofp_train_chain.h: the largest power of two <= 64 with outputs * g <= 256 threads."""
    g = 64
    while g > 1 and outputs * g > 256:
        g >>= 1
    return g


def test_lane_cases_sit_on_both_sides_of_every_change_of_g():
    """R.WGRAD_LANE_CASES, which the GPU test of the strided convolution's gradients runs: every lane count, both
    neighbours of every change (127 for the unreachable 128), the second pass above 256 outputs, one slab except for
    one case each with g = 4 and g = 2, and limits that the strided entry accepts."""
    per_g, slabs_of_g = {}, {}
    for k, stride, dil, pad, groups, cin, cout, w, n in R.WGRAD_LANE_CASES:
        assert 1 <= k <= 64 and 1 <= stride <= 4 and cin % groups == 0 and cout % groups == 0 and cout == 2
        assert 1 <= cin <= 64 and 1 <= w <= 1024 and 1 <= n <= 4096
        T = cin // groups * k + 1
        pairs = n * R.conv_width(w, k, pad, dil, stride)
        assert pairs % 64 and pairs >= 1
        g = lanes_per_output(T)
        per_g.setdefault(g, set()).add(T)
        slabs_of_g.setdefault(g, set()).add(-(-pairs // 2048))
    assert sorted(per_g) == [1, 2, 4, 8, 16, 32, 64]
    Ts = set().union(*per_g.values())
    assert Ts == {4, 5, 8, 9, 16, 17, 32, 33, 64, 65, 127, 129, 256, 257}
    for lo in (4, 8, 16, 32, 64):
        assert lanes_per_output(lo) == 2 * lanes_per_output(lo + 1)
    assert lanes_per_output(127) == lanes_per_output(128) == 2 and lanes_per_output(129) == 1
    assert all(127 % d for d in range(2, 127))  # T = 128 would need cin / groups * k = 127 with both factors <= 64
    assert {g: s for g, s in slabs_of_g.items()} == {64: {1}, 32: {1}, 16: {1}, 8: {1}, 4: {1, 2}, 2: {1, 2}, 1: {1}}
    # the references of the new shapes against autograd, at the cheapest of them
    test_conv_reference_against_autograd(R.WGRAD_LANE_CASES[3])


# ---- float32 emulations of the kernels, and planted faults -----------------------------------------------------------
def emul_conv(x, w, dz, pad, dil, groups, stride, drop_last_tap=False, ignore_stride=False):
    n, cin, win = x.shape
    cout, cin_g, k = w.shape
    wc, cout_g = dz.shape[2], cout // groups
    dw, db, dx = np.zeros(w.shape, f64), np.zeros(cout, f64), np.zeros(x.shape, f32)
    st, taps = (1 if ignore_stride else stride), (k - 1 if drop_last_tap else k)
    for s in range(n):
        for o in range(cout):
            c0 = (o // cout_g) * cin_g
            for p in range(wc):
                d = dz[s, o, p]
                db[o] += float(d)
                for ci in range(cin_g):
                    for kk in range(taps):
                        xi = p * st - pad + kk * dil
                        if 0 <= xi < win:
                            dw[o, ci, kk] += float(d) * float(x[s, c0 + ci, xi])
                            dx[s, c0 + ci, xi] = f32(dx[s, c0 + ci, xi] + f32(d * w[o, ci, kk]))
    return {"dx": dx, "dw": dw.astype(f32), "db": db.astype(f32)}


@pytest.mark.parametrize("case", [(3, 2, 1, 1, 1, 2, 3, 11, 2), (4, 3, 2, 2, 2, 4, 4, 17, 2)], ids=str)
def test_conv_emulation_inside_the_bound_and_faults_outside(case):
    k, stride, dil, pad, groups, cin, cout, w, n = case
    x, wt, dz = conv_data(*case)
    ref = R.conv1d_backward_strided_ref(x, wt, dz, pad, dil, groups, stride)
    good = emul_conv(x, wt, dz, pad, dil, groups, stride)
    assert all(inside(good[name], ref[name]) for name in ref)
    tap = emul_conv(x, wt, dz, pad, dil, groups, stride, drop_last_tap=True)
    assert not inside(tap["dx"], ref["dx"]) and not inside(tap["dw"], ref["dw"])
    flat = emul_conv(x, wt, dz, pad, dil, groups, stride, ignore_stride=True)
    assert not inside(flat["dx"], ref["dx"]) and not inside(flat["dw"], ref["dw"])


def emul_gn(x, ga, be, eps, dy, pool, no_s2=False):
    items, K, V = x.shape
    N = K * V
    xd = x.astype(f64)
    m = xd.sum((1, 2)) / N
    var = np.maximum((xd * xd).sum((1, 2)) / N - m * m, 0.0)
    mean, rstd = m.astype(f32), (1.0 / np.sqrt(var + eps)).astype(f32)
    xh = ((x - mean[:, None, None]).astype(f32) * rstd[:, None, None]).astype(f32)
    y = ((xh * ga[None, :, None]).astype(f32) + be[None, :, None]).astype(f32)
    dyf = dy
    if pool:
        y, take = R._pool(y)
        dyf = R._unpool(dy, take).astype(f32)
    dh = (dyf * ga[None, :, None]).astype(f32)
    c1 = (dh.astype(f64).sum((1, 2)) / N).astype(f32)
    c2 = ((dh.astype(f64) * xh.astype(f64)).sum((1, 2)) / N).astype(f32)
    if no_s2:
        c2 = np.zeros_like(c2)
    t = ((dh - c1[:, None, None]).astype(f32) - (xh * c2[:, None, None]).astype(f32)).astype(f32)
    dx = (t * rstd[:, None, None]).astype(f32)
    dgamma = (dyf.astype(f64) * xh.astype(f64)).sum((0, 2)).astype(f32)
    dbeta = dyf.astype(f64).sum((0, 2)).astype(f32)
    return {"y": y, "mean": mean, "rstd": rstd}, {"dx": dx, "dgamma": dgamma, "dbeta": dbeta}


@pytest.mark.parametrize("K,V,items,pool,offset", [(5, 7, 3, False, 0.0), (5, 7, 3, True, 0.0), (1, 1, 2, False, 0.0),
                                                   (2, 257, 3, False, 1000.0)])
def test_groupnorm_emulation_inside_the_bound_and_fault_outside(K, V, items, pool, offset):
    x, ga, be, dy = gn_data(K, V, items, pool, offset)
    fwd = R.groupnorm1_train_forward_ref(x, ga, be, 1e-5, pool)
    bwd = R.groupnorm1_train_backward_ref(x, ga, be, dy, 1e-5, pool)
    ef, eb = emul_gn(x, ga, be, 1e-5, dy, pool)
    assert all(inside(ef[name], fwd[name]) for name in fwd), [name for name in fwd if not inside(ef[name], fwd[name])]
    assert all(inside(eb[name], bwd[name]) for name in bwd), [name for name in bwd if not inside(eb[name], bwd[name])]
    if K * V > 1:
        _f, bad = emul_gn(x, ga, be, 1e-5, dy, pool, no_s2=True)
        assert not inside(bad["dx"], bwd["dx"])


def emul_head(f, p32, dout, wfc, C, lag0=2.0):
    items, K, V = f.shape
    L, O = 2 * V - 1, dout.shape[1]
    df = np.zeros(f.shape, f32)
    for it in range(items):
        b, c = divmod(it, C)
        dp = np.zeros(L, f32)
        for o in range(O):
            dp = (dp + (dout[b, o] * wfc[o, c * L:(c + 1) * L]).astype(f32)).astype(f32)
        dot = f32((p32[it].astype(f64) * dp.astype(f64)).sum())
        dcc = (p32[it] * (dp - dot).astype(f32)).astype(f32)
        g = (dcc + dcc[::-1]).astype(f32)
        g[V - 1] = f32(f32(lag0) * dcc[V - 1])
        for m in range(V):
            acc = np.zeros(K, f32)
            for i in range(V):
                acc = (acc + (g[i - m + V - 1] * f[it, :, i]).astype(f32)).astype(f32)
            df[it, :, m] = acc
    return df


@pytest.mark.parametrize("K,V,n,C,O,scale", [(1, 2, 1, 3, 2, None), (5, 7, 2, 2, 2, None), (2, 33, 1, 2, 3, None),
                                             (2, 9, 2, 2, 2, 30.0)])
def test_head_emulation_inside_the_bound_and_fault_outside(K, V, n, C, O, scale):
    f, dout, wfc = head_data(K, V, n, C, O, scale)
    ref = R.autocorr_softmax_backward_ref(f, dout, wfc, C)
    p32 = R.autocorr_softmax_f64(f)[1].astype(f32)
    assert inside(emul_head(f, p32, dout, wfc, C), ref)
    if scale is None:  # (saturated, the lag 0 takes everything and its dcc cancels: nothing to plant there)
        assert not inside(emul_head(f, p32, dout, wfc, C, lag0=1.0), ref)


def emul_sgd(p, g, buf, lr, first, mom, wd, skip_wd=False):
    gr = g if skip_wd else (g + (wd * p).astype(f32)).astype(f32)
    b1 = gr if first else ((mom * buf).astype(f32) + gr).astype(f32)
    return {"p": (p - (lr * b1).astype(f32)).astype(f32), "buf": b1}


@pytest.mark.parametrize("first,lr", [(True, 0.3), (False, 0.17), (False, 0.0)])
def test_sgd_emulation_inside_the_bound_and_fault_outside(first, lr):
    rng = np.random.default_rng(int(first) + 3)
    p, g = rng.standard_normal(500).astype(f32), (rng.standard_normal(500) * 0.01).astype(f32)
    buf = (rng.standard_normal(500) * 0.01).astype(f32)
    lr, mom, wd = f32(lr), f32(0.8), f32(1e-3)
    ref = R.sgd_step_ref(p, g, buf, lr, first, mom, wd)
    good = emul_sgd(p, g, buf, lr, first, mom, wd)
    assert inside(good["p"], ref["p"]) and inside(good["buf"], ref["buf"])
    bad = emul_sgd(p, g, buf, lr, first, mom, wd, skip_wd=True)
    assert not inside(bad["buf"], ref["buf"])
    if lr == 0:
        assert np.array_equal(good["p"], p) and np.all(ref["p"][1] == 0)
    else:
        assert not inside(bad["p"], ref["p"])


# ---- the host side of fit_lcccnn -------------------------------------------------------------------------------------
def test_configure_optimizers_mirrors_the_reference():
    from onset_fingerprinting_amd import model
    m = model.LCCCNN(32, 2, dropout_rate=0.0, lr=0.002)
    conf = m.configure_optimizers()
    opt, sched = conf["optimizer"], conf["lr_scheduler"]
    assert type(opt) is torch.optim.SGD
    group = opt.param_groups[0]
    assert group["lr"] == 0.002 * 100 and group["momentum"] == 0.8 and group["weight_decay"] == 1e-3
    assert group["dampening"] == 0 and group["nesterov"] is False
    assert sum(p.numel() for p in group["params"]) == sum(p.numel() for p in m.parameters())
    assert type(sched["scheduler"]) is torch.optim.lr_scheduler.CosineAnnealingLR
    assert (sched["scheduler"].T_max, sched["frequency"], sched["monitor"]) == (100, 1, "val_loss")


def test_argument_errors_come_before_any_gpu_call(monkeypatch):
    from onset_fingerprinting_amd import _lib, model

    def no_gpu(*a, **k):
        raise AssertionError("a GPU call was made")

    monkeypatch.setattr(_lib, "require_gpu", no_gpu)
    monkeypatch.setattr(_lib, "lib", no_gpu)
    M = lambda *a, **k: model.LCCCNN(*a, **{"dropout_rate": 0.0, **k})
    x, y = torch.zeros(8, 3, 32), torch.zeros(8, 2)
    for call in (model.fit_lcccnn, model.cccnn_loss_and_grads_device):
        with pytest.raises(ValueError, match="dropout_rate=0.0"):
            call(model.LCCCNN(32, 2), x, y)  # the class default is 0.5
        with pytest.raises(ValueError, match="l1_loss"):
            call(M(32, 2, loss=F.smooth_l1_loss), x, y)
        with pytest.raises(ValueError, match="limit is 1..8"):
            call(M(32, 2, layer_sizes=[2] * 9, kernel_sizes=1), x, y)
        with pytest.raises(ValueError, match="kernel size 65"):
            call(M(128, 2, layer_sizes=[2], kernel_sizes=[65]), torch.zeros(8, 3, 128), y)
        with pytest.raises(ValueError, match="stride 5"):
            call(M(32, 2, layer_sizes=[2], strides=[5]), x, y)
        with pytest.raises(ValueError, match="65 channels"):
            call(M(32, 2, layer_sizes=[65]), x, y)
        with pytest.raises(ValueError, match="68 channels"):
            call(M(32, 2, channels=4, layer_sizes=[17], group=True), torch.zeros(8, 4, 32), y)
        with pytest.raises(ValueError, match="512"):
            call(M(513, 2), torch.zeros(8, 3, 513), y)
        with pytest.raises(ValueError, match="1024"):
            call(M(32, 2), torch.zeros(1025, 3, 32), torch.zeros(1025, 2))
        with pytest.raises(ValueError, match="4096"):
            call(M(32, 2, channels=5), torch.zeros(1000, 5, 32), torch.zeros(1000, 2))
        with pytest.raises(ValueError, match="16 outputs"):
            call(M(32, 17), x, torch.zeros(8, 17))
        with pytest.raises(ValueError, match="LDS"):
            call(M(512, 2, layer_sizes=[64], kernel_sizes=1, padding=64), torch.zeros(8, 3, 512), y)
        with pytest.raises(ValueError, match="leaves no column"):
            call(M(32, 2, layer_sizes=[2], kernel_sizes=[12]), torch.zeros(8, 3, 8), y)
        with pytest.raises(ValueError, match="features"):
            call(M(32, 2), torch.zeros(8, 3, 40), y)
        with pytest.raises(ValueError, match="LCCCNN"):
            call(model.CCCNN(32, 2, dropout_rate=0.0), x, y)
        m = M(32, 2)
        m.model.conv_layers.act1 = nn.GELU()
        with pytest.raises(ValueError, match="GELU"):
            call(m, x, y)
    with pytest.raises(ValueError, match="patience"):
        model.fit_lcccnn(M(32, 2), x, y, patience=3)
    with pytest.raises(ValueError, match="go together"):
        model.fit_lcccnn(M(32, 2), x, y, x_val=x)
    with pytest.raises(ValueError, match="max_epochs"):
        model.fit_lcccnn(M(32, 2), x, y, max_epochs=0)


def test_the_reference_training_configuration_is_inside_the_limits():
    """train.py's own model with up to 620 windows of 4 sensors."""
    from onset_fingerprinting_amd import model
    m = model.LCCCNN(256, 2, 4, layer_sizes=[5] * 7, kernel_sizes=[1, 33, 64, 15, 15, 15, 1], dropout_rate=0.0,
                     batch_norm=True, loss=F.l1_loss, lr=0.001, group=False)
    _x, _y, cfg = model._cccnn_batch(m, torch.zeros(620, 4, 256), torch.zeros(620, 2))
    assert (cfg.n_conv, cfg.sensors, cfg.norm, cfg.group, cfg.width) == (7, 4, 1, 0, 256)
    assert list(cfg.kernels)[:7] == [1, 33, 64, 15, 15, 15, 1] and m.model.fc.in_features == 4 * (2 * 133 - 1)
    assert model.cccnn_head_lds_bytes(5, 133) <= model.CCCNN_TRAIN_MAX_LDS
    names = [n for n, _t in model._cccnn_tensors(m)]
    assert names == [n for n, _p in m.named_parameters()]


# ---- the fixture -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def g(golden):
    return golden("g27_cccnn_train")


def comparable_prefix(ref, pert):
    n = len(ref)
    with np.errstate(invalid="ignore"):
        spread = np.max(np.abs(pert[:, :n].astype(f64) - ref.astype(f64)), axis=0)
    bad = np.isnan(spread) | (spread > 1e-5 * ref)
    return (int(np.argmax(bad)) if bad.any() else n), spread


@pytest.mark.parametrize("case", CASES)
def test_fixture_conditions(g, case):
    from onset_fingerprinting_amd import model
    cfg = json.loads(str(g[f"{case}/cfg"]))
    ref = g[f"{case}/errors"]
    prefix, _s = comparable_prefix(ref, g[f"{case}/pert_errors"])
    g64 = {k: float(np.max(np.abs(g[k]))) for k in g.files if k.startswith(f"{case}/g64/")}
    share = min(g64.values()) / max(g64.values())
    print(f"{case}: prefix {prefix} of {len(ref)}, loss {ref[0]:.5g} -> best {ref.min():.5g}, smallest share of the "
          f"gradient {share:.3g}")
    assert share >= 1e-3 and g[f"{case}/pert_errors"].shape[0] == 8
    assert prefix >= (len(ref) if cfg.get("full_prefix") else min(16, len(ref)))
    assert ref.min() * 1.2 <= ref[0]
    assert np.array_equal(model.lcccnn_rates(cfg["lr"], cfg["epochs"])[:len(ref)], g[f"{case}/rates"])
    if "patience" in cfg:
        stop = int(g[f"{case}/stop"])
        assert stop < cfg["epochs"] and np.all(g[f"{case}/pert_stop"] == stop)
        assert len(g[f"{case}/val"]) == stop == len(ref) == len(g[f"{case}/val64"])
        best, wait = np.inf, 0  # the rule of fit_lcccnn's docstring on the recorded validation curve
        for e, v in enumerate(g[f"{case}/val"]):
            best, wait = (v, 0) if v < best else (best, wait + 1)
            if wait >= cfg["patience"]:
                break
        assert e + 1 == stop
    else:
        assert len(ref) == cfg["epochs"] >= 300
    kw = dict(cfg["kwargs"])
    kw["activation"], kw["loss"] = getattr(nn, kw["activation"]), getattr(F, kw["loss"])
    m = model.LCCCNN(cfg["width"], 2, channels=cfg["channels"], dropout_rate=0.0, lr=cfg["lr"], **kw)
    pre = f"{case}/sd0/"
    m.load_state_dict({k[len(pre):]: torch.from_numpy(g[k]) for k in g.files if k.startswith(pre)})
