"""GPU: training model.CNNRNN (csrc/ofp_cnnrnn_train.hip, model.fit_cnnrnn) against float64 references, torch, and the
reference's recorded runs (tests/golden/g28_cnnrnn_train.npz, made by make_golden_cnnrnn_train.py).

  linear      ofp_linear_backward element-wise against float64 with the derived bound (N + 4) u sum |terms|
  gru         forward and back-propagation through time against torch's float64 nn.GRU; per tensor max |ours - ref64|
              <= 4 x max |torch float32 - ref64|, floored at 2^-22 x max |ref64|; random and saturated inputs
  attention   the same rule against torch's float64 nn.MultiheadAttention (out_proj set to the identity) averaged over
              time; with dropout the site-3 mask bit for bit against numpy and the values against the float64
              reference with that mask (the float32 yardstick: the same formulas in torch float32)
  gradients   per tensor, max |ours - g64| <= 4 x max |g32 - g64|, floored at 2^-23 x max |g64|
  epoch       first losses against torch float64, graph replay against plain launches and two fits, bit for bit
  trajectory, outcome, stop, dropout, window source: the rules of tests/test_gpu_cnn_train.py
Every figure is printed before it is asserted (run with -s to see them).  Outputs of the directly called kernels go
into NaN-filled buffers with a guard tail.

Switches of the kernels and the shapes on both sides of each:
  k_lin_wgrad_partial   slabs of 256 rows (rows 255, 256, 257, 2049); 8 outputs per workgroup (out 3, 8, 9, 192);
                        256 of the in + 1 columns per workgroup (in 255 fills one, 256 and 257 need two)
  k_lin_fwd             tiles of 8 rows (rows 1, 63, 64, 65); inputs staged 128 at a time (the GRU's F = 5, 33, 257;
                        dx of the Linear backward sums over `out` = 3, 192); 256 outputs per workgroup (3H = 384)
  k_gru_fwd / _bwd      256 // H sequences per workgroup: H = 1 (256; n = 1 and 257), 6 (42, 4 threads idle; n = 5
                        and 43), 64 (4; n = 65), 128 (2; n = 3); no weights in LDS and no chunked time loop
  k_attn_fwd / _bwd     one (sequence, head) per workgroup; rows and columns go round the 256 threads (T = 1 .. 128)
"""
import copy
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

sys.path.insert(0, str(Path(__file__).resolve().parent))
import cnnrnn_train_ref as R  # noqa: E402
import train_random_ref as RR  # noqa: E402

pytestmark = pytest.mark.gpu

REPO = Path(__file__).resolve().parents[1]
CASES = ["l1_silu", "mse_tanh_bn_pool", "l1_silu_bn_wide"]
STOP = "l1_silu_stop"
U24, U23, U22 = 2.0 ** -24, 2.0 ** -23, 2.0 ** -22
GUARD = 64
f32, f64 = np.float32, np.float64


@pytest.fixture(scope="module")
def g(golden):
    return golden("g28_cnnrnn_train")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, f32)).cuda()


def guarded(*shape):
    numel = int(np.prod(shape))
    buf = torch.full((numel + GUARD,), float("nan"), dtype=torch.float32, device="cuda")
    return buf[:numel].view(*shape), buf


def guard_ok(name, buf, ctx):
    assert bool(torch.isnan(buf[-GUARD:]).all()), (name, ctx, "store past the end of the output")
    assert not bool(torch.isnan(buf[:-GUARD]).any()), (name, ctx, "an element of the output was not written")


def within(name, got, ref, bound, ctx, buf):
    """Element-wise |got - ref| <= bound (NaN fails); the guard tail behind the output is untouched."""
    guard_ok(name, buf, ctx)
    got = got.detach().cpu().numpy().astype(f64)
    assert got.shape == ref.shape, (name, ctx, got.shape, ref.shape)
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = float(np.max(np.where(np.isnan(err) | ((bound == 0) & (err > 0)), np.inf,
                                      np.where(bound > 0, err / bound, 0.0))))
    print(f"{ctx} {name}: largest error / bound {ratio:.3g}, largest error {float(np.nanmax(err)):.3e}")
    assert bool((err <= bound).all()), (name, ctx, f"error / bound = {ratio:.3g}")


def against_torch(name, got, ref64, t32, ctx, buf=None, floor=U22):
    """max |ours - ref64| <= 4 x max |torch float32 - ref64|, floored at `floor` x max |ref64|."""
    if buf is not None:
        guard_ok(name, buf, ctx)
    got = got.detach().cpu().numpy().astype(f64)
    ref64, t32 = np.asarray(ref64, f64), np.asarray(t32, f64)
    assert got.shape == ref64.shape, (name, ctx, got.shape, ref64.shape)
    err, err32 = float(np.max(np.abs(got - ref64))), float(np.max(np.abs(t32 - ref64)))
    bound = max(4 * err32, floor * float(np.max(np.abs(ref64))))
    print(f"{ctx} {name}: |ours - ref64| {err:.3e}  |torch32 - ref64| {err32:.3e}  bound {bound:.3e}  error / bound "
          f"{err / bound if bound else 0:.3g}")
    assert np.isfinite(err) and err <= bound, (name, ctx, err, bound)


# ---- the Linear backward --------------------------------------------------------------------------------------------
LIN_ROWS, LIN_IN, LIN_OUT = (1, 63, 64, 65, 255, 256, 257, 2049), (1, 7, 255, 256, 257), (1, 3, 8, 9, 192)
LIN_SHAPES = sorted({(r, 7, 3) for r in LIN_ROWS} | {(65, i, 3) for i in LIN_IN} | {(65, 7, o) for o in LIN_OUT}
                    | {(1, 1, 1), (2049, 257, 192), (257, 256, 9)})


def check_linear(shape, need_dx=True):
    from onset_fingerprinting_amd import model
    rows, n_in, n_out = shape
    rng = np.random.default_rng(list(shape))
    x, w, dy = (rng.standard_normal(s).astype(f32) for s in ((rows, n_in), (n_out, n_in), (rows, n_out)))
    ref = R.linear_backward_ref(x, w, dy)
    (dx, bx), (dw, bw), (db, bb) = guarded(rows, n_in), guarded(n_out, n_in), guarded(n_out)
    model.linear_backward(dev(x), dev(w), dev(dy), out=(dx, dw, db), need_dx=need_dx)
    torch.cuda.synchronize()
    ctx = f"linear rows{rows} in{n_in} out{n_out}"
    if need_dx:
        within("dx", dx, *ref["dx"], ctx, bx)
    else:
        assert bool(torch.isnan(bx).all()), "dx was written although it was not asked for"
    within("dw", dw, *ref["dw"], ctx, bw)
    within("db", db, *ref["db"], ctx, bb)


@pytest.mark.parametrize("shape", LIN_SHAPES, ids=lambda s: "r{}_i{}_o{}".format(*s))
def test_linear_backward(shape):
    check_linear(shape)


def test_linear_backward_without_dx_and_refusals():
    from onset_fingerprinting_amd import _lib, model
    assert int(_lib.lib().ofp_linear_backward_slab()) == 256
    check_linear((257, 9, 5), need_dx=False)
    L = _lib.lib()
    for args in ((0, 3, 3), (3, 0, 3), (3, 3, 0), (3, 4097, 3), ((1 << 20) + 1, 3, 3)):
        assert L.ofp_linear_backward_workspace_bytes(*args) == -1
    one = torch.ones(16, device="cuda")
    with pytest.raises(ValueError, match="limits"):
        model.linear_backward(one[:0].view(0, 4), one[:8].view(2, 4), one[:0].view(0, 2))


# ---- the GRU --------------------------------------------------------------------------------------------------------
GRU_SHAPES = [(1, 1, 1, 1), (3, 2, 7, 2), (2, 16, 32, 8), (5, 17, 33, 6), (65, 3, 9, 64), (2, 128, 5, 4),
              (3, 4, 257, 128), (257, 1, 2, 1), (43, 2, 3, 6)]


def gru_inputs(shape, saturated):
    n, T, Fe, H = shape
    torch.manual_seed(sum(shape) + 1000 * saturated)
    gru = nn.GRU(Fe, H, batch_first=True)
    x, dout = torch.randn(n, T, Fe), torch.randn(n, T, H)
    if saturated:  # pre-activations around 20 from either side
        with torch.no_grad():
            gx = F.linear(x, gru.weight_ih_l0)
            gru.weight_ih_l0.mul_(20.0 / float(gx.std() if gx.numel() > 1 else gx.abs().max().clamp_min(1e-3)))
            gru.weight_hh_l0.normal_(0.0, 20.0 / H ** 0.5)
    return gru, x, dout


def torch_gru(gru, x, dout, dtype):
    net = copy.deepcopy(gru).to(dtype)
    xt = x.detach().clone().to(dtype).requires_grad_(True)
    y, _h = net(xt)
    (y * dout.to(dtype)).sum().backward()
    return [t.detach().numpy() for t in (y, xt.grad, net.weight_ih_l0.grad, net.weight_hh_l0.grad,
                                         net.bias_ih_l0.grad, net.bias_hh_l0.grad)]


@pytest.mark.parametrize("saturated", [False, True], ids=["random", "saturated"])
@pytest.mark.parametrize("shape", GRU_SHAPES, ids=lambda s: "n{}_T{}_F{}_H{}".format(*s))
def test_gru_forward_and_backward(shape, saturated):
    from onset_fingerprinting_amd import model
    n, T, Fe, H = shape
    gru, x, dout = gru_inputs(shape, saturated)
    r64, r32 = torch_gru(gru, x, dout, torch.float64), torch_gru(gru, x, dout, torch.float32)
    par = [dev(p.detach().numpy()) for p in (gru.weight_ih_l0, gru.weight_hh_l0, gru.bias_ih_l0, gru.bias_hh_l0)]
    (seq, bs), (gates, bg) = guarded(n, T, H), guarded(n, T, 4 * H)
    xd = dev(x.numpy())
    model.gru_train_forward(xd, *par, out=(seq, gates))
    torch.cuda.synchronize()
    ctx = f"gru n{n} T{T} F{Fe} H{H} {'saturated' if saturated else 'random'}"
    against_torch("out", seq, r64[0], r32[0], ctx, bs)
    guard_ok("gates", bg, ctx)
    if saturated:
        pre = np.abs(np.arctanh(np.clip(R.gru_forward_ref(x.numpy(), *(p.detach().numpy() for p in gru.parameters())
                                                          )[1][..., 2 * H:3 * H], -1 + 1e-16, 1 - 1e-16)))
        print(f"{ctx}: median |pre-activation of n| {float(np.median(pre)):.3g}")
    shapes = [(n, T, Fe), (3 * H, Fe), (3 * H, H), (3 * H,), (3 * H,)]
    outs = [guarded(*s) for s in shapes]
    model.gru_train_backward(xd, par[0], par[1], seq, gates, dev(dout.numpy()), out=tuple(o[0] for o in outs))
    torch.cuda.synchronize()
    for k, name in enumerate(("dx", "dw_ih", "dw_hh", "db_ih", "db_hh")):
        against_torch(name, outs[k][0], r64[k + 1], r32[k + 1], ctx, outs[k][1])


def test_gru_refusals():
    from onset_fingerprinting_amd import _lib
    L = _lib.lib()
    for args in ((0, 2, 3, 4), (1025, 2, 3, 4), (2, 0, 3, 4), (2, 129, 3, 4), (2, 2, 0, 4), (2, 2, 1025, 4), (2, 2, 3, 0),
                 (2, 2, 3, 129)):
        assert L.ofp_gru_train_forward_workspace_bytes(*args) == -1, args
        assert L.ofp_gru_train_backward_workspace_bytes(*args) == -1, args


# ---- attention and the mean over time -------------------------------------------------------------------------------
ATT_SHAPES = [(1, 1, 2, 2), (3, 2, 4, 2), (2, 16, 8, 2), (5, 17, 6, 2), (65, 3, 64, 2), (2, 128, 16, 2), (2, 16, 128, 2)]
ATT_CASES = [(s, "random") for s in ATT_SHAPES] + [((2, 16, 8, 2), "near_equal"), ((2, 16, 8, 2), "apart_80")]


def att_inputs(shape, kind):
    n, T, E, heads = shape
    torch.manual_seed(sum(shape) + len(kind))
    att = nn.MultiheadAttention(E, heads, batch_first=True)
    h, dctx = torch.randn(n, T, E), torch.randn(n, E)
    with torch.no_grad():
        att.in_proj_bias.normal_(0.0, 0.1)
        att.out_proj.weight.copy_(torch.eye(E))  # attention(h, h, h)[0].mean(1) is then the kernel's ctx
        att.out_proj.bias.zero_()
        if kind == "near_equal":
            h.mul_(1e-3)
            att.in_proj_bias.zero_()
        elif kind == "apart_80":  # logits are quadratic in h: scale it until they spread over about 80
            att.in_proj_bias.zero_()
            s = logits(att, h.double(), heads)
            h.mul_(float((80.0 / (s.max(-1)[0] - s.min(-1)[0]).max()) ** 0.5))
    return att, h, dctx


def logits(att, h, heads):
    n, T, E = h.shape
    d = E // heads
    qkv = F.linear(h, att.in_proj_weight.to(h.dtype), att.in_proj_bias.to(h.dtype))
    q, k = (qkv[..., i * E:(i + 1) * E].reshape(n, T, heads, d).permute(0, 2, 1, 3) for i in range(2))
    return q @ k.transpose(-1, -2) / d ** 0.5


def torch_attention(att, h, dctx, heads, dtype, mask=None):
    """(ctx, dh, d in_proj_weight, d in_proj_bias): without a mask by torch's own module, with one by the same formulas
    in torch operations (the module draws its own mask)."""
    net = copy.deepcopy(att).to(dtype).train()
    ht = h.detach().clone().to(dtype).requires_grad_(True)
    if mask is None:
        ctx = net(ht, ht, ht, need_weights=False)[0].mean(1)
    else:
        n, T, E = h.shape
        d = E // heads
        qkv = F.linear(ht, net.in_proj_weight, net.in_proj_bias)
        q, k, v = (qkv[..., i * E:(i + 1) * E].reshape(n, T, heads, d).permute(0, 2, 1, 3) for i in range(3))
        p = torch.softmax(q @ k.transpose(-1, -2) / d ** 0.5, -1) * torch.from_numpy(mask).to(dtype)
        ctx = (p @ v).permute(0, 2, 1, 3).reshape(n, T, E).mean(1)
    (ctx * dctx.to(dtype)).sum().backward()
    return [t.detach().numpy() for t in (ctx, ht.grad, net.in_proj_weight.grad, net.in_proj_bias.grad)]


def check_attention(shape, kind, p=0.0, seed=None, epoch=0):
    from onset_fingerprinting_amd import model
    n, T, E, heads = shape
    att, h, dctx = att_inputs(shape, kind)
    ctx_name = f"attention n{n} T{T} E{E} heads{heads} {kind} p{p}"
    mask = None
    if p:
        mask = R.attention_dropout_mask(seed, epoch, n, heads, T, p)
        (md, bm) = guarded(n, heads, T, T)
        model.attention_dropout_mask_device(seed, epoch, n, heads, T, p, out=md)
        torch.cuda.synchronize()
        guard_ok("mask", bm, ctx_name)
        assert np.array_equal(md.cpu().numpy().view(np.uint32), mask.view(np.uint32)), "site 3 mask differs from numpy"
    r64 = torch_attention(att, h, dctx, heads, torch.float64, mask)
    r32 = torch_attention(att, h, dctx, heads, torch.float32, mask)
    if mask is not None:  # the float64 reference of tests/cnnrnn_train_ref.py, run with that mask
        wn, bn = att.in_proj_weight.detach().numpy(), att.in_proj_bias.detach().numpy()
        c, qkv_r, pr = R.attention_mean_forward_ref(h.numpy(), wn, bn, heads, mask)
        r64 = [c] + list(R.attention_mean_backward_ref(h.numpy(), wn, heads, qkv_r, pr, dctx.numpy(), mask))
    spread = logits(att, h.double(), heads)
    print(f"{ctx_name}: logits spread up to {float((spread.max(-1)[0] - spread.min(-1)[0]).max()):.4g}")
    hd, wd, bd = dev(h.numpy()), dev(att.in_proj_weight.detach().numpy()), dev(att.in_proj_bias.detach().numpy())
    (ctx, bc), (qkv, bq), (probs, bp) = guarded(n, E), guarded(n, T, 3 * E), guarded(n, heads, T, T)
    model.attention_mean_train_forward(hd, wd, bd, heads, p, seed, epoch, out=(ctx, qkv, probs))
    torch.cuda.synchronize()
    against_torch("ctx", ctx, r64[0], r32[0], ctx_name, bc)
    guard_ok("qkv", bq, ctx_name), guard_ok("probs", bp, ctx_name)
    rows = probs.sum(-1).cpu().numpy()
    assert np.all(np.abs(rows - 1) <= 4 * T * U24), "a softmax row does not sum to 1"
    outs = [guarded(*s) for s in ((n, T, E), (3 * E, E), (3 * E,))]
    model.attention_mean_train_backward(hd, wd, heads, qkv, probs, dev(dctx.numpy()), p, seed, epoch,
                                        out=tuple(o[0] for o in outs))
    torch.cuda.synchronize()
    for k, name in enumerate(("dh", "dw", "db")):
        against_torch(name, outs[k][0], r64[k + 1], r32[k + 1], ctx_name, outs[k][1])


@pytest.mark.parametrize("case", ATT_CASES, ids=lambda c: "n{}_T{}_E{}_h{}_".format(*c[0]) + c[1])
def test_attention_forward_and_backward(case):
    check_attention(*case)


@pytest.mark.parametrize("shape", [(3, 2, 4, 2), (2, 16, 8, 2), (5, 17, 6, 2)], ids=lambda s: "n{}_T{}_E{}_h{}".format(*s))
def test_attention_with_dropout(shape):
    check_attention(shape, "random", 0.5, seed=0xC0FFEE, epoch=3)


def test_attention_refusals():
    from onset_fingerprinting_amd import _lib, model
    L = _lib.lib()
    for args in ((0, 2, 4, 2), (2, 0, 4, 2), (2, 129, 4, 2), (2, 2, 5, 2), (2, 2, 130, 2), (2, 2, 4, 0), (2, 2, 18, 9)):
        assert L.ofp_attention_mean_train_forward_workspace_bytes(*args) == -1, args
        assert L.ofp_attention_mean_train_backward_workspace_bytes(*args) == -1, args
    one = torch.ones(64, device="cuda")
    with pytest.raises(ValueError, match="seed="):
        model.attention_mean_train_forward(one[:16].view(2, 2, 4), one[:48].view(12, 4), one[:12], 2, p=0.5)


# ---- whole-network gradients ----------------------------------------------------------------------------------------
def load_case(g, case):
    from onset_fingerprinting_amd import model
    cfg = json.loads(str(g[f"{case}/cfg"]))
    kw = dict(cfg["kwargs"])
    kw["activation"], kw["loss"] = getattr(nn, kw["activation"]), getattr(F, kw["loss"])
    m = model.CNNRNN(cfg["width"], 2, channels=cfg["channels"], dropout_rate=0.0, lr=cfg["lr"], **kw)
    pre = f"{case}/sd0/"
    m.load_state_dict({k[len(pre):]: torch.from_numpy(g[k]) for k in g.files if k.startswith(pre)})
    x, y = torch.from_numpy(g[f"{case}/x"]), torch.from_numpy(g[f"{case}/y"])
    val = (torch.from_numpy(g[f"{case}/x_val"]), torch.from_numpy(g[f"{case}/y_val"])) if "n_val" in cfg else None
    return cfg, m, x, y, val


def torch_forward(net, x):
    """The reference's CNNRNN.forward over the module's own torch layers (dropout 0)."""
    h, _ = net.rnn(net.conv_layers(x))
    h, _ = net.attention(h, h, h, need_weights=False)
    return net.fc(h.mean(1))


def autograd_reference(model, x, y):
    out = {}
    for dtype in (torch.float32, torch.float64):
        net = copy.deepcopy(model).cpu().to(dtype).train()
        v = model.loss(torch_forward(net, x.to(dtype)), y.to(dtype))
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


@pytest.mark.parametrize("case", CASES)
def test_gradients_at_the_start(g, case):
    from onset_fingerprinting_amd import model
    cfg, m, x, y, _val = load_case(g, case)
    loss, grads = model.cnnrnn_loss_and_grads_device(m, x.cuda(), y.cuda())
    pre32, pre64 = f"{case}/g32/", f"{case}/g64/"
    g32 = {k[len(pre32):]: g[k] for k in g.files if k.startswith(pre32)}
    g64 = {k[len(pre64):]: g[k] for k in g.files if k.startswith(pre64)}
    check_grads(grads, loss, g32, g64, float(g[f"{case}/loss64"]), 2 * len(x), case)


@pytest.mark.parametrize("n", [65, 257, 1024])
def test_gradients_past_one_slab_and_one_chunk(g, n):
    """The first case widened: n * T = 6 n rows cross the Linear backward's slabs of 256 rows, n the head's chunks of
    64 samples and the GRU's 32 sequences per workgroup."""
    from onset_fingerprinting_amd import model
    _cfg, m, _x, _y, _val = load_case(g, CASES[0])
    torch.manual_seed(n)
    x, y = torch.randn(n, 3, 32), torch.randn(n, 2)
    loss, grads = model.cnnrnn_loss_and_grads_device(m, x.cuda(), y.cuda())
    ref = autograd_reference(m, x, y)
    check_grads(grads, loss, ref[torch.float32][0], ref[torch.float64][0], ref[torch.float64][1], 2 * n, f"n{n}")


def test_gradients_of_the_class_default():
    from onset_fingerprinting_amd import model
    torch.manual_seed(11)
    m = model.CNNRNN(256, 2, 3, dropout_rate=0.0)
    x, y = torch.randn(3, 3, 256), torch.randn(3, 2)
    loss, grads = model.cnnrnn_loss_and_grads_device(m, x.cuda(), y.cuda())
    ref = autograd_reference(m, x, y)
    check_grads(grads, loss, ref[torch.float32][0], ref[torch.float64][0], ref[torch.float64][1], 6, "default")


# ---- the epoch ------------------------------------------------------------------------------------------------------
def epoch_start():
    """BatchNorm, so that the validation forward differs from the training forward; 30 validation windows > 20."""
    from onset_fingerprinting_amd import model
    torch.manual_seed(20)
    m = model.CNNRNN(32, 2, channels=3, layer_sizes=[4, 6], n_hidden=8, dropout_rate=0.0, batch_norm=True, lr=0.01)
    return m, torch.randn(20, 3, 32), torch.randn(20, 2), torch.randn(30, 3, 32), torch.randn(30, 2)


def torch_epochs(start, x, y, xv, yv, epochs, dtype):
    net = copy.deepcopy(start).cpu().to(dtype).train()
    opt = torch.optim.NAdam(net.parameters(), lr=start.lr)
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, 100)
    tl, vl = [], []
    for _e in range(epochs):
        opt.zero_grad()
        loss = start.loss(torch_forward(net, x.to(dtype)), y.to(dtype))
        loss.backward()
        opt.step()
        sched.step()
        tl.append(float(loss.detach()))
        net.eval()
        with torch.no_grad():
            vl.append(float(F.l1_loss(torch_forward(net, xv.to(dtype)), yv.to(dtype))))
        net.train()
    return np.array(tl), np.array(vl)


def test_two_epochs_with_more_validation_than_training_windows():
    from onset_fingerprinting_amd import model
    start, x, y, xv, yv = epoch_start()
    m = copy.deepcopy(start).cuda()
    fit = model.fit_cnnrnn(m, x.cuda(), y.cuda(), x_val=xv.cuda(), y_val=yv.cuda(), max_epochs=2)
    assert fit.epochs == 2 and not m.training and int(m.conv_layers.bn1.num_batches_tracked) == 2
    t32, v32 = torch_epochs(start, x, y, xv, yv, 2, torch.float32)
    t64, v64 = torch_epochs(start, x, y, xv, yv, 2, torch.float64)
    for name, ours, r32, r64 in (("train", fit.train_loss, t32, t64), ("validation", fit.val_loss, v32, v64)):
        ours = ours.cpu().numpy()[:2].astype(f64)
        bound = np.maximum(4 * np.maximum.accumulate(np.abs(r32 - r64)), U22 * r64)
        print(f"{name} losses: ours {ours.tolist()} float64 {r64.tolist()}; |ours - ref64| {np.abs(ours - r64).tolist()} "
              f"bound {bound.tolist()}")
        assert np.all(np.abs(ours - r64) <= bound), name


def five_epochs():
    from onset_fingerprinting_amd import model
    start, x, y, xv, yv = epoch_start()
    m = copy.deepcopy(start).cuda()
    fit = model.fit_cnnrnn(m, x.cuda(), y.cuda(), x_val=xv.cuda(), y_val=yv.cuda(), max_epochs=5)
    flat = torch.cat([t.detach().reshape(-1).float() for t in m.state_dict().values()])
    return fit.train_loss.cpu().numpy(), fit.val_loss.cpu().numpy(), flat.cpu().numpy()


def test_two_fits_and_plain_launches_give_the_same_bits(tmp_path):
    """Five epochs twice as a replayed graph here, and once as plain launches (OFP_CNNRNN_GRAPH=nodes) in a fresh
    child process."""
    a, b = five_epochs(), five_epochs()
    assert np.isfinite(a[0]).all() and np.isfinite(a[1]).all()
    for u, v in zip(a, b):
        assert np.array_equal(u.view(np.uint32), v.view(np.uint32))
    out = tmp_path / "nodes.npz"
    code = ("import sys, numpy as np; sys.path[:0] = [sys.argv[1], sys.argv[2]]; import test_gpu_cnnrnn_train as t; "
            "tl, vl, flat = t.five_epochs(); np.savez(sys.argv[3], tl=tl, vl=vl, flat=flat)")
    env = dict(os.environ, OFP_CNNRNN_GRAPH="nodes")
    done = subprocess.run([sys.executable, "-c", code, str(REPO), str(REPO / "tests"), str(out)], env=env, timeout=300,
                          capture_output=True, text=True)
    assert done.returncode == 0, done.stderr[-2000:]
    c = np.load(out)
    for u, v in zip(a, (c["tl"], c["vl"], c["flat"])):
        assert np.array_equal(u.view(np.uint32), v.view(np.uint32)), "graph replay and plain launches differ"


# ---- training runs --------------------------------------------------------------------------------------------------
_runs = {}


def our_run(g, case):
    """fit_cnnrnn on the golden's inputs and start, on the GPU; once per case and session."""
    from onset_fingerprinting_amd import model
    if case not in _runs:
        cfg, m, x, y, val = load_case(g, case)
        m = m.cuda()
        kw = dict(x_val=val[0].cuda(), y_val=val[1].cuda(), patience=cfg["patience"]) if val else {}
        fit = model.fit_cnnrnn(m, x.cuda(), y.cuda(), max_epochs=cfg["epochs"], **kw)
        _runs[case] = (m, fit)
    return _runs[case]


def comparable_prefix(ref, pert):
    n = len(ref)
    with np.errstate(invalid="ignore"):
        spread = np.max(np.abs(pert[:, :n].astype(f64) - ref.astype(f64)), axis=0)
    bad = np.isnan(spread) | (spread > 1e-5 * ref)
    return (int(np.argmax(bad)) if bad.any() else n), spread


def check_curve(case, what, ours, ref, ref64, pert):
    prefix, spread = comparable_prefix(ref, pert)
    assert prefix >= 24
    own = np.maximum(spread[:prefix], np.abs(ref[:prefix].astype(f64) - ref64[:prefix]))
    bound = np.maximum(4 * np.maximum.accumulate(own), U22 * ref[:prefix])
    diff = np.abs(ours[:prefix].astype(f64) - ref[:prefix])
    worst = int(np.argmax(diff / bound))
    print(f"{case} {what}: prefix {prefix} of {len(ref)}; worst epoch {worst}: |ours - ref| {diff[worst]:.3e} bound "
          f"{bound[worst]:.3e} (spread {spread[worst]:.3e}, loss {ref[worst]:.6g}), error / bound "
          f"{diff[worst] / bound[worst]:.3g}; last epoch of the prefix: {diff[prefix - 1]:.3e} against "
          f"{bound[prefix - 1]:.3e}")
    assert np.all(diff <= bound), (case, what, worst, diff[worst], bound[worst])
    return prefix


@pytest.mark.parametrize("case", CASES + [STOP])
def test_trajectory_over_the_comparable_prefix(g, case):
    _m, fit = our_run(g, case)
    ours = fit.train_loss.cpu().numpy()
    ref = g[f"{case}/errors"]
    assert fit.epochs >= min(24, len(ref)) and np.isfinite(ours[:fit.epochs]).all()
    prefix = check_curve(case, "train", ours, ref, g[f"{case}/errors64"], g[f"{case}/pert_errors"])
    assert fit.epochs >= prefix


@pytest.mark.parametrize("case", [c for c in CASES if c.startswith("l1")])
def test_outcome_of_the_l1_cases(g, case):
    ref, pert = g[f"{case}/errors"], g[f"{case}/pert_errors"]
    curves = [ref] + [pert[k] for k in range(len(pert))]
    finals = np.array([c[-1] for c in curves], f64)
    bests = np.array([c.min() for c in curves], f64)
    _m, fit = our_run(g, case)
    ours = fit.train_loss.cpu().numpy()[:fit.epochs]
    msg = (f"{case}: reference finals {finals.min():.6g} .. {finals.max():.6g} bests {bests.min():.6g} .. "
           f"{bests.max():.6g}; ours final {ours[-1]:.8g} best {ours.min():.8g} epochs {fit.epochs}")
    print(msg)
    assert fit.epochs == len(ref), msg
    assert ours[-1] <= finals.max() + (finals.max() - finals.min()), msg
    assert ours.min() <= bests.max() + (bests.max() - bests.min()), msg


def test_early_stop(g):
    cfg, _start, _x, _y, _val = load_case(g, STOP)
    stop = int(g[f"{STOP}/stop"])
    m, fit = our_run(g, STOP)
    tl, vl = fit.train_loss.cpu().numpy(), fit.val_loss.cpu().numpy()
    print(f"{STOP}: reference stops after {stop} epochs, ours after {fit.epochs}")
    assert stop == 29 and fit.epochs == stop
    assert tl.shape == vl.shape == (cfg["epochs"],) and len(fit.lrs) == stop and not m.training
    assert np.isfinite(tl[:stop]).all() and np.isfinite(vl[:stop]).all()
    assert np.isnan(tl[stop:]).all() and np.isnan(vl[stop:]).all()
    check_curve(STOP, "validation", vl, g[f"{STOP}/val"], g[f"{STOP}/val64"], g[f"{STOP}/pert_val"])


def test_inference_forward_of_the_trained_module(g):
    """The trainer's last validation loss against the inference kernels' forward of the trained module."""
    _cfg, _s, _x, _y, val = load_case(g, STOP)
    m, fit = our_run(g, STOP)
    with torch.no_grad():
        again = float(F.l1_loss(m(val[0].cuda()), val[1].cuda()))
    last = float(fit.val_loss[fit.epochs - 1])
    rel = abs(again - last) / abs(again)
    print(f"last validation loss {last:.9g}, forward of the trained module {again:.9g}, rel {rel:.3e}, bound "
          f"{2.0 ** -20:.3e}")
    assert rel <= 2.0 ** -20


# ---- dropout and the window source ----------------------------------------------------------------------------------
def dropout_fit(g, epochs, seed):
    from onset_fingerprinting_amd import model
    _cfg, m, x, y, _val = load_case(g, CASES[0])
    m.dropout.p = m.attention.dropout = 0.5
    m = m.cuda()
    fit = model.fit_cnnrnn(m, x.cuda(), y.cuda(), max_epochs=epochs, seed=seed)
    assert fit.epochs == epochs
    return m, fit, x.cuda(), y.cuda()


def test_dropout_fit(g):
    from onset_fingerprinting_amd import model
    m20, fit, x, y = dropout_fit(g, 20, 1)
    curve = fit.train_loss[:20]
    assert bool(torch.isfinite(curve).all())
    _cfg, start, _x, _y, _v = load_case(g, CASES[0])
    start.dropout.p = start.attention.dropout = 0.5
    m7, _f7, _x, _y = dropout_fit(g, 7, 1)
    for e, net in ((0, start.cuda()), (7, m7)):
        loss, _g = model.cnnrnn_loss_and_grads_device(net, x, y, seed=1, epoch=e)
        print(f"epoch {e}: the fit's loss {float(curve[e]):.9g}, loss and gradients on that epoch's parameters "
              f"{float(loss):.9g}")
        assert float(loss) == float(curve[e])
    plain, _g = model.cnnrnn_loss_and_grads_device(load_case(g, CASES[0])[1].cuda(), x, y)
    assert float(plain) != float(curve[0]), "the dropout changed nothing"
    _m, again, _x, _y = dropout_fit(g, 20, 1)
    assert torch.equal(again.train_loss.view(torch.int32), fit.train_loss.view(torch.int32))
    _m, other, _x, _y = dropout_fit(g, 20, 2)
    assert not torch.equal(other.train_loss.view(torch.int32), fit.train_loss.view(torch.int32))
    # site 0 is fit_cnn's mask over the conv features [n, C * W]
    mask = model.dropout_mask_device(1, 0, 24, 6 * 32, 0.5).cpu().numpy()
    assert np.array_equal(mask, RR.dropout_mask(1, 0, 24, 6 * 32, 0.5))


def test_window_source(g):
    from onset_fingerprinting_amd import data, model
    audio, onsets, y = RR.synthetic_hits(8, 10, 3, 32, 3)
    src = data.ShiftedWindows(audio, onsets, 32, pre_samples=2, max_shift=3, n_extractions=2)
    _cfg, m, _x, _y, _v = load_case(g, CASES[0])
    m = m.cuda()
    yt = torch.from_numpy(y)
    first, _g = model.cnnrnn_loss_and_grads_device(copy.deepcopy(m), src.windows(4, 0), yt.repeat(2, 1).cuda())
    fit = model.fit_cnnrnn(m, src, yt, max_epochs=5, seed=4)
    print(f"window source: first loss {float(fit.train_loss[0]):.9g}, on the windows of epoch 0 {float(first):.9g}")
    assert fit.epochs == 5 and bool(torch.isfinite(fit.train_loss[:5]).all())
    assert float(fit.train_loss[0]) == float(first)
