"""GPU: training model.RNN (csrc/ofp_rnn_train.hip, model.fit_rnn) against float64 references, torch, and the
reference's recorded runs (tests/golden/g29_rnn_train.npz, made by make_golden_rnn_train.py).  The rules and helpers
are those of tests/test_gpu_cnnrnn_train.py:

  layernorm   forward and backward against torch's float64 native_layer_norm; per tensor max |ours - ref64| <= 4 x max
              |torch float32 - ref64|, floored at 2^-22 x max |ref64|
  gru stack   the same rule against torch's float64 nn.GRU(num_layers=L); with dropout the site-4 mask bit for bit
              against numpy and the values against torch float64 with the layers run one by one under that mask (the
              float32 yardstick: the same in torch float32)
  attention   the CNNRNN test's checks at the RNN trainer's capacity, T up to 512
  nadam       the rule of test_gpu_cnn_train.py::test_nadam_step against torch's step with weight decay in float64
  gradients   per tensor, max |ours - g64| <= 4 x max |g32 - g64|, floored at 2^-23 x max |g64|
  epoch       first losses against torch float64, graph replay against plain launches and two fits, bit for bit
  trajectory, outcome, stop, dropout, window source: the rules of tests/test_gpu_cnn_train.py
Every figure is printed before it is asserted (run with -s to see them).  Outputs of the directly called kernels go
into NaN-filled buffers with a guard tail.

Switches of the kernels and the shapes on both sides of each:
  k_ln_fwd / _bwd_dx      four rows per workgroup, one wave each (rows 1, 3, 4, 5); lanes take columns e and e + 64
                          (E = 1, 2, 63, 64, 65, 128)
  k_ln_bwd_partial        slabs of 256 rows (rows 257); the even and the odd rows on two lanes (rows 1: no odd row)
  k_inproj_fwd / _wgrad   F = 1 .. 8; 16 outputs per workgroup (3H = 3, 6, 12, 24, 192, 384); slabs of 2048 rows
                          (n T = 1 .. 2 x 1024 + 8 = 2056 at n 8, T 257: past one slab), both strides of x
  k_gru_fwd / _bwd        no T limit of their own: T = 129, 256, 257, 512; layers 1 to 4 chained
  k_attn_fwd / _bwd<512>  rows and columns go round the 256 threads once (T <= 256) or twice (257, 512)
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
import cnn_train_ref as CR  # noqa: E402
import cnnrnn_train_ref as AR  # noqa: E402
import rnn_train_ref as R  # noqa: E402
import test_gpu_cnnrnn_train as C  # noqa: E402  (helpers only; its tests are collected from its own file)
import test_rnn_train_cpu as TC  # noqa: E402
import train_random_ref as RR  # noqa: E402
from test_gpu_cnnrnn_train import against_torch, check_grads, dev, guard_ok, guarded, within  # noqa: E402

pytestmark = pytest.mark.gpu

REPO = Path(__file__).resolve().parents[1]
CASES = ["l1_two_layers", "mse_one_layer", "l1_three_layers"]
STOP = "l1_stop"
U24, U23, U22 = 2.0 ** -24, 2.0 ** -23, 2.0 ** -22
f32, f64 = np.float32, np.float64
KEYS = ("weight_ih", "weight_hh", "bias_ih", "bias_hh")


@pytest.fixture(scope="module")
def g(golden):
    return golden("g29_rnn_train")


# ---- LayerNorm ------------------------------------------------------------------------------------------------------
LN_ROWS, LN_E = (1, 3, 4, 5, 257), (1, 2, 63, 64, 65, 128)


def torch_layernorm(x, ga, be, dy, eps, dtype):
    xt = torch.from_numpy(x).to(dtype).requires_grad_(True)
    gt, bt = (torch.from_numpy(a).to(dtype).requires_grad_(True) for a in (ga, be))
    y, mean, rstd = torch.native_layer_norm(xt, (x.shape[1],), gt, bt, eps)
    (y * torch.from_numpy(dy).to(dtype)).sum().backward()
    return [t.detach().numpy() for t in (y, mean.reshape(-1), rstd.reshape(-1), xt.grad, gt.grad, bt.grad)]


@pytest.mark.parametrize("E", LN_E)
@pytest.mark.parametrize("rows", LN_ROWS)
def test_layernorm_forward_and_backward(rows, E):
    from onset_fingerprinting_amd import model
    rng = np.random.default_rng([rows, E])
    x = (rng.standard_normal((rows, E)) * 1.5 + 0.3).astype(f32)
    ga, be = rng.uniform(0.5, 1.5, E).astype(f32), rng.standard_normal(E).astype(f32)
    dy = rng.standard_normal((rows, E)).astype(f32)
    eps = 1e-5
    r64, r32 = (torch_layernorm(x, ga, be, dy, eps, t) for t in (torch.float64, torch.float32))
    ctx = f"layernorm rows{rows} E{E}"
    xd, gd = dev(x), dev(ga)
    (y, by), (mean, bm), (rstd, br) = guarded(rows, E), guarded(rows), guarded(rows)
    model.layernorm_train_forward(xd, gd, dev(be), eps, out=(y, mean, rstd))
    torch.cuda.synchronize()
    against_torch("y", y, r64[0], r32[0], ctx, by)
    against_torch("mean", mean, r64[1], r32[1], ctx, bm)
    against_torch("rstd", rstd, r64[2], r32[2], ctx, br)
    (dx, bx), (dga, bg), (dbe, bb) = guarded(rows, E), guarded(E), guarded(E)
    model.layernorm_train_backward(xd, gd, mean, rstd, dev(dy), out=(dx, dga, dbe))
    torch.cuda.synchronize()
    against_torch("dx", dx, r64[3], r32[3], ctx, bx)
    against_torch("dgamma", dga, r64[4], r32[4], ctx, bg)
    against_torch("dbeta", dbe, r64[5], r32[5], ctx, bb)


def test_layernorm_of_rows_constant_to_one_ulp():
    """Every row is a constant and the same constant one ulp up, mixed: the variance (about 1e-15) is far below eps, so
    rstd is 1 / sqrt(eps) to 1e-10 and y - beta is (x - mean) x 316 x gamma, a few 1e-5.  The forward is measured
    against float64 from x alone.  The backward takes mean and rstd as inputs, and a float32 mean cannot tell the row's
    values from their mean: its reference is the float64 formulas on the statistics the forward returned, its
    float32 yardstick the same formulas in float32."""
    from onset_fingerprinting_amd import model
    rows, E, eps = 5, 65, 1e-5
    rng = np.random.default_rng(77)
    base = rng.uniform(0.5, 2.0, (rows, 1)).astype(f32)
    x = np.where(rng.integers(0, 2, (rows, E)) == 1, np.nextafter(base, f32(4)), base).astype(f32)
    ga, be = rng.uniform(0.5, 1.5, E).astype(f32), rng.standard_normal(E).astype(f32)
    dy = rng.standard_normal((rows, E)).astype(f32)
    y64, mean64, rstd64 = R.layernorm_forward_ref(x, ga, be, eps)
    r32 = torch_layernorm(x, ga, be, dy, eps, torch.float32)
    var = ((x.astype(f64) - mean64[:, None]) ** 2).mean(1)
    print(f"variance up to {var.max():.3e} against eps {eps}; |y - beta| up to {np.abs(y64 - be).max():.3e}")
    assert var.max() < 1e-8 * eps
    ctx = "layernorm near-constant rows"
    xd, gd = dev(x), dev(ga)
    (y, by), (mean, bm), (rstd, br) = guarded(rows, E), guarded(rows), guarded(rows)
    model.layernorm_train_forward(xd, gd, dev(be), eps, out=(y, mean, rstd))
    torch.cuda.synchronize()
    against_torch("y", y, y64, r32[0], ctx, by)
    against_torch("y - beta", y.cpu() - torch.from_numpy(be), y64 - be, r32[0] - be, ctx)
    against_torch("mean", mean, mean64, r32[1], ctx, bm)
    against_torch("rstd", rstd, rstd64, r32[2], ctx, br)
    mean_f, rstd_f = mean.cpu().numpy(), rstd.cpu().numpy()
    want = R.layernorm_backward_ref(x, ga, mean_f, rstd_f, dy)
    xh = (x - mean_f[:, None]) * rstd_f[:, None]
    gg = dy * ga
    same32 = (rstd_f[:, None] * (gg - gg.mean(1, keepdims=True, dtype=f32) - xh * (gg * xh).mean(1, keepdims=True, dtype=f32)),
              (dy * xh).sum(0, dtype=f32), dy.sum(0, dtype=f32))
    (dx, bx), (dga, bg), (dbe, bb) = guarded(rows, E), guarded(E), guarded(E)
    model.layernorm_train_backward(xd, gd, mean, rstd, dev(dy), out=(dx, dga, dbe))
    torch.cuda.synchronize()
    for name, got, buf, ref, t32 in (("dx", dx, bx, want[0], same32[0]), ("dgamma", dga, bg, want[1], same32[1]),
                                     ("dbeta", dbe, bb, want[2], same32[2])):
        against_torch(name, got, ref, t32, ctx, buf)


def test_layernorm_refusals():
    from onset_fingerprinting_amd import _lib, model
    L = _lib.lib()
    for args in ((0, 4), (3, 0), (3, 129), ((1 << 20) + 1, 4)):
        assert L.ofp_layernorm_train_backward_workspace_bytes(*args) == -1, args
    one = torch.ones(3 * 129, device="cuda")
    with pytest.raises(ValueError, match="limits"):
        model.layernorm_train_forward(one.view(3, 129), one[:129], one[:129])
    with pytest.raises(ValueError, match="limits"):
        model.layernorm_train_backward(one.view(3, 129), one[:129], one[:3], one[:3], one.view(3, 129))
    st = L.ofp_layernorm_train_forward(one.data_ptr(), 3, 129, one.data_ptr(), one.data_ptr(), 1e-5, one.data_ptr(),
                                       one.data_ptr(), one.data_ptr(), None)
    assert st != 0 and "width 1..128" in _lib.last_error()


# ---- the GRU stack --------------------------------------------------------------------------------------------------
STACK_SHAPES = [(1, 1, 1, 1, 1), (3, 2, 3, 2, 2), (2, 129, 3, 4, 2), (2, 256, 3, 8, 2), (2, 257, 4, 4, 3),
                (1, 512, 8, 2, 4), (65, 3, 3, 64, 2), (3, 4, 8, 128, 2)]
shape_id = lambda s: "n{}_T{}_F{}_H{}_L{}".format(*s)  # noqa: E731


def stack_inputs(shape, saturated):
    """The stack's form of gru_inputs: random, or with pre-activations around 20 from either side in every layer."""
    n, T, Fe, H, L = shape
    torch.manual_seed(sum(shape) + 1000 * saturated)
    gru = nn.GRU(Fe, H, L, batch_first=True)
    x, dout = torch.randn(n, T, Fe), torch.randn(n, T, H)
    if saturated:
        with torch.no_grad():
            gx = F.linear(x, gru.weight_ih_l0)
            gru.weight_ih_l0.mul_(20.0 / float(gx.std() if gx.numel() > 1 else gx.abs().max().clamp_min(1e-3)))
            for l in range(L):
                getattr(gru, f"weight_hh_l{l}").normal_(0.0, 20.0 / H ** 0.5)
                if l:
                    getattr(gru, f"weight_ih_l{l}").normal_(0.0, 20.0 / H ** 0.5)
    return gru, x, dout


def torch_stack(gru, x, dout, dtype, masks=None):
    """(out, [(dw_ih, dw_hh, db_ih, db_hh)] per layer): torch's own nn.GRU(num_layers=L) without masks, its layers
    run one by one under them."""
    if masks is not None:
        return TC.torch_stack(gru, x, dout, masks, dtype)
    net = copy.deepcopy(gru).to(dtype)
    y, _h = net(x.detach().clone().to(dtype))
    (y * dout.to(dtype)).sum().backward()
    return y.detach().numpy(), [tuple(getattr(net, f"{k}_l{l}").grad.numpy() for k in KEYS)
                                for l in range(gru.num_layers)]


def check_stack(shape, saturated, permuted=False, p=0.0, seed=None, epoch=0):
    from onset_fingerprinting_amd import model
    n, T, Fe, H, L = shape
    gru, x, dout = stack_inputs(shape, saturated)
    ctx = f"stack {shape_id(shape)} {'saturated' if saturated else 'random'}{' permuted' if permuted else ''} p{p}"
    masks = None
    if p:
        masks = R.layer_dropout_mask(seed, epoch, L - 1, n, T, H, p)
        md, bm = guarded(L - 1, n, T, H)
        model.rnn_layer_dropout_mask_device(seed, epoch, L - 1, n, T, H, p, out=md)
        torch.cuda.synchronize()
        guard_ok("mask", bm, ctx)
        assert np.array_equal(md.cpu().numpy().view(np.uint32), masks.view(np.uint32)), "site 4 mask differs from numpy"
    (o64, g64), (o32, g32) = (torch_stack(gru, x, dout, t, masks) for t in (torch.float64, torch.float32))
    params = [tuple(dev(getattr(gru, f"{k}_l{l}").detach().numpy()) for k in KEYS) for l in range(L)]
    xd = dev(x.permute(0, 2, 1).contiguous().numpy() if permuted else x.numpy())
    (seqs, bs), (gates, bg) = guarded(L, n, T, H), guarded(L, n, T, 4 * H)
    model.rnn_gru_train_forward(xd, params, p, seed, epoch, permuted=permuted, out=(seqs, gates))
    torch.cuda.synchronize()
    guard_ok("seqs", bs, ctx), guard_ok("gates", bg, ctx)
    against_torch("out", seqs[L - 1], o64, o32, ctx)
    count = sum(t.numel() for layer in params for t in layer)
    flat, bf = guarded(count)
    grads = model.rnn_gru_train_backward(xd, params, seqs, gates, dev(dout.numpy()), p, seed, epoch, permuted=permuted,
                                         out=flat)
    torch.cuda.synchronize()
    guard_ok("gradients", bf, ctx)
    for l in range(L):
        for k, name in enumerate(("dw_ih", "dw_hh", "db_ih", "db_hh")):
            against_torch(f"layer {l} {name}", grads[l][k], g64[l][k], g32[l][k], ctx)


@pytest.mark.parametrize("saturated", [False, True], ids=["random", "saturated"])
@pytest.mark.parametrize("shape", STACK_SHAPES, ids=shape_id)
def test_gru_stack_forward_and_backward(shape, saturated):
    check_stack(shape, saturated)


def test_gru_stack_on_the_window_as_it_is_stored():
    """permute_input=True: x is [n, F, T] and is read with strides; the same values as from [n, T, F]."""
    check_stack((2, 129, 3, 4, 2), False, permuted=True)
    check_stack((8, 257, 4, 4, 1), False, permuted=True)  # 2056 rows: past one slab of the input projection's gradient
    check_stack((8, 257, 4, 4, 1), False, permuted=False)


@pytest.mark.parametrize("shape", [(3, 2, 3, 2, 2), (2, 129, 3, 4, 2), (2, 257, 4, 4, 3)], ids=shape_id)
def test_gru_stack_with_dropout(shape):
    check_stack(shape, False, p=0.5, seed=0xC0FFEE, epoch=3)


def test_gru_stack_refusals():
    from onset_fingerprinting_amd import _lib, model
    L = _lib.lib()
    for args in ((0, 2, 3, 4, 2), (1025, 2, 3, 4, 2), (2, 0, 3, 4, 2), (2, 513, 3, 4, 2), (2, 2, 0, 4, 2), (2, 2, 9, 4, 2),
                 (2, 2, 3, 0, 2), (2, 2, 3, 129, 2), (2, 2, 3, 4, 0), (2, 2, 3, 4, 5)):
        assert L.ofp_rnn_gru_train_forward_workspace_bytes(*args) == -1, args
        assert L.ofp_rnn_gru_train_backward_workspace_bytes(*args) == -1, args
    for args in ((2, 512, 8, 128, 4), (1024, 1, 1, 1, 1)):
        assert L.ofp_rnn_gru_train_forward_workspace_bytes(*args) > 0, args
    one = torch.ones(4096, device="cuda")
    par = [(one[:36].view(12, 3), one[:48].view(12, 4), one[:12], one[:12])]
    with pytest.raises(ValueError, match="time steps"):
        model.rnn_gru_train_forward(one[:2 * 513 * 3].view(2, 513, 3).contiguous(), par)
    with pytest.raises(ValueError, match="seed="):
        model.rnn_gru_train_forward(one[:12].view(2, 2, 3), par, p=0.5)


# ---- attention at the trainer's capacity ----------------------------------------------------------------------------
ATT_CASES = [((2, 129, 8, 2), "random"), ((2, 256, 8, 2), "random"), ((2, 257, 8, 2), "random"),
             ((2, 512, 8, 2), "random"), ((2, 16, 128, 8), "random"), ((2, 256, 8, 2), "near_equal"),
             ((2, 256, 8, 2), "apart_80")]


def check_attention(shape, kind, p=0.0, seed=None, epoch=0):
    """test_gpu_cnnrnn_train.py's check_attention on the rnn_ entries."""
    from onset_fingerprinting_amd import model
    n, T, E, heads = shape
    att, h, dctx = C.att_inputs(shape, kind)
    ctx_name = f"rnn attention n{n} T{T} E{E} heads{heads} {kind} p{p}"
    mask = None
    if p:
        mask = AR.attention_dropout_mask(seed, epoch, n, heads, T, p)
        (md, bm) = guarded(n, heads, T, T)
        model.attention_dropout_mask_device(seed, epoch, n, heads, T, p, out=md)
        torch.cuda.synchronize()
        guard_ok("mask", bm, ctx_name)
        assert np.array_equal(md.cpu().numpy().view(np.uint32), mask.view(np.uint32)), "site 3 mask differs from numpy"
    r64 = C.torch_attention(att, h, dctx, heads, torch.float64, mask)
    r32 = C.torch_attention(att, h, dctx, heads, torch.float32, mask)
    if mask is not None:
        wn, bn = att.in_proj_weight.detach().numpy(), att.in_proj_bias.detach().numpy()
        c, qkv_r, pr = AR.attention_mean_forward_ref(h.numpy(), wn, bn, heads, mask)
        r64 = [c] + list(AR.attention_mean_backward_ref(h.numpy(), wn, heads, qkv_r, pr, dctx.numpy(), mask))
    spread = C.logits(att, h.double(), heads)
    print(f"{ctx_name}: logits spread up to {float((spread.max(-1)[0] - spread.min(-1)[0]).max()):.4g}")
    hd, wd, bd = dev(h.numpy()), dev(att.in_proj_weight.detach().numpy()), dev(att.in_proj_bias.detach().numpy())
    (ctx, bc), (qkv, bq), (probs, bp) = guarded(n, E), guarded(n, T, 3 * E), guarded(n, heads, T, T)
    model.rnn_attention_train_forward(hd, wd, bd, heads, p, seed, epoch, out=(ctx, qkv, probs))
    torch.cuda.synchronize()
    against_torch("ctx", ctx, r64[0], r32[0], ctx_name, bc)
    guard_ok("qkv", bq, ctx_name), guard_ok("probs", bp, ctx_name)
    rows = probs.sum(-1).cpu().numpy()
    assert np.all(np.abs(rows - 1) <= 4 * T * U24), "a softmax row does not sum to 1"
    outs = [guarded(*s) for s in ((n, T, E), (3 * E, E), (3 * E,))]
    model.rnn_attention_train_backward(hd, wd, heads, qkv, probs, dev(dctx.numpy()), p, seed, epoch,
                                       out=tuple(o[0] for o in outs))
    torch.cuda.synchronize()
    for k, name in enumerate(("dh", "dw", "db")):
        against_torch(name, outs[k][0], r64[k + 1], r32[k + 1], ctx_name, outs[k][1])


@pytest.mark.parametrize("case", ATT_CASES, ids=lambda c: "n{}_T{}_E{}_h{}_".format(*c[0]) + c[1])
def test_attention_forward_and_backward(case):
    check_attention(*case)


def test_attention_with_dropout():
    check_attention((2, 129, 8, 2), "random", 0.5, seed=0xC0FFEE, epoch=3)


@pytest.mark.parametrize("shape", [(2, 16, 8, 2), (5, 17, 6, 2), (2, 128, 16, 2)], ids=lambda s: "n{}_T{}_E{}_h{}".format(*s))
def test_attention_of_both_capacities_gives_the_same_bits(shape):
    """The 512-step instantiation stores its probabilities across the threads, the 128-step one along each thread's
    row; both evaluate the same expressions, so where both take the shape every output agrees bit for bit."""
    from onset_fingerprinting_amd import model
    n, T, E, heads = shape
    att, h, dctx = C.att_inputs(shape, "random")
    hd, wd, bd = dev(h.numpy()), dev(att.in_proj_weight.detach().numpy()), dev(att.in_proj_bias.detach().numpy())
    for p, seed in ((0.0, None), (0.5, 9)):
        short = model.attention_mean_train_forward(hd, wd, bd, heads, p, seed, 1)
        long_ = model.rnn_attention_train_forward(hd, wd, bd, heads, p, seed, 1)
        back_s = model.attention_mean_train_backward(hd, wd, heads, short[1], short[2], dev(dctx.numpy()), p, seed, 1)
        back_l = model.rnn_attention_train_backward(hd, wd, heads, long_[1], long_[2], dev(dctx.numpy()), p, seed, 1)
        torch.cuda.synchronize()
        for a, b in zip(short + back_s, long_ + back_l):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_attention_refusal_past_512_steps():
    from onset_fingerprinting_amd import _lib
    L = _lib.lib()
    assert L.ofp_rnn_attention_train_forward_workspace_bytes(2, 513, 4, 2) == -1
    assert L.ofp_rnn_attention_train_backward_workspace_bytes(2, 513, 4, 2) == -1
    assert L.ofp_rnn_attention_train_forward_workspace_bytes(2, 512, 4, 2) > 0
    assert L.ofp_rnn_attention_train_backward_workspace_bytes(2, 512, 4, 2) > 0


# ---- NAdam with weight decay ----------------------------------------------------------------------------------------
def nadam_inputs(step):
    from onset_fingerprinting_amd import model
    fac = model.cnn_step_factors(model.cnn_rate_table(0.01, 300))[step]
    rng = np.random.default_rng(step)
    n = 1000
    gr = rng.standard_normal(n).astype(f32)
    p = (1e3 * np.abs(gr) * rng.choice([-1.0, 1.0], n) * rng.uniform(0.5, 2.0, n)).astype(f32)  # |p| about 1e3 |g|
    m = (gr * rng.uniform(0.1, 1.0, n)).astype(f32)
    v = (gr.astype(f64) ** 2 * rng.uniform(0.1, 1.0, n)).astype(f32)
    row = np.zeros(4, f32)
    row[:3] = fac
    return p, gr, m, v, row


@pytest.mark.parametrize("step", [0, 7, 251])
def test_nadam_step_with_weight_decay(step):
    from onset_fingerprinting_amd import model
    wd = 1e-4
    p, gr, m, v, row = nadam_inputs(step)
    p1, m1, v1, upd, gd = R.nadam_decay_step_ref(p, gr, m, v, row[:3].astype(f64), float(f32(wd)))
    (pd, bp), (md, bm), (vd, bv) = guarded(len(p)), guarded(len(p)), guarded(len(p))
    pd.copy_(dev(p)), md.copy_(dev(m)), vd.copy_(dev(v))
    model.nadam_step(pd, dev(gr), md, vd, dev(row), weight_decay=wd)
    torch.cuda.synchronize()
    ctx = f"nadam with decay, step {step}"
    bounds = (8 * U24 * np.abs(upd) + U24 * np.abs(p1), 3 * U24 * (np.abs(m) + np.abs(gd)), 4 * U24 * np.abs(v1))
    within("p", pd, p1, bounds[0], ctx, bp)
    within("exp_avg", md, m1, bounds[1], ctx, bm)
    within("exp_avg_sq", vd, v1, bounds[2], ctx, bv)
    # the same bounds refuse a step without the decay term: `within` fails on one element outside, and each of the
    # three tensors has such elements (in exp_avg and exp_avg_sq every one; in p fewer at the first steps, where the
    # update is close to lr x sign(g) and the bound carries u |p| with |p| = 1e3 |g|)
    q1, n1, w1, _u = CR.nadam_step_ref(p, gr, m, v, row[:3].astype(f64))
    out = [float(np.mean(np.abs(a - b) > bd)) for a, b, bd in ((q1, p1, bounds[0]), (n1, m1, bounds[1]),
                                                                 (w1, v1, bounds[2]))]
    print(f"{ctx}: share of elements a step without decay puts outside the bound: p {out[0]:.3f} exp_avg {out[1]:.3f} "
          f"exp_avg_sq {out[2]:.3f}")
    assert min(out) > 0 and out[1] > 0.9 and out[2] > 0.9


def test_nadam_step_without_the_keyword_runs_what_it_ran():
    """model.nadam_step(p, g, m, v, row) against a direct call of ofp_nadam_step on the same inputs, bit for bit."""
    from onset_fingerprinting_amd import _lib, model
    p, gr, m, v, row = nadam_inputs(7)
    a, b = [dev(t) for t in (p, m, v)], [dev(t) for t in (p, m, v)]
    gd, rd = dev(gr), dev(row)
    model.nadam_step(a[0], gd, a[1], a[2], rd)
    _lib.check(_lib.lib().ofp_nadam_step(b[0].data_ptr(), gd.data_ptr(), b[1].data_ptr(), b[2].data_ptr(), len(p),
                                         rd.data_ptr(), None))
    torch.cuda.synchronize()
    for u, w in zip(a, b):
        assert torch.equal(u.view(torch.int32), w.view(torch.int32))
    assert not torch.equal(a[0], dev(p))
    c = [dev(t) for t in (p, m, v)]
    model.nadam_step(c[0], gd, c[1], c[2], rd, weight_decay=1e-4)
    assert not torch.equal(c[0], a[0])


# ---- whole-network gradients ----------------------------------------------------------------------------------------
def load_case(g, case):
    from onset_fingerprinting_amd import model
    cfg = json.loads(str(g[f"{case}/cfg"]))
    kw = dict(cfg["kwargs"])
    kw["loss"] = getattr(F, kw["loss"])
    m = model.RNN(cfg["width"], 2, channels=cfg["channels"], dropout_rate=0.0, lr=cfg["lr"], **kw)
    pre = f"{case}/sd0/"
    m.load_state_dict({k[len(pre):]: torch.from_numpy(g[k]) for k in g.files if k.startswith(pre)})
    x, y = torch.from_numpy(g[f"{case}/x"]), torch.from_numpy(g[f"{case}/y"])
    val = (torch.from_numpy(g[f"{case}/x_val"]), torch.from_numpy(g[f"{case}/y_val"])) if "n_val" in cfg else None
    return cfg, m, x, y, val


def torch_forward(net, x, lmask=None, amask=None):
    """The reference's RNN.forward over the module's own torch layers; with masks (dropout) the recurrent layers one by
    one under lmask [L - 1, n, T, H] and the attention's formulas under amask [n, heads, T, T]."""
    h = x.permute(0, 2, 1) if net.permute_input else x
    if lmask is None and amask is None:
        h, _ = net.rnn(h)
        h = net.layer_norm(h)
        h, _ = net.attention(h, h, h, need_weights=False)
        return net.fc(h.mean(1))
    rnn, att = net.rnn, net.attention
    for l in range(rnn.num_layers):
        one = nn.GRU(h.shape[2], rnn.hidden_size, batch_first=True)
        for k in KEYS:  # the stack's own parameters, so that their gradients land in `net`
            setattr(one, k + "_l0", getattr(rnn, f"{k}_l{l}"))
        h, _ = one(h)
        if l < rnn.num_layers - 1:
            h = h * torch.from_numpy(lmask[l]).to(h.dtype)
    h = net.layer_norm(h)
    n, T, E = h.shape
    d = E // att.num_heads
    qkv = F.linear(h, att.in_proj_weight, att.in_proj_bias)
    q, k, v = (qkv[..., i * E:(i + 1) * E].reshape(n, T, att.num_heads, d).permute(0, 2, 1, 3) for i in range(3))
    pr = torch.softmax(q @ k.transpose(-1, -2) / d ** 0.5, -1) * torch.from_numpy(amask).to(h.dtype)
    o = att.out_proj((pr @ v).permute(0, 2, 1, 3).reshape(n, T, E))
    return net.fc(o.mean(1))


def autograd_reference(model, x, y, lmask=None, amask=None):
    out = {}
    for dtype in (torch.float32, torch.float64):
        net = copy.deepcopy(model).cpu().to(dtype).train()
        v = model.loss(torch_forward(net, x.to(dtype), lmask, amask), y.to(dtype))
        v.backward()
        out[dtype] = ({k: p.grad.numpy() for k, p in net.named_parameters()}, float(v.detach()))
    return out


def check_against_autograd(m, x, y, label, **kw):
    from onset_fingerprinting_amd import model
    loss, grads = model.rnn_loss_and_grads_device(m, x.cuda(), y.cuda(), **kw)
    lmask = amask = None
    if kw:
        n, T = x.shape[0], x.shape[2] if m.permute_input else x.shape[1]
        L, H, p = m.rnn.num_layers, m.rnn.hidden_size, m.attention.dropout
        lmask = R.layer_dropout_mask(kw["seed"], kw["epoch"], L - 1, n, T, H, p) if L > 1 else None
        amask = AR.attention_dropout_mask(kw["seed"], kw["epoch"], n, m.attention.num_heads, T, p)
    ref = autograd_reference(m, x, y, lmask, amask)
    check_grads(grads, loss, ref[torch.float32][0], ref[torch.float64][0], ref[torch.float64][1], y.numel(), label)


@pytest.mark.parametrize("case", CASES)
def test_gradients_at_the_start(g, case):
    from onset_fingerprinting_amd import model
    cfg, m, x, y, _val = load_case(g, case)
    loss, grads = model.rnn_loss_and_grads_device(m, x.cuda(), y.cuda())
    pre32, pre64 = f"{case}/g32/", f"{case}/g64/"
    g32 = {k[len(pre32):]: g[k] for k in g.files if k.startswith(pre32)}
    g64 = {k[len(pre64):]: g[k] for k in g.files if k.startswith(pre64)}
    check_grads(grads, loss, g32, g64, float(g[f"{case}/loss64"]), 2 * len(x), case)


@pytest.mark.parametrize("n", [65, 257, 1024])
def test_gradients_past_one_slab_and_one_chunk(g, n):
    """The first case widened: n * T = 32 n rows cross the slabs of the dense layers (256 rows), of the input
    projection (2048) and of LayerNorm (256), n the head's chunks of 64 samples and the GRU's 32 sequences per
    workgroup."""
    _cfg, m, _x, _y, _val = load_case(g, CASES[0])
    torch.manual_seed(n)
    check_against_autograd(m, torch.randn(n, 3, 32), torch.randn(n, 2), f"n{n}")


def test_gradients_of_the_class_default():
    from onset_fingerprinting_amd import model
    torch.manual_seed(11)
    m = model.RNN(256, 2, 3, dropout_rate=0)
    check_against_autograd(m, torch.randn(3, 3, 256), torch.randn(3, 2), "default")


VARIANTS = {
    "input_size_129": (dict(hidden_size=4), 129), "input_size_512": (dict(hidden_size=4), 512),
    "one_layer": (dict(hidden_size=8, num_layers=1), 24), "four_layers": (dict(hidden_size=8, num_layers=4), 24),
    "one_head": (dict(hidden_size=8, num_heads=1), 24), "four_heads": (dict(hidden_size=8, num_heads=4), 24),
    "not_permuted": (dict(hidden_size=8, permute_input=False), 24), "mse": (dict(hidden_size=8, loss=F.mse_loss), 24),
}


@pytest.mark.parametrize("name", list(VARIANTS))
def test_gradients_of_the_variants(name):
    from onset_fingerprinting_amd import model
    kw, T = VARIANTS[name]
    torch.manual_seed(len(name))
    m = model.RNN(T, 2, channels=3, dropout_rate=0.0, **kw)
    n = 2 if T > 100 else 5
    x = torch.randn(n, T, 3) if not m.permute_input else torch.randn(n, 3, T)
    check_against_autograd(m, x, torch.randn(n, 2), name)


@pytest.mark.parametrize("layers", [1, 2, 3])
def test_gradients_with_dropout(layers):
    """dropout_rate 0.5 and a seed: against float64 autograd over the formulas under this package's two masks."""
    from onset_fingerprinting_amd import model
    torch.manual_seed(layers)
    m = model.RNN(24, 2, channels=3, hidden_size=8, num_layers=layers, dropout_rate=0.5)
    check_against_autograd(m, torch.randn(6, 3, 24), torch.randn(6, 2), f"dropout L{layers}", seed=12345, epoch=2)


# ---- the epoch ------------------------------------------------------------------------------------------------------
def epoch_start():
    """30 validation windows > 20 training windows."""
    from onset_fingerprinting_amd import model
    torch.manual_seed(20)
    m = model.RNN(32, 2, channels=3, hidden_size=8, dropout_rate=0.0, lr=0.01)
    return m, torch.randn(20, 3, 32), torch.randn(20, 2), torch.randn(30, 3, 32), torch.randn(30, 2)


def torch_epochs(start, x, y, xv, yv, epochs, dtype):
    net = copy.deepcopy(start).cpu().to(dtype).train()
    opt = torch.optim.NAdam(net.parameters(), lr=start.lr, weight_decay=1e-4)
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, 3000)
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
    fit = model.fit_rnn(m, x.cuda(), y.cuda(), x_val=xv.cuda(), y_val=yv.cuda(), max_epochs=2)
    assert fit.epochs == 2 and not m.training
    assert np.array_equal(fit.lrs, model.rnn_rates(0.01, 2))
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
    fit = model.fit_rnn(m, x.cuda(), y.cuda(), x_val=xv.cuda(), y_val=yv.cuda(), max_epochs=5)
    flat = torch.cat([t.detach().reshape(-1).float() for t in m.state_dict().values()])
    return fit.train_loss.cpu().numpy(), fit.val_loss.cpu().numpy(), flat.cpu().numpy()


def test_two_fits_and_plain_launches_give_the_same_bits(tmp_path):
    """Five epochs twice as a replayed graph here, and once as plain launches (OFP_RNN_GRAPH=nodes) in a fresh child
    process."""
    a, b = five_epochs(), five_epochs()
    assert np.isfinite(a[0]).all() and np.isfinite(a[1]).all()
    for u, v in zip(a, b):
        assert np.array_equal(u.view(np.uint32), v.view(np.uint32))
    out = tmp_path / "nodes.npz"
    code = ("import sys, numpy as np; sys.path[:0] = [sys.argv[1], sys.argv[2]]; import test_gpu_rnn_train as t; "
            "tl, vl, flat = t.five_epochs(); np.savez(sys.argv[3], tl=tl, vl=vl, flat=flat)")
    env = dict(os.environ, OFP_RNN_GRAPH="nodes")
    done = subprocess.run([sys.executable, "-c", code, str(REPO), str(REPO / "tests"), str(out)], env=env, timeout=300,
                          capture_output=True, text=True)
    assert done.returncode == 0, done.stderr[-2000:]
    c = np.load(out)
    for u, v in zip(a, (c["tl"], c["vl"], c["flat"])):
        assert np.array_equal(u.view(np.uint32), v.view(np.uint32)), "graph replay and plain launches differ"


# ---- training runs --------------------------------------------------------------------------------------------------
_runs = {}


def our_run(g, case):
    """fit_rnn on the golden's inputs and start, on the GPU; once per case and session."""
    from onset_fingerprinting_amd import model
    if case not in _runs:
        cfg, m, x, y, val = load_case(g, case)
        m = m.cuda()
        kw = dict(x_val=val[0].cuda(), y_val=val[1].cuda(), patience=cfg["patience"]) if val else {}
        fit = model.fit_rnn(m, x.cuda(), y.cuda(), max_epochs=cfg["epochs"], **kw)
        _runs[case] = (m, fit)
    return _runs[case]


def check_curve(case, what, ours, ref, ref64, pert):
    """test_gpu_cnnrnn_train.py's check_curve; the prefix is at least 24 epochs, or all of a run that ends sooner."""
    prefix, spread = C.comparable_prefix(ref, pert)
    assert prefix >= min(24, len(ref))
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
    assert stop == 11 and fit.epochs == stop
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
def dropout_model(g):
    _cfg, m, x, y, _val = load_case(g, CASES[0])
    m.rnn.dropout = m.attention.dropout = 0.5
    return m, x.cuda(), y.cuda()


def dropout_fit(g, epochs, seed):
    from onset_fingerprinting_amd import model
    m, x, y = dropout_model(g)
    m = m.cuda()
    fit = model.fit_rnn(m, x, y, max_epochs=epochs, seed=seed)
    assert fit.epochs == epochs
    return m, fit, x, y


def test_dropout_fit(g):
    from onset_fingerprinting_amd import model
    _m20, fit, x, y = dropout_fit(g, 20, 1)
    curve = fit.train_loss[:20]
    assert bool(torch.isfinite(curve).all())
    start = dropout_model(g)[0]
    m7, _f7, _x, _y = dropout_fit(g, 7, 1)
    for e, net in ((0, start.cuda()), (7, m7)):
        loss, _g = model.rnn_loss_and_grads_device(net, x, y, seed=1, epoch=e)
        print(f"epoch {e}: the fit's loss {float(curve[e]):.9g}, loss and gradients on that epoch's parameters "
              f"{float(loss):.9g}")
        assert float(loss) == float(curve[e])
    plain, _g = model.rnn_loss_and_grads_device(load_case(g, CASES[0])[1].cuda(), x, y)
    assert float(plain) != float(curve[0]), "the dropout changed nothing"
    _m, again, _x, _y = dropout_fit(g, 20, 1)
    assert torch.equal(again.train_loss.view(torch.int32), fit.train_loss.view(torch.int32))
    _m, other, _x, _y = dropout_fit(g, 20, 2)
    assert not torch.equal(other.train_loss.view(torch.int32), fit.train_loss.view(torch.int32))
    # both masks of any epoch can be had again
    for e in (0, 19):
        lm = model.rnn_layer_dropout_mask_device(1, e, 1, 24, 32, 8, 0.5).cpu().numpy()
        am = model.attention_dropout_mask_device(1, e, 24, 2, 32, 0.5).cpu().numpy()
        assert np.array_equal(lm, R.layer_dropout_mask(1, e, 1, 24, 32, 8, 0.5))
        assert np.array_equal(am, AR.attention_dropout_mask(1, e, 24, 2, 32, 0.5))


def test_window_source(g):
    from onset_fingerprinting_amd import data, model
    audio, onsets, y = RR.synthetic_hits(8, 10, 3, 32, 3)
    src = data.ShiftedWindows(audio, onsets, 32, pre_samples=2, max_shift=3, n_extractions=2)
    _cfg, m, _x, _y, _v = load_case(g, CASES[0])
    m = m.cuda()
    yt = torch.from_numpy(y)
    first, _g = model.rnn_loss_and_grads_device(copy.deepcopy(m), src.windows(4, 0), yt.repeat(2, 1).cuda())
    fit = model.fit_rnn(m, src, yt, max_epochs=5, seed=4)
    print(f"window source: first loss {float(fit.train_loss[0]):.9g}, on the windows of epoch 0 {float(first):.9g}")
    assert fit.epochs == 5 and bool(torch.isfinite(fit.train_loss[:5]).all())
    assert float(fit.train_loss[0]) == float(first)
    again = model.fit_rnn(load_case(g, CASES[0])[1].cuda(), src, yt, max_epochs=5, seed=4)
    assert torch.equal(again.train_loss.view(torch.int32), fit.train_loss.view(torch.int32))


def test_workspace_of_the_default_shape_is_reported():
    """The plan's work space at the class default and B = 620: probs and ds are n x 2 x 256^2 floats each."""
    from onset_fingerprinting_amd import model
    m = model.RNN(256, 2, 3, dropout_rate=0)
    nbytes = model.rnn_train_workspace_bytes(m, 620)
    sq = 620 * 2 * 256 * 256 * 4
    print(f"work space at B = 620: {nbytes / 1e6:.0f} MB, of which probs and ds {2 * sq / 1e6:.0f} MB")
    assert 2 * sq < nbytes < 12 * sq
