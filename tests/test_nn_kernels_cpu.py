"""The fp64 references and error bounds of oracle/nn_kernels.py, checked without a GPU.

1. Every reference agrees with torch's float64 functional op to 1e-12.
2. For every kernel a float32 emulation that follows the kernel's order of operations (fma chains in k order,
   the lane-strided sums and butterflies, the online softmax over key tiles of 16) stays inside the bound at
   every shape that tests/test_gpu_nn_kernels.py runs: the bounds do not reject a correct fp32 evaluation.
3. The same emulation with one planted fault (a dropped tap, a shifted pool pair, the neighbouring group's or
   head's columns, an unbiased variance, a phantom key in the last tile, a mean over T-1) leaves the bound on
   at least one element of every case the fault can touch: the bounds would catch a subtly wrong kernel.
"""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import nn_kernels as K

f32, f64 = np.float32, np.float64

TORCH_ACT = {K.ACT_IDENTITY: lambda v: v, K.ACT_RELU: F.relu, K.ACT_SILU: F.silu, K.ACT_LEAKYRELU: F.leaky_relu,
             K.ACT_ELU: F.elu, K.ACT_TANH: torch.tanh}


def t64(a):
    return None if a is None else torch.from_numpy(np.asarray(a, f64))


def rnd(rng, *shape):
    return rng.standard_normal(shape).astype(f32)


# ---- float32 emulations ------------------------------------------------------------------------------------------

def fma(a, b, c):
    """fp32 fma: the product of two floats is exact in double, the sum rounds once more (to double) before the
    rounding to float."""
    return (np.asarray(a, f64) * np.asarray(b, f64) + np.asarray(c, f64)).astype(f32)


def act32(v, act):
    v = np.asarray(v, f32)
    if act == K.ACT_RELU:
        return np.where(v > 0, v, f32(0))
    if act == K.ACT_SILU:
        return v / (f32(1) + np.exp(-v))
    if act == K.ACT_LEAKYRELU:
        return np.where(v >= 0, v, f32(0.01) * v)
    if act == K.ACT_ELU:
        return np.where(v > 0, v, np.expm1(np.minimum(v, f32(0))))
    if act == K.ACT_TANH:
        return np.tanh(v)
    return v


def emu_dense_acc(x, w, fault=None):
    """k_dense's accumulator: one fma per k, in k order.  fault 'last_k': the k loop stops one short."""
    acc = np.zeros((x.shape[0], w.shape[0]), f32)
    for k in range(x.shape[1] - (fault == "last_k")):
        acc = fma(x[:, k:k + 1], w[None, :, k], acc)
    return acc


def emu_dense_epilogue(acc, b, scale, shift, act):
    v = acc + (b if b is not None else f32(0))
    v = v * (scale if scale is not None else f32(1)) + (shift if shift is not None else f32(0))
    return act32(v.astype(f32), act)


def emu_conv1d(x, wt, b, stride, padding, dilation, groups, act, sc, sh, pool, fault=None):
    """k_conv1d: acc starts at the bias, one fma per (ci, kk) in that order (a tap outside the input adds an
    exact zero), activation, fma with the affine, max of the pool pair.
    faults: 'last_tap' drops kk = k-1; 'pool_shift' pools (2p+1, 2p+2); 'group' reads the next group's input."""
    n, cin, w = x.shape
    cout, cin_g, k = wt.shape
    cout_g = cout // groups
    wc = K.conv_width(w, k, padding, dilation, stride)
    xp = np.zeros((n, cin, w + 2 * padding + 2 * stride), f32)  # room for the shifted pool pair
    xp[:, :, padding:padding + w] = x
    wcx = wc + 1 if fault == "pool_shift" else wc
    v = np.zeros((n, cout, wcx), f32)
    for g in range(groups):
        gi = (g + 1) % groups if fault == "group" else g
        acc = np.zeros((n, cout_g, wcx), f32)
        if b is not None:
            acc += b[None, g * cout_g:(g + 1) * cout_g, None]
        for ci in range(cin_g):
            for kk in range(k - (fault == "last_tap")):
                seg = xp[:, gi * cin_g + ci, kk * dilation: kk * dilation + (wcx - 1) * stride + 1: stride]
                acc = fma(seg[:, None, :], wt[None, g * cout_g:(g + 1) * cout_g, ci, kk, None], acc)
        v[:, g * cout_g:(g + 1) * cout_g] = acc
    v = act32(v, act)
    if sc is not None:
        v = fma(v, sc[None, :, None], sh[None, :, None])
    if pool:
        wo, o = wc // 2, int(fault == "pool_shift")
        v = np.maximum(v[:, :, o:o + 2 * wo:2], v[:, :, o + 1:o + 1 + 2 * wo:2])
    return v[:, :, :wc] if not pool else v


def emu_groupnorm1(x, g, bt, eps, pool, fault=None):
    """k_groupnorm1: sums in double, mean and rstd rounded to float, the apply in float.
    fault 'unbiased': the variance divides by K V - 1."""
    n, Kc, V = x.shape
    xd = x.astype(f64).reshape(n, -1)
    cnt = Kc * V
    mean = xd.sum(1) / cnt
    var = np.maximum((xd * xd).sum(1) / cnt - mean * mean, 0.0)
    if fault == "unbiased":
        var = var * cnt / (cnt - 1)
    m32, r32 = mean.astype(f32)[:, None, None], (1.0 / np.sqrt(var + f64(f32(eps)))).astype(f32)[:, None, None]
    gg = (g if g is not None else np.ones(Kc, f32))[None, :, None]
    bb = (bt if bt is not None else np.zeros(Kc, f32))[None, :, None]
    y = (x - m32) * r32 * gg + bb
    if pool:
        vo = V // 2
        y = np.maximum(y[:, :, 0:2 * vo:2], y[:, :, 1:2 * vo:2])
    return y


def lane_sum(v, lanes):
    """Sum over the last axis as `lanes` strided partial sums (sequential per lane), then an xor butterfly."""
    n, L = v.shape
    pad = np.zeros((n, -(-L // lanes) * lanes), f32)
    pad[:, :L] = v
    pad = pad.reshape(n, -1, lanes)
    s = np.zeros((n, lanes), f32)
    for i in range(pad.shape[1]):
        s = s + pad[:, i]
    idx = np.arange(lanes)
    o = lanes // 2
    while o:
        s = s + s[:, idx ^ o]
        o //= 2
    return s[:, 0]


def emu_autocorr_softmax(x, fault=None):
    """k_autocorr_softmax: per lag one fma chain over (k, i), a term outside the overlap adding an exact zero;
    max, expf, the sum (256 strided partial sums, butterflies), the division.
    fault 'last_term': the positive lags stop one term short (hi = V - sh - 1)."""
    n, Kc, V = x.shape
    L = 2 * V - 1
    xp = np.zeros((n, Kc, 3 * V - 2), f32)
    xp[:, :, V - 1:2 * V - 1] = x
    sh = np.arange(L) - (V - 1)
    acc = np.zeros((n, L), f32)
    for k in range(Kc):
        for i in range(V):
            other = xp[:, k, i:i + L]  # f[i + sh] for every lag
            if fault == "last_term":
                other = np.where((sh > 0) & (i == V - sh - 1), f32(0), other)
            acc = fma(other, x[:, k, i:i + 1], acc)
    m = acc.max(axis=1, keepdims=True)
    e = np.exp(acc - m)
    return e / lane_sum(e, 256)[:, None]


def emu_layernorm(x, g, bt, eps, fault=None):
    """k_layernorm: two passes over 64 lanes in float.  fault 'unbiased': the variance divides by E - 1."""
    n, E = x.shape
    mean = (lane_sum(x, 64) / f32(E))[:, None]
    d = x - mean
    ss = lane_sum(d * d, 64)
    rstd = (f32(1) / np.sqrt(ss / f32(E - 1 if fault == "unbiased" else E) + f32(eps)))[:, None]
    v = (x - mean) * rstd
    return (v * (g if g is not None else f32(1)) + (bt if bt is not None else f32(0))).astype(f32)


def emu_attention_mean(qkv, nh, fault=None):
    """k_attn_mean for all heads at once: scores as fma chains over d, keys in tiles of 16 with the online
    softmax, P V as fma chains over the 16 keys, o / l, the query rows summed per tile, the tiles per wave
    (tile % 4), the four waves in order, and the division by T.
    faults: 'phantom_key' lets the first padding key of a partial tile through (score 0, v = 0);
    'next_head' takes v from head h+1's columns; 'mean' divides by T - 1."""
    n, T, E3 = qkv.shape
    E = E3 // 3
    d = E // nh
    split = lambda a: np.ascontiguousarray(a.reshape(n, T, nh, d).transpose(0, 2, 1, 3))  # [n, nh, T, d]
    q, k, v = split(qkv[:, :, :E]), split(qkv[:, :, E:2 * E]), split(qkv[:, :, 2 * E:])
    if fault == "next_head":
        v = np.roll(v, -1, axis=1)
    scale = f32(1.0) / np.sqrt(f32(d))
    Tp = -(-T // 16) * 16
    s = np.zeros((n, nh, T, Tp), f32)
    kp = np.zeros((n, nh, Tp, d), f32)
    vp = np.zeros((n, nh, Tp, d), f32)
    kp[:, :, :T], vp[:, :, :T] = k, v
    for i in range(d):
        s = fma(q[:, :, :, None, i], kp[:, :, None, :, i], s)
    s = s * scale
    valid = np.arange(Tp) < (T + 1 if fault == "phantom_key" else T)
    s = np.where(valid[None, None, None, :], s, f32(-np.inf))
    m = np.full((n, nh, T), -np.inf, f32)
    l = np.zeros((n, nh, T), f32)
    o = np.zeros((n, nh, T, d), f32)
    for kt in range(Tp // 16):
        st = s[..., kt * 16:(kt + 1) * 16]
        mn = np.maximum(m, st.max(axis=-1))
        with np.errstate(invalid="ignore"):
            alpha = np.exp(m - mn)
        p = np.exp(st - mn[..., None])
        ps = lane_sum(p.reshape(-1, 16), 16).reshape(n, nh, T)
        l = l * alpha + ps
        m = mn
        o = o * alpha[..., None]
        for j in range(16):
            o = fma(p[..., j:j + 1], vp[:, :, None, kt * 16 + j, :], o)
    ctx = o / l[..., None]
    part = np.zeros((4, n, nh, d), f32)
    for qt in range(Tp // 16):
        rows = ctx[:, :, qt * 16:min(T, (qt + 1) * 16)]
        cs = np.zeros((n, nh, d), f32)
        for r in range(rows.shape[2]):
            cs = cs + rows[:, :, r]
        part[qt % 4] += cs
    tot = ((part[0] + part[1]) + part[2]) + part[3]
    out = tot / f32(T - 1 if fault == "mean" else T)
    return out.reshape(n, E)


def inside(got, ref, bound):
    return bool(np.all(np.abs(np.asarray(got, f64) - ref) <= bound))


def worst(got, ref, bound):
    return float(np.max(np.abs(np.asarray(got, f64) - ref) / bound))


# ---- dense -------------------------------------------------------------------------------------------------------

def dense_variants(rng, out):
    b, sc, sh = rnd(rng, out), (0.5 + rng.random(out)).astype(f32), rnd(rng, out)
    return [(None, None, None), (b, None, None), (None, sc, sh), (b, sc, sh)]


def test_dense_ref_matches_torch_float64():
    rng = np.random.default_rng(1)
    for n, fin, out in ((1, 1, 1), (17, 5, 15), (33, 257, 40)):
        x, w = rnd(rng, n, fin), rnd(rng, out, fin)
        for act in K.ACTS:
            for b, sc, sh in dense_variants(rng, out):
                want = F.linear(t64(x), t64(w), t64(b))
                if sc is not None:
                    want = want * t64(sc) + t64(sh)
                want = TORCH_ACT[act](want).numpy()
                ref, bound = K.dense_ref(x, w, b, sc, sh, act)
                assert ref.dtype == f64 and np.abs(ref - want).max() <= 1e-12
                assert bound.shape == ref.shape and np.all(bound > 0)


def test_dense_emulation_inside_bound_and_fault_outside():
    rng = np.random.default_rng(2)
    for n in K.DENSE_N:
        for fin in K.DENSE_IN:
            for out in K.DENSE_OUT:
                x, w = rnd(rng, n, fin), rnd(rng, out, fin)
                acc, bad = emu_dense_acc(x, w), emu_dense_acc(x, w, "last_k")
                for act in K.ACTS:
                    for b, sc, sh in dense_variants(rng, out):
                        ref, bound = K.dense_ref(x, w, b, sc, sh, act)
                        got = emu_dense_epilogue(acc, b, sc, sh, act)
                        assert inside(got, ref, bound), (n, fin, out, act, worst(got, ref, bound))
                        # without a flat part every shape shows the fault; a few dozen outputs of ReLU, SiLU, ELU
                        # or tanh can all sit where the activation no longer moves
                        if act in (K.ACT_IDENTITY, K.ACT_LEAKYRELU) or n * out >= 64:
                            assert not inside(emu_dense_epilogue(bad, b, sc, sh, act), ref, bound), (n, fin, out, act)


# ---- conv1d ------------------------------------------------------------------------------------------------------

def test_conv_case_table_reaches_every_edge_the_kernel_has():
    cases = [c for w in K.CONV_W for c in K.conv_cases(w)]
    for key, values in (("w", K.CONV_W), ("k", K.CONV_K), ("dilation", K.CONV_DILATION), ("stride", K.CONV_STRIDE),
                        ("groups", K.CONV_GROUPS), ("act", K.ACTS), ("padding", (0, 1, 2, 3, 4, 5, 7))):
        for v in values:
            assert sum(c[key] == v for c in cases) >= 2, (key, v)
    for k in K.CONV_K:
        assert {c["padding"] for c in cases if c["k"] == k} == {0, 1, k - 1, k + 2}
    assert any(c["pool"] and c["wc"] % 2 == 1 and c["wc"] > 1 for c in cases)  # pool on an odd pre-pool width
    assert any(c["pool"] and c["stride"] > 1 for c in cases)  # pool together with stride
    assert any(c["pool"] and c["stride"] > 1 and c["dilation"] > 1 and c["groups"] > 1 for c in cases)
    assert any(c["wc"] == 1 for c in cases) and any(c["pool"] and c["wc"] // 2 == 1 for c in cases)  # wout == 1
    assert any(not c["bias"] for c in cases) and any(c["affine"] for c in cases)
    assert any(c["affine"] and c["pool"] and not c["bias"] for c in cases)
    assert any(c["groups"] == K.CONV_CIN and c["pool"] for c in cases)  # depthwise
    g = K.CONV_STRIDE_CASE
    assert g["n"] * g["cout"] * K.conv_width(g["w"], g["k"], g["padding"], 1, 1) == 1081344 > 256 * 16 * 256


def conv_torch(x, wt, b, c, sc, sh):
    y = F.conv1d(t64(x), t64(wt), t64(b), stride=c["stride"], padding=c["padding"], dilation=c["dilation"],
                 groups=c["groups"])
    y = TORCH_ACT[c["act"]](y)
    if sc is not None:
        y = y * t64(sc)[None, :, None] + t64(sh)[None, :, None]
    return (F.max_pool1d(y, 2, 2) if c["pool"] else y).numpy()


@pytest.mark.parametrize("w", K.CONV_W)
def test_conv1d_ref_matches_torch_and_emulation_inside_bound_and_faults_outside(w):
    hit = {"last_tap": 0, "pool_shift": 0, "group": 0}
    for i, c in enumerate(K.conv_cases(w)):
        x, wt, b, sc, sh = K.conv_inputs(c, 1000 * w + i)
        kw = dict(stride=c["stride"], padding=c["padding"], dilation=c["dilation"], groups=c["groups"], act=c["act"],
                  pool=c["pool"])
        ref, bound = K.conv1d_ref(x, wt, b, bn_scale=sc, bn_shift=sh, **kw)
        want = conv_torch(x, wt, b, c, sc, sh)
        assert ref.shape == want.shape == (K.CONV_N, K.CONV_COUT, c["wc"] // 2 if c["pool"] else c["wc"])
        assert np.abs(ref - want).max() <= 1e-12, c
        args = (x, wt, b, c["stride"], c["padding"], c["dilation"], c["groups"], c["act"], sc, sh, c["pool"])
        got = emu_conv1d(*args)
        assert inside(got, ref, bound), (c, worst(got, ref, bound))
        # a fault shows only where the taps it changes read real input (not only padding) at an output position
        # that survives the pool
        kept = range(2 * (c["wc"] // 2) if c["pool"] else c["wc"])
        real = lambda taps: any(0 <= p * c["stride"] - c["padding"] + kk * c["dilation"] < w for p in kept for kk in taps)
        faults = ["last_tap"] if real([c["k"] - 1]) else []
        if c["pool"] and c["wc"] >= 3 and w >= 7:  # narrower inputs pool mostly padding, where every column is equal
            faults.append("pool_shift")
        if c["groups"] > 1 and real(range(c["k"])):
            faults.append("group")
        for fault in faults:
            assert not inside(emu_conv1d(*args, fault=fault), ref, bound), (c, fault)
            hit[fault] += 1
    assert hit["last_tap"] and hit["group"] and (hit["pool_shift"] or w < 7)


# ---- groupnorm ---------------------------------------------------------------------------------------------------

def groupnorm_sets(Kc, V, n, seed):
    """(x, gamma, beta, pool) of every variant the GPU test runs at this shape."""
    rng = np.random.default_rng(seed)
    x, g, bt = rnd(rng, n, Kc, V), rnd(rng, Kc), rnd(rng, Kc)
    sets = [(x, g, bt, False), (x, None, None, False), (x + f32(1000), g, bt, False)]
    if V >= 2:
        sets += [(x, g, bt, True), (x + f32(1000), None, None, True)]
    return sets


@pytest.mark.parametrize("Kc,V", K.GROUPNORM_KV)
def test_groupnorm_ref_matches_torch_and_emulation_inside_bound_and_fault_outside(Kc, V):
    for n in K.GROUPNORM_N:
        for x, g, bt, pool in groupnorm_sets(Kc, V, n, 31 * Kc + V + n):
            ref, bound = K.groupnorm1_ref(x, g, bt, 1e-5, pool)
            if Kc * V == 1:  # torch refuses a single value per group: the output is beta
                assert np.array_equal(ref, np.broadcast_to(0.0 if bt is None else bt.astype(f64)[None, :, None], ref.shape))
            elif abs(float(x.mean())) < 100:  # torch's own double loses digits to the offset of 1000
                want = F.group_norm(t64(x), 1, t64(g), t64(bt), 1e-5)
                want = (F.max_pool1d(want, 2, 2) if pool else want).numpy()
                assert np.abs(ref - want).max() <= 1e-12
            got = emu_groupnorm1(x, g, bt, 1e-5, pool)
            assert got.shape == ref.shape and inside(got, ref, bound), (n, pool, worst(got, ref, bound))
            if Kc * V >= 2 and abs(float(x.mean())) < 100:
                assert not inside(emu_groupnorm1(x, g, bt, 1e-5, pool, "unbiased"), ref, bound), (n, pool)


def test_groupnorm_pool_floor_is_part_of_the_reference():
    x = rnd(np.random.default_rng(3), 2, 3, 7)
    ref, bound = K.groupnorm1_ref(x, None, None, 1e-5, True)
    full, _ = K.groupnorm1_ref(x, None, None, 1e-5, False)
    assert ref.shape == (2, 3, 3) and np.array_equal(ref[:, :, 2], np.maximum(full[:, :, 4], full[:, :, 5]))
    ceil_last = full[:, :, 6]  # what a ceil-mode pool would put into a fourth column
    assert not np.all(np.abs(ceil_last - ref[:, :, 2]) <= bound[:, :, 2])


# ---- autocorr_softmax --------------------------------------------------------------------------------------------

def autocorr_torch(x):
    n, Kc, V = x.shape
    xt = t64(x)
    cc = torch.stack([F.conv1d(xt[s][None], xt[s][:, None, :], padding=V - 1, groups=Kc)[0].sum(0) for s in range(n)])
    return torch.softmax(cc, dim=1).numpy()


@pytest.mark.parametrize("V", K.AUTOCORR_V)
def test_autocorr_softmax_ref_matches_torch_and_emulation_inside_bound_and_fault_outside(V):
    for Kc in K.AUTOCORR_K:
        rng = np.random.default_rng(100 * V + Kc)
        for scale in (1.0 / math.sqrt(V), 1.0):
            x = (rnd(rng, 3, Kc, V) * f32(scale)).astype(f32)
            ref, bound = K.autocorr_softmax_ref(x)
            assert ref.shape == (3, 2 * V - 1) and np.abs(ref - autocorr_torch(x)).max() <= 1e-12
            assert np.abs(ref.sum(1) - 1).max() < 1e-12
            got = emu_autocorr_softmax(x)
            assert inside(got, ref, bound), (Kc, V, scale, worst(got, ref, bound))
            if V >= 2 and scale < 1.0:
                assert not inside(emu_autocorr_softmax(x, "last_term"), ref, bound), (Kc, V)


# ---- layernorm ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("E", K.LAYERNORM_E)
def test_layernorm_ref_matches_torch_and_emulation_inside_bound_and_fault_outside(E):
    for n in K.LAYERNORM_N:
        rng = np.random.default_rng(7 * E + n)
        x, g, bt = rnd(rng, n, E), rnd(rng, E), rnd(rng, E)
        for xx, gg, bb in ((x, g, bt), (x, None, None), (x + f32(1000), g, bt)):
            ref, bound = K.layernorm_ref(xx, gg, bb, 1e-5)
            if xx is x:
                want = F.layer_norm(t64(xx), (E,), t64(gg), t64(bb), 1e-5).numpy()
                assert np.abs(ref - want).max() <= 1e-12
            got = emu_layernorm(xx, gg, bb, 1e-5)
            assert inside(got, ref, bound), (n, worst(got, ref, bound))
            if E >= 2 and xx is x:
                assert not inside(emu_layernorm(xx, gg, bb, 1e-5, "unbiased"), ref, bound), n


# ---- attention_mean ----------------------------------------------------------------------------------------------

def test_attention_ref_matches_torch_multihead_attention_before_out_proj():
    torch.manual_seed(5)
    for d, nh, T, n in ((1, 1, 1, 1), (3, 2, 17, 3), (20, 3, 33, 2), (65, 2, 16, 1)):
        E = d * nh
        mha = torch.nn.MultiheadAttention(E, nh, batch_first=True).double().eval()
        with torch.no_grad():
            mha.in_proj_bias.normal_()
            mha.out_proj.weight.copy_(torch.eye(E))
            mha.out_proj.bias.zero_()
            x = torch.randn(n, T, E, dtype=torch.float64)
            want = mha(x, x, x, need_weights=False)[0].mean(1).numpy()
            qkv = F.linear(x, mha.in_proj_weight, mha.in_proj_bias).numpy()
        ref, bound = K.attention_mean_ref(qkv, nh)
        assert ref.shape == (n, E) and np.abs(ref - want).max() <= 1e-12
        assert np.all(bound > 0)


def attention_qkv(d, nh, T, n, peaked=False):
    rng = np.random.default_rng(((d * 4 + nh) * 100 + T) * 4 + n)
    qkv = rnd(rng, n, T, 3 * d * nh)
    if peaked:
        qkv[:, :, :d * nh] *= f32(8)
    return qkv


@pytest.mark.parametrize("d", K.ATTN_D)
def test_attention_emulation_inside_bound_and_faults_outside(d):
    for nh in K.ATTN_HEADS:
        for T in K.ATTN_T:
            for n in K.ATTN_NSEQ:
                for peaked in ((False, True) if (T, n) == (33, 3) else (False,)):
                    qkv = attention_qkv(d, nh, T, n, peaked)
                    ref, bound = K.attention_mean_ref(qkv, nh)
                    got = emu_attention_mean(qkv, nh)
                    assert inside(got, ref, bound), (nh, T, n, peaked, worst(got, ref, bound))
                    faults = (["mean"] if T >= 2 else []) + (["next_head"] if nh >= 2 else [])
                    faults += ["phantom_key"] if T % 16 and not peaked else []  # peaked rows give a score of 0 no weight
                    for fault in faults:
                        assert not inside(emu_attention_mean(qkv, nh, fault), ref, bound), (nh, T, n, peaked, fault)


# ---- the recurrent kernel's case table ---------------------------------------------------------------------------

def test_rnn_table_lists_every_reachable_instantiation():
    """Host rules of ofp_rnn_layer: tiles = ceil(H / 16) on min(tiles, 4) waves, NT = tiles per wave (3 runs as
    4), W_hh resident while (32 + G kh)(kh + 4) floats fit 160 KiB, projection precomputed beyond 8 features."""
    reachable = {(cell,) + K.rnn_instantiation(cell, H, F) for cell in K.RNN_CELL_GATES for H in range(1, 257)
                 for F in (K.RNN_F_INLINE, K.RNN_F_PROJECTED)}
    assert len(reachable) == 32
    listed = set()
    for cell, H, F, inst, _note in K.RNN_TABLE:
        assert K.rnn_instantiation(cell, H, F) == inst, (cell, H, F)
        listed.add((cell,) + inst)
    assert listed == reachable
    tiles3 = {(c, i[1]) for c, H, F, i, _ in K.RNN_TABLE if (H + 15) // 16 in (9, 10, 11, 12)}
    assert {c for c, _ in tiles3} == set(K.RNN_CELL_GATES)  # three tiles per wave, every cell
    assert any(not i[1] and H % 4 for _c, H, _F, i, _ in K.RNN_TABLE)  # streamed, scalar tail
    rows = {(c, H, F) for c, H, F, _i, _ in K.RNN_TABLE}
    assert K.RNN_NO_BIAS <= rows and set(K.RNN_SATURATED) <= rows
    assert {c for c, _, _ in K.RNN_SATURATED} == set(K.RNN_CELL_GATES)
