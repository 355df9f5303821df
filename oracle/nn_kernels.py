"""fp64 references of the classifier kernels, one per kernel, each with an element-wise error bound
-- TEST INFRASTRUCTURE ONLY.

csrc/ofp_nn.hip (ofp_dense, ofp_conv1d, ofp_groupnorm1, ofp_autocorr_softmax) and csrc/ofp_rnn.hip
(ofp_layernorm, ofp_attention_mean) are compared against these element by element:
``|got - ref| <= bound``.  The references are written from the formulas with explicit loops and einsum;
they call neither the code under test nor torch.  Every bound is derived from fp32 arithmetic with unit
roundoff ``U = 2^-24`` and is not tuned to the kernels:

dense / conv1d
    A dot product of n_terms fp32 fma steps is off by at most n_terms * U * sum|x w| (to first order);
    bias, scale, shift and the store add four more roundings of values no larger than
    A = (sum|x w| + |b|) |scale| + |shift|.  The activation maps that error with its Lipschitz constant
    (1.1 for SiLU, whose slope peaks at 1.0998; 1 for the others) and adds its own evaluation error, for
    which 4 ulp = 8 U |ref| is allowed.  ASSUMPTION: the HIP math documentation is not available next to
    this file; 4 ulp covers the 1-2 ulp that the ROCm device library documents for expf, expm1f and tanhf
    plus the division.  bound = (n_terms + 4) U A Lip + 8 U |ref|; after MaxPool the larger of the two
    positions' bounds (|max(a, b) - max(a', b')| <= max(|a - a'|, |b - b'|)).
groupnorm (statistics in fp64, rounded to fp32; applied in fp32)
    Rounding the mean moves every output by U |mu| rstd |gamma|.  The product p = (x - mu) rstd gamma
    carries four relative roundings (rstd's own, the subtraction, two multiplications) and |p| = |ref - beta|
    <= |ref| + |beta|; the final sum rounds once more, by U |ref|.  To first order that is
    U (|mu| rstd |gamma| + 5 |ref| + 4 |beta|) <= bound = 2 U (|mu| rstd |gamma| + 4 |ref| + 4 |beta|).
    (With 1 |beta| in place of 4 |beta| the bound does not cover an output where beta cancels the product:
    there the four roundings of p, each up to U |beta|, are all that is left.  The fp32 emulation of
    tests/test_nn_kernels_cpu.py reaches 1.45 times that narrower bound at such an element.)
layernorm (fp32, two passes, 64 lanes)
    A lane sums ceil(E / 64) values, the butterfly adds 6 levels: the mean is off by about
    (ceil(E/64) + 6) U mean|x|, the variance relatively as much, and the apply adds four roundings.
    bound = U (ceil(E/64) + 16) (rstd |gamma_i| (mean_j|x_j| + |x_i - mu|) + |ref_i| + |beta_i|).
autocorr_softmax
    A lag is a dot product of at most K V terms: delta = (K V + 1) U max_j sum|f f|.  A softmax moves
    relatively by at most twice the largest logit error on each side (4 delta in all), the sum of
    L = 2V - 1 terms adds L U and expf and the division 8 U.  bound = p_j (4 delta + (L + 8) U) + 1e-30.
attention_mean
    Per head, a score is a dot product of d terms times 1/sqrt(d): delta = (d + 2) U max_{q,k}
    sum_i|q_i k_i| / sqrt(d).  The probabilities move relatively by 4 delta, the online softmax and the
    P V product sum T terms, rescaling, expf, the division and the mean add a constant number of
    roundings (32 U allowed), and the output is a convex combination of v: bound = (4 delta + (T + 32) U)
    max_t|v_{t,c}|.
"""
import math

import numpy as np

U = 2.0 ** -24

# OFP_ACT_* of include/onsetfp.h
ACT_IDENTITY, ACT_RELU, ACT_SILU, ACT_LEAKYRELU, ACT_ELU, ACT_TANH = range(6)
ACTS = (ACT_IDENTITY, ACT_RELU, ACT_SILU, ACT_LEAKYRELU, ACT_ELU, ACT_TANH)


def activate64(v, act):
    v = np.asarray(v, np.float64)
    if act == ACT_RELU:
        return np.maximum(v, 0.0)
    if act == ACT_SILU:
        return v / (1.0 + np.exp(-v))
    if act == ACT_LEAKYRELU:
        return np.where(v >= 0.0, v, 0.01 * v)
    if act == ACT_ELU:
        return np.where(v > 0.0, v, np.expm1(np.minimum(v, 0.0)))
    if act == ACT_TANH:
        return np.tanh(v)
    assert act == ACT_IDENTITY
    return v


def _lip(act):
    return 1.1 if act == ACT_SILU else 1.0


def _f64(a):
    return None if a is None else np.asarray(a, np.float64)


def dense_ref(x, w, b=None, scale=None, shift=None, act=ACT_IDENTITY):
    """act((x Wᵀ + b) scale + shift): x [n, in], w [out, in], b / scale / shift [out] or None.
    Returns (ref, bound), both float64 [n, out]."""
    x, w, b, scale, shift = map(_f64, (x, w, b, scale, shift))
    n_terms = x.shape[1]
    pre = np.einsum("ni,oi->no", x, w)
    mag = np.einsum("ni,oi->no", np.abs(x), np.abs(w))
    if b is not None:
        pre = pre + b
        mag = mag + np.abs(b)
    if scale is not None:
        pre = pre * scale
        mag = mag * np.abs(scale)
    if shift is not None:
        pre = pre + shift
        mag = mag + np.abs(shift)
    ref = activate64(pre, act)
    return ref, (n_terms + 4) * U * mag * _lip(act) + 8 * U * np.abs(ref)


def conv_width(w, k, padding, dilation, stride):
    """Conv1d's output width before pooling (<= 0: empty)."""
    span = w + 2 * padding - dilation * (k - 1)
    return (span - 1) // stride + 1 if span >= 1 else 0


def conv1d_ref(x, w, b=None, stride=1, padding=0, dilation=1, groups=1, act=ACT_IDENTITY, bn_scale=None,
               bn_shift=None, pool=False):
    """Conv1d -> activation -> per-channel affine -> MaxPool1d(2, 2) (floor): x [n, cin, width],
    w [cout, cin/groups, k].  Returns (ref, bound), float64 [n, cout, wout]."""
    x, w, b, bn_scale, bn_shift = map(_f64, (x, w, b, bn_scale, bn_shift))
    n, cin, width = x.shape
    cout, cin_g, k = w.shape
    assert cin == cin_g * groups and cout % groups == 0
    cout_g = cout // groups
    wc = conv_width(width, k, padding, dilation, stride)
    assert wc >= 1
    xp = np.zeros((n, cin, width + 2 * padding))
    xp[:, :, padding:padding + width] = x
    pre = np.zeros((n, cout, wc))
    mag = np.zeros((n, cout, wc))
    for g in range(groups):
        xs = xp[:, g * cin_g:(g + 1) * cin_g]
        ws = w[g * cout_g:(g + 1) * cout_g]
        for kk in range(k):
            seg = xs[:, :, kk * dilation: kk * dilation + (wc - 1) * stride + 1: stride]  # [n, cin_g, wc]
            pre[:, g * cout_g:(g + 1) * cout_g] += np.einsum("nip,oi->nop", seg, ws[:, :, kk])
            mag[:, g * cout_g:(g + 1) * cout_g] += np.einsum("nip,oi->nop", np.abs(seg), np.abs(ws[:, :, kk]))
    if b is not None:
        pre += b[None, :, None]
        mag += np.abs(b)[None, :, None]
    ref = activate64(pre, act)
    if bn_scale is not None:
        ref = ref * bn_scale[None, :, None] + bn_shift[None, :, None]
        mag = mag * np.abs(bn_scale)[None, :, None] + np.abs(bn_shift)[None, :, None]
    bound = (cin_g * k + 4) * U * mag * _lip(act) + 8 * U * np.abs(ref)
    if pool:
        wo = wc // 2
        assert wo >= 1
        ref = np.maximum(ref[:, :, 0:2 * wo:2], ref[:, :, 1:2 * wo:2])
        bound = np.maximum(bound[:, :, 0:2 * wo:2], bound[:, :, 1:2 * wo:2])
    return ref, bound


def groupnorm1_ref(x, gamma=None, beta=None, eps=1e-5, pool=False):
    """nn.GroupNorm(1, K) (biased variance over all K V values of an item) then optionally
    MaxPool1d(2, 2): x [n, K, V].  Returns (ref, bound), float64 [n, K, V or V // 2]."""
    x, gamma, beta = map(_f64, (x, gamma, beta))
    n, K, V = x.shape
    mu = np.zeros(n)
    var = np.zeros(n)
    for s in range(n):
        mu[s] = math.fsum(x[s].ravel()) / (K * V)
        var[s] = math.fsum(((x[s] - mu[s]) ** 2).ravel()) / (K * V)
    rstd = 1.0 / np.sqrt(var + eps)
    g = np.ones(K) if gamma is None else gamma
    bt = np.zeros(K) if beta is None else beta
    ref = (x - mu[:, None, None]) * rstd[:, None, None] * g[None, :, None] + bt[None, :, None]
    bound = 2 * U * ((np.abs(mu) * rstd)[:, None, None] * np.abs(g)[None, :, None] + 4 * np.abs(ref)
                     + 4 * np.abs(bt)[None, :, None])
    bound = np.broadcast_to(bound, ref.shape)
    if pool:
        vo = V // 2
        assert vo >= 1
        ref = np.maximum(ref[:, :, 0:2 * vo:2], ref[:, :, 1:2 * vo:2])
        bound = np.maximum(bound[:, :, 0:2 * vo:2], bound[:, :, 1:2 * vo:2])
    return ref, bound


def autocorr_lags(x):
    """cc[j] = sum_k sum_i f_k[i + j - (V-1)] f_k[i] for the 2V-1 lags, and the same sum of magnitudes:
    x [n, K, V] -> (cc, mag) float64 [n, 2V-1]."""
    x = _f64(x)
    n, K, V = x.shape
    cc = np.zeros((n, 2 * V - 1))
    mag = np.zeros((n, 2 * V - 1))
    for j in range(2 * V - 1):
        sh = j - (V - 1)
        lo, hi = max(0, -sh), min(V, V - sh)
        prod = x[:, :, lo + sh:hi + sh] * x[:, :, lo:hi]
        cc[:, j] = prod.sum(axis=(1, 2))
        mag[:, j] = np.abs(prod).sum(axis=(1, 2))
    return cc, mag


def autocorr_softmax_ref(x):
    """Auto-correlation of every map, summed over the K maps, soft-maxed over the lags: x [n, K, V].
    Returns (ref, bound), float64 [n, 2V-1]."""
    n, K, V = np.shape(x)
    L = 2 * V - 1
    cc, mag = autocorr_lags(x)
    e = np.exp(cc - cc.max(axis=1, keepdims=True))
    p = e / e.sum(axis=1, keepdims=True)
    delta = (K * V + 1) * U * mag.max(axis=1, keepdims=True)
    return p, p * (4 * delta + (L + 8) * U) + 1e-30


def layernorm_ref(x, gamma=None, beta=None, eps=1e-5):
    """nn.LayerNorm over the last axis: x [n, E].  Returns (ref, bound), float64 [n, E]."""
    x, gamma, beta = map(_f64, (x, gamma, beta))
    n, E = x.shape
    g = np.ones(E) if gamma is None else gamma
    bt = np.zeros(E) if beta is None else beta
    mu = np.array([math.fsum(r) / E for r in x])[:, None]
    var = np.array([math.fsum((r - m) ** 2) / E for r, m in zip(x, mu[:, 0])])[:, None]
    rstd = 1.0 / np.sqrt(var + eps)
    ref = (x - mu) * rstd * g + bt
    mean_abs = np.abs(x).mean(axis=1, keepdims=True)
    bound = U * (-(-E // 64) + 16) * (rstd * np.abs(g) * (mean_abs + np.abs(x - mu)) + np.abs(ref) + np.abs(bt))
    return ref, bound


def attention_mean_ref(qkv, n_heads):
    """mean_t softmax(Q Kᵀ / sqrt(d)) V per head: qkv [n, T, 3E] (q | k | v column blocks, head h in
    columns h d .. h d + d - 1 of each).  Returns (ref, bound), float64 [n, E]."""
    qkv = _f64(qkv)
    n, T, E3 = qkv.shape
    E = E3 // 3
    assert E3 == 3 * E and E % n_heads == 0
    d = E // n_heads
    ref = np.zeros((n, E))
    bound = np.zeros((n, E))
    for h in range(n_heads):
        q = qkv[:, :, h * d:(h + 1) * d]
        k = qkv[:, :, E + h * d:E + (h + 1) * d]
        v = qkv[:, :, 2 * E + h * d:2 * E + (h + 1) * d]
        s = np.einsum("nqi,nki->nqk", q, k) / math.sqrt(d)
        smag = np.einsum("nqi,nki->nqk", np.abs(q), np.abs(k)) / math.sqrt(d)
        e = np.exp(s - s.max(axis=2, keepdims=True))
        p = e / e.sum(axis=2, keepdims=True)
        ref[:, h * d:(h + 1) * d] = np.einsum("nqk,nkc->nqc", p, v).mean(axis=1)
        delta = (d + 2) * U * smag.max(axis=(1, 2))[:, None]
        bound[:, h * d:(h + 1) * d] = (4 * delta + (T + 32) * U) * np.abs(v).max(axis=1)
    return ref, bound


# ---- the shapes both test files run (tests/test_nn_kernels_cpu.py, tests/test_gpu_nn_kernels.py) ---------------

DENSE_N = (1, 15, 16, 17, 33)
DENSE_IN = (1, 3, 4, 5, 64, 257)
DENSE_OUT = (1, 15, 16, 17, 40)
DENSE_STRIDE_CASE = (131072 + 17, 3, 2)  # rows beyond the 131 072 that one pass of k_dense's grid covers

CONV_W = (1, 2, 7, 64, 257)
CONV_K = (1, 2, 3, 5)
CONV_DILATION = (1, 2, 3)
CONV_STRIDE = (1, 2, 3)
CONV_N, CONV_CIN, CONV_COUT = 2, 6, 12
CONV_GROUPS = (1, 2, CONV_CIN)
CONV_STRIDE_CASE = dict(n=33, cin=1, cout=8, w=4096, k=3, padding=1)  # 1 081 344 outputs > 1 048 576


def conv_paddings(k):
    return sorted({0, 1, k - 1, k + 2})


def conv_cases(w):
    """The full product of the conv1d parameters at input width w, less the combinations with an empty
    output.  Pool, bias, folded BatchNorm affine and the activation rotate with the running index (with
    periods 2, 3, 5 and 6), so every one of them meets every parameter value many times; a pool that
    would leave nothing is dropped from that case."""
    out = []
    i = 0
    for k in CONV_K:
        for padding in conv_paddings(k):
            for dilation in CONV_DILATION:
                for stride in CONV_STRIDE:
                    for groups in CONV_GROUPS:
                        i += 1
                        wc = conv_width(w, k, padding, dilation, stride)
                        if wc < 1:
                            continue
                        out.append(dict(w=w, k=k, padding=padding, dilation=dilation, stride=stride, groups=groups,
                                        pool=bool(i % 2) and wc >= 2, bias=i % 3 != 0, affine=i % 5 < 2,
                                        act=ACTS[(i // 2) % 6], wc=wc))
    return out


def conv_inputs(case, seed, n=CONV_N, cin=CONV_CIN, cout=CONV_COUT):
    """float32 (x, weight, bias, bn_scale, bn_shift) of a conv case; entries the case switches off are None."""
    rng = np.random.default_rng(seed)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    x, wt = f(n, cin, case["w"]), f(cout, cin // case["groups"], case["k"])
    b, sh = f(cout), f(cout)
    sc = ((0.5 + rng.random(cout)) * np.where(rng.random(cout) < 0.3, -1.0, 1.0)).astype(np.float32)  # some negative
    return (x, wt, b if case.get("bias", True) else None, sc if case.get("affine") else None,
            sh if case.get("affine") else None)


GROUPNORM_KV = ((1, 1), (1, 2), (3, 21), (1, 64), (5, 13), (1, 255), (4, 64), (1, 257), (5, 200))
GROUPNORM_N = (1, 3, 300)

AUTOCORR_V = (1, 2, 63, 64, 128, 129, 300)
AUTOCORR_K = (1, 5)
AUTOCORR_BIG_LDS = (40, 512)  # (K V + 2 V + 64) * 4 = 86 272 bytes > 64 KiB
AUTOCORR_TOO_BIG = (64, 1024)  # > 160 KiB

LAYERNORM_E = (1, 2, 63, 64, 65, 128, 200, 1000)
LAYERNORM_N = (1, 3, 4, 5, 1027)

ATTN_D = (1, 3, 16, 17, 20, 32, 33, 64, 65, 100, 128)
ATTN_HEADS = (1, 2, 3)
ATTN_T = (1, 15, 16, 17, 33, 65)
ATTN_NSEQ = (1, 3)

# ---- ofp_rnn_layer: one case per kernel instantiation that the host rules of csrc/ofp_rnn.hip can reach ---------
# k_rnn_layer<CELL, NT, WLDS, GX>: NT hidden tiles of 16 per wave (1, 2, or 4 -- a count of 3 runs as 4 with
# the last slot skipped), WLDS = W_hh resident in LDS (ofp_rnn_lds_bytes(cell, H) <= 160 KiB), GX = input
# projection precomputed by ofp_dense (more than 8 input features).
RNN_CELL_GATES = {"RNN_TANH": 1, "RNN_RELU": 1, "GRU": 3, "LSTM": 4}
RNN_CELL_CODES = {"RNN_TANH": 0, "RNN_RELU": 1, "GRU": 2, "LSTM": 3}  # OFP_CELL_*
RNN_LDS_MAX = 160 * 1024
RNN_B, RNN_T = 17, 5
RNN_F_INLINE, RNN_F_PROJECTED = 3, 12


def rnn_lds_bytes(cell, H):
    """What ofp_rnn_lds_bytes documents: h [2][16][st] and W_hh [G][kh][st] floats, kh = H rounded up to
    16, st = kh + 4."""
    kh = (H + 15) // 16 * 16
    return (32 * (kh + 4) + RNN_CELL_GATES[cell] * kh * (kh + 4)) * 4


def rnn_instantiation(cell, H, F):
    """(NT, WLDS, GX) that ofp_rnn_layer's dispatch picks."""
    tiles = (H + 15) // 16
    waves = min(tiles, 4)
    nt = -(-tiles // waves)
    return (nt if nt <= 2 else 4, rnn_lds_bytes(cell, H) <= RNN_LDS_MAX, F > 8)


def _rnn_rows(cell, rows):
    out = []
    for H, inst, note in rows:
        for F in (RNN_F_INLINE, RNN_F_PROJECTED):
            out.append((cell, H, F, inst + (F > 8,), note))
    return out


# (cell, H, F, (NT, WLDS, GX) the row is there for, what else it reaches); every row runs with F = 3
# (GX = False: inline input MFMA) and F = 12 (GX = True: projection read from the ofp_dense buffer)
RNN_TABLE = (
    _rnn_rows("RNN_TANH", [
        (1, (1, True), "one unit: 15 of 16 tile columns masked"),
        (100, (2, True), "7 tiles on 4 waves, the last wave's second slot is empty"),
        (176, (4, True), "11 tiles: 3 per wave runs as NT = 4, last slot skipped; largest resident W_hh"),
        (192, (4, False), "12 tiles: 3 per wave as NT = 4, first streamed size"),
        (256, (4, False), "16 tiles: all four slots of every wave; the largest H"),
    ])
    + [("RNN_TANH", 201, RNN_F_INLINE, (4, False, False), "streamed W_hh with H % 4 != 0: scalar tail of whh_global")]
    + _rnn_rows("RNN_RELU", [
        (1, (1, True), "one unit"),
        (100, (2, True), "7 tiles on 4 waves"),
        (176, (4, True), "11 tiles: NT = 4 with the last slot skipped"),
        (192, (4, False), "12 tiles, streamed"),
        (256, (4, False), "16 tiles, streamed"),
    ])
    + _rnn_rows("GRU", [
        (40, (1, True), "3 tiles on 3 waves, last tile partial"),
        (80, (2, True), "5 tiles: only wave 0 has a second tile"),
        (96, (2, True), "6 tiles: largest resident W_hh of a GRU"),
        (97, (2, False), "7 tiles, first streamed size, H % 4 != 0: scalar tail of whh_global"),
        (160, (4, False), "10 tiles: 3 per wave as NT = 4"),
        (256, (4, False), "16 tiles"),
    ])
    + _rnn_rows("LSTM", [
        (33, (1, True), "3 tiles on 3 waves, one unit in the last"),
        (80, (2, True), "5 tiles: largest resident W_hh of an LSTM"),
        (81, (2, False), "6 tiles, first streamed size, H % 4 != 0: scalar tail of whh_global"),
        (160, (4, False), "10 tiles: 3 per wave as NT = 4"),
        (256, (4, False), "16 tiles"),
    ])
)
# every second row runs both directions; these rows run without biases
RNN_NO_BIAS = {("RNN_TANH", 100, 3), ("RNN_RELU", 192, 12), ("GRU", 97, 12), ("GRU", 160, 3), ("LSTM", 81, 3),
               ("LSTM", 256, 12)}
# repeated with every parameter and the input multiplied by 3 (saturated gates), one per cell
RNN_SATURATED = (("RNN_TANH", 100, 3), ("RNN_RELU", 176, 12), ("GRU", 97, 3), ("LSTM", 80, 12))
