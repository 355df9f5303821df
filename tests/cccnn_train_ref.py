"""float64 references of the four directly tested kernels of csrc/ofp_cccnn_train.hip: the three gradients of a strided
Conv1d, GroupNorm(1, K) in training mode (forward and backward, with the optional MaxPool1d(2, 2)), the backward of
the correlation head (auto-correlation + softmax + Linear) and the SGD step.  Written from the formulas; every result
comes with an element-wise bound on what a float32 kernel may lose, derived from the roundings it has to make, not
from what the kernels give.  u = 2^-24 is the unit roundoff of float32.  A sum of N products, in any order of
summation and with or without fused multiply-adds, is off by at most (N + 4) u sum |terms|.

tests/test_cccnn_train_cpu.py checks the values against torch autograd in float64, shows that a float32 emulation of
each kernel lies inside its bound and that a planted fault lies outside."""
import numpy as np

U = 2.0 ** -24
f64 = np.float64


def conv_width(w, k, padding, dilation, stride):
    return (w + 2 * padding - dilation * (k - 1) - 1) // stride + 1


def conv1d_backward_strided_ref(x, w, dz, padding, dilation, groups, stride):
    """x [n, cin, win], w [cout, cin / groups, k], dz [n, cout, wc] -> {"dx", "dw", "db"}: (value, bound).
        dW[o][ci][k] = sum_{s,p} dz[s][o][p] x[s][g cin_g + ci][p stride - pad + k dil]      (n wc terms)
        db[o]        = sum_{s,p} dz[s][o][p]                                                (n wc terms)
        dx[s][ci][q] = sum_{o,k : p stride = q + pad - k dil} dz[s][o][p] W[o][ci][k]       (at most cout / groups * k)"""
    x, w, dz = x.astype(f64), w.astype(f64), dz.astype(f64)
    n, cin, win = x.shape
    cout, cin_g, k = w.shape
    wc = dz.shape[2]
    assert wc == conv_width(win, k, padding, dilation, stride) and cin_g * groups == cin
    cout_g = cout // groups
    # columns the taps may touch: the padded input, and never fewer than the last tap of the last output needs
    xp = np.zeros((n, cin, max(win + 2 * padding, (wc - 1) * stride + dilation * (k - 1) + 1)))
    xp[:, :, padding:padding + win] = x
    dw, dw_abs = np.zeros_like(w), np.zeros_like(w)
    dxp, dxp_abs = np.zeros_like(xp), np.zeros_like(xp)
    for g in range(groups):
        osl, isl = slice(g * cout_g, (g + 1) * cout_g), slice(g * cin_g, (g + 1) * cin_g)
        for kk in range(k):
            seg = slice(kk * dilation, kk * dilation + (wc - 1) * stride + 1, stride)
            dw[osl, :, kk] = np.einsum("sop,scp->oc", dz[:, osl], xp[:, isl, seg])
            dw_abs[osl, :, kk] = np.einsum("sop,scp->oc", np.abs(dz[:, osl]), np.abs(xp[:, isl, seg]))
            dxp[:, isl, seg] += np.einsum("sop,oc->scp", dz[:, osl], w[osl, :, kk])
            dxp_abs[:, isl, seg] += np.einsum("sop,oc->scp", np.abs(dz[:, osl]), np.abs(w[osl, :, kk]))
    crop = slice(padding, padding + win)
    db, db_abs = dz.sum((0, 2)), np.abs(dz).sum((0, 2))
    return {"dx": (dxp[:, :, crop], (cout_g * k + 4) * U * dxp_abs[:, :, crop]),
            "dw": (dw, (n * wc + 4) * U * dw_abs),
            "db": (db, (n * wc + 4) * U * db_abs)}


# The weight-gradient kernel gives the T = cin / groups * k + 1 outputs of a channel (its weights and its bias) g lanes
# each: g = 64 for T <= 4, halved at every doubling of T down to 1 above 128, and a second pass over the outputs above
# 256.  These cases sit on both sides of every change; 128 itself cannot be had (127 is prime and above the limits
# of k and of the channels), 127 stands in for it.  cout = 2, n * wc is no multiple of 64 and lies inside one slab of
# 2048 pairs, except in the last two, which span two slabs with g = 4 and g = 2.
# (k, stride, dilation, padding, groups, cin, cout, width, n)
WGRAD_LANE_CASES = [
    (3, 1, 1, 1, 1, 1, 2, 37, 5), (4, 2, 1, 1, 1, 1, 2, 41, 5),      # T = 4, 5
    (7, 1, 1, 3, 1, 1, 2, 33, 7), (4, 1, 1, 0, 2, 4, 2, 30, 5),      # T = 8, 9
    (5, 1, 1, 2, 1, 3, 2, 29, 5), (8, 1, 1, 0, 1, 2, 2, 40, 3),      # T = 16, 17
    (31, 1, 1, 15, 1, 1, 2, 35, 3), (16, 1, 1, 0, 2, 4, 2, 50, 3),   # T = 32, 33
    (21, 1, 1, 10, 1, 3, 2, 45, 3), (64, 1, 1, 0, 1, 1, 2, 100, 3),  # T = 64, 65
    (63, 1, 1, 31, 1, 2, 2, 50, 3), (64, 1, 1, 0, 1, 2, 2, 90, 3),   # T = 127, 129
    (51, 1, 1, 25, 1, 5, 2, 30, 3), (64, 2, 1, 0, 1, 4, 2, 101, 3),  # T = 256, 257
    (21, 1, 1, 10, 1, 3, 2, 45, 47), (63, 1, 1, 31, 2, 4, 2, 50, 43),  # T = 64, 127 over two slabs
]


def _gn_stats(x, eps):
    """Per item: element count, mean, biased variance, rstd and the relative error of an rstd formed from float64 sums
    of x and x^2 as E[x^2] - mean^2 (a few 2^-53 E[x^2] in the variance; 2^-48 leaves room for the sums' own
    roundings)."""
    count = x.shape[1] * x.shape[2]
    mean = x.mean((1, 2))
    var = ((x - mean[:, None, None]) ** 2).mean((1, 2))
    rstd = 1.0 / np.sqrt(var + eps)
    rel_rstd = 2.0 ** -48 * (x ** 2).mean((1, 2)) / (var + eps)
    return count, mean, var, rstd, rel_rstd


def _pool(y):
    """MaxPool1d(2, 2) of [n, K, V] -> (pooled, take): take [n, K, V] is 1 where the pooled value came from (the first
    of a pair on a tie; an odd last column is dropped)."""
    n, K, V = y.shape
    Vo = V // 2
    a, b = y[:, :, 0:2 * Vo:2], y[:, :, 1:2 * Vo:2]
    second = b > a
    take = np.zeros(y.shape, bool)
    take[:, :, 0:2 * Vo:2] = ~second
    take[:, :, 1:2 * Vo:2] = second
    return np.where(second, b, a), take


def _unpool(dy, take):
    """Route dy [n, K, V // 2] back to [n, K, V] along `take`."""
    V = take.shape[2]
    Vo = V // 2
    full = np.zeros(take.shape)
    full[:, :, 0:2 * Vo:2] = dy
    full[:, :, 1:2 * Vo:2] = dy
    return full * take


def groupnorm1_train_forward_ref(x, gamma, beta, eps, pool=False):
    """x [n, K, V] -> {"y", "mean", "rstd"}: (value, bound).  Statistics over the K V values of an item, biased
    variance; y = ((x - mean_f) * rstd_f) * gamma + beta in float32, then the larger of every pair when pooled (the
    error of a maximum is at most the larger of the two errors)."""
    x, gamma, beta = x.astype(f64), gamma.astype(f64), beta.astype(f64)
    _count, mean, _var, rstd, rel = _gn_stats(x, eps)
    xc = x - mean[:, None, None]
    g, r = np.abs(gamma)[None, :, None], rstd[:, None, None]
    y = xc * r * gamma[None, :, None] + beta[None, :, None]
    b_mean = U * np.abs(mean) + 2.0 ** -50 * np.abs(x).mean((1, 2))
    b_rstd = rstd * (U + rel)
    # the subtraction (1 rounding, and mean_f's own error), two products (rstd_f carries 1 rounding more), the sum
    b_y = g * r * ((6 * U + rel[:, None, None]) * np.abs(xc) + 2 * U * np.abs(mean)[:, None, None]) + 2 * U * np.abs(y)
    if pool:
        Vo = x.shape[2] // 2
        y, _take = _pool(y)
        b_y = np.maximum(b_y[:, :, 0:2 * Vo:2], b_y[:, :, 1:2 * Vo:2])
    return {"y": (y, b_y), "mean": (mean, b_mean), "rstd": (rstd, b_rstd)}


def groupnorm1_train_backward_ref(x, gamma, beta, dy, eps, pool=False):
    """-> {"dx", "dgamma", "dbeta"}: (value, bound).  dy is shaped like the forward's y and first routed through the
    pool.  Per item with N = K V, xhat = (x - mean) rstd, dhat = dy gamma: s1 = sum dhat, s2 = sum dhat xhat,
    dx = (dhat - s1 / N - xhat s2 / N) rstd; over items and positions dgamma_k = sum dy xhat, dbeta_k = sum dy.
    The kernel forms xhat and dhat in float32 from the rounded mean and rstd (errors e_xh, u |dhat|), sums in
    float64, rounds s1 / N and s2 / N once and evaluates dx in float32."""
    x, gamma, beta, dy = x.astype(f64), gamma.astype(f64), beta.astype(f64), dy.astype(f64)
    count, mean, _var, rstd, rel = _gn_stats(x, eps)
    r, ga = rstd[:, None, None], gamma[None, :, None]
    xh = (x - mean[:, None, None]) * r
    if pool:
        _y, take = _pool(xh * ga + beta[None, :, None])
        dy = _unpool(dy, take)
    dh = dy * ga
    s1, s2 = dh.sum((1, 2)), (dh * xh).sum((1, 2))
    e_xh = (3 * U + rel[:, None, None]) * np.abs(xh) + 2 * U * np.abs(mean)[:, None, None] * r
    dgamma, dbeta = (dy * xh).sum((0, 2)), dy.sum((0, 2))
    b_dgamma = (np.abs(dy) * e_xh).sum((0, 2)) + U * np.abs(dgamma) + 2.0 ** -50 * (np.abs(dy) * np.abs(xh)).sum((0, 2))
    b_dbeta = U * np.abs(dbeta) + 2.0 ** -50 * np.abs(dy).sum((0, 2))
    b_s1 = U * np.abs(dh).sum((1, 2))
    b_s2 = (np.abs(dh) * (e_xh + U * np.abs(xh))).sum((1, 2))
    t2 = (s1 / count)[:, None, None] + 0 * xh
    t3 = xh * (s2 / count)[:, None, None]
    dx = (dh - t2 - t3) * r
    inner = (U * np.abs(dh) + (b_s1 / count)[:, None, None] + U * np.abs(t2)
             + e_xh * np.abs(s2 / count)[:, None, None] + np.abs(xh) * (b_s2 / count)[:, None, None] + 2 * U * np.abs(t3)
             + 2 * U * (np.abs(dh) + np.abs(t2) + np.abs(t3)))
    b_dx = r * inner + (3 * U + rel[:, None, None]) * np.abs(dx)
    return {"dx": (dx, b_dx), "dgamma": (dgamma, b_dgamma), "dbeta": (dbeta, b_dbeta)}


def autocorr_softmax_f64(f):
    """f [items, K, V] -> (cc, p) float64 [items, 2V - 1]: cc[j] = sum_k sum_i f_k[i + j - (V - 1)] f_k[i]."""
    f = f.astype(f64)
    items, K, V = f.shape
    cc = np.zeros((items, 2 * V - 1))
    for j in range(2 * V - 1):
        sh = j - (V - 1)
        lo, hi = max(0, -sh), min(V, V - sh)
        cc[:, j] = (f[:, :, lo + sh:hi + sh] * f[:, :, lo:hi]).sum((1, 2))
    e = np.exp(cc - cc.max(1, keepdims=True))
    return cc, e / e.sum(1, keepdims=True)


def autocorr_softmax_backward_ref(f, dout, wfc, channels, e_p=None):
    """Backward of out = fc(flatten(p over the sensors)), p = softmax(cc(f)): f [items, K, V] with items = n *
    channels (sensor fastest), dout [n, O], wfc [O, channels * L], L = 2V - 1 -> (df, bound) [items, K, V].
        dp[j]  = sum_o dout[b][o] wfc[o][c L + j]            fmaf chain of O terms
        dot    = sum_j p[j] dp[j]                            float64 sum, rounded once
        dcc[j] = p[j] (dp[j] - dot)                          2 roundings
        g[s]   = dcc[V-1+s] + dcc[V-1-s]                     1 rounding (the lag 0 carries 2 dcc[V-1])
        df_k[m] = sum_i g[i - m] f_k[i]                      fmaf chain of V terms
    e_p [items, L]: the error of the p handed to the kernel (default: p rounded to float32)."""
    f, dout, wfc = f.astype(f64), dout.astype(f64), wfc.astype(f64)
    items, K, V = f.shape
    L, O = 2 * V - 1, dout.shape[1]
    n = items // channels
    assert items == n * channels and wfc.shape == (O, channels * L) and dout.shape[0] == n
    _cc, p = autocorr_softmax_f64(f)
    e_p = U * p if e_p is None else e_p
    w3 = wfc.reshape(O, channels, L)
    dp = np.einsum("bo,ocj->bcj", dout, w3).reshape(items, L)
    e_dp = (O + 4) * U * np.einsum("bo,ocj->bcj", np.abs(dout), np.abs(w3)).reshape(items, L)
    dot = (p * dp).sum(1, keepdims=True)
    e_dot = ((e_p * np.abs(dp) + (p + e_p) * e_dp).sum(1, keepdims=True) + U * np.abs(dot)
             + 2.0 ** -48 * (p * np.abs(dp)).sum(1, keepdims=True))
    diff = dp - dot
    dcc = p * diff
    e_dcc = e_p * np.abs(diff) + (p + e_p) * (e_dp + e_dot + U * np.abs(diff)) + U * np.abs(dcc)
    g = dcc + dcc[:, ::-1]
    e_g = e_dcc + e_dcc[:, ::-1] + U * np.abs(g)
    df, bound = np.zeros_like(f), np.zeros_like(f)
    for m in range(V):  # g index of lag s = i - m is s + V - 1
        gm, em = g[:, V - 1 - m:2 * V - 1 - m], e_g[:, V - 1 - m:2 * V - 1 - m]
        df[:, :, m] = np.einsum("ni,nki->nk", gm, f)
        bound[:, :, m] = np.einsum("ni,nki->nk", em + (V + 4) * U * np.abs(gm), np.abs(f))
    return df, bound


def sgd_step_ref(p, g, buf, lr, first, momentum, weight_decay):
    """One torch.optim.SGD step (dampening 0, no Nesterov) in float64 from float32 state: g' = g + wd p, buf' = g' on
    the first step and momentum buf + g' after it, p' = p - lr buf'.  momentum, weight_decay and lr are used as given
    (hand in the float32 values the kernel receives).  -> {"p", "buf"}: (value, bound); every product and every sum
    is one rounding.  At lr = 0 the bound on p' is 0: the parameter must not change."""
    p, g, buf = (a.astype(f64) for a in (p, g, buf))
    lr, momentum, weight_decay = float(lr), float(momentum), float(weight_decay)
    gr = g + weight_decay * p
    e_gr = U * np.abs(weight_decay * p) + U * np.abs(gr)
    if first:
        b1, e_b = gr, e_gr
    else:
        b1 = momentum * buf + gr
        e_b = e_gr + U * np.abs(momentum * buf) + U * np.abs(b1)
    p1 = p - lr * b1
    e_p = abs(lr) * e_b + U * np.abs(lr * b1) + (U * np.abs(p1) if lr != 0 else 0.0)
    return {"p": (p1, e_p), "buf": (b1, e_b)}
