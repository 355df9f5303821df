"""float64 references of the directly tested training kernels (csrc/ofp_cnn_train.hip): the three gradients of a
stride-1 Conv1d, BatchNorm1d in training mode, forward and backward, and the Linear head with its loss, forward and
backward (with the shapes and inputs of its tests).  Written from the formulas; every result
comes with an element-wise bound on what a float32 kernel may lose, derived from the roundings it has to make, not
from what the kernels give.  u = 2^-24 is the unit roundoff of float32.

tests/test_cnn_train_cpu.py checks the values against torch autograd in float64."""
import numpy as np

U = 2.0 ** -24
f64 = np.float64


def conv1d_backward_ref(x, w, dz, padding, dilation, groups):
    """x [n, cin, win], w [cout, cin / groups, k], dz [n, cout, wc] -> {"dx", "dw", "db"}: (value, bound).
        dW[o][ci][k] = sum_{s,p} dz[s][o][p] x[s][g cin_g + ci][p - pad + k dil]      (n wc terms)
        db[o]        = sum_{s,p} dz[s][o][p]                                         (n wc terms)
        dx[s][ci][q] = sum_{o,k} dz[s][o][q + pad - k dil] W[o][ci][k]               (cout / groups * k terms)
    Bound of a sum of N products, in any order of summation: (N + 4) u sum |terms|."""
    x, w, dz = x.astype(f64), w.astype(f64), dz.astype(f64)
    n, cin, win = x.shape
    cout, cin_g, k = w.shape
    wc = dz.shape[2]
    assert wc == win + 2 * padding - dilation * (k - 1) and cin_g * groups == cin
    cout_g = cout // groups
    xp = np.zeros((n, cin, win + 2 * padding))
    xp[:, :, padding:padding + win] = x
    dw, dw_abs = np.zeros_like(w), np.zeros_like(w)
    dxp, dxp_abs = np.zeros_like(xp), np.zeros_like(xp)
    for g in range(groups):
        osl, isl = slice(g * cout_g, (g + 1) * cout_g), slice(g * cin_g, (g + 1) * cin_g)
        for kk in range(k):
            seg = slice(kk * dilation, kk * dilation + wc)
            dw[osl, :, kk] = np.einsum("sop,scp->oc", dz[:, osl], xp[:, isl, seg])
            dw_abs[osl, :, kk] = np.einsum("sop,scp->oc", np.abs(dz[:, osl]), np.abs(xp[:, isl, seg]))
            dxp[:, isl, seg] += np.einsum("sop,oc->scp", dz[:, osl], w[osl, :, kk])
            dxp_abs[:, isl, seg] += np.einsum("sop,oc->scp", np.abs(dz[:, osl]), np.abs(w[osl, :, kk]))
    crop = slice(padding, padding + win)
    db, db_abs = dz.sum((0, 2)), np.abs(dz).sum((0, 2))
    return {"dx": (dxp[:, :, crop], (cout_g * k + 4) * U * dxp_abs[:, :, crop]),
            "dw": (dw, (n * wc + 4) * U * dw_abs),
            "db": (db, (n * wc + 4) * U * db_abs)}


def _bn_stats(x, eps):
    count = x.shape[0] * x.shape[2]
    mean = x.mean((0, 2))
    var = ((x - mean[None, :, None]) ** 2).mean((0, 2))
    rstd = 1.0 / np.sqrt(var + eps)
    # the kernel sums x and x^2 in float64 and takes E[x^2] - mean^2: an absolute error of a few 2^-53 E[x^2] in
    # the variance, i.e. this relative error in rstd (2^-48 leaves room for the sums' own roundings)
    rel_rstd = 2.0 ** -48 * (x ** 2).mean((0, 2)) / (var + eps)
    return count, mean, var, rstd, rel_rstd


def batchnorm_train_forward_ref(x, gamma, beta, running_mean, running_var, eps, momentum):
    """x [n, C, w] -> {"y", "mean", "rstd", "running_mean", "running_var"}: (value, bound).  Batch statistics over the
    n w values of a channel, biased variance; the running variance takes the unbiased one, n w / (n w - 1).
    `momentum` is used as the float32 the kernel receives, and 1 - momentum as the float32 difference."""
    x, gamma, beta = x.astype(f64), gamma.astype(f64), beta.astype(f64)
    count, mean, var, rstd, rel = _bn_stats(x, eps)
    xc = x - mean[None, :, None]
    g, r = np.abs(gamma)[None, :, None], rstd[None, :, None]
    y = xc * r * gamma[None, :, None] + beta[None, :, None]
    b_mean = U * np.abs(mean) + 2.0 ** -50 * np.abs(x).mean((0, 2))
    b_rstd = rstd * (U + rel)
    # y = ((x - mean_f) * rstd_f) * gamma + beta in float32: the subtraction (1 rounding, and mean_f's own error),
    # two products (rstd_f carries 1 rounding more), the sum
    b_y = g * r * ((6 * U + rel[None, :, None]) * np.abs(xc) + 2 * U * np.abs(mean)[None, :, None]) + 2 * U * np.abs(y)
    mom = float(np.float32(momentum))
    keep = float(np.float32(1.0) - np.float32(momentum))
    unbiased = var * count / (count - 1)
    rm = mom * mean + keep * running_mean.astype(f64)
    rv = mom * unbiased + keep * running_var.astype(f64)
    b_rm = 4 * U * (np.abs(mom * mean) + np.abs(keep * running_mean)) + mom * b_mean
    b_rv = 4 * U * (np.abs(mom * unbiased) + np.abs(keep * running_var)) + mom * 2.0 ** -48 * (x ** 2).mean((0, 2)) * 2
    return {"y": (y, b_y), "mean": (mean, b_mean), "rstd": (rstd, b_rstd), "running_mean": (rm, b_rm),
            "running_var": (rv, b_rv)}


def batchnorm_train_backward_ref(x, gamma, dy, eps):
    """-> {"dx", "dgamma", "dbeta"}: (value, bound).  With xhat = (x - mean) rstd, s1 = sum dy, s2 = sum dy xhat:
    dbeta = s1, dgamma = s2, dx = (dy - s1 / N - xhat s2 / N) rstd gamma.  The kernel forms xhat in float32 from the
    rounded mean and rstd (error e_xh below), sums in float64, and evaluates dx in float32."""
    x, gamma, dy = x.astype(f64), gamma.astype(f64), dy.astype(f64)
    count, mean, var, rstd, rel = _bn_stats(x, eps)
    r, ga = rstd[None, :, None], gamma[None, :, None]
    xh = (x - mean[None, :, None]) * r
    s1, s2 = dy.sum((0, 2)), (dy * xh).sum((0, 2))
    e_xh = (3 * U + rel[None, :, None]) * np.abs(xh) + 2 * U * np.abs(mean)[None, :, None] * r
    b_dgamma = (np.abs(dy) * e_xh).sum((0, 2)) + U * np.abs(s2)
    b_dbeta = U * np.abs(s1) + 2.0 ** -50 * np.abs(dy).sum((0, 2))
    t2 = (s1 / count)[None, :, None] + 0 * xh
    t3 = xh * (s2 / count)[None, :, None]
    dx = (dy - t2 - t3) * r * ga
    inner = (3 * U * np.abs(t2) + e_xh * np.abs(s2 / count)[None, :, None]
             + np.abs(xh) * (b_dgamma / count)[None, :, None] + 3 * U * np.abs(t3)
             + 2 * U * (np.abs(dy) + np.abs(t2) + np.abs(t3)))
    b_dx = r * np.abs(ga) * inner + (3 * U + rel[None, :, None]) * np.abs(dx)
    return {"dx": (dx, b_dx), "dgamma": (s2, b_dgamma), "dbeta": (s1, b_dbeta)}


U53 = 2.0 ** -53


def _sum64(n_terms, abs_sum):
    """What an fp64 sum of n_terms exact terms may lose, in any order of summation."""
    return (n_terms + 4) * U53 * abs_sum


def _rounded(value, before):
    """Bound of a value computed to within `before` and then rounded to float32 once."""
    return before + U * (np.abs(value) + before)


def linear_head_ref(h, w, b, y, loss):
    """The Linear head with its loss: h [n, F], w [O, F], b [O], y [n, O], loss 0 = L1 / 1 = MSE ->
    {"out", "dy", "loss", "dw", "db", "dh"}: (value, bound).
        out[s][j] = b[j] + sum_f h[s][f] w[j][f]          fp64 sum of F + 1 exact terms, rounded once
        r         = out - y                               the rounded out, rounded once more
        dy        = sign(r) inv  |  (2 inv) r             inv the float32 1 / (float)(n O); 2 inv is exact
        loss      = mean |r|  |  mean r^2                 fp64 sum of n O terms, rounded once
        db[j]     = sum_s dy[s][j]                        fp64 sum of the float32 dy, rounded once
        dw[j][f]  = sum_s dy[s][j] h[s][f]                fp64 sum of exact products, rounded once
        dh[s][f]  = sum_j dy[s][j] w[j][f]                float32 fmaf chain of O terms: (O + 4) u sum |terms|
    Everything after `out` is computed from rounded values, so its bound also carries what those may be off by.  For
    L1 the sign is taken as exact: the caller keeps |out - y| clear of out's bound (l1_margin)."""
    h, w, b, y = (a.astype(f64) for a in (h, w, b, y))
    n, F = h.shape
    O = w.shape[0]
    inv = float(np.float32(1.0) / np.float32(n * O))
    out = h @ w.T + b
    out_abs = np.abs(h) @ np.abs(w).T + np.abs(b)
    b_out = _rounded(out, _sum64(F + 1, out_abs))
    r = out - y
    b_r = _rounded(r, b_out)
    if loss == 0:
        dy, b_dy = np.sign(r) * inv, np.zeros_like(r)
        terms, b_terms = np.abs(r), b_r
    else:
        dy = (2.0 * inv) * r
        b_dy = _rounded(dy, (2.0 * inv) * b_r)
        terms, b_terms = r * r, b_r * (2.0 * np.abs(r) + b_r)
    total = terms.sum()
    mean = np.array([total / (n * O)])
    b_mean = _rounded(mean, (b_terms.sum() + _sum64(n * O, total)) / (n * O) + 2 * U53 * mean)
    db = dy.sum(0)
    b_db = _rounded(db, b_dy.sum(0) + _sum64(n, np.abs(dy).sum(0)))
    dw = dy.T @ h
    b_dw = _rounded(dw, b_dy.T @ np.abs(h) + _sum64(n, np.abs(dy).T @ np.abs(h)))
    dh = dy @ w
    b_dh = b_dy @ np.abs(w) + (O + 4) * U * ((np.abs(dy) + b_dy) @ np.abs(w))
    return {"out": (out, b_out), "dy": (dy, b_dy), "loss": (mean, b_mean), "dw": (dw, b_dw), "db": (db, b_db),
            "dh": (dh, b_dh)}


def l1_margin(ref, y):
    """Smallest |out - y| / bound of out over the batch: the sign L1 takes is the exact one while this is far above 1."""
    out, b_out = ref["out"]
    return float(np.min(np.abs(out - y.astype(f64)) / b_out))


# (n, F, O) of the Linear head's direct tests: each axis in full with the others at a mid value, and four corners.
#   n  one chunk of 64 samples or two, a last chunk of one sample, the 256-thread stride of the loss kernel, the limit
#   F  the forward's stride of 256 features, the backward's grid over F
#   O  the odd tail of the loops that take two outputs at a time, the limit of 16
HEAD_N, HEAD_F, HEAD_O = (1, 63, 64, 65, 128, 129, 256, 257, 1024), (1, 255, 256, 257, 600), (1, 2, 3, 15, 16)
HEAD_MID = (65, 257, 3)
HEAD_SHAPES = sorted({(n, HEAD_MID[1], HEAD_MID[2]) for n in HEAD_N} | {(HEAD_MID[0], F, HEAD_MID[2]) for F in HEAD_F}
                     | {(HEAD_MID[0], HEAD_MID[1], O) for O in HEAD_O}
                     | {(1, 1, 1), (1024, 600, 16), (129, 257, 15), (257, 255, 1)})


def linear_head_inputs(n, F, O):
    """float32 h, w, b, y of one shape.  The weights are scaled so that out is of order 1; the targets lie 0.25 to 2
    away from the float64 out, on either side, so that no residual is near the kink of L1."""
    rng = np.random.default_rng([n, F, O])
    h = rng.standard_normal((n, F)).astype(np.float32)
    w = (rng.standard_normal((O, F)) / np.sqrt(F)).astype(np.float32)
    b = rng.standard_normal(O).astype(np.float32)
    out = h.astype(f64) @ w.astype(f64).T + b.astype(f64)
    y = (out + rng.choice([-1.0, 1.0], (n, O)) * rng.uniform(0.25, 2.0, (n, O))).astype(np.float32)
    return h, w, b, y


def nadam_step_ref(p, g, m, v, factors):
    """One torch.optim.NAdam step (defaults) in float64 from float32 state; factors = (c1, c2, bias_correction2) of
    model.cnn_step_factors.  -> (p', m', v', update): update = p' - p."""
    p, g, m, v = (a.astype(f64) for a in (p, g, m, v))
    c1, c2, bc2 = (float(f) for f in factors)
    m1 = m + (1 - 0.9) * (g - m)
    v1 = v * 0.999 + (1 - 0.999) * g * g
    denom = np.sqrt(v1 / bc2) + 1e-8
    upd = c1 * g / denom + c2 * m1 / denom
    return p + upd, m1, v1, upd
