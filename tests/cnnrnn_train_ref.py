"""float64 references of the directly tested kernels of the CNNRNN trainer (csrc/ofp_cnnrnn_train.hip), written from
the formulas: the general Linear backward (with an element-wise bound on what a float32 kernel may lose), the GRU in
training form, forward and back-propagation through time, self-attention with the mean over time, forward and backward
with a given dropout mask, and the site-3 mask of the random stream restated in numpy beside the sites of
tests/train_random_ref.py.  u = 2^-24 is the unit roundoff of float32.

tests/test_cnnrnn_train_cpu.py checks the values against torch autograd in float64."""
import numpy as np

from train_random_ref import scale, threshold, words

U = 2.0 ** -24
f64 = np.float64
SITE_ATTENTION = 3


def attention_dropout_mask(seed, epoch, n, heads, T, p):
    """float32 [n, heads, T, T], row-major element index into site 3: 0 where dropped (word < T), float32(1 / (1 - p))
    where kept."""
    w = words(seed, epoch, SITE_ATTENTION, n * heads * T * T)
    return np.where(w < np.uint32(threshold(p)), np.float32(0.0), scale(p)).astype(np.float32).reshape(n, heads, T, T)


def linear_backward_ref(x, w, dy):
    """y = x w^T + b: x [R, I], w [O, I], dy [R, O] -> {"dx", "dw", "db"}: (value, bound).
        dx[r][i] = sum_o dy[r][o] w[o][i]      (O terms)
        dw[o][i] = sum_r dy[r][o] x[r][i]      (R terms)
        db[o]    = sum_r dy[r][o]              (R terms)
    Bound of a sum of N products, in any order of summation: (N + 4) u sum |terms| (tests/cnn_train_ref.py)."""
    x, w, dy = x.astype(f64), w.astype(f64), dy.astype(f64)
    R, O = dy.shape
    return {"dx": (dy @ w, (O + 4) * U * (np.abs(dy) @ np.abs(w))),
            "dw": (dy.T @ x, (R + 4) * U * (np.abs(dy).T @ np.abs(x))),
            "db": (dy.sum(0), (R + 4) * U * np.abs(dy).sum(0))}


def _sigmoid(v):
    return 1.0 / (1.0 + np.exp(-v))


def gru_forward_ref(x, w_ih, w_hh, b_ih, b_hh):
    """x [n, T, F], gate order r, z, n, h_0 = 0: n_t = tanh(gx_n + r (W_hn h + b_hn)), h_t = (1 - z) n_t + z h_{t-1}.
    -> (out [n, T, H], gates [n, T, 4H] = r, z, n, W_hn h + b_hn)."""
    x, w_ih, w_hh, b_ih, b_hh = (a.astype(f64) for a in (x, w_ih, w_hh, b_ih, b_hh))
    n, T, _ = x.shape
    H = w_hh.shape[1]
    gx = x @ w_ih.T + b_ih
    h = np.zeros((n, H))
    out, gates = np.zeros((n, T, H)), np.zeros((n, T, 4 * H))
    for t in range(T):
        a = h @ w_hh.T + b_hh
        r = _sigmoid(gx[:, t, :H] + a[:, :H])
        z = _sigmoid(gx[:, t, H:2 * H] + a[:, H:2 * H])
        c = np.tanh(gx[:, t, 2 * H:] + r * a[:, 2 * H:])
        h = (1 - z) * c + z * h
        out[:, t] = h
        gates[:, t] = np.concatenate([r, z, c, a[:, 2 * H:]], 1)
    return out, gates


def gru_backward_ref(x, w_ih, w_hh, out, gates, dout):
    """Back-propagation through time from the forward's own out and gates: -> dx, dw_ih, dw_hh, db_ih, db_hh."""
    x, w_ih, w_hh, out, gates, dout = (a.astype(f64) for a in (x, w_ih, w_hh, out, gates, dout))
    n, T, _ = x.shape
    H = w_hh.shape[1]
    dgx, dgh, hprev = np.zeros((n, T, 3 * H)), np.zeros((n, T, 3 * H)), np.zeros((n, T, H))
    back = np.zeros((n, H))
    for t in range(T - 1, -1, -1):
        r, z, c, hn = (gates[:, t, k * H:(k + 1) * H] for k in range(4))
        hp = out[:, t - 1] if t > 0 else np.zeros((n, H))
        dh = dout[:, t] + back
        dc = dh * (1 - z) * (1 - c * c)
        dzp = dh * (hp - c) * z * (1 - z)
        drp = dc * hn * r * (1 - r)
        dgx[:, t] = np.concatenate([drp, dzp, dc], 1)
        dgh[:, t] = np.concatenate([drp, dzp, dc * r], 1)
        hprev[:, t] = hp
        back = dh * z + dgh[:, t] @ w_hh
    gx2, gh2, hp2, x2 = dgx.reshape(n * T, -1), dgh.reshape(n * T, -1), hprev.reshape(n * T, H), x.reshape(n * T, -1)
    return (gx2 @ w_ih).reshape(x.shape), gx2.T @ x2, gh2.T @ hp2, gx2.sum(0), gh2.sum(0)


def attention_mean_forward_ref(h, in_w, in_b, heads, mask=None):
    """h [n, T, E] -> (ctx [n, E], qkv [n, T, 3E], probs [n, heads, T, T]): softmax(q k^T / sqrt(d)) per head, the
    probabilities multiplied by `mask` [n, heads, T, T] (dropout: 0 or 1 / (1 - p)), times v, heads side by side, the
    mean over time; no out_proj."""
    h, in_w, in_b = h.astype(f64), in_w.astype(f64), in_b.astype(f64)
    n, T, E = h.shape
    d = E // heads
    qkv = h @ in_w.T + in_b
    q, k, v = (qkv[:, :, i * E:(i + 1) * E].reshape(n, T, heads, d).transpose(0, 2, 1, 3) for i in range(3))
    s = q @ k.transpose(0, 1, 3, 2) / np.sqrt(d)
    e = np.exp(s - s.max(-1, keepdims=True))
    probs = e / e.sum(-1, keepdims=True)
    pm = probs if mask is None else probs * mask.astype(f64)
    ctx = (pm @ v).transpose(0, 2, 1, 3).reshape(n, T, E).mean(1)
    return ctx, qkv, probs


def attention_mean_backward_ref(h, in_w, heads, qkv, probs, dctx, mask=None):
    """-> (dh [n, T, E], d in_w [3E, E], d in_b [3E]) from the forward's own qkv and probs."""
    h, in_w, qkv, probs, dctx = (a.astype(f64) for a in (h, in_w, qkv, probs, dctx))
    n, T, E = h.shape
    d = E // heads
    m = np.ones_like(probs) if mask is None else mask.astype(f64)
    q, k, v = (qkv[:, :, i * E:(i + 1) * E].reshape(n, T, heads, d).transpose(0, 2, 1, 3) for i in range(3))
    dc = np.broadcast_to((dctx / T).reshape(n, 1, heads, d).transpose(0, 2, 1, 3), (n, heads, T, d))  # at (pm @ v)
    dv = (probs * m).transpose(0, 1, 3, 2) @ dc
    dp = (dc @ v.transpose(0, 1, 3, 2)) * m
    ds = probs * (dp - (dp * probs).sum(-1, keepdims=True))
    dq = ds @ k / np.sqrt(d)
    dk = ds.transpose(0, 1, 3, 2) @ q / np.sqrt(d)
    dqkv = np.concatenate([a.transpose(0, 2, 1, 3).reshape(n, T, E) for a in (dq, dk, dv)], 2).reshape(n * T, 3 * E)
    return (dqkv @ in_w).reshape(n, T, E), dqkv.T @ h.reshape(n * T, E), dqkv.sum(0)
