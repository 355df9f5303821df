"""float64 references of the directly tested kernels of the RNN trainer (csrc/ofp_rnn_train.hip), written from the
formulas: LayerNorm forward and backward, the stacked GRU in training form with a dropout mask between the layers
(on tests/cnnrnn_train_ref.py's one-layer GRU), torch's NAdam step with coupled weight decay, and the site-4 mask of the
random stream restated in numpy beside the sites of tests/train_random_ref.py.

tests/test_rnn_train_cpu.py checks the values against torch autograd in float64."""
import numpy as np

from cnnrnn_train_ref import gru_backward_ref, gru_forward_ref
from train_random_ref import scale, threshold, words

f64 = np.float64
SITE_LAYER = 4


def layer_dropout_mask(seed, epoch, layers, n, T, H, p):
    """float32 [layers, n, T, H], row-major element index ((l n + s) T + t) H + j into site 4: 0 where dropped (word <
    T), float32(1 / (1 - p)) where kept.  `layers` counts the layers whose output is dropped: the stack's less one."""
    w = words(seed, epoch, SITE_LAYER, layers * n * T * H)
    return np.where(w < np.uint32(threshold(p)), np.float32(0.0), scale(p)).astype(np.float32).reshape(layers, n, T, H)


def layernorm_forward_ref(x, gamma, beta, eps):
    """x [R, E] -> (y, mean [R], rstd [R]): the biased variance about the mean, rstd = 1 / sqrt(var + eps)."""
    x, gamma, beta = (a.astype(f64) for a in (x, gamma, beta))
    mean = x.mean(1)
    d = x - mean[:, None]
    rstd = 1.0 / np.sqrt((d * d).mean(1) + eps)
    return d * rstd[:, None] * gamma + beta, mean, rstd


def layernorm_backward_ref(x, gamma, mean, rstd, dy):
    """From the statistics given: xhat = (x - mean) rstd, g = dy gamma, dx = rstd (g - mean_e g - xhat mean_e (g xhat)),
    dgamma = sum_r dy xhat, dbeta = sum_r dy.  -> (dx, dgamma, dbeta)."""
    x, gamma, mean, rstd, dy = (a.astype(f64) for a in (x, gamma, mean, rstd, dy))
    xh = (x - mean[:, None]) * rstd[:, None]
    g = dy * gamma
    dx = rstd[:, None] * (g - g.mean(1, keepdims=True) - xh * (g * xh).mean(1, keepdims=True))
    return dx, (dy * xh).sum(0), dy.sum(0)


def gru_stack_forward_ref(x, params, masks=None):
    """x [n, T, F]; params = [(w_ih, w_hh, b_ih, b_hh)] per layer; masks [L - 1, n, T, H] (or None) multiplies the
    output of every layer but the last before the next layer reads it.  -> (seqs [L, n, T, H], the outputs before the
    masks; gates [L, n, T, 4H])."""
    seqs, gates, inp = [], [], x.astype(f64)
    for l, par in enumerate(params):
        out, g = gru_forward_ref(inp, *par)
        seqs.append(out), gates.append(g)
        inp = out if masks is None or l == len(params) - 1 else out * masks[l].astype(f64)
    return np.stack(seqs), np.stack(gates)


def gru_stack_backward_ref(x, params, seqs, gates, dseq, masks=None):
    """dseq [n, T, H] at the last layer's output -> [(dw_ih, dw_hh, db_ih, db_hh)] per layer; layer l + 1's dx, times
    layer l's mask, is the gradient at layer l's output."""
    L = len(params)
    grads, d = [None] * L, dseq.astype(f64)
    for l in range(L - 1, -1, -1):
        if l == 0:
            inp = x.astype(f64)
        else:
            inp = seqs[l - 1].astype(f64) * (1.0 if masks is None else masks[l - 1].astype(f64))
        dx, dw_ih, dw_hh, db_ih, db_hh = gru_backward_ref(inp, params[l][0], params[l][1], seqs[l], gates[l], d)
        grads[l] = (dw_ih, dw_hh, db_ih, db_hh)
        if l > 0:
            d = dx * (1.0 if masks is None else masks[l - 1].astype(f64))
    return grads


def nadam_decay_step_ref(p, g, m, v, factors, weight_decay):
    """One torch.optim.NAdam step with weight_decay in float64 from float32 state (_single_tensor_nadam: grad =
    grad.add(param, alpha=weight_decay) before anything else); factors = (c1, c2, bias_correction2) of
    model.cnn_step_factors.  -> (p', m', v', update, the decayed gradient)."""
    p, g, m, v = (a.astype(f64) for a in (p, g, m, v))
    c1, c2, bc2 = (float(f) for f in factors)
    g = g + weight_decay * p
    m1 = m + (1 - 0.9) * (g - m)
    v1 = v * 0.999 + (1 - 0.999) * g * g
    denom = np.sqrt(v1 / bc2) + 1e-8
    upd = c1 * g / denom + c2 * m1 / denom
    return p + upd, m1, v1, upd, g
