"""The classifiers of the reference's ``model.py`` with their forward passes on MI355X.

``CNN`` (model.py:52-120), ``CCCNN`` / ``LCCCNN`` (:443-580), ``RNN`` (:168-307) and ``CNNRNN``
(:310-440) take the same constructor arguments and use the same parameter names as the reference,
so its ``state_dict`` loads unchanged.  ``forward`` is inference-only (eval semantics: dropout off,
BatchNorm on its running statistics) and runs as HIP kernels (csrc/ofp_nn.hip, csrc/ofp_xcorr.hip,
csrc/ofp_rnn.hip); torch only allocates memory and makes views.  ``rnn_forward`` runs a torch
``nn.GRU`` / ``nn.LSTM`` / ``nn.RNN`` module (its full output sequence) on the same kernels.
Lightning training steps and optimisers are out of scope.
"""
import ctypes

import torch
from torch import nn
from torch.nn import functional as F

from . import _lib
from ._lib import check
from .calibration import ACT_CODES, dense_forward


def _stream(dev):
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def conv1d_forward(x, weight, bias, padding, dilation, act_code, groups=1, bn=None, pool=False, stride=1):
    """Conv1d + bias + activation (+ eval-mode BatchNorm1d `bn` + MaxPool1d(2, 2)): the layer of
    model.py:91-107 in one kernel."""
    L = _lib.lib()
    n, cin, w = x.shape
    cout, _, k = weight.shape
    wout = (w + 2 * padding - dilation * (k - 1) - 1) // stride + 1
    if pool:
        wout //= 2
    scale = shift = None
    if bn is not None:  # y = (v - mean) / sqrt(var + eps) * gamma + beta, folded in double
        inv = (bn.running_var.double() + bn.eps).rsqrt()
        g = bn.weight.double() if bn.weight is not None else torch.ones_like(inv)
        b = bn.bias.double() if bn.bias is not None else torch.zeros_like(inv)
        scale = (g * inv).to(x.device, torch.float32).contiguous()
        shift = (b - bn.running_mean.double() * g * inv).to(x.device, torch.float32).contiguous()
    out = torch.empty((n, cout, wout), dtype=torch.float32, device=x.device)
    check(L.ofp_conv1d(x.data_ptr(), n, cin, w, weight.data_ptr(), bias.data_ptr() if bias is not None else None,
                       cout, k, padding, dilation, groups, stride, act_code,
                       scale.data_ptr() if scale is not None else None,
                       shift.data_ptr() if shift is not None else None, int(bool(pool)), out.data_ptr(),
                       _stream(x.device)), "ofp_conv1d")
    return out


def groupnorm1_forward(x, gn, pool=False):
    """nn.GroupNorm(1, K) (+ MaxPool1d(2, 2)) on x float32 CUDA [n, K, V]."""
    assert gn.num_groups == 1
    L = _lib.lib()
    n, K, V = x.shape
    out = torch.empty((n, K, V // 2 if pool else V), dtype=torch.float32, device=x.device)
    g = gn.weight.detach().to(x.device, torch.float32).contiguous() if gn.weight is not None else None
    b = gn.bias.detach().to(x.device, torch.float32).contiguous() if gn.bias is not None else None
    check(L.ofp_groupnorm1(x.data_ptr(), n, K, V, g.data_ptr() if g is not None else None,
                           b.data_ptr() if b is not None else None, float(gn.eps), int(bool(pool)), out.data_ptr(),
                           _stream(x.device)), "ofp_groupnorm1")
    return out


def _run_conv_stack(layers, h, to, padding, dilation, act_code, groups):
    mods = list(layers)
    i = 0
    while i < len(mods):
        m = mods[i]
        if isinstance(m, nn.Conv1d):
            bn, gn, pool, j = None, None, False, i + 1
            while j < len(mods) and not isinstance(mods[j], nn.Conv1d):
                if isinstance(mods[j], nn.BatchNorm1d):
                    bn = mods[j]
                elif isinstance(mods[j], nn.GroupNorm):
                    gn = mods[j]
                elif isinstance(mods[j], nn.MaxPool1d):
                    pool = True
                j += 1
            # conv + bias + activation (+ folded BatchNorm + pool) in one kernel; a GroupNorm needs the
            # whole item first, so it (and the pool after it) runs as a second kernel
            h = conv1d_forward(h, to(m.weight), to(m.bias) if m.bias is not None else None, padding, dilation,
                               act_code, groups=groups, bn=bn, pool=pool and gn is None, stride=m.stride[0])
            if gn is not None:
                h = groupnorm1_forward(h, gn, pool=pool)
            i = j
        else:
            i += 1
    return h


class CNN(nn.Module):
    def __init__(self, input_size: int, output_size: int, channels: int = 3, layer_sizes=[8, 16],
                 kernel_size: int = 3, dropout_rate: float = 0.5, loss=F.l1_loss, batch_norm=False, pool=False,
                 padding=1, dilation=1, groups=1, lr=1e-3, activation=nn.SiLU) -> None:
        super().__init__()
        if activation not in ACT_CODES:
            raise ValueError(f"activation {activation} has no HIP implementation")
        self._act_code = ACT_CODES[activation]
        self._padding, self._dilation, self._groups = padding, dilation, groups
        self.conv_layers = nn.Sequential()
        cur, width = channels, input_size
        for i, size in enumerate(layer_sizes):
            self.conv_layers.add_module(
                f"conv{i+1}", nn.Conv1d(cur, size, kernel_size, padding=padding, dilation=dilation, groups=groups))
            self.conv_layers.add_module(f"act{i+1}", activation())
            width = width + 2 * padding - dilation * (kernel_size - 1)
            if batch_norm:
                self.conv_layers.add_module(f"bn{i+1}", nn.BatchNorm1d(size))
            if pool:
                self.conv_layers.add_module(f"pool{i+1}", nn.MaxPool1d(kernel_size=2, stride=2))
                width //= 2
            cur = size
        self.dropout = nn.Dropout(dropout_rate)
        self.fc = nn.Linear(cur * width, output_size)
        self.loss = loss
        self.lr = lr

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """x [batch, channels, input_size] -> [batch, output_size] (eval-mode semantics)."""
        dev = x.device if x.is_cuda else torch.device("cuda", 0)
        _lib.require_gpu(dev.index or 0)
        to = lambda t: t.detach().to(dev, torch.float32).contiguous()
        h = _run_conv_stack(self.conv_layers, to(x), to, self._padding, self._dilation, self._act_code, self._groups)
        h = h.reshape(h.shape[0], -1)
        h = dense_forward(h, to(self.fc.weight), to(self.fc.bias), None, None, 0)
        return h if x.is_cuda else h.cpu()


def paired_xcorr(x: torch.Tensor, C: int, K: int) -> torch.Tensor:
    """model.py:12-45: cross-correlate every adjacent channel pair (1&2, 2&3, ...) in each feature
    map and average over the maps: (B, C*K, V) -> (B, C-1, 2V-1)."""
    B, CK, V = x.shape
    assert CK == C * K
    dev = x.device if x.is_cuda else torch.device("cuda", 0)
    _lib.require_gpu(dev.index or 0)
    xd = x.detach().to(dev, torch.float32).contiguous().view(B, C, K, V)
    out = torch.empty((B, C - 1, 2 * V - 1), dtype=torch.float32, device=dev)
    L = _lib.lib()
    for bi in range(B):  # rows (c, k) of a sample are contiguous: a = channels 0..C-2, b = channels 1..C-1
        a, b = xd[bi, :-1], xd[bi, 1:]
        check(L.ofp_xcorr_full(a.data_ptr(), b.data_ptr(), (C - 1) * K, V, V, V, K, out[bi].data_ptr(),
                               _stream(dev)), "ofp_xcorr_full")
    return out if x.is_cuda else out.cpu()


def autocorr_softmax(feat):
    """feat float32 CUDA [n, K, V] -> [n, 2V-1]: the correlation head of CCCNN (model.py:524-534)."""
    L = _lib.lib()
    n, K, V = feat.shape
    out = torch.empty((n, 2 * V - 1), dtype=torch.float32, device=feat.device)
    check(L.ofp_autocorr_softmax(feat.data_ptr(), n, K, V, out.data_ptr(), _stream(feat.device)),
          "ofp_autocorr_softmax")
    return out


class CCCNN(nn.Module):
    """``model.CCCNN`` (model.py:443-538): a conv stack applied to every sensor channel (shared, or one
    private stack per channel with ``group=True``), optional MaxPool, the auto-correlation of every feature map summed
    over the maps, a softmax over the lags, and a Linear on the flattened result.  Same
    constructor arguments and parameter names (``conv_layers.conv{i}``, ``fc``) as the
    reference; ``forward`` is inference-only and runs as HIP kernels."""

    def __init__(self, input_size: int, output_size: int, channels: int = 3, layer_sizes=[8, 16],
                 kernel_sizes=3, strides=1, dropout_rate: float = 0.5, batch_norm=False, pool=False, padding=1,
                 dilation=1, group: bool = False, activation=nn.SiLU) -> None:
        super().__init__()
        if isinstance(kernel_sizes, int):
            kernel_sizes = [kernel_sizes] * len(layer_sizes)
        if isinstance(strides, int):
            strides = [strides] * len(layer_sizes)
        if activation not in ACT_CODES:
            raise ValueError(f"activation {activation} has no HIP implementation")
        self.group, self.channels = group, channels
        self._act_code, self._padding, self._dilation = ACT_CODES[activation], padding, dilation
        self.conv_layers = nn.Sequential()
        g = channels if group else 1  # model.py:466,484: one private stack per sensor channel when grouped
        cur, width = g, input_size
        for i, (size, k, stride) in enumerate(zip(layer_sizes, kernel_sizes, strides)):
            self.conv_layers.add_module(
                f"conv{i+1}", nn.Conv1d(cur, size * g, k, padding=padding, dilation=dilation, stride=stride, groups=g))
            self.conv_layers.add_module(f"act{i+1}", activation())
            width = (width + 2 * padding - dilation * (k - 1) - 1) // stride + 1
            if batch_norm:  # model.py:497-501: a GroupNorm with one group, despite the argument's name
                self.conv_layers.add_module(f"bn{i+1}", nn.GroupNorm(1, size * g))
            if pool:
                self.conv_layers.add_module(f"pool{i+1}", nn.MaxPool1d(kernel_size=2, stride=2))
                width //= 2
            cur = size * g
        self.dropout = nn.Dropout(dropout_rate)
        self.fc = nn.Linear(channels * (2 * width - 1), output_size)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """x [batch, channels, input_size] -> [batch, output_size] (eval-mode semantics)."""
        dev = x.device if x.is_cuda else torch.device("cuda", 0)
        _lib.require_gpu(dev.index or 0)
        to = lambda t: t.detach().to(dev, torch.float32).contiguous()
        B, C, W = x.shape
        if self.group:  # grouped conv: [B, C*K, V], channel-major, i.e. already [B*C, K, V]
            h = _run_conv_stack(self.conv_layers, to(x), to, self._padding, self._dilation, self._act_code, C)
            h = h.reshape(B * C, h.shape[1] // C, h.shape[2])
        else:  # the shared stack sees every sensor channel as its own item
            h = _run_conv_stack(self.conv_layers, to(x).reshape(B * C, 1, W), to, self._padding, self._dilation,
                                self._act_code, 1)
        probs = autocorr_softmax(h)  # [B*C, 2V-1]
        out = dense_forward(probs.reshape(B, -1), to(self.fc.weight), to(self.fc.bias), None, None, 0)
        return out if x.is_cuda else out.cpu()


class LCCCNN(nn.Module):
    """``model.LCCCNN`` (model.py:541-580): the training wrapper around CCCNN; inference only here.
    Parameter names (``model.conv_layers.conv{i}``, ``model.fc``) follow the reference."""

    def __init__(self, input_size: int, output_size: int, channels: int = 3, layer_sizes=[8, 16], kernel_sizes=3,
                 strides=1, dropout_rate: float = 0.5, batch_norm=False, pool=False, padding=1, dilation=1,
                 group: bool = False, activation=nn.SiLU, loss=F.l1_loss, lr=1e-3) -> None:
        super().__init__()
        self.model = CCCNN(input_size, output_size, channels, layer_sizes, kernel_sizes, strides, dropout_rate,
                           batch_norm, pool, padding, dilation, group, activation)
        self.lr = lr
        self.loss = loss

    def forward(self, x):
        return self.model(x)


# ---- recurrent models (model.py:168-440) ---------------------------------------------------------------------------
CELL_GATES = {0: 1, 1: 1, 2: 3, 3: 4}  # OFP_CELL_RNN_TANH, _RNN_RELU, _GRU, _LSTM (include/onsetfp.h)
RNN_MAX_HIDDEN = 256  # ofp_rnn_layer
RNN_MAX_INLINE = 8  # wider inputs are projected with ofp_dense before the recurrence
ATTN_MAX_HEAD_DIM = 128  # ofp_attention_mean


def _cell_code(rnn):
    if isinstance(rnn, nn.LSTM):
        if rnn.proj_size:
            raise ValueError("nn.LSTM with proj_size has no HIP implementation")
        return 3
    if isinstance(rnn, nn.GRU):
        return 2
    if isinstance(rnn, nn.RNN):
        if rnn.nonlinearity not in ("tanh", "relu"):
            raise ValueError(f"nn.RNN nonlinearity {rnn.nonlinearity!r} has no HIP implementation")
        return 0 if rnn.nonlinearity == "tanh" else 1
    raise ValueError(f"{type(rnn).__name__} is not an nn.GRU, nn.LSTM or nn.RNN")


def _check_rnn(rnn):
    _cell_code(rnn)
    if rnn.hidden_size > RNN_MAX_HIDDEN:
        raise ValueError(f"hidden_size {rnn.hidden_size} > {RNN_MAX_HIDDEN} has no HIP implementation")


def _rnn_into(rnn, xt, y, to):
    """Run every layer and direction of `rnn` over xt (a float32 CUDA view [n_seq, T, features], any strides) and
    write the last layer's output into y (a CUDA view [n_seq, T, dirs * H] with unit feature stride)."""
    L = _lib.lib()
    cell = _cell_code(rnn)
    G, H = CELL_GATES[cell], rnn.hidden_size
    dirs = 2 if rnn.bidirectional else 1
    n_seq, T, _ = xt.shape
    dev = xt.device
    assert y.stride(2) == 1 and tuple(y.shape) == (n_seq, T, dirs * H)
    src = xt
    for layer in range(rnn.num_layers):
        dst = y if layer == rnn.num_layers - 1 else torch.empty((n_seq, T, dirs * H), dtype=torch.float32, device=dev)
        fin = src.shape[2]
        rows = None
        if fin > RNN_MAX_INLINE:  # wide input: x W_ihᵀ + b_ih for every (sequence, step) as one dense layer
            if not (src.is_contiguous() or src.transpose(0, 1).is_contiguous()):
                src = src.contiguous()
            rows = src if src.is_contiguous() else src.transpose(0, 1)
            rows = rows.reshape(-1, fin)
        for d in range(dirs):
            sfx = f"_l{layer}" + ("_reverse" if d else "")
            w_ih, w_hh = to(getattr(rnn, "weight_ih" + sfx)), to(getattr(rnn, "weight_hh" + sfx))
            b_ih = to(getattr(rnn, "bias_ih" + sfx)) if rnn.bias else None
            b_hh = to(getattr(rnn, "bias_hh" + sfx)) if rnn.bias else None
            gx, gs = None, (0, 0)
            if rows is not None:
                gx = dense_forward(rows, w_ih, b_ih, None, None, 0)
                gs = (src.stride(0) // fin * G * H, src.stride(1) // fin * G * H)
            p = lambda t: t.data_ptr() if t is not None else None
            check(L.ofp_rnn_layer(cell, n_seq, T, fin, H, d, src.data_ptr(), *src.stride(), p(gx), *gs, w_ih.data_ptr(),
                                  p(b_ih), w_hh.data_ptr(), p(b_hh), dst.data_ptr(), dst.stride(0), dst.stride(1),
                                  d * H, _stream(dev)), "ofp_rnn_layer")
        src = dst
    return y


def rnn_forward(rnn_module, x):
    """``rnn_module(x)[0]`` -- the full output sequence of a torch nn.GRU / nn.LSTM / nn.RNN with zero initial
    state, eval semantics -- on the HIP recurrent kernel.  x: [batch, T, features] (batch_first) or [T, batch,
    features], or unbatched [T, features]; CPU in, CPU out."""
    _check_rnn(rnn_module)
    dev = x.device if x.is_cuda else torch.device("cuda", 0)
    _lib.require_gpu(dev.index or 0)
    to = lambda t: t.detach().to(dev, torch.float32).contiguous()
    xd = x.detach().to(dev, torch.float32)
    if xd.dim() == 2:
        return rnn_forward(rnn_module, x.unsqueeze(1 if not rnn_module.batch_first else 0)).squeeze(
            1 if not rnn_module.batch_first else 0)
    if xd.shape[2] != rnn_module.input_size:
        raise ValueError(f"input has {xd.shape[2]} features, the module expects {rnn_module.input_size}")
    F_out = (2 if rnn_module.bidirectional else 1) * rnn_module.hidden_size
    out = torch.empty((xd.shape[0], xd.shape[1], F_out), dtype=torch.float32, device=dev)
    if rnn_module.batch_first:
        _rnn_into(rnn_module, xd, out, to)
    else:
        _rnn_into(rnn_module, xd.transpose(0, 1), out.transpose(0, 1), to)
    return out if x.is_cuda else out.cpu()


def layernorm_forward(x, ln):
    """nn.LayerNorm over the last axis of a float32 CUDA tensor, in place."""
    L = _lib.lib()
    E = x.shape[-1]
    g = ln.weight.detach().to(x.device, torch.float32).contiguous() if ln.weight is not None else None
    b = ln.bias.detach().to(x.device, torch.float32).contiguous() if ln.bias is not None else None
    check(L.ofp_layernorm(x.data_ptr(), x.numel() // E, E, g.data_ptr() if g is not None else None,
                          b.data_ptr() if b is not None else None, float(ln.eps), x.data_ptr(), _stream(x.device)),
          "ofp_layernorm")
    return x


def attention_mean_head(h, attn, fc, to):
    """fc(attn(h, h, h)[0].mean(1)) for h float32 CUDA contiguous [n, T, E] (eval, need_weights=False): the
    in-projection as one dense layer, self-attention + mean over time in one kernel, then out_proj and fc on
    [n, E] (the mean commutes with both)."""
    L = _lib.lib()
    n, T, E = h.shape
    qkv = dense_forward(h.reshape(n * T, E), to(attn.in_proj_weight),
                        to(attn.in_proj_bias) if attn.in_proj_bias is not None else None, None, None, 0)
    ctx = torch.empty((n, E), dtype=torch.float32, device=h.device)
    check(L.ofp_attention_mean(qkv.data_ptr(), n, T, E, attn.num_heads, ctx.data_ptr(), _stream(h.device)),
          "ofp_attention_mean")
    o = attn.out_proj
    ctx = dense_forward(ctx, to(o.weight), to(o.bias) if o.bias is not None else None, None, None, 0)
    return dense_forward(ctx, to(fc.weight), to(fc.bias) if fc.bias is not None else None, None, None, 0)


def _check_attention(E, num_heads):
    if num_heads < 1 or E % num_heads:
        raise ValueError(f"embedding width {E} is not divisible by {num_heads} heads")
    if E // num_heads > ATTN_MAX_HEAD_DIM:
        raise ValueError(f"head dim {E // num_heads} > {ATTN_MAX_HEAD_DIM} has no HIP implementation")


class RNN(nn.Module):
    """``model.RNN`` (model.py:168-307): a recurrent stack over the sensor channels (or over every adjacent channel
    pair with shared weights), LayerNorm, multi-head self-attention, the mean over time and a Linear.  Same
    constructor arguments, defaults and parameter names (``rnn``, ``layer_norm``, ``attention``, ``fc``) as the
    reference; ``forward`` is inference-only and runs as HIP kernels.  ``activation`` is accepted and unused, as in
    the reference."""

    def __init__(self, input_size: int, output_size: int, channels: int = 3, hidden_size: int = 64,
                 num_layers: int = 2, dropout_rate: float = 0.5, loss=F.l1_loss, rnn_type: str = "GRU",
                 batch_first: bool = True, bidirectional: bool = False, bias: bool = True, lr: float = 1e-3,
                 activation=nn.SiLU, num_heads: int = 2, share_input_weights: bool = False,
                 permute_input: bool = True) -> None:
        super().__init__()
        classes = {"LSTM": nn.LSTM, "GRU": nn.GRU, "RNN": nn.RNN}
        if rnn_type not in classes:
            raise ValueError(f"rnn_type {rnn_type!r}: one of {sorted(classes)}")
        if hidden_size > RNN_MAX_HIDDEN:
            raise ValueError(f"hidden_size {hidden_size} > {RNN_MAX_HIDDEN} has no HIP implementation")
        self.channels, self.hidden_size, self.num_layers = channels, hidden_size, num_layers
        self.batch_first, self.bidirectional = batch_first, bidirectional
        self.lr, self.loss = lr, loss
        self.share_input_weights, self.permute_input = share_input_weights, permute_input
        self.rnn = classes[rnn_type](input_size=channels if not share_input_weights else 2, hidden_size=hidden_size,
                                     num_layers=num_layers, dropout=dropout_rate if num_layers > 1 else 0,
                                     batch_first=batch_first, bidirectional=bidirectional, bias=bias)
        multiplier = (2 if bidirectional else 1) * (1 if not share_input_weights else channels - 1)
        E = hidden_size * multiplier
        _check_attention(E, num_heads)
        self.layer_norm = nn.LayerNorm(E)
        self.attention = nn.MultiheadAttention(E, num_heads, batch_first=True, dropout=dropout_rate)
        self.fc = nn.Linear(E, output_size)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """x [batch, channels, input_size] ([batch, input_size, channels] with permute_input=False) ->
        [batch, output_size].  With batch_first=False the recurrence runs along the batch axis, as the
        reference's does."""
        dev = x.device if x.is_cuda else torch.device("cuda", 0)
        _lib.require_gpu(dev.index or 0)
        to = lambda t: t.detach().to(dev, torch.float32).contiguous()
        xd = to(x)
        x3 = xd.permute(0, 2, 1) if self.permute_input else xd  # [batch, time, features], a view
        n0, n1, _ = x3.shape
        E = self.fc.in_features
        out = torch.empty((n0, n1, E), dtype=torch.float32, device=dev)
        # the recurrence's own [sequence, step] axes: a transposed view when batch_first=False
        xt, ot = (x3, out) if self.batch_first else (x3.transpose(0, 1), out.transpose(0, 1))
        if not self.share_input_weights:
            _rnn_into(self.rnn, xt, ot, to)
        else:  # pair i reads channels i, i+1 in place and fills slot i of torch.cat(outs, -1)
            w = E // (self.channels - 1)
            for i in range(self.channels - 1):
                _rnn_into(self.rnn, xt[..., i:i + 2], ot[..., i * w:(i + 1) * w], to)
        layernorm_forward(out, self.layer_norm)
        y = attention_mean_head(out, self.attention, self.fc, to)
        return y if x.is_cuda else y.cpu()


class CNNRNN(nn.Module):
    """``model.CNNRNN`` (model.py:310-440): the CNN conv stack, a GRU that runs over the conv *channels* as its time
    axis with the conv width as the feature, self-attention (2 heads), the mean over time and a Linear.  Same
    constructor arguments and parameter names (``conv_layers.conv{i}`` / ``bn{i}``, ``rnn``, ``attention``,
    ``fc``) as the reference; ``forward`` is inference-only and runs as HIP kernels."""

    def __init__(self, input_size: int, output_size: int, channels: int = 3, layer_sizes=[8, 16],
                 kernel_size: int = 3, dropout_rate: float = 0.5, n_hidden: int = 64, n_rnn_layers: int = 1,
                 loss=F.l1_loss, batch_norm=False, pool=False, padding=1, dilation=1, groups=1, lr=1e-3,
                 activation=nn.SiLU) -> None:
        super().__init__()
        if activation not in ACT_CODES:
            raise ValueError(f"activation {activation} has no HIP implementation")
        if n_hidden > RNN_MAX_HIDDEN:
            raise ValueError(f"n_hidden {n_hidden} > {RNN_MAX_HIDDEN} has no HIP implementation")
        _check_attention(n_hidden, 2)
        self._act_code = ACT_CODES[activation]
        self._padding, self._dilation, self._groups = padding, dilation, groups
        self.conv_layers = nn.Sequential()
        cur, width = channels, input_size
        for i, size in enumerate(layer_sizes):
            self.conv_layers.add_module(
                f"conv{i+1}", nn.Conv1d(cur, size, kernel_size, padding=padding, dilation=dilation, groups=groups))
            self.conv_layers.add_module(f"act{i+1}", activation())
            width = width + 2 * padding - dilation * (kernel_size - 1)
            if batch_norm:
                self.conv_layers.add_module(f"bn{i+1}", nn.BatchNorm1d(size))
            if pool:
                self.conv_layers.add_module(f"pool{i+1}", nn.MaxPool1d(kernel_size=2, stride=2))
                width //= 2
            cur = size
        self.dropout = nn.Dropout(dropout_rate)
        self.rnn = nn.GRU(width, n_hidden, n_rnn_layers, batch_first=True,
                          dropout=dropout_rate if n_rnn_layers > 1 else 0)
        self.attention = nn.MultiheadAttention(n_hidden, 2, batch_first=True, dropout=dropout_rate)
        self.fc = nn.Linear(n_hidden, output_size)
        self.loss = loss
        self.lr = lr

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """x [batch, channels, input_size] -> [batch, output_size] (eval-mode semantics)."""
        dev = x.device if x.is_cuda else torch.device("cuda", 0)
        _lib.require_gpu(dev.index or 0)
        to = lambda t: t.detach().to(dev, torch.float32).contiguous()
        h = _run_conv_stack(self.conv_layers, to(x), to, self._padding, self._dilation, self._act_code, self._groups)
        out = torch.empty((h.shape[0], h.shape[1], self.rnn.hidden_size), dtype=torch.float32, device=dev)
        _rnn_into(self.rnn, h, out, to)  # time axis = the conv channels
        y = attention_mean_head(out, self.attention, self.fc, to)
        return y if x.is_cuda else y.cpu()
