"""The classifiers of the reference's ``model.py`` with their forward passes on MI355X.

``CNN`` (model.py:52-120), ``CCCNN`` / ``LCCCNN`` (:443-580), ``RNN`` (:168-307) and ``CNNRNN``
(:310-440) take the same constructor arguments and use the same parameter names as the reference,
so its ``state_dict`` loads unchanged.  ``forward`` is inference-only (eval semantics: dropout off,
BatchNorm on its running statistics) and runs as HIP kernels (csrc/ofp_nn.hip, csrc/ofp_xcorr.hip,
csrc/ofp_rnn.hip); torch only allocates memory and makes views.  ``rnn_forward`` runs a torch
``nn.GRU`` / ``nn.LSTM`` / ``nn.RNN`` module (its full output sequence) on the same kernels.
``fit_cnn`` trains a ``CNN`` in place with the recipe of its ``training_step`` / ``configure_optimizers``
(full batch, NAdam, cosine warm restarts every 250 epochs) as one graph of HIP kernels per epoch
(csrc/ofp_cnn_train.hip).  ``fit_lcccnn`` trains an ``LCCCNN`` in place with the recipe of its own ``training_step`` /
``configure_optimizers`` (full batch, SGD with momentum 0.8 and weight decay 1e-3 at 100 x ``lr``, cosine annealing over
100 epochs) the same way (csrc/ofp_cccnn_train.hip).  With ``seed=`` both apply the model's dropout and, given a
``data.ShiftedWindows`` or ``data.StretchedWindows``, cut shifted (and stretched) training windows anew every epoch,
from this package's own random stream (csrc/ofp_train_random.h).  ``fit_cnnrnn`` trains a ``CNNRNN`` in place with the
recipe of its ``training_step`` / ``configure_optimizers`` (full batch, NAdam, cosine annealing over 100 epochs) the same
way, back-propagating through the GRU and the attention (csrc/ofp_cnnrnn_train.hip).  Training ``RNN`` is out of scope
(DESIGN.md section 7).
"""
import ctypes
import functools
from types import SimpleNamespace

import numpy as np
import torch
from torch import nn
from torch.nn import functional as F

from . import _lib
from ._lib import check
from .calibration import ACT_CODES, _loss_code, dense_forward
from .data import ShiftedWindows, check_seed


def _stream(dev):
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def fold_batchnorm(bn, device):
    """An eval-mode BatchNorm1d as float32 (scale, shift) on `device`: y = (v - mean) / sqrt(var + eps) * gamma + beta,
    folded in double."""
    inv = (bn.running_var.double() + bn.eps).rsqrt()
    g = bn.weight.double() if bn.weight is not None else torch.ones_like(inv)
    b = bn.bias.double() if bn.bias is not None else torch.zeros_like(inv)
    scale = (g * inv).to(device, torch.float32).contiguous()
    shift = (b - bn.running_mean.double() * g * inv).to(device, torch.float32).contiguous()
    return scale, shift


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
    if bn is not None:
        scale, shift = fold_batchnorm(bn, x.device)
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
        self.input_size, self.channels = input_size, channels

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """x [batch, channels, input_size] -> [batch, output_size] (eval-mode semantics)."""
        dev = x.device if x.is_cuda else torch.device("cuda", 0)
        _lib.require_gpu(dev.index or 0)
        to = lambda t: t.detach().to(dev, torch.float32).contiguous()
        h = _run_conv_stack(self.conv_layers, to(x), to, self._padding, self._dilation, self._act_code, self._groups)
        h = h.reshape(h.shape[0], -1)
        h = dense_forward(h, to(self.fc.weight), to(self.fc.bias), None, None, 0)
        return h if x.is_cuda else h.cpu()

    def configure_optimizers(self):
        """model.py:146-162: NAdam at ``self.lr`` and cosine warm restarts every 250 epochs, stepped once per epoch.
        ``fit_cnn`` builds its per-epoch tables from the same two torch classes."""
        optimizer = torch.optim.NAdam(self.parameters(), lr=self.lr)
        scheduler = torch.optim.lr_scheduler.CosineAnnealingWarmRestarts(optimizer, 250, 1)
        return {"optimizer": optimizer,
                "lr_scheduler": {"scheduler": scheduler, "monitor": "val_loss", "frequency": 1}}


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
        self.input_size = input_size

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
    """``model.LCCCNN`` (model.py:541-629): the training wrapper around CCCNN.  Parameter names
    (``model.conv_layers.conv{i}``, ``model.fc``) follow the reference.  ``forward`` is the HIP inference pass of
    ``CCCNN``; ``fit_lcccnn`` trains the module with the recipe of ``configure_optimizers`` on the GPU."""

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

    def configure_optimizers(self):
        """model.py:606-629: SGD at 100 x ``self.lr`` with momentum 0.8 and weight decay 1e-3 on every parameter, and
        CosineAnnealingLR(T_max = 100), stepped once per epoch.  ``fit_lcccnn`` takes its per-epoch rates from the
        same two torch classes."""
        optimizer = torch.optim.SGD(self.parameters(), lr=self.lr * 100, momentum=LCCCNN_MOMENTUM,
                                    weight_decay=LCCCNN_WEIGHT_DECAY)
        scheduler = torch.optim.lr_scheduler.CosineAnnealingLR(optimizer, 100)
        return {"optimizer": optimizer,
                "lr_scheduler": {"scheduler": scheduler, "monitor": "val_loss", "frequency": 1}}


LCCCNN_MOMENTUM, LCCCNN_WEIGHT_DECAY = 0.8, 1e-3  # model.py:608-614


# ---- the window regressor of a realtime session (realtime.HopSession(regressor=...)) ---------------------------------
def _conv_blocks(layers):
    """[(Conv1d, BatchNorm1d or None, GroupNorm or None, pooled)] of a conv stack, as _run_conv_stack walks it."""
    blocks = []
    for m in layers:
        if isinstance(m, nn.Conv1d):
            blocks.append([m, None, None, False])
        elif isinstance(m, nn.BatchNorm1d):
            blocks[-1][1] = m
        elif isinstance(m, nn.GroupNorm):
            blocks[-1][2] = m
        elif isinstance(m, nn.MaxPool1d):
            blocks[-1][3] = True
    return blocks


def hop_regressor_arch(model, what):
    """What the hop's regress stage needs to know of a ``CNN`` / ``CCCNN`` / ``LCCCNN``, read without a GPU call:
    a namespace with net (the module that owns conv_layers and fc), kind, channels, input_size, n_out, blocks, norm,
    pool.  ValueError for every other class (``RNN`` / ``CNNRNN`` by name: their forward exceeds a hop's budget) and
    for a model outside the stage's envelope."""
    if isinstance(model, (RNN, CNNRNN)):
        raise ValueError(f"{what}: model.{type(model).__name__} is refused as a regressor: the measured forward of "
                         f"RNN / CNNRNN exceeds the hop budget (README.md)")
    net = model.model if isinstance(model, LCCCNN) else model
    if not isinstance(net, (CNN, CCCNN)):
        raise ValueError(f"{what}: the regressor must be a model.CNN, CCCNN or LCCCNN, got {type(model).__name__}")
    blocks = _conv_blocks(net.conv_layers)
    if isinstance(net, CNN):
        kind = _lib.REG_KIND_CNN
        norm = _lib.REG_NORM_BATCH if blocks[0][1] is not None else _lib.REG_NORM_NONE
    else:
        kind = _lib.REG_KIND_CCCNN_GROUPED if net.group else _lib.REG_KIND_CCCNN
        norm = _lib.REG_NORM_GROUP if blocks[0][2] is not None else _lib.REG_NORM_NONE
    a = SimpleNamespace(net=net, kind=kind, channels=net.channels, input_size=net.input_size,
                        n_out=net.fc.out_features, blocks=blocks, norm=norm, pool=blocks[0][3])
    if not 1 <= a.channels <= _lib.REG_MAX_SIGNALS:
        raise ValueError(f"{what}: the regressor takes {a.channels} channels, 1..{_lib.REG_MAX_SIGNALS} supported")
    if not 1 <= len(blocks) <= _lib.REG_MAX_LAYERS:
        raise ValueError(f"{what}: the regressor has {len(blocks)} conv layers, 1..{_lib.REG_MAX_LAYERS} supported")
    if not 1 <= a.n_out <= _lib.REG_MAX_OUT:
        raise ValueError(f"{what}: the regressor has {a.n_out} outputs, 1..{_lib.REG_MAX_OUT} supported")
    if not 1 <= a.input_size <= _lib.REG_MAX_FRAME:
        raise ValueError(f"{what}: the regressor's input_size {a.input_size} is outside 1..{_lib.REG_MAX_FRAME}")
    return a


def hop_regressor_struct(model, device, frame_length, pre_samples, max_distance, min_channels, what="hop_regressor"):
    """(_lib.HopRegressor, the flat parameter tensor it points to) of a ``CNN`` / ``CCCNN`` / ``LCCCNN`` on `device`:
    weights as ``forward`` hands them to the kernels, BatchNorm folded by ``fold_batchnorm``."""
    a = hop_regressor_arch(model, what)
    net, dev = a.net, torch.device("cuda", device) if not isinstance(device, torch.device) else device
    to = lambda t: t.detach().to(dev, torch.float32).contiguous().reshape(-1)
    parts = []
    r = _lib.HopRegressor()
    r.kind, r.channels, r.width, r.n_out, r.n_conv = a.kind, a.channels, a.input_size, a.n_out, len(a.blocks)
    for i, (conv, bn, gn, _) in enumerate(a.blocks):
        r.cout[i], r.kernels[i], r.strides[i] = conv.out_channels, conv.kernel_size[0], conv.stride[0]
        parts.append(to(conv.weight))
        parts.append(to(conv.bias) if conv.bias is not None else torch.zeros(conv.out_channels, device=dev))
        if bn is not None:
            parts += list(fold_batchnorm(bn, dev))
        elif gn is not None:
            parts.append(to(gn.weight) if gn.weight is not None else torch.ones(conv.out_channels, device=dev))
            parts.append(to(gn.bias) if gn.bias is not None else torch.zeros(conv.out_channels, device=dev))
            r.gn_eps = float(gn.eps)
    parts += [to(net.fc.weight), to(net.fc.bias)]
    flat = torch.cat([p.reshape(-1).to(torch.float32) for p in parts]).contiguous()
    r.padding, r.dilation, r.act, r.norm, r.pool = net._padding, net._dilation, net._act_code, a.norm, int(a.pool)
    r.groups = a.blocks[0][0].groups
    r.d_params, r.n_params = flat.data_ptr(), flat.numel()
    r.frame_length, r.pre_samples, r.max_distance, r.min_channels = frame_length, pre_samples, max_distance, min_channels
    return r, flat


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
    the reference.

    Training: ``fit_rnn(model, x, y, ...)`` trains the module in place by the reference's recipe (NAdam with weight
    decay 1e-4, CosineAnnealingLR(3000), one full batch per epoch) as one captured graph of HIP kernels per epoch;
    ``rnn_loss_and_grads_device`` returns the loss and every gradient of one batch.  Trained are GRU stacks of 1 to 4
    unidirectional layers with batch_first, biases and their own input weights, hidden_size up to 128, up to 8 channels
    and windows of up to 512 samples; LSTM, the plain RNN cell, bidirectional stacks, share_input_weights=True and
    batch_first=False run here (inference) but are not trained."""

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


# ---- training model.CNN (model.py:122-162, train.py) ---------------------------------------------------------------
CNN_TRAIN_MAX_LAYERS, CNN_TRAIN_MAX_CHANNELS, CNN_TRAIN_MAX_KERNEL = 3, 128, 8  # csrc/ofp_cnn_train.hip
CNN_TRAIN_MAX_WIDTH, CNN_TRAIN_MAX_BATCH, CNN_TRAIN_MAX_OUT = 512, 1024, 16


@functools.lru_cache(maxsize=256)
def cnn_rates(lr, num_epochs):
    """The learning rate of every epoch of CNN.configure_optimizers(): torch's own CosineAnnealingWarmRestarts(T_0 =
    250, T_mult = 1) stepped once per epoch on a dummy parameter.  float64 [num_epochs]."""
    p = nn.Parameter(torch.zeros(1))
    opt = torch.optim.NAdam([p], lr=lr)
    sched = torch.optim.lr_scheduler.CosineAnnealingWarmRestarts(opt, 250, 1)
    opt.step()
    rates = np.empty(num_epochs, np.float64)
    for e in range(num_epochs):
        rates[e] = float(opt.param_groups[0]["lr"])
        sched.step()
    rates.setflags(write=False)
    return rates


def cnn_rate_table(lr, num_epochs):
    """float64 [num_epochs][5]: lr_t, mu_t, mu_{t+1}, mu_product_t and bias_correction2_t of torch.optim.NAdam's
    defaults (betas 0.9 / 0.999, momentum_decay 0.004), computed as _single_tensor_nadam computes them: Python
    doubles, except the running mu_product, which torch keeps in a tensor of its scalar dtype (float32 unless the
    default dtype is float64) and multiplies by mu_t there."""
    rates = cnn_rates(float(lr), int(num_epochs))
    scalar = torch.float64 if torch.get_default_dtype() == torch.float64 else torch.float32
    mu_product = torch.tensor(1.0, dtype=scalar)
    table = np.empty((num_epochs, 5), np.float64)
    for e in range(num_epochs):
        step = float(e + 1)
        bias_correction2 = 1 - 0.999 ** step
        mu = 0.9 * (1.0 - 0.5 * (0.96 ** (step * 0.004)))
        mu_next = 0.9 * (1.0 - 0.5 * (0.96 ** ((step + 1) * 0.004)))
        mu_product *= mu
        table[e] = rates[e], mu, mu_next, mu_product.item(), bias_correction2
    return table


def cnn_step_factors(table):
    """Rows of cnn_rate_table -> float64 [n][3]: the factor of g / denom, the factor of exp_avg / denom, and
    bias_correction2, as _single_tensor_nadam forms them in double."""
    lr, mu, mu_next, mu_product, bc2 = np.asarray(table, np.float64).T
    return np.stack([-lr * (1.0 - mu) / (1.0 - mu_product), (-lr * mu_next) / (1.0 - mu_product * mu_next), bc2], 1)


def _cnn_device_rows(lr, num_epochs):
    """float32 [num_epochs][4] for ofp_cnn_train: cnn_step_factors rounded once, and a pad."""
    rows = np.zeros((num_epochs, 4), np.float32)
    rows[:, :3] = cnn_step_factors(cnn_rate_table(lr, num_epochs))
    return rows


def _check_dropout(p, seed):
    """The trainers' dropout is this package's own stream (include/onsetfp.h) and needs the user's seed."""
    if seed is not None:
        check_seed(seed)
    if not 0 <= p < 1:
        raise ValueError(f"dropout_rate {p}: the trainer needs 0 <= dropout_rate < 1")
    if p > 0 and seed is None:
        raise ValueError(f"dropout_rate {p} cannot be trained on the GPU: torch's dropout stream cannot "
                         "be matched (construct the model with dropout_rate=0.0, or pass seed= for this package's "
                         "own dropout stream)")


def _train_random(p, seed, epoch=0, source=None):
    """(_lib.TrainRandom or None, what it points to): the random options of a trainer call.  None when nothing is
    random (no dropout, no window source): the call is then the one without options."""
    if (seed is None or p == 0) and source is None:
        return None, None
    if int(epoch) < 0:
        raise ValueError("epoch must not be negative")
    r = _lib.TrainRandom()
    r.epoch = int(epoch)
    if seed is not None:
        r.seed, r.dropout_p = int(seed), float(p)
    keep = None
    if source is not None:
        keep = audio, starts = source.resident()
        r.max_shift, r.n_extractions, r.audio_channels = source.max_shift, source.n_extractions, source.channels
        r.d_audio, r.audio_len, r.d_starts, r.n_onsets = audio.data_ptr(), audio.shape[0], starts.data_ptr(), \
            source.n_onsets
    return r, keep


def _batch_of(x, y, what):
    """(x, y, (n, channels, width)) of a batch; x may be a data.ShiftedWindows, whose y [n_onsets, outputs] is tiled."""
    if isinstance(x, ShiftedWindows):
        if what != "x":
            raise ValueError("a window source cannot be x_val: the validation forward takes the windows themselves")
        y = torch.as_tensor(y)
        if y.dim() != 2 or y.shape[0] != x.n_onsets:
            raise ValueError(f"y {tuple(y.shape)}: expected [{x.n_onsets}, outputs], one row per onset of the window "
                             "source")
        return x, y.repeat(x.n_extractions, 1), (x.n, x.channels, x.frame_length)
    x, y = torch.as_tensor(x), torch.as_tensor(y)
    if x.dim() != 3 or y.dim() != 2 or x.shape[0] != y.shape[0]:
        raise ValueError(f"{what} {tuple(x.shape)} / y {tuple(y.shape)}: expected [n, channels, width] and [n, outputs]")
    return x, y, tuple(int(d) for d in x.shape)


def _stretch_span(source):
    """The stretch span of a window source: a data.StretchedWindows' span, else 0."""
    return int(getattr(source, "stretch_span", 0)) if source is not None else 0


def _check_source(x, seed):
    if isinstance(x, ShiftedWindows) and (x.max_shift > 0 or _stretch_span(x) > 0) and seed is None:
        raise ValueError("a window source with max_shift > 0 or a stretch needs seed=")


def _cnn_arch(model, width=None, seed=None, flat_head=True):
    """(CnnConfig, convs, batch norms) of a CNN for the trainer; ValueError for what it cannot run.  flat_head=False:
    ``fc`` does not read the flattened conv features (a CNNRNN; _cnnrnn_arch checks what does)."""
    _check_dropout(model.dropout.p, seed)
    loss = _loss_code(model.loss)
    mods = list(model.conv_layers)
    convs = [m for m in mods if isinstance(m, nn.Conv1d)]
    bns = [m for m in mods if isinstance(m, nn.BatchNorm1d)]
    pools = [m for m in mods if isinstance(m, nn.MaxPool1d)]
    acts = [m for m in mods if not isinstance(m, (nn.Conv1d, nn.BatchNorm1d, nn.MaxPool1d))]
    codes = set()
    for a in acts:
        if type(a) not in ACT_CODES:
            raise ValueError(f"activation {type(a).__name__} has no HIP implementation")
        codes.add(ACT_CODES[type(a)])
    if len(acts) != len(convs) or len(codes) != 1:
        raise ValueError("every Conv1d must be followed by one and the same activation")
    if not 1 <= len(convs) <= CNN_TRAIN_MAX_LAYERS:
        raise ValueError(f"{len(convs)} conv layers: the trainer's limit is 1..{CNN_TRAIN_MAX_LAYERS}")
    if len(bns) not in (0, len(convs)) or len(pools) not in (0, len(convs)):
        raise ValueError("BatchNorm1d / MaxPool1d must follow every Conv1d or none")
    c0 = convs[0]
    key = lambda m: (m.kernel_size, m.stride, m.padding, m.dilation, m.groups, m.padding_mode, m.bias is not None)
    if any(key(m) != key(c0) for m in convs) or c0.stride != (1,) or c0.padding_mode != "zeros" or c0.bias is None \
            or not isinstance(c0.padding[0], int):
        raise ValueError("the Conv1d layers must share kernel size, padding, dilation and groups, with stride 1, "
                         "zero padding and a bias")
    if any(m.kernel_size != 2 or m.stride != 2 or m.padding != 0 or m.dilation != 1 or m.ceil_mode for m in pools):
        raise ValueError("only MaxPool1d(kernel_size=2, stride=2) is trained")
    for m in bns:
        if m.momentum is None:
            raise ValueError("BatchNorm1d(momentum=None), the cumulative average, is not trained on the GPU")
        if not (m.affine and m.track_running_stats) or (m.eps, m.momentum) != (bns[0].eps, bns[0].momentum):
            raise ValueError("the BatchNorm1d layers must be affine, track running statistics and share eps and "
                             "momentum")
    channels = [c0.in_channels] + [m.out_channels for m in convs]
    if max(channels) > CNN_TRAIN_MAX_CHANNELS:
        raise ValueError(f"{max(channels)} channels: the trainer's limit is {CNN_TRAIN_MAX_CHANNELS}")
    k = c0.kernel_size[0]
    if k > CNN_TRAIN_MAX_KERNEL:
        raise ValueError(f"kernel size {k}: the trainer's limit is {CNN_TRAIN_MAX_KERNEL}")
    if model.fc.out_features > CNN_TRAIN_MAX_OUT or model.fc.bias is None:
        raise ValueError(f"the Linear head needs a bias and at most {CNN_TRAIN_MAX_OUT} outputs")
    cfg = _lib.CnnConfig()
    cfg.n_conv = len(convs)
    for i, c in enumerate(channels):
        cfg.channels[i] = c
    cfg.kernel, cfg.padding, cfg.dilation, cfg.groups = k, c0.padding[0], c0.dilation[0], c0.groups
    cfg.act, cfg.batch_norm, cfg.pool, cfg.loss = codes.pop(), int(bool(bns)), int(bool(pools)), loss
    cfg.n_out = model.fc.out_features
    cfg.bn_momentum, cfg.bn_eps = (bns[0].momentum, bns[0].eps) if bns else (0.1, 1e-5)
    if width is not None:
        if not 1 <= width <= CNN_TRAIN_MAX_WIDTH:
            raise ValueError(f"window of {width} samples: the trainer's limit is 1..{CNN_TRAIN_MAX_WIDTH}")
        cfg.width = w = width
        for _ in convs:
            w = w + 2 * cfg.padding - cfg.dilation * (k - 1)
            w = w // 2 if pools else w
            if w < 1:
                raise ValueError(f"a window of {width} samples leaves no column after the conv layers")
        if flat_head and channels[-1] * w != model.fc.in_features:
            raise ValueError(f"a window of {width} samples gives {channels[-1] * w} features; the model's Linear "
                             f"expects {model.fc.in_features}")
    return cfg, convs, bns


def _cnn_tensors(model, seed=None):
    """[(state_dict name, tensor)] of the parameters in packing order, and the running statistics likewise."""
    _cfg, convs, bns = _cnn_arch(model, seed=seed)
    names = {id(m): n for n, m in model.conv_layers.named_children()}
    ps, st = [], []
    for i, conv in enumerate(convs):
        n = "conv_layers." + names[id(conv)]
        ps += [(n + ".weight", conv.weight), (n + ".bias", conv.bias)]
        if bns:
            b = "conv_layers." + names[id(bns[i])]
            ps += [(b + ".weight", bns[i].weight), (b + ".bias", bns[i].bias)]
            st += [(b + ".running_mean", bns[i].running_mean), (b + ".running_var", bns[i].running_var)]
    ps += [("fc.weight", model.fc.weight), ("fc.bias", model.fc.bias)]
    return ps, st


def _flat(tensors, dev):
    if not tensors:
        return torch.zeros(1, dtype=torch.float32, device=dev)
    return torch.cat([t.detach().reshape(-1).to(dev, torch.float32) for _n, t in tensors]).contiguous()


def _cnn_batch(model, x, y, what="x", seed=None):
    x, y, shape = _batch_of(x, y, what)
    if not 1 <= shape[0] <= CNN_TRAIN_MAX_BATCH:
        raise ValueError(f"{shape[0]} windows: the trainer's limit is 1..{CNN_TRAIN_MAX_BATCH} (one full batch)")
    cfg, _c, bns = _cnn_arch(model, shape[2], seed)
    if shape[1] != cfg.channels[0] or y.shape[1] != cfg.n_out:
        raise ValueError(f"{what} {shape} / y {tuple(y.shape)} do not fit a model of {cfg.channels[0]} "
                         f"channels and {cfg.n_out} outputs")
    if bns and shape[0] * (shape[2] + 2 * cfg.padding - cfg.dilation * (cfg.kernel - 1)) < 2:
        raise ValueError("Expected more than 1 value per channel when training (BatchNorm1d)")
    return x, y, cfg


def _train_device(model, x):
    if isinstance(x, ShiftedWindows):
        return x.resident()[0].device
    if x.is_cuda:
        return x.device
    p = model.fc.weight
    return p.device if p.is_cuda else torch.device("cuda", 0)


def _workspace(nbytes, dev):
    return torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=dev)


def _split(flat, tensors, copy=False):
    """The pieces of a flat tensor that belong to a (name, tensor) list: copied into the tensors, or {name: view}."""
    named, o = {}, 0
    for name, t in tensors:
        piece = flat[o:o + t.numel()].reshape(t.shape)
        o += t.numel()
        if copy:
            t.copy_(piece)
        else:
            named[name] = piece
    return named


def _loss_and_grads(spec, model, x, y, seed, epoch):
    """cnn_ / cccnn_ / cnnrnn_ / rnn_loss_and_grads_device; `spec` is _CNN, _LCCCNN, _CNNRNN or _RNN."""
    x, y, cfg = spec.batch(model, x, y, seed=seed)
    net = spec.net(model)
    rnd, _keep = _train_random(spec.dropout(net), seed, epoch)
    dev = _train_device(net, x)
    _lib.require_gpu(dev.index or 0)
    L = _lib.lib()
    ps, _st = spec.tensors(model, seed)
    p0 = _flat(ps, dev)
    xd, yd = x.detach().to(dev, torch.float32).contiguous(), y.detach().to(dev, torch.float32).contiguous()
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    grads = torch.empty_like(p0)
    n = int(xd.shape[0])
    rp = ctypes.byref(rnd) if rnd is not None else None
    ws_bytes = int(getattr(L, spec.c_workspace)(ctypes.byref(cfg), n, 0, rp))
    if ws_bytes < 0:
        raise ValueError(_lib.last_error())
    ws = _workspace(ws_bytes, dev)
    with torch.cuda.device(dev):
        check(getattr(L, spec.c_grads + "_random")(ctypes.byref(cfg), n, xd.data_ptr(), yd.data_ptr(), p0.data_ptr(),
                                                   loss.data_ptr(), grads.data_ptr(), ws.data_ptr(), ws_bytes,
                                                   _stream(dev), rp), spec.c_grads)
    return loss[0], _split(grads, ps)


def _fit(spec, model, x, y, x_val, y_val, max_epochs, min_epochs, patience, seed):
    """fit_cnn / fit_lcccnn / fit_cnnrnn / fit_rnn; `spec` is _CNN, _LCCCNN, _CNNRNN or _RNN."""
    x, y, cfg = spec.batch(model, x, y, seed=seed)
    _check_source(x, seed)
    source = x if isinstance(x, ShiftedWindows) else None
    have_val = x_val is not None or y_val is not None
    if have_val:
        if x_val is None or y_val is None:
            raise ValueError("x_val and y_val go together")
        x_val, y_val, cfg_v = spec.batch(model, x_val, y_val, "x_val", seed)
        if cfg_v.width != cfg.width:
            raise ValueError(f"x_val is {cfg_v.width} samples wide, x {cfg.width}")
    max_epochs, min_epochs = int(max_epochs), int(min_epochs)
    if max_epochs < 1 or min_epochs < 0:
        raise ValueError("max_epochs must be at least 1 and min_epochs at least 0")
    if patience is not None and (not have_val or int(patience) < 0):
        raise ValueError("patience needs x_val / y_val and must not be negative")
    lr = float(model.lr)

    net = spec.net(model)
    dev = _train_device(net, x)
    _lib.require_gpu(dev.index or 0)
    L = _lib.lib()
    ps, st = spec.tensors(model, seed)
    params = _flat(ps, dev)
    stats = (_flat(st, dev),) if spec.stats else ()
    to = lambda t: t.detach().to(dev, torch.float32).contiguous()
    xd, yd = (None if source else to(x)), to(y)
    rnd, _keep = _train_random(spec.dropout(net), seed, 0, source)
    rp = ctypes.byref(rnd) if rnd is not None else None
    xv, yv = (to(x_val), to(y_val)) if have_val else (None, None)
    rates = torch.from_numpy(spec.device_rates(lr, max_epochs)).to(dev)
    train_loss = torch.full((max_epochs,), float("nan"), dtype=torch.float32, device=dev)
    val_loss = torch.full_like(train_loss, float("nan")) if have_val else None
    n, nv = int(yd.shape[0]), int(xv.shape[0]) if have_val else 0
    span = _stretch_span(source)  # 0: the entries below are the `_random` ones
    ws_bytes = int(getattr(L, spec.c_train + "_stretch_workspace_bytes")(ctypes.byref(cfg), n, nv, rp, span))
    if ws_bytes < 0:
        raise ValueError(_lib.last_error())
    ws = _workspace(ws_bytes, dev)
    epochs = ctypes.c_int32(0)
    ptr = lambda t: t.data_ptr() if t is not None else None
    # the epoch graph is captured on a stream of its own (the null stream cannot be captured); the call returns
    # after that stream has drained
    cur = torch.cuda.current_stream(dev)
    side = torch.cuda.Stream(dev)
    side.wait_stream(cur)
    with torch.cuda.device(dev):
        check(getattr(L, spec.c_train + "_stretch")(ctypes.byref(cfg), n, ptr(xd), yd.data_ptr(), nv, ptr(xv), ptr(yv),
                                                    rates.data_ptr(), max_epochs, min_epochs,
                                                    -1 if patience is None else int(patience), params.data_ptr(),
                                                    *(t.data_ptr() for t in stats), train_loss.data_ptr(),
                                                    ptr(val_loss), ctypes.byref(epochs), ws.data_ptr(), ws_bytes,
                                                    ctypes.c_void_p(side.cuda_stream), rp, span), spec.c_train)
    cur.wait_stream(side)
    with torch.no_grad():
        _split(params, ps, copy=True)
        if spec.stats:
            _split(stats[0], st, copy=True)
        spec.after_fit(model, epochs.value)
    model.eval()
    return SimpleNamespace(train_loss=train_loss, val_loss=val_loss, epochs=int(epochs.value),
                           lrs=np.array(spec.rates(lr, max_epochs)[:epochs.value]), seed=seed)


def _cnn_count_batches(model, epochs):
    for m in model.conv_layers:
        if isinstance(m, nn.BatchNorm1d):
            m.num_batches_tracked += epochs


# What differs between the trainable models (_CNN, _LCCCNN, _CNNRNN, _RNN), for _fit and _loss_and_grads: the batch
# checker, the (name, tensor) lists (parameters, running statistics), the module that carries `fc`, its dropout rate,
# the rate table sent to the device and the rates returned, the C entries, whether the train entry takes d_stats, and
# what is left to do after a fit.
_CNN = SimpleNamespace(
    batch=_cnn_batch, tensors=_cnn_tensors, net=lambda model: model, device_rates=_cnn_device_rows, rates=cnn_rates,
    c_workspace="ofp_cnn_train_random_workspace_bytes", c_train="ofp_cnn_train", c_grads="ofp_cnn_loss_grads",
    stats=True, after_fit=_cnn_count_batches, dropout=lambda net: net.dropout.p)


def cnn_loss_and_grads_device(model, x, y, seed=None, epoch=0):
    """Loss (``model.loss``) and the gradient of every parameter of a CNN for the full batch x [n, channels, width],
    y [n, outputs], in training mode (BatchNorm on batch statistics; the module's running statistics are not
    touched), by the trainer's own forward and backward kernels.  With a seed the model's dropout is applied as
    epoch `epoch` of ``fit_cnn(..., seed=seed)`` applies it (``dropout_mask_device``).  Returns (loss, {state_dict
    name: gradient}) on the GPU."""
    return _loss_and_grads(_CNN, model, x, y, seed, epoch)


def fit_cnn(model, x, y, *, x_val=None, y_val=None, max_epochs=1000, min_epochs=0, patience=None, seed=None):
    """Train a ``CNN`` in place, as ``Trainer.fit(model, ...)`` does with the reference's recipe (model.py:122-162,
    train.py): the whole of x [n, channels, width] / y [n, outputs] is one batch; every epoch is one training-mode
    forward, ``model.loss`` (F.l1_loss or F.mse_loss), backward and one NAdam step at the learning rate of
    CosineAnnealingWarmRestarts(250, 1) starting from ``model.lr``; then, with a validation set, an eval-mode forward
    of x_val and its L1 loss (the reference's validation_step always uses F.l1_loss).  One epoch is one launch of a
    captured graph of HIP kernels; the optimiser state starts fresh at every call, as a new Trainer's does.

    Stop rule (``patience`` given; needs the validation set): Lightning's EarlyStopping(monitor="val_loss",
    mode="min", patience=patience) with min_delta 0, restated here because Lightning is not installed: an epoch whose
    validation loss is not below the best so far counts towards patience, a lower loss resets the count; training ends
    after the epoch at which the count reaches patience, but not before min_epochs epochs have run.

    Parameters, BatchNorm running statistics and num_batches_tracked of `model` are updated where they live (CPU or
    GPU) and the model is left in eval mode.  Returns a record with ``train_loss`` and ``val_loss`` (or None): float32
    GPU tensors [max_epochs], NaN beyond the epochs run; ``epochs``: epochs run; ``lrs``: float64 [epochs]; ``seed``.

    ``seed`` (an int in [0, 2**64)) opts into this package's own random stream (Philox4x32-10 keyed by the seed and
    counted by epoch and element; include/onsetfp.h), which is not torch's: ``model.dropout`` is then applied to the
    features in front of ``fc`` in the training forward, with a new mask every epoch (``dropout_mask_device`` returns
    the mask of any epoch); the validation forward is eval mode and has none.  ``x`` may be a ``data.ShiftedWindows``:
    the epoch graph then cuts the training windows from its audio as its first kernel, shifted anew every epoch, and
    ``y`` is [n_onsets, outputs] (tiled over the extractions); with ``max_shift > 0`` that needs the seed too.  A
    ``data.StretchedWindows`` is such a source whose windows that kernel also cuts a few samples longer or shorter,
    anew every epoch, and Fourier-resamples to the window length (the reference's StretchFrameExtractor; site 2 of the
    stream); it needs the seed, and ``x.shifts`` / ``x.stretches`` / ``x.windows(seed, epoch)`` return what any epoch
    used.

    ValueError, before anything runs on the GPU: dropout_rate > 0 without a seed, dropout_rate >= 1, a seed out of
    range, a window source as x_val or with other rows in y than onsets, a shifting or stretching source without a
    seed, a loss other than F.l1_loss / F.mse_loss, an activation without HIP implementation,
    BatchNorm1d(momentum=None), shapes beyond the limits (3 conv layers, 128 channels, kernel 8, window 512, batch 1024,
    16 outputs)."""
    return _fit(_CNN, model, x, y, x_val, y_val, max_epochs, min_epochs, patience, seed)


def dropout_mask_device(seed, epoch, n, features, p, device=0, *, out=None):
    """The dropout mask of epoch `epoch` of a fit with `seed`: float32 GPU tensor [n, features] of 0 (dropped) and
    float32(1 / (1 - p)) (kept), by the kernel the epoch graph runs (``ofp_dropout_mask``).  ``out``: a contiguous
    float32 GPU tensor [n, features] to write into."""
    seed = check_seed(seed)
    n, features = int(n), int(features)
    if not 0 <= p < 1 or n < 1 or features < 1 or int(epoch) < 0:
        raise ValueError("dropout_mask_device needs 0 <= p < 1, n >= 1, features >= 1 and epoch >= 0")
    if out is not None:
        if not (out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.shape == (n, features)):
            raise ValueError("out must be a contiguous float32 GPU tensor [n, features]")
        dev = out.device
    else:
        dev = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
    _lib.require_gpu(dev.index or 0)
    if out is None:
        out = torch.empty((n, features), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        check(_lib.lib().ofp_dropout_mask(seed, int(epoch), n, features, float(p), out.data_ptr(), _stream(dev)),
              "ofp_dropout_mask")
    return out


def conv1d_backward(x, weight, dz, padding, dilation, groups=1, *, dx=None, dw=None, db=None, need_dx=True):
    """The three gradients of a stride-1 Conv1d (ofp_conv1d_backward) on float32 CUDA tensors: x [n, cin, w], weight
    [cout, cin / groups, k], dz [n, cout, wc] -> (dx or None, dw, db); preallocated outputs may be passed."""
    L = _lib.lib()
    n, cin, w = x.shape
    cout, _, k = weight.shape
    dev = x.device
    ws_bytes = int(L.ofp_conv1d_backward_workspace_bytes(n, cin, w, cout, k, padding, dilation, groups))
    if ws_bytes < 0:
        raise ValueError(_lib.last_error())
    if need_dx and dx is None:
        dx = torch.empty_like(x)
    dw = torch.empty_like(weight) if dw is None else dw
    db = torch.empty(cout, dtype=torch.float32, device=dev) if db is None else db
    ws = _workspace(ws_bytes, dev)
    check(L.ofp_conv1d_backward(x.data_ptr(), n, cin, w, weight.data_ptr(), cout, k, padding, dilation, groups,
                                dz.data_ptr(), dx.data_ptr() if need_dx else None, dw.data_ptr(), db.data_ptr(),
                                ws.data_ptr(), ws_bytes, _stream(dev)), "ofp_conv1d_backward")
    return (dx if need_dx else None), dw, db


def linear_head_train(h, weight, bias, y, loss=0, *, out=None, dy=None, loss_out=None, dw=None, db=None, dh=None):
    """The Linear head of both trainers with its loss, forward and backward (ofp_linear_head_train), on float32 CUDA
    tensors: h [n, F], weight [O, F], bias [O], targets y [n, O], loss 0 = L1 / 1 = MSE -> (out [n, O], dy [n, O] =
    d loss / d out, the mean loss [1], dw [O, F], db [O], dh [n, F]); preallocated outputs may be passed."""
    L = _lib.lib()
    n, F_ = h.shape
    O = weight.shape[0]
    dev = h.device
    if weight.shape != (O, F_) or bias.shape != (O,) or y.shape != (n, O):
        raise ValueError(f"h {tuple(h.shape)}, weight {tuple(weight.shape)}, bias {tuple(bias.shape)}, y "
                         f"{tuple(y.shape)} do not fit together")
    ws_bytes = int(L.ofp_linear_head_train_workspace_bytes(n, F_, O))
    if ws_bytes < 0:
        raise ValueError(f"n {n}, {F_} features, {O} outputs: beyond the Linear head's limits (1..{CNN_TRAIN_MAX_BATCH},"
                         f" >= 1, 1..{CNN_TRAIN_MAX_OUT})")

    def new(*shape):
        return torch.empty(shape, dtype=torch.float32, device=dev)

    out = new(n, O) if out is None else out
    dy = new(n, O) if dy is None else dy
    loss_out = new(1) if loss_out is None else loss_out
    dw = new(O, F_) if dw is None else dw
    db = new(O) if db is None else db
    dh = new(n, F_) if dh is None else dh
    ws = _workspace(ws_bytes, dev)
    check(L.ofp_linear_head_train(h.data_ptr(), n, F_, weight.data_ptr(), O, bias.data_ptr(), y.data_ptr(), int(loss),
                                  out.data_ptr(), dy.data_ptr(), loss_out.data_ptr(), dw.data_ptr(), db.data_ptr(),
                                  dh.data_ptr(), ws.data_ptr(), ws_bytes, _stream(dev)), "ofp_linear_head_train")
    return out, dy, loss_out, dw, db, dh


def batchnorm_train_forward(x, gamma, beta, running_mean, running_var, eps=1e-5, momentum=0.1, *, out=None):
    """BatchNorm1d in training mode on float32 CUDA x [n, C, w]: -> (y, mean, rstd); running_mean / running_var are
    updated in place (the variance written is the unbiased one)."""
    L = _lib.lib()
    n, C, w = x.shape
    dev = x.device
    ws_bytes = int(L.ofp_batchnorm_train_workspace_bytes(n, C, w))
    if ws_bytes < 0:
        raise ValueError(f"n {n}, {C} channels, width {w}: beyond the BatchNorm kernels' limits")
    y = torch.empty_like(x) if out is None else out
    mean = torch.empty(C, dtype=torch.float32, device=dev)
    rstd = torch.empty(C, dtype=torch.float32, device=dev)
    ws = _workspace(ws_bytes, dev)
    check(L.ofp_batchnorm_train_forward(x.data_ptr(), n, C, w, gamma.data_ptr(), beta.data_ptr(), float(eps),
                                        float(momentum), running_mean.data_ptr(), running_var.data_ptr(),
                                        y.data_ptr(), mean.data_ptr(), rstd.data_ptr(), ws.data_ptr(), ws_bytes,
                                        _stream(dev)), "ofp_batchnorm_train_forward")
    return y, mean, rstd


def batchnorm_train_backward(x, gamma, mean, rstd, dy, *, out=None):
    """Backward of batchnorm_train_forward: -> (dx, dgamma, dbeta)."""
    L = _lib.lib()
    n, C, w = x.shape
    dev = x.device
    ws_bytes = int(L.ofp_batchnorm_train_workspace_bytes(n, C, w))
    if ws_bytes < 0:
        raise ValueError(f"n {n}, {C} channels, width {w}: beyond the BatchNorm kernels' limits")
    dx = torch.empty_like(x) if out is None else out
    dgamma = torch.empty(C, dtype=torch.float32, device=dev)
    dbeta = torch.empty(C, dtype=torch.float32, device=dev)
    ws = _workspace(ws_bytes, dev)
    check(L.ofp_batchnorm_train_backward(x.data_ptr(), n, C, w, gamma.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
                                         dy.data_ptr(), dx.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(),
                                         ws.data_ptr(), ws_bytes, _stream(dev)), "ofp_batchnorm_train_backward")
    return dx, dgamma, dbeta


def nadam_step(p, g, m, v, row, weight_decay=0.0):
    """One NAdam step in place on float32 CUDA tensors p, m, v with gradient g; row: float32 CUDA [>= 3] =
    cnn_step_factors of the step, rounded.  With weight_decay > 0 the gradient is g + weight_decay p, torch's coupled
    form (ofp_nadam_decay_step, the RNN trainer's step); without it the call is ofp_nadam_step."""
    if weight_decay < 0:
        raise ValueError("weight_decay must not be negative")
    if weight_decay == 0:
        check(_lib.lib().ofp_nadam_step(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(),
                                        row.data_ptr(), _stream(p.device)), "ofp_nadam_step")
    else:
        check(_lib.lib().ofp_nadam_decay_step(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(),
                                              row.data_ptr(), float(weight_decay), _stream(p.device)),
              "ofp_nadam_decay_step")
    return p


# ---- training model.LCCCNN (model.py:541-629, train.py) ------------------------------------------------------------
CCCNN_TRAIN_MAX_LAYERS, CCCNN_TRAIN_MAX_CHANNELS, CCCNN_TRAIN_MAX_KERNEL = 8, 64, 64  # csrc/ofp_cccnn_train.hip
CCCNN_TRAIN_MAX_STRIDE, CCCNN_TRAIN_MAX_WIDTH, CCCNN_TRAIN_MAX_BATCH = 4, 512, 1024
CCCNN_TRAIN_MAX_ITEMS, CCCNN_TRAIN_MAX_OUT, CCCNN_TRAIN_MAX_LDS = 4096, 16, 160 * 1024


def cccnn_head_lds_bytes(K, V):
    """LDS the correlation head's training kernels need for K maps of V columns (maps, two rows of 2V - 1 lags and
    64 words of scratch, float32)."""
    return (K * V + 2 * (2 * V - 1) + 64) * 4


@functools.lru_cache(maxsize=256)
def lcccnn_rates(lr, num_epochs):
    """The learning rate of every epoch of LCCCNN.configure_optimizers() for ``model.lr == lr``: torch's own SGD at
    100 x lr and CosineAnnealingLR(T_max = 100) stepped once per epoch on a dummy parameter (the rate reaches 0 at
    epoch 100 and rises again after it).  float64 [num_epochs]."""
    p = nn.Parameter(torch.zeros(1))
    opt = torch.optim.SGD([p], lr=lr * 100, momentum=LCCCNN_MOMENTUM, weight_decay=LCCCNN_WEIGHT_DECAY)
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, 100)
    opt.step()
    rates = np.empty(num_epochs, np.float64)
    for e in range(num_epochs):
        rates[e] = float(opt.param_groups[0]["lr"])
        sched.step()
    rates.setflags(write=False)
    return rates


def _cccnn_net(model):
    if not isinstance(model, LCCCNN):
        raise ValueError(f"{type(model).__name__} is not an LCCCNN (the loss and the learning rate live there)")
    return model.model


def _cccnn_arch(model, width=None, seed=None):
    """(CccnnConfig, convs, group norms) of an LCCCNN for the trainer; ValueError for what it cannot run."""
    net = _cccnn_net(model)
    _check_dropout(net.dropout.p, seed)
    loss = _loss_code(model.loss)
    mods = list(net.conv_layers)
    convs = [m for m in mods if isinstance(m, nn.Conv1d)]
    gns = [m for m in mods if isinstance(m, nn.GroupNorm)]
    pools = [m for m in mods if isinstance(m, nn.MaxPool1d)]
    acts = [m for m in mods if not isinstance(m, (nn.Conv1d, nn.GroupNorm, nn.MaxPool1d))]
    codes = set()
    for a in acts:
        if type(a) not in ACT_CODES:
            raise ValueError(f"activation {type(a).__name__} has no HIP implementation")
        codes.add(ACT_CODES[type(a)])
    if not 1 <= len(convs) <= CCCNN_TRAIN_MAX_LAYERS:
        raise ValueError(f"{len(convs)} conv layers: the trainer's limit is 1..{CCCNN_TRAIN_MAX_LAYERS}")
    if len(acts) != len(convs) or len(codes) != 1:
        raise ValueError("every Conv1d must be followed by one and the same activation")
    if len(gns) not in (0, len(convs)) or len(pools) not in (0, len(convs)):
        raise ValueError("GroupNorm / MaxPool1d must follow every Conv1d or none")
    C = net.channels
    groups = C if net.group else 1
    c0 = convs[0]
    key = lambda m: (m.padding, m.dilation, m.groups, m.padding_mode, m.bias is not None)
    if any(key(m) != key(c0) for m in convs) or c0.groups != groups or c0.in_channels != groups \
            or c0.padding_mode != "zeros" or c0.bias is None or not isinstance(c0.padding[0], int):
        raise ValueError("the Conv1d layers must share padding and dilation, with zero padding, a bias and one group "
                         "per sensor channel (group=True) or a single input channel (group=False)")
    if any(m.kernel_size != 2 or m.stride != 2 or m.padding != 0 or m.dilation != 1 or m.ceil_mode for m in pools):
        raise ValueError("only MaxPool1d(kernel_size=2, stride=2) is trained")
    for m in gns:
        if m.num_groups != 1 or not m.affine or m.eps != gns[0].eps:
            raise ValueError("the GroupNorm layers must have one group, be affine and share eps")
    for i, m in enumerate(convs):
        k, st = m.kernel_size[0], m.stride[0]
        if k > CCCNN_TRAIN_MAX_KERNEL:
            raise ValueError(f"kernel size {k} of layer {i + 1}: the trainer's limit is {CCCNN_TRAIN_MAX_KERNEL}")
        if st > CCCNN_TRAIN_MAX_STRIDE:
            raise ValueError(f"stride {st} of layer {i + 1}: the trainer's limit is {CCCNN_TRAIN_MAX_STRIDE}")
        if m.out_channels > CCCNN_TRAIN_MAX_CHANNELS or m.out_channels % groups:
            raise ValueError(f"{m.out_channels} channels in layer {i + 1}: the trainer's limit is "
                             f"{CCCNN_TRAIN_MAX_CHANNELS} (layer size x sensor channels when grouped)")
        if i and m.in_channels != convs[i - 1].out_channels:
            raise ValueError("the Conv1d layers do not form a chain")
    if net.fc.out_features > CCCNN_TRAIN_MAX_OUT or net.fc.bias is None:
        raise ValueError(f"the Linear head needs a bias and at most {CCCNN_TRAIN_MAX_OUT} outputs")
    cfg = _lib.CccnnConfig()
    cfg.n_conv, cfg.sensors = len(convs), C
    for i, m in enumerate(convs):
        cfg.layer_sizes[i], cfg.kernels[i], cfg.strides[i] = m.out_channels // groups, m.kernel_size[0], m.stride[0]
    cfg.padding, cfg.dilation, cfg.group = c0.padding[0], c0.dilation[0], int(bool(net.group))
    cfg.act, cfg.norm, cfg.pool, cfg.loss = codes.pop(), int(bool(gns)), int(bool(pools)), loss
    cfg.n_out = net.fc.out_features
    cfg.momentum, cfg.weight_decay = LCCCNN_MOMENTUM, LCCCNN_WEIGHT_DECAY
    cfg.gn_eps = gns[0].eps if gns else 1e-5
    if width is not None:
        if not 1 <= width <= CCCNN_TRAIN_MAX_WIDTH:
            raise ValueError(f"window of {width} samples: the trainer's limit is 1..{CCCNN_TRAIN_MAX_WIDTH}")
        cfg.width = w = width
        for i, m in enumerate(convs):
            span = w + 2 * cfg.padding - cfg.dilation * (m.kernel_size[0] - 1)
            w = (span - 1) // m.stride[0] + 1 if span >= 1 else 0
            w = w // 2 if pools else w
            if w < 1:
                raise ValueError(f"a window of {width} samples leaves no column after conv layer {i + 1}")
            if w > 2 * CCCNN_TRAIN_MAX_WIDTH:
                raise ValueError(f"layer {i + 1} is {w} wide: the trainer's limit is {2 * CCCNN_TRAIN_MAX_WIDTH}")
        K = cfg.layer_sizes[len(convs) - 1]
        if cccnn_head_lds_bytes(K, w) > CCCNN_TRAIN_MAX_LDS:
            raise ValueError(f"the head's {K} maps of {w} columns need {cccnn_head_lds_bytes(K, w)} bytes of LDS: the "
                             f"limit is {CCCNN_TRAIN_MAX_LDS}")
        if C * (2 * w - 1) != net.fc.in_features:
            raise ValueError(f"a window of {width} samples gives {C * (2 * w - 1)} features; the model's Linear "
                             f"expects {net.fc.in_features}")
    return cfg, convs, gns


def _cccnn_tensors(model, seed=None):
    """[(state_dict name, tensor)] of an LCCCNN's parameters in packing order."""
    _cfg, convs, gns = _cccnn_arch(model, seed=seed)
    net = model.model
    names = {id(m): n for n, m in net.conv_layers.named_children()}
    ps = []
    for i, conv in enumerate(convs):
        n = "model.conv_layers." + names[id(conv)]
        ps += [(n + ".weight", conv.weight), (n + ".bias", conv.bias)]
        if gns:
            b = "model.conv_layers." + names[id(gns[i])]
            ps += [(b + ".weight", gns[i].weight), (b + ".bias", gns[i].bias)]
    ps += [("model.fc.weight", net.fc.weight), ("model.fc.bias", net.fc.bias)]
    return ps


def _cccnn_batch(model, x, y, what="x", seed=None):
    x, y, shape = _batch_of(x, y, what)
    C = _cccnn_net(model).channels
    if not 1 <= shape[0] <= CCCNN_TRAIN_MAX_BATCH or shape[0] * C > CCCNN_TRAIN_MAX_ITEMS:
        raise ValueError(f"{shape[0]} windows of {C} channels: the trainer's limits are 1..{CCCNN_TRAIN_MAX_BATCH} "
                         f"windows and {CCCNN_TRAIN_MAX_ITEMS} (window, channel) pairs (one full batch)")
    cfg, _c, _g = _cccnn_arch(model, shape[2], seed)
    if shape[1] != C or y.shape[1] != cfg.n_out:
        raise ValueError(f"{what} {shape} / y {tuple(y.shape)} do not fit a model of {C} channels and "
                         f"{cfg.n_out} outputs")
    return x, y, cfg


_LCCCNN = SimpleNamespace(
    batch=_cccnn_batch, tensors=lambda model, seed: (_cccnn_tensors(model, seed), []), net=lambda model: model.model,
    device_rates=lambda lr, num_epochs: np.asarray(lcccnn_rates(lr, num_epochs), np.float32), rates=lcccnn_rates,
    c_workspace="ofp_cccnn_train_random_workspace_bytes", c_train="ofp_cccnn_train", c_grads="ofp_cccnn_loss_grads",
    stats=False, after_fit=lambda model, epochs: None, dropout=lambda net: net.dropout.p)


def cccnn_loss_and_grads_device(model, x, y, seed=None, epoch=0):
    """Loss (``model.loss``) and the gradient of every parameter of an LCCCNN for the full batch x [n, channels,
    width], y [n, outputs], by the trainer's own forward and backward kernels.  With a seed the model's dropout is
    applied as epoch `epoch` of ``fit_lcccnn(..., seed=seed)`` applies it.  Returns (loss, {state_dict name:
    gradient}) on the GPU."""
    return _loss_and_grads(_LCCCNN, model, x, y, seed, epoch)


def fit_lcccnn(model, x, y, *, x_val=None, y_val=None, max_epochs=1000, min_epochs=0, patience=None, seed=None):
    """Train an ``LCCCNN`` in place, as ``Trainer.fit(model, ...)`` does with the reference's recipe (model.py:541-629,
    train.py): the whole of x [n, channels, width] / y [n, outputs] is one batch; every epoch is one forward,
    ``model.loss`` (F.l1_loss or F.mse_loss), backward and one SGD step (momentum 0.8, weight decay 1e-3 on every
    parameter, dampening 0, no Nesterov) at the learning rate of CosineAnnealingLR(100) starting from 100 x
    ``model.lr``; then, with a validation set, a forward of x_val and its L1 loss (the reference's validation_step
    always uses F.l1_loss).  GroupNorm keeps no running statistics, so both forwards are the same computation.  One
    epoch is one launch of a captured graph of HIP kernels; the optimiser state starts fresh at every call, as a new
    Trainer's does.

    Stop rule (``patience`` given; needs the validation set): Lightning's EarlyStopping(monitor="val_loss",
    mode="min", patience=patience) with min_delta 0, restated here because Lightning is not installed: an epoch whose
    validation loss is not below the best so far counts towards patience, a lower loss resets the count; training ends
    after the epoch at which the count reaches patience, but not before min_epochs epochs have run.

    The parameters of `model` are updated where they live (CPU or GPU) and the model is left in eval mode.  Returns a
    record with ``train_loss`` and ``val_loss`` (or None): float32 GPU tensors [max_epochs], NaN beyond the epochs
    run; ``epochs``: epochs run; ``lrs``: float64 [epochs]; ``seed``.

    ``seed`` and a ``data.ShiftedWindows`` or ``data.StretchedWindows`` as ``x`` work as in ``fit_cnn``: the seed opts
    into this package's own random stream, with which the net's dropout is applied to the head's softmax values in
    front of ``fc`` in the training forward (a new mask every epoch, none in the validation forward), and the window
    source makes the epoch graph cut its training windows from the resident audio, shifted -- and, by a
    ``StretchedWindows``, stretched and resampled -- anew every epoch.

    ValueError, before anything runs on the GPU: dropout_rate > 0 without a seed, dropout_rate >= 1, a seed out of
    range, a window source as x_val or with other rows in y than onsets, a loss other than F.l1_loss / F.mse_loss, an
    activation without HIP implementation, shapes beyond the limits: 1..8 conv layers, kernel size 64, stride 4, 64
    channels per layer (layer size x sensor channels when group=True), window 512, 1024 windows and 4096 (window,
    sensor) pairs, 16 outputs, a head of K maps x V columns with cccnn_head_lds_bytes(K, V) <= 160 KiB, and every
    layer must leave at least one column."""
    return _fit(_LCCCNN, model, x, y, x_val, y_val, max_epochs, min_epochs, patience, seed)


def conv1d_backward_strided(x, weight, dz, padding, dilation, groups=1, stride=1, *, dx=None, dw=None, db=None,
                            need_dx=True):
    """conv1d_backward for any stride (ofp_conv1d_backward_strided): dz [n, cout, wc] with wc = (w + 2 padding -
    dilation (k - 1) - 1) // stride + 1 -> (dx or None, dw, db)."""
    L = _lib.lib()
    n, cin, w = x.shape
    cout, _, k = weight.shape
    dev = x.device
    ws_bytes = int(L.ofp_conv1d_backward_strided_workspace_bytes(n, cin, w, cout, k, padding, dilation, groups,
                                                                 stride))
    if ws_bytes < 0:
        raise ValueError(_lib.last_error())
    if need_dx and dx is None:
        dx = torch.empty_like(x)
    dw = torch.empty_like(weight) if dw is None else dw
    db = torch.empty(cout, dtype=torch.float32, device=dev) if db is None else db
    ws = _workspace(ws_bytes, dev)
    check(L.ofp_conv1d_backward_strided(x.data_ptr(), n, cin, w, weight.data_ptr(), cout, k, padding, dilation,
                                        groups, stride, dz.data_ptr(), dx.data_ptr() if need_dx else None,
                                        dw.data_ptr(), db.data_ptr(), ws.data_ptr(), ws_bytes, _stream(dev)),
          "ofp_conv1d_backward_strided")
    return (dx if need_dx else None), dw, db


def groupnorm1_train_forward(x, gamma, beta, eps=1e-5, pool=False, *, out=None):
    """nn.GroupNorm(1, K) (+ MaxPool1d(2, 2)) on float32 CUDA x [n, K, V], keeping what the backward needs:
    -> (y, mean [n], rstd [n])."""
    L = _lib.lib()
    n, K, V = x.shape
    dev = x.device
    y = torch.empty((n, K, V // 2 if pool else V), dtype=torch.float32, device=dev) if out is None else out
    mean = torch.empty(n, dtype=torch.float32, device=dev)
    rstd = torch.empty(n, dtype=torch.float32, device=dev)
    check(L.ofp_groupnorm1_train_forward(x.data_ptr(), n, K, V, gamma.data_ptr(), beta.data_ptr(), float(eps),
                                         int(bool(pool)), y.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
                                         _stream(dev)), "ofp_groupnorm1_train_forward")
    return y, mean, rstd


def groupnorm1_train_backward(x, gamma, beta, mean, rstd, dy, pool=False, *, out=None):
    """Backward of groupnorm1_train_forward: dy shaped like its y -> (dx [n, K, V], dgamma [K], dbeta [K])."""
    L = _lib.lib()
    n, K, V = x.shape
    dev = x.device
    ws_bytes = int(L.ofp_groupnorm1_train_workspace_bytes(n, K, V))
    if ws_bytes < 0:
        raise ValueError(f"{n} items, {K} channels, width {V}: beyond the GroupNorm kernels' limits")
    dx = torch.empty_like(x) if out is None else out
    dgamma = torch.empty(K, dtype=torch.float32, device=dev)
    dbeta = torch.empty(K, dtype=torch.float32, device=dev)
    ws = _workspace(ws_bytes, dev)
    check(L.ofp_groupnorm1_train_backward(x.data_ptr(), n, K, V, gamma.data_ptr(), beta.data_ptr(), mean.data_ptr(),
                                          rstd.data_ptr(), int(bool(pool)), dy.data_ptr(), dx.data_ptr(),
                                          dgamma.data_ptr(), dbeta.data_ptr(), ws.data_ptr(), ws_bytes,
                                          _stream(dev)), "ofp_groupnorm1_train_backward")
    return dx, dgamma, dbeta


def autocorr_softmax_backward(feat, probs, dout, fc_weight, channels, *, out=None):
    """Backward of the correlation head and the Linear behind it: feat [n * channels, K, V], probs = the forward's
    autocorr_softmax(feat), dout [n, O] = d loss / d out, fc_weight [O, channels * (2V - 1)] -> d loss / d feat."""
    items, K, V = feat.shape
    df = torch.empty_like(feat) if out is None else out
    check(_lib.lib().ofp_autocorr_softmax_backward(feat.data_ptr(), probs.data_ptr(), dout.data_ptr(),
                                                   fc_weight.data_ptr(), items, channels, K, V, dout.shape[1],
                                                   df.data_ptr(), _stream(feat.device)),
          "ofp_autocorr_softmax_backward")
    return df


def sgd_step(p, g, buf, lr, first, momentum=LCCCNN_MOMENTUM, weight_decay=LCCCNN_WEIGHT_DECAY):
    """One torch.optim.SGD step (dampening 0, no Nesterov) in place on float32 CUDA tensors p and buf with gradient g;
    lr: float32 CUDA [>= 1]; first: the momentum buffer is initialised with the gradient."""
    check(_lib.lib().ofp_sgd_step(p.data_ptr(), g.data_ptr(), buf.data_ptr(), p.numel(), lr.data_ptr(),
                                  int(bool(first)), float(momentum), float(weight_decay), _stream(p.device)),
          "ofp_sgd_step")
    return p


# ---- training model.CNNRNN (model.py:310-440) ----------------------------------------------------------------------
CNNRNN_TRAIN_MAX_HIDDEN, CNNRNN_TRAIN_MAX_STEPS, CNNRNN_TRAIN_HEADS = 128, 128, 2  # csrc/ofp_cnnrnn_train.hip
SITE_ATTENTION = 3  # the random stream's site of the attention dropout (include/onsetfp.h)


@functools.lru_cache(maxsize=256)
def cnnrnn_rates(lr, num_epochs):
    """The learning rate of every epoch of CNNRNN.configure_optimizers(): torch's own NAdam at ``lr`` and
    CosineAnnealingLR(T_max = 100) stepped once per epoch on a dummy parameter (the rate reaches 0 at epoch 100 and
    rises again after it).  float64 [num_epochs]."""
    p = nn.Parameter(torch.zeros(1))
    opt = torch.optim.NAdam([p], lr=lr)
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, 100)
    opt.step()
    rates = np.empty(num_epochs, np.float64)
    for e in range(num_epochs):
        rates[e] = float(opt.param_groups[0]["lr"])
        sched.step()
    rates.setflags(write=False)
    return rates


def _cnnrnn_device_rows(lr, num_epochs):
    """float32 [num_epochs][4] for ofp_cnnrnn_train_stretch: cnn_step_factors of NAdam at cnnrnn_rates, rounded once."""
    table = np.array(cnn_rate_table(lr, num_epochs))  # NAdam's own factors do not depend on the schedule
    table[:, 0] = cnnrnn_rates(float(lr), int(num_epochs))
    rows = np.zeros((num_epochs, 4), np.float32)
    rows[:, :3] = cnn_step_factors(table)
    return rows


def _cnnrnn_arch(model, width=None, seed=None):
    """(CnnrnnConfig, convs, batch norms) of a CNNRNN for the trainer; ValueError for what it cannot run."""
    if not isinstance(model, CNNRNN):
        raise ValueError(f"{type(model).__name__} is not a CNNRNN")
    cnn, convs, bns = _cnn_arch(model, width, seed, flat_head=False)
    rnn, att = model.rnn, model.attention
    if not isinstance(rnn, nn.GRU) or rnn.num_layers != 1 or not rnn.batch_first or rnn.bidirectional or not rnn.bias:
        raise ValueError("the trainer runs one unidirectional nn.GRU layer with batch_first and biases "
                         f"(n_rnn_layers={getattr(rnn, 'num_layers', '?')} is not trained on the GPU)")
    H = rnn.hidden_size
    if H % 2 or not 2 <= H <= CNNRNN_TRAIN_MAX_HIDDEN:
        raise ValueError(f"n_hidden {H}: the trainer needs an even hidden size of at most {CNNRNN_TRAIN_MAX_HIDDEN}")
    if convs[-1].out_channels > CNNRNN_TRAIN_MAX_STEPS:
        raise ValueError(f"{convs[-1].out_channels} channels in the last conv layer are the GRU's time steps: the "
                         f"trainer's limit is {CNNRNN_TRAIN_MAX_STEPS}")
    if att.num_heads != CNNRNN_TRAIN_HEADS or not att.batch_first or att.in_proj_bias is None \
            or att.in_proj_weight is None or att.embed_dim != H or att.bias_k is not None or att.add_zero_attn \
            or att.out_proj.bias is None:
        raise ValueError(f"the attention must have {CNNRNN_TRAIN_HEADS} heads, batch_first, biases and one embed dim "
                         f"of n_hidden for q, k and v")
    if att.dropout != model.dropout.p:
        raise ValueError(f"the attention's dropout {att.dropout} differs from the model's {model.dropout.p}")
    if model.fc.in_features != H:
        raise ValueError(f"fc reads {model.fc.in_features} features, the attention gives {H}")
    cfg = _lib.CnnrnnConfig()
    cfg.cnn, cfg.hidden, cfg.heads = cnn, H, att.num_heads
    if width is not None:
        w = width
        for _ in convs:
            w = w + 2 * cnn.padding - cnn.dilation * (cnn.kernel - 1)
            w = w // 2 if cnn.pool else w
        if w != rnn.input_size:
            raise ValueError(f"a window of {width} samples gives conv features {w} wide; the model's GRU expects "
                             f"{rnn.input_size}")
    return cfg, convs, bns


def _cnnrnn_tensors(model, seed=None):
    """[(state_dict name, tensor)] of a CNNRNN's parameters in packing order, and the running statistics likewise."""
    _cnnrnn_arch(model, seed=seed)
    ps, st = _cnn_tensors(model, seed)
    rnn, att = model.rnn, model.attention
    ps = ps[:-2] + [("rnn.weight_ih_l0", rnn.weight_ih_l0), ("rnn.weight_hh_l0", rnn.weight_hh_l0),
                    ("rnn.bias_ih_l0", rnn.bias_ih_l0), ("rnn.bias_hh_l0", rnn.bias_hh_l0),
                    ("attention.in_proj_weight", att.in_proj_weight), ("attention.in_proj_bias", att.in_proj_bias),
                    ("attention.out_proj.weight", att.out_proj.weight), ("attention.out_proj.bias", att.out_proj.bias)
                    ] + ps[-2:]
    return ps, st


def _cnnrnn_batch(model, x, y, what="x", seed=None):
    x, y, shape = _batch_of(x, y, what)
    if not 1 <= shape[0] <= CNN_TRAIN_MAX_BATCH:
        raise ValueError(f"{shape[0]} windows: the trainer's limit is 1..{CNN_TRAIN_MAX_BATCH} (one full batch)")
    cfg, _c, bns = _cnnrnn_arch(model, shape[2], seed)
    c = cfg.cnn
    if shape[1] != c.channels[0] or y.shape[1] != c.n_out:
        raise ValueError(f"{what} {shape} / y {tuple(y.shape)} do not fit a model of {c.channels[0]} "
                         f"channels and {c.n_out} outputs")
    if bns and shape[0] * (shape[2] + 2 * c.padding - c.dilation * (c.kernel - 1)) < 2:
        raise ValueError("Expected more than 1 value per channel when training (BatchNorm1d)")
    return x, y, cfg


_CNNRNN = SimpleNamespace(
    batch=_cnnrnn_batch, tensors=_cnnrnn_tensors, net=lambda model: model, device_rates=_cnnrnn_device_rows,
    rates=cnnrnn_rates, c_workspace="ofp_cnnrnn_loss_grads_random_workspace_bytes", c_train="ofp_cnnrnn_train",
    c_grads="ofp_cnnrnn_loss_grads", stats=True, after_fit=_cnn_count_batches, dropout=lambda net: net.dropout.p)


def cnnrnn_loss_and_grads_device(model, x, y, seed=None, epoch=0):
    """Loss (``model.loss``) and the gradient of every parameter of a CNNRNN for the full batch x [n, channels, width],
    y [n, outputs], in training mode (BatchNorm on batch statistics; the module's running statistics are not
    touched), by the trainer's own forward and backward kernels.  With a seed both dropouts are applied as epoch
    `epoch` of ``fit_cnnrnn(..., seed=seed)`` applies them (``dropout_mask_device`` on the conv features [n, C * W],
    ``attention_dropout_mask_device`` on the probabilities).  Returns (loss, {state_dict name: gradient}) on the GPU."""
    return _loss_and_grads(_CNNRNN, model, x, y, seed, epoch)


def fit_cnnrnn(model, x, y, *, x_val=None, y_val=None, max_epochs=1000, min_epochs=0, patience=None, seed=None):
    """Train a ``CNNRNN`` in place with the reference's recipe (model.py:400-440): the whole of x [n, channels, width] /
    y [n, outputs] is one batch; every epoch is one training-mode forward, ``model.loss`` (F.l1_loss or F.mse_loss),
    backward and one NAdam step (no weight decay) at the learning rate of CosineAnnealingLR(100) starting from
    ``model.lr`` (``cnnrnn_rates``); then, with a validation set, an eval-mode forward of x_val and its L1 loss.  The
    contract, the stop rule and the returned record are ``fit_cnn``'s: trained in place, left in eval mode, BatchNorm
    running statistics and num_batches_tracked updated; one epoch is one launch of a captured graph of HIP kernels
    (csrc/ofp_cnnrnn_train.hip).

    ``seed`` opts into this package's own random stream as in ``fit_cnn``: ``model.dropout`` is then applied to the
    conv features [n, C * W] in front of the GRU (site 0; ``dropout_mask_device(seed, epoch, n, C * W, p)`` is the
    mask) and the attention's dropout to its softmax probabilities [n, 2, T, T] (site 3;
    ``attention_dropout_mask_device``), both scaled by 1 / (1 - p), neither in the validation forward.  ``x`` may be a
    ``data.ShiftedWindows`` / ``StretchedWindows`` as for ``fit_cnn``.

    ValueError, before anything runs on the GPU: everything ``fit_cnn`` refuses about the conv stack, the batch, the
    loss, the dropout and the window source; an ``rnn`` that is not one unidirectional batch_first nn.GRU layer with
    biases whose input size is the conv output width; an odd n_hidden or one above 128; more than 128 channels in the
    last conv layer (they are the GRU's time steps); an attention without 2 heads, batch_first, biases and a single
    embed dim, or whose dropout differs from the model's; ``fc`` without a bias."""
    return _fit(_CNNRNN, model, x, y, x_val, y_val, max_epochs, min_epochs, patience, seed)


def _f32_cuda(name, t, shape):
    if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == tuple(shape)):
        raise ValueError(f"{name} must be a contiguous float32 GPU tensor {list(shape)}, got {tuple(t.shape)}")
    return t


def _outs(dev, given, shapes):
    """The output tensors of a stand-alone kernel call: those given (checked), the others new."""
    return [torch.empty(s, dtype=torch.float32, device=dev) if g is None else _f32_cuda("an out= tensor", g, s)
            for g, s in zip(given, shapes)]


def linear_backward(x, w, dy, *, out=None, need_dx=True):
    """The three gradients of y = x w^T + b (ofp_linear_backward) on float32 CUDA tensors: x [rows, in], w [out, in],
    dy [rows, out] -> (dx [rows, in] or None, dw [out, in], db [out]); ``out=(dx, dw, db)`` are preallocated outputs."""
    L = _lib.lib()
    R, I = x.shape
    O = w.shape[0]
    _f32_cuda("x", x, (R, I)), _f32_cuda("w", w, (O, I)), _f32_cuda("dy", dy, (R, O))
    ws_bytes = int(L.ofp_linear_backward_workspace_bytes(R, I, O))
    if ws_bytes < 0:
        raise ValueError(f"{R} rows, {I} inputs, {O} outputs: beyond the Linear backward's limits (2^20, 4096, 4096)")
    dx, dw, db = _outs(x.device, out or (None,) * 3, [(R, I), (O, I), (O,)])
    ws = _workspace(ws_bytes, x.device)
    check(L.ofp_linear_backward(x.data_ptr(), R, I, w.data_ptr(), O, dy.data_ptr(), dx.data_ptr() if need_dx else None,
                                dw.data_ptr(), db.data_ptr(), ws.data_ptr(), ws_bytes, _stream(x.device)),
          "ofp_linear_backward")
    return (dx if need_dx else None), dw, db


def gru_train_forward(x, w_ih, w_hh, b_ih, b_hh, *, out=None):
    """A one-layer batch_first GRU with zero initial state in training form (ofp_gru_train_forward) on float32 CUDA
    tensors: x [n, T, F], w_ih [3H, F], w_hh [3H, H], b_ih, b_hh [3H] (gate order r, z, n) -> (the output sequence
    [n, T, H], gates [n, T, 4H] = r, z, n and W_hn h + b_hn of every step, for gru_train_backward);
    ``out=(sequence, gates)`` are preallocated outputs."""
    L = _lib.lib()
    n, T, F_ = x.shape
    H = w_hh.shape[1]
    _f32_cuda("x", x, (n, T, F_)), _f32_cuda("w_ih", w_ih, (3 * H, F_)), _f32_cuda("w_hh", w_hh, (3 * H, H))
    _f32_cuda("b_ih", b_ih, (3 * H,)), _f32_cuda("b_hh", b_hh, (3 * H,))
    ws_bytes = int(L.ofp_gru_train_forward_workspace_bytes(n, T, F_, H))
    if ws_bytes < 0:
        raise ValueError(_lib.last_error())
    seq, gates = _outs(x.device, out or (None,) * 2, [(n, T, H), (n, T, 4 * H)])
    ws = _workspace(ws_bytes, x.device)
    check(L.ofp_gru_train_forward(x.data_ptr(), n, T, F_, H, w_ih.data_ptr(), w_hh.data_ptr(), b_ih.data_ptr(),
                                  b_hh.data_ptr(), seq.data_ptr(), gates.data_ptr(), ws.data_ptr(), ws_bytes,
                                  _stream(x.device)), "ofp_gru_train_forward")
    return seq, gates


def gru_train_backward(x, w_ih, w_hh, seq, gates, dseq, *, out=None):
    """Back-propagation through time of gru_train_forward (ofp_gru_train_backward): dseq [n, T, H] = the gradient at the
    output sequence -> (dx [n, T, F], dw_ih, dw_hh, db_ih, db_hh); ``out=`` are those five, preallocated."""
    L = _lib.lib()
    n, T, F_ = x.shape
    H = w_hh.shape[1]
    _f32_cuda("x", x, (n, T, F_)), _f32_cuda("w_ih", w_ih, (3 * H, F_)), _f32_cuda("w_hh", w_hh, (3 * H, H))
    _f32_cuda("seq", seq, (n, T, H)), _f32_cuda("gates", gates, (n, T, 4 * H)), _f32_cuda("dseq", dseq, (n, T, H))
    ws_bytes = int(L.ofp_gru_train_backward_workspace_bytes(n, T, F_, H))
    if ws_bytes < 0:
        raise ValueError(_lib.last_error())
    outs = _outs(x.device, out or (None,) * 5, [(n, T, F_), (3 * H, F_), (3 * H, H), (3 * H,), (3 * H,)])
    ws = _workspace(ws_bytes, x.device)
    check(L.ofp_gru_train_backward(x.data_ptr(), n, T, F_, H, w_ih.data_ptr(), w_hh.data_ptr(), seq.data_ptr(),
                                   gates.data_ptr(), dseq.data_ptr(), *(t.data_ptr() for t in outs), ws.data_ptr(),
                                   ws_bytes, _stream(x.device)), "ofp_gru_train_backward")
    return tuple(outs)


def _attention_random(p, seed, epoch):
    if p and seed is None:
        raise ValueError("attention dropout needs seed=")
    rnd, _k = _train_random(float(p), seed, epoch)
    return rnd


def attention_mean_train_forward(h, in_proj_w, in_proj_b, num_heads, p=0.0, seed=None, epoch=0, *, out=None):
    """``attention(h, h, h)[0].mean(1)`` without out_proj, in training form (ofp_attention_mean_train_forward), on
    float32 CUDA tensors: h [n, T, E], in_proj_w [3E, E], in_proj_b [3E] -> (ctx [n, E], qkv [n, T, 3E], probs [n,
    heads, T, T] = the softmax before dropout).  With p > 0 and a seed the probabilities are dropped by site 3 of the
    random stream (``attention_dropout_mask_device``).  ``out=(ctx, qkv, probs)`` are preallocated outputs."""
    L = _lib.lib()
    n, T, E = h.shape
    _f32_cuda("h", h, (n, T, E)), _f32_cuda("in_proj_w", in_proj_w, (3 * E, E)), _f32_cuda("in_proj_b", in_proj_b, (3 * E,))
    rnd = _attention_random(p, seed, epoch)
    ws_bytes = int(L.ofp_attention_mean_train_forward_workspace_bytes(n, T, E, num_heads))
    if ws_bytes < 0:
        raise ValueError(_lib.last_error())
    ctx, qkv, probs = _outs(h.device, out or (None,) * 3, [(n, E), (n, T, 3 * E), (n, num_heads, T, T)])
    ws = _workspace(ws_bytes, h.device)
    check(L.ofp_attention_mean_train_forward(h.data_ptr(), n, T, E, num_heads, in_proj_w.data_ptr(),
                                             in_proj_b.data_ptr(), ctypes.byref(rnd) if rnd is not None else None,
                                             qkv.data_ptr(), probs.data_ptr(), ctx.data_ptr(), ws.data_ptr(), ws_bytes,
                                             _stream(h.device)), "ofp_attention_mean_train_forward")
    return ctx, qkv, probs


def attention_mean_train_backward(h, in_proj_w, num_heads, qkv, probs, dctx, p=0.0, seed=None, epoch=0, *, out=None):
    """Backward of attention_mean_train_forward with the same p, seed and epoch: dctx [n, E] -> (dh [n, T, E],
    d in_proj_w [3E, E], d in_proj_b [3E]); ``out=`` are those three, preallocated."""
    L = _lib.lib()
    n, T, E = h.shape
    _f32_cuda("h", h, (n, T, E)), _f32_cuda("in_proj_w", in_proj_w, (3 * E, E)), _f32_cuda("qkv", qkv, (n, T, 3 * E))
    _f32_cuda("probs", probs, (n, num_heads, T, T)), _f32_cuda("dctx", dctx, (n, E))
    rnd = _attention_random(p, seed, epoch)
    ws_bytes = int(L.ofp_attention_mean_train_backward_workspace_bytes(n, T, E, num_heads))
    if ws_bytes < 0:
        raise ValueError(_lib.last_error())
    outs = _outs(h.device, out or (None,) * 3, [(n, T, E), (3 * E, E), (3 * E,)])
    ws = _workspace(ws_bytes, h.device)
    check(L.ofp_attention_mean_train_backward(h.data_ptr(), n, T, E, num_heads, in_proj_w.data_ptr(), qkv.data_ptr(),
                                              probs.data_ptr(), dctx.data_ptr(),
                                              ctypes.byref(rnd) if rnd is not None else None,
                                              *(t.data_ptr() for t in outs), ws.data_ptr(), ws_bytes,
                                              _stream(h.device)), "ofp_attention_mean_train_backward")
    return tuple(outs)


def attention_dropout_mask_device(seed, epoch, n, heads, T, p, device=0, *, out=None):
    """The attention dropout mask of epoch `epoch` of ``fit_cnnrnn(..., seed=seed)``: float32 GPU tensor [n, heads, T,
    T] of 0 (dropped) and float32(1 / (1 - p)) (kept), site 3 of the random stream (``ofp_attention_dropout_mask``)."""
    seed = check_seed(seed)
    n, heads, T = int(n), int(heads), int(T)
    if not 0 <= p < 1 or n < 1 or heads < 1 or T < 1 or int(epoch) < 0:
        raise ValueError("attention_dropout_mask_device needs 0 <= p < 1, n, heads, T >= 1 and epoch >= 0")
    if out is not None:
        dev = _f32_cuda("out", out, (n, heads, T, T)).device
    else:
        dev = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
    _lib.require_gpu(dev.index or 0)
    if out is None:
        out = torch.empty((n, heads, T, T), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        check(_lib.lib().ofp_attention_dropout_mask(seed, int(epoch), n, heads, T, float(p), out.data_ptr(),
                                                    _stream(dev)), "ofp_attention_dropout_mask")
    return out


# ---- training model.RNN (model.py:168-307) ---------------------------------------------------------------------------
RNN_TRAIN_MAX_LAYERS, RNN_TRAIN_MAX_HIDDEN, RNN_TRAIN_MAX_HEADS = 4, 128, 8  # csrc/ofp_rnn_train.hip
RNN_TRAIN_MAX_CHANNELS, RNN_TRAIN_MAX_STEPS, RNN_TRAIN_MAX_ROWS = 8, 512, 1 << 20
RNN_WEIGHT_DECAY, RNN_T_MAX = 1e-4, 3000  # RNN.configure_optimizers
SITE_LAYER = 4  # the random stream's site of the dropout between recurrent layers (include/onsetfp.h)


@functools.lru_cache(maxsize=256)
def rnn_rates(lr, num_epochs):
    """The learning rate of every epoch of RNN.configure_optimizers(): torch's own NAdam at ``lr`` (weight decay 1e-4)
    and CosineAnnealingLR(T_max = 3000) stepped once per epoch on a dummy parameter.  float64 [num_epochs]."""
    p = nn.Parameter(torch.zeros(1))
    opt = torch.optim.NAdam([p], lr=lr, weight_decay=RNN_WEIGHT_DECAY)
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, RNN_T_MAX)
    opt.step()
    rates = np.empty(num_epochs, np.float64)
    for e in range(num_epochs):
        rates[e] = float(opt.param_groups[0]["lr"])
        sched.step()
    rates.setflags(write=False)
    return rates


def _rnn_device_rows(lr, num_epochs):
    """float32 [num_epochs][4] for ofp_rnn_train_stretch: cnn_step_factors of NAdam at rnn_rates, rounded once (the
    weight decay is part of the config, not of the rows)."""
    table = np.array(cnn_rate_table(lr, num_epochs))
    table[:, 0] = rnn_rates(float(lr), int(num_epochs))
    rows = np.zeros((num_epochs, 4), np.float32)
    rows[:, :3] = cnn_step_factors(table)
    return rows


def _rnn_arch(model, seed=None):
    """The RnnConfig of an RNN for the trainer, without the window length; ValueError for what it cannot run."""
    if not isinstance(model, RNN):
        raise ValueError(f"{type(model).__name__} is not an RNN")
    rnn, att, ln = model.rnn, model.attention, model.layer_norm
    if isinstance(rnn, nn.LSTM):
        raise ValueError("rnn_type 'LSTM' is not trained on the GPU (only 'GRU' is)")
    if not isinstance(rnn, nn.GRU):
        raise ValueError("rnn_type 'RNN', the plain recurrent cell, is not trained on the GPU (only 'GRU' is)")
    if rnn.bidirectional:
        raise ValueError("a bidirectional stack is not trained on the GPU")
    if model.share_input_weights:
        raise ValueError("share_input_weights=True is not trained on the GPU")
    if not rnn.batch_first:
        raise ValueError("batch_first=False is not trained on the GPU")
    if not rnn.bias:
        raise ValueError("a recurrent stack without biases (bias=False) is not trained on the GPU")
    L_, H, C = rnn.num_layers, rnn.hidden_size, rnn.input_size
    if not 1 <= L_ <= RNN_TRAIN_MAX_LAYERS:
        raise ValueError(f"num_layers {L_}: the trainer's limit is 1..{RNN_TRAIN_MAX_LAYERS}")
    if not 1 <= H <= RNN_TRAIN_MAX_HIDDEN:
        raise ValueError(f"hidden_size {H}: the trainer's limit is 1..{RNN_TRAIN_MAX_HIDDEN}")
    if not 1 <= att.num_heads <= RNN_TRAIN_MAX_HEADS or H % att.num_heads:
        raise ValueError(f"num_heads {att.num_heads}: the trainer needs 1..{RNN_TRAIN_MAX_HEADS} heads that divide "
                         f"hidden_size {H}")
    if not 1 <= C <= RNN_TRAIN_MAX_CHANNELS:
        raise ValueError(f"{C} channels: the trainer's limit is 1..{RNN_TRAIN_MAX_CHANNELS}")
    if not att.batch_first or att.in_proj_bias is None or att.in_proj_weight is None or att.embed_dim != H \
            or att.bias_k is not None or att.add_zero_attn or att.out_proj.bias is None:
        raise ValueError("the attention must have batch_first, biases and one embed dim of hidden_size for q, k and v")
    p = float(att.dropout)
    _check_dropout(p, seed)
    if L_ > 1 and float(rnn.dropout) != p:
        raise ValueError(f"the stack's dropout {rnn.dropout} differs from the attention's {att.dropout}")
    if tuple(ln.normalized_shape) != (H,) or not ln.elementwise_affine or ln.bias is None:
        raise ValueError(f"layer_norm must be an affine LayerNorm({H}) with a bias")
    if model.fc.in_features != H or model.fc.bias is None or not 1 <= model.fc.out_features <= CNN_TRAIN_MAX_OUT:
        raise ValueError(f"the Linear head needs {H} inputs, a bias and at most {CNN_TRAIN_MAX_OUT} outputs")
    cfg = _lib.RnnConfig()
    cfg.channels, cfg.hidden, cfg.layers, cfg.heads, cfg.n_out = C, H, L_, att.num_heads, model.fc.out_features
    cfg.loss, cfg.permute_input = _loss_code(model.loss), int(bool(model.permute_input))
    cfg.weight_decay, cfg.ln_eps = RNN_WEIGHT_DECAY, float(ln.eps)
    return cfg


def _rnn_tensors(model, seed=None):
    """[(state_dict name, tensor)] of an RNN's parameters in packing order, which is named_parameters()'; no running
    statistics."""
    _rnn_arch(model, seed)
    rnn, att = model.rnn, model.attention
    ps = []
    for l in range(rnn.num_layers):
        ps += [(f"rnn.{k}_l{l}", getattr(rnn, f"{k}_l{l}")) for k in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
    ps += [("layer_norm.weight", model.layer_norm.weight), ("layer_norm.bias", model.layer_norm.bias),
           ("attention.in_proj_weight", att.in_proj_weight), ("attention.in_proj_bias", att.in_proj_bias),
           ("attention.out_proj.weight", att.out_proj.weight), ("attention.out_proj.bias", att.out_proj.bias),
           ("fc.weight", model.fc.weight), ("fc.bias", model.fc.bias)]
    return ps, []


def _rnn_check_stream(n, heads, T, layers, hidden):
    """The random stream indexes the elements of a site with 32 bits.  Inside the other limits (batch 1024, 8 heads,
    512 steps, 4 layers, hidden 128) neither count reaches 2^32; the C entries check the same."""
    if n * heads * T * T >= 1 << 32:
        raise ValueError(f"{n} windows x {heads} heads x {T}^2 attention probabilities: the random stream indexes "
                         "2^32 elements")
    if (layers - 1) * n * T * hidden >= 1 << 32:
        raise ValueError(f"{layers - 1} x {n} x {T} x {hidden} outputs between the layers: the random stream "
                         "indexes 2^32 elements")


def _rnn_batch(model, x, y, what="x", seed=None):
    cfg = _rnn_arch(model, seed)
    x, y, shape = _batch_of(x, y, what)
    if isinstance(x, ShiftedWindows) and not model.permute_input:
        raise ValueError("a window source gives [n, channels, width]: it needs permute_input=True")
    n, (C, T) = shape[0], (shape[1:] if model.permute_input else shape[:0:-1])
    if not 1 <= n <= CNN_TRAIN_MAX_BATCH:
        raise ValueError(f"{n} windows: the trainer's limit is 1..{CNN_TRAIN_MAX_BATCH} (one full batch)")
    if not 1 <= T <= RNN_TRAIN_MAX_STEPS:
        raise ValueError(f"input_size {T}: the trainer's limit is 1..{RNN_TRAIN_MAX_STEPS} (the window is the "
                         "sequence)")
    if C != cfg.channels or y.shape[1] != cfg.n_out:
        raise ValueError(f"{what} {shape} / y {tuple(y.shape)} do not fit a model of {cfg.channels} channels and "
                         f"{cfg.n_out} outputs")
    _rnn_check_stream(n, cfg.heads, T, cfg.layers, cfg.hidden)
    cfg.width = T
    return x, y, cfg


_RNN = SimpleNamespace(
    batch=_rnn_batch, tensors=_rnn_tensors, net=lambda model: model, device_rates=_rnn_device_rows, rates=rnn_rates,
    c_workspace="ofp_rnn_loss_grads_random_workspace_bytes", c_train="ofp_rnn_train", c_grads="ofp_rnn_loss_grads",
    stats=False, after_fit=lambda model, epochs: None, dropout=lambda net: float(net.attention.dropout))


def rnn_train_workspace_bytes(model, n, n_val=0, input_size=256, seed=None):
    """Bytes of GPU work space ``fit_rnn`` asks for at n training and n_val validation windows of `input_size` samples
    (the plan of ofp_rnn_train_stretch; nothing runs on the GPU)."""
    cfg = _rnn_arch(model, seed)
    cfg.width = int(input_size)
    rnd, _k = _train_random(float(model.attention.dropout), seed)
    nbytes = int(_lib.lib().ofp_rnn_train_stretch_workspace_bytes(
        ctypes.byref(cfg), int(n), int(n_val), ctypes.byref(rnd) if rnd is not None else None, 0))
    if nbytes < 0:
        raise ValueError(_lib.last_error())
    return nbytes


def rnn_loss_and_grads_device(model, x, y, seed=None, epoch=0):
    """Loss (``model.loss``) and the gradient of every parameter of an RNN for the full batch x [n, channels,
    input_size] ([n, input_size, channels] with permute_input=False), y [n, outputs], in training mode, by the trainer's
    own forward and backward kernels.  With a seed both dropouts are applied as epoch `epoch` of ``fit_rnn(...,
    seed=seed)`` applies them (``rnn_layer_dropout_mask_device`` between the layers, ``attention_dropout_mask_device``
    on the probabilities).  Returns (loss, {state_dict name: gradient}) on the GPU."""
    return _loss_and_grads(_RNN, model, x, y, seed, epoch)


def fit_rnn(model, x, y, *, x_val=None, y_val=None, max_epochs=1000, min_epochs=0, patience=None, seed=None):
    """Train an ``RNN`` in place with the reference's recipe (model.py:265-307): the whole of x [n, channels,
    input_size] ([n, input_size, channels] with permute_input=False) / y [n, outputs] is one batch; every epoch is one
    training-mode forward, ``model.loss`` (F.l1_loss or F.mse_loss), backward and one NAdam step with weight decay 1e-4
    in torch's coupled form (g + 1e-4 p enters the moments) at the learning rate of CosineAnnealingLR(3000) starting
    from ``model.lr`` (``rnn_rates``); then, with a validation set, an eval-mode forward of x_val and its L1 loss.  The
    contract, the stop rule and the returned record are ``fit_cnn``'s: trained in place, left in eval mode, a fresh
    optimiser state per call; one epoch is one launch of a captured graph of HIP kernels (csrc/ofp_rnn_train.hip;
    OFP_RNN_GRAPH=nodes in the environment launches the kernels one by one).

    The window is the sequence: ``input_size`` time steps of ``channels`` features, read in place with the strides
    ``permute_input`` asks for.  ``seed`` opts into this package's own random stream as in ``fit_cnn``: nn.GRU's dropout
    on the output of every layer but the last (site 4; ``rnn_layer_dropout_mask_device``) and the attention's dropout on
    its softmax probabilities [n, heads, T, T] (site 3; ``attention_dropout_mask_device``), both at ``dropout_rate``
    and scaled by 1 / (1 - p), neither in the validation forward.  ``x`` may be a ``data.ShiftedWindows`` /
    ``StretchedWindows`` as for ``fit_cnn`` (with permute_input=True, the layout those give).

    ValueError, before anything runs on the GPU: rnn_type 'LSTM' or 'RNN', a bidirectional stack,
    share_input_weights=True, batch_first=False, bias=False; num_layers outside 1..4, hidden_size outside 1..128 or not
    divisible by num_heads (1..8), more than 8 channels, input_size above 512, a batch above 1024, more than 16
    outputs; dropout_rate > 0 without a seed, dropout_rate >= 1; a window source with permute_input=False, as x_val, or
    shifting or stretching without a seed; n * heads * input_size^2 or (num_layers - 1) * n * input_size * hidden_size
    of 2^32 or more (the random stream indexes elements with 32 bits); a loss other than F.l1_loss / F.mse_loss."""
    return _fit(_RNN, model, x, y, x_val, y_val, max_epochs, min_epochs, patience, seed)


def layernorm_train_forward(x, gamma, beta, eps=1e-5, *, out=None):
    """nn.LayerNorm over the last axis in training form (ofp_layernorm_train_forward) on float32 CUDA tensors: x [rows,
    E] (E <= 128), gamma, beta [E] -> (y [rows, E], mean [rows], rstd [rows] = 1 / sqrt(biased variance + eps));
    ``out=(y, mean, rstd)`` are preallocated outputs."""
    R_, E = x.shape
    _f32_cuda("x", x, (R_, E)), _f32_cuda("gamma", gamma, (E,)), _f32_cuda("beta", beta, (E,))
    if not (1 <= R_ <= RNN_TRAIN_MAX_ROWS and 1 <= E <= RNN_TRAIN_MAX_HIDDEN and eps > 0):
        raise ValueError(f"{R_} rows of {E}, eps {eps}: beyond the LayerNorm kernels' limits (2^20 rows, width "
                         f"{RNN_TRAIN_MAX_HIDDEN}, eps > 0)")
    y, mean, rstd = _outs(x.device, out or (None,) * 3, [(R_, E), (R_,), (R_,)])
    check(_lib.lib().ofp_layernorm_train_forward(x.data_ptr(), R_, E, gamma.data_ptr(), beta.data_ptr(), float(eps),
                                                 y.data_ptr(), mean.data_ptr(), rstd.data_ptr(), _stream(x.device)),
          "ofp_layernorm_train_forward")
    return y, mean, rstd


def layernorm_train_backward(x, gamma, mean, rstd, dy, *, out=None):
    """Backward of layernorm_train_forward (ofp_layernorm_train_backward): dy [rows, E] -> (dx [rows, E], dgamma [E],
    dbeta [E]); ``out=`` are those three, preallocated."""
    R_, E = x.shape
    _f32_cuda("x", x, (R_, E)), _f32_cuda("gamma", gamma, (E,)), _f32_cuda("dy", dy, (R_, E))
    _f32_cuda("mean", mean, (R_,)), _f32_cuda("rstd", rstd, (R_,))
    L = _lib.lib()
    ws_bytes = int(L.ofp_layernorm_train_backward_workspace_bytes(R_, E))
    if ws_bytes < 0:
        raise ValueError(f"{R_} rows of {E}: beyond the LayerNorm kernels' limits (2^20 rows, width "
                         f"{RNN_TRAIN_MAX_HIDDEN})")
    dx, dgamma, dbeta = _outs(x.device, out or (None,) * 3, [(R_, E), (E,), (E,)])
    ws = _workspace(ws_bytes, x.device)
    check(L.ofp_layernorm_train_backward(x.data_ptr(), R_, E, gamma.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
                                         dy.data_ptr(), dx.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(),
                                         ws.data_ptr(), ws_bytes, _stream(x.device)), "ofp_layernorm_train_backward")
    return dx, dgamma, dbeta


def _stack_args(x, params_per_layer, permuted):
    """(n, T, F, H, L, the stack's parameters packed) of a stand-alone GRU stack call; x is [n, T, F], or [n, F, T]
    with permuted=True."""
    if not (x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and x.dim() == 3):
        raise ValueError("x must be a contiguous float32 GPU tensor [n, T, F] ([n, F, T] with permuted=True)")
    n, T, F_ = (x.shape[0], x.shape[2], x.shape[1]) if permuted else x.shape
    L_ = len(params_per_layer)
    if L_ < 1:
        raise ValueError("params_per_layer is empty")
    H = params_per_layer[0][1].shape[1]
    for l, (w_ih, w_hh, b_ih, b_hh) in enumerate(params_per_layer):
        _f32_cuda(f"w_ih of layer {l}", w_ih, (3 * H, H if l else F_)), _f32_cuda(f"w_hh of layer {l}", w_hh, (3 * H, H))
        _f32_cuda(f"b_ih of layer {l}", b_ih, (3 * H,)), _f32_cuda(f"b_hh of layer {l}", b_hh, (3 * H,))
    flat = torch.cat([t.reshape(-1) for layer in params_per_layer for t in layer])
    return int(n), int(T), int(F_), int(H), L_, flat


def rnn_gru_train_forward(x, params_per_layer, p=0.0, seed=None, epoch=0, *, permuted=False, out=None):
    """An L-layer batch_first GRU stack with zero initial states in training form (ofp_rnn_gru_train_forward) on
    float32 CUDA tensors: x [n, T, F] (or the window as stored, [n, F, T], with permuted=True; F <= 8, T <= 512),
    params_per_layer = [(w_ih, w_hh, b_ih, b_hh)] per layer -> (seqs [L, n, T, H], every layer's output before its
    dropout, seqs[-1] being the stack's; gates [L, n, T, 4H]).  With p > 0 and a seed the output of every layer but the
    last is dropped by site 4 of the random stream (``rnn_layer_dropout_mask_device``) before the next layer reads it.
    ``out=(seqs, gates)`` are preallocated outputs."""
    n, T, F_, H, L_, flat = _stack_args(x, params_per_layer, permuted)
    rnd = _attention_random(p, seed, epoch)
    L = _lib.lib()
    ws_bytes = int(L.ofp_rnn_gru_train_forward_workspace_bytes(n, T, F_, H, L_))
    if ws_bytes < 0:
        raise ValueError(_lib.last_error())
    seqs, gates = _outs(x.device, out or (None,) * 2, [(L_, n, T, H), (L_, n, T, 4 * H)])
    ws = _workspace(ws_bytes, x.device)
    check(L.ofp_rnn_gru_train_forward(x.data_ptr(), int(bool(permuted)), n, T, F_, H, L_, flat.data_ptr(),
                                      ctypes.byref(rnd) if rnd is not None else None, seqs.data_ptr(),
                                      gates.data_ptr(), ws.data_ptr(), ws_bytes, _stream(x.device)),
          "ofp_rnn_gru_train_forward")
    return seqs, gates


def rnn_gru_train_backward(x, params_per_layer, seqs, gates, dseq, p=0.0, seed=None, epoch=0, *, permuted=False,
                           out=None):
    """Back-propagation through time and through the layers of rnn_gru_train_forward with the same p, seed and epoch
    (ofp_rnn_gru_train_backward): dseq [n, T, H] = the gradient at the last layer's output -> [(dw_ih, dw_hh, db_ih,
    db_hh)] per layer, views of one tensor packed like the parameters (``out=``: that tensor, preallocated, of as many
    elements as the parameters have).  The input x gets no gradient: it is the window."""
    n, T, F_, H, L_, flat = _stack_args(x, params_per_layer, permuted)
    _f32_cuda("seqs", seqs, (L_, n, T, H)), _f32_cuda("gates", gates, (L_, n, T, 4 * H))
    _f32_cuda("dseq", dseq, (n, T, H))
    rnd = _attention_random(p, seed, epoch)
    L = _lib.lib()
    ws_bytes = int(L.ofp_rnn_gru_train_backward_workspace_bytes(n, T, F_, H, L_))
    if ws_bytes < 0:
        raise ValueError(_lib.last_error())
    (grads,) = _outs(x.device, (out,), [(flat.numel(),)])
    ws = _workspace(ws_bytes, x.device)
    check(L.ofp_rnn_gru_train_backward(x.data_ptr(), int(bool(permuted)), n, T, F_, H, L_, flat.data_ptr(),
                                       ctypes.byref(rnd) if rnd is not None else None, seqs.data_ptr(),
                                       gates.data_ptr(), dseq.data_ptr(), grads.data_ptr(), ws.data_ptr(), ws_bytes,
                                       _stream(x.device)), "ofp_rnn_gru_train_backward")
    per_layer, o = [], 0
    for layer in params_per_layer:
        pieces = []
        for t in layer:
            pieces.append(grads[o:o + t.numel()].reshape(t.shape))
            o += t.numel()
        per_layer.append(tuple(pieces))
    return per_layer


def rnn_attention_train_forward(h, in_proj_w, in_proj_b, num_heads, p=0.0, seed=None, epoch=0, *, out=None):
    """``attention_mean_train_forward`` at the RNN trainer's capacity, T <= 512 (ofp_rnn_attention_train_forward)."""
    n, T, E = h.shape
    _f32_cuda("h", h, (n, T, E)), _f32_cuda("in_proj_w", in_proj_w, (3 * E, E)), _f32_cuda("in_proj_b", in_proj_b, (3 * E,))
    rnd = _attention_random(p, seed, epoch)
    L = _lib.lib()
    ws_bytes = int(L.ofp_rnn_attention_train_forward_workspace_bytes(n, T, E, num_heads))
    if ws_bytes < 0:
        raise ValueError(_lib.last_error())
    ctx, qkv, probs = _outs(h.device, out or (None,) * 3, [(n, E), (n, T, 3 * E), (n, num_heads, T, T)])
    ws = _workspace(ws_bytes, h.device)
    check(L.ofp_rnn_attention_train_forward(h.data_ptr(), n, T, E, num_heads, in_proj_w.data_ptr(),
                                            in_proj_b.data_ptr(), ctypes.byref(rnd) if rnd is not None else None,
                                            qkv.data_ptr(), probs.data_ptr(), ctx.data_ptr(), ws.data_ptr(), ws_bytes,
                                            _stream(h.device)), "ofp_rnn_attention_train_forward")
    return ctx, qkv, probs


def rnn_attention_train_backward(h, in_proj_w, num_heads, qkv, probs, dctx, p=0.0, seed=None, epoch=0, *, out=None):
    """``attention_mean_train_backward`` at the RNN trainer's capacity, T <= 512 (ofp_rnn_attention_train_backward)."""
    n, T, E = h.shape
    _f32_cuda("h", h, (n, T, E)), _f32_cuda("in_proj_w", in_proj_w, (3 * E, E)), _f32_cuda("qkv", qkv, (n, T, 3 * E))
    _f32_cuda("probs", probs, (n, num_heads, T, T)), _f32_cuda("dctx", dctx, (n, E))
    rnd = _attention_random(p, seed, epoch)
    L = _lib.lib()
    ws_bytes = int(L.ofp_rnn_attention_train_backward_workspace_bytes(n, T, E, num_heads))
    if ws_bytes < 0:
        raise ValueError(_lib.last_error())
    outs = _outs(h.device, out or (None,) * 3, [(n, T, E), (3 * E, E), (3 * E,)])
    ws = _workspace(ws_bytes, h.device)
    check(L.ofp_rnn_attention_train_backward(h.data_ptr(), n, T, E, num_heads, in_proj_w.data_ptr(), qkv.data_ptr(),
                                             probs.data_ptr(), dctx.data_ptr(),
                                             ctypes.byref(rnd) if rnd is not None else None,
                                             *(t.data_ptr() for t in outs), ws.data_ptr(), ws_bytes,
                                             _stream(h.device)), "ofp_rnn_attention_train_backward")
    return tuple(outs)


def rnn_layer_dropout_mask_device(seed, epoch, layers, n, T, H, p, device=0, *, out=None):
    """The dropout masks between the recurrent layers of epoch `epoch` of ``fit_rnn(..., seed=seed)``: float32 GPU
    tensor [layers, n, T, H] of 0 (dropped) and float32(1 / (1 - p)) (kept), site 4 of the random stream
    (``ofp_rnn_layer_dropout_mask``); `layers` counts the layers whose output is dropped, num_layers - 1."""
    seed = check_seed(seed)
    layers, n, T, H = int(layers), int(n), int(T), int(H)
    if not 0 <= p < 1 or min(layers, n, T, H) < 1 or int(epoch) < 0 or layers * n * T * H > 1 << 32:
        raise ValueError("rnn_layer_dropout_mask_device needs 0 <= p < 1, layers, n, T, H >= 1 with at most 2^32 "
                         "elements, and epoch >= 0")
    if out is not None:
        dev = _f32_cuda("out", out, (layers, n, T, H)).device
    else:
        dev = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
    _lib.require_gpu(dev.index or 0)
    if out is None:
        out = torch.empty((layers, n, T, H), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        check(_lib.lib().ofp_rnn_layer_dropout_mask(seed, int(epoch), layers, n, T, H, float(p), out.data_ptr(),
                                                    _stream(dev)), "ofp_rnn_layer_dropout_mask")
    return out
