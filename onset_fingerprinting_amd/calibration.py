"""``calibration.FCNN`` (calibration.py:463-560) with its forward pass on MI355X.

The module builds the same ``network`` Sequential as the reference so that a
reference ``state_dict`` (``network.{k}.weight`` ...) loads unchanged
(realtime/config.py:105-107); ``forward`` is inference-only and runs the WHOLE
network as one HIP kernel (``ofp_mlp_forward``: every layer a chain of fp32 MFMA
tiles + bias + folded eval-mode BatchNorm1d + activation, the activations staying
in LDS, csrc/ofp_mlp.h); a network too large for the LDS runs layer by layer
through ``ofp_dense`` -- bit-identical either way.

``train_location_model`` (calibration.py:685-754) and ``optimize_positions``
(:563-682) run on the GPU too: the whole optimisation -- every epoch's forward,
loss, early-stop test, backward, gradient clipping and Adam step -- is one launch
by one workgroup per problem (csrc/ofp_train.hip), so ``train_location_models_device``
and ``optimize_positions_device`` fit M independent problems in the time of one.
``calibration_locations`` (:423-460) is the host helper that makes their inputs.
Out of scope: ``tdoa_calib_loss*``, ``optimize_C`` and ``calibrate``, scipy ``TNC``
drivers around a Python loop over some 40 hits with no data-parallel work in them.
"""
import ctypes
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

from . import _lib
from ._lib import check

ACT_CODES = {nn.Identity: 0, nn.ReLU: 1, nn.SiLU: 2, nn.LeakyReLU: 3, nn.ELU: 4, nn.Tanh: 5}


def _stream(dev):
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def dense_forward(x, weight, bias, scale, shift, act_code, out=None):
    """One fused layer on the GPU: act((x @ W^T + b) * scale + shift)."""
    L = _lib.lib()
    n, fin = x.shape
    fout = weight.shape[0]
    if out is None:
        out = torch.empty((n, fout), dtype=torch.float32, device=x.device)
    p = lambda t: t.data_ptr() if t is not None else None
    check(L.ofp_dense(x.data_ptr(), n, fin, fout, weight.data_ptr(), p(bias), p(scale), p(shift), act_code,
                      out.data_ptr(), _stream(x.device)), "ofp_dense")
    return out


class DeviceMLP:
    """Owner of an ``ofp_mlp`` handle (include/onsetfp.h): the folded layers of one network,
    resident on the current device."""

    def __init__(self, plan):
        """plan: list of (W [out, in], b, scale, shift, act_code) with CPU float32 tensors / None."""
        L = _lib.lib()
        n = len(plan)
        dims = [int(plan[0][0].shape[1])] + [int(w.shape[0]) for (w, *_r) in plan]
        self.n_in, self.n_out = dims[0], dims[-1]
        keep = []

        def arr(ts):
            out = (ctypes.c_void_p * n)()
            for i, t in enumerate(ts):
                if t is not None:
                    a = np.ascontiguousarray(t.detach().cpu().numpy(), dtype=np.float32)
                    keep.append(a)
                    out[i] = a.ctypes.data
            return out

        h = ctypes.c_void_p()
        check(L.ofp_mlp_create(n, (ctypes.c_int32 * (n + 1))(*dims), (ctypes.c_int32 * n)(*[pl[4] for pl in plan]),
                               arr([pl[0] for pl in plan]), arr([pl[1] for pl in plan]), arr([pl[2] for pl in plan]),
                               arr([pl[3] for pl in plan]), ctypes.byref(h)), "ofp_mlp_create")
        self.handle = h
        self.lds_bytes = int(L.ofp_mlp_lds_bytes(h))
        self.fits = self.lds_bytes <= 160 * 1024

    def forward(self, x, out=None):
        n = x.shape[0]
        if out is None:
            out = torch.empty((n, self.n_out), dtype=torch.float32, device=x.device)
        check(_lib.lib().ofp_mlp_forward(self.handle, x.data_ptr(), n, out.data_ptr(), _stream(x.device)),
              "ofp_mlp_forward")
        return out

    def __del__(self):
        try:
            if getattr(self, "handle", None):
                _lib.lib().ofp_mlp_destroy(self.handle)
                self.handle = None
        except Exception:
            pass


class FCNN(nn.Module):
    def __init__(self, input_size: int, output_size: int, hidden_layers=[10, 10, 10], activation=nn.ReLU,
                 dropout: float = 0.0, batch_norm: bool = True, l2_reg: float = 0.0, eye_init=False,
                 eye_noise_floor=0.01, bias=True) -> None:
        super().__init__()
        if activation not in ACT_CODES:
            raise ValueError(f"activation {activation} has no HIP implementation "
                             f"(supported: {[a.__name__ for a in ACT_CODES]})")
        self.l2_reg = l2_reg
        self._act_code = ACT_CODES[activation]
        sizes = [input_size] + list(hidden_layers)
        mods = []
        for a, b in zip(sizes[:-1], sizes[1:]):
            lin = nn.Linear(a, b, bias=bias)
            if eye_init:
                self.init_eye_weights(lin, eye_noise_floor)
            mods.append(lin)
            if batch_norm:
                mods.append(nn.BatchNorm1d(b))
            mods.append(activation())
            if dropout > 0:
                mods.append(nn.Dropout(p=dropout))
        last = nn.Linear(sizes[-1], output_size, bias=bias)
        if eye_init:
            self.init_eye_weights(last, eye_noise_floor)
        mods.append(last)
        self.network = nn.Sequential(*mods)
        self._plan = None
        self._plan_key = None
        self._mlp = None

    def init_eye_weights(self, layer, noise_floor=0.001):
        noise = torch.randn(layer.out_features, layer.in_features) * noise_floor
        layer.weight.data = torch.eye(layer.out_features, layer.in_features) + noise

    def _build_plan(self, device):
        """(W, b, scale, shift, act) per Linear, BatchNorm folded with running stats."""
        plan = []
        mods = list(self.network)
        i = 0
        while i < len(mods):
            lin = mods[i]
            assert isinstance(lin, nn.Linear)
            scale = shift = None
            act = 0
            j = i + 1
            if j < len(mods) and isinstance(mods[j], nn.BatchNorm1d):
                bn = mods[j]
                inv = (bn.running_var.double() + bn.eps).rsqrt()
                g = bn.weight.double() if bn.affine else torch.ones_like(inv)
                be = bn.bias.double() if bn.affine else torch.zeros_like(inv)
                scale = (g * inv).float()
                shift = (be - bn.running_mean.double() * g * inv).float()
                j += 1
            if j < len(mods) and type(mods[j]) in ACT_CODES:
                act = ACT_CODES[type(mods[j])]
                j += 1
            if j < len(mods) and isinstance(mods[j], nn.Dropout):
                j += 1  # identity in eval mode
            to = lambda t: None if t is None else t.detach().to(device, torch.float32).contiguous()
            plan.append((to(lin.weight), to(lin.bias), to(scale), to(shift), act))
            i = j
        return plan

    def _versions(self, dev):
        # the folded device copy is rebuilt whenever any parameter or buffer is replaced or changed
        # in place (load_state_dict on any submodule, init_eye_weights, optimiser steps ...)
        ts = list(self.parameters()) + list(self.buffers())
        return (str(dev),) + tuple((id(t), t.data_ptr(), t._version) for t in ts)

    def device_mlp(self, device=0):
        """The network as an ``ofp_mlp`` handle on `device` (rebuilt when the parameters changed);
        also what the fused STFT->mel->classifier kernel and the per-hop session take."""
        dev = device if isinstance(device, torch.device) else torch.device("cuda", int(device))
        key = self._versions(dev)
        if self._plan is None or self._plan_key != key:
            with torch.cuda.device(dev):
                self._plan = self._build_plan(dev)
                self._mlp = DeviceMLP(self._build_plan(torch.device("cpu")))
            self._plan_key = key
        return self._mlp

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """x [batch, input_size] -> [batch, output_size].  Inference only: BatchNorm uses its running
        statistics and Dropout is the identity, so a module in training mode that has either is
        refused (the reference would use batch statistics there, calibration.py:520-527)."""
        if self.training and any(isinstance(m, (nn.BatchNorm1d, nn.Dropout)) for m in self.network):
            raise RuntimeError("FCNN.forward on the GPU is inference-only: call .eval() first (BatchNorm1d / Dropout "
                               "in training mode are not implemented)")
        dev = x.device if x.is_cuda else torch.device("cuda", 0)
        _lib.require_gpu(dev.index or 0)
        mlp = self.device_mlp(dev)
        h = x.detach().to(dev, torch.float32).contiguous()
        if mlp.fits:
            h = mlp.forward(h)
        else:  # too large for the LDS: the same arithmetic, one launch per layer
            for (w, b, sc, sh, act) in self._plan:
                h = dense_forward(h, w, b, sc, sh, act)
        return h if x.is_cuda else h.cpu()

    def forward_layerwise(self, x: torch.Tensor) -> torch.Tensor:
        """The same forward pass as a chain of ``ofp_dense`` launches (what round 1 shipped): kept as
        the bit-for-bit cross-check of the fused kernel."""
        dev = x.device if x.is_cuda else torch.device("cuda", 0)
        self.device_mlp(dev)
        h = x.detach().to(dev, torch.float32).contiguous()
        for (w, b, sc, sh, act) in self._plan:
            h = dense_forward(h, w, b, sc, sh, act)
        return h if x.is_cuda else h.cpu()

    def l2_loss(self) -> torch.Tensor:
        if self.l2_reg == 0.0:
            return torch.tensor(0.0)
        return self.l2_reg * sum(torch.sum(p ** 2) for p in self.parameters())

    def call_np(self, lags) -> np.ndarray:
        """calibration.py:552-560: one sample in, one numpy row out."""
        with torch.no_grad():
            return self(torch.tensor([lags], dtype=torch.float32)).numpy()[0]


# ---- calibration on the GPU: train_location_model, optimize_positions ------------------------------------------

LOSS_CODES = {F.l1_loss: 0, F.mse_loss: 1}
TRAIN_MAX_LAYERS, TRAIN_MAX_WIDTH, TRAIN_MAX_BATCH, TDOA_MAX_SOUNDS = 8, 128, 1024, 4096
_ACT_CLASSES = {code: cls for cls, code in ACT_CODES.items()}


def calibration_locations(n_lugs, n_each, radius, add_z=None, clockwise=False):
    """calibration.py:423-460: (radius, angle in degrees[, z]) of calibration hits next to the drum's lugs, lug by
    lug; `n_each` hits at every lug, or a list with one count per lug."""
    angles = np.repeat(np.arange(0, 360, int(360 / n_lugs)), n_each)
    if not clockwise:
        angles = 360 - angles
    columns = [np.full(len(angles), radius), angles]
    if add_z is not None:
        assert isinstance(add_z, int), f"add_z needs to be an integer! (given: {add_z} ({type(add_z)}))"
        columns.append(np.full(len(angles), add_z))
    return list(zip(*columns))


def _loss_code(lossfun):
    for fn, code in LOSS_CODES.items():
        if lossfun is fn:
            return code
    raise ValueError(f"lossfun {lossfun!r} has no HIP implementation (supported: F.l1_loss, F.mse_loss)")


def _adam_scalars(t):
    """torch's single-tensor Adam computes these as Python doubles (optim/adam.py)."""
    return 1 - 0.9 ** t, (1 - 0.999 ** t) ** 0.5


@functools.lru_cache(maxsize=1024)
def location_model_rates(lr, num_epochs):
    """The learning rate train_location_model uses at every epoch: CosineAnnealingLR with T_max = num_epochs / 10,
    run past T_max, by torch's own scheduler stepped on a dummy parameter.  float64 [num_epochs]."""
    p = nn.Parameter(torch.zeros(1))
    opt = torch.optim.Adam([{"params": [p], "lr": lr}])
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, num_epochs / 10)
    opt.step()
    rates = np.empty(num_epochs, np.float64)
    for e in range(num_epochs):
        rates[e] = opt.param_groups[0]["lr"]
        sched.step()
    rates.setflags(write=False)
    return rates


def location_model_rate_table(lr, num_epochs):
    """float32 [num_epochs][2]: Adam's step size lr_t / (1 - beta1^t) and sqrt(1 - beta2^t), each rounded once."""
    rates = location_model_rates(float(lr), int(num_epochs))
    table = np.empty((num_epochs, 2), np.float32)
    for e in range(num_epochs):
        bc1, bc2_sqrt = _adam_scalars(e + 1)
        table[e] = rates[e] / bc1, bc2_sqrt
    return table


@functools.lru_cache(maxsize=1024)
def _position_tables(lr, num_epochs):
    lrs = torch.tensor([2e-3, 1e-4, 0.1], dtype=torch.float32) * lr
    opt = torch.optim.Adam([{"params": [nn.Parameter(torch.zeros(1))], "lr": lrs[k]} for k in range(3)])
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, num_epochs)
    opt.step()
    rates = np.empty((num_epochs, 3), np.float64)
    table = np.empty((num_epochs, 4), np.float32)
    for e in range(num_epochs):
        bc1, bc2_sqrt = _adam_scalars(e + 1)
        for k, group in enumerate(opt.param_groups):
            rates[e, k] = float(group["lr"])
            table[e, k] = float(group["lr"] / bc1)  # a float32 tensor divided in float32, as Adam does
        table[e, 3] = bc2_sqrt
        sched.step()
    rates.setflags(write=False)
    table.setflags(write=False)
    return rates, table


def position_rates(lr, num_epochs):
    """The three learning rates of optimize_positions (sensors, sounds, C) at every epoch: lr times (2e-3, 1e-4,
    0.1) held as float32 tensors, CosineAnnealingLR with T_max = num_epochs.  float64 [num_epochs][3]."""
    return _position_tables(float(lr), int(num_epochs))[0]


def _fcnn_arch(model):
    """(dims, act code, batch_norm, bias, linears, batch norms) of an FCNN; ValueError for what the trainer cannot
    run."""
    mods = list(model.network)
    if any(isinstance(m, nn.Dropout) and m.p > 0 for m in mods):
        raise ValueError("dropout > 0 cannot be trained on the GPU: torch's dropout stream cannot be matched")
    lins = [m for m in mods if isinstance(m, nn.Linear)]
    bns = [m for m in mods if isinstance(m, nn.BatchNorm1d)]
    if bns and len(bns) != len(lins) - 1:
        raise ValueError("BatchNorm1d must follow every hidden Linear or none")
    bias = lins[0].bias is not None
    if any((l.bias is not None) != bias for l in lins):
        raise ValueError("every Linear must have a bias or none")
    dims = [lins[0].in_features] + [l.out_features for l in lins]
    if len(lins) > TRAIN_MAX_LAYERS:
        raise ValueError(f"{len(lins)} linear layers: the trainer's limit is {TRAIN_MAX_LAYERS}")
    if max(dims) > TRAIN_MAX_WIDTH:
        raise ValueError(f"layer width {max(dims)}: the trainer's limit is {TRAIN_MAX_WIDTH}")
    return dims, model._act_code, bool(bns), bias, lins, bns


def _pack(model):
    """Parameters and running statistics as the two flat float32 vectors of ofp_fcnn_train (include/onsetfp.h)."""
    dims, act, bn, bias, lins, bns = _fcnn_arch(model)
    ps, st = [], []
    for i, lin in enumerate(lins):
        ps.append(lin.weight)
        if bias:
            ps.append(lin.bias)
        if bn and i < len(bns):
            ps += [bns[i].weight, bns[i].bias]
            st += [bns[i].running_mean, bns[i].running_var]
    flat = lambda ts: (torch.cat([t.detach().reshape(-1).to("cpu", torch.float32) for t in ts]) if ts
                       else torch.zeros(0))
    return flat(ps), flat(st)


def _param_names(model):
    dims, act, bn, bias, lins, bns = _fcnn_arch(model)
    index = {id(m): k for k, m in enumerate(model.network)}
    names = []
    for i, lin in enumerate(lins):
        names.append((f"network.{index[id(lin)]}.weight", lin.weight.shape))
        if bias:
            names.append((f"network.{index[id(lin)]}.bias", lin.bias.shape))
        if bn and i < len(bns):
            names.append((f"network.{index[id(bns[i])]}.weight", bns[i].weight.shape))
            names.append((f"network.{index[id(bns[i])]}.bias", bns[i].bias.shape))
    return names


def _check_batch(n, bn, hidden):
    if n < 1 or n > TRAIN_MAX_BATCH:
        raise ValueError(f"{n} hits: the trainer's limit is 1..{TRAIN_MAX_BATCH}")
    if bn and hidden and n < 2:
        raise ValueError("Expected more than 1 value per channel when training (BatchNorm1d with one hit)")


def _device_of(t):
    return t.device if isinstance(t, torch.Tensor) and t.is_cuda else torch.device("cuda", 0)


def _i32s(vals):
    return (ctypes.c_int32 * len(vals))(*vals)


def _per_problem(v, M, what):
    vals = [float(x) for x in (v.reshape(-1).tolist() if isinstance(v, (torch.Tensor, np.ndarray)) else
                               (list(v) if isinstance(v, (list, tuple)) else [v]))]
    if len(vals) == 1:
        vals = vals * M
    if len(vals) != M:
        raise ValueError(f"{what}: {len(vals)} values for {M} problems")
    return vals


def _rate_rows(lrs, table_of):
    uniq = sorted(set(lrs))
    row = {v: k for k, v in enumerate(uniq)}
    table = np.stack([table_of(v) for v in uniq])
    return torch.from_numpy(np.ascontiguousarray(table)), torch.tensor([row[v] for v in lrs], dtype=torch.int32)


class TrainedModels:
    """What train_location_models_device returns.  Device tensors: ``params`` [M, n_params] and ``stats``
    [M, n_stats] (packed as include/onsetfp.h describes), ``losses`` [M, num_epochs] (NaN beyond the stop),
    ``epochs`` [M] (losses recorded).  ``model(i)`` is entry i as an FCNN in eval mode, ``errors(i)`` its loss
    curve as the reference's list."""

    def __init__(self, template, params, stats, losses, epochs, tracked):
        self._template, self._tracked = template, tracked
        self.params, self.stats, self.losses, self.epochs = params, stats, losses, epochs

    def __len__(self):
        return self.params.shape[0]

    def errors(self, i):
        n = int(self.epochs[i])
        return [np.asarray(v) for v in self.losses[i, :n].cpu().numpy()]

    def model(self, i):
        dims, act, bn, bias, _l, _b = _fcnn_arch(self._template)
        with torch.random.fork_rng(devices=[]):
            out = FCNN(dims[0], dims[-1], hidden_layers=dims[1:-1], activation=_ACT_CLASSES[act], batch_norm=bn,
                       bias=bias, l2_reg=self._template.l2_reg)
        p, s, n = self.params[i].cpu(), self.stats[i].cpu(), int(self.epochs[i])
        _d, _a, _bn, _bi, lins, bns = _fcnn_arch(out)
        with torch.no_grad():
            o = q = 0
            for k, lin in enumerate(lins):
                ts = [lin.weight] + ([lin.bias] if bias else [])
                if bn and k < len(bns):
                    ts += [bns[k].weight, bns[k].bias]
                    for t in (bns[k].running_mean, bns[k].running_var):
                        t.copy_(s[q:q + t.numel()].reshape(t.shape))
                        q += t.numel()
                    bns[k].num_batches_tracked.fill_(self._tracked[i][k] + n)
                for t in ts:
                    t.copy_(p[o:o + t.numel()].reshape(t.shape))
                    o += t.numel()
        return out.eval()


def train_location_models_device(observed_lags, sound_positions, lr=0.01, lossfun=F.l1_loss, num_epochs=1000,
                                 eps=1e-9, patience=10, *, models=None, n_models=None, **kwargs):
    """M independent train_location_model runs in one launch, one workgroup each.

    observed_lags [M, N, F] (or one shared [N, F]), sound_positions [M, N, >= 2] (or [N, >= 2]; the first two
    columns are the targets), lr a number or M of them; `models`: M FCNNs of one architecture whose parameters are
    the starting points (default: M fresh ``FCNN(F, 2, **kwargs)`` drawn in order from torch's RNG).  Loss,
    num_epochs, eps and patience are shared.  Returns TrainedModels (device tensors; no host round trip per
    epoch)."""
    loss = _loss_code(lossfun)
    if kwargs.get("dropout", 0.0) > 0:
        raise ValueError("dropout > 0 cannot be trained on the GPU: torch's dropout stream cannot be matched")
    x = torch.as_tensor(observed_lags)
    y = torch.as_tensor(sound_positions)
    if x.dim() not in (2, 3) or y.dim() not in (2, 3) or y.shape[-1] < 2 or x.shape[-2] != y.shape[-2]:
        raise ValueError(f"observed_lags {tuple(x.shape)} / sound_positions {tuple(y.shape)}: expected [N, F] and "
                         "[N, >= 2], or with a leading M")
    if models is not None:
        M = len(models)
    elif x.dim() == 3 or y.dim() == 3:
        M = x.shape[0] if x.dim() == 3 else y.shape[0]
    elif isinstance(lr, (list, tuple, np.ndarray, torch.Tensor)) and np.size(lr) > 1:
        M = int(np.size(lr))
    else:
        M = int(n_models or 1)
    for t in (x, y):
        if t.dim() == 3 and t.shape[0] != M:
            raise ValueError(f"{t.shape[0]} batches for {M} problems")
    N, n_in = int(x.shape[-2]), int(x.shape[-1])
    if models is None:
        models = [FCNN(n_in, 2, **kwargs) for _ in range(M)]
    elif kwargs:
        raise ValueError(f"model given: the FCNN arguments {sorted(kwargs)} have no effect")
    dims, act, bn, bias, _l, bns0 = _fcnn_arch(models[0])
    for mdl in models[1:]:
        if _fcnn_arch(mdl)[:4] != (dims, act, bn, bias):
            raise ValueError("the models of one launch must share one architecture")
    if dims[0] != n_in or dims[-1] != 2:
        raise ValueError(f"the model maps {dims[0]} -> {dims[-1]} values; the data needs {n_in} -> 2")
    _check_batch(N, bn, len(dims) > 2)
    lrs = _per_problem(lr, M, "lr")
    num_epochs, patience = int(num_epochs), int(math.ceil(patience))
    if num_epochs < 1:
        raise ValueError("num_epochs must be at least 1")

    dev = _device_of(x)
    _lib.require_gpu(dev.index or 0)
    L = _lib.lib()
    packed = [_pack(mdl) for mdl in models]
    tracked = [[int(b.num_batches_tracked) for b in _fcnn_arch(mdl)[5]] for mdl in models]
    p0 = torch.stack([p for p, _s in packed]).to(dev)
    s0 = torch.stack([s for _p, s in packed]).to(dev)
    xd = x.detach().to(dev, torch.float32).contiguous()
    yd = y.detach()[..., :2].to(dev, torch.float32).contiguous()
    table, rows = _rate_rows(lrs, lambda v: location_model_rate_table(v, num_epochs))
    table, rows = table.to(dev), rows.to(dev)
    params, stats, losses, epochs = _fcnn_train_launch((dims, act, bn, bias), loss, xd, yd, p0, s0, table, rows,
                                                       num_epochs, eps, patience)
    return TrainedModels(models[0], params, stats, losses, epochs, tracked)


def _fcnn_train_launch(arch, loss, xd, yd, p0, s0, table, rows, num_epochs, eps, patience):
    """The one launch of ofp_fcnn_train on prepared device tensors (also what tools/calib_latency.py times)."""
    dims, act, bn, bias = arch
    L, dev = _lib.lib(), p0.device
    M, N = p0.shape[0], xd.shape[-2]
    params, stats = torch.empty_like(p0), torch.empty_like(s0)
    losses = torch.full((M, num_epochs), float("nan"), dtype=torch.float32, device=dev)
    epochs = torch.zeros(M, dtype=torch.int32, device=dev)
    cdims = _i32s(dims)
    ws_bytes = int(L.ofp_fcnn_train_workspace_bytes(len(dims) - 1, cdims, int(bn), int(bias), N, M))
    ws = torch.empty(max(ws_bytes // 4, 1), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        check(L.ofp_fcnn_train(len(dims) - 1, cdims, act, int(bn), int(bias), loss, M, N, xd.data_ptr(),
                               N * dims[0] if xd.dim() == 3 else 0, yd.data_ptr(), N * 2 if yd.dim() == 3 else 0,
                               p0.data_ptr(), s0.data_ptr(), table.data_ptr(), rows.data_ptr(), num_epochs,
                               float(eps), patience, params.data_ptr(), stats.data_ptr(), losses.data_ptr(),
                               epochs.data_ptr(), ws.data_ptr(), ws_bytes, _stream(dev)), "ofp_fcnn_train")
    return params, stats, losses, epochs


def train_location_model(observed_lags, sound_positions, lr=0.01, lossfun=F.l1_loss, num_epochs=1000, eps=1e-9,
                         patience=10, print_every=10, debug=False, *, model=None, **kwargs):
    """calibration.py:685-754 on the GPU: trains ``FCNN(F, 2, **kwargs)`` to map lags to the hit's (x, y) and
    returns ``(model, errors)``.  The whole run is one kernel launch (train_location_models_device with M = 1).
    `model`: an FCNN to start from (left untouched).  The returned model is in eval mode."""
    x = torch.as_tensor(observed_lags)
    if x.dim() != 2:
        raise ValueError(f"observed_lags {tuple(x.shape)}: expected [N, F]")
    run = train_location_models_device(x, sound_positions, lr, lossfun, num_epochs, eps, patience,
                                       models=None if model is None else [model], **kwargs)
    errors = run.errors(0)
    out = run.model(0)
    if x.is_cuda:
        out = out.to(x.device)
    updates = _updates_of(errors, eps, int(math.ceil(patience)))
    for e in range(updates):
        if e % print_every == 0:
            print(f"Epoch {e}, Loss {float(errors[e])}")
    print(f"Epoch {len(errors) - 1}, Loss {float(errors[-1])}")
    if debug:
        with torch.no_grad():
            print(out(x.float())[:10], "\n", torch.as_tensor(sound_positions)[:10])
    return out, errors


def _updates_of(errors, eps, patience):
    """Number of optimiser steps behind a recorded loss curve: the early-stop rule replayed in float32."""
    last, counter, eps = np.float32(np.inf), 0, np.float32(eps)
    for e, v in enumerate(errors):
        if np.float32(v) < last - eps:
            last, counter = np.float32(v), 0
        elif counter < patience:
            counter += 1
        else:
            return e
    return len(errors)


def fcnn_loss_and_grads_device(model, x, y, lossfun=F.l1_loss):
    """Loss and the unclipped gradient of every parameter of `model` for the full batch (x [N, F], y [N, out]),
    with BatchNorm on batch statistics, by the trainer's own forward and backward pass (one epoch of
    k_fcnn_train, csrc/ofp_train.hip).  Returns (loss, {state_dict name: gradient}) on the GPU."""
    loss = _loss_code(lossfun)
    dims, act, bn, bias, _l, _b = _fcnn_arch(model)
    x, y = torch.as_tensor(x), torch.as_tensor(y)
    if x.dim() != 2 or y.dim() != 2 or x.shape[0] != y.shape[0] or x.shape[1] != dims[0] or y.shape[1] != dims[-1]:
        raise ValueError(f"x {tuple(x.shape)} / y {tuple(y.shape)} do not fit a {dims[0]} -> {dims[-1]} model")
    N = int(x.shape[0])
    _check_batch(N, bn, len(dims) > 2)
    dev = _device_of(x)
    _lib.require_gpu(dev.index or 0)
    L = _lib.lib()
    p0 = _pack(model)[0].to(dev)
    xd, yd = x.detach().to(dev, torch.float32).contiguous(), y.detach().to(dev, torch.float32).contiguous()
    out_loss = torch.empty(1, dtype=torch.float32, device=dev)
    grads = torch.empty_like(p0)
    cdims = _i32s(dims)
    ws_bytes = int(L.ofp_fcnn_train_workspace_bytes(len(dims) - 1, cdims, int(bn), int(bias), N, 1))
    ws = torch.empty(max(ws_bytes // 4, 1), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        check(L.ofp_fcnn_loss_grads(len(dims) - 1, cdims, act, int(bn), int(bias), loss, 1, N, xd.data_ptr(), 0,
                                    yd.data_ptr(), 0, p0.data_ptr(), out_loss.data_ptr(), grads.data_ptr(),
                                    ws.data_ptr(), ws_bytes, _stream(dev)), "ofp_fcnn_loss_grads")
    named, o = {}, 0
    for name, shape in _param_names(model):
        n = int(np.prod(shape))
        named[name] = grads[o:o + n].reshape(shape)
        o += n
    return out_loss[0], named


def fcnn_train_lds_bytes(model, n):
    """Bytes of parameters, Adam moments and activations one training problem keeps on chip
    (ofp_fcnn_train_lds_bytes); above 160 KiB less 512 B they go to a global work space."""
    dims, act, bn, bias, _l, _b = _fcnn_arch(model)
    return int(_lib.lib().ofp_fcnn_train_lds_bytes(len(dims) - 1, _i32s(dims), int(bn), int(bias), int(n)))


class PositionFits:
    """What optimize_positions_device returns, all on the GPU: ``sensors`` [M, 4, 3], ``sounds`` [M, N, 3] (the
    positions the last forward pass used, z = 0), ``C`` [M], ``losses`` [M, num_epochs] (NaN beyond the stop; entry
    ``epochs[m]`` is the stopping epoch's loss, which the reference does not record), ``epochs`` [M] (updates
    made = length of the reference's ``errors``)."""

    def __init__(self, sensors, sounds, C, losses, epochs):
        self.sensors, self.sounds, self.C, self.losses, self.epochs = sensors, sounds, C, losses, epochs

    def __len__(self):
        return self.sensors.shape[0]

    def errors(self, i):
        return [np.asarray(v) for v in self.losses[i, :int(self.epochs[i])].cpu().numpy()]


def _position_inputs(observed_lags, sensor_positions, sound_positions, per_problem, sr):
    """Shapes, broadcasting and refusals shared by optimize_positions_device and tdoa_loss_and_grads_device:
    (M, N, device, obs [N, 2] or [M, N, 2] in seconds, sensors [M, 4, 3], sounds [M, N, 2], the per-problem value
    lists); nothing touches the GPU before every ValueError had its chance."""
    lags = torch.as_tensor(observed_lags)
    sens = torch.as_tensor(sensor_positions)
    snd = torch.as_tensor(sound_positions)
    if sens.dim() not in (2, 3) or tuple(sens.shape[-2:]) != (4, 3):
        raise ValueError(f"initial_sensor_positions {tuple(sens.shape)}: exactly 4 sensors [4, 3] are needed (the "
                         "lags pair sensor 0 with 2 and 1 with 3)")
    if lags.dim() not in (2, 3) or lags.shape[-1] != 2:
        raise ValueError(f"observed_lags {tuple(lags.shape)}: expected [N, 2]")
    if snd.dim() not in (2, 3) or snd.shape[-1] < 2 or snd.shape[-2] != lags.shape[-2]:
        raise ValueError(f"initial_sound_positions {tuple(snd.shape)}: expected [N, >= 2] with N = {lags.shape[-2]}")
    N = int(lags.shape[-2])
    if N < 1 or N > TDOA_MAX_SOUNDS:
        raise ValueError(f"{N} sounds: the limit is 1..{TDOA_MAX_SOUNDS}")
    sizes = [t.shape[0] for t in (lags, sens, snd) if t.dim() == 3]
    sizes += [int(np.size(v)) for _w, v in per_problem if np.size(v) > 1]
    M = max(sizes) if sizes else 1
    if any(s != M for s in sizes):
        raise ValueError(f"inputs disagree on the number of problems: {sizes}")
    values = [_per_problem(v, M, what) for what, v in per_problem]
    dev = _device_of(lags)
    _lib.require_gpu(dev.index or 0)
    obs = (lags.detach().to(dev) / sr).to(torch.float32).contiguous()
    sens0 = sens.detach().to(dev, torch.float32).expand(M, 4, 3).contiguous()
    snd0 = snd.detach()[..., :2].to(dev, torch.float32).expand(M, N, 2).contiguous()
    return M, N, dev, obs, sens0, snd0, values


def optimize_positions_device(observed_lags, initial_sensor_positions, initial_sound_positions, lr=0.01,
                              lossfun=F.mse_loss, num_epochs=1000, C=342.29, sr=96000, eps=1e-12, patience=10):
    """M independent optimize_positions fits in one launch.  observed_lags [M, N, 2] (or [N, 2]) in samples,
    initial_sensor_positions [M, 4, 3] (or [4, 3]), initial_sound_positions [M, N, >= 2] (or [N, >= 2]); lr and C
    numbers or M of them.  Returns PositionFits."""
    loss = _loss_code(lossfun)
    num_epochs, patience = int(num_epochs), int(math.ceil(patience))
    if num_epochs < 1:
        raise ValueError("num_epochs must be at least 1")

    M, N, dev, obs, sens0, snd0, (lrs, cs) = _position_inputs(observed_lags, initial_sensor_positions,
                                                             initial_sound_positions, (("lr", lr), ("C", C)), sr)
    L = _lib.lib()
    c0 = torch.tensor(cs, dtype=torch.float32, device=dev)
    table, rows = _rate_rows(lrs, lambda v: _position_tables(v, num_epochs)[1])
    table, rows = table.to(dev), rows.to(dev)
    sensors = torch.empty_like(sens0)
    sounds = torch.empty((M, N, 3), dtype=torch.float32, device=dev)
    c_out = torch.empty_like(c0)
    losses = torch.full((M, num_epochs), float("nan"), dtype=torch.float32, device=dev)
    epochs = torch.zeros(M, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        check(L.ofp_tdoa_fit(M, N, obs.data_ptr(), N * 2 if obs.dim() == 3 else 0, sens0.data_ptr(), snd0.data_ptr(),
                             c0.data_ptr(), loss, table.data_ptr(), rows.data_ptr(), num_epochs, float(eps), patience,
                             sensors.data_ptr(), sounds.data_ptr(), c_out.data_ptr(), losses.data_ptr(),
                             epochs.data_ptr(), _stream(dev)), "ofp_tdoa_fit")
    return PositionFits(sensors, sounds, c_out, losses, epochs)


def tdoa_loss_and_grads_device(observed_lags, sensor_positions, sound_positions, C=342.29, lossfun=F.mse_loss,
                               sr=96000):
    """Loss and unclipped gradients of optimize_positions' objective at the given point, by the fit's own forward
    and reduction (k_tdoa_fit leaving after its first epoch's sums, csrc/ofp_train.hip).  Inputs broadcast as in
    optimize_positions_device.  Returns (loss [M], {"sensors": [M, 4, 3], "sounds": [M, N, 2], "C": [M]}) on the
    GPU."""
    loss = _loss_code(lossfun)
    M, N, dev, obs, sens0, snd0, (cs,) = _position_inputs(observed_lags, sensor_positions, sound_positions,
                                                          (("C", C),), sr)
    L = _lib.lib()
    c0 = torch.tensor(cs, dtype=torch.float32, device=dev)
    out_loss = torch.empty(M, dtype=torch.float32, device=dev)
    g_sens, g_snd, g_c = torch.empty_like(sens0), torch.empty_like(snd0), torch.empty_like(c0)
    with torch.cuda.device(dev):
        check(L.ofp_tdoa_loss_grads(M, N, obs.data_ptr(), N * 2 if obs.dim() == 3 else 0, sens0.data_ptr(),
                                    snd0.data_ptr(), c0.data_ptr(), loss, out_loss.data_ptr(), g_sens.data_ptr(),
                                    g_snd.data_ptr(), g_c.data_ptr(), _stream(dev)), "ofp_tdoa_loss_grads")
    return out_loss, {"sensors": g_sens, "sounds": g_snd, "C": g_c}


def optimize_positions(observed_lags, initial_sensor_positions, initial_sound_positions, lr=0.01,
                       lossfun=F.mse_loss, num_epochs=1000, C=342.29, sr=96000, radius=0.1778, eps=1e-12,
                       patience=10, print_every=10, debug=False):
    """calibration.py:563-682 on the GPU: fits the 4 sensor positions, the x and y of every sound and the speed of
    sound C to the observed lags of sensor pairs (0, 2) and (1, 3); returns ``(sensor_positions [4, 3],
    sound_positions [N, 3], C)``.  `radius` is unused, as in the reference.  One kernel launch."""
    lags = torch.as_tensor(observed_lags)
    if lags.dim() != 2:
        raise ValueError(f"observed_lags {tuple(lags.shape)}: expected [N, 2]")
    fit = optimize_positions_device(lags, initial_sensor_positions, initial_sound_positions, lr, lossfun, num_epochs,
                                    C, sr, eps, patience)
    n = int(fit.epochs[0])
    curve = fit.losses[0].cpu().numpy()
    last, eps32 = np.float32(np.inf), np.float32(eps)
    for e in range(n):
        if curve[e] < last - eps32:
            last = curve[e]
        if e % print_every == 0:
            print(f"Epoch {e}, Loss {float(curve[e])}, LL {float(last) - eps}")
    final = n if n < int(num_epochs) else n - 1
    print(f"Epoch {final}, Loss {float(curve[final])}")
    to = (lambda t: t) if lags.is_cuda else (lambda t: t.cpu())
    sensors, sounds, c = to(fit.sensors[0]), to(fit.sounds[0]), to(fit.C[0])
    if debug:
        d = (sounds[:10, None, :] - sensors[None, :, :]).pow(2).sum(-1).sqrt()
        print((d[:, :2] - d[:, 2:]) / c, "\n", (lags / sr)[:10])
    return sensors, sounds, c
