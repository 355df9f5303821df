"""The two sequence trainers (model.fit_rnn, model.fit_cnnrnn) under the trainers' random stream over whole epochs: the
case tables of tests/test_seq_train_random_cpu.py and tests/test_gpu_seq_train_random.py, and the CPU torch replay they
are held to -- the sequence-model counterpart of train_random_ref.replay / replays.

The replay trains the module's own torch layers on the CPU, in float32 or float64, by each trainer's own recipe (RNN:
NAdam with weight decay 1e-4 and CosineAnnealingLR(3000); CNNRNN: NAdam without decay and CosineAnnealingLR(100)), one
full batch per epoch.  The batch of epoch e comes from the caller; the masks of epoch e come from the numpy generators
(site 0: train_random_ref.dropout_mask on the CNNRNN's conv features, site 3: cnnrnn_train_ref.attention_dropout_mask
on the attention probabilities, site 4: rnn_train_ref.layer_dropout_mask between the RNN's layers) and are applied by
the masked form of tests/test_gpu_rnn_train.py::torch_forward.  A CNNRNN behind its conv stack is that function's
network with one recurrent layer and no LayerNorm, so the same helper serves both.

What the values of the case tables straddle (the four constants are restated in test_seq_train_random_cpu.py):

  axis             values        what they straddle
  audio channels   1, 3, 8       k_inproj_wgrad_partial keeps kMaxIn + 1 = 9 sums per thread and uses the first F and the
                                 last (the bias): 1 uses the fewest, 8 = kMaxIn all, 3 is the reference's; the window
                                 kernels' item layout and k_stretch_windows' LDS are sized from the channel count each
                                 entry passes to make_random
  width            31, 32        31 is odd and no multiple of 4: the strided read {F T, 1, T} of [n][channels][width]
                                 has rows that start off a 16-byte boundary; the stretch span is 3 at both
  windows          42, 66        66 = 33 onsets x 2 extractions: two head chunks of 64 samples and three GRU workgroups
                                 of 32 sequences; for the RNN (T = 32) 2 112 rows: nine dense slabs of 256 rows and two
                                 input-projection slabs of 2 048; for the CNNRNN (T = 6) 396 rows: two dense slabs
  n_val            70 > n = 42   the validation batch sizes the work space while o_X is sized by n; 70 is also past one
                                 head chunk
  layers (RNN)     1, 2, 3       no site-4 mask, one, two (the mask's layer index)
  BatchNorm        off, on       (CNNRNN) batch statistics in the training forward, running ones in the validation
  p                0.1, 0.5      both thresholds of the mask
  source           shifted, stretched   k_shift_windows or k_stretch_windows as the epoch's first kernel
"""
import copy
import functools
import sys
from pathlib import Path
from types import SimpleNamespace

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent))
import cnnrnn_train_ref as AR  # noqa: E402
import rnn_train_ref as LR  # noqa: E402
import train_random_ref as R  # noqa: E402
import train_stretch_ref as S  # noqa: E402

f32, f64 = np.float32, np.float64
SEED = 2024
MAX_SHIFT, REPS, MAX_STRETCH, SPAN, PRE = 3, 2, 0.1, 3, 2
ONSETS = 21  # x 2 extractions = 42 windows
N_VAL = 70
RNN_WEIGHT_DECAY, RNN_T_MAX, CNNRNN_T_MAX = 1e-4, 3000, 100


def case(kind, p, source, traj=False, channels=3, width=32, onsets=ONSETS, **kw):
    return SimpleNamespace(kind=kind, p=p, source=source, traj=traj, channels=channels, width=width, onsets=onsets,
                           kw=kw)


# every case of the anchor test; the four per trainer with traj=True are also trained for 40 epochs against the replay.
# Each edge is one extra case at p = 0.5 with the stretched source.
CASES = {
    "rnn_p0.1_shifted": case("rnn", 0.1, "shifted", True),
    "rnn_p0.1_stretched": case("rnn", 0.1, "stretched", True),
    "rnn_p0.5_shifted": case("rnn", 0.5, "shifted", True),
    "rnn_p0.5_stretched": case("rnn", 0.5, "stretched", True),
    "rnn_one_layer": case("rnn", 0.5, "stretched", num_layers=1),
    "rnn_three_layers": case("rnn", 0.5, "stretched", num_layers=3),
    "rnn_1_channel": case("rnn", 0.5, "stretched", channels=1),
    "rnn_8_channels": case("rnn", 0.5, "stretched", channels=8),
    "rnn_width_31": case("rnn", 0.5, "stretched", width=31),
    "rnn_66_windows": case("rnn", 0.5, "stretched", onsets=33),
    "cnnrnn_p0.1_shifted": case("cnnrnn", 0.1, "shifted", True),
    "cnnrnn_bn_p0.1_stretched": case("cnnrnn", 0.1, "stretched", True, batch_norm=True),
    "cnnrnn_bn_p0.5_shifted": case("cnnrnn", 0.5, "shifted", True, batch_norm=True),
    "cnnrnn_p0.5_stretched": case("cnnrnn", 0.5, "stretched", True),
    "cnnrnn_bn_p0.5_stretched": case("cnnrnn", 0.5, "stretched", batch_norm=True),
    "cnnrnn_1_channel": case("cnnrnn", 0.5, "stretched", channels=1),
    "cnnrnn_8_channels": case("cnnrnn", 0.5, "stretched", channels=8),
    "cnnrnn_66_windows": case("cnnrnn", 0.5, "stretched", onsets=33),
}
TRAJ = [k for k, c in CASES.items() if c.traj]
# the case the graph, off-means-off and validation tests run, per trainer (p is set by those tests)
MAIN = {"rnn": "rnn_p0.5_stretched", "cnnrnn": "cnnrnn_bn_p0.5_stretched"}


def make_model(c, p=None):
    """The case's module at dropout p (the case's own by default).  MSE and Tanh: the smooth kind the comparable prefix
    asks for, as tests/test_gpu_train_random.py's TRAJ found for the CNN."""
    import torch
    import torch.nn.functional as F
    from torch import nn

    from onset_fingerprinting_amd import model
    p = c.p if p is None else p
    torch.manual_seed(31)
    if c.kind == "rnn":
        kw = dict(hidden_size=8, num_heads=2, num_layers=2, lr=0.003, loss=F.mse_loss)
        kw.update(c.kw)
        m = model.RNN(c.width, 2, channels=c.channels, dropout_rate=p, **kw)
        # The softmax does not see the keys' bias, so its gradient is rounding noise, which NAdam normalises to steps
        # of the learning rate: from torch's zero start the eight values walk at random (4e-4 between the disturbed
        # replays after 40 epochs, against 3e-7 for every other parameter) and the end-parameter check measures that
        # walk.  From a start that is not zero the weight decay's 1e-4 x bias is their gradient, the same in every run.
        with torch.no_grad():
            m.attention.in_proj_bias.normal_(0.0, 0.1)
        return m
    kw = dict(layer_sizes=[4, 6], n_hidden=8, lr=0.003, loss=F.mse_loss, activation=nn.Tanh)
    kw.update(c.kw)
    return model.CNNRNN(c.width, 2, channels=c.channels, dropout_rate=p, **kw)


def steps_of(c):
    """The GRU's time steps: the window for the RNN, the last conv layer's channels for the CNNRNN."""
    return c.width if c.kind == "rnn" else c.kw.get("layer_sizes", [4, 6])[-1]


def hits(c):
    """(audio [N, channels], onsets [O, channels], y [O, 2]) with room for every shift and stretch."""
    return R.synthetic_hits(8, c.onsets, c.channels, c.width, MAX_SHIFT + SPAN)


def make_source(c, kind=None, **kw):
    """The case's window source on the GPU (kind: "shifted" or "stretched", the case's own by default)."""
    from onset_fingerprinting_amd import data
    audio, onsets, _y = hits(c)
    args = dict(pre_samples=PRE, max_shift=MAX_SHIFT, n_extractions=REPS)
    if (kind or c.source) == "stretched":
        args["max_stretch"] = MAX_STRETCH
        args.update(kw)
        return data.StretchedWindows(audio, onsets, c.width, **args)
    args.update(kw)
    return data.ShiftedWindows(audio, onsets, c.width, **args)


def labels(c):
    """y of the whole batch, float32 [O x REPS, 2]."""
    return np.tile(hits(c)[2], (REPS, 1))


def cpu_batches(c, seed, epochs):
    """The batches of the first epochs from the numpy references alone (the stretched ones are the float64 resampling
    rounded to float32, not the kernel's bits): for what can be said of the replay without a GPU."""
    audio, onsets, _y = hits(c)
    starts = onsets.min(1) - PRE
    if c.source == "shifted":
        return [R.shifted_windows(audio, starts, c.width, seed, e, MAX_SHIFT, REPS)[1] for e in range(epochs)]
    return [S.stretched_windows(audio, starts, c.width, seed, e, MAX_SHIFT, SPAN, REPS)[2].astype(f32)
            for e in range(epochs)]


# the masks of an epoch are the same in all ten replays of a case
_layer_mask = functools.lru_cache(maxsize=256)(LR.layer_dropout_mask)
_attention_mask = functools.lru_cache(maxsize=256)(AR.attention_dropout_mask)
_feature_mask = functools.lru_cache(maxsize=256)(R.dropout_mask)


def forward(kind, net, x, seed, epoch, p):
    """The training forward of epoch `epoch` over the module's torch layers, under the stream's masks when p > 0."""
    import torch

    import test_gpu_cnnrnn_train as GC
    import test_gpu_rnn_train as GR
    if kind == "rnn":
        if p == 0:
            return GR.torch_forward(net, x)
        n, T = x.shape[0], x.shape[2]
        L, H = net.rnn.num_layers, net.rnn.hidden_size
        lmask = _layer_mask(seed, epoch, L - 1, n, T, H, p) if L > 1 else None
        return GR.torch_forward(net, x, lmask, _attention_mask(seed, epoch, n, net.attention.num_heads, T, p))
    if p == 0:
        return GC.torch_forward(net, x)
    h = net.conv_layers(x)  # [n, C, W]: C time steps of W features
    n, C, W = h.shape
    h = h * torch.from_numpy(_feature_mask(seed, epoch, n, C * W, p).reshape(n, C, W)).to(h.dtype)
    tail = SimpleNamespace(permute_input=False, rnn=net.rnn, layer_norm=lambda t: t, attention=net.attention, fc=net.fc)
    return GR.torch_forward(tail, h, None, _attention_mask(seed, epoch, n, net.attention.num_heads, C, p))


def optimiser(kind, net, lr):
    import torch
    if kind == "rnn":
        opt = torch.optim.NAdam(net.parameters(), lr=lr, weight_decay=RNN_WEIGHT_DECAY)
        return opt, torch.optim.lr_scheduler.CosineAnnealingLR(opt, RNN_T_MAX)
    opt = torch.optim.NAdam(net.parameters(), lr=lr)
    return opt, torch.optim.lr_scheduler.CosineAnnealingLR(opt, CNNRNN_T_MAX)


def replay(kind, module, batch_of_epoch, y, epochs, seed, p, dtype):
    """`epochs` epochs of the trainer's recipe on the CPU; batch_of_epoch(e) -> float32 numpy [n, C, W].
    -> (loss curve float64 [epochs], final parameters flat float64)."""
    import torch
    net = copy.deepcopy(module).cpu().to(dtype).train()
    opt, sched = optimiser(kind, net, module.lr)
    yt = torch.as_tensor(y).to(dtype)
    curve = []
    for e in range(epochs):
        x = torch.from_numpy(np.ascontiguousarray(batch_of_epoch(e))).to(dtype)
        opt.zero_grad()
        loss = module.loss(forward(kind, net, x, seed, e, p), yt)
        loss.backward()
        opt.step()
        sched.step()
        curve.append(float(loss.detach()))
    flat = torch.cat([q.detach().reshape(-1) for q in net.parameters()]).numpy().astype(f64)
    return np.array(curve, f64), flat


def replays(kind, module, batches, y, seed, p, n_pert=8):
    """The float32 replay, the float64 one and n_pert float32 ones with one element of every epoch's batch moved by one
    ulp (train_random_ref.one_ulp); batches: the float32 [n, C, W] batch of every epoch.
    -> dict(ref32, ref64, pert [n_pert, epochs], flat [1 + n_pert, n_params]) for train_random_ref.comparable_prefix."""
    import torch
    epochs = len(batches)
    c32, flat = replay(kind, module, lambda e: batches[e], y, epochs, seed, p, torch.float32)
    c64, _f = replay(kind, module, lambda e: batches[e], y, epochs, seed, p, torch.float64)
    pert = [replay(kind, module, lambda e, k=k: R.one_ulp(batches[e], k + 1), y, epochs, seed, p, torch.float32)
            for k in range(n_pert)]
    return dict(ref32=c32, ref64=c64, pert=np.stack([c for c, _f in pert]), flat=np.stack([flat] + [f for _c, f in pert]))
