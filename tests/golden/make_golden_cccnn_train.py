#!/usr/bin/env python3
"""Golden vectors g27_cccnn_train: the reference's model.LCCCNN trained by its own training_step and
configure_optimizers (SGD at 100 x lr with momentum 0.8 and weight decay 1e-3, CosineAnnealingLR(100)), one full
batch per epoch, with torch on the host, one thread.

Run in the build container only, after `make -C oracle ref`:   python tests/golden/make_golden_cccnn_train.py
A second run writes the same bytes.

The loop, the data (windows()), the eight disturbed runs, the float64 run and the keys are those of
make_golden_cnn_train.py; see its docstring.  There are no running statistics here (GroupNorm), so `stats` is
empty.  Two things differ:

With PyTorch's default initialisation the softmax of the correlation head is saturated at lag 0 (after GroupNorm
cc[0] is about K V), and the conv stack's gradients are some 1e-9 of fc.bias's: such a start pins nothing.  The
cases therefore scale GroupNorm's initial weights (`gn_scale`, applied to sd0) or the inputs (`x_scale`), and
check_case asserts that every parameter tensor's largest float64 gradient at the start is at least 1e-3 of the
largest tensor's.

The comparable prefix of the L1 cases is shorter than the CNN's (SGD at a rate of 0.3 amplifies a disturbance
faster than NAdam at 0.01): at least 16 epochs are asserted for them, the whole length for the MSE case.
"""
import json
import sys
import warnings
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
REPO = HERE.parents[1]
sys.path.insert(0, str(HERE))
sys.path.insert(0, str(REPO))

from _refload import load_reference  # noqa: E402
from make_golden_cnn_train import N_PERT, comparable_prefix, padded, windows  # noqa: E402
from make_golden_locate import write_npz  # noqa: E402

warnings.filterwarnings("ignore")

EPOCHS = 300
MIN_PREFIX = 16
MIN_GRAD_SHARE = 1e-3

_SHARED = dict(n=24, channels=3, width=32, lr=0.003, seed=3, epochs=EPOCHS, gn_scale=0.2, x_scale=1.0,
               kwargs=dict(layer_sizes=[3, 2], kernel_sizes=[9, 1], strides=1, loss="l1_loss", batch_norm=True,
                           pool=False, padding=1, dilation=1, group=False, activation="SiLU"))
CASES = {
    "shared_gn_l1_silu": _SHARED,
    "grouped_strided_l1": dict(n=20, channels=4, width=33, lr=0.003, seed=5, epochs=EPOCHS, gn_scale=1.0, x_scale=6.0,
                               kwargs=dict(layer_sizes=[2, 2], kernel_sizes=[5, 3], strides=[2, 1], loss="l1_loss",
                                           batch_norm=False, pool=False, padding=1, dilation=1, group=True,
                                           activation="SiLU")),
    "shared_gn_pool_mse_tanh_dil": dict(n=20, channels=3, width=36, lr=0.002, seed=7, epochs=EPOCHS, gn_scale=0.25,
                                        x_scale=1.0, full_prefix=True,
                                        kwargs=dict(layer_sizes=[3], kernel_sizes=12, strides=1, loss="mse_loss",
                                                    batch_norm=True, pool=True, padding=2, dilation=2, group=False,
                                                    activation="Tanh")),
    # the first case with a validation set and a patience that ends it early.  Its own seed: with seed 3 the
    # validation loss has its best value at epoch 2 and no other until epoch 131, so that every patience either stops
    # before the network has learnt anything or not at all; with seed 9 the best lies at epoch 121, 4e-3 below what
    # follows, and all runs stop after 125 epochs, inside the comparable prefix
    "shared_gn_l1_silu_stop": dict(_SHARED, seed=9, n_val=16, patience=4),
}


def build(ref, cfg, state=None, dtype=None):
    import torch
    import torch.nn.functional as F
    from torch import nn
    kw = dict(cfg["kwargs"])
    kw["activation"] = getattr(nn, kw["activation"])
    kw["loss"] = getattr(F, kw["loss"])
    torch.manual_seed(cfg["seed"])
    m = ref.model.LCCCNN(cfg["width"], 2, channels=cfg["channels"], dropout_rate=0.0, lr=cfg["lr"], **kw)
    m.log = lambda *a, **k: None
    if state is None:
        with torch.no_grad():
            for mod in m.model.conv_layers:
                if isinstance(mod, nn.GroupNorm):
                    mod.weight.mul_(cfg["gn_scale"])
    else:
        m.load_state_dict(state)
    if dtype is not None:
        m = m.to(dtype)
    return m


def fit(ref, cfg, start, x, y, dtype, val=None):
    """The reference's loop.  -> (model, train curve, lrs, val curve, epochs run)."""
    import torch
    m = build(ref, cfg, start, dtype).train()
    conf = m.configure_optimizers()
    opt, sched = conf["optimizer"], conf["lr_scheduler"]["scheduler"]
    x, y = x.to(dtype), y.to(dtype)
    curve, lrs, vals = [], [], []
    best, wait, reached = float("inf"), 0, False
    for _e in range(cfg["epochs"]):
        opt.zero_grad()
        loss = m.training_step((x, y), 0)
        loss.backward()
        lrs.append(float(opt.param_groups[0]["lr"]))
        opt.step()
        sched.step()
        curve.append(loss.item())
        if val is not None:
            m.eval()
            with torch.no_grad():
                v = m.validation_step((val[0].to(dtype), val[1].to(dtype)), 0).item()
            m.train()
            vals.append(v)
            # EarlyStopping(monitor="val_loss", mode="min", min_delta=0, patience=...), as fit_lcccnn states it
            if v < best:
                best, wait = v, 0
            else:
                wait += 1
            reached = reached or wait >= cfg["patience"]
            if reached:
                break
    return m, np.array(curve), np.array(lrs, np.float64), np.array(vals), len(curve)


def run_case(ref, name, cfg, out):
    import torch
    rng = np.random.default_rng(cfg["seed"])
    xs, ys = windows(rng, cfg["n"] + cfg.get("n_val", 0), cfg["channels"], cfg["width"])
    xs = (xs * np.float32(cfg["x_scale"])).astype(np.float32)
    n, E = cfg["n"], cfg["epochs"]
    x, y = torch.from_numpy(xs[:n]), torch.from_numpy(ys[:n])
    val = (torch.from_numpy(xs[n:]), torch.from_numpy(ys[n:])) if "n_val" in cfg else None
    pre = name + "/"
    start = {k: v.clone() for k, v in build(ref, cfg).state_dict().items()}
    for k, v in start.items():
        out[pre + "sd0/" + k] = v.numpy().copy()
    grads64 = {}
    for dtype, tag in ((torch.float32, "32"), (torch.float64, "64")):
        net = build(ref, cfg, start, dtype).train()
        loss = net.training_step((x.to(dtype), y.to(dtype)), 0)
        loss.backward()
        out[pre + "loss" + tag] = np.array(loss.item(), np.float64)
        for k, p in net.named_parameters():
            out[pre + f"g{tag}/" + k] = p.grad.numpy().copy()
            if tag == "64":
                grads64[k] = float(p.grad.abs().max())
    runs = [fit(ref, cfg, start, x * np.float32(1 + k * 2.0 ** -23), y, torch.float32, val) for k in range(N_PERT + 1)]
    m64, curve64, _l, val64, _n = fit(ref, cfg, start, x, y, torch.float64, val)
    model, curve, lrs, vals, ran = runs[0]
    for k, v in model.state_dict().items():
        out[pre + "sd1/" + k] = v.numpy().copy()
    out[pre + "x"], out[pre + "y"] = x.numpy(), y.numpy()
    out[pre + "cfg"] = np.array(json.dumps(cfg, sort_keys=True))
    out[pre + "errors"] = curve.astype(np.float32)
    out[pre + "errors64"] = curve64.astype(np.float64)
    out[pre + "rates"] = lrs
    out[pre + "pert_errors"] = np.stack([padded(r[1], E) for r in runs[1:]])
    out[pre + "flat"] = np.stack([torch.cat([p.detach().reshape(-1) for p in r[0].parameters()]).numpy() for r in runs])
    out[pre + "stats"] = np.zeros((len(runs), 0), np.float32)
    if val is not None:
        out[pre + "x_val"], out[pre + "y_val"] = val[0].numpy(), val[1].numpy()
        out[pre + "val"] = vals.astype(np.float32)
        out[pre + "val64"] = val64.astype(np.float64)
        out[pre + "pert_val"] = np.stack([padded(r[3], E) for r in runs[1:]])
        out[pre + "stop"] = np.array(ran, np.int64)
        out[pre + "pert_stop"] = np.array([r[4] for r in runs[1:]], np.int64)
    check_case(name, cfg, runs, len(curve64), grads64)


def check_case(name, cfg, runs, ran64, grads64):
    """What the tests rely on: no parameter tensor whose gradient at the start is noise, a comparable prefix of at
    least 16 epochs (the whole run where the case says so), a network that learns (the loss falls by a factor of 1.2
    at least), and for the stop case one stopping epoch, before the end, for all."""
    curve, ran = runs[0][1], runs[0][4]
    pert = np.stack([padded(r[1], cfg["epochs"]) for r in runs[1:]])
    prefix = comparable_prefix(curve.astype(np.float32), pert[:, :ran])
    finals = [float(r[1][-1]) for r in runs]
    share = min(grads64.values()) / max(grads64.values())
    print(f"{name}: prefix {prefix} of {ran}, loss {curve[0]:.5g} -> {curve[-1]:.5g} (best {curve.min():.5g}), finals "
          f"{min(finals):.4g} .. {max(finals):.4g}, epochs run {[r[4] for r in runs]} and {ran64} in float64, smallest "
          f"share of the gradient {share:.3g}")
    assert share >= MIN_GRAD_SHARE, (name, grads64)
    assert prefix >= (ran if cfg.get("full_prefix") else min(MIN_PREFIX, ran)), (name, prefix)
    assert curve.min() * 1.2 <= curve[0], (name, curve[0], curve.min())
    if "patience" in cfg:
        assert ran < cfg["epochs"], (name, prefix, ran)
        assert all(r[4] == ran for r in runs) and ran64 == ran, (name, [r[4] for r in runs], ran64)


def main():
    import torch
    torch.set_num_threads(1)
    ref = load_reference()
    out = {}
    for name, cfg in CASES.items():
        run_case(ref, name, cfg, out)
    path = HERE / "g27_cccnn_train.npz"
    write_npz(path, out)
    print(path, path.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
