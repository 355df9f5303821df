#!/usr/bin/env python3
"""Golden vectors g28_cnnrnn_train: the reference's model.CNNRNN trained by its own training_step and
configure_optimizers (NAdam, CosineAnnealingLR(100)), one full batch per epoch, with torch on the host, one thread.

Run in the build container only:   python tests/golden/make_golden_cnnrnn_train.py
A second run writes the same bytes.

Built like make_golden_cnn_train.py, whose synthetic windows, comparable prefix and padding it imports: each epoch is
zero_grad, training_step, backward, optimizer.step, scheduler.step; the stop case then evaluates validation_step in
eval mode.  dropout_rate is 0.0, so neither the dropout in front of the GRU nor the attention's draws anything.  Every
run is repeated 8 times with the inputs scaled by (1 + k * 2^-23), k = 1..8, and once in float64;
tests/test_gpu_cnnrnn_train.py derives its bounds from how far the reference strays from itself.  This script asserts
the conditions those tests rely on (check_case) and prints, per case, the smallest share any parameter's float64
start gradient has of the largest (a figure, not a condition).

Contents: the keys of g26_cnn_train (make_golden_cnn_train.py), every key prefixed by <case>/.
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
MIN_PREFIX = 24

_FIRST = dict(layer_sizes=[4, 6], kernel_size=3, n_hidden=8, loss="l1_loss", batch_norm=False, pool=False, padding=1,
              dilation=1, groups=1, activation="SiLU")
CASES = {
    "l1_silu": dict(n=24, channels=3, width=32, lr=0.01, seed=3, epochs=EPOCHS, kwargs=_FIRST),
    "mse_tanh_bn_pool": dict(n=20, channels=4, width=36, lr=0.003, seed=7, epochs=EPOCHS,
                             kwargs=dict(layer_sizes=[5], kernel_size=3, n_hidden=6, loss="mse_loss", batch_norm=True,
                                         pool=True, padding=1, dilation=2, groups=1, activation="Tanh")),
    "l1_silu_bn_wide": dict(n=37, channels=4, width=33, lr=0.003, seed=5, epochs=EPOCHS,
                            kwargs=dict(layer_sizes=[5, 7], kernel_size=5, n_hidden=16, loss="l1_loss",
                                        batch_norm=True, pool=False, padding=2, dilation=1, groups=1,
                                        activation="SiLU")),
    # the first case with another seed, a validation set and a patience that ends it early
    "l1_silu_stop": dict(n=24, channels=3, width=32, lr=0.01, seed=9, epochs=EPOCHS, n_val=16, patience=4,
                         kwargs=_FIRST),
}


def build(ref, cfg, state=None, dtype=None):
    import torch
    import torch.nn.functional as F
    from torch import nn
    kw = dict(cfg["kwargs"])
    kw["activation"] = getattr(nn, kw["activation"])
    kw["loss"] = getattr(F, kw["loss"])
    torch.manual_seed(cfg["seed"])
    m = ref.model.CNNRNN(cfg["width"], 2, channels=cfg["channels"], dropout_rate=0.0, lr=cfg["lr"], **kw)
    m.log = lambda *a, **k: None
    if state is not None:
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
            # EarlyStopping(monitor="val_loss", mode="min", min_delta=0, patience=...), as fit_cnn states it
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
    n, E = cfg["n"], cfg["epochs"]
    x, y = torch.from_numpy(xs[:n]), torch.from_numpy(ys[:n])
    val = (torch.from_numpy(xs[n:]), torch.from_numpy(ys[n:])) if "n_val" in cfg else None
    pre = name + "/"
    start = {k: v.clone() for k, v in build(ref, cfg).state_dict().items()}
    for k, v in start.items():
        out[pre + "sd0/" + k] = v.numpy().copy()
    for dtype, tag in ((torch.float32, "32"), (torch.float64, "64")):
        net = build(ref, cfg, start, dtype).train()
        loss = net.training_step((x.to(dtype), y.to(dtype)), 0)
        loss.backward()
        out[pre + "loss" + tag] = np.array(loss.item(), np.float64)
        for k, p in net.named_parameters():
            out[pre + f"g{tag}/" + k] = p.grad.numpy().copy()
    tops = {k[len(pre) + 4:]: float(np.max(np.abs(v))) for k, v in out.items() if k.startswith(pre + "g64/")}
    low = min(tops, key=tops.get)
    print(f"{name}: smallest share of the largest float64 start gradient {tops[low] / max(tops.values()):.3g} ({low})")
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
    stats = [[b.detach().reshape(-1) for k, b in r[0].named_buffers() if "running" in k] for r in runs]
    out[pre + "stats"] = np.stack([torch.cat(s).numpy() if s else np.zeros(0, np.float32) for s in stats])
    if val is not None:
        out[pre + "x_val"], out[pre + "y_val"] = val[0].numpy(), val[1].numpy()
        out[pre + "val"] = vals.astype(np.float32)
        out[pre + "val64"] = val64.astype(np.float64)
        out[pre + "pert_val"] = np.stack([padded(r[3], E) for r in runs[1:]])
        out[pre + "stop"] = np.array(ran, np.int64)
        out[pre + "pert_stop"] = np.array([r[4] for r in runs[1:]], np.int64)
    check_case(name, cfg, runs, len(curve64))


def check_case(name, cfg, runs, ran64):
    """What the tests rely on: a comparable prefix of at least 24 epochs with all eight disturbed runs, a network
    that learns (the best loss is at most the first divided by 1.2), and for the stop case one stopping epoch for all
    ten runs, inside the prefix and before the full length."""
    curve, ran = runs[0][1], runs[0][4]
    pert = np.stack([padded(r[1], cfg["epochs"]) for r in runs[1:]])
    prefix = comparable_prefix(curve.astype(np.float32), pert[:, :ran])
    finals = [float(r[1][-1]) for r in runs]
    print(f"{name}: prefix {prefix} of {ran}, loss {curve[0]:.5g} -> {curve[-1]:.5g} (best {curve.min():.5g}), "
          f"finals {min(finals):.5g} .. {max(finals):.5g}, epochs run {[r[4] for r in runs]} and {ran64} in float64")
    assert prefix >= MIN_PREFIX, (name, prefix)
    assert curve.min() * 1.2 <= curve[0], (name, curve[0], curve.min())
    if "patience" in cfg:
        assert ran < cfg["epochs"] and prefix == ran, (name, prefix, ran)  # every epoch run is comparable
        assert all(r[4] == ran for r in runs) and ran64 == ran, (name, [r[4] for r in runs], ran64)


def main():
    import torch
    torch.set_num_threads(1)
    ref = load_reference()
    out = {}
    for name, cfg in CASES.items():
        run_case(ref, name, cfg, out)
    path = HERE / "g28_cnnrnn_train.npz"
    write_npz(path, out)
    print(path, path.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
