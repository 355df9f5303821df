#!/usr/bin/env python3
"""Golden vectors g24_calibration: the reference's train_location_model, optimize_positions and
calibration_locations (calibration.py), run with torch on the host, one thread.

Run in the build container only:   python tests/golden/make_golden_calib.py
A second run writes the same bytes.

Synthetic drumhead data, seeded: four sensors at 0.9 r of a 0.1778 m head, hits uniform on the head, lags rounded to
samples at 96 kHz with +-1 sample of noise.  The location models see lags / 300 (as the notebooks scale them) and
learn positions in units of the radius.

The L1 training runs are chaotic: a last-bit disturbance of the inputs changes where they end.  Every run is
therefore repeated 8 times with the inputs scaled by (1 + k * 2^-23), k = 1..8, and the fixture records how far the
reference strays from itself; tests/test_gpu_calibration.py derives its bounds from that spread.  This script
asserts the two conditions those tests rely on (see check_case).

Contents (every key is prefixed by its section):
  train/<case>/{x, y, cfg}            inputs [N, 3] / [N, 3] float32, cfg = JSON (lr, loss, num_epochs, eps,
                                      patience, kwargs of FCNN, seed)
  train/<case>/sd0/<key>, sd1/<key>   state_dict at the start and as returned
  train/<case>/{errors, rates}        loss curve float32 [n]; learning rate of every optimiser step float64
  train/<case>/{loss32, loss64}       loss at the start, float32 network and a float64 copy of it
  train/<case>/g32/<key>, g64/<key>   gradients after the first backward (unclipped), both precisions
  train/<case>/{pert_errors, pert_len, flat}   disturbed runs: curves [8, num_epochs] (NaN padded), their lengths;
                                      flat [9, n_params] the returned parameters of the undisturbed and the 8 runs
  pos/<case>/{lags, sensors0, sounds0, cfg}    optimize_positions inputs
  pos/<case>/{sensors, sounds, C, curve, steps, rates}   results; curve = every loss evaluated (the stopping epoch's
                                      included), steps = optimiser steps = len(errors) of the reference, rates
                                      [steps, 3]
  pos/<case>/{pert_sensors, pert_sounds, pert_C, pert_curve, pert_steps}   the 8 disturbed runs
  loc/<i>/{args, out}                 calibration_locations(**args) as an array [n, 2 or 3]
  sig/<function>                      JSON list of [parameter name, default] of the reference's signature
"""
import contextlib
import inspect
import io
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
from make_golden_locate import write_npz  # noqa: E402

warnings.filterwarnings("ignore")

RADIUS, SR = 0.1778, 96000
N_PERT = 8

TRAIN = {
    "l1_silu6": dict(n=164, lr=0.0015, loss="l1_loss", num_epochs=3000, eps=1e-9, patience=10, seed=11,
                     kwargs=dict(hidden_layers=[6], activation="SiLU", batch_norm=False, bias=False)),
    "l1_silu11_bn": dict(n=164, lr=0.004, loss="l1_loss", num_epochs=1000, eps=1e-9, patience=10, seed=12,
                         kwargs=dict(hidden_layers=[11], activation="SiLU", batch_norm=True)),
    # seed: the data and start of this case decide whether the nine runs satisfy check_case (a heavy-tailed run
    # among the nine breaks it); 13 and 30, 31 do not, 32 is the first tried that does
    "l1_default": dict(n=164, lr=0.01, loss="l1_loss", num_epochs=1000, eps=1e-9, patience=10, seed=32, kwargs={}),
    "mse_tanh8x8": dict(n=120, lr=0.01, loss="mse_loss", num_epochs=400, eps=1e-9, patience=400, seed=14,
                        kwargs=dict(hidden_layers=[8, 8], activation="Tanh", batch_norm=False)),
    # the same problem with the default patience, which ends it early: the early-stop case of the tests
    "mse_tanh8x8_stop": dict(n=120, lr=0.01, loss="mse_loss", num_epochs=400, eps=1e-9, patience=10, seed=14,
                             kwargs=dict(hidden_layers=[8, 8], activation="Tanh", batch_norm=False)),
}
POS = {
    "defaults": dict(n=84, seed=21, args={}),
    "long": dict(n=84, seed=22, args=dict(lr=0.1, num_epochs=3000, patience=50)),
}
LOC = [
    dict(n_lugs=8, n_each=3, radius=0.9),
    dict(n_lugs=8, n_each=3, radius=0.9, clockwise=True),
    dict(n_lugs=10, n_each=2, radius=0.5, add_z=0),
    dict(n_lugs=4, n_each=[1, 2, 1, 3], radius=0.75),
    dict(n_lugs=4, n_each=[2, 0, 1, 3], radius=0.75, add_z=1, clockwise=True),
]


def sensors_xyz():
    ang = np.deg2rad([0.0, 90.0, 180.0, 270.0])
    return np.stack([0.9 * RADIUS * np.cos(ang), 0.9 * RADIUS * np.sin(ang), np.zeros(4)], 1)


def hits(rng, n):
    r = RADIUS * np.sqrt(rng.uniform(0, 1, n))
    phi = rng.uniform(0, 2 * np.pi, n)
    return np.stack([r * np.cos(phi), r * np.sin(phi), np.zeros(n)], 1)


def sample_lags(rng, pos, sens, c, pairs):
    d = np.linalg.norm(pos[:, None, :] - sens[None, :, :], axis=-1)
    lags = np.stack([np.round((d[:, a] - d[:, b]) / c * SR) for a, b in pairs], 1)
    return lags + rng.integers(-1, 2, lags.shape)


class AdamLog:
    """Records the learning rates of every torch.optim.Adam step made while it is active."""

    def __enter__(self):
        import torch
        self.rates = []
        self._orig = torch.optim.Adam.step
        log, orig = self, self._orig

        def step(opt, *a, **k):
            log.rates.append([float(g["lr"]) for g in opt.param_groups])
            return orig(opt, *a, **k)

        torch.optim.Adam.step = step
        return self

    def __exit__(self, *exc):
        import torch
        torch.optim.Adam.step = self._orig


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def flat_params(model):
    import torch
    return torch.cat([p.detach().reshape(-1) for p in model.parameters()]).numpy().copy()


def curve_array(errors, width):
    out = np.full(width, np.nan, np.float32)
    out[:len(errors)] = np.array([float(e) for e in errors], np.float32)
    return out


def comparable_prefix(ref_curve, pert_curves):
    """Epochs before the first at which the disturbed curves stray more than 1e-5 relative from the undisturbed."""
    n = len(ref_curve)
    for e in range(n):
        col = pert_curves[:, e]
        spread = np.nanmax(np.abs(col - ref_curve[e])) if np.isfinite(col).any() else np.inf
        if np.isnan(col).any() or spread > 1e-5 * ref_curve[e]:
            return e
    return n


def outcome_ok(one, others_final, others_best, others_len, wobble, num_epochs, prefix):
    """The rules of test_gpu_calibration's outcome test, applied to one run against the others."""
    final, best, length = one
    w = max(np.max(others_final) - np.min(others_final), wobble)
    wb = max(np.max(others_best) - np.min(others_best), wobble)
    ok = final <= np.max(others_final) + w and best <= np.max(others_best) + wb
    lo, hi = np.min(others_len), np.max(others_len)
    if lo == num_epochs:
        return ok and length >= prefix
    return ok and lo - (hi - lo) <= length <= hi + (hi - lo)


def train_case(ref, name, cfg, out):
    import torch
    import torch.nn.functional as F
    from torch import nn
    rng = np.random.default_rng(cfg["seed"])
    sens = sensors_xyz()
    pos = hits(rng, cfg["n"])
    lags = sample_lags(rng, pos, sens, 82.0, [(1, 0), (2, 0), (3, 0)])
    x = torch.tensor(lags / 300.0, dtype=torch.float32)
    y = torch.tensor(pos / RADIUS, dtype=torch.float32)
    kw = dict(cfg["kwargs"])
    if "activation" in kw:
        kw["activation"] = getattr(nn, kw["activation"])
    lossfun = getattr(F, cfg["loss"])
    E = cfg["num_epochs"]
    call = dict(lr=cfg["lr"], lossfun=lossfun, num_epochs=E, eps=cfg["eps"], patience=cfg["patience"], **kw)
    pre = f"train/{name}/"

    torch.manual_seed(cfg["seed"])
    start = ref.calibration.FCNN(3, 2, **kw)
    for k, v in start.state_dict().items():
        out[pre + "sd0/" + k] = v.numpy().copy()
    for dtype, tag in ((torch.float32, "32"), (torch.float64, "64")):
        net = ref.calibration.FCNN(3, 2, **kw)
        net.load_state_dict(start.state_dict())
        net = net.to(dtype).train()
        loss = lossfun(net(x.to(dtype)), y[:, :2].to(dtype))
        loss.backward()
        out[pre + "loss" + tag] = np.array(loss.item(), np.float64)
        for k, p in net.named_parameters():
            out[pre + f"g{tag}/" + k] = p.grad.numpy().copy()

    runs = []
    for k in range(N_PERT + 1):
        torch.manual_seed(cfg["seed"])
        xk = x * np.float32(1 + k * 2.0 ** -23)
        with AdamLog() as log:
            model, errors = quiet(ref.calibration.train_location_model, xk, y, **call)
        runs.append((model, curve_array(errors, E), len(errors), np.array(log.rates, np.float64)[:, 0]))
    model, curve, n, rates = runs[0]
    for k, v in model.state_dict().items():
        out[pre + "sd1/" + k] = v.numpy().copy()
    out[pre + "x"], out[pre + "y"] = x.numpy(), y.numpy()
    out[pre + "cfg"] = np.array(json.dumps(cfg, sort_keys=True))
    out[pre + "errors"] = curve[:n]
    out[pre + "rates"] = rates
    out[pre + "pert_errors"] = np.stack([r[1] for r in runs[1:]])
    out[pre + "pert_len"] = np.array([r[2] for r in runs[1:]], np.int64)
    out[pre + "flat"] = np.stack([flat_params(r[0]) for r in runs])
    check_case(name, cfg, runs)


def check_case(name, cfg, runs):
    """The two conditions the GPU tests rely on: a comparable prefix of at least 8 epochs, and every one of the
    runs passing the outcome rules against the others."""
    E = cfg["num_epochs"]
    curve, n = runs[0][1], runs[0][2]
    pert = np.stack([r[1] for r in runs[1:]])
    prefix = comparable_prefix(curve[:n], pert[:, :n])
    assert prefix >= 8, (name, prefix)
    finals = np.array([r[1][r[2] - 1] for r in runs])
    bests = np.array([np.nanmin(r[1]) for r in runs])
    lens = np.array([r[2] for r in runs])
    tail = curve[max(n - 51, 0):n]
    wobble = float(np.max(np.abs(np.diff(tail)))) if len(tail) > 1 else 0.0
    for i in range(len(runs)):
        rest = [j for j in range(len(runs)) if j != i]
        assert outcome_ok((finals[i], bests[i], lens[i]), finals[rest], bests[rest], lens[rest], wobble, E,
                          prefix), (name, i, finals, bests, lens, wobble)
    print(f"{name}: prefix {prefix} of {n}, lengths {lens.tolist()}, final {finals.min():.6g}..{finals.max():.6g}, "
          f"wobble {wobble:.3g}")


def pos_case(ref, name, cfg, out):
    import torch
    import torch.nn.functional as F
    rng = np.random.default_rng(cfg["seed"])
    n = cfg["n"]
    true_sens = sensors_xyz() + rng.normal(0, 0.004, (4, 3))
    pos = hits(rng, n)
    lags = sample_lags(rng, pos, true_sens, 335.0, [(0, 2), (1, 3)]).astype(np.float32)
    sensors0 = torch.tensor(sensors_xyz(), dtype=torch.float32)
    sounds0 = torch.tensor(pos + rng.normal(0, 0.003, pos.shape) * [1, 1, 0], dtype=torch.float32)
    pre = f"pos/{name}/"
    res = []
    for k in range(N_PERT + 1):
        curve = []

        def lossfun(a, b):
            v = F.mse_loss(a, b)
            curve.append(v.item())
            return v

        lk = torch.tensor(lags) * np.float32(1 + k * 2.0 ** -23)
        with AdamLog() as log:
            s, p, c = quiet(ref.calibration.optimize_positions, lk, sensors0.clone(), sounds0.clone(),
                            lossfun=lossfun, **cfg["args"])
        res.append((s.numpy().copy(), p.numpy().copy(), np.array(c.item(), np.float32),
                    np.array(curve, np.float32), len(log.rates), np.array(log.rates, np.float64)))
    out[pre + "lags"], out[pre + "sensors0"], out[pre + "sounds0"] = lags, sensors0.numpy(), sounds0.numpy()
    out[pre + "cfg"] = np.array(json.dumps(cfg, sort_keys=True))
    for key, i in (("sensors", 0), ("sounds", 1), ("C", 2), ("curve", 3), ("rates", 5)):
        out[pre + key] = res[0][i]
    out[pre + "steps"] = np.array(res[0][4], np.int64)
    E = cfg["args"].get("num_epochs", 1000)
    out[pre + "pert_sensors"] = np.stack([r[0] for r in res[1:]])
    out[pre + "pert_sounds"] = np.stack([r[1] for r in res[1:]])
    out[pre + "pert_C"] = np.stack([r[2] for r in res[1:]])
    out[pre + "pert_curve"] = np.stack([curve_array(r[3], E) for r in res[1:]])
    out[pre + "pert_steps"] = np.array([r[4] for r in res[1:]], np.int64)
    print(f"{name}: steps {[r[4] for r in res]}, final loss {res[0][3][-1]:.4g}, C {res[0][2]}")


def signature(fn):
    rows = []
    for p in inspect.signature(fn).parameters.values():
        if p.kind is p.VAR_KEYWORD:
            rows.append(["**" + p.name, None])
        elif p.default is p.empty:
            rows.append([p.name, "<required>"])
        elif callable(p.default):
            rows.append([p.name, p.default.__name__])
        else:
            rows.append([p.name, p.default])
    return np.array(json.dumps(rows))


def main():
    import torch
    torch.set_num_threads(1)
    ref = load_reference()
    out = {}
    for name, cfg in TRAIN.items():
        train_case(ref, name, cfg, out)
    for name, cfg in POS.items():
        pos_case(ref, name, cfg, out)
    for i, args in enumerate(LOC):
        out[f"loc/{i}/args"] = np.array(json.dumps(args, sort_keys=True))
        out[f"loc/{i}/out"] = np.array(ref.calibration.calibration_locations(**args), np.float64)
    for fn in ("train_location_model", "optimize_positions", "calibration_locations"):
        out["sig/" + fn] = signature(getattr(ref.calibration, fn))
    path = HERE / "g24_calibration.npz"
    write_npz(path, out)
    print(path, path.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
