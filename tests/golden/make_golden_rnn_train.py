#!/usr/bin/env python3
"""Golden vectors g29_rnn_train: the reference's model.RNN trained by its own training_step and configure_optimizers
(NAdam with weight decay 1e-4, CosineAnnealingLR(3000)), one full batch per epoch, with torch on the host, one thread.

Run in the build container only:   python tests/golden/make_golden_rnn_train.py
A second run writes the same bytes.

Built like make_golden_cnnrnn_train.py, whose loop, per-case contents and conditions (check_case) it imports; only the
module that is built differs.  dropout_rate is 0.0, so neither nn.GRU's dropout between the layers nor the
attention's draws anything.  Every run is repeated 8 times with the inputs scaled by (1 + k * 2^-23), k = 1..8, and
once in float64; tests/test_gpu_rnn_train.py derives its bounds from how far the reference strays from itself.

Contents: the keys of g26_cnn_train (make_golden_cnn_train.py), every key prefixed by <case>/; `stats` is empty, the
network has no running statistics.
"""
import sys
import warnings
from pathlib import Path

HERE = Path(__file__).resolve().parent
REPO = HERE.parents[1]
sys.path.insert(0, str(HERE))
sys.path.insert(0, str(REPO))

import make_golden_cnnrnn_train as base  # noqa: E402
from _refload import load_reference  # noqa: E402
from make_golden_locate import write_npz  # noqa: E402

warnings.filterwarnings("ignore")

EPOCHS = 300

_FIRST = dict(hidden_size=8, num_layers=2, num_heads=2, loss="l1_loss")
CASES = {
    "l1_two_layers": dict(n=24, channels=3, width=32, lr=0.01, seed=3, epochs=EPOCHS, kwargs=_FIRST),
    "mse_one_layer": dict(n=20, channels=4, width=24, lr=0.003, seed=7, epochs=EPOCHS,
                          kwargs=dict(hidden_size=6, num_layers=1, num_heads=3, loss="mse_loss")),
    "l1_three_layers": dict(n=37, channels=4, width=40, lr=0.003, seed=5, epochs=EPOCHS,
                            kwargs=dict(hidden_size=16, num_layers=3, num_heads=2, loss="l1_loss")),
    # the first case with another seed, a validation set and a patience that ends it early
    "l1_stop": dict(n=24, channels=3, width=32, lr=0.01, seed=9, epochs=EPOCHS, n_val=16, patience=4, kwargs=_FIRST),
}


def build(ref, cfg, state=None, dtype=None):
    import torch
    import torch.nn.functional as F
    kw = dict(cfg["kwargs"])
    kw["loss"] = getattr(F, kw["loss"])
    torch.manual_seed(cfg["seed"])
    m = ref.model.RNN(cfg["width"], 2, channels=cfg["channels"], dropout_rate=0.0, lr=cfg["lr"], **kw)
    m.log = lambda *a, **k: None
    if state is not None:
        m.load_state_dict(state)
    if dtype is not None:
        m = m.to(dtype)
    return m


def check_case(name, cfg, runs, ran64):
    """What the tests rely on.  A case trained to its full length: a comparable prefix of at least 24 epochs with all
    eight disturbed runs, and a network that learns (the best loss is at most the first divided by 1.2).  The stop
    case, which ends after 11 epochs: every epoch it ran is comparable, all ten runs stop at the same epoch before the
    full length, and a patience one shorter would have stopped earlier (the stop is not the first stall)."""
    import numpy as np
    curve, ran = runs[0][1], runs[0][4]
    pert = np.stack([base.padded(r[1], cfg["epochs"]) for r in runs[1:]])
    prefix = base.comparable_prefix(curve.astype(np.float32), pert[:, :ran])
    finals = [float(r[1][-1]) for r in runs]
    print(f"{name}: prefix {prefix} of {ran}, loss {curve[0]:.5g} -> {curve[-1]:.5g} (best {curve.min():.5g}), "
          f"finals {min(finals):.5g} .. {max(finals):.5g}, epochs run {[r[4] for r in runs]} and {ran64} in float64")
    if "patience" not in cfg:
        assert ran == cfg["epochs"] and prefix >= base.MIN_PREFIX, (name, prefix)
        assert curve.min() * 1.2 <= curve[0], (name, curve[0], curve.min())
        return
    assert ran < cfg["epochs"] and prefix == ran, (name, prefix, ran)
    assert all(r[4] == ran for r in runs) and ran64 == ran, (name, [r[4] for r in runs], ran64)
    best, wait, first = float("inf"), 0, None
    for e, v in enumerate(runs[0][3]):
        best, wait = (v, 0) if v < best else (best, wait + 1)
        if wait >= cfg["patience"] - 1 and first is None:
            first = e + 1
    print(f"{name}: stops after {ran} epochs; patience {cfg['patience'] - 1} would stop after {first}")
    assert first is not None and first < ran, (name, first, ran)


def main():
    import torch
    torch.set_num_threads(1)
    ref = load_reference()
    base.build, base.check_case = build, check_case  # fit and run_case of the CNNRNN generator, on this module
    out = {}
    for name, cfg in CASES.items():
        base.run_case(ref, name, cfg, out)
    path = HERE / "g29_rnn_train.npz"
    write_npz(path, out)
    print(path, path.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
