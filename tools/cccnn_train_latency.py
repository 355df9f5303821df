#!/usr/bin/env python3
"""Wall time per epoch of model.fit_lcccnn (one graph launch per epoch, csrc/ofp_cccnn_train.hip) beside the same
recipe as a torch loop on the same GPU: the module's own conv_layers and fc, the correlation head written with
F.conv1d as the reference writes it, model.loss, and the optimiser and scheduler of configure_optimizers(), one full
batch per epoch.

    python tools/cccnn_train_latency.py [--out profiles/cccnn_train_latency.json] [--rounds 3] [--reps 5]

Both run in this one process, alternating, `rounds` times.  A measurement is the host clock around `epochs` epochs
that end in a device synchronise, divided by the epochs; fit_lcccnn's figure therefore includes everything a call
does (packing the parameters, the rates, capturing the graph, copying the result back).  Each round reports the p50
of `reps` such measurements per side, after one untimed warm-up call of each.  One JSON line per shape.

    python tools/cccnn_train_latency.py --random [--modes p0 p0.5 p0.5_shift p0.5_shift_stretch] [--repo OTHER_TREE]

measures what the trainer's own random stream costs at the class defaults (defaults_B620): fit_lcccnn with
dropout_rate 0 (the chain without any of the new kernels), with dropout_rate 0.5 and a seed (k_dropout_fwd and
k_dropout_bwd per epoch), and with that plus a data.ShiftedWindows source of 155 onsets x 4 extractions shifted by up
to 16 samples (k_shift_windows as well), and with a data.StretchedWindows source of the same hits that also stretches
by max_stretch 0.03 (a span of 7: k_stretch_windows in place of k_shift_windows), alternating over `rounds` rounds in
this one process.  `--repo` imports the package from another built tree (a checkout of the parent commit, which lacks
the newest mode: name the others with --modes), so that both can be measured in one visit to the GPU."""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
if "--repo" in sys.argv:
    REPO = Path(sys.argv[sys.argv.index("--repo") + 1]).resolve()
sys.path.insert(0, str(REPO))

# train.py's own configuration at its smallest and largest training set, and the class defaults
_TRAIN = dict(width=256, channels=4, layer_sizes=[5] * 7, kernel_sizes=[1, 33, 64, 15, 15, 15, 1], batch_norm=True)
SHAPES = {
    "train_py_B78": dict(_TRAIN, n=78, epochs=50),
    "train_py_B620": dict(_TRAIN, n=620, epochs=20),
    "defaults_B620": dict(width=256, channels=3, layer_sizes=[8, 16], kernel_sizes=3, batch_norm=False, n=620,
                          epochs=50),
}


RANDOM_SHAPE, RANDOM_MODES = "defaults_B620", ("p0", "p0.5", "p0.5_shift", "p0.5_shift_stretch")
MAX_SHIFT, EXTRACTIONS, SEED = 16, 4, 1  # train.py: MCPOSD.from_file(..., w, pre_samp, 16, 4)
MAX_STRETCH = 0.03                       # train.py: data.StretchFrameExtractor(w, 0, 0.03), commented out there


def make(cfg, dropout_rate=0.0):
    import torch

    from onset_fingerprinting_amd import model
    torch.manual_seed(0)
    m = model.LCCCNN(cfg["width"], 2, cfg["channels"], layer_sizes=cfg["layer_sizes"],
                     kernel_sizes=cfg["kernel_sizes"], dropout_rate=dropout_rate, batch_norm=cfg["batch_norm"]).cuda()
    gen = torch.Generator().manual_seed(1)
    x = torch.randn(cfg["n"], cfg["channels"], cfg["width"], generator=gen).cuda()
    y = (torch.rand(cfg["n"], 2, generator=gen) - 0.5).cuda()
    return m, x, y


def window_source(n, channels, width, stretch=False):
    """(data.ShiftedWindows -- with `stretch` data.StretchedWindows -- of n / EXTRACTIONS onsets in seeded noise,
    y [onsets, 2])."""
    import numpy as np
    import torch

    from onset_fingerprinting_amd import data
    onsets_n = n // EXTRACTIONS
    assert onsets_n * EXTRACTIONS == n
    gap = width + 2 * MAX_SHIFT + 8
    rng = np.random.default_rng(1)
    audio = rng.standard_normal((gap * (onsets_n + 1), channels)).astype(np.float32)
    onsets = gap * (1 + np.arange(onsets_n))
    if stretch:  # (the gap's 8 spare samples hold the longest window's span - 1 more)
        src = data.StretchedWindows(audio, onsets, width, pre_samples=8, max_stretch=MAX_STRETCH, max_shift=MAX_SHIFT,
                                    n_extractions=EXTRACTIONS)
    else:
        src = data.ShiftedWindows(audio, onsets, width, pre_samples=8, max_shift=MAX_SHIFT, n_extractions=EXTRACTIONS)
    return src, torch.from_numpy((rng.random((onsets_n, 2)) - 0.5).astype(np.float32)).cuda()


def ours(m, x, y, epochs, **kw):
    import torch

    from onset_fingerprinting_amd import model
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fit = model.fit_lcccnn(m, x, y, max_epochs=epochs, **kw)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    assert fit.epochs == epochs
    return dt / epochs


def torch_forward(net, x):
    """model.py:513-538 over the torch layers of a CCCNN."""
    import torch
    import torch.nn.functional as F
    B, C, W = x.shape
    h = net.conv_layers(x if net.group else x.reshape(B * C, 1, W))
    V = h.shape[-1]
    f = h.reshape(B * C, -1, V)
    BC, K, _ = f.shape
    cc = F.conv1d(f.reshape(1, BC * K, V), f.reshape(BC * K, 1, V), groups=BC * K, padding=V - 1)
    probs = F.softmax(cc.view(BC, K, -1).sum(dim=1), dim=-1).view(B, C, -1)
    return net.fc(torch.flatten(probs, start_dim=1))


def torch_loop(m, x, y, epochs):
    import torch
    m.train()
    conf = m.configure_optimizers()
    opt, sched = conf["optimizer"], conf["lr_scheduler"]["scheduler"]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(epochs):
        opt.zero_grad()
        loss = m.loss(torch_forward(m.model, x), y)
        loss.backward()
        opt.step()
        sched.step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / epochs


def random_modes(args):
    """One JSON line: p50 us per epoch of every mode in every round, the modes alternating inside a round."""
    import copy

    import torch
    cfg = SHAPES[RANDOM_SHAPE]
    E = cfg["epochs"]
    run = {}
    for mode in args.modes:
        start, x, y = make(cfg, 0.0 if mode == "p0" else 0.5)
        kw = {} if mode == "p0" else dict(seed=SEED)
        if "_shift" in mode:
            x, y = window_source(cfg["n"], cfg["channels"], cfg["width"], stretch=mode.endswith("_stretch"))
        run[mode] = lambda start=start, x=x, y=y, kw=kw: ours(copy.deepcopy(start), x, y, E, **kw)
    for fn in run.values():
        fn()
    rounds = []
    for _ in range(args.rounds):
        samples = {mode: [] for mode in run}
        for _rep in range(args.reps):
            for mode, fn in run.items():
                samples[mode].append(fn())
        rounds.append({mode: round(statistics.median(v) * 1e6, 2) for mode, v in samples.items()})
    rec = dict(tool="cccnn_train_latency --random", tree=str(REPO.name), shape=RANDOM_SHAPE, n=cfg["n"],
               layer_sizes=cfg["layer_sizes"], kernel_sizes=cfg["kernel_sizes"], width=cfg["width"],
               channels=cfg["channels"], batch_norm=cfg["batch_norm"], max_shift=MAX_SHIFT,
               n_extractions=EXTRACTIONS, max_stretch=MAX_STRETCH, epochs_per_measurement=E, reps=args.reps,
               p50_us_per_epoch=rounds,
               device=torch.cuda.get_device_name(0))
    print(json.dumps(rec), flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        with open(args.out, "a") as f:
            f.write(json.dumps(rec) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", nargs="*", default=list(SHAPES))
    ap.add_argument("--random", action="store_true", help="the cost of dropout and shifted windows (see above)")
    ap.add_argument("--modes", nargs="*", default=list(RANDOM_MODES), choices=RANDOM_MODES)
    ap.add_argument("--repo", default=None, help="import the package from this built tree")
    args = ap.parse_args()
    if args.random:
        return random_modes(args)
    import copy

    import torch
    lines = []
    for name in args.shapes:
        cfg = SHAPES[name]
        start, x, y = make(cfg)
        E = cfg["epochs"]
        run = {"ours": lambda: ours(copy.deepcopy(start), x, y, E),
               "torch": lambda: torch_loop(copy.deepcopy(start), x, y, E)}
        for fn in run.values():  # code objects, MIOpen's choice of algorithm
            fn()
        rounds = []
        for _ in range(args.rounds):
            rounds.append({side: statistics.median(fn() for _ in range(args.reps)) * 1e6 for side, fn in run.items()})
        rec = dict(shape=name, n=cfg["n"], layer_sizes=cfg["layer_sizes"], kernel_sizes=cfg["kernel_sizes"],
                   width=cfg["width"], channels=cfg["channels"], batch_norm=cfg["batch_norm"],
                   epochs_per_measurement=E, reps=args.reps,
                   p50_us_per_epoch=[{k: round(v, 2) for k, v in r.items()} for r in rounds],
                   ours_lower_in_every_round=all(r["ours"] < r["torch"] for r in rounds),
                   device=torch.cuda.get_device_name(0))
        print(json.dumps(rec), flush=True)
        lines.append(json.dumps(rec))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
