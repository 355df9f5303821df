#!/usr/bin/env python3
"""Wall time per epoch of model.fit_cnn (one graph launch per epoch, csrc/ofp_cnn_train.hip) beside the same
recipe as a torch loop on the same GPU: the model's own conv_layers and fc in training mode, model.loss, and the
optimiser and scheduler of configure_optimizers(), one full batch per epoch.

    python tools/cnn_train_latency.py [--out results/cnn_train_latency.jsonl] [--rounds 3] [--reps 5]

Both run in this one process, alternating, `rounds` times.  A measurement is the host clock around `epochs` epochs
that end in a device synchronise, divided by the epochs; fit_cnn's figure therefore includes everything a call does
(packing the parameters, the rate table, capturing the graph, copying the result back).  Each round reports the p50
of `reps` such measurements per side, after one untimed warm-up call of each.  One JSON line per shape.

    python tools/cnn_train_latency.py --random [--modes p0 p0.5 p0.5_shift p0.5_shift_stretch] [--repo OTHER_TREE]

measures what the trainer's own random stream costs at the default architecture (default_bn_B620): fit_cnn with
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

SHAPES = {
    "default_bn_B78": dict(n=78, layer_sizes=[8, 16], kernel_size=3, padding=1, epochs=200),
    "default_bn_B620": dict(n=620, layer_sizes=[8, 16], kernel_size=3, padding=1, epochs=200),
    "wide_128x128_k5_B620": dict(n=620, layer_sizes=[128, 128], kernel_size=5, padding=2, epochs=10),
}
WIDTH, CHANNELS = 264, 4


RANDOM_SHAPE, RANDOM_MODES = "default_bn_B620", ("p0", "p0.5", "p0.5_shift", "p0.5_shift_stretch")
MAX_SHIFT, EXTRACTIONS, SEED = 16, 4, 1  # train.py: MCPOSD.from_file(..., w, pre_samp, 16, 4)
MAX_STRETCH = 0.03                       # train.py: data.StretchFrameExtractor(w, 0, 0.03), commented out there


def make(cfg, dropout_rate=0.0):
    import torch

    from onset_fingerprinting_amd import model
    torch.manual_seed(0)
    m = model.CNN(WIDTH, 2, CHANNELS, cfg["layer_sizes"], cfg["kernel_size"], dropout_rate=dropout_rate,
                  batch_norm=True, padding=cfg["padding"]).cuda()
    gen = torch.Generator().manual_seed(1)
    x = torch.randn(cfg["n"], CHANNELS, WIDTH, generator=gen).cuda()
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
    fit = model.fit_cnn(m, x, y, max_epochs=epochs, **kw)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    assert fit.epochs == epochs
    return dt / epochs


def torch_loop(m, x, y, epochs):
    import torch
    m.train()
    conf = m.configure_optimizers()
    opt, sched = conf["optimizer"], conf["lr_scheduler"]["scheduler"]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(epochs):
        opt.zero_grad()
        loss = m.loss(m.fc(torch.flatten(m.conv_layers(x), start_dim=1)), y)
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
            x, y = window_source(cfg["n"], CHANNELS, WIDTH, stretch=mode.endswith("_stretch"))
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
    rec = dict(tool="cnn_train_latency --random", tree=str(REPO.name), shape=RANDOM_SHAPE, n=cfg["n"],
               layer_sizes=cfg["layer_sizes"], width=WIDTH, channels=CHANNELS, batch_norm=True, max_shift=MAX_SHIFT,
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
        rec = dict(shape=name, n=cfg["n"], layer_sizes=cfg["layer_sizes"], kernel_size=cfg["kernel_size"],
                   width=WIDTH, channels=CHANNELS, batch_norm=True, epochs_per_measurement=E, reps=args.reps,
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
