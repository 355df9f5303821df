#!/usr/bin/env python3
"""Wall time per epoch of model.fit_cnn (one graph launch per epoch, csrc/ofp_cnn_train.hip) beside the same
recipe as a torch loop on the same GPU: the model's own conv_layers and fc in training mode, model.loss, and the
optimiser and scheduler of configure_optimizers(), one full batch per epoch.

    python tools/cnn_train_latency.py [--out results/cnn_train_latency.jsonl] [--rounds 3] [--reps 5]

Both run in this one process, alternating, `rounds` times.  A measurement is the host clock around `epochs` epochs
that end in a device synchronise, divided by the epochs; fit_cnn's figure therefore includes everything a call does
(packing the parameters, the rate table, capturing the graph, copying the result back).  Each round reports the p50
of `reps` such measurements per side, after one untimed warm-up call of each.  One JSON line per shape."""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))

SHAPES = {
    "default_bn_B78": dict(n=78, layer_sizes=[8, 16], kernel_size=3, padding=1, epochs=200),
    "default_bn_B620": dict(n=620, layer_sizes=[8, 16], kernel_size=3, padding=1, epochs=200),
    "wide_128x128_k5_B620": dict(n=620, layer_sizes=[128, 128], kernel_size=5, padding=2, epochs=10),
}
WIDTH, CHANNELS = 264, 4


def make(cfg):
    import torch

    from onset_fingerprinting_amd import model
    torch.manual_seed(0)
    m = model.CNN(WIDTH, 2, CHANNELS, cfg["layer_sizes"], cfg["kernel_size"], dropout_rate=0.0, batch_norm=True,
                  padding=cfg["padding"]).cuda()
    gen = torch.Generator().manual_seed(1)
    x = torch.randn(cfg["n"], CHANNELS, WIDTH, generator=gen).cuda()
    y = (torch.rand(cfg["n"], 2, generator=gen) - 0.5).cuda()
    return m, x, y


def ours(m, x, y, epochs):
    import torch

    from onset_fingerprinting_amd import model
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fit = model.fit_cnn(m, x, y, max_epochs=epochs)
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", nargs="*", default=list(SHAPES))
    args = ap.parse_args()
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
