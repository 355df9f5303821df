#!/usr/bin/env python3
"""Wall time per epoch of model.fit_lcccnn (one graph launch per epoch, csrc/ofp_cccnn_train.hip) beside the same
recipe as a torch loop on the same GPU: the module's own conv_layers and fc, the correlation head written with
F.conv1d as the reference writes it, model.loss, and the optimiser and scheduler of configure_optimizers(), one full
batch per epoch.

    python tools/cccnn_train_latency.py [--out profiles/cccnn_train_latency.json] [--rounds 3] [--reps 5]

Both run in this one process, alternating, `rounds` times.  A measurement is the host clock around `epochs` epochs
that end in a device synchronise, divided by the epochs; fit_lcccnn's figure therefore includes everything a call
does (packing the parameters, the rates, capturing the graph, copying the result back).  Each round reports the p50
of `reps` such measurements per side, after one untimed warm-up call of each.  One JSON line per shape."""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))

# train.py's own configuration at its smallest and largest training set, and the class defaults
_TRAIN = dict(width=256, channels=4, layer_sizes=[5] * 7, kernel_sizes=[1, 33, 64, 15, 15, 15, 1], batch_norm=True)
SHAPES = {
    "train_py_B78": dict(_TRAIN, n=78, epochs=50),
    "train_py_B620": dict(_TRAIN, n=620, epochs=20),
    "defaults_B620": dict(width=256, channels=3, layer_sizes=[8, 16], kernel_sizes=3, batch_norm=False, n=620,
                          epochs=50),
}


def make(cfg):
    import torch

    from onset_fingerprinting_amd import model
    torch.manual_seed(0)
    m = model.LCCCNN(cfg["width"], 2, cfg["channels"], layer_sizes=cfg["layer_sizes"],
                     kernel_sizes=cfg["kernel_sizes"], dropout_rate=0.0, batch_norm=cfg["batch_norm"]).cuda()
    gen = torch.Generator().manual_seed(1)
    x = torch.randn(cfg["n"], cfg["channels"], cfg["width"], generator=gen).cuda()
    y = (torch.rand(cfg["n"], 2, generator=gen) - 0.5).cuda()
    return m, x, y


def ours(m, x, y, epochs):
    import torch

    from onset_fingerprinting_amd import model
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fit = model.fit_lcccnn(m, x, y, max_epochs=epochs)
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
