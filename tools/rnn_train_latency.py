#!/usr/bin/env python3
"""Wall time per epoch of model.fit_rnn (one graph launch per epoch, csrc/ofp_rnn_train.hip) beside the same recipe as
a torch loop on the same GPU: the model's own rnn, layer_norm, attention and fc in training mode, model.loss, and the
optimiser and scheduler of RNN.configure_optimizers() (NAdam with weight decay 1e-4, CosineAnnealingLR(3000)), one full
batch per epoch.

    python tools/rnn_train_latency.py [--out profiles/rnn_train_latency.json] [--rounds 3] [--reps 3]
    python tools/rnn_train_latency.py --only ours --shapes default_B620 --rounds 1 --reps 1    (under a profiler)

The model is RNN(256, 2, 3) with the class defaults and dropout 0.  Both sides run in this one process, alternating,
`rounds` times.  A measurement is the host clock around `epochs` epochs that end in a device synchronise, divided by the
epochs; fit_rnn's figure therefore includes everything a call does (packing the parameters, the rate table, capturing
the graph, copying the result back).  Each round reports the p50 of `reps` such measurements per side, after one untimed
warm-up call of each.  A third side, `ours_dropout`, is fit_rnn alone with dropout_rate 0.5 and a seed: torch's own
dropout draws another stream, so it has no torch column.  One JSON record per shape, with the work space the plan asks
for."""
import argparse
import copy
import json
import statistics
import sys
import time
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))

SHAPES = {"default_B78": dict(n=78, epochs=20), "default_B620": dict(n=620, epochs=20)}
WIDTH, CHANNELS = 256, 3


def make(cfg, dropout_rate=0.0):
    import torch

    from onset_fingerprinting_amd import model
    torch.manual_seed(0)
    m = model.RNN(WIDTH, 2, CHANNELS, dropout_rate=dropout_rate).cuda()
    gen = torch.Generator().manual_seed(1)
    x = torch.randn(cfg["n"], CHANNELS, WIDTH, generator=gen).cuda()
    y = (torch.rand(cfg["n"], 2, generator=gen) - 0.5).cuda()
    return m, x, y


def ours(m, x, y, epochs, seed=None):
    import torch

    from onset_fingerprinting_amd import model
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fit = model.fit_rnn(m, x, y, max_epochs=epochs, seed=seed)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    assert fit.epochs == epochs
    return dt / epochs


def torch_loop(m, x, y, epochs):
    import torch
    m.train()
    opt = torch.optim.NAdam(m.parameters(), lr=m.lr, weight_decay=1e-4)
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, 3000)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(epochs):
        opt.zero_grad()
        h, _ = m.rnn(x.permute(0, 2, 1))
        h = m.layer_norm(h)
        h, _ = m.attention(h, h, h, need_weights=False)
        loss = m.loss(m.fc(h.mean(1)), y)
        loss.backward()
        opt.step()
        sched.step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / epochs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--shapes", nargs="*", default=list(SHAPES))
    ap.add_argument("--only", choices=("ours", "torch", "ours_dropout"), default=None,
                    help="one side alone (for a kernel trace)")
    args = ap.parse_args()
    import torch

    from onset_fingerprinting_amd import model
    records = []
    for name in args.shapes:
        cfg = SHAPES[name]
        start, x, y = make(cfg)
        dropped = make(cfg, 0.5)[0]
        E = cfg["epochs"]
        run = {"ours": lambda: ours(copy.deepcopy(start), x, y, E),
               "torch": lambda: torch_loop(copy.deepcopy(start), x, y, E),
               "ours_dropout": lambda: ours(copy.deepcopy(dropped), x, y, E, seed=1)}
        if args.only:
            run = {args.only: run[args.only]}
        for fn in run.values():  # code objects, the libraries' choice of algorithm
            fn()
        rounds = []
        for _ in range(args.rounds):
            rounds.append({side: statistics.median(fn() for _ in range(args.reps)) * 1e6 for side, fn in run.items()})
        rec = dict(tool="rnn_train_latency", shape=name, n=cfg["n"], model="RNN(256, 2, 3)", width=WIDTH,
                   channels=CHANNELS, epochs_per_measurement=E, reps=args.reps,
                   p50_us_per_epoch=[{k: round(v, 2) for k, v in r.items()} for r in rounds],
                   workspace_bytes=model.rnn_train_workspace_bytes(start, cfg["n"], 0, WIDTH),
                   workspace_bytes_dropout=model.rnn_train_workspace_bytes(dropped, cfg["n"], 0, WIDTH, seed=1),
                   device=torch.cuda.get_device_name(0))
        if not args.only:
            rec["torch_over_ours"] = [round(r["torch"] / r["ours"], 3) for r in rounds]
        print(json.dumps(rec), flush=True)
        records.append(rec)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(records, indent=1) + "\n")


if __name__ == "__main__":
    main()
