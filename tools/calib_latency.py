#!/usr/bin/env python3
"""Time of calibration.train_location_model / optimize_positions (one launch per call, csrc/ofp_train.hip) for
M = 1, 256 and 4 096 independent problems, beside the same loop written with plain torch modules on the same GPU
and on one host core.

    python tools/calib_latency.py [--out results/calib_latency.jsonl]

Every measurement runs in a fresh child process under its own `timeout -k 10 <s>`; the driver stops at the first
child that fails, times out or dies on a signal.  The HIP figures are HIP events around `iters` launches on prepared
device tensors after `warmup` launches, median over `repeats`; early stopping is disabled (patience = num_epochs)
so that every run does the same work.  The torch loops are timed once each with the wall clock (they synchronise
every epoch).  One JSON line per measurement, with the barriers per epoch and the bytes of LDS the case needs.
"""
import argparse
import json
import statistics
import subprocess
import sys
import time
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]

FCNN = {
    "fcnn_3-6-2": dict(n=164, epochs=3000, lr=0.0015,
                       kwargs=dict(hidden_layers=[6], activation="SiLU", batch_norm=False, bias=False)),
    "fcnn_default": dict(n=164, epochs=1000, lr=0.01, kwargs={}),
}
JOBS = ([("hip", c, m) for c in FCNN for m in (1, 256, 4096)] + [("tdoa", "tdoa", n) for n in (84, 4096)] +
        [("torch_gpu", c, 1) for c in FCNN] + [("torch_cpu", c, 1) for c in FCNN])


def data(n, seed=0):
    import torch
    gen = torch.Generator().manual_seed(seed)
    pos = torch.rand(n, 3, generator=gen) - 0.5
    pos[:, 2] = 0
    sens = torch.tensor([[0.9, 0, 0], [0, 0.9, 0], [-0.9, 0, 0], [0, -0.9, 0]]) * 0.5
    d = (pos[:, None] - sens[None]).norm(dim=-1)
    return (d[:, 1:] - d[:, :1]) * 2, pos, sens, d


def make_model(cfg):
    import torch
    from torch import nn

    from onset_fingerprinting_amd import calibration
    kw = dict(cfg["kwargs"])
    if "activation" in kw:
        kw["activation"] = getattr(nn, kw["activation"])
    torch.manual_seed(0)
    return calibration.FCNN(3, 2, **kw)


def events(fn, warmup, iters, repeats):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / iters)
    return statistics.median(out)  # ms per call


def child_hip(name, M, args):
    import torch

    from onset_fingerprinting_amd import calibration
    cfg = FCNN[name]
    model = make_model(cfg)
    x, pos, _s, _d = data(cfg["n"])
    E = cfg["epochs"]
    dims, act, bn, bias, _l, _b = calibration._fcnn_arch(model)
    p, s = calibration._pack(model)
    gen = torch.Generator().manual_seed(1)
    p0 = (p[None] + 0.01 * torch.randn(M, p.numel(), generator=gen)).cuda()
    s0 = s[None].repeat(M, 1).cuda()
    table = torch.from_numpy(calibration.location_model_rate_table(cfg["lr"], E)[None].copy()).cuda()
    rows = torch.zeros(M, dtype=torch.int32, device="cuda")
    xd, yd = x.cuda(), pos[:, :2].contiguous().cuda()
    run = lambda: calibration._fcnn_train_launch((dims, act, bn, bias), 0, xd, yd, p0, s0, table, rows, E, 1e-9, E)
    ms = events(run, args.warmup, args.iters, args.repeats)
    assert int(run()[3].min()) == E
    L = len(dims) - 1
    return dict(kind="hip", config=name, M=M, n=cfg["n"], epochs=E, ms_per_call=round(ms, 3),
                us_per_epoch=round(ms * 1000 / E, 3), barriers_per_epoch=2 * L + 1 + (L - 1 if bn else 0),
                lds_bytes=calibration.fcnn_train_lds_bytes(model, cfg["n"]))


def child_tdoa(n, args):
    import torch

    from onset_fingerprinting_amd import calibration
    _x, pos, sens, d = data(n)
    lags = ((torch.stack([d[:, 0] - d[:, 2], d[:, 1] - d[:, 3]], 1) / 342.29 * 96000).round()).cuda()
    E = 1000
    run = lambda: calibration.optimize_positions_device(lags, sens * 1.01, pos, num_epochs=E, patience=E)
    t0 = time.perf_counter()
    for _ in range(args.warmup):
        run()
    torch.cuda.synchronize()
    ms = []
    for _ in range(args.repeats):  # the call prepares its inputs on the host; the wall clock includes that
        t0 = time.perf_counter()
        fit = run()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1000)
    assert int(fit.epochs[0]) == E
    ms = statistics.median(ms)
    return dict(kind="hip", config="optimize_positions", M=1, n=n, epochs=E, ms_per_call=round(ms, 3),
                us_per_epoch=round(ms * 1000 / E, 3), barriers_per_epoch=1, lds_bytes=n * 32)


def child_torch(name, device, args):
    """train_location_model's loop on the FCNN's own torch modules."""
    import torch
    import torch.nn.functional as F
    torch.set_num_threads(1)
    cfg = FCNN[name]
    net = make_model(cfg).network.to(device).train()
    x, pos, _s, _d = data(cfg["n"])
    x, y = x.to(device), pos[:, :2].to(device)
    E = cfg["epochs"]
    if device == "cuda":  # warm the allocator and the kernels' code objects
        F.l1_loss(net(x), y).backward()
        net.zero_grad()
        torch.cuda.synchronize()
    opt = torch.optim.Adam(net.parameters(), lr=cfg["lr"])
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, E / 10)
    last = torch.inf
    t0 = time.perf_counter()
    for _ in range(E):
        opt.zero_grad(set_to_none=True)
        loss = F.l1_loss(net(x), y)
        if loss < last - 1e-9:  # the reference's early-stop test: one synchronisation per epoch
            last = loss
        loss.backward()
        torch.nn.utils.clip_grad_norm_(net.parameters(), 1)
        opt.step()
        sched.step()
    if device == "cuda":
        torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1000
    return dict(kind="torch_" + ("gpu" if device == "cuda" else "cpu_1core"), config=name, M=1, n=cfg["n"], epochs=E,
                ms_per_call=round(ms, 1), us_per_epoch=round(ms * 1000 / E, 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", nargs=3, metavar=("KIND", "CONFIG", "SIZE"))
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=240, help="seconds per measurement")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.child:
        sys.path.insert(0, str(REPO))
        kind, name, size = args.child[0], args.child[1], int(args.child[2])
        if kind == "hip":
            row = child_hip(name, size, args)
        elif kind == "tdoa":
            row = child_tdoa(size, args)
        else:
            row = child_torch(name, "cuda" if kind == "torch_gpu" else "cpu", args)
        print(json.dumps(row), flush=True)
        return
    lines = []
    for kind, name, size in JOBS:
        cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, __file__, "--child", kind, name, str(size),
               "--warmup", str(args.warmup), "--iters", str(args.iters), "--repeats", str(args.repeats)]
        p = subprocess.run(cmd, capture_output=True, text=True)
        if p.returncode != 0:
            sys.stderr.write(p.stdout + p.stderr)
            print(f"{kind} {name} {size}: exit status {p.returncode}; stopping", file=sys.stderr)
            break
        line = p.stdout.strip().splitlines()[-1]
        print(line, flush=True)
        lines.append(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")
    if len(lines) != len(JOBS):
        sys.exit(1)


if __name__ == "__main__":
    main()
