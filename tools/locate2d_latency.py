#!/usr/bin/env python3
"""Latency and throughput of the 2-D grid-voting locator (onset_fingerprinting_amd.multilateration:
MultilateratePaired, find_lags_device), the reference's default millimetre grid: four drumhead sensors at 0.9 r,
96 kHz, scale 10 (357 x 357 lag maps), 256-sample windows.

    python tools/locate2d_latency.py [--out results/locate2d_latency.json]

  locate_cc   one MultilateratePaired.locate_cc call (with its vote grid ``res``): host clock around the call, which
              ends in device synchronisations of its own
  batched     locate_cc_device over B = 1, 10^3, 10^5 hits: HIP events around `iters` calls after warm-up, the
              recording, maps and vote index resident on the GPU
  find_lags   find_lags_device throughput on 256-sample row pairs (argmax only, and with the top 3 peaks)
  host numpy  the reference's locate_cc on one CPU core: two np.correlate calls, the vote over both neighbour maps
              and the argmax, restated here because the reference does not travel with the project
"""
import argparse
import json
import os
import sys

os.environ.setdefault("OMP_NUM_THREADS", "1")  # the host comparison runs on one core
import time
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))

LAYOUT = dict(sensor_locations=[(0.9, 0), (0.9, 90), (0.9, 180), (0.9, 270)], scale=10, medium="drumhead",
              sr=96000)
RIGHT = 256


def recording(m, n_hits, seed=0, spacing=600):
    """[N, 4] float32: decaying bursts reaching sensor k after |p - s_k| / c * sr samples; onsets and first sensors."""
    rng = np.random.default_rng(seed)
    from onset_fingerprinting_amd import multilateration as ml
    c = ml.speed_of_sound(100 * m.scale, medium="drumhead")
    S = len(m.sensor_locs)
    N = spacing * n_hits + 1000
    x = 1e-3 * rng.standard_normal((N, S)).astype(np.float32)
    ang, rad = rng.uniform(0, 2 * np.pi, n_hits), m.radius * 0.8 * np.sqrt(rng.uniform(0, 1, n_hits))
    s = np.array(m.sensor_locs)
    onsets, first = np.zeros(n_hits, np.int64), np.zeros(n_hits, np.int32)
    t = np.arange(300)
    for h in range(n_hits):
        d = np.hypot(rad[h] * np.cos(ang[h]) - s[:, 0], rad[h] * np.sin(ang[h]) - s[:, 1]) / c * m.sr
        i = int(np.argmin(d))
        t0 = 200 + h * spacing
        for k in range(S):
            o = t0 + int(round(d[k] - d[i]))
            x[o:o + 300, k] += (np.exp(-t / 30.0) * rng.standard_normal(300)).astype(np.float32)
        onsets[h], first[h] = t0, i
    return x, onsets, first


def host_locate_cc(m, x, onset, i, tol=2, left=0, right=RIGHT):
    """multilateration.py:836-875 on the host."""
    res = np.zeros_like(m.lag_maps[0][1])
    for j, lm in m.lag_maps[i].items():
        a, b = x[onset - left:onset + right, i], x[onset - left:onset + right, j]
        lag = np.argmax(np.correlate(a, b, mode="full")) - (len(a) - 1)
        res += (lm < lag + tol) & (lm > lag - tol)
    row, col = np.unravel_index(np.argmax(res), res.shape)
    xc, yc = col - (res.shape[1] - 1) / 2, (res.shape[0] - 1) / 2 - row
    return np.sqrt(xc ** 2 + yc ** 2) / m.radius, np.degrees(np.arctan2(yc, xc) % (2 * np.pi))


def events(fn, iters):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--iters", type=int, default=50)
    args = ap.parse_args()
    import torch

    from onset_fingerprinting_amd import multilateration as ml
    torch.set_num_threads(1)
    dev = torch.device("cuda", 0)
    t0 = time.perf_counter()
    m = ml.MultilateratePaired(**LAYOUT)
    torch.cuda.synchronize()
    res = {"layout": LAYOUT, "device": torch.cuda.get_device_name(0),
           "construct_ms": (time.perf_counter() - t0) * 1e3, "n_buckets": m.n_buckets}

    x, onsets, first = recording(m, 1000, seed=1)
    times = []
    for it in range(args.iters + 10):
        h = it % len(onsets)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        m.locate_cc(x, int(onsets[h]), int(first[h]))
        if it >= 10:
            times.append((time.perf_counter() - t0) * 1e6)
    res["locate_cc_us"] = {"p50": float(np.median(times)), "p90": float(np.percentile(times, 90)),
                           "calls": len(times)}

    res["batched"] = {}
    xd = torch.from_numpy(x).to(dev)
    for B in (1, 1000, 100000):
        sel = np.arange(B) % len(onsets)
        on = torch.from_numpy(onsets[sel]).to(dev)
        fi = torch.from_numpy(first[sel]).to(dev)
        for _ in range(3):
            m.locate_cc_device(xd, on, fi)
        torch.cuda.synchronize()
        ms, (_, cell, st) = events(lambda: m.locate_cc_device(xd, on, fi), max(5, min(args.iters, 2000000 // B)))
        res["batched"][str(B)] = {"ms_per_call": ms, "hits_per_s": B / (ms * 1e-3),
                                  "ok": int((st == 0).sum().item())}

    res["find_lags"] = {}
    n = 100000
    a = torch.randn((n, RIGHT), dtype=torch.float32, device=dev)
    b = torch.randn((n, RIGHT), dtype=torch.float32, device=dev)
    for top_n in (0, 3):
        ml.find_lags_device(a, b, top_n)
        torch.cuda.synchronize()
        ms, _ = events(lambda: ml.find_lags_device(a, b, top_n), 10)
        res["find_lags"][f"top{top_n}"] = {"ms_per_1e5_pairs": ms, "pairs_per_s": n / (ms * 1e-3)}

    # the host path on one core, and a check that it agrees with the device on the same hits
    k = 200
    t0 = time.perf_counter()
    host = [host_locate_cc(m, x, int(onsets[h]), int(first[h])) for h in range(k)]
    dt = time.perf_counter() - t0
    dev_r = [m.locate_cc(x, int(onsets[h]), int(first[h])) for h in range(k)]
    res["host_numpy"] = {"us_per_hit": dt / k * 1e6, "hits_per_s": k / dt,
                         "agree": int(sum(np.allclose(p, q, rtol=0, atol=1e-12) for p, q in zip(host, dev_r)))}
    line = json.dumps(res)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
