#!/usr/bin/env python3
"""Latency and throughput of the hit locator (onset_fingerprinting_amd.multilateration), the realtime layout:
three drumhead sensors at 96 kHz.

    python tools/locate_latency.py [--planar] [--out results/locate_latency.json]

  locate      one Multilaterate3D.locate call that completes a group (the realtime case; budget 1 333 us per
              128-sample hop at 96 kHz), without and with the ring's cross-correlation step: host clock around
              the call, which ends in device synchronisations of its own
  batched     locate_groups_device over G = 1, 10^3, 10^5 groups: HIP events around `iters` calls after warm-up,
              lag maps and sensors resident on the GPU
  host scipy  the reference's per-group path on one CPU core: numpy legality search + scipy.optimize.fsolve with the
              same equations, Jacobian and arguments (xtol 0.01, maxfev 20)

--planar measures the 2-D Multilaterate on the same three sensors instead: its locate (no ring: the class has no
cross-correlation step), locate_groups_device with it, and the reference's 2-D steps on the host (no reordering, deltas
lag * c / sr).
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

LAYOUT = dict(sensor_locations=[(0.9, 30, 0), (0.9, 150, 0), (0.9, 270, 0)], medium="drumhead", sr=96000)
LAYOUT_2D = dict(LAYOUT, sensor_locations=[s[:2] for s in LAYOUT["sensor_locations"]])


def strike_rows(m, G, seed=0):
    """Onset rows [G, 3] of strikes at random points: per-sensor delay distance / c * sr."""
    rng = np.random.default_rng(seed)
    ang, rad = rng.uniform(0, 2 * np.pi, G), m.radius * 0.8 * np.sqrt(rng.uniform(0, 1, G))
    p = np.stack([rad * np.cos(ang), rad * np.sin(ang)], 1)
    s = np.array([list(v) + [0.0] * (3 - len(v)) for v in m.sensor_locs])
    d = np.sqrt(((p[:, None, :] - s[None, :, :2]) ** 2).sum(-1) + s[None, :, 2] ** 2)
    return 100000 + np.round(d / speed(m) * m.sr).astype(np.int64)


def speed(m):
    """cm/s: Multilaterate3D keeps it, the 2-D class computes it where it is used."""
    from onset_fingerprinting_amd import multilateration as ml
    return m.c if hasattr(m, "c") else ml.speed_of_sound(100, medium=m.medium)


def host_scipy(m, rows, planar=False):
    """The reference's per-group steps on the host (multilateration.py:413-426, 536-565, 230-316; planar: :662-675,
    :714-733, :170-227 -- sensors with z = 0, no reordering, deltas lag * c / sr)."""
    from scipy.optimize import fsolve
    loc = [np.array(list(v) + [0.0] * (3 - len(v)), np.float64) for v in m.sensor_locs]
    c = speed(m)
    tol = m.samples_per_cm
    maps = {(i, j): m.lag_maps[i][j] for i in range(3) for j in range(3) if i != j}
    out = []
    for row in rows:
        s = [int(v) for v in np.argsort(row, kind="stable")]
        o = [int(row[v]) for v in s]
        l1, l2 = o[1] - o[0], o[2] - o[0]
        if not (m.is_legal(s[0], s[1], l1) and m.is_legal(s[0], s[2], l2)):
            out.append(None)
            continue
        lm1, lm2 = maps[(s[0], s[1])], maps[(s[0], s[2])]
        legal = (lm1 < l1 + tol) & (lm1 > l1 - tol) & (lm2 < l2 + tol) & (lm2 > l2 - tol)
        res = np.unravel_index(np.argmax(legal > 0), legal.shape, "F")
        if res == (0, 0):
            out.append(None)
            continue
        if s[1] == 1 and not planar:
            s[1:], o[1:] = [0, 1], o[2:0:-1]
        a, b, c0 = loc[s[1]], loc[s[2]], loc[s[0]]
        if planar:
            dda, ddb = (o[1] - o[0]) * c / m.sr, (o[2] - o[0]) * c / m.sr
        else:
            dda, ddb = (o[1] - o[0]) / m.sr * c, (o[2] - o[0]) / m.sr * c

        def f(p):
            da, db, d0 = (np.sqrt((p[0] - q[0]) ** 2 + (p[1] - q[1]) ** 2 + q[2] ** 2) for q in (a, b, c0))
            return np.array([da - d0 - dda, db - d0 - ddb])

        def jac(p):
            da, db, d0 = (np.sqrt((p[0] - q[0]) ** 2 + (p[1] - q[1]) ** 2 + q[2] ** 2) for q in (a, b, c0))
            return np.array([[(p[0] - a[0]) / da - (p[0] - c0[0]) / d0, (p[1] - a[1]) / da - (p[1] - c0[1]) / d0],
                             [(p[0] - b[0]) / db - (p[0] - c0[0]) / d0, (p[1] - b[1]) / db - (p[1] - c0[1]) / d0]])

        root, info, ier, _ = fsolve(f, np.array(res) - m.radius, full_output=True, xtol=0.01, maxfev=20, fprime=jac)
        out.append(tuple(root) if ier == 1 else None)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--planar", action="store_true", help="the 2-D Multilaterate instead of Multilaterate3D")
    args = ap.parse_args()
    import torch

    from onset_fingerprinting_amd import multilateration as ml
    torch.set_num_threads(1)
    m = ml.Multilaterate(**LAYOUT_2D) if args.planar else ml.Multilaterate3D(**LAYOUT)
    res = {"locator": type(m).__name__, "layout": LAYOUT_2D if args.planar else LAYOUT,
           "device": torch.cuda.get_device_name(0)}

    # realtime: the third onset of a strike completes the group
    row = strike_rows(m, 1, seed=4)[0]  # a strike the reference locates
    order = np.argsort(row, kind="stable")
    audio = np.zeros((row.max() + 4096, 3), np.float32)
    rng = np.random.default_rng(1)
    for ch in range(3):
        t = np.arange(600)
        audio[row[ch]:row[ch] + 600, ch] = 0.8 * np.exp(-t / 120.0) * np.sin(2 * np.pi * (3000 + 700 * ch) / 96000 * t)
    audio += 1e-3 * rng.standard_normal(audio.shape).astype(np.float32)

    class Ring:
        def __init__(self, counter):
            self.counter = counter

        def __getitem__(self, idx):
            return audio[: self.counter][idx]

    def feed(k, ring):
        if args.planar:
            return m.locate(int(k), int(row[k]))
        return m.locate(int(k), int(row[k]), Ring(int(row[k]) + 256) if ring else None)

    for name, ring in (("locate_us", None),) + (() if args.planar else (("locate_with_ring_us", True),)):
        times, located = [], 0
        for it in range(args.iters + 10):
            m.ongoing = []
            for k in order[:2]:
                feed(k, ring)
            k = order[2]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = feed(k, ring)
            torch.cuda.synchronize()
            if it >= 10:
                times.append((time.perf_counter() - t0) * 1e6)
                located += r is not None
        res[name] = {"p50": float(np.median(times)), "p90": float(np.percentile(times, 90)), "located": located,
                     "calls": len(times)}

    # batched
    res["batched"] = {}
    for G in (1, 1000, 100000):
        g = torch.from_numpy(strike_rows(m, G, seed=G)[None].copy()).cuda()
        for _ in range(3):
            xy, st = ml.locate_groups_device(g, None, m)
        torch.cuda.synchronize()
        iters = max(5, min(args.iters, 2000000 // max(G, 1)))
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            xy, st = ml.locate_groups_device(g, None, m)
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / iters
        res["batched"][str(G)] = {"ms_per_call": ms, "groups_per_s": G / (ms * 1e-3),
                                  "located": int((st == 1).sum().item())}

    # the host path on one core
    rows = strike_rows(m, 300, seed=11)
    t0 = time.perf_counter()
    host = host_scipy(m, rows, args.planar)
    dt = time.perf_counter() - t0
    res["host_scipy"] = {"us_per_group": dt / len(rows) * 1e6, "groups_per_s": len(rows) / dt,
                         "located": sum(r is not None for r in host)}
    line = json.dumps(res)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
