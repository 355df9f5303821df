#!/usr/bin/env python3
"""Per-hop latency of the realtime chain with hit location, at the reference's realtime setup: 3 channels x 128
samples at 96 kHz (budget 1 333 us per hop), n_fft 2048, three drumhead sensors, the ring as rec_audio.

    python tools/hop_locate_latency.py [--mode auto|graph|host] [--planar] [--passes 4] [--package-root DIR]
                                       [--out FILE]

The stream is the first case of the golden g25 (tests/golden/g25_hoplocate.npz), looped: every pass resets the
session and plays all its hops; the first pass is warm-up.  Per hop, the host clock runs around everything a caller
needs for the hop's answer:

  graph   ``HopSession(locator=...)``: one call, the position comes back with the onsets
  host    a locator-less ``HopSession`` call, then ``Multilaterate3D.locate`` per onset (sorted by sample) with a ring
          over ``sess.audio`` until one returns a position: the only form before the locator moved into the hop's graph

``auto`` takes ``graph`` when ``HopSession`` accepts ``locator=`` and ``host`` otherwise, so the same tool measures an
older checkout (--package-root: the tree to import the package from).  Reported per class of hop: p50 / p99 / count
for hops without onsets, hops with onsets that complete no group, and hops that complete a group (a position is
returned).  One JSON line on stdout.

``--planar`` takes the 2-D ``Multilaterate`` on the same three sensors instead (no ring: that class has no
cross-correlation step); ``host`` is then ``Multilaterate.locate`` per onset.

``--paired`` takes the voting locator instead: ``MultilateratePaired`` on three drumhead sensors (scale 10, the default
grid), ``locate_cc`` with a window of 256 samples, groups of ``max_distance`` 1000 with all three channels.

  graph   ``HopSession(locator=MultilateratePaired(...))``: one call, the position comes back with the onsets
  host    a locator-less ``HopSession`` call, the grouping state machine on the host, and on the hop that completes a
          group's window ``sess.audio(n)`` and ``m.locate_cc`` on it
  plain   a locator-less ``HopSession`` call and nothing else (the form an older checkout can run: --package-root);
          the hops are classified by the same host state machine, outside the clock

The classes are then "no_onsets", "onsets_no_group" (carries onsets, evaluates nothing) and "completes_group" (evaluates
a hit).
"""
import argparse
import inspect
import json
import sys
import time
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parents[1]
BUDGET_US = 128 / 96000 * 1e6


class SessionRing:
    def __init__(self, sess):
        self.sess, self.counter = sess, sess.current_index

    def __getitem__(self, idx):
        return self.sess.audio(-idx.start)


class HostGroups:
    """detection.find_onset_groups made online, with the FIFO and the due rule of the hop's grouping stages
    ("The window regressor in the hop"): step(channels, onsets, end) -> None or the row that is due."""

    def __init__(self, C, F, pre, D, min_channels):
        self.C, self.F, self.pre, self.D, self.min_channels = C, F, pre, D, min_channels
        self.cur, self.fifo = [], []

    def _close(self):
        if len({c for _, c in self.cur}) >= self.min_channels:
            row = np.full(self.C, -1, np.int64)
            for s, c in self.cur:
                row[c] = s
            self.fifo.append((int(row[row >= 0].min()) - self.pre, row))
        self.cur = []

    def step(self, channels, onsets, end):
        for i in np.argsort(onsets, kind="stable"):
            s, c = int(onsets[i]), int(channels[i])
            if self.cur and s - self.cur[0][0] > self.D:
                self._close()
            self.cur.append((s, c))
        if self.cur and end > self.cur[0][0] + self.D:
            self._close()
        if self.fifo and end >= self.fifo[0][0] + self.F:
            return self.fifo.pop(0)
        return None


PAIRED = dict(tol=2, left=0, right=256, max_distance=1000, min_channels=3)


def paired_main(args, realtime, ml, torch, g, case, a, det):
    """--paired: the three forms' per-hop latency, one form per call."""
    audio, B = g[f"{case}/audio"], a["hop"]
    mode = "graph" if args.mode == "auto" else args.mode
    kw = dict(sr=96000, n_fft=2048, ring_seconds=1.0, **det)
    m = None
    if mode != "plain":
        m = ml.MultilateratePaired([s[:2] for s in a["layout"]["sensor_locations"]], scale=10, sr=96000)
    sess = realtime.HopSession(3, B, locator=m, **PAIRED, **kw) if mode == "graph" else realtime.HopSession(3, B, **kw)
    hops = [np.ascontiguousarray(audio[h * B:(h + 1) * B]) for h in range(len(audio) // B)]
    times = {"no_onsets": [], "onsets_no_group": [], "completes_group": []}
    p = PAIRED
    for k in range(args.passes):
        sess.reset()
        host = HostGroups(3, p["left"] + p["right"], p["left"], p["max_distance"], p["min_channels"])
        for h, hop in enumerate(hops):
            end = (h + 1) * B
            t0 = time.perf_counter_ns()
            r = sess(hop)
            n = len(r["onsets"])
            if mode == "graph":
                hit = r["cc_hit"] is not None
            elif mode == "host":
                due = host.step(r["channels"], r["onsets"], end)
                hit = due is not None
                if hit and due[0] >= 0:
                    start, row = due
                    onset, first = min((int(v), c) for c, v in enumerate(row) if v >= 0)
                    x = sess.audio(end - start)
                    m.locate_cc(x, p["left"], first, tol=p["tol"], left=p["left"], right=p["right"])
            dt = (time.perf_counter_ns() - t0) * 1e-3
            if mode == "plain":
                hit = host.step(r["channels"], r["onsets"], end) is not None
            if k:
                times["completes_group" if hit else "onsets_no_group" if n else "no_onsets"].append(dt)
    out = {"mode": mode, "locator": "MultilateratePaired", "case": case, "device": torch.cuda.get_device_name(0),
           "package_root": "parent" if args.package_root != str(REPO) else "this", "budget_us": BUDGET_US,
           "hops_timed": sum(len(v) for v in times.values()),
           "classes": {k: {"p50_us": float(np.percentile(v, 50)), "p99_us": float(np.percentile(v, 99)),
                           "max_us": float(np.max(v)), "hops": len(v)} for k, v in times.items() if v}}
    line = json.dumps(out)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        with open(args.out, "a") as f:  # (rounds of the three forms alternate: one line per call)
            f.write(line + "\n")
    sess.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["auto", "graph", "host", "plain"], default="auto")
    ap.add_argument("--paired", action="store_true", help="the voting MultilateratePaired (locate_cc) instead")
    ap.add_argument("--planar", action="store_true", help="the 2-D Multilaterate instead of Multilaterate3D")
    ap.add_argument("--passes", type=int, default=4, help="passes over the stream, the first is warm-up")
    ap.add_argument("--package-root", default=str(REPO))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, args.package_root)
    import torch

    from onset_fingerprinting_amd import multilateration as ml
    from onset_fingerprinting_amd import realtime

    g = np.load(REPO / "tests" / "golden" / "g25_hoplocate.npz", allow_pickle=False)
    case = json.loads(str(g["cases"]))[0]
    a = json.loads(str(g[f"{case}/args"]))
    audio, B = g[f"{case}/audio"], a["hop"]
    assert (audio.shape[1], B, a["sr"]) == (3, 128, 96000)
    det = {k: (tuple(v) if isinstance(v, list) else v) for k, v in a["detector"].items()}
    if args.paired:
        return paired_main(args, realtime, ml, torch, g, case, a, det)
    if args.mode == "plain":
        raise SystemExit("--mode plain goes with --paired")
    has_locator = "locator" in inspect.signature(realtime.HopSession.__init__).parameters
    mode = ("graph" if has_locator else "host") if args.mode == "auto" else args.mode
    if mode == "graph" and not has_locator:
        raise SystemExit("this checkout's HopSession has no locator=")
    if args.planar:
        m = ml.Multilaterate(**dict(a["layout"], sensor_locations=[s[:2] for s in a["layout"]["sensor_locations"]]))
    else:
        m = ml.Multilaterate3D(**a["layout"])
    kw = dict(sr=96000, n_fft=2048, ring_seconds=1.0, **det)
    sess = realtime.HopSession(3, B, locator=m, **kw) if mode == "graph" else realtime.HopSession(3, B, **kw)
    hops = [np.ascontiguousarray(audio[h * B:(h + 1) * B]) for h in range(len(audio) // B)]
    times = {"no_onsets": [], "onsets_no_group": [], "completes_group": []}
    located = 0
    for p in range(args.passes):
        sess.reset()
        m.ongoing = []
        for hop in hops:
            t0 = time.perf_counter_ns()
            r = sess(hop)
            n = len(r["onsets"])
            if mode == "graph":
                res = r["location"]
            else:
                res = None
                if n:
                    for i in np.argsort(r["onsets"], kind="stable"):
                        if args.planar:
                            res = m.locate(int(r["channels"][i]), int(r["onsets"][i]))
                        else:
                            res = m.locate(int(r["channels"][i]), int(r["onsets"][i]), SessionRing(sess))
                        if res is not None:
                            break
            dt = (time.perf_counter_ns() - t0) * 1e-3
            if p == 0:
                continue
            times["no_onsets" if n == 0 else "completes_group" if res is not None else "onsets_no_group"].append(dt)
            located += res is not None
    # (the golden holds the 3-D locator's positions only)
    want = None if args.planar else int(g[f"{case}/audio/res"][:, 0].sum()) * (args.passes - 1)
    out = {"mode": mode, "locator": "Multilaterate" if args.planar else "Multilaterate3D", "case": case, "device": torch.cuda.get_device_name(0), "budget_us": BUDGET_US,
           "hops_timed": sum(len(v) for v in times.values()), "located": located, "located_expected": want,
           "classes": {k: {"p50_us": float(np.percentile(v, 50)), "p99_us": float(np.percentile(v, 99)),
                           "max_us": float(np.max(v)), "hops": len(v)} for k, v in times.items() if v}}
    line = json.dumps(out)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")
    sess.close()


if __name__ == "__main__":
    main()
