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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["auto", "graph", "host"], default="auto")
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
