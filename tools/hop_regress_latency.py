#!/usr/bin/env python3
"""Per-hop latency of the realtime chain with a window regressor, at the reference's realtime setup: 3 channels x 128
samples at 96 kHz (budget 1 333 us per hop), n_fft 2048.

    python tools/hop_regress_latency.py [--mode auto|graph|host|plain] [--model cnn|lcccnn] [--hops N]
                                        [--package-root DIR] [--out FILE]

The stream is the first case of the golden g25 (tests/golden/g25_hoplocate.npz), looped: every pass resets the
session and plays all its hops; the first pass is warm-up, then whole passes until 6 000 hops are timed.  Per
hop, the host clock runs around everything a caller needs for the hop's answer:

  graph   ``HopSession(regressor=...)``: one call, the model's position comes back with the onsets
  host    a regressor-less ``HopSession`` call, the grouping on the host, and on the hop that completes a window
          ``sess.audio(n)`` + ``model(x)``: the only form before the regressor moved into the hop's graph
  plain   a regressor-less ``HopSession`` call and nothing else: what a session without the feature costs (run it on
          this tree and, with --package-root, on an older checkout)

``auto`` takes ``graph`` when ``HopSession`` accepts ``regressor=`` and ``plain`` otherwise.  Models: ``cnn`` is the
``fit_cnn``-shaped default ``CNN(256, 2, 3)``, ``lcccnn`` the reference's train.py configuration (seven layers of five
maps, kernels 1 / 33 / 64 / 15 / 15 / 15 / 1, GroupNorm).  Reported per class of hop: p50 / p99 / count for hops that
evaluate a hit, hops that carry onsets, and hops without onsets.  One JSON line on stdout.
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
STAGE = dict(frame_length=256, pre_samples=32, max_distance=1000, min_channels=3)


class HostGrouping:
    """The stage's state machine on the host ("The window regressor in the hop")."""

    def __init__(self, B, C, frame_length, pre_samples, max_distance, min_channels):
        self.B, self.C, self.F, self.pre, self.D, self.minc = B, C, frame_length, pre_samples, max_distance, min_channels
        self.reset()

    def reset(self):
        self.cur, self.fifo, self.h = [], [], 0

    def _close(self):
        if len({c for _, c in self.cur}) >= self.minc:
            row = np.full(self.C, -1, np.int64)
            for s, c in self.cur:
                row[c] = s
            self.fifo.append((int(row[row >= 0].min()) - self.pre, row))
        self.cur = []

    def hop(self, channels, onsets):
        """-> the start of the window this hop completes, or None."""
        self.h += 1
        end = self.h * self.B
        for i in np.argsort(onsets, kind="stable"):
            s, c = int(onsets[i]), int(channels[i])
            if self.cur and s - self.cur[0][0] > self.D:
                self._close()
            self.cur.append((s, c))
        if self.cur and end > self.cur[0][0] + self.D:
            self._close()
        if self.fifo and end >= self.fifo[0][0] + self.F:
            return self.fifo.pop(0)[0]
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["auto", "graph", "host", "plain"], default="auto")
    ap.add_argument("--model", choices=["cnn", "lcccnn"], default="cnn")
    ap.add_argument("--hops", type=int, default=6000, help="hops timed after one warm-up pass over the stream")
    ap.add_argument("--package-root", default=str(REPO))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, args.package_root)
    import torch

    from onset_fingerprinting_amd import model, realtime

    g = np.load(REPO / "tests" / "golden" / "g25_hoplocate.npz", allow_pickle=False)
    case = json.loads(str(g["cases"]))[0]
    a = json.loads(str(g[f"{case}/args"]))
    audio, B = g[f"{case}/audio"], a["hop"]
    assert (audio.shape[1], B, a["sr"]) == (3, 128, 96000)
    det = {k: (tuple(v) if isinstance(v, list) else v) for k, v in a["detector"].items()}
    has = "regressor" in inspect.signature(realtime.HopSession.__init__).parameters
    mode = ("graph" if has else "plain") if args.mode == "auto" else args.mode
    if mode == "graph" and not has:
        raise SystemExit("this checkout's HopSession has no regressor=")
    torch.manual_seed(0)
    if args.model == "cnn":
        m = model.CNN(256, 2, 3).eval()
    else:
        m = model.LCCCNN(256, 2, 3, layer_sizes=[5] * 7, kernel_sizes=[1, 33, 64, 15, 15, 15, 1], dropout_rate=0.0,
                         batch_norm=True, group=False).eval()
    m = m.cuda()
    kw = dict(sr=96000, n_fft=2048, ring_seconds=1.0, **det)
    sess = realtime.HopSession(3, B, regressor=m, **STAGE, **kw) if mode == "graph" else realtime.HopSession(3, B, **kw)
    host = HostGrouping(B, 3, **STAGE)
    F, hops = STAGE["frame_length"], [np.ascontiguousarray(audio[h * B:(h + 1) * B]) for h in range(len(audio) // B)]
    times = {"evaluates_hit": [], "carries_onsets": [], "no_onsets": []}
    hits = 0
    for p in range(1 + -(-args.hops // len(hops))):
        sess.reset()
        host.reset()
        for hop in hops:
            t0 = time.perf_counter_ns()
            r = sess(hop)
            n = len(r["onsets"])
            if mode == "graph":
                hit = r["hit"] is not None
            elif mode == "host":
                start = host.hop(r["channels"], r["onsets"])
                hit = start is not None
                if hit:
                    # rows from the window's first to the newest (rows before sample 0 are the ring's zeros)
                    w = sess.audio(sess.current_index - start)[:F]
                    with torch.no_grad():
                        m(torch.from_numpy(np.ascontiguousarray(w.T[None])).cuda()).cpu()
            else:
                hit = False
            dt = (time.perf_counter_ns() - t0) * 1e-3
            if mode == "plain":  # classed by what the hop would do with the feature
                hit = host.hop(r["channels"], r["onsets"]) is not None
            if p == 0:
                continue
            times["evaluates_hit" if hit else "carries_onsets" if n else "no_onsets"].append(dt)
            hits += hit
    out = {"mode": mode, "model": args.model, "case": case, "device": torch.cuda.get_device_name(0),
           "package_root": "this tree" if Path(args.package_root).resolve() == REPO else "other checkout",
           "budget_us": BUDGET_US, "hops_timed": sum(len(v) for v in times.values()), "hits": hits,
           "classes": {k: {"p50_us": float(np.percentile(v, 50)), "p99_us": float(np.percentile(v, 99)),
                           "max_us": float(np.max(v)), "hops": len(v)} for k, v in times.items() if v}}
    line = json.dumps(out)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")
    sess.close()


if __name__ == "__main__":
    main()
