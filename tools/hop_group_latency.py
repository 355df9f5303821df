#!/usr/bin/env python3
"""Per-hop latency of S realtime streams served together, at the reference's realtime setup: 3 channels x 128 samples
at 96 kHz (budget 1 333 us per hop period), n_fft 2048, a seeded FCNN on the mel bands, three drumhead sensors with the
locator in the hop's graph.

    python tools/hop_group_latency.py [--sizes 1,2,4,...] [--hops 5000] [--rounds 3] [--out FILE]

The stream is the first case of the golden g25 (tests/golden/g25_hoplocate.npz), looped; member i starts 7 i hops into
it, so the members' onsets fall into different hops.  For every S, in one process and alternating, `--rounds` rounds of

  group        ``HopSessionGroup.push_raw``: one graph launch and one wait for the S hops
  sequential   S stand-alone ``HopSession.push_raw`` calls one after the other: S launches and S waits, the only way to
               serve S streams without the group

with the host clock around everything a caller needs to have all S answers (the hops are laid out before the clock
starts).  p50 / p99 per round; `largest_S_within_budget` is the largest S whose group p99 stays below the hop period in
every round.  One JSON document on stdout and in --out.
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))
BUDGET_US = 128 / 96000 * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1,2,4,8,16,32,64,128")
    ap.add_argument("--hops", type=int, default=5000, help="timed hops per round and form")
    ap.add_argument("--warmup", type=int, default=300, help="untimed hops per form before the first round")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=str(REPO / "profiles" / "hop_group_latency.json"))
    args = ap.parse_args()
    import torch

    from onset_fingerprinting_amd import multilateration as ml
    from onset_fingerprinting_amd import realtime
    from onset_fingerprinting_amd.pipeline import seeded_fcnn

    g = np.load(REPO / "tests" / "golden" / "g25_hoplocate.npz", allow_pickle=False)
    case = json.loads(str(g["cases"]))[0]
    a = json.loads(str(g[f"{case}/args"]))
    audio, B = g[f"{case}/audio"], a["hop"]
    assert (audio.shape[1], B, a["sr"]) == (3, 128, 96000)
    det = {k: (tuple(v) if isinstance(v, list) else v) for k, v in a["detector"].items()}
    nh = len(audio) // B
    stream = np.ascontiguousarray(audio[: nh * B].reshape(nh, B, 3))
    locator = ml.Multilaterate3D(**a["layout"])
    clf = seeded_fcnn(40, 8)

    def make():
        return realtime.HopSession(3, B, sr=96000, n_fft=2048, ring_seconds=1.0, classifier=clf, locator=locator, **det)

    def pcts(v):
        return {"p50_us": float(np.percentile(v, 50)), "p99_us": float(np.percentile(v, 99)), "max_us": float(np.max(v))}

    results = []
    for S in [int(v) for v in args.sizes.split(",")]:
        members, alone = [make() for _ in range(S)], [make() for _ in range(S)]
        group = realtime.HopSessionGroup(members)
        offs = 7 * np.arange(S)
        clock = time.perf_counter_ns

        def run_group(n, h0):
            t = np.empty(n)
            onsets = 0
            for k in range(n):
                hops = stream[(h0 + k + offs) % nh]  # [S, B, 3]
                t0 = clock()
                counts = group.push_raw(hops)
                t[k] = (clock() - t0) * 1e-3
                onsets += sum(counts)
            return t, onsets

        def run_alone(n, h0):
            t = np.empty(n)
            onsets = 0
            for k in range(n):
                hops = stream[(h0 + k + offs) % nh]
                t0 = clock()
                counts = [s.push_raw(hop) for s, hop in zip(alone, hops)]
                t[k] = (clock() - t0) * 1e-3
                onsets += sum(counts)
            return t, onsets

        run_group(args.warmup, 0)
        run_alone(args.warmup, 0)
        row = {"S": S, "workgroups": 4 * S, "group": [], "sequential": []}
        h0 = args.warmup
        for _ in range(args.rounds):
            tg, og = run_group(args.hops, h0)
            ta, oa = run_alone(args.hops, h0)
            assert og == oa, (S, og, oa)  # the two forms saw the same streams and found the same onsets
            row["group"].append(pcts(tg))
            row["sequential"].append(pcts(ta))
            row["onsets_per_round"] = og
            h0 += args.hops
        results.append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
        group.close()
        for s in members + alone:
            s.close()
    within = [r["S"] for r in results if all(q["p99_us"] < BUDGET_US for q in r["group"])]
    out = {"tool": "hop_group_latency", "device": torch.cuda.get_device_name(0), "budget_us": BUDGET_US, "case": case,
           "hops_per_round": args.hops, "rounds": args.rounds, "warmup_hops": args.warmup,
           "largest_S_within_budget": max(within) if within else None, "results": results}
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
