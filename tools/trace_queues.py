"""Which hardware queues the in-flight window of a rocprofv3 kernel trace of bench.py used (the window of
tools/trace_regime.py), how many launches and streams each carried, how busy each was, and the share of the window
spent with n kernels running.

    python tools/trace_queues.py <rocprof output dir>  > queues.json
"""
import csv, glob, json, sys
from collections import defaultdict

f = sorted(glob.glob(sys.argv[1] + "/*/*kernel_trace.csv"))[-1]
rows = list(csv.DictReader(open(f)))
anchor = sorted(int(r["Start_Timestamp"]) for r in rows if "k_transpose_in" in r["Kernel_Name"])
cut = max(1, int(0.15 * len(anchor)))
t_lo, t_hi = anchor[cut], anchor[-cut]
T = t_hi - t_lo
qbusy = defaultdict(int)
qn = defaultdict(int)
streams = defaultdict(set)
ev = []
for r in rows:
    s, e = int(r["Start_Timestamp"]), int(r["End_Timestamp"])
    if s < t_lo or s >= t_hi:
        continue
    q = r.get("Queue_Id", "?")
    qbusy[q] += min(e, t_hi) - s
    qn[q] += 1
    if "Stream_Id" in r:
        streams[q].add(r["Stream_Id"])
    ev.append((s, 1))
    ev.append((min(e, t_hi), -1))
ev.sort()
hist = defaultdict(int)
n, last = 0, t_lo
for t, d in ev:
    hist[n] += t - last
    n += d
    last = t
print(json.dumps({"queues_used": len(qbusy),
                  "per_queue": {q: {"launches": qn[q], "kernel_time_over_window": round(qbusy[q] / T, 3),
                                    "streams": len(streams[q])} for q in sorted(qbusy)},
                  "share_of_window_with_n_kernels_running": {str(k): round(v / T, 4) for k, v in sorted(hist.items())}}, indent=1))
