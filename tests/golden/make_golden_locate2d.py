#!/usr/bin/env python3
"""Golden vectors g23_locate2d: the reference's find_lag / find_lag_multi, MultilateratePaired, the 2-D
Multilaterate and lag_intensity_map (multilateration.py), run with scipy on the host.

Run in the build container only:   python tests/golden/make_golden_locate2d.py
find_lag and scipy.optimize.fsolve are wrapped in the reference module's namespace while this runs, so that every
locate_cc call also records its lags and every solve its ier and info["nfev"].  A second run writes the same bytes.

Contents (every key is prefixed by its section):
  fl/{data, off, len_a, len_b, top_n, lag, peaks, vals, n_found, near_tie}
        find_lag / find_lag_multi on row pairs; a row is data[off : off + len] / 256 (int16 samples, exact in fp32).
        peaks / vals [n][8] (padded with 0 / NaN), n_found = number of returned peaks; near_tie: the fp64 correlation
        has a tie within 1e-6 * max|cc| at a decision (argmax, peak existence or peak order) that fp32 rounding can
        flip
  pair/<layout>/{args, sensor_locs, radius, side, keys, map_sha, map0, map0_nan}
        MultilateratePaired(**args): keys [K][2] = (i, j) of lag_maps[i][j] in dict order, map_sha [K] the sha256 of
        each map's bytes, map0 / map0_nan lag_maps[0][1] as int16 plus NaN mask
  pair/<layout>/loc/{lags, first, rphi, raised, ier, nfev}    locate(lags, i); raised: TypeError (failed solve)
  pair/<layout>/cc/{x, onset, first, left, right, lags, rphi, cell, res_idx, res}
        locate_cc over a synthetic recording x [N, C] (int16, / 4096); lags [B][2] from find_lag (the second repeats the
        first when S == 2), cell = np.argmax(res); res [R][side][side] uint8 for the hits res_idx [R]
  m2d/<layout>/{args, sensor_locs, min, max, max_max, maps}   Multilaterate: min / max [S][S] (NaN diagonal)
  m2d/<layout>/legal/{sensors, onsets, idx}                     is_legal_3d queries
  m2d/<layout>/trace/{sensor, onset, res, ier, nfev}          locate over an onset stream; res [calls][3] =
        (returned?, r, phi); ier / nfev per solve, in call order
  lim/<case>/{args, lag_sha, lag, a, b}                          lag_intensity_map (lag [side][side] float32 stored
        only for small grids)
"""
import hashlib
import json
import sys
import warnings
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
REPO = HERE.parents[1]
sys.path.insert(0, str(HERE))
sys.path.insert(0, str(REPO))

from _refload import load_reference  # noqa: E402
from make_golden_locate import _FsolveLog, write_npz  # noqa: E402

warnings.filterwarnings("ignore")

TOP = 8
PAIRED = {
    "p4mm": dict(sensor_locations=[(0.9, 0), (0.9, 90), (0.9, 180), (0.9, 270)], scale=10, medium="drumhead",
                 sr=96000),
    "p3air": dict(sensor_locations=[(0.95, 20), (0.9, 140), (1.0, 260)], scale=1, medium="air", sr=48000),
    "p2": dict(sensor_locations=[(0.8, 45), (0.85, 225)], scale=1, medium="drumhead", sr=96000),
}
M2D = {
    "m3": dict(sensor_locations=[(0.9, 30), (0.9, 150), (0.9, 270)], medium="drumhead", sr=96000),
    "m4air": dict(sensor_locations=[(1.05, 0), (1.05, 90), (1.1, 180), (1.05, 270)], medium="air", sr=48000),
}
LIM = {
    "s1_a": dict(mic_a=(12.0, -3.0, 6.0), mic_b=(-9.5, 8.0, 10.0), reflectivity=0.5, sr=96000, scale=1, medium="air"),
    "s1_b": dict(mic_a=(0.0, 17.0, 3.0), mic_b=(15.0, 0.0, 20.0), reflectivity=0.9, sr=48000, scale=1,
                 medium="drumhead"),
    "s10_a": dict(mic_a=(30.0, -12.5, 40.0), mic_b=(-25.0, 20.0, 55.0), reflectivity=0.3, d=8.0, sr=96000, scale=10,
                  medium="air"),
    "s10_b": dict(mic_a=(-5.0, 35.0, 20.0), mic_b=(40.0, -40.0, 80.0), reflectivity=0.0, d=7.5, sr=44100, scale=10,
                  medium="air"),
}


class _LagLog:
    def __init__(self, fn):
        self.fn, self.calls = fn, []

    def __call__(self, a, b):
        lag = self.fn(a, b)
        self.calls.append(int(lag))
        return lag


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def near_tie(cc32, a, b, top_n):
    """Does the fp64 correlation hold a near-tie at one of the decisions find_lag / find_lag_multi take?"""
    cc = np.correlate(a.astype(np.float64), b.astype(np.float64), "full")
    eps = 1e-6 * max(np.max(np.abs(cc)), 1e-300)
    close = lambda u, v: abs(u - v) <= eps
    o = np.sort(cc)[::-1]
    if len(o) > 1 and close(o[0], o[1]):
        return True
    d = np.abs(np.diff(cc))
    if np.any((d <= eps) & (d > 0)) or np.any((np.diff(cc32) == 0) != (np.diff(cc) == 0)):
        return True  # a step that rounding can turn into a plateau, or the reverse
    import scipy.signal
    p, _ = scipy.signal.find_peaks(cc)
    v = np.sort(cc[p])[::-1][:top_n + 1]
    return bool(np.any(np.diff(v) >= -eps))  # peak order (exact ties included: argsort's order is undefined)


def find_lag_cases(ml, rng):
    pairs = []

    def q(x):
        return np.clip(np.round(np.asarray(x) * 256), -32768, 32767).astype(np.int16)

    def onset(n, at, decay, amp=1.0):
        t = np.arange(n) - at
        env = np.where(t >= 0, np.exp(-np.maximum(t, 0) / decay), 0.0)
        return amp * env * np.abs(rng.normal(0, 1, n))

    for k in range(540):
        kind = k % 3
        if k < 12:
            la = lb = int(rng.integers(1, 4))
        elif k % 40 == 7:
            la, lb = int(rng.integers(1000, 4097)), int(rng.integers(1000, 4097))
        elif k % 5 == 0:
            la, lb = int(rng.integers(1, 300)), int(rng.integers(1, 300))
        else:
            la = lb = int(rng.integers(16, 300))
        if kind == 0:
            a, b = rng.normal(0, 4, la), rng.normal(0, 4, lb)
        elif kind == 1:
            d = int(rng.integers(-20, 21))
            a = onset(la, la // 4, 10 + 30 * rng.random(), 20)
            b = onset(lb, max(lb // 4 + d, 0), 10 + 30 * rng.random(), 20)
        else:
            per = 4 + 20 * rng.random()
            a = 10 * np.sin(2 * np.pi * np.arange(la) / per) + rng.normal(0, 0.5, la)
            b = 10 * np.sin(2 * np.pi * (np.arange(lb) + rng.integers(0, 10)) / per)
        pairs.append((q(a), q(b), 1 + k % TOP))
    # plateaus, fewer peaks than top_n, end points
    hand = [([0, 0, 1, 1, 1, 0, 0], [1], 3), ([0, 2, 2, 0, 2, 2, 0], [1], 4), ([1, 2, 3, 4, 5], [1], 2),
            ([5, 4, 3, 2, 1], [1], 2), ([0, 1, 1, 0], [1, 1], 8), ([0, 0, 0, 0], [0, 0], 3),
            ([3, 0, 3, 0, 3], [1, 1], 5),
            ([1, 1, 2, 2, 1, 1], [1, 0, 1], 6)]
    for a, b, t in hand:
        pairs.append((np.array(a, np.int16) * 256, np.array(b, np.int16) * 256, t))
    data, off, la, lb, tn, lag, peaks, vals, nf, tie = [], [], [], [], [], [], [], [], [], []
    pos = 0
    for a_i, b_i, t in pairs:
        a, b = a_i.astype(np.float32) / 256, b_i.astype(np.float32) / 256
        data += [a_i, b_i]
        off.append([pos, pos + len(a_i)])
        pos += len(a_i) + len(b_i)
        la.append(len(a))
        lb.append(len(b))
        tn.append(t)
        lag.append(int(ml.find_lag(a, b)))
        p, v = ml.find_lag_multi(a, b, top_n=t)
        pp = np.zeros(TOP, np.int64)
        vv = np.full(TOP, np.nan, np.float32)
        pp[:len(p)], vv[:len(v)] = p, v
        peaks.append(pp)
        vals.append(vv)
        nf.append(len(p))
        tie.append(near_tie(np.correlate(a, b, "full"), a, b, t))
    return {"fl/data": np.concatenate(data), "fl/off": np.array(off, np.int64), "fl/len_a": np.array(la, np.int32),
            "fl/len_b": np.array(lb, np.int32), "fl/top_n": np.array(tn, np.int32), "fl/lag": np.array(lag, np.int64),
            "fl/peaks": np.array(peaks), "fl/vals": np.array(vals), "fl/n_found": np.array(nf, np.int32),
            "fl/near_tie": np.array(tie)}


def recording(rng, locs, c, sr, n_hits, radius, N_per=500, extra_end=True, glitch_every=0):
    """Synthetic recording [N, C] on a silent background: decaying bursts that reach sensor k after
    |p - s_k| / c * sr samples (plus 300 on every glitch_every-th hit: no cell matches), quantised to multiples of
    1 / 4096 (stored as int16, exact in fp32)."""
    S = len(locs)
    N = N_per * n_hits + 400
    x = np.zeros((N, S), np.float64)
    onsets, firsts = [], []
    for h in range(n_hits):
        while True:
            p = rng.uniform(-radius, radius, 2)
            if np.hypot(*p) < 0.9 * radius:
                break
        t0 = 200 + h * N_per
        if extra_end and h == n_hits - 1:
            t0 = N - 120  # the window is clipped at the clip's end
        d = [np.hypot(p[0] - s[0], p[1] - s[1]) / c * sr for s in locs]
        first = int(np.argmin(d))
        for k in range(S):
            glitch = glitch_every and h % glitch_every == 2 and k != first
            t = t0 + int(round(d[k] - d[first])) + (300 if glitch else 0)
            n = min(160, N - t)
            if n <= 0:
                continue
            env = np.exp(-np.arange(n) / (8 + 3 * k)) * (1 + 0.5 * rng.random())
            x[t:t + n, k] += env * rng.normal(0, 1, n)
        onsets.append(t0)
        firsts.append(first)
    xq = np.clip(np.round(x * 4096), -32768, 32767).astype(np.int16)
    return xq.astype(np.float32) / 4096, xq, onsets, firsts


def paired(ml, rng, name, kw, log, laglog):
    out = {}
    m = ml.MultilateratePaired(**kw)
    S = len(m.sensor_locs)
    pre = f"pair/{name}"
    out[f"{pre}/args"] = np.array(json.dumps(kw))
    out[f"{pre}/sensor_locs"] = np.array(m.sensor_locs, np.float64)
    out[f"{pre}/radius"] = np.array(m.radius, np.int64)
    side = m.lag_maps[0][1].shape[0]
    out[f"{pre}/side"] = np.array(side, np.int64)
    keys = [(i, j) for i in range(S) for j in m.lag_maps[i]]
    out[f"{pre}/keys"] = np.array(keys, np.int64)
    out[f"{pre}/map_sha"] = np.array([sha(m.lag_maps[i][j]) for i, j in keys])
    mp = m.lag_maps[0][1]
    out[f"{pre}/map0"] = np.nan_to_num(mp, nan=0).astype(np.int16)
    out[f"{pre}/map0_nan"] = np.isnan(mp)
    # locate on lag pairs: plausible ones, and large ones whose solve fails
    c = ml.speed_of_sound(100 * m.scale, medium=m.medium)
    span = max(int(np.nanmax(np.abs(mp))), 2)
    n_loc = 240 if name == "p4mm" else 60
    lags, first, rphi, raised, ier, nfev = [], [], [], [], [], []
    for k in range(n_loc):
        lim = span if k % 6 else 4 * span
        lg = [int(rng.integers(-lim, lim + 1)), int(rng.integers(-lim, lim + 1))]
        i = int(rng.integers(0, S))
        n0 = len(log.calls)
        try:
            rphi.append(np.array(m.locate(lg, i), np.float64))
            raised.append(False)
        except TypeError:
            rphi.append(np.full(2, np.nan))
            raised.append(True)
        assert len(log.calls) == n0 + 1
        ier.append(log.calls[-1][1])
        nfev.append(log.calls[-1][2])
        lags.append(lg)
        first.append(i)
    out.update({f"{pre}/loc/lags": np.array(lags, np.int64), f"{pre}/loc/first": np.array(first, np.int64),
                f"{pre}/loc/rphi": np.array(rphi), f"{pre}/loc/raised": np.array(raised),
                f"{pre}/loc/ier": np.array(ier, np.int32), f"{pre}/loc/nfev": np.array(nfev, np.int32)})
    # locate_cc over a synthetic recording
    n_hits = {"p4mm": 320, "p3air": 60, "p2": 24}[name]
    x, xq, onsets, firsts = recording(rng, m.sensor_locs, c, m.sr, n_hits, m.radius,
                                      glitch_every=5 if name == "p3air" else 0)
    on_l, fi_l, le_l, ri_l, lg_l, rp_l, cell_l, res_idx, res_l = [], [], [], [], [], [], [], [], []
    for h in range(n_hits):
        left = 0 if h % 7 else int(rng.integers(1, 64))
        right = 256 if h % 11 else int(rng.integers(32, 512))
        onset = onsets[h] if h % 13 else onsets[h] + int(rng.integers(-30, 30))
        i = firsts[h] if h % 9 else int(rng.integers(0, S))
        n0 = len(laglog.calls)
        rp = m.locate_cc(x, onset, i, left=left, right=right)
        lg = laglog.calls[n0:]
        assert len(lg) == len(m.lag_maps[i])
        if len(lg) == 1:
            lg = lg * 2
        on_l.append(onset)
        fi_l.append(i)
        le_l.append(left)
        ri_l.append(right)
        lg_l.append(lg)
        rp_l.append(np.array(rp, np.float64))
        cell_l.append(int(np.argmax(m.res)))
        if h < 3 or h == n_hits - 1:
            res_idx.append(h)
            res_l.append(m.res.astype(np.uint8))
    out.update({f"{pre}/cc/x": xq, f"{pre}/cc/onset": np.array(on_l, np.int64),
                f"{pre}/cc/first": np.array(fi_l, np.int64),
                f"{pre}/cc/left": np.array(le_l, np.int64), f"{pre}/cc/right": np.array(ri_l, np.int64),
                f"{pre}/cc/lags": np.array(lg_l, np.int64), f"{pre}/cc/rphi": np.array(rp_l),
                f"{pre}/cc/cell": np.array(cell_l, np.int64), f"{pre}/cc/res_idx": np.array(res_idx, np.int64),
                f"{pre}/cc/res": np.array(res_l)})
    return out


def multilaterate2d(ml, rng, name, kw, log):
    out = {}
    m = ml.Multilaterate(**kw)
    S = len(m.sensor_locs)
    pre = f"m2d/{name}"
    n = m.lag_maps[0][1].shape[0]
    mn = np.full((S, S), np.nan, np.float32)
    mx = np.full((S, S), np.nan, np.float32)
    maps = np.full((S, S, n, n), np.nan, np.float32)
    for i in range(S):
        for j in m.lag_maps[i]:
            mn[i, j], mx[i, j], maps[i, j] = m.min_lags[i][j], m.max_lags[i][j], m.lag_maps[i][j]
    out.update({f"{pre}/args": np.array(json.dumps(kw)), f"{pre}/sensor_locs": np.array(m.sensor_locs, np.float64),
                f"{pre}/min": mn, f"{pre}/max": mx, f"{pre}/maps": maps,
                f"{pre}/max_max": np.array(m.max_max_lags, np.float32)})
    c = ml.speed_of_sound(100, medium=m.medium)
    sens, ons, idx = [], [], []
    for qn in range(1100):
        s = [int(v) for v in rng.permutation(S)[:3]]
        while True:
            p = rng.uniform(-m.radius, m.radius, 2)
            if np.hypot(*p) < 0.9 * m.radius:
                break
        t = [int(round(np.hypot(p[0] - m.sensor_locs[k][0], p[1] - m.sensor_locs[k][1]) / c * m.sr)) for k in s]
        if qn % 4 == 0:
            t = [t[0], t[0] + int(rng.integers(-300, 300)), t[0] + int(rng.integers(-300, 300))]
        base = 5000 + int(rng.integers(0, 3000))
        o = [base + v - t[0] for v in t]
        sens.append(s)
        ons.append(o)
        idx.append([int(v) for v in m.is_legal_3d((s, o))])
    out.update({f"{pre}/legal/sensors": np.array(sens, np.int32), f"{pre}/legal/onsets": np.array(ons, np.int64),
                f"{pre}/legal/idx": np.array(idx, np.int32)})
    # an onset stream: every hit reaches all sensors, in arrival order, with some jitter and stray onsets
    stream = []
    t0 = 1000
    for h in range(80):
        while True:
            p = rng.uniform(-m.radius, m.radius, 2)
            if np.hypot(*p) < 0.9 * m.radius:
                break
        arr = [(t0 + int(round(np.hypot(p[0] - s[0], p[1] - s[1]) / c * m.sr)) + int(rng.integers(-1, 2)), k)
               for k, s in enumerate(m.sensor_locs)]
        if h % 10 == 3:
            arr.append((t0 + int(rng.integers(0, 40)), int(rng.integers(0, S))))
        stream += sorted(arr)
        t0 += int(rng.integers(300, 3000))
    res, ier, nfev = [], [], []
    for onset, k in stream:
        n0 = len(log.calls)
        r = m.locate(k, onset)
        for cl in log.calls[n0:]:
            ier.append(cl[1])
            nfev.append(cl[2])
        res.append([0.0, np.nan, np.nan] if r is None else [1.0, float(r[0]), float(r[1])])
    out.update({f"{pre}/trace/sensor": np.array([k for _, k in stream], np.int64),
                f"{pre}/trace/onset": np.array([o for o, _ in stream], np.int64),
                f"{pre}/trace/res": np.array(res), f"{pre}/trace/ier": np.array(ier, np.int32),
                f"{pre}/trace/nfev": np.array(nfev, np.int32)})
    return out


def main():
    import scipy.optimize

    load_reference()
    from onset_fingerprinting import multilateration as ml
    log = _FsolveLog(scipy.optimize.fsolve)
    ml.fsolve = log
    rng = np.random.default_rng(23)
    out = find_lag_cases(ml, rng)
    laglog = _LagLog(ml.find_lag)
    ml.find_lag = laglog
    for name, kw in PAIRED.items():
        out.update(paired(ml, rng, name, kw, log, laglog))
    ml.find_lag = laglog.fn
    for name, kw in M2D.items():
        out.update(multilaterate2d(ml, rng, name, kw, log))
    for name, kw in LIM.items():
        lag, a, b = ml.lag_intensity_map(**kw)
        pre = f"lim/{name}"
        out[f"{pre}/args"] = np.array(json.dumps(kw))
        out[f"{pre}/lag_sha"] = np.array(sha(lag))
        out[f"{pre}/lag"] = lag
        out[f"{pre}/a"], out[f"{pre}/b"] = a, b
    write_npz(HERE / "g23_locate2d.npz", out)
    print("fl near-ties:", int(out["fl/near_tie"].sum()), "of", len(out["fl/near_tie"]))


if __name__ == "__main__":
    main()
