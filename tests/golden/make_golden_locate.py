#!/usr/bin/env python3
"""Golden vectors g22_locate: the reference's own multilateration.py (lag maps, Multilaterate3D, the fsolve
trilateration, the locate state machine), run with scipy on the host.

Run in the build container only (after `make -C oracle ref`):   python tests/golden/make_golden_locate.py
scipy.optimize.fsolve is wrapped in the reference module's namespace while this runs so that every solve also
records fsolve's ier and info["nfev"] (the reference itself keeps only the root, and only when ier == 1).

Contents (every key is prefixed by its section):
  map/<case>/{args, map}           lag_map_3d / lag_map_2d (args: JSON of the call)
  m3d/<layout>/{args, sensor_locs, min, max, max_max, maps}  Multilaterate3D(**args): min_lags / max_lags as
                                   [S][S] (NaN on the diagonal), max_max_lags [S], lag_maps [S][S][n][n]
  legal/<layout>/{sensors, onsets, idx}   is_legal_3d queries [Q][3] -> [Q][2]
  solve3/{geom, delta, guess, root, ier, nfev}   solve_trilateration_3d: geom [K][9] = origin, a, b
  solve2/{geom, delta, guess, root, ier, nfev}   solve_trilateration (2-D; z = 0 in geom)
  trace/{audio, sensor, onset, counter, res_audio, res_plain}  Multilaterate3D.locate over an onset stream of a
                                   synthetic recording, with rec_audio (a ring holding audio[:counter]) and without;
                                   res_* [calls][3] = (returned?, x, y)
  rows/{groups, status, guess, xy} the recording's groups (reference detect_onsets_amplitude -> find_onset_groups ->
                                   fix_onsets) and the per-row replay of is_legal / is_legal_3d / trilaterate
                                   (status: ier, or -2 few channels, -3 illegal lag, -4 no legal cell)
"""
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

warnings.filterwarnings("ignore")

SR_RT = 96000
LAYOUTS = {
    # the realtime setup: three optical / magnetic sensors on the drumhead (realtime/audio.py:53-59)
    "rt3": dict(sensor_locations=[(0.9, 30, 0), (0.9, 150, 0), (0.9, 270, 0)], medium="drumhead", sr=SR_RT),
    # four microphones above the surface, in air
    "air4": dict(sensor_locations=[(1.05, 0, 8), (1.05, 90, 12), (1.1, 180, 8), (1.05, 270, 15)], medium="air",
                 sr=48000),
}


class _Ring:
    """rec_audio stand-in: .counter = samples written; [-k:] = the last k rows (the ring's read pattern)."""

    def __init__(self, audio, counter):
        self.audio, self.counter = audio, counter

    def __getitem__(self, idx):
        return self.audio[: self.counter][idx]


class _FsolveLog:
    def __init__(self, fsolve):
        self.fsolve, self.calls = fsolve, []

    def __call__(self, *a, **k):
        root, info, ier, msg = self.fsolve(*a, **k)
        self.calls.append((np.array(root, dtype=np.float64), int(ier), int(info["nfev"])))
        return root, info, ier, msg


def write_npz(path, arrays):
    """np.savez_compressed with fixed entry timestamps, so that a second run writes the same bytes."""
    import io
    import zipfile
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as z:
        for key in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[key]), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())


def strikes(rng, n, radius):
    p = []
    while len(p) < n:
        q = rng.uniform(-radius, radius, 2)
        if np.hypot(*q) < 0.85 * radius:
            p.append(q)
    return np.array(p)


def main():
    import scipy.optimize

    ref = load_reference()
    from onset_fingerprinting import multilateration as ml
    log = _FsolveLog(scipy.optimize.fsolve)
    ml.fsolve = log
    rng = np.random.default_rng(22)
    out = {}

    # ---- host formulas ----
    sos = [ml.speed_of_sound(sc, t, h, md) for sc in (1, 100, 1000) for t in (0.0, 20.0, 31.5) for h in (0.0, 0.5, 0.9)
           for md in ("air", "drumhead")]
    out["host/speed_of_sound"] = np.array(sos, np.float64)
    pts = np.concatenate([rng.normal(0, 20, (200, 3)), [[0.0, 0.0, 1.0], [1.0, 0.0, 0.0], [-3.0, -4.0, -2.0]]])
    out["host/xyz"] = pts
    out["host/c2p"] = np.array([ml.cartesian_to_polar(x, y) for x, y, _ in pts])
    out["host/c2p_r"] = np.array([ml.cartesian_to_polar(x, y, 17.78) for x, y, _ in pts])
    out["host/c2s"] = np.array([ml.cartesian_to_spherical(x, y, z) for x, y, z in pts])
    out["host/c2cyl"] = np.array([ml.cartesian_to_cylindrical(x, y, z, 7.0) for x, y, z in pts])
    rpt = np.stack([rng.uniform(0, 20, 200), rng.uniform(-400, 400, 200), rng.uniform(-90, 90, 200)], 1)
    out["host/rpt"] = rpt
    out["host/p2c"] = np.array([ml.polar_to_cartesian(r, p) for r, p, _ in rpt])
    out["host/s2c"] = np.array([ml.spherical_to_cartesian(r, p, t) for r, p, t in rpt])
    out["host/cyl2c"] = np.array([ml.cylindrical_to_cartesian(r, p, t) for r, p, t in rpt])

    # ---- lag maps ----
    ms = {name: ml.Multilaterate3D(**kw) for name, kw in LAYOUTS.items()}
    rt, air = ms["rt3"], ms["air4"]
    map_cases = {
        "rt3_s1_t1": ("3d", dict(mic_a=rt.sensor_locs[1], mic_b=rt.sensor_locs[0], sr=SR_RT, scale=1, medium="drumhead",
                                 tol=1)),
        "rt3_s1_t2": ("3d", dict(mic_a=rt.sensor_locs[2], mic_b=rt.sensor_locs[1], sr=SR_RT, scale=1, medium="drumhead",
                                 tol=2)),
        "rt3_s10_t1": ("3d", dict(mic_a=tuple(10 * v for v in rt.sensor_locs[0]),
                                  mic_b=tuple(10 * v for v in rt.sensor_locs[2]), sr=SR_RT, scale=10,
                                  medium="drumhead", tol=1)),
        "air4_s1_t1": ("3d", dict(mic_a=air.sensor_locs[3], mic_b=air.sensor_locs[1], sr=48000, scale=1, medium="air",
                                  tol=1)),
        "air4_s10_t2": ("3d", dict(mic_a=tuple(10 * v for v in air.sensor_locs[0]),
                                   mic_b=tuple(10 * v for v in air.sensor_locs[2]), sr=48000, scale=10, medium="air",
                                   tol=2)),
        "air4_s1_t2_c": ("3d", dict(mic_a=air.sensor_locs[2], mic_b=air.sensor_locs[0], sr=48000, scale=1, tol=2,
                                    c=air.c)),
        "2d_s1_t1": ("2d", dict(mic_a=(12.0, -3.5), mic_b=(-10.25, 7.0), sr=SR_RT, scale=1, medium="drumhead", tol=1)),
    }
    for name, (kind, kw) in map_cases.items():
        kw = {k: (tuple(float(x) for x in v) if isinstance(v, tuple) else v) for k, v in kw.items()}
        fn = ml.lag_map_3d if kind == "3d" else ml.lag_map_2d
        out[f"map/{name}/args"] = np.array(json.dumps(dict(kind=kind, **kw)))
        out[f"map/{name}/map"] = fn(**kw)

    # ---- Multilaterate3D extremes and maps ----
    for name, m in ms.items():
        S = len(m.sensor_locs)
        mn = np.full((S, S), np.nan, np.float32)
        mx = np.full((S, S), np.nan, np.float32)
        n = m.lag_maps[0][1].shape[0]
        maps = np.full((S, S, n, n), np.nan, np.float32)
        for i in range(S):
            for j in m.lag_maps[i]:
                mn[i, j], mx[i, j], maps[i, j] = m.min_lags[i][j], m.max_lags[i][j], m.lag_maps[i][j]
        out[f"m3d/{name}/args"] = np.array(json.dumps(LAYOUTS[name]))
        out[f"m3d/{name}/sensor_locs"] = np.array(m.sensor_locs, dtype=np.float64)
        out[f"m3d/{name}/min"], out[f"m3d/{name}/max"], out[f"m3d/{name}/maps"] = mn, mx, maps
        out[f"m3d/{name}/max_max"] = np.array(m.max_max_lags, dtype=np.float32)

    # ---- is_legal_3d queries ----
    for name, m in ms.items():
        S = len(m.sensor_locs)
        sens, ons, idx = [], [], []
        pts = strikes(rng, 1000, m.radius)
        for q in range(1000):
            s = [int(v) for v in rng.permutation(S)[:3]]
            d = [np.sqrt((pts[q][0] - m.sensor_locs[k][0]) ** 2 + (pts[q][1] - m.sensor_locs[k][1]) ** 2
                         + m.sensor_locs[k][2] ** 2) for k in s]
            t = [int(round(v / m.c * m.sr)) for v in d]
            if q % 5 == 0:
                t = [t[0], t[0] + int(rng.integers(-600, 600)), t[0] + int(rng.integers(-600, 600))]  # mostly no cell
            elif q % 5 == 1:
                t = [v + int(rng.integers(-4, 5)) for v in t]
            base = 10000 + int(rng.integers(0, 5000))
            o = [base + v - t[0] for v in t]
            sens.append(s)
            ons.append(o)
            idx.append(m.is_legal_3d((list(s), list(o))))
        out[f"legal/{name}/sensors"] = np.array(sens, np.int32)
        out[f"legal/{name}/onsets"] = np.array(ons, np.int64)
        out[f"legal/{name}/idx"] = np.array(idx, np.int32)

    # ---- trilateration ----
    def solve_cases(kind, K):
        geom, delta, guess, root, ier, nfev = [], [], [], [], [], []
        for k in range(K):
            if kind == 3:
                m = rt if k % 2 == 0 else air
                s = [int(v) for v in rng.permutation(len(m.sensor_locs))[:3]]
                loc = [np.array(m.sensor_locs[v], np.float64) for v in s]
                R = m.radius
            else:
                R = ml.DIAMETER / 2
                ang = rng.uniform(0, 360, 3)
                loc = [np.array(ml.polar_to_cartesian(0.9 * R, a) + (0.0,), np.float64) for a in ang]
            p = strikes(rng, 1, R)[0]
            dist = [np.sqrt((p[0] - v[0]) ** 2 + (p[1] - v[1]) ** 2 + v[2] ** 2) for v in loc]
            dda, ddb = dist[1] - dist[0], dist[2] - dist[0]
            case = k % 10
            if case in (1, 2):
                dda, ddb = dda + rng.normal(0, 3), ddb + rng.normal(0, 3)
            elif case == 3:
                dda, ddb = rng.uniform(40, 90) * rng.choice([-1, 1]), rng.uniform(40, 90)  # no point satisfies these
            x0 = p + rng.normal(0, 6, 2)
            if case == 4:
                x0 = loc[0][:2].copy()  # on the origin sensor
            elif case == 5:
                x0 = loc[1][:2].copy()
            elif case in (6, 7):
                x0 = np.round(rng.uniform(-R, R, 2)) - R % 1  # grid-cell guesses, as is_legal_3d makes them
            elif case == 8:
                x0 = rng.uniform(-4 * R, 4 * R, 2)
            n0 = len(log.calls)
            if kind == 3:
                ml.solve_trilateration_3d(tuple(loc[1]), tuple(loc[2]), tuple(loc[0]), dda, ddb, x0)
            else:
                ml.solve_trilateration(tuple(loc[1][:2]), tuple(loc[2][:2]), tuple(loc[0][:2]), dda, ddb, x0)
            assert len(log.calls) == n0 + 1
            r, e, nf = log.calls[-1]
            geom.append(np.concatenate(loc))
            delta.append([dda, ddb])
            guess.append(np.asarray(x0, np.float64))
            root.append(r)
            ier.append(e)
            nfev.append(nf)
        return dict(geom=np.array(geom), delta=np.array(delta), guess=np.array(guess), root=np.array(root),
                    ier=np.array(ier, np.int32), nfev=np.array(nfev, np.int32))

    for k, v in solve_cases(3, 2000).items():
        out[f"solve3/{k}"] = v
    for k, v in solve_cases(2, 300).items():
        out[f"solve2/{k}"] = v

    # ---- synthetic recording: strikes at known positions, delays distance / c * sr ----
    m = rt
    C, N, period = 3, 48000, 3000
    audio = np.zeros((N, C), np.float32)
    pts = strikes(rng, N // period - 1, m.radius)
    t_burst = np.arange(600)
    stream = []
    for h, p in enumerate(pts):
        t0 = 1500 + h * period
        for ch in range(C):
            s = m.sensor_locs[ch]
            d = np.sqrt((p[0] - s[0]) ** 2 + (p[1] - s[1]) ** 2 + s[2] ** 2)
            on = t0 + int(round(d / m.c * m.sr))
            f = 3000.0 + 700.0 * ch
            burst = 0.8 * np.exp(-t_burst / 120.0) * np.sin(2 * np.pi * f / m.sr * t_burst + 0.3 * h)
            audio[on:on + len(burst), ch] += burst.astype(np.float32)
            stream.append((on, ch))
        if h % 4 == 3:  # a spurious onset between strikes
            stream.append((t0 + 1700, int(rng.integers(0, C))))
    stream.sort()
    sensor = np.array([c for _, c in stream], np.int64)
    onset = np.array([o for o, _ in stream], np.int64)
    counter = (onset // 128 + 2) * 128  # the ring holds the hop that carried the onset and the next one
    out["trace/audio"], out["trace/sensor"], out["trace/onset"], out["trace/counter"] = audio, sensor, onset, counter
    for key, with_audio in (("res_audio", True), ("res_plain", False)):
        mm = ml.Multilaterate3D(**LAYOUTS["rt3"])
        res = []
        for c, o, n in zip(sensor, onset, counter):
            r = mm.locate(int(c), int(o), _Ring(audio, int(n)) if with_audio else None)
            res.append((0.0, np.nan, np.nan) if r is None else (1.0, float(r[0]), float(r[1])))
        out[f"trace/{key}"] = np.array(res, np.float64)

    # ---- grouped rows of the recording and the per-row replay ----
    ch, on, _ = ref.detection.detect_onsets_amplitude(audio, block_size=128, sr=SR_RT)
    groups = ref.detection.find_onset_groups(list(on), list(ch), max_distance=1000, min_channels=3)
    groups = ref.detection.fix_onsets(audio, np.asarray(groups), d=1, take_abs=True, onset_tolerance=30)
    status, guess, xy = [], [], []
    for row in groups:
        present = [(int(row[c]), c) for c in range(len(row)) if row[c] >= 0]
        present.sort()
        if len(present) < 3:
            status.append(-2), guess.append((np.nan, np.nan)), xy.append((np.nan, np.nan))
            continue
        s = [c for _, c in present[:3]]
        o = [v for v, _ in present[:3]]
        if not (m.is_legal(s[0], s[1], o[1] - o[0]) and m.is_legal(s[0], s[2], o[2] - o[0])):
            status.append(-3), guess.append((np.nan, np.nan)), xy.append((np.nan, np.nan))
            continue
        grp = (list(s), list(o))
        res = m.is_legal_3d(grp)
        if res == (0, 0):
            status.append(-4), guess.append((np.nan, np.nan)), xy.append((np.nan, np.nan))
            continue
        g0 = np.array(res) - m.radius
        n0 = len(log.calls)
        m.trilaterate(grp, initial_guess=g0)
        assert len(log.calls) == n0 + 1
        r, e, _ = log.calls[-1]
        status.append(e), guess.append(tuple(g0)), xy.append(tuple(r))
    out["rows/groups"] = np.asarray(groups, np.int64)
    out["rows/status"] = np.array(status, np.int32)
    out["rows/guess"] = np.array(guess, np.float64)
    out["rows/xy"] = np.array(xy, np.float64)

    path = HERE / "g22_locate.npz"
    write_npz(path, out)
    print(f"wrote {path} ({path.stat().st_size} bytes); solve3 ier counts",
          np.unique(out["solve3/ier"], return_counts=True), "rows", np.unique(out["rows/status"], return_counts=True),
          "trace located", int(out["trace/res_audio"][:, 0].sum()), int(out["trace/res_plain"][:, 0].sum()))


if __name__ == "__main__":
    main()
