"""Shared inputs of the planar-locator device tests (tests/test_gpu_locate2d_device.py and its CPU companion), all
made on the CPU:

* ``HostModel``: ``Multilaterate.locate`` in plain numpy on the tables of golden g23 (``m2d/<layout>``), with
  scipy's fsolve when scipy is present.  It only plans inputs (which hops of a stream complete a group); no expected
  value of a GPU test comes from it.
* ``group_rows``: the batched test's groups, built from a trace's hits plus crafted rows.
* ``head_stream`` / ``hop_plan``: the hop test's synthetic recording (decaying bursts at the arrival times of random
  points on the head, as tests/golden/make_golden_hoplocate.py builds its recordings) and what the oracle's detector
  and the model make of it hop by hop.
"""
import functools
import json

import numpy as np

import oracle
from oracle.locate_kernels import legal_mask
from tests.conftest import load_golden

LAYOUTS = ("m3", "m4air")
HOP, SR = 128, 96000
DETECTOR = dict(hipass_freq=0, fast_ar=(3.0, 800), slow_ar=(8000, 8000), on_threshold=0.45, off_threshold=0.45,
                cooldown=1323, backtrack=False)
PERIOD, BURST, N_HITS, FIRST = 3000, 600, 12, 1500


@functools.lru_cache(maxsize=None)
def g23():
    return load_golden("g23_locate2d")


def layout_args(name):
    return json.loads(str(g23()[f"m2d/{name}/args"]))


def trace(name):
    g = g23()
    pre = f"m2d/{name}/trace"
    return g[f"{pre}/sensor"], g[f"{pre}/onset"], g[f"{pre}/res"]


class HostModel:
    """Multilaterate (multilateration.py:578-733) on the golden's tables."""

    def __init__(self, name):
        from onset_fingerprinting_amd import multilateration as ml
        g, kw = g23(), layout_args(name)
        self.radius = kw.get("drum_diameter", ml.DIAMETER) / 2
        self.sr = kw["sr"]
        self.c = ml.speed_of_sound(100, medium=kw.get("medium", "drumhead"))
        self.spc = self.sr / self.c
        self.locs = g[f"m2d/{name}/sensor_locs"]
        self.maps, self.mn, self.mx = g[f"m2d/{name}/maps"], g[f"m2d/{name}/min"], g[f"m2d/{name}/max"]
        self.mml = g[f"m2d/{name}/max_max"]
        self.ongoing = []

    def is_legal(self, a, b, lag):
        return bool(self.mn[a, b] < lag < self.mx[a, b])

    def cell(self, sens, ons):
        side = self.maps.shape[2]
        mask = legal_mask(self.maps[sens[0], sens[1]], self.maps[sens[0], sens[2]], float(ons[1] - ons[0]),
                          float(ons[2] - ons[0]), self.spc)
        k = int(np.argmax(mask))
        return k % side, k // side

    def solve(self, sens, ons, guess):
        """True when the TDoA system converges from `guess` (scipy present), else None: not known here."""
        try:
            from scipy.optimize import fsolve
        except ImportError:
            return None
        o, a, b = (self.locs[s] for s in sens[:3])
        da, db = ((ons[k] - ons[0]) * self.c / self.sr for k in (1, 2))

        def f(p):
            d0 = np.hypot(*(p - o))
            return [np.hypot(*(p - a)) - d0 - da, np.hypot(*(p - b)) - d0 - db]

        def jac(p):
            u0 = (p - o) / np.hypot(*(p - o))
            return [(p - a) / np.hypot(*(p - a)) - u0, (p - b) / np.hypot(*(p - b)) - u0]

        return fsolve(f, guess, fprime=jac, xtol=0.01, maxfev=20, full_output=True)[2] == 1

    def locate(self, sensor, onset):
        """'located' (also when a cell was found and the solver is absent), 'no root' for a search that found a cell
        whose solve did not converge, else None; the last two are the reference's None."""
        new = []
        for group in self.ongoing:
            lag = onset - group[1][0]
            if sensor not in group[0]:
                if self.is_legal(group[0][0], sensor, lag):
                    group = (group[0] + [sensor], group[1] + [onset])
                    if len(group[0]) == 3:
                        res = self.cell(*group)
                        if res != (0, 0):
                            self.ongoing = new
                            ok = self.solve(group[0], group[1], np.array(res, np.float64) - self.radius)
                            return "located" if ok in (True, None) else "no root"
                    new.append(group)
            if lag <= self.mml[group[0][0]]:
                new.append(group)
        new.append(([sensor], [onset]))
        self.ongoing = new
        return None


def trace_hits(name):
    """The trace's onsets as rows [S] (-1: channel absent): a row ends where its sensor repeats or the lag from the
    row's first onset passes the largest legal one."""
    sens, ons, _ = trace(name)
    S, mml = len(layout_args(name)["sensor_locations"]), float(np.max(g23()[f"m2d/{name}/max_max"]))
    rows, cur, first = [], None, 0
    for s, o in zip(sens, ons):
        if cur is None or cur[s] >= 0 or o - first > mml:
            cur, first = np.full(S, -1, np.int64), int(o)
            rows.append(cur)
        cur[s] = o
    return rows


SWAPPED_ROWS = 40


@functools.lru_cache(maxsize=None)
def swapped_stream(name="m3"):
    """(sensors int32 [3 n], onsets int64 [3 n]) for the first n = SWAPPED_ROWS full rows of ``trace_hits``: each row
    is fed with its two earliest arrivals exchanged, then the third, so a row's second call lies before the onset
    its first call seeded a group with (or on it, where the two arrive in one sample).  The golden traces never go
    back in time; this stream is where the planar routine has to take a negative lag as it is (the 3-D one would
    swap)."""
    full = [r for r in trace_hits(name) if (r >= 0).all()][:SWAPPED_ROWS]
    assert len(full) == SWAPPED_ROWS
    sens, ons = [], []
    for r in full:
        order = [int(k) for k in np.argsort(r, kind="stable")[:3]]
        for k in (order[1], order[0], order[2]):
            sens.append(k)
            ons.append(int(r[k]))
    return np.array(sens, np.int32), np.array(ons, np.int64)


def no_cell_lags(model, o, a, b):
    """Two positive lags (so that `o` stays the earliest), each legal for its pair, that meet in no cell of the grid."""
    for la in range(int(model.mx[o, a]) - 1, 0, -7):
        for lb in range(1, la, 7):
            if model.is_legal(o, a, la) and model.is_legal(o, b, lb) and model.cell((o, a, b), (0, la, lb)) == (0, 0):
                return la, lb
    raise AssertionError("every pair of legal lags meets somewhere")


def row_kind(model, row):
    """What the row rule makes of one row, by the numpy model: 'few', 'illegal', 'no cell' or 'cell'."""
    order = sorted((int(v), k) for k, v in enumerate(row) if v >= 0)[:3]
    if len(order) < 3:
        return "few"
    sens, ons = [k for _, k in order], [v for v, _ in order]
    if not (model.is_legal(sens[0], sens[1], ons[1] - ons[0]) and model.is_legal(sens[0], sens[2], ons[2] - ons[0])):
        return "illegal"
    return "no cell" if model.cell(sens, ons) == (0, 0) else "cell"


CAP = 48


@functools.lru_cache(maxsize=None)
def group_rows(name):
    """groups int64 [2, CAP, S] and n_groups [2] (the second clip shorter than the capacity): the trace's hits, then
    crafted rows: a missing channel, fewer than three channels, a tie on the onset, an illegal lag, lags without a
    common cell."""
    model = HostModel(name)
    hits = [r for r in trace_hits(name) if (r >= 0).sum() >= 3]
    S = len(hits[0])
    full = [r for r in hits if (r >= 0).all()]
    assert len(full) >= 40
    crafted = []
    r = full[0].copy()
    r[int(np.argmax(r))] = -1            # the latest channel missing: S - 1 channels remain
    crafted.append(r)
    r = full[1].copy()
    r[np.argsort(r)[2:]] = -1            # two channels
    crafted.append(r)
    crafted.append(np.full(S, -1, np.int64))
    r = full[2].copy()
    order = np.argsort(r, kind="stable")
    r[order[2]] = r[order[1]]            # second and third arrive in the same sample
    crafted.append(r)
    r = full[3].copy()
    r[np.argsort(r, kind="stable")[2:]] += 5000  # the third arrival far past every legal lag
    crafted.append(r)
    la, lb = no_cell_lags(model, 0, 1, 2)
    r = np.full(S, -1, np.int64)
    r[0], r[1], r[2] = 7000, 7000 + la, 7000 + lb
    crafted.append(r)
    groups = np.full((2, CAP, S), -1, np.int64)
    pool = full[4:] + [h for h in hits if not (h >= 0).all()]
    first = crafted + pool[:CAP - len(crafted)]
    second = pool[CAP - len(crafted):][:CAP]
    for c, rows in enumerate((first, second)):
        for k, r in enumerate(rows):
            groups[c, k] = r
    n_groups = np.array([CAP, min(len(second), CAP) - 5], np.int64)
    assert n_groups[1] >= 10
    groups.setflags(write=False)
    return groups, n_groups


@functools.lru_cache(maxsize=None)
def head_stream(name="m3", seed=31):
    """float32 [n, S]: N_HITS strikes at random points of the head, one decaying burst per sensor at its arrival time,
    and a spurious burst on one channel after every fourth strike."""
    model = HostModel(name)
    S = len(model.locs)
    rng = np.random.default_rng(seed)
    n = (FIRST + (N_HITS + 2) * PERIOD) // HOP * HOP
    audio = np.zeros((n, S), np.float64)
    t = np.arange(BURST)
    for h in range(N_HITS):
        while True:
            p = rng.uniform(-model.radius, model.radius, 2)
            if np.hypot(*p) < 0.85 * model.radius:
                break
        t0 = FIRST + h * PERIOD
        for ch in range(S):
            on = t0 + int(round(np.hypot(*(p - model.locs[ch])) / model.c * model.sr))
            f = 3000.0 + 700.0 * ch
            audio[on:on + BURST, ch] += 0.8 * np.exp(-t / 120.0) * np.sin(2 * np.pi * f / model.sr * t + 0.3 * h)
        if h % 4 == 3:
            ch = int(rng.integers(0, S))
            audio[t0 + 1700:t0 + 1700 + BURST, ch] += 0.5 * np.exp(-t / 120.0) * np.sin(2 * np.pi * 0.04 * t)
    audio = (np.round(audio * 4096) / 4096).astype(np.float32)
    audio.setflags(write=False)
    return audio


@functools.lru_cache(maxsize=None)
def hop_plan(name="m3"):
    """Per hop with onsets: (hop, outcome) where outcome is what feeding the oracle detector's sorted onsets to the
    model until one returns gives: 'located', 'no root' or None."""
    audio = head_stream(name)
    det = oracle.OracleDetector(audio.shape[1], HOP, sr=SR, **DETECTOR)
    model = HostModel(name)
    plan = []
    for h in range(len(audio) // HOP):
        ch, d, _ = det(np.ascontiguousarray(audio[h * HOP:(h + 1) * HOP]))
        if len(ch) == 0:
            continue
        res = None
        for i in np.argsort(d, kind="stable"):
            res = model.locate(int(ch[i]), h * HOP + int(d[i]))
            if res == "located":
                break
        plan.append((h, res))
    return plan
