"""Case tables and exact numpy references for the locator kernels of csrc/ofp_locate.hip, csrc/ofp_locate2d.hip and
first_legal / med5 of csrc/ofp_locate_dev.h, one by one -- TEST INFRASTRUCTURE ONLY.
tests/test_gpu_locate_kernels.py runs the kernels on these tables; tests/test_locate_kernels_cpu.py shows that the
references reproduce the committed goldens and that every table has the edges it names.  Nothing here calls the code
under test or torch; every reference is written from the formulas in the kernels' header comments and the
docstrings of onset_fingerprinting_amd/multilateration.py.

Everything is compared for equality, because kernel and reference compute the same numbers:

* geometry is fp64 with IEEE sqrt and division and no contraction, in the order the kernels write it;
* the correlation inputs are integers in [-127, 127] divided by 256, so every product is a multiple of 2**-16 below
  1/4 and every sum of up to 4096 of them is exact in fp64 in any order (order_independent() shows it per row); the
  one rounding to fp32 is then the same on both sides;
* the legality search, the counting sort and the vote are integer work on integer-valued maps.

One bit is left open: the sign of an extreme that is zero.  A map can hold cells of -0.0 (rint of a small negative
lag) next to cells of +0.0; np.minimum and np.maximum return either operand when both are zero, so the sign
np.nanmin / np.nanmax report depends on numpy's reduction order, and there is no reference for it.  plus_zero() maps
both sides to +0.0 for the extremes; the maps themselves are compared with their signs.

Two outputs are bounded instead: the polar coordinates (atan2 and a product by 180 / pi; 4 ulp of fp64) and the
intensity maps (acos, cos and log10 in fp64, rounded once to fp32; one fp32 ulp).
"""
import functools

import numpy as np
from scipy.ndimage import median_filter
from scipy.signal import find_peaks

f32, f64 = np.float32, np.float64
i32, i64 = np.int32, np.int64
WG, WAVE = 256, 64  # workgroup and wavefront of the kernels
INT_MIN = -2 ** 31

LOCATE_UNUSED, LOCATE_FEW_CHANNELS, LOCATE_ILLEGAL_LAG, LOCATE_NO_CELL = -1, -2, -3, -4
PAIRED_OK, PAIRED_UNUSED, PAIRED_NO_CHANNEL = 0, -1, -2
PAIRED_NEG_WINDOW, PAIRED_EMPTY_WINDOW, PAIRED_BAD_HIT = -5, -6, -7


# ---- host formulas (multilateration.py's docstrings) ------------------------------------------------------------

def speed_of_sound(scale=1, temperature=20.0, humidity=0.5, medium="air"):
    if medium != "air":
        return scale * 82
    return scale * (331.3 + 0.606 * temperature) * (1 + 0.0124 * humidity)


def grid_3d(d, scale, tol):
    r = int(np.round(d, 1) * scale) // 2
    return r, float((r + tol * scale) ** 2)


def grid_2d(d, scale, tol):
    r = int(np.round(d * scale / 2))
    return r, float((r + tol * scale) ** 2)


def polar_to_cartesian(r, phi):
    a = np.radians(phi)
    return r * np.cos(a), r * np.sin(a)


def spherical_to_cartesian(r, phi, theta):
    p = np.radians(phi)
    t = np.radians(-theta if theta < 0 else 90 - theta)
    return r * np.cos(p) * np.sin(t), r * np.sin(p) * np.sin(t), r * np.cos(t)


def cartesian_to_polar(x, y, r):
    return np.sqrt(x ** 2 + y ** 2) / r, np.degrees(np.arctan2(y, x) % (2 * np.pi))


def sensors3(s):
    s = np.array(s, f64)
    if s.shape[1] == 2:
        s = np.concatenate([s, np.zeros((len(s), 1))], 1)
    return np.ascontiguousarray(s)


# ---- 1. ofp_lag_maps: k_lag_maps, k_lag_minmax ----------------------------------------------------------------

def lag_maps_ref(sensors, r, c, sr, mask_r2, floor=-np.inf):
    """maps float32 [S, S, side, side], nanmin and nanmax float32 [S, S] (NaN for a map without a cell): map (i, j)
    holds rint((|p - s_j| / c - |p - s_i| / c) * sr) at p = (col - r, row - r, 0), NaN where col^2 + row^2 (centred)
    exceeds mask_r2, where the value is below `floor`, and on i == j."""
    s = sensors3(sensors)
    S, side = len(s), 2 * r + 1
    g = np.arange(-r, r + 1, dtype=f64)
    x, y = g[None, :], g[:, None]
    lag = []
    for k in range(S):
        dx, dy, dz = x - s[k, 0], y - s[k, 1], 0.0 - s[k, 2]
        lag.append(np.sqrt(dx * dx + dy * dy + dz * dz) / c)
    outside = (x * x + y * y) > mask_r2
    maps = np.full((S, S, side, side), np.nan, f32)
    for i in range(S):
        for j in range(S):
            if i == j:
                continue
            v = np.rint((lag[j] - lag[i]) * sr).astype(f32)
            v[outside] = np.nan
            with np.errstate(invalid="ignore"):
                v[v.astype(f64) < floor] = np.nan
            maps[i, j] = v
    return maps, *minmax_ref(maps)


def plus_zero(a):
    """-0.0 -> +0.0, everything else (NaN included) unchanged."""
    return np.asarray(a) + np.zeros((), np.asarray(a).dtype)


def minmax_ref(maps):
    S = maps.shape[0]
    flat = maps.reshape(S, S, -1)
    some = ~np.isnan(flat).all(-1)
    mn, mx = np.full((S, S), np.nan, f32), np.full((S, S), np.nan, f32)
    mn[some] = np.nanmin(flat[some], -1)
    mx[some] = np.nanmax(flat[some], -1)
    return mn, mx


MAP_SHAPES = ((2, 0), (2, 7), (3, 8), (5, 11), (64, 1))  # (S, r): 1, 225, 289, 529 and 9 cells
MAP_VARIANTS = ("open", "circle", "centre", "none", "floor_some", "floor_all")
MAP_MEDIA = ((8200.0, 96000.0), (speed_of_sound(100, medium="air"), 48000.0))  # (c in cm/s, sr)


def map_sensors(S, r, seed):
    """S sensors around a grid of radius r: off the plane (z != 0) except the first, the second exactly on a grid
    point of the plane."""
    rng = np.random.default_rng(seed)
    s = np.concatenate([rng.uniform(-1.3 * (r + 1), 1.3 * (r + 1), (S, 2)), rng.uniform(0.5, 9.0, (S, 1))], 1)
    s[0, 2] = 0.0
    s[1] = (float(min(r, 3)), float(-min(r, 2)), 0.0)
    return s


def map_cases():
    """(name, sensors, r, c, sr, mask_r2, floor) per launch."""
    out = []
    for k, (S, r) in enumerate(MAP_SHAPES):
        c, sr = MAP_MEDIA[k % 2]
        s = map_sensors(S, r, 100 + k)
        for v in MAP_VARIANTS:
            mask_r2 = {"circle": float(r * r), "centre": 0.0, "none": -1.0}.get(v, np.inf)
            floor = {"floor_some": 0.0, "floor_all": np.inf}.get(v, -np.inf)
            out.append((f"S{S}_r{r}_{v}", s, r, c, sr, mask_r2, floor))
    return out


# ---- 2. ofp_locate_legal: k_legal, first_legal ------------------------------------------------------------------

def legal_mask(m1, m2, lag1, lag2, tol):
    m1, m2 = m1.astype(f64).reshape(-1), m2.astype(f64).reshape(-1)
    with np.errstate(invalid="ignore"):
        return (m1 < lag1 + tol) & (m1 > lag1 - tol) & (m2 < lag2 + tol) & (m2 > lag2 - tol)


def legal_ref(maps, sens, onsets, tol):
    """int32 [G, 2]: (col, row) of np.argmax over the flattened mask, (0, 0) when no cell is legal, (-1, -1) for a
    sensor index outside the maps."""
    S, side = maps.shape[0], maps.shape[2]
    out = np.zeros((len(sens), 2), i32)
    for g, (s, o) in enumerate(zip(sens, onsets)):
        if min(s) < 0 or max(s) >= S:
            out[g] = -1
            continue
        k = int(np.argmax(legal_mask(maps[s[0], s[1]], maps[s[0], s[2]], float(o[1] - o[0]), float(o[2] - o[0]), tol)))
        out[g] = (k % side, k // side)
    return out


LEGAL_SIDES = (1, 15, 17)
LEGAL_FLAT = (0, 255, 256, 257)  # and cells - 1


def legal_table(side, seed=7):
    """Synthetic integer maps [S, S, side, side]: case q owns sensor q as origin and the maps (q, q+1), (q, q+2), so
    one launch holds every case.  Returns maps, sens int32 [G, 3], onsets int64 [G, 3], tol, and per case
    (name, expected flat index of the first legal cell or None)."""
    rng = np.random.default_rng(seed + side)
    cells = side * side
    plans = []  # (name, fill(m1, m2, lag1, lag2), flat index of the first legal cell or None)
    tol = 2.0

    def only(k):
        def fill(m1, m2, l1, l2):
            m1[k], m2[k] = l1 + 1, l2 - 1
        return fill

    for k in sorted({f for f in LEGAL_FLAT + (cells - 1,) if f < cells}):
        plans.append((f"only_{k}", only(k), k))

    def scattered(m1, m2, l1, l2):
        for k in scattered.cells:
            m1[k], m2[k] = l1 + int(rng.integers(-1, 2)), l2 + int(rng.integers(-1, 2))
    scattered.cells = sorted(rng.choice(cells, min(cells, 6), replace=False).tolist())
    plans.append(("scattered", scattered, scattered.cells[0]))

    edge_at = min(cells - 1, 5)

    def edges(m1, m2, l1, l2):  # the comparison is strict: a value at lag +- tol is not legal
        for k, (d1, d2) in enumerate(((-2, 0), (2, 0), (0, -2), (0, 2), (2, 2))):
            if k < edge_at:
                m1[k], m2[k] = l1 + d1, l2 + d2
        m1[edge_at], m2[edge_at] = l1 + 1, l2 - 1
    plans.append(("edges_then_legal", edges, edge_at))

    def edges_only(m1, m2, l1, l2):
        for k, (d1, d2) in enumerate(((-2, 0), (2, 0), (0, -2), (0, 2), (2, 2))):
            if k < cells:
                m1[k], m2[k] = l1 + d1, l2 + d2
    plans.append(("edges_only", edges_only, None))

    def nans(m1, m2, l1, l2):  # a NaN in either map is never legal
        for k in range(min(cells - 1, 2 * side)):
            m1[k], m2[k] = (np.nan, l2) if k % 2 else (l1, np.nan)
        m1[cells - 1], m2[cells - 1] = l1, l2
    plans.append(("nans_then_legal", nans, cells - 1))

    def all_nan(m1, m2, l1, l2):
        m1[:], m2[:] = np.nan, np.nan
    plans.append(("all_nan", all_nan, None))
    plans.append(("none", lambda m1, m2, l1, l2: None, None))

    G = len(plans)
    S = G + 2
    maps = (1000 + rng.integers(0, 50, (S, S, cells))).astype(f32)  # far from every lag
    sens, onsets, info = np.zeros((G + 2, 3), i32), np.zeros((G + 2, 3), i64), []
    for q, (name, fill, want) in enumerate(plans):
        l1, l2 = int(rng.integers(-40, 40)), int(rng.integers(-40, 40))
        a, b = q + 1, q + 2
        fill(maps[q, a], maps[q, b], l1, l2)
        o0 = int(rng.integers(0, 10 ** 9))
        sens[q], onsets[q] = (q, a, b), (o0, o0 + l1, o0 + l2)
        info.append((name, want))
    sens[G], onsets[G] = (0, S, 1), (5, 6, 7)      # a sensor index out of range
    sens[G + 1], onsets[G + 1] = (-1, 0, 1), (5, 6, 7)
    info += [("sensor_high", "refused"), ("sensor_negative", "refused")]
    return maps.reshape(S, S, side, side), sens, onsets, tol, info


# ---- 3. ofp_locate_groups: k_locate_rows, k_locate_solve ------------------------------------------------------------

M3D_LOCATIONS = [[1.05, 10, 0], [0.95, 80, 25], [1.1, 150, -70], [1.0, 220, 10], [0.9, 300, 40]]
M3D_DIAMETERS = (14, 16)  # r = 7 and 8: 225 and 289 cells
M3D_SR, M3D_C = 44100, 82.0  # Multilaterate3D(..., sr=44100, c=82.0): 8200 cm/s
ROWS_CAP = 7
ROWS_N_GROUPS = (0, 3, 7, 9)  # none, fewer than cap_groups, cap_groups, more


class M3D:
    """The tables Multilaterate3D(M3D_LOCATIONS, drum_diameter=d, sr=M3D_SR, c=M3D_C) builds, from its docstring."""

    def __init__(self, d):
        self.c, self.sr, self.radius = M3D_C * 100, M3D_SR, d / 2
        self.sensors = sensors3([spherical_to_cartesian(x[0] * self.radius, x[1], x[2]) for x in M3D_LOCATIONS])
        self.spc = self.sr / self.c
        self.r, mask_r2 = grid_3d(d, 1, 2)
        self.maps, self.mn, self.mx = lag_maps_ref(self.sensors, self.r, self.c, self.sr, mask_r2, floor=-self.spc)


@functools.lru_cache(None)
def m3d(d):
    return M3D(d)


def replay_row(m, row):
    """One row of locate_groups_device on the host: (status, guess, (origin, a, b), (lag_a, lag_b)); status 0 means
    'to be solved' from that guess, geometry and lags."""
    present = sorted((int(v), c) for c, v in enumerate(row) if v >= 0)[:3]
    nan2 = (np.nan, np.nan)
    if len(present) < 3:
        return LOCATE_FEW_CHANNELS, nan2, None, None
    s, o = [c for _, c in present], [v for v, _ in present]
    for k in (1, 2):
        if not (m.mn[s[0], s[k]] < o[k] - o[0] < m.mx[s[0], s[k]]):
            return LOCATE_ILLEGAL_LAG, nan2, tuple(s), None
    col, rw = legal_ref(m.maps, [s], [o], m.spc)[0]
    if col == 0 and rw == 0:
        return LOCATE_NO_CELL, nan2, tuple(s), None
    guess = (float(col) - m.radius, float(rw) - m.radius)
    if s[1] == 1:
        s[1:] = [0, 1]
        o[1:] = o[2:0:-1]
    return 0, guess, tuple(s), (o[1] - o[0], o[2] - o[0])


def replay_rows(m, groups, n_groups):
    """status int32 [n_clips, cap] (0: solved on the device), guess [.., 2], geom [.., 9], delta [.., 2]."""
    n_clips, cap, _ = groups.shape
    status = np.zeros((n_clips, cap), i32)
    guess = np.full((n_clips, cap, 2), np.nan)
    geom, delta = np.zeros((n_clips, cap, 9)), np.zeros((n_clips, cap, 2))
    for c in range(n_clips):
        for g in range(cap):
            if n_groups is not None and g >= min(int(n_groups[c]), cap):
                status[c, g] = LOCATE_UNUSED
                continue
            st, gs, s, lags = replay_row(m, groups[c, g])
            status[c, g], guess[c, g] = st, gs
            if st == 0:
                geom[c, g] = m.sensors[list(s)].reshape(-1)
                delta[c, g] = (lags[0] / m.sr * m.c, lags[1] / m.sr * m.c)
    return status, guess, geom, delta


def hit_row(m, p, C, base):
    """Onsets of a hit at p = (x, y) on the head: base + rint(distance / c * sr) per channel."""
    d = np.sqrt((p[0] - m.sensors[:C, 0]) ** 2 + (p[1] - m.sensors[:C, 1]) ** 2 + m.sensors[:C, 2] ** 2)
    return (base + np.rint(d / m.c * m.sr)).astype(i64)


@functools.lru_cache(None)
def rows_table(d, C):
    """groups int64 [4, ROWS_CAP, C], n_groups int64 [4], and {property: (clip, row)} of the rows built for it.  The
    special rows sit in the two clips whose rows are all used."""
    m = m3d(d)
    rng = np.random.default_rng(1000 * d + C)
    S = len(m.sensors)
    pts = [(x, y) for x in range(-m.r, m.r + 1) for y in range(-m.r, m.r + 1) if x * x + y * y <= (m.r - 1) ** 2]
    hits = [hit_row(m, pts[k], C, int(rng.integers(0, 10 ** 6))) for k in rng.permutation(len(pts))]
    solved = [h for h in hits if replay_row(m, h)[0] == 0]
    special = {}

    def first(name, rows, pred):
        for h in rows:
            if pred(h):
                special[name] = h
                return
        raise AssertionError(f"rows_table({d}, {C}): no row for {name}")

    order = lambda h: [c for _, c in sorted((int(v), c) for c, v in enumerate(h) if v >= 0)[:3]]
    first("second_is_1", solved, lambda h: order(h)[1] == 1)
    first("plain", solved, lambda h: order(h)[1] != 1)
    if C > 3:
        first("not_first_three", solved, lambda h: max(order(h)) > 2)
        h = special["not_first_three"].copy()
        h[[c for c in range(C) if c not in order(h)][0]] = -1
        special["absent"] = h
    few = solved[3].copy()
    few[1:] = -1
    few[rng.integers(1, C)] = few[0] + 3
    special["few_two"] = few
    special["few_none"] = np.full(C, -1, i64)

    def tied(k):  # the k channels after the earliest share its onset (lags 0): ties resolve by channel index
        def pred(h):
            t = h.copy()
            t[order(h)[1:k]] = t[order(h)[0]]
            pred.row = t
            return replay_row(m, t)[0] == 0 and order(t) != order(h)
        return pred
    for name, k in (("tie_two", 2), ("tie_three", 3)):
        p = tied(k)
        try:
            first(name, solved, p)
        except AssertionError:  # no reordering tie that still locates: any tie
            t = solved[0].copy()
            t[order(t)[1:k]] = t[order(t)[0]]
            p.row = t
        special[name] = p.row
    # a lag equal to the pair's largest map value: is_legal is strict
    o, a, b = 0, 1, 2
    at_max = np.full(C, -1, i64)
    at_max[[o, a, b]] = (500, 500 + int(m.mx[o, a]), 501)
    special["lag_at_max"] = at_max
    below = at_max.copy()
    below[a] -= 1
    special["lag_below_max"] = below
    # both lags legal on their own, no cell fits both
    found = None
    for l1 in range(1, int(m.mx[o, a])):
        for l2 in range(int(m.mx[o, b]) - 1, 0, -1):
            t = np.full(C, -1, i64)
            t[[o, a, b]] = (900, 900 + l1, 900 + l2)
            if replay_row(m, t)[0] == LOCATE_NO_CELL:
                found = t
                break
        if found is not None:
            break
    assert found is not None, "no pair of lags without a common cell"
    special["no_cell"] = found
    groups = np.zeros((len(ROWS_N_GROUPS), ROWS_CAP, C), i64)
    where = {}
    slots = [(c, g) for c in (2, 3) for g in range(ROWS_CAP)]
    assert len(special) <= len(slots)
    fill = iter(solved[5:])
    for c in range(groups.shape[0]):
        for g in range(ROWS_CAP):
            groups[c, g] = next(fill)
    for (c, g), (name, h) in zip(slots, special.items()):
        groups[c, g], where[name] = h, (c, g)
    return groups, np.array(ROWS_N_GROUPS, i64), where


# ---- 4. ofp_locate_section: k_section, med5 ---------------------------------------------------------------------

SECTION_N = (3, 4, 5, 257, 258, 600)
SECTION_LD = (2, 5)


def section_cases():
    """(n, ld, c0, c1, x float32 [n, ld]) with small-integer samples, so medians tie."""
    out = []
    for k, n in enumerate(SECTION_N):
        for ld in SECTION_LD:
            rng = np.random.default_rng(40 + 7 * k + ld)
            x = rng.integers(-3, 4, (n, ld)).astype(f32)
            for c0, c1 in ((0, ld - 1), (ld - 1, ld - 1), (ld // 2, 0)):
                out.append((n, ld, c0, c1, x))
    return out


def section_ref(x, c0, c1):
    """float32 [2, n - 1]: median of 5 along time ('reflect'), first difference, values >= 0 zeroed, absolute."""
    m = median_filter(x.astype(f32), size=(5, 1), mode="reflect")[:, [c0, c1]]
    d = np.diff(m, axis=0)
    d[d >= 0] = 0
    return np.ascontiguousarray(np.abs(d).T.astype(f32))


# ---- 5. ofp_find_lags: k_find_lags ------------------------------------------------------------------------------

FIND_SHAPES = ((1, 1), (1, 4096), (4096, 1), (4096, 4096), (128, 129), (129, 129), (256, 257))
FIND_TOP = (0, 1, 16)
UNIT = 1.0 / 256


def correlate32(a, b):
    """np.correlate(a, b, "full") in fp64, rounded once to float32."""
    with np.errstate(invalid="ignore", over="ignore"):
        return np.correlate(a.astype(f64), b.astype(f64), "full").astype(f32)


def order_independent(a, b):
    """Every entry of the correlation summed term by term in ascending and in descending order gives the same fp64
    value (np.cumsum adds sequentially; the zeros outside the overlap change no sum)."""
    a, b = a.astype(f64), b.astype(f64)
    if len(a) < 1 or len(b) < 1 or not (np.isfinite(a).all() and np.isfinite(b).all()):
        return True  # an empty or a non-finite row has no sums to compare: NaN / inf positions do not depend on the order
    lb = len(b)
    pad = np.concatenate([np.zeros(lb - 1), a, np.zeros(lb - 1)])
    win = np.lib.stride_tricks.sliding_window_view(pad, lb)  # win[j, n] = a[n + j - (lb - 1)]
    for j in range(0, len(win), 512):
        p = win[j:j + 512] * b[None, :]
        if not np.array_equal(np.cumsum(p, 1)[:, -1], np.cumsum(p[:, ::-1], 1)[:, -1]):
            return False
    return True


def find_ref(a, b, top_n):
    """lag, peak_lag int32 [top_n], peak_val float32 [top_n], n_peaks for one row pair (find_lags_device's
    docstring): an empty row gives (INT_MIN, -2), a non-finite correlation n_peaks -1 and no peaks."""
    pl, pv = np.zeros(top_n, i32), np.full(top_n, np.nan, f32)
    if len(a) < 1 or len(b) < 1:
        return INT_MIN, pl, pv, -2
    cc = correlate32(a, b)
    lag = int(np.argmax(cc)) - (len(a) - 1)
    if top_n == 0:
        return lag, pl, pv, 0
    if not np.isfinite(cc).all():
        return lag, pl, pv, -1
    peaks, _ = find_peaks(cc)
    top = sorted(peaks.tolist(), key=lambda p: (-float(cc[p]), p))[:top_n]
    for k, p in enumerate(top):
        pl[k], pv[k] = p - (len(a) - 1), cc[p] * cc[p]
    return lag, pl, pv, len(top)


def _pattern(m, kind, at):
    """An integer sequence of length m (>= 64) whose features start at index `at`."""
    d = np.zeros(m, i64)
    w = d[at:at + 64]
    if kind == "constant":
        d[:] = 5
    elif kind == "plateaus":  # widths 3, 4 and 2: peaks at (p + q - 1) // 2 = at + 3, at + 11, at + 20
        w[2:5], w[10:14], w[20:22] = 7, 7, 9
    elif kind == "ends":  # plateaus touching both ends are no peaks; the only peak is w[30]
        d[:3], d[-3:], w[30] = 8, 8, 2
    elif kind == "peaks16":  # exactly 16 peaks, values 1..16
        w[1:49:3] = np.arange(1, 17)
    elif kind == "peaks20":  # 20 peaks of three values: the top 16 are cut inside a run of equal values
        w[1:61:3] = np.tile((3, 9, 6), 7)[:20]
    elif kind == "negative":  # every value negative, peaks -3, -5, -3
        d[:] = -90
        w[5], w[9], w[13] = -3, -5, -3
    elif kind == "max_first":
        d[0], w[10], w[20] = 100, 4, 4
    elif kind == "max_last":
        d[-1], w[10], w[20] = 100, 4, 4
    else:
        raise ValueError(kind)
    return d


PATTERNS = ("constant", "plateaus", "ends", "peaks16", "peaks20", "negative", "max_first", "max_last")
# the peaks of each pattern, relative to `at`
PATTERN_PEAKS = {"constant": [], "plateaus": [3, 11, 20], "ends": [30], "peaks16": list(range(1, 49, 3)),
                 "peaks20": list(range(1, 61, 3)), "negative": [5, 9, 13], "max_first": [10, 20],
                 "max_last": [10, 20]}


def pattern_rows(m, at):
    """(name, a, b) per pattern: b is the single sample 64 / 256, so the correlation is a / 4 exactly; and the
    mirrored pair (a single sample, b reversed) with the same correlation."""
    out = []
    for kind in PATTERNS:
        d = _pattern(m, kind, at).astype(f32) * f32(UNIT)
        out.append((f"{kind}_{m}", d, np.array([0.25], f32)))
        out.append((f"{kind}_{m}_mirrored", np.array([0.25], f32), d[::-1].copy()))
    return out


@functools.lru_cache(None)
def find_table(La, Lb):
    """Rows of one launch with buffers [R, La] and [R, Lb]: (name, a, b, len_a, len_b) with a, b the samples the
    kernel may read (len clipped to the buffer) and len_a / len_b the per-row lengths passed, which may be 0 or
    exceed the buffer."""
    rng = np.random.default_rng(La * 8191 + Lb)
    rnd = lambda n, lo=-127, hi=127: rng.integers(lo, hi + 1, n).astype(f32) * f32(UNIT)
    rows = [("random_full", rnd(La), rnd(Lb)), ("ternary_full", rnd(La, -1, 1), rnd(Lb, -1, 1)),
            ("coarse_full", rnd(La, -3, 3), rnd(Lb, -2, 2))]
    if La > 2 and Lb > 2:
        rows.append(("random_short", rnd(La - 1), rnd(Lb // 2)))
    for m, at in ((64, 0), (256, 192), (257, 193), (512, 226), (4096, 3810)):
        for name, a, b in pattern_rows(m, at):
            if len(a) <= La and len(b) <= Lb:
                rows.append((name, a, b))
    const = np.full(max(La, Lb), 5 * UNIT, f32)
    rows.append(("constant_rows", const[:La], const[:1]))
    n = min(La, 40)
    nan_a, inf_a, inf_b = rnd(n), rnd(n), rnd(min(Lb, 7))
    nan_a[n // 2] = np.nan
    inf_a[n // 3] = np.inf
    inf_b[0] = 0.0  # inf * 0: a NaN where it meets the zero
    rows += [("nan_sample", nan_a, rnd(min(Lb, 5))), ("inf_sample", inf_a, np.abs(rnd(min(Lb, 5))) + f32(UNIT)),
             ("inf_times_zero", inf_a, inf_b)]
    out = [(name, a, b, len(a), len(b)) for name, a, b in rows]
    out += [("len_a_zero", rnd(La), rnd(Lb), 0, Lb), ("len_b_zero", rnd(La), rnd(Lb), La, 0),
            ("len_a_above", rnd(La), rnd(Lb), La + 1, Lb), ("len_b_above", rnd(La), rnd(Lb), La, Lb + 1),
            ("len_negative", rnd(La), rnd(Lb), -3, Lb)]
    return out


def find_row_inputs(row, La, Lb):
    """The (a, b) the reference sees: empty when a length is outside 1..buffer."""
    _, a, b, la, lb = row
    if la < 1 or lb < 1 or la > La or lb > Lb:
        return a[:0], b[:0]
    return a[:la], b[:lb]


@functools.lru_cache(None)
def find_expected(La, Lb, top_n):
    return [find_ref(*find_row_inputs(row, La, Lb), top_n) for row in find_table(La, Lb)]


# ---- 6. ofp_vote_index: k_vote_index ------------------------------------------------------------------------------

def vote_index_ref(m, vmin, nb):
    """starts int32 [nb + 1] (cumulative counts), the cells in stable order of their bucket, and `bad`: 1 when a
    cell that is not NaN holds a non-integer or a value outside [vmin, vmin + nb); such cells are left out."""
    v = m.astype(f64).reshape(-1) - vmin
    with np.errstate(invalid="ignore"):
        valid = ~np.isnan(v) & (v == np.rint(v)) & (v >= 0) & (v < nb)
    bad = int((~np.isnan(v) & ~valid).any())
    idx = np.flatnonzero(valid)
    b = v[idx].astype(i64)
    starts = np.concatenate([[0], np.cumsum(np.bincount(b, minlength=nb))]).astype(i32)
    return starts, idx[np.argsort(b, kind="stable")].astype(i32), bad


# (cells, n_buckets, n_maps, kind)
INDEX_CASES = ((1, 1, 1, "one"), (63, 1, 3, "one"), (64, 1, 1, "one"), (64, 256, 1, "distinct"),
               (65, 255, 3, "random"), (81, 256, 3, "random"), (81, 257, 128, "random"), (65, 32768, 1, "distinct"),
               (64, 32768, 3, "ends"), (1 << 20, 32768, 1, "random"), (1 << 20, 1, 1, "one"),
               (1 << 20, 257, 3, "random"))
INDEX_REFUSED = ((4, 16, 129), ((1 << 20) + 1, 16, 1), (4, 32769, 1))  # (cells, n_buckets, n_maps)


@functools.lru_cache(None)
def index_table(cells, nb, n_maps, kind):
    """pool float32 [n_maps + 1, cells], map_ids int32 [n_maps] (not the identity), vmin int32 [n_maps] (negative),
    and which maps hold a bad value."""
    rng = np.random.default_rng(cells % 9973 + 31 * nb + n_maps)
    ids = rng.permutation(n_maps + 1)[:n_maps].astype(i32)
    vmin = -rng.integers(1, 400, n_maps).astype(i32)
    pool = np.full((n_maps + 1, cells), 1e9, f32)  # the unused map is never read
    bad = np.zeros(n_maps, i32)
    for k in range(n_maps):
        if kind == "one":  # every cell of a wave step in the same bucket
            b = np.full(cells, int(rng.integers(0, nb)))
        elif kind == "distinct":
            b = rng.permutation(nb)[:cells]
            if nb > cells + 2:  # the first and the last bucket are among them
                b = 1 + rng.permutation(nb - 2)[:cells]
                b[0], b[-1] = nb - 1, 0
        elif kind == "ends":
            b = rng.choice([0, nb - 1], cells)
        else:
            b = rng.integers(0, nb, cells)
        m = (b + int(vmin[k])).astype(f32)
        if cells > 8 and kind not in ("one", "distinct"):
            m[rng.choice(cells, max(1, cells // 9), replace=False)] = np.nan
        if n_maps > 1 and cells > 8 and k % 3 == 1:  # a non-integer and two out-of-range values: left out, bad = 1
            where = rng.choice(cells, 3, replace=False)
            m[where] = (m[where[0]] + 0.5 if not np.isnan(m[where[0]]) else 0.5, float(vmin[k]) - 1.0,
                        float(vmin[k]) + nb)
            bad[k] = 1
        pool[ids[k]] = m
    return pool, ids, vmin, bad


# ---- 7. ofp_paired_windows, ofp_paired_vote (k_vote_grid), ofp_paired_solve ----------------------------------------

# (sensor_locations, drum_diameter, scale, sr): side 5, 9, 17; S = 2, 3, 5; the last with more than 256 buckets
PAIRED_MODELS = (([[0.8, 45], [0.85, 225]], 4, 1, 44100),
                 ([[0.95, 20], [0.9, 140], [1.0, 260]], 8, 1, 48000),
                 ([[0.9, 0], [0.95, 72], [0.9, 144], [1.0, 216], [0.9, 288]], 16, 1, 192000))
PAIRED_TOLS = (0, 0.5, 1, 2, 2.5)


class Paired:
    """The tables MultilateratePaired(locations, drum_diameter=d, scale=scale, sr=sr) builds, from its docstring."""

    def __init__(self, locations, d, scale, sr):
        self.S, self.sr, self.scale = len(locations), sr, scale
        self.radius = int(np.round(d * scale / 2, 1))
        self.sensors = sensors3([polar_to_cartesian(x[0] * self.radius, x[1]) for x in locations])
        self.c = speed_of_sound(100 * scale, medium="drumhead")
        self.r, mask_r2 = grid_2d(d, scale, 1)
        self.side = 2 * self.r + 1
        self.maps, mn, mx = lag_maps_ref(self.sensors, self.r, self.c, sr, mask_r2)
        S = self.S
        self.neighbours = [((i - 1) % S, (i + 1) % S) for i in range(S)]
        self.ids = np.array([j * S + i for i in range(S) for j in self.neighbours[i]], i32)
        mn, mx = mn.reshape(-1)[self.ids], mx.reshape(-1)[self.ids]
        empty = np.isnan(mn)
        self.vmin = np.where(empty, 0, mn).astype(i64)
        self.n_buckets = int((np.where(empty, 0, mx).astype(i64) - self.vmin).max()) + 1

    def slot_map(self, slot):
        return self.maps.reshape(self.S * self.S, -1)[self.ids[slot]]


@functools.lru_cache(None)
def paired(k):
    return Paired(*PAIRED_MODELS[k])


def vote_ref(slot_maps, S, first, lags, tol):
    """(res float32 [cells], cell): res = sum_k (map_k > lag_k - tol) & (map_k < lag_k + tol) over the hit's one
    (S == 2) or two neighbour maps, cell = np.argmax(res)."""
    res = np.zeros(slot_maps[0].size, f32)
    for k in range(2 if S > 2 else 1):
        m = slot_maps[2 * first + k].astype(f64).reshape(-1)
        with np.errstate(invalid="ignore"):
            res += ((m > float(lags[k]) - tol) & (m < float(lags[k]) + tol)).astype(f32)
    return res, int(np.argmax(res))


def cell_xy(cell, side):
    half = (side - 1) / 2.0
    return float(cell % side) - half, half - float(cell // side)


def vote_kind(slot_maps, S, first, lags, tol):
    """Which branch of the vote a hit takes: 'both_empty', 'one_empty', 'disjoint' or 'overlap' ('single' for S == 2
    with a non-empty run)."""
    runs = []
    for k in range(2 if S > 2 else 1):
        m = slot_maps[2 * first + k].astype(f64).reshape(-1)
        with np.errstate(invalid="ignore"):
            runs.append((m > float(lags[k]) - tol) & (m < float(lags[k]) + tol))
    if not any(r.any() for r in runs):
        return "both_empty"
    if len(runs) == 1:
        return "single"
    if not all(r.any() for r in runs):
        return "one_empty"
    return "overlap" if (runs[0] & runs[1]).any() else "disjoint"


def vote_hits(slot_maps, S, seed):
    """first int32 [B], lags int32 [B, 2]: lags of real cells (overlap), of two different cells, at and beyond the
    extremes of the maps and at the ends of int32 (the clamps)."""
    rng = np.random.default_rng(seed)
    first, lags = [], []
    for i in range(S):
        m0, m1 = slot_maps[2 * i].reshape(-1), slot_maps[2 * i + 1].reshape(-1)
        both = np.flatnonzero(~np.isnan(m0) & ~np.isnan(m1))
        lo0, hi0, lo1, hi1 = (int(v) for v in (np.nanmin(m0), np.nanmax(m0), np.nanmin(m1), np.nanmax(m1)))
        picks = [(int(m0[c]), int(m1[c])) for c in rng.choice(both, min(len(both), 4), replace=False)]
        c, e = rng.choice(both, 2, replace=False) if len(both) > 1 else (both[0], both[0])
        picks += [(int(m0[c]), int(m1[e])), (int(m0[e]), int(m1[c])),  # often no common cell
                  (lo0, hi1), (hi0, lo1), (lo0, lo1), (hi0, hi1),
                  (lo0 - 1, lo1 - 1), (hi0 + 1, hi1 + 1), (lo0 - 3, int(m1[c])), (int(m0[c]), hi1 + 3),
                  (lo0 - 10 ** 6, hi1 + 10 ** 6), (2 ** 31 - 1, INT_MIN), (INT_MIN, int(m1[e])), (0, 0)]
        first += [i] * len(picks)
        lags += picks
    return np.array(first, i32), np.array(lags, i64).astype(i32)


def synthetic_maps(side, S, seed=3):
    """slot maps float32 [2 S, side * side] of integers in [-300, 300] with NaN cells, as smooth ramps so that runs
    of equal lag are long; vmin and n_buckets as MultilateratePaired forms them."""
    rng = np.random.default_rng(seed)
    g = np.arange(side, dtype=f64)
    maps = []
    for k in range(2 * S):
        a, b = rng.uniform(-0.28, 0.28, 2)
        m = np.rint(a * (g[None, :] - side / 2) + b * (g[:, None] - side / 2)).astype(f32)
        m[(g[None, :] - side / 2) ** 2 + (g[:, None] - side / 2) ** 2 > (side / 2) ** 2] = np.nan
        maps.append(m.reshape(-1))
    maps = np.stack(maps)
    vmin = np.nanmin(maps, 1).astype(i64)
    return maps, vmin, int((np.nanmax(maps, 1).astype(i64) - vmin).max()) + 1


def windows_ref(n_clips, N, C, S, left, right, onset=None, first=None, clip=None, groups=None, n_groups=None):
    """a_off, b_off int64 [B, 2], len int32 [B, 2], first int32 [B], status int32 [B] of ofp_paired_windows: the
    window x[clip, onset - left : min(onset + right, N)] of the first channel against its neighbours
    (first - 1) % S and (first + 1) % S, as element offsets into x [n_clips, N, C]; zeros under a status."""
    if groups is not None:
        cap = groups.shape[1]
        B = n_clips * cap
        flat = groups.reshape(B, C)
    else:
        B = len(onset)
    a_off, b_off = np.zeros((B, 2), i64), np.zeros((B, 2), i64)
    ln, first_out, status = np.zeros((B, 2), i32), np.zeros(B, i32), np.zeros(B, i32)
    for h in range(B):
        st, f, on, cl = PAIRED_OK, -1, 0, 0
        if groups is not None:
            cl = h // cap
            if n_groups is not None and h % cap >= min(int(n_groups[cl]), cap):
                st = PAIRED_UNUSED
            else:
                present = [(int(v), k) for k, v in enumerate(flat[h]) if v >= 0]
                if not present:
                    st = PAIRED_NO_CHANNEL
                else:
                    on, f = min(present)
                    if f >= S:
                        st = PAIRED_BAD_HIT
        else:
            on, f, cl = int(onset[h]), int(first[h]), int(clip[h]) if clip is not None else 0
            if f < 0 or f >= S or cl < 0 or cl >= n_clips:
                st = PAIRED_BAD_HIT
        if st == PAIRED_OK:
            start = on - left
            n = min(on + right, N) - start
            if start < 0:
                st = PAIRED_NEG_WINDOW
            elif n < 1:
                st = PAIRED_EMPTY_WINDOW
        first_out[h], status[h] = f, st
        if st == PAIRED_OK:
            base = (cl * N + start) * C
            a_off[h] = base + f
            b_off[h] = (base + (f + S - 1) % S, base + (f + 1) % S)
            ln[h] = n
    return a_off, b_off, ln, first_out, status


def window_hits(N, S, left, right):
    """onset, first, clip for two clips: windows inside, starting below 0, clipped at N, empty, and hits with
    `first` or `clip` out of range."""
    onset = [left, left - 1, 0, N - right, N - right + 1, N - 1, N + left - 1, N + left, N + left + 5, 50, 50, 50, 50,
             N // 2]
    first = [0, 1, S - 1, 0, 1, S - 1, 0, 1, 0, -1, S, 0, 1, S - 1]
    clip = [0, 1, 0, 1, 0, 1, 0, 1, 0, 0, 1, -1, 2, 1]
    return np.array(onset, i64), np.array(first, i32), np.array(clip, i32)


def window_groups(N, C, S, left, right, cap=5):
    """groups int64 [3, cap, C] and n_groups [3] = (0, 3, cap + 2): ties, absent channels, all absent, the earliest
    channel without a sensor (C > S), windows below 0 and past N."""
    rng = np.random.default_rng(N + C)
    g = rng.integers(left, N - right, (3, cap, C)).astype(i64)
    g[2, 0, :] = g[2, 0, 0]                      # all channels tie: channel 0
    g[2, 1, 1:3] = g[2, 1].min() - 1             # two tie for earliest: channel 1
    g[2, 1, 0] = -1                              # absent
    g[2, 2, :] = -1                              # no channel
    g[2, 3, :] = N
    g[2, 3, C - 1] = 40 + left                   # earliest is the last channel: no sensor when C > S
    g[2, 4, :] = (-1,) * (C - 1) + (left - 1,)   # window below 0 (or a channel without a sensor)
    g[1, 0, :] = N + left + 3                    # empty after clipping
    g[1, 1, :] = N - 1                           # clipped at N
    g[1, 2, :] = (left - 1,) + (-1,) * (C - 1)   # window below 0 on channel 0
    return g, np.array([0, 3, cap + 2], i64)


def paired_guess(p, lags, first):
    """MultilateratePaired.locate's geometry (origin, a, b), deltas and weighted guess for every row with a valid
    `first`: geom [B, 9], delta [B, 2], guess [B, 2]."""
    B = len(first)
    geom, delta, guess = np.zeros((B, 9)), np.zeros((B, 2)), np.zeros((B, 2))
    for g in range(B):
        i = int(first[g])
        if not 0 <= i < p.S:
            continue
        sa, sb, so = p.sensors[(i - 1) % p.S], p.sensors[(i + 1) % p.S], p.sensors[i]
        da, db = float(lags[g, 0]) * p.c / p.sr, float(lags[g, 1]) * p.c / p.sr
        wa, wb, wo = abs(da) / p.radius, abs(db) / p.radius, abs(da + db) / (2 * p.radius)
        geom[g] = np.concatenate([so, sa, sb])
        delta[g] = (da, db)
        guess[g] = (sa[0] * wa + sb[0] * wb + so[0] * wo, sa[1] * wa + sb[1] * wb + so[1] * wo)
    return geom, delta, guess


def solve_rows(p, B, seed=11):
    """lags int32 [B, 2] within the model's range and first int32 [B]; the last row of a batch past one wave has
    `first` out of range."""
    rng = np.random.default_rng(seed + B)
    span = max(2, int(0.6 * p.radius * p.sr / p.c))
    lags = rng.integers(-span, span + 1, (B, 2)).astype(i32)
    first = rng.integers(0, p.S, B).astype(i32)
    if B > WAVE:
        first[-1] = p.S
    return lags, first


# ---- 8. ofp_intensity_maps: k_intensity -------------------------------------------------------------------------

INTENSITY_CASES = ((0, [0.0, 0.0, 3.0], [2.5, -1.0, 0.5], 0.3), (7, [3.0, -2.0, 6.0], [-9.5, 8.0, 10.0], 0.5),
                   (8, [0.0, 17.0, 3.0], [15.0, 0.25, 20.0], 0.9), (8, [-4.0, 4.0, 1.0], [30.0, 30.0, 0.75], 0.0))


def intensity_ref(mics, r, refl):
    """fp64 [2, side, side]: 10 log10((1 + refl (1 - |cos theta|)) / dist) at every cell p = (col - r, row - r, 0),
    dist = |mic - p| and theta = arccos(z / dist) the angle to the surface normal."""
    g = np.arange(-r, r + 1, dtype=f64)
    out = []
    for mic in np.asarray(mics, f64):
        x, y, z = mic[0] - g[None, :], mic[1] - g[:, None], mic[2] - 0.0
        dist = np.sqrt(x * x + y * y + z * z)
        theta = np.arccos(z / dist)
        out.append(10.0 * np.log10(1.0 * (1.0 + refl * (1.0 - np.abs(np.cos(theta)))) / dist))
    return np.stack(out)
