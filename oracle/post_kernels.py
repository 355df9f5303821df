"""Case tables, fp64 references and bounds for the kernels of csrc/ofp_xcorr.hip and csrc/ofp_post.hip, one by
one -- TEST INFRASTRUCTURE ONLY.  tests/test_gpu_post_kernels.py runs the kernels on these tables;
tests/test_post_kernels_cpu.py shows that the references, bounds and margins are sound.  Nothing here calls the code
under test or torch.

The integer kernels (ofp_xcorr_lag, ofp_adjust_onset, ofp_fix_onsets, ofp_onset_region) and ofp_filter_direction are
compared for equality; ofp_xcorr_lag's correlation values bit for bit (the canon of oracle/ofp_oracle.c).  Two
kernels round differently from their references and get a bound per output element:

ofp_xcorr_full.  out[i][j] = (1 / mean_k) sum_m sum_t a[m][t + j - (L-1)] b[m][t].  The kernel runs, per row m, a
chain of `terms` fp32 fma steps (terms = L - |j - (L-1)|, the overlap of that lag), adds the mean_k row sums in fp32
and divides once.  Every product therefore passes through at most terms + mean_k + 1 roundings (terms fma steps,
mean_k additions, one division), each of relative size U = 2**-24, so to first order
    |out - ref| <= (terms + mean_k + 2) * U * (sum_m sum_t |a b|) / mean_k,
the +1 over the count covering the second-order terms ((1+U)**n - 1 <= n U (1 + n U), n U < 1e-3 here).  Inputs that
are small integers make every step exact; the bound is not used there, equality is demanded.

ofp_resample_windows.  y[m] = (1/Nx) (Y[0] + sum_{k=1..K} c_k Re(Y[k] e^{2 pi i k m / num})), Y[k] = sum_n x[n]
e^{-2 pi i k n / Nx}, c_k = 2 except at the Nyquist bins, K = min(Nx, num) // 2: a double sum of (2K + 1) Nx
elementary terms x[n] * twiddle * twiddle * c_k / Nx.  Kernel and reference both evaluate it in fp64 (u = 2**-53);
an elementary term passes through at most Nx additions of the forward sum, K additions of the synthesis and a
handful of further roundings (two twiddles, their products, c_k, the scale: 8 is generous), and the moduli of the
elementary terms add up to at most (2K + 1) / Nx * sum|x|.  Each side is thus within
(Nx + K + 8) u max(1, (2K + 1) / Nx) sum|x| of the exact value to first order, the two together within twice that:
    |fp64 kernel value - fp64 reference| <= (Nx + K + 8) * 2**-52 * max(1, (2K + 1) / Nx) * sum|x|.
The kernel then rounds once to fp32: U * |ref| more (plus U times the fp64 term, which the 8 swallows).  The
reference reduces k n modulo Nx before it forms the phase, as the kernel does, so its twiddles are within a few u.
Denormal outputs do not occur at the tables' magnitudes.

adjust_onset decides by `da > db`, two fp64 sums that kernel and numpy add in different orders.  A decision is
comparable when both sums have at most one term (then both sides are exact and an exact tie is legitimate) or when
the margin |da - db| / (A + B) is at least MARGIN = 1e-9, A and B being the sums of the absolute terms over the
maxima: sums of at most 5000 fp64 terms differ by at most about 5000 * 2**-53 = 6e-13 of A (resp. B) between any
two orders, three orders below MARGIN.  For non-negative terms A + B = |da| + |db|.  Sums whose terms are all
exactly zero are exact in any order and count as exact.  A table may lose at most LEAVE_OUT_CAP = 1 % of its cases
to this rule.
"""
import numpy as np
from scipy.ndimage import median_filter

from . import xcorr as X
from .spectral import fourier_resample

f32, f64 = np.float32, np.float64
U = 2.0 ** -24
MARGIN = 1e-9
LEAVE_OUT_CAP = 0.01
XT, XW = 256, 64  # workgroup and wave of the kernels (tile seams, tie positions)
X_MAXN = 4096


def ratio(err, bound):
    """err / bound per element; NaN or an error above a bound of 0 is inf."""
    err, bound = np.asarray(err, f64), np.asarray(bound, f64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(np.isnan(err) | ((bound == 0) & (err > 0)), np.inf, np.where(bound > 0, err / bound, 0.0))


def too_many_left_out(left_out, total):
    return left_out > LEAVE_OUT_CAP * total


# ---- 1. ofp_xcorr_lag ---------------------------------------------------------------------------------------------

LAG_D = (0, 1, 2, 3, 4)
LAG_ABS = (0, 1)


def lag_n_in(d):
    return (d + 1, d + 2, 255, 256, 257, 258, 513, 4096)


def lag_cutoffs(n):
    return (0, 1, 10, n, 2 * n)


def lag_windows(n):
    """(lo, hi) per pair of one launch: whole, lo < 0, hi past the end, empty (lo > hi, lo == hi, lo past the end),
    width 1 at the first and the last lag, width 257 around the zero lag."""
    T = 2 * n - 1
    k = max(0, n - 129)
    return [(0, T), (-5, min(T, 300)), (max(0, T - 300), T + 7), (5, 3), (4, 4), (T + 3, T + 9), (0, 1), (T - 1, T),
            (k, k + 257)]


def clamp_window(lo, hi, n, cc_stride=None):
    """The window ofp_xcorr_lag searches: [lo, hi) clamped to [0, 2n-1), and to cc_stride values when they are kept."""
    T = 2 * n - 1
    lo = max(0, min(lo, T))
    hi = max(lo, min(hi, T))
    if cc_stride is not None:
        hi = min(hi, lo + cc_stride)
    return lo, hi


def lag_inputs(seed, n_pairs, n_in):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n_pairs, n_in)).astype(f32), rng.standard_normal((n_pairs, n_in)).astype(f32)


def lag_ref(x, y, d, take_abs, cutoff, lo, hi, cc_stride=None):
    """One pair -> (argmax or -1, cc values of the clamped window as float32)."""
    x, y = np.diff(np.asarray(x, f32), d), np.diff(np.asarray(y, f32), d)
    if take_abs:
        x, y = np.abs(x), np.abs(y)
    lo, hi = clamp_window(lo, hi, len(x), cc_stride)
    cc = X.xcorr_slice(x, y, cutoff, lo, hi)
    return (int(np.argmax(cc)) if len(cc) else -1), cc


LAG_STRIDE_CASE = dict(n_in=600, d=1, cutoff=10, strides=(1, 100, 256, 257))

TIE_N = 1024


def tie_cases():
    """Exact ties: y is one impulse at sample 0, x has impulses of one height at `pos`, so that with the whole
    window the normalised correlation is that height (over the constant count, cutoff >= n) at lags
    pos + n - 1 and 0 elsewhere.  `first` is the expected argmax.  Thread of lag j: j % 256; wave: that // 64."""
    n = TIE_N
    base = n - 1
    cases = []

    def add(name, pos):
        cases.append(dict(name=name, n=n, pos=tuple(pos), first=base + min(pos)))
    add("same thread", (10, 10 + 256, 10 + 512))
    add("same thread, later first in memory", (522, 10 + 256))
    add("lanes of one wave, lower lane first", (2, 40))              # lags 1025, 1063: threads 1, 39
    add("lanes of one wave, higher lane first", (51, 51 + 256 - 20))  # threads 50 and 30
    add("different waves, lower wave first", (2, 2 + 70, 2 + 140, 2 + 200))
    add("different waves, higher wave first", (201, 201 + 100))      # threads 200 (wave 3) and 44 (wave 0)
    add("all four waves and a later pass", (250, 250 + 64 + 256, 250 + 128, 250 + 192 + 512))
    return cases


def tie_inputs(case, sign=1.0):
    n = case["n"]
    x, y = np.zeros(n, f32), np.zeros(n, f32)
    x[list(case["pos"])] = 2.0 * sign
    y[0] = 3.0
    return x, y


# ---- 2. ofp_xcorr_full --------------------------------------------------------------------------------------------

FULL_L = (1, 2, 128, 129, 255, 256, 257, 4096)
FULL_MEAN_K = (1, 2, 5)
FULL_ROWS = (1, 3)
FULL_PAD_A, FULL_PAD_B = 3, 7  # a_stride = L + 3, b_stride = L + 7


def full_inputs(seed, rows, L):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((rows, L)).astype(f32), rng.standard_normal((rows, L)).astype(f32)


def full_exact_inputs(seed, rows, L):
    rng = np.random.default_rng(seed)
    return rng.integers(-3, 4, (rows, L)).astype(f32), rng.integers(-3, 4, (rows, L)).astype(f32)


def full_ref(a, b, mean_k):
    """a, b [rows, L] -> (ref [rows / mean_k, 2L-1] fp64, bound): see the module docstring."""
    a, b = np.asarray(a, f64), np.asarray(b, f64)
    rows, L = a.shape
    assert rows % mean_k == 0
    out = np.zeros((rows // mean_k, 2 * L - 1))
    mag = np.zeros_like(out)
    for r in range(rows):
        out[r // mean_k] += np.correlate(a[r], b[r], "full")  # [j] = sum_t a[t + j - (L-1)] b[t]
        mag[r // mean_k] += np.correlate(np.abs(a[r]), np.abs(b[r]), "full")
    terms = L - np.abs(np.arange(2 * L - 1) - (L - 1))
    return out / mean_k, (terms + mean_k + 2) * U * mag / mean_k


def full_emulate(a, b, mean_k, drop=None):
    """The kernel's arithmetic in numpy: per lag an fp32 fma chain over ascending t, fp32 sum over the rows, one
    fp32 division.  (fma(p, q, acc) = the fp64 value p q + acc rounded to fp32; the double rounding of that fp64
    sum is 2**-29 of U.)  `drop` = (row, lag index, t): leave one product out."""
    a, b = np.asarray(a, f32), np.asarray(b, f32)
    rows, L = a.shape
    nl = 2 * L - 1
    out = np.zeros((rows // mean_k, nl), f32)
    for r in range(rows):
        acc = np.zeros(nl, f32)
        for t in range(L):  # b[t] meets a[0..L) at the lags j = L-1-t .. 2L-2-t
            j0 = L - 1 - t
            new = (a[r].astype(f64) * f64(b[r, t]) + acc[j0:j0 + L].astype(f64)).astype(f32)
            if drop is not None and drop[0] == r and drop[2] == t:
                new[drop[1] - j0] = acc[drop[1]]
            acc[j0:j0 + L] = new
        out[r // mean_k] = out[r // mean_k] + acc
    return out / f32(mean_k) if mean_k > 1 else out


# ---- 3. ofp_adjust_onset ------------------------------------------------------------------------------------------

ADJUST_N = (1, 2, 63, 64, 65, 400, 5000)
ADJUST_BRANCHES = ("o0 + lag_diff < 0", "o1 - lag_diff > n", "lag_diff = 0", "|lag_diff| = 1",
                   "segment longer than a wave",
                   "da > db", "da <= db", "o0 + lag_diff = -1, da > db", "o0 + lag_diff = 0, da > db",
                   "o0 + lag_diff = 1, da > db")


def adjust_detail(onsets, x, y, new_lag):
    """oracle.adjust_onset with its working shown: -> dict(moves, margin, exact, Lx, Ly, lag_diff, branches)."""
    oa, ob = int(onsets[0]), int(onsets[1])
    lag_diff = (ob - oa) - int(new_lag)
    w = np.exp(np.linspace(0, -np.e, abs(lag_diff)))
    n = len(x)
    if lag_diff < 0:
        x_start, x_end = max(oa + lag_diff, 0), min(oa, n)
        y_start, y_end = min(ob, n), min(ob - lag_diff, n)
    else:
        x_start, x_end = oa, min(oa + lag_diff, n)
        y_start, y_end = max(ob - lag_diff, 0), min(ob, n)
    Lx, Ly = max(x_end - x_start, 0), max(y_end - y_start, 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        ta = x[x_start:x_end] * w[len(w) - Lx:] if Lx else np.zeros(0)
        tb = y[y_start:y_end] * w[len(w) - Ly:][::-1] if Ly else np.zeros(0)
        da = np.sum(ta) / x.max() if Lx else 0.0
        db = np.sum(tb) / y.max() if Ly else 0
        A = np.sum(np.abs(ta)) / abs(f64(x.max())) if Lx else 0.0
        B = np.sum(np.abs(tb)) / abs(f64(y.max())) if Ly else 0.0
    if da > db:
        moves = (0, -lag_diff) if oa + lag_diff < 0 else (lag_diff, 0)
    else:
        moves = (0, -lag_diff)
    exact = (Lx <= 1 and Ly <= 1) or (not np.any(ta) and not np.any(tb))
    if not (np.isfinite(da) and np.isfinite(db) and np.isfinite(A + B)):
        margin, exact = 0.0, False  # a maximum of 0: the reference divides by it, nothing to compare
    elif A + B == 0:
        margin = 0.0
    else:
        margin = float(abs(da - db) / (A + B))
    br = set()
    if oa + lag_diff < 0:
        br.add("o0 + lag_diff < 0")
    if ob - lag_diff > n:
        br.add("o1 - lag_diff > n")
    if lag_diff == 0:
        br.add("lag_diff = 0")
    if abs(lag_diff) == 1:
        br.add("|lag_diff| = 1")
    if max(Lx, Ly) > XW:
        br.add("segment longer than a wave")
    br.add("da > db" if da > db else "da <= db")
    if da > db and abs(oa + lag_diff) <= 1:
        br.add(f"o0 + lag_diff = {oa + lag_diff}, da > db")
    return dict(moves=moves, margin=margin, exact=bool(exact), Lx=Lx, Ly=Ly, lag_diff=lag_diff, branches=br)


def comparable(detail):
    return detail["exact"] or detail["margin"] >= MARGIN


def adjust_table(n):
    """-> x, y [P, n] float32 (|N(0,1)| + 0.01), onsets [P, 2] in [0, n], new_lag [P] in [-n, n].  n <= 2: every
    combination; else 200 pairs, the first ones with lag_diff 0, +-1, onsets at the ends
    and the anchor's new position at -1, 0 and 1 with da > db."""
    rng = np.random.default_rng(300 + n)
    if n <= 2:
        combos = [(a, b, l) for a in range(n + 1) for b in range(n + 1) for l in range(-n, n + 1)]
        onsets = np.array([(a, b) for a, b, _ in combos], np.int32)
        new_lag = np.array([l for _, _, l in combos], np.int32)
    else:
        P = 200
        onsets = rng.integers(0, n + 1, (P, 2)).astype(np.int32)
        new_lag = rng.integers(-n, n + 1, P).astype(np.int32)
        onsets[0], onsets[1], onsets[2], onsets[3] = (0, n), (n, 0), (0, 0), (n, n)
        cur = onsets[:, 1] - onsets[:, 0]
        for i, delta in enumerate((0, 1, -1, 0, 1, -1)):  # lag_diff = delta where the lag stays inside [-n, n]
            new_lag[4 + i] = np.clip(cur[4 + i] - delta, -n, n)
        new_lag[10], new_lag[11] = n, -n
        onsets[12], new_lag[12] = (n // 2, n // 2), n  # lag_diff = -n: o0 + lag_diff < 0, o1 - lag_diff > n
        onsets[13], new_lag[13] = (n // 2, n // 2), -n
        for i, delta in enumerate((-1, 0, 1)):  # o0 + lag_diff = -1, 0, 1 (rows 14..16; y made quiet below: da > db)
            onsets[14 + i], new_lag[14 + i] = (n // 4, n // 2), n // 2 - delta
    P = len(new_lag)
    x = (np.abs(rng.standard_normal((P, n))) + 0.01).astype(f32)
    y = (np.abs(rng.standard_normal((P, n))) + 0.01).astype(f32)
    if n > 2:
        y[14:17] = 0.01  # the segment of y, [n/2, n/2 + n/4 + 1), stays clear of the one loud sample
        y[14:17, n - 1] = 3.0
    return x, y, onsets, new_lag


# ---- 4. ofp_fix_onsets --------------------------------------------------------------------------------------------

DIRECTIONS = {None: 0, "up": 1, "down": 2}
FIX_DEFAULTS = dict(filter_size=5, d=0, onset_direction=None, take_abs=False, zero_left=False, normalization_cutoff=10,
                    onset_tolerance=30, shift_onsets=0)


def fix_group(audio, og, opt, max_section):
    """One onset group `og` (int64 [C], modified in place) of one clip -> (status, smallest margin, comparable).
    oracle.fix_onsets with the kernel's documented statuses: a group whose section leaves the clip or is longer than
    max_section is shifted only (status 1)."""
    o = {**FIX_DEFAULTS, **opt}
    look = o["normalization_cutoff"] + o["onset_tolerance"]
    og += o["shift_onsets"]
    idx = np.argsort(og, kind="stable")
    a, b = int(og[idx[0]]), int(og[idx[-1]])
    n_sec = b - a + 2 * look
    if not (a - look >= 0 and b + look <= len(audio) and n_sec <= max_section and n_sec - o["d"] >= 1):
        return 1, np.inf, True
    section = np.diff(median_filter(audio[a - look:b + look], o["filter_size"], axes=0), o["d"], axis=0)
    if o["onset_direction"] == "up":
        section[section < 0] = 0
    elif o["onset_direction"] == "down":
        section[section > 0] = 0
    if o["take_abs"]:
        section = np.abs(section)
    sog = og - (a - look)
    margin, ok = np.inf, True
    for i in idx[1:]:
        pair = [int(sog[idx[0]]), int(sog[i])]
        x, y = section[:, idx[0]], section[:, i]
        if o["zero_left"]:
            x[:pair[0]] = 0.0
            y[:pair[1]] = 0.0
        new_lag = X.cross_correlation_lag(x, y, pair, normalization_cutoff=o["normalization_cutoff"],
                                          onset_tolerance=o["onset_tolerance"])
        if new_lag is not None:
            det = adjust_detail(pair, x, y, new_lag)
            if not det["exact"]:
                margin = min(margin, det["margin"])
            ok = ok and comparable(det)
            ca, cb = det["moves"]
            og[idx[0]] += ca
            og[i] += cb
            sog[idx[0]] += ca
            sog[i] += cb
    return 0, margin, ok


def fix_ref(audio, onsets, opt, max_section=X_MAXN, n_groups=None):
    """audio [N, C] or [n_clips, N, C]; onsets [G, C] or [n_clips, cap, C]; n_groups [n_clips] or None ->
    (fixed onsets, status, comparable, smallest margin), the last three one per group (shaped like onsets without
    the channel axis); the margin is inf for a group without an inexact decision."""
    audio = np.asarray(audio, f32)
    out = np.array(onsets, np.int64)
    a3 = audio[None] if audio.ndim == 2 else audio
    o3 = out[None] if audio.ndim == 2 else out
    status = np.zeros(o3.shape[:2], np.int32)
    ok = np.ones(o3.shape[:2], bool)
    margin = np.full(o3.shape[:2], np.inf)
    for c in range(o3.shape[0]):
        for g in range(o3.shape[1]):
            if n_groups is not None and g >= n_groups[c]:
                status[c, g] = 2
                continue
            status[c, g], margin[c, g], ok[c, g] = fix_group(a3[c], o3[c, g], opt, max_section)
    if audio.ndim == 2:
        return out, status[0], ok[0], margin[0]
    return out, status, ok, margin


def fix_bulk_cases():
    """synth.sensor_hits inputs: (name, seed, C, n, hits, options)."""
    return [
        ("C1", 41, 1, 6000, 3, dict(filter_size=3)),
        ("C2 plain", 42, 2, 8000, 5, dict(filter_size=1)),
        ("C2 up abs shift-3", 43, 2, 8000, 5, dict(filter_size=3, d=1, onset_direction="up", take_abs=True,
                                                   shift_onsets=-3)),
        ("C64 down abs zero_left shift4", 44, 64, 6000, 3, dict(filter_size=3, d=2, onset_direction="down",
                                                                take_abs=True, zero_left=True, shift_onsets=4)),
        ("C64 f15 d3", 45, 64, 6000, 3, dict(filter_size=15, d=3, take_abs=True, zero_left=True)),
        ("C128 f15 d4", 46, 128, 6000, 3, dict(filter_size=15, d=4, onset_direction="up")),
    ]


def fix_noise(seed, n, C):
    """Noise with a decaying burst per channel every 700 samples, so that sections anywhere have structure."""
    rng = np.random.default_rng(seed)
    a = 0.05 * rng.standard_normal((n, C))
    t = np.arange(200)
    for c in range(C):
        for p in range(100 + 13 * c, n - 200, 700):
            a[p:p + 200, c] += np.exp(-t / 40.0) * np.sin(2 * np.pi * t / 19.0) * (0.5 + 0.5 * rng.random())
    return a.astype(f32)


SHORT_OPT = dict(filter_size=15, normalization_cutoff=0, onset_tolerance=1)


def fix_short_case():
    """Sections shorter than the filter: look = 1, equal onsets (n_sec 2) and adjacent ones (n_sec 3), C = 2 and 3."""
    audio = fix_noise(50, 400, 3)
    onsets = np.array([[100, 100, 100], [150, 151, 150], [201, 200, 201], [1, 1, 2], [398, 399, 399], [250, 250, 251]],
                      np.int64)
    return audio, onsets, SHORT_OPT


def fix_equal_case():
    """Equal onsets inside ordinary groups: stable argsort, current_lag 0."""
    audio = fix_noise(51, 3000, 4)
    onsets = np.array([[800, 800, 800, 800], [1500, 1510, 1500, 1510], [2230, 2200, 2230, 2200]], np.int64)
    return audio, onsets, dict(filter_size=3, d=1, take_abs=True)


def fix_capacity_cases():
    """(name, audio, onsets [2, 2], options, max_section, expected status): n_sec == max_section and one more."""
    audio = fix_noise(52, 4400, 2)
    out = []
    for name, ms in (("capacity 4096", 4096), ("caller max_section 500", 500)):
        spread = ms - 80  # look = 40
        onsets = np.array([[100, 100 + spread], [100 + spread + 1, 100]], np.int64)
        out.append((name, audio, onsets, dict(filter_size=3, take_abs=True), ms, (0, 1)))
    return out


def fix_edge_case():
    """Clip edges at equality (status 0) and one sample beyond (status 1); look = 40, N = 1000."""
    audio = fix_noise(53, 1000, 2)
    onsets = np.array([[40, 70], [39, 70], [930, 960], [930, 961], [40, 960]], np.int64)
    return audio, onsets, dict(filter_size=3, take_abs=True), (0, 1, 0, 1, 0)


def fix_batch_case():
    """[n_clips, cap, C] with an n_groups mask and a different mix per clip: ordinary groups, an edge group, a group
    with a missing channel (-1), rows not in use (status 2, left as they are)."""
    C, N, cap = 3, 3000, 4
    audio = np.stack([fix_noise(60 + c, N, C) for c in range(3)])
    onsets = np.full((3, cap, C), -7, np.int64)
    onsets[0, :3] = [[500, 520, 510], [1200, 1200, 1215], [30, 60, 50]]
    onsets[1, :1] = [[2100, 2080, 2090]]
    onsets[2, :4] = [[700, 705, 699], [1400, -1, 1410], [2950, 2959, 2940], [2100, 2130, 2110]]
    n_groups = np.array([3, 1, 4], np.int64)
    return audio, onsets, n_groups, dict(filter_size=5, d=1, take_abs=True, shift_onsets=0)


def median_at_rule(col, t, fs):
    """The kernel's window for sample t of a section column: scipy.ndimage 'reflect', applied until inside."""
    n = len(col)
    w = []
    for k in range(fs):
        u = t - fs // 2 + k
        while u < 0 or u >= n:
            u = -u - 1 if u < 0 else 2 * n - 1 - u
        w.append(col[u])
    return np.sort(np.array(w, f32))[fs // 2]


# ---- 5. ofp_onset_region ------------------------------------------------------------------------------------------

REGION_N = (0, 1, 2, 100, 4096)
REGION_MED = (1, 3, 33)
REGION_AUDIO_LEN = 6000


def region_audio():
    rng = np.random.default_rng(500)
    a = 0.02 * rng.standard_normal(REGION_AUDIO_LEN)
    t = np.arange(400)
    for p in (0, 700, 2500, 2540, 4100, REGION_AUDIO_LEN - 300):
        m = min(400, REGION_AUDIO_LEN - p)
        a[p:p + m] += (np.exp(-t / 90.0) * rng.standard_normal(400))[:m]
    return a.astype(f32)


def region_onsets(n):
    N, h = REGION_AUDIO_LEN, n // 2
    return np.array([0, 1, 10, h // 2, 700, 730, 2530, 4000, 4100, N - h // 2 - 1, N - 10, N - 1, N,
                     N + h - 1 if h else N + 1, N + h, N + h + 5], np.int64)


def region_ref(audio, onset, n, med, factor):
    """oracle.detect_onset_region; for an empty region (the reference raises) the kernel's documented answer, start."""
    start = max(int(onset) - n // 2, 0)
    end = min(int(onset) + n // 2, len(audio))
    if end - start <= 0:
        return start
    return X.detect_onset_region(audio, int(onset), n, med, factor)


def region_hand_cases():
    """(name, audio, onset, n, med, factor, expected).  Runs of 1.0 on a floor of 0.1, median size 1, threshold 0.5."""
    def sig(runs, length=100):
        a = np.full(length, 0.1, f32)
        for s, e in runs:
            a[s:e] = 1.0
        return a
    return [
        ("run of 4 removed, run of 5 kept", sig([(20, 24), (40, 45)]), 50, 100, 1, 0.5, 40),
        ("run of 5 at the first sample", sig([(0, 5), (60, 70)]), 50, 100, 1, 0.5, 0),
        ("run of 5 at the last sample", sig([(95, 100)]), 50, 100, 1, 0.5, 95),
        ("run of 5 at the last sample of an inner region", sig([(75, 80)], 200), 40, 80, 1, 0.5, 75),
        ("run of 5 at the first sample of an inner region", sig([(30, 35)], 200), 70, 80, 1, 0.5, 30),
        ("run of 4 at the last sample", sig([(96, 100)]), 50, 100, 1, 0.5, 0),
        ("nothing above threshold", sig([(20, 30)]), 50, 100, 1, 1.0, 0),
        ("nothing above threshold, factor 2, inner region", sig([(20, 30)], 300), 150, 100, 3, 2.0, 100),
        ("constant", np.full(100, 0.7, f32), 50, 100, 1, 0.5, 0),
        ("constant, median 33, inner region", np.full(300, 0.7, f32), 150, 100, 33, 0.5, 100),
    ]


# ---- 6. ofp_resample_windows --------------------------------------------------------------------------------------

RESAMPLE_PAIRS = ((1, 1), (1, 4), (2, 1), (2, 3), (3, 2), (4, 4), (255, 256), (256, 255), (256, 257), (257, 256),
                  (256, 256), (2048, 2048), (2048, 1000), (1001, 2048))
RESAMPLE_CLIP = 5000


def resample_audio(C):
    return np.random.default_rng(600 + C).standard_normal((RESAMPLE_CLIP, C)).astype(f32)


def resample_launches():
    """One launch per output length: dict(num, max_nx, nx [items], start [items]).  Every (Nx, num) pair appears
    inside the clip, once more starting before sample 0 and once running past the clip end."""
    launches = []
    for num in sorted({p[1] for p in RESAMPLE_PAIRS}):
        nxs = [p[0] for p in RESAMPLE_PAIRS if p[1] == num]
        nx, start = [], []
        for i, v in enumerate(nxs):
            nx += [v, v, v]
            start += [37 + 501 * i, -(v // 3) - 1, RESAMPLE_CLIP - v // 2]
        launches.append(dict(num=num, max_nx=min(2048, max(nxs) + 5), nx=np.array(nx, np.int32),
                             start=np.array(start, np.int64)))
    return launches


def resample_window(audio, start, nx, c):
    """audio [N, C] -> the nx samples from `start` of channel c; outside the clip 0."""
    t = np.arange(start, start + nx)
    inside = (t >= 0) & (t < audio.shape[0])
    w = np.zeros(nx, f32)
    w[inside] = audio[t[inside], c]
    return w


def resample_bound(x, num, ref):
    Nx = len(x)
    K = min(Nx, num) // 2
    sum_x = float(np.sum(np.abs(np.asarray(x, f64))))
    return U * np.abs(ref) + (Nx + K + 8) * 2.0 ** -52 * max(1.0, (2 * K + 1) / Nx) * sum_x


def resample_ref(x, num):
    """-> (oracle.spectral.fourier_resample in fp64, bound)."""
    ref = fourier_resample(x, num)
    return ref, resample_bound(x, num, ref)


def resample_emulate(x, num, fault=None):
    """The kernel's arithmetic in numpy: tabulated fp64 twiddles indexed by k n mod Nx and k m mod num, fp64 sums,
    one rounding to fp32.  fault: "nyquist scale" leaves the x2 / x0.5 of the shorter length's Nyquist bin out,
    "nyquist real" doubles the last bin of an even num like every other, "dropped term" leaves x[Nx // 2] out of
    bin 1 (bin 0 when there is no other)."""
    x = np.asarray(x, f32).astype(f64)
    Nx = len(x)
    N = min(num, Nx)
    K = N // 2
    twx = np.exp(-2j * np.pi * np.arange(Nx) / Nx)
    twy = np.exp(2j * np.pi * np.arange(num) / num)
    n = np.arange(Nx)
    Y = np.array([np.sum(x * twx[(k * n) % Nx]) for k in range(K + 1)])
    if fault == "dropped term":
        k = 1 if K >= 1 else 0
        Y[k] -= x[Nx // 2] * twx[(k * (Nx // 2)) % Nx]
    if N % 2 == 0 and fault != "nyquist scale":
        if num < Nx:
            Y[K] *= 2.0
        elif Nx < num:
            Y[K] *= 0.5
    m = np.arange(num)
    acc = np.full(num, Y[0].real)
    for k in range(1, K + 1):
        e = twy[(k * m) % num]
        if 2 * k == num and fault != "nyquist real":
            acc += Y[k].real * e.real
        else:
            acc += 2.0 * (Y[k].real * e.real - Y[k].imag * e.imag)
    return (acc * ((num / Nx) / num)).astype(f32)


# ---- 7. ofp_filter_direction --------------------------------------------------------------------------------------

FILTER_GRID_PASS = 4096 * 256  # elements one pass of the capped grid covers
FILTER_STRIDE_CASE = (149797, 7)  # n, C: 1 048 579 elements
FILTER_SMALL = ((1, 1), (1, 3), (2, 1), (257, 3), (1000, 1), (1000, 3))


def filter_input(seed, n, C):
    """Half the rows small integers (equal neighbours, difference exactly 0, both zeros' signs), half noise; row 0
    negative."""
    rng = np.random.default_rng(seed)
    q = rng.integers(-2, 3, (n, C)).astype(f32)
    q[q == 0] = np.where(rng.random(int((q == 0).sum())) < 0.5, f32(-0.0), f32(0.0))
    x = np.where(rng.random((n, 1)) < 0.5, q, rng.standard_normal((n, C)).astype(f32)).astype(f32)
    x[0] = -np.abs(x[0]) - 1.0
    return x


def filter_ref(x, direction):
    return X.filter_data(x, direction)
