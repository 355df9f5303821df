"""The references, bounds and margins of oracle/post_kernels.py are sound -- no GPU here.  For the bounded primitives
a numpy emulation of the kernel's arithmetic stays inside the bound and a planted fault leaves it by a wide factor;
for the integer primitives the hand-built cases give the intended answers under the oracle, the tables reach every
branch they claim to reach, and the margin rule leaves out no more than its cap.
"""
import warnings

import numpy as np
import pytest

import oracle
from oracle import post_kernels as K

f32, f64 = np.float32, np.float64
WIDE = 50.0  # a planted fault must exceed the bound by at least this factor somewhere


# ---- 1. ofp_xcorr_lag ---------------------------------------------------------------------------------------------

def test_lag_windows_hold_every_kind():
    for n in (1, 2, 255, 513, 4096):
        T = 2 * n - 1
        w = K.lag_windows(n)
        clamped = [K.clamp_window(lo, hi, n) for lo, hi in w]
        assert (0, T) in w and any(lo < 0 for lo, _ in w) and any(hi > T for _, hi in w)
        assert any(lo > hi for lo, hi in w) and any(lo == hi for lo, hi in w) and any(lo > T for lo, _ in w)
        assert (0, 1) in clamped and (T - 1, T) in clamped
        assert all(0 <= lo <= hi <= T for lo, hi in clamped)
        if n >= 129:
            assert any(hi - lo == K.XT + 1 for lo, hi in clamped)
    assert K.clamp_window(0, 1199, 600, 100) == (0, 100) and K.clamp_window(-3, 5000, 600) == (0, 1199)


def test_lag_ref_is_the_oracle_on_the_clamped_window():
    x, y = K.lag_inputs(1, 1, 300)
    am, cc = K.lag_ref(x[0], y[0], 2, 1, 10, -5, 2000)
    lag, cc2 = oracle.cross_correlation_lag(x[0], y[0], legal_lags=(-297, 298), d=2, take_abs=True, return_cc=True)
    assert np.array_equal(cc.view(np.uint32), cc2.view(np.uint32)) and lag == -(am - 298)
    assert K.lag_ref(x[0], y[0], 0, 0, 10, 5, 3) == (-1, pytest.approx(np.zeros(0)))
    am, cc = K.lag_ref(x[0], y[0], 0, 0, 10, 0, 599, cc_stride=100)
    assert len(cc) == 100 and am == int(np.argmax(cc))


def test_tie_cases_tie_where_intended():
    n = K.TIE_N
    T = 2 * n - 1
    kinds = set()
    for c in K.tie_cases():
        x, y = K.tie_inputs(c)
        for cutoff in (n, 2 * n):
            am, cc = K.lag_ref(x, y, 0, 0, cutoff, 0, T)
            lags = sorted(p + n - 1 for p in c["pos"])
            assert np.flatnonzero(cc == cc.max()).tolist() == lags and cc.max() == f32(6.0) / f32(cutoff)
            assert am == c["first"] == lags[0] and np.count_nonzero(cc) == len(lags)
        thread = [j % K.XT for j in lags]
        first_thread = thread[0]
        for t in thread[1:]:
            if t == first_thread:
                kinds.add("same thread")
            elif t // K.XW == first_thread // K.XW:
                kinds.add("lower lane first" if first_thread < t else "higher lane first")
            else:
                kinds.add("lower wave first" if first_thread // K.XW < t // K.XW else "higher wave first")
        x, y = K.tie_inputs(c, -1.0)
        assert K.lag_ref(x, y, 0, 0, n, 0, T)[0] == 0
    assert kinds == {"same thread", "lower lane first", "higher lane first", "lower wave first", "higher wave first"}
    assert K.lag_ref(np.zeros(n, f32), np.zeros(n, f32), 0, 0, n, 0, T)[0] == 0


# ---- 2. ofp_xcorr_full --------------------------------------------------------------------------------------------

def test_full_ref_is_the_stated_sum():
    a, b = K.full_inputs(3, 4, 5)
    ref, _ = K.full_ref(a, b, 2)
    for i in range(2):
        for j in range(9):
            want = sum(f64(a[m, t + j - 4]) * f64(b[m, t]) for m in (2 * i, 2 * i + 1) for t in range(5)
                       if 0 <= t + j - 4 < 5) / 2
            assert ref[i, j] == pytest.approx(want, rel=1e-14, abs=1e-300)


@pytest.mark.parametrize("length,mean_k,rows", [(1, 1, 1), (2, 5, 3), (129, 2, 3), (257, 5, 1), (4096, 1, 1)])
def test_full_emulation_is_inside_the_bound_and_faults_are_not(length, mean_k, rows):
    a, b = K.full_inputs(2000 + 10 * length + mean_k + rows, rows * mean_k, length)
    ref, bound = K.full_ref(a, b, mean_k)
    emu = K.full_emulate(a, b, mean_k).astype(f64)
    r = K.ratio(np.abs(emu - ref), bound)
    print(f"\nemulated ofp_xcorr_full L={length} mean_k={mean_k}: largest error / bound {r.max():.3g}", end="")
    assert r.max() <= 1.0
    if length >= 129:
        j = length - 1 + 7
        shifted = emu.copy()
        shifted[0, j] = emu[0, j + 1]  # one lag shifted by one
        assert K.ratio(np.abs(shifted - ref), bound).max() > WIDE
        # one dropped term, as an off-by-one in the overlap limits gives at every lag: judged at a lag of 64 terms
        # (at the 4096-term lags the worst-case bound is itself a few percent of one product)
        k = length - 64
        j = length - 1 + k
        t = int(np.argmax(np.abs(a[0, k:] * b[0, :64])))
        dropped = K.full_emulate(a, b, mean_k, drop=(0, j, t)).astype(f64)
        assert K.ratio(np.abs(dropped - ref), bound).max() > WIDE


def test_full_exact_inputs_are_exact_in_fp32():
    for mean_k in (1, 2):
        a, b = K.full_exact_inputs(257 + mean_k, 3 * mean_k, 257)
        ref, _ = K.full_ref(a, b, mean_k)
        assert np.array_equal(K.full_emulate(a, b, mean_k).astype(f64), ref)
        assert np.abs(ref).max() * mean_k < 2 ** 24 and np.abs(ref).max() > 20
        wrong = np.roll(ref, 1, axis=1)  # the other lag convention
        assert not np.array_equal(wrong, ref)


# ---- 3. ofp_adjust_onset ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", K.ADJUST_N)
def test_adjust_table_margins_and_branches(n):
    x, y, onsets, new_lag = K.adjust_table(n)
    P = len(new_lag)
    assert x.min() >= f32(0.01) and onsets.min() >= 0 and onsets.max() <= n and np.abs(new_lag).max() <= n
    seen, out = set(), 0
    for p in range(P):
        det = K.adjust_detail(onsets[p], x[p], y[p], new_lag[p])
        assert det["moves"] == tuple(oracle.adjust_onset(onsets[p], x[p], y[p], int(new_lag[p])))
        seen |= det["branches"]
        out += not K.comparable(det)
        if det["Lx"] <= 1 and det["Ly"] <= 1:
            assert det["exact"]
    print(f"\nadjust_onset table n={n}: {out} of {P} left out", end="")
    assert not K.too_many_left_out(out, P)
    if n >= 63:
        assert out == 0
    want = set(K.ADJUST_BRANCHES)
    if n <= K.XW:  # a segment is at most n samples
        want.discard("segment longer than a wave")
    if n == 1:
        want.discard("o0 + lag_diff = -1, da > db")  # n = 1 has no segment on the x side then
    assert seen >= want, want - seen



def test_margin_is_far_above_the_reordering_error():
    rng = np.random.default_rng(8)
    t = np.abs(rng.standard_normal(5000))
    worst = max(abs(np.sum(t) - np.sum(t[rng.permutation(5000)])) / np.sum(t) for _ in range(20))
    pairwise_vs_serial = abs(np.sum(t) - float(np.cumsum(t)[-1])) / np.sum(t)
    assert max(worst, pairwise_vs_serial) <= 5000 * 2.0 ** -53 < K.MARGIN / 1000


# ---- 4. ofp_fix_onsets --------------------------------------------------------------------------------------------

def fix_tables():
    from onset_fingerprinting_amd import synth
    for name, seed, C, n, hits, opt in K.fix_bulk_cases():
        audio, onsets = synth.sensor_hits(seed, n_channels=C, n=n, hits=hits)
        yield name, audio, onsets, opt, K.X_MAXN, None
    audio, onsets, opt = K.fix_short_case()
    yield "short", audio, onsets, opt, K.X_MAXN, None
    audio, onsets, opt = K.fix_equal_case()
    yield "equal", audio, onsets, opt, K.X_MAXN, None
    for name, audio, onsets, opt, ms, _ in K.fix_capacity_cases():
        yield name, audio, onsets, opt, ms, None
    audio, onsets, opt, _ = K.fix_edge_case()
    yield "edges", audio, onsets, opt, K.X_MAXN, None
    audio, onsets, n_groups, opt = K.fix_batch_case()
    yield "batch", audio, onsets, opt, K.X_MAXN, n_groups


def test_fix_ref_is_the_oracle_and_the_margin_rule_keeps_the_tables():
    for name, audio, onsets, opt, ms, n_groups in fix_tables():
        ref, status, comparable, margin = K.fix_ref(audio, onsets, opt, ms, n_groups)
        out = int((~comparable).sum())
        print(f"\nfix_onsets table {name}: {out} of {comparable.size} left out, smallest margin {margin.min():.3g}",
              end="")
        assert np.array_equal(comparable, margin >= K.MARGIN)
        assert not K.too_many_left_out(out, comparable.size), name
        a3 = audio[None] if audio.ndim == 2 else audio
        o3, r3, s3 = (v[None] if audio.ndim == 2 else v for v in (onsets, ref, status))
        for c in range(a3.shape[0]):
            fixed = s3[c] == 0
            if fixed.any():
                assert np.array_equal(oracle.fix_onsets(a3[c], o3[c][fixed], **opt), r3[c][fixed]), name
            shift = {**K.FIX_DEFAULTS, **opt}["shift_onsets"]
            assert np.array_equal(r3[c][s3[c] == 1], o3[c][s3[c] == 1] + shift)
            assert np.array_equal(r3[c][s3[c] == 2], o3[c][s3[c] == 2])


def test_fix_tables_are_what_they_claim():
    opts = [{**K.FIX_DEFAULTS, **c[5]} for c in K.fix_bulk_cases()]
    assert {c[2] for c in K.fix_bulk_cases()} == {1, 2, 64, 128}
    assert {o["filter_size"] for o in opts} >= {1, 3, 15} and {o["d"] for o in opts} == {0, 1, 2, 3, 4}
    assert {o["onset_direction"] for o in opts} == {None, "up", "down"}
    assert {o["shift_onsets"] for o in opts} == {-3, 0, 4}
    assert any(o["take_abs"] for o in opts) and any(o["zero_left"] for o in opts)
    assert any(c[2] == 128 and o["d"] == 4 and o["filter_size"] == 15 for c, o in zip(K.fix_bulk_cases(), opts))
    # sections shorter than the filter
    audio, onsets, opt = K.fix_short_case()
    look = opt["normalization_cutoff"] + opt["onset_tolerance"]
    n_sec = onsets.max(axis=1) - onsets.min(axis=1) + 2 * look
    assert set(n_sec.tolist()) == {2, 3} and opt["filter_size"] == 15
    assert (K.fix_ref(audio, onsets, opt)[1] == 0).all()
    # equal onsets
    audio, onsets, opt = K.fix_equal_case()
    assert all(len(set(row.tolist())) < len(row) for row in onsets) and (K.fix_ref(audio, onsets, opt)[1] == 0).all()
    # capacity and caller-given max_section at equality
    for name, audio, onsets, opt, ms, want in K.fix_capacity_cases():
        n_sec = onsets.max(axis=1) - onsets.min(axis=1) + 80
        assert n_sec.tolist() == [ms, ms + 1] and K.fix_ref(audio, onsets, opt, ms)[1].tolist() == list(want) == [0, 1]
    assert {c[4] for c in K.fix_capacity_cases()} == {4096, 500}
    # clip edges
    audio, onsets, opt, want = K.fix_edge_case()
    lo, hi = onsets.min(axis=1) - 40, onsets.max(axis=1) + 40
    assert lo.tolist()[:2] == [0, -1] and hi.tolist()[2:4] == [len(audio), len(audio) + 1]
    assert (lo[4], hi[4]) == (0, len(audio)) and K.fix_ref(audio, onsets, opt)[1].tolist() == list(want)
    # batch
    audio, onsets, n_groups, opt = K.fix_batch_case()
    assert K.fix_ref(audio, onsets, opt, n_groups=n_groups)[1].tolist() == [[0, 0, 1, 2], [0, 2, 2, 2], [0, 1, 0, 0]]


def test_reflection_rule_is_scipys_for_sections_shorter_than_the_filter():
    from scipy.ndimage import median_filter
    rng = np.random.default_rng(4)
    for n in (2, 3, 5, 7, 40):
        for fs in (1, 3, 15):
            col = rng.standard_normal(n).astype(f32)
            want = median_filter(col[:, None], fs, axes=0)[:, 0]
            got = np.array([K.median_at_rule(col, t, fs) for t in range(n)], f32)
            assert np.array_equal(got, want), (n, fs)


# ---- 5. ofp_onset_region ------------------------------------------------------------------------------------------

def test_region_hand_cases_give_the_intended_answers():
    for name, audio, onset, n, med, factor, want in K.region_hand_cases():
        assert K.region_ref(audio, onset, n, med, factor) == want, name
    name, audio, onset, n, med, factor, want = K.region_hand_cases()[0]
    assert want == 40 and audio[20:24].tolist() == [1.0] * 4 and audio[40:45].tolist() == [1.0] * 5  # the second run


def test_region_ref_agrees_with_scipy_and_covers_the_positions():
    from scipy.ndimage import binary_opening
    from scipy.signal import medfilt
    audio = K.region_audio()
    N = len(audio)
    for n in K.REGION_N:
        onsets = K.region_onsets(n)
        h = n // 2
        lens = [min(o + h, N) - max(o - h, 0) for o in onsets]
        assert 0 in onsets.tolist() and any(ln <= 0 for ln in lens)
        if n >= 100:
            assert any(0 < ln < n and ln % 2 == 1 for ln in lens) and any(o - h < 0 < o for o in onsets)
            assert any(o + h > N > o for o in onsets) and n in lens
        for o, ln in zip(onsets, lens):
            if ln <= 0:
                assert K.region_ref(audio, o, n, 3, 0.5) == max(o - h, 0)
                continue
            for med in K.REGION_MED:
                a = np.abs(audio[max(o - h, 0):min(o + h, N)])
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")  # scipy warns when it zero-pads a region shorter than the filter
                    f = medfilt(a, med) if med > 1 else a
                want = max(o - h, 0) + int(np.argmax(binary_opening(f > f32(0.5) * f.max(), np.ones(5))))
                assert K.region_ref(audio, o, n, med, 0.5) == want, (n, o, med)


# ---- 6. ofp_resample_windows --------------------------------------------------------------------------------------

def test_resample_launches_hold_every_pair_inside_and_past_the_clip():
    seen = set()
    for c in K.resample_launches():
        assert c["max_nx"] >= c["nx"].max() and c["max_nx"] <= 2048 and len(set(c["nx"].tolist())) >= 1
        for st, nx in zip(c["start"], c["nx"]):
            where = "before" if st < 0 else "past" if st + nx > K.RESAMPLE_CLIP else "inside"
            seen.add((int(nx), c["num"], where))
    assert seen == {(nx, num, w) for nx, num in K.RESAMPLE_PAIRS for w in ("before", "past", "inside")}
    w = K.resample_window(K.resample_audio(3), -2, 5, 1)
    assert w[:2].tolist() == [0, 0] and np.array_equal(w[2:], K.resample_audio(3)[:3, 1])


@pytest.mark.parametrize("nx,num", K.RESAMPLE_PAIRS)
def test_resample_emulation_is_inside_the_bound_and_faults_are_not(nx, num):
    from scipy.signal import resample
    x = np.random.default_rng(nx * 3000 + num).standard_normal(nx).astype(f32)
    ref, bound = K.resample_ref(x, num)
    assert np.abs(ref - resample(x.astype(f64), num)).max() <= 1e-11 * np.abs(x).sum()  # the same function as scipy's
    r = K.ratio(np.abs(K.resample_emulate(x, num).astype(f64) - ref), bound)
    print(f"\nemulated ofp_resample_windows {nx}->{num}: largest error / bound {r.max():.3g}", end="")
    assert r.max() <= 1.0
    N = min(nx, num)
    faults = ["dropped term"] if nx > 1 else []
    if N % 2 == 0 and nx != num:
        faults.append("nyquist scale")
    if num % 2 == 0 and num <= nx:
        faults.append("nyquist real")
    for fault in faults:
        rf = K.ratio(np.abs(K.resample_emulate(x, num, fault).astype(f64) - ref), bound)
        assert rf.max() > WIDE, (fault, rf.max())


def test_every_nyquist_branch_is_in_the_pairs():
    kinds = set()
    for nx, num in K.RESAMPLE_PAIRS:
        N = min(nx, num)
        kinds.add(("even" if N % 2 == 0 else "odd", "down" if num < nx else "up" if nx < num else "equal",
                   "last bin real" if num % 2 == 0 and num <= nx else "-"))
    assert kinds >= {("even", "down", "last bin real"), ("even", "up", "-"), ("even", "equal", "last bin real"),
                     ("odd", "down", "-"), ("odd", "up", "-"), ("odd", "equal", "-")}


# ---- 7. ofp_filter_direction --------------------------------------------------------------------------------------

def test_filter_inputs_hold_the_edges():
    n, C = K.FILTER_STRIDE_CASE
    assert K.FILTER_GRID_PASS < n * C and C == 7 and K.FILTER_GRID_PASS % C != 0
    assert {c for _, c in K.FILTER_SMALL} == {1, 3}
    x = K.filter_input(71, 1000, 3)
    d = np.diff(x, axis=0)
    assert (x[0] < 0).all() and (d == 0).sum() > 20 and np.signbit(x[x == 0]).any() and (~np.signbit(x[x == 0])).any()
    for name in ("up", "down"):
        y = K.filter_ref(x, name)
        assert np.array_equal(y[0], x[0])
        keep = np.vstack([np.ones((1, 3), bool), (d >= 0) if name == "up" else (d <= 0)])
        assert np.array_equal(y[keep].view(np.uint32), x[keep].view(np.uint32)) and (y[~keep] == 0).all()
        assert not np.signbit(y[~keep]).any() and keep[1:][d == 0].all()
