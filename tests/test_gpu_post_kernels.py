"""The kernels of csrc/ofp_xcorr.hip and csrc/ofp_post.hip one by one, through the C ABI, on the case tables of
oracle/post_kernels.py: ofp_xcorr_lag bit for bit, ofp_xcorr_full and ofp_resample_windows within their derived
bounds per element, ofp_adjust_onset, ofp_fix_onsets, ofp_onset_region and ofp_filter_direction for equality, at the
capacities, tile seams, clamps and ties the golden captures never reach.  tests/test_post_kernels_cpu.py shows that
the references, bounds and margins are sound.

Every output is written into a buffer filled with NaN (integers: INT32_MIN / INT64_MIN) with a guard tail, so an
element that was not written or a store past the end fails as well.  `pytest -s` prints the largest error / bound
of the two bounded primitives and the number of cases the margin rule left out.
"""
import ctypes

import numpy as np
import pytest
import torch

from oracle import post_kernels as K

pytestmark = pytest.mark.gpu

f32, f64 = np.float32, np.float64
GUARD = 64
I32_MIN, I64_MIN = -2 ** 31, -2 ** 63
RATIOS = {}    # primitive -> largest error / bound seen
LEFT_OUT = {}  # primitive -> [left out, total]


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    for name in sorted(RATIOS):
        print(f"\nlargest error / bound, {name}: {RATIOS[name]:.3g}", end="")
    for name in sorted(LEFT_OUT):
        print(f"\nleft out by the margin rule, {name}: {LEFT_OUT[name][0]} of {LEFT_OUT[name][1]}", end="")
    print()


def L():
    from onset_fingerprinting_amd import _lib
    return _lib.lib()


def last_error():
    from onset_fingerprinting_amd import _lib
    return _lib.last_error()


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def ok(rc, what):
    from onset_fingerprinting_amd import _lib
    _lib.check(rc, what)


def dev(a, dt=f32):
    return torch.from_numpy(np.ascontiguousarray(a, dt)).cuda()


_FILL = {torch.float32: float("nan"), torch.int32: I32_MIN, torch.int64: I64_MIN}


def guarded(*shape, dtype=torch.float32):
    """(view of `shape`, whole buffer): NaN (integers: the most negative value) everywhere, GUARD elements behind."""
    numel = int(np.prod(shape))
    buf = torch.full((numel + GUARD,), _FILL[dtype], dtype=dtype, device="cuda")
    return buf[:numel].view(*shape), buf


def untouched(t):
    return bool(torch.isnan(t).all()) if t.dtype == torch.float32 else bool((t == _FILL[t.dtype]).all())


def guard_ok(buf):
    return untouched(buf[-GUARD:])


def padded(rows, stride):
    """rows [R, L] -> device buffer [R * stride] with NaN between the rows."""
    R, n = rows.shape
    buf = torch.full((R, stride), float("nan"), dtype=torch.float32, device="cuda")
    buf[:, :n] = dev(rows)
    return buf


def within(name, got, ref, bound, ctx):
    got = got.detach().cpu().numpy().astype(f64) if torch.is_tensor(got) else np.asarray(got, f64)
    assert got.shape == ref.shape, (name, ctx, got.shape, ref.shape)
    r = K.ratio(np.abs(got - ref), bound)
    RATIOS[name] = max(RATIOS.get(name, 0.0), float(r.max()) if r.size else 0.0)
    assert bool((r <= 1.0).all()), (name, ctx, f"error / bound = {r.max():.3g} at {np.argwhere(r > 1.0)[:4].tolist()}")


def refused(rc, what):
    assert rc != 0, (what, "was accepted")
    assert last_error().strip(), (what, "no message")


def left_out(name, n_out, total):
    LEFT_OUT.setdefault(name, [0, 0])
    LEFT_OUT[name][0] += n_out
    LEFT_OUT[name][1] += total
    assert not K.too_many_left_out(n_out, total), (name, f"{n_out} of {total} cases below the margin")


# ---- 1. ofp_xcorr_lag ---------------------------------------------------------------------------------------------

def xcorr_lag(x, y, d, take_abs, cutoff, windows, cc_stride):
    """-> (argmax [P] numpy, cc [P, cc_stride] numpy or None); cc_stride None: no cc buffer."""
    P, n_in = x.shape
    lo, hi = dev([w[0] for w in windows], np.int32), dev([w[1] for w in windows], np.int32)
    am, abuf = guarded(P, dtype=torch.int32)
    cc, cbuf = guarded(P, cc_stride) if cc_stride else (None, None)
    ok(L().ofp_xcorr_lag(x.data_ptr(), y.data_ptr(), P, n_in, d, take_abs, cutoff, lo.data_ptr(), hi.data_ptr(),
                         am.data_ptr(), cc.data_ptr() if cc_stride else None, cc_stride or 0, stream()),
       "ofp_xcorr_lag")
    torch.cuda.synchronize()
    assert guard_ok(abuf) and (cbuf is None or guard_ok(cbuf)), "store past the end"
    return am.cpu().numpy(), (cc.cpu().numpy() if cc_stride else None)


def check_lag(xs, ys, d, take_abs, cutoff, windows, cc_stride, truncating, ctx):
    am, cc = xcorr_lag(dev(xs), dev(ys), d, take_abs, cutoff, windows, cc_stride)
    am_only, _ = xcorr_lag(dev(xs), dev(ys), d, take_abs, cutoff, windows, None)
    for p, (lo, hi) in enumerate(windows):
        ref_am, ref_cc = K.lag_ref(xs[p], ys[p], d, take_abs, cutoff, lo, hi, cc_stride if truncating else None)
        w = len(ref_cc)
        assert w <= cc_stride
        assert np.array_equal(cc[p, :w].view(np.uint32), ref_cc.view(np.uint32)), (ctx, p, lo, hi, "cc bits")
        assert np.isnan(cc[p, w:]).all(), (ctx, p, lo, hi, "written past the window")
        assert am[p] == ref_am, (ctx, p, lo, hi, int(am[p]), ref_am)
        if not truncating:
            assert am_only[p] == ref_am, (ctx, p, lo, hi, "without a cc buffer", int(am_only[p]), ref_am)


@pytest.mark.parametrize("d", K.LAG_D)
def test_xcorr_lag_every_seam_cutoff_and_window(d):
    for take_abs in K.LAG_ABS:
        for n_in in K.lag_n_in(d):
            n = n_in - d
            windows = K.lag_windows(n)
            xs, ys = K.lag_inputs(1000 * d + 10 * n_in + take_abs, len(windows), n_in)
            stride = max(K.clamp_window(lo, hi, n)[1] - K.clamp_window(lo, hi, n)[0] for lo, hi in windows) + 3
            for cutoff in K.lag_cutoffs(n):
                check_lag(xs, ys, d, take_abs, cutoff, windows, stride, False, (d, take_abs, n_in, cutoff))


def test_xcorr_lag_cc_stride_smaller_than_the_window():
    c = K.LAG_STRIDE_CASE
    n = c["n_in"] - c["d"]
    windows = [(0, 2 * n - 1), (-4, 700), (n - 100, n + 157), (3, 3)]
    xs, ys = K.lag_inputs(77, len(windows), c["n_in"])
    for stride in c["strides"]:
        check_lag(xs, ys, c["d"], 1, c["cutoff"], windows, stride, True, ("cc_stride", stride))


def test_xcorr_lag_ties_take_the_first_index():
    cases = K.tie_cases()
    n = K.TIE_N
    T = 2 * n - 1
    for sign in (1.0, -1.0):
        pairs = [K.tie_inputs(c, sign) for c in cases] + [(np.zeros(n, f32), np.zeros(n, f32))]
        xs, ys = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
        for lo in (0, 100):
            windows = [(lo, T)] * len(pairs)
            for cutoff in (n, 2 * n):
                am, cc = xcorr_lag(dev(xs), dev(ys), 0, 0, cutoff, windows, T)
                for p in range(len(pairs)):
                    ref_am, ref_cc = K.lag_ref(xs[p], ys[p], 0, 0, cutoff, lo, T)
                    assert np.array_equal(cc[p, :T - lo].view(np.uint32), ref_cc.view(np.uint32))
                    assert am[p] == ref_am, (sign, lo, cutoff, p, int(am[p]), ref_am)
                    if p == len(cases):
                        assert am[p] == 0  # all zero
                    elif sign > 0:
                        assert am[p] == cases[p]["first"] - lo, (cases[p]["name"], lo, int(am[p]))
                    else:
                        assert am[p] == 0  # the planted lags are the minima, every other lag ties at 0


def test_xcorr_lag_refusals():
    n_in = 300
    xs, ys = K.lag_inputs(5, 2, 4097)
    x, y = dev(xs), dev(ys)
    lo, hi = dev([0, 0], np.int32), dev([50, 50], np.int32)
    for what, (ni, d, cutoff) in {"n_in = 4097": (4097, 0, 10), "d = 5": (n_in, 5, 10), "n_in - d = 0": (3, 3, 10),
                                  "cutoff < 0": (n_in, 0, -1)}.items():
        am, abuf = guarded(2, dtype=torch.int32)
        cc, cbuf = guarded(2, 50)
        rc = L().ofp_xcorr_lag(x.data_ptr(), y.data_ptr(), 2, ni, d, 0, cutoff, lo.data_ptr(), hi.data_ptr(),
                               am.data_ptr(), cc.data_ptr(), 50, stream())
        torch.cuda.synchronize()
        refused(rc, what)
        assert untouched(abuf) and untouched(cbuf), (what, "output written")
        check_lag(xs[:, :n_in].copy(), ys[:, :n_in].copy(), 1, 0, 10, [(0, 50), (100, 150)], 50, False, ("after", what))


# ---- 2. ofp_xcorr_full --------------------------------------------------------------------------------------------

def xcorr_full(a, b, mean_k):
    rows, n = a.shape
    sa, sb = n + K.FULL_PAD_A, n + K.FULL_PAD_B
    ad, bd = padded(a, sa), padded(b, sb)
    out, buf = guarded(rows // mean_k, 2 * n - 1)
    ok(L().ofp_xcorr_full(ad.data_ptr(), bd.data_ptr(), rows, n, sa, sb, mean_k, out.data_ptr(), stream()),
       "ofp_xcorr_full")
    torch.cuda.synchronize()
    assert guard_ok(buf), "store past the end"
    return out.cpu().numpy()


@pytest.mark.parametrize("length", K.FULL_L)
def test_xcorr_full_within_the_fma_chain_bound(length):
    for mean_k in K.FULL_MEAN_K:
        for out_rows in K.FULL_ROWS:
            a, b = K.full_inputs(2000 + 10 * length + mean_k + out_rows, out_rows * mean_k, length)
            ref, bound = K.full_ref(a, b, mean_k)
            within("ofp_xcorr_full", xcorr_full(a, b, mean_k), ref, bound, (length, mean_k, out_rows))


@pytest.mark.parametrize("mean_k", (1, 2))
def test_xcorr_full_exact_on_small_integers(mean_k):
    for length in (1, 2, 129, 257):
        a, b = K.full_exact_inputs(length + mean_k, 3 * mean_k, length)
        ref, _ = K.full_ref(a, b, mean_k)
        got = xcorr_full(a, b, mean_k)
        assert np.array_equal(got.astype(f64), ref), (length, mean_k, np.argwhere(got != ref)[:4].tolist())


def test_xcorr_full_refusals():
    a, b = K.full_inputs(9, 4, 4097)
    ad, bd = dev(a), dev(b)
    for what, (rows, n, mean_k) in {"L = 4097": (4, 4097, 1), "n_rows % mean_k != 0": (4, 100, 3),
                                    "mean_k = 0": (4, 100, 0)}.items():
        out, buf = guarded(4, 2 * n - 1)
        rc = L().ofp_xcorr_full(ad.data_ptr(), bd.data_ptr(), rows, n, 4097, 4097, mean_k, out.data_ptr(), stream())
        torch.cuda.synchronize()
        refused(rc, what)
        assert untouched(buf), (what, "output written")
        ref, bound = K.full_ref(a[:, :100], b[:, :100], 2)
        within("ofp_xcorr_full", xcorr_full(a[:, :100].copy(), b[:, :100].copy(), 2), ref, bound, ("after", what))


# ---- 3. ofp_adjust_onset ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", K.ADJUST_N)
def test_adjust_onset_every_clamp(n):
    x, y, onsets, new_lag = K.adjust_table(n)
    P = len(new_lag)
    moves, buf = guarded(P, 2, dtype=torch.int32)
    xd, yd, od, ld = dev(x), dev(y), dev(onsets, np.int32), dev(new_lag, np.int32)
    ok(L().ofp_adjust_onset(xd.data_ptr(), yd.data_ptr(), P, n, od.data_ptr(), ld.data_ptr(), moves.data_ptr(),
                            stream()), "ofp_adjust_onset")
    torch.cuda.synchronize()
    assert guard_ok(buf)
    got = moves.cpu().numpy()
    details = [K.adjust_detail(onsets[p], x[p], y[p], new_lag[p]) for p in range(P)]
    keep = [p for p in range(P) if K.comparable(details[p])]
    left_out("ofp_adjust_onset", P - len(keep), P)
    assert (got != I32_MIN).all(), "a move was not written"
    for p in keep:
        assert tuple(got[p]) == details[p]["moves"], (n, p, onsets[p].tolist(), int(new_lag[p]), got[p].tolist(),
                                                      details[p])


# ---- 4. ofp_fix_onsets --------------------------------------------------------------------------------------------

def fix_onsets(audio, onsets, opt, max_section=4096, n_groups=None, ws_short=0, raw=None):
    """-> (rc, onsets numpy, status numpy).  The work space is exactly the size asked for (less ws_short bytes), with
    a guard behind it."""
    o = {**K.FIX_DEFAULTS, **opt, **(raw or {})}
    a3 = audio[None] if audio.ndim == 2 else audio
    o3 = onsets[None] if audio.ndim == 2 else onsets
    n_clips, N, C = a3.shape
    cap = o3.shape[1]
    ad = dev(a3)
    od, obuf = guarded(n_clips, cap, C, dtype=torch.int64)
    od.copy_(dev(o3, np.int64))
    st, sbuf = guarded(n_clips, cap, dtype=torch.int32)
    ws_bytes = int(L().ofp_fix_onsets_workspace_bytes(n_clips * cap, C, max_section))
    assert ws_bytes == n_clips * cap * C * max_section * 4
    ws = torch.full((ws_bytes + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    ng = None if n_groups is None else dev(n_groups, np.int64)
    direction = o["direction"] if "direction" in o else K.DIRECTIONS[o["onset_direction"]]
    rc = L().ofp_fix_onsets(ad.data_ptr(), n_clips, N, C, od.data_ptr(), cap, None if ng is None else ng.data_ptr(),
                            o["filter_size"], o["d"], direction, int(o["take_abs"]), int(o["zero_left"]),
                            o["normalization_cutoff"], o["onset_tolerance"], o["shift_onsets"], max_section,
                            st.data_ptr(), ws.data_ptr(), ws_bytes - ws_short, stream())
    torch.cuda.synchronize()
    assert guard_ok(obuf) and guard_ok(sbuf) and bool((ws[-GUARD:] == 0xA5).all()), "store past the end"
    return rc, od.cpu().numpy().reshape(onsets.shape), st.cpu().numpy().reshape(onsets.shape[:-1])


def check_fix(name, audio, onsets, opt, max_section=4096, n_groups=None, want_status=None):
    ref, ref_status, comparable, _ = K.fix_ref(audio, onsets, opt, max_section, n_groups)
    rc, got, status = fix_onsets(audio, onsets, opt, max_section, n_groups)
    ok(rc, "ofp_fix_onsets")
    left_out("ofp_fix_onsets", int((~comparable).sum()), comparable.size)
    assert np.array_equal(status, ref_status), (name, status.tolist(), ref_status.tolist())
    if want_status is not None:
        assert status.ravel().tolist() == list(want_status), (name, status.tolist())
    assert np.array_equal(got[status == 2], onsets[status == 2]), (name, "a row not in use was touched")
    shift = {**K.FIX_DEFAULTS, **opt}["shift_onsets"]
    assert np.array_equal(got[status == 1], onsets[status == 1] + shift), (name, "status 1 is shifted only")
    assert np.array_equal(got[comparable], ref[comparable]), (name, np.argwhere(got != ref)[:6].tolist())
    return status


@pytest.mark.parametrize("case", K.fix_bulk_cases(), ids=lambda c: c[0])
def test_fix_onsets_channel_counts_and_options(case):
    from onset_fingerprinting_amd import synth
    name, seed, C, n, hits, opt = case
    audio, onsets = synth.sensor_hits(seed, n_channels=C, n=n, hits=hits)
    status = check_fix(name, audio, onsets, opt)
    assert (status == 0).all(), (name, status.tolist())


def test_fix_onsets_section_shorter_than_the_filter():
    audio, onsets, opt = K.fix_short_case()
    status = check_fix("short sections", audio, onsets, opt)
    assert (status == 0).all()
    check_fix("short sections, C 2", np.ascontiguousarray(audio[:, :2]), np.ascontiguousarray(onsets[:, :2]), opt)


def test_fix_onsets_equal_onsets_in_a_group():
    audio, onsets, opt = K.fix_equal_case()
    assert (check_fix("equal onsets", audio, onsets, opt) == 0).all()


@pytest.mark.parametrize("case", K.fix_capacity_cases(), ids=lambda c: c[0])
def test_fix_onsets_max_section_at_equality(case):
    name, audio, onsets, opt, max_section, want = case
    check_fix(name, audio, onsets, opt, max_section, want_status=want)


def test_fix_onsets_clip_edges_at_equality():
    audio, onsets, opt, want = K.fix_edge_case()
    check_fix("clip edges", audio, onsets, opt, want_status=want)


def test_fix_onsets_batch_with_group_mask():
    audio, onsets, n_groups, opt = K.fix_batch_case()
    status = check_fix("batch", audio, onsets, opt, n_groups=n_groups)
    assert status.tolist() == [[0, 0, 1, 2], [0, 2, 2, 2], [0, 1, 0, 0]]


def test_fix_onsets_refusals():
    from onset_fingerprinting_amd import synth
    audio, onsets = synth.sensor_hits(47, n_channels=2, n=6000, hits=3)
    wide = np.zeros((6000, 129), f32)
    wide_onsets = np.full((1, 129), 3000, np.int64)
    attempts = {"work space one byte short": dict(ws_short=1), "filter_size = 16": dict(raw=dict(filter_size=16)),
                "d = 5": dict(raw=dict(d=5)), "direction = 3": dict(raw=dict(direction=3))}
    for what, kw in attempts.items():
        rc, got, status = fix_onsets(audio, onsets, {}, **kw)
        refused(rc, what)
        assert np.array_equal(got, onsets) and (status == I32_MIN).all(), (what, "something was launched")
    rc, got, status = fix_onsets(wide, wide_onsets, {})
    refused(rc, "C = 129")
    assert np.array_equal(got, wide_onsets) and (status == I32_MIN).all()
    check_fix("after the refusals", audio, onsets, {})


# ---- 5. ofp_onset_region ------------------------------------------------------------------------------------------

def onset_region(audio, onsets, n, med, factor):
    out, buf = guarded(len(onsets), dtype=torch.int64)
    ad, od = dev(audio), dev(onsets, np.int64)
    rc = L().ofp_onset_region(ad.data_ptr(), len(audio), od.data_ptr(), len(onsets), n, med, factor, out.data_ptr(),
                              stream())
    torch.cuda.synchronize()
    assert guard_ok(buf)
    return rc, out.cpu().numpy(), buf


@pytest.mark.parametrize("n", K.REGION_N)
def test_onset_region_sizes_and_positions(n):
    audio = K.region_audio()
    onsets = K.region_onsets(n)
    for med in K.REGION_MED:
        for factor in (0.5, 0.2):
            rc, got, _ = onset_region(audio, onsets, n, med, factor)
            ok(rc, "ofp_onset_region")
            ref = [K.region_ref(audio, o, n, med, factor) for o in onsets]
            assert got.tolist() == ref, (n, med, factor, onsets.tolist())
    empty = [o for o in onsets if min(o + n // 2, len(audio)) - max(o - n // 2, 0) <= 0]
    assert empty and all(K.region_ref(audio, o, n, 3, 0.5) == max(o - n // 2, 0) for o in empty)


def test_onset_region_hand_built_signals():
    for name, audio, onset, n, med, factor, want in K.region_hand_cases():
        rc, got, _ = onset_region(audio, np.array([onset, onset], np.int64), n, med, factor)
        ok(rc, "ofp_onset_region")
        assert got.tolist() == [want, want], (name, got.tolist(), want)


def test_onset_region_refusals():
    audio = K.region_audio()
    onsets = np.array([700, 4100], np.int64)
    for what, (n, med) in {"n = 4098": (4098, 5), "median_filter_size = 35": (256, 35),
                           "even median_filter_size": (256, 4)}.items():
        rc, got, buf = onset_region(audio, onsets, n, med, 0.5)
        refused(rc, what)
        assert untouched(buf), (what, "output written")
        rc, got, _ = onset_region(audio, onsets, 256, 5, 0.5)
        ok(rc, "ofp_onset_region")
        assert got.tolist() == [K.region_ref(audio, o, 256, 5, 0.5) for o in onsets], ("after", what)


# ---- 6. ofp_resample_windows --------------------------------------------------------------------------------------

def resample(ad, n_samples, C, start, nx, max_nx, num):
    out, buf = guarded(len(nx), C, num)
    sd, nd = dev(start, np.int64), dev(nx, np.int32)
    rc = L().ofp_resample_windows(ad.data_ptr(), n_samples, C, sd.data_ptr(), nd.data_ptr(), len(nx), max_nx, num,
                                  out.data_ptr(), stream())
    torch.cuda.synchronize()
    assert guard_ok(buf)
    return rc, out.cpu().numpy(), buf


@pytest.mark.parametrize("launch", K.resample_launches(), ids=lambda c: f"num{c['num']}")
def test_resample_every_parity_and_window_position(launch):
    c = launch
    for C in (3, 1) if c["num"] <= 257 else (3,):
        audio = K.resample_audio(C)
        rc, got, _ = resample(dev(audio), len(audio), C, c["start"], c["nx"], c["max_nx"], c["num"])
        ok(rc, "ofp_resample_windows")
        for i, (st, nx) in enumerate(zip(c["start"], c["nx"])):
            for ch in range(C):
                ref, bound = K.resample_ref(K.resample_window(audio, int(st), int(nx), ch), c["num"])
                within("ofp_resample_windows", got[i, ch], ref, bound, (int(nx), c["num"], int(st), C, ch))


def test_resample_refusals():
    audio = K.resample_audio(1)
    ad = dev(audio)
    start, nx = np.array([10, 500], np.int64), np.array([300, 256], np.int32)
    for what, (max_nx, num) in {"num = 2049": (300, 2049), "max_nx = 2049": (2049, 256)}.items():
        rc, got, buf = resample(ad, len(audio), 1, start, nx, max_nx, num)
        refused(rc, what)
        assert untouched(buf), (what, "output written")
        rc, got, _ = resample(ad, len(audio), 1, start, nx, 300, 256)
        ok(rc, "ofp_resample_windows")
        for i in range(2):
            ref, bound = K.resample_ref(K.resample_window(audio, int(start[i]), int(nx[i]), 0), 256)
            within("ofp_resample_windows", got[i, 0], ref, bound, ("after", what, i))


# ---- 7. ofp_filter_direction --------------------------------------------------------------------------------------

def filter_direction(xd, n, C, direction, yd=None):
    out, buf = guarded(n, C)
    rc = L().ofp_filter_direction(xd.data_ptr(), n, C, direction, (out if yd is None else yd).data_ptr(), stream())
    torch.cuda.synchronize()
    assert guard_ok(buf)
    return rc, out, buf


def check_filter(n, C, seed):
    x = K.filter_input(seed, n, C)
    xd = dev(x)
    for name, direction in (("up", 1), ("down", 2)):
        rc, out, _ = filter_direction(xd, n, C, direction)
        ok(rc, "ofp_filter_direction")
        ref = K.filter_ref(x, name)
        got = out.cpu().numpy()
        assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), (n, C, name,
                                                                           np.argwhere(got != ref)[:4].tolist())
        assert np.array_equal(got[0].view(np.uint32), x[0].view(np.uint32)), "row 0 is always kept"


def test_filter_direction_grid_stride():
    n, C = K.FILTER_STRIDE_CASE
    assert K.FILTER_GRID_PASS < n * C < K.FILTER_GRID_PASS + 64
    check_filter(n, C, 70)


@pytest.mark.parametrize("shape", K.FILTER_SMALL, ids=lambda s: f"{s[0]}x{s[1]}")
def test_filter_direction_small(shape):
    check_filter(shape[0], shape[1], 71 + shape[0] + shape[1])


def test_filter_direction_refusals():
    x = K.filter_input(72, 100, 3)
    xd = dev(x)
    rc, out, buf = filter_direction(xd, 100, 3, 1, yd=xd)
    refused(rc, "d_x == d_y")
    assert np.array_equal(xd.cpu().numpy().view(np.uint32), x.view(np.uint32)), "the input was written"
    for direction in (0, 3):
        rc, out, buf = filter_direction(xd, 100, 3, direction)
        refused(rc, f"direction = {direction}")
        assert untouched(buf)
    check_filter(100, 3, 72)
