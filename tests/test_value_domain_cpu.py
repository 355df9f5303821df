"""CPU-only companion of tests/test_gpu_canon.py and tests/test_gpu_value_domain.py.

1. The host canon of include/ofp_math.h over ALL of the sets L and E (tests/value_domain_cases.py) against numpy's fp64
   log10 / power rounded once: never more than 1 ulp apart, and every value that differs is adjudicated with mpmath at 256
   bits -- the canon is the correctly rounded float, or the exact result lies within 2^-50 (relative) of a rounding tie, the
   bound the header states for itself.  At most 8 values may differ per function (a cap: the adjudication cannot hide a
   broken polynomial).
2. The arithmetic around the two transcendental maps (rect_db, rel_linear) and the three step functions against a
   restatement in numpy float32 operations, bit for bit, on the specials, the step pairs and samples of the dense sets.
3. What ofp_canon_eval and ofp_detector_create refuse (the refusals come before the first HIP call).
4. Every value class of the detector tests reaches, on the oracle alone, what it is there for."""
import ctypes

import numpy as np
import pytest

import oracle
from tests import value_domain_cases as vd

MAX_DIFFERING = 8


def ulps_apart(a, b):
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def adjudicate(fn_exact, x, canon, other):
    """x: one input (float), canon / other: the two float32 results, 1 ulp apart.  -> (ok, log2 of the relative distance of
    the exact result from the tie between them)."""
    import mpmath
    with mpmath.workprec(256):
        exact = fn_exact(mpmath.mpf(float(x)))
        c, o = mpmath.mpf(float(canon)), mpmath.mpf(float(other))
        tie = (c + o) / 2
        dist = abs(exact - tie) / abs(exact)
        canon_is_nearest = abs(exact - c) < abs(exact - o)
        return bool(canon_is_nearest or dist <= mpmath.mpf(2) ** -50), float(mpmath.log(dist, 2)) if dist else -np.inf


def check_against_fp64(groups, canon_fn, np_fn, mp_fn, both_signs):
    differing = []
    for name, make in groups.items():
        for neg in ((False, True) if both_signs else (False,)):
            x = make(neg)
            got = canon_fn(x)
            with np.errstate(all="ignore"):
                want = np_fn(x.astype(np.float64)).astype(np.float32)
            d = ulps_apart(got, want)
            assert d.max() <= 1, (name, neg, x[np.argmax(d)], "more than 1 ulp from the fp64 evaluation")
            for i in np.nonzero(d)[0]:
                differing.append((name, float(x[i]), got[i], want[i]))
    print(f"{len(differing)} values differ from the fp64 evaluation rounded once")
    assert len(differing) <= MAX_DIFFERING, differing
    for name, x, c, w in differing:
        ok, log2_dist = adjudicate(mp_fn, x, c, w)
        print(f"  {name}: x = {x!r}: canon {float(c)!r}, fp64 path {float(w)!r}, exact result 2^{log2_dist:.1f} from the tie")
        assert ok, (name, x, float(c), float(w), log2_dist)


def test_log10_canon_over_all_of_L():
    import mpmath
    check_against_fp64(vd.L_GROUPS, oracle.log10f, np.log10, mpmath.log10, both_signs=False)


def test_exp10_canon_over_all_of_E():
    import mpmath
    check_against_fp64(vd.E_GROUPS, oracle.exp10f, lambda v: np.power(10.0, v), lambda v: mpmath.power(10, v),
                       both_signs=True)


def test_log10_and_exp10_on_the_specials():
    s = vd.specials()
    with np.errstate(all="ignore"):
        lg, ex = oracle.log10f(s), oracle.exp10f(s)
        want_lg = np.log10(s.astype(np.float64)).astype(np.float32)
        want_ex = np.power(10.0, s.astype(np.float64)).astype(np.float32)
    # (numpy's fp64 path rounded once: same zeros, infinities and NaN positions; values within 1 ulp)
    for got, want in ((lg, want_lg), (ex, want_ex)):
        assert np.array_equal(np.isnan(got), np.isnan(want))
        fin = ~np.isnan(want)
        assert np.array_equal(np.isinf(got[fin]), np.isinf(want[fin])) and ulps_apart(got[fin], want[fin]).max() <= 1
    assert vd.bits(oracle.exp10f(np.float32([39.0, -46.0]))).tolist() == [0x7F800000, 0]


def _dense_sample(groups, both_signs, step=997):
    parts = []
    for make in groups.values():
        for neg in ((False, True) if both_signs else (False,)):
            parts.append(make(neg)[::step])
    return np.concatenate(parts + [vd.specials()])


@pytest.mark.parametrize("floor", vd.RECT_DB_FLOORS)
def test_rect_db_is_the_reference_formula_around_log10(floor):
    x = _dense_sample({**vd.L_GROUPS, **vd.L93_GROUPS}, True)
    got = oracle.rect_db(x, floor)
    want = vd.np_rect_db(x, floor, oracle.log10f)
    assert len(vd.same_where_not_nan(got, want)) == 0
    # the cancellation x + 1e-10f == 0 gives -inf, then the floor
    assert oracle.rect_db(np.float32([-1e-10]), floor)[0] == np.float32(floor)


@pytest.mark.parametrize("floor", vd.REL_LINEAR_FLOORS)
def test_rel_linear_is_the_reference_formula_around_exp10(floor):
    d = _dense_sample({**vd.E_GROUPS, **vd.E9_GROUPS}, True)
    got = oracle.rel_linear(d, floor)
    want = vd.np_rel_linear(d, floor, oracle.exp10f)
    assert len(vd.same_where_not_nan(got, want)) == 0
    assert got[~np.isnan(got)].min() == 0.0 and got[~np.isnan(got)].max() == np.float32(-floor)


@pytest.mark.parametrize("pairs", list(vd.STEP_SETS))
def test_step_functions_are_the_reference_formulas(pairs):
    x, y = vd.STEP_SETS[pairs]()
    for att, rel in vd.AR_COEFFS:
        assert len(vd.same_where_not_nan(oracle.ar_step(x, y, att, rel), vd.np_ar_step(x, y, att, rel))) == 0, (att, rel)
    for alpha, minmin in vd.MIN_COEFFS:
        assert len(vd.same_where_not_nan(oracle.min_step(x, y, alpha, minmin), vd.np_min_step(x, y, alpha, minmin))) == 0
    for (alpha,) in vd.MAX_COEFFS:
        assert len(vd.same_where_not_nan(oracle.max_step(x, y, alpha), vd.np_max_step(x, y, alpha))) == 0


def test_the_sets_have_the_stated_sizes():
    n_L = sum(len(m()) for m in vd.L_GROUPS.values())
    n_E = 2 * sum(len(m()) for m in vd.E_GROUPS.values())
    assert n_L == 6 * (1 << 23) - 1 + 254 * len(vd.SWEEP_MANT) and len(vd.SWEEP_MANT) == 4100
    assert n_E == 8 * (1 << 23)
    assert max(len(m()) for g in (vd.L_GROUPS, vd.L93_GROUPS, vd.E_GROUPS, vd.E9_GROUPS) for m in g.values()) <= vd.CHUNK
    x, y = vd.near_pairs()
    assert len(x) > (1 << 20) and np.all(np.abs(x.astype(np.float64) - y) < 1e-10)
    assert (x != y).sum() > 100000 and (x == y).sum() > 100000


# ---------------------------------------------------------------------------------------------------------------------
def test_canon_eval_refuses_bad_calls_before_any_launch():
    from onset_fingerprinting_amd import _lib
    L = _lib.lib()
    buf = (ctypes.c_float * 4)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    for args, word in (((7, p, p, 4, 0.0, 0.0, 0.0, p, None), "unknown op"),
                       ((-1, p, p, 4, 0.0, 0.0, 0.0, p, None), "unknown op"),
                       ((0, p, None, -1, 0.0, 0.0, 0.0, p, None), "negative n"),
                       ((0, None, None, 4, 0.0, 0.0, 0.0, p, None), "NULL"),
                       ((0, p, None, 4, 0.0, 0.0, 0.0, None, None), "NULL"),
                       ((4, p, None, 4, 0.5, 0.5, 0.0, p, None), "second operand"),
                       ((6, p, None, 4, 0.5, 0.0, 0.0, p, None), "second operand")):
        assert L.ofp_canon_eval(*args) != 0
        assert word in _lib.last_error(), (args, _lib.last_error())
    # n = 0 is a call that does nothing: no array is looked at, nothing is launched
    assert L.ofp_canon_eval(0, None, None, 0, 0.0, 0.0, 0.0, None, None) == 0


@pytest.mark.parametrize("floor", [1e-30, 70.0, float("inf"), float("nan")])
def test_detector_create_refuses_a_positive_or_nan_floor(floor):
    """rel.clip(0, -floor) (detection.py:754) with floor > 0: numpy returns the upper bound, the NEGATIVE constant -floor,
    for every value; with a NaN floor every value is NaN.  No onset follows from either and the block extremes of the
    back-to-linear pass assume clipped, non-negative values: such a floor is refused, before any HIP call."""
    from onset_fingerprinting_amd import _lib
    from onset_fingerprinting_amd.detection import _detector_params
    p, on, off = _detector_params(3, 64, floor, 2000.0, (3.0, 383.0), (2205.0, 2205.0), 0.5, 0.1, 1323, False, 128, 5, 48000)
    h = ctypes.c_void_p()
    dp = ctypes.POINTER(ctypes.c_double)
    status = _lib.lib().ofp_detector_create(ctypes.byref(p), on.ctypes.data_as(dp), off.ctypes.data_as(dp), ctypes.byref(h))
    assert status != 0 and h.value is None and "floor_db" in _lib.last_error()
    with np.errstate(all="ignore"):  # what the reference's expression gives: why there is nothing to reproduce
        r = (np.float32(10) ** (np.float32([-5.0, 0.0, 5.0]) / 20) - 1e-10).clip(0, np.float32(-floor))
    assert np.all(np.isnan(r)) if np.isnan(floor) else np.all(r == np.float32(-floor))


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", vd.ALL_CASES, ids=vd.case_ids(vd.ALL_CASES))
def test_value_class_reaches_what_it_claims(case):
    name, i = case
    x = vd.class_input(name)
    assert x.shape == (72000, 4 if name in vd.WIDE else 3) and x.dtype == np.float32 and np.all(np.isfinite(x))
    ch, on, rel = vd.oracle_batch(name, i)
    claim = vd.CLASSES[name][2]
    assert not np.isnan(rel).any()
    if claim is None:
        return
    kind, least = claim
    print(name, vd.class_kw(name, i), "onsets", len(on), "distinct rel", len(np.unique(vd.bits(rel))))
    if kind == "onsets":
        assert len(on) >= least
    elif kind == "distinct":
        assert len(on) == 0 and len(np.unique(vd.bits(rel))) >= least
    else:
        # every sample vanishes against 1e-10f: the dB stream is the one value 20 * log10(1e-10f), the followers climb to it
        # from the floor, and `rel` settles where their fp32 steps stall (about 1.0019, not exactly 1)
        import oracle as o
        _, _, silent = o.OracleDetector(vd.C, vd.B, sr=vd.SR, **vd.class_kw(name, i)).detect(np.zeros_like(x), vd.WARM)
        assert len(on) == 0 and np.array_equal(vd.bits(rel), vd.bits(silent))
        assert len(np.unique(vd.bits(rel[-4800:]))) == 1 and abs(float(rel[-1, 0]) - 1.0) < 0.01


def test_value_class_inputs_hold_the_values_they_are_named_for():
    g0, gm0, cancel = vd.class_input("gapped0"), vd.class_input("gapped-0"), vd.class_input("cancel")
    gaps = ~vd.hit_mask()
    assert gaps.sum() == 144000
    assert np.all(vd.bits(g0)[gaps] == 0) and np.all(vd.bits(gm0)[gaps] == 0x80000000)
    assert np.all(cancel[gaps] + np.float32(1e-10) == 0) and (cancel + np.float32(1e-10) == 0).sum() == 144000
    flat = vd.class_input("tiny-flat")
    assert ((flat != 0) & (np.abs(flat) < np.float32(1.1754944e-38))).sum() >= 92000
    huge = vd.class_input("huge-hpoff")
    assert np.abs(huge).max() == np.float32(3.4e38)
    # cancel at floor -1000: rel spans the whole clip range 0 .. 1000
    _, _, rel = vd.oracle_batch("cancel", 2)
    assert rel.min() == 0.0 and rel.max() == 1000.0
    _, _, rel = vd.oracle_batch("huge-hpoff", 1)
    assert rel.max() == 1000.0


# ---------------------------------------------------------------------------------------------------------------------
def test_non_finite_cases_on_the_oracle():
    """What the GPU tests of the non-finite samples rely on: the bad sample makes channel 1 NaN from its row (the overflow:
    within eight rows) to the end, channels 0 and 2 keep every bit of the clean run, and 16 to 24 of the clean run's 24 onsets
    remain."""
    clean = vd.nonfinite_oracle("clean", None)
    assert len(clean[2]) == 24 and not np.isnan(clean[3]).any()
    rows = vd.nonfinite_rows()
    assert rows["warm"] < vd.N_WB and all(0 <= r < 72000 for r in rows.values())
    for value, row in vd.NONFINITE_CASES:
        x, ch, on, rel = vd.nonfinite_oracle(value, row)
        assert (~np.isfinite(x)).sum() == (0 if value == "overflow" else 1)
        if value != "overflow":
            assert vd.bits(x)[rows[row], vd.BAD_CHANNEL] == vd.NONFINITE[value]
        nan = np.isnan(rel[:, vd.BAD_CHANNEL])
        first = int(np.argmax(nan))
        # (a sample inside the warm-up has made the filter state NaN before the first block)
        want_first = 0 if rows[row] < vd.WARM else min(rows[row], 72000 - 8) if value == "overflow" else rows[row]
        assert nan.any() and nan[first:].all() and want_first <= first <= want_first + 8, (value, row, first)
        assert vd.nonfinite_mismatch(rel, rel) is None
        assert 16 <= len(on) <= 24 and set(ch[on >= first + 2000].tolist()) <= {0, 2}, (value, row, len(on))
