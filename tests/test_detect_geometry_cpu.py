"""The detector's layout guards without a GPU: make_layout (through the plan query ofp_detect_plan_for, which launches
nothing) against its restatement in tests/detect_geometry_cases.py, on every row of the case table and on a small
exhaustive sweep; the table's own claims (which conjuncts fail on a row, an on row and an off row for every conjunct of
every flag, no off row that fails more conjuncts than it has to); and, with the oracle alone, that every row has onsets
where they decide something."""
import ctypes
import time

import numpy as np
import pytest

from tests import detect_geometry_cases as cases
import oracle
from onset_fingerprinting_amd import _lib, detection

N_CUS = 256
ROWS = cases.ROWS
IDS = [r["name"] for r in ROWS]


def query(row, n_cus=N_CUS):
    return detection.detect_plan(row["C"], row.get("clips", 1), row["N"], block_size=row["B"], sr=cases.SR,
                                 warm=row["warm"], want_rel=row.get("rel", True), rel_aligned=row.get("rel_off", 0) == 0,
                                 tuning=row["tuning"], n_cus=n_cus, **row.get("kw", {}))


def test_the_query_reports_every_field_the_table_names():
    assert [n for n, _ in _lib.DetectPlan._fields_] == list(cases.GEOMETRY + cases.NUMBERS + cases.BITS)
    assert len(set(IDS)) == len(IDS)


@pytest.mark.parametrize("row", ROWS, ids=IDS)
def test_restatement_equals_the_plan_query(row):
    for n_cus in (N_CUS, 32):
        want, (got, _) = query(row, n_cus), cases.restate_row(row, n_cus)
        assert got == want, (row["name"], n_cus, {k: (got[k], want[k]) for k in want if got[k] != want[k]})


@pytest.mark.parametrize("row", [r for r in ROWS if r["flag"]], ids=[r["name"] for r in ROWS if r["flag"]])
def test_recorded_failing_conjuncts_are_the_ones_that_fail(row):
    plan = query(row)
    assert cases.failing(row) == row["fails"], row["name"]
    assert plan[row["flag"]] == (1 if row["side"] == "on" else 0), row["name"]
    assert (row["side"] == "on") == (row["fails"] == []), row["name"]
    if row["conjunct"] is not None:
        assert row["side"] == "off" and row["conjunct"] in row["fails"], row["name"]


def test_every_conjunct_of_every_flag_has_an_on_row_and_an_off_row():
    _, conj = cases.restate_row(ROWS[0])
    missing = []
    for flag, cs in conj.items():
        if not any(r["flag"] == flag and r["side"] == "on" for r in ROWS):
            missing.append((flag, "on"))
        for c in cs:
            if (flag, c) in cases.IMPLIED:
                continue
            if not any(r["flag"] == flag and r["side"] == "off" and r["conjunct"] == c for r in ROWS):
                missing.append((flag, c, "off"))
    assert not missing, missing
    for flag, c in cases.IMPLIED:
        assert c in conj[flag], (flag, c)
    # every variant bit of the plan that a guard decides is a flag of the table
    assert set(conj) == {"hp_lines", "ar_through", "ar_lines", "db_sym", "mm_il", "mm_through", "ar_il", "use_sum",
                         "hp_early", "sm_seg"}


@pytest.mark.parametrize("row", [r for r in ROWS if r["conjunct"]], ids=[r["name"] for r in ROWS if r["conjunct"]])
def test_an_off_row_fails_no_more_conjuncts_than_arithmetic_forces(row):
    fewest, call = cases.fewest_failing(row)
    assert fewest is None or len(row["fails"]) <= fewest, (row["name"], row["fails"], fewest, call)


_oracle = {}


def oracle_onsets(row):
    key = (row["C"], row["B"], row["N"], row["warm"], row.get("clips", 1), row.get("seed", 7), repr(row.get("kw", {})))
    if key not in _oracle:
        _oracle[key] = [oracle.OracleDetector(row["C"], row["B"], sr=cases.SR, **row.get("kw", {})).detect(xc, row["warm"])[1]
                        for xc in cases.make_input(row)]
    return _oracle[key]


@pytest.mark.parametrize("row", ROWS, ids=IDS)
def test_every_row_has_onsets_and_one_soon_after_the_warm_up(row):
    """No record is decided by luck: at least 4 onsets per clip, one of them within two IIR chunks of the restart."""
    hp_L = cases.restate_row(row)[0]["hp_L"]
    for on in oracle_onsets(row):
        assert len(on) >= 4, (row["name"], len(on))
        assert np.sum(np.asarray(on) < 2 * hp_L) >= 1, (row["name"], list(on)[:4], hp_L)


def test_the_random_geometries_have_onsets():
    """tests/test_gpu_fuzz.py::test_random_geometries_match_the_oracle asserts the same sum on the GPU."""
    rng = np.random.default_rng(cases.FUZZ_SEED)
    n = 0
    for _ in range(cases.FUZZ_CASES):
        case = cases.random_geometry_case(rng)
        x = cases.make_input(case)[0]
        n += len(oracle.OracleDetector(case["C"], case["B"], sr=cases.SR).detect(x, cases.fuzz_warm(case))[1])
    assert n > 3 * cases.FUZZ_CASES, n


PLAN_DTYPE = np.dtype([(n, "i8" if c is ctypes.c_int64 else "i4") for n, c in _lib.DetectPlan._fields_])


def test_sweep_of_block_sizes_and_warm_ups():
    """B in 8..130, warm in 0..130 and 4096..4140, N in {40 B, 40 B + 1, 41 B - 1}, C in {1, 2, 3, 4, 5, 8, 64} and the
    table's three tunings: the restatement (elementwise on arrays) against one query per call.  The conjuncts listed as
    IMPLIED never fail while the others of their flag hold."""
    t0 = time.perf_counter()
    Bs = np.arange(8, 131, dtype=np.int64)
    warms = np.concatenate([np.arange(0, 131), np.arange(4096, 4141)]).astype(np.int64)
    B, warm, k = [a.ravel() for a in np.meshgrid(Bs, warms, np.arange(3), indexing="ij")]
    N = np.where(k == 0, 40 * B, np.where(k == 1, 40 * B + 1, 41 * B - 1))
    fn = _lib.lib().ofp_detect_plan_for
    plans = (_lib.DetectPlan * len(B))()
    got = np.frombuffer(plans, dtype=PLAN_DTYPE)
    calls = list(zip(N.tolist(), warm.tolist(), plans))
    for C in (1, 2, 3, 4, 5, 8, 64):
        params = {int(b): detection._detector_params(C, int(b), -70.0, 2000.0, (3.0, 383.0), (2205.0, 2205.0), 0.5, 0.1,
                                                     1323, False, 128, 5, cases.SR)[0] for b in Bs}
        refs = [ctypes.byref(params[b]) for b in B.tolist()]
        for name, tuning in cases.TUNINGS.items():
            t = ctypes.byref(detection._tuning(tuning))
            for p, (n, w, out) in zip(refs, calls):
                fn(p, t, N_CUS, 1, n, w, 1, None, out)
            want, conj = cases.restate_plan(dict(n_signals=C, block_size=B, sr=cases.SR), tuning, N_CUS, 1, N, warm, True, True)
            for f in PLAN_DTYPE.names:
                bad = np.nonzero(got[f] != want[f])[0]
                assert len(bad) == 0, (f, name, C, int(B[bad[0]]), int(warm[bad[0]]), int(N[bad[0]]),
                                       int(got[f][bad[0]]), int(want[f][bad[0]]))
            for flag, c in cases.IMPLIED:
                others = np.logical_and.reduce([v for k2, v in conj[flag].items() if k2 != c and (flag, k2) not in cases.IMPLIED])
                assert not np.any(others & ~conj[flag][c]), (flag, c, name, C)
    print(f"{7 * 3 * len(B)} plans in {time.perf_counter() - t0:.1f} s")
