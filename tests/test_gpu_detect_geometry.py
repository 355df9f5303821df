"""The detector on both sides of every layout guard (tests/detect_geometry_cases.py): for every row of the table the plan
the detector reports (ofp_detect_plan_query) equals the restatement evaluated with the device's CU count, and the records
and every bit of `rel` equal the C oracle's run with the same warm-up.  Where a fast form of the row has a slow twin
(tuning line_stores, interleaved, walk_through, scan_skip, fuse_db_sums = -1) the twin gives the same bits.  For the rows
about the followers' interleaved stores the work space is filled with a byte pattern first: only that form leaves a stretch
as long as the planar `dif` array untouched (tests/test_gpu_rel_il_stores_small.py), and that observation must agree with
the plan's bit.

Everything is an equality.  tests/test_detect_geometry_cpu.py checks the table itself without a GPU."""
import numpy as np
import pytest
import torch

import oracle
from onset_fingerprinting_amd.detection import BatchDetector
from tests import detect_geometry_cases as cases
from tests.detect_geometry_cases import bits

pytestmark = pytest.mark.gpu

FILL = 0xA5
ROWS = cases.ROWS
# the tuning field that switches the row's subject to its slow twin
TWIN_OF = dict(hp_lines="line_stores", ar_lines="line_stores", ar_il="interleaved", mm_il="interleaved",
               ar_through="walk_through", mm_through="walk_through", use_sum="scan_skip", db_sym="fuse_db_sums")

_detectors, _oracle, _runs = {}, {}, {}


def detector(row):
    """One BatchDetector per (C, B, detector arguments)."""
    key = (row["C"], row["B"], repr(row.get("kw", {})))
    if key not in _detectors:
        _detectors[key] = BatchDetector(row["C"], row["B"], sr=cases.SR, device=0, **row.get("kw", {}))
    return _detectors[key]


def reference(row):
    """(x [clips][N][C], per clip (channels, samples, rel)) of the oracle, once per input and detector."""
    key = (row["C"], row["B"], row["N"], row["warm"], row.get("clips", 1), row.get("seed", 7), repr(row.get("kw", {})))
    if key not in _oracle:
        x = cases.make_input(row)
        per_clip = []
        for xc in x:
            c, o, rel = oracle.OracleDetector(row["C"], row["B"], sr=cases.SR, **row.get("kw", {})).detect(xc, row["warm"])
            per_clip.append((np.array(c, np.int64), np.array(o, np.int64), rel))
        _oracle[key] = (x, per_clip)
    return _oracle[key]


def untouched_run(ws):
    """Longest stretch of bytes of the work space that still hold the fill pattern."""
    changed = torch.nonzero(ws != FILL).flatten()
    edges = torch.cat([torch.tensor([-1], device=ws.device), changed, torch.tensor([ws.numel()], device=ws.device)])
    return int((edges[1:] - edges[:-1] - 1).max())


def run(row, tuning):
    """The row's call under `tuning`, once: (records, rel, plan, longest untouched stretch of the filled work space)."""
    key = (row["C"], row["B"], row["N"], row["warm"], row.get("clips", 1), row.get("seed", 7), repr(row.get("kw", {})),
           row.get("rel", True), row.get("x_off", 0), row.get("rel_off", 0), tuple(sorted(tuning.items())))
    if key not in _runs:
        x, _ = reference(row)
        bd = detector(row)
        bd.set_tuning(**tuning)
        recs, rel, plan, ws = cases.gpu_detect(bd, x, row["warm"], row.get("x_off", 0), row.get("rel_off", 0),
                                               row.get("rel", True), fill=FILL)
        _runs[key] = (recs, rel, plan, untouched_run(ws))
    return _runs[key]


def twins(row, n_cus):
    """The tunings of the row's slow twins: its subject's own switch, and all five switches at once, where they change
    the plan."""
    plan = cases.restate_row(row, n_cus)[0]
    found = []
    own = TWIN_OF.get(row["flag"])
    for off in ([{own: -1}] if own else []) + [{k: -1 for k in cases.TWINS}]:
        t = dict(row["tuning"], **off)
        if t != row["tuning"] and cases.restate_row(dict(row, tuning=t), n_cus)[0] != plan and t not in found:
            found.append(t)
    return found


@pytest.mark.parametrize("row", ROWS, ids=[r["name"] for r in ROWS])
def test_row(row):
    n_cus = torch.cuda.get_device_properties(0).multi_processor_count
    x, per_clip = reference(row)
    want_plan = cases.restate_row(row, n_cus)[0]
    recs, rel, plan, run_bytes = run(row, row["tuning"])
    assert plan == want_plan, {k: (plan[k], want_plan[k]) for k in plan if plan[k] != want_plan[k]}
    if row["flag"]:
        assert plan[row["flag"]] == (row["side"] == "on")
    dif_bytes = row.get("clips", 1) * row["C"] * plan["U"] * 4
    if row["flag"] == "ar_il":
        assert (run_bytes >= dif_bytes) == bool(plan["ar_il"]), (run_bytes, dif_bytes, "the planar `dif` array is written "
                                                                "by the planar form only")
    for i, (c, o, orel) in enumerate(per_clip):
        assert np.array_equal(recs[i]["channel"], c) and np.array_equal(recs[i]["sample"], o), (row["name"], i, "records")
        if rel is not None:
            assert cases.same_as_oracle(rel[i], orel), (row["name"], i, "relative envelope not bit-identical to the oracle's")
    for t in twins(row, n_cus):
        trecs, trel, tplan, trun = run(row, t)
        assert tplan == cases.restate_row(dict(row, tuning=t), n_cus)[0], t
        if row["flag"] == "ar_il":
            assert (trun >= dif_bytes) == bool(tplan["ar_il"]), (t, trun, dif_bytes)
        for a, b in zip(recs, trecs):
            assert np.array_equal(a, b), (row["name"], t, "records of the two forms differ")
        if rel is not None:
            assert np.array_equal(bits(rel), bits(trel)), (row["name"], t, "the two forms differ")
