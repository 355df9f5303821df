"""The detector, the stream kernels and the hop session on value classes of audio (tests/value_domain_cases.py): exact zeros
of both signs, samples that cancel against 1e-10f, audio of 1e-9 and of subnormal size, audio near FLT_MAX, and floors from
0 to -1000 -- where the dB pass sees log10 of tiny and cancelled arguments and the back-to-linear pass sees exp10 up to its
cut-offs.  Every path gives the oracle's records index for index and every bit of its `rel`.

tests/test_value_domain_cpu.py shows on the oracle alone that each class reaches what it is there for."""
import numpy as np
import pytest
import torch

from onset_fingerprinting_amd import detection
from tests import value_domain_cases as vd
from tests.detect_geometry_cases import LINES, gpu_detect

pytestmark = pytest.mark.gpu

# the batch detector's tunings: the default; many chunks per stage (the states at the extremes cross chunk boundaries and the
# repair passes run); the host-verified passes; and the slow twins of the interleaved tracker and of the block extremes
TUNINGS = {"default": {}, "chunks": dict(hp_chunk=1024, ar_chunk=512, mm_chunk=1024), "host_verify": dict(host_verify=1),
           "planar": dict(interleaved=-1), "no_extremes": dict(scan_skip=-1)}
WIDE_TUNINGS = {"lines": LINES, "lines_planar": dict(LINES, interleaved=-1), "default": {}}
N = 72000


def same_bits(got, want):
    return got.shape == want.shape and np.array_equal(vd.bits(got), vd.bits(want))


def batch_detector(name, i):
    return detection.BatchDetector(vd.class_input(name).shape[1], vd.B, sr=vd.SR, device=0, **vd.class_kw(name, i))


def check_batch(name, i, tunings):
    ch, on, rel = vd.oracle_batch(name, i)
    assert not np.isnan(rel).any()
    x = np.array(vd.class_input(name))[None]
    bd = batch_detector(name, i)
    plans = {}
    for tname, tuning in tunings.items():
        bd.set_tuning(**tuning)
        recs, grel, plan, _ = gpu_detect(bd, x, vd.case_warm(name))
        plans[tname] = plan
        assert np.array_equal(recs[0]["channel"], ch) and np.array_equal(recs[0]["sample"], on), (name, i, tname, "records")
        assert same_bits(grel[0], rel), (name, i, tname, int((vd.bits(grel[0]) != vd.bits(rel)).sum()), "values of rel differ")
    return plans


@pytest.mark.parametrize("case", vd.CASES, ids=vd.case_ids(vd.CASES))
def test_detect_batch_on_a_value_class(case):
    plans = check_batch(*case, TUNINGS)
    kw = vd.class_kw(*case)
    assert plans["default"]["use_sum"] == 1 and plans["no_extremes"]["use_sum"] == 0
    assert plans["default"]["db_sym"] == int(kw.get("hipass_freq", 2000.0) != 0)
    assert plans["chunks"]["hp_L"] == 1024 and plans["chunks"]["ar_L"] == 512 and plans["chunks"]["mm_L"] == 1024
    assert all(p["ar_il"] == 0 for p in plans.values())  # (three channels: see the four-channel classes)


@pytest.mark.parametrize("case", vd.WIDE_CASES, ids=vd.case_ids(vd.WIDE_CASES))
def test_detect_batch_with_the_followers_interleaved_stores(case):
    plans = check_batch(*case, WIDE_TUNINGS)
    assert plans["lines"]["ar_il"] == 1 and plans["lines"]["mm_il"] == 1
    assert plans["lines_planar"]["ar_il"] == 0 and plans["lines_planar"]["mm_il"] == 0


def test_plan_bits_are_seen_from_both_sides():
    """use_sum, db_sym and ar_il are each 1 in one case of this file and 0 in another (the plan query launches nothing)."""
    seen = {k: set() for k in ("use_sum", "db_sym", "ar_il")}
    for cases, tunings in ((vd.CASES, TUNINGS), (vd.WIDE_CASES, WIDE_TUNINGS)):
        for name, i in cases:
            bd = batch_detector(name, i)
            rel = torch.empty((1, N, bd.n_signals), dtype=torch.float32, device="cuda")
            for tuning in tunings.values():
                bd.set_tuning(**tuning)
                plan = bd.plan(1, N, vd.case_warm(name), True, rel)
                for k in seen:
                    seen[k].add(plan[k])
    assert all(v == {0, 1} for v in seen.values()), seen


@pytest.mark.parametrize("kernel", ["par", "seq"])
@pytest.mark.parametrize("case", vd.CASES, ids=vd.case_ids(vd.CASES))
def test_stream_detector_on_a_value_class(case, kernel, monkeypatch):
    """AmplitudeOnsetDetector over the stream in calls of 1, 7 and the remaining blocks, under the default kernel choice
    (k_stream_par at this shape) and under OFP_STREAM_KERNEL=seq (k_stream)."""
    name, i = case
    if kernel == "seq":
        monkeypatch.setenv("OFP_STREAM_KERNEL", "seq")
    else:
        monkeypatch.delenv("OFP_STREAM_KERNEL", raising=False)
    ch, on, rel = vd.oracle_batch(name, i)
    x = np.array(vd.class_input(name))
    C, B, nb = x.shape[1], vd.B, N // vd.B
    od = detection.AmplitudeOnsetDetector(C, B, sr=vd.SR, **vd.class_kw(name, i))
    od.init_minmax_tracker(x[:vd.WARM])
    xd = torch.from_numpy(x).cuda()
    grel = torch.empty((nb * B, C), dtype=torch.float32, device="cuda")
    rec = torch.zeros((len(on) + 64, 16), dtype=torch.uint8, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    k = 0
    for n in (1, 7, nb - 8):
        od.process(xd[k * B:(k + n) * B], n, k * B, grel[k * B:(k + n) * B], rec, cnt)
        k += n
    torch.cuda.synchronize()
    count = int(cnt.item())
    recs = rec.cpu().numpy().view(detection.ONSET_DTYPE).reshape(-1)
    assert count == len(on), (count, len(on))
    assert np.array_equal(recs["channel"][:count], ch) and np.array_equal(recs["sample"][:count], on)
    assert same_bits(grel.cpu().numpy(), rel), int((vd.bits(grel.cpu().numpy()) != vd.bits(rel)).sum())


@pytest.mark.parametrize("graph", ["fused", "nodes"])
@pytest.mark.parametrize("case", vd.CASES, ids=vd.case_ids(vd.CASES))
def test_hop_session_detector_outputs_on_a_value_class(case, graph, monkeypatch):
    """realtime.HopSession hop by hop, as one fused kernel and as the five-node graph: channels, absolute onsets and `rel`
    (the spectral outputs are not the subject here)."""
    from onset_fingerprinting_amd import realtime
    from tests.test_gpu_stream_shapes import session_form
    name, i = case
    if graph == "nodes":
        monkeypatch.setenv("OFP_HOP_GRAPH", "nodes")
    else:
        monkeypatch.delenv("OFP_HOP_GRAPH", raising=False)
    ch, on, rel = vd.oracle_batch(name, i)
    x = np.array(vd.class_input(name))
    C, B, nb = x.shape[1], vd.B, N // vd.B
    sess = realtime.HopSession(C, B, sr=vd.SR, n_fft=256, n_mels=20, want_rel=True, ring_seconds=0.1, **vd.class_kw(name, i))
    assert session_form(sess) == graph
    sess.init_minmax_tracker(x[:vd.WARM])
    got_ch, got_on = [], []
    grel = np.empty((nb * B, C), np.float32)
    for h in range(nb):
        r = sess(x[h * B:(h + 1) * B])
        got_ch += [int(v) for v in r["channels"]]
        got_on += [int(v) for v in r["onsets"]]
        grel[h * B:(h + 1) * B] = r["rel"]
    sess.close()
    assert got_ch == ch.tolist() and got_on == on.tolist()
    assert same_bits(grel, rel), int((vd.bits(grel) != vd.bits(rel)).sum())


# ---- non-finite samples ------------------------------------------------------------------------------------------------
# DESIGN.md ("Value-domain tests") says for every loop of these paths that waits for convergence why it ends whatever the
# values are: the states it compares are compared as bit patterns.

_shared = {}


def shared_batch_detector():
    """ONE detector and work space for every non-finite batch case: a later call finds the earlier calls' NaN states in the
    slots it marks empty."""
    if "bd" not in _shared:
        _shared["bd"] = detection.BatchDetector(vd.C, vd.B, sr=vd.SR, device=0)
    return _shared["bd"]


def check_nonfinite(what, recs_ch, recs_on, grel, value, row):
    _, ch, on, rel = vd.nonfinite_oracle(value, row)
    assert np.array_equal(recs_ch, ch) and np.array_equal(recs_on, on), (what, value, row, "records")
    assert vd.nonfinite_mismatch(grel, rel) is None, (what, value, row, vd.nonfinite_mismatch(grel, rel))


@pytest.mark.parametrize("case", vd.NONFINITE_CASES, ids=[f"{v}-{r}" for v, r in vd.NONFINITE_CASES])
def test_detect_batch_with_a_non_finite_sample(case):
    value, row = case
    x = vd.nonfinite_oracle(value, row)[0][None]
    bd = shared_batch_detector()
    for tname, tuning in (("default", {}), ("chunks", vd.CHUNKS), ("host_verify", dict(vd.CHUNKS, host_verify=1))):
        bd.set_tuning(**tuning)
        recs, grel, plan, _ = gpu_detect(bd, x, vd.WARM)
        if tname != "default":
            assert (plan["hp_L"], plan["ar_L"], plan["mm_L"]) == (1024, 512, 1024) and (plan["n_w"], plan["n_wb"]) == (vd.N_W, vd.N_WB)
        check_nonfinite(tname, recs[0]["channel"], recs[0]["sample"], grel[0], value, row)


def test_detect_batch_with_floor_minus_infinity():
    """floor = -inf (what k_calibrate passes to the dB pass) as the detector's own floor: the followers start at -inf, their
    first step is -inf + coefficient * inf = NaN, and `rel` is NaN throughout -- on the oracle and on the device alike."""
    import oracle
    x = np.array(vd.class_input("gapped0"))
    with np.errstate(all="ignore"):
        ch, on, rel = oracle.OracleDetector(vd.C, vd.B, sr=vd.SR, floor=-np.inf).detect(x, vd.WARM)
    assert len(on) == 0 and np.isnan(rel).all()
    bd = detection.BatchDetector(vd.C, vd.B, sr=vd.SR, device=0, floor=-np.inf)
    for tuning in ({}, vd.CHUNKS):
        bd.set_tuning(**tuning)
        recs, grel, _, _ = gpu_detect(bd, x[None], vd.WARM)
        assert len(recs[0]) == 0 and np.isnan(grel[0]).all()


STREAM_NONFINITE = [(v, r) for v, r in vd.NONFINITE_CASES if r in vd.STREAM_ROWS]


@pytest.mark.parametrize("kernel", ["par", "seq"])
@pytest.mark.parametrize("case", STREAM_NONFINITE, ids=[f"{v}-{r}" for v, r in STREAM_NONFINITE])
def test_stream_detector_with_a_non_finite_sample(case, kernel, monkeypatch):
    value, row = case
    if kernel == "seq":
        monkeypatch.setenv("OFP_STREAM_KERNEL", "seq")
    else:
        monkeypatch.delenv("OFP_STREAM_KERNEL", raising=False)
    x, _, on, _ = vd.nonfinite_oracle(value, row)
    C, B, nb = vd.C, vd.B, N // vd.B
    od = detection.AmplitudeOnsetDetector(C, B, sr=vd.SR)
    od.init_minmax_tracker(x[:vd.WARM])
    xd = torch.from_numpy(x).cuda()
    grel = torch.empty((nb * B, C), dtype=torch.float32, device="cuda")
    rec = torch.zeros((len(on) + 64, 16), dtype=torch.uint8, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    k = 0
    for n in (1, 7, nb - 8):
        od.process(xd[k * B:(k + n) * B], n, k * B, grel[k * B:(k + n) * B], rec, cnt)
        k += n
    torch.cuda.synchronize()
    count = int(cnt.item())
    assert count <= len(on) + 64
    recs = rec.cpu().numpy().view(detection.ONSET_DTYPE).reshape(-1)[:count]
    check_nonfinite(kernel, recs["channel"], recs["sample"], grel.cpu().numpy(), value, row)


@pytest.mark.parametrize("graph", ["fused", "nodes"])
@pytest.mark.parametrize("case", STREAM_NONFINITE, ids=[f"{v}-{r}" for v, r in STREAM_NONFINITE])
def test_hop_session_with_a_non_finite_sample(case, graph, monkeypatch):
    from onset_fingerprinting_amd import realtime
    value, row = case
    if graph == "nodes":
        monkeypatch.setenv("OFP_HOP_GRAPH", "nodes")
    else:
        monkeypatch.delenv("OFP_HOP_GRAPH", raising=False)
    x = vd.nonfinite_oracle(value, row)[0]
    C, B, nb = vd.C, vd.B, N // vd.B
    sess = realtime.HopSession(C, B, sr=vd.SR, n_fft=256, n_mels=20, want_rel=True, ring_seconds=0.1)
    sess.init_minmax_tracker(x[:vd.WARM])
    got_ch, got_on = [], []
    grel = np.empty((nb * B, C), np.float32)
    for h in range(nb):
        r = sess(x[h * B:(h + 1) * B])
        got_ch += [int(v) for v in r["channels"]]
        got_on += [int(v) for v in r["onsets"]]
        grel[h * B:(h + 1) * B] = r["rel"]
    sess.close()
    check_nonfinite(graph, np.array(got_ch, np.int64), np.array(got_on, np.int64), grel, value, row)
