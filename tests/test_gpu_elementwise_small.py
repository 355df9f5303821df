"""The dB pass and the back-to-linear pass (k_rect_db_sym, k_rect_db, k_rel_out, k_rel_out_il<4/8>) at the smallest shapes
at which each of their paths can go wrong, through BatchDetector.detect against the oracle.

All four read the canon's tables from a copy in LDS that the workgroup fills before anything else (csrc/ofp_canon_dev.h), and
walk their trips with the next trip's loads issued early (stream_trips).  What can go wrong is therefore a matter of shape:
  * k_rect_db_sym: four waves per workgroup, one (chain, follower chunk) each -- a last workgroup with idle waves (they
    must pass the fill's barrier and leave); chunks of several full trips (256 16-byte groups each), of full trips and a
    tail, and of a tail alone;
  * k_rect_db: in place (asymmetric slow follower: no closed-form guess, so no fused pass) with one trip per thread, with
    two (more than 4096 x 256 groups) and with values left over after the 16-byte groups; from the audio itself (no
    high-pass), one and two trips per thread;
  * k_rel_out: the 16-byte branch with its four-group trips (16 channels) and with single groups (3 channels), and the
    scalar branch (U no multiple of 4);
  * k_rel_out_il<8> and <4>: blocks of a tail alone, of one full trip, of two, and of a full trip and a tail.
Each case asserts from BatchDetector.plan (and the kernels' own conditions restated on its numbers) that the intended
variant is the one that ran.  Sizes come from the plan, not from the workload: the first case searches the smallest
n_samples for which the plan reports db_sym and ar_il.

Inputs: the drum-hit synthesiser at gains 1, 1e-3 and 1e3, and a clip with a stretch of silence and -inf, +inf and NaN
samples in channel 1; two sets of clips per case so that every case sees all four.  Records must be equal and `rel` is
compared as uint32 bits; where the oracle's value is a NaN the detector's must be a NaN (sign and payload of a NaN that
arithmetic produces are the processor's choice and differ between x86 and the GPU: see tests/test_gpu_rel_il_stores_small.py)."""
import numpy as np
import pytest
import torch

import oracle
from onset_fingerprinting_amd import synth
from onset_fingerprinting_amd.detection import BatchDetector

pytestmark = pytest.mark.gpu

SR = 48000
KINDS = ("g1", "g1e-3", "g1e3", "special")
GAIN = {"g1": 1.0, "g1e-3": 1e-3, "g1e3": 1e3, "special": 1.0}
THROUGHPUT = dict(lane_merge=1, hp_dedupe=1)
ASYM = dict(slow_ar=(2205.0, 1000.0))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def clip(kind, C, N, seed):
    x = synth.drum_hits(C, N / SR + 0.05, SR, seed=seed, period=0.11, gain=GAIN[kind])[:N].copy()
    assert x.shape == (N, C) and x.dtype == np.float32
    if kind == "special":
        x[N // 8:N // 4] = 0.0
        x[(N * 7) // 20, 1] = -np.inf
        x[(N * 9) // 20, 1] = np.inf
        x[(N * 11) // 20, 1] = np.nan
    return x


_ref = {}


def reference(key, C, N, B, warm, start, n_clips, kw):
    """(x [clips][N][C], per clip (channels, samples, rel)) of the oracle, once per case and clip set."""
    if key not in _ref:
        x = np.stack([clip(KINDS[(start + i) % 4], C, N, 100 * start + i + 1) for i in range(n_clips)])
        per_clip = []
        with np.errstate(all="ignore"):
            for xc in x:
                c, o, rel = oracle.OracleDetector(C, B, sr=SR, **kw).detect(xc, warm)
                per_clip.append((np.array(c, np.int64), np.array(o, np.int64), rel))
        x.setflags(write=False)
        _ref[key] = (x, per_clip)
    return _ref[key]


def variant(plan, C, B, kw):
    """Which kernels a call with this plan launches and which of their branches its shape takes (decibels() and rel_out()
    of csrc/ofp_detect.hip, and the kernels' own conditions)."""
    U, tu, n_wb, Nm = plan["U"], plan["tu"], plan["n_wb"], plan["Nm"]
    v = {"db": "sym" if plan["db_sym"] else ("in_place" if kw.get("hipass_freq", 2000.0) > 0 else "from_x"),
         "rel": "il" if plan["ar_il"] else "tile"}
    if v["db"] == "sym":
        L = plan["ar_L"]
        v["chunks"] = -(-U // L)
        v["db_groups"] = sorted({min(L, U - j * L) // 4 for j in range(v["chunks"])})  # 16-byte groups per chunk
    if v["rel"] == "tile":
        last = U % tu
        v["vec"] = [U % 4 == 0 and tu % 4 == 0 and nt % 4 == 0 and (n_wb * C) % 4 == 0 and (tu * C) % 4 == 0 and (Nm * C) % 4 == 0
                    for nt in ([tu] if U >= tu else []) + ([last] if last else [])]
        v["rel_groups"] = [nt // 4 * C for nt in ([tu] if U >= tu else []) + ([last] if last else [])]  # per tile
    else:
        v["rel_groups"] = [B * C // 4]  # per block
    return v


def run(name, C, B, warm, N, start, tuning, kw, n_clips=2):
    x, per_clip = reference((name, start), C, N, B, warm, start, n_clips, kw)
    bd = BatchDetector(C, B, device=0, sr=SR, **kw)
    bd.set_tuning(**tuning)
    plan = bd.plan(n_clips, N, warm)
    out = bd.detect(torch.tensor(x).cuda(), warm=warm)
    recs = BatchDetector.records_to_numpy(out)
    rel = out["rel"].cpu().numpy()
    for i, (c, o, orel) in enumerate(per_clip):
        kind = KINDS[(start + i) % 4]
        assert np.array_equal(recs[i]["channel"], c) and np.array_equal(recs[i]["sample"], o), (name, kind, "records")
        assert rel[i].shape == orel.shape
        g, w = bits(rel[i]), bits(orel)
        same = (g == w) | (np.isnan(rel[i]) & np.isnan(orel))
        assert bool(same.all()), (name, kind, f"{int((~same).sum())} values of rel differ from the oracle's bits")
        if kind != "special":
            assert not np.isnan(orel).any()
    return plan, variant(plan, C, B, kw), sum(len(c) for c, _, _ in per_clip)


STARTS = pytest.mark.parametrize("start", [0, 2])  # clips (g1, g1e-3, ..) and (g1e3, special, ..)


@STARTS
@pytest.mark.parametrize("C", [8, 4])
def test_the_smallest_call_that_takes_the_fused_db_pass_and_the_in_place_linear_pass(C, start):
    B, warm = 64, 64
    bd = BatchDetector(C, B, device=0, sr=SR)
    bd.set_tuning(**THROUGHPUT)
    N = next(n for n in range(B, 64 * B) if (lambda p: p["db_sym"] == 1 and p["ar_il"] == 1)(bd.plan(2, n, warm)))
    plan, v, _ = run(f"smallest{C}", C, B, warm, N, start, THROUGHPUT, {})
    assert v["db"] == "sym" and v["rel"] == "il" and v["chunks"] == 1, (N, plan)
    assert v["db_groups"] == [plan["U"] // 4] and plan["U"] // 4 <= 192  # dB pass: a tail alone
    assert v["rel_groups"] == [B * C // 4] and B * C // 4 <= 192  # linear pass: a tail alone


@STARTS
def test_a_last_workgroup_with_idle_waves(start):
    """2 clips x 3 channels x 3 chunks = 18 (chain, chunk) waves: the fifth workgroup of k_rect_db_sym has two waves without
    one.  Chunks of 2 048 steps (512 groups: two full trips) and a last one of 768 (192 groups: a tail alone).  Three
    channels: k_rel_out's 16-byte branch, single groups (192 per tile)."""
    C, B, warm, N = 3, 64, 64, 64 * 75
    plan, v, _ = run("idle", C, B, warm, N, start, dict(THROUGHPUT, ar_chunk=2048), {})
    assert v["db"] == "sym" and (2 * C * v["chunks"]) % 4 == 2 and v["db_groups"] == [192, 512], (plan, v)
    assert v["rel"] == "tile" and all(v["vec"]) and v["rel_groups"] == [192], (plan, v)


@STARTS
def test_chunks_of_full_trips_and_a_tail(start):
    """Chunks of 4 896 steps = 1 224 groups = four full trips, then 200 groups (a fifth full trip for lanes 0..7, three
    single-group trips for the others); a last chunk of 1 792 steps = one full trip and 192 groups."""
    C, B, warm, N = 8, 64, 64, 64 * 180
    plan, v, _ = run("tail", C, B, warm, N, start, dict(THROUGHPUT, ar_chunk=4896), {})
    assert v["db"] == "sym" and v["db_groups"] == [448, 1224], (plan, v)
    assert v["rel"] == "il" and v["rel_groups"] == [128]


@STARTS
@pytest.mark.parametrize("B,trips", [(256, "two full trips"), (160, "one full trip and a tail of 64 groups")])
def test_linear_pass_in_place_with_full_trips(B, trips, start):
    C, warm, N = 8, B, B * 48
    plan, v, _ = run(f"il{B}", C, B, warm, N, start, THROUGHPUT, {})
    assert v["db"] == "sym" and v["rel"] == "il" and v["rel_groups"] == [{256: 512, 160: 320}[B]], (plan, v)


@STARTS
def test_sixteen_channels_take_four_group_trips_of_the_tile_pass(start):
    """16 channels x 256 steps per tile = 1 024 groups: one full trip of k_rel_out's 16-byte branch for every thread; the
    last tile (U = 1 344 = 5 x 256 + 64) has 256 groups: single groups."""
    C, B, warm, N = 16, 64, 64, 64 * 20
    plan, v, _ = run("c16", C, B, warm, N, start, THROUGHPUT, {})
    assert v["db"] == "sym" and v["rel"] == "tile" and all(v["vec"]) and v["rel_groups"] == [1024, 256], (plan, v)


@STARTS
def test_asymmetric_slow_follower_small_and_no_multiple_of_4(start):
    """3 clips x 3 channels x U = 1 650: k_rect_db in place over 14 850 values = 3 712 groups and two values left over;
    U % 4 = 2: k_rel_out's scalar branch."""
    C, B, warm, N = 3, 50, 50, 50 * 32
    plan, v, _ = run("asym_small", C, B, warm, N, start, THROUGHPUT, ASYM, n_clips=3)
    assert plan["ar_sym"] == 0 and v["db"] == "in_place" and plan["U"] == 1650 and (3 * C * plan["U"]) % 4 == 2
    assert v["rel"] == "tile" and not any(v["vec"])


@STARTS
def test_asymmetric_slow_follower_with_two_trips_per_thread(start):
    """8 chains x U = 531 264: 1 062 528 groups for k_rect_db's 4 096 x 256 threads -- the first 13 952 take a second trip."""
    C, B, warm, N = 4, 64, 64, 64 * 8300
    plan, v, n = run("asym_big", C, B, warm, N, start, THROUGHPUT, ASYM)
    assert v["db"] == "in_place" and 4096 * 256 < 2 * C * plan["U"] // 4 < 2 * 4096 * 256
    assert v["rel"] == "tile" and all(v["vec"])
    assert n > 100


@STARTS
@pytest.mark.parametrize("N,trips", [(64 * 40, 1), (64 * 2100, 2)])
def test_no_high_pass_reads_the_audio_itself(N, trips, start):
    """k_rect_db's from_x branch, one value per thread and trip: 8 x 2 624 values, and 8 x 134 464 = 1 075 712 for 1 048 576
    threads."""
    C, B, warm = 4, 64, 64
    plan, v, _ = run(f"from_x{trips}", C, B, warm, N, start, THROUGHPUT, dict(hipass_freq=0.0))
    assert plan["db_sym"] == 0 and v["db"] == "from_x" and -(-2 * C * plan["U"] // (4096 * 256)) == trips
