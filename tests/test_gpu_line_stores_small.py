"""Complete-line stores of the output walks (walk_lines_to: k_hp_run_lines, k_ar_warm_both<true>, k_ar_chunk<true>) at the
smallest shapes at which they can go wrong.  The row owners hand element offsets from the kernel's own output pointer round
the wave; lanes whose batches have run out load a shared line instead of skipping their loads.  Every case must give the
oracle's records and `rel` bit for bit, and the bits of the same call with lane-private stores (line_stores=-1).

Each case checks make_layout's conditions for the line forms by arithmetic (`takes_lines`: with lane_merge=1 they are
geometric only) and asks the detector's plan (BatchDetector.plan) which form the call takes.

Offsets past 2^32 bytes have no case here: 24 clips x 8 channels x 60 s is a 2.2 GB stream (offsets below 2^32 bytes), and a
call whose stream passes 4.3 GB needs as much again for its input and for each of the two `rel` outputs compared.  The
64-channel 600 s test (tests/test_gpu_pipeline.py, 7.4 GB per stream, line forms by its size) covers them."""
import numpy as np
import pytest

import oracle
from onset_fingerprinting_amd import synth

pytestmark = pytest.mark.gpu

SR = 48000


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def takes_lines(N, B, sr, hp_chunk, ar_chunk):
    """make_layout's conditions for hp_lines and ar_lines under lane_merge=1 (merged layout, closed-form guess)."""
    n_w = min(int(0.5 * sr), N)
    n_wb, Nm = n_w // B * B, N // B * B
    U, V = n_wb + Nm, n_w + Nm
    S = 4 if hp_chunk % 256 == 0 else 1
    hp = all(v % 32 == 0 for v in (n_w, n_wb, U, V, hp_chunk, hp_chunk // S))
    ar = U % 32 == 0 and ar_chunk % 32 == 0
    return hp and ar, dict(n_w=n_w, n_wb=n_wb, U=U, V=V)


_oracle = {}


def reference(key, make, **kw):
    """(x, channels, samples, rel) of the oracle, computed once per input."""
    if key not in _oracle:
        x = make()
        c, o, rel = oracle.detect_onsets_amplitude(x, **kw)
        _oracle[key] = (x, np.array(c, np.int64), np.array(o, np.int64), rel)
    return _oracle[key]


def check(key, make, tuning, **kw):
    from onset_fingerprinting_amd import detection
    x, c, o, orel = reference(key, make, **kw)
    got = {}
    for ls in (0, -1):
        # (every case here asserts `takes_lines`: the plan must say the same, and say no for the lane-private twin)
        bd = detection.BatchDetector(x.shape[1], device=0, **kw)
        bd.set_tuning(**dict(tuning, lane_merge=1, line_stores=ls))
        plan = bd.plan(1, len(x))
        assert plan["hp_lines"] == plan["ar_lines"] == int(ls == 0), (ls, plan)
        recs, rel, _ = detection.detect_batch(x[None], tuning=dict(tuning, lane_merge=1, line_stores=ls), **kw)
        assert np.array_equal(recs[0]["channel"], c) and np.array_equal(recs[0]["sample"], o), f"records, line_stores={ls}"
        assert rel[0].shape == orel.shape
        assert np.array_equal(bits(rel[0]), bits(orel)), f"relative envelope not bit-identical, line_stores={ls}"
        got[ls] = (recs[0], rel[0])
    assert np.array_equal(got[0][0], got[-1][0]) and np.array_equal(bits(got[0][1]), bits(got[-1][1]))
    return len(c)


@pytest.mark.parametrize("ar_chunk,hp_chunk", [(2048, 4096), (2080, 4128)])
def test_lanes_with_different_trip_counts_and_odd_batch_counts(ar_chunk, hp_chunk):
    """1 clip x 4 channels, 6 s: about 150 follower chunks and 76 IIR chunks per chain in waves that are not full, the last
    chunk of each chain shorter, so the lanes of a wave differ in their batch counts and some have none.
    Chunks of 2048 / 4096 steps are 64 / 32 batches (the paired loop alone), 2080 / 4128 are 65 / 129 (the tail batch
    after it)."""
    N = 288_077
    ok, g = takes_lines(N, 256, SR, hp_chunk, ar_chunk)
    assert ok and g["U"] % ar_chunk and g["V"] % hp_chunk, g
    n = check("drums4", lambda: synth.c2_drums(6.1, 4, SR, seed=3)[:N], dict(ar_chunk=ar_chunk, hp_chunk=hp_chunk),
              block_size=256, sr=SR)
    assert n > 10


def test_batches_without_output_in_the_dropped_gap():
    """Blocks of 96 and a warm-up of 23 936 samples (sr 47 872; 24 000 is a whole number of such blocks): n_wb = 23 904, so
    the 32 IIR outputs between them -- one batch, inside a sub-chunk -- go nowhere, and the batches on its two sides land
    in the two other regions of the stream."""
    sr, N = 47872, 143_700
    ok, g = takes_lines(N, 96, sr, 4096, 2048)
    assert ok and g["n_w"] == 23936 and g["n_wb"] == 23904, g
    n = check("gap", lambda: synth.c2_drums(3.1, 4, sr, seed=4)[:N], dict(ar_chunk=2048, hp_chunk=4096),
              block_size=96, sr=sr, cooldown=20)
    assert n > 5


@pytest.mark.parametrize("C", [8, 64])
def test_one_short_clip_of_8_and_64_channels(C):
    N = 96_000
    ok, g = takes_lines(N, 256, SR, 4096, 2048)
    assert ok, g
    check(f"short{C}", lambda: synth.c2_drums(2.0, C, SR, seed=20 + C)[:N], dict(ar_chunk=2048, hp_chunk=4096),
          block_size=256, sr=SR)
