"""The followers' interleaved line stores (walk_lines_to<C>: k_ar_warm_both<true, C>, k_ar_chunk<true, C>) and the in-place
back-to-linear stream behind them (k_rel_out_il<C>) at the smallest shapes at which they can go wrong.

With this layout the followers write their differences into the caller's `rel` and into the warm-up rows themselves, 32
rows of all channels per store group, and the planar `dif` array of the work space is not touched.  Every case must give
the oracle's records and `rel` bit for bit (oracle.OracleDetector.detect is what oracle.detect_onsets_amplitude calls, with
the warm-up length as an argument: the shapes here need warm-ups of one and of a few batches), and the bits of the same call
with tuning interleaved=-1, the planar path.  The block extremes (sum_max / sum_minv) are not exposed: what they decide is
the crossing pass, so the records stand for them.

Which form a call took: `takes_il` restates make_layout's conditions by arithmetic (with lane_merge=1 and line_stores=1
they are geometric only), the detector's plan reports it (BatchDetector.plan), and `untouched_run` observes it -- the work space is filled with a byte pattern before the call,
and only the new form leaves a stretch as long as the planar `dif` array (C x U floats per clip) as it was.

A value that is NaN compares as NaN on both sides instead of bit for bit against the ORACLE only: the sign and payload of
a NaN that arithmetic produces are the processor's choice (IEEE 754 leaves them open; x86 sets the sign bit of the NaN
it makes from inf - inf) and no property of the detector.  Between the two GPU forms NaNs compare bit for bit like everything else."""
import numpy as np
import pytest
import torch

import oracle
from onset_fingerprinting_amd import synth
from onset_fingerprinting_amd.detection import BatchDetector

pytestmark = pytest.mark.gpu

SR = 48000
FILL = 0xA5


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def geometry(N, B, warm):
    n_w = min(warm, N)
    n_wb, Nm = n_w // B * B, N // B * B
    return dict(n_w=n_w, n_wb=n_wb, Nm=Nm, U=n_wb + Nm)


def takes_il(C, N, B, warm, ar_chunk):
    """make_layout's ar_il under lane_merge=1, line_stores=1, relative thresholds, symmetric slow follower, `rel` asked for."""
    g = geometry(N, B, warm)
    return (C in (4, 8) and g["U"] % 32 == 0 and ar_chunk % 32 == 0 and g["n_wb"] % 32 == 0 and g["Nm"] % 32 == 0
            and B * C >= 256)


def untouched_run(ws):
    """Longest stretch of bytes of the work space that still hold the fill pattern."""
    changed = torch.nonzero(ws != FILL).flatten()
    edges = torch.cat([torch.tensor([-1], device=ws.device), changed, torch.tensor([ws.numel()], device=ws.device)])
    return int((edges[1:] - edges[:-1] - 1).max())


_oracle = {}


def reference(key, make, B, warm, **kw):
    """(x [clips][N][C], per clip (channels, samples, rel)) of the oracle, computed once per input."""
    if key not in _oracle:
        x = np.ascontiguousarray(make(), np.float32)
        per_clip = []
        for xc in x:
            c, o, rel = oracle.OracleDetector(xc.shape[1], B, **kw).detect(xc, warm)
            per_clip.append((np.array(c, np.int64), np.array(o, np.int64), rel))
        _oracle[key] = (x, per_clip)
    return _oracle[key]


def same_as_oracle(got, want):
    g, w = bits(got), bits(want)
    return got.shape == want.shape and bool(np.all((g == w) | (np.isnan(got) & np.isnan(want))))


def check(key, make, B, warm, tuning, expect_il, **kw):
    x, per_clip = reference(key, make, B, warm, **kw)
    n_clips, N, C = x.shape
    g = geometry(N, B, warm)
    assert takes_il(C, N, B, warm, tuning["ar_chunk"]) == expect_il, g
    xt = torch.from_numpy(x).cuda()
    got, info = {}, {}
    for il in (0, -1):
        bd = BatchDetector(C, B, device=0, **kw)
        bd.set_tuning(**dict(tuning, lane_merge=1, line_stores=1, interleaved=il))
        plan = bd.plan(n_clips, N, warm)
        assert plan["ar_il"] == int(expect_il and il == 0) and plan["mm_il"] == int(il == 0 and C in (4, 8, 64)), (il, plan)
        assert {k: plan[k] for k in g} == g
        ws = bd.reserve(n_clips, N, warm)
        ws.fill_(FILL)
        out = bd.detect(xt, warm=warm)
        recs = BatchDetector.records_to_numpy(out)
        rel = out["rel"].cpu().numpy()
        run, dif_bytes = untouched_run(ws), n_clips * C * g["U"] * 4
        print(f"{key} interleaved={il}: {bd.last_info['ar_passes']} follower passes, {bd.last_info['repaired']} repaired, "
              f"repeated {bd.last_info['repeated_host_verified']}, longest untouched stretch {run} B (dif: {dif_bytes} B)")
        assert (run >= dif_bytes) == (expect_il and il == 0), "the planar `dif` array: written by the planar path only"
        for i, (c, o, orel) in enumerate(per_clip):
            assert np.array_equal(recs[i]["channel"], c) and np.array_equal(recs[i]["sample"], o), (il, i, "records")
            assert same_as_oracle(rel[i], orel), (il, i, "relative envelope not bit-identical to the oracle's")
        got[il], info[il] = (recs, rel), bd.last_info
    for a, b in zip(got[0][0], got[-1][0]):
        assert np.array_equal(a, b)
    assert np.array_equal(bits(got[0][1]), bits(got[-1][1])), "the two forms differ"
    return info[0], sum(len(c) for c, _, _ in per_clip)


def drums(seconds, C, seed, N, clips=1):
    return lambda: np.stack([synth.drum_hits(C, seconds, SR, seed=seed + i, period=0.11)[:N] for i in range(clips)])


def test_warm_up_of_one_batch_and_a_last_chunk_of_one_batch():
    """8 channels, blocks of 32 (one 16-byte group per lane of the linear pass's wave), 32 warm-up rows: the first batch
    of chunk 0 goes to the warm-up rows and the next to row 0 of `rel`.  U = 20 512 = 10 chunks of 2 048 and one of 32
    steps; groups of two chunks, so the walk-through of k_ar_warm_both and pass 0 of k_ar_chunk alternate."""
    N, B, warm = 20480, 32, 32
    assert geometry(N, B, warm)["U"] == 10 * 2048 + 32
    _, n = check("b32", drums(0.5, 8, 11, N), B, warm, dict(ar_chunk=2048, ar_span=2), True, sr=SR)
    assert n > 4


def test_three_clips_of_4_channels_and_one_chunk_more_than_a_group():
    """3 clips x 4 channels x 5 chunks = 60 lanes: a wave with lanes that have no chunk; two chunk groups per store
    instruction.  A warm-up of 192 rows (six batches; n_w = 200 is no multiple of 32, so only the followers take line
    stores); groups of 4 chunks: chunk 4 is a group of its own, the last chunk 3 008 = 94 x 32 steps."""
    N, B, warm = 64 * 300 + 17, 64, 200
    g = geometry(N, B, warm)
    assert g["n_wb"] == 192 and g["U"] == 4 * 4096 + 3008
    _, n = check("c4x3", drums(0.41, 4, 21, N, clips=3), B, warm, dict(ar_chunk=4096, ar_span=4), True, sr=SR)
    assert n > 6


@pytest.mark.parametrize("ar_chunk", [8192, 4096])
def test_exactly_one_chunk_and_two_chunks_with_a_short_second(ar_chunk):
    """U = 6 464: one chunk (k_ar_chunk's pass 0 alone writes, no verifying pass), or 4 096 + 2 368 (74 x 32) steps with
    chunk 0 walked through by k_ar_warm_both."""
    N, B, warm = 6400, 64, 64
    assert geometry(N, B, warm)["U"] == 6464
    info, _ = check("short8", drums(0.14, 8, 31, N), B, warm, dict(ar_chunk=ar_chunk, ar_span=2), True, sr=SR)
    assert info["ar_passes"] == (1 if ar_chunk == 8192 else 2)


@pytest.mark.parametrize("C", [3, 64])
def test_other_channel_counts_take_the_planar_path(C):
    N, B, warm = 6400, 64, 64
    check(f"short{C}", drums(0.14, C, 40 + C, N), B, warm, dict(ar_chunk=4096, ar_span=2), False, sr=SR)


def test_a_length_that_is_no_multiple_of_32_takes_the_planar_path():
    N, B, warm = 48 * 133, 48, 48
    assert geometry(N, B, warm)["Nm"] % 32 == 16
    check("odd48", drums(0.14, 8, 51, N), B, warm, dict(ar_chunk=4096, ar_span=2), False, sr=SR)


def test_a_verifying_pass_repairs_some_channels_of_a_chunk():
    """No exact warm-up (ar_warm=-1): a group's first chunk starts from the floor and the closed-form guess, which is wrong
    for every channel that carries signal and right, bit for bit, for a silent one (its followers never leave the floor).
    Channels 2 and 5 are silent: the verifying passes repair six channels of a chunk, the lanes of the other two walk
    with them and must leave their rows as they were."""
    N, B, warm = 20480, 64, 128

    def make():
        x = drums(0.5, 8, 61, N)()
        x[:, :, 2] = 0.0
        x[:, :, 5] = 0.0
        return x

    info, n = check("silent2", make, B, warm, dict(ar_chunk=2048, ar_span=2, ar_warm=-1), True, sr=SR)
    assert info["repaired"] > 0 and info["ar_passes"] > 1
    assert n > 4


def test_nan_and_infinities_in_one_channel():
    """No high-pass, so the values reach the dB pass as they are.  Channel 1: -inf (a block with a value clipped to
    -floor), later +inf and NaN: from the second step after the first of them the channel's envelope is NaN to the end --
    blocks with a clipped value, with NaN and numbers, and with NaN alone, for the extremes' rule."""
    N, B, warm = 20480, 64, 128

    def make():
        x = drums(0.5, 4, 71, N)()
        x[0, 7000, 1] = -np.inf
        x[0, 9000, 1] = np.inf
        x[0, 11000, 1] = np.nan
        return x

    _, n = check("nan4", make, B, warm, dict(ar_chunk=2048, ar_span=2), True, sr=SR, hipass_freq=0.0)
    assert n > 2
