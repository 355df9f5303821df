"""Oracle-only checks of tests/stream_shape_cases.py: every case of tests/test_gpu_stream_shapes.py is on the side of
the kernel-choice rules it claims to be on and exercises what it claims to exercise, so that none of them can pass
vacuously.  No GPU."""
import re
from pathlib import Path

import numpy as np
import pytest

from tests import stream_shape_cases as sc

CSRC = Path(__file__).resolve().parents[1] / "onset_fingerprinting_amd" / "csrc"


def squeeze(text):
    return re.sub(r"\s+", " ", text)


def test_the_restated_rules_are_the_ones_in_the_sources():
    """The conditions of ofp_stream_process and ofp_hop_create as they stand in the sources: whoever changes one of
    them meets this test, then the case tables below."""
    stream, dev, hop = (squeeze((CSRC / n).read_text()) for n in ("ofp_stream.hip", "ofp_stream_dev.h", "ofp_hop.hip"))
    assert "constexpr int PAR_MAX_C = 512;" in dev and sc.PAR_MAX_C == 512
    assert "const size_t par_lds = (size_t)3 * d->p.block_size * C * sizeof(float);" in stream
    assert "const bool par_ok = !warmup && C <= PAR_MAX_C && par_lds <= 120 * 1024;" in stream
    assert "par_lds, attr, 65536 - 16384)" in stream and sc.PAR_RAISED_ATTR == 65536 - 16384
    assert "d->p.n_channels <= 1024" in stream and sc.STREAM_MAX_C == 1024
    assert "const size_t par_lds = (size_t)3 * B * C * sizeof(float);" in hop
    assert ("2 * C <= fused_threads && C <= ofpstream::PAR_MAX_C && par_lds <= 96 * 1024;") in hop
    assert "static constexpr int WGS = HopCfg<F>::T <= 64 ? 256 : HopCfg<F>::T;" in hop
    assert [sc.fused_threads(F) for F in (256, 512, 1024, 2048, 4096)] == [256, 256, 256, 256, 256]


def test_block_shapes_sit_on_the_stated_side_of_the_rule():
    for name, cfg in sc.BLOCK_SHAPES.items():
        assert name == f"{cfg['C']}x{cfg['B']}"
        assert sc.takes_phase_split(cfg["C"], cfg["B"]) == cfg["par"], name
        assert cfg["C"] <= sc.STREAM_MAX_C
    pb = sc.plane_bytes
    assert pb(65, 96) == 74880 > sc.PAR_RAISED_ATTR                     # the raised attribute
    assert pb(130, 32) == 49920 and 0 < pb(130, 32) - sc.PAR_RAISED_ATTR < 1024   # just above 48 KiB
    assert pb(160, 64) == sc.PAR_MAX_LDS and pb(161, 64) > sc.PAR_MAX_LDS   # exactly the limit, one channel past it
    assert sc.BLOCK_SHAPES["512x16"]["C"] == sc.PAR_MAX_C and pb(512, 16) <= sc.PAR_MAX_LDS
    assert sc.BLOCK_SHAPES["513x16"]["C"] == sc.PAR_MAX_C + 1 and pb(513, 16) <= sc.PAR_MAX_LDS   # only C decides
    assert sc.BLOCK_SHAPES["1024x8"]["C"] == sc.STREAM_MAX_C
    # the option sets the issue asks for, on the two shapes it names
    for name in ("65x96", "130x32"):
        assert set(sc.BLOCK_SHAPES[name]["options"]) >= {"defaults", "nohp_manual", "cooldown0", "backtrack", "realtime"}


@pytest.mark.parametrize("shape,option", sc.BLOCK_CASES)
def test_wide_block_cases_cross_wavefronts(shape, option):
    """At least 5 blocks whose onsets span two or more wavefronts and at least 100 onsets, for every shape and option
    set; the call split leaves a last call of several blocks."""
    ref = sc.block_reference(shape, option)
    C, B = sc.BLOCK_SHAPES[shape]["C"], sc.BLOCK_SHAPES[shape]["B"]
    assert C > sc.WAVE
    print(f"{shape} {option}: {ref['nb']} blocks, {len(ref['channels'])} onsets, {ref['spanning_blocks']} blocks span "
          f"wavefronts, {ref['flip_blocks']} flip blocks, {ref['consequential']} consequential")
    assert ref["spanning_blocks"] >= 5
    assert len(ref["channels"]) >= 100
    assert ref["nb"] > sum(sc.CALL_SPLIT) + 10 and ref["x"].shape == (ref["nb"] * B, C)
    assert len(set((ref["channels"] // sc.WAVE).tolist())) == (C + sc.WAVE - 1) // sc.WAVE   # every wavefront fires
    assert ref["rel"].shape == ref["x"].shape and np.isfinite(ref["rel"]).all()


@pytest.mark.parametrize("shape", sorted(sc.PROBE_CHANNELS))
def test_probe_input_makes_the_cross_wave_maximum_decide_a_record(shape):
    """The tiled input alone never has a channel whose `last >= omax` test depends on another wavefront's onset index
    (all wavefronts fire within a few rows of each other, and a channel that is "on" stays above `off` until it
    decays for good): flip_blocks is 0 for every option set on it.  The "probe" input has such blocks, and in at least
    one of them the channel goes on to cross `on` while still "on": a wave-local maximum changes the records.  (The
    block need not be one whose onsets span wavefronts: the probe's own wavefront is silent in it, which is what makes
    its local maximum 0.)"""
    probe, far = sc.PROBE_CHANNELS[shape]
    assert probe // sc.WAVE != far // sc.WAVE and "probe" in sc.BLOCK_SHAPES[shape]["options"]
    assert sc.OPTIONS["probe"] == dict(cooldown=0)
    ref = sc.block_reference(shape, "probe")
    assert ref["flip_blocks"] >= 1 and ref["consequential"] >= 1
    for option in ("defaults", "cooldown0"):
        assert sc.block_reference(shape, option)["flip_blocks"] == 0


def test_init_cases_are_wide_and_find_onsets():
    assert {c["C"] for c in sc.INIT_CASES.values()} == {65, 130}
    for name, cfg in sc.INIT_CASES.items():
        _, _, ch, de, blk, rel = sc.init_reference(name)
        assert (cfg["C"] + 63) // 64 >= 2   # k_calibrate's grid
        assert rel.shape == (cfg["follow_blocks"] * cfg["B"], cfg["C"])
        if name.startswith("manual"):  # (as the C <= 4 test asks of this argument set)
            assert len(ch) > 0
        if name == "manual_48k_64-130":
            assert len(set((ch // sc.WAVE).tolist())) >= 2   # k_calibrate workgroups 0 and 1 at least


def test_hop_cases_take_the_stated_form_and_reach_what_they_claim():
    assert set(sc.HOP_FUSED) == set(sc.HOP_CASES)
    for name, cfg in sc.HOP_CASES.items():
        C, B, F = cfg["C"], cfg["B"], cfg["F"]
        assert sc.takes_fused(C, B, F) == sc.HOP_FUSED[name], name
        assert 40 <= cfg["hops"] <= 80
        empty, nnz, segs = sc.band_layout(cfg["sr"], F, cfg["n_mels"])
        assert empty == cfg["empty"], (name, empty)
        assert nnz == cfg.get("nnz", nnz) and segs == cfg.get("segments", segs), (name, nnz, segs)
        assert nnz // 32 + cfg["n_mels"] == cfg.get("segment_bound", nnz // 32 + cfg["n_mels"]) <= 256
        ref = sc.hop_detector_reference(name)
        assert len(ref["on"]) >= 3, (name, len(ref["on"]))
        if cfg.get("tiled"):  # the conditions of part A
            assert ref["spanning_blocks"] >= 5 and len(ref["on"]) >= 100, (name, ref["spanning_blocks"], len(ref["on"]))
    fr = {n: sc.HOP_CASES[n] for n in sc.HOP_CASES}
    assert {c["F"] for c in fr.values()} >= {256, 512, 1024}
    # the frame comes from the hop alone / the ring at its minimum with a hop that does not divide it
    assert fr["3x256x256"]["B"] == fr["3x256x256"]["F"] and fr["2x512x256"]["B"] > fr["2x512x256"]["F"]
    c = fr["2x96x512"]
    R = sc.hop_ring_rows(c)
    assert R == 512 and R % c["B"] != 0 and c["hops"] * c["B"] >= 3 * R
    assert sc.hop_ring_rows(fr["3x256x256"]) == 256
    # both limits of the one-kernel form at once, and one step past each
    assert 2 * 128 == sc.fused_threads(256) and sc.plane_bytes(128, 64) == sc.FUSED_MAX_LDS > 64 * 1024
    assert 2 * 129 > sc.fused_threads(256) and sc.plane_bytes(129, 32) <= sc.FUSED_MAX_LDS
    assert sc.takes_phase_split(129, 32) and (2 * 129 + 63) // 64 * 64 == 320   # k_stream_par at 320 lanes
    assert 2 * 128 <= sc.fused_threads(256) and sc.plane_bytes(128, 65) - sc.FUSED_MAX_LDS == 3 * 128 * 4
    assert sc.takes_phase_split(128, 65)
    # the filterbanks of the issue
    assert sc.band_layout(48000, 256, 127)[0] == 33 and sc.band_layout(96000, 512, 64)[0] == 4
    assert sc.band_layout(48000, 1024, 127) == (0, 1007, 128)


def test_strength_cases_cover_both_short_frames():
    assert {c["F"] for c in sc.STRENGTH_CASES.values()} == {256, 512}
    assert sum(c["ring_min"] for c in sc.STRENGTH_CASES.values()) >= 1
    for name, c in sc.STRENGTH_CASES.items():
        assert c["C"] == 3 and c["B"] == 64 and c["hops"] >= 150
        assert sc.takes_fused(c["C"], c["B"], c["F"])
        assert sc.strength_input(name).shape == (c["hops"] * c["B"], c["C"])
        assert sc.STRENGTH_KW["tg_win_length"] <= sc.STRENGTH_KW["ring"]
