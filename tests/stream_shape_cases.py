"""Case tables and input builders of the realtime-path shape tests (tests/test_stream_shapes_cpu.py checks on the
oracle that every case reaches what it claims, tests/test_gpu_stream_shapes.py runs them on the GPU).

Part A: the two block kernels of csrc/ofp_stream.hip (k_stream, k_stream_par) with more than one wavefront of channels
and on both sides of the rule that chooses between them.  Part B: realtime.HopSession at every frame length, with
hop >= frame, the ring at its minimum, filterbanks with empty bands, and on both sides of the rule that chooses the
one-kernel form.

Every reference here comes from the CPU oracle; it is computed once per case (lru_cache) and returned read-only.
"""
import functools

import numpy as np

import oracle
from onset_fingerprinting_amd import synth

SR = 48000
WARM = 2400   # rows given to init_minmax_tracker on both sides
WAVE = 64     # lanes of a wavefront: channel c is lane c % 64 of wave c // 64 in both block kernels

# ---- the rules, restated once ---------------------------------------------------------------------------------

PAR_MAX_C = 512               # csrc/ofp_stream_dev.h
PAR_MAX_LDS = 120 * 1024      # ofp_stream_process
PAR_RAISED_ATTR = 48 * 1024   # ofp_stream_process raises k_stream_par's dynamic-LDS attribute above this
STREAM_MAX_C = 1024           # ofp_stream_process refuses more channels
FUSED_MAX_LDS = 96 * 1024     # ofp_hop_create


def plane_bytes(C, B):
    """The three [B][C] float planes the phase-split kernel stages a block in."""
    return 3 * B * C * 4


def takes_phase_split(C, B):
    """ofp_stream_process (csrc/ofp_stream.hip): k_stream_par when this holds (and OFP_STREAM_KERNEL is not "seq"),
    else the one-lane-per-channel k_stream."""
    return C <= PAR_MAX_C and plane_bytes(C, B) <= PAR_MAX_LDS


def fused_threads(F):
    """FusedCfg<F>::WGS (csrc/ofp_hop.hip) from Cfg<F>::T (csrc/ofp_fft.h): 256 lanes while a frame fits one wave."""
    m8 = F // 16
    T = 16 if m8 < 16 else (64 if m8 > 64 and F <= 2048 else m8)
    return 256 if T <= 64 else T


def takes_fused(C, B, F):
    """ofp_hop_create (csrc/ofp_hop.hip): the one-kernel form when this holds (and OFP_HOP_GRAPH is not "nodes"),
    else the five-node graph."""
    return 2 * C <= fused_threads(F) and C <= PAR_MAX_C and plane_bytes(C, B) <= FUSED_MAX_LDS


# ---- inputs ---------------------------------------------------------------------------------------------------

def tiled_hits(C, seconds, sr=SR, seed=1, period=0.05, amp=0.8):
    """synth.drum_hits offsets channel c by 37 c samples: with many channels and a short block at most one channel
    fires per block.  Eight channels tiled over C with per-channel gains instead: channels c, c + 8, c + 16, ... fire
    in the same block, in every wavefront."""
    base = synth.drum_hits(8, seconds, sr, seed, period=period, amp=amp)
    gains = (0.5 + np.random.default_rng(C).random(C)).astype(np.float32)
    x = np.ascontiguousarray(base[:, np.arange(C) % 8] * gains)
    assert x.dtype == np.float32
    return x


PROBE_DIP = 362   # rows after a hit at which the default detector's envelope is about to fall below `off` (measured
                  # on the oracle: 367 to 389 rows once the tracker has settled)


def probe_hits(x, B, probe, far, sr=SR, period=0.05):
    """x (tiled_hits, hits every `period`) plus, in the quiet stretch of every period, an event that makes the
    cross-wave maximum matter: channel `probe` is hit, stays "on", and is hit again in the block in which its envelope
    has just dipped below `off` -- it dips and recovers inside one block, so its last row below `off` lies in the
    middle of that block.  Channel `far`, in another wavefront, is hit a few rows later: its onset index is the
    block's largest and lies above that row, so `last >= omax` is false and `probe` stays "on" -- while its own
    wavefront's largest onset index (nothing fires there) is 0 and would clear it.  A third hit on `probe` 350 rows on
    crosses `on` while the true state is still "on": with cooldown=0 a detector that cleared the state reports an
    onset there, the reference does not."""
    x = x.copy()
    k = np.arange(300)
    rng = np.random.default_rng(B)
    row2, delta = (B - 10, 4) if B <= 32 else (60, 10)
    for s in (np.arange(period, len(x) / sr - 0.2, period) * sr).astype(np.int64):
        p = s + 1000
        p += -(p + PROBE_DIP) % B           # the dip begins in the first rows of a block,
        t2 = p + PROBE_DIP + row2           # the second hit comes later in that block
        for t, c in ((p, probe), (t2, probe), (t2 + 350, probe), (t2 + delta, far)):
            x[t:t + 300, c] += (0.8 * np.exp(-k / 40) * rng.standard_normal(300)).astype(np.float32)
    return x


def _readonly(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


# ---- part A: block kernels ------------------------------------------------------------------------------------

def _options():
    from onset_fingerprinting_amd import realtime
    return {
        "defaults": dict(),
        "nohp_manual": dict(hipass_freq=0, on_threshold=6.0, off_threshold=4.0),
        "cooldown0": dict(cooldown=0),
        "backtrack": dict(backtrack=True, backtrack_buffer_size=128, backtrack_smooth_size=5),
        "realtime": dict(realtime.REALTIME_DETECTOR_KWARGS),
        # cooldown=0 on probe_hits(): the input on which a wave-local maximum changes the records
        "probe": dict(cooldown=0),
    }


OPTIONS = _options()
ALL_OPTIONS = tuple(OPTIONS)
PROBE_CHANNELS = {"65x96": (5, 64), "130x32": (5, 129)}   # (probe, far): first and last wavefront

# C x B -> duration, the side of the rule it is on (par: k_stream_par under the default choice), option sets
BLOCK_SHAPES = {
    # one lane into the second wave; 73 KiB of planes: above the raised-attribute threshold
    "65x96": dict(C=65, B=96, seconds=0.6, par=True, options=ALL_OPTIONS),
    # three waves, the last partial; 48.75 KiB: just above 48 KiB
    "130x32": dict(C=130, B=32, seconds=0.6, par=True, options=ALL_OPTIONS),
    # PAR_MAX_C: 1024 role lanes, 16 waves, every s_red slot
    "512x16": dict(C=512, B=16, seconds=0.3, par=True, options=("defaults",)),
    # one past PAR_MAX_C: the one-lane kernel
    "513x16": dict(C=513, B=16, seconds=0.3, par=False, options=("defaults",)),
    # exactly 120 KiB and one channel past it
    "160x64": dict(C=160, B=64, seconds=0.6, par=True, options=("defaults",)),
    "161x64": dict(C=161, B=64, seconds=0.6, par=False, options=("defaults",)),
    # the most channels the streaming form takes: k_stream with 16 waves
    "1024x8": dict(C=1024, B=8, seconds=0.3, par=False, options=("defaults",)),
}
BLOCK_CASES = [(s, o) for s, cfg in BLOCK_SHAPES.items() for o in cfg["options"]]
CALL_SPLIT = (1, 7, 2)   # blocks per process() call, then the rest: state is handed over both ways


@functools.lru_cache(maxsize=None)
def block_input(shape, probe=False):
    cfg = BLOCK_SHAPES[shape]
    x = tiled_hits(cfg["C"], 1.0 if probe else cfg["seconds"], SR, seed=cfg["C"] + cfg["B"])
    if probe:
        x = probe_hits(x, cfg["B"], *PROBE_CHANNELS[shape])
    x = x[: len(x) // cfg["B"] * cfg["B"]]
    x.setflags(write=False)
    return x


def thresholds_f32(kw, mn, mx):
    """The float32 on / off thresholds of a block from the post-block tracker (detection.py:763, :787)."""
    on = np.float32(kw.get("on_threshold", 0.5))
    off = np.float32(kw.get("off_threshold", 0.1))
    if on > 1:  # manual
        return np.full(len(mn), on, np.float32), np.full(len(mn), off, np.float32)
    return (mx * on).astype(np.float32) + mn, (mx * off).astype(np.float32) + mn


@functools.lru_cache(maxsize=None)
def block_reference(shape, option):
    """The oracle over the case's input, block by block: rel, records (channel, absolute sample) in order, the state
    it leaves, and what the vacuity conditions need:
      spanning_blocks  blocks whose onsets lie in two or more wavefronts
      flip_blocks      blocks in which a channel that is "on" after the block has its last row below `off` at or above
                       the largest onset index of its OWN wavefront but below the block's largest, held by another
                       wavefront alone: a wave-local maximum would have cleared its state
      consequential    of those channels, the ones that cross `on` upwards in a later block while still "on" with
                       cooldown=0: there a detector that cleared the state writes a record the reference does not
    (flip_blocks / consequential stay 0 with backtracking: the first-crossing indices are then not in the oracle's
    outputs.)"""
    cfg, kw = BLOCK_SHAPES[shape], OPTIONS[option]
    C, B = cfg["C"], cfg["B"]
    x = block_input(shape, probe=option == "probe")
    od = oracle.OracleDetector(C, B, sr=SR, **kw)
    od.init_minmax_tracker(x[:WARM])
    nb = len(x) // B
    rels, ch, on = [], [], []
    spanning, flips, consequential, pending = 0, 0, 0, set()
    for i in range(nb):
        before = od.state()
        c, d, rel = od(x[i * B:(i + 1) * B])
        rels.append(rel)
        ch += [int(v) for v in c]
        on += [i * B + int(v) for v in d]
        spanning += len(set(int(v) // WAVE for v in c)) >= 2
        if kw.get("backtrack") or not (len(c) or pending):
            continue
        st = od.state()
        on_t, off_t = thresholds_f32(kw, st["mn"], st["mx"])
        if pending:
            row_before = np.concatenate([before["prev"][None, :], rel[:-1].astype(np.float64)])
            up = ((rel > on_t[None, :]) & (row_before < on_t[None, :].astype(np.float64))).any(0)
            for p in sorted(pending):
                if before["state"][p] != 1:
                    pending.discard(p)
                elif up[p] and kw.get("cooldown", 1323) == 0:
                    consequential += 1
                    pending.discard(p)
        if not len(c):
            continue
        oi = np.zeros(C, np.int64)
        oi[c] = d
        omax = int(oi.max())
        waves_of_max = set((np.nonzero(oi == omax)[0] // WAVE).tolist())
        below = rel < off_t[None, :]
        last = np.where(below.any(0), B - 1 - np.argmax(below[::-1], axis=0), -1)
        flipped = False
        for w in range((C + WAVE - 1) // WAVE):
            if waves_of_max == {w}:
                continue
            lo = w * WAVE
            sl = slice(lo, min(C, lo + WAVE))
            hit = (st["state"][sl] == 1) & (last[sl] >= int(oi[sl].max())) & (last[sl] < omax)
            flipped |= bool(hit.any())
            pending |= set((np.nonzero(hit)[0] + lo).tolist())
        flips += flipped
    return _readonly(dict(x=x, nb=nb, rel=np.concatenate(rels), channels=np.array(ch, np.int64),
                          samples=np.array(on, np.int64), state=_readonly(od.state()), spanning_blocks=spanning,
                          flip_blocks=flips, consequential=consequential))


# AmplitudeOnsetDetector.init with more than one workgroup of k_calibrate: two argument sets of G15 at wide channel
# counts, fresh seeds
def init_cases():
    from tests.golden.make_golden_init_cfg import G15
    out = {}
    for name, C, seed in (("manual_48k_64", 65, 651), ("manual_48k_64", 130, 1301),
                          ("fast_ar_32", 65, 652), ("fast_ar_32", 130, 1302)):
        out[f"{name}-{C}"] = dict(G15[name], C=C, seed=seed)
    return out


INIT_CASES = init_cases()


@functools.lru_cache(maxsize=None)
def init_reference(name):
    """run_init_case (tests/test_oracle_golden.py) on the oracle: (detector, (x, y), channels, deltas, blocks, rel)."""
    from tests.test_oracle_golden import run_init_case
    return run_init_case(lambda C, B, sr, kw: oracle.OracleDetector(C, B, sr=sr, **kw), INIT_CASES[name])


# ---- part B: hop sessions -------------------------------------------------------------------------------------

# n_out None: no classifier.  ring_min: ring_seconds=0, the ring has max(F, B) rows.  empty: bands without a weight.
HOP_CASES = {
    # n_fft 512; the hop does not divide the ring; ring at its minimum, at least 3 wraps
    "2x96x512": dict(C=2, B=96, F=512, sr=48000, n_mels=40, n_out=8, hops=80, ring_min=True, empty=0),
    # one channel; 4 empty bands; odd output width
    "1x64x512-96k": dict(C=1, B=64, F=512, sr=96000, n_mels=64, n_out=5, hops=80, ring_min=False, empty=4),
    # B == F: the whole frame comes from the hop; ring at its minimum
    "3x256x256": dict(C=3, B=256, F=256, sr=48000, n_mels=40, n_out=8, hops=60, ring_min=True, empty=0),
    # B > F; 127 bands (the limit), 33 of them empty
    "2x512x256": dict(C=2, B=512, F=256, sr=48000, n_mels=127, n_out=8, hops=40, ring_min=False, empty=33),
    # a single band
    "2x64x256-1band": dict(C=2, B=64, F=256, sr=48000, n_mels=1, n_out=None, hops=80, ring_min=False, empty=0),
    # 127 non-empty bands: 1007 weights in 128 32-tap segments (158 by the bound ofp_hop_create admits them with,
    # fb_nnz / 32 + n_mels)
    "2x128x1024": dict(C=2, B=128, F=1024, sr=48000, n_mels=127, n_out=3, hops=60, ring_min=False, empty=0,
                       nnz=1007, segments=128, segment_bound=158),
    # fused at both limits (2C == 256, planes == 96 KiB): the fused kernel's LDS is set by the detector planes, above
    # 64 KiB; two waves of channel lanes inside the fused kernel
    "128x64x256": dict(C=128, B=64, F=256, sr=48000, n_mels=40, n_out=8, hops=80, ring_min=False, empty=0, tiled=True),
    # one channel past 2C <= WGS: nodes form, with k_stream_par at 320 lanes
    "129x32x256": dict(C=129, B=32, F=256, sr=48000, n_mels=40, n_out=None, hops=80, ring_min=False, empty=0,
                       tiled=True),
    # one sample past 96 KiB: nodes form; a hop that is a multiple of nothing
    "128x65x256": dict(C=128, B=65, F=256, sr=48000, n_mels=40, n_out=None, hops=80, ring_min=False, empty=0,
                       tiled=True),
}
# which form each takes with OFP_HOP_GRAPH unset
HOP_FUSED = {"2x96x512": True, "1x64x512-96k": True, "3x256x256": True, "2x512x256": True, "2x64x256-1band": True,
             "2x128x1024": True, "128x64x256": True, "129x32x256": False, "128x65x256": False}


# Hits of the hop cases: amplitude 0.03 (0.1 at 96 kHz) instead of synth.drum_hits' 0.8.  check_spectral holds EVERY
# band of every frame to 1e-4 of the fp64 oracle.  A float32 transform leaves each bin with an error of a few 2^-24 of
# the frame's LARGEST bin, so a band 90-100 dB below the frame's largest -- the 1e-3 noise floor next to the 200 Hz
# body of hits at 0.8 that pile up when they come every 20 ms -- cannot be held to 1e-4 by any float32 kernel (a
# float32 pocketfft on the same frames is off by up to 1e-3 there).  At 0.03 the bands stay within about 70 dB of each
# other, as they do in the streams of tests/test_gpu_stream.py, and the detector still fires on every hit.
HOP_AMP, HOP_AMP_96K = 0.03, 0.1
HOP_PERIOD = {"128x64x256": 0.05, "128x65x256": 0.05}   # the tiled recipe's own period where 80 hops hold two hits


@functools.lru_cache(maxsize=None)
def hop_input(case, seed=0):
    """[max(hops * B, WARM), C] float32, hits every 20 ms (8 ms at 96 kHz) so that 40-80 hops hold several."""
    cfg = HOP_CASES[case]
    C, B, sr, n = cfg["C"], cfg["B"], cfg["sr"], cfg["hops"] * cfg["B"]
    n = max(n, WARM)
    secs = n / sr + 0.21
    period = HOP_PERIOD.get(case, 0.02 if sr == 48000 else 0.008)
    amp = HOP_AMP if sr == 48000 else HOP_AMP_96K
    sd = 7 * C + B + cfg["F"] + seed
    if cfg.get("tiled"):
        x = tiled_hits(C, secs, sr, sd, period, amp)
    else:
        x = synth.drum_hits(C, secs, sr, sd, period=period, amp=amp)
    x = np.ascontiguousarray(x[:n])
    x.setflags(write=False)
    return x


def hop_ring_rows(cfg):
    return max(cfg["F"], cfg["B"]) if cfg["ring_min"] else None


@functools.lru_cache(maxsize=None)
def hop_detector_reference(case, seed=0):
    """The oracle detector over hop_input(case), hop by hop, as replay() of tests/test_gpu_stream.py collects it."""
    cfg = HOP_CASES[case]
    C, B = cfg["C"], cfg["B"]
    x = hop_input(case, seed)
    od = oracle.OracleDetector(C, B, sr=cfg["sr"])
    od.init_minmax_tracker(x[:WARM])
    ch, on, rels, spanning = [], [], [], 0
    for i in range(cfg["hops"]):
        c, d, rel = od(x[i * B:(i + 1) * B])
        ch += [int(v) for v in c]
        on += [i * B + int(v) for v in d]
        rels.append(rel)
        spanning += len(set(int(v) // WAVE for v in c)) >= 2
    return _readonly(dict(ch=ch, on=on, rel=np.concatenate(rels), spanning_blocks=spanning))


def band_layout(sr, F, n_mels):
    """(empty bands, weights, 32-tap segments) of the filterbank as the session uploads it."""
    from onset_fingerprinting_amd import realtime
    from onset_fingerprinting_amd.data import mel_filterbank
    lo, ln, off, w = realtime._band_csr(mel_filterbank(sr, F, n_mels))
    return int((ln == 0).sum()), int(ln.sum()), int(((ln + 31) // 32).sum())


# onset strength and tempogram at the two short frames: idle lanes of the workgroup take part in every reduction
STRENGTH_KW = dict(max_length=12, avg_length=40, ring=64, tg_win_length=48)
STRENGTH_CASES = {
    "F256-ring-min": dict(C=3, B=64, F=256, sr=48000, hops=160, ring_min=True),
    "F512": dict(C=3, B=64, F=512, sr=48000, hops=160, ring_min=False),
}


@functools.lru_cache(maxsize=None)
def strength_input(case):
    cfg = STRENGTH_CASES[case]
    n = cfg["hops"] * cfg["B"]
    x = np.ascontiguousarray(synth.drum_hits(cfg["C"], n / cfg["sr"] + 0.21, cfg["sr"], seed=cfg["F"], period=0.03)[:n])
    x.setflags(write=False)
    return x
