"""The realtime path at the shapes between the ones tests/test_gpu_stream.py runs: the block kernels of
csrc/ofp_stream.hip with several wavefronts of channels and on both sides of the rule that chooses between them,
AmplitudeOnsetDetector.init with more than one workgroup, and realtime.HopSession / HopSessionGroup at every frame
length, with hop >= frame, the ring at its minimum, empty mel bands and at both limits of the one-kernel form.

The bars are those of tests/test_gpu_stream.py: everything the detector produces bit for bit the CPU oracle's, mel and
logits bit for bit the dense kernel's and within RTOL of the fp64 oracle element-wise.  The case tables live in
tests/stream_shape_cases.py; tests/test_stream_shapes_cpu.py shows on the oracle that no case passes vacuously.
"""
import numpy as np
import pytest
import torch

import oracle
from tests import stream_shape_cases as sc
from tests.test_gpu_stream import RTOL, bits, check_spectral, replay, spectral_reference
from tests.test_oracle_golden import run_init_case

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()  # (a copy: the cached inputs are read-only)


# ---- A: block kernels -----------------------------------------------------------------------------------------

def device_state(od, C):
    """The carried state of a streaming detector as oracle.OracleDetector.state() names it (the layout of
    ofpstream::carve, csrc/ofp_stream_dev.h)."""
    raw = od._state.cpu().numpy()
    out, at = {}, 0
    for name, dt, n in (("prev", np.float64, C), ("deb", np.int64, C), ("zi", np.float32, 4 * C), ("yf", np.float32, C),
                        ("ys", np.float32, C), ("mn", np.float32, C), ("mx", np.float32, C), ("state", np.int32, C)):
        nbytes = n * np.dtype(dt).itemsize
        out[name] = raw[at:at + nbytes].view(dt).copy()
        at += nbytes
    out["zi"] = out["zi"].reshape(4, C)
    return out, raw


@pytest.mark.parametrize("shape,option", sc.BLOCK_CASES)
def test_block_kernels_match_the_oracle_with_several_wavefronts(shape, option, monkeypatch):
    """AmplitudeOnsetDetector.process over the whole stream in four calls of 1, 7, 2 and the remaining blocks, under
    the default kernel choice (k_stream_par for the shapes the table marks `par`, else k_stream) and under
    OFP_STREAM_KERNEL=seq (k_stream): rel, the records in order, the count and the state left behind equal the
    oracle's bit for bit, and the two runs leave the same state bytes."""
    from onset_fingerprinting_amd import detection
    cfg, kw = sc.BLOCK_SHAPES[shape], sc.OPTIONS[option]
    C, B = cfg["C"], cfg["B"]
    assert sc.takes_phase_split(C, B) == cfg["par"]
    ref = sc.block_reference(shape, option)
    x, nb = ref["x"], ref["nb"]
    xd = dev(x)
    n_exp = len(ref["channels"])
    raws = []
    for mode in ("seq", None):
        if mode:
            monkeypatch.setenv("OFP_STREAM_KERNEL", mode)
        else:
            monkeypatch.delenv("OFP_STREAM_KERNEL", raising=False)
        od = detection.AmplitudeOnsetDetector(C, B, sr=sc.SR, **kw)
        od.init_minmax_tracker(np.array(x[: sc.WARM]))
        rel = torch.empty((nb * B, C), dtype=torch.float32, device="cuda")
        rec = torch.zeros((n_exp + 64, 16), dtype=torch.uint8, device="cuda")
        cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
        k = 0
        for n in sc.CALL_SPLIT + (nb - sum(sc.CALL_SPLIT),):
            od.process(xd[k * B:(k + n) * B], n, k * B, rel[k * B:(k + n) * B], rec, cnt)
            k += n
        torch.cuda.synchronize()
        assert k == nb
        count = int(cnt.item())
        recs = rec.cpu().numpy().view(detection.ONSET_DTYPE).reshape(-1)
        assert count == n_exp, (mode, count, n_exp)
        assert np.array_equal(recs["channel"][:count], ref["channels"]), mode
        assert np.array_equal(recs["sample"][:count], ref["samples"]), mode
        assert not recs["clip"].any() and not rec.cpu().numpy()[count:].any()
        assert np.array_equal(bits(rel.cpu().numpy()), bits(ref["rel"])), mode
        st, raw = device_state(od, C)
        for key, want in ref["state"].items():
            got = st[key]
            assert got.shape == want.shape, key
            if want.dtype == np.float32:
                assert np.array_equal(bits(got), bits(want)), (mode, key)
            elif want.dtype == np.float64:
                assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), (mode, key)
            else:
                assert np.array_equal(got.astype(np.int64), want.astype(np.int64)), (mode, key)
        raws.append(raw)
    n_state = raws[0].size - B * C * 4  # (the trailing scratch block of the state is not state)
    assert np.array_equal(raws[0][:n_state], raws[1][:n_state])


@pytest.mark.parametrize("name", sorted(sc.INIT_CASES))
def test_init_calibration_with_several_workgroups_matches_the_oracle(name):
    """AmplitudeOnsetDetector.init at 65 and 130 channels (k_calibrate: two and three workgroups of 64 lanes, the
    last one partial): thresholds, mins / maxs / noise_max of every channel and the records and rel of the blocks that
    follow, bit for bit the oracle's."""
    from onset_fingerprinting_amd import detection
    cfg = sc.INIT_CASES[name]
    d, _, ch, de, blk, rel = run_init_case(
        lambda C, B, sr, kw: detection.AmplitudeOnsetDetector(C, B, sr=sr, **kw), cfg)
    o, _, och, ode, oblk, orel = sc.init_reference(name)
    for key in ("on_threshold", "off_threshold", "mins", "maxs", "noise_max"):
        a, b = getattr(d, key), getattr(o, key)
        assert np.asarray(a).dtype == np.float32 and np.asarray(a).shape == (cfg["C"],), key
        assert np.array_equal(bits(a), bits(b)), key
    assert np.array_equal(ch, och) and np.array_equal(de, ode) and np.array_equal(blk, oblk)
    assert np.array_equal(bits(rel), bits(orel))


# ---- B: hop sessions ------------------------------------------------------------------------------------------

def session_form(sess):
    """"fused" when the session can join a HopSessionGroup (which then gives it back), "nodes" when the library
    refuses it as a five-node graph."""
    from onset_fingerprinting_amd import realtime
    from onset_fingerprinting_amd._lib import OnsetFPError
    try:
        group = realtime.HopSessionGroup([sess])
    except OnsetFPError as e:
        assert "five-node graph" in str(e)
        assert sess._group is None
        return "nodes"
    group.close()
    assert sess._group is None
    return "fused"


def make_session(cfg, clf, **extra):
    from onset_fingerprinting_amd import realtime
    ring = 0.0 if cfg["ring_min"] else 0.1
    sess = realtime.HopSession(cfg["C"], cfg["B"], sr=cfg["sr"], n_fft=cfg["F"], n_mels=cfg.get("n_mels", 40),
                               classifier=clf, want_rel=True, ring_seconds=ring, **extra)
    if cfg["ring_min"]:
        assert sess.ring_samples == max(cfg["F"], cfg["B"])
    return sess


def classifier_of(cfg):
    from onset_fingerprinting_amd.pipeline import seeded_fcnn
    return seeded_fcnn(cfg["n_mels"], cfg["n_out"]) if cfg["n_out"] else None


def mel_reference(x, nb, B, F, sr, n_mels):
    """spectral_reference of tests/test_gpu_stream.py without a classifier."""
    C = x.shape[1]
    xp = np.concatenate([np.zeros((F - B, C), np.float32), x[: nb * B]]) if F >= B else x[B - F: nb * B]
    P = oracle.dense_power_frames(xp, F, B)
    return xp, P @ oracle.mel_filterbank(sr, F, n_mels).astype(np.float64).T


def check_mel(got, mel_ref):
    """The mel half of check_spectral."""
    mel = np.stack(got["mel"], axis=1)
    assert mel.shape == mel_ref.shape
    live = mel_ref > 0
    assert np.array_equal(mel[~live], mel_ref[~live])
    assert (np.abs(mel - mel_ref)[live] / mel_ref[live]).max() < RTOL
    return mel


@pytest.mark.parametrize("graph", ["default", "nodes"])
@pytest.mark.parametrize("case", list(sc.HOP_CASES))
def test_hop_session_shapes_match_the_oracle_hop_by_hop(case, graph, monkeypatch):
    """graph = "default": OFP_HOP_GRAPH unset, the session takes the form the table states (asserted); "nodes": the
    five-node graph for every case."""
    from onset_fingerprinting_amd.data import MelBank, stft_power_mel_dense, stft_power_mel_mlp_dense
    if graph == "nodes":
        monkeypatch.setenv("OFP_HOP_GRAPH", "nodes")
    else:
        monkeypatch.delenv("OFP_HOP_GRAPH", raising=False)
    cfg = sc.HOP_CASES[case]
    C, B, F, sr, n_mels, nb = cfg["C"], cfg["B"], cfg["F"], cfg["sr"], cfg["n_mels"], cfg["hops"]
    x = sc.hop_input(case)[: nb * B]
    clf = classifier_of(cfg)
    sess = make_session(cfg, clf)
    form = session_form(sess)
    assert form == ("fused" if graph == "default" and sc.HOP_FUSED[case] else "nodes")
    odet = oracle.OracleDetector(C, B, sr=sr)
    warm = np.array(sc.hop_input(case)[: sc.WARM])
    sess.init_minmax_tracker(warm)
    odet.init_minmax_tracker(warm)
    got, exp, n = replay(sess, odet, x, B)
    assert n == nb and len(exp["on"]) >= 3
    assert got["ch"] == exp["ch"] and got["on"] == exp["on"]
    assert np.array_equal(bits(np.concatenate(got["rel"])), bits(np.concatenate(exp["rel"])))
    # the fp64 oracle; the figures first, then the assertions
    if clf is not None:
        xp, mel_ref, log_ref = spectral_reference(x, nb, B, F, sr, n_mels, clf)
    else:
        xp, mel_ref = mel_reference(x, nb, B, F, sr, n_mels)
    mel_got = np.stack(got["mel"], axis=1)
    live = mel_ref > 0
    mel_err = float((np.abs(mel_got - mel_ref)[live] / mel_ref[live]).max())
    log_err = float("nan")
    if clf is not None:
        log_err = float(np.abs(np.stack(got["logits"], axis=1) - log_ref).max() / np.abs(log_ref).max())
    print(f"\n{case} [{graph}]: form {form}, {nb} hops, {len(exp['on'])} onsets, mel err {mel_err:.3g}, "
          f"logit err {log_err:.3g} (relative to the fp64 oracle)")
    if clf is not None:
        mel, logits = check_spectral(got, mel_ref, log_ref)
    else:
        mel = check_mel(got, mel_ref)
        assert all(v is None for v in got["logits"])
    # an empty band's value is exactly 0, in every frame
    lens = (oracle.mel_filterbank(sr, F, n_mels) != 0).sum(axis=1)
    assert int((lens == 0).sum()) == cfg["empty"]
    assert not mel[:, :, lens == 0].any() and not np.signbit(mel[:, :, lens == 0]).any()
    # ... and bit for bit what the dense kernel gives on the same (zero-prefixed) stream
    bank = MelBank(sr, F, n_mels)
    if clf is not None:
        _, dmel, dlog = stft_power_mel_mlp_dense(dev(xp)[None], F, B, bank, clf.device_mlp(0))
        assert np.array_equal(bits(dlog[0].cpu().numpy()), bits(logits))
    else:
        _, dmel = stft_power_mel_dense(dev(xp)[None], F, B, bank, want_power=False)
    assert np.array_equal(bits(dmel[0].cpu().numpy()), bits(mel))
    # the ring buffer holds the stream
    R = min(sess.ring_samples, 5 * B + 3)
    assert np.array_equal(sess.audio(R), x[nb * B - R: nb * B])
    assert sess.current_index == nb * B
    sess.close()


def test_more_than_127_bands_are_refused_and_the_process_stays_usable():
    from onset_fingerprinting_amd import realtime
    from onset_fingerprinting_amd._lib import OnsetFPError
    with pytest.raises(OnsetFPError, match="at most 127 bands"):
        realtime.HopSession(2, 64, sr=48000, n_fft=1024, n_mels=128, ring_seconds=0.1)
    sess = realtime.HopSession(2, 64, sr=48000, n_fft=1024, n_mels=127, ring_seconds=0.1)
    x = sc.hop_input("2x64x256-1band")
    r = sess(np.array(x[:64]))
    P = oracle.dense_power_frames(np.concatenate([np.zeros((960, 2), np.float32), x[:64]]), 1024, 64)[:, 0]
    mel_ref = P @ oracle.mel_filterbank(48000, 1024, 127).astype(np.float64).T
    big = mel_ref >= 1e-5 * mel_ref.max()  # (as test_wide_session_takes_the_five_node_graph_and_the_one_lane_kernel)
    assert (np.abs(r["mel"] - mel_ref)[big] / mel_ref[big]).max() < RTOL
    sess.close()


@pytest.mark.parametrize("graph", ["default", "nodes"])
@pytest.mark.parametrize("case", list(sc.STRENGTH_CASES))
def test_onset_strength_and_tempogram_at_the_short_frames(case, graph, monkeypatch):
    """hop_strength_body at 256 and 512 points: 16 / 32 frame lanes inside a workgroup of 64 (nodes) or 256 (fused)
    lanes whose idle lanes take part in every reduction.  The error expression and RTOL of
    test_per_hop_onset_strength_matches_the_oracle_restatement."""
    from onset_fingerprinting_amd import realtime
    if graph == "nodes":
        monkeypatch.setenv("OFP_HOP_GRAPH", "nodes")
    else:
        monkeypatch.delenv("OFP_HOP_GRAPH", raising=False)
    cfg = sc.STRENGTH_CASES[case]
    C, B, F, sr, W = cfg["C"], cfg["B"], cfg["F"], cfg["sr"], sc.STRENGTH_KW["tg_win_length"]
    x = sc.strength_input(case)
    sess = realtime.HopSession(C, B, sr=sr, n_fft=F, ring_seconds=0.0 if cfg["ring_min"] else 0.1,
                               onset_strength=dict(sc.STRENGTH_KW))
    if cfg["ring_min"]:
        assert sess.ring_samples == max(F, B)
    assert session_form(sess) == ("fused" if graph == "default" else "nodes")
    ref = oracle.HopStrength(F, C, sc.STRENGTH_KW["max_length"], sc.STRENGTH_KW["avg_length"], sc.STRENGTH_KW["ring"],
                             tg_win_length=W)
    worst = worst_tg = 0.0
    for i in range(cfg["hops"]):
        hop = np.array(x[i * B:(i + 1) * B])
        r = sess(hop)
        want = ref(hop)
        err = np.abs(r["strength"] - want) / (np.abs(want) + 1e-2)
        worst = max(worst, float(err.max()))
        assert err.max() < RTOL, (i, r["strength"], want)
        tg_err = np.abs(r["tempogram"] - ref.tempogram()).max()
        worst_tg = max(worst_tg, float(tg_err))
        assert r["tempogram"].shape == (W,) and tg_err < RTOL, i
    print(f"\nstrength {case} [{graph}]: {cfg['hops']} hops, worst strength err {worst:.3g}, tempogram err {worst_tg:.3g}")
    assert worst > 0 and cfg["hops"] >= 150
    assert np.array_equal(sess.audio(sess.ring_samples if cfg["ring_min"] else 3 * B + 1),
                          x[-(sess.ring_samples if cfg["ring_min"] else 3 * B + 1):])
    sess.close()


def test_group_of_two_wide_members_equals_their_twins():
    """Two members at both limits of the one-kernel form (128 channels, hop 64: two waves of channel lanes, 96 KiB of
    detector planes per member) with different streams: every output of every hop is bit for bit the stand-alone
    twin's."""
    from onset_fingerprinting_amd import realtime
    case = "128x64x256"
    cfg = sc.HOP_CASES[case]
    C, B, nb = cfg["C"], cfg["B"], cfg["hops"]
    xs = [sc.hop_input(case, seed) for seed in (0, 1)]
    assert not np.array_equal(xs[0], xs[1])
    clf = classifier_of(cfg)
    members = [make_session(cfg, clf) for _ in xs]
    twins = [make_session(cfg, clf) for _ in xs]
    for m, t, x in zip(members, twins, xs):
        m.init_minmax_tracker(np.array(x[: sc.WARM]))
        t.init_minmax_tracker(np.array(x[: sc.WARM]))
    group = realtime.HopSessionGroup(members)
    n_on = [0, 0]
    for i in range(nb):
        hops = np.stack([x[i * B:(i + 1) * B] for x in xs])
        got = group(hops)
        for s in range(2):
            want = twins[s](np.array(hops[s]))
            assert got[s].keys() == want.keys()
            for key in ("channels", "onsets"):
                assert np.array_equal(got[s][key], want[key]), (s, i, key)
            for key in ("rel", "mel", "logits"):
                assert np.array_equal(bits(got[s][key]), bits(want[key])), (s, i, key)
            n_on[s] += len(want["onsets"])
    assert min(n_on) >= 100
    for m, t in zip(members, twins):
        assert m.current_index == t.current_index == nb * B
        assert np.array_equal(bits(m.audio(m.ring_samples)), bits(t.audio(t.ring_samples)))
    group.close()
    for s in members + twins:
        s.close()
