"""The fp64 references, error bars and shape tables of oracle/spectral_kernels.py, checked without a GPU.

1. Every reference agrees with an independent formulation to 1e-12 (a direct DFT sum, oracle.dense_power_frames,
   oracle.stft_frame, oracle.power_to_db + scipy's DCT, explicit loops).
2. The fp32 emulation of the plan of csrc/ofp_fft.h stays within A, B and every derived bound at every size and
   input family; A and B are twice what it reaches.
3. The same emulation with one planted fault leaves its bar: the bars would catch a subtly wrong kernel.
4. The tables reach every path and cap that tests/test_gpu_spectral_kernels.py claims to reach.
"""
import math

import numpy as np
import pytest
import scipy.fft

import oracle
from oracle import spectral_kernels as K

f32, f64 = np.float32, np.float64


def windowed(fr, w):
    return fr * np.asarray(w, f64).astype(f32)


# ---- 1. references against independent formulations --------------------------------------------------------------

def test_transform_references_agree_with_independent_formulations():
    rng = np.random.default_rng(1)
    x = rng.standard_normal((3, 3000, 2)).astype(f32)
    for n_fft, hop in ((256, 64), (512, 37), (1024, 1031)):
        for clip in range(3):
            ref = oracle.dense_power_frames(x[clip], n_fft, hop)
            got = K.dense_power_ref(x[clip:clip + 1], n_fft, hop)[0]
            assert got.shape == ref.shape and np.abs(got - ref).max() <= 1e-12 * ref.max()
    # the gathered frames: a direct DFT sum, the pad of an odd difference, clipped starts and valid ranges
    n_fft, L = 256, 201
    win = np.zeros(n_fft)
    win[(n_fft - L) // 2:(n_fft - L) // 2 + L] = rng.random(L)
    starts = np.array([-50, 0, 7, 2900, 2999, 3100, 500, 500])
    lo = np.array([0, 0, 0, 0, 0, 0, 520, 0])
    hi = np.array([3000, 3000, 3000, 3000, 3000, 3000, 3000, 600])
    clip = np.array([0, 1, 2, 0, 1, 2, 0, 1])
    ch = np.array([0, 1, 0, 1, 0, 1, 1, 0])
    X = K.frames_ref(x, starts, L, n_fft, win, lo, hi, clip, ch)
    n = np.arange(n_fft)
    D = np.exp(-2j * np.pi * np.outer(np.arange(n_fft // 2 + 1), n) / n_fft)
    for f in range(len(starts)):
        fr = np.zeros(n_fft)
        for q in range(L):
            i = starts[f] + q
            if lo[f] <= i < hi[f] and 0 <= i < 3000:
                fr[(n_fft - L) // 2 + q] = x[clip[f], i, ch[f]]
        assert np.abs(X[f] - D @ (fr * win)).max() <= 1e-12 * max(np.abs(X[f]).max(), 1.0), f
    assert np.abs(X[5]).max() == 0.0  # a frame past the end is all zeros
    # ... and the reference's own stft_frame (centre padding)
    seg = x[1, 7:7 + L, 0]
    ref = oracle.stft_frame(seg, n_fft, win)
    got = K.frames_ref(x, [7], L, n_fft, win, 0, 3000, [1], [0])[0]
    assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max()
    assert np.abs(K.hann_periodic64(4096) - oracle.hann_periodic(4096)).max() <= 1e-15


def test_mel_mfcc_flux_references_agree_with_independent_formulations():
    rng = np.random.default_rng(2)
    for sr, n_fft, n_mels, fmin, fmax, _ in K.MEL_CASES:
        n_mels = n_mels or 100
        fb = oracle.mel_filterbank(sr, n_fft, n_mels, fmin, fmax)
        P = (rng.standard_normal((3, n_fft // 2 + 1)) ** 2).astype(f32)
        ref, _ = K.mel_ref(P, fb)
        lo, ln, off, w = K.band_csr(fb)
        for b in range(n_mels):
            s = sum(f64(P[1, lo[b] + k]) * f64(w[off[b] + k]) for k in range(ln[b]))
            assert abs(ref[1, b] - s) <= 1e-12 * max(abs(s), 1e-300), (n_fft, n_mels, b)
    for rows, n_mels, n_mfcc, top_db, kind in K.MFCC_CASES[:-1]:
        mel = K.mfcc_mel(rows, n_mels, kind)
        ref, _ = K.mfcc_ref(mel, K.dct_ortho64(n_mfcc, n_mels), top_db=top_db)
        db = oracle.power_to_db(mel.astype(f64), amin=f64(f32(1e-10)), top_db=top_db)
        ind = scipy.fft.dct(db, axis=-1, type=2, norm="ortho")[:, :n_mfcc]
        assert np.abs(ref - ind).max() <= 1e-12 * np.abs(ind).max(), (rows, n_mels, n_mfcc, top_db, kind)
    P = (rng.standard_normal((5, 65)) ** 2).astype(f32)
    w = rng.random(65).astype(f32)
    ref, _ = K.flux_ref(P, w)
    for t in range(4):
        s = sum(max(0.0, f64(w[k]) * (math.sqrt(P[t + 1, k]) - math.sqrt(P[t, k]))) for k in range(65)) / 65
        assert abs(ref[t] - s) <= 1e-12 * s
    a = rng.standard_normal((500, 3)).astype(f32)
    on = np.array([[40, 50, 45], [300, 280, 290]])
    assert np.array_equal(K.extract_ref(a, np.repeat(on.min(1)[:, None] - 16, 3, 1), 64),
                          oracle.frame_extract(a, on, 64, 16))
    assert np.array_equal(K.extract_ref(a, [[-3, 498, 600]], 4)[0],
                          np.array([[0, 0, 0, a[0, 0]], [a[498, 1], a[499, 1], 0, 0], [0, 0, 0, 0]], f32))


# ---- 2. the emulation stays inside every bar -----------------------------------------------------------------------

@pytest.fixture(scope="module")
def ab():
    return K.measure_ab()


def test_a_and_b_are_twice_what_the_emulation_reaches(ab):
    r2 = max(v[0] for v in ab.values())
    rmax = max(v[1] for v in ab.values())
    print(f"\nemulation: largest 2-norm ratio {r2:.3f}, largest bin ratio {rmax:.3f}; A = {K.A}, B = {K.B}")
    for F in K.NFFT:
        print(F, {n: (round(ab[(F, n)][0], 2), round(ab[(F, n)][1], 2)) for n in K.FAMILIES})
    # the recorded ratios are what the emulation reaches (a different build of pocketfft may move them a little)
    assert r2 <= K.R2_EMU <= 1.05 * r2 and rmax <= K.RMAX_EMU <= 1.05 * rmax
    assert K.A == 2 * K.R2_EMU and K.B == 2 * K.RMAX_EMU
    assert K.A <= 2 * 3.5 and K.B <= 2 * 9  # no more than twice the orientation values: nothing to explain
    # exact stand-ins exist (and the emulation is exact there): the all-zero frame and the one-hot at F/2
    for F in K.NFFT:
        assert ab[(F, "zero")] == (0.0, 0.0) and ab[(F, "onehot_half")] == (0.0, 0.0)


@pytest.mark.parametrize("n_fft", K.NFFT)
def test_emulated_transform_within_bars_every_family(n_fft):
    w = K.hann_periodic64(n_fft)
    for name, fr in K.family_frames(n_fft).items():
        X, e2, emax = K.stand_in(fr, w)
        r2, rm = K.complex_ratios(K.emu_rfft(windowed(fr, w)), X, e2, emax)
        rel, rp2 = K.power_ratios(K.emu_power(windowed(fr, w)), X, e2, emax)
        assert max(r2.max(), rm.max()) <= 0.5 + 1e-9 and max(rel.max(), rp2.max()) <= 1.0, (name, r2.max(), rm.max(),
                                                                                         rel.max(), rp2.max())
        if name in ("zero", "onehot_half"):
            assert (e2 == 0).all()  # an exact stand-in: the bars demand exact output
        if name.startswith("onehot"):  # flat magnitude: a permutation fault of the autosort would show
            assert np.allclose(np.abs(X), np.abs(X[:, :1]), rtol=1e-12)
    # the two split forms agree to rounding
    fr = K.family_frames(n_fft)["noise"][:4]
    G, P = K.emu_rfft(windowed(fr, w)).astype(np.complex128), K.emu_power(windowed(fr, w))
    assert np.abs(P - np.abs(G) ** 2).max() <= 1e-5 * P.max()


@pytest.mark.parametrize("case", K.MEL_CASES, ids=lambda c: c[5])
def test_emulated_mel_within_bound(case):
    sr, n_fft, n_mels, fmin, fmax, _ = case
    n_mels = n_mels or K.largest_band_count(oracle.mel_filterbank, sr, n_fft)
    fb = oracle.mel_filterbank(sr, n_fft, n_mels, fmin, fmax)
    w = K.hann_periodic64(n_fft)
    fam = K.family_frames(n_fft, reps=2)
    fr = np.concatenate([fam[k] for k in ("noise", "tone", "hit", "zero", "onehot_1")])
    X, e2, emax = K.stand_in(fr, w)
    P32 = K.emu_power(windowed(fr, w))
    # fused: from the true power with the bar of every bin; ofp_mel: from the fp32 power as given
    ref, bound = K.mel_ref(np.abs(X) ** 2, fb, K.power_bar(X, emax))
    got = K.emu_mel(P32, fb).astype(f64)
    assert (np.abs(got - ref) <= bound).all(), np.max(np.abs(got - ref) / np.maximum(bound, 1e-300))
    ref, bound = K.mel_ref(P32, fb)
    assert (np.abs(got - ref) <= bound).all(), np.max(np.abs(got - ref) / np.maximum(bound, 1e-300))


@pytest.mark.parametrize("case", K.MFCC_CASES, ids=lambda c: "-".join(map(str, c)))
def test_emulated_mfcc_within_bound(case):
    rows, n_mels, n_mfcc, top_db, kind = case
    mel = K.mfcc_mel(rows, n_mels, kind)
    dct = K.dct_ortho64(n_mfcc, n_mels).astype(f32)
    ref, bound = K.mfcc_ref(mel, dct, top_db=top_db)
    got = K.emu_mfcc(mel, dct, top_db=top_db).astype(f64)
    assert np.isfinite(ref).all() and (np.abs(got - ref) <= bound).all(), np.max(np.abs(got - ref) / bound)
    if top_db is not None and kind != "all_zero":  # the derivation's condition on the floor
        db_max = 10 * np.log10(mel.max())
        assert abs(db_max - top_db) >= abs(db_max)


def flux_power(rng, n_frames, n_bins):
    p = (rng.standard_normal((n_frames, n_bins)) ** 2 * 10.0 ** rng.uniform(-4, 2, (n_frames, 1))).astype(f32)
    p[rng.random(p.shape) < 0.05] = 0.0
    return p, rng.random(n_bins).astype(f32)


def test_emulated_flux_within_bound():
    rng = np.random.default_rng(5)
    for n_bins in K.FLUX_BINS:
        for n_frames in K.FLUX_FRAMES:
            p, w = flux_power(rng, n_frames, n_bins)
            p[1] = p[0]  # two identical frames: exactly 0
            ref, bound = K.flux_ref(p, w)
            got = K.emu_flux(p, w).astype(f64)
            assert ref[0] == 0 and bound[0] > 0 and got[0] == 0
            assert (np.abs(got - ref) <= bound).all(), (n_bins, n_frames)


# ---- 3. planted faults ---------------------------------------------------------------------------------------------

def leaves(fr, w_true, wx, fault=None):
    """Does the emulation of the (faulty) plan leave a bar of the complex and of the power output?"""
    X, e2, emax = K.stand_in(fr, w_true)
    r2, rm = K.complex_ratios(K.emu_rfft(wx, fault), X, e2, emax)
    rel, rp2 = K.power_ratios(K.emu_power(wx, fault), X, e2, emax)
    return max(r2.max(), rm.max()) > 1.0, max(rel.max(), rp2.max()) > 1.0


@pytest.mark.parametrize("n_fft", K.NFFT)
def test_planted_transform_faults_leave_the_bars(n_fft):
    w = K.hann_periodic64(n_fft)
    fam = K.family_frames(n_fft, reps=4)
    fr = np.concatenate([fam["noise"], fam["tone"]])
    assert leaves(fr, w, windowed(fr, w)) == (False, False)
    n = np.arange(n_fft)
    sym = 0.5 - 0.5 * np.cos(2 * np.pi * n / (n_fft - 1))
    assert leaves(fr, w, windowed(fr, sym)) == (True, True), f"symmetric Hann at {n_fft}"
    assert leaves(fr, w, windowed(fr, np.roll(w, 1))) == (True, True), f"window shifted by one sample at {n_fft}"
    late = np.roll(fr, -1, axis=1)
    assert leaves(fr, w, windowed(late, w)) == (True, True), f"frame read one sample late at {n_fft}"
    assert leaves(fr, w, windowed(fr, w), "swap") == (True, True), f"bins p and M - p swapped at {n_fft}"
    assert leaves(fr, w, windowed(fr, w), "nyquist") == (True, True), f"Nyquist bin dropped at {n_fft}"
    # twiddles W^k = W^(k-1) W^1 in fp32: off by 23 to 180 U at the last twiddle -- except at 512 points, where the
    # rounding of W_256^1 happens to keep the recurrence within 3 U of the exact table: no fault to catch there
    c, s = K.twiddles(n_fft // 2, n_fft // 2, "recurrence")
    c0, s0 = K.twiddles(n_fft // 2, n_fft // 2)
    drift = np.abs((c - c0) + 1j * (s - s0)).max() / K.U
    if n_fft == 512:
        assert drift < 3
    else:
        assert drift > 20
        assert leaves(fr, w, windowed(fr, w), "recurrence") == (True, True), f"fp32 twiddle recurrence at {n_fft}"
    # the one-hot frames alone catch the permutation fault
    one = fam["onehot_last"]
    assert leaves(one, w, windowed(one, w), "swap")[0], n_fft


def test_planted_mel_mfcc_flux_faults_leave_the_bounds():
    rng = np.random.default_rng(6)
    fb = oracle.mel_filterbank(K.MEL_SR, 1024, 40)
    assert K.band_csr(fb)[1].max() > K.MEL_SEG  # a band with a second segment
    P = (rng.standard_normal((4, 513)) ** 2).astype(f32)
    ref, bound = K.mel_ref(P, fb)
    assert (np.abs(K.emu_mel(P, fb) - ref) <= bound).all()
    for fault in ("tap", "lo"):
        assert (np.abs(K.emu_mel(P, fb, fault) - ref) > bound).any(), f"mel {fault} at 1024 / 40"
    dct = K.dct_ortho64(14, 40).astype(f32)
    mel = K.mfcc_mel(5, 40, "below_floor")
    ref, bound = K.mfcc_ref(mel, dct)
    assert (np.abs(K.emu_mfcc(mel, dct) - ref) <= bound).all()
    assert (np.abs(K.emu_mfcc(mel, dct, fault="row_max") - ref) > bound).any(), "MFCC floor from the row maximum"
    mel = K.mfcc_mel(5, 40, "zeros")
    ref, bound = K.mfcc_ref(mel, dct, top_db=None)
    assert (np.abs(K.emu_mfcc(mel, dct, top_db=None) - ref) <= bound).all()
    assert not (np.abs(K.emu_mfcc(mel, dct, top_db=None, fault="amin") - ref) <= bound).all(), "MFCC amin not applied"
    p, w = flux_power(rng, 6, 129)
    ref, bound = K.flux_ref(p, w)
    for fault in ("abs", "n_minus_1"):
        assert (np.abs(K.emu_flux(p, w, fault) - ref) > bound).any(), f"flux {fault} at 129 bins"


# ---- 4. the tables reach what they claim -------------------------------------------------------------------------

def test_grid_stride_cases_pass_the_grid_cap_on_the_path_they_name():
    by_path = {}
    for c in K.STRIDE_CASES:
        F, fpw = c["n_fft"], K.FPW[c["n_fft"]]
        assert c["total"] > K.GRID_CAP * fpw, c["name"]                 # a second grid iteration
        assert c["total"] == c["n_clips"] * c["C"] * (1 + (c["N"] - F) // c["hop"])
        groups = -(-c["total"] // fpw)
        assert groups % K.GRID_CAP != 0                                 # the last iteration is not full
        # ... and the last iteration holds slots without a frame, per mapping of k_stft_power:
        grid = min(groups, K.GRID_CAP)
        if c["path"] == "plain":    # groups of FPW consecutive frames, interleaved over the workgroups
            assert fpw == 1 or c["total"] % fpw != 0, c["name"]         # (FPW = 1: the short last iteration is all)
        elif c["path"] == "slide":  # every slot owns n_it consecutive frames
            n_it = -(-groups // grid)
            assert n_it >= 2 and grid * fpw * n_it > c["total"] > grid * fpw * (n_it - 1), c["name"]
        else:                       # il: every run of C slots owns n_it consecutive row-frames (clip, hop)
            runs, total_rf = grid * (fpw // c["C"]), c["total"] // c["C"]
            n_it = -(-total_rf // runs)
            assert n_it >= 2 and runs * n_it > total_rf > runs * (n_it - 1), c["name"]
        assert c["total"] * (F // 2 + 1) * 4 < 40e6                     # output size
        base_mod8 = 4 * c["base_off"]
        assert K.dispatch(F, c["stride"], c["hop"], c["C"], base_mod8) == c["path"], c["name"]
        by_path.setdefault((c["path"], c["layout"]), set()).add(F)
        if c["layout"] == "planar":
            assert c["stride"] >= c["N"] and c["stride"] % 2 == ("oddstride" in c["name"])
            aligned, straddling = K.straddles(F, c["stride"], c["hop"], c["n_clips"] * c["C"], c["H"], base_mod8)
            if c["path"] == "slide":
                assert straddling == 0
            elif "off4" in c["name"]:
                assert aligned == 0
            else:
                assert aligned > 0.2 and straddling > 0.2, c["name"]    # both load forms in one launch
    assert by_path[("plain", "interleaved")] == set(K.NFFT) and by_path[("plain", "planar")] == set(K.NFFT)
    assert by_path[("slide", "planar")] == {256, 512, 1024, 2048} and by_path[("il", "interleaved")] == {256, 512, 1024}
    assert [K.INTERLEAVED_HOP[F] for F in K.NFFT] == [4, 8, 8, 16, 64]
    # what keeps a 4096-point planar input, an odd channel count and a misaligned base off the sliding paths
    assert K.dispatch(4096, 8192, 1024, 3) == "plain" and K.dispatch(1024, 0, 256, 3) == "plain"
    assert K.dispatch(1024, 0, 256, 8, 2) == "plain" and K.dispatch(2048, 0, 512, 4) == "plain"
    assert K.FPW == {F: (512 if F == 1024 else 256) // max(16, min(F // 16, 64 if F <= 2048 else F // 16)) for F in K.NFFT}
    assert all(math.prod(K.RADICES[F // 2]) == F // 2 for F in K.NFFT)


def test_mel_and_cap_tables():
    for sr, n_fft, n_mels, fmin, fmax, what in K.MEL_CASES:
        bins = n_fft // 2 + 1
        if n_mels is None:
            n_mels = K.largest_band_count(oracle.mel_filterbank, sr, n_fft)
            more = len(K.band_csr(oracle.mel_filterbank(sr, n_fft, n_mels + 1))[3])
            assert not K.mel_admitted(more, n_mels + 1, bins)
        lo, ln, off, w = K.band_csr(oracle.mel_filterbank(sr, n_fft, n_mels, fmin, fmax))
        assert K.mel_admitted(len(w), n_mels, bins), what
        assert (ln == 0).any() == (what == "empty bands"), what
    for bins, n_mels, ln, why in K.MEL_REJECTED:
        assert not K.mel_admitted(n_mels * ln, n_mels, bins), why
    assert K.mel_admitted(127 * 8, 127, 2049) and K.mel_admitted(127 * 32, 127, 2049) and K.mel_admitted(10 * 50, 10, 129)
    assert K.ELEM_CAP == 1048576
    rows, n_mels, n_mfcc = K.MFCC_CASES[-1][:3]
    assert rows * n_mfcc > K.ELEM_CAP
    assert {c[1] for c in K.MFCC_CASES} >= {1, 40, 127} and {c[2] for c in K.MFCC_CASES} >= {1, 14, 40, 127}
    assert {c[3] for c in K.MFCC_CASES} == {80.0, None}
