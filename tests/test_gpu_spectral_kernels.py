"""The spectral kernels of csrc/ofp_spectral.hip and csrc/ofp_onset_spectral.hip one by one against the fp64
references and error bars of oracle/spectral_kernels.py: k_stft_power past the grid cap on every load path and
size (all frames compared), its small edges, k_stft_frames, the mel / MFCC / flux kernels at their ragged sizes
and the exact kernels.  tests/test_spectral_kernels_cpu.py shows that the bars hold for a correct fp32 evaluation
of the same plan and catch planted faults.

Outputs are written into NaN-filled buffers with a guard tail, so an element that was not written or a store past
the end fails as well.  `pytest -s` prints the largest error / bar of every primitive and path.
"""
import ctypes
import types

import numpy as np
import pytest
import torch

import oracle
from oracle import spectral_kernels as K

pytestmark = pytest.mark.gpu

f32, f64 = np.float32, np.float64
GUARD = 64
RATIOS = {}


@pytest.fixture(scope="module", autouse=True)
def report_ratios():
    yield
    for name in sorted(RATIOS):
        print(f"\nlargest error / bar, {name}: {RATIOS[name]:.3f}", end="")
    print()


def L():
    from onset_fingerprinting_amd import _lib
    return _lib.lib()


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def ok(rc, what):
    from onset_fingerprinting_amd import _lib
    _lib.check(rc, what)


def err_type():
    from onset_fingerprinting_amd import _lib
    return _lib.OnsetFPError


def dev(a, dt=f32):
    return torch.from_numpy(np.ascontiguousarray(a, dt)).cuda()


def guarded(*shape, dtype=torch.float32):
    """(view of `shape`, whole buffer): NaN everywhere, GUARD elements behind the view."""
    numel = int(np.prod(shape))
    buf = torch.full((numel + GUARD,), float("nan"), dtype=dtype, device="cuda")
    return buf[:numel].view(*shape), buf


def guard_ok(buf):
    return bool(torch.isnan(buf[-GUARD:]).all())  # (a complex element is NaN when either part is)


def note(name, ratio):
    RATIOS[name] = max(RATIOS.get(name, 0.0), float(ratio))


def within(name, got, ref, bound, ctx, buf=None):
    if buf is not None:
        assert guard_ok(buf), (name, ctx, "store past the end of the output")
    got = got.detach().cpu().numpy().astype(f64) if torch.is_tensor(got) else np.asarray(got, f64)
    assert got.shape == ref.shape, (name, ctx, got.shape, ref.shape)
    r = K._ratio(np.abs(got - ref), bound)
    note(name, r.max() if r.size else 0.0)
    assert bool((r <= 1.0).all()), (name, ctx, f"error / bar = {r.max():.3g} at {np.argwhere(r > 1.0)[:4].tolist()}")


def check_transform(name, xs, n_fft, hop, P=None, mel=None, fb=None, ctx=None):
    """Every frame of every series of xs [n_series, N] against fp64: P [n_series, H, bins], mel [n_series, H, n_mels]
    (or a list of such outputs of several runs on the same input; the references are computed once)."""
    w = K.hann_periodic64(n_fft)
    Ps = [p for p in (P if isinstance(P, list) else [P]) if p is not None]
    mels = [m for m in (mel if isinstance(mel, list) else [mel]) if m is not None]
    for cc in range(xs.shape[0]):
        X, e2, emax = K.stand_in(K.dense_frames(xs[cc], n_fft, hop), w)
        for i, p in enumerate(Ps):
            assert p[cc].shape == X.shape, (name, ctx, p[cc].shape, X.shape)
            r_el, r_2 = K.power_ratios(p[cc], X, e2, emax)
            note(f"k_stft_power {name}, bins", r_el.max())
            note(f"k_stft_power {name}, 2-norm", r_2.max())
            assert r_el.max() <= 1.0 and r_2.max() <= 1.0, (name, ctx, i, cc, float(r_el.max()), float(r_2.max()),
                                                           int(r_el.argmax()), int(r_2.argmax()))
        if mels:
            ref, bound = K.mel_ref(np.abs(X) ** 2, fb, K.power_bar(X, emax))
            for i, m in enumerate(mels):
                within(f"fused mel {name}", m[cc], ref, bound, (ctx, i, cc))


def noise_series(seed, n_series, N):
    """Broadband noise, one gain per series over six decades of power."""
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((n_series, N)) * np.exp(rng.uniform(-6, 0, (n_series, 1)))).astype(f32)


def interleave(xs, n_clips, C):
    return np.ascontiguousarray(xs.reshape(n_clips, C, -1).transpose(0, 2, 1))


# ---- k_stft_power past the grid cap, once per load path and size ---------------------------------------------------

@pytest.mark.parametrize("case", K.STRIDE_CASES, ids=lambda c: c["name"])
def test_stft_power_past_the_grid_cap(case):
    from onset_fingerprinting_amd import data
    c = case
    F, hop, n_clips, C, N, H = c["n_fft"], c["hop"], c["n_clips"], c["C"], c["N"], c["H"]
    n_series, bins = n_clips * C, F // 2 + 1
    assert c["total"] > K.GRID_CAP * K.FPW[F]
    xs = noise_series(F + hop, n_series, N)
    mb = data.MelBank(K.MEL_SR, F, 40)
    runs = []
    if c["layout"] == "interleaved":
        x = dev(interleave(xs, n_clips, C))
        assert K.dispatch(F, 0, hop, C, x.data_ptr() % 8) == c["path"]
        planar = None
        out, buf = guarded(n_clips, C, H, bins)
        data.stft_power_dense(x, F, hop, out=out)
        runs.append((out, buf, None, None))
    else:
        base = torch.zeros(n_series * c["stride"] + 2, dtype=torch.float32, device="cuda")
        base[c["base_off"]:c["base_off"] + n_series * c["stride"]].view(n_series, c["stride"])[:, :N] = dev(xs)
        addr = base.data_ptr() + 4 * c["base_off"]
        assert K.dispatch(F, c["stride"], hop, C, addr % 8) == c["path"]
        planar = (addr, c["stride"])
        x = types.SimpleNamespace(shape=(n_clips, N, C), device=base.device)
    for want_power in (True, False):
        out, buf = guarded(n_clips, C, H, bins) if want_power else (None, None)
        mel, mbuf = guarded(n_clips, C, H, 40)
        data.stft_power_mel_dense(x, F, hop, mb, out_power=out, out_mel=mel, want_power=want_power, planar=planar)
        runs.append((out, buf, mel, mbuf))
    torch.cuda.synchronize()
    for i, (out, buf, mel, mbuf) in enumerate(runs):
        assert (buf is None or guard_ok(buf)) and (mbuf is None or guard_ok(mbuf)), (c["name"], i)
    straddling = "odd" in c["name"] or "off4" in c["name"]
    check_transform(c["path"] + " " + c["layout"] + (" straddling" if straddling else ""), xs, F, hop,
                    [None if r[0] is None else r[0].cpu().numpy().reshape(n_series, H, bins) for r in runs],
                    [None if r[2] is None else r[2].cpu().numpy().reshape(n_series, H, 40) for r in runs], mb.dense,
                    c["name"])


# ---- k_stft_power, small edges ---------------------------------------------------------------------------------------

def power_gpu(x, n_fft, hop):
    from onset_fingerprinting_amd import data
    n_clips, N, C = x.shape
    H = 1 + (N - n_fft) // hop
    out, buf = guarded(n_clips, C, H, n_fft // 2 + 1)
    data.stft_power_dense(dev(x), n_fft, hop, out=out)
    assert guard_ok(buf)
    return out.cpu().numpy().reshape(n_clips * C, H, -1)


@pytest.mark.parametrize("n_fft", K.NFFT)
def test_stft_power_small_edges(n_fft):
    rng = np.random.default_rng(n_fft + 3)
    for name, n_clips, C, N, hop in (("one frame", 1, 1, n_fft, n_fft // 4), ("one frame, 64 channels", 1, 64, n_fft, 7),
                                     ("hop 1", 2, 2, n_fft + 20, 1), ("hop n_fft + 3", 2, 3, 4 * n_fft + 11, n_fft + 3)):
        xs = noise_series(rng.integers(1 << 30), n_clips * C, N)
        check_transform("small edges", xs, n_fft, hop, power_gpu(interleave(xs, n_clips, C), n_fft, hop), ctx=name)
    # n_samples == n_fft - 1: no frame; OK is returned and nothing is written
    out, buf = guarded(129)
    x = dev(rng.standard_normal((1, n_fft - 1, 2)))
    ok(L().ofp_stft_power(x.data_ptr(), 1, n_fft - 1, 2, n_fft, 64, out.data_ptr(), stream()), "ofp_stft_power")
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf).all())


@pytest.mark.parametrize("n_fft", K.NFFT)
def test_stft_power_every_input_family(n_fft):
    """One frame per family frame (hop = n_fft); an all-zero frame and the one-hot at n_fft / 2, whose single-precision
    stand-in is exact, must come out exact."""
    fam = K.family_frames(n_fft, reps=8)
    for name, fr in fam.items():
        xs = fr.reshape(1, -1)
        P = power_gpu(interleave(xs, 1, 1), n_fft, n_fft)
        check_transform("input families", xs, n_fft, n_fft, P, ctx=name)
        if name == "zero":
            assert (P == 0).all()
        if name == "onehot_half":
            assert (P == 1).all()


# ---- k_stft_frames ---------------------------------------------------------------------------------------------------

def frames_gpu(x, clip, ch, starts, lo, hi, frame_length, n_fft, win, C=None):
    n = len(starts)
    out, buf = guarded(max(n, 1), n_fft // 2 + 1, dtype=torch.complex64)
    keep = [dev(x), dev(clip, np.int32), dev(ch, np.int32), dev(starts, np.int64), dev(lo, np.int64), dev(hi, np.int64),
            dev(win)]
    n_clips, N, Cx = x.shape
    rc = L().ofp_stft_frames(keep[0].data_ptr(), n_clips, N, Cx if C is None else C, keep[1].data_ptr(), keep[2].data_ptr(),
                             keep[3].data_ptr(), keep[4].data_ptr(), keep[5].data_ptr(), n, frame_length, n_fft,
                             keep[6].data_ptr(), out.data_ptr(), stream())
    ok(rc, "ofp_stft_frames")
    torch.cuda.synchronize()
    assert guard_ok(buf)
    return out, buf


def check_frames(ctx, x, clip, ch, starts, lo, hi, frame_length, n_fft, win):
    out, _ = frames_gpu(x, clip, ch, starts, lo, hi, frame_length, n_fft, win)
    G = out.cpu().numpy()
    fr = K.gather_frames(x, starts, frame_length, n_fft, lo, hi, clip, ch)
    for i in range(0, len(starts), 8192):
        X, e2, emax = K.stand_in(fr[i:i + 8192], np.asarray(win, f32).astype(f64))
        r2, rm = K.complex_ratios(G[i:i + 8192], X, e2, emax)
        note("k_stft_frames, 2-norm", r2.max())
        note("k_stft_frames, bins", rm.max())
        assert r2.max() <= 1.0 and rm.max() <= 1.0, (ctx, float(r2.max()), float(rm.max()), i + int(rm.argmax()))


def frame_args(rng, n, n_clips, N, C, span):
    clip = rng.integers(0, n_clips, n)
    ch = rng.integers(0, C, n)
    starts = rng.integers(-span, N + span // 2, n)
    lo, hi = np.zeros(n, np.int64), np.full(n, N, np.int64)
    cut = rng.random(n)
    lo[cut < 0.2] = starts[cut < 0.2] + span // 4           # cut on the left
    hi[cut > 0.8] = starts[cut > 0.8] + span // 2           # cut on the right
    return clip, ch, starts, lo, hi


def test_stft_frames_past_the_grid_cap_three_clips_odd_pad_random_window():
    rng = np.random.default_rng(31)
    n_fft, L_, n = 256, 201, K.GRID_CAP * K.FPW[256] + K.FPW[256] + 1
    x = rng.standard_normal((3, 5000, 2)).astype(f32)
    clip, ch, starts, lo, hi = frame_args(rng, n, 3, 5000, 2, L_)
    assert set(clip) == {0, 1, 2} and (starts < 0).any() and (starts >= 5000).any()
    win = rng.standard_normal(n_fft).astype(f32)  # asymmetric, signed, non-zero in the pad as well
    check_frames("256 / 201", x, clip, ch, starts, lo, hi, L_, n_fft, win)


def test_stft_frames_4096_past_the_grid_cap_full_length():
    rng = np.random.default_rng(32)
    n_fft, n = 4096, K.GRID_CAP + 2
    x = rng.standard_normal((3, 20000, 3)).astype(f32)
    clip, ch, starts, lo, hi = frame_args(rng, n, 3, 20000, 3, n_fft)
    check_frames("4096 / 4096", x, clip, ch, starts, lo, hi, n_fft, n_fft, K.hann_periodic64(n_fft).astype(f32))


@pytest.mark.parametrize("n_fft", K.NFFT)
def test_stft_frames_small_edges(n_fft):
    rng = np.random.default_rng(n_fft + 33)
    x = rng.standard_normal((3, 3 * n_fft, 2)).astype(f32)
    for frame_length in (1, n_fft - 55, n_fft):
        clip, ch, starts, lo, hi = frame_args(rng, 37, 3, 3 * n_fft, 2, max(frame_length, 8))
        win = oracle.spectral.pad_center(oracle.hann_periodic(frame_length), n_fft).astype(f32) if frame_length > 1 \
            else rng.standard_normal(n_fft).astype(f32)
        check_frames((n_fft, frame_length), x, clip, ch, starts, lo, hi, frame_length, n_fft, win)
    # n_frames = 0: OK, nothing written
    z = np.zeros(0, np.int64)
    out, buf = frames_gpu(x, z, z, z, z, z, n_fft, n_fft, np.ones(n_fft, f32))
    assert bool(torch.isnan(buf).all())


def test_stft_frames_device_wrapper():
    """data.stft_frames_device with host arrays of other integer types and a float64 window: the wrapper's
    conversions hand the kernel what the direct calls above give it."""
    from onset_fingerprinting_amd import data
    rng = np.random.default_rng(34)
    n_fft, frame_length = 512, 301
    x = rng.standard_normal((3, 4000, 2)).astype(f32)
    clip, ch, starts, lo, hi = frame_args(rng, 41, 3, 4000, 2, frame_length)
    win = oracle.spectral.pad_center(oracle.hann_periodic(frame_length), n_fft)  # float64: rounded by the wrapper
    G = data.stft_frames_device(dev(x), clip.astype(np.int64), list(ch), starts.astype(np.int32), torch.from_numpy(lo),
                                dev(hi, np.int64), frame_length, n_fft, win)
    assert G.shape == (41, n_fft // 2 + 1) and G.dtype == torch.complex64
    fr = K.gather_frames(x, starts, frame_length, n_fft, lo, hi, clip, ch)
    X, e2, emax = K.stand_in(fr, win.astype(f32).astype(f64))
    r2, rm = K.complex_ratios(G.cpu().numpy(), X, e2, emax)
    note("k_stft_frames, 2-norm", r2.max())
    note("k_stft_frames, bins", rm.max())
    assert r2.max() <= 1.0 and rm.max() <= 1.0, (float(r2.max()), float(rm.max()))


# ---- mel ---------------------------------------------------------------------------------------------------------------

class Bank:
    """Device band-CSR of a dense filterbank (as data.MelBank keeps it), or of given CSR arrays."""

    def __init__(self, dense=None, csr=None):
        lo, ln, off, w = K.band_csr(dense) if csr is None else csr
        self.dense, self.n_mels = dense, len(lo)
        self.lo, self.len, self.off, self.w = dev(lo, np.int32), dev(ln, np.int32), dev(off, np.int32), dev(w)

    def mel(self, power, n_bins, n_mels=None):
        rows = power.numel() // max(n_bins, 1)
        out, buf = guarded(rows, self.n_mels)
        ok(L().ofp_mel(power.data_ptr(), rows, n_bins, self.n_mels if n_mels is None else n_mels, self.lo.data_ptr(),
                       self.len.data_ptr(), self.off.data_ptr(), self.w.data_ptr(), out.data_ptr(), stream()), "ofp_mel")
        torch.cuda.synchronize()
        return out, buf


@pytest.mark.parametrize("case", K.MEL_CASES, ids=lambda c: c[5])
def test_mel_fused_and_separate(case):
    from onset_fingerprinting_amd import data
    sr, n_fft, n_mels, fmin, fmax, what = case
    if n_mels is None:
        n_mels = K.largest_band_count(data.mel_filterbank, sr, n_fft)
    mb = data.MelBank(sr, n_fft, n_mels, fmin, fmax)
    assert K.mel_admitted(mb.w.numel(), n_mels, n_fft // 2 + 1)
    assert (mb.len == 0).any().item() == (what == "empty bands")
    hop, H, bins = n_fft // 4, 9, n_fft // 2 + 1
    xs = noise_series(n_fft + n_mels, 2, n_fft + (H - 1) * hop + 1)
    xs[1, :] += (0.5 * np.sin(2 * np.pi * 0.0731 * np.arange(xs.shape[1]))).astype(f32)
    x = dev(interleave(xs, 1, 2))
    P, pbuf = guarded(1, 2, H, bins)
    mel, mbuf = guarded(1, 2, H, n_mels)
    data.stft_power_mel_dense(x, n_fft, hop, mb, out_power=P, out_mel=mel)
    mel2, m2buf = guarded(1, 2, H, n_mels)
    data.stft_power_mel_dense(x, n_fft, hop, mb, out_mel=mel2, want_power=False)
    mel3, m3buf = guarded(1, 2, H, n_mels)
    mb(P, out=mel3)
    torch.cuda.synchronize()
    assert guard_ok(pbuf) and guard_ok(mbuf) and guard_ok(m2buf) and guard_ok(m3buf)
    Ph = P.cpu().numpy().reshape(2, H, bins)
    check_transform("mel cases", xs, n_fft, hop, Ph, [m.cpu().numpy().reshape(2, H, n_mels) for m in (mel, mel2)],
                    mb.dense, what)
    ref, bound = K.mel_ref(Ph, mb.dense)  # from the fp32 power as given: only the chain's own rounding
    within("ofp_mel", mel3.reshape(2, H, n_mels), ref, bound, what)
    if what == "empty bands":
        assert (mel3.cpu().numpy()[..., (mb.len == 0).cpu().numpy()] == 0).all()


def test_mel_seven_bins_one_row_and_past_the_cap():
    rng = np.random.default_rng(41)
    fb = np.zeros((3, 7), f32)
    fb[0, 1:4], fb[1, 2:7], fb[2, 6:7] = rng.random(3), rng.random(5), 0.5
    p = (rng.standard_normal((1, 7)) ** 2).astype(f32)
    out, buf = Bank(fb).mel(dev(p), 7)
    within("ofp_mel", out, *K.mel_ref(p, fb), "7 bins, 1 row", buf)
    n_mels, bins = 40, 33
    fb = np.zeros((n_mels, bins), f32)
    for b in range(n_mels):
        lo = rng.integers(0, bins - 1)
        fb[b, lo:min(bins, lo + 1 + b)] = rng.random(min(bins, lo + 1 + b) - lo) + 0.1
    rows = K.ELEM_CAP // n_mels + 77
    assert rows * n_mels > K.ELEM_CAP
    p = (rng.standard_normal((rows, bins)) ** 2).astype(f32)
    out, buf = Bank(fb).mel(dev(p), bins)
    within("ofp_mel", out, *K.mel_ref(p, fb), "past the cap", buf)


def test_fused_mel_rejections():
    """ofp_stft_power_mel refuses, on the host and for the reason named, what its segment table cannot hold."""
    from onset_fingerprinting_amd import data
    from onset_fingerprinting_amd.pipeline import seeded_fcnn
    for bins, n_mels, ln, why in K.MEL_REJECTED:
        n_fft = 2 * (bins - 1)
        csr = (np.zeros(n_mels, np.int32), np.full(n_mels, ln, np.int32), np.arange(n_mels, dtype=np.int32) * ln,
               np.ones(n_mels * ln, f32))
        bank = Bank(csr=csr)
        x = torch.zeros((1, n_fft, 1), device="cuda")
        mel, mbuf = guarded(1, 1, 1, n_mels)
        message = rf"filterbank with {n_mels * ln} weights for {bins} bins" if "fb_nnz" in why else \
            r"at most 127 bands and 256 32-tap segments"
        with pytest.raises(err_type(), match=message):
            data.stft_power_mel_dense(x, n_fft, n_fft // 4, bank, out_mel=mel, want_power=False)
        torch.cuda.synchronize()
        assert bool(torch.isnan(mbuf).all()), why
    mb = data.MelBank(K.MEL_SR, 1024, 20)
    with pytest.raises(err_type(), match=r"the classifier takes 40 inputs, the filterbank has 20 bands"):
        data.stft_power_mel_mlp_dense(torch.zeros((1, 2048, 1), device="cuda"), 1024, 256, mb, seeded_fcnn(40, 8).device_mlp(0))


def test_mel_size_rejections():
    bank = Bank(csr=(np.zeros(128, np.int32), np.ones(128, np.int32), np.arange(128, dtype=np.int32), np.ones(128, f32)))
    p = torch.ones(4, 9, device="cuda")
    for n_bins, n_mels, message in ((9, 128, r"ofp_mel: at most 127 bands \(got 128\)"), (9, 0, r"ofp_mel: 0 bands on 9 bins"),
                                    (0, 5, r"ofp_mel: 5 bands on 0 bins"), (9, -1, r"ofp_mel: -1 bands on 9 bins")):
        with pytest.raises(err_type(), match=message):
            bank.mel(p, n_bins, n_mels)


def test_mfcc_size_rejections():
    out, buf = guarded(8)
    keep = torch.ones(64, device="cuda")
    for n_mels, n_mfcc in ((0, 4), (4, 0), (-1, 4)):
        with pytest.raises(err_type(), match=rf"ofp_mfcc: {n_mfcc} coefficients from {n_mels} bands"):
            ok(L().ofp_mfcc(keep.data_ptr(), 2, n_mels, n_mfcc, 1e-10, 80.0, keep.data_ptr(), out.data_ptr(),
                            keep.data_ptr(), stream()), "ofp_mfcc")
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf).all())


def test_stft_frames_channel_count_rejection():
    x = np.zeros((1, 300, 1), f32)
    z = np.zeros(1, np.int64)
    for C in (0, -2):
        with pytest.raises(err_type(), match=rf"ofp_stft_frames: {C} channels"):
            frames_gpu(x, z, z, z, z, z + 300, 256, 256, np.ones(256, f32), C=C)


# ---- MFCC --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", K.MFCC_CASES, ids=lambda c: "-".join(map(str, c)))
def test_mfcc(case):
    from onset_fingerprinting_amd import data
    rows, n_mels, n_mfcc, top_db, kind = case
    mel = K.mfcc_mel(rows, n_mels, kind)
    dct = data.dct_ortho(n_mfcc, n_mels)
    out, buf = guarded(rows, n_mfcc)
    keep = [dev(mel), dev(dct), torch.zeros(4, device="cuda")]
    ok(L().ofp_mfcc(keep[0].data_ptr(), rows, n_mels, n_mfcc, 1e-10, -1.0 if top_db is None else top_db,
                    keep[1].data_ptr(), out.data_ptr(), keep[2].data_ptr(), stream()), "ofp_mfcc")
    torch.cuda.synchronize()
    ref, bound = K.mfcc_ref(mel, dct, top_db=top_db)
    within("ofp_mfcc", out, ref, bound, case, buf)


# ---- k_extract ---------------------------------------------------------------------------------------------------------

EXTRACT_CASES = [(1, 1, 50), (5, 1, 9), (1, 300, 3), (5, 7, K.ELEM_CAP // 35 + 11)]  # (C, width, n_onsets)
assert max(C * width * n for C, width, n in EXTRACT_CASES) > K.ELEM_CAP == 1048576  # one case passes k_extract's cap


@pytest.mark.parametrize("C,width,n_onsets", EXTRACT_CASES)
def test_extract_frames_exact(C, width, n_onsets):
    rng = np.random.default_rng(C + width)
    N = 4000
    x = rng.standard_normal((N, C)).astype(f32)
    starts = rng.integers(-2 * width - 5, N + width + 5, (n_onsets, C))
    starts[0, 0], starts[-1, -1] = -width, N  # entirely outside on either side: zeros
    out, buf = guarded(n_onsets, C, width)
    keep = [dev(x), dev(starts, np.int64)]
    ok(L().ofp_extract_frames(keep[0].data_ptr(), N, C, keep[1].data_ptr(), n_onsets, width, out.data_ptr(), stream()),
       "ofp_extract_frames")
    torch.cuda.synchronize()
    assert guard_ok(buf) and np.array_equal(out.cpu().numpy().view(np.uint32), K.extract_ref(x, starts, width).view(np.uint32))


# ---- spectral flux, scale, rank, peaks -----------------------------------------------------------------------------------

@pytest.mark.parametrize("n_bins", K.FLUX_BINS)
def test_spectral_flux(n_bins):
    rng = np.random.default_rng(n_bins)
    for n_frames in (1,) + K.FLUX_FRAMES:
        p = (rng.standard_normal((n_frames, n_bins)) ** 2 * 10.0 ** rng.uniform(-4, 2, (n_frames, 1))).astype(f32)
        p[rng.random(p.shape) < 0.05] = 0.0
        if n_frames > 1:
            p[1] = p[0]
        w = rng.random(n_bins).astype(f32)
        out, buf = guarded(max(n_frames - 1, 1))
        keep = [dev(p), dev(w)]
        ok(L().ofp_spectral_flux(keep[0].data_ptr(), n_frames, n_bins, keep[1].data_ptr(), out.data_ptr(), stream()),
           "ofp_spectral_flux")
        torch.cuda.synchronize()
        if n_frames == 1:
            assert bool(torch.isnan(buf).all())  # untouched
            continue
        ref, bound = K.flux_ref(p, w)
        within("ofp_spectral_flux", out, ref, bound, (n_bins, n_frames), buf)
        assert float(out[0]) == 0.0  # two identical frames


@pytest.mark.parametrize("n", K.DIVIDE_N)
def test_scale_inverse_exact(n):
    rng = np.random.default_rng(n)
    x = (rng.standard_normal(n) * 10.0 ** rng.uniform(-20, 20, n)).astype(f32)
    buf = torch.full((n + GUARD,), float("nan"), device="cuda")
    buf[:n] = dev(x)
    scale = dev(np.array([0.3717], f32))
    ok(L().ofp_scale_inverse(buf.data_ptr(), n, scale.data_ptr(), stream()), "ofp_scale_inverse")
    torch.cuda.synchronize()
    assert guard_ok(buf)
    assert np.array_equal(buf[:n].cpu().numpy().view(np.uint32), K.divide_ref(x, f32(0.3717)).view(np.uint32))


def test_select_rank_edges():
    rng = np.random.default_rng(51)
    tiny = np.array([0.0, 1e-45, 3e-42, 1e-39], f32)  # +0 and denormals
    cases = {"n = 1": np.array([2.5], f32), "all equal": np.full(700, 0.125, f32),
             "1025": np.abs(rng.standard_normal(1025)).astype(f32),
             "zero, denormals, inf": np.concatenate([tiny, np.abs(rng.standard_normal(40)).astype(f32),
                                                     np.array([np.inf, np.inf], f32)])}
    for name, v in cases.items():
        n = len(v)
        d = dev(rng.permutation(v))
        out, buf = guarded(1)
        for r in sorted({0, n - 1, n // 2, min(3, n - 1), max(n - 2, 0)}):
            ok(L().ofp_select_rank(d.data_ptr(), n, r, out.data_ptr(), stream()), "ofp_select_rank")
            got = out.cpu().numpy()
            assert guard_ok(buf) and got.view(np.uint32)[0] == np.array([K.select_rank_ref(v, r)], f32).view(np.uint32)[0], (name, r)


def peaks_gpu(x, args, cap):
    n = len(x)
    d = dev(x) if n else torch.zeros(1, device="cuda")
    peaks = torch.full((max(n, 1) + GUARD,), -7, dtype=torch.int64, device="cuda")
    cnt = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    fl = torch.zeros(max(n, 1), dtype=torch.uint8, device="cuda")
    ok(L().ofp_peak_pick(d.data_ptr(), n, *args[:4], args[4], args[5], peaks.data_ptr(), cap, cnt.data_ptr(),
                         fl.data_ptr(), stream()), "ofp_peak_pick")
    return int(cnt.cpu()[0]), peaks.cpu().numpy()


def test_peak_pick_edges():
    rng = np.random.default_rng(52)
    plateau = np.zeros(200, f32)
    plateau[50:60] = 1.0
    plateau[120] = 1.0
    envs = {"n = 0": np.zeros(0, f32), "n = 1": np.array([0.7], f32), "below every window": np.array([0.1, 0.9, 0.3], f32),
            "plateau": plateau, "all zeros": np.zeros(300, f32),
            "ragged": (np.abs(rng.standard_normal(1000)) ** 4).astype(f32)}
    for name, x in envs.items():
        for args in ((30, 5, 30, 6, 0.1, 20), (0, 1, 0, 1, 0.0, 0), (5, 2, 5, 3, 0.05, 0)):
            ref = oracle.peak_pick(x, *args)
            count, peaks = peaks_gpu(x, args, len(x))
            assert count == len(ref) and np.array_equal(peaks[:count], ref) and (peaks[count:] == -7).all(), (name, args)
            if len(ref) > 2:  # cap below the count: the count is reported in full, nothing is written past cap
                cap = len(ref) - 2
                count, peaks = peaks_gpu(x, args, cap)
                assert count == len(ref) and np.array_equal(peaks[:cap], ref[:cap]) and (peaks[cap:] == -7).all(), (name, args)
    assert len(oracle.peak_pick(envs["ragged"], 0, 1, 0, 1, 0.0, 0)) > 100 and len(oracle.peak_pick(plateau, 0, 1, 0, 1, 0.0, 0)) == 11
