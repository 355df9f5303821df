"""fp64 references of the spectral kernels, their error bars, an fp32 emulation of the FFT plan and the shape
tables shared by tests/test_spectral_kernels_cpu.py and tests/test_gpu_spectral_kernels.py
-- TEST INFRASTRUCTURE ONLY.

Covers csrc/ofp_spectral.hip (k_stft_power, k_stft_frames, k_extract, k_mel, k_mfcc), csrc/ofp_fft.h and
csrc/ofp_onset_spectral.hip (k_spectral_flux, k_divide, k_select_rank, k_peak_*).  Every reference is plain
numpy in float64 written from the formula; none calls the library or torch.  U = 2^-24.

The transform (k_stft_power, k_stft_frames)
    Reference: X = np.fft.rfft(float64(frame) * float64(window)) after a float64 gather with the kernel's
    zero rules.  The error bar is MEASURED PER FRAME against an independent fp32 transform, not a worst-case
    bound (the rigorous ||wx||_2 sqrt(F) (2U + sqrt(2) log2(M) eta) is 70-100 times what an fp32 FFT really
    does and no sharper than the 1e-4 of tests/test_gpu_spectral.py):
        S32 = scipy.fft.rfft(float32(window) * frame)      (complex64: pocketfft in single precision)
        e2 = ||S32 - X||_2,  emax = max_k |S32_k - X_k|
    complex output G:  ||G - X||_2 <= A e2   and   |G_k - X_k| <= B emax for every bin;
    power output P:    with e = B emax,  |P_k - |X_k|^2| <= 2 |X_k| e + e^2 + 4 U |X_k|^2 for every bin (no floor,
                       no bin skipped: |X + d|^2 - |X|^2 = 2 Re(conj X d) + |d|^2, two roundings of the squares
                       and one of their sum on the last term)  and  ||sqrt(P) - |X|||_2 <= A e2;
    a frame whose stand-in is exact (e2 == 0, e.g. all zeros) must be exact.

A and B
    Set on the CPU from `emu_rfft` / `emu_power` below -- an fp32 numpy emulation of the plan ofp_fft.h
    describes (packed M = F/2 point sequence, Stockham passes with the radices of Radices<M>, twiddles built in
    fp64 and rounded once, the fma complex product, the split pass of rfft_bin / rfft_power_pair), written
    from that description.  A = 2 max ||emu - X||_2 / e2 and B = 2 max max_k|emu - X| / emax over the five sizes
    and the input families of `family_frames`; the factor 2 covers the difference between the emulation's and
    the hardware's rounding of the same plan.  `measure_ab()` recomputes the ratios (256 frames of each random
    family and size: the largest ratio of a set grows with the number of frames, and the GPU tests run tens of
    thousands); tests/test_spectral_kernels_cpu.py holds A and B to them.  Measured: the emulation reaches
    R2_EMU = 1.77 (||.||_2; the tone family at 1024 points) and RMAX_EMU = 4.46 (largest bin; the tone family at
    2048 points; broadband noise stays under 2.2), so A = 3.54 and B = 8.92.  A cruder stand-in (pocketfft
    complex64 on the packed sequence plus an fp32 split) gave 1.7 and 4.4.

mel (k_mel, the epilogue of k_stft_power)
    Reference P64 @ fb64 from the power the kernel was given (ofp_mel: float64 of the fp32 power, bar of the
    input 0) or made (fused: |X|^2 with the power bar of every bin).  bound_b = sum_k w_k bar_k +
    (min(len_b, 32) + ceil(len_b / 32) + 1) U sum_k w_k P_k: a 32-tap fma chain from 0 is off by at most
    32 U sum|p w|, adding ceil(len/32) segment sums rounds as often again, one more for slack.  An empty band
    has bound 0: it must be exactly 0.

MFCC (k_max, k_mfcc) from a given fp32 mel
    Reference: float64 power_to_db (10 log10 max(amin, m), floored at the GLOBAL maximum minus top_db) and
    the DCT matrix product.  bound = sum_b |d_b| 8 U |db_b| + (n_mels + 1) U sum_b |db_b d_b|.
    ASSUMPTION (the same as oracle/nn_kernels.py makes for expf / tanhf): the HIP math documentation is not
    available next to this file; 4 ulp = 8 U |db| covers log10f (documented at 2 ulp) and the multiplication
    by 10.  Clamping against the floor is 1-Lipschitz, so it adds nothing (the floor's own error, 8 U |max_db|
    and one subtraction, is covered where |max_db - top_db| >= |max_db|, as in every case of MFCC_CASES: their
    maxima lie under +20 dB, their floors under -60 dB).

spectral flux (k_spectral_flux)
    Reference float64 mean_k max(0, w_k (sqrt p1_k - sqrt p0_k)).  With a_k = w_k sqrt p0_k, b_k = w_k sqrt p1_k:
    the square root, the product and the difference round once each (3 U (a_k + b_k) in all, an upper bound
    for the difference's own U |b_k - a_k|); a lane adds ceil(n_bins / 64) terms, the butterfly 6 levels and
    the division one more.  bound = (sum_k 3 U (a_k + b_k) + (ceil(n_bins/64) + 7) U sum_k max(0, b_k - a_k)) / n_bins.

k_extract, k_divide, k_select_rank, ofp_peak_pick are exact: numpy gather, float32 division, np.sort and
oracle.peak_pick.
"""
import math

import numpy as np
import scipy.fft

U = 2.0 ** -24
f32, f64 = np.float32, np.float64

NFFT = (256, 512, 1024, 2048, 4096)
FPW = {256: 16, 512: 8, 1024: 8, 2048: 4, 4096: 1}   # Cfg<F>::FPW: frames per workgroup iteration
RADICES = {128: (8, 4, 4), 256: (8, 8, 4), 512: (8, 8, 8), 1024: (8, 8, 4, 4), 2048: (8, 8, 8, 4)}  # Radices<M>
GRID_CAP = 2048          # launch_power_s, launch_frames: workgroups
ELEM_CAP = 256 * 16 * 256  # k_extract, k_mel, k_mfcc: elements one pass of the capped grid covers (1 048 576)
MEL_SEG, MEL_MAXSEG = 32, 256

# 2 x the largest ratio the emulation reaches (measure_ab(), tests/test_spectral_kernels_cpu.py)
R2_EMU, RMAX_EMU = 1.77, 4.46
A, B = 2 * R2_EMU, 2 * RMAX_EMU


# ---- windows, gathers, references ------------------------------------------------------------------------------------

def hann_periodic64(n):
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n) / n)


def gather_frames(x, starts, frame_length, n_fft, valid_lo, valid_hi, clip=None, channel=None):
    """k_stft_frames' gather: x [n_clips, N, C] (or a 1-D series), one frame per start.  Position p of a frame
    holds sample start + p - lpad, lpad = (n_fft - frame_length) // 2, when 0 <= p - lpad < frame_length and the
    sample index lies in [valid_lo, valid_hi) and in [0, N); zero otherwise.  float32 [n, n_fft] (exact)."""
    x = np.asarray(x)
    if x.ndim == 1:
        x = x[None, :, None]
    n_clips, N, C = x.shape
    starts = np.asarray(starts, np.int64)
    n = len(starts)
    clip = np.zeros(n, np.int64) if clip is None else np.asarray(clip, np.int64)
    channel = np.zeros(n, np.int64) if channel is None else np.asarray(channel, np.int64)
    lo = np.broadcast_to(np.asarray(valid_lo, np.int64), (n,))
    hi = np.broadcast_to(np.asarray(valid_hi, np.int64), (n,))
    lpad = (n_fft - frame_length) // 2
    q = np.arange(n_fft)[None, :] - lpad
    idx = starts[:, None] + q
    ok = (q >= 0) & (q < frame_length) & (idx >= lo[:, None]) & (idx < hi[:, None]) & (idx >= 0) & (idx < N)
    v = x[clip[:, None], np.clip(idx, 0, N - 1), channel[:, None]]
    return np.where(ok, v, 0).astype(f32)


def frames_ref(x, starts, frame_length, n_fft, window, valid_lo, valid_hi, clip=None, channel=None):
    """Reference of k_stft_frames: complex128 [n, n_fft/2+1]."""
    fr = gather_frames(x, starts, frame_length, n_fft, valid_lo, valid_hi, clip, channel)
    return np.fft.rfft(fr.astype(f64) * np.asarray(window, f64), axis=-1)


def dense_frames(series, n_fft, hop):
    """The frames k_stft_power takes from one series [N]: [H, n_fft] (a view), H = 1 + (N - n_fft) // hop."""
    N = len(series)
    if N < n_fft:
        return np.zeros((0, n_fft), series.dtype)
    H = 1 + (N - n_fft) // hop
    return np.lib.stride_tricks.sliding_window_view(series, n_fft)[::hop][:H]


def dense_power_ref(x, n_fft, hop):
    """Reference of k_stft_power: x [n_clips, N, C] -> float64 [n_clips, C, H, n_fft/2+1]."""
    x = np.asarray(x)
    n_clips, N, C = x.shape
    w = hann_periodic64(n_fft)
    H = 1 + (N - n_fft) // hop if N >= n_fft else 0
    out = np.zeros((n_clips, C, H, n_fft // 2 + 1))
    for i in range(n_clips):
        for c in range(C):
            X = np.fft.rfft(dense_frames(x[i, :, c], n_fft, hop).astype(f64) * w, axis=-1)
            out[i, c] = X.real ** 2 + X.imag ** 2
    return out


def stand_in(frames, window):
    """(X, e2, emax) of float32 frames [n, F] under the float64 window [F]: the fp64 reference and the per-frame
    error of pocketfft's single-precision transform of float32(window) * frame."""
    frames = np.ascontiguousarray(frames, f32)
    window = np.asarray(window, f64)
    X = np.fft.rfft(frames.astype(f64) * window, axis=-1)
    S32 = scipy.fft.rfft(window.astype(f32) * frames, axis=-1)
    assert S32.dtype == np.complex64, S32.dtype  # pocketfft computed in single precision
    d = np.abs(S32.astype(np.complex128) - X)
    return X, np.sqrt((d ** 2).sum(-1)), d.max(-1)


def _ratio(err, bar):
    """err / bar; 0 where both are 0, inf where the bar is 0 and the error is not (or the error is NaN)."""
    err, bar = np.asarray(err, f64), np.broadcast_to(np.asarray(bar, f64), np.shape(err))
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bar > 0, err / bar, np.where(err == 0, 0.0, np.inf))
    return np.where(np.isnan(err), np.inf, r)


def complex_ratios(G, X, e2, emax, a=None, b=None):
    """Per frame: (||G - X||_2 / (A e2), max_k |G_k - X_k| / (B emax)); each must be <= 1."""
    a, b = A if a is None else a, B if b is None else b
    d = np.abs(np.asarray(G).astype(np.complex128) - X)
    return _ratio(np.sqrt((d ** 2).sum(-1)), a * e2), _ratio(d.max(-1), b * emax)


def power_bar(X, emax, b=None):
    """Element-wise bar of a power spectrum whose complex bins are each within e = B emax of X."""
    e = ((B if b is None else b) * np.asarray(emax, f64))[..., None]
    m = np.abs(X)
    return 2 * m * e + e * e + 4 * U * m * m


def power_ratios(P, X, e2, emax, a=None, b=None):
    """Per frame: (max_k |P_k - |X_k|^2| / bar_k, ||sqrt P - |X|||_2 / (A e2)); each must be <= 1."""
    a = A if a is None else a
    P = np.asarray(P, f64)
    m = np.abs(X)
    r_el = _ratio(np.abs(P - m * m), power_bar(X, emax, b)).max(-1)
    with np.errstate(invalid="ignore"):
        dm = np.sqrt(P) - m  # (a negative power is NaN: fails)
    return r_el, _ratio(np.sqrt((dm ** 2).sum(-1)), a * e2)


# ---- fp32 emulation of the plan of ofp_fft.h -----------------------------------------------------------------------

def fma(a, b, c):
    """fp32 fma: the product of two floats is exact in double, the sum rounds to double and then to float."""
    return (np.asarray(a, f64) * np.asarray(b, f64) + np.asarray(c, f64)).astype(f32)


def twiddles(n, count, fault=None):
    """W_n^k = exp(-2 pi i k / n), k < count, built in fp64 (exact at the multiples of a quarter turn, as sincospi
    is) and rounded once.  fault 'recurrence': W^k = W^(k-1) W^1 by repeated fp32 products instead."""
    k = np.arange(count)
    ang = 2.0 * np.pi * k / n
    c, s = np.cos(ang), -np.sin(ang)
    q = (4 * k) % n == 0
    quarter = ((4 * k) // n) % 4
    c = np.where(q, np.array([1.0, 0.0, -1.0, 0.0])[quarter], c)
    s = np.where(q, np.array([0.0, -1.0, 0.0, 1.0])[quarter], s)
    c, s = c.astype(f32), s.astype(f32)
    if fault == "recurrence":
        for i in range(2, count):
            c[i], s[i] = _cmul((c[i - 1], s[i - 1]), (c[1], s[1]))
    return c, s


def _cmul(a, b):
    (ar, ai), (br, bi) = a, b
    return fma(ar, br, -(ai * bi)), fma(ar, bi, ai * br)


def _add(a, b):
    return a[0] + b[0], a[1] + b[1]


def _sub(a, b):
    return a[0] - b[0], a[1] - b[1]


def _mul_mi(a):
    return a[1], -a[0]


def _dft2(v, i, j):
    v[i], v[j] = _add(v[i], v[j]), _sub(v[i], v[j])


def _dft4(v):
    _dft2(v, 0, 2)
    _dft2(v, 1, 3)
    v[3] = _mul_mi(v[3])
    _dft2(v, 0, 1)
    _dft2(v, 2, 3)
    v[1], v[2] = v[2], v[1]


def _dft8(v):
    h = f32(0.70710678118654752440)
    for i in range(4):
        _dft2(v, i, i + 4)
    v[5] = ((v[5][0] + v[5][1]) * h, (v[5][1] - v[5][0]) * h)
    v[6] = _mul_mi(v[6])
    v[7] = ((v[7][1] - v[7][0]) * h, -(v[7][0] + v[7][1]) * h)
    _dft2(v, 0, 2)
    _dft2(v, 1, 3)
    v[3] = _mul_mi(v[3])
    _dft2(v, 4, 6)
    _dft2(v, 5, 7)
    v[7] = _mul_mi(v[7])
    for i in (0, 2, 4, 6):
        _dft2(v, i, i + 1)
    v[1], v[4] = v[4], v[1]
    v[3], v[6] = v[6], v[3]


def emu_cfft(zr, zi, fault=None):
    """Stockham autosort FFT of [n, M] float32 points with the radices of Radices<M>."""
    M = zr.shape[-1]
    twr, twi = twiddles(M, M, fault)
    Ns = 1
    for R in RADICES[M]:
        L = M // R
        j = np.arange(L)
        k = j % Ns
        tstep = k * (M // (Ns * R))
        v = [(zr[:, j + i * L], zi[:, j + i * L]) for i in range(R)]
        if Ns > 1:
            for i in range(1, R):
                t = (i * tstep) % M
                v[i] = _cmul(v[i], (twr[t], twi[t]))
        _dft8(v) if R == 8 else _dft4(v)
        zr, zi = np.empty_like(zr), np.empty_like(zi)
        for i in range(R):
            zr[:, (j - k) * R + k + i * Ns], zi[:, (j - k) * R + k + i * Ns] = v[i]
        Ns *= R
    return zr, zi


def _split(wx, fault):
    """e, t = W_F^k o of the split pass for k in [0, M] (rfft_bin) from windowed float32 frames [n, F]."""
    wx = np.ascontiguousarray(wx, f32)
    M = wx.shape[-1] // 2
    zr, zi = emu_cfft(np.ascontiguousarray(wx[:, 0::2]), np.ascontiguousarray(wx[:, 1::2]), fault)
    k = np.arange(M + 1)
    ik, im = k % M, (M - k) % M
    if fault == "swap":  # bins p and M - p of the packed transform swapped for one p
        p = M // 4 + 3
        ik, im = ik.copy(), im.copy()
        ik[p], im[p] = im[p], ik[p]
    zk = (zr[:, ik], zi[:, ik])
    zm = (zr[:, im], -zi[:, im])
    half = f32(0.5)
    e = (half * (zk[0] + zm[0]), half * (zk[1] + zm[1]))
    o = (half * (zk[0] - zm[0]), half * (zk[1] - zm[1]))
    fr, fi = twiddles(2 * M, M + 1)
    return e, _cmul((fr, fi), o)


def emu_rfft(wx, fault=None):
    """k_stft_frames' arithmetic on windowed float32 frames [n, F]: complex64 [n, F/2+1] (rfft_bin)."""
    e, t = _split(wx, fault)
    G = np.empty(e[0].shape, np.complex64)
    G.real, G.imag = e[0] + t[1], e[1] - t[0]
    if fault == "nyquist":
        G[:, -1] = 0
    return G


def emu_power(wx, fault=None):
    """k_stft_power's arithmetic: float32 [n, F/2+1] (rfft_power_pair: bins p and M - p from one pair)."""
    e, t = _split(wx, fault)
    M = e[0].shape[-1] - 1
    p = np.arange(M // 2 + 1)
    er, ei, tr, ti = e[0][:, p], e[1][:, p], t[0][:, p], t[1][:, p]
    ar, ai = er + ti, ei - tr
    br, bi = er - ti, ei + tr
    P = np.zeros((e[0].shape[0], M + 1), f32)
    P[:, M - p[:M // 2]] = fma(br, br, bi * bi)[:, :M // 2]
    P[:, p] = fma(ar, ar, ai * ai)
    if fault == "nyquist":
        P[:, -1] = 0
    return P


# ---- input families ------------------------------------------------------------------------------------------------

FAMILIES = ("noise", "tone", "hit", "constant", "zero", "nyquist", "onehot_1", "onehot_half", "onehot_last")


def family_frames(F, seed=0, reps=256):
    """name -> float32 [n, F]: the input families the transform is measured and tested on (seeded)."""
    rng = np.random.default_rng(1000 * seed + F)
    t = np.arange(F)
    out = {}
    out["noise"] = rng.standard_normal((reps, F))
    out["tone"] = np.stack([1e-3 * rng.standard_normal(F) +
                            0.5 * np.sin(2 * np.pi * ((rng.integers(4, F // 2 - 4) + rng.uniform(0.2, 0.8)) / F) * t + r)
                            for r in range(reps)])  # between two bin centres
    out["hit"] = np.stack([(t >= F // 3) * np.exp(-(t - F // 3) / (F / 12.0)) * rng.standard_normal(F)
                           for r in range(reps)])
    out["constant"] = 0.7 + 1e-4 * rng.standard_normal((reps, F))
    out["zero"] = np.zeros((1, F))
    out["nyquist"] = np.where(t % 2 == 0, 1.0, -1.0)[None]
    for name, pos in (("onehot_1", 1), ("onehot_half", F // 2), ("onehot_last", F - 1)):
        out[name] = np.zeros((1, F))
        out[name][0, pos] = 1.0
    return {k: v.astype(f32) for k, v in out.items()}


def measure_ab(seeds=(0,)):
    """{(F, family): (largest ||emu - X||_2 / e2, largest max|emu - X| / emax)} of the emulation's complex output;
    A and B are twice the largest of each."""
    res = {}
    for F in NFFT:
        w = hann_periodic64(F)
        for seed in seeds:
            for name, fr in family_frames(F, seed).items():
                X, e2, emax = stand_in(fr, w)
                r2, rm = complex_ratios(emu_rfft(fr * w.astype(f32)), X, e2, emax, 1.0, 1.0)
                old = res.get((F, name), (0.0, 0.0))
                res[(F, name)] = (max(old[0], float(r2.max())), max(old[1], float(rm.max())))
    return res


# ---- mel -----------------------------------------------------------------------------------------------------------

def band_csr(fb):
    """Band-CSR of a dense filterbank [n_mels, bins] as data.MelBank builds it: (lo, len, off, w)."""
    lo, ln, off, w = [], [], [], []
    for row in np.asarray(fb):
        nz = np.nonzero(row)[0]
        off.append(len(w))
        if len(nz) == 0:
            lo.append(0), ln.append(0)
            continue
        lo.append(int(nz[0])), ln.append(int(nz[-1] - nz[0] + 1))
        w.extend(row[nz[0]:nz[-1] + 1].tolist())
    return (np.array(lo, np.int32), np.array(ln, np.int32), np.array(off, np.int32),
            np.array(w if w else [0.0], f32))


def mel_ref(P, fb, pbar=None):
    """(ref, bound) of the band sums: P [..., bins] (float64 of what the kernel was given, or |X|^2), fb float32
    [n_mels, bins], pbar the element-wise bar of P (None: P is the kernel's exact input)."""
    P, fb = np.asarray(P, f64), np.asarray(fb, f64)
    ln = band_csr(fb)[1].astype(f64)
    ref = P @ fb.T
    steps = np.minimum(ln, MEL_SEG) + np.ceil(ln / MEL_SEG) + 1
    bound = steps * U * (np.abs(P) @ fb.T)
    if pbar is not None:
        bound = bound + np.asarray(pbar, f64) @ fb.T
    return ref, bound


def emu_mel(P, fb, fault=None):
    """k_mel / mel_bands in float32: 32-tap fma chains from 0, added in order.  faults: 'tap' drops the first tap
    of the second segment (tap 32, a segment-boundary tap), 'lo' reads band b with the neighbouring band's lo."""
    P = np.asarray(P, f32)
    lo, ln, off, w = band_csr(fb)
    out = np.zeros(P.shape[:-1] + (len(lo),), f32)
    for b in range(len(lo)):
        blo = lo[(b + 1) % len(lo)] if fault == "lo" else lo[b]
        acc = None
        for q in range(0, int(ln[b]), MEL_SEG):
            part = np.zeros(P.shape[:-1], f32)
            for k in range(q, min(int(ln[b]), q + MEL_SEG)):
                if fault == "tap" and k == MEL_SEG:
                    continue
                part = fma(P[..., min(blo + k, P.shape[-1] - 1)], w[off[b] + k], part)
            acc = part if acc is None else acc + part
        if acc is not None:
            out[..., b] = acc
    return out


# ---- MFCC ----------------------------------------------------------------------------------------------------------

def dct_ortho64(n_mfcc, n_mels):
    n = np.arange(n_mels)
    k = np.arange(n_mfcc)[:, None]
    D = np.cos(np.pi * k * (2 * n + 1) / (2.0 * n_mels)) * np.sqrt(2.0 / n_mels)
    D[0] *= np.sqrt(0.5)
    return D


def mfcc_ref(mel, dct, amin=1e-10, top_db=80.0):
    """(ref, bound): mel float32 [rows, n_mels] as given, dct float32 [n_mfcc, n_mels] as given."""
    mel, dct = np.asarray(mel, f64), np.asarray(dct, f64)
    db = 10.0 * np.log10(np.maximum(f64(f32(amin)), mel))
    if top_db is not None:
        db = np.maximum(db, db.max() - top_db)  # the floor comes from the maximum over ALL rows
    n_mels = mel.shape[-1]
    ref = db @ dct.T
    mag = np.abs(db) @ np.abs(dct).T
    return ref, 8 * U * mag + (n_mels + 1) * U * mag


def emu_mfcc(mel, dct, amin=1e-10, top_db=80.0, fault=None):
    """k_mfcc in float32.  faults: 'row_max' takes the floor from each row's own maximum, 'amin' does not apply
    amin (log10 of 0 is -inf)."""
    mel, dct = np.asarray(mel, f32), np.asarray(dct, f32)
    am = f32(0.0) if fault == "amin" else f32(amin)
    with np.errstate(divide="ignore"):
        db = f32(10.0) * np.log10(np.maximum(am, mel)).astype(f32)
        if top_db is not None:
            g = mel.max(-1, keepdims=True) if fault == "row_max" else mel.max()
            db = np.maximum(db, f32(10.0) * np.log10(np.maximum(am, g)).astype(f32) - f32(top_db))
    acc = np.zeros(mel.shape[:-1] + (dct.shape[0],), f32)
    with np.errstate(invalid="ignore"):
        for b in range(mel.shape[-1]):
            acc = fma(db[..., b:b + 1], dct[None, :, b], acc)
    return acc


# ---- spectral flux ---------------------------------------------------------------------------------------------------

def flux_ref(power, w):
    """(ref, bound): power float32 [n_frames, n_bins] as given, w float32 [n_bins] -> [n_frames - 1]."""
    mag = np.sqrt(np.asarray(power, f64)) * np.asarray(w, f64)
    a, b = mag[:-1], mag[1:]
    n_bins = mag.shape[1]
    pos = np.maximum(0.0, b - a)
    ref = pos.sum(-1) / n_bins
    bound = (3 * U * (a + b).sum(-1) + (math.ceil(n_bins / 64) + 7) * U * pos.sum(-1)) / n_bins
    return ref, bound


def emu_flux(power, w, fault=None):
    """k_spectral_flux in float32: lanes over bins (stride 64), a 6-level butterfly, one division.
    faults: 'abs' takes |b - a| in place of max(0, b - a), 'n_minus_1' divides by n_bins - 1."""
    power, w = np.asarray(power, f32), np.asarray(w, f32)
    n_frames, n_bins = power.shape
    mag = np.sqrt(power) * w
    d = mag[1:] - mag[:-1]
    d = np.abs(d) if fault == "abs" else np.maximum(f32(0), d)
    pad = np.zeros((n_frames - 1, -n_bins % 64), f32)
    lanes = np.concatenate([d, pad], 1).reshape(n_frames - 1, -1, 64)
    acc = np.zeros((n_frames - 1, 64), f32)
    for r in range(lanes.shape[1]):
        acc = acc + lanes[:, r]
    o = 32
    while o:
        acc = acc + acc[:, np.arange(64) ^ o]
        o >>= 1
    return acc[:, 0] / f32(n_bins - 1 if fault == "n_minus_1" else n_bins)


# ---- exact kernels ---------------------------------------------------------------------------------------------------

def extract_ref(x, starts, width):
    """k_extract: x [N, C], starts [O, C] -> [O, C, width], samples outside [0, N) read as zero."""
    x, starts = np.asarray(x), np.asarray(starts, np.int64)
    N, C = x.shape
    t = starts[:, :, None] + np.arange(width)[None, None, :]
    ok = (t >= 0) & (t < N)
    return np.where(ok, x[np.clip(t, 0, N - 1), np.arange(C)[None, :, None]], 0).astype(x.dtype)


def divide_ref(x, scale):
    return (np.asarray(x, f32) / f32(scale)).astype(f32)


def select_rank_ref(v, rank):
    return np.sort(np.asarray(v, f32))[rank]


# ---- shape tables ----------------------------------------------------------------------------------------------------

def dispatch(n_fft, planar_stride, hop, C, base_mod8=0):
    """launch_power_t restated: 'slide' (planar, consecutive frames per wave), 'il' (the same on the interleaved
    input) or 'plain'.  base_mod8: the input address modulo 8."""
    if n_fft <= 2048 and planar_stride and hop * 4 == n_fft and planar_stride % 2 == 0 and base_mod8 % 8 == 0:
        return "slide"
    if n_fft <= 1024 and not planar_stride and hop * 4 == n_fft and C in (4, 8) and FPW[n_fft] % C == 0 and \
            base_mod8 % 4 == 0:
        return "il"
    return "plain"


def straddles(n_fft, planar_stride, hop, n_series, H, base_mod8=0):
    """Fractions (aligned, straddling) of the frames of a planar input under the plain mapping: a frame takes the
    4-byte loads of lines 146-150 when its first sample is not 8-byte aligned."""
    cc, h = np.meshgrid(np.arange(n_series), np.arange(H), indexing="ij")
    odd = ((base_mod8 // 4) + cc * planar_stride + h * hop) % 2 == 1
    return float((~odd).mean()), float(odd.mean())


def _stride_case(name, n_fft, layout, hop, path, n_clips=2, C=3, odd_stride=False, base_off=0):
    need = GRID_CAP * FPW[n_fft] + FPW[n_fft] + 1
    H = -(-need // (n_clips * C))
    for _ in range(FPW[n_fft]):  # the last group stays partly filled (where the channel count allows it)
        if (n_clips * C * H) % FPW[n_fft] == 0:
            H += 1
    N = n_fft + (H - 1) * hop + min(hop - 1, 3)
    stride = 0
    if layout == "planar":
        stride = N + (N + int(odd_stride)) % 2 + 2 * 5  # even (or odd) and further apart than the series are long
    return dict(name=name, n_fft=n_fft, layout=layout, hop=hop, path=path, n_clips=n_clips, C=C, N=N, H=H,
                stride=stride, base_off=base_off, total=n_clips * C * H)


INTERLEAVED_HOP = {256: 4, 512: 8, 1024: 8, 2048: 16, 4096: 64}
STRIDE_CASES = (
    [_stride_case(f"interleaved-{F}", F, "interleaved", INTERLEAVED_HOP[F], "plain") for F in NFFT] +
    [_stride_case(f"planar-oddhop-{F}", F, "planar", INTERLEAVED_HOP[F] + 1, "plain") for F in NFFT] +
    [_stride_case(f"planar-oddstride-{F}", F, "planar", F // 4, "plain", odd_stride=True) for F in NFFT] +
    [_stride_case(f"planar-off4-{F}", F, "planar", F // 4, "plain", base_off=1) for F in NFFT] +
    [_stride_case(f"planar-slide-{F}", F, "planar", F // 4, "slide") for F in NFFT[:4]] +
    [_stride_case(f"il-slide-{F}-C{C}", F, "interleaved", F // 4, "il", n_clips=3, C=C) for F in NFFT[:3] for C in (4, 8)]
)

# (sr, n_fft, n_mels, fmin, fmax, what the case is there for)
MEL_SR = 48000
MEL_CASES = (
    (MEL_SR, 1024, 1, 0.0, None, "one band"),
    (MEL_SR, 1024, 40, 0.0, None, "the default"),
    (MEL_SR, 1024, 127, 0.0, None, "127 bands"),
    (MEL_SR, 256, 127, 0.0, None, "empty bands"),
    (MEL_SR, 4096, None, 0.0, None, "the most bands the segment table admits"),
    (MEL_SR, 512, 40, 300.0, 8000.0, "fmin / fmax"),
)


def mel_admitted(nnz, n_mels, n_bins):
    """The host's conditions on a fused filterbank (ofp_stft_power_mel)."""
    return 1 <= n_mels <= 127 and nnz // MEL_SEG + n_mels <= MEL_MAXSEG and nnz <= 4 * n_bins


def largest_band_count(filterbank, sr, n_fft):
    """The largest n_mels <= 127 whose filterbank the segment table admits."""
    for n_mels in range(127, 0, -1):
        nnz = len(band_csr(filterbank(sr, n_fft, n_mels))[3])
        if mel_admitted(nnz, n_mels, n_fft // 2 + 1):
            return n_mels
    raise AssertionError("no band count admitted")


# artificial band-CSR shapes the host must refuse: (n_bins, n_mels, len of every band, reason)
MEL_REJECTED = (
    (2049, 128, 8, "128 bands"),
    (2049, 127, 40, "over the segment table"),   # 5080 / 32 + 127 = 285 > 256
    (129, 10, 60, "fb_nnz too large for the bins"),  # 600 > 4 * 129
)

# (rows, n_mels, n_mfcc, top_db, kind of mel)
MFCC_CASES = (
    (7, 40, 14, 80.0, "plain"),
    (7, 40, 14, None, "plain"),
    (5, 40, 14, 80.0, "zeros"),
    (5, 40, 14, None, "zeros"),
    (5, 40, 14, 80.0, "below_floor"),
    (3, 40, 14, 80.0, "all_zero"),
    (9, 1, 1, 80.0, "plain"),
    (9, 127, 127, 80.0, "plain"),
    (9, 127, 1, None, "plain"),
    (6, 40, 40, 80.0, "below_floor"),
    (ELEM_CAP // 14 + 3, 16, 14, 80.0, "plain"),   # rows * n_mfcc past the cap
)


def mfcc_mel(rows, n_mels, kind, seed=0):
    """A float32 mel [rows, n_mels] of the given kind: values over twelve decades; 'zeros' adds exact zeros,
    'below_floor' values more than top_db under the maximum, 'all_zero' is all zeros."""
    rng = np.random.default_rng(seed)
    mel = (10.0 ** rng.uniform(-3, 2, (rows, n_mels))).astype(f32)
    if kind == "zeros":
        mel[rng.random((rows, n_mels)) < 0.2] = 0.0
    elif kind == "below_floor":
        mel[rng.random((rows, n_mels)) < 0.3] *= f32(1e-11)
    elif kind == "all_zero":
        mel[:] = 0.0
    return mel


FLUX_BINS = (1, 63, 64, 65, 129, 2049)
FLUX_FRAMES = (2, 6, 4098)
DIVIDE_N = (0, 1, 255, 257, 70001)
