"""GPU: per-epoch stretch augmentation in the trainers' epoch graph (k_stretch_windows, csrc/ofp_train_random.h; site 2
of the stream, include/onsetfp.h), against tests/train_stretch_ref.py.

  kernel        ofp_stretch_windows: shifts and stretches equal the numpy rule; the windows are bit-equal to
                ofp_resample_windows called with start = starts[j % O] + shift_j and nx = W + stretch_j, and within
                oracle/post_kernels.py's derived bound of the fp64 reference (the bound that function is held to: no new
                tolerance); outputs go into NaN-filled buffers with a guard tail
  class         data.StretchedWindows is that call; max_stretch = 0 is a ShiftedWindows
  off           a fit from StretchedWindows(max_stretch=0) has the bits of the fit from ShiftedWindows
  the epoch     graph and plain launches give the same bits, so do two runs with one seed; two seeds differ
  trajectory    the scheme of tests/test_gpu_train_random.py, the CPU replay taking the batch of epoch e from
                src.windows(seed, e): |ours - ref32| <= max(4 x running max of (spread of eight float32 replays with one
                batch element moved by one ulp, |ref32 - ref64|), 2^-22 x loss) over the comparable prefix, which must
                reach that file's MIN_PREFIX
  refusals      through the ABI's error return and the Python exception; the next valid call is right
Every figure is printed before it is asserted (run with -s to see them)."""
import ctypes
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from oracle import post_kernels as K

sys.path.insert(0, str(Path(__file__).resolve().parent))
import test_gpu_train_random as T  # noqa: E402  (its models, data and constants; none of its tests run from here)
import train_random_ref as R  # noqa: E402
import train_stretch_ref as S  # noqa: E402

pytestmark = pytest.mark.gpu

f32, f64 = np.float32, np.float64
guarded, guard_intact, stream = T.guarded, T.guard_intact, T.stream


def lib():
    from onset_fingerprinting_amd import _lib
    return _lib.lib()


def last_error():
    from onset_fingerprinting_amd import _lib
    return _lib.last_error()


def dev(a, dt):
    return torch.from_numpy(np.ascontiguousarray(a, dt)).cuda()


def stretch_call(audio_d, N, C, starts_d, O, reps, m, span, W, seed, epoch, outputs=True):
    """-> (rc, windows, shifts, stretches) of ofp_stretch_windows into guarded buffers (guards checked)."""
    n = O * reps
    (win, bw), (sh, bs), (sd, bd) = guarded((n, C, W)), guarded((n,), torch.int32), guarded((n,), torch.int32)
    rc = lib().ofp_stretch_windows(seed, epoch, audio_d.data_ptr(), N, C, starts_d.data_ptr(), O, reps, m, span, W,
                                   sh.data_ptr() if outputs else None, sd.data_ptr() if outputs else None,
                                   win.data_ptr(), stream())
    torch.cuda.synchronize()
    assert guard_intact(bw) and guard_intact(bs) and guard_intact(bd)
    return rc, win, sh, sd


def resampled(audio_d, N, C, start, nx, max_nx, W):
    """ofp_resample_windows of the same rows: float32 [items, C, W]."""
    out, buf = guarded((len(nx), C, W))
    sd_, nd = dev(start, np.int64), dev(nx, np.int32)
    rc = lib().ofp_resample_windows(audio_d.data_ptr(), N, C, sd_.data_ptr(), nd.data_ptr(), len(nx), max_nx, W,
                                    out.data_ptr(), stream())
    torch.cuda.synchronize()
    assert rc == 0, last_error()
    assert guard_intact(buf)
    return out.cpu().numpy()


def layout(rng, O, W, m, span):
    """(N, starts [O]): hit 0's earliest window starts at row 0, the last hit's longest, furthest shifted window ends at
    row N, the others lie between with room to spare."""
    longest = W + span - 1
    gap = longest + 2 * m + 3
    N = gap * O + m
    starts = (m + gap * np.arange(O) + rng.integers(0, 3, O)).astype(np.int64)
    starts[0], starts[-1] = m, N - m - longest
    return N, starts


def check_windows(audio, starts, C, W, span, m, reps, seed, epoch, seen=None):
    N, O = audio.shape[0], len(starts)
    a, s = dev(audio, f32), dev(starts, np.int64)
    rc, win, sh, sd = stretch_call(a, N, C, s, O, reps, m, span, W, seed, epoch)
    ctx = (W, span, C, O, reps, m, epoch)
    assert rc == 0, (ctx, last_error())
    ref_sh, ref_sd, ref, bound = S.stretched_windows(audio, starts, W, seed, epoch, m, span, reps)
    assert np.array_equal(sh.cpu().numpy(), ref_sh), ctx
    assert np.array_equal(sd.cpu().numpy(), ref_sd), ctx
    got = win.cpu().numpy()
    same = resampled(a, N, C, np.tile(starts, reps) + ref_sh, W + ref_sd, W + span - 1, W)
    assert np.array_equal(got.view(np.uint32), same.view(np.uint32)), (ctx, "differs from ofp_resample_windows")
    ratio = K.ratio(np.abs(got.astype(f64) - ref), bound)
    assert bool((ratio <= 1.0).all()), (ctx, f"error / bound = {ratio.max():.3g}")
    # the optional outputs left out: the same windows
    rc, win2, sh2, sd2 = stretch_call(a, N, C, s, O, reps, m, span, W, seed, epoch, outputs=False)
    assert rc == 0, (ctx, last_error())
    assert np.array_equal(win2.cpu().numpy().view(np.uint32), got.view(np.uint32)), (ctx, "without d_shifts")
    assert bool((sh2 == -12345).all()) and bool((sd2 == -12345).all()), (ctx, "optional outputs written")
    if seen is not None:
        seen.update(int(v) for v in ref_sd)
    return float(ratio.max())


# ---- 1. the kernel alone --------------------------------------------------------------------------------------------
# W 8, 9, 31 with span 3: Nx in {W-2, W-1, W+1, W+2}, both parities of both lengths (every Nyquist branch), up and down;
# W 300 with span 9: Nx up to 308, every thread-strided loop wraps past 256
@pytest.mark.parametrize("C", [1, 3, 5])
@pytest.mark.parametrize("W,span", [(8, 3), (9, 3), (31, 3), (300, 9)], ids=lambda v: str(v))
def test_stretched_windows(W, span, C):
    rng = np.random.default_rng([W, C])
    seen, worst = set(), 0.0
    for O, reps in ((5, 1), (3, 3)):  # 5 and 9 items: no multiple of 4, the Philox word index
        for m in (0, 2):
            N, starts = layout(rng, O, W, m, span)
            audio = rng.standard_normal((N, C)).astype(f32)
            for epoch in (0, 5):
                worst = max(worst, check_windows(audio, starts, C, W, span, m, reps, 1000 + 7 * W + C, epoch, seen))
    print(f"W {W} span {span} C {C}: stretches seen {sorted(seen)}, largest error / bound {worst:.3g}")
    if span == 3:
        assert seen == {-2, -1, 1, 2}, seen
    else:
        assert min(seen) < 0 < max(seen) and 0 not in seen and max(abs(v) for v in seen) <= span - 1


def test_the_longest_windows_the_resampler_takes():
    """width + span - 1 = 2048 with one channel needs more LDS than the default dynamic limit: the launch raises it."""
    W, span, C, m = 2046, 3, 1, 1
    rng = np.random.default_rng(2046)
    N, starts = layout(rng, 2, W, m, span)
    audio = rng.standard_normal((N, C)).astype(f32)
    worst = check_windows(audio, starts, C, W, span, m, 1, 5, 2)
    print(f"W {W} span {span}: largest error / bound {worst:.3g}")


# ---- 2. the class ---------------------------------------------------------------------------------------------------
def test_stretched_windows_class():
    from onset_fingerprinting_amd import data
    audio, onsets, _y = R.synthetic_hits(4, 6, 3, 31, 18)
    src = data.StretchedWindows(audio, onsets, 31, pre_samples=2, max_stretch=0.1, max_shift=16, n_extractions=3)
    assert (src.n, src.n_onsets, src.channels, src.stretch_span) == (18, 6, 3, 3)
    starts = onsets.min(1) - 2
    a, s = dev(audio, f32), dev(starts, np.int64)
    rc, win, sh, sd = stretch_call(a, len(audio), 3, s, 6, 3, 16, 3, 31, 9, 5)
    assert rc == 0, last_error()
    ref_sh, ref_sd = S.draws(9, 5, 18, 16, 3)
    assert np.array_equal(src.shifts(9, 5).cpu().numpy(), ref_sh)
    assert np.array_equal(src.stretches(9, 5).cpu().numpy(), ref_sd)
    assert torch.equal(src.windows(9, 5).view(torch.int32), win.view(torch.int32))
    assert not torch.equal(src.stretches(9, 0), src.stretches(9, 1))
    one = data.StretchedWindows(audio[:, 0], onsets[:, 0], 31, max_stretch=0.1, max_shift=1)
    assert tuple(one.windows(1, 0).shape) == (6, 31)
    with pytest.raises(ValueError, match="seed"):
        src.windows()
    with pytest.raises(ValueError, match="seed"):
        data.StretchedWindows(audio, onsets, 31, max_stretch=0.1).windows()  # no shift, but a stretch
    # no stretch: a ShiftedWindows, to the bit
    off = data.StretchedWindows(audio, onsets, 31, pre_samples=2, max_stretch=0, max_shift=16, n_extractions=3)
    plain = data.ShiftedWindows(audio, onsets, 31, pre_samples=2, max_shift=16, n_extractions=3)
    assert off.stretch_span == 0
    assert torch.equal(off.windows(9, 5).view(torch.int32), plain.windows(9, 5).view(torch.int32))
    assert torch.equal(off.shifts(9, 5), plain.shifts(9, 5))
    assert not bool(off.stretches(9, 5).any())


# ---- models and data: those of tests/test_gpu_train_random.py, with room for the longer windows ----------------------
W_, SPAN, MAX_STRETCH, MAX_SHIFT, REPS = 31, 3, 0.1, 3, 2


def hits():
    return R.synthetic_hits(8, T.N, 3, W_, MAX_SHIFT + SPAN)


def source(max_stretch=MAX_STRETCH, reps=REPS):
    from onset_fingerprinting_amd import data
    audio, onsets, y = hits()
    src = data.StretchedWindows(audio, onsets, W_, pre_samples=2, max_stretch=max_stretch, max_shift=MAX_SHIFT,
                                n_extractions=reps)
    return src, torch.from_numpy(y)


def fit_bits(fit_fn, make, x, y, **kw):
    m = make().cuda()
    fit = fit_fn(m, x, y, **kw)
    return fit.train_loss, torch.cat([t.detach().reshape(-1).float() for t in m.state_dict().values()])


# ---- 3. off means off -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["cnn", "lcccnn"])
def test_no_stretch_is_the_shifted_source(kind):
    from onset_fingerprinting_amd import data, model
    fit_fn = model.fit_cnn if kind == "cnn" else model.fit_lcccnn
    make = (lambda: T.cnn_model(0.0, batch_norm=True)) if kind == "cnn" else (lambda: T.lcccnn_model(0.0))
    audio, onsets, y = hits()
    y = torch.from_numpy(y).cuda()
    plain = data.ShiftedWindows(audio, onsets, W_, pre_samples=2, max_shift=MAX_SHIFT, n_extractions=REPS)
    off, _y = source(max_stretch=0)
    base_l, base_p = fit_bits(fit_fn, make, plain, y, max_epochs=10, seed=9)
    l, q = fit_bits(fit_fn, make, off, y, max_epochs=10, seed=9)
    assert bool(torch.isfinite(base_l).all())
    assert torch.equal(l.view(torch.int32), base_l.view(torch.int32)) and torch.equal(q, base_p)


# ---- 4. the epoch reaches the stream --------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["cnn", "lcccnn"])
def test_the_epoch_reaches_the_stretches(kind, monkeypatch):
    from onset_fingerprinting_amd import model
    fit_fn = model.fit_cnn if kind == "cnn" else model.fit_lcccnn
    env = "OFP_CNN_GRAPH" if kind == "cnn" else "OFP_CCCNN_GRAPH"
    p = 0.5
    make = (lambda: T.cnn_model(p, batch_norm=True)) if kind == "cnn" else (lambda: T.lcccnn_model(p, group=True))

    def run(seed, mode=None):
        if mode:
            monkeypatch.setenv(env, mode)
        src, y = source()
        out = fit_bits(fit_fn, make, src, y.cuda(), max_epochs=12, seed=seed)
        monkeypatch.delenv(env, raising=False)
        return out

    (la, pa), (lb, pb), (lc, pc), (ld, _pd) = run(7), run(7), run(7, "nodes"), run(8)
    assert bool(torch.isfinite(la).all())
    assert torch.equal(la.view(torch.int32), lb.view(torch.int32)) and torch.equal(pa, pb)
    assert torch.equal(la.view(torch.int32), lc.view(torch.int32)) and torch.equal(pa, pc)
    assert float(la[0]) != float(ld[0]), "two seeds gave the same first loss"
    src, _y = source()
    assert not torch.equal(src.stretches(7, 0), src.stretches(7, 1))
    # and the stretch is in the batch: the same fit from the shifted source alone starts at another loss
    from onset_fingerprinting_amd import data
    audio, onsets, y = hits()
    plain = data.ShiftedWindows(audio, onsets, W_, pre_samples=2, max_shift=MAX_SHIFT, n_extractions=REPS)
    le, _pe = fit_bits(fit_fn, make, plain, torch.from_numpy(y).cuda(), max_epochs=2, seed=7)
    assert float(le[0]) != float(la[0])


# ---- 5. trajectory --------------------------------------------------------------------------------------------------
def stretched_replays(module, batches, y, seed, p, n_pert=8):
    """The float32 replay, the float64 one and n_pert float32 ones with one element of every epoch's batch moved by one
    ulp; batches: the float32 [n, C, W] batch of every epoch."""
    epochs = len(batches)
    c32, _f = R.replay(module, lambda e: batches[e], y, epochs, seed, p, torch.float32)
    c64, _f = R.replay(module, lambda e: batches[e], y, epochs, seed, p, torch.float64)
    pert = [R.replay(module, lambda e, k=k: R.one_ulp(batches[e], k + 1), y, epochs, seed, p, torch.float32)[0]
            for k in range(n_pert)]
    return c32, c64, np.stack(pert)


@pytest.mark.parametrize("case", list(T.TRAJ))
def test_trajectory_with_stretched_batches(case):
    from onset_fingerprinting_amd import model
    torch.set_num_threads(1)
    kind, p, kw = T.TRAJ[case]
    make = lambda: (T.cnn_model if kind == "cnn" else T.lcccnn_model)(p, **kw)  # noqa: E731
    src, y = source()
    seed, epochs = T.TRAJ_SEED, T.EPOCHS
    # the batches the epoch graph trains on, held to the resampler's bits by test_stretched_windows
    batches = [src.windows(seed, e).cpu().numpy() for e in range(epochs)]
    assert not np.array_equal(batches[0], batches[1])
    ref32, ref64, pert = stretched_replays(make(), batches, np.tile(y.numpy(), (REPS, 1)), seed, p)
    prefix, spread = R.comparable_prefix(ref32, pert)
    print(f"{case}: comparable prefix {prefix} of {epochs}; loss {ref32[0]:.6g} -> {ref32[-1]:.6g}")
    assert prefix >= T.MIN_PREFIX
    m = make().cuda()
    fit = (model.fit_cnn if kind == "cnn" else model.fit_lcccnn)(m, src, y.cuda(), max_epochs=epochs, seed=seed)
    ours = fit.train_loss.cpu().numpy().astype(f64)
    assert fit.epochs == epochs and np.isfinite(ours).all()
    own = np.maximum(spread[:prefix], np.abs(ref32[:prefix] - ref64[:prefix]))
    bound = np.maximum(4 * np.maximum.accumulate(own), T.U22 * ref32[:prefix])
    diff = np.abs(ours[:prefix] - ref32[:prefix].astype(f32).astype(f64))
    worst = int(np.argmax(diff / bound))
    print(f"{case}: prefix {prefix}; worst ratio {diff[worst] / bound[worst]:.3g} at epoch {worst}: |ours - ref32| "
          f"{diff[worst]:.3e} bound {bound[worst]:.3e} (spread {spread[worst]:.3e}, |ref32 - ref64| "
          f"{abs(ref32[worst] - ref64[worst]):.3e}, loss {ref32[worst]:.6g})")
    assert np.all(diff <= bound), (case, worst, diff[worst], bound[worst])


# ---- 6. refusals ----------------------------------------------------------------------------------------------------
def refused(rc, what):
    assert rc != 0, (what, "was accepted")
    assert last_error().strip(), (what, "no message")


def cnnrnn_model():
    from onset_fingerprinting_amd import model
    return model.CNNRNN(W_, 2, channels=3, layer_sizes=[4, 6], n_hidden=8, dropout_rate=0.0)


def rnn_model(**kw):
    from onset_fingerprinting_amd import model
    return model.RNN(W_, 2, channels=3, hidden_size=8, dropout_rate=0.0, **kw)


def test_refusals():
    from onset_fingerprinting_amd import _lib, data, model
    L = lib()
    W, span, C, m, O = 31, 3, 2, 1, 3
    rng = np.random.default_rng(6)
    N, starts = layout(rng, O, W, m, span)
    audio = rng.standard_normal((N, C)).astype(f32)
    a, s = dev(audio, f32), dev(starts, np.int64)

    def still_right(after):
        worst = check_windows(audio, starts, C, W, span, m, 2, 11, 1)
        print(f"after {after}: the next call's largest error / bound {worst:.3g}")

    def untouched(win, sh, sd):
        return bool(torch.isnan(win).all()) and bool((sh == -12345).all()) and bool((sd == -12345).all())

    # the stand-alone entry
    for what, (width, sp, n_rows) in {"a span of 1": (W, 1, N), "a span of 0": (W, 0, N), "a negative span": (W, -3, N),
                                      "a span above the width": (2, 3, N), "width + span - 1 = 2049": (2047, 3, N),
                                      "audio one row too short": (W, span, W + 2 * m + span - 2)}.items():
        rc, win, sh, sd = stretch_call(a, n_rows, C, s, O, 1, m, sp, width, 1, 0)
        refused(rc, what)
        assert untouched(win, sh, sd), (what, "output written")
        still_right(what)

    # the trainers' entries: nothing is touched before the options are checked, so the pointers can stay NULL
    cfg_cnn, _c, _b = model._cnn_arch(T.cnn_model(0.0), W_, None)
    cfg_cc, _c, _g = model._cccnn_arch(T.lcccnn_model(0.0), W_, None)
    cfg_cr, _c, _b = model._cnnrnn_arch(cnnrnn_model(), W_, None)
    cfg_rnn = model._rnn_arch(rnn_model())
    cfg_rnn.width = W_
    src, _y = source()
    rnd, keep = model._train_random(0.0, 3, 0, src)
    none = _lib.TrainRandom()
    none.seed = 3
    epochs = ctypes.c_int32(0)
    for name, cfg, plain in (("cnn", cfg_cnn, "train_random"), ("cccnn", cfg_cc, "train_random"),
                             ("cnnrnn", cfg_cr, "loss_grads_random"), ("rnn", cfg_rnn, "loss_grads_random")):
        ws_fn = getattr(L, f"ofp_{name}_train_stretch_workspace_bytes")
        assert ws_fn(ctypes.byref(cfg), src.n, 0, ctypes.byref(rnd), SPAN) > 0, last_error()
        assert ws_fn(ctypes.byref(cfg), src.n, 0, ctypes.byref(rnd), 0) == \
            getattr(L, f"ofp_{name}_{plain}_workspace_bytes")(ctypes.byref(cfg), src.n, 0, ctypes.byref(rnd))
        for what, (r, sp) in {"a span of 1": (ctypes.byref(rnd), 1), "a negative span": (ctypes.byref(rnd), -2),
                              "a span without options": (None, SPAN),
                              "a span without a window source": (ctypes.byref(none), SPAN),
                              "a span above the width": (ctypes.byref(rnd), W_ + 1)}.items():
            assert ws_fn(ctypes.byref(cfg), src.n, 0, r, sp) == -1, (name, what)
            assert last_error().strip(), (name, what)
            extra = (None,) if name in ("cnn", "cnnrnn") else ()  # d_stats
            rc = getattr(L, f"ofp_{name}_train_stretch")(ctypes.byref(cfg), src.n, None, None, 0, None, None, None, 5,
                                                        0, -1, None, *extra, None, None, ctypes.byref(epochs), None,
                                                        0, stream(), r, sp)
            refused(rc, (name, what))
        still_right(f"the refusals of ofp_{name}_train_stretch")
    del keep

    # Python
    with pytest.raises(ValueError, match=r"randint\(1, 1\)"):
        data.StretchedWindows(audio, starts, W, max_stretch=0.04, max_shift=m)
    long_audio = np.zeros((3000, 1), f32)
    too_long = data.StretchedWindows(long_audio, [10], 2047, max_stretch=0.0015)
    assert too_long.stretch_span == 3
    with pytest.raises(_lib.OnsetFPError, match="2048"):
        too_long.windows(1, 0)
    still_right("width + span - 1 = 2049 through the class")
    xs, y = source()
    with pytest.raises(ValueError, match="permute_input=True"):
        model.fit_rnn(rnn_model(permute_input=False).cuda(), xs, y.cuda(), max_epochs=2, seed=1)
    for fit_fn, m_ in ((model.fit_cnn, T.cnn_model(0.0)), (model.fit_lcccnn, T.lcccnn_model(0.0)),
                       (model.fit_cnnrnn, cnnrnn_model()), (model.fit_rnn, rnn_model())):
        with pytest.raises(ValueError, match="x_val"):
            fit_fn(m_.cuda(), xs, y.cuda(), x_val=xs, y_val=y.cuda(), max_epochs=2, seed=1)
        with pytest.raises(ValueError, match="needs seed="):
            fit_fn(m_.cuda(), xs, y.cuda(), max_epochs=2)
    still_right("the refusals of the fit functions")
