"""GPU: the two calibration kernels of csrc/ofp_train.hip (k_tdoa_fit, k_fcnn_train) against the float64 references of
tests/calib_train_ref.py, at the sizes where their loops, reductions and memory arenas change shape.

Position fit      loss and all gradients (calibration.tdoa_loss_and_grads_device / ofp_tdoa_loss_grads: the fit
                  kernel leaving after its first epoch's sums) element-wise inside the derived bounds, for one wave
                  and its neighbours, one pass of the 256 threads and its neighbours, two passes and the limit of
                  4096 sounds with its 128 KiB of LDS; per-problem and shared lags; an exactly zero residual; short
                  fits and early stops against the restated loop (tdoa_fit_ref) in float64.
FCNN trainer      gradients at the batch sizes and widths where group_size and the row loops change shape, and on
                  both sides of the LDS / work-space switch, by the rule of tests/test_gpu_calibration.py; BatchNorm
                  running statistics inside derived bounds after one epoch and by the short-fit rule after three.
Short-fit rule    |ours - ref64| <= max(4 x max(spread, |ref32 - ref64|), floor): spread from 8 float32 runs of the
                  restated loop on inputs disturbed by one ulp; floor = the loss's derived bound, or 2^-23 x
                  max |ref64| for a parameter tensor.
Every figure is printed before it is asserted (run with -s to see them)."""
import copy
import sys
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

sys.path.insert(0, str(Path(__file__).resolve().parent))
import calib_train_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513, 4095, 4096]
LOSSFUN = {"l1": F.l1_loss, "mse": F.mse_loss}
U23, U24 = 2.0 ** -23, 2.0 ** -24
GUARD = 64
KEYS = ("loss", "sensors", "sounds", "C")
WORST = {}


def note(label, ratio):
    WORST[label] = max(WORST.get(label, 0.0), float(ratio))


@pytest.fixture(scope="module", autouse=True)
def worst_ratios():
    yield
    print("\nlargest error / bound measured, per output:")
    for k in sorted(WORST):
        print(f"  {k}: {WORST[k]:.3f}")


@pytest.fixture(scope="module")
def tdoa_cases():
    """{(n, loss): (inputs, reference)}; the inputs of a size are shared by both losses."""
    out = {}
    for n in SIZES:
        inputs = R.make_tdoa_inputs(n, 100 + n)
        assert R.residual_margin(*inputs) >= 1e-6
        for loss in LOSSFUN:
            out[n, loss] = (inputs, R.tdoa_loss_and_grads_ref(*inputs, loss))
    return out


def raw_loss_grads(obs, sensors, sounds, c, loss):
    """ofp_tdoa_loss_grads on NaN-filled buffers with a guard tail: obs [N, 2] (shared) or [M, N, 2], sensors
    [M, 4, 3], sounds [M, N, 2], c [M] -> list of {"loss", "sensors", "sounds", "C"} per problem."""
    from onset_fingerprinting_amd import _lib
    from onset_fingerprinting_amd.calibration import _stream
    _lib.require_gpu(0)
    L = _lib.lib()
    dev = torch.device("cuda", 0)
    M, N = sounds.shape[0], sounds.shape[1]
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)
    d_obs, d_sens, d_snd, d_c = up(obs), up(sensors), up(sounds), up(np.asarray(c, np.float32).reshape(M))
    sizes = {"loss": M, "sensors": M * 12, "sounds": M * N * 2, "C": M}
    bufs = {k: torch.full((n + GUARD,), float("nan"), dtype=torch.float32, device=dev) for k, n in sizes.items()}
    _lib.check(L.ofp_tdoa_loss_grads(M, N, d_obs.data_ptr(), N * 2 if obs.ndim == 3 else 0, d_sens.data_ptr(),
                                     d_snd.data_ptr(), d_c.data_ptr(), R.LOSSES[loss], bufs["loss"].data_ptr(),
                                     bufs["sensors"].data_ptr(), bufs["sounds"].data_ptr(), bufs["C"].data_ptr(),
                                     _stream(dev)), "ofp_tdoa_loss_grads")
    torch.cuda.synchronize()
    host = {k: b.cpu().numpy() for k, b in bufs.items()}
    for k, n in sizes.items():
        assert np.isnan(host[k][n:]).all(), f"{k}: written beyond its {n} values"
        assert np.isfinite(host[k][:n]).all(), f"{k}: not every value written"
    return [{"loss": host["loss"][m], "sensors": host["sensors"][m * 12:(m + 1) * 12].reshape(4, 3),
             "sounds": host["sounds"][m * N * 2:(m + 1) * N * 2].reshape(N, 2), "C": host["C"][m]} for m in range(M)]


def one_problem(inputs, loss):
    obs, sensors, sounds, c = inputs
    return raw_loss_grads(obs, sensors[None], sounds[None], [c], loss)[0]


def check_against(got, ref, label, group):
    ratios = R.worst_ratio(got, ref)
    for k in KEYS:
        val, bound = ref[k]
        err = np.max(np.abs(np.asarray(got[k], np.float64) - val))
        print(f"{label} {k}: max |ours - ref64| {err:.3e}  largest |ref64| {np.max(np.abs(val)):.3e}  "
              f"largest bound {np.max(bound):.3e}  error / bound {ratios[k]:.3f}")
        note(f"{group} {k}", ratios[k])
    assert max(ratios.values()) <= 1, (label, ratios)


# ---- position fit: gradients ------------------------------------------------------------------------------------

@pytest.mark.parametrize("loss", ["l1", "mse"])
@pytest.mark.parametrize("n", SIZES)
def test_position_gradients(tdoa_cases, n, loss):
    inputs, ref = tdoa_cases[n, loss]
    got = one_problem(inputs, loss)
    check_against(got, ref, f"N {n} {loss}", f"position gradients {loss}")
    # the Python entry returns the same bits (sr = 1: the lags are the observed times)
    from onset_fingerprinting_amd import calibration
    obs, sensors, sounds, c = inputs
    v, grads = calibration.tdoa_loss_and_grads_device(obs, sensors, sounds, C=float(c), lossfun=LOSSFUN[loss], sr=1)
    assert v.shape == (1,) and grads["sensors"].shape == (1, 4, 3) and grads["sounds"].shape == (1, n, 2)
    assert grads["C"].shape == (1,)
    assert np.array_equal(v.cpu().numpy()[0], got["loss"]) and np.array_equal(grads["C"].cpu().numpy()[0], got["C"])
    assert np.array_equal(grads["sensors"][0].cpu().numpy(), got["sensors"])
    assert np.array_equal(grads["sounds"][0].cpu().numpy(), got["sounds"])


@pytest.mark.parametrize("loss", ["l1", "mse"])
def test_small_launch_after_the_largest(tdoa_cases, loss):
    """128 KiB of dynamic LDS raise the kernel's attribute; a 2 KiB launch follows in the same process."""
    for n in (4096, 63):
        inputs, ref = tdoa_cases[n, loss]
        check_against(one_problem(inputs, loss), ref, f"N {n} {loss} in sequence", f"position gradients {loss}")


@pytest.mark.parametrize("loss", ["l1", "mse"])
def test_position_gradients_of_a_batch(loss):
    """M = 3 problems with different starts at N = 257 (two passes): with lags of their own [3, N, 2], then with
    shared lags [N, 2]; every problem equals its single call bit for bit and is inside its own reference's bounds."""
    n = 257
    own = [R.make_tdoa_inputs(n, 500 + m) for m in range(3)]
    # shared lags: the starts of problem 0 moved by some 20 micrometres (below 3e-7 s), which keeps every sign
    rng = np.random.default_rng(77)
    obs0, sensors0, sounds0, c0 = own[0]
    shared = [(obs0, (sensors0 + rng.normal(0, 2e-5, (4, 3))).astype(np.float32),
               (sounds0 + rng.normal(0, 2e-5, (n, 2))).astype(np.float32), np.float32(c0 + 0.01 * m))
              for m in range(3)]
    for kind, probs in (("own", own), ("shared", shared)):
        obs, sensors, sounds, c = (np.stack([p[k] for p in probs]) for k in range(4))
        assert all(R.residual_margin(*p) >= 1e-6 for p in probs)
        assert not np.array_equal(sensors[0], sensors[1]) and not np.array_equal(sounds[1], sounds[2])
        batch = raw_loss_grads(obs[0] if kind == "shared" else obs, sensors, sounds, c, loss)
        for m in range(3):
            single = one_problem(probs[m], loss)
            for k in KEYS:
                assert np.array_equal(np.asarray(batch[m][k]).view(np.uint32), np.asarray(single[k]).view(np.uint32)), \
                    (kind, m, k)
            check_against(batch[m], R.tdoa_loss_and_grads_ref(*probs[m], loss), f"batch, {kind} lags, problem {m} "
                          f"{loss}", f"position gradients {loss}")


def test_exactly_zero_residuals():
    inputs = R.make_tdoa_inputs(257, 7, zero_case=True)
    ref = R.tdoa_loss_and_grads_ref(*inputs, "l1")
    got = one_problem(inputs, "l1")
    print(f"sound 0: gradients {got['sounds'][0]}")
    assert got["sounds"][0].tolist() == [0.0, 0.0]
    check_against(got, ref, "zero case l1", "position gradients l1")
    # it adds nothing to the sums: its float64 terms are 0, so the bounds above leave no room for a contribution
    # (sign(0) = +1 misses the sensors' bound by a factor above 100, tests/test_calib_train_ref_cpu.py)
    assert np.all(ref["terms"]["sensors"][0] == 0) and ref["terms"]["loss"][0] == 0 and ref["terms"]["C"][0] == 0


def test_refusals_come_before_any_launch(tdoa_cases):
    from onset_fingerprinting_amd import _lib, calibration
    inputs, ref = tdoa_cases[65, "mse"]
    obs, sensors, sounds, c = inputs
    call = calibration.tdoa_loss_and_grads_device
    with pytest.raises(ValueError, match="limit"):
        call(np.zeros((0, 2), np.float32), sensors, np.zeros((0, 2), np.float32))
    with pytest.raises(ValueError, match="limit"):
        call(np.zeros((4097, 2), np.float32), sensors, np.zeros((4097, 2), np.float32))
    with pytest.raises(ValueError, match="4 sensors"):
        call(obs, sensors[:3], sounds)
    with pytest.raises(ValueError, match="observed_lags"):
        call(obs[:, :1], sensors, sounds)
    with pytest.raises(ValueError, match="initial_sound_positions"):
        call(obs, sensors, sounds[:64])
    with pytest.raises(ValueError, match="disagree"):
        call(np.stack([obs] * 2), np.stack([sensors] * 3), sounds)
    with pytest.raises(ValueError, match="HIP implementation"):
        call(obs, sensors, sounds, lossfun=F.smooth_l1_loss)
    # the C entry refuses the same sizes itself, and NULL buffers
    L = _lib.lib()
    one = torch.zeros(16, dtype=torch.float32, device="cuda")
    p = one.data_ptr()
    for M, n, out in ((1, 0, p), (1, 4097, p), (0, 4, p), (1, 4, None)):
        assert L.ofp_tdoa_loss_grads(M, n, p, 0, p, p, p, 1, p, p, out, p, None) != 0
    assert L.ofp_tdoa_loss_grads(1, 4, p, 0, p, p, p, 2, p, p, p, p, None) != 0
    assert b"ofp_tdoa_loss_grads" in L.ofp_last_error()
    torch.cuda.synchronize()
    check_against(one_problem(inputs, "mse"), ref, "after the refusals", "position gradients mse")


# ---- position fit: short fits and early stops -------------------------------------------------------------------

def fit_on_gpu(inputs, loss, num_epochs, eps=1e-12, patience=10):
    from onset_fingerprinting_amd import calibration
    obs, sensors, sounds, c = inputs
    fit = calibration.optimize_positions_device(obs, sensors, sounds, lr=0.01, lossfun=LOSSFUN[loss],
                                                num_epochs=num_epochs, C=float(c), sr=1, eps=eps, patience=patience)
    return {"curve": fit.losses[0].cpu().numpy().astype(np.float64), "updates": int(fit.epochs[0]),
            "sensors": fit.sensors[0].cpu().numpy().astype(np.float64),
            "sounds": fit.sounds[0].cpu().numpy().astype(np.float64), "C": float(fit.C[0])}


def check_fit(ours, ref64, bounds, label, group, keys=("curve", "sensors", "sounds", "C")):
    n_loss = len(ref64["curve"])
    assert ours["updates"] == ref64["updates"], (label, ours["updates"], ref64["updates"])
    assert np.isfinite(ours["curve"][:n_loss]).all() and np.isnan(ours["curve"][n_loss:]).all(), label
    worst = 0.0
    for k in keys:
        mine = ours[k][:n_loss] if k == "curve" else ours[k]
        err = np.abs(np.asarray(mine, np.float64) - np.asarray(ref64[k], np.float64))
        ratio = float(np.max(err / bounds[k]))
        print(f"{label} {k}: max |ours - ref64| {np.max(err):.3e}  largest bound {np.max(bounds[k]):.3e}  "
              f"error / bound {ratio:.3f}")
        note(f"{group} {k}", ratio)
        worst = max(worst, ratio)
    assert worst <= 1, (label, worst)


@pytest.mark.parametrize("loss", ["l1", "mse"])
@pytest.mark.parametrize("n", [1, 257, 4096])
@pytest.mark.parametrize("E", [2, 3, 8])
def test_short_fits(tdoa_cases, E, n, loss):
    """E = 2 is the first run in which a sound's update is visible: the kernel returns the sounds its last forward
    pass used, i.e. after E - 1 updates."""
    inputs, _ref = tdoa_cases[n, loss]
    ref64, bounds = R.tdoa_short_fit_case(inputs, loss, E)
    assert ref64["updates"] == E and len(ref64["curve"]) == E
    assert np.any(ref64["sounds"][:, :2] != inputs[2].astype(np.float64))
    check_fit(fit_on_gpu(inputs, loss, E), ref64, bounds, f"E {E} N {n} {loss}", f"short fits {loss}")


@pytest.mark.parametrize("patience", [0, 3])
@pytest.mark.parametrize("n", [257, 4096])
def test_early_stop(tdoa_cases, n, patience):
    """eps = 1e9: the first loss beats +inf and none after it counts, so `patience` more epochs update and the next
    one stops; its loss is stored behind the curve, and the sounds are those that loss was evaluated at."""
    E = 10
    for loss in ("l1", "mse"):
        inputs, _ref = tdoa_cases[n, loss]
        ref64, bounds = R.tdoa_short_fit_case(inputs, loss, E, eps=1e9, patience=patience)
        assert ref64["updates"] == patience + 1 and len(ref64["curve"]) == patience + 2
        assert np.array_equal(ref64["sounds"][:, :2], ref64["history"][-1][1])
        ours = fit_on_gpu(inputs, loss, E, eps=1e9, patience=patience)
        print(f"N {n} patience {patience} {loss}: updates {ours['updates']}, curve {ours['curve']}")
        check_fit(ours, ref64, bounds, f"stop N {n} patience {patience} {loss}", f"early stop {loss}")


# ---- FCNN trainer: gradients at the size edges ------------------------------------------------------------------

def torch_grads(model, x, y, lossfun, device, dtype, perm=None):
    net = copy.deepcopy(model.network).to(device, dtype).train()
    if perm is not None:
        x, y = x[perm], y[perm]
    v = lossfun(net(x.to(device, dtype)), y.to(device, dtype))
    v.backward()
    return {"network." + k: p.grad.cpu().numpy().astype(np.float64) for k, p in net.named_parameters()}, float(v.detach())


def check_fcnn_grads(model, x, y, loss, label):
    """The rule of test_gpu_calibration.check_grads against float64 autograd: per tensor max |ours - g64| <=
    max(4 x max |g32 - g64|, 2^-23 x max |g64|), the float32 error being the largest over torch's GPU float32, its
    CPU float32 and four row permutations of the batch on the CPU (a permutation changes only the order of
    summation, which guards the rule against a float32 run that lands on float64 by luck at tiny N).  The loss by
    the same rule, and never tighter than the N x 2^-24 relative of check_grads."""
    from onset_fingerprinting_amd import calibration
    lossfun = LOSSFUN[loss]
    n = len(x)
    v, grads = calibration.fcnn_loss_and_grads_device(model, x.cuda(), y.cuda(), lossfun)
    g64, l64 = torch_grads(model, x, y, lossfun, "cpu", torch.float64)
    gen = torch.Generator().manual_seed(n)
    refs = [torch_grads(model, x, y, lossfun, "cuda", torch.float32),
            torch_grads(model, x, y, lossfun, "cpu", torch.float32)]
    refs += [torch_grads(model, x, y, lossfun, "cpu", torch.float32, torch.randperm(n, generator=gen))
             for _k in range(4)]
    assert sorted(grads) == sorted(g64)
    worst = 0.0
    for k, want in g64.items():
        ours = grads[k].detach().cpu().numpy().astype(np.float64)
        assert np.isfinite(ours).all(), (label, k)
        err = np.max(np.abs(ours - want))
        err32 = max(np.max(np.abs(g32[k] - want)) for g32, _l in refs)
        bound = max(4 * err32, U23 * np.max(np.abs(want)))
        ratio = 0.0 if err == 0 else err / bound if bound > 0 else np.inf
        print(f"{label} {k}: |ours - g64| {err:.3e}  |g32 - g64| {err32:.3e}  bound {bound:.3e}  ratio {ratio:.3f}")
        worst = max(worst, ratio)
    l_err = abs(float(v) - l64)
    l_bound = max(4 * max(abs(l32 - l64) for _g, l32 in refs), U23 * abs(l64), n * U24 * abs(l64))
    print(f"{label} loss: ours {float(v):.9g} ref64 {l64:.9g} |ours - ref64| {l_err:.3e} bound {l_bound:.3e}")
    note(f"fcnn gradients {loss}", worst)
    note(f"fcnn loss {loss}", l_err / l_bound)
    assert worst <= 1 and l_err <= l_bound, (label, worst, l_err, l_bound)


def fcnn(n_in, n_out, hidden, seed, **kw):
    from onset_fingerprinting_amd import calibration
    torch.manual_seed(seed)
    model = calibration.FCNN(n_in, n_out, hidden_layers=list(hidden), **kw)
    if kw.get("batch_norm", True):
        with torch.no_grad():
            for m in model.network:
                if isinstance(m, nn.BatchNorm1d):
                    m.weight.copy_(0.5 + torch.rand(m.num_features))
                    m.bias.copy_(0.3 * torch.randn(m.num_features))
                    m.running_mean.copy_(torch.randn(m.num_features))
                    m.running_var.copy_(0.5 + torch.rand(m.num_features))
    return model


def batch(n, n_in, n_out, seed):
    gen = torch.Generator().manual_seed(seed)
    return torch.randn(n, n_in, generator=gen), torch.randn(n, n_out, generator=gen)


@pytest.mark.parametrize("hidden", [(5,), (7, 5)], ids=["3-5-2", "3-7-5-2"])
@pytest.mark.parametrize("n", [1, 2, 3, 63, 64, 65, 255, 256, 257, 1023, 1024])
def test_fcnn_gradients_at_batch_edges(n, hidden):
    from onset_fingerprinting_amd import calibration
    x, y = batch(n, 3, 2, 40 + n)
    for bn in (False, True):
        model = fcnn(3, 2, hidden, 7, activation=nn.SiLU, batch_norm=bn)
        for loss in ("l1", "mse"):
            if bn and n == 1:
                with pytest.raises(ValueError, match="more than 1"):
                    calibration.fcnn_loss_and_grads_device(model, x.cuda(), y.cuda(), LOSSFUN[loss])
                continue
            check_fcnn_grads(model, x, y, loss, f"N {n} {'-'.join(map(str, hidden))} {'bn ' if bn else ''}{loss}")


WIDTH_CASES = {
    "hidden-1": dict(n_in=3, n_out=2, hidden=(1,)),
    "hidden-127": dict(n_in=3, n_out=2, hidden=(127,)),
    "hidden-128": dict(n_in=3, n_out=2, hidden=(128,)),
    "in-1": dict(n_in=1, n_out=2, hidden=(6,)),
    "out-1": dict(n_in=3, n_out=1, hidden=(6,)),
    "8-linear": dict(n_in=3, n_out=2, hidden=(9, 8, 7, 6, 5, 4, 3)),
    "bn-no-bias": dict(n_in=3, n_out=2, hidden=(7, 5), bias=False, batch_norm=True),
}


@pytest.mark.parametrize("case", list(WIDTH_CASES))
def test_fcnn_gradients_at_width_edges(case):
    cfg = dict(WIDTH_CASES[case])
    n_in, n_out, hidden = cfg.pop("n_in"), cfg.pop("n_out"), cfg.pop("hidden")
    x, y = batch(65, n_in, n_out, 77)
    for bn in ([True] if "batch_norm" in cfg else [False, True]):
        kw = dict(cfg, batch_norm=bn, activation=nn.Tanh)
        model = fcnn(n_in, n_out, hidden, 9, **kw)
        assert len([m for m in model.network if isinstance(m, nn.Linear)]) == len(hidden) + 1
        for loss in ("l1", "mse"):
            check_fcnn_grads(model, x, y, loss, f"{case} {'bn ' if bn else ''}{loss}")


@pytest.mark.parametrize("bn", [False, True], ids=["plain", "bn"])
def test_fcnn_gradients_on_both_sides_of_the_arena_switch(bn):
    """The same network one row below the switch from LDS to the global work space and one row above it."""
    from onset_fingerprinting_amd import calibration
    budget = 160 * 1024 - 512
    model = fcnn(3, 2, (64, 64), 11, activation=nn.SiLU, batch_norm=bn)
    size = lambda n: calibration.fcnn_train_lds_bytes(model, n)
    below = max(n for n in range(2, 1025) if size(n) <= budget)
    print(f"hidden [64, 64]{' bn' if bn else ''}: {below} rows take {size(below)} B, {below + 1} rows "
          f"{size(below + 1)} B; the switch is at {budget} B")
    assert 2 <= below < 1024 and size(below) <= budget < size(below + 1)
    for n in (below, below + 1):
        x, y = batch(n, 3, 2, 300 + n)
        for loss in ("l1", "mse"):
            check_fcnn_grads(model, x, y, loss, f"arena N {n} {'bn ' if bn else ''}{loss}")


# ---- FCNN trainer: BatchNorm running statistics -----------------------------------------------------------------

def unpack_stats(stats, model):
    out, o = [], 0
    flat = stats.cpu().numpy().astype(np.float64)
    for m in model.network:
        if isinstance(m, nn.BatchNorm1d):
            w = m.num_features
            out.append((flat[o:o + w], flat[o + w:o + 2 * w]))
            o += 2 * w
    assert o == len(flat)
    return out


STATS_CASES = [(act, 65) for act in (nn.Identity, nn.ReLU, nn.SiLU, nn.LeakyReLU, nn.ELU, nn.Tanh)]
STATS_CASES += [(nn.SiLU, 2), (nn.SiLU, 1024)]


@pytest.mark.parametrize("act,n", STATS_CASES, ids=[f"{a.__name__}-{n}" for a, n in STATS_CASES])
def test_running_statistics(act, n):
    from onset_fingerprinting_amd import calibration
    model = fcnn(3, 2, (7, 5), 13, activation=act, batch_norm=True)
    x, y = batch(n, 3, 2, 60 + n)
    # one epoch: inside the derived bounds, element-wise
    run = calibration.train_location_models_device(x.cuda(), y.cuda(), 0.01, F.l1_loss, num_epochs=1, models=[model])
    assert int(run.epochs[0]) == 1
    ref = R.fcnn_running_stats_ref(model.network, x.numpy())
    for layer, ((rm, rv), ((m, bm), (v, bv))) in enumerate(zip(unpack_stats(run.stats[0], model), ref)):
        r_m, r_v = np.max(np.abs(rm - m) / bm), np.max(np.abs(rv - v) / bv)
        print(f"{act.__name__} N {n} layer {layer}: mean max |ours - ref64| {np.max(np.abs(rm - m)):.3e} error / "
              f"bound {r_m:.3f};  var {np.max(np.abs(rv - v)):.3e} error / bound {r_v:.3f}")
        note("running mean, 1 epoch", r_m)
        note("running var, 1 epoch", r_v)
        assert r_m <= 1 and r_v <= 1
    tracked = [int(m.num_batches_tracked) for m in run.model(0).network if isinstance(m, nn.BatchNorm1d)]
    assert tracked == [1, 1]
    # three epochs: the short-fit rule, spread and float32 error from torch's own modules
    E, lr = 3, 0.01
    run = calibration.train_location_models_device(x.cuda(), y.cuda(), lr, F.l1_loss, num_epochs=E, models=[model])
    assert int(run.epochs[0]) == E
    xs, ys = x.numpy(), y.numpy()
    ref64 = R.fcnn_running_stats_ref(model.network, xs, ys, lr, "l1", E)
    ref32 = R.running_stats_of(R.train_fcnn_torch(model.network, xs, ys, lr, "l1", E, torch.float32))
    pert = [R.running_stats_of(R.train_fcnn_torch(model.network, xs * np.float32(1 + k * U23), ys, lr, "l1", E,
                                                  torch.float32)) for k in range(1, 9)]
    for layer, mine in enumerate(unpack_stats(run.stats[0], model)):
        for which, name in ((0, "mean"), (1, "var")):
            a64, a32 = ref64[layer][which], ref32[layer][which]
            spread = np.max([np.abs(p[layer][which] - a32) for p in pert], axis=0)
            bound = np.maximum(4 * np.maximum(spread, np.abs(a32 - a64)), U23 * np.max(np.abs(a64)))
            err = np.abs(mine[which] - a64)
            ratio = float(np.max(err / bound))
            print(f"{act.__name__} N {n} layer {layer} running {name} after {E} epochs: max |ours - ref64| "
                  f"{np.max(err):.3e}  largest bound {np.max(bound):.3e}  error / bound {ratio:.3f}")
            note(f"running {name}, {E} epochs", ratio)
            assert ratio <= 1
