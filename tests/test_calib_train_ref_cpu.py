"""No GPU: the float64 references of tests/calib_train_ref.py against torch autograd, the restated position fit against
the recorded reference runs, and the proof that the derived bounds separate a correct float32 kernel from a wrong
one: both float32 emulations of the kernel's expressions (ascending sums, and the kernel's strided tree) stay inside
every bound at every size the GPU tests use, and every planted fault falls outside the bound of the output it
corrupts."""
import json
import sys
from pathlib import Path

import numpy as np
import pytest
import torch
from torch import nn

sys.path.insert(0, str(Path(__file__).resolve().parent))
import calib_train_ref as R  # noqa: E402

SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513, 4095, 4096]
FAULT_SIZES = [257, 4096]
LOSSES = ["l1", "mse"]
U24 = 2.0 ** -24


@pytest.fixture(scope="module")
def cases():
    """{(n, loss): (inputs, reference)}, computed once."""
    out = {}
    for n in SIZES:
        inputs = R.make_tdoa_inputs(n, 100 + n)
        for loss in LOSSES:
            out[n, loss] = (inputs, R.tdoa_loss_and_grads_ref(*inputs, loss))
    return out


@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("n", [1, 65, 513])
def test_reference_agrees_with_autograd(cases, n, loss):
    (obs, sensors, sounds, c), ref = cases[n, loss]
    s = torch.tensor(sensors, dtype=torch.float64, requires_grad=True)
    p = torch.tensor(sounds, dtype=torch.float64, requires_grad=True)
    cc = torch.tensor(float(c), dtype=torch.float64, requires_grad=True)
    xyz = torch.cat((p, torch.zeros(n, 1, dtype=torch.float64)), 1)
    d = (xyz[:, None, :] - s[None, :, :]).pow(2).sum(-1).sqrt()
    t = (d[:, :2] - d[:, 2:]) / cc
    o = torch.tensor(obs, dtype=torch.float64)
    v = nn.functional.l1_loss(t, o) if loss == "l1" else nn.functional.mse_loss(t, o)
    v.backward()
    for key, got in (("loss", v.detach()), ("sensors", s.grad), ("sounds", p.grad), ("C", cc.grad)):
        want = np.asarray(ref[key][0])
        err = np.max(np.abs(got.numpy() - want))
        scale = np.max(np.abs(want))
        print(f"N {n} {loss} {key}: |ref - autograd| {err:.3e} of {scale:.3e}")
        assert err <= 1e-12 * scale
    # the terms handed out for the fault tests are the terms of the sums
    assert np.allclose(ref["terms"]["sensors"].sum(0), ref["sensors"][0], rtol=1e-12, atol=0)
    assert np.isclose(ref["terms"]["C"].sum(), ref["C"][0], rtol=1e-12, atol=0)


def test_input_conditions(cases):
    for (n, loss), (inputs, _ref) in cases.items():
        margin = R.residual_margin(*inputs)
        obs, sensors, sounds, c = inputs
        _t, d = R.tdoa_times64(sensors, sounds, c)
        t_rounding = np.max(d[:, :2] + d[:, 2:]) / float(c)
        assert margin >= 1e-6 and t_rounding <= 2.2e-3, (n, margin, t_rounding)
        assert np.all(np.hypot(sounds[:, 0], sounds[:, 1]) < R.RADIUS + 0.02)
    # the exact-zero case: both residuals of sound 0 are 0 in float64 and in the float32 emulation, its two
    # gradients are exactly 0.0, and it adds nothing to the sums
    inputs = R.make_tdoa_inputs(257, 7, zero_case=True)
    obs, sensors, sounds, c = inputs
    t, _d = R.tdoa_times64(sensors, sounds, c)
    assert np.all(t[0] == 0) and np.all(obs[0] == 0) and R.residual_margin(*inputs) >= 1e-6
    ref = R.tdoa_loss_and_grads_ref(*inputs, "l1")
    assert np.all(ref["sounds"][0][0] == 0) and np.all(ref["sounds"][1][0] == 0)
    assert ref["terms"]["loss"][0] == 0 and np.all(ref["terms"]["sensors"][0] == 0) and ref["terms"]["C"][0] == 0
    for order in ("tree", "ascending"):
        emu = R.emu_tdoa_loss_and_grads(*inputs, "l1", order)
        assert np.all(emu["sounds"][0] == 0.0)
        ratios = R.worst_ratio(emu, ref)
        print(f"zero case, {order}: {ratios}")
        assert max(ratios.values()) <= 1


@pytest.mark.parametrize("loss", LOSSES)
def test_emulations_are_inside_every_bound(cases, loss):
    worst = {}
    for n in SIZES:
        inputs, ref = cases[n, loss]
        for order in ("tree", "ascending"):
            ratios = R.worst_ratio(R.emu_tdoa_loss_and_grads(*inputs, loss, order), ref)
            print(f"N {n} {loss} {order}: error / bound {ratios}")
            for k, v in ratios.items():
                worst[k] = max(worst.get(k, 0), v)
            assert max(ratios.values()) <= 1, (n, order, ratios)
    print(f"{loss}: largest error / bound over all sizes and both orders {worst}")


@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("n", FAULT_SIZES)
def test_planted_faults_are_rejected(cases, n, loss):
    inputs, ref = cases[n, loss]
    for order in ("tree", "ascending"):
        # a sound missing from the sums: the one with the largest term of each output, and all beyond the first pass
        for fault in ("drop_largest", "drop_256"):
            ratios = R.worst_ratio(R.emu_tdoa_loss_and_grads(*inputs, loss, order, fault), ref)
            print(f"N {n} {loss} {order} {fault}: error / bound {ratios}")
            assert ratios["loss"] > 1 and ratios["sensors"] > 1, ratios
            assert ratios["sounds"] <= 1  # not a sum over the sounds: untouched
            # C: wherever the missing term is not itself negligible
            cterm = np.abs(ref["terms"]["C"])
            missing = cterm.max() if fault == "drop_largest" else cterm[R.KT:].sum()
            if missing > 2 * ref["C"][1] or fault == "drop_256":
                assert ratios["C"] > 1, (missing, ref["C"])
        if loss == "mse":
            ratios = R.worst_ratio(R.emu_tdoa_loss_and_grads(*inputs, loss, order, "mse_half"), ref)
            print(f"N {n} {loss} {order} mse_half: error / bound {ratios}")
            assert ratios["loss"] <= 1 and min(ratios["sensors"], ratios["sounds"], ratios["C"]) > 1
    # problem 1 reading problem 0's lags
    obs, sensors, sounds, c = inputs
    other = R.make_tdoa_inputs(n, 900 + n)
    batch = [np.stack([a, b]) for a, b in zip(inputs, other)]
    ref1 = R.tdoa_loss_and_grads_ref(*other, loss)
    good = R.emu_tdoa_batch(*batch, loss)
    bad = R.emu_tdoa_batch(*batch, loss, fault="lags0")
    assert max(R.worst_ratio(good[1], ref1).values()) <= 1 and max(R.worst_ratio(good[0], ref).values()) <= 1
    ratios = R.worst_ratio(bad[1], ref1)
    print(f"N {n} {loss} lags0: error / bound {ratios}")
    assert min(ratios.values()) > 1, ratios
    assert max(R.worst_ratio(bad[0], ref).values()) <= 1


@pytest.mark.parametrize("n", FAULT_SIZES)
def test_sign_of_zero_fault_is_rejected(n):
    inputs = R.make_tdoa_inputs(n, 7, zero_case=True)
    ref = R.tdoa_loss_and_grads_ref(*inputs, "l1")
    for order in ("tree", "ascending"):
        assert max(R.worst_ratio(R.emu_tdoa_loss_and_grads(*inputs, "l1", order), ref).values()) <= 1
        bad = R.emu_tdoa_loss_and_grads(*inputs, "l1", order, "sign0")
        ratios = R.worst_ratio(bad, ref)
        print(f"N {n} sign0 {order}: error / bound {ratios}")
        assert np.all(bad["sounds"][0] != 0.0) and ratios["sounds"] > 1 and ratios["sensors"] > 1, ratios


def _golden_pos(case):
    g = np.load(Path(__file__).resolve().parent / "golden" / "g24_calibration.npz", allow_pickle=False)
    args = json.loads(str(g[f"pos/{case}/cfg"]))["args"]
    return g, args


@pytest.mark.parametrize("case", ["defaults", "long"])
def test_restated_fit_follows_the_recorded_runs(case):
    """float32 tdoa_fit_ref on the recorded inputs: the recorded number of updates, and a curve inside the rule
    tests/test_gpu_calibration.py applies to the kernel: max(4 x spread, N x 2^-24 x ref)."""
    g, args = _golden_pos(case)
    lags = g[f"pos/{case}/lags"]
    run = R.tdoa_fit_ref(lags, g[f"pos/{case}/sensors0"], g[f"pos/{case}/sounds0"], loss="mse", **args)
    ref = g[f"pos/{case}/curve"].astype(np.float64)
    assert run["updates"] == int(g[f"pos/{case}/steps"]) and len(run["curve"]) == len(ref)
    spread = np.max(np.abs(g[f"pos/{case}/pert_curve"][:, :len(ref)].astype(np.float64) - ref), axis=0)
    diff = np.abs(run["curve"] - ref)
    bound = np.maximum(4 * spread, len(lags) * U24 * ref)
    worst = int(np.argmax(diff / bound))
    print(f"{case}: {run['updates']} updates; worst epoch {worst}: |restated - recorded| {diff[worst]:.3e} bound "
          f"{bound[worst]:.3e}")
    assert np.all(diff <= bound)
    for key in ("sensors", "sounds", "C"):
        want = g[f"pos/{case}/{key}"].astype(np.float64)
        sp = np.max(np.abs(g[f"pos/{case}/pert_{key}"].astype(np.float64) - want))
        err = np.max(np.abs(run[key] - want))
        print(f"{case} {key}: |restated - recorded| {err:.3e}, spread {sp:.3e}")
        assert err <= max(4 * sp, 2.0 ** -23 * np.max(np.abs(want)))


def test_early_stop_of_the_restated_fit():
    inputs = R.make_tdoa_inputs(65, 3)
    for patience in (0, 3):
        run = R.tdoa_fit_ref(inputs[0], inputs[1], inputs[2], loss="mse", num_epochs=10, C=float(inputs[3]), sr=1,
                             eps=1e9, patience=patience)
        # the first loss beats +inf, none after it counts as an improvement
        assert run["updates"] == patience + 1 and len(run["curve"]) == patience + 2
        assert run["stop_loss"] == run["curve"][-1]
        assert np.array_equal(run["sounds"][:, :2], run["history"][-1][1]) and np.all(run["sounds"][:, 2] == 0)


ACTS = [nn.Identity, nn.ReLU, nn.SiLU, nn.LeakyReLU, nn.ELU, nn.Tanh]


def bn_network(act, n_in=3, hidden=(7, 5), seed=0, bias=True):
    """Linear -> BatchNorm1d -> act per hidden width, then Linear to 2: the layout of calibration.FCNN's Sequential.
    BatchNorm weights, biases and running statistics start at random values."""
    gen = torch.Generator().manual_seed(seed)
    mods, prev = [], n_in
    for w in hidden:
        bn = nn.BatchNorm1d(w)
        with torch.no_grad():
            bn.weight.copy_(0.5 + torch.rand(w, generator=gen))
            bn.bias.copy_(0.3 * torch.randn(w, generator=gen))
            bn.running_mean.copy_(torch.randn(w, generator=gen))
            bn.running_var.copy_(0.5 + torch.rand(w, generator=gen))
        mods += [nn.Linear(prev, w, bias=bias), bn, act()]
        prev = w
    mods.append(nn.Linear(prev, 2, bias=bias))
    net = nn.Sequential(*mods)
    with torch.no_grad():
        for m in net:
            if isinstance(m, nn.Linear):
                m.weight.copy_(torch.randn(m.weight.shape, generator=gen) / m.in_features ** 0.5)
                if bias:
                    m.bias.copy_(0.2 * torch.randn(m.bias.shape, generator=gen))
    return net


@pytest.mark.parametrize("act", ACTS, ids=lambda a: a.__name__)
@pytest.mark.parametrize("n", [2, 65, 1024])
def test_running_statistics_reference_and_faults(act, n):
    net = bn_network(act, seed=n)
    x = torch.randn(n, 3, generator=torch.Generator().manual_seed(n + 1)).numpy()
    ref = R.fcnn_running_stats_ref(net, x)
    # the values: torch's own modules in float64, one training-mode forward
    copy64 = R.train_fcnn_torch(net, x, np.zeros((n, 2), np.float32), 0.01, "l1", 1, torch.float64)
    for (rm, rv), ((m, _bm), (v, _bv)) in zip(R.running_stats_of(copy64), ref):
        assert np.allclose(rm, m, rtol=1e-12, atol=1e-14) and np.allclose(rv, v, rtol=1e-12, atol=1e-14)
    emu = R.emu_fcnn_running_stats(net, x)
    for layer, ((m, bm), (v, bv)) in enumerate(ref):
        rm, rv = np.max(np.abs(emu[layer][0] - m) / bm), np.max(np.abs(emu[layer][1] - v) / bv)
        print(f"{act.__name__} N {n} layer {layer}: emulation error / bound: mean {rm:.3f} var {rv:.3f}; "
              f"largest relative bound: mean {np.max(bm / np.abs(m)):.2e} var {np.max(bv / v):.2e}")
        assert rm <= 1 and rv <= 1
    swapped = R.emu_fcnn_running_stats(net, x, "momenta_swapped")
    biased = R.emu_fcnn_running_stats(net, x, "biased_var")
    for layer, ((m, bm), (v, bv)) in enumerate(ref):
        assert np.all(np.abs(swapped[layer][1] - v) > bv) and np.max(np.abs(swapped[layer][0] - m) / bm) > 1
        assert np.all(np.abs(biased[layer][1] - v) > bv)
        assert np.all(np.abs(biased[layer][0] - m) <= bm)


def test_running_statistics_reference_over_epochs():
    """More than one epoch: the reference trains torch's modules; after 1 epoch both routes agree."""
    net = bn_network(nn.Tanh, seed=5)
    gen = torch.Generator().manual_seed(6)
    x, y = torch.randn(65, 3, generator=gen).numpy(), torch.randn(65, 2, generator=gen).numpy()
    one = R.running_stats_of(R.train_fcnn_torch(net, x, y, 0.01, "mse", 1, torch.float64))
    for (rm, rv), ((m, _bm), (v, _bv)) in zip(one, R.fcnn_running_stats_ref(net, x)):
        assert np.allclose(rm, m, rtol=1e-12, atol=1e-14) and np.allclose(rv, v, rtol=1e-12, atol=1e-14)
    three = R.fcnn_running_stats_ref(net, x, y, 0.01, "mse", 3)
    assert len(three) == 2 and all(not np.allclose(a[1], b[1]) for a, b in zip(three, one))
    assert all(int(m.num_batches_tracked) == 0 for m in net if isinstance(m, nn.BatchNorm1d)), "the input is a copy"
