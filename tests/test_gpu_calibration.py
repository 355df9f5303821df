"""GPU: calibration.train_location_model / optimize_positions (csrc/ofp_train.hip) against the reference's recorded
runs (tests/golden/g24_calibration.npz, made by make_golden_calib.py).

The L1 training runs are chaotic (a last-bit disturbance of the inputs changes where the reference itself ends), so
nothing here asks for "equals the reference after 3 000 epochs".  The bounds come from the reference's own error:
  gradients   per tensor, max |ours - g64| <= 4 x max |g32 - g64| (floored at 2^-23 x max |g64|); the factor 4 covers
              a different but equally valid summation order
  trajectory  over the comparable prefix (the epochs before the 8 disturbed reference curves first stray more than
              1e-5 relative from the undisturbed one): |ours_e - ref_e| <= max(4 x spread_e, N x 2^-24 x loss_e)
  outcome     best and final loss at most the largest of the nine reference runs plus the width of their range (not
              less than the curve's own wobble); the stopping epoch inside their range widened by its width
Every figure is printed before it is asserted (run with -s to see them)."""
import json

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

pytestmark = pytest.mark.gpu

TRAIN_CASES = ["l1_silu6", "l1_silu11_bn", "l1_default", "mse_tanh8x8", "mse_tanh8x8_stop"]
CHAOTIC = ["l1_silu6", "l1_silu11_bn", "l1_default"]
POS_CASES = ["defaults", "long"]
U24, U23 = 2.0 ** -24, 2.0 ** -23


@pytest.fixture(scope="module")
def g(golden):
    return golden("g24_calibration")


def load_case(g, case):
    from onset_fingerprinting_amd import calibration
    cfg = json.loads(str(g[f"train/{case}/cfg"]))
    kw = dict(cfg["kwargs"])
    if "activation" in kw:
        kw["activation"] = getattr(nn, kw["activation"])
    model = calibration.FCNN(3, 2, **kw)
    pre = f"train/{case}/sd0/"
    model.load_state_dict({k[len(pre):]: torch.from_numpy(g[k]) for k in g.files if k.startswith(pre)})
    x, y = torch.from_numpy(g[f"train/{case}/x"]), torch.from_numpy(g[f"train/{case}/y"])
    call = dict(lr=cfg["lr"], lossfun=getattr(F, cfg["loss"]), num_epochs=cfg["num_epochs"], eps=cfg["eps"],
                patience=cfg["patience"])
    return cfg, model, x, y, call


_runs = {}


def our_run(g, case):
    """train_location_model on the golden's inputs and start; once per case and session."""
    from onset_fingerprinting_amd import calibration
    if case not in _runs:
        cfg, model, x, y, call = load_case(g, case)
        out, errors = calibration.train_location_model(x.cuda(), y.cuda(), print_every=10 ** 9, model=model, **call)
        _runs[case] = (out, np.array([float(e) for e in errors], np.float32))
    return _runs[case]


def comparable_prefix(ref, pert):
    """(prefix, spread): spread_e = largest distance of the disturbed curves from the undisturbed one."""
    n = len(ref)
    with np.errstate(invalid="ignore"):
        spread = np.max(np.abs(pert[:, :n].astype(np.float64) - ref.astype(np.float64)), axis=0)
    bad = np.isnan(spread) | (spread > 1e-5 * ref)
    return (int(np.argmax(bad)) if bad.any() else n), spread


def check_grads(named_ours, loss_ours, g32, g64, loss64, n, label):
    worst = 0.0
    for k, ref64 in g64.items():
        ours = named_ours[k].detach().cpu().numpy().astype(np.float64)
        err = np.max(np.abs(ours - ref64))
        err32 = max(np.max(np.abs(r[k].astype(np.float64) - ref64)) for r in (g32 if isinstance(g32, list) else [g32]))
        bound = max(4 * err32, U23 * np.max(np.abs(ref64)))
        print(f"{label} {k}: |ours - g64| {err:.3e}  |g32 - g64| {err32:.3e}  bound {bound:.3e}  "
              f"ratio to the reference's own error {err / max(err32, 1e-300):.2f}")
        worst = max(worst, err / bound)
        assert err <= bound, (label, k, err, bound)
    rel = abs(float(loss_ours) - loss64) / loss64
    print(f"{label} loss: ours {float(loss_ours):.9g} ref64 {loss64:.9g} rel {rel:.3e} bound {n * U24:.3e}")
    assert rel <= n * U24
    return worst


@pytest.mark.parametrize("case", TRAIN_CASES)
def test_gradients_at_the_start(g, case):
    from onset_fingerprinting_amd import calibration
    cfg, model, x, y, call = load_case(g, case)
    loss, grads = calibration.fcnn_loss_and_grads_device(model, x.cuda(), y[:, :2].cuda(), call["lossfun"])
    pre32, pre64 = f"train/{case}/g32/", f"train/{case}/g64/"
    g32 = {k[len(pre32):]: g[k] for k in g.files if k.startswith(pre32)}
    g64 = {k[len(pre64):]: g[k] for k in g.files if k.startswith(pre64)}
    assert sorted(grads) == sorted(g64)
    check_grads(grads, loss, g32, g64, float(g[f"train/{case}/loss64"]), len(x), case)


@pytest.mark.parametrize("case", TRAIN_CASES)
def test_trajectory_over_the_comparable_prefix(g, case):
    cfg, _m, x, _y, _c = load_case(g, case)
    ref = g[f"train/{case}/errors"]
    prefix, spread = comparable_prefix(ref, g[f"train/{case}/pert_errors"])
    assert prefix >= 8
    model, ours = our_run(g, case)
    assert len(ours) >= prefix
    diff = np.abs(ours[:prefix].astype(np.float64) - ref[:prefix])
    bound = np.maximum(4 * spread[:prefix], len(x) * U24 * ref[:prefix])
    worst = int(np.argmax(diff / bound))
    print(f"{case}: prefix {prefix} of {len(ref)}; worst epoch {worst}: |ours - ref| {diff[worst]:.3e} bound "
          f"{bound[worst]:.3e} (spread {spread[worst]:.3e}, loss {ref[worst]:.6g})")
    assert np.all(diff <= bound), (case, worst, diff[worst], bound[worst])
    if prefix == len(ref):  # a smooth case: the parameters are comparable too
        assert len(ours) == len(ref)
        flat = g[f"train/{case}/flat"].astype(np.float64)
        mine = torch.cat([p.detach().reshape(-1) for p in model.parameters()]).cpu().numpy().astype(np.float64)
        p_spread = np.max(np.abs(flat[1:] - flat[0]))
        p_err = np.max(np.abs(mine - flat[0]))
        p_bound = max(4 * p_spread, U23 * np.max(np.abs(flat[0])))
        print(f"{case}: parameters max |ours - ref| {p_err:.3e}, spread of the disturbed runs {p_spread:.3e}, bound "
              f"{p_bound:.3e}")
        assert p_err <= p_bound


@pytest.mark.parametrize("case", CHAOTIC)
def test_outcome_of_the_chaotic_cases(g, case):
    cfg, _m, _x, _y, _c = load_case(g, case)
    E = cfg["num_epochs"]
    ref = g[f"train/{case}/errors"]
    pert, pert_len = g[f"train/{case}/pert_errors"], g[f"train/{case}/pert_len"]
    prefix, _s = comparable_prefix(ref, pert)
    curves = [ref] + [pert[k, :pert_len[k]] for k in range(len(pert))]
    finals = np.array([c[-1] for c in curves], np.float64)
    bests = np.array([c.min() for c in curves], np.float64)
    lens = np.array([len(c) for c in curves])
    wobble = float(np.max(np.abs(np.diff(ref[-51:].astype(np.float64)))))
    _model, ours = our_run(g, case)
    w_final = max(finals.max() - finals.min(), wobble)
    w_best = max(bests.max() - bests.min(), wobble)
    msg = (f"{case}: reference finals {finals.tolist()} bests {bests.tolist()} lengths {lens.tolist()} wobble "
           f"{wobble:.4g}; ours final {ours[-1]:.8g} best {ours.min():.8g} length {len(ours)}")
    print(msg)
    assert ours[-1] <= finals.max() + w_final, msg
    assert ours.min() <= bests.max() + w_best, msg
    if lens.min() == E:
        assert len(ours) >= prefix, msg
    else:
        width = lens.max() - lens.min()
        assert lens.min() - width <= len(ours) <= lens.max() + width, msg


def pos_inputs(g, case):
    args = json.loads(str(g[f"pos/{case}/cfg"]))["args"]
    return (torch.from_numpy(g[f"pos/{case}/lags"]), torch.from_numpy(g[f"pos/{case}/sensors0"]),
            torch.from_numpy(g[f"pos/{case}/sounds0"]), args)


@pytest.mark.parametrize("case", POS_CASES)
def test_optimize_positions_follows_the_reference(g, case):
    from onset_fingerprinting_amd import calibration
    lags, sensors0, sounds0, args = pos_inputs(g, case)
    fit = calibration.optimize_positions_device(lags.cuda(), sensors0, sounds0, **args)
    steps, ref = int(g[f"pos/{case}/steps"]), g[f"pos/{case}/curve"]
    prefix, spread = comparable_prefix(ref, g[f"pos/{case}/pert_curve"])
    n = int(fit.epochs[0])
    ours = fit.losses[0].cpu().numpy()
    print(f"{case}: reference steps {steps}, losses evaluated {len(ref)}; ours steps {n}")
    # smooth: the nine reference runs stop at the same epoch, so the whole curve is comparable.  (The 1e-5 prefix
    # rule of the training cases does not apply: this loss is a mean of squared differences of nearly equal times,
    # and scaling the lags by one ulp already moves it by more than 1e-5 relative at epoch 0.)
    assert np.all(g[f"pos/{case}/pert_steps"] == steps) and np.isfinite(spread).all()
    prefix = len(ref)
    assert n == steps
    # the stopping epoch's loss is evaluated but not recorded by the reference; ours keeps it after the curve
    assert np.isfinite(ours[:len(ref)]).all() and np.isnan(ours[len(ref):]).all()
    diff = np.abs(ours[:prefix].astype(np.float64) - ref)
    bound = np.maximum(4 * spread, len(lags) * U24 * ref)
    worst = int(np.argmax(diff / bound))
    print(f"{case}: worst epoch {worst}: |ours - ref| {diff[worst]:.3e} bound {bound[worst]:.3e}")
    assert np.all(diff <= bound), (worst, diff[worst], bound[worst])
    for key, mine in (("sensors", fit.sensors[0]), ("sounds", fit.sounds[0]), ("C", fit.C[0])):
        want = g[f"pos/{case}/{key}"].astype(np.float64)
        sp = np.max(np.abs(g[f"pos/{case}/pert_{key}"].astype(np.float64) - want))
        err = np.max(np.abs(mine.cpu().numpy().astype(np.float64) - want))
        b = max(4 * sp, U23 * np.max(np.abs(want)))
        print(f"{case} {key}: max |ours - ref| {err:.3e}, spread of the disturbed runs {sp:.3e}, bound {b:.3e}")
        assert err <= b, (key, err, b)
    # the single call returns the same, on the input's device
    s, p, c = calibration.optimize_positions(lags, sensors0, sounds0, print_every=10 ** 9, **args)
    assert not s.is_cuda and s.shape == (4, 3) and p.shape == (len(lags), 3) and c.dim() == 0
    assert torch.equal(s, fit.sensors[0].cpu()) and torch.equal(p, fit.sounds[0].cpu()) and torch.equal(c, fit.C[0].cpu())


def test_determinism(g):
    from onset_fingerprinting_amd import calibration
    for case in ("l1_default", "l1_silu6"):
        cfg, model, x, y, call = load_case(g, case)
        call["num_epochs"] = min(call["num_epochs"], 500)
        a = calibration.train_location_models_device(x.cuda(), y.cuda(), models=[model], **call)
        b = calibration.train_location_models_device(x.cuda(), y.cuda(), models=[model], **call)
        for u, v in ((a.params, b.params), (a.stats, b.stats), (a.epochs, b.epochs)):
            assert torch.equal(u, v)
        assert torch.equal(a.losses.view(torch.int32), b.losses.view(torch.int32))
    lags, sensors0, sounds0, args = pos_inputs(g, "defaults")
    a = calibration.optimize_positions_device(lags.cuda(), sensors0, sounds0, **args)
    b = calibration.optimize_positions_device(lags.cuda(), sensors0, sounds0, **args)
    for u, v in ((a.sensors, b.sensors), (a.sounds, b.sounds), (a.C, b.C), (a.epochs, b.epochs)):
        assert torch.equal(u, v)
    assert torch.equal(a.losses.view(torch.int32), b.losses.view(torch.int32))


@pytest.mark.parametrize("kwargs", [dict(hidden_layers=[6], activation=nn.SiLU, batch_norm=False, bias=False), {}],
                         ids=["3-6-2", "default"])
def test_batch_entries_equal_single_calls(g, kwargs):
    """M = 300 problems (more than the CUs) that differ in start and lr."""
    from onset_fingerprinting_amd import calibration
    _cfg, _m, x, y, _c = load_case(g, "l1_silu6")
    M, E = 300, 120
    torch.manual_seed(5)
    models = [calibration.FCNN(3, 2, **kwargs) for _ in range(M)]
    lrs = [0.001 + 2e-5 * i for i in range(M)]
    run = calibration.train_location_models_device(x.cuda(), y.cuda(), lrs, num_epochs=E, models=models)
    assert len(run) == M and run.losses.shape == (M, E)
    for i in (0, 137, 299):
        one = calibration.train_location_models_device(x.cuda(), y.cuda(), lrs[i], num_epochs=E, models=[models[i]])
        assert torch.equal(one.params[0], run.params[i]) and torch.equal(one.stats[0], run.stats[i])
        assert torch.equal(one.losses[0].view(torch.int32), run.losses[i].view(torch.int32))
        assert int(one.epochs[0]) == int(run.epochs[i])
    # per-problem batches [M, N, F] give the same as one shared batch
    few = calibration.train_location_models_device(x.cuda().expand(3, -1, -1).contiguous(),
                                                   y.cuda().expand(3, -1, -1).contiguous(), lrs[:3], num_epochs=E,
                                                   models=models[:3])
    assert torch.equal(few.params, run.params[:3])


def test_position_batch_entries_equal_single_calls(g):
    from onset_fingerprinting_amd import calibration
    lags, sensors0, sounds0, _a = pos_inputs(g, "defaults")
    M, E = 300, 150
    gen = torch.Generator().manual_seed(9)
    sens = sensors0[None] + 0.002 * torch.randn(M, 4, 3, generator=gen)
    lrs = [0.01 + 1e-4 * i for i in range(M)]
    cs = [340.0 + 0.01 * i for i in range(M)]
    fit = calibration.optimize_positions_device(lags.cuda(), sens, sounds0, lr=lrs, num_epochs=E, C=cs)
    assert len(fit) == M
    for i in (0, 137, 299):
        one = calibration.optimize_positions_device(lags.cuda(), sens[i], sounds0, lr=lrs[i], num_epochs=E, C=cs[i])
        assert torch.equal(one.sensors[0], fit.sensors[i]) and torch.equal(one.sounds[0], fit.sounds[i])
        assert torch.equal(one.C[0], fit.C[i]) and int(one.epochs[0]) == int(fit.epochs[i])
        assert torch.equal(one.losses[0].view(torch.int32), fit.losses[i].view(torch.int32))


def test_early_stop(g):
    from onset_fingerprinting_amd import calibration
    case = "mse_tanh8x8_stop"
    cfg, _m, _x, _y, _c = load_case(g, case)
    ref = g[f"train/{case}/errors"]
    prefix, _s = comparable_prefix(ref, g[f"train/{case}/pert_errors"])
    assert prefix == len(ref) < cfg["num_epochs"], "the comparable prefix covers the stop"
    _model, ours = our_run(g, case)
    assert len(ours) == len(ref)
    # the same stop in both loops: the first loss always beats +inf, and with eps this large no later one counts as
    # an improvement, so `patience` more epochs update and the next one stops.  train_location_model records the
    # stopping epoch's loss, optimize_positions does not.
    _cfg, model, x, y, _call = load_case(g, "l1_silu6")
    _out, errors = calibration.train_location_model(x, y, eps=1e9, patience=4, print_every=10 ** 9, model=model)
    assert len(errors) == 6
    lags, sensors0, sounds0, _a = pos_inputs(g, "defaults")
    fit = calibration.optimize_positions_device(lags, sensors0, sounds0, eps=1e9, patience=4)
    assert int(fit.epochs[0]) == len(fit.errors(0)) == len(errors) - 1


def test_round_trip(g, golden, capsys):
    from onset_fingerprinting_amd import calibration
    from onset_fingerprinting_amd import multilateration as ml
    for case in ("l1_default", "mse_tanh8x8_stop"):
        model, _e = our_run(g, case)
        assert isinstance(model, calibration.FCNN) and not model.training
        pre = f"train/{case}/sd1/"
        want = {k[len(pre):]: g[k] for k in g.files if k.startswith(pre)}
        sd = model.state_dict()
        assert list(sd) == [k for k in sd if k in want] and len(sd) == len(want)
        assert all(tuple(sd[k].shape) == want[k].shape for k in want)
    model, errors = our_run(g, "l1_default")
    start = load_case(g, "l1_default")[1]
    for a, b in zip(model.network, start.network):
        if isinstance(a, nn.BatchNorm1d):
            assert int(a.num_batches_tracked) == int(b.num_batches_tracked) + len(errors)
    # a run ended by the early stop made no update after its last loss: the returned model reproduces it
    case = "mse_tanh8x8_stop"
    cfg, _m, x, y, _c = load_case(g, case)
    model, errors = our_run(g, case)
    with torch.no_grad():
        again = float(F.mse_loss(model(x.cuda()), y[:, :2].cuda()))
    rel = abs(again - float(errors[-1])) / float(errors[-1])
    # two float32 evaluations of a mean of 2N terms through three small dot products each
    bound = (2 * len(x) + 64) * U24
    print(f"{case}: last loss {float(errors[-1]):.9g}, forward of the returned model {again:.9g}, rel {rel:.3e}, "
          f"bound {bound:.3e}")
    assert rel <= bound
    # from recorded lags to a located hit without leaving the package
    g22 = golden("g22_locate")
    capsys.readouterr()
    two, errs = calibration.train_location_model(x[:, :2], y, num_epochs=40, hidden_layers=[6], activation=nn.SiLU,
                                                 batch_norm=False)
    out = capsys.readouterr().out
    assert out.startswith("Epoch 0, Loss ") and f"Epoch {len(errs) - 1}, Loss " in out.splitlines()[-1]
    m = ml.Multilaterate3D(**json.loads(str(g22["m3d/rt3/args"])), model=two)
    gd = torch.from_numpy(g22["rows/groups"][None].copy()).cuda()
    xy, status = ml.locate_groups_device(gd, None, m)
    assert xy.shape[0] == 1 and xy.shape[-1] == 2 and status.shape[:2] == xy.shape[:2]


def autograd_reference(model, ctor, x, y, lossfun, device="cuda"):
    """Loss and gradients of torch autograd on the model's own modules (batch statistics), float32 and float64."""
    ref = {}
    for dtype in (torch.float32, torch.float64):
        net = ctor()
        net.load_state_dict(model.state_dict())
        net = net.network.to(device, dtype).train()
        v = lossfun(net(x.to(device, dtype)), y.to(device, dtype))
        v.backward()
        ref[dtype] = ({"network." + k: p.grad.cpu().numpy() for k, p in net.named_parameters()}, float(v.detach()))
    return ref


@pytest.mark.parametrize("batch_norm", [False, True], ids=["plain", "bn"])
@pytest.mark.parametrize("act", [nn.Identity, nn.ReLU, nn.SiLU, nn.LeakyReLU, nn.ELU, nn.Tanh],
                         ids=lambda a: a.__name__)
def test_every_activation_backward(act, batch_norm):
    """Every activation of calibration.ACT_CODES, two hidden layers, in LDS, against torch autograd.  The bound is
    that of the golden cases; the reference's own float32 error is the larger of torch's two float32 backends (GPU
    and CPU kernels), since on tensors this small one backend alone can land within a fifth of an ulp of float64
    (measured: 3.4e-10 against 8.1e-10 on the first bias of the SiLU case, where one ulp of its largest entry is
    1.9e-9), which says nothing about what an equally valid summation order may lose."""
    from onset_fingerprinting_amd import calibration
    assert set(calibration.ACT_CODES) == {nn.Identity, nn.ReLU, nn.SiLU, nn.LeakyReLU, nn.ELU, nn.Tanh}
    torch.manual_seed(23)
    ctor = lambda: calibration.FCNN(3, 2, hidden_layers=[7, 5], activation=act, batch_norm=batch_norm)
    model = ctor()
    x, y = torch.randn(50, 3).cuda(), torch.randn(50, 2).cuda()
    loss, grads = calibration.fcnn_loss_and_grads_device(model, x, y, F.mse_loss)
    ref = autograd_reference(model, ctor, x, y, F.mse_loss)
    cpu32 = autograd_reference(model, ctor, x, y, F.mse_loss, "cpu")[torch.float32][0]
    check_grads(grads, loss, [ref[torch.float32][0], cpu32], ref[torch.float64][0], ref[torch.float64][1], 50,
                f"{act.__name__}{'+bn' if batch_norm else ''}")


@pytest.mark.parametrize("kwargs", [dict(activation=nn.Tanh, batch_norm=True),
                                    dict(activation=nn.SiLU, batch_norm=False)], ids=["tanh-bn", "silu"])
@pytest.mark.parametrize("lossfun", [F.l1_loss, F.mse_loss], ids=["l1", "mse"])
def test_envelope(kwargs, lossfun):
    """Width 128 x 6 hidden layers at N = 1 024 (beyond the LDS: the global work space) against torch autograd on
    the same GPU tensors, float32 and a float64 copy."""
    from onset_fingerprinting_amd import calibration
    torch.manual_seed(17)
    model = calibration.FCNN(3, 2, hidden_layers=[128] * 6, **kwargs)
    assert calibration.fcnn_train_lds_bytes(model, 1024) > 160 * 1024
    x, y = torch.randn(1024, 3).cuda(), torch.randn(1024, 2).cuda()
    loss, grads = calibration.fcnn_loss_and_grads_device(model, x, y, lossfun)
    ref = autograd_reference(model, lambda: calibration.FCNN(3, 2, hidden_layers=[128] * 6, **kwargs), x, y, lossfun)
    check_grads(grads, loss, ref[torch.float32][0], ref[torch.float64][0], ref[torch.float64][1], 1024, "envelope")
    with pytest.raises(ValueError, match="128"):
        calibration.fcnn_loss_and_grads_device(calibration.FCNN(3, 2, hidden_layers=[129]), x, y, lossfun)
