"""CPU-only: the host side of fit_cnn (model.py) -- the NAdam / warm-restart tables, the g26_cnn_train fixture's own
conditions, the argument errors raised before any GPU call, and the float64 references of tests/cnn_train_ref.py
against torch autograd."""
import json
import sys
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

sys.path.insert(0, str(Path(__file__).resolve().parent))
import cnn_train_ref as R  # noqa: E402

CASES = ["l1_silu_bn", "l1_silu_pool", "mse_tanh_dil_bn", "l1_silu_bn_stop"]


@pytest.fixture(scope="module")
def g(golden):
    return golden("g26_cnn_train")


def our_model(g, case):
    from onset_fingerprinting_amd import model
    cfg = json.loads(str(g[f"{case}/cfg"]))
    kw = dict(cfg["kwargs"])
    kw["activation"], kw["loss"] = getattr(nn, kw["activation"]), getattr(F, kw["loss"])
    m = model.CNN(cfg["width"], 2, channels=cfg["channels"], dropout_rate=0.0, lr=cfg["lr"], **kw)
    pre = f"{case}/sd0/"
    sd0 = {k[len(pre):]: torch.from_numpy(g[k]) for k in g.files if k.startswith(pre)}
    return cfg, m, sd0


def comparable_prefix(ref, pert):
    n = len(ref)
    with np.errstate(invalid="ignore"):
        spread = np.max(np.abs(pert[:, :n].astype(np.float64) - ref.astype(np.float64)), axis=0)
    bad = np.isnan(spread) | (spread > 1e-5 * ref)
    return (int(np.argmax(bad)) if bad.any() else n), spread


def test_rate_table_reproduces_torch_nadam():
    """A float64 numpy NAdam driven only by cnn_rate_table's rows against torch.optim.NAdam +
    CosineAnnealingWarmRestarts(250, 1) in float64 on random gradients, 600 steps (two restarts)."""
    from onset_fingerprinting_amd import model
    steps, lr = 600, 0.01
    table = model.cnn_rate_table(lr, steps)
    assert table.shape == (steps, 5) and table.dtype == np.float64
    fac = model.cnn_step_factors(table)
    torch.manual_seed(1)
    p = nn.Parameter(torch.randn(64, dtype=torch.float64))
    q = p.detach().numpy().copy()
    opt = torch.optim.NAdam([p], lr=lr)
    sched = torch.optim.lr_scheduler.CosineAnnealingWarmRestarts(opt, 250, 1)
    m, v = np.zeros(64), np.zeros(64)
    worst = 0.0
    for e in range(steps):
        grad = torch.randn(64, dtype=torch.float64)
        assert opt.param_groups[0]["lr"] == table[e, 0]
        p.grad = grad.clone()
        opt.step()
        sched.step()
        gr = grad.numpy()
        m = m + (1 - 0.9) * (gr - m)
        v = v * 0.999 + (1 - 0.999) * gr * gr
        denom = np.sqrt(v / fac[e, 2]) + 1e-8
        q = q + fac[e, 0] * gr / denom
        q = q + fac[e, 1] * m / denom
        worst = max(worst, float(np.max(np.abs(q - p.detach().numpy()) / np.abs(q))))
    print(f"largest relative distance of the parameters over {steps} steps: {worst:.3e}")
    assert worst <= 1e-12
    assert table[0, 0] == lr and table[250, 0] == lr and table[500, 0] == lr and table[249, 0] < lr * 1e-3
    rows = model._cnn_device_rows(lr, steps)
    assert rows.dtype == np.float32 and rows.shape == (steps, 4)
    assert np.array_equal(rows[:, :3], fac.astype(np.float32))


@pytest.mark.parametrize("case", CASES)
def test_rates_equal_the_recorded_learning_rates(g, case):
    from onset_fingerprinting_amd import model
    cfg, _m, _sd = our_model(g, case)
    rec = g[f"{case}/rates"]
    assert np.array_equal(model.cnn_rates(cfg["lr"], cfg["epochs"])[:len(rec)], rec)


@pytest.mark.parametrize("case", CASES)
def test_fixture_conditions(g, case):
    cfg, m, sd0 = our_model(g, case)
    ref = g[f"{case}/errors"]
    prefix, _s = comparable_prefix(ref, g[f"{case}/pert_errors"])
    print(f"{case}: prefix {prefix} of {len(ref)}, loss {ref[0]:.5g} -> best {ref.min():.5g}")
    assert prefix >= min(24, len(ref)) and g[f"{case}/pert_errors"].shape[0] == 8
    assert ref.min() * 1.2 <= ref[0]
    if "patience" in cfg:
        stop = int(g[f"{case}/stop"])
        assert prefix >= 24 and stop < cfg["epochs"] and np.all(g[f"{case}/pert_stop"] == stop)
        assert len(g[f"{case}/val"]) == stop == len(ref) == len(g[f"{case}/val64"])
        # the rule of fit_cnn's docstring applied to the recorded validation curve gives the recorded epoch
        best, wait = np.inf, 0
        for e, v in enumerate(g[f"{case}/val"]):
            best, wait = (v, 0) if v < best else (best, wait + 1)
            if wait >= cfg["patience"]:
                break
        assert e + 1 == stop
    else:
        assert len(ref) == cfg["epochs"] >= 300
    own = m.state_dict()
    assert sorted(own) == sorted(sd0) and all(own[k].shape == sd0[k].shape for k in sd0)
    m.load_state_dict(sd0)


def test_argument_errors_come_before_any_gpu_call(monkeypatch):
    from onset_fingerprinting_amd import _lib, model

    def no_gpu(*a, **k):
        raise AssertionError("a GPU call was made")

    monkeypatch.setattr(_lib, "require_gpu", no_gpu)
    monkeypatch.setattr(_lib, "lib", no_gpu)
    x, y = torch.zeros(8, 3, 32), torch.zeros(8, 2)
    with pytest.raises(ValueError, match="dropout_rate=0.0"):
        model.fit_cnn(model.CNN(32, 2), x, y)  # the class default is 0.5
    with pytest.raises(ValueError, match="l1_loss"):
        model.fit_cnn(model.CNN(32, 2, dropout_rate=0.0, loss=F.smooth_l1_loss), x, y)
    m = model.CNN(32, 2, dropout_rate=0.0, batch_norm=True)
    m.conv_layers.bn1.momentum = None
    with pytest.raises(ValueError, match="momentum"):
        model.fit_cnn(m, x, y)
    m = model.CNN(32, 2, dropout_rate=0.0)
    m.conv_layers.act1 = nn.GELU()
    with pytest.raises(ValueError, match="GELU"):
        model.fit_cnn(m, x, y)
    with pytest.raises(ValueError, match="128"):
        model.fit_cnn(model.CNN(32, 2, layer_sizes=[129], dropout_rate=0.0), x, y)
    with pytest.raises(ValueError, match="512"):
        model.fit_cnn(model.CNN(513, 2, dropout_rate=0.0), torch.zeros(8, 3, 513), y)
    with pytest.raises(ValueError, match="1024"):
        model.fit_cnn(model.CNN(32, 2, dropout_rate=0.0), torch.zeros(1025, 3, 32), torch.zeros(1025, 2))
    with pytest.raises(ValueError, match="limit is 1..3"):
        model.fit_cnn(model.CNN(32, 2, layer_sizes=[4, 4, 4, 4], dropout_rate=0.0), x, y)
    with pytest.raises(ValueError, match="patience"):
        model.fit_cnn(model.CNN(32, 2, dropout_rate=0.0), x, y, patience=3)
    with pytest.raises(ValueError):
        model.cnn_loss_and_grads_device(model.CNN(32, 2), x, y)
    conf = model.CNN(32, 2, dropout_rate=0.0, lr=0.02).configure_optimizers()
    assert isinstance(conf["optimizer"], torch.optim.NAdam) and conf["optimizer"].param_groups[0]["lr"] == 0.02
    sched = conf["lr_scheduler"]
    assert isinstance(sched["scheduler"], torch.optim.lr_scheduler.CosineAnnealingWarmRestarts)
    assert (sched["scheduler"].T_0, sched["scheduler"].T_mult, sched["frequency"]) == (250, 1, 1)
    assert sched["monitor"] == "val_loss"


@pytest.mark.parametrize("k,dil,pad,groups,cin,cout,w", [(3, 1, 1, 1, 5, 6, 9), (5, 2, 4, 2, 6, 4, 17),
                                                         (2, 3, 0, 3, 3, 6, 8), (1, 1, 0, 1, 2, 3, 1)])
def test_conv_backward_reference_against_autograd(k, dil, pad, groups, cin, cout, w):
    rng = np.random.default_rng(k * 100 + w)
    x = rng.standard_normal((3, cin, w)).astype(np.float32)
    wt = rng.standard_normal((cout, cin // groups, k)).astype(np.float32)
    wc = w + 2 * pad - dil * (k - 1)
    dz = rng.standard_normal((3, cout, wc)).astype(np.float32)
    ref = R.conv1d_backward_ref(x, wt, dz, pad, dil, groups)
    xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    wtt = torch.tensor(wt, dtype=torch.float64, requires_grad=True)
    b = torch.zeros(cout, dtype=torch.float64, requires_grad=True)
    F.conv1d(xt, wtt, b, padding=pad, dilation=dil, groups=groups).backward(torch.tensor(dz, dtype=torch.float64))
    for name, t in (("dx", xt), ("dw", wtt), ("db", b)):
        val, bound = ref[name]
        assert val.shape == tuple(t.shape) == bound.shape
        assert np.max(np.abs(val - t.grad.numpy())) <= 1e-12 * max(1.0, np.max(np.abs(val)))
        assert np.all(bound >= 0)


@pytest.mark.parametrize("n,C,w", [(3, 4, 5), (2, 3, 1), (7, 2, 11)])
def test_batchnorm_reference_against_autograd(n, C, w):
    rng = np.random.default_rng(n * 10 + w)
    x = (rng.standard_normal((n, C, w)) * 2 + 0.5).astype(np.float32)
    ga, be = rng.standard_normal(C).astype(np.float32), rng.standard_normal(C).astype(np.float32)
    rm, rv = rng.standard_normal(C).astype(np.float32), rng.uniform(0.5, 2, C).astype(np.float32)
    dy = rng.standard_normal((n, C, w)).astype(np.float32)
    fwd = R.batchnorm_train_forward_ref(x, ga, be, rm, rv, 1e-5, 0.1)
    bwd = R.batchnorm_train_backward_ref(x, ga, dy, 1e-5)
    bn = nn.BatchNorm1d(C, momentum=float(np.float32(0.1))).double().train()
    with torch.no_grad():
        bn.weight.copy_(torch.tensor(ga)), bn.bias.copy_(torch.tensor(be))
        bn.running_mean.copy_(torch.tensor(rm)), bn.running_var.copy_(torch.tensor(rv))
    xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    yt = bn(xt)
    yt.backward(torch.tensor(dy, dtype=torch.float64))
    close = lambda a, b, tol=1e-9: np.max(np.abs(a - b)) <= tol * max(1.0, np.max(np.abs(b)))
    assert close(fwd["y"][0], yt.detach().numpy())
    # 1 - momentum is the float32 difference in the reference and the double one in torch
    assert close(fwd["running_mean"][0], bn.running_mean.numpy(), 1e-7)
    assert close(fwd["running_var"][0], bn.running_var.numpy(), 1e-7)
    assert close(bwd["dx"][0], xt.grad.numpy()) and close(bwd["dgamma"][0], bn.weight.grad.numpy())
    assert close(bwd["dbeta"][0], bn.bias.grad.numpy())
    assert close(fwd["mean"][0], x.astype(np.float64).mean((0, 2)))
    assert close(fwd["rstd"][0], 1 / np.sqrt(x.astype(np.float64).var((0, 2)) + 1e-5))
    for d in (fwd, bwd):
        for val, bound in d.values():
            assert bound.shape == val.shape and np.all(bound >= 0)


@pytest.mark.parametrize("loss", [0, 1], ids=["l1", "mse"])
@pytest.mark.parametrize("n,Fe,O", [(1, 1, 1), (5, 7, 3), (65, 257, 3), (129, 40, 16)])
def test_linear_head_reference_against_autograd(n, Fe, O, loss):
    """nn.Linear + F.l1_loss / F.mse_loss in float64.  The reference scales d loss / d out by the float32 1 / (n O) the
    kernel receives, autograd by the exact quotient: the ratio of the two is taken out before comparing."""
    h, w, b, y = R.linear_head_inputs(n, Fe, O)
    ref = R.linear_head_ref(h, w, b, y, loss)
    lin = nn.Linear(Fe, O).double()
    with torch.no_grad():
        lin.weight.copy_(torch.tensor(w)), lin.bias.copy_(torch.tensor(b))
    ht = torch.tensor(h, dtype=torch.float64, requires_grad=True)
    out = lin(ht)
    out.retain_grad()
    v = (F.mse_loss if loss else F.l1_loss)(out, torch.tensor(y, dtype=torch.float64))
    v.backward()
    scale = float(np.float32(1.0) / np.float32(n * O)) * (n * O)
    assert abs(scale - 1) <= 2.0 ** -24
    close = lambda a, t, s=1.0: np.max(np.abs(a - s * t.detach().numpy())) <= 1e-12 * max(1.0, np.max(np.abs(a)))
    assert close(ref["out"][0], out) and close(ref["loss"][0], v.reshape(1))
    assert close(ref["dy"][0], out.grad, scale) and close(ref["dh"][0], ht.grad, scale)
    assert close(ref["dw"][0], lin.weight.grad, scale) and close(ref["db"][0], lin.bias.grad, scale)
    shapes = {"out": (n, O), "dy": (n, O), "loss": (1,), "dw": (O, Fe), "db": (O,), "dh": (n, Fe)}
    for name, (val, bound) in ref.items():
        assert val.shape == bound.shape == shapes[name] and np.all(bound >= 0) and np.all(np.isfinite(bound))
    # the bounds are roundings, not slack: a few units of float32 on values of order 1
    assert np.all(ref["out"][1] <= 4 * R.U * (1 + np.abs(ref["out"][0])))


def test_linear_head_shapes_and_the_margin_of_l1():
    """The table of the GPU test: every axis in full, the corners, and for every shape a residual |out - y| at least
    2^16 bounds of out away from the kink of L1 (a condition on the inputs, asserted here without a GPU)."""
    S = set(R.HEAD_SHAPES)
    assert len(S) == len(R.HEAD_SHAPES) == 9 + 5 + 5 - 2 + 4
    assert {s[0] for s in S} == set(R.HEAD_N) and {s[1] for s in S} == set(R.HEAD_F)
    assert {s[2] for s in S} == set(R.HEAD_O)
    assert {(1, 1, 1), (1024, 600, 16), (129, 257, 15), (257, 255, 1)} <= S
    for n, Fe, O in R.HEAD_SHAPES:
        h, w, b, y = R.linear_head_inputs(n, Fe, O)
        margin = R.l1_margin(R.linear_head_ref(h, w, b, y, 0), y)
        print(f"n {n} F {Fe} O {O}: smallest |out - y| / bound of out {margin:.3g}")
        assert margin >= 2.0 ** 16
