"""CPU-only: the host side of calibration.train_location_model / optimize_positions / calibration_locations against
the reference's recorded behaviour (tests/golden/g24_calibration.npz, made by make_golden_calib.py): signatures,
calibration_locations, argument errors raised before the GPU is asked for, and the per-epoch learning rates."""
import inspect
import json

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from onset_fingerprinting_amd import calibration

TRAIN_CASES = ["l1_silu6", "l1_silu11_bn", "l1_default", "mse_tanh8x8", "mse_tanh8x8_stop"]
POS_CASES = ["defaults", "long"]


@pytest.fixture(scope="module")
def g(golden):
    return golden("g24_calibration")


@pytest.mark.parametrize("i", range(5))
def test_calibration_locations_equal_the_reference(g, i):
    args = json.loads(str(g[f"loc/{i}/args"]))
    want = g[f"loc/{i}/out"]
    got = calibration.calibration_locations(**args)
    assert isinstance(got, list) and all(isinstance(t, tuple) for t in got)
    assert len(got) == len(want) and all(len(t) == want.shape[1] for t in got)
    assert np.array_equal(np.array(got, np.float64), want)


def test_calibration_locations_refuses_a_float_z():
    with pytest.raises(AssertionError):
        calibration.calibration_locations(4, 2, 0.5, add_z=0.5)


@pytest.mark.parametrize("name", ["train_location_model", "optimize_positions", "calibration_locations"])
def test_signatures_follow_the_reference(g, name):
    want = json.loads(str(g["sig/" + name]))
    params = list(inspect.signature(getattr(calibration, name)).parameters.values())
    positional = [p for p in params if p.kind is p.POSITIONAL_OR_KEYWORD]
    ref_positional = [(n, d) for n, d in want if not n.startswith("**")]
    assert [p.name for p in positional] == [n for n, _d in ref_positional]
    for p, (_n, d) in zip(positional, ref_positional):
        if d == "<required>":
            assert p.default is p.empty
        elif callable(p.default):
            assert p.default.__name__ == d
        else:
            assert p.default == d and type(p.default) is type(d)
    if any(n.startswith("**") for n, _d in want):
        assert any(p.kind is p.VAR_KEYWORD for p in params)
    # what this package adds is keyword-only
    extra = [p for p in params if p.kind not in (p.POSITIONAL_OR_KEYWORD, p.VAR_KEYWORD)]
    assert all(p.kind is p.KEYWORD_ONLY for p in extra)


def _data(n=12):
    gen = torch.Generator().manual_seed(3)
    return torch.randn(n, 3, generator=gen), torch.randn(n, 3, generator=gen)


def test_argument_errors_come_before_the_gpu():
    x, y = _data()
    with pytest.raises(ValueError, match="dropout"):
        calibration.train_location_model(x, y, dropout=0.1)
    with pytest.raises(ValueError, match="lossfun"):
        calibration.train_location_model(x, y, lossfun=F.smooth_l1_loss)
    with pytest.raises(ValueError, match="lossfun"):
        calibration.train_location_model(x, y, lossfun=lambda a, b: F.l1_loss(a, b))
    with pytest.raises(ValueError, match="more than 1 value"):
        calibration.train_location_model(x[:1], y[:1])
    with pytest.raises(ValueError, match="128"):
        calibration.train_location_model(x, y, hidden_layers=[129])
    with pytest.raises(ValueError, match="8"):
        calibration.train_location_model(x, y, hidden_layers=[4] * 8)
    with pytest.raises(ValueError, match="1024"):
        calibration.train_location_model(torch.zeros(1025, 3), torch.zeros(1025, 3))
    lags = torch.zeros(12, 2)
    with pytest.raises(ValueError, match="4 sensors"):
        calibration.optimize_positions(lags, torch.zeros(3, 3), y)
    with pytest.raises(ValueError, match="lossfun"):
        calibration.optimize_positions(lags, torch.zeros(4, 3), y, lossfun=F.huber_loss)
    with pytest.raises(ValueError, match=r"\[N, 2\]"):
        calibration.optimize_positions(torch.zeros(12, 3), torch.zeros(4, 3), y)
    with pytest.raises(ValueError, match="dropout"):
        calibration.fcnn_loss_and_grads_device(calibration.FCNN(3, 2, dropout=0.2), x, y[:, :2])


def test_without_a_gpu_the_calls_fail_loudly():
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    from onset_fingerprinting_amd._lib import OnsetFPError
    x, y = _data()
    with pytest.raises(OnsetFPError):
        calibration.train_location_model(x, y, num_epochs=3)
    with pytest.raises(OnsetFPError):
        calibration.optimize_positions(torch.zeros(12, 2), torch.zeros(4, 3), y, num_epochs=3)


@pytest.mark.parametrize("case", TRAIN_CASES)
def test_location_model_rates_equal_the_recorded_ones_bit_for_bit(g, case):
    cfg = json.loads(str(g[f"train/{case}/cfg"]))
    want = g[f"train/{case}/rates"]
    got = calibration.location_model_rates(cfg["lr"], cfg["num_epochs"])
    assert got.dtype == np.float64 and len(got) == cfg["num_epochs"] >= len(want)
    assert np.array_equal(got[:len(want)].view(np.uint64), want.view(np.uint64))
    table = calibration.location_model_rate_table(cfg["lr"], cfg["num_epochs"])
    assert table.dtype == np.float32 and table.shape == (cfg["num_epochs"], 2)
    t = np.arange(1, cfg["num_epochs"] + 1)
    assert np.allclose(table[:, 0], got / (1 - 0.9 ** t), rtol=1e-6) and np.allclose(table[:, 1],
                                                                                    np.sqrt(1 - 0.999 ** t), rtol=1e-6)


@pytest.mark.parametrize("case", POS_CASES)
def test_position_rates_equal_the_recorded_ones_bit_for_bit(g, case):
    args = json.loads(str(g[f"pos/{case}/cfg"]))["args"]
    lr, num_epochs = args.get("lr", 0.01), args.get("num_epochs", 1000)
    want = g[f"pos/{case}/rates"]
    got = calibration.position_rates(lr, num_epochs)
    assert got.shape == (num_epochs, 3) and len(want) <= num_epochs
    assert np.array_equal(got[:len(want)].view(np.uint64), want.view(np.uint64))


def test_fresh_models_follow_the_reference_construction_order(g):
    """The same torch.manual_seed gives the start the reference drew."""
    from torch import nn
    for case in TRAIN_CASES:
        cfg = json.loads(str(g[f"train/{case}/cfg"]))
        kw = dict(cfg["kwargs"])
        if "activation" in kw:
            kw["activation"] = getattr(nn, kw["activation"])
        torch.manual_seed(cfg["seed"])
        sd = calibration.FCNN(3, 2, **kw).state_dict()
        keys = [k[len(f"train/{case}/sd0/"):] for k in g.files if k.startswith(f"train/{case}/sd0/")]
        assert sorted(keys) == sorted(sd)
        for k in keys:
            assert np.array_equal(sd[k].numpy(), g[f"train/{case}/sd0/{k}"]), (case, k)
