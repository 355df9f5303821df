"""CPU-only: the host side of fit_cnnrnn (model.py) -- the rate table, the g28_cnnrnn_train fixture's own conditions,
the argument errors raised before any GPU call, the site-3 mask of the random stream, and the float64 references of
tests/cnnrnn_train_ref.py against torch autograd."""
import json
import sys
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

sys.path.insert(0, str(Path(__file__).resolve().parent))
import cnnrnn_train_ref as R  # noqa: E402
import train_random_ref as RR  # noqa: E402

CASES = ["l1_silu", "mse_tanh_bn_pool", "l1_silu_bn_wide", "l1_silu_stop"]
f64 = np.float64


@pytest.fixture(scope="module")
def g(golden):
    return golden("g28_cnnrnn_train")


def our_model(g, case):
    from onset_fingerprinting_amd import model
    cfg = json.loads(str(g[f"{case}/cfg"]))
    kw = dict(cfg["kwargs"])
    kw["activation"], kw["loss"] = getattr(nn, kw["activation"]), getattr(F, kw["loss"])
    m = model.CNNRNN(cfg["width"], 2, channels=cfg["channels"], dropout_rate=0.0, lr=cfg["lr"], **kw)
    pre = f"{case}/sd0/"
    sd0 = {k[len(pre):]: torch.from_numpy(g[k]) for k in g.files if k.startswith(pre)}
    return cfg, m, sd0


def comparable_prefix(ref, pert):
    n = len(ref)
    with np.errstate(invalid="ignore"):
        spread = np.max(np.abs(pert[:, :n].astype(f64) - ref.astype(f64)), axis=0)
    bad = np.isnan(spread) | (spread > 1e-5 * ref)
    return (int(np.argmax(bad)) if bad.any() else n), spread


@pytest.mark.parametrize("case", CASES)
def test_fixture_conditions(g, case):
    cfg, m, sd0 = our_model(g, case)
    ref = g[f"{case}/errors"]
    prefix, _s = comparable_prefix(ref, g[f"{case}/pert_errors"])
    pre = f"{case}/g64/"
    tops = {k[len(pre):]: float(np.max(np.abs(g[k]))) for k in g.files if k.startswith(pre)}
    low = min(tops, key=tops.get)
    print(f"{case}: prefix {prefix} of {len(ref)}, loss {ref[0]:.5g} -> best {ref.min():.5g}; smallest share of the "
          f"largest float64 start gradient {tops[low] / max(tops.values()):.3g} ({low})")
    assert prefix >= 24 and g[f"{case}/pert_errors"].shape[0] == 8
    assert ref.min() * 1.2 <= ref[0]
    if "patience" in cfg:
        stop = int(g[f"{case}/stop"])
        assert stop < cfg["epochs"] and stop <= prefix and np.all(g[f"{case}/pert_stop"] == stop)
        assert len(g[f"{case}/val"]) == stop == len(ref) == len(g[f"{case}/val64"]) == len(g[f"{case}/errors64"])
        # the rule of fit_cnn's docstring applied to the recorded validation curve gives the recorded epoch, and a
        # patience one shorter would have stopped earlier: the recorded stop is not the first stall
        stops = {}
        for patience in (cfg["patience"] - 1, cfg["patience"]):
            best, wait = np.inf, 0
            for e, v in enumerate(g[f"{case}/val"]):
                best, wait = (v, 0) if v < best else (best, wait + 1)
                if wait >= patience:
                    break
            stops[patience] = e + 1
        print(f"{case}: stops {stops}")
        assert stops[cfg["patience"]] == stop and stops[cfg["patience"] - 1] < stop
    else:
        assert len(ref) == cfg["epochs"] >= 300
    own = m.state_dict()
    assert sorted(own) == sorted(sd0) and all(own[k].shape == sd0[k].shape for k in sd0)
    m.load_state_dict(sd0)
    ps, _st = model_tensors(m)
    assert [n for n, _t in ps] == [k for k, _p in m.named_parameters()]


def model_tensors(m):
    from onset_fingerprinting_amd import model
    return model._cnnrnn_tensors(m)


@pytest.mark.parametrize("case", CASES)
def test_rates_equal_the_recorded_learning_rates(g, case):
    from onset_fingerprinting_amd import model
    cfg, _m, _sd = our_model(g, case)
    rec = g[f"{case}/rates"]
    assert np.array_equal(model.cnnrnn_rates(cfg["lr"], cfg["epochs"])[:len(rec)], rec)


def test_rates_come_back_up_after_the_half_period():
    from onset_fingerprinting_amd import model
    r = model.cnnrnn_rates(0.01, 250)
    assert r.dtype == np.float64 and r[0] == 0.01 and r[100] < 1e-12 and r[200] > 0.0099 and r[150] > r[100]
    rows = model._cnnrnn_device_rows(0.01, 250)
    table = np.array(model.cnn_rate_table(0.01, 250))
    table[:, 0] = r
    assert rows.dtype == np.float32 and np.array_equal(rows[:, :3], model.cnn_step_factors(table).astype(np.float32))


# ---- the float64 references against torch autograd ------------------------------------------------------------------
def close(name, got, ref, tol=1e-11):
    ref = np.asarray(ref, f64)
    err = float(np.max(np.abs(np.asarray(got, f64) - ref))) if ref.size else 0.0
    top = float(np.max(np.abs(ref))) if ref.size else 0.0
    print(f"{name}: max |ref - torch| {err:.3e} of {top:.3e}")
    assert err <= tol * max(top, 1e-300), name


def test_linear_backward_reference():
    rng = np.random.default_rng(0)
    x, w, dy = rng.standard_normal((9, 5)), rng.standard_normal((4, 5)), rng.standard_normal((9, 4))
    xt, wt = torch.tensor(x, requires_grad=True), torch.tensor(w, requires_grad=True)
    b = torch.zeros(4, dtype=torch.float64, requires_grad=True)
    (F.linear(xt, wt, b) * torch.tensor(dy)).sum().backward()
    ref = R.linear_backward_ref(x, w, dy)
    close("dx", ref["dx"][0], xt.grad.numpy())
    close("dw", ref["dw"][0], wt.grad.numpy())
    close("db", ref["db"][0], b.grad.numpy())
    assert all(np.all(v[1] > 0) and v[1].shape == v[0].shape for v in ref.values())


@pytest.mark.parametrize("shape", [(1, 1, 1, 1), (3, 5, 7, 4), (2, 16, 9, 6)], ids=str)
@pytest.mark.parametrize("gain", [1.0, 20.0])
def test_gru_reference(shape, gain):
    n, T, Fe, H = shape
    torch.manual_seed(n + T + Fe + H)
    gru = nn.GRU(Fe, H, batch_first=True).double()
    with torch.no_grad():
        for p in gru.parameters():
            p.mul_(gain)
    x = torch.randn(n, T, Fe, dtype=torch.float64, requires_grad=True)
    dout = torch.randn(n, T, H, dtype=torch.float64)
    y, _h = gru(x)
    (y * dout).sum().backward()
    par = [p.detach().numpy() for p in (gru.weight_ih_l0, gru.weight_hh_l0, gru.bias_ih_l0, gru.bias_hh_l0)]
    out, gates = R.gru_forward_ref(x.detach().numpy(), *par)
    close("out", out, y.detach().numpy())
    grads = R.gru_backward_ref(x.detach().numpy(), par[0], par[1], out, gates, dout.numpy())
    for name, got, ref in zip(("dx", "dw_ih", "dw_hh", "db_ih", "db_hh"), grads,
                              (x.grad, gru.weight_ih_l0.grad, gru.weight_hh_l0.grad, gru.bias_ih_l0.grad,
                               gru.bias_hh_l0.grad)):
        close(name, got, ref.numpy(), 1e-9)


@pytest.mark.parametrize("shape", [(1, 1, 2, 2), (3, 5, 8, 2), (2, 7, 6, 3)], ids=str)
@pytest.mark.parametrize("p", [0.0, 0.5])
def test_attention_reference(shape, p):
    """Against torch's own nn.MultiheadAttention without a mask; with a mask against the same formulas written with
    torch operations and differentiated by autograd (torch's module draws its own)."""
    n, T, E, heads = shape
    torch.manual_seed(n + T + E)
    att = nn.MultiheadAttention(E, heads, batch_first=True).double()
    with torch.no_grad():
        att.in_proj_bias.normal_()
    h = torch.randn(n, T, E, dtype=torch.float64, requires_grad=True)
    dctx = torch.randn(n, E, dtype=torch.float64)
    mask = R.attention_dropout_mask(5, 2, n, heads, T, p) if p else None
    w, b = att.in_proj_weight, att.in_proj_bias
    d = E // heads
    qkv = F.linear(h, w, b)
    q, k, v = (qkv[..., i * E:(i + 1) * E].reshape(n, T, heads, d).permute(0, 2, 1, 3) for i in range(3))
    pr = torch.softmax(q @ k.transpose(-1, -2) / d ** 0.5, -1)
    if mask is not None:
        pr = pr * torch.from_numpy(mask).double()
    ctx_t = (pr @ v).permute(0, 2, 1, 3).reshape(n, T, E).mean(1)
    if mask is None:  # the formulas above are the module's: out_proj taken back out of its output
        o = att.out_proj
        y = att(h, h, h, need_weights=False)[0].mean(1)
        back = torch.linalg.solve(o.weight.detach(), (y.detach() - o.bias.detach()).T).T
        close("ctx against nn.MultiheadAttention", ctx_t.detach().numpy(), back.numpy(), 1e-9)
    (ctx_t * dctx).sum().backward()
    hn, wn = h.detach().numpy(), w.detach().numpy()
    ctx, qkv_r, probs = R.attention_mean_forward_ref(hn, wn, b.detach().numpy(), heads, mask)
    close("ctx", ctx, ctx_t.detach().numpy())
    dh, dw, db = R.attention_mean_backward_ref(hn, wn, heads, qkv_r, probs, dctx.numpy(), mask)
    close("dh", dh, h.grad.numpy(), 1e-10)
    close("dw", dw, w.grad.numpy(), 1e-10)
    close("db", db, b.grad.numpy(), 1e-10)


def test_site_3_mask_is_the_stream_restated():
    """Element ((s heads + h) T + i) T + j of site 3: word idx % 4 of Philox counter (idx // 4, 3, epoch, 0)."""
    seed, epoch, n, heads, T, p = 0x1234567890ABCDEF, 7, 3, 2, 5, 0.5
    m = R.attention_dropout_mask(seed, epoch, n, heads, T, p)
    assert m.shape == (n, heads, T, T) and m.dtype == np.float32 and set(np.unique(m)) == {0.0, 2.0}
    flat = m.reshape(-1)
    for idx in (0, 1, 5, 17, 149):
        c = np.array([[idx // 4, 3, epoch, 0]], np.uint32)
        word = RR.philox4x32(c, RR.key_of(seed))[0, idx % 4]
        assert flat[idx] == (0.0 if word < RR.threshold(p) else 2.0)
    assert not np.array_equal(m, RR.dropout_mask(seed, epoch, n, heads * T * T, p).reshape(m.shape))  # site 0 differs
    assert not np.array_equal(m, R.attention_dropout_mask(seed, epoch + 1, n, heads, T, p))
    assert 0.3 < float((R.attention_dropout_mask(1, 0, 8, 2, 16, 0.5) == 0).mean()) < 0.7


# ---- the envelope ---------------------------------------------------------------------------------------------------
def small(**kw):
    from onset_fingerprinting_amd import model
    return model.CNNRNN(32, 2, channels=3, **{"layer_sizes": [4, 6], "n_hidden": 8, "dropout_rate": 0.0, **kw})


def test_every_refusal_comes_before_the_gpu(monkeypatch):
    from onset_fingerprinting_amd import _lib, data, model

    def no_gpu(*a, **k):
        raise AssertionError("a refused call reached the GPU")

    monkeypatch.setattr(_lib, "require_gpu", no_gpu)
    monkeypatch.setattr(_lib, "lib", no_gpu)
    x, y = torch.zeros(5, 3, 32), torch.zeros(5, 2)
    odd = small()
    odd.rnn = nn.GRU(32, 7, batch_first=True)
    wide = small()
    wide.rnn = nn.GRU(32, 130, batch_first=True)
    lstm = small()
    lstm.rnn = nn.LSTM(32, 8, batch_first=True)
    heads = small()
    heads.attention = nn.MultiheadAttention(8, 4, batch_first=True)
    nobias = small()
    nobias.fc = nn.Linear(8, 2, bias=False)
    steps = small()
    steps.conv_layers.conv2 = nn.Conv1d(4, 129, 3, padding=1)
    for what, m, match in (("two layers", small(n_rnn_layers=2), "n_rnn_layers=2"), ("odd hidden", odd, "even"),
                           ("hidden 130", wide, "at most 128"), ("an LSTM", lstm, "nn.GRU"),
                           ("dropout without seed", small(dropout_rate=0.5), "seed="),
                           ("a loss", small(loss=F.smooth_l1_loss), "loss"), ("4 heads", heads, "2 heads"),
                           ("fc without bias", nobias, "bias"), ("129 steps", steps, "channels"),
                           ("a wrong class", model.CNN(32, 2, dropout_rate=0.0), "not a CNNRNN")):
        for call in (model.fit_cnnrnn, model.cnnrnn_loss_and_grads_device):
            with pytest.raises(ValueError, match=match):
                call(m, x, y)
            print(f"{what}: refused by {call.__name__}")
    with pytest.raises(ValueError, match="1..1024"):
        model.fit_cnnrnn(small(), torch.zeros(1025, 3, 32), torch.zeros(1025, 2))
    with pytest.raises(ValueError, match="GRU expects"):
        model.fit_cnnrnn(small(), torch.zeros(5, 3, 30), y)
    with pytest.raises(ValueError, match="patience"):
        model.fit_cnnrnn(small(), x, y, patience=3)


def test_a_window_source_as_x_val_is_refused():
    from onset_fingerprinting_amd import data, model
    src = object.__new__(data.ShiftedWindows)  # _batch_of refuses by type, before it reads anything of the source
    with pytest.raises(ValueError, match="x_val"):
        model.fit_cnnrnn(small(), torch.zeros(5, 3, 32), torch.zeros(5, 2), x_val=src, y_val=torch.zeros(4, 2))


def test_stand_alone_wrappers_refuse_cpu_tensors():
    from onset_fingerprinting_amd import model
    with pytest.raises(ValueError, match="GPU tensor"):
        model._f32_cuda("x", torch.zeros(2, 3), (2, 3))
    with pytest.raises(ValueError, match="seed="):
        model._attention_random(0.5, None, 0)
