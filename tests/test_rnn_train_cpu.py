"""CPU-only: the host side of fit_rnn (model.py) -- the rate table, the g29_rnn_train fixture's own conditions, the
packing order, every refusal of the envelope raised before any GPU call, the site-4 mask of the random stream, and the
float64 references of tests/rnn_train_ref.py against torch autograd."""
import json
import sys
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

sys.path.insert(0, str(Path(__file__).resolve().parent))
import rnn_train_ref as R  # noqa: E402
import train_random_ref as RR  # noqa: E402

CASES = ["l1_two_layers", "mse_one_layer", "l1_three_layers", "l1_stop"]
f64 = np.float64


@pytest.fixture(scope="module")
def g(golden):
    return golden("g29_rnn_train")


@pytest.fixture
def no_gpu_calls(monkeypatch):
    """Any use of the library or of torch's device fails the test."""
    from onset_fingerprinting_amd import _lib

    def refuse(*a, **k):
        raise AssertionError("a GPU call was made before the arguments were checked")

    monkeypatch.setattr(_lib, "lib", refuse)
    monkeypatch.setattr(_lib, "require_gpu", refuse)
    monkeypatch.setattr(torch.cuda, "device", refuse)


def our_model(g, case):
    from onset_fingerprinting_amd import model
    cfg = json.loads(str(g[f"{case}/cfg"]))
    kw = dict(cfg["kwargs"])
    kw["loss"] = getattr(F, kw["loss"])
    m = model.RNN(cfg["width"], 2, channels=cfg["channels"], dropout_rate=0.0, lr=cfg["lr"], **kw)
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
    """The conditions of test_cnnrnn_train_cpu.py::test_fixture_conditions and the packing order.  The stop case ends
    after 11 epochs, so a prefix of 24 epochs and a loss 1.2 x below the start are asked of the cases that run their
    full length, and of the stop case that every epoch it ran is comparable."""
    from onset_fingerprinting_amd import model
    cfg, m, sd0 = our_model(g, case)
    ref = g[f"{case}/errors"]
    prefix, _s = comparable_prefix(ref, g[f"{case}/pert_errors"])
    pre = f"{case}/g64/"
    tops = {k[len(pre):]: float(np.max(np.abs(g[k]))) for k in g.files if k.startswith(pre)}
    low = min(tops, key=tops.get)
    print(f"{case}: prefix {prefix} of {len(ref)}, loss {ref[0]:.5g} -> best {ref.min():.5g}; smallest share of the "
          f"largest float64 start gradient {tops[low] / max(tops.values()):.3g} ({low})")
    assert g[f"{case}/pert_errors"].shape[0] == 8
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
        assert prefix == stop  # the case ends after 11 epochs: every one of them is comparable
    else:
        assert prefix >= 24 and ref.min() * 1.2 <= ref[0]
        assert len(ref) == cfg["epochs"] >= 300
    own = m.state_dict()
    assert sorted(own) == sorted(sd0) and all(own[k].shape == sd0[k].shape for k in sd0)
    m.load_state_dict(sd0)
    ps, st = model._rnn_tensors(m)
    assert [n for n, _t in ps] == [k for k, _p in m.named_parameters()] and st == []
    assert all(t is p for (_n, t), (_k, p) in zip(ps, m.named_parameters()))


@pytest.mark.parametrize("case", CASES)
def test_rates_equal_the_recorded_learning_rates(g, case):
    from onset_fingerprinting_amd import model
    cfg, _m, _sd = our_model(g, case)
    rec = g[f"{case}/rates"]
    assert np.array_equal(model.rnn_rates(cfg["lr"], cfg["epochs"])[:len(rec)], rec)


def test_rates_against_the_scheduler():
    from onset_fingerprinting_amd import model
    p = nn.Parameter(torch.zeros(1))
    opt = torch.optim.NAdam([p], lr=0.01, weight_decay=1e-4)
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, 3000)
    opt.step()
    want = []
    for _e in range(3200):
        want.append(float(opt.param_groups[0]["lr"]))
        sched.step()
    r = model.rnn_rates(0.01, 3200)
    assert r.dtype == np.float64 and np.array_equal(r, np.array(want))
    assert r[0] == 0.01 and r[3000] < 1e-12 and r[3100] > r[3000] and np.all(np.diff(r[:3001]) < 0)
    rows = model._rnn_device_rows(0.01, 40)
    table = np.array(model.cnn_rate_table(0.01, 40))
    table[:, 0] = r[:40]
    assert rows.dtype == np.float32 and np.array_equal(rows[:, :3], model.cnn_step_factors(table).astype(np.float32))
    assert model.RNN_WEIGHT_DECAY == 1e-4 and model._rnn_arch(small()).weight_decay == np.float32(1e-4)


# ---- the float64 references against torch autograd ------------------------------------------------------------------
def close(name, got, ref, tol=1e-11, floor=1e-300):
    """max |got - ref| <= tol x max |ref|; `floor` stands in for max |ref| where the exact value is 0."""
    ref = np.asarray(ref, f64)
    err = float(np.max(np.abs(np.asarray(got, f64) - ref))) if ref.size else 0.0
    top = float(np.max(np.abs(ref))) if ref.size else 0.0
    print(f"{name}: max |ref - torch| {err:.3e} of {top:.3e}")
    assert err <= tol * max(top, floor), name


@pytest.mark.parametrize("shape", [(1, 1), (5, 2), (7, 63), (3, 128)], ids=str)
def test_layernorm_reference(shape):
    rows, E = shape
    torch.manual_seed(rows + E)
    ln = nn.LayerNorm(E).double()
    with torch.no_grad():
        ln.weight.uniform_(0.5, 1.5), ln.bias.normal_()
    x = (torch.randn(rows, E, dtype=torch.float64) * 1.5 + 0.3).requires_grad_(True)
    dy = torch.randn(rows, E, dtype=torch.float64)
    y = ln(x)
    (y * dy).sum().backward()
    xn, ga = x.detach().numpy(), ln.weight.detach().numpy()
    yr, mean, rstd = R.layernorm_forward_ref(xn, ga, ln.bias.detach().numpy(), ln.eps)
    close("y", yr, y.detach().numpy())
    dx, dga, dbe = R.layernorm_backward_ref(xn, ga, mean, rstd, dy.numpy())
    top = float(np.abs(dy.numpy()).max())  # at E = 1 dx and dgamma are 0: measured against the gradient that came in
    close("dx", dx, x.grad.numpy(), 1e-10, top)
    close("dgamma", dga, ln.weight.grad.numpy(), 1e-10, top)
    close("dbeta", dbe, ln.bias.grad.numpy(), 1e-10)


def torch_stack(gru, x, dout, masks, dtype=torch.float64):
    """The layers of `gru` run one by one under the masks: -> (last output, per layer (dw_ih, dw_hh, db_ih, db_hh))."""
    L, H = gru.num_layers, gru.hidden_size
    layers = []
    for l in range(L):
        one = nn.GRU(gru.input_size if l == 0 else H, H, batch_first=True).to(dtype)
        with torch.no_grad():
            for k in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"):
                getattr(one, k + "_l0").copy_(getattr(gru, f"{k}_l{l}"))
        layers.append(one)
    h = x.to(dtype)
    for l, one in enumerate(layers):
        h, _ = one(h)
        if masks is not None and l < L - 1:
            h = h * torch.from_numpy(masks[l]).to(dtype)
    (h * dout.to(dtype)).sum().backward()
    return h.detach().numpy(), [tuple(getattr(one, k + "_l0").grad.numpy() for k in
                                      ("weight_ih", "weight_hh", "bias_ih", "bias_hh")) for one in layers]


@pytest.mark.parametrize("shape", [(1, 1, 1, 1, 1), (3, 5, 3, 4, 2), (2, 9, 8, 6, 3)], ids=str)
@pytest.mark.parametrize("p", [0.0, 0.5])
def test_gru_stack_reference(shape, p):
    """Without a mask against torch's own nn.GRU(num_layers=L); with one against its layers run one by one."""
    n, T, Fe, H, L = shape
    torch.manual_seed(sum(shape))
    gru = nn.GRU(Fe, H, L, batch_first=True).double()
    x, dout = torch.randn(n, T, Fe, dtype=torch.float64), torch.randn(n, T, H, dtype=torch.float64)
    masks = R.layer_dropout_mask(11, 3, L - 1, n, T, H, p) if p and L > 1 else None
    params = [tuple(getattr(gru, f"{k}_l{l}").detach().numpy() for k in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"))
              for l in range(L)]
    seqs, gates = R.gru_stack_forward_ref(x.numpy(), params, masks)
    grads = R.gru_stack_backward_ref(x.numpy(), params, seqs, gates, dout.numpy(), masks)
    if masks is None:
        y, _h = gru(x)
        (y * dout).sum().backward()
        close("out", seqs[-1], y.detach().numpy())
        want = [tuple(getattr(gru, f"{k}_l{l}").grad.numpy() for k in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"))
                for l in range(L)]
    else:
        y, want = torch_stack(gru, x, dout, masks)
        close("out", seqs[-1], y)
    for l in range(L):
        for name, got, ref in zip(("dw_ih", "dw_hh", "db_ih", "db_hh"), grads[l], want[l]):
            close(f"layer {l} {name}", got, ref, 1e-9)


def test_site_4_mask_is_the_stream_restated():
    """Element ((l n + s) T + t) H + j of site 4: word idx % 4 of Philox counter (idx // 4, 4, epoch, 0)."""
    from onset_fingerprinting_amd import model
    assert model.SITE_LAYER == R.SITE_LAYER == 4
    seed, epoch, layers, n, T, H, p = 0x1234567890ABCDEF, 7, 2, 3, 5, 4, 0.5
    m = R.layer_dropout_mask(seed, epoch, layers, n, T, H, p)
    assert m.shape == (layers, n, T, H) and m.dtype == np.float32 and set(np.unique(m)) == {0.0, 2.0}
    flat = m.reshape(-1)
    for idx in (0, 1, 5, 17, 119):
        c = np.array([[idx // 4, 4, epoch, 0]], np.uint32)
        word = RR.philox4x32(c, RR.key_of(seed))[0, idx % 4]
        assert flat[idx] == (0.0 if word < RR.threshold(p) else 2.0)
    assert flat[((1 * n + 2) * T + 3) * H + 1] == m[1, 2, 3, 1]
    assert not np.array_equal(m, RR.dropout_mask(seed, epoch, layers * n, T * H, p).reshape(m.shape))  # site 0 differs
    assert not np.array_equal(m, R.layer_dropout_mask(seed, epoch + 1, layers, n, T, H, p))
    assert 0.3 < float((R.layer_dropout_mask(1, 0, 1, 8, 16, 8, 0.5) == 0).mean()) < 0.7
    assert set(np.unique(R.layer_dropout_mask(1, 0, 1, 8, 16, 8, 0.25))) == {0.0, float(np.float32(1 / 0.75))}


def test_nadam_decay_reference():
    """Two steps of torch.optim.NAdam(weight_decay=1e-4) in float64 against the restatement; the second starts from
    moments that are not zero, so the size of the decayed gradient matters and not only its sign."""
    from onset_fingerprinting_amd import model
    rng = np.random.default_rng(3)
    p0, grads = rng.standard_normal(50) * 1e3, rng.standard_normal((2, 50))
    p = nn.Parameter(torch.tensor(p0))
    opt = torch.optim.NAdam([p], lr=0.01, weight_decay=1e-4)
    table = np.array(model.cnn_rate_table(0.01, 2))
    table[:, 0] = 0.01  # no scheduler here
    fac = model.cnn_step_factors(table)
    with_decay, without = (p0, np.zeros(50), np.zeros(50)), (p0, np.zeros(50), np.zeros(50))
    for step in range(2):
        before = p.detach().numpy().copy()
        p.grad = torch.tensor(grads[step])
        opt.step()
        with_decay = R.nadam_decay_step_ref(with_decay[0], grads[step], with_decay[1], with_decay[2], fac[step], 1e-4)
        without = R.nadam_decay_step_ref(without[0], grads[step], without[1], without[2], fac[step], 0.0)
        # torch keeps mu_product in float32 unless the default dtype is float64: the factors carry that rounding
        close(f"update of step {step}", with_decay[3], p.detach().numpy() - before, 1e-6)
    top = float(np.max(np.abs(with_decay[3])))
    gap = float(np.max(np.abs(without[3] - with_decay[3])))
    print(f"second update up to {top:.3e}; without the decay term it differs by up to {gap:.3e}")
    assert gap > 1e-2 * top


# ---- the envelope ---------------------------------------------------------------------------------------------------
def small(**kw):
    from onset_fingerprinting_amd import model
    return model.RNN(32, 2, **{"channels": 3, "hidden_size": 8, "dropout_rate": 0.0, **kw})


def test_every_refusal_comes_before_the_gpu(no_gpu_calls):
    from onset_fingerprinting_amd import model
    x, y = torch.zeros(5, 3, 32), torch.zeros(5, 2)
    nobias_fc = small()
    nobias_fc.fc = nn.Linear(8, 2, bias=False)
    rates = small(num_layers=2)
    rates.attention.dropout = 0.25
    for what, m, match in (("an LSTM", small(rnn_type="LSTM"), "LSTM"), ("a plain RNN", small(rnn_type="RNN"), "RNN"),
                           ("bidirectional", small(bidirectional=True), "bidirectional"),
                           ("shared input weights", small(share_input_weights=True), "share_input_weights"),
                           ("batch_first=False", small(batch_first=False), "batch_first=False"),
                           ("bias=False", small(bias=False), "bias=False"),
                           ("five layers", small(num_layers=5), "num_layers 5"),
                           ("nine channels", small(channels=9), "9 channels"),
                           ("nine heads", small(hidden_size=18, num_heads=9), "num_heads 9"),
                           ("dropout without seed", small(dropout_rate=0.5), "seed="),
                           ("dropout of one layer without seed", small(dropout_rate=0.5, num_layers=1), "seed="),
                           ("a loss", small(loss=F.smooth_l1_loss), "loss"),
                           ("fc without bias", nobias_fc, "bias"),
                           ("a wrong class", nn.Linear(2, 2), "not an RNN")):
        for call in (model.fit_rnn, model.rnn_loss_and_grads_device):
            with pytest.raises(ValueError, match=match):
                call(m, torch.zeros(5, 9, 32) if what == "nine channels" else x, y)
            print(f"{what}: refused by {call.__name__}")
    for call in (model.fit_rnn, model.rnn_loss_and_grads_device):
        with pytest.raises(ValueError, match="differs"):
            call(rates, x, y, seed=1)
        with pytest.raises(ValueError, match="dropout_rate 1"):
            call(small(dropout_rate=1.0), x, y, seed=1)
        with pytest.raises(ValueError, match="1..1024"):
            call(small(), torch.zeros(1025, 3, 32), torch.zeros(1025, 2))
        with pytest.raises(ValueError, match="input_size 513"):
            call(small(), torch.zeros(2, 3, 513), torch.zeros(2, 2))
        with pytest.raises(ValueError, match="do not fit"):
            call(small(), torch.zeros(5, 4, 32), y)
        with pytest.raises(ValueError, match="do not fit"):
            call(small(), x, torch.zeros(5, 17))
        with pytest.raises(ValueError, match="do not fit"):  # permute_input=False reads [n, input_size, channels]
            call(small(permute_input=False), x, y)
    with pytest.raises(ValueError, match="outputs"):
        model.fit_rnn(model.RNN(32, 17, hidden_size=8, dropout_rate=0.0), x, torch.zeros(5, 17))
    with pytest.raises(ValueError, match="patience"):
        model.fit_rnn(small(), x, y, patience=3)
    with pytest.raises(ValueError, match="hidden_size 130"):  # inference runs it, the trainer does not
        model.fit_rnn(small(hidden_size=130), x, y)
    with pytest.raises(ValueError, match="num_heads 3"):
        wrong = small()
        wrong.attention = nn.MultiheadAttention(9, 3, batch_first=True)
        model.fit_rnn(wrong, x, y)
    # the random stream's 32-bit index: inside the other limits the largest counts are 2^31 and 3 x 2^26, so the
    # guard is reached through its own function alone
    model._rnn_check_stream(1024, 8, 512, 4, 128)
    with pytest.raises(ValueError, match="attention probabilities"):
        model._rnn_check_stream(2048, 8, 512, 2, 8)
    with pytest.raises(ValueError, match="between the layers"):
        model._rnn_check_stream(1024, 1, 512, 4, 4096)
    with pytest.raises(ValueError, match="seed"):
        model.fit_rnn(small(), x, y, seed=-1)


def test_window_sources_are_checked_before_the_gpu(no_gpu_calls):
    from onset_fingerprinting_amd import data, model
    src = object.__new__(data.ShiftedWindows)  # _batch_of refuses by type, before it reads anything of the source
    with pytest.raises(ValueError, match="x_val"):
        model.fit_rnn(small(), torch.zeros(5, 3, 32), torch.zeros(5, 2), x_val=src, y_val=torch.zeros(4, 2))
    src.n_onsets, src.n_extractions, src.n, src.channels, src.frame_length = 4, 2, 8, 3, 32
    with pytest.raises(ValueError, match="permute_input=True"):
        model.fit_rnn(small(permute_input=False), src, torch.zeros(4, 2))


def test_stand_alone_wrappers_refuse_before_the_gpu(no_gpu_calls):
    from onset_fingerprinting_amd import model
    with pytest.raises(ValueError, match="GPU tensor"):
        model.layernorm_train_forward(torch.zeros(2, 3), torch.zeros(3), torch.zeros(3))
    with pytest.raises(ValueError, match="GPU tensor"):
        model.rnn_gru_train_forward(torch.zeros(2, 3, 4), [])
    with pytest.raises(ValueError, match="GPU tensor"):
        model.rnn_attention_train_forward(torch.zeros(2, 2, 4), torch.zeros(12, 4), torch.zeros(12), 2)
    with pytest.raises(ValueError, match="2\\^32"):
        model.rnn_layer_dropout_mask_device(1, 0, 4, 1024, 512, 4096, 0.5)
    with pytest.raises(ValueError, match="0 <= p < 1"):
        model.rnn_layer_dropout_mask_device(1, 0, 1, 2, 3, 4, 1.0)
    with pytest.raises(ValueError, match="negative"):
        model.nadam_step(None, None, None, None, None, weight_decay=-1.0)
