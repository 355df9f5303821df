"""GPU parity of the recurrent classifiers (model.RNN, model.CNNRNN, rnn_forward; csrc/ofp_rnn.hip) against the
reference's golden outputs (g21) and torch's own CPU modules; tolerance 1e-4 relative to the largest magnitude."""
import json

import numpy as np
import pytest
import torch

from tests.conftest import load_golden

pytestmark = pytest.mark.gpu


def rel_err(a, b):
    return np.abs(np.asarray(a, np.float64) - b).max() / max(np.abs(b).max(), 1e-12)


def build(cfg):
    from onset_fingerprinting_amd import model
    kw = dict(cfg)
    cls = getattr(model, kw.pop("class"))
    if "activation" in kw:
        kw["activation"] = getattr(torch.nn, kw["activation"])
    return cls(**kw)


def golden_model(g, name):
    m = build(json.loads(str(g[f"{name}/cfg"])))
    skip = ("cfg", "x", "y", "rnn_in")
    sd = {k.split("/", 1)[1]: torch.from_numpy(g[k]) for k in g.files
          if k.startswith(name + "/") and k.split("/", 1)[1] not in skip and "/seq_l" not in k}
    m.load_state_dict(sd, strict=True)
    return m.eval()


def torch_forward(m, x):
    """The reference's forward (model.py:231-253, 404-413) on m's own torch modules, CPU, eval."""
    from onset_fingerprinting_amd import model
    m = m.eval()
    with torch.no_grad():
        if isinstance(m, model.RNN):
            if m.permute_input:
                x = x.permute(0, 2, 1)
            if not m.share_input_weights:
                out = m.rnn(x)[0]
            else:
                out = torch.cat([m.rnn(x[..., i:i + 2])[0] for i in range(m.channels - 1)], -1)
            out = m.layer_norm(out)
        else:
            out = m.rnn(m.conv_layers(x))[0]
        out = m.attention(out, out, out, need_weights=False)[0]
        return m.fc(out.mean(1))


G21 = sorted({k.split("/", 1)[0] for k in load_golden("g21_rnn_models").files})


@pytest.mark.parametrize("name", G21)
def test_g21_model_matches_reference(name):
    g = load_golden("g21_rnn_models")
    m = golden_model(g, name)
    y = m(torch.from_numpy(g[f"{name}/x"]))  # CPU in, CPU out
    assert not y.is_cuda and y.shape == g[f"{name}/y"].shape
    assert rel_err(y.numpy(), g[f"{name}/y"]) < 1e-4, name
    yd = m(torch.from_numpy(g[f"{name}/x"]).cuda())
    assert yd.is_cuda and torch.equal(yd.cpu(), y)


@pytest.mark.parametrize("name", [n for n in G21 if f"{n}/seq_l0" in load_golden("g21_rnn_models").files])
def test_g21_layer_sequences_match_reference(name):
    from onset_fingerprinting_amd.model import rnn_forward
    g = load_golden("g21_rnn_models")
    r = golden_model(g, name).rnn
    x = torch.from_numpy(g[f"{name}/rnn_in"])
    for k in range(r.num_layers):
        sub = type(r)(r.input_size, r.hidden_size, k + 1, bias=r.bias, batch_first=True, bidirectional=r.bidirectional)
        sub.load_state_dict({n: v for n, v in r.state_dict().items() if int(n.split("_l")[1][0]) <= k})
        want = g[f"{name}/seq_l{k}"]
        got = rnn_forward(sub, x).numpy()
        assert got.shape == want.shape
        assert rel_err(got, want) < 1e-4, (name, k)


# (module type, kwargs, batch, T, input features)
RNN_CASES = [
    ("GRU", dict(hidden_size=16), 1, 1, 3),
    ("GRU", dict(hidden_size=64, num_layers=2), 15, 256, 3),
    ("GRU", dict(hidden_size=64, num_layers=2), 4096, 64, 3),
    ("GRU", dict(hidden_size=128), 2, 1000, 2),  # W_hh streamed from L2
    ("GRU", dict(hidden_size=16, bidirectional=True), 17, 2, 40),  # wide input: projection by ofp_dense
    ("GRU", dict(hidden_size=20, num_layers=2, bidirectional=True), 17, 16, 5),  # partial hidden tile
    ("LSTM", dict(hidden_size=128, num_layers=2, bidirectional=True), 17, 16, 3),  # streamed, 2 tiles per wave
    ("LSTM", dict(hidden_size=64), 4096, 16, 4),
    ("LSTM", dict(hidden_size=16, num_layers=2, bias=False), 15, 1000, 8),
    ("RNN", dict(hidden_size=64, nonlinearity="tanh"), 4096, 16, 3),
    ("RNN", dict(hidden_size=16, nonlinearity="relu", num_layers=2), 17, 1000, 2),
    ("RNN", dict(hidden_size=30, nonlinearity="tanh", bidirectional=True), 1, 256, 4),
    ("LSTM", dict(hidden_size=200), 5, 16, 3),  # 4 tiles per wave, streamed
]


@pytest.mark.parametrize("kind,kw,B,T,F", RNN_CASES)
def test_rnn_forward_matches_torch(kind, kw, B, T, F):
    from onset_fingerprinting_amd.model import rnn_forward
    torch.manual_seed(B * 7 + T + F)
    r = getattr(torch.nn, kind)(F, batch_first=True, **kw).eval()
    x = torch.randn(B, T, F)
    with torch.no_grad():
        want = r(x)[0].numpy()
    got = rnn_forward(r, x.cuda()).cpu().numpy()
    assert got.shape == want.shape
    assert rel_err(got, want) < 1e-4


def test_rnn_forward_saturated_gates():
    from onset_fingerprinting_amd.model import rnn_forward
    torch.manual_seed(3)
    for kind in ("GRU", "LSTM"):
        r = getattr(torch.nn, kind)(3, 64, 2, batch_first=True).eval()
        with torch.no_grad():
            for p in r.parameters():
                p.mul_(3.0)
        x = torch.randn(15, 256, 3) * 3
        with torch.no_grad():
            want = r(x)[0].numpy()
        assert rel_err(rnn_forward(r, x).numpy(), want) < 1e-4, kind


def test_rnn_forward_time_major_and_non_contiguous():
    from onset_fingerprinting_amd.model import rnn_forward
    torch.manual_seed(4)
    r = torch.nn.GRU(3, 32, 2, bidirectional=True).eval()  # batch_first=False: [T, batch, features]
    big = torch.randn(40, 9, 7).cuda()
    x = big[::2, 1:8, 1:4]  # non-contiguous in every axis
    assert not x.is_contiguous()
    with torch.no_grad():
        want = r(x.cpu())[0].numpy()
    assert rel_err(rnn_forward(r, x).cpu().numpy(), want) < 1e-4
    r2 = torch.nn.LSTM(12, 16, batch_first=True).eval()
    xw = torch.randn(6, 30, 24).cuda()[:, :, ::2]  # wide, strided features
    with torch.no_grad():
        want = r2(xw.cpu())[0].numpy()
    assert rel_err(rnn_forward(r2, xw).cpu().numpy(), want) < 1e-4


def test_full_models_at_long_sequences_and_options():
    from onset_fingerprinting_amd import model
    torch.manual_seed(5)
    cases = [
        (model.RNN(1024, 2, 3, 16, 2), (3, 3, 1024)),  # T = 1024: 64 key tiles in the attention
        (model.RNN(1000, 2, 4, 32, 2, rnn_type="LSTM", bidirectional=True, share_input_weights=True), (2, 4, 1000)),
        (model.RNN(64, 2, 3, 16, 2, batch_first=False), (5, 3, 64)),  # recurs along the batch axis, as the reference
        (model.CNNRNN(256, 2, 3, n_hidden=64), (3, 3, 256)),
    ]
    for m, shape in cases:
        m.eval()
        x = torch.randn(*shape)
        want = torch_forward(m, x).numpy()
        assert rel_err(m(x).numpy(), want) < 1e-4, type(m).__name__


def test_sequence_alone_is_bit_identical_to_inside_a_large_batch():
    from onset_fingerprinting_amd import model
    g = load_golden("g21_rnn_models")
    for name in ("gru64", "lstm_bi", "cnnrnn"):
        m = golden_model(g, name)
        x = torch.from_numpy(g[f"{name}/x"])[:1].cuda()
        batch = torch.randn((4099,) + tuple(x.shape[1:]), device="cuda")
        batch[2050] = x[0]
        alone, inside = m(x), m(batch)
        assert torch.equal(alone[0], inside[2050]), name
    r = torch.nn.GRU(3, 64, 2, batch_first=True).eval()
    xb = torch.randn(4099, 64, 3, device="cuda")
    full = model.rnn_forward(r, xb)
    one = model.rnn_forward(r, xb[4097:4098].clone())
    assert torch.equal(full[4097], one[0])


def test_invalid_calls_raise_and_leave_the_device_usable():
    from onset_fingerprinting_amd import _lib, model
    L = _lib.lib()
    torch.cuda.synchronize()
    y = torch.zeros(4, 8, 16, device="cuda")
    w = torch.zeros(48, 16, device="cuda")
    s = model._stream(y.device)
    # T = 0
    rc = L.ofp_rnn_layer(2, 4, 0, 3, 16, 0, y.data_ptr(), 24, 3, 1, None, 0, 0, w.data_ptr(), None, w.data_ptr(), None,
                         y.data_ptr(), 128, 16, 0, s)
    assert rc == 1 and "T" in _lib.last_error()
    # hidden size beyond the kernel
    rc = L.ofp_rnn_layer(2, 4, 8, 3, 300, 0, y.data_ptr(), 24, 3, 1, None, 0, 0, w.data_ptr(), None, w.data_ptr(),
                         None, y.data_ptr(), 128, 16, 0, s)
    assert rc == 1 and "hidden" in _lib.last_error()
    # wide input without a precomputed projection
    rc = L.ofp_rnn_layer(2, 4, 8, 40, 16, 0, y.data_ptr(), 24, 3, 1, None, 0, 0, w.data_ptr(), None, w.data_ptr(),
                         None, y.data_ptr(), 128, 16, 0, s)
    assert rc == 1
    # E not divisible by the heads
    with pytest.raises(_lib.OnsetFPError, match="divisible"):
        _lib.check(L.ofp_attention_mean(y.data_ptr(), 4, 8, 10, 3, y.data_ptr(), s), "ofp_attention_mean")
    with pytest.raises(_lib.OnsetFPError):
        _lib.check(L.ofp_attention_mean(y.data_ptr(), 4, 0, 16, 2, y.data_ptr(), s), "ofp_attention_mean")
    torch.cuda.synchronize()
    assert torch.count_nonzero(y).item() == 0  # nothing was launched
    r = torch.nn.GRU(3, 16, batch_first=True).eval()
    x = torch.randn(2, 8, 3)
    with torch.no_grad():
        want = r(x)[0].numpy()
    assert rel_err(model.rnn_forward(r, x).numpy(), want) < 1e-4
