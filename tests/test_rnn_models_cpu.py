"""CPU-only checks of model.RNN / model.CNNRNN: the reference's state_dicts of the g21 golden set load strictly,
and options without a HIP implementation are refused at construction."""
import json

import pytest
import torch

from tests.conftest import load_golden


def g21_cases():
    g = load_golden("g21_rnn_models")
    return g, sorted({k.split("/", 1)[0] for k in g.files})


def build(cfg):
    from onset_fingerprinting_amd import model
    kw = dict(cfg)
    cls = getattr(model, kw.pop("class"))
    if "activation" in kw:
        kw["activation"] = getattr(torch.nn, kw["activation"])
    return cls(**kw)


def state_dict(g, name):
    keys = [k for k in g.files if k.startswith(name + "/") and k.split("/", 1)[1] not in ("cfg", "x", "y", "rnn_in")
            and not k.split("/", 1)[1].startswith("seq_l")]
    return {k.split("/", 1)[1]: torch.from_numpy(g[k]) for k in keys}


def test_golden_set_covers_the_issue_cases():
    g, names = g21_cases()
    assert len(names) == 10
    classes = {json.loads(str(g[f"{n}/cfg"]))["class"] for n in names}
    assert classes == {"RNN", "CNNRNN"}
    cells = {json.loads(str(g[f"{n}/cfg"])).get("rnn_type", "GRU") for n in names if f"{n}/seq_l0" in g.files}
    assert cells == {"GRU", "LSTM", "RNN"}


def test_every_reference_state_dict_loads_strictly():
    g, names = g21_cases()
    for name in names:
        m = build(json.loads(str(g[f"{name}/cfg"])))
        sd = state_dict(g, name)
        m.load_state_dict(sd, strict=True)
        assert set(m.state_dict()) == set(sd), name


def test_unsupported_options_raise():
    from onset_fingerprinting_amd import model
    with pytest.raises(ValueError):
        model.CNNRNN(64, 2, activation=torch.nn.GELU)
    with pytest.raises(ValueError):
        model.RNN(256, 2, rnn_type="QRNN")
    with pytest.raises(ValueError):
        model.RNN(256, 2, hidden_size=512)
    with pytest.raises(ValueError):
        model.RNN(256, 2, hidden_size=16, num_heads=3)  # 16 is not divisible by 3 heads
    with pytest.raises(ValueError):
        model.RNN(256, 2, hidden_size=256, bidirectional=True, num_heads=2)  # head dim 256
    with pytest.raises(ValueError):
        model.CNNRNN(64, 2, n_hidden=300)
    with pytest.raises(ValueError):
        model.rnn_forward(torch.nn.LSTM(3, 16, proj_size=8), torch.zeros(2, 5, 3))
    with pytest.raises(ValueError):
        model.rnn_forward(torch.nn.GRU(3, 300), torch.zeros(2, 5, 3))


def test_rnn_forward_is_public():
    from onset_fingerprinting_amd import model
    assert callable(model.rnn_forward)
    assert model.RNN(256, 2).rnn.input_size == 3 and model.RNN(256, 2, share_input_weights=True).rnn.input_size == 2
