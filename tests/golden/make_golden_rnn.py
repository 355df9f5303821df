#!/usr/bin/env python3
"""Golden vectors g21_rnn_models: the reference's own model.RNN / model.CNNRNN (model.py:168-440), eval mode.

Run in the build container only:   python tests/golden/make_golden_rnn.py
Per case <name>: cfg (JSON constructor arguments; an activation by its torch.nn class name), every state_dict
entry (<name>/<key>), x, y = model(x); for one case per cell type also the output sequence of every recurrent
layer (<name>/seq_l{k} = the first k+1 layers of model.rnn run on <name>/rnn_in, the first 96 steps of the first
sequence of the model's recurrent input; kept short so that the file stays small).
Biases, LayerNorm / BatchNorm affines and BatchNorm statistics are randomised so that every term is exercised.
"""
import json
import sys
import warnings
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
REPO = HERE.parents[1]
sys.path.insert(0, str(HERE))
sys.path.insert(0, str(REPO))

from _refload import load_reference  # noqa: E402

warnings.filterwarnings("ignore")

# name -> (class, constructor arguments, batch, per-layer sequences stored)
CASES = {
    "gru16": ("RNN", dict(input_size=256, output_size=2, channels=3, hidden_size=16, num_layers=2), 3, True),
    "gru64": ("RNN", dict(input_size=256, output_size=2, channels=3, hidden_size=64, num_layers=2), 3, False),
    "share": ("RNN", dict(input_size=256, output_size=2, channels=3, hidden_size=16, num_layers=2,
                          share_input_weights=True), 4, False),
    "lstm_bi": ("RNN", dict(input_size=256, output_size=2, channels=3, hidden_size=16, num_layers=2, rnn_type="LSTM",
                            bidirectional=True), 2, True),
    "rnn_tanh": ("RNN", dict(input_size=320, output_size=2, channels=4, hidden_size=32, num_layers=1,
                             rnn_type="RNN"), 2, True),
    "nobias": ("RNN", dict(input_size=256, output_size=2, channels=3, hidden_size=16, num_layers=2, bias=False), 4, False),
    "heads4": ("RNN", dict(input_size=256, output_size=3, channels=3, hidden_size=32, num_layers=2, num_heads=4), 3,
               False),
    "noperm": ("RNN", dict(input_size=256, output_size=2, channels=3, hidden_size=16, num_layers=2,
                           permute_input=False), 4, False),
    "cnnrnn": ("CNNRNN", dict(input_size=64, output_size=2, channels=3), 4, False),
    "cnnrnn_bn_pool": ("CNNRNN", dict(input_size=128, output_size=2, channels=3, batch_norm=True, pool=True,
                                      n_rnn_layers=2, n_hidden=32, activation="ReLU"), 4, False),
}


def main():
    import torch
    torch.set_num_threads(1)
    ref = load_reference()
    torch.manual_seed(21)
    out = {}
    for name, (cls, kw, batch, per_layer) in CASES.items():
        args = dict(kw)
        if "activation" in args:
            args["activation"] = getattr(torch.nn, args["activation"])
        m = getattr(ref.model, cls)(**args)
        with torch.no_grad():
            for mod in m.modules():
                if isinstance(mod, torch.nn.BatchNorm1d):
                    mod.running_mean.normal_(0, 0.3)
                    mod.running_var.uniform_(0.5, 2.0)
                if isinstance(mod, (torch.nn.BatchNorm1d, torch.nn.LayerNorm)):
                    mod.weight.uniform_(0.5, 1.5)
                    mod.bias.normal_(0, 0.2)
            for pname, p in m.named_parameters():
                if "bias" in pname and not pname.startswith(("rnn.", "conv_layers")):
                    p.normal_(0, 0.1)  # in_proj / out_proj / fc start at zero
        m.eval()
        C, W = kw["channels"], kw["input_size"]
        shape = (batch, W, C) if kw.get("permute_input", True) is False else (batch, C, W)
        x = torch.randn(*shape)
        with torch.no_grad():
            y = m(x)
        out[f"{name}/cfg"] = np.array(json.dumps({"class": cls, **kw}))
        for k, v in m.state_dict().items():
            out[f"{name}/{k}"] = v.numpy()
        out[f"{name}/x"], out[f"{name}/y"] = x.numpy(), y.numpy()
        if per_layer:  # RNN cases: the first sequence of the recurrent input (the permuted x), first 96 steps
            r = m.rnn
            rin = (x.permute(0, 2, 1) if kw.get("permute_input", True) else x)[:1, :96]
            out[f"{name}/rnn_in"] = rin.contiguous().numpy()
            for k in range(r.num_layers):
                sub = type(r)(r.input_size, r.hidden_size, k + 1, bias=r.bias, batch_first=True,
                              bidirectional=r.bidirectional)
                sub.load_state_dict({n: v for n, v in r.state_dict().items() if int(n.split("_l")[1][0]) <= k})
                with torch.no_grad():
                    out[f"{name}/seq_l{k}"] = sub(rin)[0].numpy()
    path = HERE / "g21_rnn_models.npz"
    np.savez_compressed(path, **out)
    print(f"g21_rnn_models: {path.stat().st_size / 1024:.1f} KiB, {len(CASES)} cases")


if __name__ == "__main__":
    main()
