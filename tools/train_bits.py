#!/usr/bin/env python3
"""The bits of a short fit by each of the four GPU trainers (fit_cnn, fit_lcccnn, fit_cnnrnn, fit_rnn), for comparing
two builds of the package: a refactor of the trainers' host side must leave every one of them unchanged.

    python tools/train_bits.py [--package-root DIR] [--only cnn cccnn cnnrnn rnn] [--out FILE]

Each trainer fits 5 epochs with seed 3 on the smallest shapes that still go through every shared part: CNN and CNNRNN
with 2 conv layers, BatchNorm and pool; RNN with 2 GRU layers (dropout between them); LCCCNN with one conv layer;
hidden size 8, 2 heads; windows of 16 samples (12 for the RNN) and 3 channels from a data.ShiftedWindows source of 5
onsets with max_shift 2, a validation set of 7 (more than the batch), dropout_rate 0.5, once with the L1 and once with
the MSE loss.  Printed per fit, as one JSON object: the int32 view of train_loss and val_loss and the SHA-256 of the
final parameters' and running statistics' bytes (state_dict order).  `--package-root` imports the package from another
built tree.  Same build, same output; a committed copy would not survive the next compiler."""
import argparse
import hashlib
import json
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
EPOCHS, SEED, N, N_VAL, CHANNELS = 5, 3, 5, 7, 3


def fits(model):
    kw = dict(dropout_rate=0.5)
    conv = dict(layer_sizes=[4, 6], kernel_size=3, batch_norm=True, pool=True, **kw)
    return {
        "cnn": (16, lambda loss: model.CNN(16, 2, CHANNELS, loss=loss, **conv), model.fit_cnn),
        "cccnn": (16, lambda loss: model.LCCCNN(16, 2, CHANNELS, layer_sizes=[2], kernel_sizes=3, loss=loss, **kw),
                  model.fit_lcccnn),
        "cnnrnn": (16, lambda loss: model.CNNRNN(16, 2, CHANNELS, n_hidden=8, loss=loss, **conv), model.fit_cnnrnn),
        "rnn": (12, lambda loss: model.RNN(12, 2, CHANNELS, hidden_size=8, num_layers=2, num_heads=2, loss=loss, **kw),
                model.fit_rnn),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--package-root", default=str(REPO))
    ap.add_argument("--only", nargs="*", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, str(Path(args.package_root).resolve()))
    import numpy as np
    import torch
    import torch.nn.functional as F

    from onset_fingerprinting_amd import data, model

    out = {}
    for name, (width, make, fit) in fits(model).items():
        if args.only and name not in args.only:
            continue
        for loss in (F.l1_loss, F.mse_loss):
            torch.manual_seed(0)
            m = make(loss)
            rng = np.random.default_rng(1)
            audio = rng.standard_normal((400, CHANNELS)).astype(np.float32)
            src = data.ShiftedWindows(audio, 20 + 60 * np.arange(N), width, max_shift=2)
            y = torch.from_numpy(rng.random((N, 2), dtype=np.float32) - 0.5)
            x_val = torch.from_numpy(rng.standard_normal((N_VAL, CHANNELS, width)).astype(np.float32))
            y_val = torch.from_numpy(rng.random((N_VAL, 2), dtype=np.float32) - 0.5)
            r = fit(m, src, y, x_val=x_val, y_val=y_val, max_epochs=EPOCHS, seed=SEED)
            assert r.epochs == EPOCHS
            h = hashlib.sha256()
            for t in m.state_dict().values():
                h.update(t.detach().cpu().contiguous().numpy().tobytes())
            out[f"{name}/{loss.__name__}"] = dict(
                train_loss=r.train_loss.cpu().numpy().view(np.int32).tolist(),
                val_loss=r.val_loss.cpu().numpy().view(np.int32).tolist(), state_sha256=h.hexdigest())
    text = json.dumps(out, indent=1) + "\n"
    print(text, end="")
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text)


if __name__ == "__main__":
    main()
