#!/usr/bin/env python3
"""Forward latency of model.RNN / model.CNNRNN (HIP kernels, csrc/ofp_rnn.hip) beside torch-ROCm's own modules
(MIOpen RNNs, torch attention) on the same GPU, for the notebook anchors at B = 1 and B = 4096.

    python tools/rnn_latency.py [--out results/rnn_latency.jsonl]

Every configuration runs in a fresh child process under its own `timeout -k 10 <s>`; the driver stops at the
first child that fails, times out or dies on a signal.  Times are HIP events around `iters` forwards after
`warmup` forwards (device-resident input, so no host copy is in the window); one JSON line per config.
"""
import argparse
import json
import subprocess
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]

CONFIGS = {
    "rnn_gru16": ("RNN", dict(input_size=256, output_size=2, channels=3, hidden_size=16, num_layers=2)),
    "rnn_gru64": ("RNN", dict(input_size=256, output_size=2, channels=3, hidden_size=64, num_layers=2)),
    "rnn_gru64_share": ("RNN", dict(input_size=256, output_size=2, channels=3, hidden_size=64, num_layers=2,
                                    share_input_weights=True)),
    "cnnrnn": ("CNNRNN", dict(input_size=256, output_size=2, channels=3)),
}


def child(name, batch, warmup, iters):
    import torch

    sys.path.insert(0, str(REPO))
    from onset_fingerprinting_amd import model

    cls, kw = CONFIGS[name]
    torch.manual_seed(0)
    m = getattr(model, cls)(**kw).eval().cuda()  # parameters resident, as a deployed model keeps them
    x = torch.randn(batch, kw["channels"], kw["input_size"], device="cuda")
    ref = type(m)(**kw).eval()
    ref.load_state_dict(m.state_dict())
    ref = ref.cuda()
    from tests.test_gpu_rnn import torch_forward  # the reference's forward on m's own torch modules

    def timed(fn):
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1000.0 / iters  # us per forward

    with torch.no_grad():
        hip_us = timed(lambda: m(x))
        torch_us = timed(lambda: torch_forward(ref, x))
        diff = (m(x) - torch_forward(ref, x)).abs().max().item()
    print(json.dumps(dict(config=name, batch=batch, hip_us=round(hip_us, 1), torch_rocm_us=round(torch_us, 1),
                          max_abs_diff=diff, iters=iters)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", nargs=2, metavar=("CONFIG", "BATCH"))
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--timeout", type=int, default=300, help="seconds per configuration")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.child:
        child(args.child[0], int(args.child[1]), args.warmup, args.iters)
        return
    lines = []
    for name in CONFIGS:
        for batch in (1, 4096):
            cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, __file__, "--child", name, str(batch),
                   "--warmup", str(args.warmup), "--iters", str(args.iters)]
            p = subprocess.run(cmd, capture_output=True, text=True)
            if p.returncode != 0:
                sys.stderr.write(p.stdout + p.stderr)
                print(f"{name} B={batch}: exit status {p.returncode}; stopping", file=sys.stderr)
                break
            line = p.stdout.strip().splitlines()[-1]
            print(line, flush=True)
            lines.append(line)
        else:
            continue
        break
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")
    if len(lines) != 2 * len(CONFIGS):
        sys.exit(1)


if __name__ == "__main__":
    main()
