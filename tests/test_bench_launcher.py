"""CPU-only: `bench.py --gpus N` is its own launcher.  The rehearsal
mode runs the launcher, the rendezvous, the clip sharding, the one-collective exchange, the max-over-ranks
timing and the JSON line over gloo with fabricated onset records -- no GPU work, and the line says so."""
import json
import os
import socket
import subprocess
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
BENCH = str(REPO / "bench.py")


def _run(cmd, env=None, timeout=240):
    e = dict(os.environ)
    e.pop("RANK", None), e.pop("WORLD_SIZE", None), e.pop("LOCAL_RANK", None)
    e.update(env or {})
    return subprocess.run(cmd, env=e, capture_output=True, text=True, timeout=timeout, cwd=str(REPO))


def _json_line(stdout):
    lines = [l for l in stdout.splitlines() if l.strip()]
    assert len(lines) == 1, lines  # ONE line on stdout
    return json.loads(lines[0])


def test_gpus_2_launches_two_ranks_and_prints_one_line():
    r = _run([sys.executable, BENCH, "--gpus", "2", "--steps", "3", "--warmup", "1", "--rehearsal"])
    assert r.returncode == 0, r.stderr[-2000:]
    j = _json_line(r.stdout)
    assert j["n_gpus"] == 2 and j["steps"] == 3 and j["warmup"] == 1
    assert j["scaling"] == "strong" and j["config"]["workload"] == "c4"
    c = j["config"]
    assert c["ranks_in_exchange"] == 2 and c["clips_per_rank"] == 256 and c["clips_total"] == 512
    assert c["clips_seen"] == 512 and c["onsets_gathered"] == 3 * 512  # every clip of both shards arrived
    assert "rehearsal" in j["data"] and j["value"] == 0.0            # not presented as a measurement


def test_three_ranks_shard_512_clips_unevenly():
    r = _run([sys.executable, BENCH, "--gpus", "3", "--steps", "2", "--warmup", "1", "--rehearsal"])
    assert r.returncode == 0, r.stderr[-2000:]
    c = _json_line(r.stdout)["config"]
    assert c["ranks_in_exchange"] == 3 and c["clips_seen"] == 512 and c["clips_per_rank"] == 171


def test_under_torch_distributed_run_the_ranks_are_used_as_they_are():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    r = _run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
              "127.0.0.1", "--master-port", str(port), BENCH, "--gpus", "2", "--steps", "2", "--warmup", "1",
              "--rehearsal", "--workload", "c2", "--clips", "3"])
    assert r.returncode == 0, r.stderr[-2000:]
    j = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert j["n_gpus"] == 2 and j["scaling"] == "weak" and j["config"]["clips_seen"] == 6


def test_gpus_must_equal_world_size():
    r = _run([sys.executable, BENCH, "--gpus", "1", "--rehearsal"], env={"RANK": "0", "WORLD_SIZE": "2", "LOCAL_RANK": "0"})
    assert r.returncode == 2 and "WORLD_SIZE is 2" in r.stderr and r.stdout.strip() == ""


def test_a_failed_rank_fails_the_launcher():
    r = _run([sys.executable, BENCH, "--gpus", "2", "--steps", "2", "--warmup", "1", "--rehearsal"],
             env={"OFP_BENCH_TEST_FAIL_RANK": "1"})
    assert r.returncode != 0 and r.stdout.strip() == "" and "ranks failed" in r.stderr


def test_dump_outputs_writes_the_last_steps_exchanged_records(tmp_path):
    """--dump-outputs in a rehearsal: rank 0 writes the records the last step's exchange delivered (every rank's)."""
    import numpy as np
    d = tmp_path / "dump"
    r = _run([sys.executable, BENCH, "--gpus", "2", "--steps", "2", "--warmup", "1", "--rehearsal", "--dump-outputs", str(d)])
    assert r.returncode == 0, r.stderr[-2000:]
    assert _json_line(r.stdout)["steps"] == 2
    assert sorted(p.name for p in d.iterdir()) == ["onsets.npy"]
    on = np.load(d / "onsets.npy")
    assert on.dtype == np.float64 and on.shape == (3 * 512, 3)
    assert np.array_equal(np.unique(on[:, 0]), np.arange(512))   # (clip, channel, sample) of both shards
    assert np.array_equal(on[:, 2], 1000 * on[:, 0] + np.tile(np.arange(3), 512))


def test_synth_batch_gives_the_recipes_clips_bit_for_bit():
    """The bench's clips come from threads that write into one batch, or into a given tensor row by row (the GPU
    batch in a real run): every row is the synth recipe's clip, bit for bit, in the order of the seeds."""
    import numpy as np
    import torch

    import bench
    from onset_fingerprinting_amd import synth
    seeds = [1, 1 + 7919, 2 + 97]
    x = bench.synth_batch("c2", seeds, 2.0, 8, 2)
    assert x.shape == (3, 96000, 8) and x.dtype == np.float32
    for row, s in zip(x, seeds):
        assert np.array_equal(row.view(np.uint32), synth.c2_drums(2.0, 8, 48000, seed=s).view(np.uint32))
    t = torch.empty((5, 480000, 4))
    assert bench.synth_batch("c4", range(3, 8), 10.0, 4, 3, out=t) is t
    for i in range(5):
        assert np.array_equal(t[i].numpy().view(np.uint32), synth.c4_clip(3 + i, 10.0, 4, 48000).view(np.uint32))
