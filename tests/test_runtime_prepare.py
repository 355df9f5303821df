"""ofp_runtime_prepare (include/onsetfp.h): importing the package asks the HIP runtime for 16 hardware queues while
the runtime can still be asked, and leaves a process alone whose runtime is already up.  Each case runs in a fresh
child process: the setting is per process and is read once."""
import subprocess
import sys
from pathlib import Path

import pytest

REPO = Path(__file__).resolve().parent.parent

# what the C library sees: os.environ is Python's copy, getenv() is what the HIP runtime reads
_GETENV = """
import ctypes
def c_getenv(name):
    f = ctypes.CDLL(None).getenv
    f.restype, f.argtypes = ctypes.c_char_p, [ctypes.c_char_p]
    v = f(name.encode())
    return None if v is None else v.decode()
"""


def _child(code, env_value):
    import os
    env = {k: v for k, v in os.environ.items() if k != "GPU_MAX_HW_QUEUES"}
    if env_value is not None:
        env["GPU_MAX_HW_QUEUES"] = env_value
    r = subprocess.run([sys.executable, "-c", _GETENV + code], cwd=str(REPO), env=env, capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout.strip().splitlines()[-1]


@pytest.mark.parametrize("before", [None, "4"])
def test_import_sets_sixteen_queues_before_torch_cuda(before):
    out = _child("""
import os, sys
import torch                       # bench.py's order: torch first, torch.cuda untouched
assert not torch.cuda.is_initialized()
import onset_fingerprinting_amd
assert not torch.cuda.is_initialized()
print(c_getenv("GPU_MAX_HW_QUEUES"), os.environ.get("GPU_MAX_HW_QUEUES"))
""", before)
    assert out == "16 16"


def test_prepare_makes_no_hip_call():
    """The function decides without touching the runtime: called twice in a process that never uses the GPU it sets the
    variable both times (the runtime is still down after the first call)."""
    out = _child("""
from onset_fingerprinting_amd import _lib
print(_lib.lib().ofp_runtime_prepare(), _lib.lib().ofp_runtime_prepare(), c_getenv("GPU_MAX_HW_QUEUES"))
""", None)
    assert out == "1 1 16"


@pytest.mark.gpu
def test_prepare_leaves_a_running_runtime_alone():
    out = _child("""
import os
import torch
torch.zeros(1, device="cuda").sum().item()        # the HIP runtime is up, with whatever it read
from onset_fingerprinting_amd import _lib           # (the import's own call comes too late as well)
print(_lib.lib().ofp_runtime_prepare(), _lib.runtime_prepare(), c_getenv("GPU_MAX_HW_QUEUES"),
      os.environ.get("GPU_MAX_HW_QUEUES"))
""", "4")
    assert out == "0 0 4 4"
