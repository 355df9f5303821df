"""Loader for the upstream reference, used ONLY by make_golden.py in the build
container (the reference cannot travel to the GPU box; tests never import this).

The reference's hot-path modules import packages that are not installed
(librosa, loopmate, lightning, audiomentations, soundfile, seaborn).  Placeholder
modules are registered in ``sys.modules`` so the imports succeed; nothing is
fetched.  Two thin delegations make ``data.stft`` runnable:
``librosa.filters.get_window -> scipy.signal.get_window`` and
``librosa.util.pad_center -> numpy.pad``.

The reference's ctypes followers look for ``envelope_follower.so`` next to
``detection.py`` (detection.py:517-519); /root/reference is read-only, so the
library is built from the reference's own C file by ``oracle/Makefile`` into
``$OFP_REF_DIR`` (default ``oracle/_ref``, git-ignored) and ``detection.__file__``
is pointed there after import.
"""
import os
import sys
import types
from pathlib import Path

import numpy as np
import scipy.signal

REPO = Path(__file__).resolve().parents[2]
REF_ROOT = Path("/root/reference")
REF_SO_DIR = Path(os.environ.get("OFP_REF_DIR", str(REPO / "oracle" / "_ref")))


def _pad_center(data, *, size, axis=-1, **kwargs):
    n = data.shape[axis]
    lpad = int((size - n) // 2)
    lengths = [(0, 0)] * data.ndim
    lengths[axis] = (lpad, int(size - n - lpad))
    return np.pad(data, lengths, **kwargs)


class _RingStandIn:
    """STAND-IN for loopmate.circular_array.CircularArray (absent, not vendored), generator side only, for
    the backtracking fixture g18: the three things detection.py uses (:719-721 constructor on an array,
    :756 write(block), :802-803 .N and [-N:] = the last N rows, oldest first).  The reference backs it
    with np.empty (uninitialised rows before the ring has filled); the stand-in zeroes them so that the
    fixture is deterministic.  Because this is OUR reading of the absent class, the Python backtracking
    loop bound stays "parity unpinned"  -- the fixture pins everything else of
    that code path (the loop at detection.py:806-824 itself is the reference's own code, executed)."""

    def __init__(self, data, *a, **k):
        self.data = data
        self.data[...] = 0
        self.N = data.shape[0]

    def write(self, x):
        n = len(x)
        self.data = np.concatenate([self.data[n:], np.asarray(x, dtype=self.data.dtype)])[-self.N:]

    def __getitem__(self, idx):
        return self.data[idx]


def _install_placeholders(ring_stand_in=False):
    def mod(name):
        m = types.ModuleType(name)
        sys.modules[name] = m
        return m

    if "librosa" not in sys.modules:
        librosa = mod("librosa")
        librosa.filters = mod("librosa.filters")
        librosa.util = mod("librosa.util")
        librosa.feature = mod("librosa.feature")
        librosa.filters.get_window = (
            lambda window, Nx, fftbins=True: scipy.signal.get_window(
                window, Nx, fftbins=fftbins
            )
        )
        librosa.util.pad_center = _pad_center
    if "loopmate" not in sys.modules:
        loopmate = mod("loopmate")
        ca = mod("loopmate.circular_array")

        class CircularArray:  # placeholder: backtrack=True path is not run
            def __init__(self, *a, **k):
                raise RuntimeError("loopmate is not available")

        ca.CircularArray = _RingStandIn if ring_stand_in else CircularArray
        loopmate.circular_array = ca
    class _Anything(types.ModuleType):
        # module-level constants in data.py instantiate augmentation objects
        def __getattr__(self, attr):
            if attr.startswith("__"):
                raise AttributeError(attr)
            return lambda *a, **k: None

    for name in ("audiomentations", "soundfile", "seaborn"):
        if name not in sys.modules:
            sys.modules[name] = _Anything(name)
    if "lightning" not in sys.modules:
        import torch

        L = mod("lightning")
        L.LightningModule = torch.nn.Module


def load_reference(ring_stand_in=False):
    """Returns the reference package modules (detection, data, model, calibration).
    ring_stand_in: make ``backtrack=True`` runnable with the ring-buffer stand-in above (g18 only)."""
    if not (REF_SO_DIR / "envelope_follower.so").exists():
        raise RuntimeError("run `make -C oracle ref` first")
    _install_placeholders(ring_stand_in)
    if str(REF_ROOT) not in sys.path:
        sys.path.insert(0, str(REF_ROOT))
    sys.dont_write_bytecode = True
    from onset_fingerprinting import calibration, data, detection, model

    detection.__file__ = str(REF_SO_DIR / "detection.py")
    return types.SimpleNamespace(
        detection=detection, data=data, model=model, calibration=calibration
    )
