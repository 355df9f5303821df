"""numpy reference of site 2 of the trainers' random stream (include/onsetfp.h, "Site 2, stretches"), written from the
rule alone on top of tests/train_random_ref.py, and the stretched windows of an epoch: for every (item, channel) the
fp64 Fourier resampling of the rows the item reads with the bound oracle/post_kernels.py derives for
ofp_resample_windows."""
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent))
import train_random_ref as R  # noqa: E402

SITE_STRETCH = 2
_32 = np.uint64(32)


def stretch_of_words(words, S):
    """uint32 words -> int32 stretches: v = (word * 2 (S - 1)) >> 32, then the lower half maps to -(S-1) .. -1 and the
    upper half to 1 .. S-1; never 0."""
    assert S >= 2
    v = ((np.asarray(words, np.uint32).astype(np.uint64) * np.uint64(2 * (S - 1))) >> _32).astype(np.int64)
    return np.where(v < S - 1, v - (S - 1), v - (S - 1) + 1).astype(np.int32)


def stretches(seed, epoch, n, S):
    """int32 [n]: the stretch of item i is drawn from word i of (seed, epoch, site 2)."""
    return stretch_of_words(R.words(seed, epoch, SITE_STRETCH, n), S)


def draws(seed, epoch, n_items, max_shift, S):
    """(shifts, stretches) of an epoch, int32 [n_items] each; the shifts are site 1's, untouched by the stretch."""
    sh = R.shifts(seed, epoch, n_items, max_shift) if max_shift else np.zeros(n_items, np.int32)
    return sh, stretches(seed, epoch, n_items, S)


def stretched_windows(audio, starts, W, seed, epoch, max_shift, S, n_extractions):
    """audio [N, C], starts int64 [O] -> (shifts [n], stretches [n], ref float64 [n, C, W], bound float64 [n, C, W]),
    n = R O, item j = r O + i: the rows starts[i] + shift_j .. + W + stretch_j of every channel, resampled to W."""
    from oracle import post_kernels as K
    audio = np.asarray(audio, np.float32)
    starts = np.asarray(starts, np.int64)
    O, C = len(starts), audio.shape[1]
    n = O * n_extractions
    sh, sd = draws(seed, epoch, n, max_shift, S)
    ref, bound = np.empty((n, C, W)), np.empty((n, C, W))
    for j in range(n):
        for c in range(C):
            x = K.resample_window(audio, int(starts[j % O]) + int(sh[j]), W + int(sd[j]), c)
            ref[j, c], bound[j, c] = K.resample_ref(x, W)
    return sh, sd, ref, bound
