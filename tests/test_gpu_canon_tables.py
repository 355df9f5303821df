"""The dB and back-to-linear canon with its tables in LDS (csrc/ofp_canon_dev.h, what the detector's elementwise passes
run) against the header's form (include/ofp_math.h, tables in global memory), device against device, over ALL 2^32 float32
bit patterns.

The header's form is pinned to the oracle by tests/test_gpu_canon.py over whole binades; the two forms are the same fp64
operations and differ only in where `OFP_LOG_R[i]`, `OFP_LOG_T[i]` and `OFP_EXP2_T[n & 31]` are read from, so they must agree
on every bit of every input, NaN payloads included: the comparison is torch.equal on the raw bits.  A wrong or unfilled
table slot shows on the inputs that index it; the second test asserts on the CPU that the sweep's inputs index every slot, so
that a later narrowing of the sweep cannot hide one."""
import numpy as np
import pytest
import torch

from onset_fingerprinting_amd.detection import canon_eval

CHUNK = 1 << 26
SWEEP = [(lo, CHUNK) for lo in range(0, 1 << 32, CHUNK)]  # (first bit pattern, count): all of float32
FLOORS = (-70.0, -90.0)
OPS = (("rect_db", "rect_db_lds"), ("rel_linear", "rel_linear_lds"))


def chunk_bits(lo, n, device):
    """Bit patterns lo .. lo + n - 1 as an int32 tensor (a chunk never straddles 2^31)."""
    assert (lo < 1 << 31) == (lo + n - 1 < 1 << 31)
    s = lo - (1 << 32) if lo >= 1 << 31 else lo
    return torch.arange(s, s + n, dtype=torch.int32, device=device)


@pytest.mark.gpu
@pytest.mark.parametrize("floor", FLOORS)
@pytest.mark.parametrize("op,op_lds", OPS)
def test_tables_in_lds_give_the_headers_bits_for_every_float32(op, op_lds, floor):
    assert sum(n for _, n in SWEEP) == 1 << 32 and [lo for lo, _ in SWEEP] == list(range(0, 1 << 32, CHUNK))
    dev = torch.device("cuda", 0)
    want = torch.empty(CHUNK, dtype=torch.float32, device=dev)
    got = torch.empty(CHUNK, dtype=torch.float32, device=dev)
    for lo, n in SWEEP:
        x = chunk_bits(lo, n, dev).view(torch.float32)
        canon_eval(op, x, p0=floor, out=want[:n])
        got.fill_(-1.0)
        canon_eval(op_lds, x, p0=floor, out=got[:n])
        if not torch.equal(got[:n].view(torch.int32), want[:n].view(torch.int32)):
            bad = torch.nonzero(got[:n].view(torch.int32) != want[:n].view(torch.int32)).flatten()
            i = int(bad[0])
            pytest.fail(f"{op_lds}, floor {floor}: {bad.numel()} of the patterns from {lo:#010x} differ; first {lo + i:#010x}: "
                        f"{int(got[i].view(torch.int32)) & 0xFFFFFFFF:#010x} for {int(want[i].view(torch.int32)) & 0xFFFFFFFF:#010x}")


LOG2_10 = 3.321928094887362


def log_index(x):
    """(table index of ofp_log10f inside ofp_rect_db, mask of the inputs that reach the table)"""
    with np.errstate(all="ignore"):
        a = np.abs(x + np.float32(1e-10))
        reach = np.isfinite(a) & (a > 0)
        mant = a.astype(np.float64).view(np.uint64) & np.uint64(0x000FFFFFFFFFFFFF)
        return (mant >> np.uint64(45)).astype(np.int64), reach


def exp_index(d):
    """(table index of ofp_exp10f inside ofp_rel_linear, mask of the inputs that reach the table)"""
    with np.errstate(all="ignore"):
        v = d / np.float32(20.0)
        reach = (v < np.float32(39.0)) & (v > np.float32(-46.0))  # (false for NaN)
        tn = np.where(reach, v, np.float32(0.0)).astype(np.float64) * LOG2_10 * 32.0
        n = np.trunc(tn + np.where(tn >= 0, 0.5, -0.5)).astype(np.int64)
        return n & 31, reach


def test_the_sweep_reaches_every_table_slot():
    """Every 2^14-th pattern of every chunk of SWEEP (so: inputs the sweep holds) -- the seven mantissa bits that index the log
    tables are among those that vary, and so is every residue of exp10's n."""
    x = np.concatenate([np.arange(lo, lo + n, 1 << 14, dtype=np.uint64) for lo, n in SWEEP]).astype(np.uint32).view(np.float32)
    i, reach = log_index(x)
    seen = set(i[reach].tolist())
    assert seen == set(range(128)), sorted(set(range(128)) - seen)
    assert min(seen) < 53 <= max(seen)  # both sides of the m / 2 switch
    for side in (i[reach] < 53, i[reach] >= 53):
        assert side.sum() > 1000
    n, reach = exp_index(x)
    seen = set(n[reach].tolist())
    assert seen == set(range(32)), sorted(set(range(32)) - seen)
