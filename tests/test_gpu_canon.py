"""The canon of include/ofp_math.h on the device (ofp_canon_eval) against the same functions on the host (the C oracle), over
the sets of tests/value_domain_cases.py: whole binades of bit patterns, the specials, and the step pairs.

The rule of every comparison: the device's value is bit-equal to the host's wherever the host's is no NaN, and a NaN exactly
where the host's is.  Sign and payload of a NaN are left open (x86 and gfx950 differ there legitimately).  No tolerance
anywhere.  tests/test_value_domain_cpu.py checks the host side against independent evaluations without a GPU."""
import numpy as np
import pytest
import torch

import oracle
from onset_fingerprinting_amd import detection
from tests import value_domain_cases as vd

pytestmark = pytest.mark.gpu

CANARY = 0x7FA5A5A5  # a NaN pattern no op produces
GUARD = 64


def device_eval(op, x, y=None, p0=0.0, p1=0.0):
    xd = torch.from_numpy(x).cuda()
    yd = torch.from_numpy(y).cuda() if y is not None else None
    out = detection.canon_eval(op, xd, yd, float(p0), float(p1))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def assert_same(got, want, x, what, y=None):
    bad = vd.same_where_not_nan(got, want)
    if len(bad):
        i = bad[0]
        raise AssertionError(f"{what}: {len(bad)} of {len(x)} values differ; first at x = {x[i]!r} (0x{vd.bits(x)[i]:08x})"
                             + (f", y = {y[i]!r} (0x{vd.bits(y)[i]:08x})" if y is not None else "")
                             + f": device 0x{vd.bits(got)[i]:08x}, host 0x{vd.bits(want)[i]:08x}")


HOST1 = {"log10": lambda x, f: oracle.log10f(x), "exp10": lambda x, f: oracle.exp10f(x),
         "rect_db": oracle.rect_db, "rel_linear": oracle.rel_linear}


def unary_cases():
    cases = []
    for g in vd.L_GROUPS:
        cases.append(("log10", vd.L_GROUPS, g, False, 0.0))
    for g in vd.E_GROUPS:
        cases.append(("exp10", vd.E_GROUPS, g, True, 0.0))
    for f in vd.RECT_DB_FLOORS:
        for groups in (vd.L_GROUPS, vd.L93_GROUPS):
            for g in groups:
                cases.append(("rect_db", groups, g, True, f))
    for f in vd.REL_LINEAR_FLOORS:
        for groups in (vd.E_GROUPS, vd.E9_GROUPS):
            for g in groups:
                cases.append(("rel_linear", groups, g, True, f))
    return cases


UNARY = unary_cases()


@pytest.mark.parametrize("case", UNARY, ids=[f"{op}-{g}-{f}" for op, _, g, _, f in UNARY])
def test_unary_op_over_a_chunk_group(case):
    op, groups, g, both_signs, floor = case
    for neg in ((False, True) if both_signs else (False,)):
        x = groups[g](neg)
        with np.errstate(all="ignore"):
            want = HOST1[op](x, floor)
        assert_same(device_eval(op, x, None, floor), want, x, f"{op} {g} {'-' if neg else '+'} floor {floor}")


@pytest.mark.parametrize("op", list(HOST1))
def test_unary_op_on_the_specials(op):
    x = vd.specials()
    for floor in (vd.RECT_DB_FLOORS if op == "rect_db" else vd.REL_LINEAR_FLOORS if op == "rel_linear" else (0.0,)):
        with np.errstate(all="ignore"):
            want = HOST1[op](x, floor)
        assert_same(device_eval(op, x, None, floor), want, x, f"{op} specials floor {floor}")


def step_runs():
    """(op, parameters, host function) for every coefficient set."""
    runs = [("ar_step", c, oracle.ar_step) for c in vd.AR_COEFFS]
    runs += [("min_step", c, oracle.min_step) for c in vd.MIN_COEFFS]
    runs += [("max_step", c, oracle.max_step) for c in vd.MAX_COEFFS]
    return runs


@pytest.mark.parametrize("pairs", list(vd.STEP_SETS))
@pytest.mark.parametrize("op", ["ar_step", "min_step", "max_step"])
def test_step_op_over_a_pair_set(op, pairs):
    x, y = vd.STEP_SETS[pairs]()
    xd, yd = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    for name, coeffs, host in step_runs():
        if name != op:
            continue
        got = detection.canon_eval(op, xd, yd, *[float(c) for c in coeffs]).cpu().numpy()
        with np.errstate(all="ignore"):
            want = host(x, y, *coeffs)
        assert_same(got, want, x, f"{op} {pairs} {coeffs}", y)


@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "4_bytes_off"])
@pytest.mark.parametrize("n", [0, 1, 255, 256, 257])
def test_sizes_and_alignment_with_guarded_outputs(n, off):
    """Every op at n around one workgroup, on arrays that start on and 4 bytes off a 16-byte boundary; the output lies between
    guard zones filled with a canary, and holds the canary itself before the call."""
    rng = np.random.default_rng(1000 + n)
    s = vd.specials()
    x = np.ascontiguousarray(np.resize(np.concatenate([s, vd.f32(rng.integers(0, 1 << 32, 300, dtype=np.uint64).astype(np.uint32))]), n))
    y = np.ascontiguousarray(np.resize(np.concatenate([s[::-1], np.float32(rng.uniform(-70, 10, 300))]), n))

    def placed(a):
        flat = torch.empty(n + 4, dtype=torch.float32, device="cuda")
        t = flat[off:off + n]
        t.copy_(torch.from_numpy(a))
        assert n == 0 or t.data_ptr() % 16 == 4 * off
        return t
    xd, yd = placed(x), placed(y)
    hosts = [("log10", (), lambda: oracle.log10f(x)), ("exp10", (), lambda: oracle.exp10f(x)),
             ("rect_db", (-70.0,), lambda: oracle.rect_db(x, -70.0)), ("rel_linear", (-70.0,), lambda: oracle.rel_linear(x, -70.0))]
    hosts += [(op, c, (lambda h=h, c=c: h(x, y, *c))) for op, c, h in step_runs()[::2]]
    for op, params, host in hosts:
        buf = torch.full((GUARD + n + 4 + GUARD,), 0, dtype=torch.int32, device="cuda")
        buf.fill_(CANARY)
        out = buf.view(torch.float32)[GUARD + off:GUARD + off + n]
        detection.canon_eval(op, xd, yd if op.endswith("_step") else None, *[float(p) for p in params], out=out)
        torch.cuda.synchronize()
        got = buf.cpu().numpy().view(np.uint32)
        assert np.all(got[:GUARD + off] == CANARY) and np.all(got[GUARD + off + n:] == CANARY), (op, n, off, "guard overwritten")
        if n:
            with np.errstate(all="ignore"):
                want = host()
            assert_same(got[GUARD + off:GUARD + off + n].view(np.float32), want, x, f"{op} n={n} off={off}", y)
