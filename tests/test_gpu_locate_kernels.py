"""The locator kernels of csrc/ofp_locate.hip, csrc/ofp_locate2d.hip and first_legal / med5 of
csrc/ofp_locate_dev.h one by one on the case tables of oracle/locate_kernels.py, against plain numpy references:
bit for bit everywhere, except the polar coordinates (4 ulp of fp64) and the intensity maps (one float32 ulp).  The
tables sit at the grid and capacity edges the recordings of the reference project never reach: one cell and one
partial workgroup, 64 sensors, the first legal cell around the 256-slot reduction, C > 3 channels, correlation
lengths of 256, 257 and 512 and rows of 4096 samples, 16 peaks, 32768 buckets, 2^20 cells and 128 maps.
tests/test_locate_kernels_cpu.py shows that the references and tables are sound.

The kernels are reached through the wrappers of onset_fingerprinting_amd.multilateration; where a test needs a
shape the wrappers cannot form, or a guard behind the output, it calls the C ABI.  Such outputs go into buffers filled
with NaN (integers: the most negative value) with a guard tail, so an element that was not written or a store past
the end fails as well.
"""
import ctypes

import numpy as np
import pytest
import torch

from oracle import locate_kernels as K

pytestmark = pytest.mark.gpu

f32, f64 = np.float32, np.float64
GUARD = 64
_FILL = {torch.float32: float("nan"), torch.float64: float("nan"), torch.int32: -2 ** 31, torch.int64: -2 ** 63}


def L():
    from onset_fingerprinting_amd import _lib
    return _lib.lib()


def ml():
    from onset_fingerprinting_amd import multilateration
    return multilateration


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def ok(rc, what):
    from onset_fingerprinting_amd import _lib
    _lib.check(rc, what)


_LIVE = []


def dev(a, dt=f32):
    """A device copy that lives until the test ends: a temporary whose data_ptr() is handed to the C ABI would be
    freed, and its block given to the next copy, before the kernel has read it."""
    _LIVE.append(torch.from_numpy(np.ascontiguousarray(a, dt)).cuda())
    return _LIVE[-1]


@pytest.fixture(autouse=True)
def release():
    yield
    torch.cuda.synchronize()
    _LIVE.clear()


def guarded(*shape, dtype=torch.float32):
    """(view of `shape`, whole buffer): the fill value everywhere, GUARD elements behind the view."""
    numel = int(np.prod(shape))
    buf = torch.full((numel + GUARD,), _FILL[dtype], dtype=dtype, device="cuda")
    return buf[:numel].view(*shape), buf


def untouched(t):
    return bool(torch.isnan(t).all()) if t.dtype.is_floating_point else bool((t == _FILL[t.dtype]).all())


def guard_ok(*bufs):
    return all(untouched(b[-GUARD:]) for b in bufs)


def host(t):
    return t.detach().cpu().numpy()


def same(got, want, ctx):
    """Equal bit patterns, NaN matching NaN."""
    got = host(got) if torch.is_tensor(got) else np.asarray(got)
    want = np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (ctx, got.dtype, want.dtype, got.shape, want.shape)
    if got.dtype.kind == "f":
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got), nan), (ctx, "NaN positions", np.argwhere(np.isnan(got) != nan)[:4].tolist())
        bits = {4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
        got, want = np.where(nan, 0, got).view(bits), np.where(nan, 0, want).view(bits)
    assert np.array_equal(got, want), (ctx, np.argwhere(got != want)[:4].tolist())


# ---- 1. ofp_lag_maps --------------------------------------------------------------------------------------------

def test_lag_maps_and_extremes():
    for name, s, r, c, sr, mask_r2, floor in K.map_cases():
        S, side = len(s), 2 * r + 1
        want, want_mn, want_mx = K.lag_maps_ref(s, r, c, sr, mask_r2, floor)
        maps, b0 = guarded(S, S, side, side)
        mn, b1 = guarded(S, S)
        mx, b2 = guarded(S, S)
        ok(L().ofp_lag_maps(dev(s, f64).data_ptr(), S, r, c, sr, mask_r2, floor, maps.data_ptr(), mn.data_ptr(),
                            mx.data_ptr(), stream()), name)
        same(maps, want, name)
        # (the sign of an extreme that is zero is not defined by numpy's reduction: oracle/locate_kernels.py)
        same(K.plus_zero(host(mn)), K.plus_zero(want_mn), name)
        same(K.plus_zero(host(mx)), K.plus_zero(want_mx), name)
        assert guard_ok(b0, b1, b2), name
        w_maps, w_mn, w_mx = ml().lag_maps_device(s, r, c, sr, mask_r2, floor=floor)  # the wrapper's own call
        same(w_maps, want, name)
        same(w_mn, host(mn), name)
        same(w_mx, host(mx), name)


def test_lag_maps_refuses_past_the_caps():
    s = dev(np.zeros((65, 3)), f64)
    maps, b0 = guarded(1024)
    mn, b1 = guarded(64)
    args = lambda S, r: (s.data_ptr(), S, r, 8200.0, 96000.0, 1e9, -np.inf, maps.data_ptr(), mn.data_ptr(),
                         mn.data_ptr(), stream())
    assert L().ofp_lag_maps(*args(65, 0)) == 1
    assert L().ofp_lag_maps(*args(2, 4097)) == 1
    torch.cuda.synchronize()
    assert untouched(b0) and untouched(b1)


# ---- 2. ofp_locate_legal ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("side", K.LEGAL_SIDES)
def test_first_legal_cell(side):
    maps, sens, onsets, tol, _ = K.legal_table(side)
    want = K.legal_ref(maps, sens, onsets, tol)
    md = dev(maps)
    for t in (tol, 2.5, 1.0, 0.0):  # 2.5: the values at lag +- 2 are legal too; 0: no value is
        same(ml().legal_cells_device(md, dev(sens, np.int32), dev(onsets, np.int64), t),
             K.legal_ref(maps, sens, onsets, t), (side, t))
    S = maps.shape[0]
    for G in (0, 1, 3, len(sens)):
        idx, buf = guarded(max(G, 1), 2, dtype=torch.int32)
        ok(L().ofp_locate_legal(md.data_ptr(), S, (side - 1) // 2, dev(sens[:G], np.int32).data_ptr(),
                                dev(onsets[:G], np.int64).data_ptr(), G, tol, idx.data_ptr(), stream()), (side, G))
        same(idx[:G], want[:G], (side, G))
        assert untouched(idx[G:]) and guard_ok(buf), (side, G)


# ---- 3. ofp_locate_groups, ofp_trilaterate ----------------------------------------------------------------------

@pytest.fixture(scope="module")
def layouts():
    out = {}
    for d in K.M3D_DIAMETERS:
        m = ml().Multilaterate3D(K.M3D_LOCATIONS, drum_diameter=d, sr=K.M3D_SR, c=K.M3D_C)
        ref = K.m3d(d)
        assert m.grid_radius == ref.r and m.radius == ref.radius and m.c == ref.c
        same(np.array(m.sensor_locs, f64), ref.sensors, d)
        same(m.maps_dev, ref.maps, d)
        same(K.plus_zero(host(m.min_dev)), K.plus_zero(ref.mn), d)
        same(K.plus_zero(host(m.max_dev)), K.plus_zero(ref.mx), d)
        out[d] = m
    return out


@pytest.mark.parametrize("d", K.M3D_DIAMETERS)
@pytest.mark.parametrize("C", [3, 4, 5])
def test_locate_groups_rows(layouts, d, C):
    m, ref = layouts[d], K.m3d(d)
    groups, n_groups, _ = K.rows_table(d, C)
    gd = dev(groups, np.int64)

    def expected(ng):
        """status (the solver's ier where a row is solved), xy (bit for bit trilaterate_device's) and guess."""
        status, guess, geom, delta = K.replay_rows(ref, groups, ng)
        solved = status == 0
        root, ier, _ = ml().trilaterate_device(dev(geom[solved], f64), dev(delta[solved], f64),
                                               dev(guess[solved], f64))
        want_st, want_xy = status.copy(), np.full(status.shape + (2,), np.nan)
        want_st[solved], want_xy[solved] = host(ier), host(root)
        return want_st, want_xy, guess

    for ng in (n_groups, None):
        want_st, want_xy, guess = expected(ng)
        xy, st, gs = ml().locate_groups_device(gd, dev(ng, np.int64) if ng is not None else None, m,
                                               return_guess=True)
        same(st, want_st, (d, C))
        same(gs, guess, (d, C))
        same(xy, want_xy, (d, C))
    want_st, want_xy, guess = expected(n_groups)
    # the C ABI with guards behind every output
    n_clips, cap = groups.shape[:2]
    rows = n_clips * cap
    xy, b0 = guarded(rows, 2, dtype=torch.float64)
    st, b1 = guarded(rows, dtype=torch.int32)
    gs, b2 = guarded(rows, 2, dtype=torch.float64)
    ws = torch.empty(int(L().ofp_locate_workspace_bytes(rows)), dtype=torch.uint8, device="cuda")
    ok(L().ofp_locate_groups(gd.data_ptr(), n_clips, cap, C, dev(n_groups, np.int64).data_ptr(),
                             m.sensors_dev.data_ptr(), 5, m.maps_dev.data_ptr(), m.min_dev.data_ptr(),
                             m.max_dev.data_ptr(), m.grid_radius, float(m.samples_per_cm), float(m.sr), float(m.c),
                             float(m.radius), ml().XTOL, ml().MAXFEV, None, xy.data_ptr(), st.data_ptr(),
                             gs.data_ptr(), ws.data_ptr(), ws.numel(), stream()), (d, C))
    same(st.view(n_clips, cap), want_st, (d, C))
    same(xy.view(n_clips, cap, 2), want_xy, (d, C))
    same(gs.view(n_clips, cap, 2), guess, (d, C))
    assert guard_ok(b0, b1, b2)


def test_trilaterate_rows_do_not_depend_on_the_batch():
    from tests.conftest import load_golden
    g = load_golden("g22_locate")
    geom, delta, guess = (np.ascontiguousarray(g[f"solve3/{k}"][:200]) for k in ("geom", "delta", "guess"))
    full = [host(t) for t in ml().trilaterate_device(dev(geom, f64), dev(delta, f64), dev(guess, f64))]
    for G in (1, 64, 65):
        for at in (0, 200 - G):
            root, b0 = guarded(G, 2, dtype=torch.float64)
            ier, b1 = guarded(G, dtype=torch.int32)
            nfev, b2 = guarded(G, dtype=torch.int32)
            sl = slice(at, at + G)
            ok(L().ofp_trilaterate(dev(geom[sl], f64).data_ptr(), dev(delta[sl], f64).data_ptr(),
                                   dev(guess[sl], f64).data_ptr(), G, ml().XTOL, ml().MAXFEV, root.data_ptr(),
                                   ier.data_ptr(), nfev.data_ptr(), stream()), G)
            same(root, full[0][sl], (G, at))
            same(ier, full[1][sl], (G, at))
            same(nfev, full[2][sl], (G, at))
            assert guard_ok(b0, b1, b2), (G, at)


# ---- 4. ofp_locate_section --------------------------------------------------------------------------------------

def test_section_filter():
    for n, ld, c0, c1, x in K.section_cases():
        out, buf = guarded(2, n - 1)
        ok(L().ofp_locate_section(dev(x).data_ptr(), n, ld, c0, c1, out.data_ptr(), stream()), (n, ld, c0, c1))
        same(out, K.section_ref(x, c0, c1), (n, ld, c0, c1))
        assert guard_ok(buf), (n, ld, c0, c1)


# ---- 5. ofp_find_lags -------------------------------------------------------------------------------------------

def find_buffers(rows, La, Lb):
    A, B = np.full((len(rows), La), np.nan, f32), np.full((len(rows), Lb), np.nan, f32)  # NaN behind every row
    for k, (_, a, b, la, lb) in enumerate(rows):
        A[k, :len(a)], B[k, :len(b)] = a, b
    return dev(A), dev(B), dev([r[3] for r in rows], np.int32), dev([r[4] for r in rows], np.int32)


@pytest.mark.parametrize("La,Lb", K.FIND_SHAPES)
def test_find_lags(La, Lb):
    rows = K.find_table(La, Lb)
    R = len(rows)
    A, B, len_a, len_b = find_buffers(rows, La, Lb)
    for top in K.FIND_TOP:
        exp = K.find_expected(La, Lb, top)
        want_lag = np.array([e[0] for e in exp], np.int32)
        want_pl = np.stack([e[1] for e in exp]).reshape(R, top)
        want_pv = np.stack([e[2] for e in exp]).reshape(R, top)
        want_n = np.array([e[3] for e in exp], np.int32)
        lag, b0 = guarded(R, dtype=torch.int32)
        pl, b1 = guarded(R, max(top, 1), dtype=torch.int32)
        pv, b2 = guarded(R, max(top, 1))
        npk, b3 = guarded(R, dtype=torch.int32)
        ok(L().ofp_find_lags(A.data_ptr(), B.data_ptr(), R, La, Lb, 1, None, None, La, Lb, len_a.data_ptr(),
                             len_b.data_ptr(), top, lag.data_ptr(), pl.data_ptr() if top else None,
                             pv.data_ptr() if top else None, npk.data_ptr(), stream()), (La, Lb, top))
        names = [r[0] for r in rows]
        bad = np.flatnonzero(host(lag) != want_lag)
        assert bad.size == 0, (La, Lb, top, [(names[k], int(host(lag)[k]), int(want_lag[k])) for k in bad[:4]])
        bad = np.flatnonzero(host(npk) != want_n)
        assert bad.size == 0, (La, Lb, top, [(names[k], int(host(npk)[k]), int(want_n[k])) for k in bad[:4]])
        if top:
            same(pl.view(-1)[:R * top].view(R, top), want_pl, (La, Lb, top))
            same(pv.view(-1)[:R * top].view(R, top), want_pv, (La, Lb, top))
            assert untouched(pl.view(-1)[R * top:]) and untouched(pv.view(-1)[R * top:])
        else:
            assert untouched(pl) and untouched(pv)
        assert guard_ok(b0, b1, b2, b3), (La, Lb, top)
        w = ml().find_lags_device(A, B, top, len_a, len_b)  # the wrapper's own call
        same(w[0], want_lag, (La, Lb, top))
        same(w[1], want_pl, (La, Lb, top))
        same(w[2], want_pv, (La, Lb, top))
        same(w[3], want_n, (La, Lb, top))
    full = [k for k, r in enumerate(rows) if r[3:] == (La, Lb)]  # without per-row lengths: the buffers' own
    A2, B2 = A[full].contiguous(), B[full].contiguous()
    w = ml().find_lags_device(A2, B2, 16)
    exp = K.find_expected(La, Lb, 16)
    same(w[0], np.array([exp[k][0] for k in full], np.int32), (La, Lb))
    same(w[1], np.stack([exp[k][1] for k in full]), (La, Lb))
    same(w[2], np.stack([exp[k][2] for k in full]), (La, Lb))


# ---- 6. ofp_vote_index ------------------------------------------------------------------------------------------

def run_index(pool, ids, vmin, nb):
    n_maps, cells = len(ids), pool.shape[1]
    starts, b0 = guarded(n_maps, nb + 1, dtype=torch.int32)
    order, b1 = guarded(n_maps, cells, dtype=torch.int32)
    bad, b2 = guarded(n_maps, dtype=torch.int32)
    ok(L().ofp_vote_index(pool.data_ptr(), cells, dev(ids, np.int32).data_ptr(), n_maps,
                          dev(vmin, np.int32).data_ptr(), nb, starts.data_ptr(), order.data_ptr(), bad.data_ptr(),
                          stream()), (cells, nb, n_maps))
    assert guard_ok(b0, b1, b2), (cells, nb, n_maps)
    return starts, order, bad


@pytest.mark.parametrize("cells,nb,n_maps,kind", K.INDEX_CASES)
def test_vote_index(cells, nb, n_maps, kind):
    pool, ids, vmin, want_bad = K.index_table(cells, nb, n_maps, kind)
    starts, order, bad = run_index(dev(pool), ids, vmin, nb)
    starts, order = host(starts), host(order)
    same(bad, want_bad, (cells, nb, n_maps))
    for k in range(n_maps):
        w_starts, w_order, _ = K.vote_index_ref(pool[ids[k]], int(vmin[k]), nb)
        same(starts[k], w_starts, (cells, nb, n_maps, k))
        same(order[k, :len(w_order)], w_order, (cells, nb, n_maps, k))  # the tail behind starts[nb] is unspecified


def test_vote_index_refuses_past_the_caps():
    pool = dev(np.zeros((1, 8), f32))
    out, buf = guarded(64, dtype=torch.int32)
    z = torch.zeros(256, dtype=torch.int32, device="cuda")
    for cells, nb, n_maps in K.INDEX_REFUSED:
        assert L().ofp_vote_index(pool.data_ptr(), cells, z.data_ptr(), n_maps, z.data_ptr(), nb, out.data_ptr(),
                                  out.data_ptr(), out.data_ptr(), stream()) == 1, (cells, nb, n_maps)
    torch.cuda.synchronize()
    assert untouched(buf)


# ---- 7. ofp_paired_windows, ofp_paired_vote, ofp_paired_solve ----------------------------------------------------------

@pytest.fixture(scope="module")
def models():
    out = []
    for k, (loc, d, scale, sr) in enumerate(K.PAIRED_MODELS):
        m = ml().MultilateratePaired(loc, drum_diameter=d, scale=scale, sr=sr)
        p = K.paired(k)
        assert (m.side, m.radius, m.n_buckets) == (p.side, p.radius, p.n_buckets)
        same(np.array(m.sensor_locs, f64), p.sensors[:, :2], k)
        same(m.maps_dev, p.maps, k)
        same(m.map_ids, p.ids, k)
        same(m.vmin, p.vmin.astype(np.int32), k)
        starts, order = host(m.starts), host(m.sorted_cells)
        for s in range(2 * p.S):  # the constructor's own ofp_vote_index call
            w_starts, w_order, bad = K.vote_index_ref(p.slot_map(s), int(p.vmin[s]), p.n_buckets)
            assert bad == 0
            same(starts[s], w_starts, (k, s))
            same(order[s, :len(w_order)], w_order, (k, s))
        out.append(m)
    return out


def run_vote(maps, ids, starts, order, vmin, nb, S, side, radius, first, lags, status_in, tol, want_res=True):
    B = len(first)
    cell, b0 = guarded(B, dtype=torch.int32)
    xy, b1 = guarded(B, 2, dtype=torch.float64)
    rphi, b2 = guarded(B, 2, dtype=torch.float64)
    st, b3 = guarded(B, dtype=torch.int32)
    res, b4 = guarded(B, side * side) if want_res else (None, b3)
    ok(L().ofp_paired_vote(maps.data_ptr(), ids.data_ptr(), starts.data_ptr(), order.data_ptr(), vmin.data_ptr(), nb,
                           S, side, dev(first, np.int32).data_ptr(), dev(lags, np.int32).data_ptr(),
                           dev(status_in, np.int32).data_ptr(), B, float(tol), float(radius), cell.data_ptr(),
                           xy.data_ptr(), rphi.data_ptr(), st.data_ptr(), res.data_ptr() if want_res else None,
                           stream()), (side, tol))
    assert guard_ok(b0, b1, b2, b3, b4), (side, tol)
    return host(cell), host(xy), host(rphi), host(st), host(res) if want_res else None


def check_vote(got, slots, S, side, radius, first, lags, status_in, tol, ctx):
    cell, xy, rphi, st, res = got
    same(st, np.asarray(status_in, np.int32), ctx)
    for h in range(len(first)):
        if status_in[h] != K.PAIRED_OK:
            assert cell[h] == -1 and np.isnan(xy[h]).all() and np.isnan(rphi[h]).all(), (ctx, h)
            assert res is None or not res[h].any(), (ctx, h)
            continue
        w_res, w_cell = K.vote_ref(slots, S, int(first[h]), lags[h], tol)
        assert cell[h] == w_cell, (ctx, h, int(cell[h]), w_cell, lags[h].tolist())
        if res is not None:
            same(res[h], w_res, (ctx, h))
        x, y = K.cell_xy(w_cell, side)
        same(xy[h], np.array([x, y]), (ctx, h))
        want = np.array(K.cartesian_to_polar(x, y, radius), f64)
        assert (np.abs(rphi[h] - want) <= 4 * np.spacing(np.maximum(np.abs(want), 1e-300))).all(), (ctx, h)


@pytest.mark.parametrize("k", range(len(K.PAIRED_MODELS)))
def test_paired_vote(models, k):
    m, p = models[k], K.paired(k)
    slots = [p.slot_map(s) for s in range(2 * p.S)]
    first, lags = K.vote_hits(slots, p.S, 5 + k)
    status_in = np.zeros(len(first), np.int32)
    status_in[1::7] = (K.PAIRED_NEG_WINDOW, K.PAIRED_EMPTY_WINDOW, K.PAIRED_BAD_HIT, K.PAIRED_UNUSED)[k]
    for tol in K.PAIRED_TOLS:
        got = run_vote(m.maps_dev, m.map_ids, m.starts, m.sorted_cells, m.vmin, m.n_buckets, p.S, p.side, p.radius,
                       first, lags, status_in, tol)
        check_vote(got, slots, p.S, p.side, p.radius, first, lags, status_in, tol, (k, tol))


def test_paired_vote_at_the_cell_cap():
    side, S = 1024, 3
    slots, vmin, nb = K.synthetic_maps(side, S)
    maps = dev(slots)
    ids = np.arange(2 * S, dtype=np.int32)
    starts, order, bad = run_index(maps, ids, vmin, nb)
    assert not host(bad).any()
    first, lags = K.vote_hits(list(slots), S, 9)
    first, lags = first[::3], lags[::3]
    status_in = np.zeros(len(first), np.int32)
    got = run_vote(maps, dev(ids, np.int32), starts, order, dev(vmin, np.int32), nb, S, side, side / 2.0, first, lags,
                   status_in, 2)
    check_vote(got, list(slots), S, side, side / 2.0, first, lags, status_in, 2, "2^20 cells")
    z = torch.zeros(8, dtype=torch.int32, device="cuda")
    out, buf = guarded(8, dtype=torch.int32)
    f = torch.zeros(8, dtype=torch.float64, device="cuda")
    assert L().ofp_paired_vote(None, None, z.data_ptr(), z.data_ptr(), z.data_ptr(), 4, S, 1025, z.data_ptr(),
                               z.data_ptr(), z.data_ptr(), 1, 2.0, 512.0, out.data_ptr(), f.data_ptr(), f.data_ptr(),
                               out.data_ptr(), None, stream()) == 1
    torch.cuda.synchronize()
    assert untouched(buf)


def run_windows(n_clips, N, C, S, left, right, B, onset=None, first=None, clip=None, groups=None, n_groups=None):
    a_off, b0 = guarded(B, 2, dtype=torch.int64)
    b_off, b1 = guarded(B, 2, dtype=torch.int64)
    ln, b2 = guarded(B, 2, dtype=torch.int32)
    f, b3 = guarded(B, dtype=torch.int32)
    st, b4 = guarded(B, dtype=torch.int32)
    p = lambda a, dt: dev(a, dt).data_ptr() if a is not None else None
    cap = groups.shape[1] if groups is not None else 0
    ok(L().ofp_paired_windows(n_clips, N, C, S, p(onset, np.int64), p(first, np.int32), p(clip, np.int32),
                              p(groups, np.int64), cap, p(n_groups, np.int64), B, left, right, a_off.data_ptr(),
                              b_off.data_ptr(), ln.data_ptr(), f.data_ptr(), st.data_ptr(), stream()), (S, C))
    assert guard_ok(b0, b1, b2, b3, b4), (S, C)
    return a_off, b_off, ln, f, st


def test_paired_windows():
    N, left, right = 300, 10, 40
    for S, C in ((2, 2), (3, 5), (5, 5)):
        onset, first, clip = K.window_hits(N, S, left, right)
        got = run_windows(2, N, C, S, left, right, len(onset), onset, first, clip)
        for g, w in zip(got, K.windows_ref(2, N, C, S, left, right, onset, first, clip)):
            same(g, w, ("hits", S, C))
        got = run_windows(1, N, C, S, left, right, len(onset), onset, first, None)  # no clip index: clip 0
        for g, w in zip(got, K.windows_ref(1, N, C, S, left, right, onset, first, None)):
            same(g, w, ("hits of one clip", S, C))
        groups, n_groups = K.window_groups(N, C, S, left, right)
        for ng in (n_groups, None):
            got = run_windows(3, N, C, S, left, right, groups.shape[0] * groups.shape[1], groups=groups, n_groups=ng)
            for g, w in zip(got, K.windows_ref(3, N, C, S, left, right, groups=groups, n_groups=ng)):
                same(g, w, ("groups", S, C))


@pytest.mark.parametrize("k", range(len(K.PAIRED_MODELS)))
def test_locate_cc_from_audio(models, k):
    """The three kernels chained by the wrappers: impulses whose distance is the lag wanted, one window per hit."""
    m, p = models[k], K.paired(k)
    slots = [p.slot_map(s) for s in range(2 * p.S)]
    first, lags = K.vote_hits(slots, p.S, 5 + k)
    w = 1024
    keep = np.flatnonzero((np.abs(lags.astype(np.int64)) < w // 2).all(1))[:24]
    first, lags = first[keep], lags[keep]
    B, C = len(keep), p.S + 1  # one channel without a sensor
    x = np.zeros((1, B * w, C), f32)
    for h in range(B):  # lag = position in the first channel - position in the neighbour
        i, at = int(first[h]), h * w + w // 2
        x[0, at, i] = 0.25
        x[0, at - lags[h, 0], (i - 1) % p.S] += 0.25
        if p.S > 2:
            x[0, at - lags[h, 1], (i + 1) % p.S] += 0.25
    onset = np.arange(B, dtype=np.int64) * w
    for tol in (2, 0.5):
        rphi, cell, status = m.locate_cc_device(dev(x), dev(onset, np.int64), dev(first, np.int32), tol=tol, left=0,
                                                right=w)
        assert not host(status).any()
        for h in range(B):
            lg = lags[h] if p.S > 2 else np.array([lags[h, 0], lags[h, 0]])
            w_cell = K.vote_ref(slots, p.S, int(first[h]), lg, tol)[1]
            assert host(cell)[h] == w_cell, (k, tol, h)
            want = np.array(K.cartesian_to_polar(*K.cell_xy(w_cell, p.side), p.radius), f64)
            assert (np.abs(host(rphi)[h] - want) <= 4 * np.spacing(np.maximum(np.abs(want), 1e-300))).all()
    h = B // 2  # the reference's call form, with the vote grid
    m.locate_cc(x[0], int(onset[h]), int(first[h]), tol=2, left=0, right=w)
    lg = lags[h] if p.S > 2 else np.array([lags[h, 0], lags[h, 0]])
    same(m.res.reshape(-1), K.vote_ref(slots, p.S, int(first[h]), lg, 2)[0], k)


@pytest.mark.parametrize("k", range(len(K.PAIRED_MODELS)))
def test_paired_solve(models, k):
    m, p = models[k], K.paired(k)
    for B in (1, 64, 65):
        lags, first = K.solve_rows(p, B)
        geom, delta, guess = K.paired_guess(p, lags, first)
        root, b0 = guarded(B, 2, dtype=torch.float64)
        rphi, b1 = guarded(B, 2, dtype=torch.float64)
        ier, b2 = guarded(B, dtype=torch.int32)
        ok(L().ofp_paired_solve(m.sensors_dev.data_ptr(), p.S, dev(lags, np.int32).data_ptr(),
                                dev(first, np.int32).data_ptr(), B, float(m._c()), float(m.sr), float(m.radius),
                                ml().XTOL, ml().MAXFEV, root.data_ptr(), rphi.data_ptr(), ier.data_ptr(), stream()),
           (k, B))
        assert guard_ok(b0, b1, b2), (k, B)
        w_root, w_ier, _ = ml().trilaterate_device(dev(geom, f64), dev(delta, f64), dev(guess, f64))
        w_root, w_ier = host(w_root), host(w_ier)
        valid = (first >= 0) & (first < p.S)
        w_root[~valid], w_ier[~valid] = np.nan, K.PAIRED_BAD_HIT
        same(root, w_root, (k, B))
        same(ier, w_ier, (k, B))
        want = np.stack(K.cartesian_to_polar(w_root[:, 0], w_root[:, 1], p.radius), 1)
        got = host(rphi)
        assert np.array_equal(np.isnan(got), np.isnan(want)), (k, B)
        assert (np.abs(got - want)[valid] <= 4 * np.spacing(np.maximum(np.abs(want[valid]), 1e-300))).all(), (k, B)
        w_rphi, w_ier2 = m.locate_device(dev(lags, np.int32), dev(first, np.int32))  # the wrapper's own call
        same(w_rphi, got, (k, B))
        same(w_ier2, w_ier, (k, B))


# ---- 8. ofp_intensity_maps --------------------------------------------------------------------------------------

def test_intensity_maps():
    for r, a, b, refl in K.INTENSITY_CASES:
        want = K.intensity_ref([a, b], r, refl).astype(f32)
        side = 2 * r + 1
        out, buf = guarded(2, side, side)
        ok(L().ofp_intensity_maps(dev([a, b], f64).data_ptr(), r, refl, out.data_ptr(), stream()), r)
        assert guard_ok(buf), r
        got = host(out)
        assert (np.abs(got - want) <= np.spacing(np.abs(want))).all(), (r, np.abs(got - want).max())
        d = {0: 1, 7: 14, 8: 16}[r]  # lag_intensity_map's grid radius is int(round(d, 1) * scale) // 2
        lag, wa, wb = ml().lag_intensity_map(a, b, reflectivity=refl, d=d, sr=96000, scale=1, medium="air")
        same(np.stack([wa, wb]), got, r)
        c = K.speed_of_sound(100, medium="air")
        same(lag, K.lag_maps_ref([b, a], r, c, 96000, np.inf)[0][0, 1], r)
