"""oracle/locate_kernels.py without a GPU: its numpy references reproduce the committed recordings of the reference
project (g22: lag maps with their extremes and the legality queries; g23: every find_lag / find_lag_multi case, the
paired vote's cells and grids, the 2-D maps and the intensity maps), every case table has the edges it is there
for, and every correlation row of the tables sums to the same fp64 value in either order."""
import json

import numpy as np
import pytest

from oracle import locate_kernels as K
from tests.conftest import load_golden

f32, f64 = np.float32, np.float64
DIAMETER = 14 * 2.54


def same_bits(got, want):
    assert got.dtype == want.dtype and got.shape == want.shape
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan)
    assert np.array_equal(got[~nan], want[~nan])


# ---- the references against the recordings ----------------------------------------------------------------------

def test_lag_map_reference_reproduces_g22_maps():
    g = load_golden("g22_locate")
    names = sorted({k.split("/")[1] for k in g.files if k.startswith("map/")})
    assert len(names) == 7
    for name in names:
        kw = json.loads(str(g[f"map/{name}/args"]))
        scale, tol = kw.get("scale", 1), kw.get("tol", 1)
        c = kw.get("c") or K.speed_of_sound(100 * scale, medium=kw.get("medium", "air"))
        r, mask_r2 = (K.grid_3d if kw["kind"] == "3d" else K.grid_2d)(kw.get("d", DIAMETER), scale, tol)
        mics = [list(kw["mic_b"])[:3], list(kw["mic_a"])[:3]]
        if kw["kind"] == "2d":
            mics = [m[:2] for m in mics]
        maps, _, _ = K.lag_maps_ref(mics, r, c, kw.get("sr", 96000), mask_r2)
        same_bits(maps[0, 1], g[f"map/{name}/map"])


@pytest.mark.parametrize("name", ["rt3", "air4"])
def test_references_reproduce_g22_layouts_and_legality(name):
    g = load_golden("g22_locate")
    kw = json.loads(str(g[f"m3d/{name}/args"]))
    c = K.speed_of_sound(100, medium=kw["medium"])
    radius = DIAMETER / 2
    sensors = K.sensors3([K.spherical_to_cartesian(x[0] * radius, x[1], x[2]) for x in kw["sensor_locations"]])
    assert np.array_equal(sensors, g[f"m3d/{name}/sensor_locs"])
    r, mask_r2 = K.grid_3d(DIAMETER, 1, 2)
    spc = kw["sr"] / c
    maps, mn, mx = K.lag_maps_ref(sensors, r, c, kw["sr"], mask_r2, floor=-spc)
    same_bits(maps, g[f"m3d/{name}/maps"])
    same_bits(mn, g[f"m3d/{name}/min"])
    same_bits(mx, g[f"m3d/{name}/max"])
    got = K.legal_ref(g[f"m3d/{name}/maps"], g[f"legal/{name}/sensors"], g[f"legal/{name}/onsets"], spc)
    assert np.array_equal(got, g[f"legal/{name}/idx"])
    assert (got != 0).any() and (got == 0).all(1).any()


@pytest.mark.parametrize("name", ["m3", "m4air"])
def test_references_reproduce_g23_2d_maps(name):
    g = load_golden("g23_locate2d")
    kw = json.loads(str(g[f"m2d/{name}/args"]))
    c = K.speed_of_sound(100, medium=kw["medium"])
    sensors = [K.polar_to_cartesian(x[0] * DIAMETER / 2, x[1]) for x in kw["sensor_locations"]]
    assert np.array_equal(np.array(sensors, f64), g[f"m2d/{name}/sensor_locs"])
    r, mask_r2 = K.grid_2d(DIAMETER, 1, 2)
    spc = kw["sr"] / c
    maps, mn, mx = K.lag_maps_ref(sensors, r, c, kw["sr"], mask_r2, floor=-spc)
    same_bits(maps, g[f"m2d/{name}/maps"])
    same_bits(mn, g[f"m2d/{name}/min"])
    same_bits(mx, g[f"m2d/{name}/max"])
    pre = f"m2d/{name}/legal"
    assert np.array_equal(K.legal_ref(maps, g[f"{pre}/sensors"], g[f"{pre}/onsets"], spc), g[f"{pre}/idx"])


def test_find_reference_reproduces_every_g23_case():
    g = load_golden("g23_locate2d")
    n = len(g["fl/lag"])
    assert n == 548 and int(g["fl/near_tie"].sum()) == 59
    d = g["fl/data"]
    for k in range(n):  # no case is left out, the near-ties included
        o, la, lb = g["fl/off"][k], int(g["fl/len_a"][k]), int(g["fl/len_b"][k])
        a, b = d[o[0]:o[0] + la].astype(f32) / 256, d[o[1]:o[1] + lb].astype(f32) / 256
        t, nf = int(g["fl/top_n"][k]), int(g["fl/n_found"][k])
        lag, pl, pv, npk = K.find_ref(a, b, t)
        assert lag == int(g["fl/lag"][k]), k
        assert npk == nf and np.array_equal(pl[:nf], g["fl/peaks"][k, :nf]), k
        # the recording's values come from a correlation accumulated in fp32; test_gpu_locate2d.py's bound for them
        want_v = g["fl/vals"][k, :nf]
        assert nf == 0 or np.abs(pv[:nf] - want_v).max() <= 1e-6 * max(float(np.max(want_v)), 1e-30), k
        assert np.isnan(pv[nf:]).all()


@pytest.mark.parametrize("name", ["p4mm", "p3air", "p2"])
def test_vote_reference_reproduces_g23_cells_and_grids(name):
    g = load_golden("g23_locate2d")
    kw = json.loads(str(g[f"pair/{name}/args"]))
    p = K.Paired(kw["sensor_locations"], DIAMETER, kw["scale"], kw["sr"])
    assert p.side == int(g[f"pair/{name}/side"]) and p.radius == int(g[f"pair/{name}/radius"])
    assert np.array_equal(p.sensors[:, :2], g[f"pair/{name}/sensor_locs"])
    m0 = p.maps[1, 0]  # the reference's map (0, 1)
    assert np.array_equal(np.isnan(m0), g[f"pair/{name}/map0_nan"])
    assert np.array_equal(np.nan_to_num(m0, nan=0).astype(np.int16), g[f"pair/{name}/map0"])
    slots = [p.slot_map(s) for s in range(2 * p.S)]
    pre = f"pair/{name}/cc"
    res_idx = list(g[f"{pre}/res_idx"])
    for h in range(len(g[f"{pre}/cell"])):
        res, cell = K.vote_ref(slots, p.S, int(g[f"{pre}/first"][h]), g[f"{pre}/lags"][h], 2)
        assert cell == int(g[f"{pre}/cell"][h]), h
        if h in res_idx:
            assert np.array_equal(res.reshape(p.side, p.side), g[f"{pre}/res"][res_idx.index(h)].astype(f32)), h
        x, y = K.cell_xy(cell, p.side)
        assert np.array_equal(np.array(K.cartesian_to_polar(x, y, p.radius)), g[f"{pre}/rphi"][h]), h


def test_intensity_reference_reproduces_g23_within_one_ulp():
    g = load_golden("g23_locate2d")
    for name in sorted({k.split("/")[1] for k in g.files if k.startswith("lim/")}):
        kw = json.loads(str(g[f"lim/{name}/args"]))
        r = int(np.round(kw.get("d", DIAMETER), 1) * kw["scale"]) // 2
        ref = K.intensity_ref([kw["mic_a"], kw["mic_b"]], r, kw["reflectivity"]).astype(f32)
        for k, key in enumerate("ab"):
            want = g[f"lim/{name}/{key}"]
            assert (np.abs(ref[k] - want) <= np.spacing(np.abs(want))).all(), (name, key)


# ---- the tables have the edges they name ------------------------------------------------------------------------

def test_plus_zero_only_changes_the_sign_of_zero():
    a = np.array([-0.0, 0.0, -1.5, np.nan, np.inf, 1e-45], f32)
    got = K.plus_zero(a)
    assert got.dtype == f32 and not np.signbit(got[:2]).any()
    assert np.array_equal(got[2:].view(np.uint32), a[2:].view(np.uint32))
    m = np.array([-0.0, 0.0, -3.0], f32)  # either zero is a correct maximum
    assert np.nanmax(m) == 0 and np.nanmax(m[::-1]) == 0


def test_map_table_edges():
    cases = K.map_cases()
    assert {(len(s), r) for _, s, r, *_ in cases} == set(K.MAP_SHAPES)
    assert [(2 * r + 1) ** 2 for _, r in K.MAP_SHAPES] == [1, 225, 289, 529, 9]
    assert 225 < K.WG < 289 and max(S for S, _ in K.MAP_SHAPES) == 64 and 5 * 5 == 25
    for name, s, r, c, sr, mask_r2, floor in cases:
        maps, mn, mx = K.lag_maps_ref(s, r, c, sr, mask_r2, floor)
        S, side = len(s), 2 * r + 1
        assert (s[2:, 2] != 0).all() and s[1, 2] == 0 and float(s[1, 0]).is_integer() and abs(s[1, 0]) <= r
        off = ~np.eye(S, dtype=bool)
        assert np.isnan(maps[~off]).all() and np.isnan(mn[~off]).all()
        valid = ~np.isnan(maps[off])
        if name.endswith("open"):
            assert valid.all()
            assert np.array_equal(maps[off], np.rint(maps[off]))
        elif name.endswith("circle") and r > 1:
            assert valid.any() and not valid.all()
        elif name.endswith("centre"):
            assert valid.reshape(-1, side, side)[:, r, r].all() and valid.sum() == S * (S - 1)
        elif name.endswith(("none", "floor_all")):
            assert not valid.any() and np.isnan(mn).all() and np.isnan(mx).all()
        elif name.endswith("floor_some") and r > 0:
            assert valid.any() and not valid.all() and (maps[off][valid] >= 0).all()


@pytest.mark.parametrize("side", K.LEGAL_SIDES)
def test_legal_table_edges(side):
    maps, sens, onsets, tol, info = K.legal_table(side)
    cells = side * side
    assert cells in (1, 225, 289)
    ref = K.legal_ref(maps, sens, onsets, tol)
    names = [n for n, _ in info]
    want_only = {0, cells - 1} | {k for k in K.LEGAL_FLAT if k < cells}
    assert {int(n[5:]) for n in names if n.startswith("only_")} == want_only
    for q, (name, want) in enumerate(info):
        if want == "refused":
            assert tuple(ref[q]) == (-1, -1) and (sens[q].min() < 0 or sens[q].max() >= maps.shape[0])
            continue
        s, o = sens[q], onsets[q]
        m1, m2 = maps[s[0], s[1]].reshape(-1), maps[s[0], s[2]].reshape(-1)
        l1, l2 = float(o[1] - o[0]), float(o[2] - o[0])
        mask = K.legal_mask(m1, m2, l1, l2, tol)
        assert np.array_equal(maps[s[0], s[1]], np.rint(maps[s[0], s[1]]), equal_nan=True)
        if want is None:
            assert not mask.any() and tuple(ref[q]) == (0, 0), name
        else:
            assert int(np.flatnonzero(mask)[0]) == want and tuple(ref[q]) == (want % side, want // side), name
        if name.startswith("only_"):
            assert mask.sum() == 1
        if name == "scattered" and cells > 1:
            assert mask.sum() > 1
        if name.startswith("edges") and cells > 4:  # values exactly at lag - tol and lag + tol, not legal
            at = ((m1 == l1 - tol) | (m1 == l1 + tol) | (m2 == l2 - tol) | (m2 == l2 + tol))
            assert at.sum() >= 4 and not (at & mask).any()
        if name.startswith("nans") and cells > 1:
            assert np.isnan(m1).any() and np.isnan(m2).any()
    assert tuple(ref[names.index("only_0")]) == (0, 0) == tuple(ref[names.index("none")])
    if cells > 4:  # the other tolerances the kernel is run with change the answers
        q = names.index("edges_then_legal")  # at 2.5 the cells at lag +- 2 are legal: cell 0 comes first
        assert tuple(ref[q]) == (5, 0) and tuple(K.legal_ref(maps, sens, onsets, 2.5)[q]) == (0, 0)
        assert not K.legal_ref(maps, sens, onsets, 0.0)[:len(names) - 2].any()


@pytest.mark.parametrize("d", K.M3D_DIAMETERS)
@pytest.mark.parametrize("C", [3, 4, 5])
def test_rows_table_edges(d, C):
    m = K.m3d(d)
    assert (2 * m.r + 1) ** 2 == {14: 225, 16: 289}[d] and len(m.sensors) == 5
    assert len({round(float(z), 6) for z in m.sensors[:, 2]}) > 2  # mixed elevations
    groups, n_groups, where = K.rows_table(d, C)
    assert groups.shape == (4, K.ROWS_CAP, C) and K.ROWS_CAP == 7
    assert sorted(n_groups) == [0, 3, 7, 9]
    status, guess, geom, delta = K.replay_rows(m, groups, n_groups)
    st = lambda name: int(status[where[name]])
    row = lambda name: groups[where[name]]
    order = lambda h: [c for _, c in sorted((int(v), c) for c, v in enumerate(h) if v >= 0)[:3]]
    assert (status[0] == K.LOCATE_UNUSED).all() and (status[1, 3:] == K.LOCATE_UNUSED).all()
    assert (status[1, :3] != K.LOCATE_UNUSED).all() and (status[2:] != K.LOCATE_UNUSED).all()
    assert (K.replay_rows(m, groups, None)[0] != K.LOCATE_UNUSED).all()
    assert st("few_two") == st("few_none") == K.LOCATE_FEW_CHANNELS
    assert (row("few_two") >= 0).sum() == 2 and (row("few_none") >= 0).sum() == 0
    assert st("second_is_1") == 0 and order(row("second_is_1"))[1] == 1
    g1 = geom[where["second_is_1"]].reshape(3, 3)
    assert np.array_equal(g1[1], m.sensors[0]) and np.array_equal(g1[2], m.sensors[1])  # the reordering
    assert st("plain") == 0
    for name, k in (("tie_two", 2), ("tie_three", 3)):
        h = row(name)
        o = order(h)
        assert len({int(h[c]) for c in o[:k]}) == 1 and o[:k] == sorted(o[:k])
    if C > 3:
        assert st("not_first_three") == 0 and max(order(row("not_first_three"))) > 2
        assert (row("absent") < 0).sum() == 1 and st("absent") == 0
    h = row("lag_at_max")
    assert h[1] - h[0] == m.mx[0, 1] and st("lag_at_max") == K.LOCATE_ILLEGAL_LAG
    assert st("lag_below_max") != K.LOCATE_ILLEGAL_LAG
    off = ~np.eye(5, dtype=bool)
    assert (m.mn[off] < 0).all()  # a lag is >= 0, so it never meets a pair's smallest value
    assert st("no_cell") == K.LOCATE_NO_CELL
    h = row("no_cell")
    assert m.mn[0, 1] < h[1] - h[0] < m.mx[0, 1] and m.mn[0, 2] < h[2] - h[0] < m.mx[0, 2]
    assert (status == 0).sum() >= 8 and not np.isnan(guess[status == 0]).any()


def test_section_table_edges():
    cases = K.section_cases()
    assert {c[0] for c in cases} == {3, 4, 5, 257, 258, 600} and {c[1] for c in cases} == {2, 5}
    assert any(c[2] == c[3] for c in cases) and any(c[2] != c[3] for c in cases)
    for n, ld, c0, c1, x in cases:
        assert x.shape == (n, ld) and np.array_equal(x, np.rint(x)) and np.abs(x).max() <= 3
        ref = K.section_ref(x, c0, c1)
        assert ref.shape == (2, n - 1) and ref.dtype == f32 and (ref >= 0).all()
        if c0 == c1:
            assert np.array_equal(ref[0], ref[1])
        # the median of 5 written out with the reflection d c b a | a b c d | d c b a
        col = x[:, c0]
        pad = np.concatenate([col[1::-1], col, col[:-3:-1]])
        med = np.array([np.sort(pad[t:t + 5])[2] for t in range(n)])
        d = np.diff(med)
        assert np.array_equal(ref[0], np.where(d >= 0, 0, -d).astype(f32))
    assert any(K.section_ref(x, c0, c1).any() for _, _, c0, c1, x in cases)


@pytest.mark.parametrize("La,Lb", K.FIND_SHAPES)
def test_find_table_edges(La, Lb):
    assert (128 + 129 - 1, 129 + 129 - 1, 256 + 257 - 1) == (256, 257, 512) and K.FIND_TOP == (0, 1, 16)
    rows = K.find_table(La, Lb)
    names = [r[0] for r in rows]
    exp = dict(zip(names, K.find_expected(La, Lb, 16)))
    for name, a, b, la, lb in rows:
        assert len(a) <= La and len(b) <= Lb
        for v in (a[np.isfinite(a)], b[np.isfinite(b)]):  # integers in [-127, 127] over 256
            assert np.array_equal(v * 256, np.rint(v * 256)) and np.abs(v * 256).max(initial=0) <= 127
    assert rows[names.index("random_full")][3:] == (La, Lb)
    for name in ("len_a_zero", "len_b_zero", "len_a_above", "len_b_above", "len_negative"):
        assert exp[name][0] == K.INT_MIN and exp[name][3] == -2
    r = rows[names.index("len_a_above")]
    assert r[3] == La + 1 and rows[names.index("len_b_above")][4] == Lb + 1
    if La > 2 and Lb > 2:
        r = rows[names.index("random_short")]
        assert 1 <= r[3] < La and 1 <= r[4] < Lb
    for name in ("nan_sample", "inf_sample", "inf_times_zero"):
        _, a, b, la, lb = rows[names.index(name)]
        cc = K.correlate32(a, b)
        assert exp[name][3] == -1 and not np.isfinite(cc).all()
        assert exp[name][0] == int(np.argmax(cc)) - (la - 1)
        if np.isnan(cc).any():
            assert exp[name][0] == int(np.flatnonzero(np.isnan(cc))[0]) - (la - 1)  # the first NaN wins
    _, a, b, la, lb = rows[names.index("constant_rows")]
    cc = K.correlate32(a, b)
    assert (cc == cc[0]).all() and exp["constant_rows"][0] == -(la - 1) and exp["constant_rows"][3] == 0
    for m, at in ((64, 0), (256, 192), (257, 193), (512, 226), (4096, 3810)):
        for mirrored in ("", "_mirrored"):
            if f"plateaus_{m}{mirrored}" not in exp:
                assert (m > Lb) if mirrored else (m > La)
                continue
            for kind in K.PATTERNS:
                name = f"{kind}_{m}{mirrored}"
                _, a, b, la, lb = rows[names.index(name)]
                cc = K.correlate32(a, b)
                assert len(cc) == m
                lag, pl, pv, npk = exp[name]
                want = [at + k for k in K.PATTERN_PEAKS[kind]]
                got = sorted((pl[:npk] + (la - 1)).tolist())
                if len(want) <= 16:
                    assert got == want, name
                else:  # more than 16 peaks: the 16 largest, equal values by ascending index
                    top = sorted(want, key=lambda p: (-float(cc[p]), p))[:16]
                    assert npk == 16 and (pl[:16] + (la - 1)).tolist() == top, name
                    assert cc[top[15]] == cc[sorted(want, key=lambda p: (-float(cc[p]), p))[16]]  # cut inside a tie
                assert np.array_equal(pv[:npk], (cc * cc)[pl[:npk] + (la - 1)]) and np.isnan(pv[npk:]).all()
                assert (np.diff(cc[pl[:npk] + (la - 1)]) <= 0).all()
                if kind == "constant":
                    assert lag == -(la - 1) and npk == 0
                if kind == "negative":
                    assert (cc < 0).all() and npk == 3 and (pl[:2] + (la - 1)).tolist() == [at + 5, at + 13]
                if kind == "peaks16":
                    assert npk == 16
                if kind == "plateaus":  # odd width 3, even widths 4 and 2
                    assert cc[at + 2] == cc[at + 4] and cc[at + 10] == cc[at + 13] and cc[at + 20] == cc[at + 21]
                if kind == "ends":
                    assert cc[0] == cc[2] == cc[-1] == cc[-3] == cc.max() and npk == 1
                if kind == "max_first":
                    assert int(np.argmax(cc)) == 0 and lag == -(la - 1)
                if kind == "max_last":
                    assert int(np.argmax(cc)) == m - 1 and lag == m - 1 - (la - 1)
    if (La, Lb) == (4096, 4096):
        assert "peaks20_4096" in exp and "peaks20_4096_mirrored" in exp
    e1 = K.find_expected(La, Lb, 1)
    for (lag, pl, pv, npk), (lag1, pl1, pv1, npk1) in zip(K.find_expected(La, Lb, 16), e1):
        assert lag1 == lag and npk1 == min(npk, 1) and (npk < 1 or pl1[0] == pl[0])


@pytest.mark.parametrize("La,Lb", K.FIND_SHAPES)
def test_correlation_rows_are_order_independent(La, Lb):
    for row in K.find_table(La, Lb):
        a, b = K.find_row_inputs(row, La, Lb)
        assert K.order_independent(a, b), row[0]
        if np.isfinite(a).all() and np.isfinite(b).all() and len(a):
            # and the ascending sum is what np.correlate returns, so the reference has no rounding of its own
            pad = np.concatenate([np.zeros(len(b) - 1), a.astype(f64), np.zeros(len(b) - 1)])
            j = len(pad) - len(b) - (len(a) - 1) // 2  # one lag in the middle
            up = np.cumsum(pad[j:j + len(b)] * b.astype(f64))[-1]
            assert np.correlate(a.astype(f64), b.astype(f64), "full")[j] == up, row[0]


def test_order_check_sees_a_rounding():
    a = np.array([1.0, 2.0 ** -53, 2.0 ** -53], f32)  # (1 + h) + h = 1 but (h + h) + 1 = 1 + 2**-52 in fp64
    assert not K.order_independent(a, np.ones(3, f32))
    assert K.order_independent(np.array([0.25, -0.5, 0.125], f32), np.ones(3, f32))


def test_index_table_edges():
    assert {c[0] for c in K.INDEX_CASES} == {1, 63, 64, 65, 81, 1 << 20}
    assert {c[1] for c in K.INDEX_CASES} == {1, 255, 256, 257, 32768}
    assert {c[2] for c in K.INDEX_CASES} == {1, 3, 128}
    assert K.INDEX_REFUSED == ((4, 16, 129), ((1 << 20) + 1, 16, 1), (4, 32769, 1))
    seen_bad = seen_nan = False
    for cells, nb, n_maps, kind in K.INDEX_CASES:
        pool, ids, vmin, bad = K.index_table(cells, nb, n_maps, kind)
        assert (vmin < 0).all() and len(set(ids.tolist())) == n_maps
        assert n_maps == 1 or not np.array_equal(ids, np.arange(n_maps))
        for k in range(n_maps):
            m = pool[ids[k]]
            starts, order, b = K.vote_index_ref(m, int(vmin[k]), nb)
            assert b == bad[k] and starts[0] == 0 and starts[-1] == len(order) and len(starts) == nb + 1
            seen_bad |= bool(b)
            seen_nan |= bool(np.isnan(m).any())
            if b:
                assert starts[-1] < (~np.isnan(m)).sum()
                assert (m != np.rint(m)).any() and (m[~np.isnan(m)] >= vmin[k] + nb).any() and \
                    (m[~np.isnan(m)] < vmin[k]).any()
            v = m[order].astype(f64) - vmin[k]
            assert (np.diff(v) >= 0).all() and (np.diff(order)[np.diff(v) == 0] > 0).all()  # stable
            if kind == "one":
                assert np.count_nonzero(np.diff(starts)) == 1 and starts[-1] == cells - 3 * b
            if kind == "distinct":
                assert np.diff(starts).max() == 1 and starts[-1] == cells
                assert nb == cells or (starts[1] == 1 and starts[nb] - starts[nb - 1] == 1)
            if kind == "ends":
                assert starts[1] > 0 and starts[nb] - starts[nb - 1] > 0 and starts[nb - 1] == starts[1]
    assert seen_bad and seen_nan


@pytest.mark.parametrize("k", range(len(K.PAIRED_MODELS)))
def test_paired_table_edges(k):
    p = K.paired(k)
    assert (p.side, p.S) == ((5, 2), (9, 3), (17, 5))[k] and p.side ** 2 in (25, 81, 289)
    if k == 2:
        assert p.n_buckets + 1 > K.WG
    slots = [p.slot_map(s) for s in range(2 * p.S)]
    for s, m in enumerate(slots):
        assert np.array_equal(m, np.rint(m), equal_nan=True)
        assert K.vote_index_ref(m, int(p.vmin[s]), p.n_buckets)[2] == 0
    first, lags = K.vote_hits(slots, p.S, 5 + k)
    kinds = {t: set() for t in K.PAIRED_TOLS}
    for t in K.PAIRED_TOLS:
        for f, l in zip(first, lags):
            kind = K.vote_kind(slots, p.S, int(f), l, t)
            kinds[t].add(kind)
            res, cell = K.vote_ref(slots, p.S, int(f), l, t)
            if kind == "both_empty":
                assert cell == 0 and not res.any()
            elif kind == "overlap":
                assert res[cell] == 2 and not (res[:cell] == 2).any()
            elif kind in ("disjoint", "one_empty", "single"):
                assert res.max() == 1 and cell == int(np.flatnonzero(res)[0])
    assert kinds[0] == {"both_empty"}  # lag - 0 < v < lag + 0 holds for no value
    want = {"both_empty", "single"} if p.S == 2 else {"both_empty", "one_empty", "disjoint", "overlap"}
    for t in (1, 2, 2.5):
        assert want <= kinds[t], (t, kinds[t])
    assert "overlap" in kinds[0.5] or p.S == 2
    lo = min(int(np.nanmin(m)) for m in slots)
    hi = max(int(np.nanmax(m)) for m in slots)
    assert lags.min() == K.INT_MIN and lags.max() == 2 ** 31 - 1 and (lags[:, 0] < lo).any() and (lags[:, 1] > hi).any()
    for B in (1, 64, 65):
        l, f = K.solve_rows(p, B)
        assert l.shape == (B, 2) and ((f >= p.S).sum() == (1 if B > 64 else 0))
        geom, delta, guess = K.paired_guess(p, l, f)
        assert np.isfinite(guess).all()


def test_synthetic_vote_tables_at_the_cell_cap():
    side = 1024
    maps, vmin, nb = K.synthetic_maps(side, 3)
    assert maps.shape == (6, 1 << 20) and nb <= 32768 and np.isnan(maps).any()
    assert np.array_equal(maps, np.rint(maps), equal_nan=True)
    first, lags = K.vote_hits(list(maps), 3, 9)
    kinds = {K.vote_kind(list(maps), 3, int(f), l, 2) for f, l in zip(first, lags)}
    assert {"both_empty", "one_empty", "overlap"} <= kinds


def test_window_tables_edges():
    N, left, right = 300, 10, 40
    for S, C in ((2, 2), (3, 5)):
        onset, first, clip = K.window_hits(N, S, left, right)
        a_off, b_off, ln, f, st = K.windows_ref(2, N, C, S, left, right, onset, first, clip)
        assert {K.PAIRED_OK, K.PAIRED_NEG_WINDOW, K.PAIRED_EMPTY_WINDOW, K.PAIRED_BAD_HIT} == set(st.tolist())
        ok = st == K.PAIRED_OK
        assert (ln[ok, 0] == left + right).any() and (ln[ok, 0] < left + right).any() and (ln[ok] >= 1).all()
        assert (ln[~ok] == 0).all() and (a_off[~ok] == 0).all()
        assert ((first < 0) | (first >= S)).any() and ((clip < 0) | (clip >= 2)).any()
        assert (a_off[ok] + (ln[ok].astype(np.int64) - 1) * C < 2 * N * C).all()  # the last sample read is inside x
        g, ng = K.window_groups(N, C, S, left, right)
        a_off, b_off, ln, f, st = K.windows_ref(3, N, C, S, left, right, groups=g, n_groups=ng)
        want = {K.PAIRED_OK, K.PAIRED_UNUSED, K.PAIRED_NO_CHANNEL, K.PAIRED_NEG_WINDOW, K.PAIRED_EMPTY_WINDOW}
        if C > S:
            want.add(K.PAIRED_BAD_HIT)
        assert want == set(st.tolist()), (S, C, set(st.tolist()))
        cap = g.shape[1]
        assert f[2 * cap] == 0 and len(set(g[2, 0].tolist())) == 1  # a tie of all channels: channel 0
        assert f[2 * cap + 1] == 1 and g[2, 1, 1] == g[2, 1, min(2, C - 1)] and g[2, 1, 0] == -1
        assert (st[:cap] == K.PAIRED_UNUSED).all() and (st[cap + 3:2 * cap] == K.PAIRED_UNUSED).all()
        assert (K.windows_ref(3, N, C, S, left, right, groups=g)[4] != K.PAIRED_UNUSED).all()


def test_intensity_table_edges():
    assert {c[0] for c in K.INTENSITY_CASES} == {0, 7, 8}
    for r, a, b, refl in K.INTENSITY_CASES:
        assert a[2] > 0 and b[2] > 0
        ref = K.intensity_ref([a, b], r, refl)
        assert ref.shape == (2, 2 * r + 1, 2 * r + 1) and np.isfinite(ref).all()
