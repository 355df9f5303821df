"""oracle/group_kernels.py without a GPU: every row of its case tables has the edge its name claims, recomputed
from the row; the kept-pattern lists reach exactly the group counts and kept sets they are there for; the references
reproduce the committed goldens (g5 grouping, g11 filter through scipy, g1 / g2 / g9 legacy symbols through the C
oracle); and the numpy restatement of the collation block equals the CPU tensor form of distributed.pack_clips."""
import numpy as np
import pytest

from oracle import group_kernels as K
from tests.conftest import load_golden

f32, i64 = np.float32, np.int64


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def by_name(table, prefix):
    rows = [c for c in table if c.name.startswith(prefix)]
    assert rows, prefix
    return rows


def test_names_are_unique():
    for table in (K.GROUP_TABLE, K.OFFSET_CASES, K.WINDOW_CASES, K.PACK_CASES, K.LFILTER_CASES, K.LEGACY_CASES):
        names = [c.name for c in table]
        assert len(set(names)) == len(names)


# ---- GROUP_TABLE: anchor walk -----------------------------------------------------------------------------------

def test_length_rows_put_the_closing_record_on_every_lane_edge():
    rows = by_name(K.GROUP_TABLE, "len")
    assert len(rows) == 2 * 2 * len(K.GROUP_LENGTHS)
    lanes = {False: set(), True: set()}
    tails = {False: set(), True: set()}
    for c in rows:
        spans = K.group_spans(c.onsets, c.md)
        assert tuple(e - a for a, e in spans) == c.lens, c.name
        assert len(K.case_ref(c)) == len(c.lens), c.name           # min_channels 1: every group is a row
        assert (np.diff(c.onsets) >= 0).all()
        L = int(c.name.split("-")[0][3:])
        if c.where == "middle":
            a, e = spans[1]
            assert e - a == L and e < len(c.onsets)
            lanes[c.exact].add(K.far_lane(L))
            assert a + 1 + 64 * K.far_lane(L)[1] + K.far_lane(L)[0] == e   # where the walk from a + 1 meets it
        else:
            a, e = spans[-1]
            assert e - a == L and e == len(c.onsets)
            tails[c.exact].add((e - a - 1) % 64)
        if c.exact:
            for (a, e), nxt in zip(spans, spans[1:] + [None]):
                if e - a > 1:
                    assert c.onsets[e - 1] - c.onsets[a] == c.md, c.name        # the last near one
                if nxt:
                    assert c.onsets[e] - c.onsets[a] == c.md + 1, c.name        # the first far one
    want = {(0, 0), (1, 0), (62, 0), (63, 0), (0, 1), (1, 1), (63, 1), (0, 2), (1, 2)}
    assert lanes[False] == want and lanes[True] == want
    assert 0 in tails[False] and 0 in tails[True]  # a last group whose tail ends exactly at a step (65, 129)


def test_distance_rows():
    t = {c.name: c for c in K.GROUP_TABLE}
    for name in ("md0-equal-runs", "unsorted-below-anchor", "unsorted-leaves-and-returns",
                 "unsorted-returns-past-a-step", "samples-plus-2^40", "samples-minus-2^40", "samples-negative",
                 "distance-2^33"):
        c = t[name]
        spans = K.group_spans(c.onsets, c.md)
        assert tuple(e - a for a, e in spans) == tuple(c.lens), name
        assert len(K.case_ref(c)) == len(spans), name
    c = t["md0-equal-runs"]
    assert c.md == 0 and all(len(set(c.onsets[a:e].tolist())) == 1 for a, e in K.group_spans(c.onsets, 0))
    assert {64, 65, 1} <= set(c.lens)
    c = t["unsorted-below-anchor"]
    a0 = c.onsets[0]
    assert a0 - c.onsets[1] == c.md and a0 - c.onsets[3] == c.md + 1 and K.group_spans(c.onsets, c.md)[0] == (0, 3)
    for name in ("unsorted-leaves-and-returns", "unsorted-returns-past-a-step"):
        c = t[name]
        (a, e) = K.group_spans(c.onsets, c.md)[0]
        assert abs(c.onsets[e] - c.onsets[a]) > c.md                        # closed here ...
        assert (np.abs(c.onsets[e + 1:] - c.onsets[a]) <= c.md).any(), name  # ... though later records are near again
    assert K.group_spans(t["unsorted-returns-past-a-step"].onsets, 100)[0][1] > 64
    assert t["samples-plus-2^40"].onsets.min() >= 2 ** 40 and t["samples-minus-2^40"].onsets.max() < -2 ** 40 + 10 ** 6
    assert t["samples-negative"].onsets.min() < 0
    c = t["distance-2^33"]
    assert c.md > 2 ** 31 and np.abs(np.diff(c.onsets)).max() > 2 ** 31


# ---- GROUP_TABLE: channel chunks --------------------------------------------------------------------------------

def test_close_rows():
    rows = by_name(K.GROUP_TABLE, "close-")
    seen = {}
    for c in rows:
        seen.setdefault(c.C, set()).add(c.cc)
        ref = K.case_ref(c)
        assert np.array_equal(ref, c.rows[np.array(c.kept)]), c.name
        assert len(K.group_spans(c.onsets, c.md)) == len(c.kinds), c.name
        x = c.x
        for kind, row, kept in zip(c.kinds, c.rows, c.kept):
            absent = np.flatnonzero(row == -1)
            present = row[row >= 0]
            if kind == "strict_min":
                assert len(absent) == 0 and (row[x] < np.delete(row, x)).all() and kept
            elif kind == "tie":
                assert len(absent) == 0 and row[x] == row.min() and (row == row.min()).sum() == 2 and kept
            elif kind == "above":
                assert len(absent) == 0 and row[x] == row.min() + 1 and kept == (c.cc is None)
            elif kind == "close_absent":
                assert absent.tolist() == [x] and kept
            elif kind == "absent_same_chunk":
                assert len(absent) == 1 and absent[0] // 64 == x // 64 and row[x] == present.min()
                assert kept == (c.cc is None)
            elif kind == "absent_other_chunk":
                assert len(absent) == 1 and absent[0] // 64 != x // 64 and row[x] == present.min()
                assert kept == (c.cc is None)
            else:
                assert kind == "both_absent" and len(absent) == 2 and x in absent and kept
                assert len({a // 64 for a in absent}) == 2
        if c.C > 64:
            assert {"absent_other_chunk", "both_absent"} <= set(c.kinds)
    assert set(seen) == set(K.CHANNEL_COUNTS)
    for C, ccs in seen.items():
        assert ccs == {cc for cc in (None, 0, 63, 64, C - 1) if cc is None or cc < C}, C
    assert 63 in seen[64] and 64 in seen[65] and 199 in seen[200]


def test_min_channel_rows():
    for C in (130, 3):
        rows = by_name(K.GROUP_TABLE, f"minch-C{C}-")
        mcs = set()
        for c in rows:
            spans = K.group_spans(c.onsets, c.md)
            distinct = [len(set(c.channels[a:e].tolist())) for a, e in spans]
            assert tuple(distinct) == c.distinct
            keep = np.array(distinct) >= c.mc
            assert np.array_equal(K.case_ref(c), c.rows[keep]), c.name
            mcs.add(c.mc)
            a, e = spans[-1]                       # the group with one channel several times
            assert e - a == 5 and distinct[-1] == 2
            last0 = max(k for k in range(a, e) if c.channels[k] == 0)
            assert c.onsets[last0] == c.rows[-1][0] and c.onsets[last0] < c.onsets[a]  # the last and smaller wins
        d = set(rows[0].distinct)
        assert any(m in d for m in mcs) and any(m - 1 in d and m not in d for m in mcs)  # equal, and one above
        assert {0, C + 1} <= mcs
        assert len(K.case_ref(next(c for c in rows if c.mc == C + 1))) == 0
        assert len(K.case_ref(next(c for c in rows if c.mc == 0))) == len(rows[0].distinct)
    c = by_name(K.GROUP_TABLE, "minch-C130-mc4")[0]
    assert {ch // 64 for ch in c.channels.tolist()} == {0, 1, 2}   # distinct is summed over three chunks


# ---- GROUP_TABLE: keep scan and capacity ------------------------------------------------------------------------

def test_pattern_rows_reach_their_group_counts_and_kept_sets():
    want = {
        "all": lambda ng: set(range(ng)),
        "none": lambda ng: set(),
        "g%4==3": lambda ng: set(range(3, ng, 4)),
        "g>=256": lambda ng: set(range(256, ng)),
        "g in (255,256)": lambda ng: {255, 256} & set(range(ng)),
        "alternating": lambda ng: set(range(0, ng, 2)),
        "scan-wave-3": lambda ng: {g for g in range(ng) if g % 256 >= 192},
    }
    seen = set()
    for c in by_name(K.GROUP_TABLE, "pattern-"):
        assert len(K.group_spans(c.onsets, c.md)) == c.ng, c.name
        assert len(c.onsets) == c.ng * c.mc
        ref = K.case_ref(c)
        kept = set((ref[:, 0] // 1000).tolist())
        assert kept == want[c.pattern](c.ng) == {g for g in range(c.ng) if c.kept[g]}, c.name
        assert len(ref) == len(kept)
        seen.add((c.ng, c.pattern, c.cap_groups))
    assert {(ng, p, None) for ng in (255, 256, 257, 513) for p in want} <= seen
    ng, p = K.CAP_PATTERN
    assert sum(next(c for c in K.GROUP_TABLE if c.name == f"pattern-ng{ng}-{p}").kept) == K.CAP_KEPT
    assert {cap for n, q, cap in seen if cap is not None} == {1, K.CAP_KEPT, K.CAP_KEPT - 1, K.CAP_KEPT + 1}


def test_multi_clip_case():
    m = K.multi_clip_case()
    assert len(m.counts) >= 7 and {0, 1, m.cap, m.cap + 5} <= set(m.counts.tolist())
    assert ((m.counts > 1) & (m.counts < m.cap)).any()
    assert (m.counts[1:-1][(m.counts[:-2] > 0) & (m.counts[2:] > 0)] == 0).any()  # an empty clip between full ones
    refs = K.multi_clip_ref(m)
    assert max(len(r) for r in refs) > m.cap_groups and any(0 < len(r) < m.cap_groups for r in refs)
    assert len({r.tobytes() for r in refs if len(r)}) == sum(len(r) > 0 for r in refs)   # different data per clip
    assert (m.records["clip"] != np.arange(len(m.counts))[:, None]).all()
    # the records behind a count are valid ones: grouping them too would change the rows
    k = int(np.flatnonzero((m.counts > 1) & (m.counts < m.cap))[0])
    full = K.groups_ref(m.records["sample"][k], m.records["channel"][k], m.C, m.md, m.mc, None)
    assert full.tobytes() != refs[k].tobytes()
    s = K.singleton_clips_case()
    assert (s.counts == s.cap).all() and s.cap_groups == s.cap and len(s.counts) >= 7
    for k, ref in enumerate(K.multi_clip_ref(s)):
        assert len(K.group_spans(s.records["sample"][k], s.md)) == s.cap and len(ref) == s.cap, k
    rec, counts = K.table_as_batch()
    assert rec.shape[0] == len(K.GROUP_TABLE) and rec.shape[1] == counts.max()
    assert all(max(c.C for c in K.GROUP_TABLE) <= p[0] for p in K.BATCH_PARAMS)


def test_grouping_reference_reproduces_g5():
    g = load_golden("g5_groups")
    n = 0
    for k in range(int(g["n_cases"])):
        md, mc, cc = (int(v) for v in g[f"c{k}_args"])
        on, ch = g[f"c{k}_onsets"], g[f"c{k}_channels"]
        got = K.groups_ref(on, ch, int(ch.max()) + 1, md, mc, None if cc < 0 else cc)
        if bool(g[f"c{k}_none"]):
            assert len(got) == 0
        else:
            assert np.array_equal(got, g[f"c{k}_groups"]), k
            n += 1
    assert n >= 25


# ---- OFFSET_CASES, WINDOW_CASES ---------------------------------------------------------------------------------

def test_offset_cases():
    assert [c.n_clips for c in K.OFFSET_CASES] == [1, 2, 255, 256, 257, 600]
    for c in K.OFFSET_CASES:
        off = K.offsets_ref(c.n_groups, c.cap_groups)
        assert off.dtype == i64 and len(off) == c.n_clips + 1 and off[0] == 0
        assert off[-1] == sum(min(int(n), c.cap_groups) for n in c.n_groups)
        if c.n_clips >= 8:
            ng = c.n_groups
            assert (ng == 0).any() and ((ng > 0) & (ng < c.cap_groups)).any() and (ng == c.cap_groups).any() \
                and (ng > c.cap_groups).any()
    assert K.OFFSET_CASES[0].n_groups[0] > K.OFFSET_CASES[0].cap_groups


def test_window_cases():
    shapes = {(w.C, w.width) for w in K.WINDOW_CASES if w.kinds}
    assert shapes == set(K.WINDOW_SHAPES)
    assert any(w.C * w.width % 256 for w in K.WINDOW_CASES) and any(w.C > 256 for w in K.WINDOW_CASES)
    short = [w for w in K.WINDOW_CASES if w.name.endswith("-short")]
    assert {w.n_samples for w in short} == {1, 40} and all(w.n_samples < w.width for w in short)
    for w in K.WINDOW_CASES:
        n = np.minimum(w.n_groups, w.cap_groups)
        live = [(k, g) for k in range(len(n)) for g in range(n[k])]
        assert (w.n_groups == 0).any() or w in short
        assert (w.n_groups > w.cap_groups).any() or w in short
        if w in short:
            for use_min in (True, False):
                starts = [K.window_starts(w.groups[k, g], w.pre, use_min) for k, g in live]
                assert any(((st < 0) & (st + w.width > w.n_samples)).any() for st in starts), w.name  # both sides
            continue
        if not w.kinds:
            continue
        seen = set()
        for k, g in live:
            kind = w.kinds[(g + k) % len(w.kinds)]
            row = w.groups[k, g]
            seen.add(kind)
            for use_min in (True, False):
                st = K.window_starts(row, w.pre, use_min)
                en = st + w.width
                if kind == "inside":
                    assert (st >= 0).all() and (en <= w.n_samples).all()
                elif kind == "before_0":
                    assert (st < 0).all() and (en <= w.n_samples).all()
                    assert w.width <= 7 or (en > 0).all()
                elif kind == "past_end":
                    assert (st >= 0).all() and (en > w.n_samples).all()
                    assert (st < w.n_samples).all() if w.width > 1 else (st == w.n_samples).all()
                elif kind == "outside_left":
                    assert (en <= 0).all()
                elif kind == "outside_right":
                    assert (st >= w.n_samples).all()
            if kind == "minus_1":
                assert (row == -1).sum() == 1 and row.min() == -1
            if kind == "min_first":
                assert row.argmin() == 0 and (row == row.min()).sum() == 1
            if kind == "min_last":
                assert row.argmin() == w.C - 1 and (row == row.min()).sum() == 1
            if kind == "min_high":
                assert row.argmin() >= 256 and (row == row.min()).sum() == 1
        assert seen == set(w.kinds), w.name
        assert w.C != 300 or "min_high" in seen
    big = next(w for w in K.WINDOW_CASES if w.name == "windows-past-the-grid")
    assert len(big.n_groups) * big.cap_groups > K.WINDOW_GRID
    n = np.minimum(big.n_groups, big.cap_groups)
    assert max(k * big.cap_groups + n[k] - 1 for k in range(len(n)) if n[k]) >= K.WINDOW_GRID  # a live pair past it
    assert (big.n_groups == 0).any() and (big.n_groups > big.cap_groups).any() and len(set(big.n_groups.tolist())) > 4
    assert (big.groups == -1).any()
    for w in K.WINDOW_CASES:
        off = K.offsets_ref(w.n_groups, w.cap_groups)
        total, zero, cut = K.window_cap_totals(w)
        assert total == off[-1] and zero == 0
        assert any(off[k] < cut < off[k + 1] for k in range(len(off) - 1)), w.name
        _, rows = K.windows_ref(w, True)
        assert rows.shape == (total, w.C, w.width) and rows.dtype == f32


# ---- PACK_CASES -------------------------------------------------------------------------------------------------

def test_pack_cases_cover_the_issue():
    P = K.PACK_CASES
    assert {p.n_clips for p in P} == {1, 2, 255, 256, 257, 1500, 65535}
    assert {p.cap for p in P} == {0, 1, 16} and {p.clip_offset for p in P} == {0, 7, -3}
    assert {p.over for p in P} == {True, False}
    assert all((p.counts > p.cap).any() == p.over and (p.counts >= 0).all() for p in P)
    assert all((p.records is None) == (p.cap == 0) for p in P)
    assert any(p.n_clips == 65535 and p.cap == 1 for p in P)
    for n in (1, 2, 255, 256, 257, 1500):
        assert {p.cap for p in P if p.n_clips == n} >= {16} and len([p for p in P if p.n_clips == n]) >= 2
    for p in P:
        t = K.pack_total(p)
        assert set(K.pack_cap_totals(p)) == {0, max(t - 1, 0), t, t + 3}
    assert any(K.pack_total(p) > 1 for p in P)


def test_collation_reference_equals_the_tensor_form():
    import torch
    from onset_fingerprinting_amd.distributed import pack_clips, unpack_gathered
    for p in K.PACK_CASES:
        rec = p.records if p.records is not None else np.zeros((p.n_clips, 0), K.ONSET)
        r8 = torch.from_numpy(rec.view(np.uint8).reshape(p.n_clips, p.cap, 16).copy())
        total = K.pack_total(p)
        for cap_total in K.pack_cap_totals(p):
            want = K.pack_ref(p.records, p.counts, p.cap, cap_total, p.clip_offset)
            assert len(want) == 1 + min(total, cap_total)
            assert want[0]["clip"] == 0 and want[0]["channel"] == int(p.over) and want[0]["sample"] == total
            got = pack_clips(r8, torch.from_numpy(p.counts), cap_total, clip_offset=p.clip_offset)
            assert tuple(got.shape) == (cap_total + 1, 16)
            assert got[:len(want)].numpy().tobytes() == want.tobytes(), (p.name, cap_total)
            if cap_total >= total:
                if p.over:
                    with pytest.raises(RuntimeError):
                        unpack_gathered(got[None])
                else:
                    assert unpack_gathered(got[None]).numpy().tobytes() == want[1:].tobytes(), (p.name, cap_total)


# ---- LFILTER_CASES ----------------------------------------------------------------------------------------------

def test_lfilter_cases():
    plain = [c for c in K.LFILTER_CASES if c.split is None and not hasattr(c, "special")]
    assert [c.order for c in plain] == list(range(9))
    assert {c.C for c in plain} == set(K.LFILTER_CHANNELS) and {c.n for c in plain} == set(K.LFILTER_LENGTHS)
    split = [c for c in K.LFILTER_CASES if c.split is not None]
    assert [c.order for c in split] == list(range(9))
    for c in K.LFILTER_CASES:
        assert c.b.dtype == c.a.dtype == c.x.dtype == c.zi.dtype == f32
        assert c.b.shape == c.a.shape == (c.order + 1,) and c.zi.shape == (c.order, c.C) and c.x.shape == (c.n, c.C)
        assert (np.abs(np.roots(c.a.astype(np.float64))) < 0.85).all(), c.name
    for c in split:
        assert c.a[0] == 2 and (c.order == 0 or c.zi.any()) and 0 < c.split < c.n
        y, zf = K.lfilter_ref(c.x, c.b, c.a, c.zi)
        y0, z0 = K.lfilter_ref(c.x[:c.split], c.b, c.a, c.zi)
        y1, z1 = K.lfilter_ref(c.x[c.split:], c.b, c.a, z0)
        assert np.array_equal(bits(np.concatenate([y0, y1])), bits(y)) and np.array_equal(bits(z1), bits(zf))
    c = next(c for c in K.LFILTER_CASES if c.name == "lfilter-inf-nan")
    y, zf = K.lfilter_ref(c.x, c.b, c.a, c.zi)
    yc, zc = K.lfilter_ref(c.clean, c.b, c.a, c.zi)
    assert np.isinf(c.x[:, c.special]).sum() == 1 and np.isnan(c.x[:, c.special]).sum() == 1
    others = [k for k in range(c.C) if k != c.special]
    assert np.isnan(y[:, c.special]).any() and np.isfinite(y[:, others]).all()
    assert np.array_equal(bits(y[:, others]), bits(yc[:, others])) and np.array_equal(bits(zf[:, others]),
                                                                                      bits(zc[:, others]))


def test_filter_reference_reproduces_g11():
    g = load_golden("g11_lfilter")
    x = g["x"]
    for k in range(3):
        zi = np.zeros((4, x.shape[1]), f32)
        ys = []
        for i in range(0, 3000, 500):
            y, zi = K.lfilter_ref(x[i:i + 500], g[f"b{k}"], g[f"a{k}"], zi)
            ys.append(y)
        assert np.array_equal(bits(np.concatenate(ys)), bits(g[f"y{k}"]))
        assert np.array_equal(bits(zi), bits(g[f"zi{k}"]))


# ---- LEGACY_CASES -----------------------------------------------------------------------------------------------

def test_legacy_references_reproduce_g1_g2_g9():
    from types import SimpleNamespace as NS
    g = load_golden("g1_ar_envelope")
    x = g["x"]
    for k, (a, r) in enumerate(g["pairs"]):
        y = np.full((64, x.shape[1]), -70.0, f32)
        outs = []
        for i in range(0, len(x), 64):
            y = K.ar_ref(NS(x=np.ascontiguousarray(x[i:i + 64]), y0=y, attack=f32(1 / a), release=f32(1 / r)))
            outs.append(y)
        assert np.array_equal(bits(np.concatenate(outs)), bits(g[f"y{k}"]))
    g = load_golden("g2_minmax")
    x, B = g["x"], int(g["B"])
    mn, mx = np.zeros(x.shape[1], f32), np.full(x.shape[1], 10, f32)
    for i in range(0, len(x), B):
        mn, mx = K.minmax_ref(NS(x=np.ascontiguousarray(x[i:i + B]), mn0=mn, mx0=mx, alpha_min=f32(1e-4),
                                 alpha_max=f32(1e-5), minmin=f32(2.0)))
        assert np.array_equal(bits(mn), bits(g["mins"][i // B])) and np.array_equal(bits(mx), bits(g["maxs"][i // B]))
    g = load_golden("g9_backtrack")
    for k in range(3):
        d = K.backtrack_ref(NS(buffer=g["buf"], channels=g["channels"], deltas0=g["deltas0"], alpha=g[f"alpha_{k}"],
                               tol=g[f"tol_{k}"], B=int(g["B"])))
        assert np.array_equal(d, g[f"deltas_{k}"])


def test_legacy_cases():
    for kind in ("ar", "minmax"):
        rows = [c for c in K.LEGACY_CASES if c.kind == kind]
        assert {(c.C, c.n) for c in rows} == {(C, n) for C in K.LEGACY_CHANNELS for n in K.LEGACY_LENGTHS}
    for c in (c for c in K.LEGACY_CASES if c.kind == "ar"):
        other = c.y0.copy()
        other[-1] += 1
        assert not np.array_equal(K.ar_ref(c), K.ar_ref(type(c)(**{**vars(c), "y0": other})))  # the last row is read
        if c.n > 1:
            other = c.y0.copy()
            other[:-1] += 1
            assert np.array_equal(K.ar_ref(c), K.ar_ref(type(c)(**{**vars(c), "y0": other})))  # and no other
    bt = [c for c in K.LEGACY_CASES if c.kind in ("monotone", "falling", "tol")]
    assert {c.n_onsets for c in bt} == {1, 64, 65, 130} and len({c.C for c in bt}) >= 3
    for c in bt:
        i0 = c.B - c.deltas0
        assert (i0 >= 1).all() and (i0 + 1 < c.N).all() and (c.channels < c.C).all()   # every read inside the buffer
        d = K.backtrack_ref(c)
        if c.kind == "monotone":
            assert (d == c.B + 1 - c.N).all() and (d < c.deltas0).all()   # walked to the start of the buffer
        elif c.kind == "falling":
            assert np.array_equal(d, c.deltas0)
        else:
            assert ((d < c.deltas0) & (d > c.B + 1 - c.N)).all()           # moved, and stopped on the way
