"""Case tables and exact references for the kernels of csrc/ofp_groups.hip (k_group_onsets, k_group_offsets,
k_group_windows, k_pack_records) and csrc/ofp_core.hip (k_lfilter and the three legacy symbols ar_envelope,
minmax_envelope, backtrack_onsets) -- TEST INFRASTRUCTURE ONLY.
tests/test_gpu_group_kernels.py runs the kernels on these tables; tests/test_group_kernels_cpu.py shows that every
row has the edge its name claims and that the references reproduce the committed goldens.  Nothing here calls the
code under test or torch.

Everything is compared for equality: grouping, offsets and the collation block are integer work, the windows are
copies, and the filter and the followers are fp32 recurrences that both sides evaluate in the same order without
contraction.

References
  grouping          oracle.groups.find_onset_groups per clip with width = n_channels (pinned by golden g5)
  windows           oracle.groups.group_windows
  offsets           cumsum(min(n_groups, cap_groups)) behind a leading 0
  collation block   pack_ref, written from the contract in include/onsetfp.h
  lfilter           scipy.signal.lfilter on float32 arrays with float32 zi
  legacy symbols    the C restatement oracle/ofp_oracle.c (pinned by goldens g1, g2, g9)

The tables are built by construction: a row's edge follows from how the row is made, `name` says which edge it is and
the remaining fields of the row carry what the construction promises (group lengths, kept flags, rows), so that the
CPU test can recompute it from the row alone.
"""
from types import SimpleNamespace as NS

import numpy as np

from .detector import ar_envelope, backtrack_onsets, minmax_envelope
from .groups import find_onset_groups, group_windows

f32, i32, i64 = np.float32, np.int32, np.int64
WAVE, WG = 64, 256       # wavefront and workgroup of every kernel here
WINDOW_GRID = 4096       # grid cap of k_group_windows: pairs beyond it are reached by the grid stride
ONSET = np.dtype([("clip", i32), ("channel", i32), ("sample", i64)])  # ofp_onset


# ---- 1. ofp_group_onsets ----------------------------------------------------------------------------------------

def group_spans(onsets, max_distance):
    """[a, e) of every group of the greedy scan, kept or not: anchored at a, closed by the first later record farther
    than max_distance from the anchor."""
    on = [int(s) for s in onsets]
    spans, a = [], 0
    while a < len(on):
        e = a + 1
        while e < len(on) and abs(on[e] - on[a]) <= max_distance:
            e += 1
        spans.append((a, e))
        a = e
    return spans


def far_lane(length):
    """(lane, step) at which the anchor walk, which tests 64 candidates per step from anchor + 1, meets the record
    that closes a group of `length` records."""
    return (length - 1) % WAVE, (length - 1) // WAVE


def groups_ref(onsets, channels, C, md, mc, cc):
    """int64 [G, C], G = 0 included."""
    if len(onsets) == 0:
        return np.zeros((0, C), i64)
    g = find_onset_groups(onsets, channels, md, mc, cc, width=C)
    return np.zeros((0, C), i64) if g is None else g


def case_ref(case):
    return groups_ref(case.onsets, case.channels, case.C, case.md, case.mc, case.cc)


def _case(name, onsets, channels, C, md, mc, cc=None, cap_groups=None, **meta):
    on, ch = np.asarray(onsets, i64), np.asarray(channels, i32)
    assert on.ndim == 1 and on.shape == ch.shape and len(on) and ch.min() >= 0 and ch.max() < C, name
    assert cc is None or 0 <= cc < C, name
    return NS(name=name, onsets=on, channels=ch, C=C, md=md, mc=mc, cc=cc, cap_groups=cap_groups, **meta)


GROUP_LENGTHS = (1, 2, 63, 64, 65, 66, 128, 129, 130)


def by_lengths(lens, md, C, exact, base=0):
    """Sorted records forming groups of the given lengths; channel = position in the group mod C.  exact: the last
    record of a group is max_distance from its anchor and the next anchor max_distance + 1."""
    on, ch, s0 = [], [], base
    for L in lens:
        on.append(s0)
        for k in range(1, L):
            on.append(s0 + (-(-k * md // (L - 1)) if exact else k % (md // 2 + 1)))
        ch += [k % C for k in range(L)]
        s0 += md + 1 if exact else 3 * md + 7
    return on, ch


def _length_cases():
    out = []
    for exact in (False, True):
        tag = "exact" if exact else "loose"
        for L in GROUP_LENGTHS:
            for where, lens in (("middle", (3, L, 2)), ("last", (2, L))):
                on, ch = by_lengths(lens, 1000, 4, exact, base=17)
                out.append(_case(f"len{L}-{where}-{tag}", on, ch, 4, 1000, 1, lens=lens, exact=exact, where=where))
    return out


def _distance_cases():
    out = []
    # runs of equal samples, max_distance 0: every run is one group
    runs = (1, 3, 64, 65, 2, 1, 129)
    on = [s for k, n in enumerate(runs) for s in [5 + 2 * k] * n]
    ch = [k % 3 for n in runs for k in range(n)]
    out.append(_case("md0-equal-runs", on, ch, 3, 0, 1, lens=runs))
    # unsorted: records below the anchor, at exactly max_distance (inside) and max_distance + 1 (closes)
    md = 50
    on = [10000, 10000 - md, 10000 + md, 10000 - md - 1, 10000 - md - 1 - md, 10000 - 2 * md - 2 - md]
    out.append(_case("unsorted-below-anchor", on, [0, 1, 2, 0, 1, 2], 3, md, 1, lens=(3, 2, 1)))
    # unsorted: leaves the reach and returns; the greedy scan closes at the FIRST far record, so the records that
    # are near the first anchor again open groups of their own
    on = [1000, 1010, 5000, 1020, 1030, 5010, 5020, 1040]
    out.append(_case("unsorted-leaves-and-returns", on, [0, 1, 2, 0, 1, 2, 0, 1], 3, 100, 1, lens=(2, 1, 2, 2, 1)))
    # the same over more than one step of the walk: 70 near records, one far, 70 near again
    on = [1000 + k for k in range(70)] + [9000] + [1000 + k for k in range(70)]
    out.append(_case("unsorted-returns-past-a-step", on, [k % 4 for k in range(141)], 4, 100, 1, lens=(70, 1, 70)))
    for name, base in (("plus-2^40", 2 ** 40), ("minus-2^40", -2 ** 40), ("negative", -5000)):
        on, ch = by_lengths((3, 65, 1, 4), 1000, 4, True, base=base)
        out.append(_case(f"samples-{name}", on, ch, 4, 1000, 1, lens=(3, 65, 1, 4)))
    # differences and a max_distance that do not fit 32 bits
    on = [-2 ** 40, -2 ** 40 + 2 ** 33, 0, 2 ** 33, 2 ** 33 + 1, 2 ** 40, 2 ** 40 + 2 ** 33]
    out.append(_case("distance-2^33", on, [0, 1, 2, 0, 1, 2, 0], 3, 2 ** 33, 1, lens=(2, 2, 1, 2)))
    return out


CHANNEL_COUNTS = (1, 2, 63, 64, 65, 128, 129, 200)
CLOSE_KINDS = ("strict_min", "tie", "above", "close_absent", "absent_same_chunk", "absent_other_chunk", "both_absent")


def close_group(kind, C, x):
    """{channel: offset} of one group around the channel x, and whether close_channel = x keeps it.  Offsets are in
    [3, 61]."""
    off = {c: 11 + (c * 7) % 50 for c in range(C)}
    y = (x + 1) % C                              # a second channel
    z_same = x ^ 1 if (x ^ 1) < C else x - 1     # a channel of x's 64-chunk
    z_other = x - WAVE if x >= WAVE else WAVE + x % max(C - WAVE, 1)  # a channel of another 64-chunk (C > 64)
    if kind == "strict_min":
        off[x] = 3
        return off, True
    if kind == "tie":
        off[x] = off[y] = 10
        return off, True
    if kind == "above":
        off[y], off[x] = 10, 11
        return off, False
    if kind == "close_absent":                   # -1 <= every entry
        del off[x]
        return off, True
    off[x] = 3
    if kind == "absent_same_chunk":
        if z_same // WAVE != x // WAVE:          # x is alone in the last chunk (C = 65, 129)
            return None, None
        del off[z_same]
        return off, False
    assert C > WAVE and z_other // WAVE != x // WAVE
    del off[z_other]
    if kind == "absent_other_chunk":
        return off, False
    del off[x]                                   # both_absent
    return off, True


def _close_cases():
    out = []
    for C in CHANNEL_COUNTS:
        for cc in sorted({None, 0, 63, 64, C - 1} - {None}) + [None]:
            if cc is not None and cc >= C:
                continue
            x = 0 if cc is None else cc
            kinds = CLOSE_KINDS[:1] if C == 1 else CLOSE_KINDS[:5] if C <= WAVE else CLOSE_KINDS
            kinds = [k for k in kinds if close_group(k, C, x)[0] is not None]
            on, ch, rows, kept = [], [], [], []
            for g, kind in enumerate(kinds):
                off, keep = close_group(kind, C, x)
                s0 = 1000 * (g + 1)
                order = [c for c in list(range(C))[::-1] if c in off]
                order = order[g % len(order):] + order[:g % len(order)]
                on += [s0 + off[c] for c in order]
                ch += order
                rows.append([s0 + off[c] if c in off else -1 for c in range(C)])
                kept.append(keep or cc is None)
            out.append(_case(f"close-C{C}-cc{cc}", on, ch, C, 100, 1, cc, kinds=tuple(kinds), kept=tuple(kept),
                             rows=np.array(rows, i64).reshape(len(kinds), C), x=x))
    return out


def _min_channel_cases():
    out = []
    for C, sets in ((130, ((0,), (0, 63), (0, 63, 64), (0, 63, 64, 129), (5, 62, 63, 64, 128))),
                    (3, ((0,), (0, 2), (0, 1, 2)))):
        on, ch, distinct, rows = [], [], [], []
        for g, chans in enumerate(sets):
            s0 = 1000 * (g + 1)
            on += [s0 + 2 * k for k in range(len(chans))]
            ch += list(chans)
            distinct.append(len(chans))
            rows.append([s0 + 2 * chans.index(c) if c in chans else -1 for c in range(C)])
        # one channel several times: five records, two channels; the last record of a channel wins, also when it
        # is the smaller sample
        s0 = 1000 * (len(sets) + 1)
        on += [s0 + 40, s0 + 30, s0 + 20, s0 + 5, s0 + 25]
        ch += [0, 1, 1, 0, 1]
        distinct.append(2)
        rows.append([s0 + 5, s0 + 25] + [-1] * (C - 2))
        for mc in sorted(set(range(0, max(distinct) + 2)) | {C + 1}):
            out.append(_case(f"minch-C{C}-mc{mc}", on, ch, C, 100, mc, distinct=tuple(distinct),
                             rows=np.array(rows, i64)))
    return out


PATTERN_NG = (255, 256, 257, 513)
PATTERNS = {
    "all": lambda g: True,
    "none": lambda g: False,
    "g%4==3": lambda g: g % 4 == 3,                 # the groups whose keep flag wave 3 decides
    "g>=256": lambda g: g >= 256,                   # nothing in the first scan tile
    "g in (255,256)": lambda g: g in (255, 256),    # the last of tile 0 and the first of tile 1
    "alternating": lambda g: g % 2 == 0,
    "scan-wave-3": lambda g: g % WG >= 3 * WAVE,    # only the last wave of every scan tile holds kept groups
}


def pattern_case(ng, pattern, cap_groups=None):
    """ng groups of min_channels = 3 records each, 1000 samples apart: channels (0, 1, 2) are kept, (0, 0, 1) fail
    min_channels."""
    kept = [bool(PATTERNS[pattern](g)) for g in range(ng)]
    on = [1000 * g + k for g in range(ng) for k in range(3)]
    ch = [c for g in range(ng) for c in ((0, 1, 2) if kept[g] else (0, 0, 1))]
    tag = "" if cap_groups is None else f"-cap{cap_groups}"
    return _case(f"pattern-ng{ng}-{pattern}{tag}", on, ch, 4, 100, 3, cap_groups=cap_groups, ng=ng, pattern=pattern,
                 kept=tuple(kept))


CAP_PATTERN = (257, "alternating")   # 129 kept groups
CAP_KEPT = 129


def _pattern_cases():
    out = [pattern_case(ng, p) for ng in PATTERN_NG for p in PATTERNS]
    out += [pattern_case(*CAP_PATTERN, cap_groups=c) for c in (1, CAP_KEPT, CAP_KEPT - 1, CAP_KEPT + 1)]
    return out


GROUP_TABLE = tuple(_length_cases() + _distance_cases() + _close_cases() + _min_channel_cases() + _pattern_cases())


def multi_clip_case():
    """Nine clips of one call: counts 0, 1, cap, cap + 5 (clamped) and mixed, different data per clip, every slot of
    every clip filled with valid records (a missing clamp to the count changes the groups), junk in the clip field,
    and a cap_groups below the kept groups of the full clips."""
    cap, C, md, mc = 40, 5, 50, 2
    counts = np.array([0, 1, cap, cap + 5, 17, 0, cap, 3, 29], i64)
    rec = np.zeros((len(counts), cap), ONSET)
    lens = (3, 5, 1, 4, 2, 6, 1, 3, 7, 2, 5, 4, 3)
    for k in range(len(counts)):
        rot = lens[k:] + lens[:k]
        on, ch = by_lengths(rot, md, C, k % 2 == 1, base=1000 * k - 3000)
        rec["sample"][k], rec["channel"][k] = on[:cap], ch[:cap]
        rec["clip"][k] = (0x7FFFFFFF, -5, 123456, -2 ** 31)[k % 4]
    return NS(name="multi-clip", records=rec, counts=counts, cap=cap, C=C, md=md, mc=mc, cc=None, cap_groups=6)


def singleton_clips_case():
    """Forty full clips in which every record is a group of its own and is kept: each clip fills all cap + 1 anchor
    slots and all cap keep slots of its work space, next to a neighbour that does the same."""
    n_clips, cap = 40, 8
    rec = np.zeros((n_clips, cap), ONSET)
    rec["sample"] = 1000 * np.arange(cap)[None, :] + 7 * np.arange(n_clips)[:, None]
    rec["channel"] = (np.arange(cap)[None, :] + np.arange(n_clips)[:, None]) % 3
    rec["clip"] = -1
    return NS(name="singleton-clips", records=rec, counts=np.full(n_clips, cap, i64), cap=cap, C=3, md=100, mc=1,
              cc=None, cap_groups=cap)


def multi_clip_ref(m, cc=None):
    n = np.minimum(m.counts, m.cap)
    return [groups_ref(m.records["sample"][k, :n[k]], m.records["channel"][k, :n[k]], m.C, m.md, m.mc, cc)
            for k in range(len(n))]


def table_as_batch():
    """Every row of GROUP_TABLE as one clip of a single call: records [n, cap] padded to the longest list with valid
    records behind the count, and the counts."""
    cap = max(len(c.onsets) for c in GROUP_TABLE)
    rec = np.zeros((len(GROUP_TABLE), cap), ONSET)
    rec["channel"], rec["sample"] = 1, 123
    for k, c in enumerate(GROUP_TABLE):
        rec["sample"][k, :len(c.onsets)], rec["channel"][k, :len(c.onsets)] = c.onsets, c.channels
        rec["clip"][k] = k
    return rec, np.array([len(c.onsets) for c in GROUP_TABLE], i64)


BATCH_PARAMS = ((200, 100, 2, None), (200, 0, 1, 64), (200, 1000, 3, None))  # (C, max_distance, min_channels, close)


# ---- 2. k_group_offsets -----------------------------------------------------------------------------------------

def offsets_ref(n_groups, cap_groups):
    return np.concatenate([[0], np.cumsum(np.minimum(np.asarray(n_groups, i64), cap_groups))]).astype(i64)


def _offset_cases():
    out = []
    for n_clips in (1, 2, 255, 256, 257, 600):
        cap_groups = 3
        ng = np.array([(0, 2, 3, 7, 1, 3, 0, 4)[(k + n_clips) % 8] for k in range(n_clips)], i64)
        if n_clips == 1:
            ng[0] = 7
        out.append(NS(name=f"offsets-{n_clips}", n_clips=n_clips, cap_groups=cap_groups, n_groups=ng))
    return out


OFFSET_CASES = tuple(_offset_cases())


# ---- 3. k_group_windows -----------------------------------------------------------------------------------------

WINDOW_SHAPES = ((1, 1), (3, 85), (4, 256), (64, 5), (257, 3), (300, 1))
ROW_KINDS = ("inside", "before_0", "past_end", "outside_left", "outside_right", "minus_1", "min_first", "min_last")


def window_row(kind, C, width, n_samples, pre, g):
    """One row of onsets whose windows have the named position in a clip of n_samples."""
    spread = np.array([(c * 5 + g) % 7 for c in range(C)], i64)  # 0..6; channel (-g / 5 mod 7) holds the minimum
    if kind in ("inside", "min_first", "min_last", "min_high", "minus_1"):
        base = pre + max(0, (n_samples - width - 7 - pre) // 2)
    elif kind == "before_0":
        base = pre - 1 - 2 * spread                               # row = pre - 1 - spread: every start in [-7, -1]
    elif kind == "past_end":                                      # at least one column past the end, and, where the
        spread = spread % max(width - 1, 1)                       # width allows, one inside (width 1: at n_samples)
        base = n_samples - width + 1 + pre
    elif kind == "outside_left":
        base = pre - width - 7
    else:
        assert kind == "outside_right"
        base = n_samples + pre
    row = base + spread
    if kind == "min_first":
        row[0] = row.min() - 1
    if kind == "min_last":
        row[C - 1] = row.min() - 1
    if kind == "min_high":
        row[270] = row.min() - 1
    if kind == "minus_1":
        row[(g + C // 2) % C] = -1
    return row


def window_starts(row, pre, use_min):
    return (np.full(len(row), row.min()) if use_min else np.asarray(row)) - pre


def _window_cases():
    out = []
    rng = np.random.default_rng(20)
    for C, width in WINDOW_SHAPES:
        for short in (False, True):
            if short and (C, width) not in ((3, 85), (4, 256)):
                continue
            n_samples = (40 if width == 85 else 1) if short else 2 * width + 50
            pre = 4 if width > 1 else 1
            kinds = list(ROW_KINDS) + (["min_high"] if C == 300 else [])
            n_clips, cap_groups = 3, len(kinds)
            groups = np.full((n_clips, cap_groups, C), -7, i64)
            for k in range(n_clips):
                for g in range(cap_groups):
                    groups[k, g] = window_row(kinds[(g + k) % len(kinds)], C, width, n_samples, pre, g + k)
            n_groups = np.array([cap_groups, 0, cap_groups + 2], i64) if not short else \
                np.array([2, cap_groups, 3], i64)
            x = rng.standard_normal((n_clips, n_samples, C)).astype(f32)
            out.append(NS(name=f"windows-C{C}-w{width}" + ("-short" if short else ""), C=C, width=width,
                          n_samples=n_samples, pre=pre, x=x, groups=groups, n_groups=n_groups, cap_groups=cap_groups,
                          kinds=tuple(kinds)))
    # more (clip, row) pairs than the grid cap: the grid-stride loop
    n_clips, cap_groups, C, width, n_samples, pre = 70, 64, 2, 4, 60, 2
    groups = np.zeros((n_clips, cap_groups, C), i64)
    for k in range(n_clips):
        for g in range(cap_groups):
            groups[k, g] = ((7 * k + 3 * g) % 62 - 1, (5 * k + 11 * g) % 62 - 1)   # -1 .. 60: every position
    n_groups = np.array([(64, 0, 13, 70, 1, 63, 64, 40)[k % 8] for k in range(n_clips)], i64)
    n_groups[-1] = 64
    x = rng.standard_normal((n_clips, n_samples, C)).astype(f32)
    out.append(NS(name="windows-past-the-grid", C=C, width=width, n_samples=n_samples, pre=pre, x=x, groups=groups,
                  n_groups=n_groups, cap_groups=cap_groups, kinds=()))
    return out


WINDOW_CASES = tuple(_window_cases())


def windows_ref(w, use_min, cap_total=None):
    """(offsets [n_clips + 1], rows [min(total, cap_total), C, width])."""
    n = np.minimum(w.n_groups, w.cap_groups)
    rows = [group_windows(w.x[k], w.groups[k, :n[k]], w.width, w.pre, use_min) for k in range(len(n)) if n[k]]
    rows = np.concatenate(rows) if rows else np.zeros((0, w.C, w.width), f32)
    return offsets_ref(w.n_groups, w.cap_groups), rows if cap_total is None else rows[:cap_total]


def offset_windows(c):
    """An OFFSET_CASES row as the smallest window call: one channel, windows of one sample."""
    n_samples = 8
    groups = ((np.arange(c.n_clips)[:, None] * 3 + np.arange(c.cap_groups)[None, :]) % n_samples).astype(i64)
    x = (np.arange(c.n_clips * n_samples, dtype=f32) + 1).reshape(c.n_clips, n_samples, 1)
    return NS(name=c.name, C=1, width=1, n_samples=n_samples, pre=0, x=x, groups=groups[:, :, None].copy(),
              n_groups=c.n_groups, cap_groups=c.cap_groups, kinds=())


def window_cap_totals(w):
    """cap_total equal to the total, 0, and cutting the rows of the last clip that has at least two in two."""
    off = offsets_ref(w.n_groups, w.cap_groups)
    k = max(k for k in range(len(w.n_groups)) if off[k + 1] - off[k] >= 2)
    return int(off[-1]), 0, int(off[k]) + 1


# ---- 4. k_pack_records ------------------------------------------------------------------------------------------

def pack_ref(records, counts, cap, cap_total, clip_offset):
    """include/onsetfp.h: record 0 is {clip 0, channel = some count > cap, sample = sum(min(count, cap))}; the
    records follow in clip order with clip_offset added to their clip ids; rows that do not fit cap_total are
    dropped.  Returns the 1 + min(total, cap_total) rows that are written.  counts >= 0."""
    counts = np.asarray(counts, i64)
    assert (counts >= 0).all()
    c = np.minimum(counts, cap)
    head = np.zeros(1, ONSET)
    head["channel"], head["sample"] = int((counts > cap).any()), int(c.sum())
    if cap == 0:
        return head
    body = records[np.arange(cap)[None, :] < c[:, None]].copy()   # row-major: clip order, then record order
    body["clip"] += i32(clip_offset)
    return np.concatenate([head, body[:cap_total]])


def _pack_cases():
    out = []
    rng = np.random.default_rng(21)
    shapes = ((1, 16, 0, False), (1, 1, 7, True), (2, 16, -3, True), (2, 0, 7, False), (255, 1, 7, False),
              (255, 16, 0, True), (256, 16, -3, False), (256, 0, 0, True), (257, 1, 0, True), (257, 16, 7, False),
              (1500, 16, 7, True), (1500, 1, -3, False), (1500, 0, -3, False), (65535, 1, 0, False))
    for n_clips, cap, off, over in shapes:
        counts = rng.integers(0, cap + 1, n_clips).astype(i64)
        if n_clips > 2:
            counts[0], counts[1], counts[-1] = cap, 0, cap
        if over:
            counts[n_clips // 2] = cap + 2
        rec = None
        if cap:
            rec = np.zeros((n_clips, cap), ONSET)
            rec["clip"] = np.arange(n_clips)[:, None]
            rec["channel"] = rng.integers(0, 8, (n_clips, cap))
            rec["sample"] = rng.integers(-2 ** 40, 2 ** 40, (n_clips, cap))
        out.append(NS(name=f"pack-{n_clips}x{cap}-off{off}" + ("-over" if over else ""), n_clips=n_clips, cap=cap,
                      counts=counts, records=rec, clip_offset=off, over=over))
    return out


PACK_CASES = tuple(_pack_cases())


def pack_total(p):
    return int(np.minimum(p.counts, p.cap).sum())


def pack_cap_totals(p):
    t = pack_total(p)
    return sorted({0, max(t - 1, 0), t, t + 3})


# ---- 5. k_lfilter -----------------------------------------------------------------------------------------------

def lfilter_ref(x, b, a, zi):
    """(y, final zi) of scipy.signal.lfilter along axis 0, all float32; zi [order][C] (empty for order 0)."""
    from scipy.signal import lfilter
    y, zf = lfilter(np.asarray(b, f32), np.asarray(a, f32), np.asarray(x, f32), axis=0, zi=np.asarray(zi, f32))
    assert y.dtype == f32 and zf.dtype == f32 and zf.shape == np.shape(zi)
    return y, zf


def stable_ba(order, rng):
    """float32 (b, a) with a[0] = 1 and every pole within 0.8 of the origin."""
    roots = []
    for _ in range(order // 2):
        r, th = rng.uniform(0.3, 0.8), rng.uniform(0.2, 2.9)
        roots += [r * np.exp(1j * th), r * np.exp(-1j * th)]
    if order % 2:
        roots.append(rng.uniform(-0.8, 0.8))
    a = np.real(np.poly(roots)) if roots else np.ones(1)
    return rng.uniform(-1, 1, order + 1).astype(f32), a.astype(f32)


LFILTER_CHANNELS = (1, 63, 64, 65, 130)
LFILTER_LENGTHS = (1, 2, 257)


def _lfilter_cases():
    out = []
    rng = np.random.default_rng(22)
    for order in range(9):
        b, a = stable_ba(order, rng)
        C, n = LFILTER_CHANNELS[order % 5], LFILTER_LENGTHS[order % 3]
        out.append(NS(name=f"lfilter-order{order}-C{C}-n{n}", order=order, C=C, n=n, b=b, a=a, split=None,
                      x=rng.standard_normal((n, C)).astype(f32), zi=np.zeros((order, C), f32)))
        # a[0] = 2 (normalised in fp32), a state that is not zero, and the stream cut in two calls
        C = LFILTER_CHANNELS[(order + 2) % 5]
        out.append(NS(name=f"lfilter-order{order}-C{C}-a0=2-split", order=order, C=C, n=257, b=b * f32(2),
                      a=a * f32(2), split=100, x=rng.standard_normal((257, C)).astype(f32),
                      zi=rng.standard_normal((order, C)).astype(f32)))
    b, a = stable_ba(2, rng)
    x = rng.standard_normal((64, 3)).astype(f32)
    clean = x.copy()
    x[5, 1], x[20, 1] = np.inf, np.nan
    out.append(NS(name="lfilter-inf-nan", order=2, C=3, n=64, b=b, a=a, split=None, x=x, clean=clean, special=1,
                  zi=np.zeros((2, 3), f32)))
    return out


LFILTER_CASES = tuple(_lfilter_cases())


# ---- 6. legacy symbols ------------------------------------------------------------------------------------------

LEGACY_CHANNELS = (1, 63, 64, 65, 200)
LEGACY_LENGTHS = (1, 64)


def _follower_cases():
    out = []
    rng = np.random.default_rng(23)
    for C in LEGACY_CHANNELS:
        for n in LEGACY_LENGTHS:
            # y holds the previous call's output: row 0 continues from its LAST row, the other rows are never read
            out.append(NS(name=f"ar-C{C}-n{n}", kind="ar", C=C, n=n, x=rng.uniform(-70, 0, (n, C)).astype(f32),
                          y0=rng.uniform(-70, 0, (n, C)).astype(f32), attack=f32(1 / 3.0), release=f32(1 / 383.0)))
            am, aM, mm = ((1e-4, 1e-5, 2.0), (1e-2, 3e-3, 0.0))[(C + n) % 2]
            out.append(NS(name=f"minmax-C{C}-n{n}", kind="minmax", C=C, n=n,
                          x=rng.uniform(0, 30, (n, C)).astype(f32), mn0=rng.uniform(0, 3, C).astype(f32),
                          mx0=rng.uniform(5, 15, C).astype(f32), alpha_min=f32(am), alpha_max=f32(aM), minmin=f32(mm)))
    return out


def ar_ref(c):
    y = c.y0.copy()
    ar_envelope(c.x, y, c.attack, c.release)
    return y


def minmax_ref(c):
    mn, mx = c.mn0.copy(), c.mx0.copy()
    minmax_envelope(c.x, mn, mx, c.alpha_min, c.alpha_max, c.minmin)
    return mn, mx


def _backtrack_cases():
    """buffer [N][C], newest row last.  monotone: every row above the one before, so the walk only stops at the
    start of the buffer (i + 1 < N) and every delta ends at B + 1 - N; falling: nothing moves; tol: steps of 1
    in the newest rows and of 2^-20 before them, so the tolerance stops the walk on the way."""
    out = []
    N, B = 48, 16
    alpha = f32(2 / (5 + 1))
    rng = np.random.default_rng(24)
    for n_onsets, C in ((1, 1), (64, 3), (65, 8), (130, 3)):
        t = np.arange(N, dtype=np.float64)[:, None] + np.arange(C)[None, :] / 8
        bufs = {"monotone": (t * 0.5, 0.0), "falling": (-t * 0.5, 0.0),
                "tol": (np.where(t >= N - 24, t - (N - 24), (t - (N - 24)) * 2.0 ** -20), 0.01)}
        for kind, (buf, tol) in bufs.items():
            out.append(NS(name=f"backtrack-{kind}-n{n_onsets}-C{C}", kind=kind, N=N, B=B, C=C, n_onsets=n_onsets,
                          buffer=np.ascontiguousarray(buf, f32), channels=rng.integers(0, C, n_onsets).astype(i64),
                          deltas0=rng.integers(0, B, n_onsets).astype(i64), alpha=alpha, tol=f32(tol)))
    return out


def backtrack_ref(c):
    d = c.deltas0.copy()
    backtrack_onsets(c.buffer, c.channels, d, c.alpha, c.tol, c.B)
    return d


LEGACY_CASES = tuple(_follower_cases() + _backtrack_cases())
