"""The detector's layout guards, stated a second time, and the table of calls that stands on both sides of each.

`make_layout` (csrc/ofp_detect.hip) picks the kernel variants of a call from its geometry; every variant flag is a
conjunction, and the fast kernel behind it relies on each conjunct.  `restate_plan` states the same decisions in plain
Python, one conjunct per line, from what the kernels say they assume -- NOT from the C++ expression: a conjunct lost on one
side must show as a difference from the other (tests/test_detect_geometry_cpu.py compares them through the plan query,
ofp_detect_plan_for, without a GPU).

ROWS holds, for every flag and every conjunct of it, an `on` row (the flag set) and an `off` row (that conjunct false, and
as few of the others as arithmetic allows).  Conjuncts are tied by the geometry -- n_w % 32 != 0 with n_wb % 32 == 0 makes
V or U odd too -- so a row records every conjunct of its flag that fails (`fails`), and the CPU test recomputes that set.
A conjunct that no geometry can make fail on its own account is listed in IMPLIED with the reason; the CPU sweep checks the
reason.  A new guard in make_layout therefore needs: its line in restate_plan (or the query differs), and an on row and an
off row here (or the coverage test fails).

The rows were found by `python tests/detect_geometry_cases.py` (a search over (C, B, N, warm, tuning) that prints, for a
conjunct, the calls failing the fewest others) and are frozen below as literals."""
import numpy as np

SR = 48000

# The three tunings of the table (lane_merge=1: the occupancy terms of the guards drop out, the rest is geometry).
# LINES: the line forms are the subject; PLAIN: line_stores left to the layout; SLOW: every fast form switched off.
CHUNKS = dict(hp_chunk=4096, ar_chunk=2048, mm_chunk=1024)
LINES = dict(CHUNKS, lane_merge=1, line_stores=1)
PLAIN = dict(CHUNKS, lane_merge=1)
SLOW = dict(CHUNKS, lane_merge=1, line_stores=-1, interleaved=-1, walk_through=-1, scan_skip=-1, fuse_db_sums=-1)
TUNINGS = dict(LINES=LINES, PLAIN=PLAIN, SLOW=SLOW)

# tuning fields whose negative value selects the slow twin of a fast form (the results must not change)
TWINS = ("line_stores", "interleaved", "walk_through", "scan_skip", "fuse_db_sums")

GEOMETRY = ("n_w", "n_wb", "Nm", "U", "V", "Nv")
NUMBERS = ("hp_L", "hp_S", "hp_R", "hp_span", "ar_L", "ar_S", "mm_L", "mm_S", "tu")
BITS = ("sm_seg", "merge", "hp_early", "hp_staged", "hp_spread", "hp_lines", "ar_sym", "ar_through", "ar_lines", "db_sym",
        "mm_il", "mm_through", "ar_il", "use_sum")


def cdiv(a, b):
    return -(-a // b)


def round_up(a, b):
    return cdiv(a, b) * b


def f32(v):
    return float(np.float32(v))


def _doubled(L, cap, too_many):
    """L doubled while it is below `cap` and too_many(L) holds (elementwise)."""
    L = np.asarray(L, np.int64)
    going = np.ones(L.shape, bool)
    for _ in range(8):
        going = going & (L < cap) & too_many(L)
        L = np.where(going, 2 * L, L)
    return L


def _span(user, W, L, n_chunks, ns_per_step, share, chains):
    """Chunks one speculative warm-up run walks through: the largest of 1, 2, 4, 8, 16 (no more than there are chunks)
    whose estimated launch time -- the longer of the dependent walk and the bytes read at 3 TB/s -- is within 10 % of the
    best estimate."""
    n_chunks = np.maximum(n_chunks, 1)
    if user > 0:
        return np.minimum(user, n_chunks)
    est = {}
    for s in (1, 2, 4, 8, 16):
        walk = (W + (s - 1) * L).astype(np.float64)
        est[s] = np.maximum(walk * ns_per_step * 1e-9,
                            float(share) * float(chains) * cdiv(n_chunks, s).astype(np.float64) * walk * 4.0 / 3.0e12)
    best = np.minimum.reduce(list(est.values()))
    S = np.ones_like(n_chunks)
    for s in (1, 2, 4, 8, 16):
        S = np.where((est[s] <= 1.10 * best) & (s <= n_chunks), s, S)
    return S


def restate_plan(params, tuning, n_cus, n_clips, N, warm, rel, rel_aligned):
    """-> (plan, conjuncts): the plan as the query reports it (GEOMETRY + NUMBERS + BITS), and for every guarded flag the
    dict {conjunct name: holds}; the flag is set when all hold.

    params: BatchDetector's arguments as a dict (n_signals, block_size and whatever differs from its defaults);
    tuning: ofp_detect_tuning fields (missing: 0); rel: the call asks for `rel`; rel_aligned: at a 16-byte boundary.
    N, warm and block_size may be integer arrays of one shape (the sweep of the CPU test): every value is then an array
    (`&` and `|` stand for `and` and `or` throughout)."""
    t = lambda k: int(tuning.get(k, 0))  # noqa: E731
    scalar = np.ndim(N) == 0 and np.ndim(warm) == 0 and np.ndim(params["block_size"]) == 0
    N, warm, B = np.broadcast_arrays(np.asarray(N, np.int64), np.asarray(warm, np.int64),
                                     np.asarray(params["block_size"], np.int64))
    C = int(params["n_signals"])
    fast_ar, slow_ar = params.get("fast_ar", (3.0, 383.0)), params.get("slow_ar", (2205.0, 2205.0))
    high_pass = params.get("hipass_freq", 2000.0) != 0
    manual = bool(np.all(np.asarray(params.get("on_threshold", 0.5)) > 1))
    cooldown = int(params.get("cooldown", 1323))

    # --- the streams of one clip.  The warm-up plays x[0:n_w] through the high-pass; followers and tracker take whole
    # blocks only, so they see n_wb of those samples; then everything restarts at x[0] for the Nm samples of whole blocks.
    n_w = np.maximum(0, np.minimum(warm, N))
    n_wb = n_w - n_w % B
    Nm = N - N % B
    V = n_w + Nm    # high-pass stream
    U = n_wb + Nm   # follower / tracker stream
    Nv = round_up(n_w + N, 4)  # the planar input copy of one series, in whole 16-byte groups
    nb = Nm // B
    chains = n_clips * C

    # --- chunk lengths: the caller's, or grown from the latency defaults until the launch fits the device's share
    share = max(1, t("concurrent_calls"))
    cus = max(1, n_cus // share)
    two_waves_per_simd = 2 * 4 * 64 * cus
    hpL, hpR = np.full(N.shape, 8192), np.full(N.shape, 16)
    if t("hp_chunk") <= 0 and t("hp_candidates") <= 0:
        hpR = np.where(chains * cdiv(V, hpL) * hpR > two_waves_per_simd, 8, hpR)  # (fewer leave too many chain breaks)
        hpL = _doubled(hpL, 131072, lambda L: chains * cdiv(V, L) * hpR > two_waves_per_simd)
    arL = _doubled(np.full(N.shape, 4096), 32768, lambda L: chains * cdiv(U, L) > 3 * 64 * cus)
    mmL = _doubled(np.full(N.shape, 4096), 32768, lambda L: chains * cdiv(U, L) > two_waves_per_simd)
    hp_L = np.full(N.shape, t("hp_chunk")) if t("hp_chunk") > 0 else hpL
    ar_L = np.full(N.shape, t("ar_chunk")) if t("ar_chunk") > 0 else arL
    mm_L = np.full(N.shape, t("mm_chunk")) if t("mm_chunk") > 0 else mmL
    warm_of = lambda user, dflt: user if user > 0 else (0 if user < 0 else dflt)  # noqa: E731
    hp_W = warm_of(t("hp_warm"), 40960)
    hp_R = np.maximum(1, np.minimum(16, t("hp_candidates") if t("hp_candidates") > 0 else hpR))
    hp_chunks = np.maximum(1, cdiv(V, hp_L))
    ar_chunks = np.maximum(1, cdiv(U, ar_L))
    mm_chunks = np.maximum(1, cdiv(U, mm_L))

    # --- IIR candidates: a run walks through 1, 2 or 4 chunks; throughput-bound launches share a warm-up between two,
    # or take the staged form, where every chunk has its own candidates again
    more_than_a_wave_per_simd = chains * cdiv(V, hp_L) * hp_R > 64 * 4 * cus
    hp_span = np.where(hp_R % t("hp_span") == 0, t("hp_span"), 1) if t("hp_span") in (2, 4) else np.ones_like(N)
    if t("hp_span") <= 0:
        hp_span = np.where((hp_R % 2 == 0) & more_than_a_wave_per_simd, 2, hp_span)
    hp_staged = (t("hp_dedupe") > 0) | ((t("hp_dedupe") == 0 and t("hp_span") <= 0 and t("concurrent_calls") >= 2)
                                        & more_than_a_wave_per_simd)
    hp_staged = hp_staged & (hp_W >= 8192) & (hp_R >= 2)
    hp_span = np.where(hp_staged, 1, hp_span)
    # sub-chunks: four when each is a whole number of waves' steps (64), about 4096 samples each in long chunks
    hp_S = np.where(hp_L % 256 == 0, 4, 1)
    hp_S = np.where((hp_L >= 32768) & (hp_L % 1024 == 0), np.minimum(16, hp_L // 4096), hp_S)
    hp_spread = (cdiv(chains * hp_chunks * (hp_R // hp_span), 256) <= n_cus) & (t("concurrent_calls") <= 1)

    # --- followers: closed-form guess when the slow follower is symmetric; its exact warm-up is 11 slow / 24 fast time
    # constants, rounded to whole chunks (the guess exists at chunk boundaries)
    fa, fr, sa, sr_ = f32(1 / fast_ar[0]), f32(1 / fast_ar[1]), f32(1 / slow_ar[0]), f32(1 / slow_ar[1])
    symmetric = sa == sr_ and 0 < sa < 1
    ar_sym = False if t("ar_guess") == 1 else symmetric
    cmin = min(fa, fr, sa, sr_)
    tau = 1.0 / cmin if cmin > 0 else 1.0
    ar_W = np.full(N.shape, warm_of(t("ar_warm"), round_up(int(min(10.0 * tau, 4.0e6)), 1024)))
    if ar_sym:
        cf = min(fa, fr)
        tau_s, tau_f = 1.0 / sa, (1.0 / cf if cf > 0 else 1.0)
        ar_W = round_up(warm_of(t("ar_warm"), round_up(int(min(max(11.0 * tau_s, 24.0 * tau_f), 4.0e6)), 1024)), ar_L)
    mm_W = np.full(N.shape, warm_of(t("mm_warm"), 49152))
    merge = t("lane_merge") > 0 or (t("lane_merge") == 0 and t("concurrent_calls") >= 2)
    ar_S = _span(t("ar_span"), ar_W, ar_L, ar_chunks, 16.0, share, chains) if ar_sym else np.ones_like(N)
    mm_S = _span(t("mm_span"), mm_W, mm_L, mm_chunks, 11.0, share, chains)
    tu = max(1, min(256, 8192 // C))  # time steps per transpose tile: at most 8192 floats of LDS

    holds = lambda cs: np.logical_and.reduce([np.broadcast_to(v, N.shape) for v in cs.values()])  # noqa: E731
    conj = {}
    # k_hp_run_lines: a lane hands over batches of 32 outputs.  A batch must lie inside ONE region of the high-pass
    # stream -- warm-up rows [0, n_wb), the dropped gap [n_wb, n_w), the rest [n_w, V) -- so both borders and the end
    # are batch borders; its image in the follower stream ends at a batch border (U); a chunk and a sub-chunk start at
    # one; the source series is whole 16-byte groups.
    conj["hp_lines"] = {
        "line_stores>=0": t("line_stores") >= 0,
        "throughput": merge | (t("line_stores") > 0) | (chains * hp_chunks * hp_S >= 2 * 64 * 4 * n_cus),
        "n_w%32": n_w % 32 == 0,
        "n_wb%32": n_wb % 32 == 0,
        "V%32": V % 32 == 0,
        "U%32": U % 32 == 0,
        "Nv%4": Nv % 4 == 0,
        "hp_L%32": hp_L % 32 == 0,
        "sub%32": (hp_L // hp_S) % 32 == 0,
        "hp_L%hp_S": hp_L % hp_S == 0,
    }
    # k_ar_warm_both: one lane per chunk (merge) that starts from the closed-form guess (ar_sym); input and output are
    # walked in 16-byte groups, so the stream and every chunk start are multiples of 4
    conj["ar_through"] = {
        "walk_through>=0": t("walk_through") >= 0,
        "merge": merge,
        "ar_sym": ar_sym,
        "U%4": U % 4 == 0,
        "ar_L%4": ar_L % 4 == 0,
    }
    ar_through = holds(conj["ar_through"])
    # walk_lines for the followers: batches of 32 from every chunk start to the end of the stream
    conj["ar_lines"] = {
        "line_stores>=0": t("line_stores") >= 0,
        "throughput": ar_through | (t("line_stores") > 0) | (chains * ar_chunks >= 32 * 4 * n_cus),
        "U%32": U % 32 == 0,
        "ar_L%32": ar_L % 32 == 0,
    }
    # k_rect_db_sym: the sums of the closed-form guess per chunk, formed from the high-pass output in 16-byte groups
    conj["db_sym"] = {
        "fuse_db_sums>=0": t("fuse_db_sums") >= 0,
        "ar_sym": ar_sym,
        "high_pass": high_pass,
        "U%4": U % 4 == 0,
        "ar_L%4": ar_L % 4 == 0,
    }
    # the *_il kernels read the caller's `rel`: it must exist, the thresholds must be relative (the tracker runs), and the
    # kernels are instantiated for 4, 8 and 64 channels; interleaved -1 and its alias 2 switch them off
    conj["mm_il"] = {
        "interleaved on": t("interleaved") >= 0 and t("interleaved") != 2,
        "merge": merge,
        "rel": bool(rel),
        "relative thresholds": not manual,
        "C in 4,8,64": C in (4, 8, 64),
    }
    mm_il = holds(conj["mm_il"])
    conj["mm_through"] = {"mm_il": mm_il, "walk_through>=0": t("walk_through") >= 0}
    ar_lines = holds(conj["ar_lines"])
    # walk_lines_to<C>: every chunk is written by a line walk (ar_lines, ar_through), read by the *_il kernels (mm_il),
    # C is 4 or 8; a batch of 32 rows lies on one side of the warm-up / main split (n_wb) and the main part ends at a batch
    # border (Nm); k_rel_out_il wants whole blocks of at least one 16-byte group per lane (64 lanes: 256 floats); and the
    # 16-byte stores need an aligned `rel`
    conj["ar_il"] = {
        "ar_lines": ar_lines,
        "ar_through": ar_through,
        "mm_il": mm_il,
        "C in 4,8": C in (4, 8),
        "n_wb%32": n_wb % 32 == 0,
        "Nm%32": Nm % 32 == 0,
        "B*C>=256": B * C >= 256,
        "rel aligned": bool(rel_aligned) or not rel,
    }
    # k_rel_out's 16-byte path on every tile (stream, tile, both parts of `rel` and a tile's rows in whole groups), a group
    # of four rows inside one block, and blocks long enough for the extremes to pay
    conj["use_sum"] = {
        "scan_skip>=0": t("scan_skip") >= 0,
        "U%4": U % 4 == 0,
        "tu%4": tu % 4 == 0,
        "n_wb*C%4": (n_wb * C) % 4 == 0,
        "tu*C%4": (tu * C) % 4 == 0,
        "Nm*C%4": (Nm * C) % 4 == 0,
        "B%4": B % 4 == 0,
        "B>=32": B >= 32,
    }
    conj["hp_early"] = {"sub-chunks": hp_S > 1,
                        "wanted": (t("hp_early") > 0) | ((t("hp_early") == 0) & (hp_L // hp_S >= 4096))}
    # k_sm_seg: segments of 256 visited blocks; long clips, or forced
    conj["sm_seg"] = {
        "sm_segments>=0": t("sm_segments") >= 0,
        "C<=64": C <= 64,
        "cooldown<2^30": cooldown < (1 << 30),
        "B<2^30": B < (1 << 30),
        "long or forced": (nb >= 16384) | (t("sm_segments") > 0),
        "nb>256": nb > 256,
    }
    plan = dict(n_w=n_w, n_wb=n_wb, Nm=Nm, U=U, V=V, Nv=Nv, hp_L=hp_L, hp_S=hp_S, hp_R=hp_R, hp_span=hp_span, ar_L=ar_L,
                ar_S=ar_S, mm_L=mm_L, mm_S=mm_S, tu=tu, merge=merge, hp_staged=hp_staged, hp_spread=hp_spread, ar_sym=ar_sym)
    for flag, cs in conj.items():
        plan[flag] = holds(cs)
    plan = {k: np.broadcast_to(np.asarray(v, np.int64), N.shape) for k, v in plan.items()}
    conj = {flag: {k: np.broadcast_to(np.asarray(v, bool), N.shape) for k, v in cs.items()} for flag, cs in conj.items()}
    if scalar:
        plan = {k: int(v) for k, v in plan.items()}
        conj = {flag: {k: bool(v) for k, v in cs.items()} for flag, cs in conj.items()}
    return plan, conj


# Conjuncts that cannot fail while the others of their flag hold, and why (the CPU sweep asserts the implication):
IMPLIED = {
    ("hp_lines", "Nv%4"): "Nv is rounded up to a multiple of 4",
    ("hp_lines", "hp_L%hp_S"): "hp_S is 4 only when 256 divides hp_L, more only when 1024 does",
    ("hp_lines", "sub%32"): "hp_S > 1 only when 64 * hp_S divides hp_L; with hp_S = 1 it is hp_L%32",
    ("ar_il", "n_wb%32"): "n_wb = U - Nm, and U%32 (in ar_lines) and Nm%32 hold: any one of the three follows from the other "
                          "two, so dropping this conjunct alone changes no plan (il_n_wb is the row where it fails with Nm%32)",
    ("use_sum", "tu*C%4"): "a multiple of 4 times C (tu%4 fails with it otherwise)",
    ("sm_seg", "C<=64"): "out of the table's range (C <= 64)",
    ("sm_seg", "cooldown<2^30"): "out of the table's range (clips of at most 60 000 samples)",
    ("sm_seg", "B<2^30"): "block_size is at most 2^20",
}


def params_of(row):
    return dict(row.get("kw", {}), n_signals=row["C"], block_size=row["B"], sr=SR)


def restate_row(row, n_cus=256):
    return restate_plan(params_of(row), row["tuning"], n_cus, row.get("clips", 1), row["N"], row["warm"],
                        row.get("rel", True), row.get("rel_off", 0) == 0)


def failing(row, n_cus=256):
    """The conjuncts of the row's subject flag that do not hold."""
    _, conj = restate_row(row, n_cus)
    if row["flag"] is None:
        return []
    return sorted(k for k, v in conj[row["flag"]].items() if not v)


def make_input(row):
    """[clips][N][C] float32: drum hits every 0.11 s (37 samples apart from channel to channel), so every region of the
    stream -- the blocks next to the warm-up included -- holds onsets."""
    from onset_fingerprinting_amd import synth
    N, C = row["N"], row["C"]
    secs = N / SR + 0.25
    return np.stack([synth.drum_hits(C, secs, SR, seed=row.get("seed", 7) + i, period=0.11)[:N]
                     for i in range(row.get("clips", 1))])


def R(name, flag, conjunct, side, fails, C, B, N, warm, tuning, **extra):
    """A row: `flag` / `conjunct` is its subject, side "on" (flag set) or "off" (conjunct false), fails: every conjunct of
    the flag that is false.  extra: clips, rel (False: not requested), rel_off / x_off (floats the `rel` / `x` arrays
    start off a 16-byte boundary), kw (detector arguments), seed."""
    return dict(extra, name=name, flag=flag, conjunct=conjunct, side=side, fails=sorted(fails), C=C, B=B, N=N, warm=warm,
                tuning=tuning)


def T(base, **kw):
    return dict(base, **kw)


MANUAL = dict(on_threshold=6.0, off_threshold=4.0)
ASYM = dict(slow_ar=(1500.0, 3000.0))
NO_HP = dict(hipass_freq=0.0)

ROWS = [
    # ROWS-BEGIN
    # --- the historical shape at its smallest: blocks of 100, a warm-up that is no whole number of blocks.  U and V are
    # multiples of 32, n_w and n_wb are not: the 32 outputs of the gap [n_wb, n_w) go nowhere
    R("hist_4132", "hp_lines", "n_wb%32", "off", ["n_w%32", "n_wb%32"], 4, 100, 47937, 4132, LINES),
    R("hist_4128", "hp_lines", None, "off", ["n_wb%32", "V%32"], 4, 100, 47937, 4128, LINES),
    R("hist_4100", "hp_lines", None, "off", ["n_w%32", "n_wb%32"], 4, 100, 47937, 4100, LINES),
    # --- hp_lines
    R("hpl_on", "hp_lines", None, "on", [], 4, 64, 48000, 4096, LINES),
    R("hpl_on_3clips", "hp_lines", None, "on", [], 4, 64, 19200, 4096, LINES, clips=3),
    R("hpl_n_w_by4", "hp_lines", "n_w%32", "off", ["n_w%32", "V%32"], 4, 64, 48000, 4100, LINES),
    R("hpl_n_w_by1", "hp_lines", "n_w%32", "off", ["n_w%32", "V%32"], 4, 64, 48000, 4097, LINES),
    R("hpl_n_wb_by4", "hp_lines", "n_wb%32", "off", ["n_wb%32", "U%32"], 4, 100, 48000, 4128, LINES),
    R("hpl_n_wb_by1", "hp_lines", "n_wb%32", "off", ["n_wb%32", "U%32"], 4, 33, 47520, 1120, LINES),
    R("hpl_VU_by4", "hp_lines", "V%32", "off", ["V%32", "U%32"], 4, 100, 47937, 3200, LINES),
    R("hpl_VU_by1", "hp_lines", "U%32", "off", ["V%32", "U%32"], 4, 33, 47560, 1056, LINES),
    R("hpl_chunk_4128", "hp_lines", None, "on", [], 4, 64, 48000, 4096, T(LINES, hp_chunk=4128)),
    R("hpl_chunk_4100", "hp_lines", "hp_L%32", "off", ["hp_L%32", "sub%32"], 4, 64, 48000, 4096, T(LINES, hp_chunk=4100)),
    R("hpl_chunk_4004", "hp_lines", "hp_L%32", "off", ["hp_L%32", "sub%32"], 4, 64, 48000, 4096, T(LINES, hp_chunk=4004)),
    R("hpl_gap_32", "hp_lines", None, "on", [], 4, 96, 48000, 4160, LINES),
    R("hpl_gap_64", "hp_lines", None, "on", [], 4, 96, 48000, 4192, LINES),
    R("hpl_gap_31", "hp_lines", None, "off", ["n_w%32", "V%32"], 4, 96, 48000, 4159, LINES),
    R("hpl_tuned_off", "hp_lines", "line_stores>=0", "off", ["line_stores>=0"], 4, 64, 48000, 4096, T(LINES, line_stores=-1)),
    R("hpl_latency", "hp_lines", "throughput", "off", ["throughput"], 4, 64, 48000, 4096, T(CHUNKS, lane_merge=-1)),
    # --- warm-up lengths (B = 64): none, inside the first block, whole blocks, a block and a batch, the whole clip
    R("warm_0", "hp_lines", None, "on", [], 4, 64, 48000, 0, LINES),
    R("warm_1", "hp_lines", None, "off", ["n_w%32", "V%32"], 4, 64, 48000, 1, LINES),
    R("warm_31", "hp_lines", None, "off", ["n_w%32", "V%32"], 4, 64, 48000, 31, LINES),
    R("warm_32", "hp_lines", None, "on", [], 4, 64, 48000, 32, LINES),
    R("warm_33", "hp_lines", None, "off", ["n_w%32", "V%32"], 4, 64, 48000, 33, LINES),
    R("warm_B-1", "hp_lines", None, "off", ["n_w%32", "V%32"], 4, 64, 48000, 63, LINES),
    R("warm_B", "hp_lines", None, "on", [], 4, 64, 48000, 64, LINES),
    R("warm_B+1", "hp_lines", None, "off", ["n_w%32", "V%32"], 4, 64, 48000, 65, LINES),
    R("warm_3B+32", "hp_lines", None, "on", [], 4, 64, 48000, 224, LINES),
    R("warm_N", "hp_lines", None, "on", [], 4, 64, 24000, 24000, LINES),
    R("warm_N+1", "hp_lines", None, "off", ["n_w%32", "V%32"], 4, 64, 24001, 24002, LINES),
    # --- ar_through and db_sym: 16-byte groups of the follower stream (blocks of 30: U is even, a multiple of 4 for an
    # even number of blocks), an asymmetric slow follower, no high-pass
    R("art_on", "ar_through", None, "on", [], 4, 30, 48000, 60, PLAIN),
    R("art_U", "ar_through", "U%4", "off", ["U%4"], 4, 30, 48000, 30, PLAIN),
    R("art_L", "ar_through", "ar_L%4", "off", ["ar_L%4"], 4, 30, 48000, 60, T(PLAIN, ar_chunk=2050)),
    R("art_L_on", "ar_through", None, "on", [], 4, 30, 48000, 60, T(PLAIN, ar_chunk=2052)),
    R("art_asym", "ar_through", "ar_sym", "off", ["ar_sym"], 4, 64, 48000, 4096, PLAIN, kw=ASYM),
    R("art_tuned_off", "ar_through", "walk_through>=0", "off", ["walk_through>=0"], 4, 64, 48000, 4096, T(PLAIN, walk_through=-1)),
    R("art_latency", "ar_through", "merge", "off", ["merge"], 4, 64, 48000, 4096, T(CHUNKS, lane_merge=-1)),
    R("dbs_on", "db_sym", None, "on", [], 4, 30, 48000, 60, PLAIN),
    R("dbs_U", "db_sym", "U%4", "off", ["U%4"], 4, 30, 48000, 30, PLAIN),
    R("dbs_L", "db_sym", "ar_L%4", "off", ["ar_L%4"], 4, 30, 48000, 60, T(PLAIN, ar_chunk=2050)),
    R("dbs_asym", "db_sym", "ar_sym", "off", ["ar_sym"], 4, 64, 48000, 4096, PLAIN, kw=ASYM),
    R("dbs_no_hp", "db_sym", "high_pass", "off", ["high_pass"], 4, 64, 48000, 4096, PLAIN, kw=NO_HP),
    R("dbs_tuned_off", "db_sym", "fuse_db_sums>=0", "off", ["fuse_db_sums>=0"], 4, 64, 48000, 4096, T(PLAIN, fuse_db_sums=-1)),
    # --- ar_lines
    R("arl_on", "ar_lines", None, "on", [], 4, 64, 48000, 4096, LINES),
    R("arl_on_3clips", "ar_lines", None, "on", [], 4, 64, 19200, 4096, LINES, clips=3),
    R("arl_chunk_2080", "ar_lines", None, "on", [], 4, 64, 48000, 4096, T(LINES, ar_chunk=2080)),
    R("arl_chunk_2052", "ar_lines", "ar_L%32", "off", ["ar_L%32"], 4, 64, 48000, 4096, T(LINES, ar_chunk=2052)),
    R("arl_U", "ar_lines", "U%32", "off", ["U%32"], 4, 100, 47937, 3200, LINES),
    R("arl_tuned_off", "ar_lines", "line_stores>=0", "off", ["line_stores>=0"], 4, 64, 48000, 4096, T(LINES, line_stores=-1)),
    R("arl_latency", "ar_lines", "throughput", "off", ["throughput"], 4, 64, 48000, 4096, T(PLAIN, walk_through=-1)),
    # --- ar_il
    R("il_c4", "ar_il", None, "on", [], 4, 64, 48000, 4096, LINES),
    R("il_c8_b32", "ar_il", None, "on", [], 8, 32, 48000, 4096, LINES),
    R("il_c8_b48", "ar_il", None, "on", [], 8, 48, 48000, 96, LINES),
    R("il_c8_b96", "ar_il", None, "on", [], 8, 96, 48000, 4160, LINES),
    R("il_c4_b100", "ar_il", None, "on", [], 4, 100, 48000, 3200, LINES),
    R("il_3clips", "ar_il", None, "on", [], 4, 64, 19200, 4096, LINES, clips=3),
    R("il_c2", "ar_il", None, "off", ["C in 4,8", "mm_il"], 2, 128, 48000, 4096, LINES),
    R("il_c5", "ar_il", None, "off", ["C in 4,8", "mm_il"], 5, 64, 48000, 4096, LINES),
    R("il_c64", "ar_il", "C in 4,8", "off", ["C in 4,8"], 64, 64, 19200, 4096, LINES),
    R("il_n_wb", "ar_il", "n_wb%32", "off", ["n_wb%32", "Nm%32"], 4, 100, 47937, 4132, LINES),
    R("il_n_wb_b48", "ar_il", None, "off", ["n_wb%32", "ar_lines"], 8, 48, 48000, 48, LINES),
    R("il_Nm", "ar_il", "Nm%32", "off", ["Nm%32", "ar_lines"], 8, 48, 48048, 96, LINES),
    R("il_BC_192", "ar_il", "B*C>=256", "off", ["B*C>=256"], 8, 24, 48000, 96, LINES),
    R("il_BC_128", "ar_il", "B*C>=256", "off", ["B*C>=256"], 4, 32, 48000, 4096, LINES),
    R("il_rel_4_bytes_off", "ar_il", "rel aligned", "off", ["rel aligned"], 4, 64, 48000, 4096, LINES, rel_off=1),
    R("il_no_lines", "ar_il", "ar_lines", "off", ["ar_lines"], 4, 64, 48000, 4096, T(LINES, ar_chunk=2052)),
    R("il_no_through", "ar_il", "ar_through", "off", ["ar_through"], 4, 64, 48000, 4096, T(LINES, walk_through=-1)),
    # --- mm_il and mm_through
    R("mm_c4", "mm_il", None, "on", [], 4, 64, 48000, 4096, PLAIN),
    R("mm_c8", "mm_il", None, "on", [], 8, 64, 48000, 4096, PLAIN),
    R("mm_c64", "mm_il", None, "on", [], 64, 64, 19200, 4096, PLAIN),
    R("mm_il_1", "mm_il", None, "on", [], 4, 64, 48000, 4096, T(PLAIN, interleaved=1)),
    R("mm_il_3", "mm_il", None, "on", [], 4, 64, 48000, 4096, T(PLAIN, interleaved=3)),
    R("mm_c1", "mm_il", "C in 4,8,64", "off", ["C in 4,8,64"], 1, 64, 48000, 4096, PLAIN),
    R("mm_c3", "mm_il", "C in 4,8,64", "off", ["C in 4,8,64"], 3, 64, 48000, 4096, PLAIN),
    R("mm_c16", "mm_il", "C in 4,8,64", "off", ["C in 4,8,64"], 16, 64, 48000, 4096, PLAIN),
    R("mm_no_rel", "mm_il", "rel", "off", ["rel"], 4, 64, 48000, 4096, PLAIN, rel=False),
    R("mm_manual", "mm_il", "relative thresholds", "off", ["relative thresholds"], 4, 64, 48000, 4096, PLAIN, kw=MANUAL),
    R("mm_il_-1", "mm_il", "interleaved on", "off", ["interleaved on"], 4, 64, 48000, 4096, T(PLAIN, interleaved=-1)),
    R("mm_il_2", "mm_il", "interleaved on", "off", ["interleaved on"], 4, 64, 48000, 4096, T(PLAIN, interleaved=2)),
    R("mm_latency", "mm_il", "merge", "off", ["merge"], 4, 64, 48000, 4096, T(CHUNKS, lane_merge=-1)),
    R("mmt_on", "mm_through", None, "on", [], 4, 64, 48000, 4096, PLAIN),
    R("mmt_tuned_off", "mm_through", "walk_through>=0", "off", ["walk_through>=0"], 4, 64, 48000, 4096, T(PLAIN, walk_through=-1)),
    # --- use_sum
    R("sum_b32", "use_sum", None, "on", [], 4, 32, 48000, 4096, PLAIN),
    R("sum_b36", "use_sum", None, "on", [], 4, 36, 48000, 4096, PLAIN),
    R("sum_c3", "use_sum", None, "on", [], 3, 32, 48000, 4096, PLAIN),
    R("sum_b20", "use_sum", "B>=32", "off", ["B>=32"], 4, 20, 48000, 4096, PLAIN),
    R("sum_b30", "use_sum", None, "off", ["U%4", "B%4", "B>=32"], 4, 30, 48000, 30, PLAIN),
    R("sum_U", "use_sum", "U%4", "off", ["U%4", "B%4"], 4, 34, 47937, 0, PLAIN),
    R("sum_b34", "use_sum", "B%4", "off", ["B%4"], 4, 34, 47600, 68, PLAIN),
    R("sum_c3_b34", "use_sum", "n_wb*C%4", "off", ["n_wb*C%4", "Nm*C%4", "B%4"], 3, 34, 47634, 34, PLAIN),
    R("sum_c5_b34", "use_sum", "Nm*C%4", "off", ["n_wb*C%4", "Nm*C%4", "B%4"], 5, 34, 47634, 34, PLAIN),
    R("sum_c35", "use_sum", "tu%4", "off", ["tu%4", "tu*C%4"], 35, 32, 19200, 4096, PLAIN),
    R("sum_tuned_off", "use_sum", "scan_skip>=0", "off", ["scan_skip>=0"], 4, 32, 48000, 4096, T(PLAIN, scan_skip=-1)),
    # --- hp_S and hp_early
    R("early_on", "hp_early", None, "on", [], 4, 64, 48000, 4096, T(LINES, hp_chunk=16384)),
    R("early_forced", "hp_early", None, "on", [], 4, 64, 48000, 4096, T(LINES, hp_early=1)),
    R("early_s8", "hp_early", None, "on", [], 4, 64, 48000, 4096, T(LINES, hp_chunk=32768)),
    R("early_short", "hp_early", "wanted", "off", ["wanted"], 4, 64, 48000, 4096, LINES),
    R("early_never", "hp_early", "wanted", "off", ["wanted"], 4, 64, 48000, 4096, T(LINES, hp_chunk=16384, hp_early=-1)),
    R("early_one_sub", "hp_early", "sub-chunks", "off", ["sub-chunks"], 4, 64, 48000, 4096, T(LINES, hp_chunk=4100, hp_early=1)),
    # --- sm_seg
    R("seg_on", "sm_seg", None, "on", [], 4, 32, 48000, 4096, T(PLAIN, sm_segments=1)),
    R("seg_short", "sm_seg", "long or forced", "off", ["long or forced"], 4, 32, 48000, 4096, PLAIN),
    R("seg_few_blocks", "sm_seg", "nb>256", "off", ["nb>256"], 4, 256, 48000, 4096, T(PLAIN, sm_segments=1)),
    R("seg_tuned_off", "sm_seg", "sm_segments>=0", "off", ["sm_segments>=0", "long or forced"], 4, 32, 48000, 4096, T(PLAIN, sm_segments=-1)),
    R("il_no_tracker_il", "ar_il", "mm_il", "off", ["mm_il"], 4, 64, 48000, 4096, T(LINES, interleaved=-1)),
    R("mmt_no_il", "mm_through", "mm_il", "off", ["mm_il"], 4, 64, 48000, 4096, T(PLAIN, interleaved=-1)),
    # --- chunk seams (chunks of 4096 / 2048 / 1024; 8 channels, blocks of 32: every line form and the interleaved stores):
    # the warm-up ends, and the stream ends, at a chunk start, one batch into a chunk, and in the last batch of one
    R("seam_warm_chunk_start", "ar_il", None, "on", [], 8, 32, 45056, 4096, LINES),
    R("seam_warm_one_batch_in", "ar_il", None, "on", [], 8, 32, 45056, 4128, LINES),
    R("seam_warm_last_batch", "ar_il", None, "on", [], 8, 32, 45056, 4064, LINES),
    R("seam_gap_starts_a_chunk", "hp_lines", None, "on", [], 8, 64, 45056, 4128, LINES),
    R("seam_gap_ends_a_chunk", "hp_lines", None, "on", [], 8, 254, 48768, 4096, LINES),
    R("seam_end_one_batch_in", "ar_il", None, "on", [], 8, 32, 45088, 4096, LINES),
    R("seam_end_last_batch", "ar_il", None, "on", [], 8, 32, 45024, 4096, LINES),
    R("seam_one_chunk", "ar_il", None, "on", [], 8, 32, 12288, 4096, T(LINES, hp_chunk=16384, ar_chunk=16384, mm_chunk=16384)),
    R("seam_chunk_and_batch", "ar_il", None, "on", [], 8, 32, 12320, 4096, T(LINES, hp_chunk=16384, ar_chunk=16384, mm_chunk=16384)),
    # --- guards inside kernels (no plan bit).  k_transpose_in's fast path: C and the tile (256 steps) powers of two, a full
    # tile, N * C, n_w and Nv multiples of 4, x 16-byte aligned; k_rel_out's 16-byte path; hp_span's 16-byte stores when
    # input and output positions are congruent (n_w - n_wb and U multiples of 4, see also hpl_n_w_by1, art_U)
    R("tr_c1", None, None, None, [], 1, 64, 48128, 4096, PLAIN),
    R("tr_c2", None, None, None, [], 2, 64, 48128, 4096, PLAIN),
    R("tr_c4", None, None, None, [], 4, 64, 48128, 4096, PLAIN),
    R("tr_c8", None, None, None, [], 8, 64, 48128, 4096, PLAIN),
    R("tr_c3", None, None, None, [], 3, 64, 48128, 4096, PLAIN),
    R("tr_c5", None, None, None, [], 5, 64, 48128, 4096, PLAIN),
    R("tr_c6", None, None, None, [], 6, 64, 48128, 4096, PLAIN),
    R("tr_c1_partial_tile", None, None, None, [], 1, 64, 48000, 4096, PLAIN),
    R("tr_c2_partial_tile", None, None, None, [], 2, 64, 48000, 4096, PLAIN),
    R("tr_c1_NC_odd", None, None, None, [], 1, 64, 48129, 4096, PLAIN),
    R("tr_c2_NC_2mod4", None, None, None, [], 2, 64, 48129, 4096, PLAIN),
    R("tr_c4_n_w_2mod4", None, None, None, [], 4, 64, 48128, 4098, PLAIN),
    R("tr_c4_Nv_1", None, None, None, [], 4, 64, 48129, 4096, PLAIN),
    R("tr_c4_Nv_2", None, None, None, [], 4, 64, 48130, 4096, PLAIN),
    R("tr_c4_Nv_3", None, None, None, [], 4, 64, 48131, 4096, PLAIN),
    R("tr_c8_Nv_3", None, None, None, [], 8, 64, 48131, 4097, PLAIN),
    R("tr_c4_x_4_bytes_off", None, None, None, [], 4, 64, 48128, 4096, PLAIN, x_off=1),
    R("tr_c4_x_8_bytes_off", None, None, None, [], 4, 64, 48128, 4096, PLAIN, x_off=2),
    R("tr_c4_x_12_bytes_off", None, None, None, [], 4, 64, 48128, 4096, PLAIN, x_off=3),
    R("tr_c8_x_4_bytes_off_lines", "hp_lines", None, "on", [], 8, 32, 45056, 4096, LINES, x_off=1),
    R("tr_c4_x_and_rel_off", "ar_il", None, "off", ["rel aligned"], 4, 64, 48128, 4097, LINES, x_off=3, rel_off=1),
    # ROWS-END
]


def by_name():
    return {r["name"]: r for r in ROWS}


# ---------------------------------------------------------------------------
# the search that found the rows
SEARCH_B = np.array(sorted(set(range(8, 131)) | {254, 256}), np.int64)
SEARCH_N = ("40B", "40B+1", "41B-1", 47937, 48000, 47560, 19200)


def search_grid(B=SEARCH_B):
    """(B, warm, N) arrays of small calls around the table's sizes: every block size from 8 to 130, warm-ups on and off
    block and batch borders, lengths that leave Nm on and off a batch border."""
    B = np.asarray(B, np.int64)
    warms = [np.full(B.shape, w) for w in (0, 1, 31, 32, 33, 60, 68, 96, 1056, 1120, 3200, 4096, 4100, 4128, 4132, 4160)]
    warms += [B - 1, B, B + 1, 3 * B + 32]
    Ns = [{"40B": 40 * B, "40B+1": 40 * B + 1, "41B-1": 41 * B - 1}.get(n, np.full(B.shape, n if isinstance(n, int) else 0))
          for n in SEARCH_N]
    Bs, Ws, Nn = [], [], []
    for w in warms:
        for n in Ns:
            Bs.append(B), Ws.append(w), Nn.append(n)
    return np.concatenate(Bs), np.concatenate(Ws), np.concatenate(Nn)


def fewest_failing(row, n_cus=256):
    """Over the search grid, with the row's channels, tuning, detector arguments and `rel`: the smallest number of
    conjuncts of the row's flag that fail when its subject conjunct does (None: it never fails there), and one call
    (B, warm, N) that attains it."""
    B, warm, N = search_grid()
    _, conj = restate_plan(dict(params_of(row), block_size=B), row["tuning"], n_cus, row.get("clips", 1), N, warm,
                           row.get("rel", True), row.get("rel_off", 0) == 0)
    cs = conj[row["flag"]]
    n_fail = sum((~v).astype(np.int64) for v in cs.values())
    where = np.nonzero(~cs[row["conjunct"]])[0]
    if len(where) == 0:
        return None, None
    i = where[np.argmin(n_fail[where])]
    return int(n_fail[i]), dict(B=int(B[i]), warm=int(warm[i]), N=int(N[i]))


# ---------------------------------------------------------------------------
# random geometries (tests/test_gpu_fuzz.py; the CPU test counts their onsets with the oracle alone)
FUZZ_CASES, FUZZ_SEED = 80, 20261020


def random_geometry_case(rng):
    """-> dict(C, B, N, warm (None: the default, half a second), x_off, rel_off, tuning, seed): a clip of 0.5-1.2 s cut to
    a random length, any block size from 8 to 300, warm-ups at the edges, arrays off their 16-byte boundaries."""
    C = int(rng.choice([1, 2, 3, 4, 5, 8]))
    B = int(rng.integers(8, 301))
    if rng.random() < 0.5:
        B = max(8, B // 4 * 4)
    N = int(rng.integers(int(0.5 * SR), int(1.2 * SR) + 1))
    warm = [None, 0, 1, B - 1, B, int(rng.integers(2, 6001)), N, N + 7][int(rng.integers(0, 8))]
    tuning = dict(lane_merge=int(rng.choice([-1, 1])), line_stores=int(rng.choice([-1, 0, 1])),
                  interleaved=int(rng.choice([-1, 0, 1])), walk_through=int(rng.choice([-1, 0])),
                  scan_skip=int(rng.choice([-1, 0])), hp_chunk=int(rng.choice([1024, 4096, 4100, 4128])),
                  ar_chunk=int(rng.choice([1024, 2048, 2052, 2080])), mm_chunk=int(rng.choice([1024, 1999])))
    for k in ("hp_warm", "ar_warm", "mm_warm"):
        if rng.random() < 0.5:
            tuning[k] = -1
    return dict(C=C, B=B, N=N, warm=warm, x_off=int(rng.integers(0, 4)), rel_off=int(rng.integers(0, 2)), tuning=tuning,
                seed=int(rng.integers(1 << 30)))


def fuzz_warm(case):
    return int(0.5 * SR) if case["warm"] is None else case["warm"]


# ---------------------------------------------------------------------------
# running a call on the GPU with arrays that start off a 16-byte boundary
def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_as_oracle(got, want):
    """Bit for bit; a NaN compares as NaN on both sides (the sign and payload of a NaN that arithmetic produces are the
    processor's choice, see tests/test_gpu_rel_il_stores_small.py)."""
    g, w = bits(got), bits(want)
    return got.shape == want.shape and bool(np.all((g == w) | (np.isnan(got) & np.isnan(want))))


def offset_tensor(shape, off, device, dtype):
    """A contiguous tensor of `shape` that starts `off` elements into a flat buffer (allocations are 256-byte aligned)."""
    import torch
    n = int(np.prod(shape))
    flat = torch.empty(n + 4, dtype=dtype, device=device)
    t = flat[off:off + n].view(*shape)
    assert t.data_ptr() % 16 == (4 * off) % 16 and t.is_contiguous()
    return t


def gpu_detect(bd, x, warm, x_off=0, rel_off=0, want_rel=True, fill=None):
    """One call of `bd` on x [clips][N][C] (numpy) -> (records per clip, rel numpy or None, plan of the call, work space).
    fill: byte the work space is filled with before the call."""
    import torch
    from onset_fingerprinting_amd.detection import BatchDetector
    n_clips, N, C = x.shape
    xt = offset_tensor(x.shape, x_off, "cuda", torch.float32)
    xt.copy_(torch.from_numpy(x))
    nb = N // bd.block_size
    cap = max(1, nb * C)
    out = dict(records=torch.empty((n_clips, cap, 16), dtype=torch.uint8, device="cuda"),
               counts=torch.zeros(n_clips, dtype=torch.int64, device="cuda"),
               rel=offset_tensor((n_clips, nb * bd.block_size, C), rel_off, "cuda", torch.float32) if want_rel else None)
    plan = bd.plan(n_clips, N, warm, want_rel, out["rel"])
    ws = bd.reserve(n_clips, N, warm)[:bd.workspace_bytes(n_clips, N, warm)]  # (the reserved array may be a longer one)
    if fill is not None:
        ws.fill_(fill)
    out = bd.detect(xt, warm=warm, want_rel=want_rel, cap_per_clip=cap, out=out)
    recs = BatchDetector.records_to_numpy(out)
    return recs, (out["rel"].cpu().numpy() if want_rel else None), plan, ws


if __name__ == "__main__":
    import sys
    row = dict(flag=sys.argv[1], conjunct=sys.argv[2], C=int(sys.argv[4]) if len(sys.argv) > 4 else 4, B=64,
               tuning=TUNINGS[sys.argv[3] if len(sys.argv) > 3 else "LINES"])
    print(fewest_failing(row))
