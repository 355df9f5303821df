// Device functions of the hit locator shared by ofp_locate.hip (the batched entry points), the replay kernel
// and the per-hop graph (ofp_hop.hip): the legality search, the section filter, the rules of trilaterate, and
// Multilaterate3D.locate (reference multilateration.py:428-575) together with the planar Multilaterate.locate
// (:677-733) as ONE state machine run by ONE workgroup on a state held in LDS.
//
// loc_feed<PLANAR> is the reference's locate, line by line (the host versions in multilateration.py are its models);
// what the planar routine leaves out stands under `if constexpr (PLANAR)`, so each kind is compiled without a test
// of the other.  The bookkeeping is done by thread 0; every thread follows the same control flow on the same LDS
// values, so the three parallel parts are reached by the whole workgroup: the lag x sample products of the
// correlation (one lag per lane), the is_legal_3d scan (first-hit reduction) and the section filter.  hybrj runs on
// one lane in fp64.  Static bounds: groups <= OFP_LOCS_GROUPS, members <= OFP_LOCS_MEMBERS, lags <= 2 *
// LOC_ONSET_TOL, section rows <= the caller's max_section, hybrj's maxfev.
#pragma once
#include <cmath>

#include "ofp_common.h"
#include "ofp_hybrj.h"
#include "ofp_mlp.h"
#include "ofp_xcorr_dev.h"

namespace ofp {

// is_legal_3d (multilateration.py:413-426) for one group, by the whole workgroup; every thread gets the result.
// Returns the first legal flat index (row * side + col) or -1.  smin: one slot per thread.
__device__ inline int64_t first_legal(const float* __restrict__ maps, int S, int side, int s0, int s1, int s2,
                                      double lag1, double lag2, double tol, int64_t* smin) {
    const int64_t cells = (int64_t)side * side;
    const float* m1 = maps + ((int64_t)s0 * S + s1) * cells;
    const float* m2 = maps + ((int64_t)s0 * S + s2) * cells;
    const double hi1 = lag1 + tol, lo1 = lag1 - tol, hi2 = lag2 + tol, lo2 = lag2 - tol;
    int64_t best = cells;
    for (int64_t k = threadIdx.x; k < cells; k += blockDim.x) {
        const double a = (double)m1[k], b = (double)m2[k];
        if (a < hi1 && a > lo1 && b < hi2 && b > lo2) {
            best = k;  // k only grows within a thread: the first hit is this thread's minimum
            break;
        }
    }
    smin[threadIdx.x] = best;
    __syncthreads();
    for (int s = blockDim.x / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s && smin[threadIdx.x + s] < smin[threadIdx.x]) smin[threadIdx.x] = smin[threadIdx.x + s];
        __syncthreads();
    }
    const int64_t r = smin[0];
    __syncthreads();
    return r < cells ? r : -1;
}

// first_legal's index as np.unravel_index(.., "F") returns it for a square map: (column, row), and (0, 0) for -1.
// The reference takes (0, 0) for "no cell", so a hit in that very cell counts as none.
struct LocCell {
    int64_t ix, iy;
    __device__ bool none() const { return ix == 0 && iy == 0; }
    // trilaterate's initial guess: np.array(res) - self.radius
    __device__ void guess(double radius, double* g) const {
        g[0] = (double)ix - radius;
        g[1] = (double)iy - radius;
    }
};

__device__ __forceinline__ LocCell loc_cell(int64_t k, int side) {
    return LocCell{k < 0 ? 0 : k % side, k < 0 ? 0 : k / side};
}

// Multilaterate3D.trilaterate's reordering (multilateration.py:542-544): a group whose second sensor is sensor 1 is
// solved as (origin, 0, 1) with the two later onsets exchanged.  The planar class has no such step.
__device__ __forceinline__ void loc_reorder_3d(int32_t* sens, int64_t* on) {
    if (sens[1] == 1) {
        sens[1] = 0;
        sens[2] = 1;
        const int64_t t = on[1];
        on[1] = on[2];
        on[2] = t;
    }
}

// trilaterate's system for a group (origin, a, b).  The two classes form the path differences in another order of
// operations, and they round differently: lag / sr * c (Multilaterate3D, :563-564), lag * c / sr (Multilaterate,
// :724-725).
__device__ __forceinline__ hybrj::Tdoa loc_tdoa(const double* __restrict__ sensors, const int32_t* sens,
                                                const int64_t* on, double sr, double c, bool planar) {
    hybrj::Tdoa t;
    for (int q = 0; q < 3; ++q) {
        t.o[q] = sensors[3 * sens[0] + q];
        t.a[q] = sensors[3 * sens[1] + q];
        t.b[q] = sensors[3 * sens[2] + q];
    }
    const double da = (double)(on[1] - on[0]), db = (double)(on[2] - on[0]);
    t.dda = planar ? da * c / sr : da / sr * c;
    t.ddb = planar ? db * c / sr : db / sr * c;
    return t;
}

__device__ __forceinline__ float med5(const float* in) {
    float v[5];
    for (int i = 0; i < 5; ++i) {  // insertion sort of five finite samples
        const float x = in[i];
        int j = i;
        while (j > 0 && v[j - 1] > x) {
            v[j] = v[j - 1];
            --j;
        }
        v[j] = x;
    }
    return v[2];
}

// Value t (0 <= t < n - 1) of locate's cross-correlation input (multilateration.py:466-476) over n rows of one
// channel: median filter of size 5 ('reflect': d c b a | a b c d | d c b a) along time, first difference,
// non-negative values zeroed, absolute value.  at(u): row u of the channel, 0 <= u < n.
template <class At>
__device__ __forceinline__ float section_value(At&& at, int64_t n, int64_t t) {
    float md[2];
    for (int q = 0; q < 2; ++q) {
        float w[5];
        for (int k = 0; k < 5; ++k) {
            int64_t u = t + q + k - 2;
            if (u < 0) u = -u - 1;
            if (u >= n) u = 2 * n - u - 1;
            w[k] = at(u);
        }
        md[q] = med5(w);
    }
    float d = md[1] - md[0];
    if (d >= 0.0f) d = 0.0f;
    return fabsf(d);
}

// ---- locate ------------------------------------------------------------------------------------------------

constexpr int LOC_ONSET_TOL = 50;    // multilateration.py: ONSET_TOL
constexpr int LOC_NORM_CUTOFF = 10;  // NORM_CUTOFF
constexpr int LOC_LOOKAROUND = LOC_ONSET_TOL + LOC_NORM_CUTOFF;
constexpr int LOC_MAX_SECTION = 4096;  // ofp_xcorr_lag's longest row

struct LocTables {
    const double* sensors;
    int S;
    const float* maps;
    const float* mn;
    const float* mx;
    int side;
    double spc, sr, c, radius, xtol;
    int maxfev;
    int use_audio;
    int max_section;
    int planar;    // 1: the 2-D Multilaterate (loc_feed<true>), sensors with z = 0; never with use_audio or a network
    MlpPlan plan;  // n_layers == 0: hybrj
};

// One group outside the lists (the extended group of a call, and the located one)
struct LocGroup {
    int32_t len, pad;
    int32_t sens[OFP_LOCS_MEMBERS];
    int64_t on[OFP_LOCS_MEMBERS];
};

// The workgroup's LDS.  Fixed part first; the section rows and the network's tiles follow it.
struct LocLds {
    ofp_locate_state st[2];  // `ongoing` and new_groups, swapped after every call
    LocGroup ext;
    double mml[64];          // max_max_lags
    double res[2];
    int64_t mv[2];           // adjust_onset's moves
    float cc[2 * LOC_ONSET_TOL + 4];
    float red[2][16];
    int32_t found;           // the solve's verdict
    int32_t kept;            // groups left by remove_seed (a word of its own: `found` is still being read)
    int32_t cur;             // which of st[] is `ongoing`
    int32_t pad;
};

__host__ __device__ inline size_t loc_lds_bytes(int nthreads, int max_section, const MlpPlan& plan, size_t extra = 0) {
    size_t b = (sizeof(LocLds) + 15) & ~(size_t)15;
    b += (size_t)nthreads * 8;                            // first_legal's slots
    b += (size_t)2 * ((max_section + 3) & ~3) * 4;        // the two section rows
    if (plan.n_layers > 0) b += (size_t)16 * (plan.st_a + plan.st_b) * 4;
    return b + extra + 16;  // extra: bytes a caller keeps behind all this (LocView::extra)
}

struct LocView {
    LocLds* L;
    int64_t* smin;
    float* xs;
    float* ys;
    float* ta;
    float* tb;
    float* extra;  // behind the last tile: the caller's own rows (the hop of csrc/ofp_hop.hip)
};

__device__ inline LocView loc_carve(unsigned char* smem, int nthreads, int max_section, const MlpPlan& plan) {
    LocView v;
    unsigned char* p = reinterpret_cast<unsigned char*>((reinterpret_cast<uintptr_t>(smem) + 15) & ~(uintptr_t)15);
    v.L = reinterpret_cast<LocLds*>(p);
    p += (sizeof(LocLds) + 15) & ~(size_t)15;
    v.smin = reinterpret_cast<int64_t*>(p);
    p += (size_t)nthreads * 8;
    const int ms = (max_section + 3) & ~3;
    v.xs = reinterpret_cast<float*>(p);
    v.ys = v.xs + ms;
    v.ta = v.ys + ms;
    v.tb = v.ta + (plan.n_layers > 0 ? 16 * plan.st_a : 0);
    v.extra = v.tb + (plan.n_layers > 0 ? 16 * plan.st_b : 0);
    return v;
}

// `ongoing` from device memory into LDS (whole workgroup; g == NULL: an empty one) and the tables' max_max_lags
__device__ inline void loc_load(const LocTables& T, const LocView& v, const ofp_locate_state* g) {
    const int tid = threadIdx.x, nt = blockDim.x;
    const int32_t* src = reinterpret_cast<const int32_t*>(g);
    int32_t* dst = reinterpret_cast<int32_t*>(&v.L->st[0]);
    for (int i = tid; i < (int)(sizeof(ofp_locate_state) / 4); i += nt) dst[i] = g ? src[i] : 0;
    for (int s = tid; s < T.S; s += nt) {  // np.nanmax over the sensor's pairs (NaN when it has none)
        double m = __builtin_nan("");
        for (int j = 0; j < T.S; ++j) {
            const double x = (double)T.mx[s * T.S + j];
            if (x == x && !(m >= x)) m = x;
        }
        v.L->mml[s] = m;
    }
    if (tid == 0) v.L->cur = 0;
    __syncthreads();
}

__device__ inline void loc_store(const LocView& v, ofp_locate_state* g) {
    const int tid = threadIdx.x, nt = blockDim.x;
    __syncthreads();
    const int32_t* src = reinterpret_cast<const int32_t*>(&v.L->st[v.L->cur]);
    int32_t* dst = reinterpret_cast<int32_t*>(g);
    for (int i = tid; i < (int)(sizeof(ofp_locate_state) / 4); i += nt) dst[i] = src[i];
}

__device__ __forceinline__ void loc_copy_group(ofp_locate_state* dst, int di, const int32_t* sens, const int64_t* on,
                                               int len, int alias) {
    dst->len[di] = len;
    dst->alias[di] = alias;
    for (int k = 0; k < OFP_LOCS_MEMBERS; ++k) {
        dst->sensors[di][k] = k < len ? sens[k] : 0;
        dst->onsets[di][k] = k < len ? on[k] : 0;
    }
}

// The lists of one call: `ongoing` as the call found it, and new_groups with its length and the sticky flags.  Every
// thread holds the same values.
struct LocCall {
    ofp_locate_state* cur;
    ofp_locate_state* nxt;
    int nn;     // len(new_groups)
    int flags;
};

// new_groups.append(group): returns the entry's index, or -1 with OFP_LOCF_GROUPS set when the list is full
__device__ __forceinline__ int loc_append(LocCall& c, const int32_t* sens, const int64_t* on, int len, int alias) {
    if (c.nn >= OFP_LOCS_GROUPS) {
        c.flags |= OFP_LOCF_GROUPS;
        return -1;
    }
    if (threadIdx.x == 0) loc_copy_group(c.nxt, c.nn, sens, on, len, alias);
    return c.nn++;
}

// self.ongoing = new_groups
__device__ __forceinline__ void loc_publish(LocLds& L, const LocCall& c) {
    __syncthreads();
    if (threadIdx.x == 0) {
        c.nxt->n_groups = c.nn;
        c.nxt->flags = c.flags;
        L.cur ^= 1;
    }
    __syncthreads();
}

// group = (group[0] + [sensor], group[1] + [onset]), into L.ext
__device__ __forceinline__ void loc_extend(LocLds& L, const ofp_locate_state* cur, int src, int len, int sensor,
                                           int64_t onset) {
    __syncthreads();
    if (threadIdx.x == 0) {
        L.ext.len = len + 1;
        for (int k = 0; k < len; ++k) {
            L.ext.sens[k] = cur->sensors[src][k];
            L.ext.on[k] = cur->onsets[src][k];
        }
        L.ext.sens[len] = sensor;
        L.ext.on[len] = onset;
    }
    __syncthreads();
}

// Multilaterate3D.locate's cross-correlation refinement (multilateration.py:452-497) of the lag between the group's
// first onset o0 (sensor s0; entry src of `ongoing`) and the new one: the section rows rec_audio[-i - 1:] of the two
// channels through section_value, cross_correlation_lag over the window around the current lag, adjust_onset.
// Moves o0 in place -- in `ongoing`, and in the copy new_groups holds when the entry is an alias (my_prev >= 0) --
// and `onset`, and replaces `lag`; leaves all three alone when the window is empty.  A section the LDS rows cannot
// hold sets OFP_LOCF_SECTION.
template <class Audio>
__device__ __forceinline__ void loc_cc_adjust(const LocTables& T, const LocView& v, LocCall& c, Audio&& audio,
                                              int64_t counter, bool zero_pad, int src, int my_prev, int s0, int sensor,
                                              int64_t& o0, int64_t& onset, int64_t& lag) {
    LocLds& L = *v.L;
    const int tid = threadIdx.x, nt = blockDim.x;
    const int64_t want = counter - o0 + LOC_LOOKAROUND + 1;
    int64_t start = counter - want;
    if (!zero_pad && start < 0) start = 0;
    const int64_t n64 = counter - start;
    if (n64 < 3 || n64 > T.max_section) {
        c.flags |= OFP_LOCF_SECTION;
        return;
    }
    const int n = (int)n64, m = n - 1;
    float mx = -INFINITY, my = -INFINITY;
    for (int i = tid; i < 2 * m; i += nt) {
        const int which = i >= m, t = which ? i - m : i;
        const int col = which ? sensor : s0;
        const float d = section_value([&](int64_t u) { return audio(start + u, col); }, n, t);
        if (which) {
            v.ys[t] = d;
            my = fmaxf(my, d);
        } else {
            v.xs[t] = d;
            mx = fmaxf(mx, d);
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        mx = fmaxf(mx, __shfl_xor(mx, o));
        my = fmaxf(my, __shfl_xor(my, o));
    }
    if ((tid & 63) == 0) {
        L.red[0][tid >> 6] = mx;
        L.red[1][tid >> 6] = my;
    }
    __syncthreads();
    for (int w = 0; w < (nt + 63) / 64; ++w) {
        mx = w ? fmaxf(mx, L.red[0][w]) : L.red[0][0];
        my = w ? fmaxf(my, L.red[1][w]) : L.red[1][0];
    }
    // cross_correlation_lag(x, y, onsets=(first, new), d=0, onset_tolerance, normalization_cutoff)
    const int current = (int)(onset - o0);
    int lo, hi;
    py_slice(m - current - LOC_ONSET_TOL, m - current + LOC_ONSET_TOL, 2 * m - 1, &lo, &hi);
    if (hi > lo) {
        for (int j = lo + tid; j < hi; j += nt) L.cc[j - lo] = cc_entry(v.xs, v.ys, m, LOC_NORM_CUTOFF, j);
        __syncthreads();
        int am = 0;  // np.argmax: the first maximum
        float bv = L.cc[0];
        for (int j = 1; j < hi - lo; ++j) {
            if (L.cc[j] > bv) {
                bv = L.cc[j];
                am = j;
            }
        }
        const int new_lag = -(am - (current + LOC_ONSET_TOL));
        if (tid < XCORR_WAVE) {
            int64_t ca = 0, cb = 0;
            adjust_onset_wave(v.xs, v.ys, m, LOC_LOOKAROUND, current + LOC_LOOKAROUND, new_lag, mx, my, tid, &ca, &cb);
            if (tid == 0) {
                L.mv[0] = (int32_t)ca;
                L.mv[1] = (int32_t)cb;
            }
        }
        __syncthreads();
        lag = new_lag;
        o0 += L.mv[0];
        onset += L.mv[1];
        if (tid == 0) {
            c.cur->onsets[src][0] = o0;
            if (my_prev >= 0) c.nxt->onsets[my_prev][0] = o0;
        }
    }
    __syncthreads();
}

// trilaterate for the three-member group in L.ext from the cell the search found: the root into L.res and the
// return value 1 (every thread), or 0.  3-D: its reordering first (:536-575), then the network's output * 100 when
// there is one, else hybrj on lane 0; planar (:714-733): hybrj on the group as it stands.
template <bool PLANAR>
__device__ __forceinline__ int loc_solve(const LocTables& T, const LocView& v, const LocCell& cell) {
    LocLds& L = *v.L;
    const int tid = threadIdx.x;
    if constexpr (!PLANAR) {
        if (tid == 0) {
            loc_reorder_3d(L.ext.sens, L.ext.on);
            L.found = 0;
        }
        __syncthreads();
    }
    if (!PLANAR && T.plan.n_layers > 0) {  // self.model.call_np((d_a1, d_b1)) * 100: a float32 product
        if (tid < 64) {
            for (int i = tid; i < 16 * T.plan.st_a; i += 64) v.ta[i] = 0.0f;
            ofp_wave_lds_sync();
            if (tid == 0) {
                v.ta[0] = (float)(L.ext.on[1] - L.ext.on[0]);
                v.ta[1] = (float)(L.ext.on[2] - L.ext.on[0]);
            }
            ofp_wave_lds_sync();
            ofp_mlp_tile(T.plan, T.plan.params, v.ta, v.tb, tid, [&](int r, int col, float val) {
                if (r == 0 && col < 2) L.res[col] = (double)(val * 100.0f);
            });
            if (tid == 0) L.found = 1;
        }
    } else if (tid == 0) {
        const hybrj::Tdoa t = loc_tdoa(T.sensors, L.ext.sens, L.ext.on, T.sr, T.c, PLANAR);
        double guess[2];
        cell.guess(T.radius, guess);
        const hybrj::Result r = hybrj::solve(t, guess, T.xtol, T.maxfev);
        L.res[0] = r.x[0];
        L.res[1] = r.x[1];
        L.found = r.info == 1 ? 1 : 0;
    }
    __syncthreads();
    return L.found;
}

// remove_seed(new_groups, group) for the group in L.ext (3-D only)
__device__ __forceinline__ void loc_remove_seed(LocLds& L, LocCall& c) {
    if (threadIdx.x == 0) {
        ofp_locate_state* nxt = c.nxt;
        int w = 0;
        for (int q = 0; q < c.nn; ++q) {
            if (nxt->sensors[q][0] == L.ext.sens[0] && nxt->onsets[q][0] == L.ext.on[0]) continue;
            if (w != q) loc_copy_group(nxt, w, nxt->sensors[q], nxt->onsets[q], nxt->len[q], nxt->alias[q]);
            ++w;
        }
        L.kept = w;
    }
    __syncthreads();
    c.nn = L.kept;
}

// One call of locate by the whole workgroup: Multilaterate3D.locate(sensor, onset, rec_audio), or with PLANAR the
// 2-D Multilaterate.locate(sensor, onset), which reads no audio (counter, zero_pad and audio are then unused).
// audio(t, col): sample t of the stream (start <= t < counter); zero_pad: a section that starts before sample 0 keeps
// its length (rows there are what audio returns) instead of being cut at row 0.  Returns 1 when a position was
// returned (xy: the Cartesian root in cm), else 0; `located` (LDS, may be NULL) receives the group as trilaterate left
// it.  Every thread returns the same values.
template <bool PLANAR, class Audio>
__device__ inline int loc_feed(const LocTables& T, const LocView& v, int sensor, int64_t onset, int64_t counter,
                               bool zero_pad, Audio&& audio, double* xy, LocGroup* located) {
    LocLds& L = *v.L;
    const int tid = threadIdx.x;
    LocCall c{&L.st[L.cur], &L.st[L.cur ^ 1], 0, L.st[L.cur].flags};
    ofp_locate_state* cur = c.cur;
    const int n_cur = cur->n_groups;
    int prev_out = -1;   // where the previous iteration appended its (unextended) group object
    int found = 0;
    bool returned = false;
    __syncthreads();
    for (int gi = 0; gi < n_cur && !returned; ++gi) {
        // an alias entry is the same Python object as the entry before it: it shares that entry's storage.  (The
        // planar routine changes nothing in place, so there the mark only records that two entries are one object.)
        const bool alias = gi > 0 && cur->alias[gi] != 0;
        const int src = alias ? gi - 1 : gi;
        const int my_prev = alias ? prev_out : -1;
        prev_out = -1;
        const int len = cur->len[src];
        int s0 = cur->sensors[src][0];
        int64_t o0 = cur->onsets[src][0];
        int64_t lag = onset - o0;
        if constexpr (!PLANAR) {  // planar: no skip at the top of the loop: a group past its largest lag is still tried
            if ((double)lag > L.mml[s0]) continue;
        }
        if constexpr (!PLANAR) {  // planar: no swap: a negative lag goes to is_legal as it is
            if (lag < 0) {  // an adjustment moved an onset behind this one: swap them
                __syncthreads();
                if (tid == 0) {
                    cur->sensors[src][0] = sensor;
                    cur->onsets[src][0] = onset;
                    if (my_prev >= 0) {
                        c.nxt->sensors[my_prev][0] = sensor;
                        c.nxt->onsets[my_prev][0] = onset;
                    }
                }
                const int ts = s0;
                const int64_t to = o0;
                s0 = sensor;
                o0 = onset;
                sensor = ts;
                onset = to;
                lag = -lag;
                __syncthreads();
            }
        }
        bool in_group = false;
        for (int k = 0; k < len; ++k) in_group = in_group || cur->sensors[src][k] == sensor;
        bool extended = false;
        if (!in_group) {
            if constexpr (!PLANAR) {  // planar: no cross-correlation step: locate takes no recording
                if (T.use_audio)
                    loc_cc_adjust(T, v, c, audio, counter, zero_pad, src, my_prev, s0, sensor, o0, onset, lag);
            }
            const double dl = (double)lag;
            const bool legal = (double)T.mn[s0 * T.S + sensor] < dl && dl < (double)T.mx[s0 * T.S + sensor];
            if (legal && len >= OFP_LOCS_MEMBERS) {
                c.flags |= OFP_LOCF_MEMBERS;
            } else if (legal) {
                loc_extend(L, cur, src, len, sensor, onset);
                extended = true;
                if (len + 1 == 3) {  // (planar groups grow beyond three members; only this one is searched)
                    if constexpr (!PLANAR) {  // planar: no break on equal first sensors: without a swap there are none
                        if (L.ext.sens[0] == L.ext.sens[1]) break;
                    }
                    const LocCell cell = loc_cell(
                        first_legal(T.maps, T.S, T.side, L.ext.sens[0], L.ext.sens[1], L.ext.sens[2],
                                    (double)(L.ext.on[1] - L.ext.on[0]), (double)(L.ext.on[2] - L.ext.on[0]), 1 * T.spc,
                                    v.smin),
                        T.side);
                    if (!cell.none()) {
                        // planar: no reordering, and deltas formed as lag * c / sr (loc_solve, loc_tdoa)
                        found = loc_solve<PLANAR>(T, v, cell);
                        if (found) {
                            if constexpr (!PLANAR) loc_remove_seed(L, c);  // planar: no remove_seed in its locate
                            xy[0] = L.res[0];
                            xy[1] = L.res[1];
                        }
                        if (located && tid == 0) *located = L.ext;
                        // self.ongoing = new_groups; return res -- in both kinds a found cell ends the call whether
                        // or not the solve succeeds
                        returned = true;
                        continue;
                    }
                }
                loc_append(c, L.ext.sens, L.ext.on, L.ext.len, 0);
            }
        }
        // not past the largest possible lag: keep the group (the test sees the extended group, which is appended a
        // second time)
        if ((double)lag <= L.mml[s0]) {
            if (extended) loc_append(c, L.ext.sens, L.ext.on, L.ext.len, 1);
            else prev_out = loc_append(c, cur->sensors[src], cur->onsets[src], len, my_prev >= 0 ? 1 : 0);
        }
        __syncthreads();
    }
    if (!returned) {  // new_groups.append(([sensor_index], [onset_index]))
        const int32_t s1[1] = {sensor};
        const int64_t o1[1] = {onset};
        loc_append(c, s1, o1, 1, 0);
    }
    loc_publish(L, c);
    return found;
}

// One call of locate of the tables' kind: the 3-D or the planar instantiation.  T.planar is the same for every thread
// and every call of a launch.
template <class Audio>
__device__ __forceinline__ int loc_feed_kind(const LocTables& T, const LocView& v, int sensor, int64_t onset,
                                             int64_t counter, bool zero_pad, Audio&& audio, double* xy,
                                             LocGroup* located) {
    return T.planar ? loc_feed<true>(T, v, sensor, onset, counter, zero_pad, audio, xy, located)
                    : loc_feed<false>(T, v, sensor, onset, counter, zero_pad, audio, xy, located);
}

}  // namespace ofp

// the launch form of a locator's tables, checked (ofp_locate.hip); `who` names the entry point in the error text
int ofp_locate_tables(const ofp_hop_locator* loc, const char* who, ofp::LocTables* out);
// the same for the planar kind: use_audio and max_section are ignored, a network is refused
int ofp_locate_tables_2d(const ofp_hop_locator* loc, const char* who, ofp::LocTables* out);
