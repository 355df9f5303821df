// Device functions of the hit locator shared by ofp_locate.hip (the batched entry points), the replay kernel
// and the per-hop graph (ofp_hop.hip): the legality search, the section filter, and Multilaterate3D.locate
// (reference multilateration.py:428-575) as a state machine run by ONE workgroup on a state held in LDS.
//
// loc_feed is the reference's locate, line by line (the host version in multilateration.py is its model).  The
// bookkeeping is done by thread 0; every thread follows the same control flow on the same LDS values, so the three
// parallel parts are reached by the whole workgroup: the lag x sample products of the correlation (one lag per
// lane), the is_legal_3d scan (first-hit reduction) and the section filter.  hybrj runs on one lane in fp64.
// Static bounds: groups <= OFP_LOCS_GROUPS, members <= OFP_LOCS_MEMBERS, lags <= 2 * LOC_ONSET_TOL, section rows <=
// the caller's max_section, hybrj's maxfev.
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

// ---- Multilaterate3D.locate --------------------------------------------------------------------------------

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
    int planar;    // 1: the 2-D Multilaterate (loc_feed_2d), sensors with z = 0; never with use_audio or a network
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

// One call of locate(sensor, onset, rec_audio) by the whole workgroup.  audio(t, col): sample t of the stream
// (start <= t < counter); zero_pad: a section that starts before sample 0 keeps its length (rows there are what
// audio returns) instead of being cut at row 0.  Returns 1 when a position was returned (xy), else 0; `located`
// (LDS, may be NULL) receives the group as trilaterate left it.  Every thread returns the same values.
template <class Audio>
__device__ inline int loc_feed(const LocTables& T, const LocView& v, int sensor, int64_t onset, int64_t counter,
                               bool zero_pad, Audio&& audio, double* xy, LocGroup* located) {
    LocLds& L = *v.L;
    const int tid = threadIdx.x, nt = blockDim.x;
    ofp_locate_state* cur = &L.st[L.cur];
    ofp_locate_state* nxt = &L.st[L.cur ^ 1];
    const int n_cur = cur->n_groups;
    int flags = cur->flags;
    int nn = 0;          // len(new_groups)
    int prev_out = -1;   // where the previous iteration appended its (unextended) group object
    int found = 0;
    bool returned = false;
    __syncthreads();
    for (int gi = 0; gi < n_cur && !returned; ++gi) {
        // an alias entry is the same Python object as the entry before it: it shares that entry's storage
        const bool alias = gi > 0 && cur->alias[gi] != 0;
        const int src = alias ? gi - 1 : gi;
        const int my_prev = alias ? prev_out : -1;
        prev_out = -1;
        const int len = cur->len[src];
        int s0 = cur->sensors[src][0];
        int64_t o0 = cur->onsets[src][0];
        int64_t lag = onset - o0;
        if ((double)lag > L.mml[s0]) continue;
        if (lag < 0) {  // an adjustment moved an onset behind this one: swap them
            __syncthreads();
            if (tid == 0) {
                cur->sensors[src][0] = sensor;
                cur->onsets[src][0] = onset;
                if (my_prev >= 0) {
                    nxt->sensors[my_prev][0] = sensor;
                    nxt->onsets[my_prev][0] = onset;
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
        bool in_group = false;
        for (int k = 0; k < len; ++k) in_group = in_group || cur->sensors[src][k] == sensor;
        bool extended = false;
        if (!in_group) {
            if (T.use_audio) {
                // rec_audio[-i - 1:] of the two channels -> median 5 -> diff -> negative part -> abs
                const int64_t want = counter - o0 + LOC_LOOKAROUND + 1;
                int64_t start = counter - want;
                if (!zero_pad && start < 0) start = 0;
                const int64_t n64 = counter - start;
                if (n64 < 3 || n64 > T.max_section) {
                    flags |= OFP_LOCF_SECTION;
                } else {
                    const int n = (int)n64, m = n - 1;
                    float mx = -INFINITY, my = -INFINITY;
                    for (int i = tid; i < 2 * m; i += nt) {
                        const int which = i >= m, t = which ? i - m : i;
                        const int col = which ? sensor : s0;
                        float md[2];
                        for (int q = 0; q < 2; ++q) {
                            float w[5];
                            for (int k = 0; k < 5; ++k) {
                                int64_t u = t + q + k - 2;
                                if (u < 0) u = -u - 1;
                                if (u >= n) u = 2 * (int64_t)n - u - 1;
                                w[k] = audio(start + u, col);
                            }
                            md[q] = med5(w);
                        }
                        float d = md[1] - md[0];
                        if (d >= 0.0f) d = 0.0f;
                        d = fabsf(d);
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
                            adjust_onset_wave(v.xs, v.ys, m, LOC_LOOKAROUND, current + LOC_LOOKAROUND, new_lag, mx, my, tid,
                                              &ca, &cb);
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
                            cur->onsets[src][0] = o0;
                            if (my_prev >= 0) nxt->onsets[my_prev][0] = o0;
                        }
                    }
                    __syncthreads();
                }
            }
            const double dl = (double)lag;
            const bool legal = (double)T.mn[s0 * T.S + sensor] < dl && dl < (double)T.mx[s0 * T.S + sensor];
            if (legal && len >= OFP_LOCS_MEMBERS) {
                flags |= OFP_LOCF_MEMBERS;
            } else if (legal) {
                __syncthreads();
                if (tid == 0) {
                    L.ext.len = len + 1;
                    for (int k = 0; k < len; ++k) {
                        L.ext.sens[k] = cur->sensors[src][k];
                        L.ext.on[k] = cur->onsets[src][k];
                    }
                    L.ext.sens[len] = sensor;
                    L.ext.on[len] = onset;
                }
                __syncthreads();
                extended = true;
                if (len + 1 == 3) {
                    if (L.ext.sens[0] == L.ext.sens[1]) break;
                    const int64_t k = first_legal(T.maps, T.S, T.side, L.ext.sens[0], L.ext.sens[1], L.ext.sens[2],
                                                  (double)(L.ext.on[1] - L.ext.on[0]), (double)(L.ext.on[2] - L.ext.on[0]),
                                                  1 * T.spc, v.smin);
                    const int64_t ix = k < 0 ? 0 : k % T.side, iy = k < 0 ? 0 : k / T.side;
                    if (!(ix == 0 && iy == 0)) {
                        // trilaterate (:536-575), its reordering included
                        if (tid == 0) {
                            if (L.ext.sens[1] == 1) {
                                L.ext.sens[1] = 0;
                                L.ext.sens[2] = 1;
                                const int64_t t = L.ext.on[1];
                                L.ext.on[1] = L.ext.on[2];
                                L.ext.on[2] = t;
                            }
                            L.found = 0;
                        }
                        __syncthreads();
                        const int64_t da = L.ext.on[1] - L.ext.on[0], db = L.ext.on[2] - L.ext.on[0];
                        if (T.plan.n_layers > 0) {  // self.model.call_np((d_a1, d_b1)) * 100: a float32 product
                            if (tid < 64) {
                                for (int i = tid; i < 16 * T.plan.st_a; i += 64) v.ta[i] = 0.0f;
                                ofp_wave_lds_sync();
                                if (tid == 0) {
                                    v.ta[0] = (float)da;
                                    v.ta[1] = (float)db;
                                }
                                ofp_wave_lds_sync();
                                ofp_mlp_tile(T.plan, T.plan.params, v.ta, v.tb, tid, [&](int r, int col, float val) {
                                    if (r == 0 && col < 2) L.res[col] = (double)(val * 100.0f);
                                });
                                if (tid == 0) L.found = 1;
                            }
                        } else if (tid == 0) {
                            hybrj::Tdoa t;
                            for (int q = 0; q < 3; ++q) {
                                t.o[q] = T.sensors[3 * L.ext.sens[0] + q];
                                t.a[q] = T.sensors[3 * L.ext.sens[1] + q];
                                t.b[q] = T.sensors[3 * L.ext.sens[2] + q];
                            }
                            t.dda = (double)da / T.sr * T.c;
                            t.ddb = (double)db / T.sr * T.c;
                            const double guess[2] = {(double)ix - T.radius, (double)iy - T.radius};
                            const hybrj::Result r = hybrj::solve(t, guess, T.xtol, T.maxfev);
                            L.res[0] = r.x[0];
                            L.res[1] = r.x[1];
                            L.found = r.info == 1 ? 1 : 0;
                        }
                        __syncthreads();
                        found = L.found;
                        if (found) {  // remove_seed(new_groups, group)
                            if (tid == 0) {
                                int w = 0;
                                for (int q = 0; q < nn; ++q) {
                                    if (nxt->sensors[q][0] == L.ext.sens[0] && nxt->onsets[q][0] == L.ext.on[0]) continue;
                                    if (w != q) loc_copy_group(nxt, w, nxt->sensors[q], nxt->onsets[q], nxt->len[q], nxt->alias[q]);
                                    ++w;
                                }
                                L.kept = w;
                            }
                            __syncthreads();
                            nn = L.kept;
                            xy[0] = L.res[0];
                            xy[1] = L.res[1];
                        }
                        if (located && tid == 0) *located = L.ext;
                        returned = true;  // self.ongoing = new_groups; return res
                        continue;
                    }
                }
                if (nn < OFP_LOCS_GROUPS) {
                    if (tid == 0) loc_copy_group(nxt, nn, L.ext.sens, L.ext.on, L.ext.len, 0);
                    ++nn;
                } else {
                    flags |= OFP_LOCF_GROUPS;
                }
            }
        }
        // not past the largest possible lag: keep the group (an extended one a second time)
        if ((double)lag <= L.mml[s0]) {
            if (nn < OFP_LOCS_GROUPS) {
                if (tid == 0) {
                    if (extended) loc_copy_group(nxt, nn, L.ext.sens, L.ext.on, L.ext.len, 1);
                    else loc_copy_group(nxt, nn, cur->sensors[src], cur->onsets[src], len, my_prev >= 0 ? 1 : 0);
                }
                if (!extended) prev_out = nn;
                ++nn;
            } else {
                flags |= OFP_LOCF_GROUPS;
            }
        }
        __syncthreads();
    }
    if (!returned) {  // new_groups.append(([sensor_index], [onset_index]))
        if (nn < OFP_LOCS_GROUPS) {
            if (tid == 0) {
                const int32_t s1[1] = {sensor};
                const int64_t o1[1] = {onset};
                loc_copy_group(nxt, nn, s1, o1, 1, 0);
            }
            ++nn;
        } else {
            flags |= OFP_LOCF_GROUPS;
        }
    }
    __syncthreads();
    if (tid == 0) {
        nxt->n_groups = nn;
        nxt->flags = flags;
        L.cur ^= 1;
    }
    __syncthreads();
    return found;
}

// ---- Multilaterate.locate (the planar locator) ---------------------------------------------------------------

// One call of the 2-D Multilaterate.locate(sensor, onset) (reference multilateration.py:677-733) by the whole
// workgroup, on the same state as loc_feed.  Where it differs from the 3-D routine: no skip of a group past its
// largest lag at the top of the loop, no swap on a negative lag and no cross-correlation step (nothing is ever changed
// in place, so an alias entry only records that two entries are one object); no break on equal first sensors and no
// remove_seed; groups grow beyond three members and only the group that has just reached three is searched and
// solved; a call whose search finds a cell ends with `ongoing` = new_groups whether or not the solve succeeds;
// trilaterate keeps the sensors' order and forms its deltas as lag * c / sr.  Returns 1 when a position was returned
// (xy: the Cartesian root in cm), else 0; `located` as in loc_feed.
__device__ inline int loc_feed_2d(const LocTables& T, const LocView& v, int sensor, int64_t onset, double* xy,
                                  LocGroup* located) {
    LocLds& L = *v.L;
    const int tid = threadIdx.x;
    ofp_locate_state* cur = &L.st[L.cur];
    ofp_locate_state* nxt = &L.st[L.cur ^ 1];
    const int n_cur = cur->n_groups;
    int flags = cur->flags;
    int nn = 0;          // len(new_groups)
    int prev_out = -1;   // where the previous iteration appended its (unextended) group object
    int found = 0;
    bool returned = false;
    __syncthreads();
    for (int gi = 0; gi < n_cur && !returned; ++gi) {
        const bool alias = gi > 0 && cur->alias[gi] != 0;
        const int src = alias ? gi - 1 : gi;
        const int my_prev = alias ? prev_out : -1;
        prev_out = -1;
        const int len = cur->len[src];
        const int s0 = cur->sensors[src][0];
        const int64_t lag = onset - cur->onsets[src][0];
        bool in_group = false;
        for (int k = 0; k < len; ++k) in_group = in_group || cur->sensors[src][k] == sensor;
        bool extended = false;
        if (!in_group) {
            const double dl = (double)lag;
            const bool legal = (double)T.mn[s0 * T.S + sensor] < dl && dl < (double)T.mx[s0 * T.S + sensor];
            if (legal && len >= OFP_LOCS_MEMBERS) {
                flags |= OFP_LOCF_MEMBERS;
            } else if (legal) {
                __syncthreads();
                if (tid == 0) {
                    L.ext.len = len + 1;
                    for (int k = 0; k < len; ++k) {
                        L.ext.sens[k] = cur->sensors[src][k];
                        L.ext.on[k] = cur->onsets[src][k];
                    }
                    L.ext.sens[len] = sensor;
                    L.ext.on[len] = onset;
                }
                __syncthreads();
                extended = true;
                if (len + 1 == 3) {
                    const int64_t da = L.ext.on[1] - L.ext.on[0], db = L.ext.on[2] - L.ext.on[0];
                    const int64_t k = first_legal(T.maps, T.S, T.side, L.ext.sens[0], L.ext.sens[1], L.ext.sens[2],
                                                  (double)da, (double)db, 1 * T.spc, v.smin);
                    const int64_t ix = k < 0 ? 0 : k % T.side, iy = k < 0 ? 0 : k / T.side;
                    if (!(ix == 0 && iy == 0)) {
                        if (tid == 0) {  // trilaterate (:714-733)
                            hybrj::Tdoa t;
                            for (int q = 0; q < 3; ++q) {
                                t.o[q] = T.sensors[3 * L.ext.sens[0] + q];
                                t.a[q] = T.sensors[3 * L.ext.sens[1] + q];
                                t.b[q] = T.sensors[3 * L.ext.sens[2] + q];
                            }
                            t.dda = (double)da * T.c / T.sr;
                            t.ddb = (double)db * T.c / T.sr;
                            const double guess[2] = {(double)ix - T.radius, (double)iy - T.radius};
                            const hybrj::Result r = hybrj::solve(t, guess, T.xtol, T.maxfev);
                            L.res[0] = r.x[0];
                            L.res[1] = r.x[1];
                            L.found = r.info == 1 ? 1 : 0;
                        }
                        __syncthreads();
                        found = L.found;
                        if (found) {
                            xy[0] = L.res[0];
                            xy[1] = L.res[1];
                        }
                        if (located && tid == 0) *located = L.ext;
                        returned = true;  // self.ongoing = new_groups; return res
                        continue;
                    }
                }
                if (nn < OFP_LOCS_GROUPS) {
                    if (tid == 0) loc_copy_group(nxt, nn, L.ext.sens, L.ext.on, L.ext.len, 0);
                    ++nn;
                } else {
                    flags |= OFP_LOCF_GROUPS;
                }
            }
        }
        // the test sees the extended group: one that passed is_legal is appended a second time
        if ((double)lag <= L.mml[s0]) {
            if (nn < OFP_LOCS_GROUPS) {
                if (tid == 0) {
                    if (extended) loc_copy_group(nxt, nn, L.ext.sens, L.ext.on, L.ext.len, 1);
                    else loc_copy_group(nxt, nn, cur->sensors[src], cur->onsets[src], len, my_prev >= 0 ? 1 : 0);
                }
                if (!extended) prev_out = nn;
                ++nn;
            } else {
                flags |= OFP_LOCF_GROUPS;
            }
        }
        __syncthreads();
    }
    if (!returned) {  // new_groups.append(([sensor_index], [onset_index]))
        if (nn < OFP_LOCS_GROUPS) {
            if (tid == 0) {
                const int32_t s1[1] = {sensor};
                const int64_t o1[1] = {onset};
                loc_copy_group(nxt, nn, s1, o1, 1, 0);
            }
            ++nn;
        } else {
            flags |= OFP_LOCF_GROUPS;
        }
    }
    __syncthreads();
    if (tid == 0) {
        nxt->n_groups = nn;
        nxt->flags = flags;
        L.cur ^= 1;
    }
    __syncthreads();
    return found;
}

}  // namespace ofp

// the launch form of a locator's tables, checked (ofp_locate.hip); `who` names the entry point in the error text
int ofp_locate_tables(const ofp_hop_locator* loc, const char* who, ofp::LocTables* out);
// the same for the planar kind: use_audio and max_section are ignored, a network is refused
int ofp_locate_tables_2d(const ofp_hop_locator* loc, const char* who, ofp::LocTables* out);
