// The voting locator's device functions (multilateration.py: find_lag, MultilateratePaired.locate_cc): the lag search
// and the vote as functions that take their rows and LDS from the caller, and the locator as a stage of a stream
// ("The voting locator in the hop") -- the grouping state machine and FIFO of ofp_regress_dev.h, and
// locate_cc on the window of the group that is due, one step per hop by one workgroup of 256 threads.  The batched
// kernels (k_find_lags, k_paired_vote, ofp_locate2d.hip), the hop's fused kernel and node (ofp_hop.hip) and the replay
// (ofp_locate_cc_stream, ofp_locate2d.hip) run these functions.
#pragma once
#include <climits>
#include <cmath>

#include "ofp_common.h"
#include "ofp_regress_dev.h"
#include "ofp_xcorr_canon.h"

namespace ofppair {

constexpr int FT = 256;  // threads per workgroup
constexpr int FW = 64;   // wavefront

// Is (ov, oi) before (v, i) in np.argmax order?  i < 0: empty slot; a NaN beats any number; ties by index.
static __device__ __forceinline__ bool argmax_before(float ov, int oi, float v, int i) {
    if (oi < 0) return false;
    if (i < 0) return true;
    const bool on = isnan(ov), n = isnan(v);
    if (on != n) return on;
    if (n) return oi < i;
    return ov > v || (ov == v && oi < i);
}

// Workgroup-wide argmax of one (value, index) per thread; s_v / s_i hold one slot per wave.  Every thread gets the
// result.
static __device__ void wg_argmax(float& v, int& i, float* s_v, int* s_i) {
    for (int o = FW / 2; o > 0; o >>= 1) {
        const float ov = __shfl_xor(v, o);
        const int oi = __shfl_xor(i, o);
        if (argmax_before(ov, oi, v, i)) {
            v = ov;
            i = oi;
        }
    }
    const int lane = threadIdx.x & (FW - 1), wave = threadIdx.x / FW;
    __syncthreads();
    if (lane == 0) {
        s_v[wave] = v;
        s_i[wave] = i;
    }
    __syncthreads();
    v = s_v[0];
    i = s_i[0];
    for (int w = 1; w < FT / FW; ++w)
        if (argmax_before(s_v[w], s_i[w], v, i)) {
            v = s_v[w];
            i = s_i[w];
        }
}

static __device__ int wg_min(int v, int* s_i) {
    for (int o = FW / 2; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o));
    const int lane = threadIdx.x & (FW - 1), wave = threadIdx.x / FW;
    __syncthreads();
    if (lane == 0) s_i[wave] = v;
    __syncthreads();
    v = s_i[0];
    for (int w = 1; w < FT / FW; ++w) v = min(v, s_i[w]);
    return v;
}

// np.argmax(np.correlate(a, b, "full")) of two rows in LDS, by the canon of ofp_xcorr_canon.h: every lag's dot product
// rounded once to float32, the first maximum, a NaN wins.  each(j, v) sees every entry.  The lag is the result minus
// (la - 1).  Every thread gets the result.
template <class Each>
static __device__ __forceinline__ int lag_search(const float* sa, int la, const float* sb, int lb, float* s_v, int* s_i,
                                                 Each each) {
    const int n = la + lb - 1;
    float bv = 0.f;
    int bi = -1;
    for (int j = threadIdx.x; j < n; j += FT) {
        const float v = (float)ofp::cc_dot(sa, la, sb, lb, j - (lb - 1));
        each(j, v);
        if (argmax_before(v, j, bv, bi)) {
            bv = v;
            bi = j;
        }
    }
    wg_argmax(bv, bi, s_v, s_i);
    return bi;
}

// numpy's cartesian_to_polar(x, y, radius): (sqrt(x^2 + y^2) / radius, degrees(arctan2(y, x) % 2 pi))
static __device__ __forceinline__ void polar(double x, double y, double radius, double* out) {
    const double two_pi = 2.0 * M_PI;
    double a = atan2(y, x);
    double m = fmod(a, two_pi);  // npy_divmod: the remainder takes the divisor's sign
    if (m != 0.0) {
        if (m < 0.0) m += two_pi;
    } else {
        m = copysign(0.0, two_pi);
    }
    out[0] = sqrt(x * x + y * y) / radius;
    out[1] = m * (180.0 / M_PI);
}

// The vote's index as its users hold it (`Index`: anything with starts, sorted, vmin, nb, S, side, tol -- the batched
// kernel's arguments or the stage's configuration).
// The run of sorted cells of map m whose value v satisfies lag - tol < v < lag + tol.
template <class Index>
static __device__ __forceinline__ void lag_run(const Index& A, int m, int lag, int64_t cells, int64_t* p0, int64_t* p1) {
    const double lo = floor((double)lag - A.tol) + 1.0 - A.vmin[m];
    const double hi = ceil((double)lag + A.tol) - 1.0 - A.vmin[m];
    const int b0 = (int)fmin(fmax(lo, 0.0), (double)A.nb);  // clamped before the conversion
    const int b1 = (int)fmax(fmin(hi, (double)(A.nb - 1)), -1.0);
    const int32_t* st = A.starts + (int64_t)m * (A.nb + 1);
    if (b0 > b1) {
        *p0 = *p1 = 0;
        return;
    }
    *p0 = (int64_t)m * cells + st[b0];
    *p1 = (int64_t)m * cells + st[b1 + 1];
}

// locate_cc's vote for first sensor i and its two lags: np.argmax of the vote grid -- the smallest cell in both runs,
// else the smallest cell of either, else cell 0.  bits: ceil(side^2 / 32) words of LDS.  Every thread gets the result.
template <class Index>
static __device__ __forceinline__ int vote_cell(const Index& A, int i, int lag0, int lag1, unsigned int* bits, int* s_i) {
    const int64_t cells = (int64_t)A.side * A.side;
    int64_t a0, a1, b0 = 0, b1 = 0;
    lag_run(A, 2 * i, lag0, cells, &a0, &a1);
    if (A.S > 2) lag_run(A, 2 * i + 1, lag1, cells, &b0, &b1);
    int best = INT_MAX;
    if (a0 < a1 && b0 < b1) {  // two votes possible: the smallest cell in both runs
        const int words = (int)ofp::cdiv(cells, 32);
        for (int w = threadIdx.x; w < words; w += FT) bits[w] = 0u;
        __syncthreads();
        for (int64_t p = b0 + threadIdx.x; p < b1; p += FT) {
            const int c = A.sorted[p];
            atomicOr(&bits[c >> 5], 1u << (c & 31));
        }
        __syncthreads();
        int mine = INT_MAX;
        for (int64_t p = a0 + threadIdx.x; p < a1; p += FT) {
            const int c = A.sorted[p];
            if (bits[c >> 5] & (1u << (c & 31))) mine = min(mine, c);
        }
        best = wg_min(mine, s_i);
    }
    if (best == INT_MAX) {  // at most one vote: the smallest cell of either run (cell 0 when both are empty)
        int mine = INT_MAX;
        for (int64_t p = a0 + threadIdx.x; p < a1; p += FT) mine = min(mine, A.sorted[p]);
        for (int64_t p = b0 + threadIdx.x; p < b1; p += FT) mine = min(mine, A.sorted[p]);
        best = wg_min(mine, s_i);
        if (best == INT_MAX) best = 0;
    }
    return best;
}

// The cell's Cartesian coordinates (col - (side-1)/2, (side-1)/2 - row).
static __device__ __forceinline__ void cell_xy(int cell, int side, double* x, double* y) {
    const double half = (side - 1) / 2.0;
    *x = (double)(cell % side) - half;
    *y = half - (double)(cell / side);
}

// ---- the stage ----------------------------------------------------------------------------------------------------

constexpr int MAX_WINDOW = 1024;  // left + right: 12 KiB of rows
constexpr size_t LDS_RED = 32;    // the stage's LDS starts with the reductions' partials: 4 floats, 4 ints

// The index of a MultilateratePaired (ofp_vote_index; map 2i + k: sensor i's neighbour k) with locate_cc's and the
// grouping's parameters.  F, pre: the names the state machine of ofp_regress_dev.h knows the window by.
struct Cfg {
    const int32_t* starts;
    const int32_t* sorted;
    const int32_t* vmin;
    int nb, S, side;
    double tol, radius;
    int B, F, pre, D, min_channels;  // block size, left + right, left, max_distance
    ofp_regress_state* state;
};

// What one hop of the stage reports; written only when the hop evaluates a hit, `flags` always.
struct Out {
    int64_t* onset;
    int64_t* row;     // [S] the group's row
    int32_t* first;
    int32_t* status;  // OFP_PAIRED_OK, or OFP_PAIRED_NEG_WINDOW (then cell -1, lags INT_MIN, NaN coordinates)
    int32_t* lags;    // [2]
    int32_t* cell;
    double* xy;       // [2]
    double* rphi;     // [2]
    int32_t* flags;
};

inline size_t lds_bytes(int window, int side) {
    return LDS_RED + 3 * (size_t)window * 4 + 4 * (size_t)ofp::cdiv((int64_t)side * side, 32);
}

// One hop of the stage that is not idle (ofpreg::idle); h, n, rec, sample as ofpreg::step takes them.  lds:
// lds_bytes(F, side) of LDS nobody else uses.  Returns 1 when a hit was evaluated (the same on every thread).
template <class Rec, class Sample>
__device__ __forceinline__ int step(const Cfg& g, int64_t h, int n, Rec rec, Sample sample, unsigned char* lds,
                                    const Out& o) {
    __shared__ int s_first;
    __shared__ int64_t s_start;
    const int S = g.S, w = g.F;
    if (threadIdx.x == 0) {
        int64_t start = 0;
        const int slot = ofpreg::queue_step(g, S, h, n, rec, &start, o.row, o.flags);
        int first = -1;
        if (slot >= 0) {  // the earliest channel of the row, ties by channel (k_paired_windows)
            int64_t onset = 0;
            for (int c = 0; c < S; ++c) {
                const int64_t v = g.state->q_row[slot][c];
                if (v >= 0 && (first < 0 || v < onset)) {
                    first = c;
                    onset = v;
                }
            }
            *o.onset = onset;
            *o.first = first;
        }
        s_first = first;
        s_start = start;
    }
    __syncthreads();
    const int first = s_first;
    if (first < 0) return 0;
    const int64_t start = s_start;
    if (start < 0) {  // locate_cc's slice would wrap: refused, as the batched form refuses it
        if (threadIdx.x == 0) {
            *o.status = OFP_PAIRED_NEG_WINDOW;
            *o.cell = -1;
            for (int k = 0; k < 2; ++k) {
                o.lags[k] = INT_MIN;
                o.xy[k] = __builtin_nan("");
                o.rphi[k] = __builtin_nan("");
            }
        }
        return 1;
    }
    float* s_v = reinterpret_cast<float*>(lds);
    int* s_i = reinterpret_cast<int*>(lds + 16);
    float* rows = reinterpret_cast<float*>(lds + LDS_RED);  // [3][w]: first, (first - 1) % S, (first + 1) % S
    unsigned int* bits = reinterpret_cast<unsigned int*>(rows + 3 * w);
    for (int i = threadIdx.x; i < 3 * w; i += FT) {
        const int r = i / w, j = i - r * w;
        const int col = r == 0 ? first : (first + (r == 1 ? S - 1 : 1)) % S;
        rows[i] = sample(start + j, col);
    }
    __syncthreads();
    int lag[2];
    for (int k = 0; k < 2; ++k)
        lag[k] = lag_search(rows, w, rows + (1 + k) * w, w, s_v, s_i, [](int, float) {}) - (w - 1);
    const int best = vote_cell(g, first, lag[0], lag[1], bits, s_i);
    if (threadIdx.x == 0) {
        double x, y;
        cell_xy(best, g.side, &x, &y);
        *o.status = OFP_PAIRED_OK;
        *o.cell = best;
        o.lags[0] = lag[0];
        o.lags[1] = lag[1];
        o.xy[0] = x;
        o.xy[1] = y;
        polar(x, y, g.radius, o.rphi);
    }
    return 1;
}

}  // namespace ofppair

// The checked stage form of `p` (ofp_locate2d.hip), without B and state; OFP_ERR_INVALID with `who` in the message
// outside the envelope.
int ofp_paired_cfg(const ofp_hop_paired* p, const char* who, ofppair::Cfg* out);
