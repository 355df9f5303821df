// 2-D hit location (multilateration.py: find_lag / find_lag_multi, MultilateratePaired, lag_intensity_map).
// All geometry is fp64 as in numpy; with -ffp-contract=off every value is rounded as numpy rounds it.
//
// k_find_lags:      one workgroup per row pair: both rows staged in LDS, np.correlate(a, b, "full") by the canon of
//                   ofp_xcorr_canon.h, np.argmax (first maximum, a NaN wins), and optionally scipy.signal.find_peaks
//                   with default arguments followed by a top-n selection (descending value, ties by ascending index).
// k_vote_index:     one workgroup per neighbour map: a stable counting sort of the map's cells by their (integer) lag
//                   value -- histogram, prefix, in-order scatter by one wave -- so that the cells of one lag value are
//                   a contiguous run, in ascending cell order.
// k_paired_windows: per hit, the window x[onset - left : onset + right] of the first channel and its two neighbours
//                   as row offsets for k_find_lags (from explicit hits or from ofp_group_onsets' rows).
// k_paired_vote:    per hit, one workgroup: MultilateratePaired.locate_cc's vote.  The cells that match a lag within
//                   tol are a contiguous run of the index; the answer (np.argmax of the vote) is the smallest cell in
//                   both runs, else the smallest cell of either, else cell 0.  Only the runs are read.
// k_vote_grid:      the full vote grid (the reference's self.res) for a few hits.
// k_paired_solve:   MultilateratePaired.locate per row, one lane each: the weighted guess, hybrj, polar.
// k_intensity:      lag_intensity_map's two dB grids, one thread per cell and microphone.
// k_locate_cc_stream: the replay of the voting locator's stream stage (ofp_paired_dev.h, which also holds the lag
//                   search and the vote that k_find_lags and k_paired_vote run).
#include <cmath>
#include <climits>
#include <cstring>

#include "ofp_common.h"
#include "ofp_hybrj.h"
#include "ofp_paired_dev.h"
#include "ofp_xcorr_canon.h"

namespace {

using ofp::cdiv;
using ofppair::argmax_before;
using ofppair::FT;  // threads per workgroup
using ofppair::FW;  // wavefront
using ofppair::polar;
using ofppair::wg_argmax;

constexpr int F_MAXN = 4096;     // longest row
constexpr int F_MAXTOP = 16;     // most peaks reported
constexpr int64_t V_MAXCELLS = 1 << 20;  // largest grid the vote's LDS bitmap holds (128 KiB)
constexpr int V_MAXBUCKETS = 32768;      // widest lag range of one map (LDS histogram of 128 KiB)

ofp::LdsAttrCache g_find_lds, g_index_lds, g_vote_lds;

struct FindArgs {
    const float* a;
    const float* b;
    int64_t a_stride, b_stride;
    int es;  // element stride of both rows
    const int64_t* a_off;
    const int64_t* b_off;
    int len_a, len_b;  // lengths, or upper bounds of d_len_a / d_len_b
    const int32_t* d_len_a;
    const int32_t* d_len_b;
    int top_n;
    int32_t* lag;
    int32_t* peak_lag;
    float* peak_val;
    int32_t* n_peaks;
};

__global__ void __launch_bounds__(FT) k_find_lags(FindArgs A) {
    extern __shared__ float lds[];
    __shared__ float s_v[FT / FW];
    __shared__ int s_i[FT / FW];
    const int64_t row = blockIdx.x;
    const int la = A.d_len_a ? A.d_len_a[row] : A.len_a;
    const int lb = A.d_len_b ? A.d_len_b[row] : A.len_b;
    if (la < 1 || lb < 1 || la > A.len_a || lb > A.len_b) {  // empty (a refused window): no correlation
        if (threadIdx.x == 0) {
            A.lag[row] = INT_MIN;
            if (A.n_peaks) A.n_peaks[row] = -2;
        }
        for (int k = threadIdx.x; k < A.top_n; k += FT) {
            A.peak_lag[row * A.top_n + k] = 0;
            A.peak_val[row * A.top_n + k] = __builtin_nanf("");
        }
        return;
    }
    float* sa = lds;
    float* sb = sa + A.len_a;
    float* cc = sb + A.len_b;  // la + lb - 1 entries, only with top_n > 0
    unsigned char* flag = (unsigned char*)(cc + (A.len_a + A.len_b - 1));
    const float* ga = A.a + (A.a_off ? A.a_off[row] : row * A.a_stride);
    const float* gb = A.b + (A.b_off ? A.b_off[row] : row * A.b_stride);
    for (int t = threadIdx.x; t < la; t += FT) sa[t] = ga[(int64_t)t * A.es];
    for (int t = threadIdx.x; t < lb; t += FT) sb[t] = gb[(int64_t)t * A.es];
    __syncthreads();
    const int n = la + lb - 1;
    bool bad = false;
    const int bi = ofppair::lag_search(sa, la, sb, lb, s_v, s_i, [&](int j, float v) {
        if (A.top_n > 0) {
            cc[j] = v;
            flag[j] = 0;
        }
        bad |= !isfinite(v);
    });
    if (threadIdx.x == 0) {
        A.lag[row] = bi - (la - 1);
        if (A.top_n <= 0 && A.n_peaks) A.n_peaks[row] = 0;
    }
    if (A.top_n <= 0) return;
    const int top = A.top_n;
    if (__syncthreads_or(bad)) {  // scipy's peaks of a non-finite correlation are not a meaningful target
        if (threadIdx.x == 0) A.n_peaks[row] = -1;
        for (int k = threadIdx.x; k < top; k += FT) {
            A.peak_lag[row * top + k] = 0;
            A.peak_val[row * top + k] = __builtin_nanf("");
        }
        return;
    }
    // scipy.signal._peak_finding_utils._local_maxima_1d: a run [p, q) of equal values with cc[p-1] < cc[p] and
    // cc[q] < cc[p], 1 <= p, q <= n - 1, is a peak at (p + q - 1) // 2.  Only left edges walk, runs are disjoint.
    for (int p = 1 + threadIdx.x; p < n - 1; p += FT) {
        if (!(cc[p - 1] < cc[p])) continue;
        int q = p + 1;
        while (q < n - 1 && cc[q] == cc[p]) ++q;
        if (cc[q] < cc[p]) flag[(p + q - 1) / 2] = 1;
    }
    __syncthreads();
    int found = 0;
    for (; found < top; ++found) {
        float v = 0.f;
        int i = -1;
        for (int j = threadIdx.x; j < n; j += FT)
            if (flag[j] && argmax_before(cc[j], j, v, i)) {
                v = cc[j];
                i = j;
            }
        wg_argmax(v, i, s_v, s_i);
        if (i < 0) break;
        if (threadIdx.x == 0) {
            A.peak_lag[row * top + found] = i - (la - 1);
            A.peak_val[row * top + found] = v * v;
            flag[i] = 0;
        }
        __syncthreads();
    }
    for (int k = found + (int)threadIdx.x; k < top; k += FT) {
        A.peak_lag[row * top + k] = 0;
        A.peak_val[row * top + k] = __builtin_nanf("");
    }
    if (threadIdx.x == 0) A.n_peaks[row] = found;
}

// Stable counting sort of one map's cells by value - vmin (values must be integers in [vmin, vmin + nb)).
__global__ void __launch_bounds__(FT) k_vote_index(const float* __restrict__ maps, int64_t cells,
                                                   const int32_t* __restrict__ map_ids,
                                                   const int32_t* __restrict__ vmin, int nb,
                                                   int32_t* __restrict__ starts, int32_t* __restrict__ sorted,
                                                   int32_t* __restrict__ bad) {
    extern __shared__ int hist[];  // nb + 1
    __shared__ int s_part[FT];
    const int m = blockIdx.x;
    const float* map = maps + (int64_t)map_ids[m] * cells;
    const int v0 = vmin[m];
    for (int b = threadIdx.x; b <= nb; b += FT) hist[b] = 0;
    __syncthreads();
    bool wrong = false;
    for (int64_t c = threadIdx.x; c < cells; c += FT) {
        const float v = map[c];
        if (isnan(v)) continue;
        const double b = (double)v - v0;
        if (b != rint(b) || b < 0 || b >= nb) {
            wrong = true;
            continue;
        }
        atomicAdd(&hist[(int)b], 1);
    }
    wrong = __syncthreads_or(wrong);
    // exclusive prefix: each thread sums a chunk, the chunk sums are scanned, then each chunk is written
    const int chunk = (int)cdiv(nb + 1, FT);
    const int c0 = min((int)threadIdx.x * chunk, nb + 1), c1 = min(c0 + chunk, nb + 1);
    int sum = 0;
    for (int b = c0; b < c1; ++b) sum += hist[b];
    s_part[threadIdx.x] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        int run = 0;
        for (int t = 0; t < FT; ++t) {
            const int s = s_part[t];
            s_part[t] = run;
            run += s;
        }
    }
    __syncthreads();
    int run = s_part[threadIdx.x];
    for (int b = c0; b < c1; ++b) {
        const int h = hist[b];
        hist[b] = run;
        starts[(int64_t)m * (nb + 1) + b] = run;
        run += h;
    }
    __syncthreads();
    if (threadIdx.x == 0) bad[m] = wrong ? 1 : 0;
    if (threadIdx.x >= FW) return;
    // in-order scatter by wave 0, 64 cells at a time: a cell's slot is its bucket's cursor plus the number of lower
    // lanes with the same bucket; the last lane of a bucket advances the cursor
    int32_t* out = sorted + (int64_t)m * cells;
    const int lane = threadIdx.x;
    for (int64_t base = 0; base < cells; base += FW) {
        const int64_t c = base + lane;
        int b = -1;
        if (c < cells) {
            const float v = map[c];
            if (!isnan(v)) {
                const double d = (double)v - v0;
                if (d == rint(d) && d >= 0 && d < nb) b = (int)d;
            }
        }
        int rank = 0, cnt = 0;
        for (int k = 0; k < FW; ++k) {
            const int ob = __shfl(b, k);
            if (ob == b) {
                rank += k < lane;
                ++cnt;
            }
        }
        const int cur = b >= 0 ? hist[b] : 0;
        __builtin_amdgcn_wave_barrier();
        if (b >= 0) {
            out[cur + rank] = (int32_t)c;
            if (rank == cnt - 1) hist[b] = cur + cnt;
        }
        __builtin_amdgcn_wave_barrier();
    }
}

struct WinArgs {
    int64_t n_clips, N;
    int C, S;
    const int64_t* onset;
    const int32_t* first;
    const int32_t* clip;
    const int64_t* groups;
    int64_t cap;
    const int64_t* n_groups;
    int64_t B;
    int left, right;
    int64_t* a_off;
    int64_t* b_off;
    int32_t* len;
    int32_t* first_out;
    int32_t* status;
};

__global__ void k_paired_windows(WinArgs A) {
    const int64_t h = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (h >= A.B) return;
    int st = OFP_PAIRED_OK, first = -1;
    int64_t onset = 0, clip = 0;
    if (A.groups) {
        clip = h / A.cap;
        const int64_t r = h % A.cap;
        if (A.n_groups && r >= min(A.n_groups[clip], A.cap)) {
            st = OFP_PAIRED_UNUSED;
        } else {
            const int64_t* g = A.groups + h * A.C;
            for (int k = 0; k < A.C; ++k) {  // earliest channel, ties by channel
                const int64_t v = g[k];
                if (v >= 0 && (first < 0 || v < onset)) {
                    first = k;
                    onset = v;
                }
            }
            if (first < 0)
                st = OFP_PAIRED_NO_CHANNEL;
            else if (first >= A.S)
                st = OFP_PAIRED_BAD_HIT;  // a channel without a sensor
        }
    } else {
        onset = A.onset[h];
        first = A.first[h];
        clip = A.clip ? A.clip[h] : 0;
        if (first < 0 || first >= A.S || clip < 0 || clip >= A.n_clips) st = OFP_PAIRED_BAD_HIT;
    }
    int64_t start = 0, len = 0;
    if (st == OFP_PAIRED_OK) {
        start = onset - A.left;
        const int64_t stop = min(onset + (int64_t)A.right, A.N);
        len = stop - start;
        if (start < 0)
            st = OFP_PAIRED_NEG_WINDOW;
        else if (len < 1)
            st = OFP_PAIRED_EMPTY_WINDOW;
    }
    A.first_out[h] = first;
    A.status[h] = st;
    for (int k = 0; k < 2; ++k) {
        const int j = st == OFP_PAIRED_OK ? (first + (k == 0 ? A.S - 1 : 1)) % A.S : 0;
        const int64_t base = (clip * A.N + start) * A.C;
        A.a_off[2 * h + k] = st == OFP_PAIRED_OK ? base + first : 0;
        A.b_off[2 * h + k] = st == OFP_PAIRED_OK ? base + j : 0;
        A.len[2 * h + k] = st == OFP_PAIRED_OK ? (int32_t)len : 0;
    }
}

struct VoteArgs {
    const int32_t* starts;
    const int32_t* sorted;
    const int32_t* vmin;
    int nb, S, side;
    const int32_t* first;
    const int32_t* lags;
    const int32_t* status_in;
    double tol, radius;
    int32_t* cell;
    double* xy;
    double* rphi;
    int32_t* status;
};

__global__ void __launch_bounds__(FT) k_paired_vote(VoteArgs A) {
    extern __shared__ unsigned int bits[];
    __shared__ int s_i[FT / FW];
    const int64_t h = blockIdx.x;
    const int st = A.status_in[h];
    if (st != OFP_PAIRED_OK) {
        if (threadIdx.x == 0) {
            A.status[h] = st;
            A.cell[h] = -1;
            for (int k = 0; k < 2; ++k) {
                A.xy[2 * h + k] = __builtin_nan("");
                A.rphi[2 * h + k] = __builtin_nan("");
            }
        }
        return;
    }
    const int best = ofppair::vote_cell(A, A.first[h], A.lags[2 * h], A.lags[2 * h + 1], bits, s_i);
    if (threadIdx.x == 0) {
        double x, y;
        ofppair::cell_xy(best, A.side, &x, &y);
        A.status[h] = OFP_PAIRED_OK;
        A.cell[h] = best;
        A.xy[2 * h] = x;
        A.xy[2 * h + 1] = y;
        polar(x, y, A.radius, A.rphi + 2 * h);
    }
}

// res[h][c] = the number of the hit's neighbour maps with lag - tol < map[c] < lag + tol (float32, as the reference's
// self.res), zeros for a hit with a status.
__global__ void k_vote_grid(const float* __restrict__ maps, int64_t cells, const int32_t* __restrict__ map_ids, int S,
                            const int32_t* __restrict__ first, const int32_t* __restrict__ lags,
                            const int32_t* __restrict__ status, double tol, float* __restrict__ res) {
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t h = blockIdx.y;
    if (c >= cells) return;
    float v = 0.f;
    if (status[h] == OFP_PAIRED_OK) {
        const int i = first[h];
        for (int k = 0; k < (S > 2 ? 2 : 1); ++k) {
            const double m = maps[(int64_t)map_ids[2 * i + k] * cells + c];
            const double lag = lags[2 * h + k];
            v += (m < lag + tol && m > lag - tol) ? 1.f : 0.f;
        }
    }
    res[h * cells + c] = v;
}

__global__ void k_paired_solve(const double* __restrict__ sensors, int S, const int32_t* __restrict__ lags,
                               const int32_t* __restrict__ first, int64_t B, double c, double sr, double radius,
                               double xtol, int maxfev, double* __restrict__ root, double* __restrict__ rphi,
                               int32_t* __restrict__ ier) {
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= B) return;
    const int i = first[g];
    if (i < 0 || i >= S) {
        for (int k = 0; k < 2; ++k) root[2 * g + k] = rphi[2 * g + k] = __builtin_nan("");
        ier[g] = OFP_PAIRED_BAD_HIT;
        return;
    }
    const double* sa = sensors + 3 * ((i + S - 1) % S);
    const double* sb = sensors + 3 * ((i + 1) % S);
    const double* so = sensors + 3 * i;
    // multilateration.py:802-826, left to right
    const double da = (double)lags[2 * g] * c / sr, db = (double)lags[2 * g + 1] * c / sr;
    const double wa = fabs(da) / radius, wb = fabs(db) / radius, wo = fabs(da + db) / (2.0 * radius);
    const double x0[2] = {sa[0] * wa + sb[0] * wb + so[0] * wo, sa[1] * wa + sb[1] * wb + so[1] * wo};
    ofp::hybrj::Tdoa t;
    for (int k = 0; k < 3; ++k) {
        t.o[k] = so[k];
        t.a[k] = sa[k];
        t.b[k] = sb[k];
    }
    t.dda = da;
    t.ddb = db;
    const ofp::hybrj::Result res = ofp::hybrj::solve(t, x0, xtol, maxfev);
    root[2 * g] = res.x[0];
    root[2 * g + 1] = res.x[1];
    polar(res.x[0], res.x[1], radius, rphi + 2 * g);
    ier[g] = res.info;
}

// attenuate_intensity (multilateration.py:1011-1035) at every cell p = (col - r, row - r, 0) for microphone m, then
// 10 log10.  norm = sqrt((x^2 + y^2) + z^2) as np.linalg.norm reduces three values; the dot with (0, 0, 1) is z / norm.
__global__ void k_intensity(const double* __restrict__ mics, int r, double refl, float* __restrict__ out) {
    const int side = 2 * r + 1;
    const int64_t cells = (int64_t)side * side;
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int m = blockIdx.y;
    if (k >= cells) return;
    const double* mic = mics + 3 * m;
    const double x = mic[0] - (double)(k % side - r), y = mic[1] - (double)(k / side - r), z = mic[2] - 0.0;
    const double dist = sqrt(x * x + y * y + z * z);
    const double theta = acos(z / dist);
    const double a = 1.0 * (1.0 + refl * (1.0 - fabs(cos(theta)))) / dist;
    out[m * cells + k] = (float)(10.0 * log10(a));
}

// The voting locator's stage (ofppair::step) over a resident recording and a given onset list: a loop over the hops,
// by one workgroup, as k_regress_stream runs the window regressor's.
struct CcReplayArgs {
    ofppair::Cfg g;
    const float* audio;
    int64_t n_rows, K;
    const int32_t* channel;
    const int64_t* onset;
    int32_t *hit, *status, *first, *lags, *cell, *pending, *flags;
    int64_t *onset_out, *row;
    double *xy, *rphi;
};

__global__ void __launch_bounds__(FT) k_locate_cc_stream(CcReplayArgs a) {
    extern __shared__ __align__(16) unsigned char smem[];
    const int S = a.g.S, B = a.g.B;
    const int64_t H = a.n_rows / B;
    ofp_regress_state* st = a.g.state;
    int64_t next = 0;  // first onset not yet fed (the same on every thread)
    auto sample = [&](int64_t t, int col) -> float { return t < 0 ? 0.0f : a.audio[t * S + col]; };
    for (int64_t h = 1; h <= H; ++h) {
        const int64_t end = h * (int64_t)B;
        int n = 0;
        while (next + n < a.K && a.onset[next + n] < end) ++n;
        const int64_t base = next;
        auto rec = [&](int i, int& ch, int64_t& s) {
            ch = a.channel[base + i];
            s = a.onset[base + i];
        };
        int ev = 0;
        const bool busy = !ofpreg::idle(a.g, h, n, st->wake);
        __syncthreads();  // every thread has read `wake` before thread 0 of a busy hop stores the next one
        if (busy) {
            const int64_t k = h - 1;
            const ofppair::Out o{a.onset_out + k, a.row + k * S, a.first + k, a.status + k, a.lags + 2 * k,
                                 a.cell + k,      a.xy + 2 * k,  a.rphi + 2 * k, a.flags};
            ev = ofppair::step(a.g, h, n, rec, sample, smem, o);
        }
        __syncthreads();  // the state thread 0 left, and the step's shared words, before the next hop reads them
        if (threadIdx.x == 0) {
            a.hit[h - 1] = ev;
            a.pending[h - 1] = st->len + ev;  // (the FIFO is longest after the hop's closes, before its evaluation)
        }
        next += n;
    }
    if (threadIdx.x == 0) *a.flags = st->flags;
}

}  // namespace

int ofp_paired_cfg(const ofp_hop_paired* p, const char* who, ofppair::Cfg* out) {
    OFP_REQUIRE(p && out, "%s: NULL argument", who);
    OFP_REQUIRE(p->d_starts && p->d_sorted && p->d_vmin, "%s: NULL index table", who);
    OFP_REQUIRE(p->S >= 2 && p->S <= OFP_REG_MAX_SIGNALS, "%s: %d sensors (2..%d supported)", who, p->S, OFP_REG_MAX_SIGNALS);
    OFP_REQUIRE(p->side >= 1 && (int64_t)p->side * p->side <= V_MAXCELLS, "%s: grid side %d (at most %lld cells)", who,
                p->side, (long long)V_MAXCELLS);
    OFP_REQUIRE(p->n_buckets >= 1 && p->n_buckets <= V_MAXBUCKETS, "%s: lag range of %d values", who, p->n_buckets);
    OFP_REQUIRE(p->tol >= 0.0 && p->radius > 0.0, "%s: tol must be >= 0 and radius > 0", who);
    OFP_REQUIRE(p->left >= 0 && p->right >= 1 && (int64_t)p->left + p->right <= ofppair::MAX_WINDOW,
                "%s: left %d, right %d (left >= 0, right >= 1, a window of at most %d samples)", who, p->left, p->right,
                ofppair::MAX_WINDOW);
    OFP_REQUIRE(p->max_distance >= 0 && p->min_channels >= 1 && p->min_channels <= p->S,
                "%s: need max_distance >= 0 and 1 <= min_channels <= %d", who, p->S);
    const size_t lds = ofppair::lds_bytes(p->left + p->right, p->side);
    OFP_REQUIRE(lds <= ofpreg::LDS_SWITCH, "%s: the stage needs %zu bytes of LDS (vote bitmap of a %d x %d grid and a %d-sample "
                "window), %zu allowed", who, lds, p->side, p->side, p->left + p->right, ofpreg::LDS_SWITCH);
    ofppair::Cfg g;
    std::memset(&g, 0, sizeof(g));
    g.starts = p->d_starts;
    g.sorted = p->d_sorted;
    g.vmin = p->d_vmin;
    g.nb = p->n_buckets;
    g.S = p->S;
    g.side = p->side;
    g.tol = p->tol;
    g.radius = p->radius;
    g.F = p->left + p->right;
    g.pre = p->left;
    g.D = p->max_distance;
    g.min_channels = p->min_channels;
    *out = g;
    return OFP_OK;
}

extern "C" {

int ofp_locate_cc_stream(const ofp_hop_paired* p, const float* d_audio, int64_t n_rows, int32_t block_size,
                         const int32_t* d_channel, const int64_t* d_onset, int64_t K, int32_t* d_hit, int32_t* d_status,
                         int64_t* d_onset_out, int32_t* d_first, int64_t* d_row, int32_t* d_lags, int32_t* d_cell,
                         double* d_xy, double* d_rphi, int32_t* d_pending, int32_t* d_flags, void* stream) {
    CcReplayArgs a;
    std::memset(&a, 0, sizeof(a));
    if (int rc = ofp_paired_cfg(p, "ofp_locate_cc_stream", &a.g)) return rc;
    OFP_REQUIRE(d_audio && d_hit && d_status && d_onset_out && d_first && d_row && d_lags && d_cell && d_xy && d_rphi &&
                    d_pending && d_flags && (K == 0 || (d_channel && d_onset)),
                "ofp_locate_cc_stream: NULL argument");
    OFP_REQUIRE(block_size >= 1 && n_rows >= 0 && K >= 0, "ofp_locate_cc_stream: bad sizes");
    hipStream_t st = (hipStream_t)stream;
    ofp_regress_state* d_state = nullptr;
    OFP_HIP(hipMalloc(&d_state, sizeof(ofp_regress_state)));
    auto run = [&]() -> int {
        OFP_HIP(hipMemsetAsync(d_state, 0, sizeof(ofp_regress_state), st));
        OFP_HIP(hipMemsetAsync(d_flags, 0, sizeof(int32_t), st));
        a.g.B = block_size;
        a.g.state = d_state;
        a.audio = d_audio;
        a.n_rows = n_rows;
        a.K = K;
        a.channel = d_channel;
        a.onset = d_onset;
        a.hit = d_hit;
        a.status = d_status;
        a.first = d_first;
        a.lags = d_lags;
        a.cell = d_cell;
        a.pending = d_pending;
        a.flags = d_flags;
        a.onset_out = d_onset_out;
        a.row = d_row;
        a.xy = d_xy;
        a.rphi = d_rphi;
        const size_t lds = ofppair::lds_bytes(a.g.F, a.g.side);
        static ofp::LdsAttrCache attr;
        if (int rc = ofp::ensure_dynamic_lds(reinterpret_cast<const void*>(k_locate_cc_stream), lds, attr)) return rc;
        hipLaunchKernelGGL(k_locate_cc_stream, dim3(1), dim3(FT), lds, st, a);
        OFP_LAUNCH_CHECK("k_locate_cc_stream");
        OFP_HIP(hipStreamSynchronize(st));  // (the state is freed below)
        return OFP_OK;
    };
    const int rc = run();
    (void)hipFree(d_state);
    return rc;
}

int ofp_find_lags(const float* d_a, const float* d_b, int64_t n_rows, int64_t a_stride, int64_t b_stride,
                  int32_t elem_stride, const int64_t* d_a_off, const int64_t* d_b_off, int32_t len_a, int32_t len_b,
                  const int32_t* d_len_a, const int32_t* d_len_b, int32_t top_n, int32_t* d_lag, int32_t* d_peak_lag,
                  float* d_peak_val, int32_t* d_n_peaks, void* stream) {
    OFP_REQUIRE(n_rows >= 0 && n_rows < (1ll << 31), "ofp_find_lags: row count %lld outside 0..2^31-1",
                (long long)n_rows);
    OFP_REQUIRE(len_a >= 1 && len_a <= F_MAXN && len_b >= 1 && len_b <= F_MAXN,
                "ofp_find_lags: row lengths %d, %d outside 1..%d", len_a, len_b, F_MAXN);
    OFP_REQUIRE(top_n >= 0 && top_n <= F_MAXTOP, "ofp_find_lags: top_n %d outside 0..%d", top_n, F_MAXTOP);
    OFP_REQUIRE(elem_stride >= 1, "ofp_find_lags: element stride %d < 1", elem_stride);
    if (n_rows == 0) return OFP_OK;
    OFP_REQUIRE(d_a && d_b && d_lag, "ofp_find_lags: NULL argument");
    OFP_REQUIRE(top_n == 0 || (d_peak_lag && d_peak_val && d_n_peaks), "ofp_find_lags: NULL peak output");
    size_t lds = 4 * (size_t)(len_a + len_b);
    if (top_n > 0) lds += 5 * (size_t)(len_a + len_b - 1);
    int e = ofp::ensure_dynamic_lds((const void*)k_find_lags, lds, g_find_lds);
    if (e != OFP_OK) return e;
    FindArgs A{d_a, d_b, a_stride, b_stride, elem_stride, d_a_off, d_b_off, len_a, len_b, d_len_a, d_len_b,
               top_n, d_lag, d_peak_lag, d_peak_val, d_n_peaks};
    hipLaunchKernelGGL(k_find_lags, dim3((unsigned)n_rows), dim3(FT), lds, (hipStream_t)stream, A);
    OFP_LAUNCH_CHECK("k_find_lags");
    return OFP_OK;
}

int ofp_vote_index(const float* d_maps, int64_t cells, const int32_t* d_map_ids, int32_t n_maps,
                   const int32_t* d_vmin, int32_t n_buckets, int32_t* d_starts, int32_t* d_sorted, int32_t* d_bad,
                   void* stream) {
    OFP_REQUIRE(n_maps >= 1 && n_maps <= 128, "ofp_vote_index: %d maps (1..128)", n_maps);
    OFP_REQUIRE(cells >= 1 && cells <= V_MAXCELLS, "ofp_vote_index: %lld cells (1..%lld)", (long long)cells,
                (long long)V_MAXCELLS);
    OFP_REQUIRE(n_buckets >= 1 && n_buckets <= V_MAXBUCKETS, "ofp_vote_index: lag range of %d values (1..%d)",
                n_buckets, V_MAXBUCKETS);
    OFP_REQUIRE(d_maps && d_map_ids && d_vmin && d_starts && d_sorted && d_bad, "ofp_vote_index: NULL argument");
    const size_t lds = 4 * (size_t)(n_buckets + 1);
    int e = ofp::ensure_dynamic_lds((const void*)k_vote_index, lds, g_index_lds);
    if (e != OFP_OK) return e;
    hipLaunchKernelGGL(k_vote_index, dim3((unsigned)n_maps), dim3(FT), lds, (hipStream_t)stream, d_maps, cells,
                       d_map_ids, d_vmin, (int)n_buckets, d_starts, d_sorted, d_bad);
    OFP_LAUNCH_CHECK("k_vote_index");
    return OFP_OK;
}

int ofp_paired_windows(int64_t n_clips, int64_t n_samples, int32_t n_channels, int32_t S, const int64_t* d_onset,
                       const int32_t* d_first, const int32_t* d_clip, const int64_t* d_groups, int64_t cap_groups,
                       const int64_t* d_n_groups, int64_t B, int32_t left, int32_t right, int64_t* d_a_off,
                       int64_t* d_b_off, int32_t* d_len, int32_t* d_first_out, int32_t* d_status, void* stream) {
    OFP_REQUIRE(S >= 2 && S <= 64 && n_channels >= S && n_clips >= 1 && n_samples >= 1,
                "ofp_paired_windows: %d sensors (2..64) and %d channels (>= sensors)", S, n_channels);
    OFP_REQUIRE(left >= 0 && right >= 1 && (int64_t)left + right <= F_MAXN,
                "ofp_paired_windows: left %d, right %d (left >= 0, right >= 1, left + right <= %d)", left, right,
                F_MAXN);
    OFP_REQUIRE(B >= 0, "ofp_paired_windows: negative hit count");
    OFP_REQUIRE(!d_groups || (cap_groups >= 1 && B == n_clips * cap_groups),
                "ofp_paired_windows: group rows need B == n_clips * cap_groups");
    if (B == 0) return OFP_OK;
    OFP_REQUIRE(d_groups || (d_onset && d_first), "ofp_paired_windows: give the hits or the group rows");
    OFP_REQUIRE(d_a_off && d_b_off && d_len && d_first_out && d_status, "ofp_paired_windows: NULL output");
    WinArgs A{n_clips, n_samples, n_channels, S, d_onset, d_first, d_clip, d_groups, cap_groups, d_n_groups, B, left,
              right, d_a_off, d_b_off, d_len, d_first_out, d_status};
    hipLaunchKernelGGL(k_paired_windows, dim3((unsigned)cdiv(B, FT)), dim3(FT), 0, (hipStream_t)stream, A);
    OFP_LAUNCH_CHECK("k_paired_windows");
    return OFP_OK;
}

int ofp_paired_vote(const float* d_maps, const int32_t* d_map_ids, const int32_t* d_starts, const int32_t* d_sorted,
                    const int32_t* d_vmin, int32_t n_buckets, int32_t S, int32_t side, const int32_t* d_first,
                    const int32_t* d_lags, const int32_t* d_status_in, int64_t B, double tol, double radius,
                    int32_t* d_cell, double* d_xy, double* d_rphi, int32_t* d_status, float* d_res, void* stream) {
    OFP_REQUIRE(S >= 2 && S <= 64, "ofp_paired_vote: %d sensors (2..64)", S);
    OFP_REQUIRE(side >= 1 && (int64_t)side * side <= V_MAXCELLS, "ofp_paired_vote: grid side %d (at most %lld cells)",
                side, (long long)V_MAXCELLS);
    OFP_REQUIRE(n_buckets >= 1 && n_buckets <= V_MAXBUCKETS, "ofp_paired_vote: lag range of %d values", n_buckets);
    OFP_REQUIRE(B >= 0 && B < (1ll << 31), "ofp_paired_vote: hit count %lld", (long long)B);
    OFP_REQUIRE(tol >= 0.0 && radius > 0.0, "ofp_paired_vote: tol must be >= 0 and radius > 0");
    if (B == 0) return OFP_OK;
    OFP_REQUIRE(d_starts && d_sorted && d_vmin && d_first && d_lags && d_status_in && d_cell && d_xy && d_rphi &&
                    d_status,
                "ofp_paired_vote: NULL argument");
    OFP_REQUIRE(!d_res || (d_maps && d_map_ids && B <= 65535), "ofp_paired_vote: the vote grid needs the maps");
    const int64_t cells = (int64_t)side * side;
    const size_t lds = 4 * (size_t)cdiv(cells, 32);
    int e = ofp::ensure_dynamic_lds((const void*)k_paired_vote, lds, g_vote_lds);
    if (e != OFP_OK) return e;
    hipStream_t s = (hipStream_t)stream;
    VoteArgs A{d_starts, d_sorted, d_vmin, n_buckets, S, side, d_first, d_lags, d_status_in, tol, radius,
               d_cell, d_xy, d_rphi, d_status};
    hipLaunchKernelGGL(k_paired_vote, dim3((unsigned)B), dim3(FT), lds, s, A);
    OFP_LAUNCH_CHECK("k_paired_vote");
    if (d_res) {
        hipLaunchKernelGGL(k_vote_grid, dim3((unsigned)cdiv(cells, FT), (unsigned)B), dim3(FT), 0, s, d_maps, cells,
                           d_map_ids, S, d_first, d_lags, d_status_in, tol, d_res);
        OFP_LAUNCH_CHECK("k_vote_grid");
    }
    return OFP_OK;
}

int ofp_paired_solve(const double* d_sensors, int32_t S, const int32_t* d_lags, const int32_t* d_first, int64_t B,
                     double c, double sr, double radius, double xtol, int32_t maxfev, double* d_root, double* d_rphi,
                     int32_t* d_ier, void* stream) {
    OFP_REQUIRE(S >= 2 && S <= 64, "ofp_paired_solve: %d sensors (2..64)", S);
    OFP_REQUIRE(B >= 0, "ofp_paired_solve: negative row count");
    OFP_REQUIRE(xtol >= 0.0 && maxfev > 0 && sr > 0.0, "ofp_paired_solve: xtol >= 0, maxfev > 0, sr > 0");
    if (B == 0) return OFP_OK;
    OFP_REQUIRE(d_sensors && d_lags && d_first && d_root && d_rphi && d_ier, "ofp_paired_solve: NULL argument");
    hipLaunchKernelGGL(k_paired_solve, dim3((unsigned)cdiv(B, 64)), dim3(64), 0, (hipStream_t)stream, d_sensors, S,
                       d_lags, d_first, B, c, sr, radius, xtol, (int)maxfev, d_root, d_rphi, d_ier);
    OFP_LAUNCH_CHECK("k_paired_solve");
    return OFP_OK;
}

int ofp_intensity_maps(const double* d_mics, int32_t r, double reflectivity, float* d_out, void* stream) {
    OFP_REQUIRE(r >= 0 && r <= 4096, "ofp_intensity_maps: grid radius %d outside 0..4096", r);
    OFP_REQUIRE(d_mics && d_out, "ofp_intensity_maps: NULL argument");
    const int side = 2 * r + 1;
    const int64_t cells = (int64_t)side * side;
    hipLaunchKernelGGL(k_intensity, dim3((unsigned)cdiv(cells, FT), 2), dim3(FT), 0, (hipStream_t)stream, d_mics, r,
                       reflectivity, d_out);
    OFP_LAUNCH_CHECK("k_intensity");
    return OFP_OK;
}

}  // extern "C"
