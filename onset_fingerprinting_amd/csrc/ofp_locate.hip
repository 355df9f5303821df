// Hit location (multilateration.py: lag_map_2d / lag_map_3d, Multilaterate3D.is_legal / is_legal_3d /
// trilaterate, solve_trilateration_3d).  All geometry is fp64 as in numpy; with -ffp-contract=off every
// value is rounded as numpy rounds it.
//
// k_lag_maps:    one thread per cell of every ordered sensor pair: the map of pair (i, j) holds
//                rint((|p - s_j| / c - |p - s_i| / c) * sr) over the grid p = (col - r, row - r, 0), NaN outside
//                the circle and below the floor.
// k_lag_minmax:  nanmin / nanmax of each map, one workgroup per pair.
// k_legal:       is_legal_3d for a batch of three-sensor groups, one workgroup per group: the first legal cell
//                in row-major order (np.argmax over the flattened mask), returned as np.unravel_index(.., "F")
//                returns it for a square map, i.e. (column, row); (0, 0) when no cell is legal.
// k_trilaterate: MINPACK hybrj per group (ofp_hybrj.h), one lane per group.
// k_locate_rows: the per-row front of ofp_locate_groups: earliest three channels, is_legal on both pairs and the
//                legality search, one workgroup per row.
// k_locate_solve: the back: trilaterate (or the model's output * 100) per row, one lane per row.  Both serve the 2-D
//                Multilaterate as well (LocateArgs::planar: its trilaterate keeps the sensors' order).
// k_locate_stream: Multilaterate3D.locate itself (or the 2-D Multilaterate.locate), K calls through one
//                device-resident state (ofp_locate_dev.h: loc_feed_kind), one workgroup.
// k_section:     Multilaterate3D.locate's cross-correlation input (multilateration.py:466-476): median filter of
//                size 5 ('reflect') along time, first difference, non-negative values zeroed, absolute value.
// The rules these kernels share with the state machine are written once in ofp_locate_dev.h: loc_cell (flat index ->
// cell -> guess), loc_reorder_3d, loc_tdoa (the system and each kind's delta rule), section_value.
#include <cmath>
#include <cstring>

#include "ofp_common.h"
#include "ofp_hybrj.h"
#include "ofp_locate_dev.h"
#include "ofp_mlp.h"

namespace {

using ofp::cdiv;
using ofp::first_legal;  // ofp_locate_dev.h

constexpr int LOC_THREADS = 256;

__device__ __forceinline__ double dist0(double x, double y, const double* s) {
    const double dx = x - s[0], dy = y - s[1], dz = 0.0 - s[2];
    return sqrt(dx * dx + dy * dy + dz * dz);
}

__global__ void k_lag_maps(const double* __restrict__ sensors, int S, int r, double c, double sr, double mask_r2,
                           double floor_v, float* __restrict__ maps) {
    const int side = 2 * r + 1;
    const int64_t cells = (int64_t)side * side;
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int pair = blockIdx.y;
    if (k >= cells) return;
    const int i = pair / S, j = pair % S;
    float* out = maps + (int64_t)pair * cells;
    if (i == j) {
        out[k] = __builtin_nanf("");
        return;
    }
    const int row = (int)(k / side), col = (int)(k % side);
    const int64_t gi = col - r, gj = row - r;  // np.meshgrid: i on columns, j on rows
    const double x = (double)gi, y = (double)gj;
    const double la = dist0(x, y, sensors + 3 * j) / c;
    const double lb = dist0(x, y, sensors + 3 * i) / c;
    float v = (float)rint((la - lb) * sr);
    if ((double)(gi * gi + gj * gj) > mask_r2) v = __builtin_nanf("");
    if ((double)v < floor_v) v = __builtin_nanf("");
    out[k] = v;
}

__global__ void k_lag_minmax(const float* __restrict__ maps, int64_t cells, float* __restrict__ d_min,
                             float* __restrict__ d_max) {
    __shared__ float smin[LOC_THREADS], smax[LOC_THREADS];
    const float* m = maps + (int64_t)blockIdx.x * cells;
    const float inf = __builtin_inff();
    float lo = inf, hi = -inf;
    for (int64_t k = threadIdx.x; k < cells; k += blockDim.x) {
        const float v = m[k];
        if (v == v) {
            lo = fminf(lo, v);
            hi = fmaxf(hi, v);
        }
    }
    smin[threadIdx.x] = lo;
    smax[threadIdx.x] = hi;
    __syncthreads();
    for (int s = blockDim.x / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
            smin[threadIdx.x] = fminf(smin[threadIdx.x], smin[threadIdx.x + s]);
            smax[threadIdx.x] = fmaxf(smax[threadIdx.x], smax[threadIdx.x + s]);
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const bool any = smin[0] != inf;  // np.nanmin of an all-NaN map is NaN
        d_min[blockIdx.x] = any ? smin[0] : __builtin_nanf("");
        d_max[blockIdx.x] = any ? smax[0] : __builtin_nanf("");
    }
}

__global__ void k_legal(const float* __restrict__ maps, int S, int side, const int32_t* __restrict__ sens,
                        const int64_t* __restrict__ onsets, double tol, int32_t* __restrict__ idx) {
    __shared__ int64_t smin[LOC_THREADS];
    const int64_t g = blockIdx.x;
    const int s0 = sens[3 * g], s1 = sens[3 * g + 1], s2 = sens[3 * g + 2];
    if (s0 < 0 || s0 >= S || s1 < 0 || s1 >= S || s2 < 0 || s2 >= S) {  // uniform over the block
        if (threadIdx.x == 0) idx[2 * g] = idx[2 * g + 1] = -1;
        return;
    }
    const double lag1 = (double)(onsets[3 * g + 1] - onsets[3 * g]);
    const double lag2 = (double)(onsets[3 * g + 2] - onsets[3 * g]);
    const int64_t k = first_legal(maps, S, side, s0, s1, s2, lag1, lag2, tol, smin);
    if (threadIdx.x == 0) {
        const ofp::LocCell cell = ofp::loc_cell(k, side);
        idx[2 * g] = (int32_t)cell.ix;
        idx[2 * g + 1] = (int32_t)cell.iy;
    }
}

__global__ void k_trilaterate(const double* __restrict__ geom, const double* __restrict__ delta,
                              const double* __restrict__ guess, int64_t G, double xtol, int maxfev,
                              double* __restrict__ root, int32_t* __restrict__ ier, int32_t* __restrict__ nfev) {
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= G) return;
    ofp::hybrj::Tdoa t;
    for (int k = 0; k < 3; ++k) {
        t.o[k] = geom[9 * g + k];
        t.a[k] = geom[9 * g + 3 + k];
        t.b[k] = geom[9 * g + 6 + k];
    }
    t.dda = delta[2 * g];
    t.ddb = delta[2 * g + 1];
    const double x0[2] = {guess[2 * g], guess[2 * g + 1]};
    const ofp::hybrj::Result res = ofp::hybrj::solve(t, x0, xtol, maxfev);
    root[2 * g] = res.x[0];
    root[2 * g + 1] = res.x[1];
    if (ier) ier[g] = res.info;
    if (nfev) nfev[g] = res.nfev;
}

// Per-row state of ofp_locate_groups kept in the work space between its kernels.
struct RowState {
    int32_t sens[3];   // origin, a, b after trilaterate's reordering
    int32_t status;    // OFP_LOCATE_* (< 0) or 0 = to be solved
    int64_t on[3];
    double guess[2];
};

struct LocateArgs {
    const int64_t* groups;
    int64_t n_clips, cap_groups;
    int C;
    const int64_t* n_groups;
    const double* sensors;
    int S;
    const float* maps;
    const float* min_lags;
    const float* max_lags;
    int side;
    double tol, sr, c, radius, xtol;
    int maxfev;
    int planar;  // 1: the 2-D Multilaterate's trilaterate (no reordering, delta = lag * c / sr)
    RowState* rows;
    float* lags;
};

__global__ void k_locate_rows(LocateArgs A) {
    __shared__ int64_t smin[LOC_THREADS];
    __shared__ RowState st;
    const int64_t row = blockIdx.x;
    const int64_t clip = row / A.cap_groups, gi = row % A.cap_groups;
    if (threadIdx.x == 0) {
        RowState s;
        s.status = 0;
        s.guess[0] = s.guess[1] = __builtin_nan("");
        int64_t ng = A.n_groups ? A.n_groups[clip] : A.cap_groups;
        ng = ng < A.cap_groups ? ng : A.cap_groups;
        int n = 0;
        if (gi >= ng) {
            s.status = OFP_LOCATE_UNUSED;
        } else {
            // the three earliest present channels, ordered by onset, ties by channel
            const int64_t* g = A.groups + row * A.C;
            int ch[3] = {-1, -1, -1};
            int64_t on[3] = {0, 0, 0};
            for (int cc = 0; cc < A.C; ++cc) {
                const int64_t v = g[cc];
                if (v < 0) continue;
                int p = n < 3 ? n : 3;
                while (p > 0 && on[p - 1] > v) --p;
                if (p >= 3) continue;
                for (int q = (n < 3 ? n : 2); q > p; --q) {
                    on[q] = on[q - 1];
                    ch[q] = ch[q - 1];
                }
                on[p] = v;
                ch[p] = cc;
                ++n;
            }
            for (int k = 0; k < 3; ++k) {
                s.sens[k] = ch[k];
                s.on[k] = on[k];
            }
            if (n < 3) {
                s.status = OFP_LOCATE_FEW_CHANNELS;
            } else {
                const int o = ch[0];
                const double l1 = (double)(on[1] - on[0]), l2 = (double)(on[2] - on[0]);
                const int64_t p1 = (int64_t)o * A.S + ch[1], p2 = (int64_t)o * A.S + ch[2];
                const bool ok1 = (double)A.min_lags[p1] < l1 && l1 < (double)A.max_lags[p1];
                const bool ok2 = (double)A.min_lags[p2] < l2 && l2 < (double)A.max_lags[p2];
                if (!(ok1 && ok2)) s.status = OFP_LOCATE_ILLEGAL_LAG;
            }
        }
        st = s;
    }
    __syncthreads();
    RowState s = st;
    if (s.status == 0) {
        const ofp::LocCell cell = ofp::loc_cell(
            first_legal(A.maps, A.S, A.side, s.sens[0], s.sens[1], s.sens[2], (double)(s.on[1] - s.on[0]),
                        (double)(s.on[2] - s.on[0]), A.tol, smin),
            A.side);
        if (cell.none()) {
            s.status = OFP_LOCATE_NO_CELL;
        } else {
            cell.guess(A.radius, s.guess);
            if (!A.planar) ofp::loc_reorder_3d(s.sens, s.on);
        }
    }
    if (threadIdx.x == 0) {
        A.rows[row] = s;
        A.lags[2 * row] = s.status == 0 ? (float)(s.on[1] - s.on[0]) : 0.0f;
        A.lags[2 * row + 1] = s.status == 0 ? (float)(s.on[2] - s.on[0]) : 0.0f;
    }
}

__global__ void k_locate_solve(LocateArgs A, int64_t n_rows, const float* __restrict__ model_out,
                               double* __restrict__ xy, int32_t* __restrict__ status, double* __restrict__ guess) {
    const int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= n_rows) return;
    const RowState s = A.rows[row];
    if (guess) {
        guess[2 * row] = s.guess[0];
        guess[2 * row + 1] = s.guess[1];
    }
    if (s.status != 0) {
        xy[2 * row] = xy[2 * row + 1] = __builtin_nan("");
        status[row] = s.status;
        return;
    }
    if (model_out) {  // self.model.call_np((d_a1, d_b1)) * 100: a float32 product
        xy[2 * row] = (double)(model_out[2 * row] * 100.0f);
        xy[2 * row + 1] = (double)(model_out[2 * row + 1] * 100.0f);
        status[row] = 1;
        return;
    }
    const ofp::hybrj::Tdoa t = ofp::loc_tdoa(A.sensors, s.sens, s.on, A.sr, A.c, A.planar != 0);
    const ofp::hybrj::Result res = ofp::hybrj::solve(t, s.guess, A.xtol, A.maxfev);
    xy[2 * row] = res.x[0];
    xy[2 * row + 1] = res.x[1];
    status[row] = res.info;
}

__global__ void k_section(const float* __restrict__ x, int64_t n, int ld, int c0, int c1, float* __restrict__ out) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int which = blockIdx.y;
    if (t >= n - 1) return;
    const int col = which == 0 ? c0 : c1;
    out[(int64_t)which * (n - 1) + t] = ofp::section_value([&](int64_t u) { return x[u * ld + col]; }, n, t);
}

// The replay entry: K calls of locate through one state machine, one workgroup (ofp_locate_dev.h).
__global__ __launch_bounds__(LOC_THREADS) void k_locate_stream(ofp::LocTables T, const int32_t* __restrict__ sensor,
                                                               const int64_t* __restrict__ onset,
                                                               const int64_t* __restrict__ counter, int64_t K,
                                                               const float* __restrict__ audio, int64_t n_rows, int C,
                                                               ofp_locate_state* state, int32_t* __restrict__ found,
                                                               double* __restrict__ xy) {
    extern __shared__ __align__(16) unsigned char loc_smem[];
    const ofp::LocView v = ofp::loc_carve(loc_smem, LOC_THREADS, T.max_section, T.plan);
    ofp::loc_load(T, v, nullptr);
    auto sample = [&](int64_t t, int col) -> float { return t >= 0 && t < n_rows ? audio[t * C + col] : 0.0f; };
    for (int64_t k = 0; k < K; ++k) {
        const int s = sensor[k];
        const int64_t cnt = counter ? counter[k] : 0;  // (the planar kind has no counter)
        double r[2] = {__builtin_nan(""), __builtin_nan("")};
        int f = 0;
        if (s < 0 || s >= T.S || (T.use_audio && (cnt < 0 || cnt > n_rows))) {  // uniform over the workgroup
            __syncthreads();
            if (threadIdx.x == 0) v.L->st[v.L->cur].flags |= OFP_LOCF_BAD_CALL;
            __syncthreads();
        } else {
            f = ofp::loc_feed_kind(T, v, s, onset[k], cnt, false, sample, r, nullptr);
        }
        if (threadIdx.x == 0) {
            found[k] = f;
            xy[2 * k] = f ? r[0] : __builtin_nan("");
            xy[2 * k + 1] = f ? r[1] : __builtin_nan("");
        }
    }
    ofp::loc_store(v, state);
}

}  // namespace

int ofp_locate_tables(const ofp_hop_locator* loc, const char* who, ofp::LocTables* out) {
    OFP_REQUIRE(loc, "%s: NULL locator", who);
    OFP_REQUIRE(loc->S >= 3 && loc->S <= 64, "%s: need 3..64 sensors (S = %d)", who, loc->S);
    OFP_REQUIRE(loc->r >= 0 && loc->r <= 4096, "%s: grid radius %d outside 0..4096", who, loc->r);
    OFP_REQUIRE(loc->d_sensors && loc->d_maps && loc->d_min && loc->d_max, "%s: NULL table", who);
    OFP_REQUIRE(loc->xtol >= 0.0 && loc->maxfev > 0, "%s: xtol must be >= 0 and maxfev > 0", who);
    OFP_REQUIRE(loc->sr > 0.0 && loc->c > 0.0 && loc->samples_per_cm > 0.0,
                "%s: speed of sound, sampling rate and samples per cm must be positive", who);
    OFP_REQUIRE(!loc->use_audio || (loc->max_section >= 3 && loc->max_section <= ofp::LOC_MAX_SECTION),
                "%s: max_section %d outside 3..%d", who, loc->max_section, ofp::LOC_MAX_SECTION);
    ofp::LocTables& T = *out;
    std::memset(&T, 0, sizeof(T));
    if (loc->mlp) {
        const MlpPlan& P = loc->mlp->plan;
        OFP_REQUIRE(P.dims[0] == 2 && P.dims[P.n_layers] == 2,
                    "%s: the network must map 2 lags to 2 coordinates (got %d -> %d)", who, P.dims[0],
                    P.dims[P.n_layers]);
        T.plan = P;
        T.plan.params = loc->mlp->d_params;
    }
    T.sensors = loc->d_sensors;
    T.S = loc->S;
    T.maps = loc->d_maps;
    T.mn = loc->d_min;
    T.mx = loc->d_max;
    T.side = 2 * loc->r + 1;
    T.spc = loc->samples_per_cm;
    T.sr = loc->sr;
    T.c = loc->c;
    T.radius = loc->radius;
    T.xtol = loc->xtol;
    T.maxfev = loc->maxfev;
    T.use_audio = loc->use_audio ? 1 : 0;
    T.max_section = loc->use_audio ? loc->max_section : 4;
    return OFP_OK;
}

int ofp_locate_tables_2d(const ofp_hop_locator* loc, const char* who, ofp::LocTables* out) {
    OFP_REQUIRE(loc, "%s: NULL locator", who);
    OFP_REQUIRE(!loc->mlp, "%s: the planar locator has no model path", who);
    ofp_hop_locator plain = *loc;
    plain.use_audio = 0;
    plain.max_section = 0;
    if (int rc = ofp_locate_tables(&plain, who, out)) return rc;
    out->planar = 1;
    return OFP_OK;
}

extern "C" {

int ofp_lag_maps(const double* d_sensors, int32_t S, int32_t r, double c, double sr, double mask_r2, double floor_v,
                 float* d_maps, float* d_min, float* d_max, void* stream) {
    OFP_REQUIRE(S >= 2 && S <= 64, "ofp_lag_maps: need 2..64 sensors (S = %d)", S);
    OFP_REQUIRE(r >= 0 && r <= 4096, "ofp_lag_maps: grid radius %d outside 0..4096", r);
    OFP_REQUIRE(d_sensors && d_maps, "ofp_lag_maps: NULL argument");
    OFP_REQUIRE((d_min == nullptr) == (d_max == nullptr), "ofp_lag_maps: give both d_min and d_max or neither");
    OFP_REQUIRE(c > 0.0 && sr > 0.0, "ofp_lag_maps: speed of sound and sampling rate must be positive");
    const int side = 2 * r + 1;
    const int64_t cells = (int64_t)side * side;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_lag_maps, dim3((unsigned)cdiv(cells, LOC_THREADS), (unsigned)(S * S)), dim3(LOC_THREADS), 0, s,
                       d_sensors, S, r, c, sr, mask_r2, floor_v, d_maps);
    OFP_LAUNCH_CHECK("k_lag_maps");
    if (d_min) {
        hipLaunchKernelGGL(k_lag_minmax, dim3((unsigned)(S * S)), dim3(LOC_THREADS), 0, s, d_maps, cells, d_min, d_max);
        OFP_LAUNCH_CHECK("k_lag_minmax");
    }
    return OFP_OK;
}

int ofp_locate_legal(const float* d_maps, int32_t S, int32_t r, const int32_t* d_sensors, const int64_t* d_onsets,
                     int64_t G, double tolerance, int32_t* d_idx, void* stream) {
    OFP_REQUIRE(S >= 2, "ofp_locate_legal: need at least two sensors (S = %d)", S);
    OFP_REQUIRE(r >= 0 && r <= 4096, "ofp_locate_legal: grid radius %d outside 0..4096", r);
    OFP_REQUIRE(G >= 0, "ofp_locate_legal: negative group count");
    if (G == 0) return OFP_OK;
    OFP_REQUIRE(d_maps && d_sensors && d_onsets && d_idx, "ofp_locate_legal: NULL argument");
    OFP_REQUIRE(G <= 0x7fffffff, "ofp_locate_legal: more than 2^31 - 1 groups");
    hipLaunchKernelGGL(k_legal, dim3((unsigned)G), dim3(LOC_THREADS), 0, (hipStream_t)stream, d_maps, S, 2 * r + 1,
                       d_sensors, d_onsets, tolerance, d_idx);
    OFP_LAUNCH_CHECK("k_legal");
    return OFP_OK;
}

int ofp_trilaterate(const double* d_geom, const double* d_delta, const double* d_guess, int64_t G, double xtol,
                    int32_t maxfev, double* d_root, int32_t* d_ier, int32_t* d_nfev, void* stream) {
    OFP_REQUIRE(G >= 0, "ofp_trilaterate: negative group count");
    OFP_REQUIRE(xtol >= 0.0 && maxfev > 0, "ofp_trilaterate: xtol must be >= 0 and maxfev > 0");
    if (G == 0) return OFP_OK;
    OFP_REQUIRE(d_geom && d_delta && d_guess && d_root, "ofp_trilaterate: NULL argument");
    hipLaunchKernelGGL(k_trilaterate, dim3((unsigned)cdiv(G, 64)), dim3(64), 0, (hipStream_t)stream, d_geom, d_delta,
                       d_guess, G, xtol, (int)maxfev, d_root, d_ier, d_nfev);
    OFP_LAUNCH_CHECK("k_trilaterate");
    return OFP_OK;
}

int64_t ofp_locate_workspace_bytes(int64_t n_rows) {
    if (n_rows < 0) return -1;
    return ofp::align_up(n_rows * (int64_t)sizeof(RowState), 256) + 2 * ofp::align_up(n_rows * 2 * 4, 256);
}

// ofp_locate_groups and ofp_locate_groups_2d: the same two kernels, the kind in LocateArgs::planar
static int locate_groups(const char* who, int planar, const int64_t* d_groups, int64_t n_clips, int64_t cap_groups,
                         int32_t n_channels, const int64_t* d_n_groups, const double* d_sensors, int32_t S,
                         const float* d_maps, const float* d_min, const float* d_max, int32_t r, double tolerance,
                         double sr, double c, double radius, double xtol, int32_t maxfev, const ofp_mlp* mlp,
                         double* d_xy, int32_t* d_status, double* d_guess, void* d_ws, int64_t ws_bytes,
                         void* stream) {
    OFP_REQUIRE(S >= 2, "%s: need at least two sensors (S = %d)", who, S);
    OFP_REQUIRE(n_channels >= 1 && n_channels <= S,
                "%s: n_channels %d must be in 1..S (channel k is sensor k, S = %d)", who, n_channels, S);
    OFP_REQUIRE(r >= 0 && r <= 4096, "%s: grid radius %d outside 0..4096", who, r);
    OFP_REQUIRE(n_clips >= 0 && cap_groups >= 0, "%s: negative n_clips or cap_groups", who);
    OFP_REQUIRE(xtol >= 0.0 && maxfev > 0, "%s: xtol must be >= 0 and maxfev > 0", who);
    OFP_REQUIRE(sr > 0.0 && c > 0.0, "%s: speed of sound and sampling rate must be positive", who);
    const int64_t n_rows = n_clips * cap_groups;
    if (n_rows == 0) return OFP_OK;
    OFP_REQUIRE(n_rows <= 0x7fffffff, "%s: more than 2^31 - 1 rows", who);
    OFP_REQUIRE(d_groups && d_sensors && d_maps && d_min && d_max && d_xy && d_status && d_ws,
                "%s: NULL argument", who);
    OFP_REQUIRE(ws_bytes >= ofp_locate_workspace_bytes(n_rows), "%s: work space of %lld bytes < %lld", who,
                (long long)ws_bytes, (long long)ofp_locate_workspace_bytes(n_rows));
    if (mlp) {
        const MlpPlan& P = mlp->plan;
        OFP_REQUIRE(P.dims[0] == 2 && P.dims[P.n_layers] == 2,
                    "%s: the network must map 2 lags to 2 coordinates (got %d -> %d)", who, P.dims[0],
                    P.dims[P.n_layers]);
    }
    char* ws = (char*)d_ws;
    LocateArgs A;
    A.groups = d_groups;
    A.n_clips = n_clips;
    A.cap_groups = cap_groups;
    A.C = n_channels;
    A.n_groups = d_n_groups;
    A.sensors = d_sensors;
    A.S = S;
    A.maps = d_maps;
    A.min_lags = d_min;
    A.max_lags = d_max;
    A.side = 2 * r + 1;
    A.tol = tolerance;
    A.sr = sr;
    A.c = c;
    A.radius = radius;
    A.xtol = xtol;
    A.maxfev = maxfev;
    A.planar = planar;
    A.rows = (RowState*)ws;
    A.lags = (float*)(ws + ofp::align_up(n_rows * (int64_t)sizeof(RowState), 256));
    float* model_out = A.lags + ofp::align_up(n_rows * 2 * 4, 256) / 4;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_locate_rows, dim3((unsigned)n_rows), dim3(LOC_THREADS), 0, s, A);
    OFP_LAUNCH_CHECK("k_locate_rows");
    if (mlp) {
        const int rc = ofp_mlp_forward(mlp, A.lags, n_rows, model_out, stream);
        if (rc != OFP_OK) return rc;
    }
    hipLaunchKernelGGL(k_locate_solve, dim3((unsigned)cdiv(n_rows, 64)), dim3(64), 0, s, A, n_rows,
                       mlp ? (const float*)model_out : nullptr, d_xy, d_status, d_guess);
    OFP_LAUNCH_CHECK("k_locate_solve");
    return OFP_OK;
}

int ofp_locate_groups(const int64_t* d_groups, int64_t n_clips, int64_t cap_groups, int32_t n_channels,
                      const int64_t* d_n_groups, const double* d_sensors, int32_t S, const float* d_maps,
                      const float* d_min, const float* d_max, int32_t r, double tolerance, double sr, double c,
                      double radius, double xtol, int32_t maxfev, const ofp_mlp* mlp, double* d_xy,
                      int32_t* d_status, double* d_guess, void* d_ws, int64_t ws_bytes, void* stream) {
    return locate_groups("ofp_locate_groups", 0, d_groups, n_clips, cap_groups, n_channels, d_n_groups, d_sensors, S,
                         d_maps, d_min, d_max, r, tolerance, sr, c, radius, xtol, maxfev, mlp, d_xy, d_status, d_guess,
                         d_ws, ws_bytes, stream);
}

int ofp_locate_groups_2d(const int64_t* d_groups, int64_t n_clips, int64_t cap_groups, int32_t n_channels,
                         const int64_t* d_n_groups, const double* d_sensors, int32_t S, const float* d_maps,
                         const float* d_min, const float* d_max, int32_t r, double tolerance, double sr, double c,
                         double radius, double xtol, int32_t maxfev, double* d_xy, int32_t* d_status,
                         double* d_guess, void* d_ws, int64_t ws_bytes, void* stream) {
    return locate_groups("ofp_locate_groups_2d", 1, d_groups, n_clips, cap_groups, n_channels, d_n_groups, d_sensors,
                         S, d_maps, d_min, d_max, r, tolerance, sr, c, radius, xtol, maxfev, nullptr, d_xy, d_status,
                         d_guess, d_ws, ws_bytes, stream);
}

int ofp_locate_section(const float* d_x, int64_t n, int32_t ld, int32_t c0, int32_t c1, float* d_out, void* stream) {
    OFP_REQUIRE(n >= 3, "ofp_locate_section: need at least 3 rows (got %lld)", (long long)n);
    OFP_REQUIRE(ld >= 1 && c0 >= 0 && c0 < ld && c1 >= 0 && c1 < ld,
                "ofp_locate_section: columns %d, %d outside a row of %d", c0, c1, ld);
    OFP_REQUIRE(d_x && d_out, "ofp_locate_section: NULL argument");
    hipLaunchKernelGGL(k_section, dim3((unsigned)cdiv(n - 1, LOC_THREADS), 2), dim3(LOC_THREADS), 0,
                       (hipStream_t)stream, d_x, n, ld, c0, c1, d_out);
    OFP_LAUNCH_CHECK("k_section");
    return OFP_OK;
}

// ofp_locate_stream and ofp_locate_stream_2d: one launch of k_locate_stream on tables their caller has checked
static int locate_stream(const char* who, const ofp::LocTables& T, const int32_t* d_sensor, const int64_t* d_onset,
                         const int64_t* d_counter, int64_t K, const float* d_audio, int64_t n_rows, int32_t n_channels,
                         ofp_locate_state* d_state, int32_t* d_found, double* d_xy, void* stream) {
    OFP_REQUIRE(K >= 0, "%s: negative call count", who);
    OFP_REQUIRE(d_state, "%s: NULL state", who);
    if (K == 0) return OFP_OK;
    OFP_REQUIRE(d_sensor && d_onset && (d_counter || T.planar) && d_found && d_xy, "%s: NULL argument", who);
    const size_t lds = ofp::loc_lds_bytes(LOC_THREADS, T.max_section, T.plan);
    OFP_REQUIRE(lds <= 150 * 1024, "%s: %zu bytes of LDS needed", who, lds);
    static ofp::LdsAttrCache attr;
    if (int rc = ofp::ensure_dynamic_lds(reinterpret_cast<const void*>(k_locate_stream), lds, attr, 32768)) return rc;
    hipLaunchKernelGGL(k_locate_stream, dim3(1), dim3(LOC_THREADS), lds, (hipStream_t)stream, T, d_sensor, d_onset,
                       d_counter, K, d_audio, n_rows, (int)n_channels, d_state, d_found, d_xy);
    OFP_LAUNCH_CHECK("k_locate_stream");
    return OFP_OK;
}

int ofp_locate_stream(const ofp_hop_locator* loc, const int32_t* d_sensor, const int64_t* d_onset,
                      const int64_t* d_counter, int64_t K, const float* d_audio, int64_t n_rows, int32_t n_channels,
                      ofp_locate_state* d_state, int32_t* d_found, double* d_xy, void* stream) {
    ofp::LocTables T;
    if (int rc = ofp_locate_tables(loc, "ofp_locate_stream", &T)) return rc;
    OFP_REQUIRE((d_audio != nullptr) == (loc->use_audio != 0),
                "ofp_locate_stream: use_audio and the recording must be given together");
    OFP_REQUIRE(!d_audio || (n_rows >= 0 && n_channels >= loc->S),
                "ofp_locate_stream: the recording has %d channels for %d sensors", n_channels, loc->S);
    return locate_stream("ofp_locate_stream", T, d_sensor, d_onset, d_counter, K, d_audio, n_rows, n_channels, d_state,
                         d_found, d_xy, stream);
}

int ofp_locate_stream_2d(const ofp_hop_locator* loc, const int32_t* d_sensor, const int64_t* d_onset, int64_t K,
                         ofp_locate_state* d_state, int32_t* d_found, double* d_xy, void* stream) {
    ofp::LocTables T;
    if (int rc = ofp_locate_tables_2d(loc, "ofp_locate_stream_2d", &T)) return rc;
    return locate_stream("ofp_locate_stream_2d", T, d_sensor, d_onset, nullptr, K, nullptr, 0, 0, d_state, d_found,
                         d_xy, stream);
}

}  // extern "C"
