// Recurrent layers and the attention head of model.RNN / model.CNNRNN (model.py:168-440), eval mode.
//
// k_rnn_layer: one (layer, direction) of nn.GRU / nn.LSTM / nn.RNN with zero initial state as ONE
// persistent launch.  A workgroup owns a tile of 16 sequences and walks all T steps: h lives in LDS
// (double-buffered, one barrier per step), W_hh stays in LDS for the whole sequence when it fits
// (otherwise it is streamed from L2 every step), and h W_hhᵀ runs on v_mfma_f32_16x16x4_f32.  The
// waves split the hidden units in tiles of 16 and compute every gate of their units, so the cell
// update is lane-local: lane l owns units j = tile*16 + (l&15) of sequences (l>>4)*4 + r, and keeps
// their c (LSTM) and previous h in registers.  The input projection x W_ihᵀ + b_ih is either computed
// inline (narrow inputs, <= 8 features: one MFMA per gate and step) or read from a buffer the caller
// filled with ofp_dense (wide inputs).  Every output element depends only on its own sequence.
//
// k_layernorm: nn.LayerNorm over the last axis, one wave per row.
// k_attn_mean: nn.MultiheadAttention self-attention (softmax(QKᵀ/√d)·V per head) followed by the mean
// over time, one workgroup per (sequence, head); its waves take query tiles of 16 and stream the keys
// in tiles of 16 with an online softmax, so any T works.  out_proj and fc commute with the mean and run
// afterwards on [n, E] with ofp_dense.
#include <algorithm>

#include "ofp_common.h"
#include "ofp_mlp.h"

namespace {

using ofp::cdiv;
typedef ofp_f32x4 f32x4;

constexpr int RNN_WAVES = 4;
constexpr int RNN_MAX_H = 256;
constexpr int RNN_MAX_INLINE = 8;  // inputs up to this width are projected inline
constexpr size_t LDS_MAX = 160 * 1024;

__host__ __device__ constexpr int cell_gates(int cell) {
    return cell == OFP_CELL_GRU ? 3 : cell == OFP_CELL_LSTM ? 4 : 1;
}

__device__ __forceinline__ float sigm(float v) { return 1.0f / (1.0f + expf(-v)); }

struct RnnArgs {
    int64_t n_seq;
    int T, in, H, reverse;
    const float* x;
    int64_t x_seq, x_t, x_f;
    const float* gx;
    int64_t gx_seq, gx_t;
    const float* w_ih;
    const float* b_ih;
    const float* w_hh;
    const float* b_hh;
    float* y;
    int64_t y_seq, y_t;
    int y_off;
    int kh;       // H rounded up to 16
    int st;       // LDS row stride (floats) of h and W_hh: kh + 4
    int w_vec;    // W_hh rows may be read as float4 (H % 4 == 0, 16-byte aligned)
};

// W_hh[row][k .. k+3] for the streamed path (zero outside [H) x [H))
__device__ __forceinline__ float4 whh_global(const RnnArgs& a, int row_ok, int64_t row, int k) {
    float4 b = make_float4(0.f, 0.f, 0.f, 0.f);
    if (!row_ok) return b;
    const float* wr = a.w_hh + row * a.H;
    if (a.w_vec && k + 3 < a.H) return *reinterpret_cast<const float4*>(wr + k);
    if (k < a.H) b.x = wr[k];
    if (k + 1 < a.H) b.y = wr[k + 1];
    if (k + 2 < a.H) b.z = wr[k + 2];
    if (k + 3 < a.H) b.w = wr[k + 3];
    return b;
}

// CELL: OFP_CELL_*; NT: hidden tiles of 16 per wave; WLDS: W_hh resident in LDS; GX: input projection
// precomputed by the caller.  LDS: h [2][16][st], then (WLDS) W_hh [G][kh][st], zero-padded.
template <int CELL, int NT, bool WLDS, bool GX>
__global__ __launch_bounds__(64 * RNN_WAVES) void k_rnn_layer(RnnArgs a) {
    constexpr int G = cell_gates(CELL);
    extern __shared__ __align__(16) float sm[];
    const int st = a.st, kh = a.kh, H = a.H;
    float* hbuf = sm;
    float* wl = sm + 32 * st;
    for (int i = threadIdx.x; i < 32 * st; i += blockDim.x) hbuf[i] = 0.0f;
    if (WLDS) {
        for (int i = threadIdx.x; i < G * kh * st; i += blockDim.x) {
            const int row = i / st, k = i - row * st;
            const int g = row / kh, j = row - g * kh;
            wl[i] = (j < H && k < H) ? a.w_hh[(int64_t)(g * H + j) * H + k] : 0.0f;
        }
    }
    __syncthreads();

    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const int li = lane & 15, lk = lane >> 4;
    const int64_t s0 = (int64_t)blockIdx.x * 16;
    const int64_t seq_a = s0 + li;  // the sequence this lane loads A-fragment inputs for
    const bool seq_a_ok = seq_a < a.n_seq;

    float c[NT][4], hp[NT][4], bh[NT][G], bi[NT][G], wi[NT][G][2];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const int j = (w + nt * nw) * 16 + li;
        const bool jok = j < H;
#pragma unroll
        for (int r = 0; r < 4; ++r) c[nt][r] = hp[nt][r] = 0.0f;
#pragma unroll
        for (int g = 0; g < G; ++g) {
            bh[nt][g] = (jok && a.b_hh) ? a.b_hh[g * H + j] : 0.0f;
            bi[nt][g] = (!GX && jok && a.b_ih) ? a.b_ih[g * H + j] : 0.0f;
#pragma unroll
            for (int kc = 0; kc < 2; ++kc) {
                const int k = kc * 4 + lk;
                wi[nt][g][kc] = (!GX && jok && k < a.in) ? a.w_ih[(int64_t)(g * H + j) * a.in + k] : 0.0f;
            }
        }
    }

    // inputs of one step: inline, the A fragment x[seq_a][t][kc*4 + lk]; precomputed, gx of the lane's
    // four sequences and units
    float xa[2], xn[2];
    float ga[NT][G][4], gn[NT][G][4];
    auto load_inputs = [&](int t, float (&xv)[2], float (&gv)[NT][G][4]) {
        if (!GX) {
#pragma unroll
            for (int kc = 0; kc < 2; ++kc) {
                const int k = kc * 4 + lk;
                xv[kc] = (seq_a_ok && k < a.in) ? a.x[seq_a * a.x_seq + (int64_t)t * a.x_t + (int64_t)k * a.x_f] : 0.0f;
            }
        } else {
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const int j = (w + nt * nw) * 16 + li;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int64_t s = s0 + lk * 4 + r;
                    const bool ok = j < H && s < a.n_seq;
                    const float* src = a.gx + s * a.gx_seq + (int64_t)t * a.gx_t + j;
#pragma unroll
                    for (int g = 0; g < G; ++g) gv[nt][g][r] = ok ? src[g * H] : 0.0f;
                }
            }
        }
    };
    load_inputs(a.reverse ? a.T - 1 : 0, xa, ga);

#pragma unroll 1
    for (int step = 0; step < a.T; ++step) {
        const int t = a.reverse ? a.T - 1 - step : step;
        const float* hc = hbuf + (step & 1) * 16 * st;
        float* hn = hbuf + ((step + 1) & 1) * 16 * st;
        if (step + 1 < a.T) load_inputs(a.reverse ? t - 1 : t + 1, xn, gn);  // in flight during this step
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const int ht = w + nt * nw;
            if (ht * 16 >= kh) continue;  // wave-uniform
            const int j = ht * 16 + li;
            f32x4 ah[G], ax[G];
#pragma unroll
            for (int g = 0; g < G; ++g) ah[g] = ax[g] = f32x4{0.f, 0.f, 0.f, 0.f};
            // h W_hhᵀ: lane (li, lk) feeds k = k0 + lk*4 + 0..3 in four MFMAs (any k order sums the same terms)
#pragma unroll 1
            for (int k0 = 0; k0 < kh; k0 += 16) {
                const int k = k0 + lk * 4;
                const float4 av = *reinterpret_cast<const float4*>(hc + li * st + k);
#pragma unroll
                for (int g = 0; g < G; ++g) {
                    const float4 bv = WLDS ? *reinterpret_cast<const float4*>(wl + (g * kh + j) * st + k)
                                           : whh_global(a, j < H, (int64_t)g * H + j, k);
                    ah[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.x, bv.x, ah[g], 0, 0, 0);
                    ah[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.y, bv.y, ah[g], 0, 0, 0);
                    ah[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.z, bv.z, ah[g], 0, 0, 0);
                    ah[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.w, bv.w, ah[g], 0, 0, 0);
                }
            }
            if (!GX) {
#pragma unroll
                for (int g = 0; g < G; ++g) {
                    ax[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[0], wi[nt][g][0], ax[g], 0, 0, 0);
                    if (a.in > 4) ax[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[1], wi[nt][g][1], ax[g], 0, 0, 0);
#pragma unroll
                    for (int r = 0; r < 4; ++r) ax[g][r] += bi[nt][g];
                }
            } else {
#pragma unroll
                for (int g = 0; g < G; ++g)
#pragma unroll
                    for (int r = 0; r < 4; ++r) ax[g][r] = ga[nt][g][r];
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float h;
                if (CELL == OFP_CELL_GRU) {
                    const float rg = sigm(ax[0][r] + (ah[0][r] + bh[nt][0]));
                    const float z = sigm(ax[1][r] + (ah[1][r] + bh[nt][1]));
                    const float n = tanhf(ax[2][r] + rg * (ah[2][r] + bh[nt][2]));
                    h = n + z * (hp[nt][r] - n);
                } else if (CELL == OFP_CELL_LSTM) {
                    const float ig = sigm(ax[0][r] + (ah[0][r] + bh[nt][0]));
                    const float fg = sigm(ax[1][r] + (ah[1][r] + bh[nt][1]));
                    const float gg = tanhf(ax[2][r] + (ah[2][r] + bh[nt][2]));
                    const float og = sigm(ax[3][r] + (ah[3][r] + bh[nt][3]));
                    c[nt][r] = fg * c[nt][r] + ig * gg;
                    h = og * tanhf(c[nt][r]);
                } else {
                    const float v = ax[0][r] + (ah[0][r] + bh[nt][0]);
                    h = CELL == OFP_CELL_RNN_RELU ? fmaxf(v, 0.0f) : tanhf(v);
                }
                hp[nt][r] = h;
                if (j < H) {
                    hn[(lk * 4 + r) * st + j] = h;
                    const int64_t s = s0 + lk * 4 + r;
                    if (s < a.n_seq) a.y[s * a.y_seq + (int64_t)t * a.y_t + a.y_off + j] = h;
                }
            }
        }
        __syncthreads();
        if (!GX) {
            xa[0] = xn[0];
            xa[1] = xn[1];
        } else {
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                for (int g = 0; g < G; ++g)
#pragma unroll
                    for (int r = 0; r < 4; ++r) ga[nt][g][r] = gn[nt][g][r];
        }
    }
}

template <int CELL, int NT, bool WLDS, bool GX>
int launch_rnn(const RnnArgs& a, size_t lds, int threads, hipStream_t stream) {
    static ofp::LdsAttrCache attr;
    auto fn = k_rnn_layer<CELL, NT, WLDS, GX>;
    if (int rc = ofp::ensure_dynamic_lds(reinterpret_cast<const void*>(fn), lds, attr)) return rc;
    hipLaunchKernelGGL(fn, dim3((unsigned)cdiv(a.n_seq, 16)), dim3(threads), lds, stream, a);
    OFP_LAUNCH_CHECK("k_rnn_layer");
    return OFP_OK;
}

template <int CELL, int NT>
int launch_rnn_nt(const RnnArgs& a, bool wlds, size_t lds, int threads, hipStream_t s) {
    const bool gx = a.gx != nullptr;
    if (wlds) return gx ? launch_rnn<CELL, NT, true, true>(a, lds, threads, s) : launch_rnn<CELL, NT, true, false>(a, lds, threads, s);
    return gx ? launch_rnn<CELL, NT, false, true>(a, lds, threads, s) : launch_rnn<CELL, NT, false, false>(a, lds, threads, s);
}

template <int CELL>
int launch_rnn_cell(const RnnArgs& a, int nt, bool wlds, size_t lds, int threads, hipStream_t s) {
    if (nt == 1) return launch_rnn_nt<CELL, 1>(a, wlds, lds, threads, s);
    if (nt == 2) return launch_rnn_nt<CELL, 2>(a, wlds, lds, threads, s);
    return launch_rnn_nt<CELL, 4>(a, wlds, lds, threads, s);
}

// nn.LayerNorm over rows of E: one wave per row, two passes in fp32.
constexpr int LN_WAVES = 4;
__global__ __launch_bounds__(64 * LN_WAVES) void k_layernorm(const float* __restrict__ x, int64_t n, int E,
                                                             const float* __restrict__ gamma,
                                                             const float* __restrict__ beta, float eps,
                                                             float* __restrict__ y) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * LN_WAVES + (threadIdx.x >> 6);
    if (row >= n) return;
    const float* xr = x + row * E;
    float s = 0.0f;
    for (int i = lane; i < E; i += 64) s += xr[i];
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    const float mean = s / (float)E;
    float ss = 0.0f;
    for (int i = lane; i < E; i += 64) {
        const float d = xr[i] - mean;
        ss += d * d;
    }
    for (int o = 32; o > 0; o >>= 1) ss += __shfl_xor(ss, o);
    const float rstd = 1.0f / sqrtf(ss / (float)E + eps);
    float* yr = y + row * E;
    for (int i = lane; i < E; i += 64) {
        const float v = (xr[i] - mean) * rstd;
        yr[i] = v * (gamma ? gamma[i] : 1.0f) + (beta ? beta[i] : 0.0f);
    }
}

// Self-attention of one (sequence, head) and its mean over the T queries.  qkv [n][T][3E] (q | k | v as
// nn.MultiheadAttention's in-projection lays them out), head h uses columns h*d .. h*d + d - 1 of each.
// Fragments as k_dense: S = Q Kᵀ has rows = queries (lk*4 + r), columns = keys (li); P goes through a
// per-wave LDS tile to become the A operand of P·V.  DC: head dim in chunks of 4 (d <= 4*DC).
constexpr int ATT_WAVES = 4;
template <int DC>
__global__ __launch_bounds__(64 * ATT_WAVES) void k_attn_mean(const float* __restrict__ qkv, int T, int E, int nh,
                                                              int d, float scale, float* __restrict__ out) {
    constexpr int DT = (4 * DC + 15) / 16;  // column tiles of the context
    __shared__ float ptile[ATT_WAVES][16][17];
    __shared__ float part[ATT_WAVES][DT * 16];
    const int64_t seq = blockIdx.x / nh;
    const int head = blockIdx.x - (int)(seq * nh);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int li = lane & 15, lk = lane >> 4;
    const int64_t rs = 3 * (int64_t)E;
    const float* base = qkv + seq * T * rs;
    const float* qb = base + head * d;
    const float* kb = base + E + head * d;
    const float* vb = base + 2 * E + head * d;
    float colsum[DT];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) colsum[dt] = 0.0f;

    for (int qt = w; qt * 16 < T; qt += ATT_WAVES) {
        const int q = qt * 16 + li;
        float qa[DC];
#pragma unroll
        for (int kc = 0; kc < DC; ++kc) {
            const int k = kc * 4 + lk;
            qa[kc] = (q < T && k < d) ? qb[q * rs + k] : 0.0f;
        }
        float m[4], l[4];
        f32x4 o[DT];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            m[r] = -INFINITY;
            l[r] = 0.0f;
        }
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int kt = 0; kt * 16 < T; ++kt) {
            const int key = kt * 16 + li;
            f32x4 s = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int kc = 0; kc < DC; ++kc) {
                const int k = kc * 4 + lk;
                const float b = (key < T && k < d) ? kb[key * rs + k] : 0.0f;
                s = __builtin_amdgcn_mfma_f32_16x16x4f32(qa[kc], b, s, 0, 0, 0);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float v = key < T ? s[r] * scale : -INFINITY;
                float mx = v;
                for (int o2 = 1; o2 < 16; o2 <<= 1) mx = fmaxf(mx, __shfl_xor(mx, o2));
                const float mn = fmaxf(m[r], mx);  // finite: key 0 of every tile is valid
                const float alpha = expf(m[r] - mn);
                const float p = expf(v - mn);
                float ps = p;
                for (int o2 = 1; o2 < 16; o2 <<= 1) ps += __shfl_xor(ps, o2);
                l[r] = l[r] * alpha + ps;
                m[r] = mn;
#pragma unroll
                for (int dt = 0; dt < DT; ++dt) o[dt][r] *= alpha;
                ptile[w][lk * 4 + r][li] = p;
            }
            ofp_wave_lds_sync();
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) {
                const int col = dt * 16 + li;
#pragma unroll
                for (int k4 = 0; k4 < 4; ++k4) {
                    const int kv = kt * 16 + k4 * 4 + lk;
                    const float av = ptile[w][li][k4 * 4 + lk];
                    const float bv = (kv < T && col < d) ? vb[kv * rs + col] : 0.0f;
                    o[dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, o[dt], 0, 0, 0);
                }
            }
            ofp_wave_lds_sync();
        }
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) {
            float cs = 0.0f;
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (qt * 16 + lk * 4 + r < T) cs += o[dt][r] / l[r];
            cs += __shfl_xor(cs, 16);
            cs += __shfl_xor(cs, 32);
            colsum[dt] += cs;
        }
    }
    if (lane < 16) {
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) part[w][dt * 16 + li] = colsum[dt];
    }
    __syncthreads();
    for (int cidx = threadIdx.x; cidx < d; cidx += blockDim.x) {
        float v = 0.0f;
        for (int ww = 0; ww < ATT_WAVES; ++ww) v += part[ww][cidx];  // fixed order: batch-independent
        out[seq * E + head * d + cidx] = v / (float)T;
    }
}

template <int DC>
int launch_attn(const float* qkv, int64_t n, int T, int E, int nh, int d, float* out, hipStream_t s) {
    hipLaunchKernelGGL(k_attn_mean<DC>, dim3((unsigned)(n * nh)), dim3(64 * ATT_WAVES), 0, s, qkv, T, E, nh, d,
                       1.0f / sqrtf((float)d), out);
    OFP_LAUNCH_CHECK("k_attn_mean");
    return OFP_OK;
}

}  // namespace

extern "C" {

int64_t ofp_rnn_lds_bytes(int32_t cell, int32_t H) {
    if (cell < OFP_CELL_RNN_TANH || cell > OFP_CELL_LSTM || H < 1 || H > RNN_MAX_H) return -1;
    const int64_t kh = (H + 15) / 16 * 16, st = kh + 4;
    return (32 * st + cell_gates(cell) * kh * st) * (int64_t)sizeof(float);
}

int ofp_rnn_layer(int32_t cell, int64_t n_seq, int32_t T, int32_t in, int32_t H, int32_t reverse, const float* d_x,
                  int64_t x_seq, int64_t x_t, int64_t x_f, const float* d_gx, int64_t gx_seq, int64_t gx_t,
                  const float* d_w_ih, const float* d_b_ih, const float* d_w_hh, const float* d_b_hh, float* d_y,
                  int64_t y_seq, int64_t y_t, int32_t y_off, void* stream) {
    OFP_REQUIRE(cell >= OFP_CELL_RNN_TANH && cell <= OFP_CELL_LSTM, "ofp_rnn_layer: unknown cell %d", cell);
    OFP_REQUIRE(n_seq >= 0 && n_seq < (1ll << 35), "ofp_rnn_layer: n_seq %lld", (long long)n_seq);
    OFP_REQUIRE(T >= 1, "ofp_rnn_layer: T = %d (need >= 1)", T);
    OFP_REQUIRE(H >= 1 && H <= RNN_MAX_H, "ofp_rnn_layer: hidden size %d (1..%d supported)", H, RNN_MAX_H);
    OFP_REQUIRE(in >= 1, "ofp_rnn_layer: input width %d", in);
    OFP_REQUIRE(d_w_hh && d_y, "ofp_rnn_layer: NULL w_hh or y");
    OFP_REQUIRE(y_off >= 0, "ofp_rnn_layer: y_off %d", y_off);
    if (!d_gx) {
        OFP_REQUIRE(d_x && d_w_ih, "ofp_rnn_layer: NULL x or w_ih (and no precomputed projection)");
        OFP_REQUIRE(in <= RNN_MAX_INLINE, "ofp_rnn_layer: input width %d > %d: precompute x W_ih^T + b_ih with "
                    "ofp_dense and pass it as gx", in, RNN_MAX_INLINE);
    }
    if (n_seq == 0) return OFP_OK;
    RnnArgs a;
    a.n_seq = n_seq;
    a.T = T;
    a.in = in;
    a.H = H;
    a.reverse = reverse ? 1 : 0;
    a.x = d_x;
    a.x_seq = x_seq;
    a.x_t = x_t;
    a.x_f = x_f;
    a.gx = d_gx;
    a.gx_seq = gx_seq;
    a.gx_t = gx_t;
    a.w_ih = d_w_ih;
    a.b_ih = d_b_ih;
    a.w_hh = d_w_hh;
    a.b_hh = d_b_hh;
    a.y = d_y;
    a.y_seq = y_seq;
    a.y_t = y_t;
    a.y_off = y_off;
    a.kh = (H + 15) / 16 * 16;
    a.st = a.kh + 4;
    a.w_vec = (H % 4 == 0) && ((uintptr_t)d_w_hh % 16 == 0);
    const int tiles = a.kh / 16;
    const int waves = std::min(tiles, RNN_WAVES);
    const int nt = (tiles + waves - 1) / waves;  // 1, 2, 3 or 4
    const size_t full = (size_t)ofp_rnn_lds_bytes(cell, H);
    const bool wlds = full <= LDS_MAX;  // otherwise W_hh is streamed from L2 every step
    const size_t lds = wlds ? full : (size_t)32 * a.st * sizeof(float);
    const hipStream_t s = (hipStream_t)stream;
    const int ntc = nt == 1 ? 1 : nt == 2 ? 2 : 4;
    switch (cell) {
        case OFP_CELL_RNN_TANH: return launch_rnn_cell<OFP_CELL_RNN_TANH>(a, ntc, wlds, lds, 64 * waves, s);
        case OFP_CELL_RNN_RELU: return launch_rnn_cell<OFP_CELL_RNN_RELU>(a, ntc, wlds, lds, 64 * waves, s);
        case OFP_CELL_GRU: return launch_rnn_cell<OFP_CELL_GRU>(a, ntc, wlds, lds, 64 * waves, s);
        default: return launch_rnn_cell<OFP_CELL_LSTM>(a, ntc, wlds, lds, 64 * waves, s);
    }
}

int ofp_layernorm(const float* d_x, int64_t n, int32_t E, const float* d_gamma, const float* d_beta, float eps,
                  float* d_y, void* stream) {
    OFP_REQUIRE(n >= 0 && E >= 1, "ofp_layernorm: bad sizes");
    if (n == 0) return OFP_OK;
    OFP_REQUIRE(d_x && d_y, "ofp_layernorm: NULL argument");
    hipLaunchKernelGGL(k_layernorm, dim3((unsigned)cdiv(n, LN_WAVES)), dim3(64 * LN_WAVES), 0, (hipStream_t)stream,
                       d_x, n, E, d_gamma, d_beta, eps, d_y);
    OFP_LAUNCH_CHECK("k_layernorm");
    return OFP_OK;
}

int ofp_attention_mean(const float* d_qkv, int64_t n_seq, int32_t T, int32_t E, int32_t n_heads, float* d_out,
                       void* stream) {
    OFP_REQUIRE(T >= 1, "ofp_attention_mean: T = %d (need >= 1)", T);
    OFP_REQUIRE(E >= 1 && n_heads >= 1 && E % n_heads == 0, "ofp_attention_mean: E %d is not divisible by %d heads",
                E, n_heads);
    const int d = E / n_heads;
    OFP_REQUIRE(d <= 128, "ofp_attention_mean: head dim %d > 128", d);
    OFP_REQUIRE(n_seq >= 0 && n_seq * n_heads < (1ll << 31), "ofp_attention_mean: n_seq %lld", (long long)n_seq);
    if (n_seq == 0) return OFP_OK;
    OFP_REQUIRE(d_qkv && d_out, "ofp_attention_mean: NULL argument");
    const hipStream_t s = (hipStream_t)stream;
    if (d <= 16) return launch_attn<4>(d_qkv, n_seq, T, E, n_heads, d, d_out, s);
    if (d <= 32) return launch_attn<8>(d_qkv, n_seq, T, E, n_heads, d, d_out, s);
    if (d <= 64) return launch_attn<16>(d_qkv, n_seq, T, E, n_heads, d, d_out, s);
    return launch_attn<32>(d_qkv, n_seq, T, E, n_heads, d, d_out, s);
}

}  // extern "C"
