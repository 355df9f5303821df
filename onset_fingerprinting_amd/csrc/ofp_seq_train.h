// The sequence part of model.CNNRNN and model.RNN as both of their trainers run it (csrc/ofp_cnnrnn_train.hip,
// csrc/ofp_rnn_train.hip): the dense layer forward and its three gradients, the GRU recurrence that keeps its gates and
// back-propagation through time, self-attention with the mean over time forward and backward (LDS capacity as a
// template parameter: 128 steps for the CNNRNN, 512 for the RNN), the mask of one site of the random stream, and their
// launch helpers and limit checks; and the attention head as a part of a trainer's Plan (ofp_train_chain.h): AttnHead
// with plan_attn_head, take_attn_head_blocks, enqueue_attn_head_fwd and enqueue_attn_head_bwd, the capacity an argument.  File-local like
// ofp_cnn_stack.h, which it builds on: each trainer compiles its own copy.
//
// Every dense layer (GRU input projection, in_proj, out_proj) runs k_lin_fwd on a transposed copy of its weight
// (k_transpose, once per forward); its backward is k_lin_fwd again for dx = dy W (W as stored is the transposed operand)
// and k_lin_wgrad_partial / _final for dW and db.  k_gru_fwd runs the recurrence and keeps r, z, n and W_hn h + b_hn of
// every step; k_gru_bwd walks t = T-1 .. 0 and writes the gate gradients on the input side (dgx), on the hidden side
// (dgh) and the sequence of previous states, from which the Linear backward forms dW_hh, dW_ih, both bias gradients and
// dX.  k_attn_fwd keeps the softmax probabilities (before dropout; the mask is recomputed from the stream); k_attn_bwd
// goes back through the mean, PV, the mask, the softmax and the scaling to dQKV.
//
// Sums.  No atomics.  Every dot product and every sum over rows is accumulated in fp64 in ascending index order by one
// thread and rounded to fp32 once; sums over the rows of a batch (dW, db of a dense layer) are cut into slabs of
// kLinSlab rows, one thread per (slab, output, input) sums its slab in row order and k_lin_wgrad_final adds the slabs
// in slab order.  The shapes depend on the dimensions alone, so results are bitwise reproducible.  The gates'
// sigmoid / tanh and the softmax's exp are evaluated in fp64 from those sums and rounded once.
#pragma once
#include "ofp_cnn_stack.h"

#include <algorithm>
#include <cmath>

namespace {

constexpr uint32_t kSiteAttention = 3;  // dropout on the attention's softmax probabilities [n][heads][T][T]
constexpr int kLinSlab = 256;           // rows one thread of a dense layer's weight gradient sums
constexpr int kLinRows = 8;             // rows of a dense layer's forward that share one read of the weight
constexpr int kLinChunk = 128;          // inputs of those rows staged in LDS at a time
constexpr int kLinOut = 8;              // outputs per workgroup of the weight gradient
constexpr int kMaxHidden = 128;         // GRU hidden size = attention width
constexpr int kMaxHeads = 8;
constexpr int kAttnCapShort = 128;      // time steps the attention kernels hold in LDS: the CNNRNN's instantiation
constexpr int kAttnCapLong = 512;       // ... and the RNN's
constexpr int64_t kMaxRows = (int64_t)1 << 20;

// wt[i][o] = w[o][i]
__global__ __launch_bounds__(kT) void k_transpose(const Ctl* ctl, const float* __restrict__ w, int O, int I,
                                                  float* __restrict__ wt) {
    OFP_CNN_STOPPED(ctl);
    const int64_t total = (int64_t)O * I;
    for (int64_t e = (int64_t)blockIdx.x * kT + threadIdx.x; e < total; e += (int64_t)gridDim.x * kT) {
        const int i = (int)(e / O), o = (int)(e - (int64_t)i * O);
        wt[e] = w[(int64_t)o * I + i];
    }
}

// y[r][o] = b[o] + sum_i x[r][i] wt[i][o] (b may be NULL): workgroup (tile of kLinRows rows, 256 outputs), thread per
// output; the rows' inputs go through LDS kLinChunk at a time, the sum runs over i in ascending order in fp64
__global__ __launch_bounds__(kT) void k_lin_fwd(const Ctl* ctl, const float* __restrict__ x, int64_t R, int I, int O,
                                                const float* __restrict__ wt, const float* __restrict__ b,
                                                float* __restrict__ y) {
    OFP_CNN_STOPPED(ctl);
    __shared__ float xs[kLinRows][kLinChunk];
    const int64_t r0 = (int64_t)blockIdx.x * kLinRows;
    const int o = blockIdx.y * kT + threadIdx.x;
    const int rows = (int)(R - r0 < kLinRows ? R - r0 : kLinRows);
    double acc[kLinRows];
#pragma unroll
    for (int u = 0; u < kLinRows; ++u) acc[u] = 0.0;
    for (int i0 = 0; i0 < I; i0 += kLinChunk) {
        const int len = I - i0 < kLinChunk ? I - i0 : kLinChunk;
        __syncthreads();  // the previous chunk has been read
        for (int e = threadIdx.x; e < kLinRows * kLinChunk; e += kT) {
            const int u = e / kLinChunk, ii = e - u * kLinChunk;
            xs[u][ii] = (u < rows && ii < len) ? x[(r0 + u) * I + i0 + ii] : 0.0f;
        }
        __syncthreads();
        if (o < O)
#pragma unroll 4
            for (int ii = 0; ii < len; ++ii) {
                const double wv = (double)wt[(int64_t)(i0 + ii) * O + o];
#pragma unroll
                for (int u = 0; u < kLinRows; ++u) acc[u] = fma((double)xs[u][ii], wv, acc[u]);
            }
    }
    if (o < O) {
        const double bv = b ? (double)b[o] : 0.0;
#pragma unroll
        for (int u = 0; u < kLinRows; ++u)
            if (u < rows) y[(r0 + u) * O + o] = (float)(acc[u] + bv);
    }
}

// dW[o][i] = sum_r dy[r][o] x[r][i], db[o] = sum_r dy[r][o] (column i == I, x taken as 1) over the rows of one slab:
// workgroup (slab, kLinOut outputs, 256 of the I + 1 columns), rows in ascending order in fp64
__global__ __launch_bounds__(kT) void k_lin_wgrad_partial(const Ctl* ctl, const float* __restrict__ x,
                                                          const float* __restrict__ dy, int64_t R, int I, int O,
                                                          double* __restrict__ partial) {
    OFP_CNN_STOPPED(ctl);
    const int slab = blockIdx.x, o0 = blockIdx.y * kLinOut, i = blockIdx.z * kT + threadIdx.x;
    if (i > I) return;
    const int64_t ra = (int64_t)slab * kLinSlab, rb = ra + kLinSlab < R ? ra + kLinSlab : R;
    const int no = O - o0 < kLinOut ? O - o0 : kLinOut;
    double acc[kLinOut];
#pragma unroll
    for (int u = 0; u < kLinOut; ++u) acc[u] = 0.0;
#pragma unroll 8  // the rows' loads go out together; each sum keeps its row order
    for (int64_t r = ra; r < rb; ++r) {
        const double xv = i < I ? (double)x[r * I + i] : 1.0;
        const float* dr = dy + r * O + o0;
#pragma unroll
        for (int u = 0; u < kLinOut; ++u)
            if (u < no) acc[u] = fma((double)dr[u], xv, acc[u]);
    }
#pragma unroll
    for (int u = 0; u < kLinOut; ++u)
        if (u < no) partial[((int64_t)slab * O + o0 + u) * (I + 1) + i] = acc[u];
}

// the slabs in slab order; dw or db may be NULL
__global__ __launch_bounds__(kT) void k_lin_wgrad_final(const Ctl* ctl, const double* __restrict__ partial, int nslab,
                                                        int I, int O, float* __restrict__ dw, float* __restrict__ db) {
    OFP_CNN_STOPPED(ctl);
    const int64_t e = (int64_t)blockIdx.x * kT + threadIdx.x, per = (int64_t)O * (I + 1);
    if (e >= per) return;
    const int o = (int)(e / (I + 1)), i = (int)(e - (int64_t)o * (I + 1));
    double s = 0.0;
    for (int j = 0; j < nslab; ++j) s += partial[(int64_t)j * per + e];
    if (i == I) {
        if (db) db[o] = (float)s;
    } else if (dw) {
        dw[(int64_t)o * I + i] = (float)s;
    }
}

__device__ __forceinline__ double sigmoid64(double v) { return 1.0 / (1.0 + exp(-v)); }

// The GRU recurrence of kT / H sequences per workgroup, thread per (sequence, hidden unit j); gate order r, z, n, h_0 =
// 0.  gx [n][T][3H] = x W_ih^T + b_ih, whht [H][3H] = W_hh^T.  Per step a = W_hh h + b_hh (three sums over k in
// ascending order, fp64), r = sigmoid(gx_r + a_r), z = sigmoid(gx_z + a_z), n = tanh(gx_n + r a_n), h = (1 - z) n + z
// h_prev.  out [n][T][H]; gates [n][T][4H] = r, z, n, a_n as the backward needs them.
__global__ __launch_bounds__(kT) void k_gru_fwd(const Ctl* ctl, const float* __restrict__ gx,
                                                const float* __restrict__ whht, const float* __restrict__ bhh,
                                                int64_t n, int T, int H, float* __restrict__ out,
                                                float* __restrict__ gates) {
    OFP_CNN_STOPPED(ctl);
    __shared__ float hs[kT];
    const int per = kT / H, sl = threadIdx.x / H, j = threadIdx.x - sl * H;
    const int64_t seq = (int64_t)blockIdx.x * per + sl;
    const bool active = sl < per && seq < n;
    const int H3 = 3 * H;
    const double br = active ? (double)bhh[j] : 0.0, bz = active ? (double)bhh[H + j] : 0.0,
                 bn = active ? (double)bhh[2 * H + j] : 0.0;
    double h = 0.0;
    hs[threadIdx.x] = 0.0f;
    __syncthreads();
    for (int t = 0; t < T; ++t) {
        float hf = 0.0f;
        if (active) {
            double ar = 0.0, az = 0.0, an = 0.0;
            const float* hp = hs + sl * H;
#pragma unroll 4
            for (int k = 0; k < H; ++k) {
                const double hk = (double)hp[k];
                const float* wr = whht + (int64_t)k * H3 + j;
                ar = fma((double)wr[0], hk, ar);
                az = fma((double)wr[H], hk, az);
                an = fma((double)wr[2 * H], hk, an);
            }
            const int64_t row = seq * T + t;
            const float* g = gx + row * H3 + j;
            const double hn = an + bn;
            const double r = sigmoid64((double)g[0] + (ar + br));
            const double z = sigmoid64((double)g[H] + (az + bz));
            const double c = tanh((double)g[2 * H] + r * hn);
            h = (1.0 - z) * c + z * h;
            hf = (float)h;
            h = (double)hf;  // the next step starts from the state as stored
            float* gt = gates + row * 4 * H + j;
            gt[0] = (float)r, gt[H] = (float)z, gt[2 * H] = (float)c, gt[3 * H] = (float)hn;
            out[row * H + j] = hf;
        }
        __syncthreads();  // every thread has read the previous state
        hs[threadIdx.x] = hf;
        __syncthreads();
    }
}

// Back-propagation through time, the mapping of k_gru_fwd.  At step t with dh = dout[t] + (what step t + 1 handed
// back): dn = dh (1 - z), dz = dh (h_prev - n), dc = dn (1 - n^2), dr = dc a_n; gate gradients at the pre-activations
// dgx = (dr r (1 - r), dz z (1 - z), dc) on the input side and dgh = (the same two, dc r) on the hidden side; handed back:
// dh z + W_hh^T dgh (a sum over the 3H gate rows in ascending order, fp64).  hprev [n][T][H] is the state each step
// started from (0 at t = 0), the left operand of dW_hh.
__global__ __launch_bounds__(kT) void k_gru_bwd(const Ctl* ctl, const float* __restrict__ whh,
                                                const float* __restrict__ out, const float* __restrict__ gates,
                                                const float* __restrict__ dout, int64_t n, int T, int H,
                                                float* __restrict__ dgx, float* __restrict__ dgh,
                                                float* __restrict__ hprev) {
    OFP_CNN_STOPPED(ctl);
    __shared__ float dg[3][kT];
    const int per = kT / H, sl = threadIdx.x / H, j = threadIdx.x - sl * H;
    const int64_t seq = (int64_t)blockIdx.x * per + sl;
    const bool active = sl < per && seq < n;
    const int H3 = 3 * H;
    double back = 0.0;
    for (int t = T - 1; t >= 0; --t) {
        float g0 = 0.0f, g1 = 0.0f, g2 = 0.0f;
        double dh = 0.0, z = 0.0;
        const int64_t row = seq * T + t;
        if (active) {
            const float* gt = gates + row * 4 * H + j;
            const double r = (double)gt[0], c = (double)gt[2 * H], hn = (double)gt[3 * H];
            z = (double)gt[H];
            const float hpf = t > 0 ? out[(row - 1) * H + j] : 0.0f;
            dh = (double)dout[row * H + j] + back;
            const double dc = dh * (1.0 - z) * (1.0 - c * c);
            const double dzp = dh * ((double)hpf - c) * z * (1.0 - z);
            const double drp = dc * hn * r * (1.0 - r);
            g0 = (float)drp, g1 = (float)dzp, g2 = (float)(dc * r);
            float* dx = dgx + row * H3 + j;
            dx[0] = g0, dx[H] = g1, dx[2 * H] = (float)dc;
            float* dq = dgh + row * H3 + j;
            dq[0] = g0, dq[H] = g1, dq[2 * H] = g2;
            hprev[row * H + j] = hpf;
        }
        __syncthreads();  // the previous step's gate gradients have been read
        dg[0][threadIdx.x] = g0, dg[1][threadIdx.x] = g1, dg[2][threadIdx.x] = g2;
        __syncthreads();
        if (active) {
            double acc = 0.0;
            for (int g = 0; g < 3; ++g) {
                const float* dv = dg[g] + sl * H;
                const float* wr = whh + (int64_t)g * H * H + j;
#pragma unroll 4
                for (int k = 0; k < H; ++k) acc = fma((double)wr[(int64_t)k * H], (double)dv[k], acc);
            }
            back = dh * z + acc;
        }
    }
}

// what the dropout of `site` does to element idx: 0 (dropped) or the scale s; 1 without dropout
__device__ __forceinline__ float keep_scale(const Ctl* ctl, const Stream& r, uint32_t thr, float s, bool drop,
                                            uint32_t site, uint32_t idx) {
    if (!drop) return 1.0f;
    return item_word(stream_words(ctl, r, idx >> 2, site), (int)(idx & 3u)) < thr ? 0.0f : s;
}

struct Attn {
    int64_t n;
    int T, E, heads;
    bool drop;
    Stream st;
    uint32_t thr;
    float s;
};

// Self-attention of one (sequence, head) per workgroup and its mean over time, for T <= kCap.  qkv [n][T][3E] is the
// in-projection; with d = E / heads and q, k, v the head's columns: p[i][.] = softmax_j(q_i . k_j / sqrt(d)) (thread
// per row i: the row's largest logit first, then exp(logit - max) and their sum, fp64), kept in probs
// [n][heads][T][T]; p' = p * (dropout of site 3 at element ((s heads + h) T + i) T + j); ctx[s][h d + c] = (1 / T) sum_j
// (sum_i p'[i][j]) v[j][c], both sums in ascending order in fp64.
template <int kCap>
__global__ __launch_bounds__(kT) void k_attn_fwd(const Ctl* ctl, const Attn a, const float* __restrict__ qkv,
                                                 float* __restrict__ probs, float* __restrict__ ctx) {
    OFP_CNN_STOPPED(ctl);
    __shared__ double cs[kCap];
    const int T = a.T, E = a.E, d = E / a.heads;
    const int64_t s = blockIdx.x / a.heads;
    const int hd = blockIdx.x - (int)s * a.heads;
    const float* q = qkv + s * T * 3 * E + hd * d;
    const float* k = q + E;
    const float* v = q + 2 * E;
    float* P = probs + (int64_t)blockIdx.x * T * T;
    const double inv = 1.0 / sqrt((double)d);
    for (int i = threadIdx.x; i < T; i += kT) {
        const float* qi = q + (int64_t)i * 3 * E;
        double top = -INFINITY;
        for (int j = 0; j < T; ++j) {
            const float* kj = k + (int64_t)j * 3 * E;
            double dot = 0.0;
            for (int c = 0; c < d; ++c) dot = fma((double)qi[c], (double)kj[c], dot);
            top = fmax(top, dot * inv);
        }
        double sum = 0.0;
        for (int j = 0; j < T; ++j) {
            const float* kj = k + (int64_t)j * 3 * E;
            double dot = 0.0;
            for (int c = 0; c < d; ++c) dot = fma((double)qi[c], (double)kj[c], dot);
            const float e = (float)exp(dot * inv - top);
            P[(int64_t)i * T + j] = e;
            sum += (double)e;
        }
        for (int j = 0; j < T; ++j) P[(int64_t)i * T + j] = (float)((double)P[(int64_t)i * T + j] / sum);
    }
    __syncthreads();
    const uint32_t base = (uint32_t)((int64_t)blockIdx.x * T * T);
    for (int j = threadIdx.x; j < T; j += kT) {
        double col = 0.0;
        for (int i = 0; i < T; ++i)
            col += (double)(P[(int64_t)i * T + j] * keep_scale(ctl, a.st, a.thr, a.s, a.drop, kSiteAttention,
                                                               base + (uint32_t)(i * T + j)));
        cs[j] = col;
    }
    __syncthreads();
    for (int c = threadIdx.x; c < d; c += kT) {
        double acc = 0.0;
        for (int j = 0; j < T; ++j) acc = fma(cs[j], (double)v[(int64_t)j * 3 * E + c], acc);
        ctx[s * E + hd * d + c] = (float)(acc / (double)T);
    }
}

// Backward of k_attn_fwd: dctx [n][E] -> dqkv [n][T][3E].  With g[j] = (1 / T) sum_c dctx[c] v[j][c] the gradient at
// p'[i][j] is g[j] for every i; dv[j][c] = (1 / T) (sum_i p'[i][j]) dctx[c]; through the mask and the softmax ds[i][j] =
// p[i][j] (m[i][j] g[j] - sum_j' m[i][j'] g[j'] p[i][j']), kept in `ds` [n][heads][T][T]; dq[i][c] = sum_j ds[i][j]
// k[j][c] / sqrt(d), dk[j][c] = sum_i ds[i][j] q[i][c] / sqrt(d).  Sums in ascending order in fp64.
template <int kCap>
__global__ __launch_bounds__(kT) void k_attn_bwd(const Ctl* ctl, const Attn a, const float* __restrict__ qkv,
                                                 const float* __restrict__ probs, const float* __restrict__ dctx,
                                                 float* __restrict__ ds, float* __restrict__ dqkv) {
    OFP_CNN_STOPPED(ctl);
    __shared__ double cs[kCap];
    __shared__ double gs[kCap];
    const int T = a.T, E = a.E, d = E / a.heads;
    const int64_t s = blockIdx.x / a.heads;
    const int hd = blockIdx.x - (int)s * a.heads;
    const float* q = qkv + s * T * 3 * E + hd * d;
    const float* k = q + E;
    const float* v = q + 2 * E;
    float* dq = dqkv + s * T * 3 * E + hd * d;
    float* dk = dq + E;
    float* dv = dq + 2 * E;
    const float* P = probs + (int64_t)blockIdx.x * T * T;
    float* D = ds + (int64_t)blockIdx.x * T * T;
    const float* dc = dctx + s * E + hd * d;
    const double inv = 1.0 / sqrt((double)d);
    const uint32_t base = (uint32_t)((int64_t)blockIdx.x * T * T);
    for (int j = threadIdx.x; j < T; j += kT) {
        double col = 0.0, g = 0.0;
        for (int i = 0; i < T; ++i)
            col += (double)(P[(int64_t)i * T + j] * keep_scale(ctl, a.st, a.thr, a.s, a.drop, kSiteAttention,
                                                               base + (uint32_t)(i * T + j)));
        for (int c = 0; c < d; ++c) g = fma((double)dc[c], (double)v[(int64_t)j * 3 * E + c], g);
        cs[j] = col, gs[j] = g / (double)T;
    }
    __syncthreads();
    for (int e = threadIdx.x; e < T * d; e += kT) {
        const int j = e / d, c = e - j * d;
        dv[(int64_t)j * 3 * E + c] = (float)(cs[j] * (double)dc[c] / (double)T);
    }
    if constexpr (kCap > kAttnCapShort) {
        // long sequences, as in k_attn_fwd: the row's thread forms the row's sum alone, in the same order; ds is then
        // written element by element across the threads, coalesced, from the same expression
        __shared__ double rowdot[kCap];
        for (int i = threadIdx.x; i < T; i += kT) {
            double dot = 0.0;
            for (int j = 0; j < T; ++j) {
                const double m = (double)keep_scale(ctl, a.st, a.thr, a.s, a.drop, kSiteAttention,
                                                    base + (uint32_t)(i * T + j));
                dot = fma(m * gs[j], (double)P[(int64_t)i * T + j], dot);
            }
            rowdot[i] = dot;
        }
        __syncthreads();
        for (int e = threadIdx.x; e < T * T; e += kT) {
            const int i = e / T, j = e - i * T;
            const double m = (double)keep_scale(ctl, a.st, a.thr, a.s, a.drop, kSiteAttention, base + (uint32_t)e);
            D[e] = (float)((double)P[e] * (m * gs[j] - rowdot[i]));
        }
    } else {
        for (int i = threadIdx.x; i < T; i += kT) {
            double dot = 0.0;
            for (int j = 0; j < T; ++j) {
                const double m = (double)keep_scale(ctl, a.st, a.thr, a.s, a.drop, kSiteAttention,
                                                    base + (uint32_t)(i * T + j));
                dot = fma(m * gs[j], (double)P[(int64_t)i * T + j], dot);
            }
            for (int j = 0; j < T; ++j) {
                const double m = (double)keep_scale(ctl, a.st, a.thr, a.s, a.drop, kSiteAttention,
                                                    base + (uint32_t)(i * T + j));
                D[(int64_t)i * T + j] = (float)((double)P[(int64_t)i * T + j] * (m * gs[j] - dot));
            }
        }
    }
    __syncthreads();
    for (int e = threadIdx.x; e < T * d; e += kT) {
        const int i = e / d, c = e - i * d;
        double aq = 0.0, ak = 0.0;
        for (int j = 0; j < T; ++j) {
            aq = fma((double)D[(int64_t)i * T + j], (double)k[(int64_t)j * 3 * E + c], aq);
            ak = fma((double)D[(int64_t)j * T + i], (double)q[(int64_t)j * 3 * E + c], ak);
        }
        dq[(int64_t)i * 3 * E + c] = (float)(aq * inv);
        dk[(int64_t)i * 3 * E + c] = (float)(ak * inv);
    }
}

// the mask of one site over `total` consecutive elements: 0 and s
__global__ __launch_bounds__(kT) void k_site_mask(const Stream r, uint32_t thr, float s, uint32_t site, int64_t total,
                                                  float* __restrict__ mask) {
    for (int64_t i = (int64_t)blockIdx.x * kT + threadIdx.x; i < total; i += (int64_t)gridDim.x * kT)
        mask[i] = keep_scale(nullptr, r, thr, s, true, site, (uint32_t)i);
}

// ---- host side ------------------------------------------------------------------------------------------------------

int lin_slabs(int64_t R) { return (int)ofp::cdiv(R, kLinSlab); }
int64_t lin_part_bytes(int64_t R, int I, int O) { return (int64_t)lin_slabs(R) * O * (I + 1) * 8; }

int enqueue_transpose(const Ctl* ctl, const float* w, int O, int I, float* wt, hipStream_t st) {
    hipLaunchKernelGGL(k_transpose, dim3(grid_for((int64_t)O * I)), dim3(kT), 0, st, ctl, w, O, I, wt);
    OFP_LAUNCH_CHECK("k_transpose");
    return OFP_OK;
}

// y [R][O] = x [R][I] wt [I][O] + b
int enqueue_lin_fwd(const Ctl* ctl, const float* x, int64_t R, int I, int O, const float* wt, const float* b, float* y,
                    hipStream_t st) {
    hipLaunchKernelGGL(k_lin_fwd, dim3((unsigned)ofp::cdiv(R, kLinRows), (unsigned)ofp::cdiv(O, kT)), dim3(kT), 0, st,
                       ctl, x, R, I, O, wt, b, y);
    OFP_LAUNCH_CHECK("k_lin_fwd");
    return OFP_OK;
}

// the three gradients of y = x w^T + b: dx [R][I] (unless NULL), dw [O][I], db [O]; `part` takes lin_part_bytes
int enqueue_lin_bwd(const Ctl* ctl, const float* x, int64_t R, int I, int O, const float* w, const float* dy,
                    double* part, float* dx, float* dw, float* db, hipStream_t st) {
    const int nslab = lin_slabs(R);
    hipLaunchKernelGGL(k_lin_wgrad_partial,
                       dim3(nslab, (unsigned)ofp::cdiv(O, kLinOut), (unsigned)ofp::cdiv(I + 1, kT)), dim3(kT), 0, st,
                       ctl, x, dy, R, I, O, part);
    OFP_LAUNCH_CHECK("k_lin_wgrad_partial");
    hipLaunchKernelGGL(k_lin_wgrad_final, dim3((unsigned)ofp::cdiv((int64_t)O * (I + 1), kT)), dim3(kT), 0, st, ctl,
                       part, nslab, I, O, dw, db);
    OFP_LAUNCH_CHECK("k_lin_wgrad_final");
    if (dx) return enqueue_lin_fwd(ctl, dy, R, O, I, w, nullptr, dx, st);
    return OFP_OK;
}

unsigned gru_grid(int64_t n, int H) { return (unsigned)ofp::cdiv(n, kT / H); }

int enqueue_gru_fwd(const Ctl* ctl, const float* gx, const float* whht, const float* bhh, int64_t n, int T, int H,
                    float* out, float* gates, hipStream_t st) {
    hipLaunchKernelGGL(k_gru_fwd, dim3(gru_grid(n, H)), dim3(kT), 0, st, ctl, gx, whht, bhh, n, T, H, out, gates);
    OFP_LAUNCH_CHECK("k_gru_fwd");
    return OFP_OK;
}

int enqueue_gru_bwd(const Ctl* ctl, const float* whh, const float* out, const float* gates, const float* dout,
                    int64_t n, int T, int H, float* dgx, float* dgh, float* hprev, hipStream_t st) {
    hipLaunchKernelGGL(k_gru_bwd, dim3(gru_grid(n, H)), dim3(kT), 0, st, ctl, whh, out, gates, dout, n, T, H, dgx, dgh,
                       hprev);
    OFP_LAUNCH_CHECK("k_gru_bwd");
    return OFP_OK;
}

Attn attn_of(int64_t n, int T, int E, int heads, const Random& rnd, bool train) {
    return Attn{n, T, E, heads, train && rnd.drop, rnd.st, rnd.T, rnd.s};
}

// `cap` is the instantiation: kAttnCapShort or kAttnCapLong, at least a.T (the callers' limit checks see to it)
int enqueue_attn_fwd(const Ctl* ctl, const Attn& a, int cap, const float* qkv, float* probs, float* ctx,
                     hipStream_t st) {
    if (cap == kAttnCapShort)
        hipLaunchKernelGGL((k_attn_fwd<kAttnCapShort>), dim3((unsigned)(a.n * a.heads)), dim3(kT), 0, st, ctl, a, qkv,
                           probs, ctx);
    else
        hipLaunchKernelGGL((k_attn_fwd<kAttnCapLong>), dim3((unsigned)(a.n * a.heads)), dim3(kT), 0, st, ctl, a, qkv,
                           probs, ctx);
    OFP_LAUNCH_CHECK("k_attn_fwd");
    return OFP_OK;
}

int enqueue_attn_bwd(const Ctl* ctl, const Attn& a, int cap, const float* qkv, const float* probs, const float* dctx,
                     float* ds, float* dqkv, hipStream_t st) {
    if (cap == kAttnCapShort)
        hipLaunchKernelGGL((k_attn_bwd<kAttnCapShort>), dim3((unsigned)(a.n * a.heads)), dim3(kT), 0, st, ctl, a, qkv,
                           probs, dctx, ds, dqkv);
    else
        hipLaunchKernelGGL((k_attn_bwd<kAttnCapLong>), dim3((unsigned)(a.n * a.heads)), dim3(kT), 0, st, ctl, a, qkv,
                           probs, dctx, ds, dqkv);
    OFP_LAUNCH_CHECK("k_attn_bwd");
    return OFP_OK;
}

int check_gru(const char* who, int64_t n, int T, int F, int H, int max_steps, int max_feat) {
    OFP_REQUIRE(n >= 1 && n <= kMaxBatch, "%s: %lld sequences (limit: 1..%d)", who, (long long)n, kMaxBatch);
    OFP_REQUIRE(T >= 1 && T <= max_steps, "%s: %d time steps (limit: 1..%d)", who, T, max_steps);
    OFP_REQUIRE(F >= 1 && F <= max_feat, "%s: %d input features (limit: 1..%d)", who, F, max_feat);
    OFP_REQUIRE(H >= 1 && H <= kMaxHidden, "%s: hidden size %d (limit: 1..%d)", who, H, kMaxHidden);
    return OFP_OK;
}

int check_attn(const char* who, int64_t n, int T, int E, int heads, int max_steps) {
    OFP_REQUIRE(n >= 1 && n <= kMaxBatch, "%s: %lld sequences (limit: 1..%d)", who, (long long)n, kMaxBatch);
    OFP_REQUIRE(T >= 1 && T <= max_steps, "%s: %d time steps (limit: 1..%d)", who, T, max_steps);
    OFP_REQUIRE(heads >= 1 && heads <= kMaxHeads && E >= heads && E <= kMaxHidden && E % heads == 0,
                "%s: width %d with %d heads (limits: width 1..%d, heads 1..%d dividing the width)", who, E, heads,
                kMaxHidden, kMaxHeads);
    return OFP_OK;
}

// ---- the attention head as a part of a trainer's Plan ----------------------------------------------------------------
// in_proj -> self-attention with the mean over time -> out_proj -> Linear with the loss, on sequences [n][T][H]

struct AttnHead {
    int T, H, heads, O, loss;
    int inw_off, inb_off, ow_off, ob_off, fcw_off, fcb_off;
    // work space, byte offsets: both transposed weights, what the forward keeps, the gradients on the way back
    int64_t o_inwt, o_owt, o_qkv, o_P, o_ctx, o_ao, o_out, o_dy, o_lpart, o_dao, o_dctx, o_ds, o_dqkv;
};

// Checks the head's dimensions against `cap` and plans it for a training batch of n: its parameters go behind the
// caller's np, max_part_bytes is raised to what its partial sums need, and the two transposed weights take their blocks
// from `ws`.  The other eleven blocks are taken by take_attn_head_blocks, which the trainer calls after the blocks of what
// feeds the head, so that the large buffers keep the order they had when each trainer planned them itself
// (profiles/README.md, r10, has the timings behind this).
int plan_attn_head(const char* who, int64_t n, int T, int H, int heads, int O, int loss, int cap,
                   WsPlan& ws, int& np, int64_t& max_part_bytes, AttnHead& a) {
    if (int rc = check_attn(who, n, T, H, heads, cap)) return rc;
    a = AttnHead{};
    a.T = T, a.H = H, a.heads = heads, a.O = O, a.loss = loss;
    a.inw_off = np, np += 3 * H * H;
    a.inb_off = np, np += 3 * H;
    a.ow_off = np, np += H * H;
    a.ob_off = np, np += H;
    a.fcw_off = np, np += O * H;
    a.fcb_off = np, np += O;
    max_part_bytes = std::max<int64_t>(max_part_bytes, (int64_t)fc_chunks(n) * O * H * 8);
    max_part_bytes = std::max<int64_t>(max_part_bytes, lin_part_bytes(n * T, H, 3 * H));
    max_part_bytes = std::max<int64_t>(max_part_bytes, lin_part_bytes(n, H, H));
    a.o_inwt = ws.take((int64_t)3 * H * H * 4);
    a.o_owt = ws.take((int64_t)H * H * 4);
    return OFP_OK;
}

// what the head's forward keeps and its backward writes, for nmax = max(n, n_val) and n samples
void take_attn_head_blocks(WsPlan& ws, int64_t n, int64_t nmax, AttnHead& a) {
    const int T = a.T, H = a.H, heads = a.heads, O = a.O;
    a.o_qkv = ws.take(nmax * T * 3 * H * 4);
    a.o_P = ws.take(nmax * heads * T * T * 4);
    a.o_ctx = ws.take(nmax * H * 4);
    a.o_ao = ws.take(nmax * H * 4);
    a.o_out = ws.take(nmax * O * 4);
    a.o_dy = ws.take(nmax * O * 4);
    a.o_lpart = ws.take(nmax * 8);
    a.o_dao = ws.take(n * H * 4);
    a.o_dctx = ws.take(n * H * 4);
    a.o_ds = ws.take(n * heads * T * T * 4);
    a.o_dqkv = ws.take(n * T * 3 * H * 4);
}

// the head on `in` [n T][H] with targets y, the batch's mean loss into `curve` (enqueue_fc_forward); train: dropout on
// the probabilities, d loss / d out kept and the Linear's bias gradient
template <class Plan>
int enqueue_attn_head_fwd(const Run<Plan>& r, const AttnHead& a, int cap, const float* in, int64_t n, const float* y,
                          bool train, float* curve, int patience) {
    const int T = a.T, H = a.H;
    float* inwt = r.template at<float>(a.o_inwt);
    float* owt = r.template at<float>(a.o_owt);
    float* qkv = r.template at<float>(a.o_qkv);
    float* ctx = r.template at<float>(a.o_ctx);
    float* ao = r.template at<float>(a.o_ao);
    if (int rc = enqueue_transpose(r.ctl, r.P + a.inw_off, 3 * H, H, inwt, r.st)) return rc;
    if (int rc = enqueue_transpose(r.ctl, r.P + a.ow_off, H, H, owt, r.st)) return rc;
    if (int rc = enqueue_lin_fwd(r.ctl, in, n * T, H, 3 * H, inwt, r.P + a.inb_off, qkv, r.st)) return rc;
    if (int rc = enqueue_attn_fwd(r.ctl, attn_of(n, T, H, a.heads, r.rnd, train), cap, qkv,
                                  r.template at<float>(a.o_P), ctx, r.st))
        return rc;
    if (int rc = enqueue_lin_fwd(r.ctl, ctx, n, H, H, owt, r.P + a.ob_off, ao, r.st)) return rc;
    const Fc f{ao, n, H, a.O, r.P + a.fcw_off, r.P + a.fcb_off, y};
    return enqueue_fc_forward(r.ctl, f, a.loss, r.template at<float>(a.o_out),
                              train ? r.template at<float>(a.o_dy) : nullptr, r.template at<double>(a.o_lpart), curve,
                              patience, r.G + a.fcb_off, r.st);
}

// backward of the head from the d loss / d out its forward kept: the head's gradients go to r.G, the gradient at `in`
// to d_in [n T][H]; `part` takes the partial sums
template <class Plan>
int enqueue_attn_head_bwd(const Run<Plan>& r, const AttnHead& a, int cap, const float* in, int64_t n, double* part,
                          float* d_in) {
    const int T = a.T, H = a.H;
    float* dao = r.template at<float>(a.o_dao);
    float* dctx = r.template at<float>(a.o_dctx);
    float* dqkv = r.template at<float>(a.o_dqkv);
    const Fc f{r.template at<float>(a.o_ao), n, H, a.O, r.P + a.fcw_off, r.P + a.fcb_off, nullptr};
    if (int rc = enqueue_fc_backward(r.ctl, f, r.template at<float>(a.o_dy), part, r.G + a.fcw_off, dao, r.st))
        return rc;
    if (int rc = enqueue_lin_bwd(r.ctl, r.template at<float>(a.o_ctx), n, H, H, r.P + a.ow_off, dao, part, dctx,
                                 r.G + a.ow_off, r.G + a.ob_off, r.st))
        return rc;
    if (int rc = enqueue_attn_bwd(r.ctl, attn_of(n, T, H, a.heads, r.rnd, true), cap, r.template at<float>(a.o_qkv),
                                  r.template at<float>(a.o_P), dctx, r.template at<float>(a.o_ds), dqkv, r.st))
        return rc;
    return enqueue_lin_bwd(r.ctl, in, n * T, H, 3 * H, r.P + a.inw_off, dqkv, part, d_in, r.G + a.inw_off,
                           r.G + a.inb_off, r.st);
}

// the random options of a stand-alone attention call: dropout alone, no window source
int attn_random(const char* who, const ofp_train_random* random, Random& rnd) {
    OFP_REQUIRE(random == nullptr || random->n_extractions == 0, "%s: takes no window source", who);
    return make_random(who, random, 0, 0, 0, 0, false, rnd);
}

// The stand-alone attention pair of both trainers (ofp_attention_mean_train_*, ofp_rnn_attention_train_*), which
// differ in `cap` alone.  Forward work space: in_proj_weight^T.  Backward: ds, dqkv, the in_proj gradients' slabs.
int64_t attn_fwd_alone_bytes(const char* who, int64_t n, int T, int E, int heads, int cap) {
    if (check_attn(who, n, T, E, heads, cap)) return -1;
    return (int64_t)3 * E * E * 4;
}

int attn_fwd_alone(const char* who, int cap, const float* d_h, int64_t n, int T, int E, int heads, const float* d_in_w,
                   const float* d_in_b, const ofp_train_random* random, float* d_qkv, float* d_probs, float* d_ctx,
                   void* d_ws, int64_t ws_bytes, void* stream) {
    Random rnd;
    if (int rc = check_attn(who, n, T, E, heads, cap)) return rc;
    if (int rc = attn_random(who, random, rnd)) return rc;
    OFP_REQUIRE(d_h && d_in_w && d_in_b && d_qkv && d_probs && d_ctx, "%s: NULL argument", who);
    if (int rc = check_ws(who, d_ws, ws_bytes, (int64_t)3 * E * E * 4)) return rc;
    hipStream_t st = (hipStream_t)stream;
    float* inwt = (float*)d_ws;
    if (int rc = enqueue_transpose(nullptr, d_in_w, 3 * E, E, inwt, st)) return rc;
    if (int rc = enqueue_lin_fwd(nullptr, d_h, n * T, E, 3 * E, inwt, d_in_b, d_qkv, st)) return rc;
    return enqueue_attn_fwd(nullptr, attn_of(n, T, E, heads, rnd, true), cap, d_qkv, d_probs, d_ctx, st);
}

int64_t attn_bwd_alone_bytes(const char* who, int64_t n, int T, int E, int heads, int cap) {
    if (check_attn(who, n, T, E, heads, cap)) return -1;
    return ofp::align_up(n * heads * T * T * 4, 256) + ofp::align_up(n * T * 3 * E * 4, 256) +
           lin_part_bytes(n * T, E, 3 * E);
}

int attn_bwd_alone(const char* who, int cap, const float* d_h, int64_t n, int T, int E, int heads, const float* d_in_w,
                   const float* d_qkv, const float* d_probs, const float* d_dctx, const ofp_train_random* random,
                   float* d_dh, float* d_dw, float* d_db, void* d_ws, int64_t ws_bytes, void* stream) {
    Random rnd;
    if (int rc = check_attn(who, n, T, E, heads, cap)) return rc;
    if (int rc = attn_random(who, random, rnd)) return rc;
    OFP_REQUIRE(d_h && d_in_w && d_qkv && d_probs && d_dctx && d_dh && d_dw && d_db, "%s: NULL argument", who);
    if (int rc = check_ws(who, d_ws, ws_bytes, attn_bwd_alone_bytes(who, n, T, E, heads, cap))) return rc;
    hipStream_t st = (hipStream_t)stream;
    float* ds = (float*)d_ws;
    float* dqkv = reinterpret_cast<float*>((char*)d_ws + ofp::align_up(n * heads * T * T * 4, 256));
    double* part = reinterpret_cast<double*>((char*)dqkv + ofp::align_up(n * T * 3 * E * 4, 256));
    if (int rc = enqueue_attn_bwd(nullptr, attn_of(n, T, E, heads, rnd, true), cap, d_qkv, d_probs, d_dctx, ds, dqkv,
                                  st))
        return rc;
    return enqueue_lin_bwd(nullptr, d_h, n * T, E, 3 * E, d_in_w, dqkv, part, d_dh, d_dw, d_db, st);
}

}  // namespace
