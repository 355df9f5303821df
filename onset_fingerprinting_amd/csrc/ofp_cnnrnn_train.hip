// Training model.CNNRNN on the GPU (the reference's model.py:310-440): the conv stack of model.CNN (csrc/ofp_cnn_stack.h),
// the model's dropout on the conv features (site 0 of the random stream), a one-layer GRU whose time axis is the last
// conv layer's channels and whose features are its columns, 2-head self-attention with dropout on the softmax
// probabilities (site 3), the mean over time, out_proj and the Linear head with its loss; backward through all of it,
// one NAdam step, and optionally an eval-mode validation pass with the early-stop rule.  One epoch is a linear chain of
// kernels on one stream, captured once and replayed by run_epochs (csrc/ofp_train_chain.h), as for the other trainers.
//
// Kernels of this file.  Every dense layer (GRU input projection, in_proj, out_proj) runs k_lin_fwd on a transposed
// copy of its weight (k_transpose, once per forward); its backward is k_lin_fwd again for dx = dy W (W as stored is
// the transposed operand) and k_lin_wgrad_partial / _final for dW and db.  k_gru_fwd runs the recurrence and keeps r,
// z, n and W_hn h + b_hn of every step; k_gru_bwd walks t = T-1 .. 0 and writes the gate gradients on the input side
// (dgx), on the hidden side (dgh) and the sequence of previous states, from which the Linear backward forms dW_hh,
// dW_ih, both bias gradients and dX.  k_attn_fwd keeps the softmax probabilities (before dropout; the mask is
// recomputed from the stream); k_attn_bwd goes back through the mean, PV, the mask, the softmax and the scaling to dQKV.
//
// Sums.  No atomics.  Every dot product and every sum over rows is accumulated in fp64 in ascending index order by one
// thread and rounded to fp32 once; sums over the rows of a batch (dW, db of a dense layer) are cut into slabs of
// kLinSlab rows, one thread per (slab, output, input) sums its slab in row order and k_lin_wgrad_final adds the slabs
// in slab order.  The shapes depend on the dimensions alone, so results are bitwise reproducible.  The gates'
// sigmoid / tanh and the softmax's exp are evaluated in fp64 from those sums and rounded once.
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
constexpr int kMaxSteps = 128;          // GRU / attention time steps (the last conv layer's channels)
constexpr int kMaxFeat = 2 * kMaxWidth; // GRU input features (the last conv layer's columns)
constexpr int kMaxHeads = 8;
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

// Self-attention of one (sequence, head) per workgroup and its mean over time.  qkv [n][T][3E] is the in-projection;
// with d = E / heads and q, k, v the head's columns: p[i][.] = softmax_j(q_i . k_j / sqrt(d)) (thread per row i: the
// row's largest logit first, then exp(logit - max) and their sum, fp64), kept in probs [n][heads][T][T];
// p' = p * (dropout of site 3 at element ((s heads + h) T + i) T + j); ctx[s][h d + c] = (1 / T) sum_j (sum_i p'[i][j])
// v[j][c], both sums in ascending order in fp64.
__global__ __launch_bounds__(kT) void k_attn_fwd(const Ctl* ctl, const Attn a, const float* __restrict__ qkv,
                                                 float* __restrict__ probs, float* __restrict__ ctx) {
    OFP_CNN_STOPPED(ctl);
    __shared__ double cs[kMaxSteps];
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
__global__ __launch_bounds__(kT) void k_attn_bwd(const Ctl* ctl, const Attn a, const float* __restrict__ qkv,
                                                 const float* __restrict__ probs, const float* __restrict__ dctx,
                                                 float* __restrict__ ds, float* __restrict__ dqkv) {
    OFP_CNN_STOPPED(ctl);
    __shared__ double cs[kMaxSteps];
    __shared__ double gs[kMaxSteps];
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

int enqueue_attn_fwd(const Ctl* ctl, const Attn& a, const float* qkv, float* probs, float* ctx, hipStream_t st) {
    hipLaunchKernelGGL(k_attn_fwd, dim3((unsigned)(a.n * a.heads)), dim3(kT), 0, st, ctl, a, qkv, probs, ctx);
    OFP_LAUNCH_CHECK("k_attn_fwd");
    return OFP_OK;
}

int enqueue_attn_bwd(const Ctl* ctl, const Attn& a, const float* qkv, const float* probs, const float* dctx, float* ds,
                     float* dqkv, hipStream_t st) {
    hipLaunchKernelGGL(k_attn_bwd, dim3((unsigned)(a.n * a.heads)), dim3(kT), 0, st, ctl, a, qkv, probs, dctx, ds,
                       dqkv);
    OFP_LAUNCH_CHECK("k_attn_bwd");
    return OFP_OK;
}

int check_gru(const char* who, int64_t n, int T, int F, int H) {
    OFP_REQUIRE(n >= 1 && n <= kMaxBatch, "%s: %lld sequences (limit: 1..%d)", who, (long long)n, kMaxBatch);
    OFP_REQUIRE(T >= 1 && T <= kMaxSteps, "%s: %d time steps (limit: 1..%d)", who, T, kMaxSteps);
    OFP_REQUIRE(F >= 1 && F <= kMaxFeat, "%s: %d input features (limit: 1..%d)", who, F, kMaxFeat);
    OFP_REQUIRE(H >= 1 && H <= kMaxHidden, "%s: hidden size %d (limit: 1..%d)", who, H, kMaxHidden);
    return OFP_OK;
}

int check_attn(const char* who, int64_t n, int T, int E, int heads) {
    OFP_REQUIRE(n >= 1 && n <= kMaxBatch, "%s: %lld sequences (limit: 1..%d)", who, (long long)n, kMaxBatch);
    OFP_REQUIRE(T >= 1 && T <= kMaxSteps, "%s: %d time steps (limit: 1..%d)", who, T, kMaxSteps);
    OFP_REQUIRE(heads >= 1 && heads <= kMaxHeads && E >= heads && E <= kMaxHidden && E % heads == 0,
                "%s: width %d with %d heads (limits: width 1..%d, heads 1..%d dividing the width)", who, E, heads,
                kMaxHidden, kMaxHeads);
    return OFP_OK;
}

struct Plan : WsPlan {
    int L, act, bn, pool, loss, O, np, ns;
    int T, F, H, heads;  // GRU steps (last conv channels), features (last conv columns), hidden size = attention width
    double eps;
    float mom;
    Conv conv[kMaxConv];
    int wo[kMaxConv];
    int w_off[kMaxConv], b_off[kMaxConv], g_off[kMaxConv], be_off[kMaxConv], rs_off[kMaxConv];
    int wih_off, whh_off, bih_off, bhh_off, inw_off, inb_off, ow_off, ob_off, fcw_off, fcb_off;
    // work space, byte offsets
    int64_t o_Z[kMaxConv], o_H[kMaxConv], o_HD, o_wiht, o_whht, o_inwt, o_owt, o_gx, o_gates, o_hseq, o_qkv, o_P, o_ctx,
        o_ao, o_out, o_dy, o_lpart, o_dao, o_dctx, o_ds, o_dqkv, o_dhseq, o_dgx, o_dgh, o_hprev, o_gh, o_gz, o_save,
        o_s12, o_part, o_G, o_M, o_V, o_RS, o_ctl, o_X;
};

int make_plan(const ofp_cnnrnn_config* cc, int64_t n, int64_t n_val, Plan& p, const Random& rnd = Random{}) {
    OFP_REQUIRE(cc != nullptr, "cnnrnn training: config is NULL");
    const ofp_cnn_config* c = &cc->cnn;
    OFP_REQUIRE(c->n_conv >= 1 && c->n_conv <= kMaxConv, "cnnrnn training: %d conv layers (limit: 1..%d)", c->n_conv,
                kMaxConv);
    OFP_REQUIRE(n_val >= 0 && n_val <= kMaxBatch, "cnnrnn training: validation batch of %lld (limit: 0..%d)",
                (long long)n_val, kMaxBatch);
    OFP_REQUIRE(c->act >= 0 && c->act <= OFP_ACT_TANH, "cnnrnn training: unknown activation %d", c->act);
    OFP_REQUIRE(c->loss == 0 || c->loss == 1, "cnnrnn training: loss %d (0 = L1, 1 = MSE)", c->loss);
    OFP_REQUIRE(c->n_out >= 1 && c->n_out <= kMaxOut, "cnnrnn training: %d outputs (limit: 1..%d)", c->n_out, kMaxOut);
    if (c->batch_norm)
        OFP_REQUIRE(c->bn_momentum > 0.0f && c->bn_momentum <= 1.0f && c->bn_eps > 0.0,
                    "cnnrnn training: BatchNorm momentum %g, eps %g (a cumulative average, momentum=None, is not built)",
                    (double)c->bn_momentum, c->bn_eps);
    p = Plan{};
    p.L = c->n_conv, p.act = c->act, p.bn = c->batch_norm ? 1 : 0, p.pool = c->pool ? 1 : 0, p.loss = c->loss;
    p.O = c->n_out, p.eps = c->bn_eps, p.mom = c->bn_momentum;
    const int64_t nmax = n > n_val ? n : n_val;
    int width = c->width, np = 0, ns = 0;
    int64_t max_h = 0, max_z = 0, max_part = 2 * 8;  // bytes
    for (int l = 0; l < p.L; ++l) {
        const int cin = c->channels[l], cout = c->channels[l + 1];
        if (int rc = check_conv("cnnrnn training", n, cin, width, cout, c->kernel, c->padding, c->dilation, c->groups))
            return rc;
        Conv& v = p.conv[l];
        v = Conv{cin, cout, width, width + 2 * c->padding - c->dilation * (c->kernel - 1), c->kernel, c->padding,
                 c->dilation, c->groups, 1};
        OFP_REQUIRE(v.wc <= 2 * kMaxWidth, "cnnrnn training: layer %d is %d wide (limit: %d)", l + 1, v.wc,
                    2 * kMaxWidth);
        p.wo[l] = p.pool ? v.wc / 2 : v.wc;
        OFP_REQUIRE(p.wo[l] >= 1, "cnnrnn training: the pool of layer %d leaves no output column", l + 1);
        OFP_REQUIRE(!p.bn || n * v.wc >= 2, "cnnrnn training: BatchNorm needs more than 1 value per channel");
        const int Tw = cin / c->groups * c->kernel + 1;
        p.w_off[l] = np, np += cout * (Tw - 1);
        p.b_off[l] = np, np += cout;
        if (p.bn) {
            p.g_off[l] = np, np += cout;
            p.be_off[l] = np, np += cout;
            p.rs_off[l] = ns, ns += 2 * cout;
        }
        max_part = std::max<int64_t>(max_part, (int64_t)cout * Tw * slabs_of(n * v.wc) * 8);
        max_h = std::max<int64_t>(max_h, nmax * cout * p.wo[l]);
        max_z = std::max<int64_t>(max_z, nmax * cout * v.wc);
        width = p.wo[l];
    }
    p.T = c->channels[p.L], p.F = width, p.H = cc->hidden, p.heads = cc->heads;
    if (int rc = check_gru("cnnrnn training", n, p.T, p.F, p.H)) return rc;
    if (int rc = check_attn("cnnrnn training", n, p.T, p.H, p.heads)) return rc;
    const int H = p.H, F = p.F, T = p.T;
    p.wih_off = np, np += 3 * H * F;
    p.whh_off = np, np += 3 * H * H;
    p.bih_off = np, np += 3 * H;
    p.bhh_off = np, np += 3 * H;
    p.inw_off = np, np += 3 * H * H;
    p.inb_off = np, np += 3 * H;
    p.ow_off = np, np += H * H;
    p.ob_off = np, np += H;
    p.fcw_off = np, np += p.O * H;
    p.fcb_off = np, np += p.O;
    p.np = np, p.ns = ns;
    max_part = std::max<int64_t>(max_part, (int64_t)fc_chunks(n) * p.O * H * 8);
    max_part = std::max<int64_t>(max_part, lin_part_bytes(n * T, F, 3 * H));
    max_part = std::max<int64_t>(max_part, lin_part_bytes(n * T, H, 3 * H));
    max_part = std::max<int64_t>(max_part, lin_part_bytes(n, H, H));
    for (int l = 0; l < p.L; ++l) {
        p.o_Z[l] = p.take(nmax * p.conv[l].cout * p.conv[l].wc * 4);
        p.o_H[l] = p.take(nmax * p.conv[l].cout * p.wo[l] * 4);
    }
    const int64_t rows = nmax * T, sq = nmax * p.heads * T * T;
    p.o_wiht = p.take((int64_t)3 * H * F * 4);
    p.o_whht = p.take((int64_t)3 * H * H * 4);
    p.o_inwt = p.take((int64_t)3 * H * H * 4);
    p.o_owt = p.take((int64_t)H * H * 4);
    p.o_gx = p.take(rows * 3 * H * 4);
    p.o_gates = p.take(rows * 4 * H * 4);
    p.o_hseq = p.take(rows * H * 4);
    p.o_qkv = p.take(rows * 3 * H * 4);
    p.o_P = p.take(sq * 4);
    p.o_ctx = p.take(nmax * H * 4);
    p.o_ao = p.take(nmax * H * 4);
    p.o_out = p.take(nmax * p.O * 4);
    p.o_dy = p.take(nmax * p.O * 4);
    p.o_lpart = p.take(nmax * 8);
    p.o_dao = p.take(n * H * 4);
    p.o_dctx = p.take(n * H * 4);
    p.o_ds = p.take(n * p.heads * T * T * 4);
    p.o_dqkv = p.take(n * T * 3 * H * 4);
    p.o_dhseq = p.take(n * T * H * 4);
    p.o_dgx = p.take(n * T * 3 * H * 4);
    p.o_dgh = p.take(n * T * 3 * H * 4);
    p.o_hprev = p.take(n * T * H * 4);
    p.o_gh = p.take(max_h * 4);
    p.o_gz = p.take(max_z * 4);
    p.o_save = p.take((int64_t)ns * 4);
    p.o_s12 = p.take((int64_t)ns * 4);
    p.o_part = p.take(max_part);
    p.o_G = p.take((int64_t)np * 4);
    p.o_M = p.take((int64_t)np * 4);
    p.o_V = p.take((int64_t)np * 4);
    p.o_RS = p.take((int64_t)ns * 4);
    p.o_ctl = p.take(sizeof(Ctl));
    if (rnd.drop) p.o_HD = p.take(n * T * F * 4);
    if (rnd.windows) p.o_X = p.take(n * c->channels[0] * c->width * 4);
    return OFP_OK;
}

struct Run : WsRun {
    const Plan* p;
    float* P;    // packed parameters
    float* RS;   // packed running statistics
    float* G;    // packed gradients
    Ctl* ctl;    // NULL: a single pass, epoch 0 (rnd.st.epoch for the random stream)
    hipStream_t st;
    Random rnd;  // dropout (conv features, attention probabilities) and the window source; both off by default
};

Post post_of(const Run& r, int l, int mode) {
    const Plan& p = *r.p;
    Post t{};
    t.C = p.conv[l].cout, t.wc = p.conv[l].wc, t.wo = p.wo[l], t.act = p.act, t.pool = p.pool, t.mode = mode;
    t.eps = p.eps;
    if (mode) {
        t.ga = r.P + p.g_off[l], t.be = r.P + p.be_off[l];
        if (mode == 1) {
            t.mean = r.at<float>(p.o_save) + p.rs_off[l], t.rs = t.mean + t.C;
        } else {
            t.mean = r.RS + p.rs_off[l], t.rs = t.mean + t.C;
        }
    }
    return t;
}

// the features the GRU reads: the last conv layer's output, dropped when the run has dropout
const float* features_of(const Run& r) {
    const Plan& p = *r.p;
    return r.at<float>(r.rnd.drop ? p.o_HD : p.o_H[p.L - 1]);
}

// the whole network on a batch, its mean loss into `curve`; train: batch statistics, both dropouts, d loss / d out
// kept and the head's bias gradient; else running statistics, no dropout, L1 and the early-stop rule
int enqueue_forward(const Run& r, const float* x, const float* y, int64_t n, bool train, float* curve, int patience) {
    const Plan& p = *r.p;
    const float* in = x;
    for (int l = 0; l < p.L; ++l) {
        const Conv& c = p.conv[l];
        float* Z = r.at<float>(p.o_Z[l]);
        float* Hl = r.at<float>(p.o_H[l]);
        hipLaunchKernelGGL(k_conv_fwd, dim3(grid_for(n * c.cout * c.wc)), dim3(kT), 0, r.st, r.ctl, c, n, in,
                           r.P + p.w_off[l], r.P + p.b_off[l], Z);
        OFP_LAUNCH_CHECK("k_conv_fwd");
        const Post t = post_of(r, l, p.bn ? (train ? 1 : 2) : 0);
        if (p.bn && train) {
            float* save = r.at<float>(p.o_save) + p.rs_off[l];
            if (int rc = enqueue_bn_stats(r.ctl, Z, n, c.cout, c.wc, p.act, p.eps, p.mom, r.at<double>(p.o_part), save,
                                          save + c.cout, r.RS + p.rs_off[l], r.RS + p.rs_off[l] + c.cout, r.st))
                return rc;
        }
        hipLaunchKernelGGL(k_post, dim3(grid_for(n * c.cout * p.wo[l])), dim3(kT), 0, r.st, r.ctl, t, n, Z, Hl);
        OFP_LAUNCH_CHECK("k_post");
        in = Hl;
    }
    const int T = p.T, F = p.F, H = p.H;
    if (train && r.rnd.drop) {
        float* HD = r.at<float>(p.o_HD);
        if (int rc = enqueue_dropout_fwd(r.ctl, r.rnd, in, HD, n * T * F, r.st)) return rc;
        in = HD;
    }
    float* wiht = r.at<float>(p.o_wiht);
    float* whht = r.at<float>(p.o_whht);
    float* inwt = r.at<float>(p.o_inwt);
    float* owt = r.at<float>(p.o_owt);
    if (int rc = enqueue_transpose(r.ctl, r.P + p.wih_off, 3 * H, F, wiht, r.st)) return rc;
    if (int rc = enqueue_transpose(r.ctl, r.P + p.whh_off, 3 * H, H, whht, r.st)) return rc;
    if (int rc = enqueue_transpose(r.ctl, r.P + p.inw_off, 3 * H, H, inwt, r.st)) return rc;
    if (int rc = enqueue_transpose(r.ctl, r.P + p.ow_off, H, H, owt, r.st)) return rc;
    float* gx = r.at<float>(p.o_gx);
    float* hseq = r.at<float>(p.o_hseq);
    float* qkv = r.at<float>(p.o_qkv);
    float* ctx = r.at<float>(p.o_ctx);
    float* ao = r.at<float>(p.o_ao);
    if (int rc = enqueue_lin_fwd(r.ctl, in, n * T, F, 3 * H, wiht, r.P + p.bih_off, gx, r.st)) return rc;
    if (int rc = enqueue_gru_fwd(r.ctl, gx, whht, r.P + p.bhh_off, n, T, H, hseq, r.at<float>(p.o_gates), r.st))
        return rc;
    if (int rc = enqueue_lin_fwd(r.ctl, hseq, n * T, H, 3 * H, inwt, r.P + p.inb_off, qkv, r.st)) return rc;
    if (int rc = enqueue_attn_fwd(r.ctl, attn_of(n, T, H, p.heads, r.rnd, train), qkv, r.at<float>(p.o_P), ctx, r.st))
        return rc;
    if (int rc = enqueue_lin_fwd(r.ctl, ctx, n, H, H, owt, r.P + p.ob_off, ao, r.st)) return rc;
    const Fc f{ao, n, H, p.O, r.P + p.fcw_off, r.P + p.fcb_off, y};
    return enqueue_fc_forward(r.ctl, f, p.loss, r.at<float>(p.o_out), train ? r.at<float>(p.o_dy) : nullptr,
                              r.at<double>(p.o_lpart), curve, patience, r.G + p.fcb_off, r.st);
}

int enqueue_backward(const Run& r, const float* x, int64_t n) {
    const Plan& p = *r.p;
    const int T = p.T, F = p.F, H = p.H;
    float* GH = r.at<float>(p.o_gh);
    float* GZ = r.at<float>(p.o_gz);
    double* part = r.at<double>(p.o_part);
    float* dao = r.at<float>(p.o_dao);
    float* dctx = r.at<float>(p.o_dctx);
    float* dqkv = r.at<float>(p.o_dqkv);
    float* dhseq = r.at<float>(p.o_dhseq);
    float* dgx = r.at<float>(p.o_dgx);
    float* dgh = r.at<float>(p.o_dgh);
    float* hprev = r.at<float>(p.o_hprev);
    const float* hseq = r.at<float>(p.o_hseq);
    const float* qkv = r.at<float>(p.o_qkv);
    const Fc f{r.at<float>(p.o_ao), n, H, p.O, r.P + p.fcw_off, r.P + p.fcb_off, nullptr};
    if (int rc = enqueue_fc_backward(r.ctl, f, r.at<float>(p.o_dy), part, r.G + p.fcw_off, dao, r.st)) return rc;
    if (int rc = enqueue_lin_bwd(r.ctl, r.at<float>(p.o_ctx), n, H, H, r.P + p.ow_off, dao, part, dctx,
                                 r.G + p.ow_off, r.G + p.ob_off, r.st))
        return rc;
    if (int rc = enqueue_attn_bwd(r.ctl, attn_of(n, T, H, p.heads, r.rnd, true), qkv, r.at<float>(p.o_P), dctx,
                                  r.at<float>(p.o_ds), dqkv, r.st))
        return rc;
    if (int rc = enqueue_lin_bwd(r.ctl, hseq, n * T, H, 3 * H, r.P + p.inw_off, dqkv, part, dhseq, r.G + p.inw_off,
                                 r.G + p.inb_off, r.st))
        return rc;
    if (int rc = enqueue_gru_bwd(r.ctl, r.P + p.whh_off, hseq, r.at<float>(p.o_gates), dhseq, n, T, H, dgx, dgh, hprev,
                                 r.st))
        return rc;
    if (int rc = enqueue_lin_bwd(r.ctl, hprev, n * T, H, 3 * H, r.P + p.whh_off, dgh, part, nullptr, r.G + p.whh_off,
                                 r.G + p.bhh_off, r.st))
        return rc;
    if (int rc = enqueue_lin_bwd(r.ctl, features_of(r), n * T, F, 3 * H, r.P + p.wih_off, dgx, part, GH,
                                 r.G + p.wih_off, r.G + p.bih_off, r.st))
        return rc;
    if (r.rnd.drop)
        if (int rc = enqueue_dropout_bwd(r.ctl, r.rnd, GH, n * T * F, r.st)) return rc;
    for (int l = p.L - 1; l >= 0; --l) {
        const Post t = post_of(r, l, p.bn ? 1 : 0);
        const float* Z = r.at<float>(p.o_Z[l]);
        if (int rc = enqueue_post_bwd(r.ctl, t, n, Z, GH, part, r.at<float>(p.o_s12) + p.rs_off[l],
                                      r.G + p.g_off[l], r.G + p.be_off[l], GZ, r.st))
            return rc;
        const float* in = l == 0 ? x : r.at<float>(p.o_H[l - 1]);
        if (int rc = enqueue_conv_bwd(r.ctl, p.conv[l], n, in, r.P + p.w_off[l], GZ, part, r.G + p.w_off[l],
                                      r.G + p.b_off[l], l == 0 ? nullptr : GH, r.st))
            return rc;
    }
    return OFP_OK;
}

int enqueue_step(const Run& r, const float* rows) {
    const Plan& p = *r.p;
    hipLaunchKernelGGL(k_nadam, dim3(grid_for(p.np)), dim3(kT), 0, r.st, r.ctl, rows, r.P, r.G, r.at<float>(p.o_M),
                       r.at<float>(p.o_V), (int64_t)p.np);
    OFP_LAUNCH_CHECK("k_nadam");
    return OFP_OK;
}

// the random options of a stand-alone attention call: dropout alone, no window source
int attn_random(const char* who, const ofp_train_random* random, Random& rnd) {
    OFP_REQUIRE(random == nullptr || random->n_extractions == 0, "%s: takes no window source", who);
    return make_random(who, random, 0, 0, 0, 0, false, rnd);
}

}  // namespace

extern "C" {

int32_t ofp_linear_backward_slab(void) { return kLinSlab; }

int64_t ofp_cnnrnn_train_stretch_workspace_bytes(const ofp_cnnrnn_config* cfg, int64_t n, int64_t n_val,
                                                 const ofp_train_random* random, int32_t stretch_span) {
    Plan p;
    Random rnd;
    if (cfg == nullptr ||
        make_random("cnnrnn training", random, stretch_span, n, cfg->cnn.channels[0], cfg->cnn.width, true, rnd))
        return -1;
    if (make_plan(cfg, n, n_val, p, rnd)) return -1;
    return p.bytes;
}

int ofp_cnnrnn_train_stretch(const ofp_cnnrnn_config* cfg, int64_t n, const float* d_x, const float* d_y,
                             int64_t n_val, const float* d_x_val, const float* d_y_val, const float* d_rates,
                             int32_t num_epochs, int32_t min_epochs, int32_t patience, float* d_params, float* d_stats,
                             float* d_train_loss, float* d_val_loss, int32_t* h_epochs, void* d_ws, int64_t ws_bytes,
                             void* stream, const ofp_train_random* random, int32_t stretch_span) {
    Plan p;
    Random rnd;
    OFP_REQUIRE(cfg != nullptr, "cnnrnn training: config is NULL");
    if (int rc = make_random("ofp_cnnrnn_train", random, stretch_span, n, cfg->cnn.channels[0], cfg->cnn.width, true,
                             rnd))
        return rc;
    if (int rc = make_plan(cfg, n, n_val, p, rnd)) return rc;
    if (rnd.windows && d_ws) d_x = reinterpret_cast<const float*>((const char*)d_ws + p.o_X);
    const TrainArgs a{d_x, d_y, n, d_x_val, d_y_val, n_val, d_rates, min_epochs, patience, d_train_loss, d_val_loss};
    if (int rc = check_train("ofp_cnnrnn_train", a, num_epochs, d_params, h_epochs)) return rc;
    OFP_REQUIRE(p.ns == 0 || d_stats, "ofp_cnnrnn_train: BatchNorm statistics are NULL");
    if (int rc = check_ws("ofp_cnnrnn_train", d_ws, ws_bytes, p.bytes)) return rc;
    hipStream_t st = (hipStream_t)stream;
    Run r{{(char*)d_ws}, &p, d_params, d_stats, nullptr, nullptr, st, rnd};
    r.G = r.at<float>(p.o_G);
    r.ctl = r.at<Ctl>(p.o_ctl);
    return run_epochs(
        "ofp_cnnrnn_train", "OFP_CNNRNN_GRAPH", st, r.ctl, num_epochs, patience, h_epochs,
        [&] {
            OFP_HIP(hipMemsetAsync(r.at<float>(p.o_M), 0, (size_t)p.np * 4, st));
            OFP_HIP(hipMemsetAsync(r.at<float>(p.o_V), 0, (size_t)p.np * 4, st));
            return OFP_OK;
        },
        [&] { return enqueue_epoch(r, a); });
}

int64_t ofp_cnnrnn_loss_grads_random_workspace_bytes(const ofp_cnnrnn_config* cfg, int64_t n, int64_t n_val,
                                                     const ofp_train_random* random) {
    return ofp_cnnrnn_train_stretch_workspace_bytes(cfg, n, n_val, random, 0);
}

int ofp_cnnrnn_loss_grads_random(const ofp_cnnrnn_config* cfg, int64_t n, const float* d_x, const float* d_y,
                                 const float* d_params, float* d_loss, float* d_grads, void* d_ws, int64_t ws_bytes,
                                 void* stream, const ofp_train_random* random) {
    Plan p;
    Random rnd;
    if (int rc = make_random("ofp_cnnrnn_loss_grads", random, 0, n, 0, 0, false, rnd)) return rc;
    if (int rc = make_plan(cfg, n, 0, p, rnd)) return rc;
    OFP_REQUIRE(d_x && d_y && d_params && d_loss && d_grads, "ofp_cnnrnn_loss_grads: NULL argument");
    if (int rc = check_ws("ofp_cnnrnn_loss_grads", d_ws, ws_bytes, p.bytes)) return rc;
    // the trainer's own forward and backward; the running statistics it would update are a scratch copy
    Run r{{(char*)d_ws}, &p, const_cast<float*>(d_params), nullptr, d_grads, nullptr, (hipStream_t)stream, rnd};
    r.RS = r.at<float>(p.o_RS);
    OFP_HIP(hipMemsetAsync(r.RS, 0, (size_t)(p.ns > 0 ? p.ns : 1) * 4, r.st));
    return enqueue_loss_grads(r, d_x, d_y, n, d_loss);
}

int64_t ofp_linear_backward_workspace_bytes(int64_t rows, int32_t n_in, int32_t n_out) {
    if (rows < 1 || rows > kMaxRows || n_in < 1 || n_in > 4096 || n_out < 1 || n_out > 4096) return -1;
    return lin_part_bytes(rows, n_in, n_out);
}

int ofp_linear_backward(const float* d_x, int64_t rows, int32_t n_in, const float* d_w, int32_t n_out,
                        const float* d_dy, float* d_dx, float* d_dw, float* d_db, void* d_ws, int64_t ws_bytes,
                        void* stream) {
    const int64_t need = ofp_linear_backward_workspace_bytes(rows, n_in, n_out);
    OFP_REQUIRE(need >= 0, "ofp_linear_backward: %lld rows, %d inputs, %d outputs (limits: 1..%lld, 1..4096, 1..4096)",
                (long long)rows, n_in, n_out, (long long)kMaxRows);
    OFP_REQUIRE(d_x && d_w && d_dy && d_dw && d_db, "ofp_linear_backward: NULL argument");
    if (int rc = check_ws("ofp_linear_backward", d_ws, ws_bytes, need)) return rc;
    return enqueue_lin_bwd(nullptr, d_x, rows, n_in, n_out, d_w, d_dy, (double*)d_ws, d_dx, d_dw, d_db,
                           (hipStream_t)stream);
}

// work space of the GRU forward alone: W_ih^T, W_hh^T, the input projection
int64_t ofp_gru_train_forward_workspace_bytes(int64_t n, int32_t T, int32_t F, int32_t H) {
    if (check_gru("ofp_gru_train_forward", n, T, F, H)) return -1;
    return ofp::align_up((int64_t)3 * H * F * 4, 256) + ofp::align_up((int64_t)3 * H * H * 4, 256) + n * T * 3 * H * 4;
}

int ofp_gru_train_forward(const float* d_x, int64_t n, int32_t T, int32_t F, int32_t H, const float* d_w_ih,
                          const float* d_w_hh, const float* d_b_ih, const float* d_b_hh, float* d_out, float* d_gates,
                          void* d_ws, int64_t ws_bytes, void* stream) {
    if (int rc = check_gru("ofp_gru_train_forward", n, T, F, H)) return rc;
    OFP_REQUIRE(d_x && d_w_ih && d_w_hh && d_b_ih && d_b_hh && d_out && d_gates, "ofp_gru_train_forward: NULL argument");
    if (int rc = check_ws("ofp_gru_train_forward", d_ws, ws_bytes, ofp_gru_train_forward_workspace_bytes(n, T, F, H)))
        return rc;
    hipStream_t st = (hipStream_t)stream;
    float* wiht = (float*)d_ws;
    float* whht = reinterpret_cast<float*>((char*)d_ws + ofp::align_up((int64_t)3 * H * F * 4, 256));
    float* gx = reinterpret_cast<float*>((char*)whht + ofp::align_up((int64_t)3 * H * H * 4, 256));
    if (int rc = enqueue_transpose(nullptr, d_w_ih, 3 * H, F, wiht, st)) return rc;
    if (int rc = enqueue_transpose(nullptr, d_w_hh, 3 * H, H, whht, st)) return rc;
    if (int rc = enqueue_lin_fwd(nullptr, d_x, n * T, F, 3 * H, wiht, d_b_ih, gx, st)) return rc;
    return enqueue_gru_fwd(nullptr, gx, whht, d_b_hh, n, T, H, d_out, d_gates, st);
}

// work space of the GRU backward alone: dgx, dgh, the previous states, the weight gradients' slabs
int64_t ofp_gru_train_backward_workspace_bytes(int64_t n, int32_t T, int32_t F, int32_t H) {
    if (check_gru("ofp_gru_train_backward", n, T, F, H)) return -1;
    return 2 * ofp::align_up(n * T * 3 * H * 4, 256) + ofp::align_up(n * T * H * 4, 256) +
           lin_part_bytes(n * T, F > H ? F : H, 3 * H);
}

int ofp_gru_train_backward(const float* d_x, int64_t n, int32_t T, int32_t F, int32_t H, const float* d_w_ih,
                           const float* d_w_hh, const float* d_out, const float* d_gates, const float* d_dout,
                           float* d_dx, float* d_dw_ih, float* d_dw_hh, float* d_db_ih, float* d_db_hh, void* d_ws,
                           int64_t ws_bytes, void* stream) {
    if (int rc = check_gru("ofp_gru_train_backward", n, T, F, H)) return rc;
    OFP_REQUIRE(d_x && d_w_ih && d_w_hh && d_out && d_gates && d_dout && d_dx && d_dw_ih && d_dw_hh && d_db_ih &&
                    d_db_hh,
                "ofp_gru_train_backward: NULL argument");
    if (int rc = check_ws("ofp_gru_train_backward", d_ws, ws_bytes, ofp_gru_train_backward_workspace_bytes(n, T, F, H)))
        return rc;
    hipStream_t st = (hipStream_t)stream;
    const int64_t g3 = ofp::align_up(n * T * 3 * H * 4, 256);
    float* dgx = (float*)d_ws;
    float* dgh = reinterpret_cast<float*>((char*)d_ws + g3);
    float* hprev = reinterpret_cast<float*>((char*)d_ws + 2 * g3);
    double* part = reinterpret_cast<double*>((char*)hprev + ofp::align_up(n * T * H * 4, 256));
    if (int rc = enqueue_gru_bwd(nullptr, d_w_hh, d_out, d_gates, d_dout, n, T, H, dgx, dgh, hprev, st)) return rc;
    if (int rc = enqueue_lin_bwd(nullptr, hprev, n * T, H, 3 * H, d_w_hh, dgh, part, nullptr, d_dw_hh, d_db_hh, st))
        return rc;
    return enqueue_lin_bwd(nullptr, d_x, n * T, F, 3 * H, d_w_ih, dgx, part, d_dx, d_dw_ih, d_db_ih, st);
}

// work space of the attention forward alone: in_proj_weight^T
int64_t ofp_attention_mean_train_forward_workspace_bytes(int64_t n, int32_t T, int32_t E, int32_t heads) {
    if (check_attn("ofp_attention_mean_train_forward", n, T, E, heads)) return -1;
    return (int64_t)3 * E * E * 4;
}

int ofp_attention_mean_train_forward(const float* d_h, int64_t n, int32_t T, int32_t E, int32_t heads,
                                     const float* d_in_w, const float* d_in_b, const ofp_train_random* random,
                                     float* d_qkv, float* d_probs, float* d_ctx, void* d_ws, int64_t ws_bytes,
                                     void* stream) {
    Random rnd;
    if (int rc = check_attn("ofp_attention_mean_train_forward", n, T, E, heads)) return rc;
    if (int rc = attn_random("ofp_attention_mean_train_forward", random, rnd)) return rc;
    OFP_REQUIRE(d_h && d_in_w && d_in_b && d_qkv && d_probs && d_ctx, "ofp_attention_mean_train_forward: NULL argument");
    if (int rc = check_ws("ofp_attention_mean_train_forward", d_ws, ws_bytes, (int64_t)3 * E * E * 4)) return rc;
    hipStream_t st = (hipStream_t)stream;
    float* inwt = (float*)d_ws;
    if (int rc = enqueue_transpose(nullptr, d_in_w, 3 * E, E, inwt, st)) return rc;
    if (int rc = enqueue_lin_fwd(nullptr, d_h, n * T, E, 3 * E, inwt, d_in_b, d_qkv, st)) return rc;
    return enqueue_attn_fwd(nullptr, attn_of(n, T, E, heads, rnd, true), d_qkv, d_probs, d_ctx, st);
}

// work space of the attention backward alone: ds, dqkv, the in_proj gradients' slabs
int64_t ofp_attention_mean_train_backward_workspace_bytes(int64_t n, int32_t T, int32_t E, int32_t heads) {
    if (check_attn("ofp_attention_mean_train_backward", n, T, E, heads)) return -1;
    return ofp::align_up(n * heads * T * T * 4, 256) + ofp::align_up(n * T * 3 * E * 4, 256) +
           lin_part_bytes(n * T, E, 3 * E);
}

int ofp_attention_mean_train_backward(const float* d_h, int64_t n, int32_t T, int32_t E, int32_t heads,
                                      const float* d_in_w, const float* d_qkv, const float* d_probs,
                                      const float* d_dctx, const ofp_train_random* random, float* d_dh, float* d_dw,
                                      float* d_db, void* d_ws, int64_t ws_bytes, void* stream) {
    Random rnd;
    if (int rc = check_attn("ofp_attention_mean_train_backward", n, T, E, heads)) return rc;
    if (int rc = attn_random("ofp_attention_mean_train_backward", random, rnd)) return rc;
    OFP_REQUIRE(d_h && d_in_w && d_qkv && d_probs && d_dctx && d_dh && d_dw && d_db,
                "ofp_attention_mean_train_backward: NULL argument");
    if (int rc = check_ws("ofp_attention_mean_train_backward", d_ws, ws_bytes,
                          ofp_attention_mean_train_backward_workspace_bytes(n, T, E, heads)))
        return rc;
    hipStream_t st = (hipStream_t)stream;
    float* ds = (float*)d_ws;
    float* dqkv = reinterpret_cast<float*>((char*)d_ws + ofp::align_up(n * heads * T * T * 4, 256));
    double* part = reinterpret_cast<double*>((char*)dqkv + ofp::align_up(n * T * 3 * E * 4, 256));
    if (int rc = enqueue_attn_bwd(nullptr, attn_of(n, T, E, heads, rnd, true), d_qkv, d_probs, d_dctx, ds, dqkv, st))
        return rc;
    return enqueue_lin_bwd(nullptr, d_h, n * T, E, 3 * E, d_in_w, dqkv, part, d_dh, d_dw, d_db, st);
}

int ofp_attention_dropout_mask(uint64_t seed, int32_t epoch, int64_t n, int32_t heads, int32_t T, double p,
                               float* d_mask, void* stream) {
    OFP_REQUIRE(d_mask && n >= 1 && heads >= 1 && T >= 1 && n * heads * T * T <= ((int64_t)1 << 32),
                "ofp_attention_dropout_mask: NULL mask, or n %lld x %d heads x T %d outside 1..2^32 elements",
                (long long)n, heads, T);
    ofp_train_random o{};
    o.seed = seed, o.epoch = epoch, o.dropout_p = p;
    Random r;
    if (int rc = make_random("ofp_attention_dropout_mask", &o, 0, n, 0, 0, false, r)) return rc;
    const int64_t total = n * heads * T * T;
    hipLaunchKernelGGL(k_site_mask, dim3(grid_for(total)), dim3(kT), 0, (hipStream_t)stream, r.st, r.T, r.s,
                       kSiteAttention, total, d_mask);
    OFP_LAUNCH_CHECK("k_site_mask");
    return OFP_OK;
}

}  // extern "C"
