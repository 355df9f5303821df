// Training model.RNN on the GPU (the reference's model.py:168-307): a stack of L unidirectional GRU layers over the
// window itself (time = the window's samples, features = its channels), nn.GRU's dropout between the layers (site 4 of
// the random stream), LayerNorm, multi-head self-attention with dropout on the softmax probabilities (site 3), the mean
// over time, out_proj and the Linear head with its loss; backward through all of it, one NAdam step with torch's
// coupled weight decay, and optionally an eval-mode validation pass with the early-stop rule.  One epoch is a linear
// chain of kernels on one stream, captured once and replayed by run_epochs (csrc/ofp_train_chain.h).
//
// Shared with the CNNRNN trainer (csrc/ofp_seq_train.h): the dense layer, k_gru_fwd / k_gru_bwd, the attention pair
// (here its 512-step instantiation) and how they sum.  Kernels of this file:
//   k_inproj_fwd / k_inproj_wgrad_partial  layer 0's input projection and its weight gradient, read from the window
//       with strides (sequence, step, feature), F <= 8 features;
//   k_site_dropout  the inverted dropout of any site over consecutive elements from a base index, out of place (the
//       forward) or in place (the backward);
//   k_ln_fwd / k_ln_bwd_dx / k_ln_bwd_partial / k_ln_bwd_final  LayerNorm over rows of E <= 128, one wave per row;
//   k_nadam_decay  k_nadam with g + weight_decay p in place of g.
//
// Sums.  As in ofp_seq_train.h: no atomics, fp64, a fixed order that depends on the dimensions alone.  The sums over a
// LayerNorm row are an xor butterfly over the wave's 64 lanes (each lane first adds its elements e = lane, lane + 64);
// d gamma / d beta are cut into slabs of kLnSlab rows, two lanes per (slab, column) take the even and the odd rows in
// ascending order and are added even + odd, then the slabs in slab order.  The input projection's weight gradient cuts
// the n T rows into slabs of kInSlab; a workgroup takes (slab, 16 outputs), its 16 row lanes per output take rows sub,
// sub + 16, ... in ascending order and are joined by an xor butterfly inside the wave and then in wave order.
//
// Host side, by the contract of csrc/ofp_train_chain.h: the Plan is this file's GRU stack and LayerNorm and the AttnHead
// part (ofp_seq_train.h; it reads the LayerNorm output and hands dln back); enqueue_forward / _backward / _step / _reset
// for Run<Plan>; the traits Rnn.  The ofp_rnn_train_stretch* and ofp_rnn_loss_grads_random entries forward into
// train_workspace_bytes / train_entry / loss_grads_entry<Rnn>; the model has no running statistics (ns = 0).
#include "ofp_seq_train.h"

namespace {

constexpr uint32_t kSiteLayer = 4;   // nn.GRU's dropout on the output of every layer but the last [L - 1][n][T][H]
constexpr int kMaxSteps = kAttnCapLong;
constexpr int kMaxLayers = 4;
constexpr int kMaxIn = 8;            // channels of the window = features of layer 0
constexpr int kInSlab = 2048;        // rows one workgroup of the input projection's weight gradient sums
constexpr int kInOut = 16;           // ... and its outputs
constexpr int kLnRows = kT / 64;     // LayerNorm rows per workgroup, one wave each
constexpr int kLnSlab = 256;         // rows one workgroup of d gamma / d beta sums

// where element (sequence, step, feature) of the window lies
struct InStrides {
    int64_t seq, t, f;
};

// gx[r][o] = b[o] + sum_f x[r][f] w[o][f] for row r = seq T + t: thread per (row, output), the sum over f in ascending
// order in fp64, the bias added last -- the arithmetic of k_lin_fwd
__global__ __launch_bounds__(kT) void k_inproj_fwd(const Ctl* ctl, const float* __restrict__ x, const InStrides sx,
                                                   int64_t R, int T, int F, int O, const float* __restrict__ w,
                                                   const float* __restrict__ b, float* __restrict__ gx) {
    OFP_CNN_STOPPED(ctl);
    const int64_t total = R * O;
    for (int64_t e = (int64_t)blockIdx.x * kT + threadIdx.x; e < total; e += (int64_t)gridDim.x * kT) {
        const int64_t r = e / O;
        const int o = (int)(e - r * O);
        const int64_t s = r / T;
        const float* xr = x + s * sx.seq + (r - s * T) * sx.t;
        double acc = 0.0;
        for (int f = 0; f < F; ++f) acc = fma((double)xr[f * sx.f], (double)w[o * F + f], acc);
        gx[e] = (float)(acc + (double)b[o]);
    }
}

// dW[o][f] = sum_r dgx[r][o] x[r][f], db[o] = sum_r dgx[r][o] (column f == F) over the rows of one slab: workgroup
// (slab, kInOut outputs); thread = (row lane sub = tid / 16, output o0 + tid % 16) holds the F + 1 sums of its output
// over rows sub, sub + 16, ...; partial [slab][O][F + 1] as k_lin_wgrad_final reads it
__global__ __launch_bounds__(kT) void k_inproj_wgrad_partial(const Ctl* ctl, const float* __restrict__ x,
                                                             const InStrides sx, const float* __restrict__ dgx,
                                                             int64_t R, int T, int F, int O,
                                                             double* __restrict__ partial) {
    OFP_CNN_STOPPED(ctl);
    __shared__ double red[kT / 64][kInOut][kMaxIn + 1];
    const int slab = blockIdx.x, ol = threadIdx.x & (kInOut - 1), sub = threadIdx.x / kInOut;
    const int o = blockIdx.y * kInOut + ol;
    const int64_t ra = (int64_t)slab * kInSlab, rb = ra + kInSlab < R ? ra + kInSlab : R;
    double acc[kMaxIn + 1];
#pragma unroll
    for (int f = 0; f <= kMaxIn; ++f) acc[f] = 0.0;
    if (o < O)
        for (int64_t r = ra + sub; r < rb; r += kT / kInOut) {
            const int64_t s = r / T;
            const float* xr = x + s * sx.seq + (r - s * T) * sx.t;
            const double d = (double)dgx[r * O + o];
#pragma unroll
            for (int f = 0; f < kMaxIn; ++f)
                if (f < F) acc[f] = fma(d, (double)xr[f * sx.f], acc[f]);
            acc[kMaxIn] += d;
        }
    // the wave's four row lanes of an output (lanes ol, ol + 16, ol + 32, ol + 48), then the four waves in wave order
#pragma unroll
    for (int f = 0; f <= kMaxIn; ++f) {
        acc[f] += __shfl_xor(acc[f], 16);
        acc[f] += __shfl_xor(acc[f], 32);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane < kInOut) {
#pragma unroll
        for (int f = 0; f <= kMaxIn; ++f) red[wave][lane][f] = acc[f];
    }
    __syncthreads();
    for (int e = threadIdx.x; e < kInOut * (F + 1); e += kT) {
        const int u = e / (F + 1), f = e - u * (F + 1);
        const int c = f < F ? f : kMaxIn;
        if (blockIdx.y * kInOut + u < O)
            partial[((int64_t)slab * O + blockIdx.y * kInOut + u) * (F + 1) + f] =
                ((red[0][u][c] + red[1][u][c]) + red[2][u][c]) + red[3][u][c];
    }
}

// out[i] = in[i] * (0 or s) by word base + i of `site`; in == out is the backward's in-place form
__global__ __launch_bounds__(kT) void k_site_dropout(const Ctl* ctl, const Stream r, uint32_t thr, float s,
                                                     uint32_t site, uint32_t base, const float* in, float* out,
                                                     int64_t total) {
    OFP_CNN_STOPPED(ctl);
    for (int64_t i = (int64_t)blockIdx.x * kT + threadIdx.x; i < total; i += (int64_t)gridDim.x * kT)
        out[i] = in[i] * keep_scale(ctl, r, thr, s, true, site, base + (uint32_t)i);
}

__device__ __forceinline__ double wave_sum(double a) {
    for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o);
    return a;
}

// LayerNorm of one row per wave: mean and the biased variance about it in fp64, rstd = 1 / sqrt(var + eps), y = (x -
// mean) rstd gamma + beta evaluated in fp64 and rounded once; mean and rstd (rounded) are kept when asked for
__global__ __launch_bounds__(kT) void k_ln_fwd(const Ctl* ctl, const float* __restrict__ x, int64_t R, int E,
                                               const float* __restrict__ gamma, const float* __restrict__ beta,
                                               double eps, float* __restrict__ y, float* __restrict__ mean,
                                               float* __restrict__ rstd) {
    OFP_CNN_STOPPED(ctl);
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * kLnRows + (threadIdx.x >> 6);
    if (r >= R) return;  // a whole wave: no barrier follows
    const float* xr = x + r * E;
    const bool h0 = lane < E, h1 = lane + 64 < E;
    const double x0 = h0 ? (double)xr[lane] : 0.0, x1 = h1 ? (double)xr[lane + 64] : 0.0;
    const double m = wave_sum(x0 + x1) / (double)E;
    const double d0 = h0 ? x0 - m : 0.0, d1 = h1 ? x1 - m : 0.0;
    const double var = wave_sum(d0 * d0 + d1 * d1) / (double)E;
    const double rs = 1.0 / sqrt(var + eps);
    if (h0) y[r * E + lane] = (float)(d0 * rs * (double)gamma[lane] + (double)beta[lane]);
    if (h1) y[r * E + lane + 64] = (float)(d1 * rs * (double)gamma[lane + 64] + (double)beta[lane + 64]);
    if (lane == 0 && mean != nullptr) mean[r] = (float)m, rstd[r] = (float)rs;
}

// dx of one row per wave: with xhat = (x - mean) rstd and g = dy gamma, dx = rstd (g - mean_e(g) - xhat mean_e(g xhat))
__global__ __launch_bounds__(kT) void k_ln_bwd_dx(const Ctl* ctl, const float* __restrict__ x, int64_t R, int E,
                                                  const float* __restrict__ gamma, const float* __restrict__ mean,
                                                  const float* __restrict__ rstd, const float* __restrict__ dy,
                                                  float* __restrict__ dx) {
    OFP_CNN_STOPPED(ctl);
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * kLnRows + (threadIdx.x >> 6);
    if (r >= R) return;
    const float* xr = x + r * E;
    const float* dr = dy + r * E;
    const bool h0 = lane < E, h1 = lane + 64 < E;
    const double m = (double)mean[r], rs = (double)rstd[r];
    const double xh0 = h0 ? ((double)xr[lane] - m) * rs : 0.0, xh1 = h1 ? ((double)xr[lane + 64] - m) * rs : 0.0;
    const double g0 = h0 ? (double)dr[lane] * (double)gamma[lane] : 0.0;
    const double g1 = h1 ? (double)dr[lane + 64] * (double)gamma[lane + 64] : 0.0;
    const double a = wave_sum(g0 + g1) / (double)E;
    const double b = wave_sum(g0 * xh0 + g1 * xh1) / (double)E;
    if (h0) dx[r * E + lane] = (float)(rs * (g0 - a - xh0 * b));
    if (h1) dx[r * E + lane + 64] = (float)(rs * (g1 - a - xh1 * b));
}

// d gamma[e] = sum_r dy[r][e] xhat[r][e], d beta[e] = sum_r dy[r][e] over the rows of one slab: thread (half = tid /
// 128, e = tid % 128) takes rows half, half + 2, ... of the slab; partial [slab][2][E] = even + odd
__global__ __launch_bounds__(kT) void k_ln_bwd_partial(const Ctl* ctl, const float* __restrict__ x, int64_t R, int E,
                                                       const float* __restrict__ mean, const float* __restrict__ rstd,
                                                       const float* __restrict__ dy, double* __restrict__ partial) {
    OFP_CNN_STOPPED(ctl);
    __shared__ double odd[2][kT / 2];
    const int e = threadIdx.x & (kT / 2 - 1), half = threadIdx.x / (kT / 2);
    const int64_t ra = (int64_t)blockIdx.x * kLnSlab, rb = ra + kLnSlab < R ? ra + kLnSlab : R;
    double sg = 0.0, sb = 0.0;
    if (e < E)
        for (int64_t r = ra + half; r < rb; r += 2) {
            const double d = (double)dy[r * E + e];
            sg = fma(d, ((double)x[r * E + e] - (double)mean[r]) * (double)rstd[r], sg);
            sb += d;
        }
    if (half == 1) odd[0][e] = sg, odd[1][e] = sb;
    __syncthreads();
    if (half == 0 && e < E) {
        partial[((int64_t)blockIdx.x * 2) * E + e] = sg + odd[0][e];
        partial[((int64_t)blockIdx.x * 2 + 1) * E + e] = sb + odd[1][e];
    }
}

// the slabs in slab order
__global__ __launch_bounds__(kT) void k_ln_bwd_final(const Ctl* ctl, const double* __restrict__ partial, int nslab,
                                                     int E, float* __restrict__ dgamma, float* __restrict__ dbeta) {
    OFP_CNN_STOPPED(ctl);
    const int i = blockIdx.x * kT + threadIdx.x;
    if (i >= 2 * E) return;
    const int which = i / E, e = i - which * E;
    double s = 0.0;
    for (int j = 0; j < nslab; ++j) s += partial[((int64_t)j * 2 + which) * E + e];
    (which ? dbeta : dgamma)[e] = (float)s;
}

// k_nadam (csrc/ofp_cnn_stack.h) with torch's coupled weight decay: the gradient that enters the moments and the step
// is g + wd p, one fused multiply-add in fp32
__global__ __launch_bounds__(kT) void k_nadam_decay(const Ctl* ctl, const float* __restrict__ rows,
                                                    float* __restrict__ p, const float* __restrict__ g,
                                                    float* __restrict__ m, float* __restrict__ v, int64_t np, float wd) {
    OFP_CNN_STOPPED(ctl);
    const float* row = rows + (int64_t)(ctl ? ctl->epoch : 0) * 4;
    const float c1 = row[0], c2 = row[1], bc2 = row[2];
    for (int64_t i = (int64_t)blockIdx.x * kT + threadIdx.x; i < np; i += (int64_t)gridDim.x * kT) {
        const float gr = fmaf(wd, p[i], g[i]);
        const float mo = fmaf(0.1f, gr - m[i], m[i]);
        const float vo = v[i] * 0.999f + (0.001f * gr) * gr;
        m[i] = mo, v[i] = vo;
        const float denom = sqrtf(vo / bc2) + 1e-8f;
        p[i] = p[i] + ((c1 * gr) / denom + (c2 * mo) / denom);
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------

int in_slabs(int64_t R) { return (int)ofp::cdiv(R, kInSlab); }
int64_t in_part_bytes(int64_t R, int F, int O) { return (int64_t)in_slabs(R) * O * (F + 1) * 8; }
int ln_slabs(int64_t R) { return (int)ofp::cdiv(R, kLnSlab); }
int64_t ln_part_bytes(int64_t R, int E) { return (int64_t)ln_slabs(R) * 2 * E * 8; }

int enqueue_inproj_fwd(const Ctl* ctl, const float* x, const InStrides& sx, int64_t n, int T, int F, int O,
                       const float* w, const float* b, float* gx, hipStream_t st) {
    hipLaunchKernelGGL(k_inproj_fwd, dim3(grid_for(n * T * O)), dim3(kT), 0, st, ctl, x, sx, n * T, T, F, O, w, b, gx);
    OFP_LAUNCH_CHECK("k_inproj_fwd");
    return OFP_OK;
}

// dw [O][F] and db [O] of the input projection; `part` takes in_part_bytes
int enqueue_inproj_wgrad(const Ctl* ctl, const float* x, const InStrides& sx, const float* dgx, int64_t n, int T, int F,
                         int O, double* part, float* dw, float* db, hipStream_t st) {
    const int nslab = in_slabs(n * T);
    hipLaunchKernelGGL(k_inproj_wgrad_partial, dim3(nslab, (unsigned)ofp::cdiv(O, kInOut)), dim3(kT), 0, st, ctl, x, sx,
                       dgx, n * T, T, F, O, part);
    OFP_LAUNCH_CHECK("k_inproj_wgrad_partial");
    hipLaunchKernelGGL(k_lin_wgrad_final, dim3((unsigned)ofp::cdiv((int64_t)O * (F + 1), kT)), dim3(kT), 0, st, ctl,
                       part, nslab, F, O, dw, db);
    OFP_LAUNCH_CHECK("k_lin_wgrad_final");
    return OFP_OK;
}

// the dropout nn.GRU puts on layer l's output [n][T][H] (l < L - 1)
int enqueue_layer_dropout(const Ctl* ctl, const Random& r, int l, int64_t n, int T, int H, const float* in, float* out,
                          hipStream_t st) {
    const int64_t total = n * T * H;
    hipLaunchKernelGGL(k_site_dropout, dim3(grid_for(total)), dim3(kT), 0, st, ctl, r.st, r.T, r.s, kSiteLayer,
                       (uint32_t)((int64_t)l * total), in, out, total);
    OFP_LAUNCH_CHECK("k_site_dropout");
    return OFP_OK;
}

int enqueue_ln_fwd(const Ctl* ctl, const float* x, int64_t R, int E, const float* gamma, const float* beta, double eps,
                   float* y, float* mean, float* rstd, hipStream_t st) {
    hipLaunchKernelGGL(k_ln_fwd, dim3((unsigned)ofp::cdiv(R, kLnRows)), dim3(kT), 0, st, ctl, x, R, E, gamma, beta, eps,
                       y, mean, rstd);
    OFP_LAUNCH_CHECK("k_ln_fwd");
    return OFP_OK;
}

// `part` takes ln_part_bytes
int enqueue_ln_bwd(const Ctl* ctl, const float* x, int64_t R, int E, const float* gamma, const float* mean,
                   const float* rstd, const float* dy, double* part, float* dx, float* dgamma, float* dbeta,
                   hipStream_t st) {
    const int nslab = ln_slabs(R);
    hipLaunchKernelGGL(k_ln_bwd_partial, dim3(nslab), dim3(kT), 0, st, ctl, x, R, E, mean, rstd, dy, part);
    OFP_LAUNCH_CHECK("k_ln_bwd_partial");
    hipLaunchKernelGGL(k_ln_bwd_final, dim3(1), dim3(kT), 0, st, ctl, part, nslab, E, dgamma, dbeta);
    OFP_LAUNCH_CHECK("k_ln_bwd_final");
    hipLaunchKernelGGL(k_ln_bwd_dx, dim3((unsigned)ofp::cdiv(R, kLnRows)), dim3(kT), 0, st, ctl, x, R, E, gamma, mean,
                       rstd, dy, dx);
    OFP_LAUNCH_CHECK("k_ln_bwd_dx");
    return OFP_OK;
}

// ---- the GRU stack ---------------------------------------------------------------------------------------------------
// Parameters of the stack packed as nn.GRU lists them: per layer weight_ih [3H][F_l], weight_hh [3H][H], bias_ih [3H],
// bias_hh [3H], with F_0 = F and F_l = H above.

struct Stack {
    int64_t n;
    int T, F, H, L;
    InStrides sx;
    int wih[kMaxLayers], whh[kMaxLayers], bih[kMaxLayers], bhh[kMaxLayers], np;
};

Stack stack_of(int64_t n, int T, int F, int H, int L, const InStrides& sx) {
    Stack s{n, T, F, H, L, sx, {}, {}, {}, {}, 0};
    for (int l = 0; l < L; ++l) {
        s.wih[l] = s.np, s.np += 3 * H * (l ? H : F);
        s.whh[l] = s.np, s.np += 3 * H * H;
        s.bih[l] = s.np, s.np += 3 * H;
        s.bhh[l] = s.np, s.np += 3 * H;
    }
    return s;
}

int check_stack(const char* who, int64_t n, int T, int F, int H, int L) {
    if (int rc = check_gru(who, n, T, F, H, kMaxSteps, kMaxIn)) return rc;
    OFP_REQUIRE(L >= 1 && L <= kMaxLayers, "%s: %d layers (limit: 1..%d)", who, L, kMaxLayers);
    OFP_REQUIRE((int64_t)(L - 1) * n * T * H < ((int64_t)1 << 32),
                "%s: %d layers x %lld x %d x %d outputs between the layers: the random stream indexes 2^32 elements",
                who, L, (long long)n, T, H);
    return OFP_OK;
}

// the stack's buffers: `seqs` and `gates` hold every layer ([L][rows][H], [L][rows][4H]); `drop` [L - 1][rows][H] the
// dropped outputs (only with dropout); the others are scratch of one layer
struct StackBufs {
    float* wt;     // a weight's transposed copy, 3H x max(H, 1) floats
    float* gx;     // [rows][3H]
    float* seqs;
    float* gates;
    float* drop;
    float* dgx;    // backward: [rows][3H]
    float* dgh;    // [rows][3H]
    float* hprev;  // [rows][H]
    float* dseq;   // [rows][H]: the gradient at the current layer's output; the caller fills it for the last layer
    double* part;
};

int64_t stack_part_bytes(int64_t n, int T, int F, int H) {
    return std::max(lin_part_bytes(n * T, H, 3 * H), in_part_bytes(n * T, F, 3 * H));
}

// what layer l + 1 reads of layer l
const float* layer_output(const Stack& s, const StackBufs& b, bool drop, int l) {
    const int64_t per = s.n * s.T * s.H;
    return (drop ? b.drop : b.seqs) + (int64_t)l * per;
}

int enqueue_stack_fwd(const Ctl* ctl, const Stack& s, const StackBufs& b, const Random& rnd, bool train, const float* x,
                      const float* P, hipStream_t st) {
    const int H = s.H, T = s.T;
    const int64_t rows = s.n * T;
    const bool drop = train && rnd.drop;
    for (int l = 0; l < s.L; ++l) {
        if (l == 0) {
            if (int rc = enqueue_inproj_fwd(ctl, x, s.sx, s.n, T, s.F, 3 * H, P + s.wih[0], P + s.bih[0], b.gx, st))
                return rc;
        } else {
            if (int rc = enqueue_transpose(ctl, P + s.wih[l], 3 * H, H, b.wt, st)) return rc;
            if (int rc = enqueue_lin_fwd(ctl, layer_output(s, b, drop, l - 1), rows, H, 3 * H, b.wt, P + s.bih[l], b.gx,
                                         st))
                return rc;
        }
        if (int rc = enqueue_transpose(ctl, P + s.whh[l], 3 * H, H, b.wt, st)) return rc;
        float* seq = b.seqs + (int64_t)l * rows * H;
        if (int rc = enqueue_gru_fwd(ctl, b.gx, b.wt, P + s.bhh[l], s.n, T, H, seq, b.gates + (int64_t)l * rows * 4 * H,
                                     st))
            return rc;
        if (drop && l < s.L - 1)
            if (int rc = enqueue_layer_dropout(ctl, rnd, l, s.n, T, H, seq, b.drop + (int64_t)l * rows * H, st))
                return rc;
    }
    return OFP_OK;
}

// b.dseq holds the gradient at the last layer's output and is overwritten on the way down; G is packed like P
int enqueue_stack_bwd(const Ctl* ctl, const Stack& s, const StackBufs& b, const Random& rnd, const float* x,
                      const float* P, float* G, hipStream_t st) {
    const int H = s.H, T = s.T;
    const int64_t rows = s.n * T;
    for (int l = s.L - 1; l >= 0; --l) {
        if (int rc = enqueue_gru_bwd(ctl, P + s.whh[l], b.seqs + (int64_t)l * rows * H,
                                     b.gates + (int64_t)l * rows * 4 * H, b.dseq, s.n, T, H, b.dgx, b.dgh, b.hprev, st))
            return rc;
        if (int rc = enqueue_lin_bwd(ctl, b.hprev, rows, H, 3 * H, P + s.whh[l], b.dgh, b.part, nullptr, G + s.whh[l],
                                     G + s.bhh[l], st))
            return rc;
        if (l == 0)
            return enqueue_inproj_wgrad(ctl, x, s.sx, b.dgx, s.n, T, s.F, 3 * H, b.part, G + s.wih[0], G + s.bih[0],
                                        st);
        // layer l's dx is the gradient at what it read: layer l - 1's output after its dropout
        if (int rc = enqueue_lin_bwd(ctl, layer_output(s, b, rnd.drop, l - 1), rows, H, 3 * H, P + s.wih[l], b.dgx,
                                     b.part, b.dseq, G + s.wih[l], G + s.bih[l], st))
            return rc;
        if (rnd.drop)
            if (int rc = enqueue_layer_dropout(ctl, rnd, l - 1, s.n, T, H, b.dseq, b.dseq, st)) return rc;
    }
    return OFP_OK;
}

// the strides of x [n][T][F] (permuted == 0) or [n][F][T] (the window as it is stored)
InStrides strides_of(int T, int F, int permuted) {
    return permuted ? InStrides{(int64_t)F * T, 1, T} : InStrides{(int64_t)T * F, F, 1};
}

// ---- the trainer -----------------------------------------------------------------------------------------------------

struct Plan : WsPlan {
    Stack s;
    AttnHead head;
    double eps;
    float wd;
    int lnw_off, lnb_off;
    int64_t o_wt, o_gx, o_seqs, o_gates, o_drop, o_ln, o_mean, o_rstd, o_dln, o_dseq, o_dgx, o_dgh, o_hprev, o_part, o_M,
        o_V;
};

int make_plan(const char* who, const ofp_rnn_config* c, int64_t n, int64_t n_val, Plan& p, const Random& rnd) {
    OFP_REQUIRE(c != nullptr, "%s: config is NULL", who);
    OFP_REQUIRE(n_val >= 0 && n_val <= kMaxBatch, "%s: validation batch of %lld (limit: 0..%d)", who, (long long)n_val,
                kMaxBatch);
    if (int rc = check_stack(who, n, c->width, c->channels, c->hidden, c->layers)) return rc;
    OFP_REQUIRE(n * c->heads * c->width * c->width < ((int64_t)1 << 32),
                "%s: %lld x %d heads x %d^2 attention probabilities: the random stream indexes 2^32 elements", who,
                (long long)n, c->heads, c->width);
    OFP_REQUIRE(c->loss == 0 || c->loss == 1, "%s: loss %d (0 = L1, 1 = MSE)", who, c->loss);
    OFP_REQUIRE(c->n_out >= 1 && c->n_out <= kMaxOut, "%s: %d outputs (limit: 1..%d)", who, c->n_out, kMaxOut);
    OFP_REQUIRE(c->ln_eps > 0.0 && c->weight_decay >= 0.0f, "%s: LayerNorm eps %g, weight decay %g", who, c->ln_eps,
                (double)c->weight_decay);
    OFP_REQUIRE(!rnd.windows || c->permute_input, "%s: a window source gives [n][channels][width] (permute_input)", who);
    p = Plan{};
    const int T = c->width, F = c->channels, H = c->hidden, L = c->layers;
    const int64_t nmax = n > n_val ? n : n_val, rows = nmax * T;
    p.s = stack_of(n, T, F, H, L, strides_of(T, F, c->permute_input));
    p.eps = c->ln_eps, p.wd = c->weight_decay;
    p.np = p.s.np;
    p.lnw_off = p.np, p.np += H;
    p.lnb_off = p.np, p.np += H;
    int64_t max_part = std::max(stack_part_bytes(n, T, F, H), ln_part_bytes(n * T, H));
    p.o_wt = p.take((int64_t)3 * H * H * 4);
    if (int rc = plan_attn_head(who, n, T, H, c->heads, c->n_out, c->loss, kMaxSteps, p, p.np, max_part, p.head))
        return rc;
    p.o_gx = p.take(rows * 3 * H * 4);
    p.o_seqs = p.take(L * rows * H * 4);
    p.o_gates = p.take(L * rows * 4 * H * 4);
    p.o_ln = p.take(rows * H * 4);
    p.o_mean = p.take(rows * 4);
    p.o_rstd = p.take(rows * 4);
    take_attn_head_blocks(p, n, nmax, p.head);
    p.o_dln = p.take(n * T * H * 4);
    p.o_dseq = p.take(n * T * H * 4);
    p.o_dgx = p.take(n * T * 3 * H * 4);
    p.o_dgh = p.take(n * T * 3 * H * 4);
    p.o_hprev = p.take(n * T * H * 4);
    p.o_part = p.take(max_part);
    p.o_G = p.take((int64_t)p.np * 4);
    p.o_M = p.take((int64_t)p.np * 4);
    p.o_V = p.take((int64_t)p.np * 4);
    p.o_ctl = p.take(sizeof(Ctl));
    if (rnd.drop && L > 1) p.o_drop = p.take((int64_t)(L - 1) * n * T * H * 4);
    if (rnd.windows) p.o_X = p.take(n * F * T * 4);
    return OFP_OK;
}

// the stack's view of the work space for a batch of n sequences
Stack stack_for(const Run<Plan>& r, int64_t n) {
    Stack s = r.p->s;
    s.n = n;
    return s;
}

StackBufs bufs_of(const Run<Plan>& r) {
    const Plan& p = *r.p;
    return StackBufs{r.at<float>(p.o_wt),  r.at<float>(p.o_gx),    r.at<float>(p.o_seqs), r.at<float>(p.o_gates),
                     r.at<float>(p.o_drop), r.at<float>(p.o_dgx),  r.at<float>(p.o_dgh),  r.at<float>(p.o_hprev),
                     r.at<float>(p.o_dseq), r.at<double>(p.o_part)};
}

// the whole network on a batch, its mean loss into `curve`; train: both dropouts, d loss / d out kept and the head's
// bias gradient; else no dropout, L1 and the early-stop rule
int enqueue_forward(const Run<Plan>& r, const float* x, const float* y, int64_t n, bool train, float* curve,
                    int patience) {
    const Plan& p = *r.p;
    const Stack s = stack_for(r, n);
    const int T = s.T, H = s.H;
    if (int rc = enqueue_stack_fwd(r.ctl, s, bufs_of(r), r.rnd, train, x, r.P, r.st)) return rc;
    const float* top = r.at<float>(p.o_seqs) + (int64_t)(s.L - 1) * n * T * H;
    float* ln = r.at<float>(p.o_ln);
    if (int rc = enqueue_ln_fwd(r.ctl, top, n * T, H, r.P + p.lnw_off, r.P + p.lnb_off, p.eps, ln,
                                r.at<float>(p.o_mean), r.at<float>(p.o_rstd), r.st))
        return rc;
    return enqueue_attn_head_fwd(r, p.head, kMaxSteps, ln, n, y, train, curve, patience);
}

int enqueue_backward(const Run<Plan>& r, const float* x, int64_t n) {
    const Plan& p = *r.p;
    const Stack s = stack_for(r, n);
    const int T = s.T, H = s.H;
    double* part = r.at<double>(p.o_part);
    float* dln = r.at<float>(p.o_dln);
    const float* top = r.at<float>(p.o_seqs) + (int64_t)(s.L - 1) * n * T * H;
    if (int rc = enqueue_attn_head_bwd(r, p.head, kMaxSteps, r.at<float>(p.o_ln), n, part, dln)) return rc;
    if (int rc = enqueue_ln_bwd(r.ctl, top, n * T, H, r.P + p.lnw_off, r.at<float>(p.o_mean), r.at<float>(p.o_rstd),
                                dln, part, r.at<float>(p.o_dseq), r.G + p.lnw_off, r.G + p.lnb_off, r.st))
        return rc;
    return enqueue_stack_bwd(r.ctl, s, bufs_of(r), r.rnd, x, r.P, r.G, r.st);
}

int enqueue_step(const Run<Plan>& r, const float* rows) {
    const Plan& p = *r.p;
    hipLaunchKernelGGL(k_nadam_decay, dim3(grid_for(p.np)), dim3(kT), 0, r.st, r.ctl, rows, r.P, r.G,
                       r.at<float>(p.o_M), r.at<float>(p.o_V), (int64_t)p.np, p.wd);
    OFP_LAUNCH_CHECK("k_nadam_decay");
    return OFP_OK;
}

int enqueue_reset(const Run<Plan>& r) {
    return zero_moments(r.at<float>(r.p->o_M), r.at<float>(r.p->o_V), r.p->np, r.st);
}

struct Rnn {
    using Config = ofp_rnn_config;
    using Plan = ::Plan;
    static constexpr const char* train = "ofp_rnn_train";
    static constexpr const char* grads = "ofp_rnn_loss_grads";
    static constexpr const char* env = "OFP_RNN_GRAPH";
    static Window window_of(const Config& c) { return Window{c.channels, c.width}; }
    static constexpr auto make_plan = ::make_plan;
};

}  // namespace

extern "C" {

int64_t ofp_rnn_train_stretch_workspace_bytes(const ofp_rnn_config* cfg, int64_t n, int64_t n_val,
                                              const ofp_train_random* random, int32_t stretch_span) {
    return train_workspace_bytes<Rnn>(cfg, n, n_val, random, stretch_span);
}

int ofp_rnn_train_stretch(const ofp_rnn_config* cfg, int64_t n, const float* d_x, const float* d_y, int64_t n_val,
                          const float* d_x_val, const float* d_y_val, const float* d_rates, int32_t num_epochs,
                          int32_t min_epochs, int32_t patience, float* d_params, float* d_train_loss,
                          float* d_val_loss, int32_t* h_epochs, void* d_ws, int64_t ws_bytes, void* stream,
                          const ofp_train_random* random, int32_t stretch_span) {
    return train_entry<Rnn>(cfg, n, d_x, d_y, n_val, d_x_val, d_y_val, d_rates, num_epochs, min_epochs, patience, d_params,
                            nullptr, d_train_loss, d_val_loss, h_epochs, d_ws, ws_bytes, stream, random, stretch_span);
}

int64_t ofp_rnn_loss_grads_random_workspace_bytes(const ofp_rnn_config* cfg, int64_t n, int64_t n_val,
                                                  const ofp_train_random* random) {
    return ofp_rnn_train_stretch_workspace_bytes(cfg, n, n_val, random, 0);
}

int ofp_rnn_loss_grads_random(const ofp_rnn_config* cfg, int64_t n, const float* d_x, const float* d_y,
                              const float* d_params, float* d_loss, float* d_grads, void* d_ws, int64_t ws_bytes,
                              void* stream, const ofp_train_random* random) {
    return loss_grads_entry<Rnn>(cfg, n, d_x, d_y, d_params, d_loss, d_grads, d_ws, ws_bytes, stream, random);
}

int ofp_layernorm_train_forward(const float* d_x, int64_t rows, int32_t E, const float* d_gamma, const float* d_beta,
                                double eps, float* d_y, float* d_mean, float* d_rstd, void* stream) {
    OFP_REQUIRE(rows >= 1 && rows <= kMaxRows && E >= 1 && E <= kMaxHidden && eps > 0.0,
                "ofp_layernorm_train_forward: %lld rows of %d, eps %g (limits: 1..%lld rows, width 1..%d, eps > 0)",
                (long long)rows, E, eps, (long long)kMaxRows, kMaxHidden);
    OFP_REQUIRE(d_x && d_gamma && d_beta && d_y && d_mean && d_rstd, "ofp_layernorm_train_forward: NULL argument");
    return enqueue_ln_fwd(nullptr, d_x, rows, E, d_gamma, d_beta, eps, d_y, d_mean, d_rstd, (hipStream_t)stream);
}

int64_t ofp_layernorm_train_backward_workspace_bytes(int64_t rows, int32_t E) {
    if (rows < 1 || rows > kMaxRows || E < 1 || E > kMaxHidden) return -1;
    return ln_part_bytes(rows, E);
}

int ofp_layernorm_train_backward(const float* d_x, int64_t rows, int32_t E, const float* d_gamma, const float* d_mean,
                                 const float* d_rstd, const float* d_dy, float* d_dx, float* d_dgamma, float* d_dbeta,
                                 void* d_ws, int64_t ws_bytes, void* stream) {
    const int64_t need = ofp_layernorm_train_backward_workspace_bytes(rows, E);
    OFP_REQUIRE(need >= 0, "ofp_layernorm_train_backward: %lld rows of %d (limits: 1..%lld rows, width 1..%d)",
                (long long)rows, E, (long long)kMaxRows, kMaxHidden);
    OFP_REQUIRE(d_x && d_gamma && d_mean && d_rstd && d_dy && d_dx && d_dgamma && d_dbeta,
                "ofp_layernorm_train_backward: NULL argument");
    if (int rc = check_ws("ofp_layernorm_train_backward", d_ws, ws_bytes, need)) return rc;
    return enqueue_ln_bwd(nullptr, d_x, rows, E, d_gamma, d_mean, d_rstd, d_dy, (double*)d_ws, d_dx, d_dgamma, d_dbeta,
                          (hipStream_t)stream);
}

// work space of the stack's forward alone: a transposed weight, the input projection, the dropped outputs
int64_t ofp_rnn_gru_train_forward_workspace_bytes(int64_t n, int32_t T, int32_t F, int32_t H, int32_t L) {
    if (check_stack("ofp_rnn_gru_train_forward", n, T, F, H, L)) return -1;
    return ofp::align_up((int64_t)3 * H * H * 4, 256) + ofp::align_up(n * T * 3 * H * 4, 256) +
           ofp::align_up((int64_t)(L > 1 ? L - 1 : 1) * n * T * H * 4, 256);
}

int ofp_rnn_gru_train_forward(const float* d_x, int32_t permuted, int64_t n, int32_t T, int32_t F, int32_t H, int32_t L,
                              const float* d_params, const ofp_train_random* random, float* d_seqs, float* d_gates,
                              void* d_ws, int64_t ws_bytes, void* stream) {
    Random rnd;
    if (int rc = check_stack("ofp_rnn_gru_train_forward", n, T, F, H, L)) return rc;
    if (int rc = attn_random("ofp_rnn_gru_train_forward", random, rnd)) return rc;
    OFP_REQUIRE(d_x && d_params && d_seqs && d_gates, "ofp_rnn_gru_train_forward: NULL argument");
    if (int rc = check_ws("ofp_rnn_gru_train_forward", d_ws, ws_bytes,
                          ofp_rnn_gru_train_forward_workspace_bytes(n, T, F, H, L)))
        return rc;
    StackBufs b{};
    b.wt = (float*)d_ws;
    b.gx = reinterpret_cast<float*>((char*)d_ws + ofp::align_up((int64_t)3 * H * H * 4, 256));
    b.drop = reinterpret_cast<float*>((char*)b.gx + ofp::align_up(n * T * 3 * H * 4, 256));
    b.seqs = d_seqs, b.gates = d_gates;
    return enqueue_stack_fwd(nullptr, stack_of(n, T, F, H, L, strides_of(T, F, permuted)), b, rnd, true, d_x, d_params,
                             (hipStream_t)stream);
}

// work space of the stack's backward alone: dgx, dgh, the previous states, the running gradient, the dropped outputs
// (recomputed from d_seqs), the weight gradients' slabs
int64_t ofp_rnn_gru_train_backward_workspace_bytes(int64_t n, int32_t T, int32_t F, int32_t H, int32_t L) {
    if (check_stack("ofp_rnn_gru_train_backward", n, T, F, H, L)) return -1;
    return 2 * ofp::align_up(n * T * 3 * H * 4, 256) + 2 * ofp::align_up(n * T * H * 4, 256) +
           ofp::align_up((int64_t)(L > 1 ? L - 1 : 1) * n * T * H * 4, 256) + stack_part_bytes(n, T, F, H);
}

int ofp_rnn_gru_train_backward(const float* d_x, int32_t permuted, int64_t n, int32_t T, int32_t F, int32_t H, int32_t L,
                               const float* d_params, const ofp_train_random* random, const float* d_seqs,
                               const float* d_gates, const float* d_dseq, float* d_grads, void* d_ws, int64_t ws_bytes,
                               void* stream) {
    Random rnd;
    if (int rc = check_stack("ofp_rnn_gru_train_backward", n, T, F, H, L)) return rc;
    if (int rc = attn_random("ofp_rnn_gru_train_backward", random, rnd)) return rc;
    OFP_REQUIRE(d_x && d_params && d_seqs && d_gates && d_dseq && d_grads, "ofp_rnn_gru_train_backward: NULL argument");
    if (int rc = check_ws("ofp_rnn_gru_train_backward", d_ws, ws_bytes,
                          ofp_rnn_gru_train_backward_workspace_bytes(n, T, F, H, L)))
        return rc;
    hipStream_t st = (hipStream_t)stream;
    const int64_t g3 = ofp::align_up(n * T * 3 * H * 4, 256), g1 = ofp::align_up(n * T * H * 4, 256);
    const Stack s = stack_of(n, T, F, H, L, strides_of(T, F, permuted));
    StackBufs b{};
    char* w = (char*)d_ws;
    b.dgx = (float*)w, w += g3;
    b.dgh = (float*)w, w += g3;
    b.hprev = (float*)w, w += g1;
    b.dseq = (float*)w, w += g1;
    b.drop = (float*)w, w += ofp::align_up((int64_t)(L > 1 ? L - 1 : 1) * n * T * H * 4, 256);
    b.part = (double*)w;
    b.seqs = const_cast<float*>(d_seqs), b.gates = const_cast<float*>(d_gates);
    OFP_HIP(hipMemcpyAsync(b.dseq, d_dseq, (size_t)(n * T * H) * 4, hipMemcpyDeviceToDevice, st));
    if (rnd.drop)
        for (int l = 0; l + 1 < L; ++l)
            if (int rc = enqueue_layer_dropout(nullptr, rnd, l, n, T, H, d_seqs + (int64_t)l * n * T * H,
                                               b.drop + (int64_t)l * n * T * H, st))
                return rc;
    return enqueue_stack_bwd(nullptr, s, b, rnd, d_x, d_params, d_grads, st);
}

int64_t ofp_rnn_attention_train_forward_workspace_bytes(int64_t n, int32_t T, int32_t E, int32_t heads) {
    return attn_fwd_alone_bytes("ofp_rnn_attention_train_forward", n, T, E, heads, kMaxSteps);
}

int ofp_rnn_attention_train_forward(const float* d_h, int64_t n, int32_t T, int32_t E, int32_t heads,
                                    const float* d_in_w, const float* d_in_b, const ofp_train_random* random,
                                    float* d_qkv, float* d_probs, float* d_ctx, void* d_ws, int64_t ws_bytes,
                                    void* stream) {
    OFP_REQUIRE(n * heads * (int64_t)T * T < ((int64_t)1 << 32),
                "ofp_rnn_attention_train_forward: %lld x %d heads x %d^2 probabilities: the random stream indexes 2^32 "
                "elements",
                (long long)n, heads, T);
    return attn_fwd_alone("ofp_rnn_attention_train_forward", kMaxSteps, d_h, n, T, E, heads, d_in_w, d_in_b, random,
                          d_qkv, d_probs, d_ctx, d_ws, ws_bytes, stream);
}

int64_t ofp_rnn_attention_train_backward_workspace_bytes(int64_t n, int32_t T, int32_t E, int32_t heads) {
    return attn_bwd_alone_bytes("ofp_rnn_attention_train_backward", n, T, E, heads, kMaxSteps);
}

int ofp_rnn_attention_train_backward(const float* d_h, int64_t n, int32_t T, int32_t E, int32_t heads,
                                     const float* d_in_w, const float* d_qkv, const float* d_probs,
                                     const float* d_dctx, const ofp_train_random* random, float* d_dh, float* d_dw,
                                     float* d_db, void* d_ws, int64_t ws_bytes, void* stream) {
    OFP_REQUIRE(n * heads * (int64_t)T * T < ((int64_t)1 << 32),
                "ofp_rnn_attention_train_backward: %lld x %d heads x %d^2 probabilities: the random stream indexes 2^32 "
                "elements",
                (long long)n, heads, T);
    return attn_bwd_alone("ofp_rnn_attention_train_backward", kMaxSteps, d_h, n, T, E, heads, d_in_w, d_qkv, d_probs,
                          d_dctx, random, d_dh, d_dw, d_db, d_ws, ws_bytes, stream);
}

int ofp_rnn_layer_dropout_mask(uint64_t seed, int32_t epoch, int32_t layers, int64_t n, int32_t T, int32_t H, double p,
                               float* d_mask, void* stream) {
    OFP_REQUIRE(d_mask && layers >= 1 && n >= 1 && T >= 1 && H >= 1 && (int64_t)layers * n * T * H <= ((int64_t)1 << 32),
                "ofp_rnn_layer_dropout_mask: NULL mask, or %d layers x n %lld x T %d x H %d outside 1..2^32 elements",
                layers, (long long)n, T, H);
    ofp_train_random o{};
    o.seed = seed, o.epoch = epoch, o.dropout_p = p;
    Random r;
    if (int rc = make_random("ofp_rnn_layer_dropout_mask", &o, 0, n, 0, 0, false, r)) return rc;
    const int64_t total = (int64_t)layers * n * T * H;
    hipLaunchKernelGGL(k_site_mask, dim3(grid_for(total)), dim3(kT), 0, (hipStream_t)stream, r.st, r.T, r.s, kSiteLayer,
                       total, d_mask);
    OFP_LAUNCH_CHECK("k_site_mask");
    return OFP_OK;
}

int ofp_nadam_decay_step(float* d_p, const float* d_g, float* d_m, float* d_v, int64_t n, const float* d_row,
                         float weight_decay, void* stream) {
    OFP_REQUIRE(d_p && d_g && d_m && d_v && d_row && n >= 1 && weight_decay >= 0.0f,
                "ofp_nadam_decay_step: NULL argument, n < 1 or a negative weight decay");
    hipLaunchKernelGGL(k_nadam_decay, dim3(grid_for(n)), dim3(kT), 0, (hipStream_t)stream, (const Ctl*)nullptr, d_row,
                       d_p, d_g, d_m, d_v, n, weight_decay);
    OFP_LAUNCH_CHECK("k_nadam_decay");
    return OFP_OK;
}

}  // extern "C"
