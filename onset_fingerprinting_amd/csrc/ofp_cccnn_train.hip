// Training model.CCCNN / model.LCCCNN on the GPU (the reference's model.py:443-629 and the loop of train.py): full-batch
// forward, mean L1 / MSE loss, backward through the correlation head, SGD with momentum and weight decay, and
// optionally a validation pass with Lightning's early-stop rule.  As in csrc/ofp_cnn_train.hip one epoch is a linear
// chain of short kernels on one stream, captured once as a hipGraph and replayed; the epoch index is a device counter
// and once the stop word is set every kernel returns at once.  With random options (ofp_cccnn_train_random) the
// epoch's windows come from k_shift_windows (k_stretch_windows with a stretch span, ofp_cccnn_train_stretch) and the
// head's p goes through k_dropout_fwd in front of the Linear (csrc/ofp_train_random.h), as in csrc/ofp_cnn_train.hip.
//
// The conv stack works on items: with group = 0 every (sample, sensor) pair is an item with 1 input channel (the
// shared stack), with group = 1 every sample is an item with `sensors` input channels and a grouped convolution.
// Layer order as the reference builds it: conv (own kernel size and stride) + bias -> activation -> GroupNorm(1, C)
// -> MaxPool1d(2, 2).  GroupNorm normalises one item over all its channels and has no running statistics, so the
// training forward is the eval forward.  Kept per layer: the pre-activation z [items][C][Wc], the output
// [items][C][Wo] and the item's mean / rstd; the head keeps the softmax p [n * sensors][2V - 1].  Activation,
// normalised value and pool choice are recomputed from z in the backward (ties take the first of the pair, an odd
// last column gets no gradient).
//
// Reductions.  No atomics.  Sums inside an item (GroupNorm's statistics and its two backward sums, the head's
// p . dp) are one workgroup's fp64 sums in an order fixed by the thread index.  Sums over the batch (GroupNorm's
// d gamma / d beta, the convolution's weight and bias gradients, the Linear head's) go through the partial-slab
// reducer of ofp_train_chain.h.  Results are bitwise reproducible.
//
// Host side, by the contract of csrc/ofp_train_chain.h: this file's own Plan (GroupNorm and a strided stack: no part is
// shared), enqueue_forward / _backward / _step / _reset for Run<Plan>, the traits Cccnn.  The ofp_cccnn_train* and
// ofp_cccnn_loss_grads* entries forward into train_workspace_bytes / train_entry / loss_grads_entry<Cccnn>; the model
// has no running statistics (ns = 0).
#include "ofp_train_random.h"

#include <algorithm>

namespace {

constexpr int kMaxConv = 8;
constexpr int kMaxCh = 64;
constexpr int kMaxKernel = 64;
constexpr int kMaxStride = 4;
constexpr int kMaxWidth = 512;
constexpr int kMaxBatch = 1024;
constexpr int kMaxItems = 4096;
constexpr size_t kMaxLds = 160 * 1024;

// what follows the convolution inside an item: activation, GroupNorm(1, C) (norm != 0), pool
struct Norm {
    int C, wc, wo, act, pool, norm;
    double eps;
    const float* ga;
    const float* be;
};

__device__ __forceinline__ float gn_value(const Norm& t, float mean, float rstd, float g, float b, float z) {
    const float a = ofp_activate(z, t.act);
    return t.norm ? (a - mean) * rstd * g + b : a;
}

// gradient that reaches position p of the un-pooled row zr (see routed_dy of csrc/ofp_cnn_train.hip)
__device__ __forceinline__ float gn_routed(const Norm& t, float mean, float rstd, float g, float b, const float* zr,
                                           const float* dhr, int p) {
    if (!t.pool) return dhr[p];
    const int po = p >> 1;
    if (po >= t.wo) return 0.0f;
    const float y0 = gn_value(t, mean, rstd, g, b, zr[2 * po]);
    const float y1 = gn_value(t, mean, rstd, g, b, zr[2 * po + 1]);
    const bool second = y1 > y0;
    return ((p & 1) != 0) == second ? dhr[po] : 0.0f;
}

// the layer's output of one item per workgroup: mean and rstd of act(z) over the item's C * wc values from fp64
// sums (saved), then MaxPool(GroupNorm(act(z))) in fp32 as k_groupnorm1 (csrc/ofp_nn.hip) evaluates it
__global__ __launch_bounds__(kT) void k_gn_fwd(const Ctl* ctl, const Norm t, const float* __restrict__ z,
                                               float* __restrict__ h, float* __restrict__ mean_out,
                                               float* __restrict__ rstd_out) {
    OFP_CNN_STOPPED(ctl);
    __shared__ double red[2][kT / 64];
    const int64_t item = blockIdx.x;
    const float* src = z + item * (int64_t)t.C * t.wc;
    const int count = t.C * t.wc;
    float mean = 0.0f, rstd = 1.0f;
    if (t.norm) {
        double s1 = 0.0, s2 = 0.0;
        for (int i = threadIdx.x; i < count; i += kT) {
            const double a = (double)ofp_activate(src[i], t.act);
            s1 += a;
            s2 += a * a;
        }
        block_sum2(s1, s2, red);
        const double m = s1 / (double)count;
        double var = s2 / (double)count - m * m;
        var = var > 0.0 ? var : 0.0;
        mean = (float)m;
        rstd = (float)(1.0 / sqrt(var + t.eps));
        if (threadIdx.x == 0) mean_out[item] = mean, rstd_out[item] = rstd;
    }
    float* dst = h + item * (int64_t)t.C * t.wo;
    for (int i = threadIdx.x; i < t.C * t.wo; i += kT) {
        const int k = i / t.wo, p = i - k * t.wo;
        const float g = t.norm ? t.ga[k] : 1.0f, b = t.norm ? t.be[k] : 0.0f;
        const float* zr = src + k * t.wc;
        if (t.pool) {
            const float y0 = gn_value(t, mean, rstd, g, b, zr[2 * p]);
            const float y1 = gn_value(t, mean, rstd, g, b, zr[2 * p + 1]);
            dst[i] = y1 > y0 ? y1 : y0;
        } else {
            dst[i] = gn_value(t, mean, rstd, g, b, zr[p]);
        }
    }
}

// d gamma[c] = sum dy * xhat, d beta[c] = sum dy over one slab of the (item, position) pairs of channel c
__global__ __launch_bounds__(kT) void k_gn_param_partial(const Ctl* ctl, const Norm t, int64_t items,
                                                         const float* __restrict__ z, const float* __restrict__ dh,
                                                         const float* __restrict__ mean, const float* __restrict__ rstd,
                                                         double* __restrict__ partial) {
    OFP_CNN_STOPPED(ctl);
    __shared__ double red[2][kT / 64];
    const int slab = blockIdx.x, c = blockIdx.y, nslab = gridDim.x;
    const int pairs = (int)items * t.wc, q0 = slab * kSlab;  // items * wc <= 2^22: 32-bit index arithmetic
    const int q1 = q0 + kSlab < pairs ? q0 + kSlab : pairs;
    const float g = t.ga[c], b = t.be[c];
    double s1 = 0.0, s2 = 0.0;
    for (int q = q0 + (int)threadIdx.x; q < q1; q += kT) {
        const int s = q / t.wc;
        const int p = q - s * t.wc;
        const float m = mean[s], r = rstd[s];
        const float* zr = z + ((int64_t)s * t.C + c) * t.wc;
        const float dy = gn_routed(t, m, r, g, b, zr, dh + ((int64_t)s * t.C + c) * t.wo, p);
        const float xh = (ofp_activate(zr[p], t.act) - m) * r;
        s1 += (double)dy;
        s2 += (double)dy * (double)xh;
    }
    block_sum2(s1, s2, red);
    if (threadIdx.x == 0) {
        partial[((int64_t)c * nslab + slab) * 2] = s1;
        partial[((int64_t)c * nslab + slab) * 2 + 1] = s2;
    }
}

__global__ __launch_bounds__(kT) void k_gn_param_final(const Ctl* ctl, const double* __restrict__ partial, int nslab,
                                                       int C, float* __restrict__ dgamma, float* __restrict__ dbeta) {
    OFP_CNN_STOPPED(ctl);
    const int c = blockIdx.x * kT + threadIdx.x;
    if (c >= C) return;
    double s1 = 0.0, s2 = 0.0;
    for (int i = 0; i < nslab; ++i) {
        s1 += partial[((int64_t)c * nslab + i) * 2];
        s2 += partial[((int64_t)c * nslab + i) * 2 + 1];
    }
    dbeta[c] = (float)s1, dgamma[c] = (float)s2;
}

// gradient at the pre-activation of one item per workgroup: pool routing, GroupNorm backward with dhat = dy * gamma,
// s1 = sum dhat, s2 = sum dhat * xhat over the item (fp64), dx = (dhat - s1 / N - xhat * s2 / N) * rstd, then the
// activation's derivative.  xhat is the forward's fp32 value; dx is evaluated in fp64 and rounded once: s1 / N and
// s2 / N are common to the item's N elements, dx sums to zero over the item, and a rounding of either would be all
// that is left of that sum in the bias gradient of the convolution in front
__global__ __launch_bounds__(kT) void k_gn_bwd(const Ctl* ctl, const Norm t, const float* __restrict__ z,
                                               const float* __restrict__ dh, const float* __restrict__ mean_in,
                                               const float* __restrict__ rstd_in, float* __restrict__ dz) {
    OFP_CNN_STOPPED(ctl);
    __shared__ double red[2][kT / 64];
    const int64_t item = blockIdx.x;
    const float* src = z + item * (int64_t)t.C * t.wc;
    const float* dsrc = dh + item * (int64_t)t.C * t.wo;
    float* dst = dz + item * (int64_t)t.C * t.wc;
    const int count = t.C * t.wc;
    float mean = 0.0f, rstd = 1.0f;
    double c1 = 0.0, c2 = 0.0;
    if (t.norm) {
        mean = mean_in[item], rstd = rstd_in[item];
        double s1 = 0.0, s2 = 0.0;
        for (int i = threadIdx.x; i < count; i += kT) {
            const int k = i / t.wc, p = i - k * t.wc;
            const float g = t.ga[k];
            const float* zr = src + k * t.wc;
            const double dhat = (double)gn_routed(t, mean, rstd, g, t.be[k], zr, dsrc + k * t.wo, p) * (double)g;
            const float xh = (ofp_activate(zr[p], t.act) - mean) * rstd;
            s1 += dhat;
            s2 += dhat * (double)xh;
        }
        block_sum2(s1, s2, red);
        c1 = s1 / (double)count, c2 = s2 / (double)count;
    }
    for (int i = threadIdx.x; i < count; i += kT) {
        const int k = i / t.wc, p = i - k * t.wc;
        const float* zr = src + k * t.wc;
        const float a = ofp_activate(zr[p], t.act);
        float d;
        if (t.norm) {
            const float g = t.ga[k];
            const double dhat = (double)gn_routed(t, mean, rstd, g, t.be[k], zr, dsrc + k * t.wo, p) * (double)g;
            const float xh = (a - mean) * rstd;
            d = (float)(((dhat - c1) - (double)xh * c2) * (double)rstd);
        } else {
            d = gn_routed(t, mean, rstd, 1.0f, 0.0f, zr, dsrc + k * t.wo, p);
        }
        dst[i] = d * act_grad(zr[p], a, t.act);
    }
}

// The correlation head of one (sample, sensor) item per workgroup, as k_autocorr_softmax (csrc/ofp_nn.hip) lays it out:
// cc[j] = sum_k sum_i f_k[i + j - (V - 1)] f_k[i], p = softmax(cc).  Unlike the inference kernel the K V products of
// a lag are added in fp64 (each is exact there) and cc stays in fp64 until the largest lag has been subtracted: the
// softmax turns an absolute error of cc into a relative error of p, cc[V-1] = sum f^2 is some tens after GroupNorm,
// and one fp32 rounding of it (let alone an fp32 chain of several hundred terms) is then the largest error of every
// gradient behind the head -- measured on train.py's own network, rounding cc alone accounts for 5e-9 of conv7.bias's
// gradient of 1e-2, every other fp32 value the head stores for at most 3e-10.  cc - max is small where p is not, so
// it is rounded to fp32 for expf.  The softmax's denominator is an fp64 sum as well: its error is common to all lags of the item, sum_j p[j] moves
// away from 1 by it, and the backward's lag weights g, which sum to zero, then no longer do -- the bias gradients of
// the conv stack are sums over df in which everything but that remainder cancels.  LDS: cc [L] fp64, maps.
__global__ __launch_bounds__(kT) void k_head_fwd(const Ctl* ctl, const float* __restrict__ x, int K, int V,
                                                 float* __restrict__ out) {
    OFP_CNN_STOPPED(ctl);
    extern __shared__ double smd[];
    __shared__ double dred[2][kT / 64];
    const int64_t item = blockIdx.x;
    const int L = 2 * V - 1;
    double* cc = smd;
    float* f = reinterpret_cast<float*>(smd + L);
    const float* src = x + item * (int64_t)K * V;
    for (int i = threadIdx.x; i < K * V; i += kT) f[i] = src[i];
    __syncthreads();
    for (int j = threadIdx.x; j < L; j += kT) {
        const int sh = j - (V - 1);
        const int lo = sh < 0 ? -sh : 0, hi = sh > 0 ? V - sh : V;
        double acc = 0.0;
        for (int k = 0; k < K; ++k) {
            const float* fk = f + k * V;
            for (int i = lo; i < hi; ++i) acc += (double)fk[i + sh] * (double)fk[i];
        }
        cc[j] = acc;
    }
    __syncthreads();
    double m = -INFINITY;
    for (int j = threadIdx.x; j < L; j += kT) m = fmax(m, cc[j]);
    for (int o = 32; o > 0; o >>= 1) m = fmax(m, __shfl_xor(m, o));
    if ((threadIdx.x & 63) == 0) dred[0][threadIdx.x >> 6] = m;
    __syncthreads();
    m = fmax(fmax(dred[0][0], dred[0][1]), fmax(dred[0][2], dred[0][3]));
    double ssum = 0.0, none = 0.0;
    for (int j = threadIdx.x; j < L; j += kT) {  // own elements only
        const float e = expf((float)(cc[j] - m));
        cc[j] = (double)e;
        ssum += (double)e;
    }
    block_sum2(ssum, none, dred);
    float* dst = out + item * (int64_t)L;
    for (int j = threadIdx.x; j < L; j += kT) dst[j] = (float)(cc[j] / ssum);
}

// Backward of the head for item (b, c) = (item / C, item % C): dp[j] = sum_o dout[b][o] Wfc[o][c L + j] (fmaf chain
// over o), dot = sum_j p[j] dp[j] (fp64, fixed order), dcc[j] = p[j] (dp[j] - dot) (the difference in fp64: dp and
// dot may nearly cancel), g[s] = dcc[V-1+s] + dcc[V-1-s], df_k[m] = sum_i g[i - m] f_k[i] (over i = 0 .. V-1 in
// fp64, rounded once; the lag 0 carries 2 dcc[V-1]).  LDS: maps [K V], dcc [L], g [L].  With kGiven the item's dp is
// read from `dpin` [items][L] instead (k_fc_bwd's d h, the same fmaf chain, after k_dropout_bwd has gone over it).
template <bool kGiven>
__global__ __launch_bounds__(kT) void k_head_bwd(const Ctl* ctl, const float* __restrict__ x,
                                                 const float* __restrict__ prob, const float* __restrict__ dout,
                                                 const float* __restrict__ wfc, int C, int K, int V, int O,
                                                 float* __restrict__ df, const float* __restrict__ dpin) {
    OFP_CNN_STOPPED(ctl);
    extern __shared__ float sm[];
    __shared__ double red[2][kT / 64];
    const int64_t item = blockIdx.x;
    const int64_t b = item / C;
    const int c = (int)(item - b * C);
    const int L = 2 * V - 1;
    float* f = sm;
    float* dcc = sm + (size_t)K * V;
    float* g = dcc + L;
    const float* src = x + item * (int64_t)K * V;
    const float* pr = prob + item * (int64_t)L;
    for (int i = threadIdx.x; i < K * V; i += kT) f[i] = src[i];
    double dot = 0.0, none = 0.0;
    for (int j = threadIdx.x; j < L; j += kT) {
        float dp = 0.0f;
        if (kGiven)
            dp = dpin[item * (int64_t)L + j];
        else
            for (int o = 0; o < O; ++o) dp = fmaf(dout[b * O + o], wfc[((int64_t)o * C + c) * L + j], dp);
        dcc[j] = dp;
        dot += (double)pr[j] * (double)dp;
    }
    block_sum2(dot, none, red);
    for (int j = threadIdx.x; j < L; j += kT) dcc[j] = (float)((double)pr[j] * ((double)dcc[j] - dot));  // own elements
    __syncthreads();
    for (int j = threadIdx.x; j < L; j += kT) g[j] = dcc[j] + dcc[L - 1 - j];
    __syncthreads();
    float* dst = df + item * (int64_t)K * V;
    for (int e = threadIdx.x; e < K * V; e += kT) {
        const int k = e / V, m = e - k * V;
        const float* fk = f + k * V;
        const float* gm = g + (V - 1 - m);
        double acc = 0.0;
        for (int i = 0; i < V; ++i) acc += (double)gm[i] * (double)fk[i];
        dst[e] = (float)acc;
    }
}

// torch.optim.SGD (momentum, weight decay, dampening 0, no Nesterov), one element per thread:
// g' = g + wd p, buf = g' on the first step and momentum buf + g' after it, p -= lr buf.  lr = rates[epoch].
__global__ __launch_bounds__(kT) void k_sgd(const Ctl* ctl, const float* __restrict__ rates, int first, float momentum,
                                            float wd, float* __restrict__ p, const float* __restrict__ g,
                                            float* __restrict__ buf, int64_t np) {
    OFP_CNN_STOPPED(ctl);
    const int e = ctl ? ctl->epoch : 0;
    if (ctl) first = e == 0;
    const float lr = rates[e];
    for (int64_t i = (int64_t)blockIdx.x * kT + threadIdx.x; i < np; i += (int64_t)gridDim.x * kT) {
        const float gr = g[i] + wd * p[i];
        const float bu = first ? gr : momentum * buf[i] + gr;
        buf[i] = bu;
        p[i] = p[i] - lr * bu;
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------

size_t head_lds(int K, int V) { return ((size_t)K * V + 2 * (size_t)(2 * V - 1) + 64) * sizeof(float); }

ofp::LdsAttrCache g_fwd_attr, g_bwd_attr, g_bwd_given_attr;

int check_conv(const char* who, int64_t n, int cin, int w, int cout, int k, int padding, int dilation, int groups,
               int stride) {
    OFP_REQUIRE(n >= 1 && n <= kMaxItems, "%s: %lld items (limit: 1..%d)", who, (long long)n, kMaxItems);
    OFP_REQUIRE(cin >= 1 && cin <= kMaxCh && cout >= 1 && cout <= kMaxCh, "%s: %d -> %d channels (limit: 1..%d)", who,
                cin, cout, kMaxCh);
    OFP_REQUIRE(w >= 1 && w <= 2 * kMaxWidth, "%s: width %d (limit: 1..%d)", who, w, 2 * kMaxWidth);
    OFP_REQUIRE(k >= 1 && k <= kMaxKernel, "%s: kernel size %d (limit: 1..%d)", who, k, kMaxKernel);
    OFP_REQUIRE(stride >= 1 && stride <= kMaxStride, "%s: stride %d (limit: 1..%d)", who, stride, kMaxStride);
    OFP_REQUIRE(dilation >= 1 && dilation <= 64 && padding >= 0 && padding <= kMaxWidth,
                "%s: dilation %d, padding %d", who, dilation, padding);
    OFP_REQUIRE(groups >= 1 && cin % groups == 0 && cout % groups == 0, "%s: groups %d do not divide %d and %d", who,
                groups, cin, cout);
    OFP_REQUIRE(w + 2 * padding - dilation * (k - 1) >= 1, "%s: the convolution leaves no output column", who);
    return OFP_OK;
}

struct Plan : WsPlan {
    int L, act, norm, pool, loss, O, C, K, V, F, group;
    double eps;
    float mom, wd;
    Conv conv[kMaxConv];
    int wo[kMaxConv];
    int w_off[kMaxConv], b_off[kMaxConv], g_off[kMaxConv], be_off[kMaxConv], fcw_off, fcb_off;
    // work space, byte offsets
    int64_t o_Z[kMaxConv], o_H[kMaxConv], o_stat[kMaxConv], o_P, o_out, o_dy, o_lpart, o_gh, o_gz, o_part, o_B, o_HD,
        o_DP;  // o_HD: the dropped p, o_DP: its gradient
    int64_t items(int64_t n) const { return group ? n : n * C; }
};

int make_plan(const char* who, const ofp_cccnn_config* c, int64_t n, int64_t n_val, Plan& p, const Random& rnd) {
    OFP_REQUIRE(c != nullptr, "%s: config is NULL", who);
    OFP_REQUIRE(c->n_conv >= 1 && c->n_conv <= kMaxConv, "%s: %d conv layers (limit: 1..%d)", who, c->n_conv, kMaxConv);
    OFP_REQUIRE(c->sensors >= 1 && c->sensors <= kMaxCh, "%s: %d sensor channels (limit: 1..%d)", who, c->sensors,
                kMaxCh);
    OFP_REQUIRE(n >= 1 && n <= kMaxBatch && n * c->sensors <= kMaxItems,
                "%s: batch of %lld with %d sensor channels (limits: 1..%d windows, %d (window, sensor) pairs)", who,
                (long long)n, c->sensors, kMaxBatch, kMaxItems);
    OFP_REQUIRE(n_val >= 0 && n_val <= kMaxBatch && n_val * c->sensors <= kMaxItems,
                "%s: validation batch of %lld (limits: 0..%d windows, %d (window, sensor) pairs)", who,
                (long long)n_val, kMaxBatch, kMaxItems);
    OFP_REQUIRE(c->width >= 1 && c->width <= kMaxWidth, "%s: window of %d samples (limit: 1..%d)", who, c->width,
                kMaxWidth);
    OFP_REQUIRE(c->act >= 0 && c->act <= OFP_ACT_TANH, "%s: unknown activation %d", who, c->act);
    OFP_REQUIRE(c->loss == 0 || c->loss == 1, "%s: loss %d (0 = L1, 1 = MSE)", who, c->loss);
    OFP_REQUIRE(c->n_out >= 1 && c->n_out <= kMaxOut, "%s: %d outputs (limit: 1..%d)", who, c->n_out, kMaxOut);
    OFP_REQUIRE(!c->norm || c->gn_eps > 0.0, "%s: GroupNorm eps %g", who, c->gn_eps);
    OFP_REQUIRE(c->momentum >= 0.0f && c->momentum < 1.0f && c->weight_decay >= 0.0f,
                "%s: momentum %g, weight decay %g", who, (double)c->momentum, (double)c->weight_decay);
    p = Plan{};
    p.L = c->n_conv, p.act = c->act, p.norm = c->norm ? 1 : 0, p.pool = c->pool ? 1 : 0, p.loss = c->loss;
    p.O = c->n_out, p.C = c->sensors, p.group = c->group ? 1 : 0, p.eps = c->gn_eps;
    p.mom = c->momentum, p.wd = c->weight_decay;
    const int mult = p.group ? p.C : 1, groups = mult;
    const int64_t nmax = n > n_val ? n : n_val;
    const int64_t it = p.items(n), itmax = p.items(nmax);
    int width = c->width, np = 0, cin = mult;
    int64_t max_h = 0, max_z = 0, max_part = 2;
    for (int l = 0; l < p.L; ++l) {
        OFP_REQUIRE(c->layer_sizes[l] >= 1 && (int64_t)c->layer_sizes[l] * mult <= kMaxCh,
                    "%s: layer %d has %d channels%s (limit: 1..%d)", who, l + 1, c->layer_sizes[l],
                    p.group ? " per sensor" : "", kMaxCh / mult);
        const int cout = c->layer_sizes[l] * mult;
        if (int rc = check_conv(who, it, cin, width, cout, c->kernels[l], c->padding, c->dilation, groups,
                                c->strides[l]))
            return rc;
        Conv& v = p.conv[l];
        v = Conv{cin, cout, width, conv_width(width, c->kernels[l], c->padding, c->dilation, c->strides[l]),
                 c->kernels[l], c->padding, c->dilation, groups, c->strides[l]};
        OFP_REQUIRE(v.wc <= 2 * kMaxWidth, "%s: layer %d is %d wide (limit: %d)", who, l + 1, v.wc, 2 * kMaxWidth);
        p.wo[l] = p.pool ? v.wc / 2 : v.wc;
        OFP_REQUIRE(p.wo[l] >= 1, "%s: the pool of layer %d leaves no output column", who, l + 1);
        const int T = cin / groups * v.k + 1;
        p.w_off[l] = np, np += cout * (T - 1);
        p.b_off[l] = np, np += cout;
        if (p.norm) {
            p.g_off[l] = np, np += cout;
            p.be_off[l] = np, np += cout;
        }
        const int64_t part = (int64_t)cout * T * slabs_of(it * v.wc);
        max_part = part > max_part ? part : max_part;
        max_h = std::max<int64_t>(max_h, itmax * cout * p.wo[l]);
        max_z = std::max<int64_t>(max_z, itmax * cout * v.wc);
        width = p.wo[l];
        cin = cout;
    }
    p.K = c->layer_sizes[p.L - 1], p.V = width;
    OFP_REQUIRE(head_lds(p.K, p.V) <= kMaxLds, "%s: the head's %d maps of %d columns do not fit the LDS (%d bytes)", who,
                p.K, p.V, (int)kMaxLds);
    p.F = p.C * (2 * p.V - 1);
    max_part = std::max<int64_t>(max_part, (int64_t)fc_chunks(n) * p.O * p.F);
    max_h = std::max<int64_t>(max_h, nmax * p.F);
    p.fcw_off = np, np += p.O * p.F;
    p.fcb_off = np, np += p.O;
    p.np = np;
    for (int l = 0; l < p.L; ++l) {
        p.o_Z[l] = p.take(itmax * p.conv[l].cout * p.conv[l].wc * 4);
        p.o_H[l] = p.take(itmax * p.conv[l].cout * p.wo[l] * 4);
        p.o_stat[l] = p.take(itmax * 2 * 4);
    }
    p.o_P = p.take(nmax * p.F * 4);
    p.o_out = p.take(nmax * p.O * 4);
    p.o_dy = p.take(nmax * p.O * 4);
    p.o_lpart = p.take(nmax * 8);
    p.o_gh = p.take(max_h * 4);
    p.o_gz = p.take(max_z * 4);
    p.o_part = p.take(max_part * 8);
    p.o_G = p.take((int64_t)np * 4);
    p.o_B = p.take((int64_t)np * 4);
    p.o_ctl = p.take(sizeof(Ctl));
    if (rnd.drop) p.o_HD = p.take(n * p.F * 4), p.o_DP = p.take(n * p.F * 4);
    if (rnd.windows) p.o_X = p.take(n * p.C * c->width * 4);
    return OFP_OK;
}

Norm norm_of(const Run<Plan>& r, int l) {
    const Plan& p = *r.p;
    Norm t{};
    t.C = p.conv[l].cout, t.wc = p.conv[l].wc, t.wo = p.wo[l], t.act = p.act, t.pool = p.pool, t.norm = p.norm;
    t.eps = p.eps;
    if (p.norm) t.ga = r.P + p.g_off[l], t.be = r.P + p.be_off[l];
    return t;
}

int enqueue_conv_fwd(const Ctl* ctl, const Conv& c, int64_t n, const float* x, const float* w, const float* b,
                     float* z, hipStream_t st) {
    hipLaunchKernelGGL(k_conv_fwd, dim3(grid_for(n * c.cout * c.wc)), dim3(kT), 0, st, ctl, c, n, x, w, b, z);
    OFP_LAUNCH_CHECK("k_conv_fwd");
    return OFP_OK;
}

int enqueue_gn_fwd(const Ctl* ctl, const Norm& t, int64_t items, const float* z, float* h, float* mean, float* rstd,
                   hipStream_t st) {
    hipLaunchKernelGGL(k_gn_fwd, dim3((unsigned)items), dim3(kT), 0, st, ctl, t, z, h, mean, rstd);
    OFP_LAUNCH_CHECK("k_gn_fwd");
    return OFP_OK;
}

// dh -> dz (and d gamma, d beta when the layer has a GroupNorm)
int enqueue_gn_bwd(const Ctl* ctl, const Norm& t, int64_t items, const float* z, const float* dh, const float* mean,
                   const float* rstd, double* part, float* dgamma, float* dbeta, float* dz, hipStream_t st) {
    if (t.norm) {
        const int nslab = slabs_of(items * t.wc);
        hipLaunchKernelGGL(k_gn_param_partial, dim3(nslab, t.C), dim3(kT), 0, st, ctl, t, items, z, dh, mean, rstd,
                           part);
        OFP_LAUNCH_CHECK("k_gn_param_partial");
        hipLaunchKernelGGL(k_gn_param_final, dim3((unsigned)ofp::cdiv(t.C, kT)), dim3(kT), 0, st, ctl, part, nslab,
                           t.C, dgamma, dbeta);
        OFP_LAUNCH_CHECK("k_gn_param_final");
    }
    hipLaunchKernelGGL(k_gn_bwd, dim3((unsigned)items), dim3(kT), 0, st, ctl, t, z, dh, mean, rstd, dz);
    OFP_LAUNCH_CHECK("k_gn_bwd");
    return OFP_OK;
}

int enqueue_head_fwd(const Ctl* ctl, const float* f, int64_t items, int K, int V, float* prob, hipStream_t st) {
    const size_t lds = head_lds(K, V);
    if (int rc = ofp::ensure_dynamic_lds(reinterpret_cast<const void*>(k_head_fwd), lds, g_fwd_attr)) return rc;
    hipLaunchKernelGGL(k_head_fwd, dim3((unsigned)items), dim3(kT), lds, st, ctl, f, K, V, prob);
    OFP_LAUNCH_CHECK("k_head_fwd");
    return OFP_OK;
}

int enqueue_head_bwd(const Ctl* ctl, const float* f, const float* prob, const float* dout, const float* wfc,
                     int64_t items, int C, int K, int V, int O, float* df, hipStream_t st,
                     const float* dpin = nullptr) {
    const size_t lds = head_lds(K, V);
    if (dpin != nullptr) {
        if (int rc = ofp::ensure_dynamic_lds(reinterpret_cast<const void*>(k_head_bwd<true>), lds, g_bwd_given_attr))
            return rc;
        hipLaunchKernelGGL(k_head_bwd<true>, dim3((unsigned)items), dim3(kT), lds, st, ctl, f, prob, dout, wfc, C, K,
                           V, O, df, dpin);
    } else {
        if (int rc = ofp::ensure_dynamic_lds(reinterpret_cast<const void*>(k_head_bwd<false>), lds, g_bwd_attr))
            return rc;
        hipLaunchKernelGGL(k_head_bwd<false>, dim3((unsigned)items), dim3(kT), lds, st, ctl, f, prob, dout, wfc, C, K,
                           V, O, df, dpin);
    }
    OFP_LAUNCH_CHECK("k_head_bwd");
    return OFP_OK;
}

Fc fc_of(const Run<Plan>& r, const float* h, int64_t n, const float* y) {
    const Plan& p = *r.p;
    return Fc{h, n, p.F, p.O, r.P + p.fcw_off, r.P + p.fcb_off, y};
}

// conv stack, correlation head and Linear of a batch, its mean loss into `curve`; train: model.loss, d loss / d out
// kept and the Linear's bias gradient; else L1 and the early-stop rule
int enqueue_forward(const Run<Plan>& r, const float* x, const float* y, int64_t n, bool train, float* curve, int patience) {
    const Plan& p = *r.p;
    const int64_t items = p.items(n);
    const float* in = x;
    for (int l = 0; l < p.L; ++l) {
        float* Z = r.at<float>(p.o_Z[l]);
        float* H = r.at<float>(p.o_H[l]);
        float* stat = r.at<float>(p.o_stat[l]);
        if (int rc = enqueue_conv_fwd(r.ctl, p.conv[l], items, in, r.P + p.w_off[l], r.P + p.b_off[l], Z, r.st))
            return rc;
        if (int rc = enqueue_gn_fwd(r.ctl, norm_of(r, l), items, Z, H, stat, stat + items, r.st)) return rc;
        in = H;
    }
    float* prob = r.at<float>(p.o_P);
    if (int rc = enqueue_head_fwd(r.ctl, in, n * p.C, p.K, p.V, prob, r.st)) return rc;
    const float* feat = prob;  // k_head_bwd needs the undropped p: the dropped copy has a buffer of its own
    if (train && r.rnd.drop) {
        if (int rc = enqueue_dropout_fwd(r.ctl, r.rnd, prob, r.at<float>(p.o_HD), n * p.F, r.st)) return rc;
        feat = r.at<float>(p.o_HD);
    }
    return enqueue_fc_forward(r.ctl, fc_of(r, feat, n, y), p.loss, r.at<float>(p.o_out),
                              train ? r.at<float>(p.o_dy) : nullptr, r.at<double>(p.o_lpart), curve, patience,
                              r.G + p.fcb_off, r.st);
}

int enqueue_backward(const Run<Plan>& r, const float* x, int64_t n) {
    const Plan& p = *r.p;
    const int64_t items = p.items(n);
    float* GH = r.at<float>(p.o_gh);
    float* GZ = r.at<float>(p.o_gz);
    double* part = r.at<double>(p.o_part);
    // the Linear head's weight gradient; the d p it also writes is not used (k_head_bwd forms its own, per item)
    // unless there is a dropout: then it is masked in place and k_head_bwd takes it
    float* DP = r.rnd.drop ? r.at<float>(p.o_DP) : nullptr;
    if (int rc = enqueue_fc_backward(r.ctl, fc_of(r, r.at<float>(r.rnd.drop ? p.o_HD : p.o_P), n, nullptr),
                                     r.at<float>(p.o_dy), part, r.G + p.fcw_off, DP ? DP : GH, r.st))
        return rc;
    if (DP)
        if (int rc = enqueue_dropout_bwd(r.ctl, r.rnd, DP, n * p.F, r.st)) return rc;
    if (int rc = enqueue_head_bwd(r.ctl, r.at<float>(p.o_H[p.L - 1]), r.at<float>(p.o_P), r.at<float>(p.o_dy),
                                  r.P + p.fcw_off, n * p.C, p.C, p.K, p.V, p.O, GH, r.st, DP))
        return rc;
    for (int l = p.L - 1; l >= 0; --l) {
        const float* Z = r.at<float>(p.o_Z[l]);
        const float* stat = r.at<float>(p.o_stat[l]);
        if (int rc = enqueue_gn_bwd(r.ctl, norm_of(r, l), items, Z, GH, stat, stat + items, part, r.G + p.g_off[l],
                                    r.G + p.be_off[l], GZ, r.st))
            return rc;
        const float* in = l == 0 ? x : r.at<float>(p.o_H[l - 1]);
        if (int rc = enqueue_conv_bwd(r.ctl, p.conv[l], items, in, r.P + p.w_off[l], GZ, part, r.G + p.w_off[l],
                                      r.G + p.b_off[l], l == 0 ? nullptr : GH, r.st))
            return rc;
    }
    return OFP_OK;
}

int enqueue_step(const Run<Plan>& r, const float* rates) {
    const Plan& p = *r.p;
    hipLaunchKernelGGL(k_sgd, dim3(grid_for(p.np)), dim3(kT), 0, r.st, r.ctl, rates, 0, p.mom, p.wd, r.P, r.G,
                       r.at<float>(p.o_B), (int64_t)p.np);
    OFP_LAUNCH_CHECK("k_sgd");
    return OFP_OK;
}

int enqueue_reset(const Run<Plan>& r) {
    OFP_HIP(hipMemsetAsync(r.at<float>(r.p->o_B), 0, (size_t)r.p->np * 4, r.st));
    return OFP_OK;
}

struct Cccnn {
    using Config = ofp_cccnn_config;
    using Plan = ::Plan;
    static constexpr const char* train = "ofp_cccnn_train";
    static constexpr const char* grads = "ofp_cccnn_loss_grads";
    static constexpr const char* env = "OFP_CCCNN_GRAPH";
    static Window window_of(const Config& c) { return Window{c.sensors, c.width}; }
    static constexpr auto make_plan = ::make_plan;
};

}  // namespace

extern "C" {

int64_t ofp_cccnn_train_workspace_bytes(const ofp_cccnn_config* cfg, int64_t n, int64_t n_val) {
    return ofp_cccnn_train_random_workspace_bytes(cfg, n, n_val, nullptr);
}

int64_t ofp_cccnn_train_random_workspace_bytes(const ofp_cccnn_config* cfg, int64_t n, int64_t n_val,
                                               const ofp_train_random* random) {
    return ofp_cccnn_train_stretch_workspace_bytes(cfg, n, n_val, random, 0);
}

int64_t ofp_cccnn_train_stretch_workspace_bytes(const ofp_cccnn_config* cfg, int64_t n, int64_t n_val,
                                                const ofp_train_random* random, int32_t stretch_span) {
    return train_workspace_bytes<Cccnn>(cfg, n, n_val, random, stretch_span);
}

int ofp_cccnn_train(const ofp_cccnn_config* cfg, int64_t n, const float* d_x, const float* d_y, int64_t n_val,
                    const float* d_x_val, const float* d_y_val, const float* d_rates, int32_t num_epochs,
                    int32_t min_epochs, int32_t patience, float* d_params, float* d_train_loss, float* d_val_loss,
                    int32_t* h_epochs, void* d_ws, int64_t ws_bytes, void* stream) {
    return ofp_cccnn_train_random(cfg, n, d_x, d_y, n_val, d_x_val, d_y_val, d_rates, num_epochs, min_epochs,
                                  patience, d_params, d_train_loss, d_val_loss, h_epochs, d_ws, ws_bytes, stream,
                                  nullptr);
}

int ofp_cccnn_train_random(const ofp_cccnn_config* cfg, int64_t n, const float* d_x, const float* d_y, int64_t n_val,
                           const float* d_x_val, const float* d_y_val, const float* d_rates, int32_t num_epochs,
                           int32_t min_epochs, int32_t patience, float* d_params, float* d_train_loss,
                           float* d_val_loss, int32_t* h_epochs, void* d_ws, int64_t ws_bytes, void* stream,
                           const ofp_train_random* random) {
    return ofp_cccnn_train_stretch(cfg, n, d_x, d_y, n_val, d_x_val, d_y_val, d_rates, num_epochs, min_epochs,
                                   patience, d_params, d_train_loss, d_val_loss, h_epochs, d_ws, ws_bytes, stream,
                                   random, 0);
}

int ofp_cccnn_train_stretch(const ofp_cccnn_config* cfg, int64_t n, const float* d_x, const float* d_y, int64_t n_val,
                            const float* d_x_val, const float* d_y_val, const float* d_rates, int32_t num_epochs,
                            int32_t min_epochs, int32_t patience, float* d_params, float* d_train_loss,
                            float* d_val_loss, int32_t* h_epochs, void* d_ws, int64_t ws_bytes, void* stream,
                            const ofp_train_random* random, int32_t stretch_span) {
    return train_entry<Cccnn>(cfg, n, d_x, d_y, n_val, d_x_val, d_y_val, d_rates, num_epochs, min_epochs, patience,
                              d_params, nullptr, d_train_loss, d_val_loss, h_epochs, d_ws, ws_bytes, stream, random,
                              stretch_span);
}

int ofp_cccnn_loss_grads(const ofp_cccnn_config* cfg, int64_t n, const float* d_x, const float* d_y,
                         const float* d_params, float* d_loss, float* d_grads, void* d_ws, int64_t ws_bytes,
                         void* stream) {
    return ofp_cccnn_loss_grads_random(cfg, n, d_x, d_y, d_params, d_loss, d_grads, d_ws, ws_bytes, stream, nullptr);
}

int ofp_cccnn_loss_grads_random(const ofp_cccnn_config* cfg, int64_t n, const float* d_x, const float* d_y,
                                const float* d_params, float* d_loss, float* d_grads, void* d_ws, int64_t ws_bytes,
                                void* stream, const ofp_train_random* random) {
    return loss_grads_entry<Cccnn>(cfg, n, d_x, d_y, d_params, d_loss, d_grads, d_ws, ws_bytes, stream, random);
}

int64_t ofp_conv1d_backward_strided_workspace_bytes(int64_t n, int32_t cin, int32_t w, int32_t cout, int32_t k,
                                                    int32_t padding, int32_t dilation, int32_t groups,
                                                    int32_t stride) {
    if (check_conv("ofp_conv1d_backward_strided", n, cin, w, cout, k, padding, dilation, groups, stride)) return -1;
    return conv_bwd_bytes(n, cin, w, cout, k, padding, dilation, groups, stride);
}

int ofp_conv1d_backward_strided(const float* d_x, int64_t n, int32_t cin, int32_t w, const float* d_w, int32_t cout,
                                int32_t k, int32_t padding, int32_t dilation, int32_t groups, int32_t stride,
                                const float* d_dz, float* d_dx, float* d_dw, float* d_db, void* d_ws, int64_t ws_bytes,
                                void* stream) {
    return conv_bwd_alone(
        "ofp_conv1d_backward_strided",
        ofp_conv1d_backward_strided_workspace_bytes(n, cin, w, cout, k, padding, dilation, groups, stride), d_x, n, cin,
        w, d_w, cout, k, padding, dilation, groups, stride, d_dz, d_dx, d_dw, d_db, d_ws, ws_bytes, stream);
}

int64_t ofp_groupnorm1_train_workspace_bytes(int64_t n, int32_t K, int32_t V) {
    if (n < 1 || n > kMaxItems || K < 1 || K > kMaxCh || V < 1 || V > 2 * kMaxWidth) return -1;
    return (int64_t)K * slabs_of(n * V) * 2 * 8;
}

namespace {
int check_gn(const char* who, int64_t n, int32_t K, int32_t V, int32_t pool) {
    OFP_REQUIRE(ofp_groupnorm1_train_workspace_bytes(n, K, V) >= 0,
                "%s: %lld items, %d channels, width %d (limits: 1..%d, 1..%d, 1..%d)", who, (long long)n, K, V,
                kMaxItems, kMaxCh, 2 * kMaxWidth);
    OFP_REQUIRE(!pool || V >= 2, "%s: nothing left after pooling", who);
    return OFP_OK;
}
Norm gn_of(int32_t K, int32_t V, int32_t pool, double eps, const float* gamma, const float* beta) {
    Norm t{};
    t.C = K, t.wc = V, t.wo = pool ? V / 2 : V, t.act = OFP_ACT_IDENTITY, t.pool = pool ? 1 : 0, t.norm = 1;
    t.eps = eps, t.ga = gamma, t.be = beta;
    return t;
}
}  // namespace

int ofp_groupnorm1_train_forward(const float* d_x, int64_t n, int32_t K, int32_t V, const float* d_gamma,
                                 const float* d_beta, double eps, int32_t pool, float* d_y, float* d_mean,
                                 float* d_rstd, void* stream) {
    if (int rc = check_gn("ofp_groupnorm1_train_forward", n, K, V, pool)) return rc;
    OFP_REQUIRE(d_x && d_gamma && d_beta && d_y && d_mean && d_rstd && eps > 0.0,
                "ofp_groupnorm1_train_forward: NULL argument or eps <= 0");
    return enqueue_gn_fwd(nullptr, gn_of(K, V, pool, eps, d_gamma, d_beta), n, d_x, d_y, d_mean, d_rstd,
                          (hipStream_t)stream);
}

int ofp_groupnorm1_train_backward(const float* d_x, int64_t n, int32_t K, int32_t V, const float* d_gamma,
                                  const float* d_beta, const float* d_mean, const float* d_rstd, int32_t pool,
                                  const float* d_dy, float* d_dx, float* d_dgamma, float* d_dbeta, void* d_ws,
                                  int64_t ws_bytes, void* stream) {
    if (int rc = check_gn("ofp_groupnorm1_train_backward", n, K, V, pool)) return rc;
    OFP_REQUIRE(d_x && d_gamma && d_beta && d_mean && d_rstd && d_dy && d_dx && d_dgamma && d_dbeta,
                "ofp_groupnorm1_train_backward: NULL argument");
    if (int rc = check_ws("ofp_groupnorm1_train_backward", d_ws, ws_bytes,
                          ofp_groupnorm1_train_workspace_bytes(n, K, V)))
        return rc;
    return enqueue_gn_bwd(nullptr, gn_of(K, V, pool, 1.0, d_gamma, d_beta), n, d_x, d_dy, d_mean, d_rstd,
                          (double*)d_ws, d_dgamma, d_dbeta, d_dx, (hipStream_t)stream);
}

int64_t ofp_autocorr_softmax_lds_bytes(int32_t K, int32_t V) {
    if (K < 1 || V < 1) return -1;
    return (int64_t)head_lds(K, V);
}

int ofp_autocorr_softmax_backward(const float* d_f, const float* d_p, const float* d_dout, const float* d_wfc,
                                  int64_t items, int32_t C, int32_t K, int32_t V, int32_t O, float* d_df,
                                  void* stream) {
    OFP_REQUIRE(d_f && d_p && d_dout && d_wfc && d_df, "ofp_autocorr_softmax_backward: NULL argument");
    OFP_REQUIRE(C >= 1 && K >= 1 && V >= 1 && O >= 1 && O <= kMaxOut && items >= 1 && items <= kMaxItems &&
                    items % C == 0,
                "ofp_autocorr_softmax_backward: %lld items of %d sensors, %d maps of %d columns, %d outputs (limits: "
                "items 1..%d and a multiple of the sensors, outputs 1..%d)",
                (long long)items, C, K, V, O, kMaxItems, kMaxOut);
    OFP_REQUIRE(head_lds(K, V) <= kMaxLds, "ofp_autocorr_softmax_backward: K*V = %d floats do not fit the LDS", K * V);
    return enqueue_head_bwd(nullptr, d_f, d_p, d_dout, d_wfc, items, C, K, V, O, d_df, (hipStream_t)stream);
}

int ofp_sgd_step(float* d_p, const float* d_g, float* d_buf, int64_t n, const float* d_lr, int32_t first,
                 float momentum, float weight_decay, void* stream) {
    OFP_REQUIRE(d_p && d_g && d_buf && d_lr && n >= 1, "ofp_sgd_step: NULL argument or n < 1");
    hipLaunchKernelGGL(k_sgd, dim3(grid_for(n)), dim3(kT), 0, (hipStream_t)stream, (const Ctl*)nullptr, d_lr,
                       first ? 1 : 0, momentum, weight_decay, d_p, d_g, d_buf, n);
    OFP_LAUNCH_CHECK("k_sgd");
    return OFP_OK;
}

}  // extern "C"
