// The conv stack of model.CNN as both of its trainers run it (csrc/ofp_cnn_train.hip, csrc/ofp_cnnrnn_train.hip): what
// follows a convolution (activation, BatchNorm1d on batch or running statistics, MaxPool1d(2, 2)) forward and backward,
// the NAdam step, the limits of the stack and the launch helpers of the BatchNorm reductions; and the stack as a part of
// a trainer's Plan (ofp_train_chain.h): ConvStack with plan_conv_stack, which makes the checks and takes the blocks,
// post_of, enqueue_conv_stack_fwd and enqueue_conv_stack_bwd.  A trainer keeps what is behind the stack's features.
// File-local like ofp_train_chain.h and ofp_train_random.h, which it builds on: each trainer compiles its own copy.
#pragma once
#include "ofp_train_random.h"

#include <algorithm>

namespace {

constexpr int kMaxConv = 3;
constexpr int kMaxCh = 128;
constexpr int kMaxKernel = 8;
constexpr int kMaxWidth = 512;
constexpr int kMaxBatch = 1024;

// what follows the convolution: activation, BatchNorm (mode 0 none, 1 batch statistics, 2 running statistics), pool
struct Post {
    int C, wc, wo, act, pool, mode;
    double eps;
    const float* ga;
    const float* be;
    const float* mean;  // mode 1: saved batch mean; mode 2: running mean
    const float* rs;    // mode 1: saved 1 / sqrt(var + eps); mode 2: running variance
};

struct Aff {
    float mean, rstd, ga, be;
};

__device__ __forceinline__ Aff load_aff(const Post& t, int c) {
    Aff f{0.0f, 1.0f, 1.0f, 0.0f};
    if (t.mode == 1) {
        f.mean = t.mean[c], f.rstd = t.rs[c], f.ga = t.ga[c], f.be = t.be[c];
    } else if (t.mode == 2) {  // the fold of model.conv1d_forward, in double, rounded once
        const double inv = 1.0 / sqrt((double)t.rs[c] + t.eps);
        const double g = (double)t.ga[c];
        f.ga = (float)(g * inv);
        f.be = (float)((double)t.be[c] - (double)t.mean[c] * g * inv);
    }
    return f;
}

__device__ __forceinline__ float aff_apply(const Aff& f, int mode, float a) {
    if (mode == 1) return ((a - f.mean) * f.rstd) * f.ga + f.be;
    if (mode == 2) return fmaf(a, f.ga, f.be);
    return a;
}

// BatchNorm, batch statistics: sum a, sum a^2 (a = act(z)) of one slab of one channel
__global__ __launch_bounds__(kT) void k_bn_stats_partial(const Ctl* ctl, const float* __restrict__ z, int64_t n, int C,
                                                         int wc, int act, double* __restrict__ partial) {
    OFP_CNN_STOPPED(ctl);
    __shared__ double red[2][kT / 64];
    const int slab = blockIdx.x, c = blockIdx.y, nslab = gridDim.x;
    const int pairs = (int)n * wc, q0 = slab * kSlab;  // n * wc <= 2^20: 32-bit index arithmetic
    const int q1 = q0 + kSlab < pairs ? q0 + kSlab : pairs;
    double s1 = 0.0, s2 = 0.0;
    for (int q = q0 + (int)threadIdx.x; q < q1; q += kT) {
        const int s = q / wc;
        const int p = q - s * wc;
        const double a = (double)ofp_activate(z[((int64_t)s * C + c) * wc + p], act);
        s1 += a;
        s2 += a * a;
    }
    block_sum2(s1, s2, red);
    if (threadIdx.x == 0) {
        partial[((int64_t)c * nslab + slab) * 2] = s1;
        partial[((int64_t)c * nslab + slab) * 2 + 1] = s2;
    }
}

// slabs in slab order -> mean, 1 / sqrt(biased var + eps); running statistics with the unbiased variance
__global__ __launch_bounds__(kT) void k_bn_stats_final(const Ctl* ctl, const double* __restrict__ partial, int nslab,
                                                       int C, int64_t count, double eps, float mom,
                                                       float* __restrict__ mean, float* __restrict__ rstd,
                                                       float* __restrict__ run_mean, float* __restrict__ run_var) {
    OFP_CNN_STOPPED(ctl);
    const int c = blockIdx.x * kT + threadIdx.x;
    if (c >= C) return;
    double s1 = 0.0, s2 = 0.0;
    for (int i = 0; i < nslab; ++i) {
        s1 += partial[((int64_t)c * nslab + i) * 2];
        s2 += partial[((int64_t)c * nslab + i) * 2 + 1];
    }
    const double m = s1 / (double)count;
    double var = s2 / (double)count - m * m;
    var = var > 0.0 ? var : 0.0;
    mean[c] = (float)m;
    rstd[c] = (float)(1.0 / sqrt(var + eps));
    const float unbiased = (float)(var * ((double)count / (double)(count - 1)));
    run_mean[c] = mom * (float)m + (1.0f - mom) * run_mean[c];
    run_var[c] = mom * unbiased + (1.0f - mom) * run_var[c];
}

// the layer's output: MaxPool(BatchNorm(act(z)))
__global__ __launch_bounds__(kT) void k_post(const Ctl* ctl, const Post t, int64_t n, const float* __restrict__ z,
                                             float* __restrict__ h) {
    OFP_CNN_STOPPED(ctl);
    const int64_t total = n * t.C * t.wo;
    for (int64_t i = (int64_t)blockIdx.x * kT + threadIdx.x; i < total; i += (int64_t)gridDim.x * kT) {
        const int po = (int)(i % t.wo);
        const int64_t row = i / t.wo;
        const int c = (int)(row % t.C);
        const Aff f = load_aff(t, c);
        const float* zr = z + row * t.wc;
        if (t.pool) {
            const float y0 = aff_apply(f, t.mode, ofp_activate(zr[2 * po], t.act));
            const float y1 = aff_apply(f, t.mode, ofp_activate(zr[2 * po + 1], t.act));
            h[i] = y1 > y0 ? y1 : y0;
        } else {
            h[i] = aff_apply(f, t.mode, ofp_activate(zr[po], t.act));
        }
    }
}

// gradient that reaches position p of the un-pooled row: the pool hands its gradient to the larger of the pair
// (the first on a tie); a dropped odd last column gets none
__device__ __forceinline__ float routed_dy(const Post& t, const Aff& f, const float* zr, const float* dhr, int p) {
    if (!t.pool) return dhr[p];
    const int po = p >> 1;
    if (po >= t.wo) return 0.0f;
    const float y0 = aff_apply(f, t.mode, ofp_activate(zr[2 * po], t.act));
    const float y1 = aff_apply(f, t.mode, ofp_activate(zr[2 * po + 1], t.act));
    const bool second = y1 > y0;
    return ((p & 1) != 0) == second ? dhr[po] : 0.0f;
}

// BatchNorm backward: sum dy, sum dy * xhat of one slab of one channel
__global__ __launch_bounds__(kT) void k_bn_bwd_partial(const Ctl* ctl, const Post t, int64_t n,
                                                       const float* __restrict__ z, const float* __restrict__ dh,
                                                       double* __restrict__ partial) {
    OFP_CNN_STOPPED(ctl);
    __shared__ double red[2][kT / 64];
    const int slab = blockIdx.x, c = blockIdx.y, nslab = gridDim.x;
    const int pairs = (int)n * t.wc, q0 = slab * kSlab;
    const int q1 = q0 + kSlab < pairs ? q0 + kSlab : pairs;
    const Aff f = load_aff(t, c);
    double s1 = 0.0, s2 = 0.0;
    for (int q = q0 + (int)threadIdx.x; q < q1; q += kT) {
        const int s = q / t.wc;
        const int p = q - s * t.wc;
        const float* zr = z + ((int64_t)s * t.C + c) * t.wc;
        const float dy = routed_dy(t, f, zr, dh + ((int64_t)s * t.C + c) * t.wo, p);
        const float xh = (ofp_activate(zr[p], t.act) - f.mean) * f.rstd;
        s1 += (double)dy;
        s2 += (double)dy * (double)xh;
    }
    block_sum2(s1, s2, red);
    if (threadIdx.x == 0) {
        partial[((int64_t)c * nslab + slab) * 2] = s1;
        partial[((int64_t)c * nslab + slab) * 2 + 1] = s2;
    }
}

__global__ __launch_bounds__(kT) void k_bn_bwd_final(const Ctl* ctl, const double* __restrict__ partial, int nslab,
                                                     int C, float* __restrict__ s12, float* __restrict__ dgamma,
                                                     float* __restrict__ dbeta) {
    OFP_CNN_STOPPED(ctl);
    const int c = blockIdx.x * kT + threadIdx.x;
    if (c >= C) return;
    double s1 = 0.0, s2 = 0.0;
    for (int i = 0; i < nslab; ++i) {
        s1 += partial[((int64_t)c * nslab + i) * 2];
        s2 += partial[((int64_t)c * nslab + i) * 2 + 1];
    }
    s12[c] = (float)s1, s12[C + c] = (float)s2;
    dbeta[c] = (float)s1, dgamma[c] = (float)s2;
}

// gradient at the pre-activation: pool routing, BatchNorm backward (needs the two sums), activation backward
__global__ __launch_bounds__(kT) void k_dz(const Ctl* ctl, const Post t, int64_t n, const float* __restrict__ z,
                                           const float* __restrict__ dh, const float* __restrict__ s12,
                                           float* __restrict__ dz) {
    OFP_CNN_STOPPED(ctl);
    const int64_t total = n * t.C * t.wc;
    const float inv_count = 1.0f / (float)(n * t.wc);
    for (int64_t i = (int64_t)blockIdx.x * kT + threadIdx.x; i < total; i += (int64_t)gridDim.x * kT) {
        const int p = (int)(i % t.wc);
        const int64_t row = i / t.wc;
        const int c = (int)(row % t.C);
        const Aff f = load_aff(t, c);
        const float* zr = z + row * t.wc;
        float d = routed_dy(t, f, zr, dh + row * t.wo, p);
        const float a = ofp_activate(zr[p], t.act);
        if (t.mode == 1) {
            const float xh = (a - f.mean) * f.rstd;
            d = (d - s12[c] * inv_count - xh * (s12[t.C + c] * inv_count)) * f.rstd * f.ga;
        }
        dz[i] = d * act_grad(zr[p], a, t.act);
    }
}

// torch.optim.NAdam (_single_tensor_nadam, defaults: betas 0.9 / 0.999, eps 1e-8, no weight decay), one element per
// thread.  row = (c1, c2, bias_correction2), denom = sqrt(v / bias_correction2) + eps, p += (c1 g + c2 m) / denom.
// torch adds the two terms to p one after the other (two addcdiv_ calls, p rounded twice); here they are added to
// each other first, so that p is rounded once per step.
__global__ __launch_bounds__(kT) void k_nadam(const Ctl* ctl, const float* __restrict__ rows, float* __restrict__ p,
                                              const float* __restrict__ g, float* __restrict__ m,
                                              float* __restrict__ v, int64_t np) {
    OFP_CNN_STOPPED(ctl);
    const float* row = rows + (int64_t)(ctl ? ctl->epoch : 0) * 4;
    const float c1 = row[0], c2 = row[1], bc2 = row[2];
    for (int64_t i = (int64_t)blockIdx.x * kT + threadIdx.x; i < np; i += (int64_t)gridDim.x * kT) {
        const float gr = g[i];
        const float mo = fmaf(0.1f, gr - m[i], m[i]);
        const float vo = v[i] * 0.999f + (0.001f * gr) * gr;
        m[i] = mo, v[i] = vo;
        const float denom = sqrtf(vo / bc2) + 1e-8f;
        p[i] = p[i] + ((c1 * gr) / denom + (c2 * mo) / denom);
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------

// k_nadam's state: the zeroing of its two moments in front of the first epoch (every NAdam trainer's enqueue_reset)
int zero_moments(float* m, float* v, int64_t np, hipStream_t st) {
    OFP_HIP(hipMemsetAsync(m, 0, (size_t)np * 4, st));
    OFP_HIP(hipMemsetAsync(v, 0, (size_t)np * 4, st));
    return OFP_OK;
}

int check_conv(const char* who, int64_t n, int cin, int w, int cout, int k, int padding, int dilation, int groups) {
    OFP_REQUIRE(n >= 1 && n <= kMaxBatch, "%s: batch of %lld (limit: 1..%d)", who, (long long)n, kMaxBatch);
    OFP_REQUIRE(cin >= 1 && cin <= kMaxCh && cout >= 1 && cout <= kMaxCh, "%s: %d -> %d channels (limit: 1..%d)", who,
                cin, cout, kMaxCh);
    OFP_REQUIRE(w >= 1 && w <= kMaxWidth, "%s: width %d (limit: 1..%d)", who, w, kMaxWidth);
    OFP_REQUIRE(k >= 1 && k <= kMaxKernel, "%s: kernel size %d (limit: 1..%d)", who, k, kMaxKernel);
    OFP_REQUIRE(dilation >= 1 && dilation <= 64 && padding >= 0 && padding <= kMaxWidth,
                "%s: dilation %d, padding %d", who, dilation, padding);
    OFP_REQUIRE(groups >= 1 && cin % groups == 0 && cout % groups == 0, "%s: groups %d do not divide %d and %d", who,
                groups, cin, cout);
    OFP_REQUIRE(w + 2 * padding - dilation * (k - 1) >= 1, "%s: the convolution leaves no output column", who);
    return OFP_OK;
}

// batch statistics of act(z) for one BatchNorm: saved mean / rstd, running statistics updated
int enqueue_bn_stats(const Ctl* ctl, const float* z, int64_t n, int C, int wc, int act, double eps, float mom,
                     double* part, float* mean, float* rstd, float* run_mean, float* run_var, hipStream_t st) {
    const int nslab = slabs_of(n * wc);
    hipLaunchKernelGGL(k_bn_stats_partial, dim3(nslab, C), dim3(kT), 0, st, ctl, z, n, C, wc, act, part);
    OFP_LAUNCH_CHECK("k_bn_stats_partial");
    hipLaunchKernelGGL(k_bn_stats_final, dim3((unsigned)ofp::cdiv(C, kT)), dim3(kT), 0, st, ctl, part, nslab, C,
                       n * wc, eps, mom, mean, rstd, run_mean, run_var);
    OFP_LAUNCH_CHECK("k_bn_stats_final");
    return OFP_OK;
}

// pool routing, BatchNorm backward, activation backward: dh -> dz (and d gamma, d beta)
int enqueue_post_bwd(const Ctl* ctl, const Post& t, int64_t n, const float* z, const float* dh, double* part,
                     float* s12, float* dgamma, float* dbeta, float* dz, hipStream_t st) {
    if (t.mode == 1) {
        const int nslab = slabs_of(n * t.wc);
        hipLaunchKernelGGL(k_bn_bwd_partial, dim3(nslab, t.C), dim3(kT), 0, st, ctl, t, n, z, dh, part);
        OFP_LAUNCH_CHECK("k_bn_bwd_partial");
        hipLaunchKernelGGL(k_bn_bwd_final, dim3((unsigned)ofp::cdiv(t.C, kT)), dim3(kT), 0, st, ctl, part, nslab, t.C,
                           s12, dgamma, dbeta);
        OFP_LAUNCH_CHECK("k_bn_bwd_final");
    }
    hipLaunchKernelGGL(k_dz, dim3(grid_for(n * t.C * t.wc)), dim3(kT), 0, st, ctl, t, n, z, dh, s12, dz);
    OFP_LAUNCH_CHECK("k_dz");
    return OFP_OK;
}

// ---- the stack as a part of a trainer's Plan -------------------------------------------------------------------------

struct ConvStack {
    int L, act, bn, pool;
    double eps;
    float mom;
    Conv conv[kMaxConv];
    int wo[kMaxConv];  // columns of a layer's output: conv[l].wc, halved by the pool
    int w_off[kMaxConv], b_off[kMaxConv], g_off[kMaxConv], be_off[kMaxConv], rs_off[kMaxConv];
    // work space, byte offsets: pre-activations and outputs per layer, the running gradient at an output and at a
    // pre-activation, BatchNorm's saved statistics and its two backward sums
    int64_t o_Z[kMaxConv], o_H[kMaxConv], o_gh, o_gz, o_save, o_s12;
};

// Checks the CNN part of a configuration for a training batch of n (the work space holds nmax = max(n, n_val) samples)
// and plans the stack into `ws`: the layers' parameters go behind the caller's np, their running statistics behind ns,
// max_part_bytes is raised to what the stack's partial sums need.  The last layer's channels and columns are
// s.conv[s.L - 1].cout and s.wo[s.L - 1].
int plan_conv_stack(const char* who, const ofp_cnn_config* c, int64_t n, int64_t nmax, WsPlan& ws, int& np, int& ns,
                    int64_t& max_part_bytes, ConvStack& s) {
    OFP_REQUIRE(c->n_conv >= 1 && c->n_conv <= kMaxConv, "%s: %d conv layers (limit: 1..%d)", who, c->n_conv, kMaxConv);
    OFP_REQUIRE(c->act >= 0 && c->act <= OFP_ACT_TANH, "%s: unknown activation %d", who, c->act);
    OFP_REQUIRE(c->loss == 0 || c->loss == 1, "%s: loss %d (0 = L1, 1 = MSE)", who, c->loss);
    OFP_REQUIRE(c->n_out >= 1 && c->n_out <= kMaxOut, "%s: %d outputs (limit: 1..%d)", who, c->n_out, kMaxOut);
    if (c->batch_norm)
        OFP_REQUIRE(c->bn_momentum > 0.0f && c->bn_momentum <= 1.0f && c->bn_eps > 0.0,
                    "%s: BatchNorm momentum %g, eps %g (a cumulative average, momentum=None, is not built)", who,
                    (double)c->bn_momentum, c->bn_eps);
    s = ConvStack{};
    s.L = c->n_conv, s.act = c->act, s.bn = c->batch_norm ? 1 : 0, s.pool = c->pool ? 1 : 0;
    s.eps = c->bn_eps, s.mom = c->bn_momentum;
    int width = c->width;
    int64_t max_h = 0, max_z = 0;
    max_part_bytes = std::max<int64_t>(max_part_bytes, 2 * 8);
    for (int l = 0; l < s.L; ++l) {
        const int cin = c->channels[l], cout = c->channels[l + 1];
        if (int rc = check_conv(who, n, cin, width, cout, c->kernel, c->padding, c->dilation, c->groups)) return rc;
        Conv& v = s.conv[l];
        v = Conv{cin, cout, width, width + 2 * c->padding - c->dilation * (c->kernel - 1), c->kernel, c->padding,
                 c->dilation, c->groups, 1};
        OFP_REQUIRE(v.wc <= 2 * kMaxWidth, "%s: layer %d is %d wide (limit: %d)", who, l + 1, v.wc, 2 * kMaxWidth);
        s.wo[l] = s.pool ? v.wc / 2 : v.wc;
        OFP_REQUIRE(s.wo[l] >= 1, "%s: the pool of layer %d leaves no output column", who, l + 1);
        OFP_REQUIRE(!s.bn || n * v.wc >= 2, "%s: BatchNorm needs more than 1 value per channel", who);
        const int T = cin / c->groups * c->kernel + 1;
        s.w_off[l] = np, np += cout * (T - 1);
        s.b_off[l] = np, np += cout;
        if (s.bn) {
            s.g_off[l] = np, np += cout;
            s.be_off[l] = np, np += cout;
            s.rs_off[l] = ns, ns += 2 * cout;
        }
        max_part_bytes = std::max<int64_t>(max_part_bytes, (int64_t)cout * T * slabs_of(n * v.wc) * 8);
        max_h = std::max<int64_t>(max_h, nmax * cout * s.wo[l]);
        max_z = std::max<int64_t>(max_z, nmax * cout * v.wc);
        width = s.wo[l];
    }
    for (int l = 0; l < s.L; ++l) {
        s.o_Z[l] = ws.take(nmax * s.conv[l].cout * s.conv[l].wc * 4);
        s.o_H[l] = ws.take(nmax * s.conv[l].cout * s.wo[l] * 4);
    }
    s.o_gh = ws.take(max_h * 4);
    s.o_gz = ws.take(max_z * 4);
    s.o_save = ws.take((int64_t)ns * 4);
    s.o_s12 = ws.take((int64_t)ns * 4);
    return OFP_OK;
}

template <class Plan>
Post post_of(const Run<Plan>& r, const ConvStack& s, int l, int mode) {
    Post t{};
    t.C = s.conv[l].cout, t.wc = s.conv[l].wc, t.wo = s.wo[l], t.act = s.act, t.pool = s.pool, t.mode = mode;
    t.eps = s.eps;
    if (mode) {
        t.ga = r.P + s.g_off[l], t.be = r.P + s.be_off[l];
        if (mode == 1) {
            t.mean = r.template at<float>(s.o_save) + s.rs_off[l], t.rs = t.mean + t.C;
        } else {
            t.mean = r.RS + s.rs_off[l], t.rs = t.mean + t.C;
        }
    }
    return t;
}

// the stack on a batch x [n][channels][width]; train: batch statistics (`part` takes the partial sums), else running
// statistics.  *features is the last layer's output [n][channels][columns].
template <class Plan>
int enqueue_conv_stack_fwd(const Run<Plan>& r, const ConvStack& s, const float* x, int64_t n, bool train, double* part,
                           const float** features) {
    const float* in = x;
    for (int l = 0; l < s.L; ++l) {
        const Conv& c = s.conv[l];
        float* Z = r.template at<float>(s.o_Z[l]);
        float* H = r.template at<float>(s.o_H[l]);
        hipLaunchKernelGGL(k_conv_fwd, dim3(grid_for(n * c.cout * c.wc)), dim3(kT), 0, r.st, r.ctl, c, n, in,
                           r.P + s.w_off[l], r.P + s.b_off[l], Z);
        OFP_LAUNCH_CHECK("k_conv_fwd");
        const Post t = post_of(r, s, l, s.bn ? (train ? 1 : 2) : 0);
        if (s.bn && train) {
            float* save = r.template at<float>(s.o_save) + s.rs_off[l];
            if (int rc = enqueue_bn_stats(r.ctl, Z, n, c.cout, c.wc, s.act, s.eps, s.mom, part, save, save + c.cout,
                                          r.RS + s.rs_off[l], r.RS + s.rs_off[l] + c.cout, r.st))
                return rc;
        }
        hipLaunchKernelGGL(k_post, dim3(grid_for(n * c.cout * s.wo[l])), dim3(kT), 0, r.st, r.ctl, t, n, Z, H);
        OFP_LAUNCH_CHECK("k_post");
        in = H;
    }
    *features = in;
    return OFP_OK;
}

// backward of the stack from the gradient at its features, which the caller has put into o_gh (overwritten on the way
// down); the parameters' gradients go to r.G
template <class Plan>
int enqueue_conv_stack_bwd(const Run<Plan>& r, const ConvStack& s, const float* x, int64_t n, double* part) {
    float* GH = r.template at<float>(s.o_gh);
    float* GZ = r.template at<float>(s.o_gz);
    for (int l = s.L - 1; l >= 0; --l) {
        const Post t = post_of(r, s, l, s.bn ? 1 : 0);
        const float* Z = r.template at<float>(s.o_Z[l]);
        if (int rc = enqueue_post_bwd(r.ctl, t, n, Z, GH, part, r.template at<float>(s.o_s12) + s.rs_off[l],
                                      r.G + s.g_off[l], r.G + s.be_off[l], GZ, r.st))
            return rc;
        const float* in = l == 0 ? x : r.template at<float>(s.o_H[l - 1]);
        if (int rc = enqueue_conv_bwd(r.ctl, s.conv[l], n, in, r.P + s.w_off[l], GZ, part, r.G + s.w_off[l],
                                      r.G + s.b_off[l], l == 0 ? nullptr : GH, r.st))
            return rc;
    }
    return OFP_OK;
}

}  // namespace
