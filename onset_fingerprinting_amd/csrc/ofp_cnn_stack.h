// The conv stack of model.CNN as both of its trainers run it (csrc/ofp_cnn_train.hip, csrc/ofp_cnnrnn_train.hip): what
// follows a convolution (activation, BatchNorm1d on batch or running statistics, MaxPool1d(2, 2)) forward and backward,
// the NAdam step, the limits of the stack and the launch helpers of the BatchNorm reductions.  File-local like
// ofp_train_chain.h and ofp_train_random.h, which it builds on: each trainer compiles its own copy.
#pragma once
#include "ofp_train_random.h"

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

}  // namespace
