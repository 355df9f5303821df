// Per-item forward passes of the window regressors (model.CNN, model.CCCNN) as device functions: what k_conv1d,
// k_groupnorm1, k_autocorr_softmax and k_dense (ofp_nn.hip) compute for a batch, computed for ONE item by ONE
// workgroup of 256 threads, so that a kernel which already holds the window (the hop's regress stage,
// ofp_regress_dev.h) runs the whole network without a launch per layer.
//
// Every output is formed by the batched kernel's own sequence of floating-point operations (the library is built
// with -ffp-contract=off, so the sequence written here is the sequence executed):
//   conv      bias, then one fmaf per (ci, kk) in that order; activation; fmaf with the folded BatchNorm; max of the pair
//   groupnorm fp64 sums over i = tid, tid + 256, ...; xor-shuffle tree 32..1; the four wave partials added in order
//   autocorr  one fmaf per (k, i); max / sum by the same strided loops, shuffle tree and four partials (the batched
//             kernel's LDS copy of the lags is the in-place array here: the same values)
//   dense     v_mfma_f32_16x16x4_f32 over k0 = 0, 4, ... with row 0 the only valid row (the other rows of the A
//             fragment are the zeros k_dense feeds for rows past n)
// so the results are bit-equal to the batched kernels on the same item.  Pointers may address LDS or global memory.
// The callers' barriers: every function ends with its outputs written but NOT synchronised, except where noted.
#pragma once
#include <hip/hip_runtime.h>

#include "ofp_mlp.h"

namespace ofpnn {

constexpr int WG = 256;  // threads of the workgroup (four waves: the reductions below keep four partials)

// k_conv1d for n items [cin][w] -> [cout][wout] (wout after the optional pool); thread per output element.
__device__ __forceinline__ void conv_items(const float* x, int n, int cin, int w, const float* __restrict__ wt,
                                           const float* __restrict__ b, int cout, int k, int padding, int dilation,
                                           int groups, int stride, int act, const float* __restrict__ bn_scale,
                                           const float* __restrict__ bn_shift, int pool, int wout, float* y) {
    const int total = n * cout * wout;
    const int cin_g = cin / groups, cout_g = cout / groups;
    for (int i = threadIdx.x; i < total; i += WG) {
        const int p = i % wout;
        const int t = i / wout;
        const int o = t % cout;
        const int s = t / cout;
        const float* xs = x + (s * cin + (o / cout_g) * cin_g) * w;
        const float* ws = wt + o * cin_g * k;
        float best = 0.0f;
        for (int h = 0; h <= pool; ++h) {
            const int pc = (pool ? 2 * p + h : p) * stride;
            const int q0 = pc - padding;
            float acc = b ? b[o] : 0.0f;
            // The chain is k_conv1d's: one fmaf per (ci, kk) with the tap inside the input, in that order.  The loads
            // do not depend on it, so they are issued unconditionally (an outside tap reads a clamped address and its
            // product is dropped) and the unrolled loop keeps several in flight.
            if (q0 >= 0 && q0 + (k - 1) * dilation < w) {
                for (int ci = 0; ci < cin_g; ++ci) {
                    const float* xr = xs + ci * w + q0;
                    const float* wr = ws + ci * k;
#pragma unroll 8
                    for (int kk = 0; kk < k; ++kk) acc = fmaf(xr[kk * dilation], wr[kk], acc);
                }
            } else {
                for (int ci = 0; ci < cin_g; ++ci) {
                    const float* xr = xs + ci * w;
                    const float* wr = ws + ci * k;
#pragma unroll 4
                    for (int kk = 0; kk < k; ++kk) {
                        const int q = q0 + kk * dilation;
                        const bool ok = q >= 0 && q < w;
                        const float t = fmaf(xr[q < 0 ? 0 : q < w ? q : w - 1], wr[kk], acc);
                        acc = ok ? t : acc;
                    }
                }
            }
            float v = ofp_activate(acc, act);
            if (bn_scale) v = fmaf(v, bn_scale[o], bn_shift[o]);
            best = h == 0 ? v : fmaxf(best, v);
        }
        y[i] = best;
    }
}

// k_groupnorm1 for one item [K][V] -> [K][V or V/2].  Contains barriers (all 256 threads must call it); the
// caller's data must be visible before the call.
__device__ __forceinline__ void groupnorm_item(const float* src, int K, int V, const float* __restrict__ gamma,
                                               const float* __restrict__ beta, float eps, int pool, float* dst) {
    __shared__ double red[2][4];
    __shared__ float stat[2];
    const int n = K * V;
    double s = 0.0, ss = 0.0;
    for (int i = threadIdx.x; i < n; i += WG) {
        const double v = (double)src[i];
        s += v;
        ss += v * v;
    }
    for (int o = 32; o > 0; o >>= 1) {
        s += __shfl_xor(s, o);
        ss += __shfl_xor(ss, o);
    }
    if ((threadIdx.x & 63) == 0) {
        red[0][threadIdx.x >> 6] = s;
        red[1][threadIdx.x >> 6] = ss;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const double ts = red[0][0] + red[0][1] + red[0][2] + red[0][3];
        const double tss = red[1][0] + red[1][1] + red[1][2] + red[1][3];
        const double mean = ts / n;
        const double var = fmax(tss / n - mean * mean, 0.0);
        stat[0] = (float)mean;
        stat[1] = (float)(1.0 / sqrt(var + (double)eps));
    }
    __syncthreads();
    const float mean = stat[0], rstd = stat[1];
    const int Vo = pool ? V / 2 : V;
    for (int i = threadIdx.x; i < K * Vo; i += WG) {
        const int k = i / Vo, p = i - k * Vo;
        const float g = gamma ? gamma[k] : 1.0f, b = beta ? beta[k] : 0.0f;
        if (pool) {
            const float a0 = (src[k * V + 2 * p] - mean) * rstd * g + b;
            const float a1 = (src[k * V + 2 * p + 1] - mean) * rstd * g + b;
            dst[i] = fmaxf(a0, a1);
        } else {
            dst[i] = (src[k * V + p] - mean) * rstd * g + b;
        }
    }
    __syncthreads();  // red / stat are free for the next item
}

// The lags of k_autocorr_softmax for n items at once: maps f [n][K][V] -> dst [n][2V-1], thread per (item, lag) so
// that the 256 threads stay busy when 2V - 1 is just above a multiple of 256; every lag is k_autocorr_softmax's chain
// (one fmaf per (k, i)).
__device__ __forceinline__ void autocorr_items(const float* f, int n, int K, int V, float* dst) {
    const int L = 2 * V - 1;
    for (int t = threadIdx.x; t < n * L; t += WG) {
        const int it = t / L, j = t - it * L;
        const int sh = j - (V - 1);
        const int lo = sh < 0 ? -sh : 0, hi = sh > 0 ? V - sh : V;
        float acc = 0.0f;
        for (int k = 0; k < K; ++k) {
            const float* fk = f + (it * K + k) * V;
#pragma unroll 8
            for (int i = lo; i < hi; ++i) acc = fmaf(fk[i + sh], fk[i], acc);
        }
        dst[t] = acc;
    }
}

// The softmax of k_autocorr_softmax over one item's lags, in place: v [L] holds the lags and receives the
// probabilities (thread j touches only the entries j, j + 256, ... it owns).  red: 4 floats of LDS.  Contains
// barriers; the caller's data must be visible before the call.
__device__ __forceinline__ void softmax_item(float* v, int L, float* red) {
    float m = -INFINITY;
    for (int j = threadIdx.x; j < L; j += WG) m = fmaxf(m, v[j]);
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    __syncthreads();
    float ssum = 0.0f;
    for (int j = threadIdx.x; j < L; j += WG) {
        const float e = expf(v[j] - m);
        v[j] = e;
        ssum += e;
    }
    for (int o = 32; o > 0; o >>= 1) ssum += __shfl_xor(ssum, o);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = ssum;
    __syncthreads();
    ssum = red[0] + red[1] + red[2] + red[3];
    for (int j = threadIdx.x; j < L; j += WG) v[j] = v[j] / ssum;
    __syncthreads();  // red is free for the next item
}

// k_dense for one row: y[col] = act((x . W[col] + b[col]) * scale[col] + shift[col]), W [out][in].  The four waves
// take the 16-column tiles in turn; lane l feeds A with x[k0 + (l >> 4)] in row l & 15 == 0 only.  The MFMA chain over
// k is serial by definition; the operands of the next DENSE_AHEAD steps are loaded while the current ones multiply.
constexpr int DENSE_AHEAD = 16;
__device__ __forceinline__ void dense_row(const float* x, int in, int out, const float* __restrict__ w,
                                          const float* __restrict__ b, const float* __restrict__ scale,
                                          const float* __restrict__ shift, int act, float* y) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int li = lane & 15, lk = lane >> 4;
    const int col_tiles = (out + 15) / 16;
    for (int ct = wave; ct < col_tiles; ct += WG / 64) {
        const int bcol = ct * 16 + li;
        const float* wr = w + bcol * in;
        const bool bcol_ok = bcol < out;
        ofp_f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        float an[DENSE_AHEAD], bn[DENSE_AHEAD];
        auto load = [&](int k0) {
#pragma unroll
            for (int u = 0; u < DENSE_AHEAD; ++u) {
                const int k = k0 + 4 * u + lk;
                an[u] = (li == 0 && k < in) ? x[k] : 0.0f;
                bn[u] = (bcol_ok && k < in) ? wr[k] : 0.0f;
            }
        };
        load(0);
        for (int k0 = 0; k0 < in; k0 += 4 * DENSE_AHEAD) {
            float ac[DENSE_AHEAD], bc[DENSE_AHEAD];
#pragma unroll
            for (int u = 0; u < DENSE_AHEAD; ++u) {
                ac[u] = an[u];
                bc[u] = bn[u];
            }
            if (k0 + 4 * DENSE_AHEAD < in) load(k0 + 4 * DENSE_AHEAD);
#pragma unroll
            for (int u = 0; u < DENSE_AHEAD; ++u)
                if (k0 + 4 * u < in) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(ac[u], bc[u], acc, 0, 0, 0);
        }
        if (bcol_ok && lk == 0) {  // row 0 is acc[0] of the lanes with lane >> 4 == 0
            const float bias = b ? b[bcol] : 0.0f;
            const float sc = scale ? scale[bcol] : 1.0f;
            const float sh = shift ? shift[bcol] : 0.0f;
            y[bcol] = ofp_activate((acc[0] + bias) * sc + sh, act);
        }
    }
}

}  // namespace ofpnn
