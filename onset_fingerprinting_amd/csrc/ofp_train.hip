// Calibration on the GPU (calibration.py: train_location_model :685-754, optimize_positions :563-682).
//
// One workgroup runs one whole optimisation: forward, mean loss, early-stop test, backward, clip_grad_norm_(1),
// Adam and the loss curve, for every epoch, inside ONE launch; the grid is the M independent problems.  Workgroups
// never talk to each other.  Parameters, Adam moments and the batch's activations live in one arena: the LDS while
// it fits the 160 KiB, a per-problem slice of a caller-provided global work space otherwise (same code, the arena
// pointer is the template parameter).
//
// Every reduction over the batch has a fixed shape: an output (a weight gradient, a BatchNorm statistic) is summed by
// a group of g adjacent lanes (g a power of two chosen from the number of outputs alone), lane s taking rows s, s+g,
// ... in ascending order, then an xor butterfly over the g lanes.  The loss and the gradient norm are summed per
// thread, per wave (butterfly), then over the four waves in wave order.  Nothing depends on M, the workgroup's
// position, or timing; there are no atomics.
//
// Barriers per epoch (k_fcnn_train, L linear layers): L - 1 hidden forwards, 1 output + loss, L backward phases,
// 1 after Adam = 2L + 1; BatchNorm adds L - 1 (its backward needs the two batch sums before dz).  k_tdoa_fit: 1.
#include "ofp_common.h"
#include "ofp_mlp.h"

#include <cmath>

namespace {

constexpr int kT = 256;  // threads per workgroup
constexpr int kW = kT / 64;
constexpr int kMaxLin = 8;
constexpr int kMaxWidth = 128;
constexpr int kMaxBatch = 1024;
constexpr int kMaxSounds = 4096;
constexpr int64_t kLdsBudget = 160 * 1024 - 512;  // the static partial-sum arrays share the 160 KiB

struct FcnnDesc {
    int n_lin, act, bn, bias, loss, N, np, ns;
    int dims[kMaxLin + 1];
    int w_off[kMaxLin], b_off[kMaxLin], g_off[kMaxLin], be_off[kMaxLin], rs_off[kMaxLin];
    int o_P, o_G, o_M, o_V, o_RS, o_BS, o_Y, o_D0, o_D1;
    int o_A[kMaxLin], o_Z[kMaxLin];
    int arena_floats;
};

struct FcnnArgs {
    const float* x;
    int64_t x_stride;
    const float* y;
    int64_t y_stride;
    const float* p0;
    const float* stats0;
    const float* rates;  // [U][E][2]: lr_t / (1 - beta1^t), sqrt(1 - beta2^t)
    const int32_t* rate_idx;
    int E;
    float eps;
    int patience;
    int grads_only;
    float* params;
    float* stats;
    float* loss;
    int32_t* epochs;
    float* grads;
    float* ws;
};

// dims and options -> parameter packing (state_dict order: weight, bias, then BatchNorm weight, bias per layer) and
// the arena layout.  Activations are feature-major ([feature][N]) so that the lanes of a group read consecutive rows.
int fcnn_layout(int32_t n_lin, const int32_t* dims, int32_t act, int32_t bn, int32_t bias, int32_t loss, int64_t n,
                FcnnDesc& d) {
    OFP_REQUIRE(dims != nullptr, "fcnn training: dims is NULL");
    OFP_REQUIRE(n_lin >= 1 && n_lin <= kMaxLin, "fcnn training: %d linear layers (limit: 1..%d)", n_lin, kMaxLin);
    for (int i = 0; i <= n_lin; ++i)
        OFP_REQUIRE(dims[i] >= 1 && dims[i] <= kMaxWidth, "fcnn training: layer width %d (limit: 1..%d)", dims[i],
                    kMaxWidth);
    OFP_REQUIRE(n >= 1 && n <= kMaxBatch, "fcnn training: batch of %lld rows (limit: 1..%d)", (long long)n,
                kMaxBatch);
    OFP_REQUIRE(!(bn && n_lin > 1 && n < 2), "fcnn training: BatchNorm needs more than 1 row");
    OFP_REQUIRE(act >= 0 && act <= OFP_ACT_TANH, "fcnn training: unknown activation %d", act);
    OFP_REQUIRE(loss == 0 || loss == 1, "fcnn training: loss %d (0 = L1, 1 = MSE)", loss);
    d = FcnnDesc{};
    d.n_lin = n_lin, d.act = act, d.bn = bn ? 1 : 0, d.bias = bias ? 1 : 0, d.loss = loss, d.N = (int)n;
    int np = 0, ns = 0, maxw = 0;
    for (int l = 0; l < n_lin; ++l) {
        const int in = dims[l], w = dims[l + 1];
        d.dims[l] = in, d.dims[l + 1] = w;
        d.w_off[l] = np, np += w * in;
        d.b_off[l] = np, np += bias ? w : 0;
        if (bn && l < n_lin - 1) {
            d.g_off[l] = np, np += w;
            d.be_off[l] = np, np += w;
            d.rs_off[l] = ns, ns += 2 * w;
        }
        maxw = w > maxw ? w : maxw;
    }
    d.np = np, d.ns = ns;
    const int N = (int)n;
    int o = 0;
    d.o_P = o, o += np;
    d.o_G = o, o += np;
    d.o_M = o, o += np;
    d.o_V = o, o += np;
    d.o_RS = o, o += ns;
    d.o_BS = o, o += ns;
    d.o_Y = o, o += dims[n_lin] * N;
    for (int l = 0; l < n_lin; ++l) d.o_A[l] = o, o += dims[l] * N;
    for (int l = 0; l + 1 < n_lin; ++l) d.o_Z[l] = o, o += dims[l + 1] * N;
    d.o_D0 = o, o += maxw * N;
    d.o_D1 = o, o += maxw * N;
    d.arena_floats = o;
    return OFP_OK;
}

// Compensated (Kahan) running sum: a lane's share of a batch reduction is up to N / g terms long, and a plain fp32
// chain of that length loses several ulps; the arithmetic is free next to the barriers and LDS latency.  The
// log2(g) additions that join the lanes' partial sums (group_sum) are plain fp32, each rounded at the size of the
// result: that is what is left of the error (up to about 1.5 ulp of a gradient entry, measured).
struct KSum {
    float s = 0.0f, c = 0.0f;
    __device__ __forceinline__ void add(float v) {
        const float y = v - c;
        const float t = s + y;
        c = (t - s) - y;
        s = t;
    }
};

__device__ __forceinline__ float group_sum(float v, int g) {
    for (int o = g >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
// lanes per output: the largest power of two <= 64 that still gives every output its own group in one pass
__device__ __forceinline__ int group_size(int outputs) {
    int g = 64;
    while (g > 1 && outputs * g > kT) g >>= 1;
    return g;
}

// d act / d y at pre-activation y (a = act(y))
__device__ __forceinline__ float act_grad(float y, float a, int act) {
    switch (act) {
        case OFP_ACT_RELU: return y > 0.0f ? 1.0f : 0.0f;
        case OFP_ACT_SILU: {
            const float s = 1.0f / (1.0f + expf(-y));
            return s * (1.0f + y * (1.0f - s));
        }
        case OFP_ACT_LEAKYRELU: return y > 0.0f ? 1.0f : 0.01f;
        case OFP_ACT_ELU: return y > 0.0f ? 1.0f : expf(y);
        case OFP_ACT_TANH: return 1.0f - a * a;
        default: return 1.0f;
    }
}

// sum_k ap[k][n] * w[k * ws], from `acc`
__device__ __forceinline__ float dot_rows(const float* ap, int N, int n, const float* w, int in, float acc) {
    for (int k = 0; k < in; ++k) acc = fmaf(ap[k * N + n], w[k], acc);
    return acc;
}

template <bool LDS>
__global__ __launch_bounds__(kT) void k_fcnn_train(const FcnnDesc d, const FcnnArgs a) {
    extern __shared__ float smem[];
    __shared__ float s_loss[kW];
    __shared__ float s_gn[kW];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t m = blockIdx.x;
    float* ar;
    if constexpr (LDS)
        ar = smem;
    else
        ar = a.ws + m * (int64_t)d.arena_floats;
    const int N = d.N, L = d.n_lin, np = d.np, ns = d.ns, E = a.E;
    const int n_out = d.dims[L];
    float* P = ar + d.o_P;
    float* G = ar + d.o_G;
    float* Mo = ar + d.o_M;
    float* Vo = ar + d.o_V;
    float* RS = ar + d.o_RS;
    float* BS = ar + d.o_BS;
    float* Y = ar + d.o_Y;

    for (int i = tid; i < np; i += kT) {
        P[i] = a.p0[m * np + i];
        Mo[i] = 0.0f;
        Vo[i] = 0.0f;
    }
    for (int i = tid; i < ns; i += kT) RS[i] = a.stats0[m * ns + i];
    {
        const float* x = a.x + m * a.x_stride;
        const float* y = a.y + m * a.y_stride;
        const int F = d.dims[0];
        float* A0 = ar + d.o_A[0];
        for (int i = tid; i < N * F; i += kT) A0[(i % F) * N + i / F] = x[i];
        for (int i = tid; i < N * n_out; i += kT) Y[(i % n_out) * N + i / n_out] = y[i];
    }
    __syncthreads();

    const float* rates = a.grads_only ? nullptr : a.rates + (int64_t)a.rate_idx[m] * E * 2;
    const float inv_numel = 1.0f / (float)(n_out * N);
    const float mse_scale = 2.0f / (float)(n_out * N);
    float last = INFINITY;
    int counter = 0, n_rec = 0;

    for (int e = 0; e < E; ++e) {
        float gsq = 0.0f;
        // ---- forward, hidden layers ----
        for (int l = 0; l + 1 < L; ++l) {
            const int in = d.dims[l], w = d.dims[l + 1];
            const float* Ap = ar + d.o_A[l];
            float* Z = ar + d.o_Z[l];
            float* An = ar + d.o_A[l + 1];
            const float* W = P + d.w_off[l];
            const float* B = P + d.b_off[l];
            if (!d.bn) {
                for (int idx = tid; idx < w * N; idx += kT) {
                    const int j = idx / N, n = idx - j * N;
                    const float z = dot_rows(Ap, N, n, W + j * in, in, d.bias ? B[j] : 0.0f);
                    Z[idx] = z;
                    An[idx] = ofp_activate(z, d.act);
                }
            } else {
                // one lane group per feature: linear, batch mean, biased variance, normalise, activate
                const int g = group_size(w), per = kT / g, sub = tid & (g - 1);
                for (int base = 0; base < w; base += per) {
                    const int j = base + tid / g;
                    const bool valid = j < w;
                    KSum s;
                    if (valid)
                        for (int n = sub; n < N; n += g) {
                            const float z = dot_rows(Ap, N, n, W + j * in, in, d.bias ? B[j] : 0.0f);
                            Z[j * N + n] = z;
                            s.add(z);
                        }
                    const float mean = group_sum(s.s, g) / (float)N;
                    KSum qs;
                    if (valid)
                        for (int n = sub; n < N; n += g) {
                            const float dd = Z[j * N + n] - mean;
                            qs.add(dd * dd);
                        }
                    const float q = group_sum(qs.s, g);
                    const float invstd = 1.0f / sqrtf(q / (float)N + 1e-5f);
                    if (valid) {
                        const float ga = P[d.g_off[l] + j], be = P[d.be_off[l] + j];
                        for (int n = sub; n < N; n += g) {
                            const float y = (Z[j * N + n] - mean) * invstd * ga + be;
                            An[j * N + n] = ofp_activate(y, d.act);
                        }
                        if (sub == 0) {
                            float* bs = BS + d.rs_off[l];
                            float* rs = RS + d.rs_off[l];
                            bs[j] = mean, bs[w + j] = invstd;
                            rs[j] = 0.1f * mean + 0.9f * rs[j];
                            rs[w + j] = 0.1f * (q / (float)(N - 1)) + 0.9f * rs[w + j];
                        }
                    }
                }
            }
            __syncthreads();
        }
        // ---- output layer, residual, d loss / d output ----
        float* cur = ar + d.o_D0;
        float* nxt = ar + d.o_D1;
        {
            const int in = d.dims[L - 1];
            const float* Ap = ar + d.o_A[L - 1];
            const float* W = P + d.w_off[L - 1];
            const float* B = P + d.b_off[L - 1];
            KSum psum;
            for (int idx = tid; idx < n_out * N; idx += kT) {
                const int j = idx / N, n = idx - j * N;
                const float o = dot_rows(Ap, N, n, W + j * in, in, d.bias ? B[j] : 0.0f);
                const float r = o - Y[idx];
                if (d.loss == 0) {
                    psum.add(fabsf(r));
                    cur[idx] = r > 0.0f ? inv_numel : (r < 0.0f ? -inv_numel : 0.0f);
                } else {
                    psum.add(r * r);
                    cur[idx] = mse_scale * r;
                }
            }
            const float part = group_sum(psum.s, 64);
            if (lane == 0) s_loss[wave] = part;
        }
        __syncthreads();
        const float loss = (((s_loss[0] + s_loss[1]) + s_loss[2]) + s_loss[3]) * inv_numel;
        if (!a.grads_only) {
            if (tid == 0) a.loss[m * E + e] = loss;
            ++n_rec;
            if (loss < last - a.eps) {
                last = loss;
                counter = 0;
            } else if (counter < a.patience) {
                ++counter;
            } else {
                break;
            }
        }
        // ---- backward ----
        for (int l = L - 1; l >= 0; --l) {
            const int in = d.dims[l], w = d.dims[l + 1];
            const float* dz = cur;
            const float* Ap = ar + d.o_A[l];
            const float* W = P + d.w_off[l];
            {
                const int O = w * in + (d.bias ? w : 0);
                const int g = group_size(O), per = kT / g, sub = tid & (g - 1);
                for (int base = 0; base < O; base += per) {
                    const int o = base + tid / g;
                    const bool valid = o < O;
                    KSum ks;
                    if (valid) {
                        if (o < w * in) {
                            const int j = o / in, k = o - j * in;
                            for (int n = sub; n < N; n += g) ks.add(dz[j * N + n] * Ap[k * N + n]);
                        } else {
                            const int j = o - w * in;
                            for (int n = sub; n < N; n += g) ks.add(dz[j * N + n]);
                        }
                    }
                    const float s = group_sum(ks.s, g);
                    if (valid && sub == 0) {
                        G[(o < w * in ? d.w_off[l] + o : d.b_off[l] + o - w * in)] = s;
                        gsq = fmaf(s, s, gsq);
                    }
                }
            }
            if (l > 0) {
                const float* Zp = ar + d.o_Z[l - 1];
                for (int idx = tid; idx < in * N; idx += kT) {
                    const int k = idx / N, n = idx - k * N;
                    float s = 0.0f;
                    for (int j = 0; j < w; ++j) s = fmaf(dz[j * N + n], W[j * in + k], s);
                    if (!d.bn) s *= act_grad(Zp[idx], Ap[idx], d.act);
                    nxt[idx] = s;
                }
            } else {
                gsq = group_sum(gsq, 64);
                if (lane == 0) s_gn[wave] = gsq;
            }
            __syncthreads();
            if (l > 0 && d.bn) {
                // BatchNorm + activation backward of layer l - 1 (width `in`), in place on nxt
                const float* Zp = ar + d.o_Z[l - 1];
                const float* bs = BS + d.rs_off[l - 1];
                const int g = group_size(in), per = kT / g, sub = tid & (g - 1);
                for (int base = 0; base < in; base += per) {
                    const int j = base + tid / g;
                    const bool valid = j < in;
                    KSum k1, k2;
                    float mean = 0.0f, invstd = 0.0f, ga = 0.0f, be = 0.0f;
                    if (valid) {
                        mean = bs[j], invstd = bs[in + j];
                        ga = P[d.g_off[l - 1] + j], be = P[d.be_off[l - 1] + j];
                        for (int n = sub; n < N; n += g) {
                            const float xh = (Zp[j * N + n] - mean) * invstd;
                            const float y = (Zp[j * N + n] - mean) * invstd * ga + be;
                            const float dy = nxt[j * N + n] * act_grad(y, Ap[j * N + n], d.act);
                            nxt[j * N + n] = dy;
                            k1.add(dy);
                            k2.add(dy * xh);
                        }
                    }
                    const float s1 = group_sum(k1.s, g), s2 = group_sum(k2.s, g);
                    if (valid) {
                        const float m1 = s1 / (float)N, m2 = s2 / (float)N;
                        for (int n = sub; n < N; n += g) {
                            const float xh = (Zp[j * N + n] - mean) * invstd;
                            nxt[j * N + n] = (nxt[j * N + n] - m1 - xh * m2) * invstd * ga;
                        }
                        if (sub == 0) {
                            G[d.g_off[l - 1] + j] = s2;
                            G[d.be_off[l - 1] + j] = s1;
                            gsq = fmaf(s2, s2, fmaf(s1, s1, gsq));
                        }
                    }
                }
                __syncthreads();
            }
            float* t = cur;
            cur = nxt, nxt = t;
        }
        if (a.grads_only) {
            for (int i = tid; i < np; i += kT) a.grads[m * np + i] = G[i];
            if (tid == 0) a.loss[m] = loss;
            return;
        }
        // ---- clip_grad_norm_(max_norm = 1), Adam ----
        const float total = sqrtf(((s_gn[0] + s_gn[1]) + s_gn[2]) + s_gn[3]);
        const float coef = fminf(1.0f / (total + 1e-6f), 1.0f);
        const float nstep = -rates[2 * e], bc2 = rates[2 * e + 1];
        for (int i = tid; i < np; i += kT) {
            const float gr = G[i] * coef;
            const float mo = fmaf(0.1f, gr - Mo[i], Mo[i]);
            const float vo = Vo[i] * 0.999f + (0.001f * gr) * gr;
            Mo[i] = mo, Vo[i] = vo;
            P[i] = P[i] + (nstep * mo) / (sqrtf(vo) / bc2 + 1e-8f);
        }
        __syncthreads();
    }
    for (int i = tid; i < np; i += kT) a.params[m * np + i] = P[i];
    for (int i = tid; i < ns; i += kT) a.stats[m * ns + i] = RS[i];
    if (tid == 0) a.epochs[m] = n_rec;
}

struct TdoaArgs {
    const float* obs;  // [M][N][2] seconds (or one shared [N][2])
    int64_t obs_stride;
    const float* sensors0;  // [M][4][3]
    const float* sounds0;   // [M][N][2]
    const float* c0;        // [M]
    const float* rates;     // [U][E][4]: the three step sizes, sqrt(1 - beta2^t)
    const int32_t* rate_idx;
    int N, E, loss;
    float eps;
    int patience;
    float* sensors;
    float* sounds;  // [M][N][3]
    float* c;
    float* lossc;
    int32_t* epochs;
    int grads_only;  // leave after the first epoch's sums: loss [M], g_sensors [M][12], g_sounds [M][N][2], g_c [M]
    float* g_sensors;
    float* g_sounds;
    float* g_c;
};

__device__ __forceinline__ void adam1(float& p, float& mo, float& vo, float gr, float nstep, float bc2) {
    mo = fmaf(0.1f, gr - mo, mo);
    vo = vo * 0.999f + (0.001f * gr) * gr;
    p = p + (nstep * mo) / (sqrtf(vo) / bc2 + 1e-8f);
}

// optimize_positions: 4 sensors [4][3], x and y of every sound, C.  Sensors and C (and their moments) are kept by
// every thread in registers and updated redundantly, the sounds in LDS by the thread that owns them: one barrier
// (the sums of the 12 sensor gradients, C's, the loss and the sounds' squared gradients) per epoch.
__global__ __launch_bounds__(kT) void k_tdoa_fit(const TdoaArgs a) {
    extern __shared__ float smem[];
    __shared__ float s_part[2][kW][16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t m = blockIdx.x;
    const int N = a.N, E = a.E;
    float* SP = smem;
    float* SG = SP + 2 * N;
    float* SM = SG + 2 * N;
    float* SV = SM + 2 * N;
    const float* obs = a.obs + m * a.obs_stride;
    float s[12], sm[12], sv[12], c = a.c0[m], cm = 0.0f, cv = 0.0f;
#pragma unroll
    for (int i = 0; i < 12; ++i) s[i] = a.sensors0[m * 12 + i], sm[i] = 0.0f, sv[i] = 0.0f;
    for (int n = tid; n < N; n += kT) {
        SP[n] = a.sounds0[(m * N + n) * 2], SP[N + n] = a.sounds0[(m * N + n) * 2 + 1];
        SM[n] = SM[N + n] = SV[n] = SV[N + n] = 0.0f;
    }
    const float* rates = a.grads_only ? nullptr : a.rates + (int64_t)a.rate_idx[m] * E * 4;
    const float inv_numel = 1.0f / (float)(2 * N);
    const float mse_scale = 2.0f / (float)(2 * N);
    float last = INFINITY;
    int counter = 0, n_rec = 0;
    for (int e = 0; e < E; ++e) {
        float acc[15];
#pragma unroll
        for (int i = 0; i < 15; ++i) acc[i] = 0.0f;
        for (int n = tid; n < N; n += kT) {
            const float x = SP[n], y = SP[N + n];
            float df[4][3], dist[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                df[i][0] = x - s[3 * i], df[i][1] = y - s[3 * i + 1], df[i][2] = 0.0f - s[3 * i + 2];
                dist[i] = sqrtf((df[i][0] * df[i][0] + df[i][1] * df[i][1]) + df[i][2] * df[i][2]);
            }
            const float t0 = (dist[0] - dist[2]) / c, t1 = (dist[1] - dist[3]) / c;
            const float r0 = t0 - obs[2 * n], r1 = t1 - obs[2 * n + 1];
            float dl0, dl1;
            if (a.loss == 0) {
                acc[13] += fabsf(r0) + fabsf(r1);
                dl0 = r0 > 0.0f ? inv_numel : (r0 < 0.0f ? -inv_numel : 0.0f);
                dl1 = r1 > 0.0f ? inv_numel : (r1 < 0.0f ? -inv_numel : 0.0f);
            } else {
                acc[13] += r0 * r0 + r1 * r1;
                dl0 = mse_scale * r0, dl1 = mse_scale * r1;
            }
            acc[12] += -(dl0 * (t0 / c)) - (dl1 * (t1 / c));
            const float gd[4] = {dl0 / c, dl1 / c, -(dl0 / c), -(dl1 / c)};
            float gx = 0.0f, gy = 0.0f;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float f = gd[i] / (2.0f * dist[i]);
                const float fx = f * (2.0f * df[i][0]), fy = f * (2.0f * df[i][1]), fz = f * (2.0f * df[i][2]);
                gx += fx, gy += fy;
                acc[3 * i] -= fx, acc[3 * i + 1] -= fy, acc[3 * i + 2] -= fz;
            }
            SG[n] = gx, SG[N + n] = gy;
            acc[14] = fmaf(gx, gx, fmaf(gy, gy, acc[14]));
        }
#pragma unroll
        for (int i = 0; i < 15; ++i) {
            acc[i] = group_sum(acc[i], 64);
            if (lane == 0) s_part[e & 1][wave][i] = acc[i];
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 15; ++i)
            acc[i] = ((s_part[e & 1][0][i] + s_part[e & 1][1][i]) + s_part[e & 1][2][i]) + s_part[e & 1][3][i];
        const float loss = acc[13] * inv_numel;
        if (a.grads_only) {  // the fit's own sums, unclipped; every thread wrote its own SG entries
            for (int n = tid; n < N; n += kT) {
                float* o = a.g_sounds + (m * N + n) * 2;
                o[0] = SG[n], o[1] = SG[N + n];
            }
            if (tid == 0) {
                a.lossc[m] = loss;
                for (int i = 0; i < 12; ++i) a.g_sensors[m * 12 + i] = acc[i];
                a.g_c[m] = acc[12];
            }
            return;
        }
        bool stop = false;
        if (loss < last - a.eps) {
            last = loss;
            counter = 0;
        } else if (counter < a.patience) {
            ++counter;
        } else {
            stop = true;
        }
        if (stop || e == E - 1)  // the reference returns the sound positions its last forward pass used
            for (int n = tid; n < N; n += kT) {
                float* o = a.sounds + (m * N + n) * 3;
                o[0] = SP[n], o[1] = SP[N + n], o[2] = 0.0f;
            }
        if (tid == 0) a.lossc[m * E + e] = loss;  // the stopping epoch's loss is stored but not counted
        if (stop) break;
        ++n_rec;
        float gsq = acc[14];
#pragma unroll
        for (int i = 0; i < 13; ++i) gsq = fmaf(acc[i], acc[i], gsq);
        const float coef = fminf(1.0f / (sqrtf(gsq) + 1e-6f), 1.0f);
        const float bc2 = rates[4 * e + 3];
        const float n_sens = -rates[4 * e], n_snd = -rates[4 * e + 1], n_c = -rates[4 * e + 2];
#pragma unroll
        for (int i = 0; i < 12; ++i) adam1(s[i], sm[i], sv[i], acc[i] * coef, n_sens, bc2);
        adam1(c, cm, cv, acc[12] * coef, n_c, bc2);
        for (int n = tid; n < N; n += kT) {
            adam1(SP[n], SM[n], SV[n], SG[n] * coef, n_snd, bc2);
            adam1(SP[N + n], SM[N + n], SV[N + n], SG[N + n] * coef, n_snd, bc2);
        }
    }
    if (tid == 0) {
        for (int i = 0; i < 12; ++i) a.sensors[m * 12 + i] = s[i];
        a.c[m] = c;
        a.epochs[m] = n_rec;
    }
}

ofp::LdsAttrCache g_train_lds, g_tdoa_lds;

int tdoa_launch(const TdoaArgs& a, int64_t M, hipStream_t st) {
    const size_t bytes = (size_t)a.N * 8 * sizeof(float);
    if (int rc = ofp::ensure_dynamic_lds((const void*)k_tdoa_fit, bytes, g_tdoa_lds)) return rc;
    hipLaunchKernelGGL(k_tdoa_fit, dim3((unsigned)M), dim3(kT), bytes, st, a);
    OFP_LAUNCH_CHECK("k_tdoa_fit");
    return OFP_OK;
}

int fcnn_launch(const FcnnDesc& d, const FcnnArgs& a, int64_t M, int64_t ws_bytes, hipStream_t st) {
    const int64_t bytes = (int64_t)d.arena_floats * 4;
    if (bytes <= kLdsBudget) {
        if (int rc = ofp::ensure_dynamic_lds((const void*)k_fcnn_train<true>, (size_t)bytes, g_train_lds)) return rc;
        hipLaunchKernelGGL(k_fcnn_train<true>, dim3((unsigned)M), dim3(kT), (size_t)bytes, st, d, a);
    } else {
        if (a.ws == nullptr || ws_bytes < bytes * M)
            return ofp::fail(OFP_ERR_WORKSPACE, "fcnn training: work space of %lld bytes needed, %lld given",
                             (long long)(bytes * M), (long long)ws_bytes);
        hipLaunchKernelGGL(k_fcnn_train<false>, dim3((unsigned)M), dim3(kT), 0, st, d, a);
    }
    OFP_LAUNCH_CHECK("k_fcnn_train");
    return OFP_OK;
}

}  // namespace

extern "C" {

int64_t ofp_fcnn_train_lds_bytes(int32_t n_layers, const int32_t* dims, int32_t batch_norm, int32_t bias, int64_t n) {
    FcnnDesc d;
    if (fcnn_layout(n_layers, dims, 0, batch_norm, bias, 0, n, d)) return -1;
    return (int64_t)d.arena_floats * 4;
}

int64_t ofp_fcnn_train_workspace_bytes(int32_t n_layers, const int32_t* dims, int32_t batch_norm, int32_t bias,
                                       int64_t n, int64_t M) {
    const int64_t bytes = ofp_fcnn_train_lds_bytes(n_layers, dims, batch_norm, bias, n);
    if (bytes < 0) return -1;
    return bytes <= kLdsBudget ? 0 : bytes * M;
}

int ofp_fcnn_train(int32_t n_layers, const int32_t* dims, int32_t act, int32_t batch_norm, int32_t bias,
                   int32_t loss, int64_t M, int64_t n, const float* d_x, int64_t x_stride, const float* d_y,
                   int64_t y_stride, const float* d_p0, const float* d_stats0, const float* d_rates,
                   const int32_t* d_rate_idx, int32_t num_epochs, float eps, int32_t patience, float* d_params,
                   float* d_stats, float* d_loss, int32_t* d_epochs, void* d_ws, int64_t ws_bytes, void* stream) {
    FcnnDesc d;
    if (int rc = fcnn_layout(n_layers, dims, act, batch_norm, bias, loss, n, d)) return rc;
    OFP_REQUIRE(M >= 1 && M <= 1 << 20, "ofp_fcnn_train: %lld problems (limit: 1..2^20)", (long long)M);
    OFP_REQUIRE(num_epochs >= 1 && patience >= 0, "ofp_fcnn_train: num_epochs %d, patience %d", num_epochs, patience);
    OFP_REQUIRE(d_x && d_y && d_p0 && d_rates && d_rate_idx && d_params && d_loss && d_epochs,
                "ofp_fcnn_train: NULL argument");
    OFP_REQUIRE(d.ns == 0 || (d_stats0 && d_stats), "ofp_fcnn_train: BatchNorm statistics are NULL");
    FcnnArgs a{d_x,   x_stride, d_y,      y_stride, d_p0,    d_stats0, d_rates,  d_rate_idx, num_epochs,
               eps,   patience, 0,        d_params, d_stats, d_loss,   d_epochs, nullptr,    (float*)d_ws};
    return fcnn_launch(d, a, M, ws_bytes, (hipStream_t)stream);
}

int ofp_fcnn_loss_grads(int32_t n_layers, const int32_t* dims, int32_t act, int32_t batch_norm, int32_t bias,
                        int32_t loss, int64_t M, int64_t n, const float* d_x, int64_t x_stride, const float* d_y,
                        int64_t y_stride, const float* d_p0, float* d_loss, float* d_grads, void* d_ws,
                        int64_t ws_bytes, void* stream) {
    FcnnDesc d;
    if (int rc = fcnn_layout(n_layers, dims, act, batch_norm, bias, loss, n, d)) return rc;
    OFP_REQUIRE(M >= 1 && M <= 1 << 20, "ofp_fcnn_loss_grads: %lld problems (limit: 1..2^20)", (long long)M);
    OFP_REQUIRE(d_x && d_y && d_p0 && d_loss && d_grads, "ofp_fcnn_loss_grads: NULL argument");
    // the trainer itself, one epoch, leaving after the backward pass; the running statistics are not read
    // (ns floats of the start vector stand in for them) and nothing but loss and gradients is written
    OFP_REQUIRE(d.ns <= d.np, "ofp_fcnn_loss_grads: internal layout");
    FcnnArgs a{d_x,  x_stride, d_y, y_stride, d_p0,    d_p0,    d_p0,   nullptr, 1,
               0.0f, 0,        1,   nullptr,  nullptr, d_loss,  nullptr, d_grads, (float*)d_ws};
    return fcnn_launch(d, a, M, ws_bytes, (hipStream_t)stream);
}

int ofp_tdoa_fit(int64_t M, int64_t n, const float* d_obs, int64_t obs_stride, const float* d_sensors0,
                 const float* d_sounds0, const float* d_c0, int32_t loss, const float* d_rates,
                 const int32_t* d_rate_idx, int32_t num_epochs, float eps, int32_t patience, float* d_sensors,
                 float* d_sounds, float* d_c, float* d_loss, int32_t* d_epochs, void* stream) {
    OFP_REQUIRE(M >= 1 && M <= 1 << 20, "ofp_tdoa_fit: %lld problems (limit: 1..2^20)", (long long)M);
    OFP_REQUIRE(n >= 1 && n <= kMaxSounds, "ofp_tdoa_fit: %lld sounds (limit: 1..%d)", (long long)n, kMaxSounds);
    OFP_REQUIRE(loss == 0 || loss == 1, "ofp_tdoa_fit: loss %d (0 = L1, 1 = MSE)", loss);
    OFP_REQUIRE(num_epochs >= 1 && patience >= 0, "ofp_tdoa_fit: num_epochs %d, patience %d", num_epochs, patience);
    OFP_REQUIRE(d_obs && d_sensors0 && d_sounds0 && d_c0 && d_rates && d_rate_idx && d_sensors && d_sounds && d_c &&
                    d_loss && d_epochs,
                "ofp_tdoa_fit: NULL argument");
    TdoaArgs a{d_obs,      obs_stride, d_sensors0, d_sounds0, d_c0,      d_rates,  d_rate_idx, (int)n,
               num_epochs, loss,       eps,        patience,  d_sensors, d_sounds, d_c,        d_loss,
               d_epochs,   0,          nullptr,    nullptr,   nullptr};
    return tdoa_launch(a, M, (hipStream_t)stream);
}

int ofp_tdoa_loss_grads(int64_t M, int64_t n, const float* d_obs, int64_t obs_stride, const float* d_sensors,
                        const float* d_sounds, const float* d_c, int32_t loss, float* d_loss, float* d_g_sensors,
                        float* d_g_sounds, float* d_g_c, void* stream) {
    OFP_REQUIRE(M >= 1 && M <= 1 << 20, "ofp_tdoa_loss_grads: %lld problems (limit: 1..2^20)", (long long)M);
    OFP_REQUIRE(n >= 1 && n <= kMaxSounds, "ofp_tdoa_loss_grads: %lld sounds (limit: 1..%d)", (long long)n,
                kMaxSounds);
    OFP_REQUIRE(loss == 0 || loss == 1, "ofp_tdoa_loss_grads: loss %d (0 = L1, 1 = MSE)", loss);
    OFP_REQUIRE(d_obs && d_sensors && d_sounds && d_c && d_loss && d_g_sensors && d_g_sounds && d_g_c,
                "ofp_tdoa_loss_grads: NULL argument");
    // the fit itself, leaving after the first epoch's reduction; no rate tables are read, no state is written
    TdoaArgs a{d_obs,   obs_stride, d_sensors, d_sounds, d_c,     nullptr, nullptr, (int)n,
               1,       loss,       0.0f,      0,        nullptr, nullptr, nullptr, d_loss,
               nullptr, 1,          d_g_sensors, d_g_sounds, d_g_c};
    return tdoa_launch(a, M, (hipStream_t)stream);
}

}  // extern "C"
