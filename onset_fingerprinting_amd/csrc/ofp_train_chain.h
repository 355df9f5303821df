// Device code and launch helpers shared by the four epoch-graph trainers (csrc/ofp_cnn_train.hip, ofp_cccnn_train.hip,
// ofp_cnnrnn_train.hip, ofp_rnn_train.hip): the control block of a run, the partial-slab reducer's shape, the convolution's
// forward and three gradients (any stride), the Linear head with its loss, and the chain's first and last kernels; on the
// host the work space's base, the checks every trainer makes, one epoch, the driver that captures it as a graph and
// replays it, and the bodies of the public entries (train_workspace_bytes, train_entry, loss_grads_entry), which a trainer
// instantiates with its traits -- the contract is spelt out in front of them.  Everything here is file-local (anonymous
// namespace): each trainer compiles its own copy.
#pragma once
#include "ofp_common.h"
#include "ofp_mlp.h"

#include <cmath>
#include <cstdlib>
#include <cstring>

namespace {

constexpr int kT = 256;        // threads per workgroup
constexpr int kSlab = 2048;    // (sample, position) pairs one workgroup sums
constexpr int kFcChunk = 64;   // samples one thread of the Linear head's weight gradient sums
constexpr int kMaxOut = 16;
constexpr int kCheckEvery = 64;  // epochs between two looks at the stop word

struct Ctl {
    int32_t epoch, stop, wait, reached;
    float best;
    int32_t pad[3];
};

#define OFP_CNN_STOPPED(ctl) \
    if ((ctl) != nullptr && (ctl)->stop) return

struct Conv {
    int cin, cout, win, wc, k, pad, dil, groups, stride;  // wc = (win + 2 pad - dil (k - 1) - 1) / stride + 1
};

// d act / d z at pre-activation z (a = act(z)), as csrc/ofp_train.hip evaluates it
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

// sum of (a, b) over the workgroup: xor butterfly inside each wave, then the four waves in wave order
__device__ __forceinline__ void block_sum2(double& a, double& b, double (*red)[kT / 64]) {
    for (int o = 32; o > 0; o >>= 1) {
        a += __shfl_xor(a, o);
        b += __shfl_xor(b, o);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();  // a previous use of `red` has been read
    if (lane == 0) red[0][wave] = a, red[1][wave] = b;
    __syncthreads();
    a = ((red[0][0] + red[0][1]) + red[0][2]) + red[0][3];
    b = ((red[1][0] + red[1][1]) + red[1][2]) + red[1][3];
}

__global__ __launch_bounds__(kT) void k_init(Ctl* ctl) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        *ctl = Ctl{};
        ctl->best = INFINITY;
    }
}

// z[s][o][p] = b[o] + sum_{ci, kk} x[s][g*cin_g + ci][p*stride - pad + kk*dil] * w[o][ci][kk]: thread per element, the
// arithmetic of k_conv1d (csrc/ofp_nn.hip)
__global__ __launch_bounds__(kT) void k_conv_fwd(const Ctl* ctl, const Conv c, int64_t n, const float* __restrict__ x,
                                                 const float* __restrict__ w, const float* __restrict__ b,
                                                 float* __restrict__ z) {
    OFP_CNN_STOPPED(ctl);
    const int64_t total = n * c.cout * c.wc;
    const int cin_g = c.cin / c.groups, cout_g = c.cout / c.groups;
    for (int64_t i = (int64_t)blockIdx.x * kT + threadIdx.x; i < total; i += (int64_t)gridDim.x * kT) {
        const int p = (int)(i % c.wc);
        const int64_t t = i / c.wc;
        const int o = (int)(t % c.cout);
        const int64_t s = t / c.cout;
        const float* xs = x + (s * c.cin + (int64_t)(o / cout_g) * cin_g) * c.win;
        const float* ws = w + (int64_t)o * cin_g * c.k;
        float acc = b[o];
        for (int ci = 0; ci < cin_g; ++ci)
            for (int kk = 0; kk < c.k; ++kk) {
                const int q = p * c.stride - c.pad + kk * c.dil;
                if (q >= 0 && q < c.win) acc = fmaf(xs[(int64_t)ci * c.win + q], ws[ci * c.k + kk], acc);
            }
        z[i] = acc;
    }
}

// lanes per output of the weight-gradient kernel: the largest power of two <= 64 with outputs * g <= kT
__host__ __device__ inline int lanes_per_output(int outputs) {
    int g = 64;
    while (g > 1 && outputs * g > kT) g >>= 1;
    return g;
}

// dW[o][ci][kk] = sum_{s, p} dz[s][o][p] * x[s][g*cin_g + ci][p*stride - pad + kk*dil], db[o] = sum dz: workgroup (slab, o);
// the cin_g * k weights of channel o and its bias are the T outputs, g adjacent lanes share one output and take
// the slab's pairs sub, sub + g, ... in ascending order, then an xor butterfly joins them
__global__ __launch_bounds__(kT) void k_wgrad_partial(const Ctl* ctl, const Conv c, int64_t n,
                                                      const float* __restrict__ x, const float* __restrict__ dz,
                                                      double* __restrict__ partial) {
    OFP_CNN_STOPPED(ctl);
    const int slab = blockIdx.x, o = blockIdx.y, nslab = gridDim.x;
    const int cin_g = c.cin / c.groups, cout_g = c.cout / c.groups;
    const int T = cin_g * c.k + 1;
    const int g = lanes_per_output(T), per = kT / g, sub = threadIdx.x & (g - 1);
    const int pairs = (int)n * c.wc, q0 = slab * kSlab;
    const int q1 = q0 + kSlab < pairs ? q0 + kSlab : pairs;
    const int ch0 = (o / cout_g) * cin_g;
    for (int base = 0; base < T; base += per) {
        const int wi = base + threadIdx.x / g;
        const bool valid = wi < T;
        const int ci = wi / c.k, kk = wi - ci * c.k;
        const bool bias = wi == T - 1;
        const int shift = kk * c.dil - c.pad;
        double acc = 0.0;
        if (valid)
            for (int q = q0 + sub; q < q1; q += g) {
                const int s = q / c.wc;
                const int p = q - s * c.wc;
                const float d = dz[((int64_t)s * c.cout + o) * c.wc + p];
                if (bias) {
                    acc += (double)d;
                } else {
                    const int xi = p * c.stride + shift;
                    if (xi >= 0 && xi < c.win) acc += (double)d * (double)x[((int64_t)s * c.cin + ch0 + ci) * c.win + xi];
                }
            }
        for (int off = g >> 1; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
        if (valid && sub == 0) partial[((int64_t)o * T + wi) * nslab + slab] = acc;
    }
}

__global__ __launch_bounds__(kT) void k_wgrad_final(const Ctl* ctl, const double* __restrict__ partial, int nslab,
                                                    int cout, int T, float* __restrict__ dw, float* __restrict__ db) {
    OFP_CNN_STOPPED(ctl);
    const int i = blockIdx.x * kT + threadIdx.x;
    if (i >= cout * T) return;
    const int o = i / T, wi = i - o * T;
    double s = 0.0;
    for (int j = 0; j < nslab; ++j) s += partial[(int64_t)i * nslab + j];
    if (wi == T - 1)
        db[o] = (float)s;
    else
        dw[o * (T - 1) + wi] = (float)s;
}

// dx[s][ci][q] = sum_{o in ci's group, kk} dz[s][o][p] * w[o][ci][kk] over the p with p*stride = q + pad - kk*dil:
// thread per element
__global__ __launch_bounds__(kT) void k_dgrad(const Ctl* ctl, const Conv c, int64_t n, const float* __restrict__ dz,
                                              const float* __restrict__ w, float* __restrict__ dx) {
    OFP_CNN_STOPPED(ctl);
    const int64_t total = n * c.cin * c.win;
    const int cin_g = c.cin / c.groups, cout_g = c.cout / c.groups;
    for (int64_t i = (int64_t)blockIdx.x * kT + threadIdx.x; i < total; i += (int64_t)gridDim.x * kT) {
        const int q = (int)(i % c.win);
        const int64_t t = i / c.win;
        const int ci = (int)(t % c.cin);
        const int64_t s = t / c.cin;
        const int grp = ci / cin_g, cil = ci - grp * cin_g;
        float acc = 0.0f;
        for (int oo = 0; oo < cout_g; ++oo) {
            const int o = grp * cout_g + oo;
            const float* dr = dz + (s * c.cout + o) * c.wc;
            const float* wr = w + ((int64_t)o * cin_g + cil) * c.k;
            for (int kk = 0; kk < c.k; ++kk) {
                int p = q + c.pad - kk * c.dil;
                if (c.stride > 1) {
                    if (p < 0 || p % c.stride) continue;
                    p /= c.stride;
                }
                if (p >= 0 && p < c.wc) acc = fmaf(dr[p], wr[kk], acc);
            }
        }
        dx[i] = acc;
    }
}

// Linear head of one sample per workgroup: out = W h + b (fp64 sums over the F features), the sample's share of
// the loss (sum over its outputs of |r| or r^2) and, when dy is given, d loss / d out
__global__ __launch_bounds__(kT) void k_fc_fwd(const Ctl* ctl, const float* __restrict__ h, int F, int O,
                                               const float* __restrict__ w, const float* __restrict__ b,
                                               const float* __restrict__ y, int loss, float inv_numel,
                                               float* __restrict__ out, float* __restrict__ dy,
                                               double* __restrict__ part) {
    OFP_CNN_STOPPED(ctl);
    __shared__ double red[2][kT / 64];
    const int64_t s = blockIdx.x;
    const float* hr = h + s * F;
    double lsum = 0.0;
    for (int j = 0; j < O; j += 2) {
        const bool two = j + 1 < O;
        double a0 = 0.0, a1 = 0.0;
        for (int f = threadIdx.x; f < F; f += kT) {
            const double hv = (double)hr[f];
            a0 += hv * (double)w[(int64_t)j * F + f];
            if (two) a1 += hv * (double)w[(int64_t)(j + 1) * F + f];
        }
        block_sum2(a0, a1, red);
        if (threadIdx.x == 0) {
            for (int u = 0; u < (two ? 2 : 1); ++u) {
                const float o = (float)((u ? a1 : a0) + (double)b[j + u]);
                const float r = o - y[s * O + j + u];
                out[s * O + j + u] = o;
                if (loss == 0) {
                    lsum += (double)fabsf(r);
                    if (dy) dy[s * O + j + u] = r > 0.0f ? inv_numel : (r < 0.0f ? -inv_numel : 0.0f);
                } else {
                    lsum += (double)r * (double)r;
                    if (dy) dy[s * O + j + u] = (2.0f * inv_numel) * r;
                }
            }
        }
    }
    if (threadIdx.x == 0) part[s] = lsum;
}

// mean loss of the batch into slot `epoch` of a curve (and the head's bias gradient); for the validation loss also Lightning's early-stop rule
// (min_delta 0): a loss that is not below the best so far counts towards patience
__global__ __launch_bounds__(kT) void k_loss_final(Ctl* ctl, const double* __restrict__ part, int64_t n, int O,
                                                   float* __restrict__ curve, int validation, int patience,
                                                   const float* __restrict__ dy, float* __restrict__ db) {
    OFP_CNN_STOPPED(ctl);
    __shared__ double red[2][kT / 64];
    if (db)  // the Linear head's bias gradient, db[j] = sum_s dy[s][j], two outputs at a time
        for (int j = 0; j < O; j += 2) {
            const bool two = j + 1 < O;
            double b0 = 0.0, b1 = 0.0;
            for (int64_t i = threadIdx.x; i < n; i += kT) {
                b0 += (double)dy[i * O + j];
                if (two) b1 += (double)dy[i * O + j + 1];
            }
            block_sum2(b0, b1, red);
            if (threadIdx.x == 0) {
                db[j] = (float)b0;
                if (two) db[j + 1] = (float)b1;
            }
        }
    double a = 0.0, z = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += kT) a += part[i];
    block_sum2(a, z, red);
    if (threadIdx.x == 0) {
        const float loss = (float)(a / (double)(n * O));
        curve[ctl ? ctl->epoch : 0] = loss;
        if (validation && ctl) {
            if (loss < ctl->best) {
                ctl->best = loss;
                ctl->wait = 0;
            } else {
                ctl->wait += 1;
            }
            if (patience >= 0 && ctl->wait >= patience) ctl->reached = 1;
        }
    }
}

// dW[j][f] = sum_s dy[s][j] h[s][f], dh[s][f] = sum_j dy[s][j] W[j][f]: thread per feature and chunk of kFcChunk
// samples (fp64, samples in ascending order); k_fc_wfinal adds the chunks in chunk order
__global__ __launch_bounds__(kT) void k_fc_bwd(const Ctl* ctl, const float* __restrict__ h,
                                               const float* __restrict__ dy, int64_t n, int F, int O,
                                               const float* __restrict__ w, double* __restrict__ partial,
                                               float* __restrict__ dh) {
    OFP_CNN_STOPPED(ctl);
    const int f = blockIdx.x * kT + threadIdx.x, ck = blockIdx.y;
    if (f >= F) return;
    double acc[kMaxOut];
    float wj[kMaxOut];
#pragma unroll
    for (int j = 0; j < kMaxOut; ++j) acc[j] = 0.0, wj[j] = j < O ? w[(int64_t)j * F + f] : 0.0f;
    const int64_t s0 = (int64_t)ck * kFcChunk, s1 = s0 + kFcChunk < n ? s0 + kFcChunk : n;
    for (int64_t s = s0; s < s1; ++s) {
        const float hv = h[s * F + f];
        float d = 0.0f;
#pragma unroll
        for (int j = 0; j < kMaxOut; ++j)
            if (j < O) {
                const float g = dy[s * O + j];
                acc[j] += (double)g * (double)hv;
                d = fmaf(g, wj[j], d);
            }
        dh[s * F + f] = d;
    }
#pragma unroll
    for (int j = 0; j < kMaxOut; ++j)
        if (j < O) partial[((int64_t)ck * O + j) * F + f] = acc[j];
}

__global__ __launch_bounds__(kT) void k_fc_wfinal(const Ctl* ctl, const double* __restrict__ partial, int nchunk,
                                                  int64_t OF, float* __restrict__ dw) {
    OFP_CNN_STOPPED(ctl);
    const int64_t i = (int64_t)blockIdx.x * kT + threadIdx.x;
    if (i >= OF) return;
    double s = 0.0;
    for (int c = 0; c < nchunk; ++c) s += partial[(int64_t)c * OF + i];
    dw[i] = (float)s;
}

// the chain's last kernel: the epoch is over; stop once patience has run out and min_epochs are done
__global__ __launch_bounds__(kT) void k_epoch_end(Ctl* ctl, int min_epochs) {
    OFP_CNN_STOPPED(ctl);
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        ctl->epoch += 1;
        if (ctl->reached && ctl->epoch >= min_epochs) ctl->stop = 1;
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------

unsigned grid_for(int64_t total) {
    const int64_t g = ofp::cdiv(total, kT);
    return (unsigned)(g < 1 ? 1 : (g > (1 << 20) ? (1 << 20) : g));
}
int slabs_of(int64_t pairs) { return (int)ofp::cdiv(pairs, kSlab); }

int enqueue_conv_bwd(const Ctl* ctl, const Conv& c, int64_t n, const float* x, const float* w, const float* dz,
                     double* part, float* dw, float* db, float* dx, hipStream_t st) {
    const int nslab = slabs_of(n * c.wc), T = c.cin / c.groups * c.k + 1;
    hipLaunchKernelGGL(k_wgrad_partial, dim3(nslab, c.cout), dim3(kT), 0, st, ctl, c, n, x, dz, part);
    OFP_LAUNCH_CHECK("k_wgrad_partial");
    hipLaunchKernelGGL(k_wgrad_final, dim3((unsigned)ofp::cdiv(c.cout * T, kT)), dim3(kT), 0, st, ctl, part, nslab,
                       c.cout, T, dw, db);
    OFP_LAUNCH_CHECK("k_wgrad_final");
    if (dx) {
        hipLaunchKernelGGL(k_dgrad, dim3(grid_for(n * c.cin * c.win)), dim3(kT), 0, st, ctl, c, n, dz, w, dx);
        OFP_LAUNCH_CHECK("k_dgrad");
    }
    return OFP_OK;
}

// The Linear head of a batch: h [n][F], w [O][F], b [O], targets y [n][O]; `lpart` takes n doubles, `part` (backward)
// fc_chunks(n) * O * F doubles.
struct Fc {
    const float* h;
    int64_t n;
    int F, O;
    const float* w;
    const float* b;
    const float* y;
};

int fc_chunks(int64_t n) { return (int)ofp::cdiv(n, kFcChunk); }

// out = W h + b and the batch's mean loss into `curve` (slot `epoch` of it inside a run).  With dy (training):
// d loss / d out and the bias gradient db; without (validation, L1): the early-stop rule with `patience`.
int enqueue_fc_forward(Ctl* ctl, const Fc& f, int loss, float* out, float* dy, double* lpart, float* curve,
                       int patience, float* db, hipStream_t st) {
    const float inv_numel = 1.0f / (float)(f.n * f.O);
    hipLaunchKernelGGL(k_fc_fwd, dim3((unsigned)f.n), dim3(kT), 0, st, ctl, f.h, f.F, f.O, f.w, f.b, f.y,
                       dy ? loss : 0, inv_numel, out, dy, lpart);
    OFP_LAUNCH_CHECK("k_fc_fwd");
    hipLaunchKernelGGL(k_loss_final, dim3(1), dim3(kT), 0, st, ctl, lpart, f.n, f.O, curve, dy ? 0 : 1,
                       dy ? -1 : patience, (const float*)dy, dy ? db : (float*)nullptr);
    OFP_LAUNCH_CHECK("k_loss_final");
    return OFP_OK;
}

// dw = dy^T h (chunks of kFcChunk samples through `part`, added in chunk order) and dh = dy W
int enqueue_fc_backward(const Ctl* ctl, const Fc& f, const float* dy, double* part, float* dw, float* dh,
                        hipStream_t st) {
    const int nchunk = fc_chunks(f.n);
    hipLaunchKernelGGL(k_fc_bwd, dim3((unsigned)ofp::cdiv(f.F, kT), nchunk), dim3(kT), 0, st, ctl, f.h, dy, f.n, f.F,
                       f.O, f.w, part, dh);
    OFP_LAUNCH_CHECK("k_fc_bwd");
    hipLaunchKernelGGL(k_fc_wfinal, dim3((unsigned)ofp::cdiv((int64_t)f.O * f.F, kT)), dim3(kT), 0, st, ctl, part,
                       nchunk, (int64_t)f.O * f.F, dw);
    OFP_LAUNCH_CHECK("k_fc_wfinal");
    return OFP_OK;
}

int check_ws(const char* who, const void* ws, int64_t given, int64_t need) {
    if (ws == nullptr || given < need)
        return ofp::fail(OFP_ERR_WORKSPACE, "%s: work space of %lld bytes needed, %lld given", who, (long long)need,
                         (long long)given);
    return OFP_OK;
}

int conv_width(int w, int k, int padding, int dilation, int stride) {
    return (w + 2 * padding - dilation * (k - 1) - 1) / stride + 1;
}

// The stand-alone convolution backward of both trainers (ofp_conv1d_backward, ofp_conv1d_backward_strided): `need` is
// what the entry's own _workspace_bytes returns for the same shape, negative when its limits do not hold.
int64_t conv_bwd_bytes(int64_t n, int cin, int w, int cout, int k, int padding, int dilation, int groups, int stride) {
    return (int64_t)cout * (cin / groups * k + 1) * slabs_of(n * conv_width(w, k, padding, dilation, stride)) * 8;
}

int conv_bwd_alone(const char* who, int64_t need, const float* d_x, int64_t n, int cin, int w, const float* d_w,
                   int cout, int k, int padding, int dilation, int groups, int stride, const float* d_dz, float* d_dx,
                   float* d_dw, float* d_db, void* d_ws, int64_t ws_bytes, void* stream) {
    if (need < 0) return OFP_ERR_INVALID;
    OFP_REQUIRE(d_x && d_w && d_dz && d_dw && d_db, "%s: NULL argument", who);
    if (int rc = check_ws(who, d_ws, ws_bytes, need)) return rc;
    const Conv c{cin, cout, w, conv_width(w, k, padding, dilation, stride), k, padding, dilation, groups, stride};
    return enqueue_conv_bwd(nullptr, c, n, d_x, d_w, d_dz, (double*)d_ws, d_dw, d_db, d_dx, (hipStream_t)stream);
}

// ---- one epoch, its driver and the entries ---------------------------------------------------------------------------
// What a trainer supplies.
//   * Its Plan, derived from WsPlan: the dimensions, the parameter offsets and the byte offsets of its work-space blocks.
//     Parts that more than one trainer has plan themselves into it: ConvStack (csrc/ofp_cnn_stack.h) and AttnHead
//     (csrc/ofp_seq_train.h) take their blocks from the Plan's bump allocator, advance its parameter and statistics
//     counters and raise its partial-sum size.
//   * For Run<Plan>, found by overload: enqueue_forward(r, x, y, n, train, curve, patience), which ends in
//     enqueue_fc_forward; enqueue_backward(r, x, n); enqueue_step(r, rates), its optimiser; enqueue_reset(r), which zeroes
//     the optimiser's state in front of the first epoch.
//   * A traits struct T for the entry templates at the end of this file: Config and Plan (types), train and grads (the
//     names of the public training and loss-and-gradients entries, as messages give them), env (the variable that turns
//     graph capture off), window_of(cfg) -> Window, and make_plan(who, cfg, n, n_val, plan, rnd).
// The extern "C" functions of a trainer are one-line forwards into the entry templates.

// base of a Plan: the byte offsets of the work space's blocks come from a bump allocator.  Every block is rounded up on
// its own, so the size does not depend on the order in which the parts take theirs.
struct WsPlan {
    int64_t bytes;  // taken so far; in the end the work space's size
    int np, ns;     // packed parameters; packed running statistics (0: the model has none)
    int64_t o_G, o_RS, o_ctl, o_X;  // gradients, scratch running statistics (ns > 0), Ctl, the epoch's windows (a source)
    int64_t take(int64_t n) {
        const int64_t at = bytes;
        bytes += ofp::align_up(n > 0 ? n : 1, 256);
        return at;
    }
};

// base of a Run: the work space itself
struct WsRun {
    char* ws;
    template <class T>
    T* at(int64_t off) const {
        return reinterpret_cast<T*>(ws + off);
    }
};

// The random options of a run are csrc/ofp_train_random.h's Random.  That header builds on this one (its kernels take
// Ctl and kT), so the type is only declared here and enters Run as a defaulted template parameter: it is complete where
// a trainer instantiates Run and the templates below, and make_random / enqueue_windows are found there by their
// Random argument.
struct Random;

template <class Plan, class Rnd = Random>
struct Run : WsRun {
    const Plan* p;
    float* P;    // packed parameters
    float* RS;   // packed running statistics; NULL where the model has none
    float* G;    // packed gradients
    Ctl* ctl;    // NULL: a single pass, epoch 0 (rnd.st.epoch for the random stream)
    hipStream_t st;
    Rnd rnd;     // the model's dropouts and the window source; all off by default
};

// what a configuration's windows look like to the window source
struct Window {
    int channels, width;
};

struct TrainArgs {
    const float* x;
    const float* y;
    int64_t n;
    const float* xv;
    const float* yv;
    int64_t nv;
    const float* rates;
    int min_epochs, patience;
    float* train_loss;
    float* val_loss;
};

int check_train(const char* who, const TrainArgs& a, int num_epochs, const float* params, const int32_t* h_epochs) {
    OFP_REQUIRE(num_epochs >= 1 && a.min_epochs >= 0, "%s: num_epochs %d, min_epochs %d", who, num_epochs,
                a.min_epochs);
    OFP_REQUIRE(a.x && a.y && a.rates && params && a.train_loss && h_epochs, "%s: NULL argument", who);
    OFP_REQUIRE(a.nv == 0 || (a.xv && a.yv && a.val_loss), "%s: NULL validation argument", who);
    OFP_REQUIRE(a.patience < 0 || a.nv > 0, "%s: patience needs a validation set", who);
    return OFP_OK;
}

// training forward, the batch's mean loss into `loss` (slot `epoch` of it inside a run) and backward
template <class Run>
int enqueue_loss_grads(const Run& r, const float* x, const float* y, int64_t n, float* loss) {
    if (int rc = enqueue_forward(r, x, y, n, true, loss, -1)) return rc;
    return enqueue_backward(r, x, n);
}

template <class Run>
int enqueue_epoch(const Run& r, const TrainArgs& a) {
    const auto& p = *r.p;
    if (r.rnd.windows)  // a.x is the work space's window buffer
        if (int rc = enqueue_windows(r.ctl, r.rnd, r.template at<float>(p.o_X), r.st)) return rc;
    if (int rc = enqueue_loss_grads(r, a.x, a.y, a.n, a.train_loss)) return rc;
    if (int rc = enqueue_step(r, a.rates)) return rc;
    if (a.nv > 0)
        if (int rc = enqueue_forward(r, a.xv, a.yv, a.nv, false, a.val_loss, a.patience)) return rc;
    hipLaunchKernelGGL(k_epoch_end, dim3(1), dim3(kT), 0, r.st, r.ctl, a.min_epochs);
    OFP_LAUNCH_CHECK("k_epoch_end");
    return OFP_OK;
}

// the captured epoch and its executable form: freed on every way out of run_epochs
struct EpochGraph {
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    ~EpochGraph() {
        if (exec) (void)hipGraphExecDestroy(exec);
        if (graph) (void)hipGraphDestroy(graph);
    }
};

// Up to num_epochs epochs on `st`: the first launched plainly, the others as replays of its captured graph (plain
// launches too when the environment has `env`=nodes), until the device's stop word is seen; the epochs run go to
// *h_epochs.  `reset` enqueues the zeroing of the optimiser's state, `epoch` one epoch.
template <class Reset, class Epoch>
int run_epochs(const char* who, const char* env, hipStream_t st, Ctl* ctl, int num_epochs, int patience,
               int32_t* h_epochs, Reset reset, Epoch epoch) {
    const char* mode = getenv(env);
    const bool plain = mode != nullptr && std::strcmp(mode, "nodes") == 0;
    OFP_REQUIRE(plain || st != nullptr,
                "%s: the epoch graph cannot be captured on the null stream (pass a created stream, or set %s=nodes for "
                "plain launches)",
                who, env);
    if (int rc = reset()) return rc;
    hipLaunchKernelGGL(k_init, dim3(1), dim3(kT), 0, st, ctl);
    OFP_LAUNCH_CHECK("k_init");
    // the first epoch is launched plainly: it loads every code object and sets the LDS size of kernels that need more
    // than the default (the LCCCNN's head, k_stretch_windows at long windows), neither of which may happen during capture
    if (int rc = epoch()) return rc;
    EpochGraph g;
    if (!plain && num_epochs > 1) {
        OFP_HIP(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
        const int rc = epoch();
        const hipError_t ce = hipStreamEndCapture(st, &g.graph);
        if (rc != OFP_OK) return rc;
        if (ce != hipSuccess) return ofp::fail(OFP_ERR_HIP, "hipStreamEndCapture failed: %s", hipGetErrorString(ce));
        const hipError_t ie = hipGraphInstantiate(&g.exec, g.graph, nullptr, nullptr, 0);
        if (ie != hipSuccess) return ofp::fail(OFP_ERR_HIP, "hipGraphInstantiate failed: %s", hipGetErrorString(ie));
    }
    int rc = OFP_OK;
    Ctl seen{};
    for (int e = 1; e < num_epochs && rc == OFP_OK; ++e) {
        if (patience >= 0 && e % kCheckEvery == 0) {  // has the device stopped?  (at most once per 64 epochs)
            hipError_t he = hipMemcpyAsync(&seen, ctl, sizeof(Ctl), hipMemcpyDeviceToHost, st);
            if (he == hipSuccess) he = hipStreamSynchronize(st);
            if (he != hipSuccess) {
                rc = ofp::fail(OFP_ERR_HIP, "%s: %s", who, hipGetErrorString(he));
                break;
            }
            if (seen.stop) break;
        }
        if (g.exec) {
            const hipError_t he = hipGraphLaunch(g.exec, st);
            if (he != hipSuccess) rc = ofp::fail(OFP_ERR_HIP, "hipGraphLaunch failed: %s", hipGetErrorString(he));
        } else {
            rc = epoch();
        }
    }
    hipError_t he = hipMemcpyAsync(&seen, ctl, sizeof(Ctl), hipMemcpyDeviceToHost, st);
    if (he == hipSuccess) he = hipStreamSynchronize(st);
    if (rc != OFP_OK) return rc;
    if (he != hipSuccess) return ofp::fail(OFP_ERR_HIP, "%s: %s", who, hipGetErrorString(he));
    *h_epochs = seen.epoch;
    return OFP_OK;
}

// ---- the public entries ------------------------------------------------------------------------------------------------
// Refusals come in this order: config, random options, plan, arguments, statistics, work space.

// a training call's random options into r.rnd, then its plan
template <class T>
int plan_train(const typename T::Config* cfg, int64_t n, int64_t n_val, const ofp_train_random* random, int span,
               typename T::Plan& p, Run<typename T::Plan>& r) {
    OFP_REQUIRE(cfg != nullptr, "%s: config is NULL", T::train);
    const Window w = T::window_of(*cfg);
    if (int rc = make_random(T::train, random, span, n, w.channels, w.width, true, r.rnd)) return rc;
    return T::make_plan(T::train, cfg, n, n_val, p, r.rnd);
}

template <class T>
int64_t train_workspace_bytes(const typename T::Config* cfg, int64_t n, int64_t n_val, const ofp_train_random* random,
                              int span) {
    typename T::Plan p;
    Run<typename T::Plan> r{};
    return plan_train<T>(cfg, n, n_val, random, span, p, r) ? -1 : p.bytes;
}

// d_stats is NULL for a model without running statistics
template <class T>
int train_entry(const typename T::Config* cfg, int64_t n, const float* d_x, const float* d_y, int64_t n_val,
                const float* d_x_val, const float* d_y_val, const float* d_rates, int num_epochs, int min_epochs,
                int patience, float* d_params, float* d_stats, float* d_train_loss, float* d_val_loss,
                int32_t* h_epochs, void* d_ws, int64_t ws_bytes, void* stream, const ofp_train_random* random,
                int span) {
    typename T::Plan p;
    Run<typename T::Plan> r{};
    if (int rc = plan_train<T>(cfg, n, n_val, random, span, p, r)) return rc;
    if (r.rnd.windows && d_ws) d_x = reinterpret_cast<const float*>((const char*)d_ws + p.o_X);
    const TrainArgs a{d_x, d_y, n, d_x_val, d_y_val, n_val, d_rates, min_epochs, patience, d_train_loss, d_val_loss};
    if (int rc = check_train(T::train, a, num_epochs, d_params, h_epochs)) return rc;
    OFP_REQUIRE(p.ns == 0 || d_stats, "%s: BatchNorm statistics are NULL", T::train);
    if (int rc = check_ws(T::train, d_ws, ws_bytes, p.bytes)) return rc;
    r.ws = (char*)d_ws, r.p = &p, r.P = d_params, r.RS = d_stats, r.st = (hipStream_t)stream;
    r.G = r.template at<float>(p.o_G);
    r.ctl = r.template at<Ctl>(p.o_ctl);
    return run_epochs(
        T::train, T::env, r.st, r.ctl, num_epochs, patience, h_epochs, [&] { return enqueue_reset(r); },
        [&] { return enqueue_epoch(r, a); });
}

// the trainer's own forward and backward on the caller's batch; the running statistics it would update are a scratch copy
template <class T>
int loss_grads_entry(const typename T::Config* cfg, int64_t n, const float* d_x, const float* d_y,
                     const float* d_params, float* d_loss, float* d_grads, void* d_ws, int64_t ws_bytes, void* stream,
                     const ofp_train_random* random) {
    typename T::Plan p;
    Run<typename T::Plan> r{};
    if (int rc = make_random(T::grads, random, 0, n, 0, 0, false, r.rnd)) return rc;
    if (int rc = T::make_plan(T::grads, cfg, n, 0, p, r.rnd)) return rc;
    OFP_REQUIRE(d_x && d_y && d_params && d_loss && d_grads, "%s: NULL argument", T::grads);
    if (int rc = check_ws(T::grads, d_ws, ws_bytes, p.bytes)) return rc;
    r.ws = (char*)d_ws, r.p = &p, r.P = const_cast<float*>(d_params), r.G = d_grads, r.st = (hipStream_t)stream;
    if (p.ns > 0) {
        r.RS = r.template at<float>(p.o_RS);
        OFP_HIP(hipMemsetAsync(r.RS, 0, (size_t)p.ns * 4, r.st));
    }
    return enqueue_loss_grads(r, d_x, d_y, n, d_loss);
}

}  // namespace
