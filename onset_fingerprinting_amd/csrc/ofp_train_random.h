// The random stream of the two epoch-graph trainers: Philox4x32-10 keyed by the user's seed, with the counter
// (index / 4, site, epoch, 0) and output word index % 4.  The epoch is read from the run's control block on the device,
// so a replayed graph draws a new mask and new shifts at every launch without any argument changing; without a
// control block (the stand-alone forms and the loss-and-gradients functions) it is an argument.  Nothing is stored: any
// mask, shift or stretch can be recomputed from (seed, epoch, index).  Site 0 is the dropout in front of the Linear
// head, site 1 the shift of the training windows, site 2 their stretch.  Site 3 is the dropout on the attention's softmax
// probabilities in csrc/ofp_cnnrnn_train.hip, where site 0 is the dropout on the conv features in front of the GRU.
// Site 4 is nn.GRU's dropout between the recurrent layers in csrc/ofp_rnn_train.hip, which has site 3 too.
// File-local like ofp_train_chain.h, which it builds on.
#pragma once
#include "ofp_resample_dev.h"
#include "ofp_train_chain.h"

#include <cstdint>

namespace {

constexpr uint32_t kSiteDropout = 0, kSiteShift = 1, kSiteStretch = 2;

struct Words {
    uint32_t w[4];
};

__host__ __device__ __forceinline__ Words philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3,
                                                        uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c0 = n0, c1 = (uint32_t)p1, c2 = n2, c3 = (uint32_t)p0;
        k0 += 0x9E3779B9u, k1 += 0xBB67AE85u;
    }
    return Words{{c0, c1, c2, c3}};
}

// what a kernel needs of the stream: the key, and the epoch to use when there is no control block
struct Stream {
    uint32_t k0, k1, epoch;
};

__device__ __forceinline__ Words stream_words(const Ctl* ctl, const Stream& r, uint32_t q, uint32_t site) {
    return philox4x32_10(q, site, ctl ? (uint32_t)ctl->epoch : r.epoch, 0u, r.k0, r.k1);
}

// Inverted dropout over `total` consecutive values: element i is dropped iff word i < T and is scaled by s where
// kept; a thread draws once for the four elements 4q .. 4q + 3.  h == nullptr stands for all ones (the mask itself);
// h == out is the in-place form of the backward.  Whole float4 where both pointers are 16-byte aligned and the four
// elements exist, single elements otherwise.
__device__ __forceinline__ void dropout4(const Ctl* ctl, const Stream& r, uint32_t T, float s, const float* h,
                                         float* out, int64_t total, bool aligned, int64_t q) {
    const Words d = stream_words(ctl, r, (uint32_t)q, kSiteDropout);
    const int64_t i0 = q * 4;
    if (aligned && i0 + 4 <= total) {
        float4 v = h ? *reinterpret_cast<const float4*>(h + i0) : float4{1.0f, 1.0f, 1.0f, 1.0f};
        v.x = d.w[0] < T ? 0.0f : v.x * s;
        v.y = d.w[1] < T ? 0.0f : v.y * s;
        v.z = d.w[2] < T ? 0.0f : v.z * s;
        v.w = d.w[3] < T ? 0.0f : v.w * s;
        *reinterpret_cast<float4*>(out + i0) = v;
    } else {
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (i0 + u < total) out[i0 + u] = d.w[u] < T ? 0.0f : (h ? h[i0 + u] : 1.0f) * s;
    }
}

__global__ __launch_bounds__(kT) void k_dropout_fwd(const Ctl* ctl, const Stream r, uint32_t T, float s,
                                                    const float* h, float* hd, int64_t total) {
    OFP_CNN_STOPPED(ctl);
    const bool aligned = (((uintptr_t)h | (uintptr_t)hd) & 15) == 0;
    const int64_t quads = (total + 3) / 4;
    for (int64_t q = (int64_t)blockIdx.x * kT + threadIdx.x; q < quads; q += (int64_t)gridDim.x * kT)
        dropout4(ctl, r, T, s, h, hd, total, aligned, q);
}

// dh = dhd * s where kept, 0 where dropped, in place
__global__ __launch_bounds__(kT) void k_dropout_bwd(const Ctl* ctl, const Stream r, uint32_t T, float s, float* dh,
                                                    int64_t total) {
    OFP_CNN_STOPPED(ctl);
    const bool aligned = ((uintptr_t)dh & 15) == 0;
    const int64_t quads = (total + 3) / 4;
    for (int64_t q = (int64_t)blockIdx.x * kT + threadIdx.x; q < quads; q += (int64_t)gridDim.x * kT)
        dropout4(ctl, r, T, s, dh, dh, total, aligned, q);
}

// where the training windows come from: interleaved audio [N][C], one start per onset (minimum onset of the hit less
// pre_samples), R extractions of each, every one shifted by up to +-m samples and, with a span S >= 2, cut
// 1 .. S - 1 samples longer or shorter and resampled to W
struct Windows {
    const float* audio;
    int64_t N;
    const int64_t* starts;
    int O, R, C, W, m, S;
};

__device__ __forceinline__ int shift_of_word(uint32_t word, int m) {
    return (int)(((uint64_t)word * (uint32_t)(2 * m + 1)) >> 32) - m;
}

__device__ __forceinline__ int shift_of(const Ctl* ctl, const Stream& r, int item, int m) {
    const Words d = stream_words(ctl, r, (uint32_t)item >> 2, kSiteShift);
    return shift_of_word(d.w[item & 3], m);
}

// x[j][c][t] = audio[starts[j % O] + shift_j + t][c] for item j = r * O + i: thread per (item, t) reads the C adjacent
// samples of one audio row and writes C values, each store coalesced along t.  A row outside the audio (the callers
// rule it out) reads as 0.
__global__ __launch_bounds__(kT) void k_shift_windows(const Ctl* ctl, const Stream r, const Windows w,
                                                      float* __restrict__ x, int32_t* __restrict__ shifts) {
    OFP_CNN_STOPPED(ctl);
    const int64_t total = (int64_t)w.O * w.R * w.W;
    for (int64_t i = (int64_t)blockIdx.x * kT + threadIdx.x; i < total; i += (int64_t)gridDim.x * kT) {
        const int t = (int)(i % w.W);
        const int item = (int)(i / w.W);
        const int sh = w.m > 0 ? shift_of(ctl, r, item, w.m) : 0;
        if (shifts != nullptr && t == 0) shifts[item] = sh;
        const int64_t row = w.starts[item % w.O] + sh + t;
        const bool inside = row >= 0 && row < w.N;
        const float* src = w.audio + row * w.C;
        float* dst = x + (int64_t)item * w.C * w.W + t;
        for (int c = 0; c < w.C; ++c) dst[(int64_t)c * w.W] = inside ? src[c] : 0.0f;
    }
}

// uniform on {-(S-1), ..., -1, 1, ..., S-1}: the reference's randint(1, S) * choice((-1, 1)), never 0
__device__ __forceinline__ int stretch_of_word(uint32_t word, int S) {
    const int v = (int)(((uint64_t)word * (uint32_t)(2 * (S - 1))) >> 32);
    return v < S - 1 ? v - (S - 1) : v - (S - 1) + 1;
}

// output word item % 4 by selects: k_stretch_windows indexes with the workgroup's number, and a register array indexed
// by a value the compiler takes for variable goes through scratch memory
__device__ __forceinline__ uint32_t item_word(const Words& d, int item) {
    const int u = item & 3;
    return u == 0 ? d.w[0] : u == 1 ? d.w[1] : u == 2 ? d.w[2] : d.w[3];
}

// The stretched form of k_shift_windows: item j reads Nx_j = W + stretch_j rows from row starts[j % O] + shift_j and
// every channel of them is resampled to W samples, to the bits ofp_resample_windows gives for the same rows
// (csrc/ofp_resample_dev.h).  One workgroup per item: the rows are copied to LDS as they lie in the audio ([Nx][C]),
// the two twiddle tables are computed once for all C channels, and the (bin, channel) and then the (sample, channel)
// pairs go round the kT threads, in both rounds with the channel on adjacent lanes: they read one twiddle (a
// broadcast) and C adjacent samples or bins.  With the samples on adjacent lanes instead, the 16 lanes that a 16-byte
// LDS read serves per cycle would take twy at a stride of k entries, an up-to-16-way bank conflict at every even k
// (3 x the cycles on average over k); the price is stores in runs of 64 / C lanes per channel row.
// LDS: twx [max_nx] | twy [W] | Y [W / 2 + 1][C] | rows [max_nx][C], sized by the host for max_nx = W + S - 1; Nx is
// clamped to it.
__global__ __launch_bounds__(kT) void k_stretch_windows(const Ctl* ctl, const Stream r, const Windows w, int max_nx,
                                                        float* __restrict__ x, int32_t* __restrict__ shifts,
                                                        int32_t* __restrict__ stretches) {
    OFP_CNN_STOPPED(ctl);
    extern __shared__ __align__(16) unsigned char stretch_smem[];
    const int item = blockIdx.x, C = w.C, W = w.W;
    const int sh =
        w.m > 0 ? shift_of_word(item_word(stream_words(ctl, r, (uint32_t)item >> 2, kSiteShift), item), w.m) : 0;
    const int sd = stretch_of_word(item_word(stream_words(ctl, r, (uint32_t)item >> 2, kSiteStretch), item), w.S);
    const int Nx = max(1, min(W + sd, max_nx));  // (the host checks S <= W; never overrun the LDS)
    const int K = resample_bins(Nx, W);
    double2* twx = reinterpret_cast<double2*>(stretch_smem);
    double2* twy = twx + max_nx;
    double2* Y = twy + W;
    float* rows = reinterpret_cast<float*>(Y + C * (W / 2 + 1));
    if (threadIdx.x == 0) {
        if (shifts != nullptr) shifts[item] = sh;
        if (stretches != nullptr) stretches[item] = sd;
    }
    const int64_t row0 = w.starts[item % w.O] + sh;
    const float* src = w.audio + row0 * C;
    for (int i = threadIdx.x; i < Nx * C; i += kT) {
        const int64_t row = row0 + i / C;
        rows[i] = (row >= 0 && row < w.N) ? src[i] : 0.0f;
    }
    for (int j = threadIdx.x; j < Nx; j += kT) twx[j] = resample_twx(j, Nx);
    for (int j = threadIdx.x; j < W; j += kT) twy[j] = resample_twy(j, W);
    __syncthreads();
    for (int p = threadIdx.x; p < (K + 1) * C; p += kT) {
        const int k = p / C, c = p - k * C;
        Y[p] = resample_bin(rows + c, C, twx, Nx, W, k);
    }
    __syncthreads();
    float* dst = x + (int64_t)item * C * W;
    for (int p = threadIdx.x; p < C * W; p += kT) {
        const int m = p / C, c = p - m * C;
        dst[c * W + m] = resample_sample(Y + c, C, twy, Nx, W, m);
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------

constexpr int kMaxStretched = 2048;              // the resampler's longest window (ofp_resample_windows)
constexpr size_t kStretchMaxLds = 160 * 1024;    // of a gfx950 compute unit

size_t stretch_lds(int C, int W, int max_nx) {
    return (size_t)(max_nx + W + (size_t)C * (W / 2 + 1)) * 16 + (size_t)max_nx * C * 4;
}

ofp::LdsAttrCache g_stretch_attr;

// the random options of a run, checked and turned into what the kernels take
struct Random {
    bool drop = false, windows = false;
    Stream st{0, 0, 0};
    uint32_t T = 0;
    float s = 1.0f;
    Windows w{};
};

int make_random(const char* who, const ofp_train_random* o, int stretch_span, int64_t n, int channels, int width,
                bool allow_windows, Random& r) {
    r = Random{};
    OFP_REQUIRE(stretch_span == 0 || stretch_span >= 2,
                "%s: stretch span %d (0: no stretch; from 2: stretches of 1 .. span - 1 samples; 1 leaves nothing to "
                "draw, the reference's randint(1, 1) raises)",
                who, stretch_span);
    OFP_REQUIRE(stretch_span == 0 || (o != nullptr && o->n_extractions > 0),
                "%s: a stretch span of %d needs a window source", who, stretch_span);
    if (o == nullptr) return OFP_OK;
    OFP_REQUIRE(o->dropout_p >= 0.0 && o->dropout_p < 1.0, "%s: dropout p %g (0 <= p < 1)", who, o->dropout_p);
    OFP_REQUIRE(o->epoch >= 0 && o->max_shift >= 0 && o->n_extractions >= 0,
                "%s: epoch %d, max_shift %d, n_extractions %d", who, o->epoch, o->max_shift, o->n_extractions);
    r.st = Stream{(uint32_t)(o->seed & 0xffffffffu), (uint32_t)(o->seed >> 32), (uint32_t)o->epoch};
    r.drop = o->dropout_p > 0.0;
    r.T = (uint32_t)(o->dropout_p * 4294967296.0);
    r.s = (float)(1.0 / (1.0 - o->dropout_p));
    if (o->n_extractions > 0) {
        OFP_REQUIRE(allow_windows, "%s: takes the windows themselves, not a window source", who);
        OFP_REQUIRE(o->d_audio && o->d_starts, "%s: the window source's audio or starts are NULL", who);
        OFP_REQUIRE(o->n_onsets >= 1 && o->n_onsets * o->n_extractions == n,
                    "%s: %lld onsets x %d extractions are not the batch of %lld", who, (long long)o->n_onsets,
                    o->n_extractions, (long long)n);
        OFP_REQUIRE(o->audio_channels == channels, "%s: audio of %d channels for a model of %d", who,
                    o->audio_channels, channels);
        OFP_REQUIRE(o->max_shift <= (1 << 20) && o->audio_len >= (int64_t)width + 2 * o->max_shift,
                    "%s: audio of %lld samples for windows of %d shifted by up to %d", who, (long long)o->audio_len,
                    width, o->max_shift);
        if (stretch_span > 0) {
            OFP_REQUIRE(stretch_span <= width && width + stretch_span - 1 <= kMaxStretched,
                        "%s: windows of %d samples stretched by up to %d (limits: span <= width, width + span - 1 <= "
                        "%d)",
                        who, width, stretch_span - 1, kMaxStretched);
            OFP_REQUIRE(o->audio_len >= (int64_t)width + 2 * o->max_shift + stretch_span - 1,
                        "%s: audio of %lld samples for windows of %d shifted by up to %d and stretched by up to %d",
                        who, (long long)o->audio_len, width, o->max_shift, stretch_span - 1);
            OFP_REQUIRE(stretch_lds(channels, width, width + stretch_span - 1) <= kStretchMaxLds,
                        "%s: stretched windows of %d channels and %d samples need %lld bytes of LDS (limit: %lld)", who,
                        channels, width, (long long)stretch_lds(channels, width, width + stretch_span - 1),
                        (long long)kStretchMaxLds);
        }
        r.windows = true;
        r.w = Windows{o->d_audio, o->audio_len, o->d_starts, (int)o->n_onsets, o->n_extractions, channels, width,
                      o->max_shift, stretch_span};
    }
    return OFP_OK;
}

unsigned quad_grid(int64_t total) { return grid_for((total + 3) / 4); }

int enqueue_dropout_fwd(const Ctl* ctl, const Random& r, const float* h, float* hd, int64_t total, hipStream_t st) {
    hipLaunchKernelGGL(k_dropout_fwd, dim3(quad_grid(total)), dim3(kT), 0, st, ctl, r.st, r.T, r.s, h, hd, total);
    OFP_LAUNCH_CHECK("k_dropout_fwd");
    return OFP_OK;
}

int enqueue_dropout_bwd(const Ctl* ctl, const Random& r, float* dh, int64_t total, hipStream_t st) {
    hipLaunchKernelGGL(k_dropout_bwd, dim3(quad_grid(total)), dim3(kT), 0, st, ctl, r.st, r.T, r.s, dh, total);
    OFP_LAUNCH_CHECK("k_dropout_bwd");
    return OFP_OK;
}

int enqueue_shift_windows(const Ctl* ctl, const Random& r, float* x, int32_t* shifts, hipStream_t st) {
    const int64_t total = (int64_t)r.w.O * r.w.R * r.w.W;
    hipLaunchKernelGGL(k_shift_windows, dim3(grid_for(total)), dim3(kT), 0, st, ctl, r.st, r.w, x, shifts);
    OFP_LAUNCH_CHECK("k_shift_windows");
    return OFP_OK;
}

// the windows of a source that stretches (r.w.S >= 2); the first call of a shape may set the kernel's LDS size and so
// has to come outside a capture (run_epochs launches the first epoch plainly)
int enqueue_stretch_windows(const Ctl* ctl, const Random& r, float* x, int32_t* shifts, int32_t* stretches,
                            hipStream_t st) {
    const int max_nx = r.w.W + r.w.S - 1;
    const size_t lds = stretch_lds(r.w.C, r.w.W, max_nx);
    if (int rc = ofp::ensure_dynamic_lds(reinterpret_cast<const void*>(k_stretch_windows), lds, g_stretch_attr))
        return rc;
    hipLaunchKernelGGL(k_stretch_windows, dim3((unsigned)(r.w.O * r.w.R)), dim3(kT), lds, st, ctl, r.st, r.w, max_nx, x,
                       shifts, stretches);
    OFP_LAUNCH_CHECK("k_stretch_windows");
    return OFP_OK;
}

// the epoch's windows, by the kernel the source asks for
int enqueue_windows(const Ctl* ctl, const Random& r, float* x, hipStream_t st) {
    return r.w.S > 0 ? enqueue_stretch_windows(ctl, r, x, nullptr, nullptr, st)
                     : enqueue_shift_windows(ctl, r, x, nullptr, st);
}

}  // namespace
