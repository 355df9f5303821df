// The random stream of the two epoch-graph trainers: Philox4x32-10 keyed by the user's seed, with the counter
// (index / 4, site, epoch, 0) and output word index % 4.  The epoch is read from the run's control block on the device,
// so a replayed graph draws a new mask and new shifts at every launch without any argument changing; without a
// control block (the stand-alone forms and the loss-and-gradients functions) it is an argument.  Nothing is stored: any
// mask or shift can be recomputed from (seed, epoch, index).  Site 0 is the dropout in front of the Linear head,
// site 1 the shift of the training windows.  File-local like ofp_train_chain.h, which it builds on.
#pragma once
#include "ofp_train_chain.h"

#include <cstdint>

namespace {

constexpr uint32_t kSiteDropout = 0, kSiteShift = 1;

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
// pre_samples), R extractions of each, every one shifted by up to +-m samples
struct Windows {
    const float* audio;
    int64_t N;
    const int64_t* starts;
    int O, R, C, W, m;
};

__device__ __forceinline__ int shift_of(const Ctl* ctl, const Stream& r, int item, int m) {
    const Words d = stream_words(ctl, r, (uint32_t)item >> 2, kSiteShift);
    return (int)(((uint64_t)d.w[item & 3] * (uint32_t)(2 * m + 1)) >> 32) - m;
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

// ---- host side ------------------------------------------------------------------------------------------------------

// the random options of a run, checked and turned into what the kernels take
struct Random {
    bool drop = false, windows = false;
    Stream st{0, 0, 0};
    uint32_t T = 0;
    float s = 1.0f;
    Windows w{};
};

int make_random(const char* who, const ofp_train_random* o, int64_t n, int channels, int width, bool allow_windows,
                Random& r) {
    r = Random{};
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
        r.windows = true;
        r.w = Windows{o->d_audio, o->audio_len, o->d_starts, (int)o->n_onsets, o->n_extractions, channels, width,
                      o->max_shift};
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

}  // namespace
