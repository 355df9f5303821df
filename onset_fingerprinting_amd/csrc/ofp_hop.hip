// Per-hop streaming session (BASELINE config 5): the reference's realtime call pattern
//
//   PortAudio callback (realtime/audio.py:81-120): ring-buffer write (:97) -> AmplitudeOnsetDetector
//   on the hop (:62-74, detection.py:727-798) -> classifier (multilateration.py:555-557 ->
//   calibration.py:552-560), and the per-hop spectral frame of the trailing n_fft samples
//   (realtime/recording.py:273-280)
//
// as ONE captured hipGraph per hop on a device-resident ring buffer:
//
//   H2D of the hop (B x C floats, pinned)  ->  k_hop_begin (hop counter, onset count = 0)
//   ->  k_stream (the detector, csrc/ofp_stream.hip: state in HBM)
//   ->  k_hop_spectral (one workgroup per channel: ring write, Hann x trailing n_fft samples,
//       rFFT, |X|^2, mel bands, the whole FCNN -- nothing but mel + logits leaves the chip)
//   ->  D2H of one packed result block {count, records, logits, mel, rel}.
//
// Fused form (default whenever the detector fits one workgroup): the five nodes above collapse into ONE
// kernel node, k_hop_fused -- workgroup 0 runs the detector while workgroups 1..C run the spectral
// branch, the hop is read from and the result block written to pinned host memory directly.
//
// With a locator attached (ofp_hop_set_locator, or ofp_hop_set_locator_2d for the planar Multilaterate, which runs
// loc_feed's planar instantiation in the same stage) the hop also carries Multilaterate3D.locate (ofp_locate_dev.h):
// the detector's workgroup (fused form) or one more kernel node after the detector (nodes form) feeds the hop's onsets,
// sorted by sample, to the device-resident state and writes the location block next to the records.  A hop without
// onsets takes one uniform branch on the count and touches nothing of the stage.
//
// With a regressor attached (ofp_hop_set_regressor) the same workgroup / one more node then runs the window regressor's
// step (ofp_regress_dev.h): the hop's onsets go through the grouping state machine, and the group whose window the hop
// completes goes through the model; a hop with nothing to feed, close or evaluate takes uniform branches only.
//
// With the voting locator attached (ofp_hop_set_locator_paired; a session's only stage) the workgroup / one node runs
// MultilateratePaired.locate_cc's stage (ofp_paired_dev.h): the regressor's grouping state machine, then the lag search
// and the vote on the window of the group that is due.
//
// A replay needs no argument update: the write cursor is a counter in device memory.  The frame the
// spectral kernel computes for the hop that ends at sample e is bit-identical to frame (e - n_fft)/B
// of the dense kernel (k_stft_power, hop = B) on the same stream: same tables, same FFT, same mel
// and classifier epilogue.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "ofp_detector.h"
#include "ofp_fft.h"
#include "ofp_locate_dev.h"
#include "ofp_mlp.h"
#include "ofp_paired_dev.h"
#include "ofp_regress_dev.h"
#include "ofp_stream_dev.h"

using namespace ofpfft;

namespace {

// Per-hop onset strength of the channel mean (realtime/recording.py:273-311, RecAnalysis.fft +
// onset_strength): symmetric float32 Hann x mean over channels of audio[-n_fft:], rFFT, |X|^2 in dB floored 80 dB
// below a tracked maximum, positive flux against the previous frame averaged over the bins, normalised by a
// tracked min / max, moving max / mean over the last frames.  The two trackers are loopmate.EMA_MinMaxTracker
// objects -- loopmate is not available, their arithmetic is ASSUMED to be that of envelope_follower.c:27-57
// with one alpha (PARITY UNPINNED).
struct StrengthArgs {
    int enabled, n_ring, max_length, avg_length;
    float ls_alpha, ls_minmax, oe_alpha, oe_minmin;
    const float* wsym;  // [F] scipy.signal.windows.hann(F) as float32
    float* prev;        // [F/2+1] power spectrum of the previous hop's frame
    float* st;          // [4] ls_max, oe_min, oe_max
    float* ring;        // [n_ring] normalised onset envelope, one entry per hop
    float* out;         // [4 + tg_len] raw flux, normalised, moving max, moving mean, then the tempogram (result block)
    int tg_len;         // tempogram window (realtime/recording.py:313-327), 0: off
    const float* tgw;   // [tg_len] scipy.signal.windows.hann(tg_len) as float32
};

struct HopArgs {
    StrengthArgs sg;
    int C, B, n_mels, nnz;
    int64_t R;             // rows of the ring buffer
    int64_t* ctl;          // [0] hops pushed so far (incremented by k_hop_begin), [1] spare
    const float* hop;      // [B][C] the hop just uploaded
    float* ring;           // [R][C]
    const float2* twM;     // precomputed once per session by k_hop_tables (the same values
    const float2* twF;     // k_stft_power builds in LDS)
    const float* win;
    const int32_t *flo, *flen, *foff;
    const float* fw;
    MlpPlan plan;          // n_layers == 0: no classifier
    float* logits;         // [C][n_out]
    float* mel;            // [C][n_mels]
    int64_t* count;        // onset count of the hop (zeroed by k_hop_begin)
    int64_t* hop_index;    // result header: index of the hop this block belongs to
    volatile int64_t* done_flag;  // fused form: hops completed, written to pinned host memory by the workgroup that
                                  // finishes last, after every result of the hop (the host polls it)
};

__global__ void k_hop_begin(HopArgs a) {
    if (threadIdx.x == 0) {
        const int64_t h = a.ctl[0];
        a.ctl[0] = h + 1;
        *a.count = 0;
        *a.hop_index = h;
    }
}

template <int F>
__global__ void k_hop_tables(float2* twM, float2* twF, float* win, float* wsym) {
    build_tables<F>(twM, twF, nullptr, F);
    // the periodic Hann exactly as k_stft_power holds it: F/2 + 1 computed entries, mirrored above
    for (int n = threadIdx.x; n <= F / 2; n += blockDim.x) win[n] = (float)(0.5 - 0.5 * cospi(2.0 * (double)n / (double)F));
    __syncthreads();
    for (int n = F / 2 + 1 + threadIdx.x; n < F; n += blockDim.x) win[n] = win[F - n];
    for (int n = threadIdx.x; n < F; n += blockDim.x)  // symmetric Hann (recording.py:249), fp64 then float32
        wsym[n] = (float)(0.5 - 0.5 * cospi(2.0 * (double)n / (double)(F - 1)));
}

template <int F>
struct HopCfg {
    static constexpr int M = F / 2;
    static constexpr int T = Cfg<F>::T;
    static constexpr int WGS = T < 64 ? 64 : T;
};

// The dynamic LDS of the two bodies below is laid out once each, by a constructor that walks a cursor: LdsCarve hands
// out the pointers (the body), LdsSize only adds up (ofp_hop_create).
struct LdsCarve {
    unsigned char* p;
    template <class T, class N>
    __device__ T* take(N n) {
        T* at = reinterpret_cast<T*>(p);
        p = reinterpret_cast<unsigned char*>(at + n);
        return at;
    }
    __device__ void align16() { p = reinterpret_cast<unsigned char*>((reinterpret_cast<uintptr_t>(p) + 15) & ~(uintptr_t)15); }
};
struct LdsSize {
    size_t bytes = 0;
    template <class T, class N>
    T* take(N n) {
        bytes += (size_t)n * sizeof(T);
        return nullptr;
    }
    void align16() { bytes += 16; }  // (room for the rounding, whatever the base)
};

template <int F>
struct SpectralLds {
    float2 *twM, *twF, *A;
    float *win, *fw, *partial, *mprm, *tileA, *tileB, *hcol;
    int32_t *flo, *flen, *foff;
    MelSegs* segs;
    template <class Cursor>
    __host__ __device__ SpectralLds(Cursor& c, int nnz, int n_mels, const MlpPlan& plan, int B) {
        constexpr int M = F / 2;
        twM = c.template take<float2>(M);
        twF = c.template take<float2>(M + 2);
        win = c.template take<float>(F);
        A = c.template take<float2>(FftBuf<M>::words);
        fw = c.template take<float>(nnz);
        flo = c.template take<int32_t>(n_mels);
        flen = c.template take<int32_t>(n_mels);
        foff = c.template take<int32_t>(n_mels);
        c.align16();
        segs = c.template take<MelSegs>(1);
        partial = c.template take<float>(MEL_MAXSEG);
        mprm = c.template take<float>((plan.n_params + 3) & ~3);
        tileA = c.template take<float>(16 * plan.st_a);
        tileB = c.template take<float>(16 * plan.st_b);
        hcol = c.template take<float>(B);  // [B] this channel's column of the hop
    }
};

template <int F>
struct StrengthLds {
    float2 *twM, *twF, *A;
    float *hbuf, *red, *y, *tg;
    template <class Cursor>
    __host__ __device__ StrengthLds(Cursor& c, int B, int C, int tg_len) {
        constexpr int M = F / 2;
        twM = c.template take<float2>(M);
        twF = c.template take<float2>(M + 2);
        A = c.template take<float2>(FftBuf<M>::words);
        hbuf = c.template take<float>((size_t)B * C);  // [B][C] the hop
        red = c.template take<float>(64);              // reduction slots: one per wave, and the dB floor
        y = c.template take<float>(tg_len);            // tempogram: [W] windowed envelope, then [W] the raw lags
        tg = c.template take<float>(tg_len);
    }
};

// One channel's share of a hop: ring write, Hann x trailing n_fft samples, rFFT, |X|^2, mel bands and the
// classifier.  Executed by one workgroup of WGS lanes (WGS == T when a frame needs more than one wave:
// the FFT passes then synchronise with workgroup barriers); h = hops pushed including this one.
template <int F, int WGS>
__device__ __forceinline__ void hop_spectral_body(const HopArgs& a, int c, int64_t h, unsigned char* smem) {
    constexpr int M = HopCfg<F>::M, T = HopCfg<F>::T;
    static_assert(T <= 64 ? WGS >= 64 : WGS == T, "lanes of a multi-wave frame must be the whole workgroup");
    LdsCarve carve{smem};
    const SpectralLds<F> l(carve, a.nnz, a.n_mels, a.plan, a.B);
    const int C = a.C, B = a.B;
    const int tid = threadIdx.x;
    // the hop may live in pinned host memory: every sample is fetched exactly once
    for (int t = tid; t < B; t += WGS) l.hcol[t] = a.hop[(int64_t)t * C + c];
    // tables, filterbank and classifier parameters: L2-resident copies -> LDS
    for (int k = tid; k < M; k += WGS) l.twM[k] = a.twM[k];
    for (int k = tid; k <= M; k += WGS) l.twF[k] = a.twF[k];
    for (int n = tid; n < F; n += WGS) l.win[n] = a.win[n];
    for (int i = tid; i < a.nnz; i += WGS) l.fw[i] = a.fw[i];
    for (int i = tid; i < a.n_mels; i += WGS) {
        l.flo[i] = a.flo[i];
        l.flen[i] = a.flen[i];
        l.foff[i] = a.foff[i];
    }
    for (int i = tid; i < a.plan.n_params; i += WGS) l.mprm[i] = a.plan.params[i];
    if (a.plan.n_layers > 0)
        for (int i = tid; i < 16 * a.plan.st_a; i += WGS) l.tileA[i] = 0.0f;
    if (tid == 0) mel_build_segs(l.segs, a.flen, a.n_mels);
    const int64_t first = (h - 1) * B;  // stream index of this hop's first sample
    __syncthreads();
    // ring-buffer write of this channel's column (realtime/audio.py:97)
    for (int t = tid; t < B; t += WGS) a.ring[((first + t) % a.R) * C + c] = l.hcol[t];
    // trailing n_fft samples of the stream (realtime/recording.py:276: audio[-n_fft:]); samples before
    // the stream started read as the zeros the ring was created with
    const int64_t base = h * B - F;
    auto sample = [&](int64_t s) -> float {
        if (s < 0) return 0.0f;
        if (s >= first) return l.hcol[s - first];
        return a.ring[(s % a.R) * C + c];
    };
    for (int p = tid; p < M; p += WGS)
        l.A[fft_pad<M>(p)] = make_float2(sample(base + 2 * p) * l.win[2 * p], sample(base + 2 * p + 1) * l.win[2 * p + 1]);
    __syncthreads();
    if (tid < T) {
        cfft<M, T>(l.A, l.twM, tid);
        // the same paired power bins, LDS staging and band sums as k_stft_power (bit-identical to its frame)
        constexpr int NQ = (M / 2) / T + 1;
        float pa[NQ], pb[NQ];
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            const int pp = tid + q * T;
            pa[q] = pb[q] = 0.0f;
            if (pp <= M / 2) rfft_power_pair<M>(l.A, l.twF, pp, pa[q], pb[q]);
        }
        frame_sync<T>();  // every bin of the spectrum has been read
        float* pf = reinterpret_cast<float*>(l.A);
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            const int pp = tid + q * T;
            if (pp <= M / 2) {
                pf[pp] = pa[q];
                if (pp < M / 2) pf[M - pp] = pb[q];
            }
        }
        frame_sync<T>();
        mel_bands(l.segs, pf, l.fw, l.flo, l.flen, l.foff, a.n_mels, tid, T, l.partial, [] { frame_sync<T>(); },
                  [&](int b, float acc) {
                      a.mel[c * a.n_mels + b] = acc;
                      if (a.plan.n_layers > 0) l.tileA[b] = acc;  // row 0 of the classifier's tile
                  });
    }
    if (a.plan.n_layers > 0) {
        __syncthreads();
        if (tid < 64) {
            const int nout = a.plan.dims[a.plan.n_layers];
            ofp_mlp_tile(a.plan, l.mprm, l.tileA, l.tileB, tid, [&](int r, int col, float v) {
                if (r == 0) a.logits[c * nout + col] = v;
            });
        }
    }
}

// One workgroup: the channel-mean frame of the hop that ends at sample h*B and its onset strength.
template <int F, int WGS>
__device__ __forceinline__ void hop_strength_body(const HopArgs& a, int64_t h, unsigned char* smem) {
    constexpr int M = HopCfg<F>::M, T = HopCfg<F>::T;
    static_assert(T <= 64 ? WGS >= 64 : WGS == T, "lanes of a multi-wave frame must be the whole workgroup");
    const StrengthArgs& g = a.sg;
    static_assert(WGS / 64 + 2 <= 64, "one reduction slot per wave and the dB floor");
    LdsCarve carve{smem};
    const StrengthLds<F> l(carve, a.B, a.C, g.tg_len);
    const int C = a.C, B = a.B, tid = threadIdx.x;
    for (int k = tid; k < M; k += WGS) l.twM[k] = a.twM[k];
    for (int k = tid; k <= M; k += WGS) l.twF[k] = a.twF[k];
    for (int i = tid; i < B * C; i += WGS) l.hbuf[i] = a.hop[i];
    __syncthreads();
    const int64_t first = (h - 1) * B, base = h * B - F;
    auto mean_sample = [&](int64_t s) -> float {  // audio[-n_fft:].mean(-1): float32 sum in channel order, then / C
        if (s < 0) return 0.0f;
        float m = 0.0f;
        if (s >= first) {
            for (int c = 0; c < C; ++c) m += l.hbuf[(s - first) * C + c];
        } else {
            const float* r = a.ring + (s % a.R) * C;
            for (int c = 0; c < C; ++c) m += r[c];
        }
        return m / (float)C;
    };
    for (int p = tid; p < M; p += WGS)
        l.A[fft_pad<M>(p)] = make_float2(g.wsym[2 * p] * mean_sample(base + 2 * p), g.wsym[2 * p + 1] * mean_sample(base + 2 * p + 1));
    __syncthreads();
    constexpr int NK = M / T + 1;
    float pw[NK], sdb[NK];
    float smax = -INFINITY;
    if (tid < T) {
        cfft<M, T>(l.A, l.twM, tid);
#pragma unroll
        for (int q = 0; q < NK; ++q) {
            const int k = tid + q * T;
            pw[q] = 0.0f;
            sdb[q] = -INFINITY;
            if (k <= M) {
                const float2 X = rfft_bin<M>(l.A, l.twF, k);
                pw[q] = X.x * X.x + X.y * X.y;
                sdb[q] = 10.0f * log10f(fmaxf(1e-10f, pw[q]));   // :290
                smax = fmaxf(smax, sdb[q]);
            }
        }
    }
    // block maximum of the dB spectrum -> the tracked maximum (:291), floor 80 dB below it (:292-294)
    for (int o = 32; o > 0; o >>= 1) smax = fmaxf(smax, __shfl_xor(smax, o));
    if ((tid & 63) == 0) l.red[tid >> 6] = smax;
    __syncthreads();
    if (tid == 0) {
        float m = l.red[0];
        for (int w = 1; w < (WGS + 63) / 64; ++w) m = fmaxf(m, l.red[w]);
        float ls = g.st[0];
        ls = m > ls ? m : (1.0f - g.ls_alpha) * ls + g.ls_alpha * m;
        ls = fmaxf(ls, g.ls_minmax);
        g.st[0] = ls;
        l.red[WGS / 64 + 1] = ls - 80.0f;
    }
    __syncthreads();
    const float floor_db = l.red[WGS / 64 + 1];
    float fsum = 0.0f;
    if (tid < T) {
#pragma unroll
        for (int q = 0; q < NK; ++q) {
            const int k = tid + q * T;
            if (k <= M) {
                const float s1 = fmaxf(sdb[q], floor_db);
                const float s0 = fmaxf(10.0f * log10f(fmaxf(1e-10f, g.prev[k])), floor_db);
                fsum += fmaxf(0.0f, s1 - s0);                       // :296
                g.prev[k] = pw[q];
            }
        }
    }
    for (int o = 32; o > 0; o >>= 1) fsum += __shfl_xor(fsum, o);
    __syncthreads();
    if ((tid & 63) == 0) l.red[tid >> 6] = fsum;
    __syncthreads();
    if (tid == 0) {
        float sum = 0.0f;
        for (int w = 0; w < (WGS + 63) / 64; ++w) sum += l.red[w];
        const float oe = sum / (float)(M + 1);
        float mn = g.st[1], mx = g.st[2];
        mx = oe > mx ? oe : (1.0f - g.oe_alpha) * mx + g.oe_alpha * oe;   // :299 add_sample
        mn = oe < mn ? oe : (1.0f - g.oe_alpha) * mn + g.oe_alpha * oe;
        mn = fmaxf(mn, g.oe_minmin);
        g.st[1] = mn;
        g.st[2] = mx;
        const float norm = (oe - mn) / (mx - mn);                          // :300-302 normalize_sample
        g.ring[(h - 1) % g.n_ring] = norm;
        g.out[0] = oe;
        g.out[1] = norm;
    }
    __syncthreads();
    // moving max / mean over the last MAX_LENGTH / AVG_LENGTH entries (:304-311; entries before the stream
    // started are the zeros the ring was created with)
    float vmax = -INFINITY, vsum = 0.0f;
    for (int i = tid; i < max(g.max_length, g.avg_length); i += WGS) {
        const int64_t e = h - 1 - i;
        const float v = e >= 0 ? g.ring[e % g.n_ring] : 0.0f;
        if (i < g.max_length) vmax = fmaxf(vmax, v);
        if (i < g.avg_length) vsum += v;
    }
    for (int o = 32; o > 0; o >>= 1) {
        vmax = fmaxf(vmax, __shfl_xor(vmax, o));
        vsum += __shfl_xor(vsum, o);
    }
    if ((tid & 63) == 0) {
        l.red[tid >> 6] = vmax;
        l.hbuf[tid >> 6] = vsum;
    }
    __syncthreads();
    if (tid == 0) {
        float m = l.red[0], sm = l.hbuf[0];
        for (int w = 1; w < (WGS + 63) / 64; ++w) {
            m = fmaxf(m, l.red[w]);
            sm += l.hbuf[w];
        }
        g.out[2] = m;
        g.out[3] = sm / (float)g.avg_length;
    }
    // Tempogram frame (realtime/recording.py:313-327): irfft(|rfft(w * onset_env[-W:], n = 2W - 1)|^2)[:W] -- the
    // transform length 2W - 1 makes the circular correlation the LINEAR autocorrelation of the windowed envelope, so the
    // W lags are computed as what they are, tg[k] = sum_i y[i] y[i + k] (float32 fma chain over ascending i; the
    // reference's float FFT round trip agrees to its own rounding), then tg / (max(tg) + 1e-10).  Lags k and W-1-k go
    // to the same thread: W + 1 products each.  PARITY UNPINNED like the envelope it reads.
    if (g.tg_len > 0) {
        const int W = g.tg_len;
        for (int i = tid; i < W; i += WGS) {
            const int64_t e = h - W + i;   // onset_env[-W + i]; entries before the stream started are the ring's zeros
            l.y[i] = e >= 0 ? g.tgw[i] * g.ring[e % g.n_ring] : 0.0f;
        }
        __syncthreads();
        float mx = -INFINITY;
        for (int k = tid; 2 * k < W; k += WGS) {
            const int k2 = W - 1 - k;
            float a0 = 0.0f, a1 = 0.0f;
            for (int i = 0; i + k < W; ++i) a0 = fmaf(l.y[i], l.y[i + k], a0);
            if (k2 != k)
                for (int i = 0; i + k2 < W; ++i) a1 = fmaf(l.y[i], l.y[i + k2], a1);
            l.tg[k] = a0;
            mx = fmaxf(mx, a0);
            if (k2 != k) {
                l.tg[k2] = a1;
                mx = fmaxf(mx, a1);
            }
        }
        for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
        __syncthreads();
        if ((tid & 63) == 0) l.red[tid >> 6] = mx;
        __syncthreads();
        float m = l.red[0];
        for (int w = 1; w < (WGS + 63) / 64; ++w) m = fmaxf(m, l.red[w]);
        const float den = m + 1e-10f;
        for (int k = tid; k < W; k += WGS) g.out[4 + k] = l.tg[k] / den;
    }
}

template <int F>
__global__ __launch_bounds__(HopCfg<F>::WGS) void k_hop_strength(HopArgs a) {
    extern __shared__ __align__(16) unsigned char smem[];
    hop_strength_body<F, HopCfg<F>::WGS>(a, a.ctl[0], smem);
}

template <int F>
__global__ __launch_bounds__(HopCfg<F>::WGS) void k_hop_spectral(HopArgs a) {
    extern __shared__ __align__(16) unsigned char smem[];
    hop_spectral_body<F, HopCfg<F>::WGS>(a, blockIdx.x, a.ctl[0], smem);
}

// The location block of a hop in the result block (ofp_hop_collect_location)
struct HopLocBlock {
    int32_t status, fed, dropped, flags, n_members, pad;
    double xy[2];
    int32_t sens[OFP_LOCS_MEMBERS];
    int64_t on[OFP_LOCS_MEMBERS];
};

struct HopLocArgs {
    int enabled;
    ofp::LocTables T;
    ofp_locate_state* state;
    HopLocBlock* out;
};

// detect_hits' loop (realtime/audio.py:62-74) for one hop, by one workgroup: the hop's n records sorted by onset
// (np.argsort; ties keep record order), each fed to locate with counter = h * B until one returns a position.  Rows
// of the current hop come from the hop buffer (other workgroups are writing the ring during a fused launch), older
// rows from the ring, rows before sample 0 are zeros.  h = hops pushed including this one.
__device__ __forceinline__ void hop_locate_stage(const HopArgs& a, const HopLocArgs& la, int64_t h, int n,
                                                 const ofp_onset* recs, unsigned char* smem) {
    __shared__ int s_order[64];
    __shared__ ofp::LocGroup s_located;
    const ofp::LocTables& T = la.T;
    const int tid = threadIdx.x, nt = blockDim.x;
    const int C = a.C, B = a.B;
    const ofp::LocView v = ofp::loc_carve(smem, nt, T.max_section, T.plan);
    float* hopbuf = v.extra;  // [B][C] the hop
    n = n < C ? n : C;
    __syncthreads();  // the detector is done with this LDS
    ofp::loc_load(T, v, la.state);
    if (T.use_audio)
        for (int i = tid; i < B * C; i += nt) hopbuf[i] = a.hop[i];
    if (tid == 0) {
        for (int i = 0; i < n; ++i) {  // stable insertion argsort
            int q = i;
            while (q > 0 && recs[s_order[q - 1]].sample > recs[i].sample) {
                s_order[q] = s_order[q - 1];
                --q;
            }
            s_order[q] = i;
        }
    }
    __syncthreads();
    const int64_t first = (h - 1) * B, counter = h * B;
    auto sample = [&](int64_t t, int col) -> float {
        if (t < 0) return 0.0f;
        if (t >= first) return hopbuf[(t - first) * C + col];
        return a.ring[(t % a.R) * C + col];
    };
    int fed = 0, status = 0;
    double xy[2] = {0.0, 0.0};
    for (int i = 0; i < n && !status; ++i) {  // the locator's kind (T.planar) is the session's
        const ofp_onset r = recs[s_order[i]];
        status = ofp::loc_feed_kind(T, v, r.channel, first + r.sample, counter, true, sample, xy, &s_located);
        ++fed;
    }
    __syncthreads();
    if (tid == 0) {
        HopLocBlock* o = la.out;
        o->status = status;
        o->fed = fed;
        o->dropped = n - fed;
        o->flags = v.L->st[v.L->cur].flags;
        o->n_members = status ? s_located.len : 0;
        o->xy[0] = xy[0];
        o->xy[1] = xy[1];
        for (int k = 0; k < OFP_LOCS_MEMBERS; ++k) {
            o->sens[k] = status && k < s_located.len ? s_located.sens[k] : 0;
            o->on[k] = status && k < s_located.len ? s_located.on[k] : 0;
        }
    }
    ofp::loc_store(v, la.state);
}

// Nodes form: the stage as a kernel of its own after the detector node.
__global__ __launch_bounds__(256) void k_hop_locate(HopArgs a, HopLocArgs la, const ofp_onset* recs) {
    extern __shared__ __align__(16) unsigned char smem[];
    const int64_t n = *a.count;
    if (n <= 0) return;
    hop_locate_stage(a, la, a.ctl[0], (int)(n < a.C ? n : a.C), recs, smem);
}

// The hit block of a hop in the result block (ofp_hop_collect_hit); `hop` names the hop (counted from 1) that wrote
// start, row and y, so a hop that evaluates nothing writes nothing
struct HopRegBlock {
    int64_t hop;
    int32_t flags, pad;
    int64_t start;
    int64_t row[OFP_REG_MAX_SIGNALS];
    float y[OFP_REG_MAX_OUT];
};

struct HopRegArgs {
    int enabled;
    ofpreg::Cfg g;
    HopRegBlock* out;
};

// How a grouping stage (the window regressor's, the voting locator's) takes one hop, by one workgroup of 256 threads
// after the detector and the locator stage: the hop's n records in the locator stage's order (sorted by sample, ties
// in record order), rows by the same rule (current hop from the hop buffer -- each needed sample is fetched once --,
// older rows from the ring, rows before sample 0 zero).  h = hops pushed including this one; wake: the state's word of
// that name, loaded by the caller before the detector ran, so that a hop with nothing to feed, close or evaluate
// leaves on one uniform comparison.  g: the stage's configuration; run(n, rec, sample): its step.
template <class G, class Run>
__device__ __forceinline__ void hop_grouping_stage(const HopArgs& a, const G& g, int64_t h, int n, int64_t wake,
                                                   const ofp_onset* recs, Run run) {
    const int C = a.C, B = a.B;
    n = n < C ? n : C;
    if (ofpreg::idle(g, h, n, wake)) return;
    __syncthreads();  // the detector and the locator stage are done with this LDS
    const int64_t first = (h - 1) * B;
    auto rec = [&](int i, int& ch, int64_t& s) {  // the i-th record of the stable argsort (n <= 8: by rank)
        for (int j = 0; j < n; ++j) {
            int rank = 0;
            for (int k = 0; k < n; ++k)
                rank += recs[k].sample < recs[j].sample || (recs[k].sample == recs[j].sample && k < j);
            if (rank == i) {
                ch = recs[j].channel;
                s = first + recs[j].sample;
                return;
            }
        }
    };
    auto sample = [&](int64_t t, int col) -> float {
        if (t < 0) return 0.0f;
        if (t >= first) return a.hop[(t - first) * C + col];
        return a.ring[(t % a.R) * C + col];
    };
    run(n, rec, sample);
}

// The window regressor's step for one hop (ofp_regress_dev.h).
__device__ __forceinline__ void hop_regress_stage(const HopArgs& a, const HopRegArgs& ra, int64_t h, int n, int64_t wake,
                                                  const ofp_onset* recs, unsigned char* smem) {
    hop_grouping_stage(a, ra.g, h, n, wake, recs, [&](int m, auto rec, auto sample) {
        HopRegBlock* o = ra.out;
        const int ev = ofpreg::step(ra.g, h, m, rec, sample, smem, &o->start, o->row, o->y, &o->flags);
        if (ev && threadIdx.x == 0) o->hop = h;
    });
}

// The block of the voting locator in the result block (ofp_hop_collect_cc_hit); `hop` as in HopRegBlock
struct HopPairBlock {
    int64_t hop;
    int32_t flags, status;
    int64_t onset;
    int64_t row[OFP_REG_MAX_SIGNALS];
    int32_t first, cell;
    int32_t lags[2];
    double xy[2], rphi[2];
};

struct HopPairArgs {
    int enabled;
    ofppair::Cfg g;
    HopPairBlock* out;
};

// The voting locator's step for one hop (ofp_paired_dev.h), by one workgroup of 256 threads after the detector.
__device__ __forceinline__ void hop_paired_stage(const HopArgs& a, const HopPairArgs& pa, int64_t h, int n, int64_t wake,
                                                 const ofp_onset* recs, unsigned char* smem) {
    hop_grouping_stage(a, pa.g, h, n, wake, recs, [&](int m, auto rec, auto sample) {
        HopPairBlock* b = pa.out;
        const ofppair::Out o{&b->onset, b->row, &b->first, &b->status, b->lags, &b->cell, b->xy, b->rphi, &b->flags};
        const int ev = ofppair::step(pa.g, h, m, rec, sample, smem, o);
        if (ev && threadIdx.x == 0) b->hop = h;
    });
}

// Nodes form: the stage as a kernel of its own where the locate node is, before the spectral node.
__global__ __launch_bounds__(256) void k_hop_paired(HopArgs a, HopPairArgs pa, const ofp_onset* recs) {
    extern __shared__ __align__(16) unsigned char smem[];
    const int64_t n = *a.count;
    hop_paired_stage(a, pa, a.ctl[0], (int)(n < a.C ? n : a.C), pa.g.state->wake, recs, smem);
}

// Nodes form: the stage as a kernel of its own after the detector and the locate node.
__global__ __launch_bounds__(256) void k_hop_regress(HopArgs a, HopRegArgs ra, const ofp_onset* recs) {
    extern __shared__ __align__(16) unsigned char smem[];
    const int64_t n = *a.count;
    hop_regress_stage(a, ra, a.ctl[0], (int)(n < a.C ? n : a.C), ra.g.state->wake, recs, smem);
}

// The whole hop in ONE launch: workgroup 0 is the detector (the phase-split block step of
// ofp_stream_dev.h), workgroups 1..C the spectral branch of one channel each -- the two do not depend
// on each other, so the hop takes max(detector, spectral) instead of their sum plus three launch gaps.
// The hop is read straight from the pinned host buffer and the result block written straight to pinned
// host memory (no copy nodes).  The hop counter is advanced by the workgroup that finishes last.
template <int F>
struct FusedCfg {
    static constexpr int WGS = HopCfg<F>::T <= 64 ? 256 : HopCfg<F>::T;
};

// Which hit stages the detector's workgroup runs after the detector: a compile-time kind.  Five are legal -- none, LOC,
// REG, LOC | REG and PAIR (the voting locator is a session's only stage) -- and HitArgs<K> exists for those alone: the
// stage argument structs that K names, and nothing else (a session without a stage passes no stage arguments).
enum : int { HIT_NONE = 0, HIT_LOC = 1, HIT_REG = 2, HIT_PAIR = 4 };
template <int K> struct HitArgs;
template <> struct HitArgs<HIT_NONE> {};
template <> struct HitArgs<HIT_LOC> { HopLocArgs la; };
template <> struct HitArgs<HIT_REG> { HopRegArgs ra; };
template <> struct HitArgs<HIT_LOC | HIT_REG> { HopLocArgs la; HopRegArgs ra; };
template <> struct HitArgs<HIT_PAIR> { HopPairArgs pa; };

// Everything a workgroup of the fused hop does, from the read of the hop counter to the completion word; the
// arguments are the caller's (kernel arguments or a group's device arrays), never copies.  K: the session's hit kind;
// without a stage the detector's workgroup is the one it always was.
template <int F, int K>
__device__ __forceinline__ void hop_fused_body(const HopArgs& a, const ofpstream::StreamArgs& sa, const HitArgs<K>& ha,
                                               unsigned char* smem) {
    static_assert(!(K & HIT_PAIR) || K == HIT_PAIR, "the voting locator is a session's only stage");
    const int64_t done = a.ctl[0];  // hops completed before this one
    if (blockIdx.x == 0) {
        if (threadIdx.x == 0) *a.hop_index = done;
        if constexpr (K != HIT_NONE) {
            int64_t wake = 0;
            if constexpr (K & HIT_REG) wake = ha.ra.g.state->wake;  // (in flight while the detector runs)
            if constexpr (K & HIT_PAIR) wake = ha.pa.g.state->wake;
            const long long n_on = ofpstream::stream_par_blocks<true>(sa, reinterpret_cast<float*>(smem));
            const int n = (int)(n_on < a.C ? n_on : a.C);
            if constexpr (K & HIT_LOC)
                if (n_on > 0) hop_locate_stage(a, ha.la, done + 1, n, sa.mirror, smem);
            if constexpr (K & HIT_REG) {
                static_assert(FusedCfg<F>::WGS == ofpnn::WG, "the per-item forward passes are written for 256 threads");
                hop_regress_stage(a, ha.ra, done + 1, n, wake, sa.mirror, smem);
            }
            if constexpr (K & HIT_PAIR) {
                static_assert(FusedCfg<F>::WGS == ofppair::FT, "the lag search and the vote are written for 256 threads");
                hop_paired_stage(a, ha.pa, done + 1, n, wake, sa.mirror, smem);
            }
        } else {
            ofpstream::stream_par_blocks(sa, reinterpret_cast<float*>(smem));
        }
    } else if ((int)blockIdx.x <= a.C) {
        hop_spectral_body<F, FusedCfg<F>::WGS>(a, (int)blockIdx.x - 1, done + 1, smem);
    } else {  // the onset-strength workgroup (only launched when enabled)
        hop_strength_body<F, FusedCfg<F>::WGS>(a, done + 1, smem);
    }
    // EVERY thread drains its own stores to the result block (pinned host memory) and the ring before the barrier:
    // the barrier does not wait for outstanding stores, and a fence by thread 0 alone covers only its own wave, so
    // the completion word could otherwise become visible while another wave's `rel` / `mel` rows are still in flight
    __threadfence_system();
    __syncthreads();
    if (threadIdx.x == 0) {
        __threadfence_system();  // (orders the ticket after the barrier's view of the other waves' fences)
        const unsigned long long t = atomicAdd(reinterpret_cast<unsigned long long*>(a.ctl + 1), 1ull);
        if (t == gridDim.x - 1) {  // every workgroup (gridDim.x of them) has read ctl[0] and published its results
            a.ctl[1] = 0;
            a.ctl[0] = done + 1;
            __threadfence_system();
            *a.done_flag = done + 1;
        }
    }
}

template <int F, int K>
__global__ __launch_bounds__(FusedCfg<F>::WGS) void k_hop_fused(HopArgs a, ofpstream::StreamArgs sa, HitArgs<K> ha) {
    extern __shared__ __align__(16) unsigned char smem[];
    hop_fused_body<F, K>(a, sa, ha, smem);
}

// S sessions' hops in ONE launch: grid (C + 1 + strength, S), row blockIdx.y is member blockIdx.y of an
// ofp_hop_group and runs hop_fused_body on that member's three argument structs in the group's device arrays
// (uniform, read-only addresses: scalar loads, as for kernel arguments) -- the member's own ticket, counter and
// completion word; the stages' architectures, locators and windows may differ from member to member.  Members share
// nothing and no workgroup waits for another, so a grid larger than the device simply queues.  n_fft, the channel
// count, the hit kind and whether the onset strength is on fix the instantiation and gridDim.x: a group's members
// agree on these four.  dry != 0: every workgroup returns at once (the un-captured launch at group creation that loads
// the code and sets the dynamic-LDS attribute must not touch a member's state).
template <int F, int K>
__global__ __launch_bounds__(FusedCfg<F>::WGS) void k_hop_fused_group(const HopArgs* __restrict__ args,
                                                                      const ofpstream::StreamArgs* __restrict__ sargs,
                                                                      const HitArgs<K>* __restrict__ hargs, int dry) {
    extern __shared__ __align__(16) unsigned char smem[];
    if (dry) return;
    hop_fused_body<F, K>(args[blockIdx.y], sargs[blockIdx.y], hargs[blockIdx.y], smem);
}

}  // namespace

struct ofp_hop_session {
    ofp_detector* det = nullptr;
    int C = 0, B = 0, n_fft = 0, n_mels = 0, n_out = 0, want_rel = 0;
    int64_t R = 0;
    hipStream_t stream = nullptr;
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    void* d_state = nullptr;
    float* d_hop = nullptr;
    float* d_ring = nullptr;
    int64_t* d_ctl = nullptr;
    float2* d_twM = nullptr;
    float2* d_twF = nullptr;
    float* d_win = nullptr;
    float* d_wsym = nullptr;
    float* d_tgw = nullptr;   // tempogram window
    float* d_sg = nullptr;      // onset strength: prev power [bins] | st [4] | ring [n_ring]
    float sg_init[4] = {10.0f, 0.0f, 1.0f, 0.0f};  // ls_max0, oe_min0, oe_max0
    size_t sg_floats = 0;
    size_t lds_strength = 0;
    int32_t* d_fb_i = nullptr;  // lo | len | off
    float* d_fb_w = nullptr;
    float* d_prm = nullptr;     // own copy of the classifier's parameters
    unsigned char* d_res = nullptr;
    float* h_hop = nullptr;           // pinned
    unsigned char* h_res = nullptr;   // pinned
    // result block layout (bytes)
    int64_t o_count = 0, o_index = 8, o_done = 16, o_rec = 24, o_logits = 0, o_mel = 0, o_rel = 0, o_sg = 0, res_bytes = 0;
    HopArgs args;
    ofpstream::StreamArgs sargs;  // fused form: the detector workgroup's arguments
    bool fused = false;
    int threads = 256;  // of the workgroup that runs the detector and the locator (fused form: the fused kernel's)
    unsigned char* res_dev = nullptr;  // the result block as the kernels address it (point_results)
    size_t lds_fused = 0;
    size_t lds = 0;
    int64_t pushed = 0;   // hops submitted
    bool in_flight = false;
    bool retired = true;   // the last hop's kernel is known to have left the stream (a polled completion is not that)
    // the locator (ofp_hop_set_locator)
    HopLocArgs largs;
    ofp_locate_state* d_loc_state = nullptr;
    float* d_loc_prm = nullptr;     // own copy of the locator network's parameters
    ofp_onset* d_mirror = nullptr;  // fused form: the records in device memory
    int64_t o_loc = 0;
    size_t lds_loc = 0;
    // the regressor (ofp_hop_set_regressor)
    HopRegArgs rargs;
    ofp_regress_state* d_reg_state = nullptr;
    float* d_reg_prm = nullptr;  // own copy of the model's parameters
    float* d_reg_ws = nullptr;   // activations of a model too large for the LDS
    int64_t o_reg = 0;
    size_t lds_reg = 0;
    // the voting locator (ofp_hop_set_locator_paired); its index tables are the caller's
    HopPairArgs pargs;
    ofp_regress_state* d_pair_state = nullptr;
    int64_t o_pair = 0;
    size_t lds_pair = 0;
    int device = 0;
    ofp_hop_group* owner = nullptr;  // the group whose launches carry this session's hops (ofp_hop_group_create)
};

// S fused sessions served by one launch per hop period.  The members keep their state, ring, pinned blocks and
// counters; the group owns the stream the launches go to, copies of the members' kernel arguments and the graph.
struct ofp_hop_group {
    std::vector<ofp_hop_session*> members;
    int device = 0, n_fft = 0, grid_x = 0;
    bool loc = false, reg = false, pair = false;
    size_t lds = 0;
    hipStream_t stream = nullptr;
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    HopArgs* d_args = nullptr;
    ofpstream::StreamArgs* d_sargs = nullptr;
    void* d_hargs = nullptr;  // [members] HitArgs<K>, K the kind that loc, reg and pair name
};

namespace {

// Every launch goes through ensure_dynamic_lds with a cache of its own instantiation: the attribute is set by the
// un-captured first pass (capture_hop, group_build) and found in the cache during capture, where it may not be set.
template <int F>
int hop_tables(ofp_hop_session* s) {
    hipLaunchKernelGGL(k_hop_tables<F>, dim3(1), dim3(256), 0, s->stream, s->d_twM, s->d_twF, s->d_win, s->d_wsym);
    OFP_LAUNCH_CHECK("k_hop_tables");
    return OFP_OK;
}

template <int F>
int hop_spectral(ofp_hop_session* s) {
    static ofp::LdsAttrCache attr;
    if (int rc = ofp::ensure_dynamic_lds(reinterpret_cast<const void*>(k_hop_spectral<F>), s->lds, attr)) return rc;
    hipLaunchKernelGGL(k_hop_spectral<F>, dim3((unsigned)s->C), dim3(HopCfg<F>::WGS), s->lds, s->stream, s->args);
    OFP_LAUNCH_CHECK("k_hop_spectral");
    return OFP_OK;
}

template <int F>
int hop_strength(ofp_hop_session* s) {
    static ofp::LdsAttrCache attr;
    if (int rc = ofp::ensure_dynamic_lds(reinterpret_cast<const void*>(k_hop_strength<F>), s->lds_strength, attr)) return rc;
    hipLaunchKernelGGL(k_hop_strength<F>, dim3(1), dim3(HopCfg<F>::WGS), s->lds_strength, s->stream, s->args);
    OFP_LAUNCH_CHECK("k_hop_strength");
    return OFP_OK;
}

constexpr size_t FUSED_LDS_THRESHOLD = 65536 - 20480;  // (the detector's static LDS comes on top)

// The run-time flags of a session or a group as one of the five compile-time hit kinds: f(integral_constant<int, K>).
template <class Fn>
int with_hit_kind(bool loc, bool reg, bool pair, Fn f) {
    switch ((loc ? HIT_LOC : 0) | (reg ? HIT_REG : 0) | (pair ? HIT_PAIR : 0)) {
        case HIT_NONE: return f(std::integral_constant<int, HIT_NONE>());
        case HIT_LOC: return f(std::integral_constant<int, HIT_LOC>());
        case HIT_REG: return f(std::integral_constant<int, HIT_REG>());
        case HIT_LOC | HIT_REG: return f(std::integral_constant<int, HIT_LOC | HIT_REG>());
        case HIT_PAIR: return f(std::integral_constant<int, HIT_PAIR>());
    }
    return ofp::fail(OFP_ERR_INVALID, "the voting locator is a session's only stage");
}

// the stage arguments of a session of kind K, as the fused kernels take them
template <int K>
HitArgs<K> hit_args(const ofp_hop_session* s) {
    HitArgs<K> ha{};
    if constexpr (K & HIT_LOC) ha.la = s->largs;
    if constexpr (K & HIT_REG) ha.ra = s->rargs;
    if constexpr (K & HIT_PAIR) ha.pa = s->pargs;
    return ha;
}

template <int F, int K>
int hop_fused_launch(ofp_hop_session* s) {
    static ofp::LdsAttrCache attr;
    if (int rc = ofp::ensure_dynamic_lds((const void*)k_hop_fused<F, K>, s->lds_fused, attr, FUSED_LDS_THRESHOLD)) return rc;
    hipLaunchKernelGGL((k_hop_fused<F, K>), dim3((unsigned)s->C + 1 + (s->args.sg.enabled ? 1 : 0)),
                       dim3(FusedCfg<F>::WGS), s->lds_fused, s->stream, s->args, s->sargs, hit_args<K>(s));
    OFP_LAUNCH_CHECK("k_hop_fused");
    return OFP_OK;
}

// Nodes form: a hit stage as a node of its own, one workgroup of 256 threads on the records the detector node wrote.
template <auto Kernel, class StageArgs>
int hop_stage_node(ofp_hop_session* s, const StageArgs& stage, size_t lds, const char* name) {
    static ofp::LdsAttrCache attr;
    if (int rc = ofp::ensure_dynamic_lds(reinterpret_cast<const void*>(Kernel), lds, attr)) return rc;
    hipLaunchKernelGGL(Kernel, dim3(1), dim3(256), lds, s->stream, s->args, stage,
                       reinterpret_cast<const ofp_onset*>(s->d_res + s->o_rec));
    OFP_LAUNCH_CHECK(name);
    return OFP_OK;
}

// the per-hop sequence, enqueued on the session's stream (captured once, then replayed)
int enqueue_hop(ofp_hop_session* s) {
    if (s->fused)  // one kernel: no copy nodes, no begin kernel
        return with_n_fft(s->n_fft, [&](auto f) {
            return with_hit_kind(s->largs.enabled, s->rargs.enabled, s->pargs.enabled,
                                 [&](auto k) { return hop_fused_launch<decltype(f)::value, decltype(k)::value>(s); });
        });
    OFP_HIP(hipMemcpyAsync(s->d_hop, s->h_hop, (size_t)s->B * s->C * sizeof(float), hipMemcpyHostToDevice, s->stream));
    hipLaunchKernelGGL(k_hop_begin, dim3(1), dim3(64), 0, s->stream, s->args);
    OFP_LAUNCH_CHECK("k_hop_begin");
    int rc = ofp_stream_process(s->det, s->d_state, s->d_hop, 1, 0, 0, 0,
                                s->want_rel ? reinterpret_cast<float*>(s->d_res + s->o_rel) : nullptr,
                                reinterpret_cast<ofp_onset*>(s->d_res + s->o_rec), s->C,
                                reinterpret_cast<int64_t*>(s->d_res + s->o_count), s->stream);
    if (rc != OFP_OK) return rc;
    if (s->largs.enabled)  // (before the spectral node: the ring holds the older hops only)
        if ((rc = hop_stage_node<k_hop_locate>(s, s->largs, s->lds_loc, "k_hop_locate")) != OFP_OK) return rc;
    if (s->pargs.enabled)  // (where the locate node is: the ring holds the older hops only)
        if ((rc = hop_stage_node<k_hop_paired>(s, s->pargs, s->lds_pair, "k_hop_paired")) != OFP_OK) return rc;
    if (s->rargs.enabled)  // (after the locate node, before the spectral node: the ring holds the older hops only)
        if ((rc = hop_stage_node<k_hop_regress>(s, s->rargs, s->lds_reg, "k_hop_regress")) != OFP_OK) return rc;
    if (s->args.sg.enabled) {  // (before the spectral node: it reads ring rows the spectral node is about to overwrite
                               //  only for hops older than the ring, never the current one)
        rc = with_n_fft(s->n_fft, [&](auto f) { return hop_strength<decltype(f)::value>(s); });
        if (rc != OFP_OK) return rc;
    }
    rc = with_n_fft(s->n_fft, [&](auto f) { return hop_spectral<decltype(f)::value>(s); });
    if (rc != OFP_OK) return rc;
    // (the hit block and, after it, the voting locator's are the result block's tail: a session without them copies
    //  the bytes it always copied)
    const int64_t copied = s->pargs.enabled ? s->res_bytes : s->rargs.enabled ? s->o_pair : s->o_reg;
    OFP_HIP(hipMemcpyAsync(s->h_res, s->d_res, (size_t)copied, hipMemcpyDeviceToHost, s->stream));
    return OFP_OK;
}

int reset_state(ofp_hop_session* s) {
    int rc = ofp_stream_state_init(s->det, s->d_state, s->stream);
    if (rc != OFP_OK) return rc;
    OFP_HIP(hipMemsetAsync(s->d_ring, 0, (size_t)s->R * s->C * sizeof(float), s->stream));
    OFP_HIP(hipMemsetAsync(s->d_ctl, 0, 2 * sizeof(int64_t), s->stream));
    OFP_HIP(hipMemsetAsync(s->d_res, 0, (size_t)s->res_bytes, s->stream));
    if (s->d_loc_state) OFP_HIP(hipMemsetAsync(s->d_loc_state, 0, sizeof(ofp_locate_state), s->stream));
    if (s->d_reg_state) OFP_HIP(hipMemsetAsync(s->d_reg_state, 0, sizeof(ofp_regress_state), s->stream));
    if (s->d_pair_state) OFP_HIP(hipMemsetAsync(s->d_pair_state, 0, sizeof(ofp_regress_state), s->stream));
    if (s->d_sg) {
        OFP_HIP(hipMemsetAsync(s->d_sg, 0, s->sg_floats * 4, s->stream));
        OFP_HIP(hipMemcpyAsync(s->args.sg.st, s->sg_init, 16, hipMemcpyHostToDevice, s->stream));
    }
    OFP_HIP(hipStreamSynchronize(s->stream));
    std::memset(s->h_res, 0, (size_t)s->res_bytes);
    s->pushed = 0;
    s->in_flight = false;
    return OFP_OK;
}

// What `enqueue` puts on the stream, as an instantiated graph.  The capture is ended whatever enqueue returns (a
// stream left capturing is of no use to anyone); enqueue's result is returned only after that.
template <class Enqueue>
int capture_graph(hipStream_t stream, Enqueue enqueue, hipGraph_t* graph, hipGraphExec_t* exec) {
    OFP_HIP(hipStreamBeginCapture(stream, hipStreamCaptureModeThreadLocal));
    const int rc = enqueue();
    const hipError_t ce = hipStreamEndCapture(stream, graph);
    if (rc != OFP_OK) return rc;
    if (ce != hipSuccess) return ofp::fail(OFP_ERR_HIP, "hipStreamEndCapture failed: %s", hipGetErrorString(ce));
    OFP_HIP(hipGraphInstantiate(exec, *graph, nullptr, nullptr, 0));
    return OFP_OK;
}

// one un-captured pass over zeros loads every code object and sets the kernel attributes
// (neither may happen during capture), then the state is reset and the sequence captured
int capture_hop(ofp_hop_session* s) {
    int rc = reset_state(s);
    if (rc != OFP_OK) return rc;
    if ((rc = enqueue_hop(s)) != OFP_OK) return rc;
    OFP_HIP(hipStreamSynchronize(s->stream));
    if ((rc = reset_state(s)) != OFP_OK) return rc;
    if (s->exec) (void)hipGraphExecDestroy(s->exec);
    if (s->graph) (void)hipGraphDestroy(s->graph);
    s->exec = nullptr;
    s->graph = nullptr;
    return capture_graph(s->stream, [&] { return enqueue_hop(s); }, &s->graph, &s->exec);
}

// The kernel arguments' pointers into the result block at `base`: d_res, or the mapped h_res as the device sees it
// (fused form, which alone has the detector's arguments and the completion word).
void point_results(ofp_hop_session* s, unsigned char* base) {
    HopArgs& a = s->args;
    s->res_dev = base;
    a.logits = reinterpret_cast<float*>(base + s->o_logits);
    a.mel = reinterpret_cast<float*>(base + s->o_mel);
    a.count = reinterpret_cast<int64_t*>(base + s->o_count);
    a.hop_index = reinterpret_cast<int64_t*>(base + s->o_index);
    if (a.sg.enabled) a.sg.out = reinterpret_cast<float*>(base + s->o_sg);
    if (base == s->d_res) return;
    a.done_flag = reinterpret_cast<volatile int64_t*>(base + s->o_done);
    s->sargs.rel = s->want_rel ? reinterpret_cast<float*>(base + s->o_rel) : nullptr;
    s->sargs.records = reinterpret_cast<ofp_onset*>(base + s->o_rec);
    s->sargs.count = a.count;
}

// the stream the session's last hop was launched to
hipStream_t hop_stream(const ofp_hop_session* s) { return s->owner ? s->owner->stream : s->stream; }

// The copies of ring_read / locator_state are not stream-ordered and reset / warm-up run on the session's own
// stream: the last hop's kernel (polled, not synchronised) must have left the stream it was launched to.
int retire_last_hop(ofp_hop_session* s) {
    if (!s->retired) {
        OFP_HIP(hipStreamSynchronize(hop_stream(s)));
        s->retired = true;
    }
    return OFP_OK;
}

// The fused kernel's last workgroup publishes the hop count after every result: poll it instead of paying the
// stream synchronisation's wake-up.  Bounded: an error or a lost launch falls through to the synchronisation of
// `stream` (*synced, when given, says that it came to that).
int wait_done(const ofp_hop_session* s, hipStream_t stream, bool* synced = nullptr) {
    const volatile int64_t* flag = reinterpret_cast<const volatile int64_t*>(s->h_res + s->o_done);
    for (int spin = 0; spin < 2000000 && *flag != s->pushed; ++spin) __builtin_ia32_pause();
    const bool late = *flag != s->pushed;
    if (late) OFP_HIP(hipStreamSynchronize(stream));
    if (synced) *synced = late;
    return OFP_OK;
}

#define OFP_NOT_IN_GROUP(s, what)                                                                                  \
    OFP_REQUIRE(!(s)->owner, what ": the session is a member of an ofp_hop_group (its hops go through "            \
                                  "ofp_hop_group_submit; ofp_hop_group_destroy releases it)")

template <int F, int K>
int hop_group_launch(ofp_hop_group* g, int dry) {
    static ofp::LdsAttrCache attr;
    if (int rc = ofp::ensure_dynamic_lds((const void*)k_hop_fused_group<F, K>, g->lds, attr, FUSED_LDS_THRESHOLD)) return rc;
    hipLaunchKernelGGL((k_hop_fused_group<F, K>), dim3((unsigned)g->grid_x, (unsigned)g->members.size()),
                       dim3(FusedCfg<F>::WGS), g->lds, g->stream, g->d_args, g->d_sargs,
                       static_cast<const HitArgs<K>*>(g->d_hargs), dry);
    OFP_LAUNCH_CHECK("k_hop_fused_group");
    return OFP_OK;
}

void group_free(ofp_hop_group* g) {
    if (g->stream) (void)hipStreamSynchronize(g->stream);
    if (g->exec) (void)hipGraphExecDestroy(g->exec);
    if (g->graph) (void)hipGraphDestroy(g->graph);
    if (g->d_args) (void)hipFree(g->d_args);
    if (g->d_sargs) (void)hipFree(g->d_sargs);
    if (g->d_hargs) (void)hipFree(g->d_hargs);
    if (g->stream) (void)hipStreamDestroy(g->stream);
    delete g;
}

// one argument struct per member, get(member), as a device array at *d
template <class Get>
int group_upload(const ofp_hop_group* g, void** d, Get get) {
    std::vector<decltype(get(g->members[0]))> v;
    for (const ofp_hop_session* s : g->members) v.push_back(get(s));
    OFP_HIP(hipMalloc(d, v.size() * sizeof(v[0])));
    OFP_HIP(hipMemcpy(*d, v.data(), v.size() * sizeof(v[0]), hipMemcpyHostToDevice));
    return OFP_OK;
}

// the group's resources on the members' device: the argument arrays, the dry launch, the captured graph
int group_build(ofp_hop_group* g) {
    OFP_HIP(hipStreamCreateWithFlags(&g->stream, hipStreamNonBlocking));
    if (int rc = group_upload(g, (void**)&g->d_args, [](const ofp_hop_session* s) { return s->args; })) return rc;
    if (int rc = group_upload(g, (void**)&g->d_sargs, [](const ofp_hop_session* s) { return s->sargs; })) return rc;
    if (int rc = with_hit_kind(g->loc, g->reg, g->pair, [&](auto k) {
            return group_upload(g, &g->d_hargs, [](const ofp_hop_session* s) { return hit_args<decltype(k)::value>(s); });
        }))
        return rc;
    // a member that joins mid-stream: its last stand-alone hop must have left its own stream
    for (ofp_hop_session* s : g->members)
        if (int rc = retire_last_hop(s)) return rc;
    // code loading and the kernel attribute may not happen during capture: one launch that touches nothing
    auto launch = [&](int dry) {
        return with_n_fft(g->n_fft, [&](auto f) {
            return with_hit_kind(g->loc, g->reg, g->pair, [&](auto k) {
                return hop_group_launch<decltype(f)::value, decltype(k)::value>(g, dry);
            });
        });
    };
    if (int rc = launch(1)) return rc;
    OFP_HIP(hipStreamSynchronize(g->stream));
    return capture_graph(g->stream, [&] { return launch(0); }, &g->graph, &g->exec);
}

// What a hit stage owns of its session: its argument struct (largs / rargs / pargs), its LDS size (lds_loc / lds_reg /
// lds_pair) and its device allocations.
template <class StageArgs>
struct StageOwned {
    StageArgs& args;
    size_t& lds;
    void** dev[3];
};

// Attaches a hit stage that has passed its setter's checks: fill() makes the stage's allocations and fills its
// arguments, the rest is the same for every stage.  The record mirror of the fused form belongs to the stage that finds
// none (a regressor after a locator shares the locator's).  If anything from the first allocation on fails, the session
// is again exactly the one it was and a later call is accepted.
// (No stage is refused by the LDS bound that was accepted without it: ofp_paired_cfg allows the voting locator 96 KiB.)
template <class StageArgs, class Fill>
int attach_stage(ofp_hop_session* s, const char* who, size_t lds, Fill fill, StageOwned<StageArgs> own) {
    OFP_REQUIRE(lds <= 128 * 1024, "%s: %zu bytes of LDS needed", who, lds);
    const size_t lds_fused = s->lds_fused;
    const bool own_mirror = s->fused && !s->d_mirror;
    auto attach = [&]() -> int {
        if (int rc = fill()) return rc;
        own.lds = lds;
        if (own_mirror) {
            OFP_HIP(hipMalloc(&s->d_mirror, (size_t)s->C * sizeof(ofp_onset)));
            OFP_HIP(hipMemset(s->d_mirror, 0, (size_t)s->C * sizeof(ofp_onset)));
            s->sargs.mirror = s->d_mirror;
        }
        if (s->fused) s->lds_fused = std::max(s->lds_fused, lds);
        own.args.enabled = 1;
        return capture_hop(s);
    };
    const int rc = attach();
    if (rc == OFP_OK) return OFP_OK;
    const std::string why = ofp::err_buf();
    for (void** p : {own.dev[0], own.dev[1], own.dev[2], own_mirror ? (void**)&s->d_mirror : nullptr}) {
        if (p && *p) (void)hipFree(*p);
        if (p) *p = nullptr;
    }
    std::memset(&own.args, 0, sizeof(StageArgs));
    if (own_mirror) s->sargs.mirror = nullptr;
    s->lds_fused = lds_fused;
    own.lds = 0;
    if (!s->exec) (void)capture_hop(s);  // (the failure came after the earlier graph had been given up)
    return ofp::fail(rc, "%s", why.c_str());
}

// The bounds of a grouping stage whose window reaches `before` samples before its anchor and `after` samples after it
// (INTEGRATION.md): a group is evaluated at most K hops after the hop that closes it; that bounds the groups pending
// at once and the oldest row a window still needs.  realtime.regress_hold_hops, regress_pending_bound and
// regress_ring_rows state the same arithmetic.
int grouping_bounds(const ofp_hop_session* s, const char* who, int64_t D, int64_t before, int64_t after) {
    const int64_t B = s->B, span = D + after;
    const int64_t K = std::max<int64_t>(0, (span + B - 1) / B - 1);
    const int64_t pending = std::min<int64_t>(K + 1, (K * B + D - 1) / (D + 1) + 1);
    OFP_REQUIRE(pending <= OFP_REG_QUEUE, "%s: up to %lld groups can be pending, the queue holds %d", who, (long long)pending,
                OFP_REG_QUEUE);
    const int64_t rows = D + before + (K + 1) * B;
    OFP_REQUIRE(s->R >= rows, "%s: the ring (%lld rows) must hold the oldest row a pending window can need plus one hop (%lld)",
                who, (long long)s->R, (long long)rows);
    return OFP_OK;
}

}  // namespace

extern "C" {

int ofp_hop_destroy(ofp_hop_session* s) {
    if (!s) return OFP_OK;
    OFP_NOT_IN_GROUP(s, "ofp_hop_destroy");
    if (s->stream) (void)hipStreamSynchronize(s->stream);
    if (s->exec) (void)hipGraphExecDestroy(s->exec);
    if (s->graph) (void)hipGraphDestroy(s->graph);
    void* dev[] = {s->d_state, s->d_hop, s->d_ring, s->d_ctl, s->d_twM, s->d_twF, s->d_win, s->d_wsym, s->d_tgw, s->d_sg, s->d_fb_i, s->d_fb_w,
                   s->d_prm, s->d_res, s->d_loc_state, s->d_loc_prm, s->d_mirror, s->d_reg_state, s->d_reg_prm, s->d_reg_ws,
                   s->d_pair_state};
    for (void* p : dev)
        if (p) (void)hipFree(p);
    if (s->h_hop) (void)hipHostFree(s->h_hop);
    if (s->h_res) (void)hipHostFree(s->h_res);
    if (s->stream) (void)hipStreamDestroy(s->stream);
    delete s;
    return OFP_OK;
}

int ofp_hop_create(ofp_detector* det, const ofp_hop_config* cfg, ofp_hop_session** out) {
    OFP_REQUIRE(det && cfg && out, "ofp_hop_create: NULL argument");
    const int C = det->p.n_channels, B = det->p.block_size;
    OFP_REQUIRE(C <= 1024, "ofp_hop_create: at most 1024 channels (got %d)", C);
    MlpPlan plan;
    std::memset(&plan, 0, sizeof(plan));
    if (cfg->mlp) plan = cfg->mlp->plan;
    size_t lds = 0, lds_strength = 0;  // of the spectral and the strength workgroup
    int fused_threads = 0;
    if (int rc = with_n_fft(cfg->n_fft, [&](auto f) {
            constexpr int F = decltype(f)::value;
            fused_threads = FusedCfg<F>::WGS;
            LdsSize spectral, strength;
            SpectralLds<F>(spectral, cfg->fb_nnz, cfg->n_mels, plan, B);
            lds = spectral.bytes + 64;  // (sizing slack)
            if (cfg->strength) {
                StrengthLds<F>(strength, B, C, cfg->tg_win_length);
                lds_strength = strength.bytes + (F > 1024 ? F / 4 : 0);  // (padding no frame above 1024 has, but
                                                                         //  earlier versions counted: no total shrinks)
            }
            return OFP_OK;
        }))
        return rc;
    OFP_REQUIRE(cfg->ring_samples >= cfg->n_fft && cfg->ring_samples >= B,
                "ofp_hop_create: the ring buffer (%lld rows) must hold n_fft = %d and one hop = %d samples",
                (long long)cfg->ring_samples, cfg->n_fft, B);
    OFP_REQUIRE(cfg->n_mels >= 1 && cfg->fb_lo && cfg->fb_len && cfg->fb_off && cfg->fb_w && cfg->fb_nnz >= 1,
                "ofp_hop_create: NULL / empty filterbank");
    OFP_REQUIRE(cfg->fb_nnz <= 4 * (cfg->n_fft / 2 + 1), "ofp_hop_create: filterbank with %d weights for %d bins",
                cfg->fb_nnz, cfg->n_fft / 2 + 1);
    OFP_REQUIRE(cfg->n_mels <= 127 && cfg->fb_nnz / MEL_SEG + cfg->n_mels <= MEL_MAXSEG,
                "ofp_hop_create: at most 127 bands and %d 32-tap segments", MEL_MAXSEG);
    OFP_REQUIRE(!cfg->strength || (cfg->strength_ring >= 1 && cfg->max_length >= 1 && cfg->avg_length >= 1 &&
                                   cfg->max_length <= cfg->strength_ring && cfg->avg_length <= cfg->strength_ring),
                "ofp_hop_create: onset strength needs 1 <= max_length, avg_length <= strength_ring");
    OFP_REQUIRE(cfg->tg_win_length >= 0 && cfg->tg_win_length <= 4096 && (cfg->tg_win_length == 0 || (cfg->strength && cfg->tg_win_length <= cfg->strength_ring && cfg->tg_win_length >= 2)),
                "ofp_hop_create: the tempogram needs the onset strength and 2 <= tg_win_length <= min(strength_ring, 4096)");
    OFP_REQUIRE(!cfg->mlp || cfg->mlp->plan.dims[0] == cfg->n_mels,
                "ofp_hop_create: the classifier takes %d inputs, the filterbank has %d bands",
                cfg->mlp ? cfg->mlp->plan.dims[0] : 0, cfg->n_mels);
    OFP_REQUIRE(lds <= 160 * 1024, "ofp_hop_create: %zu bytes of LDS needed, 160 KiB available", lds);
    OFP_REQUIRE(lds_strength <= 160 * 1024, "ofp_hop_create: the hop (%d x %d samples) does not fit the LDS", B, C);
    ofp_hop_session* s = new (std::nothrow) ofp_hop_session();
    if (!s) return ofp::fail(OFP_ERR_INVALID, "out of host memory");
    s->det = det;
    s->C = C;
    s->B = B;
    s->n_fft = cfg->n_fft;
    s->n_mels = cfg->n_mels;
    s->R = cfg->ring_samples;
    s->want_rel = cfg->want_rel ? 1 : 0;
    s->n_out = cfg->mlp ? plan.dims[plan.n_layers] : 0;
    auto up8 = [](int64_t v) { return (v + 7) / 8 * 8; };
    s->o_logits = up8(s->o_rec + (int64_t)C * (int64_t)sizeof(ofp_onset));
    s->o_mel = up8(s->o_logits + (int64_t)C * s->n_out * 4);
    s->o_rel = up8(s->o_mel + (int64_t)C * s->n_mels * 4);
    s->o_sg = up8(s->o_rel + (s->want_rel ? (int64_t)B * C * 4 : 0));
    s->o_loc = up8(s->o_sg + 16 + (cfg->strength ? 4 * (int64_t)cfg->tg_win_length : 0));
    s->o_reg = up8(s->o_loc + (int64_t)sizeof(HopLocBlock));
    s->o_pair = up8(s->o_reg + (int64_t)sizeof(HopRegBlock));
    s->res_bytes = up8(s->o_pair + (int64_t)sizeof(HopPairBlock));
    const int M = s->n_fft / 2;
    s->lds = lds;
    s->lds_strength = lds_strength;
    int rc = OFP_OK;
    auto fail = [&](int code) {
        ofp_hop_destroy(s);
        return code;
    };
#define HOP_TRY(call)                                                                                           \
    do {                                                                                                        \
        hipError_t e__ = (call);                                                                                \
        if (e__ != hipSuccess) {                                                                                \
            ofp_hop_destroy(s);                                                                                 \
            return ofp::fail(OFP_ERR_HIP, "%s failed: %s", #call, hipGetErrorString(e__));                      \
        }                                                                                                       \
    } while (0)
    HOP_TRY(hipGetDevice(&s->device));
    HOP_TRY(hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking));
    const int64_t sb = ofp_stream_state_bytes(det);
    HOP_TRY(hipMalloc(&s->d_state, (size_t)sb));
    HOP_TRY(hipMalloc(&s->d_hop, (size_t)B * C * 4));
    HOP_TRY(hipMalloc(&s->d_ring, (size_t)s->R * C * 4));
    HOP_TRY(hipMalloc(&s->d_ctl, 16));
    HOP_TRY(hipMalloc(&s->d_twM, (size_t)M * 8));
    HOP_TRY(hipMalloc(&s->d_twF, (size_t)(M + 2) * 8));
    HOP_TRY(hipMalloc(&s->d_win, (size_t)s->n_fft * 4));
    HOP_TRY(hipMalloc(&s->d_wsym, (size_t)s->n_fft * 4));
    HOP_TRY(hipMalloc(&s->d_fb_i, (size_t)3 * s->n_mels * 4));
    HOP_TRY(hipMalloc(&s->d_fb_w, (size_t)cfg->fb_nnz * 4));
    HOP_TRY(hipMalloc(&s->d_res, (size_t)s->res_bytes));
    HOP_TRY(hipHostMalloc((void**)&s->h_hop, (size_t)B * C * 4, hipHostMallocMapped));
    HOP_TRY(hipHostMalloc((void**)&s->h_res, (size_t)s->res_bytes, hipHostMallocMapped));
    std::memset(s->h_res, 0, (size_t)s->res_bytes);
    std::memset(s->h_hop, 0, (size_t)B * C * 4);
    HOP_TRY(hipMemcpy(s->d_fb_i, cfg->fb_lo, (size_t)s->n_mels * 4, hipMemcpyHostToDevice));
    HOP_TRY(hipMemcpy(s->d_fb_i + s->n_mels, cfg->fb_len, (size_t)s->n_mels * 4, hipMemcpyHostToDevice));
    HOP_TRY(hipMemcpy(s->d_fb_i + 2 * s->n_mels, cfg->fb_off, (size_t)s->n_mels * 4, hipMemcpyHostToDevice));
    HOP_TRY(hipMemcpy(s->d_fb_w, cfg->fb_w, (size_t)cfg->fb_nnz * 4, hipMemcpyHostToDevice));
    if (cfg->mlp) {  // the session keeps its own copy: the handle may be destroyed afterwards
        HOP_TRY(hipMalloc(&s->d_prm, (size_t)plan.n_params * 4));
        HOP_TRY(hipMemcpy(s->d_prm, cfg->mlp->d_params, (size_t)plan.n_params * 4, hipMemcpyDeviceToDevice));
        plan.params = s->d_prm;
    }
    HopArgs& a = s->args;
    std::memset(&a, 0, sizeof(a));
    std::memset(&s->largs, 0, sizeof(s->largs));
    std::memset(&s->rargs, 0, sizeof(s->rargs));
    std::memset(&s->pargs, 0, sizeof(s->pargs));
    a.C = C;
    a.B = B;
    a.n_mels = s->n_mels;
    a.nnz = cfg->fb_nnz;
    a.R = s->R;
    a.ctl = s->d_ctl;
    a.hop = s->d_hop;
    a.ring = s->d_ring;
    a.twM = s->d_twM;
    a.twF = s->d_twF;
    a.win = s->d_win;
    a.flo = s->d_fb_i;
    a.flen = s->d_fb_i + s->n_mels;
    a.foff = s->d_fb_i + 2 * s->n_mels;
    a.fw = s->d_fb_w;
    a.plan = plan;
    if (cfg->strength) {
        const int bins = s->n_fft / 2 + 1;
        s->sg_floats = (size_t)bins + 4 + (size_t)cfg->strength_ring;
        HOP_TRY(hipMalloc(&s->d_sg, s->sg_floats * 4));
        StrengthArgs& g = a.sg;
        g.enabled = 1;
        g.n_ring = cfg->strength_ring;
        g.max_length = cfg->max_length;
        g.avg_length = cfg->avg_length;
        g.ls_alpha = cfg->ls_alpha;
        g.ls_minmax = cfg->ls_minmax;
        g.oe_alpha = cfg->oe_alpha;
        g.oe_minmin = cfg->oe_minmin;
        g.wsym = s->d_wsym;
        g.prev = s->d_sg;
        g.st = s->d_sg + bins;
        g.ring = s->d_sg + bins + 4;
        s->sg_init[0] = cfg->ls_max0;
        s->sg_init[1] = cfg->oe_min0;
        s->sg_init[2] = cfg->oe_max0;
        g.tg_len = cfg->tg_win_length;
        g.tgw = nullptr;
        if (cfg->tg_win_length > 0) {  // scipy.signal.windows.hann(W) (symmetric) as float32 (recording.py:250)
            const int W = cfg->tg_win_length;
            std::vector<float> w(W);
            for (int i = 0; i < W; ++i) w[i] = (float)(0.5 - 0.5 * cos(2.0 * 3.14159265358979323846 * i / (W - 1)));
            HOP_TRY(hipMalloc(&s->d_tgw, (size_t)W * 4));
            HOP_TRY(hipMemcpy(s->d_tgw, w.data(), (size_t)W * 4, hipMemcpyHostToDevice));
            g.tgw = s->d_tgw;
        }
    }
    // Fused form (one launch per hop, hop and result block in pinned host memory) whenever the detector
    // fits one workgroup of the fused kernel; OFP_HOP_GRAPH=nodes keeps the five-node graph.
    {
        const char* mode = getenv("OFP_HOP_GRAPH");
        const size_t par_lds = (size_t)3 * B * C * sizeof(float);
        s->fused = !(mode && mode[0] == 'n') && 2 * C <= fused_threads && C <= ofpstream::PAR_MAX_C &&
                   par_lds <= 96 * 1024;
        s->lds_fused = std::max(std::max(s->lds, par_lds), s->lds_strength);
        point_results(s, s->d_res);
        if (s->fused) {
            s->threads = fused_threads;
            float* dev_hop = nullptr;
            unsigned char* dev_res = nullptr;
            HOP_TRY(hipHostGetDevicePointer((void**)&dev_hop, s->h_hop, 0));
            HOP_TRY(hipHostGetDevicePointer((void**)&dev_res, s->h_res, 0));
            a.hop = dev_hop;
            ofpstream::StreamArgs& q = s->sargs;
            q = ofpstream::make_stream_args(det);
            q.state = s->d_state;
            q.x = dev_hop;
            q.n_blocks = 1;
            q.n_rows = 0;
            q.warmup = 0;
            q.sample_base = 0;
            q.cap = C;
            q.fresh_count = 1;
            point_results(s, dev_res);
        }
    }
    if ((rc = with_n_fft(s->n_fft, [&](auto f) { return hop_tables<decltype(f)::value>(s); })) != OFP_OK) return fail(rc);
    if ((rc = capture_hop(s)) != OFP_OK) return fail(rc);
#undef HOP_TRY
    *out = s;
    return OFP_OK;
}

int ofp_hop_reset(ofp_hop_session* s) {
    OFP_REQUIRE(s, "ofp_hop_reset: NULL session");
    if (s->owner)  // (the group's launches go to the group's stream, the reset to the session's)
        if (int rc = retire_last_hop(s)) return rc;
    return reset_state(s);
}

int ofp_hop_warmup(ofp_hop_session* s, const float* h_x, int64_t n_rows) {
    OFP_REQUIRE(s && (h_x || n_rows == 0), "ofp_hop_warmup: NULL argument");
    OFP_REQUIRE(!s->in_flight, "ofp_hop_warmup: a hop is in flight (collect it first)");
    if (n_rows <= 0) return OFP_OK;
    if (s->owner)
        if (int rc = retire_last_hop(s)) return rc;
    float* d = nullptr;
    OFP_HIP(hipMalloc(&d, (size_t)n_rows * s->C * 4));
    hipError_t e = hipMemcpyAsync(d, h_x, (size_t)n_rows * s->C * 4, hipMemcpyHostToDevice, s->stream);
    int rc = e == hipSuccess ? ofp_stream_process(s->det, s->d_state, d, 0, n_rows, 1, 0, nullptr, nullptr, 0, nullptr,
                                                  s->stream)
                             : ofp::fail(OFP_ERR_HIP, "ofp_hop_warmup: %s", hipGetErrorString(e));
    (void)hipStreamSynchronize(s->stream);
    s->retired = true;
    (void)hipFree(d);
    return rc;
}

int ofp_hop_submit(ofp_hop_session* s, const float* h_hop) {
    OFP_REQUIRE(s && h_hop, "ofp_hop_submit: NULL argument");
    OFP_NOT_IN_GROUP(s, "ofp_hop_submit");
    OFP_REQUIRE(!s->in_flight, "ofp_hop_submit: the previous hop has not been collected");
    std::memcpy(s->h_hop, h_hop, (size_t)s->B * s->C * sizeof(float));
    OFP_HIP(hipGraphLaunch(s->exec, s->stream));
    s->in_flight = true;
    s->pushed += 1;
    return OFP_OK;
}

int ofp_hop_collect(ofp_hop_session* s, int64_t* n_onsets, ofp_onset* h_records, float* h_logits, float* h_mel,
                    float* h_rel, float* h_strength) {
    OFP_REQUIRE(s, "ofp_hop_collect: NULL session");
    OFP_REQUIRE(s->in_flight, "ofp_hop_collect: no hop in flight");
    if (s->fused) {
        if (int rc = wait_done(s, hop_stream(s))) return rc;
        __atomic_thread_fence(__ATOMIC_ACQUIRE);
        s->retired = false;  // the kernel has published its results; it may not have retired from the stream yet
    } else {
        OFP_HIP(hipStreamSynchronize(s->stream));
        s->retired = true;
    }
    s->in_flight = false;
    const unsigned char* r = s->h_res;
    int64_t count, index;
    std::memcpy(&count, r + s->o_count, 8);
    std::memcpy(&index, r + s->o_index, 8);
    if (index != s->pushed - 1)
        return ofp::fail(OFP_ERR_HIP, "ofp_hop_collect: result block of hop %lld, expected %lld", (long long)index,
                         (long long)(s->pushed - 1));
    if (n_onsets) *n_onsets = count;
    if (h_records) {
        const int64_t n = count < s->C ? count : s->C;
        std::memcpy(h_records, r + s->o_rec, (size_t)n * sizeof(ofp_onset));
        for (int64_t i = 0; i < n; ++i) h_records[i].sample += index * s->B;  // audio.py:65: current_index + delta
    }
    if (h_logits && s->n_out) std::memcpy(h_logits, r + s->o_logits, (size_t)s->C * s->n_out * 4);
    if (h_mel) std::memcpy(h_mel, r + s->o_mel, (size_t)s->C * s->n_mels * 4);
    if (h_rel && s->want_rel) std::memcpy(h_rel, r + s->o_rel, (size_t)s->B * s->C * 4);
    if (h_strength && s->args.sg.enabled) std::memcpy(h_strength, r + s->o_sg, 16 + (size_t)4 * s->args.sg.tg_len);
    return OFP_OK;
}

int ofp_hop_push(ofp_hop_session* s, const float* h_hop, int64_t* n_onsets, ofp_onset* h_records, float* h_logits,
                 float* h_mel, float* h_rel, float* h_strength) {
    int rc = ofp_hop_submit(s, h_hop);
    if (rc != OFP_OK) return rc;
    return ofp_hop_collect(s, n_onsets, h_records, h_logits, h_mel, h_rel, h_strength);
}

int ofp_hop_ring_read(ofp_hop_session* s, int64_t n_rows, float* h_out) {
    OFP_REQUIRE(s && h_out && n_rows >= 0 && n_rows <= s->R, "ofp_hop_ring_read: bad argument");
    OFP_REQUIRE(!s->in_flight, "ofp_hop_ring_read: a hop is in flight (collect it first)");
    if (int rc = retire_last_hop(s)) return rc;
    // audio[-n_rows:] of the reference's CircularArray: the rows ending at the write cursor, oldest first
    const int64_t end = s->pushed * s->B;
    const size_t row = (size_t)s->C * 4;
    for (int64_t done = 0; done < n_rows;) {
        const int64_t t = end - n_rows + done;
        const int64_t p = ((t % s->R) + s->R) % s->R;
        const int64_t run = std::min<int64_t>(n_rows - done, s->R - p);
        OFP_HIP(hipMemcpy(h_out + done * s->C, reinterpret_cast<char*>(s->d_ring) + p * row, (size_t)run * row,
                          hipMemcpyDeviceToHost));
        done += run;
    }
    return OFP_OK;
}

// ofp_hop_set_locator and ofp_hop_set_locator_2d behind their own checks: T is the checked launch form of `loc`
// (T.planar: the kind; a planar locator reads no section, so no ring-length condition applies to it)
static int hop_attach_locator(ofp_hop_session* s, const ofp_hop_locator* loc, ofp::LocTables T, const char* who) {
    OFP_REQUIRE(s->pushed == 0 && !s->in_flight, "%s: the session has already taken a hop", who);
    OFP_REQUIRE(!s->largs.enabled && !s->pargs.enabled, "%s: the session already has a locator", who);
    OFP_REQUIRE(!s->rargs.enabled, "%s: the session already has a regressor (attach the locator first)", who);
    OFP_REQUIRE(loc->S == s->C, "%s: %d sensors for %d channels", who, loc->S, s->C);
    OFP_REQUIRE(!s->det->p.backtrack, "%s: a detector that backtracks moves onsets behind the hop", who);
    OFP_REQUIRE(!T.use_audio || s->R >= (int64_t)loc->max_section + s->B,
                "%s: the ring (%lld rows) must hold the longest section (%d) and one hop (%d)", who, (long long)s->R,
                loc->max_section, s->B);
    const size_t lds = ofp::loc_lds_bytes(s->threads, T.max_section, T.plan, (size_t)s->B * s->C * 4);  // (+ the hop rows)
    auto fill = [&]() -> int {
        if (loc->mlp) {  // the session keeps its own copy: the handle may be destroyed afterwards
            OFP_HIP(hipMalloc(&s->d_loc_prm, (size_t)T.plan.n_params * 4));
            OFP_HIP(hipMemcpy(s->d_loc_prm, loc->mlp->d_params, (size_t)T.plan.n_params * 4, hipMemcpyDeviceToDevice));
            T.plan.params = s->d_loc_prm;
        }
        OFP_HIP(hipMalloc(&s->d_loc_state, sizeof(ofp_locate_state)));
        OFP_HIP(hipMemset(s->d_loc_state, 0, sizeof(ofp_locate_state)));
        s->largs.T = T;
        s->largs.state = s->d_loc_state;
        s->largs.out = reinterpret_cast<HopLocBlock*>(s->res_dev + s->o_loc);
        return OFP_OK;
    };
    return attach_stage(s, who, lds, fill,
                        StageOwned<HopLocArgs>{s->largs, s->lds_loc, {(void**)&s->d_loc_prm, (void**)&s->d_loc_state}});
}

int ofp_hop_set_locator(ofp_hop_session* s, const ofp_hop_locator* loc) {
    OFP_REQUIRE(s && loc, "ofp_hop_set_locator: NULL argument");
    OFP_NOT_IN_GROUP(s, "ofp_hop_set_locator");
    ofp::LocTables T;
    if (int rc = ofp_locate_tables(loc, "ofp_hop_set_locator", &T)) return rc;
    return hop_attach_locator(s, loc, T, "ofp_hop_set_locator");
}

int ofp_hop_set_locator_2d(ofp_hop_session* s, const ofp_hop_locator* loc) {
    OFP_REQUIRE(s && loc, "ofp_hop_set_locator_2d: NULL argument");
    OFP_NOT_IN_GROUP(s, "ofp_hop_set_locator_2d");
    ofp::LocTables T;
    if (int rc = ofp_locate_tables_2d(loc, "ofp_hop_set_locator_2d", &T)) return rc;
    return hop_attach_locator(s, loc, T, "ofp_hop_set_locator_2d");
}

int ofp_hop_collect_location(ofp_hop_session* s, int32_t* status, double* h_xy, int32_t* n_members,
                             int32_t* h_sensors, int64_t* h_onsets, int32_t* fed, int32_t* dropped, int32_t* flags) {
    OFP_REQUIRE(s, "ofp_hop_collect_location: NULL session");
    OFP_REQUIRE(s->largs.enabled, "ofp_hop_collect_location: the session has no locator");
    OFP_REQUIRE(!s->in_flight && s->pushed > 0, "ofp_hop_collect_location: no collected hop");
    HopLocBlock b;
    std::memset(&b, 0, sizeof(b));
    int64_t count;
    std::memcpy(&count, s->h_res + s->o_count, 8);
    if (count > 0) std::memcpy(&b, s->h_res + s->o_loc, sizeof(b));  // a hop without onsets leaves the block alone
    if (status) *status = b.status;
    if (h_xy) {
        h_xy[0] = b.xy[0];
        h_xy[1] = b.xy[1];
    }
    if (n_members) *n_members = b.n_members;
    if (h_sensors) std::memcpy(h_sensors, b.sens, sizeof(b.sens));
    if (h_onsets) std::memcpy(h_onsets, b.on, sizeof(b.on));
    if (fed) *fed = b.fed;
    if (dropped) *dropped = b.dropped;
    if (flags) *flags = b.flags;
    return OFP_OK;
}

int ofp_hop_locator_state(ofp_hop_session* s, ofp_locate_state* h_state) {
    OFP_REQUIRE(s && h_state, "ofp_hop_locator_state: NULL argument");
    OFP_REQUIRE(s->largs.enabled, "ofp_hop_locator_state: the session has no locator");
    OFP_REQUIRE(!s->in_flight, "ofp_hop_locator_state: a hop is in flight (collect it first)");
    if (int rc = retire_last_hop(s)) return rc;
    OFP_HIP(hipMemcpy(h_state, s->d_loc_state, sizeof(ofp_locate_state), hipMemcpyDeviceToHost));
    return OFP_OK;
}

int ofp_hop_set_regressor(ofp_hop_session* s, const ofp_hop_regressor* r) {
    const char* who = "ofp_hop_set_regressor";
    OFP_REQUIRE(s && r, "%s: NULL argument", who);
    OFP_NOT_IN_GROUP(s, "ofp_hop_set_regressor");
    OFP_REQUIRE(s->pushed == 0 && !s->in_flight, "%s: the session has already taken a hop", who);
    OFP_REQUIRE(!s->rargs.enabled, "%s: the session already has a regressor", who);
    OFP_REQUIRE(!s->pargs.enabled, "%s: the session has a voting locator (the two grouping stages do not share a session)", who);
    ofpreg::Plan plan;
    if (int rc = ofp_regress_plan(r, who, &plan)) return rc;
    OFP_REQUIRE(r->channels == s->C, "%s: the model takes %d channels, the session has %d", who, r->channels, s->C);
    OFP_REQUIRE(!s->det->p.backtrack, "%s: a detector that backtracks moves onsets behind the hop", who);
    OFP_REQUIRE(r->max_distance >= s->B, "%s: max_distance %d is shorter than one hop (%d): two groups could close in one hop",
                who, r->max_distance, s->B);
    if (int rc = grouping_bounds(s, who, r->max_distance, r->pre_samples, (int64_t)r->frame_length - r->pre_samples)) return rc;
    auto fill = [&]() -> int {
        OFP_HIP(hipMalloc(&s->d_reg_prm, (size_t)plan.n_params * 4));
        OFP_HIP(hipMemcpy(s->d_reg_prm, r->d_params, (size_t)plan.n_params * 4, hipMemcpyDeviceToDevice));
        plan.params = s->d_reg_prm;
        OFP_HIP(hipMalloc(&s->d_reg_state, sizeof(ofp_regress_state)));
        OFP_HIP(hipMemset(s->d_reg_state, 0, sizeof(ofp_regress_state)));
        if (!plan.use_lds) OFP_HIP(hipMalloc(&s->d_reg_ws, (size_t)2 * plan.act_floats * 4));
        ofpreg::Cfg& g = s->rargs.g;
        g.plan = plan;
        g.B = s->B;
        g.F = r->frame_length;
        g.pre = r->pre_samples;
        g.D = r->max_distance;
        g.min_channels = r->min_channels;
        g.state = s->d_reg_state;
        g.ws = s->d_reg_ws;
        s->rargs.out = reinterpret_cast<HopRegBlock*>(s->res_dev + s->o_reg);
        return OFP_OK;
    };
    return attach_stage(s, who, ofpreg::lds_bytes(plan), fill,
                        StageOwned<HopRegArgs>{s->rargs, s->lds_reg,
                                               {(void**)&s->d_reg_prm, (void**)&s->d_reg_state, (void**)&s->d_reg_ws}});
}

int ofp_hop_collect_hit(ofp_hop_session* s, int32_t* status, int64_t* start, int64_t* h_row, float* h_y, int32_t* flags) {
    OFP_REQUIRE(s, "ofp_hop_collect_hit: NULL session");
    OFP_REQUIRE(s->rargs.enabled, "ofp_hop_collect_hit: the session has no regressor");
    OFP_REQUIRE(!s->in_flight && s->pushed > 0, "ofp_hop_collect_hit: no collected hop");
    HopRegBlock b;
    std::memcpy(&b, s->h_res + s->o_reg, sizeof(b));
    const bool hit = b.hop == s->pushed;  // (a hop that evaluates nothing leaves the block of an earlier one)
    if (status) *status = hit ? 1 : 0;
    if (flags) *flags = b.flags;
    if (!hit) return OFP_OK;
    if (start) *start = b.start;
    if (h_row) std::memcpy(h_row, b.row, (size_t)s->C * sizeof(int64_t));
    if (h_y) std::memcpy(h_y, b.y, (size_t)s->rargs.g.plan.n_out * sizeof(float));
    return OFP_OK;
}

int ofp_hop_set_locator_paired(ofp_hop_session* s, const ofp_hop_paired* p) {
    const char* who = "ofp_hop_set_locator_paired";
    OFP_REQUIRE(s && p, "%s: NULL argument", who);
    OFP_NOT_IN_GROUP(s, "ofp_hop_set_locator_paired");
    OFP_REQUIRE(s->pushed == 0 && !s->in_flight, "%s: the session has already taken a hop", who);
    OFP_REQUIRE(!s->pargs.enabled && !s->largs.enabled, "%s: the session already has a locator", who);
    OFP_REQUIRE(!s->rargs.enabled, "%s: the session has a regressor (the two grouping stages do not share a session)", who);
    ofppair::Cfg g;
    if (int rc = ofp_paired_cfg(p, who, &g)) return rc;
    OFP_REQUIRE(p->S == s->C, "%s: %d sensors for %d channels", who, p->S, s->C);
    OFP_REQUIRE(!s->det->p.backtrack, "%s: a detector that backtracks moves onsets behind the hop", who);
    OFP_REQUIRE(p->max_distance >= s->B, "%s: max_distance %d is shorter than one hop (%d): two groups could close in one hop",
                who, p->max_distance, s->B);
    if (int rc = grouping_bounds(s, who, p->max_distance, p->left, p->right)) return rc;
    auto fill = [&]() -> int {
        OFP_HIP(hipMalloc(&s->d_pair_state, sizeof(ofp_regress_state)));
        OFP_HIP(hipMemset(s->d_pair_state, 0, sizeof(ofp_regress_state)));
        g.B = s->B;
        g.state = s->d_pair_state;
        s->pargs.g = g;
        s->pargs.out = reinterpret_cast<HopPairBlock*>(s->res_dev + s->o_pair);
        return OFP_OK;
    };
    return attach_stage(s, who, ofppair::lds_bytes(g.F, g.side), fill,
                        StageOwned<HopPairArgs>{s->pargs, s->lds_pair, {(void**)&s->d_pair_state}});
}

int ofp_hop_collect_cc_hit(ofp_hop_session* s, int32_t* hit, int32_t* status, int64_t* onset, int32_t* first,
                           int64_t* h_row, int32_t* h_lags, int32_t* cell, double* h_xy, double* h_rphi, int32_t* flags) {
    OFP_REQUIRE(s, "ofp_hop_collect_cc_hit: NULL session");
    OFP_REQUIRE(s->pargs.enabled, "ofp_hop_collect_cc_hit: the session has no voting locator");
    OFP_REQUIRE(!s->in_flight && s->pushed > 0, "ofp_hop_collect_cc_hit: no collected hop");
    HopPairBlock b;
    std::memcpy(&b, s->h_res + s->o_pair, sizeof(b));
    const bool got = b.hop == s->pushed;  // (a hop that evaluates nothing leaves the block of an earlier one)
    if (hit) *hit = got ? 1 : 0;
    if (flags) *flags = b.flags;
    if (!got) return OFP_OK;
    if (status) *status = b.status;
    if (onset) *onset = b.onset;
    if (first) *first = b.first;
    if (h_row) std::memcpy(h_row, b.row, (size_t)s->C * sizeof(int64_t));
    if (h_lags) std::memcpy(h_lags, b.lags, sizeof(b.lags));
    if (cell) *cell = b.cell;
    if (h_xy) std::memcpy(h_xy, b.xy, sizeof(b.xy));
    if (h_rphi) std::memcpy(h_rphi, b.rphi, sizeof(b.rphi));
    return OFP_OK;
}

int ofp_hop_group_create(ofp_hop_session* const* sessions, int n, ofp_hop_group** out) {
    OFP_REQUIRE(sessions && out, "ofp_hop_group_create: NULL argument");
    OFP_REQUIRE(n >= 1 && n <= 1024, "ofp_hop_group_create: 1..1024 members (got %d)", n);
    const ofp_hop_session* f = sessions[0];
    size_t lds = 0;
    for (int i = 0; i < n; ++i) {
        const ofp_hop_session* s = sessions[i];
        OFP_REQUIRE(s, "ofp_hop_group_create: member %d is NULL", i);
        for (int j = 0; j < i; ++j)
            OFP_REQUIRE(sessions[j] != s, "ofp_hop_group_create: members %d and %d are the same session", j, i);
        OFP_REQUIRE(!s->owner, "ofp_hop_group_create: member %d already belongs to a group", i);
        OFP_REQUIRE(!s->in_flight, "ofp_hop_group_create: member %d has a hop in flight (collect it first)", i);
        OFP_REQUIRE(s->fused, "ofp_hop_group_create: member %d runs the five-node graph (OFP_HOP_GRAPH=nodes, or a shape "
                              "too wide for the one-kernel form); only one-kernel sessions can be grouped", i);
        OFP_REQUIRE(s->device == f->device, "ofp_hop_group_create: member %d lives on device %d, member 0 on device %d", i,
                    s->device, f->device);
        OFP_REQUIRE(s->n_fft == f->n_fft, "ofp_hop_group_create: member %d has n_fft %d, member 0 has %d", i, s->n_fft,
                    f->n_fft);
        OFP_REQUIRE(s->C == f->C, "ofp_hop_group_create: member %d has %d channels, member 0 has %d", i, s->C, f->C);
        OFP_REQUIRE(!s->args.sg.enabled == !f->args.sg.enabled,
                    "ofp_hop_group_create: members 0 and %d differ in having the onset strength enabled", i);
        OFP_REQUIRE(!s->largs.enabled == !f->largs.enabled, "ofp_hop_group_create: members 0 and %d differ in having a locator",
                    i);
        OFP_REQUIRE(!s->rargs.enabled == !f->rargs.enabled, "ofp_hop_group_create: members 0 and %d differ in having a regressor",
                    i);
        OFP_REQUIRE(!s->pargs.enabled == !f->pargs.enabled,
                    "ofp_hop_group_create: members 0 and %d differ in having a voting locator (paired)", i);
        lds = std::max(lds, s->lds_fused);
    }
    ofp_hop_group* g = new (std::nothrow) ofp_hop_group();
    if (!g) return ofp::fail(OFP_ERR_INVALID, "out of host memory");
    g->members.assign(sessions, sessions + n);
    g->device = f->device;
    g->n_fft = f->n_fft;
    g->grid_x = f->C + 1 + (f->args.sg.enabled ? 1 : 0);
    g->loc = f->largs.enabled != 0;
    g->reg = f->rargs.enabled != 0;
    g->pair = f->pargs.enabled != 0;
    g->lds = lds;
    int prev = 0;
    hipError_t e = hipGetDevice(&prev);
    if (e == hipSuccess && prev != g->device) e = hipSetDevice(g->device);
    int rc = e == hipSuccess ? group_build(g) : ofp::fail(OFP_ERR_HIP, "ofp_hop_group_create: %s", hipGetErrorString(e));
    if (e == hipSuccess && prev != g->device) (void)hipSetDevice(prev);
    if (rc != OFP_OK) {
        group_free(g);
        return rc;
    }
    for (ofp_hop_session* s : g->members) s->owner = g;
    *out = g;
    return OFP_OK;
}

int ofp_hop_group_destroy(ofp_hop_group* g) {
    if (!g) return OFP_OK;
    const hipError_t e = hipStreamSynchronize(g->stream);
    for (ofp_hop_session* s : g->members) {
        s->owner = nullptr;
        s->retired = true;
    }
    group_free(g);
    if (e != hipSuccess) return ofp::fail(OFP_ERR_HIP, "ofp_hop_group_destroy: %s", hipGetErrorString(e));
    return OFP_OK;
}

int ofp_hop_group_submit(ofp_hop_group* g, const float* const* h_hops) {
    OFP_REQUIRE(g && h_hops, "ofp_hop_group_submit: NULL argument");
    const size_t n = g->members.size();
    for (size_t i = 0; i < n; ++i) {
        OFP_REQUIRE(h_hops[i], "ofp_hop_group_submit: the hop of member %zu is NULL", i);
        OFP_REQUIRE(!g->members[i]->in_flight, "ofp_hop_group_submit: the previous hop of member %zu has not been collected",
                    i);
    }
    for (size_t i = 0; i < n; ++i) {
        ofp_hop_session* s = g->members[i];
        std::memcpy(s->h_hop, h_hops[i], (size_t)s->B * s->C * sizeof(float));
    }
    OFP_HIP(hipGraphLaunch(g->exec, g->stream));
    for (ofp_hop_session* s : g->members) {
        s->in_flight = true;
        s->retired = false;
        s->pushed += 1;
    }
    return OFP_OK;
}

int ofp_hop_group_wait(ofp_hop_group* g) {
    OFP_REQUIRE(g, "ofp_hop_group_wait: NULL group");
    // the members' completion words, as ofp_hop_collect polls its own; the members of one launch finish within
    // microseconds of each other, so the walk costs the slowest member's time, not the sum
    for (ofp_hop_session* s : g->members) {
        if (!s->in_flight) continue;
        bool synced = false;
        if (int rc = wait_done(s, g->stream, &synced)) return rc;
        if (synced) break;  // (the whole launch has left the stream)
    }
    __atomic_thread_fence(__ATOMIC_ACQUIRE);
    return OFP_OK;
}

}  // extern "C"
