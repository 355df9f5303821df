// The library's one Fourier-resample arithmetic (scipy.signal.resample: real input, time domain, no window) as device
// functions, for k_resample (csrc/ofp_post.hip) and k_stretch_windows (csrc/ofp_train_random.h): both give the same
// bits for the same samples and the same (Nx, num).  The spectrum is taken and synthesised directly: a DFT with
// tabulated fp64 twiddles indexed by k n mod Nx and k m mod num (the lengths are arbitrary, a few hundred samples),
// fp64 sums in ascending n and k, the Nyquist rules of the shorter length, one rounding to fp32.  The kernels differ
// only in how they spread these calls over their threads.  (Compiled with -ffp-contract=off: no operation is fused.)
#pragma once
#include <hip/hip_runtime.h>

namespace {

// e^{-2 pi i j / Nx}: the forward table's entry j < Nx
__device__ __forceinline__ double2 resample_twx(int j, int Nx) {
    double s, co;
    sincospi(-2.0 * (double)j / (double)Nx, &s, &co);
    return make_double2(co, s);
}

// e^{+2 pi i j / num}: the synthesis table's entry j < num
__device__ __forceinline__ double2 resample_twy(int j, int num) {
    double s, co;
    sincospi(2.0 * (double)j / (double)num, &s, &co);
    return make_double2(co, s);
}

// bins 0 .. resample_bins(Nx, num) of the rfft survive
__device__ __forceinline__ int resample_bins(int Nx, int num) { return min(num, Nx) / 2; }

// rfft bin k <= K of the Nx samples xs[0], xs[stride], ..., scaled where it is the Nyquist bin of the shorter length
__device__ __forceinline__ double2 resample_bin(const float* xs, int stride, const double2* twx, int Nx, int num,
                                                int k) {
    const int N = min(num, Nx), K = N / 2;
    double re = 0.0, im = 0.0;
    int ph = 0;  // k * n mod Nx
    for (int n = 0; n < Nx; ++n) {
        const double v = (double)xs[n * stride];
        re += v * twx[ph].x;
        im += v * twx[ph].y;
        ph += k;
        if (ph >= Nx) ph -= Nx;
    }
    if (N % 2 == 0 && k == K) {  // the Nyquist component of the shorter length
        if (num < Nx) { re *= 2.0; im *= 2.0; }
        else if (Nx < num) { re *= 0.5; im *= 0.5; }
    }
    return make_double2(re, im);
}

// output sample m < num from the bins Y[0], Y[stride], ..., Y[K stride]: irfft's 1/num, then y *= num / Nx
__device__ __forceinline__ float resample_sample(const double2* Y, int stride, const double2* twy, int Nx, int num,
                                                 int m) {
    const int K = resample_bins(Nx, num);
    const double scale = ((double)num / (double)Nx) / (double)num;
    double acc = Y[0].x;
    int ph = 0;  // k * m mod num
    for (int k = 1; k <= K; ++k) {
        ph += m;
        if (ph >= num) ph -= num;
        const double2* y = Y + k * stride;
        if (2 * k == num) acc += y->x * twy[ph].x;  // irfft takes the last bin of an even length as real
        else acc += 2.0 * (y->x * twy[ph].x - y->y * twy[ph].y);
    }
    return (float)(acc * scale);
}

}  // namespace
