// Device functions of the small cross-correlations shared by ofp_xcorr.hip (the batched entry points) and
// ofp_locate_dev.h (the locate state machine): Python's slice bounds, one entry of the normalised correlation
// (cross_correlation_lag, reference detection.py:195-268) and adjust_onset (:299-352).  One definition, so the
// host-driven chain and the in-graph locator produce the same integers.
#pragma once
#include "ofp_common.h"
#include "ofp_xcorr_canon.h"

namespace ofp {

constexpr int XCORR_WAVE = 64;  // adjust_onset_wave's lane count (fixes its summation order)

// Python's a[start:stop] on an array of `len`: negative indices wrap once, then clamp.
__device__ __forceinline__ void py_slice(int start, int stop, int len, int* lo, int* hi) {
    if (start < 0) start = max(start + len, 0);
    if (stop < 0) stop = max(stop + len, 0);
    start = min(start, len);
    stop = min(stop, len);
    *lo = start;
    *hi = max(stop, start);
}

// Entry j of the normalised full correlation of xs, ys (length n), detection.py:244-250.
__device__ __forceinline__ float cc_entry(const float* xs, const float* ys, int n, int cutoff, int j) {
    const double acc = ofp::cc_dot(xs, n, ys, n, j - (n - 1));
    const int m = j < n ? j : 2 * n - 2 - j;
    const int cnt = m < cutoff ? cutoff : m + 1;
    return __fdiv_rn((float)acc, (float)cnt);
}

// adjust_onset (detection.py:299-352) for one pair, executed by one wave: which of the two onsets moves to
// make their lag `new_lag`, decided by the exponentially weighted signal between the old and the new
// position (weights np.exp(np.linspace(0, -e, |lag_diff|)), sums in fp64 as np.sum of the float64
// products, normalised by the signals' maxima mx / my).  *ca / *cb: what to add to onset 0 / onset 1
// (valid on lane 0).
__device__ __forceinline__ void adjust_onset_wave(const float* xs, const float* ys, int n, int o0, int o1, int new_lag,
                                                  float mx, float my, int lane, int64_t* ca, int64_t* cb) {
    constexpr int XW = XCORR_WAVE;
    const int lag_diff = (o1 - o0) - new_lag;
    const int k = lag_diff < 0 ? -lag_diff : lag_diff;
    int x_start, x_end, y_start, y_end;
    if (lag_diff < 0) {
        x_start = max(o0 + lag_diff, 0);
        x_end = min(o0, n);
        y_start = min(o1, n);
        y_end = min(o1 - lag_diff, n);
    } else {
        x_start = o0;
        x_end = min(o0 + lag_diff, n);
        y_start = max(o1 - lag_diff, 0);
        y_end = min(o1, n);
    }
    x_start = max(0, min(x_start, n));
    y_start = max(0, min(y_start, n));
    // weights np.exp(np.linspace(0, -e, k)): w[m] = exp(m * (-e / (k - 1))), w[k-1] = exp(-e)
    const double step = k > 1 ? -2.718281828459045 / (double)(k - 1) : 0.0;
    const int Lx = x_end - x_start, Ly = y_end - y_start;
    double sa = 0.0, sb = 0.0;
    for (int q = lane; q < Lx; q += XW) {
        int m = k - Lx + q;
        double w = exp(m == k - 1 && k > 1 ? -2.718281828459045 : (double)m * step);
        sa += (double)xs[x_start + q] * w;
    }
    for (int q = lane; q < Ly; q += XW) {
        int m = k - 1 - q;
        double w = exp(m == k - 1 && k > 1 ? -2.718281828459045 : (double)m * step);
        sb += (double)ys[y_start + q] * w;
    }
    for (int o = XW / 2; o > 0; o >>= 1) {
        sa += __shfl_xor(sa, o);
        sb += __shfl_xor(sb, o);
    }
    const double da = Lx > 0 ? sa / (double)mx : 0.0;
    const double db = Ly > 0 ? sb / (double)my : 0.0;
    if (da > db) {
        if (o0 + lag_diff < 0) {
            *ca = 0;
            *cb = -lag_diff;
        } else {
            *ca = lag_diff;
            *cb = 0;
        }
    } else {
        *ca = 0;
        *cb = -lag_diff;
    }
}

}  // namespace ofp
