// The correlation canon shared by ofp_xcorr.hip and ofp_locate2d.hip: entry k of the correlation of a (length la)
// with b (length lb), sum over ascending n of a[n + k] * b[n] (0 <= n < lb, 0 <= n + k < la), accumulated in fp64 by
// ONE thread (fp32 x fp32 products are exact in fp64).  Callers round the sum once to fp32.
#pragma once
#include <hip/hip_runtime.h>

namespace ofp {

__device__ __forceinline__ double cc_dot(const float* a, int la, const float* b, int lb, int k) {
    const int n0 = k < 0 ? -k : 0, n1 = lb < la - k ? lb : la - k;
    double acc = 0.0;
    for (int n = n0; n < n1; ++n) acc += (double)a[n + k] * (double)b[n];
    return acc;
}

}  // namespace ofp
