// The dB and back-to-linear canon of include/ofp_math.h with its three tables taken from the caller.
//
// ofp_log10f and ofp_exp10f index OFP_LOG_R / OFP_LOG_T / OFP_EXP2_T with a value that depends on every sample's mantissa.
// From the `__device__ const` arrays that is a per-lane gather through the vector-memory path, and the wait for its result
// (vmcnt) also waits for every streaming load and store the lane has issued before it: one memory drain per sample.  The
// functions here are those of the header operation for operation -- the same fp64 sequence in the same order, the same
// special cases, no FMA contraction, the `dif / 20.0f` division as it is -- and differ only in where the table values come
// from: pointers the caller supplies.  The detector's elementwise kernels pass copies in LDS (LogTables / ExpTable, filled
// once per workgroup by fill()), which are read with ds_read_b64 and waited for on lgkmcnt alone.
//
// include/ofp_math.h stays the spec: tests/test_gpu_canon_tables.py compares the two forms on the device over all 2^32
// float32 bit patterns (ofp_canon_eval_lds runs these functions, ofp_canon_eval the header's).
#ifndef OFP_CANON_DEV_H
#define OFP_CANON_DEV_H

#include "../../include/ofp_math.h"

#pragma clang fp contract(off)

namespace ofp_canon {

// log10 of a non-negative fp32 value: ofp_log10f with OFP_LOG_R -> log_r and OFP_LOG_T -> log_t
OFP_D float log10f_from(float a, const double* log_r, const double* log_t) {
    if (a != a) return a;
    if (a == 0.0f) return ofp_u2f(0xff800000u); /* -inf */
    if (a < 0.0f) return ofp_u2f(0x7fc00000u);  /* nan  */
    if (ofp_f2u(a) == 0x7f800000u) return a;    /* +inf */
    uint64_t u = ofp_d2u((double)a);
    int k = (int)((u >> 52) & 0x7ff) - 1023;
    uint64_t mant = u & 0x000fffffffffffffull;
    int i = (int)(mant >> 45);
    uint64_t ebits = 0x3ff0000000000000ull;
    if (i >= 53) {
        ebits = 0x3fe0000000000000ull;
        k += 1;
    }
    double m = ofp_u2d(ebits | mant);
    double z = m * log_r[i] - 1.0;
    double p = -0.1;
    p = p * z + (1.0 / 9.0);
    p = p * z - 0.125;
    p = p * z + (1.0 / 7.0);
    p = p * z - (1.0 / 6.0);
    p = p * z + 0.2;
    p = p * z - 0.25;
    p = p * z + (1.0 / 3.0);
    p = p * z - 0.5;
    p = p * z + 1.0;
    p = p * z;
    double r = (double)k * OFP_LOG10_2 + log_t[i];
    r = r + p * OFP_LOG10_E;
    return (float)r;
}

// 10**v: ofp_exp10f with OFP_EXP2_T -> exp2_t
OFP_D float exp10f_from(float v, const double* exp2_t) {
    if (v != v) return v;
    if (v >= 39.0f) return ofp_u2f(0x7f800000u);
    if (v <= -46.0f) return 0.0f;
    double t = (double)v * OFP_LOG2_10;
    double tn = t * 32.0;
    int n = (int)(tn + (tn >= 0.0 ? 0.5 : -0.5));
    double f = t - (double)n * 0.03125;
    double y = f * OFP_LN2;
    double p = 1.0 / 5040.0;
    p = p * y + (1.0 / 720.0);
    p = p * y + (1.0 / 120.0);
    p = p * y + (1.0 / 24.0);
    p = p * y + (1.0 / 6.0);
    p = p * y + 0.5;
    p = p * y + 1.0;
    p = p * y + 1.0;
    int e = n >> 5;
    double s = ofp_u2d((uint64_t)(1023 + e) << 52);
    double r = exp2_t[n & 31] * p;
    r = r * s;
    return (float)r;
}

// ofp_rect_db
OFP_D float rect_db(float x, float floor_db, const double* log_r, const double* log_t) {
    float a = x + 1e-10f;
    a = a < 0.0f ? -a : a;
    float v = 20.0f * log10f_from(a, log_r, log_t);
    return v < floor_db ? floor_db : v;
}

// ofp_rel_linear
OFP_D float rel_linear(float dif, float floor_db, const double* exp2_t) {
    float v = exp10f_from(dif / 20.0f, exp2_t) - 1e-10f;
    float hi = -floor_db;
    v = v < 0.0f ? 0.0f : v;
    v = v > hi ? hi : v;
    return v;
}

// The tables as a workgroup holds them: 2 KiB and 256 B of LDS.
struct LogTables {
    double r[128], t[128];
};
struct ExpTable {
    double t[32];
};

// Every thread of the workgroup calls fill() before any of them leaves the kernel: it ends in a barrier.  Workgroups of
// at least 128 threads in x (the kernels that use it have 256): one entry per thread, no loop.
OFP_D void fill(LogTables& s) {
    const int i = threadIdx.x;
    if (i < 128) {
        s.r[i] = OFP_LOG_R[i];
        s.t[i] = OFP_LOG_T[i];
    }
    __syncthreads();
}
OFP_D void fill(ExpTable& s) {
    const int i = threadIdx.x;
    if (i < 32) s.t[i] = OFP_EXP2_T[i];
    __syncthreads();
}

}  // namespace ofp_canon

#endif /* OFP_CANON_DEV_H */
