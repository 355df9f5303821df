// The arithmetic canon of include/ofp_math.h, evaluated on the device one value at a time (ofp_canon_eval).
//
// The detector's kernels call these functions on whatever values audio produces; this entry runs each of them on a
// caller-chosen array of bit patterns, so that a test can compare the device's result with the host's over whole
// binades (tests/test_gpu_canon.py).  The file is built with the library's flags like every other translation unit: what
// it computes is what the same functions compute inside the detector.  Each op calls the header's function and nothing
// else.
//
// The detector's dB and back-to-linear passes evaluate the canon with its tables held in LDS (ofp_canon_dev.h).
// ofp_canon_eval_lds runs exactly that form of RECT_DB and REL_LINEAR, tables filled per workgroup as the passes fill them,
// so that a test can hold it against the header's form over every float32 bit pattern (tests/test_gpu_canon_tables.py).
#include "ofp_common.h"
#include "../../include/ofp_math.h"
#include "ofp_canon_dev.h"

namespace {

using ofp::cdiv;

struct CanonArgs {
    int32_t op;
    float p0, p1, p2;  // op's parameters; MIN_STEP / MAX_STEP: p2 = ofp_ialpha(p0), formed on the host
};

__global__ __launch_bounds__(256) void k_canon_eval(CanonArgs a, const float* __restrict__ x, const float* __restrict__ y,
                                                    int64_t n, float* __restrict__ out) {
    const int64_t step = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += step) {
        const float xi = x[i];
        float r;
        switch (a.op) {
            case OFP_CANON_LOG10: r = ofp_log10f(xi); break;
            case OFP_CANON_EXP10: r = ofp_exp10f(xi); break;
            case OFP_CANON_RECT_DB: r = ofp_rect_db(xi, a.p0); break;
            case OFP_CANON_REL_LINEAR: r = ofp_rel_linear(xi, a.p0); break;
            case OFP_CANON_AR_STEP: r = ofp_ar_step(xi, y[i], a.p0, a.p1); break;
            case OFP_CANON_MIN_STEP: r = ofp_min_step(xi, y[i], a.p2, a.p0, a.p1); break;
            default: r = ofp_max_step(xi, y[i], a.p2, a.p0); break;  // OFP_CANON_MAX_STEP (the host refuses any other)
        }
        out[i] = r;
    }
}

__global__ __launch_bounds__(256) void k_canon_eval_lds(CanonArgs a, const float* __restrict__ x, int64_t n,
                                                        float* __restrict__ out) {
    __shared__ ofp_canon::LogTables lg;
    __shared__ ofp_canon::ExpTable ex;
    ofp_canon::fill(lg);
    ofp_canon::fill(ex);
    const int64_t step = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += step) {
        const float xi = x[i];
        out[i] = a.op == OFP_CANON_RECT_DB ? ofp_canon::rect_db(xi, a.p0, lg.r, lg.t) : ofp_canon::rel_linear(xi, a.p0, ex.t);
    }
}

}  // namespace

extern "C" int ofp_canon_eval(int32_t op, const float* d_x, const float* d_y, int64_t n, float p0, float p1, float p2,
                              float* d_out, void* stream) {
    OFP_REQUIRE(op >= OFP_CANON_LOG10 && op <= OFP_CANON_MAX_STEP, "ofp_canon_eval: unknown op %d", (int)op);
    OFP_REQUIRE(n >= 0, "ofp_canon_eval: negative n");
    if (n == 0) return OFP_OK;
    OFP_REQUIRE(d_x && d_out, "ofp_canon_eval: NULL argument");
    const bool two = op >= OFP_CANON_AR_STEP;
    OFP_REQUIRE(!two || d_y, "ofp_canon_eval: op %d takes a second operand, d_y is NULL", (int)op);
    CanonArgs a{op, p0, p1, p2};
    if (op == OFP_CANON_MIN_STEP || op == OFP_CANON_MAX_STEP) a.p2 = ofp_ialpha(p0);  // as ofp_detector_create forms it
    const unsigned blocks = (unsigned)(cdiv(n, 256) < 8192 ? cdiv(n, 256) : 8192);
    hipLaunchKernelGGL(k_canon_eval, dim3(blocks), dim3(256), 0, (hipStream_t)stream, a, d_x, d_y, n, d_out);
    OFP_LAUNCH_CHECK("k_canon_eval");
    return OFP_OK;
}

extern "C" int ofp_canon_eval_lds(int32_t op, const float* d_x, int64_t n, float floor_db, float* d_out, void* stream) {
    OFP_REQUIRE(op == OFP_CANON_RECT_DB || op == OFP_CANON_REL_LINEAR, "ofp_canon_eval_lds: unknown op %d", (int)op);
    OFP_REQUIRE(n >= 0, "ofp_canon_eval_lds: negative n");
    if (n == 0) return OFP_OK;
    OFP_REQUIRE(d_x && d_out, "ofp_canon_eval_lds: NULL argument");
    CanonArgs a{op, floor_db, 0.0f, 0.0f};
    const unsigned blocks = (unsigned)(cdiv(n, 256) < 8192 ? cdiv(n, 256) : 8192);
    hipLaunchKernelGGL(k_canon_eval_lds, dim3(blocks), dim3(256), 0, (hipStream_t)stream, a, d_x, n, d_out);
    OFP_LAUNCH_CHECK("k_canon_eval_lds");
    return OFP_OK;
}
