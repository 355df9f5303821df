// Training model.CNN on the GPU (the reference's model.py:52-162 and the loop of train.py): full-batch forward in
// training mode, mean L1 / MSE loss, backward, NAdam, and optionally an eval-mode validation pass with Lightning's
// early-stop rule -- one epoch is a linear chain of short kernels on one stream, captured once as a hipGraph and
// replayed.  The epoch index (row of the rate table, slot of the loss curves) is a device counter that the chain's
// last kernel advances, so every replay is the same graph; once the stop word is set every kernel returns at once.
// With random options (ofp_cnn_train_random; csrc/ofp_train_random.h) the same counter drives a counter-based random
// stream: the epoch's windows are cut from resident audio by k_shift_windows, the chain's first kernel (with a stretch
// span, ofp_cnn_train_stretch, by k_stretch_windows, which also resamples them), and the
// features in front of the Linear head go through k_dropout_fwd (their gradient through k_dropout_bwd).
//
// Layer order as the reference builds it: conv + bias -> activation -> BatchNorm1d -> MaxPool1d(2, 2).  Only the
// pre-activation z [B][C][Wc] and the layer's output [B][C][Wo] are kept; the activation, the normalised value and
// the pool's choice are recomputed from z where the backward needs them (ties take the first, an odd last column is
// dropped and gets no gradient).
//
// Reductions.  No atomics anywhere.  Everything summed over the batch (BatchNorm's sums, forward and backward; the
// convolution's weight and bias gradients) goes through one partial-slab reducer: the B * Wc (sample, position)
// pairs of a channel are cut into slabs of kSlab pairs; a workgroup sums one slab in fp64 in an order fixed by the
// thread index, and a second kernel adds the slabs in slab order.  The shape depends on the problem's dimensions
// alone, so results are bitwise reproducible.  The Linear head sums over features (forward, one workgroup per
// sample) and over samples (backward, one thread per feature and chunk of 64 samples, the chunks added in order) in
// fp64 as well.  Convolution forward and input
// gradient are fp32 fmaf chains of at most cin/groups * k (cout/groups * k) terms, in k_conv1d's order.
// What follows a convolution, the NAdam step and the stack's limits are in csrc/ofp_cnn_stack.h, shared with the CNNRNN
// trainer (csrc/ofp_cnnrnn_train.hip).
//
// Host side, by the contract of csrc/ofp_train_chain.h: the Plan is the ConvStack part (its checks, offsets, blocks and
// launch loops are in ofp_cnn_stack.h) and this file's own flat head with its dropout; enqueue_forward / _backward /
// _step / _reset for Run<Plan>; the traits Cnn.  The ofp_cnn_train* and ofp_cnn_loss_grads* entries forward into
// train_workspace_bytes / train_entry / loss_grads_entry<Cnn>.
#include "ofp_cnn_stack.h"

#include <algorithm>
#include <cmath>

namespace {

// the generator alone (ofp_philox4x32): counters [n][4], keys [n][2] -> words [n][4]
__global__ __launch_bounds__(kT) void k_philox(const uint32_t* __restrict__ counters, const uint32_t* __restrict__ keys,
                                               int64_t n, uint32_t* __restrict__ out) {
    for (int64_t i = (int64_t)blockIdx.x * kT + threadIdx.x; i < n; i += (int64_t)gridDim.x * kT) {
        const uint32_t* c = counters + i * 4;
        const Words d = philox4x32_10(c[0], c[1], c[2], c[3], keys[i * 2], keys[i * 2 + 1]);
        for (int u = 0; u < 4; ++u) out[i * 4 + u] = d.w[u];
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------

struct Plan : WsPlan {
    ConvStack cs;
    int loss, O, F;  // F: the features of the flat head, the last layer's channels x columns
    int fcw_off, fcb_off;
    // work space, byte offsets
    int64_t o_out, o_dy, o_lpart, o_part, o_M, o_V, o_HD;  // o_HD: the dropped features
};

int make_plan(const char* who, const ofp_cnn_config* c, int64_t n, int64_t n_val, Plan& p, const Random& rnd) {
    OFP_REQUIRE(c != nullptr, "%s: config is NULL", who);
    OFP_REQUIRE(n_val >= 0 && n_val <= kMaxBatch, "%s: validation batch of %lld (limit: 0..%d)", who, (long long)n_val,
                kMaxBatch);
    p = Plan{};
    const int64_t nmax = n > n_val ? n : n_val;
    int64_t max_part = 0;  // bytes
    if (int rc = plan_conv_stack(who, c, n, nmax, p, p.np, p.ns, max_part, p.cs)) return rc;
    p.loss = c->loss, p.O = c->n_out;
    p.F = p.cs.conv[p.cs.L - 1].cout * p.cs.wo[p.cs.L - 1];
    max_part = std::max<int64_t>(max_part, (int64_t)fc_chunks(n) * p.O * p.F * 8);
    p.fcw_off = p.np, p.np += p.O * p.F;
    p.fcb_off = p.np, p.np += p.O;
    p.o_out = p.take(nmax * p.O * 4);
    p.o_dy = p.take(nmax * p.O * 4);
    p.o_lpart = p.take(nmax * 8);
    p.o_part = p.take(max_part);
    p.o_G = p.take((int64_t)p.np * 4);
    p.o_M = p.take((int64_t)p.np * 4);
    p.o_V = p.take((int64_t)p.np * 4);
    p.o_RS = p.take((int64_t)p.ns * 4);
    p.o_ctl = p.take(sizeof(Ctl));
    if (rnd.drop) p.o_HD = p.take(n * p.F * 4);
    if (rnd.windows) p.o_X = p.take(n * c->channels[0] * c->width * 4);
    return OFP_OK;
}

Fc fc_of(const Run<Plan>& r, const float* h, int64_t n, const float* y) {
    const Plan& p = *r.p;
    return Fc{h, n, p.F, p.O, r.P + p.fcw_off, r.P + p.fcb_off, y};
}

// conv stack and head of a batch, its mean loss into `curve`; train: batch statistics, d loss / d out kept and the
// head's bias gradient; else running statistics, L1 and the early-stop rule
int enqueue_forward(const Run<Plan>& r, const float* x, const float* y, int64_t n, bool train, float* curve,
                    int patience) {
    const Plan& p = *r.p;
    const float* in;
    if (int rc = enqueue_conv_stack_fwd(r, p.cs, x, n, train, r.at<double>(p.o_part), &in)) return rc;
    if (train && r.rnd.drop) {
        float* HD = r.at<float>(p.o_HD);
        if (int rc = enqueue_dropout_fwd(r.ctl, r.rnd, in, HD, n * p.F, r.st)) return rc;
        in = HD;
    }
    return enqueue_fc_forward(r.ctl, fc_of(r, in, n, y), p.loss, r.at<float>(p.o_out),
                              train ? r.at<float>(p.o_dy) : nullptr, r.at<double>(p.o_lpart), curve, patience,
                              r.G + p.fcb_off, r.st);
}

int enqueue_backward(const Run<Plan>& r, const float* x, int64_t n) {
    const Plan& p = *r.p;
    float* GH = r.at<float>(p.cs.o_gh);
    double* part = r.at<double>(p.o_part);
    const float* feat = r.at<float>(r.rnd.drop ? p.o_HD : p.cs.o_H[p.cs.L - 1]);
    if (int rc = enqueue_fc_backward(r.ctl, fc_of(r, feat, n, nullptr), r.at<float>(p.o_dy), part, r.G + p.fcw_off, GH,
                                     r.st))
        return rc;
    if (r.rnd.drop)
        if (int rc = enqueue_dropout_bwd(r.ctl, r.rnd, GH, n * p.F, r.st)) return rc;
    return enqueue_conv_stack_bwd(r, p.cs, x, n, part);
}

int enqueue_step(const Run<Plan>& r, const float* rows) {
    const Plan& p = *r.p;
    hipLaunchKernelGGL(k_nadam, dim3(grid_for(p.np)), dim3(kT), 0, r.st, r.ctl, rows, r.P, r.G, r.at<float>(p.o_M),
                       r.at<float>(p.o_V), (int64_t)p.np);
    OFP_LAUNCH_CHECK("k_nadam");
    return OFP_OK;
}

int enqueue_reset(const Run<Plan>& r) {
    return zero_moments(r.at<float>(r.p->o_M), r.at<float>(r.p->o_V), r.p->np, r.st);
}

struct Cnn {
    using Config = ofp_cnn_config;
    using Plan = ::Plan;
    static constexpr const char* train = "ofp_cnn_train";
    static constexpr const char* grads = "ofp_cnn_loss_grads";
    static constexpr const char* env = "OFP_CNN_GRAPH";
    static Window window_of(const Config& c) { return Window{c.channels[0], c.width}; }
    static constexpr auto make_plan = ::make_plan;
};

}  // namespace

extern "C" {

int32_t ofp_cnn_train_slab(void) { return kSlab; }

int64_t ofp_cnn_train_workspace_bytes(const ofp_cnn_config* cfg, int64_t n, int64_t n_val) {
    return ofp_cnn_train_random_workspace_bytes(cfg, n, n_val, nullptr);
}

int64_t ofp_cnn_train_random_workspace_bytes(const ofp_cnn_config* cfg, int64_t n, int64_t n_val,
                                             const ofp_train_random* random) {
    return ofp_cnn_train_stretch_workspace_bytes(cfg, n, n_val, random, 0);
}

int64_t ofp_cnn_train_stretch_workspace_bytes(const ofp_cnn_config* cfg, int64_t n, int64_t n_val,
                                              const ofp_train_random* random, int32_t stretch_span) {
    return train_workspace_bytes<Cnn>(cfg, n, n_val, random, stretch_span);
}

int ofp_cnn_train(const ofp_cnn_config* cfg, int64_t n, const float* d_x, const float* d_y, int64_t n_val,
                  const float* d_x_val, const float* d_y_val, const float* d_rates, int32_t num_epochs,
                  int32_t min_epochs, int32_t patience, float* d_params, float* d_stats, float* d_train_loss,
                  float* d_val_loss, int32_t* h_epochs, void* d_ws, int64_t ws_bytes, void* stream) {
    return ofp_cnn_train_random(cfg, n, d_x, d_y, n_val, d_x_val, d_y_val, d_rates, num_epochs, min_epochs, patience,
                                d_params, d_stats, d_train_loss, d_val_loss, h_epochs, d_ws, ws_bytes, stream,
                                nullptr);
}

int ofp_cnn_train_random(const ofp_cnn_config* cfg, int64_t n, const float* d_x, const float* d_y, int64_t n_val,
                         const float* d_x_val, const float* d_y_val, const float* d_rates, int32_t num_epochs,
                         int32_t min_epochs, int32_t patience, float* d_params, float* d_stats, float* d_train_loss,
                         float* d_val_loss, int32_t* h_epochs, void* d_ws, int64_t ws_bytes, void* stream,
                         const ofp_train_random* random) {
    return ofp_cnn_train_stretch(cfg, n, d_x, d_y, n_val, d_x_val, d_y_val, d_rates, num_epochs, min_epochs, patience,
                                 d_params, d_stats, d_train_loss, d_val_loss, h_epochs, d_ws, ws_bytes, stream, random,
                                 0);
}

int ofp_cnn_train_stretch(const ofp_cnn_config* cfg, int64_t n, const float* d_x, const float* d_y, int64_t n_val,
                          const float* d_x_val, const float* d_y_val, const float* d_rates, int32_t num_epochs,
                          int32_t min_epochs, int32_t patience, float* d_params, float* d_stats, float* d_train_loss,
                          float* d_val_loss, int32_t* h_epochs, void* d_ws, int64_t ws_bytes, void* stream,
                          const ofp_train_random* random, int32_t stretch_span) {
    return train_entry<Cnn>(cfg, n, d_x, d_y, n_val, d_x_val, d_y_val, d_rates, num_epochs, min_epochs, patience, d_params,
                            d_stats, d_train_loss, d_val_loss, h_epochs, d_ws, ws_bytes, stream, random, stretch_span);
}

int ofp_cnn_loss_grads(const ofp_cnn_config* cfg, int64_t n, const float* d_x, const float* d_y,
                       const float* d_params, float* d_loss, float* d_grads, void* d_ws, int64_t ws_bytes,
                       void* stream) {
    return ofp_cnn_loss_grads_random(cfg, n, d_x, d_y, d_params, d_loss, d_grads, d_ws, ws_bytes, stream, nullptr);
}

int ofp_cnn_loss_grads_random(const ofp_cnn_config* cfg, int64_t n, const float* d_x, const float* d_y,
                              const float* d_params, float* d_loss, float* d_grads, void* d_ws, int64_t ws_bytes,
                              void* stream, const ofp_train_random* random) {
    return loss_grads_entry<Cnn>(cfg, n, d_x, d_y, d_params, d_loss, d_grads, d_ws, ws_bytes, stream, random);
}

int64_t ofp_conv1d_backward_workspace_bytes(int64_t n, int32_t cin, int32_t w, int32_t cout, int32_t k,
                                            int32_t padding, int32_t dilation, int32_t groups) {
    if (check_conv("ofp_conv1d_backward", n, cin, w, cout, k, padding, dilation, groups)) return -1;
    return conv_bwd_bytes(n, cin, w, cout, k, padding, dilation, groups, 1);
}

int ofp_conv1d_backward(const float* d_x, int64_t n, int32_t cin, int32_t w, const float* d_w, int32_t cout,
                        int32_t k, int32_t padding, int32_t dilation, int32_t groups, const float* d_dz, float* d_dx,
                        float* d_dw, float* d_db, void* d_ws, int64_t ws_bytes, void* stream) {
    return conv_bwd_alone("ofp_conv1d_backward",
                          ofp_conv1d_backward_workspace_bytes(n, cin, w, cout, k, padding, dilation, groups), d_x, n,
                          cin, w, d_w, cout, k, padding, dilation, groups, 1, d_dz, d_dx, d_dw, d_db, d_ws, ws_bytes,
                          stream);
}

// work space of the head alone: the samples' loss shares, then the chunks of the weight gradient
int64_t ofp_linear_head_train_workspace_bytes(int64_t n, int32_t F, int32_t O) {
    if (n < 1 || n > kMaxBatch || O < 1 || O > kMaxOut || F < 1) return -1;
    return ofp::align_up(n * 8, 256) + (int64_t)fc_chunks(n) * O * F * 8;
}

int ofp_linear_head_train(const float* d_h, int64_t n, int32_t F, const float* d_w, int32_t O, const float* d_b,
                          const float* d_y, int32_t loss, float* d_out, float* d_dy, float* d_loss, float* d_dw,
                          float* d_db, float* d_dh, void* d_ws, int64_t ws_bytes, void* stream) {
    const int64_t need = ofp_linear_head_train_workspace_bytes(n, F, O);
    OFP_REQUIRE(need >= 0, "ofp_linear_head_train: n %lld, %d features, %d outputs (limits: 1..%d, >= 1, 1..%d)",
                (long long)n, F, O, kMaxBatch, kMaxOut);
    OFP_REQUIRE(loss == 0 || loss == 1, "ofp_linear_head_train: loss %d (0 = L1, 1 = MSE)", loss);
    OFP_REQUIRE(d_h && d_w && d_b && d_y && d_out && d_dy && d_loss && d_dw && d_db && d_dh,
                "ofp_linear_head_train: NULL argument");
    if (int rc = check_ws("ofp_linear_head_train", d_ws, ws_bytes, need)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const Fc f{d_h, n, F, O, d_w, d_b, d_y};
    double* lpart = (double*)d_ws;
    double* part = reinterpret_cast<double*>((char*)d_ws + ofp::align_up(n * 8, 256));
    if (int rc = enqueue_fc_forward(nullptr, f, loss, d_out, d_dy, lpart, d_loss, -1, d_db, st)) return rc;
    return enqueue_fc_backward(nullptr, f, d_dy, part, d_dw, d_dh, st);
}

int64_t ofp_batchnorm_train_workspace_bytes(int64_t n, int32_t C, int32_t w) {
    if (n < 1 || n > kMaxBatch || C < 1 || C > kMaxCh || w < 1 || w > 2 * kMaxWidth) return -1;
    return (int64_t)C * slabs_of(n * w) * 2 * 8 + (int64_t)C * 2 * 4;
}

namespace {
int check_bn(const char* who, int64_t n, int32_t C, int32_t w, void* d_ws, int64_t ws_bytes) {
    const int64_t need = ofp_batchnorm_train_workspace_bytes(n, C, w);
    OFP_REQUIRE(need >= 0, "%s: n %lld, %d channels, width %d (limits: 1..%d, 1..%d, 1..%d)", who, (long long)n, C, w,
                kMaxBatch, kMaxCh, 2 * kMaxWidth);
    OFP_REQUIRE(n * w >= 2, "%s: BatchNorm needs more than 1 value per channel", who);
    return check_ws(who, d_ws, ws_bytes, need);
}
}  // namespace

int ofp_batchnorm_train_forward(const float* d_x, int64_t n, int32_t C, int32_t w, const float* d_gamma,
                                const float* d_beta, double eps, float momentum, float* d_running_mean,
                                float* d_running_var, float* d_y, float* d_mean, float* d_rstd, void* d_ws,
                                int64_t ws_bytes, void* stream) {
    if (int rc = check_bn("ofp_batchnorm_train_forward", n, C, w, d_ws, ws_bytes)) return rc;
    OFP_REQUIRE(d_x && d_gamma && d_beta && d_running_mean && d_running_var && d_y && d_mean && d_rstd,
                "ofp_batchnorm_train_forward: NULL argument");
    OFP_REQUIRE(momentum > 0.0f && momentum <= 1.0f && eps > 0.0, "ofp_batchnorm_train_forward: momentum %g, eps %g",
                (double)momentum, eps);
    hipStream_t st = (hipStream_t)stream;
    if (int rc = enqueue_bn_stats(nullptr, d_x, n, C, w, OFP_ACT_IDENTITY, eps, momentum, (double*)d_ws, d_mean,
                                  d_rstd, d_running_mean, d_running_var, st))
        return rc;
    Post t{};
    t.C = C, t.wc = w, t.wo = w, t.act = OFP_ACT_IDENTITY, t.pool = 0, t.mode = 1, t.eps = eps;
    t.ga = d_gamma, t.be = d_beta, t.mean = d_mean, t.rs = d_rstd;
    hipLaunchKernelGGL(k_post, dim3(grid_for(n * C * w)), dim3(kT), 0, st, (const Ctl*)nullptr, t, n, d_x, d_y);
    OFP_LAUNCH_CHECK("k_post");
    return OFP_OK;
}

int ofp_batchnorm_train_backward(const float* d_x, int64_t n, int32_t C, int32_t w, const float* d_gamma,
                                 const float* d_mean, const float* d_rstd, const float* d_dy, float* d_dx,
                                 float* d_dgamma, float* d_dbeta, void* d_ws, int64_t ws_bytes, void* stream) {
    if (int rc = check_bn("ofp_batchnorm_train_backward", n, C, w, d_ws, ws_bytes)) return rc;
    OFP_REQUIRE(d_x && d_gamma && d_mean && d_rstd && d_dy && d_dx && d_dgamma && d_dbeta,
                "ofp_batchnorm_train_backward: NULL argument");
    Post t{};
    t.C = C, t.wc = w, t.wo = w, t.act = OFP_ACT_IDENTITY, t.pool = 0, t.mode = 1;
    t.ga = d_gamma, t.be = d_gamma /* not read by the backward */, t.mean = d_mean, t.rs = d_rstd;
    float* s12 = reinterpret_cast<float*>((char*)d_ws + (int64_t)C * slabs_of(n * w) * 2 * 8);
    return enqueue_post_bwd(nullptr, t, n, d_x, d_dy, (double*)d_ws, s12, d_dgamma, d_dbeta, d_dx,
                            (hipStream_t)stream);
}

int ofp_nadam_step(float* d_p, const float* d_g, float* d_m, float* d_v, int64_t n, const float* d_row, void* stream) {
    OFP_REQUIRE(d_p && d_g && d_m && d_v && d_row && n >= 1, "ofp_nadam_step: NULL argument or n < 1");
    hipLaunchKernelGGL(k_nadam, dim3(grid_for(n)), dim3(kT), 0, (hipStream_t)stream, (const Ctl*)nullptr, d_row, d_p,
                       d_g, d_m, d_v, n);
    OFP_LAUNCH_CHECK("k_nadam");
    return OFP_OK;
}

// ---- the random stream alone (csrc/ofp_train_random.h), by the kernels the two epoch graphs run -------------------------

int ofp_philox4x32(const uint32_t* d_counters, const uint32_t* d_keys, int64_t n, uint32_t* d_out, void* stream) {
    OFP_REQUIRE(d_counters && d_keys && d_out && n >= 1, "ofp_philox4x32: NULL argument or n < 1");
    hipLaunchKernelGGL(k_philox, dim3(grid_for(n)), dim3(kT), 0, (hipStream_t)stream, d_counters, d_keys, n, d_out);
    OFP_LAUNCH_CHECK("k_philox");
    return OFP_OK;
}

int ofp_dropout_mask(uint64_t seed, int32_t epoch, int64_t n, int32_t F, double p, float* d_mask, void* stream) {
    OFP_REQUIRE(d_mask && n >= 1 && F >= 1 && n * F <= ((int64_t)1 << 32),
                "ofp_dropout_mask: NULL mask, or n %lld x F %d outside 1..2^32 elements", (long long)n, F);
    ofp_train_random o{};
    o.seed = seed, o.epoch = epoch, o.dropout_p = p;
    Random r;
    if (int rc = make_random("ofp_dropout_mask", &o, 0, n, 0, 0, false, r)) return rc;
    return enqueue_dropout_fwd(nullptr, r, nullptr, d_mask, n * F, (hipStream_t)stream);
}

int ofp_shift_windows(uint64_t seed, int32_t epoch, const float* d_audio, int64_t audio_len, int32_t channels,
                      const int64_t* d_starts, int64_t n_onsets, int32_t n_extractions, int32_t max_shift,
                      int32_t width, int32_t* d_shifts, float* d_windows, void* stream) {
    OFP_REQUIRE(d_windows && channels >= 1 && width >= 1 && n_extractions >= 1 && n_onsets >= 1 &&
                    n_onsets * n_extractions <= (1 << 20),
                "ofp_shift_windows: NULL windows, or %d channels, width %d, %lld onsets x %d extractions", channels,
                width, (long long)n_onsets, n_extractions);
    ofp_train_random o{};
    o.seed = seed, o.epoch = epoch, o.max_shift = max_shift, o.n_extractions = n_extractions;
    o.audio_channels = channels, o.d_audio = d_audio, o.audio_len = audio_len, o.d_starts = d_starts;
    o.n_onsets = n_onsets;
    Random r;
    if (int rc = make_random("ofp_shift_windows", &o, 0, n_onsets * n_extractions, channels, width, true, r)) return rc;
    return enqueue_shift_windows(nullptr, r, d_windows, d_shifts, (hipStream_t)stream);
}

int ofp_stretch_windows(uint64_t seed, int32_t epoch, const float* d_audio, int64_t audio_len, int32_t channels,
                        const int64_t* d_starts, int64_t n_onsets, int32_t n_extractions, int32_t max_shift,
                        int32_t stretch_span, int32_t width, int32_t* d_shifts, int32_t* d_stretches,
                        float* d_windows, void* stream) {
    OFP_REQUIRE(d_windows && channels >= 1 && width >= 1 && n_extractions >= 1 && n_onsets >= 1 &&
                    n_onsets * n_extractions <= (1 << 20),
                "ofp_stretch_windows: NULL windows, or %d channels, width %d, %lld onsets x %d extractions", channels,
                width, (long long)n_onsets, n_extractions);
    OFP_REQUIRE(stretch_span >= 2, "ofp_stretch_windows: stretch span %d (from 2; 1 leaves nothing to draw, the "
                "reference's randint(1, 1) raises; without a stretch the call is ofp_shift_windows)", stretch_span);
    ofp_train_random o{};
    o.seed = seed, o.epoch = epoch, o.max_shift = max_shift, o.n_extractions = n_extractions;
    o.audio_channels = channels, o.d_audio = d_audio, o.audio_len = audio_len, o.d_starts = d_starts;
    o.n_onsets = n_onsets;
    Random r;
    if (int rc = make_random("ofp_stretch_windows", &o, stretch_span, n_onsets * n_extractions, channels, width, true, r))
        return rc;
    return enqueue_stretch_windows(nullptr, r, d_windows, d_shifts, d_stretches, (hipStream_t)stream);
}

}  // extern "C"
