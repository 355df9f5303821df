// Training model.CNNRNN on the GPU (the reference's model.py:310-440): the conv stack of model.CNN (csrc/ofp_cnn_stack.h),
// the model's dropout on the conv features (site 0 of the random stream), a one-layer GRU whose time axis is the last
// conv layer's channels and whose features are its columns, 2-head self-attention with dropout on the softmax
// probabilities (site 3), the mean over time, out_proj and the Linear head with its loss; backward through all of it,
// one NAdam step, and optionally an eval-mode validation pass with the early-stop rule.  One epoch is a linear chain of
// kernels on one stream, captured once and replayed by run_epochs (csrc/ofp_train_chain.h), as for the other trainers.
//
// The dense layer, GRU and attention kernels, their launch helpers and how they sum are in csrc/ofp_seq_train.h, which
// the RNN trainer (csrc/ofp_rnn_train.hip) shares; here the attention runs its 128-step instantiation.
//
// Host side, by the contract of csrc/ofp_train_chain.h: the Plan is the ConvStack part (ofp_cnn_stack.h), the AttnHead
// part (ofp_seq_train.h; it reads hseq and hands dhseq back) and, between them, this file's own dropout and GRU;
// enqueue_forward / _backward / _step / _reset for Run<Plan>; the traits Cnnrnn.  The ofp_cnnrnn_train_stretch* and
// ofp_cnnrnn_loss_grads_random entries forward into train_workspace_bytes / train_entry / loss_grads_entry<Cnnrnn>.
#include "ofp_seq_train.h"

namespace {

constexpr int kMaxSteps = kAttnCapShort;  // GRU / attention time steps (the last conv layer's channels)
constexpr int kMaxFeat = 2 * kMaxWidth;   // GRU input features (the last conv layer's columns)

int check_gru(const char* who, int64_t n, int T, int F, int H) {
    return check_gru(who, n, T, F, H, kMaxSteps, kMaxFeat);
}

struct Plan : WsPlan {
    ConvStack cs;
    AttnHead head;
    int T, F, H;  // GRU steps (last conv channels), features (last conv columns), hidden size = attention width
    int wih_off, whh_off, bih_off, bhh_off;
    // work space, byte offsets
    int64_t o_HD, o_wiht, o_whht, o_gx, o_gates, o_hseq, o_dhseq, o_dgx, o_dgh, o_hprev, o_part, o_M, o_V;
};

int make_plan(const char* who, const ofp_cnnrnn_config* cc, int64_t n, int64_t n_val, Plan& p, const Random& rnd) {
    OFP_REQUIRE(cc != nullptr, "%s: config is NULL", who);
    const ofp_cnn_config* c = &cc->cnn;
    OFP_REQUIRE(n_val >= 0 && n_val <= kMaxBatch, "%s: validation batch of %lld (limit: 0..%d)", who, (long long)n_val,
                kMaxBatch);
    p = Plan{};
    const int64_t nmax = n > n_val ? n : n_val;
    int64_t max_part = 0;  // bytes
    if (int rc = plan_conv_stack(who, c, n, nmax, p, p.np, p.ns, max_part, p.cs)) return rc;
    const int T = p.T = p.cs.conv[p.cs.L - 1].cout, F = p.F = p.cs.wo[p.cs.L - 1], H = p.H = cc->hidden;
    if (int rc = check_gru(who, n, T, F, H)) return rc;
    p.wih_off = p.np, p.np += 3 * H * F;
    p.whh_off = p.np, p.np += 3 * H * H;
    p.bih_off = p.np, p.np += 3 * H;
    p.bhh_off = p.np, p.np += 3 * H;
    p.o_wiht = p.take((int64_t)3 * H * F * 4);
    p.o_whht = p.take((int64_t)3 * H * H * 4);
    if (int rc = plan_attn_head(who, n, T, H, cc->heads, c->n_out, c->loss, kMaxSteps, p, p.np, max_part, p.head))
        return rc;
    max_part = std::max<int64_t>(max_part, lin_part_bytes(n * T, F, 3 * H));
    const int64_t rows = nmax * T;
    p.o_gx = p.take(rows * 3 * H * 4);
    p.o_gates = p.take(rows * 4 * H * 4);
    p.o_hseq = p.take(rows * H * 4);
    take_attn_head_blocks(p, n, nmax, p.head);
    p.o_dhseq = p.take(n * T * H * 4);
    p.o_dgx = p.take(n * T * 3 * H * 4);
    p.o_dgh = p.take(n * T * 3 * H * 4);
    p.o_hprev = p.take(n * T * H * 4);
    p.o_part = p.take(max_part);
    p.o_G = p.take((int64_t)p.np * 4);
    p.o_M = p.take((int64_t)p.np * 4);
    p.o_V = p.take((int64_t)p.np * 4);
    p.o_RS = p.take((int64_t)p.ns * 4);
    p.o_ctl = p.take(sizeof(Ctl));
    if (rnd.drop) p.o_HD = p.take(n * T * F * 4);
    if (rnd.windows) p.o_X = p.take(n * c->channels[0] * c->width * 4);
    return OFP_OK;
}

// the whole network on a batch, its mean loss into `curve`; train: batch statistics, both dropouts, d loss / d out
// kept and the head's bias gradient; else running statistics, no dropout, L1 and the early-stop rule
int enqueue_forward(const Run<Plan>& r, const float* x, const float* y, int64_t n, bool train, float* curve,
                    int patience) {
    const Plan& p = *r.p;
    const int T = p.T, F = p.F, H = p.H;
    const float* in;
    if (int rc = enqueue_conv_stack_fwd(r, p.cs, x, n, train, r.at<double>(p.o_part), &in)) return rc;
    if (train && r.rnd.drop) {
        float* HD = r.at<float>(p.o_HD);
        if (int rc = enqueue_dropout_fwd(r.ctl, r.rnd, in, HD, n * T * F, r.st)) return rc;
        in = HD;
    }
    float* wiht = r.at<float>(p.o_wiht);
    float* whht = r.at<float>(p.o_whht);
    float* gx = r.at<float>(p.o_gx);
    float* hseq = r.at<float>(p.o_hseq);
    if (int rc = enqueue_transpose(r.ctl, r.P + p.wih_off, 3 * H, F, wiht, r.st)) return rc;
    if (int rc = enqueue_transpose(r.ctl, r.P + p.whh_off, 3 * H, H, whht, r.st)) return rc;
    if (int rc = enqueue_lin_fwd(r.ctl, in, n * T, F, 3 * H, wiht, r.P + p.bih_off, gx, r.st)) return rc;
    if (int rc = enqueue_gru_fwd(r.ctl, gx, whht, r.P + p.bhh_off, n, T, H, hseq, r.at<float>(p.o_gates), r.st))
        return rc;
    return enqueue_attn_head_fwd(r, p.head, kMaxSteps, hseq, n, y, train, curve, patience);
}

int enqueue_backward(const Run<Plan>& r, const float* x, int64_t n) {
    const Plan& p = *r.p;
    const int T = p.T, F = p.F, H = p.H;
    float* GH = r.at<float>(p.cs.o_gh);
    double* part = r.at<double>(p.o_part);
    float* dhseq = r.at<float>(p.o_dhseq);
    float* dgx = r.at<float>(p.o_dgx);
    float* dgh = r.at<float>(p.o_dgh);
    float* hprev = r.at<float>(p.o_hprev);
    const float* hseq = r.at<float>(p.o_hseq);
    // the features the GRU read: the last conv layer's output, dropped when the run has dropout
    const float* feat = r.at<float>(r.rnd.drop ? p.o_HD : p.cs.o_H[p.cs.L - 1]);
    if (int rc = enqueue_attn_head_bwd(r, p.head, kMaxSteps, hseq, n, part, dhseq)) return rc;
    if (int rc = enqueue_gru_bwd(r.ctl, r.P + p.whh_off, hseq, r.at<float>(p.o_gates), dhseq, n, T, H, dgx, dgh, hprev,
                                 r.st))
        return rc;
    if (int rc = enqueue_lin_bwd(r.ctl, hprev, n * T, H, 3 * H, r.P + p.whh_off, dgh, part, nullptr, r.G + p.whh_off,
                                 r.G + p.bhh_off, r.st))
        return rc;
    if (int rc = enqueue_lin_bwd(r.ctl, feat, n * T, F, 3 * H, r.P + p.wih_off, dgx, part, GH, r.G + p.wih_off,
                                 r.G + p.bih_off, r.st))
        return rc;
    if (r.rnd.drop)
        if (int rc = enqueue_dropout_bwd(r.ctl, r.rnd, GH, n * T * F, r.st)) return rc;
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

struct Cnnrnn {
    using Config = ofp_cnnrnn_config;
    using Plan = ::Plan;
    static constexpr const char* train = "ofp_cnnrnn_train";
    static constexpr const char* grads = "ofp_cnnrnn_loss_grads";
    static constexpr const char* env = "OFP_CNNRNN_GRAPH";
    static Window window_of(const Config& c) { return Window{c.cnn.channels[0], c.cnn.width}; }
    static constexpr auto make_plan = ::make_plan;
};

}  // namespace

extern "C" {

int32_t ofp_linear_backward_slab(void) { return kLinSlab; }

int64_t ofp_cnnrnn_train_stretch_workspace_bytes(const ofp_cnnrnn_config* cfg, int64_t n, int64_t n_val,
                                                 const ofp_train_random* random, int32_t stretch_span) {
    return train_workspace_bytes<Cnnrnn>(cfg, n, n_val, random, stretch_span);
}

int ofp_cnnrnn_train_stretch(const ofp_cnnrnn_config* cfg, int64_t n, const float* d_x, const float* d_y,
                             int64_t n_val, const float* d_x_val, const float* d_y_val, const float* d_rates,
                             int32_t num_epochs, int32_t min_epochs, int32_t patience, float* d_params, float* d_stats,
                             float* d_train_loss, float* d_val_loss, int32_t* h_epochs, void* d_ws, int64_t ws_bytes,
                             void* stream, const ofp_train_random* random, int32_t stretch_span) {
    return train_entry<Cnnrnn>(cfg, n, d_x, d_y, n_val, d_x_val, d_y_val, d_rates, num_epochs, min_epochs, patience,
                               d_params, d_stats, d_train_loss, d_val_loss, h_epochs, d_ws, ws_bytes, stream, random,
                               stretch_span);
}

int64_t ofp_cnnrnn_loss_grads_random_workspace_bytes(const ofp_cnnrnn_config* cfg, int64_t n, int64_t n_val,
                                                     const ofp_train_random* random) {
    return ofp_cnnrnn_train_stretch_workspace_bytes(cfg, n, n_val, random, 0);
}

int ofp_cnnrnn_loss_grads_random(const ofp_cnnrnn_config* cfg, int64_t n, const float* d_x, const float* d_y,
                                 const float* d_params, float* d_loss, float* d_grads, void* d_ws, int64_t ws_bytes,
                                 void* stream, const ofp_train_random* random) {
    return loss_grads_entry<Cnnrnn>(cfg, n, d_x, d_y, d_params, d_loss, d_grads, d_ws, ws_bytes, stream, random);
}

int64_t ofp_linear_backward_workspace_bytes(int64_t rows, int32_t n_in, int32_t n_out) {
    if (rows < 1 || rows > kMaxRows || n_in < 1 || n_in > 4096 || n_out < 1 || n_out > 4096) return -1;
    return lin_part_bytes(rows, n_in, n_out);
}

int ofp_linear_backward(const float* d_x, int64_t rows, int32_t n_in, const float* d_w, int32_t n_out,
                        const float* d_dy, float* d_dx, float* d_dw, float* d_db, void* d_ws, int64_t ws_bytes,
                        void* stream) {
    const int64_t need = ofp_linear_backward_workspace_bytes(rows, n_in, n_out);
    OFP_REQUIRE(need >= 0, "ofp_linear_backward: %lld rows, %d inputs, %d outputs (limits: 1..%lld, 1..4096, 1..4096)",
                (long long)rows, n_in, n_out, (long long)kMaxRows);
    OFP_REQUIRE(d_x && d_w && d_dy && d_dw && d_db, "ofp_linear_backward: NULL argument");
    if (int rc = check_ws("ofp_linear_backward", d_ws, ws_bytes, need)) return rc;
    return enqueue_lin_bwd(nullptr, d_x, rows, n_in, n_out, d_w, d_dy, (double*)d_ws, d_dx, d_dw, d_db,
                           (hipStream_t)stream);
}

// work space of the GRU forward alone: W_ih^T, W_hh^T, the input projection
int64_t ofp_gru_train_forward_workspace_bytes(int64_t n, int32_t T, int32_t F, int32_t H) {
    if (check_gru("ofp_gru_train_forward", n, T, F, H)) return -1;
    return ofp::align_up((int64_t)3 * H * F * 4, 256) + ofp::align_up((int64_t)3 * H * H * 4, 256) + n * T * 3 * H * 4;
}

int ofp_gru_train_forward(const float* d_x, int64_t n, int32_t T, int32_t F, int32_t H, const float* d_w_ih,
                          const float* d_w_hh, const float* d_b_ih, const float* d_b_hh, float* d_out, float* d_gates,
                          void* d_ws, int64_t ws_bytes, void* stream) {
    if (int rc = check_gru("ofp_gru_train_forward", n, T, F, H)) return rc;
    OFP_REQUIRE(d_x && d_w_ih && d_w_hh && d_b_ih && d_b_hh && d_out && d_gates, "ofp_gru_train_forward: NULL argument");
    if (int rc = check_ws("ofp_gru_train_forward", d_ws, ws_bytes, ofp_gru_train_forward_workspace_bytes(n, T, F, H)))
        return rc;
    hipStream_t st = (hipStream_t)stream;
    float* wiht = (float*)d_ws;
    float* whht = reinterpret_cast<float*>((char*)d_ws + ofp::align_up((int64_t)3 * H * F * 4, 256));
    float* gx = reinterpret_cast<float*>((char*)whht + ofp::align_up((int64_t)3 * H * H * 4, 256));
    if (int rc = enqueue_transpose(nullptr, d_w_ih, 3 * H, F, wiht, st)) return rc;
    if (int rc = enqueue_transpose(nullptr, d_w_hh, 3 * H, H, whht, st)) return rc;
    if (int rc = enqueue_lin_fwd(nullptr, d_x, n * T, F, 3 * H, wiht, d_b_ih, gx, st)) return rc;
    return enqueue_gru_fwd(nullptr, gx, whht, d_b_hh, n, T, H, d_out, d_gates, st);
}

// work space of the GRU backward alone: dgx, dgh, the previous states, the weight gradients' slabs
int64_t ofp_gru_train_backward_workspace_bytes(int64_t n, int32_t T, int32_t F, int32_t H) {
    if (check_gru("ofp_gru_train_backward", n, T, F, H)) return -1;
    return 2 * ofp::align_up(n * T * 3 * H * 4, 256) + ofp::align_up(n * T * H * 4, 256) +
           lin_part_bytes(n * T, F > H ? F : H, 3 * H);
}

int ofp_gru_train_backward(const float* d_x, int64_t n, int32_t T, int32_t F, int32_t H, const float* d_w_ih,
                           const float* d_w_hh, const float* d_out, const float* d_gates, const float* d_dout,
                           float* d_dx, float* d_dw_ih, float* d_dw_hh, float* d_db_ih, float* d_db_hh, void* d_ws,
                           int64_t ws_bytes, void* stream) {
    if (int rc = check_gru("ofp_gru_train_backward", n, T, F, H)) return rc;
    OFP_REQUIRE(d_x && d_w_ih && d_w_hh && d_out && d_gates && d_dout && d_dx && d_dw_ih && d_dw_hh && d_db_ih &&
                    d_db_hh,
                "ofp_gru_train_backward: NULL argument");
    if (int rc = check_ws("ofp_gru_train_backward", d_ws, ws_bytes, ofp_gru_train_backward_workspace_bytes(n, T, F, H)))
        return rc;
    hipStream_t st = (hipStream_t)stream;
    const int64_t g3 = ofp::align_up(n * T * 3 * H * 4, 256);
    float* dgx = (float*)d_ws;
    float* dgh = reinterpret_cast<float*>((char*)d_ws + g3);
    float* hprev = reinterpret_cast<float*>((char*)d_ws + 2 * g3);
    double* part = reinterpret_cast<double*>((char*)hprev + ofp::align_up(n * T * H * 4, 256));
    if (int rc = enqueue_gru_bwd(nullptr, d_w_hh, d_out, d_gates, d_dout, n, T, H, dgx, dgh, hprev, st)) return rc;
    if (int rc = enqueue_lin_bwd(nullptr, hprev, n * T, H, 3 * H, d_w_hh, dgh, part, nullptr, d_dw_hh, d_db_hh, st))
        return rc;
    return enqueue_lin_bwd(nullptr, d_x, n * T, F, 3 * H, d_w_ih, dgx, part, d_dx, d_dw_ih, d_db_ih, st);
}

int64_t ofp_attention_mean_train_forward_workspace_bytes(int64_t n, int32_t T, int32_t E, int32_t heads) {
    return attn_fwd_alone_bytes("ofp_attention_mean_train_forward", n, T, E, heads, kMaxSteps);
}

int ofp_attention_mean_train_forward(const float* d_h, int64_t n, int32_t T, int32_t E, int32_t heads,
                                     const float* d_in_w, const float* d_in_b, const ofp_train_random* random,
                                     float* d_qkv, float* d_probs, float* d_ctx, void* d_ws, int64_t ws_bytes,
                                     void* stream) {
    return attn_fwd_alone("ofp_attention_mean_train_forward", kMaxSteps, d_h, n, T, E, heads, d_in_w, d_in_b, random,
                          d_qkv, d_probs, d_ctx, d_ws, ws_bytes, stream);
}

int64_t ofp_attention_mean_train_backward_workspace_bytes(int64_t n, int32_t T, int32_t E, int32_t heads) {
    return attn_bwd_alone_bytes("ofp_attention_mean_train_backward", n, T, E, heads, kMaxSteps);
}

int ofp_attention_mean_train_backward(const float* d_h, int64_t n, int32_t T, int32_t E, int32_t heads,
                                      const float* d_in_w, const float* d_qkv, const float* d_probs,
                                      const float* d_dctx, const ofp_train_random* random, float* d_dh, float* d_dw,
                                      float* d_db, void* d_ws, int64_t ws_bytes, void* stream) {
    return attn_bwd_alone("ofp_attention_mean_train_backward", kMaxSteps, d_h, n, T, E, heads, d_in_w, d_qkv, d_probs,
                          d_dctx, random, d_dh, d_dw, d_db, d_ws, ws_bytes, stream);
}

int ofp_attention_dropout_mask(uint64_t seed, int32_t epoch, int64_t n, int32_t heads, int32_t T, double p,
                               float* d_mask, void* stream) {
    OFP_REQUIRE(d_mask && n >= 1 && heads >= 1 && T >= 1 && n * heads * T * T <= ((int64_t)1 << 32),
                "ofp_attention_dropout_mask: NULL mask, or n %lld x %d heads x T %d outside 1..2^32 elements",
                (long long)n, heads, T);
    ofp_train_random o{};
    o.seed = seed, o.epoch = epoch, o.dropout_p = p;
    Random r;
    if (int rc = make_random("ofp_attention_dropout_mask", &o, 0, n, 0, 0, false, r)) return rc;
    const int64_t total = n * heads * T * T;
    hipLaunchKernelGGL(k_site_mask, dim3(grid_for(total)), dim3(kT), 0, (hipStream_t)stream, r.st, r.T, r.s,
                       kSiteAttention, total, d_mask);
    OFP_LAUNCH_CHECK("k_site_mask");
    return OFP_OK;
}

}  // extern "C"
