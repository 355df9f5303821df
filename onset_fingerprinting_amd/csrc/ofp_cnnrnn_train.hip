// Training model.CNNRNN on the GPU (the reference's model.py:310-440): the conv stack of model.CNN (csrc/ofp_cnn_stack.h),
// the model's dropout on the conv features (site 0 of the random stream), a one-layer GRU whose time axis is the last
// conv layer's channels and whose features are its columns, 2-head self-attention with dropout on the softmax
// probabilities (site 3), the mean over time, out_proj and the Linear head with its loss; backward through all of it,
// one NAdam step, and optionally an eval-mode validation pass with the early-stop rule.  One epoch is a linear chain of
// kernels on one stream, captured once and replayed by run_epochs (csrc/ofp_train_chain.h), as for the other trainers.
//
// The dense layer, GRU and attention kernels, their launch helpers and how they sum are in csrc/ofp_seq_train.h, which
// the RNN trainer (csrc/ofp_rnn_train.hip) shares; here the attention runs its 128-step instantiation.
#include "ofp_seq_train.h"

namespace {

constexpr int kMaxSteps = kAttnCapShort;  // GRU / attention time steps (the last conv layer's channels)
constexpr int kMaxFeat = 2 * kMaxWidth;   // GRU input features (the last conv layer's columns)

int check_gru(const char* who, int64_t n, int T, int F, int H) {
    return check_gru(who, n, T, F, H, kMaxSteps, kMaxFeat);
}

int check_attn(const char* who, int64_t n, int T, int E, int heads) {
    return check_attn(who, n, T, E, heads, kMaxSteps);
}

struct Plan : WsPlan {
    int L, act, bn, pool, loss, O, np, ns;
    int T, F, H, heads;  // GRU steps (last conv channels), features (last conv columns), hidden size = attention width
    double eps;
    float mom;
    Conv conv[kMaxConv];
    int wo[kMaxConv];
    int w_off[kMaxConv], b_off[kMaxConv], g_off[kMaxConv], be_off[kMaxConv], rs_off[kMaxConv];
    int wih_off, whh_off, bih_off, bhh_off, inw_off, inb_off, ow_off, ob_off, fcw_off, fcb_off;
    // work space, byte offsets
    int64_t o_Z[kMaxConv], o_H[kMaxConv], o_HD, o_wiht, o_whht, o_inwt, o_owt, o_gx, o_gates, o_hseq, o_qkv, o_P, o_ctx,
        o_ao, o_out, o_dy, o_lpart, o_dao, o_dctx, o_ds, o_dqkv, o_dhseq, o_dgx, o_dgh, o_hprev, o_gh, o_gz, o_save,
        o_s12, o_part, o_G, o_M, o_V, o_RS, o_ctl, o_X;
};

int make_plan(const ofp_cnnrnn_config* cc, int64_t n, int64_t n_val, Plan& p, const Random& rnd = Random{}) {
    OFP_REQUIRE(cc != nullptr, "cnnrnn training: config is NULL");
    const ofp_cnn_config* c = &cc->cnn;
    OFP_REQUIRE(c->n_conv >= 1 && c->n_conv <= kMaxConv, "cnnrnn training: %d conv layers (limit: 1..%d)", c->n_conv,
                kMaxConv);
    OFP_REQUIRE(n_val >= 0 && n_val <= kMaxBatch, "cnnrnn training: validation batch of %lld (limit: 0..%d)",
                (long long)n_val, kMaxBatch);
    OFP_REQUIRE(c->act >= 0 && c->act <= OFP_ACT_TANH, "cnnrnn training: unknown activation %d", c->act);
    OFP_REQUIRE(c->loss == 0 || c->loss == 1, "cnnrnn training: loss %d (0 = L1, 1 = MSE)", c->loss);
    OFP_REQUIRE(c->n_out >= 1 && c->n_out <= kMaxOut, "cnnrnn training: %d outputs (limit: 1..%d)", c->n_out, kMaxOut);
    if (c->batch_norm)
        OFP_REQUIRE(c->bn_momentum > 0.0f && c->bn_momentum <= 1.0f && c->bn_eps > 0.0,
                    "cnnrnn training: BatchNorm momentum %g, eps %g (a cumulative average, momentum=None, is not built)",
                    (double)c->bn_momentum, c->bn_eps);
    p = Plan{};
    p.L = c->n_conv, p.act = c->act, p.bn = c->batch_norm ? 1 : 0, p.pool = c->pool ? 1 : 0, p.loss = c->loss;
    p.O = c->n_out, p.eps = c->bn_eps, p.mom = c->bn_momentum;
    const int64_t nmax = n > n_val ? n : n_val;
    int width = c->width, np = 0, ns = 0;
    int64_t max_h = 0, max_z = 0, max_part = 2 * 8;  // bytes
    for (int l = 0; l < p.L; ++l) {
        const int cin = c->channels[l], cout = c->channels[l + 1];
        if (int rc = check_conv("cnnrnn training", n, cin, width, cout, c->kernel, c->padding, c->dilation, c->groups))
            return rc;
        Conv& v = p.conv[l];
        v = Conv{cin, cout, width, width + 2 * c->padding - c->dilation * (c->kernel - 1), c->kernel, c->padding,
                 c->dilation, c->groups, 1};
        OFP_REQUIRE(v.wc <= 2 * kMaxWidth, "cnnrnn training: layer %d is %d wide (limit: %d)", l + 1, v.wc,
                    2 * kMaxWidth);
        p.wo[l] = p.pool ? v.wc / 2 : v.wc;
        OFP_REQUIRE(p.wo[l] >= 1, "cnnrnn training: the pool of layer %d leaves no output column", l + 1);
        OFP_REQUIRE(!p.bn || n * v.wc >= 2, "cnnrnn training: BatchNorm needs more than 1 value per channel");
        const int Tw = cin / c->groups * c->kernel + 1;
        p.w_off[l] = np, np += cout * (Tw - 1);
        p.b_off[l] = np, np += cout;
        if (p.bn) {
            p.g_off[l] = np, np += cout;
            p.be_off[l] = np, np += cout;
            p.rs_off[l] = ns, ns += 2 * cout;
        }
        max_part = std::max<int64_t>(max_part, (int64_t)cout * Tw * slabs_of(n * v.wc) * 8);
        max_h = std::max<int64_t>(max_h, nmax * cout * p.wo[l]);
        max_z = std::max<int64_t>(max_z, nmax * cout * v.wc);
        width = p.wo[l];
    }
    p.T = c->channels[p.L], p.F = width, p.H = cc->hidden, p.heads = cc->heads;
    if (int rc = check_gru("cnnrnn training", n, p.T, p.F, p.H)) return rc;
    if (int rc = check_attn("cnnrnn training", n, p.T, p.H, p.heads)) return rc;
    const int H = p.H, F = p.F, T = p.T;
    p.wih_off = np, np += 3 * H * F;
    p.whh_off = np, np += 3 * H * H;
    p.bih_off = np, np += 3 * H;
    p.bhh_off = np, np += 3 * H;
    p.inw_off = np, np += 3 * H * H;
    p.inb_off = np, np += 3 * H;
    p.ow_off = np, np += H * H;
    p.ob_off = np, np += H;
    p.fcw_off = np, np += p.O * H;
    p.fcb_off = np, np += p.O;
    p.np = np, p.ns = ns;
    max_part = std::max<int64_t>(max_part, (int64_t)fc_chunks(n) * p.O * H * 8);
    max_part = std::max<int64_t>(max_part, lin_part_bytes(n * T, F, 3 * H));
    max_part = std::max<int64_t>(max_part, lin_part_bytes(n * T, H, 3 * H));
    max_part = std::max<int64_t>(max_part, lin_part_bytes(n, H, H));
    for (int l = 0; l < p.L; ++l) {
        p.o_Z[l] = p.take(nmax * p.conv[l].cout * p.conv[l].wc * 4);
        p.o_H[l] = p.take(nmax * p.conv[l].cout * p.wo[l] * 4);
    }
    const int64_t rows = nmax * T, sq = nmax * p.heads * T * T;
    p.o_wiht = p.take((int64_t)3 * H * F * 4);
    p.o_whht = p.take((int64_t)3 * H * H * 4);
    p.o_inwt = p.take((int64_t)3 * H * H * 4);
    p.o_owt = p.take((int64_t)H * H * 4);
    p.o_gx = p.take(rows * 3 * H * 4);
    p.o_gates = p.take(rows * 4 * H * 4);
    p.o_hseq = p.take(rows * H * 4);
    p.o_qkv = p.take(rows * 3 * H * 4);
    p.o_P = p.take(sq * 4);
    p.o_ctx = p.take(nmax * H * 4);
    p.o_ao = p.take(nmax * H * 4);
    p.o_out = p.take(nmax * p.O * 4);
    p.o_dy = p.take(nmax * p.O * 4);
    p.o_lpart = p.take(nmax * 8);
    p.o_dao = p.take(n * H * 4);
    p.o_dctx = p.take(n * H * 4);
    p.o_ds = p.take(n * p.heads * T * T * 4);
    p.o_dqkv = p.take(n * T * 3 * H * 4);
    p.o_dhseq = p.take(n * T * H * 4);
    p.o_dgx = p.take(n * T * 3 * H * 4);
    p.o_dgh = p.take(n * T * 3 * H * 4);
    p.o_hprev = p.take(n * T * H * 4);
    p.o_gh = p.take(max_h * 4);
    p.o_gz = p.take(max_z * 4);
    p.o_save = p.take((int64_t)ns * 4);
    p.o_s12 = p.take((int64_t)ns * 4);
    p.o_part = p.take(max_part);
    p.o_G = p.take((int64_t)np * 4);
    p.o_M = p.take((int64_t)np * 4);
    p.o_V = p.take((int64_t)np * 4);
    p.o_RS = p.take((int64_t)ns * 4);
    p.o_ctl = p.take(sizeof(Ctl));
    if (rnd.drop) p.o_HD = p.take(n * T * F * 4);
    if (rnd.windows) p.o_X = p.take(n * c->channels[0] * c->width * 4);
    return OFP_OK;
}

struct Run : WsRun {
    const Plan* p;
    float* P;    // packed parameters
    float* RS;   // packed running statistics
    float* G;    // packed gradients
    Ctl* ctl;    // NULL: a single pass, epoch 0 (rnd.st.epoch for the random stream)
    hipStream_t st;
    Random rnd;  // dropout (conv features, attention probabilities) and the window source; both off by default
};

Post post_of(const Run& r, int l, int mode) {
    const Plan& p = *r.p;
    Post t{};
    t.C = p.conv[l].cout, t.wc = p.conv[l].wc, t.wo = p.wo[l], t.act = p.act, t.pool = p.pool, t.mode = mode;
    t.eps = p.eps;
    if (mode) {
        t.ga = r.P + p.g_off[l], t.be = r.P + p.be_off[l];
        if (mode == 1) {
            t.mean = r.at<float>(p.o_save) + p.rs_off[l], t.rs = t.mean + t.C;
        } else {
            t.mean = r.RS + p.rs_off[l], t.rs = t.mean + t.C;
        }
    }
    return t;
}

// the features the GRU reads: the last conv layer's output, dropped when the run has dropout
const float* features_of(const Run& r) {
    const Plan& p = *r.p;
    return r.at<float>(r.rnd.drop ? p.o_HD : p.o_H[p.L - 1]);
}

// the whole network on a batch, its mean loss into `curve`; train: batch statistics, both dropouts, d loss / d out
// kept and the head's bias gradient; else running statistics, no dropout, L1 and the early-stop rule
int enqueue_forward(const Run& r, const float* x, const float* y, int64_t n, bool train, float* curve, int patience) {
    const Plan& p = *r.p;
    const float* in = x;
    for (int l = 0; l < p.L; ++l) {
        const Conv& c = p.conv[l];
        float* Z = r.at<float>(p.o_Z[l]);
        float* Hl = r.at<float>(p.o_H[l]);
        hipLaunchKernelGGL(k_conv_fwd, dim3(grid_for(n * c.cout * c.wc)), dim3(kT), 0, r.st, r.ctl, c, n, in,
                           r.P + p.w_off[l], r.P + p.b_off[l], Z);
        OFP_LAUNCH_CHECK("k_conv_fwd");
        const Post t = post_of(r, l, p.bn ? (train ? 1 : 2) : 0);
        if (p.bn && train) {
            float* save = r.at<float>(p.o_save) + p.rs_off[l];
            if (int rc = enqueue_bn_stats(r.ctl, Z, n, c.cout, c.wc, p.act, p.eps, p.mom, r.at<double>(p.o_part), save,
                                          save + c.cout, r.RS + p.rs_off[l], r.RS + p.rs_off[l] + c.cout, r.st))
                return rc;
        }
        hipLaunchKernelGGL(k_post, dim3(grid_for(n * c.cout * p.wo[l])), dim3(kT), 0, r.st, r.ctl, t, n, Z, Hl);
        OFP_LAUNCH_CHECK("k_post");
        in = Hl;
    }
    const int T = p.T, F = p.F, H = p.H;
    if (train && r.rnd.drop) {
        float* HD = r.at<float>(p.o_HD);
        if (int rc = enqueue_dropout_fwd(r.ctl, r.rnd, in, HD, n * T * F, r.st)) return rc;
        in = HD;
    }
    float* wiht = r.at<float>(p.o_wiht);
    float* whht = r.at<float>(p.o_whht);
    float* inwt = r.at<float>(p.o_inwt);
    float* owt = r.at<float>(p.o_owt);
    if (int rc = enqueue_transpose(r.ctl, r.P + p.wih_off, 3 * H, F, wiht, r.st)) return rc;
    if (int rc = enqueue_transpose(r.ctl, r.P + p.whh_off, 3 * H, H, whht, r.st)) return rc;
    if (int rc = enqueue_transpose(r.ctl, r.P + p.inw_off, 3 * H, H, inwt, r.st)) return rc;
    if (int rc = enqueue_transpose(r.ctl, r.P + p.ow_off, H, H, owt, r.st)) return rc;
    float* gx = r.at<float>(p.o_gx);
    float* hseq = r.at<float>(p.o_hseq);
    float* qkv = r.at<float>(p.o_qkv);
    float* ctx = r.at<float>(p.o_ctx);
    float* ao = r.at<float>(p.o_ao);
    if (int rc = enqueue_lin_fwd(r.ctl, in, n * T, F, 3 * H, wiht, r.P + p.bih_off, gx, r.st)) return rc;
    if (int rc = enqueue_gru_fwd(r.ctl, gx, whht, r.P + p.bhh_off, n, T, H, hseq, r.at<float>(p.o_gates), r.st))
        return rc;
    if (int rc = enqueue_lin_fwd(r.ctl, hseq, n * T, H, 3 * H, inwt, r.P + p.inb_off, qkv, r.st)) return rc;
    if (int rc = enqueue_attn_fwd(r.ctl, attn_of(n, T, H, p.heads, r.rnd, train), kMaxSteps, qkv, r.at<float>(p.o_P),
                                  ctx, r.st))
        return rc;
    if (int rc = enqueue_lin_fwd(r.ctl, ctx, n, H, H, owt, r.P + p.ob_off, ao, r.st)) return rc;
    const Fc f{ao, n, H, p.O, r.P + p.fcw_off, r.P + p.fcb_off, y};
    return enqueue_fc_forward(r.ctl, f, p.loss, r.at<float>(p.o_out), train ? r.at<float>(p.o_dy) : nullptr,
                              r.at<double>(p.o_lpart), curve, patience, r.G + p.fcb_off, r.st);
}

int enqueue_backward(const Run& r, const float* x, int64_t n) {
    const Plan& p = *r.p;
    const int T = p.T, F = p.F, H = p.H;
    float* GH = r.at<float>(p.o_gh);
    float* GZ = r.at<float>(p.o_gz);
    double* part = r.at<double>(p.o_part);
    float* dao = r.at<float>(p.o_dao);
    float* dctx = r.at<float>(p.o_dctx);
    float* dqkv = r.at<float>(p.o_dqkv);
    float* dhseq = r.at<float>(p.o_dhseq);
    float* dgx = r.at<float>(p.o_dgx);
    float* dgh = r.at<float>(p.o_dgh);
    float* hprev = r.at<float>(p.o_hprev);
    const float* hseq = r.at<float>(p.o_hseq);
    const float* qkv = r.at<float>(p.o_qkv);
    const Fc f{r.at<float>(p.o_ao), n, H, p.O, r.P + p.fcw_off, r.P + p.fcb_off, nullptr};
    if (int rc = enqueue_fc_backward(r.ctl, f, r.at<float>(p.o_dy), part, r.G + p.fcw_off, dao, r.st)) return rc;
    if (int rc = enqueue_lin_bwd(r.ctl, r.at<float>(p.o_ctx), n, H, H, r.P + p.ow_off, dao, part, dctx,
                                 r.G + p.ow_off, r.G + p.ob_off, r.st))
        return rc;
    if (int rc = enqueue_attn_bwd(r.ctl, attn_of(n, T, H, p.heads, r.rnd, true), kMaxSteps, qkv, r.at<float>(p.o_P),
                                  dctx, r.at<float>(p.o_ds), dqkv, r.st))
        return rc;
    if (int rc = enqueue_lin_bwd(r.ctl, hseq, n * T, H, 3 * H, r.P + p.inw_off, dqkv, part, dhseq, r.G + p.inw_off,
                                 r.G + p.inb_off, r.st))
        return rc;
    if (int rc = enqueue_gru_bwd(r.ctl, r.P + p.whh_off, hseq, r.at<float>(p.o_gates), dhseq, n, T, H, dgx, dgh, hprev,
                                 r.st))
        return rc;
    if (int rc = enqueue_lin_bwd(r.ctl, hprev, n * T, H, 3 * H, r.P + p.whh_off, dgh, part, nullptr, r.G + p.whh_off,
                                 r.G + p.bhh_off, r.st))
        return rc;
    if (int rc = enqueue_lin_bwd(r.ctl, features_of(r), n * T, F, 3 * H, r.P + p.wih_off, dgx, part, GH,
                                 r.G + p.wih_off, r.G + p.bih_off, r.st))
        return rc;
    if (r.rnd.drop)
        if (int rc = enqueue_dropout_bwd(r.ctl, r.rnd, GH, n * T * F, r.st)) return rc;
    for (int l = p.L - 1; l >= 0; --l) {
        const Post t = post_of(r, l, p.bn ? 1 : 0);
        const float* Z = r.at<float>(p.o_Z[l]);
        if (int rc = enqueue_post_bwd(r.ctl, t, n, Z, GH, part, r.at<float>(p.o_s12) + p.rs_off[l],
                                      r.G + p.g_off[l], r.G + p.be_off[l], GZ, r.st))
            return rc;
        const float* in = l == 0 ? x : r.at<float>(p.o_H[l - 1]);
        if (int rc = enqueue_conv_bwd(r.ctl, p.conv[l], n, in, r.P + p.w_off[l], GZ, part, r.G + p.w_off[l],
                                      r.G + p.b_off[l], l == 0 ? nullptr : GH, r.st))
            return rc;
    }
    return OFP_OK;
}

int enqueue_step(const Run& r, const float* rows) {
    const Plan& p = *r.p;
    hipLaunchKernelGGL(k_nadam, dim3(grid_for(p.np)), dim3(kT), 0, r.st, r.ctl, rows, r.P, r.G, r.at<float>(p.o_M),
                       r.at<float>(p.o_V), (int64_t)p.np);
    OFP_LAUNCH_CHECK("k_nadam");
    return OFP_OK;
}

}  // namespace

extern "C" {

int32_t ofp_linear_backward_slab(void) { return kLinSlab; }

int64_t ofp_cnnrnn_train_stretch_workspace_bytes(const ofp_cnnrnn_config* cfg, int64_t n, int64_t n_val,
                                                 const ofp_train_random* random, int32_t stretch_span) {
    Plan p;
    Random rnd;
    if (cfg == nullptr ||
        make_random("cnnrnn training", random, stretch_span, n, cfg->cnn.channels[0], cfg->cnn.width, true, rnd))
        return -1;
    if (make_plan(cfg, n, n_val, p, rnd)) return -1;
    return p.bytes;
}

int ofp_cnnrnn_train_stretch(const ofp_cnnrnn_config* cfg, int64_t n, const float* d_x, const float* d_y,
                             int64_t n_val, const float* d_x_val, const float* d_y_val, const float* d_rates,
                             int32_t num_epochs, int32_t min_epochs, int32_t patience, float* d_params, float* d_stats,
                             float* d_train_loss, float* d_val_loss, int32_t* h_epochs, void* d_ws, int64_t ws_bytes,
                             void* stream, const ofp_train_random* random, int32_t stretch_span) {
    Plan p;
    Random rnd;
    OFP_REQUIRE(cfg != nullptr, "cnnrnn training: config is NULL");
    if (int rc = make_random("ofp_cnnrnn_train", random, stretch_span, n, cfg->cnn.channels[0], cfg->cnn.width, true,
                             rnd))
        return rc;
    if (int rc = make_plan(cfg, n, n_val, p, rnd)) return rc;
    if (rnd.windows && d_ws) d_x = reinterpret_cast<const float*>((const char*)d_ws + p.o_X);
    const TrainArgs a{d_x, d_y, n, d_x_val, d_y_val, n_val, d_rates, min_epochs, patience, d_train_loss, d_val_loss};
    if (int rc = check_train("ofp_cnnrnn_train", a, num_epochs, d_params, h_epochs)) return rc;
    OFP_REQUIRE(p.ns == 0 || d_stats, "ofp_cnnrnn_train: BatchNorm statistics are NULL");
    if (int rc = check_ws("ofp_cnnrnn_train", d_ws, ws_bytes, p.bytes)) return rc;
    hipStream_t st = (hipStream_t)stream;
    Run r{{(char*)d_ws}, &p, d_params, d_stats, nullptr, nullptr, st, rnd};
    r.G = r.at<float>(p.o_G);
    r.ctl = r.at<Ctl>(p.o_ctl);
    return run_epochs(
        "ofp_cnnrnn_train", "OFP_CNNRNN_GRAPH", st, r.ctl, num_epochs, patience, h_epochs,
        [&] {
            OFP_HIP(hipMemsetAsync(r.at<float>(p.o_M), 0, (size_t)p.np * 4, st));
            OFP_HIP(hipMemsetAsync(r.at<float>(p.o_V), 0, (size_t)p.np * 4, st));
            return OFP_OK;
        },
        [&] { return enqueue_epoch(r, a); });
}

int64_t ofp_cnnrnn_loss_grads_random_workspace_bytes(const ofp_cnnrnn_config* cfg, int64_t n, int64_t n_val,
                                                     const ofp_train_random* random) {
    return ofp_cnnrnn_train_stretch_workspace_bytes(cfg, n, n_val, random, 0);
}

int ofp_cnnrnn_loss_grads_random(const ofp_cnnrnn_config* cfg, int64_t n, const float* d_x, const float* d_y,
                                 const float* d_params, float* d_loss, float* d_grads, void* d_ws, int64_t ws_bytes,
                                 void* stream, const ofp_train_random* random) {
    Plan p;
    Random rnd;
    if (int rc = make_random("ofp_cnnrnn_loss_grads", random, 0, n, 0, 0, false, rnd)) return rc;
    if (int rc = make_plan(cfg, n, 0, p, rnd)) return rc;
    OFP_REQUIRE(d_x && d_y && d_params && d_loss && d_grads, "ofp_cnnrnn_loss_grads: NULL argument");
    if (int rc = check_ws("ofp_cnnrnn_loss_grads", d_ws, ws_bytes, p.bytes)) return rc;
    // the trainer's own forward and backward; the running statistics it would update are a scratch copy
    Run r{{(char*)d_ws}, &p, const_cast<float*>(d_params), nullptr, d_grads, nullptr, (hipStream_t)stream, rnd};
    r.RS = r.at<float>(p.o_RS);
    OFP_HIP(hipMemsetAsync(r.RS, 0, (size_t)(p.ns > 0 ? p.ns : 1) * 4, r.st));
    return enqueue_loss_grads(r, d_x, d_y, n, d_loss);
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
