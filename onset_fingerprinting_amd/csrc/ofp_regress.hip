// The window regressor outside a session: the checked plan of an ofp_hop_regressor (shared with ofp_hop.hip) and the
// replay ofp_regress_stream -- the stage of ofp_regress_dev.h over a resident recording and a given onset list, every
// hop in one launch of one workgroup.
#include <algorithm>
#include <cstring>

#include "ofp_regress_dev.h"

int ofp_regress_plan(const ofp_hop_regressor* r, const char* who, ofpreg::Plan* out) {
    using namespace ofpreg;
    OFP_REQUIRE(r && out, "%s: NULL argument", who);
    OFP_REQUIRE(r->kind >= KIND_CNN && r->kind <= KIND_CCCNN_GROUPED, "%s: unknown model kind %d", who, r->kind);
    OFP_REQUIRE(r->channels >= 1 && r->channels <= OFP_REG_MAX_SIGNALS, "%s: %d channels (1..%d supported)", who,
                r->channels, OFP_REG_MAX_SIGNALS);
    OFP_REQUIRE(r->n_conv >= 1 && r->n_conv <= OFP_REG_MAX_LAYERS, "%s: %d conv layers (1..%d supported)", who, r->n_conv,
                OFP_REG_MAX_LAYERS);
    OFP_REQUIRE(r->n_out >= 1 && r->n_out <= OFP_REG_MAX_OUT, "%s: %d outputs (1..%d supported)", who, r->n_out,
                OFP_REG_MAX_OUT);
    OFP_REQUIRE(r->width >= 1 && r->width <= OFP_REG_MAX_FRAME, "%s: input width %d (1..%d supported)", who, r->width,
                OFP_REG_MAX_FRAME);
    OFP_REQUIRE(r->frame_length == r->width, "%s: frame_length %d, the model takes %d samples", who, r->frame_length,
                r->width);
    OFP_REQUIRE(r->padding >= 0 && r->dilation >= 1, "%s: need padding >= 0 and dilation >= 1", who);
    OFP_REQUIRE(r->act >= OFP_ACT_IDENTITY && r->act <= OFP_ACT_TANH, "%s: unknown activation %d", who, r->act);
    OFP_REQUIRE(r->norm == NORM_NONE || (r->norm == NORM_BATCH && r->kind == KIND_CNN) ||
                    (r->norm == NORM_GROUP && r->kind != KIND_CNN),
                "%s: norm %d does not go with model kind %d", who, r->norm, r->kind);
    OFP_REQUIRE(r->pre_samples >= 0 && r->max_distance >= 0 && r->min_channels >= 1 && r->min_channels <= r->channels,
                "%s: need pre_samples >= 0, max_distance >= 0 and 1 <= min_channels <= %d", who, r->channels);
    OFP_REQUIRE(r->d_params, "%s: NULL parameters", who);
    Plan p;
    std::memset(&p, 0, sizeof(p));
    p.kind = r->kind;
    p.C = r->channels;
    p.W = r->width;
    p.n_out = r->n_out;
    p.n_conv = r->n_conv;
    p.padding = r->padding;
    p.dilation = r->dilation;
    p.act = r->act;
    p.norm = r->norm;
    p.eps = r->gn_eps;
    p.items = r->kind == KIND_CCCNN ? r->channels : 1;
    p.groups = r->kind == KIND_CCCNN ? 1 : r->kind == KIND_CCCNN_GROUPED ? r->channels : r->groups;
    OFP_REQUIRE(r->kind != KIND_CNN || r->groups >= 1, "%s: groups %d", who, r->groups);
    OFP_REQUIRE(r->kind == KIND_CNN || r->groups == p.groups, "%s: model kind %d runs its convolutions with %d groups, got %d",
                who, r->kind, p.groups, r->groups);
    int64_t off = 0, most = (int64_t)r->channels * r->width;
    int cin = r->kind == KIND_CCCNN ? 1 : r->channels, w = r->width;
    for (int l = 0; l < r->n_conv; ++l) {
        Layer& L = p.L[l];
        L.cin = cin;
        L.cout = r->cout[l];
        L.k = r->kernels[l];
        L.stride = r->strides[l];
        L.win = w;
        OFP_REQUIRE(L.cout >= 1 && L.cout <= 4096 && L.k >= 1 && L.stride >= 1, "%s: conv layer %d: cout %d, kernel %d, stride %d",
                    who, l, L.cout, L.k, L.stride);
        OFP_REQUIRE(cin % p.groups == 0 && L.cout % p.groups == 0, "%s: conv layer %d: groups %d must divide %d and %d", who,
                    l, p.groups, cin, L.cout);
        const int64_t span = (int64_t)w + 2 * (int64_t)r->padding - (int64_t)r->dilation * (L.k - 1);
        OFP_REQUIRE(span >= 1, "%s: conv layer %d leaves no output (width %d)", who, l, w);
        int wc = (int)((span - 1) / L.stride + 1);
        L.pool_conv = r->pool && r->norm != NORM_GROUP;
        L.pool_gn = r->pool && r->norm == NORM_GROUP;
        L.wout = L.pool_conv ? wc / 2 : wc;
        L.wgn = L.pool_gn ? L.wout / 2 : L.wout;
        OFP_REQUIRE(L.wout >= 1 && L.wgn >= 1, "%s: nothing left after the pool of layer %d", who, l);
        L.w_off = (int)off;
        off += (int64_t)L.cout * (cin / p.groups) * L.k;
        L.b_off = (int)off;
        off += L.cout;
        L.p0_off = L.p1_off = -1;
        if (r->norm != NORM_NONE) {
            L.p0_off = (int)off;
            L.p1_off = (int)off + L.cout;
            off += 2 * (int64_t)L.cout;
        }
        most = std::max(most, (int64_t)p.items * L.cout * L.wout);
        cin = L.cout;
        w = r->norm == NORM_GROUP ? L.wgn : L.wout;
        OFP_REQUIRE(most <= (1 << 20) && off < (1 << 28), "%s: conv layer %d is too large for the stage", who, l);
    }
    if (r->kind == KIND_CNN) {
        p.fc_in = cin * w;
    } else {
        p.K = r->kind == KIND_CCCNN ? cin : cin / r->channels;
        p.V = w;
        p.fc_in = r->channels * (2 * w - 1);
        most = std::max(most, (int64_t)p.fc_in);
    }
    p.fc_w = (int)off;
    off += (int64_t)p.n_out * p.fc_in;
    p.fc_b = (int)off;
    off += p.n_out;
    OFP_REQUIRE(off == r->n_params, "%s: the model has %lld parameters, the caller packed %lld", who, (long long)off,
                (long long)r->n_params);
    p.n_params = (int)off;
    p.act_floats = (int)((most + 3) & ~(int64_t)3);
    p.use_lds = 1;
    if (lds_bytes(p) > LDS_SWITCH) p.use_lds = 0;
    *out = p;
    return OFP_OK;
}

namespace {

struct ReplayArgs {
    ofpreg::Cfg g;
    const float* audio;
    int64_t n_rows, K;
    const int32_t* channel;
    const int64_t* onset;
    int32_t *status, *pending, *flags;
    int64_t *start, *row;
    float* y;
};

__global__ __launch_bounds__(256) void k_regress_stream(ReplayArgs a) {
    extern __shared__ __align__(16) unsigned char smem[];
    const ofpreg::Plan& p = a.g.plan;
    const int C = p.C, B = a.g.B;
    const int64_t H = a.n_rows / B;
    ofp_regress_state* st = a.g.state;
    int64_t next = 0;  // first onset not yet fed (the same on every thread)
    auto sample = [&](int64_t t, int col) -> float { return t < 0 ? 0.0f : a.audio[t * C + col]; };
    for (int64_t h = 1; h <= H; ++h) {
        const int64_t end = h * (int64_t)B;
        int n = 0;
        while (next + n < a.K && a.onset[next + n] < end) ++n;
        const int64_t base = next;
        auto rec = [&](int i, int& ch, int64_t& s) {
            ch = a.channel[base + i];
            s = a.onset[base + i];
        };
        // (the FIFO is longest after this hop's closes and before its evaluation: len + 1 if one was evaluated)
        int ev = 0;
        const bool busy = !ofpreg::idle(a.g, h, n, st->wake);
        __syncthreads();  // every thread has read `wake` before thread 0 of a busy hop stores the next one
        if (busy)
            ev = ofpreg::step(a.g, h, n, rec, sample, smem, a.start + (h - 1), a.row + (h - 1) * C, a.y + (h - 1) * p.n_out,
                              a.flags);
        __syncthreads();  // the state thread 0 left, and the step's shared words, before the next hop reads them
        if (threadIdx.x == 0) {
            a.status[h - 1] = ev;
            a.pending[h - 1] = st->len + ev;
        }
        next += n;
    }
    if (threadIdx.x == 0) *a.flags = st->flags;
}

}  // namespace

extern "C" {

int64_t ofp_regress_workspace_floats(const ofp_hop_regressor* r) {
    ofpreg::Plan p;
    if (ofp_regress_plan(r, "ofp_regress_workspace_floats", &p) != OFP_OK) return -1;
    return p.use_lds ? 0 : p.act_floats;
}

int ofp_regress_stream(const ofp_hop_regressor* r, const float* d_audio, int64_t n_rows, int32_t block_size,
                       const int32_t* d_channel, const int64_t* d_onset, int64_t K, int32_t* d_status, int64_t* d_start,
                       int64_t* d_row, float* d_y, int32_t* d_pending, int32_t* d_flags, float* d_ws, void* stream) {
    ReplayArgs a;
    std::memset(&a, 0, sizeof(a));
    if (int rc = ofp_regress_plan(r, "ofp_regress_stream", &a.g.plan)) return rc;
    OFP_REQUIRE(d_audio && d_status && d_start && d_row && d_y && d_pending && d_flags && (K == 0 || (d_channel && d_onset)),
                "ofp_regress_stream: NULL argument");
    OFP_REQUIRE(block_size >= 1 && n_rows >= 0 && K >= 0, "ofp_regress_stream: bad sizes");
    OFP_REQUIRE(a.g.plan.use_lds || d_ws, "ofp_regress_stream: the model needs a workspace (ofp_regress_workspace_floats)");
    hipStream_t st = (hipStream_t)stream;
    ofp_regress_state* d_state = nullptr;
    OFP_HIP(hipMalloc(&d_state, sizeof(ofp_regress_state)));
    auto run = [&]() -> int {
        OFP_HIP(hipMemsetAsync(d_state, 0, sizeof(ofp_regress_state), st));
        OFP_HIP(hipMemsetAsync(d_flags, 0, sizeof(int32_t), st));
        a.g.plan.params = r->d_params;
        a.g.B = block_size;
        a.g.F = r->frame_length;
        a.g.pre = r->pre_samples;
        a.g.D = r->max_distance;
        a.g.min_channels = r->min_channels;
        a.g.state = d_state;
        a.g.ws = d_ws;
        a.audio = d_audio;
        a.n_rows = n_rows;
        a.K = K;
        a.channel = d_channel;
        a.onset = d_onset;
        a.status = d_status;
        a.pending = d_pending;
        a.flags = d_flags;
        a.start = d_start;
        a.row = d_row;
        a.y = d_y;
        const size_t lds = ofpreg::lds_bytes(a.g.plan);
        static ofp::LdsAttrCache attr;
        if (int rc = ofp::ensure_dynamic_lds(reinterpret_cast<const void*>(k_regress_stream), lds, attr)) return rc;
        hipLaunchKernelGGL(k_regress_stream, dim3(1), dim3(256), lds, st, a);
        OFP_LAUNCH_CHECK("k_regress_stream");
        OFP_HIP(hipStreamSynchronize(st));  // (the state is freed below)
        return OFP_OK;
    };
    const int rc = run();
    (void)hipFree(d_state);
    return rc;
}

}  // extern "C"
