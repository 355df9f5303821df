// The window regressor of a stream ("The window regressor in the hop"): detection.find_onset_groups
// as an online state machine, the FIFO of kept groups, the window of the group that is due, and the forward pass of a
// model.CNN / model.CCCNN on it (ofp_nn_dev.h) -- one step per hop, by one workgroup of 256 threads.  The hop's fused
// kernel and regress node (ofp_hop.hip) and the replay (ofp_regress_stream, ofp_regress.hip) run this one function.
#pragma once
#include "ofp_common.h"
#include "ofp_nn_dev.h"

namespace ofpreg {

constexpr int KIND_CNN = 0, KIND_CCCNN = 1, KIND_CCCNN_GROUPED = 2;
constexpr int NORM_NONE = 0, NORM_BATCH = 1, NORM_GROUP = 2;
// Activations live in LDS while the stage's whole dynamic LDS stays within this; above it they live in the
// session's device workspace (the fused kernel's static LDS, about 20 KiB, comes on top of either).
constexpr size_t LDS_SWITCH = 96 * 1024;
constexpr size_t LDS_RED = 16;  // the stage's LDS starts with the softmax's four partials

struct Layer {
    int cin, cout, k, stride, win, wout;  // wout: after the pool fused into the conv kernel, if any
    int pool_conv, pool_gn, wgn;          // wgn: width after the GroupNorm (and its pool)
    int w_off, b_off, p0_off, p1_off;     // float offsets: weight, bias, (scale, shift) or (gamma, beta)
};

struct Plan {
    int kind, C, W, n_out, n_conv, padding, dilation, groups, act, norm;
    float eps;
    int items;        // items the conv stack sees: C for the shared CCCNN stack, 1 otherwise
    int K, V;         // CCCNN: maps per sensor channel and their width after the stack
    int fc_in, fc_w, fc_b;
    int act_floats;   // floats of one activation buffer (the largest tensor between two layers, the window included)
    int n_params;
    int use_lds;      // activations in LDS (else in `ws`)
    const float* params;
    Layer L[OFP_REG_MAX_LAYERS];
};

struct Cfg {
    Plan plan;
    int B, F, pre, D, min_channels;  // block size, frame_length, pre_samples, max_distance
    ofp_regress_state* state;
    float* ws;                       // [2 * act_floats] when !plan.use_lds
};

inline size_t lds_bytes(const Plan& p) { return LDS_RED + (p.use_lds ? 2 * (size_t)p.act_floats * 4 : 0); }

// The forward pass on the window in `a` ([C][W]); b is the other activation buffer.  y [n_out] receives the result.
__device__ __forceinline__ void forward(const Plan& p, float* a, float* b, float* red, float* y) {
    const float* prm = p.params;
    float *src = a, *dst = b;
    auto swap = [&] {
        float* t = src;
        src = dst;
        dst = t;
    };
    for (int l = 0; l < p.n_conv; ++l) {
        const Layer& L = p.L[l];
        const bool bn = p.norm == NORM_BATCH;
        ofpnn::conv_items(src, p.items, L.cin, L.win, prm + L.w_off, L.b_off >= 0 ? prm + L.b_off : nullptr, L.cout, L.k,
                          p.padding, p.dilation, p.groups, L.stride, p.act, bn ? prm + L.p0_off : nullptr,
                          bn ? prm + L.p1_off : nullptr, L.pool_conv, L.wout, dst);
        __syncthreads();
        swap();
        if (p.norm == NORM_GROUP) {
            for (int it = 0; it < p.items; ++it)
                ofpnn::groupnorm_item(src + it * L.cout * L.wout, L.cout, L.wout, prm + L.p0_off, prm + L.p1_off, p.eps,
                                      L.pool_gn, dst + it * L.cout * L.wgn);
            swap();
        }
    }
    if (p.kind == KIND_CNN) {
        ofpnn::dense_row(src, p.fc_in, p.n_out, prm + p.fc_w, prm + p.fc_b, nullptr, nullptr, OFP_ACT_IDENTITY, y);
        return;
    }
    const int Lags = 2 * p.V - 1;
    // [C][K][V] either way: the shared stack's items, or the grouped conv's channel order
    ofpnn::autocorr_items(src, p.C, p.K, p.V, dst);
    __syncthreads();
    for (int c = 0; c < p.C; ++c) ofpnn::softmax_item(dst + c * Lags, Lags, red);
    ofpnn::dense_row(dst, p.fc_in, p.n_out, prm + p.fc_w, prm + p.fc_b, nullptr, nullptr, OFP_ACT_IDENTITY, y);
}

// The window from row `start` into `a` ([C][F]: FrameExtractor, use_min_onset, the same rows for every channel) and the
// forward pass on it.  Called once with LDS buffers and once with the workspace's, so that each copy of the layers
// addresses one kind of memory.
template <class Sample>
__device__ __forceinline__ void evaluate(const Cfg& g, int64_t start, Sample sample, float* a, float* red, float* o_y) {
    const int C = g.plan.C;
    for (int i = threadIdx.x; i < C * g.F; i += ofpnn::WG) {
        const int c = i / g.F, j = i - c * g.F;
        a[i] = sample(start + j, c);
    }
    __syncthreads();
    forward(g.plan, a, a + g.plan.act_floats, red, o_y);
}

// A hop with nothing to feed, close or evaluate: one comparison with the word the last busy hop left (`wake`: the
// first hop end at which the open group times out or the FIFO's head is due).  The caller loads st->wake, as early
// as it likes.  G: a stage's configuration with B, F, pre, D, min_channels and state (this stage's Cfg, or the voting
// locator's, ofp_paired_dev.h).
template <class G>
__device__ __forceinline__ bool idle(const G& g, int64_t h, int n, int64_t wake) {
    return n <= 0 && h * (int64_t)g.B < wake;
}

// The grouping state machine and the FIFO for one hop, by ONE thread: the hop's n onsets are fed, groups close, and
// the head is taken off the FIFO if its window is complete.  Returns the head's slot (its q_start and q_row stay in
// the state until a later group takes the slot), or -1 when nothing is due; then *o_start and o_row [C] are written.
// *o_flags always.  h, n, rec as `step` takes them.
template <class G, class Rec>
__device__ __forceinline__ int queue_step(const G& g, int C, int64_t h, int n, Rec rec, int64_t* o_start, int64_t* o_row,
                                          int32_t* o_flags) {
    ofp_regress_state* st = g.state;
    const int64_t end = h * (int64_t)g.B;
    int open = st->open, head = st->head, len = st->len, flags = st->flags;
    int64_t anchor = st->anchor;
    auto close = [&] {
        int present = 0;
        int64_t first = -1;
        for (int c = 0; c < C; ++c) {
            const int64_t v = st->row[c];
            if (v >= 0) {
                ++present;
                if (first < 0 || v < first) first = v;
            }
        }
        if (present >= g.min_channels) {
            if (len >= OFP_REG_QUEUE) {
                flags |= OFP_REGF_QUEUE;
            } else {
                const int q = (head + len) % OFP_REG_QUEUE;
                st->q_start[q] = first - g.pre;
                for (int c = 0; c < C; ++c) st->q_row[q][c] = st->row[c];
                ++len;
            }
        }
        open = 0;
    };
    for (int i = 0; i < n; ++i) {
        int ch;
        int64_t s;
        rec(i, ch, s);
        if (ch < 0 || ch >= C || s < 0) {
            flags |= OFP_REGF_BAD_ONSET;
            continue;
        }
        if (open && s - anchor > g.D) close();
        if (!open) {
            open = 1;
            anchor = s;
            for (int c = 0; c < C; ++c) st->row[c] = -1;
        }
        st->row[ch] = s;
    }
    if (open && end > anchor + g.D) close();
    int slot = -1;
    if (len > 0 && end >= st->q_start[head] + g.F) {
        slot = head;
        *o_start = st->q_start[head];
        for (int c = 0; c < C; ++c) o_row[c] = st->q_row[head][c];
        head = (head + 1) % OFP_REG_QUEUE;
        --len;
    }
    int64_t wake = INT64_MAX;
    if (open) wake = anchor + g.D + 1;
    if (len > 0) wake = min(wake, (int64_t)(st->q_start[head] + g.F));
    st->open = open;
    st->anchor = anchor;
    st->wake = wake;
    st->head = head;
    st->len = len;
    st->flags = flags;
    *o_flags = flags;
    return slot;
}

// One hop of the stage that is not idle.  h: hops pushed including this one; rec(i) -> (channel, absolute sample) of
// the hop's i-th onset in feed order (sorted by sample, stable), n of them; sample(t, col): the stream's row t, column
// col, for start <= t < h * B.  lds: lds_bytes(plan) of LDS nobody else uses.  Outputs are written only when a hit
// is evaluated (return value 1, the same on every thread): o_start, o_row [C], o_y [n_out]; *o_flags always.
template <class Rec, class Sample>
__device__ __forceinline__ int step(const Cfg& g, int64_t h, int n, Rec rec, Sample sample, unsigned char* lds,
                                    int64_t* o_start, int64_t* o_row, float* o_y, int32_t* o_flags) {
    __shared__ int s_eval;
    __shared__ int64_t s_start;
    if (threadIdx.x == 0) {
        const int slot = queue_step(g, g.plan.C, h, n, rec, o_start, o_row, o_flags);
        s_eval = slot >= 0;
        if (slot >= 0) s_start = g.state->q_start[slot];
    }
    __syncthreads();
    const int eval = s_eval;
    if (!eval) return 0;
    float* red = reinterpret_cast<float*>(lds);
    if (g.plan.use_lds)
        evaluate(g, s_start, sample, reinterpret_cast<float*>(lds + LDS_RED), red, o_y);
    else
        evaluate(g, s_start, sample, g.ws, red, o_y);
    return 1;
}

}  // namespace ofpreg

// The checked launch form of `r` (ofp_regress.hip): the plan with its offsets into a parameter block laid out as
// ofp_hop_regressor documents, without `params`; OFP_ERR_INVALID with `who` in the message outside the envelope.
int ofp_regress_plan(const ofp_hop_regressor* r, const char* who, ofpreg::Plan* out);
