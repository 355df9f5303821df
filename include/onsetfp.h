/*
 * onsetfp.h -- C ABI of libonsetfp.so, the MI355X (gfx950) implementation of the
 * onset-fingerprinting hot path:
 *
 *   envelope follower / amplitude onset detector  ->  framing + Hann + rFFT
 *   power spectrum  ->  mel fingerprint  ->  small classifier forward.
 *
 * Plain pointers and sizes only; no torch or C++ types.  All `d_` pointers are
 * DEVICE pointers (HBM); `stream` is a hipStream_t passed as void* (NULL = the
 * null stream).  Every entry point except the three legacy symbols returns an
 * int status (OFP_OK == 0) and records a message retrievable with
 * ofp_last_error().  The library never allocates inside a launch function:
 * work space is provided by the caller (size from the *_workspace_bytes
 * query), so every launch function can be captured into a hipGraph.
 *
 * Reference interfaces replaced (paths under the upstream repo's
 * onset_fingerprinting/ directory):
 *   envelope_follower.c:6,27,59     the ctypes boundary of detection.py:517-578
 *   detection.py:595-888            AmplitudeOnsetDetector (__call__, warm-up)
 *   detection.py:19-86              detect_onsets_amplitude driver loop
 *   data.py:55-120                  FrameExtractor gather
 *   data.py:581-654                 stft_frame / stft
 *   data.py:657-680                 cspec_to_mfcc (mel + dB + DCT)
 *   calibration.py:463-560          FCNN forward
 *   model.py:52-120                 CNN forward
 *   model.py:168-440                RNN / CNNRNN forward
 */
#ifndef ONSETFP_H
#define ONSETFP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OFP_OK 0
#define OFP_ERR_INVALID 1   /* bad argument (shape, NULL, unsupported option) */
#define OFP_ERR_HIP 2       /* a HIP runtime call or kernel launch failed */
#define OFP_ERR_NODEVICE 3  /* no usable GPU */
#define OFP_ERR_WORKSPACE 4 /* caller-provided work space too small */
#define OFP_ERR_NOCONVERGE 5 /* speculative time-parallel pass did not converge */

#define OFP_ABI_VERSION 3

/* ---- status ---------------------------------------------------------------- */
int ofp_abi_version(void);
const char* ofp_last_error(void);
/* number of visible GPUs (>= 0) or a negative OFP_ERR_* */
int ofp_device_count(void);
/* writes the gcnArchName of `device` into buf; fails unless it is gfx950 */
int ofp_device_check(int device, char* buf, int buflen);

/* Process-wide settings of the HIP runtime that the library's in-flight use depends on.  A caller that keeps
 * several steps in flight gives every step two streams (its own and the spectral branch's); the runtime maps all
 * streams of a process onto GPU_MAX_HW_QUEUES hardware queues (its default: 4) in submission order, so with twelve
 * streams on four queues a short kernel of one step waits behind another step's long one.  Measured:
 * 8 and 16 queues equal, 32 slightly slower, 4 limits three and more steps in flight.
 *   ofp_runtime_prepare() sets GPU_MAX_HW_QUEUES=16 in the process environment (replacing any value) and returns 1.
 * The runtime reads the variable once, at the first HIP call of the process: when the runtime is already up the
 * function changes nothing and returns 0.  It makes no HIP call itself.  The Python package calls it at import. */
#define OFP_RUNTIME_QUEUES_VAR "GPU_MAX_HW_QUEUES"
#define OFP_RUNTIME_QUEUES "16"
int ofp_runtime_prepare(void);

/* ---- legacy symbols: drop-in for envelope_follower.so ---------------------------
 * Identical names, signatures and HOST-pointer semantics as envelope_follower.c:6,
 * :27 and :59, so that the reference's detection.py:517-578 can CDLL this library
 * unchanged.  Each call stages its arrays to the GPU, runs one kernel and copies
 * the in/out arrays back; they return void and report failures only through
 * ofp_last_error() (the reference ABI has no status).  */
void ar_envelope(float* x, float* y, float attack, float release, int size, int num_samples);
void minmax_envelope(float* x, float* min_val, float* max_val, float alpha_min, float alpha_max,
                     float minmin, int n_samples, int n_channels);
void backtrack_onsets(float* buffer, long* channels, long* deltas, float alpha, float tol,
                      long buffer_length, long n_onsets, long n_channels, long block_size);

/* ButterworthFilter.__call__ (detection.py:499-501): scipy.signal.lfilter(b, a, x, axis=0, zi) in
 * float32 (direct form II transposed, coefficients normalised by a[0] in fp32), HOST pointers like
 * the legacy symbols: x,y [n][n_channels]; b,a [order+1]; zi [order][n_channels] in/out; order <= 8 */
int ofp_lfilter(const float* x, float* y, const float* b, const float* a, int order, float* zi, long n,
                int n_channels);

/* ---- amplitude onset detector (detection.py:595-888) ----------------------------- */
typedef struct ofp_detector_params {
    int32_t n_channels;   /* C: signals per detector instance (detection.py:633) */
    int32_t block_size;   /* B (detection.py:634) */
    float floor_db;       /* floor (detection.py:635); zero or negative (-inf allowed): a positive or NaN floor is refused */
    int32_t hp_enabled;   /* hipass_freq != 0 (detection.py:692-696) */
    float hp_b[5];        /* np.float32(butter(4, f, "high", fs=sr)) (detection.py:492-496) */
    float hp_a[5];
    float fast_attack;    /* np.float32(1/attack): the COEFFICIENT (detection.py:514-515) */
    float fast_release;
    float slow_attack;
    float slow_release;
    float alpha_min;      /* 1e-4 (detection.py:705) */
    float alpha_max;      /* 1e-5 */
    float minmin;         /* 2 */
    float min0;           /* tracker start: 0 (detection.py:704) */
    float max0;           /* 10 */
    int32_t manual;       /* scalar on_threshold > 1 (detection.py:687) */
    int64_t cooldown;     /* samples (detection.py:640) */
    int32_t backtrack;    /* detection.py:641 */
    int64_t backtrack_buffer_size;
    float backtrack_alpha; /* np.float32(2/(smooth+1)) (detection.py:722) */
    float backtrack_tol;   /* np.float32((1-alpha)**buffer_size) (detection.py:723-725) */
} ofp_detector_params;

/* one detected onset: 16 bytes, also the record all-gathered across ranks */
typedef struct ofp_onset {
    int32_t clip;     /* clip (detector instance) index within the call */
    int32_t channel;  /* channel index in [0, C) */
    int64_t sample;   /* block_start + delta, relative to the clip's first sample */
} ofp_onset;

/* tuning of the speculative time-parallel passes; zero-initialise for defaults */
typedef struct ofp_detect_tuning {
    int64_t hp_chunk, hp_warm;   /* samples per chunk / speculative warm-up, IIR stage */
    int64_t ar_chunk, ar_warm;   /* follower stage */
    int64_t mm_chunk, mm_warm;   /* min/max tracker stage */
    int32_t max_passes;          /* repair passes before giving up (0: no limit) */
    int64_t ar_coarse_warm;      /* follower stage: approximate-arithmetic warm-up that
                                    produces the guess for the exact warm-up (<0: none) */
    int64_t hp_candidates;       /* IIR stage: speculative candidates per chunk (default 16, max 16) */
    int64_t hp_candidate_offset; /* IIR stage: samples between candidate starts (default 8); < 0: all
                                    candidates of a chunk start at the same sample from slightly
                                    different states */
    int64_t ar_guess;            /* follower stage, how the exact warm-up gets its starting guess:
                                    0 auto, 1 sequential approximate pass, 2 closed-form dot product
                                    (needs slow attack == slow release; auto picks it when they are) */
    int64_t hp_span;             /* IIR stage: 1 (default), 2 or 4 = chunks one speculative run walks through
                                    after its warm-up; > 1 shares the warm-up between chunks: less work,
                                    fewer waves, longer launch (throughput instead of latency) */
    int64_t ar_span, mm_span;    /* follower / tracker stage: chunks one speculative warm-up run walks through
                                    (0: chosen from the batch size, see make_layout) */
    int64_t verify_group;        /* verification passes / rounds enqueued per host synchronisation (0: default 2-3;
                                    1: one host round trip per pass, the round-1 behaviour) */
    int64_t hp_dedupe;           /* IIR stage: speculative candidates in stages with duplicate runs removed between
                                    them (a third of the steps, six launches instead of one): 0 auto (batches whose
                                    candidate launch is throughput-bound, when concurrent_calls >= 2), 1 always,
                                    < 0 never */
    int64_t hp_early;            /* IIR stage: a chunk re-run whole from its true start state stops at the first
                                    sub-chunk boundary where it has joined a candidate's recorded trajectory:
                                    0 auto (chunks of 32768 samples and more), 1 always, < 0 never */
    int64_t lane_merge;          /* follower / tracker stage: the two recurrences of a chunk (fast / slow follower,
                                    min / max) in one lane instead of two: half the reads of those passes, a longer
                                    dependent chain per lane: more frames/s when calls overlap, a slower lone call.
                                    0 auto (on when concurrent_calls >= 2), 1 always, < 0 never */
    int64_t fuse_db_sums;        /* the dB pass also forms the per-chunk sums of the slow follower's closed-form guess
                                    (one pass over the filtered stream instead of two): 0 on, < 0 off */
    int64_t sm_segments;         /* hysteresis / cooldown machine time-parallel over the list of visited blocks (clips of
                                    up to 64 channels): 0 auto (clips of 16384 blocks and more), 1 always, < 0 never; 2 = as 1 and then
                                    the sequential machine as if the segments had not converged (tests) */
    int64_t concurrent_calls;    /* how many detector calls of about this size the caller keeps in flight on the GPU
                                    at once (0 / 1: this call has the GPU to itself).  The layout of the
                                    speculative passes is chosen for the GPU's share: with k calls in flight each
                                    gets 1/k of the lane budget, i.e. the work-efficient layout of a k times larger
                                    batch instead of the latency layout of a lone call.  Results do not change. */
    int64_t scan_skip;           /* crossing pass: blocks whose extremes (left by the back-to-linear pass) show that they
                                    hold no value above `on` and whose last row is below `off` are decided without
                                    reading their samples: 0 on, < 0 off */
    int64_t host_verify;         /* who drives the verification passes of the three time-parallel stages.  0 (default):
                                    a bounded number of passes is enqueued ahead -- IIR rounds up to HP_MAX_ROUNDS (16),
                                    follower / tracker passes up to AHEAD_MAX_PASSES / 2 (12) -- sized by what the
                                    detector's recent calls needed; each pass is gated on the device by its
                                    predecessor's change counter and returns at once when there is nothing left to
                                    repair.  No host round trip, the call can be captured in a hipGraph.  If the last
                                    enqueued pass of a stage still changed something, the completion repeats the call
                                    (or its tail from the follower or tracker stage) in the host-verified form,
                                    reports it in info[15] and enqueues more passes in later calls.  1: the
                                    host-verified form throughout -- one launch per pass, the host reads the change
                                    counters group by group (verify_group, max_passes apply to this form only).
                                    2 / 3: aliases of 1 kept for old callers.  -2 / -3 / -4: test hooks that force the
                                    completion's repeat from the IIR / follower / tracker stage.  Results do not
                                    change. */
    int64_t interleaved;         /* 4, 8 or 64 channels, throughput layout (lane_merge), `rel` requested: tracker, crossing
                                    pass and backtracking read the caller's interleaved `rel` output, no planar copy of it
                                    is written (+7 % frames/s in flight).  0 (default) and 1: whenever those conditions
                                    hold; < 0 off; 2 (= -1) and 3 (= 1) are aliases kept for old callers.  Results do not
                                    change. */
    int64_t walk_through;        /* throughput layout: the chunks a speculative warm-up run walks through after its warm-up
                                    (all but the last of every group of `span` chunks) count as their pass 0 -- the run
                                    leaves their outputs and end states, the chunk pass runs the others only: one pass
                                    over the stream less for those chunks (followers: the merged layout with the
                                    closed-form guess; tracker: on the interleaved envelope).  0 on, < 0 off.  Results
                                    do not change. */
    int64_t line_stores;         /* throughput layout (lane_merge), everything a multiple of 32 steps: the output walks of
                                    the IIR stage and the followers hand every batch of 32 outputs over through LDS and
                                    the wave stores complete 128-byte lines (8 lanes x 16 B) instead of 64 lane-private
                                    16-byte pieces per instruction: +11 % frames/s in flight, +5 % for a lone BIG call
                                    (C3), slower for a small one.  0 auto (the throughput layout, or launches of more
                                    than two / half a wave per SIMD), 1 whenever the sizes allow, < 0 off.  Where the
                                    interleaved `rel` is what the later stages read (`interleaved`, 4 or 8 channels) and
                                    the warm-up and main parts are multiples of 32 rows, the followers' lines go
                                    straight into that array and the conversion back to linear runs in place there.
                                    Results do not change. */
} ofp_detect_tuning;

typedef struct ofp_detector ofp_detector; /* opaque */

/* on_threshold / off_threshold: C doubles each (the reference's scalar broadcast,
 * or per-channel values as set by AmplitudeOnsetDetector.init, detection.py:866-867) */
int ofp_detector_create(const ofp_detector_params* p, const double* on_threshold,
                        const double* off_threshold, ofp_detector** out);
int ofp_detector_destroy(ofp_detector* det);
int ofp_detector_set_tuning(ofp_detector* det, const ofp_detect_tuning* t);

/* Work space (bytes) ofp_detect_offline needs for n_clips clips of n_samples. */
int64_t ofp_detect_workspace_bytes(const ofp_detector* det, int64_t n_clips, int64_t n_samples,
                                   int64_t warm_samples);

/* The plan of a call: which of the detector's kernel variants a call of these sizes runs, and the geometry that decides
 * it.  Host arithmetic only: the queries launch nothing and allocate nothing on the device. */
typedef struct ofp_detect_plan {
    int64_t n_w;        /* warm samples through the high-pass: min(warm, n_samples), at least 0 */
    int64_t n_wb;       /* warm samples through followers and tracker: whole blocks of n_w */
    int64_t Nm;         /* floor(n_samples / B) * B: rows of `rel` */
    int64_t U;          /* follower stream length n_wb + Nm */
    int64_t V;          /* high-pass stream length n_w + Nm */
    int64_t Nv;         /* floats per series of the planar input copy: n_w + n_samples rounded up to 4 */
    int64_t hp_L;       /* IIR stage: samples per chunk */
    int64_t hp_S;       /* sub-chunks per chunk */
    int64_t hp_R;       /* speculative candidates per chunk */
    int64_t hp_span;    /* chunks one speculative run walks through */
    int64_t ar_L;       /* follower stage: samples per chunk */
    int64_t ar_S;       /* chunks one speculative warm-up run walks through */
    int64_t mm_L;       /* tracker stage: samples per chunk */
    int64_t mm_S;       /* chunks one speculative warm-up run walks through */
    int64_t tu;         /* time steps per tile of the entry and exit transposes */
    int32_t sm_seg;     /* hysteresis machine time-parallel over the visit list */
    int32_t merge;      /* followers / tracker: the two recurrences of a chunk in one lane */
    int32_t hp_early;   /* whole IIR re-runs stop early at a sub-chunk boundary */
    int32_t hp_staged;  /* IIR candidates in stages with duplicate runs removed between them */
    int32_t hp_spread;  /* the candidates launch has no more workgroups than the device has CUs */
    int32_t hp_lines;   /* IIR output walk stores complete 128-byte lines */
    int32_t ar_sym;     /* closed-form guess for a symmetric slow follower */
    int32_t ar_through; /* followers: walk-through chunks are their own pass 0 */
    int32_t ar_lines;   /* followers: output walks store complete 128-byte lines */
    int32_t db_sym;     /* the dB pass also forms the per-chunk sums of the closed-form guess */
    int32_t mm_il;      /* tracker, crossing pass and backtracking read the caller's interleaved `rel` */
    int32_t mm_through; /* tracker: walk-through chunks are their own pass 0 */
    int32_t ar_il;      /* followers write the caller's interleaved `rel` themselves; back to linear in place */
    int32_t use_sum;    /* the back-to-linear pass leaves block extremes for the crossing pass */
} ofp_detect_plan;
/* What ofp_detect_offline (and every other entry point) decides for a call of `det` with these sizes.  want_rel: the
 * call passes a d_rel; d_rel: its address (only its low four bits are used: the followers write `rel` themselves only
 * into a 16-byte-aligned array), or NULL to leave the alignment out. */
int ofp_detect_plan_query(const ofp_detector* det, int64_t n_clips, int64_t n_samples, int64_t warm, int want_rel,
                          const void* d_rel, ofp_detect_plan* out);
/* The same for a detector that is never created: its parameters, a tuning (NULL: defaults) and the device's CU count.
 * Makes no HIP call, so it also runs on a machine without a GPU. */
int ofp_detect_plan_for(const ofp_detector_params* p, const ofp_detect_tuning* t, int n_cus, int64_t n_clips,
                        int64_t n_samples, int64_t warm, int want_rel, const void* d_rel, ofp_detect_plan* out);

/* The arithmetic canon of include/ofp_math.h on the device, one value at a time (tests): d_out[i] = op(d_x[i], d_y[i]) for
 * i < n, each op calling the header's function and nothing else.  d_x, d_y, d_out: device arrays of n floats, any 4-byte
 * alignment; d_y may be NULL for the one-operand ops.  Parameters per op:
 *   LOG10(x), EXP10(x)                 none
 *   RECT_DB(x), REL_LINEAR(x)          p0 = floor_db
 *   AR_STEP(x, y)                      p0 = attack, p1 = release (the coefficients)
 *   MIN_STEP(x, y = mn)                p0 = alpha, p1 = minmin; ialpha = ofp_ialpha(alpha) is formed on the host, as
 *   MAX_STEP(x, y = mx)                p0 = alpha                ofp_detector_create forms it
 * p2 is not used by any op yet.  An unknown op, a negative n or a missing array is refused and nothing is launched;
 * n = 0 launches nothing. */
enum {
    OFP_CANON_LOG10 = 0,
    OFP_CANON_EXP10 = 1,
    OFP_CANON_RECT_DB = 2,
    OFP_CANON_REL_LINEAR = 3,
    OFP_CANON_AR_STEP = 4,
    OFP_CANON_MIN_STEP = 5,
    OFP_CANON_MAX_STEP = 6
};
int ofp_canon_eval(int32_t op, const float* d_x, const float* d_y, int64_t n, float p0, float p1, float p2, float* d_out,
                   void* stream);
/* RECT_DB and REL_LINEAR (no other op) with the canon's tables read from a copy in LDS that each workgroup fills: the form
 * the detector's elementwise passes run (csrc/ofp_canon_dev.h).  Same arrays and refusals as ofp_canon_eval. */
int ofp_canon_eval_lds(int32_t op, const float* d_x, int64_t n, float floor_db, float* d_out, void* stream);

/* detect_onsets_amplitude (detection.py:19-86) for a batch of independent clips.
 *   d_x        [n_clips][n_samples][C] float32, interleaved as the reference expects
 *   warm       number of leading samples double-processed by init_minmax_tracker
 *              (detection.py:70: int(0.5*sr)); clipped to n_samples; 0 = no warm-up
 *   d_rel      [n_clips][floor(n_samples/B)*B][C] float32 relative envelope, or NULL
 *   d_records  [n_clips][cap_per_clip] onset records, ordered as the reference orders
 *              them (block, then channel)
 *   d_counts   [n_clips] int64 number of onsets per clip (may exceed cap_per_clip:
 *              only cap_per_clip are stored)
 *   d_ws       work space of at least ofp_detect_workspace_bytes()
 * Synchronises `stream` ONCE, at its end (the speculative passes are enqueued ahead and gated on the
 * device; a stage they do not settle is repeated host-verified, see tuning host_verify); on return
 * all outputs are complete.  h_info (optional, host, int64
 * [OFP_DETECT_INFO_LEN]) receives {0: hp passes, 1: follower passes, 2: tracker
 * passes, 3: repaired chunks, 4..9: nanoseconds (HIP events on `stream`) spent in
 * the hp, dB, follower, linear, tracker and crossing/state-machine stages,
 * 10: total nanoseconds, 11: nanoseconds of the IIR candidate launch(es) (k_hp_candidates, the
 * longest single launch; or the stages k_hp_seg0 .. k_hp_seg_chunk), 12: IIR steps they execute
 * over all their lanes (17 fp32 operations each), 13: staged candidates only: distinct runs that
 * walked a chunk, of chains * chunks * candidates, 14: 1 if the segmented state machine did not converge within its
 * pre-enqueued passes and the sequential one decided, 15: non-zero if (a part of) the call was repeated with
 * host-verified passes because what had been enqueued ahead did not converge (1, + 1: the IIR rounds -- the whole call
 * again; + 2: the follower passes -- again from the follower stage; + 4: the tracker passes -- again from the tracker
 * stage; the detector then enqueues more passes in its next calls)}. */
#define OFP_DETECT_INFO_LEN 16
int ofp_detect_offline(ofp_detector* det, const float* d_x, int64_t n_clips, int64_t n_samples,
                       int64_t warm, float* d_rel, ofp_onset* d_records, int64_t cap_per_clip,
                       int64_t* d_counts, void* d_ws, int64_t ws_bytes, int64_t* h_info,
                       void* stream);

/* ofp_detect_offline without its synchronisation, in two calls.  _enqueue only ENQUEUES the whole call on `stream`
 * (nothing in it blocks or reads a device result on the host: the stream may be capturing a hipGraph, and a captured
 * graph may be replayed on new contents of the same buffers); after the caller has synchronised the stream (or the
 * graph launch), _complete with the same arguments reads the few words the call left in pinned host memory, fills
 * h_info (stage times only when the call was not captured) and, in the one case that needs a decision on the host --
 * the segmented state machine of a long clip did not converge within its pre-enqueued passes (info 14; never observed)
 * -- runs the sequential machine on `stream` and synchronises.  One enqueued call per detector at a time (it may be
 * completed once per replay of a graph that captured it).  Not with tuning host_verify > 0.  ofp_detect_offline == _enqueue + hipStreamSynchronize + _complete. */
int ofp_detect_offline_enqueue(ofp_detector* det, const float* d_x, int64_t n_clips, int64_t n_samples,
                               int64_t warm, float* d_rel, ofp_onset* d_records, int64_t cap_per_clip,
                               int64_t* d_counts, void* d_ws, int64_t ws_bytes, void* stream);
int ofp_detect_offline_complete(ofp_detector* det, const float* d_x, int64_t n_clips, int64_t n_samples,
                                int64_t warm, float* d_rel, ofp_onset* d_records, int64_t cap_per_clip,
                                int64_t* d_counts, void* d_ws, int64_t ws_bytes, int64_t* h_info, void* stream);

/* The same call in two halves, so that a caller can overlap other work with the long, sparsely
 * occupied tail: _begin only ENQUEUES the head (input transpose + the IIR candidate launch, the
 * part that is heavy on the memory system) and returns; _finish does everything else and
 * synchronises.  Both take the arguments of ofp_detect_offline. */
int ofp_detect_offline_begin(ofp_detector* det, const float* d_x, int64_t n_clips, int64_t n_samples,
                             int64_t warm, void* d_ws, int64_t ws_bytes, void* stream);
int ofp_detect_offline_finish(ofp_detector* det, const float* d_x, int64_t n_clips, int64_t n_samples,
                              int64_t warm, float* d_rel, ofp_onset* d_records, int64_t cap_per_clip,
                              int64_t* d_counts, void* d_ws, int64_t ws_bytes, int64_t* h_info, void* stream);

/* _finish without its synchronisation (complete it with ofp_detect_offline_complete after synchronising). */
int ofp_detect_offline_finish_enqueue(ofp_detector* det, const float* d_x, int64_t n_clips, int64_t n_samples,
                                      int64_t warm, float* d_rel, ofp_onset* d_records, int64_t cap_per_clip,
                                      int64_t* d_counts, void* d_ws, int64_t ws_bytes, void* stream);

/* _begin in two calls: _begin_input enqueues the planar copy of the input only (ofp_detect_planar_input
 * is valid once it has run), _begin_iir the IIR candidate launch. */
int ofp_detect_offline_begin_input(ofp_detector* det, const float* d_x, int64_t n_clips, int64_t n_samples,
                                   int64_t warm, void* d_ws, int64_t ws_bytes, void* stream);
int ofp_detect_offline_begin_iir(ofp_detector* det, const float* d_x, int64_t n_clips, int64_t n_samples,
                                 int64_t warm, void* d_ws, int64_t ws_bytes, void* stream);
/* Collation block of a rank (the all-gather of onset indices): the onset records of a batch of
 * clips, d_records [n_clips][cap_per_clip] with d_counts [n_clips] as ofp_detect_offline leaves them, compacted
 * in clip order into d_block [1 + cap_total] without a host round trip (no data-dependent shape).  Record 0 is
 * the header {clip: 0, channel: 1 if some clip counted more onsets than cap_per_clip (lost records), sample:
 * total number of records}; records 1.. follow with clip_offset added to their clip ids; records that do not
 * fit cap_total are dropped (the header still carries the true total, so the reader can tell); rows beyond
 * the total are not written.  One launch. */
int ofp_pack_records(const ofp_onset* d_records, const int64_t* d_counts, int64_t n_clips, int64_t cap_per_clip,
                     int64_t cap_total, int32_t clip_offset, ofp_onset* d_block, void* stream);

/* Streaming form: AmplitudeOnsetDetector.__call__ (detection.py:727-798) on
 * n_blocks consecutive blocks with the detector state carried in d_state
 * (ofp_stream_state_bytes() bytes, initialised by ofp_stream_state_init).
 * One launch, no host synchronisation: capturable into a hipGraph.
 *   d_x [n_blocks*B][C]; d_rel same shape or NULL; d_records [cap]; d_count [1]
 *   (int64, ACCUMULATED: zero it to start a new list); record.sample is relative to
 *   sample_base + the first sample of this call.
 *   warmup != 0: run init_minmax_tracker (detection.py:827-840) over the n_rows
 *   rows of d_x instead (n_blocks is then ignored; rows beyond the last full block
 *   pass through the high-pass filter only). */
int64_t ofp_stream_state_bytes(const ofp_detector* det);
int ofp_stream_state_init(ofp_detector* det, void* d_state, void* stream);
int ofp_stream_process(ofp_detector* det, void* d_state, const float* d_x, int64_t n_blocks,
                       int64_t n_rows, int32_t warmup, int64_t sample_base, float* d_rel,
                       ofp_onset* d_records, int64_t cap, int64_t* d_count, void* stream);

/* AmplitudeOnsetDetector.init (detection.py:842-888), the passes over the samples, with the state in
 * d_state: high-pass over the n_rows rows of d_x (:849-850), unclipped rectified dB (:852), the
 * followers over rows [r0, r1) (the settling blocks, :855-860), over all rows with
 * d_rel[n_rows][C] = fast - slow in dB (:862-867), and over rows n_rev-1 .. 0 (:883-888).
 * d_scratch [n_rows][C].  Tracker and hysteresis state are untouched.  The thresholds init derives
 * from statistics of d_rel (:869-872) are installed with ofp_detector_set_thresholds.  Only enqueues. */
int ofp_stream_calibrate(ofp_detector* det, void* d_state, const float* d_x, int64_t n_rows, int64_t r0,
                         int64_t r1, int64_t n_rev, float* d_scratch, float* d_rel, void* stream);
/* Replaces the per-channel thresholds given to ofp_detector_create (host arrays of C doubles);
 * synchronous.  Applies to launches enqueued afterwards. */
int ofp_detector_set_thresholds(ofp_detector* det, const double* on_threshold, const double* off_threshold);

/* ---- framing + STFT (data.py:55-120, 581-654) ------------------------------------ */
/* Dense power spectra, the metric's frame definition (one frame per hop):
 *   d_x [n_clips][n_samples][C] interleaved;  frame h of channel c covers samples
 *   [h*hop, h*hop + n_fft);  H = 1 + (n_samples - n_fft)/hop.
 *   d_power [n_clips][C][H][n_fft/2+1] float32 = |rfft(hann_periodic(n_fft) * frame)|^2
 *   n_fft in {256, 512, 1024, 2048, 4096}.  d_power may be NULL when only the mel
 *   output below is wanted. */
int ofp_stft_power(const float* d_x, int64_t n_clips, int64_t n_samples, int32_t n_channels,
                   int32_t n_fft, int32_t hop, float* d_power, void* stream);
/* The same with the mel filterbank of ofp_mel applied while a frame's power spectrum is still on
 * chip: d_mel [n_clips][C][H][n_mels] (same values as ofp_mel on d_power); d_power may be NULL
 * when only the mel fingerprint is wanted.  fb_nnz = number of weights in d_fb_w. */
int ofp_stft_power_mel(const float* d_x, int64_t n_clips, int64_t n_samples, int32_t n_channels, int32_t n_fft,
                       int32_t hop, float* d_power, int32_t n_mels, const int32_t* d_fb_lo,
                       const int32_t* d_fb_len, const int32_t* d_fb_off, const float* d_fb_w, int32_t fb_nnz,
                       float* d_mel, int64_t planar_stride, void* stream);
/* ... and the classifier on top (the fingerprint path of SURVEY.md 8a rows a9 -> a11 -> a13 in one
 * launch): the 40 band sums of 16 frames at a time go through the whole FCNN while they are still in
 * LDS.  d_logits [n_clips][C][H][mlp outputs]; d_power and d_mel may each be NULL (nothing but the
 * logits then leaves the chip: 32 B per frame instead of 2 052 + 160).  mlp inputs == n_mels. */
typedef struct ofp_mlp ofp_mlp;
int ofp_stft_power_mel_mlp(const float* d_x, int64_t n_clips, int64_t n_samples, int32_t n_channels, int32_t n_fft,
                           int32_t hop, float* d_power, int32_t n_mels, const int32_t* d_fb_lo,
                           const int32_t* d_fb_len, const int32_t* d_fb_off, const float* d_fb_w, int32_t fb_nnz,
                           float* d_mel, int64_t planar_stride, const ofp_mlp* mlp, float* d_logits, void* stream);
/* planar_stride != 0: d_x points at one series per (clip, channel), planar_stride floats apart, e.g.
 * the planar copy the detector keeps in its work space between ofp_detect_offline_begin and the next
 * begin (each series there is preceded by the warm-up part of the detector's stream): */
const float* ofp_detect_planar_input(const ofp_detector* det, int64_t n_clips, int64_t n_samples, int64_t warm,
                                     const void* d_ws);
int64_t ofp_detect_planar_stride(const ofp_detector* det, int64_t n_clips, int64_t n_samples, int64_t warm);

/* Gathered complex STFT frames (data.py:593-654 semantics are built on this by
 * the Python layer): for each of n_frames (clip, channel, start) triples,
 * d_spec[f][n_fft/2+1] complex64 = rfft(window * pad_center(x[start : start+frame_length]))
 * with samples outside [0, n_samples) read as zero.  d_window is float32[n_fft]
 * (the zero-padded periodic Hann, data.py:627-629).  starts may be negative.
 * n_channels < 1 or a frame_length outside [1, n_fft] is OFP_ERR_INVALID (nothing is launched). */
int ofp_stft_frames(const float* d_x, int64_t n_clips, int64_t n_samples, int32_t n_channels,
                    const int32_t* d_clip, const int32_t* d_channel, const int64_t* d_start,
                    const int64_t* d_valid_lo, const int64_t* d_valid_hi, int64_t n_frames,
                    int32_t frame_length, int32_t n_fft, const float* d_window, float* d_spec,
                    void* stream);

/* FrameExtractor gather (data.py:90-120): d_out[o][c][w] = x[clip][start[o][c] + w][c] */
int ofp_extract_frames(const float* d_x, int64_t n_samples, int32_t n_channels,
                       const int64_t* d_start /* [O][C] */, int64_t n_onsets, int32_t width,
                       float* d_out, void* stream);

/* ---- fingerprint: mel + dB + DCT (data.py:657-680) ------------------------------- */
/* d_power [n_rows][n_bins] -> d_mel [n_rows][n_mels] = power @ fb^T with the sparse
 * triangular filterbank given in CSR-by-band form (band b covers bins
 * [d_fb_lo[b], d_fb_lo[b]+d_fb_len[b]) with weights d_fb_w[d_fb_off[b] ...]).
 * n_mels outside [1, 127] or n_bins < 1 is OFP_ERR_INVALID (nothing is launched). */
int ofp_mel(const float* d_power, int64_t n_rows, int32_t n_bins, int32_t n_mels,
            const int32_t* d_fb_lo, const int32_t* d_fb_len, const int32_t* d_fb_off,
            const float* d_fb_w, float* d_mel, void* stream);
/* power_to_db (ref 1, amin, top_db relative to the max over the n values) then
 * DCT-II ortho over the mel axis keeping n_mfcc: d_mel [n_rows][n_mels] ->
 * d_mfcc [n_rows][n_mfcc].  d_dct is float32 [n_mfcc][n_mels].  top_db < 0: no floor.
 * d_scratch: >= 4 bytes.  n_mels < 1 or n_mfcc < 1 is OFP_ERR_INVALID (nothing is launched). */
int ofp_mfcc(const float* d_mel, int64_t n_rows, int32_t n_mels, int32_t n_mfcc, float amin,
             float top_db, const float* d_dct, float* d_mfcc, float* d_scratch, void* stream);

/* ---- classifier forward ---------------------------------------------------------- */
#define OFP_ACT_IDENTITY 0
#define OFP_ACT_RELU 1
#define OFP_ACT_SILU 2
#define OFP_ACT_LEAKYRELU 3
#define OFP_ACT_ELU 4
#define OFP_ACT_TANH 5
/* One fused dense layer: d_y[n][out] = act((d_x[n][in] @ W^T + b) * scale + shift)
 * (W [out][in] row-major as torch stores Linear.weight; scale/shift fold an eval-mode
 * BatchNorm1d, NULL = identity; b NULL = no bias).  fp32 MFMA (v_mfma_f32_16x16x4_f32). */
int ofp_dense(const float* d_x, int64_t n, int32_t in, int32_t out, const float* d_w,
              const float* d_b, const float* d_scale, const float* d_shift, int32_t act,
              float* d_y, void* stream);
/* The whole FCNN (calibration.py:463-527, eval mode) as one handle and ONE launch: n_layers fused
 * dense layers (1..8) with the activations kept in LDS; per output element the arithmetic is that of
 * the ofp_dense chain, so results are bit-identical to it.  All arrays are HOST pointers and are copied:
 * dims [n_layers+1] (dims[0] inputs ... dims[n_layers] outputs), act [n_layers] (OFP_ACT_*), and per
 * layer h_w[L] [dims[L+1]][dims[L]] (torch Linear.weight), h_b[L] / h_scale[L] / h_shift[L]
 * [dims[L+1]] or NULL (h_b, h_scale, h_shift themselves may be NULL).  ofp_mlp_forward: d_x [n][dims[0]]
 * -> d_y [n][dims[n_layers]]; fails with OFP_ERR_INVALID when ofp_mlp_lds_bytes() exceeds the 160 KiB of
 * LDS (run such a network layer by layer with ofp_dense). */
typedef struct ofp_mlp ofp_mlp; /* opaque */
int ofp_mlp_create(int32_t n_layers, const int32_t* dims, const int32_t* act, const float* const* h_w,
                   const float* const* h_b, const float* const* h_scale, const float* const* h_shift,
                   ofp_mlp** out);
int ofp_mlp_destroy(ofp_mlp* mlp);
int64_t ofp_mlp_lds_bytes(const ofp_mlp* mlp);
int ofp_mlp_forward(const ofp_mlp* mlp, const float* d_x, int64_t n, float* d_y, void* stream);

/* Conv1d (any stride, any groups that divide cin and cout) + bias + activation, then the optional
 * per-channel affine of an eval-mode BatchNorm1d, then optionally MaxPool1d(2, 2) (model.py:84-107):
 * d_x [n][cin][w] -> d_y [n][cout][wout] with
 *   wconv = (w + 2*padding - dilation*(k-1) - 1) / stride + 1   (integer division)
 *   wout  = pool ? wconv / 2 : wconv                            (floor: an odd last column is dropped)
 * OFP_ERR_INVALID: cin, cout, w or k < 1, dilation < 1, padding < 0, stride < 1, groups that do not divide
 * cin and cout, only one of d_bn_scale / d_bn_shift, an unknown activation, wout < 1. */
int ofp_conv1d(const float* d_x, int64_t n, int32_t cin, int32_t w, const float* d_w /*[cout][cin/groups][k]*/,
               const float* d_b, int32_t cout, int32_t k, int32_t padding, int32_t dilation, int32_t groups,
               int32_t stride, int32_t act, const float* d_bn_scale /*[cout] or NULL*/, const float* d_bn_shift,
               int32_t pool /* MaxPool1d(2, 2) after the affine */, float* d_y, void* stream);
/* nn.GroupNorm(1, K) over items d_x [n][K][V] (CCCNN with batch_norm=True, model.py:497-501), then
 * optionally MaxPool1d(2, 2): d_y [n][K][V or V/2]; d_gamma / d_beta [K] or NULL.  Not in place. */
int ofp_groupnorm1(const float* d_x, int64_t n, int32_t K, int32_t V, const float* d_gamma, const float* d_beta,
                   float eps, int32_t pool, float* d_y, void* stream);

/* CCCNN correlation head (model.py:524-534): d_x [n][K][V] feature maps -> d_out [n][2V-1]:
 * full auto-correlation of every map, summed over the K maps, soft-maxed over the lags. */
int ofp_autocorr_softmax(const float* d_x, int64_t n, int32_t K, int32_t V, float* d_out, void* stream);

/* ---- recurrent classifiers: model.RNN / model.CNNRNN (model.py:168-440), eval mode ----------------
 * Cell codes of ofp_rnn_layer: torch's gate order and equations, zero initial state.
 *   RNN:  h' = act(W_ih x + b_ih + W_hh h + b_hh)                        (nn.RNN, tanh or relu)
 *   GRU:  r, z, n;  n = tanh(W_in x + b_in + r * (W_hn h + b_hn)),  h' = (1 - z) n + z h   (nn.GRU)
 *   LSTM: i, f, g, o;  c' = f c + i g,  h' = o tanh(c')                   (nn.LSTM, no projection) */
#define OFP_CELL_RNN_TANH 0
#define OFP_CELL_RNN_RELU 1
#define OFP_CELL_GRU 2
#define OFP_CELL_LSTM 3
/* One layer and direction of an nn.RNN / nn.GRU / nn.LSTM over n_seq sequences of T steps, one launch.
 * With G gates per cell (1, 3, 4) and H <= 256 hidden units:
 *   input, one of:
 *     d_gx != NULL: the input projection x W_ihᵀ + b_ih, already computed (e.g. by ofp_dense), element
 *       (s, t, g*H + j) at d_gx[s*gx_seq + t*gx_t + g*H + j]; d_x, d_w_ih, d_b_ih are then ignored;
 *     d_gx == NULL: element (s, t, f) of the input at d_x[s*x_seq + t*x_t + f*x_f] (any strides, so a
 *       channel slice or a permuted view is read in place), in <= 8 features, d_w_ih [G*H][in],
 *       d_b_ih [G*H] or NULL;
 *   d_w_hh [G*H][H], d_b_hh [G*H] or NULL (torch's weight_hh_l{k}, bias_hh_l{k});
 *   reverse != 0: the backward direction (t = T-1 .. 0);
 *   output: h_t of sequence s, unit j at d_y[s*y_seq + t*y_t + y_off + j] (so the two directions, or
 *     several runs, fill their slots of one [.., T, F] tensor without a copy).
 * Every output element depends only on its own sequence.  W_hh is kept in LDS when
 * ofp_rnn_lds_bytes(cell, H) <= 160 KiB and streamed from L2 otherwise.  OFP_ERR_INVALID: unknown cell,
 * T < 1, H outside 1..256, in > 8 without d_gx, NULL d_w_hh / d_y. */
int ofp_rnn_layer(int32_t cell, int64_t n_seq, int32_t T, int32_t in, int32_t H, int32_t reverse, const float* d_x,
                  int64_t x_seq, int64_t x_t, int64_t x_f, const float* d_gx, int64_t gx_seq, int64_t gx_t,
                  const float* d_w_ih, const float* d_b_ih, const float* d_w_hh, const float* d_b_hh, float* d_y,
                  int64_t y_seq, int64_t y_t, int32_t y_off, void* stream);
/* LDS a workgroup of ofp_rnn_layer needs to keep W_hh resident; -1 for an invalid cell or H */
int64_t ofp_rnn_lds_bytes(int32_t cell, int32_t H);
/* nn.LayerNorm(E) over rows: d_x [n][E] -> d_y [n][E] (may alias d_x); d_gamma / d_beta [E] or NULL. */
int ofp_layernorm(const float* d_x, int64_t n, int32_t E, const float* d_gamma, const float* d_beta, float eps,
                  float* d_y, void* stream);
/* nn.MultiheadAttention self-attention (eval, need_weights=False) before out_proj, averaged over time:
 * d_qkv [n_seq][T][3E] is the in-projection (q | k | v column blocks, head h in columns h*d .. h*d+d-1 of
 * each, d = E / n_heads); d_out [n_seq][E] = mean_t of softmax(Q Kᵀ / sqrt(d)) V per head.  out_proj and
 * a following Linear commute with the mean and are applied to d_out (ofp_dense).  Keys are streamed with
 * an online softmax, so T is unbounded.  OFP_ERR_INVALID: T < 1, E not divisible by n_heads, d > 128. */
int ofp_attention_mean(const float* d_qkv, int64_t n_seq, int32_t T, int32_t E, int32_t n_heads, float* d_out,
                       void* stream);

/* ---- per-hop streaming session (BASELINE config 5) -------------------------------------------
 * The reference's realtime pattern -- PortAudio callback: ring-buffer write (realtime/audio.py:97),
 * AmplitudeOnsetDetector on the hop (:62-74), classifier (multilateration.py:555-557 ->
 * calibration.py:552-560), one spectral frame of the trailing n_fft samples per hop
 * (realtime/recording.py:273-280) -- as ONE hipGraph per hop, captured at creation:
 *   H2D hop -> detector (state in HBM) -> per channel: ring write, Hann x audio[-n_fft:], rFFT,
 *   |X|^2, mel bands, FCNN -> D2H of {count, records, logits, mel, rel}.
 * The ring buffer ([ring_samples][C] float32, zeros at start: realtime/config.py:45,59) and all
 * detector state stay on the device.  The detector handle is borrowed and must outlive the session;
 * hop length and channel count are the detector's block_size and n_channels.  All h_ pointers are
 * HOST memory.  One hop may be in flight per session (submit -> collect; push = both). */
typedef struct ofp_hop_config {
    int32_t n_fft;          /* 256, 512, 1024, 2048 or 4096; periodic Hann of n_fft (data.py:627) */
    int64_t ring_samples;   /* rows of the ring buffer, >= max(n_fft, block_size) */
    int32_t n_mels;         /* mel filterbank, band-CSR as for ofp_mel; HOST arrays, copied */
    const int32_t* fb_lo;
    const int32_t* fb_len;
    const int32_t* fb_off;
    const float* fb_w;
    int32_t fb_nnz;
    const ofp_mlp* mlp;     /* classifier on the n_mels bands, or NULL; parameters are copied */
    int32_t want_rel;       /* != 0: the hop's relative envelope [B][C] is copied back too */
    /* Per-hop onset strength of the channel mean (realtime/recording.py:273-311, RecAnalysis.fft +
     * onset_strength): symmetric float32 Hann x audio[-n_fft:].mean(-1), rFFT, dB floored 80 dB below a tracked
     * maximum, positive flux against the previous frame averaged over the bins, normalised by a tracked
     * min / max, moving max / mean over the last max_length / avg_length entries (the reference reads these
     * two from config.MAX_LENGTH / AVG_LENGTH, which its config.py does not define).  The trackers are
     * loopmate.EMA_MinMaxTracker objects (:251-256); loopmate is absent, their update is ASSUMED to be
     * envelope_follower.c:27-57 with a single alpha: PARITY UNPINNED. */
    int32_t strength;       /* != 0: enabled */
    int32_t strength_ring;  /* entries of the onset-envelope ring (the reference's n_stft) */
    int32_t max_length, avg_length;
    float ls_max0, ls_minmax, ls_alpha;            /* EMA_MinMaxTracker(max0=10, minmax=0, alpha=0.0005) */
    float oe_min0, oe_minmin, oe_max0, oe_alpha;   /* EMA_MinMaxTracker(min0=0, minmin=0, max0=1, alpha=0.001) */
    int32_t tg_win_length;  /* > 0: the tempogram frame of the hop as well (realtime/recording.py:313-327, config.py:55:
                               TG_WIN_LENGTH): autocorrelation of the Hann-windowed last tg_win_length entries of the
                               normalised onset envelope, lags 0 .. tg_win_length - 1, divided by (its maximum + 1e-10);
                               needs strength, tg_win_length <= strength_ring.  PARITY UNPINNED like the envelope. */
} ofp_hop_config;
typedef struct ofp_hop_session ofp_hop_session; /* opaque */
int ofp_hop_create(ofp_detector* det, const ofp_hop_config* cfg, ofp_hop_session** out);
/* (OFP_ERR_INVALID while the session is a member of an ofp_hop_group, as for submit / push / set_locator) */
int ofp_hop_destroy(ofp_hop_session* s);
/* back to the state after creation (zero ring, fresh detector state, hop counter 0) */
int ofp_hop_reset(ofp_hop_session* s);
/* AmplitudeOnsetDetector.init_minmax_tracker (detection.py:827-840) over h_x [n_rows][C] */
int ofp_hop_warmup(ofp_hop_session* s, const float* h_x, int64_t n_rows);
/* One hop, h_hop [B][C].  Outputs (each may be NULL): *n_onsets; h_records [C] with .sample =
 * hop_index * B + delta (audio.py:65) and .clip = 0, in channel order; h_logits [C][mlp outputs];
 * h_mel [C][n_mels]; h_rel [B][C] (needs want_rel); h_strength [4 + tg_win_length] = {flux, normalised, moving max,
 * moving mean, then the tempogram frame} (needs strength). */
int ofp_hop_submit(ofp_hop_session* s, const float* h_hop);
int ofp_hop_collect(ofp_hop_session* s, int64_t* n_onsets, ofp_onset* h_records, float* h_logits, float* h_mel,
                    float* h_rel, float* h_strength);
int ofp_hop_push(ofp_hop_session* s, const float* h_hop, int64_t* n_onsets, ofp_onset* h_records, float* h_logits,
                 float* h_mel, float* h_rel, float* h_strength);
/* audio[-n_rows:] of the ring buffer (oldest row first), h_out [n_rows][C]; n_rows <= ring_samples */
int ofp_hop_ring_read(ofp_hop_session* s, int64_t n_rows, float* h_out);

/* ---- S sessions per hop period in ONE launch ---------------------------------------------------
 * A group binds n sessions (several drums, players or streams with the same hop clock) to one captured graph whose
 * single kernel node has a second grid dimension: row i runs member i's hop exactly as the member's own graph
 * would -- same device code, same state, nothing shared or summed across members -- so every output is bit for bit
 * what the stand-alone session gives.  The group owns a stream, device copies of the members' kernel arguments and
 * the graph; the members keep their state, ring, pinned hop / result blocks and hop counters, and may join warmed
 * up or mid-stream.
 *   ofp_hop_group_create   OFP_ERR_INVALID (nothing is launched): n outside 1..1024, a NULL member, a member listed
 *       twice, already in a group, with a hop in flight, or not in the fused one-kernel form (OFP_HOP_GRAPH=nodes, or
 *       a shape too wide for it); members on different devices; members that differ in n_fft, in the channel count,
 *       in whether the onset strength is enabled or in whether a locator is attached (these four fix the kernel and
 *       its grid).  Block size, sample rate, detector arguments, ring length, want_rel, filterbank, classifier and
 *       the locator's geometry and model may differ per member.
 *   ofp_hop_group_submit   h_hops[i] is member i's hop, HOST memory [B_i][C]; one graph launch for all members.  No
 *       member may have an uncollected hop.
 *   ofp_hop_group_wait     returns once every member's results are published.  Then read each member with
 *       ofp_hop_collect (required before the next submit; it no longer waits) and ofp_hop_collect_location /
 *       ofp_hop_locator_state / ofp_hop_ring_read as for a stand-alone session.
 *   ofp_hop_group_destroy  waits for the last launch and releases the members, which work stand-alone again (an
 *       uncollected hop can still be collected); the sessions themselves are not destroyed.
 * While a session is a member: ofp_hop_reset and ofp_hop_warmup still work (they first wait for the group's last
 * launch); ofp_hop_submit, ofp_hop_push, ofp_hop_set_locator and ofp_hop_destroy return OFP_ERR_INVALID -- destroy the
 * group first.  A group must be destroyed before any of its members or their detectors. */
typedef struct ofp_hop_group ofp_hop_group; /* opaque */
int ofp_hop_group_create(ofp_hop_session* const* sessions, int n, ofp_hop_group** out);
int ofp_hop_group_destroy(ofp_hop_group* g);
int ofp_hop_group_submit(ofp_hop_group* g, const float* const* h_hops);
int ofp_hop_group_wait(ofp_hop_group* g);

/* ---- onset groups and their windows --------------------------------
 * find_onset_groups (detection.py:131-189) per clip, straight from the records
 * ofp_detect_offline wrote, without a host round trip.
 *   d_records [n_clips][cap_per_clip], d_counts [n_clips]   as ofp_detect_offline leaves them
 *   n_channels      row width (the reference uses max(channels)+1, detection.py:158,170);
 *                   every record's channel must be in [0, n_channels)
 *   max_distance, min_channels   detection.py:134-135
 *   close_channel   detection.py:136,185; < 0 for None
 *   d_groups  [n_clips][cap_groups][n_channels] int64 rows, -1 where a channel has no onset,
 *             in the reference's order; d_n_groups [n_clips] kept groups per clip (may exceed
 *             cap_groups: only cap_groups rows are stored)
 *   d_ws      ofp_group_workspace_bytes(n_clips, cap_per_clip) bytes */
int64_t ofp_group_workspace_bytes(int64_t n_clips, int64_t cap_per_clip);
int ofp_group_onsets(const ofp_onset* d_records, int64_t cap_per_clip, const int64_t* d_counts, int64_t n_clips,
                     int32_t n_channels, int64_t max_distance, int32_t min_channels, int32_t close_channel,
                     int64_t* d_groups, int64_t cap_groups, int64_t* d_n_groups, void* d_ws, int64_t ws_bytes,
                     void* stream);
/* FrameExtractor.__call__ (data.py:90-120, max_shift = 0) over those rows: window c of a
 * group starts at min_c(row) - pre_samples (use_min_onset != 0) or row[c] - pre_samples.
 *   d_x [n_clips][n_samples][n_channels] interleaved
 *   d_offsets [n_clips + 1] (out): first output row of each clip; [n_clips] = total rows
 *   d_out [cap_total][n_channels][width]: rows of all clips back to back (rows beyond
 *   cap_total are dropped).  Samples outside the clip read as 0. */
int ofp_group_windows(const float* d_x, int64_t n_clips, int64_t n_samples, int32_t n_channels,
                      const int64_t* d_groups, int64_t cap_groups, const int64_t* d_n_groups, int32_t pre_samples,
                      int32_t use_min_onset, int32_t width, float* d_out, int64_t cap_total, int64_t* d_offsets,
                      void* stream);

/* ---- cross-correlation lag and onset fixing --------------------------
 * cross_correlation_lag (detection.py:195-268) for a batch of pairs.
 *   d_x, d_y [n_pairs][n_in] float32; d: difference order applied first (np.diff, :238-239);
 *   take_abs (:240-242); cutoff = normalization_cutoff (:247-250).  With n = n_in - d,
 *   d_lo/d_hi [n_pairs] give the slice [lo, hi) of the normalised full correlation (length
 *   2n-1) that is searched, i.e. what Python's slicing at :257 / :263 selects.
 *   d_argmax [n_pairs]: np.argmax over the slice (first maximum), -1 for an empty slice; the
 *   lag is max_adjust - argmax (:268).  d_cc (optional) [n_pairs][cc_stride]: the slice values.
 * Dot products are accumulated in fp64 and rounded once to fp32 (see csrc/ofp_xcorr.hip).
 * n_in <= 4096, d <= 4. */
int ofp_xcorr_lag(const float* d_x, const float* d_y, int64_t n_pairs, int32_t n_in, int32_t d, int32_t take_abs,
                  int32_t cutoff, const int32_t* d_lo, const int32_t* d_hi, int32_t* d_argmax, float* d_cc,
                  int32_t cc_stride, void* stream);
/* adjust_onset (detection.py:299-352) for a batch of pairs, one wave each: d_x, d_y [n_pairs][n] float32,
 * d_onsets [n_pairs][2] (onset in x, onset in y), d_new_lag [n_pairs] -> d_moves [n_pairs][2], the amounts
 * the reference returns to be added to the two onsets.  Weighted sums in fp64 as in ofp_fix_onsets. */
int ofp_adjust_onset(const float* d_x, const float* d_y, int64_t n_pairs, int32_t n, const int32_t* d_onsets,
                     const int32_t* d_new_lag, int32_t* d_moves, void* stream);
/* filter_data (detection.py:355-370): d_y[t][c] = d_x[t][c], or 0 where the first difference along time is
 * negative (direction 1, "up") / positive (direction 2, "down"); row 0 is kept.  Not in place. */
int ofp_filter_direction(const float* d_x, int64_t n, int32_t n_channels, int32_t direction, float* d_y, void* stream);
/* detect_onset_region (detection.py:454-484) for n_onsets onsets of one 1-D signal d_audio [n_audio]:
 * region = audio[onset - n/2 : onset + n/2] (clipped), |.|, scipy medfilt (zero-padded, odd size <= 33),
 * threshold_factor * max, binary_opening with ones(5), first True -> d_out [n_onsets] absolute indices.
 * n/2*2 <= 4096. */
int ofp_onset_region(const float* d_audio, int64_t n_audio, const int64_t* d_onsets, int64_t n_onsets, int32_t n,
                     int32_t median_filter_size, float threshold_factor, int64_t* d_out, void* stream);
/* StretchFrameExtractor's resampling (data.py:212-222): scipy.signal.resample (Fourier method, real input) of
 * the windows audio[d_start[i] : d_start[i] + d_nx[i], c] to `num` samples each: d_out [n_items][C][num].
 * d_audio [n_samples][C]; samples outside the clip read as 0; d_nx[i] <= max_nx <= 2048, num <= 2048. */
int ofp_resample_windows(const float* d_audio, int64_t n_samples, int32_t n_channels, const int64_t* d_start,
                         const int32_t* d_nx, int64_t n_items, int32_t max_nx, int32_t num, float* d_out, void* stream);
/* Full cross-correlation of row pairs (batch_cc, data.py:226-230; paired_xcorr, model.py:12-45):
 * d_out[i][j] = sum_t a[i][t + j - (L-1)] b[i][t], j in [0, 2L-1); rows i of d_a / d_b start at
 * i*a_stride / i*b_stride floats.  mean_k > 1: output row i is the mean of input rows
 * [i*mean_k, (i+1)*mean_k) (paired_xcorr's mean over feature maps).  length <= 4096. */
int ofp_xcorr_full(const float* d_a, const float* d_b, int64_t n_rows, int32_t length, int64_t a_stride,
                   int64_t b_stride, int32_t mean_k, float* d_out, void* stream);
/* fix_onsets (detection.py:373-451) for every onset group, one workgroup per group:
 * median filter (scipy.ndimage 'reflect') over audio[a-look : b+look], d-th difference,
 * rectification by direction (0 none, 1 "up", 2 "down"), abs, then for every channel after the
 * earliest one cross_correlation_lag + adjust_onset (:299-352), in the reference's order.
 *   d_audio [n_clips][n_samples][n_channels]; d_onsets [n_clips][cap_groups][n_channels] int64
 *   (the layout ofp_group_onsets writes), updated in place (shift is added first, :414);
 *   d_n_groups [n_clips] rows in use per clip (clamped to cap_groups) or NULL for all rows;
 *   max_section: longest b - a + 2*(cutoff + tol) the work space holds (<= 4096);
 *   d_status [n_clips][cap_groups]: 0 fixed, 1 = group outside the clip, with a missing
 *   channel (-1) or longer than max_section (only shifted), 2 = row not in use.
 *   d_ws: ofp_fix_onsets_workspace_bytes(n_clips * cap_groups, ...) bytes. */
int64_t ofp_fix_onsets_workspace_bytes(int64_t n_groups, int32_t n_channels, int32_t max_section);
int ofp_fix_onsets(const float* d_audio, int64_t n_clips, int64_t n_samples, int32_t n_channels, int64_t* d_onsets,
                   int64_t cap_groups, const int64_t* d_n_groups, int32_t filter_size, int32_t d, int32_t direction, int32_t take_abs, int32_t zero_left,
                   int32_t cutoff, int32_t tol, int32_t shift, int32_t max_section, int32_t* d_status, void* d_ws,
                   int64_t ws_bytes, void* stream);

/* ---- spectral-flux onset detector (detection.py:89-128) --------------
 * The STFT is ofp_stft_power on the centre-padded signal (librosa.stft, center=True).
 *   ofp_spectral_flux: d_power [n_frames][n_bins] -> d_oe [n_frames-1] =
 *     mean_k max(0, w_k sqrt(P[t+1][k]) - w_k sqrt(P[t][k]))   (detection.py:106-110; d_weight is
 *     the normalised A-weighting of :105-106)
 *   ofp_select_rank: the value of ascending rank `rank` among n non-negative floats (the order
 *     statistics np.percentile interpolates, :111); d_out [1]
 *   ofp_scale_inverse: d_x[i] /= d_scale[0]
 *   ofp_peak_pick: librosa.util.peak_pick (:113-121): i is a peak iff x[i] == max(x[i-pre_max :
 *     i+post_max]), x[i] >= mean(x[i-pre_avg : i+post_avg]) + delta and i - previous peak > wait;
 *     d_peaks [cap] int64 indices, d_count [1] (may exceed cap), d_flags [n] scratch.
 * librosa is not available to pin these against: restated from its published definition. */
int ofp_spectral_flux(const float* d_power, int64_t n_frames, int32_t n_bins, const float* d_weight, float* d_oe,
                      void* stream);
int ofp_select_rank(const float* d_v, int64_t n, int64_t rank, float* d_out, void* stream);
int ofp_scale_inverse(float* d_x, int64_t n, const float* d_scale, void* stream);
int ofp_peak_pick(const float* d_x, int64_t n, int32_t pre_max, int32_t post_max, int32_t pre_avg, int32_t post_avg,
                  float delta, int64_t wait, int64_t* d_peaks, int64_t cap, int64_t* d_count, uint8_t* d_flags,
                  void* stream);

/* ---- hit location: lag maps, legality search, TDoA trilateration (multilateration.py) ------------
 * All geometry is fp64 (numpy's float64), positions in cm.  Grid of a lag map: side = 2r+1 cells, cell
 * (row, col) is the point (col - r, row - r, 0) (np.meshgrid puts i on columns, j on rows).
 * ofp_lag_maps: d_sensors [S][3] -> d_maps [S][S][side][side] float32 with map (i, j) =
 *   rint((|p - s_j| / c - |p - s_i| / c) * sr), i.e. lag_map_3d(s_j, s_i) (multilateration.py:945-1001; 2-D
 *   sensors have z = 0, lag_map_2d :902-942); NaN where col'^2 + row'^2 > mask_r2 (the caller's
 *   (r + tol*scale)^2) and where the value is below floor_v (-INFINITY for none; Multilaterate3D uses
 *   -samples_per_cm, :372); maps (i, i) are all NaN.  d_min / d_max [S][S] (both or neither): nanmin /
 *   nanmax of each map, NaN for an all-NaN map.  S in 2..64, r <= 4096.
 * ofp_locate_legal: is_legal_3d (:413-426) for G groups: d_sensors [G][3] int32 (origin, a, b), d_onsets
 *   [G][3] -> d_idx [G][2] = np.unravel_index(np.argmax(legal), shape, "F") of the mask
 *   |map(o,a) - lag_a| < tolerance and |map(o,b) - lag_b| < tolerance (strict, NaN illegal): the first
 *   legal cell in row-major order as (col, row); (0, 0) if none; (-1, -1) for a sensor index outside 0..S-1.
 * ofp_trilaterate: solve_trilateration_3d (:230-316) for G groups: scipy.optimize.fsolve(xtol, maxfev,
 *   fprime) = MINPACK hybrj, mode 1, factor 100 (csrc/ofp_hybrj.h).  d_geom [G][9] = origin, a, b (x, y, z);
 *   d_delta [G][2] = delta_d_a, delta_d_b; d_guess [G][2] -> d_root [G][2] (the last iterate), d_ier [G]
 *   (fsolve's ier; the reference accepts only 1) and d_nfev [G] (MINPACK's count; fsolve's info["nfev"]
 *   also counts two calls of its own and is 2 higher), both may be NULL.
 * ofp_locate_groups: per row of ofp_group_onsets' output (d_groups [n_clips][cap_groups][n_channels], rows
 *   beyond d_n_groups[clip] unused, d_n_groups may be NULL; channel k is sensor k, n_channels <= S): the three
 *   earliest channels present, ordered by onset (ties by channel), are origin, a, b; is_legal on (origin, a)
 *   and (origin, b) against d_min / d_max, the legality search with `tolerance` (samples), the guess
 *   (col, row) - radius, trilaterate's reordering when a's slot holds sensor 1 (:542-544), then hybrj with
 *   delta = lag / sr * c -- or, with mlp != NULL, the network on the float32 lags, times 100 (:554-557).
 *   d_xy [rows][2] (NaN unless a solve ran), d_status [rows]: the ier (1 = located) or an OFP_LOCATE_* code,
 *   d_guess [rows][2] or NULL; d_ws: ofp_locate_workspace_bytes(n_clips * cap_groups) bytes.
 * ofp_locate_section: Multilaterate3D.locate's cross-correlation input (:466-476) from d_x [n][ld] (a ring
 *   section): for columns c0, c1, median filter of size 5 along time (scipy.ndimage 'reflect'), first
 *   difference, values >= 0 set to 0, absolute value -> d_out [2][n-1].  n >= 3. */
#define OFP_LOCATE_UNUSED (-1)        /* row beyond the clip's group count */
#define OFP_LOCATE_FEW_CHANNELS (-2)  /* fewer than three channels in the row */
#define OFP_LOCATE_ILLEGAL_LAG (-3)   /* is_legal failed for (origin, a) or (origin, b) */
#define OFP_LOCATE_NO_CELL (-4)       /* is_legal_3d returned (0, 0) */
int ofp_lag_maps(const double* d_sensors, int32_t S, int32_t r, double c, double sr, double mask_r2, double floor_v,
                 float* d_maps, float* d_min, float* d_max, void* stream);
int ofp_locate_legal(const float* d_maps, int32_t S, int32_t r, const int32_t* d_sensors, const int64_t* d_onsets,
                     int64_t G, double tolerance, int32_t* d_idx, void* stream);
int ofp_trilaterate(const double* d_geom, const double* d_delta, const double* d_guess, int64_t G, double xtol,
                    int32_t maxfev, double* d_root, int32_t* d_ier, int32_t* d_nfev, void* stream);
int64_t ofp_locate_workspace_bytes(int64_t n_rows);
int ofp_locate_groups(const int64_t* d_groups, int64_t n_clips, int64_t cap_groups, int32_t n_channels,
                      const int64_t* d_n_groups, const double* d_sensors, int32_t S, const float* d_maps,
                      const float* d_min, const float* d_max, int32_t r, double tolerance, double sr, double c,
                      double radius, double xtol, int32_t maxfev, const ofp_mlp* mlp, double* d_xy,
                      int32_t* d_status, double* d_guess, void* d_ws, int64_t ws_bytes, void* stream);
int ofp_locate_section(const float* d_x, int64_t n, int32_t ld, int32_t c0, int32_t c1, float* d_out, void* stream);
/* ofp_locate_groups for the 2-D Multilaterate (multilateration.py:677-733; d_sensors [S][3] with z = 0, maps of the
 * 2-D grid): the same row rule and OFP_LOCATE_* codes, but trilaterate as that class has it -- origin, a, b stay in
 * onset order (no reordering) and delta = lag * c / sr (multiply first).  d_xy is the Cartesian root in cm; the
 * reference's tuple is cartesian_to_polar(x, y, radius), a host formula.  No model path. */
int ofp_locate_groups_2d(const int64_t* d_groups, int64_t n_clips, int64_t cap_groups, int32_t n_channels,
                         const int64_t* d_n_groups, const double* d_sensors, int32_t S, const float* d_maps,
                         const float* d_min, const float* d_max, int32_t r, double tolerance, double sr, double c,
                         double radius, double xtol, int32_t maxfev, double* d_xy, int32_t* d_status,
                         double* d_guess, void* d_ws, int64_t ws_bytes, void* stream);

/* ---- Multilaterate3D.locate as device code (multilateration.py:428-575) ---------------------------------------
 * The reference's state machine with its state (`ongoing`) in device memory: one call feeds (sensor, onset, counter)
 * and returns what locate returns.  Every quirk is kept: lags are measured from a group's first onset, the swap on
 * a negative lag stays in force for the rest of the call, the cross-correlation step (section of the last
 * counter - first_onset + 61 rows, median 5, diff, negative part, abs; the arithmetic of ofp_locate_section,
 * ofp_xcorr_lag and ofp_adjust_onset) moves the group's first onset in place, an extended group is appended twice
 * (the two entries are ONE Python object: a later in-place change of one shows in the other, which `alias` records),
 * the third member breaks out of the loop when the first two sensors are equal, and a call that reaches trilaterate
 * returns with `ongoing` = the groups collected so far (remove_seed only after a successful solve).
 * Capacity: OFP_LOCS_GROUPS groups of up to OFP_LOCS_MEMBERS members; the flags are sticky and never silent. */
#define OFP_LOCS_GROUPS 64
#define OFP_LOCS_MEMBERS 8
#define OFP_LOCF_GROUPS 1    /* a group was not appended: more than OFP_LOCS_GROUPS groups */
#define OFP_LOCF_MEMBERS 2   /* a group was not extended: more than OFP_LOCS_MEMBERS members */
#define OFP_LOCF_SECTION 4   /* a cross-correlation step was skipped: section longer than the bound or under 3 rows */
#define OFP_LOCF_BAD_CALL 8  /* a call was ignored: sensor outside 0..S-1 or counter outside the recording */
typedef struct ofp_locate_state {
    int32_t n_groups;
    int32_t flags;                                        /* OFP_LOCF_* seen so far */
    int32_t len[OFP_LOCS_GROUPS];                         /* members per group */
    int32_t alias[OFP_LOCS_GROUPS];                       /* 1: the same object as the group before it */
    int32_t sensors[OFP_LOCS_GROUPS][OFP_LOCS_MEMBERS];
    int64_t onsets[OFP_LOCS_GROUPS][OFP_LOCS_MEMBERS];
} ofp_locate_state;
/* the locator's tables (all device pointers, as ofp_locate_groups takes them) */
typedef struct ofp_hop_locator {
    const double* d_sensors;   /* [S][3] */
    int32_t S;                 /* 3..64 */
    const float* d_maps;       /* [S][S][2r+1][2r+1] */
    const float* d_min;        /* [S][S] */
    const float* d_max;
    int32_t r;
    double samples_per_cm, sr, c, radius, xtol;
    int32_t maxfev;
    const ofp_mlp* mlp;        /* 2 -> 2 network replacing the solver, or NULL; parameters are copied by a session */
    int32_t use_audio;         /* != 0: the cross-correlation step runs (locate's rec_audio is given) */
    int32_t max_section;       /* most rows of a section, 3..4096; a longer one sets OFP_LOCF_SECTION */
} ofp_hop_locator;
/* Replay: K calls through one state machine in ONE launch of one workgroup.  d_sensor [K] int32, d_onset [K],
 * d_counter [K] int64; d_audio [n_rows][n_channels] float32 or NULL (then no cross-correlation step; with it,
 * loc->use_audio must be set and call k sees rows [0, d_counter[k]), a section that would start before row 0 is cut
 * there as a Python slice is).  The replay starts from an empty `ongoing`; d_state receives the final one.
 * d_found [K] int32 (1: a position was returned), d_xy [K][2] (NaN otherwise). */
int ofp_locate_stream(const ofp_hop_locator* loc, const int32_t* d_sensor, const int64_t* d_onset,
                      const int64_t* d_counter, int64_t K, const float* d_audio, int64_t n_rows, int32_t n_channels,
                      ofp_locate_state* d_state, int32_t* d_found, double* d_xy, void* stream);
/* The replay for the 2-D Multilaterate.locate (multilateration.py:677-733) on the same state: no counter and no
 * recording (the class has no cross-correlation step), loc->use_audio and loc->max_section are ignored, loc->mlp must
 * be NULL, S >= 3.  What differs from the 3-D routine is kept: no skip past the largest lag at the top of the loop, no
 * swap, no break on equal first sensors, no remove_seed; a group that passes is_legal is appended twice (the second
 * entry with alias = 1); groups grow beyond three members and only a group that has just reached three is searched and
 * solved; a search that finds a cell ends the call with `ongoing` = the groups collected so far whether or not the
 * solve succeeds; deltas are lag * c / sr.  d_xy is the Cartesian root in cm.  A sensor outside 0..S-1 sets
 * OFP_LOCF_BAD_CALL. */
int ofp_locate_stream_2d(const ofp_hop_locator* loc, const int32_t* d_sensor, const int64_t* d_onset, int64_t K,
                         ofp_locate_state* d_state, int32_t* d_found, double* d_xy, void* stream);
/* The stage inside the hop graph of a session (before its first hop; the graph is captured again): after the
 * detector, the hop's onsets sorted by absolute sample (ties in record order) are fed with counter =
 * (hop_index + 1) * block_size until one returns a position (detect_hits, realtime/audio.py:62-74).  Rows of the
 * current hop are read from the hop buffer, older ones from the ring, rows before sample 0 are zeros (PARITY
 * UNPINNED: the reference's ring class is absent).  OFP_ERR_INVALID: S != channels, a detector that backtracks,
 * a ring shorter than max_section + block_size rows, a network that is not 2 -> 2.  ofp_hop_reset clears the state. */
int ofp_hop_set_locator(ofp_hop_session* s, const ofp_hop_locator* loc);
/* The same stage with the 2-D Multilaterate.locate (as ofp_locate_stream_2d: use_audio / max_section ignored, no
 * network, no ring-length condition since no section is read).  h_xy of ofp_hop_collect_location is then the Cartesian
 * root in cm; everything else -- collect_location, locator_state, reset, both graph forms, groups -- is unchanged. */
int ofp_hop_set_locator_2d(ofp_hop_session* s, const ofp_hop_locator* loc);
/* The location block of the last collected hop: *status 0 none / 1 located, h_xy [2], the located group as
 * trilaterate left it (*n_members, h_sensors / h_onsets [OFP_LOCS_MEMBERS]), *fed onsets given to the state machine,
 * *dropped onsets of the hop after the one that located (never fed, as in the reference), *flags. */
int ofp_hop_collect_location(ofp_hop_session* s, int32_t* status, double* h_xy, int32_t* n_members,
                             int32_t* h_sensors, int64_t* h_onsets, int32_t* fed, int32_t* dropped, int32_t* flags);
/* copies `ongoing` out (no hop may be in flight) */
int ofp_hop_locator_state(ofp_hop_session* s, ofp_locate_state* h_state);

/* ---- the window regressor of a stream ("The window regressor in the hop") ------------------------
 * detection.find_onset_groups (detection.py:131-189) as an online state machine, fed the stream's onsets hop by hop,
 * each hop's sorted by sample (stable): a group is anchored at its first onset and takes every following onset with
 * sample - anchor <= max_distance; the first onset outside closes it, and so does the end of hop h (hops from 1) as
 * soon as h * block > anchor + max_distance.  A closed group with at least min_channels channels waits in a FIFO of
 * OFP_REG_QUEUE groups with start = min(row entries >= 0) - pre_samples; at the end of a hop the head is evaluated
 * when h * block >= start + frame_length: the window [channels][frame_length] from `start` (rows before sample 0
 * are zeros) goes through the model.  At most one group per hop.  The flags are sticky and never silent. */
#define OFP_REG_MAX_LAYERS 8
#define OFP_REG_MAX_SIGNALS 8
#define OFP_REG_MAX_OUT 64
#define OFP_REG_MAX_FRAME 4096
#define OFP_REG_QUEUE 8
#define OFP_REGF_QUEUE 1      /* a kept group was lost: more than OFP_REG_QUEUE groups pending */
#define OFP_REGF_BAD_ONSET 2  /* an onset was ignored: channel outside 0..channels-1 or a negative sample */
typedef struct ofp_regress_state {
    int32_t open, head, len, flags;   /* a group is open; the FIFO's head slot and length; OFP_REGF_* seen so far */
    int64_t anchor;
    int64_t wake;                      /* the first hop end at which the open group times out or the head is due */
    int64_t row[OFP_REG_MAX_SIGNALS];  /* the open group's row */
    int64_t q_start[OFP_REG_QUEUE];
    int64_t q_row[OFP_REG_QUEUE][OFP_REG_MAX_SIGNALS];
} ofp_regress_state;
/* A model.CNN (kind 0), the shared-stack model.CCCNN (kind 1) or the grouped one (kind 2) in eval semantics, and the
 * stage's four parameters.  cout / kernels / strides [n_conv] and groups are the Conv1d modules' own (kind 1: groups
 * 1 and one input channel, every sensor channel an item; kind 2: groups = channels).  norm 0: none; 1: an eval-mode
 * BatchNorm1d folded into (scale, shift) by the caller (kind 0 only); 2: GroupNorm(1, cout) with gn_eps (kinds 1, 2).
 * d_params, device memory, n_params floats: per conv layer weight [cout][cin / groups][k], bias [cout], then with a
 * norm (scale, shift) or (gamma, beta) [cout] each; then fc weight [n_out][fc_in], fc bias [n_out].  A session and
 * the replay copy nothing but read it while they run; a session keeps its own copy.
 * Envelope: channels 1..OFP_REG_MAX_SIGNALS, n_conv 1..OFP_REG_MAX_LAYERS, n_out 1..OFP_REG_MAX_OUT, width ==
 * frame_length <= OFP_REG_MAX_FRAME, every tensor between two layers at most 2^20 floats. */
typedef struct ofp_hop_regressor {
    int32_t kind, channels, width, n_out, n_conv;
    int32_t cout[OFP_REG_MAX_LAYERS], kernels[OFP_REG_MAX_LAYERS], strides[OFP_REG_MAX_LAYERS];
    int32_t padding, dilation, groups, act, norm, pool;
    float gn_eps;
    const float* d_params;
    int64_t n_params;
    int32_t frame_length, pre_samples, max_distance, min_channels;
} ofp_hop_regressor;
/* Replay: the state machine and the model over a resident recording d_audio [n_rows][channels] and a given onset
 * list (d_channel / d_onset [K], already in feed order: sorted by sample, stable), hop by hop (n_rows / block_size
 * hops; onset k belongs to hop d_onset[k] / block_size + 1) in ONE launch of one workgroup, from an empty state.
 * Per hop h - 1: d_status 1 when a hit was evaluated, then d_start, d_row [channels] and d_y [n_out] (untouched
 * otherwise); d_pending the FIFO's length before the hop's evaluation (its highest value during the hop);
 * *d_flags the final OFP_REGF_*.  d_ws: 2 * ofp_regress_workspace_floats floats, or NULL when that is 0. */
int64_t ofp_regress_workspace_floats(const ofp_hop_regressor* r);
int ofp_regress_stream(const ofp_hop_regressor* r, const float* d_audio, int64_t n_rows, int32_t block_size,
                       const int32_t* d_channel, const int64_t* d_onset, int64_t K, int32_t* d_status, int64_t* d_start,
                       int64_t* d_row, float* d_y, int32_t* d_pending, int32_t* d_flags, float* d_ws, void* stream);
/* The stage inside the hop graph of a session (before its first hop; the graph is captured again; on failure the
 * session is the one it was).  It runs after the detector and the locator stage, in the detector's workgroup (one
 * kernel form) or as one more node before the spectral node.  OFP_ERR_INVALID: channels != the session's, a detector
 * that backtracks, max_distance < block_size, min_channels outside 1..channels, more groups pending than
 * OFP_REG_QUEUE or a ring shorter than max_distance + pre_samples + (K + 1) * block_size rows, K = max(0,
 * ceil((max_distance + frame_length - pre_samples) / block_size) - 1) (INTEGRATION.md derives both).
 * ofp_hop_reset clears the state. */
int ofp_hop_set_regressor(ofp_hop_session* s, const ofp_hop_regressor* r);
/* The hit block of the last collected hop: *status 0 none / 1 evaluated, then *start, h_row [channels] and h_y
 * [n_out]; *flags always. */
int ofp_hop_collect_hit(ofp_hop_session* s, int32_t* status, int64_t* start, int64_t* h_row, float* h_y, int32_t* flags);

/* ---- 2-D hit location: find_lag, MultilateratePaired, lag_intensity_map (multilateration.py) -------------------
 * ofp_find_lags: find_lag / find_lag_multi (:878-899) for n_rows row pairs.  Row r of a starts at
 *   d_a + (d_a_off ? d_a_off[r] : r * a_stride) and steps elem_stride floats (b likewise, same element stride), so
 *   the rows can be columns of an [N][C] clip; lengths d_len_a[r] / d_len_b[r] (or len_a / len_b for every row,
 *   which are also the upper bounds of the per-row lengths), 1..4096.  The correlation is np.correlate(a, b,
 *   "full") by the canon of ofp_xcorr_lag (fp64 over ascending index, rounded once to fp32).
 *   d_lag [n_rows]: np.argmax (first maximum, a NaN wins) - (len_a - 1); INT32_MIN for a row of length 0.
 *   top_n in 0..16; with top_n > 0: d_peak_lag / d_peak_val [n_rows][top_n] the peaks of
 *   scipy.signal.find_peaks(cc) (strict local maxima, a plateau at its middle (left + right) // 2, never an end
 *   point) by descending value, exact ties by ascending index (numpy's argsort leaves their order undefined), as
 *   lags and cc ** 2 in fp32; unused slots (0, NaN).  d_n_peaks [n_rows] (may be NULL when top_n == 0): the slots
 *   used (<= top_n; 0 when top_n == 0), -1 when the correlation holds a non-finite value (no peaks reported), -2
 *   for a row of length 0.
 * ofp_vote_index: a bucket index of n_maps lag maps (map k is d_maps + d_map_ids[k] * cells), built once: every
 *   value must be NaN or an integer in [d_vmin[k], d_vmin[k] + n_buckets).  d_starts [n_maps][n_buckets + 1]: the
 *   first slot of each value; d_sorted [n_maps][cells]: the non-NaN cells ordered by value, ascending cell index
 *   within a value (a stable counting sort).  d_bad [n_maps]: 1 where a value broke the rule (the index is then
 *   incomplete).  cells <= 2^20, n_buckets <= 32768, n_maps <= 128.
 * ofp_paired_windows: MultilateratePaired.locate_cc's windows x[onset - left : onset + right] (clipped at the
 *   clip's end) of B hits in clips [n_clips][n_samples][n_channels] (channel k is sensor k, n_channels >= S), for
 *   the first channel i and its neighbours (i - 1) % S, (i + 1) % S: rows 2h, 2h + 1 of d_a_off / d_b_off / d_len
 *   [2B], ready for ofp_find_lags (elem_stride n_channels).  Hits are d_onset / d_first / d_clip [B] (d_clip may
 *   be NULL: clip 0), or, with d_groups, the rows of ofp_group_onsets (B = n_clips * cap_groups): the earliest
 *   channel present, ties by channel.  d_first_out, d_status [B]: OFP_PAIRED_OK or an OFP_PAIRED_* code (length 0
 *   rows then).  left >= 0, right >= 1, left + right <= 4096.
 * ofp_paired_vote: the vote of locate_cc (:839-875) for B hits, from the index (map 2i + k of the index is
 *   sensor i's neighbour k, as above) and d_lags [B][2] (from ofp_find_lags): the cells with
 *   lag - tol < map < lag + tol are counted over the neighbour maps (one map when S == 2) and the smallest flat
 *   index among the cells with the highest count is returned (np.argmax; cell 0 when no cell counts).  Hits whose
 *   d_status_in is not OFP_PAIRED_OK keep it and get cell -1, NaN coordinates.  d_cell [B], d_xy [B][2] = (col -
 *   (side-1)/2, (side-1)/2 - row), d_rphi [B][2] = cartesian_to_polar(x, y, radius), d_status [B].  d_res (NULL, or
 *   with d_maps and d_map_ids): the full vote grids [B][side][side] float32 (the reference's self.res), B <= 65535.
 * ofp_paired_solve: MultilateratePaired.locate (:798-834) for B rows: d_sensors [S][3] (z = 0), d_lags [B][2],
 *   d_first [B] -> the weighted initial guess, hybrj as ofp_trilaterate (origin i, a = (i-1) % S, b = (i+1) % S,
 *   delta = lag * c / sr), d_root [B][2], d_rphi [B][2] = cartesian_to_polar(root, radius), d_ier [B] (fsolve's
 *   ier; the reference raises unless 1; OFP_PAIRED_BAD_HIT for a first sensor outside 0..S-1).
 * ofp_intensity_maps: lag_intensity_map's signal strengths (:1065-1101): d_mics [2][3] -> d_out [2][side][side],
 *   10 log10 of attenuate_intensity (source intensity 1) at p = (col - r, row - r, 0), fp64 rounded to float32. */
#define OFP_PAIRED_OK 0
#define OFP_PAIRED_UNUSED (-1)        /* group row beyond the clip's group count */
#define OFP_PAIRED_NO_CHANNEL (-2)    /* group row without a channel */
#define OFP_PAIRED_NEG_WINDOW (-5)    /* onset - left < 0 (refused; the reference's slice would wrap) */
#define OFP_PAIRED_EMPTY_WINDOW (-6)  /* the window is empty (onset beyond the clip) */
#define OFP_PAIRED_BAD_HIT (-7)       /* first sensor or clip index out of range */
int ofp_find_lags(const float* d_a, const float* d_b, int64_t n_rows, int64_t a_stride, int64_t b_stride,
                  int32_t elem_stride, const int64_t* d_a_off, const int64_t* d_b_off, int32_t len_a, int32_t len_b,
                  const int32_t* d_len_a, const int32_t* d_len_b, int32_t top_n, int32_t* d_lag, int32_t* d_peak_lag,
                  float* d_peak_val, int32_t* d_n_peaks, void* stream);
int ofp_vote_index(const float* d_maps, int64_t cells, const int32_t* d_map_ids, int32_t n_maps,
                   const int32_t* d_vmin, int32_t n_buckets, int32_t* d_starts, int32_t* d_sorted, int32_t* d_bad,
                   void* stream);
int ofp_paired_windows(int64_t n_clips, int64_t n_samples, int32_t n_channels, int32_t S, const int64_t* d_onset,
                       const int32_t* d_first, const int32_t* d_clip, const int64_t* d_groups, int64_t cap_groups,
                       const int64_t* d_n_groups, int64_t B, int32_t left, int32_t right, int64_t* d_a_off,
                       int64_t* d_b_off, int32_t* d_len, int32_t* d_first_out, int32_t* d_status, void* stream);
int ofp_paired_vote(const float* d_maps, const int32_t* d_map_ids, const int32_t* d_starts, const int32_t* d_sorted,
                    const int32_t* d_vmin, int32_t n_buckets, int32_t S, int32_t side, const int32_t* d_first,
                    const int32_t* d_lags, const int32_t* d_status_in, int64_t B, double tol, double radius,
                    int32_t* d_cell, double* d_xy, double* d_rphi, int32_t* d_status, float* d_res, void* stream);
int ofp_paired_solve(const double* d_sensors, int32_t S, const int32_t* d_lags, const int32_t* d_first, int64_t B,
                     double c, double sr, double radius, double xtol, int32_t maxfev, double* d_root, double* d_rphi,
                     int32_t* d_ier, void* stream);
int ofp_intensity_maps(const double* d_mics, int32_t r, double reflectivity, float* d_out, void* stream);

/* ---- the voting locator of a stream ("The voting locator in the hop") -----------------------------
 * MultilateratePaired.locate_cc as a stage of a stream: the grouping state machine and FIFO of the window regressor
 * above (ofp_regress_state, with frame_length = left + right and pre_samples = left), and for the group that is due
 * -- the first hop whose end is >= onset + right; the window is never clipped -- the first channel (the row's
 * earliest, ties by channel) and its onset, ofp_find_lags' lags of the window x[onset - left : onset + right] against
 * the two neighbours, and ofp_paired_vote's cell and coordinates.  A window that starts below sample 0 is reported
 * with OFP_PAIRED_NEG_WINDOW (cell -1, lags INT32_MIN, NaN coordinates).  No vote grid is written.
 * d_starts / d_sorted / d_vmin / n_buckets: the index ofp_vote_index built over the 2 S neighbour maps (map 2i + k is
 * sensor i's neighbour k); they are read while a session or the replay runs and must outlive it.
 * Envelope: S 2..OFP_REG_MAX_SIGNALS, left + right <= 1024, and 32 + 12 (left + right) + 4 ceil(side^2 / 32) bytes of
 * LDS (partials, three rows, vote bitmap) at most 96 KiB; there is no global-memory fallback. */
typedef struct ofp_hop_paired {
    const int32_t* d_starts;
    const int32_t* d_sorted;
    const int32_t* d_vmin;
    int32_t n_buckets, S, side;
    double radius, tol;
    int32_t left, right, max_distance, min_channels;
} ofp_hop_paired;
/* Replay, as ofp_regress_stream: d_audio [n_rows][S], the onset list in feed order, n_rows / block_size hops in ONE
 * launch of one workgroup from an empty state.  Per hop h - 1: d_hit 1 when a group was evaluated, then d_status,
 * d_onset_out, d_first, d_row [S], d_lags [2], d_cell, d_xy [2] and d_rphi [2] (untouched otherwise); d_pending the
 * FIFO's length before the hop's evaluation; *d_flags the final OFP_REGF_*. */
int ofp_locate_cc_stream(const ofp_hop_paired* p, const float* d_audio, int64_t n_rows, int32_t block_size,
                         const int32_t* d_channel, const int64_t* d_onset, int64_t K, int32_t* d_hit, int32_t* d_status,
                         int64_t* d_onset_out, int32_t* d_first, int64_t* d_row, int32_t* d_lags, int32_t* d_cell,
                         double* d_xy, double* d_rphi, int32_t* d_pending, int32_t* d_flags, void* stream);
/* The stage inside the hop graph of a session (before its first hop; the graph is captured again; on failure the
 * session is the one it was).  It runs after the detector, in the detector's workgroup (one kernel form) or as one
 * more node before the spectral node.  OFP_ERR_INVALID: S != the session's channels, a session that already has a
 * locator or a regressor, a detector that backtracks, max_distance < block_size, and the queue and ring conditions of
 * ofp_hop_set_regressor with frame_length = left + right, pre_samples = left.  ofp_hop_reset clears the state. */
int ofp_hop_set_locator_paired(ofp_hop_session* s, const ofp_hop_paired* p);
/* The block of the last collected hop: *hit 0 none / 1 evaluated, then *status, *onset, *first, h_row [S], h_lags [2],
 * *cell, h_xy [2] and h_rphi [2]; *flags always. */
int ofp_hop_collect_cc_hit(ofp_hop_session* s, int32_t* hit, int32_t* status, int64_t* onset, int32_t* first,
                           int64_t* h_row, int32_t* h_lags, int32_t* cell, double* h_xy, double* h_rphi, int32_t* flags);

/* ---- calibration: train_location_model, optimize_positions (calibration.py:563-754) ----------------------------
 * One workgroup runs one whole optimisation inside one launch (full-batch forward, mean loss, early stop, backward,
 * clip_grad_norm_ with max_norm 1, Adam with torch's defaults); the grid is the M independent problems.  fp32, no
 * atomics, every batch reduction in a fixed order that does not depend on M.
 * Network: n_layers Linear layers of dims [n_layers + 1], every one but the last followed by BatchNorm1d (when
 *   batch_norm; batch statistics, running statistics with momentum 0.1) and the activation act (OFP_ACT_*).
 *   Parameters are packed per layer as weight [out][in], bias [out] (when bias), BatchNorm weight, bias [out]; the
 *   running statistics as mean [out], var [out] per BatchNorm.  Limits: 1..8 layers, widths 1..128, n 1..1024
 *   (n >= 2 with BatchNorm); beyond them OFP_ERR_INVALID.
 * ofp_fcnn_train_lds_bytes: the bytes of parameters, moments and activations one problem keeps; up to 160 KiB less
 *   512 B they live in LDS, beyond that in d_ws (ofp_fcnn_train_workspace_bytes, 0 when the LDS is used).  -1 for
 *   arguments outside the limits.
 * ofp_fcnn_train: problem m reads d_x + m * x_stride [n][dims[0]] and d_y + m * y_stride [n][dims[n_layers]] (a
 *   stride of 0 shares one batch), starts at d_p0 [M][n_params] / d_stats0 [M][n_stats], and takes its per-epoch
 *   Adam scalars from row d_rate_idx[m] of d_rates [U][num_epochs][2] = (lr_t / (1 - 0.9^t), sqrt(1 - 0.999^t)).
 *   loss: 0 = L1, 1 = MSE (mean).  Per epoch the loss is stored in d_loss [M][num_epochs] first; then
 *   loss < last - eps resets the patience counter, else it rises while below patience, else the run ends before
 *   that epoch's update.  d_epochs [M]: losses stored.  d_params / d_stats: the final state.
 * ofp_fcnn_loss_grads: the same kernel for one epoch, leaving after the backward pass: d_loss [M], d_grads
 *   [M][n_params] (unclipped).
 * ofp_tdoa_fit: optimize_positions.  d_obs + m * obs_stride [n][2] observed TDoA in seconds (pairs 0-2 and 1-3),
 *   d_sensors0 [M][4][3], d_sounds0 [M][n][2], d_c0 [M]; d_rates [U][num_epochs][4] = the step sizes of sensors,
 *   sounds and C, then sqrt(1 - 0.999^t).  The early-stop test comes before the loss is counted: d_epochs [M] is
 *   the number of updates, and d_loss [m][d_epochs[m]] holds the stopping epoch's loss when the run stopped.  d_sounds
 *   [M][n][3] are the positions the last forward pass used (z = 0), as the reference returns them.  n 1..4096.
 * ofp_tdoa_loss_grads: the same kernel, leaving after the first epoch's sums: d_loss [M], d_g_sensors [M][4][3],
 *   d_g_sounds [M][n][2] and d_g_c [M], the unclipped gradients at d_sensors / d_sounds [M][n][2] / d_c.  No rate
 *   tables; the limits of ofp_tdoa_fit. */
int64_t ofp_fcnn_train_lds_bytes(int32_t n_layers, const int32_t* dims, int32_t batch_norm, int32_t bias, int64_t n);
int64_t ofp_fcnn_train_workspace_bytes(int32_t n_layers, const int32_t* dims, int32_t batch_norm, int32_t bias,
                                       int64_t n, int64_t M);
int ofp_fcnn_train(int32_t n_layers, const int32_t* dims, int32_t act, int32_t batch_norm, int32_t bias,
                   int32_t loss, int64_t M, int64_t n, const float* d_x, int64_t x_stride, const float* d_y,
                   int64_t y_stride, const float* d_p0, const float* d_stats0, const float* d_rates,
                   const int32_t* d_rate_idx, int32_t num_epochs, float eps, int32_t patience, float* d_params,
                   float* d_stats, float* d_loss, int32_t* d_epochs, void* d_ws, int64_t ws_bytes, void* stream);
int ofp_fcnn_loss_grads(int32_t n_layers, const int32_t* dims, int32_t act, int32_t batch_norm, int32_t bias,
                        int32_t loss, int64_t M, int64_t n, const float* d_x, int64_t x_stride, const float* d_y,
                        int64_t y_stride, const float* d_p0, float* d_loss, float* d_grads, void* d_ws,
                        int64_t ws_bytes, void* stream);
int ofp_tdoa_fit(int64_t M, int64_t n, const float* d_obs, int64_t obs_stride, const float* d_sensors0,
                 const float* d_sounds0, const float* d_c0, int32_t loss, const float* d_rates,
                 const int32_t* d_rate_idx, int32_t num_epochs, float eps, int32_t patience, float* d_sensors,
                 float* d_sounds, float* d_c, float* d_loss, int32_t* d_epochs, void* stream);
int ofp_tdoa_loss_grads(int64_t M, int64_t n, const float* d_obs, int64_t obs_stride, const float* d_sensors,
                        const float* d_sounds, const float* d_c, int32_t loss, float* d_loss, float* d_g_sensors,
                        float* d_g_sounds, float* d_g_c, void* stream);

/* ---- training model.CNN (model.py:52-162, the loop of train.py) -----------------------------------------------
 * Network: n_conv layers of Conv1d (stride 1, bias) -> activation -> BatchNorm1d (when batch_norm) -> MaxPool1d(2, 2)
 *   (when pool), flatten, Linear to n_out values; channels[0] inputs of `width` samples, channels[i] outputs of
 *   conv i.  Activations are [n][channels][width], as torch lays them out.  fp32 data; every sum over the batch in
 *   fp64 with a shape fixed by the dimensions alone (no atomics: results are bitwise reproducible).
 * Parameters are packed in state_dict order: per conv layer weight [cout][cin/groups][kernel], bias [cout], then
 *   (when batch_norm) BatchNorm weight [cout], bias [cout]; last fc weight [n_out][channels[n_conv] * width_last],
 *   bias [n_out].  The running statistics are packed as mean [cout], var [cout] per BatchNorm.
 * Limits (beyond them OFP_ERR_INVALID, or -1 from the size functions): 1..3 conv layers, 1..128 channels, kernel
 *   1..8, width 1..512, n and n_val 1..1024 (n * width >= 2 with BatchNorm), n_out 1..16, 0 < bn_momentum <= 1.
 * ofp_cnn_train_slab: the (sample, position) pairs one workgroup of the batch reductions sums.
 * ofp_cnn_train: fits up to num_epochs epochs of: training-mode forward of d_x [n][channels[0]][width] (batch
 *   statistics; running statistics updated with the unbiased variance), mean loss against d_y [n][n_out] (loss 0 =
 *   L1, 1 = MSE) into d_train_loss[epoch], backward, one torch.optim.NAdam step with row `epoch` of d_rates
 *   [num_epochs][4] = (-lr (1 - mu_t) / (1 - mu_product_t), -lr mu_{t+1} / (1 - mu_product_t mu_{t+1}),
 *   1 - 0.999^t, unused); then, when n_val > 0, an eval-mode forward of d_x_val on the running statistics and its
 *   mean L1 loss into d_val_loss[epoch].  Stop rule (patience >= 0, needs n_val > 0): a validation loss that is not
 *   below the best so far counts, a lower one resets the count; once the count has reached patience the run ends
 *   after the first epoch at which at least min_epochs epochs are done.  d_params / d_stats are read and updated in
 *   place; curve slots of epochs not run are left untouched; *h_epochs (host memory) = epochs run.  One epoch is a
 *   linear chain of kernels captured once as a hipGraph and replayed (the first epoch is launched plainly); the
 *   host looks at the stop word every 64 epochs and synchronises the stream before it returns.  `stream` must be a
 *   created stream (capture is not possible on the null stream) unless the environment has OFP_CNN_GRAPH=nodes,
 *   which launches the same chain without a graph.  Nothing is allocated: d_ws of ofp_cnn_train_workspace_bytes.
 * ofp_cnn_loss_grads: one training-mode forward and backward: d_loss [1], d_grads packed like the parameters.
 * ofp_conv1d_backward: d_dz [n][cout][wc] (wc = w + 2 padding - dilation (k - 1)) -> d_dw [cout][cin/groups][k],
 *   d_db [cout] and, unless NULL, d_dx [n][cin][w].  ofp_batchnorm_train_forward / _backward: BatchNorm1d in training
 *   mode on d_x [n][C][w]: d_y, the saved d_mean / d_rstd [C], running statistics updated in place; and d_dx,
 *   d_dgamma, d_dbeta from d_dy.  ofp_nadam_step: one NAdam step of n elements with one row of the rate table.
 * ofp_linear_head_train: the Linear head both trainers end in, by the launches of their epochs: d_h [n][F], d_w [O][F],
 *   d_b [O], targets d_y [n][O], loss 0 = L1, 1 = MSE -> d_out [n][O] = h W^T + b, d_dy [n][O] = d loss / d out of
 *   the mean loss, d_loss [1] the mean loss, d_dw [O][F], d_db [O], d_dh [n][F].  Sums over features and over samples
 *   are fp64 rounded once (samples in chunks of 64, the chunks added in order); d_dh is an fp32 fmaf chain over the
 *   outputs.  Limits: n 1..1024, O 1..16, F >= 1; beyond them OFP_ERR_INVALID before any launch (-1 from the size
 *   function). */
typedef struct ofp_cnn_config {
    int32_t n_conv;
    int32_t channels[4];
    int32_t kernel, padding, dilation, groups;
    int32_t act, batch_norm, pool;
    int32_t width, n_out, loss;
    float bn_momentum;
    double bn_eps;
} ofp_cnn_config;
int32_t ofp_cnn_train_slab(void);
int64_t ofp_cnn_train_workspace_bytes(const ofp_cnn_config* cfg, int64_t n, int64_t n_val);
int ofp_cnn_train(const ofp_cnn_config* cfg, int64_t n, const float* d_x, const float* d_y, int64_t n_val,
                  const float* d_x_val, const float* d_y_val, const float* d_rates, int32_t num_epochs,
                  int32_t min_epochs, int32_t patience, float* d_params, float* d_stats, float* d_train_loss,
                  float* d_val_loss, int32_t* h_epochs, void* d_ws, int64_t ws_bytes, void* stream);
int ofp_cnn_loss_grads(const ofp_cnn_config* cfg, int64_t n, const float* d_x, const float* d_y,
                       const float* d_params, float* d_loss, float* d_grads, void* d_ws, int64_t ws_bytes,
                       void* stream);
int64_t ofp_conv1d_backward_workspace_bytes(int64_t n, int32_t cin, int32_t w, int32_t cout, int32_t k,
                                            int32_t padding, int32_t dilation, int32_t groups);
int ofp_conv1d_backward(const float* d_x, int64_t n, int32_t cin, int32_t w, const float* d_w, int32_t cout,
                        int32_t k, int32_t padding, int32_t dilation, int32_t groups, const float* d_dz, float* d_dx,
                        float* d_dw, float* d_db, void* d_ws, int64_t ws_bytes, void* stream);
int64_t ofp_linear_head_train_workspace_bytes(int64_t n, int32_t F, int32_t O);
int ofp_linear_head_train(const float* d_h, int64_t n, int32_t F, const float* d_w, int32_t O, const float* d_b,
                          const float* d_y, int32_t loss, float* d_out, float* d_dy, float* d_loss, float* d_dw,
                          float* d_db, float* d_dh, void* d_ws, int64_t ws_bytes, void* stream);
int64_t ofp_batchnorm_train_workspace_bytes(int64_t n, int32_t C, int32_t w);
int ofp_batchnorm_train_forward(const float* d_x, int64_t n, int32_t C, int32_t w, const float* d_gamma,
                                const float* d_beta, double eps, float momentum, float* d_running_mean,
                                float* d_running_var, float* d_y, float* d_mean, float* d_rstd, void* d_ws,
                                int64_t ws_bytes, void* stream);
int ofp_batchnorm_train_backward(const float* d_x, int64_t n, int32_t C, int32_t w, const float* d_gamma,
                                 const float* d_mean, const float* d_rstd, const float* d_dy, float* d_dx,
                                 float* d_dgamma, float* d_dbeta, void* d_ws, int64_t ws_bytes, void* stream);
int ofp_nadam_step(float* d_p, const float* d_g, float* d_m, float* d_v, int64_t n, const float* d_row, void* stream);

/* ---- training model.CCCNN / model.LCCCNN (csrc/ofp_cccnn_train.hip) ------------------------------------------------
 * The reference's recipe (model.py:443-629, train.py): the whole training set is one batch; one epoch is a forward,
 *   the mean loss, a backward and one torch.optim.SGD step (momentum, weight decay on every parameter, dampening 0,
 *   no Nesterov) at the learning rate d_rates[epoch].  The conv stack sees items: group = 0 makes every (window,
 *   sensor) pair an item with one input channel (n * sensors items, layer l has layer_sizes[l] channels), group = 1
 *   makes every window an item with `sensors` input channels and a convolution of `sensors` groups (layer l has
 *   sensors * layer_sizes[l] channels).  Per layer: Conv1d (kernels[l], strides[l], shared padding / dilation) + bias,
 *   activation `act`, GroupNorm(1, channels) over the whole item when `norm`, MaxPool1d(2, 2) when `pool`.  Head, per
 *   (window, sensor) with maps f [K][V], K = layer_sizes[n_conv - 1]: cc[j] = sum_k sum_i f_k[i + j - (V - 1)]
 *   f_k[i], p = softmax(cc) over the 2V - 1 lags, out = fc(p of all sensors).  GroupNorm keeps no running
 *   statistics: the validation forward is the same forward.
 * Parameters are packed in state_dict order: per conv layer weight [cout][cin/groups][kernel], bias [cout], then
 *   (when norm) GroupNorm weight [cout], bias [cout]; last fc weight [n_out][sensors * (2V - 1)], bias [n_out].
 * Limits (beyond them OFP_ERR_INVALID, or -1 from the size functions): 1..8 conv layers, kernel 1..64, stride 1..4,
 *   1..64 channels per layer (sensors * layer_sizes[l] when grouped), width 1..512 (no layer wider than 1024), n and
 *   n_val 1..1024 with n * sensors <= 4096, n_out 1..16, ofp_autocorr_softmax_lds_bytes(K, V) <= 160 KiB, every layer
 *   leaves at least one column.
 * ofp_cccnn_train: as ofp_cnn_train (d_train_loss / d_val_loss [num_epochs], the stop rule, *h_epochs, one captured
 *   graph per epoch with the first epoch launched plainly, the stop word looked at every 64 epochs, a created
 *   stream); d_rates is float [num_epochs]; OFP_CCCNN_GRAPH=nodes launches the same chain without a graph.  The
 *   validation loss is always L1.  The momentum buffer starts fresh at every call.  Nothing is allocated: d_ws of
 *   ofp_cccnn_train_workspace_bytes.
 * ofp_cccnn_loss_grads: one forward and backward: d_loss [1], d_grads packed like the parameters.
 * ofp_conv1d_backward_strided: ofp_conv1d_backward with a stride; wc = (w + 2 padding - dilation (k - 1) - 1) /
 *   stride + 1; n 1..4096, channels 1..64, k 1..64, stride 1..4, w 1..1024.
 * ofp_groupnorm1_train_forward: GroupNorm(1, K) (+ MaxPool1d(2, 2)) of d_x [n][K][V] -> d_y [n][K][V or V/2] and the
 *   saved d_mean / d_rstd [n] (fp64 sums over the item's K V values, biased variance).  _backward: d_dy (shaped like
 *   d_y) -> d_dx [n][K][V], d_dgamma / d_dbeta [K]; the pool hands its gradient to the larger of a pair (the first
 *   on a tie), an odd last column gets none.  d_ws of ofp_groupnorm1_train_workspace_bytes.
 * ofp_autocorr_softmax_backward: d_f [items][K][V] (items = windows * C, sensor fastest), the forward's d_p
 *   [items][2V - 1], d_dout [windows][O], d_wfc [O][C * (2V - 1)] -> d_df [items][K][V].
 * ofp_sgd_step: g' = g + weight_decay p; buf = g' when `first`, else momentum buf + g'; p -= d_lr[0] buf. */
typedef struct ofp_cccnn_config {
    int32_t n_conv;
    int32_t sensors;
    int32_t layer_sizes[8];
    int32_t kernels[8];
    int32_t strides[8];
    int32_t padding, dilation, group;
    int32_t act, norm, pool;
    int32_t width, n_out, loss;
    float momentum, weight_decay;
    double gn_eps;
} ofp_cccnn_config;
int64_t ofp_cccnn_train_workspace_bytes(const ofp_cccnn_config* cfg, int64_t n, int64_t n_val);
int ofp_cccnn_train(const ofp_cccnn_config* cfg, int64_t n, const float* d_x, const float* d_y, int64_t n_val,
                    const float* d_x_val, const float* d_y_val, const float* d_rates, int32_t num_epochs,
                    int32_t min_epochs, int32_t patience, float* d_params, float* d_train_loss, float* d_val_loss,
                    int32_t* h_epochs, void* d_ws, int64_t ws_bytes, void* stream);
int ofp_cccnn_loss_grads(const ofp_cccnn_config* cfg, int64_t n, const float* d_x, const float* d_y,
                         const float* d_params, float* d_loss, float* d_grads, void* d_ws, int64_t ws_bytes,
                         void* stream);
int64_t ofp_conv1d_backward_strided_workspace_bytes(int64_t n, int32_t cin, int32_t w, int32_t cout, int32_t k,
                                                    int32_t padding, int32_t dilation, int32_t groups,
                                                    int32_t stride);
int ofp_conv1d_backward_strided(const float* d_x, int64_t n, int32_t cin, int32_t w, const float* d_w, int32_t cout,
                                int32_t k, int32_t padding, int32_t dilation, int32_t groups, int32_t stride,
                                const float* d_dz, float* d_dx, float* d_dw, float* d_db, void* d_ws, int64_t ws_bytes,
                                void* stream);
int64_t ofp_groupnorm1_train_workspace_bytes(int64_t n, int32_t K, int32_t V);
int ofp_groupnorm1_train_forward(const float* d_x, int64_t n, int32_t K, int32_t V, const float* d_gamma,
                                 const float* d_beta, double eps, int32_t pool, float* d_y, float* d_mean,
                                 float* d_rstd, void* stream);
int ofp_groupnorm1_train_backward(const float* d_x, int64_t n, int32_t K, int32_t V, const float* d_gamma,
                                  const float* d_beta, const float* d_mean, const float* d_rstd, int32_t pool,
                                  const float* d_dy, float* d_dx, float* d_dgamma, float* d_dbeta, void* d_ws,
                                  int64_t ws_bytes, void* stream);
int64_t ofp_autocorr_softmax_lds_bytes(int32_t K, int32_t V);
int ofp_autocorr_softmax_backward(const float* d_f, const float* d_p, const float* d_dout, const float* d_wfc,
                                  int64_t items, int32_t C, int32_t K, int32_t V, int32_t O, float* d_df,
                                  void* stream);
int ofp_sgd_step(float* d_p, const float* d_g, float* d_buf, int64_t n, const float* d_lr, int32_t first,
                 float momentum, float weight_decay, void* stream);

/* ---- the trainers' random stream: dropout, per-epoch shift and stretch augmentation (csrc/ofp_train_random.h) ------
 * Both trainers can regularise as the reference's train.py does: a dropout in front of the Linear head, and training
 *   windows cut anew every epoch, each shifted by up to +-max_shift samples.  torch's random stream cannot be
 *   reproduced; this is a documented stream of the library's own, and the user opts in by naming a seed.
 * Generator: Philox4x32 with 10 rounds (multipliers 0xD2511F53, 0xCD9E8D57; key increments 0x9E3779B9, 0xBB67AE85;
 *   round: p0 = M0 c0, p1 = M1 c2, c' = (hi(p1) ^ c1 ^ k0, lo(p1), hi(p0) ^ c3 ^ k1, lo(p0)), then the key is bumped).
 *   Key (seed & 0xffffffff, seed >> 32).  Counter (index / 4, site, epoch, 0), output word index % 4.  The epoch is the
 *   0-based epoch of the run, read on the device from the run's control block, so every replay of the epoch graph
 *   draws anew with no argument changed; ofp_*_loss_grads_random and the stand-alone forms take it as `epoch`.
 * Site 0, dropout: index = s F + f over the features [n][F] that feed the Linear head; dropped iff word <
 *   (uint32)(dropout_p 2^32); kept values are multiplied by (float)(1 / (1 - dropout_p)), dropped ones are 0; the
 *   backward does the same to the gradient.  0 <= dropout_p < 1; 0 launches nothing.  The validation forward has none.
 * Site 1, shifts: index = item; shift = ((word (2 max_shift + 1)) >> 32) - max_shift.  With n_extractions > 0 the
 *   trainer ignores d_x and first gathers, every epoch, x[j][c][t] = d_audio[d_starts[j % n_onsets] + shift_j + t][c]
 *   for the n = n_extractions * n_onsets items (item j = r * n_onsets + i is extraction r of onset i; d_y [n] is tiled
 *   to match by the caller) from the interleaved audio [audio_len][audio_channels]; d_starts [n_onsets] int64 is the
 *   hit's minimum onset less pre_samples.  The caller rules out windows that leave the audio (such rows read as 0).
 *   n_extractions = 0: no window source, d_x is used as it is.
 * Site 2, stretches (the reference's StretchFrameExtractor, which its train.py prepares and leaves commented out as
 *   too slow): index = item.  With the span S = int(frame_length * max_stretch) the reference draws randint(1, S) *
 *   choice((-1, 1)), uniform on {-(S-1), ..., -1, 1, ..., S-1} and never 0; S = 1 raises inside randint.  Here v =
 *   (word (uint32)(2 (S - 1))) >> 32, and stretch = v - (S - 1) if v < S - 1, else v - (S - 1) + 1.  stretch_span = 0
 *   means no stretch, 1 is refused, S >= 2 stretches; the shift of site 1 is unchanged and independent.  Item j then
 *   reads Nx_j = width + stretch_j rows of the audio from row d_starts[j % n_onsets] + shift_j, and every channel of
 *   them is resampled to width samples by the arithmetic of ofp_resample_windows: the same bits as that function
 *   gives for the same (start, nx, num).  A row outside the audio reads as 0; the caller rules it out.  Limits:
 *   stretch_span <= width, width + stretch_span - 1 <= 2048, audio_len >= width + 2 max_shift + stretch_span - 1, and
 *   16 (2 width + stretch_span - 1 + channels (width / 2 + 1)) + 4 channels (width + stretch_span - 1) bytes of LDS
 *   <= 160 KiB; a span needs a window source.
 * Site 3, attention dropout (ofp_cnnrnn_train_stretch only): index = ((s heads + h) T + i) T + j over the softmax
 *   probabilities [n][heads][T][T]; the rule and the scale of site 0, with the same dropout_p.  In that trainer site 0
 *   indexes the conv features [n][C W] in front of the GRU.  ofp_rnn_train_stretch has it too.
 * Site 4, dropout between recurrent layers (ofp_rnn_train_stretch only): index = ((l n + s) T + t) H + j over the
 *   output [n][T][H] of layer l, for every layer but the last; the rule and the scale of site 0, with the same
 *   dropout_p; in the training forward and the backward, not in the validation forward.
 * ofp_*_train_random / ofp_*_loss_grads_random / ofp_*_train_random_workspace_bytes: the functions without
 *   `_random`, which they are with random = NULL, plus these options (ofp_*_loss_grads_random takes no window source).
 * ofp_*_train_stretch / ofp_*_train_stretch_workspace_bytes: the `_random` functions, which they are with
 *   stretch_span = 0, plus the span of site 2.
 * ofp_philox4x32: d_counters [n][4], d_keys [n][2] -> d_out [n][4].  ofp_dropout_mask: d_mask [n][F] of 0 and
 *   (float)(1 / (1 - p)).  ofp_shift_windows: d_shifts [n] (or NULL) and d_windows [n][channels][width], n =
 *   n_extractions * n_onsets.  ofp_stretch_windows: the same with stretch_span >= 2, and d_stretches [n] (or NULL).
 *   All four run the device code of the epoch graphs. */
typedef struct ofp_train_random {
    uint64_t seed;
    double dropout_p;
    int32_t epoch;          /* used where there is no control block */
    int32_t max_shift;
    int32_t n_extractions;  /* 0: no window source */
    int32_t audio_channels;
    const float* d_audio;
    int64_t audio_len;
    const int64_t* d_starts;
    int64_t n_onsets;
} ofp_train_random;
int64_t ofp_cnn_train_random_workspace_bytes(const ofp_cnn_config* cfg, int64_t n, int64_t n_val,
                                             const ofp_train_random* random);
int ofp_cnn_train_random(const ofp_cnn_config* cfg, int64_t n, const float* d_x, const float* d_y, int64_t n_val,
                         const float* d_x_val, const float* d_y_val, const float* d_rates, int32_t num_epochs,
                         int32_t min_epochs, int32_t patience, float* d_params, float* d_stats, float* d_train_loss,
                         float* d_val_loss, int32_t* h_epochs, void* d_ws, int64_t ws_bytes, void* stream,
                         const ofp_train_random* random);
int ofp_cnn_loss_grads_random(const ofp_cnn_config* cfg, int64_t n, const float* d_x, const float* d_y,
                              const float* d_params, float* d_loss, float* d_grads, void* d_ws, int64_t ws_bytes,
                              void* stream, const ofp_train_random* random);
int64_t ofp_cccnn_train_random_workspace_bytes(const ofp_cccnn_config* cfg, int64_t n, int64_t n_val,
                                               const ofp_train_random* random);
int ofp_cccnn_train_random(const ofp_cccnn_config* cfg, int64_t n, const float* d_x, const float* d_y, int64_t n_val,
                           const float* d_x_val, const float* d_y_val, const float* d_rates, int32_t num_epochs,
                           int32_t min_epochs, int32_t patience, float* d_params, float* d_train_loss,
                           float* d_val_loss, int32_t* h_epochs, void* d_ws, int64_t ws_bytes, void* stream,
                           const ofp_train_random* random);
int ofp_cccnn_loss_grads_random(const ofp_cccnn_config* cfg, int64_t n, const float* d_x, const float* d_y,
                                const float* d_params, float* d_loss, float* d_grads, void* d_ws, int64_t ws_bytes,
                                void* stream, const ofp_train_random* random);
int ofp_philox4x32(const uint32_t* d_counters, const uint32_t* d_keys, int64_t n, uint32_t* d_out, void* stream);
int ofp_dropout_mask(uint64_t seed, int32_t epoch, int64_t n, int32_t F, double p, float* d_mask, void* stream);
int ofp_shift_windows(uint64_t seed, int32_t epoch, const float* d_audio, int64_t audio_len, int32_t channels,
                      const int64_t* d_starts, int64_t n_onsets, int32_t n_extractions, int32_t max_shift,
                      int32_t width, int32_t* d_shifts, float* d_windows, void* stream);
int ofp_stretch_windows(uint64_t seed, int32_t epoch, const float* d_audio, int64_t audio_len, int32_t channels,
                        const int64_t* d_starts, int64_t n_onsets, int32_t n_extractions, int32_t max_shift,
                        int32_t stretch_span, int32_t width, int32_t* d_shifts, int32_t* d_stretches,
                        float* d_windows, void* stream);
int64_t ofp_cnn_train_stretch_workspace_bytes(const ofp_cnn_config* cfg, int64_t n, int64_t n_val,
                                              const ofp_train_random* random, int32_t stretch_span);
int ofp_cnn_train_stretch(const ofp_cnn_config* cfg, int64_t n, const float* d_x, const float* d_y, int64_t n_val,
                          const float* d_x_val, const float* d_y_val, const float* d_rates, int32_t num_epochs,
                          int32_t min_epochs, int32_t patience, float* d_params, float* d_stats, float* d_train_loss,
                          float* d_val_loss, int32_t* h_epochs, void* d_ws, int64_t ws_bytes, void* stream,
                          const ofp_train_random* random, int32_t stretch_span);
int64_t ofp_cccnn_train_stretch_workspace_bytes(const ofp_cccnn_config* cfg, int64_t n, int64_t n_val,
                                                const ofp_train_random* random, int32_t stretch_span);
int ofp_cccnn_train_stretch(const ofp_cccnn_config* cfg, int64_t n, const float* d_x, const float* d_y, int64_t n_val,
                            const float* d_x_val, const float* d_y_val, const float* d_rates, int32_t num_epochs,
                            int32_t min_epochs, int32_t patience, float* d_params, float* d_train_loss,
                            float* d_val_loss, int32_t* h_epochs, void* d_ws, int64_t ws_bytes, void* stream,
                            const ofp_train_random* random, int32_t stretch_span);

/* ---- training model.CNNRNN (model.py:310-440; csrc/ofp_cnnrnn_train.hip) -------------------------------------------
 * Network: the conv stack of ofp_cnn_config (`cnn`; its n_out and loss are the head's), the model's dropout on the
 *   conv features, a one-layer GRU (batch_first, biases, gate order r, z, n, h_0 = 0) that takes the last conv layer's
 *   C channels as T time steps and its W columns as features, self-attention of `heads` heads over the `hidden` wide
 *   output sequence with dropout on the softmax probabilities, the mean over time, out_proj, and a Linear to n_out
 *   values.  The recipe is ofp_cnn_train's (NAdam rows in d_rates [num_epochs][4], the validation loss always L1, the
 *   stop rule, one captured graph per epoch with the first epoch launched plainly, a created stream);
 *   OFP_CNNRNN_GRAPH=nodes launches the same chain without a graph.
 * Parameters are packed in state_dict order: the conv stack as for ofp_cnn_train, then rnn.weight_ih_l0 [3 hidden][W],
 *   weight_hh_l0 [3 hidden][hidden], bias_ih_l0, bias_hh_l0 [3 hidden], attention.in_proj_weight [3 hidden][hidden],
 *   in_proj_bias [3 hidden], out_proj.weight [hidden][hidden], out_proj.bias [hidden], fc.weight [n_out][hidden],
 *   fc.bias [n_out].  The running statistics as for ofp_cnn_train.
 * Limits (beyond them OFP_ERR_INVALID, or -1 from the size functions): those of ofp_cnn_train, hidden 1..128, heads
 *   1..8 dividing hidden, C <= 128 time steps.
 * Random stream (ofp_train_random): site 0 is the dropout on the conv features [n][C W], element s C W + f; site 3 the
 *   dropout on the attention's probabilities [n][heads][T][T], element ((s heads + h) T + i) T + j; both with dropout_p,
 *   word < (uint32)(dropout_p 2^32) drops, kept values are multiplied by (float)(1 / (1 - dropout_p)).  Neither is
 *   applied in the validation forward.  The window source (sites 1 and 2) is ofp_cnn_train_stretch's.
 * Sums: no atomics; every dot product and every sum over rows is fp64 in ascending order, rounded to fp32 once; the
 *   weight and bias gradients of a dense layer are summed over slabs of ofp_linear_backward_slab() rows and the slabs
 *   added in order.
 * ofp_cnnrnn_loss_grads_random: one training-mode forward and backward (no window source): d_loss [1], d_grads packed
 *   like the parameters; d_ws of ofp_cnnrnn_loss_grads_random_workspace_bytes (n_val = 0).
 * ofp_linear_backward: y = x w^T + b with d_x [rows][n_in], d_w [n_out][n_in], d_dy [rows][n_out] -> d_dx [rows][n_in]
 *   (unless NULL), d_dw [n_out][n_in], d_db [n_out].  rows 1..2^20, n_in and n_out 1..4096.
 * ofp_gru_train_forward: d_x [n][T][F] -> d_out [n][T][H] and d_gates [n][T][4 H] = r, z, n and W_hn h + b_hn of every
 *   step.  ofp_gru_train_backward: with those and d_dout [n][T][H] -> d_dx [n][T][F], d_dw_ih [3H][F], d_dw_hh [3H][H],
 *   d_db_ih, d_db_hh [3H].  n 1..1024, T 1..128, F 1..1024, H 1..128.
 * ofp_attention_mean_train_forward: d_h [n][T][E] -> d_qkv [n][T][3E] (the in-projection), d_probs [n][heads][T][T]
 *   (softmax, before dropout) and d_ctx [n][E] = attention(h, h, h) before out_proj, averaged over time; `random`
 *   (NULL: none) gives seed, epoch and dropout_p of site 3.  _backward: with those and d_dctx [n][E] -> d_dh [n][T][E],
 *   d_dw [3E][E], d_db [3E] of the in-projection.  n 1..1024, T 1..128, E 1..128, heads 1..8 dividing E.
 * ofp_attention_dropout_mask: d_mask [n][heads][T][T] of 0 and (float)(1 / (1 - p)), site 3. */
typedef struct ofp_cnnrnn_config {
    ofp_cnn_config cnn;
    int32_t hidden, heads;
} ofp_cnnrnn_config;
int32_t ofp_linear_backward_slab(void);
int64_t ofp_cnnrnn_train_stretch_workspace_bytes(const ofp_cnnrnn_config* cfg, int64_t n, int64_t n_val,
                                                 const ofp_train_random* random, int32_t stretch_span);
int ofp_cnnrnn_train_stretch(const ofp_cnnrnn_config* cfg, int64_t n, const float* d_x, const float* d_y,
                             int64_t n_val, const float* d_x_val, const float* d_y_val, const float* d_rates,
                             int32_t num_epochs, int32_t min_epochs, int32_t patience, float* d_params, float* d_stats,
                             float* d_train_loss, float* d_val_loss, int32_t* h_epochs, void* d_ws, int64_t ws_bytes,
                             void* stream, const ofp_train_random* random, int32_t stretch_span);
int64_t ofp_cnnrnn_loss_grads_random_workspace_bytes(const ofp_cnnrnn_config* cfg, int64_t n, int64_t n_val,
                                                     const ofp_train_random* random);
int ofp_cnnrnn_loss_grads_random(const ofp_cnnrnn_config* cfg, int64_t n, const float* d_x, const float* d_y,
                                 const float* d_params, float* d_loss, float* d_grads, void* d_ws, int64_t ws_bytes,
                                 void* stream, const ofp_train_random* random);
int64_t ofp_linear_backward_workspace_bytes(int64_t rows, int32_t n_in, int32_t n_out);
int ofp_linear_backward(const float* d_x, int64_t rows, int32_t n_in, const float* d_w, int32_t n_out,
                        const float* d_dy, float* d_dx, float* d_dw, float* d_db, void* d_ws, int64_t ws_bytes,
                        void* stream);
int64_t ofp_gru_train_forward_workspace_bytes(int64_t n, int32_t T, int32_t F, int32_t H);
int ofp_gru_train_forward(const float* d_x, int64_t n, int32_t T, int32_t F, int32_t H, const float* d_w_ih,
                          const float* d_w_hh, const float* d_b_ih, const float* d_b_hh, float* d_out, float* d_gates,
                          void* d_ws, int64_t ws_bytes, void* stream);
int64_t ofp_gru_train_backward_workspace_bytes(int64_t n, int32_t T, int32_t F, int32_t H);
int ofp_gru_train_backward(const float* d_x, int64_t n, int32_t T, int32_t F, int32_t H, const float* d_w_ih,
                           const float* d_w_hh, const float* d_out, const float* d_gates, const float* d_dout,
                           float* d_dx, float* d_dw_ih, float* d_dw_hh, float* d_db_ih, float* d_db_hh, void* d_ws,
                           int64_t ws_bytes, void* stream);
int64_t ofp_attention_mean_train_forward_workspace_bytes(int64_t n, int32_t T, int32_t E, int32_t heads);
int ofp_attention_mean_train_forward(const float* d_h, int64_t n, int32_t T, int32_t E, int32_t heads,
                                     const float* d_in_w, const float* d_in_b, const ofp_train_random* random,
                                     float* d_qkv, float* d_probs, float* d_ctx, void* d_ws, int64_t ws_bytes,
                                     void* stream);
int64_t ofp_attention_mean_train_backward_workspace_bytes(int64_t n, int32_t T, int32_t E, int32_t heads);
int ofp_attention_mean_train_backward(const float* d_h, int64_t n, int32_t T, int32_t E, int32_t heads,
                                      const float* d_in_w, const float* d_qkv, const float* d_probs,
                                      const float* d_dctx, const ofp_train_random* random, float* d_dh, float* d_dw,
                                      float* d_db, void* d_ws, int64_t ws_bytes, void* stream);
int ofp_attention_dropout_mask(uint64_t seed, int32_t epoch, int64_t n, int32_t heads, int32_t T, double p,
                               float* d_mask, void* stream);

/* ---- training model.RNN (model.py:168-307; csrc/ofp_rnn_train.hip) ------------------------------------------------
 * Network: `layers` unidirectional GRU layers (batch_first, biases, gate order r, z, n, h_0 = 0) over the window
 *   itself -- `width` time steps of `channels` features, read in place from d_x [n][channels][width] (permute_input
 *   != 0) or [n][width][channels] (permute_input == 0) --, nn.GRU's dropout on the output of every layer but the last,
 *   LayerNorm(hidden, eps = ln_eps), self-attention of `heads` heads with dropout on the softmax probabilities, the mean
 *   over time, out_proj, and a Linear to n_out values.  The recipe is ofp_cnn_train's (rows in d_rates
 *   [num_epochs][4], the validation loss always L1, the stop rule, one captured graph per epoch with the first epoch
 *   launched plainly, a created stream) with one difference: NAdam has torch's coupled weight decay, the gradient that
 *   enters the moments and the step is g + weight_decay p.  OFP_RNN_GRAPH=nodes launches the same chain without a
 *   graph.  There are no running statistics, so no d_stats.
 * Parameters are packed in state_dict order: per layer l rnn.weight_ih_l [3 hidden][channels, or hidden for l > 0],
 *   weight_hh_l [3 hidden][hidden], bias_ih_l, bias_hh_l [3 hidden]; layer_norm.weight, layer_norm.bias [hidden];
 *   attention.in_proj_weight [3 hidden][hidden], in_proj_bias [3 hidden], out_proj.weight [hidden][hidden],
 *   out_proj.bias [hidden]; fc.weight [n_out][hidden], fc.bias [n_out].
 * Limits (beyond them OFP_ERR_INVALID, or -1 from the size functions): n and n_val 1..1024 (n_val from 0), channels
 *   1..8, width 1..512, hidden 1..128, layers 1..4, heads 1..8 dividing hidden, n_out 1..16; n heads width^2 and
 *   (layers - 1) n width hidden below 2^32, because the random stream indexes elements with 32 bits; a window source
 *   needs permute_input.
 * Random stream (ofp_train_random), both sites with dropout_p, the rule and the scale of site 0: site 3 is the dropout
 *   on the attention's probabilities [n][heads][T][T], element ((s heads + h) T + i) T + j.
 * Site 4, the dropout between recurrent layers (ofp_rnn_train_stretch only): index = ((l n + s) T + t) hidden + j over
 *   the output of layer l < layers - 1, [layers - 1][n][T][hidden]; applied in the training forward and in the
 *   backward, absent from the validation forward.  The window source (sites 1 and 2) is ofp_cnn_train_stretch's.
 * Sums: as for ofp_cnnrnn_train_stretch; the sums over a LayerNorm row are a butterfly over the 64 lanes of a wave,
 *   d gamma / d beta and the input projection's weight gradient go through fp64 slabs added in slab order.
 * ofp_rnn_loss_grads_random: one training-mode forward and backward (no window source): d_loss [1], d_grads packed
 *   like the parameters; d_ws of ofp_rnn_loss_grads_random_workspace_bytes (n_val = 0).
 * ofp_layernorm_train_forward: d_x [rows][E] -> d_y, and d_mean, d_rstd [rows] (1 / sqrt(biased variance + eps)).
 *   _backward: with those and d_dy [rows][E] -> d_dx [rows][E], d_dgamma, d_dbeta [E].  rows 1..2^20, E 1..128.
 * ofp_rnn_gru_train_forward: the GRU stack alone.  d_x [n][T][F] (permuted == 0) or [n][F][T] (permuted != 0), d_params
 *   the stack's parameters packed as above, `random` (NULL: none) seed, epoch and dropout_p of site 4 -> d_seqs
 *   [L][n][T][H], every layer's output before its dropout, and d_gates [L][n][T][4 H] as ofp_gru_train_forward keeps
 *   them.  _backward: with those and d_dseq [n][T][H], the gradient at the last layer's output -> d_grads packed like
 *   d_params (the window gets no gradient).  n 1..1024, T 1..512, F 1..8, H 1..128, L 1..4.
 * ofp_rnn_attention_train_forward / _backward: ofp_attention_mean_train_forward / _backward with T 1..512.
 * ofp_rnn_layer_dropout_mask: d_mask [layers][n][T][H] of 0 and (float)(1 / (1 - p)), site 4; `layers` counts the
 *   layers that have a dropout, the network's less one.
 * ofp_nadam_decay_step: ofp_nadam_step with the gradient g + weight_decay p. */
typedef struct ofp_rnn_config {
    int32_t channels, width, hidden, layers, heads, n_out, loss, permute_input;
    float weight_decay;
    double ln_eps;
} ofp_rnn_config;
int64_t ofp_rnn_train_stretch_workspace_bytes(const ofp_rnn_config* cfg, int64_t n, int64_t n_val,
                                              const ofp_train_random* random, int32_t stretch_span);
int ofp_rnn_train_stretch(const ofp_rnn_config* cfg, int64_t n, const float* d_x, const float* d_y, int64_t n_val,
                          const float* d_x_val, const float* d_y_val, const float* d_rates, int32_t num_epochs,
                          int32_t min_epochs, int32_t patience, float* d_params, float* d_train_loss,
                          float* d_val_loss, int32_t* h_epochs, void* d_ws, int64_t ws_bytes, void* stream,
                          const ofp_train_random* random, int32_t stretch_span);
int64_t ofp_rnn_loss_grads_random_workspace_bytes(const ofp_rnn_config* cfg, int64_t n, int64_t n_val,
                                                  const ofp_train_random* random);
int ofp_rnn_loss_grads_random(const ofp_rnn_config* cfg, int64_t n, const float* d_x, const float* d_y,
                              const float* d_params, float* d_loss, float* d_grads, void* d_ws, int64_t ws_bytes,
                              void* stream, const ofp_train_random* random);
int ofp_layernorm_train_forward(const float* d_x, int64_t rows, int32_t E, const float* d_gamma, const float* d_beta,
                                double eps, float* d_y, float* d_mean, float* d_rstd, void* stream);
int64_t ofp_layernorm_train_backward_workspace_bytes(int64_t rows, int32_t E);
int ofp_layernorm_train_backward(const float* d_x, int64_t rows, int32_t E, const float* d_gamma, const float* d_mean,
                                 const float* d_rstd, const float* d_dy, float* d_dx, float* d_dgamma, float* d_dbeta,
                                 void* d_ws, int64_t ws_bytes, void* stream);
int64_t ofp_rnn_gru_train_forward_workspace_bytes(int64_t n, int32_t T, int32_t F, int32_t H, int32_t L);
int ofp_rnn_gru_train_forward(const float* d_x, int32_t permuted, int64_t n, int32_t T, int32_t F, int32_t H, int32_t L,
                              const float* d_params, const ofp_train_random* random, float* d_seqs, float* d_gates,
                              void* d_ws, int64_t ws_bytes, void* stream);
int64_t ofp_rnn_gru_train_backward_workspace_bytes(int64_t n, int32_t T, int32_t F, int32_t H, int32_t L);
int ofp_rnn_gru_train_backward(const float* d_x, int32_t permuted, int64_t n, int32_t T, int32_t F, int32_t H, int32_t L,
                               const float* d_params, const ofp_train_random* random, const float* d_seqs,
                               const float* d_gates, const float* d_dseq, float* d_grads, void* d_ws, int64_t ws_bytes,
                               void* stream);
int64_t ofp_rnn_attention_train_forward_workspace_bytes(int64_t n, int32_t T, int32_t E, int32_t heads);
int ofp_rnn_attention_train_forward(const float* d_h, int64_t n, int32_t T, int32_t E, int32_t heads,
                                    const float* d_in_w, const float* d_in_b, const ofp_train_random* random,
                                    float* d_qkv, float* d_probs, float* d_ctx, void* d_ws, int64_t ws_bytes,
                                    void* stream);
int64_t ofp_rnn_attention_train_backward_workspace_bytes(int64_t n, int32_t T, int32_t E, int32_t heads);
int ofp_rnn_attention_train_backward(const float* d_h, int64_t n, int32_t T, int32_t E, int32_t heads,
                                     const float* d_in_w, const float* d_qkv, const float* d_probs,
                                     const float* d_dctx, const ofp_train_random* random, float* d_dh, float* d_dw,
                                     float* d_db, void* d_ws, int64_t ws_bytes, void* stream);
int ofp_rnn_layer_dropout_mask(uint64_t seed, int32_t epoch, int32_t layers, int64_t n, int32_t T, int32_t H, double p,
                               float* d_mask, void* stream);
int ofp_nadam_decay_step(float* d_p, const float* d_g, float* d_m, float* d_v, int64_t n, const float* d_row,
                         float weight_decay, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ONSETFP_H */
