// call_policy.hpp -- what the C ABI host (esac_capi.hip) DECIDES from a caller's parameters, before and beside any HIP call: the
// argument checks with their status codes and messages, the implied flags and defaults, the score / pack routes, the training
// path's sizing, the forward team latch and the size table of esac_hip_read.  Plain C++ over include/esac_hip.h (no HIP header):
// the CPU suite reads it through tests/native/call_policy_probe.cpp.  Values that only a kernel translation unit defines
// (tiled_sub_tiles(P), corr_entries(P), bwd_rows(N), refine_slots_can_team, refine_folds_select) come in as plain arguments.
#pragma once
#include <float.h>
#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../include/esac_hip.h"

namespace esac {

// mirrors of esac_kernels.hpp (checked by static_assert in esac_capi.hip)
constexpr int POLICY_TILED_HC = 256, POLICY_TILED_MAX_EXPERTS = 4096, POLICY_LDS_CAP = 8192, POLICY_SAMPLE_LIST_PER_HYP = 16;
constexpr int ESAC_SLOT_TEAMS_MAX = 32;  // training path: slots refined by teams when the call selects at most this many
constexpr int ESAC_TEAM_STRIKES = 2;
constexpr long long ESAC_TEAM_REARM_CALLS = 1000;

// the error channel of every entry point: a negative status + the message esac_hip_last_error returns
inline thread_local char g_err[512] = "";
inline int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

// One camera's checks (cam_frame >= 0: a record of a per-frame table, the error names the frame)
// (H, W: the grid the camera looks at -- p's own, or the frame's in a ragged batch)
inline int check_cam(const esac_hip_params* p, int shift_x, int shift_y, float focal, int cam_frame, int H, int W) {
    char where[32] = "";
    if (cam_frame >= 0) snprintf(where, sizeof(where), " in frame %d", cam_frame);
    // pixel centres col*sub + sub/2 - shift (esac_util.h:64-66) are formed in int32 on the device
    const int64_t lim = 0x7fffffffLL, half = p->sub_sampling / 2;
    const int64_t xs[4] = {half - shift_x, (int64_t)(W - 1) * p->sub_sampling + half - shift_x, half - shift_y, (int64_t)(H - 1) * p->sub_sampling + half - shift_y};
    for (int64_t v : xs)
        if (v > lim || v < -lim) return fail(-4, "pixel positions overflow int32 (subSampling=%d, shift=(%d,%d))%s", p->sub_sampling, shift_x, shift_y, where);
    if (!(focal > 0)) return fail(-4, "focal length must be positive%s", where);
    return 0;
}
inline int check_cam(const esac_hip_params* p, int shift_x, int shift_y, float focal, int cam_frame) {
    return check_cam(p, shift_x, shift_y, focal, cam_frame, p->H, p->W);
}
// The grid-size rule of a call, and of every frame of a ragged batch (frame >= 0: the error names it)
inline int check_grid(int H, int W, int frame) {
    char where[32] = "";
    if (frame >= 0) snprintf(where, sizeof(where), " in frame %d", frame);
    if (H < 3 || W < 3 || (int64_t)(H - 1) * (W - 1) < 4)
        return fail(-4, "grid %dx%d too small: 4 distinct cells must exist in [0,W-2]x[0,H-2] (esac_util.h:164-176)%s", H, W, where);
    if ((int64_t)H * W > (int64_t)1 << 28 || H > 65535 || W > 65535)
        return fail(-4, "grid %dx%d too large (at most 65535 rows / columns, 2^28 cells)%s", H, W, where);
    return 0;
}
// Validation of a call's parameters: what the reference leaves to accessor<>() / OpenCV asserts.  ctx, tensors: the context /
// both of the coordinate and assignment pointers are there.
// training: the call is one of esac_hip_backward* (the only entry points that honour ESAC_FLAG_STRICT_TRAINING)
inline int check_args(bool ctx, bool tensors, const esac_hip_params* p, int B, int cam_frame, bool training) {
    if (!ctx) return fail(-1, "null context");
    if (!p) return fail(-1, "null params");
    if (!tensors) return fail(-1, "null scene-coordinate or assignment pointer");
    if (p->E <= 0 || p->N <= 0) return fail(-4, "E=%d, N=%d must be positive", p->E, p->N);
    if (int rc_grid = check_grid(p->H, p->W, -1)) return rc_grid;
    if (p->sub_sampling <= 0) return fail(-4, "subSampling=%d must be positive", p->sub_sampling);
    if ((p->flags & ESAC_FLAG_STRICT_REFERENCE) && (p->flags & (ESAC_FLAG_SCORE_TILED | ESAC_FLAG_SCORE_STREAM | ESAC_FLAG_AUTO_EXACT)))
        return fail(-4, "ESAC_FLAG_STRICT_REFERENCE cannot be combined with ESAC_FLAG_SCORE_TILED, ESAC_FLAG_SCORE_STREAM or ESAC_FLAG_AUTO_EXACT "
                        "(flags=%d): strict mode scores every hypothesis in reference arithmetic", p->flags);
    if (p->flags & ESAC_FLAG_STRICT_TRAINING) {
        if (p->flags & ESAC_FLAG_STRICT_REFERENCE)
            return fail(-4, "ESAC_FLAG_STRICT_TRAINING cannot be combined with ESAC_FLAG_STRICT_REFERENCE (flags=%d): one is the training "
                            "path's strict mode, the other the forward path's", p->flags);
        if (!training)
            return fail(-4, "ESAC_FLAG_STRICT_TRAINING is a flag of esac_hip_backward, esac_hip_backward_batch and esac_hip_backward_batch_cams "
                            "(flags=%d): the forward path's strict mode is ESAC_FLAG_STRICT_REFERENCE", p->flags);
    }
    if (int rc_cam = check_cam(p, p->shift_x, p->shift_y, p->focal, cam_frame)) return rc_cam;
    if (B < 1 || B > ESAC_MAX_BATCH) return fail(-4, "batch size %d outside [1,%d]", B, ESAC_MAX_BATCH);
    return 0;
}
// The scalar fields of a call's argument block that are derived from its parameters (cap_n: hypotheses the workspace holds)
struct CallScalars {
    int max_tries, max_ref_steps, samp_cap, flags;
    float margin;
};
// band of the fp32 maximum that is re-scored exactly: the stream's rounding (<= 2e-5 * alpha measured) plus two
// cells' weight -- an ill-conditioned projection (scene point next to the camera centre) can put a cell on the other
// side of tau under fp32, which moves a score by alpha / (H*W); on small grids that exceeds alpha * 1e-3.
// (cells: the grid the score is summed over -- a frame's own in a ragged batch, never the capacity's: the band of a small
// frame is wider than the capacity's)
inline float rescore_margin(const esac_hip_params* p, int cells) {
    return p->rescore_margin > 0 ? p->rescore_margin : fabsf(p->inlier_alpha) * (ESAC_DEFAULT_MARGIN + 2.0f / (float)cells);
}
inline CallScalars call_scalars(const esac_hip_params* p, long long cap_n) {
    CallScalars v;
    v.max_tries = p->max_tries > 0 ? p->max_tries : ESAC_MAX_SAMPLING_TRIES;
    v.max_ref_steps = p->max_ref_steps >= 0 ? (p->max_ref_steps < ESAC_MAX_REF_STEPS ? p->max_ref_steps : ESAC_MAX_REF_STEPS)
                                            : ESAC_MAX_REF_STEPS;
    v.samp_cap = (int)((cap_n * POLICY_SAMPLE_LIST_PER_HYP) > 0x7fffffffLL ? 0x7fffffff : cap_n * POLICY_SAMPLE_LIST_PER_HYP);
    v.flags = p->flags;
    if (v.flags & ESAC_FLAG_STRICT_REFERENCE) v.flags |= ESAC_FLAG_EXACT_SCORES | ESAC_FLAG_EXACT_SAMPLING;  // (implied)
    // the training path's strict mode: the strict bit the samplers, k_rescore_strict and trial_rejected read, and the two exact routes
    if (v.flags & ESAC_FLAG_STRICT_TRAINING) v.flags |= ESAC_FLAG_STRICT_REFERENCE | ESAC_FLAG_EXACT_SCORES | ESAC_FLAG_EXACT_SAMPLING;
    v.margin = rescore_margin(p, p->H * p->W);
    return v;
}
// ESAC_FLAG_AUTO_EXACT: the guaranteed routes where they are free (include/esac_hip.h)
inline int auto_exact_flags(int flags, int B, int E, int N, int H, int W) {
    if ((flags & ESAC_FLAG_AUTO_EXACT) && B == 1 && E == 1 && (long long)N * H * W <= ESAC_AUTO_EXACT_MAX_WORK)
        flags |= ESAC_FLAG_EXACT_SCORES | ESAC_FLAG_EXACT_SAMPLING;
    return flags;
}
// Which shape the fp32 score runs in.  Per-hypothesis stream (k_score_fast): every hypothesis re-reads its expert's map,
// fine while a map is L2-resident and hypotheses are few.  Tile-stationary (esac_score_tiled.hip): each map tile is read
// once per chunk of <= 256 hypotheses -- pays when a map no longer fits the caches next to the other experts' maps
// (full-resolution 480x640 maps: 3.7 MB each) and enough hypotheses share it.  ESAC_FLAG_SCORE_TILED / _STREAM override.
// n_sub: tiled_sub_tiles(H * W)
inline bool want_tiled(const esac_hip_params* p, const void* d_sc, int B, int n_sub) {
    const long long P = (long long)p->H * p->W;
    const bool legal = B == 1 && (p->W & 3) == 0 && (reinterpret_cast<uintptr_t>(d_sc) & 15) == 0 && p->E <= POLICY_TILED_MAX_EXPERTS && P >= 4;
    const long long partial_bytes = (long long)n_sub * p->N * 4;
    if (!legal || partial_bytes > (4LL << 30) || (p->flags & ESAC_FLAG_SCORE_STREAM)) return false;
    // the tile kernel folds k = |beta| log2(e) into the pose rows and multiplies by 2^(-+k tau) after the exp2: beyond
    // k tau ~ 126 that constant under- / overflows (scores NaN or saturated); the stream keeps the subtraction in the
    // exponent and is right for any parameters
    if (!(fabsf(p->inlier_beta) * 1.4426950408889634f * fabsf(p->inlier_thresh) <= 100.0f)) return false;
    if (p->flags & ESAC_FLAG_SCORE_TILED) return true;
    return P >= 32768 && p->N >= 64;
}
inline int tiled_chunks(int N, int E) { return N / POLICY_TILED_HC + (E < N ? E : N) + 1; }  // chunks of <= 256 hypotheses of one expert
// Packed (x,y,z,0) copy of the maps for the sampler: worth one extra pass over the maps when they are far beyond the L2s
// (every random 4-byte gather would otherwise fetch its own cache line, three per cell) and hypotheses of several experts
// will need many tries.  Single frames only.
inline bool want_pack(const esac_hip_params* p, int B) {
    if (B != 1) return false;
    if (p->flags & ESAC_FLAG_PACK_MAPS) return true;
    return p->E > 1 && (long long)p->E * p->H * p->W * 12 >= (32LL << 20) && p->N >= 256;
}
// The forward path's team latch.  A team timed out: twice in a row and the context stops asking for teams (a caller that keeps
// the GPU's CUs busy on another stream would otherwise pay the time-out on every frame) until it is re-armed -- after
// ESAC_TEAM_REARM_CALLS forward calls, with one strike left, or by an explicit request (esac_hip_set_refine_team).  The latch is
// the FORWARD path's: the training path's slot teams have a switch of their own (esac_hip_ctx::team.slot_teams).
struct TeamLatch {
    int strikes = 0;           // consecutive forward calls whose team timed out (a call whose team held clears it)
    bool off = false;
    long long solo_since = 0;  // forward calls since the latch closed
    long long fallbacks = 0;   // team time-outs so far (ESAC_BUF_REFINE_INFO[6])
    void timed_out() {
        fallbacks++;
        if (++strikes >= ESAC_TEAM_STRIKES && !off) off = true, solo_since = 0;
    }
    void forward_call() {  // (blocking or not: every forward call counts) try a team again; one more time-out latches at once
        if (off && ++solo_since > ESAC_TEAM_REARM_CALLS) off = false, strikes = ESAC_TEAM_STRIKES - 1;
    }
    void requested() { off = false; strikes = 0; }
};
// The forward path's team request: off while the context is latched, and for ESAC_FLAG_REFINE_SOLO
inline void forward_team(const TeamLatch& latch, int flags, int* team, int* solo) {
    if (latch.off) *team = 0;
    if (flags & ESAC_FLAG_REFINE_SOLO) {
        *team = 0;
        *solo = 1;
    }
}
inline int check_refine_team(bool ctx, int members) {
    if (!ctx) return fail(-1, "null context");
    if (members < ESAC_REFINE_TEAM_AUTO || members > ESAC_REFINE_TEAM_MAX)
        return fail(-4, "esac_hip_set_refine_team: %d members (0..%d, or ESAC_REFINE_TEAM_AUTO)", members, ESAC_REFINE_TEAM_MAX);
    return 0;
}
// ESAC_REFINE_TEAM_AUTO: back to the default policy (the size chosen per grid); a number: exactly that many
inline int requested_team(int members) { return members == ESAC_REFINE_TEAM_AUTO ? ESAC_REFINE_TEAM_DEFAULT : members < 2 ? 0 : members; }
inline int check_wait(bool ctx, int mode) {
    if (!ctx) return fail(-1, "null context");
    if (mode != ESAC_WAIT_SPIN && mode != ESAC_WAIT_YIELD && mode != ESAC_WAIT_BLOCK) return fail(-4, "esac_hip_set_wait: unknown mode %d", mode);
    return 0;
}

// ---------------------------------------------------------------- training path
// Bytes of slot workspace one slot is CHARGED against the context's budget (ESAC_BWD_BATCH_BUDGET_MB): two inlier maps, the two
// 3P-double slabs, and the correspondence list at its true size corr_entries(P).  The batched calls size their chunks by this
// and nothing else.  It is less than ensure_bws allocates per slot: that rounds the list up to its bound P + 2048 entries and
// adds the slot's team granules (2 * ESAC_REFINE_TEAM_MAX * 32 granules of 16 bytes), and the per-frame tables (selection,
// probabilities, losses, poses, dloss, map_info: a few dozen bytes per hypothesis) are not charged at all.  The chunk sizes
// that tests and callers see under a given budget follow from this value, so it stays what it is.
inline long long bwd_slot_bytes(int P, long long corr_entries_P) {
    return 2LL * P + 2LL * 3 * P * (long long)sizeof(double) + (P > POLICY_LDS_CAP ? corr_entries_P * 16 : 0);
}
// The slot count a rerun after an overflow is sized by: the selection's true count in whole 32s, at most the worst case
inline int grown_cap(int needed, int worst) { return needed + 31 > worst ? worst : (needed + 31) / 32 * 32; }
// Slots per frame a training call starts with.  How many hypotheses reach PROB_THRESH is only known on the device: a blocking
// call starts from what earlier calls needed (`seen`, at least 64 slots) and reruns when the selection overflows it; an
// asynchronous call cannot look at the count and reserves the worst case min(N, 1000).
inline int start_cap(bool blocking, int seen, int worst) {
    if (!blocking) return worst;
    const int cap = seen > 64 ? seen : 64;
    return cap > worst ? worst : cap;
}
// Frames of a batch's next chunk: as many of the `left` as the budget holds at `cap` slots each, at least one
inline int chunk_frames(long long budget, int cap, long long slot_bytes, int left) {
    const long long f = budget / ((long long)cap * slot_bytes);
    return (int)(f < 1 ? 1 : (f > left ? left : f));
}
// ... of the asynchronous batch, whose chunking is known before anything is launched: cap is the worst case
inline int check_async_budget(long long budget, int cap, long long slot_bytes) {
    if (budget / ((long long)cap * slot_bytes) < 1)
        return fail(-4, "esac_hip_backward_batch_dev: one frame's worst case (%d slots, %lld MiB) exceeds the slot-workspace budget of "
                        "%lld MiB (ESAC_BWD_BATCH_BUDGET_MB); the blocking esac_hip_backward_batch sizes the workspace by the "
                        "selection's true count", cap, ((long long)cap * slot_bytes) >> 20, budget >> 20);
    return 0;
}

// The checks of the two batched entry points, before either touches the device.  Both report under `who` (the asynchronous call
// under the blocking call's name too: its callers match these messages); what they differ in is the result pointer -- `out` is
// host memory of the blocking call (async == false) and device memory of the asynchronous one, each with its own message and
// its own place in the order.
inline int check_batch_call(const char* who, bool ctx, const esac_hip_params* p, int B, bool tensors, bool async, bool out, int64_t sc_frame_stride, int64_t grad_frame_stride) {
    if (!ctx) return fail(-1, "null context");
    if (!p) return fail(-1, "null params");
    if (!tensors) return fail(-1, "%s: null coordinate, gradient, assignment or ground-truth pointer", who);
    if (async && !out) return fail(-1, "esac_hip_backward_batch_dev: d_out (device double[B,4]) is required");
    if (p->flags & ESAC_FLAG_STRICT_REFERENCE)
        return fail(-4, "%s: the training path has no strict mode (ESAC_FLAG_STRICT_REFERENCE is a forward flag)", who);
    if (!async && !out) return fail(-4, "%s: the batched call is blocking only: h_out (host double[B,4]) is required", who);
    if (B < 1 || B > ESAC_MAX_BATCH) return fail(-4, "%s: batch size %d outside [1,%d]", who, B, ESAC_MAX_BATCH);
    if (p->d_hyp_index || p->hyp_offset)
        return fail(-4, "%s: sharded calls are not supported (the expectation needs every hypothesis)", who);
    if (p->E > 65535) return fail(-4, "%s: at most 65535 experts (one grid row per expert in the accumulation kernel)", who);
    if (p->E <= 0 || p->H <= 0 || p->W <= 0 || p->N <= 0) return fail(-4, "E=%d, H=%d, W=%d, N=%d must be positive", p->E, p->H, p->W, p->N);
    const long long slab = (long long)p->E * 3 * p->H * p->W;
    if (sc_frame_stride < 0) return fail(-4, "%s: negative coordinate frame stride", who);
    if (B > 1 && grad_frame_stride < slab)
        return fail(-4, "%s: gradient frame stride %lld < E*3*H*W = %lld (frames would share gradients)", who, (long long)grad_frame_stride, slab);
    return 0;
}
// esac_hip_set_bwd_pose_records armed `frames` records (armed: with a buffer) for a call of B frames
inline int check_pose_arm(const char* who, bool armed, int frames, int B) {
    if (armed && frames < B) return fail(-4, "%s: esac_hip_set_bwd_pose_records armed %d frame(s), the call has %d", who, frames, B);
    return 0;
}
// esac_hip_backward's own checks: in front of check_args, and behind it
inline int check_backward_entry(bool tensors, bool ctx, const esac_hip_params* p) {
    if (!tensors) return fail(-1, "esac_hip_backward: null gradient tensor or ground-truth pose");
    if (!ctx) return fail(-1, "null context");
    if (p && (p->flags & ESAC_FLAG_STRICT_REFERENCE))
        return fail(-4, "esac_hip_backward: the training path has no strict mode (ESAC_FLAG_STRICT_REFERENCE is a forward flag)");
    return 0;
}
inline int check_backward_call(const esac_hip_params* p) {
    if (p->E > 65535) return fail(-4, "esac_hip_backward: at most 65535 experts (one grid row per expert in the accumulation kernel)");
    if (p->d_hyp_index || p->hyp_offset)
        return fail(-4, "esac_hip_backward: sharded calls are not supported (the expectation needs every hypothesis)");
    return 0;
}
inline int check_eval_batch(bool ctx, int B, bool records, bool gt_poses, bool out, float rot_thresh_deg, float trans_thresh_cm) {
    if (!ctx) return fail(-1, "null context");
    if (B < 1 || B > ESAC_MAX_BATCH) return fail(-4, "esac_hip_eval_batch: batch size %d outside [1,%d]", B, ESAC_MAX_BATCH);
    if (!records || !gt_poses || !out)
        return fail(-4, "esac_hip_eval_batch: null %s pointer", !records ? "d_records" : !gt_poses ? "d_gt_poses" : "d_out");
    if (!(rot_thresh_deg >= 0.0f) || !(rot_thresh_deg <= FLT_MAX) || !(trans_thresh_cm >= 0.0f) || !(trans_thresh_cm <= FLT_MAX))
        return fail(-4, "esac_hip_eval_batch: the thresholds must be finite and not negative (rotation %g deg, translation %g cm)", (double)rot_thresh_deg, (double)trans_thresh_cm);
    return 0;
}
inline int check_shard_balanced(bool pointers, int N, int E, int world, int rank) {
    if (!pointers) return fail(-1, "esac_hip_shard_balanced: null argument");
    if (N <= 0 || E <= 0 || E > POLICY_TILED_MAX_EXPERTS) return fail(-4, "esac_hip_shard_balanced: N=%d, E=%d (1 <= E <= %d)", N, E, POLICY_TILED_MAX_EXPERTS);
    if (world < 1 || rank < 0 || rank >= world) return fail(-4, "esac_hip_shard_balanced: rank %d of %d", rank, world);
    return 0;
}

// ---------------------------------------------------------------- esac_hip_read
// After a batched call the per-frame buffers hold its (last chunk's) frames frame-major: B x the single-frame size reads them all
enum ReadFrames { READ_ONE, READ_FWD_FRAMES, READ_BWD_FRAMES };
// X(buffer id, the workspace member in esac_capi.hip, bytes per element, elements from (N, P, rows), which frames)
#define ESAC_READ_TABLE(X)                                                                    \
    X(ESAC_BUF_HYPS, ws.hyps, 8, N * 6, READ_FWD_FRAMES)                                      \
    X(ESAC_BUF_SAMPLE_XY, ws.sample_xy, 4, N * 8, READ_FWD_FRAMES)                            \
    X(ESAC_BUF_TRIES, ws.tries, 4, N, READ_FWD_FRAMES)                                        \
    X(ESAC_BUF_SCORES, ws.scores, 8, N, READ_FWD_FRAMES)                                      \
    X(ESAC_BUF_RESULT, ws.result, 8, ESAC_RES_DOUBLES, READ_ONE)                              \
    X(ESAC_BUF_INLIER_COUNTS, ws.inlier_counts, 4, ESAC_MAX_REF_STEPS + 1, READ_FWD_FRAMES)   \
    X(ESAC_BUF_WINNER_ERRS, ws.errs, 4, P, READ_ONE)                                          \
    X(ESAC_BUF_EXACT_FLAGS, ws.exact_flag, 1, N, READ_ONE)                                    \
    X(ESAC_BUF_SPEC_FLAGS, ws.spec_flag, 1, N, READ_ONE)                                      \
    X(ESAC_BUF_CYCLES, ws.cycles, 8, 32, READ_ONE)                                            \
    X(ESAC_BUF_BWD_PROBS, train.ws.probs, 8, N, READ_BWD_FRAMES)                                   \
    X(ESAC_BUF_BWD_LOSSES, train.ws.losses, 8, N, READ_BWD_FRAMES)                                 \
    X(ESAC_BUF_BWD_REF_HYPS, train.ws.ref_hyps, 8, N * 6, READ_BWD_FRAMES)                         \
    X(ESAC_BUF_BWD_SCORE_GRADS, train.ws.sgrad, 8, N, READ_BWD_FRAMES)                             \
    X(ESAC_BUF_BWD_SLOTS, train.ws.sel, 4, N, READ_BWD_FRAMES)                                     \
    X(ESAC_BUF_BWD_SLOT_INFO, train.ws.map_info, 4, rows * 4, READ_BWD_FRAMES)                     \
    X(ESAC_BUF_BWD_DLOSS, train.ws.dloss, 8, rows * 6, READ_BWD_FRAMES)
// What the context holds when esac_hip_read is called: the shape of the most recent call (rows: bwd_rows(N)), the frames of the
// most recent forward / training launch set, the slots the slab workspace holds per frame, esac_hip_set_debug's error image
struct ReadDims {
    size_t N, P, rows;
    int fwd_frames, bwd_frames;
    size_t slot_cap;
    bool keep_errs;
};
// The bytes a read of buffer `which` moves (*want), or why the caller's `bytes` are refused (have_src: the buffer exists).  The
// inlier map, the three info words, the slabs and the maps are then served by code of their own in esac_hip_read.
inline int read_size(int which, size_t bytes, bool have_src, const ReadDims& d, size_t* want) {
    const size_t N = d.N, P = d.P, rows = d.rows;
    int frames = READ_ONE;
    *want = 0;
    switch (which) {
#define ESAC_READ_ROW(id, member, elem, count, fr) case id: *want = (size_t)(count) * (elem); frames = fr; break;
        ESAC_READ_TABLE(ESAC_READ_ROW)
#undef ESAC_READ_ROW
        case ESAC_BUF_INLIER_MAP:
            if (bytes != P) return fail(-7, "esac_hip_read: inlier map holds %zu bytes, caller asked for %zu", P, bytes);
            *want = P;
            return 0;
        case ESAC_BUF_BWD_TEAM_INFO:
        case ESAC_BUF_SPEC_INFO:
        case ESAC_BUF_REFINE_INFO: {  // int32 words of the context's own
            const bool refine = which == ESAC_BUF_REFINE_INFO;
            *want = (refine ? 8 : 4) * sizeof(int32_t);
            if (bytes != *want)
                return fail(-7, "esac_hip_read: the %s info holds %zu bytes, caller asked for %zu", refine ? "refinement" : which == ESAC_BUF_SPEC_INFO ? "speculation" : "slot-team", *want, bytes);
            if (refine && !have_src) return fail(-6, "esac_hip_read: buffer %d is empty (no call has run yet)", which);
            return 0;
        }
        case ESAC_BUF_BWD_PATH1:
        case ESAC_BUF_BWD_PATH2:
        case ESAC_BUF_BWD_MAPS: {
            // [slots,3,P] doubles / [slots,2,P] bytes (both map buffers of each slot); the caller asks for the first k slots
            // (k = bytes / unit) of the slots the workspace holds (>= the slots of the last call); after a batch, frame 0's
            const bool maps = which == ESAC_BUF_BWD_MAPS;
            const size_t unit = maps ? 2 * P : 3 * P * sizeof(double);
            if (!have_src || unit == 0) return fail(-6, "esac_hip_read: buffer %d is empty (no backward call has run yet)", which);
            if (bytes == 0 || bytes % unit || bytes / unit > d.slot_cap)
                return fail(-7, "esac_hip_read: buffer %d is read in whole %s of %zu bytes, at most %zu", which, maps ? "slots" : "slabs", unit, d.slot_cap);
            *want = bytes;
            return 0;
        }
        default: return fail(-5, "esac_hip_read: unknown buffer id %d", which);
    }
    if (which == ESAC_BUF_WINNER_ERRS && !d.keep_errs)
        return fail(-6, "esac_hip_read: the error image is only kept after esac_hip_set_debug(ctx, ESAC_DEBUG_ERROR_IMAGE)");
    const int B = frames == READ_BWD_FRAMES ? d.bwd_frames : frames == READ_FWD_FRAMES ? d.fwd_frames : 1;
    if (B > 1 && *want > 0 && bytes == *want * (size_t)B) *want = bytes;
    if (!have_src || *want == 0) return fail(-6, "esac_hip_read: buffer %d is empty (no call has run yet)", which);
    if (bytes != *want) return fail(-7, "esac_hip_read: buffer %d holds %zu bytes, caller asked for %zu", which, *want, bytes);
    return 0;
}

}  // namespace esac

#include "ragged_policy.hpp"  // check_shapes, shape_record: the ragged batch (esac_hip_forward_batch_shapes)
