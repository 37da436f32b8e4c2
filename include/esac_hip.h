/*
 * esac_hip.h -- C ABI of the MI355X-native ESAC hypothesis/inlier hot path.
 *
 * This is the drop-in boundary: a plain-C shared library (libesac_hip.so) with
 * no torch / pybind types in any signature.  It replaces what the reference
 * binds through pybind11 in code/esac/esac.cpp:513-516
 *     m.def("forward",  &esac_forward)   // esac.cpp:64-190
 *     m.def("backward", &esac_backward)  // esac.cpp:213-511 -> esac_hip_backward
 * The Python module `esac` (esac.py -> esac_amd/api.py) binds these entry points
 * with ctypes and keeps the reference's positional `esac.forward(...)` signature;
 * INTEGRATION.md shows the binding a reference maintainer would add.
 *
 * Conventions
 *   - every function returns 0 on success, <0 on error; esac_hip_last_error()
 *     returns a thread-local message (the Python layer raises RuntimeError,
 *     the exception type pybind11 turns the reference's c10::Error into).
 *   - pointers named d_* are DEVICE pointers on the context's GPU, h_* are HOST.
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream).
 *   - tensors are dense row-major: scene coordinates [E,3,H,W] float32
 *     (esac_types.h:45 coord_t), hypothesis assignment [N] int64
 *     (esac_types.h:46 hyp_assign_t).
 *   - there is NO CPU fallback: without a HIP device every call fails.
 */
#ifndef ESAC_HIP_H
#define ESAC_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ESAC_HIP_ABI_VERSION 6

/* reference compile-time constants (esac.cpp:44-45) */
#define ESAC_MAX_SAMPLING_TRIES 1000000
#define ESAC_MAX_REF_STEPS 100
#define ESAC_MAX_BATCH 1024 /* frames per esac_hip_forward_batch call */

/* Scalar arguments of esac_forward (esac.cpp:64-77) plus the knobs the
 * reference hard-codes or hides (RNG key, limits, multi-GPU shard offset). */
typedef struct esac_hip_params {
    int32_t E, H, W;          /* sceneCoordinates.size(0,2,3)  esac.cpp:87-88      */
    int32_t N;                /* hypAssignment.size(0)         esac.cpp:90         */
    int32_t shift_x, shift_y; /* esac.cpp:67-68                                    */
    float focal, ppx, ppy;    /* esac.cpp:69-71; camMat is float, esac.cpp:93-97   */
    float inlier_thresh;      /* tau,   esac.cpp:72                                */
    float inlier_alpha;       /* alpha, esac.cpp:73                                */
    float inlier_beta;        /* beta,  esac.cpp:74                                */
    float max_reproj;         /* esac.cpp:75                                       */
    int32_t sub_sampling;     /* esac.cpp:76                                       */
    uint64_t seed;            /* RNG key; reference: fixed 1305, thread_rand.h:103 */
    uint64_t call;            /* call counter (reference RNG state persists across calls) */
    int32_t max_tries;        /* <=0 -> ESAC_MAX_SAMPLING_TRIES                    */
    int32_t max_ref_steps;    /* <0  -> ESAC_MAX_REF_STEPS                         */
    int32_t hyp_offset;       /* global index of local hypothesis 0 (multi-GPU sharding; RNG and
                                 tie-breaks use global indices so results do not depend on the
                                 number of ranks) */
    float rescore_margin;     /* fast-score band re-scored exactly; <=0 -> alpha*(ESAC_DEFAULT_MARGIN + 2/(H*W)) */
    const int32_t* d_hyp_index; /* optional DEVICE int32[N]: global index of each local hypothesis, for
                                 shards that are not a contiguous range (expert-sharded multi-GPU);
                                 NULL -> hyp_offset + i */
    int32_t flags;            /* ESAC_FLAG_* below, 0 = default */
    int32_t expert_base;      /* added to the winner's (local) expert index in ESAC_RES_EXPERT: a rank that holds only a
                                 slice of the experts' maps (multi-GPU, esac_hip_shard_balanced) passes the global id of
                                 its first map so that the record carries what esac.cpp:189 returns; 0 otherwise */
} esac_hip_params;

/* One frame's camera in a batch whose frames differ in shift, focal length or principal point (esac_hip_forward_batch_cams,
 * esac_hip_backward_batch_cams): the five per-image values of esac_hip_params, padded to 32 bytes (one aligned record per frame
 * on the device).  The padding is ignored by the _cams entry points (it may hold anything); esac_hip_forward_batch_shapes reads
 * the frame's grid from it. */
typedef struct esac_hip_frame_cam {
    int32_t shift_x, shift_y; /* esac.cpp:67-68: the image's random shift (training) or 0 */
    float focal, ppx, ppy;    /* esac.cpp:69-71 */
    int32_t reserved[3];      /* esac_hip_forward_batch_shapes, esac_hip_backward_batch_shapes, _dev_shapes: [0] rows h, [1] columns w
                                 of the frame's grid; [2] ignored */
} esac_hip_frame_cam;

/* esac_hip_forward / _batch: score EVERY hypothesis in the reference's mixed float/double arithmetic
 * (esac_util.h:235-260, 292-360) instead of ranking with the fp32 stream and re-scoring only the contenders.
 * The score vector, ESAC_RES_PROB and ESAC_RES_ENTROPY are then the reference's own values (softMax / entropy,
 * esac_util.h:461-497) for every hypothesis; the winner and the pose are the same either way. */
#define ESAC_FLAG_EXACT_SCORES 1
/* Shape of the fp32 ranking score (results are the same to fp32 rounding; default: chosen from grid size and N).
 * TILED: map tiles stationary in registers, hypotheses bucketed by expert stream past them (large maps);
 * STREAM: one hypothesis per workgroup streams its expert's whole map (small, cache-resident maps).
 * Both rank only.  One documented difference from the reference's projection (esac_util.h:302-305, `z ? 1/z : 1`): a cell
 * whose camera-frame depth is EXACTLY 0 in fp32 gets the clamped error maxReproj in the TILED stream (rcp(0) = inf)
 * instead of the x,y-as-is projection; the exact re-score of the contenders and the refinement follow the reference. */
#define ESAC_FLAG_SCORE_TILED 2
#define ESAC_FLAG_SCORE_STREAM 4
/* Sampling reads the maps through a packed (x,y,z,0)-per-cell copy made at the start of the call (default: only when
 * the maps are far larger than the caches and several experts are in play).  Results are unchanged. */
#define ESAC_FLAG_PACK_MAPS 8
/* Sampling without the screen: every try of every hypothesis is solved and decided by the fp64 route (the reference's own
 * loop, esac_util.h:152-223, try by try).  The default route screens the tries of long searches (wrong-expert hypotheses)
 * with a one-sided fp32 test first and decides only what the screen cannot rule out; the accepted
 * try is the same either way -- this flag is the guaranteed route, several times slower on such hypotheses, like
 * ESAC_FLAG_EXACT_SCORES for the scores.  The P3P of either route aligns the two triangles with orthonormal triads and Newton
 * steps, not with the reference's eigen-solve: on collinear base points and ill-conditioned slivers the two can accept different
 * tries.  ESAC_FLAG_STRICT_REFERENCE is the route with the reference's alignment. */
#define ESAC_FLAG_EXACT_SAMPLING 16
/* d_scores_out is indexed by GLOBAL hypothesis index (d_hyp_index[i], or hyp_offset + i) instead of by local position:
 * a multi-GPU shard writes its scores straight into its slots of the exchange buffer. */
#define ESAC_FLAG_SCORES_BY_INDEX 32
/* Take the two guaranteed routes (ESAC_FLAG_EXACT_SCORES | ESAC_FLAG_EXACT_SAMPLING) WHERE THEY ARE FREE: a single frame of ONE
 * expert with N * H * W <= 2^21 (BASELINE configs[0] / [1]: 64 or 256 hypotheses on the 60x80 grid).  There the exact score of
 * every hypothesis is one ~10 us launch on the whole chip, its softmax statistics run in the refinement kernel's prologue and
 * the sampler has no screened stage anyway: the call costs what the default route costs (bench.py: `value` runs with this flag,
 * `value_fast` without it) and the score vector, ESAC_RES_PROB and ESAC_RES_ENTROPY are the reference's own values.  Everywhere
 * else the flag changes nothing (several experts, many hypotheses, large maps, batches: the fp32 ranking stream + exact re-score of
 * the contenders is several times faster there).  esac.forward() of the Python module sets it unless told otherwise. */
#define ESAC_FLAG_AUTO_EXACT 64
#define ESAC_AUTO_EXACT_MAX_WORK (1 << 21) /* N * H * W up to which ESAC_FLAG_AUTO_EXACT applies */
/* The winner is refined by ONE workgroup whatever the shape (no team on one XCD, no cooperating workgroups): the route that
 * needs no co-residency of several workgroups.  What a blocking call falls back to by itself after a team time-out; a caller of
 * ASYNCHRONOUS calls (the multi-GPU exchange: esac_hip_pick_record returned -12) sets it to run the frame again. */
#define ESAC_FLAG_REFINE_SOLO 128
/* The reference, as written, in the three places where the default knowingly differs -- for validating a
 * port, chasing a disagreement with the CPU code or regenerating published numbers on the device:
 *   - P3P alignment: Horn's unit-quaternion method with a cyclic Jacobi eigen-solve of the 4x4 (operation by operation the
 *     oracle's restatement) instead of triads + Newton steps, so collinear base points and ill-conditioned minimal sets give the
 *     reference's pose and the sampling loop accepts the reference's try;
 *   - non-finite scene coordinates: std::min(l, maxReproj) lets a NaN error through (esac_util.h:358), every score of that
 *     expert's hypotheses is NaN, softMax makes every probability NaN, the entropy is 0 and draw keeps hypothesis 0, which is
 *     refined (default: such a cell is an outlier at maxReproj);
 *   - LM: a trial is rejected iff sqrt(err2) > sqrt(prev2), also a converged one whose two norms are a few ulp apart (default:
 *     accepted inside 8 eps when it ends its re-fit).
 * Implies ESAC_FLAG_EXACT_SCORES | ESAC_FLAG_EXACT_SAMPLING and the serial route: every try solved in fp64 without the fp32
 * screen, every hypothesis scored in reference arithmetic, no speculative straggler chain, the selection in a launch of its own.
 * It costs what those two flags cost plus the eigen-solve in every candidate of every try: measured on an MI355X, 1.45 times
 * the call with the two exact flags at 1 expert / 256 hypotheses (0.137 against 0.094 ms), 4.2 times at 10 experts / 1024
 * hypotheses (2.23 against 0.54 ms); it is a verification route, not a fast one.
 * It does NOT pin OpenCV's own internals: the oracle restates the published algorithms (Gao P3P, Horn, Numerical Recipes'
 * jacobi, CvLevMarq), and libm's last bits (pow, acos, cos) differ between host and device, so a try that rounding decides may
 * still differ.
 * Honoured by esac_hip_forward, esac_hip_forward_batch and esac_hip_forward_batch_cams.  Combined with ESAC_FLAG_SCORE_TILED,
 * ESAC_FLAG_SCORE_STREAM or ESAC_FLAG_AUTO_EXACT it is an argument error (-4); esac_hip_backward* return -4 with it ("the
 * training path has no strict mode" under THIS flag: its form for the training path is ESAC_FLAG_STRICT_TRAINING). */
#define ESAC_FLAG_STRICT_REFERENCE 256
/* The strict mode of the TRAINING path: every stage of esac_backward follows the reference where the default knowingly differs,
 * so that the gradient of the four sampled cells of a hypothesis (central differences of the 4-point solver, step 1e-3: the two
 * solvers' disagreement times 500) meets the bar of every other cell:
 *   - sampling, scores, LM trial test: as under ESAC_FLAG_STRICT_REFERENCE (Horn / Jacobi alignment, NaN scores, plain test);
 *   - path II: the 18 perturbed solves of dPNP use the Horn / Jacobi alignment;
 *   - path I: (J^T J).inv(DECOMP_SVD) -- the cyclic-Jacobi pseudo-inverse -- on EVERY slot (default: LDL^T at full rank);
 *   - a non-finite scene coordinate: every probability is NaN (softMax), the entropy is 0, the expected loss is NaN, no slot is
 *     refined (h_out[1] = 0) and every gradient entry of every expert that owns a hypothesis becomes NaN, the other experts'
 *     entries stay as they were -- what the reference's `+=` of NaN-weighted slabs leaves.  The call returns 0.
 * Honoured by esac_hip_backward (blocking and asynchronous), esac_hip_backward_batch and esac_hip_backward_batch_cams.  An
 * argument error (-4, before any launch) on every forward / phase entry point, and together with ESAC_FLAG_STRICT_REFERENCE.
 * Inside the library it implies the exact-sampling and exact-score routes.  A verification route, several times slower where
 * wrong-expert hypotheses search long (LAB_NOTES.md, "Strict training"). */
#define ESAC_FLAG_STRICT_TRAINING 512

#define ESAC_DEFAULT_MARGIN 1e-3f

/* Layout of the result record (doubles).  Written by the refinement kernel. */
enum {
    ESAC_RES_SCORE = 0,      /* exact soft-inlier score of the winner (esac_util.h:235-260)     */
    ESAC_RES_HYP = 1,        /* winner hypothesis index (GLOBAL = hyp_offset + local)            */
    ESAC_RES_EXPERT = 2,     /* hypAssignment[winner]  (esac.cpp:189, the return value)          */
    ESAC_RES_RVEC = 3,       /* refined rvec[3], tvec[3] (scene->camera, OpenCV convention)      */
    ESAC_RES_TVEC = 6,
    ESAC_RES_POSE = 9,       /* 16 values: float(inverse([R t;0 1])) row-major (esac.cpp:182-187) */
    ESAC_RES_REF_STEPS = 25, /* accepted re-fits in refineHyp (esac_util.h:396-452)              */
    ESAC_RES_INLIERS = 26,   /* inlier count of the last accepted set                            */
    ESAC_RES_PROB = 27,      /* softmax probability of the winner (esac.cpp:157)                 */
    ESAC_RES_ENTROPY = 28,   /* entropy of the hypothesis distribution (esac.cpp:158)            */
    ESAC_RES_CONTENDERS = 29,/* how many hypotheses were re-scored exactly                       */
    ESAC_RES_LM_ITERS = 30,  /* total LM iterations spent in refinement                          */
    ESAC_RES_VALID = 31,     /* d_result_out only: 1.0 once a record has been written (multi-GPU exchange buffers
                                are zero-padded; the host copy carries the inlier-map buffer index here instead);
                                3.0: the workgroups sharing the refinement timed out -- no record, and not an empty shard */
    ESAC_RES_DOUBLES = 32
};

/* Stage buffers that can be read back / written for stage-wise parity tests. */
enum {
    ESAC_BUF_HYPS = 0,       /* double[N][6]  rvec,tvec per hypothesis (esac_types.h:40 pose_t)  */
    ESAC_BUF_SAMPLE_XY = 1,  /* int32[N][4][2] sampled cells (esac_util.h:187 sampledPoints)     */
    ESAC_BUF_TRIES = 2,      /* int32[N] accepted try index, -1 = budget exhausted               */
    ESAC_BUF_SCORES = 3,     /* double[N] scores (fp32-path value, exact for re-scored ones)     */
    ESAC_BUF_RESULT = 4,     /* double[ESAC_RES_DOUBLES]                                          */
    ESAC_BUF_INLIER_MAP = 5, /* uint8[H*W] last accepted inlier set (esac_util.h:440 inlierMap)  */
    ESAC_BUF_INLIER_COUNTS = 6, /* int32[ESAC_MAX_REF_STEPS+1] inlier count seen at each step    */
    ESAC_BUF_WINNER_ERRS = 7,   /* float[H*W] reprojection errors of the refined pose; only kept after
                                   esac_hip_set_debug(ctx, ESAC_DEBUG_ERROR_IMAGE)               */
    ESAC_BUF_EXACT_FLAGS = 8,   /* uint8[N] 1 where ESAC_BUF_SCORES holds an exact re-score      */
    ESAC_BUF_CYCLES = 9,        /* int64[32] shader-cycle counters of the refinement kernel (profiling) */
    /* stage outputs of the most recent esac_hip_backward */
    ESAC_BUF_BWD_PROBS = 10,       /* double[N]   selection probabilities (softmax of the exact scores)      */
    ESAC_BUF_BWD_LOSSES = 11,      /* double[N]   pose loss of every (refined) hypothesis                    */
    ESAC_BUF_BWD_REF_HYPS = 12,    /* double[N,6] refined poses (initial pose where p < PROB_THRESH)          */
    ESAC_BUF_BWD_SCORE_GRADS = 13, /* double[N]   d expected loss / d score                                  */
    ESAC_BUF_BWD_SLOTS = 14,       /* int32[N]    hypothesis index per slot, first h_out[1] entries valid    */
    ESAC_BUF_BWD_SLOT_INFO = 15,   /* int32[min(N,ESAC_BWD_MAX_SLOTS),4] per slot: accepted map buffer (-1 none),
                                      inliers of the last accepted step, accepted steps, LM iterations        */
    ESAC_BUF_BWD_DLOSS = 16,       /* double[min(N,ESAC_BWD_MAX_SLOTS),6] d loss / d refined pose per slot    */
    ESAC_BUF_BWD_PATH1 = 17,       /* double[k,3,H,W] gradient slabs of the first k slots, path I (unweighted)  */
    ESAC_BUF_BWD_PATH2 = 18,       /* double[k,3,H,W] the same for path II; k = bytes / (3*H*W*8) <= #slots     */
    ESAC_BUF_BWD_TEAM_INFO = 20,   /* int32[4] training path: [0] 1 when the slots of the most recent esac_hip_backward were refined by
                                      teams of 8 workgroups (one XCD each) instead of one workgroup per slot -- blocking calls
                                      that THEMSELVES select <= 32 hypotheses (decided on the device), grids of 1024..8192 cells; [1] calls that issued the team launch so
                                      far; [2] of them, calls in which a team timed out and the slots were refined again by one
                                      workgroup each (teams stay off on this context afterwards); [3] slots of the last call */
    ESAC_BUF_SPEC_INFO = 21,       /* int32[4] speculative forward (ESAC_DEBUG_NO_SPECULATION): [0] forward calls on this context that took the
                                      speculative route, [1] those among them whose speculation failed (the refinement ran again for
                                      the true winner), [2] 1 when the most recent forward call was speculative, [3] 1 when its
                                      speculation failed */
    ESAC_BUF_SPEC_FLAGS = 22,      /* uint8[N] after a speculative call: 1 where the sampler's first pass left the hypothesis to the straggler chain */
    ESAC_BUF_BWD_MAPS = 23,        /* uint8[k,2,H*W] the two inlier-map buffers of the first k slots of the most recent blocking
                                      esac_hip_backward, cells as y * W + x; ESAC_BUF_BWD_SLOT_INFO[s][0] names the one that holds the
                                      last accepted inlier set of slot s (-1: neither); k = bytes / (2*H*W) <= #slots             */
    ESAC_BUF_REFINE_INFO = 19      /* int32[8] how the most recent winner refinement ran (refineHyp, esac_util.h:378-454):
                                      [0] 0 one workgroup, 1 cooperating workgroups (grids beyond one LDS list), 2 a team on
                                      one XCD (small grids); [1] workgroups sharing it; [2] XCD census of a team: byte x = members
                                      that ran on XCD x, x = 0..3, [7] the same for XCDs 4..7; [3] bit 0: all members shared one
                                      XCD, bit 1: the team ran the route kernel (esac_hip_set_refine_route); [4] exchanges between them; [5] 1 when an exchange timed out; [6] bits 0..29: blocking calls on this
                                      context so far whose team timed out and were refined again by one workgroup, bit 30: the
                                      context has stopped asking for teams (two time-outs in a row; esac_hip_set_refine_team)   */
};

/* Hypotheses that take part in the training expectation: selection probability >= PROB_THRESH = 0.001
 * (esac_derivative.h:33), so never more than 1000 whatever N is. */
#define ESAC_BWD_MAX_SLOTS 1000

typedef struct esac_hip_ctx esac_hip_ctx;

/* library / device */
int esac_hip_abi_version(void);
const char* esac_hip_last_error(void);
int esac_hip_device_count(void);

/* A context owns the device workspaces for one GPU; not thread-safe, one call in
 * flight per context (the reference extension is not re-entrant either:
 * static RNG, thread_rand.cpp:4-5). */
int esac_hip_create(esac_hip_ctx** ctx, int device);
int esac_hip_destroy(esac_hip_ctx* ctx);

/*
 * The whole of esac_forward (esac.cpp:64-190) on the device:
 *   sample+P3P -> soft-inlier scores -> select (+exact re-score of the contenders)
 *   -> refine the winner -> pose.
 * d_scene_coords  [E,3,H,W] float32, d_hyp_assign [N] int64 (device).
 * d_scores_out    optional device double[N]  (the score vector; all-reduced across ranks by the caller)
 * d_result_out    optional device double[ESAC_RES_DOUBLES]
 * h_result_out    optional host   double[ESAC_RES_DOUBLES]; when non-NULL the call blocks until the
 *                 refinement kernel has delivered the record (it stores it into pinned host memory and
 *                 the host polls an epoch word: no copy kernel, no completion-signal round trip);
 *                 the reference call is blocking too.
 */
int esac_hip_forward(esac_hip_ctx* ctx, const float* d_scene_coords, const int64_t* d_hyp_assign,
                     const esac_hip_params* p, void* stream, double* d_scores_out,
                     double* d_result_out, double* h_result_out);

/*
 * B frames in ONE set of launches (new, beside the drop-in call): one blocking call per frame
 * occupies a single CU for its refinement tail, so independent frames are what fills the other 255.
 * d_scene_coords  frame b at d_scene_coords + b * sc_frame_stride (elements; 0 = every frame uses the same maps),
 *                 each [E,3,H,W]; d_hyp_assign [B,N]; p describes ONE frame (N = hypotheses per frame).
 * Frame b draws the RNG streams of call p->call + b: the batch equals B sequential esac_hip_forward calls with consecutive
 * call counters -- every discrete output identical, the poses bit for bit when the single calls refine on the batch's route
 * (esac_hip_set_refine_team(ctx, 8): a batch's teams are 8 per frame, a single call's default team is chosen per grid), else to
 * the rounding of the LM sums (~1e-9).
 * Outputs are frame-major: d_scores_out [B,N], d_result_out / h_result_out [B,ESAC_RES_DOUBLES].
 */
int esac_hip_forward_batch(esac_hip_ctx* ctx, int B, const float* d_scene_coords, int64_t sc_frame_stride,
                           const int64_t* d_hyp_assign, const esac_hip_params* p, void* stream,
                           double* d_scores_out, double* d_result_out, double* h_result_out);

/*
 * esac_hip_forward_batch with a camera per frame: h_cams = HOST array of B records, frame b is computed with h_cams[b]'s
 * shift_x, shift_y, focal, ppx, ppy and the five fields of p are ignored; everything else in p stays one value per batch.
 * Frame b then equals esac_hip_forward with p's five fields replaced by h_cams[b] and call p->call + b (same routes, same
 * bits as described above).  h_cams == NULL is esac_hip_forward_batch exactly.
 * Every record is checked like a single call's camera (focal > 0, pixel positions within int32) before anything is launched;
 * the error (-4) names the first offending frame.  The table is copied into pinned memory the context owns and uploaded on
 * `stream` into a context-owned device buffer that only grows: the caller's array may be reused as soon as the call returns,
 * also for an asynchronous call (h_result_out == NULL).
 */
int esac_hip_forward_batch_cams(esac_hip_ctx* ctx, int B, const float* d_scene_coords, int64_t sc_frame_stride,
                                const int64_t* d_hyp_assign, const esac_hip_params* p, const esac_hip_frame_cam* h_cams,
                                void* stream, double* d_scores_out, double* d_result_out, double* h_result_out);

/*
 * A RAGGED batch: esac_hip_forward_batch_cams whose frames also differ in image size (test sets resized by the shorter edge:
 * grids such as 60x80, 80x60 and 60x90 side by side).  Frame b's grid is h_cams[b].reserved[0] rows x reserved[1] columns
 * (reserved[2] is ignored); h_cams is required.  Additive: the ABI version stays.
 *   layout    frame b's maps lie DENSE as [E,3,h_b,w_b] floats at d_scene_coords + b * sc_frame_stride -- no row strides; the
 *             rest of the slot is never read.  sc_frame_stride >= 3 * E * h_b * w_b for every frame, and a multiple of 4
 *             floats (the 16-byte loads of the score and refinement kernels).
 *   capacity  p->H * p->W is the number of cells every per-frame buffer and every launch is sized for: h_b * w_b <= p->H * p->W.
 *             Only the product matters (60x80 and 80x60 share a capacity of 4800); p->H x p->W must itself be a legal grid.
 *   contract  frame b is esac_hip_forward on that frame alone: its own [E,3,h_b,w_b] maps, h_cams[b]'s camera, call p->call + b,
 *             and the re-score margin of ITS grid (p->rescore_margin, or the default for h_b * w_b cells) -- discrete outputs
 *             and ESAC_RES_CONTENDERS identical, scores and poses as described for esac_hip_forward_batch.
 *   checks    every frame passes a single call's grid rule (at least 3x3, (h-1)(w-1) >= 4, at most 65535 rows / columns), fits
 *             the capacity and its slot, and its camera fits ITS pixel range; the error (-4) names the first offending frame.
 *   read-back esac_hip_read keeps the capacity stride: after the call, frame b's per-cell data is the first h_b * w_b entries
 *             of its slot of p->H * p->W (ESAC_BUF_INLIER_MAP, frame 0's: p->H * p->W bytes whose first h_0 * w_0 are the map).
 * A table whose shapes all equal p->H x p->W computes what esac_hip_forward_batch_cams computes, bit for bit.  B == 1 is the
 * single call on h_cams[0]'s grid.  h_result_out == NULL is the asynchronous form.  The training calls: esac_hip_backward_batch_shapes, _dev_shapes.
 */
int esac_hip_forward_batch_shapes(esac_hip_ctx* ctx, int B, const float* d_scene_coords, int64_t sc_frame_stride,
                                  const int64_t* d_hyp_assign, const esac_hip_params* p, const esac_hip_frame_cam* h_cams,
                                  void* stream, double* d_scores_out, double* d_result_out, double* h_result_out);

/*
 * Multi-GPU exchange (new; the reference has no multi-device path): d_records = `world` result records of
 * ESAC_RES_DOUBLES doubles each (device), e.g. the tail of the all-reduced buffer [N scores | world records] with
 * all-zero records for ranks without hypotheses (ESAC_RES_VALID marks real ones).  Picks the global winner -- highest
 * exact score, lowest global hypothesis index on ties (esac_util.h:519) -- on the device and delivers it to
 * h_record_out (blocking, through pinned memory).  -11: no rank contributed a record.  -12: the refinement team of at least one
 * rank timed out (ESAC_RES_VALID = 3 in its record): no winner is declared without that rank's candidate; every rank reads the
 * same records and gets the same status, so all of them run the frame again with ESAC_FLAG_REFINE_SOLO (esac_amd/distributed.py).
 * d_zero / n_zero: optional (NULL / 0) device doubles the same launch sets to 0 -- a caller that alternates between two
 * exchange buffers hands over the one the NEXT call will use, so that no call starts with a memset of its own.
 */
int esac_hip_pick_record(esac_hip_ctx* ctx, const double* d_records, int world, void* stream, double* h_record_out, double* d_zero,
                         int n_zero);

/*
 * The ONE collective of the multi-GPU path -- all-reduce(SUM) of the exchange buffer [N scores | world x 32-double records] over
 * RCCL / xGMI -- issued by the library itself on the launch stream (new).  esac_hip_comm_unique_id: rank 0 makes an RCCL unique
 * id (ESAC_COMM_ID_BYTES bytes) and hands it to every rank by whatever means the caller has (esac_amd/distributed.py: one
 * broadcast over the torch.distributed process group, once); esac_hip_comm_init: every rank joins with it (collective,
 * blocking); esac_hip_allreduce_sum: in place on `stream`, asynchronous.  -13: no communicator on this context.  RCCL is bound
 * when the first of these is called (dlopen of librccl.so.1: the copy the process already holds, else ROCm's), not at link time:
 * a single-GPU process never loads it; -14: it could not be loaded.  -300 - r: RCCL returned ncclResult_t r.
 */
#define ESAC_COMM_ID_BYTES 128
int esac_hip_comm_unique_id(void* out_id, size_t bytes);
int esac_hip_comm_init(esac_hip_ctx* ctx, int nranks, int rank, const void* unique_id, size_t bytes);
int esac_hip_comm_destroy(esac_hip_ctx* ctx);
int esac_hip_allreduce_sum(esac_hip_ctx* ctx, double* d_buf, size_t count, void* stream);
/* What the context's communicator ITSELF reports: out[0] = ncclCommCount, out[1] = ncclCommUserRank, out[2] = ncclCommCuDevice
 * (-1 when the loaded RCCL lacks the query), out[3] = the context's GPU.  -13: no communicator.  (bench.py: `ranks_seen`.) */
int esac_hip_comm_info(esac_hip_ctx* ctx, int32_t out[4]);

/*
 * Load-balanced multi-GPU shard, built on the device (new; SURVEY.md 8e: "a load-balanced assignment from the
 * hypAssignment histogram", test_esac.py:178).  The hypotheses are ordered by (expert, index) -- the stable counting sort
 * of d_hyp_assign [N] -- and rank r of `world` takes the sorted positions [r*N/world, (r+1)*N/world) (remainder to the
 * first ranks): every rank gets N/world hypotheses (+-1) whatever the gating distribution is, its hypotheses belong to a
 * CONTIGUOUS range of experts [first, last], and only the experts at the two ends of that range are shared with a
 * neighbour (their maps are needed on both ranks).  The plan is a pure function of the assignment vector, so every rank
 * computes the same one without communication.
 * d_index_out   int32[n_local]  global indices of this rank's hypotheses (pass as esac_hip_params.d_hyp_index)
 * d_assign_out  int64[n_local]  their experts minus `expert_base` (pass as d_hyp_assign of the forward call; values
 *               outside [0,E) are copied unchanged so that the forward call still reports them)
 * d_info_out    optional int32[4]: first expert, last expert, n_local, 1 if a value was outside [0,E)
 * n_local = N/world (+1 for rank < N % world) is known to the caller.  expert_base: 0 when the forward call sees all E
 * maps; the rank's first expert when it sees only the maps [first, last] (then also esac_hip_params.expert_base).
 * One launch on `stream`, asynchronous.  E <= 4096.
 */
int esac_hip_shard_balanced(esac_hip_ctx* ctx, const int64_t* d_hyp_assign, int N, int E, int world, int rank,
                            int expert_base, void* stream, int32_t* d_index_out, int64_t* d_assign_out, int32_t* d_info_out);

/*
 * The test loop's figures of a batch, computed on the device (new; test_esac.py:209-247): what a caller of the batched forward
 * needs to report a test set without a host round trip per image.  Frame b takes its pose from ESAC_RES_POSE of record b -- the
 * 16 values as FLOATS, the numbers esac.forward puts into outPose -- and its row of ESAC_EVAL_DOUBLES doubles holds, in fp64:
 *   ESAC_EVAL_ROT_DEG   |axis-angle(out_R * gt_R^T)| * 180 / pi                (test_esac.py:213-216)
 *   ESAC_EVAL_TRANS_CM  |gt_t - out_t| * 100                                    (test_esac.py:211)
 *   ESAC_EVAL_POSE_OK   1 when TRANS_CM < trans_thresh_cm and ROT_DEG < rot_thresh_deg (strict), else 0
 *   ESAC_EVAL_CLASS_OK  1 when ESAC_RES_EXPERT == d_gt_experts[b], else 0; -1 when d_gt_experts is NULL
 *   ESAC_EVAL_QUAT      qw qx qy qz and ESAC_EVAL_INV_T tx ty tz of the INVERTED pose (general 4x4 inverse, then
 *                       (cos(a/2), sin(a/2) * axis), axis (1,0,0) at angle 0): one line of poses_esac_*.txt (test_esac.py:230-247)
 *   ESAC_EVAL_EXPERT, ESAC_EVAL_HYP   copied from the record
 *   ESAC_EVAL_STATUS    0: a delivered record (ESAC_RES_VALID == 1); 3: ESAC_RES_VALID == 3, the refinement team of an
 *                       asynchronous batch timed out -- run that frame again with ESAC_FLAG_REFINE_SOLO at call + b; 1: no record.
 *                       With a status other than 0 the two errors, the quaternion and the translation are NaN and both flags 0
 *                       (CLASS_OK stays -1 without d_gt_experts).
 * A non-finite pose gives NaN figures and POSE_OK = 0 with status 0; a singular one a NaN quaternion and translation.
 * The axis-angle step is the one of esac_amd/harness.py (rodrigues_vector), branch by branch: rows differ from the harness's host
 * functions by libm's last bits.
 * d_records    DEVICE [B,ESAC_RES_DOUBLES]: what esac_hip_forward_batch* wrote through d_result_out.
 * d_gt_poses   DEVICE float [B,4,4]; d_gt_experts DEVICE int64 [B] or NULL; d_out DEVICE [B,ESAC_EVAL_DOUBLES].
 * Asynchronous: one launch on `stream`, no allocation, no wait, no state of a forward call in flight is touched; everything is
 * read in stream order, so the call may be enqueued right behind an asynchronous esac_hip_forward_batch*.
 * -4 before any launch: B outside [1,ESAC_MAX_BATCH], a null d_records, d_gt_poses or d_out, a negative or non-finite threshold.
 */
#define ESAC_EVAL_DOUBLES 16
enum { ESAC_EVAL_ROT_DEG = 0, ESAC_EVAL_TRANS_CM = 1, ESAC_EVAL_POSE_OK = 2, ESAC_EVAL_CLASS_OK = 3,
       ESAC_EVAL_QUAT = 4 /* qw qx qy qz */, ESAC_EVAL_INV_T = 8 /* tx ty tz */, ESAC_EVAL_EXPERT = 11,
       ESAC_EVAL_HYP = 12, ESAC_EVAL_STATUS = 13 /* 14, 15 reserved, written 0 */ };
int esac_hip_eval_batch(esac_hip_ctx* ctx, int B, const double* d_records /* [B,ESAC_RES_DOUBLES] */,
                        const float* d_gt_poses /* DEVICE [B,4,4] */, const int64_t* d_gt_experts /* DEVICE [B] or NULL */,
                        float rot_thresh_deg, float trans_thresh_cm, void* stream, double* d_out /* DEVICE [B,ESAC_EVAL_DOUBLES] */);

/*
 * Pose verification (new, additive: the ABI version stays): how well do the scene-coordinate maps support a GIVEN pose, and how
 * certain is it?  K poses per frame -- a ground-truth pose, the previous frame's, an odometry prediction, a hypothesis read back --
 * each evaluated against ONE expert's map of its frame, on that frame's grid and camera.  Row [b,k] of ESAC_VERIFY_DOUBLES doubles:
 *   ESAC_VERIFY_SCORE   the reference-arithmetic soft-inlier score (esac_util.h:235-260): what ESAC_RES_SCORE holds for the winner.
 *                       A non-finite cell is an outlier at max_reproj; under ESAC_FLAG_STRICT_REFERENCE the score is NaN.
 *   ESAC_VERIFY_N       cells with err < tau, err the clamped float reprojection error: the refinement's inlier rule (a NaN error is
 *                       never an inlier).  Over THESE cells, in fp64, with (ex, ey) = projection - pixel and its Jacobian rows Ju, Jv
 *                       with respect to (rvec, tvec) -- the LM's own parameters:
 *   ESAC_VERIFY_SSE     sum of ex^2 + ey^2
 *   ESAC_VERIFY_A       the 21 upper-triangle entries, row-major, of A = sum of Ju^T Ju + Jv^T Jv
 *   ESAC_VERIFY_SIGMA2  SSE / (2 n - 6)
 *   ESAC_VERIFY_C       the 6x6 covariance sigma^2 A^-1 of (rvec, tvec), row-major, both triangles
 *   ESAC_VERIFY_STATUS  ESAC_VERIFY_OK; _FEW: n < 4 -- score, n, SSE and A stand, sigma^2 and C are NaN; _PINV: A is rank deficient
 *                       to rounding (e.g. collinear inliers) and C is sigma^2 times its pseudo-inverse (eigenvalues below 2 eps
 *                       sum|w| dropped); _BAD_POSE: the pose is not finite, or its 4x4 is singular; _BAD_EXPERT: the expert is
 *                       outside [0,E).  Under the last two every figure is NaN.  They are outcomes of THAT row, like the record
 *                       flags of esac_hip_backward_batch_dev: the other rows of the call are unaffected and nothing is read out of
 *                       bounds (the expert is checked before an address is formed from it).
 *   doubles 5 and 27 are reserved and written 0.
 * d_sc         DEVICE, frame b's [E,3,H,W] maps at d_sc + b * sc_frame_stride (elements; 0: every frame reads the same maps); a
 *              ragged call: the packed rows of esac_hip_forward_batch_shapes, dense [E,3,h_b,w_b] per frame.
 * d_poses      DEVICE.  ESAC_VERIFY_POSE_RT: double [B,K,6], rvec | tvec, scene -> camera (ESAC_RES_RVEC, ESAC_BUF_HYPS);
 *              ESAC_VERIFY_POSE_4X4: float [B,K,4,4] CAMERA poses as outPose and gtPoses carry them, inverted on the device (general
 *              inverse, nearest rotation, Rodrigues: the training path's treatment of a ground-truth pose).
 * d_experts    DEVICE int32 [B,K]: the map each pose is held against.
 * p            ONE frame, as in esac_hip_forward_batch.  Read: E, H, W, shift_x, shift_y, focal, ppx, ppy, inlier_thresh,
 *              inlier_alpha, inlier_beta, max_reproj, sub_sampling and ESAC_FLAG_STRICT_REFERENCE of flags (the flag word must
 *              be a legal forward call's).  Everything else is ignored, N included.
 * cams         HOST, B records or NULL, as in esac_hip_forward_batch_cams (copied before the call returns; the five camera fields of
 *              p are then ignored).  ragged != 0: reserved[0..1] of record b is frame b's grid h_b x w_b and p's H * W the capacity,
 *              with the layout and the per-frame checks of esac_hip_forward_batch_shapes; the table is then required.
 * d_out        DEVICE double [B,K,ESAC_VERIFY_DOUBLES].
 * One launch on `stream`, asynchronous, a workgroup per row: no allocation on the calling path after the first call with a table,
 * no wait but the one on the PREVIOUS verify call's table copy having left its staging buffer.  Everything is read in stream
 * order, so the call may be enqueued right behind an asynchronous esac_hip_forward_batch* and read its records' poses.  It touches
 * no hypothesis, score or result workspace of the context: esac_hip_read after it returns what it returned before.  A row is a
 * function of its pose, map, grid and camera alone (fixed summation order): the same in any batch, run to run.
 * -1: null ctx or p.  -4 before anything is launched, naming the argument: B outside [1,ESAC_MAX_BATCH], K outside
 * [1,ESAC_VERIFY_MAX_POSES], an unknown pose_format, a null d_sc, d_poses, d_experts or d_out, ragged without a table, a negative
 * stride; then the parameter block, the table and the grids with the codes and messages of the forward batch calls.
 */
#define ESAC_VERIFY_DOUBLES 64
#define ESAC_VERIFY_MAX_POSES 1024
enum { ESAC_VERIFY_SCORE = 0, ESAC_VERIFY_N = 1, ESAC_VERIFY_SSE = 2, ESAC_VERIFY_SIGMA2 = 3, ESAC_VERIFY_STATUS = 4 /* 5 reserved */,
       ESAC_VERIFY_A = 6 /* 21 values; 27 reserved */, ESAC_VERIFY_C = 28 /* 36 values */ };
enum { ESAC_VERIFY_OK = 0, ESAC_VERIFY_FEW = 1, ESAC_VERIFY_PINV = 2, ESAC_VERIFY_BAD_POSE = 3, ESAC_VERIFY_BAD_EXPERT = 4 };
enum { ESAC_VERIFY_POSE_RT = 0, ESAC_VERIFY_POSE_4X4 = 1 };
int esac_hip_verify_batch(esac_hip_ctx* ctx, int B, int K, const float* d_sc, int64_t sc_frame_stride, const void* d_poses,
                          int pose_format, const int32_t* d_experts, const esac_hip_params* p, const esac_hip_frame_cam* cams,
                          int ragged, void* stream, double* d_out);

/*
 * esac_backward (esac.cpp:213-520): expected pose loss over the hypothesis distribution and its gradient wrt the
 * scene coordinates, everything on the device.
 * Status -10: hypAssignment held a value outside [0,E) (the reference reads out of bounds there).
 * d_out_gradients [E,3,H,W] float32 (device), ACCUMULATED into (`+=`, esac.cpp:491-508) -- the caller zeroes it,
 *                 as train_esac.py:176 does.
 * h_gt_pose       host float[16], the ground-truth camera pose (4x4 row-major; gtPose, esac.cpp:219).
 * w_loss_rot / w_loss_trans / loss_cut: wLossRot, wLossTrans, lossCut (esac.cpp:220-222).
 * h_out           optional host double[4]: expected loss (the return value of esac_backward), number of
 *                 hypotheses with p >= PROB_THRESH, entropy of the distribution, 1 if an assignment was out of range.  When non-NULL the call
 *                 blocks on `stream` (the reference call is blocking); otherwise it is asynchronous.
 * Uses the same Philox streams as esac_hip_forward for (seed, call): the hypotheses of a backward call are the
 * hypotheses of the forward call with the same counter.  Hypothesis sharding (hyp_offset / d_hyp_index) is
 * rejected: the softmax expectation needs every hypothesis on one device.
 */
int esac_hip_backward(esac_hip_ctx* ctx, const float* d_scene_coords, float* d_out_gradients,
                      const int64_t* d_hyp_assign, const float* h_gt_pose, float w_loss_rot, float w_loss_trans,
                      float loss_cut, const esac_hip_params* p, void* stream, double* h_out);

/*
 * B frames of the training path in one set of launches (new, beside esac_hip_forward_batch): independent frames fill the CUs
 * that one frame's selection, slot refinement and accumulation leave idle.  p describes ONE frame (N = hypotheses per frame).
 * d_scene_coords   frame b at d_scene_coords + b * sc_frame_stride (elements; 0 = every frame reads the same maps), each [E,3,H,W].
 * d_out_gradients  frame b's tensor [E,3,H,W] at d_out_gradients + b * grad_frame_stride (elements; >= E*3*H*W when B > 1: no
 *                  two frames alias), ACCUMULATED into (`+=`); within a frame the slots are added in hypothesis order.
 * d_hyp_assign     [B,N] int64 (device); h_gt_poses host float [B,4,4].
 * h_out            host double[B,4], REQUIRED (blocking only; NULL: -4): frame b's record at h_out[b*4 + 0..3], the four values
 *                  of esac_hip_backward.  An out-of-range assignment in frame b sets h_out[b*4+3] = 1 and the call returns -10
 *                  after every frame has run.
 * Frame b draws the Philox streams of call p->call + b, so it is the b-th of B consecutive esac_hip_backward calls: the same
 * hypotheses, slot list, losses, entropy and record; the gradient bit for bit when the single calls refine their slots with one
 * workgroup each (a context created with ESAC_SLOT_TEAMS=0), else to the rounding of the slot teams' LM sums.
 * Rejected before anything is launched (the gradients stay untouched): B outside [1,ESAC_MAX_BATCH], null pointers, sharding
 * (hyp_offset / d_hyp_index), a too small grad_frame_stride, a singular ground-truth pose in any frame, E > 65535.
 * Slot workspace: B x cap slots (~50 H W bytes each) within a per-context budget (2 GiB; ESAC_BWD_BATCH_BUDGET_MB at context
 * creation); beyond it the frames run in chunks of consecutive frames, each with its own launches -- the results do not depend on
 * the chunking.  A frame selecting more slots than the workspace holds stops the accumulation of every frame of its chunk; the
 * chunk's selection .. accumulation then runs once more with the workspace grown to the largest frame's count.
 * esac_hip_read afterwards: the ESAC_BUF_BWD_* buffers of the hypotheses and slot tables (PROBS, LOSSES, REF_HYPS,
 * SCORE_GRADS, SLOTS, SLOT_INFO, DLOSS) hold the last chunk's frames frame-major -- B x the single-frame size reads them all
 * (a size that fits neither B nor one frame fails), the single-frame size reads frame 0; PATH1 / PATH2 read frame 0's slabs (at most
 * the batch's slots per frame).
 */
int esac_hip_backward_batch(esac_hip_ctx* ctx, int B, const float* d_scene_coords, int64_t sc_frame_stride,
                            float* d_out_gradients, int64_t grad_frame_stride, const int64_t* d_hyp_assign,
                            const float* h_gt_poses, float w_loss_rot, float w_loss_trans, float loss_cut,
                            const esac_hip_params* p, void* stream, double* h_out);

/*
 * esac_hip_backward_batch with a camera per frame (the training loop draws a new random shift for every image and reads the
 * focal length per image): h_cams = HOST array of B records as in esac_hip_forward_batch_cams, the five fields of p are ignored.
 * Frame b is the esac_hip_backward call with h_cams[b]'s camera and call p->call + b, bit for bit under the conditions above.
 * Chunks of a batch beyond the workspace budget and the re-run after a slot overflow keep frame b with record b.  A bad record
 * (focal <= 0, pixel positions beyond int32) is rejected with -4 naming the frame before anything is launched: the gradients
 * stay untouched.  h_cams == NULL is esac_hip_backward_batch exactly.
 */
int esac_hip_backward_batch_cams(esac_hip_ctx* ctx, int B, const float* d_scene_coords, int64_t sc_frame_stride,
                                 float* d_out_gradients, int64_t grad_frame_stride, const int64_t* d_hyp_assign,
                                 const float* h_gt_poses, const esac_hip_frame_cam* h_cams, float w_loss_rot,
                                 float w_loss_trans, float loss_cut, const esac_hip_params* p, void* stream, double* h_out);

/*
 * The ASYNCHRONOUS batch of the training path: esac_hip_backward_batch_cams with the ground truth and the records in device
 * memory.  The call returns once its launches are enqueued on `stream`; it waits for nothing on the stream, polls nothing and
 * runs nothing twice (the one host wait it can meet is on the PREVIOUS call's camera-table copy having left its staging buffer).
 * Everything it reads -- coordinates, assignment, ground-truth poses, the gradients' prior content -- is read in stream order: a
 * producer queued ahead on `stream` is honoured, a consumer queued behind it sees the final gradients and records.
 * d_gt_poses   DEVICE float [B,4,4].  The 4x4 inverse, polar factor and Rodrigues step run in a kernel (the same text the
 *              blocking calls run on the host).  A singular pose cannot be rejected before the launch: it is a per-frame outcome
 *              -- that frame's gradients are left untouched, its record is (NaN, 0, 0, 2), the other frames are unaffected, and
 *              esac_hip_check afterwards returns -4 naming the frame.
 * h_cams       host, B records or NULL, as in esac_hip_backward_batch_cams (copied before the call returns).
 * d_out        DEVICE double [B,4], REQUIRED: frame b's record at d_out[b*4 + 0..3], the four values of esac_hip_backward.  An
 *              out-of-range assignment in frame b sets d_out[b*4+3] = 1; esac_hip_check afterwards returns -10.
 * Slot workspace: the host cannot look at the selection's count, so every frame owns the worst case min(N, ESAC_BWD_MAX_SLOTS)
 * slots -- no overflow, no second pass -- and the frames run in chunks of consecutive frames within the context's budget
 * (ESAC_BWD_BATCH_BUDGET_MB), one launch set after the other on `stream`.  One frame's worst case beyond the budget: -4 before
 * anything is launched (the blocking call sizes the workspace by the true count).  Slots are refined with one workgroup each:
 * frame b is bit for bit frame b of the blocking batch on the same inputs.
 * ESAC_FLAG_STRICT_TRAINING and per-frame cameras as in esac_hip_backward_batch_cams; ESAC_FLAG_STRICT_REFERENCE, sharding, B
 * outside [1,ESAC_MAX_BATCH], null pointers, a too small grad_frame_stride, E > 65535 and a bad camera record are rejected with
 * its codes and messages before anything is launched.  esac_hip_read after a device synchronisation: as after the blocking batch
 * (the last chunk's frames, frame-major).
 */
int esac_hip_backward_batch_dev(esac_hip_ctx* ctx, int B, const float* d_scene_coords, int64_t sc_frame_stride,
                                float* d_out_gradients, int64_t grad_frame_stride, const int64_t* d_hyp_assign,
                                const float* d_gt_poses, const esac_hip_frame_cam* h_cams, float w_loss_rot,
                                float w_loss_trans, float loss_cut, const esac_hip_params* p, void* stream, double* d_out);

/*
 * RAGGED training batches (new, additive: the ABI version stays): esac_hip_backward_batch_cams / esac_hip_backward_batch_dev whose
 * frames also differ in image size, as in esac_hip_forward_batch_shapes.  Frame b's grid is h_cams[b].reserved[0] rows x
 * reserved[1] columns (reserved[2] is ignored); h_cams is required (-1 without it).
 *   layout    frame b's maps lie DENSE as [E,3,h_b,w_b] floats at d_scene_coords + b * sc_frame_stride, and its gradients DENSE
 *             as [E,3,h_b,w_b] floats at d_out_gradients + b * grad_frame_stride, accumulated into (+=).  Nothing beyond the
 *             3 * E * h_b * w_b floats of either slot is read or written.  sc_frame_stride as in esac_hip_forward_batch_shapes;
 *             with B > 1, grad_frame_stride >= 3 * E * h_b * w_b for every frame (so >= 3 * E * max(h_b * w_b)).
 *   capacity  p->H * p->W >= every h_b * w_b: what the slot workspace, its chunks within ESAC_BWD_BATCH_BUDGET_MB (a slot is
 *             charged at the capacity whatever its frame's size -- a chunk of small frames could hold more of them) and every
 *             launch are sized for.  The gradient stride is NOT held against the capacity.
 *   contract  frame b is esac_hip_backward on that frame alone: its own maps, h_cams[b]'s camera, its ground truth, call p->call
 *             + b; bit for bit under the conditions of esac_hip_backward_batch.  Chunks, the blocking call's re-run after a slot
 *             overflow, the asynchronous call's worst-case slots, ESAC_FLAG_STRICT_TRAINING and armed pose records
 *             (esac_hip_set_bwd_pose_records) work as in the shared-shape calls.
 *   checks    those of the shared-shape call (its codes and messages), every frame as in esac_hip_forward_batch_shapes, and the
 *             gradient slots; the error (-4) names the first offending frame.  All before anything is launched: the gradients
 *             stay untouched.
 *   read-back per-hypothesis and per-slot tables as after esac_hip_backward_batch.  ESAC_BUF_BWD_PATH1 / _PATH2 / _MAPS (frame
 *             0 of the last chunk): inside a frame's region slot k lies at the frame's OWN cells p_0 = h_0 * w_0 -- slabs of
 *             3 * p_0 doubles, slot maps of 2 * p_0 bytes -- and that is the unit these reads take after such a call.
 * A table whose shapes all equal p->H x p->W computes what esac_hip_backward_batch_cams / _dev compute, bit for bit; B == 1 is
 * that call with B == 1 on h_cams[0]'s grid.
 */
int esac_hip_backward_batch_shapes(esac_hip_ctx* ctx, int B, const float* d_scene_coords, int64_t sc_frame_stride,
                                   float* d_out_gradients, int64_t grad_frame_stride, const int64_t* d_hyp_assign,
                                   const float* h_gt_poses, const esac_hip_frame_cam* h_cams, float w_loss_rot,
                                   float w_loss_trans, float loss_cut, const esac_hip_params* p, void* stream, double* h_out);
int esac_hip_backward_batch_dev_shapes(esac_hip_ctx* ctx, int B, const float* d_scene_coords, int64_t sc_frame_stride,
                                       float* d_out_gradients, int64_t grad_frame_stride, const int64_t* d_hyp_assign,
                                       const float* d_gt_poses, const esac_hip_frame_cam* h_cams, float w_loss_rot,
                                       float w_loss_trans, float loss_cut, const esac_hip_params* p, void* stream, double* d_out);

/*
 * The winner's refined pose of a training call, as a forward record (new, additive: the ABI version stays).  A training call
 * draws the hypotheses of the forward call with the same (seed, call), scores all of them in reference arithmetic and refines
 * every hypothesis with p >= PROB_THRESH -- the argmax among them, for N <= 1000 always.  An armed call hands that one out in the
 * ESAC_RES_* format, so a training loop that logs pose errors, the winning expert or gating accuracy needs no forward call
 * beside it: esac_hip_eval_batch reads the records as it reads a forward batch's.
 *
 * Arms the NEXT training call on ctx (esac_hip_backward, _backward_batch, _batch_cams, _batch_dev): frame b's
 * forward-format record goes to d_records + b * ESAC_RES_DOUBLES (DEVICE memory), in stream order.  One-shot: consumed
 * by that call whether it is accepted or rejected.  NULL disarms.  frames < that call's B: the call returns -4 before
 * anything is launched.
 *
 * The record of frame b (one small launch per chunk behind the slot refinement; an unarmed call launches what it always did):
 *   ESAC_RES_HYP        the argmax of the frame's exact scores: highest score, first index on ties, a NaN never wins
 *                       (hypothesis 0 when every score is NaN) -- the hypothesis esac_hip_forward refines at this (seed, call)
 *   ESAC_RES_SCORE, _EXPERT (expert_base included), _PROB (the softmax value of the training call), _ENTROPY (the value of the
 *                       call's own record, h_out / d_out [b*4+2]), _CONTENDERS (N: as a forward call under
 *                       ESAC_FLAG_EXACT_SCORES, every score is exact)
 *   ESAC_RES_RVEC|TVEC  the slot's refined pose; ESAC_RES_POSE its inverted 4x4 as floats; _REF_STEPS, _INLIERS, _LM_ITERS of
 *                       the slot's refinement; ESAC_RES_VALID = 1.  The slot route and the forward's team sum the LM moments in
 *                       different orders: poses agree to ~1e-8, the discrete fields exactly.
 * NO SLOT: the winner's probability is below PROB_THRESH (possible from N > 1000 on a flat distribution), the frame selected
 * nothing (a singular ground-truth pose on the asynchronous route, NaN scores under ESAC_FLAG_STRICT_TRAINING).  Then SCORE, HYP,
 * EXPERT, PROB, ENTROPY and CONTENDERS stand, RVEC|TVEC and POSE are NaN, REF_STEPS, INLIERS and LM_ITERS are 0 and
 * ESAC_RES_VALID is 0 -- "no record" to esac_hip_eval_batch (ESAC_EVAL_STATUS 1).
 * All ESAC_RES_DOUBLES doubles of every frame of the call are written by every pass: a batch beyond the workspace budget runs in
 * chunks and frame b's record still lands in row b; the second pass of a blocking call (slot overflow, a slot team that timed
 * out) overwrites what the first left, so after a blocking call every row is final.  Sharded calls stay rejected.
 * -1: null ctx.  -4: d_records with frames < 1.
 */
int esac_hip_set_bwd_pose_records(esac_hip_ctx* ctx, double* d_records, int frames);

/* The same phases one at a time (asynchronous on `stream`), for stage-wise parity
 * tests and for callers that interleave other work.  Order: sample, score, select, refine. */
int esac_hip_sample(esac_hip_ctx* ctx, const float* d_scene_coords, const int64_t* d_hyp_assign,
                    const esac_hip_params* p, void* stream);   /* esac_util.h:129-225 */
int esac_hip_score(esac_hip_ctx* ctx, const float* d_scene_coords, const int64_t* d_hyp_assign,
                   const esac_hip_params* p, void* stream);    /* esac.cpp:131-147   */
int esac_hip_select(esac_hip_ctx* ctx, const float* d_scene_coords, const int64_t* d_hyp_assign,
                    const esac_hip_params* p, void* stream);   /* esac.cpp:153-155   */
int esac_hip_refine(esac_hip_ctx* ctx, const float* d_scene_coords, const int64_t* d_hyp_assign,
                    const esac_hip_params* p, void* stream);   /* esac.cpp:167-187   */

/* Exact (reference-arithmetic) scoring of every hypothesis; slow path used by tests
 * and by callers that want scores identical to esac_util.h:235-260 for all N. */
int esac_hip_score_exact(esac_hip_ctx* ctx, const float* d_scene_coords, const int64_t* d_hyp_assign,
                         const esac_hip_params* p, void* stream);

/* Waits for the device; -10 when the most recent SAMPLING launch on this context (esac_hip_forward / _batch / _sample /
 * _backward) met a hypAssignment value outside [0,E), -12 when the workgroups sharing its most recent winner refinement
 * could not synchronise (blocking calls report the former themselves and, when a small-grid team timed out, run the
 * refinement again in one workgroup; asynchronous ones -- no host result pointer -- cannot: their device record then
 * carries ESAC_RES_VALID = 3 and this function counts the time-out towards the same two-in-a-row latch), else 0.
 * Out-of-range values never cause an out-of-bounds read: such hypotheses are evaluated against expert 0.
 * When the most recent call was esac_hip_backward_batch_dev, its per-frame outcomes are reported: -4 naming the first frame
 * whose ground-truth pose was singular, else -10 naming the first frame whose assignment was out of range. */
int esac_hip_check(esac_hip_ctx* ctx);

/* Stage buffer access (synchronous). `bytes` must match the buffer size for (which, N, H, W).  After a batched call of B frames
 * the per-frame buffers ESAC_BUF_HYPS, _SAMPLE_XY, _TRIES, _SCORES and _INLIER_COUNTS also accept B x that size and then return
 * every frame's, frame-major (the single-frame size reads frame 0). */
int esac_hip_read(esac_hip_ctx* ctx, int which, void* h_dst, size_t bytes);
int esac_hip_write_hyps(esac_hip_ctx* ctx, const double* h_hyps, int N);

/* Time of the most recent launch of each phase on this context in milliseconds
 * (hipEvents around each kernel; the StopWatch prints of esac.cpp:124,149,161,179).
 * out[0..4] = sample, score, select+rescore, refine, total; out[5] = an empty event interval (the
 * bracketing overhead contained in each of the four phase figures).  Synchronises on the last event. */
int esac_hip_phase_ms(esac_hip_ctx* ctx, float out[6]);
/* Mean duration of the score kernel itself over every launch since timing was enabled, measured on the
 * device: max(end) - min(start) over its workgroups on the constant 100 MHz wall clock -- the figure
 * rocprofv3's kernel trace reports (hipEvents around one ~3 us launch also contain the launch gap).
 * Synchronises the device. */
int esac_hip_score_span_ms(esac_hip_ctx* ctx, float* mean_ms, int* launches);
/* Mean GPU time (ms) of each stage -- sample, score, select(+re-score), refine -- for this input: the chain runs once,
 * then each stage is launched `reps` times back to back between one pair of hipEvents on `stream` (includes the ~1.5 us
 * dependent-kernel boundary per launch, excludes the per-event overhead that brackets around single launches carry).
 * Blocking.  out_ms[0..3]. */
int esac_hip_time_stages(esac_hip_ctx* ctx, const float* d_scene_coords, const int64_t* d_hyp_assign,
                         const esac_hip_params* p, void* stream, int reps, float out_ms[4]);
/* Where the HOST's time of the most recent blocking esac_hip_forward / _batch on this context went (CLOCK_MONOTONIC, always
 * recorded: six clock reads, ~0.15 us): out_ns[0..5] = nanoseconds after entry at which the argument block was ready, the
 * sampling / score / refinement launch calls had returned, the result record had landed in pinned memory, and the call
 * returned; out_ns[6] = the entry time itself (absolute, for the caller's own stamps around the call); out_ns[7] unused.
 * What remains of a step beyond the kernels' own durations -- the "host turn" -- is [1] + the gap to the first kernel's
 * start + ([5] - [4]) + the caller's own time between calls (scripts/dev/host_turn.py puts them side by side). */
int esac_hip_host_turn(esac_hip_ctx* ctx, double out_ns[8]);
/* The same stamps as MEANS over the blocking esac_hip_forward / _batch calls since the last reset (running sums kept by the
 * library: the caller's timed loop is not disturbed by collecting them): out_ns[0..5] as above, out_ns[6] = mean time between the
 * return of one call and the entry of the next (the caller's own share of a step), out_ns[7] = number of calls averaged.
 * reset != 0 clears the sums afterwards. */
int esac_hip_host_turn_mean(esac_hip_ctx* ctx, double out_ns[8], int reset);
/* enable/disable the per-phase events (off by default: zero overhead).  enabled = k > 1 samples every k-th forward
 * call only, starting with the next one (the events themselves cost GPU time: an empty pair reads ~5 us). */
int esac_hip_set_timing(esac_hip_ctx* ctx, int enabled);
/* debug options (off by default). ESAC_DEBUG_ERROR_IMAGE: the refinement also stores the reprojection-error image of
 * the pose it is refining (ESAC_BUF_WINNER_ERRS); nothing downstream needs it, so the stores are skipped otherwise. */
#define ESAC_DEBUG_ERROR_IMAGE 1
/* ESAC_DEBUG_COOP_STALL (tests only): the cooperating refinement workgroups of a large-grid call wait for one workgroup
 * more than was launched, with a short spin limit -- exercises the "not all workgroups became resident" failure path
 * (status -12) without having to occupy the GPU. */
#define ESAC_DEBUG_COOP_STALL 2
/* ESAC_DEBUG_TEAM_SPREAD (tests only): the members of a refinement team are launched as CONSECUTIVE workgroups, which the
 * hardware places on different XCDs -- the placement the team's exchange must survive (it is correct at any placement,
 * only slower across XCDs); ESAC_BUF_REFINE_INFO[3] then reads 0. */
#define ESAC_DEBUG_TEAM_SPREAD 4
/* ESAC_DEBUG_NO_SPECULATION (tests, A/B measurements): esac_hip_forward runs its kernels strictly one after the other on the
 * caller's stream.  By default a single-frame call with several experts and at most 8192 hypotheses (the screened sampling
 * route, the fp32 ranking stream, grids below 32768 cells) is SPECULATIVE: once the sampler's first pass (32 tries per
 * hypothesis) has settled the hypotheses of usable experts, those are scored and the best of them (fp32 ranking) is refined on
 * the caller's stream, while on two streams the context owns the sampler's straggler chain -- the wrong-expert hypotheses that
 * need ~10^3 tries each and practically never win -- with the stragglers' scores, and the selection among the settled hypotheses
 * (band, exact re-scores) run beside that refinement; a join kernel then completes the selection over all hypotheses (band,
 * re-scores, softmax statistics, argmax: the serial route's arithmetic statement by statement) and delivers the record, or, when
 * the winner is not the hypothesis that was refined, has the refinement run again (a second launch, enqueued with the call on the
 * caller's stream and gated on the join's verdict: work the caller enqueues behind the call sees the final outputs).  Every
 * output -- poses, scores, flags, statistics, the record -- is what the serial order produces (ESAC_BUF_SPEC_INFO counts). */
#define ESAC_DEBUG_NO_SPECULATION 8
/* ESAC_DEBUG_SPEC_SECOND_BEST (tests only): the speculative refinement starts from the SECOND-best settled hypothesis of the fp32
 * ranking instead of the best -- the situation in which the fp32 stream and the reference arithmetic order two near-equal scores
 * differently.  The join must find that the refined hypothesis is not the winner and the gated second refinement must deliver
 * the serial route's outputs. */
#define ESAC_DEBUG_SPEC_SECOND_BEST 16
/* ESAC_DEBUG_SPEC_LOSE_CHAIN (tests only): the last launch of the straggler chain's stream -- the one that reports "the chain is
 * done" -- is left out, as if it had failed.  The join's wait is bounded (20 ms): it must report status 5, a blocking call must run
 * again in stream order and return that route's outputs, and the context must stop speculating; an asynchronous call's device
 * record carries ESAC_RES_VALID = 3 (esac_hip_pick_record: -12). */
#define ESAC_DEBUG_SPEC_LOSE_CHAIN 32
int esac_hip_set_debug(esac_hip_ctx* ctx, int flags);

/* The winner's refinement (refineHyp, esac_util.h:378-454) on a single frame whose grid fits one workgroup's LDS list
 * (1024 <= H*W <= 32768 cells) is shared by a TEAM of workgroups on one XCD, each owning a slice of the cells: `members` of
 * them (2..ESAC_REFINE_TEAM_MAX = the CUs of an XCD; default ESAC_REFINE_TEAM_DEFAULT: measured 8 = 19 > 10, 12, 16 at 60x80),
 * never more than give every lane of a member one cell (ceil(H*W / 256)) and never fewer than a member's lanes can hold
 * the cells of (ceil(H*W / 1024): four per lane); 0 or 1: one workgroup refines, as on every other shape.
 * Results do not depend on the setting beyond the rounding of the LM sums (every discrete output is identical).
 * esac_hip_forward_batch with up to 32 frames gives every frame's winner a team of 8 (all 32 teams are resident together);
 * larger batches refine with one workgroup per frame.
 * A member waits at most 1 ms (wall clock) for the others at an exchange: a team whose members do not all become resident
 * (a shared / partitioned GPU) gives up, the blocking call refines again in ONE workgroup and returns that result; two such
 * calls in a row and the context stops asking for teams (ESAC_BUF_REFINE_INFO[6] bit 30) -- every call would pay the wait
 * first -- until 1000 further calls have passed or this function is called again (it re-arms the training path's slot
 * teams too). */
#define ESAC_REFINE_TEAM_MAX 32
#define ESAC_REFINE_TEAM_DEFAULT 8
/* The default POLICY (a fresh context; esac_hip_set_refine_team(ctx, ESAC_REFINE_TEAM_AUTO) restores it): ESAC_REFINE_TEAM_DEFAULT
 * members, or -- round 6 -- the smallest team of at most 16 that lowers the cells a lane holds: every lane of a member walks as
 * many cells per pass as its fullest lane owns, eight members of 600 cells hold three per lane on the 60x80 grid, TEN of 480
 * hold two (a pass 0.3 us shorter, the call 2.5 us; teams of up to 16 exchange without an LDS stage).  Batches and the training
 * path's slot teams stay at 8 per team (32 teams of 8 are the chip's 256 CUs).  A number asks for exactly that many. */
#define ESAC_REFINE_TEAM_AUTO (-1)
int esac_hip_set_refine_team(esac_hip_ctx* ctx, int members);
/* A single frame's team of at most 16 members that refines a call with ESAC_FLAG_EXACT_SCORES in force (ESAC_FLAG_AUTO_EXACT
 * where it applies), at most 256 hypotheses, one expert, no speculation and no debug knob runs a kernel with exactly that
 * combination compiled in (same arithmetic, same outputs bit for bit; fewer instructions issued).  on = 0: every team runs
 * the general kernel (A/B measurements, tests).  Default: on; the environment variable ESAC_REFINE_ROUTE=0 starts a context
 * with it off. */
int esac_hip_set_refine_route(esac_hip_ctx* ctx, int on);
/* The two kernels in front of that team -- the sampler and the exact score -- have a route form too: a blocking or asynchronous
 * esac_hip_forward of a single frame with one expert, at most 256 hypotheses on a grid of at most 8192 cells,
 * ESAC_FLAG_EXACT_SCORES in force (ESAC_FLAG_AUTO_EXACT where it applies) and not ESAC_FLAG_STRICT_REFERENCE, no hyp_offset /
 * d_hyp_index, no speculation and no debug knob runs kernels with exactly that combination compiled in (same draws, same
 * arithmetic, same outputs bit for bit).  The route sampler does not store the fp32 pose rows of the streaming score, which
 * nothing on such a call reads; the next stage call that does (esac_hip_score, esac_hip_select) rebuilds them first.
 * on = 0: every call runs the general kernels (A/B measurements, tests).  Default: on; the environment variable
 * ESAC_FRONT_ROUTE=0 starts a context with it off.  The stage entry points, the batches and the training path always run the
 * general kernels. */
int esac_hip_set_front_route(esac_hip_ctx* ctx, int on);
/* 1: the most recent esac_hip_forward* call on this context sampled and scored with the route kernels; 0: with the general ones. */
int esac_hip_front_route_taken(esac_hip_ctx* ctx);
/* Tests: the [N,9] row-major rotation matrices the sampler stored beside the hypotheses of the most recent call (what the exact
 * score multiplies with), N at most that call's; synchronises the device. */
int esac_hip_read_rotations(esac_hip_ctx* ctx, double* h_dst, int N);

/* How a blocking call waits for its result record (written by the last kernel into pinned host memory):
 * ESAC_WAIT_SPIN (default) polls the epoch word -- lowest latency, one host core busy for the ~0.2 ms of the call;
 * ESAC_WAIT_YIELD polls with sched_yield() between reads (a DataLoader-heavy caller keeps its cores);
 * ESAC_WAIT_BLOCK sleeps in hipStreamSynchronize (adds the completion-signal round trip, ~15-20 us). */
#define ESAC_WAIT_SPIN 0
#define ESAC_WAIT_YIELD 1
#define ESAC_WAIT_BLOCK 2
int esac_hip_set_wait(esac_hip_ctx* ctx, int mode);

#ifdef __cplusplus
}
#endif
#endif /* ESAC_HIP_H */
