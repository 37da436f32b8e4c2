// esac_backward.hip -- the training path of the extension (esac_backward, code/esac/esac.cpp:213-520) as HIP
// kernels for gfx950.  Forward kernels re-used: k_sample, k_rescore(all) (exact scores of every hypothesis)
// and k_refine in its SLOTS mode (one workgroup per hypothesis that takes part in the expectation).
//
//   K5 k_bwd_select      softMax, entropy, ordered list of hypotheses with p >= PROB_THRESH   esac.cpp:319-331
//   K6 k_bwd_loss        loss per hypothesis, expected loss, dLoss, d expectation / d score    esac.cpp:354-362,
//                                                                                              esac_derivative.h:405-420
//   K7 k_bwd_path1       refined pose -> scene coordinates through the last re-fit             esac.cpp:375-463
//   K8 k_bwd_path2       score -> scene coordinates (direct + via the 4 sampled points)        esac_derivative.h:205-330
//   K9 k_bwd_accumulate  outGradients += p_h * pathI_h + pathII_h, hypotheses in order          esac.cpp:491-508
//      k_bwd_gt_prepare  per-frame ground truth of the asynchronous batch, on the device          esac_util.h:555-568
//      k_bwd_pose_record the argmax hypothesis' refined pose as a forward-format record (armed calls)  esac.cpp:153-187
//
// The reference allocates per-hypothesis (1 x 3P) and (P x 3) double matrices on the host heap for ALL N
// hypotheses and adds them into the float tensor one hypothesis after the other.  Here only the <= 1000
// hypotheses that can pass the probability threshold own a slab, one workgroup fills each slab, and K9 walks the
// slabs in hypothesis order per output element, so the float `+=` chain rounds exactly like the reference's.
// Everything is fp64 VALU work on small per-hypothesis problems plus one streaming pass over the H x W cells per
// slot: no contraction large enough for MFMA.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bwd_math.hpp"
#include "bwd_record_math.hpp"
#include "device_common.hpp"
#include "esac_kernels.hpp"
#include "gt_math.hpp"
#include "pose_math.hpp"
#include "select_math.hpp"

namespace esac {

constexpr int BWD_B = 512;  // threads per slot in the gradient kernels: 8 wavefronts, 256-VGPR budget each

// ================================================================= K5: softmax + ordered selection
// BATCH: esac_hip_backward_batch -- one workgroup per frame, the batch-wide overflow word, the frame's assignment check
// STRICT (ESAC_FLAG_STRICT_TRAINING): the reference on NaN scores (k_rescore_strict lets a non-finite coordinate through).  softMax
// divides by a NaN sum: EVERY probability is NaN, the entropy is 0 (`dist > 0` is false), the expected loss is NaN; no hypothesis
// is below PROB_THRESH (`NaN < t` is false), so the reference carries all N through its loops and adds NaN-weighted slabs: every
// gradient entry of every expert that owns a hypothesis ends as NaN.  Here that end state is produced directly: nothing is
// selected (no slot, no refinement, no slab), n_sel[3] = 1 tells k_bwd_accumulate_strict to store the NaNs.
template <int B, bool BATCH, bool STRICT = false>
__global__ __launch_bounds__(B) void k_bwd_select(KArgs a) {
    __shared__ double s_part[2 * (B / 64)];
    __shared__ double s_tot[2];
    __shared__ double s_max[B / 64];
    __shared__ int s_wcount[B / 64];
    __shared__ int s_base;
    if (BATCH) {
        train_frame_view(a, (int)blockIdx.y);
    }
    // a batch: does this frame's assignment row hold a value outside [0,E)?  (the sampler's status word is shared by the frames;
    // the same test as flag_bad_assignment: one expert never reads the row)
    int bad = 0;
    if (BATCH && a.E > 1) {
        int mine = 0;
        for (int h = threadIdx.x; h < a.N; h += B) mine |= (unsigned long long)a.assign[h] >= (unsigned long long)a.E;
        bad = __syncthreads_or(mine);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double m = -INFINITY;
    for (int i = threadIdx.x; i < a.N; i += B) {
        const double s = a.scores[i];
        m = s > m ? s : m;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double om = __shfl_xor(m, o);
        m = om > m ? om : m;
    }
    if (lane == 0) s_max[wave] = m;
    if (threadIdx.x == 0) s_base = 0;
    __syncthreads();
    m = s_max[0];
#pragma unroll
    for (int w = 1; w < B / 64; w++) m = s_max[w] > m ? s_max[w] : m;
    double acc[2] = {0, 0};
    for (int i = threadIdx.x; i < a.N; i += B) acc[0] += exp(a.scores[i] - m);
    block_sum<2, B>(acc, s_part, s_tot);
    const double sum = acc[0];
    const bool poisoned = STRICT && sum != sum;  // (workgroup-uniform: block_sum hands every lane the same total)
    // esac_hip_backward_batch_dev: a frame whose ground-truth pose is singular (k_bwd_gt_prepare) selects nothing -- no slot, no
    // slab, nothing accumulated: its gradients stay as they are (workgroup-uniform)
    const bool dead = BATCH && a.bwd.frame_status && a.bwd.frame_status[blockIdx.y] == 2;
    // probabilities, entropy, the pose every unselected hypothesis keeps, and the ordered selection:
    // rounds of B consecutive hypotheses, ballot prefix inside a wavefront, wavefront offsets through LDS
    double ent = 0;
    for (int base = 0; base < a.N; base += B) {
        const int i = base + (int)threadIdx.x;
        bool pick = false;
        if (i < a.N) {
            const double p = exp(a.scores[i] - m) / sum;
            a.bwd.probs[i] = p;
            if (p > 0) ent -= p * log2(p);
#pragma unroll
            for (int k = 0; k < 6; k++) a.bwd.ref_hyps[(size_t)i * 6 + k] = a.hyps[(size_t)i * 6 + k];
            pick = !(p < kProbThresh) && !poisoned && !dead;
        }
        const unsigned long long bal = __ballot(pick);
        if (lane == 0) s_wcount[wave] = __popcll(bal);
        __syncthreads();
        int off = s_base;
        for (int w = 0; w < wave; w++) off += s_wcount[w];
        if (pick) {
            const int slot = off + __popcll(bal & ((1ull << lane) - 1ull));
            if (slot < a.bwd.cap) a.bwd.sel[slot] = i;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            int tot = 0;
            for (int w = 0; w < B / 64; w++) tot += s_wcount[w];
            s_base += tot;
        }
        __syncthreads();
    }
    acc[0] = ent;
    acc[1] = 0;
    block_sum<2, B>(acc, s_part, s_tot);
    if (threadIdx.x == 0) {
        if (BATCH) a.bwd.n_sel[2] = bad != 0;
        if (STRICT) a.bwd.n_sel[3] = poisoned && !dead ? 1 : 0;
        a.bwd.n_sel[0] = s_base < a.bwd.cap ? s_base : a.bwd.cap;
        a.bwd.n_sel[1] = s_base;  // unclamped: > cap tells the host to grow the slot workspace and run the call again
        if (BATCH) atomicMax(a.bwd.sel_max, s_base);  // a batch: the accumulation of every frame looks at the largest
        a.stats[0] = m;
        a.stats[1] = sum;
        a.stats[2] = acc[0];
    }
}

// ================================================================= K6: losses, expectation, dLoss
// BATCH: esac_hip_backward_batch (one workgroup per frame, the frame's ground truth from BwdArgs::gt_frames); the single call's
// instantiation keeps the ground truth in the kernel arguments
template <int B, bool BATCH>
__global__ __launch_bounds__(B) void k_bwd_loss(KArgs a) {
    __shared__ double s_part[B / 64];
    __shared__ double s_tot[1];
    double gt[16], gt_pose[6];
    if (BATCH) {
        train_frame_view(a, (int)blockIdx.y);
        bwd_load_gt(a, (int)blockIdx.y, gt, gt_pose);
    } else {
#pragma unroll
        for (int k = 0; k < 16; k++) gt[k] = a.bwd.gt[k];
#pragma unroll
        for (int k = 0; k < 6; k++) gt_pose[k] = a.bwd.gt_pose[k];
    }
    const double wR = a.bwd.w_rot, wT = a.bwd.w_trans, cut = a.bwd.cut;
    double acc[1] = {0};
    for (int h = threadIdx.x; h < a.N; h += B) {
        const double* hp = a.bwd.ref_hyps + (size_t)h * 6;
        const double pose[6] = {hp[0], hp[1], hp[2], hp[3], hp[4], hp[5]};
        const double l = pose_loss(pose, gt, wR, wT, cut);
        a.bwd.losses[h] = l;
        acc[0] += a.bwd.probs[h] * l;
    }
    block_sum<1, B>(acc, s_part, s_tot);
    const double expected = acc[0];
    // d E[loss] / d score_i = p_i l_i - p_i sum_j p_j l_j  (softmax derivative, esac_derivative.h:405-420)
    for (int h = threadIdx.x; h < a.N; h += B) {
        const double p = a.bwd.probs[h];
        a.bwd.sgrad[h] = p < kProbThresh ? 0.0 : p * a.bwd.losses[h] - p * expected;
    }
    const int n_sel = a.bwd.n_sel[0];
    for (int slot = threadIdx.x; slot < n_sel; slot += B) {
        const double* hp = a.bwd.ref_hyps + (size_t)a.bwd.sel[slot] * 6;
        const double pose[6] = {hp[0], hp[1], hp[2], hp[3], hp[4], hp[5]};
        double j[6];
        pose_dloss(pose, gt_pose, wR, wT, cut, j);
#pragma unroll
        for (int k = 0; k < 6; k++) a.bwd.dloss[(size_t)slot * 6 + k] = j[k];
    }
    // out-of-range hypAssignment: the sampler's status word on a single call; a batch shares that word, so each frame looks at
    // its own assignment row (k_bwd_select looked at it: n_sel[2])
    const bool bad = BATCH ? a.bwd.n_sel[2] != 0 : a.status[0] == (unsigned long long)a.sample_epoch;
    if (threadIdx.x == 0) {
        double rec[4] = {expected, (double)a.bwd.n_sel[1], a.stats[2], bad ? 1.0 : 0.0};
        if (BATCH && a.bwd.frame_status) {  // esac_hip_backward_batch_dev: per-frame outcomes, read by esac_hip_check
            int* st = a.bwd.frame_status + blockIdx.y;
            if (*st == 2) {  // singular ground truth: the record says so, nothing else of the frame is meaningful
                rec[0] = __builtin_nan("");
                rec[1] = 0.0; rec[2] = 0.0; rec[3] = 2.0;
            } else if (bad) {
                *st = 1;
            }
        }
#pragma unroll
        for (int k = 0; k < 4; k++) a.bwd.out[k] = rec[k];
        if (BATCH && a.bwd.rec_dev) {  // the record does not depend on the accumulation: no slot overflow exists on this route
#pragma unroll
            for (int k = 0; k < 4; k++) a.bwd.rec_dev[(size_t)blockIdx.y * 4 + k] = rec[k];
        }
    }
}

// ================================================================= ground truth on the device (esac_hip_backward_batch_dev)
// One lane per frame: the float 4x4 pose -> gt[16] | gt_pose[6], the text the blocking calls run on the host (gt_math.hpp).  A
// singular pose leaves NaNs in the record and 2 in the frame's status word; every other frame's word is reset to 0.
__global__ __launch_bounds__(64) void k_bwd_gt_prepare(const float* __restrict__ poses, int B, double* __restrict__ gt_frames,
                                                       int* __restrict__ status) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    float in[16];
#pragma unroll
    for (int k = 0; k < 16; k++) in[k] = poses[(size_t)b * 16 + k];
    double gt[16], gt_pose[6];
    const bool ok = gt_from_pose(in, gt, gt_pose);
    double* g = gt_frames + (size_t)b * ESAC_GT_DOUBLES;
    for (int k = 0; k < 16; k++) g[k] = ok ? gt[k] : __builtin_nan("");
    for (int k = 0; k < 6; k++) g[16 + k] = ok ? gt_pose[k] : __builtin_nan("");
    status[b] = ok ? 0 : 2;
}

// ================================================================= the winner's refined pose as a forward record
// esac_hip_set_bwd_pose_records armed this call: frame b's ESAC_RES_* record of its ARGMAX hypothesis -- the hypothesis the forward
// call with the same (seed, call) refines -- from what the selection and the slot refinement left in the workspace.  One workgroup
// per frame, directly behind the slot refinement; reads only, beside the record itself.  The argmax is draw's (select_math.hpp:
// highest score, first global index on ties, a NaN never wins, hypothesis 0 when nothing can win -- refine_pick_winner's rule
// through the same two functions; every score of a training call is exact).  A winner without a slot gets the no-slot record
// (bwd_record_math.hpp).  All 32 doubles are written on every pass, so the rerun after a slot overflow or a slot-team time-out
// overwrites what the aborted pass left.
static_assert(BWD_REC_SCORE == ESAC_RES_SCORE_K && BWD_REC_HYP == ESAC_RES_HYP_K && BWD_REC_EXPERT == ESAC_RES_EXPERT_K &&
              BWD_REC_RVEC == ESAC_RES_RVEC_K && BWD_REC_POSE == ESAC_RES_POSE_K && BWD_REC_REF_STEPS == ESAC_RES_REF_STEPS_K &&
              BWD_REC_INLIERS == ESAC_RES_INLIERS_K && BWD_REC_PROB == ESAC_RES_PROB_K && BWD_REC_ENTROPY == ESAC_RES_ENTROPY_K &&
              BWD_REC_CONTENDERS == ESAC_RES_CONTENDERS_K && BWD_REC_LM_ITERS == ESAC_RES_LM_ITERS_K, "record layout");
template <int B>
__global__ __launch_bounds__(B) void k_bwd_pose_record(KArgs a) {
    __shared__ double s_best[B / 64];
    __shared__ int s_besti[B / 64], s_bestg[B / 64];
    // (both indexed by the frame of the launch, not moved by the frame's view)
    double* const rec = a.bwd.pose_rec + (size_t)blockIdx.y * BWD_REC_DOUBLES;
    const bool dead = a.bwd.frame_status && a.bwd.frame_status[blockIdx.y] == 2;  // singular ground truth: k_bwd_loss reports entropy 0
    train_frame_view(a, (int)blockIdx.y);
    double bs = -INFINITY;
    int bi = BEST_NONE, bg = BEST_NONE;
    for (int h = threadIdx.x; h < a.N; h += B) best_take(bs, bi, bg, a.scores[h], h, global_hyp(a, h));
    block_best<B, false>(bs, bi, bg, s_best, s_besti, s_bestg);
    if (threadIdx.x != 0) return;
    const int win = bi == BEST_NONE ? 0 : bi;
    // the slots were refined by teams and one of them timed out: ref_hyps / map_info are not to be trusted (the host refines again)
    const bool team_failed = a.bwd.team && __hip_atomic_load(a.coop_counter + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == a.bwd.team_tag;
    const BwdRecordHead head{a.scores[win], global_hyp(a, win), expert_of(a, win) + a.expert_base, a.bwd.probs[win],
                             dead ? 0.0 : a.stats[2], a.N};
    bwd_record_frame(head, win, a.bwd.sel, a.bwd.n_sel[0] /* = min(n_sel, cap) */, !team_failed, a.bwd.ref_hyps, a.bwd.map_info, rec);
}

// ================================================================= K7: path I
// One workgroup per slot.  jacobeanR = -(J^T J)^-1 J^T over the inliers of the last accepted refinement step
// (rows = d residual norm / d pose at the refined pose), clamped to zero as a whole when any entry exceeds 10;
// the slab entry of inlier q is dLoss (1x6) * jacobeanR[:, q] * dProject/dObj (1x3).
// The rare branch of path I: J^T J is rank deficient to rounding (inv_spd6 returned false) -- the reference's own route,
// the SVD pseudo-inverse (bwd_math.hpp:pinv_sym6_jacobi: the same operations in the same order).  Here it must cost the
// common path nothing: ONE lane runs rolled loops over matrices in LDS (a few hundred bytes of code, no registers beyond the
// loop's own -- unrolled into registers it took the kernel to 480 of them and one wavefront per SIMD), the others wait.  Every
// lane reaches this together (U21 is the same in all of them), so the barriers are uniform.  lds: >= 108 doubles.
__device__ __forceinline__ void pinv_sym6_lds(const double (&U21)[21], double (&Ainv)[36], double* lds) {
    double* A = lds;        // [6][6]
    double* V = lds + 36;   // [6][6]
    double* out = lds + 72; // [6][6]
    __syncthreads();
    if (threadIdx.x == 0) pinv_sym6_rolled(U21, A, V, out);  // (bwd_math.hpp: host + device, the CPU suite runs it against the oracle)
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 36; i++) Ainv[i] = out[i];
    __syncthreads();
}

// STRICT (ESAC_FLAG_STRICT_TRAINING): the pseudo-inverse on EVERY slot, as the reference computes (J^T J).inv(DECOMP_SVD)
template <int B, bool STRICT>
__device__ __forceinline__ void bwd_path1(const KArgs& a, int slot, double* s_part, double* s_tot, double* s_max) {
    if (slot >= a.bwd.n_sel[0]) return;
    const int h = a.bwd.sel[slot];
    const int P = a.H * a.W;
    double* __restrict__ g = a.bwd.grad1 + (size_t)slot * P * 3;
    const int* mi = a.bwd.map_info + 4 * slot;
    const int buf = mi[0], n_inl = mi[1];
    if (buf < 0 || n_inl < 4) {  // no accepted re-fit (empty inlier map) or fewer than 4 inliers: zero gradient
        for (int i = threadIdx.x; i < 3 * P; i += B) g[i] = 0;
        return;
    }
    const uint8_t* __restrict__ map = a.bwd.maps + ((size_t)slot * 2 + buf) * P;
    const int e = expert_of(a, h);
    const float* __restrict__ mx = a.sc + (size_t)e * 3 * P;
    const Cam cam = make_cam(a);
    const double* hp = a.bwd.ref_hyps + (size_t)h * 6;
    const double rv[3] = {hp[0], hp[1], hp[2]};
    const double t[3] = {hp[3], hp[4], hp[5]};
    double R[9], dRdr[27];
    rodrigues_vec2mat<true>(rv, R, dRdr);

    double U[21];
#pragma unroll
    for (int k = 0; k < 21; k++) U[k] = 0;
    for (int i = threadIdx.x; i < P; i += B) {
        if (!map[i]) continue;
        const int row = i / a.W, col = i - row * a.W;
        double r6[6];
        norm_jac_row(R, dRdr, t, cam, mx[i], mx[P + i], mx[2 * P + i], cell_px(a, col), cell_py(a, row), a.max_reproj, r6);
        int k = 0;
#pragma unroll
        for (int p = 0; p < 6; p++)
#pragma unroll
            for (int q = p; q < 6; q++) U[k++] += r6[p] * r6[q];
    }
    block_sum28<21, B>(U, s_part, s_tot);
    double Ainv[36];
    if (STRICT) pinv_sym6_lds(U, Ainv, s_part);
    else if (!inv_spd6(U, Ainv)) pinv_sym6_lds(U, Ainv, s_part);  // workgroup-uniform: every lane holds the same sums
    double dL[6];
#pragma unroll
    for (int k = 0; k < 6; k++) dL[k] = a.bwd.dloss[(size_t)slot * 6 + k];

    double vmax = 0;
    for (int i = threadIdx.x; i < P; i += B) {
        double o0 = 0, o1 = 0, o2 = 0;
        if (map[i]) {
            const int row = i / a.W, col = i - row * a.W;
            const float X = mx[i], Y = mx[P + i], Z = mx[2 * P + i];
            const float px = cell_px(a, col), py = cell_py(a, row);
            double r6[6], c6[6], dNdO[3];
            norm_jac_row(R, dRdr, t, cam, X, Y, Z, px, py, a.max_reproj, r6);
#pragma unroll
            for (int p = 0; p < 6; p++) {
                double s = 0;
#pragma unroll
                for (int q = 0; q < 6; q++) s += -Ainv[p * 6 + q] * r6[q];
                c6[p] = s;
                const double av = fabs(s);
                vmax = av > vmax ? av : vmax;
            }
            dproject_dobj(px, py, X, Y, Z, R, t, a.focal, a.ppx, a.ppy, a.max_reproj, dNdO);
#pragma unroll
            for (int p = 0; p < 6; p++) {
                o0 += dL[p] * (c6[p] * dNdO[0]);
                o1 += dL[p] * (c6[p] * dNdO[1]);
                o2 += dL[p] * (c6[p] * dNdO[2]);
            }
        }
        g[i] = o0;
        g[(size_t)P + i] = o1;
        g[2 * (size_t)P + i] = o2;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double ov = __shfl_xor(vmax, o);
        vmax = ov > vmax ? ov : vmax;
    }
    if ((threadIdx.x & 63) == 0) s_max[threadIdx.x >> 6] = vmax;
    __syncthreads();
    vmax = s_max[0];
#pragma unroll
    for (int w = 1; w < B / 64; w++) vmax = s_max[w] > vmax ? s_max[w] : vmax;
    if (vmax > 10) {  // "clamping for stability" (esac.cpp:436-437): the whole pseudo-inverse is dropped
        for (int i = threadIdx.x; i < 3 * P; i += B) g[i] = 0;
    }
}

// ================================================================= K8: path II
// One workgroup per slot.  d score / d coordinates of the INITIAL hypothesis: every cell directly through its own
// reprojection error, and the four sampled cells through the pose (dPNP: central differences of the 4-point solver
// with a float step of 1e-3, esac_derivative.h:128-185).  sum_cells (dRE * dErr/dPose) * dPose/dObj is linear in the
// per-cell term, so the 6 pose-space sums are reduced first and multiplied with the 6x12 dPNP matrix once.
// STRICT (ESAC_FLAG_STRICT_TRAINING): the 18 perturbed solves align with Horn / Jacobi (bwd_math.hpp: dpnp_solve<AlignHorn>)
template <int B, bool STRICT>
__device__ __forceinline__ void bwd_path2(const KArgs& a, int slot, double* s_part, double* s_tot, double (*s_sol)[6], double* s_J, int& s_bad) {
    if (slot >= a.bwd.n_sel[0]) return;
    const int h = a.bwd.sel[slot];
    const int P = a.H * a.W;
    double* __restrict__ g = a.bwd.grad2 + (size_t)slot * P * 3;
    const int e = expert_of(a, h);
    const float* __restrict__ mx = a.sc + (size_t)e * 3 * P;
    const Cam cam = make_cam(a);
    const int* sxy = a.sample_xy + (size_t)h * 8;
    if (threadIdx.x == 0) s_bad = 0;
    if (threadIdx.x < 72) s_J[threadIdx.x] = 0;
    __syncthreads();

    // ---- dPNP: lane 2q / 2q+1 solves with coordinate q (point q/3, axis q%3) moved by +eps / -eps
    if (threadIdx.x < 18) {
        const float eps = 0.001f;
        const int q = threadIdx.x >> 1;
        const bool minus = threadIdx.x & 1;
        float obj[12];
        double mu[4], mv[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int idx = sxy[2 * j + 1] * a.W + sxy[2 * j];
            obj[3 * j] = mx[idx];
            obj[3 * j + 1] = mx[P + idx];
            obj[3 * j + 2] = mx[2 * P + idx];
            mu[j] = (double)cell_px(a, sxy[2 * j]);
            mv[j] = (double)cell_py(a, sxy[2 * j + 1]);
        }
        if constexpr (STRICT) {
            double sol[6];
            if (dpnp_solve<AlignHorn>(obj, mu, mv, cam, q, minus, sol)) {
                double* o = s_sol[threadIdx.x];
#pragma unroll
                for (int k = 0; k < 6; k++) o[k] = sol[k];
            } else {
                atomicOr(&s_bad, 1);
            }
        } else {
            // the reference perturbs in place (+eps, -2eps, +eps), which does not always restore the float value:
            // coordinates handled before q carry that residue into this solve
#pragma unroll
            for (int k = 0; k < 9; k++) {
                const float up = obj[k] + eps;
                const float down = up - 2 * eps;
                const float back = down + eps;
                obj[k] = k < q ? back : (k == q ? (minus ? down : up) : obj[k]);
            }
            V3 Pt[4];
#pragma unroll
            for (int j = 0; j < 4; j++) Pt[j] = V3{(double)obj[3 * j], (double)obj[3 * j + 1], (double)obj[3 * j + 2]};
            double Rp[9], Tp[3], rvec[3];
            if (p3p_4pt(Pt, mu, mv, cam, Rp, Tp)) {
                rodrigues_mat2vec(Rp, rvec);
                double* o = s_sol[threadIdx.x];
                o[0] = rvec[0]; o[1] = rvec[1]; o[2] = rvec[2];
                o[3] = Tp[0]; o[4] = Tp[1]; o[5] = Tp[2];
            } else {
                atomicOr(&s_bad, 1);
            }
        }
    }
    __syncthreads();
    double jv = 0;
    if (threadIdx.x < 54) {
        const int k = threadIdx.x / 9, q = threadIdx.x - 9 * k;
        const float eps = 0.001f;
        jv = (s_sol[2 * q][k] - s_sol[2 * q + 1][k]) / (double)(2 * eps);
        if (jv != jv) atomicOr(&s_bad, 1);
    }
    __syncthreads();
    const bool bad = s_bad != 0;
    // getMax(abs) > 10 -> the whole matrix is dropped (esac_derivative.h:274-275)
    double amax = bad ? 0.0 : fabs(jv);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double ov = __shfl_xor(amax, o);
        amax = ov > amax ? ov : amax;
    }
    if (threadIdx.x < 54 && !bad && !(amax > 10)) {  // all 54 entries sit in wavefront 0
        const int k = threadIdx.x / 9, q = threadIdx.x - 9 * k;
        s_J[k * 12 + q] = jv;
    }
    __syncthreads();

    // ---- every cell: direct term + pose-space sums
    const double* hp = a.hyps + (size_t)h * 6;
    const double rv[3] = {hp[0], hp[1], hp[2]};
    const double t[3] = {hp[3], hp[4], hp[5]};
    double R[9], dRdr[27];
    rodrigues_vec2mat<true>(rv, R, dRdr);
    const float scale = a.alpha / a.W / a.H;
    const double sg = a.bwd.sgrad[h];
    double S[6] = {0, 0, 0, 0, 0, 0};
    for (int i = threadIdx.x; i < P; i += B) {
        const int row = i / a.W, col = i - row * a.W;
        const float X = mx[i], Y = mx[P + i], Z = mx[2 * P + i];
        const float px = cell_px(a, col), py = cell_py(a, row);
        float err = project_exact_err(R, t, cam, X, Y, Z, px, py);
        err = err < a.max_reproj ? err : a.max_reproj;
        double st = a.beta * (err - a.tau);  // float product, widened
        st = 1 / (1 + exp(-st));
        double dRE = -st * (1 - st) * a.beta * sg;
        dRE *= scale;
        double dPdO[3], r6[6];
        dproject_dobj(px, py, X, Y, Z, R, t, a.focal, a.ppx, a.ppy, a.max_reproj, dPdO);
        g[i] = dPdO[0] * dRE;
        g[(size_t)P + i] = dPdO[1] * dRE;
        g[2 * (size_t)P + i] = dPdO[2] * dRE;
        norm_jac_row(R, dRdr, t, cam, X, Y, Z, px, py, a.max_reproj, r6);
#pragma unroll
        for (int k = 0; k < 6; k++) S[k] += dRE * r6[k];
    }
    block_sum28<6, B>(S, s_part, s_tot);
    __syncthreads();  // the slab writes above are visible to the lanes that add the support terms
    if (threadIdx.x < 12) {
        const int m = threadIdx.x;
        double s = 0;
#pragma unroll
        for (int k = 0; k < 6; k++) s += S[k] * s_J[k * 12 + m];
        const int j = m / 3, c = m - 3 * j;
        const int idx = sxy[2 * j + 1] * a.W + sxy[2 * j];
        g[(size_t)c * P + idx] += s;
    }
}

// ================================================================= K7 + K8 in ONE launch
// Neither path reads the other's output (path I: the refined pose, its inlier set, dLoss; path II: the initial hypothesis, its four
// cells, d E / d score), and with a few dozen slots either one is a chain one workgroup long on an otherwise empty chip: workgroups
// [0, slots) take path I, [slots, 2 slots) path II -- 47 + 36 us in sequence became max(path I, path II), with no second stream
// and no event between them (round 6 measured that variant: the fork and the join cost 7 us each).
// STRICT: ESAC_FLAG_STRICT_TRAINING, an instantiation of its own so that the default keeps its registers (250 VGPRs).  The strict
// one fits the same budget (249, no scratch, two wavefronts per SIMD): one lane runs one solve at a time, the eigen-solve's 4x4s
// live after the quartic's state has died
template <int B, bool STRICT = false>
__global__ __launch_bounds__(B) void k_bwd_paths(KArgs a) {
    __shared__ double s_part[28 * (B / 64) > 108 ? 28 * (B / 64) : 108];
    __shared__ double s_tot[28];
    __shared__ double s_max[B / 64];
    __shared__ double s_sol[18][6];
    __shared__ double s_J[72];
    __shared__ int s_bad;
    train_frame_view(a, (int)blockIdx.y);  // (a batch: grid (2 slots, frames))
    const int slots = (int)gridDim.x >> 1;
    if ((int)blockIdx.x < slots) bwd_path1<B, STRICT>(a, (int)blockIdx.x, s_part, s_tot, s_max);
    else                         bwd_path2<B, STRICT>(a, (int)blockIdx.x - slots, s_part, s_tot, s_sol, s_J, s_bad);
}

// ================================================================= K9: ordered accumulation into the float tensor
// grid = (tiles of 3P elements, experts).  Wavefront 0 first compacts, in slot order, the slots whose hypothesis
// belongs to this expert (ballot prefix) together with their probabilities into LDS; then one thread per tensor
// element walks that list with unconditional, coalesced slab loads (slabs are planar like the tensor), U loads in
// flight, while the float `+=` chain itself stays in slot order.
// STRICT (ESAC_FLAG_STRICT_TRAINING): a frame whose scores held a NaN (k_bwd_select<.., true>: n_sel[3]) -- every entry of every
// expert that owns a hypothesis becomes NaN (the reference's float += of NaN-weighted slabs), the other experts' entries stay.
template <bool STRICT>
__device__ __forceinline__ void bwd_accumulate_body(const KArgs& a) {
    __shared__ int s_slot[ESAC_BWD_SLOTS_K];
    __shared__ double s_prob[ESAC_BWD_SLOTS_K];
    __shared__ int s_count;
    const int e = blockIdx.y;
    KArgs f = a;  // frame blockIdx.z of a batch (grid (tiles, experts, frames)); `a` keeps the batch's record and pinned slots
    train_frame_view(f, (int)blockIdx.z);
    // the FRAME's cells: its gradients are dense [E,3,h,w] at the head of its slot, its slabs lie at its own 3 h w.  (The grid's
    // tiles cover the capacity of a ragged batch; `rem < 3 * P` below keeps a smaller frame's workgroups inside its own tensor.)
    const int P = f.H * f.W;
    const int n_sel = f.bwd.n_sel[0];
    // more slots than the workspace holds: nothing is accumulated, the host grows it and retries.  The slots were refined by
    // teams and one of them timed out (a member never became resident): nothing is accumulated either, the host refines the
    // slots again with one workgroup each.  (Both are the same answer in every workgroup of the launch.)
    const bool team_failed = a.bwd.team && __hip_atomic_load(a.coop_counter + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == a.bwd.team_tag;
    // A batch: ONE frame's overflow stops every frame (the host reruns all of them), so they all read the batch-wide maximum.
    const bool skip = (a.bwd.sel_max ? a.bwd.sel_max[0] : f.bwd.n_sel[1]) > a.bwd.cap || team_failed;
    if (STRICT && !skip && f.bwd.n_sel[3] != 0) {  // (workgroup-uniform)
        int mine = 0;
        for (int h = threadIdx.x; h < f.N; h += blockDim.x) mine |= expert_of(f, h) == e;
        const int owns = __syncthreads_or(mine);
        const int rem = blockIdx.x * blockDim.x + threadIdx.x;
        if (owns && rem < 3 * P) {
            float* o = f.bwd.out_grad + (size_t)e * 3 * P + rem;
            *o = *o + __builtin_nanf("");
        }
    } else if (!skip) {
        if (threadIdx.x < 64) {
            int count = 0;
            for (int base = 0; base < n_sel; base += 64) {
                const int slot = base + (int)threadIdx.x;
                int h = 0;
                bool mine = false;
                if (slot < n_sel) {
                    h = f.bwd.sel[slot];
                    mine = expert_of(f, h) == e;
                }
                const unsigned long long bal = __ballot(mine);
                if (mine) {
                    const int pos = count + __popcll(bal & ((1ull << threadIdx.x) - 1ull));
                    s_slot[pos] = slot;
                    s_prob[pos] = f.bwd.probs[h];
                }
                count += __popcll(bal);
            }
            if (threadIdx.x == 0) s_count = count;
        }
        __syncthreads();
        const int n = s_count;
        const int rem = blockIdx.x * blockDim.x + threadIdx.x;  // c * P + cell
        if (n > 0 && rem < 3 * P) {
            float* o = f.bwd.out_grad + (size_t)e * 3 * P + rem;
            float v = *o;
            constexpr int U = 8;
            for (int base = 0; base < n; base += U) {
                double t[U];
#pragma unroll
                for (int u = 0; u < U; u++) {
                    const int q = base + u < n ? base + u : n - 1;  // clamped: the loads are unconditional
                    const size_t k = (size_t)s_slot[q] * 3 * P + rem;
                    t[u] = s_prob[q] * f.bwd.grad1[k] + f.bwd.grad2[k];
                }
#pragma unroll
                for (int u = 0; u < U; u++)
                    if (base + u < n) v = (float)((double)v + t[u]);  // float += double (esac.cpp:501-506)
            }
            *o = v;
        }
    }
    // The call's record -- expected loss, slots, entropy, out-of-range flag (k_bwd_loss wrote them), "a slot team timed out" --
    // goes to the pinned slot the host polls (as the forward's record does: no copy, no stream-completion round trip), by the
    // LAST workgroup of this launch to finish: every one arrives at a counter once its stores are issued.
    if (!a.result_pin) return;
    __syncthreads();
    if (threadIdx.x >= 64) return;
    int last = 0;
    if (threadIdx.x == 0) {
        __threadfence();
        last = atomicAdd(a.bwd.arrived, 1) == (int)(gridDim.x * gridDim.y * gridDim.z) - 1;
        if (last) a.bwd.arrived[0] = 0;  // (every workgroup has arrived: ready for the next call)
    }
    if (!__shfl(last, 0)) return;
    const int lane = threadIdx.x;
    for (int fr = 0; fr < (int)gridDim.z; fr++) {  // one record per frame, into the frame's pinned slot
        const double v = lane < 4 ? a.bwd.out[fr * 4 + lane] : lane == 4 ? (team_failed ? 1.0 : 0.0) : lane == 32 ? a.epoch : 0.0;
        pin_deliver(a.result_pin + (size_t)fr * ESAC_PIN_DOUBLES, v);
    }
}
__global__ __launch_bounds__(256) void k_bwd_accumulate(KArgs a) { bwd_accumulate_body<false>(a); }
__global__ __launch_bounds__(256) void k_bwd_accumulate_strict(KArgs a) { bwd_accumulate_body<true>(a); }

// ---------------------------------------------------------------- launchers
static inline int slot_grid(const KArgs& a) { return a.N < a.bwd.cap ? a.N : a.bwd.cap; }

// (a.frames > 1: esac_hip_backward_batch -- frame b in grid row / layer b)
static inline bool bwd_strict(const KArgs& a) { return (a.flags & ESAC_FLAG_STRICT_TRAINING_K) != 0; }

void launch_bwd_select(const KArgs& a, hipStream_t s) {
    if (bwd_strict(a)) {
        if (a.bwd.gt_frames) hipLaunchKernelGGL((k_bwd_select<1024, true, true>), dim3(1, a.frames), dim3(1024), 0, s, a);
        else                 hipLaunchKernelGGL((k_bwd_select<1024, false, true>), dim3(1), dim3(1024), 0, s, a);
        return;
    }
    if (a.bwd.gt_frames) hipLaunchKernelGGL((k_bwd_select<1024, true>), dim3(1, a.frames), dim3(1024), 0, s, a);
    else                 hipLaunchKernelGGL((k_bwd_select<1024, false>), dim3(1), dim3(1024), 0, s, a);
}
void launch_bwd_loss(const KArgs& a, hipStream_t s) {
    if (a.bwd.gt_frames) hipLaunchKernelGGL((k_bwd_loss<BWD_B, true>), dim3(1, a.frames), dim3(BWD_B), 0, s, a);
    else                 hipLaunchKernelGGL((k_bwd_loss<BWD_B, false>), dim3(1), dim3(BWD_B), 0, s, a);
}
void launch_bwd_paths(const KArgs& a, hipStream_t s) {
    if (bwd_strict(a)) hipLaunchKernelGGL((k_bwd_paths<BWD_B, true>), dim3(2 * slot_grid(a), a.frames), dim3(BWD_B), 0, s, a);
    else               hipLaunchKernelGGL(k_bwd_paths<BWD_B>, dim3(2 * slot_grid(a), a.frames), dim3(BWD_B), 0, s, a);
}
void launch_bwd_gt_prepare(const float* d_gt_poses, int B, double* gt_frames, int* status, hipStream_t s) {
    hipLaunchKernelGGL(k_bwd_gt_prepare, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, s, d_gt_poses, B, gt_frames, status);
}
void launch_bwd_pose_record(const KArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(k_bwd_pose_record<256>, dim3(1, a.frames), dim3(256), 0, s, a);
}
void launch_bwd_accumulate(const KArgs& a, hipStream_t s) {
    const int per_expert = 3 * a.H * a.W;
    const dim3 grid((unsigned)((per_expert + 255) / 256), a.E, a.frames);
    if (bwd_strict(a)) hipLaunchKernelGGL(k_bwd_accumulate_strict, grid, dim3(256), 0, s, a);
    else               hipLaunchKernelGGL(k_bwd_accumulate, grid, dim3(256), 0, s, a);
}

}  // namespace esac
