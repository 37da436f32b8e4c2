// bwd_record_math.hpp -- the forward-format record of a TRAINING call's argmax hypothesis (k_bwd_pose_record, esac_backward.hip;
// esac_hip_set_bwd_pose_records), host + device (ESAC_HD) like eval_math.hpp and select_math.hpp: everything that touches no thread
// index -- the search of the ordered slot list, the assembly of the ESAC_RES_* record from what the selection and the slot
// refinement left in the workspace, and the record of a winner that holds no slot.  The CPU suite compiles it into a stand-alone
// program (tests/native/bwd_record_probe.cpp) and holds it against the oracle's forward call.
// Every index below is a compile-time constant: the record goes from registers straight to its destination, no local array with
// a run-time index (scratch memory).  Compiled without contraction (-ffp-contract=off).
#pragma once
#include "pose_math.hpp"

namespace esac {

// layout of the record (doubles): include/esac_hip.h ESAC_RES_*, held equal by static_asserts in esac_backward.hip
enum { BWD_REC_SCORE = 0, BWD_REC_HYP = 1, BWD_REC_EXPERT = 2, BWD_REC_RVEC = 3, BWD_REC_POSE = 9, BWD_REC_REF_STEPS = 25,
       BWD_REC_INLIERS = 26, BWD_REC_PROB = 27, BWD_REC_ENTROPY = 28, BWD_REC_CONTENDERS = 29, BWD_REC_LM_ITERS = 30,
       BWD_REC_VALID = 31, BWD_REC_DOUBLES = 32 };

// What the record says about the DISTRIBUTION: known for every frame, slot or no slot.
struct BwdRecordHead {
    double score;    // the winner's exact score (score buffer)
    int hyp;         // its global hypothesis index
    int expert;      // its expert, expert_base included
    double prob;     // its selection probability (BwdArgs::probs)
    double entropy;  // the word k_bwd_loss reports for the frame
    int contenders;  // N: what a forward call under ESAC_FLAG_EXACT_SCORES writes (every score is exact)
};

// Position of hypothesis `win` in the ordered slot list sel[0, n) (k_bwd_select writes it ascending), -1: it holds no slot.
// A lower bound by bisection: <= 10 dependent loads for the 1000 slots a frame can own.
ESAC_HD int bwd_record_find_slot(const int* sel, int n, int win) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (sel[mid] < win) lo = mid + 1;
        else                hi = mid;
    }
    return lo < n && sel[lo] == win ? lo : -1;
}

ESAC_HD void bwd_record_head(const BwdRecordHead& h, double* rec) {
    rec[BWD_REC_SCORE] = h.score;
    rec[BWD_REC_HYP] = (double)h.hyp;
    rec[BWD_REC_EXPERT] = (double)h.expert;
    rec[BWD_REC_PROB] = h.prob;
    rec[BWD_REC_ENTROPY] = h.entropy;
    rec[BWD_REC_CONTENDERS] = (double)h.contenders;
}

// The winner holds slot `info`: pose = its refined rvec | tvec (BwdArgs::ref_hyps), info = the slot's map_info row (accepted
// buffer, inliers of the last accepted step, accepted steps, LM iterations).  pose2trans and the float round trip of the 4x4 are
// refine_write_record's (refine_common.hpp): the same two calls, the same cast.
ESAC_HD void bwd_record_with_slot(const BwdRecordHead& h, const double pose[6], const int info[4], double* rec) {
    double R[9], T[16];
    rodrigues_vec2mat<false>(pose, R, nullptr);
    pose_to_inverse_transform(R, pose + 3, T);
    bwd_record_head(h, rec);
#pragma unroll
    for (int k = 0; k < 6; k++) rec[BWD_REC_RVEC + k] = pose[k];
#pragma unroll
    for (int k = 0; k < 16; k++) rec[BWD_REC_POSE + k] = (double)(float)T[k];
    rec[BWD_REC_REF_STEPS] = (double)info[2];
    rec[BWD_REC_INLIERS] = (double)info[1];
    rec[BWD_REC_LM_ITERS] = (double)info[3];
    rec[BWD_REC_VALID] = 1.0;
}

// The winner holds no slot (p < PROB_THRESH, a frame that selected nothing, a slot beyond the workspace of an overflowed pass, a
// pass whose slot teams failed): the distribution's fields stand, no pose exists.  ESAC_RES_VALID = 0 is "no record" to
// esac_hip_eval_batch (status 1).
ESAC_HD void bwd_record_no_slot(const BwdRecordHead& h, double* rec) {
    const double nan = __builtin_nan("");
    bwd_record_head(h, rec);
#pragma unroll
    for (int k = 0; k < 6; k++) rec[BWD_REC_RVEC + k] = nan;
#pragma unroll
    for (int k = 0; k < 16; k++) rec[BWD_REC_POSE + k] = nan;
    rec[BWD_REC_REF_STEPS] = 0.0;
    rec[BWD_REC_INLIERS] = 0.0;
    rec[BWD_REC_LM_ITERS] = 0.0;
    rec[BWD_REC_VALID] = 0.0;
}

// One frame: slot search, then one of the two records.  sel / n: the frame's slot list and its length min(n_sel, cap);
// ref_hyps [N,6], map_info [rows,4]: the frame's.  slots_ok false: the slot tables are not to be trusted (the slot teams failed).
ESAC_HD void bwd_record_frame(const BwdRecordHead& h, int win, const int* sel, int n, bool slots_ok, const double* ref_hyps,
                              const int* map_info, double* rec) {
    const int slot = slots_ok ? bwd_record_find_slot(sel, n, win) : -1;
    if (slot < 0) {
        bwd_record_no_slot(h, rec);
        return;
    }
    const double* hp = ref_hyps + (size_t)win * 6;
    const int* mi = map_info + 4 * slot;
    const double pose[6] = {hp[0], hp[1], hp[2], hp[3], hp[4], hp[5]};
    const int info[4] = {mi[0], mi[1], mi[2], mi[3]};
    bwd_record_with_slot(h, pose, info, rec);
}

}  // namespace esac
