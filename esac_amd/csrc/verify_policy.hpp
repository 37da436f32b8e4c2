// verify_policy.hpp -- the C ABI host's checks of esac_hip_verify_batch and the plan of its frame table, before anything is staged
// or launched.  Plain C++ over include/esac_hip.h like call_policy.hpp (no HIP header): esac_capi.hip calls plan_verify once per
// call, tests/native/verify_policy_probe.cpp the same function.  A file of its own because tests/test_call_policy_host.py holds
// every message of call_policy.hpp against a recording.
// The order: context and parameter block (-1, call_policy's words), then what is new here -- B, K, the pose format, the four
// pointers, a ragged call without a table, a negative stride: -4 naming the argument -- then the parameter block, the table and
// the grids through plan_batch / check_args / check_shapes / check_cam with their own messages.
#pragma once
#include "batch_plan.hpp"

namespace esac {

constexpr int VERIFY_MAX_POSES = 1024;  // = ESAC_VERIFY_MAX_POSES (include/esac_hip.h): poses per frame, the launch grid's x

inline int plan_verify(bool ctx, int B, int K, bool sc, int64_t sc_frame_stride, bool poses, int pose_format, bool experts, const esac_hip_params* p,
                       const esac_hip_frame_cam* cams, bool ragged, bool out, BatchPlan* plan) {
    const char* who = "esac_hip_verify_batch";
    if (!ctx) return fail(-1, "null context");
    if (!p) return fail(-1, "null params");
    if (B < 1 || B > ESAC_MAX_BATCH) return fail(-4, "%s: B = %d outside [1,%d]", who, B, ESAC_MAX_BATCH);
    if (K < 1 || K > VERIFY_MAX_POSES) return fail(-4, "%s: K = %d outside [1,%d]", who, K, VERIFY_MAX_POSES);
    if (pose_format != 0 && pose_format != 1)
        return fail(-4, "%s: pose_format = %d (0: double [B,K,6] rvec | tvec, 1: float [B,K,4,4] camera poses)", who, pose_format);
    if (!sc || !poses || !experts || !out)
        return fail(-4, "%s: null %s pointer", who, !sc ? "d_sc" : !poses ? "d_poses" : !experts ? "d_experts" : "d_out");
    if (ragged && !cams) return fail(-4, "%s: ragged without a frame table (cams carries every frame's grid in reserved[0..1])", who);
    if (sc_frame_stride < 0) return fail(-4, "%s: negative sc_frame_stride %lld", who, (long long)sc_frame_stride);
    // the rest of p as a forward batch's; N is not an argument of this call (the kernels never read it): K stands in
    esac_hip_params q = *p;
    q.N = K;
    plan->p = q;
    if (!cams) {  // (plan_batch leaves such a call to make_args' check_args; there is no make_args here)
        plan->stage = false; plan->shapes = 0; plan->cells0 = 0;
        return check_args(true, true, &q, B, -1, false);
    }
    return plan_batch(BATCH_FORWARD, who, true, true, true, &q, B, cams, ragged, sc_frame_stride, 0, plan);
}

}  // namespace esac
