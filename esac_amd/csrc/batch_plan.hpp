// batch_plan.hpp -- what a batch call's frame table MEANS, decided once and before anything is allocated, staged or launched:
// the checks of the three batch routes in their one order, the parameter block make_args is given, whether a table goes to the
// device, the refinement mode of a ragged table and the records to upload.  Plain C++ (no HIP header, no context): esac_capi.hip
// calls plan_batch once per batch route, tests/native/ragged_policy_probe.cpp and ragged_backward_policy_probe.cpp the same function.
// Every message is one of call_policy.hpp's or ragged_policy.hpp's.  The order of checks:
//   training: null table (ragged), check_batch_call (a ragged call: the capacity is no bound of the gradient stride), check_args
//             with record 0 inline, then every frame -- and, ragged, its gradient slot
//   forward:  null table (ragged), B range (a table: before record 0 is read), check_args with record 0 inline, every frame
#pragma once
#include "ragged_policy.hpp"

namespace esac {

enum BatchRoute { BATCH_FORWARD, BATCH_TRAIN_BLOCKING, BATCH_TRAIN_ASYNC };
struct BatchPlan {
    esac_hip_params p;  // what make_args is given: record 0's camera inline (device_common.hpp:frame_view); a ragged call of ONE frame is
                        // the single call on that frame's grid, and carries its H x W.  (A forward call without a table: the caller's block.)
    bool stage = false;  // a table goes to the device (plan_records); a forward call of one frame has record 0 inline and no table
    int shapes = 0;      // KArgs::shapes over the WHOLE table: 0 shared shape, 1 ragged and every width a multiple of 4, 2 ragged
    size_t cells0 = 0;   // a ragged call: frame 0's own cells (where its second inlier-map buffer starts), else 0
};

inline esac_hip_params with_cam(const esac_hip_params& p, const esac_hip_frame_cam& cam) {
    esac_hip_params q = p;
    q.shift_x = cam.shift_x; q.shift_y = cam.shift_y; q.focal = cam.focal; q.ppx = cam.ppx; q.ppy = cam.ppy;
    return q;
}

// who: the ragged entry point the messages name.  ctx, tensors: the context / every device tensor of the call is there; out: the
// training routes' result pointer is.  ragged: cams[b].reserved[0..1] is frame b's grid and p's H x W the capacity in cells.
inline int plan_batch(BatchRoute route, const char* who, bool ctx, bool tensors, bool out, const esac_hip_params* p, int B, const esac_hip_frame_cam* cams,
                      bool ragged, int64_t sc_frame_stride, int64_t grad_frame_stride, BatchPlan* plan) {
    const bool training = route != BATCH_FORWARD;
    plan->stage = false; plan->shapes = 0; plan->cells0 = 0;
    if (!training && !cams && !ragged) return 0;  // (the single-frame forward: make_args checks the caller's block, as it always has)
    int rc;
    if (ragged && (rc = check_bwd_shapes_entry(who, cams != nullptr))) return rc;
    // (the forward route's B range in check_args' own words: a table's record 0 is read before check_args runs)
    if ((rc = training ? check_batch_call("esac_hip_backward_batch", ctx, p, B, tensors, route == BATCH_TRAIN_ASYNC, out, sc_frame_stride, ragged ? INT64_MAX : grad_frame_stride)
                       : B < 1 || B > ESAC_MAX_BATCH ? fail(-4, "batch size %d outside [1,%d]", B, ESAC_MAX_BATCH) : 0)) return rc;
    if (!ctx || !p) return check_args(ctx, tensors, p, B, -1, training);
    plan->p = cams ? with_cam(*p, cams[0]) : *p;
    plan->stage = cams && (training || B > 1);
    if ((rc = check_args(ctx, tensors, &plan->p, B, cams ? 0 : -1, training))) return rc;
    if (ragged) {
        bool all_vec = true;
        if ((rc = training ? check_bwd_shapes(who, &plan->p, B, cams, sc_frame_stride, grad_frame_stride, &all_vec)
                           : check_shapes(&plan->p, B, cams, sc_frame_stride, &all_vec, who))) return rc;
        // one frame: every single-frame route (tiled score, packed maps, speculation) is open to it
        if (B == 1) plan->p.H = cams[0].reserved[0], plan->p.W = cams[0].reserved[1];
        else plan->shapes = all_vec ? 1 : 2, plan->cells0 = (size_t)cams[0].reserved[0] * (size_t)cams[0].reserved[1];
    }
    for (int b = 0; !ragged && cams && !rc && b < B; b++) rc = check_cam(&plan->p, cams[b].shift_x, cams[b].shift_y, cams[b].focal, b);
    return rc;
}

// The B records a planned call uploads: a ragged table's with each frame's own re-score margin (shape_record), else the caller's
inline void plan_records(const BatchPlan& plan, const esac_hip_frame_cam* cams, int B, esac_hip_frame_cam* out) {
    for (int b = 0; b < B; b++) out[b] = plan.shapes ? shape_record(&plan.p, cams[b]) : cams[b];
}

}  // namespace esac
