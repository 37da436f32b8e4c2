// ragged_policy.hpp -- the C ABI host's checks of a RAGGED batch (esac_hip_forward_batch_shapes: frames that differ in image size)
// and the per-frame record its kernels read.  Part of call_policy.hpp (which includes it at its end: plain C++ over
// include/esac_hip.h, no HIP header); a file of its own because tests/test_call_policy_host.py holds every message of
// call_policy.hpp against a recording that predates this entry point.  The checks of a ragged TRAINING batch
// (esac_hip_backward_batch_shapes, _dev_shapes) are at its end.  batch_plan.hpp (plan_batch) is their one caller and sets their
// order; the host and tests/native/ragged_policy_probe.cpp, ragged_backward_policy_probe.cpp reach them through it.
#pragma once
#include "call_policy.hpp"

namespace esac {

// Frame b's grid is cams[b].reserved[0] x reserved[1]; p->H * p->W is the CAPACITY in cells that every per-frame buffer and
// launch is sized for (p has passed check_args).  Every frame: the grid rule of a single call (check_grid), within the capacity,
// within its slot of the packed maps, its camera against its OWN pixel range (check_cam).  Each rejection names the frame.
// *all_vec: every frame's width is a multiple of 4 (KArgs::shapes 1, else 2).
// (who: the entry point the messages name -- the training calls pass their own)
inline int check_shapes(const esac_hip_params* p, int B, const esac_hip_frame_cam* cams, int64_t sc_frame_stride, bool* all_vec,
                        const char* who = "esac_hip_forward_batch_shapes") {
    const long long cap = (long long)p->H * p->W;
    if (sc_frame_stride & 3)
        return fail(-4, "%s: sc_frame_stride %lld is not a multiple of 4 floats (the 16-byte loads of the score and refinement kernels)", who, (long long)sc_frame_stride);
    *all_vec = true;
    for (int b = 0; b < B; b++) {
        const int h = cams[b].reserved[0], w = cams[b].reserved[1];
        if (int rc = check_grid(h, w, b)) return rc;
        const long long cells = (long long)h * w;
        if (cells > cap) return fail(-4, "%s: grid %dx%d in frame %d holds %lld cells, the capacity H*W = %dx%d is %lld", who, h, w, b, cells, p->H, p->W, cap);
        if (3LL * p->E * cells > (long long)sc_frame_stride)
            return fail(-4, "%s: the maps of frame %d (3*E*h*w = %lld floats, grid %dx%d) exceed its slot, sc_frame_stride = %lld", who, b, 3LL * p->E * cells, h, w, (long long)sc_frame_stride);
        if (int rc = check_cam(p, cams[b].shift_x, cams[b].shift_y, cams[b].focal, b, h, w)) return rc;
        if (w & 3) *all_vec = false;
    }
    return 0;
}
// ... and the record the kernels read for frame b: the caller's, with that frame's own re-score margin (float bits) in
// reserved[2] -- what call_scalars gives the single call on h x w, bit for bit.  (The capacity's margin is narrower than a small
// frame's: the band of contenders, and so ESAC_RES_CONTENDERS, would differ from the single call's.)
inline esac_hip_frame_cam shape_record(const esac_hip_params* p, const esac_hip_frame_cam& cam) {
    esac_hip_frame_cam r = cam;
    const float m = rescore_margin(p, cam.reserved[0] * cam.reserved[1]);
    memcpy(&r.reserved[2], &m, sizeof(m));
    return r;
}

// ---------------------------------------------------------------- ragged TRAINING batches
// esac_hip_backward_batch_shapes / esac_hip_backward_batch_dev_shapes (who): the table is required (check_bwd_shapes_entry: the
// first check of every ragged route, forward included), and checked like a forward table; then the gradient slots.  Frame b's gradients are the dense [E,3,h_b,w_b] tensor at d_out_gradients + b *
// grad_frame_stride, so with B > 1 every frame's 3*E*h_b*w_b floats must fit the stride -- the first frame that does not is
// named, and the stride is then >= 3*E*max(h_b*w_b): no two frames share an element.  (One frame has no stride to fit.)  The
// capacity H*W plays no part: it may exceed the largest frame, and a gradient slot need not hold it.
inline int check_bwd_shapes_entry(const char* who, bool table) {
    if (!table) return fail(-1, "%s: null frame table (h_cams carries every frame's grid)", who);
    return 0;
}
inline int check_bwd_shapes(const char* who, const esac_hip_params* p, int B, const esac_hip_frame_cam* cams, int64_t sc_frame_stride,
                            int64_t grad_frame_stride, bool* all_vec) {
    if (int rc = check_shapes(p, B, cams, sc_frame_stride, all_vec, who)) return rc;
    for (int b = 0; B > 1 && b < B; b++) {
        const int h = cams[b].reserved[0], w = cams[b].reserved[1];
        const long long need = 3LL * p->E * h * w;
        if (need > (long long)grad_frame_stride)
            return fail(-4, "%s: the gradients of frame %d (3*E*h*w = %lld floats, grid %dx%d) exceed its slot, grad_frame_stride = %lld "
                            "(frames would share gradients)", who, b, need, h, w, (long long)grad_frame_stride);
    }
    return 0;
}

}  // namespace esac
