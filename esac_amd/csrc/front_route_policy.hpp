// front_route_policy.hpp -- which kernels sample and score a forward call: the general ones (k_sample, k_rescore: every mode read
// from the argument block at run time) or the FRONT ROUTE's (k_sample_route, k_rescore_route: the headline call's combination of
// modes fixed at compile time, no fp32 rows stored -- esac_front_route.hip).  Decided once per call on the host.  Plain C++ (no HIP
// header): the CPU suite reads it through tests/native/front_route_probe.cpp.
#pragma once
#include "sample_plan.hpp"

namespace esac {

constexpr int FRONT_ROUTE_MAX_HYPS = 256;        // one workgroup per hypothesis, every one resident at once (SAMPLE_256x2's range)
constexpr int FRONT_ROUTE_SCORE_THREADS = 1024;  // threads of k_rescore_route (= k_rescore<1024>'s: the same summation order)
constexpr int FRONT_ROUTE_MAX_CELLS = 8 * FRONT_ROUTE_SCORE_THREADS;  // the scorer holds at most 8 cells per lane in registers
                                                                      // (64x128: the largest grid ESAC_FLAG_AUTO_EXACT takes at 256 hypotheses)
constexpr int FRONT_FLAG_EXACT_SCORES = 1;       // mirror of include/esac_hip.h (static_assert in esac_capi.hip and the probe)

// What forward_impl knows about a call when it chooses (the fields of the argument block the general kernels branch on)
struct FrontRouteQuery {
    bool enabled;      // esac_hip_set_front_route / ESAC_FRONT_ROUTE
    bool serial;       // the serial route of forward_impl (not the speculative one)
    int frames;        // 1: a single frame
    int N, E, H, W;
    int flags;         // the call's flags, implied ones included (ESAC_FLAG_AUTO_EXACT applied)
    int max_tries;     // the call's budget (call_scalars)
    int first_try;     // KArgs::first_try
    int hyp_offset;    // a shard's offset into the global hypothesis indices
    bool cams;         // a camera table is attached
    int shapes;        // KArgs::shapes: a ragged batch
    bool packed;       // KArgs::sc4: packed maps for the sampler's gathers
    bool hyp_index;    // a list of global hypothesis indices is attached
    bool spec_flag;    // the speculation's flags are attached
    bool tstamps;      // a timestamp buffer is attached
    bool errs;         // ESAC_DEBUG_ERROR_IMAGE: an error-image buffer is attached
};

// The route kernels compile in: one frame, one expert, the sampler's plan exactly "k_sample<256, 2> from try 0, whole budget, no
// hand-over, no packing, not strict" (the plan the general route would run -- sample_plan), every score exact (k_rescore's
// arithmetic, not the strict one), at most 8 cells per lane of the scorer.  Everything else is the general kernels'.
inline bool front_takes_route(const FrontRouteQuery& q) {
    if (!q.enabled || !q.serial || q.frames != 1 || q.E != 1 || q.N < 1 || q.N > FRONT_ROUTE_MAX_HYPS) return false;
    if (q.H < 1 || q.W < 1 || (long long)q.H * q.W > FRONT_ROUTE_MAX_CELLS) return false;
    if (!(q.flags & FRONT_FLAG_EXACT_SCORES) || (q.flags & ESAC_FLAG_STRICT_REFERENCE_K)) return false;
    if (q.cams || q.shapes != 0 || q.packed || q.hyp_index || q.hyp_offset != 0 || q.spec_flag || q.first_try != 0 || q.tstamps || q.errs) return false;
    const SamplePlan p = sample_plan(q.N, q.frames, q.E, q.max_tries, q.flags, q.first_try, q.packed);
    return p.first == SAMPLE_256x2 && p.passes == 1 && p.grid_x == q.N && p.block == 256 && !p.strict && !p.pack && p.tail == SAMPLE_TAIL_NONE &&
           !p.pending_list && p.handover == 0x7fffffff;
}

}  // namespace esac
