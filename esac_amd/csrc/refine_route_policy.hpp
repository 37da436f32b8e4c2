// refine_route_policy.hpp -- which kernel a single frame's refinement team runs: the general one (k_refine_team, every mode read
// from the argument block at run time) or the ROUTE kernel (k_refine_team_route: the headline call's combination of modes fixed
// at compile time -- esac_refine_team_route.hip).  Plain C++ (no HIP header): the CPU suite reads it through
// tests/native/refine_route_probe.cpp.  Also here, for the same reason: when the team kernel's prologue runs the selection
// (KArgs::fold_select), as a function of plain values.
#pragma once

namespace esac {

constexpr int ROUTE_TEAM_THREADS = 256;       // mirror of REFINE_B (checked by static_assert in refine_team.hpp)
constexpr int ROUTE_TEAM_MAX_MEMBERS = 16;    // the route kernel is instantiated for the direct exchanges (WIDE 8 and 16) only
constexpr int ROUTE_FLAG_EXACT_SCORES = 1, ROUTE_FLAG_STRICT_REFERENCE = 256;  // mirrors of include/esac_hip.h (static_assert, same place)

// KArgs::fold_select of a call whose winner a team of `members` refines (0: no team).
//   1: softmax statistics, band of contenders and their re-score in the team kernel's prologue (the fp32 score route)
//   2: ESAC_FLAG_EXACT_SCORES -- statistics and argmax of the final scores in the prologue (not under
//      ESAC_FLAG_STRICT_REFERENCE: the reference's behaviour on NaN scores lives in k_stats_strict alone)
// Both need one hypothesis per thread of a member; the first also that no device-side span stamps are to be reduced.
inline bool team_folds_select(int members, int N, int flags, bool tstamps) {
    return members > 0 && N <= ROUTE_TEAM_THREADS && !(flags & ROUTE_FLAG_EXACT_SCORES) && !tstamps;
}
inline bool team_folds_exact_stats(int members, int N, int flags) {
    return members > 0 && N <= ROUTE_TEAM_THREADS && (flags & ROUTE_FLAG_EXACT_SCORES) != 0 && !(flags & ROUTE_FLAG_STRICT_REFERENCE);
}
inline int team_fold_select(bool fold_enabled, int members, int N, int flags, bool tstamps) {
    return !fold_enabled ? 0 : team_folds_select(members, N, flags, tstamps) ? 1 : team_folds_exact_stats(members, N, flags) ? 2 : 0;
}

// What launch_refine_team knows about a launch (the fields of the argument block the general kernel branches on)
struct RouteQuery {
    bool enabled;      // esac_hip_set_refine_route / ESAC_REFINE_ROUTE
    int frames;        // 1: a single frame
    int members;       // the team's size
    int N;             // hypotheses
    int E;             // experts
    int flags;         // the call's flags, implied ones included
    int fold_select;   // KArgs::fold_select
    int spec_mode, spec_gate, spec_debug;  // the speculative route
    int coop_extra;    // ESAC_DEBUG_COOP_STALL
    bool errs;         // ESAC_DEBUG_ERROR_IMAGE: an error-image buffer is attached
    bool tstamps;      // a timestamp buffer is attached
};

// The route kernel compiles in: one frame, a team of at most 16 members, fold_select == 2 (exact scores, their statistics and
// argmax in the prologue), one expert, no speculation, no debug knob.  Everything else is the general kernel's.
inline bool refine_takes_route(const RouteQuery& q) {
    return q.enabled && q.frames == 1 && q.members >= 2 && q.members <= ROUTE_TEAM_MAX_MEMBERS && q.fold_select == 2 && q.N <= ROUTE_TEAM_THREADS &&
           q.E == 1 && q.spec_mode == 0 && q.spec_gate == 0 && q.coop_extra == 0 && q.spec_debug == 0 && !q.errs && !q.tstamps &&
           !(q.flags & ROUTE_FLAG_STRICT_REFERENCE);
}

}  // namespace esac
