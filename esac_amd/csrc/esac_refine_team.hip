// esac_refine_team.hip -- draw(argmax) + refineHyp + pose2trans of ONE frame on a grid of a few thousand cells, shared by a
// TEAM of workgroups on one XCD (round 4): 8 on the 60x80 grid, up to 32 on grids of up to 32768 cells.
//
// Reference: refineHyp esac_util.h:378-454 (the loop), cv::solvePnP(SOLVEPNP_ITERATIVE, useExtrinsicGuess) reached from
// esac_util.h:426-436 (the re-fit: CvLevMarq, 6 parameters, max_iter 20, eps FLT_EPSILON), draw esac_util.h:505-530,
// pose2trans esac_util.h:537-548.  esac_refine.hip holds the same refinement for one workgroup (and for cooperating
// workgroups on grids beyond one LDS list); this file is the latency shape of the headline call: a 60x80 grid, where one
// workgroup spends 150 us on ~33 dependent passes of 2-6 us each.
//
// What is different here:
//   * CELLS LIVE IN REGISTERS.  Member g of G owns the cells [g P / G, (g+1) P / G); with G = 8 that is <= 1024 cells, at
//     most 4 per lane (600 at 60x80: 3 per lane), loaded once.  No correspondence list, no compaction, no LDS but the
//     reduction scratch: an inlier set is a bit mask per lane.
//   * ONE KIND OF PASS at a pose: the fp64 projection chain of every owned cell (lm_math.hpp: the LM chain, contraction and
//     Newton reciprocal allowed), from it (a) the squared residual over the set the running re-fit works on, (b) `err < tau`
//     for EVERY cell -- decided by the fp64 error against tau +- a band that covers what the reference's float rounding
//     can do, the bit-exact project_exact_err sequence for what is left (practically never) -- i.e. the NEXT inlier set,
//     its count and its squared residual, (c) the 24 moments of the normal equations over the running set or over the
//     next one.  27 sums per pass.
//   * FUSED ROUNDS.  The reference evaluates the error image at a pose, then starts the re-fit with a pass at the SAME
//     pose; and it ends a re-fit with a pass at the pose whose error image it evaluates next.  Whether an LM trial, if
//     accepted, ends the re-fit (iteration 20, or relative step < FLT_EPSILON) is known BEFORE the trial is evaluated
//     (it depends on the step, not on the residual), so such a trial is evaluated as a full pass with the moments over
//     the next set: accepted -- the common case -- it IS the next step's error image and first LM pass.  Rejected, the
//     re-fit goes on with a larger lambda from the normal equations of the last accepted point (they stay in registers,
//     team_step); nothing was overwritten (the sets are register masks).  ~25 rounds per frame instead of ~33, same
//     accepted points, same decisions.
//   * ONE HOP PER ROUND between the members: refine_common.hpp, tagged granules.  The chain-rule matrices of the pose are
//     computed while the exchange is in flight.
//   * COUNTED IN INSTRUCTIONS.  A member runs one wavefront per SIMD; such a wavefront issues one VALU instruction every
//     ~4.8 cycles and waits 10 for a dependent fp64 result (scripts/dev/lat_probe.hip): a round is ~1,100 instructions + the
//     hop + two LDS round trips, and it is the COUNT that binds.  Hence ONE step site, a loop that carries only the pose,
//     the cells and a few registers, the arrays ahead of the pad in ONE LDS allocation (16-bit offsets: no address
//     materialised per access), accumulators that die at their reduction, the series of the rotation at a quarter of the
//     angle (16 constants of two scalar moves each instead of 48), the normal equations in units of f.
//   * THE SERIAL SECTION DEALT TO LANES (round 5, lm_lanes.hpp).  Every lane of every wavefront used to compute all 27
//     entries of the (rvec, tvec)-space normal equations and the whole 6x6 LDL^T alike (~350 instructions a round).  Now
//     lane j of a 16-lane row holds column j: the totals of a pass are gathered per lane from LDS (6 loads instead of 27),
//     the two 3x3-block products and a Gauss-Jordan elimination run on v_fmac_f64_dpp ... row_newbcast (a DPP broadcast
//     folded into the FMA: 6 instructions for a row of outputs, 5 for an elimination step), the chain-rule matrices are
//     formed column-wise in the lanes while the exchange is in flight, and what a rejected trial needs again is 26
//     registers instead of an LDS stash.  Same-box A/B of the headline call: 0.1255-0.130 -> 0.1144-0.1155 ms.
//   * THE SELECTION IN THE PROLOGUE (a.fold_select: single frames of <= 256 hypotheses, the headline call).  softMax /
//     entropy statistics of the fp32 scores, the band of contenders and their re-score in reference arithmetic
//     (esac_util.h:235-260, 461-530 -- what k_select_rescore does in a launch of its own) run here: every member scores
//     ITS cells for every contender, one exchange adds them up, every member picks the winner from the same totals.  A
//     launch, its boundary and a 256-workgroup ramp less on a call whose selection re-scores one to three hypotheses.
// All members carry the same pose and take the same decisions from bitwise identical sums; member 0 writes the outputs,
// every member writes its cells of the inlier map once, at the end.
#include "refine_team.hpp"

namespace esac {

template <int CPL, int MODE = TEAM_SINGLE, int WIDE = 8>
__global__ __launch_bounds__(REFINE_B) void k_refine_team(KArgs a) {
    refine_team_body<CPL, MODE, WIDE, ROUTE_ANY>(a);
}

// Members of the team that refines a single frame (0: one workgroup refines): grids of 1024 .. 32768 cells; as many members
// as give every lane ONE cell (the pass is then as short as it gets: 19 at 60x80), at most what was asked for
// (esac_hip_set_refine_team) and the CUs of one XCD, at least so many that a member's slice fits its lanes' registers
// (four cells per lane); the device must hold the whole launch at once.
int refine_team_members(const KArgs& a) {
    const int P = a.H * a.W;
    if (a.team < 2 || P > TEAM_MAX * TEAM_CPL_MAX * REFINE_B || P < ESAC_REFINE_TEAM_MIN_CELLS || !a.coop_partials) return 0;
    if (a.errs) return 0;  // ESAC_DEBUG_ERROR_IMAGE: the error image is written by the one-workgroup kernel (k_refine)
    if (a.frames != 1) {  // a small batch: a team of 8 per frame (k_refine_team<CPL, TEAM_FRAMES>), all teams resident together
        return a.frames <= ESAC_TEAM_BATCH_MAX && P <= 8 * TEAM_CPL_MAX * REFINE_B && a.coop_max >= 8 * ESAC_TEAM_BATCH_MAX ? 8 : 0;
    }
    int G = (P + REFINE_B - 1) / REFINE_B;
    if (G > a.team) G = a.team;
    if (G > TEAM_MAX) G = TEAM_MAX;
    const int need = (P + TEAM_CPL_MAX * REFINE_B - 1) / (TEAM_CPL_MAX * REFINE_B);
    if (G < need) G = need;
    if (G < 2) G = 2;
    // the default size (round 6): a pass costs a lane its cells, and every lane of a member walks as many as its fullest lane
    // holds -- eight members of 600 cells hold THREE per lane on the 60x80 grid, ten of 480 hold two.  Up to 16 members exchange
    // without LDS staging (refine_common.hpp: team_collect_lds), so: the smallest team <= 16 that lowers the cells per lane.
    if (a.team_auto && a.team == ESAC_REFINE_TEAM_DEFAULT_K && G <= 16) {
        const int cpl = ((P + G - 1) / G + REFINE_B - 1) / REFINE_B;
        if (cpl >= 2) {
            const int G2 = (P + REFINE_B * (cpl - 1) - 1) / (REFINE_B * (cpl - 1));
            if (G2 > G && G2 <= 16) G = G2;
        }
    }
    if (a.coop_max < G * (a.team_stride > 0 ? a.team_stride : 8)) return 0;
    return G;
}

// Training path: a team of 8 per selection slot (k_refine_team<CPL, true>) -- grids whose eighth fits a member's registers
bool refine_slots_can_team(const KArgs& a) {
    const int P = a.H * a.W;
    return a.team >= 2 && a.frames == 1 && P >= ESAC_REFINE_TEAM_MIN_CELLS && P <= 8 * TEAM_CPL_MAX * REFINE_B && a.bwd.team_gran != nullptr;
}
unsigned long long launch_refine_slots_team(KArgs& a, hipStream_t s) {
    a.bwd.team_tag = next_refine_tag();
    a.bwd.team = 8;
    const int P = a.H * a.W;
    const int cpl = ((P + 7) / 8 + REFINE_B - 1) / REFINE_B;
    int cap = a.N < a.bwd.cap ? a.N : a.bwd.cap;
    if (cap > a.bwd.team_max_slots) cap = a.bwd.team_max_slots;  // (a selection of more slots is refined by launch_refine_slots)
    const dim3 grid((unsigned)((cap + 7) / 8) * 64), block(REFINE_B);
    switch (cpl) {
        case 1: hipLaunchKernelGGL((k_refine_team<1, TEAM_SLOTS>), grid, block, 0, s, a); break;
        case 2: hipLaunchKernelGGL((k_refine_team<2, TEAM_SLOTS>), grid, block, 0, s, a); break;
        case 3: hipLaunchKernelGGL((k_refine_team<3, TEAM_SLOTS>), grid, block, 0, s, a); break;
        default: hipLaunchKernelGGL((k_refine_team<4, TEAM_SLOTS>), grid, block, 0, s, a); break;
    }
    return a.bwd.team_tag;
}

// The selection can run in the team kernel's prologue: a team refines this call, one hypothesis per thread of a member, the
// default score route (ESAC_FLAG_EXACT_SCORES has statistics of its own), no device-side span stamps to reduce.
bool refine_folds_select(const KArgs& a) {
    return team_folds_select(refine_team_members(a), a.N, a.flags, a.tstamps != nullptr);
}
// ESAC_FLAG_EXACT_SCORES: the scores are final when the refinement starts; their softmax statistics and argmax are a few
// reductions over <= 256 values -- in the team kernel's prologue instead of a launch of their own (k_stats_exact)
bool refine_folds_exact_stats(const KArgs& a) {
    return team_folds_exact_stats(refine_team_members(a), a.N, a.flags);
}

unsigned long long launch_refine_team(const KArgs& a, hipStream_t s) {
    const int G = refine_team_members(a);
    KArgs b = a;
    if (b.team_stride <= 0) b.team_stride = 8;
    b.coop_tag = next_refine_tag();
    const int P = a.H * a.W;
    const int slice = (P + G - 1) / G;  // the largest member slice: floor((g+1) P / G) - floor(g P / G) <= ceil(P / G)
    const int cpl = (slice + REFINE_B - 1) / REFINE_B;
    if (a.frames != 1) {  // a team of 8 per frame, eight teams per 64 blocks (one per XCD)
        const dim3 grid((unsigned)((a.frames + 7) / 8) * 64), block(REFINE_B);
        switch (cpl) {
            case 1: hipLaunchKernelGGL((k_refine_team<1, TEAM_FRAMES>), grid, block, 0, s, b); break;
            case 2: hipLaunchKernelGGL((k_refine_team<2, TEAM_FRAMES>), grid, block, 0, s, b); break;
            case 3: hipLaunchKernelGGL((k_refine_team<3, TEAM_FRAMES>), grid, block, 0, s, b); break;
            default: hipLaunchKernelGGL((k_refine_team<4, TEAM_FRAMES>), grid, block, 0, s, b); break;
        }
        return b.coop_tag;
    }
    const dim3 grid(G * b.team_stride), block(REFINE_B);
    const bool route = refine_takes_route(RouteQuery{a.route != 0, a.frames, G, a.N, a.E, a.flags, a.fold_select, a.spec_mode, a.spec_gate, a.spec_debug,
                                                     a.coop_extra, a.errs != nullptr, a.tstamps != nullptr});
    if (route) {
        launch_refine_team_route(b, cpl, G, s);
        return b.coop_tag;
    }
    // one instantiation per (cells per lane, members it can collect): see team_collect_lds
#define ESAC_LAUNCH_TEAM(CPL_)                                                                                 \
    do {                                                                                                       \
        if (G <= 8)       hipLaunchKernelGGL((k_refine_team<CPL_, TEAM_SINGLE, 8>), grid, block, 0, s, b);     \
        else if (G <= 16) hipLaunchKernelGGL((k_refine_team<CPL_, TEAM_SINGLE, 16>), grid, block, 0, s, b);    \
        else              hipLaunchKernelGGL((k_refine_team<CPL_, TEAM_SINGLE, 32>), grid, block, 0, s, b);    \
    } while (0)
    switch (cpl) {
        case 1: ESAC_LAUNCH_TEAM(1); break;
        case 2: ESAC_LAUNCH_TEAM(2); break;
        case 3: ESAC_LAUNCH_TEAM(3); break;
        default: ESAC_LAUNCH_TEAM(4); break;
    }
#undef ESAC_LAUNCH_TEAM
    return b.coop_tag;
}

}  // namespace esac
