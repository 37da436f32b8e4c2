// esac_refine_team_route.hip -- the refinement team's ROUTE kernel: the body of k_refine_team (refine_team.hpp) with the headline
// call's combination of modes as compile-time constants -- fold_select == 2 (ESAC_FLAG_EXACT_SCORES: softmax statistics and
// argmax of the final scores in the prologue), no speculation, one expert, no debug knob.  A single frame, a team of at most 16
// members; launch_refine_team (esac_refine_team.hip) takes it where refine_takes_route (refine_route_policy.hpp) says so, and
// every other launch keeps the general kernel.  Same arithmetic, same exchanges, same outputs bit for bit
// (tests/test_gpu_headline_route.py); what is gone is the code of the modes not taken and the scalar registers and spills their
// branches kept alive through the start-up and the record (tests/test_headline_route_isa_budget.py).
// A translation unit of its own: the two kinds of kernel compile side by side.
#include "refine_team.hpp"

namespace esac {

template <int CPL, int WIDE>
__global__ __launch_bounds__(REFINE_B) void k_refine_team_route(KArgs a) {
    refine_team_body<CPL, TEAM_SINGLE, WIDE, ROUTE_HEADLINE>(a);
}

// b: the launch's argument block as launch_refine_team made it (tag, stride); cpl: cells per lane of the largest slice
void launch_refine_team_route(const KArgs& b, int cpl, int G, hipStream_t s) {
    const dim3 grid(G * b.team_stride), block(REFINE_B);
#define ESAC_LAUNCH_ROUTE(CPL_)                                                                        \
    do {                                                                                               \
        if (G <= 8) hipLaunchKernelGGL((k_refine_team_route<CPL_, 8>), grid, block, 0, s, b);          \
        else        hipLaunchKernelGGL((k_refine_team_route<CPL_, 16>), grid, block, 0, s, b);         \
    } while (0)
    switch (cpl) {
        case 1: ESAC_LAUNCH_ROUTE(1); break;
        case 2: ESAC_LAUNCH_ROUTE(2); break;
        case 3: ESAC_LAUNCH_ROUTE(3); break;
        default: ESAC_LAUNCH_ROUTE(4); break;
    }
#undef ESAC_LAUNCH_ROUTE
}

}  // namespace esac
