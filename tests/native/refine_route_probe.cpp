// refine_route_probe.cpp -- stand-alone host program over esac_amd/csrc/refine_route_policy.hpp (no HIP header, no GPU): which
// kernel a single frame's refinement team runs, as tests/test_refine_route_policy.py drives it.
// One request per input line, one answer per output line:
//   call enabled fold_enabled caller_flags frames members N E H W spec_mode spec_gate spec_debug coop_extra errs tstamps
//        -> call|<flags with the implied ones>|<fold_select>|<route 0/1>
//        (the flags as the host derives them -- call_scalars, auto_exact_flags -- and fold_select as serial_fold does)
//   raw  enabled frames members N E flags fold_select spec_mode spec_gate spec_debug coop_extra errs tstamps
//        -> raw|<route 0/1>                                           (the predicate alone, every field as given)
#include <stdio.h>
#include <string.h>

#include <sstream>
#include <string>

#include "../../esac_amd/csrc/call_policy.hpp"
#include "../../esac_amd/csrc/refine_route_policy.hpp"

using namespace esac;

static_assert(ROUTE_FLAG_EXACT_SCORES == ESAC_FLAG_EXACT_SCORES && ROUTE_FLAG_STRICT_REFERENCE == ESAC_FLAG_STRICT_REFERENCE, "mirrors of include/esac_hip.h");

int main() {
    char line[4096];
    while (fgets(line, sizeof(line), stdin)) {
        std::istringstream in(line);
        std::string kind;
        if (!(in >> kind)) continue;
        if (kind == "call") {
            int enabled, fold_enabled, caller_flags, frames, members, N, E, H, W, spec_mode, spec_gate, spec_debug, coop_extra, errs, tstamps;
            in >> enabled >> fold_enabled >> caller_flags >> frames >> members >> N >> E >> H >> W >> spec_mode >> spec_gate >> spec_debug >> coop_extra >> errs >> tstamps;
            if (!in) { printf("call|bad row\n"); continue; }
            esac_hip_params p;
            memset(&p, 0, sizeof(p));
            p.E = E; p.H = H; p.W = W; p.N = N;
            p.inlier_alpha = 100.0f; p.sub_sampling = 8; p.max_ref_steps = -1;
            p.flags = caller_flags;
            const int flags = auto_exact_flags(call_scalars(&p, N).flags, frames, E, N, H, W);
            const int fold = team_fold_select(fold_enabled != 0, members, N, flags, tstamps != 0);
            const RouteQuery q{enabled != 0, frames, members, N, E, flags, fold, spec_mode, spec_gate, spec_debug, coop_extra, errs != 0, tstamps != 0};
            printf("call|%d|%d|%d\n", flags, fold, (int)refine_takes_route(q));
        } else if (kind == "raw") {
            int enabled, frames, members, N, E, flags, fold, spec_mode, spec_gate, spec_debug, coop_extra, errs, tstamps;
            in >> enabled >> frames >> members >> N >> E >> flags >> fold >> spec_mode >> spec_gate >> spec_debug >> coop_extra >> errs >> tstamps;
            if (!in) { printf("raw|bad row\n"); continue; }
            const RouteQuery q{enabled != 0, frames, members, N, E, flags, fold, spec_mode, spec_gate, spec_debug, coop_extra, errs != 0, tstamps != 0};
            printf("raw|%d\n", (int)refine_takes_route(q));
        } else {
            printf("%s|unknown request\n", kind.c_str());
        }
    }
    return 0;
}
