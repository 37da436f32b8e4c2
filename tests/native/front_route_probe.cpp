// front_route_probe.cpp -- stand-alone host program over esac_amd/csrc/front_route_policy.hpp (no HIP header, no GPU): which
// kernels sample and score a forward call, as tests/test_front_route_policy.py drives it.
// One request per input line, one answer per output line:
//   call enabled serial caller_flags frames N E H W max_tries first_try hyp_offset cams shapes pack_flag hyp_index spec_flag tstamps errs
//        -> call|<flags with the implied ones>|<max_tries>|<packed 0/1>|<route 0/1>
//        (flags, budget and packing as the host derives them: call_scalars, auto_exact_flags, want_pack)
//   raw  enabled serial frames N E H W flags max_tries first_try hyp_offset cams shapes packed hyp_index spec_flag tstamps errs
//        -> raw|<route 0/1>                                           (the predicate alone, every field as given)
#include <stdio.h>
#include <string.h>

#include <sstream>
#include <string>

#include "../../esac_amd/csrc/call_policy.hpp"
#include "../../esac_amd/csrc/front_route_policy.hpp"

using namespace esac;

static_assert(FRONT_FLAG_EXACT_SCORES == ESAC_FLAG_EXACT_SCORES && ESAC_FLAG_STRICT_REFERENCE_K == ESAC_FLAG_STRICT_REFERENCE &&
              ESAC_FLAG_EXACT_SAMPLING_K == ESAC_FLAG_EXACT_SAMPLING, "mirrors of include/esac_hip.h");

int main() {
    char line[4096];
    while (fgets(line, sizeof(line), stdin)) {
        std::istringstream in(line);
        std::string kind;
        if (!(in >> kind)) continue;
        if (kind == "call") {
            int enabled, serial, caller_flags, frames, N, E, H, W, max_tries, first_try, hyp_offset, cams, shapes, pack_flag, hyp_index, spec_flag, tstamps, errs;
            in >> enabled >> serial >> caller_flags >> frames >> N >> E >> H >> W >> max_tries >> first_try >> hyp_offset >> cams >> shapes >> pack_flag >>
                hyp_index >> spec_flag >> tstamps >> errs;
            if (!in) { printf("call|bad row\n"); continue; }
            esac_hip_params p;
            memset(&p, 0, sizeof(p));
            p.E = E; p.H = H; p.W = W; p.N = N;
            p.inlier_alpha = 100.0f; p.sub_sampling = 8; p.max_ref_steps = -1; p.max_tries = max_tries;
            p.flags = caller_flags | (pack_flag ? ESAC_FLAG_PACK_MAPS : 0);
            const CallScalars v = call_scalars(&p, N);
            const int flags = auto_exact_flags(v.flags, frames, E, N, H, W);
            const bool packed = want_pack(&p, frames);
            const FrontRouteQuery q{enabled != 0, serial != 0, frames, N, E, H, W, flags, v.max_tries, first_try, hyp_offset, cams != 0, shapes, packed,
                                    hyp_index != 0, spec_flag != 0, tstamps != 0, errs != 0};
            printf("call|%d|%d|%d|%d\n", flags, v.max_tries, (int)packed, (int)front_takes_route(q));
        } else if (kind == "raw") {
            int enabled, serial, frames, N, E, H, W, flags, max_tries, first_try, hyp_offset, cams, shapes, packed, hyp_index, spec_flag, tstamps, errs;
            in >> enabled >> serial >> frames >> N >> E >> H >> W >> flags >> max_tries >> first_try >> hyp_offset >> cams >> shapes >> packed >> hyp_index >>
                spec_flag >> tstamps >> errs;
            if (!in) { printf("raw|bad row\n"); continue; }
            const FrontRouteQuery q{enabled != 0, serial != 0, frames, N, E, H, W, flags, max_tries, first_try, hyp_offset, cams != 0, shapes, packed != 0,
                                    hyp_index != 0, spec_flag != 0, tstamps != 0, errs != 0};
            printf("raw|%d\n", (int)front_takes_route(q));
        } else {
            printf("%s|unknown request\n", kind.c_str());
        }
    }
    return 0;
}
