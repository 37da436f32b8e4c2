// sample_plan_probe.cpp -- TEST-ONLY: the sampler's launch plan (esac_amd/csrc/sample_plan.hpp, plain C++) behind a C entry point,
// so that the CPU suite can hold it against a table of what the launchers decided before the plan existed.
// Built by tests/native/build.py (build_sample_plan_probe).  Not part of the product library.
#include "../../esac_amd/csrc/sample_plan.hpp"
extern "C" void probe_sample_plan(int N, int frames, int E, int max_tries, int flags, int first_try, int packed, int out[13]) {
    const esac::SamplePlan p = esac::sample_plan(N, frames, E, max_tries, flags, first_try, packed != 0);
    const int v[13] = {p.pack, p.strict, p.first, p.grid_x, p.block, p.passes, p.pass_tries, p.handover, p.tail, p.pending_list,
                       p.tail_first_try, p.chain_waves, p.splittable};
    for (int i = 0; i < 13; i++) out[i] = v[i];
}
