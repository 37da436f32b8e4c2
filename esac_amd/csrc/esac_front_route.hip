// esac_front_route.hip -- the two kernels in FRONT of the refinement team on the headline call, with that call's combination of
// modes as compile-time constants: the sampler k_sample_route<256, 2> and the exact score k_rescore_route<1024, CPL>.
// forward_impl (esac_capi.hip) takes them where front_takes_route (front_route_policy.hpp) says so -- a single frame on the serial
// route, one expert, at most 256 hypotheses, ESAC_FLAG_EXACT_SCORES in force, no table, packed map, index list, speculation or
// debug buffer -- and every other call, every stage entry point, the training path and the batches keep the general kernels of
// esac_kernels.hip.  Same draws, same arithmetic, same summation order, same outputs bit for bit (tests/test_gpu_front_route.py),
// with ONE exception that is the point: the sampler stores no fp32 [R | t] rows (KArgs::rt32).  No kernel of such a call reads
// them; the context marks them stale, and the first stage that does read them forms them from the stored (rvec, tvec) --
// k_hyps_to_rt32, the rows esac_hip_write_hyps always got.
// A translation unit of its own: the general kernels keep their code (tests/test_headline_isa_budget.py).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pose_math.hpp"
#include "rng.hpp"
#include "esac_kernels.hpp"
#include "device_common.hpp"
#include "select_math.hpp"
#include "sample_helpers.hpp"
#include "front_route_policy.hpp"

#ifndef ESAC_FRONT_ROUTE_RT32
#define ESAC_FRONT_ROUTE_RT32 0  // 1 (measurement builds: -DESAC_FRONT_ROUTE_RT32=1): the route sampler stores the fp32 rows after all
#endif
#ifndef ESAC_FRONT_ROUTE_DIV
#define ESAC_FRONT_ROUTE_DIV 0   // 1 (measurement builds): the route scorer divides by W for every cell, as the general kernel does
#endif

namespace esac {

// The fields of the argument block whose value eligibility fixes, as constants: every branch on them folds away, and the
// scalar registers that carried them through the try loop are free.
__device__ __forceinline__ void front_route_modes(KArgs& a) {
    a.E = 1;
    a.frames = 1;
    a.cams = nullptr;
    a.shapes = 0;
    a.sc4 = nullptr;
    a.hyp_index = nullptr;
    a.hyp_offset = 0;
    a.first_try = 0;
    a.handover = 0x7fffffff;
    a.spec_flag = nullptr;
}

#define ESAC_K_SAMPLE_FIRST k_sample_first_route_unused
#define ESAC_K_SAMPLE k_sample_route
#define ESAC_SAMPLE_ALIGN AlignTriad
#define ESAC_SAMPLE_FIRST_ATTR
#define ESAC_SAMPLE_ROUTE 1
#define ESAC_SAMPLE_RT32 ESAC_FRONT_ROUTE_RT32
#include "sample_kernels.inc.hpp"
#undef ESAC_K_SAMPLE_FIRST
#undef ESAC_K_SAMPLE
#undef ESAC_SAMPLE_ALIGN
#undef ESAC_SAMPLE_FIRST_ATTR
#undef ESAC_SAMPLE_ROUTE
#undef ESAC_SAMPLE_RT32

// The exact score of hypothesis blockIdx.x: rescore_body / block_exact_score (select_math.hpp) for ONE hypothesis per workgroup
// on one expert's map.  A lane's cells are threadIdx.x + k * B, k < CPL -- their addresses depend on nothing but the thread
// index, so all of the lane's loads (3 * CPL map values, the hypothesis' R and t) are issued before the first use and share
// one trip to memory; in the general kernel each cell's loads sit behind the previous cell's ~120-operation chain.  The lane
// then adds its cells' terms in ascending cell order into one accumulator and the workgroup sums with block_sum<1, B>: the
// general kernel's order, term for term.  (row, col) of a cell: ONE 32-bit division by W for the lane's first cell; every next
// cell is B cells on, i.e. B / W rows and B % W columns (both uniform) with at most one carry -- the same integers.
template <int B, int CPL>
__global__ __launch_bounds__(B) void k_rescore_route(KArgs a) {
    __shared__ double s_part[B / 64];
    __shared__ double s_tot[1];
    front_route_modes(a);
    const int h = blockIdx.x;
    const int P = a.H * a.W;
    const Cam cam = make_cam(a);
    const float* __restrict__ mx = a.sc;
    float X[CPL], Y[CPL], Z[CPL];
#pragma unroll
    for (int k = 0; k < CPL; k++) {
        const int i = (int)threadIdx.x + k * B;
        const int ic = i < P ? i : 0;  // (a lane past the grid's end loads cell 0 and uses nothing of it)
        X[k] = mx[ic];
        Y[k] = mx[P + ic];
        Z[k] = mx[2 * P + ic];
    }
    const double* hp = a.hyps + (size_t)h * 6;
    const double t[3] = {hp[3], hp[4], hp[5]};
    double R[9];
#pragma unroll
    for (int k = 0; k < 9; k++) R[k] = a.hyps_R[(size_t)h * 9 + k];
    double acc[1] = {0};
    const int step_row = B / a.W, step_col = B - step_row * a.W;
    int row = (int)threadIdx.x / a.W, col = (int)threadIdx.x - row * a.W;
#pragma unroll
    for (int k = 0; k < CPL; k++) {
        const int i = (int)threadIdx.x + k * B;
        if (ESAC_FRONT_ROUTE_DIV) row = i / a.W, col = i - row * a.W;
        if (i < P) acc[0] += exact_cell_term<false>(R, t, cam, X[k], Y[k], Z[k], cell_px(a, col), cell_py(a, row), a.max_reproj, a.tau, a.beta);
        col += step_col;
        row += step_row;
        if (col >= a.W) col -= a.W, row++;
    }
    block_sum<1, B>(acc, s_part, s_tot);
    if (threadIdx.x == 0) store_score(a, h, exact_score_scaled(acc[0], a.alpha, a.W, a.H), 1);
}

void launch_sample_route(const KArgs& a, hipStream_t s) {
    hipLaunchKernelGGL((k_sample_route<256, 2>), dim3(a.N), dim3(256), 0, s, a);
}

void launch_rescore_route(const KArgs& a, hipStream_t s) {
    constexpr int B = FRONT_ROUTE_SCORE_THREADS;
    static_assert(FRONT_ROUTE_MAX_CELLS == 8 * B, "the scorer is instantiated for 1..8 cells per lane");
    const dim3 grid(a.N), block(B);
    switch ((a.H * a.W + B - 1) / B) {
        case 1: hipLaunchKernelGGL((k_rescore_route<B, 1>), grid, block, 0, s, a); break;
        case 2: hipLaunchKernelGGL((k_rescore_route<B, 2>), grid, block, 0, s, a); break;
        case 3: hipLaunchKernelGGL((k_rescore_route<B, 3>), grid, block, 0, s, a); break;
        case 4: hipLaunchKernelGGL((k_rescore_route<B, 4>), grid, block, 0, s, a); break;
        case 5: hipLaunchKernelGGL((k_rescore_route<B, 5>), grid, block, 0, s, a); break;
        case 6: hipLaunchKernelGGL((k_rescore_route<B, 6>), grid, block, 0, s, a); break;
        case 7: hipLaunchKernelGGL((k_rescore_route<B, 7>), grid, block, 0, s, a); break;
        default: hipLaunchKernelGGL((k_rescore_route<B, 8>), grid, block, 0, s, a); break;  // (front_takes_route: at most 8)
    }
}

}  // namespace esac
