// device_math_probe.hip -- TEST-ONLY: the math headers of the kernels, function by function, ON THE DEVICE.
//
// tests/native/host_math_probe.cpp compiles pose_math.hpp / lm_math.hpp / lm_lanes.hpp / bwd_math.hpp / p3p_screen.hpp for
// the host, where every `#if defined(__HIP_DEVICE_COMPILE__)` branch takes its #else side: 1.0 / d for fast_rcp, sqrt / cos /
// sin for the trigonometric route of lm_pose_rotation, a 16-lane emulation (or stubs) for the DPP row of lm_lanes.hpp.  This
// file compiles the SAME headers, unchanged, for gfx950 with the product's own flags and runs each routine on inputs the
// tests choose (tests/device_math_cases.py), so that the text the GPU executes -- v_rcp_f64 / v_rsq_f64 + Newton, the
// interleaved reciprocals and asm 0/1 weights of lm_point_terms, row_newbcast FMAs with hand-managed hazard padding, the
// one-lane Jacobi sweeps of lm_solve6_pinv -- is held to a reference per function (tests/test_gpu_device_math.py).
// Every launcher takes HOST arrays, copies, launches one small kernel, copies back and returns the HIP status (0 = fine).
// Built by tests/native/build.py:build_device_math_probe().
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "math_probe_bodies.hpp"
#include "../../esac_amd/csrc/refine_common.hpp"

using namespace esac;
using namespace esac_probe;

namespace {

__global__ __launch_bounds__(64) void k_scalars(int op, int n, const double* __restrict__ in, double* __restrict__ out) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i < n) out[i] = body_scalar(op, in[i]);
}

__global__ __launch_bounds__(64) void k_rotation(int n, const double* __restrict__ in, double* __restrict__ out) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i < n) body_rotation(in + (size_t)6 * i, out + (size_t)ROT_OUT * i);
}

template <int NP>
__global__ __launch_bounds__(64) void k_point_terms(int n, const double* __restrict__ in, double* __restrict__ out) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i < n) body_point_terms<NP>(in + (size_t)PT_IN * i, out + (size_t)PT_OUT * i);
}

__global__ __launch_bounds__(64) void k_solves(int n, const double* __restrict__ in, double* __restrict__ out) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i < n) body_solves(in + (size_t)SOLVE_IN * i, out + (size_t)SOLVE_OUT * i);
}

// One wavefront per case, set up as k_refine_team sets a wavefront up for team_step (esac_refine_team.hip): the totals of a
// pass in LDS at [0, 27), their negatives at [32, 59), zeros between; lane l gathers its X_k / Y_k through
// lm_lane_slot(l & 15, .); hot[k] is 1 in lane k of every row, keep is 1 in lanes 3..6.  Then the sequence of a fresh step
// followed by a rejected trial: the second solve re-uses c, dg with another lambda BEHIND A UNIFORM BRANCH TAKEN FROM DATA
// (the first DPP operation behind a branch is what the s_nop 4 of lane_gj_step<0> is for).
// The system is written out before and after that solve (c must not change by a bit) and a third, straight-line solve at
// the same lambda follows (stale registers or a short hazard pad behind the branch would make the two differ).
__global__ __launch_bounds__(64) void k_lane_step(const double* __restrict__ in, double* __restrict__ out) {
    __shared__ double lds[LM_LANE_SLOTS];
    const int lane = threadIdx.x, l16 = lane & 15;
    const double* q = in + (size_t)LANE_IN * blockIdx.x;
    lds[lane] = 0.0;
    __syncthreads();
    if (lane < 27) {
        lds[lane] = q[lane];
        lds[LM_LANE_NEG + lane] = -q[lane];
    }
    __syncthreads();
    double X[3], Y[3], hot[6], keep, M[3], K[3], c[6], dg, dx1[6], dx2[6], dx3[6], U[21], g[6];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        X[k] = lds[lm_lane_slot(l16, k)];
        Y[k] = lds[lm_lane_slot(l16, 3 + k)];
    }
#pragma unroll
    for (int k = 0; k < 6; k++) hot[k] = l16 == k ? 1.0 : 0.0;
    keep = (l16 >= 3 && l16 <= 6) ? 1.0 : 0.0;
    double pose[6], R[9];
#pragma unroll
    for (int k = 0; k < 6; k++) pose[k] = q[27 + k];
    const double lambda1 = q[33], lambda2 = q[34];
    LmTrig tg;
    lm_pose_rotation(pose, R, tg);
    lm_lane_chain<double>(tg, pose + 3, hot, M, K);
    lm_lane_transform<double>(X, Y, M, K, hot, keep, c, dg);
    const bool ok1 = lm_lane_solve<double>(c, dg, hot, lambda1, dx1);
    lm_lane_to_u21<double>(c, U, g);  // the system BEFORE the rejected trial ...
    double* o = out + ((size_t)blockIdx.x * 64 + lane) * LANE_OUT;
#pragma unroll
    for (int k = 0; k < 21; k++) o[k] = U[k];
#pragma unroll
    for (int k = 0; k < 6; k++) o[21 + k] = g[k];
    bool ok2 = false;
#pragma unroll
    for (int k = 0; k < 6; k++) dx2[k] = 0.0;
    if (lambda2 >= 0.0) ok2 = lm_lane_solve<double>(c, dg, hot, lambda2, dx2);  // (always taken: the compiler cannot know)
    lm_lane_to_u21<double>(c, U, g);  // ... and AFTER it: c must be untouched, bit for bit
    // a third, straight-line solve at the same lambda (through a value the optimiser cannot identify with lambda2, so that
    // it is not merged with the one behind the branch): must equal the second bit for bit
    double lambda3 = lambda2;
    asm volatile("" : "+v"(lambda3));
    const bool ok3 = lm_lane_solve<double>(c, dg, hot, lambda3, dx3);
#pragma unroll
    for (int k = 0; k < 6; k++) {
        o[27 + k] = dx1[k];
        o[33 + k] = dx2[k];
        o[39 + k] = dx3[k];
    }
    o[45] = ok1 ? 1.0 : 0.0;
    o[46] = ok2 ? 1.0 : 0.0;
    o[47] = ok3 ? 1.0 : 0.0;
#pragma unroll
    for (int k = 0; k < 21; k++) o[48 + k] = U[k];
#pragma unroll
    for (int k = 0; k < 6; k++) o[69 + k] = g[k];
}

// lm_solve6_pinv in a workgroup of the refinement kernels' size: in: U21[21], g6[6], lambda; out: dx[6] of EVERY thread
__global__ __launch_bounds__(REFINE_B) void k_pinv_step(const double* __restrict__ in, double* __restrict__ out) {
    __shared__ double lds[84];
    const double* q = in + (size_t)SOLVE_IN * blockIdx.x;
    double U21[21], g[6], dx[6];
#pragma unroll
    for (int k = 0; k < 21; k++) U21[k] = q[k];
#pragma unroll
    for (int k = 0; k < 6; k++) g[k] = q[21 + k];
    lm_solve6_pinv(U21, g, q[27], dx, lds);
    double* o = out + ((size_t)blockIdx.x * REFINE_B + threadIdx.x) * 6;
#pragma unroll
    for (int k = 0; k < 6; k++) o[k] = dx[k];
}

// host arrays in and out around one launch
template <class Launch>
int run(const double* h_in, size_t n_in, double* h_out, size_t n_out, Launch launch) {
    double *d_in = nullptr, *d_out = nullptr;
    if (hipMalloc((void**)&d_in, n_in * sizeof(double)) != hipSuccess) return 1;
    if (hipMalloc((void**)&d_out, n_out * sizeof(double)) != hipSuccess) {
        (void)hipFree(d_in);
        return 1;
    }
    hipError_t e = hipMemcpy(d_in, h_in, n_in * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(d_out, 0xff, n_out * sizeof(double));  // (NaN: an output nobody wrote shows)
    if (e == hipSuccess) {
        launch(d_in, d_out);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(h_out, d_out, n_out * sizeof(double), hipMemcpyDeviceToHost);
    (void)hipFree(d_in);
    (void)hipFree(d_out);
    return e == hipSuccess ? 0 : (int)e;
}

}  // namespace

extern "C" {
int dev_scalars(int op, int n, const double* in, double* out) {
    if (n <= 0 || op < 0 || op > 4) return -1;
    return run(in, n, out, n, [&](const double* di, double* dout) { hipLaunchKernelGGL(k_scalars, dim3((n + 63) / 64), dim3(64), 0, 0, op, n, di, dout); });
}
int dev_rotation(int n, const double* in, double* out) {
    if (n <= 0) return -1;
    return run(in, (size_t)6 * n, out, (size_t)ROT_OUT * n,
               [&](const double* di, double* dout) { hipLaunchKernelGGL(k_rotation, dim3((n + 63) / 64), dim3(64), 0, 0, n, di, dout); });
}
int dev_point_terms(int np, int n, const double* in, double* out) {
    if (n <= 0 || np < 1 || np > 4) return -1;
    return run(in, (size_t)PT_IN * n, out, (size_t)PT_OUT * n, [&](const double* di, double* dout) {
        const dim3 grid((n + 63) / 64), block(64);
        if (np == 1) hipLaunchKernelGGL(k_point_terms<1>, grid, block, 0, 0, n, di, dout);
        if (np == 2) hipLaunchKernelGGL(k_point_terms<2>, grid, block, 0, 0, n, di, dout);
        if (np == 3) hipLaunchKernelGGL(k_point_terms<3>, grid, block, 0, 0, n, di, dout);
        if (np == 4) hipLaunchKernelGGL(k_point_terms<4>, grid, block, 0, 0, n, di, dout);
    });
}
int dev_solves(int n, const double* in, double* out) {
    if (n <= 0) return -1;
    return run(in, (size_t)SOLVE_IN * n, out, (size_t)SOLVE_OUT * n,
               [&](const double* di, double* dout) { hipLaunchKernelGGL(k_solves, dim3((n + 63) / 64), dim3(64), 0, 0, n, di, dout); });
}
// out: [n][64 lanes][LANE_OUT]
int dev_lane_step(int n, const double* in, double* out) {
    if (n <= 0) return -1;
    return run(in, (size_t)LANE_IN * n, out, (size_t)LANE_OUT * 64 * n,
               [&](const double* di, double* dout) { hipLaunchKernelGGL(k_lane_step, dim3(n), dim3(64), 0, 0, di, dout); });
}
// out: [n][dev_pinv_threads()][6]
int dev_pinv_threads(void) { return REFINE_B; }
int dev_pinv_step(int n, const double* in, double* out) {
    if (n <= 0) return -1;
    return run(in, (size_t)SOLVE_IN * n, out, (size_t)6 * REFINE_B * n,
               [&](const double* di, double* dout) { hipLaunchKernelGGL(k_pinv_step, dim3(n), dim3(REFINE_B), 0, 0, di, dout); });
}
}
