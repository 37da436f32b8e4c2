// esac_verify.hip -- esac_hip_verify_batch: K given poses per frame, each evaluated against one expert's scene-coordinate map of
// its frame -- the reference-arithmetic soft-inlier score, the inlier set of the refinement's rule, and over it the normal matrix,
// the residual sum of squares and the covariance sigma^2 A^-1 (verify_math.hpp: the text the host probe compiles).
// One workgroup of 256 threads per (pose k, frame b), grid (K, B); the frame's camera and grid through frame_view like every batch
// kernel.  The pose is uniform over the workgroup: every lane expands R and dR/dr itself (no LDS broadcast, no barrier in front of
// the loop).  Thread t walks the cells t, t + 256, ... of the frame's own h_b * w_b, VERIFY_UNROLL at a time with their fp64
// chains side by side (gfx950 issues in order; a dependent fp64 op is ~32 cycles away), 24 fp64 sums per lane, combined by
// block_sum28 in its fixed order: a row depends on the pose, the map and the camera, never on the batch around it.
// Reads 12 bytes per cell and pose (three coalesced planes); writes one row of 64 doubles with plain vector stores; no atomics,
// no workspace, one launch on the caller's stream.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_common.hpp"
#include "esac_kernels.hpp"
#include "verify_math.hpp"

namespace esac {

constexpr int VERIFY_THREADS = 256;
// cells per lane side by side; -DESAC_VERIFY_UNROLL=n builds an A/B variant (LAB_NOTES, "Pose verification": 1, 2 and 4 measured).
// The sums are taken in the same order whatever it is
#ifndef ESAC_VERIFY_UNROLL
#define ESAC_VERIFY_UNROLL 4
#endif
constexpr int VERIFY_UNROLL = ESAC_VERIFY_UNROLL;

// the rolled pseudo-inverse over LDS (bwd_math.hpp: operation by operation pinv_sym6_jacobi): the one lane that finishes a row
// runs it, on the rare degenerate inlier set
struct VerifyPinvLds {
    double* lds;  // >= 108 doubles
    __device__ __forceinline__ void operator()(const double (&U21)[21], double (&Ainv)[36]) const {
        pinv_sym6_rolled(U21, lds, lds + 36, lds + 72);
#pragma unroll
        for (int i = 0; i < 36; i++) Ainv[i] = lds[72 + i];
    }
};

template <bool STRICT>
__global__ __launch_bounds__(VERIFY_THREADS) void k_verify_batch(KArgs a, VerifyArgs v) {
    __shared__ double s_part[28 * (VERIFY_THREADS / 64)];
    __shared__ double s_tot[28];
    __shared__ double s_row[ESAC_VERIFY_DOUBLES_K];
    __shared__ double s_pinv[108];
    const int b = (int)blockIdx.y;
    frame_view(a, b);
    const size_t idx = (size_t)b * v.K + blockIdx.x;
    double* __restrict__ dst = v.out + idx * ESAC_VERIFY_DOUBLES_K;

    // the expert is checked before any address is formed from it; a bad pose or expert is the row's outcome (workgroup-uniform)
    const int e = v.experts[idx];
    double pose[6];
    const bool pose_ok = verify_fetch_pose(v.poses, v.format, idx, pose);
    const bool expert_ok = (unsigned)e < (unsigned)a.E;
    if (!expert_ok || !pose_ok) {
        if (threadIdx.x == 0) verify_row_nan(expert_ok ? ESAC_VERIFY_BAD_POSE_K : ESAC_VERIFY_BAD_EXPERT_K, s_row);
        __syncthreads();
        if (threadIdx.x < ESAC_VERIFY_DOUBLES_K) dst[threadIdx.x] = s_row[threadIdx.x];
        return;
    }

    const int P = a.H * a.W;
    const float* __restrict__ mx = a.sc + (size_t)e * 3 * P;
    const Cam cam = make_cam(a);
    const double rv[3] = {pose[0], pose[1], pose[2]};
    const double t[3] = {pose[3], pose[4], pose[5]};
    double R[9], dRdr[27];
    rodrigues_vec2mat<true>(rv, R, dRdr);

    double acc[VERIFY_ACC];
#pragma unroll
    for (int k = 0; k < VERIFY_ACC; k++) acc[k] = 0;
    for (int base = 0; base < P; base += VERIFY_THREADS * VERIFY_UNROLL) {
        float X[VERIFY_UNROLL], Y[VERIFY_UNROLL], Z[VERIFY_UNROLL], px[VERIFY_UNROLL], py[VERIFY_UNROLL];
        bool live[VERIFY_UNROLL];
#pragma unroll
        for (int u = 0; u < VERIFY_UNROLL; u++) {
            const int i = base + u * VERIFY_THREADS + (int)threadIdx.x;
            live[u] = i < P;
            const int j = live[u] ? i : 0;  // (a lane past the end reads cell 0 and adds selected zeros)
            const int row = j / a.W, col = j - row * a.W;
            X[u] = mx[j];
            Y[u] = mx[P + j];
            Z[u] = mx[2 * P + j];
            px[u] = cell_px(a, col);
            py[u] = cell_py(a, row);
        }
        verify_accumulate<STRICT, VERIFY_UNROLL>(R, dRdr, t, cam, X, Y, Z, px, py, live, a.tau, a.beta, a.max_reproj, acc);
    }
    block_sum28<VERIFY_ACC, VERIFY_THREADS>(acc, s_part, s_tot);
    if (threadIdx.x == 0) verify_finish(acc, a.alpha, a.W, a.H, VerifyPinvLds{s_pinv}, s_row);
    __syncthreads();
    if (threadIdx.x < ESAC_VERIFY_DOUBLES_K) dst[threadIdx.x] = s_row[threadIdx.x];
}

void launch_verify_batch(const KArgs& a, const VerifyArgs& v, hipStream_t s) {
    const dim3 grid((unsigned)v.K, (unsigned)a.frames);
    if (a.flags & ESAC_FLAG_STRICT_REFERENCE_K) hipLaunchKernelGGL(k_verify_batch<true>, grid, dim3(VERIFY_THREADS), 0, s, a, v);
    else hipLaunchKernelGGL(k_verify_batch<false>, grid, dim3(VERIFY_THREADS), 0, s, a, v);
}

}  // namespace esac
