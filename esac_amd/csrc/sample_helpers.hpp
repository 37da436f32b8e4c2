// sample_helpers.hpp -- the device helpers of the fp64 sampling kernels (sample_kernels.inc.hpp): the cells of a try, the
// acceptance test of a solved sample and the stores of an accepted hypothesis.  ONE definition for the two translation units that
// compile such kernels: esac_kernels.hip (every caller's) and esac_front_route.hip (the headline call's route sampler).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pose_math.hpp"
#include "rng.hpp"
#include "esac_kernels.hpp"
#include "device_common.hpp"

namespace esac {

// Stored pose and acceptance of a solved sample: the reference keeps (rvec, tvec), re-expands it when projecting
// (esac_util.h:202) and accepts iff the 4 sampled points reproject within tau (esac_util.h:210-221, norm in double).
__device__ __forceinline__ bool accept_sample(const double Rp[9], const double Tp[3], const float (&Pf)[4][3], const double (&mu)[4],
                                              const double (&mv)[4], const Cam& cam, double tau, double rvec[3], double T[3],
                                              double R[9]) {
    rodrigues_mat2vec(Rp, rvec);
    rodrigues_vec2mat<false>(rvec, R, nullptr);
    T[0] = Tp[0]; T[1] = Tp[1]; T[2] = Tp[2];
    bool accepted = true;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const double Xd = Pf[j][0], Yd = Pf[j][1], Zd = Pf[j][2];
        double x = R[0] * Xd + R[1] * Yd + R[2] * Zd + T[0];
        double y = R[3] * Xd + R[4] * Yd + R[5] * Zd + T[1];
        double z = R[6] * Xd + R[7] * Yd + R[8] * Zd + T[2];
        z = z ? 1. / z : 1;
        x *= z;
        y *= z;
        const float u = (float)(x * cam.fx + cam.cx), v = (float)(y * cam.fy + cam.cy);
        const float dx = (float)mu[j] - u, dy = (float)mv[j] - v;
        const double nrm = sqrt((double)dx * dx + (double)dy * dy);
        if (nrm < tau) continue;
        accepted = false;
    }
    return accepted;
}

// A solved sample whose 4th point already misses tau by a clear margin under the chosen candidate cannot pass the
// acceptance test: the stored pose differs from the candidate only by the rvec round trip (~1e-12 px) and the
// reference's float rounding of the projection (< 1e-4 px).  Such a try needs neither the matrix->vector->matrix
// conversion nor the four reprojections -- unless it is the LAST try of the budget, whose state must remain.
__device__ __forceinline__ bool cannot_pass(double reproj2, double tau) {
    const double lim = tau + 0.01;
    return reproj2 > lim * lim;  // NaN: false -> the full test decides
}

// the 4 cells of try t of hypothesis gh, their scene points and pixel positions.  With the planar [E,3,H,W] layout a
// cell is three 4-byte reads from three cache lines; when the maps are too large for the caches (KArgs::sc4, see
// k_pack_cells) the sampler reads one 16-byte (x, y, z, -) record per cell instead.
// (shift_x, shift_y, W, H: the frame's -- a.shift_x, a.shift_y, a.W, a.H wherever the frame's view has been applied)
__device__ __forceinline__ void gather_sample(const KArgs& a, const float* __restrict__ map, int P, const Philox& rng, uint32_t gh,
                                              uint32_t t, int (&cx)[4], int (&cy)[4], V3 (&Pt)[4], float (&Pf)[4][3],
                                              double (&mu)[4], double (&mv)[4], int shift_x, int shift_y, int W, int H) {
    draw_cells(rng, gh, t, W, H, cx, cy);
    const float4* __restrict__ map4 = a.sc4 ? a.sc4 + (size_t)(map - a.sc) / 3 : nullptr;  // (map - sc) / 3 = expert * P
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int idx = cy[j] * W + cx[j];
        if (map4) {
            const float4 v = map4[idx];
            Pf[j][0] = v.x; Pf[j][1] = v.y; Pf[j][2] = v.z;
        } else {
            Pf[j][0] = map[idx];
            Pf[j][1] = map[P + idx];
            Pf[j][2] = map[2 * P + idx];
        }
        Pt[j] = V3{(double)Pf[j][0], (double)Pf[j][1], (double)Pf[j][2]};
        mu[j] = (double)(float)(cx[j] * a.sub + a.sub / 2 - shift_x);  // cell_px / cell_py
        mv[j] = (double)(float)(cy[j] * a.sub + a.sub / 2 - shift_y);
    }
}
__device__ __forceinline__ void gather_sample(const KArgs& a, const float* __restrict__ map, int P, const Philox& rng, uint32_t gh,
                                              uint32_t t, int (&cx)[4], int (&cy)[4], V3 (&Pt)[4], float (&Pf)[4][3],
                                              double (&mu)[4], double (&mv)[4]) {
    gather_sample(a, map, P, rng, gh, t, cx, cy, Pt, Pf, mu, mv, a.shift_x, a.shift_y, a.W, a.H);
}

// float [R | t + R c] for the fp32 scoring stream, c = origin of the expert's map (device_common.hpp:map_centre);
// the shifted translation is formed in double
__device__ __forceinline__ void store_rt32(const KArgs& a, int h, const float* __restrict__ map, const double R[9], const double T[3]) {
    const Centre c = map_centre(a, map);
    const double cx = c.x, cy = c.y, cz = c.z;
    float* rt = a.rt32 + (size_t)h * 12;
#pragma unroll
    for (int k = 0; k < 9; k++) rt[k] = (float)R[k];
    rt[9] = (float)(R[0] * cx + R[1] * cy + R[2] * cz + T[0]);
    rt[10] = (float)(R[3] * cx + R[4] * cy + R[5] * cz + T[1]);
    rt[11] = (float)(R[6] * cx + R[7] * cy + R[8] * cz + T[2]);
}

// RT32 = false: everything but the fp32 rows -- for a call on which no kernel reads them (the front route, front_route_policy.hpp);
// the first stage that does read them forms them from (rvec, tvec): k_hyps_to_rt32
template <bool RT32>
__device__ __forceinline__ void store_hypothesis_rows(const KArgs& a, int h, const float* __restrict__ map, const double rvec[3],
                                                      const double T[3], const double R[9], const int (&cx)[4], const int (&cy)[4],
                                                      int tries_val) {
    double* hp = a.hyps + (size_t)h * 6;
    hp[0] = rvec[0]; hp[1] = rvec[1]; hp[2] = rvec[2];
    hp[3] = T[0]; hp[4] = T[1]; hp[5] = T[2];
    double* hr = a.hyps_R + (size_t)h * 9;
#pragma unroll
    for (int k = 0; k < 9; k++) hr[k] = R[k];
    if (RT32) store_rt32(a, h, map, R, T);
    int* sx = a.sample_xy + (size_t)h * 8;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        sx[2 * j] = cx[j];
        sx[2 * j + 1] = cy[j];
    }
    a.tries[h] = tries_val;
}
__device__ __forceinline__ void store_hypothesis(const KArgs& a, int h, const float* __restrict__ map, const double rvec[3],
                                                 const double T[3], const double R[9], const int (&cx)[4], const int (&cy)[4],
                                                 int tries_val) {
    store_hypothesis_rows<true>(a, h, map, rvec, T, R, cx, cy, tries_val);
}

constexpr int SAMPLE_PENDING = -2;  // tries[h] between the two phases of the throughput-shaped sampling

}  // namespace esac
