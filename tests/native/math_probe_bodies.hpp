// math_probe_bodies.hpp -- TEST-ONLY: one item of work per call, written once for both probes.  host_math_probe.cpp loops
// over the items on the CPU (the #else side of every __HIP_DEVICE_COMPILE__ branch of the product's headers),
// device_math_probe.hip runs one thread per item on the GPU (the device side: v_rcp_f64 / v_rsq_f64 + Newton, the
// interleaved reciprocals and asm weights of lm_point_terms, the device library's sincos / frexp).  The layouts below are
// what tests/device_math_cases.py packs and unpacks.
#pragma once
#include "../../esac_amd/csrc/pose_math.hpp"
#include "../../esac_amd/csrc/lm_math.hpp"
#include "../../esac_amd/csrc/bwd_math.hpp"
#include "../../esac_amd/csrc/lm_lanes.hpp"
#include "../../esac_amd/csrc/p3p_screen.hpp"

namespace esac_probe {
using namespace esac;

// ---- scalars: op 0 fast_rcp, 1 scr_sqrt, 2 cbrt_pos, 3 cos_third_acos, 4 lane_rcp_neg (the one-double-per-lane overload)
ESAC_HD double body_scalar(int op, double v) {
    switch (op) {
        case 0: return fast_rcp(v);
        case 1: return scr_sqrt(v);
        case 2: return cbrt_pos(v);
        case 3: return cos_third_acos(v);
        default: return lane_rcp_neg(v);
    }
}

// ---- rotation: pose[6] in; out[ROT_OUT]:
//   [0,9) R, 9 A, 10 B, 11 identity, 12 x          lm_pose_rotation
//   [13,22) Mw                                      lm_pose_left_jacobian of that LmTrig
//   [22,31) R, [31,40) Mw, [40,49) K                lm_pose_chain
//   [49,58) R, [58,85) dR/dr                        rodrigues_vec2mat<true>
//   [85,88) rvec                                    rodrigues_mat2vec of [49,58)
constexpr int ROT_OUT = 88;
ESAC_HD void body_rotation(const double* pose, double* out) {
    LmTrig tg;
    lm_pose_rotation(pose, out, tg);
    out[9] = tg.A; out[10] = tg.B; out[11] = tg.identity ? 1.0 : 0.0; out[12] = tg.x;
    double Mw[3][3];
    lm_pose_left_jacobian(tg, Mw);
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) out[13 + 3 * i + j] = Mw[i][j];
    LmChain ch;
    lm_pose_chain(pose, out + 22, ch);
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) { out[31 + 3 * i + j] = ch.Mw[i][j]; out[40 + 3 * i + j] = ch.K[i][j]; }
    rodrigues_vec2mat<true>(pose, out + 49, out + 58);
    rodrigues_mat2vec(out + 49, out + 85);
}

// ---- point terms: PT_N correspondences a case, taken NP at a time (PT_N is a multiple of 1, 2, 3, 4).
// in[PT_IN]: pose[6], f, cx, cy, then PT_N x (X, Y, Z, mx, my, on);  out[PT_OUT]: PT_N x (x, y, iz, ex, ey, w) as
// lm_point_terms leaves them, then U21[21], g6[6], e2 through lm_accumulate_moments -> lm_moments_to_acc -> lm_transform.
constexpr int PT_N = 12, PT_IN = 9 + 6 * PT_N, PT_OUT = 6 * PT_N + 28;
template <int NP>
ESAC_HD void body_point_terms(const double* in, double* out) {
    const double f = in[6];
    Cam cam{f, f, in[7], in[8]};
    double R[9], mom[LM_NMOM], acc[LM_NACC];
    LmChain ch;
    lm_pose_chain(in, R, ch);
    for (int k = 0; k < LM_NMOM; k++) mom[k] = 0;
    for (int i = 0; i < PT_N; i += NP) {
        double X[NP], Y[NP], Z[NP], mx[NP], my[NP];
        bool on[NP];
        for (int p = 0; p < NP; p++) {
            const double* q = in + 9 + 6 * (i + p);
            X[p] = q[0]; Y[p] = q[1]; Z[p] = q[2]; mx[p] = q[3]; my[p] = q[4]; on[p] = q[5] != 0.0;
        }
        LmTerms<NP> t;
        lm_point_terms<NP>(R, in + 3, cam, X, Y, Z, mx, my, on, t);
        for (int p = 0; p < NP; p++) {
            double* o = out + 6 * (i + p);
            o[0] = t.x[p]; o[1] = t.y[p]; o[2] = t.iz[p]; o[3] = t.ex[p]; o[4] = t.ey[p]; o[5] = t.w[p];
        }
        lm_accumulate_moments<NP>(t, mom);
    }
    lm_moments_to_acc(mom, f, acc);
    lm_transform(acc, ch, out + 6 * PT_N, out + 6 * PT_N + 21);
    out[6 * PT_N + 27] = acc[26];
}

// ---- solves: in[SOLVE_IN]: U21[21], g6[6], lambda;  out[SOLVE_OUT]: dx[6], verdict (lm_solve6) | Ainv[36], verdict
// (inv_spd6) | Ainv[36] (pinv_sym6_jacobi)
constexpr int SOLVE_IN = 28, SOLVE_OUT = 80;
ESAC_HD void body_solves(const double* in, double* out) {
    out[6] = lm_solve6(in, in + 21, in[27], out) ? 1.0 : 0.0;
    out[43] = inv_spd6(in, out + 7) ? 1.0 : 0.0;
    pinv_sym6_jacobi(in, out + 44);
}

// ---- device-only steps (device_math_probe.hip): the lane-dealt LM step of one wavefront and the pseudo-inverse step of one
// workgroup.  LANE_IN: totals[27], pose[6], lambda, lambda of the second (rejected-trial) solve;
// LANE_OUT per lane: U21[21], g6[6] after the first solve | dx[6] | dx of the second solve (behind a branch) [6] | dx of a third,
// straight-line solve at the second lambda [6] | the three verdicts | U21[21], g6[6] after the second solve
constexpr int LANE_IN = 35, LANE_OUT = 75;

}  // namespace esac_probe
