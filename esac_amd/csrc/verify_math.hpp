// verify_math.hpp -- what one GIVEN pose is worth on one expert's map (esac_hip_verify_batch), host + device (ESAC_HD) like
// eval_math.hpp: the reference-arithmetic soft-inlier score, the inlier set of the refinement's own rule, and over that set the
// Gauss-Newton normal matrix of the reprojection residuals, their sum of squares and the pose covariance sigma^2 A^-1.
// Every piece is one the kernels already run: exact_cell_term / exact_score_scaled (select_math.hpp), project_exact_err and
// pnp_point_terms (pose_math.hpp), inv_spd6 / pinv_sym6_* (bwd_math.hpp), the steps of gt_from_pose (gt_math.hpp).  The kernel
// (esac_verify.hip) and the host probe (tests/native/verify_probe.cpp) differ in the ORDER the cells are summed in and in libm's
// last bits, nothing else.  Compiled without contraction (-ffp-contract=off).
#pragma once
#include "bwd_math.hpp"
#include "eval_math.hpp"
#include "select_math.hpp"

namespace esac {

// layout of one output row (doubles); include/esac_hip.h: ESAC_VERIFY_*, held equal by a static_assert in esac_capi.hip
enum { ESAC_VERIFY_SCORE_K = 0, ESAC_VERIFY_N_K = 1, ESAC_VERIFY_SSE_K = 2, ESAC_VERIFY_SIGMA2_K = 3, ESAC_VERIFY_STATUS_K = 4,
       ESAC_VERIFY_A_K = 6, ESAC_VERIFY_C_K = 28, ESAC_VERIFY_DOUBLES_K = 64 };
enum { ESAC_VERIFY_OK_K = 0, ESAC_VERIFY_FEW_K = 1, ESAC_VERIFY_PINV_K = 2, ESAC_VERIFY_BAD_POSE_K = 3, ESAC_VERIFY_BAD_EXPERT_K = 4 };
enum { ESAC_VERIFY_POSE_RT_K = 0, ESAC_VERIFY_POSE_4X4_K = 1 };

// what a lane accumulates: the 21 upper-triangle sums of A (row-major), then SSE, the sum of the score terms, the inlier count
constexpr int VERIFY_ACC = 24, VERIFY_ACC_SSE = 21, VERIFY_ACC_SCORE = 22, VERIFY_ACC_N = 23;

ESAC_HD bool verify_finite(double x) { return fabs(x) <= DBL_MAX; }  // false for NaN and +-inf

// Pose k of the caller's array as rvec | tvec (scene -> camera).  format 0: six doubles, taken as they are; format 1: the float
// 4x4 CAMERA pose (what outPose and gtPoses carry), inverted and reduced as gt_math.hpp's gt_from_pose does it -- general inverse,
// nearest rotation, Rodrigues -- with the inverse in its register-only form (eval_math.hpp: eval_inv4, bit for bit inv4; inv4's
// run-time row index would put a tableau of 256 bytes per lane into scratch).  The host probe holds the result against
// gt_from_pose bit for bit.  false: a non-finite pose, or a 4x4 that the inverse calls singular (ESAC_VERIFY status 3).
ESAC_HD bool verify_fetch_pose(const void* poses, int format, size_t k, double pose[6]) {
    bool ok = true;
    if (format == ESAC_VERIFY_POSE_RT_K) {
        const double* p = static_cast<const double*>(poses) + k * 6;
#pragma unroll
        for (int i = 0; i < 6; i++) pose[i] = p[i];
    } else {
        const float* T = static_cast<const float*>(poses) + k * 16;
        double gt[16], Ti[16];
#pragma unroll
        for (int i = 0; i < 16; i++) {
            gt[i] = (double)T[i];
            ok &= verify_finite(gt[i]);
        }
        ok &= eval_inv4(gt, Ti);
        double Rg[9] = {Ti[0], Ti[1], Ti[2], Ti[4], Ti[5], Ti[6], Ti[8], Ti[9], Ti[10]};
        nearest_rotation(Rg);
        rodrigues_mat2vec(Rg, pose);
        pose[3] = Ti[3]; pose[4] = Ti[7]; pose[5] = Ti[11];
    }
#pragma unroll
    for (int i = 0; i < 6; i++) ok &= verify_finite(pose[i]);
    return ok;
}

// U cells of one map under one pose, added to the lane's sums in the order u = 0 .. U-1.  The U chains are independent and free of
// branches (a cell outside the grid or outside the inlier set adds selected zeros), so that they overlap in an in-order pipeline.
//   score term  exact_cell_term<STRICT>: the clamp of the exact score (a NaN error: an outlier at maxReproj, or NaN under STRICT)
//   inlier      (maxReproj < err ? maxReproj : err) < tau, the refinement's rule: a NaN error stays NaN and is never an inlier
//   residuals   pnp_point_terms: (ex, ey) = projection - pixel in double and the two Jacobian rows d / d(rvec, tvec)
template <bool STRICT, int U>
ESAC_HD void verify_accumulate(const double (&R)[9], const double (&dRdr)[27], const double (&t)[3], const Cam& cam, const float (&X)[U],
                               const float (&Y)[U], const float (&Z)[U], const float (&px)[U], const float (&py)[U], const bool (&live)[U],
                               float tau, float beta, float max_reproj, double (&acc)[VERIFY_ACC]) {
#pragma unroll
    for (int u = 0; u < U; u++) {
        const double term = exact_cell_term<STRICT>(R, t, cam, X[u], Y[u], Z[u], px[u], py[u], max_reproj, tau, beta);
        float err = project_exact_err(R, t, cam, X[u], Y[u], Z[u], px[u], py[u]);
        err = max_reproj < err ? max_reproj : err;
        const bool in = live[u] && err < tau;
        double ex, ey, Ju[6], Jv[6];
        pnp_point_terms(R, dRdr, t, cam, (double)X[u], (double)Y[u], (double)Z[u], (double)px[u], (double)py[u], ex, ey, Ju, Jv);
        int k = 0;
#pragma unroll
        for (int p = 0; p < 6; p++)
#pragma unroll
            for (int q = p; q < 6; q++) {
                const double v = Ju[p] * Ju[q] + Jv[p] * Jv[q];
                acc[k++] += in ? v : 0.0;
            }
        const double e2 = ex * ex + ey * ey;
        acc[VERIFY_ACC_SSE] += in ? e2 : 0.0;
        acc[VERIFY_ACC_SCORE] += live[u] ? term : 0.0;
        acc[VERIFY_ACC_N] += in ? 1.0 : 0.0;
    }
}

// a row whose every figure is NaN (status 3 and 4)
ESAC_HD void verify_row_nan(int status, double* row) {
    const double nan = __builtin_nan("");
#pragma unroll
    for (int i = 0; i < ESAC_VERIFY_DOUBLES_K; i++) row[i] = nan;
    row[ESAC_VERIFY_STATUS_K] = (double)status;
    row[5] = 0;
    row[27] = 0;
}

// The pseudo-inverse of the host: pinv_sym6_jacobi in registers.  (The kernel hands verify_finish the rolled form over LDS,
// operation by operation the same: bwd_math.hpp.)
struct VerifyPinvRegisters {
    ESAC_HD void operator()(const double (&U21)[21], double (&Ainv)[36]) const { pinv_sym6_jacobi(U21, Ainv); }
};

// The totals of a pose -> its row.  sigma^2 = SSE / (2n - 6), C = sigma^2 A^-1 through inv_spd6, or `pinv` where that refuses.
template <class Pinv>
ESAC_HD void verify_finish(const double (&acc)[VERIFY_ACC], float alpha, int W, int H, const Pinv& pinv, double* row) {
    const double nan = __builtin_nan("");
    const double n = acc[VERIFY_ACC_N], sse = acc[VERIFY_ACC_SSE];
    row[ESAC_VERIFY_SCORE_K] = exact_score_scaled(acc[VERIFY_ACC_SCORE], alpha, W, H);
    row[ESAC_VERIFY_N_K] = n;
    row[ESAC_VERIFY_SSE_K] = sse;
    row[5] = 0;
    row[27] = 0;
    double U21[21];
#pragma unroll
    for (int k = 0; k < 21; k++) row[ESAC_VERIFY_A_K + k] = U21[k] = acc[k];
    if (n < 4.0) {
        row[ESAC_VERIFY_SIGMA2_K] = nan;
        row[ESAC_VERIFY_STATUS_K] = (double)ESAC_VERIFY_FEW_K;
#pragma unroll
        for (int i = 0; i < 36; i++) row[ESAC_VERIFY_C_K + i] = nan;
        return;
    }
    const double sigma2 = sse / (2.0 * n - 6.0);
    double Ainv[36];
    int status = ESAC_VERIFY_OK_K;
    if (!inv_spd6(U21, Ainv)) {
        pinv(U21, Ainv);
        status = ESAC_VERIFY_PINV_K;
    }
    row[ESAC_VERIFY_SIGMA2_K] = sigma2;
    row[ESAC_VERIFY_STATUS_K] = (double)status;
    // both triangles from the upper one: the row is symmetric bit for bit
#pragma unroll
    for (int i = 0; i < 6; i++)
#pragma unroll
        for (int j = i; j < 6; j++) {
            const double c = sigma2 * Ainv[i * 6 + j];
            row[ESAC_VERIFY_C_K + i * 6 + j] = c;
            row[ESAC_VERIFY_C_K + j * 6 + i] = c;
        }
}

// One pose against one map, cells in index order: the host's form of the kernel (tests/native/verify_probe.cpp).  map: the
// expert's [3,H,W] planes; the pixel of cell (row, col) is createSampling's (esac_util.h:64-66).
template <bool STRICT>
ESAC_HD void verify_pose_host(const float* map, int H, int W, int sub, int shift_x, int shift_y, const Cam& cam, const double pose[6],
                              float tau, float alpha, float beta, float max_reproj, double* row) {
    const double rv[3] = {pose[0], pose[1], pose[2]}, t[3] = {pose[3], pose[4], pose[5]};
    double R[9], dRdr[27], acc[VERIFY_ACC];
    rodrigues_vec2mat<true>(rv, R, dRdr);
    for (int k = 0; k < VERIFY_ACC; k++) acc[k] = 0;
    const int P = H * W;
    for (int i = 0; i < P; i++) {
        const int r = i / W, c = i - r * W;
        const float X[1] = {map[i]}, Y[1] = {map[P + i]}, Z[1] = {map[2 * P + i]};
        const float px[1] = {(float)(c * sub + sub / 2 - shift_x)}, py[1] = {(float)(r * sub + sub / 2 - shift_y)};
        const bool live[1] = {true};
        verify_accumulate<STRICT, 1>(R, dRdr, t, cam, X, Y, Z, px, py, live, tau, beta, max_reproj, acc);
    }
    verify_finish(acc, alpha, W, H, VerifyPinvRegisters{}, row);
}

}  // namespace esac
