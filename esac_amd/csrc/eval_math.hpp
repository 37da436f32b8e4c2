// eval_math.hpp -- what the test loop reports about one frame (test_esac.py:209-247), host + device (ESAC_HD) like pose_math.hpp
// and gt_math.hpp: rotation error in degrees, translation error in cm, the 5 cm / 5 deg flag, "expert chosen == true expert" and
// the quaternion + translation of the INVERTED pose for poses_esac_*.txt.  It restates esac_amd/harness.py -- rodrigues_vector,
// pose_errors_deg_cm, pose_file_line -- branch by branch in fp64, so that a row of esac_hip_eval_batch and the harness's host
// functions differ by libm's last bits only (tests/test_eval_math_host.py holds the two against each other on the CPU).
// rodrigues_mat2vec of pose_math.hpp is NOT that function: it takes the near-pi branch at s < 1e-5 and has a third sign rule.
// Compiled without contraction (-ffp-contract=off).
#pragma once
#include "gt_math.hpp"

namespace esac {

// layout of one output row (doubles); include/esac_hip.h: ESAC_EVAL_*, held equal by a static_assert in esac_capi.hip
enum { ESAC_EVAL_ROT_DEG_K = 0, ESAC_EVAL_TRANS_CM_K = 1, ESAC_EVAL_POSE_OK_K = 2, ESAC_EVAL_CLASS_OK_K = 3, ESAC_EVAL_QUAT_K = 4,
       ESAC_EVAL_INV_T_K = 8, ESAC_EVAL_EXPERT_K = 11, ESAC_EVAL_HYP_K = 12, ESAC_EVAL_STATUS_K = 13, ESAC_EVAL_DOUBLES_K = 16 };
constexpr int ESAC_EVAL_REC_DOUBLES = 32;                                           // ESAC_RES_DOUBLES
constexpr int ESAC_EVAL_REC_HYP = 1, ESAC_EVAL_REC_EXPERT = 2, ESAC_EVAL_REC_POSE = 9, ESAC_EVAL_REC_VALID = 31;  // ESAC_RES_*

constexpr double ESAC_EVAL_PI = 3.141592653589793;  // math.pi

ESAC_HD double eval_norm3(double x, double y, double z) { return sqrt(x * x + y * y + z * z); }  // np.linalg.norm of three

// harness.rodrigues_vector: rotation matrix (row-major R[9]) -> axis-angle vector
ESAC_HD void eval_rodrigues_vector(const double R[9], double r[3]) {
    const double kx = 0.5 * (R[7] - R[5]), ky = 0.5 * (R[2] - R[6]), kz = 0.5 * (R[3] - R[1]);
    const double s = eval_norm3(kx, ky, kz);
    const double c = (R[0] + R[4] + R[8] - 1.0) / 2.0;
    const double angle = atan2(s, c);
    if (s < 1e-12) {
        if (c > 0) {
            r[0] = 0; r[1] = 0; r[2] = 0;
            return;
        }
        // angle ~ pi: axis from the diagonal of (R + I) / 2 (a NaN diagonal stays NaN, as np.clip leaves it)
        const double d0 = (R[0] + 1.0) / 2.0, d1 = (R[4] + 1.0) / 2.0, d2 = (R[8] + 1.0) / 2.0;
        double ax = sqrt(d0 < 0.0 ? 0.0 : d0), ay = sqrt(d1 < 0.0 ? 0.0 : d1), az = sqrt(d2 < 0.0 ? 0.0 : d2);
        if (R[1] < 0) ay = -ay;
        if (R[2] < 0) az = -az;
        const double n = eval_norm3(ax, ay, az);
        const double m = n > 1e-300 ? n : (n != n ? n : 1e-300);  // Python's max(n, 1e-300): a NaN first argument is kept
        r[0] = ax / m * angle; r[1] = ay / m * angle; r[2] = az / m * angle;
        return;
    }
    r[0] = kx / s * angle; r[1] = ky / s * angle; r[2] = kz / s * angle;
}

// harness.pose_errors_deg_cm: (rotation error in degrees, translation error in cm) of two 4x4 row-major poses
ESAC_HD void eval_pose_errors(const double P[16], const double G[16], double* rot_deg, double* trans_cm) {
    const double dx = G[3] - P[3], dy = G[7] - P[7], dz = G[11] - P[11];
    const double t_err = eval_norm3(dx, dy, dz);
    double M[9];  // out_R @ gt_R.T
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) M[3 * i + j] = P[4 * i] * G[4 * j] + P[4 * i + 1] * G[4 * j + 1] + P[4 * i + 2] * G[4 * j + 2];
    double r[3];
    eval_rodrigues_vector(M, r);
    *rot_deg = eval_norm3(r[0], r[1], r[2]) * 180.0 / ESAC_EVAL_PI;
    *trans_cm = t_err * 100.0;
}

// inv4 of gt_math.hpp -- Gauss-Jordan with partial pivoting, the same operations in the same order, bit for bit (the host test
// holds the two against each other) -- for a kernel that keeps one frame per LANE: inv4 swaps rows through a run-time row index,
// which puts its 4x8 tableau into scratch memory (272 bytes a lane); here every index is a compile-time constant, the pivot row
// is exchanged by selects, and the tableau stays in registers.
ESAC_HD bool eval_inv4(const double A[16], double Ai[16]) {
    double M[4][8];
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) {
            M[i][j] = A[4 * i + j];
            M[i][4 + j] = i == j;
        }
    bool ok = true;
#pragma unroll
    for (int col = 0; col < 4; col++) {
        int piv = col;
        double best = fabs(M[col][col]);
#pragma unroll
        for (int r = col + 1; r < 4; r++)
            if (fabs(M[r][col]) > best) {
                piv = r;
                best = fabs(M[r][col]);
            }
#pragma unroll
        for (int r = col + 1; r < 4; r++) {
            const bool sw = piv == r;
#pragma unroll
            for (int j = 0; j < 8; j++) {
                const double a = M[col][j], b = M[r][j];
                M[col][j] = sw ? b : a;
                M[r][j] = sw ? a : b;
            }
        }
        if (M[col][col] == 0) ok = false;  // (inv4 returns here; the lanes of a wavefront go on together and the result is dropped)
        const double d = 1.0 / M[col][col];
#pragma unroll
        for (int j = 0; j < 8; j++) M[col][j] *= d;
#pragma unroll
        for (int r = 0; r < 4; r++) {
            if (r == col) continue;
            const double f = M[r][col];
#pragma unroll
            for (int j = 0; j < 8; j++) M[r][j] = f == 0 ? M[r][j] : M[r][j] - f * M[col][j];
        }
    }
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) Ai[4 * i + j] = M[i][4 + j];
    return ok;
}

// harness.pose_file_line without the formatting: q[4] = qw qx qy qz and t[3] of the INVERTED pose.  false (all seven NaN): the
// pose holds a non-finite value or is singular (np.linalg.inv raises there; a NaN pose prints seven "nan").
ESAC_HD bool eval_pose_file_values(const double P[16], double q[4], double t[3]) {
    const double nan = __builtin_nan("");
    bool finite = true;
#pragma unroll
    for (int k = 0; k < 16; k++) finite = finite && (fabs(P[k]) <= DBL_MAX);
    double inv[16];
    if (!eval_inv4(P, inv) || !finite) {
        q[0] = q[1] = q[2] = q[3] = nan;
        t[0] = t[1] = t[2] = nan;
        return false;
    }
    const double R[9] = {inv[0], inv[1], inv[2], inv[4], inv[5], inv[6], inv[8], inv[9], inv[10]};
    double rot[3];
    eval_rodrigues_vector(R, rot);
    const double angle = eval_norm3(rot[0], rot[1], rot[2]);
    double ax = 1.0, ay = 0.0, az = 0.0;
    if (angle > 0) {
        ax = rot[0] / angle; ay = rot[1] / angle; az = rot[2] / angle;
    }
    const double sh = sin(angle * 0.5);
    q[0] = cos(angle * 0.5);
    q[1] = sh * ax; q[2] = sh * ay; q[3] = sh * az;
    t[0] = inv[3]; t[1] = inv[7]; t[2] = inv[11];
    return true;
}

// One row from two fp64 poses: errors, flags, quaternion, translation (the record-independent part of a frame).
// gt_expert < 0: no ground-truth expert was given (CLASS_OK = -1).
ESAC_HD void eval_pose_row(const double P[16], const double G[16], double expert, double hyp, bool has_gt_expert, long long gt_expert,
                           double rot_thresh_deg, double trans_thresh_cm, double row[ESAC_EVAL_DOUBLES_K]) {
    double r_deg, t_cm;
    eval_pose_errors(P, G, &r_deg, &t_cm);
    double q[4], t[3];
    eval_pose_file_values(P, q, t);
    row[ESAC_EVAL_ROT_DEG_K] = r_deg;
    row[ESAC_EVAL_TRANS_CM_K] = t_cm;
    row[ESAC_EVAL_POSE_OK_K] = (t_cm < trans_thresh_cm && r_deg < rot_thresh_deg) ? 1.0 : 0.0;
    row[ESAC_EVAL_CLASS_OK_K] = has_gt_expert ? ((double)gt_expert == expert ? 1.0 : 0.0) : -1.0;
    row[ESAC_EVAL_QUAT_K] = q[0]; row[ESAC_EVAL_QUAT_K + 1] = q[1]; row[ESAC_EVAL_QUAT_K + 2] = q[2]; row[ESAC_EVAL_QUAT_K + 3] = q[3];
    row[ESAC_EVAL_INV_T_K] = t[0]; row[ESAC_EVAL_INV_T_K + 1] = t[1]; row[ESAC_EVAL_INV_T_K + 2] = t[2];
    row[ESAC_EVAL_EXPERT_K] = expert;
    row[ESAC_EVAL_HYP_K] = hyp;
    row[ESAC_EVAL_STATUS_K] = 0.0;
    row[14] = 0.0;
    row[15] = 0.0;
}

// One frame of esac_hip_eval_batch: rec = the frame's result record (ESAC_RES_DOUBLES doubles, as esac_hip_forward_batch* wrote
// it through d_result_out), gt = its ground-truth pose (16 floats).  The pose is read as FLOATS -- the numbers esac.forward puts
// into outPose.  STATUS: 0 a delivered record, 3 the refinement team timed out (ESAC_RES_VALID = 3), 1 no record.
ESAC_HD void eval_frame(const double* rec, const float* gt, bool has_gt_expert, long long gt_expert, double rot_thresh_deg,
                        double trans_thresh_cm, double row[ESAC_EVAL_DOUBLES_K]) {
    const double valid = rec[ESAC_EVAL_REC_VALID];
    const double expert = rec[ESAC_EVAL_REC_EXPERT], hyp = rec[ESAC_EVAL_REC_HYP];
    if (valid == 1.0) {
        double P[16], G[16];
#pragma unroll
        for (int k = 0; k < 16; k++) {
            P[k] = (double)(float)rec[ESAC_EVAL_REC_POSE + k];
            G[k] = (double)gt[k];
        }
        eval_pose_row(P, G, expert, hyp, has_gt_expert, gt_expert, rot_thresh_deg, trans_thresh_cm, row);
        return;
    }
    const double nan = __builtin_nan("");
#pragma unroll
    for (int k = 0; k < ESAC_EVAL_DOUBLES_K; k++) row[k] = 0.0;
    row[ESAC_EVAL_ROT_DEG_K] = nan;
    row[ESAC_EVAL_TRANS_CM_K] = nan;
#pragma unroll
    for (int k = 0; k < 7; k++) row[ESAC_EVAL_QUAT_K + k] = nan;
    row[ESAC_EVAL_CLASS_OK_K] = has_gt_expert ? 0.0 : -1.0;
    row[ESAC_EVAL_EXPERT_K] = expert;
    row[ESAC_EVAL_HYP_K] = hyp;
    row[ESAC_EVAL_STATUS_K] = valid == 3.0 ? 3.0 : 1.0;
}

}  // namespace esac
