// gt_math.hpp -- the loss's view of a ground-truth camera pose (esac_util.h:555-568), host + device (ESAC_HD) like pose_math.hpp:
// the blocking training entry points run it on the host, esac_hip_backward_batch_dev in k_bwd_gt_prepare on the device.  One text
// for both, compiled without contraction (-ffp-contract=off): the two routes hand the kernels the same 22 doubles.
#pragma once
#include "pose_math.hpp"

namespace esac {

constexpr int ESAC_GT_DOUBLES = 22;  // one frame's record: gt[16] | gt_pose[6] (BwdArgs::gt_frames)

// general 4x4 inverse, Gauss-Jordan with partial pivoting (cv::Mat::inv() of trans2pose, esac_util.h:557)
ESAC_HD bool inv4(const double A[16], double Ai[16]) {
    double M[4][8];
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++) {
            M[i][j] = A[4 * i + j];
            M[i][4 + j] = i == j;
        }
    for (int col = 0; col < 4; col++) {
        int piv = col;
        for (int r = col + 1; r < 4; r++)
            if (fabs(M[r][col]) > fabs(M[piv][col])) piv = r;
        if (M[piv][col] == 0) return false;
        if (piv != col)
            for (int j = 0; j < 8; j++) {
                const double t = M[piv][j];
                M[piv][j] = M[col][j];
                M[col][j] = t;
            }
        const double d = 1.0 / M[col][col];
        for (int j = 0; j < 8; j++) M[col][j] *= d;
        for (int r = 0; r < 4; r++) {
            if (r == col) continue;
            const double f = M[r][col];
            if (f == 0) continue;
            for (int j = 0; j < 8; j++) M[r][j] -= f * M[col][j];
        }
    }
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++) Ai[4 * i + j] = M[i][4 + j];
    return true;
}

// nearest rotation of a 3x3 (orthogonal polar factor = U*Vt of its SVD, what cv::Rodrigues applies to a matrix
// input): Newton iteration X <- (X + X^-T) / 2, quadratic from the ~1e-7 non-orthonormality of a float pose
ESAC_HD void nearest_rotation(double R[9]) {
    for (int it = 0; it < 20; it++) {
        const double* a = R;
        const double c00 = a[4] * a[8] - a[5] * a[7], c01 = a[5] * a[6] - a[3] * a[8], c02 = a[3] * a[7] - a[4] * a[6];
        const double c10 = a[2] * a[7] - a[1] * a[8], c11 = a[0] * a[8] - a[2] * a[6], c12 = a[1] * a[6] - a[0] * a[7];
        const double c20 = a[1] * a[5] - a[2] * a[4], c21 = a[2] * a[3] - a[0] * a[5], c22 = a[0] * a[4] - a[1] * a[3];
        const double det = a[0] * c00 + a[1] * c01 + a[2] * c02;
        if (det == 0) return;
        const double invT[9] = {c00 / det, c01 / det, c02 / det, c10 / det, c11 / det, c12 / det, c20 / det, c21 / det, c22 / det};
        double delta = 0;
        for (int k = 0; k < 9; k++) {
            const double n = 0.5 * (R[k] + invT[k]);
            delta += fabs(n - R[k]);
            R[k] = n;
        }
        if (delta < 1e-15) break;
    }
}

// gt (double of the float input) and trans2pose(gt) (esac_util.h:555-568).  false: singular.
ESAC_HD bool gt_from_pose(const float* gt_pose_f, double gt[16], double gt_pose[6]) {
    double Ti[16];
    for (int i = 0; i < 16; i++) gt[i] = (double)gt_pose_f[i];
    if (!inv4(gt, Ti)) return false;
    double Rg[9] = {Ti[0], Ti[1], Ti[2], Ti[4], Ti[5], Ti[6], Ti[8], Ti[9], Ti[10]};
    nearest_rotation(Rg);
    rodrigues_mat2vec(Rg, gt_pose);
    gt_pose[3] = Ti[3]; gt_pose[4] = Ti[7]; gt_pose[5] = Ti[11];
    return true;
}

}  // namespace esac
