// strict_probe.cpp -- TEST-ONLY: the Horn variant of the device P3P (pose_math.hpp: align_horn, p3p_4pt<AlignHorn>) compiled
// for the host, so that the CPU suite can compare the strict-reference route's own source with the oracle bit by bit.
// Built by tests/native/build_strict.py with the flags of host_math_probe.cpp.  Not part of the product library.
#include "../../esac_amd/csrc/pose_math.hpp"
using namespace esac;
extern "C" {
int probe_p3p_strict(const double* obj, const double* img, double fx, double fy, double cx, double cy, double* rvec, double* tvec, double* Rout) {
    V3 P[4]; double mu[4], mv[4];
    for (int j = 0; j < 4; j++) { P[j] = V3{obj[3*j], obj[3*j+1], obj[3*j+2]}; mu[j] = img[2*j]; mv[j] = img[2*j+1]; }
    Cam cam{fx, fy, cx, cy};
    double R[9], T[3];
    if (!p3p_4pt<AlignHorn>(P, mu, mv, cam, R, T)) return 0;
    rodrigues_mat2vec(R, rvec);
    for (int i = 0; i < 3; i++) tvec[i] = T[i];
    if (Rout) for (int i = 0; i < 9; i++) Rout[i] = R[i];
    return 1;
}
// R * P_k + T = Q_k: P, Q three points each (row-major 3x3)
void probe_align_horn(const double* P, const double* Q, double* R, double* T) {
    align_horn(V3{P[0], P[1], P[2]}, V3{P[3], P[4], P[5]}, V3{P[6], P[7], P[8]}, V3{Q[0], Q[1], Q[2]}, V3{Q[3], Q[4], Q[5]},
               V3{Q[6], Q[7], Q[8]}, R, T);
}
}
