// TEST-ONLY host build of eval_math.hpp (the arithmetic of esac_hip_eval_batch): the table of pose pairs the CPU test walks, one
// row / one frame at a time for tests/test_eval_math_host.py, and a main() that walks the same table as a stand-alone program
// (built once with -fsanitize=address,undefined; nothing loaded into Python is sanitized).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../esac_amd/csrc/eval_math.hpp"

using namespace esac;

namespace {

struct Rng {  // splitmix64: the table is the same in every build
    uint64_t s;
    uint64_t next() {
        uint64_t z = (s += 0x9e3779b97f4a7c15ull);
        z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
        z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
        return z ^ (z >> 31);
    }
    double uni() { return (double)(next() >> 11) * (1.0 / 9007199254740992.0); }  // [0,1)
    double sym(double a) { return (2.0 * uni() - 1.0) * a; }
};

void pose_from(const double r[3], const double t[3], double P[16]) {
    double R[9];
    rodrigues_vec2mat<false>(r, R, nullptr);
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) P[4 * i + j] = R[3 * i + j];
        P[4 * i + 3] = t[i];
    }
    P[12] = 0; P[13] = 0; P[14] = 0; P[15] = 1;
}

// P = [R(angle about axis) * G_R | G_t + dt]
void rotated(const double G[16], const double axis[3], double angle, const double dt[3], double P[16]) {
    const double r[3] = {axis[0] * angle, axis[1] * angle, axis[2] * angle};
    const double zero[3] = {0, 0, 0};
    double D[16];
    pose_from(r, zero, D);
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) P[4 * i + j] = D[4 * i] * G[j] + D[4 * i + 1] * G[4 + j] + D[4 * i + 2] * G[8 + j];
        P[4 * i + 3] = G[4 * i + 3] + dt[i];
    }
    P[12] = 0; P[13] = 0; P[14] = 0; P[15] = 1;
}

void to_float(double P[16]) {
    for (int k = 0; k < 16; k++) P[k] = (double)(float)P[k];
}

}  // namespace

// kinds of a table entry
enum { KIND_IDENTICAL = 0, KIND_SMALL = 1, KIND_NEAR_PI = 2, KIND_RANDOM = 3, KIND_NAN = 4, KIND_NAN_ROT = 5 };

// Fills up to `cap` pose pairs (P = estimate, G = ground truth, 16 doubles each, row-major) and their kinds; returns how many the
// table holds (call with cap = 0 to ask).
extern "C" int eval_probe_table(double* P, double* G, int* kind, int cap) {
    const int total = 4 + 6 + 30 + 1000 + 2;
    if (cap < total) return total;
    Rng rng{20261018ull};
    int n = 0;
    auto put = [&](const double* p, const double* g, int k) {
        memcpy(P + 16 * n, p, 16 * sizeof(double));
        memcpy(G + 16 * n, g, 16 * sizeof(double));
        kind[n++] = k;
    };
    const double zero3[3] = {0, 0, 0};
    double I4[16], Gr[16];  // ground truths: the identity rotation with a translation, and a fixed general pose
    {
        const double t[3] = {0.5, -1.25, 2.0};
        pose_from(zero3, t, I4);
        const double r[3] = {0.7, -1.1, 0.4}, t2[3] = {-1.5, 0.3, 4.0};
        pose_from(r, t2, Gr);
    }
    // identical poses: exactly 0.0 and 0.0
    {
        double E4[16];
        pose_from(zero3, zero3, E4);
        put(E4, E4, KIND_IDENTICAL);
        put(I4, I4, KIND_IDENTICAL);
        put(Gr, Gr, KIND_IDENTICAL);
        double Gf[16];
        memcpy(Gf, Gr, sizeof(Gf));
        to_float(Gf);
        put(Gf, Gf, KIND_IDENTICAL);
    }
    // rotations of 1e-9, 1e-7, 1e-3 rad
    const double small[3] = {1e-9, 1e-7, 1e-3};
    const double ax_s[3] = {0.2672612419124244, -0.5345224838248488, 0.8017837257372732};  // (1,-2,3)/sqrt(14)
    const double dt_s[3] = {0.01, -0.02, 0.005};
    for (int k = 0; k < 3; k++) {
        double Pk[16];
        rotated(I4, ax_s, small[k], dt_s, Pk);
        put(Pk, I4, KIND_SMALL);
        rotated(Gr, ax_s, small[k], dt_s, Pk);
        put(Pk, Gr, KIND_SMALL);
    }
    // pi - 1e-9, pi - 1e-13 and pi about x, y, z, (1,1,0)/sqrt2, (1,-1,1)/sqrt3: the diagonal branch and its two sign rules
    const double s2 = 0.7071067811865476, s3 = 0.5773502691896258;
    const double axes[5][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}, {s2, s2, 0}, {s3, -s3, s3}};
    const double back[3] = {1e-9, 1e-13, 0.0};
    for (int a = 0; a < 5; a++)
        for (int k = 0; k < 3; k++) {
            double Pk[16];
            rotated(I4, axes[a], ESAC_EVAL_PI - back[k], dt_s, Pk);
            put(Pk, I4, KIND_NEAR_PI);
            rotated(Gr, axes[a], ESAC_EVAL_PI - back[k], dt_s, Pk);
            put(Pk, Gr, KIND_NEAR_PI);
        }
    // 1000 random pose pairs, rounded to float32 first (the records carry floats: R is orthonormal only to 1e-7)
    for (int i = 0; i < 1000; i++) {
        double r[3], t[3], Pk[16], Gk[16];
        const double ang = (i % 4 == 0) ? rng.uni() * 0.05 : rng.uni() * ESAC_EVAL_PI;  // a quarter of them near the ground truth
        double a[3] = {rng.sym(1), rng.sym(1), rng.sym(1)};
        const double na = sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]) + 1e-30;
        for (int k = 0; k < 3; k++) {
            r[k] = rng.sym(2.0);
            t[k] = rng.sym(5.0);
            a[k] /= na;
        }
        pose_from(r, t, Gk);
        const double dt[3] = {rng.sym(0.1), rng.sym(0.1), rng.sym(0.1)};
        rotated(Gk, a, ang, dt, Pk);
        to_float(Pk);
        to_float(Gk);
        put(Pk, Gk, KIND_RANDOM);
    }
    // a NaN pose; a pose with one NaN in its rotation
    {
        double Pn[16];
        for (int k = 0; k < 16; k++) Pn[k] = __builtin_nan("");
        put(Pn, Gr, KIND_NAN);
        memcpy(Pn, Gr, sizeof(Pn));
        Pn[5] = __builtin_nan("");
        put(Pn, Gr, KIND_NAN_ROT);
    }
    return n;
}

extern "C" void eval_probe_row(const double* P, const double* G, double expert, double hyp, int has_gt_expert, long long gt_expert,
                               double rot_thresh_deg, double trans_thresh_cm, double* row) {
    eval_pose_row(P, G, expert, hyp, has_gt_expert != 0, gt_expert, rot_thresh_deg, trans_thresh_cm, row);
}

extern "C" void eval_probe_frame(const double* rec, const float* gt, int has_gt_expert, long long gt_expert, double rot_thresh_deg,
                                 double trans_thresh_cm, double* row) {
    eval_frame(rec, gt, has_gt_expert != 0, gt_expert, rot_thresh_deg, trans_thresh_cm, row);
}

// the register-only inverse against gt_math.hpp's: both results and both verdicts
extern "C" void eval_probe_inv4(const double* A, double* by_eval, double* by_gt, int* ok) {
    ok[0] = eval_inv4(A, by_eval) ? 1 : 0;
    ok[1] = inv4(A, by_gt) ? 1 : 0;
}

#ifdef EVAL_PROBE_MAIN
// The stand-alone walk: every entry of the table through eval_pose_row and through eval_frame (a record made from it), with the
// properties that need no second implementation; a sanitizer build reports what it finds by itself.
int main() {
    const int total = eval_probe_table(nullptr, nullptr, nullptr, 0);
    static double P[16 * 2048], G[16 * 2048];
    static int kind[2048];
    if (total > 2048 || eval_probe_table(P, G, kind, 2048) != total) {
        printf("eval_probe: table size\n");
        return 2;
    }
    int bad = 0;
    for (int i = 0; i < total; i++) {
        double row[16], inv_a[16], inv_b[16];
        int ok[2];
        eval_probe_row(P + 16 * i, G + 16 * i, 1.0, 7.0, 1, i % 2, 5.0, 5.0, row);
        const bool nan_kind = kind[i] == KIND_NAN || kind[i] == KIND_NAN_ROT;
        if (kind[i] == KIND_IDENTICAL && !(row[0] == 0.0 && row[1] == 0.0 && row[2] == 1.0)) bad++;
        if (nan_kind && !(row[0] != row[0] && row[2] == 0.0 && row[4] != row[4])) bad++;
        if (!nan_kind) {
            const double qn = sqrt(row[4] * row[4] + row[5] * row[5] + row[6] * row[6] + row[7] * row[7]);
            if (!(fabs(qn - 1.0) < 1e-12) || !(row[0] >= 0.0 && row[0] <= 180.0 + 1e-9) || !(row[1] >= 0.0)) bad++;
            eval_probe_inv4(P + 16 * i, inv_a, inv_b, ok);
            if (ok[0] != 1 || ok[1] != 1 || memcmp(inv_a, inv_b, sizeof(inv_a)) != 0) bad++;
        }
        if (row[3] != ((i % 2) == 1 ? 1.0 : 0.0) || row[11] != 1.0 || row[12] != 7.0 || row[13] != 0.0 || row[14] != 0.0 || row[15] != 0.0) bad++;
        // the same pair as a frame: record + float ground truth, delivered / timed out / absent
        double rec[32] = {0};
        float gt[16];
        for (int k = 0; k < 16; k++) {
            rec[9 + k] = P[16 * i + k];
            gt[k] = (float)G[16 * i + k];
        }
        rec[1] = 7.0; rec[2] = 1.0;
        const double valid[3] = {1.0, 3.0, 0.0}, status[3] = {0.0, 3.0, 1.0};
        for (int v = 0; v < 3; v++) {
            double fr[16];
            rec[31] = valid[v];
            eval_probe_frame(rec, gt, v != 1, 1, 5.0, 5.0, fr);
            if (fr[13] != status[v] || fr[11] != 1.0 || fr[12] != 7.0) bad++;
            if (v > 0 && !(fr[0] != fr[0] && fr[1] != fr[1] && fr[2] == 0.0 && fr[4] != fr[4] && fr[10] != fr[10])) bad++;
            if (fr[3] != (v == 0 ? 1.0 : v == 1 ? -1.0 : 0.0)) bad++;
        }
    }
    printf("eval_probe: %d entries, %d bad\n", total, bad);
    return bad ? 1 : 0;
}
#endif
