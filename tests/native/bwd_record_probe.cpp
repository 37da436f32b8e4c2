// TEST-ONLY host build of bwd_record_math.hpp (the arithmetic of k_bwd_pose_record): one frame's record from the stages of a training
// call for tests/test_bwd_record_math_host.py -- the argmax through best_take of select_math.hpp, walked serially in hypothesis
// order (what the kernel's strided walk + block_best reduce to), then bwd_record_frame -- and a main() that walks slot lists of its
// own as a stand-alone program (the form a sanitizer build runs; nothing loaded into Python is sanitized).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <string.h>

#include "../../esac_amd/csrc/bwd_record_math.hpp"
#include "../../esac_amd/csrc/select_math.hpp"

using namespace esac;

// draw's argmax over scores[0, N): highest score, first index on ties, a NaN never wins; hypothesis 0 when nothing can win
extern "C" int bwd_record_probe_winner(const double* scores, int N) {
    double bs = -INFINITY;
    int bi = BEST_NONE, bg = BEST_NONE;
    for (int h = 0; h < N; h++) best_take(bs, bi, bg, scores[h], h, h);
    return bi == BEST_NONE ? 0 : bi;
}

extern "C" int bwd_record_probe_find(const int* sel, int n, int win) { return bwd_record_find_slot(sel, n, win); }

// One frame: scores / probs [N], entropy, experts [N] (already with expert_base), the ordered slot list sel[0, n), ref_hyps [N,6],
// map_info [n,4] -> rec[32].  Returns the winner.
extern "C" int bwd_record_probe_frame(const double* scores, const double* probs, double entropy, const int* experts, int N, const int* sel,
                                      int n, int slots_ok, const double* ref_hyps, const int* map_info, double* rec) {
    const int win = bwd_record_probe_winner(scores, N);
    const BwdRecordHead head{scores[win], win, experts[win], probs[win], entropy, N};
    bwd_record_frame(head, win, sel, n, slots_ok != 0, ref_hyps, map_info, rec);
    return win;
}

#ifdef BWD_RECORD_PROBE_MAIN
static bool is_nan(double v) { return v != v; }

int main() {
    int bad = 0, cases = 0;
    // slot lists of every length up to 40 (ascending, with gaps), every member and every non-member looked for
    for (int n = 0; n <= 40; n++) {
        int sel[40];
        for (int k = 0; k < n; k++) sel[k] = 3 * k + (k % 2);
        for (int win = -1; win <= 3 * n + 2; win++) {
            int want = -1;
            for (int k = 0; k < n; k++)
                if (sel[k] == win) want = k;
            if (bwd_record_probe_find(sel, n, win) != want) bad++;
            cases++;
        }
    }
    // records: a winner with a slot (first, last, only), without one (absent, empty list, slot tables not to be trusted)
    const int N = 7;
    double scores[N] = {0.5, 2.0, __builtin_nan(""), 2.0, -1.0, 1.5, 0.0}, probs[N], ref[N * 6];
    int experts[N];
    for (int h = 0; h < N; h++) {
        probs[h] = 0.1 * (h + 1);
        experts[h] = 10 + h;
        for (int k = 0; k < 6; k++) ref[6 * h + k] = 0.1 * (h + 1) * (k + 1) * (k % 2 ? -1.0 : 1.0);
    }
    if (bwd_record_probe_winner(scores, N) != 1) bad++;  // the tie goes to the first index, the NaN never wins
    const double all_nan[2] = {__builtin_nan(""), __builtin_nan("")};
    if (bwd_record_probe_winner(all_nan, 2) != 0) bad++;
    const int lists[6][3] = {{1, 4, 6}, {0, 1, -1}, {1, -1, -1}, {0, 3, 5}, {-1, -1, -1}, {1, 4, 6}};
    const int lens[6] = {3, 2, 1, 3, 0, 3};
    const int ok[6] = {1, 1, 1, 1, 1, 0};
    const int want_slot[6] = {0, 1, 0, -1, -1, -1};
    for (int c = 0; c < 6; c++) {
        int info[12];
        for (int k = 0; k < 12; k++) info[k] = 100 * c + k;
        double rec[32];
        for (int k = 0; k < 32; k++) rec[k] = -7.0;
        const int win = bwd_record_probe_frame(scores, probs, 1.25, experts, N, lists[c], lens[c], ok[c], ref, info, rec);
        cases++;
        if (win != 1 || rec[BWD_REC_SCORE] != 2.0 || rec[BWD_REC_HYP] != 1.0 || rec[BWD_REC_EXPERT] != 11.0 || rec[BWD_REC_PROB] != probs[1] ||
            rec[BWD_REC_ENTROPY] != 1.25 || rec[BWD_REC_CONTENDERS] != (double)N)
            bad++;
        for (int k = 0; k < 32; k++)
            if (rec[k] == -7.0) bad++;  // every double is written
        if (want_slot[c] >= 0) {
            const int* mi = info + 4 * want_slot[c];
            if (rec[BWD_REC_VALID] != 1.0 || rec[BWD_REC_REF_STEPS] != mi[2] || rec[BWD_REC_INLIERS] != mi[1] || rec[BWD_REC_LM_ITERS] != mi[3]) bad++;
            if (memcmp(rec + BWD_REC_RVEC, ref + 6, 6 * sizeof(double)) != 0) bad++;
            // the 4x4 is a rigid transform rounded to float: last row 0 0 0 1, rotation orthonormal to float rounding
            const double* T = rec + BWD_REC_POSE;
            if (T[12] != 0 || T[13] != 0 || T[14] != 0 || T[15] != 1) bad++;
            for (int i = 0; i < 3; i++)
                for (int j = 0; j < 3; j++) {
                    double d = 0;
                    for (int k = 0; k < 3; k++) d += T[4 * i + k] * T[4 * j + k];
                    if (!(fabs(d - (i == j)) < 1e-6)) bad++;
                }
            for (int k = 0; k < 16; k++)
                if (T[k] != (double)(float)T[k]) bad++;
        } else {
            if (rec[BWD_REC_VALID] != 0.0 || rec[BWD_REC_REF_STEPS] != 0.0 || rec[BWD_REC_INLIERS] != 0.0 || rec[BWD_REC_LM_ITERS] != 0.0) bad++;
            for (int k = 0; k < 22; k++)
                if (!is_nan(rec[BWD_REC_RVEC + k])) bad++;
        }
    }
    printf("bwd_record_probe: %d cases, %d bad\n", cases, bad);
    return bad ? 1 : 0;
}
#endif
