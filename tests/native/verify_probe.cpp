// TEST-ONLY host build of verify_math.hpp (the arithmetic of esac_hip_verify_batch): a stand-alone program that evaluates poses
// against maps it reads from stdin and prints the rows, for tests/test_verify_host.py and tests/test_gpu_verify.py (built once more
// with -fsanitize=address,undefined; nothing loaded into Python is sanitized).  Every number travels as a C99 hex float, so the
// program sees the test's bits and the test the program's.
// One request per block of input lines, one answer line per pose:
//   map H W sub shift_x shift_y focal ppx ppy tau alpha beta max_reproj strict format K
//   <3*H*W floats: the expert's planes>          (one line)
//   <K*6 doubles (format 0) or K*16 floats (1)>  (one line)
//     -> K lines "row <status of the fetch: 1 ok, 0 status 3> <64 doubles>"
//   fetch  <16 floats>  ->  "fetch <ok> <6 doubles of verify_fetch_pose> <ok> <6 doubles of gt_from_pose>"
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../esac_amd/csrc/verify_math.hpp"

using namespace esac;

static bool read_token(char* tok, size_t cap) {
    int c;
    do c = getchar(); while (c == ' ' || c == '\n' || c == '\t' || c == '\r');
    if (c == EOF) return false;
    size_t n = 0;
    while (c != EOF && c != ' ' && c != '\n' && c != '\t' && c != '\r') {
        if (n + 1 < cap) tok[n++] = (char)c;
        c = getchar();
    }
    tok[n] = 0;
    return true;
}
static bool read_double(double* v) {
    char tok[64];
    if (!read_token(tok, sizeof(tok))) return false;
    *v = strtod(tok, nullptr);
    return true;
}
static bool read_int(int* v) {
    double d;
    if (!read_double(&d)) return false;
    *v = (int)d;
    return true;
}
static void print_doubles(const double* v, int n) {
    for (int i = 0; i < n; i++) {
        if (v[i] != v[i]) printf(" nan");
        else printf(" %a", v[i]);
    }
}

int main() {
    char kind[64];
    while (read_token(kind, sizeof(kind))) {
        if (!strcmp(kind, "map")) {
            int H, W, sub, sx, sy, strict, format, K;
            double focal, ppx, ppy, tau, alpha, beta, max_reproj;
            if (!read_int(&H) || !read_int(&W) || !read_int(&sub) || !read_int(&sx) || !read_int(&sy) || !read_double(&focal) || !read_double(&ppx) ||
                !read_double(&ppy) || !read_double(&tau) || !read_double(&alpha) || !read_double(&beta) || !read_double(&max_reproj) ||
                !read_int(&strict) || !read_int(&format) || !read_int(&K) || H < 1 || W < 1 || K < 1 || (format != 0 && format != 1)) {
                printf("bad map header\n");
                return 2;
            }
            std::vector<float> map((size_t)3 * H * W);
            for (auto& m : map) {
                double d;
                if (!read_double(&d)) return 2;
                m = (float)d;
            }
            std::vector<double> rt((size_t)K * 6);
            std::vector<float> T((size_t)K * 16);
            for (size_t i = 0; i < (format == 0 ? rt.size() : T.size()); i++) {
                double d;
                if (!read_double(&d)) return 2;
                if (format == 0) rt[i] = d;
                else T[i] = (float)d;
            }
            const Cam cam{(double)(float)focal, (double)(float)focal, (double)(float)ppx, (double)(float)ppy};  // (KArgs carries floats: make_cam)
            for (int k = 0; k < K; k++) {
                double pose[6], row[ESAC_VERIFY_DOUBLES_K];
                const bool ok = verify_fetch_pose(format == 0 ? (const void*)rt.data() : (const void*)T.data(), format, (size_t)k, pose);
                if (!ok) verify_row_nan(ESAC_VERIFY_BAD_POSE_K, row);
                else if (strict) verify_pose_host<true>(map.data(), H, W, sub, sx, sy, cam, pose, (float)tau, (float)alpha, (float)beta, (float)max_reproj, row);
                else verify_pose_host<false>(map.data(), H, W, sub, sx, sy, cam, pose, (float)tau, (float)alpha, (float)beta, (float)max_reproj, row);
                printf("row %d", ok ? 1 : 0);
                print_doubles(row, ESAC_VERIFY_DOUBLES_K);
                printf("\n");
            }
        } else if (!strcmp(kind, "fetch")) {
            float T[16];
            for (auto& t : T) {
                double d;
                if (!read_double(&d)) return 2;
                t = (float)d;
            }
            double mine[6], gt[16], theirs[6] = {0, 0, 0, 0, 0, 0};
            const bool ok_mine = verify_fetch_pose(T, ESAC_VERIFY_POSE_4X4_K, 0, mine);
            const bool ok_theirs = gt_from_pose(T, gt, theirs);
            printf("fetch %d", ok_mine ? 1 : 0);
            print_doubles(mine, 6);
            printf(" %d", ok_theirs ? 1 : 0);
            print_doubles(theirs, 6);
            printf("\n");
        } else {
            printf("unknown request %s\n", kind);
            return 2;
        }
    }
    return 0;
}
