// ragged_backward_policy_probe.cpp -- stand-alone host program over esac_amd/csrc/ragged_policy.hpp (no HIP header, no GPU): the
// checks of a ragged TRAINING batch (check_bwd_shapes_entry, check_bwd_shapes) in the order the C ABI host runs them, as
// tests/test_ragged_backward_policy_host.py drives them.  One request per input line, one answer per output line:
//   bwd who table E H W sub sc_stride grad_stride B  {shift_x shift_y focal h w} x B  ->  bwd|<status>|<all_vec or -1>|<message>
//       who: 0 esac_hip_backward_batch_shapes, 1 esac_hip_backward_batch_dev_shapes; table: 0 = a null h_cams
//   chunk budget cap P left                                                             ->  chunk|<frames of the next chunk>|<slot bytes>
//       (a ragged batch's chunks: bwd_slot_bytes of the capacity P, whatever the frames' own sizes)
#include <inttypes.h>
#include <stdio.h>
#include <string.h>

#include <sstream>
#include <string>
#include <vector>

#include "../../esac_amd/csrc/ragged_policy.hpp"

using namespace esac;

static esac_hip_params params(int E, int H, int W, int sub) {
    esac_hip_params p;
    memset(&p, 0, sizeof(p));
    p.E = E; p.H = H; p.W = W; p.N = 64;
    p.focal = 525.0f; p.ppx = 320.0f; p.ppy = 240.0f;
    p.inlier_thresh = 10.0f; p.inlier_alpha = 100.0f; p.inlier_beta = 0.5f; p.max_reproj = 100.0f;
    p.sub_sampling = sub;
    p.max_ref_steps = -1;
    return p;
}

// corr_entries(P) of esac_kernels.hpp (a HIP header): 4 wavefronts, regions of whole 2048-cell trips
static long long corr_entries_host(int P) { return (long long)((P + 2047) / 2048 * 512) * 4; }

int main() {
    char line[1 << 16];
    while (fgets(line, sizeof(line), stdin)) {
        std::istringstream in(line);
        std::string kind;
        if (!(in >> kind)) continue;
        if (kind == "bwd") {
            int who, table, E, H, W, sub, B;
            long long sc_stride, grad_stride;
            in >> who >> table >> E >> H >> W >> sub >> sc_stride >> grad_stride >> B;
            std::vector<esac_hip_frame_cam> cams((size_t)(B > 0 ? B : 0));
            for (auto& c : cams) {
                memset(&c, 0, sizeof(c));
                in >> c.shift_x >> c.shift_y >> c.focal >> c.reserved[0] >> c.reserved[1];
                c.ppx = 320.0f; c.ppy = 240.0f;
                c.reserved[2] = 0x7fc00000;  // (garbage the library must overwrite, never read)
            }
            if (!in) { printf("bwd|bad row\n"); continue; }
            const char* const name = who ? "esac_hip_backward_batch_dev_shapes" : "esac_hip_backward_batch_shapes";
            const esac_hip_params p = params(E, H, W, sub);
            g_err[0] = 0;
            bool all_vec = false;
            // the host's order: the table, the shared-shape call's own checks (the capacity is no bound of the gradient stride:
            // INT64_MAX stands in), the parameters, then every frame and its gradient slot
            int rc = check_bwd_shapes_entry(name, table != 0);
            if (!rc) rc = check_batch_call("esac_hip_backward_batch", true, &p, B, true, who != 0, true, (int64_t)sc_stride, INT64_MAX);
            if (!rc) rc = check_args(true, true, &p, B, -1, true);
            if (!rc) rc = check_bwd_shapes(name, &p, B, cams.data(), (int64_t)sc_stride, (int64_t)grad_stride, &all_vec);
            printf("bwd|%d|%d|%s\n", rc, rc ? -1 : (int)all_vec, rc ? g_err : "");
        } else if (kind == "chunk") {
            long long budget;
            int cap, P, left;
            in >> budget >> cap >> P >> left;
            const long long slot = bwd_slot_bytes(P, corr_entries_host(P));
            printf("chunk|%d|%lld\n", chunk_frames(budget, cap, slot, left), slot);
        } else {
            printf("%s|unknown request\n", kind.c_str());
        }
    }
    return 0;
}
