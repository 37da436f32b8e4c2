// ragged_policy_probe.cpp -- stand-alone host program over esac_amd/csrc/batch_plan.hpp and ragged_policy.hpp (no HIP header, no
// GPU): the forward route's plan of a ragged batch (plan_batch: the function the C ABI host calls, so the order of checks is the
// library's) and the per-frame re-score margin (shape_record) as tests/test_ragged_policy_host.py drives them.
// One request per input line, one answer per output line:
//   check E H W sub stride B  {shift_x shift_y focal h w} x B   ->  check|<status>|<all_vec or -1>|<message>
//       (all_vec: KArgs::shapes == 1; of one frame, which the plan hands to the single call: that call's width is a multiple of 4)
//   margin alpha rescore_margin H W h w                         ->  margin|<bits of the frame's record>|<bits of call_scalars on h x w>
#include <inttypes.h>
#include <stdio.h>
#include <string.h>

#include <sstream>
#include <string>
#include <vector>

#include "../../esac_amd/csrc/batch_plan.hpp"

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

int main() {
    char line[1 << 16];
    while (fgets(line, sizeof(line), stdin)) {
        std::istringstream in(line);
        std::string kind;
        if (!(in >> kind)) continue;
        if (kind == "check") {
            int E, H, W, sub, B;
            long long stride;
            in >> E >> H >> W >> sub >> stride >> B;
            std::vector<esac_hip_frame_cam> cams((size_t)(B > 0 ? B : 0));
            cams.reserve(1);  // (B = 0: still a table)
            for (auto& c : cams) {
                memset(&c, 0, sizeof(c));
                in >> c.shift_x >> c.shift_y >> c.focal >> c.reserved[0] >> c.reserved[1];
                c.ppx = 320.0f; c.ppy = 240.0f;
                c.reserved[2] = 0x7fc00000;  // (garbage the library must overwrite, never read)
            }
            if (!in) { printf("check|bad row\n"); continue; }
            const esac_hip_params p = params(E, H, W, sub);
            g_err[0] = 0;
            BatchPlan plan;
            const int rc = plan_batch(BATCH_FORWARD, "esac_hip_forward_batch_shapes", true, true, true, &p, B, cams.data(), true, (int64_t)stride, 0, &plan);
            const bool all_vec = plan.shapes ? plan.shapes == 1 : (plan.p.W & 3) == 0;
            printf("check|%d|%d|%s\n", rc, rc ? -1 : (int)all_vec, rc ? g_err : "");
        } else if (kind == "margin") {
            float alpha, rescore;
            int H, W, h, w;
            in >> alpha >> rescore >> H >> W >> h >> w;
            esac_hip_params cap = params(1, H, W, 8), own = params(1, h, w, 8);
            cap.inlier_alpha = own.inlier_alpha = alpha;
            cap.rescore_margin = own.rescore_margin = rescore;
            esac_hip_frame_cam c;
            memset(&c, 0, sizeof(c));
            c.focal = 525.0f;
            c.reserved[0] = h; c.reserved[1] = w; c.reserved[2] = -1;
            const esac_hip_frame_cam r = shape_record(&cap, c);
            const float single = call_scalars(&own, 64).margin;
            uint32_t a, b;
            memcpy(&a, &r.reserved[2], 4);
            memcpy(&b, &single, 4);
            const bool rest = r.shift_x == c.shift_x && r.shift_y == c.shift_y && r.focal == c.focal && r.reserved[0] == h && r.reserved[1] == w;
            printf("margin|%08" PRIx32 "|%08" PRIx32 "|%d\n", a, b, (int)rest);
        } else {
            printf("%s|unknown request\n", kind.c_str());
        }
    }
    return 0;
}
