// verify_policy_probe.cpp -- stand-alone host program over esac_amd/csrc/verify_policy.hpp (no HIP header, no GPU): plan_verify,
// the function esac_hip_verify_batch calls before it stages or launches anything, as tests/test_verify_args.py drives it.
// One request per input line, one answer per output line:
//   plan ctx params B K sc poses format experts out ragged table E H W sub stride flags  {shift_x shift_y focal h w} x max(B, 0)
//     -> plan|<status>|<stage>|<shapes>|<plan H>x<plan W>|<plan N>|<message>
//   (ctx, params, sc, poses, experts, out, table: 1 there, 0 null)
#include <stdio.h>
#include <string.h>

#include <sstream>
#include <string>
#include <vector>

#include "../../esac_amd/csrc/verify_policy.hpp"

using namespace esac;

int main() {
    char line[1 << 16];
    while (fgets(line, sizeof(line), stdin)) {
        std::istringstream in(line);
        std::string kind;
        if (!(in >> kind)) continue;
        if (kind != "plan") {
            printf("%s|unknown request\n", kind.c_str());
            continue;
        }
        int ctx, params, B, K, sc, poses, format, experts, out, ragged, table, E, H, W, sub, flags;
        long long stride;
        in >> ctx >> params >> B >> K >> sc >> poses >> format >> experts >> out >> ragged >> table >> E >> H >> W >> sub >> stride >> flags;
        std::vector<esac_hip_frame_cam> cams((size_t)(B > 0 && B <= 4096 ? B : 0));
        cams.reserve(1);
        for (auto& c : cams) {
            memset(&c, 0, sizeof(c));
            in >> c.shift_x >> c.shift_y >> c.focal >> c.reserved[0] >> c.reserved[1];
            c.ppx = 64.0f; c.ppy = 48.0f;
            c.reserved[2] = 0x7fc00000;  // (garbage the library must overwrite, never read)
        }
        if (!in) { printf("plan|bad row\n"); continue; }
        esac_hip_params p;
        memset(&p, 0, sizeof(p));
        p.E = E; p.H = H; p.W = W; p.N = 0;  // (N is no argument of this call)
        p.focal = 100.0f; p.ppx = 64.0f; p.ppy = 48.0f;
        p.inlier_thresh = 10.0f; p.inlier_alpha = 100.0f; p.inlier_beta = 0.5f; p.max_reproj = 100.0f;
        p.sub_sampling = sub;
        p.flags = flags;
        g_err[0] = 0;
        BatchPlan plan;
        memset(&plan.p, 0, sizeof(plan.p));
        const int rc = plan_verify(ctx != 0, B, K, sc != 0, (int64_t)stride, poses != 0, format, experts != 0, params ? &p : nullptr,
                                   table ? cams.data() : nullptr, ragged != 0, out != 0, &plan);
        printf("plan|%d|%d|%d|%dx%d|%d|%s\n", rc, rc ? -1 : (int)plan.stage, rc ? -1 : plan.shapes, rc ? 0 : plan.p.H, rc ? 0 : plan.p.W,
               rc ? 0 : plan.p.N, rc ? g_err : "");
    }
    return 0;
}
