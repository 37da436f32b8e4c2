// ragged_backward_policy_probe.cpp -- stand-alone host program over esac_amd/csrc/batch_plan.hpp and ragged_policy.hpp (no HIP
// header, no GPU): the plan of a batch call (plan_batch: the function the C ABI host calls, so the order of checks is the
// library's), as tests/test_ragged_backward_policy_host.py drives it.  One request per input line, one answer per output line:
//   bwd who table E H W sub sc_stride grad_stride B  {shift_x shift_y focal h w} x B  ->  bwd|<status>|<all_vec or -1>|<message>
//       a ragged training batch.  who: 0 esac_hip_backward_batch_shapes, 1 esac_hip_backward_batch_dev_shapes; table: 0 = a null h_cams
//       (all_vec: KArgs::shapes == 1; of one frame, which the plan hands to the shared-shape call: that call's width is a multiple of 4)
//   plan route ragged table E H W sub sc_stride grad_stride B  {shift_x shift_y focal h w} x B
//       ->  plan|<status>|<stage>|<shapes>|<H>|<W>|<frame 0's cells>|<record b's margin bits:the single call's on h_b x w_b>,...|<message>
//       route: 0 forward, 1 blocking training batch, 2 asynchronous training batch; the records are plan_records'
//   chunk budget cap P left                                                             ->  chunk|<frames of the next chunk>|<slot bytes>
//       (a ragged batch's chunks: bwd_slot_bytes of the capacity P, whatever the frames' own sizes)
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
            cams.reserve(1);  // (B = 0: still a table)
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
            BatchPlan plan;
            const int rc = plan_batch(who ? BATCH_TRAIN_ASYNC : BATCH_TRAIN_BLOCKING, name, true, true, true, &p, B, table ? cams.data() : nullptr, true,
                                      (int64_t)sc_stride, (int64_t)grad_stride, &plan);
            const bool all_vec = plan.shapes ? plan.shapes == 1 : (plan.p.W & 3) == 0;
            printf("bwd|%d|%d|%s\n", rc, rc ? -1 : (int)all_vec, rc ? g_err : "");
        } else if (kind == "plan") {
            int route, ragged, table, E, H, W, sub, B;
            long long sc_stride, grad_stride;
            in >> route >> ragged >> table >> E >> H >> W >> sub >> sc_stride >> grad_stride >> B;
            std::vector<esac_hip_frame_cam> cams((size_t)(B > 0 ? B : 0));
            cams.reserve(1);  // (B = 0: still a table)
            for (auto& c : cams) {
                memset(&c, 0, sizeof(c));
                in >> c.shift_x >> c.shift_y >> c.focal >> c.reserved[0] >> c.reserved[1];
                c.ppx = 320.0f; c.ppy = 240.0f;
                c.reserved[2] = 0x7fc00000;
            }
            if (!in) { printf("plan|bad row\n"); continue; }
            const char* const names[3] = {"esac_hip_forward_batch_shapes", "esac_hip_backward_batch_shapes", "esac_hip_backward_batch_dev_shapes"};
            const esac_hip_params p = params(E, H, W, sub);
            g_err[0] = 0;
            BatchPlan plan;
            const int rc = plan_batch((BatchRoute)route, names[route], true, true, true, &p, B, table ? cams.data() : nullptr, ragged != 0,
                                      (int64_t)sc_stride, (int64_t)grad_stride, &plan);
            if (rc) { printf("plan|%d|-1|-1|-1|-1|-1||%s\n", rc, g_err); continue; }
            std::string margins;
            std::vector<esac_hip_frame_cam> rec(cams.size());
            if (plan.stage) plan_records(plan, cams.data(), B, rec.data());
            for (size_t b = 0; plan.stage && b < rec.size(); b++) {
                esac_hip_params own = plan.p;  // the single call on frame b's grid
                own.H = cams[b].reserved[0]; own.W = cams[b].reserved[1];
                const float single = call_scalars(&own, 64).margin;
                uint32_t m, s1;
                memcpy(&m, &rec[b].reserved[2], 4);
                memcpy(&s1, &single, 4);
                char buf[32];
                snprintf(buf, sizeof(buf), "%s%08" PRIx32 ":%08" PRIx32, b ? "," : "", m, s1);
                margins += buf;
            }
            const bool table_less = !table && !ragged;  // (the forward route leaves the block to the caller then)
            printf("plan|0|%d|%d|%d|%d|%zu|%s|\n", (int)plan.stage, plan.shapes, table_less && route == 0 ? H : plan.p.H, table_less && route == 0 ? W : plan.p.W,
                   plan.cells0, margins.c_str());
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
