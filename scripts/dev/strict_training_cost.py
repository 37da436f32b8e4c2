"""Cost of ESAC_FLAG_STRICT_TRAINING: blocking esac.backward, default against strict, at cfg2's shape (1 expert, 256 hypotheses)
and at 10 experts / 1024 hypotheses -- medians of `calls` calls, the two alternated `rounds` times.
python scripts/dev/strict_training_cost.py [calls, default 200] [rounds, default 3]"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import esac  # noqa: E402
from esac_amd import synthetic as S  # noqa: E402

calls = int(sys.argv[1]) if len(sys.argv) > 1 else 200
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 3
for name, E, N, mode in (("cfg2 (1 expert, 256)", 1, 256, "single"), ("10 experts, 1024", 10, 1024, "gating")):
    f = S.make_frame(700, E=E, true_expert=0)
    ha = torch.from_numpy(S.gating_assignment(f, N, mode=mode)).cuda()
    sc = torch.from_numpy(f["coords"]).cuda()
    gt = np.array(f["gt_pose"], np.float32)
    gt[:3, 3] += np.float32(0.03)
    gt = torch.from_numpy(gt)
    g = torch.zeros_like(sc)

    def run(strict, n):
        esac.set_strict_training(strict)
        esac.set_seed(1305, 0)
        ts = []
        for _ in range(n):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            esac.backward(sc, g, ha, gt, 1.0, 100.0, 100.0, 0, 0, f["focal"], f["ppx"], f["ppy"], 10.0, 100.0, 0.5, 100.0, f["sub"])
            ts.append(time.perf_counter() - t0)
        esac.set_strict_training(False)
        return 1e3 * float(np.median(ts))

    run(False, 20), run(True, 20)  # warm-up of both routes
    d, s = [], []
    for _ in range(rounds):
        d.append(run(False, calls))
        s.append(run(True, calls))
    print("%s: esac.backward default %s ms, strict %s ms, ratio %.2f" % (
        name, " ".join("%.4f" % v for v in d), " ".join("%.4f" % v for v in s), np.median(s) / np.median(d)), flush=True)
