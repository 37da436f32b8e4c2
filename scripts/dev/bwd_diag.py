"""Which gradient path of which slot deviates on a frame of bwd_sweep.py -- from the ORACLE (upstream differences included) and
from the REPLAY of the device's own stages (tests/bwd_replay.py: that kernel's rounding alone): python scripts/dev/bwd_diag.py <k> ..."""
import os
import sys

import numpy as np

sys.path.insert(0, os.environ.get("GRAFT_REPO_ROOT", "."))
from esac_amd import api, synthetic as S  # noqa: E402
from oracle import esac_oracle as O  # noqa: E402
from tests import bwd_replay as R  # noqa: E402

eng = api.Engine(0)
for k in [int(v) for v in sys.argv[1:]]:
    E = 1 if k % 3 else 3
    f = S.make_frame(2000 + k, E=E, true_expert=k % E)
    N = (64, 128, 256)[k % 3]
    ha = S.gating_assignment(f, N, mode="gating" if E > 1 else "single")
    gt = np.array(f["gt_pose"], np.float32)
    gt[:3, 3] += np.float32(0.02 * (k % 5))
    alpha = (100.0, 30.0)[k % 2]
    c = R.case_of(f, ha, gt, np.zeros_like(f["coords"]), alpha, 55, k)
    ref = R.run_oracle(O, c)
    out, g, stages, dev = R.run_device(eng, api, c)
    rp = R.replay_with_inputs(O, c, stages)
    scale = np.abs(ref["grad"]).max()
    print("frame %d: E %d N %d alpha %g slots %d, |grad|max %.3g, total grad err %.2e; against the replay: direct term %.3g of its bar, "
          "path I %.3g of its bar (%d slots)" % ((k, E, N, alpha, len(dev["slots"]), scale, np.abs(g - ref["grad"]).max() / scale) + R.slab_ratios(c, stages, dev, rp)))
    for s_, h in enumerate(dev["slots"]):
        r1, r2 = ref["grad_path1"][h].T, ref["grad_path2"][h].T  # [3,P], cells as y * W + x on both sides
        pr = ref["probs"][h]
        d1 = np.abs(dev["slab1"][s_] - r1).max() * pr / scale
        d2 = np.abs(dev["slab2"][s_] - r2).max() / scale
        if d1 > 2e-7 or d2 > 2e-7:
            print("   slot %2d hyp %3d prob %.3g  path I err %.2e (|pI| %.3g, oracle %.3g; replay %.2e)  path II err %.2e (|pII| %.3g; replay %.2e)  steps %d inliers %d" % (
                s_, h, pr, d1, np.abs(dev["slab1"][s_]).max(), np.abs(r1).max(), np.abs(dev["slab1"][s_] - rp["grad_path1"][h].T).max() * pr / scale,
                d2, np.abs(dev["slab2"][s_]).max(), np.abs(dev["slab2"][s_] - rp["grad_path2"][h].T).max() / scale, dev["info"][s_][2], dev["info"][s_][1]))
