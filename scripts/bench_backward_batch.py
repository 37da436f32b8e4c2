"""Batched training path vs sequential single calls, in one process (bench.py stays the headline measurement).

For cfg2 (1 expert, 256 hypotheses, 60x80) and cfg3's shape (10 experts, 1024 hypotheses, gating assignment) it times
`Engine.backward_batch` over B frames against B sequential `Engine.backward_device` calls on the same frames and counters,
alternating the two after a warm-up, and prints one JSON line per (config, B): ms per frame of each, the speed-up, and the
mean number of slots (hypotheses with p >= PROB_THRESH) per frame.

    python scripts/bench_backward_batch.py [--batches 1,8,32,128] [--reps 5] [--configs cfg2,cfg3]
    python scripts/bench_backward_batch.py --only-batch 32 --configs cfg2 --reps 3   # one shape, e.g. under a kernel trace
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from esac_amd import api  # noqa: E402
from esac_amd import synthetic as S  # noqa: E402

CONFIGS = {"cfg2": dict(E=1, N=256, mode="single"), "cfg3": dict(E=10, N=1024, mode="gating")}


def make_inputs(cfg, B):
    frames = [S.make_frame(700 + b, E=cfg["E"], true_expert=b % cfg["E"]) for b in range(B)]
    has = [S.gating_assignment(f, cfg["N"], mode=cfg["mode"]) for f in frames]
    gts = []
    for b, f in enumerate(frames):
        gt = np.array(f["gt_pose"], np.float64)
        gt[:3, 3] += np.random.default_rng(b).normal(size=3) * 0.05
        gts.append(gt.astype(np.float32))
    sc = torch.from_numpy(np.stack([f["coords"] for f in frames])).cuda()
    ha = torch.from_numpy(np.stack(has)).cuda()
    return frames[0], sc, ha, np.stack(gts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,8,32,128")
    ap.add_argument("--configs", default="cfg2,cfg3")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only-batch", type=int, default=0, help="time the batched call only, at this B")
    args = ap.parse_args()
    eng = api.Engine(0)
    batches = [args.only_batch] if args.only_batch else [int(x) for x in args.batches.split(",")]
    for name in args.configs.split(","):
        cfg = CONFIGS[name]
        f0, sc, ha, gts = make_inputs(cfg, max(batches))
        E, _, H, W = f0["coords"].shape
        grads = torch.zeros((max(batches), E, 3, H, W), dtype=torch.float32, device="cuda")

        def params(call):
            return eng.make_params(E, H, W, cfg["N"], focal=f0["focal"], ppx=f0["ppx"], ppy=f0["ppy"], sub_sampling=f0["sub"],
                                   inlier_alpha=100.0, call=call)

        for B in batches:
            def run_batch():
                return eng.backward_batch(sc[:B], grads[:B], ha[:B], gts[:B], 1.0, 100.0, 100.0, params(0))

            def run_seq():
                for b in range(B):
                    eng.backward_device(sc[b], grads[b], ha[b], gts[b], 1.0, 100.0, 100.0, params(b))

            out = run_batch()  # warm-up (grows the slot workspace), then alternate
            if not args.only_batch:
                run_seq()
            t_batch, t_seq = [], []
            for _ in range(args.reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = run_batch()
                t_batch.append(time.perf_counter() - t0)
                if args.only_batch:
                    continue
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                run_seq()
                t_seq.append(time.perf_counter() - t0)
            line = {"config": name, "B": B, "E": E, "N": cfg["N"], "grid": "%dx%d" % (H, W),
                    "batch_ms_per_frame": round(1e3 * float(np.median(t_batch)) / B, 4),
                    "slots_per_frame": round(float(out[:, 1].mean()), 2), "reps": args.reps}
            if t_seq:
                line["sequential_ms_per_frame"] = round(1e3 * float(np.median(t_seq)) / B, 4)
                line["speedup"] = round(float(np.median(t_seq)) / float(np.median(t_batch)), 2)
            print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
