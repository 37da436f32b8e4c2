"""Batched training path vs sequential single calls, in one process (bench.py stays the headline measurement).

For cfg2 (1 expert, 256 hypotheses, 60x80) and cfg3's shape (10 experts, 1024 hypotheses, gating assignment) it times
`Engine.backward_batch` over B frames against B sequential `Engine.backward_device` calls on the same frames and counters,
alternating the two after a warm-up, and prints one JSON line per (config, B): ms per frame of each, the speed-up, and the
mean number of slots (hypotheses with p >= PROB_THRESH) per frame.

    python scripts/bench_backward_batch.py [--batches 1,8,32,128] [--reps 5] [--configs cfg2,cfg3]
    python scripts/bench_backward_batch.py --only-batch 32 --configs cfg2 --reps 3   # one shape, e.g. under a kernel trace
    python scripts/bench_backward_batch.py --strict-training  # the same measurement with ESAC_FLAG_STRICT_TRAINING
    python scripts/bench_backward_batch.py --per-frame-cams   # after each shared-camera line, the same frames and counters with a
                                                              # shift (|shift| <= sub/2) and a focal length per frame
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


def frame_cam(b, sub=8):
    """Frame b's own camera for --per-frame-cams: a shift within +-sub/2 and a focal length between 480 and 720."""
    rng = np.random.default_rng(5000 + b)
    sx, sy = (int(v) for v in rng.integers(-(sub // 2), sub // 2 + 1, size=2))
    return (sx, sy), float(480 + 8 * int(rng.integers(0, 31)))


def make_inputs(cfg, B, per_frame=False):
    if per_frame:
        frames = [S.make_frame(700 + b, E=cfg["E"], true_expert=b % cfg["E"], shift=frame_cam(b)[0], focal=frame_cam(b)[1])
                  for b in range(B)]
    else:
        frames = [S.make_frame(700 + b, E=cfg["E"], true_expert=b % cfg["E"]) for b in range(B)]
    has = [S.gating_assignment(f, cfg["N"], mode=cfg["mode"]) for f in frames]
    gts = []
    for b, f in enumerate(frames):
        gt = np.array(f["gt_pose"], np.float64)
        gt[:3, 3] += np.random.default_rng(b).normal(size=3) * 0.05
        gts.append(gt.astype(np.float32))
    sc = torch.from_numpy(np.stack([f["coords"] for f in frames])).cuda()
    ha = torch.from_numpy(np.stack(has)).cuda()
    cams = api.make_cams([f["shift"][0] for f in frames], [f["shift"][1] for f in frames], [f["focal"] for f in frames],
                         [f["ppx"] for f in frames], [f["ppy"] for f in frames])
    return frames[0], sc, ha, np.stack(gts), cams


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,8,32,128")
    ap.add_argument("--configs", default="cfg2,cfg3")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only-batch", type=int, default=0, help="time the batched call only, at this B")
    ap.add_argument("--per-frame-cams", action="store_true",
                    help="also time every (config, B) with a shift and a focal length per frame (one more JSON line, cams=per-frame)")
    ap.add_argument("--strict-training", action="store_true",
                    help="every call with ESAC_FLAG_STRICT_TRAINING (the verification route: each JSON line says strict_training=true)")
    args = ap.parse_args()
    eng = api.Engine(0)
    batches = [args.only_batch] if args.only_batch else [int(x) for x in args.batches.split(",")]
    for name in args.configs.split(","):
        cfg = CONFIGS[name]
        shared = make_inputs(cfg, max(batches))
        own = make_inputs(cfg, max(batches), per_frame=True) if args.per_frame_cams else None
        E, _, H, W = shared[0]["coords"].shape
        grads = torch.zeros((max(batches), E, 3, H, W), dtype=torch.float32, device="cuda")
        for B, per_frame in [(B, pf) for B in batches for pf in ((False, True) if own else (False,))]:
            f0, sc, ha, gts, cams = own if per_frame else shared

            def params(call, b=0):  # (a sequential call of a per-frame batch carries frame b's camera in its own params)
                c = cams[b] if per_frame else cams[0]
                return eng.make_params(E, H, W, cfg["N"], shift_x=int(c["shift_x"]), shift_y=int(c["shift_y"]), focal=float(c["focal"]),
                                       ppx=float(c["ppx"]), ppy=float(c["ppy"]), sub_sampling=f0["sub"], inlier_alpha=100.0, call=call,
                                       strict_training=args.strict_training)

            def run_batch():
                return eng.backward_batch(sc[:B], grads[:B], ha[:B], gts[:B], 1.0, 100.0, 100.0, params(0),
                                          cams=cams[:B] if per_frame else None)

            def run_seq():
                for b in range(B):
                    eng.backward_device(sc[b], grads[b], ha[b], gts[b], 1.0, 100.0, 100.0, params(b, b))

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
            line = {"config": name, "B": B, "E": E, "N": cfg["N"], "grid": "%dx%d" % (H, W), "cams": "per-frame" if per_frame else "shared",
                    "batch_ms_per_frame": round(1e3 * float(np.median(t_batch)) / B, 4),
                    "slots_per_frame": round(float(out[:, 1].mean()), 2), "reps": args.reps, "strict_training": args.strict_training}
            if t_seq:
                line["sequential_ms_per_frame"] = round(1e3 * float(np.median(t_seq)) / B, 4)
                line["speedup"] = round(float(np.median(t_seq)) / float(np.median(t_batch)), 2)
            print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
