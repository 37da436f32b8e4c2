"""Pose verification against the forward batch it sits behind, in one process (bench.py stays the headline measurement).

For each shape (B frames, K poses per frame, grid, 10 experts) it times `Engine.verify_batch` -- K poses near the ground truth on
the true expert's map of every frame -- and, next to it in the same run, `Engine.forward_batch` (asynchronous form, 256
hypotheses) on the same maps: device events around --calls back-to-back calls of each after a warm-up, the two alternated --reps
times, medians.  One JSON line per shape: ms per call of each and their ratio, the kernel's algorithmic bytes (12 B per cell and
pose: three float32 planes) and fp64 operations per call, computed from the shape.  The achieved rate needs the KERNEL's time:
run one shape under a kernel trace in a run of its own and divide --

    python scripts/bench_verify_batch.py [--calls 200] [--reps 5] [--shapes 32x1@60x80,32x8@60x80,256x1@60x80,4x1@480x640]
    python scripts/bench_verify_batch.py --only 256x1@60x80 --calls 200 --no-forward     # e.g. under rocprofv3 --kernel-trace --stats
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from esac_amd import api  # noqa: E402
from esac_amd import synthetic as S  # noqa: E402

E, N_HYPS, DISTINCT = 10, 256, 8
# fp64 operations per cell and pose of k_verify_batch (esac_amd/csrc/verify_math.hpp: verify_accumulate), divisions, square roots
# and the exponential counted as one each: the projection and its float error 29, the soft-inlier term 4, the residuals and the
# two Jacobian rows 81 (the projection shared), the 21 sums of A 84, SSE / score / count 6
FP64_OPS_PER_CELL = 29 + 4 + 81 + 84 + 6
BYTES_PER_CELL = 12


def rvec_tvec(T):
    """camera pose 4x4 (camera -> scene) -> rvec | tvec (scene -> camera)"""
    Ti = np.linalg.inv(T)
    R = Ti[:3, :3]
    w = 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    s, c = np.linalg.norm(w), 0.5 * (np.trace(R) - 1.0)
    return np.concatenate([w * (np.arctan2(s, c) / s) if s > 0 else np.zeros(3), Ti[:3, 3]])


def make_inputs(B, K, H, W):
    sub = 8 if (H, W) == (60, 80) else 1
    frames = [S.make_frame(800 + b, E=E, true_expert=b % E, H=H, W=W, sub=sub) for b in range(min(B, DISTINCT))]
    idx = [b % len(frames) for b in range(B)]
    sc = torch.from_numpy(np.stack([f["coords"] for f in frames])).cuda()[torch.tensor(idx, device="cuda")].contiguous()
    rng = np.random.default_rng(1)
    poses = np.stack([np.stack([rvec_tvec(frames[i]["gt_pose"]) + (rng.normal(size=6) * 2e-3 if k else 0.0) for k in range(K)]) for i in idx])
    experts = np.array([[frames[i]["true_expert"]] * K for i in idx], np.int32)
    ha = np.stack([S.gating_assignment(frames[i], N_HYPS, mode="gating", rng=np.random.default_rng(7 + b)) for b, i in enumerate(idx)])
    return frames[0], sub, sc, torch.from_numpy(poses).cuda(), torch.from_numpy(experts).cuda(), torch.from_numpy(ha).cuda()


def timed(fn, calls):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(calls):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="32x1@60x80,32x8@60x80,256x1@60x80,4x1@480x640")
    ap.add_argument("--only", default=None)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-forward", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_verify_batch: no HIP device -- nothing is measured without one")
    eng = api.Engine(0)
    for shape in (args.only or args.shapes).split(","):
        bk, grid = shape.split("@")
        B, K = (int(v) for v in bk.split("x"))
        H, W = (int(v) for v in grid.split("x"))
        f0, sub, sc, poses, experts, ha = make_inputs(B, K, H, W)
        pv = eng.make_params(E, H, W, K, focal=f0["focal"], ppx=f0["ppx"], ppy=f0["ppy"], sub_sampling=sub)
        out = torch.empty((B, K, api.VERIFY_DOUBLES), dtype=torch.float64, device="cuda")
        records = torch.zeros((B, api.RES_DOUBLES), dtype=torch.float64, device="cuda")
        calls = [0]

        def verify():
            eng.verify_batch(sc, poses, experts, pv, out=out)

        def forward():
            pf = eng.make_params(E, H, W, N_HYPS, focal=f0["focal"], ppx=f0["ppx"], ppy=f0["ppy"], sub_sampling=sub, call=calls[0])
            calls[0] += B
            eng.forward_batch(sc, ha, pf, result_out=records, want_host=False)

        timed(verify, args.warmup)
        if not args.no_forward:
            timed(forward, args.warmup)
        tv, tf = [], []
        for _ in range(args.reps):
            tv.append(timed(verify, args.calls))
            if not args.no_forward:
                tf.append(timed(forward, args.calls))
        torch.cuda.synchronize()
        rows = out.cpu().numpy()
        ms_v = float(np.median(tv))
        line = {"bench": "verify_batch", "B": B, "K": K, "grid": "%dx%d" % (H, W), "experts": E, "calls": args.calls, "reps": args.reps,
                "verify_ms_per_call": round(ms_v, 5), "verify_ms_spread": [round(min(tv), 5), round(max(tv), 5)],
                "algorithmic_bytes_per_call": BYTES_PER_CELL * H * W * B * K, "fp64_ops_per_call": FP64_OPS_PER_CELL * H * W * B * K,
                "fp64_ops_per_cell": FP64_OPS_PER_CELL, "status_ok": int((rows[:, :, api.VERIFY_STATUS] == 0).sum()),
                "mean_inliers": round(float(rows[:, :, api.VERIFY_N].mean()), 1)}
        if tf:
            ms_f = float(np.median(tf))
            line.update({"forward_hypotheses": N_HYPS, "forward_ms_per_call": round(ms_f, 5), "forward_ms_spread": [round(min(tf), 5), round(max(tf), 5)],
                         "verify_over_forward": round(ms_v / ms_f, 4)})
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
