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
    python scripts/bench_backward_batch.py --asynchronous [--batches 8,32,128] [--steps 4] [--reps 5]
                                                              # Engine.backward_batch_async against the blocking batch (see main_async)
    python scripts/bench_backward_batch.py --pose-records [--batches 1,8,32] [--steps 4] [--reps 5]
                                                              # training calls armed with pose records against unarmed ones, and
                                                              # against unarmed + one blocking forward per frame (see main_pose_records)
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


def main_async(args):
    """--asynchronous: K = --steps batches both ways in this process, interleaved rep by rep after a warm-up of both.
      (a) K blocking `backward_batch` calls;
      (b) K `backward_batch_async` calls enqueued back to back (device ground truth), one synchronisation at the end.
    Per (config, B) one JSON line: wall time per frame of each (for (a) the host waits inside every call, so this is its device
    time plus its launch-to-drain gaps; for (b) the stream never drains), the host time spent inside the calls, and a
    step-overlap leg: a fixed filler (--filler-matmuls fp32 4096^3 products, standing in for the CNN backward) enqueued behind
    each call, K steps both ways.  Medians over --reps, with the min..max spread of each."""
    eng = api.Engine(0)
    batches = [int(x) for x in (args.batches if args.batches != "1,8,32,128" else "8,32,128").split(",")]
    K = args.steps
    fa = torch.randn(4096, 4096, device="cuda")
    fc = torch.empty_like(fa)

    def filler():
        for _ in range(args.filler_matmuls):
            torch.mm(fa, fa, out=fc)

    for name in args.configs.split(","):
        cfg = CONFIGS[name]
        f0, sc_all, ha_all, gts_all, _ = make_inputs(cfg, max(batches))
        E, _, H, W = f0["coords"].shape
        grads = torch.zeros((max(batches), E, 3, H, W), dtype=torch.float32, device="cuda")
        gt_dev_all = torch.from_numpy(gts_all).cuda()
        for B in batches:
            sc, ha, gts, gt_dev, g = sc_all[:B], ha_all[:B], gts_all[:B], gt_dev_all[:B], grads[:B]
            recs = [torch.empty((B, 4), dtype=torch.float64, device="cuda") for _ in range(K)]

            def params(call):
                return eng.make_params(E, H, W, cfg["N"], focal=f0["focal"], ppx=f0["ppx"], ppy=f0["ppy"], sub_sampling=f0["sub"],
                                       inlier_alpha=100.0, call=call, strict_training=args.strict_training)

            def blocking(with_filler):
                host = 0.0
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for k in range(K):
                    t1 = time.perf_counter()
                    out = eng.backward_batch(sc, g, ha, gts, 1.0, 100.0, 100.0, params(k * B))
                    host += time.perf_counter() - t1
                    if with_filler:
                        filler()
                torch.cuda.synchronize()
                return time.perf_counter() - t0, host, out

            def asynchronous(with_filler):
                host = 0.0
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for k in range(K):
                    t1 = time.perf_counter()
                    eng.backward_batch_async(sc, g, ha, gt_dev, 1.0, 100.0, 100.0, params(k * B), out=recs[k])
                    host += time.perf_counter() - t1
                    if with_filler:
                        filler()
                torch.cuda.synchronize()
                return time.perf_counter() - t0, host

            out = blocking(True)[2]  # warm-up of both routes and the filler (the workspaces grow here)
            asynchronous(True)
            eng.check()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(K):
                filler()
            torch.cuda.synchronize()
            filler_ms = 1e3 * (time.perf_counter() - t0) / K
            rows = {"a": [], "b": [], "a_host": [], "b_host": [], "a_step": [], "b_step": []}
            for _ in range(args.reps):
                t, h, _ = blocking(False)
                rows["a"].append(t), rows["a_host"].append(h)
                t, h = asynchronous(False)
                rows["b"].append(t), rows["b_host"].append(h)
                rows["a_step"].append(blocking(True)[0])
                rows["b_step"].append(asynchronous(True)[0])
            per_frame = lambda v: 1e3 * np.asarray(v) / (K * B)
            per_step = lambda v: 1e3 * np.asarray(v) / K
            med = lambda v: round(float(np.median(v)), 4)
            spread = lambda v: [round(float(np.min(v)), 4), round(float(np.max(v)), 4)]
            a, b = per_frame(rows["a"]), per_frame(rows["b"])
            line = {"config": name, "B": B, "E": E, "N": cfg["N"], "grid": "%dx%d" % (H, W), "steps": K, "reps": args.reps,
                    "slots_per_frame": round(float(out[:, 1].mean()), 2), "strict_training": args.strict_training,
                    "blocking_ms_per_frame": med(a), "blocking_spread": spread(a),
                    "async_ms_per_frame": med(b), "async_spread": spread(b),
                    "async_over_blocking": round(float(np.median(b) / np.median(a)), 4),
                    "blocking_host_ms_per_call": med(per_step(rows["a_host"])), "async_host_ms_per_call": med(per_step(rows["b_host"])),
                    "filler_ms": round(filler_ms, 4),
                    "blocking_step_ms": med(per_step(rows["a_step"])), "blocking_step_spread": spread(per_step(rows["a_step"])),
                    "async_step_ms": med(per_step(rows["b_step"])), "async_step_spread": spread(per_step(rows["b_step"]))}
            line["step_ms_saved"] = round(line["blocking_step_ms"] - line["async_step_ms"], 4)
            print(json.dumps(line), flush=True)


def main_pose_records(args):
    """--pose-records: what arming a training call costs, and what it saves a loop that logs poses.  Per (config, B), interleaved rep
    by rep after a warm-up of all legs, K = --steps calls per timed run:
      (u) unarmed: B = 1 `backward_device`, else `backward_batch` (blocking) -- and `backward_batch_async`, enqueued back to back;
      (a) the same calls armed (device record tensors): one more small launch per chunk;
      (f) unarmed + one blocking `forward_device` per frame at the same counter: what a training loop pays today for the pose.
    One JSON line each: ms per frame of every leg (medians over --reps with min..max), armed - unarmed, and (f) - (a)."""
    eng = api.Engine(0)
    batches = [int(x) for x in (args.batches if args.batches != "1,8,32,128" else "1,8,32").split(",")]
    K = args.steps
    for name in args.configs.split(","):
        cfg = CONFIGS[name]
        f0, sc_all, ha_all, gts_all, _ = make_inputs(cfg, max(batches))
        E, _, H, W = f0["coords"].shape
        grads = torch.zeros((max(batches), E, 3, H, W), dtype=torch.float32, device="cuda")
        gt_dev_all = torch.from_numpy(gts_all).cuda()
        for B in batches:
            sc, ha, gts, gt_dev, g = sc_all[:B], ha_all[:B], gts_all[:B], gt_dev_all[:B], grads[:B]
            recs = torch.zeros((B, api.RES_DOUBLES), dtype=torch.float64, device="cuda")
            out4 = torch.empty((B, 4), dtype=torch.float64, device="cuda")

            def params(call, **kw):
                return eng.make_params(E, H, W, cfg["N"], focal=f0["focal"], ppx=f0["ppx"], ppy=f0["ppy"], sub_sampling=f0["sub"],
                                       inlier_alpha=100.0, call=call, **kw)

            def blocking(armed, forward=False):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for k in range(K):
                    if B == 1:
                        out = eng.backward_device(sc[0], g[0], ha[0], gts[0], 1.0, 100.0, 100.0, params(k),
                                                  pose_record=recs[0] if armed else None)[None]
                    else:
                        out = eng.backward_batch(sc, g, ha, gts, 1.0, 100.0, 100.0, params(k * B), pose_records=recs if armed else None)
                    if forward:
                        for b in range(B):
                            eng.forward_device(sc[b], ha[b], params(k * B + b, exact_scores="auto"))
                torch.cuda.synchronize()
                return time.perf_counter() - t0, out

            def asynchronous(armed):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for k in range(K):
                    eng.arm_pose_records(recs if armed else None)
                    eng.backward_batch_async(sc, g, ha, gt_dev, 1.0, 100.0, 100.0, params(k * B), out=out4)
                torch.cuda.synchronize()
                return time.perf_counter() - t0

            out = blocking(True, forward=True)[1]  # warm-up of every leg (the workspaces grow here)
            blocking(False)
            asynchronous(True)
            asynchronous(False)
            eng.check()
            assert float(recs[:, api.RES_VALID].min()) == 1.0, "a frame's winner held no slot: the armed legs would time the no-slot record"
            rows = {"u": [], "a": [], "f": [], "u_async": [], "a_async": []}
            for _ in range(args.reps):
                rows["u"].append(blocking(False)[0])
                rows["a"].append(blocking(True)[0])
                rows["f"].append(blocking(False, forward=True)[0])
                rows["u_async"].append(asynchronous(False))
                rows["a_async"].append(asynchronous(True))
            ms = {k: 1e3 * np.asarray(v) / (K * B) for k, v in rows.items()}
            med = lambda v: round(float(np.median(v)), 4)
            spread = lambda v: [round(float(np.min(v)), 4), round(float(np.max(v)), 4)]
            line = {"config": name, "B": B, "E": E, "N": cfg["N"], "grid": "%dx%d" % (H, W), "steps": K, "reps": args.reps,
                    "slots_per_frame": round(float(out[:, 1].mean()), 2), "route": "backward_device" if B == 1 else "backward_batch"}
            for key, label in (("u", "unarmed"), ("a", "armed"), ("f", "unarmed_plus_forward"), ("u_async", "async_unarmed"),
                               ("a_async", "async_armed")):
                line[label + "_ms_per_frame"] = med(ms[key])
                line[label + "_spread"] = spread(ms[key])
            line["arming_costs_ms_per_frame"] = round(line["armed_ms_per_frame"] - line["unarmed_ms_per_frame"], 4)
            line["async_arming_costs_ms_per_frame"] = round(line["async_armed_ms_per_frame"] - line["async_unarmed_ms_per_frame"], 4)
            line["saved_against_a_forward_per_frame_ms"] = round(line["unarmed_plus_forward_ms_per_frame"] - line["armed_ms_per_frame"], 4)
            print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--asynchronous", action="store_true",
                    help="Engine.backward_batch_async against the blocking batch: time per frame, host time in the call, step overlap")
    ap.add_argument("--steps", type=int, default=4, help="--asynchronous: batches per timed run (K)")
    ap.add_argument("--filler-matmuls", type=int, default=4, help="--asynchronous: fp32 4096^3 products behind each call in the step leg")
    ap.add_argument("--batches", default="1,8,32,128")
    ap.add_argument("--configs", default="cfg2,cfg3")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only-batch", type=int, default=0, help="time the batched call only, at this B")
    ap.add_argument("--per-frame-cams", action="store_true",
                    help="also time every (config, B) with a shift and a focal length per frame (one more JSON line, cams=per-frame)")
    ap.add_argument("--strict-training", action="store_true",
                    help="every call with ESAC_FLAG_STRICT_TRAINING (the verification route: each JSON line says strict_training=true)")
    ap.add_argument("--pose-records", action="store_true",
                    help="training calls armed with pose records against unarmed ones, and against unarmed + a blocking forward per frame")
    args = ap.parse_args()
    if args.pose_records:
        return main_pose_records(args)
    if args.asynchronous:
        return main_async(args)
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
