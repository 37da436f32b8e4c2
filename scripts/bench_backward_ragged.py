"""Ragged TRAINING batches -- frames that differ in image size, esac_hip_backward_batch_shapes -- against the two ways such frames
could be trained on before they existed, and the existing shared-shape calls by themselves (for an A/B against another build of
the library: ESAC_HIP_LIB), in one process (bench.py stays the headline measurement).

Device-resident inputs, the same frames and RNG keys in every setting; one JSON line per setting: frames/s as the median over
--reps timed passes (each --iters calls, after a warm-up pass) with the lowest and the highest pass.
  --part shared   `Engine.backward_batch` and `Engine.backward_batch_async` at B = 32 on cfg2's shape (1 expert x 256 hypotheses)
                  and on 10 experts x 1024 hypotheses, 60x80 -- calls this change leaves as they were: run it against two builds
                  alternately and compare the medians with either build's own spread.  Needs none of the new entry points.
  --part mixed    B = 32, a third each of 60x80, 80x60 and 60x90:
                    ragged   ONE `Engine.backward_batch_shapes` over the packed frames;
                    grouped  the same frames grouped by shape into three `Engine.backward_batch` calls (per-frame cameras);
                    single   the same frames as B blocking `Engine.backward_device` calls.

    python scripts/bench_backward_ragged.py [--part shared|mixed|both] [--frames 32] [--experts 10] [--hypotheses 1024] [--reps 7] [--iters 3]
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

GRIDS = [(60, 80), (80, 60), (60, 90)]
LOSS = (1.0, 100.0, 100.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=["shared", "mixed", "both"], default="both")
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--experts", type=int, default=10)
    ap.add_argument("--hypotheses", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--label", default="")
    args = ap.parse_args()
    B = args.frames
    eng = api.engine(0)

    def make(shapes, E, N, first):
        frames = [S.make_frame(first + b, E=E, true_expert=b % E, H=h, W=w, ppx=w * 4.0, ppy=h * 4.0, focal=525.0 + 5.0 * (b % 7))
                  for b, (h, w) in enumerate(shapes)]
        has = torch.from_numpy(np.stack([S.gating_assignment(f, N, mode="gating" if E > 1 else "single") for f in frames])).cuda()
        maps = [torch.from_numpy(f["coords"]).cuda() for f in frames]
        gts = np.stack([np.asarray(f["gt_pose"], np.float32) for f in frames])
        cams = api.make_cams([0] * len(frames), [0] * len(frames), [f["focal"] for f in frames], [f["ppx"] for f in frames],
                             [f["ppy"] for f in frames])
        return frames, has, maps, gts, cams

    def timed(call):
        call()  # warm-up: workspaces (and the rerun after a first slot overflow), the caching allocator
        torch.cuda.synchronize()
        rates = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            for _ in range(args.iters):
                call()
            torch.cuda.synchronize()
            rates.append(B * args.iters / (time.perf_counter() - t0))
        return float(np.median(rates)), float(min(rates)), float(max(rates))

    def report(setting, E, N, grids, rate, versus=None):
        line = {"bench": "backward_ragged", "label": args.label, "setting": setting, "frames": B, "experts": E, "hypotheses": N, "grids": grids,
                "frames_per_s": round(rate[0], 1), "lowest": round(rate[1], 1), "highest": round(rate[2], 1), "reps": args.reps,
                "iters": args.iters}
        if versus:
            line["vs_" + versus[0]] = round(rate[0] / versus[1][0], 3)
        print(json.dumps(line), flush=True)
        return rate

    if args.part in ("shared", "both"):
        for name, E, N in (("cfg2", 1, 256), ("10x1024", args.experts, args.hypotheses)):
            frames, has, maps, gts, cams = make([(60, 80)] * B, E, N, 900)
            sc = torch.stack(maps)
            grads = torch.zeros_like(sc)
            gt_dev = torch.from_numpy(gts).cuda()
            rec = torch.empty((B, 4), dtype=torch.float64, device="cuda")

            def blocking():
                return eng.backward_batch(sc, grads, has, gts, *LOSS, eng.make_params(E, 60, 80, N, seed=1305, call=0), cams=cams)

            def asynchronous():
                return eng.backward_batch_async(sc, grads, has, gt_dev, *LOSS, eng.make_params(E, 60, 80, N, seed=1305, call=0), cams=cams, out=rec)

            for k in range(2):  # (twice: a drift of the machine shows as a difference between the two passes of one setting)
                report("backward_batch_%s_pass%d" % (name, k), E, N, "60x80", timed(blocking))
                report("backward_batch_async_%s_pass%d" % (name, k), E, N, "60x80", timed(asynchronous))

    if args.part in ("mixed", "both"):
        E, N = args.experts, args.hypotheses
        shapes = [GRIDS[b % 3] for b in range(B)]
        frames, has, maps, gts, cams = make(shapes, E, N, 900)
        packed, _ = api.pack_frames(maps, device=eng.device)
        packed_grads = torch.zeros_like(packed)
        H, W = api.capacity_shape(shapes)
        dense_grads = [torch.zeros_like(m) for m in maps]

        def ragged():
            return eng.backward_batch_shapes(packed, packed_grads, has, gts, *LOSS, eng.make_params(E, H, W, N, seed=1305, call=0), shapes, cams=cams)

        def single():
            out = []
            for b, f in enumerate(frames):
                h, w = shapes[b]
                p = eng.make_params(E, h, w, N, focal=f["focal"], ppx=f["ppx"], ppy=f["ppy"], seed=1305, call=b)
                out.append(eng.backward_device(maps[b], dense_grads[b], has[b], gts[b], *LOSS, p))
            return np.stack(out)

        groups = [[b for b in range(B) if shapes[b] == g] for g in GRIDS]
        stacked = [(torch.stack([maps[b] for b in members]), has[members].contiguous(), gts[members], cams[members], members)
                   for members in groups if members]
        stacked = [s + (torch.zeros_like(s[0]),) for s in stacked]

        def grouped():
            # (a group's frames keep their own RNG keys only when they are consecutive; here the keys differ from `ragged`, the work does not)
            out = np.zeros((B, 4))
            for sc, ha, gt, cm, members, g in stacked:
                h, w = shapes[members[0]]
                out[members] = eng.backward_batch(sc, g, ha, gt, *LOSS, eng.make_params(E, h, w, N, seed=1305, call=members[0]), cams=cm)
            return out

        a, s = ragged(), single()
        same = int((a[:, 1] == s[:, 1]).sum())
        r_ragged = report("ragged", E, N, "60x80,80x60,60x90", timed(ragged))
        report("grouped_by_shape", E, N, "60x80,80x60,60x90", timed(grouped), ("ragged", r_ragged))
        report("single_calls", E, N, "60x80,80x60,60x90", timed(single), ("ragged", r_ragged))
        # (the single calls of a default context refine few slots by teams: their losses equal the batch's to rounding, not in bits)
        print(json.dumps({"bench": "backward_ragged", "check": "slot counts of the ragged batch equal to the single calls'", "frames": same,
                          "of": B, "losses_equal": int((a[:, 0] == s[:, 0]).sum())}), flush=True)


if __name__ == "__main__":
    main()
