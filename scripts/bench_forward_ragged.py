"""A ragged forward batch -- frames that differ in image size, esac_hip_forward_batch_shapes -- against the two ways such frames
could be solved before it existed, in one process (bench.py stays the headline measurement).

B = 32 frames, 10 experts x 1024 hypotheses, the grids a third each of 60x80, 80x60 and 60x90 (a test set resized by its shorter
edge); device-resident inputs, blocking calls, the same frames and RNG keys in every setting:
  ragged   ONE `Engine.forward_batch(shapes=)` over the packed frames;
  single   the same frames as B blocking `Engine.forward_device` calls;
  grouped  the same frames grouped by shape into three `Engine.forward_batch` calls (per-frame cameras).
And the price of the new entry on frames of ONE size: 32 frames of 60x80 through `forward_batch(shapes=)` against the same frames
through `forward_batch(cams=)` (esac_hip_forward_batch_cams).
One JSON line per setting: frames/s as the median over --reps timed passes (each --iters calls, after a warm-up pass), the lowest
and highest pass, and the ratio of the medians to the setting it is compared with.

    python scripts/bench_forward_ragged.py [--frames 32] [--experts 10] [--hypotheses 1024] [--reps 7] [--iters 5]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--experts", type=int, default=10)
    ap.add_argument("--hypotheses", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=5)
    args = ap.parse_args()
    B, E, N = args.frames, args.experts, args.hypotheses
    eng = api.engine(0)

    def make(shapes, first):
        frames = [S.make_frame(first + b, E=E, true_expert=b % E, H=h, W=w, ppx=w * 4.0, ppy=h * 4.0, focal=525.0 + 5.0 * (b % 7))
                  for b, (h, w) in enumerate(shapes)]
        has = torch.from_numpy(np.stack([S.gating_assignment(f, N, mode="gating") for f in frames])).cuda()
        maps = [torch.from_numpy(f["coords"]).cuda() for f in frames]
        cams = api.make_cams([0] * len(frames), [0] * len(frames), [f["focal"] for f in frames], [f["ppx"] for f in frames],
                             [f["ppy"] for f in frames])
        return frames, has, maps, cams

    def timed(call):
        call()  # warm-up: workspaces, the caching allocator
        torch.cuda.synchronize()
        rates = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            for _ in range(args.iters):
                call()
            torch.cuda.synchronize()
            rates.append(B * args.iters / (time.perf_counter() - t0))
        return float(np.median(rates)), float(min(rates)), float(max(rates))

    def report(setting, grids, rate, versus=None):
        line = {"bench": "forward_ragged", "setting": setting, "frames": B, "experts": E, "hypotheses": N, "grids": grids,
                "frames_per_s": round(rate[0], 1), "lowest": round(rate[1], 1), "highest": round(rate[2], 1), "reps": args.reps,
                "iters": args.iters}
        if versus:
            line["vs_" + versus[0]] = round(rate[0] / versus[1][0], 3)
        print(json.dumps(line), flush=True)
        return rate

    # ---- mixed sizes
    shapes = [GRIDS[b % 3] for b in range(B)]
    frames, has, maps, cams = make(shapes, 900)
    packed, _ = api.pack_frames(maps, device=eng.device)
    H, W = api.capacity_shape(shapes)
    scores = torch.empty(B, N, dtype=torch.float64, device="cuda")

    def ragged():
        return eng.forward_batch(packed, has, eng.make_params(E, H, W, N, seed=1305, call=0), scores_out=scores, cams=cams, shapes=shapes)

    def single():
        out = []
        for b, f in enumerate(frames):
            h, w = shapes[b]
            p = eng.make_params(E, h, w, N, focal=f["focal"], ppx=f["ppx"], ppy=f["ppy"], seed=1305, call=b)
            out.append(eng.forward_device(maps[b], has[b], p, scores_out=scores[b]))
        return np.stack(out)

    groups = [[b for b in range(B) if shapes[b] == g] for g in GRIDS]
    stacked = [(torch.stack([maps[b] for b in members]), has[members].contiguous(), cams[members], members) for members in groups if members]

    def grouped():
        # (a group's frames keep their own RNG keys only when they are consecutive; here the keys differ from `ragged`, the work does not)
        out = np.zeros((B, api.RES_DOUBLES))
        for sc, ha, cm, members in stacked:
            h, w = shapes[members[0]]
            out[members] = eng.forward_batch(sc, ha, eng.make_params(E, h, w, N, seed=1305, call=members[0]), cams=cm)
        return out

    a, s = ragged(), single()
    same = int((a[:, api.RES_HYP] == s[:, api.RES_HYP]).sum())
    r_ragged = report("ragged", "60x80,80x60,60x90", timed(ragged))
    report("single_calls", "60x80,80x60,60x90", timed(single), ("ragged", r_ragged))
    report("grouped_by_shape", "60x80,80x60,60x90", timed(grouped), ("ragged", r_ragged))
    print(json.dumps({"bench": "forward_ragged", "check": "winners of the ragged batch equal to the single calls'", "frames": same, "of": B}), flush=True)

    # ---- one size: the new entry against esac_hip_forward_batch_cams
    uni = [(60, 80)] * B
    frames, has, maps, cams = make(uni, 900)
    packed_u, _ = api.pack_frames(maps, device=eng.device)
    stacked_u = torch.stack(maps)

    def uniform_shapes():
        return eng.forward_batch(packed_u, has, eng.make_params(E, 60, 80, N, seed=1305, call=0), scores_out=scores, cams=cams, shapes=uni)

    def uniform_cams():
        return eng.forward_batch(stacked_u, has, eng.make_params(E, 60, 80, N, seed=1305, call=0), scores_out=scores, cams=cams)

    assert np.array_equal(uniform_shapes(), uniform_cams())
    # interleaved twice: a drift of the machine between two settings shows as a difference between the two passes of one setting
    for k in range(2):
        r_cams = report("uniform_cams_pass%d" % k, "60x80", timed(uniform_cams))
        report("uniform_shapes_pass%d" % k, "60x80", timed(uniform_shapes), ("uniform_cams", r_cams))


if __name__ == "__main__":
    main()
