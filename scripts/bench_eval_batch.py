"""The test loop in batches against the loop of single calls, in one process (bench.py stays the headline measurement).

`harness.evaluate` over synthetic experts (the pattern of tests/test_harness.py: an expert returns the ray-cast map of the frame,
looked up on the device by the frame number the image carries), 60x80 maps, 256 hypotheses: batch_size 1 -- the loop of blocking
`esac.forward` calls, a `.cpu()` of the activity flags and numpy Rodrigues per image, i.e. `evaluate` as it was before batches
existed -- against batch_size 8 and 32, blocking and asynchronous.  One JSON line per setting: images/s (median over --reps passes
after a warm-up pass), the ratio to batch_size 1, and the host synchronisations per image (counted: every `.cpu()` of a device
tensor and every blocking single forward call).

    python scripts/bench_eval_batch.py [--images 96] [--experts 4] [--batches 1,8,32] [--reps 5]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from esac_amd import api, harness  # noqa: E402
from esac_amd import synthetic as S  # noqa: E402


class _Expert(torch.nn.Module):
    def __init__(self, maps, e):
        super().__init__()
        self.maps, self.e = maps, e

    def forward(self, images):
        return self.maps[images[:, 0, 0, 0].long(), self.e]


class _Gating(torch.nn.Module):
    def __init__(self, log_gating):
        super().__init__()
        self.log_gating = log_gating

    def forward(self, images):
        return self.log_gating[images[:, 0, 0, 0].long()]


class SyncCounter:
    """Counts what makes the host wait for the device inside the loop: Tensor.cpu() of a device tensor, blocking single calls."""
    def __init__(self):
        self.count = 0

    def __enter__(self):
        self._cpu, self._fwd = torch.Tensor.cpu, api.Engine.forward_device
        counter = self

        def cpu(t, *a, **k):
            counter.count += int(t.is_cuda)
            return counter._cpu(t, *a, **k)

        def forward_device(eng, *a, **k):
            counter.count += int(k.get("want_host", True))
            return counter._fwd(eng, *a, **k)

        torch.Tensor.cpu, api.Engine.forward_device = cpu, forward_device
        return self

    def __exit__(self, *exc):
        torch.Tensor.cpu, api.Engine.forward_device = self._cpu, self._fwd


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=96)
    ap.add_argument("--experts", type=int, default=4)
    ap.add_argument("--hypotheses", type=int, default=256)
    ap.add_argument("--batches", default="1,8,32")
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    E, distinct = args.experts, min(args.images, 32)
    frames = [S.make_frame(900 + k, E=E, true_expert=k % E) for k in range(distinct)]
    maps = torch.from_numpy(np.stack([f["coords"] for f in frames])).cuda()
    logits = torch.full((distinct, E), -4.0, device="cuda")
    for k in range(distinct):
        logits[k, k % E] = 4.0
    gating = _Gating(torch.log_softmax(logits, dim=1))
    experts = [_Expert(maps, e) for e in range(E)]
    images = [torch.full((1, 3, 480, 640), float(k % distinct), device="cuda") for k in range(args.images)]
    samples = [("img%05d" % k, images[k], frames[k % distinct]["focal"], frames[k % distinct]["gt_pose"], (k % distinct) % E)
               for k in range(args.images)]

    def one_pass(batch_size, asynchronous):
        api.set_seed(1305, 0)
        gen = torch.Generator(device="cuda").manual_seed(1)
        torch.cuda.synchronize()
        with SyncCounter() as syncs:
            t0 = time.perf_counter()
            out = harness.evaluate(iter(samples), gating, experts, hypotheses=args.hypotheses, generator=gen, batch_size=batch_size,
                                   asynchronous=asynchronous)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
        return dt, syncs.count, out

    base = None
    for bs in [int(v) for v in args.batches.split(",")]:
        for asynchronous in ((False,) if bs == 1 else (False, True)):
            one_pass(bs, asynchronous)  # warm-up: workspaces, the caching allocator
            runs = [one_pass(bs, asynchronous) for _ in range(args.reps)]
            dt = float(np.median([r[0] for r in runs]))
            out = runs[-1][2]
            rate = args.images / dt
            if bs == 1:
                base = rate
            print(json.dumps({"bench": "eval_batch", "batch_size": bs, "asynchronous": asynchronous, "images": args.images, "experts": E,
                              "hypotheses": args.hypotheses, "grid": "60x80", "images_per_s": round(rate, 1),
                              "vs_batch_size_1": round(rate / base, 2) if base else None,
                              "host_syncs_per_image": round(runs[-1][1] / args.images, 3), "reps": args.reps,
                              "pose_acc": round(float(np.mean([r["pose_acc"] for r in out["scenes"]])), 3),
                              "class_acc": round(float(np.mean([r["class_acc"] for r in out["scenes"]])), 3)}), flush=True)


if __name__ == "__main__":
    main()
