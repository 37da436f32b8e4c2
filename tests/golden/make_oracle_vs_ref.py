#!/usr/bin/env python
"""Generates tests/golden/oracle_vs_ref/*.npz, the stored reference runs of tests/test_oracle_vs_ref.py: for every case the
outputs of the reference's own sources (oracle/_ref, built by `make -C oracle ref` where they are available) and the
irand(lo, hi) draws its single-thread mt19937 stream handed out (thread_rand.cpp:68-71) while the oracle replayed it.
The inputs are not stored: the test regenerates them from their seeds and compares their sha256 with the one stored here.
Needs oracle/_ref; re-run only after an intended change:   python tests/golden/make_oracle_vs_ref.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
from oracle import esac_oracle as O  # noqa: E402
from oracle import ref_binding as R  # noqa: E402
from tests import test_oracle_vs_ref as T  # noqa: E402

OUT = os.path.join(HERE, "oracle_vs_ref")


def record_stream(seed, run):
    """Runs `run(irand)` with the oracle on the reference's mt19937 stream and returns the draws it consumed."""
    draws = []
    replay = R.replay_irand(seed)

    def irand(lo, hi):
        v = replay(lo, hi)
        draws.append((lo, hi, v))
        return v
    out = run(irand)
    return out, np.array(draws, np.int32).reshape(-1, 3)


def save(name, inputs, draws, **ref):
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, inputs_sha256=T.inputs_digest(*inputs), draws=draws, **ref)
    print(name, os.path.getsize(path) // 1024, "KiB,", len(draws), "draws")


def staged(ref):
    return {k: ref[k] for k in ("sample_xy", "hyps", "scores", "winner", "expert", "entropy", "refined", "inlier_map", "pose")}


def main():
    assert R.build() is not None, "oracle/_ref could not be built (the reference sources are not available)"
    O.build()
    os.makedirs(OUT, exist_ok=True)
    for case in T.CASES:
        coords, ha, kw = T.forward_case(case)
        ref = R.forward(coords, ha, seed=1305, **kw)
        _, draws = record_stream(1305, lambda ir: O.forward(coords, ha, irand=ir, **kw))
        save("fwd_" + T.case_id(case), (coords, ha), draws, **staged(ref))

    coords, ha = T.budget_case()
    ref = R.forward(coords, ha, seed=77, max_tries=2)
    _, draws = record_stream(77, lambda ir: O.forward(coords, ha, irand=ir, max_tries=2))
    save("budget", (coords, ha), draws, **staged(ref))

    coords, ha = T.esac_forward_case()
    e, pose = R.esac_forward(coords, ha, seed=1305)
    _, draws = record_stream(1305, lambda ir: O.forward(coords, ha, irand=ir))
    save("esac_forward", (coords, ha), draws, expert=np.int32(e), pose=pose)

    for case in T.BWD_CASES:
        coords, g_start, ha, gt, kw = T.backward_case(case)
        g_ref = g_start.copy()
        loss = R.esac_backward(coords, g_ref, ha, gt, seed=1305, **kw)
        _, draws = record_stream(1305, lambda ir: O.backward(coords, g_start.copy(), ha, gt, irand=ir, **kw))
        save("bwd_" + T.case_id(case), (coords, g_start, ha, gt), draws, loss=np.float64(loss), gradients=g_ref)

    for bad in T.NON_FINITE:
        coords, ha, kw = T.non_finite_case(bad)
        ref = R.forward(coords, ha, seed=1305, **kw)
        _, draws = record_stream(1305, lambda ir: O.forward(coords, ha, irand=ir, **kw))
        save("nonfinite_%s" % bad, (coords, ha), draws, **staged(ref))


if __name__ == "__main__":
    main()
