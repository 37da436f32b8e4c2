"""Regenerates tests/golden/verify/verify_ref50.npz: the normal-matrix sums A and the residual sums SSE of every pose of every frozen
frame of tests/verify_reference.py at 50 digits (mpmath), stored as double-double pairs, and prints the rounding level of the
fp64 numpy reference against them -- the figures behind REF_LEVEL_A / REF_LEVEL_SSE there and in LAB_NOTES.md.

    python -m tests.golden.make_verify_ref50
"""
import numpy as np

from tests import verify_reference as V


def main():
    frames, kinds, A_hi, A_lo, s_hi, s_lo = [], [], [], [], [], []
    worst_a = worst_s = (0.0, "")
    for spec in V.FRAME_SPECS:
        fr = V.frame(spec["name"])
        for kind in V.POSE_KINDS:
            ref = V.reference(fr, kind)
            A, sse = V.reference_sums_50(fr["coords"][fr["experts"][kind]], fr["poses"][kind], fr["cam"], ref["inl"])
            pairs = [V.split_hi_lo(a) for a in A]
            frames.append(spec["name"])
            kinds.append(kind)
            A_hi.append([p[0] for p in pairs])
            A_lo.append([p[1] for p in pairs])
            hi, lo = V.split_hi_lo(sse)
            s_hi.append(hi)
            s_lo.append(lo)
            if ref["n"] > 0:
                g = dict(A_hi=np.array(A_hi[-1]), A_lo=np.array(A_lo[-1]), sse_hi=hi, sse_lo=lo)
                ea, es = V.a_error(ref["A"][V.IU], g), V.sse_error(ref["sse"], g)
                worst_a = max(worst_a, (ea, "%s/%s" % (spec["name"], kind)))
                worst_s = max(worst_s, (es, "%s/%s" % (spec["name"], kind)))
                print("%-9s %-9s n=%4d  A %.3g  SSE %.3g  cond %.3g" % (spec["name"], kind, ref["n"], ea, es, ref["cond"]))
    np.savez_compressed(V.GOLDEN, frame=np.array(frames), kind=np.array(kinds), A_hi=np.array(A_hi), A_lo=np.array(A_lo),
                        sse_hi=np.array(s_hi), sse_lo=np.array(s_lo))
    print("level A   %.3g (%s)" % worst_a)
    print("level SSE %.3g (%s)" % worst_s)


if __name__ == "__main__":
    main()
