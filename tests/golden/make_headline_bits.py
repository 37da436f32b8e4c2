#!/usr/bin/env python
"""Generates tests/golden/headline_bits/headline_bits.npz (a folder of its own: tests/test_golden.py takes every *.npz beside this
script for an oracle fixture): the device outputs of the cases in tests/headline_bits_cases.py, from the library the
kernels of the headline call are to stay bit-compatible with.  Needs an MI355X.  Run it with the library of the commit BEFORE a
change that must not move a bit (ESAC_HIP_LIB=<that build's libesac_hip.so>), then run tests/test_gpu_headline_bits.py on the
new tree:

    ESAC_HIP_LIB=/path/to/parent/libesac_hip.so python tests/golden/make_headline_bits.py [out.npz]

Re-run only after an INTENDED change of the arithmetic; the fixture is small data (integers and float64 bit patterns)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
from esac_amd import api  # noqa: E402
from tests import headline_bits_cases as H  # noqa: E402


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "headline_bits", "headline_bits.npz")
    eng = api.engine(0)
    out = {}
    for case in H.CASES:
        first = H.run_device(eng, case)
        again = H.run_device(eng, case)  # what a second call does not reproduce cannot be pinned
        for name in list(H.BUFFERS) + ["record"]:
            if not np.array_equal(H.bits(first[name]), H.bits(again[name])):
                raise SystemExit("%s/%s differs between two calls of the same library" % (case, name))
            out["%s/%s" % (case, name)] = H.bits(first[name])
        print(case, first["refine_info"]["mode"], first["refine_info"]["workgroups"], "steps", int(first["record"][api.RES_REF_STEPS]))
    np.savez_compressed(out_path, **out)
    print("wrote", out_path, os.path.getsize(out_path), "bytes")


if __name__ == "__main__":
    main()
