"""Builds the TEST-ONLY host probe of the strict training path (strict_training_probe.cpp: bwd_math.hpp's dPNP over the Horn
alignment and the rolled Jacobi pseudo-inverse compiled for the host), with the compiler flags of tests/native/build_strict.py."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "strict_training_probe.cpp")
LIB = os.path.join(HERE, "libstrict_training_probe.so")
CSRC = os.path.join(HERE, "..", "..", "esac_amd", "csrc")


def build(force=False):
    deps = [SRC, os.path.join(CSRC, "pose_math.hpp"), os.path.join(CSRC, "bwd_math.hpp")]
    if force or not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in deps):
        hipcc = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else "hipcc"
        subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC",
                               "-shared", SRC, "-o", LIB])
    return LIB
