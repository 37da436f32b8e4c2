"""Builds the TEST-ONLY host probe of the training call's pose record (bwd_record_probe.cpp: bwd_record_math.hpp compiled for the
host), with the compiler flags of the existing host probes (tests/native/build.py: build), and its stand-alone program."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "bwd_record_probe.cpp")
LIB = os.path.join(HERE, "libbwd_record_probe.so")
EXE = os.path.join(HERE, "bwd_record_probe")
CSRC = os.path.join(HERE, "..", "..", "esac_amd", "csrc")
DEPS = [SRC] + [os.path.join(CSRC, h) for h in ("bwd_record_math.hpp", "select_math.hpp", "device_common.hpp", "pose_math.hpp")]


def _hipcc():
    return "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else "hipcc"


def _stale(out):
    return not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in DEPS)


def build(force=False):
    if force or _stale(LIB):
        subprocess.check_call([_hipcc(), "--offload-arch=gfx950", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC",
                               "-shared", SRC, "-o", LIB])
    return LIB


def build_program(force=False, sanitize=False):
    """The probe's main(): slot lists and records of its own, walked by a program of its own.  sanitize: a host build with
    -fsanitize=address,undefined (a stand-alone program: run it directly on the CPU, never inside Python)."""
    exe = EXE + ("_san" if sanitize else "")
    if force or _stale(exe):
        extra = ["-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined", "-fno-omit-frame-pointer"] if sanitize else ["-O2"]
        subprocess.check_call([_hipcc(), "--offload-arch=gfx950", "-std=c++17", "-ffp-contract=off", "-DBWD_RECORD_PROBE_MAIN"] + extra +
                              [SRC, "-o", exe])
    return exe
