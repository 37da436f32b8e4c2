"""Builds the TEST-ONLY host programs of the pose verification call: verify_probe (verify_math.hpp compiled for the host with
hipcc, like the other math probes) and verify_policy_probe (verify_policy.hpp: the host compiler alone).  Both are stand-alone
programs driven through stdin / stdout; sanitize=True builds them with -fsanitize=address,undefined (run directly on the CPU,
never inside Python)."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "..", "esac_amd", "csrc")
PROBE_SRC = os.path.join(HERE, "verify_probe.cpp")
POLICY_SRC = os.path.join(HERE, "verify_policy_probe.cpp")
PROBE_DEPS = [PROBE_SRC] + [os.path.join(CSRC, h) for h in ("verify_math.hpp", "eval_math.hpp", "gt_math.hpp", "bwd_math.hpp", "select_math.hpp",
                                                            "device_common.hpp", "pose_math.hpp", "esac_kernels.hpp")]
POLICY_DEPS = [POLICY_SRC, os.path.join(HERE, "..", "..", "include", "esac_hip.h")] + \
    [os.path.join(CSRC, h) for h in ("verify_policy.hpp", "batch_plan.hpp", "ragged_policy.hpp", "call_policy.hpp")]


def _hipcc():
    return "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else "hipcc"


def _stale(out, deps):
    return not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps)


def build_probe(force=False, sanitize=False):
    exe = os.path.join(HERE, "verify_probe" + ("_san" if sanitize else ""))
    if force or _stale(exe, PROBE_DEPS):
        extra = ["-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined", "-fno-omit-frame-pointer"] if sanitize else ["-O2"]
        subprocess.check_call([_hipcc(), "--offload-arch=gfx950", "-std=c++17", "-ffp-contract=off"] + extra + [PROBE_SRC, "-o", exe + ".tmp"])
        os.replace(exe + ".tmp", exe)
    return exe


def build_policy_probe(force=False):
    """always under AddressSanitizer and UBSan, like the other policy probes"""
    exe = os.path.join(HERE, "verify_policy_probe_san")
    if force or _stale(exe, POLICY_DEPS):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=undefined", POLICY_SRC, "-o", exe + ".tmp"])
        os.replace(exe + ".tmp", exe)
    return exe


def hexf(values):
    """numbers -> one line of C99 hex floats (NaN as 'nan')"""
    return " ".join("nan" if v != v else float(v).hex() for v in values)


def run_probe(exe, requests):
    """requests: [(coords_e [3,h,w] float32, cam dict(focal, ppx, ppy, shift), score dict, strict, format, poses array)].
    Returns one float64 [K,64] array of rows and one int [K] array of fetch verdicts per request."""
    import numpy as np
    text = []
    for coords_e, cam, score, strict, fmt, poses in requests:
        _, h, w = coords_e.shape
        K = poses.shape[0]
        text.append("map %d %d %d %d %d %s %d %d %d" % (h, w, score["sub"], cam["shift"][0], cam["shift"][1],
                                                      hexf([cam["focal"], cam["ppx"], cam["ppy"], score["tau"], score["alpha"], score["beta"], score["max_reproj"]]),
                                                      int(strict), fmt, K))
        text.append(hexf(np.asarray(coords_e, np.float32).reshape(-1).tolist()))
        text.append(hexf(np.asarray(poses).reshape(-1).tolist()))
    out = subprocess.run([exe], input="\n".join(text) + "\n", capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-4000:])
    lines = [l.split() for l in out.stdout.splitlines()]
    rows, oks, at = [], [], 0
    for req in requests:
        K = req[5].shape[0]
        blk = lines[at:at + K]
        at += K
        assert len(blk) == K and all(l[0] == "row" and len(l) == 66 for l in blk), out.stdout[-2000:]
        rows.append(np.array([[float("nan") if v.endswith("nan") else float.fromhex(v) for v in l[2:]] for l in blk]))
        oks.append(np.array([int(l[1]) for l in blk]))
    assert at == len(lines), out.stdout[-2000:]
    return rows, oks
