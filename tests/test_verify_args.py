"""esac_hip_verify_batch without a device: the additive ABI symbol and the VERIFY_* mirror of the header, the argument checks of
esac.verify_batch (RuntimeError naming the argument before any device is touched), and the library's own checks before a launch
(esac_amd/csrc/verify_policy.hpp: plan_verify) through a stand-alone host program under AddressSanitizer and UBSan --
tests/native/verify_policy_probe.cpp, its own process, no GPU."""
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from esac_amd import api, harness
from tests.native import build_verify

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "esac_hip.h")).read()


def test_symbol_is_additive_and_the_version_stays():
    assert re.search(r"\bint esac_hip_verify_batch\s*\(", HEADER)
    assert "esac_hip_verify_batch" in api.ABI_SYMBOLS
    assert api.ABI_VERSION == 6 and re.search(r"#define ESAC_HIP_ABI_VERSION 6\b", HEADER)
    from esac_amd import build
    assert "esac_verify.hip" in build.SOURCES and "verify_math.hpp" in build.HEADERS and "verify_policy.hpp" in build.HEADERS


def test_verify_constants_mirror_the_header():
    def enum(first):
        body = re.search(r"enum \{ (%s.*?)\};" % first, HEADER, flags=re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        return {m.group(1): int(m.group(2)) for m in re.finditer(r"ESAC_VERIFY_(\w+)\s*=\s*(\d+)", body)}
    assert enum("ESAC_VERIFY_SCORE") == {"SCORE": api.VERIFY_SCORE, "N": api.VERIFY_N, "SSE": api.VERIFY_SSE, "SIGMA2": api.VERIFY_SIGMA2,
                                         "STATUS": api.VERIFY_STATUS, "A": api.VERIFY_A, "C": api.VERIFY_C}
    assert enum("ESAC_VERIFY_OK") == {"OK": api.VERIFY_OK, "FEW": api.VERIFY_FEW, "PINV": api.VERIFY_PINV, "BAD_POSE": api.VERIFY_BAD_POSE,
                                      "BAD_EXPERT": api.VERIFY_BAD_EXPERT}
    assert enum("ESAC_VERIFY_POSE_RT") == {"POSE_RT": api.VERIFY_POSE_RT, "POSE_4X4": api.VERIFY_POSE_4X4}
    assert int(re.search(r"#define ESAC_VERIFY_DOUBLES (\d+)", HEADER).group(1)) == api.VERIFY_DOUBLES == 64
    assert int(re.search(r"#define ESAC_VERIFY_MAX_POSES (\d+)", HEADER).group(1)) == api.VERIFY_MAX_POSES == 1024
    # the row: 5 head values + 1 reserved, 21 + 1 reserved, 36
    assert api.VERIFY_A == 6 and api.VERIFY_C == api.VERIFY_A + 22 and api.VERIFY_C + 36 == api.VERIFY_DOUBLES
    import esac
    assert esac.verify_batch is api.verify_batch


def test_signatures():
    assert list(inspect.signature(api.verify_batch).parameters) == [
        "sceneCoordinates", "poses", "experts", "shiftX", "shiftY", "focalLength", "ppointX", "ppointY", "inlierThreshold", "inlierAlpha",
        "inlierBeta", "maxReproj", "subSampling", "shapes", "out"]
    assert list(inspect.signature(api.Engine.verify_batch).parameters) == ["self", "scene_coords", "poses", "experts", "params", "cams", "shapes", "out"]
    assert inspect.signature(harness.localize_batch).parameters["verify_gt"].default is False
    assert inspect.signature(harness.evaluate).parameters["verify_gt"].default is False


CAM = dict(shiftX=0, shiftY=0, focalLength=100.0, ppointX=64.0, ppointY=48.0)
SOLVER = dict(inlierThreshold=10.0, inlierAlpha=100.0, inlierBeta=0.5, maxReproj=100.0, subSampling=8)


def _args():
    return dict(sceneCoordinates=torch.zeros(2, 3, 3, 12, 16), poses=torch.zeros(2, 5, 6, dtype=torch.float64),
                experts=torch.zeros(2, 5, dtype=torch.int64), **CAM, **SOLVER)


ERRORS = {
    "poses_type": (dict(poses=np.zeros((2, 5, 6))), "poses"),
    "poses_rt_dtype": (dict(poses=torch.zeros(2, 5, 6)), "poses"),
    "poses_4x4_dtype": (dict(poses=torch.zeros(2, 5, 4, 4, dtype=torch.float64)), "poses"),
    "poses_shape": (dict(poses=torch.zeros(2, 5, 7, dtype=torch.float64)), "poses"),
    "poses_rank": (dict(poses=torch.zeros(10, 6, dtype=torch.float64)), "poses"),
    "poses_no_frames": (dict(poses=torch.zeros(0, 5, 6, dtype=torch.float64)), "poses"),
    "poses_too_many_frames": (dict(poses=torch.zeros(1025, 1, 6, dtype=torch.float64)), "poses"),
    "poses_no_poses": (dict(poses=torch.zeros(2, 0, 6, dtype=torch.float64)), "poses"),
    "poses_too_many_poses": (dict(poses=torch.zeros(2, 1025, 6, dtype=torch.float64)), "poses"),
    "experts_dtype": (dict(experts=torch.zeros(2, 5, dtype=torch.int16)), "experts"),
    "experts_float": (dict(experts=torch.zeros(2, 5)), "experts"),
    "experts_shape": (dict(experts=torch.zeros(2, 4, dtype=torch.int64)), "experts"),
    "experts_batch": (dict(experts=torch.zeros(3, dtype=torch.int32)), "experts"),
    "experts_list_floats": (dict(experts=[[0.5] * 5] * 2), "experts"),
    "experts_type": (dict(experts="experts"), "experts"),
    "sc_type": (dict(sceneCoordinates=np.zeros((2, 3, 3, 12, 16), np.float32)), "sceneCoordinates"),
    "sc_dtype": (dict(sceneCoordinates=torch.zeros(2, 3, 3, 12, 16, dtype=torch.float64)), "sceneCoordinates"),
    "sc_rank": (dict(sceneCoordinates=torch.zeros(3, 12, 16)), "sceneCoordinates"),
    "sc_chan": (dict(sceneCoordinates=torch.zeros(2, 3, 2, 12, 16)), "sceneCoordinates"),
    "sc_batch": (dict(sceneCoordinates=torch.zeros(3, 3, 3, 12, 16)), "sceneCoordinates"),
    "sc_packed_without_shapes": (dict(sceneCoordinates=torch.zeros(2, 1728)), "sceneCoordinates"),
    "sc_list_without_shapes": (dict(sceneCoordinates=[torch.zeros(3, 3, 12, 16)] * 2), "shapes"),
    "shapes_count": (dict(sceneCoordinates=torch.zeros(2, 1728), shapes=[(12, 16)]), "shapes"),
    "shapes_grid": (dict(sceneCoordinates=torch.zeros(2, 1728), shapes=[(12, 16), (2, 16)]), "shapes"),
    "shapes_with_dense_maps": (dict(shapes=[(12, 16), (12, 16)]), "sceneCoordinates"),
    "shapes_packed_too_short": (dict(sceneCoordinates=torch.zeros(2, 400), shapes=[(12, 16), (12, 16)]), "sceneCoordinates"),
    "out_on_host": (dict(out=torch.zeros(2, 5, 64, dtype=torch.float64)), "out"),
    "out_type": (dict(out=np.zeros((2, 5, 64))), "out"),
    "focal_len": (dict(focalLength=[100.0, 100.0, 100.0]), "focalLength"),
    "focal_sign": (dict(focalLength=[100.0, -1.0]), "focalLength"),
    "shift_frac": (dict(shiftX=[0.5, 0]), "shiftX"),
    "ppoint_nan": (dict(ppointY=[48.0, float("nan")]), "ppointY"),
}


@pytest.mark.parametrize("bad", sorted(ERRORS))
def test_verify_batch_argument_errors_name_the_argument(bad, monkeypatch):
    import esac
    monkeypatch.setattr(api, "engine", lambda *a, **k: pytest.fail("an argument error must be raised before any device is touched"))
    change, name = ERRORS[bad]
    args = _args()
    args.update(change)
    before = esac.get_rng_state()
    with pytest.raises(RuntimeError, match=r"esac\.verify_batch: .*" + name):
        esac.verify_batch(**args)
    assert esac.get_rng_state() == before


def test_accepted_arguments_reach_the_engine(monkeypatch):
    """every accepted form gets as far as the engine (and no further here): both pose formats, both expert forms, shared maps,
    per-frame cameras, a ragged batch"""
    import esac

    class Reached(Exception):
        pass

    def engine(*a, **k):
        raise Reached()
    monkeypatch.setattr(api, "engine", engine)
    forms = [dict(), dict(poses=torch.zeros(2, 5, 4, 4)), dict(experts=torch.zeros(2, dtype=torch.int32)), dict(experts=[[0] * 5] * 2),
             dict(sceneCoordinates=torch.zeros(3, 3, 12, 16)), dict(focalLength=[100.0, 120.0], shiftX=torch.tensor([1, -2])),
             dict(sceneCoordinates=torch.zeros(2, 1836), shapes=[(12, 16), (17, 12)])]
    for form in forms:
        args = _args()
        args.update(form)
        with pytest.raises(Reached):
            esac.verify_batch(**args)


# ---------------------------------------------------------------- the library's checks (plan_verify)
@pytest.fixture(scope="module")
def policy():
    exe = build_verify.build_policy_probe()

    def run(lines):
        out = subprocess.run([exe], input="".join(l + "\n" for l in lines), capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-2000:])
        rows = [l.split("|") for l in out.stdout.splitlines()]
        assert len(rows) == len(lines), out.stdout
        return rows
    return run


def F(h=12, w=16, shift_x=0, shift_y=0, focal=100.0):
    return (shift_x, shift_y, focal, h, w)


def _plan(B=2, K=5, fmt=0, ctx=1, params=1, sc=1, poses=1, experts=1, out=1, ragged=0, table=0, E=3, H=12, W=16, sub=8, stride=1728, flags=0,
          frames=None):
    frames = [F()] * max(B, 0) if frames is None else frames
    assert len(frames) == (B if 0 < B <= 4096 else 0)
    return "plan %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d " % (ctx, params, B, K, sc, poses, fmt, experts, out, ragged, table, E, H, W, sub,
                                                                        stride, flags) + " ".join("%d %d %r %d %d" % f for f in frames)


# (request, status, (stage, shapes, grid of the plan) or None, what the message must contain)
POLICY_CASES = [
    (_plan(), 0, (0, 0, "12x16"), None),
    (_plan(fmt=1, K=1, B=1), 0, (0, 0, "12x16"), None),
    (_plan(B=1024, K=1024, stride=0), 0, (0, 0, "12x16"), None),                       # both upper ends, shared maps
    (_plan(table=1), 0, (1, 0, "12x16"), None),                                         # a camera table of two frames is staged
    (_plan(B=1, table=1, frames=[F(focal=90.0)]), 0, (0, 0, "12x16"), None),            # ... of one frame goes inline
    (_plan(B=3, table=1, ragged=1, H=13, W=17, stride=1992, frames=[F(12, 16), F(16, 12), F(13, 17)]), 0, (1, 1 + 1, "13x17"), None),
    (_plan(B=2, table=1, ragged=1, stride=1728, frames=[F(12, 16), F(8, 24)]), 0, (1, 1, "12x16"), None),    # every width a multiple of 4
    (_plan(B=1, table=1, ragged=1, H=13, W=17, stride=1992, frames=[F(16, 12)]), 0, (0, 0, "16x12"), None),  # one frame: the single call on its grid
    (_plan(flags=256), 0, (0, 0, "12x16"), None),                                       # ESAC_FLAG_STRICT_REFERENCE
    # null context / parameter block
    (_plan(ctx=0), -1, None, ["null context"]),
    (_plan(params=0), -1, None, ["null params"]),
    # what is new here: -4 naming the argument
    (_plan(B=0), -4, None, ["esac_hip_verify_batch", "B = 0 outside [1,1024]"]),
    (_plan(B=-3), -4, None, ["B = -3 outside [1,1024]"]),
    (_plan(B=1025, stride=0), -4, None, ["B = 1025 outside [1,1024]"]),
    (_plan(K=0), -4, None, ["esac_hip_verify_batch", "K = 0 outside [1,1024]"]),
    (_plan(K=1025), -4, None, ["K = 1025 outside [1,1024]"]),
    (_plan(fmt=2), -4, None, ["esac_hip_verify_batch", "pose_format = 2"]),
    (_plan(fmt=-1), -4, None, ["pose_format = -1"]),
    (_plan(sc=0), -4, None, ["esac_hip_verify_batch", "null d_sc pointer"]),
    (_plan(poses=0), -4, None, ["null d_poses pointer"]),
    (_plan(experts=0), -4, None, ["null d_experts pointer"]),
    (_plan(out=0), -4, None, ["null d_out pointer"]),
    (_plan(ragged=1, table=0), -4, None, ["esac_hip_verify_batch", "ragged without a frame table"]),
    (_plan(stride=-4), -4, None, ["negative sc_frame_stride -4"]),
    # the parameter block, with check_args' messages
    (_plan(E=0), -4, None, ["E=0"]),
    (_plan(H=2), -4, None, ["grid 2x16 too small"]),
    (_plan(H=65536, W=3), -4, None, ["grid 65536x3 too large"]),
    (_plan(sub=0), -4, None, ["subSampling=0 must be positive"]),
    (_plan(flags=256 | 2), -4, None, ["ESAC_FLAG_STRICT_REFERENCE cannot be combined"]),
    (_plan(flags=512), -4, None, ["ESAC_FLAG_STRICT_TRAINING is a flag of esac_hip_backward"]),
    # a bad camera: inline, and in a table (the frame is named)
    (_plan(B=1, table=1, frames=[F(focal=0.0)]), -4, None, ["focal length must be positive in frame 0"]),
    (_plan(B=3, table=1, frames=[F(), F(), F(focal=-5.0)]), -4, None, ["focal length must be positive in frame 2"]),
    (_plan(B=2, table=1, frames=[F(), F(shift_x=-(2**31 - 1 - 124) - 1)]), -4, None, ["pixel positions overflow int32", "in frame 1"]),
    # a bad grid of a ragged table, with check_shapes' messages under this entry point's name
    (_plan(B=2, table=1, ragged=1, frames=[F(12, 16), F(2, 16)]), -4, None, ["grid 2x16 too small", "in frame 1"]),
    (_plan(B=2, table=1, ragged=1, frames=[F(12, 16), F(13, 17)]), -4, None, ["esac_hip_verify_batch", "grid 13x17 in frame 1", "221 cells"]),
    (_plan(B=2, table=1, ragged=1, stride=1724, frames=[F(12, 16), F(12, 16)]), -4, None, ["esac_hip_verify_batch", "frame 0", "3*E*h*w = 1728", "sc_frame_stride = 1724"]),
    (_plan(B=2, table=1, ragged=1, stride=1730, frames=[F(12, 16), F(12, 16)]), -4, None, ["sc_frame_stride 1730", "multiple of 4"]),
    (_plan(B=2, table=1, ragged=1, stride=0, frames=[F(12, 16), F(12, 16)]), -4, None, ["exceed its slot", "sc_frame_stride = 0"]),
]


def test_library_checks_refuse_before_a_launch_and_name_the_argument(policy):
    rows = policy([c[0] for c in POLICY_CASES])
    for (req, status, plan, needles), row in zip(POLICY_CASES, rows):
        assert row[0] == "plan" and int(row[1]) == status, (req, row)
        if status == 0:
            assert (int(row[2]), int(row[3]), row[4]) == plan and row[6] == "", (req, row)
            assert int(row[5]) == int(req.split()[4])  # N of the plan is K: the caller's N is never read
        else:
            for n in needles:
                assert n in row[6], (req, n, row)
    assert {c[1] for c in POLICY_CASES} == {0, -1, -4}
