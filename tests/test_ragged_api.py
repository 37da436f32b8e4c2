"""CPU tests of the ragged-batch front end: `esac.pack_frames`, the `shapes=` keyword of `esac.forward_batch` /
`esac.forward_batch_async` (argument errors name the argument and touch no device), and the new C ABI symbol in the header and in
the ctypes binding.  No GPU."""
import os
import re

import numpy as np
import pytest
import torch

import esac
from esac_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def no_device(monkeypatch):
    """Any attempt to open an engine (the first thing that touches a device) fails the test."""
    def boom(*a, **k):
        raise AssertionError("the call touched the device")
    monkeypatch.setattr(api, "engine", boom)


def _maps(E, shapes, seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(E, 3, h, w, generator=g) for h, w in shapes]


# ---------------------------------------------------------------- pack_frames
@pytest.mark.parametrize("E, shapes, S", [
    (3, [(32, 40), (40, 32), (24, 41), (30, 30)], 11520),   # 3*3*1280, a multiple of 4 already
    (1, [(3, 3), (5, 7)], 108),                             # 3*35 = 105 -> 108
    (1, [(3, 3)], 28),                                      # 27 -> 28
    (2, [(12, 25), (16, 20)], 1920),                        # 3*2*320
    (1, [(5, 5), (3, 7)], 76),                              # 75 -> 76
])
def test_pack_frames_layout_and_rounding(E, shapes, S):
    maps = _maps(E, shapes)
    packed, got = esac.pack_frames(maps, device="cpu")
    assert got == shapes and packed.dtype == torch.float32 and tuple(packed.shape) == (len(shapes), S) and S % 4 == 0
    assert S == api.packed_stride(E, shapes) and S - 3 * E * max(h * w for h, w in shapes) in (0, 1, 2, 3)
    for b, (m, (h, w)) in enumerate(zip(maps, shapes)):
        n = 3 * E * h * w
        assert torch.equal(packed[b, :n].view(E, 3, h, w), m)   # dense [E,3,h,w] at the head of the slot: no row strides
        assert torch.count_nonzero(packed[b, n:]) == 0
    assert api.capacity_shape(shapes) == max(shapes, key=lambda s: s[0] * s[1])


def test_pack_frames_takes_strided_maps():
    m = torch.randn(2, 3, 9, 10)[:, :, ::2, 1::3]  # [2,3,5,3], not contiguous
    packed, shapes = esac.pack_frames([m, torch.zeros(2, 3, 3, 3)], device="cpu")
    assert shapes == [(5, 3), (3, 3)] and torch.equal(packed[0, :90].view(2, 3, 5, 3), m)


@pytest.mark.parametrize("maps, needle", [
    ([torch.zeros(2, 3, 4, 4), torch.zeros(3, 3, 4, 4)], "sceneCoordinates[1] holds 3 experts"),
    ([torch.zeros(2, 3, 4, 4), torch.zeros(2, 3, 4, 4, dtype=torch.float64)], "torch.float32 for sceneCoordinates[1]"),
    ([torch.zeros(2, 3, 4, 4, dtype=torch.float16)], "torch.float32 for sceneCoordinates[0]"),
    ([torch.zeros(3, 4, 4)], "sceneCoordinates[0] must be [E,3,h,w]"),
    ([torch.zeros(1, 2, 3, 4, 4)], "sceneCoordinates[0] must be [E,3,h,w]"),
    ([torch.zeros(2, 4, 4, 4)], "sceneCoordinates[0] must be [E,3,h,w]"),
    ([torch.zeros(1, 3, 2, 9)], "shapes[0] = 2x9 is no legal grid"),
    ([np.zeros((1, 3, 4, 4), np.float32)], "sceneCoordinates[0] must be a torch.Tensor"),
    ([], "non-empty list"),
    (torch.zeros(2, 1, 3, 4, 4), "non-empty list"),
])
def test_pack_frames_errors(no_device, maps, needle):
    with pytest.raises(RuntimeError) as e:
        esac.pack_frames(maps, device="cpu")
    assert "esac.pack_frames" in str(e.value) and needle in str(e.value), str(e.value)


# ---------------------------------------------------------------- forward_batch(shapes=...) argument errors
SHAPES = [(32, 40), (40, 32), (24, 41), (30, 30)]
SOLVER = (0, 0, 525.0, 160.0, 128.0, 10.0, 100.0, 0.5, 100.0, 8)


def _call(fn, sc, ha, shapes, poses=None, experts=None, cam=SOLVER):
    if fn is api.forward_batch:
        return fn(sc, ha, torch.zeros(ha.shape[0], 4, 4) if poses is None else poses, *cam, shapes=shapes, experts=experts)
    return fn(sc, ha, *cam, shapes=shapes, experts=experts)


def _bad_calls():
    ha = torch.zeros(4, 16, dtype=torch.int64)
    maps = _maps(3, SHAPES)
    packed = torch.zeros(4, 11520)
    return [
        ("shapes count", maps, ha, SHAPES[:3], {}, ["shapes must hold one (h, w) pair per frame (4), found 3"]),
        ("shapes type", maps, ha, 7, {}, ["shapes must hold one (h, w) pair per frame (4), found int"]),
        ("shapes entry", maps, ha, SHAPES[:3] + [(30,)], {}, ["shapes[3] must be a pair of integers"]),
        ("shapes fractional", maps, ha, SHAPES[:3] + [(30.5, 30)], {}, ["shapes[3] must be a pair of integers"]),
        ("shapes too small", packed, ha, SHAPES[:3] + [(2, 30)], {}, ["shapes[3] = 2x30 is no legal grid"]),
        ("shapes vs maps", maps, ha, [(32, 40), (32, 40), (24, 41), (30, 30)], {}, ["shapes[1] = 32x40, sceneCoordinates[1] is 40x32"]),
        ("list length", maps[:3], ha, SHAPES, {}, ["sceneCoordinates holds 3 frames, hypAssignment 4"]),
        ("list dtype", maps[:3] + [maps[3].double()], ha, SHAPES, {}, ["torch.float32 for sceneCoordinates[3]"]),
        ("list experts", maps[:3] + [torch.zeros(2, 3, 30, 30)], ha, SHAPES, {}, ["sceneCoordinates[3] holds 2 experts"]),
        ("list rank", maps[:3] + [torch.zeros(3, 30, 30)], ha, SHAPES, {}, ["sceneCoordinates[3] must be [E,3,h,w]"]),
        ("experts vs list", maps, ha, SHAPES, dict(experts=2), ["experts = 2, sceneCoordinates holds 3"]),
        ("experts type", packed, ha, SHAPES, dict(experts=0), ["experts must be a positive int"]),
        ("packed rank", torch.zeros(4, 3, 3, 32, 40), ha, SHAPES, {}, ["sceneCoordinates must be the packed float32 [B,S] tensor"]),
        ("packed dtype", packed.double(), ha, SHAPES, {}, ["sceneCoordinates must be the packed float32 [B,S] tensor"]),
        ("packed batch", torch.zeros(3, 11520), ha, SHAPES, {}, ["batch sizes of sceneCoordinates and hypAssignment differ"]),
        ("packed S % 4", torch.zeros(4, 11522), ha, SHAPES, {}, ["sceneCoordinates [B,S] needs S to be a multiple of 4"]),
        ("packed too short", torch.zeros(4, 3836), ha, SHAPES, {}, ["sceneCoordinates [B,3836] is too short for 1 expert(s)"]),
        ("packed short for experts", packed, ha, SHAPES, dict(experts=4), ["too short for 4 expert(s)"]),
        ("hypAssignment", maps, ha.int(), SHAPES, {}, ["hypAssignment must be"]),
        ("camera", maps, ha, SHAPES, dict(cam=(0, 0, [525.0, 0.0, 525.0, 525.0]) + SOLVER[3:]), ["focalLength must be positive (frame 1"]),
        ("camera length", maps, ha, SHAPES, dict(cam=(0, 0, 525.0, [1.0, 2.0]) + SOLVER[4:]), ["ppointX must be a scalar or hold one value per frame (4)"]),
    ]


@pytest.mark.parametrize("fn", [api.forward_batch, api.forward_batch_async], ids=["blocking", "async"])
@pytest.mark.parametrize("case", _bad_calls(), ids=lambda c: c[0])
def test_shapes_argument_errors_name_the_argument_and_touch_no_device(no_device, fn, case):
    _, sc, ha, shapes, kw, needles = case
    call0 = api._state["call"]
    with pytest.raises(RuntimeError) as e:
        _call(fn, sc, ha, shapes, **kw)
    who = "esac.forward_batch_async" if fn is api.forward_batch_async else "esac.forward_batch"
    assert str(e.value).startswith(who + ":"), str(e.value)
    for n in needles:
        assert n in str(e.value), str(e.value)
    assert api._state["call"] == call0  # a refused call draws no RNG stream


@pytest.mark.parametrize("fn", [api.forward_batch, api.forward_batch_async], ids=["blocking", "async"])
def test_more_frames_than_a_call_takes(no_device, fn):
    B = api.MAX_BATCH + 1
    call0 = api._state["call"]
    with pytest.raises(RuntimeError, match="hypAssignment holds %d frames, at most %d per call" % (B, api.MAX_BATCH)):
        _call(fn, torch.zeros(B, 28), torch.zeros(B, 4, dtype=torch.int64), [(3, 3)] * B)
    assert api._state["call"] == call0


def test_outposes_and_experts_without_shapes(no_device):
    ha = torch.zeros(4, 16, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="outPoses must be float32"):
        _call(api.forward_batch, _maps(3, SHAPES), ha, SHAPES, poses=torch.zeros(3, 4, 4))
    with pytest.raises(RuntimeError, match="experts is an argument of a ragged batch"):
        api.forward_batch(torch.zeros(4, 3, 3, 32, 40), ha, torch.zeros(4, 4, 4), *SOLVER, experts=3)
    with pytest.raises(RuntimeError, match="experts is an argument of a ragged batch"):
        api.forward_batch_async(torch.zeros(4, 3, 3, 32, 40), ha, *SOLVER, experts=3)


def test_backward_batch_has_no_shapes_keyword():
    """The training path is out of scope: no silent acceptance."""
    import inspect
    for fn in (api.backward_batch, api.backward_batch_async, api.Engine.backward_batch, api.Engine.backward_batch_async):
        assert "shapes" not in inspect.signature(fn).parameters
    for fn in (api.forward_batch, api.forward_batch_async, api.Engine.forward_batch):
        assert inspect.signature(fn).parameters["shapes"].default is None


def test_expert_count_follows_from_a_packed_row():
    for E in (1, 2, 3, 10, 50):
        for shapes in ([(3, 3)], SHAPES, [(60, 80), (80, 60), (60, 90)]):
            S = api.packed_stride(E, shapes)
            got, _ = api._ragged_args("t", torch.zeros(len(shapes), S), len(shapes), shapes, None)
            assert got == E


# ---------------------------------------------------------------- the symbol
def test_header_declares_the_symbol_and_the_binding_names_it():
    hdr = open(os.path.join(ROOT, "include", "esac_hip.h")).read()
    m = re.search(r"int esac_hip_forward_batch_shapes\(([^;]*)\);", hdr)
    assert m, "include/esac_hip.h does not declare esac_hip_forward_batch_shapes"
    args = [a.strip() for a in re.sub(r"\s+", " ", m.group(1)).split(",")]
    cams = re.search(r"int esac_hip_forward_batch_cams\(([^;]*)\);", hdr)
    assert args == [a.strip() for a in re.sub(r"\s+", " ", cams.group(1)).split(",")]  # the same eleven parameters
    assert "#define ESAC_HIP_ABI_VERSION 6" in hdr and api.ABI_VERSION == 6
    assert "esac_hip_forward_batch_shapes" in api.ABI_SYMBOLS and len(set(api.ABI_SYMBOLS)) == len(api.ABI_SYMBOLS)
    assert esac.pack_frames is api.pack_frames


def test_library_exports_and_binds_the_symbol():
    from esac_amd import build
    if not os.path.exists(build.LIB_PATH):
        build.build_hip()
    lib = api.load_library()
    fn = lib.esac_hip_forward_batch_shapes
    assert len(fn.argtypes) == 11 and fn.argtypes == lib.esac_hip_forward_batch_cams.argtypes
    # the first check of the entry point needs no device: a null table is refused before anything else
    assert fn(None, 2, None, 0, None, None, None, None, None, None, None) == -1
    assert b"esac_hip_forward_batch_shapes" in lib.esac_hip_last_error() and b"h_cams" in lib.esac_hip_last_error()
    cams = api.make_cams([0], [0], [525.0], [1.0], [1.0])
    assert fn(None, 0, None, 0, None, None, cams.ctypes.data, None, None, None, None) == -4
    assert b"batch size 0" in lib.esac_hip_last_error()
