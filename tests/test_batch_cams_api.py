"""CPU checks of the per-frame camera of the batched entry points (esac_hip_forward_batch_cams /
esac_hip_backward_batch_cams, `cams=` of the Engine calls, sequence arguments of esac.forward_batch / esac.backward_batch):
the symbols are declared and exported, the ABI is unchanged, the ctypes record is the header's, and every argument error is
raised before a device is touched."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from esac_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    with open(os.path.join(ROOT, "include", "esac_hip.h")) as fh:
        return fh.read()


def test_cams_entry_points_are_part_of_the_abi():
    text = _header()
    for name in ("esac_hip_forward_batch_cams", "esac_hip_backward_batch_cams"):
        assert name in api.ABI_SYMBOLS
        assert re.search(r"\bint %s\(esac_hip_ctx\* ctx, int B," % name, text), name
    assert "const esac_hip_frame_cam* h_cams" in text
    assert api.ABI_VERSION == 6
    assert "#define ESAC_HIP_ABI_VERSION 6" in text
    assert C.sizeof(api.Params) == 104


def test_library_exports_the_cams_entry_points():
    lib = api.load_library()
    assert lib.esac_hip_abi_version() == 6
    for name in ("esac_hip_forward_batch_cams", "esac_hip_backward_batch_cams", "esac_hip_forward_batch", "esac_hip_backward_batch"):
        getattr(lib, name)


def test_frame_cam_record_is_the_headers():
    """32 bytes, the five fields in the header's order and at its offsets (4-byte members, no implicit padding)."""
    text = _header()
    m = re.search(r"typedef struct esac_hip_frame_cam \{(.*?)\} esac_hip_frame_cam;", text, re.S)
    assert m
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields, size = [], 0
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ctype, names = decl.split(None, 1)
        assert ctype in ("int32_t", "float"), decl
        for n in names.split(","):
            n = n.strip()
            arr = re.match(r"(\w+)\[(\d+)\]", n)
            count = int(arr.group(2)) if arr else 1
            fields.append((arr.group(1) if arr else n, ctype, size))
            size += 4 * count
    assert size == 32 == C.sizeof(api.FrameCam) == api.CAM_DTYPE.itemsize
    assert [f[0] for f in fields[:5]] == ["shift_x", "shift_y", "focal", "ppx", "ppy"]
    for name, ctype, offset in fields:
        assert getattr(api.FrameCam, name).offset == offset, name
        assert api.CAM_DTYPE.fields[name][1] == offset, name
    for name, ctype, _ in fields[:5]:
        assert api.CAM_DTYPE.fields[name][0] == (np.int32 if ctype == "int32_t" else np.float32)


def test_make_cams_fills_the_records():
    cams = api.make_cams([0, 4, -3], [0, -4, 2], [525.0, 585.0, 480.0], [320.0] * 3, [240.0, 241.5, 239.0])
    assert cams.dtype == api.CAM_DTYPE and cams.shape == (3,)
    raw = np.frombuffer(cams.tobytes(), np.int32).reshape(3, 8)
    np.testing.assert_array_equal(raw[:, 0], [0, 4, -3])
    np.testing.assert_array_equal(raw[:, 1], [0, -4, 2])
    np.testing.assert_array_equal(raw[:, 2].view(np.float32), np.float32([525.0, 585.0, 480.0]))
    np.testing.assert_array_equal(raw[:, 4].view(np.float32), np.float32([240.0, 241.5, 239.0]))
    np.testing.assert_array_equal(raw[:, 5:], 0)
    rec = api.FrameCam.from_buffer_copy(cams[1].tobytes())
    assert (rec.shift_x, rec.shift_y, rec.focal, rec.ppx, rec.ppy) == (4, -4, 585.0, 320.0, 241.5)


def test_all_scalar_arguments_build_no_table():
    scalars, cams = api._per_frame_cams("esac.backward_batch", 3, 1, -2, 525.0, 320.0, 240.0)
    assert cams is None and scalars == (1, -2, 525.0, 320.0, 240.0)
    # zero-dimensional tensors / numpy scalars are scalars too
    scalars, cams = api._per_frame_cams("esac.forward_batch", 3, torch.tensor(1), np.int64(-2), np.float32(525.0), 320.0, 240.0)
    assert cams is None


def test_scalars_are_broadcast_when_one_argument_is_per_frame():
    scalars, cams = api._per_frame_cams("esac.backward_batch", 3, [1, 0, -4], 2, torch.tensor([525.0, 585.0, 1050.0]), 320.0,
                                        np.array([240.0, 239.0, 238.0], np.float32))
    assert scalars == (1, 2, 525.0, 320.0, 240.0)  # frame 0's values stand in the parameter block
    np.testing.assert_array_equal(cams["shift_x"], [1, 0, -4])
    np.testing.assert_array_equal(cams["shift_y"], [2, 2, 2])
    np.testing.assert_array_equal(cams["focal"], np.float32([525.0, 585.0, 1050.0]))
    np.testing.assert_array_equal(cams["ppx"], np.float32([320.0] * 3))
    np.testing.assert_array_equal(cams["ppy"], np.float32([240.0, 239.0, 238.0]))
    # integral shifts may arrive as floats (a tensor of pads)
    _, cams = api._per_frame_cams("esac.backward_batch", 2, torch.tensor([3.0, -1.0]), 0, 525.0, 320.0, 240.0)
    np.testing.assert_array_equal(cams["shift_x"], [3, -1])


def _bwd_args(B=2, E=1, H=12, W=16, N=8):
    sc = torch.zeros(B, E, 3, H, W)
    return [sc, torch.zeros_like(sc), torch.zeros(B, N, dtype=torch.int64), torch.eye(4).repeat(B, 1, 1),
            1.0, 100.0, 100.0, 0, 0, 525.0, 320.0, 240.0, 10.0, 100.0, 0.5, 100.0, 8]


def _fwd_args(B=2, E=1, H=12, W=16, N=8):
    return [torch.zeros(B, E, 3, H, W), torch.zeros(B, N, dtype=torch.int64), torch.zeros(B, 4, 4),
            0, 0, 525.0, 320.0, 240.0, 10.0, 100.0, 0.5, 100.0, 8]


# (offset of the camera argument within the five, bad value, what the message must name)
BAD_CAMS = [
    (0, [0, 1, 2], "shiftX"),                       # wrong length
    (1, torch.tensor([0, 1, 2]), "shiftY"),
    (2, np.array([525.0]), "focalLength"),
    (3, [320.0, 320.0, 320.0], "ppointX"),
    (4, torch.zeros(2, 1), "ppointY"),              # not 1-D
    (0, [0.5, 1], "shiftX"),                        # non-integral shift
    (1, torch.tensor([0.0, 1.25]), "shiftY"),
    (0, [0, 2**31], "shiftX"),                      # beyond int32
    (2, [525.0, float("nan")], "focalLength"),      # non-finite focal length
    (2, [float("inf"), 525.0], "focalLength"),
    (2, [525.0, 0.0], "focalLength"),               # non-positive focal length
    (2, torch.tensor([-525.0, 525.0]), "focalLength"),
    (3, [320.0, float("nan")], "ppointX"),
    (4, np.array([240.0, float("inf")]), "ppointY"),
    (2, ["a", "b"], "focalLength"),
]


@pytest.mark.parametrize("which", ["backward", "forward"])
@pytest.mark.parametrize("offset, value, name", BAD_CAMS)
def test_camera_arguments_are_validated_before_any_device(which, offset, value, name):
    import esac
    args, first, fn = (_bwd_args(), 7, esac.backward_batch) if which == "backward" else (_fwd_args(), 3, esac.forward_batch)
    args[first + offset] = value
    engines = dict(api._state["engines"])
    call = api._state["call"]
    with pytest.raises(RuntimeError, match=name):
        fn(*args)
    assert api._state["engines"] == engines  # no engine was created by the call: nothing reached a device
    assert api._state["call"] == call        # ... and no call counter was spent


def test_engine_rejects_a_table_of_the_wrong_kind_or_length():
    with pytest.raises(RuntimeError, match="cams"):
        api._cams_arg(np.zeros((3, 8), np.int32), 3, "esac.backward_batch")
    with pytest.raises(RuntimeError, match="one record per frame"):
        api._cams_arg(api.make_cams([0, 0], [0, 0], [1.0, 1.0], [0.0, 0.0], [0.0, 0.0]), 3, "esac.backward_batch")
    recs = [api.FrameCam(1, 2, 525.0, 320.0, 240.0), api.FrameCam(-1, 0, 585.0, 321.0, 239.0)]
    arr = api._cams_arg(recs, 2, "esac.forward_batch")
    np.testing.assert_array_equal(arr["shift_x"], [1, -1])
    np.testing.assert_array_equal(arr["focal"], np.float32([525.0, 585.0]))


def test_train_batch_is_exported_by_the_harness():
    import inspect
    from esac_amd import harness
    sig = inspect.signature(harness.train_batch)
    assert list(sig.parameters)[:5] == ["images", "gt_poses", "gating", "experts", "focal_lengths"]
    for name in ("shifts", "e_hyps", "generator"):
        assert sig.parameters[name].default is None
