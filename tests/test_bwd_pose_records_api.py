"""esac_hip_set_bwd_pose_records and the poseRecord(s) arguments of the training calls: the symbol is declared, bound and exported
under ABI version 6, and every argument check raises RuntimeError before a device (or the library's training path) is touched."""
import ctypes as C
import inspect
import os
import re

import pytest
import torch

from esac_amd import api, build, harness

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "esac_hip.h")).read()
ARGS = (0, 0, 525.0, 320.0, 240.0, 10.0, 100.0, 0.5, 100.0, 8)


def test_symbol_is_declared_bound_and_exported_under_abi_6():
    assert re.search(r"\bint esac_hip_set_bwd_pose_records\s*\(\s*esac_hip_ctx\s*\*\s*ctx,\s*double\s*\*\s*d_records,\s*int frames\)", HEADER)
    assert "esac_hip_set_bwd_pose_records" in api.ABI_SYMBOLS
    assert api.ABI_VERSION == 6 and re.search(r"#define\s+ESAC_HIP_ABI_VERSION\s+6\b", HEADER)
    lib = C.CDLL(build.build_hip())
    assert hasattr(lib, "esac_hip_set_bwd_pose_records")
    lib.esac_hip_abi_version.restype = C.c_int
    assert lib.esac_hip_abi_version() == 6
    # a null context is refused without touching a device
    lib.esac_hip_set_bwd_pose_records.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    lib.esac_hip_set_bwd_pose_records.restype = C.c_int
    assert lib.esac_hip_set_bwd_pose_records(None, None, 0) == -1


def test_header_documents_the_contract():
    doc = HEADER[HEADER.index("The winner's refined pose of a training call"):HEADER.index("int esac_hip_set_bwd_pose_records")]
    for phrase in ("One-shot", "NULL disarms", "NO SLOT", "ESAC_RES_VALID", "chunks", "overwrites", "Sharded calls stay rejected"):
        assert phrase in doc, phrase


def test_new_arguments_are_keyword_only_behind_the_reference_list():
    """The batched calls take poseRecords as a keyword behind the reference's positional list.  `esac.backward` keeps the
    reference's parameter list and Engine.backward_batch_async its own (both are pinned): their route is the one-shot arming call,
    set_pose_records / Engine.arm_pose_records, which the other calls honour too."""
    for fn, name in ((api.backward_batch, "poseRecords"), (api.backward_batch_async, "poseRecords")):
        params = inspect.signature(fn).parameters
        assert params[name].kind is inspect.Parameter.KEYWORD_ONLY and params[name].default is None
        assert [p for p in params.values() if p.kind is inspect.Parameter.KEYWORD_ONLY] == [params[name]]
        assert list(params)[-2] == "subSampling"
    assert list(inspect.signature(api.backward).parameters)[-1] == "subSampling"
    assert list(inspect.signature(api.set_pose_records).parameters) == ["records"]
    assert list(inspect.signature(api.Engine.arm_pose_records).parameters) == ["self", "records"]
    assert inspect.signature(api.Engine.backward_device).parameters["pose_record"].default is None
    assert inspect.signature(api.Engine.backward_batch).parameters["pose_records"].default is None
    for fn, names in ((harness.train_step, ("evaluate", "gt_expert")), (harness.train_batch, ("evaluate", "gt_experts"))):
        params = inspect.signature(fn).parameters
        assert params[names[0]].default is False and params[names[1]].default is None
    import esac
    assert esac.backward is api.backward and esac.backward_batch_async is api.backward_batch_async
    assert esac.set_pose_records is api.set_pose_records


def _single():
    sc = torch.zeros(1, 3, 6, 8)
    return sc, torch.zeros_like(sc), torch.zeros(4, dtype=torch.int64), torch.eye(4)


def _batch(B=2):
    sc = torch.zeros(B, 1, 3, 6, 8)
    return sc, torch.zeros_like(sc), torch.zeros(B, 4, dtype=torch.int64), torch.eye(4).repeat(B, 1, 1)


BAD_SINGLE = [
    ("must be a torch.Tensor", [0.0] * 32),
    ("expected scalar type torch.float64 for", torch.zeros(32)),
    (r"must be \[32\]", torch.zeros(31, dtype=torch.float64)),
    (r"must be \[32\]", torch.zeros(1, 32, dtype=torch.float64)),
    ("a CPU or a GPU tensor is required", torch.zeros(32, dtype=torch.float64, device="meta")),
]


@pytest.mark.parametrize("message,record", BAD_SINGLE)
def test_backward_refuses_a_bad_pose_record_before_the_library(message, record):
    calls = api._state["call"]
    with pytest.raises(RuntimeError, match=message):
        api.set_pose_records(record)  # (what the setter can judge it refuses itself, the rest the call does)
        api.backward(*_single(), 1.0, 100.0, 100.0, *ARGS)
    assert api._state["call"] == calls  # refused before the call counter moved: nothing ran
    assert api._state["pose_records"] is None  # one-shot: a refused call has consumed the arming


BAD_BATCH = [
    ("must be a torch.Tensor", [[0.0] * 32] * 2),
    ("expected scalar type torch.float64 for", torch.zeros(2, 32)),
    (r"must be \[2, 32\]", torch.zeros(32, dtype=torch.float64)),
    (r"must be \[2, 32\]", torch.zeros(3, 32, dtype=torch.float64)),
    (r"must be \[2, 32\]", torch.zeros(2, 16, dtype=torch.float64)),
    ("a CPU or a GPU tensor is required", torch.zeros(2, 32, dtype=torch.float64, device="meta")),
]


@pytest.mark.parametrize("message,records", BAD_BATCH)
@pytest.mark.parametrize("fn", [api.backward_batch, api.backward_batch_async])
def test_batched_calls_refuse_bad_pose_records_before_the_library(fn, message, records):
    calls = api._state["call"]
    with pytest.raises(RuntimeError, match=message):
        fn(*_batch(), 1.0, 100.0, 100.0, *ARGS, poseRecords=records)
    assert api._state["call"] == calls
    # the arming call is the same argument by another route
    with pytest.raises(RuntimeError, match=message):
        api.set_pose_records(records)
        fn(*_batch(), 1.0, 100.0, 100.0, *ARGS)
    assert api._state["call"] == calls and api._state["pose_records"] is None


def test_arming_is_one_shot_and_none_disarms():
    t = torch.zeros(2, 32, dtype=torch.float64)
    api.set_pose_records(t)
    assert api._take_pose_records(None) is t and api._take_pose_records(None) is None
    api.set_pose_records(t)
    other = torch.zeros(2, 32, dtype=torch.float64)
    assert api._take_pose_records(other) is other and api._take_pose_records(None) is None  # the call's own argument wins, both are spent
    api.set_pose_records(t)
    api.set_pose_records(None)
    assert api._take_pose_records(None) is None


def test_asynchronous_call_needs_a_device_tensor():
    """A CPU record tensor is what the blocking calls take; the asynchronous one cannot copy back."""
    with pytest.raises(RuntimeError, match="poseRecords must be a device tensor"):
        api.backward_batch_async(*_batch(), 1.0, 100.0, 100.0, *ARGS, poseRecords=torch.zeros(2, 32, dtype=torch.float64))
    # the helper both layers share: a strided device tensor, a tensor on another device than the call's
    api._check_pose_records("w", "poseRecords", torch.zeros(2, 32, dtype=torch.float64), 2, False)            # CPU, blocking: fine
    api._check_pose_records("w", "poseRecord", torch.zeros(64, dtype=torch.float64)[::2], None, False)        # CPU, strided: fine
    with pytest.raises(RuntimeError, match="must be a device tensor"):
        api._check_pose_records("w", "poseRecord", torch.zeros(32, dtype=torch.float64), None, True)


def test_the_check_order_names_the_first_wrong_thing():
    """dtype before shape before device, as the other arguments of the module are judged."""
    with pytest.raises(RuntimeError, match="scalar type"):
        api._check_pose_records("w", "poseRecords", torch.zeros(3, 31), 2, True)
    with pytest.raises(RuntimeError, match=r"must be \[2, 32\]"):
        api._check_pose_records("w", "poseRecords", torch.zeros(3, 31, dtype=torch.float64), 2, True)
