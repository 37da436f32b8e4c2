"""CPU checks of the asynchronous batched training call (esac.backward_batch_async / esac_hip_backward_batch_dev): it is
declared, bound and exported, the ABI version did not move, and every argument error is raised before a device is touched."""
import inspect
import os
import re

import pytest
import torch

from esac_amd import api, harness

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    with open(os.path.join(ROOT, "include", "esac_hip.h")) as fh:
        return fh.read()


def test_backward_batch_dev_is_part_of_the_abi():
    assert "esac_hip_backward_batch_dev" in api.ABI_SYMBOLS
    text = _header()
    assert "int esac_hip_backward_batch_dev(esac_hip_ctx* ctx, int B," in text
    m = re.search(r"int esac_hip_backward_batch_dev\(([^;]*)\);", text)
    assert m and "const float* d_gt_poses" in m.group(1) and "double* d_out" in m.group(1) and "const esac_hip_frame_cam* h_cams" in m.group(1)


def test_the_abi_version_is_still_6():
    assert api.ABI_VERSION == 6
    assert re.search(r"#define\s+ESAC_HIP_ABI_VERSION\s+6\b", _header())


def test_the_call_path_holds_no_host_wait():
    """The one body behind esac_hip_backward_batch_dev and esac_hip_backward_batch_dev_shapes, the prologue it shares with the
    blocking batch, and the helpers on its launch path (the chunk prologue, the sampling prologue, the fill of a.bwd and the
    selection .. accumulation chain, each from its signature to its closing brace): no stream synchronisation, no blocking copy,
    no polling of a pinned record, and no second pass.  The accumulation is launched from one place in the file, so no entry
    point has a chain of its own beside the shared one; both entry points call that one body with all they were given, and
    nothing reaches it through the context."""
    with open(os.path.join(ROOT, "esac_amd", "csrc", "esac_capi.hip")) as fh:
        text = fh.read()
    bodies = []

    def body_of(signature):
        assert text.count(signature) == 1, signature
        start = text.index(signature)
        return text[start:text.index("\n}\n", start) + 3]

    for signature in ("static int backward_batch_dev_impl(", "static int begin_bwd_batch(", "static int chunk_args(",
                      "static int enqueue_bwd_sampling(", "static void fill_bwd(", "static int enqueue_bwd_chain("):
        bodies.append(body_of(signature))
        assert bodies[-1].count("\n") > 5, signature  # (a body, not a declaration)
    dev = bodies[0]
    for helper in ("begin_bwd_batch(", "chunk_args(", "enqueue_bwd_sampling(", "fill_bwd(", "enqueue_bwd_chain("):
        assert helper in dev, helper
    for entry in ('extern "C" int esac_hip_backward_batch_dev(', 'extern "C" int esac_hip_backward_batch_dev_shapes('):
        wrapper = body_of(entry)
        assert wrapper.count("return backward_batch_dev_impl(c, BwdBatchIn{") == 1 and wrapper.count(";") == 1, wrapper
    assert "shapes_next" not in text
    body = "\n".join(bodies)
    assert "launch_bwd_accumulate" in body and "launch_bwd_gt_prepare" in body
    for word in ("hipStreamSynchronize", "hipDeviceSynchronize", "hipMemcpy(", "wait_record", "hipEventSynchronize", "attempt"):
        assert word not in body, word
    assert text.count("launch_bwd_accumulate(") == 1


def test_backward_batch_async_is_exported_by_the_drop_in_module():
    import esac
    assert esac.backward_batch_async is api.backward_batch_async
    assert list(inspect.signature(api.backward_batch_async).parameters) == list(inspect.signature(api.backward_batch).parameters)
    assert list(inspect.signature(api.Engine.backward_batch_async).parameters) == [
        "self", "scene_coords", "out_gradients", "hyp_assign", "gt_poses", "w_rot", "w_trans", "loss_cut", "params", "cams", "out"]


def _args(B=2, E=1, H=12, W=16, N=8):
    sc = torch.zeros(B, E, 3, H, W)
    return [sc, torch.zeros_like(sc), torch.zeros(B, N, dtype=torch.int64), torch.eye(4).repeat(B, 1, 1),
            1.0, 100.0, 100.0, 0, 0, 525.0, 320.0, 240.0, 10.0, 100.0, 0.5, 100.0, 8]


@pytest.mark.parametrize("bad, match", [
    (lambda a: None, "outGradients must be a device tensor"),  # CPU gradients
    (lambda a: a.__setitem__(1, torch.zeros(2, 1, 3, 12, 32)[..., ::2]), "outGradients must be contiguous"),  # strided gradients
    (lambda a: a.__setitem__(2, torch.zeros(2, 8, dtype=torch.int32)), "hypAssignment"),
    (lambda a: a.__setitem__(2, torch.zeros(8, dtype=torch.int64)), "hypAssignment"),
    (lambda a: a.__setitem__(2, torch.zeros(2, 0, dtype=torch.int64)), "hypAssignment"),
    (lambda a: a.__setitem__(0, torch.zeros(2, 1, 3, 12, 16, dtype=torch.float64)), "sceneCoordinates"),
    (lambda a: a.__setitem__(0, torch.zeros(2, 1, 2, 12, 16)), "sceneCoordinates"),
    (lambda a: a.__setitem__(0, torch.zeros(3, 12, 16)), "sceneCoordinates"),
    (lambda a: a.__setitem__(0, torch.zeros(3, 1, 3, 12, 16)), "batch sizes"),  # B mismatch
    (lambda a: a.__setitem__(1, torch.zeros(3, 1, 3, 12, 16)), "outGradients"),  # B mismatch
    (lambda a: a.__setitem__(1, torch.zeros(2, 1, 3, 12, 15)), "outGradients"),
    (lambda a: a.__setitem__(1, torch.zeros(2, 1, 3, 12, 16, dtype=torch.float64)), "outGradients"),
    (lambda a: a.__setitem__(3, torch.eye(4)), "gtPoses"),
    (lambda a: a.__setitem__(3, torch.eye(4).repeat(3, 1, 1)), "gtPoses"),  # B mismatch
    (lambda a: a.__setitem__(3, torch.eye(4, dtype=torch.float64).repeat(2, 1, 1)), "gtPoses"),
    (lambda a: a.__setitem__(3, [[1.0]]), "gtPoses must be a torch.Tensor"),
    # per-frame cameras
    (lambda a: a.__setitem__(7, [0, 1, 2]), "shiftX"),
    (lambda a: a.__setitem__(8, [0.5, 1]), "shiftY"),
    (lambda a: a.__setitem__(9, [525.0, 0.0]), "focalLength"),
    (lambda a: a.__setitem__(10, [320.0, float("nan")]), "ppointX"),
    (lambda a: a.__setitem__(11, "wide"), "ppointY"),
])
def test_backward_batch_async_validates_before_any_device(bad, match):
    import esac
    args = _args()
    bad(args)
    engines = dict(api._state["engines"])
    call = api.get_rng_state()
    with pytest.raises(RuntimeError, match=match):
        esac.backward_batch_async(*args)
    assert api._state["engines"] == engines  # no engine was created by the call: nothing reached a device
    assert api.get_rng_state() == call


def test_backward_batch_async_refuses_strict_reference():
    import esac
    esac.set_strict_reference(True)
    try:
        with pytest.raises(ValueError, match="backward_batch_async"):
            esac.backward_batch_async(*_args())
    finally:
        esac.set_strict_reference(False)


def test_train_batch_keywords_default_to_off():
    sig = inspect.signature(harness.train_batch)
    assert sig.parameters["asynchronous"].default is False
    assert sig.parameters["all_experts"].default is False
