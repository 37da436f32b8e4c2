"""CPU checks of the batched training entry point (esac.backward_batch / esac_hip_backward_batch): it is declared and
exported, and every shape or dtype error is raised before a device is touched."""
import os

import pytest
import torch

from esac_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_backward_batch_is_part_of_the_abi():
    assert "esac_hip_backward_batch" in api.ABI_SYMBOLS
    assert api.ABI_VERSION == 6
    with open(os.path.join(ROOT, "include", "esac_hip.h")) as fh:
        assert "int esac_hip_backward_batch(esac_hip_ctx* ctx, int B," in fh.read()


def test_backward_batch_is_exported_by_the_drop_in_module():
    import esac
    assert esac.backward_batch is api.backward_batch


def _args(B=2, E=1, H=12, W=16, N=8):
    sc = torch.zeros(B, E, 3, H, W)
    return [sc, torch.zeros_like(sc), torch.zeros(B, N, dtype=torch.int64), torch.eye(4).repeat(B, 1, 1),
            1.0, 100.0, 100.0, 0, 0, 525.0, 320.0, 240.0, 10.0, 100.0, 0.5, 100.0, 8]


@pytest.mark.parametrize("bad, match", [
    (lambda a: a.__setitem__(2, torch.zeros(2, 8, dtype=torch.int32)), "hypAssignment"),
    (lambda a: a.__setitem__(2, torch.zeros(8, dtype=torch.int64)), "hypAssignment"),
    (lambda a: a.__setitem__(2, torch.zeros(2, 0, dtype=torch.int64)), "hypAssignment"),
    (lambda a: a.__setitem__(0, torch.zeros(2, 1, 3, 12, 16, dtype=torch.float64)), "sceneCoordinates"),
    (lambda a: a.__setitem__(0, torch.zeros(2, 1, 2, 12, 16)), "sceneCoordinates"),
    (lambda a: a.__setitem__(0, torch.zeros(3, 1, 3, 12, 16)), "batch sizes"),
    (lambda a: a.__setitem__(0, torch.zeros(3, 12, 16)), "sceneCoordinates"),
    (lambda a: a.__setitem__(1, torch.zeros(2, 1, 3, 12, 15)), "outGradients"),
    (lambda a: a.__setitem__(1, torch.zeros(1, 3, 12, 16)), "outGradients"),
    (lambda a: a.__setitem__(1, torch.zeros(2, 1, 3, 12, 16, dtype=torch.float64)), "outGradients"),
    (lambda a: a.__setitem__(3, torch.eye(4)), "gtPoses"),
    (lambda a: a.__setitem__(3, torch.eye(4, dtype=torch.float64).repeat(2, 1, 1)), "gtPoses"),
    (lambda a: a.__setitem__(2, torch.full((2, 8), 1, dtype=torch.int64)), r"\[0,1\)"),
    (lambda a: a.__setitem__(3, [[1.0]]), "torch.Tensor"),
])
def test_backward_batch_validates_before_any_device(bad, match):
    import esac
    args = _args()
    bad(args)
    engines = dict(api._state["engines"])
    with pytest.raises(RuntimeError, match=match):
        esac.backward_batch(*args)
    assert api._state["engines"] == engines  # no engine was created by the call: nothing reached a device
