"""The batched evaluation path without a device: the additive ABI symbol, the EVAL_* mirror of the header, the argument checks of
esac.eval_batch / esac.forward_batch_async (RuntimeError naming the argument before any device is touched), frames_to_rerun and the
signatures of the harness."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

from esac_amd import api, harness

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "esac_hip.h")).read()


def test_symbol_is_additive_and_the_version_stays():
    assert re.search(r"\bint esac_hip_eval_batch\s*\(", HEADER)
    assert "esac_hip_eval_batch" in api.ABI_SYMBOLS
    assert api.ABI_VERSION == 6 and re.search(r"#define ESAC_HIP_ABI_VERSION 6\b", HEADER)
    from esac_amd import build
    assert "esac_eval.hip" in build.SOURCES and "eval_math.hpp" in build.HEADERS


def test_eval_constants_mirror_the_header():
    body = re.search(r"enum \{ (ESAC_EVAL_ROT_DEG.*?)\};", HEADER, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    header = {m.group(1): int(m.group(2)) for m in re.finditer(r"ESAC_EVAL_(\w+)\s*=\s*(\d+)", body)}
    assert header == {"ROT_DEG": api.EVAL_ROT_DEG, "TRANS_CM": api.EVAL_TRANS_CM, "POSE_OK": api.EVAL_POSE_OK,
                      "CLASS_OK": api.EVAL_CLASS_OK, "QUAT": api.EVAL_QUAT, "INV_T": api.EVAL_INV_T, "EXPERT": api.EVAL_EXPERT,
                      "HYP": api.EVAL_HYP, "STATUS": api.EVAL_STATUS}
    assert int(re.search(r"#define ESAC_EVAL_DOUBLES (\d+)", HEADER).group(1)) == api.EVAL_DOUBLES == 16
    assert int(re.search(r"#define ESAC_MAX_BATCH (\d+)", HEADER).group(1)) == api.MAX_BATCH
    assert int(re.search(r"ESAC_RES_VALID = (\d+),", HEADER).group(1)) == api.RES_VALID
    import esac
    assert esac.eval_batch is api.eval_batch and esac.forward_batch_async is api.forward_batch_async


def _eval_args():
    return dict(records=torch.zeros(3, 32, dtype=torch.float64), gtPoses=torch.zeros(3, 4, 4), gtExperts=torch.zeros(3, dtype=torch.int64),
                rotThreshold=5.0, transThreshold=5.0)


EVAL_ERRORS = {
    "records_type": (dict(records=np.zeros((3, 32))), "records"),
    "records_dtype": (dict(records=torch.zeros(3, 32)), "records"),
    "records_shape": (dict(records=torch.zeros(3, 31, dtype=torch.float64)), "records"),
    "records_rank": (dict(records=torch.zeros(96, dtype=torch.float64)), "records"),
    "records_empty": (dict(records=torch.zeros(0, 32, dtype=torch.float64), gtPoses=torch.zeros(0, 4, 4), gtExperts=None), "records"),
    "records_too_many": (dict(records=torch.zeros(1025, 32, dtype=torch.float64), gtPoses=torch.zeros(1025, 4, 4), gtExperts=None), "records"),
    "records_on_host": (dict(), "records"),  # everything else in order: the records of a forward batch live on the device
    "poses_dtype": (dict(gtPoses=torch.zeros(3, 4, 4, dtype=torch.float64)), "gtPoses"),
    "poses_shape": (dict(gtPoses=torch.zeros(3, 3, 4)), "gtPoses"),
    "poses_batch": (dict(gtPoses=torch.zeros(2, 4, 4)), "gtPoses"),
    "poses_array_batch": (dict(gtPoses=np.zeros((4, 4, 4))), "gtPoses"),
    "poses_type": (dict(gtPoses="poses"), "gtPoses"),
    "experts_dtype": (dict(gtExperts=torch.zeros(3, dtype=torch.int32)), "gtExperts"),
    "experts_batch": (dict(gtExperts=torch.zeros(4, dtype=torch.int64)), "gtExperts"),
    "experts_list_batch": (dict(gtExperts=[0, 1]), "gtExperts"),
    "experts_floats": (dict(gtExperts=[0.5, 1.0, 2.0]), "gtExperts"),
    "rot_negative": (dict(rotThreshold=-1.0), "rotThreshold"),
    "rot_nan": (dict(rotThreshold=float("nan")), "rotThreshold"),
    "trans_inf": (dict(transThreshold=float("inf")), "transThreshold"),
    "trans_none": (dict(transThreshold=None), "transThreshold"),
}


@pytest.mark.parametrize("bad", sorted(EVAL_ERRORS))
def test_eval_batch_argument_errors_name_the_argument(bad, monkeypatch):
    import esac
    monkeypatch.setattr(api, "engine", lambda *a, **k: pytest.fail("an argument error must be raised before any device is touched"))
    change, name = EVAL_ERRORS[bad]
    args = _eval_args()
    args.update(change)
    with pytest.raises(RuntimeError, match=r"esac\.eval_batch: .*" + name):
        esac.eval_batch(**args)


CAM = (0, 0, 525.0, 320.0, 240.0)
SOLVER = (10.0, 100.0, 0.5, 100.0, 8)
FWD_ERRORS = {
    "ha_dtype": ((torch.zeros(2, 1, 3, 60, 80), torch.zeros(2, 8, dtype=torch.int32)) + CAM, "hypAssignment"),
    "ha_rank": ((torch.zeros(2, 1, 3, 60, 80), torch.zeros(8, dtype=torch.int64)) + CAM, "hypAssignment"),
    "ha_empty": ((torch.zeros(2, 1, 3, 60, 80), torch.zeros(2, 0, dtype=torch.int64)) + CAM, "hypAssignment"),
    "ha_type": ((torch.zeros(2, 1, 3, 60, 80), [[0] * 8] * 2) + CAM, "hypAssignment"),
    "sc_dtype": ((torch.zeros(2, 1, 3, 60, 80, dtype=torch.float64), torch.zeros(2, 8, dtype=torch.int64)) + CAM, "sceneCoordinates"),
    "sc_rank": ((torch.zeros(3, 60, 80), torch.zeros(2, 8, dtype=torch.int64)) + CAM, "sceneCoordinates"),
    "sc_chan": ((torch.zeros(2, 1, 2, 60, 80), torch.zeros(2, 8, dtype=torch.int64)) + CAM, "sceneCoordinates"),
    "sc_batch": ((torch.zeros(3, 1, 3, 60, 80), torch.zeros(2, 8, dtype=torch.int64)) + CAM, "sceneCoordinates"),
    "too_many": ((torch.zeros(1, 3, 60, 80), torch.zeros(1025, 8, dtype=torch.int64)) + CAM, "hypAssignment"),
    "focal_len": ((torch.zeros(2, 1, 3, 60, 80), torch.zeros(2, 8, dtype=torch.int64), 0, 0, [525.0, 525.0, 525.0], 320.0, 240.0), "focalLength"),
    "focal_sign": ((torch.zeros(2, 1, 3, 60, 80), torch.zeros(2, 8, dtype=torch.int64), 0, 0, [525.0, -1.0], 320.0, 240.0), "focalLength"),
    "shift_frac": ((torch.zeros(2, 1, 3, 60, 80), torch.zeros(2, 8, dtype=torch.int64), [0.5, 0], 0, 525.0, 320.0, 240.0), "shiftX"),
}


@pytest.mark.parametrize("bad", sorted(FWD_ERRORS))
def test_forward_batch_async_argument_errors_name_the_argument(bad, monkeypatch):
    import esac
    monkeypatch.setattr(api, "engine", lambda *a, **k: pytest.fail("an argument error must be raised before any device is touched"))
    args, name = FWD_ERRORS[bad]
    before = esac.get_rng_state()
    with pytest.raises(RuntimeError, match=r"esac\.forward_batch_async: .*" + name):
        esac.forward_batch_async(*(args + SOLVER))
    assert esac.get_rng_state() == before  # a refused call draws no call counters


def test_forward_batch_async_signature_is_forward_batch_minus_out_poses():
    import esac
    want = [p for p in inspect.signature(esac.forward_batch).parameters if p != "outPoses"]
    assert list(inspect.signature(esac.forward_batch_async).parameters) == want
    sig = inspect.signature(esac.eval_batch)
    assert list(sig.parameters) == ["records", "gtPoses", "gtExperts", "rotThreshold", "transThreshold"]
    assert sig.parameters["gtExperts"].default is None and sig.parameters["rotThreshold"].default == 5.0 and sig.parameters["transThreshold"].default == 5.0
    eng = inspect.signature(api.Engine.eval_batch)
    assert list(eng.parameters) == ["self", "records", "gt_poses", "gt_experts", "rot_threshold_deg", "trans_threshold_cm", "out"]


def test_frames_to_rerun_on_a_hand_made_table():
    ev = np.zeros((6, api.EVAL_DOUBLES))
    ev[:, api.EVAL_STATUS] = [0, 3, 1, 3, 0, 3]
    ev[2, api.EVAL_ROT_DEG] = np.nan
    assert harness.frames_to_rerun(ev) == [1, 3, 5]
    assert harness.frames_to_rerun(ev[:1]) == [] and harness.frames_to_rerun(np.zeros((0, api.EVAL_DOUBLES))) == []
    assert harness.frames_to_rerun(torch.from_numpy(ev).numpy()[3]) == [0]  # one row
    before = ev.copy()
    harness.frames_to_rerun(ev)
    np.testing.assert_array_equal(ev, before)  # a pure function


def test_harness_signatures():
    sig = inspect.signature(harness.evaluate)
    assert sig.parameters["batch_size"].default == 1 and sig.parameters["asynchronous"].default is False
    assert list(sig.parameters)[:6] == ["samples", "gating", "experts", "trans_threshold_cm", "rot_threshold_deg", "pose_log"]
    lb = inspect.signature(harness.localize_batch)
    for name, default in (("gt_poses", None), ("gt_experts", None), ("e_hyps", None), ("expert_selection", False), ("oracle_experts", None),
                          ("generator", None), ("asynchronous", False), ("all_experts", False), ("strict_reference", False),
                          ("rot_threshold_deg", 5.0), ("trans_threshold_cm", 5.0)):
        assert lb.parameters[name].default == default or lb.parameters[name].default is default, name
    assert list(lb.parameters)[:4] == ["images", "gating", "experts", "focal_lengths"]
    assert list(inspect.signature(harness.rerun_frames).parameters) == ["batch_out", "frames"]


def test_host_row_is_the_loops_own_arithmetic():
    """eval_row_host = pose_errors_deg_cm + the numbers of pose_file_line + the loop's two comparisons."""
    from esac_amd import synthetic as S
    f = S.make_frame(0)
    gt = f["gt_pose"]
    other = gt.copy()
    other[:3, 3] += [0.03, 0.0, 0.04]
    row = harness.eval_row_host(other, gt, 2, 17, 2)
    assert (row[api.EVAL_ROT_DEG], row[api.EVAL_TRANS_CM]) == harness.pose_errors_deg_cm(other, gt)
    assert row[api.EVAL_POSE_OK] == 0.0 and row[api.EVAL_CLASS_OK] == 1.0 and row[api.EVAL_EXPERT] == 2.0 and row[api.EVAL_HYP] == 17.0
    assert harness.eval_row_host(other, gt, 2, 17, 2, trans_threshold_cm=5.1)[api.EVAL_POSE_OK] == 1.0
    assert harness.eval_row_host(other, gt, 2, 17, None)[api.EVAL_CLASS_OK] == -1.0
    line = harness.POSE_LINE_FORMAT % (("n",) + tuple(row[api.EVAL_QUAT:api.EVAL_QUAT + 7]))
    assert line == harness.pose_file_line("n", other)
