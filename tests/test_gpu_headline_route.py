"""The route kernel of the refinement team (k_refine_team_route: the headline call's modes compiled in) against the general
kernel (k_refine_team: the same body, every mode read from the argument block): the same call twice on one engine, once with
the route kernel and once with set_refine_route(False), every output compared byte for byte.  The record carries what the
kernel's prologue computes beside the winner (probability, entropy, number of contenders: the softmax statistics).

Each case asserts through refine_info that the kernel it means to run did run.  No case provokes a team time-out."""
import numpy as np
import pytest
import torch

from esac_amd import api
from esac_amd import synthetic as S

pytestmark = pytest.mark.gpu

SEED = 1320
BUFFERS = {"hyps": api.BUF_HYPS, "tries": api.BUF_TRIES, "scores": api.BUF_SCORES, "inlier_map": api.BUF_INLIER_MAP,
           "inlier_counts": api.BUF_INLIER_COUNTS}
RECORD_WORDS = 32  # the whole host record: score .. LM iterations, and which map buffer holds the accepted set


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a.view(np.uint32) if a.dtype == np.float32 else a


def _call(engine, f, ha, route, k=0, team=None, **kw):
    """One esac_hip_forward with esac.forward's default flags (ESAC_FLAG_AUTO_EXACT): everything a caller can see of it."""
    E, _, H, W = f["coords"].shape
    p = engine.make_params(E, H, W, len(ha), shift_x=f["shift"][0], shift_y=f["shift"][1], focal=f["focal"], ppx=f["ppx"], ppy=f["ppy"],
                           sub_sampling=f["sub"], seed=SEED, call=k, exact_scores="auto", **kw)
    scores_out = torch.full((len(ha),), -7.0, dtype=torch.float64, device="cuda")
    result_out = torch.full((api.RES_DOUBLES,), -7.0, dtype=torch.float64, device="cuda")
    engine.set_refine_route(route)
    if team is not None:
        engine.set_refine_team(team)
    try:
        res = engine.forward_device(torch.from_numpy(f["coords"]).cuda(), torch.from_numpy(ha).cuda(), p, scores_out=scores_out, result_out=result_out)
        out = {name: np.array(engine.read(buf)) for name, buf in BUFFERS.items()}
        out["record"] = np.array(res[:RECORD_WORDS], dtype=np.float64)
        out["scores_out"] = scores_out.cpu().numpy()
        out["result_out"] = result_out.cpu().numpy()
        info = engine.refine_info()
    finally:
        engine.set_refine_route(True)
        if team is not None:
            engine.set_refine_team(api.REFINE_TEAM_DEFAULT)
    return out, info


def _both(engine, f, ha, members, expect_route=True, **kw):
    """The call on the route kernel and on the general kernel: identical bytes; returns the route run's outputs."""
    a, info_a = _call(engine, f, ha, True, **kw)
    b, info_b = _call(engine, f, ha, False, **kw)
    for info in (info_a, info_b):
        assert info["mode"] == "team" and info["workgroups"] == members and not info["timed_out"], info
    assert info_a["route_kernel"] == expect_route and not info_b["route_kernel"], (info_a, info_b)
    assert a["record"][api.RES_HYP] >= 0 and a["result_out"][api.RES_VALID] == 1.0
    for name in a:
        np.testing.assert_array_equal(_bits(a[name]), _bits(b[name]), err_msg=name)
    return a


def _frame(N, k=0, **frame):
    f = S.make_frame(k, E=1, **frame)
    return f, S.gating_assignment(f, N)


def test_headline_call_default_team(engine):
    """60x80, 256 hypotheses: ten members, two cells per lane -- k_refine_team_route<2, 16>, the headline call itself."""
    out = _both(engine, *_frame(256), members=10)
    assert out["record"][api.RES_REF_STEPS] >= 1 and out["record"][api.RES_CONTENDERS] == 256


@pytest.mark.parametrize("N", [1, 4])
def test_few_hypotheses(engine, N):
    """Threads beyond N hold no hypothesis: the softmax sums, the argmax and the winner's hand-over through LDS."""
    out = _both(engine, *_frame(N), members=10)
    assert out["record"][api.RES_CONTENDERS] == N and 0 <= out["record"][api.RES_HYP] < N


def test_team_of_eight(engine):
    """Eight members, three cells per lane, the 8-wide exchange: k_refine_team_route<3, 8>."""
    _both(engine, *_frame(256), members=8, team=8)


def test_smallest_team_grid_one_cell_per_lane(engine):
    """32x32 = 1024 cells, the smallest grid a team refines: four members of 256 cells, k_refine_team_route<1, 8>."""
    _both(engine, *_frame(64, H=32, W=32), members=4)


def test_non_finite_scene_coordinates(engine):
    """Cells whose scene point is NaN / inf are in no inlier set (TeamCells::live)."""
    f, ha = _frame(256, k=1)
    c = f["coords"]
    c[0, 0, 3, 5] = np.nan
    c[0, 1, 17, 40] = np.inf
    c[0, 2, 30, 79] = -np.inf
    c[0, :, 59, 0] = np.nan
    out = _both(engine, f, ha, members=10, k=1)
    m = out["inlier_map"]  # [60, 80]: the buffer that holds the accepted set (a team: buffer 0)
    assert m[3, 5] == 0 and m[17, 40] == 0 and m[30, 79] == 0 and m[59, 0] == 0
    assert out["record"][api.RES_REF_STEPS] >= 1 and m.sum() > 500


def test_sampler_second_round(engine):
    """60 % outliers: hypotheses that go on past the sampler's shared rounds (try 128 and later) feed the same refinement."""
    out = _both(engine, *_frame(256, outlier_frac=0.6), members=10)
    assert int((out["tries"] >= 128).sum()) >= 8


def test_max_ref_steps_reached(engine):
    """max_ref_steps = 1: the loop leaves through the step limit, the pass that ended it evaluated at the refined pose."""
    free = _both(engine, *_frame(256), members=10)
    assert free["record"][api.RES_REF_STEPS] > 1
    out = _both(engine, *_frame(256), members=10, max_ref_steps=1)
    assert out["record"][api.RES_REF_STEPS] == 1


def test_257_hypotheses_run_the_general_kernel(engine):
    """More hypotheses than a member has threads: no folded selection, so the general kernel whatever the switch says."""
    _both(engine, *_frame(257), members=10, expect_route=False)
