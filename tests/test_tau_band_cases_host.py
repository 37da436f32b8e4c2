"""CPU conditions on the fixtures of tests/tau_band_cases.py: what makes tests/test_gpu_tau_band.py mean something.  A case that
fails one of them has a generator to be fixed, never a condition to be loosened."""
import os
import re

import numpy as np
import pytest

from tests import tau_band_cases as T

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "esac_amd", "csrc")
ALL = list(T.CASES)


@pytest.mark.parametrize("name", ALL)
def test_enough_cells_on_the_band(oracle, name):
    """At least a quarter of the tuned cells inside band2 in float64, and at least 16 cells on which the reference's float
    arithmetic and the plain float64 comparison decide differently (where there is a decision: T.DECIDING_CASES)."""
    c = T.build_case(name)
    p, tau = c["params"], T.tau32(c["params"])
    ref = T.reference(oracle, name)
    with np.errstate(invalid="ignore"):
        in_band = c["tuned"] & (np.abs(c["err64"] - tau) < c["band2"])
    disagree = (ref["inlier_map"] != 0) != T.plain_decision(c["err64"], p)
    print("%s: %d tuned, %d in band (%.0f %%), %d cells where float and fp64 disagree, farthest %.2e px from tau"
          % (name, c["tuned"].sum(), in_band.sum(), 100.0 * in_band.sum() / c["tuned"].sum(), disagree.sum(),
             np.abs(c["err64"] - tau)[disagree].max(initial=0.0)))
    assert c["tuned"].sum() <= T.MAX_TUNED
    assert 4 * in_band.sum() >= c["tuned"].sum()
    if name in T.DECIDING_CASES:
        assert disagree.sum() >= 16
    else:
        assert disagree.sum() == 0 and ref["inlier_map"].sum() == p["H"] * p["W"] - 2  # everything but the two non-finite cells
    # the adversarial kinds are there
    assert (c["cls"] == T.CLS_NONFINITE).sum() == 2 and (c["cls"] == T.CLS_PLANE).sum() == 4 and c["behind"].sum() >= 4
    for k in range(T.N_DELTA):
        assert (c["cls"] == k).sum() >= 4, T.CLASS_NAMES[k]
    if p["identity"]:  # zc == 0 exactly, and on the band
        z = c["coords"][0, 2][c["cls"] == T.CLS_PLANE].astype(np.float64) + c["hyp"][0, 5]
        assert np.all(z == 0.0) and np.all(np.abs(c["err64"][c["cls"] == T.CLS_PLANE] - tau) < 1e-5)


@pytest.mark.parametrize("name", ALL)
def test_band_is_sound(oracle, name):
    """|reference's float error - float64 error| on every cell within 1e-3 px of tau stays below band2: the second screen can
    never decide differently from the reference."""
    c = T.build_case(name)
    p, tau = c["params"], T.tau32(c["params"])
    ref = T.reference(oracle, name)
    clamped = np.minimum(c["err64"], float(np.float32(p["max_reproj"])))
    with np.errstate(invalid="ignore"):
        near = np.abs(c["err64"] - tau) < 1e-3
    worst = float(np.abs(ref["winner_errs"].astype(np.float64) - clamped)[near].max())
    print("%s: %d cells within 1e-3 px of tau, worst |reference - fp64| = %.3e px = %.3f band2 (band2 = %.3e px)"
          % (name, near.sum(), worst, worst / c["band2"], c["band2"]))
    assert near.sum() >= c["tuned"].sum() // 2
    assert worst < c["band2"]


def test_one_band_formula():
    """band2 is spelled once: the text in refine_team.hpp:make_band and in esac_refine.hip:error_pass_impl is T.BAND2_C, and
    T.band2 computes what that text says."""
    for src in ("refine_team.hpp", "esac_refine.hip"):
        with open(os.path.join(CSRC, src)) as f:
            found = re.findall(r"const double band2 = (.*);", f.read())
        assert found == [T.BAND2_C], (src, found)
    expr = T.BAND2_C.replace("(double)", "").replace("(a.W > a.H ? a.W : a.H)", "max(a.W, a.H)")

    class A:
        pass
    for name in ALL:
        p = T.case_params(name)
        a = A()
        a.W, a.H, a.sub, a.shift_x, a.shift_y, a.tau = p["W"], p["H"], p["sub"], p["shift_x"], p["shift_y"], T.tau32(p)
        assert eval(expr, {"a": a, "abs": abs, "max": max}) == T.band2(p), name


@pytest.mark.parametrize("name", T.SECOND_PASS_CASES)
def test_next_pose_is_clear_of_the_band(oracle, name):
    """At the pose the reference's first re-fit returns no cell lies within 1e-4 px of tau: a pose that differs from it by
    1e-9 decides every cell the same way, so the count of the SECOND pass can be compared too."""
    c = T.build_case(name)
    ref = T.reference(oracle, name)
    assert ref["ref_steps"] == 1
    e = T.err64(ref["refined"], c["coords"], c["params"])
    with np.errstate(invalid="ignore"):
        nearest = float(np.nanmin(np.abs(e - T.tau32(c["params"]))))
    print("%s: nearest cell to tau at the next pose: %.3e px" % (name, nearest))
    assert nearest >= 1e-4


def test_sampled_hypothesis_fixtures(oracle):
    """The fixtures of the calls that sample their own hypotheses (T.sampled_frame asserts that the band cells leave tries,
    sampled cells and hypotheses what they were, and that no tuned cell's first-pass decision moves under +-1e-9 of the pose):
    the conditions above, counted on what the stability filter left, and every later pose of the refinement clear of the band."""
    for frames in (T.TEAM_FRAMES, T.SMALL_FRAMES, [T.HEADLINE_FRAME]):
        for k, call, H, W, sub in frames:
            c = T.sampled_frame(oracle, k, call, H, W, sub, N=4 if frames is T.TEAM_FRAMES else 1)
            in_band, disagree, ratio = T.sampled_figures(c)
            print("frame %d (%dx%d): %d tuned, %d reset by the stability filter, %d in band, %d disagreeing, worst |reference - fp64| = "
                  "%.3f band2, %d steps, nearest cell at a later pose %.2e px"
                  % (k, H, W, c["tuned"].sum(), c["removed"], in_band, disagree, ratio, c["ref1"]["ref_steps"], c["nearest_later"]))
            assert 4 * in_band >= c["tuned"].sum() and ratio < 1.0
            assert c["ref1"]["ref_steps"] >= 1 and c["nearest_later"] >= 1e-4
            assert c["ref1"]["winner"] == 0
            assert disagree >= 16
            if frames is T.TEAM_FRAMES:
                assert (c["ref"]["tries"] == 0).all() and len(c["ref"]["tries"]) == 4
