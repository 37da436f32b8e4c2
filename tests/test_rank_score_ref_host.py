"""CPU: the fp64 reference of the ranking score (tests/rank_score_ref.py) pinned to the oracle, and the preconditions the GPU
cases of tests/test_gpu_rank_score.py rely on, checked from the reference alone."""
import numpy as np
import pytest

from esac_amd import synthetic as S
from tests import rank_score_cases as C
from tests import rank_score_ref as ref


@pytest.mark.parametrize("H,W,sub", [(40, 64, 10), (37, 51, 12)])
def test_reference_agrees_with_the_oracle(oracle, H, W, sub):
    """Two experts, 96 sampled hypotheses: |fp64 reference - oracle| <= |alpha| |beta| / 4 * 1e-4.  The bound is derived: the
    reference rounds each projected pixel to float, which moves an error by < 1e-4 px at coordinates < 1024 (a larger one is an
    error beyond maxReproj either way), and the slope of the sigmoid is at most |beta| / 4.  Measured: 2e-6."""
    alpha, beta, tau, max_reproj = 100.0, 0.5, 10.0, 100.0
    f = S.make_frame(310 + H, E=2, true_expert=1, H=H, W=W, sub=sub)
    ha = S.gating_assignment(f, 96, mode="gating")
    out = oracle.forward(f["coords"], ha, focal=f["focal"], ppx=f["ppx"], ppy=f["ppy"], sub_sampling=sub, inlier_thresh=tau,
                         inlier_alpha=alpha, inlier_beta=beta, max_reproj=max_reproj, seed=1305, call=4)
    assert (out["tries"] >= 0).sum() >= 48  # sampled poses, not the zero pose of an exhausted budget
    got = ref.scores(f["coords"], ha, out["hyps"], f["focal"], f["ppx"], f["ppy"], sub, (0, 0), alpha, beta, tau, max_reproj)
    d = np.abs(got - out["scores"]).max()
    print("H %d W %d: max |reference - oracle| = %.3g" % (H, W, d))
    assert d <= alpha * beta / 4.0 * 1e-4, d


def test_reference_rotation_helpers_are_inverse():
    rng = np.random.default_rng(7)
    for r in [rng.normal(size=3) * s for s in (1e-9, 1e-3, 0.5, 2.0)] + [np.array([0.0, np.pi, 0.0]), np.array([np.pi, 0.0, 0.0]) * (1 - 1e-12)]:
        R = ref.rodrigues(r)
        np.testing.assert_allclose(R @ R.T, np.eye(3), atol=1e-14)
        np.testing.assert_allclose(ref.rodrigues(ref.rotation_vector(R)), R, atol=1e-12)


def test_reference_scores_a_non_finite_cell_as_an_outlier():
    """The default route's rule: a cell with a non-finite coordinate reads err = maxReproj -- exactly the score of
    the same cell at 1e30, which the reference clamps."""
    c = C.get("healthy-stream")
    h, e = c["hyps"][0], int(c["assign"][0])
    args = (ref.rodrigues(h[:3]), h[3:], c["focal"], c["ppx"], c["ppy"], c["sub"], (0, 0), c["alpha"], c["beta"], c["tau"], c["max_reproj"])
    base = c["coords"][e].copy()
    clean = ref.score(base, *args)
    for bad in (np.nan, np.inf, -np.inf):
        m, far = base.copy(), base.copy()
        m[1, 5, 7] = bad
        far[1, 5, 7] = 1e30
        assert ref.score(m, *args) == ref.score(far, *args) <= clean


@pytest.mark.parametrize("name", C.NAMES)
def test_case_preconditions(name):
    """What the GPU test of this case relies on: no two hypotheses identical (two equal poses on different experts count as
    different), the ground-truth pose at index 0 on the true expert and, where the winner is checked, a gap of >= 1e-3 between
    the two best fp64 scores -- 8x the oracle bound of the default parameters, so `the fp64 argmax` names one hypothesis."""
    c = C.get(name)
    keyed = np.concatenate([c["hyps"], c["assign"][:, None].astype(np.float64)], axis=1)
    assert len(np.unique(keyed, axis=0)) == c["N"]
    assert len(np.unique(c["hyps"], axis=0)) == c["N"]
    assert c["hyps"].shape == (c["N"], 6) and c["assign"].shape == (c["N"],) and np.isfinite(c["hyps"]).all()
    counts = np.bincount(c["assign"], minlength=c["E"])
    if name == "chunks":
        assert tuple(counts) == C.CHUNK_COUNTS and c["N"] > 1024
        order = np.argsort(c["assign"], kind="stable")
        assert (order != np.arange(c["N"])).any()
    s = C.reference(c)
    assert np.isfinite(s).all()
    top = np.sort(s)[::-1]
    print("%s: fp64 best %.4f (index %d), gap to the second %.3g" % (name, top[0], int(np.argmax(s)), top[0] - top[1]))
    if c["winner_check"]:
        assert top[0] - top[1] >= 1e-3
        assert c["assign"][int(np.argmax(s))] == c["assign"][0]  # the best pose sits on the true expert's map
