"""GPU: the fp32 ranking score (k_score_fast<512>, k_score_fast<256>, k_score_tiled<NEG>, and k_score_stragglers through the
whole call) against a plain fp64 reference on adversarial maps.

The winner of a call is right only while the truly best hypothesis stays within margin = |alpha| (1e-3 + 2 / (H W)) of the fp32
maximum (call_policy.hpp: call_scalars; DESIGN.md, "Precision contract").  That holds when every fp32 score is within margin / 2
of its true value: the bar of check 1.  The cases (tests/rank_score_cases.py; preconditions on the CPU in
tests/test_rank_score_ref_host.py) put what a diverged expert emits where the stream takes its origin from -- the middle of the
map -- and walk the store and chunk boundaries of the tiled route.
"""
import numpy as np
import pytest
import torch

from esac_amd import api
from tests import rank_score_cases as C
from tests.test_gpu_parity import EXACT_SCORE_TOL, FAST_SCORE_TOL, _check_full

pytestmark = pytest.mark.gpu


def _params(engine, c, **kw):
    return engine.make_params(c["E"], c["H"], c["W"], c["N"], focal=c["focal"], ppx=c["ppx"], ppy=c["ppy"], sub_sampling=c["sub"],
                              inlier_thresh=c["tau"], inlier_alpha=c["alpha"], inlier_beta=c["beta"], max_reproj=c["max_reproj"],
                              score_shape=c["route"], **kw)


def _fast_max(got, flags, want):
    """The fp32 maximum of a beta < 0 case: a flagged score has been replaced by its exact value, but no fp32 score exceeds
    alpha (every weight is <= 1) and the flagged ones tied at the maximum, which the unflagged ones lie below."""
    return max(float(got[~flags].max()) if (~flags).any() else -np.inf, float(want[flags].max()))


@pytest.mark.parametrize("name", C.NAMES)
def test_rank_score_against_fp64(engine, name):
    """1. error bar: with a band of 1e-30 only the fp32 maximum and its exact ties are re-scored (at most 2); every other
          hypothesis holds |fp32 - fp64| <= margin / 2.  mid_3e38: X - c overflows when the origin is that cell, every cell of the
          expert clamps, its scores are ~0 and the set ties into the band -- correct (the band is re-scored exactly) but slow;
          such a case passes on either the ordinary bar or on `every hypothesis of the poisoned expert is flagged or < 1e-3 alpha`.
       2. band: with the default margin the fp64 argmax is flagged, and every flagged score is the reference's to
          |alpha| |beta| / 4 * 1e-4 (the bound of test_reference_agrees_with_the_oracle).
       3. winner: argmax of the scores after step 2 is the fp64 argmax (cases whose fp64 top-two gap is >= 1e-3).
       4. chunks: check 1 over all N hypotheses of the ten experts (0, 1, 63, 64, 65, 255, 256, 257, 513, 0 of them)."""
    c = C.get(name)
    want = C.reference(c)
    M, N = C.margin(c), c["N"]
    sc, hat = torch.from_numpy(c["coords"].copy()).cuda(), torch.from_numpy(c["assign"].copy()).cuda()
    engine.forward_device(sc, hat, _params(engine, c, max_tries=4))  # shapes the workspace; its hypotheses are replaced
    engine.write_hyps(c["hyps"])
    p_tight, p = _params(engine, c, rescore_margin=1e-30), _params(engine, c)
    engine.score(sc, hat, p_tight)
    engine.select(sc, hat, p_tight)
    got = engine.read(api.BUF_SCORES).copy()
    flags = engine.read(api.BUF_EXACT_FLAGS).astype(bool)
    assert got.shape == (N,) and np.isfinite(got).all()
    d = np.abs(got - want)
    worst = float(d[~flags].max() / (M / 2)) if not flags.all() else 0.0
    print("rank score %-28s worst |fp32 - fp64| / (M/2) = %.3g  (M = %.4f, %d flagged at band 1e-30)" % (name, worst, M, int(flags.sum())))
    ordinary = worst <= 1.0 and flags.sum() <= 2
    if c["tie_exception"] and not ordinary:
        mine = c["assign"] == c["poisoned"]
        assert (flags[mine] | (got[mine] < 1e-3 * c["alpha"])).all(), (worst, int(flags.sum()))
        assert (d[~flags & ~mine] <= M / 2).all()
    elif c["beta"] < 0:
        # every cell of a bad pose weighs exactly 1.0f: dozens of exact ties at the fp32 maximum alpha, all flagged.  A flagged
        # hypothesis holds the same bar: its fp64 score is within M / 2 of the fp32 maximum it tied with.
        assert worst <= 1.0, worst
        assert flags.any() and (np.abs(want[flags] - _fast_max(got, flags, want)) <= M / 2).all()
    else:
        assert worst <= 1.0, (worst, int(np.argmax(np.where(flags, 0, d))))
        assert 1 <= flags.sum() <= 2, int(flags.sum())
    # 2. the default band
    engine.select(sc, hat, p)
    got = engine.read(api.BUF_SCORES).copy()
    flags = engine.read(api.BUF_EXACT_FLAGS).astype(bool)
    best = int(np.argmax(want))
    if c["winner_check"]:
        assert flags[best], (best, got[best], want[best], float(got.max()))
    else:  # beta < 0: the bad poses tie at alpha; every fp64 maximum must be in the band
        assert flags[want >= want[best] - 1e-9].all()
    assert np.abs(got[flags] - want[flags]).max() <= C.oracle_bound(c), np.abs(got[flags] - want[flags]).max()
    # 3. the winner
    if c["winner_check"]:
        assert int(np.argmax(got)) == best


@pytest.mark.parametrize("name", ["healthy-stream", "healthy-tiled"])
def test_a_camera_beyond_fp32_range_reads_at_most_four_cells_low(engine, name):
    """The limit DESIGN.md states, pinned.  A camera 1e10 m out sees the scene as one point; when that point falls inside the
    image (here pixel (372.5, 135)) the cells around it are true inliers -- fp64 score 0.137 -- but d2n zc^2 overflows fp32 and
    every cell reads maxReproj, which tests/test_gpu_edge.py::test_fast_score_of_a_hypothesis_far_beyond_the_scene pins.  The
    fp32 score may therefore be LOW, by no more than the true score of a point-like scene: the sum over the pixel lattice of
    1 / (1 + exp(beta (r - tau))), i.e. (pi tau^2 + pi^3 / (3 beta^2)) / sub^2 = 3.55 cells at these parameters plus the
    lattice's deviation from the integral -- 4 cells' weight, 0.156, inside the margin of 0.178 and 1.75 x margin / 2.  Every
    other hypothesis keeps the bar of margin / 2."""
    c = C.get(name)
    hyps, k = C.in_image_far_camera(c)
    from tests import rank_score_ref as ref
    want = ref.scores(c["coords"], c["assign"], hyps, c["focal"], c["ppx"], c["ppy"], c["sub"], (0, 0), c["alpha"], c["beta"], c["tau"], c["max_reproj"])
    cell, M = c["alpha"] / (c["H"] * c["W"]), C.margin(c)
    assert 2 * cell < want[k] <= 4 * cell < M  # the case is what it says: a few true inliers
    sc, hat = torch.from_numpy(c["coords"].copy()).cuda(), torch.from_numpy(c["assign"].copy()).cuda()
    engine.forward_device(sc, hat, _params(engine, c, max_tries=4))
    engine.write_hyps(hyps)
    p_tight = _params(engine, c, rescore_margin=1e-30)
    engine.score(sc, hat, p_tight)
    engine.select(sc, hat, p_tight)
    got = engine.read(api.BUF_SCORES).copy()
    flags = engine.read(api.BUF_EXACT_FLAGS).astype(bool)
    print("far camera in the image, %s: fp32 %.4g, fp64 %.4g = %.2f cells" % (name, got[k], want[k], want[k] / cell))
    assert not flags[k] and 0.0 <= want[k] - got[k] <= 4 * cell, (got[k], want[k])
    rest = ~flags
    rest[k] = False
    assert np.abs(got[rest] - want[rest]).max() <= M / 2


def _far_mid_nan_frame():
    """The far map with a NaN middle cell in the true expert's map, and its twin with 1e30 there: what the oracle is run on (the
    reference turns a NaN cell into NaN scores; the default route scores it as the outlier the 1e30 cell is,
    tests/test_gpu_edge.py::test_non_finite_scene_coordinates)."""
    c = C.get("far_mid_nan-stream")
    twin = c["coords"].copy()
    assert np.isnan(twin[c["poisoned"], :, c["H"] >> 1, c["W"] >> 1]).all()
    twin[c["poisoned"], :, c["H"] >> 1, c["W"] >> 1] = (1e30, -1e30, 1e30)
    rng = np.random.default_rng(77)
    ha = np.where(rng.uniform(size=300) < 0.85, c["poisoned"], 1 - c["poisoned"]).astype(np.int64)
    kw = dict(focal=c["focal"], ppx=c["ppx"], ppy=c["ppy"], sub_sampling=c["sub"], seed=1305)
    return c, twin, ha, kw


def _oracle_on_the_device_hypotheses(oracle, twin, ha, hyps, **kw):
    """_check_full holds hypotheses, scores and the refined pose to absolute bars (1e-6, 1e-7, 1e-6) that are sized for a room at
    the world origin.  17,000 m out, both P3P solvers -- double, on the same float32 cells -- work on coordinates whose rounding
    is |FAR| / 6 m = 2900 times that of the room's, and a rotation difference d moves the translation t = -R * camera by
    d * 17,000 m.  So the device's hypotheses face the oracle's own in the map's frame (rvec; t + R * FAR: the translation the
    same room at the origin would have: at 1e-6 * 2900, the rotation vector at 1e-5); the sampled cells and accepted tries stay bit-exact, and scores, winner,
    refinement trace and pose face the oracle run ON THE DEVICE'S HYPOTHESES (in_hyps) at _check_full's own bars."""
    from tests import rank_score_ref as ref
    own = oracle.forward(twin, ha, **kw)

    def local(h):
        return np.array([np.concatenate([x[:3], x[3:] + ref.rodrigues(x[:3]) @ C.FAR]) for x in h])
    ok = own["tries"] >= 0  # (an exhausted budget leaves the zero pose on both sides)
    np.testing.assert_array_equal(hyps[~ok], own["hyps"][~ok])
    np.testing.assert_allclose(local(hyps[ok])[:, 3:], local(own["hyps"][ok])[:, 3:], rtol=0, atol=1e-6 * np.linalg.norm(C.FAR) / 6.0)
    # (the rotation has no lever arm: 1e-5 rad, ten times _check_full's bar and 25 times the 4e-7 rad the two solvers were seen
    # to differ by on this map -- an origin mishandled by the sampler would not hide behind the translation's bar)
    np.testing.assert_allclose(hyps[ok][:, :3], own["hyps"][ok][:, :3], rtol=0, atol=1e-5)
    same = oracle.forward(twin, ha, in_hyps=hyps, **kw)
    same["tries"], same["sample_xy"], same["hyps"] = own["tries"], own["sample_xy"], hyps
    return same


def test_whole_call_on_a_far_map_with_a_nan_middle_cell(engine, oracle):
    """forward_device, E = 2, N = 300 (the speculative route: k_sample_decide forms the fp32 pose rows through the same origin,
    k_score_stragglers scores through it): every stage against the oracle."""
    c, twin, ha, kw = _far_mid_nan_frame()
    p = engine.make_params(c["E"], c["H"], c["W"], 300, call=21, **kw)
    res = engine.forward_device(torch.from_numpy(c["coords"].copy()).cuda(), torch.from_numpy(ha).cuda(), p)
    ref = _oracle_on_the_device_hypotheses(oracle, twin, ha, engine.read(api.BUF_HYPS), call=21, **kw)
    _check_full(engine, res, ref)


class _BatchFrame:
    """Frame b of the last batched call behind the `read` that _check_full uses.  The library keeps no per-frame exact flags and
    one inlier map: a score counts as flagged when it IS the oracle's -- which makes _check_full's comparison of the FLAGGED
    scores true by construction; what it still holds is the fp32 bar on every other score and that the winner is flagged -- and
    the inlier map is that of the single call with the same key, whose record this frame's must equal."""

    def __init__(self, engine, b, B, scores, ref, single_map):
        self.e, self.b, self.B, self.scores, self.ref, self.map = engine, b, B, scores, ref, single_map

    def read(self, which):
        if which == api.BUF_SCORES:
            return self.scores
        if which == api.BUF_EXACT_FLAGS:
            return (np.abs(self.scores - self.ref["scores"]) <= EXACT_SCORE_TOL * 100).astype(np.uint8)
        if which == api.BUF_INLIER_MAP:
            return self.map
        return self.e.read_forward_frames(which, self.B)[self.b]


def test_batched_call_on_a_far_map_with_a_nan_middle_cell(engine, oracle):
    """The same frame twice through forward_batch (frame b: key call + b): every stage against the oracle.
    Key 40 samples a garbage pose -- hypothesis 73, score 4.0 -- whose camera plane cuts through the room: dozens of cells at
    |z| < 0.01 m, ill-conditioned projections, fp32 score 2.3e-3 from the exact one (measured on the device, reproduced by an
    fp32 emulation on the CPU).  That is the class _check_full tolerates on 1 hypothesis in 4096, an allowance that rounds to
    none at N = 300: it is counted here instead -- at most ONE hypothesis per frame beyond FAST_SCORE_TOL, by no more than two
    cells' weight (what the band carries) -- and handed to _check_full with the oracle's score in its place."""
    c, twin, ha, kw = _far_mid_nan_frame()
    B, N, KEY = 2, 300, 40
    sc1, ha1 = torch.from_numpy(c["coords"].copy()).cuda(), torch.from_numpy(ha).cuda()
    singles = []
    for b in range(B):
        r1 = engine.forward_device(sc1, ha1, engine.make_params(c["E"], c["H"], c["W"], N, call=KEY + b, **kw))
        singles.append((r1, engine.read(api.BUF_INLIER_MAP).copy()))
    scores = torch.empty(B, N, dtype=torch.float64, device="cuda")
    res = engine.forward_batch(torch.stack([sc1, sc1]), torch.stack([ha1, ha1]), engine.make_params(c["E"], c["H"], c["W"], N, call=KEY, **kw),
                               scores_out=scores)
    sc_host = scores.cpu().numpy()
    for b in range(B):
        ref = _oracle_on_the_device_hypotheses(oracle, twin, ha, engine.read_forward_frames(api.BUF_HYPS, B)[b], call=KEY + b, **kw)
        discrete = [api.RES_HYP, api.RES_EXPERT, api.RES_REF_STEPS, api.RES_INLIERS]
        np.testing.assert_array_equal(res[b][discrete], singles[b][0][discrete])
        d = np.abs(sc_host[b] - ref["scores"])
        off = d > FAST_SCORE_TOL
        print("batch frame %d: %d hypotheses beyond FAST_SCORE_TOL %s" % (b, int(off.sum()), [(int(i), float(d[i])) for i in np.nonzero(off)[0]]))
        assert off.sum() <= 1 and (d[off] <= 2 * c["alpha"] / (c["H"] * c["W"])).all(), (int(off.sum()), float(d.max()))
        _check_full(_BatchFrame(engine, b, B, np.where(off, ref["scores"], sc_host[b]), ref, singles[b][1]), res[b], ref)
