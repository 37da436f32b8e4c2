"""The front route (k_sample_route, k_rescore_route: the headline call's modes compiled in, no fp32 pose rows stored --
esac_amd/csrc/esac_front_route.hip) against the general kernels (k_sample<256, 2>, k_rescore<1024>): the same call twice on one
engine, once with the route kernels and once with set_front_route(False), compared byte for byte in everything the two kernels
write -- hyps, the rotation matrices, sample_xy, tries, the score vector (workspace and the caller's) -- and in the record the
refinement makes of them.  The reference is always the general kernels of the same build, never a recording.

Each case asserts through front_route_taken() that the kernels it means to run did run."""
import numpy as np
import pytest
import torch

from esac_amd import api
from esac_amd import synthetic as S

pytestmark = pytest.mark.gpu

SEED = 1320
BUFFERS = {"hyps": api.BUF_HYPS, "sample_xy": api.BUF_SAMPLE_XY, "tries": api.BUF_TRIES, "scores": api.BUF_SCORES}


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a.view(np.uint32) if a.dtype == np.float32 else a


def _params(engine, f, N, k=0, **kw):
    E, _, H, W = f["coords"].shape
    kw.setdefault("exact_scores", "auto")  # esac.forward's default flags (ESAC_FLAG_AUTO_EXACT)
    return engine.make_params(E, H, W, N, shift_x=f["shift"][0], shift_y=f["shift"][1], focal=f["focal"], ppx=f["ppx"], ppy=f["ppy"],
                              sub_sampling=f["sub"], seed=SEED, call=k, **kw)


def _call(engine, f, ha, front, k=0, after=None, **kw):
    """One esac_hip_forward; everything the sampler and the scorer leave behind, and the record.  after(engine, sc, ha): stage
    calls to run behind it on the same context, before the buffers are read."""
    p = _params(engine, f, len(ha), k, **kw)
    scores_out = torch.full((len(ha),), -7.0, dtype=torch.float64, device="cuda")
    sc, had = torch.from_numpy(f["coords"]).cuda(), torch.from_numpy(ha).cuda()
    engine.set_front_route(front)
    try:
        res = engine.forward_device(sc, had, p, scores_out=scores_out)
        taken = engine.front_route_taken()
        if after is not None:
            after(engine, sc, had)
        out = {name: np.array(engine.read(buf)) for name, buf in BUFFERS.items()}
        out["hyps_R"] = engine.read_rotations(len(ha))
        out["exact_flags"] = np.array(engine.read(api.BUF_EXACT_FLAGS))
        out["record"] = np.array(res[:32], dtype=np.float64)
        out["scores_out"] = scores_out.cpu().numpy()
    finally:
        engine.set_front_route(True)
    return out, taken


def _both(engine, f, ha, expect_route=True, **kw):
    """The call on the route kernels and on the general kernels: identical bytes; returns the route run's outputs."""
    a, taken_a = _call(engine, f, ha, True, **kw)
    b, taken_b = _call(engine, f, ha, False, **kw)
    assert taken_a == expect_route and not taken_b, (taken_a, taken_b)
    for name in a:
        np.testing.assert_array_equal(_bits(a[name]), _bits(b[name]), err_msg=name)
    assert (a["scores_out"] != -7.0).all()
    np.testing.assert_array_equal(_bits(a["scores_out"]), _bits(a["scores"]))
    return a


def _frame(N, k=0, E=1, **frame):
    f = S.make_frame(k, E=E, **frame)
    return f, S.gating_assignment(f, N)


def test_headline_call(engine):
    """60x80, 256 hypotheses: k_sample_route<256, 2> and k_rescore_route<1024, 5> -- lanes with five cells and lanes with four."""
    out = _both(engine, *_frame(256))
    assert (out["tries"] >= 0).all() and (out["exact_flags"] == 1).all()


@pytest.mark.parametrize("N", [1, 5])
def test_few_hypotheses(engine, N):
    _both(engine, *_frame(N))


@pytest.mark.parametrize("H,W,N", [(13, 17, 64),      # W % 4 != 0, fewer cells (221) than the scorer has lanes
                                   (33, 32, 64),      # 1056 cells: lanes with two cells and lanes with one
                                   (64, 128, 256)],   # N * H * W = 2^21, the edge of eligibility: eight cells per lane
                         ids=["13x17", "33x32", "64x128"])
def test_grids(engine, H, W, N):
    _both(engine, *_frame(N, H=H, W=W))


def test_non_finite_scene_coordinates(engine):
    f, ha = _frame(256, k=1)
    c = f["coords"]
    c[0, 0, 3, 5] = np.nan
    c[0, 1, 17, 40] = np.inf
    c[0, 2, 30, 79] = -np.inf
    c[0, :, 59, 0] = np.nan
    c[0, :, 30, 40] = np.nan  # the middle cell: the probe of the fp32 rows' origin, which the route sampler never reads
    out = _both(engine, f, ha, k=1)
    assert np.isfinite(out["scores"]).all()  # such a cell is an outlier at maxReproj


def test_shifted_image(engine):
    """Non-zero shift_x / shift_y: the pixel positions of the cells, in the sampler and in the scorer."""
    _both(engine, *_frame(256, k=2, shift=(12, -7)), k=2)


def test_sampler_second_round(engine):
    """60 % outliers (tests/headline_bits_cases.py: second_round_k0): hypotheses that go past the shared round of 128 tries."""
    out = _both(engine, *_frame(256, outlier_frac=0.6))
    assert int((out["tries"] >= 128).sum()) >= 1


def test_exhausted_budget(engine):
    """max_tries = 8: hypotheses whose budget runs out keep the state of their last try (tries = -1)."""
    out = _both(engine, *_frame(256, outlier_frac=0.6), max_tries=8)
    assert int((out["tries"] == -1).sum()) >= 1 and int((out["tries"] >= 0).sum()) >= 1


def test_fp32_rows_are_rebuilt_for_the_next_stage(engine):
    """A route call stores no fp32 pose rows; esac_hip_score on the same context rebuilds them (k_hyps_to_rt32) before it streams.
    The fp32 scores -- read where esac_hip_select leaves them, as doubles, for every hypothesis outside the band -- are the bytes
    the same sequence gives with the sampler's own rows."""
    f, ha = _frame(256)

    def stages(engine, sc, had):
        p = _params(engine, f, len(ha), exact_scores=False)
        engine.score(sc, had, p)
        engine.select(sc, had, p)

    a, taken_a = _call(engine, f, ha, True, after=stages)
    b, taken_b = _call(engine, f, ha, False, after=stages)
    assert taken_a and not taken_b
    assert int((a["exact_flags"] == 0).sum()) >= 128  # most scores are the stream's fp32 values
    for name in ("scores", "exact_flags", "hyps", "hyps_R"):
        np.testing.assert_array_equal(_bits(a[name]), _bits(b[name]), err_msg=name)


def test_two_experts_run_the_general_kernels(engine):
    f, ha = _frame(64, E=2)
    _both(engine, f, ha, expect_route=False, exact_scores=True)


def test_257_hypotheses_run_the_general_kernels(engine):
    _both(engine, *_frame(257), expect_route=False)


def test_strict_reference_runs_the_general_kernels(engine):
    _both(engine, *_frame(64), expect_route=False, exact_scores=False, strict_reference=True)


def _batch(engine, f, ha, B, front, cams=None):
    p = _params(engine, f, ha.shape[-1], exact_scores=True)
    sc = torch.from_numpy(np.stack([f["coords"]] * B)).cuda()
    had = torch.from_numpy(np.stack([ha] * B)).cuda()
    engine.set_front_route(front)
    try:
        res = engine.forward_batch(sc, had, p, cams=cams)
        return np.array(res), engine.front_route_taken(), np.array(engine.read(api.BUF_SCORES))
    finally:
        engine.set_front_route(True)


def test_a_batch_of_two_runs_the_general_kernels(engine):
    f, ha = _frame(64)
    a, b = _batch(engine, f, ha, 2, True), _batch(engine, f, ha, 2, False)
    assert not a[1] and not b[1]
    np.testing.assert_array_equal(_bits(a[0][:, :32]), _bits(b[0][:, :32]))
    np.testing.assert_array_equal(_bits(a[2]), _bits(b[2]))


def test_a_camera_table_runs_the_general_kernels(engine):
    """One frame handed in with a table (esac_hip_forward_batch_cams, B = 1): the general kernels, whatever the record holds."""
    f, ha = _frame(64)
    cams = api.make_cams([f["shift"][0]], [f["shift"][1]], [f["focal"]], [f["ppx"]], [f["ppy"]])
    a, b = _batch(engine, f, ha, 1, True, cams), _batch(engine, f, ha, 1, False, cams)
    assert not a[1] and not b[1]
    np.testing.assert_array_equal(_bits(a[0][:, :32]), _bits(b[0][:, :32]))
    np.testing.assert_array_equal(_bits(a[2]), _bits(b[2]))
    plain, taken = _call(engine, f, ha, True, exact_scores=True)  # the same frame without a table takes the route: same scores
    assert taken
    np.testing.assert_array_equal(_bits(plain["scores"]), _bits(a[2]))
