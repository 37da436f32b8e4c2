"""The refinement's `err < tau` decision on maps whose cells sit ON the threshold (tests/tau_band_cases.py), against the
oracle -- the reference's float arithmetic, pinned bit for bit by tests/test_oracle_vs_ref.py.  On these maps a device that
decided by the fp64 comparison alone gets tens to hundreds of cells per frame wrong (tests/test_tau_band_cases_host.py counts
them), so the third screen -- the bit-exact project_exact_err sequence -- is what every comparison here exercises.

Bit-exact claims are made only where both sides evaluate the same pose bits (the hypothesis is WRITTEN: esac_hip_write_hyps,
then score_exact and refine, as tests/test_gpu_ref_golden.py does), where a CPU condition shows the fixture insensitive to
the 1e-9 by which two re-fits differ (the second pass), or on cells filtered for stability (the sampled-hypothesis fixtures
at the end: training slots, batches, the headline route kernel)."""
import numpy as np
import pytest
import torch

from esac_amd import api
from tests import tau_band_cases as T

pytestmark = pytest.mark.gpu


def _members(P, asked):
    """Members of the team set_refine_team(asked) gives a P-cell grid (esac_refine_team.hip: refine_team_members, explicit size)."""
    G = min((P + 255) // 256, asked, 32)
    return max(G, (P + 1023) // 1024, 2)


def _teams(name):
    p = T.case_params(name)
    seen = {}
    for asked in (4, 8, 10, 16, 32):
        seen.setdefault(_members(p["H"] * p["W"], asked), asked)
    return [dict(team=asked, members=m) for m, asked in sorted(seen.items())]


SOLO = dict(refine_solo=True)
# (case, route): every route a case is for
FIRST_PASS = (
    [("solo_scalar", {}), ("solo_scalar", SOLO), ("solo_vec", {}), ("solo_vec", SOLO), ("solo_vec", dict(strict_reference=True)),
     ("solo_global_list", SOLO), ("coop", dict(expect="cooperating")), ("wide_pixels", {})]
    + [(n, r) for n in ("team_min", "team_60x80", "team_odd", "team_max") for r in _teams(n)]
    + [("team_60x80", dict(team=10, members=10, route=False)), ("team_60x80", dict(team=10, members=10, strict_reference=True))]
    + [(n, r) for n in ("far_origin", "shifted") for r in (SOLO, dict(team=8, members=5))]
    + [(n, SOLO) for n in ("tau_tiny", "clamp_at_tau", "all_in", "camera_plane")]
    + [(n, dict(team=8, members=4)) for n in ("tau_tiny_team", "clamp_at_tau_team", "all_in_team", "camera_plane_team")]
)


def _route_id(r):
    return "-".join("%s%s" % (k, "" if v is True else v) for k, v in r.items() if k != "members") or "default"


def _run(engine, case, max_ref_steps, team=None, members=None, route=True, expect=None, error_image=False, **flags):
    """Writes the case's hypothesis (and the decoy), scores exactly, refines; returns what the refinement left."""
    p = case["params"]
    sc = torch.from_numpy(case["coords"]).cuda()
    ha = torch.zeros(2, dtype=torch.int64, device="cuda")
    prm = engine.make_params(1, p["H"], p["W"], 2, shift_x=p["shift_x"], shift_y=p["shift_y"], focal=p["focal"], ppx=p["ppx"], ppy=p["ppy"],
                             sub_sampling=p["sub"], inlier_thresh=p["tau"], inlier_alpha=p["alpha"], inlier_beta=p["beta"],
                             max_reproj=p["max_reproj"], max_ref_steps=max_ref_steps, exact_scores=True, **flags)
    engine.set_refine_team(team if team is not None else api.REFINE_TEAM_DEFAULT)
    engine.set_refine_route(route)
    engine.set_debug(keep_error_image=error_image)
    try:
        engine.write_hyps(T.decoy(case["hyp"]))
        engine.score_exact(sc, ha, prm)
        engine.refine(sc, ha, prm)
        torch.cuda.synchronize()
        out = dict(res=engine.read(api.BUF_RESULT), imap=engine.read(api.BUF_INLIER_MAP), counts=engine.read(api.BUF_INLIER_COUNTS),
                   info=engine.refine_info())
        if error_image:
            out["errs"] = engine.read(api.BUF_WINNER_ERRS)
    finally:
        engine.set_refine_team(api.REFINE_TEAM_DEFAULT)
        engine.set_refine_route(True)
        engine.set_debug()
    info = out["info"]
    want = expect or ("team" if team is not None else "one_workgroup")
    assert info["mode"] == want and not info["timed_out"], info
    if members is not None:
        assert info["workgroups"] == members, info
    assert not info["route_kernel"]  # (the stage entry runs no selection in the team's prologue: the general kernel)
    assert int(out["res"][api.RES_HYP]) == 0
    return out


def _same_map(case, got, want):
    bad = np.flatnonzero(got.reshape(-1) != want.reshape(-1))
    assert bad.size == 0, "%d cells decided differently\n%s" % (bad.size, T.describe_cells(case, bad, got, want))


@pytest.mark.parametrize("name,route", FIRST_PASS, ids=["%s-%s" % (n, _route_id(r)) for n, r in FIRST_PASS])
def test_first_pass_is_the_references(engine, oracle, name, route):
    """One refinement step from the written pose: the inlier map, its count and the record's count are the oracle's.

    The two non-finite cells: the reference's std::min(NaN, maxReproj) keeps the NaN and `NaN < tau` is false -- never an
    inlier, ALSO where max_reproj < tau makes every finite cell one (all_in*).  The device documents the same for the
    refinement on the default and on the strict route (deviation table: "it can never be an inlier"), so the map is
    held to the oracle's there too."""
    case = T.build_case(name)
    ref = T.reference(oracle, name)
    out = _run(engine, case, 1, **route)
    _same_map(case, out["imap"], ref["inlier_map"])
    assert out["counts"][0] == ref["inlier_counts"][0] and out["counts"][1] == -1
    assert int(out["res"][api.RES_REF_STEPS]) == ref["ref_steps"] == 1
    assert int(out["res"][api.RES_INLIERS]) == ref["inlier_counts"][0]


@pytest.mark.parametrize("name", T.SECOND_PASS_CASES)
def test_second_pass_counts(engine, oracle, name):
    """Two steps: the count at the pose the first re-fit returned.  Safe to compare: no cell is within 1e-4 px of tau at that
    pose (tests/test_tau_band_cases_host.py), the two re-fits agree to ~1e-9."""
    case = T.build_case(name)
    ref = T.reference(oracle, name, 2)
    P = case["params"]["H"] * case["params"]["W"]
    route = dict(expect="cooperating") if name == "coop" else dict(team=8, members=_members(P, 8)) if 1024 <= P <= 32768 else {}
    out = _run(engine, case, 2, **route)
    np.testing.assert_array_equal(out["counts"][:3], ref["inlier_counts"][:3])
    assert int(out["res"][api.RES_REF_STEPS]) == ref["ref_steps"]


@pytest.mark.parametrize("name", ["solo_scalar", "solo_vec", "solo_global_list"])
def test_third_screen_error_bits(engine, oracle, name):
    """The error image of the written pose (no step: the only error pass is the first).  Where the fp64 error is within half
    the band of tau the stored float IS the reference's; elsewhere it lies on the reference's side of tau."""
    case = T.build_case(name)
    ref = T.reference(oracle, name)
    out = _run(engine, case, 0, error_image=True, refine_solo=True)
    tau = T.tau32(case["params"])
    got, want = out["errs"], ref["winner_errs"]
    with np.errstate(invalid="ignore"):
        close = np.abs(case["err64"] - tau) < case["band2"] / 2
    finite = np.isfinite(want)
    assert close.sum() >= case["tuned"].sum() // 2
    bad = np.flatnonzero((got.view(np.uint32) != want.view(np.uint32)) & close)
    assert bad.size == 0, "%d cells off the reference's bits\n%s" % (bad.size, T.describe_cells(case, bad, got, want))
    side = np.flatnonzero(((got < np.float32(tau)) != (want < np.float32(tau))) & finite & ~close)
    assert side.size == 0, "%d cells on the other side\n%s" % (side.size, T.describe_cells(case, side, got, want))


# ------------------------------------------------------------------------------------------ hypotheses the call samples
def _frame_params(engine, c, N, **kw):
    p = c["params"]
    return engine.make_params(1, p["H"], p["W"], N, focal=p["focal"], ppx=p["ppx"], ppy=p["ppy"], sub_sampling=p["sub"],
                              seed=T.SAMPLED_SEED, call=c["kw"]["call"], **kw)


@pytest.mark.parametrize("route", [True, False], ids=["route_kernel", "general_kernel"])
@pytest.mark.parametrize("frame,members", [(T.HEADLINE_FRAME, 10), (T.TEAM_FRAMES[0], 5)], ids=["60x80", "32x40"])
def test_headline_call_first_pass(engine, oracle, frame, members, route):
    """esac_hip_forward with exact scores on a frame whose sampled hypothesis 0 sits on the band (one hypothesis: it is the
    winner): the team kernel with the headline call's modes compiled in, and the general one.  60x80 is the headline call's
    own instantiation -- ten members, two cells per lane, the 16-wide exchange (k_refine_team_route<2, 16>); 32x40 gives five
    members with one cell per lane (<1, 8>).  One step: map and count of the first pass; then the whole trace."""
    from esac_amd import synthetic as S
    c = T.sampled_frame(oracle, *frame, N=4 if frame[2] == 32 else 1)
    sc, ha = torch.from_numpy(c["coords"]).cuda(), torch.zeros(1, dtype=torch.int64, device="cuda")
    engine.set_refine_route(route)
    try:
        res = engine.forward_device(sc, ha, _frame_params(engine, c, 1, exact_scores=True, max_ref_steps=1))
        info = engine.refine_info()
        imap, counts = engine.read(api.BUF_INLIER_MAP), engine.read(api.BUF_INLIER_COUNTS)
        full = engine.forward_device(sc, ha, _frame_params(engine, c, 1, exact_scores=True))
        full_counts = engine.read(api.BUF_INLIER_COUNTS)
    finally:
        engine.set_refine_route(True)
    assert info["mode"] == "team" and info["route_kernel"] == route and info["workgroups"] == members and not info["timed_out"], info
    # what the stability filter covers: +-1e-9 in one component at a time, so six differences of at most a sixth of that
    np.testing.assert_allclose(engine.read(api.BUF_HYPS), c["hyp"], rtol=0, atol=1e-9 / 6)
    _same_map(c, imap, c["first_map"])
    assert counts[0] == c["first_map"].sum() == int(res[api.RES_INLIERS]) and int(res[api.RES_REF_STEPS]) == 1
    ref = c["ref1"]  # every later pose is clear of the band (the host test): the whole trace
    np.testing.assert_array_equal(full_counts, ref["inlier_counts"])
    assert int(full[api.RES_REF_STEPS]) == ref["ref_steps"] and int(full[api.RES_LM_ITERS]) == ref["lm_iters"]
    r, t = S.pose_errors(full[api.RES_POSE:api.RES_POSE + 16].reshape(4, 4), ref["pose"])
    assert r <= 1e-4 and t <= 1e-3, (r, t)


@pytest.mark.parametrize("frames,mode", [(T.TEAM_FRAMES, "team"), (T.SMALL_FRAMES, "one_workgroup")], ids=["3x32x40", "33x12x16"])
def test_batches(engine, oracle, frames, mode):
    """forward_batch over frames that each sit on the band of their own sampled hypothesis (frame b samples with call + b):
    a team per frame, and one workgroup per frame beyond the batch size the teams take."""
    from esac_amd import synthetic as S
    cs = [T.sampled_frame(oracle, k, call, H, W, sub, N=4 if mode == "team" else 1) for k, call, H, W, sub in frames]
    B = len(cs)
    sc = torch.from_numpy(np.stack([c["coords"] for c in cs])).cuda()
    ha = torch.zeros((B, 1), dtype=torch.int64, device="cuda")
    recs = engine.forward_batch(sc, ha, _frame_params(engine, cs[0], 1))
    assert engine.refine_info()["mode"] == mode
    counts, tries, xy, hyps = (engine.read_forward_frames(w, B) for w in (api.BUF_INLIER_COUNTS, api.BUF_TRIES, api.BUF_SAMPLE_XY, api.BUF_HYPS))
    one = np.zeros(1, np.int64)
    worst = 0.0
    for b, c in enumerate(cs):
        ref = c["ref1"]
        np.testing.assert_array_equal(tries[b], ref["tries"], err_msg="frame %d" % b)
        np.testing.assert_array_equal(xy[b], ref["sample_xy"], err_msg="frame %d" % b)
        diff = float(np.abs(hyps[b][0] - c["hyp"][0]).max())
        worst = max(worst, diff)
        # the reference: the oracle from the DEVICE's hypothesis bits -- the same first pose on both sides, whatever the
        # sampled P3P's conditioning; the later poses are clear of the band (the host test)
        own = oracle.forward(c["coords"], one, in_hyps=hyps[b][:1], **c["kw"])
        assert counts[b][0] == own["inlier_counts"][0], "frame %d: first pass %d, reference %d" % (b, counts[b][0], own["inlier_counts"][0])
        # ... and the sampling oracle's own first pass: the device's hypothesis must lie inside what the stability filter covers
        # (+-1e-9 in one component at a time, so six differences of at most a sixth of that)
        assert diff <= 1e-9 / 6, "frame %d: sampled hypothesis 0 is %.2e from the oracle's" % (b, diff)
        assert counts[b][0] == c["first_map"].sum() == ref["inlier_counts"][0], b
        np.testing.assert_array_equal(counts[b], own["inlier_counts"], err_msg="frame %d" % b)
        rec = recs[b]
        assert int(rec[api.RES_HYP]) == 0 and int(rec[api.RES_REF_STEPS]) == own["ref_steps"] and int(rec[api.RES_LM_ITERS]) == own["lm_iters"], b
        assert int(rec[api.RES_INLIERS]) == own["inlier_counts"][own["ref_steps"] - 1], b
        r, t = S.pose_errors(rec[api.RES_POSE:api.RES_POSE + 16].reshape(4, 4), own["pose"])
        assert r <= 1e-4 and t <= 1e-3, (b, r, t)
    print("%d frames: sampled hypothesis 0, device against oracle, worst component difference %.2e" % (B, worst))


@pytest.mark.parametrize("teams", [True, False], ids=["slot_teams", "one_workgroup_per_slot"])
def test_training_slots_first_pass(oracle, monkeypatch, teams):
    """esac_hip_backward, one refinement step: every slot's accepted inlier map IS its first pass.  Slot 0 starts on the band
    (stability-filtered for it): its map and index work are those of the oracle's training call.  All four are held to the
    oracle's first pass from the device's own hypothesis bits.  By slot teams and by one workgroup per slot."""
    from tests import bwd_replay as R
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    if not teams:
        monkeypatch.setenv("ESAC_SLOT_TEAMS", "0")
    eng = api.Engine(0)  # a context of its own: the switch is read when the context is made
    c = T.sampled_frame(oracle, *T.TEAM_FRAMES[0])
    p, N = c["params"], 4
    gt = c["gt_pose"].astype(np.float32)
    gt[:3, 3] += np.float32(0.03)
    kw = dict(focal=p["focal"], ppx=p["ppx"], ppy=p["ppy"], sub_sampling=p["sub"], inlier_alpha=1.0, seed=T.SAMPLED_SEED, call=c["kw"]["call"],
              max_ref_steps=1)
    ref = oracle.backward(c["coords"], np.zeros_like(c["coords"]), c["ha"], gt, want_stages=True, **kw)
    sel = np.nonzero(ref["probs"] >= R.PROB_THRESH)[0]
    assert list(sel) == [0, 1, 2, 3] and np.array_equal(ref["maps"][0].reshape(c["first_map"].shape), c["first_map"])
    out = eng.backward_device(torch.from_numpy(c["coords"]).cuda(), torch.zeros(c["coords"].shape, device="cuda"), torch.from_numpy(c["ha"]).cuda(),
                              gt, 1.0, 100.0, 100.0, eng.make_params(1, p["H"], p["W"], N, **kw))
    case = dict(N=N, P=p["H"] * p["W"])
    stages, dev = R.device_stages(eng, api, case, out[1])
    assert eng.bwd_team_info()["teams"] == teams, eng.bwd_team_info()
    np.testing.assert_array_equal(dev["slots"], sel)
    np.testing.assert_array_equal(stages["sample_xy"], ref["sample_xy"])
    diff = np.abs(stages["init_hyps"] - ref["init_hyps"]).max(axis=1)
    print("sampled hypotheses, device against oracle, per slot:", diff)
    assert diff.max() <= 1e-6  # (the suite's bar on sampled hypotheses: tests/test_gpu_ragged.py)
    # Slot 0 is the one on the band, and stable under +-1e-9 per component: six differences of at most a sixth of that move no
    # decision (the error is linear in the pose at this scale), so the oracle's own slot 0 is the reference
    assert diff[0] <= 1e-9 / 6
    _same_map(c, stages["maps"][0], ref["maps"][0])
    assert tuple(dev["info"][0, 1:4]) == (ref["ref_inliers"][0], ref["ref_steps"][0], ref["ref_lm_iters"][0])
    # Every slot, 0 included, against the oracle's first pass from the DEVICE's hypothesis bits: the same pose on both sides.
    # (Slots 1-3 start 1e-5 .. 1e-3 rad from slot 0 -- their cells lie within ~1e-2 px of tau, unfiltered -- and a sampled
    # hypothesis can differ from the oracle's by 2e-9 where its P3P is ill-conditioned: measured on slot 3, where that moved a
    # cell 1.6e-6 px from tau across the float boundary.)
    one = np.zeros(1, np.int64)
    fkw = dict(kw)
    fkw.pop("inlier_alpha")
    # (so ref["maps"][1:], ref_inliers, ref_steps and ref_lm_iters of the oracle's TRAINING call are not compared for slots 1-3:
    # that call starts them from its own sample, 2e-9 away on slot 3; and with one step, "index work" is the first pass's count,
    # the one accepted step and its LM iterations)
    for s, h in enumerate(sel):
        own = oracle.forward(c["coords"], one, in_hyps=stages["init_hyps"][h:h + 1], **fkw)
        _same_map(c, stages["maps"][h], own["inlier_map"])
        assert tuple(dev["info"][s, 1:4]) == (own["inlier_counts"][0], own["ref_steps"], own["lm_iters"]), (h, dev["info"][s], own["inlier_counts"][:2])
    np.testing.assert_array_equal(dev["info"][:, 0] >= 0, ref["have_map"][sel] != 0)
