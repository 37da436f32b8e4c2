"""GPU checks of the semantics around the hot path that the stage-wise parity tests do not reach: the softmax statistics
of the result record, batched / harness calls against the ORACLE (not against the HIP path itself), range checking of
device-resident assignments, pixel coordinates beyond 16 bits, workspace growth, rank-deficient re-fits."""
import numpy as np
import pytest
import torch

from esac_amd import api
from esac_amd import synthetic as S
from tests.test_gpu_parity import _check_full, _run_both

pytestmark = pytest.mark.gpu


def _kw(f):
    return dict(shift_x=f["shift"][0], shift_y=f["shift"][1], focal=f["focal"], ppx=f["ppx"], ppy=f["ppy"], sub_sampling=f["sub"])


@pytest.mark.parametrize("alpha", [100.0, 10.0])
def test_selection_probability_and_entropy_against_the_oracle(engine, oracle, alpha):
    """softMax / entropy (esac_util.h:461-497).  Default path: statistics of the fp32 score stream -- scores within
    2e-5*alpha of the reference arithmetic, so probability within 1e-2 relative, entropy within 1e-2 bit (stated
    tolerances).  ESAC_FLAG_EXACT_SCORES: the reference's own values for every hypothesis."""
    f = S.make_frame(31, E=3, true_expert=1)
    ha = S.gating_assignment(f, 192, mode="gating")
    sc, hat = torch.from_numpy(f["coords"]).cuda(), torch.from_numpy(ha).cuda()
    ref = oracle.forward(f["coords"], ha, seed=9, call=4, inlier_alpha=alpha, **_kw(f))
    p = engine.make_params(3, 60, 80, 192, seed=9, call=4, inlier_alpha=alpha, **_kw(f))
    res = engine.forward_device(sc, hat, p)
    assert int(res[api.RES_HYP]) == ref["winner"]
    assert abs(res[api.RES_PROB] - ref["probs"][ref["winner"]]) <= 1e-2 * ref["probs"][ref["winner"]]
    assert abs(res[api.RES_ENTROPY] - ref["entropy"]) <= 1e-2
    q = engine.make_params(3, 60, 80, 192, seed=9, call=4, inlier_alpha=alpha, exact_scores=True, **_kw(f))
    scores = torch.empty(192, dtype=torch.float64, device="cuda")
    rex = engine.forward_device(sc, hat, q, scores_out=scores)
    np.testing.assert_allclose(scores.cpu().numpy(), ref["scores"], rtol=1e-12, atol=1e-11)  # every hypothesis, reference arithmetic
    np.testing.assert_allclose(engine.read(api.BUF_SCORES), ref["scores"], rtol=1e-12, atol=1e-11)
    assert engine.read(api.BUF_EXACT_FLAGS).all() and int(rex[api.RES_CONTENDERS]) == 192
    np.testing.assert_allclose(rex[api.RES_PROB], ref["probs"][ref["winner"]], rtol=1e-10)
    np.testing.assert_allclose(rex[api.RES_ENTROPY], ref["entropy"], rtol=1e-10, atol=1e-12)
    # the pose does not depend on the route
    np.testing.assert_array_equal(rex[api.RES_HYP:api.RES_PROB], res[api.RES_HYP:api.RES_PROB])
    # module level
    import esac
    esac.set_seed(9, 4)
    esac.set_exact_scores(True)
    try:
        out_pose = torch.zeros(4, 4)
        esac.forward(sc, hat, out_pose, f["shift"][0], f["shift"][1], f["focal"], f["ppx"], f["ppy"], 10.0, alpha, 0.5, 100.0, f["sub"])
        np.testing.assert_allclose(esac.last_result()["scores"].cpu().numpy(), ref["scores"], rtol=1e-12, atol=1e-11)
    finally:
        esac.set_exact_scores(False)


def test_batched_forward_against_the_oracle(engine, oracle):
    """esac_hip_forward_batch frame b vs the ORACLE's forward with the key (seed, call + b): winner, expert, refinement
    trace and pose, every frame."""
    B, N = 10, 160
    frames = [S.make_frame(400 + b, E=3, true_expert=b % 3) for b in range(B)]
    assigns = np.stack([S.gating_assignment(f, N, mode="gating") for f in frames])
    coords = torch.from_numpy(np.stack([f["coords"] for f in frames])).cuda()
    p = engine.make_params(3, 60, 80, N, seed=21, call=100)
    scores = torch.empty(B, N, dtype=torch.float64, device="cuda")
    res = engine.forward_batch(coords, torch.from_numpy(assigns).cuda(), p, scores_out=scores)
    sc_host = scores.cpu().numpy()
    for b in range(B):
        ref = oracle.forward(frames[b]["coords"], assigns[b], seed=21, call=100 + b)
        assert int(res[b][api.RES_HYP]) == ref["winner"] and int(res[b][api.RES_EXPERT]) == ref["expert"], b
        assert int(res[b][api.RES_REF_STEPS]) == ref["ref_steps"] and int(res[b][api.RES_LM_ITERS]) == ref["lm_iters"], b
        assert abs(res[b][api.RES_SCORE] - ref["scores"][ref["winner"]]) <= 1e-9
        assert np.abs(sc_host[b] - ref["scores"]).max() <= 2e-3
        np.testing.assert_allclose(res[b][api.RES_RVEC:api.RES_RVEC + 6], ref["refined"], rtol=0, atol=1e-6)
        r, t = S.pose_errors(res[b][api.RES_POSE:api.RES_POSE + 16].reshape(4, 4), ref["pose"])
        assert r <= 1e-4 and t <= 1e-3, (b, r, t)


def test_batched_multi_expert_frames_beyond_the_first_pass_limit(engine, oracle):
    """24 frames x 400 hypotheses on 3 experts = 9600 hypotheses in one launch set: beyond 8192 the screened chain starts
    at try 0 (no first pass: esac_kernels.hip, launch_sample) and runs per frame (pending list entries carry the frame,
    RNG key call + b) -- every frame against the oracle: winner, expert, exact winner score, refinement trace, the whole
    score vector within the fp32 stream's band (a hypothesis sampled at another try would score differently)."""
    B, N = 24, 400
    frames = [S.make_frame(430 + b, E=3, true_expert=(2 * b) % 3) for b in range(B)]
    assigns = np.stack([S.gating_assignment(f, N, mode="gating") for f in frames])
    assigns[:, ::9] = (assigns[:, ::9] + 1) % 3  # a good share of wrong-expert stragglers in every frame
    coords = torch.from_numpy(np.stack([f["coords"] for f in frames])).cuda()
    p = engine.make_params(3, 60, 80, N, seed=33, call=700)
    scores = torch.empty(B, N, dtype=torch.float64, device="cuda")
    res = engine.forward_batch(coords, torch.from_numpy(assigns).cuda(), p, scores_out=scores)
    sc_host = scores.cpu().numpy()
    for b in range(B):
        ref = oracle.forward(frames[b]["coords"], assigns[b], seed=33, call=700 + b)
        assert int(res[b][api.RES_HYP]) == ref["winner"] and int(res[b][api.RES_EXPERT]) == ref["expert"], b
        assert int(res[b][api.RES_REF_STEPS]) == ref["ref_steps"] and int(res[b][api.RES_LM_ITERS]) == ref["lm_iters"], b
        assert abs(res[b][api.RES_SCORE] - ref["scores"][ref["winner"]]) <= 1e-9
        assert np.sort(np.abs(sc_host[b] - ref["scores"]))[-2] <= 2e-3 and np.abs(sc_host[b] - ref["scores"]).max() <= 5e-2, b
        r, t = S.pose_errors(res[b][api.RES_POSE:api.RES_POSE + 16].reshape(4, 4), ref["pose"])
        assert r <= 1e-4 and t <= 1e-3, (b, r, t)


def test_harness_localize_against_the_oracle(oracle):
    """esac_amd/harness.py:localize (the reference's test loop, test_esac.py:145-207) vs the oracle on the very tensors
    it handed to esac.forward, same (seed, call)."""
    import esac
    from esac_amd import harness
    E = 4
    gen = torch.Generator(device="cuda").manual_seed(11)
    for k in range(4):
        f = S.make_frame(500 + k, E=E, true_expert=k % E)
        coords = torch.from_numpy(f["coords"]).cuda()
        logits = torch.full((1, E), -3.0, device="cuda")
        logits[0, k % E] = 3.0
        gating = lambda image, lg=torch.log_softmax(logits, dim=1): lg
        experts = [lambda image, e=e: coords[e:e + 1] for e in range(E)]
        esac.set_seed(77, 10 + k)
        out = harness.localize(torch.zeros(1, 3, 480, 640, device="cuda"), gating, experts, f["focal"], hypotheses=128, generator=gen)
        ref = oracle.forward(out["prediction"].cpu().numpy(), out["hyp_assignment"].cpu().numpy().copy(), seed=77, call=10 + k,
                             focal=f["focal"], ppx=320.0, ppy=240.0, sub_sampling=8)
        assert out["expert"] == ref["expert"] and esac.last_result()["winner"] == ref["winner"]
        r, t = S.pose_errors(out["pose"].numpy(), ref["pose"])
        assert r <= 1e-4 and t <= 1e-3, (k, r, t)


def test_device_resident_assignment_is_range_checked(engine):
    """A hypAssignment value outside [0,E): CPU tensors are rejected on the host; a DEVICE tensor reaches the kernels,
    which never read outside the maps (expert 0 instead) and flag it -- the blocking call raises."""
    import esac
    f = S.make_frame(40, E=3, true_expert=0)
    sc = torch.from_numpy(f["coords"]).cuda()
    for bad in (3, -1, 2**40):
        ha = np.zeros(64, np.int64)
        ha[17] = bad
        args = (0, 0, f["focal"], f["ppx"], f["ppy"], 10.0, 100.0, 0.5, 100.0, f["sub"])
        with pytest.raises(RuntimeError, match="hypAssignment"):
            esac.forward(sc, torch.from_numpy(ha), torch.zeros(4, 4), *args)          # host check
        with pytest.raises(RuntimeError, match="hypAssignment"):
            esac.forward(sc, torch.from_numpy(ha).cuda(), torch.zeros(4, 4), *args)   # device check
        with pytest.raises(RuntimeError, match="hypAssignment"):
            esac.backward(sc, torch.zeros_like(sc), torch.from_numpy(ha).cuda(), torch.eye(4), 1.0, 100.0, 100.0, *args)
        # asynchronous call: reported by esac_hip_check
        p = engine.make_params(3, 60, 80, 64)
        engine.forward_device(sc, torch.from_numpy(ha).cuda(), p, want_host=False)
        with pytest.raises(RuntimeError, match="hypAssignment"):
            engine.check()
    # and a clean call afterwards is clean
    ha = torch.zeros(64, dtype=torch.int64).cuda()
    esac.forward(sc, ha, torch.zeros(4, 4), *args)
    engine.forward_device(sc, ha, engine.make_params(3, 60, 80, 64), want_host=False)
    engine.check()


def test_single_expert_ignores_assignment_values_consistently(engine, oracle):
    """E == 1: every kernel (forward and backward) uses expert 0 whatever hypAssignment holds."""
    f = S.make_frame(41)
    sc = torch.from_numpy(f["coords"]).cuda()
    gt = f["gt_pose"].astype(np.float32)
    outs = []
    for val in (0, 5):
        ha = torch.full((48,), val, dtype=torch.int64).cuda()
        g = torch.zeros_like(sc)
        o = engine.backward_device(sc, g, ha, gt, 1.0, 100.0, 100.0, engine.make_params(1, 60, 80, 48, seed=2, call=7))
        outs.append((o[0], g.cpu().numpy()))
    assert outs[0][0] == outs[1][0] and np.array_equal(outs[0][1], outs[1][1]) and np.abs(outs[0][1]).max() > 0


def test_pixel_coordinates_beyond_16_bits(engine, oracle):
    """createSampling positions col*sub + sub/2 - shift (esac_util.h:64-66) have no 16-bit limit in the reference: a
    gigapixel-style camera (sub-sampling 4000) must refine with the true pixel positions."""
    f = S.make_frame(42, H=18, W=24, sub=4000, focal=52500.0, ppx=48000.0, ppy=36000.0, shift=(-70000, 1234))
    ha = S.gating_assignment(f, 64)
    sc, hat = torch.from_numpy(f["coords"]).cuda(), torch.from_numpy(ha).cuda()
    kw = dict(inlier_thresh=1000.0, inlier_beta=0.005, max_reproj=10000.0, **_kw(f))
    p = engine.make_params(1, 18, 24, 64, seed=4, call=2, **kw)
    res = engine.forward_device(sc, hat, p)
    ref = oracle.forward(f["coords"], ha, seed=4, call=2, **kw)
    assert ref["ref_steps"] >= 1
    assert int(res[api.RES_HYP]) == ref["winner"] and int(res[api.RES_REF_STEPS]) == ref["ref_steps"]
    np.testing.assert_array_equal(engine.read(api.BUF_INLIER_COUNTS), ref["inlier_counts"])
    np.testing.assert_allclose(res[api.RES_RVEC:api.RES_RVEC + 6], ref["refined"], rtol=0, atol=1e-6)
    # positions that do not fit int32 are rejected, not wrapped
    with pytest.raises(RuntimeError, match="int32"):
        engine.forward_device(sc, hat, engine.make_params(1, 18, 24, 64, sub_sampling=2**30))


def test_written_hypotheses_survive_workspace_growth(oracle):
    """esac_hip_write_hyps followed by a stage call that has to grow the workspace (larger grid than ever seen by this
    context) still scores the written hypotheses."""
    eng = api.Engine(0)  # fresh context: empty workspace
    f = S.make_frame(43, H=120, W=160, sub=4)
    ha = S.gating_assignment(f, 32)
    ref = oracle.forward(f["coords"], ha, seed=1, call=1, **_kw(f))
    eng.write_hyps(ref["hyps"])
    p = eng.make_params(1, 120, 160, 32, **_kw(f))
    eng.score_exact(torch.from_numpy(f["coords"]).cuda(), torch.from_numpy(ha).cuda(), p)
    np.testing.assert_allclose(eng.read(api.BUF_SCORES), ref["scores"], rtol=1e-12, atol=1e-11)


def _collinear_scene(noise):
    """24x32 grid, sub 20: the cells of image row 12 hold scene points on ONE 3D line (each projecting exactly to its
    cell centre under the ground-truth pose), every other cell holds a point far outside the image."""
    H, W, sub, focal, ppx, ppy = 24, 32, 20, 525.0, 320.0, 240.0
    rng = np.random.default_rng(5)
    f = S.make_frame(44, H=H, W=W, sub=sub)
    Rc2s, cam = f["gt_pose"][:3, :3], f["gt_pose"][:3, 3]
    coords = np.zeros((1, 3, H, W), np.float32)
    far = cam + Rc2s @ np.array([50.0, 40.0, 1.0])  # projects ~26,000 px off the image
    coords[0] = far.astype(np.float32)[:, None, None]
    row = 12
    y0 = (row * sub + sub // 2 - ppy) / focal
    z0, k = 2.5, 0.8
    for col in range(W):
        x0 = (col * sub + sub // 2 - ppx) / focal
        z = z0 / (1.0 - k * x0)
        pc = np.array([x0 * z, y0 * z, z]) + rng.normal(0.0, noise, 3)
        coords[0, :, row, col] = (cam + Rc2s @ pc).astype(np.float32)
    R = Rc2s.T
    t = -R @ cam
    return f, coords, R, t, (H, W, sub)


@pytest.mark.parametrize("noise", [0.0, 0.003])
def test_rank_deficient_refit_follows_the_svd_route(engine, oracle, noise):
    """Forward refinement on a COLLINEAR inlier set (J^T J of rank 5): CvLevMarq solves its damped normal equations by
    SVD (min-norm step in the unconstrained direction); the device's LDL^T must hand over to the same pseudo-inverse
    instead of taking a zero step.  The hypothesis is placed by hand near the ground truth (sampling cannot produce one
    from a collinear map); scoring, selection and refinement are compared with the oracle."""
    f, coords, R, t, (H, W, sub) = _collinear_scene(noise)
    rvec = oracle.rodrigues_mat2vec(R)
    hyps = np.tile(np.concatenate([rvec, t]), (4, 1))
    hyps[0] += np.array([2e-3, -1e-3, 1.5e-3, 4e-3, -2e-3, 3e-3])  # the best one: the others are worse copies
    hyps[1:] += np.array([3e-2, 2e-2, -2e-2, 0.05, 0.04, -0.03])
    ha = np.zeros(4, np.int64)
    kw = dict(focal=525.0, ppx=320.0, ppy=240.0, sub_sampling=sub)
    ref = oracle.forward(coords, ha, in_hyps=hyps, **kw)
    assert ref["winner"] == 0 and ref["ref_steps"] >= 1 and ref["inlier_counts"][0] == W
    sc, hat = torch.from_numpy(coords).cuda(), torch.from_numpy(ha).cuda()
    p = engine.make_params(1, H, W, 4, **kw)
    engine.write_hyps(hyps)
    engine.score_exact(sc, hat, p)
    engine.refine(sc, hat, p)
    res = engine.read(api.BUF_RESULT)
    assert int(res[api.RES_HYP]) == 0 and int(res[api.RES_REF_STEPS]) == ref["ref_steps"]
    np.testing.assert_array_equal(engine.read(api.BUF_INLIER_COUNTS), ref["inlier_counts"])
    np.testing.assert_array_equal(engine.read(api.BUF_INLIER_MAP), ref["inlier_map"])
    assert np.isfinite(res[api.RES_RVEC:api.RES_RVEC + 6]).all()
    # what the data determine -- the reprojection of the inliers -- agrees tightly; the pose itself only along the
    # five constrained directions, so it is compared through the residual it leaves
    pts = coords[0, :, 12, :].T.copy()
    uv_dev = oracle.project(res[api.RES_RVEC:api.RES_RVEC + 3], res[api.RES_TVEC:api.RES_TVEC + 3], 525.0, 525.0, 320.0, 240.0, pts)
    uv_ref = oracle.project(ref["refined"][:3], ref["refined"][3:], 525.0, 525.0, 320.0, 240.0, pts)
    assert np.abs(uv_dev - uv_ref).max() <= 2e-3, np.abs(uv_dev - uv_ref).max()
    r, tt = S.pose_errors(res[api.RES_POSE:api.RES_POSE + 16].reshape(4, 4), ref["pose"])
    assert r <= 1e-4 and tt <= 1e-3, (r, tt)


def test_stage_timing_entry_point(engine):
    """esac_hip_time_stages (what bench.py's `kernels` / `roofline` use): four positive stage times whose sum is close to
    the blocking call, and the chain it runs leaves the same result as a plain forward."""
    import time
    f = S.make_frame(50)
    ha = S.gating_assignment(f, 256)
    sc, hat = torch.from_numpy(f["coords"]).cuda(), torch.from_numpy(ha).cuda()
    p = engine.make_params(1, 60, 80, 256, seed=8, call=3)
    res = engine.forward_device(sc, hat, p)
    st = engine.time_stages(sc, hat, p, reps=8)
    assert set(st) == {"sample", "score", "select_rescore", "refine"} and all(v > 0 for v in st.values())
    np.testing.assert_array_equal(engine.read(api.BUF_RESULT)[:31], res[:31])
    calls = []
    for _ in range(21):
        t0 = time.perf_counter()
        engine.forward_device(sc, hat, p)
        calls.append((time.perf_counter() - t0) * 1e3)
    call_ms = float(np.median(calls))  # the median: one host-side stall among the calls must not decide a timing check
    assert 0.5 * call_ms < sum(st.values()) < 1.2 * call_ms, (st, call_ms)
    assert st["refine"] > st["sample"] > st["score"]  # the single frame's profile: one-CU refinement dominates


def test_bench_default_line_has_the_contract_fields():
    """`python bench.py --full --steps 30 --warmup 5` (what the driver runs, shortened, with every extra figure): ONE JSON
    line with the contract's keys, the workload of BASELINE configs[1], roofline + per-stage kernels + cpu_baseline + accuracy."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--full", "--steps", "30", "--warmup", "5", "--batch", "4"],
                         capture_output=True, text=True, timeout=900, cwd=root)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
              "dtype", "data", "config", "roofline", "cpu_baseline", "kernels", "accuracy"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 30 and d["warmup"] == 5 and d["vs_baseline"] is None and d["data"] == "synthetic"
    assert d["config"]["name"] == "cfg2" and d["config"]["hypotheses_total"] == 256 and d["config"]["grid"] == [60, 80]
    assert "model" not in d["config"] and "workload" in d["config"]
    assert abs(d["value"] - 256 / (d["ms_per_step"] * 1e-3)) < 1e-6 * d["value"]
    r = d["roofline"]
    assert r["unit"] == "GB/s" and r["peak"] == 8000.0 and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-12
    assert r["algorithmic_bytes_per_launch"] == 256 * 12 * 60 * 80
    assert d["cpu_baseline"]["value"] > 0 and d["cpu_baseline"]["cores"] >= 1 and d["cpu_baseline"]["kind"] in ("port", "reference")
    assert d["accuracy"]["winner_match"] == 1.0 and d["accuracy"]["max_rot_err_rad"] <= 1e-4 and d["accuracy"]["max_trans_err_m"] <= 1e-3
    assert [k["stage"] for k in d["kernels"]] == ["sample", "score", "select_rescore", "refine"]
    assert d["value_seed1305"] > 0 and d["profile_stale"] in (True, False, None)


def test_bench_plain_line_is_lean_and_dumps_its_last_timed_step(tmp_path):
    """`python bench.py --steps 30 --warmup 5 --dump-outputs DIR` (no --full): the contract's line and nothing measured
    beyond the K timed steps; DIR holds the record, pose and score vector of the LAST timed step (call warmup + steps - 1 on
    frame (warmup + steps - 1) % 16) -- the same call made here on a context of its own gives them bit for bit."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--steps", "30", "--warmup", "5", "--dump-outputs", str(tmp_path)],
                         capture_output=True, text=True, timeout=300, cwd=root)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in d, k
    assert d["steps"] == 30 and d["warmup"] == 5 and d["unit"] == "hypotheses/s" and d["higher_is_better"] is True
    assert abs(d["value"] - 256 / (d["ms_per_step"] * 1e-3)) < 1e-6 * d["value"]
    for k in ("cpu_baseline", "accuracy", "kernels", "roofline", "phase_ms", "value_seed1305", "value_fast", "value_exact",
              "sharded_world1", "with_h2d", "batched", "training"):
        assert k not in d, k
    record, pose, scores = (np.load(str(tmp_path / (n + ".npy"))) for n in ("record", "pose", "scores"))
    assert record.dtype == np.float64 and record.shape == (api.RES_DOUBLES,)
    assert pose.dtype == np.float32 and np.array_equal(pose, record[api.RES_POSE:api.RES_POSE + 16].astype(np.float32).reshape(4, 4))
    assert scores.dtype == np.float64 and scores.shape == (256,)
    last = 5 + 30 - 1
    f = S.make_frame(last % 16)
    ha = S.gating_assignment(f, 256)
    eng = api.Engine(0)
    p = eng.make_params(1, 60, 80, 256, seed=1320, call=last, exact_scores="auto", focal=f["focal"], ppx=f["ppx"], ppy=f["ppy"],
                        sub_sampling=f["sub"])
    sc = torch.empty(256, dtype=torch.float64, device="cuda")
    rec = eng.forward_device(torch.from_numpy(f["coords"]).cuda(), torch.from_numpy(ha).cuda(), p, scores_out=sc)
    np.testing.assert_array_equal(record, rec)
    np.testing.assert_array_equal(scores, sc.cpu().numpy())


def _adversarial_frame(kind, E=3):
    """Maps on which four random cells are near-degenerate P3P configurations (scripts/dev/screen_adversarial.py): experts
    1.. hold planar / spherical / warped maps that are INCONSISTENT with the pixel grid, so their hypotheses need many
    tries and walk the screened chain; expert 0 is an ordinary room."""
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location(
        "screen_adversarial", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts", "dev", "screen_adversarial.py"))
    A = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(A)
    maps = A.adversarial_maps()
    f = S.make_frame(300, E=E, true_expert=0)
    names = {"planar": ["plane warped 3x0.33 tilted", "plane warped 2x0.5"],
             "degenerate": ["points within 1 mm of a line", "plane warped, x and y quantised"],
             "curved": ["sphere warped 2x0.5", "room, rows swapped pairwise"]}[kind]
    for e, n in enumerate(names, start=1):
        f["coords"][e] = maps[n]
    return f


@pytest.mark.parametrize("kind", ["planar", "degenerate", "curved"])
def test_screened_sampling_on_adversarial_geometry(engine, oracle, kind):
    """The sampling screen (p3p_screen.hpp) on the geometry that breaks a naive one: wrong-expert hypotheses on planar /
    tilted / quantised / sliver-triangle / spherical maps -- near-double roots of the P3P quartic, near-collinear and
    coincident samples -- in numbers that run the whole screened chain (N = 12288: k_sample_first x2, prescreen, decide,
    commit, resume).  The screened route must give the unscreened route's (ESAC_FLAG_EXACT_SAMPLING) accepted try, cells
    and pose bit for bit -- that is the screen's guarantee -- and both must be the oracle's, except where a try's three
    base points are collinear in space (the documented divergence of the exact route's alignment, checked below).
    ~2e6 / 1.5e7 / 2e5 tries in the three cases (budget capped at 5000)."""
    f = _adversarial_frame(kind)
    N = 12288
    ha = np.arange(N, dtype=np.int64) % 3
    sc, hat = torch.from_numpy(f["coords"]).cuda(), torch.from_numpy(ha).cuda()
    kw = dict(focal=f["focal"], ppx=f["ppx"], ppy=f["ppy"], sub_sampling=f["sub"], seed=77, call=3, max_tries=5000)
    ref = oracle.forward(f["coords"], ha, **kw)
    out = {}
    for exact in (False, True):
        p = engine.make_params(3, 60, 80, N, exact_sampling=exact, **kw)
        engine.sample(sc, hat, p)
        out[exact] = (engine.read(api.BUF_TRIES), engine.read(api.BUF_SAMPLE_XY), engine.read(api.BUF_HYPS))
    np.testing.assert_array_equal(out[False][0], out[True][0])   # screened == unscreened on the device: the screen's guarantee
    np.testing.assert_array_equal(out[False][1], out[True][1])
    np.testing.assert_array_equal(out[False][2], out[True][2])
    # ... == the oracle, except the ONE documented divergence of the exact route ("collinear base
    # points"): a try whose three base points are collinear in space (on an exactly planar map: three cells of one image
    # line) has no unique pose -- the reference's eigenvector alignment (p3p::align / jacobi_4x4) returns an arbitrary
    # roll about that line, decided by rounding noise, and the 4th point then passes tau by chance; the device's triad
    # alignment takes another roll (or none: NaN).  Every disagreement must be of exactly that kind, and rare.
    bad = np.nonzero(out[False][0] != ref["tries"])[0]
    assert len(bad) <= 16, len(bad)  # ~2e-6 per try on the exactly planar maps, none elsewhere
    for h in bad:
        t_dev, t_ref = int(out[False][0][h]), int(ref["tries"][h])
        t_first = min(t for t in (t_dev, t_ref) if t >= 0)  # the try the two sides decided differently
        xy = oracle.draw_cells(77, 3, int(h), t_first, 80, 60)
        P = np.array([[f["coords"][ha[h], c, y, x] for c in range(3)] for x, y in xy[:3]], np.float64)
        e1, e2 = P[1] - P[0], P[2] - P[0]
        sin2 = np.dot(np.cross(e1, e2), np.cross(e1, e2)) / max(np.dot(e1, e1) * np.dot(e2, e2), 1e-300)
        assert sin2 < 1e-8, (int(h), t_dev, t_ref, sin2)  # a sliver: base points collinear to 1e-4 rad
    same = out[False][0] == ref["tries"]
    np.testing.assert_array_equal(out[False][1][same], ref["sample_xy"][same])
    tries = np.where(ref["tries"] < 0, 5000, ref["tries"] + 1)
    assert tries.sum() > {"planar": 1.5e6, "degenerate": 5e6, "curved": 1e5}[kind] and (ref["tries"][ha > 0] > 64).any()  # the screened chain really ran


def test_exact_sampling_flag_is_the_reference_loop(engine, oracle):
    """ESAC_FLAG_EXACT_SAMPLING / esac.set_exact_sampling: no screen anywhere -- and nothing else changes: full forward
    against the oracle at the shapes that otherwise hand stragglers to the screened chain (latency shape with several
    experts, throughput shape)."""
    import esac
    for N, seed in ((512, 5), (6000, 6)):
        f = S.make_frame(310 + seed, E=4, true_expert=2)
        ha = S.gating_assignment(f, N, mode="dirichlet")
        ha[::5] = 2
        res, ref = _run_both(engine, oracle, f, ha, seed=seed, call=2, exact_sampling=True)
        _check_full(engine, res, ref)
    f = S.make_frame(312, E=2, true_expert=1)
    ha = S.gating_assignment(f, 300, mode="gating")
    pose_a, pose_b = torch.zeros(4, 4), torch.zeros(4, 4)
    args = (0, 0, f["focal"], f["ppx"], f["ppy"], 10.0, 100.0, 0.5, 100.0, f["sub"])
    try:
        esac.set_seed(9, 0)
        ea = esac.forward(torch.from_numpy(f["coords"]), torch.from_numpy(ha), pose_a, *args)
        esac.set_exact_sampling(True)
        esac.set_seed(9, 0)
        eb = esac.forward(torch.from_numpy(f["coords"]), torch.from_numpy(ha), pose_b, *args)
    finally:
        esac.set_exact_sampling(False)
    assert ea == eb and torch.equal(pose_a, pose_b)


def test_status_word_follows_the_sampling_launch_not_the_last_call(engine):
    """An out-of-range hypAssignment (device-resident tensor) is reported for the launch that SAMPLED it: by a staged
    refine that runs several entry points later, by esac_hip_check after an asynchronous call followed by other entry
    points (pick_record bumps the context's epoch) -- and no longer once a clean call has sampled."""
    f = S.make_frame(320, E=2, true_expert=1)
    ha = S.gating_assignment(f, 128, mode="gating")
    bad = ha.copy()
    bad[5] = 7
    sc = torch.from_numpy(f["coords"]).cuda()
    p = engine.make_params(2, 60, 80, 128, seed=3, call=1)
    rec = torch.zeros(64, dtype=torch.float64, device="cuda")
    engine.forward_device(sc, torch.from_numpy(bad).cuda(), p, result_out=rec[:32], want_host=False)
    engine.pick_record(rec, 2)  # another entry point in between
    with pytest.raises(RuntimeError, match="outside"):
        engine.check()
    # staged: sample (flags it) ... refine delivers the status to a later blocking call's record
    for stage in (engine.sample, engine.score, engine.select):
        stage(sc, torch.from_numpy(bad).cuda(), p)
    with pytest.raises(RuntimeError, match="outside"):
        engine.check()
    engine.forward_device(sc, torch.from_numpy(ha).cuda(), p)  # a clean call
    engine.check()


def test_blocking_wait_modes_agree(engine):
    """esac_hip_set_wait: spin (default), yield and block deliver the same record."""
    f = S.make_frame(321)
    ha = S.gating_assignment(f, 256)
    sc, hat = torch.from_numpy(f["coords"]).cuda(), torch.from_numpy(ha).cuda()
    recs = []
    try:
        for mode in (api.WAIT_SPIN, api.WAIT_YIELD, api.WAIT_BLOCK):
            engine.set_wait(mode)
            recs.append(engine.forward_device(sc, hat, engine.make_params(1, 60, 80, 256, seed=4, call=4)).copy())
    finally:
        engine.set_wait(api.WAIT_SPIN)
    np.testing.assert_array_equal(recs[0], recs[1])
    np.testing.assert_array_equal(recs[0], recs[2])
    with pytest.raises(RuntimeError):
        engine.set_wait(7)


def test_cooperative_refinement_reports_a_barrier_time_out(engine):
    """The cooperating refinement workgroups of a large-grid call must all be resident; when one never arrives (a shared
    or partitioned GPU) the barrier times out ONCE (the counter is poisoned: every later barrier falls through), the
    blocking call fails with status -12, an asynchronous call leaves a record WITHOUT the valid marker and
    esac_hip_check reports it.  ESAC_DEBUG_COOP_STALL makes the barrier wait for one workgroup more than was launched."""
    import time
    f = S.make_frame(322, H=120, W=160, sub=4)
    ha = S.gating_assignment(f, 64)
    sc, hat = torch.from_numpy(f["coords"]).cuda(), torch.from_numpy(ha).cuda()
    p = engine.make_params(1, 120, 160, 64, seed=2, call=2)
    engine.set_refine_team(0)  # (a team would take this 19200-cell grid: the counter-barrier kernel is what is tested here)
    good = engine.forward_device(sc, hat, p).copy()
    assert engine.refine_info()["mode"] == "cooperating"
    engine.set_debug(coop_stall=True)
    try:
        t0 = time.time()
        with pytest.raises(RuntimeError, match="status -12"):
            engine.forward_device(sc, hat, p)
        assert time.time() - t0 < 5.0  # one bounded spin, not one per barrier
        rec = torch.full((32,), 7.0, dtype=torch.float64, device="cuda")
        engine.forward_device(sc, hat, p, result_out=rec, want_host=False)
        with pytest.raises(RuntimeError, match="status -12"):
            engine.check()
        assert float(rec[31]) == 3.0  # ESAC_RES_VALID = 3: not a record, and not an empty shard either
    finally:
        engine.set_debug()
    again = engine.forward_device(sc, hat, p)
    engine.set_refine_team(api.REFINE_TEAM_DEFAULT)
    np.testing.assert_array_equal(again, good)  # the context recovers
    engine.check()


# ---------------------------------------------------------------- the refinement team (esac_refine_team.hip)
def _team_run(engine, oracle, frame, ha, seed, call, **kw):
    sc, hat = torch.from_numpy(frame["coords"]).cuda(), torch.from_numpy(ha).cuda()
    E, _, H, W = frame["coords"].shape
    p = engine.make_params(E, H, W, len(ha), shift_x=frame["shift"][0], shift_y=frame["shift"][1], focal=frame["focal"],
                           ppx=frame["ppx"], ppy=frame["ppy"], sub_sampling=frame["sub"], seed=seed, call=call, **kw)
    rec = engine.forward_device(sc, hat, p).copy()
    out = {"rec": rec, "counts": engine.read(api.BUF_INLIER_COUNTS), "map": engine.read(api.BUF_INLIER_MAP), "info": engine.refine_info()}
    return out


def _same_refinement(a, b):
    """Two runs of one refinement that differ in how many workgroups shared it: every discrete output identical, the
    pose equal to what the rounding of the LM sums (their summation order differs) becomes through the damped normal
    equations: measured <= 6e-10, asserted 1e-8 (the bar against the oracle is 1e-6)."""
    discrete = [api.RES_HYP, api.RES_EXPERT, api.RES_REF_STEPS, api.RES_INLIERS, api.RES_LM_ITERS]
    np.testing.assert_array_equal(a["rec"][discrete], b["rec"][discrete])
    # (the winner's exact score: a team that also runs the selection sums the cells member by member)
    assert abs(a["rec"][api.RES_SCORE] - b["rec"][api.RES_SCORE]) <= 1e-12 * max(1.0, abs(b["rec"][api.RES_SCORE]))
    np.testing.assert_array_equal(a["counts"], b["counts"])
    np.testing.assert_array_equal(a["map"], b["map"])
    np.testing.assert_allclose(a["rec"][:31], b["rec"][:31], rtol=0, atol=1e-8)


def test_refinement_team_sizes_agree_with_one_workgroup_and_the_oracle(engine, oracle):
    """esac_hip_set_refine_team: the winner's refinement of a single 60x80 frame shared by 5..19 workgroups (fewer would
    not fit a member's slice into its lanes' registers, more than ceil(4800 / 256) = 19 would leave lanes without a cell:
    the launcher clamps the request) against ONE workgroup and the oracle -- refinement trace (steps, inlier count per
    step, inlier map, LM iterations) identical, pose to 1e-8."""
    try:
        for k in range(4):
            f = S.make_frame(400 + k)
            ha = S.gating_assignment(f, 128)
            engine.set_refine_team(0)
            solo = _team_run(engine, oracle, f, ha, 21, k)
            assert solo["info"]["mode"] == "one_workgroup" and solo["info"]["workgroups"] == 1
            ref = oracle.forward(f["coords"], ha, shift_x=f["shift"][0], shift_y=f["shift"][1], focal=f["focal"], ppx=f["ppx"],
                                 ppy=f["ppy"], sub_sampling=f["sub"], seed=21, call=k)
            for members in (2, 5, 7, 8, 9, 12, 16, 19, 32):
                engine.set_refine_team(members)
                team = _team_run(engine, oracle, f, ha, 21, k)
                info = team["info"]
                assert info["mode"] == "team" and info["workgroups"] == min(max(members, 5), 19) and not info["timed_out"], info
                # observed placement: workgroup b runs on XCD b % 8 -- the members (every eighth workgroup) share one
                assert info["same_xcd"] and sum(info["xcd_census"]) == info["workgroups"], info
                _same_refinement(team, solo)
                assert int(team["rec"][api.RES_REF_STEPS]) == ref["ref_steps"]
                np.testing.assert_array_equal(team["counts"], ref["inlier_counts"])
                np.testing.assert_array_equal(team["map"], ref["inlier_map"])
                np.testing.assert_allclose(team["rec"][api.RES_RVEC:api.RES_RVEC + 6], ref["refined"], rtol=0, atol=1e-6)
    finally:
        engine.set_refine_team(api.REFINE_TEAM_DEFAULT)


def test_refinement_team_on_different_xcds(engine, oracle):
    """ESAC_DEBUG_TEAM_SPREAD launches the members as CONSECUTIVE workgroups, which the hardware places on eight
    different XCDs -- the exchange (write-through granules, L1-bypassing polls) must not depend on where the members
    run: same trace, same pose; the info words report the mismatch."""
    f = S.make_frame(410)
    ha = S.gating_assignment(f, 128)
    engine.set_refine_team(19)  # (more members than XCDs: two or three per XCD when spread)
    try:
        together = _team_run(engine, oracle, f, ha, 22, 0)
        engine.set_debug(team_spread=True)
        spread = _team_run(engine, oracle, f, ha, 22, 0)
    finally:
        engine.set_debug()
        engine.set_refine_team(api.REFINE_TEAM_DEFAULT)
    assert together["info"]["same_xcd"] and not spread["info"]["same_xcd"], (together["info"], spread["info"])
    assert spread["info"]["mode"] == "team" and spread["info"]["workgroups"] == 19 and not spread["info"]["timed_out"]
    assert max(spread["info"]["xcd_census"]) <= 3 and sum(spread["info"]["xcd_census"]) == 19  # 19 consecutive workgroups over 8 XCDs
    np.testing.assert_array_equal(spread["rec"][:31], together["rec"][:31])  # the same sums in the same order: bit for bit
    np.testing.assert_array_equal(spread["map"], together["map"])


def test_refinement_team_time_out_falls_back_to_one_workgroup(engine, oracle):
    """A member that never becomes resident (ESAC_DEBUG_COOP_STALL: the last one leaves at once): the others give up after
    a bounded spin, the BLOCKING call refines again in one workgroup and returns that result; an asynchronous call
    leaves a record without the valid marker and esac_hip_check reports -12; the context recovers."""
    import time
    f = S.make_frame(411)
    ha = S.gating_assignment(f, 128)
    sc, hat = torch.from_numpy(f["coords"]).cuda(), torch.from_numpy(ha).cuda()
    p = engine.make_params(1, 60, 80, 128, seed=23, call=1)
    try:
        engine.set_refine_team(0)
        solo = engine.forward_device(sc, hat, p).copy()
        engine.set_refine_team(api.REFINE_TEAM_DEFAULT)
        before = engine.refine_info()["team_fallbacks"]
        engine.set_debug(coop_stall=True)
        t0 = time.time()
        rec = engine.forward_device(sc, hat, p).copy()
        assert time.time() - t0 < 5.0
        info = engine.refine_info()
        assert info["mode"] == "one_workgroup" and info["team_fallbacks"] == before + 1, info
        np.testing.assert_array_equal(rec[:31], solo[:31])
        dev_rec = torch.full((32,), 7.0, dtype=torch.float64, device="cuda")
        engine.forward_device(sc, hat, p, result_out=dev_rec, want_host=False)
        with pytest.raises(RuntimeError, match="status -12"):
            engine.check()
        assert float(dev_rec[31]) == 3.0  # ESAC_RES_VALID = 3: not a record, and not an empty shard either
    finally:
        engine.set_debug()
        engine.set_refine_team(api.REFINE_TEAM_DEFAULT)
    again = engine.forward_device(sc, hat, p)
    assert engine.refine_info()["mode"] == "team" and not engine.refine_info()["timed_out"]
    np.testing.assert_allclose(again[:31], solo[:31], rtol=0, atol=1e-8)
    engine.check()


def test_team_time_out_is_bounded_and_latches(oracle):
    """A member that never becomes resident (ESAC_DEBUG_COOP_STALL) with the PRODUCTION wait: the others give up after 1 ms of
    wall clock (round 4 spun for seconds), the blocking call refines again in one workgroup and returns that route's result;
    after two such calls in a row the context stops asking for teams -- the third call runs in one workgroup at once, stall
    or not -- until esac_hip_set_refine_team re-arms it.  The result never depends on the route beyond the rounding of the
    sums.  (What a competing kernel on another stream does to a team is in scripts/dev/contention_probe.py: the hardware
    dispatches the launch's workgroups in order, so the whole team starts late -- it is not split.)"""
    import time
    eng = api.Engine(0)  # a context of its own: this test latches it
    f = S.make_frame(433)
    ha = S.gating_assignment(f, 128)
    sc, hat = torch.from_numpy(f["coords"]).cuda(), torch.from_numpy(ha).cuda()
    p = eng.make_params(1, 60, 80, 128, seed=29, call=2)
    ref = oracle.forward(f["coords"], ha, seed=29, call=2)
    eng.set_refine_team(0)
    solo = eng.forward_device(sc, hat, p).copy()
    eng.set_refine_team(api.REFINE_TEAM_DEFAULT)
    team = eng.forward_device(sc, hat, p).copy()
    assert eng.refine_info()["mode"] == "team" and eng.refine_info()["team_fallbacks"] == 0

    def timed_call():
        t0 = time.perf_counter()
        rec = eng.forward_device(sc, hat, p).copy()
        return rec, time.perf_counter() - t0

    # (wall-clock bounds on a shared box: the references are the best of three calls, the upper bounds say "not seconds")
    dt0 = min(timed_call()[1] for _ in range(3))
    eng.set_debug(coop_stall=True)
    try:
        rec1, dt1 = timed_call()
        info = eng.refine_info()
        assert info["team_fallbacks"] == 1 and info["mode"] == "one_workgroup" and not info["team_latched_off"], (info, dt1)
        assert 0.0008 < dt1 - dt0 < 0.5, (dt0, dt1)  # the 1 ms wait + one workgroup's refinement (+ first-use costs of that route), not seconds
        np.testing.assert_array_equal(rec1[:31], solo[:31])
        rec2, dt2 = timed_call()
        info = eng.refine_info()
        assert info["team_fallbacks"] == 2 and info["team_latched_off"], info
        assert 0.0008 < dt2 - dt0 < 0.5, (dt0, dt2)  # measured 1.2 ms (scripts/dev/stall_probe.py); the bound leaves room for a loaded host
                                                     # (one run of the suite beside other jobs read 65 ms here once, 1.2 ms on three re-runs)
        np.testing.assert_array_equal(rec2[:31], solo[:31])
        rec3, dt3 = timed_call()  # latched: one workgroup at once, no time-out to wait for
        info = eng.refine_info()
        assert info["team_fallbacks"] == 2 and info["mode"] == "one_workgroup" and not info["timed_out"] and info["team_latched_off"], info
        np.testing.assert_array_equal(rec3[:31], solo[:31])
        dt3 = min([dt3] + [timed_call()[1] for _ in range(2)])  # (still latched: the same route every time)
        assert dt3 < dt0 + 0.0005, (dt0, dt3)
    finally:
        eng.set_debug()
    # the result is the oracle's on every route
    for rec in (solo, team, rec1, rec3):
        assert int(rec[api.RES_HYP]) == ref["winner"] and int(rec[api.RES_REF_STEPS]) == ref["ref_steps"] and int(rec[api.RES_LM_ITERS]) == ref["lm_iters"]
        r_err, t_err = S.pose_errors(rec[api.RES_POSE:api.RES_POSE + 16].reshape(4, 4), ref["pose"])
        assert r_err <= 1e-6 and t_err <= 1e-5
    eng.set_refine_team(api.REFINE_TEAM_DEFAULT)  # re-arm
    again = eng.forward_device(sc, hat, p)
    info = eng.refine_info()
    assert info["mode"] == "team" and not info["team_latched_off"], info
    np.testing.assert_array_equal(again[:31], team[:31])


@pytest.mark.parametrize("H,W,sub", [(32, 40, 8), (33, 47, 5), (60, 80, 8), (64, 128, 4), (59, 83, 8), (120, 160, 4), (128, 256, 2)])
def test_refinement_team_on_other_grids(engine, oracle, H, W, sub):
    """Grids of 1024 .. 32768 cells, rows that are not a multiple of four cells, 1 to 4 cells per lane, 5 to 32 members: the
    team against the oracle (trace, map, pose) and against one workgroup (or the cooperating workgroups of the large grids)."""
    f = S.make_frame(420 + H, H=H, W=W, sub=sub)
    ha = S.gating_assignment(f, 64)
    try:
        engine.set_refine_team(0)
        solo = _team_run(engine, oracle, f, ha, 24, H)
        engine.set_refine_team(api.REFINE_TEAM_DEFAULT)
        team = _team_run(engine, oracle, f, ha, 24, H)
    finally:
        engine.set_refine_team(api.REFINE_TEAM_DEFAULT)
    assert team["info"]["mode"] == "team", team["info"]
    _same_refinement(team, solo)
    ref = oracle.forward(f["coords"], ha, shift_x=f["shift"][0], shift_y=f["shift"][1], focal=f["focal"], ppx=f["ppx"], ppy=f["ppy"],
                         sub_sampling=f["sub"], seed=24, call=H)
    np.testing.assert_array_equal(team["counts"], ref["inlier_counts"])
    np.testing.assert_array_equal(team["map"], ref["inlier_map"])
    assert int(team["rec"][api.RES_LM_ITERS]) == ref.get("lm_iters", int(team["rec"][api.RES_LM_ITERS]))
    np.testing.assert_allclose(team["rec"][api.RES_RVEC:api.RES_RVEC + 6], ref["refined"], rtol=0, atol=1e-6)


def test_refinement_team_debug_error_image_and_step_limit(engine, oracle):
    """The options that change what a pass must leave behind: max_ref_steps = 0, 1, 2 (the team's loop ends on the step limit,
    esac_util.h:396) and the error image of the refined pose (ESAC_DEBUG_ERROR_IMAGE) -- which the ONE-workgroup kernel serves since
    round 6 (the debug stores and their exact projections inside the team's loop cost every call 1.2 us whether they ran or not)."""
    f = S.make_frame(430)
    ha = S.gating_assignment(f, 96)
    try:
        for steps in (0, 1, 2, -1):
            engine.set_debug()
            plain = _team_run(engine, oracle, f, ha, 25, 3, max_ref_steps=steps)
            assert plain["info"]["mode"] == "team"
            engine.set_debug(keep_error_image=True)
            team = _team_run(engine, oracle, f, ha, 25, 3, max_ref_steps=steps)
            errs = engine.read(api.BUF_WINNER_ERRS)
            ref = oracle.forward(f["coords"], ha, shift_x=f["shift"][0], shift_y=f["shift"][1], focal=f["focal"], ppx=f["ppx"],
                                 ppy=f["ppy"], sub_sampling=f["sub"], seed=25, call=3, max_ref_steps=steps)
            assert team["info"]["mode"] == "one_workgroup"
            _same_refinement(plain, team)
            assert int(plain["rec"][api.RES_REF_STEPS]) == ref["ref_steps"]
            np.testing.assert_array_equal(plain["counts"][:len(ref["inlier_counts"])], ref["inlier_counts"])
            assert int(team["rec"][api.RES_REF_STEPS]) == ref["ref_steps"]
            n = len(ref["inlier_counts"])  # (the oracle's trace has max_ref_steps + 1 entries)
            np.testing.assert_array_equal(team["counts"][:n], ref["inlier_counts"])
            assert (team["counts"][n:] == -1).all()
            np.testing.assert_array_equal(team["map"], ref["inlier_map"])
            np.testing.assert_allclose(team["rec"][api.RES_RVEC:api.RES_RVEC + 6], ref["refined"], rtol=0, atol=1e-6)
            # the error image of the REFINED pose (the last error pass of refineHyp, esac_util.h:445-452)
            pose = team["rec"][api.RES_RVEC:api.RES_RVEC + 6]
            pts = f["coords"][0].reshape(3, -1).T.copy()
            uv = oracle.project(pose[:3], pose[3:], f["focal"], f["focal"], f["ppx"], f["ppy"], pts).reshape(60, 80, 2)
            ys, xs = np.mgrid[0:60, 0:80]
            want = np.minimum(np.hypot(xs * 8 + 4 - uv[..., 0], ys * 8 + 4 - uv[..., 1]), 100.0)
            np.testing.assert_allclose(errs, want, rtol=0, atol=2e-2)
            np.testing.assert_array_equal(errs < 10.0, want < 10.0)  # the inlier side is decided exactly
    finally:
        engine.set_debug()


def test_selection_folded_into_the_team_kernel_equals_the_selection_kernel(engine, oracle):
    """A single frame of <= 256 hypotheses that a team refines runs the selection (softmax statistics, the band of
    contenders, their re-score in reference arithmetic) in the refinement kernel's prologue; the same call phase by phase
    (esac_hip_sample / _score / _select / _refine) runs k_select_rescore.  Both must leave the same score vector,
    contender flags, winner, exact score, probability, entropy and contender count -- and the oracle's winner.  Cases:
    one and several experts, a wide band (dozens of contenders: several exchanges of 16), a band that takes everything."""
    cases = [dict(E=1, N=256, alpha=100.0), dict(E=3, N=200, alpha=100.0), dict(E=1, N=97, alpha=100.0, margin=30.0),
             dict(E=2, N=64, alpha=7.0, margin=50.0)]
    for k, c in enumerate(cases):
        f = S.make_frame(440 + k, E=c["E"], true_expert=c["E"] - 1)
        ha = S.gating_assignment(f, c["N"], mode="gating" if c["E"] > 1 else "single")
        sc, hat = torch.from_numpy(f["coords"]).cuda(), torch.from_numpy(ha).cuda()
        p = engine.make_params(c["E"], 60, 80, c["N"], seed=31, call=k, inlier_alpha=c["alpha"], rescore_margin=c.get("margin", 0.0))
        rec = engine.forward_device(sc, hat, p).copy()
        assert engine.refine_info()["mode"] == "team"
        scores, flags = engine.read(api.BUF_SCORES).copy(), engine.read(api.BUF_EXACT_FLAGS).copy()
        engine.sample(sc, hat, p)
        engine.score(sc, hat, p)
        engine.select(sc, hat, p)
        engine.refine(sc, hat, p)
        torch.cuda.synchronize()
        rec2 = engine.read(api.BUF_RESULT)
        np.testing.assert_array_equal(flags, engine.read(api.BUF_EXACT_FLAGS))
        scores2 = engine.read(api.BUF_SCORES)
        np.testing.assert_array_equal(scores[flags == 0], scores2[flags == 0])
        np.testing.assert_allclose(scores[flags == 1], scores2[flags == 1], rtol=1e-12, atol=0)  # another summation order of the cells
        for field in (api.RES_HYP, api.RES_EXPERT, api.RES_CONTENDERS, api.RES_REF_STEPS, api.RES_INLIERS, api.RES_LM_ITERS):
            assert rec[field] == rec2[field], (k, field, rec[field], rec2[field])
        np.testing.assert_allclose(rec[[api.RES_SCORE, api.RES_PROB, api.RES_ENTROPY]], rec2[[api.RES_SCORE, api.RES_PROB, api.RES_ENTROPY]],
                                   rtol=1e-12, atol=0)
        assert int(rec[api.RES_CONTENDERS]) == int(flags.sum())
        if k == 2:
            assert int(rec[api.RES_CONTENDERS]) > 16  # more than one exchange of contenders
        ref = oracle.forward(f["coords"], ha, focal=f["focal"], ppx=f["ppx"], ppy=f["ppy"], sub_sampling=f["sub"], seed=31, call=k,
                             inlier_alpha=c["alpha"])
        assert int(rec[api.RES_HYP]) == ref["winner"]
        np.testing.assert_allclose(scores[flags == 1], ref["scores"][flags == 1], rtol=0, atol=1e-7 * max(1.0, c["alpha"]))


def test_sampling_screen_is_one_sided_on_the_device():
    """The screen must never reject a try the fp64 route accepts -- checked where the kernels run it: the screen's private
    root solver uses v_rcp / v_rsq / v_sqrt estimates and contraction on the device, IEEE operations in the host probe
    (tests/native/p3p_screen_probe.cpp).  tests/native/screen_campaign.hip compiles the product's headers with the
    product's flags and decides every random try both ways ON THE GPU: 1.3e8 tries per map on six adversarial maps here
    (scripts/dev/screen_campaign_device.py runs 1e11+; log under profiles/).  No accepted try may be lost at the kernels'
    3-pixel margin, nor at 2."""
    import ctypes as C
    import sys
    import os
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "scripts", "dev"))
    from tests.native import build as nb
    from screen_adversarial import adversarial_maps, quantised_maps
    from screen_campaign_device import run
    lib = C.CDLL(nb.build_screen_campaign())
    maps = adversarial_maps()
    qm = quantised_maps()
    picks = [("fronto-parallel exact", maps), ("plane warped, x and y quantised", maps), ("sphere warped 2x0.5", maps),
             ("room, 1 cell right", maps), ("room quantised 0.05 m", qm), ("clean room piecewise constant 2x2", qm)]
    accepted = 0
    for k, (name, fam) in enumerate(picks):
        out = run(lib, fam[name], 1.3e8, 4000 + k)
        accepted += out[1]
        assert out[0] >= 1e8 and out[7] == 0 and out[6] == 0, (name, out)
        assert out[8] <= 10.0 + 2.0, (name, out[8])  # largest screen error of an accepted try: well inside tau + 3
    assert accepted > 1e7


@pytest.mark.parametrize("N", [1, 2, 255, 256, 257])
def test_team_and_folded_selection_at_the_edges_of_their_shapes(engine, oracle, N):
    """One and two hypotheses, and the three sizes around the 256 hypotheses up to which the team kernel runs the selection
    itself (one hypothesis per thread of a member): full forward against the oracle."""
    f = S.make_frame(450 + N)
    ha = S.gating_assignment(f, N)
    sc, hat = torch.from_numpy(f["coords"]).cuda(), torch.from_numpy(ha).cuda()
    p = engine.make_params(1, 60, 80, N, focal=f["focal"], ppx=f["ppx"], ppy=f["ppy"], sub_sampling=f["sub"], seed=41, call=N)
    rec = engine.forward_device(sc, hat, p).copy()
    ref = oracle.forward(f["coords"], ha, focal=f["focal"], ppx=f["ppx"], ppy=f["ppy"], sub_sampling=f["sub"], seed=41, call=N)
    assert engine.refine_info()["mode"] == "team"
    assert int(rec[api.RES_HYP]) == ref["winner"] and int(rec[api.RES_REF_STEPS]) == ref["ref_steps"]
    np.testing.assert_array_equal(engine.read(api.BUF_INLIER_COUNTS), ref["inlier_counts"])
    np.testing.assert_array_equal(engine.read(api.BUF_INLIER_MAP), ref["inlier_map"])
    np.testing.assert_allclose(rec[api.RES_RVEC:api.RES_RVEC + 6], ref["refined"], rtol=0, atol=1e-6)
    flags = engine.read(api.BUF_EXACT_FLAGS).astype(bool)
    assert flags[ref["winner"]] and int(rec[api.RES_CONTENDERS]) == int(flags.sum())
    np.testing.assert_allclose(engine.read(api.BUF_SCORES)[flags], ref["scores"][flags], rtol=0, atol=1e-7)


@pytest.mark.parametrize("H,W", [(31, 33), (32, 32), (16, 64)])
def test_grids_at_the_lower_edge_of_the_team(engine, oracle, H, W):
    """1023 cells (one workgroup refines), 1024 cells in two shapes (the smallest grids a team takes): against the oracle."""
    f = S.make_frame(460 + H, H=H, W=W, sub=8)
    ha = S.gating_assignment(f, 48)
    sc, hat = torch.from_numpy(f["coords"]).cuda(), torch.from_numpy(ha).cuda()
    kw = dict(shift_x=f["shift"][0], shift_y=f["shift"][1], focal=f["focal"], ppx=f["ppx"], ppy=f["ppy"], sub_sampling=f["sub"], seed=42, call=H)
    rec = engine.forward_device(sc, hat, engine.make_params(1, H, W, 48, **kw)).copy()
    ref = oracle.forward(f["coords"], ha, **kw)
    assert engine.refine_info()["mode"] == ("team" if H * W >= 1024 else "one_workgroup")
    assert int(rec[api.RES_HYP]) == ref["winner"] and int(rec[api.RES_REF_STEPS]) == ref["ref_steps"]
    np.testing.assert_array_equal(engine.read(api.BUF_INLIER_COUNTS), ref["inlier_counts"])
    np.testing.assert_array_equal(engine.read(api.BUF_INLIER_MAP), ref["inlier_map"])
    np.testing.assert_allclose(rec[api.RES_RVEC:api.RES_RVEC + 6], ref["refined"], rtol=0, atol=1e-6)


# (call, E, N, H, W, sub-sampling, score shape) -- 6x8: the smallest workspace; 32x32 tiled: the tiled-score workspace comes into
# being; 96x96 (P > 8192): the training workspace regrows with its correspondence lists; then the first two shapes again
_REGROW_STEPS = [("forward", 1, 16, 6, 8, 80, "auto"), ("forward", 2, 64, 32, 32, 15, "tiled"), ("backward", 1, 16, 6, 8, 80, "auto"),
                 ("backward", 1, 16, 96, 96, 5, "auto"), ("forward", 1, 16, 6, 8, 80, "auto"), ("backward", 1, 16, 6, 8, 80, "auto")]


def _regrow_call(eng, step):
    """One call of the sequence on `eng`: everything the call hands out, by name.  The key (seed, call) and the inputs depend on
    the step's shape only, so the repeats at the end of the sequence are the calls of its beginning."""
    kind, E, N, H, W, sub, shape = step
    f = S.make_frame(700 + H, E=E, H=H, W=W, sub=sub)
    ha = S.gating_assignment(f, N, mode="gating")
    sc, hat = torch.from_numpy(f["coords"]).cuda(), torch.from_numpy(ha).cuda()
    p = eng.make_params(E, H, W, N, seed=77, call=H + (1000 if kind == "backward" else 0), refine_solo=True, score_shape=shape, **_kw(f))
    out = {}
    if kind == "forward":
        scores = torch.empty(N, dtype=torch.float64, device="cuda")
        out["record"] = eng.forward_device(sc, hat, p, scores_out=scores).copy()
        out["scores"] = scores.cpu().numpy()
    else:
        gt = f["gt_pose"].astype(np.float32)
        gt[:3, 3] += np.float32(0.03)
        grads = torch.zeros_like(sc)
        rec = torch.zeros(api.RES_DOUBLES, dtype=torch.float64, device="cuda")
        out["values"] = eng.backward_device(sc, grads, hat, gt, 1.0, 100.0, 100.0, p, pose_record=rec).copy()
        out["record"] = rec.cpu().numpy()
        out["scores"] = eng.read(api.BUF_SCORES)
        out["gradients"] = grads.cpu().numpy()
    out["tries"] = eng.read(api.BUF_TRIES)
    out["sample_xy"] = eng.read(api.BUF_SAMPLE_XY)
    return out


def _regrow_runs():
    """The sequence on ONE engine, and every call of it on a fresh engine of its own."""
    eng = api.Engine(0)
    return [_regrow_call(eng, s) for s in _REGROW_STEPS], [_regrow_call(api.Engine(0), s) for s in _REGROW_STEPS]


def test_a_regrown_workspace_is_invisible():
    """One engine runs _REGROW_STEPS in order: its forward workspace grows twice, its tiled-score workspace comes into being, its
    training workspace grows and then regrows with the correspondence lists of a grid above the LDS limit.  Every call must hand out
    what a fresh engine hands out for it, and the repeats at the end (steps 5, 6) what steps 1 and 3 handed out: record, score
    vector, tries, sampled cells, the four training values, the gradient tensor.  All with ESAC_FLAG_REFINE_SOLO and fixed keys.
    EXACT equality for every field, by reasoning and not yet by a measurement on the commit before the workspace owners existed (to
    be made with the first GPU run of this test): tries and sampled cells are functions of the RNG key (tests/test_gpu_parity.py
    holds them equal to the oracle's); no kernel adds floating-point values with atomics (every atomic in esac_amd/csrc is an
    integer counter or ticket), every sum runs in an order fixed by the launch shape, and with ESAC_FLAG_REFINE_SOLO one workgroup
    refines -- so scores, record, training values and gradients depend on the call's inputs and shape alone.  A field that turns
    out not to be bit-reproducible on that commit gets the tolerance tests/test_gpu_parity.py uses for it, and is named here."""
    seq, fresh = _regrow_runs()
    for k, (a, b) in enumerate(zip(seq, fresh)):
        assert a.keys() == b.keys()
        for name in a:
            print("step", k + 1, name, "differing elements:", int(np.sum(~((a[name] == b[name]) | ((a[name] != a[name]) & (b[name] != b[name]))))))
            np.testing.assert_array_equal(a[name], b[name], err_msg="step %d %s against a fresh engine" % (k + 1, name))
    for first, again in ((0, 4), (2, 5)):
        for name in seq[first]:
            np.testing.assert_array_equal(seq[first][name], seq[again][name], err_msg="step %d %s against its repeat" % (first + 1, name))
    assert seq[3]["values"][1] >= 1 and np.abs(seq[3]["gradients"]).max() > 0  # (the large grid refined slots and produced gradients)
