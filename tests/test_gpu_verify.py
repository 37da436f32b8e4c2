"""esac_hip_verify_batch on the device: every frozen case of tests/verify_reference.py against the numpy reference, the oracle and
the host build of the same arithmetic; batches against single-frame calls bit for bit; the two pose formats; every status;
isolation from a forward batch and stream order; the harness.  Grids of 192 to 768 cells, E = 3, at most 5 poses per frame."""
import ctypes as C

import numpy as np
import pytest
import torch

from esac_amd import api, harness
from oracle import esac_oracle as oracle
from tests import verify_reference as V
from tests.native import build_verify

pytestmark = pytest.mark.gpu

SOLVER = (V.SCORE["tau"], V.SCORE["alpha"], V.SCORE["beta"], V.SCORE["max_reproj"], V.SCORE["sub"])
HOLD_MS = 50.0  # inside hold_launch's 200 ms limit


@pytest.fixture(scope="module")
def gold():
    return V.golden()


def _cam_args(frames, per_frame):
    cams = [f["cam"] for f in frames]
    if not per_frame:
        c = cams[0]
        assert all(x == c for x in cams)
        return (c["shift"][0], c["shift"][1], c["focal"], c["ppx"], c["ppy"])
    return ([c["shift"][0] for c in cams], [c["shift"][1] for c in cams], [c["focal"] for c in cams], [c["ppx"] for c in cams], [c["ppy"] for c in cams])


def _call(case, rows, fmt=0, frames_of=None, poses=None, experts=None, strict=None):
    """esac.verify_batch of a frozen case (or of the frames `frames_of` of it alone).  Returns host rows [B,K,64]."""
    import esac
    sel = list(range(len(rows))) if frames_of is None else list(frames_of)
    frames = [rows[b][0][0] for b in sel]
    if poses is None:
        poses = np.stack([np.stack([r[2] for r in rows[b]]) for b in sel])
    if experts is None:
        experts = np.array([[r[3] for r in rows[b]] for b in sel], np.int64)
    if fmt == 1:
        poses = np.stack([[V.camera_pose_from_rt(p) for p in frame] for frame in poses]).astype(np.float32)
    d_poses = torch.from_numpy(np.ascontiguousarray(poses)).cuda()
    d_experts = torch.from_numpy(np.ascontiguousarray(experts)).cuda()
    kw = {}
    if case["ragged"]:
        sc = [torch.from_numpy(f["coords"]).cuda() for f in frames]
        kw["shapes"] = [(f["h"], f["w"]) for f in frames]
    elif case["shared"]:
        sc = torch.from_numpy(frames[0]["coords"]).cuda()
    else:
        sc = torch.from_numpy(np.stack([f["coords"] for f in frames])).cuda()
    esac.set_strict_reference(case["strict"] if strict is None else strict)
    try:
        out = esac.verify_batch(sc, d_poses, d_experts, *(_cam_args(frames, case["cams"] or case["ragged"]) + SOLVER), **kw)
        torch.cuda.synchronize()
    finally:
        esac.set_strict_reference(False)
    assert tuple(out.shape) == (len(sel), poses.shape[1], api.VERIFY_DOUBLES) and out.dtype == torch.float64 and out.is_cuda
    return out.cpu().numpy()


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


# ------------------------------------------------------------------------------------------------ 4: every frozen case
@pytest.mark.parametrize("name", [c["name"] for c in V.CASES])
def test_frozen_case_against_reference_oracle_and_host_probe(engine, gold, name):
    """device rows: score against the oracle at 1e-12, n exactly, SSE / A / C within the bars of verify_reference.py; and against
    the host build of verify_math.hpp: score, SSE and A to the summation-order bars, n and status equal"""
    case = next(c for c in V.CASES if c["name"] == name)
    rows = V.case_rows(case)
    got = _call(case, rows)
    reqs = [(row[0][0]["coords"][row[0][3]], row[0][0]["cam"], V.SCORE, case["strict"], 0, np.stack([r[2] for r in row])) for row in rows]
    host, _ = build_verify.run_probe(build_verify.build_probe(), reqs)
    worst = dict(A=0.0, sse=0.0, C=0.0, host_A=0.0, host_sse=0.0, host_score=0.0)
    for b, row in enumerate(rows):
        fr = row[0][0]
        coords = fr["coords"] if case["strict"] else fr["oracle_coords"]
        cam = fr["cam"]
        scores = oracle.forward(coords, np.array([r[3] for r in row], np.int64), cam["shift"][0], cam["shift"][1], cam["focal"], cam["ppx"], cam["ppy"],
                                *SOLVER, in_hyps=np.stack([r[2] for r in row]))["scores"]
        for k, (_, kind, pose, expert) in enumerate(row):
            label = "%s[%d,%d] %s/%s" % (name, b, k, fr["name"], kind)
            m = V.check_row(got[b, k], fr, kind, case["strict"], gold, oracle_score=scores[k], label=label)
            d, h = got[b, k], host[b][k]
            assert d[1] == h[1] and d[4] == h[4], (label, d[:5], h[:5])
            if np.isnan(h[0]):
                assert np.isnan(d[0]), label
            else:
                hs = abs(d[0] - h[0]) / max(abs(h[0]), 1e-300) if h[0] != 0 else abs(d[0])
                assert hs <= V.BAR_SCORE, (label, d[0], h[0])
                worst["host_score"] = max(worst["host_score"], hs)
            if h[1] > 0:
                scale = np.sqrt(np.abs(np.outer(np.diag(V.sym(h[6:27])), np.diag(V.sym(h[6:27])))))[V.IU]
                ha, hsse = float(np.max(np.abs(d[6:27] - h[6:27]) / scale)), abs(d[2] - h[2]) / h[2]
                assert ha <= V.BAR_A and hsse <= V.BAR_SSE, (label, ha, hsse)
                worst["host_A"], worst["host_sse"] = max(worst["host_A"], ha), max(worst["host_sse"], hsse)
            for key in ("A", "sse"):
                worst[key] = max(worst[key], m.get(key, 0.0))
            if "C" in m:
                worst["C"] = max(worst["C"], m["C"] / m["C_bar"])
    print("%s: against the 50-digit sums A %.3g (bar %.3g), SSE %.3g (bar %.3g), C / bar %.3g; against the host build A %.3g, SSE %.3g, score %.3g"
          % (name, worst["A"], V.BAR_A, worst["sse"], V.BAR_SSE, worst["C"], worst["host_A"], worst["host_sse"], worst["host_score"]))


# ------------------------------------------------------------------------------------------------ 5: batches against single frames
@pytest.mark.parametrize("name", ["cams_B3_K1", "cams_B3_K5", "ragged_B3_K5", "shared_B3_K5"])
def test_frame_of_a_batch_is_the_single_frame_call_bit_for_bit(engine, name):
    case = next(c for c in V.CASES if c["name"] == name)
    rows = V.case_rows(case)
    batch = _call(case, rows)
    for b in range(len(rows)):
        single = _call(case, rows, frames_of=[b])
        assert _same_bits(batch[b], single[0]), (name, b, np.argwhere(batch[b] != single[0])[:6])
    again = _call(case, rows)
    assert _same_bits(batch, again)  # run to run


# ------------------------------------------------------------------------------------------------ 6: formats
@pytest.mark.parametrize("name", ["g13x17s_B1_K5_e2", "cams_B3_K5", "ragged_B3_K5"])
def test_4x4_format_gives_the_rows_of_the_rt_format(engine, name):
    """the float32 camera pose loses ~1e-7 of the pose: the rows of the two formats differ by what the reference loses when the pose
    goes through float32 and back on the CPU (plus the bars both device rows carry), and status and n are equal"""
    case = next(c for c in V.CASES if c["name"] == name)
    rows = V.case_rows(case)
    rt, m44 = _call(case, rows, fmt=0), _call(case, rows, fmt=1)
    for b, row in enumerate(rows):
        for k, (fr, kind, pose, expert) in enumerate(row):
            label = "%s[%d,%d] %s/%s" % (name, b, k, fr["name"], kind)
            V.check_formats(rt[b, k], m44[b, k], fr, kind, label)


# ------------------------------------------------------------------------------------------------ 7: statuses
def test_every_status_without_a_fault_and_the_neighbours_unaffected(engine):
    """status 1 (the far pose), 3 (a NaN pose, an infinite one, a singular 4x4), 4 (expert -1 and E) beside good poses in one call:
    the good rows are bit for bit the rows of a call without the bad ones.  Status 2 from a map whose inliers are collinear."""
    case = next(c for c in V.CASES if c["name"] == "cams_B3_K5")
    rows = V.case_rows(case)
    clean = _call(case, rows)
    poses = np.stack([np.stack([r[2] for r in row]) for row in rows])
    experts = np.array([[r[3] for r in row] for row in rows], np.int64)
    bad_p, bad_e = poses.copy(), experts.copy()
    bad_p[0, 1, 4] = np.nan
    bad_p[1, 0, 0] = np.inf
    bad_e[1, 2], bad_e[2, 3], bad_e[2, 0] = -1, V.E, 2 ** 32 + 1  # (int64 on the way in: 2^32 + 1 must not wrap into expert 1)
    got = _call(case, rows, poses=bad_p, experts=bad_e)
    bad = {(0, 1): 3, (1, 0): 3, (1, 2): 4, (2, 3): 4, (2, 0): 4}
    for b in range(3):
        for k in range(5):
            if (b, k) in bad:
                r = got[b, k]
                assert r[4] == bad[(b, k)] and r[5] == 0 and r[27] == 0, (b, k, r[:6])
                assert np.isnan(np.delete(r, [4, 5, 27])).all(), (b, k)
            else:
                assert _same_bits(got[b, k], clean[b, k]), (b, k)
    far = [(b, k) for b, row in enumerate(rows) for k, r in enumerate(row) if r[1] == "far"]
    assert len(far) == 3 and all(clean[b, k, 4] == 1 and np.isnan(clean[b, k, 3]) and np.isnan(clean[b, k, 28:]).all() for b, k in far)
    # a singular 4x4 (two equal rows) and a NaN one beside a good one
    m44 = np.stack([[V.camera_pose_from_rt(p) for p in frame] for frame in poses]).astype(np.float32)
    good44 = _call(case, rows, fmt=1)
    m44[0, 0, 2] = m44[0, 0, 1]
    m44[2, 4, 1, 1] = np.nan
    import esac
    frames = [row[0][0] for row in rows]
    out = esac.verify_batch(torch.from_numpy(np.stack([f["coords"] for f in frames])).cuda(), torch.from_numpy(m44).cuda(), torch.from_numpy(experts).cuda(),
                            *(_cam_args(frames, True) + SOLVER)).cpu().numpy()
    for b in range(3):
        for k in range(5):
            if (b, k) in ((0, 0), (2, 4)):
                assert out[b, k, 4] == 3 and np.isnan(np.delete(out[b, k], [4, 5, 27])).all(), (b, k)
            else:
                assert _same_bits(out[b, k], good44[b, k]), (b, k)
    # status 2: collinear inliers
    coords, pose, cam = V.collinear_case()
    row = esac.verify_batch(torch.from_numpy(coords).cuda(), torch.from_numpy(pose.reshape(1, 1, 6)).cuda(), torch.tensor([1], dtype=torch.int32, device="cuda"),
                            0, 0, cam["focal"], cam["ppx"], cam["ppy"], *SOLVER).cpu().numpy()[0, 0]
    assert row[4] == 2 and row[1] == 16, row[:5]
    A = V.sym(row[6:27])
    assert (A[0] == 0).all() and np.linalg.matrix_rank(A[1:, 1:]) == 5
    Cm = row[28:64].reshape(6, 6)
    assert (Cm[0] == 0).all() and (Cm[:, 0] == 0).all() and (Cm == Cm.T).all()
    want = row[3] * oracle.pinv_sym6(A)
    np.testing.assert_allclose(Cm, want, rtol=1e-9, atol=1e-12 * np.abs(want).max())  # the bar check_solves holds the pseudo-inverse to
    # A itself, from the definition at rvec = 0: dXc / dr_i = e_i x X, dXc / dt = I
    X = coords[1, :, 5].T.astype(np.float64)
    Xc = X + pose[3:]
    dX = [np.cross(e, X) for e in np.eye(3)] + [np.broadcast_to(e, X.shape) for e in np.eye(3)]
    Ju = np.stack([cam["focal"] * (d[:, 0] / Xc[:, 2] - Xc[:, 0] * d[:, 2] / Xc[:, 2] ** 2) for d in dX], axis=1)
    Jv = np.stack([cam["focal"] * (d[:, 1] / Xc[:, 2] - Xc[:, 1] * d[:, 2] / Xc[:, 2] ** 2) for d in dX], axis=1)
    np.testing.assert_allclose(A, Ju.T @ Ju + Jv.T @ Jv, rtol=1e-13, atol=1e-13 * np.abs(A).max())


def test_library_refuses_bad_arguments_before_a_launch(engine):
    lib = engine.lib
    out = torch.zeros(2, 5, 64, dtype=torch.float64, device="cuda")
    sc = torch.zeros(2, 3, 3, 12, 16, device="cuda")
    poses = torch.zeros(2, 5, 6, dtype=torch.float64, device="cuda")
    ex = torch.zeros(2, 5, dtype=torch.int32, device="cuda")
    p = engine.make_params(3, 12, 16, 5, 0, 0, 100.0, 64.0, 48.0, *SOLVER)
    good = [2, 5, sc.data_ptr(), sc.stride(0), poses.data_ptr(), 0, ex.data_ptr(), C.byref(p), None, 0, None, out.data_ptr()]
    for at, value, needle in ((0, 0, b"B = 0"), (1, 1025, b"K = 1025"), (5, 2, b"pose_format"), (2, None, b"d_sc"), (4, None, b"d_poses"),
                              (6, None, b"d_experts"), (11, None, b"d_out"), (9, 1, b"ragged without")):
        args = list(good)
        args[at] = value
        assert lib.esac_hip_verify_batch(engine.ctx, *args) == -4, (at, value)
        assert b"esac_hip_verify_batch" in lib.esac_hip_last_error() and needle in lib.esac_hip_last_error()
    torch.cuda.synchronize()
    assert float(out.abs().max()) == 0.0  # nothing was launched


# ------------------------------------------------------------------------------------------------ 8: isolation and stream order
def _forward_inputs():
    frames = [V.frame(n) for n in ("g24x32", "g24x32e2", "g24x32")]
    sc = torch.from_numpy(np.stack([f["coords"] for f in frames])).cuda()
    ha = torch.from_numpy(np.stack([np.full(32, f["true_expert"], np.int64) for f in frames])).cuda()
    c = frames[0]["cam"]
    return frames, sc, ha, (0, 0, c["focal"], c["ppx"], c["ppy"])


def test_verify_leaves_a_forward_batch_as_it_was_and_scores_its_winner(engine):
    import esac
    frames, sc, ha, cam = _forward_inputs()
    B = 3
    try:
        esac.set_seed(1305, 900)
        fwd = esac.forward_batch_async(sc, ha, *(cam + SOLVER))
        torch.cuda.synchronize()
        engine.check()
        before = {w: engine.read_forward_frames(w, B) for w in (api.BUF_HYPS, api.BUF_SCORES, api.BUF_TRIES, api.BUF_SAMPLE_XY, api.BUF_INLIER_COUNTS)}
        rec = fwd["records"].cpu().numpy()
        scores = fwd["scores"].cpu().numpy()
        assert (rec[:, api.RES_VALID] == 1).all()
        win = rec[:, api.RES_HYP].astype(int)
        unrefined = np.stack([before[api.BUF_HYPS][b, win[b]] for b in range(B)])
        poses = np.stack([unrefined, rec[:, api.RES_RVEC:api.RES_RVEC + 6]], axis=1)  # [B,2,6]: the winning hypothesis, its refinement
        rows = esac.verify_batch(sc, torch.from_numpy(poses).cuda(), torch.from_numpy(rec[:, api.RES_EXPERT].astype(np.int64)).cuda(), *(cam + SOLVER))
        torch.cuda.synchronize()
        assert esac.last_result() is fwd and esac.get_rng_state() == (1305, 900 + B)
        for w, was in before.items():
            np.testing.assert_array_equal(engine.read_forward_frames(w, B), was)
        np.testing.assert_array_equal(fwd["records"].cpu().numpy(), rec)
        np.testing.assert_array_equal(fwd["scores"].cpu().numpy(), scores)
        rows = rows.cpu().numpy()
        for b in range(B):
            assert abs(rows[b, 0, 0] - rec[b, api.RES_SCORE]) <= V.BAR_SCORE * abs(rec[b, api.RES_SCORE]), (b, rows[b, 0, 0], rec[b, api.RES_SCORE])
            assert rows[b, 0, 4] == 0 and rows[b, 1, 4] == 0
            print("frame %d: winner n = %d, refined n = %d (RES_INLIERS %d, counted before the last re-fit), sigma %.3g px"
                  % (b, rows[b, 0, 1], rows[b, 1, 1], rec[b, api.RES_INLIERS], np.sqrt(rows[b, 1, 3])))
        # the same two calls on a side stream, nothing between them: the verify call reads the records the batch is still writing
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            esac.set_seed(1305, 900)
            fwd2 = esac.forward_batch_async(sc, ha, *(cam + SOLVER))
            refined = fwd2["records"][:, api.RES_RVEC:api.RES_RVEC + 6].reshape(B, 1, 6)
            rows2 = esac.verify_batch(sc, refined, fwd2["records"][:, api.RES_EXPERT].to(torch.int64), *(cam + SOLVER))
        side.synchronize()
        torch.cuda.synchronize()
        np.testing.assert_array_equal(fwd2["records"].cpu().numpy()[:, :31], rec[:, :31])
        assert _same_bits(rows2.cpu().numpy()[:, 0], rows[:, 1])
    finally:
        torch.cuda.synchronize()


def test_strict_mode_on_and_off_for_the_nan_map(engine):
    case = next(c for c in V.CASES if c["name"] == "nan_B1_K5")
    rows = V.case_rows(case)
    default, strict = _call(case, rows, strict=False), _call(case, rows, strict=True)
    assert np.isfinite(default[0, :, 0]).all() and np.isnan(strict[0, :, 0]).all()
    assert _same_bits(default[0, :, 1:], strict[0, :, 1:])  # the inlier set and everything over it do not depend on the rule
    again = _call(case, rows, strict=False)
    assert _same_bits(default, again)


# ------------------------------------------------------------------------------------------------ 9: harness
_hold_fn = []


def _hold(ms):
    """Queues the sleeping wavefront (tests/native/filler.hip) on torch's current stream."""
    if not _hold_fn:
        from tests.native import build as nb
        lib = C.CDLL(nb.build_filler())
        lib.hold_launch.argtypes = [C.c_void_p, C.c_float]
        lib.hold_launch.restype = C.c_int
        _hold_fn.append(lib.hold_launch)
    rc = _hold_fn[0](C.c_void_p(torch.cuda.current_stream().cuda_stream), float(ms))
    assert rc == 0, "hold_launch(%g ms) answered %d" % (ms, rc)


def test_localize_batch_verify_gt_equals_a_direct_call_and_waits_for_nothing(engine):
    import esac
    from tests.test_gpu_eval_batch import N, _eight_samples
    frames, gating, experts, samples = _eight_samples()
    Bn = 4
    images = torch.cat([s[1] for s in samples[:Bn]])
    gts = torch.from_numpy(np.stack([f["gt_pose"] for f in frames[:Bn]]).astype(np.float32)).cuda()
    ge = torch.tensor([0, 1, 0, 1], device="cuda")
    focals = [f["focal"] for f in frames[:Bn]]
    solver = (10.0, 100.0, 0.5, 100.0, 8)

    def run(**kw):
        esac.set_seed(1305, 300)
        return harness.localize_batch(images, gating, experts, focals, gt_poses=gts, hypotheses=N,
                                      generator=torch.Generator(device="cuda").manual_seed(3), verify_gt=True, **kw)

    out = run(gt_experts=ge)
    assert tuple(out["gt_verify"].shape) == (Bn, 1, 64) and out["gt_verify"].is_cuda
    direct = esac.verify_batch(out["prediction"], gts.reshape(Bn, 1, 4, 4), ge, 0, 0, focals, 320.0, 240.0, *solver)
    torch.cuda.synchronize()
    assert _same_bits(out["gt_verify"].cpu().numpy(), direct.cpu().numpy())
    got = out["gt_verify"].cpu().numpy()[:, 0]
    assert (got[:, 4] == 0).all() and (got[:, 1] > 1000).all() and (got[:, 0] > 0.5 * out["records_host"][:, api.RES_SCORE]).all(), got[:, :5]
    # without gt_experts: the winner's expert, read from the device records
    out2 = run()
    direct2 = esac.verify_batch(out2["prediction"], gts.reshape(Bn, 1, 4, 4), torch.tensor(out2["experts"]), 0, 0, focals, 320.0, 240.0, *solver)
    assert _same_bits(out2["gt_verify"].cpu().numpy(), direct2.cpu().numpy())
    plain = harness.localize_batch(images, gating, experts, focals, gt_poses=gts, gt_experts=ge, hypotheses=N,
                                   generator=torch.Generator(device="cuda").manual_seed(3))
    assert "gt_verify" not in plain
    # asynchronous: behind a hold on the stream the step returns with the stream still busy
    run(gt_experts=ge, asynchronous=True, all_experts=True)  # (everything the route allocates exists: nothing grows behind the hold)
    torch.cuda.synchronize()
    _hold(HOLD_MS)
    late = run(gt_experts=ge, asynchronous=True, all_experts=True)
    busy = not torch.cuda.current_stream().query()
    torch.cuda.synchronize()
    assert busy, "localize_batch(asynchronous=True, all_experts=True, verify_gt=True) waited for the stream"
    assert late["gt_verify"].is_cuda and _same_bits(late["gt_verify"].cpu().numpy(), out["gt_verify"].cpu().numpy())
    # evaluate(verify_gt=True): the share of frames whose ground truth outscores the winner
    kept, original = [], harness.localize_batch

    def keeping(*a, **k):
        kept.append(original(*a, **k))
        return kept[-1]
    mp = pytest.MonkeyPatch()
    mp.setattr(harness, "localize_batch", keeping)
    try:
        esac.set_seed(1305, 40)
        stats = harness.evaluate(iter(samples), gating, experts, hypotheses=N, generator=torch.Generator(device="cuda").manual_seed(5), batch_size=3,
                                 verify_gt=True)
        esac.set_seed(1305, 40)
        base = harness.evaluate(iter(samples), gating, experts, hypotheses=N, generator=torch.Generator(device="cuda").manual_seed(5), batch_size=3)
    finally:
        mp.undo()
    higher = np.concatenate([b["gt_verify"].cpu().numpy()[:, 0, 0] > b["records_host"][:, api.RES_SCORE] for b in kept[:3]])
    assert len(higher) == 8 and stats["gt_score_higher"] == float(np.mean(higher))
    assert "gt_score_higher" not in base and base["scenes"] == stats["scenes"]
