"""GPU tests of the per-frame camera of the batched calls: esac_hip_forward_batch_cams / esac_hip_backward_batch_cams through
`Engine.forward_batch(cams=)` / `Engine.backward_batch(cams=)`, the sequence arguments of `esac.forward_batch` /
`esac.backward_batch`, and `harness.train_batch`.

Frame b of such a batch is the single call with frame b's own shift, focal length and principal point at call counter
call0 + b: every frame is checked against the CPU oracle called with that camera (the bars of the training and forward paths,
restated below, not loosened), and against the single calls bit for bit where both run the same refinement route.

The eight frames: `synthetic.make_frame(900 + b, shift=SHIFTS[b], focal=FOCALS[b])`, counters 40 + b, seed 1305.  On the CPU
oracle all sixteen (1 expert x 256 hypotheses, 4 experts x 128) select between 8 and 22 slots, their losses lie between 1.8 and
22 and no probability is within 1e-5 of the selection threshold, so the slot count is asserted on every frame and nothing is
exempted; every frame's forward ends in a refined winner with > 1000 inliers.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from esac_amd import api
from esac_amd import synthetic as S

pytestmark = pytest.mark.gpu

# the bars of tests/test_gpu_backward.py / tests/test_gpu_backward_batch.py
GRAD_RTOL = 2e-6
GRAD_RTOL_SAMPLED = 1e-3
LOSS_RTOL = 1e-7

SHIFTS = [(0, 0), (4, -4), (-3, 2), (1, 4), (-4, -1), (2, 0), (0, -2), (3, 3)]
FOCALS = [525.0, 585.0, 480.0, 1050.0, 525.0, 700.0, 612.5, 560.0]
SHAPES = [(1, 256, "single"), (4, 128, "gating")]
SEED, CALL0, ALPHA = 1305, 40, 100.0
# records swapped between frames (0<->4, 1<->7, 2<->6, 3<->5).  Checked on the CPU oracle: every frame still selects 10 .. 23
# slots, nothing within 6e-6 of the threshold, and every expected loss moves (3.67 -> 3.83 at the least, 1.94 -> 159 at the most)
PERM = [4, 7, 6, 5, 0, 1, 2, 3]


def _gt(frame, seed, noise=0.05):
    gt = np.array(frame["gt_pose"], np.float64)
    gt[:3, 3] += np.random.default_rng(seed).normal(size=3) * noise
    return gt.astype(np.float32)


def _inputs(E, N, mode, B=8, first=900):
    frames = [S.make_frame(first + b, E=E, true_expert=b % E, shift=SHIFTS[b % 8], focal=FOCALS[b % 8]) for b in range(B)]
    has = [S.gating_assignment(f, N, mode=mode) for f in frames]
    gts = [_gt(f, b) for b, f in enumerate(frames)]
    return frames, has, gts


def _cams(frames, order=None):
    fs = frames if order is None else [frames[k] for k in order]
    return api.make_cams([f["shift"][0] for f in fs], [f["shift"][1] for f in fs], [f["focal"] for f in fs],
                         [f["ppx"] for f in fs], [f["ppy"] for f in fs])


def _params(eng, f, N, call, cam=None, alpha=ALPHA, **kw):
    """Parameter block of ONE frame: its own camera (or the record `cam`)."""
    E, _, H, W = f["coords"].shape
    sx, sy, fo, px, py = (f["shift"][0], f["shift"][1], f["focal"], f["ppx"], f["ppy"]) if cam is None else \
        (int(cam["shift_x"]), int(cam["shift_y"]), float(cam["focal"]), float(cam["ppx"]), float(cam["ppy"]))
    return eng.make_params(E, H, W, N, shift_x=sx, shift_y=sy, focal=fo, ppx=px, ppy=py, sub_sampling=f["sub"],
                           inlier_alpha=alpha, seed=SEED, call=call, **kw)


def _batch_params(eng, f, N, call, alpha=ALPHA):
    """Parameter block of a batch with a table: the five camera fields are ignored, so they carry values no frame uses."""
    E, _, H, W = f["coords"].shape
    return eng.make_params(E, H, W, N, shift_x=-77, shift_y=91, focal=1234.5, ppx=-5.0, ppy=9999.0, sub_sampling=f["sub"],
                           inlier_alpha=alpha, seed=SEED, call=call)


def _oracle_bwd(oracle, f, ha, gt, cam, call, alpha=ALPHA, g0=None):
    g = np.zeros_like(f["coords"]) if g0 is None else g0.copy()
    ref = oracle.backward(f["coords"], g, ha, gt, w_rot=1.0, w_trans=100.0, loss_cut=100.0, shift_x=int(cam["shift_x"]),
                          shift_y=int(cam["shift_y"]), focal=float(cam["focal"]), ppx=float(cam["ppx"]), ppy=float(cam["ppy"]),
                          sub_sampling=f["sub"], inlier_alpha=alpha, seed=SEED, call=call)
    return ref, g


def _run_bwd(eng, frames, has, gts, cams, call0=CALL0, alpha=ALPHA, g0=None, p=None):
    sc = torch.from_numpy(np.stack([f["coords"] for f in frames])).cuda()
    ha = torch.from_numpy(np.stack(has)).cuda()
    g = torch.from_numpy(g0.copy()).cuda() if g0 is not None else torch.zeros(sc.shape, dtype=torch.float32, device="cuda")
    p = p if p is not None else _batch_params(eng, frames[0], ha.shape[1], call0, alpha)
    out = eng.backward_batch(sc, g, ha, np.stack(gts), 1.0, 100.0, 100.0, p, cams=cams)
    return out, g.cpu().numpy()


def _check_bwd_frame(b, out, g_dev, ref, g_ref, probs, ref_hyps, losses, g_init=None):
    """Frame-level parity with the oracle -- record, distribution, slot count (always), refined poses, losses, gradient."""
    sel_ref = np.nonzero(ref["probs"] >= 1e-3)[0]
    err_loss = abs(out[0] - ref["loss"]) / max(1.0, abs(ref["loss"]))
    contrib = g_ref if g_init is None else g_ref - g_init
    scale = max(float(np.abs(contrib).max()), 1e-30)
    E, _, H, W = g_ref.shape
    sampled = np.zeros((H, W), bool)
    for h in sel_ref:
        for x, y in ref["sample_xy"][h]:
            sampled[y, x] = True
    diff = np.abs(g_dev - g_ref)
    err = float(diff[:, :, ~sampled].max()) / scale
    err_s = float(diff[:, :, sampled].max()) / scale if sampled.any() else 0.0
    print("frame %d: loss %.6f (oracle %.6f, rel %.2e) slots %d (oracle %d) edge %.2e grad rel %.2e sampled %.2e" %
          (b, out[0], ref["loss"], err_loss, int(out[1]), len(sel_ref), float(np.abs(ref["probs"] - 1e-3).min()), err, err_s))
    assert float(np.abs(ref["probs"] - 1e-3).min()) > 1e-12  # (the inputs keep clear of the selection threshold)
    assert int(out[1]) == len(sel_ref), (b, out[1], len(sel_ref))
    assert abs(out[2] - ref["entropy"]) < 1e-9
    np.testing.assert_allclose(probs, ref["probs"], rtol=1e-8, atol=1e-14)
    np.testing.assert_allclose(ref_hyps, ref["ref_hyps"], rtol=0, atol=1e-6)
    np.testing.assert_allclose(losses, ref["losses"], rtol=1e-6, atol=1e-6)
    assert err_loss <= LOSS_RTOL, (b, out[0], ref["loss"])
    assert out[3] == 0.0
    assert err <= GRAD_RTOL, (b, err, scale)
    assert err_s <= GRAD_RTOL_SAMPLED, (b, err_s, scale)
    assert np.isfinite(g_dev).all()
    return len(sel_ref)


# ---------------------------------------------------------------- 1. training, oracle parity per frame
@pytest.mark.parametrize("E, N, mode", SHAPES)
def test_training_every_frame_matches_the_oracle_with_its_own_camera(engine, oracle, E, N, mode):
    frames, has, gts = _inputs(E, N, mode)
    cams = _cams(frames)
    out, g = _run_bwd(engine, frames, has, gts, cams)
    probs = engine.read_frames(api.BUF_BWD_PROBS, 8)
    refh = engine.read_frames(api.BUF_BWD_REF_HYPS, 8)
    losses = engine.read_frames(api.BUF_BWD_LOSSES, 8)
    slots = []
    for b, f in enumerate(frames):
        ref, g_ref = _oracle_bwd(oracle, f, has[b], gts[b], cams[b], CALL0 + b)
        slots.append(_check_bwd_frame(b, out[b], g[b], ref, g_ref, probs[b], refh[b], losses[b]))
    assert 8 <= min(slots) and max(slots) <= 22, slots
    assert all(1.8 <= v <= 22.0 for v in out[:, 0]), out[:, 0]


# ---------------------------------------------------------------- 2. training, bit equality with single calls
@pytest.mark.parametrize("E, N, mode", SHAPES)
def test_training_batch_equals_single_calls_bit_for_bit(monkeypatch, E, N, mode):
    """One workgroup per slot on both sides (ESAC_SLOT_TEAMS=0): the batch with the table == 8 sequential backward_device calls,
    each with its own camera in its own parameter block."""
    monkeypatch.setenv("ESAC_SLOT_TEAMS", "0")
    solo = api.Engine(0)
    monkeypatch.delenv("ESAC_SLOT_TEAMS")
    frames, has, gts = _inputs(E, N, mode)
    out, g = _run_bwd(solo, frames, has, gts, _cams(frames))
    refh = solo.read_frames(api.BUF_BWD_REF_HYPS, 8)
    probs = solo.read_frames(api.BUF_BWD_PROBS, 8)
    seq_out, seq_g = [], []
    for b, f in enumerate(frames):
        sc = torch.from_numpy(f["coords"]).cuda()
        gb = torch.zeros_like(sc)
        seq_out.append(solo.backward_device(sc, gb, torch.from_numpy(has[b]).cuda(), gts[b], 1.0, 100.0, 100.0,
                                            _params(solo, f, N, CALL0 + b)))
        seq_g.append(gb.cpu().numpy())
        np.testing.assert_array_equal(solo.read(api.BUF_BWD_REF_HYPS), refh[b])
        np.testing.assert_array_equal(solo.read(api.BUF_BWD_PROBS), probs[b])
    np.testing.assert_array_equal(out, np.stack(seq_out))
    np.testing.assert_array_equal(g, np.stack(seq_g))
    assert out[:, 1].min() >= 8 and np.abs(g).max() > 0


# ---------------------------------------------------------------- 3. forward, oracle parity and bit equality
def _oracle_fwd(oracle, f, ha, cam, call, alpha=ALPHA):
    return oracle.forward(f["coords"], ha, shift_x=int(cam["shift_x"]), shift_y=int(cam["shift_y"]), focal=float(cam["focal"]),
                          ppx=float(cam["ppx"]), ppy=float(cam["ppy"]), sub_sampling=f["sub"], inlier_alpha=alpha, seed=SEED, call=call)


def _forward_case(engine, oracle, frames, has, N, single_team):
    """forward_batch with the table: every frame against the oracle called with its camera, and against the single call with its
    camera on the same refinement route (single_team: the team size of the single calls) bit for bit."""
    B = len(frames)
    cams = _cams(frames)
    coords = torch.from_numpy(np.stack([f["coords"] for f in frames])).cuda()
    ha = torch.from_numpy(np.stack(has)).cuda()
    scores_b = torch.empty(B, N, dtype=torch.float64, device="cuda")
    try:
        engine.set_refine_team(api.REFINE_TEAM_EIGHT)
        res = engine.forward_batch(coords, ha, _batch_params(engine, frames[0], N, CALL0), scores_out=scores_b, cams=cams)
        assert engine.refine_info()["mode"] == ("team" if B <= 32 else "one_workgroup")
        tries = engine.read_forward_frames(api.BUF_TRIES, B)
        cells = engine.read_forward_frames(api.BUF_SAMPLE_XY, B)
        counts = engine.read_forward_frames(api.BUF_INLIER_COUNTS, B)
        sc_host = scores_b.cpu().numpy()
        for b, f in enumerate(frames):
            ref = _oracle_fwd(oracle, f, has[b], cams[b], CALL0 + b)
            assert ref["ref_steps"] >= 1 and ref["inlier_map"].sum() > 0  # (a refined winner with a non-empty inlier set)
            assert int(res[b][api.RES_HYP]) == ref["winner"] and int(res[b][api.RES_EXPERT]) == ref["expert"], b
            np.testing.assert_array_equal(tries[b], ref["tries"], err_msg="frame %d" % b)
            np.testing.assert_array_equal(cells[b], ref["sample_xy"], err_msg="frame %d" % b)
            np.testing.assert_array_equal(counts[b], ref["inlier_counts"], err_msg="frame %d" % b)
            assert int(res[b][api.RES_REF_STEPS]) == ref["ref_steps"] and int(res[b][api.RES_LM_ITERS]) == ref["lm_iters"], b
            r, t = S.pose_errors(res[b][api.RES_POSE:api.RES_POSE + 16].reshape(4, 4), ref["pose"])
            assert r <= 1e-4 and t <= 1e-3, (b, r, t)
        engine.set_refine_team(single_team)
        for b, f in enumerate(frames):
            s1 = torch.empty(N, dtype=torch.float64, device="cuda")
            r1 = engine.forward_device(coords[b], ha[b], _params(engine, f, N, CALL0 + b), scores_out=s1)
            assert engine.refine_info()["mode"] == ("team" if single_team else "one_workgroup")
            np.testing.assert_array_equal(res[b][:31], r1[:31], err_msg="frame %d" % b)
            np.testing.assert_array_equal(sc_host[b], s1.cpu().numpy(), err_msg="frame %d" % b)
    finally:
        engine.set_refine_team(api.REFINE_TEAM_DEFAULT)
    return res


@pytest.mark.parametrize("E, N, mode", SHAPES)
def test_forward_batch_with_cams_oracle_and_single_calls(engine, oracle, E, N, mode):
    frames, has, _ = _inputs(E, N, mode)
    _forward_case(engine, oracle, frames, has, N, api.REFINE_TEAM_EIGHT)


def test_forward_batch_with_cams_beyond_32_frames(engine, oracle):
    """40 frames (the eight cameras cycled): the winners are refined by one workgroup per frame (grid row = frame), the route the
    single calls take with teams switched off."""
    frames, has, _ = _inputs(1, 48, "single", B=40)
    _forward_case(engine, oracle, frames, has, 48, 0)


def test_forward_batch_with_cams_on_another_grid(engine, oracle):
    """45 x 67 cells, sub-sampling 7, two experts, another principal point, shifts within +-3."""
    frames = []
    for b in range(4):
        sh = (SHIFTS[b + 1][0] * 3 // 4, SHIFTS[b + 1][1] * 3 // 4)
        frames.append(S.make_frame(920 + b, E=2, true_expert=b % 2, H=45, W=67, sub=7, shift=sh, focal=FOCALS[b + 1],
                                   ppx=234.5, ppy=157.5))
    has = [S.gating_assignment(f, 64, mode="gating") for f in frames]
    assert len({f["shift"] for f in frames}) == 4
    _forward_case(engine, oracle, frames, has, 64, api.REFINE_TEAM_EIGHT)


def test_forward_batch_with_cams_asynchronous_call_owns_its_table(engine):
    """want_host=False: the call returns before the kernels have run, the caller's table is overwritten at once, and a second
    asynchronous call with another table follows on the same stream -- each batch is computed with ITS records."""
    frames, has, _ = _inputs(1, 256, "single")
    cams = _cams(frames)
    coords = torch.from_numpy(np.stack([f["coords"] for f in frames])).cuda()
    ha = torch.from_numpy(np.stack(has)).cuda()
    p = _batch_params(engine, frames[0], 256, CALL0)
    want_a = engine.forward_batch(coords, ha, p, cams=cams)
    want_b = engine.forward_batch(coords, ha, p, cams=_cams(frames, PERM))
    assert not np.array_equal(want_a[:, api.RES_POSE:api.RES_POSE + 16], want_b[:, api.RES_POSE:api.RES_POSE + 16])
    rec_a = torch.zeros(8, api.RES_DOUBLES, dtype=torch.float64, device="cuda")
    rec_b = torch.zeros_like(rec_a)
    table = cams.copy()
    engine.forward_batch(coords, ha, p, result_out=rec_a, want_host=False, cams=table)
    table[:] = _cams(frames, PERM)  # the first call's upload may still be queued: it must not read this
    engine.forward_batch(coords, ha, p, result_out=rec_b, want_host=False, cams=table)
    table[:] = 0
    torch.cuda.synchronize()
    np.testing.assert_array_equal(rec_a.cpu().numpy()[:, :31], want_a[:, :31])
    np.testing.assert_array_equal(rec_b.cpu().numpy()[:, :31], want_b[:, :31])


# ---------------------------------------------------------------- 4. the table is really per frame
def test_permuted_records_change_the_losses_as_the_oracle_says(engine, oracle):
    frames, has, gts = _inputs(1, 256, "single")
    own, _ = _run_bwd(engine, frames, has, gts, _cams(frames))
    cams = _cams(frames, PERM)
    out, g = _run_bwd(engine, frames, has, gts, cams)
    for b, f in enumerate(frames):
        ref, g_ref = _oracle_bwd(oracle, f, has[b], gts[b], cams[b], CALL0 + b)
        rel = abs(out[b, 0] - ref["loss"]) / max(1.0, abs(ref["loss"]))
        print("frame %d: own camera %.6f, record %d -> %.6f (oracle %.6f, rel %.2e), slots %d (oracle %d)" %
              (b, own[b, 0], PERM[b], out[b, 0], ref["loss"], rel, int(out[b, 1]), int((ref["probs"] >= 1e-3).sum())))
        assert abs(out[b, 0] - own[b, 0]) > 1e-2 * own[b, 0], b          # the frame was computed with another camera ...
        assert rel <= LOSS_RTOL, (b, out[b, 0], ref["loss"])             # ... namely record PERM[b]
        assert int(out[b, 1]) == int((ref["probs"] >= 1e-3).sum()), b


@pytest.mark.parametrize("E, N, mode", SHAPES)
def test_equal_records_are_the_shared_camera_call(engine, E, N, mode):
    """A table whose records are all equal returns the bits of the existing call without a table -- training and forward -- so
    the NULL path and the table path run the same arithmetic."""
    frames, has, gts = _inputs(E, N, mode)
    f3 = frames[7]  # (every frame with frame 7's camera: the oracle needs at most a few thousand tries per hypothesis there)
    cams = _cams([f3] * 8)
    p_shared = _params(engine, f3, N, CALL0)
    out_s, g_s = _run_bwd(engine, frames, has, gts, None, p=p_shared)
    probs_s = engine.read_frames(api.BUF_BWD_PROBS, 8)
    out_t, g_t = _run_bwd(engine, frames, has, gts, cams)
    np.testing.assert_array_equal(out_t, out_s)
    np.testing.assert_array_equal(g_t, g_s)
    np.testing.assert_array_equal(engine.read_frames(api.BUF_BWD_PROBS, 8), probs_s)
    coords = torch.from_numpy(np.stack([f["coords"] for f in frames])).cuda()
    ha = torch.from_numpy(np.stack(has)).cuda()
    s_s = torch.empty(8, N, dtype=torch.float64, device="cuda")
    s_t = torch.empty_like(s_s)
    r_s = engine.forward_batch(coords, ha, p_shared, scores_out=s_s)
    r_t = engine.forward_batch(coords, ha, _batch_params(engine, f3, N, CALL0), scores_out=s_t, cams=cams)
    np.testing.assert_array_equal(r_t, r_s)
    assert torch.equal(s_t, s_s)


# ---------------------------------------------------------------- 5. chunking and overflow
def _overflow_inputs():
    """4 frames (N = 128, alpha 16) whose selections straddle a fresh context's 64 slots per frame: the oracle counts 81, 66, 128
    and 61 with these cameras, nothing within 2e-5 of the threshold."""
    frames = [S.make_frame(10 + b, shift=SHIFTS[b + 1], focal=FOCALS[b + 1]) for b in range(4)]
    has = [S.gating_assignment(f, 128) for f in frames]
    gts = [np.array(f["gt_pose"], np.float32) for f in frames]
    g0 = (np.random.default_rng(9).normal(size=(4,) + frames[0]["coords"].shape) * 1e-3).astype(np.float32)
    return frames, has, gts, g0


def test_chunks_keep_frame_b_with_camera_b(monkeypatch):
    """A slot-workspace budget of 32 MiB holds two 60x80 frames of 64 slots: the batch of 8 runs in 4 chunks, chunk k with the
    table offset by 2k, and returns the unchunked batch's bits."""
    monkeypatch.setenv("ESAC_BWD_BATCH_BUDGET_MB", "32")
    small = api.Engine(0)
    monkeypatch.delenv("ESAC_BWD_BATCH_BUDGET_MB")
    whole = api.Engine(0)
    for E, N, mode in SHAPES:
        frames, has, gts = _inputs(E, N, mode)
        cams = _cams(frames)
        out_w, g_w = _run_bwd(whole, frames, has, gts, cams)
        out_s, g_s = _run_bwd(small, frames, has, gts, cams)
        np.testing.assert_array_equal(out_s, out_w)
        np.testing.assert_array_equal(g_s, g_w)
        assert out_w[:, 1].min() >= 8
        with pytest.raises(RuntimeError):  # (the chunked context holds the last chunk's two frames only)
            small.read_frames(api.BUF_BWD_PROBS, 8)
        np.testing.assert_array_equal(small.read_frames(api.BUF_BWD_PROBS, 2), whole.read_frames(api.BUF_BWD_PROBS, 8)[6:])


def test_overflow_rerun_keeps_frame_b_with_camera_b(oracle, monkeypatch):
    """Fresh contexts start with 64 slots per frame.  `whole` overflows (frame 0 selects 81) and reruns all four frames at once;
    `small` (32 MiB: two frames at 64 slots, one at 96 or 128) aborts its first chunk, reruns frame 0 alone, then takes frames
    1, 2 (overflows again: 128) and 3 in chunks of their own -- table offsets 0, 1, 2, 3; `grown` has its workspace from an
    earlier call and overflows nowhere.  All three agree bit for bit, and with the oracle."""
    monkeypatch.setenv("ESAC_BWD_BATCH_BUDGET_MB", "32")
    small = api.Engine(0)
    monkeypatch.delenv("ESAC_BWD_BATCH_BUDGET_MB")
    whole, grown = api.Engine(0), api.Engine(0)
    frames, has, gts, g0 = _overflow_inputs()
    cams = _cams(frames)
    _run_bwd(grown, frames, has, gts, cams, call0=100, alpha=16.0)
    out_g, g_g = _run_bwd(grown, frames, has, gts, cams, call0=100, alpha=16.0, g0=g0)
    out_w, g_w = _run_bwd(whole, frames, has, gts, cams, call0=100, alpha=16.0, g0=g0)
    out_s, g_s = _run_bwd(small, frames, has, gts, cams, call0=100, alpha=16.0, g0=g0)
    counts = out_w[:, 1].astype(int)
    print("slots per frame", counts)
    assert counts.min() <= 64 < counts.max(), counts
    np.testing.assert_array_equal(out_w, out_g)
    np.testing.assert_array_equal(g_w, g_g)
    np.testing.assert_array_equal(out_s, out_g)
    np.testing.assert_array_equal(g_s, g_g)
    probs = whole.read_frames(api.BUF_BWD_PROBS, 4)
    refh = whole.read_frames(api.BUF_BWD_REF_HYPS, 4)
    losses = whole.read_frames(api.BUF_BWD_LOSSES, 4)
    for b, f in enumerate(frames):
        ref, g_ref = _oracle_bwd(oracle, f, has[b], gts[b], cams[b], 100 + b, alpha=16.0, g0=g0[b])
        _check_bwd_frame(b, out_w[b], g_w[b], ref, g_ref, probs[b], refh[b], losses[b], g_init=g0[b])


# ---------------------------------------------------------------- 6. errors
def test_bad_record_names_its_frame_and_launches_nothing(engine):
    frames, has, gts = _inputs(1, 64, "single")
    sc = torch.from_numpy(np.stack([f["coords"] for f in frames])).cuda()
    ha = torch.from_numpy(np.stack(has)).cuda()
    g = torch.from_numpy(np.random.default_rng(1).normal(size=tuple(sc.shape)).astype(np.float32)).cuda()
    g_keep = g.clone()
    p = _batch_params(engine, frames[0], 64, CALL0)
    for field, value in (("focal", 0.0), ("focal", -525.0), ("focal", float("nan")), ("shift_x", -2**31), ("shift_y", -(2**31 - 1))):
        cams = _cams(frames)
        cams[field][5] = value
        with pytest.raises(RuntimeError, match="frame 5") as ei:
            engine.backward_batch(sc, g, ha, np.stack(gts), 1.0, 100.0, 100.0, p, cams=cams)
        assert "status -4" in str(ei.value)
        torch.cuda.synchronize()
        assert torch.equal(g, g_keep), (field, value)
        rec = torch.full((8, api.RES_DOUBLES), -1.0, dtype=torch.float64, device="cuda")
        with pytest.raises(RuntimeError, match="frame 5"):
            engine.forward_batch(sc, ha, p, result_out=rec, cams=cams)
        torch.cuda.synchronize()
        assert bool((rec == -1.0).all()), (field, value)
    # the C entry points: a null table is the existing call, a batch size outside the range is caught before the table is read
    host = np.zeros((8, 4), np.float64)
    gt = np.stack(gts)
    slab = int(sc.stride(0))
    rc = engine.lib.esac_hip_backward_batch_cams(engine.ctx, 0, sc.data_ptr(), slab, g.data_ptr(), slab, ha.data_ptr(), gt.ctypes.data,
                                                 _cams(frames).ctypes.data, 1.0, 100.0, 100.0, C.byref(p), engine._stream(),
                                                 host.ctypes.data)
    assert rc == -4
    rc = engine.lib.esac_hip_forward_batch_cams(engine.ctx, 1025, sc.data_ptr(), slab, ha.data_ptr(), C.byref(p),
                                                _cams(frames).ctypes.data, engine._stream(), None, None, None)
    assert rc == -4
    torch.cuda.synchronize()
    assert torch.equal(g, g_keep)
    # and the same batch with a good table runs
    out = engine.backward_batch(sc, g, ha, gt, 1.0, 100.0, 100.0, p, cams=_cams(frames))
    assert (out[:, 3] == 0).all() and not torch.equal(g, g_keep)


# ---------------------------------------------------------------- 7. Python surface
def test_drop_in_surface_takes_sequences(engine, oracle):
    """esac.backward_batch / esac.forward_batch with lists, tensors, numpy arrays and mixed scalar / sequence arguments == the
    Engine-level calls with the table; the call counter advances by B."""
    import esac
    frames, has, gts = _inputs(4, 128, "gating")
    cams = _cams(frames)
    sc = torch.from_numpy(np.stack([f["coords"] for f in frames])).cuda()
    ha = torch.from_numpy(np.stack(has)).cuda()
    gt = torch.from_numpy(np.stack(gts))
    sx, sy = [s[0] for s in SHIFTS], [s[1] for s in SHIFTS]
    tail = (10.0, ALPHA, 0.5, 100.0, 8)
    want, g_want = _run_bwd(engine, frames, has, gts, cams)
    forms = [(sx, sy, FOCALS, 320.0, 240.0),                                                     # lists, scalar principal point
             (torch.tensor(sx), torch.tensor(sy, device="cuda"), torch.tensor(FOCALS), [320.0] * 8, np.full(8, 240.0)),
             (np.array(sx), np.array(sy, np.float64), np.array(FOCALS, np.float32), 320.0, torch.full((8,), 240.0))]
    for form in forms:
        esac.set_seed(SEED, CALL0)
        g = torch.zeros_like(sc)
        losses = esac.backward_batch(sc, g, ha, gt, 1.0, 100.0, 100.0, *form, *tail)
        assert esac.get_rng_state() == (SEED, CALL0 + 8)
        np.testing.assert_array_equal(np.array(losses), want[:, 0])
        np.testing.assert_array_equal(g.cpu().numpy(), g_want)
    # CPU tensors in, gradients accumulated into the caller's CPU tensor
    esac.set_seed(SEED, CALL0)
    g_cpu = torch.zeros(sc.shape)
    losses = esac.backward_batch(sc.cpu(), g_cpu, ha.cpu(), gt, 1.0, 100.0, 100.0, *forms[0], *tail)
    np.testing.assert_array_equal(np.array(losses), want[:, 0])
    np.testing.assert_array_equal(g_cpu.numpy(), g_want)
    # one per-frame argument only: the scalars are broadcast (here every frame with frame 0's shift and a common focal length)
    esac.set_seed(SEED, CALL0)
    g = torch.zeros_like(sc)
    losses = esac.backward_batch(sc, g, ha, gt, 1.0, 100.0, 100.0, 0, 0, 525.0, 320.0, [240.0] * 8, *tail)
    f0 = frames[0]
    shared, g_shared = _run_bwd(engine, frames, has, gts, None, p=_params(engine, f0, 128, CALL0, cam=cams[0]))
    np.testing.assert_array_equal(np.array(losses), shared[:, 0])
    np.testing.assert_array_equal(g.cpu().numpy(), g_shared)
    # forward
    res = engine.forward_batch(sc, ha, _batch_params(engine, f0, 128, CALL0), cams=cams)
    for form in forms:
        esac.set_seed(SEED, CALL0)
        poses = torch.zeros(8, 4, 4)
        experts = esac.forward_batch(sc, ha, poses, *form, *tail)
        assert esac.get_rng_state() == (SEED, CALL0 + 8)
        assert experts == [int(v) for v in res[:, api.RES_EXPERT]] == [b % 4 for b in range(8)]
        np.testing.assert_array_equal(poses.numpy(), res[:, api.RES_POSE:api.RES_POSE + 16].astype(np.float32).reshape(8, 4, 4))
        np.testing.assert_array_equal(esac.last_result()["result"][:, :31], res[:, :31])
    # a validation error spends no call counter
    esac.set_seed(SEED, CALL0)
    with pytest.raises(RuntimeError, match="focalLength"):
        esac.forward_batch(sc, ha, torch.zeros(8, 4, 4), sx, sy, FOCALS[:7], 320.0, 240.0, *tail)
    assert esac.get_rng_state() == (SEED, CALL0)


# ---------------------------------------------------------------- 8. harness.train_batch
class _BatchExpert(torch.nn.Module):
    """A learnable [B,3,h,w] map: the network side is elementwise, so it rounds the same whatever the batch."""

    def __init__(self, maps):
        super().__init__()
        self.map = torch.nn.Parameter(torch.from_numpy(np.ascontiguousarray(maps)).cuda())
        self.calls = 0

    def forward(self, images):
        self.calls += 1
        assert images.size(0) == self.map.size(0)
        return self.map


class _BatchGating(torch.nn.Module):
    def __init__(self, logits):
        super().__init__()
        self.logits = torch.nn.Parameter(torch.tensor(logits, dtype=torch.float32).cuda())

    def forward(self, images):
        return torch.log_softmax(self.logits, dim=1)


def test_train_batch_equals_single_backward_calls(monkeypatch):
    """train_batch with given shifts and assignments against B single esac.backward calls from the same call counter, each fed
    row b of the same maps, frame b's assignment, shift and focal length, on a context that refines one workgroup per slot."""
    import esac
    from esac_amd import harness
    monkeypatch.setenv("ESAC_SLOT_TEAMS", "0")
    monkeypatch.setitem(api._state, "engines", {0: api.Engine(0)})
    monkeypatch.delenv("ESAC_SLOT_TEAMS")
    E, N, B = 4, 128, 8
    frames, has, gts = _inputs(E, N, "gating")
    has = [h.copy() for h in has]
    for b in range(B):
        has[b][has[b] == (b + 2) % E] = b % E   # expert (b + 2) % 4 is inactive in frame b
    has[0][:] = 0                               # ... and frame 0 uses expert 0 only
    e_hyps = torch.from_numpy(np.stack(has)).cuda()
    maps = np.stack([f["coords"] for f in frames])  # [B,E,3,h,w]
    experts = [_BatchExpert(maps[:, e]) for e in range(E)]
    gating = _BatchGating(np.random.default_rng(3).normal(size=(B, E)))
    images = torch.zeros(B, 3, 480, 640, device="cuda")
    esac.set_seed(SEED, CALL0)
    out = harness.train_batch(images, np.stack(gts), gating, experts, FOCALS, hypotheses=N, shifts=SHIFTS, e_hyps=e_hyps)
    assert esac.get_rng_state() == (SEED, CALL0 + B)
    assert [e.calls for e in experts] == [1] * E and out["pads"] == SHIFTS
    assert tuple(out["prediction"].shape) == (B, E, 3, 60, 80) and tuple(out["e_hist"].shape) == (B, E)
    np.testing.assert_array_equal(out["e_hyps"].cpu().numpy(), np.stack(has))
    # the yardstick: B single calls
    esac.set_seed(SEED, CALL0)
    sc = torch.from_numpy(maps).cuda()
    for b in range(B):
        gb = torch.zeros_like(sc[b])
        loss = esac.backward(sc[b], gb, e_hyps[b], torch.from_numpy(gts[b]), 1.0, 100.0, 100.0, SHIFTS[b][0], SHIFTS[b][1],
                             FOCALS[b], 320.0, 240.0, 10.0, 100.0, 0.5, 100.0, 8)
        assert out["losses"][b] == loss, (b, out["losses"][b], loss)
        gb = gb.cpu().numpy()
        np.testing.assert_array_equal(out["prediction_gradients"][b].cpu().numpy(), gb, err_msg="frame %d" % b)
        hist = np.bincount(has[b], minlength=E).astype(np.float32)
        np.testing.assert_array_equal(out["e_hist"][b].cpu().numpy(), hist)
        for e in range(E):
            np.testing.assert_array_equal(experts[e].map.grad[b].cpu().numpy(), gb[e], err_msg="frame %d expert %d" % (b, e))
            if hist[e] == 0:
                assert not experts[e].map.grad[b].any(), (b, e)
        assert hist[(b + 2) % E] == 0 and np.abs(gb).max() > 0
    # gating: d/d log p of row b = loss_b * e_hist_b, pushed through log_softmax by autograd
    want = np.float32(out["losses"])[:, None] * out["e_hist"].cpu().numpy()
    leaf = gating.logits.detach().clone().requires_grad_(True)
    torch.log_softmax(leaf, dim=1).backward(torch.from_numpy(want).cuda())
    np.testing.assert_array_equal(gating.logits.grad.cpu().numpy(), leaf.grad.cpu().numpy())
    assert np.abs(want).max() > 0


def test_train_batch_draws_shifts_and_assignments_itself():
    """No shifts, no assignments: train_batch draws both from the seeded generator.  Checked: what does not depend on the order
    of the draws."""
    import esac
    from esac_amd import harness
    E, N, B = 4, 96, 8
    frames, _, gts = _inputs(E, N, "gating")
    maps = np.stack([f["coords"] for f in frames])
    experts = [_BatchExpert(maps[:, e]) for e in range(E)]
    logits = np.zeros((B, E))
    for b in range(B):
        logits[b, b % E] = 4.0
    gating = _BatchGating(logits)
    gen = torch.Generator(device="cuda").manual_seed(5)
    esac.set_seed(SEED, 700)
    out = harness.train_batch(torch.zeros(B, 3, 480, 640, device="cuda"), np.stack(gts), gating, experts, FOCALS, hypotheses=N,
                              generator=gen)
    assert esac.get_rng_state() == (SEED, 700 + B)
    assert tuple(out["e_hyps"].shape) == (B, N)
    np.testing.assert_array_equal(out["e_hist"].sum(dim=1).cpu().numpy(), np.full(B, N, np.float32))
    assert len(out["pads"]) == B and all(-4 <= v <= 4 for pad in out["pads"] for v in pad)
    assert len(out["losses"]) == B and all(np.isfinite(v) and v > 0 for v in out["losses"])
    assert gating.logits.grad is not None and torch.isfinite(gating.logits.grad).all()
    # the --expertselection form: one expert per frame, its log-probability takes the frame's loss
    for e in experts:
        e.map.grad = None
    gating.logits.grad = None
    out = harness.train_batch(torch.zeros(B, 3, 480, 640, device="cuda"), np.stack(gts), gating, experts, FOCALS, hypotheses=N,
                              generator=gen, expert_selection=True)
    assert esac.get_rng_state() == (SEED, 700 + 2 * B)
    hist = out["e_hist"].cpu().numpy()
    assert ((hist == N).sum(axis=1) == 1).all() and (hist.sum(axis=1) == N).all()
    assert all(np.isfinite(v) and v > 0 for v in out["losses"])
