"""The winner's refined pose of a training call as a forward record (esac_hip_set_bwd_pose_records; k_bwd_pose_record).

Expected values come from code that existed before the feature: a BLOCKING `engine.forward_device` under ESAC_FLAG_EXACT_SCORES at
the same (seed, call + b) and camera, the CPU oracle's forward call, and the training call's own stage buffers and record.  Bars:

    HYP, EXPERT, REF_STEPS, INLIERS, LM_ITERS   equal to the forward call's and to the oracle's
    SCORE                                        bit-equal to BUF_SCORES[win]; rel 1e-12 to the forward call's
    PROB                                         bit-equal to BUF_BWD_PROBS[win]
    ENTROPY                                      bit-equal to the call's own record (h_out[2] / d_out[b,2])
    PROB, ENTROPY, CONTENDERS                    1e-10 to the forward call's (every score exact on both sides)
    RVEC|TVEC                                    1e-8 to the forward call's (tests/test_gpu_backward.py: the slot route and the forward's
                                                 team sum the LM moments in different orders), 1e-6 to the oracle's (the bar of its
                                                 BUF_BWD_REF_HYPS comparison)
    POSE                                         1e-8 + one float32 ulp of the entry's magnitude to the forward call's RES_POSE

Grids: 24x32 and 60x80 (plus one odd 23x31 grid with a shift: the scalar error pass).
"""

import numpy as np
import pytest
import torch

from esac_amd import api, harness
from esac_amd import synthetic as S
from tests.test_eval_math_host import BAR as EVAL_BAR
from tests.test_eval_math_host import FIGURES
from tests.test_gpu_backward_batch import _gt, _overflow_inputs, _params

pytestmark = pytest.mark.gpu

DISCRETE = (api.RES_HYP, api.RES_EXPERT, api.RES_REF_STEPS, api.RES_INLIERS, api.RES_LM_ITERS)
SENTINEL = -777.25


def _small(k, **kw):
    return S.make_frame(k, H=24, W=32, sub=20, **kw)


def _forward(eng, f, ha, alpha, call, seed=1305, **kw):
    """The blocking forward call at the same key and camera, every score exact (what PROB / ENTROPY / CONTENDERS are held against)."""
    return eng.forward_device(torch.from_numpy(f["coords"]).cuda(), torch.from_numpy(ha).cuda(),
                              _params(eng, f, len(ha), alpha, call, seed=seed, exact_scores=True, **kw))


def _oracle_forward(oracle, f, ha, alpha, call, seed=1305, **kw):
    o = oracle.forward(f["coords"], ha, shift_x=f["shift"][0], shift_y=f["shift"][1], focal=f["focal"], ppx=f["ppx"], ppy=f["ppy"],
                       sub_sampling=f["sub"], inlier_alpha=alpha, seed=seed, call=call, **kw)
    o["last_inliers"] = int(o["inlier_counts"][o["ref_steps"] - 1]) if o["ref_steps"] > 0 else 0  # of the last ACCEPTED step
    return o


def _check_distribution(rec, fwd, scores, probs, entropy, N):
    """The fields every record carries, slot or no slot."""
    win = int(rec[api.RES_HYP])
    assert rec[api.RES_HYP] == fwd[api.RES_HYP] and rec[api.RES_EXPERT] == fwd[api.RES_EXPERT]
    assert rec[api.RES_SCORE].tobytes() == scores[win].tobytes()
    assert abs(rec[api.RES_SCORE] - fwd[api.RES_SCORE]) <= 1e-12 * abs(fwd[api.RES_SCORE])
    assert rec[api.RES_PROB].tobytes() == probs[win].tobytes()
    assert rec[api.RES_ENTROPY].tobytes() == np.float64(entropy).tobytes()
    assert abs(rec[api.RES_PROB] - fwd[api.RES_PROB]) <= 1e-10 and abs(rec[api.RES_ENTROPY] - fwd[api.RES_ENTROPY]) <= 1e-10
    assert rec[api.RES_CONTENDERS] == fwd[api.RES_CONTENDERS] == float(N)
    return win


def _check_record(rec, fwd, ora, scores, probs, entropy, N, what=""):
    """A record whose winner holds a slot, against the forward call, the oracle and the call's own buffers.  Returns the figures."""
    win = _check_distribution(rec, fwd, scores, probs, entropy, N)
    d_rvec = float(np.abs(rec[api.RES_RVEC:api.RES_RVEC + 6] - fwd[api.RES_RVEC:api.RES_RVEC + 6]).max())
    pose, want = rec[api.RES_POSE:api.RES_POSE + 16], fwd[api.RES_POSE:api.RES_POSE + 16]
    ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
    d_pose = float(np.max((np.abs(pose - want) - 1e-8) / ulp))
    d_ora = float(np.abs(rec[api.RES_RVEC:api.RES_RVEC + 6] - ora["refined"]).max()) if ora is not None else 0.0
    print("%s winner %d: |rvec,tvec - forward| %.2e, - oracle %.2e; pose (diff - 1e-8) / ulp32 worst %.2f; steps %d, inliers %d, LM %d"
          % (what, win, d_rvec, d_ora, d_pose, rec[api.RES_REF_STEPS], rec[api.RES_INLIERS], rec[api.RES_LM_ITERS]))
    assert rec[api.RES_VALID] == 1.0
    for k in DISCRETE:
        assert rec[k] == fwd[k], (what, k, rec[k], fwd[k])
    if ora is not None:
        assert (int(rec[api.RES_HYP]), int(rec[api.RES_EXPERT]), int(rec[api.RES_REF_STEPS]), int(rec[api.RES_INLIERS]), int(rec[api.RES_LM_ITERS])) == \
               (ora["winner"], ora["expert"], ora["ref_steps"], ora["last_inliers"], ora["lm_iters"]), what
        assert d_ora <= 1e-6, (what, d_ora)
    assert d_rvec <= 1e-8, (what, d_rvec)
    assert (np.abs(pose - want) <= 1e-8 + ulp).all(), (what, pose, want)
    assert (pose == pose.astype(np.float32).astype(np.float64)).all()  # floats, as forward writes them
    return win


def _check_no_slot(rec, fwd, scores, probs, entropy, N):
    _check_distribution(rec, fwd, scores, probs, entropy, N)
    assert rec[api.RES_VALID] == 0.0
    assert np.isnan(rec[api.RES_RVEC:api.RES_POSE + 16]).all()
    assert rec[api.RES_REF_STEPS] == 0.0 and rec[api.RES_INLIERS] == 0.0 and rec[api.RES_LM_ITERS] == 0.0


def _single(eng, f, ha, gt, alpha, call, seed=1305, rec=None, armed=True, **kw):
    """One blocking esac_hip_backward, armed with a device record tensor; returns everything the checks read."""
    sc, hat = torch.from_numpy(f["coords"]).cuda(), torch.from_numpy(ha).cuda()
    g = torch.zeros_like(sc)
    if rec is None:
        rec = torch.full((32,), SENTINEL, dtype=torch.float64, device="cuda")
    out = eng.backward_device(sc, g, hat, gt, 1.0, 100.0, 100.0, _params(eng, f, len(ha), alpha, call, seed=seed, **kw),
                              pose_record=rec if armed else None)
    return dict(out=out, grad=g.cpu().numpy(), rec=rec.cpu().numpy(), scores=eng.read(api.BUF_SCORES), probs=eng.read(api.BUF_BWD_PROBS),
                slots=eng.read(api.BUF_BWD_SLOTS)[:int(out[1])])


# (name, frame factory, N, mode, alpha, call, extra make_params / oracle keywords, slots the case is there for)
SINGLE = {
    "n1": (lambda: _small(5), 1, "single", 100.0, 0, {}, 1),
    "n5": (lambda: _small(5), 5, "single", 100.0, 4, {}, 1),
    "n64_60x80": (lambda: S.make_frame(81), 64, "single", 100.0, 6, {}, 1),
    "three_experts_gating": (lambda: S.make_frame(31, E=3, true_expert=1), 96, "gating", 10.0, 2, {}, 1),
    "odd_grid_shift": (lambda: S.make_frame(41, H=23, W=31, sub=20, shift=(7, -5)), 64, "single", 20.0, 1, {}, 1),
    # the argmax strides six times over the 256 threads; 252 slots per the oracle: the bisection walks a long list
    "n1500_24x32": (lambda: _small(242), 1500, "single", 4.0, 2, {}, 65),
    # the shape of test_backward_flat_distribution_many_slots: every one of the 128 hypotheses owns a slot
    "flat_many_slots": (lambda: S.make_frame(10), 128, "single", 2.0, 0, {}, 65),
}


@pytest.mark.parametrize("name", list(SINGLE))
def test_single_call_record_is_the_forward_call(engine, oracle, name):
    factory, N, mode, alpha, call, kw, min_slots = SINGLE[name]
    f = factory()
    if mode == "gating":  # (make_frame's own gating puts every draw of so few on the true expert: a flatter one here)
        ha = np.random.default_rng(31).choice(3, size=N, p=[0.25, 0.5, 0.25]).astype(np.int64)
    else:
        ha = S.gating_assignment(f, N, mode=mode)
    gt = _gt(f, 7, noise=0.03)
    got = _single(engine, f, ha, gt, alpha, call, **kw)
    assert len(got["slots"]) >= min_slots, len(got["slots"])
    fwd = _forward(engine, f, ha, alpha, call, **kw)
    ora = _oracle_forward(oracle, f, ha, alpha, call, **kw)
    win = _check_record(got["rec"], fwd, ora, got["scores"], got["probs"], got["out"][2], N, what=name)
    assert win in got["slots"]
    if name == "three_experts_gating":
        assert len(set(ha.tolist())) > 1 and int(got["rec"][api.RES_EXPERT]) == int(ha[win])


def test_winner_without_a_slot(engine, oracle):
    """N = 2048 on a flat distribution (alpha 1e-4): every probability is 1/2048 < 1e-3, nothing is selected -- VALID 0, a NaN pose,
    zero steps, and HYP, EXPERT, SCORE, PROB, ENTROPY still the forward call's."""
    f = _small(240)
    ha = S.gating_assignment(f, 2048)
    got = _single(engine, f, ha, _gt(f, 340), 1e-4, 1)
    assert got["out"][1] == 0.0 and got["probs"].max() < 1e-3
    fwd = _forward(engine, f, ha, 1e-4, 1)
    _check_no_slot(got["rec"], fwd, got["scores"], got["probs"], got["out"][2], 2048)
    assert int(got["rec"][api.RES_HYP]) == _oracle_forward(oracle, f, ha, 1e-4, 1)["winner"]


def test_tied_scores_go_to_the_first_index(engine, oracle):
    """A map of pure noise, 3 tries and a 1 px clamp: several hypotheses share the highest score bit for bit (ten in the oracle's
    arithmetic, seven on the device); the record's HYP is the forward call's -- the first of the device's."""
    f = _small(104, outlier_frac=1.0)
    ha = S.gating_assignment(f, 48)
    kw = dict(max_tries=3, max_reproj=1.0)
    got = _single(engine, f, ha, _gt(f, 4), 5.0, 3, **kw)
    tied = np.flatnonzero(got["scores"] == got["scores"].max())
    assert len(tied) >= 2, tied
    fwd = _forward(engine, f, ha, 5.0, 3, **kw)
    ora = _oracle_forward(oracle, f, ha, 5.0, 3, **kw)
    rec = got["rec"]
    ora_tied = np.flatnonzero(ora["scores"] == ora["scores"].max())
    print("tied: record %d, forward %d, oracle %d; device ties %r (score %r), oracle ties %r (score %r)"
          % (rec[api.RES_HYP], fwd[api.RES_HYP], ora["winner"], tied.tolist(), got["scores"].max(), ora_tied.tolist(), ora["scores"].max()))
    # (not the oracle's winner: the 48 scores of this map agree to 1e-13, so WHICH of them are bit-equal maxima is a matter of the
    # summation order of the exact score, and the oracle's differs from the device's -- 4.945149037924179 against ...2413 on the
    # device; the forward call and the training call share the device's order)
    assert int(rec[api.RES_HYP]) == int(fwd[api.RES_HYP]) == int(tied[0])
    assert len(ora_tied) >= 2 and abs(ora["scores"].max() - got["scores"].max()) <= 1e-12 * ora["scores"].max()
    _check_distribution(rec, fwd, got["scores"], got["probs"], got["out"][2], 48)
    assert rec[api.RES_VALID] == 1.0 and all(rec[k] == fwd[k] for k in DISCRETE)
    print("tied: %d share the maximum, winner %d; |rvec,tvec - forward| %.2e" % (len(tied), tied[0], np.abs(rec[3:9] - fwd[3:9]).max()))


# ---------------------------------------------------------------- batches
def _cams(frames):
    return api.make_cams([f["shift"][0] for f in frames], [f["shift"][1] for f in frames], [f["focal"] for f in frames],
                         [f["ppx"] for f in frames], [f["ppy"] for f in frames])


def _cam_batch():
    """B = 3, three experts, a shift and a focal length per frame."""
    shifts, focals = [(0, 0), (4, -4), (-3, 2)], [525.0, 585.0, 480.0]
    frames = [S.make_frame(1800 + b, E=3, true_expert=b % 3, shift=shifts[b], focal=focals[b]) for b in range(3)]
    has = [S.gating_assignment(f, 64, mode="gating") for f in frames]
    gts = [_gt(f, 1850 + b) for b, f in enumerate(frames)]
    return frames, has, gts


def _batch(eng, frames, has, gts, alpha, call0, cams=None, g0=None, rec=None, armed=True, asynchronous=False):
    sc = torch.from_numpy(np.stack([f["coords"] for f in frames])).cuda()
    ha = torch.from_numpy(np.stack(has)).cuda()
    B = len(has)
    g = torch.from_numpy(g0.copy()).cuda() if g0 is not None else torch.zeros(sc.shape, dtype=torch.float32, device="cuda")
    if rec is None:
        rec = torch.full((B, 32), SENTINEL, dtype=torch.float64, device="cuda")
    p = _params(eng, frames[0], ha.shape[1], alpha, call0)
    if asynchronous:
        eng.arm_pose_records(rec if armed else None)
        out = eng.backward_batch_async(sc, g, ha, torch.from_numpy(np.stack(gts)).cuda(), 1.0, 100.0, 100.0, p, cams=cams)
        torch.cuda.synchronize()
        out = out.cpu().numpy()
    else:
        out = eng.backward_batch(sc, g, ha, np.stack(gts), 1.0, 100.0, 100.0, p, cams=cams, pose_records=rec if armed else None)
    return dict(out=out, grad=g.cpu().numpy(), rec=rec.cpu().numpy())


def _check_batch(eng, oracle, frames, has, got, alpha, call0, what="batch"):
    """Every row against the blocking forward call and the oracle at call0 + b, and against the batch's own buffers (read first)."""
    B = len(has)
    scores, probs = eng.read_forward_frames(api.BUF_SCORES, B), eng.read_frames(api.BUF_BWD_PROBS, B)
    for b, f in enumerate(frames):
        fwd = _forward(eng, f, has[b], alpha, call0 + b)
        ora = _oracle_forward(oracle, f, has[b], alpha, call0 + b)
        _check_record(got["rec"][b], fwd, ora, scores[b], probs[b], got["out"][b, 2], len(has[b]), what="%s frame %d" % (what, b))


def test_blocking_batch_with_per_frame_cameras(engine, oracle):
    frames, has, gts = _cam_batch()
    got = _batch(engine, frames, has, gts, 20.0, 61, cams=_cams(frames))
    assert got["out"][:, 1].min() >= 1
    _check_batch(engine, oracle, frames, has, got, 20.0, 61)
    assert len({int(r[api.RES_HYP]) for r in got["rec"]}) > 1  # (rows are told apart)


def test_chunked_batch_puts_frame_b_into_row_b(oracle, monkeypatch):
    """A slot-workspace budget of 16 MiB holds one 60x80 frame of 64 slots: three chunks, three launch sets, and row b is still
    frame b's -- the unchunked batch's rows bit for bit."""
    monkeypatch.setenv("ESAC_BWD_BATCH_BUDGET_MB", "16")
    small = api.Engine(0)
    monkeypatch.delenv("ESAC_BWD_BATCH_BUDGET_MB")
    whole = api.Engine(0)
    frames, has, gts = _cam_batch()
    got = _batch(small, frames, has, gts, 20.0, 61, cams=_cams(frames))
    with pytest.raises(RuntimeError):
        small.read_frames(api.BUF_BWD_PROBS, 3)  # (it did run in chunks: the buffers hold the last one only)
    want = _batch(whole, frames, has, gts, 20.0, 61, cams=_cams(frames))
    _check_batch(whole, oracle, frames, has, want, 20.0, 61, what="unchunked")
    np.testing.assert_array_equal(got["rec"], want["rec"])
    np.testing.assert_array_equal(got["out"], want["out"])
    assert len({int(r[api.RES_HYP]) for r in got["rec"]}) > 1


def test_overflow_rerun_leaves_every_row_valid(oracle):
    """Frame 0 selects 79 slots, a fresh context holds 64 per frame: the first pass is aborted, the chunk runs again with a grown
    workspace, and the second pass overwrites every row."""
    eng = api.Engine(0)
    frames, has, gts, g0 = _overflow_inputs()
    got = _batch(eng, frames, has, gts, 16.0, 100, g0=g0)
    counts = got["out"][:, 1].astype(int)
    assert counts.min() <= 64 < counts.max(), counts
    assert (got["rec"][:, api.RES_VALID] == 1.0).all()
    _check_batch(eng, oracle, frames, has, got, 16.0, 100, what="overflow")


def test_asynchronous_batch_with_a_singular_ground_truth(engine, oracle):
    """B = 3, frame 1's ground-truth pose is all zeros: that frame selects nothing -- VALID 0, the distribution's fields stand, ENTROPY
    is the 0 its own record reports -- and frames 0 and 2 get their records."""
    frames, has, gts = _cam_batch()
    gts = [g.copy() for g in gts]
    gts[1][:] = 0.0
    got = _batch(engine, frames, has, gts, 20.0, 61, cams=_cams(frames), asynchronous=True)
    assert np.isnan(got["out"][1, 0]) and got["out"][1, 1:].tolist() == [0.0, 0.0, 2.0]
    scores, probs = engine.read_forward_frames(api.BUF_SCORES, 3), engine.read_frames(api.BUF_BWD_PROBS, 3)
    with pytest.raises(RuntimeError, match="frame 1 is singular"):
        engine.check()
    for b in (0, 2):
        fwd = _forward(engine, frames[b], has[b], 20.0, 61 + b)
        _check_record(got["rec"][b], fwd, _oracle_forward(oracle, frames[b], has[b], 20.0, 61 + b), scores[b], probs[b], got["out"][b, 2], 64,
                      what="async frame %d" % b)
    fwd = _forward(engine, frames[1], has[1], 20.0, 62)
    rec = got["rec"][1]
    assert rec[api.RES_VALID] == 0.0 and np.isnan(rec[api.RES_RVEC:api.RES_POSE + 16]).all() and rec[api.RES_ENTROPY] == 0.0 == got["out"][1, 2]
    assert rec[api.RES_HYP] == fwd[api.RES_HYP] and rec[api.RES_EXPERT] == fwd[api.RES_EXPERT]
    assert rec[api.RES_SCORE].tobytes() == scores[1][int(rec[api.RES_HYP])].tobytes() and rec[api.RES_PROB].tobytes() == probs[1][int(rec[api.RES_HYP])].tobytes()
    assert rec[api.RES_REF_STEPS] == 0.0 and rec[api.RES_INLIERS] == 0.0 and rec[api.RES_LM_ITERS] == 0.0


def _assert_eval_rows(got, want, what):
    """The comparison of tests/test_gpu_eval_batch.py (_assert_rows): figures within its bar, flags and copies equal."""
    for b in range(len(want)):
        np.testing.assert_array_equal(np.isnan(got[b]), np.isnan(want[b]), err_msg="%s frame %d: NaN pattern" % (what, b))
        diff = np.nan_to_num(np.abs(got[b, FIGURES] - want[b, FIGURES]))
        print("%s frame %d: worst figure difference %.3e (bar %.3e)" % (what, b, diff.max(), EVAL_BAR))
        assert diff.max() <= EVAL_BAR, (what, b, got[b], want[b])
        for col in (api.EVAL_POSE_OK, api.EVAL_CLASS_OK, api.EVAL_EXPERT, api.EVAL_HYP, api.EVAL_STATUS, 14, 15):
            assert got[b, col] == want[b, col], (what, b, col, got[b], want[b])


def test_eval_batch_right_behind_the_asynchronous_call(engine):
    """eval_batch enqueued behind the armed asynchronous call with no synchronisation between the two: its rows are eval_row_host on
    the poses of blocking forward calls."""
    frames, has, gts = _cam_batch()
    sc = torch.from_numpy(np.stack([f["coords"] for f in frames])).cuda()
    ha = torch.from_numpy(np.stack(has)).cuda()
    g = torch.zeros(sc.shape, dtype=torch.float32, device="cuda")
    gt = torch.from_numpy(np.stack(gts)).cuda()
    ge = torch.tensor([0, 1, 0], dtype=torch.int64, device="cuda")
    rec = torch.zeros((3, 32), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    engine.arm_pose_records(rec)
    engine.backward_batch_async(sc, g, ha, gt, 1.0, 100.0, 100.0, _params(engine, frames[0], 64, 20.0, 61), cams=_cams(frames))
    rows = engine.eval_batch(rec, gt, ge)
    torch.cuda.synchronize()
    engine.check()
    rows = rows.cpu().numpy()
    want = np.zeros((3, 16))
    for b, f in enumerate(frames):
        fwd = _forward(engine, f, has[b], 20.0, 61 + b)
        want[b] = harness.eval_row_host(fwd[api.RES_POSE:api.RES_POSE + 16].astype(np.float32).reshape(4, 4), gts[b],
                                        int(fwd[api.RES_EXPERT]), int(fwd[api.RES_HYP]), int(ge[b]))
    _assert_eval_rows(rows, want, "eval behind the asynchronous call")
    assert (rows[:, api.EVAL_STATUS] == 0.0).all() and set(rows[:, api.EVAL_CLASS_OK]) <= {0.0, 1.0}


# ---------------------------------------------------------------- unarmed calls, one-shot, frames < B
BWD_BUFFERS = (api.BUF_BWD_PROBS, api.BUF_BWD_LOSSES, api.BUF_BWD_REF_HYPS, api.BUF_BWD_SCORE_GRADS, api.BUF_BWD_SLOTS,
               api.BUF_BWD_SLOT_INFO, api.BUF_BWD_DLOSS)


def _valid_rows(buf, which, n_sel):
    """Of the slot tables only the first n_sel rows are defined."""
    return buf[..., :n_sel, :] if which in (api.BUF_BWD_SLOT_INFO, api.BUF_BWD_DLOSS) else buf[..., :n_sel] if which == api.BUF_BWD_SLOTS else buf


def test_unarmed_single_call_is_bit_equal_and_writes_nothing(engine):
    """Armed, then unarmed at the same key: loss record, gradients and every BUF_BWD_* buffer bit for bit; the record tensor of the
    armed call, refilled with a sentinel, stays untouched -- the arming is one-shot."""
    f = S.make_frame(81)
    ha = S.gating_assignment(f, 64)
    gt = _gt(f, 7, noise=0.03)
    rec = torch.full((32,), SENTINEL, dtype=torch.float64, device="cuda")
    armed = _single(engine, f, ha, gt, 30.0, 6, rec=rec)
    n = int(armed["out"][1])
    armed_bufs = {w: _valid_rows(engine.read(w), w, n).copy() for w in BWD_BUFFERS}
    slabs = [engine.read_slabs(w, n).copy() for w in (api.BUF_BWD_PATH1, api.BUF_BWD_PATH2)]
    assert armed["rec"][api.RES_VALID] == 1.0 and not (armed["rec"] == SENTINEL).any()
    rec.fill_(SENTINEL)
    plain = _single(engine, f, ha, gt, 30.0, 6, rec=rec, armed=False)
    assert (plain["rec"] == SENTINEL).all()
    np.testing.assert_array_equal(plain["out"], armed["out"])
    np.testing.assert_array_equal(plain["grad"], armed["grad"])
    assert np.abs(plain["grad"]).max() > 0
    for w in BWD_BUFFERS:
        np.testing.assert_array_equal(_valid_rows(engine.read(w), w, n), armed_bufs[w], err_msg=str(w))
    for w, want in zip((api.BUF_BWD_PATH1, api.BUF_BWD_PATH2), slabs):
        np.testing.assert_array_equal(engine.read_slabs(w, n), want)


@pytest.mark.parametrize("asynchronous", [False, True], ids=["blocking", "asynchronous"])
def test_unarmed_batch_is_bit_equal_and_writes_nothing(engine, asynchronous):
    frames, has, gts = _cam_batch()
    rec = torch.full((3, 32), SENTINEL, dtype=torch.float64, device="cuda")
    armed = _batch(engine, frames, has, gts, 20.0, 61, cams=_cams(frames), rec=rec, asynchronous=asynchronous)
    counts = armed["out"][:, 1].astype(int)
    armed_bufs = {w: engine.read_frames(w, 3) for w in BWD_BUFFERS}
    assert (armed["rec"][:, api.RES_VALID] == 1.0).all()
    rec.fill_(SENTINEL)
    plain = _batch(engine, frames, has, gts, 20.0, 61, cams=_cams(frames), rec=rec, armed=False, asynchronous=asynchronous)
    assert (plain["rec"] == SENTINEL).all()
    np.testing.assert_array_equal(plain["out"], armed["out"])
    np.testing.assert_array_equal(plain["grad"], armed["grad"])
    assert np.abs(plain["grad"]).max() > 0
    for w in BWD_BUFFERS:
        now = engine.read_frames(w, 3)
        for b in range(3):
            np.testing.assert_array_equal(_valid_rows(now[b], w, counts[b]), _valid_rows(armed_bufs[w][b], w, counts[b]), err_msg="%s frame %d" % (w, b))


def test_too_few_armed_frames_are_refused_before_anything_runs(engine):
    """frames < B: -4, the prefilled gradients untouched, nothing written; the refused call has consumed the arming, so the next
    call is an unarmed one."""
    frames, has, gts = _cam_batch()
    sc = torch.from_numpy(np.stack([f["coords"] for f in frames])).cuda()
    ha = torch.from_numpy(np.stack(has)).cuda()
    g0 = (np.random.default_rng(2).normal(size=tuple(sc.shape)) * 1e-3).astype(np.float32)
    p = _params(engine, frames[0], 64, 20.0, 61)
    rec = torch.full((3, 32), SENTINEL, dtype=torch.float64, device="cuda")
    lib = engine.lib
    assert lib.esac_hip_set_bwd_pose_records(engine.ctx, rec.data_ptr(), 0) == -4  # (a buffer of no frames cannot be armed at all)
    for route in ("blocking", "asynchronous"):
        g = torch.from_numpy(g0.copy()).cuda()
        assert lib.esac_hip_set_bwd_pose_records(engine.ctx, rec.data_ptr(), 2) == 0
        with pytest.raises(RuntimeError, match=r"armed 2 frame\(s\), the call has 3.*\[status -4\]"):
            if route == "blocking":
                engine.backward_batch(sc, g, ha, np.stack(gts), 1.0, 100.0, 100.0, p)
            else:
                engine.backward_batch_async(sc, g, ha, torch.from_numpy(np.stack(gts)).cuda(), 1.0, 100.0, 100.0, p)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(g.cpu().numpy(), g0)
        assert (rec.cpu().numpy() == SENTINEL).all()
        out = engine.backward_batch(sc, g, ha, np.stack(gts), 1.0, 100.0, 100.0, p)  # the call after it: unarmed, and it runs
        assert out[:, 1].min() >= 1 and (rec.cpu().numpy() == SENTINEL).all()
        assert not np.array_equal(g.cpu().numpy(), g0)
    # NULL disarms
    assert lib.esac_hip_set_bwd_pose_records(engine.ctx, rec.data_ptr(), 3) == 0 and lib.esac_hip_set_bwd_pose_records(engine.ctx, None, 0) == 0
    engine.backward_batch(sc, torch.zeros_like(sc), ha, np.stack(gts), 1.0, 100.0, 100.0, p)
    assert (rec.cpu().numpy() == SENTINEL).all()


def test_cpu_record_tensors_of_the_blocking_calls(engine):
    """The blocking calls also take a CPU tensor (copied after their own wait): the device tensor's bits."""
    import esac
    frames, has, gts = _cam_batch()
    f = frames[0]
    args = (1.0, 100.0, 100.0, f["shift"][0], f["shift"][1], f["focal"], f["ppx"], f["ppy"], 10.0, 20.0, 0.5, 100.0, f["sub"])
    sc, ha, gt = torch.from_numpy(f["coords"]).cuda(), torch.from_numpy(has[0]).cuda(), torch.from_numpy(gts[0])
    on_dev, on_cpu = torch.zeros(32, dtype=torch.float64, device="cuda"), torch.zeros(64, dtype=torch.float64)[::2]
    for rec in (on_dev, on_cpu):
        esac.set_seed(1305, 61)
        esac.set_pose_records(rec)
        esac.backward(sc, torch.zeros_like(sc), ha, gt, *args)
    assert on_cpu[api.RES_VALID] == 1.0 and torch.equal(on_dev.cpu(), on_cpu)
    scb = torch.from_numpy(np.stack([x["coords"] for x in frames])).cuda()
    hab, gtb = torch.from_numpy(np.stack(has)).cuda(), torch.from_numpy(np.stack(gts))
    cam = ([x["shift"][0] for x in frames], [x["shift"][1] for x in frames], [x["focal"] for x in frames], f["ppx"], f["ppy"])
    recs = [torch.zeros(3, 32, dtype=torch.float64, device="cuda"), torch.zeros(3, 32, dtype=torch.float64)]
    for rec in recs:
        esac.set_seed(1305, 61)
        esac.backward_batch(scb, torch.zeros_like(scb), hab, gtb, 1.0, 100.0, 100.0, *cam, 10.0, 20.0, 0.5, 100.0, f["sub"], poseRecords=rec)
    assert (recs[1][:, api.RES_VALID] == 1.0).all() and torch.equal(recs[0].cpu(), recs[1])
    assert recs[1][0, api.RES_HYP] == on_cpu[api.RES_HYP]  # frame 0 of the batch is the single call at the same counter


# ---------------------------------------------------------------- harness.train_batch(evaluate=True)
class _Expert(torch.nn.Module):
    def __init__(self, maps):
        super().__init__()
        self.map = torch.nn.Parameter(torch.from_numpy(np.ascontiguousarray(maps)).cuda())

    def forward(self, images):
        return self.map * 1.0


class _Gating(torch.nn.Module):
    """Two layers on the image mean: B x 3 -> 8 -> E (the images are zeros: the biases decide)."""

    def __init__(self, E):
        super().__init__()
        torch.manual_seed(3)
        self.net = torch.nn.Sequential(torch.nn.Linear(3, 8), torch.nn.Tanh(), torch.nn.Linear(8, E)).cuda()

    def forward(self, images):
        return torch.log_softmax(self.net(images.mean(dim=(2, 3))), dim=1)


def test_train_batch_evaluate_equals_localize_batch(engine, monkeypatch):
    """harness.train_batch(evaluate=True, asynchronous=True, all_experts=True): records and eval rows stay on the device, and the
    rows are localize_batch's on the same e_hyps and keys (the forward batch + eval_batch of the test loop)."""
    import esac
    monkeypatch.setitem(api._state, "engines", {0: engine})
    E, N, B = 3, 64, 3
    frames = [S.make_frame(1900 + b, E=E, true_expert=b % E) for b in range(B)]
    e_hyps = torch.from_numpy(np.stack([S.gating_assignment(f, N, mode="gating") for f in frames])).cuda()
    maps = np.stack([f["coords"] for f in frames])
    experts, gating = [_Expert(maps[:, e]) for e in range(E)], _Gating(E)
    images = torch.zeros(B, 3, 480, 640, device="cuda")
    gts = torch.from_numpy(np.stack([_gt(f, 1950 + b) for b, f in enumerate(frames)])).cuda()
    ge = torch.tensor([f["true_expert"] for f in frames], dtype=torch.int64, device="cuda")
    esac.set_seed(1305, 70)
    out = harness.train_batch(images, gts, gating, experts, 525.0, hypotheses=N, inlier_alpha=20.0, shifts=[(0, 0)] * B, e_hyps=e_hyps,
                              asynchronous=True, all_experts=True, evaluate=True, gt_experts=ge)
    assert out["records"].is_cuda and tuple(out["records"].shape) == (B, 32) and out["eval"].is_cuda and tuple(out["eval"].shape) == (B, 16)
    torch.cuda.synchronize()
    engine.check()
    assert experts[0].map.grad is not None and float(sum(x.map.grad.abs().max() for x in experts)) > 0
    esac.set_seed(1305, 70)
    want = harness.localize_batch(images, gating, experts, 525.0, gt_poses=gts, gt_experts=ge, hypotheses=N, inlier_alpha=20.0, e_hyps=e_hyps,
                                  asynchronous=True, all_experts=True)
    torch.cuda.synchronize()
    rows, want_rows = out["eval"].cpu().numpy(), want["eval"].cpu().numpy()
    assert (want_rows[:, api.EVAL_STATUS] == 0.0).all()
    _assert_eval_rows(rows, want_rows, "train_batch(evaluate=True)")
    rec, want_rec = out["records"].cpu().numpy(), want["records"].cpu().numpy()
    for k in DISCRETE:
        np.testing.assert_array_equal(rec[:, k], want_rec[:, k])
    # the blocking single step (it draws its own assignment): its row is eval_row_host on the forward call at its key
    esac.set_seed(1305, 90)
    gt0 = gts[0].cpu().numpy()
    one = harness.train_step(images[:1], gt0, lambda im: gating(images)[:1], [lambda im, e=e: experts[e](images)[:1] for e in range(E)],
                             525.0, hypotheses=N, inlier_alpha=20.0, shift=(0, 0), generator=torch.Generator(device="cuda").manual_seed(4),
                             evaluate=True, gt_expert=int(ge[0]))
    assert tuple(one["records"].shape) == (1, 32) and tuple(one["eval"].shape) == (1, 16) and esac.get_rng_state() == (1305, 91)
    p = engine.make_params(E, 60, 80, N, focal=525.0, ppx=320.0, ppy=240.0, inlier_alpha=20.0, seed=1305, call=90, exact_scores=True)
    fwd = engine.forward_device(one["prediction"].detach().contiguous(), one["e_hyps"].contiguous(), p)
    row = harness.eval_row_host(fwd[api.RES_POSE:api.RES_POSE + 16].astype(np.float32).reshape(4, 4), gt0, int(fwd[api.RES_EXPERT]),
                                int(fwd[api.RES_HYP]), int(ge[0]))
    _assert_eval_rows(one["eval"].cpu().numpy(), row[None], "train_step(evaluate=True)")
