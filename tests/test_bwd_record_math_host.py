"""bwd_record_math.hpp -- the arithmetic of k_bwd_pose_record (esac_hip_set_bwd_pose_records) -- compiled for the host
(tests/native/bwd_record_probe.cpp) and fed the CPU oracle's TRAINING stages (oracle.backward(want_stages=True)): the record it
assembles for the argmax hypothesis is held against the oracle's FORWARD call at the same (seed, call).

The premise this checks: a training call draws the forward call's hypotheses, scores them in the same arithmetic and refines every
hypothesis with p >= 1e-3 with the same refineHyp, so the winner's slot holds the forward call's refined pose.  Bars:
HYP, EXPERT, REF_STEPS, INLIERS, LM_ITERS equal; RVEC|TVEC, SCORE, PROB, ENTROPY bit-equal (one oracle, one arithmetic); every POSE
entry within one float32 ulp of its magnitude of oracle.forward's `pose` (the oracle's C sincos against the probe's C++ one: the
doubles may differ in their last bit, which can move the float rounding by one step).
"""
import ctypes as C
import subprocess

import numpy as np
import pytest

from esac_amd import api
from esac_amd import synthetic as S

# (make_frame seed, N, call): the oracle check the feature was proposed on
CASES = [(81, 64, 6), (91, 32, 0), (1001, 256, 3), (1002, 256, 4), (1003, 128, 9), (1004, 16, 1), (1005, 8, 2), (1006, 5, 7)]
SEED = 5


@pytest.fixture(scope="module")
def probe():
    from tests.native import build_bwd_record
    lib = C.CDLL(build_bwd_record.build())
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    lib.bwd_record_probe_winner.argtypes = [dp, C.c_int]
    lib.bwd_record_probe_find.argtypes = [ip, C.c_int, C.c_int]
    lib.bwd_record_probe_frame.argtypes = [dp, dp, C.c_double, ip, C.c_int, ip, C.c_int, C.c_int, dp, ip, dp]
    return lib


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int))


def _record(probe, scores, probs, entropy, experts, sel, ref_hyps, info, slots_ok=True):
    scores, probs = np.ascontiguousarray(scores, np.float64), np.ascontiguousarray(probs, np.float64)
    experts, sel = np.ascontiguousarray(experts, np.int32), np.ascontiguousarray(sel, np.int32)
    ref_hyps, info = np.ascontiguousarray(ref_hyps, np.float64), np.ascontiguousarray(info, np.int32).reshape(-1, 4)
    rec = np.full(32, -7.0)
    win = probe.bwd_record_probe_frame(_dp(scores), _dp(probs), float(entropy), _ip(experts), len(scores), _ip(sel), len(sel),
                                       int(slots_ok), _dp(ref_hyps), _ip(info), _dp(rec))
    assert not (rec == -7.0).any()  # all 32 doubles are written, slot or no slot
    return win, rec


@pytest.fixture(scope="module")
def stages(oracle):
    """Per case: the oracle's training stages and its forward call at the same key, computed once."""
    out = []
    for k, N, call in CASES:
        f = S.make_frame(k)
        ha = S.gating_assignment(f, N)
        kw = dict(focal=f["focal"], ppx=f["ppx"], ppy=f["ppy"], sub_sampling=f["sub"], seed=SEED, call=call)
        bwd = oracle.backward(f["coords"], np.zeros_like(f["coords"]), ha, f["gt_pose"].astype(np.float32), want_stages=True, **kw)
        fwd = oracle.forward(f["coords"], ha, **kw)
        out.append((ha, bwd, fwd))
    return out


def _slot_tables(bwd):
    """What k_bwd_select and the slot refinement leave: the ordered list of hypotheses with p >= 1e-3 and a map_info row per slot
    (accepted buffer -- unused by the record --, inliers of the last accepted step, accepted steps, LM iterations)."""
    sel = np.flatnonzero(~(bwd["probs"] < 1e-3)).astype(np.int32)
    info = np.stack([np.where(bwd["have_map"][sel], 0, -1), bwd["ref_inliers"][sel], bwd["ref_steps"][sel], bwd["ref_lm_iters"][sel]], 1)
    return sel, info.astype(np.int32)


@pytest.mark.parametrize("i", range(len(CASES)))
def test_record_of_the_training_stages_is_the_forward_call(probe, stages, i):
    ha, bwd, fwd = stages[i]
    N = len(ha)
    sel, info = _slot_tables(bwd)
    win, rec = _record(probe, bwd["scores"], bwd["probs"], bwd["entropy"], ha, sel, bwd["ref_hyps"], info)
    print("case %r: winner %d, %d slots, %d accepted steps" % (CASES[i], win, len(sel), fwd["ref_steps"]))
    assert 1 <= len(sel) <= N and win in sel  # p(argmax) >= 1/N >= 1e-3
    # discrete fields: equal
    assert win == fwd["winner"] == int(rec[api.RES_HYP])
    assert int(rec[api.RES_EXPERT]) == fwd["expert"] == int(ha[win])
    assert int(rec[api.RES_REF_STEPS]) == fwd["ref_steps"]
    assert int(rec[api.RES_LM_ITERS]) == fwd["lm_iters"]
    last = int(fwd["inlier_counts"][fwd["ref_steps"] - 1]) if fwd["ref_steps"] > 0 else 0  # the last ACCEPTED step's inlier set
    assert int(rec[api.RES_INLIERS]) == last
    assert rec[api.RES_CONTENDERS] == float(N) and rec[api.RES_VALID] == 1.0
    # one arithmetic: bit-equal
    assert rec[api.RES_RVEC:api.RES_RVEC + 6].tobytes() == fwd["refined"].tobytes()
    assert rec[api.RES_SCORE].tobytes() == fwd["scores"][win].tobytes()
    assert rec[api.RES_PROB].tobytes() == fwd["probs"][win].tobytes()
    assert rec[api.RES_ENTROPY].tobytes() == np.float64(fwd["entropy"]).tobytes()
    assert bwd["scores"].tobytes() == fwd["scores"].tobytes() and bwd["probs"].tobytes() == fwd["probs"].tobytes()
    # the 4x4: floats, each within one float32 ulp of its magnitude
    pose = rec[api.RES_POSE:api.RES_POSE + 16]
    want = fwd["pose"].reshape(16).astype(np.float64)
    assert (pose == pose.astype(np.float32).astype(np.float64)).all()
    ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
    worst = float(np.max(np.abs(pose - want) / ulp))
    print("pose: worst difference %.2f float32 ulp" % worst)
    assert (np.abs(pose - want) <= ulp).all(), (pose, want)


def test_winner_is_draws_argmax(probe):
    """Highest score, first index on ties, a NaN never wins, hypothesis 0 when nothing can win."""
    for scores, want in (([1.0, 3.0, 3.0, 2.0], 1), ([np.nan, 1.0, np.nan, 1.0], 1), ([np.nan, np.nan], 0), ([-np.inf, -np.inf], 0),
                         ([5.0], 0), ([0.0, -0.0, 0.0], 0), ([np.nan, -1e300, np.inf], 2)):
        a = np.asarray(scores, np.float64)
        assert probe.bwd_record_probe_winner(_dp(a), len(a)) == want, scores


def test_slot_search(probe):
    """Every member and non-member of ascending lists of length 0 .. 70 and of a full 1000-slot list."""
    rng = np.random.default_rng(11)
    for n in list(range(0, 71)) + [1000]:
        sel = np.sort(rng.choice(4 * n + 3, size=n, replace=False)).astype(np.int32)
        where = {int(h): s for s, h in enumerate(sel)}
        for win in range(-1, 4 * n + 4):
            assert probe.bwd_record_probe_find(_ip(sel), n, win) == where.get(win, -1), (n, win)


@pytest.mark.parametrize("name,sel,slot", [("empty", [], None), ("only", [3], 0), ("first", [3, 5, 6], 0), ("last", [0, 1, 3], 2),
                                           ("absent", [0, 2, 4, 6], None), ("one, absent", [2], None)])
def test_slot_and_no_slot_records(probe, name, sel, slot):
    """The winner (hypothesis 3 of 7, expert 12) first / last / alone in the slot list: the slot's pose and trace, VALID 1.  Absent,
    or an empty list, or slot tables that are not to be trusted: NaN pose, zero steps, VALID 0 -- the discrete fields are kept."""
    rng = np.random.default_rng(3)
    scores = np.array([0.1, 0.7, 0.2, 0.9, 0.9, np.nan, 0.3])
    probs = np.array([0.05, 0.1, 0.05, 0.4, 0.3, 0.0, 0.1])
    experts = np.array([10, 11, 10, 12, 13, 10, 11], np.int32)
    ref = rng.normal(size=(7, 6))
    info = np.arange(4 * max(len(sel), 1), dtype=np.int32).reshape(-1, 4) + 20
    for ok in (True, False):
        win, rec = _record(probe, scores, probs, 1.75, experts, np.asarray(sel, np.int32), ref, info, slots_ok=ok)
        assert win == 3 and rec[api.RES_HYP] == 3.0 and rec[api.RES_EXPERT] == 12.0 and rec[api.RES_SCORE] == 0.9
        assert rec[api.RES_PROB] == 0.4 and rec[api.RES_ENTROPY] == 1.75 and rec[api.RES_CONTENDERS] == 7.0
        if slot is not None and ok:
            assert rec[api.RES_VALID] == 1.0
            assert rec[api.RES_RVEC:api.RES_RVEC + 6].tobytes() == ref[3].tobytes()
            assert (rec[api.RES_INLIERS], rec[api.RES_REF_STEPS], rec[api.RES_LM_ITERS]) == tuple(float(v) for v in info[slot][1:4])
            T = rec[api.RES_POSE:api.RES_POSE + 16].reshape(4, 4)
            assert np.isfinite(T).all() and T[3].tolist() == [0.0, 0.0, 0.0, 1.0]
            np.testing.assert_allclose(T[:3, :3] @ T[:3, :3].T, np.eye(3), atol=1e-6)
        else:
            assert rec[api.RES_VALID] == 0.0
            assert np.isnan(rec[api.RES_RVEC:api.RES_POSE + 16]).all()
            assert rec[api.RES_REF_STEPS] == 0.0 and rec[api.RES_INLIERS] == 0.0 and rec[api.RES_LM_ITERS] == 0.0


def test_no_slot_record_reads_as_no_record_to_the_evaluation(probe):
    """VALID 0 is what eval_math.hpp's eval_frame reports as status 1 with NaN figures; EXPERT and HYP are carried through."""
    from tests.native import build_eval
    ev = C.CDLL(build_eval.build())
    ev.eval_probe_frame.argtypes = [C.POINTER(C.c_double), C.POINTER(C.c_float), C.c_int, C.c_longlong, C.c_double, C.c_double,
                                    C.POINTER(C.c_double)]
    _, rec = _record(probe, [0.5, 0.2], [0.9, 0.1], 0.4, np.array([4, 5], np.int32), np.zeros(0, np.int32), np.zeros((2, 6)),
                     np.zeros((1, 4), np.int32))
    gt = np.eye(4, dtype=np.float32).reshape(16)
    row = np.full(16, -7.0)
    ev.eval_probe_frame(_dp(rec), gt.ctypes.data_as(C.POINTER(C.c_float)), 1, 4, 5.0, 5.0, _dp(row))
    assert row[api.EVAL_STATUS] == 1.0 and np.isnan(row[api.EVAL_ROT_DEG]) and row[api.EVAL_POSE_OK] == 0.0
    assert row[api.EVAL_EXPERT] == 4.0 and row[api.EVAL_HYP] == 0.0


def test_stand_alone_program_walks_its_cases():
    """The probe's own main() (the form a sanitizer build runs: tests/native/build_bwd_record.py, build_program(sanitize=True))."""
    from tests.native import build_bwd_record
    out = subprocess.run([build_bwd_record.build_program()], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "2630 cases, 0 bad" in out.stdout, out.stdout + out.stderr
