"""eval_math.hpp -- the arithmetic of esac_hip_eval_batch -- compiled for the host (tests/native/eval_probe.cpp) and held against
the harness's own functions (pose_errors_deg_cm, pose_file_values / pose_file_line) on the table the probe builds:

    identical poses (exactly 0.0 and 0.0); rotations of 1e-9, 1e-7, 1e-3 rad; pi - 1e-9, pi - 1e-13 and exactly pi about x, y, z,
    (1,1,0)/sqrt2 and (1,-1,1)/sqrt3 (the diagonal branch and its two sign rules), each against a ground truth with the identity
    rotation and against a general one; 1000 seeded random pose pairs rounded to float32 first; a NaN pose and a pose with one NaN
    in its rotation; thresholds exactly met (strict <).

Both sides are fp64 with the same formulas; what differs is libm's last bits, numpy's matrix product and LAPACK's inverse against
Gauss-Jordan.  Those last bits are AMPLIFIED where the axis of a rotation is ill-conditioned: at pi - 1e-9 the axis is the
difference of matrix entries that agree to 1e-9, divided by 1e-9, so 1e-16 of rounding becomes 1e-7 in a quaternion component.

MEASURED on the CPU over this table (worst absolute difference of any of the nine figures of a row: two errors, four quaternion
components, three translations): 3.701e-08, in a quaternion component of an entry at pi - 1e-9; over the 1000 random pairs alone:
8.5e-14.  BAR = 8 x the worst = 2.961e-07 (the device's libm differs from the host's by a few ulp more); it is the bar of the GPU
tests too (tests/test_gpu_eval_batch.py).  Flags are EQUAL, not close; so is the sign of every quaternion component that is larger
than the bar (a smaller one is a zero with rounding on it, its sign is not information).
"""
import ctypes as C
import math
import subprocess

import numpy as np
import pytest

from esac_amd import api, harness

MEASURED_WORST = 3.701e-08
BAR = 8 * MEASURED_WORST
KIND_IDENTICAL, KIND_SMALL, KIND_NEAR_PI, KIND_RANDOM, KIND_NAN, KIND_NAN_ROT = range(6)
FIGURES = [api.EVAL_ROT_DEG, api.EVAL_TRANS_CM] + list(range(api.EVAL_QUAT, api.EVAL_QUAT + 7))


@pytest.fixture(scope="module")
def probe():
    from tests.native import build_eval
    lib = C.CDLL(build_eval.build())
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    lib.eval_probe_table.argtypes = [dp, dp, ip, C.c_int]
    lib.eval_probe_table.restype = C.c_int
    lib.eval_probe_row.argtypes = [dp, dp, C.c_double, C.c_double, C.c_int, C.c_longlong, C.c_double, C.c_double, dp]
    lib.eval_probe_frame.argtypes = [dp, C.POINTER(C.c_float), C.c_int, C.c_longlong, C.c_double, C.c_double, dp]
    lib.eval_probe_inv4.argtypes = [dp, dp, dp, ip]
    return lib


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


@pytest.fixture(scope="module")
def table(probe):
    n = probe.eval_probe_table(None, None, None, 0)
    P, G, kind = np.zeros((n, 16)), np.zeros((n, 16)), np.zeros(n, np.int32)
    assert probe.eval_probe_table(_dp(P), _dp(G), kind.ctypes.data_as(C.POINTER(C.c_int)), n) == n
    assert np.bincount(kind).tolist() == [4, 6, 30, 1000, 1, 1]
    return P.reshape(n, 4, 4), G.reshape(n, 4, 4), kind


def _row(probe, P, G, expert=1.0, hyp=7.0, gt_expert=1, rot=5.0, trans=5.0):
    row = np.full(16, -7.0)
    P, G = np.ascontiguousarray(P, np.float64), np.ascontiguousarray(G, np.float64)
    probe.eval_probe_row(_dp(P), _dp(G), expert, hyp, 0 if gt_expert is None else 1, 0 if gt_expert is None else gt_expert, rot, trans, _dp(row))
    return row


def test_rows_equal_the_harness_functions_within_the_measured_bar(probe, table):
    P, G, kind = table
    worst, worst_random, where = 0.0, 0.0, None
    for i in range(len(kind)):
        ge = i % 3
        got = _row(probe, P[i], G[i], expert=1.0, hyp=float(i), gt_expert=ge)
        want = harness.eval_row_host(P[i], G[i], 1, i, ge)
        if kind[i] in (KIND_NAN, KIND_NAN_ROT):
            # NaN figures, POSE_OK 0, status 0; the host's translation error of the NaN-in-rotation pose is finite, and so is the row's
            assert math.isnan(got[api.EVAL_ROT_DEG]) and math.isnan(want[api.EVAL_ROT_DEG]), i
            assert math.isnan(got[api.EVAL_TRANS_CM]) == math.isnan(want[api.EVAL_TRANS_CM]), i
            if not math.isnan(want[api.EVAL_TRANS_CM]):
                assert abs(got[api.EVAL_TRANS_CM] - want[api.EVAL_TRANS_CM]) <= BAR
            assert np.isnan(got[api.EVAL_QUAT:api.EVAL_QUAT + 7]).all(), i
            if kind[i] == KIND_NAN:
                assert np.isnan(want[api.EVAL_QUAT:api.EVAL_QUAT + 7]).all()
            assert got[api.EVAL_POSE_OK] == 0.0 == want[api.EVAL_POSE_OK] and got[api.EVAL_STATUS] == 0.0
        else:
            diff = np.abs(got[FIGURES] - want[FIGURES])
            assert np.isfinite(diff).all(), i
            if diff.max() > worst:
                worst, where = float(diff.max()), (i, int(kind[i]), FIGURES[int(diff.argmax())])
            if kind[i] == KIND_RANDOM:
                worst_random = max(worst_random, float(diff.max()))
            assert diff.max() <= BAR, (i, int(kind[i]), got[FIGURES], want[FIGURES])
            q_got, q_want = got[api.EVAL_QUAT:api.EVAL_QUAT + 4], want[api.EVAL_QUAT:api.EVAL_QUAT + 4]
            big = (np.abs(q_got) > BAR) | (np.abs(q_want) > BAR)
            assert np.array_equal(np.sign(q_got[big]), np.sign(q_want[big])), (i, q_got, q_want)
            assert got[api.EVAL_POSE_OK] == want[api.EVAL_POSE_OK], (i, got, want)
            if kind[i] == KIND_IDENTICAL:
                assert got[api.EVAL_ROT_DEG] == 0.0 and got[api.EVAL_TRANS_CM] == 0.0 and got[api.EVAL_POSE_OK] == 1.0
        for col in (api.EVAL_CLASS_OK, api.EVAL_EXPERT, api.EVAL_HYP):
            assert got[col] == want[col], (i, col)
        assert got[api.EVAL_CLASS_OK] == float(ge == 1) and got[api.EVAL_STATUS] == 0.0 and got[14] == 0.0 and got[15] == 0.0
    print("worst absolute difference %.3e at (entry, kind, column) %r; random pairs alone %.3e; bar %.3e" % (worst, where, worst_random, BAR))


def test_helper_is_the_pose_file_line(table):
    """pose_file_values are the numbers pose_file_line prints (the rows are held against the former, the loop writes the latter)."""
    P, _, kind = table
    for i in np.flatnonzero(kind == KIND_RANDOM)[:50]:
        assert harness.pose_file_line("f%d" % i, P[i]) == harness.POSE_LINE_FORMAT % (("f%d" % i,) + tuple(harness.pose_file_values(P[i])))
        parts = harness.pose_file_line("f%d" % i, P[i]).split()
        assert len(parts) == 8 and parts[0] == "f%d" % i


def test_near_pi_entries_take_the_branches_they_are_there_for(table):
    """pi - 1e-13 and pi against the identity ground truth sit in the diagonal branch (s < 1e-12) with c < 0, pi - 1e-9 in the general
    one; among the axes both sign rules fire ((1,-1,1)/sqrt3: R01 < 0; an axis with R02 < 0 appears once the pose is inverted)."""
    P, G, kind = table
    near = np.flatnonzero(kind == KIND_NEAR_PI)
    diag, general, flipped_y = 0, 0, 0
    for i in near:
        M = P[i][:3, :3] @ G[i][:3, :3].T
        sk = 0.5 * np.array([M[2, 1] - M[1, 2], M[0, 2] - M[2, 0], M[1, 0] - M[0, 1]])
        if np.linalg.norm(sk) < 1e-12:
            diag += 1
            flipped_y += int(M[0, 1] < 0)
            assert (np.trace(M) - 1) / 2 < 0
        else:
            general += 1
    assert diag >= 10 and general >= 10 and flipped_y >= 2, (diag, general, flipped_y)


def test_thresholds_are_strict(probe):
    """Translation error exactly 6.25 cm (0.0625 m along x: every step exact), rotation error exactly 0."""
    G = np.eye(4)
    P = np.eye(4)
    P[0, 3] = 0.0625
    assert harness.pose_errors_deg_cm(P, G) == (0.0, 6.25)
    met = _row(probe, P, G, rot=5.0, trans=6.25)
    assert met[api.EVAL_TRANS_CM] == 6.25 and met[api.EVAL_ROT_DEG] == 0.0 and met[api.EVAL_POSE_OK] == 0.0
    above = _row(probe, P, G, rot=5.0, trans=float(np.nextafter(np.float32(6.25), np.float32(7))))
    assert above[api.EVAL_POSE_OK] == 1.0
    assert _row(probe, P, G, rot=0.0, trans=10.0)[api.EVAL_POSE_OK] == 0.0  # 0 < 0 is false
    assert _row(probe, P, G, rot=float(np.float32(1e-30)), trans=10.0)[api.EVAL_POSE_OK] == 1.0
    for rot, trans in ((5.0, 6.25), (0.0, 10.0), (5.0, 7.0)):
        assert _row(probe, P, G, rot=rot, trans=trans)[api.EVAL_POSE_OK] == harness.eval_row_host(P, G, 1, 7, 1, rot, trans)[api.EVAL_POSE_OK]


def test_frame_reads_floats_and_reports_the_status(probe, table):
    """eval_frame: the pose is read as floats (what esac.forward puts into outPose), the ground truth is float; VALID 1 / 3 / 0 ->
    STATUS 0 / 3 / 1 with NaN figures, zero flags, CLASS_OK -1 without ground-truth experts, EXPERT and HYP copied."""
    P, G, kind = table
    i = int(np.flatnonzero(kind == KIND_SMALL)[5])  # 1e-3 rad on a general double-precision pose: the float rounding is visible
    rec = np.zeros(32)
    rec[api.RES_POSE:api.RES_POSE + 16] = P[i].reshape(16)
    rec[api.RES_HYP], rec[api.RES_EXPERT], rec[api.RES_VALID] = 41.0, 2.0, 1.0
    gt = np.ascontiguousarray(G[i].reshape(16), np.float32)

    def frame(has, ge):
        row = np.full(16, -7.0)
        probe.eval_probe_frame(_dp(rec), gt.ctypes.data_as(C.POINTER(C.c_float)), has, ge, 5.0, 5.0, _dp(row))
        return row

    got = frame(1, 2)
    want = harness.eval_row_host(P[i].astype(np.float32), gt.reshape(4, 4), 2, 41, 2)
    assert np.abs(got[FIGURES] - want[FIGURES]).max() <= BAR
    as_double = harness.eval_row_host(P[i], G[i], 2, 41, 2)
    assert abs(as_double[api.EVAL_ROT_DEG] - want[api.EVAL_ROT_DEG]) > 1e-7  # (the case tells floats from doubles)
    assert got[api.EVAL_CLASS_OK] == 1.0 and got[api.EVAL_EXPERT] == 2.0 and got[api.EVAL_HYP] == 41.0 and got[api.EVAL_STATUS] == 0.0
    assert frame(0, 0)[api.EVAL_CLASS_OK] == -1.0 and frame(1, 1)[api.EVAL_CLASS_OK] == 0.0
    for valid, status in ((3.0, 3.0), (0.0, 1.0), (2.0, 1.0)):
        rec[api.RES_VALID] = valid
        for has, class_ok in ((1, 0.0), (0, -1.0)):
            row = frame(has, 2)
            assert row[api.EVAL_STATUS] == status and np.isnan(row[FIGURES]).all()
            assert row[api.EVAL_POSE_OK] == 0.0 and row[api.EVAL_CLASS_OK] == class_ok
            assert row[api.EVAL_EXPERT] == 2.0 and row[api.EVAL_HYP] == 41.0 and row[14] == 0.0 and row[15] == 0.0


def test_register_only_inverse_is_gt_math_inv4_bit_for_bit(probe, table):
    """eval_inv4 (selects instead of a run-time row index: no scratch memory in the kernel) against inv4 of gt_math.hpp, and
    against numpy's inverse to rounding; a singular matrix is refused by both."""
    P, _, kind = table
    for i in np.flatnonzero(kind <= KIND_RANDOM):
        a, b, ok = np.zeros(16), np.zeros(16), np.zeros(2, np.int32)
        A = np.ascontiguousarray(P[i].reshape(16))
        probe.eval_probe_inv4(_dp(A), _dp(a), _dp(b), ok.ctypes.data_as(C.POINTER(C.c_int)))
        assert ok.tolist() == [1, 1] and a.tobytes() == b.tobytes(), i
        np.testing.assert_allclose(a.reshape(4, 4), np.linalg.inv(P[i]), atol=1e-12)
    rng = np.random.default_rng(3)
    for _ in range(200):  # general matrices: every pivot row gets its turn
        A = np.ascontiguousarray(rng.normal(size=16))
        a, b, ok = np.zeros(16), np.zeros(16), np.zeros(2, np.int32)
        probe.eval_probe_inv4(_dp(A), _dp(a), _dp(b), ok.ctypes.data_as(C.POINTER(C.c_int)))
        assert ok.tolist() == [1, 1] and a.tobytes() == b.tobytes()
    A = np.zeros(16)
    a, b, ok = np.zeros(16), np.zeros(16), np.zeros(2, np.int32)
    probe.eval_probe_inv4(_dp(A), _dp(a), _dp(b), ok.ctypes.data_as(C.POINTER(C.c_int)))
    assert ok.tolist() == [0, 0]


def test_stand_alone_program_walks_the_table():
    """The probe's own main() (the form a sanitizer build runs: tests/native/build_eval.py, build_program(sanitize=True))."""
    from tests.native import build_eval
    out = subprocess.run([build_eval.build_program()], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "1042 entries, 0 bad" in out.stdout, out.stdout + out.stderr
