"""The arithmetic of esac_hip_verify_batch on the CPU: tests/native/verify_probe.cpp compiles esac_amd/csrc/verify_math.hpp for the
host and runs the frozen cases of tests/verify_reference.py.  Score against the oracle (in_hyps), inlier counts against the numpy
reference exactly, SSE / A / C against the 50-digit sums with the bars derived there.  The same program, built with
-fsanitize=address,undefined, walks the same cases once."""
import numpy as np
import pytest

from oracle import esac_oracle as oracle
from tests import verify_reference as V
from tests.native import build_verify


def _requests(fmt=0):
    """one probe request per (case, frame): the frame's expert map with all K poses of the row"""
    reqs, index = [], []
    for case in V.CASES:
        for b, row in enumerate(V.case_rows(case)):
            fr = row[0][0]
            poses = np.stack([r[2] for r in row])
            if fmt == 1:
                poses = np.stack([V.camera_pose_from_rt(p) for p in poses]).astype(np.float32)
            reqs.append((fr["coords"][row[0][3]], fr["cam"], V.SCORE, case["strict"], fmt, poses))
            index.append((case, b, row))
    return reqs, index


@pytest.fixture(scope="module")
def probe_rows():
    reqs, index = _requests()
    rows, oks = build_verify.run_probe(build_verify.build_probe(), reqs)
    return index, rows, oks


@pytest.fixture(scope="module")
def gold():
    return V.golden()


def _oracle_scores(fr, row, strict):
    """the oracle's exact scores of the row's poses (its NaN rule is the strict one: the default rule sees the map whose NaN cell
    is a point that clamps to maxReproj)"""
    coords = fr["coords"] if strict else fr["oracle_coords"]
    cam = fr["cam"]
    return oracle.forward(coords, np.array([r[3] for r in row], np.int64), cam["shift"][0], cam["shift"][1], cam["focal"], cam["ppx"], cam["ppy"],
                          V.SCORE["tau"], V.SCORE["alpha"], V.SCORE["beta"], V.SCORE["max_reproj"], V.SCORE["sub"],
                          in_hyps=np.stack([r[2] for r in row]))


def test_preconditions_hold_on_the_reference():
    """no cell within 1e-3 px of tau; every pose but the far one has n >= 12 and cond_2(A) <= 1e10; the far one n < 4; the all-inlier
    map is one; the NaN map's stand-in cell clamps like the NaN does"""
    kinds_seen, frames_seen = set(), set()
    for case in V.CASES:
        for row in V.case_rows(case):
            for fr, kind, pose, expert in row:
                ref = V.reference(fr, kind, case["strict"])
                assert np.nanmin(np.abs(ref["err"] - V.SCORE["tau"])) > V.BAND_PX, (case["name"], fr["name"], kind)
                if kind == "far":
                    assert ref["n"] < 4, (fr["name"], ref["n"])
                else:
                    assert ref["n"] >= V.MIN_INLIERS and ref["cond"] <= V.MAX_COND, (fr["name"], kind, ref["n"], ref["cond"])
                kinds_seen.add(kind)
                frames_seen.add(fr["name"])
    assert kinds_seen == set(V.POSE_KINDS) and frames_seen == {s["name"] for s in V.FRAME_SPECS}
    allin = V.frame("allin")
    assert V.reference(allin, "true")["n"] == allin["h"] * allin["w"]
    nan = V.frame("nan")
    r, c = next(s for s in V.FRAME_SPECS if s["name"] == "nan")["nan_cell"]
    assert np.isnan(nan["coords"][nan["true_expert"], :, r, c]).all() and np.isfinite(nan["oracle_coords"]).all()
    for kind in V.POSE_KINDS:
        stand_in = V.reference_row(nan["oracle_coords"][nan["true_expert"]], nan["poses"][kind], nan["cam"])
        assert stand_in["err"][r * nan["w"] + c] > V.SCORE["max_reproj"], kind
        assert np.isnan(V.reference(nan, kind, True)["score"]) and np.isfinite(V.reference(nan, kind, False)["score"])
    assert {E for E in (V.frame(s["name"])["true_expert"] for s in V.FRAME_SPECS)} == {0, V.E - 1}


def test_reference_jacobian_against_central_differences():
    """the analytic Jacobian of the numpy reference, pinned once: central differences of the projection, step 1e-6"""
    worst = 0.0
    for name, kind in (("g12x16", "true"), ("g13x17s", "winner"), ("cam2", "second")):
        fr = V.frame(name)
        pts = fr["coords"][fr["true_expert"]].reshape(3, -1).T.astype(np.float64)[::7]
        cam, pose = fr["cam"], fr["poses"][kind]
        _, Ju, Jv = V.project(pose, pts, cam["focal"], cam["ppx"], cam["ppy"])
        for j in range(6):
            d = np.zeros(6)
            d[j] = 1e-6
            up, _, _ = V.project(pose + d, pts, cam["focal"], cam["ppx"], cam["ppy"])
            dn, _, _ = V.project(pose - d, pts, cam["focal"], cam["ppx"], cam["ppy"])
            num = (up - dn) / 2e-6
            scale = np.abs(np.concatenate([Ju, Jv])).max()
            worst = max(worst, np.abs(num[:, 0] - Ju[:, j]).max() / scale, np.abs(num[:, 1] - Jv[:, j]).max() / scale)
    # truncation h^2 f''' / 6 ~ 1e-12 and rounding eps |u| / h ~ 1e-8 px over entries of ~1e2 .. 1e3
    assert worst < 1e-7, worst


def test_golden_sums_are_current_and_give_the_recorded_levels(gold):
    """tests/golden/verify/verify_ref50.npz is what make_verify_ref50 computes today (two frames recomputed at 50 digits), and the levels
    in verify_reference.py are the numpy reference's worst distance from it"""
    for name in ("g12x16", "cam2"):
        fr = V.frame(name)
        for kind in ("true", "second"):
            ref = V.reference(fr, kind)
            A, sse = V.reference_sums_50(fr["coords"][fr["experts"][kind]], fr["poses"][kind], fr["cam"], ref["inl"])
            g = gold[(name, kind)]
            assert [V.split_hi_lo(a) for a in A] == list(zip(g["A_hi"].tolist(), g["A_lo"].tolist())), (name, kind)
            assert V.split_hi_lo(sse) == (g["sse_hi"], g["sse_lo"])
    level_a = level_s = 0.0
    for spec in V.FRAME_SPECS:
        fr = V.frame(spec["name"])
        for kind in V.POSE_KINDS:
            ref = V.reference(fr, kind)
            if ref["n"] > 0:
                level_a = max(level_a, V.a_error(ref["A"][V.IU], gold[(spec["name"], kind)]))
                level_s = max(level_s, V.sse_error(ref["sse"], gold[(spec["name"], kind)]))
    print("reference level: A %.3g, SSE %.3g" % (level_a, level_s))
    assert 0.5 * V.REF_LEVEL_A < level_a <= V.REF_LEVEL_A and 0.5 * V.REF_LEVEL_SSE < level_s <= V.REF_LEVEL_SSE


def test_host_rows_of_every_frozen_case(probe_rows, gold):
    """score against the oracle at 1e-12, n exactly, SSE / A / C within the bars, the status of every row"""
    index, rows, oks = probe_rows
    worst = dict(A=(0.0, ""), sse=(0.0, ""), C=(0.0, ""))
    for (case, b, row), got, ok in zip(index, rows, oks):
        fr = row[0][0]
        scores = _oracle_scores(fr, row, case["strict"])["scores"]
        assert (ok == 1).all()
        for k, (_, kind, pose, expert) in enumerate(row):
            label = "%s[%d,%d] %s/%s" % (case["name"], b, k, fr["name"], kind)
            m = V.check_row(got[k], fr, kind, case["strict"], gold, oracle_score=scores[k], label=label)
            for key in worst:
                if key in m:
                    rel = m[key] / (m["C_bar"] if key == "C" else 1.0)
                    worst[key] = max(worst[key], (rel, label))
    print("host probe, worst: A %.3g (%s), SSE %.3g (%s), C / bar %.3g (%s)" % (worst["A"] + worst["sse"] + worst["C"]))


def test_inlier_count_of_the_winner_is_the_oracles(probe_rows):
    """oracle.forward(in_hyps=...) reports in inlier_counts[0] the cells with err < tau at the pose its refinement starts from --
    the INITIAL pose of the winner among in_hyps (refine_hyp counts before the first re-fit) -- which is this call's n"""
    index, rows, _ = probe_rows
    checked = 0
    for (case, b, row), got in zip(index, rows):
        if case["strict"] or len(row) < 2:
            continue
        fr = row[0][0]
        out = _oracle_scores(fr, row, False)
        w = out["winner"]
        assert out["inlier_counts"][0] == got[w][1], (case["name"], b, w, out["inlier_counts"][:2], got[w][1])
        checked += 1
    assert checked >= 8


def test_4x4_poses_are_fetched_as_gt_from_pose_does(probe_rows):
    """the float 4x4 format: verify_fetch_pose (register-only inverse) against gt_math.hpp's gt_from_pose, bit for bit, singular and
    non-finite poses included; and the rows of the 4x4 format against the reference at the round-tripped pose"""
    import subprocess
    mats = []
    for name in ("g12x16", "cam1", "g24x32e2"):
        for kind in V.POSE_KINDS:
            mats.append(V.camera_pose_from_rt(V.frame(name)["poses"][kind]).astype(np.float32))
    sing = mats[0].copy()
    sing[2] = sing[1]
    nan = mats[1].copy()
    nan[0, 3] = np.nan
    inf = mats[2].copy()
    inf[1, 1] = np.inf
    text = "".join("fetch %s\n" % build_verify.hexf(m.reshape(-1).tolist()) for m in mats + [sing, nan, inf])
    out = subprocess.run([build_verify.build_probe()], input=text, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l.split() for l in out.stdout.splitlines()]
    assert len(lines) == len(mats) + 3
    for i, l in enumerate(lines):
        assert l[0] == "fetch"
        if i < len(mats):
            assert l[1] == "1" and l[8] == "1" and l[2:8] == l[9:15], l
            got = np.array([float.fromhex(v) for v in l[2:8]])
            np.testing.assert_allclose(got, V.rt_from_camera_pose(mats[i]), rtol=0, atol=1e-12)
        else:
            assert l[1] == "0", l  # singular (gt_from_pose's verdict too), NaN, inf
    assert lines[len(mats)][8] == "0"


def test_sanitized_probe_walks_the_frozen_cases(probe_rows):
    """the same program under AddressSanitizer and UBSan (its own process), both pose formats: same rows, nothing reported"""
    index, rows, _ = probe_rows
    exe = build_verify.build_probe(sanitize=True)
    reqs, _ = _requests()
    san_rows, _ = build_verify.run_probe(exe, reqs)
    for a, b in zip(rows, san_rows):
        # (-O1 against -O2 of one contraction-free text: the same operations)
        assert np.array_equal(a, b, equal_nan=True)
    reqs4, _ = _requests(fmt=1)
    rows4, oks4 = build_verify.run_probe(exe, reqs4)
    assert all((ok == 1).all() for ok in oks4)
    for (case, bb, row), a, b in zip(index, rows, rows4):
        for k, (fr, kind, pose, expert) in enumerate(row):
            if not case["strict"]:
                V.check_formats(a[k], b[k], fr, kind, "%s[%d,%d] %s/%s" % (case["name"], bb, k, fr["name"], kind))


def test_collinear_inliers_take_the_pseudo_inverse():
    """status 2: sixteen inliers on the scene's x axis under rvec = 0 -- the first row and column of A are exactly zero, inv_spd6
    refuses, C is sigma^2 times the pseudo-inverse (the oracle's pinv_sym6, the bar check_solves holds the Jacobi route to)"""
    coords, pose, cam = V.collinear_case()
    rows, oks = build_verify.run_probe(build_verify.build_probe(), [(coords[1], cam, V.SCORE, False, 0, pose.reshape(1, 6))])
    row = rows[0][0]
    assert oks[0][0] == 1 and row[4] == 2 and row[1] == 16, row[:5]
    A = V.sym(row[6:27])
    assert (A[0] == 0).all() and np.linalg.matrix_rank(A[1:, 1:]) == 5
    Cm = row[28:64].reshape(6, 6)
    assert (Cm[0] == 0).all() and (Cm[:, 0] == 0).all() and (Cm == Cm.T).all()
    want = row[3] * oracle.pinv_sym6(A)
    np.testing.assert_allclose(Cm, want, rtol=1e-9, atol=1e-12 * np.abs(want).max())
