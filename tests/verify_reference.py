"""Reference and frozen cases of the pose verification call (esac_hip_verify_batch), shared by tests/test_verify_host.py (the
host build of verify_math.hpp) and tests/test_gpu_verify.py (the kernel).  Not a test module.

The reference is numpy fp64, written from the definitions and not from the device code:
  R(rvec) = I + sin(th) K + (1 - cos(th)) K^2, Xc = R X + t, (u, v) = (f Xc_x / Xc_z + cx, f Xc_y / Xc_z + cy);
  err = |(u, v) - pixel|; score = alpha / (W H) * sum of 1 - 1 / (1 + exp(-beta (min(err, maxReproj) - tau)));
  inliers: min(err, maxReproj) < tau (a NaN error is none); over them SSE = sum of |(u, v) - pixel|^2 and
  A = sum of Ju^T Ju + Jv^T Jv with the analytic Jacobian of (u, v) with respect to (rvec, tvec) -- dR/dr_i from the closed form
  of Gallego & Yezzi (2015), (r_i [r]x + [r x (I - R) e_i]x) R / th^2 --; sigma^2 = SSE / (2n - 6); C = sigma^2 A^-1.
The same formulas run at 50 digits (mpmath, the route of tests/device_math_checks.py) give the reference's own rounding level,
from which the bars below follow.  tests/golden/verify/verify_ref50.npz holds those 50-digit sums as double-double pairs (hi + lo);
tests/golden/make_verify_ref50.py regenerates it and prints the levels.
"""
import math
import os

import numpy as np

from esac_amd import synthetic

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "verify", "verify_ref50.npz")
IU = np.triu_indices(6)

# ---------------------------------------------------------------- bars (measured: tests/golden/make_verify_ref50.py)
# The reference's own rounding level over every pose of every frozen frame: the largest |A_fp64 - A_50| / sqrt(A_ii A_jj), and
# |SSE_fp64 - SSE_50| / SSE_50.  The bar is 8x the level: another summation order, contraction-free operations.
REF_LEVEL_A = 2.3e-15       # measured 2.28e-15 (frame "cam2", pose "second"), rounded up
REF_LEVEL_SSE = 2.2e-14     # measured 2.18e-14 (frame "allin", pose "second": residuals of ~0.5 px formed from pixels of ~100), rounded up
BAR_A = 8 * REF_LEVEL_A
BAR_SSE = 8 * REF_LEVEL_SSE
BAR_SCORE = 1e-12           # the project's bar for exact scores under another summation order
BAR_INV_SPD6 = 1e-8         # what tests/test_gpu_device_math.py (device_math_checks.check_solves) holds inv_spd6 to
BAND_PX = 1e-3              # LAB_NOTES: reference-float against fp64 decisions of err < tau
MIN_INLIERS, MAX_COND = 12, 1e10

SCORE = dict(tau=10.0, alpha=100.0, beta=0.5, max_reproj=100.0, sub=8)
E = 3
POSE_KINDS = ("true", "perturbed", "winner", "second", "far")


# ---------------------------------------------------------------- pose helpers (numpy fp64)
def skew(v):
    return np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]], np.float64)


def rot_from_rvec(r):
    r = np.asarray(r, np.float64)
    th = float(np.linalg.norm(r))
    if th < 1e-300:
        return np.eye(3)
    K = skew(r / th)
    return np.eye(3) + math.sin(th) * K + (1 - math.cos(th)) * (K @ K)


def rvec_from_rot(R):
    """log map of a rotation matrix (angle well inside (0, pi) for every pose of the cases)"""
    w = 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    s, c = float(np.linalg.norm(w)), 0.5 * (np.trace(R) - 1.0)
    th = math.atan2(s, c)
    return w * (th / s) if s > 1e-300 else np.zeros(3)


def rt_from_camera_pose(T):
    """camera pose (camera -> scene 4x4) -> rvec | tvec (scene -> camera): general inverse, nearest rotation, log"""
    Ti = np.linalg.inv(np.asarray(T, np.float64))
    U, _, Vt = np.linalg.svd(Ti[:3, :3])
    return np.concatenate([rvec_from_rot(U @ Vt), Ti[:3, 3]])


def camera_pose_from_rt(pose):
    T = np.eye(4)
    T[:3, :3] = rot_from_rvec(pose[:3])
    T[:3, 3] = pose[3:]
    return np.linalg.inv(T)


def drot(r):
    """dR/dr_i, i = 0..2 (Gallego & Yezzi 2015, eq. 9)"""
    r = np.asarray(r, np.float64)
    R, th2 = rot_from_rvec(r), float(r @ r)
    return [(r[i] * skew(r) + skew(np.cross(r, (np.eye(3) - R)[:, i]))) @ R / th2 for i in range(3)]


def pixels(h, w, sub, shift):
    """createSampling (esac_util.h:64-66): the pixel of cell (row, col), as float32 values"""
    px = (np.arange(w) * sub + sub // 2 - shift[0]).astype(np.float32).astype(np.float64)
    py = (np.arange(h) * sub + sub // 2 - shift[1]).astype(np.float32).astype(np.float64)
    return np.broadcast_to(px[None, :], (h, w)).reshape(-1), np.broadcast_to(py[:, None], (h, w)).reshape(-1)


def project(pose, pts, focal, ppx, ppy):
    """(u, v) [P,2] and the Jacobian rows Ju, Jv [P,6] of the points pts [P,3] under pose"""
    R, t = rot_from_rvec(pose[:3]), np.asarray(pose[3:], np.float64)
    Xc = pts @ R.T + t
    iz = 1.0 / Xc[:, 2]
    u, v = focal * Xc[:, 0] * iz + ppx, focal * Xc[:, 1] * iz + ppy
    dX = [pts @ dR.T for dR in drot(pose[:3])] + [np.broadcast_to(e, Xc.shape) for e in np.eye(3)]  # dXc / d param, 6 x [P,3]
    Ju = np.stack([focal * (d[:, 0] * iz - Xc[:, 0] * d[:, 2] * iz * iz) for d in dX], axis=1)
    Jv = np.stack([focal * (d[:, 1] * iz - Xc[:, 1] * d[:, 2] * iz * iz) for d in dX], axis=1)
    return np.stack([u, v], axis=1), Ju, Jv


def reference_row(coords_e, pose, cam, strict=False, score=SCORE):
    """One pose against one expert's map coords_e [3,h,w] (float32) with cam = dict(focal, ppx, ppy, shift): the figures of a row
    and what the preconditions need.  dict(score, n, sse, sigma2, A [6,6], C [6,6] or None, err [P], inl [P] bool, cond)."""
    _, h, w = coords_e.shape
    pts = coords_e.reshape(3, -1).T.astype(np.float64)
    px, py = pixels(h, w, score["sub"], cam["shift"])
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        uv, Ju, Jv = project(np.asarray(pose, np.float64), pts, float(np.float32(cam["focal"])), float(np.float32(cam["ppx"])), float(np.float32(cam["ppy"])))
        ex, ey = uv[:, 0] - px, uv[:, 1] - py
        err = np.sqrt(ex * ex + ey * ey)
        clamped = np.where(np.isnan(err), np.nan if strict else score["max_reproj"], np.minimum(err, score["max_reproj"]))
        terms = 1.0 - 1.0 / (1.0 + np.exp(-score["beta"] * (clamped - score["tau"])))
        inl = np.minimum(err, score["max_reproj"]) < score["tau"]  # (NaN: False)
    sc = float(terms.sum() * (np.float32(score["alpha"]) / np.float32(w) / np.float32(h)))
    n = int(inl.sum())
    sse = float((ex[inl] ** 2 + ey[inl] ** 2).sum())
    A = Ju[inl].T @ Ju[inl] + Jv[inl].T @ Jv[inl]
    out = dict(score=sc, n=n, sse=sse, A=A, err=err, inl=inl, sigma2=float("nan"), C=None, cond=float("inf"))
    if n >= 4:
        out["sigma2"] = sse / (2 * n - 6)
        out["cond"] = float(np.linalg.cond(A))
        if out["cond"] < 1e15:
            out["C"] = out["sigma2"] * np.linalg.inv(A)
    return out


def reference_sums_50(coords_e, pose, cam, inl, score=SCORE, dps=50):
    """A (21 upper-triangle sums) and SSE over the inlier set `inl` by the same formulas at `dps` digits (mpmath)."""
    import mpmath
    mpmath.mp.dps = dps
    mpf = mpmath.mpf
    _, h, w = coords_e.shape
    pts = coords_e.reshape(3, -1).T.astype(np.float64)
    px, py = pixels(h, w, score["sub"], cam["shift"])
    f, cx, cy = (mpf(float(np.float32(cam[k]))) for k in ("focal", "ppx", "ppy"))
    r = [mpf(float(x)) for x in pose[:3]]
    t = [mpf(float(x)) for x in pose[3:]]
    th2 = r[0] * r[0] + r[1] * r[1] + r[2] * r[2]
    th = mpmath.sqrt(th2)

    def sk(v):
        return mpmath.matrix([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]])

    K = sk([x / th for x in r])
    I3 = mpmath.eye(3)
    R = I3 + mpmath.sin(th) * K + (1 - mpmath.cos(th)) * (K * K)
    IR = I3 - R
    dR = []
    for i in range(3):
        col = [IR[0, i], IR[1, i], IR[2, i]]
        cr = [r[1] * col[2] - r[2] * col[1], r[2] * col[0] - r[0] * col[2], r[0] * col[1] - r[1] * col[0]]
        dR.append((r[i] * sk(r) + sk(cr)) * R / th2)
    A = [mpf(0)] * 21
    sse = mpf(0)
    for i in np.flatnonzero(inl):
        X = [mpf(float(x)) for x in pts[i]]
        Xc = [R[k, 0] * X[0] + R[k, 1] * X[1] + R[k, 2] * X[2] + t[k] for k in range(3)]
        iz = 1 / Xc[2]
        d = [[dR[j][k, 0] * X[0] + dR[j][k, 1] * X[1] + dR[j][k, 2] * X[2] for k in range(3)] for j in range(3)]
        d += [[mpf(1), mpf(0), mpf(0)], [mpf(0), mpf(1), mpf(0)], [mpf(0), mpf(0), mpf(1)]]
        Ju = [f * (dj[0] * iz - Xc[0] * dj[2] * iz * iz) for dj in d]
        Jv = [f * (dj[1] * iz - Xc[1] * dj[2] * iz * iz) for dj in d]
        ex, ey = f * Xc[0] * iz + cx - mpf(float(px[i])), f * Xc[1] * iz + cy - mpf(float(py[i]))
        sse += ex * ex + ey * ey
        k = 0
        for p in range(6):
            for q in range(p, 6):
                A[k] += Ju[p] * Ju[q] + Jv[p] * Jv[q]
                k += 1
    return A, sse


def split_hi_lo(x):
    """an mpmath value as a double-double pair"""
    import mpmath
    hi = float(x)
    return hi, float(x - mpmath.mpf(hi))


# ---------------------------------------------------------------- frozen frames
def _frame(name, k, h, w, true_expert, shift=(0, 0), focal=None, pp=None, noise=0.02, outlier_frac=0.3, nan_cell=None):
    return dict(name=name, k=k, h=h, w=w, true_expert=true_expert, shift=shift, focal=focal, pp=pp, noise=noise,
                outlier_frac=outlier_frac, nan_cell=nan_cell)


# name, synthetic seed k (esac_amd/synthetic.py: default_rng(1000 + k)), grid, true expert.  The seeds are the first from each
# frame's starting value that meet the preconditions (test_verify_host.py asserts them).
FRAME_SPECS = [
    _frame("g12x16", 0, 12, 16, 0),
    _frame("g13x17s", 1, 13, 17, 2, shift=(3, -2)),
    _frame("g24x32", 2, 24, 32, 0),
    _frame("g24x32e2", 3, 24, 32, 2),
    _frame("g16x12", 4, 16, 12, 2),
    _frame("cam1", 5, 12, 16, 2, shift=(-4, 5), focal=90.0, pp=(60.0, 50.0)),
    _frame("cam2", 6, 12, 16, 0, shift=(7, 0), focal=130.0, pp=(66.5, 47.25)),
    _frame("nan", 7, 12, 16, 0, nan_cell=(5, 9)),
    _frame("allin", 8, 12, 16, 2, noise=0.005, outlier_frac=0.0),
]

_FRAMES = {}


def frame(name):
    """The frozen frame `name`: coords [E,3,h,w] float32, cam, true_expert, poses {kind: rvec | tvec}, experts {kind: int}."""
    if name in _FRAMES:
        return _FRAMES[name]
    from oracle import esac_oracle as oracle
    spec = next(s for s in FRAME_SPECS if s["name"] == name)
    h, w, sub = spec["h"], spec["w"], SCORE["sub"]
    focal = spec["focal"] if spec["focal"] is not None else 0.8 * w * sub
    ppx, ppy = spec["pp"] if spec["pp"] is not None else (w * sub / 2.0, h * sub / 2.0)
    te = spec["true_expert"]
    fr = synthetic.make_frame(spec["k"], E=E, true_expert=te, H=h, W=w, sub=sub, focal=focal, ppx=ppx, ppy=ppy, noise=spec["noise"],
                              outlier_frac=spec["outlier_frac"], shift=spec["shift"])
    coords = np.ascontiguousarray(fr["coords"])
    cam = dict(focal=float(focal), ppx=float(ppx), ppy=float(ppy), shift=tuple(int(s) for s in spec["shift"]))
    # the oracle's own sampled hypotheses on the clean map: the two best by score
    sampled = oracle.forward(coords, np.full(16, te, np.int64), cam["shift"][0], cam["shift"][1], cam["focal"], cam["ppx"], cam["ppy"],
                             SCORE["tau"], SCORE["alpha"], SCORE["beta"], SCORE["max_reproj"], sub, seed=1305, call=spec["k"])
    order = np.argsort(-sampled["scores"], kind="stable")
    gt = fr["gt_pose"]
    pert = gt.copy()
    axis = np.array([0.3, -0.5, 0.8]) / np.linalg.norm([0.3, -0.5, 0.8])
    pert[:3, :3] = rot_from_rvec(axis * math.radians(1.0)) @ gt[:3, :3]
    pert[:3, 3] = gt[:3, 3] + np.array([0.012, -0.01, 0.0125])  # |.| = 2 cm
    far = gt.copy()
    far[:3, :3] = rot_from_rvec(np.array([0.0, math.radians(100.0), 0.0])) @ gt[:3, :3]
    far[:3, 3] = gt[:3, 3] + np.array([30.0, -20.0, 25.0])
    poses = dict(true=rt_from_camera_pose(gt), perturbed=rt_from_camera_pose(pert), winner=sampled["hyps"][order[0]].copy(),
                 second=sampled["hyps"][order[1]].copy(), far=rt_from_camera_pose(far))
    clean = coords
    if spec["nan_cell"] is not None:
        coords = coords.copy()
        r, c = spec["nan_cell"]
        coords[te, :, r, c] = np.nan
        # what the default rule makes of that cell, for the oracle (whose NaN rule is the strict one): a point 1e4 m to the side
        # of every pose's camera -- its error clamps to maxReproj like the NaN's
        clean = coords.copy()
        clean[te, :, r, c] = np.float32(1e4)
    out = dict(name=name, coords=coords, oracle_coords=clean, cam=cam, h=h, w=w, true_expert=te, poses=poses,
               experts={k: te for k in POSE_KINDS}, gt_pose=gt)
    _FRAMES[name] = out
    return out


def pose_array(fr, kinds):
    return np.stack([fr["poses"][k] for k in kinds])


# ---------------------------------------------------------------- frozen cases (calls)
# frames: one name per frame of the call; kinds: the K pose kinds of every frame (rolled by b with roll=True, so that the frames
# of a call with shared maps differ); shared: one map tensor for all frames (sc_frame_stride 0); cams: per-frame camera table;
# ragged: packed rows + shapes; strict: ESAC_FLAG_STRICT_REFERENCE
def _case(name, frames, kinds, shared=False, cams=False, ragged=False, strict=False, roll=False):
    return dict(name=name, frames=frames, kinds=kinds, shared=shared, cams=cams, ragged=ragged, strict=strict, roll=roll)


CASES = [
    _case("g12x16_B1_K5_e0", ["g12x16"], POSE_KINDS),
    _case("g13x17s_B1_K5_e2", ["g13x17s"], POSE_KINDS),
    _case("g24x32_B1_K5_e0", ["g24x32"], POSE_KINDS),
    _case("g24x32_B1_K1_e2", ["g24x32e2"], ("perturbed",)),
    _case("shared_B3_K5", ["g12x16", "g12x16", "g12x16"], POSE_KINDS, shared=True, roll=True),
    _case("cams_B3_K1", ["g12x16", "cam1", "cam2"], ("winner",), cams=True, roll=True),
    _case("cams_B3_K5", ["cam2", "g12x16", "cam1"], POSE_KINDS, cams=True),
    _case("ragged_B3_K5", ["g12x16", "g16x12", "g13x17s"], POSE_KINDS, ragged=True),
    _case("nan_B1_K5", ["nan"], POSE_KINDS),
    _case("nan_strict_B1_K5", ["nan"], POSE_KINDS, strict=True),
    _case("allin_B1_K1", ["allin"], ("true",)),
    _case("allin_B1_K5", ["allin"], POSE_KINDS),
]


def case_kinds(case, b):
    kinds = list(case["kinds"])
    if case["roll"]:
        # K = 1: frame b takes the b-th kind of (winner, true, far); K = 5: the list rolled by b
        kinds = [("winner", "true", "far")[b % 3]] if len(kinds) == 1 else kinds[b % len(kinds):] + kinds[:b % len(kinds)]
    return kinds


def case_rows(case):
    """[(frame dict, kind, pose [6], expert)] per frame b: the rows [B][K] of the call"""
    return [[(frame(n), k, frame(n)["poses"][k], frame(n)["experts"][k]) for k in case_kinds(case, b)] for b, n in enumerate(case["frames"])]


_REF = {}


def reference(fr, kind, strict=False):
    """reference_row of a frozen frame's pose, computed once and shared"""
    key = (fr["name"], kind, bool(strict))
    if key not in _REF:
        _REF[key] = reference_row(fr["coords"][fr["experts"][kind]], fr["poses"][kind], fr["cam"], strict=strict)
    return _REF[key]


def golden():
    """{(frame, kind): dict(A_hi, A_lo [21], sse_hi, sse_lo)}: the 50-digit sums of tests/golden/verify/verify_ref50.npz"""
    z = np.load(GOLDEN)
    return {(str(f), str(k)): dict(A_hi=z["A_hi"][i], A_lo=z["A_lo"][i], sse_hi=float(z["sse_hi"][i]), sse_lo=float(z["sse_lo"][i]))
            for i, (f, k) in enumerate(zip(z["frame"], z["kind"]))}


def a_error(A21, g):
    """largest |A - A_50| / sqrt(A_ii A_jj) of 21 upper-triangle values against a golden entry"""
    d = np.sqrt(np.abs(np.diag(sym(g["A_hi"]))))
    scale = np.outer(d, d)[IU]
    return float(np.max(np.abs((np.asarray(A21, np.float64) - g["A_hi"]) - g["A_lo"]) / scale))


def sse_error(sse, g):
    return abs((sse - g["sse_hi"]) - g["sse_lo"]) / g["sse_hi"]


def sym(u21):
    A = np.zeros((6, 6))
    A[IU] = u21
    return A + np.triu(A, 1).T


def c_bar(g):
    """(relative 2-norm bar of C, cond_2 of the 50-digit A): first-order perturbation of an inverse"""
    cond = float(np.linalg.cond(sym(g["A_hi"])))
    return cond * BAR_A + BAR_INV_SPD6 * cond, cond


def check_row(row, fr, kind, strict, gold, oracle_score=None, label=""):
    """One row [64] (device or host probe) of a frozen pose against the reference with the bars above.  Returns the measured
    figures (for reports)."""
    ref = reference(fr, kind, strict)
    g = gold[(fr["name"], kind)]
    out = dict(label=label)
    assert row[5] == 0 and row[27] == 0, label
    assert row[1] == ref["n"], (label, row[1], ref["n"])
    if oracle_score is not None:
        if np.isnan(oracle_score):
            assert np.isnan(row[0]), (label, row[0])
        else:
            assert abs(row[0] - oracle_score) <= BAR_SCORE * abs(oracle_score), (label, row[0], oracle_score)
    if np.isnan(ref["score"]):
        assert np.isnan(row[0]), (label, row[0])
    else:
        # a sanity bound only (the oracle holds the score to 1e-12): the reference arithmetic rounds u, v and the error to float32
        # -- three roundings of at most 2^-17 px for pixels below 256 -- and a term's slope is at most beta / 4 per px
        assert abs(row[0] - ref["score"]) <= SCORE["alpha"] * SCORE["beta"] / 4 * 3 * 2.0 ** -17, (label, row[0], ref["score"])
    if ref["n"] > 0:
        out["sse"] = sse_error(row[2], g)
        out["A"] = a_error(row[6:27], g)
        assert out["sse"] <= BAR_SSE, (label, out)
        assert out["A"] <= BAR_A, (label, out)
    else:
        assert row[2] == 0 and (row[6:27] == 0).all(), label
    if ref["n"] < 4:
        assert row[4] == 1 and np.isnan(row[3]) and np.isnan(row[28:64]).all(), (label, row[3:5])
        return out
    assert row[4] == 0, (label, row[4])
    C = row[28:64].reshape(6, 6)
    assert (C == C.T).all(), label
    bar, cond = c_bar(g)
    A50 = sym(g["A_hi"])
    C_ref = (g["sse_hi"] / (2 * ref["n"] - 6)) * np.linalg.inv(A50)
    out["C"] = float(np.linalg.norm(C - C_ref, 2) / np.linalg.norm(C_ref, 2))
    out["C_bar"], out["cond"] = bar, cond
    assert out["C"] <= bar, (label, out)
    assert abs(row[3] - g["sse_hi"] / (2 * ref["n"] - 6)) <= 2 * BAR_SSE * row[3], (label, row[3])
    return out


def check_formats(a, c, fr, kind, label=""):
    """Row `a` of the rvec | tvec format and row `c` of the float32 4x4 format of one frozen pose: status and n equal, every figure
    within what the reference loses when the pose goes through float32 and back on the CPU, plus the bars both rows carry."""
    pose, expert = fr["poses"][kind], fr["experts"][kind]
    back = rt_from_camera_pose(camera_pose_from_rt(pose).astype(np.float32))
    ref, ref32 = reference(fr, kind), reference_row(fr["coords"][expert], back, fr["cam"])
    assert np.nanmin(np.abs(ref32["err"] - SCORE["tau"])) > BAND_PX and ref32["n"] == ref["n"], label  # (precondition)
    assert a[4] == c[4] and a[1] == c[1] == ref["n"], (label, a[:5], c[:5])
    # the score's errors are float32 values: a pose 1e-7 away moves u, v across float32 roundings the smooth reference does not
    # have -- at most three roundings of 2^-17 px per cell at a slope of at most beta / 4 (the sanity bound of check_row)
    assert abs(a[0] - c[0]) <= 1.01 * abs(ref32["score"] - ref["score"]) + SCORE["alpha"] * SCORE["beta"] / 4 * 3 * 2.0 ** -17, (label, a[0], c[0])
    if ref["n"] == 0:
        return
    assert abs(a[2] - c[2]) <= 1.01 * abs(ref32["sse"] - ref["sse"]) + 2 * BAR_SSE * a[2], (label, a[2], c[2])
    d = np.sqrt(np.diag(ref["A"]))
    scale = np.outer(d, d)[IU]
    loss = np.abs(ref32["A"] - ref["A"])[IU] / scale
    assert (np.abs(a[6:27] - c[6:27]) / scale <= 1.01 * loss + 2 * BAR_A).all(), (label, np.abs(a[6:27] - c[6:27]) / scale, loss)
    if ref["n"] >= 4:
        lossC = np.linalg.norm(ref32["C"] - ref["C"], 2) / np.linalg.norm(ref["C"], 2)
        got = np.linalg.norm(a[28:64].reshape(6, 6) - c[28:64].reshape(6, 6), 2) / np.linalg.norm(ref["C"], 2)
        assert got <= 1.01 * lossC + 2 * ref["cond"] * (BAR_A + BAR_INV_SPD6), (label, got, lossC)


def collinear_case():
    """A 12x16 map whose inliers are collinear: row 5's cells see points on the scene's x axis, every other cell a point far off.
    Under the pose rvec = 0 (the identity branch of the Rodrigues expansion, whose derivative is the three generators exactly) the
    rotation about x moves no point of that axis: the first row and column of A are exactly zero."""
    h, w, f, cx, cy, tz = 12, 16, 100.0, 64.0, 48.0, 2.0
    coords = np.empty((E, 3, h, w), np.float32)
    coords[:, 0], coords[:, 1], coords[:, 2] = 1e3, 1e3, 1.0
    px = np.arange(w) * 8 + 4
    coords[1, 0, 5] = (px - cx) / f * tz
    coords[1, 1, 5] = 0.0
    coords[1, 2, 5] = 0.0
    pose = np.array([0.0, 0.0, 0.0, 0.0, (5 * 8 + 4 - cy) / f * tz, tz])
    return coords, pose, dict(focal=f, ppx=cx, ppy=cy, shift=(0, 0))
