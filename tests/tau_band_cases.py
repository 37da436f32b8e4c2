"""Frames whose cells sit ON the threshold of the refinement's `err < tau` decision, and a plain float64 reference of the
reprojection error (numpy only; nothing here reads the kernels' headers).

Every refinement kernel decides `err < tau` per cell through three screens (fp32 with a guard, fp64 squared error against
tau +- band2, the reference's own float sequence for what is left).  A random room puts ~0.02 cells per pass into the second
screen's band, so the suite's ordinary frames never reach the third.  build_case() constructs maps that do: a cell's scene
point is back-projected so that its float64 error under the case's pose is tau + delta, rounded to float32 and then moved by
whole ulp steps of its three coordinates (a lattice search, evaluated exactly) until the float64 error of the FLOAT32 point is
as close to tau + delta as the lattice allows.

Cell classes (CLASS_NAMES): the delta classes (0, +-1e-7 .. +-5e-5 px, +-0.9 band2, +-1.1 band2), clear inliers, clear
outliers, cells beyond max_reproj, tuned cells BEHIND the camera (zc < 0: the reference has no cheirality test in refineHyp),
cells on the camera plane (zc == 0 exactly where a float32 point can hit it -- the identity-rotation case -- else the two
float32 neighbours of zc = 0 on either side) and two non-finite cells.
"""
import math

import numpy as np

FLOAT_DELTAS = (0.0, 1e-7, -1e-7, 1e-6, -1e-6, 3e-6, -3e-6, 1e-5, -1e-5, 5e-5, -5e-5)
BAND_DELTAS = (0.9, -0.9, 1.1, -1.1)  # times band2: both sides of both edges of the second screen
N_DELTA = len(FLOAT_DELTAS) + len(BAND_DELTAS)
CLS_INLIER, CLS_OUTLIER, CLS_BEYOND, CLS_PLANE, CLS_NONFINITE = N_DELTA, N_DELTA + 1, N_DELTA + 2, N_DELTA + 3, N_DELTA + 4
CLASS_NAMES = ["tau%+.0e" % d for d in FLOAT_DELTAS] + ["tau%+.1f*band2" % d for d in BAND_DELTAS] + \
    ["inlier", "outlier", "beyond_max_reproj", "camera_plane", "non_finite"]
MAX_TUNED = 2048

# the band of the second screen, as the two kernels' sources spell it (tests/test_tau_band_cases_host.py holds both copies
# and band2() below to this text)
BAND2_C = "2.4e-7 * ((double)(a.W > a.H ? a.W : a.H) * a.sub + abs(a.shift_x) + abs(a.shift_y) + (double)a.tau) + 2e-6"

_DEFAULT = dict(sub=8, shift=(0, 0), tau=10.0, max_reproj=100.0, focal=525.0, alpha=100.0, beta=0.5, origin=0.0, identity=False, seed=0)
CASES = {
    # the routes' smallest shapes
    "solo_scalar": dict(H=13, W=17, sub=37),
    "solo_vec": dict(H=12, W=16, sub=8),
    "solo_global_list": dict(H=96, W=96, sub=4),
    "coop": dict(H=128, W=260, sub=2),
    "team_min": dict(H=32, W=32, sub=8),
    "team_60x80": dict(H=60, W=80, sub=8),
    "team_odd": dict(H=33, W=47, sub=5),
    "team_max": dict(H=128, W=256, sub=2),
    # the scene 300-400 m from the world origin (the camera centre 350 m out): the tmag2 term of the fp32 guard
    "far_origin": dict(H=32, W=40, origin=350.0),
    "shifted": dict(H=32, W=40, shift=(5, -3), tau=6.0),
    # the parameters of test_gpu_semantics.py::test_pixel_coordinates_beyond_16_bits
    "wide_pixels": dict(H=18, W=24, sub=4000, focal=52500.0, ppx=48000.0, ppy=36000.0, shift=(-70000, 1234), tau=1000.0, beta=0.005,
                        max_reproj=10000.0),
    # parameter edges: one workgroup on 32x40, the team on 32x32
    "tau_tiny": dict(H=32, W=40, tau=5e-5),                     # tlo <= 0: lo2 = -1, everything under hi2 goes the exact route
    "tau_tiny_team": dict(H=32, W=32, tau=5e-5),
    # (seed: the generator's stream -- chosen where a case's first draw left a cell within 1e-4 px of tau at the NEXT pose)
    "clamp_at_tau": dict(H=32, W=40, max_reproj=10.0, seed=4),  # a clamped error EQUALS tau: not an inlier
    "clamp_at_tau_team": dict(H=32, W=32, max_reproj=10.0),
    "all_in": dict(H=32, W=40, max_reproj=5.0),                 # max_reproj < tau: every finite cell is an inlier
    "all_in_team": dict(H=32, W=32, max_reproj=5.0),
    # R = I and a float32 translation: zc = Z + t_z is exactly 0 at Z = -t_z -- the `z ? 1/z : 1` guard ON the band
    "camera_plane": dict(H=32, W=40, identity=True),
    "camera_plane_team": dict(H=32, W=32, identity=True),
}


def case_params(name):
    p = dict(_DEFAULT)
    p.update(CASES[name])
    p.setdefault("ppx", p["W"] * p["sub"] / 2.0)
    p.setdefault("ppy", p["H"] * p["sub"] / 2.0)
    p["shift_x"], p["shift_y"] = p["shift"]
    p["name"] = name
    return p


def tau32(params):
    """tau as the float the kernels and the reference compare against, widened."""
    return float(np.float32(params["tau"]))


def band2(params):
    """Half-width (px) of the band around tau inside which the fp64 screen does not decide."""
    extent = max(params["W"], params["H"]) * params["sub"]
    return 2.4e-7 * (extent + abs(params["shift_x"]) + abs(params["shift_y"]) + tau32(params)) + 2e-6


def oracle_kw(params, **more):
    kw = dict(shift_x=params["shift_x"], shift_y=params["shift_y"], focal=params["focal"], ppx=params["ppx"], ppy=params["ppy"],
              inlier_thresh=params["tau"], inlier_alpha=params["alpha"], inlier_beta=params["beta"], max_reproj=params["max_reproj"],
              sub_sampling=params["sub"])
    kw.update(more)
    return kw


def rodrigues(rvec):
    """exp([r]x) from the definition."""
    r = np.asarray(rvec, np.float64)
    th = math.sqrt(float(r @ r))
    if th == 0.0:
        return np.eye(3)
    k = r / th
    K = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    return math.cos(th) * np.eye(3) + (1.0 - math.cos(th)) * np.outer(k, k) + math.sin(th) * K


def pixel_grid(params):
    """Pixel positions of the cells, [H,W] each: col * sub + sub / 2 - shift (integer arithmetic)."""
    xs = np.arange(params["W"]) * params["sub"] + params["sub"] // 2 - params["shift_x"]
    ys = np.arange(params["H"]) * params["sub"] + params["sub"] // 2 - params["shift_y"]
    px, py = np.meshgrid(xs.astype(np.float64), ys.astype(np.float64))
    return px, py


def _err_points(R, t, X, px, py, params):
    """|pixel - projection| in float64 of points X[..., 3] (any leading shape; px, py broadcast against it).  A point ON the
    camera plane is projected with 1/z := 1, which is the operation's definition in the reference (`z ? 1/z : 1`)."""
    with np.errstate(all="ignore"):
        xc = R[0, 0] * X[..., 0] + R[0, 1] * X[..., 1] + R[0, 2] * X[..., 2] + t[0]
        yc = R[1, 0] * X[..., 0] + R[1, 1] * X[..., 1] + R[1, 2] * X[..., 2] + t[1]
        zc = R[2, 0] * X[..., 0] + R[2, 1] * X[..., 1] + R[2, 2] * X[..., 2] + t[2]
        iz = np.where(zc != 0.0, 1.0 / np.where(zc != 0.0, zc, 1.0), 1.0)
        u = params["focal"] * (xc * iz) + params["ppx"]
        v = params["focal"] * (yc * iz) + params["ppy"]
        return np.hypot(px - u, py - v)


def err64(pose, coords, params):
    """The reprojection error of every cell in float64, [H,W]: Rodrigues, R X + t, pinhole, hypot.  coords: [1,3,H,W] or [3,H,W]."""
    c = np.asarray(coords, np.float64).reshape(3, params["H"], params["W"])
    pose = np.asarray(pose, np.float64).reshape(6)
    px, py = pixel_grid(params)
    return _err_points(rodrigues(pose[:3]), pose[3:], np.moveaxis(c, 0, -1), px, py, params)


def plain_decision(e64, params):
    """`min(err, max_reproj) < tau` on the float64 error: what a device that stopped at the second screen would decide."""
    with np.errstate(invalid="ignore"):
        return np.minimum(e64, float(np.float32(params["max_reproj"]))) < tau32(params)


# ---------------------------------------------------------------------------------------------------------- construction
def _back_project(R, t, u, v, depth, params, plane=None):
    """Scene points (float64) that project to (u, v) at camera depth `depth`; plane: mask of points ON the camera plane
    (zc = 0, projected with 1/z := 1)."""
    z = np.where(plane, 1.0, depth) if plane is not None else depth
    Xc = np.stack([(u - params["ppx"]) / params["focal"] * z, (v - params["ppy"]) / params["focal"] * z,
                   np.where(plane, 0.0, depth) if plane is not None else depth], -1)
    return (Xc - t) @ R  # R^T (Xc - t)


def tune_points(R, t, X32, px, py, target, params, K=12, chunk=256):
    """Moves float32 points by whole ulp steps so that their float64 error gets as close to `target` as the lattice allows:
    steps n1, n2 in [-K, K] of the two coordinates the error is most sensitive to, the step of the finest one solved from the
    first-order model, every candidate evaluated exactly.  X32 [n,3] float32; returns the tuned [n,3] float32."""
    X32 = np.ascontiguousarray(X32, np.float32)
    out = X32.copy()
    ks = np.arange(-K, K + 1, dtype=np.float64)
    n1, n2 = [g.reshape(-1) for g in np.meshgrid(ks, ks, indexing="ij")]
    for lo in range(0, len(X32), chunk):
        x0 = X32[lo:lo + chunk].astype(np.float64)
        ulp = np.spacing(np.abs(X32[lo:lo + chunk])).astype(np.float64)
        ppx, ppy, tg = px[lo:lo + chunk], py[lo:lo + chunk], target[lo:lo + chunk]
        e0 = _err_points(R, t, x0, ppx, ppy, params)
        g = np.stack([_err_points(R, t, x0 + ulp * np.eye(3)[k], ppx, ppy, params) - e0 for k in range(3)], -1)
        with np.errstate(invalid="ignore"):
            g = np.where(np.isfinite(g) & (g != 0.0), g, 1e300)
        order = np.argsort(-np.abs(g), axis=1)  # coarsest first, finest last
        rows = np.arange(len(x0))
        g1, g2, g3 = (g[rows, order[:, k]] for k in range(3))
        n3 = np.rint(((tg - e0)[:, None] - g1[:, None] * n1 - g2[:, None] * n2) / g3[:, None])
        n3 = np.clip(n3, -4.0 * K, 4.0 * K)
        steps = np.zeros((len(x0), len(n1), 3))
        for k, n in enumerate((np.broadcast_to(n1, n3.shape), np.broadcast_to(n2, n3.shape), n3)):
            np.put_along_axis(steps, np.broadcast_to(order[:, None, k:k + 1], n3.shape + (1,)), n[..., None], axis=2)
        cand = (x0[:, None, :] + steps * ulp[:, None, :]).astype(np.float32)
        e = _err_points(R, t, cand.astype(np.float64), ppx[:, None], ppy[:, None], params)
        with np.errstate(invalid="ignore"):
            miss = np.where(np.isfinite(e), np.abs(e - tg[:, None]), np.inf)
        best = np.argmin(miss, axis=1)
        out[lo:lo + chunk] = cand[rows, best]
    return out


def tuned_cells(P, n, rng):
    """Which cells of a P-cell grid are tuned: n random ones, or, on a grid of more than twice MAX_TUNED cells, the first and last cell of every slice a team
    of 2..32 members, a cooperating workgroup (8192 cells), an error-pass trip (2048) and a wavefront's share of a trip can own
    -- as far as n allows, the coarsest ranges first -- then the grid's last 64 cells (the partial trip) and an even spread."""
    if P <= 2 * MAX_TUNED:
        return np.sort(rng.choice(P, size=min(n, P), replace=False))
    edges = [0, P - 1]
    for G in (32, 19, 16, 10, 8, 7, 5, 4, 2):
        for g in range(1, G):
            edges += [g * P // G - 1, g * P // G]
    for step in (8192, 2048, 256):
        for c in range(step, P, step):
            edges += [c - 1, c]
    edges += list(range(P - 64, P))
    picked = list(dict.fromkeys(edges))[:n // 2]
    spread = np.linspace(0, P - 1, n - len(picked)).astype(np.int64) + rng.integers(0, 3, size=n - len(picked))
    return np.unique(np.clip(np.concatenate([np.asarray(picked, np.int64), spread]), 0, P - 1))


def case_pose(params, rng):
    """The written hypothesis (scene -> camera) of a case."""
    if params["identity"]:
        return np.array([0.0, 0.0, 0.0, 0.25, -0.5, 2.0])  # every component a float32
    rvec = np.array([0.21, -0.33, 0.12]) + rng.uniform(-0.05, 0.05, size=3)
    centre = np.array([1.0, -0.5, 0.7]) * (1.0 if params["origin"] == 0.0 else 0.0) + params["origin"] * np.array([0.6, 0.0, 0.8])
    return np.concatenate([rvec, -rodrigues(rvec) @ centre])


def build_map(params, pose, rng, keep=None, base=None, tuned_frac=0.7, non_finite=True, generic=None):
    """The map of a case for `pose`.  keep: mask [H,W] of cells that stay what `base` ([3,H,W] float32) holds (the sampled cells
    of the sampled-hypothesis fixtures).  non_finite=False: the two non-finite cells are clear outliers instead.  generic: mask
    [H,W] of cells that must not be tuned (they keep the clear class drawn for them; every other cell is what it is without
    the mask: the random stream does not depend on it).  Returns coords [1,3,H,W] float32, cls [H,W], behind [H,W]."""
    H, W = params["H"], params["W"]
    P = H * W
    R, t = rodrigues(pose[:3]), np.asarray(pose[3:], np.float64)
    tau, b2, maxr = tau32(params), band2(params), float(np.float32(params["max_reproj"]))
    px, py = [a.reshape(-1) for a in pixel_grid(params)]
    cls = np.empty(P, np.int64)
    # generic cells: 55 % clear inliers, 30 % clear outliers, 15 % beyond max_reproj
    r = rng.uniform(size=P)
    cls[:] = np.where(r < 0.55, CLS_INLIER, np.where(r < 0.85, CLS_OUTLIER, CLS_BEYOND))
    tuned = tuned_cells(P, min(MAX_TUNED, int(tuned_frac * P)), rng)
    clear = cls.copy()
    free = np.ones(P, bool)
    free[tuned] = False
    if keep is not None:
        free &= ~keep.reshape(-1)
    special = rng.choice(np.flatnonzero(free), size=6, replace=False)  # four cells at the camera plane, two non-finite ones
    cls[tuned] = rng.permutation(len(tuned)) % N_DELTA
    if generic is not None:
        cls = np.where(generic.reshape(-1), clear, cls)
    delta = np.array(list(FLOAT_DELTAS) + [d * b2 for d in BAND_DELTAS] + [0.0] * 5)[cls]
    e = np.abs(tau + delta)
    gen = rng.uniform(size=P)
    e = np.where(cls == CLS_INLIER, (0.05 + 0.65 * gen) * tau, e)
    e = np.where(cls == CLS_OUTLIER, (1.5 + 2.5 * gen) * tau, e)
    e = np.where(cls == CLS_BEYOND, (1.5 + 1.5 * gen) * max(maxr, 5.0 * tau), e)
    th = rng.uniform(0.0, 2.0 * math.pi, size=P)
    # the clear inliers miss to one side: the re-fit then moves the pose by pixels, which takes the tuned cells far off the band
    # at the NEXT pose (the second pass can be compared, test_tau_band_cases_host.py: the next pose is clear of the band)
    th = np.where(cls == CLS_INLIER, rng.uniform(0.0, 2.0 * math.pi) + rng.normal(0.0, 0.5, size=P), th)
    depth = rng.uniform(1.5, 6.0, size=P)
    is_tuned = cls < N_DELTA
    behind = is_tuned & (rng.uniform(size=P) < 0.06)
    depth = np.where(behind, -depth, depth)
    plane = np.zeros(P, bool)
    if params["identity"]:  # zc == 0 exactly, ON the band: four cells at tau + delta of the first classes, tuned in X and Y
        plane[special[:4]] = True
        e[special[:4]] = np.abs(tau + np.array([0.0, 1e-6, -1e-6, 3e-6]))
    u, v = px - e * np.cos(th), py - e * np.sin(th)
    X = _back_project(R, t, u, v, depth, params, plane)
    if params["identity"]:
        X[plane, 2] = -t[2]
    X32 = X.astype(np.float32)
    sel = np.flatnonzero(is_tuned | plane)
    X32[sel] = tune_points(R, t, X32[sel], px[sel], py[sel], e[sel], params)
    if params["identity"]:
        assert np.all(X32[plane, 2].astype(np.float64) + t[2] == 0.0)
    else:  # the float32 neighbours of zc = 0: two cells just behind the plane, two just in front
        for j, c in enumerate(special[:4]):
            x = X32[c].astype(np.float64)
            zc0 = R[2] @ x + t[2]
            z0 = np.float32(x[2] - zc0 / R[2, 2])
            cands = [z0]
            for _ in range(3):
                cands = [np.nextafter(cands[0], np.float32(-np.inf))] + cands + [np.nextafter(cands[-1], np.float32(np.inf))]
            zc = np.array([R[2, 0] * x[0] + R[2, 1] * x[1] + R[2, 2] * float(z) + t[2] for z in cands])
            if np.any(zc == 0.0):
                pick = int(np.flatnonzero(zc == 0.0)[0])
            elif j % 2 == 0:
                pick = int(np.argmax(np.where(zc < 0, zc, -np.inf)))
            else:
                pick = int(np.argmin(np.where(zc > 0, zc, np.inf)))
            X32[c, 2] = cands[pick]
    cls[special[:4]] = CLS_PLANE
    if non_finite:
        X32[special[4], 0] = np.nan
        X32[special[5], 2] = np.inf
        cls[special[4:]] = CLS_NONFINITE
    coords = np.ascontiguousarray(X32.T.reshape(1, 3, H, W))
    cls = cls.reshape(H, W)
    cls_behind = behind.reshape(H, W).copy()
    if keep is not None:
        coords[0][:, keep] = base[:, keep]
        cls[keep] = CLS_INLIER
        cls_behind[keep] = False
    return coords, cls, cls_behind


_CACHE = {}


def build_case(name):
    """The fixture of one case (cached; fixed seed): dict(name, params, coords [1,3,H,W] float32, hyp [1,6] float64, cls [H,W]
    (index into CLASS_NAMES), behind [H,W] bool (tuned from zc < 0), tuned [H,W] bool, err64 [H,W], band2)."""
    if name in _CACHE:
        return _CACHE[name]
    params = case_params(name)
    rng = np.random.default_rng([sorted(CASES).index(name), 20260, params["seed"]])
    pose = case_pose(params, rng)
    coords, cls, behind = build_map(params, pose, rng)
    case = dict(name=name, params=params, coords=coords, hyp=pose.reshape(1, 6).copy(), cls=cls, behind=behind, tuned=cls < N_DELTA,
                err64=err64(pose, coords, params), band2=band2(params))
    _CACHE[name] = case
    return case


def decoy(hyp):
    """The written hypothesis and a far decoy behind it ([2,6]): the selection still runs, the written one wins."""
    far = hyp.reshape(6).copy()
    far[3:] += np.array([40.0, -25.0, 60.0])
    return np.stack([hyp.reshape(6), far])


def describe_cells(case, cells, got, want):
    """One line per mismatching cell: class, err64 - tau, both decisions."""
    tau = tau32(case["params"])
    W = case["params"]["W"]
    lines = []
    for c in list(cells)[:40]:
        y, x = divmod(int(c), W)
        lines.append("cell (%d,%d) %s%s: err64 - tau = %+.3e, device %s, reference %s"
                     % (y, x, CLASS_NAMES[case["cls"][y, x]], " (behind)" if case["behind"][y, x] else "", case["err64"][y, x] - tau,
                        got.reshape(-1)[c], want.reshape(-1)[c]))
    return "\n".join(lines)


# the second pass (max_ref_steps = 2) is compared where the pose after the first re-fit is clear of the band; not on
#   tau_tiny*       tau = 5e-5 px: every clear inlier lies within 1e-4 px of tau at any pose
#   all_in*         every finite cell is an inlier at every pose: nothing a second pass could get wrong that the first does not show
#   camera_plane*   the cells ON the camera plane are inliers of the re-fit (1/z := 1), the reference's LM leaves the pose where it
#                   was to 1e-17 and the tuned cells stay on the band
SECOND_PASS_CASES = [n for n in CASES if not n.startswith(("tau_tiny", "all_in", "camera_plane"))]
# where a decision exists to disagree on (max_reproj < tau forces every one)
DECIDING_CASES = [n for n in CASES if not n.startswith("all_in")]

_REF = {}


def reference(oracle, name, max_ref_steps=1):
    """The oracle on a case (cached): hypotheses written (the case's and a decoy behind it), one refinement step by default."""
    key = (name, max_ref_steps)
    if key not in _REF:
        c = build_case(name)
        ref = oracle.forward(c["coords"], np.zeros(2, np.int64), in_hyps=decoy(c["hyp"]), max_ref_steps=max_ref_steps,
                             **oracle_kw(c["params"]))
        assert ref["winner"] == 0, "the decoy won"
        _REF[key] = ref
    return _REF[key]


# ------------------------------------------------------------------------------- fixtures whose hypotheses are SAMPLED
# The training call, a batch and the headline call sample their own hypotheses: nothing can be written.  So: a noise-free
# map; the cells that the sampler's tries drew stay (on the 32x40 frames every hypothesis is accepted at its first try), every
# other cell goes on the band of hypothesis 0's pose, which leaves tries, cells and hypotheses what they were.  Device and
# oracle hypotheses agree to ~1e-12 where the sampled P3P is well-conditioned (measured on hypothesis 0 of these frames:
# <= 2.2e-13 on 32x40, <= 2.8e-11 on 12x16), not in bits, so only DECISION-STABLE cells stay tuned: a cell whose first-pass
# decision changes under +-1e-9 in any of the six pose components is reset to the clear class drawn for it.
SAMPLED_SEED = 1305
_SAMPLED = {}


def sampled_frame(oracle, k, call, H=32, W=40, sub=8, N=4):
    """dict(coords [1,3,H,W], ha [N], params, kw (the oracle's keywords), ref (the oracle's forward on the map, N hypotheses), ref1
    (the same with hypothesis 0 alone), nearest_later (px from tau of the nearest cell at any later pose of ref1's refinement),
    cls, err64 / first_map / first_errs (float64 error, the oracle's first-pass map and float errors at hypothesis 0), tuned,
    removed (cells the stability filter reset), band2)."""
    from esac_amd import synthetic as S
    key = (k, call, H, W, sub, N)
    if key in _SAMPLED:
        return _SAMPLED[key]
    ha = np.zeros(N, np.int64)
    f = S.make_frame(k, H=H, W=W, sub=sub, noise=0.0, outlier_frac=0.0, ppx=W * sub / 2.0, ppy=H * sub / 2.0)
    params = dict(_DEFAULT, H=H, W=W, sub=sub, ppx=f["ppx"], ppy=f["ppy"], shift_x=0, shift_y=0, name="sampled_%d" % k)
    kw = oracle_kw(params, seed=SAMPLED_SEED, call=call)
    clean = oracle.forward(f["coords"], ha, **kw)
    assert ((clean["tries"] >= 0) & (clean["tries"] <= 8)).all()  # (on the 32x40 frames: every hypothesis accepted at its first try)
    keep = np.zeros((H, W), bool)  # every cell a try drew, the rejected tries' too: each try decides on its own four cells
    for h in range(N):
        for t in range(int(clean["tries"][h]) + 1):
            xy = np.asarray(oracle.draw_cells(SAMPLED_SEED, call, h, t, W, H)).reshape(4, 2)
            keep[xy[:, 1], xy[:, 0]] = True
    assert keep[clean["sample_xy"][..., 1].reshape(-1), clean["sample_xy"][..., 0].reshape(-1)].all()
    pose = clean["hyps"][0].copy()
    one = np.zeros(1, np.int64)

    def build(generic):
        rng = np.random.default_rng([k, call, 20261])
        return build_map(params, pose, rng, keep=keep, base=f["coords"][0], tuned_frac=0.9, non_finite=False, generic=generic)

    def first_pass(coords, hyp):
        return oracle.forward(coords, one, in_hyps=hyp.reshape(1, 6), max_ref_steps=1, **kw)["inlier_map"]

    def unstable(coords):
        base = first_pass(coords, pose)
        moved = np.zeros((H, W), bool)
        for j in range(6):
            for s in (-1e-9, 1e-9):
                h = pose.copy()
                h[j] += s
                moved |= first_pass(coords, h) != base
        return moved

    coords, cls, behind = build(None)
    reset = unstable(coords) & (cls < N_DELTA)
    coords, cls, behind = build(reset)
    assert not (unstable(coords) & (cls < N_DELTA)).any()
    ref = oracle.forward(coords, ha, **kw)
    ref1 = oracle.forward(coords, one, **kw)  # one hypothesis: hypothesis 0 is the winner, the refinement starts ON the band
    # the poses that refinement evaluates after its first re-fit: the fixture must be clear of the band at each of them
    later = [oracle.forward(coords, one, max_ref_steps=s, **kw)["refined"] for s in range(1, ref1["ref_steps"] + 1)]
    with np.errstate(invalid="ignore"):
        nearest = min(float(np.nanmin(np.abs(err64(q, coords, params) - tau32(params)))) for q in later)
    # the band cells changed nothing of the sampling
    assert np.array_equal(ref["tries"], clean["tries"]) and np.array_equal(ref["sample_xy"], clean["sample_xy"])
    assert np.array_equal(ref["hyps"].view(np.uint64), clean["hyps"].view(np.uint64))
    out = dict(coords=coords, ha=ha, params=params, kw=kw, ref=ref, ref1=ref1, nearest_later=nearest, cls=cls, behind=behind,
               tuned=cls < N_DELTA, removed=int(reset.sum()), gt_pose=f["gt_pose"],
               err64=err64(pose, coords, params), band2=band2(params), hyp=pose.reshape(1, 6), first_map=first_pass(coords, pose),
               first_errs=oracle.forward(coords, one, in_hyps=pose.reshape(1, 6), max_ref_steps=0, **kw)["winner_errs"])
    _SAMPLED[key] = out
    return out


# (k of synthetic.make_frame, call, H, W, sub): three 32x40 frames of one batch (the teams; frame b samples with call + b),
# 33 frames of 12x16 (one workgroup per frame)
TEAM_FRAMES = [(900 + b, 70 + b, 32, 40, 8) for b in range(3)]
SMALL_FRAMES = [(940 + b, 100 + b, 12, 16, 40) for b in range(33)]
# the headline call's own grid, one hypothesis: a team of ten, two cells per lane, the 16-wide exchange (k_refine_team_route<2, 16>)
HEADLINE_FRAME = (980, 130, 60, 80, 8)


def sampled_figures(c):
    """(cells in band, cells where the reference's float decision and the float64 one differ, worst |reference - fp64| / band2)
    of a sampled-hypothesis fixture, counted on what the stability filter left."""
    tau = tau32(c["params"])
    with np.errstate(invalid="ignore"):
        in_band = c["tuned"] & (np.abs(c["err64"] - tau) < c["band2"])
        near = np.abs(c["err64"] - tau) < 1e-3
    disagree = (c["first_map"] != 0) != plain_decision(c["err64"], c["params"])
    clamped = np.minimum(c["err64"], float(np.float32(c["params"]["max_reproj"])))
    worst = float(np.abs(c["first_errs"].astype(np.float64) - clamped)[near].max())
    return int(in_band.sum()), int(disagree.sum()), worst / c["band2"]
