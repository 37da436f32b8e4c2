"""The case table of the fp32 ranking-score tests: adversarial maps x score routes x parameter sets, fixed seeds, numpy only.

A case is a dict: name, coords [E,3,H,W] float32, assign [N] int64, hyps [N,6] float64 (rvec, t: scene -> camera), the call's
parameters (H, W, sub, focal, ppx, ppy, alpha, beta, tau, max_reproj), the score route ("stream" / "tiled"), `poisoned` (the
expert whose map was tampered with, or None), `winner_check` and `tie_exception` (mid_3e38, see test_gpu_rank_score.py).
reference(case) is the fp64 score vector of tests/rank_score_ref.py, computed once per case and shared by the CPU
preconditions (tests/test_rank_score_ref_host.py) and the GPU tests (tests/test_gpu_rank_score.py).
"""
import numpy as np

from esac_amd import synthetic as S
from tests import rank_score_ref as ref

FOCAL, PPX, PPY = 525.0, 320.0, 240.0
GRID = dict(H=40, W=64, sub=10)      # 2560 cells: 640 float4 groups (> 512 threads), 4 sub-tiles of 768 cells, the last partly filled
ODD_GRID = dict(H=37, W=51, sub=12)  # W % 4 != 0: the scalar-load path of the stream
FAR = np.array([12000.0, -8000.0, 9500.0])  # a world-frame outdoor map
PARAMS = {
    "default": dict(alpha=100.0, beta=0.5, tau=10.0, max_reproj=100.0),
    "steep": dict(alpha=100.0, beta=5.0, tau=3.0, max_reproj=100.0),
    "neg": dict(alpha=100.0, beta=-0.5, tau=10.0, max_reproj=100.0),
}
# route name -> (score_shape, grid, N)
ROUTES = {
    "stream": ("stream", GRID, 300),          # k_score_fast<512>, float4 loads
    "stream_scalar": ("stream", ODD_GRID, 300),  # k_score_fast<512>, scalar loads
    "stream_2100": ("stream", GRID, 2100),    # N > 2048: k_score_fast<256>
    "tiled": ("tiled", GRID, 300),            # k_score_tiled<NEG>
}
FIRST_LAST = ("stream", "tiled")
ALL_ROUTES = tuple(ROUTES)
MAPS = {  # map name -> routes it runs on (default parameters)
    "healthy": ALL_ROUTES, "mid_1e3": FIRST_LAST, "mid_1e5": ALL_ROUTES, "mid_3e38": FIRST_LAST, "blotch_1e5": FIRST_LAST,
    "far": FIRST_LAST, "far_mid_nan": FIRST_LAST, "far_mid_inf": FIRST_LAST, "far_blotch_nan": FIRST_LAST,
    # fewer than two finite quarter-point cells (map_centre's last rule): the middle cell if finite, else the finite one
    "far_q3_nan": ("stream",), "far_q3_mid_nan": ("stream",),
}
CHUNK_COUNTS = (0, 1, 63, 64, 65, 255, 256, 257, 513, 0)  # hypotheses per expert: around the 64-wide store and the 256-wide chunk
FRAME_SEED = 300


def margin(case):
    """The default re-score band of the call (call_policy.hpp: call_scalars)."""
    return abs(case["alpha"]) * (1e-3 + 2.0 / (case["H"] * case["W"]))


def oracle_bound(case):
    """|fp64 reference - reference arithmetic|: the reference rounds a projected pixel to float (< 1e-4 px at coordinates
    < 1024 -- a larger coordinate is an error beyond maxReproj) and the sigmoid's slope is at most |beta| / 4."""
    return abs(case["alpha"]) * abs(case["beta"]) / 4.0 * 1e-4


def _unit(rng):
    v = rng.normal(size=3)
    return v / np.linalg.norm(v)


def make_hyps(gt_pose, centre, N, rng):
    """Index 0: the ground-truth pose; then perturbations of size 10^U(-3,-1) in rotation and translation; the last four wild."""
    R0 = gt_pose[:3, :3].T  # gt_pose is camera -> scene
    t0 = -R0 @ gt_pose[:3, 3]
    poses = [(R0, t0)]
    for _ in range(N - 5):
        dr = _unit(rng) * 10.0 ** rng.uniform(-3.0, -1.0)
        dt = _unit(rng) * 10.0 ** rng.uniform(-3.0, -1.0)
        dR = ref.rodrigues(dr)
        poses.append((dR @ R0, dR @ t0 + dt))  # in the camera's frame: the same perturbation wherever the map sits in the world
    # a camera 1e10 m from the scene.  From there the scene is one point: every cell projects to ppx + focal = 845, 210 px right
    # of the last pixel centre, so the true error of every cell is clamped -- as the fp32 stream reads it, whose d2n zc^2
    # overflows (tests/test_gpu_edge.py::test_fast_score_of_a_hypothesis_far_beyond_the_scene pins that clamp).  A direction
    # whose point falls INSIDE the image has the ~4 cells around it as true inliers, which the clamp cannot see: such a
    # hypothesis reads 3.5 cells' weight too low, 1.54 x (margin / 2) on this grid: held to its own bound of 4 cells by
    # tests/test_gpu_rank_score.py::test_a_camera_beyond_fp32_range_reads_at_most_four_cells_low (in_image_far_camera below).
    poses.append((R0, t0 + np.array([1.0e10, 0.0, 1.0e10]) / np.sqrt(2.0)))
    poses.append((R0, -R0 @ centre))                                  # a camera inside the point cloud
    flip = ref.rodrigues(np.array([0.0, np.pi, 0.0]))
    poses.append((flip @ R0, flip @ t0))                              # flipped by 180 degrees about the camera's y axis
    poses.append((R0, t0 + np.array([50.0, 0.0, 0.0])))              # 50 m to the side
    return np.array([np.concatenate([ref.rotation_vector(R), t]) for R, t in poses])


def _poison(coords, e, name):
    _, _, H, W = coords.shape
    my, mx = H >> 1, W >> 1
    sign = np.array([1.0, -1.0, 1.0], np.float32)
    if "_q3_" in name:  # three of the four quarter-point cells (rows H/4, 3H/4 x columns W/4, 3W/4)
        for y, x in (((H >> 2), (W >> 2)), ((H >> 2), (3 * W) >> 2), ((3 * H) >> 2, (W >> 2))):
            coords[e, :, y, x] = np.nan
    if name.endswith("blotch_1e5"):
        coords[e, :, my - 1:my + 2, mx - 1:mx + 2] = (np.float32(1e5) * sign)[:, None, None]
    elif name.endswith("blotch_nan"):
        coords[e, :, my - 1:my + 2, mx - 1:mx + 2] = np.nan
    elif name.endswith("mid_nan"):
        coords[e, :, my, mx] = np.nan
    elif name.endswith("mid_inf"):
        coords[e, :, my, mx] = np.float32(np.inf) * sign
    elif "mid_" in name:
        coords[e, :, my, mx] = np.float32(float(name.split("mid_")[1])) * sign


def in_image_far_camera(case):
    """The hypotheses of `case` with the far camera moved to t + (1e9, -2e9, 1e10) -- the pose of tests/test_gpu_edge.py::
    test_fast_score_of_a_hypothesis_far_beyond_the_scene.  From there every cell projects to pixel (372.5, 135), inside the
    image.  Returns (hyps, index of that hypothesis)."""
    k = case["N"] - 4
    hyps = case["hyps"].copy()
    gt = ref.rodrigues(hyps[0, :3])
    hyps[k, :3] = hyps[0, :3]
    hyps[k, 3:] = hyps[0, 3:] + np.array([1.0e9, -2.0e9, 1.0e10])
    assert np.allclose(ref.rodrigues(hyps[k, :3]), gt)
    return hyps, k


def build(map_name, route, params="default"):
    shape, grid, N = ROUTES[route]
    E, te = 2, 1
    f = S.make_frame(FRAME_SEED, E=E, true_expert=te, H=grid["H"], W=grid["W"], sub=grid["sub"], focal=FOCAL, ppx=PPX, ppy=PPY)
    coords, gt = f["coords"].astype(np.float64), f["gt_pose"].copy()
    centre = coords[te].reshape(3, -1).mean(axis=1)
    if map_name.startswith("far"):
        coords += FAR[None, :, None, None]
        gt[:3, 3] += FAR
        centre = centre + FAR
    coords = coords.astype(np.float32)
    poisoned = None
    if map_name not in ("healthy", "far"):
        _poison(coords, te, map_name)
        poisoned = te
    rng = np.random.default_rng([FRAME_SEED, N])
    hyps = make_hyps(gt, centre, N, rng)
    assign = np.full(N, te, np.int64)
    assign[3::5] = 1 - te  # every fifth hypothesis on the wrong expert, same poses
    name = "-".join([map_name, route] + ([params] if params != "default" else []))
    return dict(name=name, coords=coords, assign=assign, hyps=hyps, E=E, N=N, route=shape, focal=FOCAL, ppx=PPX, ppy=PPY,
                poisoned=poisoned, winner_check=params != "neg", tie_exception=map_name == "mid_3e38", **grid, **PARAMS[params])


def build_chunks():
    E, te = len(CHUNK_COUNTS), 8
    N = sum(CHUNK_COUNTS)  # 1474 > 1024: two bucket workgroups
    f = S.make_frame(FRAME_SEED + 1, E=E, true_expert=te, focal=FOCAL, ppx=PPX, ppy=PPY, **GRID)
    rng = np.random.default_rng([FRAME_SEED + 1, N])
    hyps = make_hyps(f["gt_pose"], f["coords"][te].astype(np.float64).reshape(3, -1).mean(axis=1), N, rng)
    assign = np.repeat(np.arange(E, dtype=np.int64), CHUNK_COUNTS)
    rng.shuffle(assign)  # interleaved: the order sorted by expert is not the index order
    first = int(np.nonzero(assign == te)[0][0])
    assign[[0, first]] = assign[[first, 0]]  # the ground-truth pose on the true expert
    return dict(name="chunks", coords=f["coords"], assign=assign, hyps=hyps, E=E, N=N, route="tiled", focal=FOCAL, ppx=PPX, ppy=PPY,
                poisoned=None, winner_check=True, tie_exception=False, **GRID, **PARAMS["default"])


def _table():
    t = {}
    for m, routes in MAPS.items():
        for r in routes:
            t["-".join([m, r])] = (build, (m, r))
    for prm in ("steep", "neg"):
        for m in ("healthy", "far"):
            for r in FIRST_LAST:
                t["-".join([m, r, prm])] = (build, (m, r, prm))
    t["chunks"] = (build_chunks, ())
    return t


TABLE = _table()
NAMES = tuple(TABLE)
_cases, _refs = {}, {}


def get(name):
    if name not in _cases:
        fn, args = TABLE[name]
        c = fn(*args)
        assert c["name"] == name
        for k in ("coords", "assign", "hyps"):
            c[k].setflags(write=False)
        _cases[name] = c
    return _cases[name]


def reference(case):
    """fp64 scores [N] of the case (computed once, read-only)."""
    name = case["name"]
    if name not in _refs:
        r = ref.scores(case["coords"], case["assign"], case["hyps"], case["focal"], case["ppx"], case["ppy"], case["sub"], (0, 0),
                       case["alpha"], case["beta"], case["tau"], case["max_reproj"])
        r.setflags(write=False)
        _refs[name] = r
    return _refs[name]
