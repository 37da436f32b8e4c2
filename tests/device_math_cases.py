"""Inputs of the per-function math tests, generated once with fixed seeds and shared by the CPU suite (the host build of the
math headers, tests/test_device_math_cases_host.py) and the GPU suite (the device build, tests/test_gpu_device_math.py).
The array layouts are those of tests/native/math_probe_bodies.hpp."""
import numpy as np

EPS = 2.0 ** -52
ROT_OUT, PT_N, PT_IN, PT_OUT, SOLVE_IN, SOLVE_OUT, LANE_IN, LANE_OUT = 88, 12, 9 + 6 * 12, 6 * 12 + 28, 28, 80, 35, 75
OPS = {"fast_rcp": 0, "scr_sqrt": 1, "cbrt_pos": 2, "cos_third_acos": 3, "lane_rcp_neg": 4}


# ------------------------------------------------------------------------------------------------------------ scalars
def mantissa_edges():
    """1, 1 + eps, 2 - eps, 1.5 -+ eps and all-ones / alternating bit patterns, in [1, 2)."""
    bits = [0x3FF0000000000000, 0x3FF0000000000001, 0x3FFFFFFFFFFFFFFF, 0x3FF7FFFFFFFFFFFF, 0x3FF8000000000000, 0x3FF8000000000001,
            0x3FF00000FFFFFFFF, 0x3FFFFFFF00000000, 0x3FF5555555555555, 0x3FFAAAAAAAAAAAAA, 0x3FF0000000FFFFFF, 0x3FFFFFFFFFFFFFFE]
    return np.array(bits, dtype=np.uint64).view(np.float64)


def _log_uniform(rng, lo, hi, n):
    return np.exp(rng.uniform(np.log(lo), np.log(hi), n))


def rcp_inputs():
    """fast_rcp / lane_rcp_neg: magnitudes log-uniform in 2^+-300 with both signs, mantissa edges at several exponents, and the
    ranges of the callers: depths, squared angles, pivots."""
    rng = np.random.default_rng(101)
    wide = np.ldexp(rng.uniform(1.0, 2.0, 24000), rng.integers(-300, 300, 24000)) * rng.choice([-1.0, 1.0], 24000)
    edges = np.concatenate([np.ldexp(mantissa_edges(), e) for e in (-300, -52, -1, 0, 1, 2, 53, 299)])
    edges = np.concatenate([edges, -edges])
    callers = np.concatenate([_log_uniform(rng, 1e-3, 1e3, 12000), -_log_uniform(rng, 1e-3, 1e3, 2000),   # depths
                              _log_uniform(rng, 1e-31, 40.0, 8000), [40.0, 10.0, np.nextafter(10.0, 0), np.nextafter(10.0, 11)],  # |rvec|^2
                              _log_uniform(rng, 1e-12, 1e12, 12000)])                                      # pivots
    return np.concatenate([wide, edges, callers])


def sqrt_inputs():
    """scr_sqrt: squared lengths, cosines / discriminants in [0, 1], a wide range, mantissa edges at even and odd exponents."""
    rng = np.random.default_rng(102)
    edges = np.concatenate([np.ldexp(mantissa_edges(), e) for e in (-301, -300, -3, -2, -1, 0, 1, 2, 3, 300, 301)])
    return np.concatenate([_log_uniform(rng, 1e-6, 1e6, 20000), rng.uniform(0.0, 1.0, 12000), _log_uniform(rng, 1e-16, 1.0, 6000),
                           np.ldexp(rng.uniform(1.0, 2.0, 16000), rng.integers(-300, 300, 16000)), edges])


def cbrt_inputs():
    """cbrt_pos: 1e-300 < a < 1e300 log-uniform, ordinary magnitudes, mantissa edges at every residue of the exponent mod 3
    (both signs of the exponent), and both sides of the two limits past which the routine falls back to pow."""
    rng = np.random.default_rng(103)
    edges = np.concatenate([np.ldexp(mantissa_edges(), e) for e in (-302, -301, -300, -5, -4, -3, -2, -1, 0, 1, 2, 3, 4, 5, 300, 301, 302)])
    limits = np.array([np.nextafter(1e-300, 0), 1e-300, np.nextafter(1e-300, 1), np.nextafter(1e300, 0), 1e300, np.nextafter(1e300, np.inf)])
    return np.concatenate([_log_uniform(rng, 1e-300, 1e300, 12000), _log_uniform(rng, 1e-8, 1e8, 12000), edges, limits])


def cos3_inputs():
    """cos_third_acos: c in [-1, 1], dense around the switch to the library route (-0.999), around +-1 and around 0, mantissa
    edges of both signs."""
    rng = np.random.default_rng(104)
    tiny = np.concatenate([_log_uniform(rng, 1e-300, 1e-3, 1000), 10.0 ** -np.arange(1.0, 17.0)])
    edges = np.concatenate([np.ldexp(mantissa_edges(), e) for e in (-1, -2, -3, -30)])  # mantissa edges in [0.5, 1), [0.25, 0.5), ...
    at = [-0.999, np.nextafter(-0.999, -1), np.nextafter(-0.999, 0), -1.0, 1.0, 0.0, np.nextafter(1.0, 0), np.nextafter(-1.0, 0), 0.5, -0.5]
    return np.concatenate([rng.uniform(-1.0, 1.0, 12000), -0.999 + rng.uniform(-1e-3, 1e-3, 6000), -0.999 + rng.uniform(-1e-9, 1e-9, 1000),
                           1.0 - _log_uniform(rng, 1e-16, 1e-2, 2000), -1.0 + _log_uniform(rng, 1e-16, 1e-3, 2000), tiny, -tiny, edges, -edges, at])


def specials():
    """0, -0, +-inf, NaN and denormals (smallest, mid-range, largest; both signs)."""
    d = [5e-324, 2.0 ** -1060, 2.0 ** -1030, 2.0 ** -1024, 1.5 * 2.0 ** -1023, np.nextafter(2.0 ** -1022, 0)]
    return np.array([0.0, -0.0, np.inf, -np.inf, np.nan] + d + [-v for v in d])


def ulp_error(got, want):
    """|got - want| in units of the spacing of doubles at `want` (finite, normal inputs)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return np.abs(got - want) / np.spacing(np.abs(want))


# ------------------------------------------------------------------------------------------------------------ rotation
SEAM_BELOW = np.array([3.0, 1.0 - 4 * EPS, 0.0])   # |r|^2 rounds to nextafter(10, 0): the last input of the series branch but one
SEAM_AT = np.array([3.0, 1.0, 0.0])                # |r|^2 == 10 exactly: still the series
SEAM_ABOVE = np.array([3.0, 1.0 + 4 * EPS, 0.0])   # |r|^2 rounds to nextafter(10, 11): the first input of the device branch
# (9 + b^2 is one rounding whether or not the compiler contracts it into an FMA)


def rotation_poses():
    """Poses (rvec, tvec) by class of squared angle x = |rvec|^2; returns (poses[n, 6], {class: index array})."""
    rng = np.random.default_rng(105)
    groups, poses = {}, []

    def add(name, rvecs):
        rvecs = np.atleast_2d(np.asarray(rvecs, np.float64))
        groups[name] = np.arange(len(poses), len(poses) + len(rvecs))
        for r in rvecs:
            poses.append(np.concatenate([r, rng.normal(size=3) * 3.0]))

    def at_angles(angles):
        axes = rng.normal(size=(len(angles), 3))
        axes /= np.linalg.norm(axes, axis=1, keepdims=True)
        return axes * np.asarray(angles)[:, None]
    add("identity", np.concatenate([np.zeros((1, 3)), at_angles([1e-17, 1e-20, 2e-16, 1e-300])]))
    add("tiny", at_angles(_log_uniform(rng, 1e-15, 1e-4, 60)))
    add("series", at_angles(np.concatenate([rng.uniform(0.0, np.sqrt(10.0), 300), [1e-3, 1.0, np.pi, 3.1622]])))
    add("seam", np.stack([SEAM_BELOW, SEAM_AT, SEAM_ABOVE, SEAM_BELOW[[2, 0, 1]], SEAM_AT[[2, 0, 1]], SEAM_ABOVE[[2, 0, 1]]]))
    add("device_branch", at_angles(np.concatenate([rng.uniform(np.sqrt(10.0), 2 * np.pi, 200), [3.1624, 3.5, 6.0, 2 * np.pi]])))
    add("beyond", at_angles(rng.uniform(2 * np.pi, 10.0, 100)))
    add("near_pi", at_angles([np.pi - 1e-6, np.pi + 1e-6, np.pi - 1e-7, np.pi + 1e-7, np.pi - 3e-9, np.pi + 3e-9, np.pi] * 4))
    add("nan", np.array([[np.nan, 0.1, 0.2]]))
    return np.array(poses), groups


# ------------------------------------------------------------------------------------------------------------ point terms
def point_term_cases():
    """Cases of PT_N correspondences each (float32-representable coordinates, as the kernels read them).
    Returns (cases[n, PT_IN], {class: index array}):
      random    random poses / points as the host moment test draws them, random on[] masks
      one_off   exactly one correspondence switched off, in every position (= every position of an NP-tuple, NP = 1..4)
      all / none every correspondence on / off
      exact     identity rotation: Zc = Z + t_z is ONE rounding on the host and on the device alike, depths 1e-3 .. 1e3 of both signs
      small_z   identity rotation, Zc = +-1e-6 (to the rounding of Z + t_z)
      zero_z    identity rotation, Zc == 0 exactly for some correspondences (the `Zc ? 1 / Zc : 1` guard)"""
    rng = np.random.default_rng(106)
    f, cx, cy = 525.0, 320.0, 240.0
    groups, cases = {}, []

    def project(pose, obj):
        r = pose[:3]
        th = np.linalg.norm(r)
        Kx = np.array([[0, -r[2], r[1]], [r[2], 0, -r[0]], [-r[1], r[0], 0.0]])
        R = np.eye(3) if th < 1e-12 else np.eye(3) + np.sin(th) / th * Kx + (1 - np.cos(th)) / th ** 2 * Kx @ Kx
        Xc = obj @ R.T + pose[3:]
        z = np.where(Xc[:, 2] == 0, 1.0, Xc[:, 2])
        return np.stack([f * Xc[:, 0] / z + cx, f * Xc[:, 1] / z + cy], 1)

    def add(name, pose, obj, on):
        obj = obj.astype(np.float32).astype(np.float64)
        img = np.clip(project(pose, obj) + rng.normal(0, 1, (PT_N, 2)), -1e6, 1e6).astype(np.float32).astype(np.float64)
        row = np.concatenate([pose, [f, cx, cy], np.concatenate([obj, img, np.asarray(on, np.float64)[:, None]], 1).reshape(-1)])
        groups.setdefault(name, []).append(len(cases))
        cases.append(row)

    def random_points():
        obj = rng.uniform(-2, 2, (PT_N, 3))
        obj[:, 2] += 5
        return obj

    def random_pose():
        return np.concatenate([rng.normal(size=3) * 0.3, rng.uniform(-0.3, 0.3, 3)])
    for _ in range(200):
        add("random", random_pose(), random_points(), rng.uniform(size=PT_N) < 0.7)
    for k in range(PT_N):
        add("one_off", random_pose(), random_points(), np.arange(PT_N) != k)
    add("all", random_pose(), random_points(), np.ones(PT_N))
    add("none", random_pose(), random_points(), np.zeros(PT_N))
    for _ in range(100):
        obj = random_points()
        obj[:, 2] = _log_uniform(rng, 1e-3, 1e3, PT_N) * rng.choice([-1.0, 1.0], PT_N)
        add("exact", np.concatenate([np.zeros(3), rng.uniform(-0.3, 0.3, 2), [0.0]]), obj, rng.uniform(size=PT_N) < 0.8)
    for _ in range(20):
        obj = random_points()
        obj[:, 2] = 5.0 + rng.choice([-1e-6, 1e-6], PT_N)
        add("small_z", np.concatenate([np.zeros(3), rng.uniform(-0.3, 0.3, 2), [-5.0]]), obj, rng.uniform(size=PT_N) < 0.8)
    for k in range(20):
        obj = random_points()
        obj[rng.uniform(size=PT_N) < 0.3, 2] = 4.0
        obj[k % PT_N, 2] = 4.0
        add("zero_z", np.concatenate([np.zeros(3), rng.uniform(-0.3, 0.3, 2), [-4.0]]), obj, rng.uniform(size=PT_N) < 0.8 if k % 2 else np.ones(PT_N))
    return np.array(cases), {k: np.array(v) for k, v in groups.items()}


# ------------------------------------------------------------------------------------------------------------ solves
IU = np.triu_indices(6)


def sym_from_u21(U21):
    A = np.zeros((6, 6))
    A[IU] = U21
    return A + np.triu(A, 1).T


def solve_cases():
    """The systems of the host tests (tests/test_device_math_host.py): damped normal equations of a pose re-fit, full-rank and
    rank-deficient J^T J of the training path -- and a family whose last LDL^T pivot is (1 -+ 1 %) x the threshold of the
    verdict relative to its diagonal entry, for both verdicts (lm_solve6: 1e-12, inv_spd6: 1e-7).
    Returns (cases[n, SOLVE_IN], {class: index array}, {index: pivot / diagonal})."""
    rng = np.random.default_rng(107)
    groups, cases, pivots = {}, [], {}

    def add(name, A, g, lam):
        groups.setdefault(name, []).append(len(cases))
        cases.append(np.concatenate([A[IU], g, [lam]]))
    for trial in range(40):
        J = rng.normal(size=(120, 6)) * np.array([3e3, 3e3, 1e3, 300, 300, 100.0]) * 10.0 ** rng.uniform(-1, 1)
        add("lm", J.T @ J, J.T @ rng.normal(0, 1, 120), [1e-3, 1.0, 1e-6, 100.0][trial % 4])
    for it in range(50):
        J = rng.normal(size=(40, 6)) * np.array([100, 100, 100, 30, 30, 10.0])
        add("full_rank", J.T @ J, rng.normal(size=6), 0.0)
    for trial in range(20):
        J = rng.normal(size=(40, 5)) * 30
        J = np.concatenate([J, J[:, :1] * (1 + (1e-9 if trial % 2 else 0) * rng.normal(size=(40, 1)))], axis=1)
        if trial % 5 == 4:
            J = rng.normal(size=(4, 6)) * 30  # fewer rows than parameters
        add("deficient", J.T @ J, rng.normal(size=6), 0.0)
    for delta in (1.01e-12, 0.99e-12, 1.01e-7, 0.99e-7):
        A = np.eye(6)
        A[4, 5] = A[5, 4] = np.sqrt(1.0 - delta)  # pivot 5 = 1 - A[4, 5]^2 = delta (to 1e-16 absolute: 1e-4 of the 1 % margin)
        pivots[len(cases)] = delta
        add("pivot", A, rng.normal(size=6), 0.0)
    return np.array(cases), {k: np.array(v) for k, v in groups.items()}, pivots


# ------------------------------------------------------------------------------------------------------------ lane-dealt step
# accumulator layout entry -> (moment, sign): lm_moments_to_acc with f = 1
ACC_FROM_MOMENTS = {0: (15, 1), 1: (14, -1), 2: (0, -1), 3: (9, -1), 4: (10, -1), 5: (12, 1), 6: (16, 1), 7: (1, -1), 8: (11, 1), 9: (9, 1),
                    10: (13, -1), 11: (2, 1), 12: (8, -1), 13: (7, 1), 15: (3, 1), 16: (4, -1), 17: (3, 1), 18: (5, -1), 19: (6, 1),
                    20: (17, -1), 21: (18, 1), 22: (19, 1), 23: (20, 1), 24: (21, 1), 25: (22, -1)}


def _moment_sums(rng, n):
    """the 27 totals of a pass over a real point set, so that the normal matrix is SPD with the structure the kernels produce"""
    x, y = rng.normal(size=n) * 0.4, rng.normal(size=n) * 0.3
    iz = 1.0 / rng.uniform(1.0, 6.0, size=n)
    ex, ey = rng.normal(size=n) * 3.0, rng.normal(size=n) * 3.0
    xx, yy, xy = x * x, y * y, x * y
    r2, ox, oy = xx + yy, 1 + xx, 1 + yy
    qq, p1, p2, iz2 = 1 + r2, x * iz, y * iz, iz * iz
    mom = [x, y, r2, iz2, iz2 * x, iz2 * y, iz2 * r2, p1, p2, xy * iz, oy * iz, ox * iz, p2 * qq, p1 * qq, xy * (1 + qq),
           xy * xy + oy * oy, xy * xy + ox * ox, xy * ex + oy * ey, ox * ex + xy * ey, x * ey - y * ex, iz * ex, iz * ey,
           p1 * ex + p2 * ey, ex * ex + ey * ey]
    return np.array([m.sum() for m in mom] + [1.0, 2.0, float(n)])


def lane_step_cases():
    """The 300 (totals, pose, lambda) of test_lane_dealt_lm_step_equals_the_uniform_route, in its order of drawing."""
    rng = np.random.default_rng(33)
    out = []
    for it in range(300):
        sums = _moment_sums(rng, [6, 40, 400][it % 3])
        pose = np.concatenate([rng.normal(size=3) * [1e-9, 0.3, 1.5][it % 3], rng.normal(size=3) * [0.1, 3.0][it % 2]])
        lam = 10.0 ** rng.integers(-6, 3)
        out.append((sums, pose, float(lam)))
    return out


def lane_identity_cases():
    """Poses below the identity cut of lm_pose_rotation (|rvec| < eps): tg.identity is set, M = hot."""
    rng = np.random.default_rng(34)
    out = []
    for it in range(12):
        sums = _moment_sums(rng, [6, 40, 400][it % 3])
        r = np.zeros(3) if it < 2 else rng.normal(size=3) * [1e-17, 1e-20][it % 2]
        out.append((sums, np.concatenate([r, rng.normal(size=3) * [0.1, 3.0][it % 2]]), float(10.0 ** rng.integers(-6, 3))))
    return out


def lane_rank_deficient_case():
    """all points on one viewing ray: a pivot collapses once lambda is tiny, the verdict must be "not ok" """
    sums = np.zeros(27)
    sums[[3, 23]] = [4.0, 1.0]
    return sums, np.array([0.1, 0.2, 0.3, 0.0, 0.0, 1.0]), 1e-16


def lane_reference(sums, Mw, K):
    """The uniform route on the same totals in numpy: (U[6, 6], g[6]) from the chain-rule matrices of the pose."""
    acc = np.zeros(27)
    for a, (m, sg) in ACC_FROM_MOMENTS.items():
        acc[a] = sg * sums[m]
    A6 = np.zeros((6, 6))
    A6[:3, :3] = [[acc[0], acc[1], acc[2]], [acc[1], acc[6], acc[7]], [acc[2], acc[7], acc[11]]]
    A6[:3, 3:] = [[acc[3], acc[4], acc[5]], [acc[8], acc[9], acc[10]], [acc[12], acc[13], acc[14]]]
    A6[3:, :3] = A6[:3, 3:].T
    A6[3:, 3:] = [[acc[15], 0, acc[16]], [0, acc[17], acc[18]], [acc[16], acc[18], acc[19]]]
    M6 = np.block([[Mw, np.zeros((3, 3))], [K, np.eye(3)]])
    return M6.T @ A6 @ M6, M6.T @ acc[20:26]


def second_lambda(lam):
    """the damping of the rejected trial that follows a step at `lam` (CvLevMarq multiplies by 10)"""
    return lam * 10.0


# ------------------------------------------------------------------------------------------------------------ pseudo-inverse step
PINV_THRESH = 2 * 2.220446049250313e-16  # x sum |w|: eigenvalues below are dropped (lm_solve6_pinv, pinv_sym6_jacobi)


def pinv_cases():
    """(name, A[6, 6], g[6], lambda), lambda = 0 and lambda in {1e-3, 1}: normal equations J^T J of integer-valued Jacobians (the products are exact, so the rank
    of the stored matrix IS the rank of the construction): a point and one row of a second (rank 3), two points and points on one viewing ray (rank 4), points
    on a line (rank 5) in the twist parametrisation, and a full-rank system."""
    rng = np.random.default_rng(108)
    out = []

    def twist_rows(x, y, iz):  # the rows of lm_math.hpp's twist Jacobian (f = 1), scaled to integers by the caller's choice of x, y, iz
        return np.array([[-x * y, 1 + x * x, -y, iz, 0, -iz * x], [-(1 + y * y), x * y, x, 0, iz, -iz * y]])

    def system(points, name, lam, rows=None):
        J = np.concatenate([twist_rows(*p) for p in points])[:rows]
        out.append((name, J.T @ J, J.T @ rng.integers(-3, 4, len(J)).astype(np.float64), lam))
    ray = [(1.0, 2.0, z) for z in (1.0, 2.0, 4.0, 8.0)]                                      # one viewing ray, four depths
    two = [(1.0, 2.0, 1.0), (-2.0, 1.0, 2.0)]
    line = [(float(k), 2.0 * k + 1.0, 1.0) for k in range(-3, 4)]                            # a line in a fronto-parallel plane
    full = [(float(rng.integers(-4, 5)), float(rng.integers(-4, 5)), float(rng.integers(1, 5))) for _ in range(12)]
    # undamped (lambda = 0: what a collapsed pivot at a tiny lambda amounts to -- 1 + 1e-16 == 1 in double)
    system(ray, "ray", 0.0)
    system(two, "two_points", 0.0)
    system(two, "point_and_a_row", 0.0, rows=3)                                              # (rank 3: the second point's u row only)
    system(line, "line", 0.0)
    system(full, "full", 0.0)
    # damped: (1 + lambda) on the diagonal CHANGES the stored matrix -- a routine that ignored lambda, or scaled the wrong
    # entries, fails here.  Damping lifts a rank-deficient system to full rank (its null space meets diag(A)).
    for lam in (1e-3, 1.0):
        system(full, "full_damped", lam)
        system(line, "line_damped", lam)
        system(two, "two_points_damped", lam)
    return out


def pinv_reference(A, g, lam):
    """numpy's pseudo-inverse step on the (1 + lambda)-damped matrix with the kernel's threshold; also returns the condition
    number of the kept eigenvalues (two backward-stable routes agree to eps x that) and the rank."""
    Ad = A.copy()
    Ad[np.diag_indices(6)] *= 1.0 + lam
    w, V = np.linalg.eigh(Ad)
    thresh = PINV_THRESH * np.abs(w).sum()
    keep = np.abs(w) > thresh
    dx = (V[:, keep] / w[keep]) @ (V[:, keep].T @ g)
    return dx, np.abs(w[keep]).max() / np.abs(w[keep]).min(), int(keep.sum())
