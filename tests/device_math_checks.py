"""Runners, references, bars and checks that the CPU suite (tests/test_device_math_cases_host.py: the host build of the math
headers) and the GPU suite (tests/test_gpu_device_math.py: the device build) share.  Not a test module: mpmath is a plain
import here, so a machine without it fails loudly instead of skipping the per-function tests."""
import ctypes as C

import mpmath
import numpy as np

from tests import device_math_cases as DC

# Worst error of the host build of the two Newton-polished routines against mpmath (50 digits), in ulp of the exact value,
# measured by tests/test_device_math_cases_host.py on the shared cases and rounded up (LAB_NOTES.md, "Per-function device tests"):
#   cbrt_pos        0.936   (inside (1e-300, 1e300); outside it the routine IS pow(a, 1.0 / 3.0) and is held to that function,
#                            whose exponent is the double next to 1/3: 100 ulp from the cube root at 1e-300, by design)
#   cos_third_acos  5.89    (5.889 at c = -0.9989, next to the switch to the library route at -0.999, where the cubic's root is
#                            ill-conditioned: u = 1/2 is a double root at c = -1; 1.78 on [-0.99, -0.9), below 1 for c > -0.9;
#                            the library route below -0.999: 2.21)
# The device bars of tests/test_gpu_device_math.py are these plus one ulp.
HOST_CBRT_ULP = 0.936
HOST_COS3_ULP = 5.89


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def bind_host(lib):
    vp, i = C.c_void_p, C.c_int
    lib.probe_scalars.argtypes = [i, i, vp, vp]
    lib.probe_rotation.argtypes = [i, vp, vp]
    lib.probe_point_terms.argtypes = [i, i, vp, vp]
    lib.probe_solves.argtypes = [i, vp, vp]
    lib.probe_lm_normal.argtypes = [vp, vp, i, vp] + [C.c_double] * 4 + [vp, vp, vp]
    lib.probe_lane_step.argtypes = [vp, vp, C.c_double, vp, vp, vp]
    lib.probe_pose_chain.argtypes = [vp, vp, vp, vp]
    return lib


class HostRunner:
    """the host probe behind the interface the checks below share with the device probe"""

    def __init__(self, lib):
        self.lib = lib

    def scalars(self, name, v):
        v = np.ascontiguousarray(v, np.float64)
        out = np.empty_like(v)
        self.lib.probe_scalars(DC.OPS[name], len(v), _p(v), _p(out))
        return out

    def rotation(self, poses):
        poses = np.ascontiguousarray(poses, np.float64)
        out = np.empty((len(poses), DC.ROT_OUT))
        self.lib.probe_rotation(len(poses), _p(poses), _p(out))
        return out

    def point_terms(self, np_, cases):
        cases = np.ascontiguousarray(cases, np.float64)
        out = np.empty((len(cases), DC.PT_OUT))
        assert self.lib.probe_point_terms(np_, len(cases), _p(cases), _p(out)) == 0
        return out

    def solves(self, cases):
        cases = np.ascontiguousarray(cases, np.float64)
        out = np.empty((len(cases), DC.SOLVE_OUT))
        self.lib.probe_solves(len(cases), _p(cases), _p(out))
        return out


# ------------------------------------------------------------------------------------------------------------ references
_REF_CACHE = {}


def mp_ulp_errors(got, exact):
    """|got - exact| / ulp(exact) for mpmath `exact` values"""
    out = np.empty(len(got))
    for k, (g, e) in enumerate(zip(got, exact)):
        out[k] = float(abs(mpmath.mpf(float(g)) - e) / mpmath.mpf(float(np.spacing(abs(float(e))))))
    return out


def cbrt_exact():
    if "cbrt" not in _REF_CACHE:
        mpmath.mp.dps = 50
        v = DC.cbrt_inputs()
        third = mpmath.mpf(1.0 / 3.0)  # the exponent the fallback passes to pow
        _REF_CACHE["cbrt"] = (v, [mpmath.cbrt(mpmath.mpf(float(a))) if 1e-300 < a < 1e300 else mpmath.power(mpmath.mpf(float(a)), third) for a in v])
    return _REF_CACHE["cbrt"]


def cos3_exact():
    if "cos3" not in _REF_CACHE:
        mpmath.mp.dps = 50
        v = DC.cos3_inputs()
        _REF_CACHE["cos3"] = (v, [mpmath.cos(mpmath.acos(mpmath.mpf(float(c))) / 3) for c in v])
    return _REF_CACHE["cos3"]


def rotation_exact(poses):
    """(R, A, B, left Jacobian, K = [t]x J_l) of each finite pose at 50 digits, rounded to double"""
    key = ("rot", poses.tobytes())
    if key not in _REF_CACHE:
        mpmath.mp.dps = 50
        out = np.full((len(poses), 29), np.nan)
        for n, pose in enumerate(poses):
            if not np.all(np.isfinite(pose)):
                continue
            r = [mpmath.mpf(float(v)) for v in pose[:3]]
            t = [mpmath.mpf(float(v)) for v in pose[3:]]
            x = r[0] * r[0] + r[1] * r[1] + r[2] * r[2]
            if x < mpmath.mpf(10) ** -30:  # (1 - cos would cancel at 50 digits; the next terms of the series are below 1e-60)
                A, B, Cc = 1 - x / 6, mpmath.mpf(0.5) - x / 24, mpmath.mpf(1) / 6 - x / 120
            else:
                th = mpmath.sqrt(x)
                A, B, Cc = mpmath.sin(th) / th, (1 - mpmath.cos(th)) / x, (th - mpmath.sin(th)) / (th * x)
            S = mpmath.matrix([[0, -r[2], r[1]], [r[2], 0, -r[0]], [-r[1], r[0], 0]])
            T = mpmath.matrix([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
            Rr = mpmath.eye(3) + A * S + B * (S * S)
            Jl = mpmath.eye(3) + B * S + Cc * (S * S)
            Kk = T * Jl
            out[n] = [float(Rr[i, j]) for i in range(3) for j in range(3)] + [float(A), float(B)] + \
                     [float(Jl[i, j]) for i in range(3) for j in range(3)] + [float(Kk[i, j]) for i in range(3) for j in range(3)]
        _REF_CACHE[key] = out
    return _REF_CACHE[key]


# ------------------------------------------------------------------------------------------------------------ checks shared with the GPU suite
R_BAR = 3e-15      # lm_pose_rotation / lm_pose_left_jacobian against 50 digits: the bar of test_pose_rotation_series_against_high_precision
CHAIN_BAR = 1e-13  # Mw, K of lm_pose_chain: the bar of probe_chain_diff (K relative to 1 + |K|)


def check_scalar_bars(run, rcp_ulp=0.0, cbrt_ulp=HOST_CBRT_ULP, cos3_ulp=HOST_COS3_ULP, sqrt_of_minus_zero=-0.0, report=None):
    """fast_rcp within `rcp_ulp` of 1.0 / d, scr_sqrt within 1 ulp of np.sqrt (0 -> 0, negative / NaN -> NaN), cbrt_pos and
    cos_third_acos within their bars of the 50-digit value.  Returns the measured worst errors."""
    worst = {}
    d = DC.rcp_inputs()
    worst["fast_rcp"] = DC.ulp_error(run.scalars("fast_rcp", d), 1.0 / d).max()
    s = DC.sqrt_inputs()
    worst["scr_sqrt"] = DC.ulp_error(run.scalars("scr_sqrt", s), np.sqrt(s)).max()
    edge = run.scalars("scr_sqrt", np.array([0.0, -0.0, -1.0, -1e-300, -np.inf, np.nan]))
    v, exact = cbrt_exact()
    worst["cbrt_pos"] = mp_ulp_errors(run.scalars("cbrt_pos", v), exact).max()
    c, exact = cos3_exact()
    err = mp_ulp_errors(run.scalars("cos_third_acos", c), exact)
    worst["cos_third_acos"] = err.max()
    if report is not None:
        report(worst)
    assert worst["fast_rcp"] <= rcp_ulp, worst
    assert worst["scr_sqrt"] <= 1.0, worst
    assert edge[0] == 0.0 and not np.signbit(edge[0]) and np.isnan(edge[2:]).all(), edge
    # sqrt(-0.0): the library's -0.0 in the host build, +0.0 from the device branch (p3p_screen.hpp says so)
    assert edge[1] == 0.0 and np.signbit(edge[1]) == np.signbit(sqrt_of_minus_zero), edge
    assert worst["cbrt_pos"] <= cbrt_ulp, worst
    assert worst["cos_third_acos"] <= cos3_ulp, worst
    return worst


def check_rotation(run, oracle, report=None):
    poses, G = DC.rotation_poses()
    out = run.rotation(poses)
    ref = rotation_exact(poses)
    fin = np.array([k for k in range(len(poses)) if k not in set(G["nan"])])
    R, A, B, ident, x = out[:, 0:9], out[:, 9], out[:, 10], out[:, 11], out[:, 12]
    Mw, Rc, Mwc, Kc, Rr, Jr, rv = out[:, 13:22], out[:, 22:31], out[:, 31:40], out[:, 40:49], out[:, 49:58], out[:, 58:85], out[:, 85:88]
    # the classes are what they claim to be
    assert (ident[G["identity"]] == 1).all() and (ident[np.setdiff1d(fin, G["identity"])] == 0).all()
    assert (x[G["series"]] <= 10).all() and (x[G["tiny"]] < 1e-7).all() and (x[G["device_branch"]] > 10).all() and (x[G["beyond"]] > 39.4).all()
    assert list(x[G["seam"]]) == [np.nextafter(10.0, 0), 10.0, np.nextafter(10.0, 11)] * 2
    # a NaN pose stays NaN
    assert np.isnan(out[G["nan"], 0:11]).all() and np.isnan(out[G["nan"], 13:85]).all()
    worst = {"R": np.abs(R[fin] - ref[fin, 0:9]).max(), "AB": max(np.abs(A[fin] - ref[fin, 9]).max(), np.abs(B[fin] - ref[fin, 10]).max()),
             "Jl": np.abs(Mw[fin] - ref[fin, 11:20]).max(), "chain_R": np.abs(Rc[fin] - ref[fin, 0:9]).max(),
             "chain_Mw": np.abs(Mwc[fin] - ref[fin, 11:20]).max(),
             "chain_K": (np.abs(Kc[fin] - ref[fin, 20:29]) / (1 + np.abs(ref[fin, 20:29]))).max()}
    # the seam: x = 10 - ulp runs the series, x = 10 + ulp the trigonometric route; the exact values differ by ~1e-16
    sb, sa = G["seam"][[0, 3]], G["seam"][[2, 5]]
    worst["seam"] = max(np.abs(out[sb, 0:11] - out[sa, 0:11]).max(), np.abs(out[sb, 13:22] - out[sa, 13:22]).max())
    # Rodrigues and its inverse against the oracle (the inverse on the very matrix this build produced)
    wR = wJ = wv = 0.0
    for k in fin:
        Ro, Jo = oracle.rodrigues_vec2mat(poses[k, :3], jac=True)
        wR, wJ = max(wR, np.abs(Rr[k].reshape(3, 3) - Ro).max()), max(wJ, np.abs(Jr[k].reshape(3, 9) - Jo).max())
        wv = max(wv, np.abs(rv[k] - oracle.rodrigues_mat2vec(Rr[k].reshape(3, 3))).max())
    worst.update(rodrigues_R=wR, rodrigues_J=wJ, mat2vec=wv)
    if report is not None:
        report(worst)
    assert worst["R"] < R_BAR and worst["AB"] < R_BAR and worst["Jl"] < R_BAR and worst["chain_R"] < R_BAR, worst
    assert worst["chain_Mw"] < CHAIN_BAR and worst["chain_K"] < CHAIN_BAR, worst
    assert worst["seam"] < 2 * R_BAR, worst
    assert worst["rodrigues_R"] <= 1e-15 and worst["rodrigues_J"] <= 1e-14 and worst["mat2vec"] <= 1e-15, worst
    return worst


def lm_normal_reference(lib, case):
    """(U21, g6, e2) of the correspondences of a case that are switched on, through the entry-by-entry route of the host build
    (lm_accumulate_point + lm_chain(dR/drvec) + lm_transform): the fp64 reference of test_device_math_host.py's moment test"""
    pts = case[9:].reshape(DC.PT_N, 6)
    on = pts[:, 5] != 0
    obj, img = np.ascontiguousarray(pts[on, 0:3], np.float32), np.ascontiguousarray(pts[on, 3:5], np.float32)
    U, g, e2 = np.zeros(21), np.zeros(6), np.zeros(1)
    pose = np.ascontiguousarray(case[:6])
    lib.probe_lm_normal(_p(obj), _p(img), int(on.sum()), _p(pose), case[6], case[6], case[7], case[8], _p(U), _p(g), _p(e2))
    return U, g, e2[0]


def check_point_terms(run, host_run, lib, np_, report=None):
    """lm_point_terms<np_> + the moment route of one build (`run`) against the host build (`host_run`: the `Zc ? 1 / Zc : 1` side)
    and the entry-by-entry fp64 reference"""
    cases, G = DC.point_term_cases()
    out, ref = run.point_terms(np_, cases), host_run.point_terms(np_, cases)
    terms, rterms = out[:, :6 * DC.PT_N].reshape(len(cases), DC.PT_N, 6), ref[:, :6 * DC.PT_N].reshape(len(cases), DC.PT_N, 6)
    pts = cases[:, 9:].reshape(len(cases), DC.PT_N, 6)
    on = pts[:, :, 5] != 0
    # switched-off correspondences vanish, whatever their position in the tuple; w is the mask
    assert (terms[:, :, 5] == on).all()
    assert (terms[~on] == 0).all()
    worst = {}
    # iz: the Newton reciprocal against the host's division where both builds hold the same Zc bit for bit (identity rotation)
    ex = np.concatenate([G["exact"], G["small_z"]])
    m = on[ex]
    worst["iz_ulp"] = DC.ulp_error(terms[ex][m][:, 2], rterms[ex][m][:, 2]).max()
    zc = pts[ex][m][:, 2] + cases[ex, 5][:, None].repeat(DC.PT_N, 1)[m]
    assert (rterms[ex][m][:, 2] == 1.0 / zc).all()  # (the host's value is the correctly rounded quotient)
    # Zc == 0 exactly: iz = 1, x = Xc, y = Yc, as the host's guard
    z = G["zero_z"]
    zero = on[z] & (pts[z][:, :, 2] == 4.0)
    assert zero.sum() >= len(z)
    assert (terms[z][zero][:, 2] == 1.0).all()
    np.testing.assert_array_equal(terms[z][zero][:, [0, 1, 2, 5]], rterms[z][zero][:, [0, 1, 2, 5]])
    # (ex, ey = (x f + c) - m: one rounding where the compiler contracts x f + c into an FMA, two where it does not)
    for col, c0 in ((3, cases[0, 7]), (4, cases[0, 8])):
        xy = terms[z][zero][:, col - 3]
        assert (np.abs(terms[z][zero][:, col] - rterms[z][zero][:, col]) <= 2 * DC.EPS * (np.abs(xy) * cases[0, 6] + c0)).all()
    # elsewhere Zc differs between two builds by the rounding of a four-term sum and of R (each within R_BAR of the truth):
    # |d iz| <= ulp + (4 eps sum|terms| + 2 R_BAR (|X| + |Y| + |Z|)) / Zc^2
    rnd = np.concatenate([G["random"], G["one_off"], G["all"]])
    m = on[rnd]
    mag = np.abs(pts[rnd][:, :, 0:3]).sum(2)[m]
    iz_ref = rterms[rnd][m][:, 2]
    tol = np.spacing(np.abs(iz_ref)) + (4 * DC.EPS * (mag + 0.3) + 2 * R_BAR * mag) * iz_ref ** 2
    worst["iz_random_of_tol"] = (np.abs(terms[rnd][m][:, 2] - iz_ref) / tol).max()
    assert worst["iz_random_of_tol"] <= 1.0, worst
    # (U21, g6, e2): the bar of the host's moment test, against the entry-by-entry reference; where Zc == 0 occurs that route
    # differs by design (it keeps Zc * iz = 0 where the moment route takes 1): the host's moment route is the reference there
    wU = wg = we = 0.0
    for k in range(len(cases)):
        U, g, e2 = out[k, 72:93], out[k, 93:99], out[k, 99]
        if k in set(G["zero_z"]) or not on[k].any():
            U1, g1, e1 = ref[k, 72:93], ref[k, 93:99], ref[k, 99]
        else:
            U1, g1, e1 = lm_normal_reference(lib, cases[k])
        sU, sg = max(np.abs(U1).max(), 1e-300), max(np.abs(g1).max(), 1e-300)
        wU, wg = max(wU, np.abs(U - U1).max() / sU), max(wg, np.abs(g - g1).max() / sg)
        we = max(we, abs(e2 - e1) / max(e1, 1e-300))
    worst.update(U=wU, g=wg, e2=we)
    if report is not None:
        report(worst)
    assert worst["iz_ulp"] <= 1.0, worst
    assert worst["U"] <= 1e-11 and worst["g"] <= 1e-11 and worst["e2"] <= 1e-12, worst
    return worst


def check_solves(run, oracle, report=None):
    cases, G, pivots = DC.solve_cases()
    out = run.solves(cases)
    dx, ok_lm, Ainv, ok_inv, Pinv = out[:, 0:6], out[:, 6], out[:, 7:43].reshape(-1, 6, 6), out[:, 43], out[:, 44:80].reshape(-1, 6, 6)
    for k in G["lm"]:  # damped solve == numpy (the host test's bar)
        A = DC.sym_from_u21(cases[k, :21])
        A[np.diag_indices(6)] *= 1 + cases[k, 27]
        assert ok_lm[k] == 1
        np.testing.assert_allclose(dx[k], np.linalg.solve(A, cases[k, 21:27]), rtol=1e-8, atol=1e-12)
    for k in G["full_rank"]:
        assert ok_inv[k] == 1
        np.testing.assert_allclose(Ainv[k], oracle.pinv_sym6(DC.sym_from_u21(cases[k, :21])), rtol=1e-8, atol=1e-14)
    for k in G["deficient"]:
        assert ok_inv[k] == 0
        ref = oracle.pinv_sym6(DC.sym_from_u21(cases[k, :21]))
        np.testing.assert_allclose(Pinv[k], ref, rtol=1e-9, atol=1e-12 * np.abs(ref).max())
    for k in G["pivot"]:  # the last pivot 1 % above / below the threshold of either verdict
        assert ok_lm[k] == (1 if pivots[k] > 1e-12 else 0), (pivots[k], ok_lm[k])
        assert ok_inv[k] == (1 if pivots[k] > 1e-7 else 0), (pivots[k], ok_inv[k])
        if ok_inv[k]:
            A = DC.sym_from_u21(cases[k, :21])
            np.testing.assert_allclose(dx[k], np.linalg.solve(A, cases[k, 21:27]), rtol=1e-8, atol=1e-12)
    k = G["full_rank"][0]  # on a well-conditioned matrix the pseudo-inverse is simply the inverse
    np.testing.assert_allclose(Pinv[k] @ DC.sym_from_u21(cases[k, :21]), np.eye(6), atol=1e-10)


def pinv_host_step(run, A, g, lam):
    """the host's pinv_sym6_jacobi route on the (1 + lambda)-damped matrix"""
    Ad = A.copy()
    Ad[np.diag_indices(6)] *= 1.0 + lam
    out = run.solves(np.concatenate([Ad[DC.IU], g, [0.0]])[None])
    return out[0, 44:80].reshape(6, 6) @ g


def pinv_systems(lib):
    """tests/device_math_cases.py:pinv_cases plus the rank-deficient system of the lane-dealt test (the host emulation's U21, g6)
    at that test's lambda = 1e-16 -- a bitwise no-op as damping (1 + 1e-16 == 1): it is there as the system the kernel meets"""
    sums, pose, lam = DC.lane_rank_deficient_case()
    U, g, dx = np.zeros(21), np.zeros(6), np.zeros(6)
    lib.probe_lane_step(_p(sums), _p(pose), lam, _p(U), _p(g), _p(dx))
    return DC.pinv_cases() + [("lane_rank_deficient", DC.sym_from_u21(U), g, lam)]


# Agreement of the host's Jacobi route with numpy's eigh-based pseudo-inverse step on pinv_systems: largest difference of
# the step relative to its largest entry, DIVIDED BY the condition number of the kept eigenvalues (the damped rank-deficient
# systems reach 9e3; two backward-stable routes agree to eps x that), measured by
# test_pinv_cases_have_a_decided_rank_... (tests/test_device_math_cases_host.py) and rounded up: 1.54e-16 -> 1.6e-16 (on the
# system of two points at lambda = 1e-3; unscaled: 1.39e-12 there, <= 1.9e-14 on every other system).  The device bar is
# twice that (the same algorithm in another operation order, a sqrt that may differ by 1 ulp per rotation).
HOST_PINV_AGREEMENT = 1.6e-16


def pinv_disagreement(got, ref, cond):
    return np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-300) / cond  # (g = 0 in the lane-dealt system: the step is exactly 0)
