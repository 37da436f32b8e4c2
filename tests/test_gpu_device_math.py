"""The device-only branches of the math headers, function by function, ON THE GPU.

Every `#if defined(__HIP_DEVICE_COMPILE__)` branch of pose_math.hpp / lm_math.hpp / lm_lanes.hpp / p3p_screen.hpp, and the
device-only lm_solve6_pinv of refine_common.hpp, is text the host build of the CPU suite never compiles and the whole-call
GPU tests reach only at the inputs a synthetic frame happens to produce.  tests/native/device_math_probe.hip compiles the
product's headers unchanged with the product's flags; here each routine runs on the shared cases of
tests/device_math_cases.py and is held to the reference and bar of its host test (tests/device_math_checks.py, tests/test_device_math_cases_host.py,
tests/test_device_math_host.py), or to a measured figure written down with its margin ("Precision contract")."""
import ctypes as C

import numpy as np
import pytest

from tests import device_math_cases as DC
from tests import device_math_checks as H

pytestmark = pytest.mark.gpu


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


class DeviceRunner(H.HostRunner):
    """the device probe behind the interface of the host probe: every call is one kernel launch; a HIP error fails the test"""

    def __init__(self, lib):
        super().__init__(lib)
        vp, i = C.c_void_p, C.c_int
        lib.dev_scalars.argtypes = [i, i, vp, vp]
        lib.dev_point_terms.argtypes = [i, i, vp, vp]
        for name in ("dev_rotation", "dev_solves", "dev_lane_step", "dev_pinv_step"):
            getattr(lib, name).argtypes = [i, vp, vp]
        self.pinv_threads = lib.dev_pinv_threads()

    def _run(self, fn, args, rows, width):
        out = np.empty((rows, width))
        status = fn(*args, _p(out))
        assert status == 0, "HIP error %d" % status
        return out

    def scalars(self, name, v):
        v = np.ascontiguousarray(v, np.float64)
        assert len(v) <= 2 ** 16
        return self._run(self.lib.dev_scalars, (DC.OPS[name], len(v), _p(v)), len(v), 1)[:, 0]

    def rotation(self, poses):
        poses = np.ascontiguousarray(poses, np.float64)
        return self._run(self.lib.dev_rotation, (len(poses), _p(poses)), len(poses), DC.ROT_OUT)

    def point_terms(self, np_, cases):
        cases = np.ascontiguousarray(cases, np.float64)
        return self._run(self.lib.dev_point_terms, (np_, len(cases), _p(cases)), len(cases), DC.PT_OUT)

    def solves(self, cases):
        cases = np.ascontiguousarray(cases, np.float64)
        return self._run(self.lib.dev_solves, (len(cases), _p(cases)), len(cases), DC.SOLVE_OUT)

    def lane_step(self, cases):
        cases = np.ascontiguousarray(cases, np.float64)
        return self._run(self.lib.dev_lane_step, (len(cases), _p(cases)), len(cases) * 64, DC.LANE_OUT).reshape(len(cases), 64, DC.LANE_OUT)

    def pinv_step(self, cases):
        cases = np.ascontiguousarray(cases, np.float64)
        return self._run(self.lib.dev_pinv_step, (len(cases), _p(cases)), len(cases) * self.pinv_threads, 6).reshape(len(cases), self.pinv_threads, 6)


@pytest.fixture(scope="module")
def host_lib():
    from tests.native import build
    return H.bind_host(C.CDLL(build.build()))


@pytest.fixture(scope="module")
def host(host_lib):
    return H.HostRunner(host_lib)


@pytest.fixture(scope="module")
def dev(engine):
    from tests.native import build
    return DeviceRunner(C.CDLL(build.build_device_math_probe()))


def _show(name):
    return lambda worst: print("\n[%s] %s" % (name, {k: float("%.4g" % v) for k, v in worst.items()}))


def _same_bits(a, b):
    return np.ascontiguousarray(a, np.float64).view(np.uint64) == np.ascontiguousarray(b, np.float64).view(np.uint64)


# ------------------------------------------------------------------------------------------------------------ scalars
def test_device_scalars_fast_rcp_scr_sqrt_cbrt_pos_cos_third_acos(dev):
    """fast_rcp (v_rcp_f64 + two Newton steps) within 1 ulp of the correctly rounded 1.0 / d; scr_sqrt (v_rsq_f64 + Newton +
    one correction) within 1 ulp of np.sqrt, 0 -> 0, negative / NaN -> NaN; cbrt_pos (frexp builtins, fp32 seed) and
    cos_third_acos (__cosf seed) within the host build's measured worst error against 50 digits plus one ulp: the device
    differs from the host in its reciprocal (at most 1 ulp) and in a seed that Newton forgets.
    Measured on an MI355X: fast_rcp 0 ulp (equal to the quotient on all 58 196 inputs), scr_sqrt 0 ulp, cbrt_pos 0.79 ulp
    (bar 1.936), cos_third_acos 3.62 ulp (bar 6.89)."""
    H.check_scalar_bars(dev, rcp_ulp=1.0, cbrt_ulp=H.HOST_CBRT_ULP + 1.0, cos3_ulp=H.HOST_COS3_ULP + 1.0, sqrt_of_minus_zero=0.0, report=_show("device scalars"))


LANE_RCP_NEG_WORST_ULP = 0.0  # lm_lanes.hpp: "correctly rounded": bit-equal to -1.0 / p


def test_device_lane_rcp_neg_is_what_its_comment_says(dev):
    """lane_rcp_neg (lm_lanes.hpp, the device row: v_rcp_f64, x0 (1 + e + e^2)) against the correctly rounded -1.0 / p: the
    header's claim, held exactly"""
    p = DC.rcp_inputs()
    got, want = dev.scalars("lane_rcp_neg", p), -1.0 / p
    err = DC.ulp_error(got, want)
    print("\n[device lane_rcp_neg] worst %.4g ulp, %d of %d inputs not bit-equal" % (err.max(), int((got != want).sum()), len(p)))
    assert err.max() <= LANE_RCP_NEG_WORST_ULP, (err.max(), p[np.argmax(err)])


# Host / device differences at special values, each justified from the call sites in the routine's header comment
# (pose_math.hpp:fast_rcp, lm_lanes.hpp:lane_rcp_neg, p3p_screen.hpp:scr_rcp / scr_sqrt / cbrt_pos).  {routine: {input: what the
# device returns}}: NaN, a value (bit for bit), or ("ulp", n) / ("rel", r): within n ulp / a relative r of the host's result.
# Every other special input must give the host's result bit for bit (NaN == NaN).
# (keys are repr() of the input: 0.0 and -0.0 are one dict key as floats)
_OVERFLOWING = [0.0, -0.0, np.inf, -np.inf] + [s * d for s in (1.0, -1.0) for d in (5e-324, 2.0 ** -1060, 2.0 ** -1030, 2.0 ** -1024)]
SPECIAL_DIFFERENCES = {
    "fast_rcp": {repr(float(v)): np.nan for v in _OVERFLOWING},      # 0 * inf in the Newton step where the quotient is +-inf / +-0
    "lane_rcp_neg": {repr(float(v)): np.nan for v in _OVERFLOWING},
    "scr_sqrt": {repr(-0.0): 0.0, repr(float(np.inf)): np.nan, repr(5e-324): ("rel", 0.26),
                 repr(1.5 * 2.0 ** -1023): ("ulp", 1)},  # (0.5 * d loses bits of a denormal)
    "cbrt_pos": {repr(2.0 ** -1024): ("ulp", 1)},  # the pow fallback: the device library's pow and the host's
    "cos_third_acos": {},
}


def test_device_scalars_at_special_values_equal_the_host_build(dev, host):
    """0, -0, +-inf, NaN and denormals through every scalar routine on the device and on the host: bit-equal, or one of the
    differences the routine's header comment justifies from its call sites (pinned here: the comment must stay true)"""
    v = DC.specials()
    for name in ("fast_rcp", "lane_rcp_neg", "scr_sqrt", "cbrt_pos", "cos_third_acos"):
        got, want = dev.scalars(name, v), host.scalars(name, v)
        same = _same_bits(got, want) | (np.isnan(got) & np.isnan(want))
        print("\n[device specials] %s: (input, device, host) %s" % (name, [(float(a), float(g), float(w)) for a, g, w in zip(v[~same], got[~same], want[~same])]))
        known = SPECIAL_DIFFERENCES[name]
        for a, g, w in zip(v[~same], got[~same], want[~same]):
            assert repr(float(a)) in known, (name, a, g, w)  # an undocumented difference
            k = known[repr(float(a))]
            if isinstance(k, tuple):
                assert abs(g - w) <= (k[1] * np.spacing(abs(w)) if k[0] == "ulp" else k[1] * abs(w)), (name, a, g, w)
            else:
                assert (np.isnan(k) and np.isnan(g)) or _same_bits(np.array([k]), np.array([g]))[0], (name, a, g, w)
        # a documented NaN / value must still be what the device returns: the header comments say so
        for a, k in known.items():
            if not isinstance(k, tuple):
                g = got[[repr(float(x)) == a for x in v]][0]
                assert (np.isnan(k) and np.isnan(g)) or _same_bits(np.array([k]), np.array([g]))[0], (name, a, g)


# ------------------------------------------------------------------------------------------------------------ rotation
def test_device_rotation_lm_pose_rotation_left_jacobian_chain_rodrigues(dev, oracle):
    """lm_pose_rotation on both sides of x = 10 (beyond it: v_rsq_f64 + two Newton steps + the device library's sincos),
    lm_pose_left_jacobian (fast_rcp in C), lm_pose_chain, rodrigues_vec2mat<true>, rodrigues_mat2vec: the host tests' bars,
    the seam within twice the bar, a NaN pose stays NaN"""
    H.check_rotation(dev, oracle, report=_show("device rotation"))


# ------------------------------------------------------------------------------------------------------------ point terms
@pytest.mark.parametrize("np_", [1, 2, 3, 4])
def test_device_lm_point_terms(dev, host, host_lib, np_):
    """lm_point_terms<NP> (the interleaved Newton reciprocal of Zc, the `Zc ? iz : 1` guard behind it, the asm 0/1 weights)
    and the moment route behind it: iz within 1 ulp of the host's quotient, Zc == 0 as the host's guard, switched-off
    correspondences gone in every position, (U21, g6, e2) to the bar of the host's moment test"""
    H.check_point_terms(dev, host, host_lib, np_, report=_show("device point terms NP=%d" % np_))


# ------------------------------------------------------------------------------------------------------------ solves
def test_device_lm_solve6_inv_spd6_pinv_sym6_jacobi(dev, oracle):
    """the host tests' systems and bars (lm_solve6: fast_rcp on its six pivots), and the pivot 1 % either side of each verdict"""
    H.check_solves(dev, oracle)


# ------------------------------------------------------------------------------------------------------------ lane-dealt step
def test_device_lane_dealt_lm_step(dev, host_lib):
    """lm_lanes.hpp's device row -- lane_bc (row_newbcast), lane_rcp_neg, lane_gt_lanes6 (ballot), the inline-assembly blocks
    lane_zrow / lane_urow / lane_trow / lane_gj_step with their hand-managed s_nop padding -- in one wavefront set up as
    team_step's: (a) every value bit-identical in all 64 lanes, (b) system and step against numpy within the host test's
    bars (the system of the rank-deficient totals too), (c) verdict false on the rank-deficient totals, (d) a second solve
    behind a data-dependent uniform branch equals an independent solve at its lambda -- numpy's within the bar, and BIT FOR
    BIT a third, straight-line solve of the same wavefront -- and leaves c untouched: lm_lane_to_u21 before and after it hold
    the same bits, (e) lm_lane_to_u21 is the upper triangle of (b)."""
    regular = DC.lane_step_cases() + DC.lane_identity_cases()
    cases = regular + [DC.lane_rank_deficient_case()]
    rows = np.array([np.concatenate([s, p, [lam, DC.second_lambda(lam)]]) for s, p, lam in cases])
    out = dev.lane_step(rows)
    # (a) uniform
    bits = out.view(np.uint64)
    assert (bits == bits[:, :1, :]).all(), np.argwhere(bits != bits[:, :1, :])[:8]
    o = out[:, 0, :]
    U, g, dx1, dx2, dx3, ok1, ok2, ok3 = o[:, 0:21], o[:, 21:27], o[:, 27:33], o[:, 33:39], o[:, 39:45], o[:, 45], o[:, 46], o[:, 47]
    # (d) c untouched by the solve behind the branch; that solve == the straight-line one, verdicts included (NaN == NaN: the
    # step of the rank-deficient case may be anything, but the same anything)
    assert _same_bits(o[:, 0:27], o[:, 48:75]).all(), np.argwhere(~_same_bits(o[:, 0:27], o[:, 48:75]))[:8]
    assert _same_bits(dx2, dx3).all() and (ok2 == ok3).all(), np.argwhere(~_same_bits(dx2, dx3))[:8]
    worst_sys = worst_dx1 = worst_dx2 = 0.0
    host_equal = 0
    for k, (sums, pose, lam) in enumerate(cases):
        R, Mw, K = np.zeros(9), np.zeros(9), np.zeros(9)
        host_lib.probe_pose_chain(_p(np.ascontiguousarray(pose)), _p(R), _p(Mw), _p(K))
        Uref, gref = DC.lane_reference(sums, Mw.reshape(3, 3), K.reshape(3, 3))
        # (b), (e): the system lm_lane_to_u21 hands out is the upper triangle of the reference
        worst_sys = max(worst_sys, np.abs(U[k] - Uref[DC.IU]).max() / np.abs(Uref).max())
        if k == len(regular):  # the rank-deficient totals: no residual, g is exactly zero; (c) both verdicts false
            assert (gref == 0).all() and (g[k] == 0).all()
            assert ok1[k] == 0 and ok2[k] == 0
            continue
        worst_sys = max(worst_sys, np.abs(g[k] - gref).max() / np.abs(gref).max())
        assert ok1[k] == 1 and ok2[k] == 1, k
        for lam_k, dx, which in ((lam, dx1[k], 1), (DC.second_lambda(lam), dx2[k], 2)):
            Ad = Uref.copy()
            Ad[np.diag_indices(6)] *= 1 + lam_k
            ref = np.linalg.solve(Ad, gref)
            err = np.abs(dx - ref).max() / np.abs(ref).max() / max(1.0, np.linalg.cond(Ad) * 1e-9)
            if which == 1:
                worst_dx1 = max(worst_dx1, err)
            else:
                worst_dx2 = max(worst_dx2, err)  # (d)
        hU, hg, hdx = np.zeros(21), np.zeros(6), np.zeros(6)
        host_lib.probe_lane_step(_p(sums), _p(np.ascontiguousarray(pose)), lam, _p(hU), _p(hg), _p(hdx))
        host_equal += bool(_same_bits(hU, U[k]).all() and _same_bits(hg, g[k]).all() and _same_bits(hdx, dx1[k]).all())
    print("\n[device lane step] system %.3g, step %.3g, second step %.3g; bit-equal to the host emulation in %d of %d cases"
          % (worst_sys, worst_dx1, worst_dx2, host_equal, len(regular)))  # (reported, not asserted)
    assert worst_sys < 1e-13, worst_sys
    assert worst_dx1 < 1e-8 and worst_dx2 < 1e-8, (worst_dx1, worst_dx2)


# ------------------------------------------------------------------------------------------------------------ pseudo-inverse step
def test_device_lm_solve6_pinv(dev, host, host_lib):
    """lm_solve6_pinv (refine_common.hpp: one lane runs the Jacobi sweeps in LDS between barriers, every lane reads the step)
    in a workgroup of the refinement kernels' size: every thread holds the same step, and it agrees with the host's
    pinv_sym6_jacobi route and with numpy's thresholded pseudo-inverse within twice the host's own agreement with numpy (relative to the
    conditioning of the kept eigenvalues); lambda = 1e-3 and 1 change the stored matrix, so the damping itself is checked"""
    systems = H.pinv_systems(host_lib)
    rows = np.array([np.concatenate([A[DC.IU], g, [lam]]) for _, A, g, lam in systems])
    out = dev.pinv_step(rows)
    bits = out.view(np.uint64)
    assert (bits == bits[:, :1, :]).all()
    worst_host = worst_numpy = 0.0
    for k, (name, A, g, lam) in enumerate(systems):
        ref, cond, _ = DC.pinv_reference(A, g, lam)
        href = H.pinv_host_step(host, A, g, lam)
        worst_numpy = max(worst_numpy, H.pinv_disagreement(out[k, 0], ref, cond))
        worst_host = max(worst_host, H.pinv_disagreement(out[k, 0], href, cond))
    print("\n[device pinv step] against numpy %.3g, against the host route %.3g" % (worst_numpy, worst_host))
    assert worst_numpy <= 2 * H.HOST_PINV_AGREEMENT and worst_host <= 2 * H.HOST_PINV_AGREEMENT, (worst_numpy, worst_host)
