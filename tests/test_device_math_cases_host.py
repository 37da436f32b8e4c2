"""The HOST side of every routine tests/test_gpu_device_math.py runs on the device: the new entry points of
tests/native/host_math_probe.cpp on the shared cases of tests/device_math_cases.py, against mpmath at 50 digits (or the
oracle where the oracle has the routine), through the checks of tests/device_math_checks.py.  Also: the device probe must
cross-compile for gfx950 (no GPU needed for that), so a header change that breaks it shows here."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import device_math_cases as DC
from tests import device_math_checks as K


@pytest.fixture(scope="module")
def probe():
    from tests.native import build
    return K.bind_host(C.CDLL(build.build()))


@pytest.fixture(scope="module")
def host(probe):
    return K.HostRunner(probe)


# ------------------------------------------------------------------------------------------------------------ the tests
def _show(name):
    return lambda worst: print("\n[%s] %s" % (name, {k: float("%.4g" % v) for k, v in worst.items()}))


def test_host_scalars_against_high_precision(host):
    """fast_rcp (host: 1.0 / d, bit-equal), scr_sqrt, cbrt_pos, cos_third_acos of the host build on the shared inputs; the two
    measured worst errors are the figures the device bars are derived from."""
    K.check_scalar_bars(host, report=_show("host scalars"))
    d = DC.rcp_inputs()
    assert (host.scalars("lane_rcp_neg", d) == -1.0 / d).all()


def test_host_scalars_at_special_values(host):
    """what the device build is compared with at 0, +-inf, NaN and denormals (tests/test_gpu_device_math.py)"""
    v = DC.specials()
    with np.errstate(all="ignore"):
        np.testing.assert_array_equal(host.scalars("fast_rcp", v), 1.0 / v)
        np.testing.assert_array_equal(host.scalars("scr_sqrt", v), np.sqrt(v))
    assert host.scalars("cbrt_pos", np.array([0.0]))[0] == 0.0 and host.scalars("cbrt_pos", np.array([np.inf]))[0] == np.inf
    pos = v[(v > 0) & np.isfinite(v)]
    got = host.scalars("cbrt_pos", pos)  # denormals: the pow fallback
    np.testing.assert_allclose(got, [float(K.mpmath.power(K.mpmath.mpf(float(a)), K.mpmath.mpf(1.0 / 3.0))) for a in pos], rtol=4 * DC.EPS)
    assert np.isnan(host.scalars("cos_third_acos", np.array([np.nan, 2.0, -2.0, np.inf]))[[0, 2]]).all()


def test_host_rotation_routines(host, oracle):
    """lm_pose_rotation (R, A, B, identity), lm_pose_left_jacobian, lm_pose_chain against 50 digits; rodrigues_vec2mat<true> /
    rodrigues_mat2vec against the oracle -- all classes of squared angle, the seam at |rvec|^2 = 10, angles next to pi."""
    K.check_rotation(host, oracle, report=_show("host rotation"))


@pytest.mark.parametrize("np_", [1, 2, 3, 4])
def test_host_point_terms(host, probe, np_):
    """lm_point_terms<NP> on its own and through the moment route, NP = 1..4 (the team kernel's cells per lane)"""
    K.check_point_terms(host, host, probe, np_, report=_show("host point terms NP=%d" % np_))


def test_host_solves(host, oracle):
    K.check_solves(host, oracle)


def test_lane_cases_are_what_the_gpu_test_expects(probe):
    """the identity poses are identity poses; the rank-deficient totals give verdict 0 on the host emulation"""
    poses = np.array([c[1] for c in DC.lane_identity_cases()])
    assert (K.HostRunner(probe).rotation(poses)[:, 11] == 1).all()
    sums, pose, lam = DC.lane_rank_deficient_case()
    U, g, dx = np.zeros(21), np.zeros(6), np.zeros(6)
    assert probe.probe_lane_step(K._p(sums), K._p(pose), lam, K._p(U), K._p(g), K._p(dx)) == 0


def test_pinv_cases_have_a_decided_rank_and_the_host_route_agrees_with_numpy(host, probe):
    """No eigenvalue of a pseudo-inverse test system within a factor 10 of the threshold (the arithmetic, not the rank, is
    compared), every rank from 3 to 6 present, systems whose damping changes the stored matrix present, and the host's Jacobi route against
    numpy (conditioned): the measured agreement is the
    figure the device bar is derived from."""
    K.mpmath.mp.dps = 50
    ranks, worst, damped = set(), 0.0, 0
    for name, A, g, lam in K.pinv_systems(probe):
        dx, cond, rank = DC.pinv_reference(A, g, lam)
        Ad = A.copy()
        Ad[np.diag_indices(6)] *= 1.0 + lam
        w = [abs(float(v)) for v in K.mpmath.eigsy(K.mpmath.matrix(Ad.tolist()), eigvals_only=True)]  # of the stored matrix, 50 digits
        thresh = DC.PINV_THRESH * sum(w)
        assert all(v > 10 * thresh or v < thresh / 10 for v in w), (name, w, thresh)
        assert sum(v > thresh for v in w) == rank, (name, w)
        ranks.add(rank)
        got = K.pinv_host_step(host, A, g, lam)
        worst = max(worst, K.pinv_disagreement(got, dx, cond))
        damped += bool((Ad != A).any())
    print("\n[host pinv vs numpy] %.4g" % worst)
    assert ranks >= {3, 4, 5, 6}, ranks
    assert damped >= 6  # systems whose lambda changes the stored matrix
    assert worst <= K.HOST_PINV_AGREEMENT, worst


def test_device_math_probe_cross_compiles():
    """device_math_probe.hip includes the product's headers unchanged and builds with the product's flags for gfx950"""
    from tests.native import build
    lib = build.build_device_math_probe(force=True)
    assert os.path.getsize(lib) > 0
    with open(lib, "rb") as fh:
        blob = fh.read()
    for kernel in (b"k_scalars", b"k_rotation", b"k_point_terms", b"k_solves", b"k_lane_step", b"k_pinv_step"):
        assert kernel in blob, kernel
    assert b"gfx950" in blob
