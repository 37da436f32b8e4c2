"""CPU checks of the strict-reference mode (ESAC_FLAG_STRICT_REFERENCE): the Horn / Jacobi alignment of pose_math.hpp compiled for
the host (tests/native/strict_probe.cpp) against the oracle -- bit for bit, both are host builds of the same operations with the
same libm -- and against NumPy's eigen-solver; the flag's surface in the header, the ctypes layer and the module, without a GPU."""
import ctypes as C
import importlib.util
import os
import re
import types

import numpy as np
import pytest
import torch

from esac_amd import api
from esac_amd import synthetic as S
from tests.native import build_strict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FX = FY = 525.0
CX, CY = 320.0, 240.0


@pytest.fixture(scope="module")
def strict():
    lib = C.CDLL(build_strict.build())
    vp, d = C.c_void_p, C.c_double
    lib.probe_p3p_strict.argtypes = [vp, vp, d, d, d, d, vp, vp, vp]
    lib.probe_p3p_strict.restype = C.c_int
    lib.probe_align_horn.argtypes = [vp, vp, vp, vp]
    lib.probe_align_horn.restype = None
    return lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _p3p_strict(lib, obj, img):
    obj, img = np.ascontiguousarray(obj, np.float64), np.ascontiguousarray(img, np.float64)
    r, t, R = np.zeros(3), np.zeros(3), np.zeros(9)
    ok = lib.probe_p3p_strict(_p(obj), _p(img), FX, FY, CX, CY, _p(r), _p(t), _p(R))
    return bool(ok), r, t


def _minimal_set(coords, e, cells, sub=8):
    obj = np.array([[coords[e, c, y, x] for c in range(3)] for x, y in cells], np.float64)
    img = np.array([[x * sub + sub // 2, y * sub + sub // 2] for x, y in cells], np.float64)
    return obj, img


def _reproj(obj, img, r, t):
    th = np.linalg.norm(r)
    K = np.array([[0, -r[2], r[1]], [r[2], 0, -r[0]], [-r[1], r[0], 0]]) / th
    R = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)
    P = obj @ R.T + t
    return np.hypot(FX * P[:, 0] / P[:, 2] + CX - img[:, 0], FY * P[:, 1] / P[:, 2] + CY - img[:, 1])


def test_pinned_sliver_gets_the_oracles_decision(oracle, strict):
    """The minimal set of tests/test_device_math_host.py::test_ill_conditioned_minimal_set_is_a_known_divergence (oracle: accepted at
    6.5 px, the triad / Newton alignment: rejected at 10.55 px): with the Horn alignment the device math solves it, all four
    reprojection errors stay below tau = 10 px, and the pose is the oracle's."""
    f = S.make_frame(5874, E=12, true_expert=874 % 12)
    obj, img = _minimal_set(f["coords"], 7, [(57, 47), (58, 48), (56, 48), (56, 47)])
    ok_o, r_o, t_o = oracle.p3p(obj, img, FX, FY, CX, CY)
    ok_s, r_s, t_s = _p3p_strict(strict, obj, img)
    assert ok_o and ok_s
    assert _reproj(obj, img, r_s, t_s).max() < 10.0
    np.testing.assert_array_equal(r_s, r_o)
    np.testing.assert_array_equal(t_s, t_o)


def test_strict_p3p_is_the_oracles_on_sampled_minimal_sets(oracle, strict):
    """The 512 minimal sets of test_p3p_matches_oracle_on_sampled_minimal_sets (good expert and garbage experts): ok, rvec and tvec
    equal the oracle's bit for bit."""
    f = S.make_frame(100, E=10, true_expert=0)
    ha = S.gating_assignment(f, 512, mode="gating")
    ref = oracle.forward(f["coords"], ha)
    for h in range(512):
        obj, img = _minimal_set(f["coords"], ha[h], ref["sample_xy"][h])
        ok_o, r_o, t_o = oracle.p3p(obj, img, FX, FY, CX, CY)
        ok_s, r_s, t_s = _p3p_strict(strict, obj, img)
        assert ok_s == ok_o, h
        np.testing.assert_array_equal(r_s, r_o, err_msg=str(h))
        np.testing.assert_array_equal(t_s, t_o, err_msg=str(h))


def _planar_maps():
    spec = importlib.util.spec_from_file_location("screen_adversarial", os.path.join(ROOT, "scripts", "dev", "screen_adversarial.py"))
    A = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(A)
    maps = A.adversarial_maps()
    return np.stack([maps["plane warped 3x0.33 tilted"], maps["plane warped 2x0.5"]])  # the planar frame's two wrong experts


def test_strict_p3p_is_the_oracles_on_the_planar_adversarial_maps(oracle, strict):
    """2800 tries on the two planar maps of the adversarial set: 2000 drawn as the sampler draws them, 800 built on purpose with the
    three base points in ONE image row (on an exactly planar map: collinear in space -- the alignment's optimum is a one-parameter
    family and the eigen-solve picks the member).  Bit equality with the oracle in ok, rvec and tvec."""
    m = _planar_maps()
    rng = np.random.default_rng(5)
    n_ok = n_collinear_ok = 0
    for k in range(2800):
        if k < 2000:
            cells = [(int(x), int(y)) for x, y in oracle.draw_cells(77, 3, k // 8, k % 8, 80, 60)]
        else:
            y = int(rng.integers(0, 59))
            xs = rng.choice(79, size=3, replace=False)
            cells = [(int(x), y) for x in xs] + [(int(rng.integers(0, 79)), int((y + 1 + rng.integers(0, 57)) % 59))]
        obj, img = _minimal_set(m, k % 2, cells)
        ok_o, r_o, t_o = oracle.p3p(obj, img, FX, FY, CX, CY)
        ok_s, r_s, t_s = _p3p_strict(strict, obj, img)
        assert ok_s == ok_o, (k, cells)
        np.testing.assert_array_equal(r_s, r_o, err_msg=str((k, cells)))
        np.testing.assert_array_equal(t_s, t_o, err_msg=str((k, cells)))
        n_ok += ok_o
        n_collinear_ok += ok_o and k >= 2000
    assert n_ok >= 100 and n_collinear_ok >= 10, (n_ok, n_collinear_ok)  # the comparison is not one of failed solves only


def _horn_matrix(P, Q):
    """The symmetric 4x4 of Horn's method for R P_k + T = Q_k (the oracle's construction: cross-covariance of the centred points)."""
    s = (P - P.mean(0)).T @ (Q - Q.mean(0)) / 3
    return np.array([[s[0, 0] + s[1, 1] + s[2, 2], s[1, 2] - s[2, 1], s[2, 0] - s[0, 2], s[0, 1] - s[1, 0]],
                     [s[1, 2] - s[2, 1], s[0, 0] - s[1, 1] - s[2, 2], s[1, 0] + s[0, 1], s[2, 0] + s[0, 2]],
                     [s[2, 0] - s[0, 2], s[1, 0] + s[0, 1], s[1, 1] - s[2, 2] - s[0, 0], s[2, 1] + s[1, 2]],
                     [s[0, 1] - s[1, 0], s[2, 0] + s[0, 2], s[2, 1] + s[1, 2], s[2, 2] - s[0, 0] - s[1, 1]]])


def test_align_horn_against_numpy_eigh(strict):
    """Random congruent and perturbed triangles: the rotation of align_horn is the one of the eigenvector NumPy finds for the largest
    eigenvalue of the same 4x4 (within 1e-12), proper (det +1), and T maps the centroids."""
    rng = np.random.default_rng(21)
    for k in range(400):
        P = rng.uniform(-2, 2, size=(3, 3))
        w = rng.normal(size=3)
        th = np.linalg.norm(w)
        K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]]) / th
        R0 = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)
        Q = P @ R0.T + rng.uniform(-3, 3, size=3)
        if k % 2:
            Q = Q + rng.normal(scale=0.05, size=(3, 3))  # not congruent: the least-squares optimum
        R, T = np.zeros(9), np.zeros(3)
        strict.probe_align_horn(_p(np.ascontiguousarray(P)), _p(np.ascontiguousarray(Q)), _p(R), _p(T))
        R = R.reshape(3, 3)
        w_eig, V = np.linalg.eigh(_horn_matrix(P, Q))
        q = V[:, np.argmax(w_eig)]
        Rn = np.array([[q[0]**2 + q[1]**2 - q[2]**2 - q[3]**2, 2 * (q[1] * q[2] - q[0] * q[3]), 2 * (q[1] * q[3] + q[0] * q[2])],
                       [2 * (q[1] * q[2] + q[0] * q[3]), q[0]**2 + q[2]**2 - q[1]**2 - q[3]**2, 2 * (q[2] * q[3] - q[0] * q[1])],
                       [2 * (q[1] * q[3] - q[0] * q[2]), 2 * (q[2] * q[3] + q[0] * q[1]), q[0]**2 + q[3]**2 - q[1]**2 - q[2]**2]])
        assert np.abs(R - Rn).max() < 1e-12, (k, np.abs(R - Rn).max())
        assert abs(np.linalg.det(R) - 1.0) < 1e-12
        np.testing.assert_allclose(R @ P.mean(0) + T, Q.mean(0), rtol=0, atol=1e-12)


# ---------------------------------------------------------------- the flag's surface
def test_flag_value_in_header_and_api_agree():
    with open(os.path.join(ROOT, "include", "esac_hip.h")) as fh:
        text = fh.read()
    m = re.search(r"#define ESAC_FLAG_STRICT_REFERENCE (\d+)", text)
    assert m and int(m.group(1)) == api.FLAG_STRICT_REFERENCE == 256
    others = [int(v) for v in re.findall(r"#define ESAC_FLAG_(?!STRICT_REFERENCE)\w+ (\d+)", text)]
    assert others and all(256 & v == 0 for v in others)  # a bit of its own
    assert api.ABI_VERSION == 6 and "#define ESAC_HIP_ABI_VERSION 6" in text  # additive: no new symbol, no changed record
    assert C.sizeof(api.Params) == 104


def _make_params(**kw):
    return api.Engine.make_params(types.SimpleNamespace(), 1, 60, 80, 64, **kw)  # (the method touches no device)


def test_make_params_strict_implies_the_two_exact_routes():
    assert _make_params().flags == 0
    assert _make_params(strict_reference=True).flags == 256 | 16 | 1
    assert _make_params(strict_reference=True, exact_scores=True, exact_sampling=True).flags == 256 | 16 | 1
    assert _make_params(strict_reference=True, refine_solo=True).flags == 256 | 128 | 16 | 1
    assert _make_params(strict_reference=False, exact_sampling=True).flags == 16


@pytest.mark.parametrize("kw", [dict(score_shape="tiled"), dict(score_shape="stream"), dict(exact_scores="auto")])
def test_make_params_rejects_strict_with_a_ranking_route(kw):
    with pytest.raises(ValueError, match="strict_reference"):
        _make_params(strict_reference=True, **kw)
    _make_params(**kw)  # fine without the flag


def test_module_switch_is_exported_and_training_refuses_it():
    """esac.set_strict_reference beside the other switches; backward / backward_batch raise ValueError while it is on -- before an
    engine exists, before a call counter is spent."""
    import esac
    assert esac.set_strict_reference is api.set_strict_reference
    sc = torch.zeros(1, 3, 12, 16)
    bwd = [sc, torch.zeros_like(sc), torch.zeros(8, dtype=torch.int64), torch.eye(4), 1.0, 100.0, 100.0, 0, 0, 525.0, 320.0, 240.0,
           10.0, 100.0, 0.5, 100.0, 8]
    scb = torch.zeros(2, 1, 3, 12, 16)
    bwd_b = [scb, torch.zeros_like(scb), torch.zeros(2, 8, dtype=torch.int64), torch.eye(4).repeat(2, 1, 1), 1.0, 100.0, 100.0, 0, 0,
             525.0, 320.0, 240.0, 10.0, 100.0, 0.5, 100.0, 8]
    engines, call = dict(api._state["engines"]), api._state["call"]
    assert api._state["strict_reference"] is False
    esac.set_strict_reference(True)
    try:
        with pytest.raises(ValueError, match="no strict mode"):
            esac.backward(*bwd)
        with pytest.raises(ValueError, match="no strict mode"):
            esac.backward_batch(*bwd_b)
    finally:
        esac.set_strict_reference(False)
    assert api._state["engines"] == engines and api._state["call"] == call
    assert api._state["strict_reference"] is False


def test_harness_and_sharded_forward_know_the_flag():
    import inspect
    from esac_amd import distributed, harness
    assert inspect.signature(harness.localize).parameters["strict_reference"].default is False
    assert inspect.signature(api.Engine.make_params).parameters["strict_reference"].default is False
    with pytest.raises(ValueError, match="no strict mode"):
        distributed.forward_sharded_once(None, torch.zeros(1, 3, 12, 16), torch.zeros(8, dtype=torch.int64), dict(strict_reference=True))
