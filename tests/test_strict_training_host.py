"""CPU checks of the training path's strict mode (ESAC_FLAG_STRICT_TRAINING): the flag's surface in the header, the ctypes layer,
the module and the harness, and the two routines the flag adds to the gradient kernel -- path II's dPNP over the Horn alignment and
path I's always-on Jacobi pseudo-inverse -- compiled for the host (tests/native/strict_training_probe.cpp) against the oracle, bit
for bit: both sides are host builds of the same operations in the same order with the same libm."""
import ctypes as C
import inspect
import os
import re
import types

import numpy as np
import pytest
import torch

from esac_amd import api
from esac_amd import synthetic as S
from tests.native import build_strict_training

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the frames of tests/test_gpu_strict_training.py::test_strict_parity_on_the_backward_frames: (frame kwargs, N, mode, alpha, call)
PARITY_FRAMES = [(dict(k=0), 256, "single", 100.0, 0), (dict(k=1), 64, "single", 100.0, 1), (dict(k=2), 256, "single", 100.0, 2),
                 (dict(k=3), 64, "single", 100.0, 3), (dict(k=10), 128, "single", 2.0, 0), (dict(k=21), 64, "single", 5.0, 5),
                 (dict(k=31, E=3, true_expert=1), 96, "gating", 10.0, 2),
                 (dict(k=41, H=45, W=61, sub=10, shift=(7, -5)), 64, "single", 20.0, 1),
                 (dict(k=105, H=100, W=120, sub=4), 24, "single", 3.0, 4)]


@pytest.fixture(scope="module")
def probe():
    lib = C.CDLL(build_strict_training.build())
    vp, d = C.c_void_p, C.c_double
    lib.probe_dpnp_strict.argtypes = [vp, vp, d, d, d, d, vp]
    lib.probe_dpnp_strict.restype = C.c_int
    lib.probe_pinv_rolled.argtypes = [vp, vp]
    lib.probe_pinv_rolled.restype = None
    return lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _oracle_dpnp(oracle, obj32, img, f):
    """dpnp_p3p of the oracle (oracle/esac_oracle_bwd.inc) restated on top of its exported 4-point solver: the in-place float
    perturbation (+eps, -2 eps, +eps), 18 solves, (f - b) / (double)(2 eps); zeros when a solve fails or an entry is NaN."""
    eps = np.float32(0.001)
    obj = obj32.astype(np.float32).copy()
    J = np.zeros((6, 12))
    for q in range(9):
        obj[q] = obj[q] + eps
        ok_f, rf, tf = oracle.p3p(obj.astype(np.float64).reshape(4, 3), img, f["focal"], f["focal"], f["ppx"], f["ppy"])
        obj[q] = obj[q] - np.float32(2) * eps
        ok_b, rb, tb = oracle.p3p(obj.astype(np.float64).reshape(4, 3), img, f["focal"], f["focal"], f["ppx"], f["ppy"])
        obj[q] = obj[q] + eps
        if not (ok_f and ok_b):
            return False, np.zeros((6, 12))
        J[:, q] = (np.concatenate([rf, tf]) - np.concatenate([rb, tb])) / float(np.float32(2) * eps)
        if np.isnan(J[:, q]).any():
            return False, np.zeros((6, 12))
    return True, J


def _minimal_set(f, e, cells):
    sx, sy = f["shift"]
    obj = np.array([[f["coords"][e, c, y, x] for c in range(3)] for x, y in cells], np.float32).reshape(12)
    img = np.array([[x * f["sub"] + f["sub"] // 2 - sx, y * f["sub"] + f["sub"] // 2 - sy] for x, y in cells], np.float64)
    return obj, img


def _frames():
    for kw, N, mode, alpha, call in PARITY_FRAMES:
        kw = dict(kw)
        f = S.make_frame(kw.pop("k"), **kw)
        yield f, S.gating_assignment(f, N, mode=mode), alpha, call


def test_dpnp_over_the_horn_alignment_is_the_oracles(oracle, probe):
    """Every hypothesis of the parity frames (selected or not: 1112 minimal sets, good and garbage) and the pinned sliver: the 6 x 12
    matrix of 18 perturbed Horn solves, the float perturbation residue included, equals the oracle's bit for bit."""
    n = kept = 0
    sets = []
    for f, ha, alpha, call in _frames():
        ref = oracle.forward(f["coords"], ha, shift_x=f["shift"][0], shift_y=f["shift"][1], focal=f["focal"], ppx=f["ppx"],
                             ppy=f["ppy"], sub_sampling=f["sub"], inlier_alpha=alpha, seed=1305, call=call)
        sets += [(f, int(ha[h]), [tuple(c) for c in ref["sample_xy"][h]]) for h in range(len(ha))]
    fs = S.make_frame(5874, E=12, true_expert=874 % 12)
    sets.append((fs, 7, [(57, 47), (58, 48), (56, 48), (56, 47)]))
    for f, e, cells in sets:
        obj, img = _minimal_set(f, e, cells)
        ok_o, J_o = _oracle_dpnp(oracle, obj, img, f)
        J = np.zeros((6, 12))
        ok = probe.probe_dpnp_strict(_p(obj), _p(np.ascontiguousarray(img)), f["focal"], f["focal"], f["ppx"], f["ppy"], _p(J))
        assert bool(ok) == ok_o, (n, cells)
        np.testing.assert_array_equal(J, J_o, err_msg=str((n, cells)))
        n += 1
        kept += ok_o
    assert n >= 1000 and kept >= 500, (n, kept)  # not a comparison of failed solves only


def _normal_matrix(oracle, f, e, pose, inlier_map):
    ys, xs = np.nonzero(inlier_map)
    A = np.zeros((6, 6))
    for y, x in zip(ys, xs):
        px, py = x * f["sub"] + f["sub"] // 2 - f["shift"][0], y * f["sub"] + f["sub"] // 2 - f["shift"][1]
        ok, row = oracle.norm_jac_row(pose[:3], pose[3:], f["focal"], f["ppx"], f["ppy"], [float(v) for v in f["coords"][e, :, y, x]],
                                      (float(px), float(py)), 100.0)
        A += np.outer(row, row)
    return A


def test_always_on_pseudo_inverse_is_the_oracles(oracle, probe):
    """pinv_sym6_rolled -- what the strict kernel runs on EVERY slot -- against the oracle's (J^T J).inv(DECOMP_SVD): normal
    matrices of refined slots of the parity frames (up to 4 slots a frame, the refinement run by the oracle), random full-rank
    ones, rank-deficient and badly scaled ones.  Bit equality."""
    iu = np.triu_indices(6)
    mats = []
    for f, ha, alpha, call in _frames():
        if f["coords"].shape[2] > 60:
            continue  # (12000 cells through ctypes one by one: the smaller grids say the same)
        kw = dict(shift_x=f["shift"][0], shift_y=f["shift"][1], focal=f["focal"], ppx=f["ppx"], ppy=f["ppy"], sub_sampling=f["sub"],
                  inlier_alpha=alpha, seed=1305, call=call)
        ref = oracle.forward(f["coords"], ha, **kw)
        for h in np.nonzero(ref["probs"] >= 1e-3)[0][:4]:
            one = oracle.forward(f["coords"], ha[h:h + 1], in_hyps=ref["hyps"][h:h + 1], **kw)
            if one["ref_steps"] > 0:
                mats.append(_normal_matrix(oracle, f, int(ha[h]), one["refined"], one["inlier_map"]))
    assert len(mats) >= 16
    rng = np.random.default_rng(7)
    for k in range(200):
        Jm = rng.normal(size=(40, 6)) * 10.0 ** rng.integers(-3, 4, size=6)
        if k % 4 == 1:
            Jm[:, 5] = Jm[:, 0] * 2 - Jm[:, 1]  # rank 5
        if k % 4 == 2:
            Jm = Jm[:3]  # rank 3
        mats.append(Jm.T @ Jm)
    mats.append(np.zeros((6, 6)))
    for k, A in enumerate(mats):
        A = (A + A.T) / 2
        out = np.zeros((6, 6))
        probe.probe_pinv_rolled(_p(np.ascontiguousarray(A[iu])), _p(out))
        np.testing.assert_array_equal(out, oracle.pinv_sym6(A), err_msg=str(k))


# ---------------------------------------------------------------- the flag's surface
def test_flag_value_in_header_and_api_agree():
    with open(os.path.join(ROOT, "include", "esac_hip.h")) as fh:
        text = fh.read()
    m = re.search(r"#define ESAC_FLAG_STRICT_TRAINING (\d+)", text)
    assert m and int(m.group(1)) == api.FLAG_STRICT_TRAINING == 512
    others = [int(v) for v in re.findall(r"#define ESAC_FLAG_(?!STRICT_TRAINING)\w+ (\d+)", text)]
    assert others and all(512 & v == 0 for v in others)  # a bit of its own
    assert api.ABI_VERSION == 6 and "#define ESAC_HIP_ABI_VERSION 6" in text  # additive: no new symbol, no changed record
    assert C.sizeof(api.Params) == 104
    with open(os.path.join(ROOT, "esac_amd", "csrc", "esac_kernels.hpp")) as fh:
        assert "ESAC_FLAG_STRICT_TRAINING_K = 512" in fh.read()


def _make_params(**kw):
    return api.Engine.make_params(types.SimpleNamespace(), 1, 60, 80, 64, **kw)  # (the method touches no device)


def test_make_params_flag_words_and_rejections():
    assert _make_params().flags == 0
    assert _make_params(strict_training=True).flags == 512 | 16 | 1
    assert _make_params(strict_training=True, exact_scores=True, exact_sampling=True).flags == 512 | 16 | 1
    assert _make_params(strict_reference=True).flags == 256 | 16 | 1  # unchanged
    for kw in (dict(strict_reference=True), dict(exact_scores="auto"), dict(score_shape="tiled"), dict(score_shape="stream")):
        with pytest.raises(ValueError, match="strict_training"):
            _make_params(strict_training=True, **kw)
        _make_params(**kw)  # fine without the flag


def test_module_switch_is_exported_and_forward_ignores_it(monkeypatch):
    """esac.set_strict_training beside the other switches; esac.forward hands the library the flag word it hands it today."""
    import esac
    assert esac.set_strict_training is api.set_strict_training
    assert api._state["strict_training"] is False
    seen = []

    class FakeEngine:
        device = torch.device("cpu")
        make_params = api.Engine.make_params

        def forward_device(self, sc, ha, p, scores_out=None):
            seen.append((p.flags, p.seed, p.call, p.E, p.H, p.W, p.N, p.max_tries, p.max_ref_steps))
            res = np.zeros(api.RES_DOUBLES)
            return res

    monkeypatch.setattr(api, "engine", lambda dev=None: FakeEngine())
    monkeypatch.setitem(api._state, "fwd_cache", {})
    monkeypatch.setattr(torch, "empty", lambda *a, **k: torch.zeros(*a, **{x: y for x, y in k.items() if x not in ("device", "pin_memory")}))
    sc, ha = torch.zeros(1, 3, 12, 16), torch.zeros(8, dtype=torch.int64)
    args = (0, 0, 525.0, 320.0, 240.0, 10.0, 100.0, 0.5, 100.0, 8)
    call = api._state["call"]
    try:
        class Dev:
            def __enter__(self): return self
            def __exit__(self, *a): return False
        monkeypatch.setattr(torch.cuda, "device", lambda d: Dev())
        esac.forward(sc, ha, torch.zeros(4, 4), *args)
        api._state["call"] = call
        esac.set_strict_training(True)
        esac.forward(sc, ha, torch.zeros(4, 4), *args)
    finally:
        esac.set_strict_training(False)
        api._state["call"] = call
    assert len(seen) == 2 and seen[0] == seen[1] and seen[0][0] & 512 == 0


def test_harness_knows_the_switch():
    from esac_amd import harness
    assert inspect.signature(harness.train_step).parameters["strict_training"].default is False
    assert inspect.signature(harness.train_batch).parameters["strict_training"].default is False
    assert inspect.signature(api.Engine.make_params).parameters["strict_training"].default is False
