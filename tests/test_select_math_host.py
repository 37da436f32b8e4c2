"""The selection arithmetic (esac_amd/csrc/select_math.hpp: the exact score of a hypothesis, the softMax / entropy statistics, draw's
argmax rule), compiled for the HOST by tests/native/build.py and checked on the CPU; and the guards that keep each piece defined
once -- every route of the selection calls these functions, which is what makes the routes agree bit for bit."""
import ctypes as C
import glob
import math
import os

import numpy as np
import pytest

from esac_amd import synthetic as S

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "esac_amd", "csrc")
TAU, ALPHA, BETA, MAX_REPROJ = 10.0, 100.0, 0.5, 100.0
NONE = 0x7FFFFFFF


@pytest.fixture(scope="module")
def probe():
    from tests.native import build
    lib = C.CDLL(build.build())
    d, f, i, vp = C.c_double, C.c_float, C.c_int, C.c_void_p
    lib.probe_rodrigues.argtypes = [vp, vp, vp]
    lib.probe_exact_err.argtypes = [vp, vp, d, d, d, d, f, f, f, f, f]
    lib.probe_exact_err.restype = f
    lib.probe_exact_cell_term.argtypes = [i, vp, vp, d, d, d, d, f, f, f, f, f, f, f, f]
    lib.probe_exact_cell_term.restype = d
    lib.probe_exact_score_scaled.argtypes = [d, f, i, i]
    lib.probe_exact_score_scaled.restype = d
    lib.probe_soft_inlier_exact.argtypes = [f, f, f]
    lib.probe_soft_inlier_exact.restype = d
    lib.probe_best_take.argtypes = [vp, vp, vp, d, i, i]
    lib.probe_softmax_stats.argtypes = [vp, i, d, vp]
    lib.probe_softmax_stats_inline.argtypes = [vp, i, d, vp]
    return lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _bits(x):
    return np.asarray(x, np.float64).view(np.uint64)


def test_the_exact_score_is_the_oracles_bit_for_bit(oracle, probe):
    """6x8 cells, one expert, eight hypotheses: exact_cell_term<false> summed in the oracle's own cell order (x outer, y inner,
    esac_util.h:242-251) and scaled by exact_score_scaled is the oracle's score, every bit of it.  (The kernels sum the same
    terms in another order, which the GPU suite holds to 1e-10.)"""
    H, W, sub, N = 6, 8, 80, 8
    f = S.make_frame(3, H=H, W=W, sub=sub)
    ha = S.gating_assignment(f, N)
    ref = oracle.forward(f["coords"], ha, sub_sampling=sub, inlier_thresh=TAU, inlier_alpha=ALPHA, inlier_beta=BETA, max_reproj=MAX_REPROJ)
    cam = (f["focal"], f["focal"], f["ppx"], f["ppy"])
    X, Y, Z = f["coords"][0]
    clamped = 0
    for h in range(N):
        pose = np.ascontiguousarray(ref["hyps"][h])
        R, J, t = np.zeros(9), np.zeros(27), np.ascontiguousarray(pose[3:])
        probe.probe_rodrigues(_p(pose), _p(R), _p(J))
        total = 0.0
        for x in range(W):
            for y in range(H):
                cell = (X[y, x], Y[y, x], Z[y, x], float(x * sub + sub // 2), float(y * sub + sub // 2))
                clamped += probe.probe_exact_err(_p(R), _p(t), *cam, *cell) > MAX_REPROJ
                total += probe.probe_exact_cell_term(0, _p(R), _p(t), *cam, *cell, MAX_REPROJ, TAU, BETA)
        score = probe.probe_exact_score_scaled(total, ALPHA, W, H)
        assert _bits(score) == _bits(ref["scores"][h]), (h, score, ref["scores"][h])
    assert clamped > 0  # (the map holds cells beyond maxReproj: the clamp took part)


def test_a_nan_coordinate_is_an_outlier_unless_strict(probe):
    R, t = np.eye(3).ravel().copy(), np.array([0.1, -0.2, 0.3])
    cam = (525.0, 525.0, 320.0, 240.0)
    for cell in ((math.nan, 0.5, 2.0), (0.2, math.nan, 2.0), (0.2, 0.5, math.nan)):
        term = probe.probe_exact_cell_term(0, _p(R), _p(t), *cam, *cell, 300.0, 200.0, MAX_REPROJ, TAU, BETA)
        assert _bits(term) == _bits(probe.probe_soft_inlier_exact(MAX_REPROJ, TAU, BETA))
        assert math.isnan(probe.probe_exact_cell_term(1, _p(R), _p(t), *cam, *cell, 300.0, 200.0, MAX_REPROJ, TAU, BETA))
    # a finite cell: the two orders of the clamp agree, below and beyond maxReproj
    for cell in ((0.2, 0.5, 2.0), (30.0, 0.5, 2.0)):
        a = probe.probe_exact_cell_term(0, _p(R), _p(t), *cam, *cell, 300.0, 200.0, MAX_REPROJ, TAU, BETA)
        b = probe.probe_exact_cell_term(1, _p(R), _p(t), *cam, *cell, 300.0, 200.0, MAX_REPROJ, TAU, BETA)
        assert _bits(a) == _bits(b)


@pytest.mark.parametrize("incumbent, challenger, taken", [
    ((1.0, 4, 40), (2.0, 9, 90), True),                 # a higher score wins
    ((1.0, 4, 40), (1.0, 9, 30), True),                 # an equal score with a lower global index wins
    ((1.0, 4, 40), (1.0, 2, 50), False),                # an equal score with a higher global index does not
    ((1.0, 4, 40), (1.0, 2, 40), False),
    ((1.0, 4, 40), (0.5, 2, 10), False),
    ((1.0, 4, 40), (math.nan, 2, 10), False),           # a NaN challenger never wins
    ((-math.inf, NONE, NONE), (math.nan, 2, 10), False),
    ((-math.inf, NONE, NONE), (-1e300, 7, 70), True),   # "none" loses to any finite score
    ((-math.inf, NONE, NONE), (0.0, 0, 0), True),
])
def test_best_take_is_draws_rule(probe, incumbent, challenger, taken):
    bs, bi, bg = np.array([incumbent[0]]), np.array([incumbent[1]], np.int32), np.array([incumbent[2]], np.int32)
    probe.probe_best_take(_p(bs), _p(bi), _p(bg), challenger[0], challenger[1], challenger[2])
    want = challenger if taken else incumbent
    assert (_bits(bs[0]), int(bi[0]), int(bg[0])) == (_bits(want[0]), want[1], want[2])


def test_the_statistics_are_the_inline_accumulation_bit_for_bit(probe):
    """softmax_add / entropy_bits against the same operations in the same order written out (the probe's reference): exact."""
    rng = np.random.default_rng(5)
    s = np.ascontiguousarray(rng.uniform(0.0, 60.0, size=300))
    got, want = np.zeros(3), np.zeros(3)
    probe.probe_softmax_stats(_p(s), len(s), float(s.max()), _p(got))
    probe.probe_softmax_stats_inline(_p(s), len(s), float(s.max()), _p(want))
    assert (_bits(got) == _bits(want)).all(), (got, want)
    p = np.exp(s - s.max())
    p /= p.sum()
    assert abs(got[2] + (p * np.log2(p)).sum()) < 1e-9  # (and it is the entropy in bits)


# ---- one definition of each piece, over the kernel sources

def _sources():
    out = {}
    for path in sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.hpp"))):
        with open(path) as fh:
            out[os.path.basename(path)] = fh.read()
    assert "select_math.hpp" in out and "esac_kernels.hip" in out
    return out


def test_the_soft_inlier_term_is_called_from_one_function():
    calls = {name: text.count("soft_inlier_exact(") for name, text in _sources().items() if name != "pose_math.hpp"}
    assert {n: c for n, c in calls.items() if c} == {"select_math.hpp": 1}
    text = _sources()["select_math.hpp"]
    start = text.index("ESAC_HD double exact_cell_term(")
    assert "soft_inlier_exact(" in text[start:text.index("\n}\n", start)]


def test_ln2_and_the_tie_rule_are_written_once():
    text = "\n".join(_sources().values())
    assert text.count("0.6931471805599453") == 1
    assert text.count("og < bg") == 1
