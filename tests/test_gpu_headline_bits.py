"""The headline call's kernels (k_sample<256, 2>, k_rescore, k_refine_team) on the paths the default frames do not take, each case ONE
call: against the CPU oracle the way tests/test_gpu_parity.py compares (index work with assert_array_equal -- tries, sampled cells,
inlier counts per step, inlier map, step count; hypotheses, scores and pose at that file's tolerances), and bit for bit against
tests/golden/headline_bits/headline_bits.npz -- the same calls on the library of the commit before the kernels' registers were rearranged
(tests/golden/make_headline_bits.py): where a value lives and when it is formed must not move a bit of what the call returns.

Every case asserts ON THE ORACLE'S OUTPUT that its path is taken, so none can pass by missing it."""
import os

import numpy as np
import pytest

from esac_amd import api
from tests import headline_bits_cases as H
from tests.test_gpu_parity import _check_full

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "headline_bits", "headline_bits.npz")


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def _run(engine, oracle, golden, case):
    dev = H.run_device(engine, case)
    ref = H.run_oracle(oracle, case)
    res = engine.read(api.BUF_RESULT)
    _check_full(engine, res, ref)
    for name in list(H.BUFFERS) + ["record"]:
        np.testing.assert_array_equal(H.bits(dev[name]), golden["%s/%s" % (case, name)], err_msg="%s/%s" % (case, name))
    return dev, ref


@pytest.mark.parametrize("k", range(3))
def test_second_round_one_try_per_lane(engine, oracle, golden, k):
    """60 % outliers: dozens of hypotheses find no accepted try among the first 128 (the shared rounds, two lanes a try) and go on
    in the rounds of one try per lane -- the sampler's second p3p_4pt copy."""
    dev, ref = _run(engine, oracle, golden, "second_round_k%d" % k)
    assert int((ref["tries"] >= 128).sum()) >= 8  # (the oracle here: 56 / 103 / 44)


def test_exhausted_try_budget(engine, oracle, golden):
    """max_tries = 8: half the hypotheses use up the budget -- the state of the last try remains, tries = -1."""
    dev, ref = _run(engine, oracle, golden, "exhausted_budget")
    assert int((ref["tries"] == -1).sum()) >= 64  # (the oracle here: 131)


def test_team_with_one_cell_per_lane(engine, oracle, golden):
    """A 32x40 grid, seven hypotheses: five members of 256 cells, k_refine_team<1, ...>."""
    dev, ref = _run(engine, oracle, golden, "one_cell_per_lane")
    assert ref["ref_steps"] >= 1  # (the oracle here: 3 accepted steps)
    assert dev["refine_info"]["mode"] == "team" and dev["refine_info"]["workgroups"] == 5


@pytest.mark.parametrize("case,members", [("team_default", 10), ("team_of_eight", 8)])
def test_team_with_two_and_three_cells_per_lane(engine, oracle, golden, case, members):
    """The 60x80 grid: the default team of ten (two cells per lane, k_refine_team<2, 0, 16>) and a team of eight (three per lane,
    k_refine_team<3, 0, 8>)."""
    dev, ref = _run(engine, oracle, golden, case)
    assert dev["refine_info"]["mode"] == "team" and dev["refine_info"]["workgroups"] == members
