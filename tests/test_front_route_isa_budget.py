"""Compile-time budget of the front route's two kernels, k_sample_route<256, 2> and k_rescore_route<1024, 5> (the headline call's
instantiations): the sampler's and the exact score's bodies with the headline call's modes as constants (no GPU needed: the ISA
of hipcc -S, classified by scripts/dev/isa_counts.py).  What the route kernels are for is what they do NOT contain, so their
size is pinned: ceilings are the tree's own counts + 5 % for compiler jitter, the general kernel's count of the same tree in a
comment.  The general sampler k_sample<256, 2> keeps the ceilings of tests/test_headline_isa_budget.py."""
import importlib.util
import os
import shutil

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else shutil.which("hipcc")
pytestmark = pytest.mark.skipif(HIPCC is None, reason="hipcc not available")

SAMPLE, SCORE = "k_sample_routeILi256ELi2E", "k_rescore_routeILi1024ELi"


@pytest.fixture(scope="module")
def counts():
    spec = importlib.util.spec_from_file_location("isa_counts", os.path.join(ROOT, "scripts", "dev", "isa_counts.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.HEADLINE[SCORE] = "esac_front_route.hip"  # every instantiation of the scorer
    res = mod.count_kernels([SAMPLE, SCORE])
    assert len(res) == 9, sorted(res)
    return res


def test_route_sampler_size_spills_and_registers(counts):
    (r,) = [v for n, v in counts.items() if SAMPLE in n]
    k, loop = r["kernel"], r["largest_loop"]
    assert k["total"] <= 7845, k        # 7,472 (the general kernel: 8,229)
    assert k["spill_lane"] <= 121, k    # 116   (the general kernel: 258)
    assert 6000 < loop["total"] <= 7354, loop  # 7,004: the try loop is the general kernel's (7,002)
    assert loop["spill_lane"] <= 90, loop      # 86 (the general kernel: 170)
    assert r["registers"]["ScratchSize"] == 0
    assert r["registers"]["NumVgprs"] <= 256


def test_route_scorer_every_instantiation_fits_four_wavefronts_per_simd(counts):
    """1024 threads per workgroup: at most 128 registers per lane, and nothing in scratch, for 1..8 cells per lane."""
    score = {n: v for n, v in counts.items() if SCORE in n}
    assert len(score) == 8
    for name, r in score.items():
        assert r["registers"]["ScratchSize"] == 0, (name, r)
        assert r["registers"]["NumVgprs"] + r["registers"].get("NumAgprs", 0) <= 128, (name, r)
        assert r["kernel"]["spill_lane"] == 0 and r["kernel"]["agpr"] == 0, (name, r)
        assert r["largest_loop"]["total"] == 0, (name, r)  # straight-line code: the cells are unrolled, no grid-stride loop
    (five,) = [v for n, v in score.items() if n.split(SCORE)[1].startswith("5E")]
    assert five["kernel"]["total"] <= 1156, five  # 1,101: five cells unrolled (the general kernel's loop body: 336 a cell)
