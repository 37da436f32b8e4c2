"""Compile-time budget of the headline call's refinement kernel, k_refine_team_route<2, 16>: the team kernel's body with the
headline call's modes (fold mode 2, no speculation, one expert, no debug knob) as constants (no GPU needed: the ISA of hipcc -S,
classified by scripts/dev/isa_counts.py).  What the route kernel is for is what it does NOT contain, so its size is pinned:
ceilings are the tree's own counts + 5 % for compiler jitter, the general kernel's count of the same tree in a comment.  The
general kernel k_refine_team<2, 0, 16> keeps the ceilings of tests/test_headline_isa_budget.py."""
import importlib.util
import os
import shutil

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else shutil.which("hipcc")
pytestmark = pytest.mark.skipif(HIPCC is None, reason="hipcc not available")

ROUTE, GENERAL = "k_refine_team_routeILi2ELi16EE", "k_refine_teamILi2ELi0ELi16EE"


@pytest.fixture(scope="module")
def counts():
    spec = importlib.util.spec_from_file_location("isa_counts", os.path.join(ROOT, "scripts", "dev", "isa_counts.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    res = mod.count_kernels([ROUTE, GENERAL])
    assert len(res) == 2, sorted(res)
    return {("route" if ROUTE in name else "general"): r for name, r in res.items()}


def test_route_kernel_exists_without_scratch(counts):
    assert counts["route"]["registers"]["ScratchSize"] == 0
    assert counts["route"]["registers"]["NumVgprs"] <= 256


def test_route_kernel_size_spills_and_copies(counts):
    k = counts["route"]["kernel"]
    assert k["total"] <= 5894, k       # 5,614 (the general kernel: 9,381)
    assert k["spill_lane"] <= 132, k   # 126   (the general kernel: 470)
    assert k["agpr"] <= 39, k          # 38    (the general kernel: 48)


def test_route_kernel_round_loop(counts):
    """The round loop (the largest natural loop of the kernel) is the same work in both kernels."""
    loop = counts["route"]["largest_loop"]
    assert 2000 < loop["total"] <= 3080, loop  # 2,934 (the general kernel: 2,941); under the general kernel's 3,300 in any case
    assert loop["total"] < 3300, loop
    assert loop["spill_lane"] <= 29, loop      # 28 (the general kernel: 34)
    assert loop["agpr"] <= 12, loop            # 12 (the general kernel: 12)


def test_general_kernel_still_meets_its_ceilings(counts):
    k, loop = counts["general"]["kernel"], counts["general"]["largest_loop"]
    assert k["agpr"] <= 50, k
    assert k["spill_lane"] <= 501, k
    assert 2000 < loop["total"] < 3300, loop
    assert loop["spill_lane"] <= 40, loop
    assert counts["general"]["registers"]["ScratchSize"] == 0
