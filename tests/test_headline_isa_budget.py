"""Compile-time budget of the instructions that compute nothing in the headline call's two long kernels (no GPU needed: the ISA
of hipcc -S, classified by scripts/dev/isa_counts.py).  Both kernels run one wavefront per SIMD and are bound by what they issue
(LAB_NOTES.md, rounds 4 and 11): a copy between the two register files or a lane move that reloads a spilled scalar register
costs what an FMA costs.  Ceilings: the tree's own counts + 5 % for compiler jitter; the count of the commit before them in a
comment."""
import importlib.util
import os
import shutil

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else shutil.which("hipcc")
pytestmark = pytest.mark.skipif(HIPCC is None, reason="hipcc not available")


@pytest.fixture(scope="module")
def counts():
    spec = importlib.util.spec_from_file_location("isa_counts", os.path.join(ROOT, "scripts", "dev", "isa_counts.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    res = mod.count_kernels(["k_sampleILi256ELi2E", "k_refine_teamILi2ELi0ELi16EE"])
    assert len(res) == 2, sorted(res)
    return {("sample" if "k_sample" in name else "team"): r for name, r in res.items()}


def test_sampler_register_file_copies_and_spill_lane_moves(counts):
    k = counts["sample"]["kernel"]
    assert k["agpr"] <= 1120, k        # 1,067 (the commit before: 1,067 -- the sampler's source is unchanged)
    assert k["spill_lane"] <= 281, k   # 268   (the commit before: 268)
    assert counts["sample"]["registers"]["ScratchSize"] == 0


def test_team_kernel_register_file_copies_and_spill_lane_moves(counts):
    k, loop = counts["team"]["kernel"], counts["team"]["largest_loop"]
    assert k["agpr"] <= 50, k          # 48  (the commit before: 57)
    assert k["spill_lane"] <= 501, k   # 478 (the commit before: 568)
    # the round loop (the largest natural loop of the kernel, its two rare heavy paths included)
    assert 2000 < loop["total"] < 3300, loop
    assert loop["spill_lane"] <= 40, loop  # 38 (the commit before: 50)
    assert counts["team"]["registers"]["ScratchSize"] == 0
