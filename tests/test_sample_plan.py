"""The sampler's launch plan (esac_amd/csrc/sample_plan.hpp) against a RECORDING of what the two launchers it replaced enqueued: each
row of TABLE was taken from a host-side run of launch_sample / sample_can_split as they were before the plan existed (the launch
macro redefined to log kernel, grid, block, first_try and handover), not from sample_plan itself.  At least one row on each side
of every threshold (256, 512, 1024, 4096, 8192 hypotheses in flight; 8 x hypotheses = 8192 and 131072 wavefronts; 131072
hypotheses; max_tries 1024 / 1025), the three flag settings, one expert and several.  No GPU."""
import ctypes as C
import itertools

import pytest

from tests.native import build as native_build

# mirrors of enum SampleFirst / SampleTail (sample_plan.hpp), in declaration order
FIRST = ["none", "256x2", "128x4", "64x2", "128x1", "first32", "first16"]
TAIL = ["none", "exact", "chain"]
EXACT_SAMPLING, STRICT_REFERENCE = 16, 256

# (N, frames, E, max_tries, flags, first_try, packed) ->
# (pack, strict, first kernel, grid x, block, passes, handover, tail, pending list, tail first_try, chain wavefronts, splittable)
# None: nothing of the launch sequence shows the value (no first pass: no grid; no tail: no first_try; no chain: no wavefronts)
TABLE = [
    ((256, 1, 1, 1000000, 0, 0, 0), (False, False, '256x2', 256, 256, 1, 2147483647, 'none', False, None, None, False)),
    ((257, 1, 1, 1000000, 0, 0, 0), (False, False, '128x4', 257, 128, 1, 2147483647, 'none', False, None, None, False)),
    ((512, 1, 1, 1000000, 0, 0, 0), (False, False, '128x4', 512, 128, 1, 2147483647, 'none', False, None, None, False)),
    ((513, 1, 1, 1000000, 0, 0, 0), (False, False, '128x4', 513, 128, 1, 2147483647, 'none', False, None, None, False)),
    ((1024, 1, 1, 1000000, 0, 0, 0), (False, False, '128x4', 1024, 128, 1, 2147483647, 'none', False, None, None, False)),
    ((1025, 1, 1, 1000000, 0, 0, 0), (False, False, '128x1', 1025, 128, 1, 2147483647, 'none', False, None, None, False)),
    ((4096, 1, 1, 1000000, 0, 0, 0), (False, False, '128x1', 4096, 128, 1, 2147483647, 'none', False, None, None, False)),
    ((4097, 1, 1, 1000000, 0, 0, 0), (False, False, 'first32', 2049, 64, 1, 2147483647, 'chain', True, 32, 8192, False)),
    ((8192, 1, 1, 1000000, 0, 0, 0), (False, False, 'first32', 4096, 64, 1, 2147483647, 'chain', True, 32, 8192, False)),
    ((8193, 1, 1, 1000000, 0, 0, 0), (False, False, 'first16', 2049, 64, 2, 2147483647, 'chain', True, 32, 8193, False)),
    ((16384, 1, 1, 1000000, 0, 0, 0), (False, False, 'first16', 4096, 64, 2, 2147483647, 'chain', True, 32, 16384, False)),
    ((16385, 1, 1, 1000000, 0, 0, 0), (False, False, 'first16', 4097, 64, 2, 2147483647, 'chain', True, 32, 16385, False)),
    ((131072, 1, 1, 1000000, 0, 0, 0), (False, False, 'first16', 32768, 64, 2, 2147483647, 'chain', True, 32, 131072, False)),
    ((131073, 1, 1, 1000000, 0, 0, 0), (False, False, 'first16', 32769, 64, 2, 2147483647, 'chain', True, 32, 131073, False)),
    ((256, 1, 1, 1000000, 16, 0, 0), (False, False, '256x2', 256, 256, 1, 2147483647, 'none', False, None, None, False)),
    ((257, 1, 1, 1000000, 16, 0, 0), (False, False, '128x4', 257, 128, 1, 2147483647, 'none', False, None, None, False)),
    ((1024, 1, 1, 1000000, 16, 0, 0), (False, False, '128x4', 1024, 128, 1, 2147483647, 'none', False, None, None, False)),
    ((1025, 1, 1, 1000000, 16, 0, 0), (False, False, '128x1', 1025, 128, 1, 2147483647, 'none', False, None, None, False)),
    ((4096, 1, 1, 1000000, 16, 0, 0), (False, False, '128x1', 4096, 128, 1, 2147483647, 'none', False, None, None, False)),
    ((4097, 1, 1, 1000000, 16, 0, 0), (False, False, 'first32', 2049, 64, 1, 2147483647, 'exact', False, 32, None, False)),
    ((8192, 1, 1, 1000000, 16, 0, 0), (False, False, 'first32', 4096, 64, 1, 2147483647, 'exact', False, 32, None, False)),
    ((8193, 1, 1, 1000000, 16, 0, 0), (False, False, 'first16', 2049, 64, 2, 2147483647, 'exact', False, 32, None, False)),
    ((256, 1, 1, 1000000, 256, 0, 0), (False, True, '256x2', 256, 256, 1, 2147483647, 'none', False, None, None, False)),
    ((257, 1, 1, 1000000, 256, 0, 0), (False, True, '128x4', 257, 128, 1, 2147483647, 'none', False, None, None, False)),
    ((1024, 1, 1, 1000000, 256, 0, 0), (False, True, '128x4', 1024, 128, 1, 2147483647, 'none', False, None, None, False)),
    ((1025, 1, 1, 1000000, 256, 0, 0), (False, True, '128x1', 1025, 128, 1, 2147483647, 'none', False, None, None, False)),
    ((4096, 1, 1, 1000000, 256, 0, 0), (False, True, '128x1', 4096, 128, 1, 2147483647, 'none', False, None, None, False)),
    ((4097, 1, 1, 1000000, 256, 0, 0), (False, True, 'first32', 2049, 64, 1, 2147483647, 'exact', False, 32, None, False)),
    ((8192, 1, 1, 1000000, 256, 0, 0), (False, True, 'first32', 4096, 64, 1, 2147483647, 'exact', False, 32, None, False)),
    ((8193, 1, 1, 1000000, 256, 0, 0), (False, True, 'first16', 2049, 64, 2, 2147483647, 'exact', False, 32, None, False)),
    ((256, 1, 2, 1000000, 0, 0, 0), (False, False, '256x2', 256, 256, 1, 32, 'chain', False, 32, 8192, True)),
    ((257, 1, 2, 1000000, 0, 0, 0), (False, False, '128x4', 257, 128, 1, 32, 'chain', False, 32, 8192, True)),
    ((512, 1, 2, 1000000, 0, 0, 0), (False, False, '128x4', 512, 128, 1, 32, 'chain', False, 32, 8192, True)),
    ((513, 1, 2, 1000000, 0, 0, 0), (False, False, '64x2', 513, 64, 1, 32, 'chain', False, 32, 8192, True)),
    ((1024, 1, 2, 1000000, 0, 0, 0), (False, False, '64x2', 1024, 64, 1, 32, 'chain', False, 32, 8192, True)),
    ((1025, 1, 2, 1000000, 0, 0, 0), (False, False, 'first32', 513, 64, 1, 2147483647, 'chain', True, 32, 8200, True)),
    ((4096, 1, 2, 1000000, 0, 0, 0), (False, False, 'first32', 2048, 64, 1, 2147483647, 'chain', True, 32, 32768, True)),
    ((4097, 1, 2, 1000000, 0, 0, 0), (False, False, 'first32', 2049, 64, 1, 2147483647, 'chain', True, 32, 32776, True)),
    ((8192, 1, 2, 1000000, 0, 0, 0), (False, False, 'first32', 4096, 64, 1, 2147483647, 'chain', True, 32, 65536, True)),
    ((8193, 1, 2, 1000000, 0, 0, 0), (False, False, 'none', None, None, 0, 2147483647, 'chain', True, 0, 65544, False)),
    ((16384, 1, 2, 1000000, 0, 0, 0), (False, False, 'none', None, None, 0, 2147483647, 'chain', True, 0, 131072, False)),
    ((16385, 1, 2, 1000000, 0, 0, 0), (False, False, 'none', None, None, 0, 2147483647, 'chain', True, 0, 131072, False)),
    ((131072, 1, 2, 1000000, 0, 0, 0), (False, False, 'none', None, None, 0, 2147483647, 'chain', True, 0, 131072, False)),
    ((131073, 1, 2, 1000000, 0, 0, 0), (False, False, 'none', None, None, 0, 2147483647, 'chain', True, 0, 131073, False)),
    ((256, 1, 2, 1000000, 16, 0, 0), (False, False, '256x2', 256, 256, 1, 2147483647, 'none', False, None, None, False)),
    ((257, 1, 2, 1000000, 16, 0, 0), (False, False, '128x4', 257, 128, 1, 2147483647, 'none', False, None, None, False)),
    ((1024, 1, 2, 1000000, 16, 0, 0), (False, False, '128x4', 1024, 128, 1, 2147483647, 'none', False, None, None, False)),
    ((1025, 1, 2, 1000000, 16, 0, 0), (False, False, '128x1', 1025, 128, 1, 2147483647, 'none', False, None, None, False)),
    ((4096, 1, 2, 1000000, 16, 0, 0), (False, False, '128x1', 4096, 128, 1, 2147483647, 'none', False, None, None, False)),
    ((4097, 1, 2, 1000000, 16, 0, 0), (False, False, 'first32', 2049, 64, 1, 2147483647, 'exact', False, 32, None, False)),
    ((8192, 1, 2, 1000000, 16, 0, 0), (False, False, 'first32', 4096, 64, 1, 2147483647, 'exact', False, 32, None, False)),
    ((8193, 1, 2, 1000000, 16, 0, 0), (False, False, 'first16', 2049, 64, 2, 2147483647, 'exact', False, 32, None, False)),
    ((256, 1, 2, 1000000, 256, 0, 0), (False, True, '256x2', 256, 256, 1, 2147483647, 'none', False, None, None, False)),
    ((257, 1, 2, 1000000, 256, 0, 0), (False, True, '128x4', 257, 128, 1, 2147483647, 'none', False, None, None, False)),
    ((1024, 1, 2, 1000000, 256, 0, 0), (False, True, '128x4', 1024, 128, 1, 2147483647, 'none', False, None, None, False)),
    ((1025, 1, 2, 1000000, 256, 0, 0), (False, True, '128x1', 1025, 128, 1, 2147483647, 'none', False, None, None, False)),
    ((4096, 1, 2, 1000000, 256, 0, 0), (False, True, '128x1', 4096, 128, 1, 2147483647, 'none', False, None, None, False)),
    ((4097, 1, 2, 1000000, 256, 0, 0), (False, True, 'first32', 2049, 64, 1, 2147483647, 'exact', False, 32, None, False)),
    ((8192, 1, 2, 1000000, 256, 0, 0), (False, True, 'first32', 4096, 64, 1, 2147483647, 'exact', False, 32, None, False)),
    ((8193, 1, 2, 1000000, 256, 0, 0), (False, True, 'first16', 2049, 64, 2, 2147483647, 'exact', False, 32, None, False)),
    ((1025, 1, 50, 1000000, 0, 0, 0), (False, False, 'first32', 513, 64, 1, 2147483647, 'chain', True, 32, 8200, True)),
    ((16384, 1, 50, 1000000, 0, 0, 0), (False, False, 'none', None, None, 0, 2147483647, 'chain', True, 0, 131072, False)),
    ((16385, 1, 50, 1000000, 0, 0, 0), (False, False, 'none', None, None, 0, 2147483647, 'chain', True, 0, 131072, False)),
    ((513, 1, 2, 1024, 0, 0, 0), (False, False, '128x4', 513, 128, 1, 2147483647, 'none', False, None, None, False)),
    ((513, 1, 2, 1025, 0, 0, 0), (False, False, '64x2', 513, 64, 1, 32, 'chain', False, 32, 8192, True)),
    ((1025, 1, 2, 1024, 0, 0, 0), (False, False, '128x1', 1025, 128, 1, 2147483647, 'none', False, None, None, False)),
    ((8193, 1, 1, 1024, 0, 32, 0), (False, False, 'first16', 2049, 64, 2, 2147483647, 'chain', True, 64, 8193, False)),
    ((511, 1, 2, 1000000, 0, 32, 0), (False, False, '128x4', 511, 128, 1, 32, 'chain', False, 32, 8192, False)),
    ((2048, 1, 2, 1000000, 0, 32, 0), (False, False, 'first32', 1024, 64, 1, 2147483647, 'chain', True, 64, 16384, False)),
    ((512, 1, 2, 1000000, 0, 0, 1), (True, False, '128x4', 512, 128, 1, 32, 'chain', False, 32, 8192, True)),
    ((4097, 1, 1, 1000000, 0, 0, 1), (True, False, 'first32', 2049, 64, 1, 2147483647, 'chain', True, 32, 8192, False)),
    ((256, 2, 2, 1000000, 0, 0, 0), (False, False, '128x4', 256, 128, 1, 32, 'chain', False, 32, 8192, False)),
    ((257, 2, 2, 1000000, 0, 0, 0), (False, False, '64x2', 257, 64, 1, 32, 'chain', False, 32, 8192, False)),
    ((256, 32, 2, 1000000, 0, 0, 0), (False, False, 'first32', 128, 64, 1, 2147483647, 'chain', True, 32, 65536, False)),
    ((257, 32, 2, 1000000, 0, 0, 0), (False, False, 'none', None, None, 0, 2147483647, 'chain', True, 0, 65792, False)),
    ((4096, 32, 1, 1000000, 0, 0, 0), (False, False, 'first16', 1024, 64, 2, 2147483647, 'chain', True, 32, 131072, False)),
    ((4097, 32, 2, 1000000, 0, 0, 0), (False, False, 'none', None, None, 0, 2147483647, 'chain', True, 0, 131104, False)),
    ((1, 1, 1, 1000000, 0, 0, 0), (False, False, '256x2', 1, 256, 1, 2147483647, 'none', False, None, None, False)),
]


@pytest.fixture(scope="module")
def plan():
    lib = C.CDLL(native_build.build_sample_plan_probe())
    lib.probe_sample_plan.argtypes = [C.c_int] * 7 + [C.POINTER(C.c_int)]
    lib.probe_sample_plan.restype = None
    keys = ("pack", "strict", "first", "grid_x", "block", "passes", "pass_tries", "handover", "tail", "pending_list",
            "tail_first_try", "chain_waves", "splittable")

    def call(N, frames, E, max_tries, flags, first_try, packed):
        out = (C.c_int * 13)()
        lib.probe_sample_plan(N, frames, E, max_tries, flags, first_try, packed, out)
        d = dict(zip(keys, out))
        d["first"], d["tail"] = FIRST[d["first"]], TAIL[d["tail"]]
        return d
    return call


def test_table_covers_both_sides_of_every_threshold():
    totals = {k[0] * k[1] for k, _ in TABLE}
    for t in (256, 512, 1024, 4096, 8192, 131072):
        assert t in totals and any(t < x <= t + 64 for x in totals), t
    chain8 = {8 * k[0] * k[1] for k, _ in TABLE if k[2] > 1}
    for t in (8192, 131072):
        assert t in chain8 and any(t < x <= t + 64 for x in chain8), t
    assert {k[4] for k, _ in TABLE} == {0, EXACT_SAMPLING, STRICT_REFERENCE}
    assert {k[2] == 1 for k, _ in TABLE} == {True, False}
    assert {k[3] for k, _ in TABLE} >= {1024, 1025}


def test_plan_is_what_the_launchers_decided(plan):
    for key, want in TABLE:
        p = plan(*key)
        got = (bool(p["pack"]), bool(p["strict"]), p["first"], p["grid_x"] if p["passes"] else None, p["block"] if p["passes"] else None,
               p["passes"], p["handover"], p["tail"], bool(p["pending_list"]), p["tail_first_try"] if p["tail"] != "none" else None,
               p["chain_waves"] if p["tail"] == "chain" else None, bool(p["splittable"]))
        assert got == want, key


def test_first_pass_plus_tail_is_the_full_plan_wherever_it_splits(plan):
    """launch_sample_split enqueues everything up to the tail, its caller the screened chain: together they are launch_sample's
    sequence exactly when the plan HAS a first pass and its tail IS the chain (nothing else is left out, nothing runs twice)."""
    n_split = 0
    grid = itertools.product((1, 255, 256, 257, 512, 513, 1024, 1025, 4096, 4097, 8192, 8193, 16384), (1, 2, 32), (1, 2, 50),
                             (1024, 1025, 1000000), (0, EXACT_SAMPLING, STRICT_REFERENCE), (0, 32), (0, 1))
    for key in grid:
        p = plan(*key)
        N, frames, E, max_tries, flags, first_try, _ = key
        assert bool(p["splittable"]) == (frames == 1 and E > 1 and max_tries > 1024 and flags == 0 and N <= 8192 and first_try == 0), key
        if not p["splittable"]:
            continue
        n_split += 1
        assert p["first"] in ("256x2", "128x4", "64x2", "first32") and p["passes"] == 1, key
        assert p["tail"] == "chain" and p["tail_first_try"] == 32 and not p["strict"], key
        assert bool(p["pending_list"]) == (p["first"] == "first32"), key
    assert n_split == 11 * 2 * 2 * 2
