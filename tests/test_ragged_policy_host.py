"""The host's decisions about a ragged batch (esac_hip_forward_batch_shapes; esac_amd/csrc/ragged_policy.hpp, in the order of
batch_plan.hpp's plan_batch -- the function the library's forward route calls, and the probe with it) through a
stand-alone host program -- tests/native/ragged_policy_probe.cpp, built with the host compiler under AddressSanitizer and UBSan,
its own process, no GPU: every rejection of check_shapes names the frame, accepted tables pass on both sides of every bound, and
the per-frame re-score margin is call_scalars' margin of a single call on that frame's grid, bit for bit."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "ragged_policy_probe.cpp")
EXE = os.path.join(HERE, "native", "ragged_policy_probe_san")
DEPS = [SRC] + [os.path.join(HERE, "..", "esac_amd", "csrc", h) for h in ("batch_plan.hpp", "ragged_policy.hpp", "call_policy.hpp")] + \
    [os.path.join(HERE, "..", "include", "esac_hip.h")]


@pytest.fixture(scope="module")
def probe():
    if not os.path.exists(EXE) or any(os.path.getmtime(d) > os.path.getmtime(EXE) for d in DEPS):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=undefined", SRC, "-o", EXE])

    def run(lines):
        out = subprocess.run([EXE], input="".join(l + "\n" for l in lines), capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-2000:])
        rows = [l.split("|") for l in out.stdout.splitlines()]
        assert len(rows) == len(lines), out.stdout
        return rows
    return run


def _check(E, H, W, stride, frames, sub=8):
    """frames: (shift_x, shift_y, focal, h, w) per frame"""
    return "check %d %d %d %d %d %d " % (E, H, W, sub, stride, len(frames)) + " ".join("%d %d %r %d %d" % f for f in frames)


def F(h, w, shift_x=0, shift_y=0, focal=525.0):
    return (shift_x, shift_y, focal, h, w)


# (request, status, all_vec, what the message must contain)
CASES = [
    # accepted: the mixed set of the GPU tests (capacity 32x40 = 1280, E = 3: 3*3*1280 = 11520 floats per slot)
    (_check(3, 32, 40, 11520, [F(32, 40), F(40, 32), F(24, 41), F(30, 30)]), 0, 0, None),
    (_check(3, 32, 40, 11520, [F(32, 40), F(40, 32), F(16, 80)]), 0, 1, None),          # every width a multiple of 4
    (_check(1, 60, 80, 14400, [F(60, 80), F(80, 60)]), 0, 1, None),                      # only the product matters: 80x60 under H=60, W=80
    (_check(1, 60, 80, 14400, [F(3, 3), F(3, 1600), F(1600, 3)]), 0, 0, None),           # the smallest grid, the capacity as one row band
    (_check(2, 96, 88, 50688, [F(96, 88), F(60, 80)]), 0, 1, None),                      # slot == 3*E*h*w of the largest frame exactly
    # area above the capacity
    (_check(3, 32, 40, 11520, [F(32, 40), F(33, 39)]), -4, -1, ["grid 33x39 in frame 1", "1287 cells", "32x40 is 1280"]),
    (_check(1, 60, 80, 16200, [F(60, 80), F(80, 60), F(60, 90)]), -4, -1, ["grid 60x90 in frame 2", "5400 cells"]),
    # slot too small for 3*E*h*w (the capacity would allow the frame)
    (_check(3, 32, 40, 11516, [F(24, 41), F(32, 40)]), -4, -1, ["frame 1", "3*E*h*w = 11520", "sc_frame_stride = 11516"]),
    (_check(2, 96, 88, 50684, [F(60, 80), F(60, 80), F(96, 88)]), -4, -1, ["frame 2", "50688", "50684"]),
    # the stride must keep every slot 16-byte aligned
    (_check(3, 32, 40, 11522, [F(32, 40)]), -4, -1, ["sc_frame_stride 11522", "multiple of 4"]),
    # grid below 3x3 / without four distinct cells / beyond 65535 rows
    (_check(3, 32, 40, 11520, [F(32, 40), F(2, 40)]), -4, -1, ["grid 2x40 too small", "in frame 1"]),
    (_check(3, 32, 40, 11520, [F(40, 2)]), -4, -1, ["grid 40x2 too small", "in frame 0"]),
    (_check(3, 32, 40, 11520, [F(32, 40), F(32, 40), F(0, 0)]), -4, -1, ["grid 0x0 too small", "in frame 2"]),
    (_check(3, 32, 40, 11520, [F(-32, -40)]), -4, -1, ["grid -32x-40 too small", "in frame 0"]),
    (_check(1, 3, 65535, 3 * 3 * 65535 + 1, [F(3, 65535), F(65536, 3)]), -4, -1, ["grid 65536x3 too large", "in frame 1"]),
    # the camera is checked against the frame's OWN pixel range: sub 8, w = 41 -> the last column's centre is 324 - shift_x
    (_check(3, 32, 40, 11520, [F(32, 40), F(24, 41, shift_x=-(2**31 - 1 - 324))]), 0, 0, None),
    (_check(3, 32, 40, 11520, [F(32, 40), F(24, 41, shift_x=-(2**31 - 1 - 324) - 1)]), -4, -1, ["pixel positions overflow int32", "in frame 1"]),
    # ... a shift the 40 columns of the capacity shape would still hold (316 - shift_x), but not this frame's 41
    (_check(3, 32, 40, 11520, [F(24, 41, shift_x=-(2**31 - 1 - 316))]), -4, -1, ["pixel positions overflow int32", "in frame 0"]),
    (_check(3, 32, 40, 11520, [F(40, 32, shift_y=-(2**31 - 1 - 316))]), 0, 1, None),   # 40 rows: 316 - shift_y just fits
    (_check(3, 32, 40, 11520, [F(40, 32, shift_y=-(2**31 - 1 - 316) - 1)]), -4, -1, ["pixel positions overflow int32", "in frame 0"]),
    (_check(3, 32, 40, 11520, [F(32, 40), F(30, 30, focal=0.0)]), -4, -1, ["focal length must be positive in frame 1"]),
    # the capacity shape itself must be a legal grid (check_args)
    (_check(3, 2, 640, 11520, [F(32, 40)]), -4, -1, ["grid 2x640 too small"]),
    # B is held to its range before record 0 is read
    (_check(3, 32, 40, 11520, []), -4, -1, ["batch size 0 outside [1,"]),
    # one frame: the single call on that frame's grid, whose width decides (41 is no multiple of 4, 32 is)
    (_check(3, 32, 40, 11520, [F(24, 41)]), 0, 0, None),
    (_check(3, 32, 40, 11520, [F(40, 32)]), 0, 1, None),
    # the first offending frame is the one named
    (_check(3, 32, 40, 11520, [F(32, 40), F(2, 2), F(99, 99)]), -4, -1, ["grid 2x2 too small", "in frame 1"]),
]


def test_check_shapes_rejections_name_the_frame_and_accepted_tables_pass(probe):
    rows = probe([c[0] for c in CASES])
    for (req, status, all_vec, needles), row in zip(CASES, rows):
        assert row[0] == "check" and int(row[1]) == status and int(row[2]) == all_vec, (req, row)
        if needles is None:
            assert row[3] == "", (req, row)
        else:
            for n in needles:
                assert n in row[3], (req, n, row)
    assert {c[1] for c in CASES} == {0, -4}


MARGIN_GRIDS = [(32, 40), (40, 32), (24, 41), (30, 30), (16, 20), (20, 16), (12, 25), (96, 88), (60, 80), (80, 60), (60, 90), (3, 3)]


def test_per_frame_margin_is_the_single_calls_bit_for_bit(probe):
    reqs, caps = [], []
    for alpha in (100.0, -100.0, 0.1, 1000.0):
        for h, w in MARGIN_GRIDS:
            reqs.append("margin %r 0.0 96 90 %d %d" % (alpha, h, w))  # the default margin: depends on the frame's cells
            caps.append((alpha, h, w))
    reqs.append("margin 100.0 0.25 96 90 30 30")  # an explicit rescore_margin is the margin of every frame
    rows = probe(reqs)
    seen = set()
    for req, row in zip(reqs, rows):
        assert row[0] == "margin" and row[1] == row[2] and row[3] == "1", (req, row)
        seen.add(row[1])
    assert rows[-1][1] == "3e800000"  # 0.25f
    # the margins of frames of different sizes DO differ: a margin taken from the capacity (96x90) would be none of them
    cap_row = probe(["margin 100.0 0.0 96 90 96 90"])[0]
    by_grid = {c: r[1] for c, r in zip(caps, rows) if c[0] == 100.0}
    assert by_grid[(100.0, 30, 30)] != by_grid[(100.0, 32, 40)] != cap_row[1]
    assert len(seen) > len(MARGIN_GRIDS)
