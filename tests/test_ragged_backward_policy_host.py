"""The host's decisions about a ragged TRAINING batch (esac_hip_backward_batch_shapes / esac_hip_backward_batch_dev_shapes;
esac_amd/csrc/ragged_policy.hpp) through a stand-alone host program -- tests/native/ragged_backward_policy_probe.cpp, built with
the host compiler under AddressSanitizer and UBSan, its own process, no GPU: every new fail() message, the gradient-slot check
on both sides of its bound (held against every frame's OWN grid, never the capacity), and the chunking by the capacity's slot.
The probe calls plan_batch (esac_amd/csrc/batch_plan.hpp), the function the library's three batch routes call: the order of the
checks is the library's, and what the plan hands on (parameter block, staging, KArgs::shapes, frame 0's cells, the records) is held
here too."""
import os
import re
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "ragged_backward_policy_probe.cpp")
EXE = os.path.join(HERE, "native", "ragged_backward_policy_probe_san")
POLICY = os.path.join(HERE, "..", "esac_amd", "csrc", "ragged_policy.hpp")
DEPS = [SRC, POLICY, os.path.join(HERE, "..", "esac_amd", "csrc", "batch_plan.hpp"), os.path.join(HERE, "..", "esac_amd", "csrc", "call_policy.hpp"), os.path.join(HERE, "..", "include", "esac_hip.h")]
BLOCKING, ASYNC = "esac_hip_backward_batch_shapes", "esac_hip_backward_batch_dev_shapes"


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


def F(h, w, shift_x=0, shift_y=0, focal=525.0):
    return (shift_x, shift_y, focal, h, w)


def _bwd(E, H, W, sc_stride, grad_stride, frames, who=0, table=1, sub=8):
    return "bwd %d %d %d %d %d %d %d %d %d " % (who, table, E, H, W, sub, sc_stride, grad_stride, len(frames)) + \
        " ".join("%d %d %r %d %d" % f for f in frames)


MIXED = [F(12, 16), F(16, 12), F(12, 18), F(12, 16)]  # 192, 192, 216 cells: E = 3 -> 1728, 1728, 1944 floats per frame
# (request, status, all_vec, what the message must contain)
CASES = [
    # accepted: the mixed set of the GPU tests; the stride is exactly 3*E*max(h*w)
    (_bwd(3, 12, 18, 1944, 1944, MIXED), 0, 0, None),
    (_bwd(3, 12, 18, 1944, 1944, MIXED, who=1), 0, 0, None),
    (_bwd(3, 12, 18, 1944, 1944, [F(12, 16), F(16, 12)]), 0, 1, None),
    # the capacity (here 20x20 = 400 cells) is no bound of the gradient stride: the largest FRAME is
    (_bwd(3, 20, 20, 3600, 1944, MIXED), 0, 0, None),
    # one frame has no stride to fit
    (_bwd(3, 12, 18, 1944, 0, [F(12, 18)]), 0, 0, None),
    (_bwd(2, 96, 88, 50688, 50688, [F(12, 16), F(96, 88)]), 0, 1, None),
    # one float short for the largest frame: the frame is named, whichever place it has in the table
    (_bwd(3, 12, 18, 1944, 1943, MIXED), -4, -1, [BLOCKING + ":", "the gradients of frame 2", "3*E*h*w = 1944", "grid 12x18", "grad_frame_stride = 1943", "share gradients"]),
    (_bwd(3, 12, 18, 1944, 1943, MIXED, who=1), -4, -1, [ASYNC + ":", "the gradients of frame 2", "grad_frame_stride = 1943"]),
    (_bwd(3, 12, 18, 1944, 1727, MIXED), -4, -1, ["the gradients of frame 0", "3*E*h*w = 1728", "grid 12x16"]),
    (_bwd(3, 12, 18, 1944, 0, MIXED), -4, -1, ["the gradients of frame 0", "grad_frame_stride = 0"]),
    (_bwd(3, 12, 18, 1944, -1944, MIXED), -4, -1, ["the gradients of frame 0", "grad_frame_stride = -1944"]),
    (_bwd(2, 96, 88, 50688, 50687, [F(12, 16), F(96, 88)]), -4, -1, ["the gradients of frame 1", "50688", "50687"]),
    # a null table
    (_bwd(3, 12, 18, 1944, 1944, MIXED, table=0), -1, -1, [BLOCKING + ": null frame table", "h_cams"]),
    (_bwd(3, 12, 18, 1944, 1944, MIXED, who=1, table=0), -1, -1, [ASYNC + ": null frame table"]),
    # the forward table's checks, under the training call's name
    (_bwd(3, 12, 16, 1944, 1944, MIXED), -4, -1, [BLOCKING + ": grid 12x18 in frame 2", "216 cells", "12x16 is 192"]),
    (_bwd(3, 12, 18, 1940, 1944, MIXED), -4, -1, [BLOCKING + ": the maps of frame 2", "sc_frame_stride = 1940"]),
    (_bwd(3, 12, 18, 1946, 1946, MIXED, who=1), -4, -1, [ASYNC + ": sc_frame_stride 1946", "multiple of 4"]),
    (_bwd(3, 12, 18, 1944, 1944, [F(12, 16), F(2, 16)]), -4, -1, ["grid 2x16 too small", "in frame 1"]),
    (_bwd(3, 12, 18, 1944, 1944, [F(12, 16), F(12, 18, focal=0.0)]), -4, -1, ["focal length must be positive in frame 1"]),
    # a bad shape is reported before the gradient slot that it would also break
    (_bwd(3, 12, 18, 1944, 10, [F(12, 16), F(0, 0)]), -4, -1, ["grid 0x0 too small", "in frame 1"]),
    (_bwd(3, 12, 18, 1944, 1944, [F(12, 16), F(13, 17)]), -4, -1, ["grid 13x17 in frame 1", "221 cells"]),
    # the shared-shape call's own refusals stay in front, under its name and in its words
    (_bwd(70000, 12, 18, 1944, 1944, MIXED), -4, -1, ["esac_hip_backward_batch: at most 65535 experts"]),
    (_bwd(3, 12, 18, -4, 1944, MIXED), -4, -1, ["esac_hip_backward_batch: negative coordinate frame stride"]),
    (_bwd(3, 12, 18, 1944, 1944, []), -4, -1, ["esac_hip_backward_batch: batch size 0 outside"]),
]


def test_every_refusal_names_the_frame_and_accepted_tables_pass(probe):
    rows = probe([c[0] for c in CASES])
    for (req, status, all_vec, needles), row in zip(CASES, rows):
        assert row[0] == "bwd" and int(row[1]) == status and int(row[2]) == all_vec, (req, row)
        if needles is None:
            assert row[3] == "", (req, row)
        else:
            for n in needles:
                assert n in row[3], (req, n, row)
    assert {c[1] for c in CASES} == {0, -1, -4}


def test_every_fail_message_of_the_training_checks_is_held(probe):
    """Each fail() of ragged_policy.hpp's training section is produced by at least one case above."""
    text = open(POLICY).read()
    section = text[text.index("ragged TRAINING batches"):]
    heads = re.findall(r'fail\(-?\d+, "%s: ([^"%]{12,})', section)
    assert len(heads) == 2, heads  # the null table, the gradient slot
    rows = probe([c[0] for c in CASES])
    said = " ".join(r[3] for r in rows)
    for h in heads:
        assert h.strip() in said, h


def test_chunks_are_sized_by_the_capacity(probe):
    """bwd_slot_bytes of the capacity: 2 P map bytes + two 3 P double slabs (+ the list above 8192 cells)."""
    P = 216
    slot = 2 * P + 2 * 3 * P * 8
    rows = probe(["chunk %d 64 %d 5" % (2 * 64 * slot, P), "chunk %d 64 %d 5" % (2 * 64 * slot - 1, P), "chunk %d 64 %d 5" % (1, P),
                  "chunk %d 64 %d 5" % (100 * 64 * slot, P), "chunk %d 32 %d 2" % (1 << 40, 96 * 88)])
    assert [int(r[1]) for r in rows] == [2, 1, 1, 5, 2]
    assert int(rows[0][2]) == slot
    assert int(rows[4][2]) == 2 * 8448 + 48 * 8448 + 16 * 10240  # 8448 cells: 5 trips of 2048 -> a list of 10240 entries


FORWARD, TRAIN, TRAIN_ASYNC = 0, 1, 2


def _plan(route, ragged, E, H, W, sc_stride, grad_stride, frames, table=1, sub=8):
    return "plan %d %d %d %d %d %d %d %d %d %d " % (route, ragged, table, E, H, W, sub, sc_stride, grad_stride, len(frames)) + \
        " ".join("%d %d %r %d %d" % f for f in frames)


SAME = [F(12, 18), F(12, 18), F(12, 18)]
# (request, status, (stage, shapes, H, W, frame 0's cells) or what the message must contain)
PLAN_CASES = [
    # a ragged call of ONE frame is the single call on that frame's grid: its H x W in the block, shapes 0 (a width that is no
    # multiple of 4 must not leave mode 2 set), no frame-0 cells; the forward route has record 0 inline and stages nothing
    (_plan(FORWARD, 1, 1, 12, 18, 648, 0, [F(9, 14)]), 0, (0, 0, 9, 14, 0)),
    (_plan(TRAIN, 1, 1, 12, 18, 648, 0, [F(9, 14)]), 0, (1, 0, 9, 14, 0)),
    (_plan(TRAIN_ASYNC, 1, 1, 12, 18, 648, 0, [F(9, 14)]), 0, (1, 0, 9, 14, 0)),
    # shapes over the WHOLE table: 1 when every width is a multiple of 4, 2 when any is not; the block keeps the capacity
    (_plan(TRAIN, 1, 3, 12, 18, 1944, 1944, [F(12, 16), F(16, 12)]), 0, (1, 1, 12, 18, 192)),
    (_plan(TRAIN_ASYNC, 1, 3, 12, 18, 1944, 1944, MIXED), 0, (1, 2, 12, 18, 192)),
    (_plan(TRAIN, 1, 3, 12, 18, 1944, 1944, [F(12, 16), F(16, 12), F(12, 16), F(9, 14)]), 0, (1, 2, 12, 18, 192)),  # the last width alone
    (_plan(FORWARD, 1, 3, 12, 18, 1944, 0, [F(9, 14), F(12, 16)]), 0, (1, 2, 12, 18, 126)),  # frame 0's OWN cells
    (_plan(FORWARD, 1, 3, 12, 18, 1944, 0, [F(16, 12), F(12, 16)]), 0, (1, 1, 12, 18, 192)),
    # a shared-shape table: staged as it is (forward: from two frames on), no mode, no cells
    (_plan(FORWARD, 0, 3, 12, 18, 1944, 0, SAME), 0, (1, 0, 12, 18, 0)),
    (_plan(FORWARD, 0, 3, 12, 18, 1944, 0, SAME[:1]), 0, (0, 0, 12, 18, 0)),
    (_plan(TRAIN, 0, 3, 12, 18, 1944, 1944, SAME[:1]), 0, (1, 0, 12, 18, 0)),
    (_plan(TRAIN_ASYNC, 0, 3, 12, 18, 1944, 1944, SAME), 0, (1, 0, 12, 18, 0)),
    # no table: nothing to stage
    (_plan(FORWARD, 0, 3, 12, 18, 1944, 0, [], table=0), 0, (0, 0, 12, 18, 0)),
    (_plan(TRAIN, 0, 3, 12, 18, 1944, 1944, SAME, table=0), 0, (0, 0, 12, 18, 0)),
    # a shared-shape table with a bad camera in frame b names frame b, on every route
    (_plan(FORWARD, 0, 3, 12, 18, 1944, 0, [F(12, 18), F(12, 18), F(12, 18, focal=0.0)]), -4, ["focal length must be positive in frame 2"]),
    (_plan(TRAIN, 0, 3, 12, 18, 1944, 1944, [F(12, 18), F(12, 18, focal=-1.0), F(12, 18, focal=0.0)]), -4, ["focal length must be positive in frame 1"]),
    (_plan(TRAIN_ASYNC, 0, 3, 12, 18, 1944, 1944, [F(12, 18), F(12, 18, shift_x=-(2**31 - 1))]), -4, ["pixel positions overflow int32", "in frame 1"]),
    (_plan(TRAIN, 0, 3, 12, 18, 1944, 1944, [F(12, 18, focal=0.0)]), -4, ["focal length must be positive in frame 0"]),
    # a null table wins over every other bad argument of a ragged call, B = 0 included, on both training routes and forward
    (_plan(TRAIN, 1, 3, 12, 18, 1944, 1944, [], table=0), -1, [BLOCKING + ": null frame table"]),
    (_plan(TRAIN_ASYNC, 1, 3, 12, 18, 1944, 1944, [], table=0), -1, [ASYNC + ": null frame table"]),
    (_plan(TRAIN, 1, 70000, 12, 18, -4, 1944, MIXED, table=0), -1, [BLOCKING + ": null frame table"]),
    (_plan(FORWARD, 1, 3, 12, 18, 1944, 0, [], table=0), -1, ["esac_hip_forward_batch_shapes: null frame table"]),
    # ... and B is held to its range before record 0 is read
    (_plan(FORWARD, 1, 3, 12, 18, 1944, 0, []), -4, ["batch size 0 outside [1,"]),
    (_plan(FORWARD, 0, 3, 12, 18, 1944, 0, []), -4, ["batch size 0 outside [1,"]),
    (_plan(TRAIN_ASYNC, 0, 3, 12, 18, 1944, 1944, []), -4, ["esac_hip_backward_batch: batch size 0 outside"]),
    # the shared-shape training call still holds the gradient stride against E*3*H*W
    (_plan(TRAIN, 0, 3, 12, 18, 1944, 1943, SAME), -4, ["gradient frame stride 1943 < E*3*H*W = 1944"]),
]


def test_what_the_plan_hands_on(probe):
    rows = probe([c[0] for c in PLAN_CASES])
    for (req, status, want), row in zip(PLAN_CASES, rows):
        assert row[0] == "plan" and int(row[1]) == status, (req, row)
        if status:
            for n in want:
                assert n in row[8], (req, n, row)
            continue
        assert tuple(int(v) for v in row[2:7]) == want and row[8] == "", (req, row)
        stage, shapes = want[0], want[1]
        pairs = [m.split(":") for m in row[7].split(",")] if row[7] else []
        assert len(pairs) == (int(req.split()[10]) if stage else 0), (req, row)
        for got, single in pairs:
            # a ragged table's record carries the margin of the single call on that frame's grid, bit for bit; any other table
            # goes up as the caller wrote it (the probe's reserved[2] is 0x7fc00000)
            assert got == (single if shapes else "7fc00000"), (req, row)
    assert {c[1] for c in PLAN_CASES} == {0, -1, -4}
