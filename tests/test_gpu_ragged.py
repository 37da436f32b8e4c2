"""GPU tests of the ragged batch: frames that differ in image size through esac_hip_forward_batch_shapes
(`Engine.forward_batch(shapes=)`, `esac.forward_batch(shapes=)`, `esac.forward_batch_async(shapes=)`, `harness.evaluate`).

Contract: frame b of a ragged batch is what the single call computes on that frame alone -- its own [E,3,h_b,w_b] maps, its
camera, the RNG counter call + b.  Every frame is checked against the CPU oracle run on that frame's grid; the bars are those of
tests/test_gpu_semantics.py and tests/test_gpu_edge.py, restated: tries, sampled cells, winner, expert, inlier counts, steps and
LM iterations equal; scores in reference arithmetic within 1e-12 relative of the oracle's on the same hypotheses; the pose
within 1e-4 rad / 1e-3 m.

Frames: `synthetic.make_frame(700 + b, H=h, W=w)` with the principal point at the image centre, seed 1305, counters from 60.
The shapes are the smallest that reach each route: 1280 cells of capacity for the teams (>= ESAC_REFINE_TEAM_MIN_CELLS = 1024;
the 30x30 frame is below it, the 24x41 frame has a width that is no multiple of 4), 320 for one workgroup per frame (33 frames:
beyond ESAC_TEAM_BATCH_MAX), 8448 for the global correspondence list (> ESAC_REFINE_LDS_CAP = 8192) next to a frame far below it.
"""
import io

import numpy as np
import pytest
import torch

import esac
from esac_amd import api, harness
from esac_amd import synthetic as S
from tests.test_eval_math_host import BAR, FIGURES

pytestmark = pytest.mark.gpu

SEED, CALL0, SUB = 1305, 60, 8
ROT_TOL, TRANS_TOL = 1e-4, 1e-3
TEAM_SHAPES = [(32, 40), (40, 32), (24, 41), (30, 30)]
FRAME_BUFS = (api.BUF_TRIES, api.BUF_SAMPLE_XY, api.BUF_INLIER_COUNTS, api.BUF_HYPS, api.BUF_SCORES)
DISCRETE = (api.RES_HYP, api.RES_EXPERT, api.RES_REF_STEPS, api.RES_INLIERS, api.RES_LM_ITERS, api.RES_CONTENDERS)

_cache = {}


def _inputs(shapes, E, N, mode="gating", first=700):
    """(frames, assignments) of a case, made once (the references below are shared the same way and never written to)."""
    key = (tuple(shapes), E, N, mode, first)
    if key not in _cache:
        frames = [S.make_frame(first + b, E=E, true_expert=b % E, H=h, W=w, sub=SUB, ppx=w * SUB / 2.0, ppy=h * SUB / 2.0,
                               focal=525.0 + 10.0 * (b % 5), shift=(b % 3 - 1, (b % 2) * 2 - 1)) for b, (h, w) in enumerate(shapes)]
        has = [S.gating_assignment(f, N, mode=mode) for f in frames]
        _cache[key] = (frames, has, {})
    return _cache[key]


def _cams(frames):
    cams = api.make_cams([f["shift"][0] for f in frames], [f["shift"][1] for f in frames], [f["focal"] for f in frames],
                         [f["ppx"] for f in frames], [f["ppy"] for f in frames])
    cams["reserved"][:] = -12345  # (the padding of a camera table may hold anything: forward_batch(shapes=) fills its copy)
    return cams


def _oracle(oracle, refs, frames, has, b, call0=CALL0, in_hyps=None):
    f = frames[b]
    kw = dict(shift_x=f["shift"][0], shift_y=f["shift"][1], focal=f["focal"], ppx=f["ppx"], ppy=f["ppy"], sub_sampling=SUB,
              seed=SEED, call=call0 + b)
    if in_hyps is not None:
        return oracle.forward(f["coords"], has[b], in_hyps=in_hyps, **kw)
    if (b, call0) not in refs:
        refs[(b, call0)] = oracle.forward(f["coords"], has[b], **kw)
    return refs[(b, call0)]


def _params(engine, E, H, W, N, call, **kw):
    """Parameter block of a batch with a table: the five camera fields are ignored, so they carry values no frame uses."""
    return engine.make_params(E, H, W, N, shift_x=-77, shift_y=91, focal=1234.5, ppx=-5.0, ppy=9999.0, sub_sampling=SUB, seed=SEED,
                              call=call, **kw)


def _run(engine, frames, has, call0=CALL0, tail=0.0, **kw):
    """The frames as ONE ragged batch.  tail: what the unused end of every slot holds."""
    B, N, E = len(frames), len(has[0]), frames[0]["coords"].shape[0]
    packed, shapes = api.pack_frames([torch.from_numpy(f["coords"]) for f in frames], device=engine.device)
    assert shapes == [f["coords"].shape[2:] for f in frames] and packed.shape[1] % 4 == 0
    if tail != 0.0:
        for b, (h, w) in enumerate(shapes):
            packed[b, 3 * E * h * w:] = tail
    H, W = api.capacity_shape(shapes)
    scores = torch.empty(B, N, dtype=torch.float64, device="cuda")
    res = engine.forward_batch(packed, torch.from_numpy(np.stack(has)).cuda(), _params(engine, E, H, W, N, call0, **kw),
                               scores_out=scores, cams=_cams(frames), shapes=shapes)
    out = dict(res=res, scores=scores.cpu().numpy(), mode=engine.refine_info()["mode"])
    for which in FRAME_BUFS:
        out[which] = engine.read_forward_frames(which, B)
    return out


def _check_frame(oracle, refs, frames, has, out, b, call0=CALL0, all_scores=False):
    """Frame b of a batch result against the oracle on that frame's own grid."""
    ref = _oracle(oracle, refs, frames, has, b, call0)
    rec = out["res"][b]
    assert ref["ref_steps"] >= 1 and ref["inlier_map"].sum() > 0  # (a refined winner with a non-empty inlier set)
    np.testing.assert_array_equal(out[api.BUF_TRIES][b], ref["tries"], err_msg="frame %d" % b)
    np.testing.assert_array_equal(out[api.BUF_SAMPLE_XY][b], ref["sample_xy"], err_msg="frame %d" % b)
    assert int(rec[api.RES_HYP]) == ref["winner"] and int(rec[api.RES_EXPERT]) == ref["expert"], b
    np.testing.assert_array_equal(out[api.BUF_INLIER_COUNTS][b], ref["inlier_counts"], err_msg="frame %d" % b)
    assert int(rec[api.RES_REF_STEPS]) == ref["ref_steps"] and int(rec[api.RES_LM_ITERS]) == ref["lm_iters"], b
    np.testing.assert_allclose(out[api.BUF_HYPS][b], ref["hyps"], rtol=0, atol=1e-6)
    # scores in reference arithmetic: against the oracle's score OF THE SAME HYPOTHESIS (the device's hypotheses carry the device's
    # libm: the criterion of test_exact_scores_all) -- the winner's always (its score is exact on every route), all N on the exact routes
    same = _oracle(oracle, refs, frames, has, b, call0, in_hyps=out[api.BUF_HYPS][b])
    w = ref["winner"]
    worst = float(np.abs(out["scores"][b] / same["scores"] - 1.0).max()) if all_scores else abs(rec[api.RES_SCORE] / same["scores"][w] - 1.0)
    r, t = S.pose_errors(rec[api.RES_POSE:api.RES_POSE + 16].reshape(4, 4), ref["pose"])
    print("frame %d (%dx%d): winner %d, %d steps, score rel. diff %.2e (%s), pose %.2e rad %.2e m"
          % ((b,) + frames[b]["coords"].shape[2:] + (w, ref["ref_steps"], worst, "all" if all_scores else "winner", r, t)))
    np.testing.assert_allclose(rec[api.RES_SCORE], same["scores"][w], rtol=1e-12, atol=1e-11)
    assert rec[api.RES_SCORE] == out["scores"][b][w]
    if all_scores:
        np.testing.assert_allclose(out["scores"][b], same["scores"], rtol=1e-12, atol=1e-11)
    assert r <= ROT_TOL and t <= TRANS_TOL, (b, r, t)


def _assert_same_bits(a, b, what):
    np.testing.assert_array_equal(a["res"], b["res"], err_msg=what)
    np.testing.assert_array_equal(a["scores"], b["scores"], err_msg=what)
    for which in FRAME_BUFS:
        np.testing.assert_array_equal(a[which], b[which], err_msg="%s buffer %d" % (what, which))
    assert a["mode"] == b["mode"]


# ---------------------------------------------------------------- 1. a uniform table is the old batch
@pytest.mark.parametrize("B, E, N, shape, mode", [(3, 2, 32, (32, 40), "team"), (33, 1, 16, (16, 20), "one_workgroup")])
def test_uniform_table_is_forward_batch_cams_bit_for_bit(engine, B, E, N, shape, mode):
    frames, has, _ = _inputs([shape] * B, E, N)
    new = _run(engine, frames, has)
    coords = torch.from_numpy(np.stack([f["coords"] for f in frames])).cuda()
    scores = torch.empty(B, N, dtype=torch.float64, device="cuda")
    res = engine.forward_batch(coords, torch.from_numpy(np.stack(has)).cuda(), _params(engine, E, shape[0], shape[1], N, CALL0),
                               scores_out=scores, cams=_cams(frames))
    old = dict(res=res, scores=scores.cpu().numpy(), mode=engine.refine_info()["mode"])
    for which in FRAME_BUFS:
        old[which] = engine.read_forward_frames(which, B)
    assert old["mode"] == mode
    _assert_same_bits(new, old, "uniform %dx%d" % shape)
    assert (res[:, api.RES_REF_STEPS] >= 1).all()


# ---------------------------------------------------------------- 2. mixed shapes, team route
def test_mixed_shapes_on_the_team_route_oracle_and_single_calls(engine, oracle):
    frames, has, refs = _inputs(TEAM_SHAPES, 3, 64)
    out = _run(engine, frames, has)
    assert out["mode"] == "team"
    for b in range(4):
        _check_frame(oracle, refs, frames, has, out, b)
    # ... and against the single call on the device: the discrete outputs and the number of contenders (the band of the re-score
    # is the frame's own: a margin taken from the capacity of 1280 cells would be narrower than the 900-cell frame's)
    for b, f in enumerate(frames):
        E, _, h, w = f["coords"].shape
        p = engine.make_params(E, h, w, 64, shift_x=f["shift"][0], shift_y=f["shift"][1], focal=f["focal"], ppx=f["ppx"], ppy=f["ppy"],
                               sub_sampling=SUB, seed=SEED, call=CALL0 + b)
        s1 = torch.empty(64, dtype=torch.float64, device="cuda")
        r1 = engine.forward_device(torch.from_numpy(f["coords"]).cuda(), torch.from_numpy(has[b]).cuda(), p, scores_out=s1)
        print("frame %d: single call on %s, %d contenders (batch %d)" % (b, engine.refine_info()["mode"], int(r1[api.RES_CONTENDERS]),
                                                                       int(out["res"][b][api.RES_CONTENDERS])))
        for field in DISCRETE:
            assert out["res"][b][field] == r1[field], (b, field, out["res"][b][field], r1[field])
        np.testing.assert_array_equal(engine.read(api.BUF_TRIES), out[api.BUF_TRIES][b])
        np.testing.assert_array_equal(engine.read(api.BUF_SAMPLE_XY), out[api.BUF_SAMPLE_XY][b])
        np.testing.assert_array_equal(engine.read(api.BUF_INLIER_COUNTS), out[api.BUF_INLIER_COUNTS][b])
        np.testing.assert_allclose(out["res"][b][:31], r1[:31], rtol=0, atol=1e-8)   # (the bar between two refinement routes)
        r, t = S.pose_errors(out["res"][b][api.RES_POSE:api.RES_POSE + 16].reshape(4, 4), r1[api.RES_POSE:api.RES_POSE + 16].reshape(4, 4))
        assert r <= ROT_TOL and t <= TRANS_TOL, (b, r, t)


# ---------------------------------------------------------------- 3. mixed shapes, one workgroup per frame
def test_mixed_shapes_one_workgroup_per_frame(engine, oracle):
    shapes = [[(16, 20), (20, 16), (12, 25)][b % 3] for b in range(33)]
    frames, has, refs = _inputs(shapes, 2, 16, first=740)
    out = _run(engine, frames, has)
    assert out["mode"] == "one_workgroup"
    for b in range(33):
        _check_frame(oracle, refs, frames, has, out, b)


# ---------------------------------------------------------------- 4. mixed shapes, global correspondence list
def test_mixed_shapes_on_the_global_list_route(engine, oracle):
    frames, has, refs = _inputs([(96, 88), (60, 80)], 1, 16, first=780)
    out = _run(engine, frames, has)
    # 8448 cells: beyond what a team of 8 holds (8 x 4 cells per lane x 256 lanes = 8192) and beyond ESAC_REFINE_LDS_CAP, so one
    # workgroup per frame with the list in global memory (refine_info names the route, not where the list lives)
    assert out["mode"] == "one_workgroup" and 96 * 88 > 8192
    for b in range(2):
        _check_frame(oracle, refs, frames, has, out, b)


# ---------------------------------------------------------------- 4b. reading frame 0's inlier map back
@pytest.mark.parametrize("first, buf", [(842, 1), (845, 0)], ids=["two_accepted_steps", "three_accepted_steps"])
def test_inlier_map_of_frame_0_after_a_ragged_batch(engine, oracle, first, buf):
    """esac_hip_read(ESAC_BUF_INLIER_MAP) after a ragged batch on the one-workgroup route, frame 0 (12x25 = 300 cells) below the
    capacity of 320: the accepted inlier set is the first h_0 * w_0 entries of the read.  k_refine alternates two map buffers that
    lie P cells apart with the P of the frame's OWN grid; the winner of frame `first` has an even number of accepted re-fits on the
    oracle (its set is in the second buffer), the other an odd number (the first)."""
    shapes = [(12, 25), (16, 20), (20, 16)]
    frames, has, refs = _inputs(shapes, 2, 16, first=first)
    ref = _oracle(oracle, refs, frames, has, 0)
    assert ref["ref_steps"] >= 2 and ref["ref_steps"] % 2 == 1 - buf and 0 < ref["inlier_map"].sum() < 300
    out = _run(engine, frames, has)
    assert out["mode"] == "one_workgroup" and api.capacity_shape(shapes) == (16, 20)
    assert int(engine.read(api.BUF_RESULT)[31]) == buf  # (the workspace record of frame 0 names the buffer)
    got = engine.read(api.BUF_INLIER_MAP)  # [16,20]: frame 0's slot at the capacity's size
    np.testing.assert_array_equal(got.reshape(-1)[:300].reshape(12, 25), ref["inlier_map"])
    _check_frame(oracle, refs, frames, has, out, 0)


# ---------------------------------------------------------------- 5. the slot's tail is never read
def test_the_tail_of_a_slot_is_never_read(engine):
    frames, has, _ = _inputs(TEAM_SHAPES, 3, 64)
    zero = _run(engine, frames, has)
    nan = _run(engine, frames, has, tail=float("nan"))
    _assert_same_bits(nan, zero, "NaN tail")
    assert np.isfinite(zero["scores"]).all() and np.isfinite(zero["res"]).all() and (zero["res"][:, api.RES_REF_STEPS] >= 1).all()


def test_a_ragged_batch_of_one_frame_is_the_single_call(engine):
    """B = 1: the 30x30 frame in a slot and under a capacity sized for 32x40 is the single call on 30x30, bit for bit."""
    frames, has, _ = _inputs(TEAM_SHAPES, 3, 64)
    f, ha = frames[3], torch.from_numpy(has[3]).cuda()
    packed = torch.full((1, api.packed_stride(3, TEAM_SHAPES)), float("nan"), device="cuda")
    packed[0, :3 * 3 * 900] = torch.from_numpy(f["coords"]).cuda().reshape(-1)
    s_new, s_old = torch.empty(1, 64, dtype=torch.float64, device="cuda"), torch.empty(64, dtype=torch.float64, device="cuda")
    new = engine.forward_batch(packed, ha[None], _params(engine, 3, 32, 40, 64, CALL0 + 3), scores_out=s_new, cams=_cams([f]), shapes=[(30, 30)])
    tries = engine.read(api.BUF_TRIES)
    p = engine.make_params(3, 30, 30, 64, shift_x=f["shift"][0], shift_y=f["shift"][1], focal=f["focal"], ppx=f["ppx"], ppy=f["ppy"],
                           sub_sampling=SUB, seed=SEED, call=CALL0 + 3)
    old = engine.forward_device(torch.from_numpy(f["coords"]).cuda(), ha, p, scores_out=s_old)
    np.testing.assert_array_equal(new[0], old)
    np.testing.assert_array_equal(s_new.cpu().numpy()[0], s_old.cpu().numpy())
    np.testing.assert_array_equal(tries, engine.read(api.BUF_TRIES))


# ---------------------------------------------------------------- 6. exact scores and strict reference
@pytest.mark.parametrize("kw", [dict(exact_scores=True), dict(strict_reference=True)], ids=["exact_scores", "strict_reference"])
def test_mixed_shapes_exact_scores_every_hypothesis(engine, oracle, kw):
    frames, has, refs = _inputs(TEAM_SHAPES, 3, 64)
    out = _run(engine, frames, has, **kw)
    for b in range(4):
        _check_frame(oracle, refs, frames, has, out, b, all_scores=True)
        assert int(out["res"][b][api.RES_CONTENDERS]) == 64


# ---------------------------------------------------------------- 7. asynchronous call, evaluation, harness
def test_async_call_and_eval_batch_give_the_blocking_calls_records(engine):
    frames, has, _ = _inputs(TEAM_SHAPES, 3, 64)
    maps = [torch.from_numpy(f["coords"]).cuda() for f in frames]
    ha = torch.from_numpy(np.stack(has)).cuda()
    cam = ([f["shift"][0] for f in frames], [f["shift"][1] for f in frames], [f["focal"] for f in frames], [f["ppx"] for f in frames],
           [f["ppy"] for f in frames])
    solver = (10.0, 100.0, 0.5, 100.0, SUB)
    esac.set_seed(SEED, CALL0)
    poses = torch.zeros(4, 4, 4)
    experts = esac.forward_batch(maps, ha, poses, *cam, *solver, shapes=TEAM_SHAPES)
    blocking = esac.last_result()["result"].copy()
    blocking_scores = esac.last_result()["scores"].cpu().numpy().copy()
    assert esac.get_rng_state() == (SEED, CALL0 + 4) and experts == [int(v) for v in blocking[:, api.RES_EXPERT]]
    # the same batch through the engine (test 2's call): the module-level call is that call
    np.testing.assert_array_equal(blocking, _run(engine, frames, has)["res"])
    esac.set_seed(SEED, CALL0)
    packed, shapes = esac.pack_frames(maps)
    fwd = esac.forward_batch_async(packed, ha, *cam, *solver, shapes=shapes)
    gts = np.stack([f["gt_pose"] for f in frames]).astype(np.float32)
    ge = np.array([b % 3 for b in range(4)], np.int64)
    rows = esac.eval_batch(fwd["records"], gts, ge).cpu().numpy()
    rec = fwd["records"].cpu().numpy()
    assert fwd["call"] == CALL0 and esac.get_rng_state() == (SEED, CALL0 + 4)
    np.testing.assert_array_equal(rec[:, :31], blocking[:, :31])
    assert (rec[:, api.RES_VALID] == 1.0).all()
    np.testing.assert_array_equal(fwd["scores"].cpu().numpy(), blocking_scores)
    assert esac.last_result() is fwd
    np.testing.assert_array_equal(poses.numpy(), rec[:, api.RES_POSE:api.RES_POSE + 16].astype(np.float32).reshape(4, 4, 4))
    for b in range(4):
        want = harness.eval_row_host(rec[b, api.RES_POSE:api.RES_POSE + 16].astype(np.float32).reshape(4, 4), gts[b],
                                     int(rec[b, api.RES_EXPERT]), int(rec[b, api.RES_HYP]), int(ge[b]))
        assert np.abs(rows[b, FIGURES] - want[FIGURES]).max() <= BAR, (b, rows[b], want)
        for col in (api.EVAL_POSE_OK, api.EVAL_CLASS_OK, api.EVAL_EXPERT, api.EVAL_HYP, api.EVAL_STATUS):
            assert rows[b, col] == want[col], (b, col, rows[b], want)
        assert rows[b, api.EVAL_POSE_OK] == 1.0 and rows[b, api.EVAL_CLASS_OK] == 1.0 and rows[b, api.EVAL_STATUS] == 0.0


@pytest.mark.parametrize("asynchronous", [False, True], ids=["blocking", "async"])
def test_a_table_the_library_refuses_draws_no_rng_stream(engine, asynchronous):
    """Frame 2 (24x41, sub 8: its last column's centre is 324 - shiftX) gets a shift its own 41 columns overflow int32 with, while
    the 40 columns of the capacity shape would hold it: the library names the frame, and the module's call counter stays."""
    frames, has, _ = _inputs(TEAM_SHAPES, 3, 64)
    maps = [torch.from_numpy(f["coords"]).cuda() for f in frames]
    ha = torch.from_numpy(np.stack(has)).cuda()
    shift_x = [0, 0, -(2**31 - 1 - 316), 0]
    esac.set_seed(SEED, 77)
    with pytest.raises(RuntimeError, match="pixel positions overflow int32.*in frame 2"):
        if asynchronous:
            esac.forward_batch_async(maps, ha, shift_x, 0, 525.0, 160.0, 128.0, 10.0, 100.0, 0.5, 100.0, SUB, shapes=TEAM_SHAPES)
        else:
            esac.forward_batch(maps, ha, torch.zeros(4, 4, 4), shift_x, 0, 525.0, 160.0, 128.0, 10.0, 100.0, 0.5, 100.0, SUB, shapes=TEAM_SHAPES)
    assert esac.get_rng_state() == (SEED, 77)


class _TaggedExpert(torch.nn.Module):
    """An image carries its frame number; the frame's map is looked up on the device (maps of one group have one size)."""
    def __init__(self, maps, e):
        super().__init__()
        self.maps, self.e = maps, e

    def forward(self, images):
        return torch.stack([self.maps[int(k)][self.e] for k in images[:, 0, 0, 0].tolist()])


class _TaggedGating(torch.nn.Module):
    def __init__(self, log_gating):
        super().__init__()
        self.log_gating = log_gating

    def forward(self, images):
        return self.log_gating[images[:, 0, 0, 0].long()]


def test_evaluate_in_ragged_batches_gives_the_rows_of_single_calls(engine):
    """Eight images of two sizes, landscape 480x640 and portrait 640x480 alternating in pairs, E = 2 with an oracle expert per
    run: evaluate(batch_size=4) forms two ragged batches and must report what batch_size=1 (eight blocking esac.forward calls at
    the same keys) reports -- the same experts, pose errors within 0.01 deg / 0.1 cm (1e-4 rad / 1e-3 m in the loop's units)."""
    E, N = 2, 64
    sizes = [(60, 80) if (k // 2) % 2 == 0 else (80, 60) for k in range(8)]
    frames = [S.make_frame(800 + k, E=E, true_expert=1, H=h, W=w, ppx=w * 4.0, ppy=h * 4.0, focal=525.0 + 5.0 * k) for k, (h, w) in enumerate(sizes)]
    maps = [torch.from_numpy(f["coords"]).cuda() for f in frames]
    gating = _TaggedGating(torch.log_softmax(torch.zeros(8, E, device="cuda"), dim=1))
    experts = [_TaggedExpert(maps, e) for e in range(E)]
    samples = [("img%03d" % k, torch.full((1, 3, h * 8, w * 8), float(k), device="cuda"), f["focal"], f["gt_pose"], 1)
               for k, (f, (h, w)) in enumerate(zip(frames, sizes))]
    got = {}
    for bs in (4, 1):
        esac.set_seed(SEED, 90)
        log = io.StringIO()
        stats = harness.evaluate(iter(samples), gating, experts, pose_log=log, hypotheses=N, batch_size=bs, oracle_expert=1)
        assert esac.get_rng_state() == (SEED, 98) and stats["images"] == 8
        got[bs] = (stats, [l.split() for l in log.getvalue().splitlines()])
    (s4, l4), (s1, l1) = got[4], got[1]
    assert len(l4) == len(l1) == 8
    for a, b in zip(l4, l1):
        assert a[0] == b[0]
        np.testing.assert_allclose([float(v) for v in a[1:]], [float(v) for v in b[1:]], rtol=0, atol=1e-3)  # quaternion, translation [m]
    for ra, rb in zip(s4["scenes"], s1["scenes"]):
        assert ra["class_acc"] == rb["class_acc"] and ra["pose_acc"] == rb["pose_acc"], (ra, rb)
        assert abs(ra["median_rot_deg"] - rb["median_rot_deg"]) <= 0.01 and abs(ra["median_trans_cm"] - rb["median_trans_cm"]) <= 0.1, (ra, rb)
    assert s4["scenes"][1]["pose_acc"] == 1.0 and s4["scenes"][1]["class_acc"] == 1.0
    assert s4["avg_active"] == s1["avg_active"] == 1.0 and s4["max_active"] == s1["max_active"] == 1


def test_rerun_frames_uses_the_frames_own_maps_and_shape(engine):
    """rerun_frames on a ragged localize_batch result: the blocking single call with refine_solo on that frame's own grid."""
    sizes = [(60, 80), (80, 60), (60, 90)]
    frames = [S.make_frame(820 + k, H=h, W=w, ppx=w * 4.0, ppy=h * 4.0) for k, (h, w) in enumerate(sizes)]
    maps = [torch.from_numpy(f["coords"]).cuda() for f in frames]
    images = [torch.full((1, 3, h * 8, w * 8), float(k), device="cuda") for k, (h, w) in enumerate(sizes)]
    gating = _TaggedGating(torch.zeros(3, 1, device="cuda"))
    esac.set_seed(SEED, 120)
    out = harness.localize_batch(images, gating, [_TaggedExpert(maps, 0)], [f["focal"] for f in frames],
                                 gt_poses=np.stack([f["gt_pose"] for f in frames]).astype(np.float32), hypotheses=32)
    assert out["shapes"] == sizes and tuple(out["prediction"].shape) == (3, api.packed_stride(1, sizes))
    before = out["records_host"].copy()
    done = harness.rerun_frames(out, [2, 1])
    for b in (1, 2):
        h, w = sizes[b]
        p = engine.make_params(1, h, w, 32, focal=frames[b]["focal"], ppx=w * 4.0, ppy=h * 4.0, sub_sampling=8, seed=SEED, call=120 + b,
                               refine_solo=True)
        want = engine.forward_device(maps[b], torch.zeros(32, dtype=torch.int64, device="cuda"), p)
        np.testing.assert_array_equal(done[b]["record"], want)
        for field in DISCRETE:
            assert before[b][field] == want[field], (b, field)
        np.testing.assert_allclose(before[b][:31], want[:31], rtol=0, atol=1e-8)
