"""The batched evaluation path on the device: esac_hip_eval_batch against the harness's host functions, esac.forward_batch_async +
esac.eval_batch in stream order behind a late producer, harness.evaluate(batch_size=3) against single calls, rerun_frames.
Shapes: 60x80 maps (the smallest grid on which a batch refines with teams), 2 experts, 64 hypotheses.
The bar of the error figures is the one measured on the CPU (tests/test_eval_math_host.py: 8 x the worst host-vs-host difference)."""
import io
import math

import numpy as np
import pytest
import torch

from esac_amd import api, harness
from esac_amd import synthetic as S
from tests.test_eval_math_host import BAR, FIGURES

pytestmark = pytest.mark.gpu

E, N = 2, 64
SOLVER = (10.0, 100.0, 0.5, 100.0, 8)


def _rot(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + math.sin(angle) * K + (1 - math.cos(angle)) * (K @ K)


def _hand_made(B):
    """B records and ground truths: frame 0 at angle pi (exactly: a diagonal rotation against an identity ground truth), then --
    where the batch has room -- a NaN pose, VALID = 0, VALID = 3, and random float32 pose pairs up to B (a few degrees / cm apart,
    every fourth one far off)."""
    rng = np.random.default_rng(100 + B)
    rec = np.zeros((B, 32))
    gt = np.zeros((B, 4, 4), np.float32)
    for b in range(B):
        G = np.eye(4)
        G[:3, :3] = _rot(rng.normal(size=3), rng.uniform(0, math.pi))
        G[:3, 3] = rng.uniform(-3, 3, size=3)
        P = np.eye(4)
        far = b % 4 == 3
        P[:3, :3] = _rot(rng.normal(size=3), rng.uniform(0, 3.0 if far else 0.05)) @ G[:3, :3]
        P[:3, 3] = G[:3, 3] + rng.uniform(-1, 1, size=3) * (0.5 if far else 0.03)
        if b == 0:
            G = np.eye(4)
            G[:3, 3] = [0.5, -1.25, 2.0]
            P = G.copy()
            P[:3, :3] = np.diag([1.0, -1.0, -1.0])  # pi about x
        gt[b] = G.astype(np.float32)
        rec[b, api.RES_POSE:api.RES_POSE + 16] = P.astype(np.float32).reshape(16)
        rec[b, api.RES_SCORE], rec[b, api.RES_HYP], rec[b, api.RES_EXPERT], rec[b, api.RES_VALID] = 10.0 + b, (7 * b) % N, b % E, 1.0
    if B >= 5:
        rec[1, api.RES_POSE:api.RES_POSE + 16] = np.nan
        rec[2, api.RES_VALID] = 0.0
        rec[3, api.RES_VALID] = 3.0
    if B > 64:
        rec[63, api.RES_VALID] = 3.0  # the last lane of the first workgroup
    return rec, gt, np.array([(b + b // 3) % E for b in range(B)], np.int64)


def _want_rows(rec, gt, ge, rot=5.0, trans=5.0):
    rows = np.zeros((len(rec), 16))
    for b in range(len(rec)):
        g = None if ge is None else int(ge[b])
        if rec[b, api.RES_VALID] == 1.0:
            rows[b] = harness.eval_row_host(rec[b, api.RES_POSE:api.RES_POSE + 16].astype(np.float32).reshape(4, 4), gt[b],
                                            int(rec[b, api.RES_EXPERT]), int(rec[b, api.RES_HYP]), g, rot, trans)
        else:
            rows[b, FIGURES] = np.nan
            rows[b, api.EVAL_CLASS_OK] = -1.0 if g is None else 0.0
            rows[b, api.EVAL_EXPERT], rows[b, api.EVAL_HYP] = rec[b, api.RES_EXPERT], rec[b, api.RES_HYP]
            rows[b, api.EVAL_STATUS] = 3.0 if rec[b, api.RES_VALID] == 3.0 else 1.0
    return rows


def _assert_rows(got, want, what):
    assert got.shape == want.shape
    for b in range(len(want)):
        np.testing.assert_array_equal(np.isnan(got[b]), np.isnan(want[b]), err_msg="%s frame %d: NaN pattern" % (what, b))
        diff = np.nan_to_num(np.abs(got[b, FIGURES] - want[b, FIGURES]))
        assert diff.max() <= BAR, (what, b, got[b], want[b])
        for col in (api.EVAL_POSE_OK, api.EVAL_CLASS_OK, api.EVAL_EXPERT, api.EVAL_HYP, api.EVAL_STATUS, 14, 15):
            assert got[b, col] == want[b, col], (what, b, col, got[b], want[b])
    return float(np.nan_to_num(np.abs(got[:, FIGURES] - want[:, FIGURES])).max())


@pytest.mark.parametrize("with_experts", [True, False], ids=["gt_experts", "no_gt_experts"])
@pytest.mark.parametrize("B", [1, 5, 65])
def test_kernel_against_the_host_functions_on_hand_made_records(engine, B, with_experts):
    """One lane, a partial wavefront, a second workgroup.  Every column of every row is written, nothing beyond row B - 1."""
    rec, gt, ge = _hand_made(B)
    d_rec = torch.from_numpy(rec).cuda()
    out = torch.full((B + 1, 16), -7.0, dtype=torch.float64, device="cuda")
    got = engine.eval_batch(d_rec, torch.from_numpy(gt).cuda(), torch.from_numpy(ge).cuda() if with_experts else None, out=out[:B])
    assert got.data_ptr() == out.data_ptr()
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    np.testing.assert_array_equal(host[B], np.full(16, -7.0))
    worst = _assert_rows(host[:B], _want_rows(rec, gt, ge if with_experts else None), "B=%d" % B)
    print("B=%d: worst absolute difference to the host functions %.3e (bar %.3e)" % (B, worst, BAR))
    assert host[0, api.EVAL_STATUS] == 0.0 and abs(host[0, api.EVAL_ROT_DEG] - 180.0) < 1e-9  # the frame at pi
    if B >= 5:
        assert host[1, api.EVAL_STATUS] == 0.0 and math.isnan(host[1, api.EVAL_ROT_DEG]) and host[1, api.EVAL_POSE_OK] == 0.0
        assert host[2, api.EVAL_STATUS] == 1.0 and host[3, api.EVAL_STATUS] == 3.0
        assert harness.frames_to_rerun(host[:B]) == ([3, 63] if B > 64 else [3])
        assert (host[:B, api.EVAL_POSE_OK] == 0).sum() >= 3 and (B < 65 or host[:B, api.EVAL_POSE_OK].sum() >= 1)


def test_module_call_uploads_host_ground_truth_and_honours_thresholds(engine):
    """esac.eval_batch with numpy ground truth (uploaded asynchronously) and thresholds of its own; the library's argument errors."""
    import esac
    rec, gt, ge = _hand_made(5)
    d_rec = torch.from_numpy(rec).cuda()
    got = esac.eval_batch(d_rec, gt, ge.tolist(), rotThreshold=1.0, transThreshold=2.5)
    torch.cuda.synchronize()
    _assert_rows(got.cpu().numpy(), _want_rows(rec, gt, ge, 1.0, 2.5), "thresholds 1 deg / 2.5 cm")
    loose = esac.eval_batch(d_rec, torch.from_numpy(gt), None, rotThreshold=200.0, transThreshold=1e4).cpu().numpy()
    assert loose[[0, 4], api.EVAL_POSE_OK].tolist() == [1.0, 1.0] and loose[[1, 2, 3], api.EVAL_POSE_OK].tolist() == [0.0, 0.0, 0.0]
    assert (loose[:, api.EVAL_CLASS_OK] == -1.0).all()
    lib, out = engine.lib, torch.zeros(5, 16, dtype=torch.float64, device="cuda")
    d_gt = torch.from_numpy(gt).cuda()
    stream = torch.cuda.current_stream().cuda_stream
    for args in ((0, d_rec.data_ptr(), d_gt.data_ptr(), None, 5.0, 5.0, stream, out.data_ptr()),
                 (1025, d_rec.data_ptr(), d_gt.data_ptr(), None, 5.0, 5.0, stream, out.data_ptr()),
                 (5, None, d_gt.data_ptr(), None, 5.0, 5.0, stream, out.data_ptr()),
                 (5, d_rec.data_ptr(), None, None, 5.0, 5.0, stream, out.data_ptr()),
                 (5, d_rec.data_ptr(), d_gt.data_ptr(), None, 5.0, 5.0, stream, None),
                 (5, d_rec.data_ptr(), d_gt.data_ptr(), None, -1.0, 5.0, stream, out.data_ptr()),
                 (5, d_rec.data_ptr(), d_gt.data_ptr(), None, 5.0, float("nan"), stream, out.data_ptr()),
                 (5, d_rec.data_ptr(), d_gt.data_ptr(), None, float("inf"), 5.0, stream, out.data_ptr())):
        assert lib.esac_hip_eval_batch(engine.ctx, *args) == -4, args
        assert b"esac_hip_eval_batch" in lib.esac_hip_last_error()
    torch.cuda.synchronize()
    assert float(out.abs().max()) == 0.0  # nothing was launched


def _batch(first, B):
    frames = [S.make_frame(first + b, E=E, true_expert=b % E, focal=(525.0, 585.0, 480.0)[b % 3]) for b in range(B)]
    has = np.stack([S.gating_assignment(f, N, mode="gating") for f in frames])
    coords = np.stack([f["coords"] for f in frames])
    gts = np.stack([f["gt_pose"] for f in frames]).astype(np.float32)
    return frames, coords, has, gts


@pytest.mark.parametrize("B", [3, 33], ids=["B3_teams", "B33_one_workgroup"])
def test_async_batch_and_eval_in_stream_order_behind_a_late_producer(engine, B):
    """forward_batch_async and eval_batch enqueued back to back behind a producer that is still running on the stream (the hold +
    the copy that makes the coordinates real, tests/test_gpu_stream_order.py): the rows equal a blocking esac.forward_batch at the
    same (seed, call) followed by the host functions.  Until the copy runs, frame b's maps are frame b - 1's."""
    import esac
    from tests.test_gpu_stream_order import _bound_ms, _produce
    frames, coords, has, gts = _batch(5000 + 100 * B, B)
    focals = [f["focal"] for f in frames]
    ge = np.array([f["true_expert"] for f in frames], np.int64)
    real, ha = torch.from_numpy(coords).cuda(), torch.from_numpy(has).cuda()
    cam = (0, 0, focals, 320.0, 240.0)
    poses = torch.zeros(B, 4, 4)
    esac.set_seed(1305, 700)
    experts = esac.forward_batch(real, ha, poses, *(cam + SOLVER))
    want_rec = esac.last_result()["result"].copy()
    want_scores = esac.last_result()["scores"].cpu().numpy()
    want_rec[:, api.RES_VALID] = 1.0  # (the host copy carries another value in this slot)
    want = _want_rows(want_rec, gts, ge)
    assert experts == [int(v) for v in want[:, api.EVAL_EXPERT]]
    sc = torch.roll(real, 1, 0).contiguous()
    d_gt, d_ge = torch.from_numpy(gts).cuda(), torch.from_numpy(ge).cuda()
    esac.set_seed(1305, 700)
    torch.cuda.synchronize()
    _produce(sc, real, 1.5 * _bound_ms())
    out = esac.forward_batch_async(sc, ha, *(cam + SOLVER))
    rows = esac.eval_batch(out["records"], d_gt, d_ge)
    assert esac.last_result() is out and out["call"] == 700 and out["seed"] == 1305 and esac.get_rng_state() == (1305, 700 + B)
    torch.cuda.synchronize()
    engine.check()
    assert torch.equal(sc, real)
    got_rec, got = out["records"].cpu().numpy(), rows.cpu().numpy()
    assert (got_rec[:, api.RES_VALID] == 1.0).all(), got_rec[:, api.RES_VALID]
    for col in (api.RES_HYP, api.RES_EXPERT):
        np.testing.assert_array_equal(got_rec[:, col], want_rec[:, col])
    np.testing.assert_array_equal(out["scores"].cpu().numpy(), want_scores)
    worst = _assert_rows(got, want, "B=%d behind the producer" % B)
    print("B=%d: worst absolute difference to blocking batch + host functions %.3e (bar %.3e)" % (B, worst, BAR))
    assert got[:, api.EVAL_CLASS_OK].sum() >= B // 2 and got[:, api.EVAL_POSE_OK].sum() >= B // 2  # (real localisations, not zeros)


class _TaggedExpert(torch.nn.Module):
    """The _SyntheticExpert of tests/test_harness.py for batches: an image carries its frame number, the map is looked up on the device."""
    def __init__(self, maps, e):
        super().__init__()
        self.maps, self.e = maps, e

    def forward(self, images):
        return self.maps[images[:, 0, 0, 0].long(), self.e]


class _TaggedGating(torch.nn.Module):
    def __init__(self, log_gating):
        super().__init__()
        self.log_gating = log_gating

    def forward(self, images):
        return self.log_gating[images[:, 0, 0, 0].long()]


def _eight_samples():
    """The eight synthetic samples of tests/test_harness.py (frames 200..207, the true expert's logit 4 against -4), E = 2."""
    frames = [S.make_frame(200 + k, E=E, true_expert=k % E) for k in range(8)]
    maps = torch.from_numpy(np.stack([f["coords"] for f in frames])).cuda()
    logits = torch.full((8, E), -4.0, device="cuda")
    for k in range(8):
        logits[k, k % E] = 4.0
    gating = _TaggedGating(torch.log_softmax(logits, dim=1))
    experts = [_TaggedExpert(maps, e) for e in range(E)]
    samples = [("img%03d" % k, torch.full((1, 3, 480, 640), float(k), device="cuda"), f["focal"], f["gt_pose"], k % E)
               for k, f in enumerate(frames)]
    return frames, gating, experts, samples


@pytest.mark.parametrize("asynchronous", [False, True], ids=["blocking", "asynchronous"])
def test_evaluate_in_batches_of_three_against_single_calls(engine, monkeypatch, asynchronous):
    """evaluate(batch_size=3): batches of 3, 3 and 2.  Every frame replayed as a single esac.forward at its (seed, call + b) with the
    batch's own prediction and e_hyps: the expert identical, the errors within 0.01 deg / 0.1 cm of the single call's (the
    project's parity bar of 1e-4 rad / 1e-3 m in these units); class_acc == pose_acc == 1, eight pose-log lines, each
    character-equal to pose_file_line of the batch's own pose."""
    import esac
    frames, gating, experts, samples = _eight_samples()
    kept, original = [], harness.localize_batch

    def keeping(*a, **k):
        kept.append(original(*a, **k))
        return kept[-1]

    monkeypatch.setattr(harness, "localize_batch", keeping)
    esac.set_seed(1305, 40)
    log = io.StringIO()
    out = harness.evaluate(iter(samples), gating, experts, pose_log=log, hypotheses=N, generator=torch.Generator(device="cuda").manual_seed(5),
                           batch_size=3, asynchronous=asynchronous)
    assert [int(b["records"].shape[0]) for b in kept] == [3, 3, 2] and [b["call"] for b in kept] == [40, 43, 46]
    assert esac.get_rng_state() == (1305, 48)
    assert out["images"] == 8 and 1 <= out["avg_active"] <= E and 1 <= out["max_active"] <= E and out["avg_time_s"] > 0
    for row in out["scenes"]:
        assert row["class_acc"] == 1.0 and row["pose_acc"] == 1.0
        assert row["median_rot_deg"] < 1.0 and row["median_trans_cm"] < 3.0
    lines = log.getvalue().splitlines(keepends=True)
    assert len(lines) == 8
    k = 0
    for batch in kept:
        rec = batch["records"].cpu().numpy()
        rows = batch["eval"] if isinstance(batch["eval"], np.ndarray) else batch["eval"].cpu().numpy()
        assert (rows[:, api.EVAL_STATUS] == 0.0).all()
        for b in range(len(rec)):
            f = frames[k]
            own = rec[b, api.RES_POSE:api.RES_POSE + 16].astype(np.float32).reshape(4, 4)
            assert lines[k] == harness.pose_file_line("img%03d" % k, own), k
            pose = torch.zeros(4, 4)
            esac.set_seed(batch["seed"], batch["call"] + b)
            expert = esac.forward(batch["prediction"][b], batch["e_hyps"][b], pose, 0, 0, f["focal"], 320.0, 240.0, *SOLVER)
            assert expert == int(rows[b, api.EVAL_EXPERT]) == int(rec[b, api.RES_EXPERT]) == k % E, k
            assert esac.last_result()["winner"] == int(rows[b, api.EVAL_HYP]), k
            r_single, t_single = harness.pose_errors_deg_cm(pose.numpy(), f["gt_pose"])
            assert abs(rows[b, api.EVAL_ROT_DEG] - r_single) <= 0.01 and abs(rows[b, api.EVAL_TRANS_CM] - t_single) <= 0.1, (k, rows[b], r_single, t_single)
            assert rows[b, api.EVAL_CLASS_OK] == 1.0 and rows[b, api.EVAL_POSE_OK] == 1.0
            k += 1
    assert k == 8


def test_rerun_frames_equals_the_blocking_single_call_with_refine_solo(engine):
    """One frame of a finished batch run again: the record of the blocking single call at (seed, call + b) with that frame's focal
    length and refine_solo; its eval row by the host functions; the batch's host entries updated.  (No time-out is provoked: the
    status-3 branch of the kernel is covered by the hand-made records.)"""
    import esac
    frames, gating, experts, samples = _eight_samples()
    images = torch.cat([s[1] for s in samples[:3]])
    gts = np.stack([f["gt_pose"] for f in frames[:3]]).astype(np.float32)
    focals = [525.0, 585.0, 480.0]
    esac.set_seed(1305, 90)
    out = harness.localize_batch(images, gating, experts, focals, gt_poses=gts, gt_experts=[0, 1, 0], hypotheses=N,
                                 generator=torch.Generator(device="cuda").manual_seed(9))
    assert out["call"] == 90 and out["experts"] == [0, 1, 0] and tuple(out["poses"].shape) == (3, 4, 4)
    assert out["eval"].shape == (3, 16) and (out["eval"][:, api.EVAL_STATUS] == 0.0).all() and out["active_experts"] == [int(v) for v in (out["e_hist"] > 0).sum(1).cpu()]
    before_pose, before_row = out["poses"][1].numpy().copy(), out["eval"][1].copy()
    counter = esac.get_rng_state()
    done = harness.rerun_frames(out, [1])
    assert esac.get_rng_state() == counter and list(done) == [1]
    p = engine.make_params(E, 60, 80, N, 0, 0, focals[1], 320.0, 240.0, *SOLVER, seed=1305, call=91, refine_solo=True)
    want = engine.forward_device(out["prediction"][1], out["e_hyps"][1], p)
    np.testing.assert_array_equal(done[1]["record"][:31], want[:31])
    pose = want[api.RES_POSE:api.RES_POSE + 16].astype(np.float32).reshape(4, 4)
    np.testing.assert_array_equal(done[1]["pose"], pose)
    np.testing.assert_array_equal(out["poses"][1].numpy(), pose)
    np.testing.assert_array_equal(done[1]["eval"], harness.eval_row_host(pose, gts[1], int(want[api.RES_EXPERT]), int(want[api.RES_HYP]), 1))
    np.testing.assert_array_equal(out["eval"][1], done[1]["eval"])
    # the same frame either way: winner and expert identical, the pose to the rounding of the LM sums (teams against one workgroup)
    assert done[1]["expert"] == 1 and done[1]["eval"][api.EVAL_HYP] == before_row[api.EVAL_HYP]
    r_err, t_err = S.pose_errors(pose, before_pose)
    assert r_err <= 1e-4 and t_err <= 1e-3, (r_err, t_err)
    with pytest.raises(RuntimeError, match="rerun_frames"):
        harness.rerun_frames(out, [3])


def test_asynchronous_localize_batch_returns_device_tensors_only(engine):
    """asynchronous=True, all_experts=True, device inputs: records, eval, e_hyps, prediction stay on the device, and the rows equal
    the blocking form's on the same draws and the same call counters."""
    import esac
    frames, gating, experts, samples = _eight_samples()
    images = torch.cat([s[1] for s in samples[:5]])
    gts = torch.from_numpy(np.stack([f["gt_pose"] for f in frames[:5]]).astype(np.float32)).cuda()
    ge = torch.tensor([0, 1, 0, 1, 0], device="cuda")
    focals = [f["focal"] for f in frames[:5]]
    esac.set_seed(1305, 120)
    blocking = harness.localize_batch(images, gating, experts, focals, gt_poses=gts, gt_experts=ge, hypotheses=N,
                                      generator=torch.Generator(device="cuda").manual_seed(3))
    esac.set_seed(1305, 120)
    out = harness.localize_batch(images, gating, experts, focals, gt_poses=gts, gt_experts=ge, hypotheses=N,
                                 generator=torch.Generator(device="cuda").manual_seed(3), asynchronous=True, all_experts=True)
    for key in ("records", "eval", "e_hyps", "prediction", "scores", "active_experts"):
        assert isinstance(out[key], torch.Tensor) and out[key].is_cuda, key
    assert "poses" not in out and out["call"] == 120
    torch.cuda.synchronize()
    assert torch.equal(out["e_hyps"], blocking["e_hyps"])
    np.testing.assert_array_equal(out["records"].cpu().numpy()[:, :31], blocking["records_host"][:, :31])
    np.testing.assert_array_equal(out["eval"].cpu().numpy(), blocking["eval"])
    assert harness.frames_to_rerun(out["eval"].cpu().numpy()) == []
