"""GPU tests of the asynchronous batched training call: esac_hip_backward_batch_dev through `Engine.backward_batch_async`,
`esac.backward_batch_async` and `harness.train_batch(asynchronous=True)`.

The inputs are built the way tests/test_gpu_backward_batch.py builds them (its helpers are imported, bars included).  The
reference of every comparison is the BLOCKING batch (`Engine.backward_batch`) on the same inputs and counters, on a context that
refines one workgroup per slot (ESAC_SLOT_TEAMS=0); every comparison first asserts that each frame selected at least one slot.
The asserted bar against the blocking call is the project's own (tests/test_gpu_backward.py): loss within 1e-7 relative,
gradient within 2e-6 of the frame's largest entry; what does not depend on the ground truth must be equal.  Where two
ASYNCHRONOUS runs are compared with each other (busy stream, chunking) the bar is equality.

Nothing here provokes a fault or a hang: every hold is bounded by hold_launch itself (200 ms).
"""
import contextlib
import ctypes as C

import numpy as np
import pytest
import torch

from esac_amd import api
from esac_amd import synthetic as S
from tests.test_gpu_backward_batch import GRAD_RTOL, LOSS_RTOL, _check_frame, _gt, _oracle, _params

pytestmark = pytest.mark.gpu

HOLD_MS = 50.0  # inside hold_launch's 200 ms limit
SHIFTS = [(0, 0), (4, -4), (-3, 2), (1, 4), (-4, -1), (2, 0), (0, -2), (3, 3)]
FOCALS = [525.0, 585.0, 480.0, 1050.0, 525.0, 700.0, 612.5, 560.0]
GT_FREE = (("probs", api.BUF_BWD_PROBS), ("refh", api.BUF_BWD_REF_HYPS), ("slots", api.BUF_BWD_SLOTS), ("info", api.BUF_BWD_SLOT_INFO))


@pytest.fixture(scope="module")
def solo():
    """A context that refines its slots with one workgroup each."""
    mp = pytest.MonkeyPatch()
    mp.setenv("ESAC_SLOT_TEAMS", "0")
    try:
        return api.Engine(0)
    finally:
        mp.undo()


_hold_fn = []


def _hold(ms):
    """Queues the sleeping wavefront (tests/native/filler.hip) on torch's current stream."""
    if not _hold_fn:
        from tests.native import build as nb
        lib = C.CDLL(nb.build_filler())
        lib.hold_launch.argtypes = [C.c_void_p, C.c_float]
        lib.hold_launch.restype = C.c_int
        _hold_fn.append(lib.hold_launch)
    rc = _hold_fn[0](C.c_void_p(torch.cuda.current_stream().cuda_stream), float(ms))
    assert rc == 0, "hold_launch(%g ms) answered %d" % (ms, rc)


def _on(stream):
    return torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext()


def _case(case, first=500, B=6):
    if case == "one_expert":
        frames = [S.make_frame(first + b) for b in range(B)]
        has = [S.gating_assignment(f, 96) for f in frames]
        alpha = 30.0
    else:
        frames = [S.make_frame(first + 20 + b, E=3, true_expert=b % 3) for b in range(B)]
        has = [S.gating_assignment(f, 64, mode="gating") for f in frames]
        alpha = 20.0
    gts = [_gt(f, first + 100 + b) for b, f in enumerate(frames)]
    return frames, has, gts, alpha


def _cam_case(first, B=6, E=3, N=64):
    frames = [S.make_frame(first + b, E=E, true_expert=b % E, shift=SHIFTS[b % 8], focal=FOCALS[b % 8]) for b in range(B)]
    has = [S.gating_assignment(f, N, mode="gating") for f in frames]
    gts = [_gt(f, first + 50 + b) for b, f in enumerate(frames)]
    cams = api.make_cams([f["shift"][0] for f in frames], [f["shift"][1] for f in frames], [f["focal"] for f in frames],
                         [f["ppx"] for f in frames], [f["ppy"] for f in frames])
    return frames, has, gts, cams


def _tensors(frames, has, shared=None, g0=None):
    sc = torch.from_numpy(shared if shared is not None else np.stack([f["coords"] for f in frames])).cuda()
    ha = torch.from_numpy(np.stack(has)).cuda()
    shape = (len(has),) + frames[0]["coords"].shape
    g = torch.from_numpy(g0.copy()).cuda() if g0 is not None else torch.zeros(shape, dtype=torch.float32, device="cuda")
    return sc, ha, g


def _buffers(eng, B, rec, with_losses=False):
    """The frames' buffers.  Of a frame's slot rows only the first rec[b,1] are defined (include/esac_hip.h: "first h_out[1]
    entries valid"; what lies behind them is whatever an earlier call left in the workspace): the rest is set to -1 here."""
    out = {key: eng.read_frames(buf, B) for key, buf in GT_FREE}
    for b in range(B):
        out["slots"][b, int(rec[b, 1]):] = -1
        out["info"][b, int(rec[b, 1]):] = -1
    if with_losses:
        out["losses"] = eng.read_frames(api.BUF_BWD_LOSSES, B)
    return out


def _blocking(eng, frames, has, gts, alpha, call0, shared=None, g0=None, cams=None, **pkw):
    sc, ha, g = _tensors(frames, has, shared, g0)
    p = _params(eng, frames[0], ha.shape[1], alpha, call0, **pkw)
    rec = eng.backward_batch(sc, g, ha, np.stack(gts), 1.0, 100.0, 100.0, p, cams=cams)
    out = dict(rec=rec.copy(), grad=g.cpu().numpy())
    out.update(_buffers(eng, len(has), out["rec"]))
    return out


def _async(eng, frames, has, gts, alpha, call0, shared=None, g0=None, cams=None, check=True, read=True, **pkw):
    """One asynchronous call on an idle stream with finished inputs, the ground truth a DEVICE tensor; then one synchronisation."""
    sc, ha, g = _tensors(frames, has, shared, g0)
    gt = torch.from_numpy(np.stack(gts)).cuda()
    p = _params(eng, frames[0], ha.shape[1], alpha, call0, **pkw)
    torch.cuda.synchronize()
    rec = eng.backward_batch_async(sc, g, ha, gt, 1.0, 100.0, 100.0, p, cams=cams)
    assert rec.is_cuda and rec.dtype == torch.float64 and tuple(rec.shape) == (len(has), 4)
    torch.cuda.synchronize()
    if check:
        eng.check()
    out = dict(rec=rec.cpu().numpy(), grad=g.cpu().numpy())
    if read:
        out.update(_buffers(eng, len(has), out["rec"], with_losses=True))
    return out


def _assert_selected(out, frames=None):
    counts = out["rec"][:, 1] if frames is None else out["rec"][frames, 1]
    assert counts.min() >= 1, counts  # (no comparison below is vacuous)


def _assert_matches_blocking(got, want, what, frames=None, g0=None):
    """`got` (asynchronous) against `want` (blocking): the bars of tests/test_gpu_backward.py; prints whether it was exact."""
    B = got["rec"].shape[0]
    idx = list(range(B)) if frames is None else list(frames)
    for key, _ in GT_FREE:
        if key in got and key in want:
            np.testing.assert_array_equal(got[key][idx], want[key][idx], err_msg="%s: %s" % (what, key))
    exact = np.array_equal(got["rec"][idx], want["rec"][idx]) and np.array_equal(got["grad"][idx], want["grad"][idx])
    worst_l, worst_g = 0.0, 0.0
    for b in idx:
        np.testing.assert_array_equal(got["rec"][b, 1:], want["rec"][b, 1:], err_msg="%s: frame %d slots, entropy, flag" % (what, b))
        lw, lg = want["rec"][b, 0], got["rec"][b, 0]
        if lw != lw:
            assert lg != lg, (what, b)
        else:
            rel = abs(lg - lw) / max(1.0, abs(lw))
            worst_l = max(worst_l, rel)
            assert rel <= LOSS_RTOL, (what, b, lg, lw)
        contrib = want["grad"][b] if g0 is None else want["grad"][b] - g0[b]
        if np.isfinite(want["grad"][b]).all():
            scale = max(float(np.abs(contrib).max()), 1e-30)
            err = float(np.abs(got["grad"][b] - want["grad"][b]).max()) / scale
            worst_g = max(worst_g, err)
            assert err <= GRAD_RTOL, (what, b, err, scale)
        else:
            np.testing.assert_array_equal(np.isnan(got["grad"][b]), np.isnan(want["grad"][b]), err_msg="%s: frame %d NaN pattern" % (what, b))
    print("%s: asynchronous vs blocking %s (loss rel %.3g, gradient %.3g of the frame's largest entry)"
          % (what, "EXACT" if exact else "not exact", worst_l, worst_g))


# ---------------------------------------------------------------- 1. equals the blocking batch
@pytest.mark.parametrize("case", ["one_expert", "gating"])
def test_async_equals_the_blocking_batch(solo, oracle, case):
    """B = 6 (one expert, N = 96; 3 experts with a gating assignment, N = 64): one asynchronous call, one synchronisation, against
    Engine.backward_batch on the same inputs and counters, and every frame against the CPU oracle at call0 + b."""
    frames, has, gts, alpha = _case(case)
    call0 = 23
    got = _async(solo, frames, has, gts, alpha, call0)
    want = _blocking(solo, frames, has, gts, alpha, call0)
    _assert_selected(want)
    _assert_selected(got)
    _assert_matches_blocking(got, want, case)
    assert np.abs(got["grad"]).max() > 0
    for b, f in enumerate(frames):
        ref, g_ref = _oracle(oracle, f["coords"], f, has[b], gts[b], alpha, call0 + b)
        assert _check_frame(got["rec"][b], got["grad"][b], ref, g_ref, got["probs"][b], got["refh"][b], got["losses"][b]) >= 1


# ---------------------------------------------------------------- 2. it does not block
@pytest.mark.parametrize("own_stream", [False, True], ids=["default_stream", "own_stream"])
def test_async_returns_while_the_stream_is_busy(solo, own_stream):
    """Behind a 50 ms hold and producers that finish late (until their copies run, the coordinate, assignment and ground-truth
    tensors hold ANOTHER frame's finite values and the gradients hold 3.0): the call returns with the stream still busy, a consumer
    on the stream clones gradients and record with no host synchronisation, and everything equals the idle-stream run."""
    frames, has, gts, alpha = _case("gating")
    call0 = 23
    want = _async(solo, frames, has, gts, alpha, call0)
    _assert_selected(want)
    other = _case("gating", first=700)
    _async(solo, other[0], other[1], other[2], alpha, 90)  # another batch's state in the workspace
    stream = torch.cuda.Stream() if own_stream else None
    real_sc, real_ha, _ = _tensors(frames, has)
    real_gt = torch.from_numpy(np.stack(gts)).cuda()
    p = _params(solo, frames[0], real_ha.shape[1], alpha, call0)
    torch.cuda.synchronize()
    with _on(stream):
        sc, ha, gt = (torch.roll(t, 1, 0).contiguous() for t in (real_sc, real_ha, real_gt))
        g = torch.full_like(real_sc, 3.0)
        assert bool(torch.isfinite(sc).all()) and bool(torch.isfinite(gt).all()) and not torch.equal(gt, real_gt)
        torch.cuda.current_stream().synchronize()
        _hold(HOLD_MS)
        sc.copy_(real_sc, non_blocking=True)
        ha.copy_(real_ha, non_blocking=True)
        gt.copy_(real_gt, non_blocking=True)
        g.zero_()
        rec = solo.backward_batch_async(sc, g, ha, gt, 1.0, 100.0, 100.0, p)
        busy = not torch.cuda.current_stream().query()
        clones = (g.clone(), rec.clone())  # the caller's own work behind the call: same stream, no host synchronisation
    torch.cuda.synchronize()
    assert busy, "the stream had drained when the asynchronous call returned: it waited for the hold"
    solo.check()
    assert torch.equal(sc, real_sc) and torch.equal(gt, real_gt)  # (the producers have run)
    np.testing.assert_array_equal(rec.cpu().numpy(), want["rec"])
    np.testing.assert_array_equal(g.cpu().numpy(), want["grad"])
    np.testing.assert_array_equal(clones[0].cpu().numpy(), want["grad"], err_msg="gradients as the consumer on the stream saw them")
    np.testing.assert_array_equal(clones[1].cpu().numpy(), want["rec"], err_msg="record as the consumer on the stream saw it")
    got = _buffers(solo, len(has), want["rec"], with_losses=True)
    for key in got:
        np.testing.assert_array_equal(got[key], want[key], err_msg=key)


# ---------------------------------------------------------------- 3. two calls back to back
def test_two_async_calls_back_to_back(solo):
    """Two batches (different frames, ground truths and per-frame camera tables) on one stream with nothing between them; the
    caller's camera table and host pose array are overwritten as soon as each call has returned.  Each equals its own blocking
    result."""
    a, b = _cam_case(800), _cam_case(830)
    alpha = 20.0
    want = [_blocking(solo, x[0], x[1], x[2], alpha, c0, cams=x[3]) for x, c0 in ((a, 40), (b, 60))]
    for w in want:
        _assert_selected(w)
    torch.cuda.synchronize()
    runs = []
    for x, c0 in ((a, 40), (b, 60)):
        sc, ha, g = _tensors(x[0], x[1])
        table, poses = x[3].copy(), np.stack(x[2]).copy()
        p = solo.make_params(3, 60, 80, 64, shift_x=-77, shift_y=91, focal=1234.5, ppx=-5.0, ppy=9999.0, sub_sampling=x[0][0]["sub"],
                             inlier_alpha=alpha, seed=1305, call=c0)  # (the five camera fields are ignored with a table)
        rec = solo.backward_batch_async(sc, g, ha, poses, 1.0, 100.0, 100.0, p, cams=table)
        table["focal"] = 1.0
        table["shift_x"] = 7
        poses[:] = 0.0
        runs.append((rec, g))
    torch.cuda.synchronize()
    solo.check()
    for k, (rec, g) in enumerate(runs):
        got = dict(rec=rec.cpu().numpy(), grad=g.cpu().numpy())
        _assert_matches_blocking(got, want[k], "batch %d of two" % k)
    assert not np.array_equal(want[0]["grad"], want[1]["grad"])


# ---------------------------------------------------------------- 4. chunking
def test_async_chunking_is_invisible(monkeypatch):
    """One 60x80 frame's worst case at N = 96 is 96 slots x 240 000 bytes = 22 MiB: a budget of 50 MiB holds two frames, B = 6 runs
    in 3 chunks enqueued one after another, and returns the one-chunk result exactly.  A budget of 16 MiB is below one frame's
    worst case: -4 before anything is launched, the gradients stay untouched."""
    monkeypatch.setenv("ESAC_SLOT_TEAMS", "0")
    whole = api.Engine(0)
    monkeypatch.setenv("ESAC_BWD_BATCH_BUDGET_MB", "50")
    small = api.Engine(0)
    monkeypatch.setenv("ESAC_BWD_BATCH_BUDGET_MB", "16")
    tiny = api.Engine(0)
    frames, has, gts, alpha = _case("one_expert", first=900)
    one = _async(whole, frames, has, gts, alpha, 11)
    _assert_selected(one)
    got = _async(small, frames, has, gts, alpha, 11, read=False)
    np.testing.assert_array_equal(got["rec"], one["rec"])
    np.testing.assert_array_equal(got["grad"], one["grad"])
    # the chunked context's buffers hold the last chunk: two frames, frames 4 and 5
    with pytest.raises(RuntimeError):
        small.read_frames(api.BUF_BWD_PROBS, 6)
    with pytest.raises(RuntimeError):
        small.read_frames(api.BUF_BWD_PROBS, 3)
    np.testing.assert_array_equal(small.read_frames(api.BUF_BWD_PROBS, 2), one["probs"][4:])
    # below one frame's worst case
    sc, ha, g = _tensors(frames, has, g0=np.full((6,) + frames[0]["coords"].shape, 0.25, np.float32))
    gt = torch.from_numpy(np.stack(gts)).cuda()
    with pytest.raises(RuntimeError, match=r"ESAC_BWD_BATCH_BUDGET_MB.*esac_hip_backward_batch.*\[status -4\]"):
        tiny.backward_batch_async(sc, g, ha, gt, 1.0, 100.0, 100.0, _params(tiny, frames[0], 96, alpha, 11))
    torch.cuda.synchronize()
    assert bool((g == 0.25).all())


# ---------------------------------------------------------------- 5. per-frame outcomes
def test_a_singular_pose_is_that_frames_outcome(solo):
    """Frame 2 of 4 has an all-zero ground-truth pose: its record is (NaN, 0, 0, 2), its gradients keep their non-zero initial
    content, frames 0, 1 and 3 are the blocking batch's (run with a valid pose in frame 2), and check() names frame 2."""
    frames, has, gts, alpha = _case("gating", first=1000, B=4)
    g0 = (np.random.default_rng(5).normal(size=(4,) + frames[0]["coords"].shape) * 1e-3).astype(np.float32)
    assert np.abs(g0[2]).min() > 0
    want = _blocking(solo, frames, has, gts, alpha, 31, g0=g0)
    _assert_selected(want)
    bad = [g.copy() for g in gts]
    bad[2][:] = 0.0
    got = _async(solo, frames, has, bad, alpha, 31, g0=g0, check=False)
    rec2 = got["rec"][2]
    assert np.isnan(rec2[0]) and list(rec2[1:]) == [0.0, 0.0, 2.0], rec2
    np.testing.assert_array_equal(got["grad"][2], g0[2])
    _assert_selected(got, frames=[0, 1, 3])
    _assert_matches_blocking(got, want, "beside a singular frame", frames=[0, 1, 3], g0=g0)
    with pytest.raises(RuntimeError, match=r"frame 2 is singular.*\[status -4\]"):
        solo.check()
    # the next call on the context is clean again
    clean = _async(solo, frames, has, gts, alpha, 31, g0=g0)
    _assert_matches_blocking(clean, want, "the call after it", g0=g0)


def test_an_out_of_range_assignment_flags_its_frame(solo):
    frames, has, gts, alpha = _case("gating", first=1000, B=4)
    want = _blocking(solo, frames, has, gts, alpha, 31)
    has_bad = [h.copy() for h in has]
    has_bad[1][5] = 3  # E = 3
    got = _async(solo, frames, has_bad, gts, alpha, 31, check=False)
    np.testing.assert_array_equal(got["rec"][:, 3], [0.0, 1.0, 0.0, 0.0])
    with pytest.raises(RuntimeError, match=r"\[status -10\]"):
        solo.check()
    _assert_selected(got, frames=[0, 2, 3])
    _assert_matches_blocking(got, want, "beside a flagged frame", frames=[0, 2, 3])


def test_async_rejects_bad_arguments_before_launching(solo):
    """esac_hip_backward_batch_dev's twin of test_gpu_backward_batch.py::test_batch_rejects_bad_arguments_before_launching, on its
    shape (E=3, 60x80, N=64, B=4): every argument error is reported before a launch (the prefilled gradient tensor is
    bit-unchanged after a synchronisation), with the status and the message written out here, and -- for every defect that
    both entry points check -- with the very bytes that the blocking esac_hip_backward_batch reports for the same defect."""
    f = S.make_frame(280, E=3, true_expert=0)
    B, N, slab = 4, 64, 3 * 3 * 60 * 80
    sc = torch.from_numpy(np.stack([f["coords"]] * B)).cuda()
    ha = torch.zeros((B, N), dtype=torch.int64, device="cuda")
    g = torch.from_numpy(np.random.default_rng(1).normal(size=(B,) + f["coords"].shape).astype(np.float32)).cuda()
    g_keep = g.clone()
    gt_host = np.stack([np.array(f["gt_pose"], np.float32)] * B)
    gt_dev = torch.from_numpy(gt_host).cuda()
    rec_dev = torch.zeros((B, 4), dtype=torch.float64, device="cuda")
    rec_host = np.zeros((B, 4), np.float64)
    lib = solo.lib

    def call(dev, B_=B, sc_=None, grad=None, ha_=None, gt=None, stride=slab, p=None, out=None):
        p = p if p is not None else solo.make_params(3, 60, 80, N)
        head = (solo.ctx, B_, sc.data_ptr() if sc_ is None else sc_, slab, g.data_ptr() if grad is None else grad, stride,
                ha.data_ptr() if ha_ is None else ha_)
        tail = (1.0, 100.0, 100.0, C.byref(p), solo._stream())
        if dev:
            rc = lib.esac_hip_backward_batch_dev(*head, gt_dev.data_ptr() if gt is None else gt, None, *tail,
                                                 rec_dev.data_ptr() if out is None else out)
        else:
            rc = lib.esac_hip_backward_batch(*head, gt_host.ctypes.data if gt is None else gt, *tail,
                                             rec_host.ctypes.data if out is None else out)
        return rc, lib.esac_hip_last_error()

    who = b"esac_hip_backward_batch: "
    null = (-1, who + b"null coordinate, gradient, assignment or ground-truth pointer")
    cases = [  # (the defect, status and message of the asynchronous call, whether the blocking call checks the same thing)
        (dict(B_=0), (-4, who + b"batch size 0 outside [1,1024]"), True),
        (dict(B_=1025), (-4, who + b"batch size 1025 outside [1,1024]"), True),
        (dict(sc_=0), null, True),
        (dict(grad=0), null, True),
        (dict(ha_=0), null, True),
        (dict(gt=0), null, True),
        (dict(out=0), (-1, b"esac_hip_backward_batch_dev: d_out (device double[B,4]) is required"), False),
        (dict(p=solo.make_params(3, 60, 80, N, hyp_offset=16)),
         (-4, who + b"sharded calls are not supported (the expectation needs every hypothesis)"), True),
        (dict(stride=slab - 1), (-4, who + b"gradient frame stride 43199 < E*3*H*W = 43200 (frames would share gradients)"), True),
        (dict(p=solo.make_params(70000, 60, 80, N)),
         (-4, who + b"at most 65535 experts (one grid row per expert in the accumulation kernel)"), True),
        (dict(p=solo.make_params(3, 60, 80, N, strict_reference=True)),
         (-4, who + b"the training path has no strict mode (ESAC_FLAG_STRICT_REFERENCE is a forward flag)"), True),
    ]
    for kw, want, shared in cases:
        got = call(True, **kw)
        print(sorted(kw), got)
        assert got[0] != 0 and got == want, (kw, got)
        torch.cuda.synchronize()
        assert torch.equal(g, g_keep), kw
        if shared:
            assert call(False, **kw) == got, kw
            torch.cuda.synchronize()
            assert torch.equal(g, g_keep), kw


# ---------------------------------------------------------------- 6. the other features
def test_async_with_per_frame_cameras(solo):
    frames, has, gts, cams = _cam_case(1100)
    want = _blocking(solo, frames, has, gts, 20.0, 40, cams=cams)
    _assert_selected(want)
    got = _async(solo, frames, has, gts, 20.0, 40, cams=cams)
    _assert_matches_blocking(got, want, "per-frame cameras")
    plain = _blocking(solo, frames, has, gts, 20.0, 40)  # (the table matters: frame 0's camera for every frame is another result)
    assert not np.array_equal(plain["grad"][1:], want["grad"][1:])


def test_async_strict_training(solo):
    """One small case (the inputs of tests/test_gpu_strict_training.py's batch) against the blocking strict batch."""
    frames = [S.make_frame(820 + b, E=2, true_expert=b % 2) for b in range(3)]
    has = [S.gating_assignment(f, 96, mode="gating") for f in frames]
    gts = [_gt(f, 1250 + b) for b, f in enumerate(frames)]
    want = _blocking(solo, frames, has, gts, 30.0, 9, strict_training=True)
    _assert_selected(want)
    got = _async(solo, frames, has, gts, 30.0, 9, strict_training=True)
    _assert_matches_blocking(got, want, "strict training")


def test_async_accumulates_into_prefilled_gradients(solo):
    frames, has, gts, alpha = _case("one_expert", first=1300, B=3)
    g0 = (np.random.default_rng(9).normal(size=(3,) + frames[0]["coords"].shape) * 1e-3).astype(np.float32)
    want = _blocking(solo, frames, has, gts, alpha, 5, g0=g0)
    _assert_selected(want)
    got = _async(solo, frames, has, gts, alpha, 5, g0=g0)
    _assert_matches_blocking(got, want, "pre-filled gradients", g0=g0)
    assert not np.array_equal(got["grad"], g0)


def test_async_shared_maps(solo):
    """[E,3,H,W] shared by every frame (frame stride 0)."""
    f = S.make_frame(1400, E=2, true_expert=1)
    has = [S.gating_assignment(f, 64, mode="gating", rng=np.random.default_rng(b)) for b in range(3)]
    gts = [_gt(f, 1450 + b, noise=0.1) for b in range(3)]
    want = _blocking(solo, [f] * 3, has, gts, 20.0, 5, shared=f["coords"])
    _assert_selected(want)
    got = _async(solo, [f] * 3, has, gts, 20.0, 5, shared=f["coords"])
    _assert_matches_blocking(got, want, "shared maps")


def test_async_a_frame_that_selects_nothing(solo):
    """N = 2048 and a flat distribution: nothing is refined or accumulated in any frame; the records are valid and the blocking
    call's."""
    frames = [S.make_frame(1500 + b, H=24, W=32, sub=20) for b in range(2)]
    has = [S.gating_assignment(f, 2048) for f in frames]
    gts = [_gt(f, 1550 + b) for b, f in enumerate(frames)]
    g0 = np.random.default_rng(4).normal(size=(2,) + frames[0]["coords"].shape).astype(np.float32)
    want = _blocking(solo, frames, has, gts, 1e-4, 1, g0=g0)
    got = _async(solo, frames, has, gts, 1e-4, 1, g0=g0)
    assert (got["rec"][:, 1] == 0).all() and (got["rec"][:, 3] == 0).all() and np.isfinite(got["rec"]).all()
    np.testing.assert_array_equal(got["grad"], g0)
    for b in range(2):
        assert abs(got["rec"][b, 0] - want["rec"][b, 0]) <= LOSS_RTOL * max(1.0, abs(want["rec"][b, 0]))
        np.testing.assert_array_equal(got["rec"][b, 1:], want["rec"][b, 1:])


def test_the_drop_in_surface(solo, monkeypatch):
    """esac.backward_batch_async: the [B] device losses, last_result()'s [B,4] device record, the call counter, and its refusals
    on the device side (a strided device gradient tensor)."""
    import esac
    monkeypatch.setitem(api._state, "engines", {0: solo})
    frames, has, gts, alpha = _case("gating", first=1600, B=3)
    want = _blocking(solo, frames, has, gts, alpha, 500)
    _assert_selected(want)
    sc, ha, g = _tensors(frames, has)
    f0 = frames[0]
    tail = (0, 0, f0["focal"], f0["ppx"], f0["ppy"], 10.0, alpha, 0.5, 100.0, f0["sub"])
    esac.set_seed(1305, 500)
    wide = torch.zeros(g.shape[:-1] + (2 * g.shape[-1],), device="cuda")[..., ::2]
    with pytest.raises(RuntimeError, match="outGradients must be contiguous"):
        esac.backward_batch_async(sc, wide, ha, torch.from_numpy(np.stack(gts)).cuda(), 1.0, 100.0, 100.0, *tail)
    assert esac.get_rng_state() == (1305, 500)
    losses = esac.backward_batch_async(sc, g, ha, torch.from_numpy(np.stack(gts)).cuda(), 1.0, 100.0, 100.0, *tail)
    assert esac.get_rng_state() == (1305, 503)
    assert losses.is_cuda and tuple(losses.shape) == (3,) and losses.dtype == torch.float64
    rec = esac.last_result()["backward"]
    assert rec.is_cuda and tuple(rec.shape) == (3, 4)
    torch.cuda.synchronize()
    solo.check()
    np.testing.assert_array_equal(losses.cpu().numpy(), rec.cpu().numpy()[:, 0])
    _assert_matches_blocking(dict(rec=rec.cpu().numpy(), grad=g.cpu().numpy()), want, "esac.backward_batch_async")


# ---------------------------------------------------------------- 7. harness.train_batch
class _Expert(torch.nn.Module):
    """A learnable [B,3,h,w] map (elementwise: it rounds the same whatever the batch); the first one to run may queue the hold."""

    def __init__(self, maps, state):
        super().__init__()
        self.map = torch.nn.Parameter(torch.from_numpy(np.ascontiguousarray(maps)).cuda())
        self.state = state

    def forward(self, images):
        if self.state.get("hold_ms") and not self.state.get("held"):
            self.state["held"] = True
            _hold(self.state["hold_ms"])
        return self.map * 1.0


class _Gating(torch.nn.Module):
    def __init__(self, logits):
        super().__init__()
        self.logits = torch.nn.Parameter(torch.tensor(logits, dtype=torch.float32).cuda())

    def forward(self, images):
        return torch.log_softmax(self.logits, dim=1)


def test_train_batch_asynchronous(solo, monkeypatch):
    """harness.train_batch(asynchronous=True, all_experts=True) with synthetic experts, given assignments and shifts, behind a
    50 ms hold queued by the first expert: the call returns with the stream still busy, `losses` is a device tensor, and after a
    synchronisation the parameter gradients of the experts and of the gating are the blocking train_batch's."""
    import esac
    from esac_amd import harness
    monkeypatch.setitem(api._state, "engines", {0: solo})
    E, N, B = 3, 64, 6
    frames, has, gts, _ = _cam_case(1700, B=B, E=E, N=N)
    has = [h.copy() for h in has]
    has[0][:] = 0  # frame 0 uses expert 0 only
    e_hyps = torch.from_numpy(np.stack(has)).cuda()
    maps = np.stack([f["coords"] for f in frames])
    logits = np.random.default_rng(3).normal(size=(B, E))
    images = torch.zeros(B, 3, 480, 640, device="cuda")
    gt_dev = torch.from_numpy(np.stack(gts)).cuda()

    def step(state, **kw):
        experts = [_Expert(maps[:, e], state) for e in range(E)]
        gating = _Gating(logits)
        esac.set_seed(1305, 40)
        torch.cuda.synchronize()
        out = harness.train_batch(images, gt_dev if kw else np.stack(gts), gating, experts, FOCALS[:B], hypotheses=N, inlier_alpha=20.0,
                                  shifts=SHIFTS[:B], e_hyps=e_hyps, **kw)
        busy = not torch.cuda.current_stream().query()
        torch.cuda.synchronize()
        return out, busy, [x.map.grad.cpu().numpy() for x in experts], gating.logits.grad.cpu().numpy()

    want, _, want_maps, want_logits = step({})
    step({}, asynchronous=True, all_experts=True)  # (workspaces of the asynchronous route sized: nothing grows behind the hold)
    state = {"hold_ms": HOLD_MS}
    got, busy, got_maps, got_logits = step(state, asynchronous=True, all_experts=True)
    assert state.get("held") and busy, "train_batch(asynchronous=True, all_experts=True) waited for the stream"
    assert isinstance(got["losses"], torch.Tensor) and got["losses"].is_cuda and tuple(got["losses"].shape) == (B,)
    solo.check()
    assert esac.get_rng_state() == (1305, 40 + B)
    rec = esac.last_result()["backward"].cpu().numpy()
    assert rec[:, 1].min() >= 1, rec[:, 1]
    losses = got["losses"].cpu().numpy()
    for b in range(B):
        assert abs(losses[b] - want["losses"][b]) <= LOSS_RTOL * max(1.0, abs(want["losses"][b])), (b, losses[b], want["losses"][b])
    exact = all(np.array_equal(a, w) for a, w in zip(got_maps, want_maps)) and np.array_equal(got_logits, want_logits)
    print("train_batch asynchronous vs blocking: %s" % ("EXACT" if exact else "not exact"))
    for b in range(B):
        scale = max(max(float(np.abs(w[b]).max()) for w in want_maps), 1e-30)
        for e in range(E):
            err = float(np.abs(got_maps[e][b] - want_maps[e][b]).max()) / scale
            assert err <= GRAD_RTOL, (b, e, err)
    assert np.abs(np.stack(want_maps)).max() > 0 and np.abs(want_logits).max() > 0
    assert float(np.abs(got_logits - want_logits).max()) <= GRAD_RTOL * float(np.abs(want_logits).max())
