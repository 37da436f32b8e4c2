"""Stream order behind a BUSY caller stream.  Every other GPU test calls the library on an idle stream with finished inputs; the
integrated use (harness.localize / train_step / train_batch, the sharded forward) enqueues the expert networks asynchronously
and calls esac.forward / esac.backward behind them with no host synchronisation.  Here the caller's stream holds work ahead of
every call:

    hold_launch(stream, T)                       one sleeping wavefront (tests/native/filler.hip: no LDS, it holds the STREAM, not the CUs)
    dev_coords.copy_(real_coords, non_blocking)  the producer that finishes late

and before that copy runs, dev_coords holds ANOTHER frame's finite coordinates: a kernel that reads its input early computes
something plausible and wrong, not NaN.  T is derived from the library's own bound on its hand-off waits (ESAC_SPEC_WAIT_TICKS,
parsed out of device_common.hpp): 0.25 x, 1.5 x and 3 x the bound -- 5 / 30 / 60 ms today.

The bar is the one of tests/test_gpu_speculation.py: EVERY output bit for bit what the same call produces on an idle stream with
finished inputs (for the speculative shapes: what the serial route, ESAC_DEBUG_NO_SPECULATION, produces), whatever the workspace
held before -- a different frame of the same shape runs through the context in between.  Where stated the oracle is held against
as well, at the suite's bars (discrete outputs equal, pose 1e-4 rad / 1e-3 m).  Plain correctness under load: nothing here
provokes a fault or a hang, and the hold is bounded by the wall clock (hold_launch refuses more than 200 ms).
"""
import contextlib
import ctypes as C
import os
import re
import socket

import numpy as np
import pytest
import torch

from esac_amd import api
from esac_amd import synthetic as S

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("tries", "xy", "hyps", "flags", "scores", "user", "counts", "imap")
SPEC_SHAPES = [(3, 300), (10, 1024), (12, 4096)]  # test_speculative_route_equals_the_serial_route
SHAPE_IDS = ["%dx%d" % s for s in SPEC_SHAPES]
HOLDS = [0.25, 1.5, 3.0]  # x the bound
HOLD_IDS = ["0.25x", "1.5x", "3x"]


def _bound_ms():
    """The library's bound on a hand-off wait, in ms of the 100 MHz wall clock -- from its own source, not restated here."""
    with open(os.path.join(ROOT, "esac_amd", "csrc", "device_common.hpp")) as fh:
        m = re.search(r"\bESAC_SPEC_WAIT_TICKS\s*=\s*(\d+)\s*;", fh.read())
    assert m, "ESAC_SPEC_WAIT_TICKS is not defined in device_common.hpp any more: derive the holds from what replaced it"
    return int(m.group(1)) / 1.0e5


_hold_fn = []


def _hold(ms):
    """Queues the sleeping wavefront on torch's current stream."""
    if not _hold_fn:
        from tests.native import build as nb
        lib = C.CDLL(nb.build_filler())
        lib.hold_launch.argtypes = [C.c_void_p, C.c_float]
        lib.hold_launch.restype = C.c_int
        _hold_fn.append(lib.hold_launch)
    rc = _hold_fn[0](C.c_void_p(torch.cuda.current_stream().cuda_stream), float(ms))
    assert rc == 0, "hold_launch(%g ms) answered %d" % (ms, rc)


def _produce(dst, real, ms):
    """The late producer on the current stream: the hold, then the copy that makes `dst` the call's real input."""
    _hold(ms)
    dst.copy_(real, non_blocking=True)


def _on(stream):
    return torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext()


def test_the_hold_is_bounded():
    """More than 200 ms is an error and launches nothing; the bound the holds are derived from is there."""
    assert 0.0 < 3.0 * _bound_ms() <= 200.0
    _hold(0.0)
    assert _hold_fn[0](C.c_void_p(torch.cuda.current_stream().cuda_stream), 200.5) != 0
    assert _hold_fn[0](C.c_void_p(torch.cuda.current_stream().cuda_stream), float("nan")) != 0
    assert _hold_fn[0](C.c_void_p(torch.cuda.current_stream().cuda_stream), -1.0) != 0
    import time
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    _hold(20.0)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    assert 0.019 < dt < 0.2, dt


def _forward(engine, frame, ha, call, nospec=False, hold_ms=None, stale=None, asynchronous=False, consumer=False, stream=None,
             seed=1305, **pkw):
    """One forward_device call and everything it left (test_gpu_speculation.py:_run).  hold_ms: the call runs behind the late
    producer, its input tensor holding `stale`'s coordinates until the producer's copy; otherwise finished inputs, idle stream."""
    E, _, H, W = frame["coords"].shape
    real, hat = torch.from_numpy(frame["coords"]).cuda(), torch.from_numpy(ha).cuda()
    sc = real if hold_ms is None else torch.from_numpy(stale["coords"]).cuda()
    assert sc.shape == real.shape and bool(torch.isfinite(sc).all())
    p = engine.make_params(E, H, W, len(ha), focal=frame["focal"], ppx=frame["ppx"], ppy=frame["ppy"], sub_sampling=frame["sub"],
                           seed=seed, call=call, **pkw)
    scores = torch.full((len(ha),), -7.0, dtype=torch.float64, device="cuda")
    dev_rec = torch.full((32,), -7.0, dtype=torch.float64, device="cuda") if asynchronous else None
    clones = None
    engine.set_debug(no_speculation=nospec)
    try:
        torch.cuda.synchronize()
        with _on(stream):
            if hold_ms is not None:
                _produce(sc, real, hold_ms)
            rec = engine.forward_device(sc, hat, p, scores_out=scores, result_out=dev_rec, want_host=not asynchronous)
            if consumer:  # work of the caller's own behind the call, same stream, no host synchronisation
                clones = (scores.clone(), dev_rec.clone())
        torch.cuda.synchronize()
        if asynchronous:
            engine.check()
        assert torch.equal(sc, real)  # (the producer has run)
        out = dict(rec=None if rec is None else rec.copy(), hyps=engine.read(api.BUF_HYPS), tries=engine.read(api.BUF_TRIES),
                   xy=engine.read(api.BUF_SAMPLE_XY), scores=engine.read(api.BUF_SCORES), flags=engine.read(api.BUF_EXACT_FLAGS),
                   user=scores.cpu().numpy(), counts=engine.read(api.BUF_INLIER_COUNTS), imap=engine.read(api.BUF_INLIER_MAP),
                   info=engine.spec_info(), result=engine.read(api.BUF_RESULT), refine=engine.refine_info())
        if asynchronous:
            out["dev_rec"] = dev_rec.cpu().numpy()
        if clones is not None:
            out["clones"] = (clones[0].cpu().numpy(), clones[1].cpu().numpy())
        return out
    finally:
        engine.set_debug()


def _assert_same(want, got, what):
    """`got` against the reference run `want` (a blocking call): every output, and whichever record `got` delivered."""
    for key in KEYS:
        np.testing.assert_array_equal(got[key], want[key], err_msg="%s: %s" % (what, key))
    np.testing.assert_array_equal(got["result"][:31], want["result"][:31], err_msg="%s: workspace record" % what)
    if got["rec"] is not None:
        np.testing.assert_array_equal(got["rec"], want["rec"], err_msg="%s: host record" % what)
    if "dev_rec" in got:
        assert got["dev_rec"][31] == 1.0, "%s: ESAC_RES_VALID of the device record is %r" % (what, got["dev_rec"][31])
        np.testing.assert_array_equal(got["dev_rec"][:31], want["rec"][:31], err_msg="%s: device record" % what)
    if "clones" in got:
        np.testing.assert_array_equal(got["clones"][0], want["user"], err_msg="%s: scores as the consumer on the stream saw them" % what)
        assert got["clones"][1][31] == 1.0, what
        np.testing.assert_array_equal(got["clones"][1][:31], want["rec"][:31], err_msg="%s: record as the consumer on the stream saw it" % what)


def _assert_oracle(oracle, frame, ha, call, got, seed=1305, **okw):
    ref = oracle.forward(frame["coords"], ha, focal=frame["focal"], ppx=frame["ppx"], ppy=frame["ppy"], sub_sampling=frame["sub"],
                         seed=seed, call=call, **okw)
    rec = got["rec"] if got["rec"] is not None else got["dev_rec"]
    assert int(rec[api.RES_HYP]) == ref["winner"] and int(rec[api.RES_EXPERT]) == ref["expert"]
    np.testing.assert_array_equal(got["tries"], ref["tries"])
    r_err, t_err = S.pose_errors(rec[api.RES_POSE:api.RES_POSE + 16].reshape(4, 4), ref["pose"])
    assert r_err <= 1e-4 and t_err <= 1e-3, (r_err, t_err)


def _frames(first, E, N, mode="gating", **kw):
    """The frame under test, the foreign frame (workspace state and stale input) and the frame of the call after."""
    fs = [S.make_frame(first + k, E=E, true_expert=k % E, **kw) for k in range(3)]
    return fs, [S.gating_assignment(f, N, mode=mode) for f in fs]


def _speculative_case(engine, E, N, hold_ms, asynchronous, stream=None, consumer=False, oracle=None, first=2000):
    (f, other, nxt), (ha, ha_other, ha_nxt) = _frames(first + 7 * E, E, N)
    want = _forward(engine, f, ha, call=5, nospec=True)
    want_nxt = _forward(engine, nxt, ha_nxt, call=6, nospec=True)
    assert not want["info"]["last_speculative"]
    _forward(engine, other, ha_other, call=4)  # another frame's lists, flags and scores in the workspace
    got = _forward(engine, f, ha, call=5, hold_ms=hold_ms, stale=other, asynchronous=asynchronous, consumer=consumer, stream=stream)
    what = "E=%d N=%d hold %s ms %s" % (E, N, hold_ms, "asynchronous" if asynchronous else "blocking")
    print("%s: last_speculative %s last_failed %s%s" % (what, got["info"]["last_speculative"], got["info"]["last_failed"],
                                                        ", ESAC_RES_VALID %r" % got["dev_rec"][31] if asynchronous else ""))
    assert got["info"]["last_speculative"], what + ": the call left the speculative route"
    _assert_same(want, got, what)
    if oracle is not None:
        _assert_oracle(oracle, f, ha, 5, got)
    # the next call on this context, idle stream: its own reference, and still speculative (one busy call latches nothing,
    # and leaves no counter, list or flag behind)
    after = _forward(engine, nxt, ha_nxt, call=6)
    assert after["info"]["last_speculative"], what + ": the context stopped speculating"
    _assert_same(want_nxt, after, what + ", the idle call after it")


@pytest.mark.parametrize("form", ["blocking", "asynchronous"])
@pytest.mark.parametrize("mult", HOLDS, ids=HOLD_IDS)
@pytest.mark.parametrize("E,N", SPEC_SHAPES, ids=SHAPE_IDS)
def test_speculative_route_behind_a_busy_stream(engine, oracle, E, N, mult, form):
    """The route with streams of the context's own, behind 0.25 / 1.5 / 3 bounds of backlog: the straggler chain, the selection and
    the join must not run before the caller's stream has reached the call.  Blocking (host record) and asynchronous (device record,
    ESAC_RES_VALID = 1, esac_hip_check passes); the idle call after it equals its own reference and still speculates; the smallest
    shape is held against the oracle too (winner, expert, accepted tries, pose)."""
    _speculative_case(engine, E, N, mult * _bound_ms(), form == "asynchronous", oracle=oracle if (E, N) == SPEC_SHAPES[0] else None)


@pytest.mark.parametrize("E,N", SPEC_SHAPES, ids=SHAPE_IDS)
def test_a_consumer_on_the_stream_sees_the_final_outputs(engine, E, N):
    """After an asynchronous call the caller clones the score vector and the device record ON THE SAME STREAM with no host
    synchronisation (what the multi-GPU exchange's pack does): the clones are the serial route's values."""
    _speculative_case(engine, E, N, 1.5 * _bound_ms(), True, consumer=True, first=2300)


def _plain_case(engine, E, N, hold_ms, stream=None, first=2600, mode="gating", expect=None, oracle=None, oracle_kw=None, **pkw):
    """A route that keeps every launch on the caller's stream: the same call idle is the reference."""
    (f, other, nxt), (ha, ha_other, ha_nxt) = _frames(first + 7 * E, E, N, mode=mode)
    want = _forward(engine, f, ha, call=5, **pkw)
    assert not want["info"]["last_speculative"]
    if expect is not None:
        expect(want)
    _forward(engine, other, ha_other, call=4, **pkw)
    got = _forward(engine, f, ha, call=5, hold_ms=hold_ms, stale=other, stream=stream, **pkw)
    what = "E=%d N=%d %r hold %s ms" % (E, N, pkw, hold_ms)
    assert not got["info"]["last_speculative"]
    if expect is not None:
        expect(got)
    _assert_same(want, got, what)
    asyn = _forward(engine, f, ha, call=5, hold_ms=hold_ms, stale=nxt, stream=stream, asynchronous=True, consumer=True, **pkw)
    _assert_same(want, asyn, what + " asynchronous")
    if oracle is not None:
        _assert_oracle(oracle, f, ha, 5, got, **(oracle_kw or {}))


def _team_folded(out):
    assert out["refine"]["mode"] == "team" and not out["refine"]["timed_out"], out["refine"]


@pytest.mark.parametrize("busy", [False, True], ids=["idle", "1.5x"])
@pytest.mark.parametrize("form", ["blocking", "asynchronous"])
@pytest.mark.parametrize("E,N", SPEC_SHAPES, ids=SHAPE_IDS)
def test_speculative_route_on_a_stream_of_the_callers_own(engine, E, N, form, busy):
    """Every other test calls on the default stream (stream argument 0).  The same comparisons under torch.cuda.stream(Stream()):
    the context's two streams against a caller's stream that is a stream object of its own, idle and behind the producer."""
    _speculative_case(engine, E, N, 1.5 * _bound_ms() if busy else None, form == "asynchronous", stream=torch.cuda.Stream(),
                      consumer=form == "asynchronous", first=2900)


@pytest.mark.parametrize("busy", [False, True], ids=["idle", "1.5x"])
def test_other_routes_on_a_stream_of_the_callers_own(engine, busy):
    """... and one call whose selection runs in the team's prologue (1 expert, 256 hypotheses) and one in plain stream order
    (1 expert, 512 hypotheses: selection kernel, no speculation)."""
    hold = 1.5 * _bound_ms() if busy else None
    _plain_case(engine, 1, 256, hold, stream=torch.cuda.Stream(), first=3200, mode="single", expect=_team_folded)
    _plain_case(engine, 1, 512, hold, stream=torch.cuda.Stream(), first=3300, mode="single")


def test_folded_selection_with_a_team_behind_a_busy_stream(engine, oracle):
    _plain_case(engine, 1, 256, 1.5 * _bound_ms(), first=3400, mode="single", expect=_team_folded, oracle=oracle)


@pytest.mark.parametrize("flag", ["exact_scores", "exact_sampling", "strict_reference"])
def test_exact_and_strict_routes_behind_a_busy_stream(engine, flag):
    """Shapes that would speculate without the flag: with it every launch is on the caller's stream."""
    _plain_case(engine, 3, 512, 1.5 * _bound_ms(), first=3500, **{flag: True})


# ---------------------------------------------------------------- batches with per-frame cameras
SHIFTS = [(0, 0), (4, -4), (-3, 2), (1, 4), (-4, -1), (2, 0), (0, -2), (3, 3)]
FOCALS = [525.0, 585.0, 480.0, 1050.0, 525.0, 700.0, 612.5, 560.0]


def _batch_inputs(E, N, mode, B, first):
    frames = [S.make_frame(first + b, E=E, true_expert=b % E, shift=SHIFTS[b % 8], focal=FOCALS[b % 8]) for b in range(B)]
    has = [S.gating_assignment(f, N, mode=mode) for f in frames]
    cams = api.make_cams([f["shift"][0] for f in frames], [f["shift"][1] for f in frames], [f["focal"] for f in frames],
                         [f["ppx"] for f in frames], [f["ppy"] for f in frames])
    return frames, has, cams


def _forward_batch(engine, frames, has, cams, call0, hold_ms=None):
    B, N = len(frames), len(has[0])
    E, _, H, W = frames[0]["coords"].shape
    real = torch.from_numpy(np.stack([f["coords"] for f in frames])).cuda()
    sc = real if hold_ms is None else torch.roll(real, 1, 0).contiguous()  # frame b holds frame b - 1's maps until the producer's copy
    ha = torch.from_numpy(np.stack(has)).cuda()
    p = engine.make_params(E, H, W, N, shift_x=-77, shift_y=91, focal=1234.5, ppx=-5.0, ppy=9999.0, sub_sampling=frames[0]["sub"],
                           seed=1305, call=call0)  # (the five camera fields are ignored with a table)
    scores = torch.full((B, N), -7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    if hold_ms is not None:
        _produce(sc, real, hold_ms)
    res = engine.forward_batch(sc, ha, p, scores_out=scores, cams=cams)
    torch.cuda.synchronize()
    out = dict(rec=res[:, :31].copy(), user=scores.cpu().numpy())
    for key, buf in (("tries", api.BUF_TRIES), ("xy", api.BUF_SAMPLE_XY), ("hyps", api.BUF_HYPS), ("scores", api.BUF_SCORES),
                     ("counts", api.BUF_INLIER_COUNTS)):
        out[key] = engine.read_forward_frames(buf, B)
    return out


@pytest.mark.parametrize("B,E,N,mode", [(8, 4, 128, "gating"), (40, 1, 48, "single")], ids=["B8", "B40"])
def test_forward_batch_with_cams_behind_a_busy_stream(engine, oracle, B, E, N, mode):
    """esac_hip_forward_batch_cams (the camera table's upload is on the caller's stream too) behind the producer: records, score
    vectors, sampled cells, tries, poses, refinement traces of all B frames are the idle call's; frame 0 and frame B - 1 against
    the oracle with their own cameras."""
    frames, has, cams = _batch_inputs(E, N, mode, B, 3700)
    want = _forward_batch(engine, frames, has, cams, 40)
    others = _batch_inputs(E, N, mode, B, 3800)
    _forward_batch(engine, others[0], others[1], others[2], 90)
    got = _forward_batch(engine, frames, has, cams, 40, hold_ms=1.5 * _bound_ms())
    for key in want:
        np.testing.assert_array_equal(got[key], want[key], err_msg=key)
    for b in (0, B - 1):
        f = frames[b]
        ref = oracle.forward(f["coords"], has[b], shift_x=f["shift"][0], shift_y=f["shift"][1], focal=f["focal"], ppx=f["ppx"],
                             ppy=f["ppy"], sub_sampling=f["sub"], seed=1305, call=40 + b)
        assert int(got["rec"][b][api.RES_HYP]) == ref["winner"] and int(got["rec"][b][api.RES_EXPERT]) == ref["expert"], b
        np.testing.assert_array_equal(got["tries"][b], ref["tries"])
        r_err, t_err = S.pose_errors(got["rec"][b][api.RES_POSE:api.RES_POSE + 16].reshape(4, 4), ref["pose"])
        assert r_err <= 1e-4 and t_err <= 1e-3, (b, r_err, t_err)


# ---------------------------------------------------------------- the training path
def _gt(frame, seed, noise=0.05):
    gt = np.array(frame["gt_pose"], np.float64)
    gt[:3, 3] += np.random.default_rng(seed).normal(size=3) * noise
    return gt.astype(np.float32)


def test_backward_behind_a_busy_stream(engine):
    """esac_hip_backward: expected loss, record, distribution, refined poses and the gradient tensor bit-equal to the idle call.
    The gradient tensor holds something else until a zero_() that is queued behind the hold as well (harness.train_step's
    zeros_like is such a launch)."""
    (f, other, _), (ha, ha_other, _) = _frames(3900, 3, 128)
    gt = _gt(f, 1)
    E, _, H, W = f["coords"].shape

    def run(frame, assign, call, hold_ms=None, stale=None):
        real, hat = torch.from_numpy(frame["coords"]).cuda(), torch.from_numpy(assign).cuda()
        sc = real if hold_ms is None else torch.from_numpy(stale["coords"]).cuda()
        g = torch.zeros_like(real) if hold_ms is None else torch.full_like(real, 3.0)
        p = engine.make_params(E, H, W, len(assign), focal=frame["focal"], ppx=frame["ppx"], ppy=frame["ppy"], sub_sampling=frame["sub"],
                               inlier_alpha=20.0, seed=1305, call=call)
        torch.cuda.synchronize()
        if hold_ms is not None:
            _produce(sc, real, hold_ms)
            g.zero_()
        rec = engine.backward_device(sc, g, hat, gt, 1.0, 100.0, 100.0, p)
        torch.cuda.synchronize()
        return dict(rec=rec.copy(), grad=g.cpu().numpy(), probs=engine.read(api.BUF_BWD_PROBS), hyps=engine.read(api.BUF_BWD_REF_HYPS),
                    losses=engine.read(api.BUF_BWD_LOSSES))

    want = run(f, ha, 11)
    assert want["rec"][1] >= 1 and np.abs(want["grad"]).max() > 0
    run(other, ha_other, 12)
    got = run(f, ha, 11, hold_ms=1.5 * _bound_ms(), stale=other)
    for key in want:
        np.testing.assert_array_equal(got[key], want[key], err_msg=key)


def test_backward_batch_behind_a_busy_stream(engine):
    """esac_hip_backward_batch_cams over 8 frames with per-frame cameras, the same way."""
    frames, has, cams = _batch_inputs(4, 128, "gating", 8, 4000)
    others = _batch_inputs(4, 128, "gating", 8, 4100)
    gts = np.stack([_gt(f, b) for b, f in enumerate(frames)])
    E, _, H, W = frames[0]["coords"].shape

    def run(fr, assign, table, call0, hold_ms=None):
        real = torch.from_numpy(np.stack([x["coords"] for x in fr])).cuda()
        sc = real if hold_ms is None else torch.roll(real, 1, 0).contiguous()
        g = torch.zeros_like(real) if hold_ms is None else torch.full_like(real, 3.0)
        ha = torch.from_numpy(np.stack(assign)).cuda()
        p = engine.make_params(E, H, W, 128, shift_x=-77, shift_y=91, focal=1234.5, ppx=-5.0, ppy=9999.0, sub_sampling=fr[0]["sub"],
                               inlier_alpha=100.0, seed=1305, call=call0)
        torch.cuda.synchronize()
        if hold_ms is not None:
            _produce(sc, real, hold_ms)
            g.zero_()
        rec = engine.backward_batch(sc, g, ha, gts, 1.0, 100.0, 100.0, p, cams=table)
        torch.cuda.synchronize()
        return dict(rec=rec.copy(), grad=g.cpu().numpy(), probs=engine.read_frames(api.BUF_BWD_PROBS, 8),
                    hyps=engine.read_frames(api.BUF_BWD_REF_HYPS, 8), losses=engine.read_frames(api.BUF_BWD_LOSSES, 8))

    want = run(frames, has, cams, 40)
    assert want["rec"][:, 1].min() >= 1 and np.abs(want["grad"]).max() > 0
    run(others[0], others[1], others[2], 70)
    got = run(frames, has, cams, 40, hold_ms=1.5 * _bound_ms())
    for key in want:
        np.testing.assert_array_equal(got[key], want[key], err_msg=key)


# ---------------------------------------------------------------- the callers' surfaces
def test_drop_in_forward_with_cpu_tensors_behind_a_busy_stream(engine, oracle):
    """esac.forward with CPU tensors: the pinned staging copy and its asynchronous upload go onto the launch stream behind
    whatever it holds.  A speculative shape (3 experts, 512 hypotheses); the reference is the serial route of the same call."""
    import esac
    (f, other, _), (ha, ha_other, _) = _frames(4200, 3, 512)

    def call(frame, assign, counter, hold_ms=None):
        pose = torch.zeros(4, 4)
        esac.set_seed(1305, counter)
        torch.cuda.synchronize()
        if hold_ms is not None:
            _hold(hold_ms)
        expert = esac.forward(torch.from_numpy(frame["coords"]), torch.from_numpy(assign), pose, 0, 0, frame["focal"], frame["ppx"],
                              frame["ppy"], 10.0, 100.0, 0.5, 100.0, frame["sub"])
        torch.cuda.synchronize()
        last = esac.last_result()
        return dict(expert=expert, pose=pose.numpy().copy(), rec=last["result"].copy(), user=last["scores"].cpu().numpy(),
                    tries=engine.read(api.BUF_TRIES), hyps=engine.read(api.BUF_HYPS), speculative=engine.spec_info()["last_speculative"])

    engine.set_debug(no_speculation=True)
    try:
        want = call(f, ha, 21)
    finally:
        engine.set_debug()
    assert not want["speculative"]
    assert call(other, ha_other, 22)["speculative"]
    got = call(f, ha, 21, hold_ms=1.5 * _bound_ms())
    assert got["speculative"]
    for key in ("expert", "pose", "rec", "user", "tries", "hyps"):
        np.testing.assert_array_equal(got[key], want[key], err_msg=key)
    ref = oracle.forward(f["coords"], ha, focal=f["focal"], ppx=f["ppx"], ppy=f["ppy"], sub_sampling=f["sub"], seed=1305, call=21)
    assert got["expert"] == ref["expert"] and int(got["rec"][api.RES_HYP]) == ref["winner"]
    r_err, t_err = S.pose_errors(got["pose"], ref["pose"])
    assert r_err <= 1e-4 and t_err <= 1e-3, (r_err, t_err)


@pytest.mark.parametrize("N", [192, 512])
def test_forward_sharded_world1_behind_a_busy_stream(engine, N, monkeypatch):
    """The sharded forward (asynchronous calls, the library's own RCCL communicator, one all-reduce on the launch stream) at world
    size 1 behind the producer: winner record and global score vector of the idle call.  192 hypotheses: the selection runs in
    the team's prologue; 512: the speculative route in its asynchronous form."""
    import torch.distributed as dist
    from esac_amd import distributed as D
    monkeypatch.setenv("ESAC_NATIVE_RCCL", "1")
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    monkeypatch.setenv("MASTER_ADDR", "127.0.0.1")
    monkeypatch.setenv("MASTER_PORT", str(port))
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        (f, other, _), (ha, ha_other, _) = _frames(4300, 3, N)
        real, hat = torch.from_numpy(f["coords"]).cuda(), torch.from_numpy(ha).cuda()
        kw = dict(seed=1305, call=8)
        scores_g, best = D.forward_sharded(engine, real, hat, kw, policy="range")
        torch.cuda.synchronize()
        want_scores, want_best = scores_g.cpu().numpy().copy(), best.copy()
        assert engine._comm == (1, 0)
        D.forward_sharded(engine, torch.from_numpy(other["coords"]).cuda(), torch.from_numpy(ha_other).cuda(), dict(seed=1305, call=9), policy="range")
        sc = torch.from_numpy(other["coords"]).cuda()
        torch.cuda.synchronize()
        _produce(sc, real, 1.5 * _bound_ms())
        scores_g, best = D.forward_sharded(engine, sc, hat, kw, policy="range")
        torch.cuda.synchronize()
        np.testing.assert_array_equal(best[:31], want_best[:31])
        np.testing.assert_array_equal(scores_g.cpu().numpy(), want_scores)
        engine.check()
    finally:
        dist.destroy_process_group()


class _LateExpert(torch.nn.Module):
    """Stands in for an expert network that finishes late: the first one to run queues the hold on the current stream, and each
    returns its real coordinate map (harness.localize copies it into the prediction tensor on that stream, behind the hold)."""
    def __init__(self, coords, e, state, hold_ms):
        super().__init__()
        self.coords, self.e, self.state, self.hold_ms = coords, e, state, hold_ms

    def forward(self, image):
        if not self.state["held"]:
            self.state["held"] = True
            _hold(self.hold_ms)
        return self.coords[self.e:self.e + 1]


@pytest.mark.parametrize("hypotheses", [128, 512])
def test_harness_localize_behind_late_experts(oracle, hypotheses):
    """harness.localize with expert modules that enqueue their work and return: against the oracle on the very tensors it handed
    to esac.forward, same (seed, call) -- as test_harness_localize_against_the_oracle, with the stream held for 1.5 bounds."""
    import esac
    from esac_amd import harness
    E = 4
    gen = torch.Generator(device="cuda").manual_seed(11)
    for k in range(4):
        f = S.make_frame(4400 + k, E=E, true_expert=k % E)
        coords = torch.from_numpy(f["coords"]).cuda()
        logits = torch.full((1, E), -1.0, device="cuda")
        logits[0, k % E] = 3.0
        gating = lambda image, lg=torch.log_softmax(logits, dim=1): lg
        state = {"held": False}
        experts = [_LateExpert(coords, e, state, 1.5 * _bound_ms()) for e in range(E)]
        esac.set_seed(77, 10 + k)
        torch.cuda.synchronize()
        out = harness.localize(torch.zeros(1, 3, 480, 640, device="cuda"), gating, experts, f["focal"], hypotheses=hypotheses, generator=gen)
        assert state["held"]
        ref = oracle.forward(out["prediction"].cpu().numpy(), out["hyp_assignment"].cpu().numpy().copy(), seed=77, call=10 + k,
                             focal=f["focal"], ppx=320.0, ppy=240.0, sub_sampling=8)
        assert out["expert"] == ref["expert"] and esac.last_result()["winner"] == ref["winner"]
        r, t = S.pose_errors(out["pose"].numpy(), ref["pose"])
        assert r <= 1e-4 and t <= 1e-3, (k, r, t)
