"""GPU tests of ragged TRAINING batches: frames that differ in image size through esac_hip_backward_batch_shapes /
esac_hip_backward_batch_dev_shapes (`Engine.backward_batch_shapes`, `Engine.backward_batch_shapes_async`,
`esac.backward_batch_shapes`, `esac.backward_batch_shapes_async`, `harness.train_batch` with a list of images).

Contract: frame b of a ragged training batch is what `esac.backward` computes on that frame alone -- its own dense
[E,3,h_b,w_b] maps, its camera, RNG counter call + b, its own [E,3,h_b,w_b] gradient tensor accumulated with `+=`.  Every
frame is compared with the single call bit for bit on a context that refines slots with one workgroup each (ESAC_SLOT_TEAMS=0:
a batch never uses slot teams), and with the CPU oracle under the bars of tests/test_gpu_backward.py as restated by
tests/test_gpu_backward_batch.py (`_check_frame`, imported: no tolerance of this file's own).

Grids: 12x16 and 16x12 (equal P, transposed W: a wrong row stride shows), 12x18 (another P, and a W that is no multiple of 4:
the `shapes == 2` route; a wrong frame stride shows), frames `synthetic.make_frame(1000 + b, H=h, W=w)` with the principal point
at the frame's own centre as in tests/test_gpu_ragged.py:_inputs.  Every compared frame asserts at least one selected slot and no
probability within 1e-12 of 1e-3 (`_conditions`); the seeds were chosen with the oracle alone, on the CPU (at alpha 16 it selects
30 .. 64 of the 64 hypotheses per frame, the nearest probability 7e-6 from the threshold).
The oracle's bars were set on 60x80 grids; on 192 cells one cell carries 25 times the share of a score.  The frames from 900 were
the first candidates: there the SINGLE call on the fifth frame (16x12) already differs from the oracle by 1.0e-7 relative in one
of 64 probabilities (bar: 1e-8) -- the ragged batch gives that call's bits -- while the frames from 1000 hold every bar through the
single calls (LAB_NOTES "Ragged training batches").  The bars stay as they are; the frames are the ones the path as it was meets them on.
"""
import numpy as np
import pytest
import torch

import esac
from esac_amd import api, harness
from esac_amd import synthetic as S
from tests.test_gpu_backward_batch import _check_frame

pytestmark = pytest.mark.gpu

SEED, CALL0, SUB = 1305, 70, 8
MIXED = [(12, 16), (16, 12), (12, 18), (12, 16), (16, 12)]
E, N, ALPHA = 3, 64, 16.0
LOSS = (1.0, 100.0, 100.0)

_cache = {}


def _inputs(shapes, experts=E, n=N, first=1000):
    """(frames, assignments, ground truths) of a case, made once and never written to."""
    key = (tuple(shapes), experts, n, first)
    if key not in _cache:
        frames = [S.make_frame(first + b, E=experts, true_expert=b % experts, H=h, W=w, sub=SUB, ppx=w * SUB / 2.0, ppy=h * SUB / 2.0,
                               focal=525.0 + 10.0 * (b % 5), shift=(b % 3 - 1, (b % 2) * 2 - 1)) for b, (h, w) in enumerate(shapes)]
        has = [S.gating_assignment(f, n, mode="gating" if experts > 1 else "single") for f in frames]
        gts = []
        for b, f in enumerate(frames):
            gt = np.array(f["gt_pose"], np.float64)
            gt[:3, 3] += np.random.default_rng(400 + b).normal(size=3) * 0.05
            gts.append(gt.astype(np.float32))
        _cache[key] = (frames, has, gts)
    return _cache[key]


def _g0(frames, seed=9):
    """A non-zero initial gradient per frame: `+=` is visible."""
    rng = np.random.default_rng(seed)
    return [(rng.normal(size=f["coords"].shape) * 1e-3).astype(np.float32) for f in frames]


def _cams(frames):
    cams = api.make_cams([f["shift"][0] for f in frames], [f["shift"][1] for f in frames], [f["focal"] for f in frames],
                         [f["ppx"] for f in frames], [f["ppy"] for f in frames])
    cams["reserved"][:] = -12345  # (the padding of a camera table may hold anything: backward_batch_shapes fills its copy)
    return cams


def _table_params(eng, experts, H, W, n, alpha, call, **kw):
    """Parameter block of a batch with a table: the five camera fields are ignored, so they carry values no frame uses."""
    return eng.make_params(experts, H, W, n, shift_x=-77, shift_y=91, focal=1234.5, ppx=-5.0, ppy=9999.0, sub_sampling=SUB,
                           inlier_alpha=alpha, seed=SEED, call=call, **kw)


def _frame_params(eng, f, n, alpha, call, **kw):
    experts, _, H, W = f["coords"].shape
    return eng.make_params(experts, H, W, n, shift_x=f["shift"][0], shift_y=f["shift"][1], focal=f["focal"], ppx=f["ppx"], ppy=f["ppy"],
                           sub_sampling=SUB, inlier_alpha=alpha, seed=SEED, call=call, **kw)


FRAME_BUFS = (api.BUF_BWD_PROBS, api.BUF_BWD_REF_HYPS, api.BUF_BWD_LOSSES)


def _pack(eng, frames, g0, map_tail=0.0, grad_tail=0.0, grad_stride=None):
    experts = frames[0]["coords"].shape[0]
    packed, shapes = api.pack_frames([torch.from_numpy(f["coords"]) for f in frames], device=eng.device)
    grads = torch.zeros((len(frames), packed.shape[1] if grad_stride is None else grad_stride), dtype=torch.float32, device=eng.device)
    for b, (h, w) in enumerate(shapes):
        n = 3 * experts * h * w
        packed[b, n:] = map_tail
        grads[b, n:] = grad_tail
        grads[b, :n] = torch.from_numpy(g0[b]).reshape(-1).to(eng.device)
    return packed, grads, shapes


def _unpack(grads, shapes, experts):
    return [v.cpu().numpy().copy() for v in api.unpack_frames(grads, shapes, experts)]


def _run_ragged(eng, frames, has, gts, g0, alpha=ALPHA, call0=CALL0, asynchronous=False, pose_records=None, **kw):
    """The frames as ONE ragged training batch.  Returns dict(out [B,4], grads: list of [E,3,h,w], the per-frame buffers)."""
    B, n, experts = len(frames), len(has[0]), frames[0]["coords"].shape[0]
    tails = {k: kw.pop(k) for k in ("map_tail", "grad_tail", "grad_stride") if k in kw}
    held = kw.pop("frames_held", B)  # frames of the last chunk: what the per-frame buffers hold afterwards
    packed, grads, shapes = _pack(eng, frames, g0, **tails)
    H, W = kw.pop("capacity", None) or api.capacity_shape(shapes)  # (a capacity of the caller's own may exceed every frame)
    p = _table_params(eng, experts, H, W, n, alpha, call0, **kw)
    ha = torch.from_numpy(np.stack(has)).to(eng.device)
    if asynchronous:
        if pose_records is not None:
            eng.arm_pose_records(pose_records)
        out = eng.backward_batch_shapes_async(packed, grads, ha, torch.from_numpy(np.stack(gts)).to(eng.device), *LOSS, p, shapes,
                                              cams=_cams(frames))
        torch.cuda.synchronize()
        eng.check()
        out = out.cpu().numpy()
    else:
        out = eng.backward_batch_shapes(packed, grads, ha, np.stack(gts), *LOSS, p, shapes, cams=_cams(frames), pose_records=pose_records)
    res = dict(out=out, grads=_unpack(grads, shapes, experts), packed_grads=grads, shapes=shapes)
    for which in FRAME_BUFS:
        res[which] = eng.read_frames(which, held)
    return res


def _run_singles(eng, frames, has, gts, g0, alpha=ALPHA, call0=CALL0, pose_records=False, **kw):
    """The single `backward_device` calls on each frame's dense tensors at counters call0 + b."""
    res = dict(out=[], grads=[], records=[])
    res.update({which: [] for which in FRAME_BUFS})
    for b, f in enumerate(frames):
        sc = torch.from_numpy(f["coords"]).to(eng.device)
        g = torch.from_numpy(g0[b].copy()).to(eng.device)
        rec = torch.zeros(api.RES_DOUBLES, dtype=torch.float64, device=eng.device) if pose_records else None
        res["out"].append(eng.backward_device(sc, g, torch.from_numpy(has[b]).to(eng.device), gts[b], *LOSS,
                                              _frame_params(eng, f, len(has[b]), alpha, call0 + b, **kw), pose_record=rec))
        res["grads"].append(g.cpu().numpy())
        if pose_records:
            res["records"].append(rec.cpu().numpy())
        for which in FRAME_BUFS:
            res[which].append(eng.read(which))
    res["out"] = np.stack(res["out"])
    return res


def _assert_same_bits(a, b, what):
    for k in range(len(b["grads"])):  # (printed before anything is asserted: which frame, which output)
        same = [bool(np.array_equal(a["out"][k], b["out"][k]))] + [bool(np.array_equal(a[w][k], b[w][k])) for w in FRAME_BUFS] + \
            [bool(np.array_equal(a["grads"][k], b["grads"][k]))]
        if not all(same):
            print("%s: frame %d %s record/probs/ref_hyps/losses/gradients equal: %s, record diff %s"
                  % (what, k, a["grads"][k].shape, same, np.asarray(a["out"][k]) - np.asarray(b["out"][k])))
    np.testing.assert_array_equal(a["out"], b["out"], err_msg=what)
    for which in FRAME_BUFS:
        np.testing.assert_array_equal(a[which], np.stack(b[which]), err_msg="%s buffer %d" % (what, which))
    assert len(a["grads"]) == len(b["grads"])
    for k, (x, y) in enumerate(zip(a["grads"], b["grads"])):
        assert x.shape == y.shape
        np.testing.assert_array_equal(x, y, err_msg="%s: gradients of frame %d" % (what, k))


def _conditions(res, g0):
    """Every compared frame: at least one selected slot, no probability on the selection threshold, a gradient that moved."""
    for b, probs in enumerate(res[api.BUF_BWD_PROBS]):
        assert res["out"][b][1] >= 1, b
        assert not (np.abs(np.asarray(probs) - 1e-3) < 1e-12).any(), b
        assert np.abs(res["grads"][b] - g0[b]).max() > 0, b


@pytest.fixture(scope="module")
def solo():
    """A context that refines slots with one workgroup each, as every batch does."""
    import os
    before = os.environ.get("ESAC_SLOT_TEAMS")
    os.environ["ESAC_SLOT_TEAMS"] = "0"
    try:
        eng = api.Engine(0)
    finally:
        if before is None:
            del os.environ["ESAC_SLOT_TEAMS"]
        else:
            os.environ["ESAC_SLOT_TEAMS"] = before
    return eng


@pytest.fixture(scope="module")
def mixed(solo):
    """The mixed batch and its single calls, computed once and shared (never written to)."""
    frames, has, gts = _inputs(MIXED)
    g0 = _g0(frames)
    return dict(frames=frames, has=has, gts=gts, g0=g0, ragged=_run_ragged(solo, frames, has, gts, g0),
                singles=_run_singles(solo, frames, has, gts, g0))


# ---------------------------------------------------------------- 1. single calls, bit for bit
def test_mixed_batch_equals_the_single_calls_bit_for_bit(mixed):
    _conditions(mixed["ragged"], mixed["g0"])
    _conditions(mixed["singles"], mixed["g0"])
    _assert_same_bits(mixed["ragged"], mixed["singles"], "ragged batch vs single calls")
    assert [g.shape for g in mixed["ragged"]["grads"]] == [(E, 3) + s for s in MIXED]


# ---------------------------------------------------------------- 2. the CPU oracle
def test_every_frame_matches_the_oracle(mixed, oracle):
    r = mixed["ragged"]
    _conditions(r, mixed["g0"])
    for b, f in enumerate(mixed["frames"]):
        g_ref = mixed["g0"][b].copy()
        ref = oracle.backward(f["coords"], g_ref, mixed["has"][b], mixed["gts"][b], w_rot=LOSS[0], w_trans=LOSS[1], loss_cut=LOSS[2],
                              shift_x=f["shift"][0], shift_y=f["shift"][1], focal=f["focal"], ppx=f["ppx"], ppy=f["ppy"],
                              sub_sampling=SUB, inlier_alpha=ALPHA, seed=SEED, call=CALL0 + b)
        assert (ref["probs"] >= 1e-3).sum() >= 1 and not (np.abs(ref["probs"] - 1e-3) < 1e-12).any(), b
        slots = _check_frame(r["out"][b], r["grads"][b], ref, g_ref, r[api.BUF_BWD_PROBS][b], r[api.BUF_BWD_REF_HYPS][b],
                             r[api.BUF_BWD_LOSSES][b], mixed["g0"][b])
        assert slots >= 1 and slots == int(r["out"][b][1]), b


# ---------------------------------------------------------------- 3. a uniform table is the old batch; B = 1
@pytest.mark.parametrize("shape", [(12, 16), (12, 18)], ids=["w16", "w18"])
def test_uniform_table_is_backward_batch_cams_bit_for_bit(solo, shape):
    B = 3
    frames, has, gts = _inputs([shape] * B, first=920)
    g0 = _g0(frames)
    new = _run_ragged(solo, frames, has, gts, g0)
    _conditions(new, g0)

    def dense(k):
        sc = torch.from_numpy(np.stack([f["coords"] for f in frames[:k]])).cuda()
        g = torch.from_numpy(np.stack(g0[:k])).cuda()
        out = solo.backward_batch(sc, g, torch.from_numpy(np.stack(has[:k])).cuda(), np.stack(gts[:k]), *LOSS,
                                  _table_params(solo, E, shape[0], shape[1], N, ALPHA, CALL0), cams=_cams(frames[:k]))
        res = dict(out=out, grads=list(g.cpu().numpy()))
        for which in FRAME_BUFS:
            res[which] = list(solo.read_frames(which, k))
        return res
    _assert_same_bits(new, dense(B), "uniform table vs backward_batch with cams")
    one = _run_ragged(solo, frames[:1], has[:1], gts[:1], g0[:1])
    _assert_same_bits(one, dense(1), "B = 1")
    np.testing.assert_array_equal(one["out"][0], new["out"][0])
    np.testing.assert_array_equal(one["grads"][0], new["grads"][0])


def _run_single(eng, f, ha, gt, g0, call, n):
    """`backward_device` on one frame's dense tensors: (record [4], gradients [E,3,h,w])."""
    g = torch.from_numpy(g0.copy()).to(eng.device)
    out = eng.backward_device(torch.from_numpy(f["coords"]).to(eng.device), g, torch.from_numpy(ha).to(eng.device), gt, *LOSS,
                              _frame_params(eng, f, n, ALPHA, call))
    return out, g.cpu().numpy()


@pytest.mark.parametrize("asynchronous", [False, True], ids=["blocking", "async"])
def test_one_ragged_frame_is_the_single_backward_on_its_grid(solo, asynchronous):
    """B = 1 under a capacity larger than the frame (12x18 over 9x14): the host hands the call to the shared-shape route on the
    frame's OWN grid.  14 is no multiple of 4 -- a call that kept the ragged mode of such a table, or the capacity's row
    length, would not give the single call's bits.  (test_uniform_table_is_backward_batch_cams_bit_for_bit holds B = 1 against
    backward_batch at the capacity's own shape, blocking only.)"""
    n = 16
    frames, has, gts = _inputs([(9, 14)], experts=1, n=n, first=975)  # (the oracle selects 12 of the 16, none near the threshold)
    g0 = _g0(frames, seed=14)
    got = _run_ragged(solo, frames, has, gts, g0, call0=600, asynchronous=asynchronous, capacity=(12, 18))
    _conditions(got, g0)
    want_out, want_g = _run_single(solo, frames[0], has[0], gts[0], g0[0], 600, n)
    print("record: ragged", got["out"][0], "single", want_out, "max |gradient difference|", np.abs(got["grads"][0] - want_g).max())
    np.testing.assert_array_equal(got["out"][0], want_out)
    assert got["grads"][0].shape == (1, 3, 9, 14)
    np.testing.assert_array_equal(got["grads"][0], want_g)
    for which in FRAME_BUFS:
        np.testing.assert_array_equal(got[which][0], solo.read(which), err_msg="buffer %d" % which)


# ---------------------------------------------------------------- 4. slot tails are untouched
def test_slot_tails_are_neither_read_nor_written(solo, mixed):
    SENTINEL = -4242.5
    stride = api.packed_stride(E, MIXED) + 12  # (a gradient stride of the caller's own, beyond the maps')
    got = _run_ragged(solo, mixed["frames"], mixed["has"], mixed["gts"], mixed["g0"], map_tail=float("nan"), grad_tail=SENTINEL,
                      grad_stride=stride)
    _assert_same_bits(got, mixed["ragged"], "NaN map tails, sentinel gradient tails")
    _conditions(got, mixed["g0"])
    g = got["packed_grads"].cpu().numpy()
    assert g.shape == (len(MIXED), stride)
    for b, (h, w) in enumerate(MIXED):
        tail = g[b, 3 * E * h * w:]
        assert tail.size >= 12 and (tail == SENTINEL).all(), b
    assert sorted({h * w for h, w in MIXED}) == [192, 216]  # frames below the capacity exist: their tails are 72 floats and more


# ---------------------------------------------------------------- 5. chunking
def test_chunks_of_two_equal_one_chunk(solo, monkeypatch):
    """A slot is charged 2 P + 48 P bytes at the CAPACITY P = 13 * 18 = 234, whatever the frame; a fresh context starts with 64
    slots per frame: a budget of 2 MiB holds two frames and not three, so B = 5 goes as 2 + 2 + 1."""
    shapes = [(12, 16), (16, 12), (12, 18), (13, 18), (16, 12)]
    per_frame = 50 * 234 * 64
    assert 2 * per_frame <= 2 << 20 < 3 * per_frame
    frames, has, gts = _inputs(shapes, first=930)
    g0 = _g0(frames, seed=10)
    whole = _run_ragged(solo, frames, has, gts, g0, call0=200)
    _conditions(whole, g0)
    monkeypatch.setenv("ESAC_BWD_BATCH_BUDGET_MB", "2")
    monkeypatch.setenv("ESAC_SLOT_TEAMS", "0")
    small = api.Engine(0)
    got = _run_ragged(small, frames, has, gts, g0, call0=200, frames_held=1)  # the last chunk of 2 + 2 + 1 holds ONE frame ...
    with pytest.raises(RuntimeError):
        small.read_frames(api.BUF_BWD_PROBS, 2)                               # ... and not two
    np.testing.assert_array_equal(got["out"], whole["out"])
    for b in range(len(shapes)):
        np.testing.assert_array_equal(got["grads"][b], whole["grads"][b], err_msg="frame %d" % b)
    for which in FRAME_BUFS:  # the last chunk's frame 0 is the batch's frame 4: its table pointer and counter moved with the chunk
        np.testing.assert_array_equal(got[which][0], whole[which][4])


def test_slot_reads_after_a_chunked_batch_are_the_last_chunks_frame_0(solo, monkeypatch):
    """esac_hip_read of the slot maps and the slabs after a batch that went in chunks: the slots of the LAST chunk's frame 0 (here
    the batch's frame 2, 12x18) in that frame's own 216 cells -- not the batch's frame 0 (192 cells), not the capacity (234).
    A slot is charged 50 P bytes at the capacity P = 13 * 18, a fresh context starts with 64 slots per frame: 2 MiB hold two
    frames and not three, so B = 3 goes as 2 + 1.  The yardstick is the single call on frame 2, whose bits the batch gives."""
    shapes = [(12, 16), (9, 14), (12, 18)]
    per_frame = 50 * 234 * 64
    assert 2 * per_frame <= 2 << 20 < 3 * per_frame
    frames, has, gts = _inputs(shapes, first=980)  # (the oracle selects 40, 37 and 30 of the 64: no overflow rerun)
    g0 = _g0(frames, seed=15)
    monkeypatch.setenv("ESAC_BWD_BATCH_BUDGET_MB", "2")
    monkeypatch.setenv("ESAC_SLOT_TEAMS", "0")
    small = api.Engine(0)
    got = _run_ragged(small, frames, has, gts, g0, call0=500, frames_held=1, capacity=(13, 18))
    _conditions(got, g0)
    with pytest.raises(RuntimeError):
        small.read_frames(api.BUF_BWD_PROBS, 2)  # the last chunk holds ONE frame
    k = int(got["out"][2][1])
    assert 1 <= k <= 64
    info = small.read_frames(api.BUF_BWD_SLOT_INFO, 1)[0][:k]
    maps = small.read_maps(k, shape=shapes[2])
    slabs = [small.read_slabs(w, k, shape=shapes[2]) for w in (api.BUF_BWD_PATH1, api.BUF_BWD_PATH2)]
    for other in (shapes[0], (13, 18)):  # a slot is 2 * 216 bytes: one slot in the batch's frame 0's unit, or the capacity's, is refused
        with pytest.raises(RuntimeError, match="whole slots of 432 bytes"):
            small.read_maps(1, shape=other)
    want_out, want_g = _run_single(solo, frames[2], has[2], gts[2], g0[2], 502, N)
    np.testing.assert_array_equal(got["out"][2], want_out)
    np.testing.assert_array_equal(got["grads"][2], want_g)
    want_info = solo.read(api.BUF_BWD_SLOT_INFO)[:k]
    want_maps = solo.read_maps(k)
    print("slots", k, "accepted maps", int((info[:, 0] >= 0).sum()), "inliers", info[:, 1].tolist())
    np.testing.assert_array_equal(info, want_info)
    assert (info[:, 0] >= 0).sum() >= 1
    for s in range(k):
        if info[s, 0] >= 0:  # (the other buffer of a slot holds an earlier iteration's set, or an earlier call's)
            np.testing.assert_array_equal(maps[s, info[s, 0]], want_maps[s, info[s, 0]], err_msg="slot %d" % s)
            assert maps[s, info[s, 0]].any(), s
    for w, have in zip((api.BUF_BWD_PATH1, api.BUF_BWD_PATH2), slabs):
        np.testing.assert_array_equal(have, solo.read_slabs(w, k), err_msg="slabs %d" % w)
        assert np.abs(have).max() > 0


# ---------------------------------------------------------------- 6. overflow rerun
def test_overflow_rerun_adds_nothing_twice(solo, monkeypatch):
    """A low alpha flattens the distribution: with N = 96 every hypothesis of the small frames passes 1e-3, beyond the 64 slots
    per frame a fresh context starts with.  The aborted pass adds nothing; the rerun equals the single calls."""
    shapes = [(12, 16), (12, 18), (16, 12)]
    frames, has, gts = _inputs(shapes, n=96, first=940)
    g0 = _g0(frames, seed=11)
    alpha = 0.5
    monkeypatch.setenv("ESAC_SLOT_TEAMS", "0")
    fresh = api.Engine(0)
    got = _run_ragged(fresh, frames, has, gts, g0, alpha=alpha, call0=300)
    assert got["out"][:, 1].max() > 64, got["out"][:, 1]
    _conditions(got, g0)
    singles = _run_singles(solo, frames, has, gts, g0, alpha=alpha, call0=300)
    _assert_same_bits(got, singles, "overflow rerun vs single calls")


# ---------------------------------------------------------------- 7. the global-list route
def test_global_list_frame_beside_a_small_one(solo):
    """96x88 = 8448 cells > ESAC_REFINE_LDS_CAP: the capacity puts every frame's slot refinement on the global correspondence
    list; the small frame's single call uses the LDS list -- the same correspondences in the same order."""
    shapes = [(12, 18), (96, 88), (12, 16)]
    frames, has, gts = _inputs(shapes, experts=1, n=16, first=960)
    g0 = _g0(frames, seed=13)
    got = _run_ragged(solo, frames, has, gts, g0, alpha=ALPHA, call0=400)
    _conditions(got, g0)
    _assert_same_bits(got, _run_singles(solo, frames, has, gts, g0, alpha=ALPHA, call0=400), "global list")


# ---------------------------------------------------------------- 8. the asynchronous route; refused tables
def test_asynchronous_route_equals_the_blocking_call(solo, mixed):
    got = _run_ragged(solo, mixed["frames"], mixed["has"], mixed["gts"], mixed["g0"], asynchronous=True)
    _assert_same_bits(got, mixed["ragged"], "asynchronous vs blocking")
    _conditions(got, mixed["g0"])


@pytest.mark.parametrize("asynchronous", [False, True], ids=["blocking", "async"])
@pytest.mark.parametrize("bad", ["camera", "gradient stride"])
def test_a_refused_table_draws_no_counter_and_leaves_the_gradients(solo, mixed, monkeypatch, asynchronous, bad):
    monkeypatch.setitem(api._state, "engines", {0: solo})
    frames, has, gts = mixed["frames"], mixed["has"], mixed["gts"]
    packed, grads, shapes = _pack(solo, frames, mixed["g0"])
    before = grads.clone()
    fn = esac.backward_batch_shapes_async if asynchronous else esac.backward_batch_shapes
    ha = torch.from_numpy(np.stack(has)).cuda()
    gt = torch.from_numpy(np.stack(gts))
    shift_x = [0] * len(frames)
    if bad == "camera":
        # sub 8, w = 18: the last column's centre is 140 - shift_x -- one beyond int32 for frame 2 alone
        shift_x[2] = -(2**31 - 1 - 140) - 1
        needle = "pixel positions overflow int32"
    else:
        grads = grads[:, :3 * E * 216 - 4].contiguous()  # long enough for the 192-cell frames, 4 floats short for frame 2
        before = grads.clone()
        needle = "outGradients"
    esac.set_seed(SEED, 555)
    with pytest.raises(RuntimeError) as e:
        fn(packed, grads, ha, gt.cuda() if asynchronous else gt, *LOSS, shift_x, 0, 525.0, [f["ppx"] for f in frames],
           [f["ppy"] for f in frames], 10.0, ALPHA, 0.5, 100.0, SUB, shapes=shapes, experts=E)
    assert needle in str(e.value) and (bad != "camera" or "frame 2" in str(e.value)), str(e.value)
    torch.cuda.synchronize()
    assert esac.get_rng_state() == (SEED, 555)
    assert torch.equal(grads, before)


def test_the_library_refuses_a_short_gradient_stride_itself(solo, mixed):
    """Past the Python checks (Engine level, a strided view): the C ABI names the frame, nothing is launched."""
    frames = mixed["frames"]
    packed, grads, shapes = _pack(solo, frames, mixed["g0"])
    before = grads.clone()
    lib, B = solo.lib, len(frames)
    cams = _cams(frames)
    cams["reserved"][:, :2] = np.asarray(shapes, np.int32)
    p = _table_params(solo, E, 12, 18, N, ALPHA, 9)
    ha = torch.from_numpy(np.stack(mixed["has"])).cuda()
    gt = np.ascontiguousarray(np.stack(mixed["gts"]).reshape(-1))
    host = np.zeros((B, 4))
    import ctypes as C
    rc = lib.esac_hip_backward_batch_shapes(solo.ctx, B, packed.data_ptr(), int(packed.stride(0)), grads.data_ptr(), 3 * E * 216 - 1,
                                            ha.data_ptr(), gt.ctypes.data, cams.ctypes.data, 1.0, 100.0, 100.0, C.byref(p), None,
                                            host.ctypes.data)
    msg = lib.esac_hip_last_error().decode()
    assert rc == -4 and "esac_hip_backward_batch_shapes: the gradients of frame 2" in msg and "grad_frame_stride = 1943" in msg, (rc, msg)
    torch.cuda.synchronize()
    assert torch.equal(grads, before) and not host.any()


# ---------------------------------------------------------------- 9. pose records
@pytest.mark.parametrize("asynchronous", [False, True], ids=["blocking", "async"])
def test_armed_batch_gives_the_armed_single_calls_records(solo, mixed, asynchronous):
    B = len(MIXED)
    records = torch.full((B, api.RES_DOUBLES), -1.0, dtype=torch.float64, device="cuda")
    got = _run_ragged(solo, mixed["frames"], mixed["has"], mixed["gts"], mixed["g0"], pose_records=records, asynchronous=asynchronous)
    singles = _run_singles(solo, mixed["frames"], mixed["has"], mixed["gts"], mixed["g0"], pose_records=True)
    _assert_same_bits(got, singles, "armed batch vs armed single calls")
    _assert_same_bits(got, mixed["ragged"], "armed vs unarmed batch")
    rec = records.cpu().numpy()
    for b in range(B):
        np.testing.assert_array_equal(rec[b], singles["records"][b], err_msg="record of frame %d" % b)
        assert rec[b][api.RES_VALID] == 1.0 and np.isfinite(rec[b][api.RES_POSE:api.RES_POSE + 16]).all(), b


# ---------------------------------------------------------------- 10. strict training
def test_strict_mixed_batch_equals_the_strict_single_calls(solo, mixed):
    got = _run_ragged(solo, mixed["frames"], mixed["has"], mixed["gts"], mixed["g0"], strict_training=True)
    singles = _run_singles(solo, mixed["frames"], mixed["has"], mixed["gts"], mixed["g0"], strict_training=True)
    _conditions(got, mixed["g0"])
    _assert_same_bits(got, singles, "strict batch vs strict single calls")


# ---------------------------------------------------------------- 11. harness.train_batch with a list of images
class _FrameNet(torch.nn.Module):
    """A learnable map per frame, looked up by the index every pixel of the frame's image carries (the network side is a
    lookup: it rounds the same whatever the batch, so the solver's gradients reach the parameters unchanged)."""

    def __init__(self, maps):
        super().__init__()
        self.maps = torch.nn.ParameterList([torch.nn.Parameter(torch.from_numpy(np.ascontiguousarray(m)).cuda()) for m in maps])
        self.calls = []

    def forward(self, images):
        self.calls.append(tuple(images.shape))
        idx = images[:, 0, images.size(2) // 2, images.size(3) // 2].round().long().tolist()
        return torch.stack([self.maps[i] for i in idx])


class _FrameGating(torch.nn.Module):
    def __init__(self, logits):
        super().__init__()
        self.logits = torch.nn.Parameter(torch.tensor(logits, dtype=torch.float32).cuda())

    def forward(self, images):
        idx = images[:, 0, images.size(2) // 2, images.size(3) // 2].round().long()
        return torch.log_softmax(self.logits[idx], dim=1)


@pytest.mark.parametrize("asynchronous", [False, True], ids=["blocking", "async"])
def test_train_batch_with_mixed_images_equals_train_step_per_image(solo, mixed, monkeypatch, asynchronous):
    """The bar of tests/test_gpu_batch_cams.py::test_train_batch_equals_single_backward_calls: losses, gradients and parameter
    gradients equal, bit for bit, on a context that refines one workgroup per slot."""
    monkeypatch.setitem(api._state, "engines", {0: solo})
    frames, has, gts = mixed["frames"], mixed["has"], mixed["gts"]
    B = len(frames)
    shifts = [f["shift"] for f in frames]
    focals = [f["focal"] for f in frames]
    images = [torch.full((1, 3, h * SUB, w * SUB), float(b), device="cuda") for b, (h, w) in enumerate(MIXED)]
    e_hyps = torch.from_numpy(np.stack(has)).cuda()
    kw = dict(hypotheses=N, inlier_alpha=ALPHA, subsample=SUB)

    def nets():
        return [_FrameNet([f["coords"][e] for f in frames]) for e in range(E)], _FrameGating(np.random.default_rng(5).normal(size=(B, E)))
    experts, gating = nets()
    esac.set_seed(SEED, CALL0)
    out = harness.train_batch(images, np.stack(gts), gating, experts, focals, shifts=shifts, e_hyps=e_hyps, asynchronous=asynchronous,
                              all_experts=asynchronous, **kw)
    torch.cuda.synchronize()
    assert esac.get_rng_state() == (SEED, CALL0 + B) and out["shapes"] == MIXED
    groups = len({s for s in MIXED})
    assert all(1 <= len(n.calls) <= groups for n in experts)  # once per image-size group at the most, never once per image
    losses = out["losses"].cpu().tolist() if asynchronous else out["losses"]
    batch_grads = _unpack(out["prediction_gradients"], MIXED, E)
    # the yardstick: train_step per image, same shifts, assignments and counters
    step_experts, step_gating = nets()
    esac.set_seed(SEED, CALL0)
    for b in range(B):
        step = harness.train_step(images[b], gts[b], step_gating, step_experts, focals[b], shift=shifts[b], **_step_kw(kw, e_hyps[b]))
        assert step["loss"] == losses[b], (b, step["loss"], losses[b])
        np.testing.assert_array_equal(step["prediction_gradients"].cpu().numpy(), batch_grads[b], err_msg="frame %d" % b)
        assert np.abs(batch_grads[b]).max() > 0
    for e in range(E):
        for b in range(B):
            want, got = step_experts[e].maps[b].grad, experts[e].maps[b].grad
            if want is None:
                assert got is None or not got.any(), (e, b)
            else:
                np.testing.assert_array_equal(got.cpu().numpy(), want.cpu().numpy(), err_msg="expert %d frame %d" % (e, b))
    np.testing.assert_array_equal(gating.logits.grad.cpu().numpy(), step_gating.logits.grad.cpu().numpy())
    assert np.abs(gating.logits.grad.cpu().numpy()).max() > 0


class _GivenDraws:
    """train_step takes no assignment and draws its own: this stands in for its `generator` and carries the row the draw must
    return (`_multinomial_takes_given_draws` below hands it out)."""

    def __init__(self, row):
        self.row = row


def _step_kw(kw, e_hyps_row):
    return dict(kw, generator=_GivenDraws(e_hyps_row))


@pytest.fixture(autouse=True)
def _multinomial_takes_given_draws(monkeypatch):
    real = torch.multinomial

    def multinomial(probs, n, replacement=False, generator=None):
        if isinstance(generator, _GivenDraws):
            assert generator.row.numel() == n
            return generator.row.clone()
        return real(probs, n, replacement=replacement, generator=generator)
    monkeypatch.setattr(torch, "multinomial", multinomial)
