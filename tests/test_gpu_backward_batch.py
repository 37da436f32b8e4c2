"""GPU tests of the batched training path: esac_hip_backward_batch (through `Engine.backward_batch` / `esac.backward_batch`).

Frame b of a batch is the b-th of B consecutive `esac.backward` calls (call counter call0 + b): every frame is checked against
the CPU oracle at that counter with the bars of tests/test_gpu_backward.py, and against the single calls themselves bit for
bit where both refine their slots with one workgroup each.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from esac_amd import api
from esac_amd import synthetic as S

pytestmark = pytest.mark.gpu

# the bars of tests/test_gpu_backward.py (see there for why)
GRAD_RTOL = 2e-6
GRAD_RTOL_SAMPLED = 1e-3
LOSS_RTOL = 1e-7


def _gt(frame, seed, noise=0.05):
    gt = np.array(frame["gt_pose"], np.float64)
    gt[:3, 3] += np.random.default_rng(seed).normal(size=3) * noise
    return gt.astype(np.float32)


def _params(eng, f, N, alpha, call, seed=1305, **kw):
    E, _, H, W = f["coords"].shape
    return eng.make_params(E, H, W, N, shift_x=f["shift"][0], shift_y=f["shift"][1], focal=f["focal"], ppx=f["ppx"],
                           ppy=f["ppy"], sub_sampling=f["sub"], inlier_alpha=alpha, seed=seed, call=call, **kw)


def _oracle(oracle, coords, f, ha, gt, alpha, call, seed=1305, g0=None, w_rot=1.0, w_trans=100.0, cut=100.0):
    g = np.zeros_like(coords) if g0 is None else g0.copy()
    ref = oracle.backward(coords, g, ha, gt, w_rot=w_rot, w_trans=w_trans, loss_cut=cut, shift_x=f["shift"][0],
                          shift_y=f["shift"][1], focal=f["focal"], ppx=f["ppx"], ppy=f["ppy"], sub_sampling=f["sub"],
                          inlier_alpha=alpha, seed=seed, call=call)
    return ref, g


def _run_batch(eng, frames, has, gts, alpha, call0, shared=None, g0=None, seed=1305):
    """One batched call; returns (records [B,4], gradients [B,E,3,H,W] as numpy)."""
    f0 = frames[0]
    sc = torch.from_numpy(shared if shared is not None else np.stack([f["coords"] for f in frames])).cuda()
    ha = torch.from_numpy(np.stack(has)).cuda()
    B = len(has)
    shape = (B,) + f0["coords"].shape
    g = torch.from_numpy(g0.copy()).cuda() if g0 is not None else torch.zeros(shape, dtype=torch.float32, device="cuda")
    p = _params(eng, f0, ha.shape[1], alpha, call0, seed=seed)
    out = eng.backward_batch(sc, g, ha, np.stack(gts), 1.0, 100.0, 100.0, p)
    return out, g.cpu().numpy()


def _check_frame(out, g_dev, ref, g_ref, probs, ref_hyps, losses, g_init=None):
    """Frame-level parity with the oracle: record, distribution, refined poses, losses and the gradient tensor."""
    assert abs(out[2] - ref["entropy"]) < 1e-9
    np.testing.assert_allclose(probs, ref["probs"], rtol=1e-8, atol=1e-14)
    sel_ref = np.nonzero(ref["probs"] >= 1e-3)[0]
    edge = np.abs(ref["probs"] - 1e-3) < 1e-12
    if not edge.any():
        assert int(out[1]) == len(sel_ref), (out[1], len(sel_ref))
    np.testing.assert_allclose(ref_hyps, ref["ref_hyps"], rtol=0, atol=1e-6)
    np.testing.assert_allclose(losses, ref["losses"], rtol=1e-6, atol=1e-6)
    assert abs(out[0] - ref["loss"]) <= LOSS_RTOL * max(1.0, abs(ref["loss"])), (out[0], ref["loss"])
    assert out[3] == 0.0
    contrib = g_ref if g_init is None else g_ref - g_init
    scale = max(float(np.abs(contrib).max()), 1e-30)
    E, _, H, W = g_ref.shape
    sampled = np.zeros((H, W), bool)
    for h in sel_ref:
        for x, y in ref["sample_xy"][h]:
            sampled[y, x] = True
    diff = np.abs(g_dev - g_ref)
    err = float(diff[:, :, ~sampled].max()) / scale
    err_s = float(diff[:, :, sampled].max()) / scale if sampled.any() else 0.0
    assert err <= GRAD_RTOL, (err, scale)
    assert err_s <= GRAD_RTOL_SAMPLED, (err_s, scale)
    assert np.isfinite(g_dev).all()
    return len(sel_ref)


def _check_all(eng, oracle, frames, has, gts, alpha, call0, out, g, shared=None, g0=None):
    B = len(has)
    probs = eng.read_frames(api.BUF_BWD_PROBS, B)
    refh = eng.read_frames(api.BUF_BWD_REF_HYPS, B)
    losses = eng.read_frames(api.BUF_BWD_LOSSES, B)
    slots = []
    for b in range(B):
        coords = shared if shared is not None else frames[b]["coords"]
        ref, g_ref = _oracle(oracle, coords, frames[b], has[b], gts[b], alpha, call0 + b, g0=None if g0 is None else g0[b])
        slots.append(_check_frame(out[b], g[b], ref, g_ref, probs[b], refh[b], losses[b], None if g0 is None else g0[b]))
    return slots


@pytest.mark.parametrize("case", ["one_expert", "gating"])
def test_batch_every_frame_matches_the_oracle(engine, oracle, case):
    """B = 4 frames with different ground truths (cfg2-style: 1 expert, 256 hypotheses), and 3 experts with a different gating
    assignment per frame: frame b against the oracle at call0 + b."""
    if case == "one_expert":
        frames = [S.make_frame(200 + b) for b in range(4)]
        has = [S.gating_assignment(f, 256) for f in frames]
        alpha = 100.0
    else:
        frames = [S.make_frame(210 + b, E=3, true_expert=b % 3) for b in range(4)]
        has = [S.gating_assignment(f, 64, mode="gating") for f in frames]
        alpha = 20.0
        assert len({tuple(h) for h in has}) == 4
    gts = [_gt(f, 300 + b) for b, f in enumerate(frames)]
    out, g = _run_batch(engine, frames, has, gts, alpha, call0=41)
    slots = _check_all(engine, oracle, frames, has, gts, alpha, 41, out, g)
    assert max(slots) >= 1
    assert np.abs(g).max() > 0


def test_batch_equals_sequential_calls_bit_for_bit(oracle, monkeypatch):
    """On a context that refines slots with one workgroup each (ESAC_SLOT_TEAMS=0) a batch of 6 equals 6 sequential single
    calls with counters call0 .. call0 + 5 bit for bit -- records, refined poses, gradients; B = 1 equals one single call; a
    default context (slot teams for <= 32 slots) agrees to the bound of test_slot_teams_equal_one_workgroup_per_slot."""
    monkeypatch.setenv("ESAC_SLOT_TEAMS", "0")
    solo = api.Engine(0)
    monkeypatch.delenv("ESAC_SLOT_TEAMS")
    teams = api.Engine(0)
    frames = [S.make_frame(220 + b) for b in range(6)]
    has = [S.gating_assignment(f, 96) for f in frames]
    gts = [_gt(f, 320 + b) for b, f in enumerate(frames)]
    call0, alpha = 7, 30.0
    out, g = _run_batch(solo, frames, has, gts, alpha, call0)
    refh = solo.read_frames(api.BUF_BWD_REF_HYPS, 6)
    probs = solo.read_frames(api.BUF_BWD_PROBS, 6)
    seq_out, seq_g = [], []
    for b, f in enumerate(frames):
        sc = torch.from_numpy(f["coords"]).cuda()
        gb = torch.zeros_like(sc)
        o = solo.backward_device(sc, gb, torch.from_numpy(has[b]).cuda(), gts[b], 1.0, 100.0, 100.0,
                                 _params(solo, f, 96, alpha, call0 + b))
        seq_out.append(o)
        seq_g.append(gb.cpu().numpy())
        np.testing.assert_array_equal(solo.read(api.BUF_BWD_REF_HYPS), refh[b])  # initial hypotheses + refined slots
        np.testing.assert_array_equal(solo.read(api.BUF_BWD_PROBS), probs[b])
    np.testing.assert_array_equal(out, np.stack(seq_out))
    np.testing.assert_array_equal(g, np.stack(seq_g))
    assert out[:, 1].min() >= 1
    # B = 1
    out1, g1 = _run_batch(solo, frames[:1], has[:1], gts[:1], alpha, call0)
    np.testing.assert_array_equal(out1[0], seq_out[0])
    np.testing.assert_array_equal(g1[0], seq_g[0])
    # against the default single call (slot teams)
    for b, f in enumerate(frames):
        sc = torch.from_numpy(f["coords"]).cuda()
        gb = torch.zeros_like(sc)
        o = teams.backward_device(sc, gb, torch.from_numpy(has[b]).cuda(), gts[b], 1.0, 100.0, 100.0,
                                  _params(teams, f, 96, alpha, call0 + b))
        assert o[1] == out[b, 1] and o[2] == out[b, 2]
        assert abs(o[0] - out[b, 0]) <= 1e-9 * max(1.0, abs(out[b, 0]))
        scale = np.abs(g[b]).max()
        assert np.abs(gb.cpu().numpy() - g[b]).max() <= 1e-3 * scale


def test_batch_shared_maps(engine, oracle):
    """sc_frame_stride = 0: every frame reads the same maps (its own assignment, ground truth and call counter) and
    accumulates into its own gradient tensor."""
    f = S.make_frame(230, E=2, true_expert=1)
    has = [S.gating_assignment(f, 64, mode="gating", rng=np.random.default_rng(b)) for b in range(3)]
    gts = [_gt(f, 330 + b, noise=0.1) for b in range(3)]
    out, g = _run_batch(engine, [f] * 3, has, gts, 20.0, call0=5, shared=f["coords"])
    _check_all(engine, oracle, [f] * 3, has, gts, 20.0, 5, out, g, shared=f["coords"])


def _overflow_inputs():
    """4 frames whose selections straddle a fresh context's 64 slots per frame (the oracle counts 79, 62, 53, 59 at alpha 16):
    frame 0 overflows the workspace, the other three fit it."""
    frames = [S.make_frame(10 + b) for b in range(4)]
    has = [S.gating_assignment(f, 128) for f in frames]
    gts = [np.array(f["gt_pose"], np.float32) for f in frames]
    g0 = (np.random.default_rng(9).normal(size=(4,) + frames[0]["coords"].shape) * 1e-3).astype(np.float32)
    return frames, has, gts, g0


def test_batch_overflow_accumulates_once(oracle):
    """ONE frame overflows a fresh context's 64 slots per frame, the others fit: the batch-wide word stops the accumulation of
    EVERY frame in the aborted pass (a frame that fits would otherwise be added in both passes), the workspace grows to the
    largest frame's count, and every gradient tensor ends at initial + the oracle's gradient -- nothing added twice."""
    eng = api.Engine(0)  # fresh: 64 slots per frame
    frames, has, gts, g0 = _overflow_inputs()
    out, g = _run_batch(eng, frames, has, gts, 16.0, call0=100, g0=g0)
    counts = out[:, 1].astype(int)
    assert counts.min() <= 64 < counts.max(), counts
    _check_all(eng, oracle, frames, has, gts, 16.0, 100, out, g, g0=g0)


def test_batch_overflow_in_a_chunk_that_shrinks(monkeypatch):
    """A budget of 32 MiB holds two 60x80 frames at 64 slots each but one at the 96 that frame 0's overflow asks for: the first
    chunk (frames 0, 1) aborts, reruns frame 0 alone, and frame 1 is sampled again with the next chunk.  The result is the bits
    of the same batch on a context without that budget (which overflows and reruns all four frames at once)."""
    monkeypatch.setenv("ESAC_BWD_BATCH_BUDGET_MB", "32")
    small = api.Engine(0)
    monkeypatch.delenv("ESAC_BWD_BATCH_BUDGET_MB")
    whole = api.Engine(0)
    frames, has, gts, g0 = _overflow_inputs()
    out_w, g_w = _run_batch(whole, frames, has, gts, 16.0, call0=100, g0=g0)
    out_s, g_s = _run_batch(small, frames, has, gts, 16.0, call0=100, g0=g0)
    counts = out_w[:, 1].astype(int)
    assert counts[0] > 64 and counts[1] <= 64, counts
    np.testing.assert_array_equal(out_s, out_w)
    np.testing.assert_array_equal(g_s, g_w)
    assert not np.array_equal(g_w, g0)


def test_batch_frames_that_select_nothing(engine, oracle):
    """N = 2048 and a flat distribution in every frame: nothing is refined or accumulated, the losses are the oracle's."""
    frames = [S.make_frame(240 + b, H=24, W=32, sub=20) for b in range(3)]
    has = [S.gating_assignment(f, 2048) for f in frames]
    gts = [_gt(f, 340 + b) for b, f in enumerate(frames)]
    g0 = np.random.default_rng(4).normal(size=(3,) + frames[0]["coords"].shape).astype(np.float32)
    out, g = _run_batch(engine, frames, has, gts, 1e-4, call0=1, g0=g0)
    np.testing.assert_array_equal(g, g0)
    assert (out[:, 1] == 0).all()
    for b, f in enumerate(frames):
        ref, _ = _oracle(oracle, f["coords"], f, has[b], gts[b], 1e-4, 1 + b)
        assert (ref["probs"] < 1e-3).all()
        assert abs(out[b, 0] - ref["loss"]) <= LOSS_RTOL * abs(ref["loss"])


def test_batch_chunking_is_invisible(monkeypatch):
    """A slot-workspace budget of 16 MiB holds one 60x80 frame of 64 slots: the batch of 4 runs in 4 chunks (each its own launch
    set) and returns the unchunked batch's bits."""
    monkeypatch.setenv("ESAC_BWD_BATCH_BUDGET_MB", "16")
    small = api.Engine(0)
    monkeypatch.delenv("ESAC_BWD_BATCH_BUDGET_MB")
    whole = api.Engine(0)
    frames = [S.make_frame(250 + b) for b in range(4)]
    has = [S.gating_assignment(f, 96) for f in frames]
    gts = [_gt(f, 350 + b) for b, f in enumerate(frames)]
    out_w, g_w = _run_batch(whole, frames, has, gts, 30.0, call0=11)
    out_s, g_s = _run_batch(small, frames, has, gts, 30.0, call0=11)
    np.testing.assert_array_equal(out_s, out_w)
    np.testing.assert_array_equal(g_s, g_w)
    assert out_w[:, 1].min() >= 1
    # the chunked context's buffers hold the last chunk only: a read of all 4 frames says so
    with pytest.raises(RuntimeError):
        small.read_frames(api.BUF_BWD_PROBS, 4)
    np.testing.assert_array_equal(whole.read_frames(api.BUF_BWD_PROBS, 4)[3], small.read_frames(api.BUF_BWD_PROBS, 1)[0])


@pytest.mark.parametrize("shape", ["odd_grid", "beyond_lds"])
def test_batch_other_shapes(engine, oracle, shape):
    """An odd grid with shifts and sub-sampling; a grid above the LDS correspondence list (P > 8192, global lists per slot)."""
    if shape == "odd_grid":
        frames = [S.make_frame(260 + b, H=45, W=67, sub=7, shift=(3, 5)) for b in range(3)]
        N, alpha = 64, 20.0
    else:
        frames = [S.make_frame(270 + b, H=100, W=120, sub=4) for b in range(2)]
        N, alpha = 24, 3.0
    has = [S.gating_assignment(f, N) for f in frames]
    gts = [_gt(f, 360 + b) for b, f in enumerate(frames)]
    out, g = _run_batch(engine, frames, has, gts, alpha, call0=3)
    slots = _check_all(engine, oracle, frames, has, gts, alpha, 3, out, g)
    assert max(slots) >= 1


def test_batch_rejects_bad_arguments_before_launching(engine):
    """Every argument error is reported before a launch: the gradient tensor stays bit-unchanged.  An out-of-range DEVICE
    assignment in frame 2 flags that frame's record only (the call raises after every frame has run)."""
    f = S.make_frame(280, E=3, true_expert=0)
    B, N = 4, 64
    sc = torch.from_numpy(np.stack([f["coords"]] * B)).cuda()
    ha = torch.zeros((B, N), dtype=torch.int64, device="cuda")
    g = torch.from_numpy(np.random.default_rng(1).normal(size=(B,) + f["coords"].shape).astype(np.float32)).cuda()
    g_keep = g.clone()
    gts = np.stack([np.array(f["gt_pose"], np.float32)] * B)
    host = np.zeros((B, 4), np.float64)
    lib = engine.lib
    slab = 3 * 3 * 60 * 80

    def call(B_=B, sc_=None, grad=None, ha_=None, gt=None, stride=slab, p=None, h=host.ctypes.data):
        p = p if p is not None else engine.make_params(3, 60, 80, N)
        return lib.esac_hip_backward_batch(engine.ctx, B_, sc.data_ptr() if sc_ is None else sc_, slab,
                                           g.data_ptr() if grad is None else grad, stride, ha.data_ptr() if ha_ is None else ha_,
                                           (gts if gt is None else gt).ctypes.data, 1.0, 100.0, 100.0, C.byref(p),
                                           engine._stream(), h)

    bad_gt = gts.copy()
    bad_gt[2] = 0
    p_shard = engine.make_params(3, 60, 80, N, hyp_offset=16)
    p_wide = engine.make_params(70000, 60, 80, N)
    cases = [dict(B_=0), dict(B_=1025), dict(sc_=0), dict(grad=0), dict(ha_=0), dict(h=None), dict(p=p_shard),
             dict(stride=slab - 1), dict(gt=bad_gt), dict(p=p_wide)]
    for kw in cases:
        rc = call(**kw)
        assert rc != 0, kw
        torch.cuda.synchronize()
        assert torch.equal(g, g_keep), kw
    assert call(gt=bad_gt) == -4 and b"frame 2" in lib.esac_hip_last_error()
    # out-of-range assignment in frame 2 (device tensor): that frame's record says so, the call raises
    ha[2, 17] = 3
    with pytest.raises(RuntimeError, match="hypAssignment") as ei:
        engine.backward_batch(sc, torch.zeros_like(g), ha, gts, 1.0, 100.0, 100.0, engine.make_params(3, 60, 80, N))
    np.testing.assert_array_equal(ei.value.records[:, 3], [0.0, 0.0, 1.0, 0.0])
    # and the same batch without it is clean
    ha[2, 17] = 0
    out = engine.backward_batch(sc, torch.zeros_like(g), ha, gts, 1.0, 100.0, 100.0, engine.make_params(3, 60, 80, N))
    assert (out[:, 3] == 0).all()


def test_batch_drop_in_surface(engine, oracle):
    """esac.backward_batch with CPU tensors against the oracle; the call counter advances by B (a following esac.backward draws
    the hypotheses of call0 + B); a following esac.forward_batch on the same context computes what it computed before."""
    import esac
    frames = [S.make_frame(290 + b) for b in range(3)]
    has = [S.gating_assignment(f, 64) for f in frames]
    gts = [_gt(f, 390 + b) for b, f in enumerate(frames)]
    f0 = frames[0]
    args = (0, 0, f0["focal"], f0["ppx"], f0["ppy"], 10.0, 100.0, 0.5, 100.0, f0["sub"])
    seed, call0 = 1305, 500
    # forward_batch before
    esac.set_seed(seed, 900)
    poses_a = torch.zeros(3, 4, 4)
    exp_a = esac.forward_batch(torch.from_numpy(np.stack([f["coords"] for f in frames])), torch.from_numpy(np.stack(has)),
                               poses_a, *args)
    esac.set_seed(seed, call0)
    sc = torch.from_numpy(np.stack([f["coords"] for f in frames]))
    grads = torch.zeros_like(sc)
    losses = esac.backward_batch(sc, grads, torch.from_numpy(np.stack(has)), torch.from_numpy(np.stack(gts)), 1.0, 100.0, 100.0,
                                 *args)
    assert not grads.is_cuda and len(losses) == 3
    assert esac.get_rng_state() == (seed, call0 + 3)
    for b, f in enumerate(frames):
        ref, g_ref = _oracle(oracle, f["coords"], f, has[b], gts[b], 100.0, call0 + b)
        assert abs(losses[b] - ref["loss"]) <= LOSS_RTOL * max(1.0, abs(ref["loss"]))
        scale = max(float(np.abs(g_ref).max()), 1e-30)
        assert float(np.abs(grads[b].numpy() - g_ref).max()) / scale <= GRAD_RTOL_SAMPLED
    # the next single call draws call0 + 3
    g1 = torch.zeros_like(sc[0])
    loss = esac.backward(sc[0], g1, torch.from_numpy(has[0]), torch.from_numpy(gts[0]), 1.0, 100.0, 100.0, *args)
    ref, _ = _oracle(oracle, f0["coords"], f0, has[0], gts[0], 100.0, call0 + 3)
    np.testing.assert_allclose(engine.read(api.BUF_HYPS), ref["init_hyps"], rtol=0, atol=1e-6)
    assert abs(loss - ref["loss"]) <= LOSS_RTOL * max(1.0, abs(ref["loss"]))
    # forward_batch after: the same as before
    esac.set_seed(seed, 900)
    poses_b = torch.zeros(3, 4, 4)
    exp_b = esac.forward_batch(torch.from_numpy(np.stack([f["coords"] for f in frames])), torch.from_numpy(np.stack(has)),
                               poses_b, *args)
    assert exp_a == exp_b
    torch.testing.assert_close(poses_b, poses_a, rtol=0, atol=0)
