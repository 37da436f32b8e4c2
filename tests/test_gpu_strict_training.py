"""GPU checks of the training path's strict mode (ESAC_FLAG_STRICT_TRAINING, include/esac_hip.h): esac_hip_backward* with the flag
against the CPU oracle on the same input and Philox key.  With the Horn / Jacobi alignment in the sampler AND in the 18 perturbed
solves of dPNP the four sampled cells of every selected hypothesis are held to GRAD_RTOL = 2e-6, the bar of every other cell
(tests/test_gpu_backward.py holds them to 1e-3 on the default route: central differences multiply the two solvers' disagreement
by 500).  No frame may use the "probability within 1e-12 of the threshold" escape of _check: the frames are chosen so that the
oracle alone shows no such edge, and every helper asserts that.

Measured on an MI355X (LAB_NOTES.md "Strict training", profiles/r10_strict_training.txt): sampled cells of the nine parity frames
0 .. 1.6e-7 of the largest entry, every other cell <= 2.5e-7; the bar was not touched."""
import ctypes as C

import numpy as np
import pytest
import torch

from esac_amd import api
from esac_amd import synthetic as S
from tests.test_gpu_backward import GRAD_RTOL, LOSS_RTOL, _check, _gt, _run_both
from tests.test_gpu_semantics import _adversarial_frame
from tests.test_gpu_strict_reference import _sweep_frame

pytestmark = pytest.mark.gpu

# name: (make_frame kwargs, N, assignment mode, alpha, call, (gt rng seed, gt noise), loss cut, slots expected at least)
# (the frames of tests/test_gpu_backward.py; tests/test_strict_training_host.py::PARITY_FRAMES runs their minimal sets on the host)
FRAMES = {
    "sharp0": (dict(k=0), 256, "single", 100.0, 0, (0, 0.02), 100.0, 1),
    "sharp1": (dict(k=1), 64, "single", 100.0, 1, (1, 0.02), 100.0, 1),
    "sharp2": (dict(k=2), 256, "single", 100.0, 2, (2, 0.02), 100.0, 1),
    "sharp3": (dict(k=3), 64, "single", 100.0, 3, (3, 0.02), 100.0, 1),
    "flat": (dict(k=10), 128, "single", 2.0, 0, (0, 0.05), 100.0, 20),
    "clamped": (dict(k=21), 64, "single", 5.0, 5, (3, 0.3), 2.0, 2),
    "gating": (dict(k=31, E=3, true_expert=1), 96, "gating", 10.0, 2, (4, 0.02), 100.0, 1),
    "odd_grid_shift": (dict(k=41, H=45, W=61, sub=10, shift=(7, -5)), 64, "single", 20.0, 1, (5, 0.02), 100.0, 1),
    "beyond_lds": (dict(k=105, H=100, W=120, sub=4), 24, "single", 3.0, 4, (5, 0.05), 100.0, 4),
}


@pytest.fixture(scope="module")
def solo():
    """A context that refines its slots with one workgroup each (what a batch does): bit-for-bit comparisons run on it."""
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    mp = pytest.MonkeyPatch()
    mp.setenv("ESAC_SLOT_TEAMS", "0")
    try:
        return api.Engine(0)
    finally:
        mp.undo()


def _cam(f):
    return dict(shift_x=f["shift"][0], shift_y=f["shift"][1], focal=f["focal"], ppx=f["ppx"], ppy=f["ppy"], sub_sampling=f["sub"])


def _grad_errs(g_dev, g_ref, ref):
    """(worst error off the sampled cells, worst error on them), relative to the largest entry of the oracle's gradient."""
    scale = max(float(np.abs(g_ref).max()), 1e-30)
    sampled = np.zeros(g_ref.shape[2:], bool)
    for h in np.nonzero(ref["probs"] >= 1e-3)[0]:
        for x, y in ref["sample_xy"][h]:
            sampled[y, x] = True
    diff = np.abs(g_dev - g_ref)
    return float(diff[:, :, ~sampled].max()) / scale, (float(diff[:, :, sampled].max()) / scale if sampled.any() else 0.0)


def _check_strict(engine, oracle, f, ha, out, g, ref, g_ref, expect_slots=None, **okw):
    assert not (np.abs(ref["probs"] - 1e-3) < 1e-12).any()  # no frame may take _check's escape
    n_sel, err = _check(engine, out, g, ref, g_ref, expect_slots=expect_slots)  # every bar of the default route's check
    fwd = oracle.forward(f["coords"], ha, **_cam(f), **okw)
    np.testing.assert_array_equal(engine.read(api.BUF_TRIES), fwd["tries"])
    err, err_s = _grad_errs(g, g_ref, ref)
    print("strict training parity: slots=%d grad_err=%.2e sampled cells %.2e (bar %.0e for both)" % (n_sel, err, err_s, GRAD_RTOL))
    assert err_s <= GRAD_RTOL, err_s
    return n_sel, err_s


def _make(name):
    kw, N, mode, alpha, call, (gseed, noise), cut, slots = FRAMES[name]
    kw = dict(kw)
    f = S.make_frame(kw.pop("k"), **kw)
    ha = S.gating_assignment(f, N, mode=mode)
    return f, ha, _gt(f, np.random.default_rng(gseed), noise=noise), alpha, call, cut, slots


@pytest.mark.parametrize("name", list(FRAMES))
def test_strict_parity_on_the_backward_frames(engine, oracle, name):
    f, ha, gt, alpha, call, cut, slots = _make(name)
    out, g, ref, g_ref = _run_both(engine, oracle, f, ha, gt, call=call, alpha=alpha, cut=cut, strict_training=True)
    _check_strict(engine, oracle, f, ha, out, g, ref, g_ref, expect_slots=slots, inlier_alpha=alpha, seed=1305, call=call)
    assert np.abs(g_ref).max() > 0


def _oracle_slots(oracle, f, ha, fwd, **okw):
    """Per selected hypothesis of the oracle's distribution: (h, refined pose, accepted steps, inliers of the last accepted step,
    LM iterations) -- the oracle's refinement of that hypothesis alone (in_hyps: its own initial pose)."""
    assert not (np.abs(fwd["probs"] - 1e-3) < 1e-12).any()
    rows = []
    for h in np.nonzero(fwd["probs"] >= 1e-3)[0]:
        one = oracle.forward(f["coords"], ha[h:h + 1], in_hyps=fwd["hyps"][h:h + 1], **_cam(f), **okw)
        rows.append((int(h), one["refined"].copy(), int(one["ref_steps"]), int(one["inlier_map"].sum()),
                     int(np.asarray(one["lm_iters"]).reshape(-1)[0])))
    return rows


def _check_slots(engine, rows):
    n_sel = len(rows)
    np.testing.assert_array_equal(engine.read(api.BUF_BWD_SLOTS)[:n_sel], [r[0] for r in rows])
    info = engine.read(api.BUF_BWD_SLOT_INFO)[:n_sel]
    refh = engine.read(api.BUF_BWD_REF_HYPS)
    for s, (h, pose, steps, inl, lm) in enumerate(rows):
        assert info[s, 2] == steps and info[s, 3] == lm, (s, h, info[s], steps, lm)
        assert (info[s, 0] >= 0) == (steps > 0), (s, h, info[s])
        if steps > 0:
            assert info[s, 1] == inl, (s, h, info[s], inl)
        np.testing.assert_allclose(refh[h], pose, rtol=0, atol=1e-6, err_msg=str((s, h)))
    return info


@pytest.mark.parametrize("kind", ["planar", "degenerate", "sliver"])
def test_strict_training_closes_the_divergence_classes(engine, oracle, kind):
    """The planar and degenerate adversarial maps (N = 12288, 5000 tries) and the pinned sliver frame (12 experts, 2048 hypotheses)
    through backward_device with the flag: cells, tries, slot list and refined poses are the oracle's.  Printed, not asserted: on
    how many hypotheses the default route accepts another try."""
    if kind == "sliver":
        k = 874
        f = S.make_frame(5000 + k, E=12, true_expert=k % 12, outlier_frac=0.3)
        N, okw = 2048, dict(seed=1305, call=k)
        ha = S.gating_assignment(f, N, mode="gating")
    else:
        f = _adversarial_frame(kind)
        N, okw = 12288, dict(seed=77, call=3, max_tries=5000)
        ha = np.arange(N, dtype=np.int64) % 3
    E = f["coords"].shape[0]
    fwd = oracle.forward(f["coords"], ha, **_cam(f), **okw)
    rows = _oracle_slots(oracle, f, ha, fwd, **okw)
    sc, hat = torch.from_numpy(f["coords"]).cuda(), torch.from_numpy(ha).cuda()
    gt = np.array(f["gt_pose"], np.float32)
    out = engine.backward_device(sc, torch.zeros_like(sc), hat, gt, 1.0, 100.0, 100.0,
                                 engine.make_params(E, 60, 80, N, strict_training=True, **_cam(f), **okw))
    np.testing.assert_array_equal(engine.read(api.BUF_SAMPLE_XY), fwd["sample_xy"])
    np.testing.assert_array_equal(engine.read(api.BUF_TRIES), fwd["tries"])
    assert int(out[1]) == len(rows) >= 1
    _check_slots(engine, rows)
    engine.backward_device(sc, torch.zeros_like(sc), hat, gt, 1.0, 100.0, 100.0, engine.make_params(E, 60, 80, N, **_cam(f), **okw))
    print("divergence class %s: the default route accepts another try than the oracle on %d hypotheses, the strict route on 0"
          % (kind, int((engine.read(api.BUF_TRIES) != fwd["tries"]).sum())))


def test_strict_slot_refinement_over_the_frame_kinds(engine, solo, oracle):
    """64 frames of the four sweep kinds: accepted steps, inliers of the last accepted step and LM iterations of EVERY slot are the
    oracle's, by teams (the call selects <= 32) and with one workgroup per slot, and the two routes agree in every discrete output."""
    slots = team_calls = 0
    for k in range(64):
        f, N, mode = _sweep_frame(k)
        ha = S.gating_assignment(f, N, mode=mode)
        E, _, H, W = f["coords"].shape
        okw = dict(seed=77, call=k, inlier_alpha=30.0)
        fwd = oracle.forward(f["coords"], ha, **_cam(f), **okw)
        rows = _oracle_slots(oracle, f, ha, fwd, **okw)
        sc, hat = torch.from_numpy(f["coords"]).cuda(), torch.from_numpy(ha).cuda()
        gt = np.array(f["gt_pose"], np.float32)
        infos = []
        for eng in (engine, solo):
            out = eng.backward_device(sc, torch.zeros_like(sc), hat, gt, 1.0, 100.0, 100.0,
                                      eng.make_params(E, H, W, N, strict_training=True, **_cam(f), **okw))
            assert int(out[1]) == len(rows), (k, out[1], len(rows))
            infos.append(_check_slots(eng, rows))
        team_calls += bool(engine.bwd_team_info()["teams"])
        assert not solo.bwd_team_info()["teams"]
        np.testing.assert_array_equal(infos[0][:, 1:], infos[1][:, 1:], err_msg=str(k))
        np.testing.assert_array_equal(infos[0][:, 0] >= 0, infos[1][:, 0] >= 0, err_msg=str(k))
        slots += len(rows)
    print("slot refinement: 64 frames, %d slots, %d calls refined by teams" % (slots, team_calls))
    assert slots >= 64


@pytest.mark.parametrize("k,E,N,clean_loss,clean_slots", [(5, 1, 64, 1.1021, 5), (7, 3, 96, 2.7688, 8)])
def test_non_finite_coordinates_give_the_references_answer(engine, oracle, k, E, N, clean_loss, clean_slots):
    """A NaN coordinate in the expert of hypothesis 0.  The oracle: loss NaN, every probability NaN, entropy 0, no hypothesis with
    p >= PROB_THRESH, every entry of that expert's gradient NaN and 0.0 in the others.  The device with the flag: the same masks,
    the same finite entries, no slot; the call returns, the next default call on the context is correct, esac.backward returns
    nan.  The default route on the same map still returns the finite result it returns today."""
    import esac
    f = S.make_frame(k, E=E) if E > 1 else S.make_frame(k)
    ha = S.gating_assignment(f, N)
    gt = np.array(f["gt_pose"], np.float32)
    e = int(ha[0])
    kw = dict(focal=f["focal"], ppx=f["ppx"], ppy=f["ppy"], sub_sampling=f["sub"], seed=1305, call=0)
    g_clean = np.zeros_like(f["coords"])
    clean = oracle.backward(f["coords"], g_clean, ha, gt, **kw)
    assert abs(clean["loss"] - clean_loss) < 1e-3 and int((clean["probs"] >= 1e-3).sum()) == clean_slots
    c = f["coords"].copy()
    c[e, 0, 3, 3] = np.nan
    g_ref = np.zeros_like(c)
    ref = oracle.backward(c, g_ref, ha, gt, **kw)
    assert np.isnan(ref["loss"]) and np.isnan(ref["probs"]).all() and ref["entropy"] == 0.0 and not (ref["probs"] >= 1e-3).any()
    assert np.isnan(g_ref[e]).all() and g_ref[e].size == 14400 and not np.delete(g_ref, e, axis=0).any()
    sc, hat = torch.from_numpy(c).cuda(), torch.from_numpy(ha).cuda()
    g = torch.zeros_like(sc)
    out = engine.backward_device(sc, g, hat, gt, 1.0, 100.0, 100.0, engine.make_params(E, 60, 80, N, strict_training=True, **kw))
    g = g.cpu().numpy()
    assert np.isnan(out[0]) and out[1] == 0 and out[2] == 0.0 and out[3] == 0.0
    np.testing.assert_array_equal(np.isnan(engine.read(api.BUF_BWD_PROBS)), np.isnan(ref["probs"]))
    np.testing.assert_array_equal(np.isnan(g), np.isnan(g_ref))
    np.testing.assert_array_equal(g[~np.isnan(g)], g_ref[~np.isnan(g_ref)])
    # the context's next default call is correct
    f2 = dict(f, coords=f["coords"])
    res = _run_both(engine, oracle, f2, ha, gt, call=0)
    _check(engine, *res, expect_slots=clean_slots)
    # the Python layer returns nan rather than raising
    esac.set_seed(1305, 0)
    esac.set_strict_training(True)
    try:
        grads = torch.zeros_like(sc)
        loss = esac.backward(sc, grads, hat, torch.from_numpy(gt), 1.0, 100.0, 100.0, 0, 0, f["focal"], f["ppx"], f["ppy"], 10.0,
                             100.0, 0.5, 100.0, f["sub"])
    finally:
        esac.set_strict_training(False)
    assert isinstance(loss, float) and np.isnan(loss)
    np.testing.assert_array_equal(np.isnan(grads.cpu().numpy()), np.isnan(g_ref))
    # the default route on the NaN map, as it is today: such a cell is an outlier -- a finite loss, the slots of the outlier map
    g = torch.zeros_like(sc)
    out = engine.backward_device(sc, g, hat, gt, 1.0, 100.0, 100.0, engine.make_params(E, 60, 80, N, **kw))
    c30 = c.copy()
    c30[e, 0, 3, 3] = 1e30  # (the default is what the reference gives with that cell at 1e30)
    ref30 = oracle.backward(c30, np.zeros_like(c), ha, gt, **kw)
    assert abs(out[0] - ref30["loss"]) <= LOSS_RTOL * max(1.0, abs(ref30["loss"])), (out, ref30["loss"])
    assert out[1] == int((ref30["probs"] >= 1e-3).sum()) >= 1, out
    # (its gradient: the NaN point's own d error / d point, and through path II's pose-space sums the four sampled cells of the
    # selected hypotheses of that expert -- nowhere else)
    finite = torch.isfinite(g).cpu().numpy()
    print("default route on the NaN map: %d non-finite gradient entries" % int((~finite).sum()))
    finite[e, :, 3, 3] = True
    xy = engine.read(api.BUF_SAMPLE_XY)
    for h in engine.read(api.BUF_BWD_SLOTS)[:int(out[1])]:
        for x, y in xy[h]:
            finite[int(ha[h]), :, y, x] = True
    assert finite.all() and float(torch.nan_to_num(g).abs().max()) > 0


def _batch_inputs(B, per_frame):
    frames = []
    for b in range(B):
        kw = dict(shift=(b % 5 - 2, 1 - b % 3), focal=500.0 + 12.0 * b) if per_frame else {}
        frames.append(S.make_frame(820 + b, E=2, true_expert=b % 2, **kw))
    has = [S.gating_assignment(f, 96, mode="gating") for f in frames]
    gts = [_gt(f, np.random.default_rng(900 + b), noise=0.05) for b, f in enumerate(frames)]
    return frames, has, gts


@pytest.mark.parametrize("cams", ["shared", "per_frame"])
def test_strict_batch_equals_strict_single_calls_and_the_oracle(solo, oracle, monkeypatch, cams):
    """backward_batch with the flag, B = 8, once on a context whose budget forces chunks: frame b is the strict single call at
    call + b bit for bit (one workgroup per slot on both sides) and meets the strict bars against the oracle; a batch with ONE NaN
    frame leaves every other frame's loss and gradient exactly those of its single call."""
    B, N, alpha, call0 = 8, 96, 30.0, 60
    frames, has, gts = _batch_inputs(B, cams == "per_frame")
    monkeypatch.setenv("ESAC_SLOT_TEAMS", "0")
    monkeypatch.setenv("ESAC_BWD_BATCH_BUDGET_MB", "32")
    chunked = api.Engine(0)
    f0 = frames[0]
    table = api.make_cams([f["shift"][0] for f in frames], [f["shift"][1] for f in frames], [f["focal"] for f in frames],
                          [f["ppx"] for f in frames], [f["ppy"] for f in frames]) if cams == "per_frame" else None

    def params(eng, f, call):
        return eng.make_params(2, 60, 80, N, inlier_alpha=alpha, seed=1305, call=call, strict_training=True, **_cam(f))

    def batch(eng, coords):
        g = torch.zeros((B,) + f0["coords"].shape, dtype=torch.float32, device="cuda")
        out = eng.backward_batch(torch.from_numpy(coords).cuda(), g, torch.from_numpy(np.stack(has)).cuda(), np.stack(gts), 1.0, 100.0,
                                 100.0, params(eng, f0, call0), cams=table)
        return out, g.cpu().numpy()

    coords = np.stack([f["coords"] for f in frames])
    out, g = batch(solo, coords)
    out_c, g_c = batch(chunked, coords)
    np.testing.assert_array_equal(out_c, out)
    np.testing.assert_array_equal(g_c, g)
    singles = []
    for b, f in enumerate(frames):
        sc = torch.from_numpy(f["coords"]).cuda()
        gb = torch.zeros_like(sc)
        o = solo.backward_device(sc, gb, torch.from_numpy(has[b]).cuda(), gts[b], 1.0, 100.0, 100.0, params(solo, f, call0 + b))
        singles.append((o, gb.cpu().numpy()))
        np.testing.assert_array_equal(out[b], o)
        np.testing.assert_array_equal(g[b], singles[b][1])
        g_ref = np.zeros_like(f["coords"])
        ref = oracle.backward(f["coords"], g_ref, has[b], gts[b], inlier_alpha=alpha, seed=1305, call=call0 + b, **_cam(f))
        _check_strict(solo, oracle, f, has[b], o, singles[b][1], ref, g_ref, expect_slots=1, inlier_alpha=alpha, seed=1305, call=call0 + b)
    # one NaN frame
    bad = coords.copy()
    bad[3, int(has[3][0]), 0, 3, 3] = np.nan
    out_n, g_n = batch(solo, bad)
    assert np.isnan(out_n[3, 0]) and out_n[3, 1] == 0 and np.isnan(g_n[3, int(has[3][0])]).all()
    for b in range(B):
        if b != 3:
            np.testing.assert_array_equal(out_n[b], singles[b][0])
            np.testing.assert_array_equal(g_n[b], singles[b][1])


def test_c_abi_surface(engine, solo, oracle):
    """-4 on every forward / phase entry point and together with ESAC_FLAG_STRICT_REFERENCE, the context usable afterwards; an
    asynchronous strict call followed by a stream sync gives the blocking call's gradient."""
    f = S.make_frame(5)
    ha = S.gating_assignment(f, 64)
    sc, hat = torch.from_numpy(f["coords"]).cuda(), torch.from_numpy(ha).cuda()
    gt = np.array(f["gt_pose"], np.float32)
    p = engine.make_params(1, 60, 80, 64, strict_training=True)
    for fn in (engine.forward_device, engine.sample, engine.score, engine.select, engine.refine, engine.score_exact):
        with pytest.raises(RuntimeError, match=r"ESAC_FLAG_STRICT_TRAINING.*\[status -4\]"):
            fn(sc, hat, p)
    with pytest.raises(RuntimeError, match=r"ESAC_FLAG_STRICT_TRAINING.*\[status -4\]"):
        engine.forward_batch(sc[None], hat[None], p)
    both = engine.make_params(1, 60, 80, 64, strict_training=True)
    both.flags |= api.FLAG_STRICT_REFERENCE
    g = torch.zeros_like(sc)
    with pytest.raises(RuntimeError, match=r"\[status -4\]"):
        engine.backward_device(sc, g, hat, gt, 1.0, 100.0, 100.0, both)
    with pytest.raises(RuntimeError, match=r"\[status -4\]"):
        engine.backward_batch(sc[None], g[None], hat[None], gt[None], 1.0, 100.0, 100.0, both)
    assert not g.any()
    res = _run_both(engine, oracle, f, ha, gt, call=0)  # the context is fine afterwards
    _check(engine, *res, expect_slots=1)
    ps = solo.make_params(1, 60, 80, 64, strict_training=True, call=9)
    g_block, g_async = torch.zeros_like(sc), torch.zeros_like(sc)
    solo.backward_device(sc, g_block, hat, gt, 1.0, 100.0, 100.0, ps)
    assert solo.backward_device(sc, g_async, hat, gt, 1.0, 100.0, 100.0, ps, want_host=False) is None
    torch.cuda.synchronize()
    assert torch.equal(g_async, g_block) and float(g_block.abs().max()) > 0


@pytest.mark.parametrize("E,N,mode", [(1, 256, "single"), (3, 96, "gating")])
def test_defaults_are_untouched(engine, E, N, mode):
    """Every output of a default backward_device and a default forward_device before a strict training call on the same context,
    and again after it: array_equal."""
    f = S.make_frame(77 + E, E=E, true_expert=E - 1)
    ha = S.gating_assignment(f, N, mode=mode)
    sc, hat = torch.from_numpy(f["coords"]).cuda(), torch.from_numpy(ha).cuda()
    gt = _gt(f, np.random.default_rng(1), noise=0.05)
    kw = dict(seed=3, call=9, inlier_alpha=20.0, **_cam(f))

    def snapshot():
        g = torch.zeros_like(sc)
        out = engine.backward_device(sc, g, hat, gt, 1.0, 100.0, 100.0, engine.make_params(E, 60, 80, N, **kw))
        n = int(out[1])
        got = [out.copy(), g.cpu().numpy()] + [engine.read(b).copy() for b in (
            api.BUF_HYPS, api.BUF_SAMPLE_XY, api.BUF_TRIES, api.BUF_SCORES, api.BUF_BWD_PROBS, api.BUF_BWD_LOSSES,
            api.BUF_BWD_REF_HYPS, api.BUF_BWD_SCORE_GRADS)]
        got += [engine.read(api.BUF_BWD_SLOTS)[:n].copy(), engine.read(api.BUF_BWD_SLOT_INFO)[:n, 1:].copy(), engine.read(api.BUF_BWD_DLOSS)[:n].copy()]
        res = engine.forward_device(sc, hat, engine.make_params(E, 60, 80, N, exact_scores="auto", **kw))
        got += [res[:31].copy()] + [engine.read(b).copy() for b in (api.BUF_HYPS, api.BUF_SAMPLE_XY, api.BUF_TRIES, api.BUF_SCORES,
                                                                     api.BUF_INLIER_MAP, api.BUF_INLIER_COUNTS)]
        return got

    before = snapshot()
    out = engine.backward_device(sc, torch.zeros_like(sc), hat, gt, 1.0, 100.0, 100.0, engine.make_params(E, 60, 80, N, strict_training=True, **kw))
    assert out[1] >= 1
    for a, b in zip(before, snapshot()):
        np.testing.assert_array_equal(a, b)
