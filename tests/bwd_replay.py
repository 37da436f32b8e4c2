"""Replay of the training path's gradient stages (helper module of test_bwd_replay_host.py and
test_gpu_backward_stages.py; also what scripts/dev/bwd_diag.py prints from).

The oracle's esac_backward is split at its stage boundary (oracle/esac_oracle_bwd.inc: backward_paths): path I, path II
and the assembly are a function of GIVEN upstream stages -- initial and refined poses, sampled cells, probabilities,
losses, inlier maps.  Fed with the DEVICE's own stage buffers it yields what each gradient kernel should have written from
the inputs that kernel really had; what is left between device and expectation is that one kernel's rounding, so every
bar below is derived from the arithmetic instead of inherited from upstream noise.

The frozen case list (CASES) covers the accumulation's unroll of 8 and 64-wide ballot rounds (1, 8, 9, 64, 65, 130
slots), a grid smaller than a slot's workgroup, a ragged width, several experts with one that owns no slot, the
max_reproj branch, the slot-team range, and the rank-deficient / empty-map branches of noisy frames.
"""
import numpy as np

from esac_amd import synthetic as S

PROB_THRESH = 1e-3   # esac_derivative.h:33
SEED = 7
EPS53 = 2.0 ** -53

# ---- bars (see DESIGN.md "Precision contract -> Training path")
# path II, direct term: identical fp64 inputs and formula on both sides; foreign operations are exp (<= 2 ulp), st(1-st)
# (absolute error of a few 2^-53 against a maximum of 1/4) and ~50 operations of the projection derivative on
# intermediates within 2^10 of the result: about 2^-48 of the slab's largest entry, 8 bits of head-room
DIRECT_BAR = 2.0 ** -40
# path I: jacobeanR = -(J^T J)^-1 J^T.  PATH1_REF_SPREAD is measured ON THE REFERENCE ARITHMETIC ALONE
# (test_bwd_replay_host.py::test_path1_bar_constant_measured_on_the_reference): jacobeanR from the same rows summed in
# the oracle's cell order and in reversed order differ by at most this multiple of cond_2(J^T J) * 2^-53 * max|jacobeanR|
# over every path-I slot of CASES (worst measured: 2.84, on the shifted frame; the constant is that figure rounded up).
# The device is allowed 16 x that: another backward-stable inverse (LDL^T against the SVD route) and an 8-wavefront tree.
PATH1_REF_SPREAD = 2.9
PATH1_FACTOR = 16.0
PATH1_SKIP = 1e-6        # a slot whose path-I bar exceeds this share of its slab is only held to its zero / non-zero state
PATH1_SKIP_SHARE = 0.05  # ... and at most this share of all path-I slots of the case list may be
CLAMP_EDGE = 1e-6        # a largest entry this close to the clamp's 10 may legitimately fall either side


def path1_rel_bar(cond):
    return PATH1_FACTOR * PATH1_REF_SPREAD * cond * EPS53


def _small():
    return S.make_frame(7, H=12, W=16, sub=40)


def _ragged():
    return S.make_frame(8, H=13, W=17, sub=37)


def _three():
    return S.make_frame(9, E=3, true_expert=1, H=13, W=17, sub=37)


# name -> (frame factory, N, alpha, call, options).  P = H * W; 3 P is never a multiple of 256.
CASES = {
    "small_n1": (_small, 1, 100.0, 0, {}),
    "small_n8": (_small, 8, 0.01, 1, {}),
    "small_n9_prefilled": (_small, 9, 0.01, 2, dict(prefill=True)),
    "ragged_n64": (_ragged, 64, 0.01, 3, {}),
    "ragged_n65": (_ragged, 65, 0.01, 4, dict(prefill=True)),
    "three_experts_n130": (_three, 130, 0.01, 5, dict(prefill=True, spread=True)),
    "shifted_n40": (lambda: S.make_frame(11, H=23, W=29, sub=20, shift=(7, -5), focal=500.0, ppx=300.0, ppy=230.0), 40, 5.0, 6,
                    dict(max_reproj=30.0)),
    "team_grid_n48": (lambda: S.make_frame(12, H=32, W=40, sub=16), 48, 20.0, 7, {}),
    "outliers_07_n24": (lambda: S.make_frame(13, H=12, W=16, sub=40, outlier_frac=0.7), 24, 0.01, 8, {}),
    "outliers_10_n24": (lambda: S.make_frame(14, H=13, W=17, sub=37, outlier_frac=1.0), 24, 0.01, 9, dict(max_tries=3)),
}
ALL_SELECTED = ("small_n1", "small_n8", "small_n9_prefilled", "ragged_n64", "ragged_n65", "three_experts_n130")  # slots == N


def make_case(name, prefill=None):
    """Inputs of one case: frame, assignment, float32 ground truth, the tensor the call accumulates into, keyword sets."""
    factory, N, alpha, call, opt = CASES[name]
    f = factory()
    rng = np.random.default_rng(100 + call)
    if opt.get("spread"):
        # spread over all three experts (Dirichlet), then forced: expert 2 owns none, the garbage map of expert 0 keeps every
        # eighth hypothesis (its slots are mostly rank deficient: more of them would push the share of slots that path I
        # cannot be compared on beyond PATH1_SKIP_SHARE), the true expert 1 the rest -- ownership interleaved in slot order.
        # (mode="gating" puts all 130 on the true expert)
        ha = S.gating_assignment(f, N, mode="dirichlet", rng=rng)
        ha = np.where((ha != 1) & (np.arange(N) % 8 == 3), 0, 1).astype(np.int64)
    else:
        ha = S.gating_assignment(f, N)
    gt = np.array(f["gt_pose"], np.float64)
    gt[:3, 3] += rng.normal(size=3) * 0.05
    gt = gt.astype(np.float32)
    if prefill is None:
        prefill = bool(opt.get("prefill"))
    g0 = rng.normal(size=f["coords"].shape).astype(np.float32) if prefill else np.zeros_like(f["coords"])
    return case_of(f, ha, gt, g0, alpha, SEED, call, max_tries=opt.get("max_tries", 0), max_reproj=opt.get("max_reproj", 100.0), name=name)


def case_of(f, ha, gt, g0, alpha, seed, call, max_tries=0, max_reproj=100.0, name="frame"):
    """The case record of any synthetic frame (what replay(), device_stages() and run_device() take)."""
    E, _, H, W = f["coords"].shape
    cam = dict(shift_x=f["shift"][0], shift_y=f["shift"][1], focal=f["focal"], ppx=f["ppx"], ppy=f["ppy"], sub_sampling=f["sub"],
               inlier_alpha=alpha, max_reproj=max_reproj)
    key = dict(seed=seed, call=call, max_tries=max_tries)
    return dict(name=name, coords=f["coords"], ha=ha, gt=gt, g0=g0, cam=cam, key=key, E=E, H=H, W=W, N=len(ha), P=H * W)


def run_oracle(O, c):
    """The whole oracle on a case: stages, both paths, the tensor (c['g0'] +=)."""
    g = c["g0"].copy()
    ref = O.backward(c["coords"], g, c["ha"], c["gt"], want_paths=True, want_stages=True, **c["cam"], **c["key"])
    ref["grad"] = g
    return ref


STAGE_KEYS = ("init_hyps", "ref_hyps", "sample_xy", "probs", "losses", "have_map", "maps")


def replay(O, c, stages):
    """Path I, path II and the assembly on the given stages, by the oracle's own text.  Returns, per hypothesis h:
    grad_path1 / grad_path2 [N,P,3], grad_direct (path II without the support terms), support and support_raw [N,4,3], jtj [N,6,6] with
    cond [N], jr_max (max|jacobeanR| before the clamp), path1_state, dpnp [N,6,12], dpnp_state, dpnp_max; score_grads with
    its summation bound score_grads_bar; and grad, the tensor c['g0'] accumulated."""
    g = c["g0"].copy()
    out = O.backward_paths(c["coords"], g, c["ha"], c["gt"], stages, **c["cam"])
    out["grad"] = g
    cond = np.zeros(c["N"])
    for h in np.nonzero((out["path1_state"] == 0) | (out["path1_state"] == 3))[0]:
        w = np.linalg.eigvalsh(out["jtj"][h])
        cond[h] = np.inf if w[0] <= 0 else w[-1] / w[0]
    out["cond"] = cond
    p, L = np.asarray(stages["probs"], np.float64), np.asarray(stages["losses"], np.float64)
    # p_i L_i - sum_j p_i p_j L_j: N + 1 terms, each product rounded once -- the bound of recursive summation
    out["score_grads_bar"] = (c["N"] + 4) * EPS53 * p * (np.abs(L) + float(np.sum(p * np.abs(L))))
    out["selected"] = np.nonzero(~(p < PROB_THRESH))[0]
    return out


def accumulate(g0, ha, slots, probs, slab1, slab2):
    """k_bwd_accumulate / esac.cpp:491-508 in numpy: v = float32(float64(v) + (p g1 + g2)), slot by slot in ascending
    hypothesis order, per expert.  slab1 / slab2: [len(slots),3,P] float64, slots: hypothesis index per slab."""
    g = g0.copy()
    E, _, H, W = g.shape
    for s, h in enumerate(slots):
        e = int(ha[h])
        t = probs[h] * slab1[s] + slab2[s]
        g[e] = (g[e].astype(np.float64) + t.reshape(3, H, W)).astype(np.float32)
    return g


def planar(slab):
    """[n,P,3] (the oracle's layout) -> [n,3,P] (the device's and the tensor's)."""
    return np.ascontiguousarray(np.transpose(slab, (0, 2, 1)))


def frame_scale(c, rp):
    """Largest entry of the reference gradient of the frame (what GRAD_RTOL / GRAD_RTOL_SAMPLED are relative to), from the
    replay's slabs: sum over the selected hypotheses of p g1 + g2, per expert, in float64."""
    tot = np.zeros((c["E"], c["P"], 3))
    for h in rp["selected"]:
        tot[int(c["ha"][h])] += rp["probs_in"][h] * rp["grad_path1"][h] + rp["grad_path2"][h]
    return max(float(np.abs(tot).max()), 1e-300)


def support_per_cell(c, rp, h, key="support"):
    """The support terms of hypothesis h summed per distinct sampled cell: {cell index y*W+x: [3]}.  key="support_raw": what they
    would be had the > 10 clamp not dropped the dPNP matrix (the other side of a drop decision)."""
    out = {}
    for j, (x, y) in enumerate(rp["sample_xy_in"][h]):
        out.setdefault(int(y) * c["W"] + int(x), np.zeros(3))
        out[int(y) * c["W"] + int(x)] += rp[key][h, j]
    return out


def oracle_stages(ref):
    return {k: ref[k] for k in STAGE_KEYS}


def replay_with_inputs(O, c, stages):
    rp = replay(O, c, stages)
    rp["probs_in"] = np.asarray(stages["probs"], np.float64)
    rp["sample_xy_in"] = np.asarray(stages["sample_xy"])
    return rp


# ---------------------------------------------------------------- the device side
def device_stages(engine, api, c, n_sel):
    """Every stage buffer of the most recent blocking backward call, re-indexed by hypothesis where the replay wants it.
    Returns (stages for replay(), dev) with dev: slots, info [n,4], slab1 / slab2 [n,3,P], maps [n,2,P], scores."""
    n = int(n_sel)
    N, P = c["N"], c["P"]
    dev = dict(slots=engine.read(api.BUF_BWD_SLOTS)[:n].copy(), info=engine.read(api.BUF_BWD_SLOT_INFO)[:n].copy(),
               scores=engine.read(api.BUF_SCORES), sgrad=engine.read(api.BUF_BWD_SCORE_GRADS),
               dloss=engine.read(api.BUF_BWD_DLOSS)[:n].copy(), team=engine.read(api.BUF_BWD_TEAM_INFO))
    if n:
        dev["slab1"] = engine.read_slabs(api.BUF_BWD_PATH1, n).reshape(n, 3, P)
        dev["slab2"] = engine.read_slabs(api.BUF_BWD_PATH2, n).reshape(n, 3, P)
        dev["maps"] = engine.read_maps(n)
    else:
        dev["slab1"] = dev["slab2"] = np.zeros((0, 3, P))
        dev["maps"] = np.zeros((0, 2, P), np.uint8)
    have = np.zeros(N, np.uint8)
    maps = np.zeros((N, P), np.uint8)
    dloss = np.zeros((N, 6))
    for s, h in enumerate(dev["slots"]):
        buf = int(dev["info"][s, 0])
        have[h] = buf >= 0
        if buf >= 0:
            maps[h] = dev["maps"][s, buf]
        dloss[h] = dev["dloss"][s]
    stages = dict(init_hyps=engine.read(api.BUF_HYPS), ref_hyps=engine.read(api.BUF_BWD_REF_HYPS),
                  sample_xy=engine.read(api.BUF_SAMPLE_XY), probs=engine.read(api.BUF_BWD_PROBS),
                  losses=engine.read(api.BUF_BWD_LOSSES), have_map=have, maps=maps, score_grads=dev["sgrad"], dloss=dloss)
    return stages, dev


def run_device(engine, api, c, strict=False):
    """One blocking esac_hip_backward on a case; returns (out record, float tensor, stages, dev)."""
    import torch
    sc = torch.from_numpy(c["coords"]).cuda()
    hat = torch.from_numpy(c["ha"]).cuda()
    cam = c["cam"]
    p = engine.make_params(c["E"], c["H"], c["W"], c["N"], shift_x=cam["shift_x"], shift_y=cam["shift_y"], focal=cam["focal"],
                           ppx=cam["ppx"], ppy=cam["ppy"], sub_sampling=cam["sub_sampling"], inlier_alpha=cam["inlier_alpha"],
                           max_reproj=cam["max_reproj"], seed=c["key"]["seed"], call=c["key"]["call"],
                           max_tries=c["key"]["max_tries"], strict_training=strict)
    g = torch.from_numpy(c["g0"].copy()).cuda()
    out = engine.backward_device(sc, g, hat, c["gt"], 1.0, 100.0, 100.0, p)
    stages, dev = device_stages(engine, api, c, out[1])
    return out, g.cpu().numpy(), stages, dev


def slab_ratios(c, stages, dev, rp):
    """Worst device / bar ratio of the two slab checks over the slots of a call: path II's direct term on the non-sampled
    cells (DIRECT_BAR of the slab's largest direct entry) and path I on every slot whose bar is within PATH1_SKIP
    (path1_rel_bar(cond) of the slab's largest entry).  Returns (direct, path1, slots compared on path I)."""
    w_direct = w_p1 = 0.0
    n_p1 = 0
    for s, h in enumerate(dev["slots"]):
        free = np.ones(c["P"], bool)
        for x, y in stages["sample_xy"][h]:
            free[int(y) * c["W"] + int(x)] = False
        want = rp["grad_direct"][h].T
        d = float(np.abs(dev["slab2"][s] - want)[:, free].max())
        bar = DIRECT_BAR * float(np.abs(want).max())
        w_direct = max(w_direct, 0.0 if d == 0 else d / bar if bar > 0 else np.inf)
        if rp["path1_state"][h] == 0 and path1_rel_bar(rp["cond"][h]) <= PATH1_SKIP and abs(rp["jr_max"][h] - 10.0) > CLAMP_EDGE:
            want = rp["grad_path1"][h].T
            d = float(np.abs(dev["slab1"][s] - want).max())
            bar = path1_rel_bar(rp["cond"][h]) * float(np.abs(want).max())
            w_p1 = max(w_p1, 0.0 if d == 0 else d / bar if bar > 0 else np.inf)
            n_p1 += 1
    return w_direct, w_p1, n_p1


# ---------------------------------------------------------------- the reference's own spread (path-I bar constant)
def path1_reference_spread(O, c, ref, h):
    """jacobeanR of hypothesis h from the same Jacobian rows summed in the oracle's cell order (x outer, y inner) and in
    reversed order, both by the oracle's routines: (spread / (cond * 2^-53 * max|jacobeanR|), cond, rows J [n,6] in the
    oracle's order, their cells)."""
    H, W, cam = c["H"], c["W"], c["cam"]
    pose = np.ascontiguousarray(ref["ref_hyps"][h])
    e = int(c["ha"][h])
    m = ref["maps"][h].reshape(H, W)
    rows, cells = [], []
    for x in range(W):
        for y in range(H):
            if m[y, x]:
                px = x * cam["sub_sampling"] + cam["sub_sampling"] // 2 - cam["shift_x"]
                py = y * cam["sub_sampling"] + cam["sub_sampling"] // 2 - cam["shift_y"]
                _, r = O.norm_jac_row(pose[:3].copy(), pose[3:].copy(), cam["focal"], cam["ppx"], cam["ppy"],
                                      c["coords"][e, :, y, x], (float(px), float(py)), cam["max_reproj"])
                rows.append(r)
                cells.append(y * W + x)
    J = np.array(rows)

    def jac_r(Jo):
        A = np.zeros((6, 6))
        for r in Jo:  # every entry sums its products row after row, as the oracle's loop does
            A += np.outer(r, r)
        return A, -(O.pinv_sym6(A) @ Jo.T)

    A, PI = jac_r(J)
    _, PI2 = jac_r(J[::-1])
    w = np.linalg.eigvalsh(A)
    cond = np.inf if w[0] <= 0 else w[-1] / w[0]
    spread = float(np.abs(PI - PI2[:, ::-1]).max()) / max(float(np.abs(PI).max()), 1e-300)
    return spread / (cond * EPS53), cond, J, np.array(cells), A
