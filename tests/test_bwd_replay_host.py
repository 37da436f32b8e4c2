"""The replay of the training path's gradient stages (tests/bwd_replay.py) checked against the oracle on the CPU, before
any GPU is involved: the split of esac_oracle_backward changed nothing (the replay fed with the oracle's OWN stages
returns the oracle's slabs and tensor bit for bit), the numpy form of the ordered accumulation is the oracle's, the
frozen case list reaches every workgroup-uniform branch of the gradient kernels, the constant of the path-I bar is
measured on the reference arithmetic alone, and the kernels' own headers compiled for the host meet the bars that
test_gpu_backward_stages.py holds the device to.
"""
import ctypes as C

import numpy as np
import pytest

from tests import bwd_replay as R

NAMES = list(R.CASES)


@pytest.fixture(scope="module")
def runs(oracle):
    """One oracle run and one replay on the oracle's own stages per case, every tensor PRE-FILLED; shared, never modified."""
    out = {}
    for name in NAMES:
        c = R.make_case(name, prefill=True)
        ref = R.run_oracle(oracle, c)
        out[name] = (c, ref, R.replay_with_inputs(oracle, c, R.oracle_stages(ref)))
    return out


@pytest.fixture(scope="module")
def spreads(runs, oracle):
    """path1_reference_spread of every slot that computes a path I, once."""
    return {(name, int(h)): R.path1_reference_spread(oracle, c, ref, h) for name, (c, ref, rp) in runs.items()
            for h in rp["selected"] if ref["path1_state"][h] in (0, 3)}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


@pytest.mark.parametrize("name", NAMES)
def test_replay_of_the_oracles_own_stages_is_the_oracle(runs, oracle, name):
    c, ref, rp = runs[name]
    assert np.abs(c["g0"]).min() > 0  # a non-zero pre-fill under every entry
    for k in ("grad_path1", "grad_path2", "grad", "score_grads", "dloss"):
        np.testing.assert_array_equal(_bits(rp[k]), _bits(ref[k]), err_msg=k)
    for k in ("grad_direct", "support", "support_raw", "jtj", "jr_max", "path1_state", "dpnp", "dpnp_state", "dpnp_max"):
        np.testing.assert_array_equal(rp[k], ref[k], err_msg=k)
    # the optional inputs, fed with the values the text derives itself, change nothing either
    st = dict(R.oracle_stages(ref), score_grads=ref["score_grads"], dloss=ref["dloss"])
    rp2 = R.replay(oracle, c, st)
    for k in ("grad_path1", "grad_path2", "grad"):
        np.testing.assert_array_equal(_bits(rp2[k]), _bits(ref[k]), err_msg=k)
    # path II = direct term everywhere + the support terms on the sampled cells
    for h in rp["selected"]:
        want = ref["grad_direct"][h].copy()
        for j, (x, y) in enumerate(ref["sample_xy"][h]):
            want[y * c["W"] + x] += ref["support"][h, j]
        np.testing.assert_array_equal(want, ref["grad_path2"][h])
    # a dropped dPNP matrix leaves no support term; support_raw is the term had the clamp not dropped it
    for h in rp["selected"]:
        if ref["dpnp_state"][h] == 0:
            np.testing.assert_array_equal(ref["support_raw"][h], ref["support"][h])
        else:
            assert not ref["support"][h].any() and not ref["dpnp"][h].any()
            assert (ref["dpnp_state"][h] == 2) == (ref["dpnp_max"][h] > 10)
    if name in R.ALL_SELECTED:
        assert len(rp["selected"]) == c["N"]  # the slot counts the accumulation's edges need: 1, 8, 9, 64, 65, 130
        assert (3 * c["P"]) % 256 != 0        # ... with a ragged last tile of the accumulation's 256-thread workgroups


@pytest.mark.parametrize("name", NAMES)
def test_numpy_accumulation_is_the_oracles(runs, name):
    """v = float32(float64(v) + (p g1 + g2)), slot by slot in ascending hypothesis order, per expert: the reference of the
    device's k_bwd_accumulate check."""
    c, ref, rp = runs[name]
    sel = rp["selected"]
    got = R.accumulate(c["g0"], c["ha"], sel, ref["probs"], R.planar(ref["grad_path1"][sel]), R.planar(ref["grad_path2"][sel]))
    np.testing.assert_array_equal(_bits(got), _bits(ref["grad"]))
    owners = set(int(e) for e in c["ha"][sel])
    for e in range(c["E"]):
        if e not in owners:
            np.testing.assert_array_equal(_bits(ref["grad"][e]), _bits(c["g0"][e]))  # untouched
    if name in R.ALL_SELECTED and len(sel) >= 8:
        # the order is part of the form: the same terms added in reversed slot order round differently somewhere (gradients
        # and pre-fill are both of order one on these frames)
        rev = R.accumulate(c["g0"], c["ha"], sel[::-1], ref["probs"], R.planar(ref["grad_path1"][sel[::-1]]),
                           R.planar(ref["grad_path2"][sel[::-1]]))
        assert not np.array_equal(_bits(rev), _bits(ref["grad"]))


def test_three_expert_case_leaves_one_expert_without_slots(runs):
    c, ref, rp = runs["three_experts_n130"]
    own = [int((c["ha"][rp["selected"]] == e).sum()) for e in range(3)]
    assert own[0] > 0 and own[1] > 0 and own[2] == 0, own


def test_branch_census_on_the_oracle_alone(runs):
    """Every workgroup-uniform branch of k_bwd_paths is reached by some case, on the oracle alone."""
    n = dict(no_map=0, clamped=0, ill=0, dpnp_failed=0, dpnp_clamped=0, beyond=0, slots=0, p1=0, skipped=0)
    for name in NAMES:
        c, ref, rp = runs[name]
        sel = rp["selected"]
        st, ds = ref["path1_state"][sel], ref["dpnp_state"][sel]
        assert (st >= 0).all() and (ds >= 0).all()
        n["slots"] += len(sel)
        n["no_map"] += int(((st == 1) | (st == 2)).sum())     # fewer than 4 inliers or no accepted re-fit: zero slab
        n["clamped"] += int((st == 3).sum())                  # |jacobeanR| > 10
        n["ill"] += int((rp["cond"][sel] > 1e12).sum())       # the rank-deficient route
        n["dpnp_failed"] += int((ds == 1).sum())
        n["dpnp_clamped"] += int((ds == 2).sum())
        for h in sel:
            if ref["score_grads"][h] != 0:
                n["beyond"] += int((np.abs(ref["grad_direct"][h]).sum(1) == 0).sum())  # cells beyond max_reproj (or |Z| < EPS)
            if st[list(sel).index(h)] in (1, 2):
                assert not ref["grad_path1"][h].any()
            if st[list(sel).index(h)] == 3:
                assert not ref["grad_path1"][h].any() and ref["jr_max"][h] > 10
        live = (st == 0) | (st == 3)
        n["p1"] += int(live.sum())
        n["skipped"] += int((R.path1_rel_bar(rp["cond"][sel][live]) > R.PATH1_SKIP).sum())
    print("branch census:", n)
    for k in ("no_map", "clamped", "ill", "dpnp_failed", "dpnp_clamped", "beyond"):
        assert n[k] > 0, (k, n)
    # the max_reproj branch of the frame built for it
    c, ref, rp = runs["shifted_n40"]
    assert c["cam"]["max_reproj"] == 30.0 and any((np.abs(ref["grad_direct"][h]).sum(1) == 0).any() for h in rp["selected"])
    # the slots path I can only be held to its zero / non-zero state on: a small share of those that compute one
    assert n["skipped"] <= R.PATH1_SKIP_SHARE * n["p1"], n


def test_path1_bar_constant_measured_on_the_reference(runs, spreads):
    """jacobeanR from the same Jacobian rows summed in the oracle's cell order and in reversed order, by the oracle's own
    routines: the spread in units of cond_2(J^T J) * 2^-53 * max|jacobeanR| over every path-I slot of the case list stays
    within PATH1_REF_SPREAD (LAB_NOTES.md records the figure per case)."""
    worst, conds = {}, []
    for name in NAMES:
        c, ref, rp = runs[name]
        w = 0.0
        for h in rp["selected"]:
            if ref["path1_state"][h] in (0, 3):
                ratio, cond, J, cells, A = spreads[name, int(h)]
                np.testing.assert_array_equal(A, ref["jtj"][h])  # the rows and their order really are the oracle's
                w = max(w, ratio)
                conds.append(cond)
        worst[name] = w
    print("path-I reference spread / (cond 2^-53 max|jacobeanR|):", {k: round(v, 2) for k, v in worst.items()},
          "median cond %.3g" % np.median(conds))
    assert max(worst.values()) <= R.PATH1_REF_SPREAD, worst
    assert max(worst.values()) > 0.5 * R.PATH1_REF_SPREAD  # the constant is the measurement, not a loose guess


@pytest.fixture(scope="module")
def probe():
    from tests.native import build
    lib = C.CDLL(build.build())
    f, vp = C.c_float, C.c_void_p
    lib.probe_dproject_dobj.argtypes = [f, f, f, f, f, vp, vp, f, f, f, f, vp]
    lib.probe_norm_jac_row.argtypes = [vp, vp, f, f, f, f, f, f, f, f, f, vp]
    lib.probe_inv_spd6.argtypes = [vp, vp]
    lib.probe_pinv_sym6.argtypes = [vp, vp]
    return lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def test_host_compiled_device_headers_meet_the_bars(runs, spreads, oracle, probe):
    """bwd_math.hpp compiled for the host, on the cells and normal matrices of the case list: norm_jac_row and dproject_dobj
    (the only per-cell routines of the direct term and of jacobeanR's rows) equal the oracle's bit for bit -- inside any bar;
    jacobeanR through inv_spd6 (LDL^T), or through pinv_sym6_jacobi where that reports rank deficiency, and through
    pinv_sym6_jacobi alone (the strict mode) stays within the path-I bar of every slot the GPU test compares."""
    iu = np.triu_indices(6)
    worst = 0.0
    n_spd = n_pinv = 0
    for name in NAMES:
        c, ref, rp = runs[name]
        cam = c["cam"]
        for k, h in enumerate(rp["selected"]):
            if ref["path1_state"][h] not in (0, 3):
                continue
            _, cond, J, cells, A = spreads[name, int(h)]
            pose = np.ascontiguousarray(ref["ref_hyps"][h])
            e = int(c["ha"][h])
            if k < 3:  # the per-cell routines on every inlier of the first slots
                for q, cell in enumerate(cells):
                    y, x = divmod(int(cell), c["W"])
                    px = float(x * cam["sub_sampling"] + cam["sub_sampling"] // 2 - cam["shift_x"])
                    py = float(y * cam["sub_sampling"] + cam["sub_sampling"] // 2 - cam["shift_y"])
                    X, Y, Z = (float(v) for v in c["coords"][e, :, y, x])
                    row, d_a = np.zeros(6), np.zeros(3)
                    probe.probe_norm_jac_row(_p(pose[:3].copy()), _p(pose[3:].copy()), cam["focal"], cam["ppx"], cam["ppy"], X, Y, Z,
                                             px, py, cam["max_reproj"], _p(row))
                    np.testing.assert_array_equal(row, J[q])
                    probe.probe_dproject_dobj(px, py, X, Y, Z, _p(pose[:3].copy()), _p(pose[3:].copy()), cam["focal"], cam["ppx"],
                                              cam["ppy"], cam["max_reproj"], _p(d_a))
                    np.testing.assert_array_equal(d_a, oracle.dproject_dobj((px, py), (X, Y, Z), pose[:3], pose[3:], cam["focal"],
                                                                            cam["ppx"], cam["ppy"], cam["max_reproj"]))
            bar = R.path1_rel_bar(cond)
            if bar > R.PATH1_SKIP:
                continue
            want = -(oracle.pinv_sym6(A) @ J.T)
            U = np.ascontiguousarray(A[iu])
            inv, pinv = np.zeros((6, 6)), np.zeros((6, 6))
            ok = probe.probe_inv_spd6(_p(U), _p(inv))
            probe.probe_pinv_sym6(_p(U), _p(pinv))
            n_spd += ok == 1
            n_pinv += ok != 1
            for Ai in ((inv if ok == 1 else pinv), pinv):
                got = -(Ai @ J.T)
                ratio = float(np.abs(got - want).max()) / (bar * float(np.abs(want).max()))
                worst = max(worst, ratio)
    print("host-compiled inverses: worst jacobeanR error / bar %.3g (%d slots by inv_spd6, %d by the pseudo-inverse)" % (worst, n_spd, n_pinv))
    assert n_spd > 100
    assert worst <= 1.0, worst
