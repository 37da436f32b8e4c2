"""GPU tests of what the Python front end hands to the library: the helpers of esac_amd/api.py (`_frame_table`, `_frame_stride`,
`Engine._on_device`, `_call_params`, `_stage_gradients`, `_shared_call`) can go wrong without any sentence changing -- a wrong
stride, a table that is not copied, a missing `reserved` word, a counter off by B.  `eng.lib` is wrapped in a forwarding proxy
that notes, per C call, the entry point, B, both frame strides, the ragged flag and the bytes of the per-frame table at call time;
everything is forwarded, so the kernels run.  Expected values are derived from the inputs, none is recorded.

Shapes: B = 2, E = 2, N = 16; the grids 8x12 and 12x8 packed by `pack_frames` (equal cell count, transposed), the shared-shape
8x12 forms [B,E,3,H,W] and [E,3,H,W]; cams as scalars and per frame; shapes None and a table.  (Both widths are multiples of 4;
a width that is not is a kernel route, held by tests/test_gpu_ragged.py and tests/test_gpu_ragged_backward.py.)

The last tests are a guard that the proxy forwarded: the outputs of each ragged call equal, frame by frame and bit for bit, the
same frames sent through the shared-shape call one at a time -- with the helpers of tests/test_gpu_ragged.py and
tests/test_gpu_ragged_backward.py (`_run`, `_run_ragged`, `_assert_same_bits`), no bar of this file's own."""
import ctypes as C

import numpy as np
import pytest
import torch

from esac_amd import api
from tests import test_gpu_ragged as RF
from tests import test_gpu_ragged_backward as RB

pytestmark = pytest.mark.gpu

B, E, N, K, SUB = 2, 2, 16, 3, 8
GRIDS = [(8, 12), (12, 8)]
SCORE = (10.0, 100.0, 0.5, 100.0, SUB)
LOSS = (1.0, 100.0, 100.0)
# entry point -> positions (the context is argument 0) of B, the maps' frame stride, the gradients' frame stride, the table, the flag
NOTED = {
    "esac_hip_forward_batch": (1, 3, None, None, None), "esac_hip_forward_batch_cams": (1, 3, None, 6, None),
    "esac_hip_forward_batch_shapes": (1, 3, None, 6, None),
    "esac_hip_backward_batch": (1, 3, 5, None, None), "esac_hip_backward_batch_cams": (1, 3, 5, 8, None),
    "esac_hip_backward_batch_shapes": (1, 3, 5, 8, None), "esac_hip_backward_batch_dev": (1, 3, 5, 8, None),
    "esac_hip_backward_batch_dev_shapes": (1, 3, 5, 8, None), "esac_hip_verify_batch": (1, 4, None, 9, 10),
}


class LibProxy:
    """Forwards every attribute of the ctypes library; notes the calls of NOTED."""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name not in NOTED:
            return fn
        at_b, at_sc, at_g, at_table, at_flag = NOTED[name]

        def call(*args):
            ptr = args[at_table] if at_table is not None else None
            ptr = ptr.value if isinstance(ptr, C.c_void_p) else ptr
            table = np.frombuffer(C.string_at(ptr, args[at_b] * api.CAM_DTYPE.itemsize), api.CAM_DTYPE).copy() if ptr else None
            self.calls.append(dict(name=name, B=args[at_b], sc_stride=args[at_sc], grad_stride=None if at_g is None else args[at_g],
                                   table=table, table_ptr=ptr or None,
                                   ragged=bool(args[at_flag]) if at_flag is not None else name.endswith("_shapes")))
            return fn(*args)
        return call


@pytest.fixture
def calls(engine, monkeypatch):
    proxy = LibProxy(engine.lib)
    monkeypatch.setattr(engine, "lib", proxy)
    state = api.get_rng_state()
    yield proxy.calls
    torch.cuda.synchronize()
    api.set_seed(*state)


def _frames(form):
    """(frames, assignments, ground truths) of a form: the two grids, or the 8x12 grid twice."""
    return RB._inputs(GRIDS if form == "ragged" else [GRIDS[0]] * B, experts=E, n=N)


def _cam_columns(frames):
    return ([f["shift"][0] for f in frames], [f["shift"][1] for f in frames], [f["focal"] for f in frames],
            [f["ppx"] for f in frames], [f["ppy"] for f in frames])


def _case(form, per_frame, dev):
    """The arguments of one call and what must reach the library: dict(sc, ha, gts, cam_args, shapes, stride, table, shape)."""
    frames, has, gts = _frames(form)
    cols = _cam_columns(frames)
    maps = [torch.from_numpy(f["coords"]) for f in frames]
    shapes = None
    if form == "ragged":
        sc, shapes = api.pack_frames(maps, device=dev)
        assert shapes == GRIDS
        stride = int(sc.shape[1])
    elif form == "shared":
        sc, stride = maps[0].to(dev), 0
    else:
        sc, stride = torch.stack(maps).to(dev), E * 3 * GRIDS[0][0] * GRIDS[0][1]
    table = None
    if per_frame or shapes is not None:
        table = api.make_cams(*(cols if per_frame else [[c[0]] * B for c in cols]))
        if shapes is not None:
            table["reserved"][:, :2] = np.asarray(shapes, np.int32)
    return dict(frames=frames, sc=sc, ha=torch.from_numpy(np.stack(has)).to(dev), gts=torch.from_numpy(np.stack(gts)).to(dev),
                cam_args=cols if per_frame else tuple(c[0] for c in cols), shapes=shapes, stride=stride, table=table,
                shape=(N,) + tuple(api.capacity_shape(shapes) if shapes is not None else GRIDS[0]))


def _check_note(note, name, case, grad_stride=None):
    print(note["name"], note["B"], note["sc_stride"], note["grad_stride"], note["ragged"], note["table"])
    assert note["name"] == name
    assert note["B"] == B and note["sc_stride"] == case["stride"] and note["grad_stride"] == grad_stride
    assert note["ragged"] == (case["shapes"] is not None)
    if case["table"] is None:
        assert note["table"] is None and note["table_ptr"] is None
    else:
        assert note["table"].tobytes() == case["table"].tobytes()   # (every field, the reserved words among them)
        if case["shapes"] is not None:
            assert note["table"]["reserved"][:, :2].tolist() == [list(s) for s in case["shapes"]]


FORMS = ["5d", "shared", "ragged"]
CAMS = pytest.mark.parametrize("per_frame", [False, True], ids=["scalars", "per_frame"])


# ---------------------------------------------------------------- forward batches
@CAMS
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("asynchronous", [False, True], ids=["host", "async"])
def test_forward_batch_calls(engine, calls, form, per_frame, asynchronous):
    case = _case(form, per_frame, engine.device)
    api.set_seed(1305, 5000)
    kw = dict(shapes=case["shapes"]) if case["shapes"] is not None else {}
    if asynchronous:
        out = api.forward_batch_async(case["sc"], case["ha"], *case["cam_args"], *SCORE, **kw)
        assert out["call"] == 5000 and tuple(out["records"].shape) == (B, api.RES_DOUBLES)
    else:
        poses = torch.zeros(B, 4, 4)
        experts = api.forward_batch(case["sc"], case["ha"], poses, *case["cam_args"], *SCORE, **kw)
        assert len(experts) == B
    assert len(calls) == 1
    _check_note(calls[0], "esac_hip_forward_batch" + ("_shapes" if form == "ragged" else "_cams" if per_frame else ""), case)
    assert api.get_rng_state() == (1305, 5000 + B)
    assert engine._shape == case["shape"]


# ---------------------------------------------------------------- training batches
@CAMS
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("asynchronous", [False, True], ids=["blocking", "async"])
def test_backward_batch_calls(engine, calls, form, per_frame, asynchronous):
    case = _case(form, per_frame, engine.device)
    api.set_seed(1305, 6000)
    if form == "ragged":
        grads = torch.zeros(B, case["stride"] + 4, dtype=torch.float32, device=engine.device)   # (a row stride of its own)
        fn = api.backward_batch_shapes_async if asynchronous else api.backward_batch_shapes
        out = fn(case["sc"], grads, case["ha"], case["gts"], *LOSS, *case["cam_args"], *SCORE, shapes=case["shapes"])
    else:
        grads = torch.zeros((B, E, 3) + GRIDS[0], dtype=torch.float32, device=engine.device)
        out = (api.backward_batch_async if asynchronous else api.backward_batch)(case["sc"], grads, case["ha"], case["gts"], *LOSS,
                                                                                *case["cam_args"], *SCORE)
    assert len(out) == B and len(calls) == 1
    if asynchronous:
        name = "esac_hip_backward_batch_dev" + ("_shapes" if form == "ragged" else "")
    else:
        name = "esac_hip_backward_batch" + ("_shapes" if form == "ragged" else "_cams" if per_frame else "")
    _check_note(calls[0], name, case, grad_stride=int(grads.stride(0)))
    assert api.get_rng_state() == (1305, 6000 + B)
    assert engine._shape == case["shape"]
    torch.cuda.synchronize()
    engine.check()


# ---------------------------------------------------------------- pose verification
@CAMS
@pytest.mark.parametrize("form", FORMS)
def test_verify_batch_calls(engine, calls, form, per_frame):
    case = _case(form, per_frame, engine.device)
    poses = torch.zeros(B, K, 6, dtype=torch.float64)
    poses[:, :, 5] = 2.0
    api.set_seed(1305, 7000)
    shape_before = engine._shape
    kw = dict(shapes=case["shapes"]) if case["shapes"] is not None else {}
    out = api.verify_batch(case["sc"], poses, torch.zeros(B, dtype=torch.int64), *case["cam_args"], *SCORE, **kw)
    assert tuple(out.shape) == (B, K, api.VERIFY_DOUBLES) and len(calls) == 1
    _check_note(calls[0], "esac_hip_verify_batch", case)
    assert api.get_rng_state() == (1305, 7000)   # (draws no RNG stream)
    assert engine._shape == shape_before


# ---------------------------------------------------------------- a caller's own table
def _own_table(frames):
    table = RB._cams(frames)   # (reserved holds -12345: a ragged call fills ITS copy)
    return table, table.copy()


@pytest.mark.parametrize("call", ["forward_batch", "backward_batch_shapes", "backward_batch_shapes_async", "verify_batch"])
def test_a_ragged_call_copies_the_callers_table(engine, calls, call):
    case = _case("ragged", True, engine.device)
    table, before = _own_table(case["frames"])
    H, W = api.capacity_shape(GRIDS)
    p = RB._table_params(engine, E, H, W, K if call == "verify_batch" else N, 100.0, 8000)
    grads = torch.zeros_like(case["sc"])
    if call == "forward_batch":
        engine.forward_batch(case["sc"], case["ha"], p, cams=table, shapes=GRIDS)
    elif call == "backward_batch_shapes":
        engine.backward_batch_shapes(case["sc"], grads, case["ha"], case["gts"].cpu().numpy(), *LOSS, p, GRIDS, cams=table)
    elif call == "backward_batch_shapes_async":
        engine.backward_batch_shapes_async(case["sc"], grads, case["ha"], case["gts"], *LOSS, p, GRIDS, cams=table)
    else:
        engine.verify_batch(case["sc"], torch.zeros(B, K, 6, dtype=torch.float64), torch.zeros(B, dtype=torch.int64), p, cams=table, shapes=GRIDS)
    torch.cuda.synchronize()
    assert table.tobytes() == before.tobytes()   # the caller's padding stays
    want = before.copy()
    want["reserved"][:, :2] = np.asarray(GRIDS, np.int32)
    note = calls[-1]
    assert note["ragged"] and note["table_ptr"] != table.ctypes.data and note["table"].tobytes() == want.tobytes()


@pytest.mark.parametrize("call", ["forward_batch", "backward_batch", "backward_batch_async", "verify_batch"])
def test_a_shared_shape_call_passes_the_callers_table_itself(engine, calls, call):
    case = _case("5d", True, engine.device)
    table, before = _own_table(case["frames"])
    p = RB._table_params(engine, E, GRIDS[0][0], GRIDS[0][1], K if call == "verify_batch" else N, 100.0, 8100)
    grads = torch.zeros_like(case["sc"])
    if call == "forward_batch":
        engine.forward_batch(case["sc"], case["ha"], p, cams=table)
    elif call == "backward_batch":
        engine.backward_batch(case["sc"], grads, case["ha"], case["gts"].cpu().numpy(), *LOSS, p, cams=table)
    elif call == "backward_batch_async":
        engine.backward_batch_async(case["sc"], grads, case["ha"], case["gts"], *LOSS, p, cams=table)
    else:
        engine.verify_batch(case["sc"], torch.zeros(B, K, 6, dtype=torch.float64), torch.zeros(B, dtype=torch.int64), p, cams=table)
    torch.cuda.synchronize()
    note = calls[-1]
    assert not note["ragged"] and note["table_ptr"] == table.ctypes.data and note["table"].tobytes() == before.tobytes()
    assert table.tobytes() == before.tobytes()


# ---------------------------------------------------------------- the guard: the proxy forwarded
def test_ragged_forward_equals_the_shared_shape_calls_frame_by_frame(engine, calls):
    frames, has, _ = RF._inputs(GRIDS, E, N)
    ragged = RF._run(engine, frames, has)
    rows = {k: [] for k in ("res", "scores") + RF.FRAME_BUFS}
    for b, f in enumerate(frames):
        h, w = f["coords"].shape[2:]
        p = engine.make_params(E, h, w, N, shift_x=f["shift"][0], shift_y=f["shift"][1], focal=f["focal"], ppx=f["ppx"], ppy=f["ppy"],
                               sub_sampling=SUB, seed=RF.SEED, call=RF.CALL0 + b)
        scores = torch.empty(1, N, dtype=torch.float64, device=engine.device)
        rows["res"].append(engine.forward_batch(torch.from_numpy(f["coords"])[None].to(engine.device),
                                                torch.from_numpy(has[b])[None].to(engine.device), p, scores_out=scores)[0])
        rows["scores"].append(scores.cpu().numpy()[0])
        for which in RF.FRAME_BUFS:
            rows[which].append(engine.read_forward_frames(which, 1)[0])
    singles = {k: np.stack(v) for k, v in rows.items()}
    singles["mode"] = engine.refine_info()["mode"]
    print("ragged", ragged["res"][:, :3], "one at a time", singles["res"][:, :3], ragged["mode"], singles["mode"])
    RF._assert_same_bits(ragged, singles, "ragged forward batch vs shared-shape calls of one frame")
    assert [c["name"] for c in calls] == ["esac_hip_forward_batch_shapes"] + ["esac_hip_forward_batch"] * B
    # ... and the asynchronous call's device records are the host's
    packed, shapes = api.pack_frames([torch.from_numpy(f["coords"]) for f in frames], device=engine.device)
    records = torch.zeros(B, api.RES_DOUBLES, dtype=torch.float64, device=engine.device)
    engine.forward_batch(packed, torch.from_numpy(np.stack(has)).to(engine.device), RF._params(engine, E, *api.capacity_shape(shapes), N, RF.CALL0),
                         result_out=records, want_host=False, cams=RF._cams(frames), shapes=shapes)
    torch.cuda.synchronize()
    got = records.cpu().numpy()
    np.testing.assert_array_equal(got[:, :api.RES_VALID], ragged["res"][:, :api.RES_VALID])


@pytest.mark.parametrize("asynchronous", [False, True], ids=["blocking", "async"])
def test_ragged_backward_equals_the_shared_shape_calls_frame_by_frame(engine, calls, asynchronous):
    frames, has, gts = RB._inputs(GRIDS, experts=E, n=N)
    g0 = RB._g0(frames)
    ragged = RB._run_ragged(engine, frames, has, gts, g0, asynchronous=asynchronous)
    singles = {k: [] for k in ("out", "grads") + RB.FRAME_BUFS}
    for b, f in enumerate(frames):
        g = torch.from_numpy(g0[b].copy())[None].to(engine.device)
        out = engine.backward_batch(torch.from_numpy(f["coords"])[None].to(engine.device), g, torch.from_numpy(has[b])[None].to(engine.device),
                                    gts[b][None], *RB.LOSS, RB._frame_params(engine, f, N, RB.ALPHA, RB.CALL0 + b))
        singles["out"].append(out[0])
        singles["grads"].append(g[0].cpu().numpy())
        for which in RB.FRAME_BUFS:
            singles[which].append(engine.read_frames(which, 1)[0])
    singles["out"] = np.stack(singles["out"])
    print("ragged", ragged["out"], "one at a time", singles["out"])
    RB._assert_same_bits(ragged, singles, "ragged training batch vs shared-shape calls of one frame")
    assert [c["name"] for c in calls] == ["esac_hip_backward_batch_dev_shapes" if asynchronous else "esac_hip_backward_batch_shapes"] + \
        ["esac_hip_backward_batch"] * B


def test_ragged_verify_equals_the_shared_shape_calls_frame_by_frame(engine, calls):
    frames, _, gts = RB._inputs(GRIDS, experts=E, n=N)
    poses = torch.from_numpy(np.stack([np.stack([g] * K) for g in gts]))   # float32 [B,K,4,4]: the perturbed ground truths
    experts = torch.tensor([b % E for b in range(B)])
    cols = _cam_columns(frames)
    ragged = api.verify_batch([torch.from_numpy(f["coords"]).to(engine.device) for f in frames], poses, experts, *cols, *SCORE, shapes=GRIDS)
    for b, f in enumerate(frames):
        one = api.verify_batch(torch.from_numpy(f["coords"])[None].to(engine.device), poses[b:b + 1], experts[b:b + 1],
                               *(c[b] for c in cols), *SCORE)
        print("frame", b, ragged[b, 0, :5].cpu().numpy(), one[0, 0, :5].cpu().numpy())
        np.testing.assert_array_equal(ragged[b].cpu().numpy(), one[0].cpu().numpy())
    assert [(c["name"], c["ragged"]) for c in calls] == [("esac_hip_verify_batch", True)] + [("esac_hip_verify_batch", False)] * B
