"""CPU tests of the ragged TRAINING front end: `esac.backward_batch_shapes` / `esac.backward_batch_shapes_async` with their
`shapes=` / `experts=` keywords (argument errors name the argument, touch no device and leave the call counter; functions of their
own, because the parameter lists of `backward_batch` / `backward_batch_async` are held as they are), `esac.unpack_frames`,
the list form of `harness.train_batch`, and the two new C ABI symbols in the header and in the ctypes binding.  No GPU."""
import inspect
import os
import re

import pytest
import torch

import esac
from esac_amd import api, harness

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(12, 16), (16, 12), (12, 18), (12, 16)]
E, N, S = 3, 32, 1944  # 3 * 3 * 216
LOSS = (1.0, 100.0, 100.0)
SOLVER = (0, 0, 525.0, 64.0, 48.0, 10.0, 100.0, 0.5, 100.0, 8)


@pytest.fixture
def no_device(monkeypatch):
    """Any attempt to open an engine (the first thing that touches a device) fails the test."""
    def boom(*a, **k):
        raise AssertionError("the call touched the device")
    monkeypatch.setattr(api, "engine", boom)


def _maps(shapes=SHAPES, experts=E, seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(experts, 3, h, w, generator=g) for h, w in shapes]


def _good():
    return dict(sc=torch.zeros(4, S), grads=torch.zeros(4, S), ha=torch.zeros(4, N, dtype=torch.int64), gt=torch.eye(4).repeat(4, 1, 1),
                shapes=SHAPES, experts=None, cam=SOLVER)


def _call(fn, a):
    return fn(a["sc"], a["grads"], a["ha"], a["gt"], *LOSS, *a["cam"], shapes=a["shapes"], experts=a["experts"])


def _bad_calls():
    grads_list = [torch.zeros(E, 3, h, w) for h, w in SHAPES]
    return [
        # (id, overrides, needles, which calls: "both" / "blocking" / "async")
        ("shapes count", dict(shapes=SHAPES[:3]), ["shapes must hold one (h, w) pair per frame (4), found 3"], "both"),
        ("shapes type", dict(shapes=7), ["shapes must hold one (h, w) pair per frame (4), found int"], "both"),
        ("shapes entry", dict(shapes=SHAPES[:3] + [(12,)]), ["shapes[3] must be a pair of integers"], "both"),
        ("shapes too small", dict(shapes=SHAPES[:3] + [(2, 16)]), ["shapes[3] = 2x16 is no legal grid"], "both"),
        ("shapes vs maps", dict(sc=_maps(), shapes=[(12, 16), (12, 16), (12, 18), (12, 16)]), ["shapes[1] = 12x16, sceneCoordinates[1] is 16x12"], "blocking"),
        ("maps length", dict(sc=_maps()[:3]), ["sceneCoordinates holds 3 frames, hypAssignment 4"], "blocking"),
        ("maps list async", dict(sc=_maps()), ["sceneCoordinates must be the packed device tensor"], "async"),
        ("packed rank", dict(sc=torch.zeros(4, E, 3, 12, 18)), ["sceneCoordinates must be the packed float32 [B,S] tensor"], "both"),
        ("packed batch", dict(sc=torch.zeros(3, S)), ["batch sizes of sceneCoordinates and hypAssignment differ"], "both"),
        ("packed S % 4", dict(sc=torch.zeros(4, S + 2)), ["sceneCoordinates [B,S] needs S to be a multiple of 4"], "both"),
        ("packed short", dict(sc=torch.zeros(4, S), experts=4), ["too short for 4 expert(s)"], "both"),
        ("experts type", dict(experts=0), ["experts must be a positive int"], "both"),
        ("hypAssignment dtype", dict(ha=torch.zeros(4, N, dtype=torch.int32)), ["hypAssignment must be a non-empty int64 [B,N]"], "both"),
        ("hypAssignment rank", dict(ha=torch.zeros(N, dtype=torch.int64)), ["hypAssignment must be a non-empty int64 [B,N]"], "both"),
        ("gtPoses shape", dict(gt=torch.eye(4).repeat(3, 1, 1)), ["gtPoses must be float32 [B,4,4]"], "both"),
        ("gtPoses dtype", dict(gt=torch.eye(4, dtype=torch.float64).repeat(4, 1, 1)), ["gtPoses must be float32 [B,4,4]"], "both"),
        ("grads dense 5-D", dict(grads=torch.zeros(4, E, 3, 12, 18)), ["outGradients must be a packed float32 [B,S] tensor"], "both"),
        ("grads dtype", dict(grads=torch.zeros(4, S, dtype=torch.float64)), ["outGradients must be a packed float32 [B,S] tensor"], "both"),
        ("grads batch", dict(grads=torch.zeros(3, S)), ["batch sizes of outGradients and hypAssignment differ"], "both"),
        ("grads short", dict(grads=torch.zeros(4, S - 1)), ["outGradients [B,1943] is too short for 3 expert(s)", "3*E*h*w = 1944"], "both"),
        ("grads list length", dict(grads=grads_list[:3]), ["outGradients holds 3 frames, hypAssignment 4"], "blocking"),
        ("grads list shape", dict(grads=grads_list[:2] + [torch.zeros(E, 3, 18, 12)] + grads_list[3:]), ["outGradients[2] must be float32 [3, 3, 12, 18]"], "blocking"),
        ("grads list dtype", dict(grads=grads_list[:3] + [grads_list[3].double()]), ["outGradients[3] must be float32 [3, 3, 12, 16]"], "blocking"),
        ("grads list async", dict(grads=grads_list), ["outGradients must be the packed float32 [B,S] device tensor"], "async"),
        ("assignment range", dict(ha=torch.full((4, N), 3, dtype=torch.int64)), ["hypAssignment values must lie in [0,3)"], "blocking"),
        ("camera", dict(cam=(0, 0, [525.0, 0.0, 525.0, 525.0]) + SOLVER[3:]), ["focalLength must be positive (frame 1"], "both"),
        ("camera length", dict(cam=(0, 0, 525.0, [1.0, 2.0]) + SOLVER[4:]), ["ppointX must be a scalar or hold one value per frame (4)"], "both"),
        ("host grads async", dict(), ["outGradients must be a device tensor"], "async"),
    ]


def _cases():
    out = []
    for case in _bad_calls():
        for name, fn in (("blocking", api.backward_batch_shapes), ("async", api.backward_batch_shapes_async)):
            if case[3] in ("both", name):
                out.append(pytest.param(fn, case, id="%s-%s" % (name, case[0])))
    return out


@pytest.mark.parametrize("fn, case", _cases())
def test_shapes_argument_errors_name_the_argument_and_touch_no_device(no_device, fn, case):
    _, over, needles, _ = case
    args = _good()
    args.update(over)
    call0 = api._state["call"]
    with pytest.raises(RuntimeError) as e:
        _call(fn, args)
    who = "esac.backward_batch_shapes_async" if fn is api.backward_batch_shapes_async else "esac.backward_batch_shapes"
    assert str(e.value).startswith(who + ":"), str(e.value)
    for n in needles:
        assert n in str(e.value), str(e.value)
    assert api._state["call"] == call0  # a refused call draws no RNG stream


@pytest.mark.parametrize("fn", [api.backward_batch_shapes, api.backward_batch_shapes_async], ids=["blocking", "async"])
def test_shapes_are_required_and_too_many_frames(no_device, fn):
    with pytest.raises(TypeError, match="shapes"):
        fn(torch.zeros(4, S), torch.zeros(4, S), torch.zeros(4, N, dtype=torch.int64), torch.eye(4).repeat(4, 1, 1), *LOSS, *SOLVER)
    with pytest.raises(RuntimeError, match=r"shapes must hold one \(h, w\) pair per frame \(4\), found NoneType"):
        fn(torch.zeros(4, S), torch.zeros(4, S), torch.zeros(4, N, dtype=torch.int64), torch.eye(4).repeat(4, 1, 1), *LOSS, *SOLVER, shapes=None)
    B = api.MAX_BATCH + 1
    call0 = api._state["call"]
    with pytest.raises(RuntimeError, match="hypAssignment holds %d frames, at most %d per call" % (B, api.MAX_BATCH)):
        fn(torch.zeros(B, 28), torch.zeros(B, 28), torch.zeros(B, 4, dtype=torch.int64), torch.eye(4).repeat(B, 1, 1), *LOSS, *SOLVER,
           shapes=[(3, 3)] * B)
    assert api._state["call"] == call0


def test_the_new_calls_extend_the_shared_shape_calls_by_keywords():
    for new, old in ((api.backward_batch_shapes, api.backward_batch), (api.backward_batch_shapes_async, api.backward_batch_async)):
        sig, was = inspect.signature(new).parameters, inspect.signature(old).parameters
        positional = [n for n, p in sig.items() if p.kind is not inspect.Parameter.KEYWORD_ONLY]
        assert positional == [n for n, p in was.items() if p.kind is not inspect.Parameter.KEYWORD_ONLY] and positional[-1] == "subSampling"
        assert sig["shapes"].kind is inspect.Parameter.KEYWORD_ONLY and sig["shapes"].default is inspect.Parameter.empty
        for name in ("experts", "poseRecords"):
            assert sig[name].kind is inspect.Parameter.KEYWORD_ONLY and sig[name].default is None
        assert "shapes" not in was and "experts" not in was  # the shared-shape calls are what they were
    for new, old in ((api.Engine.backward_batch_shapes, api.Engine.backward_batch), (api.Engine.backward_batch_shapes_async, api.Engine.backward_batch_async)):
        names, was = list(inspect.signature(new).parameters), list(inspect.signature(old).parameters)
        assert names == was[:9] + ["shapes"] + was[9:], (names, was)
    assert esac.unpack_frames is api.unpack_frames and esac.backward_batch_shapes is api.backward_batch_shapes
    assert esac.backward_batch_shapes_async is api.backward_batch_shapes_async


# ---------------------------------------------------------------- unpack_frames
def test_unpack_frames_is_the_inverse_of_pack_frames_and_returns_views():
    maps = _maps()
    packed, shapes = esac.pack_frames(maps, device="cpu")
    views = esac.unpack_frames(packed, shapes, E)
    assert len(views) == 4
    for v, m, (h, w) in zip(views, maps, shapes):
        assert tuple(v.shape) == (E, 3, h, w) and torch.equal(v, m)
    views[2][2, 2, 11, 17] = 7.0  # the last element of frame 2's dense tensor: element 3*E*h*w - 1 of its row
    assert packed[2, 3 * E * 216 - 1] == 7.0
    views[0].add_(1.0)  # writing a view writes the packed row, and nothing behind the frame's own 3*E*h*w
    assert torch.equal(packed[0, :1728].view(E, 3, 12, 16), maps[0] + 1.0) and torch.count_nonzero(packed[0, 1728:]) == 0
    again, _ = esac.pack_frames(esac.unpack_frames(packed, shapes, E), device="cpu")
    assert torch.equal(again, packed)
    # a wider row (a gradient buffer of the caller's own stride) unpacks the same way
    wide = torch.zeros(4, S + 8)
    assert [tuple(v.shape) for v in esac.unpack_frames(wide, shapes, E)] == [(E, 3) + s for s in shapes]


@pytest.mark.parametrize("packed, shapes, experts, needle", [
    (torch.zeros(4, E, 3, 12, 18), SHAPES, E, "packed must be a [B,S] tensor"),
    ([torch.zeros(4, S)], SHAPES, E, "packed must be a [B,S] tensor, found list"),
    (torch.zeros(4, S), SHAPES[:3], E, "shapes must hold one (h, w) pair per frame (4), found 3"),
    (torch.zeros(4, S), SHAPES[:3] + [(1, 1)], E, "shapes[3] = 1x1 is no legal grid"),
    (torch.zeros(4, S), SHAPES, 4, "packed [B,1944] is too short for E = 4"),
    (torch.zeros(4, S), SHAPES, 0, "E must be a positive int"),
    (torch.zeros(4, S), SHAPES, 3.0, "E must be a positive int"),
])
def test_unpack_frames_errors(no_device, packed, shapes, experts, needle):
    with pytest.raises(RuntimeError) as e:
        esac.unpack_frames(packed, shapes, experts)
    assert str(e.value).startswith("esac.unpack_frames:") and needle in str(e.value), str(e.value)


# ---------------------------------------------------------------- harness.train_batch, the list form
def test_train_batch_list_errors_touch_no_device(no_device):
    def net(x):
        raise AssertionError("a network ran")
    with pytest.raises(RuntimeError, match="train_batch: images must be .* non-empty list"):
        harness.train_batch([], None, net, [net], 525.0)
    with pytest.raises(RuntimeError, match="train_batch: images must be .* non-empty list"):
        harness.train_batch([torch.zeros(2, 3, 96, 128), torch.zeros(1, 3, 128, 96)], None, net, [net], 525.0)
    mixed = [torch.zeros(1, 3, 96, 128), torch.zeros(3, 128, 96)]
    with pytest.raises(RuntimeError, match=r"focal_lengths must hold one value per image \(2\), found 3"):
        harness.train_batch(mixed, None, net, [net], [525.0] * 3)
    with pytest.raises(RuntimeError, match=r"shifts must hold one pair per image \(2\), found 1"):
        harness.train_batch(mixed, None, net, [net], 525.0, shifts=[(0, 0)])


def test_train_batch_list_reaches_the_ragged_solver_with_one_packed_call(monkeypatch):
    """The list form up to the solver, on the CPU: the networks run once per image-size group, the predictions travel in ONE packed
    buffer with every frame's own grid, principal point, focal length and shift, and the gradients that come back in the packed
    buffer reach every network through ONE autograd.backward."""
    sizes = [(96, 128), (128, 96), (96, 144), (96, 128)]  # sub 8: 12x16, 16x12, 12x18, 12x16
    images = [torch.randn(1, 3, h, w) for h, w in sizes]
    calls, seen = [], {}

    class Net(torch.nn.Module):
        def __init__(self, k):
            super().__init__()
            self.k, self.w = k, torch.nn.Parameter(torch.tensor(1.0 + k))

        def forward(self, x):
            calls.append((self.k, tuple(x.shape)))
            return torch.nn.functional.avg_pool2d(x, 8, ceil_mode=True) * self.w

    class Gate(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.b = torch.nn.Parameter(torch.zeros(2))

        def forward(self, x):
            calls.append(("g", tuple(x.shape)))
            return torch.log_softmax(self.b + x.mean(dim=(1, 2, 3)).unsqueeze(1) * torch.tensor([1.0, -1.0]), dim=1)

    def solver(sc, grads, ha, gt, *rest, poseRecords=None, shapes=None, experts=None):
        seen.update(sc=sc.clone(), shapes=shapes, experts=experts, cam=rest[3:8], ha=ha)
        for b, v in enumerate(api.unpack_frames(grads, shapes, experts)):
            v += float(b + 1)
        return [float(b) for b in range(4)]

    monkeypatch.setattr(api, "backward_batch_shapes", solver)
    nets, gate = [Net(0), Net(1)], Gate()
    e_hyps = torch.tensor([[0] * 8, [1] * 8, [0, 1] * 4, [1] * 8])
    out = harness.train_batch(images, torch.eye(4).repeat(4, 1, 1), gate, nets, [500.0, 510.0, 520.0, 530.0], subsample=8,
                              shifts=[(0, 0), (1, -1), (2, 0), (-3, 3)], e_hyps=e_hyps)
    shapes = [(12, 16), (16, 12), (12, 18), (12, 16)]
    assert seen["shapes"] == shapes == out["shapes"] and seen["experts"] == 2 and out["losses"] == [0.0, 1.0, 2.0, 3.0]
    assert seen["cam"] == ([0, 1, 2, -3], [0, -1, 0, 3], [500.0, 510.0, 520.0, 530.0], [64.0, 48.0, 72.0, 64.0], [48.0, 64.0, 48.0, 48.0])
    # one gating and at most one expert pass per image-size group (3 groups); expert 0 is inactive in the 128x96 group
    assert sorted(c for c in calls if c[0] == "g") == sorted(("g", (n, 3, h, w)) for n, h, w in ((2, 96, 128), (1, 128, 96), (1, 96, 144)))
    assert sorted(c for c in calls if c[0] != "g") == sorted([(0, (2, 3, 96, 128)), (1, (2, 3, 96, 128)), (1, (1, 3, 128, 96)),
                                                              (0, (1, 3, 96, 144)), (1, (1, 3, 96, 144))])
    assert tuple(seen["sc"].shape) == (4, api.packed_stride(2, shapes))
    views = api.unpack_frames(seen["sc"], shapes, 2)
    padded = torch.nn.functional.pad(images[3], (-3, 3, 3, -3))
    assert torch.allclose(views[3][1], torch.nn.functional.avg_pool2d(padded, 8, ceil_mode=True)[0] * 2.0)
    assert torch.count_nonzero(views[1][0]) == 0  # the inactive expert's rows stay zero
    # d/dw of sum(grad * avg_pool(x) * w): frame b's gradient is b + 1 everywhere
    want = [sum((b + 1) * torch.nn.functional.avg_pool2d(torch.nn.functional.pad(images[b], (px, -px, py, -py)), 8, ceil_mode=True).sum()
                for b, (px, py) in zip(frames, pads)) for frames, pads in (((0, 2, 3), [(0, 0), (2, 0), (-3, 3)]),
                                                                          ((0, 1, 2, 3), [(0, 0), (1, -1), (2, 0), (-3, 3)]))]
    assert torch.allclose(nets[0].w.grad, want[0], rtol=1e-4) and torch.allclose(nets[1].w.grad, want[1], rtol=1e-4)
    assert gate.b.grad is not None and tuple(out["gating_log_probs"].shape) == (4, 2)
    assert torch.equal(out["e_hist"], torch.tensor([[8.0, 0.0], [0.0, 8.0], [4.0, 4.0], [0.0, 8.0]]))


def test_train_batch_list_of_one_size_is_the_tensor_form(monkeypatch):
    images = [torch.randn(1, 3, 96, 128) for _ in range(3)]
    got = {}

    def solver(sc, grads, *rest, **kw):
        got["sc"], got["kw"] = tuple(sc.shape), kw
        return [0.0, 0.0, 0.0]

    monkeypatch.setattr(api, "backward_batch", solver)
    net = lambda x: torch.nn.functional.avg_pool2d(x, 8)  # noqa: E731
    gate = lambda x: torch.log_softmax(torch.zeros(x.size(0), 1), dim=1)  # noqa: E731
    out = harness.train_batch(images, torch.eye(4).repeat(3, 1, 1), gate, [net], 525.0, shifts=[(0, 0)] * 3,
                              e_hyps=torch.zeros(3, 8, dtype=torch.int64))
    assert got["sc"] == (3, 1, 3, 12, 16) and "shapes" not in got["kw"] and "shapes" not in out


# ---------------------------------------------------------------- the symbols
def test_header_declares_the_symbols_and_the_binding_names_them():
    hdr = open(os.path.join(ROOT, "include", "esac_hip.h")).read()

    def params(name):
        m = re.search(r"int %s\(([^;]*)\);" % name, hdr)
        assert m, "include/esac_hip.h does not declare %s" % name
        return [a.strip() for a in re.sub(r"\s+", " ", m.group(1)).split(",")]
    assert params("esac_hip_backward_batch_shapes") == params("esac_hip_backward_batch_cams")
    assert params("esac_hip_backward_batch_dev_shapes") == params("esac_hip_backward_batch_dev")
    assert "#define ESAC_HIP_ABI_VERSION 6" in hdr and api.ABI_VERSION == 6
    for name in ("esac_hip_backward_batch_shapes", "esac_hip_backward_batch_dev_shapes"):
        assert name in api.ABI_SYMBOLS
    assert len(set(api.ABI_SYMBOLS)) == len(api.ABI_SYMBOLS)


def test_library_exports_and_binds_the_symbols():
    from esac_amd import build
    if not os.path.exists(build.LIB_PATH):
        build.build_hip()
    lib = api.load_library()
    cams = api.make_cams([0], [0], [525.0], [1.0], [1.0])
    for name, like in (("esac_hip_backward_batch_shapes", "esac_hip_backward_batch_cams"),
                       ("esac_hip_backward_batch_dev_shapes", "esac_hip_backward_batch_dev")):
        fn = getattr(lib, name)
        assert len(fn.argtypes) == 15 and fn.argtypes == getattr(lib, like).argtypes
        # the checks in front of the device need none: a null context, then (with everything else in place) a null table
        assert fn(None, 2, None, 0, None, 0, None, None, cams.ctypes.data, 1.0, 100.0, 100.0, None, None, None) == -1
        assert b"null context" in lib.esac_hip_last_error()
