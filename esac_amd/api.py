"""Host-side mirror of the reference's `esac` extension interface over the C ABI.

Reference: `PYBIND11_MODULE(..)  m.def("forward", &esac_forward); m.def("backward", &esac_backward)`
(code/esac/esac.cpp:513-516); call site test_esac.py:192-205.  `forward` below keeps
the positional signature, the in-place `outPose` write and the Python-int return
value; every failure the reference surfaces as a pybind11 `RuntimeError`
(c10::Error from `accessor<>()`, cv::Exception) is a `RuntimeError` here too.

The compute runs ONLY in libesac_hip.so (hand-written HIP for gfx950).  There is
no CPU fallback: without the library or without a HIP device the call raises.
torch is used for device memory, streams and (in distributed.py) RCCL -- never
for the arithmetic of this path.
"""
import ctypes as C
import os
import threading

import numpy as np
import torch

from . import build as _build

# ---------------------------------------------------------------- C ABI binding
RES_SCORE, RES_HYP, RES_EXPERT, RES_RVEC, RES_TVEC, RES_POSE = 0, 1, 2, 3, 6, 9
RES_REF_STEPS, RES_INLIERS, RES_PROB, RES_ENTROPY, RES_CONTENDERS, RES_LM_ITERS, RES_DOUBLES = 25, 26, 27, 28, 29, 30, 32
BUF_HYPS, BUF_SAMPLE_XY, BUF_TRIES, BUF_SCORES, BUF_RESULT = 0, 1, 2, 3, 4
BUF_INLIER_MAP, BUF_INLIER_COUNTS, BUF_WINNER_ERRS, BUF_EXACT_FLAGS, BUF_CYCLES = 5, 6, 7, 8, 9
BUF_BWD_PROBS, BUF_BWD_LOSSES, BUF_BWD_REF_HYPS, BUF_BWD_SCORE_GRADS, BUF_BWD_SLOTS, BUF_BWD_SLOT_INFO, BUF_BWD_DLOSS = \
    10, 11, 12, 13, 14, 15, 16
BUF_BWD_PATH1, BUF_BWD_PATH2 = 17, 18
BUF_REFINE_INFO = 19
BUF_BWD_TEAM_INFO = 20
BUF_SPEC_INFO = 21
BUF_SPEC_FLAGS = 22
BUF_BWD_MAPS = 23
REFINE_TEAM_MAX, REFINE_TEAM_EIGHT, REFINE_TEAM_AUTO = 32, 8, -1
REFINE_TEAM_DEFAULT = REFINE_TEAM_AUTO  # what a fresh context does: 8 members, or the smallest team <= 16 that lowers the cells per lane
MAX_REF_STEPS = 100
BWD_MAX_SLOTS = 1000
MAX_BATCH = 1024
RES_VALID = 31  # device records only: 1 a record, 3 the refinement team timed out, 0 none
# one row of esac_hip_eval_batch (include/esac_hip.h: ESAC_EVAL_*)
EVAL_ROT_DEG, EVAL_TRANS_CM, EVAL_POSE_OK, EVAL_CLASS_OK, EVAL_QUAT, EVAL_INV_T, EVAL_EXPERT, EVAL_HYP, EVAL_STATUS = 0, 1, 2, 3, 4, 8, 11, 12, 13
EVAL_DOUBLES = 16
# one row of esac_hip_verify_batch (include/esac_hip.h: ESAC_VERIFY_*)
VERIFY_SCORE, VERIFY_N, VERIFY_SSE, VERIFY_SIGMA2, VERIFY_STATUS, VERIFY_A, VERIFY_C = 0, 1, 2, 3, 4, 6, 28
VERIFY_DOUBLES = 64
VERIFY_MAX_POSES = 1024
VERIFY_OK, VERIFY_FEW, VERIFY_PINV, VERIFY_BAD_POSE, VERIFY_BAD_EXPERT = 0, 1, 2, 3, 4
VERIFY_POSE_RT, VERIFY_POSE_4X4 = 0, 1

ABI_SYMBOLS = [
    "esac_hip_abi_version", "esac_hip_last_error", "esac_hip_device_count", "esac_hip_create", "esac_hip_destroy",
    "esac_hip_forward", "esac_hip_sample", "esac_hip_score", "esac_hip_select", "esac_hip_refine",
    "esac_hip_score_exact", "esac_hip_read", "esac_hip_write_hyps", "esac_hip_phase_ms", "esac_hip_set_timing",
    "esac_hip_score_span_ms", "esac_hip_forward_batch", "esac_hip_backward", "esac_hip_set_debug", "esac_hip_check",
    "esac_hip_pick_record", "esac_hip_time_stages", "esac_hip_shard_balanced", "esac_hip_set_wait",
    "esac_hip_set_refine_team", "esac_hip_host_turn",
    "esac_hip_comm_unique_id", "esac_hip_comm_init", "esac_hip_comm_destroy", "esac_hip_allreduce_sum", "esac_hip_comm_info",
    "esac_hip_host_turn_mean", "esac_hip_backward_batch",
    "esac_hip_forward_batch_cams", "esac_hip_backward_batch_cams",
    "esac_hip_backward_batch_dev",  # additive: the ABI version stays
    "esac_hip_eval_batch",  # additive too
    "esac_hip_set_bwd_pose_records",  # additive too
    "esac_hip_forward_batch_shapes",  # additive too
    "esac_hip_backward_batch_shapes", "esac_hip_backward_batch_dev_shapes",  # additive too
    "esac_hip_set_refine_route",  # additive too
    "esac_hip_set_front_route", "esac_hip_front_route_taken", "esac_hip_read_rotations",  # additive too
    "esac_hip_verify_batch",  # additive too
]
COMM_ID_BYTES = 128
ABI_VERSION = 6
FLAG_EXACT_SCORES, FLAG_SCORE_TILED, FLAG_SCORE_STREAM, FLAG_PACK_MAPS, FLAG_EXACT_SAMPLING, FLAG_SCORES_BY_INDEX = 1, 2, 4, 8, 16, 32
FLAG_AUTO_EXACT = 64
FLAG_REFINE_SOLO = 128
FLAG_STRICT_REFERENCE = 256  # the reference's rule in P3P alignment, NaN scores and the LM trial test (include/esac_hip.h)
FLAG_STRICT_TRAINING = 512  # the training path's strict mode: esac_hip_backward* only (include/esac_hip.h)
WAIT_SPIN, WAIT_YIELD, WAIT_BLOCK = 0, 1, 2
DEBUG_ERROR_IMAGE, DEBUG_COOP_STALL, DEBUG_TEAM_SPREAD, DEBUG_NO_SPECULATION, DEBUG_SPEC_SECOND_BEST, DEBUG_SPEC_LOSE_CHAIN = 1, 2, 4, 8, 16, 32


class Params(C.Structure):
    """struct esac_hip_params (include/esac_hip.h)."""
    _fields_ = [
        ("E", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("N", C.c_int32),
        ("shift_x", C.c_int32), ("shift_y", C.c_int32),
        ("focal", C.c_float), ("ppx", C.c_float), ("ppy", C.c_float),
        ("inlier_thresh", C.c_float), ("inlier_alpha", C.c_float), ("inlier_beta", C.c_float),
        ("max_reproj", C.c_float), ("sub_sampling", C.c_int32),
        ("seed", C.c_uint64), ("call", C.c_uint64),
        ("max_tries", C.c_int32), ("max_ref_steps", C.c_int32), ("hyp_offset", C.c_int32),
        ("rescore_margin", C.c_float),
        ("d_hyp_index", C.c_void_p),
        ("flags", C.c_int32),
        ("expert_base", C.c_int32),
    ]


class FrameCam(C.Structure):
    """struct esac_hip_frame_cam (include/esac_hip.h): one frame's camera in a batch with per-frame cameras, 32 bytes."""
    _fields_ = [
        ("shift_x", C.c_int32), ("shift_y", C.c_int32),
        ("focal", C.c_float), ("ppx", C.c_float), ("ppy", C.c_float),
        ("reserved", C.c_int32 * 3),
    ]


CAM_DTYPE = np.dtype([("shift_x", np.int32), ("shift_y", np.int32), ("focal", np.float32), ("ppx", np.float32),
                      ("ppy", np.float32), ("reserved", np.int32, (3,))])


def make_cams(shift_x, shift_y, focal, ppx, ppy):
    """A table of B esac_hip_frame_cam records (numpy structured array, CAM_DTYPE) from five length-B sequences."""
    B = len(shift_x)
    cams = np.zeros(B, CAM_DTYPE)
    cams["shift_x"], cams["shift_y"] = np.asarray(shift_x, np.int64), np.asarray(shift_y, np.int64)
    cams["focal"], cams["ppx"], cams["ppy"] = np.asarray(focal, np.float64), np.asarray(ppx, np.float64), np.asarray(ppy, np.float64)
    return cams


def _cams_arg(cams, B, who):
    """`cams` of Engine.forward_batch / backward_batch as a contiguous CAM_DTYPE array of B records (kept alive by the caller)."""
    if isinstance(cams, np.ndarray) and cams.dtype == CAM_DTYPE:
        arr = np.ascontiguousarray(cams)
    elif isinstance(cams, (list, tuple)) and all(isinstance(c, FrameCam) for c in cams):
        arr = make_cams([c.shift_x for c in cams], [c.shift_y for c in cams], [c.focal for c in cams],
                        [c.ppx for c in cams], [c.ppy for c in cams])
    else:
        raise RuntimeError("%s: cams must be a numpy array of dtype api.CAM_DTYPE (api.make_cams) or a list of api.FrameCam" % who)
    if arr.ndim != 1 or arr.shape[0] != B:
        raise RuntimeError("%s: cams must hold one record per frame (%d), found shape %s" % (who, B, tuple(arr.shape)))
    return arr


def _shapes_arg(who, shapes, B):
    """`shapes` of a ragged batch as a list of B (h, w) int pairs.  Raises RuntimeError naming the argument; touches no device."""
    if isinstance(shapes, (torch.Tensor, np.ndarray)):
        shapes = shapes.tolist()
    if not isinstance(shapes, (list, tuple)) or len(shapes) != B:
        raise RuntimeError("%s: shapes must hold one (h, w) pair per frame (%d), found %s"
                           % (who, B, "%d" % len(shapes) if isinstance(shapes, (list, tuple)) else type(shapes).__name__))
    out = []
    for b, s in enumerate(shapes):
        try:
            h, w = s
            ok = int(h) == h and int(w) == w
        except (TypeError, ValueError):
            ok = False
        if not ok:
            raise RuntimeError("%s: shapes[%d] must be a pair of integers (h, w), found %r" % (who, b, s))
        h, w = int(h), int(w)
        # the grid rule of a single call (call_policy.hpp: check_grid)
        if h < 3 or w < 3 or (h - 1) * (w - 1) < 4 or h > 65535 or w > 65535:
            raise RuntimeError("%s: shapes[%d] = %dx%d is no legal grid (at least 3x3 with (h-1)(w-1) >= 4, at most 65535 rows / columns)"
                               % (who, b, h, w))
        out.append((h, w))
    return out


def capacity_shape(shapes):
    """The (H, W) a ragged batch's parameter block carries: the grid of the frame with the most cells (only H*W matters: it is
    the cell count every per-frame buffer and launch is sized for)."""
    return max(shapes, key=lambda s: s[0] * s[1])


def packed_stride(E, shapes):
    """Floats per frame slot of a packed ragged batch: 3*E*max(h*w), rounded up to a multiple of 4 (16-byte aligned slots)."""
    return (3 * int(E) * max(h * w for h, w in shapes) + 3) // 4 * 4


def _frame_table(who, params, cams, shapes, B):
    """The per-frame table whose pointer goes to the library, and the call's ragged flag: (None, 0) without cams and shapes;
    (the B records of cams, 0) with cams alone -- not copied: the library copies the table before it returns --; with shapes
    (a ragged call) a table of this call's own, flag 1: a COPY of cams (the caller's table keeps its padding), or the camera
    of `params` broadcast to B records, with frame b's (h, w) in reserved[b, :2].  shapes: what _shapes_arg returned -- every
    caller has judged them where its own order of checks wants it (a second pass costs 10 us per 32 frames).  Raises
    RuntimeError naming cams."""
    if shapes is None:
        return (None if cams is None else _cams_arg(cams, B, who)), 0
    if cams is None:
        table = make_cams([params.shift_x] * B, [params.shift_y] * B, [params.focal] * B, [params.ppx] * B, [params.ppy] * B)
    else:
        table = _cams_arg(cams, B, who).copy()
    table["reserved"][:, :2] = np.asarray(shapes, np.int32)
    return table, 1


def _frame_stride(sc):
    """Floats from one frame's maps to the next: the row stride of [B,E,3,H,W] or of a packed [B,S]; 0: one [E,3,H,W] shared by all."""
    return int(sc.stride(0)) if sc.dim() in (5, 2) else 0


def _ragged_maps(who, maps):
    """A list of B float32 [E,3,h_b,w_b] tensors with one E.  Returns (E, shapes); RuntimeError naming sceneCoordinates otherwise."""
    if not isinstance(maps, (list, tuple)) or len(maps) == 0:
        raise RuntimeError("%s: sceneCoordinates must be a non-empty list of float32 [E,3,h,w] tensors" % who)
    E = None
    for b, m in enumerate(maps):
        if not isinstance(m, torch.Tensor):
            raise RuntimeError("%s: sceneCoordinates[%d] must be a torch.Tensor" % (who, b))
        if m.dtype != torch.float32:
            raise RuntimeError("%s: expected scalar type torch.float32 for sceneCoordinates[%d] but found %s" % (who, b, m.dtype))
        if m.dim() != 4 or m.size(1) != 3:
            raise RuntimeError("%s: sceneCoordinates[%d] must be [E,3,h,w], found %s" % (who, b, list(m.shape)))
        if E is None:
            E = int(m.size(0))
        elif int(m.size(0)) != E:
            raise RuntimeError("%s: sceneCoordinates[%d] holds %d experts, sceneCoordinates[0] holds %d" % (who, b, m.size(0), E))
    return E, [(int(m.size(2)), int(m.size(3))) for m in maps]


def pack_frames(maps, device=None):
    """Packs frames that differ in image size for `forward_batch(shapes=...)`: maps = a list of B float32 [E,3,h_b,w_b] tensors
    (host or device).  Returns (packed, shapes): packed float32 [B,S] on the device with frame b's maps DENSE in packed[b,
    :3*E*h_b*w_b] (the rest of the row is zero and never read), S = 3*E*max(h_b*w_b) rounded up to a multiple of 4; shapes =
    [(h_b, w_b), ...].  device: where packed lives (default: the first device tensor's device, else the current GPU)."""
    who = "esac.pack_frames"
    E, shapes = _ragged_maps(who, maps)
    shapes = _shapes_arg(who, shapes, len(maps))
    if device is None:
        on_dev = [m.device for m in maps if m.is_cuda]
        device = on_dev[0] if on_dev else engine(None).device
    packed = torch.zeros(len(maps), packed_stride(E, shapes), dtype=torch.float32, device=device)
    for b, m in enumerate(maps):
        packed[b, :m.numel()].copy_(m.reshape(-1), non_blocking=True)
    return packed, shapes


def unpack_frames(packed, shapes, E):
    """The inverse of `pack_frames`: the list of B [E,3,h_b,w_b] VIEWS of a packed [B,S] tensor (no copy: writing a view writes
    the packed row) -- the maps of a packed batch, or the gradients `backward_batch_shapes` accumulated into a packed
    tensor, handed back to autograd per frame.  Raises RuntimeError naming the argument; touches no device."""
    who = "esac.unpack_frames"
    if not isinstance(packed, torch.Tensor) or packed.dim() != 2:
        raise RuntimeError("%s: packed must be a [B,S] tensor, found %s"
                           % (who, list(packed.shape) if isinstance(packed, torch.Tensor) else type(packed).__name__))
    if not isinstance(E, int) or isinstance(E, bool) or E < 1:
        raise RuntimeError("%s: E must be a positive int, found %r" % (who, E))
    shapes = _shapes_arg(who, shapes, int(packed.size(0)))
    S = int(packed.size(1))
    if 3 * E * max(h * w for h, w in shapes) > S:
        raise RuntimeError("%s: packed [B,%d] is too short for E = %d expert(s) on the largest grid of shapes (%d cells)"
                           % (who, S, E, max(h * w for h, w in shapes)))
    return [packed[b, :3 * E * h * w].view(E, 3, h, w) for b, (h, w) in enumerate(shapes)]


_lib = None
_lib_lock = threading.Lock()


def load_library():
    """dlopen libesac_hip.so (built in-tree by esac_amd.build / __graft_entry__.build)."""
    global _lib
    with _lib_lock:
        if _lib is not None:
            return _lib
        path = os.environ.get("ESAC_HIP_LIB", _build.LIB_PATH)  # override: A/B builds of the same ABI
        if not os.path.exists(path):
            raise RuntimeError(
                "esac: HIP extension %s is missing -- run `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950). There is no CPU fallback for this path." % path)
        lib = C.CDLL(path)
        vp, i32, u64 = C.c_void_p, C.c_int, C.c_uint64
        pp = C.POINTER(Params)
        lib.esac_hip_abi_version.restype = i32
        lib.esac_hip_last_error.restype = C.c_char_p
        lib.esac_hip_device_count.restype = i32
        lib.esac_hip_create.argtypes = [C.POINTER(vp), i32]
        lib.esac_hip_destroy.argtypes = [vp]
        lib.esac_hip_forward.argtypes = [vp, vp, vp, pp, vp, vp, vp, vp]
        lib.esac_hip_forward_batch.argtypes = [vp, i32, vp, C.c_int64, vp, pp, vp, vp, vp, vp]
        lib.esac_hip_forward_batch_cams.argtypes = [vp, i32, vp, C.c_int64, vp, pp, vp, vp, vp, vp, vp]
        lib.esac_hip_forward_batch_shapes.argtypes = [vp, i32, vp, C.c_int64, vp, pp, vp, vp, vp, vp, vp]
        for name in ("esac_hip_sample", "esac_hip_score", "esac_hip_select", "esac_hip_refine", "esac_hip_score_exact"):
            getattr(lib, name).argtypes = [vp, vp, vp, pp, vp]
        lib.esac_hip_backward.argtypes = [vp, vp, vp, vp, vp, C.c_float, C.c_float, C.c_float, pp, vp, vp]
        lib.esac_hip_backward_batch.argtypes = [vp, i32, vp, C.c_int64, vp, C.c_int64, vp, vp, C.c_float, C.c_float, C.c_float,
                                                pp, vp, vp]
        lib.esac_hip_backward_batch_cams.argtypes = [vp, i32, vp, C.c_int64, vp, C.c_int64, vp, vp, vp, C.c_float, C.c_float,
                                                     C.c_float, pp, vp, vp]
        lib.esac_hip_backward_batch_dev.argtypes = [vp, i32, vp, C.c_int64, vp, C.c_int64, vp, vp, vp, C.c_float, C.c_float,
                                                    C.c_float, pp, vp, vp]
        lib.esac_hip_backward_batch_shapes.argtypes = lib.esac_hip_backward_batch_cams.argtypes
        lib.esac_hip_backward_batch_dev_shapes.argtypes = lib.esac_hip_backward_batch_dev.argtypes
        lib.esac_hip_eval_batch.argtypes = [vp, i32, vp, vp, vp, C.c_float, C.c_float, vp, vp]
        lib.esac_hip_verify_batch.argtypes = [vp, i32, i32, vp, C.c_int64, vp, i32, vp, pp, vp, i32, vp, vp]
        lib.esac_hip_set_bwd_pose_records.argtypes = [vp, vp, i32]
        lib.esac_hip_read.argtypes = [vp, i32, vp, C.c_size_t]
        lib.esac_hip_write_hyps.argtypes = [vp, vp, i32]
        lib.esac_hip_phase_ms.argtypes = [vp, vp]
        lib.esac_hip_set_timing.argtypes = [vp, i32]
        lib.esac_hip_set_debug.argtypes = [vp, i32]
        lib.esac_hip_score_span_ms.argtypes = [vp, vp, vp]
        lib.esac_hip_check.argtypes = [vp]
        lib.esac_hip_pick_record.argtypes = [vp, vp, i32, vp, vp, vp, i32]
        lib.esac_hip_time_stages.argtypes = [vp, vp, vp, pp, vp, i32, vp]
        lib.esac_hip_shard_balanced.argtypes = [vp, vp, i32, i32, i32, i32, i32, vp, vp, vp, vp]
        lib.esac_hip_set_wait.argtypes = [vp, i32]
        lib.esac_hip_set_refine_team.argtypes = [vp, i32]
        lib.esac_hip_set_refine_route.argtypes = [vp, i32]
        lib.esac_hip_set_front_route.argtypes = [vp, i32]
        lib.esac_hip_front_route_taken.argtypes = [vp]
        lib.esac_hip_read_rotations.argtypes = [vp, vp, i32]
        lib.esac_hip_host_turn.argtypes = [vp, vp]
        lib.esac_hip_host_turn_mean.argtypes = [vp, vp, i32]
        lib.esac_hip_comm_unique_id.argtypes = [vp, C.c_size_t]
        lib.esac_hip_comm_init.argtypes = [vp, i32, i32, vp, C.c_size_t]
        lib.esac_hip_comm_destroy.argtypes = [vp]
        lib.esac_hip_allreduce_sum.argtypes = [vp, vp, C.c_size_t, vp]
        lib.esac_hip_comm_info.argtypes = [vp, vp]
        for name in ABI_SYMBOLS:
            if name not in ("esac_hip_last_error",):
                getattr(lib, name).restype = i32
        lib.esac_hip_last_error.restype = C.c_char_p
        if lib.esac_hip_abi_version() != ABI_VERSION:
            raise RuntimeError("esac: libesac_hip.so ABI version mismatch")
        _lib = lib
        return lib


def _check(rc, lib):
    if rc != 0:
        raise RuntimeError("esac (HIP): %s [status %d]" % (lib.esac_hip_last_error().decode(), rc))


def _check_pose_records(who, name, records, B, device_only, device=None):
    """The pose-record argument of a training call (esac_hip_set_bwd_pose_records): a float64 tensor [32] (B is None: a single
    call) or [B,32], filled in place.  device_only: the asynchronous call -- a contiguous device tensor; otherwise a CPU tensor
    (any strides) or a contiguous device tensor.  device: the device the call's tensors live on (None: not known yet).
    Raises RuntimeError naming the argument; touches no device."""
    if not isinstance(records, torch.Tensor):
        raise RuntimeError("%s: %s must be a torch.Tensor" % (who, name))
    if records.dtype != torch.float64:
        raise RuntimeError("%s: expected scalar type torch.float64 for %s but found %s" % (who, name, records.dtype))
    want = (RES_DOUBLES,) if B is None else (int(B), RES_DOUBLES)
    if tuple(records.shape) != want:
        raise RuntimeError("%s: %s must be %s, found %s" % (who, name, list(want), list(records.shape)))
    if records.device.type not in ("cpu", "cuda"):
        raise RuntimeError("%s: %s lives on %s: a CPU or a GPU tensor is required" % (who, name, records.device))
    if device_only and not records.is_cuda:
        raise RuntimeError("%s: %s must be a device tensor (an asynchronous call cannot copy back into host storage)" % (who, name))
    if records.is_cuda and not records.is_contiguous():
        raise RuntimeError("%s: %s must be contiguous on the device (the kernel writes it in place)" % (who, name))
    if records.is_cuda and device is not None and records.device != device:
        raise RuntimeError("%s: %s lives on %s, the call runs on %s" % (who, name, records.device, device))


class Engine:
    """One device context (esac_hip_ctx): workspaces + stage entry points for one GPU."""

    def __init__(self, device=None):
        self.lib = load_library()
        if not torch.cuda.is_available():
            raise RuntimeError("esac: no HIP device visible (torch.cuda.is_available() is False); "
                               "the MI355X path has no CPU fallback")
        self.device = torch.device("cuda", torch.cuda.current_device() if device is None else int(device))
        self.ctx = C.c_void_p()
        _check(self.lib.esac_hip_create(C.byref(self.ctx), self.device.index), self.lib)
        self._shape = None
        # the raw hipStream_t of torch's current stream: a private torch symbol (no Stream object on the per-call path)
        # with the public route as the fallback, resolved once
        self._raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)
        self._host_buf = (C.c_double * RES_DOUBLES)()  # host record of a blocking forward call
        self._host_addr = C.addressof(self._host_buf)
        self._host_np = np.frombuffer(self._host_buf, dtype=np.float64)
        self._comm = None  # (nranks, rank) once comm_init has run
        self._comm_key = None  # the process group (its ranks) the communicator mirrors (distributed.native_comm)
        self._pose_arm = None  # arm_pose_records: the record tensor of the next training call

    def _call(self, fn, *args):
        """One C-ABI call with this engine's device current (the library calls hipSetDevice itself; the context
        manager is only needed -- and only paid for -- when torch's current device is another one)."""
        if torch.cuda.current_device() == self.device.index:
            _check(fn(self.ctx, *args), self.lib)
        else:
            with torch.cuda.device(self.device):
                _check(fn(self.ctx, *args), self.lib)

    def __del__(self):
        try:
            if getattr(self, "ctx", None):
                self.lib.esac_hip_destroy(self.ctx)
                self.ctx = None
        except Exception:
            pass

    # -- helpers
    def _stream(self):
        # the raw hipStream_t of torch's current stream on this device
        if self._raw_stream is not None:
            return self._raw_stream(self.device.index)
        return torch.cuda.current_stream(self.device).cuda_stream

    def make_params(self, E, H, W, N, shift_x=0, shift_y=0, focal=525.0, ppx=320.0, ppy=240.0, inlier_thresh=10.0,
                    inlier_alpha=100.0, inlier_beta=0.5, max_reproj=100.0, sub_sampling=8, seed=1305, call=0,
                    max_tries=0, max_ref_steps=-1, hyp_offset=0, rescore_margin=0.0, exact_scores=False, score_shape="auto", pack_maps=False,
                    exact_sampling=False, scores_by_index=False, expert_base=0, refine_solo=False, strict_reference=False,
                    strict_training=False):
        if strict_training and (strict_reference or exact_scores == "auto" or score_shape != "auto"):
            # strict_training is the training path's flag (esac_hip_backward*), strict_reference the forward path's: never both
            raise ValueError("strict_training cannot be combined with strict_reference, exact_scores='auto' or score_shape=%r" % (score_shape,))
        if strict_reference and (exact_scores == "auto" or score_shape != "auto"):
            # (what the C ABI answers with -4: strict mode scores every hypothesis in reference arithmetic)
            raise ValueError("strict_reference cannot be combined with exact_scores='auto' or score_shape=%r" % (score_shape,))
        p = Params()
        p.E, p.H, p.W, p.N = int(E), int(H), int(W), int(N)
        p.shift_x, p.shift_y = int(shift_x), int(shift_y)
        p.focal, p.ppx, p.ppy = float(focal), float(ppx), float(ppy)
        p.inlier_thresh, p.inlier_alpha, p.inlier_beta = float(inlier_thresh), float(inlier_alpha), float(inlier_beta)
        p.max_reproj, p.sub_sampling = float(max_reproj), int(sub_sampling)
        p.seed, p.call = int(seed) & (2**64 - 1), int(call) & (2**64 - 1)
        p.max_tries, p.max_ref_steps, p.hyp_offset = int(max_tries), int(max_ref_steps), int(hyp_offset)
        p.rescore_margin = float(rescore_margin)
        p.d_hyp_index = None
        # exact_scores: True / False, or "auto" = the guaranteed routes where they are free (ESAC_FLAG_AUTO_EXACT: what esac.forward asks for)
        p.flags = (FLAG_AUTO_EXACT if exact_scores == "auto" else FLAG_EXACT_SCORES if exact_scores else 0) | \
            {"auto": 0, "tiled": FLAG_SCORE_TILED, "stream": FLAG_SCORE_STREAM}[score_shape] | \
            (FLAG_PACK_MAPS if pack_maps else 0) | (FLAG_EXACT_SAMPLING if exact_sampling else 0) | (FLAG_SCORES_BY_INDEX if scores_by_index else 0) | \
            (FLAG_REFINE_SOLO if refine_solo else 0)
        if strict_reference:  # implies the two guaranteed routes
            p.flags |= FLAG_STRICT_REFERENCE | FLAG_EXACT_SCORES | FLAG_EXACT_SAMPLING
        if strict_training:  # (the library implies the two routes itself; set here so that the flag word says what runs)
            p.flags |= FLAG_STRICT_TRAINING | FLAG_EXACT_SCORES | FLAG_EXACT_SAMPLING
        p.expert_base = int(expert_base)
        self._shape = (int(N), int(H), int(W))
        return p

    def set_hyp_index(self, params, index_tensor):
        """Global hypothesis indices (device int32 [N]) for shards that are not a contiguous range."""
        assert index_tensor.is_cuda and index_tensor.dtype == torch.int32 and index_tensor.is_contiguous()
        params.d_hyp_index = index_tensor.data_ptr()
        self._keep_idx = index_tensor

    def _dev_inputs(self, scene_coords, hyp_assign):
        sc = scene_coords if scene_coords.is_cuda else scene_coords.to(self.device, non_blocking=True)
        ha = hyp_assign if hyp_assign.is_cuda else hyp_assign.to(self.device, non_blocking=True)
        # accessor<> honours strides (incl. the stride-0 expand() of test_esac.py:171-173); the kernels want dense
        return (sc if sc.is_contiguous() else sc.contiguous()), (ha if ha.is_contiguous() else ha.contiguous())

    def _on_device(self, t):
        """`t` dense on a device: as it is when it lives on one, else uploaded to this engine's (non_blocking)."""
        return (t if t.is_cuda else t.to(self.device, non_blocking=True)).contiguous()

    # -- whole path
    def forward_device(self, scene_coords, hyp_assign, params, scores_out=None, result_out=None, want_host=True):
        """scene_coords [E,3,H,W] f32 / hyp_assign [N] i64 on this device. Returns host result (np.float64[32]) or None."""
        sc, ha = self._dev_inputs(scene_coords, hyp_assign)
        # (the library makes the context's GPU current itself: no torch device guard on this path; the host record goes
        # through one preallocated buffer whose address is known -- numpy's .ctypes costs a microsecond per call)
        rc = self.lib.esac_hip_forward(self.ctx, sc.data_ptr(), ha.data_ptr(), C.byref(params), self._stream(),
                                       scores_out.data_ptr() if scores_out is not None else None,
                                       result_out.data_ptr() if result_out is not None else None,
                                       self._host_addr if want_host else None)
        if rc != 0:
            _check(rc, self.lib)
        self._keep = (sc, ha)  # keep inputs alive until the (possibly asynchronous) kernels have run
        return self._host_np.copy() if want_host else None

    def forward_batch(self, scene_coords, hyp_assign, params, scores_out=None, result_out=None, want_host=True, cams=None, shapes=None):
        """B frames per launch set. scene_coords [B,E,3,H,W] (or [E,3,H,W] shared by all frames), hyp_assign [B,N];
        `params` describes one frame, frame b uses call + b. Returns np.float64 [B,32] (or None).
        cams: None (every frame uses the shift, focal length and principal point of `params`) or B records (make_cams):
        frame b uses cams[b] and the five fields of `params` are ignored (esac_hip_forward_batch_cams).
        shapes: None, or B (h, w) pairs -- a ragged batch (esac_hip_forward_batch_shapes): scene_coords is the packed [B,S] tensor
        of pack_frames, params.H * params.W the capacity in cells (capacity_shape), frame b's grid is shapes[b]."""
        who = "esac.forward_batch"
        sc, ha = self._on_device(scene_coords), self._on_device(hyp_assign)
        B = int(ha.shape[0])
        host = np.zeros((B, RES_DOUBLES), np.float64) if want_host else None
        outs = (scores_out.data_ptr() if scores_out is not None else None,
                result_out.data_ptr() if result_out is not None else None, host.ctypes.data if want_host else None)
        if shapes is not None:
            shapes = _shapes_arg(who, shapes, B)
            if sc.dim() != 2 or sc.shape[0] != B:
                raise RuntimeError("%s: with shapes, scene_coords must be the packed [B,S] tensor (pack_frames), found %s" % (who, list(sc.shape)))
        table, ragged = _frame_table(who, params, cams, shapes, B)
        if table is None:
            self._call(self.lib.esac_hip_forward_batch, B, sc.data_ptr(), _frame_stride(sc), ha.data_ptr(), C.byref(params), self._stream(), *outs)
        else:
            self._call(self.lib.esac_hip_forward_batch_shapes if ragged else self.lib.esac_hip_forward_batch_cams, B, sc.data_ptr(),
                       _frame_stride(sc), ha.data_ptr(), C.byref(params), table.ctypes.data, self._stream(), *outs)
        self._keep = (sc, ha)
        return host

    def arm_pose_records(self, records):
        """Arms the NEXT training call of this engine (backward_device, backward_batch, backward_batch_async) with `records`, as
        their pose_record(s) argument does -- the route for backward_batch_async, whose parameter list is fixed.  One-shot: taken
        by that call whether it runs or raises; None disarms.  Checked against that call's frames when it is made."""
        if records is not None:
            B = records.shape[0] if isinstance(records, torch.Tensor) and records.dim() == 2 else None
            _check_pose_records("Engine.arm_pose_records", "records", records, B, False, self.device)
        self._pose_arm = records

    def _take_pose_arm(self, given):
        """The records of this call: its own argument, else what arm_pose_records left (consumed either way)."""
        armed, self._pose_arm = self._pose_arm, None
        return given if given is not None else armed

    def _arm_pose_records(self, records, B):
        """Arms the next training call (esac_hip_set_bwd_pose_records) with `records` (checked by the caller: _check_pose_records)
        -- or, for a CPU tensor, with a device staging tensor the caller copies back from after the call's own wait.  Returns the
        device tensor the kernel writes."""
        dev = records if records.is_cuda else torch.empty(tuple(records.shape), dtype=torch.float64, device=self.device)
        self._call(self.lib.esac_hip_set_bwd_pose_records, dev.data_ptr(), 1 if B is None else int(B))
        return dev

    def backward_device(self, scene_coords, out_gradients, hyp_assign, gt_pose, w_rot, w_trans, loss_cut, params,
                        want_host=True, pose_record=None):
        """Training path on this device. out_gradients: float32 [E,3,H,W] on this device, contiguous, accumulated into.
        gt_pose: 16 floats (4x4 camera pose). Returns np.float64[4] = expected loss, #refined hypotheses, entropy, 0.
        pose_record: None, or a float64 tensor [32] filled in place with the forward-format record (RES_*) of the call's argmax
        hypothesis, refined (esac_hip_set_bwd_pose_records; RES_VALID 0 and a NaN pose when it holds no slot).  A device tensor
        is written in stream order; a CPU tensor needs want_host (it is copied after the call's own wait)."""
        pose_record = self._take_pose_arm(pose_record)
        if pose_record is not None:
            _check_pose_records("esac.backward", "poseRecord", pose_record, None, not want_host, self.device)
        sc, ha = self._dev_inputs(scene_coords, hyp_assign)
        if not (out_gradients.is_cuda and out_gradients.is_contiguous() and out_gradients.dtype == torch.float32
                and tuple(out_gradients.shape) == tuple(sc.shape)):
            raise RuntimeError("esac.backward: the gradient tensor must be a dense float32 device tensor shaped like sceneCoordinates")
        gt = np.ascontiguousarray(np.asarray(gt_pose, np.float32).reshape(16))
        host = np.zeros(4, np.float64) if want_host else None
        rec_dev = self._arm_pose_records(pose_record, None) if pose_record is not None else None
        # (the library makes the context's GPU current itself: no torch device guard on the call path, as in forward_device)
        rc = self.lib.esac_hip_backward(
            self.ctx, sc.data_ptr(), out_gradients.data_ptr(), ha.data_ptr(), gt.ctypes.data,
            float(w_rot), float(w_trans), float(loss_cut), C.byref(params), self._stream(),
            host.ctypes.data if want_host else None)
        if rc != 0:
            _check(rc, self.lib)
        self._keep = (sc, ha, out_gradients, rec_dev)
        if rec_dev is not None and rec_dev is not pose_record:
            pose_record.copy_(rec_dev)  # (the call has waited for its last kernel: the record is there)
        return host

    def _batch_inputs(self, who, scene_coords, out_gradients, hyp_assign):
        """The device inputs of a batched training call: dense scene coordinates and assignment on this device, the checked
        gradient tensor's batch size B and the coordinates' frame stride (0: one [E,3,H,W] shared by all frames)."""
        sc, ha = self._on_device(scene_coords), self._on_device(hyp_assign)
        B = int(ha.shape[0])
        if not (out_gradients.is_cuda and out_gradients.is_contiguous() and out_gradients.dtype == torch.float32
                and out_gradients.dim() == 5 and out_gradients.shape[0] == B and tuple(out_gradients.shape[1:]) == tuple(sc.shape[-4:])):
            raise RuntimeError("%s: the gradient tensor must be a dense float32 device tensor [B,E,3,H,W]" % who)
        return sc, ha, B, _frame_stride(sc)

    def _ragged_batch_inputs(self, who, scene_coords, out_gradients, hyp_assign, params, shapes):
        """The device inputs of a ragged training batch: the packed maps and the checked packed gradients (both [B,S'] float32 on
        this device, rows contiguous; frame b dense at the head of row b), B and the maps' frame stride.  shapes: the (h, w) pairs
        the public method has checked (_shapes_arg)."""
        sc, ha = self._on_device(scene_coords), self._on_device(hyp_assign)
        B = int(ha.shape[0])
        if sc.dim() != 2 or sc.shape[0] != B:
            raise RuntimeError("%s: with shapes, scene_coords must be the packed [B,S] tensor (pack_frames), found %s" % (who, list(sc.shape)))
        g = out_gradients
        if not (isinstance(g, torch.Tensor) and g.is_cuda and g.device == self.device and g.dtype == torch.float32 and g.dim() == 2
                and g.shape[0] == B and g.is_contiguous() and g.shape[1] >= 3 * params.E * max(h * w for h, w in shapes)):
            raise RuntimeError("%s: with shapes, the gradient tensor must be a packed float32 [B,S] tensor on this device, contiguous, "
                               "S >= 3*E*max(h*w)" % who)
        return sc, ha, B, _frame_stride(sc)

    def backward_batch(self, scene_coords, out_gradients, hyp_assign, gt_poses, w_rot, w_trans, loss_cut, params, cams=None,
                       pose_records=None):
        """Training path over B frames in one set of launches (esac_hip_backward_batch). scene_coords [B,E,3,H,W] (or [E,3,H,W]
        shared by all frames), out_gradients float32 [B,E,3,H,W] on this device, contiguous, accumulated into; hyp_assign [B,N];
        gt_poses [B,4,4]. `params` describes one frame, frame b uses call + b. Returns np.float64 [B,4] (one record per frame).
        An out-of-range device assignment raises after every frame has run; the exception's `records` holds the [B,4] records.
        cams: None or B per-frame camera records (make_cams), as in forward_batch (esac_hip_backward_batch_cams).
        pose_records: None, or a float64 tensor [B,32] (this device, contiguous; or CPU) filled in place: row b = the
        forward-format record of frame b's argmax hypothesis, as backward_device's pose_record.
        Frames that differ in image size: backward_batch_shapes."""
        return self._backward_batch(scene_coords, out_gradients, hyp_assign, gt_poses, w_rot, w_trans, loss_cut, params, cams, pose_records, None)

    def backward_batch_shapes(self, scene_coords, out_gradients, hyp_assign, gt_poses, w_rot, w_trans, loss_cut, params, shapes, cams=None,
                              pose_records=None):
        """backward_batch over a RAGGED batch (esac_hip_backward_batch_shapes): shapes = B (h, w) pairs, scene_coords the packed
        [B,S] tensor of pack_frames, out_gradients a packed float32 [B,S'] tensor of the same row layout on this device (frame b's
        [E,3,h_b,w_b] gradients dense at the head of row b: unpack_frames), params.H * params.W the capacity in cells
        (capacity_shape).  Everything else, and the return value, as backward_batch.  (A method of its own: the parameter lists
        of backward_batch and backward_batch_async are held as they are.)"""
        return self._backward_batch(scene_coords, out_gradients, hyp_assign, gt_poses, w_rot, w_trans, loss_cut, params, cams, pose_records,
                                    _shapes_arg("esac.backward_batch_shapes", shapes, int(hyp_assign.shape[0])))

    def _backward_batch(self, scene_coords, out_gradients, hyp_assign, gt_poses, w_rot, w_trans, loss_cut, params, cams, pose_records, shapes):
        pose_records = self._take_pose_arm(pose_records)
        if shapes is not None:
            who = "esac.backward_batch_shapes"
            sc, ha, B, sc_stride = self._ragged_batch_inputs(who, scene_coords, out_gradients, hyp_assign, params, shapes)
            table, ragged = _frame_table(who, params, cams, shapes, B)
        else:
            sc, ha, B, sc_stride = self._batch_inputs("esac.backward_batch", scene_coords, out_gradients, hyp_assign)
        gt = np.ascontiguousarray(np.asarray(gt_poses, np.float32).reshape(-1))
        if gt.size != 16 * B:
            raise RuntimeError("esac.backward_batch: gtPoses must hold B 4x4 poses")
        host = np.zeros((B, 4), np.float64)
        if shapes is None:  # (a shared-shape call's cams are judged behind its gtPoses, as ever)
            table, ragged = _frame_table("esac.backward_batch", params, cams, None, B)
        rec_dev = None
        if pose_records is not None:
            _check_pose_records("esac.backward_batch", "poseRecords", pose_records, B, False, self.device)
            rec_dev = self._arm_pose_records(pose_records, B)
        fn = self.lib.esac_hip_backward_batch if table is None else \
            self.lib.esac_hip_backward_batch_shapes if ragged else self.lib.esac_hip_backward_batch_cams
        rc = fn(self.ctx, B, sc.data_ptr(), sc_stride, out_gradients.data_ptr(), int(out_gradients.stride(0)), ha.data_ptr(),
                gt.ctypes.data, *(() if table is None else (table.ctypes.data,)), float(w_rot), float(w_trans), float(loss_cut),
                C.byref(params), self._stream(), host.ctypes.data)
        self._keep = (sc, ha, out_gradients, rec_dev)
        if rec_dev is not None and rec_dev is not pose_records and rc in (0, -10):  # (-10: raised after every frame has run)
            pose_records.copy_(rec_dev)
        if rc != 0:
            err = RuntimeError("esac (HIP): %s [status %d]" % (self.lib.esac_hip_last_error().decode(), rc))
            err.records = host
            raise err
        return host

    def backward_batch_async(self, scene_coords, out_gradients, hyp_assign, gt_poses, w_rot, w_trans, loss_cut, params, cams=None,
                             out=None):
        """backward_batch without the host inside the call (esac_hip_backward_batch_dev): returns once the launches are enqueued
        on torch's current stream; everything is read and written in stream order.  gt_poses: a float32 [B,4,4] tensor on this
        device (the point of the call), or a host array / tensor, uploaded with non_blocking=True on the launch stream.
        Returns the device float64 tensor [B,4] of records (`out` when given).  A singular ground-truth pose or an out-of-range
        assignment is a per-frame outcome (record[3] = 2 / 1): check() after a synchronisation raises for it.
        cams: None or B per-frame camera records (make_cams), copied before the call returns.
        Pose records: arm_pose_records(t) before the call, t a contiguous float64 tensor [B,32] on this device, written in
        stream order: row b = the forward-format record of frame b's argmax hypothesis (RES_VALID 0 and a NaN pose for a frame
        that selected nothing, a singular ground truth among them); eval_batch may be enqueued right behind the call.
        Frames that differ in image size: backward_batch_shapes_async."""
        return self._backward_batch_async(scene_coords, out_gradients, hyp_assign, gt_poses, w_rot, w_trans, loss_cut, params, cams, out, None)

    def backward_batch_shapes_async(self, scene_coords, out_gradients, hyp_assign, gt_poses, w_rot, w_trans, loss_cut, params, shapes,
                                    cams=None, out=None):
        """backward_batch_async over a RAGGED batch (esac_hip_backward_batch_dev_shapes): shapes and the packed tensors as in
        backward_batch_shapes, everything else as backward_batch_async."""
        return self._backward_batch_async(scene_coords, out_gradients, hyp_assign, gt_poses, w_rot, w_trans, loss_cut, params, cams, out,
                                          _shapes_arg("esac.backward_batch_shapes_async", shapes, int(hyp_assign.shape[0])))

    def _backward_batch_async(self, scene_coords, out_gradients, hyp_assign, gt_poses, w_rot, w_trans, loss_cut, params, cams, out, shapes):
        pose_records = self._take_pose_arm(None)
        if shapes is not None:
            who = "esac.backward_batch_shapes_async"
            sc, ha, B, sc_stride = self._ragged_batch_inputs(who, scene_coords, out_gradients, hyp_assign, params, shapes)
            table, ragged = _frame_table(who, params, cams, shapes, B)
        else:
            sc, ha, B, sc_stride = self._batch_inputs("esac.backward_batch_async", scene_coords, out_gradients, hyp_assign)
        if pose_records is not None:
            _check_pose_records("esac.backward_batch_async", "poseRecords", pose_records, B, True, self.device)
        gt = gt_poses if isinstance(gt_poses, torch.Tensor) and gt_poses.is_cuda else \
            self._upload(gt_poses if isinstance(gt_poses, torch.Tensor) else np.asarray(gt_poses, np.float32), torch.float32)
        if gt.dtype != torch.float32 or gt.numel() != 16 * B:
            raise RuntimeError("esac.backward_batch_async: gtPoses must hold B float32 4x4 poses")
        gt = gt.contiguous()
        if out is None:
            out = torch.empty((B, 4), dtype=torch.float64, device=self.device)
        elif not (out.is_cuda and out.is_contiguous() and out.dtype == torch.float64 and tuple(out.shape) == (B, 4)):
            raise RuntimeError("esac.backward_batch_async: out must be a dense float64 device tensor [B,4]")
        if shapes is None:  # (a shared-shape call's cams are judged behind gtPoses and out, as ever)
            table, ragged = _frame_table("esac.backward_batch_async", params, cams, None, B)
        if pose_records is not None:
            self._arm_pose_records(pose_records, B)
        rc = (self.lib.esac_hip_backward_batch_dev_shapes if ragged else self.lib.esac_hip_backward_batch_dev)(
            self.ctx, B, sc.data_ptr(), sc_stride, out_gradients.data_ptr(), int(out_gradients.stride(0)), ha.data_ptr(),
            gt.data_ptr(), table.ctypes.data if table is not None else None, float(w_rot), float(w_trans), float(loss_cut),
            C.byref(params), self._stream(), out.data_ptr())
        if rc != 0:
            _check(rc, self.lib)
        self._keep = (sc, ha, out_gradients, gt, out, pose_records)  # alive until the kernels have run
        return out

    def _upload(self, host, dtype):
        """A host array / tensor onto this device through pinned staging, asynchronously on the launch stream (torch's caching
        host allocator keeps the staging buffer until the copy has run: the caller's array is free when this returns)."""
        host = host.detach() if isinstance(host, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(host))
        pin = torch.empty(tuple(host.shape), dtype=dtype, pin_memory=True)
        pin.copy_(host)
        with torch.cuda.device(self.device):
            return pin.to(self.device, non_blocking=True)

    def eval_batch(self, records, gt_poses, gt_experts=None, rot_threshold_deg=5.0, trans_threshold_cm=5.0, out=None):
        """The test loop's figures of B frames on the device (esac_hip_eval_batch): records = the device float64 [B,32] a forward
        batch wrote through result_out, gt_poses float32 [B,4,4], gt_experts int64 [B] or None.  One launch on torch's current
        stream, behind whatever wrote the records; nothing is waited for.  A host gt_poses / gt_experts is uploaded with
        non_blocking=True on that stream.  Returns the device float64 tensor [B,16] of rows (`out` when given; columns: EVAL_*)."""
        B = _check_eval_args("esac.eval_batch", records, gt_poses, gt_experts, rot_threshold_deg, trans_threshold_cm)
        if out is not None and not (isinstance(out, torch.Tensor) and out.is_cuda and out.is_contiguous() and out.dtype == torch.float64
                                    and tuple(out.shape) == (B, EVAL_DOUBLES)):
            raise RuntimeError("esac.eval_batch: out must be a dense float64 device tensor [B,%d]" % EVAL_DOUBLES)
        if records.device != self.device:
            raise RuntimeError("esac.eval_batch: records live on %s, this engine on %s" % (records.device, self.device))
        gt = gt_poses if isinstance(gt_poses, torch.Tensor) and gt_poses.is_cuda else \
            self._upload(gt_poses if isinstance(gt_poses, torch.Tensor) else np.asarray(gt_poses, np.float32), torch.float32)
        gt = gt.contiguous()
        ge = None
        if gt_experts is not None:
            ge = gt_experts if isinstance(gt_experts, torch.Tensor) and gt_experts.is_cuda else \
                self._upload(gt_experts if isinstance(gt_experts, torch.Tensor) else np.asarray(gt_experts, np.int64), torch.int64)
            ge = ge.contiguous()
        if gt.device != self.device or (ge is not None and ge.device != self.device):
            raise RuntimeError("esac.eval_batch: records, gtPoses and gtExperts must live on one device")
        if out is None:
            out = torch.empty((B, EVAL_DOUBLES), dtype=torch.float64, device=self.device)
        rc = self.lib.esac_hip_eval_batch(self.ctx, B, records.data_ptr(), gt.data_ptr(), ge.data_ptr() if ge is not None else None,
                                          float(rot_threshold_deg), float(trans_threshold_cm), self._stream(), out.data_ptr())
        if rc != 0:
            _check(rc, self.lib)
        self._keep_eval = (records, gt, ge, out)  # alive until the kernel has run
        return out

    def verify_batch(self, scene_coords, poses, experts, params, cams=None, shapes=None, out=None):
        """K given poses per frame against the maps (esac_hip_verify_batch): score, inlier count, SSE, normal matrix and pose
        covariance of each.  scene_coords float32 [B,E,3,H,W], [E,3,H,W] (shared by all frames) or, with shapes, the packed
        [B,S] tensor of pack_frames; poses float64 [B,K,6] (rvec | tvec, scene -> camera) or float32 [B,K,4,4] (camera poses as
        outPose / gtPoses carry them); experts int32 / int64 [B,K], or [B]: one expert per frame for all K.  params: one frame
        (make_params; E, the grid or a ragged batch's capacity, the camera, the score parameters, strict_reference).  cams /
        shapes: as in forward_batch.  One launch on torch's current stream, behind whatever wrote the inputs; nothing is waited
        for; host poses / experts are uploaded asynchronously on that stream.  Returns the device float64 [B,K,64] of rows
        (`out` when given; columns: VERIFY_*)."""
        who = "esac.verify_batch"
        B, K, fmt = _check_verify_args(who, scene_coords, poses, experts, shapes, out)
        sc = self._on_device(scene_coords)
        po = (poses if poses.is_cuda else self._upload(poses, poses.dtype)).contiguous()
        ex = experts if isinstance(experts, torch.Tensor) and experts.is_cuda else \
            self._upload(torch.as_tensor(np.asarray(experts, np.int64) if not isinstance(experts, torch.Tensor) else experts).clamp(-1, 2 ** 31 - 1), torch.int32)
        if ex.dtype != torch.int32:
            # on the device, in stream order; clamped first: an int64 beyond int32 must stay outside [0,E), not wrap into it
            ex = ex.clamp(-1, 2 ** 31 - 1).to(torch.int32)
        if ex.dim() == 1:
            ex = ex.unsqueeze(1).expand(B, K)
        ex = ex.contiguous()
        for name, t in (("sceneCoordinates", sc), ("poses", po), ("experts", ex)) + ((("out", out),) if out is not None else ()):
            if t.device != self.device:
                raise RuntimeError("%s: %s lives on %s, this engine on %s" % (who, name, t.device, self.device))
        if out is None:
            out = torch.empty((B, K, VERIFY_DOUBLES), dtype=torch.float64, device=self.device)
        table, ragged = _frame_table(who, params, cams, shapes if shapes is None else _shapes_arg(who, shapes, B), B)
        self._call(self.lib.esac_hip_verify_batch, B, K, sc.data_ptr(), _frame_stride(sc), po.data_ptr(), fmt, ex.data_ptr(), C.byref(params),
                   table.ctypes.data if table is not None else None, ragged, self._stream(), out.data_ptr())
        self._keep_verify = (sc, po, ex, out)  # alive until the kernel has run
        return out

    def read_frames(self, which, B):
        """A training-path buffer (BUF_BWD_PROBS / _LOSSES / _REF_HYPS / _SCORE_GRADS / _SLOTS / _SLOT_INFO / _DLOSS) of all B
        frames of the last batched backward call, frame-major: [B, ...single-frame shape]."""
        N, H, W = self._shape
        rows = min(N, BWD_MAX_SLOTS)
        shapes = {BUF_BWD_PROBS: ((N,), np.float64), BUF_BWD_LOSSES: ((N,), np.float64), BUF_BWD_REF_HYPS: ((N, 6), np.float64),
                  BUF_BWD_SCORE_GRADS: ((N,), np.float64), BUF_BWD_SLOTS: ((N,), np.int32),
                  BUF_BWD_SLOT_INFO: ((rows, 4), np.int32), BUF_BWD_DLOSS: ((rows, 6), np.float64)}
        shape, dt = shapes[which]
        out = np.zeros((int(B),) + shape, dt)
        _check(self.lib.esac_hip_read(self.ctx, which, out.ctypes.data_as(C.c_void_p), out.nbytes), self.lib)
        return out

    def read_forward_frames(self, which, B):
        """BUF_HYPS / _SAMPLE_XY / _TRIES / _SCORES / _INLIER_COUNTS of all B frames of the last batched call, frame-major.
        After a ragged batch (forward_batch(shapes=...)) the strides stay the capacity's: these five are per hypothesis and
        read as ever (sampled cells index frame b's own w_b-wide grid); a per-cell buffer (read(BUF_INLIER_MAP): frame 0, returned
        at the capacity's [H,W]) holds the frame's data in its first h_b*w_b entries: out.reshape(-1)[:h*w].reshape(h, w)."""
        N, H, W = self._shape
        shapes = {BUF_HYPS: ((N, 6), np.float64), BUF_SAMPLE_XY: ((N, 4, 2), np.int32), BUF_TRIES: ((N,), np.int32),
                  BUF_SCORES: ((N,), np.float64), BUF_INLIER_COUNTS: ((MAX_REF_STEPS + 1,), np.int32)}
        shape, dt = shapes[which]
        out = np.zeros((int(B),) + shape, dt)
        _check(self.lib.esac_hip_read(self.ctx, which, out.ctypes.data_as(C.c_void_p), out.nbytes), self.lib)
        return out

    # -- single phases (stage-wise parity tests)
    def _phase(self, fn, scene_coords, hyp_assign, params):
        sc, ha = self._dev_inputs(scene_coords, hyp_assign)
        with torch.cuda.device(self.device):
            _check(fn(self.ctx, sc.data_ptr(), ha.data_ptr(), C.byref(params), self._stream()), self.lib)
        self._keep = (sc, ha)

    def sample(self, sc, ha, p):
        self._phase(self.lib.esac_hip_sample, sc, ha, p)

    def score(self, sc, ha, p):
        self._phase(self.lib.esac_hip_score, sc, ha, p)

    def select(self, sc, ha, p):
        self._phase(self.lib.esac_hip_select, sc, ha, p)

    def refine(self, sc, ha, p):
        self._phase(self.lib.esac_hip_refine, sc, ha, p)

    def score_exact(self, sc, ha, p):
        self._phase(self.lib.esac_hip_score_exact, sc, ha, p)

    def write_hyps(self, hyps):
        h = np.ascontiguousarray(hyps, np.float64)
        assert h.ndim == 2 and h.shape[1] == 6
        _check(self.lib.esac_hip_write_hyps(self.ctx, h.ctypes.data_as(C.c_void_p), h.shape[0]), self.lib)

    def read_slabs(self, which, k, shape=None):
        """Gradient slabs [k,3,H,W] (float64) of the first k slots of the last backward call (BUF_BWD_PATH1 / _PATH2).
        shape: after a ragged batch (backward_batch_shapes), the (h, w) of frame 0 of its last chunk -- that frame's slots
        lie at its own h*w, and the slabs come back as [k,3,h,w]."""
        _, H, W = self._shape
        if shape is not None:
            H, W = int(shape[0]), int(shape[1])
        out = np.zeros((int(k), 3, H, W), np.float64)
        _check(self.lib.esac_hip_read(self.ctx, which, out.ctypes.data_as(C.c_void_p), out.nbytes), self.lib)
        return out

    def read_maps(self, k, shape=None):
        """Both inlier-map buffers [k,2,H*W] (uint8, cells as y * W + x) of the first k slots of the last blocking backward call
        (BUF_BWD_MAPS); BUF_BWD_SLOT_INFO[s][0] names the one holding slot s's last accepted inlier set (-1: neither).
        shape: after a ragged batch, frame 0's own (h, w), as in read_slabs."""
        _, H, W = self._shape
        if shape is not None:
            H, W = int(shape[0]), int(shape[1])
        out = np.zeros((int(k), 2, H * W), np.uint8)
        _check(self.lib.esac_hip_read(self.ctx, BUF_BWD_MAPS, out.ctypes.data_as(C.c_void_p), out.nbytes), self.lib)
        return out

    def read(self, which):
        N, H, W = self._shape or (0, 0, 0)  # (the context-level info buffers need no shape)
        shapes = {
            BUF_HYPS: ((N, 6), np.float64), BUF_SAMPLE_XY: ((N, 4, 2), np.int32), BUF_TRIES: ((N,), np.int32),
            BUF_SCORES: ((N,), np.float64), BUF_RESULT: ((RES_DOUBLES,), np.float64),
            BUF_INLIER_MAP: ((H, W), np.uint8), BUF_INLIER_COUNTS: ((MAX_REF_STEPS + 1,), np.int32),
            BUF_WINNER_ERRS: ((H, W), np.float32), BUF_EXACT_FLAGS: ((N,), np.uint8),
            BUF_CYCLES: ((32,), np.int64), BUF_REFINE_INFO: ((8,), np.int32), BUF_BWD_TEAM_INFO: ((4,), np.int32), BUF_SPEC_INFO: ((4,), np.int32), BUF_SPEC_FLAGS: ((N,), np.uint8),
            BUF_BWD_PROBS: ((N,), np.float64), BUF_BWD_LOSSES: ((N,), np.float64), BUF_BWD_REF_HYPS: ((N, 6), np.float64),
            BUF_BWD_SCORE_GRADS: ((N,), np.float64), BUF_BWD_SLOTS: ((N,), np.int32),
            BUF_BWD_SLOT_INFO: ((min(N, BWD_MAX_SLOTS), 4), np.int32), BUF_BWD_DLOSS: ((min(N, BWD_MAX_SLOTS), 6), np.float64),
        }
        shape, dt = shapes[which]
        out = np.zeros(shape, dt)
        _check(self.lib.esac_hip_read(self.ctx, which, out.ctypes.data_as(C.c_void_p), out.nbytes), self.lib)
        return out

    def time_stages(self, scene_coords, hyp_assign, params, reps=20):
        """Mean GPU time (ms) of sample / score / select / refine for this input (esac_hip_time_stages)."""
        sc, ha = self._dev_inputs(scene_coords, hyp_assign)
        out = np.zeros(4, np.float32)
        self._call(self.lib.esac_hip_time_stages, sc.data_ptr(), ha.data_ptr(), C.byref(params), self._stream(), int(reps),
                   out.ctypes.data)
        return dict(zip(("sample", "score", "select_rescore", "refine"), (float(v) for v in out)))

    def pick_record(self, records, world, zero=None):
        """Global winner among `world` per-rank records (device float64 [world*32], e.g. the tail of the all-reduced
        exchange buffer): picked on the device, returned as np.float64[32].  zero: optional device float64 tensor the same
        launch clears (the exchange buffer of the NEXT call)."""
        assert records.is_cuda and records.dtype == torch.float64 and records.is_contiguous() and records.numel() >= 32 * world
        assert zero is None or (zero.is_cuda and zero.dtype == torch.float64 and zero.is_contiguous())
        rc = self.lib.esac_hip_pick_record(self.ctx, records.data_ptr(), int(world), self._stream(), self._host_addr,
                                           zero.data_ptr() if zero is not None else None, int(zero.numel()) if zero is not None else 0)
        if rc != 0:
            _check(rc, self.lib)
        return self._host_np.copy()

    def shard_balanced(self, hyp_assign, world, rank, E, expert_base=0, index_out=None, assign_out=None, info_out=None):
        """This rank's share of the load-balanced split of `hyp_assign` (device int64 [N]), built on the device in one
        asynchronous launch (esac_hip_shard_balanced): returns (global indices int32 [n_local], local assignment int64
        [n_local], info int32 [4] = first expert, last expert, n_local, out-of-range flag) -- all device tensors."""
        assert hyp_assign.is_cuda and hyp_assign.dtype == torch.int64 and hyp_assign.is_contiguous()
        N = int(hyp_assign.shape[0])
        n_local = N // world + (1 if rank < N % world else 0)
        dev = self.device
        if index_out is None:
            index_out = torch.empty(max(n_local, 1), dtype=torch.int32, device=dev)
        if assign_out is None:
            assign_out = torch.empty(max(n_local, 1), dtype=torch.int64, device=dev)
        if info_out is None:
            info_out = torch.empty(4, dtype=torch.int32, device=dev)
        self._call(self.lib.esac_hip_shard_balanced, hyp_assign.data_ptr(), N, int(E), int(world), int(rank), int(expert_base),
                   self._stream(), index_out.data_ptr(), assign_out.data_ptr(), info_out.data_ptr())
        self._keep_shard = (hyp_assign, index_out, assign_out, info_out)
        return index_out[:n_local], assign_out[:n_local], info_out

    def set_wait(self, mode):
        """How blocking calls wait for their record: WAIT_SPIN (default), WAIT_YIELD, WAIT_BLOCK (esac_hip_set_wait)."""
        _check(self.lib.esac_hip_set_wait(self.ctx, int(mode)), self.lib)

    def check(self):
        """Waits for the device; raises if the most recent (asynchronous) call met an out-of-range hypAssignment."""
        _check(self.lib.esac_hip_check(self.ctx), self.lib)

    def set_debug(self, keep_error_image=False, coop_stall=False, team_spread=False, no_speculation=False, spec_second_best=False,
                  spec_lose_chain=False):
        _check(self.lib.esac_hip_set_debug(self.ctx, (DEBUG_ERROR_IMAGE if keep_error_image else 0) | (DEBUG_COOP_STALL if coop_stall else 0) |
                                           (DEBUG_TEAM_SPREAD if team_spread else 0) | (DEBUG_NO_SPECULATION if no_speculation else 0) |
                                           (DEBUG_SPEC_SECOND_BEST if spec_second_best else 0) | (DEBUG_SPEC_LOSE_CHAIN if spec_lose_chain else 0)), self.lib)

    def spec_info(self):
        """The speculative forward route (several experts: the straggler chain beside the refinement; ESAC_BUF_SPEC_INFO)."""
        v = self.read(BUF_SPEC_INFO)
        return {"calls": int(v[0]), "failures": int(v[1]), "last_speculative": bool(v[2]), "last_failed": bool(v[3])}

    def set_refine_team(self, members=REFINE_TEAM_DEFAULT):
        """Workgroups that share the winner's refinement on a small single-frame grid (0 / 1: one workgroup; a number: exactly
        that many; REFINE_TEAM_AUTO = the default policy: 8, or the smallest team <= 16 that lowers the cells a lane holds --
        10 on the 60x80 grid; esac_hip_set_refine_team)."""
        _check(self.lib.esac_hip_set_refine_team(self.ctx, int(members)), self.lib)

    def set_refine_route(self, on=True):
        """May a single frame's team run the kernel with the headline call's modes compiled in (esac_hip_set_refine_route)?
        False: every team runs the general kernel -- same outputs, bit for bit."""
        _check(self.lib.esac_hip_set_refine_route(self.ctx, 1 if on else 0), self.lib)

    def set_front_route(self, on=True):
        """May a single frame's forward call sample and score with the kernels that have the headline call's modes compiled in
        (esac_hip_set_front_route)?  False: every call runs the general kernels -- same outputs, bit for bit."""
        _check(self.lib.esac_hip_set_front_route(self.ctx, 1 if on else 0), self.lib)

    def front_route_taken(self):
        """Did the most recent forward call on this engine sample and score with the route kernels (esac_hip_front_route_taken)?"""
        rc = self.lib.esac_hip_front_route_taken(self.ctx)
        _check(min(rc, 0), self.lib)
        return rc == 1

    def read_rotations(self, N):
        """The [N,3,3] rotation matrices the sampler stored beside the hypotheses of the most recent call (esac_hip_read_rotations)."""
        out = np.zeros((int(N), 3, 3), np.float64)
        _check(self.lib.esac_hip_read_rotations(self.ctx, out.ctypes.data_as(C.c_void_p), int(N)), self.lib)
        return out

    def bwd_team_info(self):
        """Training path: were the slots of the last backward call refined by teams (ESAC_BUF_BWD_TEAM_INFO)."""
        v = self.read(BUF_BWD_TEAM_INFO)
        return {"teams": bool(v[0]), "team_calls": int(v[1]), "team_fallbacks": int(v[2]), "slots": int(v[3])}

    def refine_info(self):
        """How the most recent winner refinement ran (ESAC_BUF_REFINE_INFO).  `same_xcd`: the census of the team's first
        exchange found every member on one XCD -- the exchanges after it then stayed in that XCD's L2 (plain granule stores,
        refine_common.hpp:gran_store); otherwise they were written through (valid at any placement, 0.1-0.3 us slower each)."""
        v = self.read(BUF_REFINE_INFO)
        return {"mode": ("one_workgroup", "cooperating", "team")[int(v[0])] if 0 <= int(v[0]) <= 2 else int(v[0]),
                "workgroups": int(v[1]),
                "xcd_census": [(int(v[2]) >> (8 * x)) & 255 for x in range(4)] + [(int(v[7]) >> (8 * x)) & 255 for x in range(4)],
                "same_xcd": bool(int(v[3]) & 1), "route_kernel": bool(int(v[3]) & 2),
                "exchanges": int(v[4]), "timed_out": bool(v[5]), "team_fallbacks": int(v[6]) & 0x3fffffff,
                "team_latched_off": bool(int(v[6]) & 0x40000000)}

    # -- the multi-GPU score exchange straight on RCCL (esac_hip_comm_*; distributed.py bootstraps the id)
    def comm_unique_id(self):
        buf = (C.c_ubyte * COMM_ID_BYTES)()
        _check(self.lib.esac_hip_comm_unique_id(buf, COMM_ID_BYTES), self.lib)
        return bytes(buf)

    def comm_init(self, nranks, rank, unique_id):
        assert len(unique_id) == COMM_ID_BYTES
        buf = (C.c_ubyte * COMM_ID_BYTES).from_buffer_copy(unique_id)
        _check(self.lib.esac_hip_comm_init(self.ctx, int(nranks), int(rank), buf, COMM_ID_BYTES), self.lib)
        self._comm = (int(nranks), int(rank))

    def comm_destroy(self):
        _check(self.lib.esac_hip_comm_destroy(self.ctx), self.lib)
        self._comm = None
        self._comm_key = None

    def comm_info(self):
        """What the communicator itself reports (esac_hip_comm_info): ranks it spans, this rank, the GPU RCCL bound it to, the
        context's GPU."""
        out = (C.c_int32 * 4)()
        _check(self.lib.esac_hip_comm_info(self.ctx, out), self.lib)
        return {"nranks": int(out[0]), "rank": int(out[1]), "rccl_device": int(out[2]), "device": int(out[3])}

    def allreduce_sum(self, buf):
        """In-place all-reduce(SUM) of a device float64 tensor over this engine's RCCL communicator, on the current stream."""
        rc = self.lib.esac_hip_allreduce_sum(self.ctx, buf.data_ptr(), int(buf.numel()), self._stream())
        if rc != 0:
            _check(rc, self.lib)

    def host_turn(self):
        """Host-side stamps of the most recent blocking forward (esac_hip_host_turn), in microseconds after entry."""
        out = np.zeros(8, np.float64)
        _check(self.lib.esac_hip_host_turn(self.ctx, out.ctypes.data), self.lib)
        return {"args_ready": out[0] * 1e-3, "sample_launched": out[1] * 1e-3, "score_launched": out[2] * 1e-3, "refine_launched": out[3] * 1e-3,
                "record_landed": out[4] * 1e-3, "returned": out[5] * 1e-3, "entry_ns": out[6]}

    def host_turn_mean(self, reset=True):
        """Means of the host-side stamps over the blocking forward calls since the last reset (esac_hip_host_turn_mean), in us:
        where the host's share of a step goes."""
        out = np.zeros(8, np.float64)
        _check(self.lib.esac_hip_host_turn_mean(self.ctx, out.ctypes.data, 1 if reset else 0), self.lib)
        u = out * 1e-3
        return {"calls": int(out[7]), "args_ready": u[0], "first_launch_call": u[1] - u[0], "further_launch_calls": u[3] - u[1],
                "wait_for_record": u[4] - u[3], "record_to_return": u[5] - u[4], "call_total": u[5], "between_calls": u[6]}

    def set_timing(self, on, period=1):
        """Per-phase events on every `period`-th forward call (the next call is the first sampled one)."""
        _check(self.lib.esac_hip_set_timing(self.ctx, (max(1, int(period)) if on else 0)), self.lib)

    def phase_ms(self):
        out = np.zeros(6, np.float32)
        _check(self.lib.esac_hip_phase_ms(self.ctx, out.ctypes.data_as(C.c_void_p)), self.lib)
        return out

    def score_span_ms(self):
        """(mean device-side duration of the score kernel in ms, number of launches averaged)."""
        ms, n = C.c_float(0), C.c_int(0)
        _check(self.lib.esac_hip_score_span_ms(self.ctx, C.byref(ms), C.byref(n)), self.lib)
        return float(ms.value), int(n.value)


# ---------------------------------------------------------------- module-level state
# The reference keeps a static RNG whose state advances from call to call
# (thread_rand.cpp:4-5); here that state is (seed, call counter).
_state = {"seed": 1305, "call": 0, "engines": {}, "last": None, "max_tries": 0, "max_ref_steps": -1, "fwd_cache": {},
          "exact_scores": None, "exact_sampling": False, "strict_reference": False, "strict_training": False,
          "pose_records": None}


def set_seed(seed, call=0):
    """ThreadRand::forceInit equivalent (thread_rand.cpp:7-11; not exported by the reference)."""
    _state["seed"], _state["call"] = int(seed), int(call)


def get_rng_state():
    return _state["seed"], _state["call"]


def set_limits(max_tries=0, max_ref_steps=-1):
    """Override MAX_SAMPLING_TRIES / MAX_REF_STEPS (esac.cpp:44-45); 0 / -1 restore the reference values."""
    _state["max_tries"], _state["max_ref_steps"] = int(max_tries), int(max_ref_steps)


def set_exact_scores(on):
    """True: every hypothesis is scored in the reference's arithmetic (ESAC_FLAG_EXACT_SCORES), so the score vector of
    last_result() and the record's probability / entropy are the reference's own values; the pose is the same either way.
    False: the fp32 ranking stream + exact re-score of the contenders everywhere.  None (the default): exact where it is
    free -- one expert, N * H * W <= 2^21, i.e. the reference's own 64- and 256-hypothesis configurations
    (ESAC_FLAG_AUTO_EXACT) -- and the ranking stream elsewhere."""
    _state["exact_scores"] = None if on is None else bool(on)


def set_exact_sampling(on):
    """True: no screen in the sampling loop -- every try of every hypothesis is solved and decided by the fp64 route
    (ESAC_FLAG_EXACT_SAMPLING), the reference's loop try by try (esac_util.h:152-223).  The accepted try is the same either
    way; this is the guaranteed route (several times slower on wrong-expert hypotheses)."""
    _state["exact_sampling"] = bool(on)


def set_strict_reference(on):
    """True: forward() and forward_batch() follow the reference where the default knowingly differs (ESAC_FLAG_STRICT_REFERENCE):
    Horn / Jacobi alignment in the P3P, NaN scores from non-finite scene coordinates (hypothesis 0 is then refined), the plain
    CvLevMarq trial test.  Implies exact scores and exact sampling; a verification route, several times slower.  backward() and
    backward_batch() raise ValueError while it is on: the training path has no strict mode."""
    _state["strict_reference"] = bool(on)


def set_strict_training(on):
    """True: backward() and backward_batch() follow the reference in every stage where the default knowingly differs
    (ESAC_FLAG_STRICT_TRAINING): Horn / Jacobi alignment in the sampler and in the 18 perturbed solves of dPNP, NaN scores from
    non-finite scene coordinates (the call returns a NaN loss and NaN gradients instead of raising), the plain CvLevMarq trial
    test in the slot refinement, the SVD pseudo-inverse on every slot.  A verification route; forward() ignores it."""
    _state["strict_training"] = bool(on)


def set_pose_records(records):
    """Arms the NEXT training call of this module (backward, backward_batch, backward_batch_async): a float64 tensor [32] (backward)
    or [B,32] (the batched calls), filled in place with the forward-format record (RES_*) of each frame's argmax hypothesis, as the
    batched calls' poseRecords argument does -- `backward` keeps the reference's parameter list, so this is its route.  One-shot:
    taken by that call whether it runs or raises; None disarms.  Shape and device are checked again by the call."""
    if records is not None:
        B = records.shape[0] if isinstance(records, torch.Tensor) and records.dim() == 2 else None
        _check_pose_records("esac.set_pose_records", "records", records, B, False)
    _state["pose_records"] = records


def _take_pose_records(given):
    """The record tensor of this call: its own argument, else what set_pose_records left (consumed either way)."""
    armed, _state["pose_records"] = _state["pose_records"], None
    return given if given is not None else armed


def _no_strict_training(who):
    if _state["strict_reference"]:
        raise ValueError("%s: the training path has no strict mode (esac.set_strict_reference(False) first)" % who)


def engine(device=None):
    idx = torch.cuda.current_device() if device is None else int(device)
    eng = _state["engines"].get(idx)
    if eng is None:
        eng = _state["engines"][idx] = Engine(idx)
    return eng


def _engine_for(*inputs):
    """The engine of the first device tensor among `inputs` (tensors, or lists of tensors), else the current GPU's."""
    for x in inputs:
        for t in x if isinstance(x, (list, tuple)) else (x,):
            if isinstance(t, torch.Tensor) and t.is_cuda:
                return engine(t.device.index)
    return engine(None)


def _call_params(eng, E, H, W, N, cam_scalars, score_args, *, training):
    """One call's parameter block from the module state: seed, call counter (read, not advanced), limits and the strict mode of
    the path -- training: set_strict_training's, otherwise set_strict_reference's."""
    strict = {"strict_training": _state["strict_training"]} if training else {"strict_reference": _state["strict_reference"]}
    return eng.make_params(E, H, W, N, *cam_scalars, *score_args, seed=_state["seed"], call=_state["call"],
                           max_tries=_state["max_tries"], max_ref_steps=_state["max_ref_steps"], **strict)


def _stage_gradients(outGradients, eng):
    """The gradient tensor the kernels accumulate into: (outGradients, False) when it is dense on eng's device, else (a dense
    device copy, True) -- the caller then copies it back into its own (CPU or strided) storage after the call."""
    if outGradients.is_cuda and outGradients.is_contiguous() and outGradients.device == eng.device:
        return outGradients, False
    return outGradients.to(eng.device).contiguous(), True


def _check_assignment_range(who, hypAssignment, E):
    """A host hypAssignment must lie in [0,E) (a device one is judged by the kernels: no round trip).  Touches no device."""
    if not hypAssignment.is_cuda:
        lo, hi = int(hypAssignment.min()), int(hypAssignment.max())
        if lo < 0 or hi >= E:
            raise RuntimeError("%s: hypAssignment values must lie in [0,%d), found [%d,%d]" % (who, E, lo, hi))


def _check_async_tensors(who, sceneCoordinates, outGradients, hypAssignment, gtPoses, host_gradients):
    """What an asynchronous training call asks of its tensors: a contiguous outGradients, the first three on a device, all on
    one device.  host_gradients: the call's own words for an outGradients on the host.  Touches no device."""
    if not outGradients.is_contiguous():
        raise RuntimeError("%s: outGradients must be contiguous (an asynchronous call cannot copy back into strided storage)" % who)
    for name, t, why in (("outGradients", outGradients, host_gradients),
                         ("sceneCoordinates", sceneCoordinates, "stages nothing on the host"),
                         ("hypAssignment", hypAssignment, "stages nothing on the host")):
        if not t.is_cuda:
            raise RuntimeError("%s: %s must be a device tensor (an asynchronous call %s)" % (who, name, why))
    if outGradients.device != sceneCoordinates.device or hypAssignment.device != sceneCoordinates.device or \
            (gtPoses.is_cuda and gtPoses.device != sceneCoordinates.device):
        raise RuntimeError("%s: sceneCoordinates, outGradients, hypAssignment and a device gtPoses must live on one device" % who)


def last_result():
    """Details of the most recent forward(): scores tensor (device, float64 [N]; a buffer the next call with the same
    signature overwrites -- clone it to keep it) and the result record."""
    return _state["last"]


def _validate(sceneCoordinates, hypAssignment, outPose):
    # what accessor<float,4>() / accessor<long,1>() / accessor<float,2>() enforce (esac.cpp:80-84,184)
    for name, t, dt, nd in (("sceneCoordinates", sceneCoordinates, torch.float32, 4),
                            ("hypAssignment", hypAssignment, torch.int64, 1), ("outPose", outPose, torch.float32, 2)):
        if not isinstance(t, torch.Tensor):
            raise RuntimeError("esac.forward: %s must be a torch.Tensor" % name)
        if t.dtype != dt:
            raise RuntimeError("esac.forward: expected scalar type %s for %s but found %s" % (dt, name, t.dtype))
        if t.dim() != nd:
            raise RuntimeError("esac.forward: expected %d dims for %s but tensor has %d" % (nd, name, t.dim()))
    if sceneCoordinates.size(1) != 3:
        raise RuntimeError("esac.forward: sceneCoordinates must be [E,3,H,W]")
    if tuple(outPose.shape) != (4, 4):
        raise RuntimeError("esac.forward: outPose must be [4,4]")
    if hypAssignment.numel() == 0:
        raise RuntimeError("esac.forward: hypAssignment is empty")


def forward(sceneCoordinates, hypAssignment, outPose, shiftX, shiftY, focalLength, ppointX, ppointY,
            inlierThreshold, inlierAlpha, inlierBeta, maxReproj, subSampling):
    """Drop-in for `esac.forward` (esac.cpp:64-77): estimates the pose, writes the 4x4 camera
    transform into `outPose` in place and returns the winning expert as a Python int.

    Tensors may live on the CPU (as the reference requires) or already on the GPU
    (then the `.cpu()` at test_esac.py:187 can be dropped)."""
    _validate(sceneCoordinates, hypAssignment, outPose)
    dev = sceneCoordinates.device.index if sceneCoordinates.is_cuda else None
    eng = engine(dev)
    E, _, H, W = sceneCoordinates.shape
    N = hypAssignment.shape[0]
    if not hypAssignment.is_cuda:
        lo, hi = torch.aminmax(hypAssignment)
        if int(lo) < 0 or int(hi) >= E:
            raise RuntimeError("esac.forward: hypAssignment values must lie in [0,%d), found [%d,%d]" % (E, int(lo), int(hi)))
    # parameter block and score buffer are kept per SHAPE; the scalar fields are rewritten per call (a per-frame focal
    # length -- Aachen, Dubrovnik -- must not evict anything)
    key = (eng.device.index, E, H, W, N)
    cached = _state["fwd_cache"].get(key)
    if cached is None:
        if len(_state["fwd_cache"]) > 16:
            _state["fwd_cache"].clear()
        cached = [eng.make_params(E, H, W, N), torch.empty(N, dtype=torch.float64, device=eng.device), None]
        _state["fwd_cache"][key] = cached
    p, scores = cached[0], cached[1]
    if not sceneCoordinates.is_cuda or not hypAssignment.is_cuda:
        # the reference's convention (test_esac.py:187 `.cpu()`): CPU tensors in.  They go through PINNED staging buffers kept per
        # shape -- one host copy (which also resolves strides and the stride-0 expand() of --expertselection) and an asynchronous
        # H2D on the launch stream, instead of a pageable-memory transfer and a device allocation per call.  The call is
        # blocking, so the buffers are free again when it returns.
        if cached[2] is None:
            cached[2] = (torch.empty((E, 3, H, W), dtype=torch.float32, pin_memory=True), torch.empty((E, 3, H, W), dtype=torch.float32, device=eng.device),
                         torch.empty(N, dtype=torch.int64, pin_memory=True), torch.empty(N, dtype=torch.int64, device=eng.device), None)
        pin_sc, dev_sc, pin_ha, dev_ha = cached[2][:4]
        with torch.cuda.device(eng.device):
            if not sceneCoordinates.is_cuda:
                pin_sc.copy_(sceneCoordinates)
                dev_sc.copy_(pin_sc, non_blocking=True)
                sceneCoordinates = dev_sc
            if not hypAssignment.is_cuda:
                if E == 1:
                    # one expert: the kernels never read the assignment vector (device_common.hpp:expert_of), and the host check
                    # above has seen that it holds nothing but zeros -- no transfer
                    if cached[2][4] is None:
                        cached[2] = cached[2][:4] + (torch.zeros(N, dtype=torch.int64, device=eng.device),)
                    hypAssignment = cached[2][4]
                else:
                    pin_ha.copy_(hypAssignment)
                    dev_ha.copy_(pin_ha, non_blocking=True)
                    hypAssignment = dev_ha
    p.shift_x, p.shift_y = int(shiftX), int(shiftY)
    p.focal, p.ppx, p.ppy = float(focalLength), float(ppointX), float(ppointY)
    p.inlier_thresh, p.inlier_alpha, p.inlier_beta = float(inlierThreshold), float(inlierAlpha), float(inlierBeta)
    p.max_reproj, p.sub_sampling = float(maxReproj), int(subSampling)
    p.max_tries, p.max_ref_steps = int(_state["max_tries"]), int(_state["max_ref_steps"])
    p.flags = (FLAG_AUTO_EXACT if _state["exact_scores"] is None else FLAG_EXACT_SCORES if _state["exact_scores"] else 0) | \
        (FLAG_EXACT_SAMPLING if _state["exact_sampling"] else 0)
    if _state["strict_reference"]:  # (never with FLAG_AUTO_EXACT: strict mode IS the exact routes)
        p.flags = FLAG_STRICT_REFERENCE | FLAG_EXACT_SCORES | FLAG_EXACT_SAMPLING
    p.seed, p.call = _state["seed"] & (2**64 - 1), _state["call"] & (2**64 - 1)
    eng._shape = (int(N), int(H), int(W))
    _state["call"] += 1
    res = eng.forward_device(sceneCoordinates, hypAssignment, p, scores_out=scores)
    # in place, caller-owned (esac.cpp:184-187)
    if not outPose.is_cuda and outPose.is_contiguous():
        outPose.numpy()[:] = res[RES_POSE:RES_POSE + 16].reshape(4, 4)
    else:
        outPose.copy_(torch.from_numpy(res[RES_POSE:RES_POSE + 16].astype(np.float32).reshape(4, 4)))
    _state["last"] = {"scores": scores, "result": res, "winner": int(res[RES_HYP]), "expert": int(res[RES_EXPERT])}
    return int(res[RES_EXPERT])


_CAM_ARGS = ("shiftX", "shiftY", "focalLength", "ppointX", "ppointY")


def _per_frame_cams(who, B, shiftX, shiftY, focalLength, ppointX, ppointY):
    """The five camera arguments of a batched call: each a scalar (one value for the batch) or a length-B sequence / 1-D tensor /
    numpy array (one value per frame).  Returns (scalars, cams): all five scalars -> (the five values, None), today's call;
    otherwise scalars are broadcast and cams is the table of B records (frame 0's values stand in the parameter block).
    Raises RuntimeError naming the argument; touches no device."""
    cols, per_frame = [], False
    for name, v in zip(_CAM_ARGS, (shiftX, shiftY, focalLength, ppointX, ppointY)):
        if isinstance(v, torch.Tensor):
            v = v.detach().cpu().numpy()
        if isinstance(v, (list, tuple)):
            try:
                v = np.asarray(v, dtype=np.float64)
            except (TypeError, ValueError):
                raise RuntimeError("%s: %s must be a number or a sequence of B numbers" % (who, name))
        if isinstance(v, np.ndarray) and v.ndim > 0:
            if v.ndim != 1 or v.shape[0] != B:
                raise RuntimeError("%s: %s must be a scalar or hold one value per frame (%d), found shape %s"
                                   % (who, name, B, tuple(v.shape)))
            if v.dtype.kind not in "iuf":
                raise RuntimeError("%s: %s must be numeric, found dtype %s" % (who, name, v.dtype))
            per_frame = True
            col = v.astype(np.float64)
        else:
            try:
                col = np.full(B, float(v), np.float64)
            except (TypeError, ValueError):
                raise RuntimeError("%s: %s must be a number or a sequence of B numbers" % (who, name))
        cols.append(col)
    if not per_frame:
        return (shiftX, shiftY, focalLength, ppointX, ppointY), None
    for name, col in zip(_CAM_ARGS, cols):
        if not np.all(np.isfinite(col)):
            raise RuntimeError("%s: %s holds a non-finite value (frame %d)" % (who, name, int(np.flatnonzero(~np.isfinite(col))[0])))
    for name, col in zip(_CAM_ARGS[:2], cols[:2]):
        bad = np.flatnonzero((col != np.round(col)) | (np.abs(col) > 2**31 - 1))
        if bad.size:
            raise RuntimeError("%s: %s must hold integers within int32 (frame %d: %r)" % (who, name, int(bad[0]), float(col[bad[0]])))
    bad = np.flatnonzero(~(cols[2] > 0))
    if bad.size:
        raise RuntimeError("%s: focalLength must be positive (frame %d: %r)" % (who, int(bad[0]), float(cols[2][bad[0]])))
    cams = make_cams(cols[0], cols[1], cols[2], cols[3], cols[4])
    return (int(cols[0][0]), int(cols[1][0]), float(cols[2][0]), float(cols[3][0]), float(cols[4][0])), cams


def _ragged_args(who, sceneCoordinates, B, shapes, experts):
    """The checks of a ragged batch's sceneCoordinates / shapes / experts before any device is touched.  sceneCoordinates: a list
    of B maps (packed later, on the call's device) or the packed float32 [B,S] tensor of pack_frames.  Returns (E, shapes)."""
    shapes = _shapes_arg(who, shapes, B)
    if experts is not None and (not isinstance(experts, int) or isinstance(experts, bool) or experts < 1):
        raise RuntimeError("%s: experts must be a positive int, found %r" % (who, experts))
    if isinstance(sceneCoordinates, (list, tuple)):
        E, found = _ragged_maps(who, sceneCoordinates)
        if len(found) != B:
            raise RuntimeError("%s: sceneCoordinates holds %d frames, hypAssignment %d" % (who, len(found), B))
        for b in range(B):
            if found[b] != shapes[b]:
                raise RuntimeError("%s: shapes[%d] = %dx%d, sceneCoordinates[%d] is %dx%d" % ((who, b) + shapes[b] + (b,) + found[b]))
        if experts is not None and experts != E:
            raise RuntimeError("%s: experts = %d, sceneCoordinates holds %d experts per frame" % (who, experts, E))
        return E, shapes
    if not isinstance(sceneCoordinates, torch.Tensor) or sceneCoordinates.dtype != torch.float32 or sceneCoordinates.dim() != 2:
        raise RuntimeError("%s: with shapes, sceneCoordinates must be the packed float32 [B,S] tensor of pack_frames or a list of "
                           "float32 [E,3,h,w] maps" % who)
    if sceneCoordinates.size(0) != B:
        raise RuntimeError("%s: batch sizes of sceneCoordinates and hypAssignment differ" % who)
    S, cells = int(sceneCoordinates.size(1)), max(h * w for h, w in shapes)
    if S % 4:
        raise RuntimeError("%s: sceneCoordinates [B,S] needs S to be a multiple of 4 floats, found %d (pack_frames)" % (who, S))
    # pack_frames' S is 3*E*max(h*w) rounded up by at most 3 floats, less than one expert's share: E follows from it
    E = experts if experts is not None else S // (3 * cells)
    if E < 1 or 3 * E * cells > S:
        raise RuntimeError("%s: sceneCoordinates [B,%d] is too short for %d expert(s) on the largest grid of shapes (%d cells)"
                           % (who, S, max(E, 1), cells))
    return E, shapes


def _ragged_call(who, sceneCoordinates, hypAssignment, shapes, experts, cam_args, score_args, want_host):
    """forward_batch / forward_batch_async with shapes: returns (host records or None, device records or None, scores, first call)."""
    B, N = hypAssignment.shape
    if B > MAX_BATCH:
        raise RuntimeError("%s: hypAssignment holds %d frames, at most %d per call" % (who, B, MAX_BATCH))
    E, shapes = _ragged_args(who, sceneCoordinates, B, shapes, experts)
    cam_scalars, cams = _per_frame_cams(who, B, *cam_args)
    eng = _engine_for(sceneCoordinates)
    packed = pack_frames(sceneCoordinates, device=eng.device)[0] if isinstance(sceneCoordinates, (list, tuple)) else sceneCoordinates
    p = _call_params(eng, E, *capacity_shape(shapes), N, cam_scalars, score_args, training=False)
    first = _state["call"]
    scores = torch.empty(B, N, dtype=torch.float64, device=eng.device)
    # (zeros: a frame whose kernels never reach the record write reads RES_VALID = 0 -> EVAL_STATUS 1, not stale memory)
    records = None if want_host else torch.zeros(B, RES_DOUBLES, dtype=torch.float64, device=eng.device)
    res = eng.forward_batch(packed, hypAssignment, p, scores_out=scores, result_out=records, want_host=want_host, cams=cams, shapes=shapes)
    _state["call"] += B  # (behind the call: a table the library refuses -- a frame's camera beyond its own pixel range -- draws no RNG stream)
    return res, records, scores, first


def _shared_call(who, sceneCoordinates, hypAssignment, cam_args, score_args, want_host):
    """forward_batch / forward_batch_async without shapes, from the batch-size check on: returns what _ragged_call returns."""
    B, N = hypAssignment.shape
    if sceneCoordinates.dim() == 5 and sceneCoordinates.size(0) != B:
        raise RuntimeError("%s: batch sizes of sceneCoordinates and hypAssignment differ" % who)
    cam_scalars, cams = _per_frame_cams(who, B, *cam_args)
    eng = _engine_for(sceneCoordinates)
    E, H, W = sceneCoordinates.shape[-4], sceneCoordinates.shape[-2], sceneCoordinates.shape[-1]
    p = _call_params(eng, E, H, W, N, cam_scalars, score_args, training=False)
    first = _state["call"]
    _state["call"] += B  # (ahead of the call: a shared-shape batch draws its B streams even if the library then refuses)
    scores = torch.empty(B, N, dtype=torch.float64, device=eng.device)
    # (zeros, as in _ragged_call)
    records = None if want_host else torch.zeros(B, RES_DOUBLES, dtype=torch.float64, device=eng.device)
    res = eng.forward_batch(sceneCoordinates, hypAssignment, p, scores_out=scores, result_out=records, want_host=want_host, cams=cams)
    return res, records, scores, first


def forward_batch(sceneCoordinates, hypAssignment, outPoses, shiftX, shiftY, focalLength, ppointX, ppointY,
                  inlierThreshold, inlierAlpha, inlierBeta, maxReproj, subSampling, shapes=None, experts=None):
    """Batched companion of `forward` (new API): sceneCoordinates [B,E,3,H,W] (or [E,3,H,W] shared),
    hypAssignment [B,N] int64, outPoses [B,4,4] float32 written in place; returns the list of winning experts.
    Frame b is what the b-th of B consecutive `forward` calls would compute (discrete outputs identical; poses to the rounding of
    the LM sums, bit for bit when the single calls refine with teams of 8 like a batch does: include/esac_hip.h).
    Each of shiftX, shiftY, focalLength, ppointX, ppointY is a scalar (the whole batch) or a length-B sequence / 1-D tensor /
    numpy array (frame b uses element b; test sets whose images differ in focal length).
    shapes: None, or B (h, w) pairs -- a RAGGED batch, frames that differ in image size (esac_hip_forward_batch_shapes):
    sceneCoordinates is then the packed [B,S] tensor of `pack_frames`, or a list of B float32 [E,3,h_b,w_b] maps which is packed
    here; frame b is `forward` on its own maps.  experts: the E of a packed tensor whose S is not pack_frames' own (default:
    S // (3 * the largest h*w)).  Everything else, and every return value, as without shapes."""
    if not isinstance(hypAssignment, torch.Tensor) or hypAssignment.dim() != 2 or hypAssignment.dtype != torch.int64:
        raise RuntimeError("esac.forward_batch: hypAssignment must be int64 [B,N]")
    B = hypAssignment.shape[0]
    cam_args = (shiftX, shiftY, focalLength, ppointX, ppointY)
    score_args = (inlierThreshold, inlierAlpha, inlierBeta, maxReproj, subSampling)
    if shapes is not None:
        if not isinstance(outPoses, torch.Tensor) or outPoses.dtype != torch.float32 or tuple(outPoses.shape) != (B, 4, 4):
            raise RuntimeError("esac.forward_batch: outPoses must be float32 [B,4,4]")
        res, _, scores, _ = _ragged_call("esac.forward_batch", sceneCoordinates, hypAssignment, shapes, experts, cam_args, score_args, True)
    else:
        if experts is not None:
            raise RuntimeError("esac.forward_batch: experts is an argument of a ragged batch (shapes=...)")
        if sceneCoordinates.dtype != torch.float32 or sceneCoordinates.dim() not in (4, 5) or sceneCoordinates.size(-3) != 3:
            raise RuntimeError("esac.forward_batch: sceneCoordinates must be float32 [B,E,3,H,W] or [E,3,H,W]")
        if outPoses.dtype != torch.float32 or tuple(outPoses.shape) != (B, 4, 4):
            raise RuntimeError("esac.forward_batch: outPoses must be float32 [B,4,4]")
        res, _, scores, _ = _shared_call("esac.forward_batch", sceneCoordinates, hypAssignment, cam_args, score_args, True)
    outPoses.copy_(torch.from_numpy(res[:, RES_POSE:RES_POSE + 16].astype(np.float32).reshape(B, 4, 4)))
    _state["last"] = {"scores": scores, "result": res}
    return [int(v) for v in res[:, RES_EXPERT]]


def backward(sceneCoordinates, outGradients, hypAssignment, gtPose, wLossRot, wLossTrans, lossCut, shiftX, shiftY,
             focalLength, ppointX, ppointY, inlierThreshold, inlierAlpha, inlierBeta, maxReproj, subSampling):
    """Drop-in for `esac.backward` (esac.cpp:213-230): expected pose loss over the hypothesis distribution; its
    gradient wrt the scene coordinates is ADDED to `outGradients` in place (esac.cpp:491-508, the caller passes
    zeros: train_esac.py:148). Returns the expected loss as a Python float.

    Tensors may live on the CPU (as train_esac.py:152-155 passes them) or on the GPU; with device tensors nothing
    but the ground-truth pose and the loss value crosses PCIe.
    Pose record (new; the parameter list is the reference's and stays): `set_pose_records(t)` before the call, t a float64 tensor
    [32], CPU or device, filled in place with the forward-format record (RES_*) of the call's argmax hypothesis -- the pose
    `forward` with the same counter returns, refined by the training call itself.  RES_VALID 0 and a NaN pose: the winner's
    probability was below 1e-3 (possible from N > 1000) or nothing was selected."""
    poseRecord = _take_pose_records(None)
    _no_strict_training("esac.backward")
    if sceneCoordinates.dtype != torch.float32 or sceneCoordinates.dim() != 4 or sceneCoordinates.size(1) != 3:
        raise RuntimeError("esac.backward: sceneCoordinates must be float32 [E,3,H,W]")
    if outGradients.dtype != torch.float32 or tuple(outGradients.shape) != tuple(sceneCoordinates.shape):
        raise RuntimeError("esac.backward: outGradients must be float32 and shaped like sceneCoordinates")
    if hypAssignment.dtype != torch.int64 or hypAssignment.dim() != 1 or hypAssignment.numel() == 0:
        raise RuntimeError("esac.backward: hypAssignment must be a non-empty int64 [N]")
    if gtPose.dtype != torch.float32 or tuple(gtPose.shape) != (4, 4):
        raise RuntimeError("esac.backward: gtPose must be float32 [4,4]")
    if poseRecord is not None:
        _check_pose_records("esac.backward", "poseRecord", poseRecord, None, False,
                            sceneCoordinates.device if sceneCoordinates.is_cuda else None)
    eng = _engine_for(sceneCoordinates)
    E, _, H, W = sceneCoordinates.shape
    _check_assignment_range("esac.backward", hypAssignment, E)
    p = _call_params(eng, E, H, W, hypAssignment.shape[0], (shiftX, shiftY, focalLength, ppointX, ppointY),
                     (inlierThreshold, inlierAlpha, inlierBeta, maxReproj, subSampling), training=True)
    _state["call"] += 1
    grads, copy_back = _stage_gradients(outGradients, eng)
    out = eng.backward_device(sceneCoordinates, grads, hypAssignment, gtPose.detach().cpu().numpy(), wLossRot, wLossTrans,
                              lossCut, p, pose_record=poseRecord)
    if copy_back:
        outGradients.copy_(grads)
    _state["last"] = {"backward": out}
    return float(out[0])


def _check_batch_tensors(who, sceneCoordinates, outGradients, hypAssignment, gtPoses, name_each):
    """Types, dtypes and shapes of a batched training call's four tensors; returns B, N, E, H, W.
    name_each: an argument that is no tensor is reported by its name (backward_batch_async), otherwise in one sentence for all
    four (backward_batch)."""
    for name, t in (("sceneCoordinates", sceneCoordinates), ("outGradients", outGradients), ("hypAssignment", hypAssignment),
                    ("gtPoses", gtPoses)):
        if not isinstance(t, torch.Tensor):
            raise RuntimeError("%s: %s must be a torch.Tensor" % (who, name) if name_each else
                               "%s: every tensor argument must be a torch.Tensor" % who)
    if hypAssignment.dtype != torch.int64 or hypAssignment.dim() != 2 or hypAssignment.numel() == 0:
        raise RuntimeError("%s: hypAssignment must be a non-empty int64 [B,N]" % who)
    B, N = hypAssignment.shape
    if sceneCoordinates.dtype != torch.float32 or sceneCoordinates.dim() not in (4, 5) or sceneCoordinates.size(-3) != 3:
        raise RuntimeError("%s: sceneCoordinates must be float32 [B,E,3,H,W] or [E,3,H,W]" % who)
    if sceneCoordinates.dim() == 5 and sceneCoordinates.size(0) != B:
        raise RuntimeError("%s: batch sizes of sceneCoordinates and hypAssignment differ" % who)
    E, H, W = sceneCoordinates.shape[-4], sceneCoordinates.shape[-2], sceneCoordinates.shape[-1]
    if outGradients.dtype != torch.float32 or tuple(outGradients.shape) != (B, E, 3, H, W):
        raise RuntimeError("%s: outGradients must be float32 [B,E,3,H,W]" % who)
    if gtPoses.dtype != torch.float32 or tuple(gtPoses.shape) != (B, 4, 4):
        raise RuntimeError("%s: gtPoses must be float32 [B,4,4]" % who)
    return B, N, E, H, W


def _ragged_backward_args(who, sceneCoordinates, outGradients, hypAssignment, gtPoses, shapes, experts, packed_only):
    """The checks of a ragged training batch's tensors before any device is touched and before the call counter moves.
    outGradients: a packed float32 [B,S'] tensor of pack_frames' row layout, or (blocking call only) a list of B float32
    [E,3,h_b,w_b] tensors.  Returns (B, N, E, shapes); RuntimeError naming the argument otherwise."""
    if not isinstance(hypAssignment, torch.Tensor) or hypAssignment.dtype != torch.int64 or hypAssignment.dim() != 2 or hypAssignment.numel() == 0:
        raise RuntimeError("%s: hypAssignment must be a non-empty int64 [B,N]" % who)
    B, N = hypAssignment.shape
    if B > MAX_BATCH:
        raise RuntimeError("%s: hypAssignment holds %d frames, at most %d per call" % (who, B, MAX_BATCH))
    E, shapes = _ragged_args(who, sceneCoordinates, B, shapes, experts)
    if packed_only and not isinstance(sceneCoordinates, torch.Tensor):
        raise RuntimeError("%s: with shapes, sceneCoordinates must be the packed device tensor of pack_frames (an asynchronous call "
                           "stages nothing)" % who)
    if not isinstance(gtPoses, torch.Tensor) or gtPoses.dtype != torch.float32 or tuple(gtPoses.shape) != (B, 4, 4):
        raise RuntimeError("%s: gtPoses must be float32 [B,4,4]" % who)
    need = 3 * E * max(h * w for h, w in shapes)
    if isinstance(outGradients, (list, tuple)):
        if packed_only:
            raise RuntimeError("%s: with shapes, outGradients must be the packed float32 [B,S] device tensor (an asynchronous call "
                               "cannot copy back into a list)" % who)
        if len(outGradients) != B:
            raise RuntimeError("%s: outGradients holds %d frames, hypAssignment %d" % (who, len(outGradients), B))
        for b, g in enumerate(outGradients):
            if not isinstance(g, torch.Tensor) or g.dtype != torch.float32 or tuple(g.shape) != (E, 3) + shapes[b]:
                raise RuntimeError("%s: outGradients[%d] must be float32 %s" % (who, b, [E, 3] + list(shapes[b])))
    else:
        if not isinstance(outGradients, torch.Tensor) or outGradients.dtype != torch.float32 or outGradients.dim() != 2:
            raise RuntimeError("%s: with shapes, outGradients must be a packed float32 [B,S] tensor%s" %
                               (who, "" if packed_only else " or a list of B float32 [E,3,h,w] tensors"))
        if outGradients.size(0) != B:
            raise RuntimeError("%s: batch sizes of outGradients and hypAssignment differ" % who)
        if outGradients.size(1) < need:
            raise RuntimeError("%s: outGradients [B,%d] is too short for %d expert(s) on the largest grid of shapes (3*E*h*w = %d)"
                               % (who, outGradients.size(1), E, need))
    return int(B), int(N), E, shapes


def _ragged_backward_batch(who, sceneCoordinates, outGradients, hypAssignment, gtPoses, loss_args, cam_args, score_args, shapes,
                           experts, poseRecords):
    B, N, E, shapes = _ragged_backward_args(who, sceneCoordinates, outGradients, hypAssignment, gtPoses, shapes, experts, False)
    some = sceneCoordinates[0] if isinstance(sceneCoordinates, (list, tuple)) else sceneCoordinates
    if poseRecords is not None:
        _check_pose_records(who, "poseRecords", poseRecords, B, False, some.device if some.is_cuda else None)
    _check_assignment_range(who, hypAssignment, E)
    cam_scalars, cams = _per_frame_cams(who, B, *cam_args)
    eng = _engine_for(sceneCoordinates)
    packed = pack_frames(sceneCoordinates, device=eng.device)[0] if isinstance(sceneCoordinates, (list, tuple)) else sceneCoordinates
    p = _call_params(eng, E, *capacity_shape(shapes), N, cam_scalars, score_args, training=True)
    as_list = isinstance(outGradients, (list, tuple))
    if as_list:
        grads, copy_back = pack_frames(list(outGradients), device=eng.device)[0], False
    else:
        grads, copy_back = _stage_gradients(outGradients, eng)
    out = eng.backward_batch_shapes(packed, grads, hypAssignment, gtPoses.detach().cpu().numpy(), *loss_args, p, shapes, cams=cams,
                                    pose_records=poseRecords)
    _state["call"] += B  # (behind the call: a table the library refuses draws no RNG stream)
    if as_list:
        for g, v in zip(outGradients, unpack_frames(grads, shapes, E)):
            g.copy_(v)  # the accumulated tensors back into the caller's
    elif copy_back:
        outGradients.copy_(grads)
    _state["last"] = {"backward": out}
    return [float(v) for v in out[:, 0]]


def backward_batch_shapes(sceneCoordinates, outGradients, hypAssignment, gtPoses, wLossRot, wLossTrans, lossCut, shiftX, shiftY,
                          focalLength, ppointX, ppointY, inlierThreshold, inlierAlpha, inlierBeta, maxReproj, subSampling, *, shapes,
                          experts=None, poseRecords=None):
    """`backward_batch` over a RAGGED batch -- frames that differ in image size (esac_hip_backward_batch_shapes).  shapes (keyword
    only, required): B (h, w) pairs.  sceneCoordinates is the packed [B,S] tensor of `pack_frames` or a list of B float32
    [E,3,h_b,w_b] maps; outGradients a packed float32 [B,S'] tensor of the same row layout (frame b's gradients dense at the head of
    row b: `unpack_frames`), or a list of B float32 [E,3,h_b,w_b] tensors, accumulated into and copied back.  Frame b is `backward`
    on its own maps with counter call + b.  experts: the E of a packed tensor, as in forward_batch.  Everything else, and the
    return value, as `backward_batch`; the call counter advances by B behind the call (a refused table draws no RNG stream).
    A function of its own, like the C entry point: the parameter lists of `backward_batch` and `backward_batch_async` stay as they are."""
    poseRecords = _take_pose_records(poseRecords)
    _no_strict_training("esac.backward_batch_shapes")
    return _ragged_backward_batch("esac.backward_batch_shapes", sceneCoordinates, outGradients, hypAssignment, gtPoses,
                                  (wLossRot, wLossTrans, lossCut), (shiftX, shiftY, focalLength, ppointX, ppointY),
                                  (inlierThreshold, inlierAlpha, inlierBeta, maxReproj, subSampling), shapes, experts, poseRecords)


def backward_batch_shapes_async(sceneCoordinates, outGradients, hypAssignment, gtPoses, wLossRot, wLossTrans, lossCut, shiftX, shiftY,
                                focalLength, ppointX, ppointY, inlierThreshold, inlierAlpha, inlierBeta, maxReproj, subSampling, *, shapes,
                                experts=None, poseRecords=None):
    """`backward_batch_async` over a RAGGED batch (esac_hip_backward_batch_dev_shapes): shapes and experts as in
    `backward_batch_shapes`; sceneCoordinates and outGradients are the packed DEVICE tensors (no lists: nothing is staged or copied
    back).  Everything else, and the return value, as `backward_batch_async`."""
    who = "esac.backward_batch_shapes_async"
    poseRecords = _take_pose_records(poseRecords)
    _no_strict_training(who)
    B, N, E, shapes = _ragged_backward_args(who, sceneCoordinates, outGradients, hypAssignment, gtPoses, shapes, experts, True)
    if poseRecords is not None:
        _check_pose_records(who, "poseRecords", poseRecords, B, True, sceneCoordinates.device if sceneCoordinates.is_cuda else None)
    cam_scalars, cams = _per_frame_cams(who, B, shiftX, shiftY, focalLength, ppointX, ppointY)
    _check_async_tensors(who, sceneCoordinates, outGradients, hypAssignment, gtPoses, "stages nothing on the host")
    eng = engine(sceneCoordinates.device.index)
    p = _call_params(eng, E, *capacity_shape(shapes), N, cam_scalars, (inlierThreshold, inlierAlpha, inlierBeta, maxReproj, subSampling),
                     training=True)
    eng.arm_pose_records(poseRecords)
    rec = eng.backward_batch_shapes_async(sceneCoordinates, outGradients, hypAssignment, gtPoses, wLossRot, wLossTrans, lossCut, p, shapes,
                                          cams=cams)
    _state["call"] += B  # (behind the call: a refused table draws no RNG stream)
    _state["last"] = {"backward": rec}
    return rec[:, 0]


def backward_batch(sceneCoordinates, outGradients, hypAssignment, gtPoses, wLossRot, wLossTrans, lossCut, shiftX, shiftY,
                   focalLength, ppointX, ppointY, inlierThreshold, inlierAlpha, inlierBeta, maxReproj, subSampling, *, poseRecords=None):
    """Batched companion of `backward` (new API): sceneCoordinates [B,E,3,H,W] (or [E,3,H,W] shared by all frames),
    outGradients float32 [B,E,3,H,W] accumulated into in place, hypAssignment [B,N] int64, gtPoses [B,4,4] float32.  Returns
    the list of the B expected losses.  Frame b is what the b-th of B consecutive `backward` calls would compute (the same
    hypotheses, slots and losses; the gradient bit for bit when the single calls refine their slots with one workgroup each:
    include/esac_hip.h).  Advances the call counter by B.
    Each of shiftX, shiftY, focalLength, ppointX, ppointY is a scalar (the whole batch) or a length-B sequence / 1-D tensor /
    numpy array: frame b uses element b (a training mini-batch: one random shift and one focal length per image).
    poseRecords (keyword only; or `set_pose_records` before the call): a float64 tensor [B,32], CPU or device, filled in place:
    row b is frame b's record as `backward` describes it.
    Frames that differ in image size: `backward_batch_shapes`."""
    poseRecords = _take_pose_records(poseRecords)
    _no_strict_training("esac.backward_batch")
    B, N, E, H, W = _check_batch_tensors("esac.backward_batch", sceneCoordinates, outGradients, hypAssignment, gtPoses, name_each=False)
    if poseRecords is not None:
        _check_pose_records("esac.backward_batch", "poseRecords", poseRecords, B, False,
                            sceneCoordinates.device if sceneCoordinates.is_cuda else None)
    _check_assignment_range("esac.backward_batch", hypAssignment, E)
    cam_scalars, cams = _per_frame_cams("esac.backward_batch", B, shiftX, shiftY, focalLength, ppointX, ppointY)
    eng = _engine_for(sceneCoordinates)
    p = _call_params(eng, E, H, W, N, cam_scalars, (inlierThreshold, inlierAlpha, inlierBeta, maxReproj, subSampling), training=True)
    _state["call"] += B
    grads, copy_back = _stage_gradients(outGradients, eng)
    out = eng.backward_batch(sceneCoordinates, grads, hypAssignment, gtPoses.detach().cpu().numpy(), wLossRot, wLossTrans,
                             lossCut, p, cams=cams, pose_records=poseRecords)
    if copy_back:
        outGradients.copy_(grads)
    _state["last"] = {"backward": out}
    return [float(v) for v in out[:, 0]]


def backward_batch_async(sceneCoordinates, outGradients, hypAssignment, gtPoses, wLossRot, wLossTrans, lossCut, shiftX, shiftY,
                         focalLength, ppointX, ppointY, inlierThreshold, inlierAlpha, inlierBeta, maxReproj, subSampling, *,
                         poseRecords=None):
    """`backward_batch` without a host round trip (esac_hip_backward_batch_dev): the call returns once its launches are enqueued on
    torch's current stream and reads its inputs in stream order, so the networks that produce them may still be running and the
    autograd backward can be enqueued behind it at once.  sceneCoordinates, hypAssignment and a contiguous outGradients must be
    device tensors (an asynchronous call cannot copy back into host or strided storage); gtPoses float32 [B,4,4] on the device,
    or on the host (uploaded asynchronously).  Returns the [B] DEVICE tensor of expected losses (float64; column 0 of the
    record); last_result()["backward"] holds the [B,4] device record.  A singular ground-truth pose or an out-of-range
    assignment is a per-frame outcome (record[b,3] = 2 / 1, engine().check() raises after a synchronisation).
    Advances the call counter by B.  The camera arguments are host values, as in backward_batch.
    poseRecords (keyword only; or `set_pose_records` before the call): a contiguous DEVICE float64 tensor [B,32], written in
    stream order: row b is frame b's record as `backward` describes it (RES_VALID 0 for a frame with a singular ground truth);
    `eval_batch` may be enqueued right behind the call.
    Frames that differ in image size: `backward_batch_shapes_async`."""
    who = "esac.backward_batch_async"
    poseRecords = _take_pose_records(poseRecords)
    _no_strict_training(who)
    B, N, E, H, W = _check_batch_tensors(who, sceneCoordinates, outGradients, hypAssignment, gtPoses, name_each=True)
    if poseRecords is not None:
        _check_pose_records(who, "poseRecords", poseRecords, B, True, sceneCoordinates.device if sceneCoordinates.is_cuda else None)
    cam_scalars, cams = _per_frame_cams(who, B, shiftX, shiftY, focalLength, ppointX, ppointY)
    _check_async_tensors(who, sceneCoordinates, outGradients, hypAssignment, gtPoses, "cannot copy back into host storage")
    eng = engine(sceneCoordinates.device.index)
    p = _call_params(eng, E, H, W, N, cam_scalars, (inlierThreshold, inlierAlpha, inlierBeta, maxReproj, subSampling), training=True)
    _state["call"] += B
    eng.arm_pose_records(poseRecords)
    rec = eng.backward_batch_async(sceneCoordinates, outGradients, hypAssignment, gtPoses, wLossRot, wLossTrans, lossCut, p, cams=cams)
    _state["last"] = {"backward": rec}
    return rec[:, 0]


# ---------------------------------------------------------------- the batched test loop (asynchronous forward + on-device figures)
def _check_eval_args(who, records, gtPoses, gtExperts, rotThreshold, transThreshold):
    """Types, dtypes, shapes and batch sizes of an eval_batch call; returns B.  Raises RuntimeError naming the argument; touches
    no device."""
    if not isinstance(records, torch.Tensor):
        raise RuntimeError("%s: records must be a torch.Tensor (the device records of a forward batch)" % who)
    if records.dtype != torch.float64:
        raise RuntimeError("%s: expected scalar type torch.float64 for records but found %s" % (who, records.dtype))
    if records.dim() != 2 or records.size(1) != RES_DOUBLES or records.size(0) < 1:
        raise RuntimeError("%s: records must be [B,%d], found %s" % (who, RES_DOUBLES, tuple(records.shape)))
    B = int(records.size(0))
    if B > MAX_BATCH:
        raise RuntimeError("%s: records hold %d frames, at most %d per call" % (who, B, MAX_BATCH))
    if isinstance(gtPoses, torch.Tensor):
        if gtPoses.dtype != torch.float32:
            raise RuntimeError("%s: expected scalar type torch.float32 for gtPoses but found %s" % (who, gtPoses.dtype))
        shape = tuple(gtPoses.shape)
    else:
        try:
            shape = tuple(np.asarray(gtPoses, np.float32).shape)
        except (TypeError, ValueError):
            raise RuntimeError("%s: gtPoses must be a tensor or an array of B 4x4 poses" % who)
    if shape != (B, 4, 4):
        raise RuntimeError("%s: gtPoses must be [B,4,4] with B = %d (records), found %s" % (who, B, shape))
    if gtExperts is not None:
        if isinstance(gtExperts, torch.Tensor):
            if gtExperts.dtype != torch.int64:
                raise RuntimeError("%s: expected scalar type torch.int64 for gtExperts but found %s" % (who, gtExperts.dtype))
            shape = tuple(gtExperts.shape)
        else:
            try:
                arr = np.asarray(gtExperts)
            except (TypeError, ValueError):
                raise RuntimeError("%s: gtExperts must be a tensor or a sequence of B integers" % who)
            if arr.dtype.kind not in "iu":
                raise RuntimeError("%s: gtExperts must hold integers, found dtype %s" % (who, arr.dtype))
            shape = tuple(arr.shape)
        if shape != (B,):
            raise RuntimeError("%s: gtExperts must be [B] with B = %d (records), found %s" % (who, B, shape))
    for name, v in (("rotThreshold", rotThreshold), ("transThreshold", transThreshold)):
        try:
            v = float(v)
        except (TypeError, ValueError):
            raise RuntimeError("%s: %s must be a number" % (who, name))
        if not (v >= 0.0 and v != float("inf")):
            raise RuntimeError("%s: %s must be finite and not negative, found %r" % (who, name, v))
    # (last: every other argument is judged the same way wherever the tensors live)
    if not records.is_cuda or not records.is_contiguous():
        raise RuntimeError("%s: records must be a dense device tensor (what forward_batch_async returns)" % who)
    return B


def eval_batch(records, gtPoses, gtExperts=None, rotThreshold=5.0, transThreshold=5.0):
    """The numbers the test loop reports (test_esac.py:209-247) for the B frames of a forward batch, computed on the device
    (esac_hip_eval_batch): records = the device tensor of `forward_batch_async`, gtPoses float32 [B,4,4], gtExperts int64 [B] or
    None (host values are uploaded asynchronously).  Enqueued on torch's current stream behind the batch; no host synchronisation.
    Returns a device float64 tensor [B,16]: EVAL_ROT_DEG, EVAL_TRANS_CM, EVAL_POSE_OK (strictly below both thresholds, cm / degrees),
    EVAL_CLASS_OK (-1 without gtExperts), EVAL_QUAT qw qx qy qz and EVAL_INV_T tx ty tz of the inverted pose (one line of
    poses_esac_*.txt), EVAL_EXPERT, EVAL_HYP, EVAL_STATUS (0 a record; 3 the frame's refinement team timed out: run it again,
    harness.rerun_frames; 1 no record)."""
    _check_eval_args("esac.eval_batch", records, gtPoses, gtExperts, rotThreshold, transThreshold)
    return engine(records.device.index).eval_batch(records, gtPoses, gtExperts, rotThreshold, transThreshold)


# ---------------------------------------------------------------- pose verification
def _check_verify_args(who, sceneCoordinates, poses, experts, shapes=None, out=None):
    """Types, dtypes and shapes of a verify_batch call; returns (B, K, pose format).  Raises RuntimeError naming the argument;
    touches no device."""
    if not isinstance(poses, torch.Tensor):
        raise RuntimeError("%s: poses must be a torch.Tensor (float64 [B,K,6] or float32 [B,K,4,4])" % who)
    if poses.dtype == torch.float64 and poses.dim() == 3 and poses.size(2) == 6:
        fmt = VERIFY_POSE_RT
    elif poses.dtype == torch.float32 and poses.dim() == 4 and tuple(poses.shape[2:]) == (4, 4):
        fmt = VERIFY_POSE_4X4
    else:
        raise RuntimeError("%s: poses must be float64 [B,K,6] (rvec | tvec) or float32 [B,K,4,4] (camera poses), found %s %s"
                           % (who, poses.dtype, list(poses.shape)))
    B, K = int(poses.size(0)), int(poses.size(1))
    if B < 1 or B > MAX_BATCH:
        raise RuntimeError("%s: poses hold %d frames, 1 to %d per call" % (who, B, MAX_BATCH))
    if K < 1 or K > VERIFY_MAX_POSES:
        raise RuntimeError("%s: poses hold %d poses per frame, 1 to %d per call" % (who, K, VERIFY_MAX_POSES))
    if isinstance(experts, torch.Tensor):
        if experts.dtype not in (torch.int32, torch.int64):
            raise RuntimeError("%s: expected scalar type torch.int32 or torch.int64 for experts but found %s" % (who, experts.dtype))
        shape = tuple(experts.shape)
    else:
        try:
            arr = np.asarray(experts)
        except (TypeError, ValueError):
            raise RuntimeError("%s: experts must be a tensor or a sequence of integers" % who)
        if arr.dtype.kind not in "iu":
            raise RuntimeError("%s: experts must hold integers, found dtype %s" % (who, arr.dtype))
        shape = tuple(arr.shape)
    if shape != (B, K) and shape != (B,):
        raise RuntimeError("%s: experts must be [B,K] = [%d,%d] (poses) or [B], found %s" % (who, B, K, list(shape)))
    if not isinstance(sceneCoordinates, torch.Tensor) or sceneCoordinates.dtype != torch.float32:
        raise RuntimeError("%s: sceneCoordinates must be a float32 tensor" % who)
    if shapes is None:
        if sceneCoordinates.dim() not in (4, 5) or sceneCoordinates.size(-3) != 3:
            raise RuntimeError("%s: sceneCoordinates must be float32 [B,E,3,H,W] or [E,3,H,W], found %s" % (who, list(sceneCoordinates.shape)))
        if sceneCoordinates.dim() == 5 and sceneCoordinates.size(0) != B:
            raise RuntimeError("%s: batch sizes of sceneCoordinates (%d) and poses (%d) differ" % (who, sceneCoordinates.size(0), B))
    else:
        _shapes_arg(who, shapes, B)
        if sceneCoordinates.dim() != 2 or sceneCoordinates.size(0) != B:
            raise RuntimeError("%s: with shapes, sceneCoordinates must be the packed [B,S] tensor (pack_frames), found %s"
                               % (who, list(sceneCoordinates.shape)))
    if out is not None and not (isinstance(out, torch.Tensor) and out.is_cuda and out.is_contiguous() and out.dtype == torch.float64
                                and tuple(out.shape) == (B, K, VERIFY_DOUBLES)):
        raise RuntimeError("%s: out must be a dense float64 device tensor [B,K,%d] = [%d,%d,%d]" % (who, VERIFY_DOUBLES, B, K, VERIFY_DOUBLES))
    return B, K, fmt


def verify_batch(sceneCoordinates, poses, experts, shiftX, shiftY, focalLength, ppointX, ppointY, inlierThreshold, inlierAlpha,
                 inlierBeta, maxReproj, subSampling, shapes=None, out=None):
    """How well do the scene-coordinate maps support GIVEN poses, and how certain are they (esac_hip_verify_batch)?
    sceneCoordinates float32 [B,E,3,H,W] or [E,3,H,W] (shared by all frames); with shapes (B (h, w) pairs: a ragged batch) the
    packed [B,S] tensor of `pack_frames` or a list of B [E,3,h_b,w_b] maps.  poses: float64 [B,K,6], rvec | tvec scene -> camera
    (RES_RVEC of a record, BUF_HYPS), or float32 [B,K,4,4], camera poses as outPose / gtPoses carry them (inverted on the device);
    experts int32 / int64 [B,K], or [B] for all K poses of a frame.  The five camera arguments are scalars or length-B sequences,
    as in forward_batch; the score parameters are forward's.  Honours set_strict_reference (a non-finite cell: NaN score).
    Enqueued on torch's current stream -- right behind a forward_batch_async whose records it may read --; nothing is waited for;
    host poses / experts are uploaded asynchronously.  Draws no RNG stream: the call counter stays.
    Returns a device float64 [B,K,64] (`out` when given): VERIFY_SCORE (what RES_SCORE holds for the winner), VERIFY_N (cells with
    err < tau, the refinement's rule) and over those cells VERIFY_SSE, VERIFY_A (21 upper-triangle sums of J^T J, row-major, d /
    d(rvec, tvec)), VERIFY_SIGMA2 = SSE / (2n - 6), VERIFY_C (6x6 covariance sigma^2 A^-1, row-major); VERIFY_STATUS: VERIFY_OK,
    VERIFY_FEW (n < 4: sigma^2 and C are NaN), VERIFY_PINV (rank-deficient A: pseudo-inverse), VERIFY_BAD_POSE (not finite, or a
    singular 4x4) and VERIFY_BAD_EXPERT (outside [0,E)): every figure of that row is NaN, the other rows are unaffected."""
    who = "esac.verify_batch"
    if isinstance(sceneCoordinates, (list, tuple)):
        if shapes is None:
            raise RuntimeError("%s: a list of maps is a ragged batch: shapes is required" % who)
        if not isinstance(poses, torch.Tensor) or poses.dim() < 2:
            raise RuntimeError("%s: poses must be a torch.Tensor (float64 [B,K,6] or float32 [B,K,4,4])" % who)
        E, shapes = _ragged_args(who, sceneCoordinates, int(poses.size(0)), shapes, None)
        B, K, _ = _check_verify_args(who, torch.empty((int(poses.size(0)), 0), dtype=torch.float32), poses, experts, shapes, out)
    else:
        B, K, _ = _check_verify_args(who, sceneCoordinates, poses, experts, shapes, out)
        if shapes is not None:
            E, shapes = _ragged_args(who, sceneCoordinates, B, shapes, None)
        else:
            E = int(sceneCoordinates.shape[-4])
    (shiftX, shiftY, focalLength, ppointX, ppointY), cams = _per_frame_cams(who, B, shiftX, shiftY, focalLength, ppointX, ppointY)
    eng = _engine_for(sceneCoordinates, poses)
    if isinstance(sceneCoordinates, (list, tuple)):
        sceneCoordinates, _ = pack_frames(sceneCoordinates, device=eng.device)
    H, W = capacity_shape(shapes) if shapes is not None else (int(sceneCoordinates.shape[-2]), int(sceneCoordinates.shape[-1]))
    shape_before = eng._shape
    p = eng.make_params(E, H, W, K, shiftX, shiftY, focalLength, ppointX, ppointY, inlierThreshold, inlierAlpha, inlierBeta, maxReproj,
                        subSampling, strict_reference=_state["strict_reference"])
    eng._shape = shape_before  # (read_forward_frames keeps reading the last forward call's buffers)
    return eng.verify_batch(sceneCoordinates, poses, experts, p, cams=cams, shapes=shapes, out=out)


def forward_batch_async(sceneCoordinates, hypAssignment, shiftX, shiftY, focalLength, ppointX, ppointY,
                        inlierThreshold, inlierAlpha, inlierBeta, maxReproj, subSampling, shapes=None, experts=None):
    """`forward_batch` without the host inside the call: the launches are enqueued on torch's current stream, the result records
    stay on the device and nothing is waited for (device inputs; host tensors are uploaded first).  Arguments as forward_batch,
    minus outPoses.  Returns dict(records = device float64 [B,32] -- RES_VALID 1: a record, 3: the frame's refinement team timed
    out, run it again as a blocking call with refine_solo at call + b (harness.rerun_frames) --, scores = device float64 [B,N],
    call = the call counter of frame 0, seed); last_result() returns the same dict.  Advances the call counter by B.
    shapes, experts: a ragged batch, as in forward_batch."""
    who = "esac.forward_batch_async"
    if not isinstance(hypAssignment, torch.Tensor) or hypAssignment.dim() != 2 or hypAssignment.dtype != torch.int64 or hypAssignment.numel() == 0:
        raise RuntimeError("%s: hypAssignment must be a non-empty int64 [B,N]" % who)
    cam_args = (shiftX, shiftY, focalLength, ppointX, ppointY)
    score_args = (inlierThreshold, inlierAlpha, inlierBeta, maxReproj, subSampling)
    if shapes is not None:
        _, records, scores, first = _ragged_call(who, sceneCoordinates, hypAssignment, shapes, experts, cam_args, score_args, False)
    else:
        if experts is not None:
            raise RuntimeError("%s: experts is an argument of a ragged batch (shapes=...)" % who)
        if not isinstance(sceneCoordinates, torch.Tensor) or sceneCoordinates.dtype != torch.float32 or sceneCoordinates.dim() not in (4, 5) \
                or sceneCoordinates.size(-3) != 3:
            raise RuntimeError("%s: sceneCoordinates must be float32 [B,E,3,H,W] or [E,3,H,W]" % who)
        if hypAssignment.shape[0] > MAX_BATCH:
            raise RuntimeError("%s: hypAssignment holds %d frames, at most %d per call" % (who, hypAssignment.shape[0], MAX_BATCH))
        _, records, scores, first = _shared_call(who, sceneCoordinates, hypAssignment, cam_args, score_args, False)
    _state["last"] = {"records": records, "scores": scores, "call": first, "seed": _state["seed"]}
    return _state["last"]
