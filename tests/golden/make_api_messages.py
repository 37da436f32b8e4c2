"""Records what the batched calls of an `esac_amd/api.py` answer to bad arguments: exception type, exact sentence, and
whether the call counter moved.  `tests/test_api_messages_frozen.py` holds the current api.py to the recording made from the
commit BEFORE the front end was taken apart into helpers (api_messages.json beside this file).

    git show <commit>:esac_amd/api.py > /tmp/api_then.py
    python tests/golden/make_api_messages.py /tmp/api_then.py > tests/golden/api_messages.json

The api.py given by path is loaded as a module of the esac_amd package (its relative imports resolve against the tree's
package); `engine` is replaced by a function that raises, so nothing here needs or touches a device.

A case = one call with valid host arguments, then one or two of them spoiled.  Singles cover every variant of every check that
runs before a device is opened; pairs spoil two arguments at once (one representative per check) and so pin which of two
failing checks is reported first."""
import importlib.util
import itertools
import json
import os
import sys

import numpy as np
import torch

B, E, N, H, W, K = 2, 2, 4, 4, 4, 3
SHAPES = [(4, 4), (3, 5)]
CAM = dict(shiftX=0, shiftY=0, focalLength=525.0, ppointX=2.0, ppointY=2.0)
SCORE = dict(inlierThreshold=10.0, inlierAlpha=100.0, inlierBeta=0.5, maxReproj=100.0, subSampling=8)
LOSS = dict(wLossRot=1.0, wLossTrans=1.0, lossCut=100.0)
FIRST_CALL = 1000
TOUCHED = "the call touched the device"


def load_api(path):
    root = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    if root not in sys.path:
        sys.path.insert(0, root)
    spec = importlib.util.spec_from_file_location("esac_amd._api_recorded", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _maps():
    return [torch.zeros(E, 3, h, w) for h, w in SHAPES]


def _poses():
    return torch.eye(4).repeat(B, 1, 1)


def _base(api, key):
    """(function name, valid host arguments) of one call form."""
    fn, _, form = key.partition("+")
    ha = torch.zeros(B, N, dtype=torch.int64)
    dense = torch.zeros(B, E, 3, H, W)
    packed = api.pack_frames(_maps(), device="cpu")[0]
    if form == "shapes":
        sc, ragged = packed, dict(shapes=list(SHAPES))
    elif form == "lists":
        sc, ragged = _maps(), dict(shapes=list(SHAPES))
    else:
        sc, ragged = dense, {}
    if fn == "forward_batch":
        return fn, dict(sceneCoordinates=sc, hypAssignment=ha, outPoses=torch.zeros(B, 4, 4), **CAM, **SCORE, **ragged)
    if fn == "forward_batch_async":
        return fn, dict(sceneCoordinates=sc, hypAssignment=ha, **CAM, **SCORE, **ragged)
    if fn == "backward":
        return fn, dict(sceneCoordinates=dense[0], outGradients=torch.zeros(E, 3, H, W), hypAssignment=ha[0], gtPose=torch.eye(4),
                        **LOSS, **CAM, **SCORE)
    if fn in ("backward_batch", "backward_batch_async"):
        return fn, dict(sceneCoordinates=dense, outGradients=torch.zeros(B, E, 3, H, W), hypAssignment=ha, gtPoses=_poses(),
                        **LOSS, **CAM, **SCORE)
    if fn in ("backward_batch_shapes", "backward_batch_shapes_async"):
        grads = _maps() if form == "lists" else torch.zeros_like(packed)
        return fn, dict(sceneCoordinates=sc, outGradients=grads, hypAssignment=ha, gtPoses=_poses(), **LOSS, **CAM, **SCORE, **ragged)
    if fn == "verify_batch":
        return fn, dict(sceneCoordinates=sc, poses=torch.zeros(B, K, 6, dtype=torch.float64), experts=torch.zeros(B, K, dtype=torch.int64),
                        **CAM, **SCORE, **ragged)
    if fn == "eval_batch":
        return fn, dict(records=torch.zeros(B, 32, dtype=torch.float64), gtPoses=_poses(), gtExperts=torch.zeros(B, dtype=torch.int64))
    raise KeyError(key)


KEYS = ["forward_batch", "forward_batch+shapes", "forward_batch+lists", "forward_batch_async", "forward_batch_async+shapes",
        "forward_batch_async+lists", "backward", "backward_batch", "backward_batch_async", "backward_batch_shapes+shapes",
        "backward_batch_shapes+lists", "backward_batch_shapes_async+shapes", "verify_batch", "verify_batch+shapes",
        "verify_batch+lists", "eval_batch"]


def _grow(t):
    """One frame more than the call's other arguments hold (a tensor, or a list of per-frame tensors)."""
    return t + t[:1] if isinstance(t, list) else torch.cat([t, t[:1]])


def _other_dtype(t):
    return t.to(torch.float64 if t.dtype == torch.float32 else torch.int32 if t.dtype == torch.int64 else torch.float32)


# (label, argument, new value from the valid arguments).  Arguments that begin with "_" are steps before the call:
# _armed -> set_pose_records(value), _strict_reference -> set_strict_reference(True).
def _tensor_mutations(name, t):
    muts = [("no-tensor", name, lambda a: (np.zeros((2, 2), np.float32) if not isinstance(a[name], list) else "maps")),
            ("grown", name, lambda a: _grow(a[name]))]
    if isinstance(t, torch.Tensor):
        muts += [("dtype", name, lambda a: _other_dtype(a[name])), ("rank+1", name, lambda a: a[name][None]),
                 ("rank-1", name, lambda a: a[name][0]), ("empty", name, lambda a: a[name][:0])]
        if t.dim() >= 2:
            muts.append(("strided", name, lambda a: torch.cat([a[name], a[name]], -1)[..., ::2]))
    else:
        muts += [("item-dtype", name, lambda a: [a[name][0].double()] + a[name][1:]),
                 ("item-rank", name, lambda a: [a[name][0][0]] + a[name][1:]),
                 ("item-experts", name, lambda a: a[name][:1] + [torch.zeros(E + 1, 3, *SHAPES[1])]),
                 ("item-grid", name, lambda a: a[name][:1] + [torch.zeros(E, 3, 5, 3)]),
                 ("empty", name, lambda a: [])]
    return muts


def _cam_mutations():
    muts = []
    for name, v in CAM.items():
        muts += [("non-finite", name, lambda a, v=v: [v, float("nan")]), ("non-integer", name, lambda a, v=v: [v, 0.5]),
                 ("non-positive", name, lambda a, v=v: [v, -1.0]), ("zero", name, lambda a, v=v: torch.tensor([0.0, v])),
                 ("length", name, lambda a, v=v: np.full(B + 1, v)), ("2-d", name, lambda a, v=v: np.full((B, 1), v)),
                 ("text", name, lambda a: ["a", "b"]), ("no-number", name, lambda a: None),
                 ("beyond-int32", name, lambda a, v=v: [v, 2.0 ** 40])]
    return muts


def _shapes_mutations():
    return [("length", "shapes", lambda a: SHAPES + [(4, 4)]), ("no-list", "shapes", lambda a: 5),
            ("tensor-length", "shapes", lambda a: torch.tensor(SHAPES[:1])), ("no-pair", "shapes", lambda a: [SHAPES[0], (3, 5, 1)]),
            ("no-integer", "shapes", lambda a: [SHAPES[0], (3.5, 5)]), ("text", "shapes", lambda a: [SHAPES[0], "ab"]),
            ("too-small", "shapes", lambda a: [SHAPES[0], (2, 9)]), ("too-large", "shapes", lambda a: [SHAPES[0], (3, 70000)]),
            ("other-grid", "shapes", lambda a: [SHAPES[0], (5, 3)]), ("larger-grid", "shapes", lambda a: [SHAPES[0], (6, 6)])]


def _mutations(api, key):
    """(every single mutation of this call form, the one representative per check that the pairs are made of)."""
    fn, args = _base(api, key)
    singles, reps = [], []

    def add(muts, rep_labels):
        singles.extend(muts)
        reps.extend(m for m in muts if m[0] in rep_labels)

    for name, v in args.items():
        if isinstance(v, torch.Tensor) or (isinstance(v, list) and name != "shapes"):
            add(_tensor_mutations(name, v), ("dtype", "item-dtype") + (("grown",) if name == "hypAssignment" else ()))
    # (one function judges the cameras of every call: each call gets the three per-frame faults, forward_batch every variant)
    cams = [m for m in _cam_mutations() if m[1] in args and (key == "forward_batch" or m[0] in ("non-finite", "non-integer", "non-positive"))]
    singles.extend(cams)
    reps.extend(m for m in cams if (m[1], m[0]) in (("shiftX", "non-finite"), ("shiftY", "non-integer"), ("focalLength", "non-positive"),
                                                     ("ppointX", "length"), ("ppointY", "text")))
    if "shapes" in args:
        add(_shapes_mutations(), ("length", "too-small"))
        if isinstance(args["sceneCoordinates"], torch.Tensor):
            add([("too-short", "sceneCoordinates", lambda a: a["sceneCoordinates"][:, :8].contiguous()),
                 ("S%4", "sceneCoordinates", lambda a: a["sceneCoordinates"][:, :-1])], ("too-short",))
        if isinstance(args.get("outGradients"), torch.Tensor):
            add([("too-short", "outGradients", lambda a: a["outGradients"][:, :8])], ("too-short",))
        if fn.endswith("_async") and fn.startswith("backward"):
            add([("lists", "sceneCoordinates", lambda a: _maps()), ("lists", "outGradients", lambda a: _maps())], ())
    elif fn in ("forward_batch", "forward_batch_async", "verify_batch"):
        add([("no-shapes", "sceneCoordinates", lambda a: _maps())], ())
    if fn in ("forward_batch", "forward_batch_async", "backward_batch_shapes", "backward_batch_shapes_async"):
        add([("zero", "experts", lambda a: 0), ("bool", "experts", lambda a: True), ("float", "experts", lambda a: 2.0),
             ("other", "experts", lambda a: E + 1), ("same", "experts", lambda a: E)], ("zero", "other"))
    if "hypAssignment" in args:
        add([("above-range", "hypAssignment", lambda a: a["hypAssignment"] + E), ("below-range", "hypAssignment", lambda a: a["hypAssignment"] - 1),
             ("max-batch", "hypAssignment", lambda a: torch.zeros(1025, N, dtype=torch.int64))], ("above-range", "max-batch"))
    if fn == "verify_batch":
        add([("4x4", "poses", lambda a: torch.zeros(B, K, 4, 4)), ("4x4-float64", "poses", lambda a: torch.zeros(B, K, 4, 4, dtype=torch.float64)),
             ("max-batch", "poses", lambda a: torch.zeros(1025, 1, 6, dtype=torch.float64)),
             ("max-poses", "poses", lambda a: torch.zeros(B, 1025, 6, dtype=torch.float64)),
             ("per-frame", "experts", lambda a: [0] * B), ("floats", "experts", lambda a: [[0.5] * K] * B), ("text", "experts", lambda a: "ab"),
             ("no-tensor", "out", lambda a: np.zeros((B, K, 64))), ("host", "out", lambda a: torch.zeros(B, K, 64, dtype=torch.float64))],
            ("max-batch", "floats", "host"))
    if fn == "eval_batch":
        add([("max-batch", "records", lambda a: torch.zeros(1025, 32, dtype=torch.float64)), ("31", "records", lambda a: a["records"][:, :31]),
             ("array", "gtPoses", lambda a: np.zeros((B, 4, 4))), ("array-shape", "gtPoses", lambda a: np.zeros((B, 16))),
             ("text", "gtPoses", lambda a: "ab"), ("list", "gtExperts", lambda a: [0] * B), ("floats", "gtExperts", lambda a: [0.5] * B),
             ("none", "gtExperts", lambda a: None), ("negative", "rotThreshold", lambda a: -1.0), ("inf", "transThreshold", lambda a: float("inf")),
             ("text", "rotThreshold", lambda a: "ab"), ("nan", "transThreshold", lambda a: float("nan"))],
            ("31", "array-shape", "floats", "negative", "inf"))
    if fn.startswith("backward"):
        one = fn == "backward"
        how = "_armed" if one or not fn.startswith("backward_batch") else "poseRecords"
        shape = (32,) if one else (B, 32)
        add([("records-shape", how, lambda a: torch.zeros(B + 1, 32, dtype=torch.float64)),
             ("records-31", how, lambda a: torch.zeros(shape[:-1] + (31,), dtype=torch.float64)),
             ("records-dtype", how, lambda a: torch.zeros(shape)), ("records-no-tensor", how, lambda a: np.zeros(shape)),
             ("records-host", how, lambda a: torch.zeros(shape, dtype=torch.float64)),
             ("records-armed", "_armed", lambda a: torch.zeros(B + 1, 32, dtype=torch.float64)),
             ("strict-reference", "_strict_reference", lambda a: True)], ("records-shape", "strict-reference"))
    return singles, reps


def cases(api):
    """[(id, call form, (mutation, ...)), ...] -- the ids are the keys of the recording."""
    out = []
    for key in KEYS:
        singles, reps = _mutations(api, key)
        # (two spoiled camera arguments meet in one function, the same for every call: paired in each call's first form only)
        first_form = key == [k for k in KEYS if k.partition("+")[0] == key.partition("+")[0]][0]
        # (a list of maps differs from the packed tensor in the checks of that one argument: singles only)
        combos = [(m,) for m in singles] + [p for p in itertools.combinations(reps, 2) if p[0][1] != p[1][1]
                                            and (first_form or not (p[0][1] in CAM and p[1][1] in CAM)) and not key.endswith("+lists")]
        for muts in combos:
            out.append(("%s: %s" % (key, " & ".join("%s=%s" % (m[1], m[0]) for m in muts)), key, muts))
    assert len({c[0] for c in out}) == len(out), "case ids must be unique"
    return out


def run_case(api, key, muts):
    """Makes the call (api.engine must already be the function that raises TOUCHED); returns the case's record."""
    fn, args = _base(api, key)
    new = {m[1]: m[2](args) for m in muts}
    before = {k: new.pop(k) for k in list(new) if k.startswith("_")}
    args.update(new)
    api.set_seed(1305, FIRST_CALL)
    rec = {"type": None, "message": None}
    try:
        if "_strict_reference" in before:
            api.set_strict_reference(True)
        if "_armed" in before:
            api.set_pose_records(before["_armed"])
        getattr(api, fn)(**args)
    except Exception as e:  # noqa: BLE001 -- whatever the call raises is the record
        # the interpreter's own sentences (AttributeError / TypeError of a non-tensor) are no part of the contract: type only
        rec = {"type": type(e).__name__, "message": str(e) if isinstance(e, (RuntimeError, ValueError, AssertionError)) else None}
    finally:
        api.set_strict_reference(False)
        api.set_pose_records(None)
    rec["call_moved"] = api.get_rng_state()[1] - FIRST_CALL
    return rec


def no_device(*a, **k):
    raise AssertionError(TOUCHED)


def record(api):
    """{case id: outcome}; an outcome is "<exception type>: <sentence>" ("<type>: *" where only the type is held)."""
    api.engine = no_device
    out = {}
    for cid, key, muts in cases(api):
        rec = run_case(api, key, muts)
        assert rec["type"] is not None and rec["call_moved"] == 0, (cid, rec)  # every case is an error that drew no RNG stream
        out[cid] = outcome(rec)
    return out


def outcome(rec):
    return "%s: %s" % (rec["type"], "*" if rec["message"] is None else rec["message"])


def dump(recorded, f):
    """The recording grouped by outcome, one outcome per line: {outcome: {call form: [spoiled arguments, ...]}}."""
    grouped = {}
    for cid, what in recorded.items():
        key, _, muts = cid.partition(": ")
        grouped.setdefault(what, {}).setdefault(key, []).append(muts)
    f.write("{\n" + ",\n".join("%s: %s" % (json.dumps(k), json.dumps(grouped[k])) for k in sorted(grouped)) + "\n}\n")


def load(f):
    """The inverse of dump: {case id: outcome}."""
    return {"%s: %s" % (key, muts): what for what, forms in json.load(f).items() for key, all_muts in forms.items() for muts in all_muts}


if __name__ == "__main__":
    dump(record(load_api(sys.argv[1])), sys.stdout)
