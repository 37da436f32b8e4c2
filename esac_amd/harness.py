"""Caller-side glue of the hot path: the evaluation loop of code/test_esac.py:135-289 with every tensor
device-resident.

What changes against the reference loop (and why it matters on MI355X):
  * `prediction = prediction.cpu()` (test_esac.py:187) is gone: the coordinate maps stay in HBM and go straight
    into `esac.forward`; `gating_probs.cpu()` (test_esac.py:164) is gone: `torch.multinomial` / `torch.histc`
    run on the device; only the per-expert activity mask (E booleans) and the result record cross PCIe.
  * experts are evaluated only where the gating drew at least one hypothesis (test_esac.py:178-185), as before.
  * the pose error (test_esac.py:209-217) and the quaternion pose-file line (test_esac.py:230-247) no longer
    need cv2: Rodrigues is a few lines of numpy (cv2 / skimage / torchvision are not installed here).

The expert and gating networks are whatever `nn.Module`s the caller passes (the reference's `Expert` /
`Gating` FCNs stay in PyTorch-ROCm, north_star); the tests drive the loop with synthetic experts that return
the ray-cast maps of esac_amd/synthetic.py, since no datasets or trained weights exist offline.
"""
import math
import time

import numpy as np
import torch

from . import api


def rodrigues_vector(R):
    """Rotation matrix -> axis-angle vector (what cv2.Rodrigues(R)[0] returns), numpy only."""
    R = np.asarray(R, np.float64)
    sk = 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    s = np.linalg.norm(sk)
    c = (np.trace(R) - 1.0) / 2.0
    angle = math.atan2(s, c)
    if s < 1e-12:
        if c > 0:
            return np.zeros(3)
        # angle ~ pi: axis from the diagonal of (R + I) / 2
        d = np.clip((np.diag(R) + 1.0) / 2.0, 0.0, None)
        axis = np.sqrt(d)
        if R[0, 1] < 0:
            axis[1] = -axis[1]
        if R[0, 2] < 0:
            axis[2] = -axis[2]
        return axis / max(np.linalg.norm(axis), 1e-300) * angle
    return sk / s * angle


def pose_errors_deg_cm(out_pose, gt_pose):
    """(rotation error in degrees, translation error in cm) exactly as test_esac.py:209-217 prints them."""
    out_pose = np.asarray(out_pose, np.float64)
    gt_pose = np.asarray(gt_pose, np.float64)
    t_err = float(np.linalg.norm(gt_pose[0:3, 3] - out_pose[0:3, 3]))
    r = rodrigues_vector(out_pose[0:3, 0:3] @ gt_pose[0:3, 0:3].T)
    return float(np.linalg.norm(r) * 180.0 / math.pi), t_err * 100.0


POSE_LINE_FORMAT = "%s %f %f %f %f %f %f %f\n"  # name qw qx qy qz tx ty tz


def pose_file_values(out_pose):
    """(qw, qx, qy, qz, tx, ty, tz) of the INVERTED pose: the seven numbers of a pose-file line (test_esac.py:230-247)."""
    inv = np.linalg.inv(np.asarray(out_pose, np.float64))
    t = inv[0:3, 3]
    rot = rodrigues_vector(inv[0:3, 0:3])
    angle = float(np.linalg.norm(rot))
    axis = rot / angle if angle > 0 else np.array([1.0, 0.0, 0.0])
    q_w = math.cos(angle * 0.5)
    q_xyz = math.sin(angle * 0.5) * axis
    return q_w, q_xyz[0], q_xyz[1], q_xyz[2], float(t[0]), float(t[1]), float(t[2])


def pose_file_line(name, out_pose):
    """One line of poses_esac_<session>.txt: name qw qx qy qz tx ty tz of the INVERTED pose (test_esac.py:230-247)."""
    return POSE_LINE_FORMAT % ((name,) + pose_file_values(out_pose))


def eval_row_host(out_pose, gt_pose, expert, hyp, gt_expert=None, rot_threshold_deg=5.0, trans_threshold_cm=5.0):
    """One row of esac.eval_batch (api.EVAL_*), computed by the host functions above: what the device row is held against, and
    what `rerun_frames` puts in the place of a frame it ran again."""
    row = np.zeros(api.EVAL_DOUBLES, np.float64)
    r_err, t_err = pose_errors_deg_cm(out_pose, gt_pose)
    row[api.EVAL_ROT_DEG], row[api.EVAL_TRANS_CM] = r_err, t_err
    row[api.EVAL_POSE_OK] = float(t_err < trans_threshold_cm and r_err < rot_threshold_deg)
    row[api.EVAL_CLASS_OK] = -1.0 if gt_expert is None else float(int(gt_expert) == int(expert))
    try:
        row[api.EVAL_QUAT:api.EVAL_QUAT + 7] = pose_file_values(out_pose)
    except np.linalg.LinAlgError:  # a singular pose: no inverse to print
        row[api.EVAL_QUAT:api.EVAL_QUAT + 7] = np.nan
    row[api.EVAL_EXPERT], row[api.EVAL_HYP] = float(expert), float(hyp)
    return row


@torch.no_grad()
def localize(image, gating, experts, focal_length, hypotheses=256, threshold=10.0, inlier_alpha=100.0,
             inlier_beta=0.5, max_reprojection=100.0, subsample=8, expert_selection=False, oracle_expert=None,
             generator=None, strict_reference=False):
    """One iteration of the reference test loop (test_esac.py:145-207) for `image` [1,3,H,W] on the GPU.
    strict_reference: this call follows the reference where the default knowingly differs (esac.set_strict_reference).

    gating(image) -> log-probabilities [1,E]; experts[e](image) -> scene coordinates [1,3,H/s,W/s].
    Returns dict(pose [4,4] float32 cpu, expert, active_experts, gating_probs (device), time_s, prediction, hyp_assignment
    -- the two device tensors handed to esac.forward, so a caller can replay the call elsewhere)."""
    dev = image.device
    E = len(experts)
    pp_x = float(image.size(3) / 2)
    pp_y = float(image.size(2) / 2)
    pred_w = math.ceil(image.size(3) / subsample)
    pred_h = math.ceil(image.size(2) / subsample)
    prediction = torch.zeros((E, 3, pred_h, pred_w), device=dev)
    start = time.time()
    gating_probs = torch.exp(gating(image))[0]  # stays on the device (reference: .cpu())
    if oracle_expert is not None:
        gating_probs = torch.zeros_like(gating_probs)
        gating_probs[int(oracle_expert)] = 1
    if expert_selection or oracle_expert is not None:
        expert = torch.multinomial(gating_probs, 1, replacement=True, generator=generator)
        e_hyps = expert.expand((hypotheses,))  # stride-0 view, as in the reference
    else:
        e_hyps = torch.multinomial(gating_probs, hypotheses, replacement=True, generator=generator)
    e_hist = torch.histc(e_hyps.float(), bins=E, min=0, max=E - 1)
    active = (e_hist > 0).cpu().tolist()  # E booleans: the only device->host traffic before the call
    for e, on in enumerate(active):
        if on:
            prediction[e] = experts[e](image)[0]
    out_pose = torch.zeros(4, 4)
    strict_before = api._state["strict_reference"]
    api.set_strict_reference(strict_before or strict_reference)
    try:
        winning_expert = api.forward(prediction, e_hyps, out_pose, 0, 0, float(focal_length), pp_x, pp_y, threshold,
                                     inlier_alpha, inlier_beta, max_reprojection, subsample)
    finally:
        api.set_strict_reference(strict_before)
    return dict(pose=out_pose, expert=winning_expert, active_experts=int(sum(active)), gating_probs=gating_probs,
                time_s=time.time() - start, prediction=prediction, hyp_assignment=e_hyps)


def _focal_list(who, focal_lengths, B):
    """B focal lengths from a number, a sequence, an array or a tensor."""
    focals = [float(f) for f in (focal_lengths.tolist() if isinstance(focal_lengths, (torch.Tensor, np.ndarray)) and
                                 getattr(focal_lengths, "ndim", 0) > 0 else
                                 focal_lengths if isinstance(focal_lengths, (list, tuple)) else [focal_lengths] * B)]
    if len(focals) != B:
        raise RuntimeError("%s: focal_lengths must hold one value per image (%d), found %d" % (who, B, len(focals)))
    return focals


@torch.no_grad()
def localize_batch(images, gating, experts, focal_lengths, gt_poses=None, gt_experts=None, hypotheses=256, threshold=10.0,
                   inlier_alpha=100.0, inlier_beta=0.5, max_reprojection=100.0, subsample=8, e_hyps=None, expert_selection=False,
                   oracle_experts=None, generator=None, asynchronous=False, all_experts=False, strict_reference=False,
                   rot_threshold_deg=5.0, trans_threshold_cm=5.0, verify_gt=False):
    """The test-loop counterpart of `train_batch`: B images of one size through ONE forward batch (`esac.forward_batch_async`) and,
    when `gt_poses` is given, ONE `esac.eval_batch` that turns the records into the loop's figures on the device.

    images [B,3,H,W]; focal_lengths: B numbers (or one for all), they travel as the call's per-frame camera table.
    gating(images) -> log-probabilities [B,E]; experts[e](images) -> [B,3,H/s,W/s].  The gating runs once on the batch, every frame
    gets its own multinomial row (or `e_hyps` [B,N]; expert_selection / oracle_experts: one expert per frame, a stride-0 row), and
    every expert that is active in at least one frame runs once on the batch (rows of frames in which it is inactive are never
    read).  all_experts: every expert runs and the `.cpu()` of the B x E activity flags is skipped.
    gt_poses [B,4,4] and gt_experts [B] (tensors on either side, arrays, lists) feed eval_batch; host values are uploaded
    asynchronously.  strict_reference: as in `localize`.
    verify_gt (needs gt_poses): ONE `esac.verify_batch` (K = 1, the 4x4 format) of the ground-truth poses is enqueued behind the
    forward batch -- on the map of gt_experts[b] when given, else of the winner's expert, read from the device records without a
    host synchronisation -- and the dict gains gt_verify [B,1,64] (device): does the ground truth score higher than the winner
    (VERIFY_SCORE against RES_SCORE: sampling failed), or not (scoring or the expert failed)?
    asynchronous=True with all_experts=True and device inputs: NO host synchronisation in this function; every result stays on
    the device.  A frame whose refinement team timed out then carries EVAL_STATUS / RES_VALID = 3: `frames_to_rerun` finds
    them in the host copy of `eval`, `rerun_frames` runs them again.
    Returns dict(records [B,32] device, scores [B,N] device, eval [B,16] device or None, e_hyps [B,N] device, e_hist [B,E] device,
    prediction [B,E,3,h,w] device, active_experts [B] device, call (frame 0's call counter; frame b ran at call + b), seed, time_s
    and what `rerun_frames` needs).  Not asynchronous: also poses [B,4,4] float32 cpu, experts (list of B ints), records_host,
    eval as a numpy array [B,16] (the device tensor stays under eval_device) and active_experts as a list; frames with status 3
    have been run again already.
    images may also be a LIST of B images [1,3,H_b,W_b] (or [3,H_b,W_b]) of different sizes: a ragged batch (`_localize_ragged`)."""
    if isinstance(images, (list, tuple)):
        return _localize_ragged(list(images), gating, experts, focal_lengths, gt_poses, gt_experts, hypotheses, threshold, inlier_alpha,
                                inlier_beta, max_reprojection, subsample, e_hyps, expert_selection, oracle_experts, generator,
                                asynchronous, all_experts, strict_reference, rot_threshold_deg, trans_threshold_cm, verify_gt)
    dev = images.device
    B, E = int(images.size(0)), len(experts)
    pp_x = float(images.size(3) / 2)
    pp_y = float(images.size(2) / 2)
    pred_w = math.ceil(images.size(3) / subsample)
    pred_h = math.ceil(images.size(2) / subsample)
    focals = _focal_list("localize_batch", focal_lengths, B)
    start = time.time()
    e_hyps = _draw_hyps(lambda: torch.exp(gating(images)), B, dev, e_hyps, hypotheses, expert_selection, oracle_experts, generator)
    e_hist = torch.zeros((B, E), device=dev).scatter_add_(1, e_hyps, torch.ones(e_hyps.shape, device=dev))
    active_count = (e_hist > 0).sum(dim=1)  # [B], device
    if all_experts:
        active_any = [True] * E  # no flags cross to the host: every expert runs
    else:
        active_any = (e_hist > 0).any(dim=0).cpu().tolist()  # E flags: all that reaches the host before the call
    outputs = [experts[e](images) if on else torch.zeros((B, 3, pred_h, pred_w), device=dev) for e, on in enumerate(active_any)]
    prediction = torch.stack(outputs, dim=1)  # [B,E,3,h,w]; rows of inactive experts are never read
    return _solve_batch(prediction, None, e_hyps, e_hist, active_count, focals, pp_x, pp_y, gt_poses, gt_experts, threshold, inlier_alpha,
                        inlier_beta, max_reprojection, subsample, asynchronous, strict_reference, rot_threshold_deg, trans_threshold_cm, start,
                        verify_gt)


def _draw_hyps(gating_probs_of, B, dev, e_hyps, hypotheses, expert_selection, oracle_experts, generator):
    """The hypothesis assignment [B,N] of a batch: the caller's, or one multinomial row per frame from the gating's
    probabilities (gating_probs_of() -> [B,E] on the device; only called when they are needed)."""
    if e_hyps is not None:
        e_hyps = torch.as_tensor(e_hyps, dtype=torch.int64).to(dev)
        if e_hyps.dim() != 2 or e_hyps.size(0) != B:
            raise RuntimeError("localize_batch: e_hyps must be [B,N]")
    else:
        gating_probs = gating_probs_of()  # [B,E], stays on the device
        if oracle_experts is not None:
            oracle = torch.as_tensor(oracle_experts, dtype=torch.int64).reshape(-1)
            if oracle.numel() != B:
                raise RuntimeError("localize_batch: oracle_experts must hold one expert per image (%d), found %d" % (B, oracle.numel()))
            gating_probs = torch.zeros_like(gating_probs).scatter_(1, oracle.to(dev, non_blocking=True).unsqueeze(1), 1.0)
        if expert_selection or oracle_experts is not None:
            expert = torch.multinomial(gating_probs, 1, replacement=True, generator=generator)  # [B,1]
            e_hyps = expert.expand((B, hypotheses))  # stride-0 rows, as in the reference
        else:
            e_hyps = torch.multinomial(gating_probs, hypotheses, replacement=True, generator=generator)  # one row of draws per frame
    return e_hyps


def _solve_batch(prediction, shapes, e_hyps, e_hist, active_count, focals, pp_x, pp_y, gt_poses, gt_experts, threshold, inlier_alpha,
                 inlier_beta, max_reprojection, subsample, asynchronous, strict_reference, rot_threshold_deg, trans_threshold_cm, start,
                 verify_gt=False):
    """The solver half of localize_batch: ONE forward batch, ONE eval_batch, (verify_gt) ONE verify_batch, the result dict.
    shapes: None and prediction [B,E,3,h,w], or the B grids of a ragged batch with prediction the packed [B,S] buffer (pp_x, pp_y
    then hold B values)."""
    B, E = int(e_hyps.shape[0]), int(e_hist.shape[1])
    e_hyps = e_hyps.contiguous()
    strict_before = api._state["strict_reference"]
    strict = bool(strict_before or strict_reference)
    api.set_strict_reference(strict)
    try:
        ragged = {} if shapes is None else dict(shapes=shapes, experts=E)
        fwd = api.forward_batch_async(prediction, e_hyps, 0, 0, focals, pp_x, pp_y, threshold, inlier_alpha, inlier_beta,
                                      max_reprojection, subsample, **ragged)
        gt_verify = None
        if verify_gt:
            if gt_poses is None:
                raise RuntimeError("localize_batch: verify_gt needs gt_poses")
            gt = gt_poses if isinstance(gt_poses, torch.Tensor) else torch.from_numpy(np.asarray(gt_poses, np.float32))
            # the true expert's map, or the winner's: column RES_EXPERT of the device records, in stream order
            on = gt_experts if gt_experts is not None else fwd["records"][:, api.RES_EXPERT].to(torch.int32)
            gt_verify = api.verify_batch(prediction, gt.to(torch.float32).reshape(B, 1, 4, 4), on, 0, 0, focals, pp_x, pp_y, threshold,
                                         inlier_alpha, inlier_beta, max_reprojection, subsample, shapes=shapes)
    finally:
        api.set_strict_reference(strict_before)
    ev = None
    if gt_poses is not None:
        ev = api.eval_batch(fwd["records"], gt_poses, gt_experts, rot_threshold_deg, trans_threshold_cm)
    out = dict(records=fwd["records"], scores=fwd["scores"], eval=ev, e_hyps=e_hyps, e_hist=e_hist, prediction=prediction, shapes=shapes,
               active_experts=active_count, call=fwd["call"], seed=fwd["seed"], focals=focals, gt_poses=gt_poses, gt_experts=gt_experts,
               solver=dict(pp_x=pp_x, pp_y=pp_y, threshold=threshold, inlier_alpha=inlier_alpha, inlier_beta=inlier_beta,
                           max_reprojection=max_reprojection, subsample=subsample, strict_reference=strict,
                           max_tries=api._state["max_tries"], max_ref_steps=api._state["max_ref_steps"],
                           rot_threshold_deg=rot_threshold_deg, trans_threshold_cm=trans_threshold_cm))
    if verify_gt:
        out["gt_verify"] = gt_verify
    if not asynchronous:
        rec = fwd["records"].cpu().numpy()  # the one wait of the blocking form
        out["records_host"] = rec
        out["eval_device"] = ev
        out["eval"] = ev.cpu().numpy() if ev is not None else None
        out["poses"] = torch.from_numpy(rec[:, api.RES_POSE:api.RES_POSE + 16].astype(np.float32).reshape(B, 4, 4))
        out["experts"] = [int(v) for v in rec[:, api.RES_EXPERT]]
        out["active_experts"] = active_count.cpu().tolist()
        again = [int(b) for b in np.flatnonzero(rec[:, api.RES_VALID] == 3.0)]
        if again:
            rerun_frames(out, again)
    out["time_s"] = time.time() - start
    return out


@torch.no_grad()
def _localize_ragged(images, gating, experts, focal_lengths, gt_poses, gt_experts, hypotheses, threshold, inlier_alpha, inlier_beta,
                     max_reprojection, subsample, e_hyps, expert_selection, oracle_experts, generator, asynchronous, all_experts,
                     strict_reference, rot_threshold_deg, trans_threshold_cm, verify_gt=False):
    """localize_batch over images of different sizes (test sets resized by their shorter edge).  The networks run once per group
    of equally sized images and write straight into the packed buffer of a ragged batch (esac.pack_frames' layout: frame b's
    [E,3,h_b,w_b] dense at the head of row b); every frame gets its own principal point (the image centre) and focal length; then
    ONE solver call (`esac.forward_batch_async(shapes=...)`) and ONE `esac.eval_batch` for the whole batch, as with one size.
    The result dict is localize_batch's with prediction = the packed [B,S] buffer and shapes = [(h_b, w_b)]."""
    images = [im if im.dim() == 4 else im.unsqueeze(0) for im in images]
    B, E = len(images), len(experts)
    if B == 0 or any(im.dim() != 4 or im.size(0) != 1 for im in images):
        raise RuntimeError("localize_batch: images must be a [B,3,H,W] tensor or a non-empty list of [1,3,H,W] / [3,H,W] images")
    dev = images[0].device
    focals = _focal_list("localize_batch", focal_lengths, B)
    pp_x = [float(im.size(3) / 2) for im in images]
    pp_y = [float(im.size(2) / 2) for im in images]
    shapes = [(math.ceil(im.size(2) / subsample), math.ceil(im.size(3) / subsample)) for im in images]
    groups = {}  # image size -> frames, in order of first appearance
    for b, im in enumerate(images):
        groups.setdefault(tuple(im.shape[1:]), []).append(b)
    stacked = {key: torch.cat([images[b] for b in members]) for key, members in groups.items()}
    start = time.time()

    def gating_probs():
        probs = torch.zeros((B, E), device=dev)
        for key, members in groups.items():
            probs[torch.as_tensor(members, device=dev)] = torch.exp(gating(stacked[key]))
        return probs

    e_hyps = _draw_hyps(gating_probs, B, dev, e_hyps, hypotheses, expert_selection, oracle_experts, generator)
    e_hist = torch.zeros((B, E), device=dev).scatter_add_(1, e_hyps, torch.ones(e_hyps.shape, device=dev))
    active_count = (e_hist > 0).sum(dim=1)  # [B], device
    active = None if all_experts else (e_hist > 0).cpu().tolist()  # B x E flags: all that reaches the host before the call
    packed = torch.zeros((B, api.packed_stride(E, shapes)), dtype=torch.float32, device=dev)
    for key, members in groups.items():
        h, w = shapes[members[0]]
        for e in range(E):
            if active is not None and not any(active[b][e] for b in members):
                continue  # (rows of inactive experts are never read)
            maps = experts[e](stacked[key])  # [n,3,h,w]
            for i, b in enumerate(members):
                packed[b, :3 * E * h * w].view(E, 3, h, w)[e] = maps[i]
    return _solve_batch(packed, shapes, e_hyps, e_hist, active_count, focals, pp_x, pp_y, gt_poses, gt_experts, threshold, inlier_alpha,
                        inlier_beta, max_reprojection, subsample, asynchronous, strict_reference, rot_threshold_deg, trans_threshold_cm, start,
                        verify_gt)


def frames_to_rerun(eval_host):
    """Indices of the rows of a host copy of `eval` ([n,16]) whose EVAL_STATUS is 3: frames of an asynchronous batch whose
    refinement team timed out (include/esac_hip.h, ESAC_RES_VALID = 3).  A pure function."""
    ev = np.asarray(eval_host, np.float64).reshape(-1, api.EVAL_DOUBLES)
    return [int(i) for i in np.flatnonzero(ev[:, api.EVAL_STATUS] == 3.0)]


def rerun_frames(batch_out, frames):
    """Runs the named frames of a `localize_batch` result again, each as a BLOCKING single call at the frame's own key
    (seed, call + b), with its own camera and the one-workgroup refinement (refine_solo) -- the rule of include/esac_hip.h for a
    record with ESAC_RES_VALID = 3.  The module's call counter is not touched.  Returns {b: dict(record np.float64[32], pose
    [4,4] float32 numpy, expert, eval np.float64[16] or None)}; the eval row is recomputed by the host functions (eval_row_host)
    against the float32 ground truth the device row used.  Host-side entries of `batch_out` (records_host, poses, experts, eval as
    numpy) are updated in place where they exist."""
    pred, e_hyps, s = batch_out["prediction"], batch_out["e_hyps"], batch_out["solver"]
    shapes = batch_out.get("shapes")  # a ragged batch: the frame's own maps, grid and principal point
    B, N = int(e_hyps.shape[0]), int(e_hyps.shape[1])
    E = int(batch_out["e_hist"].shape[1]) if shapes is not None else int(pred.shape[1])
    eng = api.engine(pred.device.index)
    done = {}
    for b in frames:
        b = int(b)
        if not 0 <= b < B:
            raise RuntimeError("rerun_frames: frame %d outside the batch of %d" % (b, B))
        if shapes is not None:
            H, W = shapes[b]
            maps, pp_x, pp_y = pred[b, :3 * E * H * W].view(E, 3, H, W), s["pp_x"][b], s["pp_y"][b]
        else:
            (H, W), maps, pp_x, pp_y = pred.shape[3:], pred[b], s["pp_x"], s["pp_y"]
        p = eng.make_params(E, H, W, N, 0, 0, batch_out["focals"][b], pp_x, pp_y, s["threshold"], s["inlier_alpha"],
                            s["inlier_beta"], s["max_reprojection"], s["subsample"], seed=batch_out["seed"], call=batch_out["call"] + b,
                            max_tries=s["max_tries"], max_ref_steps=s["max_ref_steps"], refine_solo=True,
                            strict_reference=s["strict_reference"])
        rec = eng.forward_device(maps, e_hyps[b], p)
        pose = rec[api.RES_POSE:api.RES_POSE + 16].astype(np.float32).reshape(4, 4)
        row = None
        if batch_out.get("gt_poses") is not None:
            gt = batch_out["gt_poses"][b]
            gt = gt.detach().cpu().numpy() if isinstance(gt, torch.Tensor) else np.asarray(gt)
            ge = batch_out.get("gt_experts")
            ge = None if ge is None else int(ge[b])
            row = eval_row_host(pose, gt.astype(np.float32), int(rec[api.RES_EXPERT]), int(rec[api.RES_HYP]), ge,
                                s["rot_threshold_deg"], s["trans_threshold_cm"])
        done[b] = dict(record=rec, pose=pose, expert=int(rec[api.RES_EXPERT]), eval=row)
        if "records_host" in batch_out:
            batch_out["records_host"][b] = rec
            batch_out["records_host"][b, api.RES_VALID] = 1.0
            batch_out["poses"][b] = torch.from_numpy(pose)
            batch_out["experts"][b] = int(rec[api.RES_EXPERT])
        if isinstance(batch_out.get("eval"), np.ndarray) and row is not None:
            batch_out["eval"][b] = row
    return done


def _statistics(E, scenes_r, scenes_t, scenes_c, trans_threshold_cm, rot_threshold_deg, avg_active, max_active, avg_time, n):
    """The statistics block of test_esac.py:249-289 from the per-scene lists."""
    def median(values):
        if len(values) == 0:
            return 0
        values = sorted(values)
        return values[int(len(values) / 2)]

    rows = []
    for s in range(E):
        class_acc = sum(scenes_c[s]) / max(len(scenes_c[s]), 1)
        ok = [(t < trans_threshold_cm and r < rot_threshold_deg) for t, r in zip(scenes_t[s], scenes_r[s])]
        rows.append(dict(scene=s, class_acc=class_acc, pose_acc=sum(ok) / max(len(ok), 1),
                         median_rot_deg=median(scenes_r[s]), median_trans_cm=median(scenes_t[s])))
    return dict(scenes=rows, avg_active=avg_active / max(n, 1), max_active=max_active, avg_time_s=avg_time / max(n, 1),
                images=n)


def evaluate(samples, gating, experts, trans_threshold_cm=5.0, rot_threshold_deg=5.0, pose_log=None, batch_size=1,
             asynchronous=False, verify_gt=False, **kw):
    """The statistics block of test_esac.py:249-289 over `samples` = iterable of
    (name, image, focal_length, gt_pose [4,4], gt_expert).
    batch_size > 1: batch_size consecutive samples form a batch (the last one may be short) and each batch goes through
    `localize_batch` -- one forward batch and one on-device evaluation instead of batch_size blocking calls with their copies.
    Images of one size are stacked; a batch whose images differ in size is a ragged batch (the networks run per group of equal
    size, the solver once: esac.forward_batch_async(shapes=...)).  The eval rows of all batches are copied to the
    host ONCE, after the last batch; frames whose status is 3 are run again (`rerun_frames`); the statistics and the pose-log lines
    (the format string of `pose_file_line` over the row's quaternion and translation) follow from the rows.  asynchronous: the
    batches are enqueued without a host synchronisation (localize_batch(asynchronous=True, all_experts=True)), given device images.
    `oracle_expert=k` in **kw applies to every image, as with batch_size 1.
    verify_gt: every batch also scores its ground-truth poses on the true experts' maps (localize_batch(verify_gt=True); the frames
    go through the batched route whatever batch_size is) and the result gains gt_score_higher: the share of frames whose ground
    truth scores higher than the winner the solver returned (VERIFY_SCORE > RES_SCORE) -- frames on which the sampling failed, not
    the scoring or the expert."""
    E = len(experts)
    if int(batch_size) > 1 or verify_gt:
        return _evaluate_batched(samples, gating, experts, trans_threshold_cm, rot_threshold_deg, pose_log, max(int(batch_size), 1),
                                 asynchronous, kw, verify_gt)
    scenes_r, scenes_t, scenes_c = [[] for _ in range(E)], [[] for _ in range(E)], [[] for _ in range(E)]
    avg_active = max_active = avg_time = n = 0
    for name, image, focal, gt_pose, gt_expert in samples:
        out = localize(image, gating, experts, focal, **kw)
        r_err, t_err = pose_errors_deg_cm(out["pose"].numpy(), np.asarray(gt_pose))
        scenes_r[gt_expert].append(r_err)
        scenes_t[gt_expert].append(t_err)
        scenes_c[gt_expert].append(int(gt_expert) == out["expert"])
        avg_active += out["active_experts"]
        max_active = max(max_active, out["active_experts"])
        avg_time += out["time_s"]
        n += 1
        if pose_log is not None:
            pose_log.write(pose_file_line(name, out["pose"].numpy()))
    return _statistics(E, scenes_r, scenes_t, scenes_c, trans_threshold_cm, rot_threshold_deg, avg_active, max_active, avg_time, n)


def _evaluate_batched(samples, gating, experts, trans_threshold_cm, rot_threshold_deg, pose_log, batch_size, asynchronous, kw,
                      verify_gt=False):
    E = len(experts)
    kw = dict(kw)
    oracle_expert = kw.pop("oracle_expert", None)
    if asynchronous:
        kw.setdefault("all_experts", True)
    start = time.time()
    batches, names, gt_exp = [], [], []  # per batch: its localize_batch result; per image: name and true expert

    def run(group):
        # one size: the stacked batch, as ever; several: a ragged batch (the list form of localize_batch)
        one_size = all(tuple(g[1].shape) == tuple(group[0][1].shape) for g in group)
        images = torch.cat([g[1] for g in group]) if one_size else [g[1] for g in group]
        gts = np.stack([np.asarray(g[3].detach().cpu() if isinstance(g[3], torch.Tensor) else g[3], np.float32) for g in group])
        out = localize_batch(images, gating, experts, [float(g[2]) for g in group], gt_poses=gts,
                             gt_experts=[int(g[4]) for g in group], asynchronous=asynchronous,
                             oracle_experts=None if oracle_expert is None else [int(oracle_expert)] * len(group),
                             rot_threshold_deg=rot_threshold_deg, trans_threshold_cm=trans_threshold_cm, verify_gt=verify_gt, **kw)
        batches.append(out)
        names.extend(g[0] for g in group)
        gt_exp.extend(int(g[4]) for g in group)

    group = []
    for sample in samples:
        if group and len(group) == batch_size:
            run(group)
            group = []
        group.append(sample)
    if group:
        run(group)
    n = len(names)
    if n == 0:
        return _statistics(E, [[] for _ in range(E)], [[] for _ in range(E)], [[] for _ in range(E)], trans_threshold_cm,
                           rot_threshold_deg, 0, 0, 0, 0)
    if asynchronous:
        # one copy for the whole test set: the eval rows and the active-expert counts of every batch
        both = torch.cat([torch.cat([b["eval"], b["active_experts"].to(torch.float64).unsqueeze(1)], dim=1) for b in batches]).cpu().numpy()
        rows, active = both[:, :api.EVAL_DOUBLES].copy(), both[:, api.EVAL_DOUBLES]
        if verify_gt:  # (a second copy, of two columns: the winners' scores and the ground truths')
            win_gt = torch.cat([torch.stack([b["records"][:, api.RES_SCORE], b["gt_verify"][:, 0, api.VERIFY_SCORE]], dim=1) for b in batches]).cpu().numpy()
        first = 0
        for b in batches:
            size = int(b["records"].shape[0])
            for f, redo in rerun_frames(b, frames_to_rerun(rows[first:first + size])).items():
                rows[first + f] = redo["eval"]
                if verify_gt:
                    win_gt[first + f, 0] = redo["record"][api.RES_SCORE]
            first += size
    else:
        rows = np.concatenate([b["eval"] for b in batches])
        active = np.concatenate([np.asarray(b["active_experts"], np.float64) for b in batches])
        if verify_gt:
            win_gt = np.concatenate([np.stack([b["records_host"][:, api.RES_SCORE], b["gt_verify"][:, 0, api.VERIFY_SCORE].cpu().numpy()], axis=1)
                                     for b in batches])
    scenes_r, scenes_t, scenes_c = [[] for _ in range(E)], [[] for _ in range(E)], [[] for _ in range(E)]
    for name, ge, row in zip(names, gt_exp, rows):
        scenes_r[ge].append(float(row[api.EVAL_ROT_DEG]))
        scenes_t[ge].append(float(row[api.EVAL_TRANS_CM]))
        scenes_c[ge].append(bool(row[api.EVAL_CLASS_OK] == 1.0))
        if pose_log is not None:
            pose_log.write(POSE_LINE_FORMAT % ((name,) + tuple(float(v) for v in row[api.EVAL_QUAT:api.EVAL_QUAT + 7])))
    stats = _statistics(E, scenes_r, scenes_t, scenes_c, trans_threshold_cm, rot_threshold_deg, float(active.sum()),
                        int(active.max()), time.time() - start, n)
    if verify_gt:
        stats["gt_score_higher"] = float(np.mean(win_gt[:, 1] > win_gt[:, 0]))
    return stats


# ---------------------------------------------------------------- training glue (train_esac.py:104-200)
def random_shift(image, max_shift, rng=None):
    """Zero-pad shift augmentation of util.py:4-11: returns (padX, padY, shifted image)."""
    import random
    r = rng if rng is not None else random
    pad_x = r.randint(-int(max_shift), int(max_shift))
    pad_y = r.randint(-int(max_shift), int(max_shift))
    return pad_x, pad_y, torch.nn.functional.pad(image, (pad_x, -pad_x, pad_y, -pad_y))


def clamp_probs(probs, n):
    """Zero all but the n largest entries in place (util.py:38-47); one topk instead of a Python loop over E."""
    if n < 0 or n >= probs.numel():
        return
    keep = torch.zeros_like(probs, dtype=torch.bool)
    if n > 0:
        keep[torch.topk(probs, n).indices] = True
    probs.masked_fill_(~keep, 0)


def train_step(image, gt_pose, gating, experts, focal_length, hypotheses=256, threshold=10.0, inlier_alpha=100.0,
               inlier_beta=0.5, max_reprojection=100.0, subsample=8, weight_rot=1.0, weight_trans=100.0, loss_cut=100.0,
               max_experts=-1, expert_selection=False, shift=None, generator=None, strict_training=False, evaluate=False,
               gt_expert=None):
    """One iteration of the end-to-end training loop (train_esac.py:104-192) up to and including
    `torch.autograd.backward`; the optimiser step stays with the caller (`ensemble.update`, train_esac.py:195).

    Differences from the reference loop, all of them removals of host round trips:
      * `prediction.cpu()` (train_esac.py:152) and `prediction_gradients.cuda()` (:185) are gone -- the coordinate
        tensor and its gradient container stay in HBM and `esac.backward` accumulates into the latter in place;
      * `torch.exp(gating_log_probs).cpu()` (:129) is gone -- clamp / multinomial / histc run on the device, only the
        E activity flags and the loss value reach the host.
    gating(image) -> log-probabilities [1,E] (with grad); experts[e](image) -> [1,3,H/s,W/s] (with grad).
    strict_training: this call's esac.backward follows the reference in every stage (esac.set_strict_training).
    evaluate: the solver call also hands out its winner's refined pose as a forward record (esac.set_pose_records) and
    esac.eval_batch(record, gt_pose, gt_expert) is enqueued right behind it: the pose error, the 5 cm / 5 deg flag and the gating
    accuracy of the step without a forward call.  The dict gains `records` [1,32] and `eval` [1,16] (device tensors, api.RES_* /
    api.EVAL_*; EVAL_STATUS 1: the winner held no slot, no pose).
    Returns dict(loss, e_hyps, e_hist, prediction, prediction_gradients, gating_log_probs, pad)."""
    dev = image.device
    E = len(experts)
    pp_x = float(image.size(3) / 2)
    pp_y = float(image.size(2) / 2)
    pred_w = math.ceil(image.size(3) / subsample)
    pred_h = math.ceil(image.size(2) / subsample)
    if shift is None:
        pad_x, pad_y, image = random_shift(image, subsample / 2)
    else:
        pad_x, pad_y = int(shift[0]), int(shift[1])
        image = torch.nn.functional.pad(image, (pad_x, -pad_x, pad_y, -pad_y))
    gating_log_probs = gating(image)
    with torch.no_grad():
        gating_probs = torch.exp(gating_log_probs)[0].clone()
        clamp_probs(gating_probs, max_experts)
        if expert_selection:
            expert = torch.multinomial(gating_probs, 1, replacement=True, generator=generator)
            e_hyps = expert.expand((hypotheses,))
        else:
            e_hyps = torch.multinomial(gating_probs, hypotheses, replacement=True, generator=generator)
        e_hist = torch.histc(e_hyps.float(), bins=E, min=0, max=E - 1)
        active = (e_hist > 0).cpu().tolist()
    outputs = [experts[e](image)[0] if on else torch.zeros((3, pred_h, pred_w), device=dev) for e, on in enumerate(active)]
    prediction = torch.stack(outputs)  # [E,3,h,w]; rows of inactive experts are zeros and never read
    prediction_gradients = torch.zeros_like(prediction)
    strict_before = api._state["strict_training"]
    api.set_strict_training(strict_before or strict_training)
    gt_t = torch.as_tensor(gt_pose, dtype=torch.float32)
    records = torch.zeros((1, api.RES_DOUBLES), dtype=torch.float64, device=dev) if evaluate else None
    try:
        if evaluate:
            api.set_pose_records(records[0])
        loss = api.backward(prediction.detach(), prediction_gradients, e_hyps, gt_t.cpu(),
                            weight_rot, weight_trans, loss_cut, pad_x, pad_y, float(focal_length), pp_x, pp_y, threshold,
                            inlier_alpha, inlier_beta, max_reprojection, subsample)
    finally:
        api.set_strict_training(strict_before)
    ev = None
    if evaluate:
        ev = api.eval_batch(records, gt_t.reshape(1, 4, 4), None if gt_expert is None else [int(gt_expert)])
    # gating gradients: REINFORCE-style, loss per drawn hypothesis (train_esac.py:171-177)
    if expert_selection:
        gating_grads = torch.zeros_like(gating_log_probs)
        gating_grads[0, int(expert)] = loss
    else:
        gating_grads = (loss * e_hist).unsqueeze(0).to(gating_log_probs.dtype)
    tensors, grads = [], []
    if prediction.requires_grad:
        tensors.append(prediction)
        grads.append(prediction_gradients)
    if gating_log_probs.requires_grad:
        tensors.append(gating_log_probs)
        grads.append(gating_grads)
    if tensors:
        torch.autograd.backward(tensors, grads)
    out = dict(loss=loss, e_hyps=e_hyps, e_hist=e_hist, prediction=prediction, prediction_gradients=prediction_gradients,
               gating_log_probs=gating_log_probs, pad=(pad_x, pad_y))
    if evaluate:
        out["records"], out["eval"] = records, ev
    return out


def _train_focals_pads(B, focal_lengths, shifts, subsample, generator):
    """train_batch's per-image focal lengths and shifts (given, or drawn within +-subsample/2)."""
    focals = [float(f) for f in (focal_lengths.tolist() if isinstance(focal_lengths, (torch.Tensor, np.ndarray)) and
                                 getattr(focal_lengths, "ndim", 0) > 0 else
                                 focal_lengths if isinstance(focal_lengths, (list, tuple)) else [focal_lengths] * B)]
    if len(focals) != B:
        raise RuntimeError("train_batch: focal_lengths must hold one value per image (%d), found %d" % (B, len(focals)))
    if shifts is None:
        m = int(subsample / 2)
        if generator is not None:
            drawn = torch.randint(-m, m + 1, (B, 2), generator=generator, device=generator.device).cpu().tolist()
            pads = [(int(x), int(y)) for x, y in drawn]
        else:
            import random
            pads = [(random.randint(-m, m), random.randint(-m, m)) for _ in range(B)]
    else:
        pads = [(int(s[0]), int(s[1])) for s in shifts]
        if len(pads) != B:
            raise RuntimeError("train_batch: shifts must hold one pair per image (%d), found %d" % (B, len(pads)))
    return focals, pads


def _train_batch_ragged(images, gt_poses, gating, experts, focal_lengths, hypotheses, threshold, inlier_alpha, inlier_beta,
                        max_reprojection, subsample, weight_rot, weight_trans, loss_cut, max_experts, expert_selection, shifts, e_hyps,
                        generator, strict_training, asynchronous, all_experts, evaluate, gt_experts):
    """train_batch over images of different sizes (training sets resized by their shorter edge).  The networks run once per group
    of equally sized images, as in `_localize_ragged`; their predictions go into ONE packed buffer (esac.pack_frames' layout),
    followed by ONE solver call (`esac.backward_batch_shapes` or `esac.backward_batch_shapes_async`) that accumulates into a packed
    gradient buffer of the same layout, and ONE `torch.autograd.backward` over every group's outputs and the gating.  Every frame
    has its own principal point (the image centre), focal length and shift.  Every option keeps train_batch's meaning.
    The result dict is train_batch's with prediction / prediction_gradients = the packed [B,S] buffers and shapes = [(h_b, w_b)]."""
    B, E = len(images), len(experts)
    dev = images[0].device
    pp_x = [float(im.size(3) / 2) for im in images]
    pp_y = [float(im.size(2) / 2) for im in images]
    shapes = [(math.ceil(im.size(2) / subsample), math.ceil(im.size(3) / subsample)) for im in images]
    focals, pads = _train_focals_pads(B, focal_lengths, shifts, subsample, generator)
    images = [torch.nn.functional.pad(im, (px, -px, py, -py)) for im, (px, py) in zip(images, pads)]
    groups = {}  # image size -> frames, in order of first appearance
    for b, im in enumerate(images):
        groups.setdefault(tuple(im.shape[1:]), []).append(b)
    stacked = {key: torch.cat([images[b] for b in members]) for key, members in groups.items()}
    order = [b for members in groups.values() for b in members]  # frame of row r of the groups' outputs, one after the other
    inverse = torch.as_tensor(sorted(range(B), key=order.__getitem__), device=dev)
    gating_log_probs = torch.cat([gating(stacked[key]) for key in groups]).index_select(0, inverse)  # [B,E], frame order
    expert = None
    with torch.no_grad():
        if e_hyps is not None:
            e_hyps = torch.as_tensor(e_hyps, dtype=torch.int64).to(dev)
            if e_hyps.dim() != 2 or e_hyps.size(0) != B:
                raise RuntimeError("train_batch: e_hyps must be [B,N]")
            if expert_selection:
                expert = e_hyps[:, :1]
        else:
            gating_probs = torch.exp(gating_log_probs).clone()
            for b in range(B):
                clamp_probs(gating_probs[b], max_experts)
            if expert_selection:
                expert = torch.multinomial(gating_probs, 1, replacement=True, generator=generator)  # [B,1]
                e_hyps = expert.expand((B, hypotheses))
            else:
                e_hyps = torch.multinomial(gating_probs, hypotheses, replacement=True, generator=generator)
        e_hist = torch.zeros((B, E), device=dev).scatter_add_(1, e_hyps, torch.ones(e_hyps.shape, device=dev))
        active = None if all_experts else (e_hist > 0).cpu().tolist()  # B x E flags: all that reaches the host before the call
    packed = torch.zeros((B, api.packed_stride(E, shapes)), dtype=torch.float32, device=dev)
    outputs = []  # (group's frames, expert, the expert's output on the group [n,3,h,w])
    for key, members in groups.items():
        for e in range(E):
            if active is not None and not any(active[b][e] for b in members):
                continue  # (rows of inactive experts are zeros, never read, and receive no gradient)
            maps = experts[e](stacked[key])
            outputs.append((members, e, maps))
            with torch.no_grad():
                for i, b in enumerate(members):
                    api.unpack_frames(packed[b:b + 1], [shapes[b]], E)[0][e] = maps[i]
    packed_gradients = torch.zeros_like(packed)
    strict_before = api._state["strict_training"]
    api.set_strict_training(strict_before or strict_training)
    gt_t = torch.as_tensor(np.asarray(gt_poses, np.float32) if not isinstance(gt_poses, torch.Tensor) else gt_poses, dtype=torch.float32)
    records = torch.zeros((B, api.RES_DOUBLES), dtype=torch.float64, device=dev) if evaluate else None
    try:
        solver = api.backward_batch_shapes_async if asynchronous else api.backward_batch_shapes
        losses = solver(packed, packed_gradients, e_hyps.contiguous(), gt_t if asynchronous else gt_t.cpu(), weight_rot, weight_trans,
                        loss_cut, [p[0] for p in pads], [p[1] for p in pads], focals, pp_x, pp_y, threshold, inlier_alpha, inlier_beta,
                        max_reprojection, subsample, poseRecords=records, shapes=shapes, experts=E)
    finally:
        api.set_strict_training(strict_before)
    ev = api.eval_batch(records, gt_t, gt_experts) if evaluate else None
    loss_t = losses.to(torch.float32) if asynchronous else torch.tensor(losses, device=dev, dtype=torch.float32)
    if expert_selection:
        gating_grads = torch.zeros_like(gating_log_probs)
        gating_grads.scatter_(1, expert, loss_t.unsqueeze(1).to(gating_log_probs.dtype))
    else:
        gating_grads = (loss_t.unsqueeze(1) * e_hist).to(gating_log_probs.dtype)
    frame_grads = api.unpack_frames(packed_gradients, shapes, E)  # views: frame b's [E,3,h_b,w_b]
    tensors, grads = [], []
    for members, e, maps in outputs:
        if maps.requires_grad:
            tensors.append(maps)
            grads.append(torch.stack([frame_grads[b][e] for b in members]))
    if gating_log_probs.requires_grad:
        tensors.append(gating_log_probs)
        grads.append(gating_grads)
    if tensors:
        torch.autograd.backward(tensors, grads)
    out = dict(losses=losses, e_hyps=e_hyps, e_hist=e_hist, prediction=packed, prediction_gradients=packed_gradients, shapes=shapes,
               gating_log_probs=gating_log_probs, pads=pads)
    if evaluate:
        out["records"], out["eval"] = records, ev
    return out


def train_batch(images, gt_poses, gating, experts, focal_lengths, hypotheses=256, threshold=10.0, inlier_alpha=100.0,
                inlier_beta=0.5, max_reprojection=100.0, subsample=8, weight_rot=1.0, weight_trans=100.0, loss_cut=100.0,
                max_experts=-1, expert_selection=False, shifts=None, e_hyps=None, generator=None, strict_training=False,
                asynchronous=False, all_experts=False, evaluate=False, gt_experts=None):
    """The mini-batch form of `train_step`: B images through ONE `esac.backward_batch` with a shift and a focal length per
    image (train_esac.py:112 reads the focal length per image, :125 draws a new shift for every image), up to and including
    one `torch.autograd.backward`.

    images [B,3,H,W]; gt_poses [B,4,4]; focal_lengths: B numbers (or one for all).  gating(images) -> log-probabilities [B,E];
    experts[e](images) -> [B,3,H/s,W/s].  Every image is padded by its own shift (`shifts`: B pairs, or drawn per image within
    +-subsample/2 -- from `generator` when one is given, else from Python's `random` like `random_shift`), the gating runs once
    on the batch, the hypothesis assignment is drawn per frame on the device (or given: `e_hyps` [B,N]), and every expert that
    is active in at least one frame runs once on the batch: the rows of frames in which it is inactive are never read by the
    kernels and receive a zero gradient.  Only the B x E activity flags and the B losses reach the host.
    strict_training: this call's esac.backward_batch follows the reference in every stage (esac.set_strict_training).
    asynchronous: the solver is `esac.backward_batch_async` -- the call returns once its launches are enqueued, `losses` stays a
    DEVICE tensor [B] (float64) and the gating gradients are formed from it on the device, so the autograd backward is enqueued
    while the solver still runs.  all_experts: every expert runs on the batch and the `.cpu()` of the B x E activity flags is
    skipped (the rows of inactive experts are still never read).  With both, the step up to and including
    `torch.autograd.backward` contains no host synchronisation, given device `images`, a device `gt_poses` tensor and `e_hyps`
    drawn on the device.  What remains host-side: the shifts (drawn or given on the host, one pad per image) and the focal lengths,
    which travel as the call's per-frame camera table; a host `gt_poses` is uploaded asynchronously.
    evaluate: the solver call is armed to hand out every frame's winner as a forward record (poseRecords) and
    esac.eval_batch(records, gt_poses, gt_experts) is enqueued right behind it; the dict gains `records` [B,32] and `eval` [B,16],
    device tensors (asynchronous: still no host synchronisation in the step, given a device `gt_experts` tensor or None).  A frame
    whose winner held no slot -- a singular ground truth on the asynchronous route among them -- has EVAL_STATUS 1 and NaN figures.
    Returns dict(losses (list of B floats; asynchronous: device tensor [B]), e_hyps [B,N], e_hist [B,E], prediction [B,E,3,h,w],
    prediction_gradients, gating_log_probs [B,E], pads (list of B pairs)).
    images may also be a LIST of B images [1,3,H_b,W_b] (or [3,H_b,W_b]) of different sizes: a ragged mini-batch
    (`_train_batch_ragged`; a list whose images share one size is stacked and takes the route above)."""
    if isinstance(images, (list, tuple)):
        images = [im if im.dim() == 4 else im.unsqueeze(0) for im in images]
        if len(images) == 0 or any(im.dim() != 4 or im.size(0) != 1 for im in images):
            raise RuntimeError("train_batch: images must be a [B,3,H,W] tensor or a non-empty list of [1,3,H,W] / [3,H,W] images")
        if any(tuple(im.shape) != tuple(images[0].shape) for im in images):
            return _train_batch_ragged(images, gt_poses, gating, experts, focal_lengths, hypotheses, threshold, inlier_alpha, inlier_beta,
                                       max_reprojection, subsample, weight_rot, weight_trans, loss_cut, max_experts, expert_selection,
                                       shifts, e_hyps, generator, strict_training, asynchronous, all_experts, evaluate, gt_experts)
        images = torch.cat(images)
    dev = images.device
    B, E = int(images.size(0)), len(experts)
    pp_x = float(images.size(3) / 2)
    pp_y = float(images.size(2) / 2)
    pred_w = math.ceil(images.size(3) / subsample)
    pred_h = math.ceil(images.size(2) / subsample)
    focals, pads = _train_focals_pads(B, focal_lengths, shifts, subsample, generator)
    images = torch.cat([torch.nn.functional.pad(images[b:b + 1], (px, -px, py, -py)) for b, (px, py) in enumerate(pads)])
    gating_log_probs = gating(images)  # [B,E]
    expert = None
    with torch.no_grad():
        if e_hyps is not None:
            e_hyps = torch.as_tensor(e_hyps, dtype=torch.int64).to(dev)
            if e_hyps.dim() != 2 or e_hyps.size(0) != B:
                raise RuntimeError("train_batch: e_hyps must be [B,N]")
            if expert_selection:
                expert = e_hyps[:, :1]
        else:
            gating_probs = torch.exp(gating_log_probs).clone()
            for b in range(B):
                clamp_probs(gating_probs[b], max_experts)
            if expert_selection:
                expert = torch.multinomial(gating_probs, 1, replacement=True, generator=generator)  # [B,1]
                e_hyps = expert.expand((B, hypotheses))
            else:
                e_hyps = torch.multinomial(gating_probs, hypotheses, replacement=True, generator=generator)  # one row of draws per frame
        e_hist = torch.zeros((B, E), device=dev).scatter_add_(1, e_hyps, torch.ones(e_hyps.shape, device=dev))
        if all_experts:
            active_any = [True] * E  # no flags cross to the host: every expert runs
        else:
            active = (e_hist > 0).cpu()  # [B,E] flags: all that reaches the host before the call
            active_any = active.any(dim=0).tolist()
    outputs = [experts[e](images) if on else torch.zeros((B, 3, pred_h, pred_w), device=dev) for e, on in enumerate(active_any)]
    prediction = torch.stack(outputs, dim=1)  # [B,E,3,h,w]
    prediction_gradients = torch.zeros_like(prediction)
    strict_before = api._state["strict_training"]
    api.set_strict_training(strict_before or strict_training)
    gt_t = torch.as_tensor(np.asarray(gt_poses, np.float32) if not isinstance(gt_poses, torch.Tensor) else gt_poses, dtype=torch.float32)
    # (zeros: a frame whose kernels never reach the record write reads RES_VALID = 0 -> EVAL_STATUS 1, not stale memory)
    records = torch.zeros((B, api.RES_DOUBLES), dtype=torch.float64, device=dev) if evaluate else None
    try:
        if asynchronous:  # (a device gt_poses stays where it is)
            losses = api.backward_batch_async(prediction.detach(), prediction_gradients, e_hyps.contiguous(), gt_t,
                                              weight_rot, weight_trans, loss_cut, [p[0] for p in pads], [p[1] for p in pads], focals,
                                              pp_x, pp_y, threshold, inlier_alpha, inlier_beta, max_reprojection, subsample,
                                              poseRecords=records)
        else:
            losses = api.backward_batch(prediction.detach(), prediction_gradients, e_hyps.contiguous(), gt_t.cpu(),
                                        weight_rot, weight_trans, loss_cut, [p[0] for p in pads], [p[1] for p in pads], focals, pp_x, pp_y,
                                        threshold, inlier_alpha, inlier_beta, max_reprojection, subsample, poseRecords=records)
    finally:
        api.set_strict_training(strict_before)
    ev = api.eval_batch(records, gt_t, gt_experts) if evaluate else None  # behind the solver on the same stream: nothing is waited for
    # gating gradients, per frame: REINFORCE-style, loss per drawn hypothesis (train_esac.py:171-177)
    loss_t = losses.to(torch.float32) if asynchronous else torch.tensor(losses, device=dev, dtype=torch.float32)
    if expert_selection:
        gating_grads = torch.zeros_like(gating_log_probs)
        gating_grads.scatter_(1, expert, loss_t.unsqueeze(1).to(gating_log_probs.dtype))
    else:
        gating_grads = (loss_t.unsqueeze(1) * e_hist).to(gating_log_probs.dtype)
    tensors, grads = [], []
    if prediction.requires_grad:
        tensors.append(prediction)
        grads.append(prediction_gradients)
    if gating_log_probs.requires_grad:
        tensors.append(gating_log_probs)
        grads.append(gating_grads)
    if tensors:
        torch.autograd.backward(tensors, grads)
    out = dict(losses=losses, e_hyps=e_hyps, e_hist=e_hist, prediction=prediction, prediction_gradients=prediction_gradients,
               gating_log_probs=gating_log_probs, pads=pads)
    if evaluate:
        out["records"], out["eval"] = records, ev
    return out
