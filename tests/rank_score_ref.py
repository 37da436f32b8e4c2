"""Plain fp64 reference of the ranking score (numpy, nothing from the oracle).

score = alpha / W / H * sum over cells of 1 / (1 + exp(beta (min(err, maxReproj) - tau))), err = |pixel - projection|, with
the reference's projection (esac_util.h:292-319: `z != 0 ? 1/z : 1`, no cheirality test) and the default route's rule for a
cell with a non-finite scene coordinate: it can never be an inlier, err = maxReproj ("non-finite scene
coordinates") -- not the strict route's NaN.  Pixel centres are x * sub + sub / 2 - shift (esac_util.h:64-66, integers).

tests/test_rank_score_ref_host.py pins this file to the oracle on the CPU; tests/test_gpu_rank_score.py holds the fp32
ranking kernels against it.
"""
import numpy as np


def rodrigues(rvec):
    """Rotation vector -> matrix (cv::Rodrigues: identity below DBL_EPSILON)."""
    r = np.asarray(rvec, np.float64)
    th = float(np.linalg.norm(r))
    if th < np.finfo(np.float64).eps:
        return np.eye(3)
    k = r / th
    K = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    return np.cos(th) * np.eye(3) + (1.0 - np.cos(th)) * np.outer(k, k) + np.sin(th) * K


def rotation_vector(R):
    """Rotation matrix -> vector, angles in [0, pi]."""
    R = np.asarray(R, np.float64)
    sk = 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    s, c = float(np.linalg.norm(sk)), (np.trace(R) - 1.0) / 2.0
    th = np.arctan2(s, c)
    if s > 1e-8:
        return sk / s * th
    if c > 0:
        return sk  # th ~ 0: sin(th) ~ th
    # th ~ pi: the axis from the symmetric part, R + I = 2 k k^T
    S = (R + np.eye(3)) / 2.0
    k = np.sqrt(np.maximum(np.diag(S), 0.0))
    j = int(np.argmax(k))
    k = np.where(S[j] < 0, -k, k)
    k[j] = abs(k[j])
    return k / np.linalg.norm(k) * th


def pixel_centres(H, W, sub, shift):
    xs = (np.arange(W) * int(sub) + int(sub) // 2 - int(shift[0])).astype(np.float64)
    ys = (np.arange(H) * int(sub) + int(sub) // 2 - int(shift[1])).astype(np.float64)
    return np.meshgrid(xs, ys)  # [H, W] each


def errors(scene_map, R, t, focal, ppx, ppy, sub, shift, max_reproj):
    """Clamped reprojection errors [H, W] of one hypothesis (R [3,3], t [3]: scene -> camera) on one map [3, H, W]."""
    m = np.asarray(scene_map, np.float64)
    _, H, W = m.shape
    finite = np.isfinite(m).all(axis=0)
    X = np.where(finite, m, 0.0)
    R = np.asarray(R, np.float64)
    t = np.asarray(t, np.float64)
    with np.errstate(all="ignore"):
        cam = np.einsum("ij,jhw->ihw", R, X) + t[:, None, None]
        iz = np.where(cam[2] != 0.0, 1.0 / cam[2], 1.0)
        u = cam[0] * iz * float(focal) + float(ppx)
        v = cam[1] * iz * float(focal) + float(ppy)
        px, py = pixel_centres(H, W, sub, shift)
        err = np.hypot(px - u, py - v)
        # std::min(err, maxReproj) = (maxReproj < err) ? maxReproj : err; a NaN here (inf - inf of a wild pose) is an error
        # that is no number below maxReproj: the clamp, like a non-finite cell
        err = np.where(err < float(max_reproj), err, float(max_reproj))
    return np.where(finite, err, float(max_reproj))


def score(scene_map, R, t, focal, ppx, ppy, sub, shift, alpha, beta, tau, max_reproj):
    err = errors(scene_map, R, t, focal, ppx, ppy, sub, shift, max_reproj)
    _, H, W = np.shape(scene_map)
    with np.errstate(over="ignore"):
        w = 1.0 / (1.0 + np.exp(float(beta) * (err - float(tau))))
    return float(w.sum() * (float(alpha) / W / H))


def scores(coords, assign, hyps, focal, ppx, ppy, sub, shift, alpha, beta, tau, max_reproj):
    """fp64 scores [N] of hypotheses [N, 6] (rvec, t), hypothesis h on map coords[assign[h]]."""
    return np.array([score(coords[int(e)], rodrigues(h[:3]), h[3:], focal, ppx, ppy, sub, shift, alpha, beta, tau, max_reproj)
                     for h, e in zip(np.asarray(hyps, np.float64), assign)])
