"""NumPy restatement of the fundamental-matrix RANSAC the HIP kernels implement, and the seeded
inputs the tests share.  Not a test module: the yardstick of tests/test_gpu_fundamental.py and test_fundamental_host.py.

Definition (all FP64).  A pair is two point lists a[N][2], b[N][2]; the caller supplies the sample table S[H][8].
For every hypothesis (and for the refit, over all inliers of the winner): Hartley normalisation of both lists, one row
[x'x, x'y, x', y'x, y'y, y', x, y, 1] per point, f = eigenvector of the smallest eigenvalue of A^T A, rank 2 through the
smallest eigenvector of F^T F, F <- T_b^T F T_a, unit Frobenius norm.  Error of a point: the larger of the two squared
point-to-epipolar-line distances; inlier iff error <= threshold^2.  Winner: the valid hypothesis with the most inliers,
the lowest index on ties; fewer than 8 inliers = failure.  The mask is the winner's, not the refit's."""
import json
import os

import numpy as np

from mocapv2_amd import synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def norm(p):
    c = p.mean(0)
    d = np.sqrt(((p - c) ** 2).sum(1)).mean()
    s = np.sqrt(2) / d
    return np.array([[s, 0, -s * c[0]], [0, s, -s * c[1]], [0, 0, 1]])


def n_point(a, b):
    """Steps 1-4 of the definition over the points given (8 of a sample, or all inliers)."""
    with np.errstate(all="ignore"):
        Ta, Tb = norm(a), norm(b)
        ha = np.c_[a, np.ones(len(a))] @ Ta.T
        hb = np.c_[b, np.ones(len(b))] @ Tb.T
        A = np.stack([hb[:, 0] * ha[:, 0], hb[:, 0] * ha[:, 1], hb[:, 0], hb[:, 1] * ha[:, 0], hb[:, 1] * ha[:, 1], hb[:, 1],
                      ha[:, 0], ha[:, 1], np.ones(len(a))], 1)
        if not np.isfinite(A).all():
            return np.full((3, 3), np.nan)
        F = np.linalg.eigh(A.T @ A)[1][:, 0].reshape(3, 3)
        v = np.linalg.eigh(F.T @ F)[1][:, 0]
        F = F - np.outer(F @ v, v)
        F = Tb.T @ F @ Ta
        return F / np.linalg.norm(F)


def errors(F, a, b):
    ha = np.c_[a, np.ones(len(a))]
    hb = np.c_[b, np.ones(len(b))]
    l2 = ha @ F.T
    l1 = hb @ F
    with np.errstate(all="ignore"):
        return np.maximum((hb * l2).sum(1) ** 2 / (l2[:, 0] ** 2 + l2[:, 1] ** 2),
                          (ha * l1).sum(1) ** 2 / (l1[:, 0] ** 2 + l1[:, 1] ** 2))


def rms_distance(F, a, b):
    """RMS of sqrt(e_i): the figure C1 and C5 compare."""
    return float(np.sqrt(errors(np.asarray(F, float), a, b).mean()))


def ransac(a, b, samples, threshold, refit=True, band_rel=1e-6):
    """The whole definition.  dict: F_all [H][3][3], counts [H], banded [H] (points of each hypothesis whose error lies within
    a relative band_rel of threshold^2), best, n_inliers, mask [N] bool, F_sample, F_refit (None without refit); best = -1
    and no matrices when the pair fails."""
    a, b = np.asarray(a, float), np.asarray(b, float)
    H, t2 = len(samples), threshold ** 2
    F_all = np.empty((H, 3, 3))
    counts = np.zeros(H, np.int64)
    band = np.zeros(H, np.int64)
    for h in range(H):
        F_all[h] = n_point(a[samples[h]], b[samples[h]])
        if np.isfinite(F_all[h]).all():
            e = errors(F_all[h], a, b)
            with np.errstate(invalid="ignore"):
                counts[h] = (e <= t2).sum()
                band[h] = (np.abs(e - t2) <= band_rel * t2).sum()
    valid = np.isfinite(F_all).all((1, 2))
    out = {"F_all": F_all, "counts": counts, "banded": band, "best": -1, "n_inliers": 0, "mask": np.zeros(len(a), bool),
           "F_sample": None, "F_refit": None}
    if not valid.any():
        return out
    best = int(np.argmax(np.where(valid, counts, -1)))  # argmax returns the first of equal maxima
    if counts[best] < 8:
        return out
    with np.errstate(invalid="ignore"):
        mask = errors(F_all[best], a, b) <= t2
    out.update(best=best, n_inliers=int(counts[best]), mask=mask, F_sample=F_all[best],
               F_refit=n_point(a[mask], b[mask]) if refit else None)
    return out


def align_sign(F, ref):
    """F or -F, whichever is closer to ref (a unit-norm matrix is defined up to sign)."""
    F, ref = np.asarray(F, float).reshape(3, 3), np.asarray(ref, float).reshape(3, 3)
    return F if np.abs(F - ref).max() <= np.abs(-F - ref).max() else -F


# ---- inputs ------------------------------------------------------------------------------------------------------------
def bundled_pair():
    """The reference's own 54 wand points (tests/golden/jsons/image_points.json, [point][camera][2])."""
    with open(os.path.join(GOLDEN, "jsons", "image_points.json")) as f:
        ip = np.transpose(np.array(json.load(f), float), (1, 0, 2))
    return ip[0].copy(), ip[1].copy()


def bundled_cv2_fundamental():
    """fundamentals.json[0]: what cv.findFundamentalMat returned on those points (reference CalculateCameraPoses.py:189)."""
    with open(os.path.join(GOLDEN, "jsons", "fundamentals.json")) as f:
        return np.array(json.load(f)[0], float)


def synthetic_pair(scene, cam_a, cam_b, n_points, seed, outlier_share, sigma=0.5, extent=0.8):
    """Seeded pair of a synth.Scene: 3-D points uniform in [-extent, extent]^3 projected without distortion, Gaussian
    jitter on both images, a share of the second image's points replaced by points uniform in the image.  Draws, in this
    order, from default_rng(seed): the 3-D points, the jitter of the first image, of the second, the outlier indices,
    the outlier positions.  Returns a, b (what a detector would deliver), a0, b0 (the noise-free projections) and the
    boolean list of true inliers."""
    rng = np.random.default_rng(seed)
    X = rng.uniform(-extent, extent, size=(n_points, 3))
    a0 = synth.project(X, scene.poses[cam_a], scene.K, synth.ZERO_DIST)
    b0 = synth.project(X, scene.poses[cam_b], scene.K, synth.ZERO_DIST)
    a = a0 + rng.normal(0, sigma, a0.shape)
    b = b0 + rng.normal(0, sigma, b0.shape)
    n_out = int(round(outlier_share * n_points))
    true_inlier = np.ones(n_points, bool)
    if n_out:
        idx = rng.choice(n_points, n_out, replace=False)
        b[idx] = rng.uniform(0, 1, (n_out, 2)) * np.array([scene.width, scene.height], float)
        true_inlier[idx] = False
    return a, b, a0, b0, true_inlier


# name -> (ring size, camera a, camera b, points, seed, outlier share, threshold, hypotheses); the table's seed is the case's
SMALL_CASES = {
    "s11": (6, 0, 1, 2000, 11, 0.30, 3.0, 1000),
    "s12": (6, 1, 2, 500, 12, 0.40, 3.0, 1000),
    "s13": (6, 2, 3, 300, 13, 0.20, 3.0, 1000),
    "s14": (6, 3, 4, 54, 14, 0.0, 3.0, 1000),
    "s15": (6, 4, 5, 1200, 15, 0.50, 3.0, 1000),
}


def small_case(name):
    """(a, b, samples, threshold, extras) of `bundled` or one of SMALL_CASES; extras = None or (a0, b0, true_inlier)."""
    from mocapv2_amd.calibrate import sample_table
    if name == "bundled":
        a, b = bundled_pair()
        return a, b, sample_table(len(a), 1000, 0), 10.0, None
    ring, ca, cb, n, seed, share, thr, H = SMALL_CASES[name]
    a, b, a0, b0, ti = synthetic_pair(synth.Scene(ring), ca, cb, n, seed, share)
    return a, b, sample_table(n, H, seed), thr, (a0, b0, ti)


def large_case(i):
    """Pair 0-i of the 16-camera ring: 20 000 points, 30 % outliers, data and table seed 40 + i, threshold 3, H = 2048."""
    from mocapv2_amd.calibrate import sample_table
    a, b, a0, b0, ti = synthetic_pair(synth.Scene(16), 0, i, 20000, 40 + i, 0.30)
    return a, b, sample_table(20000, 2048, 40 + i), 3.0, (a0, b0, ti)


def ring_points(scene, n_points, seed, outlier_share, sigma=0.5, extent=0.8):
    """The same kind of data for every camera of a rig at once (the input of calibrate.tracker_fundamentals): from
    default_rng(seed) the 3-D points, then the jitter of camera 0, 1, ..., then for every camera i >= 1 in turn its outlier
    indices and positions.  Returns image points [C][N][2], their noise-free projections and true inliers [C][N]."""
    rng = np.random.default_rng(seed)
    X = rng.uniform(-extent, extent, size=(n_points, 3))
    clean = np.stack([synth.project(X, pose, scene.K, synth.ZERO_DIST) for pose in scene.poses])
    pts = clean + np.stack([rng.normal(0, sigma, (n_points, 2)) for _ in scene.poses])
    n_out = int(round(outlier_share * n_points))
    true_inlier = np.ones((scene.n_cam, n_points), bool)
    for i in range(1, scene.n_cam):
        idx = rng.choice(n_points, n_out, replace=False)
        pts[i, idx] = rng.uniform(0, 1, (n_out, 2)) * np.array([scene.width, scene.height], float)
        true_inlier[i, idx] = False
    return pts, clean, true_inlier
