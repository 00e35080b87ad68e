"""Calibration-time batch paths: the arithmetic of the reference's
`CalculateCameraPoses.py` -- fundamental matrices from image points by RANSAC (:189), relative pose from a fundamental
matrix with the four-candidate cheirality vote (:195-231), bundle adjustment (lib/Helpers.py:158-176), origin / floor alignment (:283-361) and
`poses_to_fundamental_matrix` (:26-78) -- on top of the same HIP triangulation / reprojection kernels the per-frame
path uses.

What is batched that the reference loops over:
  * `cv.findFundamentalMat(p1, p2, cv.FM_RANSAC, 10, .)` per consecutive camera pair (:189) is ONE call for any list of
    camera pairs (`find_fundamental_matrices`; `tracker_fundamentals` for the pairs 0 -> i the tracker needs): every
    hypothesis of every pair is solved and scored on the GPU (csrc/fundamental.hip; definition in DESIGN.md section 2);
  * the four (R, t) candidates are triangulated by ONE launch over 4 N groups (the reference calls
    `triangulate_points` four times, one Python SVD per point);
  * one bundle-adjustment Jacobian (SciPy's 2-point forward differences: 6 perturbed parameter vectors per free
    camera) is ONE triangulation launch + ONE reprojection launch over 7 N groups instead of 6 x 2 x N Python calls;
    steps and rounding are SciPy's, so the optimiser walks the same iterates as the reference's
    `least_squares(..., jac='2-point')`.
Beyond the reference (whose calibration is two-camera at heart): `calibrate_rig` = `rig_initial_poses` (all camera pairs'
fundamental matrices in one RANSAC call, a spanning tree with a common scale) + `bundle_adjust_rig` (all poses and all points
on the GPU over exactly the observations that exist, csrc/rig_ba.hip; definition in DESIGN.md section 2; with
loss="cauchy" robust against the outliers of a real capture, which it reports per observation and refits without; with
`bundle_adjust_rig_intrinsics` / `calibrate_rig_intrinsics` the cameras' K and distortion are unknowns of the same adjustment,
csrc/rig_selfcal.hip).
`calibrate_intrinsics` supplies the camera_params all of these take: K and distortion of every camera from board views
(the reference's CalculateCameraIntrinsic.py:58, cv2.calibrateCamera, batched over the rig; csrc/intrinsics.hip).
Image capture and the plotting / JSON writing of that script are outside the path.  `calculate_extrinsics` is the
script's function of that name (:162-255) from image points to poses; the pieces still take fundamental matrices as
arguments.
"""
import json
from itertools import combinations

import numpy as np

from .engine import default_context


# ---- small closed forms -----------------------------------------------------------------------------------------
def poses_to_fundamental_matrix(pose1, pose2, K1=None, K2=None):
    """reference CalculateCameraPoses.py:26-78: F with x2^T F x1 = 0 from two world->camera poses; the essential
    matrix when no intrinsics are given."""
    R1, t1 = np.asarray(pose1["R"], float), np.asarray(pose1["t"], float).reshape(3, 1)
    R2, t2 = np.asarray(pose2["R"], float), np.asarray(pose2["t"], float).reshape(3, 1)
    R_rel = R2 @ R1.T
    t_rel = (t2 - R2 @ R1.T @ t1).ravel()
    E = np.array([[0, -t_rel[2], t_rel[1]], [t_rel[2], 0, -t_rel[0]], [-t_rel[1], t_rel[0], 0]]) @ R_rel
    if K1 is not None and K2 is not None:
        return np.linalg.inv(np.asarray(K2, float)).T @ E @ np.linalg.inv(np.asarray(K1, float))
    return E


def decompose_essential(E):
    """cv.decomposeEssentialMat (reference :197) in closed form: with E = U diag(1,1,0) Vt, det U = det Vt = +1,
    R1 = U W Vt, R2 = U W^T Vt, t = U[:, 2] (unit length, sign free).  The SVD's sign freedom only permutes the
    candidate set {R1, R2} x {t, -t} that `select_relative_pose` votes over."""
    U, _, Vt = np.linalg.svd(np.asarray(E, float))
    if np.linalg.det(U) < 0:
        U = -U
    if np.linalg.det(Vt) < 0:
        Vt = -Vt
    W = np.array([[0.0, 1.0, 0.0], [-1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    return U @ W @ Vt, U @ W.T @ Vt, U[:, 2].reshape(3, 1)


def _intrinsics(camera_params, n):
    K = [np.asarray(camera_params[i % len(camera_params)]["intrinsic_matrix"], float) for i in range(n)]
    d = [np.asarray(camera_params[i % len(camera_params)]["distortion_coef"], float).ravel()[:5] for i in range(n)]
    return np.array(K), np.array(d)


# ---- fundamental matrices: batched RANSAC on the GPU --------------------------------------------------------------
def sample_table(n_points, hypotheses, seed):
    """The sample table of `mocap_fundamental_ransac`: int32 [hypotheses][8] point indices, 8 distinct ones per row, from
    `default_rng(seed).integers(0, n_points, (H, 8))`; rows holding an index twice are redrawn from the same generator
    until none is left.  The host draws, the device never does: a run is reproducible from its seed."""
    n_points, hypotheses = int(n_points), int(hypotheses)
    if n_points < 8:
        raise ValueError(f"a fundamental matrix needs at least 8 points, got {n_points}")
    if hypotheses < 1:
        raise ValueError(f"hypotheses = {hypotheses}")
    rng = np.random.default_rng(seed)
    S = rng.integers(0, n_points, (hypotheses, 8))
    while True:
        srt = np.sort(S, axis=1)
        bad = np.flatnonzero((srt[:, 1:] == srt[:, :-1]).any(axis=1))
        if len(bad) == 0:
            break
        S[bad] = rng.integers(0, n_points, (len(bad), 8))
    return np.ascontiguousarray(S, np.int32)


def _scaled_like_cv2(F):
    """OpenCV's 8-point solver returns F scaled so that F[2, 2] = 1 when that entry is not negligible."""
    F = np.asarray(F, float).reshape(3, 3)
    return F / F[2, 2] if abs(F[2, 2]) > np.finfo(float).eps else F.copy()


def find_fundamental_matrices(image_points, pairs, valid=None, threshold=10.0, hypotheses=1000, seed=0, refit=True, ctx=None,
                              details=False):
    """`cv.findFundamentalMat(p_i, p_j, cv.FM_RANSAC, threshold, .)` (reference CalculateCameraPoses.py:189) for a list of
    camera pairs in ONE batched GPU call (engine.MocapContext.fundamental_ransac -> mocap_fundamental_ransac).
    image_points [C][N][2]; pairs: list of (i, j), F maps camera-i pixels to camera-j lines (x_j^T F x_i = 0); valid
    [C][N] (optional): a pair uses the points both of its cameras saw.  Pair k draws its sample table from seed + k.
    Returns a list of (F, mask) per pair in the shape of cv2's return: F 3x3 scaled to F[2, 2] = 1, mask uint8 [N, 1] over
    ALL N points (0 for points the pair did not use); (None, None) for a pair that fails (fewer than 8 common points, no
    valid hypothesis, a winner with fewer than 8 inliers), as cv2 returns None.  details=True appends the engine's dict
    (unit-norm F_sample / F_refit, best, n_inliers) to each tuple."""
    ip = np.asarray(image_points, float)
    if ip.ndim != 3 or ip.shape[2] != 2:
        raise ValueError(f"image_points must be [C][N][2], got {ip.shape}")
    Cn, N = ip.shape[:2]
    vis = np.ones((Cn, N), bool) if valid is None else np.asarray(valid).astype(bool).reshape(Cn, N)
    if not float(threshold) > 0 or int(hypotheses) < 1:
        raise ValueError(f"threshold = {threshold}, hypotheses = {hypotheses}")
    use, lists, tables = [], [], []
    for k, (i, j) in enumerate(pairs):
        if not (0 <= i < Cn and 0 <= j < Cn and i != j):
            raise ValueError(f"pair {(i, j)} is not two different cameras of {Cn}")
        idx = np.flatnonzero(vis[i] & vis[j])
        use.append(idx)
        if len(idx) >= 8:
            lists.append((ip[i][idx], ip[j][idx]))
            tables.append(sample_table(len(idx), hypotheses, seed + k))
    ctx = ctx or default_context()
    res = iter(ctx.fundamental_ransac(lists, tables, threshold, refit=refit) if lists else [])
    out = []
    for idx in use:
        r = next(res) if len(idx) >= 8 else None
        if r is None or r["best"] < 0:
            out.append((None, None, r) if details else (None, None))
            continue
        mask = np.zeros((N, 1), np.uint8)
        mask[idx, 0] = r["mask"]
        F = _scaled_like_cv2(r["F_refit"] if refit else r["F_sample"])
        out.append((F, mask, r) if details else (F, mask))
    return out


def find_fundamental_matrix(points1, points2, threshold=10.0, hypotheses=1000, seed=0, refit=True, ctx=None):
    """`cv.findFundamentalMat(points1, points2, cv.FM_RANSAC, threshold, .)` -> (F, mask) on the GPU: x2^T F x1 = 0, F
    scaled to F[2, 2] = 1, mask uint8 [N, 1]; (None, None) when the pair fails.  Defaults: the reference's threshold of 10
    pixels (CalculateCameraPoses.py:189) and 1000 hypotheses, cv2's iteration cap for this overload.  ALL hypotheses are
    evaluated: there is no early exit by confidence on a GPU (the batch is one launch sequence; cv2's 0.99999 has no
    counterpart).  The 8-point solver stands in for cv2's 7-point one and the host's seeded generator for cv2's own, so the
    result is cv2's up to the choice of samples, not bit for bit.  refit: F is the 8-point fit over
    all inliers of the best sample (cv2 does the same); the mask is the best sample's."""
    p1 = np.asarray(points1, float)
    p2 = np.asarray(points2, float)
    if p1.ndim != 2 or p1.shape[1] != 2 or p1.shape != p2.shape:
        raise ValueError(f"points1 / points2 must both be [N][2], got {p1.shape} and {p2.shape}")
    if len(p1) < 8:
        raise ValueError(f"a fundamental matrix needs at least 8 point pairs, got {len(p1)}")
    if not (np.isfinite(p1).all() and np.isfinite(p2).all()):
        raise ValueError("points must be finite")
    if int(hypotheses) < 1:
        raise ValueError(f"hypotheses = {hypotheses}")
    return find_fundamental_matrices(np.stack([p1, p2]), [(0, 1)], None, threshold, hypotheses, seed, refit, ctx)[0]


def tracker_fundamentals(image_points, valid=None, threshold=10.0, hypotheses=1000, seed=0, refit=True, ctx=None):
    """Fs of the tracker (`mocap_set_fundamentals`, lib.Helpers.Fs): Fs[i - 1] = F(camera 0 -> camera i) for EVERY camera
    i = 1..C-1, estimated from wand points in one batched call.  (The reference only estimates the chain i -> i + 1 and
    writes each matrix twice, CalculateCameraPoses.py:190-191, which serves two cameras.)  Raises when a pair fails."""
    ip = np.asarray(image_points, float)
    pairs = [(0, i) for i in range(1, len(ip))]
    res = find_fundamental_matrices(ip, pairs, valid, threshold, hypotheses, seed, refit, ctx)
    for (i, j), (F, _) in zip(pairs, res):
        if F is None:
            raise ValueError(f"no fundamental matrix for cameras {i} -> {j}")
    return [F for F, _ in res]


def calculate_extrinsics(image_points, camera_params, threshold=10.0, hypotheses=1000, seed=0, refit=True, ctx=None):
    """reference `calculate_extrinsics` (CalculateCameraPoses.py:162-255) without plotting and file writing: RANSAC per
    consecutive camera pair (:189, one batched call here), E = K2^T F K1 and the four-candidate vote
    (`extrinsics_from_fundamentals`), bundle adjustment over the first two cameras (the reference's residual is
    two-camera, lib/Helpers.py:161-167), final triangulation and mean reprojection error.
    Returns dict: poses_initial, poses (after BA; cameras beyond the second keep their initial pose), pair_Fs (one per
    consecutive pair, for `save_fundamentals`), masks, votes (per link: the four candidates' cheirality counts),
    object_points [N][3], error (mean of the per-point reprojection MSE), ba_result (SciPy's)."""
    ctx = ctx or default_context()
    ip = np.asarray(image_points, float)
    if ip.ndim != 3 or ip.shape[0] < 2 or ip.shape[2] != 2:
        raise ValueError(f"image_points must be [C >= 2][N][2], got {ip.shape}")
    pairs = [(i, i + 1) for i in range(len(ip) - 1)]
    res = find_fundamental_matrices(ip, pairs, None, threshold, hypotheses, seed, refit, ctx)
    for (i, j), (F, _) in zip(pairs, res):
        if F is None:
            raise ValueError(f"no fundamental matrix for cameras {i} -> {j}")
    pair_Fs = [F for F, _ in res]
    K2, _ = _intrinsics(camera_params, 2)
    initial, votes = [{"R": np.eye(3), "t": np.zeros((3, 1))}], []
    for i, F in enumerate(pair_Fs):  # the loop of extrinsics_from_fundamentals, keeping each link's vote
        R1, R2, t = decompose_essential(K2[1].T @ F @ K2[0])
        link = select_relative_pose(ip[i], ip[i + 1], initial[-1], R1, R2, t, camera_params, ctx)
        initial.append(link["pose"])
        votes.append(link["counts"])
    two = np.transpose(ip[:2], (1, 0, 2))
    ba_poses, result = bundle_adjustment(two, initial[:2], camera_params, ctx=ctx)
    poses = [{"R": np.asarray(p["R"], float), "t": np.asarray(p["t"], float).reshape(3, 1)} for p in ba_poses] + initial[2:]
    n = len(poses)
    K, d = _intrinsics(camera_params, n)
    ctx.set_cameras(K, d, np.array([p["R"] for p in poses]), np.array([np.asarray(p["t"], float).reshape(3) for p in poses]))
    groups = np.transpose(ip, (1, 0, 2))
    ones = np.ones(groups.shape[:2], np.uint8)
    xyz, _ = ctx.triangulate_batch(groups, ones, compact_k=True)
    mse, _ = ctx.reproject_batch(groups, ones, xyz, compact_k=True)
    return {"poses_initial": initial, "poses": poses, "pair_Fs": pair_Fs, "masks": [m for _, m in res], "votes": votes,
            "object_points": xyz,
            "error": float(np.mean(mse)), "ba_result": result}


# ---- relative pose: four candidates, one launch -----------------------------------------------------------------
def select_relative_pose(points1, points2, base_pose, R1, R2, t, camera_params, ctx=None):
    """reference CalculateCameraPoses.py:199-231.  points1/points2 [N, 2] are the same markers seen by the previous
    and the new camera; candidates (R1, t), (R1, -t), (R2, t), (R2, -t) in that order (:201-202).  Every candidate is
    triangulated against `base_pose` (the reference passes `camera_poses[-1]`) with the intrinsics of cameras 0 and 1
    -- the reference indexes them by position in the two-pose list (lib/Helpers.py:59-61) -- and scored by the number
    of points with z > 0 plus the number with (R_i^T X).z > 0 (:214-219, the reference's expression, kept as is).
    The first candidate with the strictly largest score wins (:221).

    Returns dict: index, R, t (the winning candidate), pose (chained onto base_pose, :226-227), counts [4],
    object_points [4, N, 3]."""
    ctx = ctx or default_context()
    p1 = np.asarray(points1, float).reshape(-1, 2)
    p2 = np.asarray(points2, float).reshape(-1, 2)
    N = len(p1)
    assert len(p2) == N and N > 0
    t = np.asarray(t, float).reshape(3)
    cand_R = [np.asarray(R1, float), np.asarray(R1, float), np.asarray(R2, float), np.asarray(R2, float)]
    cand_t = [t, -t, t, -t]
    Rb, tb = np.asarray(base_pose["R"], float).reshape(3, 3), np.asarray(base_pose["t"], float).reshape(3)
    # cameras: 0 = base pose, 1..4 = candidates; group (i, n) sees cameras 0 and 1 + i, so "by position" the
    # intrinsics are those of cameras 0 and 1 for every candidate
    K, d = _intrinsics(camera_params, 2)
    ctx.set_cameras(np.array([K[0]] + [K[1]] * 4), np.array([d[0]] + [d[1]] * 4), np.array([Rb] + cand_R),
                    np.array([tb] + cand_t))
    pts = np.zeros((4 * N, 5, 2))
    valid = np.zeros((4 * N, 5), np.uint8)
    for i in range(4):
        pts[i * N:(i + 1) * N, 0] = p1
        pts[i * N:(i + 1) * N, 1 + i] = p2
        valid[i * N:(i + 1) * N, 0] = 1
        valid[i * N:(i + 1) * N, 1 + i] = 1
    xyz, _ = ctx.triangulate_batch(pts, valid, compact_k=True)
    xyz = xyz.reshape(4, N, 3)
    counts = []
    for i in range(4):
        in_candidate_frame = xyz[i] @ cand_R[i]  # rows = R_i^T X, reference :214
        counts.append(int(np.sum(xyz[i][:, 2] > 0) + np.sum(in_candidate_frame[:, 2] > 0)))
    best, most = None, 0
    for i in range(4):
        if counts[i] > most:
            best, most = i, counts[i]
    if best is None:
        raise ValueError("no candidate places a point in front of a camera (the reference fails here as well: R is None)")
    pose = {"R": cand_R[best] @ Rb, "t": tb.reshape(3, 1) + Rb @ cand_t[best].reshape(3, 1)}
    return {"index": best, "R": cand_R[best], "t": cand_t[best].reshape(3, 1), "pose": pose, "counts": counts,
            "object_points": xyz}


def extrinsics_from_fundamentals(image_points, Fs, camera_params, ctx=None):
    """The pose chain of reference `calculate_extrinsics` (:166-235) once the fundamental matrices are known.
    image_points [C][N][2] (the layout `get_points` returns, :80-89), Fs[i] maps camera i pixels to camera i+1 lines.
    Camera 0 is the identity; E = K2^T F K1 always uses the intrinsics of cameras 0 and 1 (:192-195)."""
    K, _ = _intrinsics(camera_params, 2)
    poses = [{"R": np.eye(3), "t": np.zeros((3, 1))}]
    for i in range(len(image_points) - 1):
        E = K[1].T @ np.asarray(Fs[i], float) @ K[0]
        R1, R2, t = decompose_essential(E)
        poses.append(select_relative_pose(image_points[i], image_points[i + 1], poses[-1], R1, R2, t, camera_params,
                                          ctx)["pose"])
    return poses


# ---- the whole rig: initial poses over a spanning tree, then bundle adjustment on the GPU ------------------------------------
def undistort_points(pts, K, dist, normalized=False):
    """`cv.undistortPoints(pts, K, dist, P=K)` on the host: the pinhole pixel each distorted pixel [..., 2] would have, by
    cv2's fixed-point iteration (5 rounds) on the Brown model.  normalized=True: the normalised coordinates (cv2 without P).
    Only the rig path uses it, for the linear steps of its initialisation (fundamental matrices, triangulation), which know
    no distortion; the bundle adjustment itself works on the distorted pixels."""
    pts = np.asarray(pts, float)
    K = np.asarray(K, float).reshape(3, 3)
    k1, k2, p1, p2, k3 = np.asarray(dist, float).ravel()[:5]
    x0, y0 = (pts[..., 0] - K[0, 2]) / K[0, 0], (pts[..., 1] - K[1, 2]) / K[1, 1]
    x, y = x0, y0
    for _ in range(5):
        r2 = x * x + y * y
        icd = 1.0 / (1 + ((k3 * r2 + k2) * r2 + k1) * r2)
        dx, dy = 2 * p1 * x * y + p2 * (r2 + 2 * x * x), p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
        x, y = (x0 - dx) * icd, (y0 - dy) * icd
    if normalized:
        return np.stack([x, y], -1)
    return np.stack([K[0, 0] * x + K[0, 2], K[1, 1] * y + K[1, 2]], -1)


def _rig_inputs(image_points, valid, camera_params):
    ip = np.asarray(image_points, float)
    if ip.ndim != 3 or ip.shape[2] != 2 or not 2 <= ip.shape[0] <= 32:
        raise ValueError(f"image_points must be [2..32 cameras][N][2], got {ip.shape}")
    Cn, N = ip.shape[:2]
    vis = np.ones((Cn, N), bool) if valid is None else np.asarray(valid).astype(bool).reshape(Cn, N)
    if len(camera_params) < Cn:
        raise ValueError(f"{Cn} cameras but {len(camera_params)} sets of camera parameters (they are indexed by camera number)")
    if not np.isfinite(ip[vis]).all():
        raise ValueError("image points marked valid must be finite")
    K, d = _intrinsics(camera_params, Cn)
    return np.where(vis[..., None], ip, 0.0), vis, K, d


def rig_initial_poses(image_points, valid, camera_params, threshold=10.0, hypotheses=1000, seed=0, ctx=None, details=False):
    """Consistent initial poses for every camera of a rig, camera 0 at the origin.  (The reference chains consecutive cameras
    link by link, CalculateCameraPoses.py:166-235, each link with a translation of length 1: for more than two cameras the
    chain has no common scale.)  image_points [C][N][2] distorted pixels, valid [C][N], camera_params indexed by camera.
      1. every camera pair with >= 8 common points: fundamental matrix by ONE batched GPU RANSAC (`find_fundamental_matrices`)
         on undistorted points;
      2. maximum spanning tree over the inlier counts from camera 0 (Prim; on a tie the lowest camera index, then the lowest
         parent index);
      3. per tree edge a -> b, breadth first: E = K_b^T F K_a, `decompose_essential`, the four candidates triangulated in one
         launch, the winner has strictly the most inliers in front of BOTH cameras (first on ties); R_b = R_ab R_a,
         t_b = R_ab t_a + s t_ab with s = 1 on the first edge and afterwards the median, over the edge's inliers that at least
         two cameras posed so far see, of (depth in camera a of the point triangulated from those cameras) / (its depth in
         the unit-baseline triangulation of the edge).
    Raises ValueError naming the camera when the graph is disconnected or no common point fixes a scale.  Returns the list
    of poses {"R": 3x3, "t": 3x1}; details=True: (poses, dict with tree [(a, b)], inliers, scales, votes)."""
    ip, vis, K, d = _rig_inputs(image_points, valid, camera_params)
    ctx = ctx or default_context()
    Cn, N = vis.shape
    und = np.stack([undistort_points(ip[c], K[c], d[c]) for c in range(Cn)])
    pairs = [(a, b) for a in range(Cn) for b in range(a + 1, Cn) if int((vis[a] & vis[b]).sum()) >= 8]
    res = find_fundamental_matrices(und, pairs, vis, threshold, hypotheses, seed, True, ctx, details=True) if pairs else []
    weight = np.zeros((Cn, Cn), np.int64)
    found = {}
    for (a, b), (F, mask, r) in zip(pairs, res):
        if F is not None:
            weight[a, b] = weight[b, a] = r["n_inliers"]
            found[(a, b)] = (np.asarray(r["F_refit"], float), mask[:, 0].astype(bool))
    parent = {0: None}
    while len(parent) < Cn:  # Prim
        best = None
        for b in range(Cn):
            if b in parent:
                continue
            for a in sorted(parent):
                if weight[a, b] > 0 and (best is None or weight[a, b] > best[0]):
                    best = (weight[a, b], a, b)
        if best is None:
            missing = [c for c in range(Cn) if c not in parent]
            raise ValueError(f"camera {missing[0]} shares no fundamental matrix (>= 8 common points, RANSAC succeeded) with the "
                             f"cameras connected to camera 0; not connected: {missing}")
        parent[best[2]] = best[1]
    edges, queue = [], [0]
    while queue:  # breadth first, children in ascending order
        a = queue.pop(0)
        for b in sorted(c for c, p in parent.items() if p == a):
            edges.append((a, b))
            queue.append(b)
    R = {0: np.eye(3)}
    t = {0: np.zeros(3)}
    info = {"tree": edges, "inliers": [], "scales": [], "votes": []}
    for k, (a, b) in enumerate(edges):
        F, inl = found[(a, b)] if a < b else found[(b, a)]
        F_ab = F if a < b else F.T
        R1, R2, tu = decompose_essential(K[b].T @ F_ab @ K[a])
        tu = tu.reshape(3)
        cand = [(R1, tu), (R1, -tu), (R2, tu), (R2, -tu)]
        idx = np.flatnonzero(inl)
        n = len(idx)
        # relative frame: camera a at the origin (slot 0), the four candidates for camera b in slots 1..4; group (i, point)
        ctx.set_cameras(np.array([K[a]] + [K[b]] * 4), np.zeros((5, 5)), np.array([np.eye(3)] + [c[0] for c in cand]),
                        np.array([np.zeros(3)] + [c[1] for c in cand]))
        pts = np.zeros((4 * n, 5, 2))
        val = np.zeros((4 * n, 5), np.uint8)
        for i in range(4):
            pts[i * n:(i + 1) * n, 0], pts[i * n:(i + 1) * n, 1 + i] = und[a][idx], und[b][idx]
            val[i * n:(i + 1) * n, 0] = val[i * n:(i + 1) * n, 1 + i] = 1
        xyz, ok = ctx.triangulate_batch(pts, val, compact_k=False)
        xyz, ok = xyz.reshape(4, n, 3), ok.reshape(4, n).astype(bool)
        votes = [int((ok[i] & (xyz[i][:, 2] > 0) & ((xyz[i] @ cand[i][0].T + cand[i][1])[:, 2] > 0)).sum()) for i in range(4)]
        win = int(np.argmax(votes))  # the first of equal maxima
        if votes[win] == 0:
            raise ValueError(f"camera {b}: no candidate pose places a point in front of cameras {a} and {b}")
        R_ab, t_ab = cand[win]
        s = 1.0
        if k > 0:
            posed = sorted(R)
            seen = vis[posed][:, idx].sum(0) >= 2
            if not seen.any():
                raise ValueError(f"camera {b}: no inlier of the pair {a} -> {b} is seen by two cameras posed before it; its scale is free")
            Kp, dp_ = np.array([K[c] for c in posed]), np.zeros((len(posed), 5))
            ctx.set_cameras(Kp, dp_, np.array([R[c] for c in posed]), np.array([t[c] for c in posed]))
            sel = idx[seen]
            g = np.ascontiguousarray(np.transpose(und[posed][:, sel], (1, 0, 2)))
            Xw, okw = ctx.triangulate_batch(g, vis[posed][:, sel].T.astype(np.uint8), compact_k=False)
            depth_w = (Xw @ R[a].T + t[a])[:, 2]
            depth_r = xyz[win][seen][:, 2]
            good = okw.astype(bool) & ok[win][seen] & (depth_w > 0) & (depth_r > 0)
            if not good.any():
                raise ValueError(f"camera {b}: no common point in front of camera {a} fixes the scale of the edge {a} -> {b}")
            s = float(np.median(depth_w[good] / depth_r[good]))
        R[b] = R_ab @ R[a]
        t[b] = R_ab @ t[a] + s * t_ab
        info["inliers"].append(n)
        info["scales"].append(s)
        info["votes"].append(votes)
    poses = [{"R": R[c], "t": t[c].reshape(3, 1)} for c in range(Cn)]
    return (poses, info) if details else poses


def _observation_problem(ip, vis, sel):
    """The observations vis [C][N] of the points sel, point-major with ascending cameras as the C-ABI wants them: (obs_offset
    [len(sel) + 1], camera [n_obs], index into sel [n_obs], uv [n_obs][2])"""
    v = vis[:, sel]
    n_idx, c_idx = np.nonzero(v.T)
    offset = np.zeros(len(sel) + 1, np.int32)
    np.cumsum(v.sum(0), out=offset[1:])
    return offset, c_idx.astype(np.int32), n_idx, ip[c_idx, sel[n_idx]]


def _residual_lengths(ip, vis, K, d, R, t, X):
    """|projection - pixel| [C][N] of the points X under the poses (R, t) with the full Brown model, NaN where vis is False or
    the point is NaN: the reporting of bundle_adjust_rig's refit (host; every value the solver works with is the GPU's)"""
    out = np.full(vis.shape, np.nan)
    with np.errstate(all="ignore"):
        for c in range(len(K)):
            p = X @ R[c].T + t[c]
            x, y = p[:, 0] / p[:, 2], p[:, 1] / p[:, 2]
            k1, k2, p1, p2, k3 = d[c]
            r2 = x * x + y * y
            cd = 1 + ((k3 * r2 + k2) * r2 + k1) * r2
            xd = x * cd + 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
            yd = y * cd + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
            e = np.hypot(K[c][0, 0] * xd + K[c][0, 2] - ip[c, :, 0], K[c][1, 1] * yd + K[c][1, 2] - ip[c, :, 1])
            out[c] = np.where(vis[c], e, np.nan)
    return out


def _check_loss(loss, loss_scale, inlier_weight):
    """True for a robust loss, after the checks that need no GPU"""
    if loss is None or loss == "none":
        return False
    if loss != "cauchy":
        raise ValueError(f"loss {loss!r}: None or 'cauchy' (Huber is not offered: DESIGN.md section 7)")
    if loss_scale is None:
        raise ValueError("loss='cauchy' needs loss_scale, the scale c in pixels: a few sigma of the pixel noise")
    if not (np.isfinite(loss_scale) and loss_scale > 0):
        raise ValueError(f"loss_scale = {loss_scale}: a finite number of pixels > 0")
    if not 0 < inlier_weight < 1:
        raise ValueError(f"inlier_weight = {inlier_weight}: between 0 and 1")
    return True


# what refine_intrinsics names: bit i frees parameter i of (fx, fy, cx, cy, k1, k2, p1, p2, k3)
REFINE_MASKS = {"focal": 0x003, "focal+center": 0x00F, "focal+center+radial2": 0x03F, "all": 0x1FF}


def _refine_masks(refine_intrinsics, Cn):
    """int32 [C] lens masks of bundle_adjust_rig_intrinsics' refine_intrinsics (None: None), after the checks that need no GPU"""
    if refine_intrinsics is None:
        return None
    if isinstance(refine_intrinsics, str):
        if refine_intrinsics not in REFINE_MASKS:
            raise ValueError(f"refine_intrinsics {refine_intrinsics!r}: None, one of {sorted(REFINE_MASKS)}, or an int mask per camera")
        refine_intrinsics = REFINE_MASKS[refine_intrinsics]
    masks = np.asarray(refine_intrinsics)
    if masks.dtype.kind not in "iu" or masks.ndim > 1 or (masks.ndim == 1 and len(masks) != Cn):
        raise ValueError(f"refine_intrinsics: one int mask, or one per camera ({Cn})")
    masks = np.ascontiguousarray(np.broadcast_to(masks, (Cn,)), np.int64)
    if ((masks < 0) | (masks > 0x1FF)).any():
        raise ValueError("refine_intrinsics: a mask has bits 0..8 (fx, fy, cx, cy, k1, k2, p1, p2, k3)")
    if Cn == 2 and (masks & ~REFINE_MASKS["focal"]).any():
        raise ValueError("refine_intrinsics: two views determine no more than the focal lengths ('focal', mask 0x003)")
    return masks.astype(np.int32)


def _camera_entries(kd):
    """camera_params entries, as calibrate_intrinsics returns and save_intrinsics writes them, from kd [C][9]"""
    return [{"intrinsic_matrix": np.array([[k[0], 0.0, k[2]], [0.0, k[1], k[3]], [0.0, 0.0, 1.0]]), "distortion_coef": k[4:].copy()}
            for k in np.asarray(kd, float)]


def bundle_adjust_rig(image_points, valid, poses, camera_params, points=None, max_iters=50, ftol=1e-12, ctx=None, loss=None,
                      loss_scale=None, inlier_weight=0.25, refit=True):
    """Bundle adjustment of ALL cameras of a rig and all 3-D points on the GPU, over exactly the observations that exist
    (engine.MocapContext.rig_bundle_adjust -> mocap_rig_bundle_adjust; definition in DESIGN.md section 2).  The reference's
    `bundle_adjustment` (lib/Helpers.py:158-176) refines camera 1 of two and drops every point a camera missed; it stays
    available unchanged.  image_points [C][N][2] distorted pixels, valid [C][N], poses: C poses {"R", "t"} to start from
    (`rig_initial_poses`), camera_params indexed by camera; points [N][3]: start points (None: triangulated from the start
    poses on undistorted pixels).  Residuals use the full Brown model of each camera, in FP64.  Camera 0 keeps its pose;
    the scale is fixed by |t_1 - R_1 R_0^T t_0|, the distance the start poses put between cameras 0 and 1.
    Returns dict: poses (list of {"R": 3x3, "t": 3x1}), points [N][3] (NaN where not used), used [N] bool (False: fewer than
    two views, or no start point in front of its cameras), cost_initial, cost (1/2 sum r^2), rms_px (per coordinate),
    iterations, history [iterations][4] (cost, lambda, accepted, |step|), status (MOCAP_RIG_STOP_*: 1 max_iters, 2 ftol,
    3 lambda, 4 Cholesky), mirrored (the start had every point behind every camera and was adjusted as its mirror image,
    see below).
    loss="cauchy", loss_scale=c: the adjustment weighs every observation by 1 / (1 + |r|^2 / c^2) (cost 1/2 sum c^2 log1p(|r|^2
    / c^2)), so that the ghost reflections and wrong-blob picks of a wand capture stop steering the
    poses.  loss_scale is required: it is the capture's pixel noise scale (a few sigma; 2 px for sigma 0.5 was what the tests
    use), and there is no honest default for it.  The dict gains obs_err_px [C][N] (length of the unweighted residual),
    obs_weight [C][N] and outliers [C][N] bool = obs_weight < inlier_weight (0.25: |r| > sqrt(3) c); where no observation
    was used the float arrays are NaN and outliers is False.  refit=True then runs a second, plain adjustment from the robust
    result over the observations that are not outliers (a point left with fewer than two views leaves `used`): poses, points,
    used, cost, rms_px, iterations, history and status are the refit's, the robust stage's are robust_cost (1/2 sum rho),
    robust_iterations and robust_status, obs_err_px is recomputed at the final state for every valid observation of the
    points still used (the rejected ones included), obs_weight and outliers stay the robust stage's.  refit=False: cost is
    1/2 sum rho and rms_px is taken over the observations that are not outliers.  cost_initial is the robust stage's, the 1/2
    sum rho of the start.  The defaults (loss=None) are the plain adjustment with the keys above and nothing else."""
    return _bundle_adjust_rig(image_points, valid, poses, camera_params, points, max_iters, ftol, ctx, loss, loss_scale, inlier_weight, refit)


def bundle_adjust_rig_intrinsics(image_points, valid, poses, camera_params, points=None, max_iters=50, ftol=1e-12, ctx=None, loss=None,
                                 loss_scale=None, inlier_weight=0.25, refit=True, refine_intrinsics="focal+center+radial2"):
    """`bundle_adjust_rig` with the cameras' lenses among the unknowns (engine.MocapContext.rig_bundle_adjust_intrinsics ->
    mocap_rig_bundle_adjust_intrinsics; definition in DESIGN.md section 2).  Thousands of wand points through the whole volume
    hold the lenses better than the board views camera_params came from.  Every argument but the last as `bundle_adjust_rig`'s.
    refine_intrinsics: which lens parameters of every camera, camera 0 included, join the unknowns: "focal" (fx, fy),
    "focal+center" (+ cx, cy), "focal+center+radial2" (+ k1, k2), "all" (+ p1, p2, k3), or an int mask (bit i frees parameter
    i of fx, fy, cx, cy, k1, k2, p1, p2, k3) for all cameras or one per camera.  Two cameras determine no more than "focal": a
    wider mask raises ValueError.  Returns `bundle_adjust_rig`'s dict plus camera_params (entries as `calibrate_intrinsics`
    returns and `save_intrinsics` writes them: the refined lenses; a parameter that was not free has the bits it came with)
    and intrinsics_start (the same form: what camera_params held, so that the caller sees what moved).  With loss="cauchy" both
    stages move the lenses, the refit under the same mask from the robust stage's result."""
    if refine_intrinsics is None:
        raise ValueError("refine_intrinsics: a name of REFINE_MASKS or int masks (bundle_adjust_rig leaves the lenses alone)")
    return _bundle_adjust_rig(image_points, valid, poses, camera_params, points, max_iters, ftol, ctx, loss, loss_scale, inlier_weight, refit,
                              refine_intrinsics)


def _bundle_adjust_rig(image_points, valid, poses, camera_params, points, max_iters, ftol, ctx, loss, loss_scale, inlier_weight, refit,
                       refine_intrinsics=None):
    """The one body of bundle_adjust_rig and bundle_adjust_rig_intrinsics (refine_intrinsics=None: the lenses stay)"""
    robust = _check_loss(loss, loss_scale, inlier_weight)
    ip, vis, K, d = _rig_inputs(image_points, valid, camera_params)
    Cn, N = vis.shape
    masks = _refine_masks(refine_intrinsics, Cn)
    lens = {} if masks is None else {"intrinsics": np.c_[K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2], d], "refine": masks}
    if len(poses) != Cn:
        raise ValueError(f"{len(poses)} poses for {Cn} cameras")
    ctx = ctx or default_context()
    Rw = np.array([np.asarray(p["R"], float).reshape(3, 3) for p in poses])
    tw = np.array([np.asarray(p["t"], float).reshape(3) for p in poses])
    # the device works with camera 0 as the world frame
    R0, t0 = Rw[0].copy(), tw[0].copy()
    R = np.array([Rw[c] @ R0.T for c in range(Cn)])
    t = np.array([tw[c] - R[c] @ t0 for c in range(Cn)])
    R[0], t[0] = np.eye(3), 0.0
    used = vis.sum(0) >= 2
    if points is None:
        und = np.stack([undistort_points(ip[c], K[c], d[c]) for c in range(Cn)])
        ctx.set_cameras(K, d, R, t)
        X, ok = ctx.triangulate_batch(np.ascontiguousarray(np.transpose(und, (1, 0, 2))), vis.T.astype(np.uint8), compact_k=False)
        used &= ok.astype(bool)
    else:
        X = np.asarray(points, float).reshape(N, 3) @ R0.T + t0
    with np.errstate(invalid="ignore"):
        depth = np.array([(X @ R[c].T + t[c])[:, 2] for c in range(Cn)])
        # (R, -t, -X) projects like (R, t, X) with every depth negated.  A start with EVERY point behind EVERY camera that sees
        # it is that mirror image of a proper one (the reference's candidate vote produces it for its bundled capture): it is
        # adjusted as its mirror image and handed back mirrored again, in the caller's convention.
        mirror = bool(used.any() and (depth[:, used][vis[:, used]] < 0).all())
        if mirror:
            t, X, depth = -t, -X, -depth
        front = ((depth > 0) | ~vis).all(0)
    used &= front & np.isfinite(X).all(1)
    if not used.any():
        raise ValueError("no point with two views and a start position in front of its cameras")
    sel = np.flatnonzero(used)
    offset, c_idx, n_idx, uv = _observation_problem(ip, vis, sel)
    ctx.set_cameras(K, d, R, t)
    start = np.c_[R.reshape(Cn, 9), t]
    extra = {}

    def adjust(offset, c_idx, uv, poses, pts, **loss_kw):
        if lens:
            return ctx.rig_bundle_adjust_intrinsics(offset, c_idx, uv, lens["intrinsics"], lens["refine"], poses, pts, max_iters, ftol, **loss_kw)
        return ctx.rig_bundle_adjust(offset, c_idx, uv, poses, pts, max_iters, ftol, **loss_kw)

    if not robust:
        out = adjust(offset, c_idx, uv, start, X[sel])
        rms = float(np.sqrt(out["cost"] / len(uv)))
    else:
        out = adjust(offset, c_idx, uv, start, X[sel], loss=loss, loss_scale=loss_scale)
        err, weight = np.full((Cn, N), np.nan), np.full((Cn, N), np.nan)
        err[c_idx, sel[n_idx]], weight[c_idx, sel[n_idx]] = out["obs_err"], out["obs_weight"]
        with np.errstate(invalid="ignore"):
            outliers = weight < inlier_weight  # (NaN: False)
        kept = ~np.isnan(weight) & ~outliers
        rms = float(np.sqrt(np.sum(err[kept] ** 2) / (2 * max(1, int(kept.sum())))))
        extra = {"obs_weight": weight, "outliers": outliers}
        if refit:
            used = used & (kept.sum(0) >= 2)
            if not used.any():
                raise ValueError("no point keeps two views that the robust stage did not reject")
            stage = out
            X1 = np.full((N, 3), np.nan)
            X1[sel] = stage["points"]
            sel = np.flatnonzero(used)
            offset, c_idx, n_idx, uv = _observation_problem(ip, kept, sel)
            # (the robust result is a state of the device's convention: camera 0 the world frame, mirrored if the start was)
            if lens:
                lens["intrinsics"] = stage["intrinsics"]
            out = adjust(offset, c_idx, uv, stage["poses"], X1[sel])
            out["cost_initial"] = stage["cost_initial"]
            rms = float(np.sqrt(out["cost"] / len(uv)))
            extra.update(robust_cost=stage["cost"], robust_iterations=stage["iterations"], robust_status=stage["status"])
            Xf = np.full((N, 3), np.nan)
            Xf[sel] = out["points"]
            Kf, df = (K, d) if not lens else _intrinsics(_camera_entries(out["intrinsics"]), Cn)
            err = _residual_lengths(ip, vis, Kf, df, out["poses"][:, :9].reshape(Cn, 3, 3), out["poses"][:, 9:], Xf)
        extra["obs_err_px"] = err
    Rn, tn, Xn = out["poses"][:, :9].reshape(Cn, 3, 3), out["poses"][:, 9:], out["points"]
    if mirror:
        tn, Xn = -tn, -Xn
    pts = np.full((N, 3), np.nan)
    pts[sel] = (Xn - t0) @ R0  # back to the caller's world frame
    new = [{"R": Rn[c] @ R0, "t": (tn[c] + Rn[c] @ t0).reshape(3, 1)} for c in range(Cn)]
    if lens:
        extra.update(camera_params=_camera_entries(out["intrinsics"]),
                     intrinsics_start=_camera_entries(np.c_[K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2], d]))
    return {"poses": new, "points": pts, "used": used, "cost_initial": out["cost_initial"], "cost": out["cost"], "rms_px": rms,
            "iterations": out["iterations"], "history": out["history"], "status": out["status"], "mirrored": mirror, **extra}


def calibrate_rig(image_points, valid, camera_params, threshold=10.0, hypotheses=1000, seed=0, max_iters=50, ftol=1e-12, ctx=None,
                  loss=None, loss_scale=None, inlier_weight=0.25, refit=True):
    """From the wand points of a whole rig to its extrinsics: `rig_initial_poses`, then `bundle_adjust_rig`.  The N-camera
    counterpart of `calculate_extrinsics` (which keeps the reference's two-camera behaviour).  Returns `bundle_adjust_rig`'s
    dict plus poses_initial and init (the initialisation's details); its poses and points go to `set_origin`, `set_floor` and
    `save_extrinsics` as the reference's do.  loss, loss_scale, inlier_weight, refit: `bundle_adjust_rig`'s (the RANSAC of
    the initialisation protects the start; loss="cauchy" protects the adjustment from the outliers of a real capture)."""
    return _calibrate_rig(image_points, valid, camera_params, threshold, hypotheses, seed, max_iters, ftol, ctx, loss, loss_scale,
                          inlier_weight, refit)


def calibrate_rig_intrinsics(image_points, valid, camera_params, threshold=10.0, hypotheses=1000, seed=0, max_iters=50, ftol=1e-12,
                             ctx=None, loss=None, loss_scale=None, inlier_weight=0.25, refit=True, refine_intrinsics="focal+center+radial2"):
    """`calibrate_rig` whose adjustment also refines the lenses camera_params holds: `rig_initial_poses` on camera_params as they
    came, then `bundle_adjust_rig_intrinsics`.  refine_intrinsics and the two keys the dict gains, camera_params (for
    `save_intrinsics`) and intrinsics_start: `bundle_adjust_rig_intrinsics`'s."""
    if refine_intrinsics is None:
        raise ValueError("refine_intrinsics: a name of REFINE_MASKS or int masks (calibrate_rig leaves the lenses alone)")
    return _calibrate_rig(image_points, valid, camera_params, threshold, hypotheses, seed, max_iters, ftol, ctx, loss, loss_scale,
                          inlier_weight, refit, refine_intrinsics)


def _calibrate_rig(image_points, valid, camera_params, threshold, hypotheses, seed, max_iters, ftol, ctx, loss, loss_scale, inlier_weight,
                   refit, refine_intrinsics=None):
    _check_loss(loss, loss_scale, inlier_weight)
    _refine_masks(refine_intrinsics, len(np.asarray(image_points)))
    ctx = ctx or default_context()
    initial, info = rig_initial_poses(image_points, valid, camera_params, threshold, hypotheses, seed, ctx, details=True)
    out = _bundle_adjust_rig(image_points, valid, initial, camera_params, None, max_iters, ftol, ctx, loss, loss_scale, inlier_weight, refit,
                             refine_intrinsics)
    out["poses_initial"], out["init"] = initial, info
    return out


# ---- intrinsics: every camera of a rig from board views, on the GPU ------------------------------------------------------------
def calibrate_intrinsics(views, image_sizes, start=None, max_iters=50, ftol=1e-12, ctx=None):
    """K and the five distortion coefficients of every camera of a rig from planar-board corner lists, in ONE call on the GPU
    (engine.MocapContext.intrinsics_calibrate -> mocap_intrinsics_calibrate; definition in DESIGN.md section 2).  The
    reference's counterpart is cv2.calibrateCamera(objpoints, imgpoints, size, None, None) per camera
    (CalculateCameraIntrinsic.py:58); finding the corners in the images (:35-45) stays with the caller.
    views[c]: the views of camera c, each (object points [n][2] or [n][3] with Z = 0 -- the board's corners in board
    coordinates --, image points [n][2] pixels), at least 3 views of at least 4 points and at least as many equations as unknowns, 2 points >=
    9 + 6 views (3 views of 4 points fall short: 24 for 27); image_sizes: (width, height), one pair
    for all cameras or one per camera; start: None, or per camera (camera_params entry, list of {"R", "t"} poses).
    Returns one dict per camera: intrinsic_matrix (3x3) and distortion_coef ([k1, k2, p1, p2, k3]) -- the entry is a
    camera_params entry as `calibrate_rig` and `save_intrinsics` take it --, poses (list of {"R": 3x3, "t": 3x1} board ->
    camera, one per view), rms_px (sqrt(2 cost / points): cv2.calibrateCamera's return value), view_rms [views], cost,
    cost_initial, status (MOCAP_RIG_STOP_*: 1 max_iters, 2 ftol, 3 lambda, 4 Cholesky; or MOCAP_INTR_E_*: -3 a start with a
    point behind its camera, -4 views that cannot tell the focal lengths: all fronto-parallel, for one), iterations, history
    [iterations][4] (cost, lambda, accepted, |step|).  A camera that failed (status < 0) is reported, not raised, so that one bad
    camera does not lose the others: its matrices are the start's (None without one) and its rms_px is NaN.  What the host
    can see before the call -- too few views or points (also fewer equations than unknowns: the loop would fit such a camera
    exactly and report a wrong lens with rms 0), shapes, a board that is not flat -- raises ValueError naming the camera."""
    n_cams = len(views)
    if n_cams < 1:
        raise ValueError("no cameras")
    sizes = np.asarray(image_sizes, np.int64)
    sizes = np.broadcast_to(sizes.reshape(-1, 2), (n_cams, 2)) if sizes.size == 2 else sizes.reshape(-1, 2)
    if len(sizes) != n_cams:
        raise ValueError(f"{len(sizes)} image sizes for {n_cams} cameras")
    if start is not None and len(start) != n_cams:
        raise ValueError(f"{len(start)} starts for {n_cams} cameras")
    voff, poff, objs, imgs = [0], [0], [], []
    for c, cam_views in enumerate(views):
        if len(cam_views) < 3:
            raise ValueError(f"camera {c}: {len(cam_views)} views, at least 3 are needed")
        for v, (obj, img) in enumerate(cam_views):
            obj, img = np.asarray(obj, float), np.asarray(img, float)
            if obj.ndim != 2 or obj.shape[1] not in (2, 3) or img.shape != (len(obj), 2):
                raise ValueError(f"camera {c}, view {v}: object points must be [n][2] or [n][3] and image points [n][2], got {obj.shape} and {img.shape}")
            if len(obj) < 4:
                raise ValueError(f"camera {c}, view {v}: {len(obj)} points, at least 4 are needed")
            if obj.shape[1] == 3 and (obj[:, 2] != 0).any():
                raise ValueError(f"camera {c}, view {v}: the board must be planar, Z = 0 in board coordinates")
            objs.append(obj[:, :2])
            imgs.append(img)
            poff.append(poff[-1] + len(obj))
        n_pts = poff[-1] - poff[voff[-1]]
        if 2 * n_pts < 9 + 6 * len(cam_views):
            raise ValueError(f"camera {c}: {n_pts} points in {len(cam_views)} views are {2 * n_pts} equations for "
                             f"{9 + 6 * len(cam_views)} unknowns, at least as many are needed")
        voff.append(voff[-1] + len(cam_views))
    begin = None
    if start is not None:
        kd0, poses0 = [], []
        for c, (entry, poses) in enumerate(start):
            if len(poses) != len(views[c]):
                raise ValueError(f"camera {c}: {len(poses)} start poses for {len(views[c])} views")
            K, d = np.asarray(entry["intrinsic_matrix"], float), np.asarray(entry["distortion_coef"], float).ravel()[:5]
            kd0.append(np.r_[K[0, 0], K[1, 1], K[0, 2], K[1, 2], d])
            poses0 += [np.r_[np.asarray(p["R"], float).reshape(9), np.asarray(p["t"], float).reshape(3)] for p in poses]
        begin = (np.array(kd0), np.array(poses0))
    ctx = ctx or default_context()
    out = ctx.intrinsics_calibrate(voff, poff, np.concatenate(objs), np.concatenate(imgs), sizes, begin, max_iters, ftol)
    result = []
    for c in range(n_cams):
        status, kd = int(out["status"][c]), out["kd"][c]
        ok, have = status > 0, status > 0 or start is not None
        n_pts = poff[voff[c + 1]] - poff[voff[c]]
        P = out["poses"][voff[c]:voff[c + 1]]
        result.append({
            "intrinsic_matrix": np.array([[kd[0], 0.0, kd[2]], [0.0, kd[1], kd[3]], [0.0, 0.0, 1.0]]) if have else None,
            "distortion_coef": kd[4:].copy() if have else None,
            "poses": [{"R": p[:9].reshape(3, 3).copy(), "t": p[9:].reshape(3, 1).copy()} for p in P] if have else None,
            "rms_px": float(np.sqrt(2.0 * out["cost"][c] / n_pts)) if ok else float("nan"),
            "view_rms": out["view_rms"][voff[c]:voff[c + 1]].copy(), "cost": float(out["cost"][c]),
            "cost_initial": float(out["cost_initial"][c]), "status": status, "iterations": int(out["iterations"][c]),
            "history": out["history"][c]})
    return result


# ---- bundle adjustment: residual and Jacobian in batched launches ---------------------------------------------------
def residuals_batched(image_points, param_sets, camera_params, ctx=None, problem=None):
    """Residual vectors (per-point reprojection MSE, float32 -- reference lib/Helpers.py:161-167) of S parameter
    vectors at once: ONE launch (mocap_ba_residuals: rotvec -> R, triangulation, reprojection and the float32 cast on
    the device, one workgroup per parameter vector) over image points that stay resident on the GPU.  Like the
    reference's residual, two cameras are assumed (identity + params[0:6]).  `problem`: the BAProblem of an earlier call
    with the same image points (bundle_adjustment keeps one for the whole optimisation)."""
    if problem is None:
        problem = ba_problem(image_points, camera_params, ctx)
    sets = np.array([np.asarray(p, float)[:6] for p in param_sets])
    return np.stack(problem.residuals(sets))


def ba_problem(image_points, camera_params, ctx=None):
    """Uploads the image points [N, 2, 2] of a two-camera bundle adjustment once (engine.BAProblem) and sets the two
    cameras' intrinsics in the context."""
    ctx = ctx or default_context()
    ip = np.asarray(image_points, float)
    assert ip.ndim == 3 and ip.shape[1:] == (2, 2), "the reference's residual is hard-wired to two cameras (lib/Helpers.py:162)"
    K, d = _intrinsics(camera_params, 2)
    ctx.set_cameras(K, d, np.stack([np.eye(3)] * 2), np.zeros((2, 3)))
    return ctx.ba_problem(ip)


def forward_difference_steps(x0, f_dtype=np.float32):
    """SciPy's default 2-point step (scipy.optimize._numdiff): sqrt(eps) * sign(x) * max(1, |x|) with sign(0) = +1 and
    eps that of the narrower of the parameter and residual dtypes -- float32 for the reference's residuals
    (lib/Helpers.py:165), i.e. a relative step of 3.45e-4."""
    x0 = np.asarray(x0, float)
    eps = np.finfo(np.float64).eps
    if np.issubdtype(f_dtype, np.inexact) and np.dtype(f_dtype).itemsize < 8:
        eps = np.finfo(f_dtype).eps
    sign = (x0 >= 0).astype(float) * 2 - 1
    return eps ** 0.5 * sign * np.maximum(1.0, np.abs(x0))


def residual_and_jacobian(image_points, x0, camera_params, ctx=None, problem=None):
    """(f0, J) with J exactly what `least_squares(jac='2-point')` derives from the float32 residuals: column i =
    (f(x0 + h_i e_i) - f0) / ((x0 + h_i e_i)_i - x0_i), the subtraction done in float32 as NumPy does for the
    reference's float32 residual vectors."""
    x0 = np.asarray(x0, float)
    h = forward_difference_steps(x0)
    sets = [x0]
    for i in range(len(x0)):
        x1 = x0.copy()
        x1[i] = x0[i] + h[i]
        sets.append(x1)
    f = residuals_batched(image_points, sets, camera_params, ctx, problem)
    f0 = f[0]
    J = np.empty((len(f0), len(x0)))
    for i in range(len(x0)):
        dx = sets[i + 1][i] - x0[i]
        J[:, i] = (f[i + 1] - f0) / dx
    return f0, J


def bundle_adjustment(image_points, camera_poses, camera_params, batched_jacobian=True, verbose=0, ctx=None):
    """reference lib/Helpers.py:158-176: trust-region least squares (SciPy 'trf', linear loss, ftol 1e-5, xtol 1e-15)
    over rotvec + translation of camera 1, residual = float32 per-point reprojection MSE of the re-triangulated
    points.  With `batched_jacobian` each Jacobian is two launches (see module docstring); without it SciPy
    differences the batched residual itself -- both walk the same iterates.  Returns the two poses, like
    `params_to_camera_poses(result.x)`."""
    from scipy import optimize
    from scipy.spatial.transform import Rotation

    from .lib.Helpers import params_to_camera_poses

    init = np.array([])
    for pose in camera_poses[1:]:
        init = np.concatenate([init, Rotation.from_matrix(np.asarray(pose["R"], float)).as_rotvec(),
                               np.asarray(pose["t"], float).flatten()])

    problem = ba_problem(image_points, camera_params, ctx)  # image points resident for the whole optimisation

    def fun(x):
        return residuals_batched(image_points, [x], camera_params, ctx, problem)[0]

    def jac(x):
        return residual_and_jacobian(image_points, x, camera_params, ctx, problem)[1]

    result = optimize.least_squares(fun, init, jac=jac if batched_jacobian else "2-point", verbose=verbose, loss="linear",
                                    method="trf", ftol=1e-5, xtol=1e-15)
    return params_to_camera_poses(result.x), result


# ---- origin and floor ---------------------------------------------------------------------------------------------------
def set_origin(camera_poses, points_3d):
    """reference :283-294: subtract the mean of the floor points from every camera's t (in place); returns the
    origin, or None when fewer than three points were given."""
    points_3d = np.asarray(points_3d, float)
    if len(points_3d) > 2:
        origin = np.mean(points_3d, axis=0)
        for pose in camera_poses:
            pose["t"] = pose["t"] - origin
        return origin
    return None


def calculate_normal(points_3d):
    """reference :326-333: unit normal of three points (0 when they are collinear)."""
    if len(points_3d) == 3:
        p = [np.asarray(q, float) for q in points_3d]
        normal = np.cross(p[1] - p[0], p[2] - p[0])
        return 0 if np.linalg.norm(normal) == 0 else normal / np.linalg.norm(normal)
    return np.array([0, 0, 1])


def rotation_matrix_from_vectors(vec_orig, vec_rot):
    """reference :335-363: Rodrigues rotation taking vec_orig onto vec_rot.  Follows the reference's function nearly line
    for line (the same case split and the same formula), so that `set_floor` rotates exactly as the reference does."""
    a = np.asarray(vec_orig, float) / np.linalg.norm(vec_orig)
    b = np.asarray(vec_rot, float) / np.linalg.norm(vec_rot)
    cross = np.cross(a, b)
    cross_norm = np.linalg.norm(cross)
    dot = np.dot(a, b)
    if cross_norm == 0:
        if dot > 0:
            return np.eye(3)
        axis = np.array([1.0, 0.0, 0.0]) if abs(a[0]) < 0.99 else np.array([0.0, 1.0, 0.0])
        cross = np.cross(a, axis)
        cross /= np.linalg.norm(cross)
        cross_norm = 1
    Kx = np.array([[0, -cross[2], cross[1]], [cross[2], 0, -cross[0]], [-cross[1], cross[0], 0]])
    return np.eye(3) + Kx + Kx @ Kx * ((1 - dot) / (cross_norm ** 2))


def set_floor(camera_poses, points_3d):
    """reference :296-324: mean normal over all point triples, rotation taking (0, 0, -1) onto it, every pose
    [R|t] <- Rf^T [R|t] (in place; t becomes a (3, 1) column).  Returns the 3x3 rotation, or None when fewer than
    three points were given."""
    if len(points_3d) <= 2:
        return None
    normals = [calculate_normal([points_3d[a], points_3d[b], points_3d[c]])
               for a, b, c in combinations(range(len(points_3d)), 3)]
    normal = np.mean(normals, axis=0)
    Rf = rotation_matrix_from_vectors(np.array([0, 0, -1]), normal)
    for pose in camera_poses:
        RT = np.eye(4)
        RT[:3, :3] = pose["R"]
        RT[:3, 3] = np.asarray(pose["t"], float).flatten()
        R4 = np.eye(4)
        R4[:3, :3] = Rf
        RT = R4.T @ RT
        pose["R"] = RT[:3, :3]
        pose["t"] = RT[:3, 3].reshape(3, 1)
    return Rf


# ---- stage files: the JSON artefacts the reference's stages hand to each other ----------------------
def get_points(path="./jsons/image_points.json"):
    """reference `get_points` (:80-89): jsons/image_points.json holds [point][camera][2]; returned as
    [camera][point][2]."""
    with open(path) as file:
        image_points = json.load(file)
    return np.transpose(np.array(image_points), (1, 0, 2))


def save_extrinsics(camera_poses, prefix="", directory="./jsons", camera_count=None):
    """reference `save_extrinsics` (:257-273) without its module globals: writes `{directory}/{prefix}extrinsics.json`
    = [{"R": 3x3 list, "t": flat list of 3}, ...], the layout `lib.Helpers.get_extrinsics` reads back (:282-291).
    Returns the file name."""
    n = len(camera_poses) if camera_count is None else camera_count
    extrinsics = []
    for i in range(0, n):
        extrinsics.append({"R": np.asarray(camera_poses[i]["R"]).tolist(),
                           "t": np.asarray(camera_poses[i]["t"]).flatten().tolist()})
    extrinsics_filename = f"{directory}/{prefix}extrinsics.json"
    with open(extrinsics_filename, "w") as outfile:
        json.dump(extrinsics, outfile)
    print("Extrinsics saved to", extrinsics_filename)
    return extrinsics_filename


def save_intrinsics(entry, path="./jsons/camera-intrinsics.json"):
    """The file reference CalculateCameraIntrinsic.py:77-84 writes: {"intrinsic_matrix": 3x3 list, "distortion_coef": list of
    5} (`dist[0]` of cv2.calibrateCamera's 1x5 array), the layout `lib.Helpers` reads back as a camera_params entry.  entry: a
    dict of `calibrate_intrinsics`, or any camera_params entry.  Returns the file name."""
    intrinsics = {"intrinsic_matrix": np.asarray(entry["intrinsic_matrix"], float).reshape(3, 3).tolist(),
                  "distortion_coef": np.asarray(entry["distortion_coef"], float).ravel().tolist()}
    with open(path, "w") as outfile:
        json.dump(intrinsics, outfile)
    return path


def save_objects(prefix="", object_points=None, directory="./jsons"):
    """reference `save_objects` (:275-281): `{directory}/{prefix}objects.json` = [[x, y, z], ...]."""
    objects_filename = f"{directory}/{prefix}objects.json"
    with open(objects_filename, "w") as outfile:
        json.dump(np.asarray(object_points).tolist(), outfile)
    print("Object points saved to", objects_filename)
    return objects_filename


def save_fundamentals(pair_Fs, directory="./jsons"):
    """The fundamentals.json dump of reference `calculate_extrinsics` (:189-191,236-240): every camera pair's F is
    appended TWICE (`Fs.append(F.tolist())` twice), so that `lib.Helpers.Fs[i - 1]` of a two-camera rig finds its
    matrix at index 0 and a copy at index 1.  pair_Fs: one 3x3 matrix per consecutive camera pair."""
    Fs = []
    for F in pair_Fs:
        Fs.append(np.asarray(F, float).tolist())
        Fs.append(np.asarray(F, float).tolist())
    filename = f"{directory}/fundamentals.json"
    with open(filename, "w") as outfile:
        json.dump(Fs, outfile)
    return filename


def pair_fundamentals(Fs):
    """Inverse of `save_fundamentals`' doubling: the one-per-pair list `extrinsics_from_fundamentals` expects from
    the list a fundamentals.json written by the reference holds (entries 0, 2, 4, ...)."""
    return [np.asarray(F, float) for F in Fs[::2]]


__all__ = ["poses_to_fundamental_matrix", "decompose_essential", "select_relative_pose", "extrinsics_from_fundamentals",
           "residuals_batched", "forward_difference_steps", "residual_and_jacobian", "bundle_adjustment", "set_origin",
           "calculate_normal", "rotation_matrix_from_vectors", "set_floor", "get_points", "save_extrinsics", "save_objects",
           "save_fundamentals", "pair_fundamentals", "sample_table", "find_fundamental_matrix", "find_fundamental_matrices",
           "tracker_fundamentals", "calculate_extrinsics", "undistort_points", "rig_initial_poses", "bundle_adjust_rig",
           "calibrate_rig", "calibrate_intrinsics", "save_intrinsics"]
