#!/usr/bin/env python3
"""Generate tests/golden/*.npz by running the REFERENCE's own lib/Helpers.py.

Runs only in the build container (needs /root/reference, which never travels).  The reference
source is imported from where it lies; nothing of it is copied into this repository -- the
fixtures hold inputs and outputs only.

Provenance of every fixture (recorded in each file's `provenance` field):
  * `reference`      : produced by reference code that touches only NumPy/SciPy
                       (triangulate_point(s), get_extrinsics, read_camera_params).
  * `reference+cvstub`: produced by the reference's control flow, with the two OpenCV primitives it
                       calls -- cv.computeCorrespondEpilines (Helpers.py:207) and cv.projectPoints
                       (Helpers.py:133) -- supplied by the closed-form NumPy stand-ins below, because
                       cv2 is not installed here.

Usage:  python oracle/gen_golden.py            (writes tests/golden/)
        python oracle/gen_golden.py calib      (only tests/golden/calib_cheirality.npz)
        python oracle/gen_golden.py mixed      (only the rigs of unequal cameras: corr_*_mixed*.npz, reproj_none_mixed.npz,
                                                ba_residuals_mixed.npz)
"""
import copy
import json
import os
import sys
import types

import numpy as np

REF = "/root/reference"
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden")
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


# ---- closed-form stand-ins for the two cv2 calls made by lib/Helpers.py -------------------------
def _epilines(points, which, F):
    pts = np.asarray(points, np.float32).reshape(-1, 2)
    f = np.asarray(F, np.float64)
    if which == 2:
        f = f.T
    out = np.zeros((len(pts), 1, 3), np.float32)
    for i, (x, y) in enumerate(pts):
        x, y = float(x), float(y)
        a = f[0, 0] * x + f[0, 1] * y + f[0, 2]
        b = f[1, 0] * x + f[1, 1] * y + f[1, 2]
        c = f[2, 0] * x + f[2, 1] * y + f[2, 2]
        nu = a * a + b * b
        nu = 1.0 / np.sqrt(nu) if nu else 1.0
        out[i, 0] = (np.float32(a * nu), np.float32(b * nu), np.float32(c * nu))
    return out


def _project_points(obj, R, t, K, dist):
    obj = np.asarray(obj)
    out_t = np.float32 if obj.dtype == np.float32 else np.float64
    P = obj.astype(np.float64).reshape(-1, 3)
    R = np.asarray(R, np.float64).reshape(3, 3)
    t = np.asarray(t, np.float64).reshape(3)
    K = np.asarray(K, np.float64)
    k = np.zeros(5)
    d = np.asarray(dist, np.float64).ravel()
    k[: len(d)] = d[:5]
    res = np.zeros((len(P), 1, 2), out_t)
    for i, (X, Y, Z) in enumerate(P):
        x = R[0, 0] * X + R[0, 1] * Y + R[0, 2] * Z + t[0]
        y = R[1, 0] * X + R[1, 1] * Y + R[1, 2] * Z + t[1]
        z = R[2, 0] * X + R[2, 1] * Y + R[2, 2] * Z + t[2]
        z = 1.0 / z if z else 1.0
        x *= z
        y *= z
        r2 = x * x + y * y
        r4 = r2 * r2
        r6 = r4 * r2
        a1 = 2 * x * y
        a2 = r2 + 2 * x * x
        a3 = r2 + 2 * y * y
        cdist = 1 + k[0] * r2 + k[1] * r4 + k[4] * r6
        xd = x * cdist + k[2] * a1 + k[3] * a2
        yd = y * cdist + k[2] * a3 + k[3] * a1
        res[i, 0] = (xd * K[0, 0] + K[0, 2], yd * K[1, 1] + K[1, 2])
    return res, None


def load_reference():
    stub = types.ModuleType("cv2")
    stub.computeCorrespondEpilines = _epilines
    stub.projectPoints = _project_points
    sys.modules["cv2"] = stub
    sys.dont_write_bytecode = True
    sys.path.insert(0, REF)
    os.chdir(REF)  # the reference opens ./jsons/... relative to the CWD
    import lib.Helpers as H  # noqa: E402

    return H


def poses_arrays(poses):
    return (np.stack([np.asarray(p["R"], float) for p in poses]),
            np.stack([np.asarray(p["t"], float).reshape(3) for p in poses]))


def params_arrays(params):
    return (np.stack([np.asarray(p["intrinsic_matrix"], float) for p in params]),
            np.stack([np.asarray(p["distortion_coef"], float) for p in params]))


def pack_lists(lists, max_pts):
    """[C] lists of [x,y] -> (pts [C,max_pts,2] float64, counts [C])"""
    C = len(lists)
    pts = np.zeros((C, max_pts, 2))
    cnt = np.zeros(C, np.int32)
    for c, l in enumerate(lists):
        l = [p for p in l if p[0] is not None]
        cnt[c] = len(l)
        if l:
            pts[c, : len(l)] = np.asarray(l, float)
    return pts, cnt


def run_corr(H, lists, poses, params, Fs, obj_count):
    H.camera_params = np.array(params)
    H.Fs = [np.asarray(F).tolist() for F in Fs]
    arg = copy.deepcopy(lists)
    obj, img = H.find_point_correspondance_and_object_points(arg, poses, obj_count)
    return np.asarray(obj, float), np.asarray(img), arg


def save_corr(name, H, lists, poses, params, Fs, obj_count, note):
    obj, img, mutated = run_corr(H, lists, poses, params, Fs, obj_count)
    max_pts = max(1, max(len(l) for l in lists))
    pts, cnt = pack_lists(lists, max_pts)
    R, t = poses_arrays(poses)
    K, dist = params_arrays(params)
    had_sentinel = np.array([any(p[0] is None for p in l) for l in lists])
    np.savez_compressed(
        os.path.join(OUT, name + ".npz"), pts=pts, counts=cnt, had_sentinel=had_sentinel, R=R, t=t, K=K, dist=dist,
        F=np.asarray(Fs, float).reshape(-1, 3, 3), obj_count=obj_count,
        out_obj=obj, out_img=img.astype(float), out_img_is_int=np.array(img.dtype.kind in "iu"),
        out_obj_shape=np.array(obj.shape), out_img_shape=np.array(img.shape),
        mutated_counts=np.array([len(l) for l in mutated]),
        provenance="reference+cvstub: lib/Helpers.py:178-280 run in the build container; " + note)
    print(f"{name}: obj {obj.shape} img {img.shape}")


def decompose_essential(E):
    """closed form of cv.decomposeEssentialMat (CalculateCameraPoses.py:197): E = U diag(1,1,0) Vt with det(U) =
    det(Vt) = +1, R1 = U W Vt, R2 = U W^T Vt, t = U[:, 2]"""
    U, _, Vt = np.linalg.svd(np.asarray(E, float))
    if np.linalg.det(U) < 0:
        U = -U
    if np.linalg.det(Vt) < 0:
        Vt = -Vt
    W = np.array([[0.0, 1.0, 0.0], [-1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    return U @ W @ Vt, U @ W.T @ Vt, U[:, 2].reshape(3, 1)


def gen_calibration(H):
    """Calibration chain on the bundled capture (CalculateCameraPoses.py:177-231): jsons/fundamentals.json +
    camera-params-in.json + image_points.json -> the four (R, t) candidates, the reference's triangulate_points for
    each, the cheirality counts and the chosen pose, which must be jsons/before_ba_extrinsics.json[1]."""
    with open("jsons/image_points.json") as f:
        ip = np.array(json.load(f))  # [54][2][2]
    with open("jsons/camera-params-in.json") as f:
        params = json.load(f)
    with open("jsons/fundamentals.json") as f:
        F = np.array(json.load(f)[0])
    with open("jsons/before_ba_extrinsics.json") as f:
        before = json.load(f)
    K, dist = params_arrays(params)
    H.camera_params = np.array(params)
    E = K[1].T @ F @ K[0]  # :195
    R1, R2, t = decompose_essential(E)
    cand_R = [R1, R1, R2, R2]  # :201-202
    cand_t = [t, -t, t, -t]
    base = {"R": np.eye(3), "t": np.array([[0], [0], [0]], dtype=np.float32)}  # :179-182
    objs, counts = [], []
    for i in range(4):
        o = H.triangulate_points(ip, np.concatenate([[base], [{"R": cand_R[i], "t": cand_t[i]}]]))  # :213
        oc = np.array([cand_R[i].T @ p for p in o])  # :214
        objs.append(o)
        counts.append(int(np.sum(o[:, 2] > 0) + np.sum(oc[:, 2] > 0)))  # :219
    best = int(np.argmax(counts))  # first maximum, as the strict '>' of :221 keeps it
    R = cand_R[best] @ base["R"]  # :226
    tt = base["t"] + base["R"] @ cand_t[best]  # :227
    # The bundled before_ba_extrinsics.json pins the decomposition: its camera-1 pose is one of the four candidates to
    # 1e-15.  It is the mirrored twin of the candidate the selection rule above picks (the bundled object points all
    # have z < 0), i.e. that JSON was written by another revision of the selection; both facts are recorded.
    Rb, tb = np.array(before[1]["R"]), np.array(before[1]["t"])
    twin = [i for i in range(4) if np.abs(cand_R[i] - Rb).max() < 1e-12 and np.abs(cand_t[i].ravel() - tb).max() < 1e-12]
    assert len(twin) == 1, "before_ba_extrinsics.json is not among the candidates"
    assert np.abs(cand_R[twin[0]] - cand_R[best]).max() < 1e-12 and np.abs(cand_t[twin[0]] + cand_t[best]).max() < 1e-12
    np.savez_compressed(
        os.path.join(OUT, "calib_cheirality.npz"), image_points=ip, K=K, dist=dist, F=F, cand_R=np.array(cand_R),
        cand_t=np.array(cand_t).reshape(4, 3), objects=np.array(objs), counts=np.array(counts), best=best,
        chosen_R=R, chosen_t=np.asarray(tt, float).reshape(3), before_ba_R=Rb, before_ba_t=tb,
        before_ba_candidate=twin[0],
        provenance="reference+cvstub: lib/Helpers.py:87-99 run on the four candidates of CalculateCameraPoses.py:195-231; "
                   "cv.decomposeEssentialMat supplied by its closed form; jsons/before_ba_extrinsics.json[1] equals "
                   "candidate `before_ba_candidate` to 1e-12 (asserted when generated)")
    print("calib_cheirality: counts", counts, "best", best)


TRI_NONE_MASKS = [(1, 1, 1, 1), (0, 1, 1, 1), (1, 0, 1, 1), (1, 1, 0, 0), (0, 0, 1, 1), (1, 0, 0, 0), (0, 0, 0, 0)]


def capture_residual_function(H, image_points, poses):
    """residual_function of lib/Helpers.py:161-167, taken out of bundle_adjustment through a patched least_squares"""
    captured = {}

    def capture(fun, x0, **kw):
        captured["fun"], captured["x0"] = fun, np.array(x0)

        class R_:
            x = np.array(x0)

        return R_()

    orig = H.optimize.least_squares
    H.optimize.least_squares = capture
    try:
        H.bundle_adjustment(image_points, poses)
    finally:
        H.optimize.least_squares = orig
    return captured["fun"], captured["x0"]


def gen_mixed(H):
    """Rigs whose cameras all differ in K and lens (mocapv2_amd.synth.MixedScene): a read of the wrong camera's intrinsics
    changes every one of these outputs."""
    from mocapv2_amd.synth import MixedScene, MIXED_DISTS  # noqa: E402

    def mixed_case(name, C, M, seed, obj_count, jitter, drop=None, extra=0):
        sc = MixedScene(C)
        rng = np.random.default_rng(seed)
        cents = sc.centroids(sc.markers(rng, M), rng, jitter)
        lists = []
        for c in range(C):
            l = [[int(x), int(y)] for x, y in cents[c]]
            if drop and c in drop:
                l = l[: len(l) - drop[c]]
            for _ in range(extra):
                l.append([int(rng.integers(0, sc.width)), int(rng.integers(0, sc.height))])
            lists.append([l[i] for i in rng.permutation(len(l))])
        save_corr(name, H, lists, sc.poses, sc.camera_params, sc.Fs, obj_count,
                  f"synthetic ring of unequal cameras (MixedScene) C={C} M={M} seed={seed}")

    mixed_case("corr_c4_m6_mixed", 4, 6, 108, 6, jitter=0.5)
    mixed_case("corr_c6_m8_mixed_clutter", 6, 8, 109, 8, jitter=0.7, drop={3: 2}, extra=3)

    # triangulate_point and calculate_reprojection_error with [None, None] entries: both index camera_params by position after
    # the entries are dropped (Helpers.py:59-61, :137-138); here the positions carry different K AND different lenses
    sc = MixedScene(4)
    rng = np.random.default_rng(17)
    mk = sc.markers(rng, 6)
    cents = sc.centroids(mk, rng, 0.5)
    H.camera_params = np.array(sc.camera_params)
    groups, tri, obj, mse = [], [], [], []
    for m, msk in enumerate(TRI_NONE_MASKS):
        g = [[int(cents[c][m % 6][0]), int(cents[c][m % 6][1])] if msk[c] else [None, None] for c in range(4)]
        r = H.triangulate_point(copy.deepcopy(g), sc.poses)
        X = mk[m % 6] + rng.normal(0, 2e-3, 3)  # the point handed to the reprojection: near the marker, not the DLT's answer
        e = H.calculate_reprojection_error(copy.deepcopy(g), X, sc.poses)
        tri.append([np.nan] * 3 if r[0] is None else list(r))
        obj.append(X)
        mse.append(np.nan if e is None else float(e))
        groups.append([[np.nan, np.nan] if p[0] is None else p for p in g])
    R4, t4 = poses_arrays(sc.poses)
    K4, d4 = params_arrays(sc.camera_params)
    np.savez_compressed(os.path.join(OUT, "reproj_none_mixed.npz"), groups=np.array(groups, float), R=R4, t=t4, K=K4, dist=d4,
                        out=np.array(tri, float), obj=np.array(obj, float), mse=np.array(mse, float),
                        provenance="reference: lib/Helpers.py:43-84 (out) and reference+cvstub: :113-143 (mse of obj) with "
                                   "[None,None] entries (NaN here) on four cameras of different K and lens")
    print("reproj_none_mixed: mse", np.array(mse))

    # residual_function (Helpers.py:161-167) on 600 groups of a two-camera rig with two different lenses, 5 % of the groups
    # holding a [None, None]: triangulate_points skips those (:93) and calculate_reprojection_errors pairs what is left
    # positionally (:104).  A stereo pair with a small relative rotation, so that the parameter vector with a ZERO rotation
    # vector is still a well-conditioned triangulation.
    full = MixedScene(4)
    params = [full.camera_params[3], full.camera_params[2]]  # tangential + k3 barrel, pincushion
    Ka, Kb = full.Ks[3], full.Ks[2]
    rng = np.random.default_rng(23)
    N = 600
    from scipy.spatial.transform import Rotation
    w = np.array([0.02, -0.05, 0.03])
    Rrel = Rotation.from_rotvec(w).as_matrix()
    trel = -Rrel @ np.array([0.8, 0.05, 0.0])
    X = np.c_[rng.uniform(-0.6, 0.6, (N, 2)), rng.uniform(2.8, 3.8, N)]
    Xb = X @ Rrel.T + trel
    pa = np.c_[Ka[0, 0] * X[:, 0] / X[:, 2] + Ka[0, 2], Ka[1, 1] * X[:, 1] / X[:, 2] + Ka[1, 2]]
    pb = np.c_[Kb[0, 0] * Xb[:, 0] / Xb[:, 2] + Kb[0, 2], Kb[1, 1] * Xb[:, 1] / Xb[:, 2] + Kb[1, 2]]
    ip = np.floor(np.stack([pa, pb], 1) + rng.normal(0, 0.5, (N, 2, 2)))
    valid = np.ones((N, 2), bool)
    holes = rng.choice(N, 30, replace=False)
    valid[holes, rng.integers(0, 2, 30)] = False
    assert all(((holes >= lo) & (holes < hi)).any() for lo, hi in ((0, 256), (256, 512), (512, N)))
    as_lists = [[[float(p[0]), float(p[1])] if v else [None, None] for p, v in zip(g, vg)] for g, vg in zip(ip, valid)]
    H.camera_params = np.array(params)
    fun, x0 = capture_residual_function(H, as_lists, [{"R": np.eye(3), "t": np.zeros(3)}, {"R": Rrel, "t": trel}])
    assert np.abs(x0 - np.r_[w, trel]).max() < 1e-12
    xs = [x0, x0 + rng.normal(0, 1e-3, 6), np.r_[0.0, 0.0, 0.0, trel + rng.normal(0, 1e-3, 3)]]
    res = [np.asarray(fun(x)) for x in xs]
    assert all(r.dtype == np.float32 and np.isfinite(r).all() for r in res)
    Kp, dp = params_arrays(params)
    np.savez_compressed(os.path.join(OUT, "ba_residuals_mixed.npz"), image_points=np.where(valid[..., None], ip, np.nan),
                        valid=valid, params=np.array(xs), residuals=np.array(res), K=Kp, dist=dp,
                        provenance="reference+cvstub: residual_function of lib/Helpers.py:161-167 captured through a patched "
                                   "scipy.optimize.least_squares; two cameras of different K and lens, 30 of 600 groups with a "
                                   "[None,None] (NaN here) in all three 256-group rounds, params[2] has a zero rotation vector")
    print("ba_residuals_mixed:", np.array(res).shape, "median", np.median(res, 1), "max", np.max(res, 1))


def main():
    os.makedirs(OUT, exist_ok=True)
    H = load_reference()
    if len(sys.argv) > 1 and sys.argv[1] == "calib":  # only the calibration fixture
        gen_calibration(H)
        return
    if len(sys.argv) > 1 and sys.argv[1] == "mixed":  # only the rigs of unequal cameras
        gen_mixed(H)
        return
    gen_calibration(H)
    from mocapv2_amd.synth import Scene, MILD_DIST  # noqa: E402

    # ---- K1: bundled DLT known-answer --------------------------------------------------------
    poses, _ = H.get_extrinsics()
    with open("jsons/image_points.json") as f:
        ip = np.array(json.load(f))  # [54][2][2]
    with open("jsons/after_ba_objects.json") as f:
        expected = np.array(json.load(f))
    with open("jsons/camera-params-in.json") as f:
        params = json.load(f)
    with open("jsons/fundamentals.json") as f:
        Fs_b = json.load(f)
    H.camera_params = None
    got = H.triangulate_points(ip, poses)
    assert np.abs(got - expected).max() < 1e-12
    R, t = poses_arrays(poses)
    K, dist = params_arrays(params)
    # reprojection errors of the same 54 groups (cv.projectPoints stand-in)
    errs = H.calculate_reprojection_errors(ip, got, poses)
    # K2: epipolar distances of the 54 pairs under fundamentals.json[0] (expression of Helpers.py:217)
    dists = []
    for (p0, p1) in ip:
        a, b, c = _epilines(np.array([p0], np.float32), 1, np.array(Fs_b[0]))[0, 0].tolist()
        pts1 = np.array([p1])
        dists.append((np.abs(a * pts1[:, 0] + b * pts1[:, 1] + c) / np.sqrt(a ** 2 + b ** 2))[0])
    np.savez_compressed(
        os.path.join(OUT, "k1_bundled.npz"), image_points=ip, R=R, t=t, K=K, dist=dist,
        F=np.asarray(Fs_b, float), objects_json=expected, objects_ref=got, reproj_mse=errs,
        epi_dist=np.array(dists),
        provenance="reference: lib/Helpers.py:87-99 on jsons/image_points.json + after_ba_extrinsics.json "
                   "(= jsons/after_ba_objects.json to 3e-15); reproj_mse/epi_dist: reference+cvstub")
    print("k1_bundled: max|ref-json| =", np.abs(got - expected).max(), " epi max", max(dists))

    # triangulate_point with None entries (intrinsics indexed by position after removal, Helpers.py:50-61)
    sc = Scene(4, dist=MILD_DIST)
    rng = np.random.default_rng(7)
    mk = sc.markers(rng, 6)
    cents = sc.centroids(mk)
    prm4 = copy.deepcopy(sc.camera_params)
    for c in range(4):  # make the intrinsics differ per camera so the quirk is visible
        prm4[c]["intrinsic_matrix"][0][0] += 10.0 * c
        prm4[c]["intrinsic_matrix"][1][1] += 7.0 * c
    H.camera_params = np.array(prm4)
    groups, outs = [], []
    for m, msk in enumerate(TRI_NONE_MASKS):
        g = [[int(cents[c][m % 6][0]), int(cents[c][m % 6][1])] if msk[c] else [None, None] for c in range(4)]
        r = H.triangulate_point(g, sc.poses)
        outs.append([np.nan] * 3 if r[0] is None else list(r))
        groups.append([[np.nan, np.nan] if p[0] is None else p for p in g])
    R4, t4 = poses_arrays(sc.poses)
    K4, d4 = params_arrays(prm4)
    np.savez_compressed(os.path.join(OUT, "tri_none.npz"), groups=np.array(groups, float), R=R4, t=t4, K=K4,
                        dist=d4, out=np.array(outs, float),
                        provenance="reference: lib/Helpers.py:43-84 with [None,None] entries (NaN here)")
    print("tri_none:", np.array(outs).shape)

    # ---- correspondence cases ------------------------------------------------------------------
    # C=2, bundled calibration: frames made of subsets of the 54 captured pairs, camera-1 order shuffled
    rng = np.random.default_rng(11)
    for k, (lo, hi) in enumerate([(0, 6), (6, 16), (16, 24), (30, 54)]):
        sel = ip[lo:hi]
        l0 = [[int(p[0][0]), int(p[0][1])] for p in sel]
        l1 = [[int(p[1][0]), int(p[1][1])] for p in sel]
        perm = rng.permutation(len(l1))
        l1 = [l1[i] for i in perm]
        save_corr(f"corr_c2_bundled_{k}", H, [l0, l1], poses, params, Fs_b, 4,
                  f"bundled pairs {lo}:{hi}, jsons/fundamentals.json")
    # float-valued points (the dtype of jsons/image_points.json) -> float outputs
    sel = ip[0:5]
    save_corr("corr_c2_bundled_float", H, [[list(map(float, p[0])) for p in sel], [list(map(float, p[1])) for p in sel]],
              poses, params, Fs_b, 2, "float inputs")

    def synth_case(name, C, M, seed, obj_count, dist=MILD_DIST, jitter=0.0, shuffle=True, drop=None, extra=0):
        sc = Scene(C, dist=dist)
        rng = np.random.default_rng(seed)
        mk = sc.markers(rng, M)
        cents = sc.centroids(mk, rng, jitter)
        lists = []
        for c in range(C):
            l = [[int(x), int(y)] for x, y in cents[c]]
            if drop and c in drop:
                l = l[: max(0, len(l) - drop[c])]
            for _ in range(extra):
                l.append([int(rng.integers(0, 1920)), int(rng.integers(0, 1080))])
            if shuffle:
                l = [l[i] for i in rng.permutation(len(l))]
            lists.append(l)
        save_corr(name, H, lists, sc.poses, sc.camera_params, sc.Fs, obj_count, f"synthetic ring C={C} M={M} seed={seed}")

    synth_case("corr_c3_m4", 3, 4, 101, 3)
    synth_case("corr_c6_m8", 6, 8, 102, 8, jitter=0.7)
    synth_case("corr_c6_m8_objcount0", 6, 8, 103, 0)
    synth_case("corr_c6_m8_big_objcount", 6, 8, 104, 50)
    synth_case("corr_c6_m32", 6, 32, 105, 32, jitter=0.5)
    synth_case("corr_c4_m12_clutter", 4, 12, 106, 12, jitter=1.0, extra=5)
    synth_case("corr_c4_m6_dropped", 4, 6, 107, 6, drop={2: 3, 3: 1})

    # edge cases: sentinel lists, empty cameras, no matches at all
    sc = Scene(3, dist=MILD_DIST)
    rng = np.random.default_rng(9)
    cents = sc.centroids(sc.markers(rng, 3))
    L = [[[int(x), int(y)] for x, y in cents[c]] for c in range(3)]
    save_corr("corr_edge_sentinel_cam1", H, [L[0], [[None, None]], L[2]], sc.poses, sc.camera_params, sc.Fs, 2,
              "camera 1 returned the [[None,None]] sentinel")
    save_corr("corr_edge_sentinel_cam0", H, [[[None, None]], L[1], L[2]], sc.poses, sc.camera_params, sc.Fs, 2,
              "camera 0 returned the sentinel")
    save_corr("corr_edge_all_empty", H, [[[None, None]], [[None, None]], [[None, None]]], sc.poses,
              sc.camera_params, sc.Fs, 2, "all cameras empty")
    far = [[[5, 5]], [[1900, 1000]], [[10, 1070]]]
    save_corr("corr_edge_no_match", H, far, sc.poses, sc.camera_params, sc.Fs, 1, "no candidate within 10 px")
    save_corr("corr_edge_one_marker", H, [[L[0][0]], [L[1][0]], [L[2][0]]], sc.poses, sc.camera_params, sc.Fs, 0,
              "a single marker")

    # ---- bundle-adjustment residual vector (Helpers.py:158-167) -----------------------------------
    H.camera_params = np.array(params)
    with open("jsons/before_ba_extrinsics.json") as f:
        before = json.load(f)
    for p in before:
        p["R"], p["t"] = np.array(p["R"]), np.array(p["t"])
    fun, x0 = capture_residual_function(H, ip, before)
    rng = np.random.default_rng(5)
    xs = [x0, x0 + rng.normal(0, 1e-3, x0.shape), x0 + rng.normal(0, 1e-2, x0.shape)]
    res = [np.asarray(fun(x)) for x in xs]
    np.savez_compressed(os.path.join(OUT, "ba_residuals.npz"), image_points=ip, params=np.array(xs),
                        residuals=np.array(res), K=K, dist=dist,
                        provenance="reference+cvstub: residual_function of lib/Helpers.py:161-167 captured through "
                                   "a patched scipy.optimize.least_squares, before_ba_extrinsics.json start")
    print("ba_residuals:", np.array(res).shape, np.array(res).dtype)
    gen_mixed(H)


if __name__ == "__main__":
    main()
