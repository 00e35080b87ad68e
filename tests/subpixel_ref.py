"""NumPy restatement of the sub-pixel centroid (csrc/subpixel.hip, mocap_refine_centroids): the same integer
sums and the same FP64 operations in the same order, every one rounded on its own, so the device must equal this bit for bit.
Plain loops over the points; the windows are NumPy slices."""
import numpy as np

EMPTY, EDGE, NEIGHBOUR, MOVING, CUT = 1, 2, 4, 8, 16
FALLBACK = EMPTY | EDGE | NEIGHBOUR | MOVING

_f = np.float64


def distort_pt(K, dist, px, py):
    """geom_dev.h: distort_pt -- an undistorted-image pixel through the forward lens model (step 1 of the definition)"""
    K = np.asarray(K, _f).reshape(9)
    fx, cx0, fy, cy0 = K[0], K[2], K[4], K[5]
    k1, k2, p1, p2, k3 = (_f(v) for v in np.asarray(dist, _f).reshape(5))
    x, y = (_f(px) - cx0) / fx, (_f(py) - cy0) / fy
    r2 = x * x + y * y
    cd = 1 + ((k3 * r2 + k2) * r2 + k1) * r2
    xd = x * cd + (2 * p1 * x * y + p2 * (r2 + 2 * x * x))
    yd = y * cd + (p1 * (r2 + 2 * y * y) + 2 * p2 * x * y)
    return fx * xd + cx0, fy * yd + cy0


def undistort_pt(K, dist, px, py):
    """geom_dev.h: undistort_pt -- cv.undistortPoints(p, K, dist, P=K) by five fixed-point rounds"""
    K = np.asarray(K, _f).reshape(9)
    fx, cx0, fy, cy0 = K[0], K[2], K[4], K[5]
    k1, k2, p1, p2, k3 = (_f(v) for v in np.asarray(dist, _f).reshape(5))
    x0, y0 = (_f(px) - cx0) / fx, (_f(py) - cy0) / fy
    x, y = x0, y0
    for _ in range(5):
        r2 = x * x + y * y
        icd = 1.0 / (1 + ((k3 * r2 + k2) * r2 + k1) * r2)
        dx = 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
        dy = p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
        x, y = (x0 - dx) * icd, (y0 - dy) * icd
    return fx * x + cx0, fy * y + cy0


def _start_index(v, n):
    f = np.floor(v + 0.5)
    if not f >= 0.0:
        return 0
    return n - 1 if f > n - 1 else int(f)


def window_sums(gray, mx, my, r, floor):
    """(S, Sx, Sy, x0, y0, edge) of the window of radius r around (mx, my), clipped to the image"""
    H, W = gray.shape
    x0, x1, y0, y1 = max(mx - r, 0), min(mx + r, W - 1), max(my - r, 0), min(my + r, H - 1)
    w = np.maximum(gray[y0:y1 + 1, x0:x1 + 1].astype(np.int64) - floor, 0)
    xs, ys = np.arange(x0, x1 + 1), np.arange(y0, y1 + 1)
    S, Sx, Sy = int(w.sum()), int((w * (xs - x0)[None, :]).sum()), int((w * (ys - y0)[:, None]).sum())
    assert Sx < 2 ** 32 and Sy < 2 ** 32  # the device's sums are 32-bit
    ring = ((xs == mx - r) | (xs == mx + r))[None, :] | ((ys == my - r) | (ys == my + r))[:, None]
    return S, Sx, Sy, x0, y0, bool((w[ring] > 0).any())


def refine_image(gray, pts, radius, floor, iters=3, K=None, dist=None, identity=True, coords=1):
    """One image.  gray uint8 [H, W]; pts int [n, 2] = (cx, cy) in undistorted-image pixels (the first max_blobs points of the
    record); identity: the slot's table is the identity (mocap_set_undistort's identity_out), else K and dist are the slot's lens.
    Returns (xy float64 [n, 2], S int32 [n], flags int32 [n])."""
    H, W = gray.shape
    pts = np.asarray(pts, np.int64).reshape(-1, 2)
    n = len(pts)
    UV = np.empty((n, 2), _f)
    start = np.empty((n, 2), np.int64)
    for i, (cx, cy) in enumerate(pts):
        U, V = (_f(cx), _f(cy)) if identity else distort_pt(K, dist, cx, cy)
        UV[i] = U, V
        start[i] = _start_index(U, W), _start_index(V, H)
    xy = np.empty((n, 2), _f)
    Ss, flags = np.zeros(n, np.int32), np.zeros(n, np.int32)
    for i in range(n):
        mx, my = int(start[i, 0]), int(start[i, 1])
        fl, fx_, fy_, it = 0, _f(0), _f(0), 0
        while True:
            S, Sx, Sy, x0, y0, edge = window_sums(gray, mx, my, radius, floor)
            if S == 0:
                fl |= EMPTY
                break
            fx_ = _f(x0) + _f(Sx) / _f(S)
            fy_ = _f(y0) + _f(Sy) / _f(S)
            nx, ny = int(np.floor(fx_ + 0.5)), int(np.floor(fy_ + 0.5))
            if (nx, ny) == (mx, my):
                break
            if it + 1 >= iters:
                fl |= MOVING
                break
            mx, my, it = nx, ny, it + 1
        if edge:
            fl |= EDGE
        others = np.delete(start, i, axis=0)
        if len(others) and (np.abs(others - [mx, my]) <= radius).all(axis=1).any():
            fl |= NEIGHBOUR
        if mx - radius < 0 or mx + radius > W - 1 or my - radius < 0 or my + radius > H - 1:
            fl |= CUT
        if fl & FALLBACK:
            xy[i] = (_f(pts[i, 0]), _f(pts[i, 1])) if coords == 1 else UV[i]
        elif coords == 1 and not identity:
            xy[i] = undistort_pt(K, dist, fx_, fy_)
        else:
            xy[i] = fx_, fy_
        Ss[i], flags[i] = S, fl
    return xy, Ss, flags


def refine_batch(frames, xy_int, counts, radius, floor, iters=3, lenses=None, cam_mod=1, coords=1, max_blobs=None):
    """frames uint8 [n, H, W]; xy_int int [n, rows, 2]; counts [n]; lenses: per slot of the batch (index n % cam_mod) a tuple
    (K, dist, identity), or None = identity slots.  Returns (xy [n, max_blobs, 2] NaN where nothing is written, S, flags [n,
    max_blobs] with -1 there)."""
    n = len(frames)
    max_blobs = xy_int.shape[1] if max_blobs is None else max_blobs
    xy = np.full((n, max_blobs, 2), np.nan)
    S, fl = np.full((n, max_blobs), -1, np.int32), np.full((n, max_blobs), -1, np.int32)
    for i in range(n):
        c = min(int(counts[i]), max_blobs)
        if c <= 0:
            continue
        K, dist, ident = (None, None, True) if lenses is None else lenses[i % cam_mod]
        xy[i, :c], S[i, :c], fl[i, :c] = refine_image(frames[i], xy_int[i, :c], radius, floor, iters, K, dist, ident, coords)
    return xy, S, fl


def place_markers(scene, rng, n, margin, apart):
    """n markers whose projections, in every camera and in both the raw and the ideal image, keep `margin` px from the border
    and more than `apart` px (largest coordinate difference) from each other: scenes for the accuracy and pipeline tests"""
    chosen = []
    for _ in range(10000):
        m = scene.markers(rng, 1)[0]
        ok = True
        for cam in range(scene.n_cam):
            for d in (True, False):
                p = scene.pixels(np.array(chosen + [m]), cam, distorted=d)
                inside = (p[-1] > margin).all() and p[-1, 0] < scene.width - margin and p[-1, 1] < scene.height - margin
                clear = len(chosen) == 0 or np.abs(p[:-1] - p[-1]).max(axis=1).min() > apart
                ok = ok and inside and clear
        if ok:
            chosen.append(m)
            if len(chosen) == n:
                return np.array(chosen)
    raise AssertionError("no placement found")
