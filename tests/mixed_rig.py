"""What the tests of rigs whose cameras all differ (mocapv2_amd.synth.MixedScene) share.  Not a test module.

Every other multi-camera case of the suite gives all cameras one K and one lens, so a kernel or host routine that reads the
wrong camera's intrinsics passes it.  The helpers here build the unequal-camera inputs and measure, with the CPU oracle alone,
what such a read would change: a case that cannot see the fault pins nothing."""
import numpy as np

import oracle
from mocapv2_amd.synth import MIXED_DISTS, MixedScene


def arrays(scene):
    """(K [C][3][3], dist [C][5], R, t, F) of a MixedScene: pipeline.scene_arrays for per-camera intrinsics"""
    return (np.stack(scene.Ks), np.stack(scene.dists), np.stack([p["R"] for p in scene.poses]),
            np.stack([p["t"] for p in scene.poses]), np.stack(scene.Fs))


def correspondence_steps(scene, M, T, seed, floats=False):
    """T time steps of image-point lists: M markers per camera with 0.6 px jitter (floored to integers unless floats), shuffled;
    in every third step the last camera misses two markers; 0..3 clutter points per camera.  -> pts [T][C][M + 4][2] (int32 or
    float64), counts [T][C] int32"""
    C, P = scene.n_cam, M + 4
    pts = np.zeros((T, C, P, 2), np.float64 if floats else np.int32)
    cnt = np.zeros((T, C), np.int32)
    for s in range(T):
        rng = np.random.default_rng(seed + s)
        mk = scene.markers(rng, M)
        for c in range(C):
            px = scene.pixels(mk, c, distorted=False) + rng.normal(0, 0.6, (M, 2))
            l = (px if floats else np.floor(px))[rng.permutation(M)]
            if s % 3 == 1 and c == C - 1:
                l = l[: M - 2]
            extra = rng.integers(0, 1000, (rng.integers(0, 4), 2))
            l = np.concatenate([l, extra])
            cnt[s, c] = len(l)
            pts[s, c, : len(l)] = l
    return pts, cnt


def wrong_camera_sensitivity(pts, cnt, K, dist, R, t, F):
    """One time step through oracle.correspond three times: as it is, with camera 0's lens given to every camera, with camera
    0's K given to every camera (the fundamental matrices stay, so the groups do).  -> (true result, smallest relative change
    of a root's err under the wrong lens, smallest change of a root's xyz under the wrong K); (result, inf, inf) without roots"""
    ref = oracle.correspond(pts.astype(float), cnt, K, dist, R, t, F)
    if len(ref["root"]) == 0:
        return ref, np.inf, np.inf
    lens = oracle.correspond(pts.astype(float), cnt, K, np.stack([dist[0]] * len(K)), R, t, F)
    kmat = oracle.correspond(pts.astype(float), cnt, np.stack([K[0]] * len(K)), dist, R, t, F)
    assert np.array_equal(lens["root"], ref["root"]) and np.array_equal(kmat["root"], ref["root"])
    return (ref, float((np.abs(lens["err"] - ref["err"]) / ref["err"]).min()),
            float(np.abs(kmat["xyz"] - ref["xyz"]).max(1).min()))


def ba_case(C, N, seed, holes):
    """Residual-function inputs for C unequal cameras and N groups: pts [N][C][2] (integer pixels, 0.3 px jitter), valid
    [N][C], three parameter vectors around the truth (rotvec + t per camera 1.., sigma 1e-3), K, dist.  holes: about 5 % of
    the groups lose one camera's point, group 3 is seen by nobody and group 7 by camera 0 only."""
    from scipy.spatial.transform import Rotation
    sc = MixedScene(C)
    K, dist, R, t, _ = arrays(sc)
    rng = np.random.default_rng(seed)
    cents = sc.centroids(sc.markers(rng, N, extent=0.6), rng, jitter=0.3)
    pts = np.stack(cents, 1).astype(float)
    base = []
    for c in range(1, C):
        Rrel = R[c] @ R[0].T
        base += list(Rotation.from_matrix(Rrel).as_rotvec()) + list(t[c] - Rrel @ t[0])
    sets = np.array(base) + rng.normal(0, 1e-3, (3, 6 * (C - 1)))
    valid = np.ones((N, C), np.uint8)
    if holes:
        which = rng.choice(N, max(1, N // 20), replace=False)
        valid[which, rng.integers(0, C, len(which))] = 0
        valid[3, :] = 0
        valid[7, 1:] = 0
    return pts, valid, sets, K, dist


__all__ = ["MIXED_DISTS", "MixedScene", "arrays", "correspondence_steps", "wrong_camera_sensitivity", "ba_case"]
