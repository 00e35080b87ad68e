"""The bundle-adjustment residual problems of more than 256 groups (mocap_ba_residuals walks the groups in rounds of 256 and carries
its compaction base from round to round): a 3-camera scene built as test_gpu_geom's 16-camera case builds its own, the holes that
make the carried base matter, and the length of the residual vector by the reference's own rule (lib/Helpers.py:93, :104,
:127-128).  test_ba_cases_host asserts what it holds against the CPU oracle; test_gpu_geom runs it on the device.  Not a test
module."""
import numpy as np
from scipy.spatial.transform import Rotation

from mocapv2_amd.synth import MILD_DIST, Scene

C = 3
SIZES = (256, 257, 600)      # one full round and no second; a second round of one group; three rounds, the last one partial
ONE_VIEW_MISSING = (3, 255, 256, 257, 300, 511, 512)
UNSEEN, ONE_CAMERA = 100, 258  # a group nobody sees (first round); a group of the second round that camera 0 alone sees
N_TRIANGULATED, N_RESIDUALS = 591, 589


def problem(M, seed=9):
    """-> dict: K [3, 3, 3], dist [3, 5], R [3, 3, 3], t [3, 3], pts [M, 3, 2] (integer centroids with 0.3 px of jitter), sets
    [13, 12]: the rig's true rotvec / t sextuples plus N(0, 1e-3) noise -- 13 rows are a forward-difference Jacobian of C = 3"""
    sc = Scene(C, 1920, 1080, dist=MILD_DIST)
    K, dist = np.stack([sc.K] * C), np.stack([sc.dist] * C)
    R, t = np.stack([p["R"] for p in sc.poses]), np.stack([p["t"] for p in sc.poses])
    rng = np.random.default_rng(seed)
    cents = sc.centroids(sc.markers(rng, M, extent=1.0), rng, jitter=0.3)
    pts = np.stack([np.stack([cents[c][m] for c in range(C)]) for m in range(M)]).astype(float)
    base = []
    for c in range(1, C):
        Rrel = R[c] @ R[0].T
        base += list(Rotation.from_matrix(Rrel).as_rotvec()) + list(t[c] - Rrel @ t[0])
    sets = np.array(base) + rng.normal(0, 1e-3, (13, 6 * (C - 1)))
    return {"K": K, "dist": dist, "R": R, "t": t, "pts": pts, "sets": sets}


def holes(M=600):
    """valid [M, 3]: one missing view in each of ONE_VIEW_MISSING (the camera changes from group to group), UNSEEN seen by nobody,
    ONE_CAMERA by camera 0 alone.  From group 256 on every group's object index lies below its group index."""
    valid = np.ones((M, C), np.uint8)
    for k, n in enumerate(ONE_VIEW_MISSING):
        valid[n, k % C] = 0
    valid[UNSEEN, :] = 0
    valid[ONE_CAMERA, 1:] = 0
    return valid


def lengths_by_the_rule(valid):
    """(object points, residuals): groups without a hole are triangulated, in order; object point n is paired with GROUP n --
    positionally, whatever group it came from -- and the pair is kept if group n has more than one valid view"""
    valid = np.asarray(valid) != 0
    nobj = int(valid.all(axis=1).sum())
    return nobj, int((valid[:nobj].sum(axis=1) > 1).sum())
