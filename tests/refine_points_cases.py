"""The inputs the tests of mocap_refine_points share (tests/test_refine_points_host.py against the restatement,
tests/test_gpu_refine_points.py on the device).  Not a test module."""
import functools

import numpy as np

import correspond_visible_ref as cv
import refine_points_ref as rp
from mocapv2_amd import synth

# The scenes of tests/test_correspond_visible_host.py in which the definition's known miss shows, with all
# their seeds: cameras, markers, jitter (px)
WRONG_MEMBER_SCENES = {"6x8": (6, 8, 0.5), "4x4": (4, 4, 0.5), "3x4": (3, 4, 0.3)}
# The pruning limit of those scenes, from their jitter alone: a true member's squared residual length at the refined point is at
# most sigma^2 chi^2 with 2 degrees of freedom (the fit takes its share away), and P(chi2_2 > 36) = exp(-18) = 1.5e-8 per member --
# 6 sigma.  At the jitter of 0.5 px this is the 9 px^2 the first experiment started from, at 0.3 px it is 3.24 px^2.
PRUNE_SIGMAS2 = 36.0


def prune_limit(jitter):
    return PRUNE_SIGMAS2 * jitter * jitter


@functools.lru_cache(maxsize=None)
def wrong_member_case(name, seed):
    """(scene arrays K, dist, R, t; pts [C][P][2]; truth [M][C]; correspond_visible's result) of one seed"""
    C, M, jitter = WRONG_MEMBER_SCENES[name]
    scene, pts, counts, truth, markers = cv.scene_case(C, M, 0.3, seed, jitter=jitter)
    cams = cv.scene_arrays(scene)
    return cams, pts, truth, cv.correspond_visible(pts, counts, *cams)


def row_kind(row, truth):
    """"true": the index row of a marker; "subset": a strict subset of one; "wrong": it has a member that is not its marker's"""
    want = [tuple(int(v) for v in r) for r in truth]
    if tuple(row) in want:
        return "true"
    if any(all(a == -1 or a == b for a, b in zip(row, w)) for w in want):
        return "subset"
    return "wrong"


def uneven_poses(n_cam=6, radii=(2.0, 5.0), height=2.5):
    """synth.ring_cameras with the radii taken in turn: cameras at unequal distances, all looking at the origin"""
    return [synth.ring_cameras(n_cam, radius=radii[i % len(radii)], height=height)[i] for i in range(n_cam)]


@functools.lru_cache(maxsize=None)
def uneven_scene(N=2000, sigma=0.3, seed=0):
    """6 cameras alternating 2 m and 5 m from the origin at height 2.5 m, f = 1400 px, N markers in a 2 x 2 x 2 m volume seen by
    all six with Gaussian pixel noise sigma.  Returns dict: K, dist, R, t, pts [C][N][2], idx [N][C], truth [N][3], X0 [N][3]
    (the DLT over all six: correspond_visible's X for these members)"""
    C = 6
    poses = uneven_poses(C)
    K1 = synth.intrinsics(1920, 1080)
    rng = np.random.default_rng(seed)
    X = rng.uniform(-1.0, 1.0, (N, 3))
    pts = np.stack([synth.project(X, poses[c], K1, synth.ZERO_DIST) + rng.normal(0, sigma, (N, 2)) for c in range(C)])
    K, dist = np.stack([K1] * C), np.zeros((C, 5))
    R, t = np.stack([p["R"] for p in poses]), np.stack([p["t"] for p in poses])
    idx = np.tile(np.arange(N, dtype=np.int32)[:, None], (1, C))
    with np.errstate(all="ignore"):
        X0, valid = cv._solve_members(cv.Cameras(K, dist, R, t), pts, idx)
    assert valid.all()
    return dict(K=K, dist=dist, R=R, t=t, pts=pts, idx=idx, truth=X, X0=X0, sigma=sigma)


@functools.lru_cache(maxsize=None)
def uneven_refined(N=2000):
    """The restatement's rows of uneven_scene(N), computed once for the tests that look at them"""
    s = uneven_scene(N)
    rig = rp.Rig(s["K"], s["dist"], s["R"], s["t"], 0)
    return [rp.refine_row(rig, s["X0"][n], 63, lambda c, n=n: s["pts"][c, n]) for n in range(N)]


@functools.lru_cache(maxsize=None)
def status_case():
    """One time step of a 6-camera scene (8 markers every camera sees, jitter 0.5 px) whose rows reach every status an input can
    reach under one set of parameters (max_iters 10, ftol 1e-9, lambda0 1e-3), good rows between them.  Returns dict: cams, pts
    [1][C][P][2], idx [1][Q][C], views [1][Q], xyz [1][Q][3], n [1], want {row: status}, markers"""
    scene, pts, counts, truth, markers = cv.scene_case(6, 8, 0.0, 0, jitter=0.5)
    cams = cv.scene_arrays(scene)
    R0, t0 = np.asarray(cams[2][0]), np.asarray(cams[3][0])
    centre0 = -R0.T @ t0
    Q = 12
    idx = np.full((Q, 6), -1, np.int32)
    views = np.zeros(Q, np.uint32)
    xyz = np.zeros((Q, 3))
    for q in range(Q):
        idx[q] = truth[q % 8]
        views[q] = 63
        xyz[q] = markers[q % 8] + 0.001
    want = {q: rp.lm_ref.STOP_FTOL for q in range(Q)}
    xyz[1] = markers[1] + np.array([0.5, 0.0, 0.0])            # displaced by 0.5 m: converges all the same
    views[2] = 1 << 3                                           # one member
    want[2] = rp.E_VIEWS
    views[3] = 0                                                # none
    want[3] = rp.E_VIEWS
    xyz[4, 1] = np.nan                                          # the point is not finite
    want[4] = rp.E_INPUT
    idx[5, 2] = pts.shape[1]                                    # an index at P
    want[5] = rp.E_INPUT
    idx[6, 0] = -1                                              # a member without an index
    want[6] = rp.E_INPUT
    views[7] = 63 | 1 << 6                                      # a bit at C
    want[7] = rp.E_INPUT
    xyz[8] = centre0 - 0.5 * R0[2]                              # half a metre behind camera 0
    want[8] = rp.E_BEHIND
    views[9] = 0b101000                                         # two members: the smallest row that is refined
    idx[10, 4] = -7                                             # an index outside the list of a camera that is no member: not read
    views[10] = 63 & ~(1 << 4)
    idx[11] = truth[2]
    xyz[11] = centre0 + 0.3 * R0[2] + 0.4 * R0[0]               # marker 2 from close to camera 0 and far off its axis
    return dict(cams=cams, pts=pts[None], idx=idx[None], views=views[None], xyz=xyz[None], n=np.array([Q], np.int32), want=want,
                markers=markers)
