"""The runs that leave the happy path of the step control (csrc/lm.h, restated by tests/lm_ref.py): rejected steps, steps
rejected for a point behind a camera, failed factorisations and the stops other than ftol.  Not a test module: the case table
of tests/test_lm_branches_host.py (which establishes on the restatement alone that every case is far from each of its decision
boundaries) and tests/test_gpu_lm_branches.py (which walks the device loops through them).

Every start is harsh on purpose: the truth moved by seeded Gaussian steps of tenths of a radian and tenths of the scene.  The
restatement runs are memoised here, as the cases of the neighbouring test modules are."""
import numpy as np

import intrinsics_ref as ir
import rig_ba_ref as rb
import rig_robust_ref as rr
from mocapv2_amd import synth

N_PERM = 10
FLOOR = 1e-12  # the allowance of a history column whose spread under permutation is 0

# name -> points of rb.case("noisy6", .), start seed, scale s of rb.perturbed_start(rot=s, trans=s, point=s / 2), lambda0,
# max_iters, Cauchy scale in px (None: no loss)
RIG = {
    "A": (96, 9, 0.6, 1e-3, 50, None),     # three rejections by rho after the first step
    "B": (96, 13, 0.6, 1e-6, 50, None),    # five rejections in a row: nu up to 32
    "C": (96, 7, 0.8, 1e-3, 11, None),     # steps rejected although rho > 0: a point behind a camera; max_iters on the last of them
    "D": (96, 7, 0.8, 1e-8, 5, None),      # S indefinite twice: the Cholesky stop
    "F": (96, 13, 0.6, 1e-6, 50, 2.0),     # Cauchy: leading rejections and two in the middle
    "G9": (300, 9, 0.6, 1e-3, 50, None),   # two workgroups of points
    "G22": (300, 22, 0.6, 1e-3, 50, None),
}
# Structural failures: a camera without observations has a zero block in S, whose pivot is exactly 0 on any hardware.
# name -> (cameras, lambda0): 6 is noisy6 at 96 points without camera 5, 32 the 32 x 64 problem without camera 31
STRUCTURAL = {
    "E_chol": (6, 1e-3), "E_lambda": (6, 6e15), "E_lambda_1e16": (6, 1e16),
    "E32_chol": (32, 1e-3), "E32_lambda": (32, 6e15),
}
# name -> case of intrinsics_ref, start seed, the four scales of ir.perturbed_start (rel, coef, rot, trans), lambda0, max_iters
_K20 = tuple(20 * v for v in (2e-3, 2e-3, 0.01, 0.005))
INTR = {
    "mild_rho": ("noisy_mild", 3, _K20, 1e-3, 50),          # three rejections by rho in the middle
    "golden_rho": ("noisy_golden", 2, _K20, 1e-9, 50),      # four
    "golden_behind": ("noisy_golden", 2, (0.3, 0.4, 2.0, 1.0), 1e-6, 16),  # nine leading rejections with rho > 0: a point behind
    "golden_behind_cut": ("noisy_golden", 2, (0.3, 0.4, 2.0, 1.0), 1e-6, 6),  # the same, cut off while still rejecting
}
# Three cameras of one call, under one lambda0 and max_iters: the first rejects by rho in the middle, the second starts with
# rejections for a point behind, the third accepts every step; they stop at three different iterations
TRIO, TRIO_LAMBDA0, TRIO_MAX_ITERS = ("mild_rho", "golden_behind", "golden_rho"), 1e-3, 22

_memo = {}


def _memoised(f):
    def g(*key):
        k = (f.__name__, *key)
        if k not in _memo:
            _memo[k] = f(*key)
        return _memo[k]
    return g


# ---- the rig ------------------------------------------------------------------------------------------------------------------
def rig32():
    """The 32 cameras x 64 points of test_gpu_rig_ba.py::test_thirty_two_cameras_with_64_points (D = 186: the factor lives in
    global memory): (prob, (R, t, X))"""
    scene = synth.Scene(32, 1920, 1080, synth.MILD_DIST)
    rng = np.random.default_rng(32)
    Xw = rng.uniform(-0.5, 0.5, (64, 3))
    px = np.stack([synth.project(Xw, p, scene.K, scene.dist) for p in scene.poses]) + rng.normal(0, 0.5, (32, 64, 2))
    valid = rng.uniform(0, 1, (32, 64)) > 0.3
    prob = rb.problem_from_arrays(px, valid, scene.camera_params)
    return prob, rb.perturbed_start({"scene": scene, "X": Xw}, 33, rot=0.003, trans=0.005, point=0.005)


def without_camera(prob, start, cam):
    """The problem and start without the observations of camera `cam`; points left with fewer than two views leave both"""
    R, t, X = start
    sub, points = rr.without(prob, np.flatnonzero(prob.cam == cam))
    return sub, (R, t, X[points])


@_memoised
def rig_case(name):
    """dict: prob, start (R, t, X), kw (max_iters, ftol, lambda0 of the loop), loss_c"""
    if name in STRUCTURAL:
        cams, lambda0 = STRUCTURAL[name]
        if cams == 32:
            prob, start = without_camera(*rig32(), 31)
        else:
            c = rb.case("noisy6", 96)
            prob, start = without_camera(c["prob"], rb.perturbed_start(c, 202), 5)
        return {"prob": prob, "start": start, "kw": {"max_iters": 50, "ftol": rb.LOOP_FTOL, "lambda0": lambda0}, "loss_c": None}
    n, seed, s, lambda0, max_iters, loss_c = RIG[name]
    c = rb.case("noisy6", n)
    return {"prob": c["prob"], "start": rb.perturbed_start(c, seed, rot=s, trans=s, point=s / 2),
            "kw": {"max_iters": max_iters, "ftol": rb.LOOP_FTOL, "lambda0": lambda0}, "loss_c": loss_c}


def rig_lm(prob, R, t, X, loss_c=None, **kw):
    return rb.lm(prob, R, t, X, **kw) if loss_c is None else rr.lm(prob, R, t, X, loss_c, **kw)


def _column_spread(spread, base, run):
    for k, col in (("cost", 0), ("lambda", 1), ("step", 3)):
        a, b = base["history"][:, col], run["history"][:, col]
        spread[k] = np.maximum(spread[k], np.where(a == 0, np.abs(b), np.abs(b / np.where(a == 0, 1.0, a) - 1)))


def same_decisions(run, base):
    """iterations, status, the accept sequence and which solves failed"""
    return (run["iterations"] == base["iterations"] and run["status"] == base["status"]
            and np.array_equal(run["history"][:, 2], base["history"][:, 2]) and np.array_equal(np.isnan(run["rho"]), np.isnan(base["rho"])))


def loop_spread(prob, R, t, X, ftol=rb.LOOP_FTOL, max_iters=50, lambda0=1e-3, loss_c=None, n_perm=N_PERM):
    """The rig's counterpart of intrinsics_ref.loop_spreads.  The loop on the problem and on n_perm seeded permutations of its
    observations: (base run, with its trace; every run took the base run's decisions: iterations, status, accept sequence,
    failed solves; spread).  spread: dict of cost, lambda, step [iterations], the largest relative difference of that history column from the
    base run's in each iteration (0 where the base entry is 0), and of poses, points: the largest difference of the returned
    R and t, and X, relative to the array's largest entry.  Runs that decided otherwise are left out of the spread."""
    kw = {"max_iters": max_iters, "ftol": ftol, "lambda0": lambda0}
    trace = []
    base = rig_lm(prob, R, t, X, loss_c, trace=trace, **kw)
    base["trace"] = trace
    n = base["iterations"]
    same, spread = True, {"cost": np.zeros(n), "lambda": np.zeros(n), "step": np.zeros(n), "poses": 0.0, "points": 0.0}
    poses = lambda run: np.c_[run["R"].reshape(-1, 9), run["t"]]
    for s in range(n_perm):
        run = rig_lm(rb.permuted(prob, 2000 + s), R, t, X, loss_c, **kw)
        if not same_decisions(run, base):
            same = False
            continue
        _column_spread(spread, base, run)
        spread["poses"] = max(spread["poses"], float(np.abs(poses(run) - poses(base)).max() / np.abs(poses(base)).max()))
        spread["points"] = max(spread["points"], float(np.abs(run["X"] - base["X"]).max() / np.abs(base["X"]).max()))
    return base, same, spread


@_memoised
def rig_reference(name, max_iters=None):
    """(base run, same decisions, spread) of loop_spread on the named case; max_iters: in place of the case's"""
    c = rig_case(name)
    kw = dict(c["kw"], max_iters=c["kw"]["max_iters"] if max_iters is None else max_iters)
    return loop_spread(c["prob"], *c["start"], loss_c=c["loss_c"], **kw)


def rig_depth_margin(prob, state):
    """Of a trial state (R, t, X): the most negative depth z of an observed point in its camera's frame, as a fraction of that
    point's distance from the camera"""
    R, t, X = state
    p = np.einsum("oij,oj->oi", R[prob.cam], X[prob.pt]) + t[prob.cam]
    return float((p[:, 2] / np.sqrt((p * p).sum(1))).min())


def failing_pivot(S):
    """(the first pivot of the Cholesky factorisation of S that is not positive, the largest diagonal entry of S), or None
    when there is none.  Column by column, as intrinsics_ref.cholesky."""
    n = len(S)
    L = np.zeros((n, n))
    for j in range(n):
        s = S[j, j] - float(np.sum(L[j, :j] * L[j, :j]))
        if not (s > 0.0 and np.isfinite(s)):
            return s, float(np.abs(np.diag(S)).max())
        L[j, j] = np.sqrt(s)
        L[j + 1:, j] = (S[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return None


# ---- the intrinsics -----------------------------------------------------------------------------------------------------------
@_memoised
def intr_case(name):
    """dict: cam, start (kd, R, t), kw (max_iters, ftol, lambda0)"""
    case, seed, (rel, coef, rot, trans), lambda0, max_iters = INTR[name]
    c = ir.case(case)
    return {"cam": c["cam"], "start": ir.perturbed_start(c, seed, rel=rel, coef=coef, rot=rot, trans=trans),
            "kw": {"max_iters": max_iters, "ftol": ir.LOOP_FTOL, "lambda0": lambda0}}


@_memoised
def intr_reference(name, max_iters=None, lambda0=None):
    """(base run, same decisions, spread) of intrinsics_ref.loop_spreads on the named case; max_iters, lambda0: in place of
    the case's"""
    c = intr_case(name)
    kw = dict(c["kw"])
    if max_iters is not None:
        kw["max_iters"] = max_iters
    if lambda0 is not None:
        kw["lambda0"] = lambda0
    return ir.loop_spreads(c["cam"], *c["start"], n_perm=N_PERM, **kw)


def trio_reference(name):
    return intr_reference(name, TRIO_MAX_ITERS, TRIO_LAMBDA0)


@_memoised
def singular_camera():
    """noisy_mild whose view 2 is six corners all at the board's origin: q = R (0, 0, 0) = 0 makes the rotation columns of its
    Jacobian, and with them the first pivot of its V*, exactly 0 at every state and damping.  dict: cam, start"""
    c = ir.case("noisy_mild")
    views = list(c["cam"].views)
    views[2] = (np.zeros((6, 2)), views[2][1][:6])
    return {"cam": ir.Camera(views, c["cam"].size), "start": ir.perturbed_start(c, 403)}


def intr_depth_margin(cam, state):
    """As rig_depth_margin, of a trial state (kd, R, t) over every board point of every view"""
    _, R, t = state
    worst = np.inf
    for v, (obj, _) in enumerate(cam.views):
        p = obj @ R[v][:, :2].T + t[v]
        worst = min(worst, float((p[:, 2] / np.sqrt((p * p).sum(1))).min()))
    return worst


# ---- what a run shows -----------------------------------------------------------------------------------------------------------
def branches(run):
    """The set of branches of lm_ref.control a restatement run took"""
    acc, rho = run["history"][:, 2] > 0, run["rho"]
    failed = np.isnan(rho)
    by_rho = ~acc & ~failed & (np.nan_to_num(rho) <= 0)
    behind = ~acc & ~failed & (np.nan_to_num(rho) > 0)
    out = set()
    if by_rho.any():
        out.add("rho-rejection")
    if behind.any():
        out.add("trial_behind rejection")
    if (~acc[1:] & ~acc[:-1]).any():
        out.add("consecutive rejections")
    if (acc[1:] & ~acc[:-1]).any():
        out.add("accept after rejection")
    if (failed[:-1] & ~failed[1:]).any():
        out.add("failed solve, then a solved step")
    out.add({rb.STOP_MAX_ITERS: "STOP_MAX_ITERS", rb.STOP_FTOL: "STOP_FTOL", rb.STOP_LAMBDA: "STOP_LAMBDA", rb.STOP_CHOLESKY: "STOP_CHOLESKY"}[run["status"]])
    if run["status"] == rb.STOP_MAX_ITERS and not acc[-1]:
        out.add("STOP_MAX_ITERS on a rejection")
    return out


def sequence(run):
    return "".join("1" if a else "0" for a in run["history"][:, 2])


def trailing_rejections(run, start=0):
    """(k, j): the first run of j >= 1 rejections after iteration `start` that follows an accepted iteration k - 1"""
    acc = run["history"][:, 2] > 0
    for k in range(max(start, 1), len(acc)):
        if acc[k - 1] and not acc[k]:
            j = 1
            while k + j < len(acc) and not acc[k + j]:
                j += 1
            return k, j
    raise ValueError("no rejection after an accepted step")


def allowance(spread, column):
    """8 x the column's largest spread over the iterations; the floor where that is 0"""
    s = float(np.max(spread[column])) if np.size(spread[column]) else 0.0
    return 8 * s if s > 0 else FLOOR
