"""NumPy restatement of the rig bundle adjustment the HIP kernels implement, and the seeded cases the
tests share.  Not a test module: the yardstick of tests/test_rig_ba_host.py, tests/test_gpu_rig_ba.py and
tests/test_gpu_rig_ba_shapes.py.

Definition (all FP64).  N points, C <= 32 cameras, observations (n, c, u, v) point-major.  Camera 0 is the identity; cameras
1.. are (R_c, t_c) world -> camera; K and the 5 distortion coefficients are fixed and indexed by the true camera number.
Residual of an observation: proj(K_c, dist_c, R_c X_n + t_c) - (u, v), pinhole + Brown distortion as synth.project; cost 1/2
sum r^2; a point at z <= 0 in a camera that sees it makes a trial step invalid.  Analytic Jacobian under the local
perturbation R <- Exp(w) R, t <- t + dt.  Normal equations in blocks U_c (6x6), V_n (3x3), W_nc (6x3), g_c, g_n; Marquardt
damping U_c += lambda diag U_c, V_n += lambda diag V_n; Schur complement on the points S = U* - sum_n W_n V*_n^-1 W_n^T,
Cholesky, back-substitution.  Nielsen's control: lambda_0 = 1e-3, nu = 2; rho = actual / predicted reduction; rho > 0:
accept, lambda *= max(1/3, 1 - (2 rho - 1)^3), nu = 2; else lambda *= nu, nu *= 2.  A Cholesky failure counts as a rejected
step; two in a row stop the loop.  Stops: max_iters, an accepted step with relative decrease < ftol, lambda > 1e16.  On
return every t and X is scaled so that |t_1| is what it was at the start.

The camera model with its derivatives and the loop's control are tests/lm_ref.py's, shared with tests/intrinsics_ref.py as
csrc/lm.h is shared by the two kernel files.  Every per-observation quantity is formed by the same operations in the same
order as csrc/rig_ba.hip and csrc/lm.h (the library is built without fused multiply-add), so the kernels differ from this
file in the ORDER of the sums over observations and points only; `permuted` measures what that order is worth."""
import json
import os

import numpy as np

import lm_ref
from lm_ref import STOP_MAX_ITERS, STOP_FTOL, STOP_LAMBDA, STOP_CHOLESKY  # noqa: F401 (the tests read them from here)
from mocapv2_amd import synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


class Problem:
    """obs_pt [n_obs], obs_cam [n_obs], obs_uv [n_obs][2] (any order), K [C][3][3], dist [C][5], N points."""

    def __init__(self, obs_pt, obs_cam, obs_uv, K, dist, N):
        self.pt, self.cam = np.asarray(obs_pt, np.int64), np.asarray(obs_cam, np.int64)
        self.uv = np.asarray(obs_uv, float).reshape(-1, 2)
        self.K, self.dist = np.asarray(K, float), np.asarray(dist, float)
        self.C, self.N = len(self.K), int(N)
        self.D = 6 * (self.C - 1)

    def point_major(self):
        """(obs_offset [N + 1], obs_cam, obs_uv) sorted by point, then camera: the layout of the C-ABI"""
        order = np.lexsort((self.cam, self.pt))
        offset = np.zeros(self.N + 1, np.int32)
        np.cumsum(np.bincount(self.pt, minlength=self.N), out=offset[1:])
        return offset, self.cam[order].astype(np.int32), np.ascontiguousarray(self.uv[order])

    def sorted(self):
        order = np.lexsort((self.cam, self.pt))
        return Problem(self.pt[order], self.cam[order], self.uv[order], self.K, self.dist, self.N)


def observe(prob, R, t, X):
    """Per observation: residual r [n_obs][2], camera Jacobian jc [n_obs][2][6], point Jacobian jp [n_obs][2][3], front
    [n_obs] (z > 0).  R [C][3][3], t [C][3], X [N][3]."""
    c, n = prob.cam, prob.pt
    Rm, tm, Xm = R[c], t[c], X[n]
    q = [(Rm[:, i, 0] * Xm[:, 0] + Rm[:, i, 1] * Xm[:, 1]) + Rm[:, i, 2] * Xm[:, 2] for i in range(3)]
    lens = [prob.K[c, 0, 0], prob.K[c, 1, 1], prob.K[c, 0, 2], prob.K[c, 1, 2]] + [prob.dist[c, i] for i in range(5)]
    with np.errstate(all="ignore"):
        r, front, A, _ = lm_ref.project(lens, q, [tm[:, 0], tm[:, 1], tm[:, 2]], prob.uv)
        jp = np.empty((len(c), 2, 3))
        jc = np.empty((len(c), 2, 6))
        for i in range(2):
            for j in range(3):
                jp[:, i, j] = (A[i][0] * Rm[:, 0, j] + A[i][1] * Rm[:, 1, j]) + A[i][2] * Rm[:, 2, j]
            jc[:, i, :] = np.stack(lm_ref.pose_columns(A[i], q), 1)
    return r, jc, jp, front


def cost_of(prob, R, t, X):
    """(1/2 sum r^2, every observed point in front of its camera)"""
    r, _, _, front = observe(prob, R, t, X)
    return 0.5 * float(np.sum(r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1])), bool(front.all())


def _inv_sym3(V):
    """inverse of symmetric 3x3 matrices [N][3][3] by the adjugate, the kernel's operations"""
    v00, v01, v02, v11, v12, v22 = V[:, 0, 0], V[:, 0, 1], V[:, 0, 2], V[:, 1, 1], V[:, 1, 2], V[:, 2, 2]
    with np.errstate(all="ignore"):
        c00, c01, c02 = v11 * v22 - v12 * v12, v02 * v12 - v01 * v22, v01 * v12 - v02 * v11
        det = (v00 * c00 + v01 * c01) + v02 * c02
        c11, c12, c22 = v00 * v22 - v02 * v02, v01 * v02 - v00 * v12, v00 * v11 - v01 * v01
        o = np.empty_like(V)
        o[:, 0, 0], o[:, 0, 1], o[:, 0, 2] = c00 / det, c01 / det, c02 / det
        o[:, 1, 1], o[:, 1, 2], o[:, 2, 2] = c11 / det, c12 / det, c22 / det
        o[:, 1, 0], o[:, 2, 0], o[:, 2, 1] = o[:, 0, 1], o[:, 0, 2], o[:, 1, 2]
    return o


def linearize(prob, R, t, X, lam):
    """The pieces of one iteration: dict with cost, front, gc [D], gp [N][3], U [C-1][6][6], V [N][3][3], W [n_obs][6][3]
    (rows of camera-0 observations zero), Vinv (damped), S [D][D] (damped), rhs [D], gradient [D + 3 N]."""
    C, N, D = prob.C, prob.N, prob.D
    r, jc, jp, front = observe(prob, R, t, X)
    free = prob.cam > 0
    cost = 0.5 * float(np.sum(r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]))
    Uo = jc[:, 0, :, None] * jc[:, 0, None, :] + jc[:, 1, :, None] * jc[:, 1, None, :]
    gco = jc[:, 0, :] * r[:, 0, None] + jc[:, 1, :] * r[:, 1, None]
    Vo = jp[:, 0, :, None] * jp[:, 0, None, :] + jp[:, 1, :, None] * jp[:, 1, None, :]
    gpo = jp[:, 0, :] * r[:, 0, None] + jp[:, 1, :] * r[:, 1, None]
    W = jc[:, 0, :, None] * jp[:, 0, None, :] + jc[:, 1, :, None] * jp[:, 1, None, :]
    W[~free] = 0.0
    U = np.zeros((C, 6, 6))
    gc = np.zeros((C, 6))
    np.add.at(U, prob.cam, Uo)
    np.add.at(gc, prob.cam, gco)
    U, gc = U[1:], gc[1:].reshape(-1)
    V = np.zeros((N, 3, 3))
    gp = np.zeros((N, 3))
    np.add.at(V, prob.pt, Vo)
    np.add.at(gp, prob.pt, gpo)
    Vd = V.copy()
    for i in range(3):
        Vd[:, i, i] = V[:, i, i] + lam * V[:, i, i]
    Vinv = _inv_sym3(Vd)
    # Y_o = W_o V*^-1 of the observation's point; S blocks over all pairs of observations of one point, a <= b
    Vi = Vinv[prob.pt]
    Y = np.empty_like(W)
    for j in range(3):
        Y[:, :, j] = (W[:, :, 0] * Vi[:, 0, j, None] + W[:, :, 1] * Vi[:, 1, j, None]) + W[:, :, 2] * Vi[:, 2, j, None]
    S = np.zeros((C - 1, C - 1, 6, 6))
    idx = np.flatnonzero(free)
    order = idx[np.argsort(prob.pt[idx], kind="stable")]
    pts_sorted = prob.pt[order]
    starts = np.flatnonzero(np.r_[True, pts_sorted[1:] != pts_sorted[:-1]])
    counts = np.diff(np.r_[starts, len(order)])
    ia, ib = [], []
    for k in range(1, int(counts.max()) + 1 if len(counts) else 1):  # all pairs (i, j) of positions within a point's run
        for i in range(k):
            sel = starts[counts >= k]
            ia.append(order[sel + i])
            ib.append(order[sel + k - 1])
    ia, ib = np.concatenate(ia), np.concatenate(ib)
    swap = prob.cam[ia] > prob.cam[ib]
    ia, ib = np.where(swap, ib, ia), np.where(swap, ia, ib)
    blk = np.empty((len(ia), 6, 6))
    Ya, Wb = Y[ia], W[ib]
    for j in range(6):
        blk[:, :, j] = (Ya[:, :, 0] * Wb[:, j, 0, None] + Ya[:, :, 1] * Wb[:, j, 1, None]) + Ya[:, :, 2] * Wb[:, j, 2, None]
    np.add.at(S, (prob.cam[ia] - 1, prob.cam[ib] - 1), blk)
    gpn = gp[prob.pt]
    yg = (Y[:, :, 0] * gpn[:, 0, None] + Y[:, :, 1] * gpn[:, 1, None]) + Y[:, :, 2] * gpn[:, 2, None]
    red = np.zeros((C, 6))
    np.add.at(red, prob.cam[idx], yg[idx])
    rhs = red[1:].reshape(-1) - gc
    Sfull = np.zeros((D, D))
    for a in range(C - 1):
        for b in range(a, C - 1):
            if a == b:
                Ud = U[a].copy()
                for i in range(6):
                    Ud[i, i] = U[a][i, i] + lam * U[a][i, i]
                blkab = Ud - S[a, a]
                blkab = np.triu(blkab) + np.triu(blkab, 1).T
                Sfull[6 * a:6 * a + 6, 6 * a:6 * a + 6] = blkab
            else:
                Sfull[6 * a:6 * a + 6, 6 * b:6 * b + 6] = 0.0 - S[a, b]
                Sfull[6 * b:6 * b + 6, 6 * a:6 * a + 6] = (0.0 - S[a, b]).T
    return {"cost": cost, "front": bool(front.all()), "gc": gc, "gp": gp, "U": U, "V": V, "W": W, "Vinv": Vinv, "S": Sfull,
            "rhs": rhs, "gradient": np.r_[gc, gp.reshape(-1)], "r": r, "jc": jc, "jp": jp}


def exp_so3(w):
    th2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]
    th = np.sqrt(th2)
    ka, kb = (1.0, 0.5) if th < 1e-12 else (np.sin(th) / th, (1.0 - np.cos(th)) / th2)
    Kx = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    return np.eye(3) + ka * Kx + kb * (np.outer(w, w) - th2 * np.eye(3))


def apply_step(prob, R, t, X, dc, dp):
    R2, t2 = R.copy(), t.copy()
    for c in range(1, prob.C):
        d = dc[6 * (c - 1):6 * c]
        R2[c] = exp_so3(d[:3]) @ R[c]
        t2[c] = t[c] + d[3:]
    return R2, t2, X + dp


def schur_step(prob, lin, lam):
    """(dc [D], dp [N][3], predicted reduction) from the pieces, or None when S is not positive definite"""
    try:
        L = np.linalg.cholesky(lin["S"])
    except np.linalg.LinAlgError:
        return None
    if not np.isfinite(L).all():
        return None
    y = np.linalg.solve(L, lin["rhs"])
    dc = np.linalg.solve(L.T, y)
    free = prob.cam > 0
    d_obs = dc.reshape(-1, 6)[np.where(free, prob.cam - 1, 0)]
    wt = np.einsum("oij,oi->oj", lin["W"], d_obs)  # W^T d_c, zero rows for camera 0
    q = lin["gp"].copy()
    np.add.at(q, prob.pt, wt)
    dp = -np.einsum("nij,nj->ni", lin["Vinv"], q)
    ud = np.array([lin["U"][a][i, i] for a in range(prob.C - 1) for i in range(6)])
    vd = np.stack([lin["V"][:, i, i] for i in range(3)], 1)
    pred = 0.5 * (float(np.sum(dc * ((lam * ud) * dc - lin["gc"]))) + float(np.sum(dp * ((lam * vd) * dp - lin["gp"]))))
    return dc, dp, pred


def dense_step(prob, lin, lam):
    """The same step from the full damped normal equations (the check of the Schur elimination)"""
    D, N = prob.D, prob.N
    H = np.zeros((D + 3 * N, D + 3 * N))
    for a in range(prob.C - 1):
        H[6 * a:6 * a + 6, 6 * a:6 * a + 6] = lin["U"][a]
    for n in range(N):
        H[D + 3 * n:D + 3 * n + 3, D + 3 * n:D + 3 * n + 3] = lin["V"][n]
    for o in np.flatnonzero(prob.cam > 0):
        a, n = prob.cam[o] - 1, prob.pt[o]
        H[6 * a:6 * a + 6, D + 3 * n:D + 3 * n + 3] += lin["W"][o]
        H[D + 3 * n:D + 3 * n + 3, 6 * a:6 * a + 6] += lin["W"][o].T
    H[np.diag_indices_from(H)] += lam * np.diag(H)
    d = np.linalg.solve(H, -lin["gradient"])
    return d[:D], d[D:].reshape(N, 3)


def rescale(R, t, X, t1_norm):
    now = float(np.sqrt((t[1, 0] * t[1, 0] + t[1, 1] * t[1, 1]) + t[1, 2] * t[1, 2]))
    with np.errstate(all="ignore"):
        s = t1_norm / now
    if not (s > 0 and np.isfinite(s)):
        s = 1.0
    return R, t * s, X * s


def lm(prob, R, t, X, max_iters=50, ftol=1e-12, lambda0=1e-3, trace=None):
    """The loop.  dict: R, t, X (gauge restored), status, iterations, cost_initial, cost, history [iterations][4] = (cost after
    the iteration, lambda it was solved with, accepted, |step|), rho [iterations] (nan for a Cholesky failure).  trace: a list
    that gets one dict per iteration, S (the damped reduced matrix) and trial (the trial state, None for a failed solve)."""
    R, t, X = np.array(R, float), np.array(t, float).reshape(-1, 3), np.array(X, float)
    R[0], t[0] = np.eye(3), 0.0
    t1_norm = float(np.sqrt((t[1, 0] * t[1, 0] + t[1, 1] * t[1, 1]) + t[1, 2] * t[1, 2]))
    cost0, front = cost_of(prob, R, t, X)
    if not front or not np.isfinite(cost0):
        raise ValueError("the state handed in has a point behind a camera that sees it")

    def try_step(state, lam):
        lin = linearize(prob, *state, lam)
        step = schur_step(prob, lin, lam)
        if trace is not None:
            trace.append({"S": lin["S"], "trial": None})
        if step is None:
            return None
        dc, dp, pred = step
        trial_state = apply_step(prob, *state, dc, dp)
        if trace is not None:
            trace[-1]["trial"] = trial_state
        return (trial_state, *cost_of(prob, *trial_state), pred, float(np.sqrt(np.sum(dp * dp) + np.sum(dc * dc))))

    (R, t, X), cost, status, history, rho = lm_ref.control((R, t, X), cost0, try_step, max_iters, ftol, lambda0)
    R, t, X = rescale(R, t, X, t1_norm)
    return {"R": R, "t": t, "X": X, "status": status, "iterations": len(history), "cost_initial": cost0, "cost": cost,
            "history": history, "rho": rho}


# ---- SciPy as the independent minimiser ---------------------------------------------------------------------------------
def _pack(R, t, X):
    from scipy.spatial.transform import Rotation
    return np.r_[np.concatenate([np.r_[Rotation.from_matrix(R[c]).as_rotvec(), t[c]] for c in range(1, len(R))]), X.reshape(-1)]


def _unpack(x, C):
    from scipy.spatial.transform import Rotation
    R, t = np.stack([np.eye(3)] * C), np.zeros((C, 3))
    for c in range(1, C):
        R[c] = Rotation.from_rotvec(x[6 * (c - 1):6 * (c - 1) + 3]).as_matrix()
        t[c] = x[6 * (c - 1) + 3:6 * c]
    return R, t, x[6 * (C - 1):].reshape(-1, 3)


def _left_jacobian(w):
    """J_l(w) of SO(3): Exp(w + d) = Exp(J_l(w) d) Exp(w) to first order in d"""
    th2 = float(w @ w)
    th = np.sqrt(th2)
    Kx = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    if th < 1e-6:
        return np.eye(3) + 0.5 * Kx + (Kx @ Kx) / 6.0
    return np.eye(3) + ((1.0 - np.cos(th)) / th2) * Kx + ((th - np.sin(th)) / (th2 * th)) * (Kx @ Kx)


def scipy_minimum(prob, R, t, X, sparse=None, max_nfev=300, fix_poses=False):
    """least_squares ('trf', x_scale='jac', tolerances 1e-12) from the same start, driven by this file's residual and
    analytic Jacobian.  Parameters: per free camera a rotation vector w and a translation d around the START pose
    (R_c = Exp(w) R_c^0, t_c = t_c^0 + d), then the points; the rotation columns are this file's local ones times J_l(w),
    which makes them exact away from w = 0 too.  Returns (cost, R, t, X).  sparse: CSR Jacobian and the LSMR solver
    (default: when the problem has more than 2000 parameters).  fix_poses: only the points move (the poses' columns are
    zero and their parameters stay 0)."""
    from scipy import optimize, sparse as sp
    C, N, D = prob.C, prob.N, prob.D
    n_obs = len(prob.pt)
    sparse = (D + 3 * N > 2000) if sparse is None else sparse
    R0, t0 = np.array(R, float), np.array(t, float).reshape(-1, 3)
    free = prob.cam > 0
    rows = np.arange(2 * n_obs).reshape(n_obs, 2)

    def state(x):
        Rn, tn = R0.copy(), t0.copy()
        for c in range(1, C):
            d = x[6 * (c - 1):6 * c]
            Rn[c] = exp_so3(d[:3]) @ R0[c]
            tn[c] = t0[c] + d[3:]
        return Rn, tn, x[D:].reshape(N, 3)

    def fun(x):
        return observe(prob, *state(x))[0].reshape(-1)

    def jac(x):
        _, jc, jp, _ = observe(prob, *state(x))
        jc = jc.copy()
        Jl = np.stack([np.eye(3)] + [_left_jacobian(x[6 * (c - 1):6 * (c - 1) + 3]) for c in range(1, C)])
        jc[:, :, :3] = np.einsum("oij,ojk->oik", jc[:, :, :3], Jl[prob.cam])
        if fix_poses:
            jc[:] = 0.0
        ri = np.r_[np.repeat(rows[free][:, :, None], 6, axis=2).reshape(-1), np.repeat(rows[:, :, None], 3, axis=2).reshape(-1)]
        ci = np.r_[np.broadcast_to((6 * (prob.cam[free] - 1))[:, None, None] + np.arange(6)[None, None, :], (int(free.sum()), 2, 6)).reshape(-1),
                   np.broadcast_to((D + 3 * prob.pt)[:, None, None] + np.arange(3)[None, None, :], (n_obs, 2, 3)).reshape(-1)]
        J = sp.csr_matrix((np.r_[jc[free].reshape(-1), jp.reshape(-1)], (ri, ci)), shape=(2 * n_obs, D + 3 * N))
        return J if sparse else J.toarray()

    x0 = np.r_[np.zeros(D), np.array(X, float).reshape(-1)]
    res = optimize.least_squares(fun, x0, jac=jac, method="trf", x_scale="jac", ftol=1e-12, xtol=1e-12, gtol=1e-12,
                                 max_nfev=max_nfev, tr_solver="lsmr" if sparse else "exact")
    Rn, tn, Xn = state(res.x)
    return float(res.cost), Rn, tn, Xn.copy()


# ---- the cases -------------------------------------------------------------------------------------------------------------
def _rig_case(n_cam, width, height, n_points, seed, sigma, dropout=0.3, extent=0.8, mixed=False):
    """Seeded rig: from default_rng(seed), in this order, the 3-D points, the dropout draws [N][C], the pixel noise [N][C][2].
    A point is seen by the cameras it projects into (inside the image, in front), minus the dropout; points left with fewer
    than 2 views are dropped.  mixed: every camera has its own K and lens (synth.MixedScene), and no point is seen by both
    camera 0 and camera 1 (of a point both would see, the even-numbered ones lose camera 0's view and the odd-numbered ones
    camera 1's): the pair has no fundamental matrix, so rig_initial_poses must reach camera 1 over an edge (a, 1) with a > 1.
    Returns dict: scene, image_points [C][N][2], valid [C][N], X (truth, kept points), prob."""
    scene = synth.MixedScene(n_cam, width, height) if mixed else synth.Scene(n_cam, width, height, synth.MILD_DIST)
    rng = np.random.default_rng(seed)
    X = rng.uniform(-extent, extent, size=(n_points, 3))
    drop = rng.uniform(0, 1, (n_points, n_cam)) < dropout
    noise = rng.normal(0, 1.0, (n_points, n_cam, 2)) * sigma
    px = np.stack([scene.pixels(X, c) for c in range(n_cam)], 1) + noise  # [N][C][2]
    z = np.stack([(X @ np.asarray(p["R"]).T + np.asarray(p["t"]).reshape(3))[:, 2] for p in scene.poses], 1)
    seen = (px[..., 0] >= 0) & (px[..., 0] < width) & (px[..., 1] >= 0) & (px[..., 1] < height) & (z > 0) & ~drop
    if mixed:
        both = np.flatnonzero(seen[:, 0] & seen[:, 1])
        seen[both, both % 2] = False
    keep = seen.sum(1) >= 2
    X, px, seen = X[keep], px[keep], seen[keep]
    return {"scene": scene, "image_points": np.ascontiguousarray(np.transpose(px, (1, 0, 2))), "valid": np.ascontiguousarray(seen.T),
            "X": X, "sigma": sigma, "prob": problem_from_arrays(np.transpose(px, (1, 0, 2)), seen.T, scene.camera_params)}


def problem_from_arrays(image_points, valid, camera_params):
    ip, valid = np.asarray(image_points, float), np.asarray(valid, bool)
    C, N = valid.shape
    n_idx, c_idx = np.nonzero(valid.T)
    K = np.array([np.asarray(camera_params[c]["intrinsic_matrix"], float) for c in range(C)])
    d = np.array([np.asarray(camera_params[c]["distortion_coef"], float).ravel()[:5] for c in range(C)])
    return Problem(n_idx, c_idx, ip[c_idx, n_idx], K, d, N)


def truth_in_camera0(scene, X):
    """The scene's poses and points re-expressed with camera 0 as the world frame: (R [C][3][3], t [C][3], X)"""
    R0, t0 = np.asarray(scene.poses[0]["R"], float), np.asarray(scene.poses[0]["t"], float).reshape(3)
    R = np.stack([np.asarray(p["R"], float) @ R0.T for p in scene.poses])
    t = np.stack([np.asarray(p["t"], float).reshape(3) - R[c] @ t0 for c, p in enumerate(scene.poses)])
    return R, t, X @ R0.T + t0


def perturbed_start(case, seed, rot=0.01, trans=0.02, point=0.01):
    """Truth moved by seeded Gaussian steps: rotation vectors (rad), translations and points (scene units)"""
    rng = np.random.default_rng(seed)
    R, t, X = truth_in_camera0(case["scene"], case["X"])
    R, t = R.copy(), t.copy()
    for c in range(1, len(R)):
        R[c] = exp_so3(rng.normal(0, rot, 3)) @ R[c]
        t[c] = t[c] + rng.normal(0, trans, 3)
    return R, t, X + rng.normal(0, point, X.shape)


CASES = {  # name -> (cameras, width, height, points, seed, sigma); start_seed for perturbed_start
    "clean6": (6, 1920, 1080, 400, 101, 0.0),
    "noisy6": (6, 1920, 1080, 400, 102, 0.5),
    "noisy16": (16, 3840, 2160, 2000, 103, 0.5),
    "mixed6": (6, 1920, 1080, 400, 104, 0.5),        # noisy6's sizes, six cameras of different K and lens
    "mixed6_clean": (6, 1920, 1080, 400, 105, 0.0),
}
MIXED = ("mixed6", "mixed6_clean")
# (mixed6: at 204 the ten permutations of order_spread all give the same cost, a spread of 0 that allows nothing; 214 was the
# next seed tried)
START_SEED = {"clean6": 201, "noisy6": 202, "noisy16": 203, "mixed6": 214, "mixed6_clean": 205}
# ftol of the loop comparison (tests/test_gpu_rig_ba.py): the loop stops on a step whose size is far above the rounding of the
# cost, see test_rig_ba_host.py::test_loop_cases_are_far_from_every_decision_boundary
LOOP_FTOL = 1e-9


def case(name, n_points=None):
    n_cam, w, h, n, seed, sigma = CASES[name]
    return _rig_case(n_cam, w, h, n_points or n, seed, sigma, mixed=name in MIXED)


def bundled():
    """The reference's own two-camera capture: 54 points (tests/golden/jsons/image_points.json), camera-params-in.json,
    start before_ba_extrinsics.json, and the reference's result after_ba_extrinsics.json.  Returns dict: prob, image_points
    [2][54][2], valid, camera_params, start (R, t), after (R, t)."""
    def load(name):
        with open(os.path.join(GOLDEN, "jsons", name)) as f:
            return json.load(f)
    ip = np.transpose(np.array(load("image_points.json"), float), (1, 0, 2))
    params = load("camera-params-in.json")
    valid = np.ones(ip.shape[:2], bool)
    poses = lambda ex: (np.array([p["R"] for p in ex], float), np.array([np.asarray(p["t"], float).reshape(3) for p in ex]))
    return {"prob": problem_from_arrays(ip, valid, params), "image_points": ip, "valid": valid, "camera_params": params,
            "start": poses(load("before_ba_extrinsics.json")), "after": poses(load("after_ba_extrinsics.json"))}


def mirrored(R, t, X):
    """(R, -t, -X): the same projections (x / z is unchanged) with every depth negated.  The reference's candidate vote
    (CalculateCameraPoses.py:214-219) picked the solution with every point BEHIND both cameras for its bundled capture;
    its mirror image is the state with the points in front."""
    return R, -np.asarray(t, float), -np.asarray(X, float)


def triangulate_dlt(prob, R, t):
    """Linear triangulation of every point from its observations (pinhole points undistorted by 5 fixed-point rounds): the
    start points where none are given"""
    X = np.zeros((prob.N, 3))
    rows = [[] for _ in range(prob.N)]
    for o in range(len(prob.pt)):
        c = prob.cam[o]
        x, y = undistort_normalised(prob.uv[o], prob.K[c], prob.dist[c])
        P = np.c_[R[c], t[c]]
        rows[prob.pt[o]] += [x * P[2] - P[0], y * P[2] - P[1]]
    for n in range(prob.N):
        v = np.linalg.svd(np.array(rows[n]))[2][-1]
        X[n] = v[:3] / v[3]
    return X


def undistort_normalised(uv, K, dist):
    k1, k2, p1, p2, k3 = dist
    x0, y0 = (uv[0] - K[0, 2]) / K[0, 0], (uv[1] - K[1, 2]) / K[1, 1]
    x, y = x0, y0
    for _ in range(5):
        r2 = x * x + y * y
        icd = 1.0 / (1 + ((k3 * r2 + k2) * r2 + k1) * r2)
        dx, dy = 2 * p1 * x * y + p2 * (r2 + 2 * x * x), p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
        x, y = (x0 - dx) * icd, (y0 - dy) * icd
    return x, y


def permuted(prob, seed):
    """The same problem with its observations in another order (seeded): what the order of the sums is worth"""
    p = np.random.default_rng(seed).permutation(len(prob.pt))
    return Problem(prob.pt[p], prob.cam[p], prob.uv[p], prob.K, prob.dist, prob.N)


def order_spread(prob, R, t, X, lam, n_perm=10, base=None):
    """Largest difference of cost, gradient, S and rhs between the sorted problem and n_perm seeded permutations of its
    observations, each relative to the quantity's largest entry: dict name -> spread.  base: the sorted problem's pieces,
    where the caller has them already."""
    if base is None:
        base = linearize(prob.sorted(), R, t, X, lam)
    out = {k: 0.0 for k in ("cost", "gradient", "S", "rhs")}
    for s in range(n_perm):
        lin = linearize(permuted(prob, 1000 + s), R, t, X, lam)
        for k in out:
            a, b = np.asarray(base[k], float), np.asarray(lin[k], float)
            out[k] = max(out[k], float(np.abs(a - b).max() / np.abs(a).max()))
    return out


# ---- the shapes ------------------------------------------------------------------------------------------------------------
def first_points(prob, X, n):
    """(the problem of the first n points, renumbered and sorted, their start X [n][3]): sets N exactly"""
    keep = prob.pt < n
    points = np.unique(prob.pt[keep])
    assert len(points) == n
    return Problem(np.searchsorted(points, prob.pt[keep]), prob.cam[keep], prob.uv[keep], prob.K, prob.dist, n).sorted(), X[points]


def lin_blocks(N):
    """Workgroups of the point-owning kernels: PT_THREADS = 256 points each (csrc/kernels.h, rig_args' n_lin_blocks)"""
    return -(-N // 256)


def schur_chunks(N):
    """(workgroups per camera pair of rig_schur_kernel, points of the last one): SCHUR_CHUNK = 1024 points each (csrc/rig_ba.hip)"""
    chunks = -(-N // 1024)
    return chunks, N - 1024 * (chunks - 1)


# The rigs of tests/test_gpu_rig_ba_shapes.py, each named for the seam of the pose-only solver it stands on: name -> (cameras,
# points drawn, points kept, seed of _rig_case, seed of perturbed_start, loss scale or None, rig_robust_ref.dirty data, the
# small perturbation of test_thirty_two_cameras_with_64_points, walks the loop).  All 1920 x 1080, sigma 0.5 px, dropout 0.3;
# _rig_case drops the points that fewer than two cameras see, so more are drawn than kept and the first `kept` are the case.
# PT_THREADS = 256 points make a workgroup of the point kernels, SCHUR_CHUNK = 1024 one of the Schur kernel, 90 rows (16
# cameras) is the most the Cholesky holds in LDS, rig_init_kernel and rig_finish_kernel have at most 1024 x 256 = 262 144
# threads for their 3 N and N loops.
# Seeds that are not the first tried, and why (tests/test_rig_ba_host.py asserts what they are chosen for): 302 and 306 are the
# first at which points 255 and 256 of the 4-camera rigs, and 1023 and 1024 of the 3-camera ones, are each seen by two free
# cameras; pose_2049_cauchy has seed 354 AND the small perturbation, see
# test_rig_ba_host.py::test_shape_loop_cases_are_far_from_every_decision_boundary; from start 405 the fifth iteration of pose_c17 lowers the cost by 1.05 x ftol, too near the stop to compare
# loops (from 407: 17.6 x and 0.005 x).
SHAPE_CASES = {
    "pose_two": (2, 1500, 600, 301, 401, None, False, False, True),
    "pose_255": (4, 400, 255, 302, 402, None, False, False, False),
    "pose_256": (4, 400, 256, 302, 402, None, False, False, False),
    "pose_257": (4, 400, 257, 302, 402, None, False, False, True),
    "pose_1023": (3, 1600, 1023, 306, 403, None, False, False, False),
    "pose_1024": (3, 1600, 1024, 306, 403, None, False, False, False),
    "pose_1025": (3, 1600, 1025, 306, 403, None, False, False, True),
    "pose_2049_cauchy": (3, 3200, 2049, 354, 404, 2.0, True, True, True),
    "pose_c17": (17, 330, 300, 305, 407, None, False, False, True),
    "pose_c17_cauchy": (17, 330, 300, 305, 407, 2.0, False, False, True),
    "pose_c32_cauchy": (32, 150, 140, 309, 406, 2.0, False, True, True),
    "pose_stride_3n": (2, 205000, 87382, 307, 407, None, False, False, False),
    "pose_stride_n": (2, 610000, 262145, 308, 408, None, False, False, False),
}
SHAPE_LOOPS = [k for k, v in SHAPE_CASES.items() if v[8]]
SHAPE_STRIDES = ("pose_stride_3n", "pose_stride_n")  # 2 permutations for the spread, and no loop of the restatement
# the cases whose LAST point stands on a seam: the first of a second workgroup, or alone in the last Schur chunk, or on the
# second trip of a grid-stride loop
SHAPE_SEAMS = ("pose_256", "pose_257", "pose_1024", "pose_1025", "pose_2049_cauchy", "pose_stride_3n", "pose_stride_n")

_shape_cases, _shape_pieces, _shape_loops = {}, {}, {}


def shape_case(name):
    """A case of SHAPE_CASES, computed once: dict with prob (sorted, exactly the N named), R, t, X (the start; camera 0 exactly
    the world frame), loss_c (None or the Cauchy scale), cpu_s (what making it took)"""
    if name not in _shape_cases:
        import time
        t0 = time.process_time()
        n_cam, n_draw, n_keep, seed, start_seed, loss_c, dirty, small, _ = SHAPE_CASES[name]
        c = _rig_case(n_cam, 1920, 1080, n_draw, seed, 0.5)
        R, t, X = perturbed_start(c, start_seed, **({"rot": 0.003, "trans": 0.005, "point": 0.005} if small else {}))
        assert c["prob"].N >= n_keep, (name, c["prob"].N)
        c = {**c, "X": c["X"][:n_keep], "image_points": c["image_points"][:, :n_keep], "valid": c["valid"][:, :n_keep],
             "prob": first_points(c["prob"], X, n_keep)[0]}
        X = X[:n_keep]
        if dirty:
            import rig_robust_ref
            c = rig_robust_ref.dirty(c)
        # the gauge of the definition, which the device imposes on the state it is handed and `lm` on its own: perturbed_start
        # leaves camera 0 a few 1e-16 off the world frame, and `linearize` would take that as it comes
        R[0], t[0] = np.eye(3), 0.0
        _shape_cases[name] = {"prob": c["prob"].sorted(), "R": R, "t": t, "X": X, "loss_c": loss_c, "cpu_s": time.process_time() - t0}
    return _shape_cases[name]


def shape_linearize(prob, R, t, X, lam, loss_c):
    """linearize, or rig_robust_ref.linearize under a loss"""
    if loss_c is None:
        return linearize(prob, R, t, X, lam)
    import rig_robust_ref
    return rig_robust_ref.linearize(prob, R, t, X, lam, loss_c)


def shape_pieces(name):
    """(the restatement's cost, gradient, S, rhs of the case's start at lambda = 1e-3 on the sorted problem, their order_spread),
    computed once: 10 seeded permutations, 2 for SHAPE_STRIDES"""
    if name not in _shape_pieces:
        c = shape_case(name)
        args = (c["R"], c["t"], c["X"], 1e-3)
        n_perm = 2 if name in SHAPE_STRIDES else 10
        lin = shape_linearize(c["prob"], *args, c["loss_c"])
        ref = {k: lin[k] for k in ("cost", "gradient", "S", "rhs")}
        del lin
        if c["loss_c"] is None:
            spread = order_spread(c["prob"], *args, n_perm=n_perm, base=ref)
        else:
            import rig_robust_ref
            spread = rig_robust_ref.order_spread(c["prob"], *args, c["loss_c"], n_perm=n_perm)
        _shape_pieces[name] = (ref, spread)
    return _shape_pieces[name]


def shape_loop(name):
    """The restatement's loop at LOOP_FTOL from the case's start (rig_robust_ref.lm's dict under a loss), computed once"""
    if name not in _shape_loops:
        c = shape_case(name)
        if c["loss_c"] is None:
            _shape_loops[name] = lm(c["prob"], c["R"], c["t"], c["X"], ftol=LOOP_FTOL)
        else:
            import rig_robust_ref
            _shape_loops[name] = rig_robust_ref.lm(c["prob"], c["R"], c["t"], c["X"], c["loss_c"], ftol=LOOP_FTOL)
    return _shape_loops[name]
