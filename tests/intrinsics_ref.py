"""NumPy restatement of the intrinsic calibration the HIP kernels implement, and the seeded cases the
tests share.  Not a test module: the yardstick of tests/test_intrinsics_host.py, tests/test_gpu_intrinsics.py and
tests/test_gpu_intrinsics_shapes.py.

Definition (all FP64), per camera.  Views v of a planar board: board points (X, Y, 0), their pixels (u, v).  Unknowns: kd =
(fx, fy, cx, cy, k1, k2, p1, p2, k3) and per view a pose (R_v, t_v) board -> camera.  Residual of a point: the projection of
tests/lm_ref.py (pinhole + Brown distortion, shared with tests/rig_ba_ref.py) minus the pixel; cost 1/2 sum r^2; rms_px = sqrt(2 cost / points).
Analytic Jacobian, 15 columns per point: the 9 of kd, then the 6 of the local pose perturbation R <- Exp(w) R, t <- t + dt.
Per view the 136 sums of [J r]^T [J r] (16 columns) over its points in ascending order: U_v (9x9), W_v (9x6), V_v (6x6),
g_c, g_v, 2 cost.  Marquardt damping V*_v = V_v + lambda diag V_v, U* likewise; Schur complement on the views
S = U* - sum_v W_v V*_v^-1 W_v^T (views in ascending order, upper triangle, mirrored), Cholesky, back-substitution.  Gain
ratio, accept / reject, Nielsen's update, stopping rules and history row are lm_ref.control, the rig adjustment's too.  Every
camera has its own damping, stop and status.

Every per-point quantity and the small dense algebra (Cholesky 6x6 and 9x9, the triangular solves) are formed by the same
operations in the same order as csrc/intrinsics.hip and csrc/lm.h (the library is built without fused multiply-add); `permuted` measures
what the order of the sums over points and views is worth.

Initialisation (no start given): per view a Hartley-normalised DLT homography (smallest eigenvector of the 9x9 A^T A),
principal point ((w - 1) / 2, (h - 1) / 2), 1 / fx^2 and 1 / fy^2 from the 2x2 normal equations of two orthogonality
constraints per view, zero distortion, the poses from K^-1 H.  A camera must pass `layout_error` first.  `Degenerate` when the 2x2 determinant is <= 1e-10 (trace / 2)^2
or a solution is not finite and positive."""
import json
import os

import numpy as np

import lm_ref
from lm_ref import STOP_MAX_ITERS, STOP_FTOL, STOP_LAMBDA, STOP_CHOLESKY  # noqa: F401 (the tests read them from here)
from mocapv2_amd import synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
E_LAYOUT, E_BEHIND, E_DEGENERATE = -2, -3, -4  # MOCAP_INTR_E_*
LOOP_FTOL = 1e-9


class Degenerate(ValueError):
    pass


class Camera:
    """views: list of (obj [n][2], uv [n][2]); size (width, height)"""

    def __init__(self, views, size):
        self.views = [(np.ascontiguousarray(np.asarray(o, float)[:, :2]), np.ascontiguousarray(u, float).reshape(-1, 2)) for o, u in views]
        self.size = (int(size[0]), int(size[1]))
        self.n_points = sum(len(o) for o, _ in self.views)


# ---- the model ---------------------------------------------------------------------------------------------------------------
def observe(kd, R, t, obj, uv):
    """One view: residual r [n][2], Jacobian J [n][2][15] (kd's 9 columns, then w, dt), front [n] (z > 0)"""
    lens = [float(v) for v in kd]
    fx, fy = lens[:2]
    X, Y = obj[:, 0], obj[:, 1]
    q = [R[i, 0] * X + R[i, 1] * Y for i in range(3)]  # (Z = 0: the third product of R X is an exact zero and is left out)
    with np.errstate(all="ignore"):
        r, front, A, m = lm_ref.project(lens, q, t, uv)
        x, y, xy, r2, r4, r6 = m["x"], m["y"], m["xy"], m["r2"], m["r4"], m["r6"]
        J = np.zeros((len(X), 2, 15))
        J[:, 0, 0], J[:, 0, 2] = m["xd"], 1.0
        J[:, 1, 1], J[:, 1, 3] = m["yd"], 1.0
        J[:, 0, 4], J[:, 0, 5], J[:, 0, 6], J[:, 0, 7], J[:, 0, 8] = fx * (x * r2), fx * (x * r4), fx * (2.0 * xy), fx * m["tx"], fx * (x * r6)
        J[:, 1, 4], J[:, 1, 5], J[:, 1, 6], J[:, 1, 7], J[:, 1, 8] = fy * (y * r2), fy * (y * r4), fy * m["ty"], fy * (2.0 * xy), fy * (y * r6)
        for i in range(2):
            J[:, i, 9:] = np.stack(lm_ref.pose_columns(A[i], q), 1)
    return r, J, front


def view_costs(cam, kd, R, t):
    """(sum r^2 per view [n_views], every point in front)"""
    c, ok = np.zeros(len(cam.views)), True
    for v, (obj, uv) in enumerate(cam.views):
        r, _, front = observe(kd, R[v], t[v], obj, uv)
        c[v] = float(np.sum(r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]))
        ok = ok and bool(front.all())
    return c, ok


def cost_of(cam, kd, R, t):
    c, ok = view_costs(cam, kd, R, t)
    s = 0.0
    for v in c:
        s += v
    return 0.5 * s, ok


def residuals(cam, kd, R, t):
    return np.concatenate([observe(kd, R[v], t[v], obj, uv)[0].reshape(-1) for v, (obj, uv) in enumerate(cam.views)])


# ---- the small dense algebra, operation by operation as in the kernels ----------------------------------------------------------
def cholesky(A):
    """Lower factor of a symmetric positive definite matrix (its lower triangle is read), or None"""
    n = len(A)
    L = np.zeros((n, n))
    for j in range(n):
        s = A[j][j]
        for k in range(j):
            s = s - L[j][k] * L[j][k]
        if not (s > 0.0 and np.isfinite(s)):
            return None
        L[j][j] = np.sqrt(s)
        for i in range(j + 1, n):
            s = A[i][j]
            for k in range(j):
                s = s - L[i][k] * L[j][k]
            L[i][j] = s / L[j][j]
    return L


def chol_solve(L, b):
    n = len(L)
    x = np.array(b, float)
    for i in range(n):
        s = x[i]
        for k in range(i):
            s = s - L[i][k] * x[k]
        x[i] = s / L[i][i]
    for i in range(n - 1, -1, -1):
        s = x[i]
        for k in range(i + 1, n):
            s = s - L[k][i] * x[k]
        x[i] = s / L[i][i]
    return x


def linearize(cam, kd, R, t, lam):
    """The pieces of one iteration: dict with cost, front, gc [9], gv [n_views][6], gradient [9 + 6 n_views], U [9][9], S [9][9]
    (damped), rhs [9], and per view V, W, L (factor of V*), ok (every V* positive definite)."""
    nv = len(cam.views)
    U, gc, T, Yg, cost2 = np.zeros((9, 9)), np.zeros(9), np.zeros((9, 9)), np.zeros(9), 0.0
    gv, Vs, Ws, Ls = np.zeros((nv, 6)), [], [], []
    front, ok = True, True
    for v, (obj, uv) in enumerate(cam.views):
        r, J, fr = observe(kd, R[v], t[v], obj, uv)
        front = front and bool(fr.all())
        A = np.concatenate([J, r[:, :, None]], 2)  # [n][2][16]
        term = A[:, 0, :, None] * A[:, 0, None, :] + A[:, 1, :, None] * A[:, 1, None, :]
        M = np.zeros((16, 16))
        for p in range(len(obj)):
            M += term[p]
        Uv, Wv, Vv, gcv, gvv = M[:9, :9], M[:9, 9:15], M[9:15, 9:15], M[:9, 15], M[9:15, 15]
        U, gc, cost2 = U + Uv, gc + gcv, cost2 + M[15, 15]
        gv[v] = gvv
        Vd = Vv.copy()
        for i in range(6):
            Vd[i, i] = Vv[i, i] + lam * Vv[i, i]
        L = cholesky(Vd)
        Vs.append(Vv.copy()), Ws.append(Wv.copy()), Ls.append(L)
        if L is None:
            ok = False
            continue
        Y = np.array([chol_solve(L, Wv[i]) for i in range(9)])  # W V*^-1, row by row
        Tv = np.zeros((9, 9))
        for k in range(6):
            Tv += Y[:, k, None] * Wv[None, :, k]
        yg = np.zeros(9)
        for k in range(6):
            yg += Y[:, k] * gvv[k]
        T, Yg = T + Tv, Yg + yg
    S = np.zeros((9, 9))
    for i in range(9):
        for j in range(i, 9):
            u = U[i, j] + lam * U[i, j] if i == j else U[i, j]
            S[i, j] = S[j, i] = u - T[i, j]
    return {"cost": 0.5 * cost2, "front": front, "ok": ok, "gc": gc, "gv": gv, "gradient": np.r_[gc, gv.reshape(-1)], "U": U,
            "S": S, "rhs": Yg - gc, "V": Vs, "W": Ws, "L": Ls}


def exp_so3_left(w, R):
    """Exp(w) R by Rodrigues' formula, the kernel's operations (rotate_left of csrc/lm.h)"""
    th2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]
    th = np.sqrt(th2)
    ka, kb = (1.0, 0.5) if th < 1e-12 else (np.sin(th) / th, (1.0 - np.cos(th)) / th2)
    E = np.empty((3, 3))
    E[0, 0], E[1, 1], E[2, 2] = 1.0 + kb * (w[0] * w[0] - th2), 1.0 + kb * (w[1] * w[1] - th2), 1.0 + kb * (w[2] * w[2] - th2)
    E[0, 1], E[1, 0] = kb * (w[0] * w[1]) - ka * w[2], kb * (w[0] * w[1]) + ka * w[2]
    E[0, 2], E[2, 0] = kb * (w[0] * w[2]) + ka * w[1], kb * (w[0] * w[2]) - ka * w[1]
    E[1, 2], E[2, 1] = kb * (w[1] * w[2]) - ka * w[0], kb * (w[1] * w[2]) + ka * w[0]
    out = np.empty((3, 3))
    for i in range(3):
        for j in range(3):
            out[i, j] = (E[i, 0] * R[0, j] + E[i, 1] * R[1, j]) + E[i, 2] * R[2, j]
    return out


def schur_step(lin, lam):
    """(dc [9], dp [n_views][6], predicted reduction, |step|^2) from the pieces, or None when a factorisation fails"""
    if not lin["ok"]:
        return None
    L = cholesky(lin["S"])
    if L is None:
        return None
    dc = chol_solve(L, lin["rhs"])
    pred, n2 = 0.0, 0.0
    for i in range(9):
        pred += dc[i] * ((lam * lin["U"][i, i]) * dc[i] - lin["gc"][i])
        n2 += dc[i] * dc[i]
    nv = len(lin["V"])
    dp, pv, nn = np.zeros((nv, 6)), np.zeros(nv), np.zeros(nv)
    for v in range(nv):
        q = lin["gv"][v].copy()
        for i in range(9):
            q = q + lin["W"][v][i] * dc[i]
        dp[v] = -chol_solve(lin["L"][v], q)
        for k in range(6):
            pv[v] += dp[v, k] * ((lam * lin["V"][v][k, k]) * dp[v, k] - lin["gv"][v, k])
            nn[v] += dp[v, k] * dp[v, k]
    ps, ns = 0.0, 0.0
    for v in range(nv):
        ps, ns = ps + pv[v], ns + nn[v]
    return dc, dp, 0.5 * (ps + pred), ns + n2


def apply_step(kd, R, t, dc, dp):
    R2 = np.array([exp_so3_left(dp[v, :3], R[v]) for v in range(len(R))])
    return kd + dc, R2, t + dp[:, 3:]


def lm(cam, kd, R, t, max_iters=50, ftol=1e-12, lambda0=1e-3, trace=None):
    """The loop of one camera.  dict: kd, R, t, status, iterations, cost_initial, cost, rms_px, view_rms, history
    [iterations][4] = (cost after the iteration, lambda it was solved with, accepted, |step|), rho [iterations] (nan for a
    failed factorisation).  status E_BEHIND: the start is returned.  trace: a list that gets one dict per iteration, lam, lin (the
    pieces of linearize at that damping) and trial (the trial kd, R, t; None for a failed solve)."""
    kd, R, t = np.array(kd, float).reshape(9), np.array(R, float).reshape(-1, 3, 3), np.array(t, float).reshape(-1, 3)
    vc, front = view_costs(cam, kd, R, t)
    cost0 = cost_of(cam, kd, R, t)[0]
    n_pts = np.array([len(o) for o, _ in cam.views], float)
    if not front or not np.isfinite(cost0):
        return {"kd": kd, "R": R, "t": t, "status": E_BEHIND, "iterations": 0, "cost_initial": cost0, "cost": cost0,
                "history": np.zeros((0, 4)), "rho": np.zeros(0), "rms_px": np.nan, "view_rms": np.full(len(R), np.nan)}

    def try_step(state, lam):  # a state: (kd, R, t, its sum r^2 per view)
        kd, R, t, _ = state
        lin = linearize(cam, kd, R, t, lam)
        step = schur_step(lin, lam)
        if trace is not None:
            trace.append({"lam": lam, "lin": lin, "trial": None})
        if step is None:
            return None
        dc, dp, pred, n2 = step
        kd2, R2, t2 = apply_step(kd, R, t, dc, dp)
        if trace is not None:
            trace[-1]["trial"] = (kd2, R2, t2)
        vc2, ok = view_costs(cam, kd2, R2, t2)
        return (kd2, R2, t2, vc2), cost_of(cam, kd2, R2, t2)[0], ok, pred, float(np.sqrt(n2))

    (kd, R, t, vc), cost, status, history, rho = lm_ref.control((kd, R, t, vc), cost0, try_step, max_iters, ftol, lambda0)
    return {"kd": kd, "R": R, "t": t, "status": status, "iterations": len(history), "cost_initial": cost0, "cost": cost,
            "history": history, "rho": rho, "rms_px": float(np.sqrt(2.0 * cost / cam.n_points)), "view_rms": np.sqrt(vc / n_pts)}


# ---- initialisation --------------------------------------------------------------------------------------------------------------
def _hartley(p):
    c = p.mean(0)
    d = np.sqrt(((p - c) ** 2).sum(1)).mean()
    s = np.sqrt(2.0) / d
    return np.array([[s, 0, -s * c[0]], [0, s, -s * c[1]], [0, 0, 1.0]])


def layout_error(view_points):
    """The layout rule of a camera, from the point counts of its views: None, or what it lacks.  At least 3 views of at
    least 4 points each, and at least as many equations as unknowns: 2 points >= 9 + 6 views.  (3 views of 4 points, 24 for
    27, keep the damped normal matrix positive definite; the loop then fits the pixels exactly and reports a wrong lens with
    rms 0 and a positive status: tests/test_intrinsics_host.py::test_fewer_equations_than_unknowns_fit_a_wrong_lens.)"""
    n = [int(k) for k in view_points]
    if len(n) < 3:
        return f"{len(n)} views, at least 3 are needed"
    if min(n) < 4:
        return f"view {n.index(min(n))}: {min(n)} points, at least 4 are needed"
    if 2 * sum(n) < 9 + 6 * len(n):
        return f"{2 * sum(n)} equations for {9 + 6 * len(n)} unknowns"
    return None


def status_from_own_start(cam, max_iters=50, ftol=1e-12):
    """The status the definition gives a camera that brings no start: E_LAYOUT, E_DEGENERATE, or the loop's"""
    if layout_error([len(o) for o, _ in cam.views]) is not None:
        return E_LAYOUT
    try:
        start = initialise(cam)
    except Degenerate:
        return E_DEGENERATE
    return lm(cam, *start, max_iters=max_iters, ftol=ftol)["status"]


def homography(obj, uv, null="eigh"):
    """Hartley-normalised DLT over all points: H with (u, v, 1) ~ H (X, Y, 1), H[2][2] = 1.  null: the route to the null
    vector, "eigh" (smallest eigenvector of A^T A, the definition's) or "svd" (last right singular vector of A, SciPy's: a
    second correct FP64 route, for `start_spread`)"""
    To, Ti = _hartley(obj), _hartley(uv)
    o = obj * To[0, 0] + To[:2, 2]
    i = uv * Ti[0, 0] + Ti[:2, 2]
    n = len(obj)
    A = np.zeros((2 * n, 9))
    A[0::2, 0], A[0::2, 1], A[0::2, 2] = -o[:, 0], -o[:, 1], -1.0
    A[0::2, 6], A[0::2, 7], A[0::2, 8] = i[:, 0] * o[:, 0], i[:, 0] * o[:, 1], i[:, 0]
    A[1::2, 3], A[1::2, 4], A[1::2, 5] = -o[:, 0], -o[:, 1], -1.0
    A[1::2, 6], A[1::2, 7], A[1::2, 8] = i[:, 1] * o[:, 0], i[:, 1] * o[:, 1], i[:, 1]
    if null == "svd":
        from scipy import linalg
        Hn = linalg.svd(A)[2][-1].reshape(3, 3)
    else:
        w, V = np.linalg.eigh(A.T @ A)
        Hn = V[:, 0].reshape(3, 3)
    H = np.linalg.inv(Ti) @ Hn @ To
    return H / H[2, 2]


def initialise(cam, null="eigh"):
    """(kd [9], R [n_views][3][3], t [n_views][3]) of the definition; raises Degenerate"""
    w, h = cam.size
    cx, cy = (w - 1) / 2.0, (h - 1) / 2.0
    Hs = [homography(o, u, null) for o, u in cam.views]
    AtA, Atb = np.zeros((2, 2)), np.zeros(2)
    for H in Hs:
        Hc = H.copy()
        Hc[0] -= cx * H[2]
        Hc[1] -= cy * H[2]
        hh, vv = Hc[:, 0], Hc[:, 1]
        d1, d2 = (hh + vv) * 0.5, (hh - vv) * 0.5
        hh, vv, d1, d2 = (a / np.sqrt(a @ a) for a in (hh, vv, d1, d2))
        for a, b in ((hh, vv), (d1, d2)):
            row, rhs = np.array([a[0] * b[0], a[1] * b[1]]), -a[2] * b[2]
            AtA += np.outer(row, row)
            Atb += row * rhs
    det, tr = AtA[0, 0] * AtA[1, 1] - AtA[0, 1] * AtA[0, 1], AtA[0, 0] + AtA[1, 1]
    if not det > 1e-10 * (0.5 * tr) ** 2:
        raise Degenerate(f"determinant {det:.3e} of trace^2 {tr * tr:.3e}")
    a = (AtA[1, 1] * Atb[0] - AtA[0, 1] * Atb[1]) / det
    b = (AtA[0, 0] * Atb[1] - AtA[0, 1] * Atb[0]) / det
    if not (np.isfinite(a) and np.isfinite(b) and a > 0 and b > 0):
        raise Degenerate(f"1 / fx^2 = {a}, 1 / fy^2 = {b}")
    fx, fy = np.sqrt(1.0 / a), np.sqrt(1.0 / b)
    R, t = [], []
    for H in Hs:
        M = np.stack([(H[0] - cx * H[2]) / fx, (H[1] - cy * H[2]) / fy, H[2]])
        m1, m2, m3 = M[:, 0], M[:, 1], M[:, 2]
        s = 2.0 / (np.sqrt(m1 @ m1) + np.sqrt(m2 @ m2))
        if s * m3[2] < 0:
            s = -s
        r1 = s * m1
        r1 = r1 / np.sqrt(r1 @ r1)
        r3 = np.cross(r1, s * m2)
        r3 = r3 / np.sqrt(r3 @ r3)
        r2 = np.cross(r3, r1)
        R.append(np.stack([r1, r2, r3], 1))
        t.append(s * m3)
    return np.array([fx, fy, cx, cy, 0, 0, 0, 0, 0.0]), np.array(R), np.array(t)


# ---- SciPy as the independent minimiser -----------------------------------------------------------------------------------------
def scipy_minimum(cam, kd, R, t, max_nfev=400):
    """least_squares ('trf', x_scale='jac', tolerances 1e-12) on this file's residual and analytic Jacobian from the same
    start.  Parameters: kd, then per view a rotation vector and a translation around the START pose.  Returns (cost, kd)."""
    from scipy import optimize
    from rig_ba_ref import _left_jacobian
    kd0, R0, t0 = np.array(kd, float), np.array(R, float), np.array(t, float)
    nv = len(R0)
    rows = np.cumsum([0] + [2 * len(o) for o, _ in cam.views])

    def state(x):
        d = x[9:].reshape(nv, 6)
        return x[:9], np.array([exp_so3_left(d[v, :3], R0[v]) for v in range(nv)]), t0 + d[:, 3:]

    def fun(x):
        return residuals(cam, *state(x))

    def jac(x):
        k, Rn, tn = state(x)
        Jm = np.zeros((rows[-1], 9 + 6 * nv))
        for v, (obj, uv) in enumerate(cam.views):
            J = observe(k, Rn[v], tn[v], obj, uv)[1].copy()
            J[:, :, 9:12] = J[:, :, 9:12] @ _left_jacobian(x[9 + 6 * v:12 + 6 * v])
            Jm[rows[v]:rows[v + 1], :9] = J[:, :, :9].reshape(-1, 9)
            Jm[rows[v]:rows[v + 1], 9 + 6 * v:15 + 6 * v] = J[:, :, 9:].reshape(-1, 6)
        return Jm

    res = optimize.least_squares(fun, np.r_[kd0, np.zeros(6 * nv)], jac=jac, method="trf", x_scale="jac", ftol=1e-12, xtol=1e-12,
                                 gtol=1e-12, max_nfev=max_nfev)
    return float(res.cost), res.x[:9].copy()


# ---- the cases -------------------------------------------------------------------------------------------------------------------
def board(nx, ny, square):
    """nx x ny corners, row by row"""
    j, i = np.meshgrid(np.arange(ny), np.arange(nx), indexing="ij")
    return np.stack([i.reshape(-1) * square, j.reshape(-1) * square], 1).astype(float)


BOARD_54 = board(6, 9, 0.03)     # the reference's
BOARD_99 = board(9, 11, 0.022)   # more than a wave of 64


def golden_lens():
    with open(os.path.join(GOLDEN, "jsons", "camera-intrinsics.json")) as f:
        p = json.load(f)
    return np.array(p["intrinsic_matrix"], float), np.array(p["distortion_coef"], float).ravel()[:5]


LENSES = {  # name -> (K, dist, (width, height), (nearest, farthest board distance))
    "mild": lambda: (synth.intrinsics(1920, 1080), np.array(synth.MILD_DIST, float), (1920, 1080), (0.5, 1.2)),
    "golden": lambda: (*golden_lens(), (2448, 2048), (0.8, 1.6)),
}


def _rot(axis, a):
    c, s = np.cos(a), np.sin(a)
    i, j = [(1, 2), (2, 0), (0, 1)][axis]
    R = np.eye(3)
    R[i, i], R[i, j], R[j, i], R[j, j] = c, -s, s, c
    return R


def random_view(rng, pts, K, dist, size, dist_range, tilt=0.6):
    """A seeded board pose with every corner inside the image: tilt within +-tilt rad about x and y, any in-plane angle, the
    board's centre at 25-75 % of the image, its distance within dist_range.  Returns (R, t, exact pixels)."""
    w, h = size
    centre = np.r_[pts.mean(0), 0.0]
    P3 = np.c_[pts, np.zeros(len(pts))]
    for _ in range(10000):
        a, b, g = rng.uniform(-tilt, tilt), rng.uniform(-tilt, tilt), rng.uniform(-np.pi, np.pi)
        u, v, d = rng.uniform(0.25, 0.75) * w, rng.uniform(0.25, 0.75) * h, rng.uniform(*dist_range)
        R = _rot(2, g) @ _rot(0, a) @ _rot(1, b)
        pc = d * np.array([(u - K[0, 2]) / K[0, 0], (v - K[1, 2]) / K[1, 1], 1.0])
        t = pc - R @ centre
        px = synth.project(P3, {"R": R, "t": t}, K, dist)
        if (px[:, 0] >= 0).all() and (px[:, 0] <= w - 1).all() and (px[:, 1] >= 0).all() and (px[:, 1] <= h - 1).all():
            return R, t, px
    raise RuntimeError("no view fits the image")


CASES = {  # name -> (lens, seed, point counts of the views, sigma)
    "clean_mild": ("mild", 301, (54, 54, 54), 0.0),
    "clean_golden": ("golden", 302, (54,) * 5, 0.0),
    "noisy_mild": ("mild", 303, (54,) * 8, 0.3),
    "noisy_golden": ("golden", 304, (54, 99, 35, 54, 99, 35, 54, 99, 35, 54, 99, 35), 0.3),
}
RIG3 = ("clean_mild", "noisy_golden", "noisy_mild")
BOARD_20 = board(4, 5, 0.04)      # few corners, for cameras of many views
BOARD_221 = board(13, 17, 0.015)  # a fine board: four chunks of 64 points, the last of 29
# Outside the shapes the kernels' header calls typical (tests/test_gpu_intrinsics_shapes.py): name -> (lens, seed, point
# counts of the views, sigma, board).  A view of fewer points than the board has is a seeded subset, rows in board order.
SHAPE_CASES = {
    "many_views": ("mild", 501, (20,) * 70, 0.3, BOARD_20),   # past the 64 lanes that deal a camera's views, by 6
    "views_64": ("mild", 502, (20,) * 64, 0.3, BOARD_20),     # the exact edge,
    "views_65": ("mild", 503, (20,) * 65, 0.3, BOARD_20),     # and one view in the second pass
    "edge_points": ("mild", 504, (63, 64, 65, 127, 128, 129, 221), 0.3, BOARD_221),  # chunks of 64: last of 63, 64, 1, 63, 64, 1, 29
    "small": ("mild", 505, (5, 5, 5), 0.3, BOARD_54),         # 30 equations, 27 unknowns: the smallest layout with 3 views
}
SHAPES3 = ("edge_points", "many_views", "small")
RAGGED5 = ("clean_mild", "noisy_golden", "noisy_mild", "edge_points", "small")  # five different cameras, 33 views, 2 158 points
SHAPE_START_SEED ={"edge_points": 404, "many_views": 405, "small": 406}  # of perturbed_start
LAYOUT_CASES = {  # around the layout rule 2 points >= 9 + 6 views; nothing is asserted about the lens they give
    "three_by_four": ("mild", 506, (4, 4, 4), 0.3, BOARD_54),  # 24 equations, 27 unknowns: refused
    "five_by_four": ("mild", 507, (4,) * 5, 0.3, BOARD_54),    # 40 for 39: accepted by the rule
}
_made = {}


def case(name):
    """dict: cam (Camera), kd (truth), R, t (true poses), sigma.  From default_rng(seed), per view in order: the pose draws,
    the partial view's choice of corners, the pixel noise."""
    if name in _made:
        return _made[name]
    lens, seed, counts, sigma, *own = next(d[name] for d in (CASES, SHAPE_CASES, LAYOUT_CASES) if name in d)
    K, dist, size, rng_d = LENSES[lens]()
    rng = np.random.default_rng(seed)
    views, Rs, ts = [], [], []
    for n in counts:
        pts = own[0] if own else BOARD_99 if n == 99 else BOARD_54
        R, t, px = random_view(rng, pts, K, dist, size, rng_d)
        if n < len(pts):
            keep = np.sort(rng.choice(len(pts), n, replace=False))
            pts, px = pts[keep], px[keep]
        px = px + rng.normal(0, 1.0, px.shape) * sigma
        views.append((pts, px))
        Rs.append(R), ts.append(t)
    kd = np.r_[K[0, 0], K[1, 1], K[0, 2], K[1, 2], dist]
    _made[name] = {"cam": Camera(views, size), "kd": kd, "R": np.array(Rs), "t": np.array(ts), "sigma": sigma, "name": name}
    return _made[name]


def fronto_parallel(seed=305, n_views=4):
    """A camera whose views are all exactly fronto-parallel (tilt 0): the focal lengths cannot be told from the distances"""
    K, dist, size, rng_d = LENSES["mild"]()
    rng = np.random.default_rng(seed)
    views = []
    for _ in range(n_views):
        _, _, px = random_view(rng, BOARD_54, K, np.zeros(5), size, rng_d, tilt=0.0)
        views.append((BOARD_54, px))
    return Camera(views, size)


def failed_cameras():
    """Cameras that cannot be calibrated, name -> (Camera, the status it must report): two views; none at all (the offsets
    admit it); four views of which one has no points; fronto-parallel views"""
    good = case("noisy_mild")["cam"]
    none = np.zeros((0, 2))
    return {"two_views": (Camera(good.views[:2], good.size), E_LAYOUT),
            "no_views": (Camera([], good.size), E_LAYOUT),
            "empty_view": (Camera([good.views[0], (none, none), good.views[2], good.views[3]], good.size), E_LAYOUT),
            "fronto_parallel": (fronto_parallel(), E_DEGENERATE)}


def start_spread(cam, n_perm=10):
    """How far two correct FP64 routes to the initialisation lie apart, as the cost at the start relative to `initialise`'s:
    (the null vector by scipy.linalg.svd(A) instead of eigh(A^T A); the largest over n_perm seeded permutations of the points
    within the views, by eigh).  The device's route is a third, cyclic Jacobi on A^T A."""
    base = cost_of(cam, *initialise(cam))[0]
    svd = abs(cost_of(cam, *initialise(cam, "svd"))[0] / base - 1)
    perm = 0.0
    for s in range(n_perm):
        rng = np.random.default_rng(3000 + s)
        views = []
        for o, u in cam.views:
            p = rng.permutation(len(o))
            views.append((o[p], u[p]))
        cam2 = Camera(views, cam.size)
        perm = max(perm, abs(cost_of(cam2, *initialise(cam2))[0] / base - 1))
    return float(svd), float(perm)


def with_a_bad_view(cam, bad, shift=5.0, seed=306):
    """The camera with every point of view `bad` moved by `shift` px, each in its own seeded direction: a view whose corners
    were found badly.  (The same shift for all its points is no such view: it is a board moved sideways, which the view's pose
    takes up, leaving its view_rms where it was -- tests/test_intrinsics_host.py shows it.)"""
    ang = np.random.default_rng(seed).uniform(0.0, 2.0 * np.pi, len(cam.views[bad][0]))
    d = shift * np.stack([np.cos(ang), np.sin(ang)], 1)
    return Camera([(o, u + d) if v == bad else (o, u) for v, (o, u) in enumerate(cam.views)], cam.size)


def perturbed_start(c, seed, rel=2e-3, coef=2e-3, rot=0.01, trans=0.005):
    """The truth moved by seeded Gaussian steps: (kd, R, t)"""
    rng = np.random.default_rng(seed)
    kd = c["kd"].copy()
    kd[:4] *= 1.0 + rng.normal(0, rel, 4)
    kd[4:] += rng.normal(0, coef, 5)
    R = np.array([exp_so3_left(rng.normal(0, rot, 3), Rv) for Rv in c["R"]])
    return kd, R, c["t"] + rng.normal(0, trans, c["t"].shape)


def permuted(cam, R, t, seed):
    """The same problem with the points of every view and the views in another order (seeded): (cam, R, t, view order)"""
    rng = np.random.default_rng(seed)
    order = rng.permutation(len(cam.views))
    views = []
    for v in order:
        o, u = cam.views[v]
        p = rng.permutation(len(o))
        views.append((o[p], u[p]))
    return Camera(views, cam.size), np.asarray(R)[order], np.asarray(t)[order], order


def _in_order(lin, order):
    """the gradient of a permuted problem with its views back in the original order"""
    gv = np.empty_like(lin["gv"])
    gv[order] = lin["gv"]
    return np.r_[lin["gc"], gv.reshape(-1)]


def order_spread(cam, kd, R, t, lam, n_perm=10):
    """Largest difference of cost, gradient, S and rhs between the problem and n_perm seeded permutations, each relative to
    the quantity's largest entry: dict name -> spread"""
    base = linearize(cam, kd, R, t, lam)
    out = {k: 0.0 for k in ("cost", "gradient", "S", "rhs")}
    for s in range(n_perm):
        cam2, R2, t2, order = permuted(cam, R, t, 1000 + s)
        lin = linearize(cam2, kd, R2, t2, lam)
        lin = dict(lin, gradient=_in_order(lin, order))
        for k in out:
            a, b = np.asarray(base[k], float), np.asarray(lin[k], float)
            out[k] = max(out[k], float(np.abs(a - b).max() / np.abs(a).max()))
    return out


def loop_spreads(cam, kd, R, t, ftol=LOOP_FTOL, max_iters=50, lambda0=1e-3, n_perm=10):
    """The loop on the problem and on n_perm seeded permutations: (base run, with its trace; every run took the base run's
    decisions: iterations, status, accept sequence, failed solves; spread).  spread: dict of cost, lambda, step [iterations], the largest
    relative difference of that history column from the base run's in each iteration (0 where the base entry is 0), and of
    kd, poses: the largest difference of the returned state, relative to the array's largest entry (poses: R and t of every
    view as [12], views back in the problem's order).  Runs that decided otherwise are left out of the spread."""
    trace = []
    base = lm(cam, kd, R, t, max_iters, ftol, lambda0, trace=trace)
    base["trace"] = trace
    n = base["iterations"]
    same, spread = True, {"cost": np.zeros(n), "lambda": np.zeros(n), "step": np.zeros(n), "kd": 0.0, "poses": 0.0}
    state = lambda run, order=None: np.c_[run["R"].reshape(-1, 9), run["t"]] if order is None else np.c_[run["R"].reshape(-1, 9), run["t"]][np.argsort(order)]
    for s in range(n_perm):
        cam2, R2, t2, order = permuted(cam, R, t, 2000 + s)
        run = lm(cam2, kd, R2, t2, max_iters, ftol, lambda0)
        if (run["iterations"] != n or run["status"] != base["status"] or not np.array_equal(run["history"][:, 2], base["history"][:, 2])
                or not np.array_equal(np.isnan(run["rho"]), np.isnan(base["rho"]))):
            same = False
            continue
        for k, col in (("cost", 0), ("lambda", 1), ("step", 3)):
            a, b = base["history"][:, col], run["history"][:, col]
            spread[k] = np.maximum(spread[k], np.where(a == 0, np.abs(b), np.abs(b / np.where(a == 0, 1.0, a) - 1)))
        spread["kd"] = max(spread["kd"], float(np.abs(run["kd"] - base["kd"]).max() / np.abs(base["kd"]).max()))
        spread["poses"] = max(spread["poses"], float(np.abs(state(run, order) - state(base)).max() / np.abs(state(base)).max()))
    return base, same, spread


def loop_spread(cam, kd, R, t, ftol=LOOP_FTOL, n_perm=10, max_iters=50, lambda0=1e-3):
    """loop_spreads with the spread of the per-iteration cost only, as one number: (base run, same decisions, spread)"""
    base, same, spread = loop_spreads(cam, kd, R, t, ftol, max_iters, lambda0, n_perm)
    return base, same, float(spread["cost"].max()) if len(spread["cost"]) else 0.0


def param_errors(kd, truth):
    """(largest relative error of fx, fy, cx, cy; largest absolute error of the five coefficients)"""
    return float(np.abs(kd[:4] / truth[:4] - 1).max()), float(np.abs(kd[4:] - truth[4:]).max())
