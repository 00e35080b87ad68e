"""What the two NumPy restatements (tests/rig_ba_ref.py, tests/intrinsics_ref.py) share, as csrc/lm.h is what the two kernel
files share: the camera model with its derivatives, and the step-control rule.  Not a test module.

Every value is formed by the same operations in the same order as in csrc/lm.h (the library is built without fused
multiply-add)."""
import numpy as np

STOP_MAX_ITERS, STOP_FTOL, STOP_LAMBDA, STOP_CHOLESKY = 1, 2, 3, 4


def project(lens, q, t, uv):
    """Pinhole + Brown distortion of the points q + t in the camera frame, against their pixels uv [n][2].  lens = (fx, fy,
    cx, cy, k1, k2, p1, p2, k3), q = R X and t: three entries each; an entry is a number or an array [n].  Call it under
    np.errstate(all="ignore").  Returns the residual r [n][2], front [n] (z > 0), the 2x3 A = d pixel / d (q + t) as nested
    lists of arrays [n], and the intermediates the lens columns of a Jacobian need: dict of x, y, xy, r2, r4, r6, tx, ty, xd, yd."""
    fx, fy, cx, cy, k1, k2, p1, p2, k3 = lens
    px, py, pz = q[0] + t[0], q[1] + t[1], q[2] + t[2]
    x, y = px / pz, py / pz
    xx, yy, xy = x * x, y * y, x * y
    r2 = xx + yy
    r4 = r2 * r2
    r6 = r4 * r2
    cd = ((1.0 + k1 * r2) + k2 * r4) + k3 * r6
    tx, ty = r2 + 2.0 * xx, r2 + 2.0 * yy
    xd = (x * cd + (2.0 * p1) * xy) + p2 * tx
    yd = (y * cd + p1 * ty) + (2.0 * p2) * xy
    r = np.stack([(fx * xd + cx) - uv[:, 0], (fy * yd + cy) - uv[:, 1]], 1)
    e = (k1 + (2.0 * k2) * r2) + (3.0 * k3) * r4
    a00 = ((cd + (2.0 * xx) * e) + (2.0 * p1) * y) + (6.0 * p2) * x
    a01 = ((2.0 * xy) * e + (2.0 * p1) * x) + (2.0 * p2) * y
    a11 = ((cd + (2.0 * yy) * e) + (6.0 * p1) * y) + (2.0 * p2) * x
    b = [[fx * a00, fx * a01], [fy * a01, fy * a11]]
    iz = 1.0 / pz
    A = [[b[i][0] * iz, b[i][1] * iz, -((b[i][0] * x + b[i][1] * y) * iz)] for i in range(2)]
    return r, pz > 0.0, A, dict(x=x, y=y, xy=xy, r2=r2, r4=r4, r6=r6, tx=tx, ty=ty, xd=xd, yd=yd)


def pose_columns(A, q):
    """One row of the pose Jacobian under R <- Exp(w) R, t <- t + dt from the same row of A: the six columns w = A (-[q]x), dt = A"""
    return [A[2] * q[1] - A[1] * q[2], A[0] * q[2] - A[2] * q[0], A[1] * q[0] - A[0] * q[1], A[0], A[1], A[2]]


def control(state, cost, try_step, max_iters, ftol, lambda0):
    """The loop's control (Nielsen's rule) from a start `state` of cost `cost`.  try_step(state, lam) solves one step at the
    damping lam: None when a factorisation fails, else (trial state, its cost, every point in front, predicted reduction,
    |step|).  Returns (state, cost, status, history [iterations][4] = (cost after the iteration, lambda it was solved with,
    accepted, |step|), rho [iterations] (nan for a failed factorisation))."""
    lam, nu = float(lambda0), 2.0
    history, rhos, status, chol_prev = [], [], STOP_MAX_ITERS, False
    for it in range(max_iters):
        step = try_step(state, lam)
        used, accepted, norm, stop = lam, False, 0.0, 0
        if step is None:
            rhos.append(np.nan)
            if chol_prev:
                stop = STOP_CHOLESKY
            chol_prev = True
        else:
            chol_prev = False
            trial_state, trial, ok, pred, norm = step
            with np.errstate(all="ignore"):
                rho = (cost - trial) / pred
            rhos.append(rho)
            accepted = bool(ok and rho > 0.0)
            if accepted:
                with np.errstate(all="ignore"):
                    rel = (cost - trial) / cost
                state, cost = trial_state, trial
                f = 2.0 * rho - 1.0
                lam, nu = lam * max(1.0 / 3.0, 1.0 - (f * f) * f), 2.0
                if rel < ftol:
                    stop = STOP_FTOL
        if not accepted:
            lam, nu = lam * nu, 2.0 * nu
            if not stop and lam > 1e16:
                stop = STOP_LAMBDA
        history.append((cost, used, 1.0 if accepted else 0.0, norm))
        if stop:
            status = stop
            break
    return state, cost, status, np.array(history).reshape(-1, 4), np.array(rhos)
