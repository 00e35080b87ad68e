"""NumPy restatement of mocap_refine_points' definition: every row's point moved to the minimum of its
reprojection error by Levenberg-Marquardt, with (J^T J)^-1 there.  Not a test module.

FP64 only, + - * / only, every operation rounded on its own and formed in the order of csrc/refine_points.hip (the library is
built without fused multiply-add); sums run in ascending camera order, each from 0.  The camera model is lm_ref.project and the
loop's control lm_ref.control, as the kernel's are lm.h's project and lm_decide.  A row's members are handled as arrays [m];
the rows one after another (the kernel: one lane per row)."""
import numpy as np

import lm_ref

E_VIEWS, E_INPUT, E_BEHIND = -2, -3, -4
ZERO = np.float64(0.0)


def seq_sum(v):
    """0 + v[0] + v[1] + ... in that order"""
    return np.add.accumulate(np.concatenate([[0.0], v]))[-1]


def inv_sym3(v):
    """lm.h's inv_sym3: the inverse of the symmetric 3x3 with upper triangle v = (00, 01, 02, 11, 12, 22) by the adjugate, in
    the same layout, and the determinant it divides by"""
    c00, c01, c02 = v[3] * v[5] - v[4] * v[4], v[2] * v[4] - v[1] * v[5], v[1] * v[4] - v[2] * v[3]
    det = (v[0] * c00 + v[1] * c01) + v[2] * c02
    c11, c12, c22 = v[0] * v[5] - v[2] * v[2], v[1] * v[2] - v[0] * v[4], v[0] * v[3] - v[1] * v[1]
    with np.errstate(all="ignore"):
        return np.array([c00 / det, c01 / det, c02 / det, c11 / det, c12 / det, c22 / det]), det


class Rig:
    """K, dist, R, t of C cameras as the kernel stages them; distorted = 0 gives every camera five zeros for its lens"""

    def __init__(self, K, dist, R, t, distorted=0):
        self.K = np.asarray(K, np.float64).reshape(-1, 9)
        self.C = C = len(self.K)
        self.dist = np.asarray(dist, np.float64).reshape(C, 5) if distorted else np.zeros((C, 5))
        self.R = np.asarray(R, np.float64).reshape(C, 9)
        self.t = np.asarray(t, np.float64).reshape(C, 3)


def members_pass(rig, members, obs, X):
    """One pass over the members (ascending camera numbers [m]) with observations obs [m][2] at X [3].  Returns dict: S (sum of
    the squared residual lengths), H (upper triangle of J^T J), g (J^T r), front (X in front of every member), res2 [m], worst
    (position in `members` of the largest res2, the first of equals)"""
    R, K, d = rig.R[members], rig.K[members], rig.dist[members]
    with np.errstate(all="ignore"):
        q = [(R[:, 3 * i] * X[0] + R[:, 3 * i + 1] * X[1]) + R[:, 3 * i + 2] * X[2] for i in range(3)]
        lens = (K[:, 0], K[:, 4], K[:, 2], K[:, 5], d[:, 0], d[:, 1], d[:, 2], d[:, 3], d[:, 4])
        r, front, A, _ = lm_ref.project(lens, q, [rig.t[members, i] for i in range(3)], obs)
        res2 = r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]
        J = [[(A[i][0] * R[:, j] + A[i][1] * R[:, 3 + j]) + A[i][2] * R[:, 6 + j] for j in range(3)] for i in range(2)]
        H = np.array([seq_sum(J[0][a] * J[0][b] + J[1][a] * J[1][b]) for a, b in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))])
        g = np.array([seq_sum(J[0][j] * r[:, 0] + J[1][j] * r[:, 1]) for j in range(3)])
        S = seq_sum(res2)
    worst, worst_r2 = 0, -1.0
    for k, v in enumerate(res2):
        if v > worst_r2:
            worst, worst_r2 = k, v
    return dict(S=S, H=H, g=g, front=bool(front.all()), res2=res2, worst=worst)


def _try_step(rig, members, obs):
    def try_step(state, lam):
        X, e = state
        H, g = e["H"], e["g"]
        with np.errstate(all="ignore"):
            inv, det = inv_sym3(np.array([H[0] + lam * H[0], H[1], H[2], H[3] + lam * H[3], H[4], H[5] + lam * H[5]]))
            if not det > 0.0 or not np.isfinite(det):
                return None
            d = np.array([-((inv[0] * g[0] + inv[1] * g[1]) + inv[2] * g[2]), -((inv[1] * g[0] + inv[3] * g[1]) + inv[4] * g[2]),
                          -((inv[2] * g[0] + inv[4] * g[1]) + inv[5] * g[2])])
            diag = (H[0], H[3], H[5])
            pred, n2 = ZERO, ZERO
            for j in range(3):
                pred = pred + d[j] * ((lam * diag[j]) * d[j] - g[j])
                n2 = n2 + d[j] * d[j]
            Xt = X + d
            tr = members_pass(rig, members, obs, Xt)
            ok = bool(np.isfinite(Xt).all() and tr["front"])
            # (lm_decide sums the partials from 0 and adds the cameras' share, 0 here)
            return (Xt, tr), 0.5 * (ZERO + tr["S"]), ok, 0.5 * ((ZERO + pred) + ZERO), np.sqrt((ZERO + n2) + ZERO)
    return try_step


def refine_row(rig, X0, mask, obs_of, max_iters=10, ftol=1e-9, lambda0=1e-3, max_res2=0.0, min_views=2, max_drop=0):
    """One row.  mask: the member cameras' bits; obs_of(c): camera c's observation (u, v), or None for an index outside the
    list.  Returns dict: status, xyz, views -- and for a refined row err, res2 [C] (-1 = no member), cov [6], dropped, iters,
    and beside the definition's outputs cost0 (1/2 sum r^2 of the point handed in under the mask handed in), history (the
    loops' lm_ref.control histories, one after another)."""
    C = rig.C
    X = np.array(X0, np.float64).reshape(3)
    mask = int(mask)
    err_row = lambda code: dict(status=code, xyz=X.copy(), views=mask)
    if mask >> C or not np.isfinite(X).all():
        return err_row(E_INPUT)
    members = [c for c in range(C) if mask >> c & 1]
    obs = [obs_of(c) for c in members]
    if any(o is None for o in obs):
        return err_row(E_INPUT)
    if len(members) < 2:
        return err_row(E_VIEWS)
    members, obs = np.array(members), np.array(obs, np.float64).reshape(-1, 2)
    dropped, iters, drops, history, cost0 = 0, 0, 0, [], None
    while True:
        e = members_pass(rig, members, obs, X)
        if iters == 0:
            if not e["front"]:
                return err_row(E_BEHIND)
            cost0 = 0.5 * e["S"]
        (X, e), cost, status, hist, _ = lm_ref.control((X, e), 0.5 * e["S"], _try_step(rig, members, obs), max_iters, ftol, lambda0)
        iters += len(hist)
        history.append(hist)
        # (the pass behind the loop: the same operations at the same point as the pass that was accepted, so the same bits)
        if max_res2 > 0.0 and len(members) > min_views and drops < max_drop and e["res2"][e["worst"]] > max_res2:
            dropped |= 1 << int(members[e["worst"]])
            keep = np.arange(len(members)) != e["worst"]
            members, obs = members[keep], obs[keep]
            drops += 1
            continue
        break
    res2 = np.full(C, -1.0)
    res2[members] = e["res2"]
    with np.errstate(all="ignore"):
        cov, _ = inv_sym3(e["H"])
        err = e["S"] / np.float64(2 * len(members))
    return dict(status=int(status), xyz=X, views=int(sum(1 << int(c) for c in members)), err=err, res2=res2, cov=cov, dropped=dropped,
                iters=iters, cost0=cost0, history=np.concatenate(history))


OUT_KEYS = {"xyz": (np.float64, (3,)), "err": (np.float64, ()), "res2": (np.float64, None), "cov": (np.float64, (6,)),
            "views": (np.uint32, ()), "dropped": (np.uint32, ()), "iters": (np.int32, ()), "status": (np.int32, ())}


def empty_out(T, Q, C, canary=None):
    """The call's output arrays [T][Q]..., every byte `canary` (0..255) when given, else zeros"""
    out = {}
    for k, (dt, tail) in OUT_KEYS.items():
        a = np.zeros((T, Q) + ((C,) if tail is None else tail), dt)
        if canary is not None:
            a.view(np.uint8)[...] = canary
        out[k] = a
    return out


def refine_points(xyz, n, views, K, dist, R, t, pts=None, idx=None, grp=None, distorted=0, max_iters=10, ftol=1e-9, lambda0=1e-3,
                  max_res2=0.0, min_views=2, max_drop=0, out=None):
    """The whole call.  xyz [T][Q][3], n [T], views [T][Q] (uint32 bits; None with grp = all cameras), and either pts [T][C][P][2]
    (any numeric type) with idx [T][Q][C], or grp [T][Q][C][2].  out: arrays to write into (empty_out; what the call does not
    write stays as it is), xyz may be out["xyz"] itself.  Returns out."""
    xyz = np.asarray(xyz, np.float64)
    T, Q = xyz.shape[:2]
    rig = Rig(K, dist, R, t, distorted)
    C = rig.C
    out = empty_out(T, Q, C) if out is None else out
    for s in range(T):
        rows = min(int(n[s]), Q)
        for q in range(Q):
            if q >= rows:
                out["status"][s, q] = 0
                continue
            if grp is not None:
                obs_of = lambda c: grp[s, q, c]
            else:
                P = pts.shape[2]
                obs_of = lambda c: pts[s, c, idx[s, q, c]].astype(np.float64) if 0 <= idx[s, q, c] < P else None
            mask = (1 << C) - 1 if views is None else int(np.uint32(views[s, q]))
            r = refine_row(rig, xyz[s, q], mask, obs_of, max_iters, ftol, lambda0, max_res2, min_views, max_drop)
            out["xyz"][s, q] = r["xyz"]
            out["views"][s, q] = r["views"]
            out["status"][s, q] = r["status"]
            if r["status"] > 0:
                for k in ("err", "res2", "cov", "dropped", "iters"):
                    out[k][s, q] = r[k]
    return out


def specified_equal(got, want):
    """The outputs of a call against the restatement's, floats compared as bytes: every key for a refined row and for a row that
    was not written at all (status 0: the canary must stand), xyz, views and status for an error row.  Two NaNs are equal
    whatever their sign and payload, which IEEE 754 leaves to the machine (the row of test_gpu_refine_points.py whose
    determinant overflows has inf - inf in its covariance).  Returns the list of (key, number of differing rows)."""
    bad = []
    err_rows = np.asarray(want["status"]) < 0
    for k in OUT_KEYS:
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        assert a.shape == b.shape and a.dtype.itemsize == b.dtype.itemsize, (k, a.shape, b.shape, a.dtype, b.dtype)
        rows = a.shape[0] * a.shape[1]
        differs = a.view(np.uint8).reshape(rows, -1, a.dtype.itemsize) != b.view(np.uint8).reshape(rows, -1, a.dtype.itemsize)
        if a.dtype == np.float64:
            differs &= ~(np.isnan(a) & np.isnan(b)).reshape(rows, -1, 1)
        diff = differs.any(axis=(1, 2))
        if k not in ("xyz", "views", "status"):
            diff &= ~err_rows.reshape(-1)
        if diff.any():
            bad.append((k, int(diff.sum())))
    return bad
