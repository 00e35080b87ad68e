"""NumPy restatement of the rig bundle adjustment that also refines every camera's lens, built on
tests/rig_ba_ref.py, tests/rig_robust_ref.py and tests/lm_ref.py without a change to any of them, and the seeded cases the
tests share.  Not a test module: the yardstick of tests/test_rig_selfcal_host.py, tests/test_gpu_rig_selfcal.py and
tests/test_gpu_rig_selfcal_shapes.py.

Definition.  The problem of rig_robust_ref (point-major observations, partial visibility, camera 0 the world frame, loss none
or Cauchy) with nine more unknowns per camera, camera 0 included: kd = (fx, fy, cx, cy, k1, k2, p1, p2, k3).  A camera's block
is 15 wide, the 9 lens columns of tests/intrinsics_ref.py first, then the 6 of lm_ref.pose_columns.  masks [C]: bit i of
masks[c] frees lens parameter i of camera c; the pose columns of cameras 1.. are free, camera 0's are fixed.  A fixed
parameter's Jacobian column is zero; its diagonal entry of the damped reduced matrix is 1 (its row, column and right-hand side
are zero), so its step is exactly 0.  A camera with a mask other than 0 and fewer observations than twice its free lens
parameters fails the layout check.  Normal equations in blocks U_c (15x15), V_n (3x3), W_nc (15x3); Marquardt damping, the
Schur complement on the points, Cholesky of the (15 C) square S, back-substitution; lm_ref.control; on return every t and X
is scaled so that |t_1| is what it was at the start.  With a loss an observation's r and its rows of both Jacobians are
scaled by sqrt(w) and the costs sum rho, as rig_robust_ref does.

Every per-observation quantity is formed by the same operations in the same order as csrc/rig_selfcal.hip and csrc/lm.h; the
kernels differ from this file in the ORDER of the sums over observations and points (and in the Cholesky's) only;
`order_spread` measures what that order is worth."""
import numpy as np

import lm_ref
import rig_ba_ref as rb
import rig_robust_ref as rr
from lm_ref import STOP_MAX_ITERS, STOP_FTOL, STOP_LAMBDA, STOP_CHOLESKY  # noqa: F401 (the tests read them from here)

P = 15  # a camera block: 9 lens parameters, 6 pose parameters
MASKS = {"focal": 0x003, "focal+center": 0x00F, "focal+center+radial2": 0x03F, "all": 0x1FF}


def kd_of(prob):
    """[C][9] from the problem's K and dist"""
    return np.c_[prob.K[:, 0, 0], prob.K[:, 1, 1], prob.K[:, 0, 2], prob.K[:, 1, 2], prob.dist[:, :5]]


def free_columns(masks, C):
    """[C][15] bool: the free parameters of every camera block"""
    masks = np.broadcast_to(np.asarray(masks, np.int64), (C,))
    free = np.zeros((C, P), bool)
    for i in range(9):
        free[:, i] = (masks >> i) & 1
    free[1:, 9:] = True
    return free


def layout_ok(prob, masks):
    """Every camera with a mask other than 0 has at least twice as many observations as free lens parameters"""
    masks = np.broadcast_to(np.asarray(masks, np.int64), (prob.C,))
    count = np.bincount(prob.cam, minlength=prob.C)
    n_free = np.array([bin(int(m)).count("1") for m in masks])
    return bool(((masks == 0) | (count >= 2 * n_free)).all())


def observe(prob, kd, R, t, X, free, loss_c=None):
    """Per observation: residual r [n_obs][2], camera Jacobian jc [n_obs][2][15] (fixed columns zero), point Jacobian jp
    [n_obs][2][3], front [n_obs], s [n_obs] (the unscaled |r|^2).  With loss_c, r, jc and jp are scaled by sqrt(w)."""
    c, n = prob.cam, prob.pt
    Rm, tm, Xm = R[c], t[c], X[n]
    q = [(Rm[:, i, 0] * Xm[:, 0] + Rm[:, i, 1] * Xm[:, 1]) + Rm[:, i, 2] * Xm[:, 2] for i in range(3)]
    lens = [kd[c, i] for i in range(9)]
    fx, fy = lens[0], lens[1]
    with np.errstate(all="ignore"):
        r, front, A, m = lm_ref.project(lens, q, [tm[:, 0], tm[:, 1], tm[:, 2]], prob.uv)
        x, y, xy, r2, r4, r6 = m["x"], m["y"], m["xy"], m["r2"], m["r4"], m["r6"]
        jc = np.zeros((len(c), 2, P))
        jc[:, 0, 0], jc[:, 0, 2] = m["xd"], 1.0
        jc[:, 1, 1], jc[:, 1, 3] = m["yd"], 1.0
        jc[:, 0, 4], jc[:, 0, 5], jc[:, 0, 6], jc[:, 0, 7], jc[:, 0, 8] = fx * (x * r2), fx * (x * r4), fx * (2.0 * xy), fx * m["tx"], fx * (x * r6)
        jc[:, 1, 4], jc[:, 1, 5], jc[:, 1, 6], jc[:, 1, 7], jc[:, 1, 8] = fy * (y * r2), fy * (y * r4), fy * m["ty"], fy * (2.0 * xy), fy * (y * r6)
        jp = np.empty((len(c), 2, 3))
        for i in range(2):
            for j in range(3):
                jp[:, i, j] = (A[i][0] * Rm[:, 0, j] + A[i][1] * Rm[:, 1, j]) + A[i][2] * Rm[:, 2, j]
            jc[:, i, 9:] = np.stack(lm_ref.pose_columns(A[i], q), 1)
        jc = np.where(free[c][:, None, :], jc, 0.0)
        s = r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]
        if loss_c is not None:
            sw = np.sqrt(rr.weights(r, loss_c)[1])
            r, jc, jp = r * sw[:, None], jc * sw[:, None, None], jp * sw[:, None, None]
    return r, jc, jp, front, s


def cost_of(prob, kd, R, t, X, loss_c=None):
    """(1/2 sum r^2, or 1/2 sum rho with a loss; every observed point in front of its camera)"""
    _, _, _, front, s = observe(prob, kd, R, t, X, np.zeros((prob.C, P), bool))
    return 0.5 * float(np.sum(s if loss_c is None else rr.rho(s, loss_c))), bool(front.all())


def residual_vector(prob, kd, R, t, X):
    """The unscaled residuals [2 n_obs], for finite differences"""
    return observe(prob, kd, R, t, X, np.zeros((prob.C, P), bool))[0].reshape(-1)


def linearize(prob, kd, R, t, X, lam, masks, loss_c=None):
    """The pieces of one iteration: dict with cost, front, gc [15 C], gp [N][3], U [C][15][15], V [N][3][3], W [n_obs][15][3],
    Vinv (damped), S [15 C][15 C] (damped, fixed diagonal entries 1), rhs [15 C], gradient [15 C + 3 N], free [C][15]."""
    C, N, D = prob.C, prob.N, P * prob.C
    free = free_columns(masks, C)
    r, jc, jp, front, s = observe(prob, kd, R, t, X, free, loss_c)
    cost = 0.5 * float(np.sum(s if loss_c is None else rr.rho(s, loss_c)))
    Uo = jc[:, 0, :, None] * jc[:, 0, None, :] + jc[:, 1, :, None] * jc[:, 1, None, :]
    gco = jc[:, 0, :] * r[:, 0, None] + jc[:, 1, :] * r[:, 1, None]
    Vo = jp[:, 0, :, None] * jp[:, 0, None, :] + jp[:, 1, :, None] * jp[:, 1, None, :]
    gpo = jp[:, 0, :] * r[:, 0, None] + jp[:, 1, :] * r[:, 1, None]
    W = jc[:, 0, :, None] * jp[:, 0, None, :] + jc[:, 1, :, None] * jp[:, 1, None, :]
    U, gc = np.zeros((C, P, P)), np.zeros((C, P))
    np.add.at(U, prob.cam, Uo)
    np.add.at(gc, prob.cam, gco)
    V, gp = np.zeros((N, 3, 3)), np.zeros((N, 3))
    np.add.at(V, prob.pt, Vo)
    np.add.at(gp, prob.pt, gpo)
    Vd = V.copy()
    for i in range(3):
        Vd[:, i, i] = V[:, i, i] + lam * V[:, i, i]
    Vinv = rb._inv_sym3(Vd)
    Vi = Vinv[prob.pt]
    Y = np.empty_like(W)
    for j in range(3):
        Y[:, :, j] = (W[:, :, 0] * Vi[:, 0, j, None] + W[:, :, 1] * Vi[:, 1, j, None]) + W[:, :, 2] * Vi[:, 2, j, None]
    # the blocks W_a V*^-1 W_b^T over all pairs of observations of one point, camera a <= camera b (a point's own pairs too)
    Sb = np.zeros((C, C, P, P))
    order = np.argsort(prob.pt, kind="stable")
    pts_sorted = prob.pt[order]
    starts = np.flatnonzero(np.r_[True, pts_sorted[1:] != pts_sorted[:-1]])
    counts = np.diff(np.r_[starts, len(order)])
    ia, ib = [], []
    for k in range(1, int(counts.max()) + 1):
        for i in range(k):
            sel = starts[counts >= k]
            ia.append(order[sel + i])
            ib.append(order[sel + k - 1])
    ia, ib = np.concatenate(ia), np.concatenate(ib)
    swap = prob.cam[ia] > prob.cam[ib]
    ia, ib = np.where(swap, ib, ia), np.where(swap, ia, ib)
    blk = np.empty((len(ia), P, P))
    Ya, Wb = Y[ia], W[ib]
    for j in range(P):
        blk[:, :, j] = (Ya[:, :, 0] * Wb[:, j, 0, None] + Ya[:, :, 1] * Wb[:, j, 1, None]) + Ya[:, :, 2] * Wb[:, j, 2, None]
    np.add.at(Sb, (prob.cam[ia], prob.cam[ib]), blk)
    gpn = gp[prob.pt]
    yg = (Y[:, :, 0] * gpn[:, 0, None] + Y[:, :, 1] * gpn[:, 1, None]) + Y[:, :, 2] * gpn[:, 2, None]
    red = np.zeros((C, P))
    np.add.at(red, prob.cam, yg)
    gc = gc.reshape(-1)
    rhs = red.reshape(-1) - gc
    S = np.zeros((D, D))
    for a in range(C):
        for b in range(a, C):
            if a == b:
                Ud = U[a].copy()
                for i in range(P):
                    Ud[i, i] = U[a][i, i] + lam * U[a][i, i]
                blkab = Ud - Sb[a, a]
                blkab = np.triu(blkab) + np.triu(blkab, 1).T
                for i in np.flatnonzero(~free[a]):
                    blkab[i, i] = 1.0
                S[P * a:P * a + P, P * a:P * a + P] = blkab
            else:
                S[P * a:P * a + P, P * b:P * b + P] = 0.0 - Sb[a, b]
                S[P * b:P * b + P, P * a:P * a + P] = (0.0 - Sb[a, b]).T
    return {"cost": cost, "front": bool(front.all()), "gc": gc, "gp": gp, "U": U, "V": V, "W": W, "Vinv": Vinv, "S": S, "rhs": rhs,
            "gradient": np.r_[gc, gp.reshape(-1)], "r": r, "jc": jc, "jp": jp, "free": free}


def schur_step(prob, lin, lam):
    """(dc [15 C], dp [N][3], predicted reduction) from the pieces, or None when S is not positive definite"""
    try:
        L = np.linalg.cholesky(lin["S"])
    except np.linalg.LinAlgError:
        return None
    if not np.isfinite(L).all():
        return None
    dc = np.linalg.solve(L.T, np.linalg.solve(L, lin["rhs"]))
    dc[~lin["free"].reshape(-1)] = 0.0  # (they are zeros already: rows of the identity against a zero right-hand side)
    wt = np.einsum("oij,oi->oj", lin["W"], dc.reshape(-1, P)[prob.cam])
    q = lin["gp"].copy()
    np.add.at(q, prob.pt, wt)
    dp = -np.einsum("nij,nj->ni", lin["Vinv"], q)
    ud = np.array([lin["U"][a][i, i] for a in range(prob.C) for i in range(P)])
    vd = np.stack([lin["V"][:, i, i] for i in range(3)], 1)
    pred = 0.5 * (float(np.sum(dc * ((lam * ud) * dc - lin["gc"]))) + float(np.sum(dp * ((lam * vd) * dp - lin["gp"]))))
    return dc, dp, pred


def dense_step(prob, lin, lam):
    """The same step from the full damped normal equations over the free parameters (the check of the Schur elimination)"""
    D, N = P * prob.C, prob.N
    H = np.zeros((D + 3 * N, D + 3 * N))
    for a in range(prob.C):
        H[P * a:P * a + P, P * a:P * a + P] = lin["U"][a]
    for n in range(N):
        H[D + 3 * n:D + 3 * n + 3, D + 3 * n:D + 3 * n + 3] = lin["V"][n]
    for o in range(len(prob.pt)):
        a, n = prob.cam[o], prob.pt[o]
        H[P * a:P * a + P, D + 3 * n:D + 3 * n + 3] += lin["W"][o]
        H[D + 3 * n:D + 3 * n + 3, P * a:P * a + P] += lin["W"][o].T
    H[np.diag_indices_from(H)] += lam * np.diag(H)
    keep = np.r_[lin["free"].reshape(-1), np.ones(3 * N, bool)]
    d = np.zeros(D + 3 * N)
    d[keep] = np.linalg.solve(H[np.ix_(keep, keep)], -lin["gradient"][keep])
    return d[:D], d[D:].reshape(N, 3)


def apply_step(prob, kd, R, t, X, dc, dp):
    d = dc.reshape(-1, P)
    R2, t2 = R.copy(), t.copy()
    for c in range(1, prob.C):
        R2[c] = rb.exp_so3(d[c, 9:12]) @ R[c]
        t2[c] = t[c] + d[c, 12:]
    return kd + d[:, :9], R2, t2, X + dp


def lm(prob, kd, R, t, X, masks, loss_c=None, max_iters=50, ftol=1e-12, lambda0=1e-3):
    """The loop.  dict: kd, R, t, X (gauge restored), status, iterations, cost_initial, cost, history [iterations][4], rho
    [iterations], as rig_ba_ref.lm's.  Raises ValueError for a layout the check refuses and for a start with a point behind."""
    kd, R, t, X = np.array(kd, float).reshape(-1, 9), np.array(R, float), np.array(t, float).reshape(-1, 3), np.array(X, float)
    if not layout_ok(prob, masks):
        raise ValueError("a camera has fewer observations than twice its free lens parameters")
    R[0], t[0] = np.eye(3), 0.0
    t1_norm = float(np.sqrt((t[1, 0] * t[1, 0] + t[1, 1] * t[1, 1]) + t[1, 2] * t[1, 2]))
    cost0, front = cost_of(prob, kd, R, t, X, loss_c)
    if not front or not np.isfinite(cost0):
        raise ValueError("the state handed in has a point behind a camera that sees it")

    def try_step(state, lam):
        lin = linearize(prob, *state, lam, masks, loss_c)
        step = schur_step(prob, lin, lam)
        if step is None:
            return None
        dc, dp, pred = step
        trial = apply_step(prob, *state, dc, dp)
        return (trial, *cost_of(prob, *trial, loss_c), pred, float(np.sqrt(np.sum(dp * dp) + np.sum(dc * dc))))

    (kd, R, t, X), cost, status, history, rho = lm_ref.control((kd, R, t, X), cost0, try_step, max_iters, ftol, lambda0)
    R, t, X = rb.rescale(R, t, X, t1_norm)
    return {"kd": kd, "R": R, "t": t, "X": X, "status": status, "iterations": len(history), "cost_initial": cost0, "cost": cost,
            "history": history, "rho": rho}


def rms_px(prob, cost):
    """rms reprojection residual per coordinate of a cost 1/2 sum r^2"""
    return float(np.sqrt(cost / len(prob.pt)))


def order_spread(prob, kd, R, t, X, lam, masks, loss_c=None, n_perm=10, base=None):
    """rig_ba_ref.order_spread for these pieces: largest difference of cost, gradient, S and rhs between the sorted problem and
    n_perm seeded permutations of its observations, each relative to the quantity's largest entry: dict name -> spread.
    base: the sorted problem's pieces, where the caller has them already."""
    if base is None:
        base = linearize(prob.sorted(), kd, R, t, X, lam, masks, loss_c)
    out = {k: 0.0 for k in ("cost", "gradient", "S", "rhs")}
    for s in range(n_perm):
        lin = linearize(rb.permuted(prob, 1000 + s), kd, R, t, X, lam, masks, loss_c)
        for k in out:
            a, b = np.asarray(base[k], float), np.asarray(lin[k], float)
            out[k] = max(out[k], float(np.abs(a - b).max() / np.abs(a).max()))
    return out


# ---- the cases ---------------------------------------------------------------------------------------------------------------
def lens_case(n_cam, n_points, seed, sigma, dropout=0.3, width=1920, height=1080, extent=0.8, central=0):
    """Seeded ring of n_cam cameras (synth.MixedScene) whose true K and lens differ per camera by seeded draws around
    synth.intrinsics and synth.MILD_DIST: from default_rng(seed), in this order, per camera f (+-2 %, fy = fx (1 +- 0.5 %)),
    the principal point (+-20 px), k1 (+-0.02), k2 (+-0.01), p1, p2 (+-1e-3); then rig_ba_ref._rig_case's draws (points,
    dropout, noise) from default_rng(seed + 1).  central: after the draws the first `central` points are pulled to a tenth of
    their distance from the origin and lose no view to the dropout, so that every camera sees them.
    Returns dict: scene, X, prob (true intrinsics), kd_true [C][9], sigma."""
    from mocapv2_amd import synth
    rng = np.random.default_rng(seed)
    K0 = synth.intrinsics(width, height)
    Ks, dists = [], []
    for _ in range(n_cam):
        fx = K0[0, 0] * (1 + rng.uniform(-0.02, 0.02))
        fy = fx * (1 + rng.uniform(-0.005, 0.005))
        cx, cy = K0[0, 2] + rng.uniform(-20, 20), K0[1, 2] + rng.uniform(-20, 20)
        Ks.append(np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1.0]]))
        dists.append(np.array(synth.MILD_DIST) + np.r_[rng.uniform(-0.02, 0.02), rng.uniform(-0.01, 0.01), rng.uniform(-1e-3, 1e-3, 2), 0.0])
    scene = synth.MixedScene(n_cam, width, height, Ks=Ks, dists=dists)
    rng = np.random.default_rng(seed + 1)
    X = rng.uniform(-extent, extent, size=(n_points, 3))
    drop = rng.uniform(0, 1, (n_points, n_cam)) < dropout
    noise = rng.normal(0, 1.0, (n_points, n_cam, 2)) * sigma
    X[:central] *= 0.1
    drop[:central] = False
    px = np.stack([scene.pixels(X, c) for c in range(n_cam)], 1) + noise
    z = np.stack([(X @ np.asarray(p["R"]).T + np.asarray(p["t"]).reshape(3))[:, 2] for p in scene.poses], 1)
    seen = (px[..., 0] >= 0) & (px[..., 0] < width) & (px[..., 1] >= 0) & (px[..., 1] < height) & (z > 0) & ~drop
    keep = seen.sum(1) >= 2
    X, px, seen = X[keep], px[keep], seen[keep]
    prob = rb.problem_from_arrays(np.transpose(px, (1, 0, 2)), seen.T, scene.camera_params)
    return {"scene": scene, "X": X, "prob": prob, "kd_true": kd_of(prob), "sigma": sigma}


def checkerboard_start(kd_true, seed, f=3e-3, center=3.0, radial=5e-3):
    """Intrinsics of checkerboard grade around the truth: from default_rng(seed) a sign per camera and parameter; fx and fy off
    by the fraction f (the same sign for both), cx and cy by `center` px, k1 and k2 by `radial`; p1, p2, k3 as they are"""
    sign = np.random.default_rng(seed).choice([-1.0, 1.0], size=(len(kd_true), 5))
    kd = np.array(kd_true, float)
    kd[:, 0] *= 1 + f * sign[:, 0]
    kd[:, 1] *= 1 + f * sign[:, 0]
    kd[:, 2] += center * sign[:, 1]
    kd[:, 3] += center * sign[:, 2]
    kd[:, 4] += radial * sign[:, 3]
    kd[:, 5] += radial * sign[:, 4]
    return kd


def small_case(n_cam, seed=31, n_points=60, views=None, central=0):
    """The rigs of the GPU tests: lens_case at sigma 0.3 (60 points drawn unless told otherwise) and a start moved off the truth
    (rig_ba_ref.perturbed_start's steps; the intrinsics by checkerboard_start).  views: no view is hidden, and point n keeps
    that many observations: of the cameras that see it, the first counted round the ring from camera n % C.
    Returns (prob, kd_true, kd_start, R, t, X)."""
    c = lens_case(n_cam, n_points, seed, 0.3, dropout=0.0 if views else 0.3, central=central)
    prob = c["prob"].sorted()
    if views:
        keep = np.zeros(len(prob.pt), bool)
        for n in range(prob.N):
            o = np.flatnonzero(prob.pt == n)
            first = np.argsort((prob.cam[o] - n) % n_cam)[:views]  # the cameras that follow n % C round the ring
            keep[o[first]] = True
        points = np.flatnonzero(np.bincount(prob.pt[keep], minlength=prob.N) >= 2)
        keep &= np.isin(prob.pt, points)
        prob = rb.Problem(np.searchsorted(points, prob.pt[keep]), prob.cam[keep], prob.uv[keep], prob.K, prob.dist, len(points)).sorted()
        c = {**c, "X": c["X"][points]}
    R, t, X = rb.perturbed_start(c, seed + 7, rot=0.003, trans=0.005, point=0.005)
    return prob, c["kd_true"], checkerboard_start(c["kd_true"], seed + 9), R, t, X


# The rigs of tests/test_gpu_rig_selfcal.py: name -> (cameras, views kept per point or None, masks, loss scale or None).  One
# camera at mask 0 and one at 0x1FF in the mixed ones; wide7 has 105 rows, more than the Cholesky holds in LDS.
LOOP_CASES = {
    "mixed3": (3, None, [0, 0x1FF, 0x03F], None),
    "mixed3_cauchy": (3, None, [0, 0x1FF, 0x03F], 2.0),
    "mixed4": (4, None, [0, 0x1FF, 0x03F, 0x003], None),
    "mixed4_cauchy": (4, None, [0, 0x1FF, 0x03F, 0x003], 2.0),
    "wide7": (7, 3, [0x003] * 7, None),
}
# ftol of the loop comparison: with it every case stops on a step whose relative decrease is a factor 1.2 or more away from
# ftol, as is every step before it (tests/test_rig_selfcal_host.py asserts it): the rounding of the cost decides nothing
LOOP_FTOL = 2e-8

_loop_cases = {}


def loop_case(name):
    """(prob, kd_start, R, t, X, masks, loss scale, the restatement's loop at LOOP_FTOL from there), computed once"""
    if name not in _loop_cases:
        n_cam, views, masks, loss_c = LOOP_CASES[name]
        prob, _, kd, R, t, X = small_case(n_cam, views=views)
        masks = np.array(masks)
        _loop_cases[name] = (prob, kd, R, t, X, masks, loss_c, lm(prob, kd, R, t, X, masks, loss_c, ftol=LOOP_FTOL))
    return _loop_cases[name]


def first_points(prob, X, n):
    """(the problem of the first n points, renumbered and sorted, their start X [n][3]): sets N exactly"""
    keep = prob.pt < n
    points = np.unique(prob.pt[keep])
    assert len(points) == n
    return rb.Problem(np.searchsorted(points, prob.pt[keep]), prob.cam[keep], prob.uv[keep], prob.K, prob.dist, n).sorted(), X[points]


# The rigs of tests/test_gpu_rig_selfcal_shapes.py, each named for the shape it reaches: name -> (cameras, points drawn, points
# kept or None, points pulled to the centre, masks, loss scale or None, walks the loop).  PT_THREADS = SCHUR_CHUNK = 256 points
# make a workgroup, 90 rows is the most the Cholesky holds in LDS, 32 cameras (480 rows, 528 pairs) the most a rig may have.
_MIXED6 = [0, 0x1FF, 0x03F, 0x003, 0x1FF, 0x00F]
SHAPE_CASES = {
    "two": (2, 600, None, 0, [0, 0x003], None, True),
    "six_lds": (6, 60, None, 0, _MIXED6, None, True),
    "six_600": (6, 600, None, 0, _MIXED6, None, True),
    "six_600_cauchy": (6, 600, None, 0, _MIXED6, 2.0, True),
    "blocks_255": (4, 600, 255, 0, LOOP_CASES["mixed4"][2], None, True),
    "blocks_256": (4, 600, 256, 0, LOOP_CASES["mixed4"][2], None, True),
    "blocks_257": (4, 600, 257, 0, LOOP_CASES["mixed4"][2], None, True),
    "blocks_513": (4, 600, 513, 0, LOOP_CASES["mixed4"][2], None, True),
    "rig32": (32, 140, None, 4, [0x03F] * 32, None, True),
    "rig32_cauchy": (32, 140, None, 4, [0x03F] * 32, 2.0, True),
    "chunk_growth": (2, 140000, 65537, 0, [0, 0x003], None, False),  # 3 s a linearisation here: pieces only
}
SHAPE_LOOPS = [k for k, v in SHAPE_CASES.items() if v[6]]


def lin_blocks(N):
    """Workgroups of the point-owning kernels (selfcal_lin_blocks)"""
    return -(-N // 256)


def schur_chunks(N):
    """(points per workgroup of the Schur kernel, workgroups): 256 points, or what leaves 256 workgroups (selfcal_schur_chunk)"""
    chunk = max(256, -(-N // 256))
    return chunk, -(-N // chunk)


_shape_cases = {}


def shape_case(name):
    """loop_case for SHAPE_CASES; the loop is None for a case that does not walk it"""
    if name not in _shape_cases:
        n_cam, n_points, n_keep, central, masks, loss_c, loop = SHAPE_CASES[name]
        prob, _, kd, R, t, X = small_case(n_cam, n_points=n_points, central=central)
        if n_keep:
            prob, X = first_points(prob, X, n_keep)
        # the gauge of the definition, which the device imposes on the state it is handed and `lm` on its own: perturbed_start
        # leaves camera 0 a few 1e-16 off the world frame, and `linearize` would take that as it comes
        R[0], t[0] = np.eye(3), 0.0
        masks = np.array(masks)
        _shape_cases[name] = (prob, kd, R, t, X, masks, loss_c, lm(prob, kd, R, t, X, masks, loss_c, ftol=LOOP_FTOL) if loop else None)
    return _shape_cases[name]
