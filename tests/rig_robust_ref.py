"""NumPy restatement of the rig bundle adjustment under the Cauchy loss, built on tests/rig_ba_ref.py and
tests/lm_ref.py without a change to either, and the seeded outliers the tests share.  Not a test module: the yardstick of
tests/test_rig_robust_host.py and tests/test_gpu_rig_robust.py.

Definition.  Per observation with residual r = (rx, ry): s = rx rx + ry ry; scale c > 0 in pixels; loss rho(s) = c^2 log1p(s /
c^2); weight w = 1 / (1 + s / c^2); cost 1/2 sum rho.  First-order reweighting: r and the rows of jc and jp of the observation
are each multiplied by sqrt(w), and U, V, W, g, the Schur complement and the predicted reduction are rig_ba_ref's, formed from
the scaled quantities.  The trial cost is 1/2 sum rho of the trial state; the step control is lm_ref.control, unchanged.
s, w and the products are formed as csrc/lm.h and csrc/rig_ba.hip form them."""
import contextlib

import numpy as np

import lm_ref
import rig_ba_ref as rb

_plain_observe = rb.observe


def weights(r, c):
    """(s [n_obs], w [n_obs]) of residuals r [n_obs][2]"""
    c2 = c * c
    s = r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]
    with np.errstate(all="ignore"):
        return s, 1.0 / (1.0 + s / c2)


def rho(s, c):
    c2 = c * c
    with np.errstate(all="ignore"):
        return c2 * np.log1p(s / c2)


def observe(prob, R, t, X, c):
    """rig_ba_ref.observe with r, jc, jp scaled by sqrt(w); also s and w of the unscaled residual"""
    r, jc, jp, front = _plain_observe(prob, R, t, X)
    s, w = weights(r, c)
    sw = np.sqrt(w)
    return r * sw[:, None], jc * sw[:, None, None], jp * sw[:, None, None], front, s, w


def cost_of(prob, R, t, X, c):
    """(1/2 sum rho, every observed point in front of its camera)"""
    r, _, _, front = _plain_observe(prob, R, t, X)
    return 0.5 * float(np.sum(rho(weights(r, c)[0], c))), bool(front.all())


def errors_and_weights(prob, R, t, X, c):
    """(|r| [n_obs], w [n_obs]) of the unweighted residuals at a state: what the GPU reports per observation"""
    s, w = weights(_plain_observe(prob, R, t, X)[0], c)
    return np.sqrt(s), w


@contextlib.contextmanager
def _weighted(c):
    """rig_ba_ref's assembly reads its observations through rig_ba_ref.observe: inside this block that is the scaled one"""
    rb.observe = lambda prob, R, t, X: observe(prob, R, t, X, c)[:4]
    try:
        yield
    finally:
        rb.observe = _plain_observe


def linearize(prob, R, t, X, lam, c):
    """rig_ba_ref.linearize over the scaled observations; cost is 1/2 sum rho"""
    with _weighted(c):
        lin = rb.linearize(prob, R, t, X, lam)
    lin["cost"] = cost_of(prob, R, t, X, c)[0]
    return lin


def lm(prob, R, t, X, c, max_iters=50, ftol=1e-12, lambda0=1e-3, trace=None):
    """The loop of rig_ba_ref.lm under the loss; the dict of rig_ba_ref.lm plus err, w [n_obs] at the returned state.  trace: as
    rig_ba_ref.lm's"""
    R, t, X = np.array(R, float), np.array(t, float).reshape(-1, 3), np.array(X, float)
    R[0], t[0] = np.eye(3), 0.0
    t1_norm = float(np.sqrt((t[1, 0] * t[1, 0] + t[1, 1] * t[1, 1]) + t[1, 2] * t[1, 2]))
    cost0, front = cost_of(prob, R, t, X, c)
    if not front or not np.isfinite(cost0):
        raise ValueError("the state handed in has a point behind a camera that sees it")

    def try_step(state, lam):
        lin = linearize(prob, *state, lam, c)
        step = rb.schur_step(prob, lin, lam)
        if trace is not None:
            trace.append({"S": lin["S"], "trial": None})
        if step is None:
            return None
        dc, dp, pred = step
        trial_state = rb.apply_step(prob, *state, dc, dp)
        if trace is not None:
            trace[-1]["trial"] = trial_state
        return (trial_state, *cost_of(prob, *trial_state, c), pred, float(np.sqrt(np.sum(dp * dp) + np.sum(dc * dc))))

    (R, t, X), cost, status, history, rhos = lm_ref.control((R, t, X), cost0, try_step, max_iters, ftol, lambda0)
    R, t, X = rb.rescale(R, t, X, t1_norm)
    err, w = errors_and_weights(prob, R, t, X, c)
    return {"R": R, "t": t, "X": X, "status": status, "iterations": len(history), "cost_initial": cost0, "cost": cost,
            "history": history, "rho": rhos, "err": err, "w": w}


def order_spread(prob, R, t, X, lam, c, n_perm=10):
    """rig_ba_ref.order_spread for the robust pieces: largest difference of cost, gradient, S and rhs between the sorted problem
    and n_perm seeded permutations of its observations, each relative to the quantity's largest entry"""
    base = linearize(prob.sorted(), R, t, X, lam, c)
    out = {k: 0.0 for k in ("cost", "gradient", "S", "rhs")}
    for s in range(n_perm):
        lin = linearize(rb.permuted(prob, 1000 + s), R, t, X, lam, c)
        for k in out:
            a, b = np.asarray(base[k], float), np.asarray(lin[k], float)
            out[k] = max(out[k], float(np.abs(a - b).max() / np.abs(a).max()))
    return out


def dirty(case, frac=0.05, seed=7):
    """The case with a fraction of its observations moved by 20 to 80 px.  Of case["prob"].sorted(), the observations of points
    with at least 3 views are eligible; from default_rng(seed), in this order: choice(eligible, max(1, int(frac n_obs)),
    replace=False), angles uniform(0, 2 pi), lengths uniform(20, 80); the offsets length (cos, sin) are added to the chosen.
    Returns the case's dict with prob (sorted, dirty), image_points and valid replaced, plus planted_obs (indices into prob),
    planted [C][N] bool and clean_prob (sorted, as it was)."""
    clean = case["prob"].sorted()
    n_obs = len(clean.pt)
    eligible = np.flatnonzero(np.bincount(clean.pt, minlength=clean.N)[clean.pt] >= 3)
    rng = np.random.default_rng(seed)
    k = max(1, int(frac * n_obs))
    chosen = rng.choice(eligible, k, replace=False)
    angle = rng.uniform(0, 2 * np.pi, k)
    length = rng.uniform(20, 80, k)
    uv = clean.uv.copy()
    uv[chosen] += np.stack([length * np.cos(angle), length * np.sin(angle)], 1)
    prob = rb.Problem(clean.pt, clean.cam, uv, clean.K, clean.dist, clean.N)
    ip = np.array(case["image_points"], float)
    ip[prob.cam, prob.pt] = uv
    planted = np.zeros(case["valid"].shape, bool)
    planted[prob.cam[chosen], prob.pt[chosen]] = True
    return {**case, "prob": prob, "clean_prob": clean, "image_points": ip, "planted_obs": np.sort(chosen), "planted": planted}


def without(prob, obs):
    """(the problem with the observations `obs` (indices) removed, the points it keeps [N'] as indices into prob's): a point
    left with fewer than two views leaves the problem, as it leaves `used` in calibrate.bundle_adjust_rig, and the rest are
    renumbered in order"""
    keep = np.ones(len(prob.pt), bool)
    keep[obs] = False
    points = np.flatnonzero(np.bincount(prob.pt[keep], minlength=prob.N) >= 2)
    keep &= np.isin(prob.pt, points)
    return rb.Problem(np.searchsorted(points, prob.pt[keep]), prob.cam[keep], prob.uv[keep], prob.K, prob.dist, len(points)), points


def flags(w, inlier_weight=0.25):
    return np.asarray(w) < inlier_weight
