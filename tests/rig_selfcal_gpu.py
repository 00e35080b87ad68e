"""What tests/test_gpu_rig_selfcal.py and tests/test_gpu_rig_selfcal_shapes.py share: the call helpers, and the comparisons of
the device's pieces and of its loop with the NumPy restatement tests/rig_selfcal_ref.py.  Not a test module; the reasoning
behind every bound is in the docstrings of the tests that call these."""
import ctypes as C

import numpy as np

import rig_selfcal_ref as sc

U = float(np.finfo(float).eps) / 2  # unit roundoff of FP64, 1.1e-16
P = sc.P
PIECES = ("cost", "gradient", "S", "rhs")


def poses12(R, t):
    return np.c_[np.asarray(R, float).reshape(len(R), 9), np.asarray(t, float).reshape(len(R), 3)]


def gpu_args(prob, R, t, X):
    return (*prob.point_major(), poses12(R, t), X)


def loss_args(loss_c):
    return {} if loss_c is None else {"loss": "cauchy", "loss_scale": loss_c}


def adjust(ctx, prob, kd, R, t, X, masks, loss_c=None, **kw):
    return ctx.rig_bundle_adjust_intrinsics(*prob.point_major(), kd, masks, poses12(R, t), X, **loss_args(loss_c), **kw)


def linearize(ctx, prob, kd, R, t, X, masks, loss_c=None, lam=1e-3):
    return ctx.rig_linearize_intrinsics(*prob.point_major(), kd, masks, poses12(R, t), X, lam, **loss_args(loss_c))


def rot_err(Ra, Rb):
    return float(np.linalg.norm(Ra @ Rb.T - np.eye(3)) / np.sqrt(2))  # = 2 sin(angle / 2), about the angle in radians


def adjust_raw(ctx, off, cam, uv, kd, masks, poses, X, C_, N, max_iters=10):
    """mocap_rig_bundle_adjust_intrinsics through the C-ABI, where the arrays can be looked at after a negative status:
    (return code, result [4], kd, poses, points, history as the device holds them afterwards)"""
    import torch
    from mocapv2_amd.engine import _ptr, _stream
    dev = ctx.device
    d = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in
         (("off", off), ("cam", cam), ("uv", uv), ("kd", kd), ("poses", poses), ("pts", X))}
    hist = torch.zeros((max_iters, 4), dtype=torch.float64, device=dev)
    result = torch.zeros((4,), dtype=torch.float64, device=dev)
    mask = np.ascontiguousarray(masks, np.int32)
    rc = ctx.lib.mocap_rig_bundle_adjust_intrinsics(ctx._h, C_, N, len(cam), _ptr(d["off"]), _ptr(d["cam"]), _ptr(d["uv"]), _ptr(d["kd"]),
                                                    mask.ctypes.data_as(C.POINTER(C.c_int)), _ptr(d["poses"]), _ptr(d["pts"]), max_iters, 1e-12,
                                                    1e-3, _ptr(hist), _ptr(result), 0, 0.0, None, None, _stream())
    ctx.sync()
    return rc, result.cpu().numpy(), d["kd"].cpu().numpy(), d["poses"].cpu().numpy(), d["pts"].cpu().numpy(), hist.cpu().numpy()


def damping_allowance(ref):
    """What the loop test's allowance on the costs, 1e-8 of each, leaves of the damping's agreement, per iteration, from the
    restatement's own history.  An accepted step multiplies lambda by mu = max(1/3, 1 - (2 rho - 1)^3) with rho = (cost - trial)
    / predicted.  Two costs known to 1e-8 of themselves leave their difference known to 2e-8 / rel of itself, rel the step's
    relative decrease -- near the stop, where rel is about ftol, rho is hardly known at all; the predicted reduction comes
    from the step, 1e-6.  d mu / d rho = 6 (2 rho - 1)^2 above the floor of 1/3, 0 on it; a rejected step multiplies by nu
    exactly.  The errors of the factors add up along the loop: entry k is the allowance on the lambda iteration k was solved
    with."""
    h, rho = ref["history"], ref["rho"]
    before = np.r_[ref["cost_initial"], h[:-1, 0]]
    with np.errstate(all="ignore"):
        rel = (before - h[:, 0]) / before
        mu = 1.0 - (2.0 * rho - 1.0) ** 3
        factor = np.where((h[:, 2] > 0) & (mu > 1.0 / 3.0), 6.0 * (2.0 * rho - 1.0) ** 2 * np.abs(rho) / mu * (2e-8 / rel + 1e-6), 0.0)
    return 1e-12 + np.r_[0.0, np.cumsum(factor)[:-1]]


def assert_pieces_agree(name, prob, masks, got, ref, spread):
    """The device's pieces `got` against the restatement's `ref` of the sorted problem: cost, gradient, S and rhs, each relative
    to its largest entry, within 8 x the restatement's own `spread` (order_spread) and for the cost 4 unit roundoffs more; S
    symmetric to the bit; a fixed parameter's row of S the identity's, its gradient and rhs entries 0."""
    assert not got["behind"]
    allowed = {k: 8 * spread[k] + (4 * U if k == "cost" else 0.0) for k in spread}
    for k in PIECES:
        a, b = np.asarray(ref[k], float), np.asarray(got[k], float)
        diff = float(np.abs(a - b).max() / np.abs(a).max())
        print(f"{name} {k}: restatement's spread {spread[k]:.3e}  GPU - restatement {diff:.3e}  allowed {allowed[k]:.3e}")
    for k in PIECES:
        a, b = np.asarray(ref[k], float), np.asarray(got[k], float)
        assert a.shape == b.shape and np.abs(a - b).max() <= allowed[k] * np.abs(a).max(), k
        assert spread[k] > 0 or k == "cost"
    assert np.array_equal(got["S"], got["S"].T)
    fixed = ~sc.free_columns(masks, prob.C).reshape(-1)
    assert fixed.sum() >= 15 + 3  # camera 0 whole, and the three lens parameters mask 0x03F leaves out
    assert np.array_equal(got["S"][fixed], np.eye(P * prob.C)[fixed]) and not got["rhs"][fixed].any() and not got["gradient"][:P * prob.C][fixed].any()


def assert_loop_walks_the_restatements(ctx, name, case):
    """mocap_rig_bundle_adjust_intrinsics at LOOP_FTOL from the start of `case` (loop_case's or shape_case's tuple) beside the
    restatement's loop: iterations, status, accept / reject sequence, per-iteration cost, damping, step lengths, the returned
    state, the gauge, obs_err."""
    prob, kd, R, t, X, masks, loss_c, ref = case
    got = adjust(ctx, prob, kd, R, t, X, masks, loss_c, ftol=sc.LOOP_FTOL)
    m = min(len(ref["history"]), len(got["history"]))
    rel = np.abs(got["history"][:m, 0] - ref["history"][:m, 0]) / ref["history"][:m, 0]
    Rg, tg = got["poses"][:, :9].reshape(-1, 3, 3), got["poses"][:, 9:]
    moved = {"R": max(rot_err(ref["R"][c], R[c]) for c in range(1, prob.C)), "t": np.abs(ref["t"] - t).max(), "X": np.abs(ref["X"] - X).max()}
    diff = {"R": max(rot_err(Rg[c], ref["R"][c]) for c in range(prob.C)), "t": np.abs(tg - ref["t"]).max(), "X": np.abs(got["points"] - ref["X"]).max()}
    kd_moved, kd_diff = np.abs(ref["kd"] - kd).max(0), np.abs(got["intrinsics"] - ref["kd"]).max(0)
    print(f"{name}: iterations {got['iterations']} / {ref['iterations']}  status {got['status']} / {ref['status']}")
    print("accepted", got["history"][:, 2], "restatement", ref["history"][:, 2])
    print("cost, relative difference per iteration", rel, "largest", rel.max())
    print("kd: moved", kd_moved, "GPU - restatement", kd_diff)
    print("poses and points: moved", moved, "GPU - restatement", diff)
    assert got["iterations"] == ref["iterations"] and got["status"] == ref["status"] == sc.STOP_FTOL
    assert np.array_equal(got["history"][:, 2], ref["history"][:, 2])
    assert (rel <= 1e-8).all()
    lam_allowed = damping_allowance(ref)
    lam_rel, step_rel = np.abs(got["history"][:, 1] / ref["history"][:, 1] - 1), np.abs(got["history"][:, 3] / ref["history"][:, 3] - 1)
    print("lambda, relative difference", lam_rel, "allowed", lam_allowed, "step", step_rel)
    with np.errstate(all="ignore"):
        print(f"{name} summary: cost {rel.max():.1e}  kd / moved {np.nanmax(kd_diff / kd_moved):.1e}  R, t, X / moved "
              f"{max(diff[k] / moved[k] for k in diff):.1e}  lambda {lam_rel.max():.1e}  step {step_rel.max():.1e}")
    assert (lam_rel <= lam_allowed).all()              # the damping follows rho
    assert (step_rel <= 1e-6 + lam_allowed).all()      # and the steps have the same length
    assert abs(got["cost_initial"] / ref["cost_initial"] - 1) < 1e-12 and abs(got["cost"] / ref["cost"] - 1) < 1e-8
    free = sc.free_columns(masks, prob.C)[:, :9]
    assert (kd_diff <= 1e-6 * kd_moved).all() and (kd_moved[free.any(0)] > 0).all()
    for k in diff:
        assert diff[k] <= 1e-6 * moved[k], k
    # the gauge: camera 0 is the world frame, |t_1| is the start's
    assert np.array_equal(got["poses"][0], np.r_[np.eye(3).reshape(9), 0, 0, 0])
    assert abs(np.linalg.norm(tg[1]) - np.linalg.norm(t[1])) <= 4 * U * np.linalg.norm(t[1])
    # obs_err is the residual of the returned state under the returned lenses
    s = got["obs_err"] ** 2
    cost = 0.5 * np.sum(s if loss_c is None else loss_c ** 2 * np.log1p(s / loss_c ** 2))
    assert abs(cost / got["cost"] - 1) < 1e-9
