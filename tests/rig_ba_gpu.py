"""What tests/test_gpu_rig_ba_shapes.py needs of the device: the call helpers of the pose-only rig adjustment (csrc/rig_ba.hip),
and the comparisons of its pieces and of its loop with the NumPy restatements tests/rig_ba_ref.py and tests/rig_robust_ref.py.
Not a test module; the reasoning behind every bound is in the docstrings of the tests that call these."""
import numpy as np

import rig_ba_ref as rb
import rig_robust_ref as rr

U = float(np.finfo(float).eps) / 2  # unit roundoff of FP64, 1.1e-16
PIECES = ("cost", "gradient", "S", "rhs")
E_LAYOUT, E_BEHIND = -2, -3  # MOCAP_RIG_E_*


def poses12(R, t):
    return np.c_[np.asarray(R, float).reshape(len(R), 9), np.asarray(t, float).reshape(len(R), 3)]


def loss_args(loss_c):
    return {} if loss_c is None else {"loss": "cauchy", "loss_scale": loss_c}


def gpu_args(ctx, prob, R, t, X):
    ctx.set_cameras(prob.K, prob.dist, R, t)
    return (*prob.point_major(), poses12(R, t), X)


def linearize(ctx, case, X=None, lam=1e-3):
    """ctx.rig_linearize at the start of a case of rig_ba_ref.shape_case (X: other points in their place), under its loss"""
    return ctx.rig_linearize(*gpu_args(ctx, case["prob"], case["R"], case["t"], case["X"] if X is None else X), lam, **loss_args(case["loss_c"]))


def adjust(ctx, case, X=None, **kw):
    """ctx.rig_bundle_adjust from the start of a case, under its loss unless kw names one"""
    kw = {**loss_args(case["loss_c"]), **kw}
    return ctx.rig_bundle_adjust(*gpu_args(ctx, case["prob"], case["R"], case["t"], case["X"] if X is None else X), **kw)


def rot_err(Ra, Rb):
    return float(np.linalg.norm(Ra @ Rb.T - np.eye(3)) / np.sqrt(2))  # = 2 sin(angle / 2), about the angle in radians


def adjust_raw(ctx, case, off, cam, uv, X, max_iters=10):
    """mocap_rig_bundle_adjust through the C-ABI, where the arrays can be looked at after a negative status: (return code,
    result [4], poses, points, history as the device holds them afterwards).  off, cam, uv: the observation arrays handed in, in
    the place of the case's own"""
    import torch
    from mocapv2_amd._dev import _ptr, _stream
    prob, poses = case["prob"], poses12(case["R"], case["t"])
    ctx.set_cameras(prob.K, prob.dist, case["R"], case["t"])
    d = {k: torch.from_numpy(np.ascontiguousarray(v)).to(ctx.device) for k, v in
         (("off", off), ("cam", cam), ("uv", uv), ("poses", poses), ("pts", X))}
    hist = torch.zeros((max_iters, 4), dtype=torch.float64, device=ctx.device)
    result = torch.zeros((4,), dtype=torch.float64, device=ctx.device)
    rc = ctx.lib.mocap_rig_bundle_adjust(ctx._h, prob.C, prob.N, len(cam), _ptr(d["off"]), _ptr(d["cam"]), _ptr(d["uv"]), _ptr(d["poses"]),
                                         _ptr(d["pts"]), max_iters, 1e-12, 1e-3, _ptr(hist), _ptr(result), _stream())
    ctx.sync()
    return rc, result.cpu().numpy(), d["poses"].cpu().numpy(), d["pts"].cpu().numpy(), hist.cpu().numpy()


def assert_pieces_agree(name, got, ref, spread):
    """The device's pieces `got` against the restatement's `ref` of the sorted problem: cost, gradient, S and rhs, each relative
    to its largest entry, within 8 x the restatement's own `spread` (order_spread) and for the cost 4 unit roundoffs more; S
    symmetric to the bit; no point behind a camera"""
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


def assert_loop_walks_the_restatements(ctx, name):
    """mocap_rig_bundle_adjust (under a loss: _robust) at LOOP_FTOL from the start of the case beside the restatement's loop:
    iterations, status, accept / reject sequence, per-iteration cost, damping, step lengths, the returned state, the gauge,
    obs_err and, under the loss, obs_weight.  Every figure is printed and every condition looked at before the first one
    fails the test."""
    case, ref = rb.shape_case(name), rb.shape_loop(name)
    prob, R, t, X, loss_c = (case[k] for k in ("prob", "R", "t", "X", "loss_c"))
    got = adjust(ctx, case, ftol=rb.LOOP_FTOL)
    # obs_err is the robust entry's: without a loss the same call through it, which gives the plain entry's bits
    per_obs = got if loss_c is not None else adjust(ctx, case, ftol=rb.LOOP_FTOL, loss="none")
    m = min(len(ref["history"]), len(got["history"]))
    rel = np.abs(got["history"][:m, 0] - ref["history"][:m, 0]) / ref["history"][:m, 0]
    lam_rel = np.abs(got["history"][:m, 1] / ref["history"][:m, 1] - 1)
    with np.errstate(all="ignore"):
        step_rel = np.abs(got["history"][:m, 3] / ref["history"][:m, 3] - 1)
    Rg, tg = got["poses"][:, :9].reshape(-1, 3, 3), got["poses"][:, 9:]
    moved = {"R": max(rot_err(ref["R"][c], R[c]) for c in range(1, prob.C)), "t": np.abs(ref["t"] - t).max(), "X": np.abs(ref["X"] - X).max()}
    diff = {"R": max(rot_err(Rg[c], ref["R"][c]) for c in range(prob.C)), "t": np.abs(tg - ref["t"]).max(), "X": np.abs(got["points"] - ref["X"]).max()}
    s = per_obs["obs_err"] ** 2
    cost_again = 0.5 * np.sum(s if loss_c is None else loss_c ** 2 * np.log1p(s / loss_c ** 2))
    print(f"{name}: iterations {got['iterations']} / {ref['iterations']}  status {got['status']} / {ref['status']}")
    print("accepted", got["history"][:, 2], "restatement", ref["history"][:, 2])
    print("cost, relative difference per iteration", rel, "lambda", lam_rel, "step", step_rel)
    print("poses and points: moved", moved, "GPU - restatement", diff)
    print(f"{name} summary: cost {rel.max():.1e}  R, t, X / moved {max(diff[k] / moved[k] for k in diff):.1e}  lambda {lam_rel.max():.1e}  "
          f"step {step_rel.max():.1e}  obs_err's cost / cost - 1 {cost_again / got['cost'] - 1:.1e}")
    checks = {
        "iterations": got["iterations"] == ref["iterations"],
        "status": got["status"] == ref["status"] == rb.STOP_FTOL,
        "accept sequence": np.array_equal(got["history"][:, 2], ref["history"][:, 2]),
        "cost per iteration 1e-8": bool((rel <= 1e-8).all()),
        "lambda 1e-6": bool(lam_rel.max() < 1e-6),             # the damping follows rho
        "step length 1e-6": bool(step_rel.max() < 1e-6),       # and the steps have the same length
        "cost_initial 1e-12": abs(got["cost_initial"] / ref["cost_initial"] - 1) < 1e-12,
        "cost 1e-8": abs(got["cost"] / ref["cost"] - 1) < 1e-8,
        "returned state 1e-6 of what it moved": all(diff[k] <= 1e-6 * moved[k] for k in diff) and all(v > 0 for v in moved.values()),
        # the gauge: camera 0 is the world frame, |t_1| is the start's
        "camera 0": np.array_equal(got["poses"][0], np.r_[np.eye(3).reshape(9), 0, 0, 0]),
        "|t_1|": abs(np.linalg.norm(tg[1]) - np.linalg.norm(t[1])) <= 4 * U * np.linalg.norm(t[1]),
        # obs_err is the residual of the returned state
        "obs_err's cost": per_obs["obs_err"].shape == (len(prob.pt),) and abs(cost_again / got["cost"] - 1) < 1e-9,
    }
    if loss_c is None:
        for k in ("poses", "points", "history"):
            checks[f"loss none gives the plain entry's {k}"] = per_obs[k].tobytes() == got[k].tobytes()
        checks["weights of loss none"] = bool((per_obs["obs_weight"] == 1.0).all())
    else:
        err, w = rr.errors_and_weights(prob, ref["R"], ref["t"], ref["X"], loss_c)
        e_rel, w_rel = float(np.abs(got["obs_err"] / err - 1).max()), float(np.abs(got["obs_weight"] / w - 1).max())
        print(f"obs_err relative difference {e_rel:.3e}  obs_weight {w_rel:.3e}")
        checks["obs_err 1e-6"], checks["obs_weight 1e-6"] = e_rel <= 1e-6, w_rel <= 1e-6
    failed = [k for k, ok in checks.items() if not ok]
    assert not failed, failed
