"""Rig bundle adjustment on the GPU (csrc/rig_ba.hip through mocap_rig_linearize / mocap_rig_bundle_adjust and the Python
surface of mocapv2_amd.calibrate) against the NumPy restatement of the definition (tests/rig_ba_ref.py) and SciPy.  The
restatement alone meets every bar below on the CPU: tests/test_rig_ba_host.py."""
import numpy as np
import pytest

import rig_ba_ref as rb

pytestmark = pytest.mark.gpu

U = float(np.finfo(float).eps) / 2  # unit roundoff of FP64, 1.1e-16


@pytest.fixture(scope="module")
def ctx():
    from mocapv2_amd.engine import MocapContext
    return MocapContext(1, 1)


def poses12(R, t):
    return np.c_[np.asarray(R, float).reshape(len(R), 9), np.asarray(t, float).reshape(len(R), 3)]


def gpu_args(ctx, prob, R, t, X):
    ctx.set_cameras(prob.K, prob.dist, R, t)
    return (*prob.point_major(), poses12(R, t), X)


_cases = {}


def loaded(name):
    if name not in _cases:
        c = rb.case(name)
        _cases[name] = (c, rb.perturbed_start(c, rb.START_SEED[name]))
    return _cases[name]


def rms(prob, cost):
    return float(np.sqrt(cost / len(prob.pt)))


def rot_err(Ra, Rb):
    return float(np.linalg.norm(Ra @ Rb.T - np.eye(3)) / np.sqrt(2))  # = 2 sin(angle / 2), about the angle in radians


# ---- 1. pieces ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["noisy6", "noisy16"])
def test_pieces_agree_with_the_restatement(ctx, name):
    """mocap_rig_linearize at the perturbed start, lambda = 1e-3: cost, gradient, S and reduced right-hand side against the
    restatement.  Kernels and restatement form every per-observation term by the same operations; they differ in the order
    of the sums.  The allowance is 8 x the restatement's own largest spread under 10 seeded permutations of the observation
    order, each quantity relative to its largest entry.
    Restatement's spread (CPU):  noisy6   cost 1.7e-16  gradient 1.3e-15  S 1.8e-15  rhs 1.5e-15
                                 noisy16  cost 3.2e-16  gradient 2.8e-15  S 4.5e-15  rhs 3.6e-15
    GPU - restatement (MI355X):  noisy6   cost 1.7e-16  gradient 8.0e-16  S 1.3e-15  rhs 8.4e-16
                                 noisy16  cost 1.6e-16  gradient 1.8e-15  S 1.9e-15  rhs 2.4e-15   (also DESIGN.md section 2)"""
    c, (R, t, X) = loaded(name)
    prob = c["prob"]
    spread = rb.order_spread(prob, R, t, X, 1e-3)
    ref = rb.linearize(prob.sorted(), R, t, X, 1e-3)
    got = ctx.rig_linearize(*gpu_args(ctx, prob, R, t, X), 1e-3)
    assert not got["behind"]
    for k in ("cost", "gradient", "S", "rhs"):
        a, b = np.asarray(ref[k], float), np.asarray(got[k], float)
        diff = float(np.abs(a - b).max() / np.abs(a).max())
        print(f"{name} {k}: restatement's spread {spread[k]:.3e}  GPU - restatement {diff:.3e}  allowed {8 * spread[k]:.3e}")
    for k in ("cost", "gradient", "S", "rhs"):
        a, b = np.asarray(ref[k], float), np.asarray(got[k], float)
        assert spread[k] > 0 and np.abs(a - b).max() <= 8 * spread[k] * np.abs(a).max(), k
    assert np.array_equal(got["S"], got["S"].T)


# ---- 2. loop --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["noisy6", "noisy16"])
def test_loop_walks_the_restatements_iterations(ctx, name):
    """Same accept / reject sequence, same number of iterations, same stopping rule as the restatement (ftol =
    rig_ba_ref.LOOP_FTOL = 1e-9: the loop then stops on a step far above the rounding of the cost; why the default 1e-12
    cannot be compared is in test_rig_ba_host.py::test_loop_cases_are_far_from_every_decision_boundary).  The condition
    is asserted here, not assumed: no iteration of the restatement has |rho| < 1e-3.
    Per-iteration cost: allowed relative difference 1e-8.  Reasoning, not a fit: the two sides solve systems that agree to
    ~1e-15 (test 1); the damped S has a condition number below 1e6 on these cases (printed), so steps agree to ~1e-9 of
    their length and the cost, at most linearly sensitive to the state, to better than 1e-8 of itself.  Measured on the
    MI355X: cond(S) 1.5e4 / 1.8e4; largest relative cost difference 2.0e-14 (noisy6, 5 iterations) and 6.4e-14 (noisy16, 6)."""
    c, (R, t, X) = loaded(name)
    prob = c["prob"]
    ref = rb.lm(prob, R, t, X, ftol=rb.LOOP_FTOL)
    assert (np.abs(ref["rho"]) >= 1e-3).all(), ref["rho"]
    cond = np.linalg.cond(rb.linearize(prob, R, t, X, 1e-3)["S"])
    got = ctx.rig_bundle_adjust(*gpu_args(ctx, prob, R, t, X), ftol=rb.LOOP_FTOL)
    rel = np.abs(got["history"][:len(ref["history"]), 0] - ref["history"][:len(got["history"]), 0]) / ref["history"][:len(got["history"]), 0]
    print(f"{name}: iterations {got['iterations']} / {ref['iterations']}  status {got['status']} / {ref['status']}  cond(S) {cond:.3e}")
    print("accepted", got["history"][:, 2], "restatement", ref["history"][:, 2])
    print("cost, relative difference per iteration", rel, "lambda", got["history"][:, 1], "step", got["history"][:, 3])
    assert cond < 1e6
    assert got["iterations"] == ref["iterations"] and got["status"] == ref["status"] == rb.STOP_FTOL
    assert np.array_equal(got["history"][:, 2], ref["history"][:, 2])
    assert (rel <= 1e-8).all()
    assert np.abs(got["history"][:, 1] / ref["history"][:, 1] - 1).max() < 1e-6  # the damping follows rho
    assert np.abs(got["history"][:, 3] / ref["history"][:, 3] - 1).max() < 1e-6  # and the steps have the same length
    assert abs(got["cost_initial"] / ref["cost_initial"] - 1) < 1e-12 and abs(got["cost"] / ref["cost"] - 1) < 1e-8


# ---- 3. bits --------------------------------------------------------------------------------------------------------------------
def test_two_runs_give_the_same_bits_also_after_a_larger_problem(ctx):
    c6, (R6, t6, X6) = loaded("noisy6")
    c16, (R16, t16, X16) = loaded("noisy16")

    def run6():
        out = ctx.rig_bundle_adjust(*gpu_args(ctx, c6["prob"], R6, t6, X6))
        lin = ctx.rig_linearize(*gpu_args(ctx, c6["prob"], R6, t6, X6), 1e-3)
        return out, lin

    a, la = run6()
    b, lb = run6()
    ctx.rig_bundle_adjust(*gpu_args(ctx, c16["prob"], R16, t16, X16))  # unrelated, larger: the scratch grows and is reused
    d, ld = run6()
    for other, lin in ((b, lb), (d, ld)):
        for k in ("poses", "points", "history"):
            assert a[k].tobytes() == other[k].tobytes(), k
        assert (a["status"], a["iterations"], a["cost"], a["cost_initial"]) == (other["status"], other["iterations"], other["cost"], other["cost_initial"])
        for k in ("gradient", "S", "rhs"):
            assert la[k].tobytes() == lin[k].tobytes(), k
        assert la["cost"] == lin["cost"]


# ---- 4. the reference's data ----------------------------------------------------------------------------------------------------
def test_reference_capture_beats_the_references_result(ctx):
    """tests/golden/jsons, 54 points, start before_ba_extrinsics.json (a start with every point behind both cameras: adjusted
    as its mirror image, bundle_adjust_rig's docstring).  Bars: final rms <= the rms of after_ba_extrinsics.json with its
    points re-optimised (SciPy, 1.2566 px); cost within 1e-6 of SciPy's joint minimum from the same start (rms 1.00221 px);
    |t_1| unchanged.  Measured on the MI355X: rms 1.002213 px after 9 iterations, cost / joint minimum - 1 = -3.1e-14."""
    from mocapv2_amd import calibrate as cal
    b = rb.bundled()
    prob = b["prob"]
    R, t = b["start"]
    poses = [{"R": R[c], "t": t[c].reshape(3, 1)} for c in range(2)]
    out = cal.bundle_adjust_rig(b["image_points"], b["valid"], poses, b["camera_params"], ctx=ctx)
    Ra, ta = b["after"]
    after = rb.scipy_minimum(prob, Ra, ta, rb.triangulate_dlt(prob, Ra, ta), fix_poses=True)[0]
    joint = rb.scipy_minimum(prob, R, t, rb.triangulate_dlt(prob, R, t))[0]
    t1 = np.linalg.norm(out["poses"][1]["t"])
    print(f"rms {out['rms_px']:.6f}  after_ba re-optimised {rms(prob, after):.6f}  joint minimum {rms(prob, joint):.6f}  cost / joint - 1 "
          f"{out['cost'] / joint - 1:.3e}  iterations {out['iterations']} status {out['status']}  |t1| {t1!r} from {np.linalg.norm(t[1])!r}")
    assert out["mirrored"] and out["used"].all() and out["status"] in (rb.STOP_FTOL, rb.STOP_LAMBDA, rb.STOP_MAX_ITERS)
    assert abs(rms(prob, after) - 1.2566) < 1e-4 and abs(rms(prob, joint) - 1.00221) < 1e-5
    assert out["rms_px"] <= rms(prob, after)
    assert abs(out["cost"] / joint - 1) <= 1e-6
    assert abs(t1 - np.linalg.norm(t[1])) <= 4 * U * np.linalg.norm(t[1])
    # the result is a state of the caller's convention: its cost, recomputed by the restatement, is the one reported
    Rn = np.array([p["R"] for p in out["poses"]])
    tn = np.array([p["t"].reshape(3) for p in out["poses"]])
    assert abs(rb.cost_of(prob, Rn, tn, out["points"])[0] / out["cost"] - 1) < 1e-9


# ---- 5. no ground truth given ---------------------------------------------------------------------------------------------------
def aligned_errors(scene, X_true, poses):
    """(largest rotation error, largest camera-centre error) against the scene after aligning camera 0 and |t_1|"""
    R, t, _ = rb.truth_in_camera0(scene, X_true)
    R0, t0 = np.asarray(poses[0]["R"], float), np.asarray(poses[0]["t"], float).reshape(3)
    Rg = [np.asarray(p["R"], float) @ R0.T for p in poses]
    tg = [np.asarray(p["t"], float).reshape(3) - Rg[c] @ t0 for c, p in enumerate(poses)]
    s = np.linalg.norm(t[1]) / np.linalg.norm(tg[1])
    return (max(rot_err(Rg[c], R[c]) for c in range(len(R))),
            max(float(np.linalg.norm(-Rg[c].T @ tg[c] * s + R[c].T @ t[c])) for c in range(len(R))))


def restatement_from(c, poses, used, X0):
    prob = rb.problem_from_arrays(c["image_points"][:, used], c["valid"][:, used], c["scene"].camera_params)
    R = np.array([np.asarray(p["R"], float) for p in poses])
    t = np.array([np.asarray(p["t"], float).reshape(3) for p in poses])
    return prob, R, t, rb.lm(prob, R, t, X0)


def test_calibrate_rig_on_clean6(ctx):
    """No poses given, exact float pixels: the rms and, after aligning camera 0 and |t_1| to the scene, the rotation and
    camera-centre errors are at most 10 x those of the restatement run from the same initial poses and start points.
    Measured on the MI355X: tree 0-3, 3-1, 3-2, 3-4, 3-5; rms 9.0e-14 px, rotation error 6.1e-16, centre error 4.8e-15 world
    units after 37 iterations (status: lambda), the restatement's figures to all digits printed."""
    from mocapv2_amd import calibrate as cal
    c = rb.case("clean6")
    out = cal.calibrate_rig(c["image_points"], c["valid"], c["scene"].camera_params, threshold=3.0, ctx=ctx)
    used = out["used"]
    # the start points of that run: triangulated from the initial poses exactly as calibrate_rig did
    X0 = start_points(ctx, cal, c, out["poses_initial"])[used]
    prob, R, t, ref = restatement_from(c, out["poses_initial"], used, X0)
    ref_poses = [{"R": ref["R"][k], "t": ref["t"][k]} for k in range(len(R))]
    e_gpu, e_ref = aligned_errors(c["scene"], c["X"], out["poses"]), aligned_errors(c["scene"], c["X"], ref_poses)
    print(f"tree {out['init']['tree']} scales {np.round(out['init']['scales'], 4)}")
    print(f"rms GPU {out['rms_px']:.3e} restatement {rms(prob, ref['cost']):.3e}; rotation GPU {e_gpu[0]:.3e} restatement {e_ref[0]:.3e}; "
          f"centre GPU {e_gpu[1]:.3e} restatement {e_ref[1]:.3e}; iterations {out['iterations']} / {ref['iterations']}")
    assert used.sum() == len(used)
    assert out["rms_px"] <= 10 * rms(prob, ref["cost"])
    assert e_gpu[0] <= 10 * e_ref[0] and e_gpu[1] <= 10 * e_ref[1]


def start_points(ctx, cal, c, poses):
    """The start points bundle_adjust_rig triangulates when none are given (same calls)"""
    params = c["scene"].camera_params
    ip, vis, K, d = cal._rig_inputs(c["image_points"], c["valid"], params)
    und = np.stack([cal.undistort_points(ip[k], K[k], d[k]) for k in range(len(K))])
    R = np.array([np.asarray(p["R"], float) for p in poses])
    t = np.array([np.asarray(p["t"], float).reshape(3) for p in poses])
    ctx.set_cameras(K, d, R, t)
    X, _ = ctx.triangulate_batch(np.ascontiguousarray(np.transpose(und, (1, 0, 2))), vis.T.astype(np.uint8), compact_k=False)
    return X


@pytest.mark.parametrize("name", ["noisy6", "noisy16"])
def test_calibrate_rig_on_noisy_rigs(ctx, name):
    """sigma = 0.5 px.  Bars: the final rms is below sigma (the minimum lies at or below the truth's cost, about
    sigma sqrt(1 - p / m): 0.78 sigma for noisy6); the cost is within 1e-6 of SciPy's minimum from the same start (sparse
    Jacobian and LSMR for both rigs: the dense solve of noisy6 is the host test's).
    Measured on the MI355X: noisy6 rms 0.38977 px from 0.627 at the start, cost / SciPy's - 1 = -3.9e-10, 5 iterations;
    noisy16 rms 0.46586 from 0.592, -1.1e-9, 6 iterations (SciPy's LSMR stops that much above)."""
    from mocapv2_amd import calibrate as cal
    c = rb.case(name)
    out = cal.calibrate_rig(c["image_points"], c["valid"], c["scene"].camera_params, threshold=3.0, ctx=ctx)
    used = out["used"]
    X0 = start_points(ctx, cal, c, out["poses_initial"])[used]
    prob = rb.problem_from_arrays(c["image_points"][:, used], c["valid"][:, used], c["scene"].camera_params)
    R = np.array([np.asarray(p["R"], float) for p in out["poses_initial"]])
    t = np.array([np.asarray(p["t"], float).reshape(3) for p in out["poses_initial"]])
    ref = rb.scipy_minimum(prob, R, t, X0, sparse=True)[0]
    e = aligned_errors(c["scene"], c["X"], out["poses"])
    print(f"{name}: tree {out['init']['tree']} scales {np.round(out['init']['scales'], 4)} used {used.sum()} / {len(used)}")
    print(f"rms {out['rms_px']:.5f} (start {np.sqrt(out['cost_initial'] / len(prob.pt)):.3f})  cost / scipy - 1 {out['cost'] / ref - 1:.3e}  "
          f"iterations {out['iterations']} status {out['status']}  rotation error {e[0]:.3e} centre error {e[1]:.3e}")
    assert out["rms_px"] < c["sigma"]
    assert abs(out["cost"] / ref - 1) <= 1e-6
    assert abs(np.linalg.norm(out["poses"][1]["t"]) - np.linalg.norm(out["poses_initial"][1]["t"])) < 1e-14


# ---- 6. edges -------------------------------------------------------------------------------------------------------------------
def test_a_point_with_one_view_is_reported_and_left_out(ctx):
    from mocapv2_amd import calibrate as cal
    c = rb.case("noisy6", 120)
    valid = c["valid"].copy()
    lone = [3, 50]
    for n in lone:
        keep = np.flatnonzero(valid[:, n])[0]
        valid[:, n] = False
        valid[keep, n] = True
    R, t, X = rb.truth_in_camera0(c["scene"], c["X"])
    poses = [{"R": R[k], "t": t[k]} for k in range(len(R))]
    out = cal.bundle_adjust_rig(c["image_points"], valid, poses, c["scene"].camera_params, points=X, ctx=ctx)
    full = cal.bundle_adjust_rig(c["image_points"][:, out["used"]], valid[:, out["used"]], poses, c["scene"].camera_params, points=X[out["used"]], ctx=ctx)
    assert not out["used"][lone].any() and out["used"].sum() == len(X) - 2 and np.isnan(out["points"][lone]).all()
    assert np.isfinite(out["points"][out["used"]]).all()
    assert out["cost"] == full["cost"] and out["points"][out["used"]].tobytes() == full["points"].tobytes()  # they did not enter the problem


def test_a_disconnected_camera_raises(ctx):
    from mocapv2_amd import calibrate as cal
    c = rb.case("noisy6", 200)
    valid = c["valid"].copy()
    seen4 = np.flatnonzero(valid[4])
    valid[4, seen4[5:]] = False  # camera 4 keeps 5 points: no pair with 8 common points
    with pytest.raises(ValueError, match="camera 4"):
        cal.rig_initial_poses(c["image_points"], valid, c["scene"].camera_params, threshold=3.0, ctx=ctx)


def test_two_cameras(ctx):
    from mocapv2_amd import calibrate as cal
    c = rb.case("noisy6", 200)
    ip, valid = c["image_points"][:2], c["valid"][:2]
    out = cal.calibrate_rig(ip, valid, c["scene"].camera_params[:2], threshold=3.0, ctx=ctx)
    print("two cameras: used", out["used"].sum(), "rms", out["rms_px"], "iterations", out["iterations"], "status", out["status"])
    assert out["used"].sum() == (valid.sum(0) == 2).sum() and out["rms_px"] < c["sigma"]
    assert abs(np.linalg.norm(out["poses"][1]["t"]) - 1.0) < 1e-14  # the first edge has unit length


def test_thirty_two_cameras_with_64_points(ctx):
    """D = 186: the Cholesky runs in global memory.  Checked against the restatement like the loop test."""
    from mocapv2_amd import synth
    scene = synth.Scene(32, 1920, 1080, synth.MILD_DIST)
    rng = np.random.default_rng(32)
    Xw = rng.uniform(-0.5, 0.5, (64, 3))
    px = np.stack([synth.project(Xw, p, scene.K, scene.dist) for p in scene.poses]) + rng.normal(0, 0.5, (32, 64, 2))
    valid = rng.uniform(0, 1, (32, 64)) > 0.3
    prob = rb.problem_from_arrays(px, valid, scene.camera_params)
    case = {"scene": scene, "X": Xw}
    R, t, X = rb.perturbed_start(case, 33, rot=0.003, trans=0.005, point=0.005)
    assert prob.C == 32 and prob.N == 64 and np.bincount(prob.pt).min() >= 2
    ref = rb.lm(prob, R, t, X, ftol=rb.LOOP_FTOL)
    got = ctx.rig_bundle_adjust(*gpu_args(ctx, prob, R, t, X), ftol=rb.LOOP_FTOL)
    lin_ref, lin = rb.linearize(prob.sorted(), R, t, X, 1e-3), ctx.rig_linearize(*gpu_args(ctx, prob, R, t, X), 1e-3)
    print("C = 32: iterations", got["iterations"], ref["iterations"], "status", got["status"], ref["status"], "cost", got["cost"], ref["cost"],
          "rho", ref["rho"], "S difference", np.abs(lin["S"] - lin_ref["S"]).max() / np.abs(lin_ref["S"]).max())
    assert np.abs(lin["S"] - lin_ref["S"]).max() <= 1e-12 * np.abs(lin_ref["S"]).max()
    assert got["status"] > 0 and rms(prob, got["cost"]) < 0.5
    assert abs(got["cost"] / ref["cost"] - 1) < 1e-6


def test_a_broken_layout_and_a_start_behind_the_cameras_are_reported(ctx):
    from mocapv2_amd import _abi
    c, (R, t, X) = loaded("noisy6")
    prob = c["prob"]
    off, cam, uv = prob.point_major()
    ctx.set_cameras(prob.K, prob.dist, R, t)
    bad = cam.copy()
    bad[off[7]], bad[off[7] + 1] = cam[off[7] + 1], cam[off[7]]  # descending within point 7
    with pytest.raises(ValueError):
        ctx.rig_bundle_adjust(off, bad, uv, poses12(R, t), X)
    Rm, tm, Xm = rb.mirrored(R, t, X)
    with pytest.raises(_abi.MocapError) as e:
        ctx.rig_bundle_adjust(off, cam, uv, poses12(Rm, tm), Xm)
    assert e.value.code == -3
