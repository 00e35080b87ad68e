"""Rig bundle adjustment, the part that needs no GPU: the NumPy restatement of the definition (tests/rig_ba_ref.py) against
central differences, a dense solve and SciPy; the bars of tests/test_gpu_rig_ba.py met by the restatement alone; the host-side
helpers; the C-ABI surface of the two new entry points; the code-object table of the new kernels."""
import ctypes
import importlib.util
import os
import re

import numpy as np
import pytest

import rig_ba_ref as rb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rms(prob, cost):
    return float(np.sqrt(cost / len(prob.pt)))


@pytest.fixture(scope="module")
def noisy6():
    c = rb.case("noisy6")
    return c, rb.perturbed_start(c, rb.START_SEED["noisy6"])


# ---- the restatement ------------------------------------------------------------------------------------------------------
def test_the_cases_are_what_the_definition_says():
    for name, (n_cam, _, _, n, _, _) in rb.CASES.items():
        c = rb.case(name)
        prob = c["prob"]
        counts = np.bincount(prob.pt, minlength=prob.N)
        print(name, "points", prob.N, "observations", len(prob.pt), "views per point", counts.min(), counts.mean(), counts.max())
        assert prob.C == n_cam and 0.8 * n <= prob.N <= n and counts.min() >= 2
        assert c["valid"].shape == (n_cam, prob.N) and int(c["valid"].sum()) == len(prob.pt)
        assert counts.mean() < 0.75 * n_cam  # partial visibility: the 30 % dropout
        off, cam, uv = prob.point_major()
        assert off[-1] == len(cam) and all((np.diff(cam[off[i]:off[i + 1]]) > 0).all() for i in range(0, prob.N, 37))


def test_analytic_jacobian_agrees_with_central_differences(noisy6):
    """Every camera column and 40 point columns, step 1e-6 in the local perturbation: largest difference relative to the
    column's largest entry 1.1e-9 (noisy6), the accuracy of the difference quotient itself."""
    c, (R, t, X) = noisy6
    prob = c["prob"]
    lin = rb.linearize(prob, R, t, X, 1e-3)
    D, h, worst = prob.D, 1e-6, 0.0
    res = lambda dc, dp: rb.observe(prob, *rb.apply_step(prob, R, t, X, dc, dp))[0]
    for k in list(range(D)) + list(range(D, D + 3 * prob.N, 3 * prob.N // 40)):
        e = np.zeros(D + 3 * prob.N)
        e[k] = h
        num = (res(e[:D], e[D:].reshape(-1, 3)) - res(-e[:D], -e[D:].reshape(-1, 3))) / (2 * h)
        ana = np.zeros_like(num)
        if k < D:
            sel = prob.cam == k // 6 + 1
            ana[sel] = lin["jc"][sel][:, :, k % 6]
        else:
            sel = prob.pt == (k - D) // 3
            ana[sel] = lin["jp"][sel][:, :, (k - D) % 3]
        worst = max(worst, np.abs(ana - num).max() / np.abs(num).max())
    print("jacobian against central differences:", worst)
    assert worst < 1e-7
    # and the gradient is J^T r of those blocks
    g = np.zeros(D + 3 * prob.N)
    for o in range(len(prob.pt)):
        if prob.cam[o] > 0:
            g[6 * (prob.cam[o] - 1):6 * prob.cam[o]] += lin["jc"][o].T @ lin["r"][o]
        g[D + 3 * prob.pt[o]:D + 3 * prob.pt[o] + 3] += lin["jp"][o].T @ lin["r"][o]
    assert np.abs(g - lin["gradient"]).max() <= 1e-12 * np.abs(g).max()


def test_schur_step_equals_the_dense_solve(noisy6):
    c, (R, t, X) = noisy6
    prob = c["prob"]
    for lam in (1e-3, 10.0):
        lin = rb.linearize(prob, R, t, X, lam)
        dc, dp, pred = rb.schur_step(prob, lin, lam)
        dc2, dp2 = rb.dense_step(prob, lin, lam)
        print("lambda", lam, "cameras", np.abs(dc - dc2).max() / np.abs(dc2).max(), "points", np.abs(dp - dp2).max() / np.abs(dp2).max())
        assert np.abs(dc - dc2).max() < 1e-9 * np.abs(dc2).max() and np.abs(dp - dp2).max() < 1e-9 * np.abs(dp2).max()
        assert pred > 0 and np.abs(lin["S"] - lin["S"].T).max() == 0.0


def test_restatement_reaches_scipys_minimum_on_noisy6(noisy6):
    """From the perturbed truth (rms 20.5 px) the restatement's loop stops after 6 accepted iterations on the ftol rule at
    cost 251.58535733930 (rms 0.3898 px < sigma = 0.5).  SciPy least_squares (trf, x_scale='jac', tolerances 1e-12, dense
    Jacobian) from the same start: 251.58535733932.  Measured ratio - 1 = -7.2e-14."""
    c, (R, t, X) = noisy6
    prob = c["prob"]
    out = rb.lm(prob, R, t, X)
    ref = rb.scipy_minimum(prob, R, t, X, sparse=False)[0]
    print("restatement", out["cost"], "scipy", ref, "ratio - 1", out["cost"] / ref - 1, "iterations", out["iterations"], out["history"][:, 2])
    assert out["status"] == rb.STOP_FTOL and out["history"][:, 2].all()
    assert abs(out["cost"] / ref - 1) < 1e-9
    assert rms(prob, out["cost"]) < c["sigma"]


def test_restatement_meets_the_gpu_tests_bars_on_noisy16():
    """rms 0.4659 px < 0.5 after 7 iterations; SciPy with the sparse Jacobian (LSMR) stops 1.4e-9 above."""
    c = rb.case("noisy16")
    prob = c["prob"]
    R, t, X = rb.perturbed_start(c, rb.START_SEED["noisy16"])
    out = rb.lm(prob, R, t, X)
    ref = rb.scipy_minimum(prob, R, t, X)[0]
    print("restatement", out["cost"], "scipy", ref, "ratio - 1", out["cost"] / ref - 1, "rms", rms(prob, out["cost"]))
    assert rms(prob, out["cost"]) < c["sigma"] and abs(out["cost"] / ref - 1) < 1e-6


def test_restatement_on_the_reference_capture():
    """tests/golden/jsons: 54 points, two cameras.  before_ba_extrinsics.json puts every point BEHIND both cameras (the
    reference's candidate vote); its mirror image (R, -t, -X) projects the same and is the start.  Measured: start rms
    5.2057 px (DLT points), restatement 1.002213 px after 9 iterations, SciPy's joint minimum 1.002213 (ratio - 1 =
    -2.4e-14); the reference's after_ba_extrinsics.json with DLT points 1.2680, with its points re-optimised 1.256650."""
    b = rb.bundled()
    prob = b["prob"]
    R, t = b["start"]
    X = rb.triangulate_dlt(prob, R, t)
    cost0, front = rb.cost_of(prob, R, t, X)
    assert not front and ((X @ R[1].T + t[1])[:, 2] < 0).all() and (X[:, 2] < 0).all()
    Rm, tm, Xm = rb.mirrored(R, t, X)
    assert rb.cost_of(prob, Rm, tm, Xm) == (cost0, True)
    out = rb.lm(prob, Rm, tm, Xm)
    joint = rb.scipy_minimum(prob, R, t, X)[0]
    Ra, ta = b["after"]
    after = rb.scipy_minimum(prob, Ra, ta, rb.triangulate_dlt(prob, Ra, ta), fix_poses=True)[0]
    print("start", rms(prob, cost0), "restatement", rms(prob, out["cost"]), "scipy joint", rms(prob, joint), "after_ba re-optimised",
          rms(prob, after), "iterations", out["iterations"], "|t1|", np.linalg.norm(out["t"][1]))
    assert abs(rms(prob, joint) - 1.00221) < 1e-5 and abs(rms(prob, after) - 1.2566) < 1e-4  # the figures of the issue
    assert rms(prob, out["cost"]) <= rms(prob, after)
    assert abs(out["cost"] / joint - 1) < 1e-6
    assert abs(np.linalg.norm(out["t"][1]) - np.linalg.norm(t[1])) < 1e-14


def test_loop_cases_are_far_from_every_decision_boundary():
    """The condition the GPU loop test stands on, checked on the restatement: with ftol = 1e-9 no iteration of noisy6 or
    noisy16 has |rho| < 1e-3; more than that, every gain ratio lies within 0.01 of 1 (the step is far above the rounding
    of the cost) and no relative decrease lies within a factor 1.2 of ftol.  (With the default ftol = 1e-12 the last
    iteration of noisy16 lowers the cost by 4e-15 of itself -- rho = 13.9, rounding alone: its sign is not a property of the
    definition, so the loop comparison does not use that ftol.)"""
    for name in ("noisy6", "noisy16"):
        c = rb.case(name)
        out = rb.lm(c["prob"], *rb.perturbed_start(c, rb.START_SEED[name]), ftol=rb.LOOP_FTOL)
        costs = np.r_[out["cost_initial"], out["history"][:, 0]]
        rel = (costs[:-1] - costs[1:]) / costs[:-1]
        print(name, "rho", out["rho"], "relative decrease", rel)
        assert (np.abs(out["rho"]) >= 1e-3).all() and (np.abs(out["rho"] - 1) < 0.01).all()
        assert ((rel > 1.2 * rb.LOOP_FTOL) | (rel < rb.LOOP_FTOL / 1.2)).all() and out["status"] == rb.STOP_FTOL


def aligned_errors(scene, X_true, R, t):
    """(largest rotation error, largest camera-centre error) of a state with camera 0 at the origin against the scene"""
    Rt, tt, _ = rb.truth_in_camera0(scene, X_true)
    s = np.linalg.norm(tt[1]) / np.linalg.norm(t[1])
    return (max(float(np.linalg.norm(R[c] @ Rt[c].T - np.eye(3)) / np.sqrt(2)) for c in range(len(R))),
            max(float(np.linalg.norm(-R[c].T @ t[c] * s + Rt[c].T @ tt[c])) for c in range(len(R))))


def test_restatement_meets_the_gpu_tests_bars_on_the_rig_of_unequal_cameras():
    """mixed6 / mixed6_clean: six cameras that all differ in K (focal lengths 1120 .. 1750 px, fy != fx, principal points off
    centre) and in lens, no point shared by cameras 0 and 1 (tests/test_gpu_mixed_rig.py runs the GPU on them).
    mixed6 from the perturbed truth, lambda = 1e-3: spread under 10 permutations cost 1.3e-16, gradient 5.8e-16, S 2.1e-15,
    rhs 7.6e-16, cond(S) 2.0e4; with ftol = 1e-9 the loop takes 6 accepted iterations, every rho within 4e-4 of 1, rms
    0.3794 px < sigma.  mixed6_clean: rms 9.6e-14 px, rotation error 5.5e-16, centre error 2.4e-15 after 37 iterations
    (status: lambda).  With every camera given camera 0's K and lens the start of mixed6 (rms 20 px) costs 27.7 times as
    much: a wrong-camera read cannot hide in these numbers."""
    c = rb.case("mixed6")
    prob = c["prob"]
    assert len({tuple(k.ravel()) for k in prob.K}) == 6 and len({tuple(d) for d in prob.dist}) == 4
    assert not (c["valid"][0] & c["valid"][1]).any() and all((c["valid"][1] & c["valid"][k]).sum() >= 100 for k in range(2, 6))
    R, t, X = rb.perturbed_start(c, rb.START_SEED["mixed6"])
    spread = rb.order_spread(prob, R, t, X, 1e-3)
    cond = np.linalg.cond(rb.linearize(prob, R, t, X, 1e-3)["S"])
    out = rb.lm(prob, R, t, X, ftol=rb.LOOP_FTOL)
    same = rb.Problem(prob.pt, prob.cam, prob.uv, np.stack([prob.K[0]] * 6), np.stack([prob.dist[0]] * 6), prob.N)
    ratio = rb.cost_of(same, R, t, X)[0] / out["cost_initial"]
    print("mixed6 spread", spread, "cond(S)", cond, "rho", out["rho"], "iterations", out["iterations"], "rms", rms(prob, out["cost"]),
          "start cost with camera 0's K and lens for all / true", ratio)
    assert all(v > 0 for v in spread.values()) and cond < 1e6
    assert (np.abs(out["rho"]) >= 1e-3).all() and out["status"] == rb.STOP_FTOL and out["history"][:, 2].all()
    assert rms(prob, out["cost"]) < c["sigma"]
    assert ratio > 10
    c = rb.case("mixed6_clean")
    out = rb.lm(c["prob"], *rb.perturbed_start(c, rb.START_SEED["mixed6_clean"]))
    e = aligned_errors(c["scene"], c["X"], out["R"], out["t"])
    print("mixed6_clean rms", rms(c["prob"], out["cost"]), "rotation error", e[0], "centre error", e[1], "iterations", out["iterations"],
          "status", out["status"])
    assert not (c["valid"][0] & c["valid"][1]).any()
    assert rms(c["prob"], out["cost"]) < 1e-9 and e[0] < 1e-12 and e[1] < 1e-11


def test_restatement_refuses_a_start_behind_the_cameras():
    c = rb.case("noisy6", 60)
    R, t, X = rb.perturbed_start(c, 5)
    assert rb.cost_of(c["prob"], R, t, X)[1]
    with pytest.raises(ValueError):
        rb.lm(c["prob"], *rb.mirrored(R, t, X))


# ---- host helpers -------------------------------------------------------------------------------------------------------------
def test_undistort_points_inverts_the_brown_model():
    from mocapv2_amd import calibrate as cal, synth
    scene = synth.Scene(2, dist=synth.MILD_DIST)
    X = np.random.default_rng(3).uniform(-0.8, 0.8, (200, 3))
    dist = synth.project(X, scene.poses[1], scene.K, scene.dist)
    pin = synth.project(X, scene.poses[1], scene.K, synth.ZERO_DIST)
    und = cal.undistort_points(dist, scene.K, scene.dist)
    print("largest error after 5 rounds (px):", np.abs(und - pin).max(), "distortion itself:", np.abs(dist - pin).max())
    assert und.shape == dist.shape and np.abs(und - pin).max() < 1e-3 < np.abs(dist - pin).max()
    nrm = cal.undistort_points(dist, scene.K, scene.dist, normalized=True)
    assert np.abs(nrm[:, 0] * scene.K[0, 0] + scene.K[0, 2] - und[:, 0]).max() < 1e-9
    assert np.abs(cal.undistort_points(dist, scene.K, synth.ZERO_DIST) - dist).max() < 1e-9
    for name in ("undistort_points", "rig_initial_poses", "bundle_adjust_rig", "calibrate_rig"):
        assert name in cal.__all__


def test_rig_functions_check_their_arguments():
    from mocapv2_amd import calibrate as cal
    params = [{"intrinsic_matrix": np.eye(3).tolist(), "distortion_coef": [0, 0, 0, 0, 0]}] * 3
    with pytest.raises(ValueError):
        cal.rig_initial_poses(np.zeros((3, 20)), None, params)
    with pytest.raises(ValueError):
        cal.rig_initial_poses(np.zeros((4, 20, 2)), None, params)  # four cameras, three sets of parameters
    with pytest.raises(ValueError):
        cal.bundle_adjust_rig(np.zeros((3, 20, 2)), None, [{"R": np.eye(3), "t": np.zeros(3)}] * 2, params)
    with pytest.raises(ValueError):
        cal.bundle_adjust_rig(np.full((3, 20, 2), np.nan), None, [{"R": np.eye(3), "t": np.zeros(3)}] * 3, params)


# ---- the C-ABI ------------------------------------------------------------------------------------------------------------------
def test_header_signatures_and_library_export_both_entry_points():
    from mocapv2_amd import _abi
    header = open(os.path.join(ROOT, "include", "mocap_hip.h")).read()
    lib = _abi.load()
    for name, n_args in (("mocap_rig_bundle_adjust", 15), ("mocap_rig_linearize", 16)):
        decl = re.search(r"MOCAP_API int %s\((.*?)\);" % name, header, re.S)
        assert decl and len(decl.group(1).split(",")) == n_args == len(_abi.SIGNATURES[name])
        assert getattr(lib, name).argtypes == _abi.SIGNATURES[name]
    new_part = header.split("MOCAP_API int mocap_fundamental_ransac(")[1].split("MOCAP_API int mocap_rig_linearize(")[0]
    assert new_part.count("lib/Helpers.py:158-176") >= 2  # each entry's comment cites the interface it generalises
    # purely additive: the version the other tests pin
    assert "#define MOCAP_ABI_VERSION 7" in header and _abi.ABI_VERSION == 7 and lib.mocap_abi_version() == 7
    for code in ("MOCAP_RIG_STOP_MAX_ITERS = 1", "MOCAP_RIG_STOP_FTOL = 2", "MOCAP_RIG_STOP_LAMBDA = 3", "MOCAP_RIG_STOP_CHOLESKY = 4",
                 "MOCAP_RIG_E_LAYOUT = -2", "MOCAP_RIG_E_BEHIND = -3"):
        assert code in header
    assert (rb.STOP_MAX_ITERS, rb.STOP_FTOL, rb.STOP_LAMBDA, rb.STOP_CHOLESKY) == (1, 2, 3, 4)


def test_a_null_context_gives_minus_one_and_a_text():
    from mocapv2_amd import _abi
    lib = _abi.load()
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.mocap_rig_bundle_adjust(None, 2, 4, 8, p, p, p, p, p, 5, 1e-12, 1e-3, p, p, None) == -1
    assert b"null" in lib.mocap_last_error()
    assert lib.mocap_rig_linearize(None, 2, 4, 8, p, p, p, p, p, 1e-3, p, p, p, p, p, None) == -1
    assert b"null" in lib.mocap_last_error()


def test_without_a_gpu_the_python_surface_fails_loudly():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from mocapv2_amd import calibrate as cal
    c = rb.case("noisy6", 40)
    with pytest.raises(RuntimeError):
        cal.calibrate_rig(c["image_points"], c["valid"], c["scene"].camera_params)


@pytest.mark.parametrize("src, stems", [
    ("rig_ba.hip", ("rig_init", "rig_linearize", "rig_schur", "rig_reduce", "rig_solve", "rig_update", "rig_decide", "rig_finish",
                    "rig_residuals")),
    ("intrinsics.hip", ("intr_begin", "intr_homography", "intr_start", "intr_linearize", "intr_solve", "intr_update", "intr_decide",
                        "intr_finish"))], ids=["rig_ba", "intrinsics"])
def test_new_kernels_use_no_scratch_memory_and_spill_nothing(src, stems):
    """The compiler's own metadata for the two solver files (scratch/kernel_meta.py, no GPU needed): 0 bytes of scratch and 0
    spilled VGPRs for every kernel; the LDS (the rig's Cholesky is the largest) stays under 64 KB."""
    spec = importlib.util.spec_from_file_location("kernel_meta", os.path.join(ROOT, "scratch", "kernel_meta.py"))
    km = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(km)
    ks = km.kernels_of(os.path.join(km.CSRC, src))
    names = " ".join(k["name"] for k in ks)
    for want in stems:
        assert want + "_kernel" in names
    for k in ks:
        print(k)
        assert k["scratch"] == 0 and k["spill"] == 0 and k["lds"] <= 65536, k
