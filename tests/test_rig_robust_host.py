"""Robust rig bundle adjustment, the part that needs no GPU: the NumPy restatement of the Cauchy-weighted loop
(tests/rig_robust_ref.py) meets every bar of tests/test_gpu_rig_robust.py on its own, and the conditions those GPU comparisons
rest on hold; the C-ABI surface of the two new entry points; the keyword checks of the Python surface; the code objects."""
import ctypes
import importlib.util
import inspect
import os
import re

import numpy as np
import pytest

import rig_ba_ref as rb
import rig_robust_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALE = 2.0  # c in px: 4 sigma of noisy6
SIZES = (400, 96)


def aligned_errors(scene, X_true, R, t):
    """(largest rotation error, largest camera-centre error) of a state with camera 0 at the origin against the scene"""
    Rt, tt, _ = rb.truth_in_camera0(scene, X_true)
    s = np.linalg.norm(tt[1]) / np.linalg.norm(t[1])
    return (max(float(np.linalg.norm(R[c] @ Rt[c].T - np.eye(3)) / np.sqrt(2)) for c in range(len(R))),
            max(float(np.linalg.norm(-R[c].T @ t[c] * s + Rt[c].T @ tt[c])) for c in range(len(R))))


_runs = {}


def run(n):
    """The dirty case of n requested points, its perturbed start and the restatement's robust loop from it, computed once"""
    if n not in _runs:
        case = rb.case("noisy6", n)
        d = rr.dirty(case)
        start = rb.perturbed_start(case, rb.START_SEED["noisy6"])
        _runs[n] = (d, start, rr.lm(d["prob"], *start, SCALE, ftol=rb.LOOP_FTOL))
    return _runs[n]


def planted_mask(d):
    m = np.zeros(len(d["prob"].pt), bool)
    m[d["planted_obs"]] = True
    return m


# ---- the data ---------------------------------------------------------------------------------------------------------------------
def test_dirty_is_the_recipe_of_the_definition():
    for n, (points, obs, bad) in zip(SIZES, ((396, 1656, 82), (95, 423, 21))):
        d = run(n)[0]
        prob, clean = d["prob"], d["clean_prob"]
        assert (prob.N, len(prob.pt), len(d["planted_obs"])) == (points, obs, bad)
        moved = np.linalg.norm(prob.uv - clean.uv, axis=1)
        assert np.array_equal(np.flatnonzero(moved > 0), d["planted_obs"])
        assert moved[d["planted_obs"]].min() >= 20 - 1e-9 and moved[d["planted_obs"]].max() <= 80 + 1e-9
        assert (np.bincount(prob.pt)[prob.pt[d["planted_obs"]]] >= 3).all()
        # the [C][N] arrays say the same as the observation list
        assert int(d["planted"].sum()) == bad and np.array_equal(d["valid"], rb.case("noisy6", n)["valid"])
        again = rb.problem_from_arrays(d["image_points"], d["valid"], d["scene"].camera_params).sorted()
        assert np.array_equal(again.uv, prob.uv) and np.array_equal(again.cam, prob.cam)
        assert np.array_equal(rr.dirty(rb.case("noisy6", n))["prob"].uv, prob.uv)  # seeded


# ---- the restatement --------------------------------------------------------------------------------------------------------------
def test_weighted_gradient_is_the_derivative_of_half_sum_rho():
    """Every camera parameter and 30 point coordinates, central differences of 1/2 sum rho with step 1e-6 in the local
    perturbation, on the dirty 96-point case (outliers with weights down to 1e-3 are in it).  Measured: largest difference
    3e-8 of the largest gradient entry."""
    d, (R, t, X), _ = run(96)
    prob = d["prob"]
    lin = rr.linearize(prob, R, t, X, 1e-3, SCALE)
    D, h = prob.D, 1e-6
    cost = lambda dc, dp: rr.cost_of(prob, *rb.apply_step(prob, R, t, X, dc, dp), SCALE)[0]
    cols = list(range(D)) + list(range(D, D + 3 * prob.N, 3 * prob.N // 30))
    num = np.zeros(len(cols))
    for i, k in enumerate(cols):
        e = np.zeros(D + 3 * prob.N)
        e[k] = h
        num[i] = (cost(e[:D], e[D:].reshape(-1, 3)) - cost(-e[:D], -e[D:].reshape(-1, 3))) / (2 * h)
    worst = np.abs(num - lin["gradient"][cols]).max() / np.abs(lin["gradient"]).max()
    print("gradient of 1/2 sum rho against central differences:", worst)
    assert worst < 1e-6
    assert abs(lin["cost"] - 0.5 * np.sum(rr.rho(rr.weights(rb.observe(prob, R, t, X)[0], SCALE)[0], SCALE))) == 0.0
    assert rb.observe is rr._plain_observe  # the restatement leaves rig_ba_ref as it found it


@pytest.mark.parametrize("n", SIZES)
def test_loop_is_far_from_every_decision_boundary_and_flags_the_planted_set(n):
    """What the GPU loop test and the flag tests stand on (c = 2 px, ftol = LOOP_FTOL = 1e-9).  Measured, 400 / 96 points: 12 / 9
    iterations, all accepted, status ftol; smallest rho 1.26 / 1.16; the stopping step lowers the cost by 2.7e-10 / 7.5e-10 of
    itself and the one before by 1.9e-9 / 6.4e-9 (ftol 1e-9); cond(S) 2.1e4; inlier weights >= 0.546 / 0.629, outlier weights
    <= 0.042 / 0.0069, so the flags (weight < 0.25) are exactly the planted observations and stay so under any relative
    change of a weight below a factor 2."""
    d, (R, t, X), out = run(n)
    prob = d["prob"]
    costs = np.r_[out["cost_initial"], out["history"][:, 0]]
    rel = (costs[:-1] - costs[1:]) / costs[:-1]
    planted = planted_mask(d)
    cond = np.linalg.cond(rr.linearize(prob, R, t, X, 1e-3, SCALE)["S"])
    print(n, "iterations", out["iterations"], "status", out["status"], "rho", out["rho"], "relative decrease", rel, "cond(S)", cond)
    print(n, "inlier weights >=", out["w"][~planted].min(), "outlier weights <=", out["w"][planted].max())
    assert (np.abs(out["rho"]) >= 1e-3).all() and out["history"][:, 2].all()
    assert out["status"] == rb.STOP_FTOL and out["iterations"] == (12 if n == 400 else 9)
    assert ((rel > 1.2 * rb.LOOP_FTOL) | (rel < rb.LOOP_FTOL / 1.2)).all()
    assert cond < 1e6
    assert np.array_equal(rr.flags(out["w"]), planted)
    assert out["w"][~planted].min() > 0.5 and out["w"][planted].max() < 0.125
    # err and w are those of the returned state
    err, w = rr.errors_and_weights(prob, out["R"], out["t"], out["X"], SCALE)
    assert np.array_equal(err, out["err"]) and np.array_equal(w, out["w"])
    assert abs(rr.cost_of(prob, out["R"], out["t"], out["X"], SCALE)[0] / out["cost"] - 1) < 1e-12


@pytest.mark.parametrize("n", SIZES)
def test_robust_loop_and_refit_bring_the_dirty_run_back_to_the_clean_figures(n):
    """Measured, 400 / 96 points (rotation error, centre error): plain loop on dirty data 6.3e-3, 3.8e-2 / 2.3e-2, 7.0e-2; on
    clean data 6.6e-4, 2.6e-3 / 1.0e-3, 5.5e-3; Cauchy on dirty data 6.1e-4, 2.0e-3 / 1.3e-3, 7.0e-3; its refit 6.7e-4, 2.3e-3
    / 1.3e-3, 6.7e-3.  The refit (plain loop over the observations not flagged, from the robust result) ends at the minimum
    the plain loop finds from the perturbed start on the problem without the planted observations: 4e-15 / 1e-14 relative."""
    d, (R, t, X), out = run(n)
    prob, scene, Xt = d["prob"], d["scene"], d["X"]
    plain = rb.lm(prob, R, t, X, ftol=rb.LOOP_FTOL)
    clean = rb.lm(d["clean_prob"], R, t, X, ftol=rb.LOOP_FTOL)
    sub, kept = rr.without(prob, np.flatnonzero(rr.flags(out["w"])))
    print(n, "points that keep two views", len(kept), "of", prob.N)
    refit = rb.lm(sub, out["R"], out["t"], out["X"][kept])
    direct = rb.lm(rr.without(prob, d["planted_obs"])[0], R, t, X[kept])
    e = {k: aligned_errors(scene, Xt, v["R"], v["t"]) for k, v in (("plain", plain), ("clean", clean), ("robust", out), ("refit", refit))}
    print(n, e, "refit / direct - 1", refit["cost"] / direct["cost"] - 1)
    assert abs(refit["cost"] / direct["cost"] - 1) <= 1e-9
    for k in ("robust", "refit"):
        assert e[k][0] < 0.5 * e["plain"][0] and e[k][1] < 0.5 * e["plain"][1]
        assert e[k][0] < 2 * e["clean"][0] and e[k][1] < 2 * e["clean"][1]
    assert e["plain"][0] > 5 * e["clean"][0] and e["plain"][1] > 5 * e["clean"][1]  # the damage the loss is for


def test_from_triangulated_start_points_the_flags_are_nearly_the_planted_set():
    """calibrate_rig triangulates its start points over the outliers too.  The restatement from the perturbed poses with DLT
    points of the dirty observations (400 points): 80 of the 82 planted observations flagged and 1 of 1574 inliers (a 3-view
    point whose two wrong-side views agree loses a good view in place of the bad one); the GPU test's caps are >= 90 % and
    <= 2 %."""
    d, (R, t, _), _ = run(400)
    prob = d["prob"]
    out = rr.lm(prob, R, t, rb.triangulate_dlt(prob, R, t), SCALE)
    planted, flagged = planted_mask(d), rr.flags(out["w"])
    e = aligned_errors(d["scene"], d["X"], out["R"], out["t"])
    print("flagged", int((flagged & planted).sum()), "of", int(planted.sum()), "planted;", int((flagged & ~planted).sum()), "of",
          int((~planted).sum()), "inliers; errors", e, "iterations", out["iterations"], "status", out["status"])
    assert (flagged & planted).sum() >= 0.9 * planted.sum() and (flagged & ~planted).sum() <= 0.02 * (~planted).sum()
    assert out["status"] > 0


def test_clean_data_under_the_loss_flags_nothing():
    """noisy6 as it is (sigma 0.5, no outliers), c = 2: no weight below 0.25 (smallest measured 0.54) and pose errors within
    10 % of the plain loop's."""
    case = rb.case("noisy6")
    R, t, X = rb.perturbed_start(case, rb.START_SEED["noisy6"])
    out = rr.lm(case["prob"], R, t, X, SCALE)
    plain = rb.lm(case["prob"], R, t, X)
    e, p = aligned_errors(case["scene"], case["X"], out["R"], out["t"]), aligned_errors(case["scene"], case["X"], plain["R"], plain["t"])
    print("smallest weight", out["w"].min(), "errors", e, "plain", p)
    assert not rr.flags(out["w"]).any()
    assert e[0] <= 1.1 * p[0] and e[1] <= 1.1 * p[1]


# ---- the C-ABI --------------------------------------------------------------------------------------------------------------------
def test_header_signatures_and_library_export_the_robust_entry_points():
    from mocapv2_amd import _abi
    header = open(os.path.join(ROOT, "include", "mocap_hip.h")).read()
    lib = _abi.load()
    for name, n_args in (("mocap_rig_bundle_adjust_robust", 19), ("mocap_rig_linearize_robust", 18)):
        decl = re.search(r"MOCAP_API int %s\((.*?)\);" % name, header, re.S)
        plain = re.search(r"MOCAP_API int %s\((.*?)\);" % name[:-len("_robust")], header, re.S)
        args, before = [a.strip() for a in decl.group(1).split(",")], [a.strip() for a in plain.group(1).split(",")]
        assert len(args) == n_args == len(_abi.SIGNATURES[name])
        assert getattr(lib, name).argtypes == _abi.SIGNATURES[name]
        # the plain entry's arguments, then the new ones, then the stream
        assert args[:len(before) - 1] == before[:-1] and args[-1] == before[-1] == "void* stream"
        assert args[len(before) - 1:len(before) + 1] == ["int loss", "double loss_scale"]
        assert _abi.SIGNATURES[name][:len(before) - 1] == _abi.SIGNATURES[name[:-len("_robust")]][:-1]
    assert "double* obs_err_dev" in header and "double* obs_weight_dev" in header
    assert "MOCAP_RIG_LOSS_NONE = 0" in header and "MOCAP_RIG_LOSS_CAUCHY = 1" in header
    assert "#define MOCAP_ABI_VERSION 7" in header and _abi.ABI_VERSION == 7 and lib.mocap_abi_version() == 7
    from mocapv2_amd import engine
    assert engine.RIG_LOSSES == {"none": 0, "cauchy": 1}


def test_a_null_context_gives_minus_one_and_a_text():
    from mocapv2_amd import _abi
    lib = _abi.load()
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.mocap_rig_bundle_adjust_robust(None, 2, 4, 8, p, p, p, p, p, 5, 1e-12, 1e-3, p, p, 1, 2.0, p, p, None) == -1
    assert b"null" in lib.mocap_last_error()
    assert lib.mocap_rig_linearize_robust(None, 2, 4, 8, p, p, p, p, p, 1e-3, p, p, p, p, p, 1, 2.0, None) == -1
    assert b"null" in lib.mocap_last_error()


# ---- the Python surface -------------------------------------------------------------------------------------------------------------
def test_keywords_are_appended_and_default_to_todays_behaviour():
    from mocapv2_amd import calibrate as cal, engine
    for fn, before in ((cal.bundle_adjust_rig, ["image_points", "valid", "poses", "camera_params", "points", "max_iters", "ftol", "ctx"]),
                       (cal.calibrate_rig, ["image_points", "valid", "camera_params", "threshold", "hypotheses", "seed", "max_iters",
                                            "ftol", "ctx"])):
        p = inspect.signature(fn).parameters
        assert list(p) == before + ["loss", "loss_scale", "inlier_weight", "refit"]
        assert (p["loss"].default, p["loss_scale"].default, p["inlier_weight"].default, p["refit"].default) == (None, None, 0.25, True)
        assert "a few sigma; 2 px for sigma 0.5 was what the tests use" in " ".join(cal.bundle_adjust_rig.__doc__.split())
    for fn, before in ((engine.MocapContext.rig_bundle_adjust, ["self", "obs_offset", "obs_cam", "obs_uv", "poses", "points", "max_iters",
                                                                "ftol", "lambda0"]),
                       (engine.MocapContext.rig_linearize, ["self", "obs_offset", "obs_cam", "obs_uv", "poses", "points", "lam"])):
        p = inspect.signature(fn).parameters
        assert list(p) == before + ["loss", "loss_scale"] and p["loss"].default is None and p["loss_scale"].default is None


def test_cauchy_without_a_usable_scale_is_a_value_error_before_any_gpu_work():
    from mocapv2_amd import calibrate as cal
    c = rb.case("noisy6", 40)
    R, t, _ = rb.truth_in_camera0(c["scene"], c["X"])
    poses = [{"R": R[k], "t": t[k]} for k in range(len(R))]
    for kw in ({"loss": "cauchy"}, {"loss": "cauchy", "loss_scale": 0.0}, {"loss": "cauchy", "loss_scale": float("nan")},
               {"loss": "cauchy", "loss_scale": float("inf")}, {"loss": "cauchy", "loss_scale": -2.0}, {"loss": "huber", "loss_scale": 2.0},
               {"loss": "cauchy", "loss_scale": 2.0, "inlier_weight": 1.5}):
        with pytest.raises(ValueError):
            cal.bundle_adjust_rig(c["image_points"], c["valid"], poses, c["scene"].camera_params, **kw)
        with pytest.raises(ValueError):
            cal.calibrate_rig(c["image_points"], c["valid"], c["scene"].camera_params, **kw)


# ---- the code objects -------------------------------------------------------------------------------------------------------------
def test_every_instantiation_of_the_point_kernels_is_built_without_scratch():
    """The compiler's metadata (scratch/kernel_meta.py, no GPU needed): linearize, update and the per-observation kernel exist
    for both losses; none uses scratch memory or spills, and the loss costs registers only where it is compiled in (124 / 140
    VGPRs for the linearisation, 78 / 88 for the update: profiles/r12_code_objects.md; 124 and 78 were the plain kernels')."""
    spec = importlib.util.spec_from_file_location("kernel_meta", os.path.join(ROOT, "scratch", "kernel_meta.py"))
    km = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(km)
    ks = {k["name"]: k for k in km.kernels_of(os.path.join(km.CSRC, "rig_ba.hip"))}
    found = {}
    for stem in ("rig_linearize_kernel", "rig_update_kernel", "rig_residuals_kernel"):
        for loss in (0, 1):
            hit = [k for name, k in ks.items() if stem + "I" in name and "ELi%dEE" % loss in name]  # <the camera block, loss>
            assert len(hit) == 1, (stem, loss, sorted(ks))
            print(hit[0])
            assert hit[0]["scratch"] == 0 and hit[0]["spill"] == 0 and hit[0]["agpr"] == 0
            found[stem, loss] = hit[0]
    for stem in ("rig_linearize_kernel", "rig_update_kernel"):
        assert found[stem, 0]["vgpr"] <= found[stem, 1]["vgpr"]
