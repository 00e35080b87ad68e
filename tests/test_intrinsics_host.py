"""The NumPy restatement of the intrinsic calibration (tests/intrinsics_ref.py) alone meets every bar tests/test_gpu_intrinsics.py
and tests/test_gpu_intrinsics_shapes.py set for the GPU, on the CPU; the allowances those files quote are measured and printed
here (pytest -s).  Plus what of the Python surface needs no GPU."""
import json
import os

import numpy as np
import pytest

import intrinsics_ref as ir

NOISY = ("noisy_mild", "noisy_golden")
START_SEED = {"clean_mild": 401, "noisy_golden": 402, "noisy_mild": 403}


def test_analytic_jacobian_against_central_differences():
    """Every one of the 15 columns, on a 99-point view of the golden lens (k3 = 3.76) at a perturbed state.  Steps 1e-6 of
    the parameter's size: truncation ~1e-12 of the entry times the third derivative's growth, rounding ~1e-10; the bar is
    1e-6 of the column's largest entry."""
    c = ir.case("noisy_golden")
    kd, R, t = ir.perturbed_start(c, 402)
    obj, uv = c["cam"].views[1]
    _, J, _ = ir.observe(kd, R[1], t[1], obj, uv)
    for k in range(15):
        def at(h):
            kk, RR, tt = kd.copy(), R[1], t[1].copy()
            if k < 9:
                kk[k] += h
            elif k < 12:
                w = np.zeros(3)
                w[k - 9] = h
                RR = ir.exp_so3_left(w, RR)
            else:
                tt[k - 12] += h
            return ir.observe(kk, RR, tt, obj, uv)[0]
        h = 1e-6 * (max(1.0, abs(kd[k])) if k < 9 else 1.0)
        num = (at(h) - at(-h)) / (2 * h)
        err = np.abs(J[:, :, k] - num).max() / np.abs(J[:, :, k]).max()
        print(f"column {k}: {err:.2e}")
        assert err < 1e-6, k


def test_schur_step_is_the_step_of_the_full_normal_equations():
    c = ir.case("noisy_golden")
    cam = c["cam"]
    kd, R, t = ir.perturbed_start(c, 402)
    lam = 1e-3
    lin = ir.linearize(cam, kd, R, t, lam)
    dc, dp, pred, n2 = ir.schur_step(lin, lam)
    nv = len(cam.views)
    H = np.zeros((9 + 6 * nv, 9 + 6 * nv))
    H[:9, :9] = lin["U"]
    for v in range(nv):
        H[9 + 6 * v:15 + 6 * v, 9 + 6 * v:15 + 6 * v] = lin["V"][v]
        H[:9, 9 + 6 * v:15 + 6 * v] = lin["W"][v]
        H[9 + 6 * v:15 + 6 * v, :9] = lin["W"][v].T
    H[np.diag_indices_from(H)] += lam * np.diag(H)
    d = np.linalg.solve(H, -lin["gradient"])
    ref = np.r_[dc, dp.reshape(-1)]
    assert np.abs(d - ref).max() <= 1e-8 * np.abs(d).max()
    assert pred > 0 and abs(n2 - ref @ ref) <= 1e-12 * n2


@pytest.mark.parametrize("name", list(ir.CASES) + list(ir.SHAPE_CASES))
def test_restatement_from_its_initialisation(name):
    """The initialisation leaves a start from which the loop converges, on every case.  Clean: status > 0 and the truth to
    rounding (printed: test 3 of the GPU file compares with these).  Noisy: rms < sigma sqrt(2); cost within 1e-6 of SciPy's
    minimum from the same start; no bar on the coefficients (k2 and k3 are poorly determined under noise).  sum n_v view_rms_v^2
    = 2 cost.  `small` (30 equations for 27 unknowns): status > 0 and the sum only; with 3 spare equations the lens it finds
    is far from the truth and its rms far below sigma, and nothing is asserted about either.
    Shape cases (CPU):  many_views   start fx 1411.0 (truth 1400), ftol after 12 iterations, rms 0.3840 px, cost / SciPy's - 1 = 0
                        views_64     start fx 1418.9, ftol after 13, rms 0.3823, 1.9e-14
                        views_65     start fx 1436.1, ftol after 12, rms 0.4011, 9.5e-15
                        edge_points  start fx 1411.0, ftol after 14, rms 0.4107, 2.3e-14
                        small        start fx 1338.9, ftol after 45, rms 0.086, K error 0.16, coefficient error 4.2"""
    c = ir.case(name)
    cam = c["cam"]
    kd, R, t = ir.initialise(cam)
    out = ir.lm(cam, kd, R, t)
    rel, coef = ir.param_errors(out["kd"], c["kd"])
    print(f"{name}: start fx {kd[0]:.1f} fy {kd[1]:.1f} rms {np.sqrt(2 * out['cost_initial'] / cam.n_points):.3f} px; {out['iterations']} iterations, "
          f"status {out['status']}, rms {out['rms_px']:.3e} px, K error {rel:.2e}, coefficient error {coef:.2e}")
    assert out["status"] > 0
    n = np.array([len(o) for o, _ in cam.views])
    assert abs(np.sum(n * out["view_rms"] ** 2) / (2 * out["cost"]) - 1) < 1e-12
    if c["sigma"] == 0:
        assert out["rms_px"] < 1e-9 and rel < 1e-9 and coef < 1e-7
    elif name != "small":
        ref = ir.scipy_minimum(cam, kd, R, t)[0]
        print(f"  cost / SciPy's minimum - 1 = {out['cost'] / ref - 1:.2e}")
        assert out["rms_px"] < c["sigma"] * np.sqrt(2)
        assert abs(out["cost"] / ref - 1) <= 1e-6


def test_order_of_the_sums_pieces():
    """What the order of the sums over points and views is worth for the pieces of rig3 at the perturbed starts, lambda = 1e-3:
    the spreads test 1 of the GPU file allows 8 x of (its docstring quotes this output)."""
    for name in ir.RIG3:
        c = ir.case(name)
        s = ir.order_spread(c["cam"], *ir.perturbed_start(c, START_SEED[name]), 1e-3)
        print(name, " ".join(f"{k} {v:.1e}" for k, v in s.items()))
        assert all(0 < v < 1e-9 for v in s.values())


def test_order_of_the_sums_pieces_at_the_shape_cases():
    """The same for edge_points, many_views and small, the spreads test a of tests/test_gpu_intrinsics_shapes.py allows 8 x
    of, plus 2^-52.  A sum of 15 terms (small's cost) can come out the same in every order: its spread may be 0, and one
    differently rounded addition, 2^-52 of the sum, is the least another order can cost.
    Measured:  edge_points  cost 4.0e-16  gradient 5.3e-16  S 1.3e-13  rhs 8.1e-13
               many_views   cost 2.5e-16  gradient 3.7e-16  S 5.9e-14  rhs 4.1e-13
               small        cost 1.4e-16  gradient 3.0e-17  S 1.5e-13  rhs 4.7e-13"""
    for name in ir.SHAPES3:
        c = ir.case(name)
        s = ir.order_spread(c["cam"], *ir.perturbed_start(c, ir.SHAPE_START_SEED[name]), 1e-3)
        print(name, " ".join(f"{k} {v:.1e}" for k, v in s.items()))
        assert all(0 <= v < 1e-9 for v in s.values()) and all(v > 0 for k, v in s.items() if (name, k) != ("small", "cost"))


@pytest.mark.parametrize("name", NOISY + ir.SHAPES3)
def test_loop_cases_are_far_from_every_decision_boundary(name):
    """ftol = 1e-9: no iteration has |rho| < 1e-3, and 10 permuted runs (points within views, views) take the same decisions.
    Prints the largest relative spread of the per-iteration cost over those runs (test 2 of the GPU file, and test b of
    tests/test_gpu_intrinsics_shapes.py, allow 8 x).
    Measured:  noisy_mild 7.8e-14 (11 iterations, smallest |rho| 0.982)   noisy_golden 1.6e-11 (13, 0.638)
               edge_points 6.3e-14 (12, 0.994)   many_views 4.9e-14 (11, 0.983)   small 5.9e-11 (38, 0.503)"""
    c = ir.case(name)
    base, same, spread = ir.loop_spread(c["cam"], *ir.initialise(c["cam"]))
    print(f"{name}: {base['iterations']} iterations, status {base['status']}, min |rho| {np.abs(base['rho']).min():.3f}, cost spread {spread:.2e}")
    assert same and base["status"] == ir.STOP_FTOL and (np.abs(base["rho"]) >= 1e-3).all() and 0 < spread < 1e-8


def test_a_badly_found_view_has_the_largest_view_rms():
    """noisy_mild with the points of view 5 shifted by 5 px, each in its own direction: that view's rms is the largest, and
    close to the shift.  Shifted all in ONE direction they are a board moved sideways: the view's pose takes the shift up and
    its rms stays within a few percent of what it was, so that form of the case cannot single the view out."""
    cam, bad = ir.case("noisy_mild")["cam"], 5
    plain = ir.lm(cam, *ir.initialise(cam))["view_rms"]
    scattered = ir.with_a_bad_view(cam, bad)
    out = ir.lm(scattered, *ir.initialise(scattered))
    rigid = ir.Camera([(o, u + 5.0 * (v == bad)) for v, (o, u) in enumerate(cam.views)], cam.size)
    moved = ir.lm(rigid, *ir.initialise(rigid))["view_rms"]
    print("view_rms", plain, "scattered", out["view_rms"], "one direction", moved)
    assert out["status"] > 0 and int(np.argmax(out["view_rms"])) == bad and 3.0 < out["view_rms"][bad] < 5.0
    assert abs(moved[bad] / plain[bad] - 1) < 0.05


def test_degenerate_views_and_a_board_behind_the_camera():
    with pytest.raises(ir.Degenerate):
        ir.initialise(ir.fronto_parallel())
    c = ir.case("clean_mild")
    R, t = c["R"].copy(), -c["t"]
    assert ir.lm(c["cam"], c["kd"], R, t)["status"] == ir.E_BEHIND


@pytest.mark.parametrize("name", ["many_views", "views_64", "views_65", "edge_points"])
def test_two_routes_to_the_initialisation_give_the_same_start(name):
    """What the route to a homography's null vector is worth for the cost at the start: np.linalg.eigh of A^T A (the
    restatement's) against scipy.linalg.svd of A, and eigh under 10 seeded permutations of the points within the views.
    Test c of tests/test_gpu_intrinsics_shapes.py allows the device's third route, cyclic Jacobi, 8 x the larger.
    Measured (svd / eigh - 1, permuted / given - 1 at most):  many_views 3.6e-14, 9.6e-14   views_64 5.6e-14, 1.3e-13
                                                              views_65 8.9e-16, 8.1e-14   edge_points 2.4e-13, 5.5e-13"""
    svd, perm = ir.start_spread(ir.case(name)["cam"])
    print(f"{name}: cost at the start, svd / eigh - 1 = {svd:.2e}, permuted points / given - 1 at most {perm:.2e}")
    assert 0 < max(svd, perm) < 1e-8


def test_the_ragged_calls_cameras_differ_and_the_failed_ones_fail():
    """What tests d and e of tests/test_gpu_intrinsics_shapes.py build on: the five cameras their calls cycle through differ
    in their layouts, so that a neighbour's state is a wrong state, and each of the failed cameras has in the restatement
    the status it must report."""
    cams = [ir.case(n)["cam"] for n in ir.RAGGED5]
    shapes = [tuple(len(o) for o, _ in cam.views) for cam in cams]
    assert len(set(shapes)) == 5 and sum(len(s) for s in shapes) == 33 and sum(sum(s) for s in shapes) == 2158
    for name, (cam, status) in ir.failed_cameras().items():
        assert ir.status_from_own_start(cam) == status, name


def test_fewer_equations_than_unknowns_fit_a_wrong_lens():
    """Why the layout rule has its third clause.  three_by_four, 3 views of 4 points, is 24 equations for 27 unknowns: the
    damped normal matrix stays positive definite, no solve fails, and the loop fits the noisy pixels exactly.  Run past the
    rule, the restatement reports a positive status and rms 0 for a lens that is not the camera's.  The rule refuses the
    layout, and accepts the two that just suffice: 3 views of 5 points (30 for 27) and 5 views of 4 (40 for 39).
    Measured: cost 82.44 -> 2.3e-26 in 26 iterations, status 3 (lambda), rms 6.1e-14 px; fx 1394.2 for 1400, the K error 1.6e-2
    and k3 = -80.8 for 0.  five_by_four passes the rule and is Degenerate in its initialisation (1 / fx^2 = -3.5e-6)."""
    c = ir.case("three_by_four")
    out = ir.lm(c["cam"], *ir.initialise(c["cam"]))
    rel, coef = ir.param_errors(out["kd"], c["kd"])
    print(f"three_by_four past the rule: cost {out['cost_initial']:.4g} -> {out['cost']:.1e}, status {out['status']}, {out['iterations']} iterations, "
          f"rms {out['rms_px']:.1e} px, fx {out['kd'][0]:.1f} (truth {c['kd'][0]:.1f}), k3 {out['kd'][8]:.3g}, K error {rel:.2e}")
    assert out["status"] > 0 and out["rms_px"] < 1e-6 * c["sigma"] and rel > 0.01
    assert ir.layout_error((4, 4, 4)) is not None and ir.status_from_own_start(c["cam"]) == ir.E_LAYOUT
    for name in ("small", "five_by_four"):
        counts = [len(o) for o, _ in ir.case(name)["cam"].views]
        assert ir.layout_error(counts) is None, name
    assert ir.layout_error((54, 54)) is not None and ir.layout_error((54, 3, 54)) is not None and ir.layout_error(()) is not None
    print("five_by_four from its own start: status", ir.status_from_own_start(ir.case("five_by_four")["cam"]))


def test_the_host_checks_state_the_layout_rule():
    """calibrate_intrinsics refuses 3 views of 4 points naming the camera; 3 views of 5 points and 5 views of 4 pass its checks
    (without a GPU the call then fails for want of one, which is no ValueError)."""
    from mocapv2_amd import calibrate as cal
    good = ir.case("clean_mild")["cam"]
    with pytest.raises(ValueError, match="camera 1: 12 points in 3 views are 24 equations for 27 unknowns"):
        cal.calibrate_intrinsics([good.views, ir.case("three_by_four")["cam"].views], good.size)
    for name in ("small", "five_by_four"):
        try:
            cal.calibrate_intrinsics([good.views, ir.case(name)["cam"].views], good.size)
        except RuntimeError:
            pass


def test_save_intrinsics_round_trips_the_golden_file(tmp_path):
    from mocapv2_amd import calibrate as cal
    with open(os.path.join(ir.GOLDEN, "jsons", "camera-intrinsics.json")) as f:
        golden = json.load(f)
    path = cal.save_intrinsics(golden, str(tmp_path / "camera-intrinsics.json"))
    with open(path) as f:
        again = json.load(f)
    assert again == golden and list(again) == ["intrinsic_matrix", "distortion_coef"]
    K, d = cal._intrinsics([again], 1)
    assert K.shape == (1, 3, 3) and d.shape == (1, 5)


def test_layout_errors_the_host_can_see_raise_and_name_the_camera():
    from mocapv2_amd import calibrate as cal
    good = ir.case("clean_mild")["cam"]
    few_points = [(o[:3], u[:3]) if v == 1 else (o, u) for v, (o, u) in enumerate(good.views)]
    with pytest.raises(ValueError, match="camera 1, view 1"):
        cal.calibrate_intrinsics([good.views, few_points], good.size)
    with pytest.raises(ValueError, match="camera 1"):
        cal.calibrate_intrinsics([good.views, good.views[:2]], good.size)
    bent = [(np.c_[o, np.full(len(o), 1e-3 if v == 2 else 0.0)], u) for v, (o, u) in enumerate(good.views)]
    with pytest.raises(ValueError, match="camera 0, view 2.*planar"):
        cal.calibrate_intrinsics([bent], good.size)


def test_no_gpu_is_an_error_not_a_fallback():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from mocapv2_amd import calibrate as cal
    good = ir.case("clean_mild")["cam"]
    with pytest.raises(RuntimeError):
        cal.calibrate_intrinsics([good.views], good.size)
