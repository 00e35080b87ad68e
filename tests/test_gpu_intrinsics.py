"""Intrinsic calibration on the GPU (csrc/intrinsics.hip through mocap_intrinsics_linearize / mocap_intrinsics_calibrate and
calibrate.calibrate_intrinsics) against the NumPy restatement of the definition (tests/intrinsics_ref.py) and SciPy.  The
restatement alone meets every bar below on the CPU: tests/test_intrinsics_host.py, which also prints the allowances quoted
here."""
import numpy as np
import pytest

import intrinsics_ref as ir

pytestmark = pytest.mark.gpu

START_SEED = {"clean_mild": 401, "noisy_golden": 402, "noisy_mild": 403}


@pytest.fixture(scope="module")
def ctx():
    from mocapv2_amd.engine import MocapContext
    return MocapContext(1, 1)


def poses12(R, t):
    return np.c_[np.asarray(R, float).reshape(len(R), 9), np.asarray(t, float).reshape(len(R), 3)]


def layout(cams):
    """(view_offset, point_offset, obj_xy, img_uv, image_sizes) of a list of ir.Camera"""
    voff, poff, obj, img = [0], [0], [], []
    for cam in cams:
        for o, u in cam.views:
            obj.append(o), img.append(u)
            poff.append(poff[-1] + len(o))
        voff.append(voff[-1] + len(cam.views))
    return voff, poff, np.concatenate(obj), np.concatenate(img), [cam.size for cam in cams]


def run(ctx, cams, starts=None, **kw):
    """ctx.intrinsics_calibrate on a list of cameras; starts: per camera (kd, R, t), or None for the library's own"""
    start = None if starts is None else (np.array([s[0] for s in starts]), np.concatenate([poses12(s[1], s[2]) for s in starts]))
    return ctx.intrinsics_calibrate(*layout(cams), start, **kw)


def camera_of(out, cams, c):
    """camera c's share of every output, as bytes-comparable arrays"""
    v0 = sum(len(cam.views) for cam in cams[:c])
    v1 = v0 + len(cams[c].views)
    return {"kd": out["kd"][c], "poses": out["poses"][v0:v1], "view_rms": out["view_rms"][v0:v1], "history": out["history"][c],
            "result": np.array([out["status"][c], out["iterations"][c], out["cost_initial"][c], out["cost"][c]], float)}


def same_bytes(a, b, keys=("kd", "poses", "view_rms", "history", "result")):
    for k in keys:
        assert a[k].tobytes() == b[k].tobytes(), k


_memo = {}


def restatement_start(name):
    if name not in _memo:
        _memo[name] = ir.initialise(ir.case(name)["cam"])
    return _memo[name]


# ---- 1. pieces ------------------------------------------------------------------------------------------------------------------
def test_pieces_agree_with_the_restatement(ctx):
    """mocap_intrinsics_linearize on rig3 (clean_mild, noisy_golden, noisy_mild in one call: 3 + 12 + 8 views of 54, 99 and 35
    points) at the perturbed starts, lambda = 1e-3: cost, gradient, S and reduced right-hand side of every camera against the
    restatement, each relative to its largest entry of that camera.  Kernels and restatement form every per-point term and
    the small factorisations by the same operations; they differ in the order of the sums at most.  The allowance is 8 x the
    restatement's own largest spread under 10 seeded permutations of the points within the views and of the views.
    Restatement's spread (CPU):  clean_mild    cost 4.3e-16  gradient 4.7e-16  S 1.1e-13  rhs 2.5e-12
                                 noisy_golden  cost 3.9e-16  gradient 9.7e-16  S 1.5e-14  rhs 3.8e-13
                                 noisy_mild    cost 3.3e-16  gradient 4.1e-16  S 2.6e-14  rhs 8.1e-13
    GPU - restatement (MI355X):  0 for all twelve (the same bits: the kernels' sums run in the restatement's order)"""
    cases = [ir.case(n) for n in ir.RIG3]
    cams = [c["cam"] for c in cases]
    starts = [ir.perturbed_start(c, START_SEED[c["name"]]) for c in cases]
    voff, poff, obj, img, _ = layout(cams)
    got = ctx.intrinsics_linearize(voff, poff, obj, img, np.array([s[0] for s in starts]),
                                   np.concatenate([poses12(s[1], s[2]) for s in starts]), 1e-3)
    assert not got["layout"].any() and not got["behind"].any()
    for c, (case, (kd, R, t)) in enumerate(zip(cases, starts)):
        spread = ir.order_spread(case["cam"], kd, R, t, 1e-3)
        ref = ir.linearize(case["cam"], kd, R, t, 1e-3)
        mine = {"cost": got["cost"][c], "S": got["S"][c], "rhs": got["rhs"][c],
                "gradient": np.r_[got["gradient"][9 * c:9 * c + 9], got["gradient"][9 * len(cams) + 6 * voff[c]:9 * len(cams) + 6 * voff[c + 1]]]}
        diffs = {}
        for k in ("cost", "gradient", "S", "rhs"):
            a, b = np.asarray(ref[k], float), np.asarray(mine[k], float)
            diffs[k] = float(np.abs(a - b).max() / np.abs(a).max())
            print(f"{case['name']} {k}: restatement's spread {spread[k]:.3e}  GPU - restatement {diffs[k]:.3e}  allowed {8 * spread[k]:.3e}")
        for k in diffs:
            assert spread[k] > 0 and diffs[k] <= 8 * spread[k], (case["name"], k)
        assert np.array_equal(got["S"][c], got["S"][c].T)


# ---- 2. loop --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["noisy_mild", "noisy_golden"])
def test_loop_walks_the_restatements_iterations(ctx, name):
    """From the restatement's initialisation (handed in as the start, so both sides begin at the same bits), ftol = 1e-9: the
    same accept / reject sequence, the same number of iterations, the same stopping rule.  The condition is asserted, not
    assumed: no iteration of the restatement has |rho| < 1e-3, and 10 permuted restatement runs all take the same decisions.
    Per-iteration cost: allowed relative difference 8 x the largest relative spread of the restatement's per-iteration cost
    over those runs.
    Restatement's spread (CPU):  noisy_mild 7.8e-14 (11 iterations)   noisy_golden 1.6e-11 (13 iterations)
    GPU - restatement (MI355X):  noisy_mild 0 in all 11 iterations   noisy_golden at most 2.2e-16 in 13"""
    c = ir.case(name)
    kd, R, t = restatement_start(name)
    ref, same, spread = ir.loop_spread(c["cam"], kd, R, t)
    assert same and (np.abs(ref["rho"]) >= 1e-3).all(), ref["rho"]
    got = camera_of(run(ctx, [c["cam"]], [(kd, R, t)], ftol=ir.LOOP_FTOL), [c["cam"]], 0)
    h = got["history"]
    print(f"{name}: iterations {len(h)} / {ref['iterations']}  status {got['result'][0]} / {ref['status']}")
    assert len(h) == ref["iterations"] == got["result"][1] and got["result"][0] == ref["status"] == ir.STOP_FTOL
    rel = np.abs(h[:, 0] / ref["history"][:, 0] - 1)
    print("accepted", h[:, 2], "cost, relative difference per iteration", rel, "largest", rel.max(), "allowed", 8 * spread)
    assert np.array_equal(h[:, 2], ref["history"][:, 2])
    assert spread > 0 and (rel <= 8 * spread).all()
    assert np.abs(h[:, 1] / ref["history"][:, 1] - 1).max() < 1e-6  # the damping follows rho
    assert np.abs(h[:, 3] / ref["history"][:, 3] - 1).max() < 1e-6  # and the steps have the same length
    assert abs(got["result"][2] / ref["cost_initial"] - 1) < 1e-12


# ---- 3. clean recovery ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["clean_mild", "clean_golden"])
def test_clean_views_give_the_lens_back(ctx, name):
    """Exact pixels, the library's own initialisation: status > 0, and the errors of fx, fy, cx, cy (relative) and of the five
    coefficients (absolute) against the truth are at most 10 x those of the restatement run from the same initialisation (the
    definition's, restated).
    Restatement (CPU):  clean_mild    K 2.1e-14, coefficients 2.7e-13 (37 iterations, status lambda)
                        clean_golden  K 5.4e-15, coefficients 3.2e-12 (36 iterations, status lambda)
    GPU (MI355X):       clean_mild    K 1.5e-14, coefficients 1.2e-13 (32 iterations, status lambda)
                        clean_golden  K 7.1e-15, coefficients 8.5e-13 (45 iterations, status lambda)"""
    from mocapv2_amd import calibrate as cal
    c = ir.case(name)
    out = cal.calibrate_intrinsics([c["cam"].views], c["cam"].size, ctx=ctx)[0]
    ref = ir.lm(c["cam"], *restatement_start(name))
    K, d = out["intrinsic_matrix"], out["distortion_coef"]
    e_gpu = ir.param_errors(np.r_[K[0, 0], K[1, 1], K[0, 2], K[1, 2], d], c["kd"])
    e_ref = ir.param_errors(ref["kd"], c["kd"])
    print(f"{name}: GPU K {e_gpu[0]:.3e} coefficients {e_gpu[1]:.3e} rms {out['rms_px']:.3e} ({out['iterations']} iterations, status {out['status']}); "
          f"restatement K {e_ref[0]:.3e} coefficients {e_ref[1]:.3e} rms {ref['rms_px']:.3e} ({ref['iterations']}, {ref['status']})")
    assert out["status"] > 0
    assert e_gpu[0] <= 10 * e_ref[0] and e_gpu[1] <= 10 * e_ref[1]


# ---- 4. noise -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["noisy_mild", "noisy_golden"])
def test_noisy_views_reach_scipys_minimum(ctx, name):
    """sigma = 0.3 px, the library's own initialisation.  Bars: rms_px < sigma sqrt(2); the cost is within 1e-6 of the minimum
    SciPy's least_squares (x_scale='jac') finds on the restatement's residual from the same start.  No bar on the recovered
    coefficients: k2 and k3 are poorly determined under noise.
    Measured on the MI355X: noisy_mild rms 0.39256 px from 2.433 at the start, cost / SciPy's - 1 = 4.5e-14, 12 iterations;
    noisy_golden rms 0.41281 from 3.857, 9.3e-15, 14 iterations."""
    from mocapv2_amd import calibrate as cal
    c = ir.case(name)
    out = cal.calibrate_intrinsics([c["cam"].views], c["cam"].size, ctx=ctx)[0]
    ref = ir.scipy_minimum(c["cam"], *restatement_start(name))[0]
    print(f"{name}: rms {out['rms_px']:.5f} px (start {np.sqrt(2 * out['cost_initial'] / c['cam'].n_points):.3f})  cost / SciPy's - 1 "
          f"{out['cost'] / ref - 1:.3e}  iterations {out['iterations']} status {out['status']}")
    assert out["status"] > 0 and out["rms_px"] < c["sigma"] * np.sqrt(2)
    assert abs(out["cost"] / ref - 1) <= 1e-6


# ---- 5. views -------------------------------------------------------------------------------------------------------------------
def test_view_rms_adds_up_and_points_at_the_bad_view(ctx):
    """sum n_v view_rms_v^2 = 2 cost to 1e-12.  noisy_mild with the points of view 5 shifted by 5 px, each point in its own
    seeded direction (ir.with_a_bad_view): that view has the largest view_rms.  (Shifted all in one direction the view is a
    board moved sideways, which its pose takes up: library and restatement then both leave its rms at 0.375 px, below view
    1's; test_intrinsics_host.py::test_a_badly_found_view_has_the_largest_view_rms.)"""
    from mocapv2_amd import calibrate as cal
    c = ir.case("noisy_mild")
    cam = c["cam"]
    n = np.array([len(o) for o, _ in cam.views])
    out = cal.calibrate_intrinsics([cam.views], cam.size, ctx=ctx)[0]
    assert abs(np.sum(n * out["view_rms"] ** 2) / (2 * out["cost"]) - 1) <= 1e-12
    assert abs(out["rms_px"] - np.sqrt(2 * out["cost"] / n.sum())) <= 1e-15 * out["rms_px"]
    bad = 5
    shifted = cal.calibrate_intrinsics([ir.with_a_bad_view(cam, bad).views], cam.size, ctx=ctx)[0]
    print("view_rms", out["view_rms"], "with the points of view 5 shifted by 5 px", shifted["view_rms"])
    assert shifted["status"] > 0 and int(np.argmax(shifted["view_rms"])) == bad
    assert abs(np.sum(n * shifted["view_rms"] ** 2) / (2 * shifted["cost"]) - 1) <= 1e-12


# ---- 6. bits, 7. independence -----------------------------------------------------------------------------------------------------
def test_two_runs_give_the_same_bits_also_after_a_larger_call(ctx):
    cams = [ir.case(n)["cam"] for n in ir.RIG3]
    starts = [ir.perturbed_start(ir.case(n), START_SEED[n]) for n in ir.RIG3]
    voff, poff, obj, img, _ = layout(cams)

    def both():
        lin = ctx.intrinsics_linearize(voff, poff, obj, img, np.array([s[0] for s in starts]),
                                       np.concatenate([poses12(s[1], s[2]) for s in starts]), 1e-3)
        return run(ctx, cams), lin

    a, la = both()
    b, lb = both()
    run(ctx, [ir.case("clean_mild")["cam"]] * 32)  # unrelated, larger (32 cameras x 3 views): the scratch grows and is reused
    d, ld = both()
    assert (a["status"] > 0).all()
    for other, lin in ((b, lb), (d, ld)):
        for c in range(3):
            same_bytes(camera_of(a, cams, c), camera_of(other, cams, c))
        for k in ("cost", "gradient", "S", "rhs"):
            assert la[k].tobytes() == lin[k].tobytes(), k


def test_a_camera_gives_the_same_bits_alone_and_in_the_rig(ctx):
    cams = [ir.case(n)["cam"] for n in ir.RIG3]
    rig = run(ctx, cams)
    for c, cam in enumerate(cams):
        same_bytes(camera_of(rig, cams, c), camera_of(run(ctx, [cam]), [cam], 0))


# ---- 8. edges -------------------------------------------------------------------------------------------------------------------
def test_layout_errors(ctx):
    """Python raises ValueError before the call; through the raw engine call the camera reports MOCAP_INTR_E_LAYOUT, its
    arrays untouched, and the camera beside it is calibrated as if alone."""
    from mocapv2_amd import calibrate as cal
    good = ir.case("clean_mild")["cam"]
    alone = camera_of(run(ctx, [good]), [good], 0)
    three = ir.Camera([(o[:3], u[:3]) if v == 1 else (o, u) for v, (o, u) in enumerate(good.views)], good.size)
    two = ir.Camera(good.views[:2], good.size)
    for bad in (three, two):
        with pytest.raises(ValueError, match="camera 1"):
            cal.calibrate_intrinsics([good.views, bad.views], good.size, ctx=ctx)
        out = run(ctx, [good, bad])
        assert out["status"][1] == ir.E_LAYOUT and np.isnan(out["kd"][1]).all() and np.isnan(out["view_rms"][len(good.views):]).all()
        same_bytes(camera_of(out, [good, bad], 0), alone)
        start = ir.perturbed_start(ir.case("clean_mild"), 401)
        nb = len(bad.views)
        lin = ctx.intrinsics_linearize(*layout([good, bad])[:4], np.array([start[0], start[0]]),
                                       np.concatenate([poses12(start[1], start[2]), poses12(start[1][:nb], start[2][:nb])]), 1e-3)
        assert list(lin["layout"]) == [False, True] and lin["cost"][1] == 0 and not lin["S"][1].any() and lin["cost"][0] > 0


def test_fronto_parallel_views_are_degenerate(ctx):
    from mocapv2_amd import calibrate as cal
    good, flat = ir.case("clean_mild")["cam"], ir.fronto_parallel()
    alone = camera_of(run(ctx, [good]), [good], 0)
    out = run(ctx, [flat, good])
    assert out["status"][0] == ir.E_DEGENERATE and out["status"][1] > 0
    assert np.isnan(out["kd"][0]).all() and np.isnan(out["poses"][:len(flat.views)]).all()  # as they were handed in
    same_bytes(camera_of(out, [flat, good], 1), alone)
    res = cal.calibrate_intrinsics([flat.views, good.views], good.size, ctx=ctx)
    assert res[0]["status"] == ir.E_DEGENERATE and res[0]["intrinsic_matrix"] is None and np.isnan(res[0]["rms_px"]) and res[1]["status"] > 0


def test_a_start_behind_the_camera_is_reported(ctx):
    c = ir.case("clean_mild")
    kd, R, t = c["kd"], c["R"], -c["t"]
    out = run(ctx, [c["cam"]], [(kd, R, t)])
    assert out["status"][0] == ir.E_BEHIND and out["iterations"][0] == 0
    assert out["kd"][0].tobytes() == kd.tobytes() and out["poses"].tobytes() == poses12(R, t).tobytes()


def test_a_board_that_is_not_flat_raises(ctx):
    from mocapv2_amd import calibrate as cal
    cam = ir.case("clean_mild")["cam"]
    views = [(np.c_[o, np.full(len(o), 0.01 * (v == 0))], u) for v, (o, u) in enumerate(cam.views)]
    with pytest.raises(ValueError, match="planar"):
        cal.calibrate_intrinsics([views], cam.size, ctx=ctx)
    flat = [(np.c_[o, np.zeros(len(o))], u) for o, u in cam.views]
    assert cal.calibrate_intrinsics([flat], cam.size, ctx=ctx)[0]["status"] > 0


# ---- 9. chain -------------------------------------------------------------------------------------------------------------------
def test_the_entry_feeds_the_rest_of_the_calibration(ctx):
    from mocapv2_amd import calibrate as cal
    c = ir.case("clean_mild")
    entry = cal.calibrate_intrinsics([c["cam"].views], c["cam"].size, ctx=ctx)[0]
    K, d = cal._intrinsics([entry], 2)
    assert K.shape == (2, 3, 3) and d.shape == (2, 5) and abs(K[0, 0, 0] / c["kd"][0] - 1) < 1e-9
    ctx.set_cameras(K, d, np.stack([np.eye(3)] * 2), np.zeros((2, 3)))
    again = cal.calibrate_intrinsics([c["cam"].views], c["cam"].size, start=[(entry, entry["poses"])], ctx=ctx)[0]
    assert again["status"] > 0 and again["rms_px"] < 1e-9
