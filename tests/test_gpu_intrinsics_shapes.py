"""Intrinsic calibration on the GPU outside the shapes csrc/intrinsics.hip calls typical (3-12 views of 35-99 points, a few
cameras): more than 64 views in a camera, views of 63 to 221 points (LDS chunks of 64 with last chunks of 1, 29, 63 and 64),
the smallest accepted layout, 300 ragged cameras in one call (the finish kernel's second and later workgroups), cameras with
no views and views with no points among them, and the layout rule 2 points >= 9 + 6 views.  The yardstick is the NumPy
restatement (tests/intrinsics_ref.py), which meets every bar below alone on the CPU: tests/test_intrinsics_host.py, which also
prints the allowances quoted here.

Which test reaches which loop of the file:
  intr_start_kernel, v += 64            c (many_views: views 64..69; views_65: one view; views_64: none, the edge)
  intr_begin_kernel, i += 64, v0 > 0    a and b (many_views handed a start; in a it begins at view 7)
  intr_solve_kernel / lm_decide sums    a, b, c (70 terms)
  intr_linearize_kernel chunks          a, b, c (edge_points: 1 to 4 chunks, last chunks of 63, 64, 1, 63, 64, 1, 29)
  homography / update, p += 64          c / b and c (edge_points)
  intr_finish_kernel, blockIdx.x > 0    d and e (1 980 views: 8 workgroups)
  intr_args: empty cameras and views    e
The finish kernel's grid cap (1 024 workgroups, a grid-stride loop beyond) needs more than 262 144 views and is not reached."""
import numpy as np
import pytest

import intrinsics_ref as ir
from test_gpu_intrinsics import camera_of, layout, poses12, run, same_bytes

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
OWN_START = ("many_views", "views_64", "views_65", "edge_points")


@pytest.fixture(scope="module")
def ctx():
    from mocapv2_amd.engine import MocapContext
    return MocapContext(1, 1)


_memo = {}


def memo(key, make):
    if key not in _memo:
        _memo[key] = make()
    return _memo[key]


def restatement_start(name):
    return memo(("start", name), lambda: ir.initialise(ir.case(name)["cam"]))


def alone(ctx, name):
    """the camera's share of every output when it is calibrated alone, from the library's own start"""
    cam = ir.case(name)["cam"]
    return memo(("alone", name), lambda: camera_of(run(ctx, [cam]), [cam], 0))


def linearized(ctx, cams, kd, poses, lam=1e-3):
    voff, poff, obj, img, _ = layout(cams)
    return ctx.intrinsics_linearize(voff, poff, obj, img, kd, poses, lam), voff


# ---- a. pieces ------------------------------------------------------------------------------------------------------------------
def test_pieces_at_the_shape_cases(ctx):
    """mocap_intrinsics_linearize on edge_points, many_views and small in ONE call (7 + 70 + 3 views: many_views begins at view
    7 and small at view 77) at the perturbed starts, lambda = 1e-3: cost, gradient, S and reduced right-hand side of every
    camera against the restatement, each relative to its largest entry of that camera; S is symmetric.  The allowance is 8 x
    the restatement's own largest spread under 10 seeded permutations of the points within the views and of the views, plus
    2^-52: a sum of few terms can come out the same in every order (small's cost is 15 terms), and one differently rounded
    addition is the least another order can cost.
    Restatement's spread (CPU):  edge_points  cost 4.0e-16  gradient 5.3e-16  S 1.3e-13  rhs 8.1e-13
                                 many_views   cost 2.5e-16  gradient 3.7e-16  S 5.9e-14  rhs 4.1e-13
                                 small        cost 1.4e-16  gradient 3.0e-17  S 1.5e-13  rhs 4.7e-13
    GPU - restatement (MI355X):  0 for all twelve (the same bits: the kernels' sums run in the restatement's order)"""
    cases = [ir.case(n) for n in ir.SHAPES3]
    cams = [c["cam"] for c in cases]
    starts = [ir.perturbed_start(c, ir.SHAPE_START_SEED[c["name"]]) for c in cases]
    got, voff = linearized(ctx, cams, np.array([s[0] for s in starts]), np.concatenate([poses12(s[1], s[2]) for s in starts]))
    assert voff == [0, 7, 77, 80] and not got["layout"].any() and not got["behind"].any()
    for c, (case, (kd, R, t)) in enumerate(zip(cases, starts)):
        spread = ir.order_spread(case["cam"], kd, R, t, 1e-3)
        ref = ir.linearize(case["cam"], kd, R, t, 1e-3)
        mine = {"cost": got["cost"][c], "S": got["S"][c], "rhs": got["rhs"][c],
                "gradient": np.r_[got["gradient"][9 * c:9 * c + 9], got["gradient"][9 * len(cams) + 6 * voff[c]:9 * len(cams) + 6 * voff[c + 1]]]}
        diffs = {}
        for k in ("cost", "gradient", "S", "rhs"):
            a, b = np.asarray(ref[k], float), np.asarray(mine[k], float)
            diffs[k] = float(np.abs(a - b).max() / np.abs(a).max())
            print(f"{case['name']} {k}: restatement's spread {spread[k]:.3e}  GPU - restatement {diffs[k]:.3e}  allowed {8 * spread[k] + EPS:.3e}")
        for k in diffs:
            assert diffs[k] <= 8 * spread[k] + EPS, (case["name"], k)
        assert np.array_equal(got["S"][c], got["S"][c].T)


# ---- b. loops -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ir.SHAPES3)
def test_loop_walks_the_restatements_iterations_at_the_shape_cases(ctx, name):
    """What test_gpu_intrinsics.py::test_loop_walks_the_restatements_iterations asserts, at the shape cases: from the
    restatement's initialisation handed in as the start, ftol = 1e-9, the same accept / reject sequence, number of iterations
    and stopping rule; per-iteration cost within 8 x the largest relative spread of the restatement's per-iteration cost over
    10 permuted runs, which all decide alike, with no |rho| < 1e-3 (asserted); lambda and step length within 1e-6; the cost at
    the start within 1e-12.
    Restatement's spread (CPU):  edge_points 6.3e-14 (12 iterations, smallest |rho| 0.994)   many_views 4.9e-14 (11, 0.983)
                                 small 5.9e-11 (38, 0.503)
    GPU - restatement (MI355X):  edge_points at most 2.2e-16 in 12 iterations   many_views at most 2.2e-16 in 11
                                 small at most 2.2e-16 in the first 25 iterations, then up to 1.3e-12, in 38"""
    c = ir.case(name)
    kd, R, t = restatement_start(name)
    ref, same, spread = memo(("loop", name), lambda: ir.loop_spread(c["cam"], kd, R, t))
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


# ---- c. the library's own start -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", OWN_START)
def test_own_start_past_64_views_and_points(ctx, name):
    """No start given, sigma = 0.3 px.  The bars of test_noisy_views_reach_scipys_minimum: status > 0, rms_px < sigma sqrt(2),
    cost within 1e-6 of SciPy's minimum from the restatement's initialisation.  And the cost AT the start against the
    restatement's initialisation: a pose of view 64..69 formed wrongly shows here and nowhere else, the loop recovering from a
    bad start.  The device finds each homography's null vector by cyclic Jacobi, the restatement by np.linalg.eigh, so the
    bits differ; the allowance is 8 x how far two correct FP64 routes lie apart on the CPU, the larger of eigh against
    scipy.linalg.svd(A) and of eigh under 10 seeded permutations of the points, relative to the cost at the start.
    Restatement's two routes (CPU):  many_views svd 3.6e-14, permuted 9.6e-14   views_64 5.6e-14, 1.3e-13
                                     views_65 8.9e-16, 8.1e-14   edge_points 2.4e-13, 5.5e-13
    GPU - restatement (MI355X):      many_views -1.3e-14   views_64 -5.6e-14   views_65 4.3e-14   edge_points -1.1e-13
    Measured on the MI355X: many_views rms 0.38404 px from 2.767 at the start, cost / SciPy's - 1 = 1.2e-14, 12 iterations;
    views_64 0.38234 from 3.257, -2.0e-14, 13; views_65 0.40111 from 3.771, 2.1e-14, 12; edge_points 0.41068 from 3.132, 6.9e-15, 14."""
    c = ir.case(name)
    cam = c["cam"]
    start = restatement_start(name)
    out = camera_of(run(ctx, [cam]), [cam], 0)
    status, iters, cost0, cost = out["result"]
    rms = np.sqrt(2 * cost / cam.n_points)
    ref = ir.scipy_minimum(cam, *start)[0]
    ref0 = ir.cost_of(cam, *start)[0]
    allowed = 8 * max(ir.start_spread(cam))
    print(f"{name}: rms {rms:.5f} px (start {np.sqrt(2 * cost0 / cam.n_points):.3f})  cost / SciPy's - 1 {cost / ref - 1:.3e}  iterations {iters:.0f} "
          f"status {status:.0f}  cost at the start / restatement's - 1 {cost0 / ref0 - 1:.3e}  allowed {allowed:.3e}")
    assert status > 0 and rms < c["sigma"] * np.sqrt(2)
    assert abs(cost / ref - 1) <= 1e-6
    assert allowed > 0 and abs(cost0 / ref0 - 1) <= allowed
    n = np.array([len(o) for o, _ in cam.views])
    assert abs(np.sum(n * out["view_rms"] ** 2) / (2 * cost) - 1) <= 1e-12


# ---- d. many cameras, ragged ----------------------------------------------------------------------------------------------------
def test_300_ragged_cameras_each_give_the_bits_they_give_alone():
    """One call of 300 cameras cycling through clean_mild, noisy_golden, noisy_mild, edge_points and small (3, 12, 8, 7 and 3
    views of 5 to 221 points: 1 980 views, 129 480 points; the finish kernel runs 8 workgroups): camera k's share of every
    output is byte for byte that camera's result alone, for all 300.  The five differ, so a kernel that read a neighbour's
    state would give a wrong answer.  On a context of its own, so that this call is the one that grows the scratch:
    afterwards rig3 gives the bytes it gave before.  The restatement has no batch: a camera is a function of its own views
    there, the spread is 0.  Measured on the MI355X: the same bytes for all 300 cameras, and for rig3 before and after."""
    from mocapv2_amd.engine import MocapContext
    ctx = MocapContext(1, 1)
    rig = [ir.case(n)["cam"] for n in ir.RIG3]
    before = run(ctx, rig)
    single = {n: camera_of(run(ctx, [ir.case(n)["cam"]]), [ir.case(n)["cam"]], 0) for n in ir.RAGGED5}
    assert all(s["result"][0] > 0 for s in single.values())
    names = [ir.RAGGED5[k % 5] for k in range(300)]
    cams = [ir.case(n)["cam"] for n in names]
    out = run(ctx, cams)
    assert len(out["view_rms"]) == 1980 and len(out["kd"]) == 300
    for k, n in enumerate(names):
        same_bytes(camera_of(out, cams, k), single[n])
    after = run(ctx, rig)
    for k in range(3):
        same_bytes(camera_of(before, rig, k), camera_of(after, rig, k))


# ---- e. failed cameras among many -----------------------------------------------------------------------------------------------
FAILED_AT = {0: "no_views", 1: "two_views", 150: "fronto_parallel", 255: "empty_view", 256: "fronto_parallel", 257: "two_views",
             298: "empty_view", 299: "no_views"}


def test_failed_cameras_among_many_fail_alone(ctx):
    """The ragged call with cameras that cannot be calibrated at indices 0, 1, 150, 255, 256, 257, 298 and 299 (the first, the
    last, and both sides of the finish kernel's workgroup edge): a camera of 2 views, one of no views (view_offset[c] ==
    view_offset[c + 1]), one with a view of no points, and fronto-parallel views.  Each reports MOCAP_INTR_E_LAYOUT or
    MOCAP_INTR_E_DEGENERATE as the restatement says (tests/test_intrinsics_host.py), its kd and poses stay the NaN they were
    handed and its view_rms is NaN; every good camera is byte for byte its result alone.  The same layout through
    mocap_intrinsics_linearize flags the same cameras, whose entries are zero.  Measured on the MI355X: the eight statuses
    are the restatement's, the 292 good cameras give the same bytes as alone."""
    failed = ir.failed_cameras()
    names = [FAILED_AT.get(k, ir.RAGGED5[k % 5]) for k in range(300)]
    cams = [failed[n][0] if n in failed else ir.case(n)["cam"] for n in names]
    out = run(ctx, cams)
    voff = np.cumsum([0] + [len(cam.views) for cam in cams])
    for k, n in enumerate(names):
        mine = camera_of(out, cams, k)
        if n in failed:
            assert mine["result"][0] == failed[n][1], (k, n)
            assert np.isnan(mine["kd"]).all() and np.isnan(mine["poses"]).all() and np.isnan(mine["view_rms"]).all(), (k, n)
            assert mine["result"][1] == 0 and len(mine["history"]) == 0, (k, n)
        else:
            same_bytes(mine, alone(ctx, n))
    kd = np.tile(ir.case("clean_mild")["kd"], (300, 1))
    poses = np.tile(np.r_[np.eye(3).reshape(9), 0.0, 0.0, 1.0], (voff[-1], 1))
    lin, _ = linearized(ctx, cams, kd, poses)
    rule = np.array([ir.layout_error([len(o) for o, _ in cam.views]) is not None for cam in cams])
    assert np.array_equal(lin["layout"], rule) and np.array_equal(rule, out["status"] == ir.E_LAYOUT) and rule.sum() == 6
    assert not lin["behind"].any()
    for k in range(300):
        gv = lin["gradient"][9 * 300 + 6 * voff[k]:9 * 300 + 6 * voff[k + 1]]
        if rule[k]:
            assert lin["cost"][k] == 0 and not lin["S"][k].any() and not lin["rhs"][k].any() and not lin["gradient"][9 * k:9 * k + 9].any() and not gv.any(), k
        else:
            assert lin["cost"][k] > 0 and lin["S"][k].any() and gv.any(), k


# ---- f. the layout rule ---------------------------------------------------------------------------------------------------------
def test_fewer_equations_than_unknowns_are_a_layout_error(ctx):
    """3 views of 4 points, 24 equations for 27 unknowns, which the loop would fit exactly with a wrong lens (rms 0, status
    lambda: tests/test_intrinsics_host.py::test_fewer_equations_than_unknowns_fit_a_wrong_lens): MOCAP_INTR_E_LAYOUT at the C
    entry with its arrays untouched and both neighbours calibrated as if alone; calibrate_intrinsics raises ValueError naming
    the camera.  The layouts that just suffice pass the rule: small (30 for 27) is calibrated (test b), and five_by_four (40
    for 39) gets the status the restatement gives it, MOCAP_INTR_E_DEGENERATE from its initialisation (1 / fx^2 = -3.5e-6),
    the camera beside it untouched."""
    from mocapv2_amd import calibrate as cal
    good, bad, small, five = (ir.case(n)["cam"] for n in ("clean_mild", "three_by_four", "small", "five_by_four"))
    cams = [small, bad, good]
    out = run(ctx, cams)
    mine = camera_of(out, cams, 1)
    assert mine["result"][0] == ir.E_LAYOUT and np.isnan(mine["kd"]).all() and np.isnan(mine["poses"]).all() and np.isnan(mine["view_rms"]).all()
    same_bytes(camera_of(out, cams, 0), alone(ctx, "small"))
    same_bytes(camera_of(out, cams, 2), alone(ctx, "clean_mild"))
    assert alone(ctx, "small")["result"][0] > 0
    lin, _ = linearized(ctx, cams, np.tile(ir.case("clean_mild")["kd"], (3, 1)), np.tile(np.r_[np.eye(3).reshape(9), 0.0, 0.0, 1.0], (9, 1)))
    assert list(lin["layout"]) == [False, True, False] and lin["cost"][1] == 0 and not lin["S"][1].any()
    with pytest.raises(ValueError, match="camera 1: 12 points in 3 views are 24 equations for 27 unknowns"):
        cal.calibrate_intrinsics([good.views, bad.views], good.size, ctx=ctx)
    want = ir.status_from_own_start(five)
    out = run(ctx, [good, five])
    print("five_by_four: status", out["status"][1], "restatement's", want)
    assert out["status"][1] == want and want != ir.E_LAYOUT
    same_bytes(camera_of(out, [good, five], 0), alone(ctx, "clean_mild"))
    res = cal.calibrate_intrinsics([good.views, five.views, small.views], good.size, ctx=ctx)
    assert res[0]["status"] > 0 and res[1]["status"] == want and res[2]["status"] == alone(ctx, "small")["result"][0]
