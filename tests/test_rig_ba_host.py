"""Rig bundle adjustment, the part that needs no GPU: the NumPy restatement of the definition (tests/rig_ba_ref.py) against
central differences, a dense solve and SciPy; the bars of tests/test_gpu_rig_ba.py met by the restatement alone; the
conditions the cases of tests/test_gpu_rig_ba_shapes.py must meet; the host-side helpers; the C-ABI surface of the two new entry points; the code-object table of the new kernels."""
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


# ---- the shapes of tests/test_gpu_rig_ba_shapes.py -------------------------------------------------------------------------------
def test_shape_cases_have_the_shapes_they_are_named_for():
    """What each case of rig_ba_ref.SHAPE_CASES is there for, restated from its sizes: the workgroups of the point kernels
    (PT_THREADS = 256, csrc/kernels.h), rig_schur_kernel's chunks and the points of the last one (SCHUR_CHUNK = 1024,
    csrc/rig_ba.hip), the rows of S against the 90 the Cholesky holds in LDS (CHOL_LDS_ROWS, csrc/rig_lm.h), the 3 N and N of the
    grid-stride loops against grid_for's 1024 workgroups of 256 threads; every point has 2..C views in ascending camera order;
    visibility is partial (the Schur kernel finds a camera's W block by counting the mask's bits below it); camera 31 sees
    points of pose_c32_cauchy.  Prints each case's shape and the CPU time of making it."""
    source = {}
    for name in ("rig_ba.hip", "rig_lm.h", "kernels.h"):
        with open(os.path.join(ROOT, "mocapv2_amd", "csrc", name)) as f:
            source[name] = f.read()
    constants = {k: int(v) for text in source.values() for k, v in re.findall(r"constexpr int (PT_THREADS|SCHUR_CHUNK|CHOL_LDS_ROWS) = (\d+);", text)}
    assert constants == {"PT_THREADS": 256, "SCHUR_CHUNK": 1024, "CHOL_LDS_ROWS": 90}  # what lin_blocks and schur_chunks restate
    assert "g > 1024 ? 1024 : g" in source["rig_lm.h"] and "grid_for(3 * most)" in source["rig_lm.h"] and "grid_for(3 * a.N)" in source["rig_lm.h"]
    grid = 1024 * 256
    want = {  # name: (cameras, points, workgroups of the point kernels, (Schur chunks, points of the last), rows of S)
        "pose_two": (2, 600, 3, (1, 600), 6),
        "pose_255": (4, 255, 1, (1, 255), 18), "pose_256": (4, 256, 1, (1, 256), 18), "pose_257": (4, 257, 2, (1, 257), 18),
        "pose_1023": (3, 1023, 4, (1, 1023), 12), "pose_1024": (3, 1024, 4, (1, 1024), 12), "pose_1025": (3, 1025, 5, (2, 1), 12),
        "pose_2049_cauchy": (3, 2049, 9, (3, 1), 12),
        "pose_c17": (17, 300, 2, (1, 300), 96), "pose_c17_cauchy": (17, 300, 2, (1, 300), 96),
        "pose_c32_cauchy": (32, 140, 1, (1, 140), 186),
        "pose_stride_3n": (2, 87382, 342, (86, 342), 6), "pose_stride_n": (2, 262145, 1025, (257, 1), 6),
    }
    assert set(want) == set(rb.SHAPE_CASES)
    for name, (n_cam, n, blocks, chunks, rows) in want.items():
        case = rb.shape_case(name)
        prob = case["prob"]
        counts = np.bincount(prob.pt, minlength=prob.N)
        print(f"{name}: C {prob.C}  N {prob.N}  observations {len(prob.pt)}  views per point {counts.min()} .. {counts.max()}  point workgroups "
              f"{rb.lin_blocks(prob.N)}  Schur chunks {rb.schur_chunks(prob.N)}  rows of S {prob.D}  loss {case['loss_c']}  CPU {case['cpu_s']:.2f} s")
        assert (prob.C, prob.N, rb.lin_blocks(prob.N), rb.schur_chunks(prob.N), prob.D) == (n_cam, n, blocks, chunks, rows), name
        assert case["X"].shape == (n, 3) and (case["loss_c"] == 2.0) == name.endswith("_cauchy"), name
        off, cam, uv = prob.point_major()
        assert counts.min() >= 2 and counts.max() <= n_cam and off[-1] == len(cam) == len(prob.pt), name
        inner = np.ones(len(cam), bool)
        inner[off[:-1]] = False
        assert (np.diff(cam, prepend=-1)[inner] > 0).all() and np.array_equal(prob.pt, np.repeat(np.arange(n), counts)), name
        if n_cam > 2:
            # partial visibility (the 30 % dropout): most points miss a camera, and which ones they miss differs
            assert (counts < n_cam).mean() > 0.5 and len({tuple(cam[off[i]:off[i + 1]]) for i in range(n)}) >= 4, name
        assert np.array_equal(case["R"][0], np.eye(3)) and not case["t"][0].any(), name  # the gauge, to the bit
        assert rb.cost_of(prob, case["R"], case["t"], case["X"])[1], name
    D = {name: rb.shape_case(name)["prob"].D for name in want}
    assert D["pose_c17"] == 96 > constants["CHOL_LDS_ROWS"] >= 6 * (16 - 1) and 16 * 17 // 2 == 136 and 31 * 32 // 2 == 496
    rig = rb.shape_case("pose_c32_cauchy")["prob"]
    assert np.bincount(rig.cam, minlength=32)[31] >= 1
    assert 3 * 87382 == grid + 2 and 3 * 87381 < grid and 262145 == grid + 1  # a second trip of two elements, and of one point


@pytest.mark.parametrize("name", rb.SHAPE_SEAMS)
def test_a_seam_cases_last_point_cannot_be_lost_unseen(name):
    """The last point of every case that ends on a seam (the first point of a second workgroup, the one point of a last Schur
    chunk, the point of a second trip) is seen by at least two free cameras (index >= 1), so that it lands in an off-diagonal
    block of the Schur complement too; with two cameras there is one free camera and one block, and the point is in it.  And
    the restatement without that point differs from the full one in S and in rhs by more than 100 x what
    tests/test_gpu_rig_ba_shapes.py allows (8 x the order spread): a kernel that drops it fails there.  pose_256 and pose_1024
    end just before the seam: their last point is the one a `<` for a `<=` would lose.
    The seeds of the 4-camera and 3-camera families (302, 306) are the first at which points 255 and 256, and 1023 and 1024,
    all have two free cameras.
    Measured (S, rhs: without the last point / allowed): printed; the smallest factor is pose_stride_n's."""
    import time
    t0 = time.process_time()
    case = rb.shape_case(name)
    prob, R, t, X, loss_c = (case[k] for k in ("prob", "R", "t", "X", "loss_c"))
    last = prob.cam[prob.pt == prob.N - 1]
    assert (last >= 1).sum() >= min(2, prob.C - 1), last
    ref, spread = rb.shape_pieces(name)
    less, X_less = rb.first_points(prob, X, prob.N - 1)
    lost = rb.shape_linearize(less, R, t, X_less, 1e-3, loss_c)
    for k in ("S", "rhs"):
        d = float(np.abs(ref[k] - lost[k]).max() / np.abs(ref[k]).max())
        print(f"{name} {k}: without the last point {d:.3e}  allowed {8 * spread[k]:.3e}  factor {d / (8 * spread[k]):.3g}")
        assert d > 100 * 8 * spread[k], k
    print(f"{name}: last point's cameras {last}  CPU {time.process_time() - t0:.1f} s")


@pytest.mark.parametrize("name", rb.SHAPE_LOOPS)
def test_shape_loop_cases_are_far_from_every_decision_boundary(name):
    """The two conditions tests/test_gpu_rig_ba.py's loop test rests on, for the cases tests/test_gpu_rig_ba_shapes.py walks
    beside the restatement: no iteration at LOOP_FTOL has |rho| < 1e-3 (none is a failed solve either), and the damped S of the
    start has a condition number below 1e6.  More than that: the stop is ftol's, no relative decrease lies within a factor 1.2
    of ftol, and the restatement walks the same loop on two seeded permutations of the observations with every step length
    within 2.5e-7 of the sorted problem's: a quarter of the 1e-6 the device is held to, so that the restatement's own
    dependence on the order of its sums leaves three quarters of that bar to the device.
    That last condition is what pose_2049_cauchy needed another seed AND the small perturbation for.  The damping falls by 3
    with every accepted step, the cost does not depend on the rig's scale, so at a small lambda S is singular along the scale
    gauge to working precision, and the component of a step along it, which the cost does not see, is rounding: cond(S) < 1e6
    at lambda = 1e-3 says nothing about iteration 19.  With rig_robust_ref.dirty's outliers on three cameras the loop under
    the loss is slow (a point of three views that carries two outliers hangs on one good view).  From the default
    perturbation, of the seeds 300 .. 399 none stops on ftol in fewer than 17 iterations, half end in failed solves
    (at 1e-3 / 3^26 numpy's Cholesky gives up), and the first tried that stops on ftol with all other conditions met (318, 19
    iterations, lambda 8.6e-13 at the end) has step lengths that differ by 3.6e-4 between two orders of the restatement's own
    sums -- and by 3.9e-4 between the MI355X and the restatement, with every other figure of the loop test inside its bar
    (cost 1.0e-14, returned state 6.9e-14 of what it moved).  From the small perturbation four seeds of 300 .. 399 stop within 13
    iterations; of the two whose last point two free cameras see, 354 has the wider margins (2.8 x and 0.68 x ftol, 4.6e-8
    between orders; 321: 1.4 x, 0.46 x, 1.5e-7).
    Measured (iterations, smallest |rho|, the two relative decreases nearest ftol as multiples of it, cond(S), step lengths
    between orders): printed per case."""
    import time
    import rig_robust_ref as rr
    t0 = time.process_time()
    case, ref = rb.shape_case(name), rb.shape_loop(name)
    prob, start, loss_c = case["prob"], (case["R"], case["t"], case["X"]), case["loss_c"]
    lin = rb.shape_linearize(prob, *start, 1e-3, loss_c)
    cond = np.linalg.cond(lin["S"])
    costs = np.r_[ref["cost_initial"], ref["history"][:, 0]]
    ok = ref["history"][:, 2] > 0
    rel = ((costs[:-1] - costs[1:]) / costs[:-1])[ok]
    between = 0.0
    for seed in (1000, 1001):
        p = rb.permuted(prob, seed)
        other = rb.lm(p, *start, ftol=rb.LOOP_FTOL) if loss_c is None else rr.lm(p, *start, loss_c, ftol=rb.LOOP_FTOL)
        assert other["iterations"] == ref["iterations"] and np.array_equal(other["history"][:, 2], ref["history"][:, 2]), seed
        between = max(between, float(np.abs(other["history"][:, 3] / ref["history"][:, 3] - 1).max()))
    print(f"{name}: {ref['iterations']} iterations, status {ref['status']}, accepted {int(ok.sum())}, smallest |rho| {np.abs(ref['rho']).min():.3g}, "
          f"relative decreases nearest ftol {rel[np.argsort(np.abs(np.log(rel / rb.LOOP_FTOL)))[:2]] / rb.LOOP_FTOL} x ftol, cond(S) {cond:.3e}, "
          f"step lengths between orders {between:.1e}, CPU {time.process_time() - t0:.1f} s")
    assert ref["status"] == rb.STOP_FTOL and ref["iterations"] < 50
    assert np.isfinite(ref["rho"]).all() and (np.abs(ref["rho"]) >= 1e-3).all()
    assert ((rel >= 1.2 * rb.LOOP_FTOL) | (rel <= rb.LOOP_FTOL / 1.2)).all()
    assert cond < 1e6
    assert between <= 2.5e-7


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
