"""The definition of the rig bundle adjustment that refines the lenses too, checked on the CPU through its
NumPy restatement tests/rig_selfcal_ref.py: the analytic Jacobian, the Schur elimination with fixed columns, what a mask
leaves alone, and what the refinement is worth on a rig whose intrinsics are of checkerboard grade.  The GPU is held to the
same restatement by tests/test_gpu_rig_selfcal.py."""
import importlib.util
import os

import numpy as np
import pytest

import rig_ba_ref as rb
import rig_robust_ref as rr
import rig_selfcal_ref as sc

P = sc.P
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def small():
    """C = 4, N = 30 drawn (about 30 % of the views hidden), a state off the truth"""
    return sc.small_case(4, seed=31, n_points=30)


@pytest.fixture(scope="module")
def small60():
    """The same rig with 60 points drawn: every camera has the 18 observations that nine free lens parameters ask for"""
    return sc.small_case(4, seed=31, n_points=60)


def test_jacobian_against_central_differences(small):
    """Every column of the restatement's Jacobian (all 15 per camera with mask 0x1FF, camera 0's pose columns through a
    second evaluation that frees them, and the points') against central differences of its residual.  Steps: 1e-6 of the
    parameter's scale (focal lengths and principal point 1e-3 px, everything else 1e-6).  Bound, reasoned: the truncation
    error of a central difference is h^2 / 6 of the third derivative, the rounding error eps |r| / h with |r| <= 2e3 px: both
    below 1e-6 of a column's largest entry here, whose columns are at least 0.1 px per unit.  Measured: 1.3e-7."""
    prob, _, kd, R, t, X = small
    C, N = prob.C, prob.N
    assert C == 4 and 20 <= N <= 30 and 0.15 < 1 - len(prob.pt) / (C * N) < 0.45
    free = np.ones((C, P), bool)  # (camera 0's pose columns too: the derivative is the same function)
    r, jc, jp, front, _ = sc.observe(prob, kd, R, t, X, free)
    assert front.all()
    n_obs = len(prob.pt)
    J = np.zeros((2 * n_obs, P * C + 3 * N))
    for o in range(n_obs):
        J[2 * o:2 * o + 2, P * prob.cam[o]:P * prob.cam[o] + P] = jc[o]
        J[2 * o:2 * o + 2, P * C + 3 * prob.pt[o]:P * C + 3 * prob.pt[o] + 3] = jp[o]
    scale = np.r_[np.tile(np.r_[[1e-3] * 4, [1e-6] * 11], C), np.full(3 * N, 1e-6)]

    def residual(d):
        dc, dp = d[:P * C].reshape(C, P), d[P * C:].reshape(N, 3)
        R2, t2 = R.copy(), t.copy()
        for c in range(C):  # camera 0 included
            R2[c] = rb.exp_so3(dc[c, 9:12]) @ R[c]
            t2[c] = t[c] + dc[c, 12:]
        return sc.residual_vector(prob, kd + dc[:, :9], R2, t2, X + dp)

    worst = 0.0
    for k in range(J.shape[1]):
        d = np.zeros(J.shape[1])
        d[k] = scale[k]
        fd = (residual(d) - residual(-d)) / (2 * scale[k])
        assert np.abs(J[:, k]).max() > 0.1
        worst = max(worst, float(np.abs(fd - J[:, k]).max() / np.abs(J[:, k]).max()))
    print(f"largest difference of a column, relative to its largest entry: {worst:.3e}")
    assert worst < 1e-6


def test_mask_zero_is_the_plain_adjustments_problem(small):
    """With every mask 0 the pose blocks of cameras 1.. are rig_ba_ref's reduced system at the same lenses: the same
    per-observation operations, the pairs of a point's observations enumerated in another order (camera 0's take part here), so
    equal to a few roundings of the largest entry (1e-13 of it allowed; the cost, one sum in one order, to the bit), and every
    other row and column is the identity's"""
    prob, _, kd, R, t, X = small
    plain = rb.Problem(prob.pt, prob.cam, prob.uv, np.array([[[k[0], 0, k[2]], [0, k[1], k[3]], [0, 0, 1.0]] for k in kd]), kd[:, 4:], prob.N)
    a = sc.linearize(prob, kd, R, t, X, 1e-3, 0)
    b = rb.linearize(plain, R, t, X, 1e-3)
    idx = np.concatenate([np.arange(P * c + 9, P * c + P) for c in range(1, prob.C)])
    assert a["cost"] == b["cost"]
    assert np.abs(a["S"][np.ix_(idx, idx)] - b["S"]).max() <= 1e-13 * np.abs(b["S"]).max()
    assert np.abs(a["rhs"][idx] - b["rhs"]).max() <= 1e-13 * np.abs(b["rhs"]).max()
    rest = np.setdiff1d(np.arange(P * prob.C), idx)
    assert np.array_equal(a["S"][np.ix_(rest, rest)], np.eye(len(rest))) and not a["S"][np.ix_(rest, idx)].any() and not a["rhs"][rest].any()


@pytest.mark.parametrize("loss_c", [None, 2.0])
def test_schur_step_is_the_dense_step_and_fixed_parameters_do_not_move(small, loss_c):
    """The step from the reduced system against the one from the full damped normal equations over the free parameters alone,
    with mixed masks; a fixed parameter's step is exactly 0.  Bound 1e-8 of the step's largest entry: Marquardt's damping makes
    the step invariant under a scaling of the parameters, so the condition number that counts is that of S scaled to a unit
    diagonal, below 1e5 here (asserted; measured 3.9e3 and 2.9e3); times the unit roundoff and the 100-odd unknowns.
    Measured: cameras 1.5e-12 and 1.7e-12, points 7.4e-14 and 1.1e-13."""
    prob, _, kd, R, t, X = small
    masks = np.array([0, 0x1FF, 0x03F, 0x003])
    lin = sc.linearize(prob, kd, R, t, X, 1e-3, masks, loss_c)
    dc, dp, pred = sc.schur_step(prob, lin, 1e-3)
    dc2, dp2 = sc.dense_step(prob, lin, 1e-3)
    free = lin["free"].reshape(-1)
    assert free.sum() == 0 + 15 + 12 + 8 and not dc[~free].any() and np.isfinite(pred)
    d = np.sqrt(np.diag(lin["S"]))
    assert np.linalg.cond(lin["S"] / d[:, None] / d[None, :]) < 1e5
    assert np.abs(dc - dc2).max() <= 1e-8 * np.abs(dc2).max() and np.abs(dp - dp2).max() <= 1e-8 * np.abs(dp2).max()
    assert np.array_equal(lin["S"], lin["S"].T)


def test_a_masked_parameter_comes_back_with_its_bits(small):
    prob, _, kd, R, t, X = small
    masks = np.array([0, 0x1FF, 0x03F, 0x003])
    out = sc.lm(prob, kd, R, t, X, masks, max_iters=8)
    free = sc.free_columns(masks, prob.C)[:, :9]
    assert out["cost"] < out["cost_initial"]
    assert out["kd"][~free].tobytes() == kd[~free].tobytes()
    assert (out["kd"][free] != kd[free]).all()
    assert np.array_equal(out["R"][0], np.eye(3)) and not out["t"][0].any()
    assert abs(np.linalg.norm(out["t"][1]) - np.linalg.norm(t[1])) <= 4e-16 * np.linalg.norm(t[1])


def test_layout_check_counts_a_cameras_observations(small60):
    small = small60
    prob = small[0]
    count = np.bincount(prob.cam, minlength=prob.C)
    assert count.min() >= 18 and sc.layout_ok(prob, 0x1FF)
    few = np.flatnonzero(prob.cam == 2)[17:]  # camera 2 keeps 17 observations: one short of twice nine
    thin, _ = rr.without(prob, few)
    assert np.bincount(thin.cam, minlength=4)[2] <= 17
    assert not sc.layout_ok(thin, 0x1FF) and sc.layout_ok(thin, [0x1FF, 0x1FF, 0x0FF, 0x1FF]) and sc.layout_ok(thin, [0x1FF, 0x1FF, 0, 0x1FF])
    with pytest.raises(ValueError):
        sc.lm(thin, *small[2:], 0x1FF)


def test_refinement_recovers_what_checkerboard_intrinsics_lose():
    """A ring of 6 cameras with distortion, each with its own true K and lens; 200 points drawn, 30 % of the views hidden,
    0.05 px noise; the start's intrinsics are of checkerboard grade (f off by 0.3 %, the principal point by 3 px, k1 and k2 by
    5e-3, signs seeded per camera).  Yardstick: the rms reprojection residual of the restatement from the TRUE intrinsics with
    mask 0.  Margin: 1.2 x the yardstick, for the 36 more degrees of freedom that fit the noise.
    Measured (this file, CPU):  yardstick 0.03900 px (6 iterations)
                                "focal+center+radial2" from the checkerboard start 0.03846 px = 0.986 x (13 iterations, ftol)
                                intrinsics fixed at the checkerboard start 0.09309 px = 2.39 x
    (also DESIGN.md section 2).  The residual is recovered, the parameters only as far as the capture holds them: fx comes back
    within 1.5 px, fy within 4.7 px of the truth (from 4.3 px), the principal point within 1.0 px (from 3 px), k1 within 3.3e-3
    (from 5e-3), and k2 ends farther off (2.1e-2) than it began: over this field of view k2 trades against k1 and f."""
    c = sc.lens_case(6, 200, 11, 0.05)
    prob = c["prob"].sorted()
    assert prob.C == 6 and 190 <= prob.N <= 200 and 0.25 < 1 - len(prob.pt) / (6 * prob.N) < 0.35
    assert np.ptp(c["kd_true"][:, 0]) > 10 and np.abs(c["kd_true"][:, 4:6]).min() > 0
    R, t, X = rb.perturbed_start(c, 18, rot=0.003, trans=0.005, point=0.005)
    kd0 = sc.checkerboard_start(c["kd_true"], 20)
    assert np.allclose(np.abs(kd0[:, 0] / c["kd_true"][:, 0] - 1), 3e-3) and np.allclose(np.abs(kd0 - c["kd_true"])[:, 2:6], [3, 3, 5e-3, 5e-3])
    yard = sc.lm(prob, c["kd_true"], R, t, X, 0)
    fixed = sc.lm(prob, kd0, R, t, X, 0)
    refined = sc.lm(prob, kd0, R, t, X, sc.MASKS["focal+center+radial2"])
    y, f, r = (sc.rms_px(prob, o["cost"]) for o in (yard, fixed, refined))
    print(f"yardstick {y:.5f} px ({yard['iterations']} iterations)  refined {r:.5f} px = {r / y:.3f} x ({refined['iterations']} iterations, "
          f"status {refined['status']})  fixed {f:.5f} px = {f / y:.3f} x")
    print("refined - truth, largest per parameter:", np.abs(refined["kd"] - c["kd_true"]).max(0))
    assert yard["status"] == refined["status"] == sc.STOP_FTOL and refined["iterations"] < 50
    assert r <= 1.2 * y
    assert f > 2 * y  # well outside the margin
    assert refined["kd"][:, 6:].tobytes() == kd0[:, 6:].tobytes()


@pytest.mark.parametrize("name", sorted(sc.LOOP_CASES))
def test_loop_cases_are_far_from_every_decision_boundary(name):
    """The rigs tests/test_gpu_rig_selfcal.py walks beside the restatement: no gain ratio within 1e-3 of the accept / reject
    boundary, no relative decrease within a factor 1.2 of LOOP_FTOL, the stop is ftol's, and S scaled to a unit diagonal has a
    condition number below 1e6 (the loop test's reasoning rests on it).
    Measured: iterations 19 / 19 / 11 / 11 / 20 (mixed3, mixed3_cauchy, mixed4, mixed4_cauchy, wide7); smallest |rho| 0.23;
    nearest relative decrease a factor 1.29 below ftol (wide7's last); condition numbers 3.0e3 to 3.4e3."""
    prob, kd, R, t, X, masks, loss_c, ref = sc.loop_case(name)
    assert prob.C <= 7 and prob.N <= 60 and sc.layout_ok(prob, masks)
    if name == "wide7":
        assert sc.P * prob.C > 90 and (np.bincount(prob.pt) == 3).all()
    cost = np.r_[ref["cost_initial"], ref["history"][:, 0]]
    rel = (cost[:-1] - cost[1:])[ref["history"][:, 2] > 0] / cost[:-1][ref["history"][:, 2] > 0]
    lin = sc.linearize(prob, kd, R, t, X, 1e-3, masks, loss_c)
    d = np.sqrt(np.diag(lin["S"]))
    cond = np.linalg.cond(lin["S"] / d[:, None] / d[None, :])
    print(f"{name}: {ref['iterations']} iterations, status {ref['status']}, smallest |rho| {np.abs(ref['rho']).min():.3g}, relative "
          f"decreases nearest ftol {rel[np.argsort(np.abs(np.log(rel / sc.LOOP_FTOL)))[:2]]}, scaled cond(S) {cond:.3e}")
    assert ref["status"] == sc.STOP_FTOL and ref["iterations"] < 50
    assert (np.abs(ref["rho"]) >= 1e-3).all()
    assert ((rel >= 1.2 * sc.LOOP_FTOL) | (rel <= sc.LOOP_FTOL / 1.2)).all()
    assert cond < 1e6


@pytest.mark.parametrize("name", sc.SHAPE_LOOPS)
def test_shape_loop_cases_are_far_from_every_decision_boundary(name):
    """The same four conditions for the rigs tests/test_gpu_rig_selfcal_shapes.py walks beside the restatement (and the
    blocks_* cases it only linearises).
    Measured, in the order iterations, smallest |rho|, the two relative decreases nearest ftol as multiples of it, scaled
    cond(S):            two             13  0.67  9.2 x / 0.018 x   6.1e2
                        six_lds         10  0.99  2.15 x / 0.29 x   4.6e3
                        six_600          9  1.0   6.5 x / 0.072 x   4.0e3
                        six_600_cauchy   9  1.0   13 x / 0.25 x     4.2e3
                        blocks_255       9  0.99  6.8 x / 0.0077 x  3.2e3
                        blocks_256       9  0.99  7.0 x / 0.0088 x  3.2e3
                        blocks_257       9  0.99  7.8 x / 0.0094 x  3.1e3
                        blocks_513       9  1.0   8.8 x / 0.014 x   3.4e3
                        rig32           12  0.98  7.0 x / 0.36 x    4.7e3
                        rig32_cauchy    12  0.99  9.7 x / 0.67 x    5.4e3
    Every step of every case is accepted and every stop is ftol's."""
    prob, kd, R, t, X, masks, loss_c, ref = sc.shape_case(name)
    cost = np.r_[ref["cost_initial"], ref["history"][:, 0]]
    rel = (cost[:-1] - cost[1:])[ref["history"][:, 2] > 0] / cost[:-1][ref["history"][:, 2] > 0]
    lin = sc.linearize(prob, kd, R, t, X, 1e-3, masks, loss_c)
    d = np.sqrt(np.diag(lin["S"]))
    cond = np.linalg.cond(lin["S"] / d[:, None] / d[None, :])
    print(f"{name}: {ref['iterations']} iterations, status {ref['status']}, smallest |rho| {np.abs(ref['rho']).min():.3g}, relative "
          f"decreases nearest ftol {rel[np.argsort(np.abs(np.log(rel / sc.LOOP_FTOL)))[:2]] / sc.LOOP_FTOL} x ftol, scaled cond(S) {cond:.3e}")
    assert ref["status"] == sc.STOP_FTOL and ref["iterations"] < 50
    assert (np.abs(ref["rho"]) >= 1e-3).all()
    assert ((rel >= 1.2 * sc.LOOP_FTOL) | (rel <= sc.LOOP_FTOL / 1.2)).all()
    assert cond < 1e6


def test_shape_cases_have_the_shapes_they_are_named_for():
    """What each case of SHAPE_CASES is there for, restated from its sizes: the workgroups of the point kernels and the Schur
    kernel's chunks (PT_THREADS = SCHUR_CHUNK = 256: csrc/kernels.h, csrc/rig_selfcal.hip), the rows of S against the 90 the Cholesky holds in
    LDS and the 480 of the largest rig, and for rig32 a point that all 32 cameras see (bit 31 of a visibility mask, every one of
    the 528 pairs) and observations in camera 31.  Every case passes the layout check."""
    import re
    source = ""
    for name in ("rig_selfcal.hip", "rig_lm.h", "kernels.h"):  # the solver's file, the shared phases, the host's record
        with open(os.path.join(ROOT, "mocapv2_amd", "csrc", name)) as f:
            source += f.read()
    constants = {k: int(v) for k, v in re.findall(r"constexpr int (PT_THREADS|SCHUR_CHUNK|CHOL_LDS_ROWS) = (\d+);", source)}
    assert constants == {"PT_THREADS": 256, "SCHUR_CHUNK": 256, "CHOL_LDS_ROWS": 90}  # what lin_blocks and schur_chunks restate
    for name, (n_cam, _, n_keep, _, masks, _, _) in sc.SHAPE_CASES.items():
        prob, _, _, _, X, m, _, _ = sc.shape_case(name)
        assert prob.C == n_cam and len(X) == prob.N and (n_keep is None or prob.N == n_keep) and sc.layout_ok(prob, m), name
        assert np.array_equal(prob.pt, np.sort(prob.pt)) and (np.bincount(prob.pt, minlength=prob.N) >= 2).all(), name
    sizes = {name: sc.shape_case(name)[0] for name in sc.SHAPE_CASES}
    assert sizes["two"].N == 289 and sc.lin_blocks(289) == 2 and np.bincount(sizes["two"].pt).tolist() == [2] * 289
    assert sc.P * sizes["six_lds"].C == 90 and sizes["six_lds"].N == 59
    assert sizes["six_600"].N == 594 and len(sizes["six_600"].pt) == 2554 and sc.lin_blocks(594) == 3 and sc.schur_chunks(594) == (256, 3)
    for n, blocks in ((255, 1), (256, 1), (257, 2), (513, 3)):
        assert sizes[f"blocks_{n}"].N == n and sc.lin_blocks(n) == blocks and sc.schur_chunks(n) == (256, blocks)
    rig = sizes["rig32"]
    count = np.bincount(rig.cam, minlength=32)
    assert sc.P * rig.C == 480 and rig.N == 140 and rig.C * (rig.C + 1) // 2 == 528
    assert (np.bincount(rig.pt) == 32).sum() >= 1 and count[31] > 0 and count.min() >= 2 * 6
    print(f"rig32: {len(rig.pt)} observations, {(np.bincount(rig.pt) == 32).sum()} points seen by all cameras, at least {count.min()} per camera")
    grown = sizes["chunk_growth"]
    assert grown.N == 65537 and sc.schur_chunks(grown.N) == (257, 256) and sc.lin_blocks(grown.N) == 257


def test_the_named_masks_are_the_python_surfaces():
    from mocapv2_amd import calibrate
    assert calibrate.REFINE_MASKS == sc.MASKS
    assert calibrate._refine_masks(None, 4) is None
    assert calibrate._refine_masks("focal+center", 3).tolist() == [0xF] * 3 and calibrate._refine_masks([1, 2, 0x1FF], 3).tolist() == [1, 2, 0x1FF]
    assert calibrate._refine_masks("focal", 2).tolist() == [3, 3]
    with pytest.raises(ValueError):  # (None is the plain functions' business; refused before any GPU work)
        calibrate.bundle_adjust_rig_intrinsics(np.zeros((3, 4, 2)), None, [], [], refine_intrinsics=None)
    with pytest.raises(ValueError):
        calibrate.calibrate_rig_intrinsics(np.zeros((3, 4, 2)), None, [], refine_intrinsics=None)
    for bad, n in (("focal+center", 2), (0x4, 2), ("everything", 4), (0x200, 4), ([1, 2], 4), (1.5, 4)):
        with pytest.raises(ValueError):
            calibrate._refine_masks(bad, n)


def test_kernels_use_no_scratch_memory_and_spill_nothing():
    """The compiler's own metadata for csrc/rig_selfcal.hip (scratch/kernel_meta.py, no GPU needed): 0 bytes of scratch and 0
    spilled VGPRs for every kernel, the point-owning ones with their 2 x 15 Jacobians included; the LDS stays under 64 KB.
    DESIGN.md section 4 has the figures."""
    spec = importlib.util.spec_from_file_location("kernel_meta", os.path.join(ROOT, "scratch", "kernel_meta.py"))
    km = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(km)
    ks = km.kernels_of(os.path.join(km.CSRC, "rig_selfcal.hip"))
    names = " ".join(k["name"] for k in ks)
    for want in ("rig_init", "selfcal_check", "rig_linearize", "selfcal_schur", "rig_reduce", "rig_solve", "rig_update", "rig_decide",
                 "rig_finish", "rig_residuals"):
        assert f"{want}_kernel" in names
    for k in ks:
        print(k)
        assert k["scratch"] == 0 and k["spill"] == 0 and k["lds"] <= 65536, k


def test_the_library_exports_the_new_entries_and_refuses_null_arguments():
    import ctypes
    from mocapv2_amd import _abi
    lib = _abi.load()
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    mask = (ctypes.c_int * 2)(3, 3)
    assert lib.mocap_rig_bundle_adjust_intrinsics(None, 2, 4, 8, p, p, p, p, mask, p, p, 5, 1e-12, 1e-3, p, p, 0, 0.0, p, p, None) == -1
    assert b"null" in lib.mocap_last_error()
    assert lib.mocap_rig_linearize_intrinsics(None, 2, 4, 8, p, p, p, p, mask, p, p, 1e-3, p, p, p, p, p, 0, 0.0, None) == -1
    assert b"null" in lib.mocap_last_error()
