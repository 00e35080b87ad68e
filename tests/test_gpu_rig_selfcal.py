"""The rig bundle adjustment that refines the lenses too, on the GPU (csrc/rig_selfcal.hip through
mocap_rig_linearize_intrinsics / mocap_rig_bundle_adjust_intrinsics and the Python surface of mocapv2_amd.calibrate) against
the NumPy restatement of the definition (tests/rig_selfcal_ref.py).  The restatement alone meets the bars of the definition on
the CPU, and its loop cases are shown to be far from every decision boundary: tests/test_rig_selfcal_host.py.  Every rig
here has at most 7 cameras and 60 points."""
import numpy as np
import pytest

import rig_selfcal_ref as sc
from rig_selfcal_gpu import adjust, adjust_raw, assert_loop_walks_the_restatements, assert_pieces_agree, gpu_args, loss_args, poses12

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from mocapv2_amd.engine import MocapContext
    return MocapContext(1, 1)


MIXED = ["mixed3", "mixed3_cauchy", "mixed4", "mixed4_cauchy"]


# ---- 1. pieces ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MIXED)
def test_pieces_agree_with_the_restatement(ctx, name):
    """mocap_rig_linearize_intrinsics at the start of the case (C = 3 and 4, partial visibility, one camera at mask 0, one at
    0x1FF; without and with the Cauchy loss, c = 2), lambda = 1e-3: cost, gradient, S and reduced right-hand side against the
    restatement.  Kernels and restatement form every per-observation term by the same operations; they differ in the order of
    the sums.  The allowance is that of tests/test_gpu_rig_ba.py and tests/test_gpu_rig_robust.py for the same kind of sums: 8
    x the restatement's own largest spread under 10 seeded permutations of the observation order, each quantity relative to its
    largest entry, and for the cost 4 unit roundoffs more (log1p under the loss; and at 100-odd terms ten permutations can
    all give one cost, which allows nothing).
    Restatement's spread (CPU):  mixed3         cost 2.8e-16  gradient 3.5e-16  S 1.2e-15  rhs 5.0e-16
                                 mixed3_cauchy  cost 3.0e-16  gradient 4.9e-16  S 1.3e-15  rhs 8.4e-16
                                 mixed4         cost 1.5e-16  gradient 3.8e-16  S 8.8e-16  rhs 4.6e-16
                                 mixed4_cauchy  cost 2.5e-16  gradient 5.6e-16  S 1.4e-15  rhs 6.2e-16
    GPU - restatement (MI355X):  mixed3         cost 1.4e-15  gradient 4.0e-16  S 2.9e-16  rhs 1.7e-15
                                 mixed3_cauchy  cost 1.5e-16  gradient 1.5e-15  S 3.3e-15  rhs 2.3e-15
                                 mixed4         cost 1.0e-15  gradient 8.6e-16  S 1.8e-16  rhs 2.5e-15
                                 mixed4_cauchy  cost 7.4e-16  gradient 8.3e-16  S 1.7e-15  rhs 4.7e-15 (allowed 5.0e-15)
    (also DESIGN.md section 2)
    A fixed parameter: its row and column of S are zero but for the 1 on the diagonal, its gradient and rhs entries 0."""
    prob, kd, R, t, X, masks, loss_c, _ = sc.loop_case(name)
    spread = sc.order_spread(prob, kd, R, t, X, 1e-3, masks, loss_c)
    ref = sc.linearize(prob.sorted(), kd, R, t, X, 1e-3, masks, loss_c)
    got = ctx.rig_linearize_intrinsics(*prob.point_major(), kd, masks, poses12(R, t), X, 1e-3, **loss_args(loss_c))
    assert_pieces_agree(name, prob, masks, got, ref, spread)


# ---- 2. loop --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MIXED + ["wide7"])
def test_loop_walks_the_restatements_iterations(ctx, name):
    """Same accept / reject sequence, same number of iterations, same stopping rule as the restatement at ftol =
    rig_selfcal_ref.LOOP_FTOL (test_rig_selfcal_host.py: no |rho| < 1e-3, no relative decrease within a factor 1.2 of ftol).
    wide7: 7 cameras, 105 rows, more than the 90 the Cholesky holds in LDS -- the factorisation in global memory; 60 points,
    each seen by exactly 3 cameras.
    Per-iteration cost: allowed relative difference 1e-8, by the reasoning of tests/test_gpu_rig_ba.py's loop test: the two
    sides solve systems that agree to ~1e-15 (test 1); Marquardt's damping makes the step invariant under a scaling of the
    parameters, so the condition number that counts is that of S scaled to a unit diagonal, below 1e6 (asserted on the CPU,
    measured 3e3); steps then agree to ~1e-9 of their length and the cost, at most linearly sensitive to the state, to better
    than 1e-8 of itself.  The damping and the step lengths: damping_allowance, above (the plain test's flat 1e-6 holds for
    loops that stop on larger steps than these: here the last accepted steps lower the cost by some 1e-8 of itself, and rho, a
    ratio with that difference on top, carries the costs' rounding magnified).  The returned kd, poses and points: the iterates agree to ~1e-9 of a step's length per iteration, over
    some 20 iterations; each group of the returned state is allowed 1e-6 of what the group moved between the start and the
    returned state (per kd column the column's largest move, for R the largest rotation, for t and X their largest
    entries'), which leaves two orders of magnitude for a path that is longer than its displacement.
    Measured on the MI355X (mixed3, mixed3_cauchy, mixed4, mixed4_cauchy, wide7): iterations 19 / 19 / 11 / 11 / 20, all
    accepted, status ftol, as the restatement; largest relative cost difference 9.2e-12 / 2.3e-12 / 8.0e-14 / 1.7e-13 / 1.4e-13;
    kd against what it moved 6.3e-12 / 5.7e-11 / 5.7e-13 / 2.2e-12 / 6.6e-11, rotations, t and points 2.2e-12 / 2.3e-11 / 2.9e-13 /
    3.7e-13 / 7.9e-11; lambda 1.3e-7 / 4.1e-6 / 1.8e-10 / 1.8e-10 / 1.8e-7 (at the last iterations, where the allowance is 1e-4
    and more), step lengths 5.1e-9 / 3.3e-8 / 3.9e-9 / 1.4e-9 / 1.6e-7."""
    assert_loop_walks_the_restatements(ctx, name, sc.loop_case(name))


# ---- 3. masks, failures, bits -----------------------------------------------------------------------------------------------------
def test_fixed_parameters_come_back_with_their_bits(ctx):
    prob, kd, R, t, X, masks, _, ref = sc.loop_case("mixed4")
    got = adjust(ctx, prob, kd, R, t, X, masks)
    free = sc.free_columns(masks, prob.C)[:, :9]
    assert got["status"] > 0 and got["cost"] < 1e-2 * got["cost_initial"]
    assert got["intrinsics"][~free].tobytes() == kd[~free].tobytes()
    assert (got["intrinsics"][free] != kd[free]).all()
    # one parameter alone, in one camera alone
    one = np.array([0, 0, 0x010, 0])
    got = adjust(ctx, prob, kd, R, t, X, one, max_iters=5)
    keep = np.ones((4, 9), bool)
    keep[2, 4] = False
    assert got["intrinsics"][keep].tobytes() == kd[keep].tobytes() and got["intrinsics"][2, 4] != kd[2, 4]


def test_mask_zero_is_the_plain_adjustment_at_those_lenses(ctx):
    """Every mask 0: the problem of mocap_rig_bundle_adjust_robust with kd as the cameras' K and dist.  The two kernels sum in
    different orders, so the bar is the loop test's (same iterations, costs to 1e-8), not bits."""
    prob, kd, R, t, X, _, _, _ = sc.loop_case("mixed4")
    K = np.array([[[k[0], 0, k[2]], [0, k[1], k[3]], [0, 0, 1.0]] for k in kd])
    ctx.set_cameras(K, kd[:, 4:], R, t)
    plain = ctx.rig_bundle_adjust(*gpu_args(prob, R, t, X), ftol=sc.LOOP_FTOL, loss="none")
    got = adjust(ctx, prob, kd, R, t, X, 0, ftol=sc.LOOP_FTOL)
    assert got["intrinsics"].tobytes() == kd.tobytes()
    assert got["iterations"] == plain["iterations"] and got["status"] == plain["status"]
    assert np.abs(got["history"][:, 0] / plain["history"][:, 0] - 1).max() <= 1e-8
    assert np.abs(got["points"] - plain["points"]).max() <= 1e-6 * np.abs(plain["points"] - X).max()


def test_a_point_behind_a_camera_leaves_everything_as_it_was(ctx):
    prob, kd, R, t, X, masks, _, _ = sc.loop_case("mixed4")
    X2 = X.copy()
    n = prob.pt[prob.cam == 0][0]
    X2[n] = -X2[n]  # a point camera 0, the world frame, sees: now behind it
    from mocapv2_amd import _abi
    off, cam, uv = prob.point_major()
    with pytest.raises(_abi.MocapError) as e:
        adjust(ctx, prob, kd, R, t, X2, masks)
    assert e.value.code == -3
    # through the C-ABI, where the arrays can be looked at after the negative status
    rc, result, kd2, poses2, pts2, hist = adjust_raw(ctx, off, cam, uv, kd, masks, poses12(R, t), X2, prob.C, prob.N)
    assert rc == 0 and result[0] == -3
    assert kd2.tobytes() == kd.tobytes()
    assert poses2.tobytes() == poses12(R, t).tobytes() and pts2.tobytes() == X2.tobytes()
    assert not hist.any()


def test_two_runs_give_the_same_bits_also_after_a_larger_problem(ctx):
    prob, kd, R, t, X, masks, loss_c, _ = sc.loop_case("mixed4_cauchy")
    big = sc.loop_case("wide7")

    def run():
        out = adjust(ctx, prob, kd, R, t, X, masks, loss_c)
        lin = ctx.rig_linearize_intrinsics(*prob.point_major(), kd, masks, poses12(R, t), X, 1e-3, **loss_args(loss_c))
        return out, lin

    a, la = run()
    b, lb = run()
    adjust(ctx, big[0], *big[1:5], big[5], max_iters=3)  # unrelated, larger: the scratch is carved anew
    d, ld = run()
    for other, lin in ((b, lb), (d, ld)):
        for k in ("intrinsics", "poses", "points", "history", "obs_err", "obs_weight"):
            assert a[k].tobytes() == other[k].tobytes(), k
        assert (a["status"], a["iterations"], a["cost"], a["cost_initial"]) == (other["status"], other["iterations"], other["cost"], other["cost_initial"])
        for k in ("gradient", "S", "rhs"):
            assert la[k].tobytes() == lin[k].tobytes(), k
        assert la["cost"] == lin["cost"]


def test_a_camera_with_too_few_observations_for_its_mask_is_a_layout_error(ctx):
    """Camera 2 is left with 17 observations: one short of twice the nine parameters of mask 0x1FF, enough for the eight of 0x0FF"""
    import rig_robust_ref as rr
    from mocapv2_amd import _abi
    prob, kd, R, t, X, _, _, _ = sc.loop_case("mixed4")
    thin, points = rr.without(prob, np.flatnonzero(prob.cam == 2)[17:])
    assert np.bincount(thin.cam, minlength=4)[2] == 17
    masks = np.array([0x1FF, 0x1FF, 0x1FF, 0x1FF])
    assert not sc.layout_ok(thin, masks)
    with pytest.raises(_abi.MocapError) as e:
        adjust(ctx, thin, kd, R, t, X[points], masks, max_iters=3)
    assert e.value.code == -2
    with pytest.raises(_abi.MocapError) as e:
        ctx.rig_linearize_intrinsics(*thin.point_major(), kd, masks, poses12(R, t), X[points], 1e-3)
    assert e.value.code == -2
    for ok in ([0x1FF, 0x1FF, 0x0FF, 0x1FF], [0x1FF, 0x1FF, 0, 0x1FF]):
        assert sc.layout_ok(thin, ok) and adjust(ctx, thin, kd, R, t, X[points], np.array(ok), max_iters=3)["status"] > 0


def test_bad_masks_and_bad_lenses_are_invalid_arguments(ctx):
    from mocapv2_amd import _abi
    prob, kd, R, t, X, masks, _, _ = sc.loop_case("mixed3")
    for bad in (np.array([0, 0x200, 0]), np.array([-1, 0, 0]), 0x3FF):
        with pytest.raises(_abi.MocapError) as e:
            adjust(ctx, prob, kd, R, t, X, bad, max_iters=2)
        assert e.value.code == -1
    for i, j, v in ((0, 0, 0.0), (1, 1, -1400.0), (2, 4, np.nan), (0, 8, np.inf), (1, 0, np.nan)):
        k2 = kd.copy()
        k2[i, j] = v
        with pytest.raises(_abi.MocapError) as e:
            adjust(ctx, prob, k2, R, t, X, masks, max_iters=2)
        assert e.value.code == -1
        with pytest.raises(_abi.MocapError) as e:
            ctx.rig_linearize_intrinsics(*prob.point_major(), k2, masks, poses12(R, t), X, 1e-3)
        assert e.value.code == -1
    assert adjust(ctx, prob, kd, R, t, X, masks, max_iters=2)["status"] > 0  # the context is as good as before


# ---- 4. the Python surface ---------------------------------------------------------------------------------------------------------
def test_bundle_adjust_rig_refines_the_lenses_and_says_what_moved(ctx):
    """calibrate.bundle_adjust_rig_intrinsics on mixed4's rig and start (camera_params of checkerboard grade, start points handed in, so
    that the device starts where the restatement does) with refine_intrinsics="focal+center+radial2": it returns camera_params
    and intrinsics_start, ends at the restatement's cost (1e-6 allowed: this mask's loop is not among those shown to be far
    from ftol's boundary, and either side stopping a step apart changes the cost by less than ftol = 2e-8 of itself) and
    below the cost the fixed lenses leave; the Cauchy stage and its refit keep the mask.
    Restatement (CPU): refined 0.1736 px in 42 iterations, fixed lenses 0.2082 px; the GPU: the same three figures."""
    from mocapv2_amd import calibrate
    prob, kd0, R, t, X, _, _, _ = sc.loop_case("mixed4")
    ip, valid = np.zeros((prob.C, prob.N, 2)), np.zeros((prob.C, prob.N), bool)
    ip[prob.cam, prob.pt], valid[prob.cam, prob.pt] = prob.uv, True
    params = calibrate._camera_entries(kd0)
    poses = [{"R": R[k], "t": t[k]} for k in range(prob.C)]
    poses[0] = {"R": np.eye(3), "t": np.zeros(3)}
    kw = {"points": X, "ftol": sc.LOOP_FTOL, "ctx": ctx}
    fixed = calibrate.bundle_adjust_rig(ip, valid, poses, params, **kw)
    out = calibrate.bundle_adjust_rig_intrinsics(ip, valid, poses, params, refine_intrinsics="focal+center+radial2", **kw)
    assert "camera_params" not in fixed and out["used"].all() and out["status"] > 0

    def kd_of(entries):
        return np.array([np.r_[p["intrinsic_matrix"][0, 0], p["intrinsic_matrix"][1, 1], p["intrinsic_matrix"][0, 2], p["intrinsic_matrix"][1, 2],
                               p["distortion_coef"]] for p in entries])

    got = kd_of(out["camera_params"])
    assert kd_of(out["intrinsics_start"]).tobytes() == kd0.tobytes()
    assert got[:, 6:].tobytes() == kd0[:, 6:].tobytes() and (got[:, :6] != kd0[:, :6]).all()
    ref = sc.lm(prob, kd0, R, t, X, sc.MASKS["focal+center+radial2"], ftol=sc.LOOP_FTOL)
    print(f"rms: fixed {fixed['rms_px']:.4f} px  refined {out['rms_px']:.4f} px in {out['iterations']} iterations  restatement "
          f"{sc.rms_px(prob, ref['cost']):.4f} px in {ref['iterations']}")
    assert abs(out["cost"] / ref["cost"] - 1) <= 1e-6 and np.abs(got - ref["kd"]).max() <= 1e-3 * np.abs(ref["kd"] - kd0).max()
    assert out["cost"] < fixed["cost"]
    robust = calibrate.bundle_adjust_rig_intrinsics(ip, valid, poses, params, loss="cauchy", loss_scale=2.0, **kw)  # (the default mask)
    kr = kd_of(robust["camera_params"])
    assert kr[:, 6:].tobytes() == kd0[:, 6:].tobytes() and (kr[:, :6] != kd0[:, :6]).all()
    assert not robust["outliers"].any() and abs(robust["cost"] / out["cost"] - 1) <= 1e-6
    assert kd_of(robust["intrinsics_start"]).tobytes() == kd0.tobytes()
    with pytest.raises(ValueError):
        calibrate.bundle_adjust_rig_intrinsics(ip[:2], valid[:2], poses[:2], params[:2], ctx=ctx, refine_intrinsics="focal+center")
