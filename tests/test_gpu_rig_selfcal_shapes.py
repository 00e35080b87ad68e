"""The lens-refining rig adjustment (csrc/rig_selfcal.hip) at the shapes tests/test_gpu_rig_selfcal.py does not reach, against
the same NumPy restatement (tests/rig_selfcal_ref.py, SHAPE_CASES): more than one workgroup of points (255, 256, 257, 513 and
594 points: 1, 1, 2, 3 and 3 workgroups of the point kernels and chunks of the Schur kernel), 90 rows, the last size the
Cholesky factorises in LDS, two cameras, 32 cameras (480 rows, 528 camera pairs, bit 31 of the visibility masks, the factor in
global memory), and 65 537 points, where the Schur kernel's chunk grows to 257 points.  tests/test_rig_selfcal_host.py shows
on the CPU that every case has the shape it is named for and that its loop is far from every decision boundary.  A case's
restatement is computed once (rig_selfcal_ref.shape_case) and shared by the tests here."""
import time

import numpy as np
import pytest

import rig_selfcal_ref as sc
from rig_selfcal_gpu import PIECES, adjust, adjust_raw, assert_loop_walks_the_restatements, assert_pieces_agree, linearize, poses12

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from mocapv2_amd.engine import MocapContext
    return MocapContext(1, 1)


# ---- 1. pieces ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [k for k in sc.SHAPE_CASES if k != "chunk_growth"])
def test_pieces_agree_with_the_restatement(ctx, name):
    """mocap_rig_linearize_intrinsics at the start of every case, lambda = 1e-3, against the restatement, with the allowance of
    tests/test_gpu_rig_selfcal.py's pieces test: 8 x the restatement's own spread under 10 seeded permutations of the
    observation order, each quantity relative to its largest entry, 4 unit roundoffs more for the cost; S symmetric to the bit;
    fixed columns the identity's.
    Restatement's spread (CPU), then GPU - restatement (MI355X), each cost / gradient / S / rhs (also DESIGN.md section 2):
      two             1.3e-16 / 9.1e-16 / 2.7e-15 / 6.7e-15    0       / 2.6e-16 / 1.3e-15 / 6.7e-16
      six_lds         1.9e-16 / 3.3e-16 / 7.1e-16 / 9.5e-16    0       / 1.6e-16 / 2.9e-16 / 3.2e-16
      six_600         1.4e-16 / 1.4e-15 / 2.4e-15 / 2.8e-15    1.4e-16 / 5.1e-16 / 8.1e-16 / 1.4e-15
      six_600_cauchy  0       / 1.6e-15 / 2.6e-15 / 1.9e-15    0       / 6.7e-16 / 1.2e-15 / 6.9e-16
      blocks_255      0       / 6.7e-16 / 2.6e-15 / 1.2e-15    0       / 5.0e-16 / 1.2e-15 / 7.0e-16
      blocks_256      0       / 1.0e-15 / 1.9e-15 / 1.6e-15    0       / 5.0e-16 / 1.2e-15 / 7.0e-16
      blocks_257      0       / 1.0e-15 / 2.6e-15 / 1.4e-15    0       / 5.0e-16 / 1.2e-15 / 7.0e-16
      blocks_513      2.1e-16 / 1.4e-15 / 2.7e-15 / 1.8e-15    0       / 3.5e-16 / 1.3e-15 / 4.5e-16
      rig32           0       / 8.6e-16 / 9.9e-16 / 9.0e-16    0       / 6.9e-16 / 5.7e-16 / 7.2e-16 (allowed 7.2e-15)
      rig32_cauchy    1.2e-16 / 7.0e-16 / 1.0e-15 / 7.1e-16    0       / 4.3e-16 / 4.7e-16 / 4.4e-16
    Where ten permutations all give one cost the cost's allowance is the 4 unit roundoffs, 4.4e-16.  The start of these cases
    has camera 0 exactly at the world frame (rig_selfcal_ref.shape_case), as the device makes it: with perturbed_start's camera
    0, a few 1e-16 off, the restatement's residuals of camera 0 differ from the device's in their last bits and `two`'s cost
    by 2.5e-15."""
    prob, kd, R, t, X, masks, loss_c, _ = sc.shape_case(name)
    ref = sc.linearize(prob, kd, R, t, X, 1e-3, masks, loss_c)
    spread = sc.order_spread(prob, kd, R, t, X, 1e-3, masks, loss_c, base=ref)
    assert_pieces_agree(name, prob, masks, linearize(ctx, prob, kd, R, t, X, masks, loss_c), ref, spread)


def test_pieces_agree_where_the_schur_chunk_grows(ctx):
    """chunk_growth: 2 cameras, 65 537 points, one more than 256 chunks of 256: the Schur kernel's workgroups take 257 points
    each and the last one 2; 257 workgroups of the point kernels.  The same comparison and allowance as above, but the spread
    from 2 seeded permutations, not 10: one linearisation of the restatement takes about 3 s, and with the case itself, the
    sorted problem's pieces and the check below the test is at 4 to 11 seconds of CPU (the device's part is milliseconds).
    A spread from fewer permutations is no larger, so the bound is no wider.  That it still catches one lost point is shown
    here on the CPU: the restatement without its last point differs from the full one in S and in rhs by more than 100 x what
    is allowed (measured 1.7e-5 and 5.8e-5 of the largest entry against allowances of 1.5e-13 and 8.5e-13).
    Restatement's spread (CPU, 2 permutations): cost 2.8e-16  gradient 6.6e-15  S 1.9e-14  rhs 1.1e-13
    GPU - restatement (MI355X):                 cost 1.4e-16  gradient 1.0e-14  S 1.3e-14  rhs 7.4e-14
    allowed:                                    cost 2.7e-15  gradient 5.3e-14  S 1.5e-13  rhs 8.7e-13   (also DESIGN.md section 2)"""
    t0 = time.process_time()
    prob, kd, R, t, X, masks, loss_c, _ = sc.shape_case("chunk_growth")
    assert sc.schur_chunks(prob.N) == (257, 256) and sc.lin_blocks(prob.N) == 257
    ref = sc.linearize(prob, kd, R, t, X, 1e-3, masks, loss_c)
    spread = sc.order_spread(prob, kd, R, t, X, 1e-3, masks, loss_c, n_perm=2, base=ref)
    less, X_less = sc.first_points(prob, X, prob.N - 1)
    lost = sc.linearize(less, kd, R, t, X_less, 1e-3, masks, loss_c)
    for k in ("S", "rhs"):
        d = float(np.abs(ref[k] - lost[k]).max() / np.abs(ref[k]).max())
        print(f"chunk_growth {k}: without the last point {d:.3e}  allowed {8 * spread[k]:.3e}")
        assert d > 100 * 8 * spread[k], k
    print(f"chunk_growth: CPU {time.process_time() - t0:.1f} s")
    assert_pieces_agree("chunk_growth", prob, masks, linearize(ctx, prob, kd, R, t, X, masks, loss_c), ref, spread)


# ---- 2. loop --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["two", "six_lds", "six_600", "six_600_cauchy", "blocks_257", "rig32", "rig32_cauchy"])
def test_loop_walks_the_restatements_iterations(ctx, name):
    """The assertions and bounds of tests/test_gpu_rig_selfcal.py's loop test (its docstring has the reasoning), which rest on a
    scaled cond(S) below 1e6 and on the distance from the decision boundaries that tests/test_rig_selfcal_host.py asserts for
    exactly these cases: the same iterations, status and accept / reject sequence as the restatement at LOOP_FTOL, per-iteration
    cost within 1e-8, lambda within damping_allowance, step lengths within 1e-6 plus that, the returned kd, poses and points
    within 1e-6 of what they moved, the gauge, obs_err reproducing the cost.
    Measured on the MI355X (two, six_lds, six_600, six_600_cauchy, blocks_257, rig32, rig32_cauchy): iterations 13 / 10 / 9 / 9 /
    9 / 12 / 12, all accepted, status ftol, as the restatement; largest relative cost difference 5.8e-14 / 7.4e-14 / 2.3e-14 /
    6.7e-14 / 4.0e-14 / 1.2e-13 / 7.8e-13; kd against what it moved 3.2e-12 / 6.0e-13 / 9.6e-13 / 9.6e-13 / 1.7e-12 / 1.4e-12 /
    2.4e-12, rotations, t and points 1.6e-12 / 4.7e-13 / 1.8e-13 / 1.4e-13 / 1.7e-13 / 1.6e-12 / 2.3e-12; lambda 1.5e-9 for two
    and to the bit for the rest (every step's factor there is the floor of 1/3); step lengths 3.3e-9 / 2.7e-10 / 4.1e-10 /
    1.5e-10 / 1.4e-10 / 2.5e-9 / 1.8e-9."""
    assert_loop_walks_the_restatements(ctx, name, sc.shape_case(name))


# ---- 3. order and bits across workgroups -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["blocks_513", "rig32"])
def test_two_runs_give_the_same_bits_also_after_a_larger_problem(name):
    """Three workgroups' partials (blocks_513), and 528 pairs with the factor in global memory (rig32), on a context of the
    test's own, whose scratch the first call sizes: the same call twice gives the same bytes in every output, and again after
    a call on chunk_growth's problem, whose 131 074 W blocks alone are several times twice what either case needs: the
    scratch is regrown and lies elsewhere."""
    from mocapv2_amd.engine import MocapContext
    own = MocapContext(1, 1)
    prob, kd, R, t, X, masks, loss_c, _ = sc.shape_case(name)
    big = sc.shape_case("chunk_growth")
    assert len(big[0].pt) > 40 * len(prob.pt)

    def run():
        return adjust(own, prob, kd, R, t, X, masks, loss_c), linearize(own, prob, kd, R, t, X, masks, loss_c)

    a, la = run()
    b, lb = run()
    adjust(own, big[0], *big[1:5], big[5], max_iters=3)
    d, ld = run()
    assert a["status"] > 0 and a["iterations"] > 3
    for other, lin in ((b, lb), (d, ld)):
        for k in ("intrinsics", "poses", "points", "history", "obs_err", "obs_weight"):
            assert a[k].tobytes() == other[k].tobytes(), k
        assert (a["status"], a["iterations"], a["cost"], a["cost_initial"]) == (other["status"], other["iterations"], other["cost"], other["cost_initial"])
        for k in PIECES[1:]:
            assert la[k].tobytes() == lin[k].tobytes(), k
        assert la["cost"] == lin["cost"]


# ---- 4. flags raised outside workgroup 0 -----------------------------------------------------------------------------------------
def test_a_point_behind_a_camera_in_another_workgroup_leaves_everything_as_it_was(ctx):
    """blocks_513, a point of the second workgroup and the one of the third (index 256 and 512), each mirrored through the
    centre of the first camera that sees it, which negates its coordinates in that camera's frame: MOCAP_RIG_E_BEHIND, and the
    caller's kd, poses and points keep their bytes"""
    from mocapv2_amd import _abi
    prob, kd, R, t, X, masks, _, _ = sc.shape_case("blocks_513")
    off, cam, uv = prob.point_major()
    for n in (256, 512):
        c = prob.cam[prob.pt == n][0]
        X2 = X.copy()
        X2[n] = 2 * (-R[c].T @ t[c]) - X[n]
        assert (R[c] @ X2[n] + t[c])[2] < 0
        assert linearize(ctx, prob, kd, R, t, X2, masks)["behind"]
        with pytest.raises(_abi.MocapError) as e:
            adjust(ctx, prob, kd, R, t, X2, masks)
        assert e.value.code == -3
        rc, result, kd2, poses2, pts2, hist = adjust_raw(ctx, off, cam, uv, kd, masks, poses12(R, t), X2, prob.C, prob.N)
        assert rc == 0 and result[0] == -3
        assert kd2.tobytes() == kd.tobytes() and poses2.tobytes() == poses12(R, t).tobytes() and pts2.tobytes() == X2.tobytes()
        assert not hist.any()
    assert not linearize(ctx, prob, kd, R, t, X, masks)["behind"]  # the flag does not outlive the call


def test_descending_cameras_of_a_point_in_another_workgroup_are_a_layout_error(ctx):
    """blocks_513, a point with index >= 256 whose first two obs_cam entries are swapped.  The Python surface refuses the arrays
    on the host; through the C-ABI the device's own check, made by the workgroup that owns the point, gives
    MOCAP_RIG_E_LAYOUT, and nothing is written"""
    prob, kd, R, t, X, masks, _, _ = sc.shape_case("blocks_513")
    off, cam, uv = prob.point_major()
    for n in (300, 512):
        cam2 = cam.copy()
        o = off[n]
        cam2[o], cam2[o + 1] = cam[o + 1], cam[o]
        assert cam2[o] > cam2[o + 1]
        with pytest.raises(ValueError):
            ctx.rig_bundle_adjust_intrinsics(off, cam2, uv, kd, masks, poses12(R, t), X, max_iters=3)
        rc, result, kd2, poses2, pts2, hist = adjust_raw(ctx, off, cam2, uv, kd, masks, poses12(R, t), X, prob.C, prob.N)
        assert rc == 0 and result[0] == -2
        assert kd2.tobytes() == kd.tobytes() and poses2.tobytes() == poses12(R, t).tobytes() and pts2.tobytes() == X.tobytes()
        assert not hist.any()
    assert adjust(ctx, prob, kd, R, t, X, masks, max_iters=2)["status"] > 0  # the context is as good as before
