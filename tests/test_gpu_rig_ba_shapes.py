"""The pose-only rig adjustment (csrc/rig_ba.hip on csrc/rig_lm.h's phases, PoseBlock) at the shapes tests/test_gpu_rig_ba.py and
tests/test_gpu_rig_robust.py do not reach, against the same NumPy restatements (tests/rig_ba_ref.py, SHAPE_CASES;
tests/rig_robust_ref.py under the Cauchy loss): 255, 256 and 257 points (1, 1 and 2 workgroups of the point kernels); 1023, 1024,
1025 and 2049 points (1, 1, 2 and 3 chunks of rig_schur_kernel, the last of one point); 17 cameras, 96 rows, the first size the
Cholesky factorises in global memory; 32 cameras under the loss (bit 31 of the visibility masks, 496 camera pairs); two cameras
(one pair); and 87 382 and 262 145 points of two cameras, where the 3 N loops and the per-point loop of rig_init_kernel and
rig_finish_kernel take a second trip through their 262 144 threads.  tests/test_rig_ba_host.py shows on the CPU that every case
has the shape it is named for, that a seam case's last point cannot be lost unseen, and that the loops are far from every
decision boundary.  A case, its restatement's pieces and its loop are computed once (rig_ba_ref.shape_case, shape_pieces,
shape_loop) and shared by the tests here."""
import time

import numpy as np
import pytest

import rig_ba_ref as rb
import rig_selfcal_ref as sc
from rig_ba_gpu import E_BEHIND, E_LAYOUT, PIECES, adjust, adjust_raw, assert_loop_walks_the_restatements, assert_pieces_agree, linearize, poses12

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from mocapv2_amd.engine import MocapContext
    return MocapContext(1, 1)


# ---- 1. pieces ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(rb.SHAPE_CASES))
def test_pieces_agree_with_the_restatement(ctx, name):
    """mocap_rig_linearize (mocap_rig_linearize_robust, Cauchy, c = 2, for the _cauchy cases) at the start of every case, lambda =
    1e-3, against the restatement of the sorted problem, with the allowance of tests/test_gpu_rig_ba.py's and
    tests/test_gpu_rig_robust.py's pieces tests: 8 x the restatement's own spread under 10 seeded permutations of the
    observation order, each quantity relative to its largest entry, 4 unit roundoffs more for the cost (where all permutations
    give one cost that is all it gets); S symmetric to the bit; nothing behind.  The two pose_stride_* cases take their spread
    from 2 permutations (one linearisation of the restatement takes seconds there; tests/test_gpu_rig_selfcal_shapes.py's
    chunk_growth is the precedent): a spread from fewer permutations is no larger, so the bound is no wider, and
    tests/test_rig_ba_host.py shows that it still catches one lost point by a factor of more than 100.
    Restatement's spread (CPU), then GPU - restatement (MI355X), each cost / gradient / S / rhs (also DESIGN.md section 2):
      pose_two          0       / 1.6e-15 / 3.2e-15 / 2.8e-15    0       / 5.2e-16 / 2.9e-15 / 1.5e-15
      pose_255          1.9e-16 / 5.5e-16 / 3.1e-15 / 1.3e-15    1.9e-16 / 1.0e-16 / 1.6e-15 / 3.9e-16
      pose_256          1.9e-16 / 4.1e-16 / 4.0e-15 / 1.0e-15    0       / 1.0e-16 / 1.5e-15 / 3.8e-16
      pose_257          1.9e-16 / 5.5e-16 / 4.1e-15 / 1.1e-15    1.9e-16 / 1.0e-16 / 1.6e-15 / 3.8e-16
      pose_1023         2.6e-16 / 1.6e-15 / 4.8e-15 / 4.4e-15    1.3e-16 / 1.1e-15 / 1.1e-15 / 2.2e-15
      pose_1024         1.3e-16 / 1.7e-15 / 5.1e-15 / 5.7e-15    0       / 1.1e-15 / 1.3e-15 / 2.5e-15
      pose_1025         2.6e-16 / 1.6e-15 / 4.8e-15 / 5.5e-15    1.3e-16 / 1.1e-15 / 1.3e-15 / 2.5e-15
      pose_2049_cauchy  0       / 1.4e-15 / 8.1e-15 / 3.4e-15    0       / 4.6e-16 / 2.1e-15 / 8.5e-16
      pose_c17          1.4e-16 / 6.6e-16 / 1.4e-15 / 5.4e-16    0       / 3.7e-16 / 6.1e-16 / 4.2e-16
      pose_c17_cauchy   1.3e-16 / 7.8e-16 / 1.8e-15 / 8.6e-16    0       / 6.2e-16 / 1.1e-15 / 6.9e-16
      pose_c32_cauchy   1.4e-16 / 1.1e-15 / 7.6e-16 / 1.0e-15    0       / 7.4e-16 / 5.1e-16 / 6.9e-16
      pose_stride_3n    4.8e-16 / 1.5e-14 / 4.0e-14 / 2.0e-14    4.8e-16 / 8.7e-15 / 4.1e-14 / 1.3e-14 (allowed 4.3e-15 / 1.2e-13 / 3.2e-13 / 1.6e-13)
      pose_stride_n     5.0e-16 / 9.4e-15 / 5.2e-14 / 1.9e-14    1.7e-15 / 8.0e-15 / 3.8e-14 / 9.6e-15 (allowed 4.4e-15 / 7.5e-14 / 4.2e-13 / 1.5e-13)"""
    t0 = time.process_time()
    case = rb.shape_case(name)
    ref, spread = rb.shape_pieces(name)
    print(f"{name}: C {case['prob'].C}  N {case['prob'].N}  observations {len(case['prob'].pt)}  CPU {time.process_time() - t0:.1f} s")
    assert_pieces_agree(name, linearize(ctx, case), ref, spread)


# ---- 2. loop --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", rb.SHAPE_LOOPS)
def test_loop_walks_the_restatements_iterations(ctx, name):
    """The assertions and bars of tests/test_gpu_rig_ba.py's loop test (its docstring has the reasoning), which rest on a cond(S)
    below 1e6 and on no |rho| below 1e-3, both asserted for exactly these cases by tests/test_rig_ba_host.py: the same
    iterations, status and accept / reject sequence as the restatement at LOOP_FTOL, per-iteration cost within 1e-8, lambda and
    step lengths within 1e-6, the initial cost within 1e-12.  And of the returned state: poses and points within 1e-6 of what
    they moved, camera 0 the world frame and |t_1| the start's, 1/2 sum obs_err^2 (sum rho under the loss) the returned cost,
    and under the loss obs_err and obs_weight against rig_robust_ref.errors_and_weights at the restatement's result (1e-6, the
    bar of tests/test_gpu_rig_robust.py).
    Measured on the MI355X (pose_two, pose_257, pose_1025, pose_2049_cauchy, pose_c17, pose_c17_cauchy, pose_c32_cauchy): iterations
    6 / 5 / 5 / 13 / 6 / 8 / 7, all accepted, status ftol, as the restatement; largest relative cost difference 4.1e-14 / 2.1e-14 /
    4.6e-14 / 4.8e-15 / 8.3e-14 / 1.7e-14 / 9.3e-15; rotations, t and points against what they moved 6.2e-14 / 3.4e-14 / 7.6e-14 /
    1.6e-13 / 3.2e-14 / 3.4e-14 / 9.7e-14; lambda to the bit (every step's factor is the floor of 1/3); step lengths 1.2e-7 / 6.6e-9 /
    1.0e-9 / 5.0e-8 / 3.6e-10 / 2.2e-9 / 3.3e-9; the cost from obs_err within 1.0e-14; under the loss obs_err 1.4e-10 / 3.2e-11 /
    2.0e-11 and obs_weight 2.1e-13 / 2.0e-13 / 2.4e-13.  (pose_2049_cauchy was first tried at a seed whose loop takes 19 iterations:
    everything above inside its bar, but step lengths 3.9e-4 off -- as far as the restatement is from itself under another order
    of its sums, tests/test_rig_ba_host.py::test_shape_loop_cases_are_far_from_every_decision_boundary has the reason.)"""
    assert_loop_walks_the_restatements(ctx, name)


# ---- 3. the grid-stride loops of init and finish -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", rb.SHAPE_STRIDES)
def test_two_iterations_past_the_grid_of_init_and_finish(ctx, name):
    """pose_stride_3n: 3 N = 262 146, two elements more than rig_init_kernel's and rig_finish_kernel's 1024 x 256 threads;
    pose_stride_n: N = 262 145, one point more.  max_iters = 2, checked by properties (a loop of the restatement would take a
    minute): the initial cost is the restatement's at the start (1e-12: a point init did not copy, or a mask it did not build,
    changes it by about 1 / N); the status is positive; 1/2 sum obs_err^2, computed from the arrays handed back, is the returned
    cost (1e-12 relative: a point finish did not hand back is one the residuals kernel reads at its start); and every returned
    point differs from its start, those of the second trip included.
    Measured on the MI355X (pose_stride_3n, pose_stride_n): status max_iters after 2 accepted iterations; cost_initial /
    restatement's - 1 = 4.4e-16 / 1.6e-15; the cost from obs_err / cost - 1 = 4.4e-16 / 2.2e-16; no coordinate of 262 146 / 786 435
    kept its bytes."""
    t0 = time.process_time()
    case = rb.shape_case(name)
    prob, X = case["prob"], case["X"]
    cost0, front = rb.cost_of(prob, case["R"], case["t"], X)
    got = adjust(ctx, case, max_iters=2, loss="none")
    again = 0.5 * float(np.sum(got["obs_err"] ** 2))
    same = (got["points"] == X).reshape(-1)
    print(f"{name}: N {prob.N}  3 N {3 * prob.N}  status {got['status']}  iterations {got['iterations']}  cost_initial / restatement - 1 "
          f"{got['cost_initial'] / cost0 - 1:.3e}  cost {got['cost']!r}  obs_err's cost / cost - 1 {again / got['cost'] - 1:.3e}  coordinates "
          f"that kept their bytes {int(same.sum())} of {same.size}, beyond 262 144: {int(same[262144:].sum())} of {same.size - 262144}  "
          f"CPU {time.process_time() - t0:.1f} s")
    assert front and 3 * prob.N > 262144 and same.size - 262144 == {"pose_stride_3n": 2, "pose_stride_n": 3 * 262145 - 262144}[name]
    assert got["status"] > 0 and got["iterations"] == 2 and got["cost"] < got["cost_initial"]
    assert abs(got["cost_initial"] / cost0 - 1) <= 1e-12
    assert abs(again / got["cost"] - 1) <= 1e-12
    assert (got["points"] != X).any(axis=1).all()
    assert not same[262144:].any() and (got["points"][87381:] != X[87381:]).all()


def test_a_layout_error_at_the_last_point_of_the_second_trip_is_found(ctx):
    """pose_stride_n through the C-ABI with the two cameras of point 262 144 swapped: the one point that rig_init_kernel's
    per-point loop reaches on its second trip.  MOCAP_RIG_E_LAYOUT, and poses, points and history keep their bytes."""
    case = rb.shape_case("pose_stride_n")
    off, cam, uv = case["prob"].point_major()
    n = 262144
    assert n == case["prob"].N - 1 and off[n + 1] - off[n] == 2
    cam2 = cam.copy()
    cam2[off[n]], cam2[off[n] + 1] = cam[off[n] + 1], cam[off[n]]
    assert cam2[off[n]] > cam2[off[n] + 1]
    rc, result, poses2, pts2, hist = adjust_raw(ctx, case, off, cam2, uv, case["X"], max_iters=2)
    assert rc == 0 and result[0] == E_LAYOUT
    assert poses2.tobytes() == poses12(case["R"], case["t"]).tobytes() and pts2.tobytes() == case["X"].tobytes()
    assert not hist.any()
    rc, result, _, pts2, hist = adjust_raw(ctx, case, off, cam, uv, case["X"], max_iters=2)  # the arrays as they were: the call is fine
    assert rc == 0 and result[0] > 0 and hist.any() and pts2.tobytes() != case["X"].tobytes()


# ---- 4. the other solver as a second yardstick -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["pose_1025", "pose_c17"])
def test_the_lens_solver_with_every_mask_zero_walks_the_same_loop(ctx, name):
    """mocap_rig_bundle_adjust_intrinsics with every mask 0 and kd from the cameras' K and dist is this solver's problem, solved
    by other kernels (15-wide blocks, camera 0's among them, a Schur kernel of its own, 256-point chunks): the bar of
    tests/test_gpu_rig_selfcal.py::test_mask_zero_is_the_plain_adjustment_at_those_lenses -- the same iterations and status,
    costs to 1e-8, points to 1e-6 of what they moved, kd's bytes unchanged.
    Measured on the MI355X (pose_1025, pose_c17): 5 and 6 iterations on both sides, the restatement's; costs 1.0e-13 / 5.9e-14;
    points against what they moved 5.0e-14 / 9.1e-15."""
    case = rb.shape_case(name)
    prob, R, t, X = (case[k] for k in ("prob", "R", "t", "X"))
    kd = sc.kd_of(prob)
    plain = adjust(ctx, case, ftol=rb.LOOP_FTOL)
    got = ctx.rig_bundle_adjust_intrinsics(*prob.point_major(), kd, 0, poses12(R, t), X, ftol=rb.LOOP_FTOL)
    cost_rel = np.abs(got["history"][:, 0] / plain["history"][:, 0] - 1).max() if got["iterations"] == plain["iterations"] else np.nan
    print(f"{name}: iterations {got['iterations']} / {plain['iterations']}  status {got['status']} / {plain['status']}  cost {cost_rel:.1e}  "
          f"points / moved {np.abs(got['points'] - plain['points']).max() / np.abs(plain['points'] - X).max():.1e}")
    assert got["intrinsics"].tobytes() == kd.tobytes()
    assert got["iterations"] == plain["iterations"] == rb.shape_loop(name)["iterations"] and got["status"] == plain["status"]
    assert cost_rel <= 1e-8
    assert np.abs(got["points"] - plain["points"]).max() <= 1e-6 * np.abs(plain["points"] - X).max()


# ---- 5. bits --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["pose_1025", "pose_c17"])
def test_two_runs_give_the_same_bits_also_after_a_larger_problem(name):
    """Five workgroups' and two chunks' partials (pose_1025), and 136 pairs with the factor in global memory (pose_c17), on a
    context of the test's own, whose scratch the first call sizes: the same calls twice give the same bytes in every output and
    every piece, and again after a call on pose_stride_n's problem, whose W blocks alone are many times twice what either case
    needs: the scratch is regrown and lies elsewhere."""
    from mocapv2_amd.engine import MocapContext
    own = MocapContext(1, 1)
    case, big = rb.shape_case(name), rb.shape_case("pose_stride_n")
    assert len(big["prob"].pt) > 40 * len(case["prob"].pt)

    def run():
        return adjust(own, case, loss="none"), linearize(own, case)

    a, la = run()
    b, lb = run()
    assert adjust(own, big, max_iters=2)["status"] > 0
    d, ld = run()
    assert a["status"] > 0 and a["iterations"] > 3
    for other, lin in ((b, lb), (d, ld)):
        for k in ("poses", "points", "history", "obs_err", "obs_weight"):
            assert a[k].tobytes() == other[k].tobytes(), k
        assert (a["status"], a["iterations"], a["cost"], a["cost_initial"]) == (other["status"], other["iterations"], other["cost"], other["cost_initial"])
        for k in PIECES[1:]:
            assert la[k].tobytes() == lin[k].tobytes(), k
        assert la["cost"] == lin["cost"] and la["behind"] == lin["behind"]


# ---- 6. flags raised outside workgroup 0 -----------------------------------------------------------------------------------------
def test_a_point_behind_a_camera_in_another_workgroup_leaves_everything_as_it_was(ctx):
    """pose_1025, the first point of the second workgroup and the one of the fifth, which is also the second Schur chunk's (index
    256 and 1024), each mirrored through the centre of the first camera that sees it, which negates its coordinates in that
    camera's frame: MOCAP_RIG_E_BEHIND, mocap_rig_linearize reports `behind`, the caller's poses and points keep their bytes,
    and the flag does not outlive the call"""
    from mocapv2_amd import _abi
    case = rb.shape_case("pose_1025")
    prob, R, t, X = (case[k] for k in ("prob", "R", "t", "X"))
    off, cam, uv = prob.point_major()
    for n in (256, 1024):
        c = prob.cam[prob.pt == n][0]
        X2 = X.copy()
        X2[n] = 2 * (-R[c].T @ t[c]) - X[n]
        assert (R[c] @ X2[n] + t[c])[2] < 0
        assert linearize(ctx, case, X2)["behind"]
        with pytest.raises(_abi.MocapError) as e:
            adjust(ctx, case, X2)
        assert e.value.code == E_BEHIND
        rc, result, poses2, pts2, hist = adjust_raw(ctx, case, off, cam, uv, X2)
        assert rc == 0 and result[0] == E_BEHIND
        assert poses2.tobytes() == poses12(R, t).tobytes() and pts2.tobytes() == X2.tobytes()
        assert not hist.any()
        assert not linearize(ctx, case)["behind"]  # the flag does not outlive the call
    assert adjust(ctx, case, max_iters=2)["status"] > 0


def test_descending_cameras_of_a_point_in_another_workgroup_are_a_layout_error(ctx):
    """pose_1025, points 300 and 1024 with their first two obs_cam entries swapped.  The Python surface refuses the arrays on the
    host; through the C-ABI the device's own check, made by the workgroup that owns the point, gives MOCAP_RIG_E_LAYOUT, and
    nothing is written.  Afterwards a clean call still succeeds."""
    case = rb.shape_case("pose_1025")
    prob, R, t, X = (case[k] for k in ("prob", "R", "t", "X"))
    off, cam, uv = prob.point_major()
    for n in (300, 1024):
        cam2 = cam.copy()
        o = off[n]
        cam2[o], cam2[o + 1] = cam[o + 1], cam[o]
        assert cam2[o] > cam2[o + 1]
        with pytest.raises(ValueError):
            ctx.rig_bundle_adjust(off, cam2, uv, poses12(R, t), X, max_iters=3)
        rc, result, poses2, pts2, hist = adjust_raw(ctx, case, off, cam2, uv, X)
        assert rc == 0 and result[0] == E_LAYOUT
        assert poses2.tobytes() == poses12(R, t).tobytes() and pts2.tobytes() == X.tobytes()
        assert not hist.any()
    assert adjust(ctx, case, max_iters=2)["status"] > 0  # the context is as good as before
