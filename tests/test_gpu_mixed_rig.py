"""The geometry and solver kernels on rigs whose cameras all differ in K and lens (mocapv2_amd.synth.MixedScene,
tests/mixed_rig.py).  Everywhere else in the suite the cameras of a rig share one K and one lens, so a read of the wrong
camera's row -- csrc/correspond_dev.h's 38-double LDS row per camera, csrc/geom_batch.hip's `ki = compact_k ? m : c`, csrc/rig_ba.hip's Lens per
observation, calibrate.py's K[a] / K[b] over tree edges, BatchTracker's slot_of[c] -- changes nothing there.  Here it does, and
the correspondence test measures by how much (CPU oracle) before it compares.  Yardsticks: the reference's own outputs
(tests/golden/*_mixed*.npz, oracle/gen_golden.py mixed), the CPU oracle, NumPy restatements.  Tolerances are the ones the
suite already uses for the same quantities."""
import os

import numpy as np
import pytest

import mixed_rig as mr
import oracle
import rig_ba_ref as rb

pytestmark = pytest.mark.gpu

TOL_XYZ = 1e-7  # world units = 1e-4 mm (BASELINE.json)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def ctx():
    from mocapv2_amd.engine import MocapContext
    return MocapContext(1, 1)


# ---- correspondence ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("floats", [False, True], ids=["int32", "float64"])
@pytest.mark.parametrize("C,M,T", [(4, 6, 4), (6, 8, 4)])
def test_correspond_on_unequal_cameras_matches_oracle(ctx, C, M, T, floats):
    """MocapContext.correspond against oracle.correspond per time step: root, grp, order equal, xyz within 1e-7, err within
    rtol 1e-9 / atol 1e-12 (test_gpu_geom.py's bars).  Before that, per time step, what a wrong-camera read would do (CPU
    oracle): camera 0's lens for every camera must move every root's err by more than 1e-6 of itself, camera 0's K for every
    camera every root's xyz by more than 1e-3 world units.  Measured on the CPU over these steps: err moves by 1.4e-5 .. 2.5e-3
    at the least-moved root, xyz by 0.013 .. 0.19; the bars sit 4 and 5 orders of magnitude below.
    Measured on the MI355X, GPU - oracle: xyz and err equal to the last bit (0.0) in all four cases."""
    import torch
    sc = mr.MixedScene(C)
    K, dist, R, t, F = mr.arrays(sc)
    pts, cnt = mr.correspondence_steps(sc, M, T, 940 + C, floats)
    ctx.set_cameras(K, dist, R, t)
    ctx.set_fundamentals(F)
    out = ctx.correspond(torch.from_numpy(pts).cuda(), torch.from_numpy(cnt).cuda())
    out = {k: v.cpu().numpy() for k, v in out.items()}
    roots, worst_xyz, worst_err = 0, 0.0, 0.0
    for s in range(T):
        ref, moved_err, moved_xyz = mr.wrong_camera_sensitivity(pts[s], cnt[s], K, dist, R, t, F)
        k = len(ref["root"])
        print(f"step {s}: {k} roots; wrong lens moves err by >= {moved_err:.3e} (relative), wrong K moves xyz by >= {moved_xyz:.3e}")
        assert k > 0 and moved_err > 1e-6 and moved_xyz > 1e-3  # the step can see the fault
        assert out["n"][s] == k
        worst_xyz = max(worst_xyz, float(np.abs(out["xyz"][s, :k] - ref["xyz"]).max()))
        worst_err = max(worst_err, float((np.abs(out["err"][s, :k] - ref["err"]) / ref["err"]).max()))
        print(f"        GPU - oracle: xyz {worst_xyz:.3e} (allowed {TOL_XYZ})  err relative {worst_err:.3e} (allowed 1e-9)")
        assert np.array_equal(out["root"][s, :k], ref["root"])
        assert np.array_equal(out["grp"][s, :k], ref["groups"])
        assert np.array_equal(out["order"][s, :k], ref["order"])
        assert np.abs(out["xyz"][s, :k] - ref["xyz"]).max() < TOL_XYZ
        assert np.allclose(out["err"][s, :k], ref["err"], rtol=1e-9, atol=1e-12)
        roots += k
    assert roots >= 3 * T


# ---- [None, None] entries: intrinsics by position and by camera number -------------------------------------------------------
def project_f32(X, R, t, K, d):
    """cv.projectPoints as the reference calls it (lib/Helpers.py:133-139): the point rounded to float32, the model in float64,
    the pixel rounded to float32"""
    x, y, z = R @ np.asarray(X, np.float32).astype(np.float64) + t
    x, y = x / z, y / z
    r2 = x * x + y * y
    cd = 1 + d[0] * r2 + d[1] * r2 * r2 + d[4] * r2 * r2 * r2
    xd = x * cd + d[2] * 2 * x * y + d[3] * (r2 + 2 * x * x)
    yd = y * cd + d[2] * (r2 + 2 * y * y) + d[3] * 2 * x * y
    return np.array([xd * K[0, 0] + K[0, 2], yd * K[1, 1] + K[1, 2]], np.float32).astype(np.float64)


def by_camera_number(grp, valid, X, K, dist, R, t):
    """(DLT point, reprojection MSE of X) of one group with every camera's OWN K and lens: lib/Helpers.py:58-78 and :129-143
    with camera_params[c] for camera c"""
    import scipy.linalg
    cams = np.flatnonzero(valid)
    A = []
    for c in cams:
        P = K[c] @ np.c_[R[c], t[c]]
        A += [grp[c, 1] * P[2] - P[1], P[0] - grp[c, 0] * P[2]]
    A = np.array(A)
    Vh = scipy.linalg.svd(A.T @ A, full_matrices=False)[2]
    e = np.concatenate([(grp[c] - project_f32(X, R[c], t[c], K[c], dist[c])) ** 2 for c in cams])
    return Vh[3, :3] / Vh[3, 3], e.mean()


def test_none_entries_on_unequal_cameras(ctx):
    """reproj_none_mixed.npz: the reference's triangulate_point and calculate_reprojection_error on seven groups with [None,
    None] entries, four cameras that differ in K and lens.  compact_k=True is the reference's indexing (camera_params by
    position after the entries are dropped) and must give the fixture; compact_k=False (every camera its own row: what
    calibrate_rig's triangulations rely on) must give the NumPy restatement above.  Bars: xyz 1e-7, MSE rtol 1e-9 / atol 1e-9
    (test_k1_triangulate_points).  The two indexings differ by 0.08 .. 0.44 world units and by factors of 200 .. 13000 in the MSE on the three
    groups whose first entry is dropped (asserted), so neither can pass for the other.
    Measured on the MI355X, GPU - yardstick: by position xyz 5.6e-16, MSE equal; by number xyz 6.1e-16, MSE equal."""
    g = np.load(os.path.join(GOLDEN, "reproj_none_mixed.npz"))
    valid = ~np.isnan(g["groups"][:, :, 0])
    pts = np.nan_to_num(g["groups"])
    K, dist, R, t = g["K"], g["dist"], g["R"], g["t"]
    ctx.set_cameras(K, dist, R, t)
    some = valid.sum(1) >= 2
    assert some.tolist() == [True] * 5 + [False] * 2
    told_apart = 0
    for compact in (True, False):
        xyz, ok = ctx.triangulate_batch(pts, valid, compact_k=compact)
        mse, ok2 = ctx.reproject_batch(pts, valid, g["obj"], compact_k=compact)
        assert np.array_equal(ok.astype(bool), some) and np.array_equal(ok2.astype(bool), some)
        for n in np.flatnonzero(some):
            if compact:
                want_xyz, want_mse = g["out"][n], g["mse"][n]
            else:
                want_xyz, want_mse = by_camera_number(pts[n], valid[n], g["obj"][n], K, dist, R, t)
            print(f"compact_k={compact} group {n}: xyz GPU - yardstick {np.abs(xyz[n] - want_xyz).max():.3e} (allowed {TOL_XYZ})  "
                  f"MSE relative {abs(mse[n] - want_mse) / want_mse:.3e} (allowed 1e-9)")
            assert np.abs(xyz[n] - want_xyz).max() < TOL_XYZ
            assert np.allclose(mse[n], want_mse, rtol=1e-9, atol=1e-9)
            if not compact and not valid[n, :valid[n].sum()].all():  # a dropped entry before a kept one
                assert np.abs(want_xyz - g["out"][n]).max() > 1e-2 and abs(want_mse - g["mse"][n]) > 1e-2 * want_mse
                told_apart += 1
    assert told_apart == 3


# ---- bundle-adjustment residual vector ----------------------------------------------------------------------------------------
def test_ba_residuals_on_the_reference_fixture_of_two_unequal_cameras(ctx):
    """ba_residuals_mixed.npz: the reference's residual_function on 600 groups of two cameras with different K and lens, 30
    groups with a [None, None] spread over all three 256-group rounds of the kernel's block-wide compaction (the carry from
    one round to the next runs for the first time: every other case has N <= 64), three parameter vectors, the last with a
    zero rotation vector.  One vector at a time and as a batch, rtol 2e-5 / atol 1e-6 (one float32 ulp of the MSE, as
    test_gpu_geom.py).  On the CPU, camera 0's lens for both cameras moves the median residual by 5 % of itself.
    Measured on the MI355X: 545 residuals per vector, every one equal to the reference's float32 value (difference 0.0)."""
    g = np.load(os.path.join(GOLDEN, "ba_residuals_mixed.npz"))
    ip, valid = np.nan_to_num(g["image_points"]), g["valid"]
    ctx.set_cameras(g["K"], g["dist"], np.stack([np.eye(3)] * 2), np.zeros((2, 3)))
    prob = ctx.ba_problem(ip, valid)
    single = [prob.residuals(x) for x in g["params"]]
    batch = prob.residuals(np.stack(g["params"]))
    for e, b, r in zip(single, batch, g["residuals"]):
        assert e.dtype == np.float32 and e.shape == r.shape == b.shape
        print(f"{len(r)} residuals, GPU - reference relative {(np.abs(e - r) / r).max():.3e} (allowed 2e-5)")
        assert np.allclose(e, r, rtol=2e-5, atol=1e-6) and np.array_equal(e, b)


@pytest.mark.parametrize("N", [255, 256, 257, 600])
def test_ba_residuals_of_five_unequal_cameras_across_the_compaction_rounds(ctx, N):
    """C = 5 cameras of different K and lens, N groups on either side of the 256-group round and three rounds deep, without
    holes and with them (5 % of the groups lose a camera, one group is seen by nobody, one by camera 0 only: groups with a
    hole are not triangulated, lib/Helpers.py:93, the rest is paired positionally, :104, and reprojected with the intrinsics
    by position, :137-138) against oracle.ba_residuals: equal lengths, rtol 2e-5 / atol 1e-6.  On the CPU, camera 0's lens
    for all cameras moves more than 9 of 10 residuals beyond that tolerance (asserted: more than half).
    Measured on the MI355X: 255 / 239, 256 / 240, 257 / 241, 600 / 567 residuals without / with holes, all equal to the
    oracle's (difference 0.0)."""
    for holes in (False, True):
        pts, valid, sets, K, dist = mr.ba_case(5, N, 60 + N, holes)
        ctx.set_cameras(K, dist, np.stack([np.eye(3)] * 5), np.zeros((5, 3)))
        got = ctx.ba_problem(pts, valid).residuals(sets)
        for x, e in zip(sets, got):
            exp = oracle.ba_residuals(x, 5, pts, valid, K, dist)
            wrong = oracle.ba_residuals(x, 5, pts, valid, K, np.stack([dist[0]] * 5))
            assert (~np.isclose(wrong, exp, rtol=2e-5, atol=1e-6)).mean() > 0.5  # the case can see a wrong lens
            assert e.shape == exp.shape and (len(exp) == N if not holes else N - 2 * (N // 20 + 2) <= len(exp) < N)
            print(f"N {N} holes {holes}: {len(exp)} residuals, GPU - oracle relative {(np.abs(e - exp) / exp).max():.3e} (allowed 2e-5)")
            assert np.allclose(e, exp, rtol=2e-5, atol=1e-6)


# ---- rig bundle adjustment ----------------------------------------------------------------------------------------------------
def test_rig_pieces_agree_with_the_restatement_on_mixed6(ctx):
    """test_gpu_rig_ba.py::test_pieces_agree_with_the_restatement, its rule unchanged (8 x the restatement's own spread under
    10 permutations of the observation order), on six cameras of different K and lens with no point shared by cameras 0 and 1.
    Restatement's spread (CPU):  cost 1.3e-16  gradient 5.8e-16  S 2.1e-15  rhs 7.6e-16   (tests/test_rig_ba_host.py)
    GPU - restatement (MI355X):  cost 1.3e-16  gradient 1.8e-16  S 1.8e-15  rhs 2.3e-16"""
    import test_gpu_rig_ba as rig
    rig.test_pieces_agree_with_the_restatement(ctx, "mixed6")


def test_rig_loop_walks_the_restatements_iterations_on_mixed6(ctx):
    """test_gpu_rig_ba.py::test_loop_walks_the_restatements_iterations, its rules unchanged (same accept / reject sequence,
    iterations and stop; |rho| >= 1e-3 asserted; per-iteration cost within 1e-8; cond(S) < 1e6), on mixed6.  The restatement
    alone: 6 accepted iterations, every rho within 4e-4 of 1, cond(S) 2.0e4 (tests/test_rig_ba_host.py).
    Measured on the MI355X: 6 / 6 iterations, cond(S) 2.0e4, largest relative cost difference 3.7e-14."""
    import test_gpu_rig_ba as rig
    rig.test_loop_walks_the_restatements_iterations(ctx, "mixed6")


def test_calibrate_rig_on_mixed6_clean(ctx):
    """calibrate_rig without poses on exact pixels of six unequal cameras, under test_calibrate_rig_on_clean6's bar: rms,
    rotation error and centre error at most 10 x those of the restatement run from the same initial poses and start points.
    Cameras 0 and 1 share no point, so the spanning tree reaches camera 1 over an edge (a, b) with a > b (asserted): the
    transposed fundamental matrix, K[b].T @ F_ab @ K[a] and the [K[a]] + [K[b]] * 4 camera table of that edge all have a and b
    in the other order than on every edge of an equal-camera rig, where swapping them changes nothing.
    The restatement alone from the perturbed truth: rms 9.6e-14 px, rotation 5.5e-16, centre 2.4e-15 (tests/test_rig_ba_host.py).
    Measured on the MI355X: tree 0-3, 3-2, 3-4, 3-5, 4-1 (two edges with a > b); GPU / restatement from the same start: rms
    1.02e-13 / 9.8e-14 px, rotation error 9.6e-16 / 8.2e-16, centre error 6.6e-15 / 4.7e-15, iterations 34 / 40."""
    import test_gpu_rig_ba as rig
    from mocapv2_amd import calibrate as cal
    c = rb.case("mixed6_clean")
    out = cal.calibrate_rig(c["image_points"], c["valid"], c["scene"].camera_params, threshold=3.0, ctx=ctx)
    tree = out["init"]["tree"]
    used = out["used"]
    X0 = rig.start_points(ctx, cal, c, out["poses_initial"])[used]
    prob, R, t, ref = rig.restatement_from(c, out["poses_initial"], used, X0)
    ref_poses = [{"R": ref["R"][k], "t": ref["t"][k]} for k in range(len(R))]
    e_gpu, e_ref = rig.aligned_errors(c["scene"], c["X"], out["poses"]), rig.aligned_errors(c["scene"], c["X"], ref_poses)
    print(f"tree {tree} scales {np.round(out['init']['scales'], 4)} votes {out['init']['votes']}")
    print(f"rms GPU {out['rms_px']:.3e} restatement {rig.rms(prob, ref['cost']):.3e}; rotation GPU {e_gpu[0]:.3e} restatement {e_ref[0]:.3e}; "
          f"centre GPU {e_gpu[1]:.3e} restatement {e_ref[1]:.3e}; iterations {out['iterations']} / {ref['iterations']}")
    assert any(a > b for a, b in tree) and (0, 1) not in tree
    assert used.sum() == len(used)
    assert out["rms_px"] <= 10 * rig.rms(prob, ref["cost"])
    assert e_gpu[0] <= 10 * e_ref[0] and e_gpu[1] <= 10 * e_ref[1]


# ---- frames to 3-D ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tracked():
    """Three unequal cameras (a barrel with tangential terms and k3, the identity, a pincushion), 640 x 360, 4 time steps of 4
    markers; per time step the oracle's centroids (oracle.find_dot with the camera's OWN K and lens) and correspondence"""
    from test_gpu_oracle_e2e import oracle_step
    C, T, W, H = 3, 4, 640, 360
    sc = mr.MixedScene(C, W, H, dists=[mr.MIXED_DISTS[3], mr.MIXED_DISTS[1], mr.MIXED_DISTS[2]])
    arrays = mr.arrays(sc)
    markers = [sc.markers(np.random.default_rng(50 + s), 4, extent=0.6) for s in range(T)]
    frames = np.stack([np.stack([sc.render(np.random.default_rng(1000 * s + c), markers[s], c, radius_range=(16, 20)) for c in range(C)])
                       for s in range(T)])
    steps = [oracle_step(frames[s], *arrays) for s in range(T)]
    assert sum(len(ref["root"]) for _, ref in steps) >= T  # the scene gives 3-D points
    # ... and the centroids depend on whose lens undistorts the frame: the next camera's moves them in every frame
    assert all(oracle.find_dot(frames[s, c], arrays[0][c], arrays[1][(c + 1) % C]) != steps[s][0][c] for s in range(T) for c in range(C))
    return sc, arrays, frames, steps


def test_batch_tracker_on_unequal_cameras_matches_oracle(tracked):
    """BatchTracker, one rank, depth 1: every centroid record and, per time step, grp and order equal to the oracle's, xyz
    within 1e-7.  Measured on the MI355X: 3, 3, 4, 4 roots in the 4 steps, xyz GPU - oracle 0.0."""
    import torch
    from mocapv2_amd.pipeline import BatchTracker
    from test_gpu_oracle_e2e import assert_records_equal, assert_step_equal
    sc, arrays, frames, steps = tracked
    T, C, H, W = frames.shape
    trk = BatchTracker(*arrays, W, H, T, depth=1)
    out = trk.step(torch.from_numpy(frames.reshape(T * C, H, W)).cuda())
    torch.cuda.synchronize()
    rec = trk.records.cpu().numpy()
    out = {k: v.cpu().numpy() for k, v in out.items()}
    points = 0
    for s, (lists, ref) in enumerate(steps):
        for c in range(C):
            assert_records_equal(rec, s * C + c, lists[c], (s, c))
        k = assert_step_equal(out, s, ref, s)
        if k:
            print(f"step {s}: {k} roots, xyz GPU - oracle {np.abs(out['xyz'][s, :k] - ref['xyz']).max():.3e} (allowed {TOL_XYZ})")
        points += k
    assert points >= T


def test_two_rank_layout_on_unequal_cameras_matches_oracle(tracked):
    """world = 2 the way test_sharded_pipeline_equals_single_rank emulates it (both ranks on this GPU, the all-gather replaced
    by the concatenation it produces).  Rank 1 holds cameras 1 and 2 in undistort slots 0 and 1: a tracker that pairs slot
    and camera wrongly undistorts with another camera's lens, which moves the centroids (asserted by the fixture).  Every
    record and every time step against the oracle, as above."""
    import torch
    from mocapv2_amd.pipeline import BatchTracker
    from test_gpu_oracle_e2e import assert_records_equal, assert_step_equal
    sc, arrays, frames, steps = tracked
    T_total, C, H, W = frames.shape
    world = 2
    T = T_total // world
    trackers = [BatchTracker(*arrays, W, H, T, world=world, rank=r) for r in range(world)]
    assert trackers[1].slot_of == {1: 0, 2: 1}
    recs = []
    for trk in trackers:
        images = trk.local_image_list()
        rec = trk.extract(torch.from_numpy(np.stack([frames[s, c] for c, s in images])).cuda()).clone()
        host = rec.cpu().numpy()
        for i, (c, s) in enumerate(images):
            assert_records_equal(host, i, steps[s][0][c], (trk.rank, c, s))
        recs.append(rec)
    gathered = torch.cat(recs, dim=0)
    points = 0
    for r, trk in enumerate(trackers):
        out = {k: v.cpu().numpy() for k, v in trk.triangulate(gathered).items()}
        for j in range(T):
            points += assert_step_equal(out, j, steps[r * T + j][1], (r, j))
    assert points >= T_total
