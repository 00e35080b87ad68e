"""mocap_correspond_visible on the GPU against its NumPy restatement (tests/correspond_visible_ref.py).

Every case: idx, views and n equal the restatement's; xyz and err agree with it within ten times the larger of (a) the
restatement's own deviation from an independent evaluation of the same member sets (extended-precision sums and
np.linalg.eigh, exact_hypotheses) and (b) 1e-12, both relative (deviation(): |X - X_ref| / |X_ref| and |err - err_ref| /
err_ref per marker).  Measured on the CPU over the cases of this file, (a) is 4.5e-14 to 7.3e-13 per case, and 7.8e-12 in one
of the 64 scenes of the T = 64 case (a marker with a small err), so the bound is 1e-11 in most cases and 7.8e-11 at the most --
worked out per case from that case's own hypotheses, never from what the kernel returns.  Measured on the MI355X: in every
case of this file (112 time-step comparisons) the device's xyz and err equal the restatement's bit for bit (deviation 0).  Every case also asserts that the restatement's smallest decision margin exceeds 1e-6 (px, px^2): no rounding
difference can flip a comparison; the seeds below were chosen on the CPU for that."""
import numpy as np
import pytest

import correspond_visible_ref as cv

pytestmark = pytest.mark.gpu

MIN_MARGIN = 1e-6
SEEDS_64 = list(range(64))


@pytest.fixture(scope="module")
def ctx():
    from mocapv2_amd.engine import MocapContext
    return MocapContext(1, 1)


def stack_cases(cases):
    """[(scene, pts [C, P, 2], counts, truth, markers)] of one rig -> pts [T, C, P, 2], counts [T, C] (P = the largest)"""
    P = max(c[1].shape[1] for c in cases)
    C = cases[0][1].shape[0]
    pts = np.zeros((len(cases), C, P, 2))
    for t, c in enumerate(cases):
        pts[t, :, :c[1].shape[1]] = c[1]
    return pts, np.stack([c[2] for c in cases]).astype(np.int32)


def run_gpu(ctx, pts, counts, cams, **kw):
    import torch
    ctx.set_cameras(*cams)
    dt = np.int32 if np.asarray(pts).dtype.kind in "iu" else np.float64
    out = ctx.correspond_visible(torch.from_numpy(np.ascontiguousarray(pts, dt)).cuda(),
                                 torch.from_numpy(np.ascontiguousarray(counts, np.int32)).cuda(), **kw)
    torch.cuda.synchronize()
    res = {k: v.cpu().numpy() for k, v in out.items()}
    res["views"] = res["views"].view(np.uint32)
    return res


def run_ref(pts, counts, cams, **kw):
    kw = dict(kw)
    kw["distorted"] = int(kw.get("distorted", 0))
    return [cv.correspond_visible(pts[t], counts[t], *cams, **kw) for t in range(len(pts))]


def assert_equals_restatement(gpu, refs, pts, cams, distorted=0, what=""):
    for t, r in enumerate(refs):
        assert r["margin"] > MIN_MARGIN, (what, t, r["margin"])
        assert gpu["n"][t] == r["n"], (what, t, gpu["n"][t], r["n"])
        n = r["n"]
        if n <= 0:
            continue
        assert np.array_equal(gpu["idx"][t, :n], r["idx"]), (what, t)
        assert np.array_equal(gpu["views"][t, :n], r["views"]), (what, t)
        dev = cv.deviation(r["xyz"], r["err"], *cv.exact_hypotheses(pts[t], r["idx"], *cams, distorted=distorted))
        got = cv.deviation(gpu["xyz"][t, :n], gpu["err"][t, :n], r["xyz"], r["err"])
        print(f"{what} step {t}: n {n} margin {r['margin']:.2e} restatement vs exact {dev:.2e} device vs restatement {got:.2e}")
        assert got <= 10 * max(dev, 1e-12), (what, t, got, dev)


def check(ctx, cases, what, **kw):
    cams = cv.scene_arrays(cases[0][0])
    pts, counts = stack_cases(cases)
    gpu = run_gpu(ctx, pts, counts, cams, **kw)
    refs = run_ref(pts, counts, cams, **kw)
    assert_equals_restatement(gpu, refs, pts, cams, distorted=int(kw.get("distorted", 0)), what=what)
    return gpu, refs, pts, counts, cams


# ---- 1. the one that fails today -------------------------------------------------------------------------------------
def test_camera0_blind_is_nothing_to_correspond_and_all_markers_to_the_new_call(ctx):
    import torch
    cases = [cv.scene_case(4, 6, 0.2, s, blind=(0,)) for s in range(4)]
    gpu, refs, pts, counts, cams = check(ctx, cases, "camera 0 blind")
    ctx.set_fundamentals(np.stack(cases[0][0].Fs))
    old = ctx.correspond(torch.from_numpy(pts).cuda(), torch.from_numpy(counts).cuda())
    assert (old["n"].cpu().numpy() == 0).all()
    found = 0
    for t, case in enumerate(cases):
        missed, ghosts, _ = cv.check_against_truth(refs[t], case[3], case[4])
        assert not missed and not ghosts
        assert gpu["n"][t] == sum((row >= 0).sum() >= 2 for row in case[3])
        found += int(gpu["n"][t])
    assert found > 0


def test_partial_visibility_six_cameras(ctx):
    cases = [cv.scene_case(6, 8, 0.3, s) for s in (0, 1, 2, 3, 4, 5)]
    gpu, refs, *_ = check(ctx, cases, "6 x 8, p = 0.3")
    for t, case in enumerate(cases):
        missed, ghosts, _ = cv.check_against_truth(refs[t], case[3], case[4])
        assert not missed and not ghosts


# ---- 2. full visibility ------------------------------------------------------------------------------------------------
def test_full_visibility_gives_the_groups_correspond_ranks_first(ctx):
    import torch
    # seeds 0 and 4: mocap_correspond's first group takes, per camera, the candidate nearest the epipolar line of camera 0's
    # point -- another marker's point in seeds 1, 2, 3 and 5 (looked up on the CPU with oracle.correspond); here it is the marker's own
    cases = [cv.scene_case(6, 8, 0.0, s) for s in (0, 4)]
    gpu, refs, pts, counts, cams = check(ctx, cases, "6 x 8, p = 0")
    ctx.set_fundamentals(np.stack(cases[0][0].Fs))
    old = {k: v.cpu().numpy() for k, v in ctx.correspond(torch.from_numpy(pts).cuda(), torch.from_numpy(counts).cuda()).items()}
    for t in range(len(cases)):
        assert gpu["n"][t] == 8 and old["n"][t] == 8
        assert (gpu["views"][t, :8] == 0x3f).all()
        groups = set()
        for o in range(8):  # the root's first group, as indices into the cameras' lists
            row = []
            for c in range(6):
                hit = np.flatnonzero((pts[t, c, :counts[t, c]] == old["grp"][t, o, c]).all(axis=1))
                assert len(hit) == 1
                row.append(int(hit[0]))
            groups.add(tuple(row))
        assert groups == {tuple(int(v) for v in row) for row in gpu["idx"][t, :8]}


# ---- 3. later passes ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [3, 7])
def test_later_passes_find_what_the_first_pass_loses(ctx, seed):
    case = cv.scene_case(6, 24, 0.4, seed)
    _, one, *_ = check(ctx, [case], f"6 x 24 seed {seed}, one pass", max_passes=1)
    _, three, *_ = check(ctx, [case], f"6 x 24 seed {seed}, three passes", max_passes=3)
    assert three[0]["n"] > one[0]["n"] and three[0]["passes"] > 1


# ---- 4. edges ----------------------------------------------------------------------------------------------------------
def test_two_cameras(ctx):
    check(ctx, [cv.scene_case(2, 4, 0.0, s) for s in (0, 1, 2)], "C = 2")


def test_empty_cameras_and_lonely_points(ctx):
    full = cv.scene_case(4, 5, 0.0, 1)
    scene, pts, counts, truth, markers = full
    empty = (scene, pts, np.zeros(4, np.int32), truth, markers)
    one_cam_empty = (scene, pts, np.where(np.arange(4) == 2, 0, counts).astype(np.int32), truth, markers)
    lonely = (scene, pts, np.array([0, 1, 0, 0], np.int32), truth, markers)
    gpu, refs, *_ = check(ctx, [full, empty, one_cam_empty, lonely], "empty cameras")
    assert list(gpu["n"]) == [5, 0, 5, 0]
    assert (gpu["idx"][2, :5, 2] == -1).all() and (gpu["views"][2, :5] == 0b1011).all()


def test_min_views_three(ctx):
    cases = [cv.scene_case(6, 8, 0.3, s, false_blobs=2) for s in (0, 1, 2)]
    gpu, refs, *_ = check(ctx, cases, "min_views = 3", min_views=3)
    for t, case in enumerate(cases):
        missed, ghosts, _ = cv.check_against_truth(refs[t], case[3], case[4], min_views=3)
        assert not ghosts and not missed
        assert all(bin(int(v)).count("1") >= 3 for v in gpu["views"][t, :gpu["n"][t]])


def test_thirty_two_cameras_fill_the_pair_table_and_the_mask(ctx):
    cases = [cv.scene_case(32, 4, 0.3, s) for s in (0, 1)]
    gpu, refs, *_ = check(ctx, cases, "C = 32, P = 4")
    seen31 = [int(v) >> 31 for t in range(2) for v in gpu["views"][t, :gpu["n"][t]]]
    assert any(seen31) and gpu["n"].min() > 0


def test_capacity_255_points_per_camera(ctx):
    case = cv.scene_case(3, 5, 0.0, 2, P=255)
    gpu, *_ = check(ctx, [case], "P = 255, C = 3")
    assert gpu["n"][0] == 5


def test_sixty_four_time_steps_are_independent(ctx):
    cases = [cv.scene_case(4, 4, 0.3, s) for s in SEEDS_64]  # 64 different scenes: no time step can stand in for another
    cams = cv.scene_arrays(cases[0][0])
    pts, counts = stack_cases(cases)
    refs = run_ref(pts, counts, cams)
    assert len({r["xyz"].tobytes() for r in refs}) == 64
    gpu = run_gpu(ctx, pts, counts, cams)
    assert_equals_restatement(gpu, refs, pts, cams, what="T = 64")
    perm = np.random.default_rng(0).permutation(64)
    shuffled = run_gpu(ctx, pts[perm], counts[perm], cams)
    for k, t in enumerate(perm):
        n = gpu["n"][t]
        assert shuffled["n"][k] == n
        for key in ("xyz", "err", "idx", "views"):
            assert np.array_equal(shuffled[key][k, :n], gpu[key][t, :n]), key


# ---- 5. input forms ----------------------------------------------------------------------------------------------------
def test_int32_records_through_camera_major_strides_equal_the_dense_array(ctx):
    import torch
    T, C, M = 3, 4, 5
    cases = [cv.scene_case(C, M, 0.2, s) for s in range(T)]
    cams = cv.scene_arrays(cases[0][0])
    pts, counts = stack_cases(cases)
    pts = np.floor(pts)  # centroid records hold integer pixels
    dense = run_gpu(ctx, pts, counts, cams)
    assert_equals_restatement(dense, run_ref(pts, counts, cams), pts, cams, what="integer pixels")
    P = pts.shape[2]
    rec_ints = 2 + 2 * P
    records = np.zeros((C, T, rec_ints), np.int32)  # camera-major, as after the all-gather
    records[:, :, 0] = counts.T
    records[:, :, 2:] = pts.transpose(1, 0, 2, 3).reshape(C, T, 2 * P)
    out = ctx.correspond_visible_records(torch.from_numpy(records).cuda(), T, C, t0=0, stride_t=1, stride_c=T, P=P)
    torch.cuda.synchronize()
    for t in range(T):
        n = dense["n"][t]
        assert out["n"][t].item() == n and n > 0
        for key in ("xyz", "err", "idx"):
            assert np.array_equal(out[key][t, :n].cpu().numpy(), dense[key][t, :n]), key
        assert np.array_equal(out["views"][t, :n].cpu().numpy().view(np.uint32), dense["views"][t, :n])


def test_distorted_pixels_equal_undistorted_points_of_them(ctx):
    from mocapv2_amd import calibrate
    from mocapv2_amd.synth import MILD_DIST
    cases = [cv.scene_case(4, 6, 0.2, s, dist=MILD_DIST, distorted=True) for s in (0, 1)]
    gpu, refs, pts, counts, cams = check(ctx, cases, "distorted = 1", distorted=True)
    und = np.stack([[calibrate.undistort_points(pts[t, c], cams[0][c], cams[1][c]) for c in range(4)] for t in range(2)])
    plain = run_gpu(ctx, und, counts, cams, distorted=False)
    assert_equals_restatement(plain, refs, pts, cams, distorted=1, what="undistorted on the host")
    for t in range(2):
        n = gpu["n"][t]
        assert n > 0 and plain["n"][t] == n
        assert np.array_equal(plain["idx"][t, :n], gpu["idx"][t, :n]) and np.array_equal(plain["views"][t, :n], gpu["views"][t, :n])


# ---- 6. capacities, each at its edge ---------------------------------------------------------------------------------------
def test_count_limits_fail_their_step_only(ctx):
    cases = [cv.scene_case(4, 5, 0.0, s) for s in (0, 1, 2, 3)]  # P = 5 = every count: count = P passes
    cams = cv.scene_arrays(cases[0][0])
    pts, counts = stack_cases(cases)
    good = run_gpu(ctx, pts, counts, cams)
    assert_equals_restatement(good, run_ref(pts, counts, cams), pts, cams, what="count = P")
    assert (good["n"] == 5).all()
    bad = counts.copy()
    bad[1, 2] = 6    # P + 1
    bad[2, 0] = -3   # a blob-stage error code
    gpu = run_gpu(ctx, pts, bad, cams)
    assert_equals_restatement(gpu, run_ref(pts, bad, cams), pts, cams, what="count = P + 1, count < 0")
    assert list(gpu["n"]) == [5, cv.E_TRUNCATED, cv.E_BLOB, 5]
    for t in (0, 3):
        for key in ("xyz", "err", "idx", "views"):
            assert np.array_equal(gpu[key][t, :5], good[key][t, :5]), key


def test_seed_capacity_at_its_edge(ctx):
    cases = [cv.scene_case(6, 24, 0.4, s) for s in (3, 5)]
    cams = cv.scene_arrays(cases[0][0])
    pts, counts = stack_cases(cases)
    refs = run_ref(pts, counts, cams)
    most = [max(r["seeds"]) for r in refs]
    assert most[0] != most[1]
    lo, hi = min(most), max(most)
    at = run_gpu(ctx, pts, counts, cams, max_hyp=hi)       # the crowded step just fits
    assert_equals_restatement(at, refs, pts, cams, what="max_hyp = seeds")
    under = run_gpu(ctx, pts, counts, cams, max_hyp=hi - 1)  # one seed too many: that step fails, the other is untouched
    assert_equals_restatement(under, run_ref(pts, counts, cams, max_hyp=hi - 1), pts, cams, what="max_hyp = seeds - 1")
    crowded = most.index(hi)
    assert under["n"][crowded] == cv.E_GROUPS and under["n"][1 - crowded] == at["n"][1 - crowded] > 0
    assert lo <= hi - 1


def test_hypotheses_beyond_the_lds_cap_work_in_scratch(ctx):
    """C = 32 leaves LDS room for 2048 hypothesis records; a time step with more seeds in a pass works in the context's scratch."""
    case = cv.scene_case(32, 8, 0.1, 0)
    gpu, refs, *_ = check(ctx, [case], "C = 32, seeds beyond the LDS cap")
    assert max(refs[0]["seeds"]) > 2048 and gpu["n"][0] > 0


def test_output_rows_at_their_edge(ctx):
    cases = [cv.scene_case(4, 5, 0.0, s) for s in (0, 1)] + [cv.scene_case(4, 3, 0.0, 2, P=5)]
    cams = cv.scene_arrays(cases[0][0])
    pts, counts = stack_cases(cases)
    fits = run_gpu(ctx, pts, counts, cams, Q=5)
    assert_equals_restatement(fits, run_ref(pts, counts, cams, Q=5), pts, cams, what="Q = n")
    assert list(fits["n"]) == [5, 5, 3]
    short = run_gpu(ctx, pts, counts, cams, Q=4)
    assert_equals_restatement(short, run_ref(pts, counts, cams, Q=4), pts, cams, what="Q = n - 1")
    assert list(short["n"]) == [cv.E_OUTPUT, cv.E_OUTPUT, 3]
    for key in ("xyz", "err", "idx", "views"):
        assert np.array_equal(short[key][2, :3], fits[key][2, :3]), key


# ---- 7. determinism ------------------------------------------------------------------------------------------------------
def test_two_calls_give_the_same_bits(ctx):
    cases = [cv.scene_case(6, 24, 0.4, s) for s in (0, 1, 2, 3)]
    cams = cv.scene_arrays(cases[0][0])
    pts, counts = stack_cases(cases)
    a, b = run_gpu(ctx, pts, counts, cams), run_gpu(ctx, pts, counts, cams)
    assert np.array_equal(a["n"], b["n"]) and a["n"].min() > 0
    for t in range(4):
        for key in ("xyz", "err", "idx", "views"):
            assert a[key][t, :a["n"][t]].tobytes() == b[key][t, :a["n"][t]].tobytes(), key


# ---- arguments and state ------------------------------------------------------------------------------------------------
def test_argument_and_state_errors(ctx):
    import torch
    from mocapv2_amd import _abi
    from mocapv2_amd.engine import MocapContext
    case = cv.scene_case(4, 5, 0.0, 0)
    cams = cv.scene_arrays(case[0])
    pts, counts = stack_cases([case])
    d_pts, d_cnt = torch.from_numpy(pts).cuda(), torch.from_numpy(counts).cuda()
    ctx.set_cameras(*cams)
    for kw in ({"min_views": 1}, {"min_views": 5}, {"cutoff": 0.0}, {"cutoff": float("nan")}, {"gate": float("inf")}, {"gate": -1.0},
               {"max_err": 0.0}, {"max_passes": 0}, {"max_hyp": 0}, {"max_hyp": 65536}, {"Q": 0}):
        with pytest.raises(_abi.MocapError) as e:
            ctx.correspond_visible(d_pts, d_cnt, **kw)
        assert e.value.code == -1, kw
    one = torch.zeros((1, 1, 5, 2), dtype=torch.float64, device="cuda")  # C = 1
    with pytest.raises(_abi.MocapError) as e:
        ctx.correspond_visible(one, torch.zeros((1, 1), dtype=torch.int32, device="cuda"))
    assert e.value.code == -1
    big = torch.zeros((1, 2, 256, 2), dtype=torch.float64, device="cuda")  # P = 256
    with pytest.raises(_abi.MocapError) as e:
        ctx.correspond_visible(big, torch.zeros((1, 2), dtype=torch.int32, device="cuda"))
    assert e.value.code == -1
    lib, st = ctx.lib, torch.cuda.current_stream().cuda_stream
    out = ctx._vis_out(1, 10, 4)
    p = lambda t: t.data_ptr()
    rc = lib.mocap_correspond_visible(ctx._h, p(d_pts), 41, 10, p(d_cnt), 4, 1, 1, 1, 4, 5, 0, 10.0, 10.0, 2, 25.0, 3, 8192, 10,
                                      p(out["xyz"]), p(out["err"]), p(out["idx"]), p(out["views"]), p(out["n"]), st)  # odd stride
    assert rc == -1 and b"stride" in lib.mocap_last_error()
    wide = torch.zeros((1, 32, 255, 2), dtype=torch.float64, device="cuda")  # 32 x 255 points do not fit LDS beside the tables
    ctx.set_cameras(*cv.scene_arrays(cv.scene_case(32, 1, 0.0, 0)[0]))
    with pytest.raises(_abi.MocapError) as e:
        ctx.correspond_visible(wide, torch.zeros((1, 32), dtype=torch.int32, device="cuda"))
    assert e.value.code == -3 and "bytes of LDS" in str(e.value)
    fresh = MocapContext(1, 1)  # no cameras set
    with pytest.raises(_abi.MocapError) as e:
        fresh.correspond_visible(d_pts, d_cnt)
    assert e.value.code == -4
    fresh.close()


# ---- 8. trackers -------------------------------------------------------------------------------------------------------------
W, H = 320, 192
MARKERS = np.array([[-0.42, -0.30, 0.05], [0.40, 0.32, 0.12]])


def tracker_frames(T=2):
    """[T, 3, H, W]: two discs per camera, except that camera 0 does not see marker 0"""
    from mocapv2_amd.synth import ZERO_DIST, Scene
    sc = Scene(3, W, H, dist=ZERO_DIST)
    frames = np.empty((T, 3, H, W), np.uint8)
    for t in range(T):
        mk = MARKERS + 0.02 * t
        for c in range(3):
            frames[t, c] = sc.render(np.random.default_rng(100 * t + c), mk[1:] if c == 0 else mk, c, radius_range=(16.0, 17.0), noise_max=40)
    return sc, frames


def test_batch_tracker_any_equals_the_call_on_its_records():
    import torch
    from mocapv2_amd.pipeline import BatchTracker, scene_arrays
    sc, frames = tracker_frames()
    K, dist, R, t, F = scene_arrays(sc)
    T = len(frames)
    tr = BatchTracker(K, dist, R, t, None, W, H, T, visibility="any")
    out = tr.step(torch.from_numpy(frames.reshape(T * 3, H, W)).cuda())
    n = tr.finish(out)
    assert list(n) == [2] * T
    _, cnt = tr.ctx.record_views(tr.records)
    assert cnt.cpu().numpy().reshape(T, 3).tolist() == [[1, 2, 2]] * T
    direct = tr.ctx.correspond_visible_records(tr.records, T, 3, P=tr.max_points)
    torch.cuda.synchronize()
    for s in range(T):
        for key in ("xyz", "err", "idx", "views"):
            assert torch.equal(out[key][s, :2], direct[key][s, :2]), key
        views = sorted(int(v) for v in out["views"][s, :2].cpu().numpy())
        assert views == [0b110, 0b111]  # the marker camera 0 misses, and the one all three see
        hidden = int(np.flatnonzero(out["views"][s, :2].cpu().numpy() == 0b110)[0])
        assert np.linalg.norm(out["xyz"][s, hidden].cpu().numpy() - (MARKERS[0] + 0.02 * s)) < 0.03


def test_replay_tracker_any_yields_the_marker_all_misses():
    from mocapv2_amd.pipeline import scene_arrays
    from mocapv2_amd.replay import ReplayTracker
    sc, frames = tracker_frames()
    K, dist, R, t, F = scene_arrays(sc)
    T = len(frames)
    kw = dict(batch=T, max_points=8)
    every = list(ReplayTracker(K, dist, R, t, F, W, H, **kw).run(frames))
    some = list(ReplayTracker(K, dist, R, t, None, W, H, visibility="any", **kw).run(frames))
    for s in range(T):
        assert len(every[s]["object_points"]) == 1 and len(some[s]["object_points"]) == 2
        truth = MARKERS + 0.02 * s
        near = lambda pts, X: min(np.linalg.norm(np.asarray(p) - X) for p in pts)
        assert near(every[s]["object_points"], truth[0]) > 0.3 and near(some[s]["object_points"], truth[0]) < 0.03
        assert near(some[s]["object_points"], truth[1]) < 0.03
        img = some[s]["image_points"]
        assert img.shape == (2, 3, 2) and np.isnan(img).sum() == 2  # one camera of one marker has no point
        q = int(np.flatnonzero(np.isnan(img[:, 0, 0]))[0])
        assert np.linalg.norm(some[s]["object_points"][q] - truth[0]) < 0.03
        assert some[s]["message"] == __import__("mocapv2_amd.replay", fromlist=["x"]).tracker_message([0, 0, 0, 0] + list(some[s]["object_points"][0]))


def test_visibility_all_is_the_tracker_without_the_argument():
    import torch
    from mocapv2_amd.pipeline import BatchTracker, scene_arrays
    sc, frames = tracker_frames()
    arrays = scene_arrays(sc)
    T = len(frames)
    d_frames = torch.from_numpy(frames.reshape(T * 3, H, W)).cuda()
    a = BatchTracker(*arrays, W, H, T)
    b = BatchTracker(*arrays, W, H, T, visibility="all")
    oa, ob = a.step(d_frames), b.step(d_frames)
    na, nb = a.finish(oa), b.finish(ob)
    assert np.array_equal(na, nb) and na.min() > 0
    assert torch.equal(a.records, b.records)
    for s in range(T):
        for key in ("xyz", "err", "grp", "root", "order"):
            assert torch.equal(oa[key][s, :na[s]], ob[key][s, :na[s]]), key
    with pytest.raises(ValueError):
        BatchTracker(*arrays, W, H, T, visibility="some")


def test_finish_raises_capacity_error_with_the_new_codes_text():
    import torch
    from mocapv2_amd.pipeline import BatchTracker, CapacityError, scene_arrays
    sc, frames = tracker_frames()
    K, dist, R, t, F = scene_arrays(sc)
    T = len(frames)
    tr = BatchTracker(K, dist, R, t, None, W, H, T, visibility="any")
    d_frames = torch.from_numpy(frames.reshape(T * 3, H, W)).cuda()
    tr.extract(d_frames)
    tr.out = tr.ctx.correspond_visible_records(tr.records, T, 3, P=tr.max_points, Q=1)  # two markers, one output row
    with pytest.raises(CapacityError) as e:
        tr.finish()
    assert e.value.code == cv.E_OUTPUT and "MOCAP_CORR_E_OUTPUT" in str(e.value)
    # the tracker hands max_hyp (and cutoff) through: one seed slot is too few for two markers
    tight = BatchTracker(K, dist, R, t, None, W, H, T, visibility="any", max_hyp=1)
    tight.step(d_frames)
    with pytest.raises(CapacityError) as e:
        tight.finish()
    assert e.value.code == cv.E_GROUPS and "max_hyp" in str(e.value)
