"""mocap_refine_points on the GPU against its NumPy restatement (tests/refine_points_ref.py): every output of every case equals
the restatement's bit for bit, floats compared as bytes (refine_points_ref.specified_equal: every key of a refined row, the
point, the mask and the status of an error row, and the canary the outputs were filled with wherever the call writes nothing).
Then the trackers: refine=None is the path as it was, refine={...} is MocapContext.refine_points on the batch's outputs."""
import numpy as np
import pytest

import correspond_visible_ref as cv
import mixed_rig
import refine_points_cases as cases
import refine_points_ref as rp

pytestmark = pytest.mark.gpu

CANARY = 0xA5


@pytest.fixture(scope="module")
def ctx():
    from mocapv2_amd.engine import MocapContext
    return MocapContext(1, 1)


def dev_out(T, Q, C, xyz_in=None):
    """The call's outputs on the device, every byte the canary; xyz_in: the input tensor in the place of xyz (in place)"""
    import torch
    host = rp.empty_out(T, Q, C, canary=CANARY)
    out = {k: torch.from_numpy(v.view(np.int32) if v.dtype == np.uint32 else v).cuda() for k, v in host.items()}
    if xyz_in is not None:
        out["xyz"] = xyz_in
    return out


def to_host(out):
    import torch
    torch.cuda.synchronize()
    res = {k: out[k].cpu().numpy() for k in rp.OUT_KEYS}
    for k in ("views", "dropped"):
        res[k] = res[k].view(np.uint32)
    return res


def run_both(ctx, cams, xyz, n, views, pts=None, idx=None, grp=None, in_place=False, what="", **kw):
    """One call on the device and in the restatement, both into canary-filled outputs; asserts the equality; returns both"""
    import torch
    ctx.set_cameras(*cams)
    T, Q = xyz.shape[:2]
    C = len(cams[0])
    d_xyz = torch.from_numpy(np.ascontiguousarray(xyz, np.float64)).cuda()
    d_n = torch.from_numpy(np.ascontiguousarray(n, np.int32)).cuda()
    d_views = None if views is None else torch.from_numpy(np.ascontiguousarray(views, np.uint32).view(np.int32)).cuda()
    args = {}
    if grp is not None:
        args["grp"] = torch.from_numpy(np.ascontiguousarray(grp, np.float64)).cuda()
    else:
        dt = np.int32 if np.asarray(pts).dtype.kind in "iu" else np.float64
        args["pts"] = torch.from_numpy(np.ascontiguousarray(pts, dt)).cuda()
        args["idx"] = torch.from_numpy(np.ascontiguousarray(idx, np.int32)).cuda()
    want = rp.empty_out(T, Q, C, canary=CANARY)
    if in_place:
        want["xyz"] = np.array(xyz, np.float64)
    got = to_host(ctx.refine_points(d_xyz, d_n, views=d_views, out=dev_out(T, Q, C, d_xyz if in_place else None), **args, **kw))
    ref_kw = {k: (0.0 if v is None else v) for k, v in kw.items()}
    ref_kw["distorted"] = int(bool(ref_kw.get("distorted", 0)))
    rp.refine_points(xyz, n, views, *cams, pts=pts, idx=idx, grp=grp, out=want, **ref_kw)
    bad = rp.specified_equal(got, want)
    print(f"{what}: T {T} Q {Q} C {C}, statuses {np.bincount(want['status'][want['status'] >= 0].ravel(), minlength=5).tolist()}, "
          f"iterations {int(want['iters'][want['status'] > 0].sum())}, differing (key, rows): {bad}")
    assert not bad, (what, bad)
    return got, want


def stacked(name, seeds, Q=None, floor=False):
    """The wrong-member scenes' seeds as the time steps of one call: cams, xyz [T][Q][3], n [T], views, pts [T][C][P][2], idx"""
    per = [cases.wrong_member_case(name, s) for s in seeds]
    C, P = per[0][1].shape[:2]
    Q = Q or max(p[3]["n"] for p in per)
    T = len(per)
    xyz, n = np.full((T, Q, 3), 7.5), np.zeros(T, np.int32)
    views, idx, pts = np.full((T, Q), 0xFFFFFFFF, np.uint32), np.full((T, Q, C), 1 << 20, np.int32), np.zeros((T, C, P, 2))
    for s, (cams, p, truth, res) in enumerate(per):
        k = res["n"]
        xyz[s, :k], n[s], views[s, :k], idx[s, :k], pts[s] = res["xyz"], k, res["views"], res["idx"], p
    if floor:
        pts = np.floor(pts).astype(np.int32)
    return per[0][0], xyz, n, views, pts, idx


def test_six_steps_of_partial_visibility_with_empty_and_failed_steps(ctx):
    """6 x 8, seeds 0..5 as T = 6 steps (float64 points, then the same floored to int32); step 2 has n = 0, step 4 n = -3: their
    rows and the rows beyond n[t] of every step (a point of 7.5s, a full mask and indices far outside the lists) are not read,
    and hold the canary afterwards"""
    for floor in (False, True):
        cams, xyz, n, views, pts, idx = stacked("6x8", range(6), Q=10, floor=floor)
        n[2], n[4] = 0, -3
        got, want = run_both(ctx, cams, xyz, n, views, pts=pts, idx=idx, what=f"6 x 8, int32 {floor}")
        assert (want["status"][[2, 4]] == 0).all() and (want["status"][0, :n[0]] > 0).all() and (want["status"][0, n[0]:] == 0).all()
        assert (got["xyz"][2].view(np.uint8) == CANARY).all() and (got["iters"][0, n[0]:].view(np.uint8) == CANARY).all()


def test_two_cameras(ctx):
    scene, pts, counts, truth, markers = cv.scene_case(2, 4, 0.0, 1)
    cams = cv.scene_arrays(scene)
    res = cv.correspond_visible(pts, counts, *cams)
    assert res["n"] == 4
    got, want = run_both(ctx, cams, res["xyz"][None], [4], res["views"][None], pts=pts[None], idx=res["idx"][None], what="C = 2")
    assert (want["views"][0] == 3).all() and (want["status"][0] > 0).all()


def test_thirty_two_cameras_with_a_member_in_camera_31(ctx):
    from mocapv2_amd import synth
    C, M = 32, 5
    scene = synth.Scene(C, 1920, 1080)
    cams = cv.scene_arrays(scene)
    rng = np.random.default_rng(5)
    mk = scene.markers(rng, M)
    pts = np.stack([scene.pixels(mk, c, distorted=False) + rng.normal(0, 0.5, (M, 2)) for c in range(C)])
    idx = np.tile(np.arange(M, dtype=np.int32)[:, None], (1, C))
    views = np.array([0xFFFFFFFF, 1 << 31 | 1, 1 << 31 | 1 << 30 | 1 << 7, 0x80000000, 0xFFFF0000], np.uint32)
    got, want = run_both(ctx, cams, (mk + 0.002)[None], [M], views[None], pts=pts[None], idx=idx[None], what="C = 32")
    assert want["status"][0].tolist() == [2, 2, 2, rp.E_VIEWS, 2] and (want["res2"][0, :3, 31] >= 0).all()
    # pruning reaches camera 31 too: its point moved by 8 px
    pts[31, 0] += 8.0
    got, want = run_both(ctx, cams, (mk + 0.002)[None], [M], views[None], pts=pts[None], idx=idx[None], max_res2=9.0, max_drop=1,
                         what="C = 32, camera 31 pruned")
    assert want["dropped"][0, 0] == 1 << 31 and want["views"][0, 0] == 0x7FFFFFFF and want["dropped"][0, 4] == 0


@pytest.mark.parametrize("Q", [65, 130])
def test_more_rows_than_a_wavefront_and_than_the_workgroup(ctx, Q):
    """The rows of several seeds stacked into one step: Q = 65 is past one wavefront, Q = 130 past one pass of the stride loop
    (128 lanes)"""
    per = [cases.wrong_member_case("6x8", s) for s in range(20)]
    P = per[0][1].shape[1]
    pts = np.concatenate([p[1] for p in per], axis=1)[None]  # [1][C][20 P][2]
    xyz = np.concatenate([p[3]["xyz"] for p in per])
    views = np.concatenate([p[3]["views"] for p in per])
    idx = np.concatenate([np.where(p[3]["idx"] >= 0, p[3]["idx"] + s * P, -1) for s, p in enumerate(per)]).astype(np.int32)
    assert len(xyz) >= Q
    got, want = run_both(ctx, per[0][0], xyz[None, :Q], [Q], views[None, :Q], pts=pts, idx=idx[None, :Q], what=f"Q = {Q}")
    assert (want["status"][0] > 0).all()


def test_one_step_no_step_and_bad_arguments(ctx):
    import torch
    from mocapv2_amd import _abi
    cams, xyz, n, views, pts, idx = stacked("4x4", [3])
    run_both(ctx, cams, xyz, n, views, pts=pts, idx=idx, what="T = 1")
    # T = 0 launches nothing; so does a bad argument, which is MOCAP_E_INVALID
    d = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).cuda()
    args = dict(views=d(views.view(np.int32), np.int32), pts=d(pts, np.float64), idx=d(idx, np.int32))
    out = dev_out(1, xyz.shape[1], 4)
    ctx.refine_points(d(xyz, np.float64)[:0], d(n, np.int32)[:0], views=args["views"][:0], pts=args["pts"][:0], idx=args["idx"][:0],
                      out={k: v[:0] for k, v in out.items()})
    for bad in (dict(max_iters=0), dict(lambda0=0.0), dict(ftol=-1.0), dict(min_views=1), dict(min_views=5), dict(max_drop=-1),
                dict(max_res2=float("nan"), max_drop=1)):
        with pytest.raises(_abi.MocapError) as e:
            ctx.refine_points(d(xyz, np.float64), d(n, np.int32), out=out, **args, **bad)
        assert e.value.code == -1, bad
    with pytest.raises(ValueError):
        ctx.refine_points(d(xyz, np.float64), d(n, np.int32), out=out, **args, max_drop=1)  # pruning without max_res2
    with pytest.raises(ValueError):
        ctx.refine_points(d(xyz, np.float64), d(n, np.int32), out=out)
    lib = _abi.load()
    p = lambda t: _abi.C.c_void_p(t.data_ptr())
    o = [p(out[k]) for k in ("xyz", "err", "res2", "cov", "views", "dropped", "iters", "status")]
    rc = lib.mocap_refine_points(ctx._h, p(d(xyz, np.float64)), p(d(n, np.int32)), None, 1, xyz.shape[1], 33, None, 0, 0, 1, 1, None,
                                 p(d(np.zeros((1, xyz.shape[1], 33, 2)), np.float64)), 0, 10, 1e-9, 1e-3, 0.0, 2, 0, *o, None)
    assert rc == -1  # C > 32
    assert all((v.view(np.uint8) == CANARY).all() for v in to_host(out).values())


def test_strided_points_equal_the_dense_layout(ctx):
    """The same points laid out camera-major with room between the lists, read through strides (the C entry point), against
    the dense call"""
    import torch
    from mocapv2_amd import _abi
    cams, xyz, n, views, pts, idx = stacked("6x8", [0, 1, 2])
    dense, _ = run_both(ctx, cams, xyz, n, views, pts=pts, idx=idx, what="dense")
    T, C, P = pts.shape[:3]
    Q = xyz.shape[1]
    pad = P + 3
    wide = np.full((C, T, pad, 2), 1e9)
    wide[:, :, :P] = pts.transpose(1, 0, 2, 3)
    d = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).cuda()
    out = dev_out(T, Q, C)
    p = lambda t: _abi.C.c_void_p(t.data_ptr())
    keep = [d(xyz, np.float64), d(n, np.int32), d(views.view(np.int32), np.int32), d(wide, np.float64), d(idx, np.int32)]
    _abi.check(_abi.load().mocap_refine_points(ctx._h, p(keep[0]), p(keep[1]), p(keep[2]), T, Q, C, p(keep[3]), pad * 2, T * pad * 2, 1, P,
                                               p(keep[4]), None, 0, 10, 1e-9, 1e-3, 0.0, 2, 0,
                                               *[p(out[k]) for k in ("xyz", "err", "res2", "cov", "views", "dropped", "iters", "status")], None))
    assert not rp.specified_equal(to_host(out), dense)


def test_grouped_form_equals_the_indexed_form(ctx):
    cams, xyz, n, views, pts, idx = stacked("6x8", [0, 1, 2])
    T, Q, C = idx.shape
    indexed, _ = run_both(ctx, cams, xyz, n, views, pts=pts, idx=idx, what="indexed")
    live = (np.arange(Q)[None, :] < n[:, None])[:, :, None] & ((views[:, :, None] >> np.arange(C, dtype=np.uint32)) & 1).astype(bool)
    grp = np.full((T, Q, C, 2), np.nan)  # what no member reads
    for s, q, c in zip(*np.nonzero(live)):
        grp[s, q, c] = pts[s, c, idx[s, q, c]]
    grouped, _ = run_both(ctx, cams, xyz, n, views, grp=grp, what="grouped")
    assert not rp.specified_equal(grouped, indexed)
    # and without a mask every camera is a member: the rows every camera sees equal theirs, the call equals the restatement
    full = views == 63
    full &= np.arange(Q)[None, :] < n[:, None]
    assert full.sum() >= 3
    g2 = np.where(np.isnan(grp), 0.0, grp)
    allcam, want = run_both(ctx, cams, xyz, n, None, grp=g2, what="grouped, no mask")
    for k in rp.OUT_KEYS:
        assert np.array_equal(allcam[k][full].view(np.uint8), indexed[k][full].view(np.uint8)), k


@pytest.mark.parametrize("distorted", [1, 0])
def test_unequal_cameras(ctx, distorted):
    """MixedScene(5): every camera its own K and lens; raw-frame pixels with distorted = 1, ideal ones with 0.  The host test
    measures what a wrong camera's lens would change (0.087 mm at the least)."""
    sc = mixed_rig.MixedScene(5)
    K, dist, R, t, _ = mixed_rig.arrays(sc)
    rng = np.random.default_rng(11)
    M = 9
    mk = sc.markers(rng, M)
    pts = np.stack([sc.pixels(mk, c, distorted=bool(distorted)) + rng.normal(0, 0.4, (M, 2)) for c in range(5)])
    idx = np.tile(np.arange(M, dtype=np.int32)[:, None], (1, 5))
    views = np.array([31, 31, 31, 0b10101, 0b01110, 0b11000, 31, 0b00011, 31], np.uint32)
    got, want = run_both(ctx, (K, dist, R, t), (mk + 0.003)[None], [M], views[None], pts=pts[None], idx=idx[None], distorted=distorted,
                         what=f"MixedScene(5), distorted {distorted}")
    assert (want["status"][0] > 0).all() and np.linalg.norm(want["xyz"][0] - mk, axis=1).max() < 0.02


def test_status_rows_do_not_disturb_their_neighbours(ctx):
    c = cases.status_case()
    got, want = run_both(ctx, c["cams"], c["xyz"], c["n"], c["views"], pts=c["pts"], idx=c["idx"], what="statuses")
    assert {q: int(s) for q, s in enumerate(got["status"][0])} == c["want"]
    # in place: xyz_out is the input buffer
    run_both(ctx, c["cams"], c["xyz"], c["n"], c["views"], pts=c["pts"], idx=c["idx"], in_place=True, what="statuses, in place")
    # the stops: one iteration; the largest damping (a rejected step, STOP_LAMBDA); Gauss-Newton's damping (rejected steps at the
    # rounding floor behind accepted ones)
    for kw, row, status in ((dict(max_iters=1), 0, 1), (dict(lambda0=1e16), 0, 3), (dict(lambda0=1e-12), 11, 1)):
        got, want = run_both(ctx, c["cams"], c["xyz"], c["n"], c["views"], pts=c["pts"], idx=c["idx"], what=f"statuses {kw}", **kw)
        assert got["status"][0, row] == status, (kw, got["status"][0])
    # a determinant that is not finite, twice: STOP_CHOLESKY, the point stays
    K = np.array(c["cams"][0]).copy()
    K[:, 0, 0] = K[:, 1, 1] = 1e110
    got, want = run_both(ctx, (K,) + tuple(c["cams"][1:]), c["xyz"], c["n"], c["views"], pts=c["pts"], idx=c["idx"], what="focal length 1e110")
    assert got["status"][0, 0] == 4 and got["iters"][0, 0] == 2 and np.array_equal(got["xyz"][0, 0], c["xyz"][0, 0])


def test_pruning_and_its_limits(ctx):
    """Seeds 7 and 8 of 6 x 8: row 0 of each has a member that is not its marker's and loses it -- not with max_drop = 0, not with
    min_views = C; the same call twice gives the same bytes"""
    cams, xyz, n, views, pts, idx = stacked("6x8", [7, 8])
    lim = cases.prune_limit(0.5)
    got, want = run_both(ctx, cams, xyz, n, views, pts=pts, idx=idx, max_res2=lim, max_drop=1, what="pruning")
    assert got["dropped"][:, 0].tolist() == [1 << 1, 1 << 3] and (got["dropped"][:, 1:] & 63 == 0)[got["status"][:, 1:] > 0].all()
    again, _ = run_both(ctx, cams, xyz, n, views, pts=pts, idx=idx, max_res2=lim, max_drop=1, what="pruning again")
    assert not rp.specified_equal(again, got) and all(again[k].tobytes() == got[k].tobytes() for k in rp.OUT_KEYS)
    for kw in (dict(max_drop=0), dict(max_drop=1, min_views=6), dict(max_drop=3)):
        g, w = run_both(ctx, cams, xyz, n, views, pts=pts, idx=idx, max_res2=lim, what=f"pruning {kw}", **kw)
        assert (g["dropped"][:, 0] == 0).all() == (kw != dict(max_drop=3))


# ---- the trackers ---------------------------------------------------------------------------------------------------------------
PW, PH, PC, PT = 640, 480, 3, 4
SUBPIX = {"radius": 24, "floor": 64}
REFINE = {"max_iters": 8, "max_res2": 4.0, "max_drop": 1}


@pytest.fixture(scope="module")
def rendered():
    """4 markers on 4 time steps, rendered as discs into 3 cameras of 640 x 480 (the frames of the rigid-body trackers' tests)"""
    import subpixel_ref as sref
    from mocapv2_amd import synth
    scene = synth.Scene(PC, PW, PH, dist=synth.MILD_DIST)
    first = sref.place_markers(scene, np.random.default_rng(70), 4, margin=SUBPIX["radius"] + 30, apart=2 * SUBPIX["radius"] + 12)
    frames = np.empty((PT, PC, PH, PW), np.uint8)
    for s in range(PT):
        markers = first + np.array([0.004 * s, -0.003 * s, 0.002 * s])
        rng = np.random.default_rng(170 + s)
        for c in range(PC):
            frames[s, c] = scene.render(rng, markers, c, radius_range=(15.0, 19.0))
    return scene, frames, first


def bytes_of(out, keys):
    """The bytes of a batch's outputs: of the per-row ones ([T, rows, ...]) the rows below n[t] -- the correspondence calls leave
    the others unspecified -- and the others whole"""
    import torch
    torch.cuda.synchronize()
    n = out["n"].cpu().numpy()
    res = {}
    for k in keys:
        v = out[k].cpu().numpy()
        if v.ndim >= 2 and v.shape[0] == len(n):
            v = v[np.arange(v.shape[1])[None, :] < n[:, None]]
        res[k] = v.tobytes()
    return res


@pytest.mark.parametrize("visibility", ["any", "all"])
@pytest.mark.parametrize("subpixel", [None, SUBPIX])
def test_tracker_refines_what_the_context_refines_by_hand(rendered, visibility, subpixel):
    import torch
    from mocapv2_amd.pipeline import BatchTracker, scene_arrays
    scene, frames, first = rendered
    arrays = scene_arrays(scene)
    dev = torch.from_numpy(frames.reshape(PT * PC, PH, PW)).cuda()
    kw = dict(visibility=visibility, subpixel=subpixel)
    # refine=None: the keys and the bytes of the tracker built without the keyword
    plain = BatchTracker(*arrays, PW, PH, PT, **kw)
    p_out = plain.step(dev)
    assert plain.finish(p_out).tolist() == [4] * PT
    none = BatchTracker(*arrays, PW, PH, PT, refine=None, **kw)
    n_out = none.step(dev)
    assert sorted(n_out) == sorted(p_out) and not set(BatchTracker.REFINE_KEYS.values()) & set(n_out)
    assert bytes_of(n_out, sorted(p_out)) == bytes_of(p_out, sorted(p_out))
    # refine={...}: the outputs that were there stay, the new ones are the context's call on them
    trk = BatchTracker(*arrays, PW, PH, PT, refine=REFINE, **kw)
    out = trk.step(dev)
    trk.finish(out)
    assert sorted(out) == sorted(list(p_out) + list(BatchTracker.REFINE_KEYS.values()))
    assert bytes_of(out, sorted(p_out)) == bytes_of(p_out, sorted(p_out))
    ctx = trk.ctx
    if visibility == "any":
        pts = trk.lanes[0].subpix["xy"] if subpixel else ctx.record_views(trk.records)[0]
        P = pts.shape[1]
        hand = ctx.refine_points(out["xyz"], out["n"], views=out["views"], pts=pts.reshape(PT, PC, P, 2).contiguous(), idx=out["idx"],
                                 min_views=2, **REFINE)
    else:
        hand = ctx.refine_points(out["xyz"], out["n"], grp=out["grp"], **REFINE)
    rows = torch.arange(out["xyz"].shape[1], device=dev.device)[None, :] < out["n"][:, None]
    for k, v in BatchTracker.REFINE_KEYS.items():
        assert torch.equal(out[v][rows], hand[k][rows]), (k, v)
    status = out["refine_status"][rows].cpu().numpy()
    moved = (out["xyz_refined"][rows] - out["xyz"][rows]).norm(dim=1).cpu().numpy()
    print(f"{visibility} subpixel {subpixel is not None}: statuses {np.bincount(status).tolist()}, moved {moved.min():.3g} .. {moved.max():.3g} m")
    assert (status > 0).all() and (moved > 0).all() and moved.max() < 5e-3
    # two batches in flight: the same bytes
    deep = BatchTracker(*arrays, PW, PH, PT, depth=2, refine=REFINE, **kw)
    outs = [deep.step(dev) for _ in range(2)]
    deep.synchronize()
    for o in outs:
        for v in BatchTracker.REFINE_KEYS.values():
            assert torch.equal(o[v][rows], out[v][rows]), v
    if subpixel is None:  # two ranks (both on this GPU, the all-gather replaced by the concatenation it produces): each its own steps
        T = PT // 2
        ranks = [BatchTracker(*arrays, PW, PH, T, world=2, rank=r, refine=REFINE, visibility=visibility) for r in range(2)]
        recs = [tr.extract(torch.from_numpy(np.stack([frames[t, c] for c, t in tr.local_image_list()])).cuda()).clone() for tr in ranks]
        gathered = torch.cat(recs, dim=0)
        for r, tr in enumerate(ranks):
            o = tr.refine_markers(tr.triangulate(gathered), gathered)
            for v in BatchTracker.REFINE_KEYS.values():
                assert torch.equal(o[v][rows[r * T:(r + 1) * T]], out[v][r * T:(r + 1) * T][rows[r * T:(r + 1) * T]]), (r, v)


@pytest.mark.parametrize("visibility", ["any", "all"])
def test_track_and_bodies_receive_the_refined_rows(rendered, visibility):
    import torch
    from mocapv2_amd.pipeline import BatchTracker, scene_arrays
    from mocapv2_amd.replay import ReplayTracker, unpack_tracker_message
    scene, frames, first = rendered
    arrays = scene_arrays(scene)
    model = first - first.mean(axis=0)
    dev = torch.from_numpy(frames.reshape(PT * PC, PH, PW)).cuda()
    kw = dict(visibility=visibility, refine=REFINE, track={"gate": 0.05}, bodies={"models": [model], "tol": 0.03, "gate": 0.03})
    trk = BatchTracker(*arrays, PW, PH, PT, **kw)
    out = trk.step(dev)
    trk.finish(out)
    xyz = out["xyz_refined"]
    if visibility == "all":
        xyz = torch.gather(xyz, 1, out["order"].clamp(0, xyz.shape[1] - 1).to(torch.int64)[:, :, None].expand(-1, -1, 3))
    ctx = trk.ctx
    poses = ctx.rigid_poses(xyz, out["n"], trk.body_tables, tol=0.03, gate=0.03)
    ids = ctx.track_markers(xyz, out["n"], ctx.track_state(64), gate=0.05)
    assert out["body_status"].cpu().tolist() == [[0]] * PT
    for k, v in BatchTracker.BODY_KEYS.items():
        assert torch.equal(out[v], poses[k]), v
    for k in ("id", "slot", "age", "status"):
        assert torch.equal(out[k], ids[k]), k
    # the poses are not those of the unrefined rows: the refinement moved the markers
    raw = out["xyz"] if visibility == "any" else torch.gather(out["xyz"], 1, out["order"].clamp(0, xyz.shape[1] - 1).to(torch.int64)[:, :, None].expand(-1, -1, 3))
    assert not torch.equal(ctx.rigid_poses(raw, out["n"], trk.body_tables, tol=0.03, gate=0.03)["t"], out["body_t"])
    # ReplayTracker passes the option through and reports the refined points
    rk = dict(batch=PT, visibility=visibility, refine=REFINE)
    res = list(ReplayTracker(*arrays[:4], arrays[4], PW, PH, **rk).run_batches(frames))
    assert len(res) == 1
    host = xyz.cpu().numpy()
    for s in range(PT):
        assert np.array_equal(res[0]["object_points"][s, :4], host[s, :4])  # (4 markers; obj_count + 1 = 5 rows)
        assert unpack_tracker_message(res[0]["messages"][s])[4:] == host[s, 0].tolist()
    plain = list(ReplayTracker(*arrays[:4], arrays[4], PW, PH, batch=PT, visibility=visibility).run_batches(frames))
    assert sorted(plain[0]) == sorted(res[0]) and plain[0]["messages"] != res[0]["messages"]
