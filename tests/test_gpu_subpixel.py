"""Sub-pixel centroids on the GPU (csrc/subpixel.hip through mocap_refine_centroids, MocapContext.refine_centroids and the
trackers' `subpixel`): bit equality with the NumPy restatement tests/subpixel_ref.py on hand-made blobs, through two lens models,
from raw Bayer frames, and through the whole pipeline."""
import ctypes as C

import numpy as np
import pytest

import subpixel_cases as cases
import subpixel_ref as ref
from lens_cases import case
from subpixel_cases import pyramid, records_of
from mocapv2_amd import synth

pytestmark = pytest.mark.gpu

W0, H0 = 93, 67     # the hand-made frames: odd sizes, nothing is aligned
SENT_XY, SENT_INFO = -12345.0, -1


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def strided(torch, frames, pad_rows, pad_cols):
    """the frames as a view into a larger buffer: pitch > width, images more than H * pitch apart; the padding holds 255s"""
    n, H, W = frames.shape
    big = torch.full((n, H + pad_rows, W + pad_cols), 255, dtype=torch.uint8, device="cuda")
    big[:, :H, :W] = torch.from_numpy(frames).cuda()
    return big[:, :H, :W]


def run(torch, ctx, frames_dev, rec, mb, rows=None, **kw):
    """refine_centroids into pre-filled buffers of `rows` >= mb rows per image -> (xy, info) host arrays"""
    n = frames_dev.shape[0] if frames_dev.dim() == 3 else 1
    rows = mb if rows is None else rows
    out = {"xy": torch.full((n, rows, 2), SENT_XY, dtype=torch.float64, device="cuda"),
           "info": torch.full((n, rows, 2), SENT_INFO, dtype=torch.int32, device="cuda")}
    ctx.refine_centroids(frames_dev, torch.from_numpy(rec).cuda(), max_blobs=mb, out=out, **kw)
    torch.cuda.synchronize()
    return out["xy"].cpu().numpy(), out["info"].cpu().numpy()


def expect(frames, rec, mb, rows=None, coords="ideal", **kw):
    """the restatement's answer in the layout of run(): sentinels where nothing is written"""
    n, cap = len(frames), (rec.shape[1] - 2) // 2
    rows = mb if rows is None else rows
    xy_i = rec[:, 2:].reshape(n, cap, 2)
    xy, S, fl = ref.refine_batch(frames, xy_i, rec[:, 0], coords=1 if coords == "ideal" else 0, max_blobs=mb, **kw)
    exy = np.full((n, rows, 2), SENT_XY)
    einfo = np.full((n, rows, 2), SENT_INFO, np.int32)
    exy[:, :mb] = np.where(np.isnan(xy), SENT_XY, xy)
    einfo[:, :mb, 0], einfo[:, :mb, 1] = S, fl
    return exy, einfo


def same_bits(got, want):
    return got.shape == want.shape and got.tobytes() == want.tobytes()


# ---- 1. hand-made blobs, identity slot ----------------------------------------------------------------------------------
def hand_made():
    f = np.zeros((7, H0, W0), np.uint8)
    f[:] = np.random.default_rng(3).integers(0, 9, f.shape, dtype=np.uint8)  # a little noise under every floor used
    pts = []
    for cx, cy in ((3, 30), (89, 20), (40, 2), (50, 64), (90, 64)):  # windows cut by each border and by a corner
        pyramid(f[0], cx, cy)
    pts.append([(3, 30), (89, 20), (40, 2), (50, 64), (90, 64)])
    pyramid(f[1], 30, 30, half=3)                                     # a start 5 px off: needs recentring
    pts.append([(35, 27)])
    pyramid(f[2], 60, 40)                                             # a blob touching the ring of radius 5, balanced
    f[2, 40, 55] = f[2, 40, 65] = 120
    pts.append([(60, 40)])
    pyramid(f[3], 20, 50)                                             # two blobs 10 px apart
    pyramid(f[3], 30, 50)
    pts.append([(20, 50), (30, 50)])
    f[4] = 254                                                        # nothing above floor 254
    pts.append([(10, 10), (80, 60)])
    pyramid(f[5], 46, 33, half=4, step=25)                            # counts: 0, negative, above max_blobs
    pts.append([(46, 33)])
    for k in range(8):
        pyramid(f[6], 8 + 11 * k, 12 + 6 * (k % 2))
    pts.append([(8 + 11 * k, 12 + 6 * (k % 2)) for k in range(8)])
    return f, pts


@pytest.mark.parametrize("layout", ["contiguous", "pitch_and_stride"])
def test_hand_made_blobs_equal_the_restatement(torch_cuda, layout):
    from mocapv2_amd.engine import MocapContext
    torch = torch_cuda
    frames, pts = hand_made()
    ctx = MocapContext(W0, H0)
    assert ctx.set_undistort(0, synth.intrinsics(W0, H0), synth.ZERO_DIST)
    dev = torch.from_numpy(frames).cuda() if layout == "contiguous" else strided(torch, frames, 3, 11)
    rec = records_of(pts)
    seen = 0
    for radius, floor, iters in ((1, 10, 3), (5, 10, 3), (6, 10, 3), (9, 10, 1), (9, 10, 2), (12, 10, 8), (31, 10, 3), (31, 0, 3),
                                 (6, 254, 3)):
        got = run(torch, ctx, dev, rec, 8, rows=11, radius=radius, floor=floor, iters=iters)  # output strides wider than the rows
        want = expect(frames, rec, 8, rows=11, radius=radius, floor=floor, iters=iters)
        assert same_bits(got[0], want[0]) and same_bits(got[1], want[1]), (radius, floor, iters)
        fl = want[1][:, :, 1]
        if (radius, floor) == (6, 10):   # the cases are what they are meant to be
            assert (fl[0, :5] == ref.CUT).all() and fl[3, 0] == fl[3, 1] == 0
        if (radius, iters) == (9, 1):
            assert fl[1, 0] == ref.MOVING and want[0][1, 0].tolist() == [35.0, 27.0]
        if (radius, iters) == (9, 2):
            assert fl[1, 0] == 0 and want[0][1, 0].tolist() == [30.0, 30.0]
        if radius == 5:
            assert fl[2, 0] == ref.EDGE
        if radius == 12:
            assert fl[3, 0] & ref.NEIGHBOUR and fl[3, 1] & ref.NEIGHBOUR
        if floor == 254:
            assert (fl[4, :2] & ref.EMPTY).all() and (want[1][4, :2, 0] == 0).all()
        seen |= int(np.bitwise_or.reduce(fl[fl >= 0]))
    assert seen == ref.EMPTY | ref.EDGE | ref.NEIGHBOUR | ref.MOVING | ref.CUT
    # counts 0, negative and above max_blobs (the first max_blobs points are refined, nothing else is written)
    rec2 = records_of(pts, counts=[0, -3, 1, 2, 2, 1, 8])
    for mb in (1, 5, 8):
        got = run(torch, ctx, dev, rec2, mb, rows=9, radius=6, floor=10)
        want = expect(frames, rec2, mb, rows=9, radius=6, floor=10)
        assert same_bits(got[0], want[0]) and same_bits(got[1], want[1]), mb
        assert (got[1][:2] == SENT_INFO).all() and (got[1][6, :mb, 1] >= 0).all() and (got[1][6, mb:] == SENT_INFO).all()


def test_one_image_and_no_info_buffer(torch_cuda):
    """a [H, W] frame (image_stride plays no part) through the C-ABI with out_info = NULL"""
    from mocapv2_amd.engine import MocapContext, _ptr, _stream
    torch = torch_cuda
    frames, pts = hand_made()
    ctx = MocapContext(W0, H0)
    ctx.set_undistort(0, synth.intrinsics(W0, H0), synth.ZERO_DIST)
    rec = records_of(pts[:1])
    d_f, d_r = torch.from_numpy(frames[0]).cuda(), torch.from_numpy(rec).cuda()
    xy = torch.full((1, 8, 2), SENT_XY, dtype=torch.float64, device="cuda")
    rc = ctx.lib.mocap_refine_centroids(ctx._h, _ptr(d_f), 1, 1, 0, 0, W0, -1, 0, C.c_void_p(d_r.data_ptr() + 8), rec.shape[1], _ptr(d_r),
                                        rec.shape[1], 8, 6, 10, 3, 1, _ptr(xy), 16, None, 0, _stream())
    torch.cuda.synchronize()
    assert rc == 0 and same_bits(xy.cpu().numpy(), expect(frames[:1], rec, 8, radius=6, floor=10)[0])


# ---- 2. two lens models, slots 1 and 2 of a three-slot context ----------------------------------------------------------------
LENS_W, LENS_H, LENS_R, LENS_FLOOR = 640, 360, 26, 64


def lens_scene():
    a, b = case("offcentre_fy125"), case("barrel_k123")
    scene = synth.MixedScene(2, LENS_W, LENS_H, Ks=[a.K, b.K], dists=[a.dist, b.dist])
    T, M = 2, 4
    frames = np.empty((T, 2, LENS_H, LENS_W), np.uint8)
    for t in range(T):
        rng = np.random.default_rng(40 + t)
        mk = ref.place_markers(scene, rng, M, margin=LENS_R + 22, apart=2 * LENS_R + 2)
        for c in range(2):
            frames[t, c] = scene.render(rng, mk, c, radius_range=(15.0, 19.0))
    return scene, frames.reshape(T * 2, LENS_H, LENS_W), T, M


def test_two_lens_models_both_coordinates_and_the_visible_correspondence(torch_cuda):
    from mocapv2_amd.engine import MocapContext
    torch = torch_cuda
    scene, frames, T, M = lens_scene()
    ctx = MocapContext(LENS_W, LENS_H, n_slots=3)
    ident = [ctx.set_undistort(0, synth.intrinsics(LENS_W, LENS_H), synth.MILD_DIST)]  # a third lens in the slot a wrong index would take
    ident += [ctx.set_undistort(1 + c, scene.Ks[c], scene.dists[c]) for c in range(2)]
    assert ident == [False, False, False]
    dev = torch.from_numpy(frames).cuda()
    records = ctx.blob_centroids(dev, cam_mod=2, slot_base=1, max_blobs=8)
    rec = records.cpu().numpy()
    assert (rec[:, 0] == M).all()
    lenses = [(scene.Ks[c], scene.dists[c], False) for c in range(2)]
    outs = {}
    for coords in ("ideal", "raw"):
        out = ctx.refine_centroids(dev, records, cam_mod=2, slot_base=1, radius=LENS_R, floor=LENS_FLOOR, coords=coords)
        torch.cuda.synchronize()
        want = expect(frames, rec, 8, coords=coords, radius=LENS_R, floor=LENS_FLOOR, lenses=lenses, cam_mod=2)
        got_xy, got_info = out["xy"].cpu().numpy(), out["info"].cpu().numpy()
        live = want[1][:, :, 1] >= 0
        assert same_bits(got_xy[live], want[0][live]) and same_bits(got_info[live], want[1][live]), coords
        assert live.sum() == 4 * M and not (want[1][:, :, 1][live] & ref.FALLBACK).any()
        assert same_bits(out["flags"].cpu().numpy()[live], want[1][:, :, 1][live])
        outs[coords] = out["xy"]
    moved = np.abs(outs["raw"].cpu().numpy()[:, :M] - outs["ideal"].cpu().numpy()[:, :M]).max(axis=(1, 2))
    assert (moved > 0.02).all() and moved.max() > 0.25  # both lenses do move the points
    # the slot index counts: the same call on slots 0 and 1 answers differently
    other = ctx.refine_centroids(dev, records, cam_mod=2, slot_base=0, radius=LENS_R, floor=LENS_FLOOR)["xy"]
    assert not same_bits(other.cpu().numpy()[:, :M], outs["ideal"].cpu().numpy()[:, :M])
    # raw points with distorted=True and ideal points with distorted=False are the same markers
    ctx.set_cameras(np.stack(scene.Ks), np.stack(scene.dists), np.stack([p["R"] for p in scene.poses]),
                    np.stack([p["t"] for p in scene.poses]))
    counts = records[:, 0].reshape(T, 2).contiguous()
    vis = {c: ctx.correspond_visible(outs[c].reshape(T, 2, 8, 2), counts, distorted=c == "raw") for c in ("ideal", "raw")}
    torch.cuda.synchronize()
    n = vis["ideal"]["n"].cpu().numpy()
    assert (n == M).all() and np.array_equal(n, vis["raw"]["n"].cpu().numpy())
    for k in ("xyz", "err", "idx", "views"):  # (the same five rounds on the same raw points: the same bits)
        a, b = vis["ideal"][k].cpu().numpy()[:, :M], vis["raw"][k].cpu().numpy()[:, :M]
        assert same_bits(a, b), k


# ---- 3. raw Bayer frames --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", [14, 15])
def test_bayer_frames_equal_the_gray_path(torch_cuda, shift):
    from mocapv2_amd.engine import MocapContext
    torch = torch_cuda
    rng = np.random.default_rng(5)
    raw = rng.integers(0, 50, (2, H0, W0), dtype=np.uint8)
    spots = [(0, 33), (W0 - 1, 20), (45, 0), (30, H0 - 1), (W0 - 1, H0 - 1), (0, 0), (50, 35)]  # every border, two corners, the inside
    for i in range(2):
        for cx, cy in spots:
            pyramid(raw[i], cx, cy, half=4, step=20)
    raw[:, 0::2, 1::2] = (raw[:, 0::2, 1::2] * 0.8).astype(np.uint8)   # the colour sites respond differently
    raw[:, 1::2, 0::2] = (raw[:, 1::2, 0::2] * 0.9).astype(np.uint8)
    rec = records_of([spots, [(x + (1 if x < 50 else -1), y) for x, y in spots]])
    ctx = MocapContext(W0, H0)
    ctx.set_undistort(0, synth.intrinsics(W0, H0), synth.ZERO_DIST)
    d_raw = torch.from_numpy(raw).cuda()
    grays = []
    for pattern in range(4):
        gray = ctx.bayer_gray(d_raw, pattern, shift)
        torch.cuda.synchronize()
        grays.append(gray.cpu().numpy())
        for radius in (3, 7):
            a = run(torch, ctx, d_raw, rec, 8, radius=radius, floor=30, bayer_pattern=pattern, gray_shift=shift)
            b = run(torch, ctx, gray, rec, 8, radius=radius, floor=30)
            assert same_bits(a[0], b[0]) and same_bits(a[1], b[1]), (pattern, radius)
            want = expect(grays[-1], rec, 8, radius=radius, floor=30)
            assert same_bits(b[0], want[0]) and same_bits(b[1], want[1])
            assert (want[1][:, :6, 1] & ref.CUT).all() and (want[1][:, :7, 0] > 0).all()
    assert not np.array_equal(grays[0], grays[1]) and not np.array_equal(grays[0], grays[3])  # the patterns do differ


# ---- 3b. full lists of 256 blobs, and starts outside the frame (tests/subpixel_cases.py; test_subpixel_host says what they hold) --
def identity_ctx(W, H):
    from mocapv2_amd.engine import MocapContext
    ctx = MocapContext(W, H)
    assert ctx.set_undistort(0, synth.intrinsics(W, H), synth.ZERO_DIST)
    return ctx


def both(torch, ctx, frames, rec, mb, rows=None, ref_kw={}, **kw):
    """run() against expect(), bit for bit -> the restatement's (xy, info)"""
    got = run(torch, ctx, torch.from_numpy(frames).cuda(), rec, mb, rows=rows, **kw)
    want = expect(frames, rec, mb, rows=rows, **kw, **ref_kw)
    bad = np.argwhere(got[1] != want[1])
    assert same_bits(got[1], want[1]), (kw, bad[:4].tolist(), got[1][tuple(bad[0])], want[1][tuple(bad[0])])
    assert same_bits(got[0], want[0]), (kw, np.argwhere(got[0] != want[0])[:4].tolist())
    return want


@pytest.fixture(scope="module")
def dense():
    frame, centres, pts = cases.dense_frame()
    return frame[None], records_of([pts], cap=256), identity_ctx(cases.W1, cases.H1)


@pytest.mark.parametrize("radius", [4, 11, 12])
def test_256_blobs_in_permuted_rows(torch_cuda, dense, radius):
    """One centroid per thread up to the last, 64 trips of the four waves.  Radius 4: no flag; 12: every row has a neighbour at
    exactly dy == r; 11: the same one pixel short"""
    frames, rec, ctx = dense
    fl = both(torch_cuda, ctx, frames, rec, 256, radius=radius, floor=cases.FLOOR)[1][0, :, 1]
    assert not fl.any() if radius == 4 else (fl & ref.NEIGHBOUR).all() if radius == 12 else (fl == ref.EDGE).sum() == 20


def test_counts_about_a_wave_and_about_the_limit(torch_cuda, dense):
    """Counts 1, 64, 65, 255, 256 and 300 (above max_blobs = 256: the first 256 rows are refined) in one batch; max_blobs = 100 on
    a count of 256: the rows from 100 on keep the sentinel, and the first 100 see only each other as neighbours"""
    frames, rec, ctx = dense
    counts = [1, 64, 65, 255, 256, 300]
    many = np.repeat(rec, len(counts), axis=0)
    many[:, 0] = counts
    for radius in (4, 12):
        info = both(torch_cuda, ctx, np.repeat(frames, len(counts), axis=0), many, 256, radius=radius, floor=cases.FLOOR)[1]
        assert [(info[i, :, 1] >= 0).sum() for i in range(len(counts))] == [1, 64, 65, 255, 256, 256]
        assert same_bits(info[4], info[5])
    info = both(torch_cuda, ctx, frames, rec, 100, rows=256, radius=12, floor=cases.FLOOR)[1]
    assert (info[0, 100:] == SENT_INFO).all() and (info[0, :100, 1] >= 0).all()


def test_a_neighbour_only_one_lane_of_one_trip_sees(torch_cuda):
    frame, pts = cases.sparse_frame()
    info = both(torch_cuda, identity_ctx(cases.W2, cases.H2), frame[None], records_of([pts], cap=256), 256, radius=cases.RADIUS2,
                floor=cases.FLOOR)[1]
    assert np.flatnonzero(info[0, :, 1] & ref.NEIGHBOUR).tolist() == sorted(r for pair in cases.PAIRS for r in pair)


@pytest.mark.parametrize("coords", ["ideal", "raw"])
def test_starts_outside_the_frame(torch_cuda, coords):
    """Integer centroids beyond each border, beyond a corner and at the ends of the int32 range: the window starts at the clamped
    pixel; where it is empty the point comes back as it was handed in, not clamped"""
    frame, pts = cases.outside_frame()
    ctx = identity_ctx(cases.W3, cases.H3)
    empty = [k for k in range(len(pts)) if k not in cases.OUTSIDE_LIT]
    for radius, iters in cases.OUTSIDE_WINDOWS:
        xy, info = both(torch_cuda, ctx, frame[None], records_of([pts], cap=16), 16, radius=radius, floor=cases.FLOOR, iters=iters,
                        coords=coords)
        assert (info[0, empty, 1] == ref.EMPTY | ref.CUT).all() and xy[0, empty].tolist() == pts[empty].astype(float).tolist()
        assert (info[0, list(cases.OUTSIDE_LIT), 0] > 0).all()


@pytest.mark.parametrize("coords", ["ideal", "raw"])
def test_a_lens_slot_with_256_centroids_from_corner_to_corner(torch_cuda, coords):
    """distort_pt in every thread of the workgroup, undistort_pt behind 128 of the 256 windows (the others are EMPTY); the
    restatement clamps none of these starts (test_subpixel_host)"""
    from mocapv2_amd.engine import MocapContext
    frame, pts, start, clamped, lens = cases.lens_frame()
    ctx = MocapContext(cases.LENS_W, cases.LENS_H)
    assert not ctx.set_undistort(0, lens[0], lens[1])
    info = both(torch_cuda, ctx, frame[None], records_of([pts], cap=256), 256, radius=cases.LENS_RADIUS, floor=cases.FLOOR, coords=coords,
                ref_kw={"lenses": [lens]})[1]
    assert (info[0, :, 1] == 0).sum() == 128


def test_256_blobs_in_a_raw_bayer_frame(torch_cuda, dense):
    """The dense frame read as a raw Bayer frame (pattern 3, shift 14): window_sums' two-rows-per-trip form on a full list"""
    torch = torch_cuda
    frames, rec, ctx = dense
    d_raw = torch.from_numpy(frames).cuda()
    gray = ctx.bayer_gray(d_raw, 3, 14)
    torch.cuda.synchronize()
    for radius in (4, 12):
        a = run(torch, ctx, d_raw, rec, 256, radius=radius, floor=cases.FLOOR, bayer_pattern=3, gray_shift=14)
        b = run(torch, ctx, gray, rec, 256, radius=radius, floor=cases.FLOOR)
        assert same_bits(a[0], b[0]) and same_bits(a[1], b[1]), radius
        want = expect(gray.cpu().numpy(), rec, 256, radius=radius, floor=cases.FLOOR)
        assert same_bits(b[0], want[0]) and same_bits(b[1], want[1]) and (want[1][0, :, 0] > 0).all()


# ---- 4. the pipeline ------------------------------------------------------------------------------------------------------
PW, PH, PC, PT, PM = 640, 480, 3, 2, 4
SUBPIX = {"radius": 24, "floor": 64}


def pipeline_scene():
    scene = synth.Scene(PC, PW, PH, dist=synth.MILD_DIST)
    frames = np.empty((PT, PC, PH, PW), np.uint8)
    markers = []
    for t in range(PT):
        rng = np.random.default_rng(70 + t)
        mk = ref.place_markers(scene, rng, PM, margin=SUBPIX["radius"] + 22, apart=2 * SUBPIX["radius"] + 2)
        markers.append(mk)
        for c in range(PC):
            frames[t, c] = scene.render(rng, mk, c, radius_range=(15.0, 19.0))
    return scene, frames.reshape(PT * PC, PH, PW), np.array(markers)


def rms_to_truth(xyz, n, markers):
    d2 = []
    for t in range(len(n)):
        for p in xyz[t, :n[t]]:
            d2.append(((markers[t] - p) ** 2).sum(axis=1).min())
    return float(np.sqrt(np.mean(d2)))


@pytest.mark.parametrize("visibility", ["all", "any"])
def test_batch_tracker_equals_the_calls_chained_by_hand(torch_cuda, visibility):
    """BatchTracker(subpixel=...) on 3 cameras x 2 time steps x 4 markers at 640 x 480, depth 1 and 2, both batches of the deeper
    one: the outputs of blob_centroids -> refine_centroids(coords="ideal") -> correspond[_visible]_records(points=...) on a
    context of the test's own, bit for bit.  The 3-D points lie closer to the true markers than those of subpixel=None (only the
    direction is asserted; the size is test_subpixel_host's business).  RMS distance to the true markers, measured on the
    MI355X, both visibilities alike: 0.000036 world units with subpixel (0.036 mm at 3 m), 0.004941 with integer centroids."""
    from mocapv2_amd.engine import MocapContext
    from mocapv2_amd.pipeline import BatchTracker, scene_arrays
    torch = torch_cuda
    scene, frames, markers = pipeline_scene()
    K, dist, R, t, F = scene_arrays(scene)
    dev = torch.from_numpy(frames).cuda()
    ctx = MocapContext(PW, PH, n_slots=PC)
    for c in range(PC):
        ctx.set_undistort(c, K[c], dist[c])
    ctx.set_cameras(K, dist, R, t)
    ctx.set_fundamentals(F)
    records = ctx.blob_centroids(dev, cam_mod=PC, max_blobs=32)
    pts = ctx.refine_centroids(dev, records, cam_mod=PC, coords="ideal", **SUBPIX)
    if visibility == "all":
        want = ctx.correspond_records(records, PT, PC, P=32, points=pts["xy"])
    else:
        want = ctx.correspond_visible_records(records, PT, PC, P=32, points=pts["xy"])
    torch.cuda.synchronize()
    n = want["n"].cpu().numpy()
    assert (n == PM).all(), n
    assert (records[:, 0] == PM).all() and not (pts["flags"][:, :PM] & ref.FALLBACK).any()

    def rows(out):
        return {k: v.cpu().numpy()[:, :PM] if v.dim() > 1 else v.cpu().numpy() for k, v in out.items() if k != "subpix_flags"}

    want_rows = rows(want)
    rms = {}
    for depth in (1, 2):
        tr = BatchTracker(K, dist, R, t, F, PW, PH, PT, depth=depth, visibility=visibility, subpixel=SUBPIX)
        outs = [tr.step(dev) for _ in range(2)]  # the same batch twice (depth 2: in flight together, one lane each)
        tr.synchronize()
        for out in outs:
            got = rows(out)
            assert sorted(got) == sorted(want_rows)
            for k in got:
                assert same_bits(got[k], want_rows[k]), (depth, k)
            assert same_bits(out["subpix_flags"].cpu().numpy(), pts["flags"].cpu().numpy())
        rms["subpixel"] = rms_to_truth(outs[0]["xyz"].cpu().numpy(), n, markers)
    plain = BatchTracker(K, dist, R, t, F, PW, PH, PT, visibility=visibility)
    out0 = plain.step(dev)
    torch.cuda.synchronize()
    assert "subpix_flags" not in out0 and (out0["n"].cpu().numpy() == PM).all()
    rms["integer"] = rms_to_truth(out0["xyz"].cpu().numpy(), n, markers)
    print(f"visibility={visibility}: RMS distance to the true markers {rms['subpixel']:.6f} (subpixel) {rms['integer']:.6f} (integer centroids)")
    assert rms["subpixel"] < rms["integer"]


# ---- 5. bad arguments -------------------------------------------------------------------------------------------------------
def test_bad_arguments_launch_nothing(torch_cuda):
    from mocapv2_amd.engine import MocapContext, _ptr, _stream
    torch = torch_cuda
    frames, pts = hand_made()
    raw = torch.from_numpy(frames).cuda()
    rec = torch.from_numpy(records_of(pts)).cuda()
    ri = rec.shape[1]
    ctx = MocapContext(W0, H0, n_slots=2)
    ctx.set_undistort(0, synth.intrinsics(W0, H0), synth.ZERO_DIST)  # slot 1 stays unset
    tiny = MocapContext(2, 2)  # (Bayer frames need H, W >= 3: refused before anything else is looked at)
    xy = torch.full((7, 8, 2), SENT_XY, dtype=torch.float64, device="cuda")
    info = torch.full((7, 8, 2), SENT_INFO, dtype=torch.int32, device="cuda")

    def call(c=ctx, n=7, cam_mod=1, slot_base=0, pattern=-1, shift=15, mb=8, radius=6, floor=10, iters=3, coords=1, xy_st=16,
             info_st=16, out=xy):
        return c.lib.mocap_refine_centroids(c._h, _ptr(raw), n, cam_mod, slot_base, H0 * W0, W0, pattern, shift,
                                            C.c_void_p(rec.data_ptr() + 8), ri, _ptr(rec), ri, mb, radius, floor, iters, coords,
                                            _ptr(out), xy_st, _ptr(info), info_st, _stream())

    invalid = [dict(radius=0), dict(radius=32), dict(floor=-1), dict(floor=255), dict(iters=0), dict(iters=9), dict(coords=2),
               dict(coords=-1), dict(pattern=4), dict(pattern=-2), dict(pattern=3, shift=13), dict(mb=0), dict(mb=257),
               dict(xy_st=15), dict(info_st=15), dict(n=0), dict(cam_mod=0), dict(cam_mod=3), dict(slot_base=2), dict(out=None),
               dict(c=tiny, pattern=0, n=1)]
    for kw in invalid:
        assert call(**kw) == -1, kw            # MOCAP_E_INVALID
        assert ctx.lib.mocap_last_error()
    assert call(slot_base=1) == -4              # MOCAP_E_STATE: mocap_set_undistort was not called for slot 1
    assert call(cam_mod=2) == -4
    torch.cuda.synchronize()
    assert (xy == SENT_XY).all() and (info == SENT_INFO).all()
    assert call() == 0                          # ... and the same buffers with good arguments are written
    torch.cuda.synchronize()
    assert not (xy[0, :5] == SENT_XY).any() and (info[0, :5, 1] == ref.CUT).all()
