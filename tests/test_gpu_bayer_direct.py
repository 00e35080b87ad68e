"""Raw Bayer frames in, centroid records out, with no gray frame in memory (mocap_blob_centroids_bayer with a NULL gray
buffer, ABI 6).  The reference for every comparison is a second context fed ctx.bayer_gray(raw) and then blob_centroids
(the two-step path); the records must be bit-equal on the gray-less path (fused scan without write-back, box kernel's
Bayer form) and on the context's scratch fallback alike."""
import ctypes as C

import numpy as np
import pytest

import oracle
from lens_cases import case
from mocapv2_amd.synth import MILD_DIST, ZERO_DIST, Scene

pytestmark = pytest.mark.gpu

MAX_BLOBS = 32


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def bayer_frames(rng, n, H, W, n_discs, edges=False, noise_max=60):
    """Dark sensor frames with saturated discs whose colour sites respond differently; edges=True puts one disc on each
    image edge and one on a corner (the clamp at rows 0 / H-1 and columns 0 / W-1)."""
    img = rng.integers(0, noise_max + 1, (n, H, W), dtype=np.uint8)
    yy, xx = np.mgrid[0:H, 0:W]
    for i in range(n):
        k = int(0.001 * H * W)
        img[i, rng.integers(0, H, k), rng.integers(0, W, k)] = 255
        discs = [(rng.uniform(0, W), rng.uniform(0, H), rng.uniform(6, 20)) for _ in range(n_discs)]
        if edges:
            r = min(H, W) / 6
            discs += [(0.0, H / 2, r), (W - 1.0, H / 3, r), (W / 2, 0.0, r), (W / 3, H - 1.0, r), (W - 1.0, H - 1.0, r)]
        for cx, cy, r in discs:
            d = np.sqrt((xx - cx) ** 2 + (yy - cy) ** 2)
            img[i] = np.maximum(img[i], (np.clip((r + 0.75 - d) / 1.5, 0, 1) * 255).astype(np.uint8))
    img[:, 0::2, 1::2] = (img[:, 0::2, 1::2] * 0.9).astype(np.uint8)
    img[:, 1::2, 0::2] = (img[:, 1::2, 0::2] * 0.95).astype(np.uint8)
    return img


def context_pair(W, H, K, dists, min_area=60.0):
    """(context under test, reference context) with the same slots"""
    from mocapv2_amd.engine import MocapContext
    pair = []
    for _ in range(2):
        ctx = MocapContext(W, H, n_slots=len(dists))
        for sl, d in enumerate(dists):
            ctx.set_undistort(sl, K, d)
        ctx.set_blob_params(min_area=min_area)
        pair.append(ctx)
    return pair


def check_batch(torch, ctx, ref, d, cam_mod, pattern, shift):
    """records of the gray-less call = records of the two-step path; returns the centroids found"""
    rec = ctx.blob_centroids(d, cam_mod=cam_mod, max_blobs=MAX_BLOBS, bayer_pattern=pattern, gray_shift=shift).cpu().numpy()
    two = ref.blob_centroids(ref.bayer_gray(d, pattern, shift), cam_mod=cam_mod, max_blobs=MAX_BLOBS).cpu().numpy()
    for i in range(rec.shape[0]):  # count and centroid pairs (the words after them are not written)
        k = rec[i, 0]
        assert k == two[i, 0] and 0 <= k <= MAX_BLOBS and np.array_equal(rec[i, 2:2 + 2 * k], two[i, 2:2 + 2 * k]), i
    return int(rec[:, 0].sum())


def run_case(torch, W, H, dists, pattern=3, shift=15, n=4, n_discs=4, edges=False, seed=0, batches=2, K=None):
    sc = Scene(len(dists), width=W, height=H)
    ctx, ref = context_pair(W, H, sc.K if K is None else K, dists)
    rng = np.random.default_rng(seed)
    found = 0
    for _ in range(batches):  # consecutive batches on one context: the mask's carry-over
        raw = bayer_frames(rng, n, H, W, n_discs, edges=edges)
        found += check_batch(torch, ctx, ref, torch.from_numpy(raw).cuda(), len(dists), pattern, shift)
    return found


# ---- 1. the C-ABI accepts NULL ------------------------------------------------------------------------------------------
def test_abi_accepts_null_gray_buffer(torch_cuda):
    from mocapv2_amd import _abi
    from mocapv2_amd.engine import _ptr, _stream
    torch = torch_cuda
    W, H, n = 640, 360, 4
    ctx, ref = context_pair(W, H, Scene(1, width=W, height=H).K, [MILD_DIST])
    raw = torch.from_numpy(bayer_frames(np.random.default_rng(1), n, H, W, 4)).cuda()
    rec_ints = 2 + 2 * MAX_BLOBS
    records = torch.zeros((n, rec_ints), dtype=torch.int32, device="cuda")
    rc = ctx.lib.mocap_blob_centroids_bayer(ctx._h, _ptr(raw), None, n, 1, 0, H * W, W, 3, 15,
                                            C.c_void_p(records.data_ptr() + 8), rec_ints, _ptr(records), rec_ints, MAX_BLOBS,
                                            _stream())
    assert rc == 0, rc  # ABI 5 answered MOCAP_E_INVALID ("null argument")
    assert _abi.ABI_VERSION == ctx.lib.mocap_abi_version() >= 6
    two = ref.blob_centroids(ref.bayer_gray(raw, 3, 15), max_blobs=MAX_BLOBS).cpu().numpy()
    got = records.cpu().numpy()
    for i in range(n):
        k = two[i, 0]
        assert got[i, 0] == k and np.array_equal(got[i, 2:2 + 2 * k], two[i, 2:2 + 2 * k]), i
    assert two[:, 0].sum() > 0


# ---- 2. no gray tensor is allocated --------------------------------------------------------------------------------------
def test_no_frame_sized_allocation(torch_cuda):
    torch = torch_cuda
    W, H, n = 640, 360, 12
    ctx, _ = context_pair(W, H, Scene(1, width=W, height=H).K, [MILD_DIST])
    raw = torch.from_numpy(bayer_frames(np.random.default_rng(2), n, H, W, 4)).cuda()
    records = torch.zeros((n, 2 + 2 * MAX_BLOBS), dtype=torch.int32, device="cuda")
    ctx.blob_centroids(raw, max_blobs=MAX_BLOBS, records=records, bayer_pattern=3)  # first call: the library's own buffers
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.max_memory_allocated()
    ctx.blob_centroids(raw, max_blobs=MAX_BLOBS, records=records, bayer_pattern=3)
    torch.cuda.synchronize()
    assert torch.cuda.max_memory_allocated() - before < H * W  # the two-step form allocates n * H * W


# ---- 3. bit-equality across patterns, shifts, geometry and lenses --------------------------------------------------------
@pytest.mark.parametrize("pattern", [0, 1, 2, 3])
@pytest.mark.parametrize("shift", [14, 15])
def test_patterns_and_shifts(torch_cuda, pattern, shift):
    assert run_case(torch_cuda, 640, 360, [MILD_DIST, ZERO_DIST], pattern, shift, seed=10 * pattern + shift, edges=True) > 0


# sizes of the gray-less path (640 x 360, 1920 x 1080, the small 96 x 64), then sizes the scratch fallback takes: 648 x 364 (W % 16, H % 8),
# 203 x 117 (odd)
@pytest.mark.parametrize("W,H", [(640, 360), (1920, 1080), (648, 364), (96, 64), (203, 117)])
@pytest.mark.parametrize("lens", ["zero", "mild"])
def test_geometry(torch_cuda, W, H, lens):
    dist = ZERO_DIST if lens == "zero" else MILD_DIST
    found = run_case(torch_cuda, W, H, [dist], pattern=(W + H) % 4, shift=14 + W % 2, n_discs=4 if W >= 640 else 1, edges=True,
                     seed=W + H)
    assert found > 0


@pytest.mark.parametrize("name", ["barrel_k123", "pincushion", "offcentre_fy125"])
def test_strong_lenses(torch_cuda, name):
    lc = case(name)
    assert run_case(torch_cuda, lc.W, lc.H, [lc.dist, lc.dist], K=lc.K, pattern=3, n=4, n_discs=5, edges=True, seed=7) > 0


@pytest.mark.parametrize("W,H", [(640, 360), (648, 364)])
def test_identity_and_remapped_slots_in_one_batch(torch_cuda, W, H):
    """cam_mod = 2: slot 0 the identity (identity items), slot 1 remapped (staged items)"""
    assert run_case(torch_cuda, W, H, [ZERO_DIST, MILD_DIST], pattern=2, shift=14, n=6, edges=True, seed=5) > 0


@pytest.mark.parametrize("offset", [16, 1])
def test_padded_view(torch_cuda, offset):
    """pitch > W, image stride > H * pitch; offset 16 keeps the gray-less path (16-byte aligned), offset 1 takes the fallback"""
    torch = torch_cuda
    W, H, n, P = 640, 360, 4, 672
    sc = Scene(2, width=W, height=H)
    ctx, ref = context_pair(W, H, sc.K, [ZERO_DIST, MILD_DIST])
    rng = np.random.default_rng(offset)
    for _ in range(2):
        raw = bayer_frames(rng, n, H, W, 4, edges=True)
        buf = torch.zeros((n, H + 5, P), dtype=torch.uint8, device="cuda")
        view = buf[:, 2:2 + H, offset:offset + W]
        view.copy_(torch.from_numpy(raw).cuda())
        assert view.stride(1) == P and view.stride(0) > H * P
        assert check_batch(torch, ctx, ref, view, 2, 3, 15) > 0


def test_gray_buffer_is_still_filled(torch_cuda):
    """A tensor passed as `gray` keeps its meaning: it receives the gray frames."""
    from mocapv2_amd.engine import GRAY_SHIFT
    torch = torch_cuda
    W, H = 640, 360
    ctx, ref = context_pair(W, H, Scene(1, width=W, height=H).K, [MILD_DIST])
    raw = bayer_frames(np.random.default_rng(4), 3, H, W, 4)
    d = torch.from_numpy(raw).cuda()
    gray = torch.zeros_like(d)
    rec = ctx.blob_centroids(d, max_blobs=MAX_BLOBS, bayer_pattern=3, gray=gray).cpu().numpy()
    rec0 = ref.blob_centroids(d, max_blobs=MAX_BLOBS, bayer_pattern=3).cpu().numpy()
    assert np.array_equal(rec[:, 0], rec0[:, 0]) and rec[:, 0].sum() > 0
    for i in range(3):
        assert np.array_equal(rec[i, 2:2 + 2 * rec[i, 0]], rec0[i, 2:2 + 2 * rec[i, 0]])
    g = gray.cpu().numpy()
    for i in range(3):
        assert np.array_equal(g[i], oracle.bayer_gray(raw[i], 3, GRAY_SHIFT))


# ---- 4. every source path of the Bayer box kernel, and the fallback switches ---------------------------------------------
@pytest.mark.parametrize("env", [
    {"MOCAP_BOX_STAGE_BYTES": "0"},      # taps from memory
    {"MOCAP_BOX_STAGE_BYTES": "600"},    # staged and unstaged items side by side
    {"MOCAP_WIDE_QUADS": "0,0"},         # tiles that would be wide (the gray-less path makes them box items)
    {"MOCAP_SKIP_DARK": "0"},            # scratch fallback: the dense path
    {"MOCAP_GENERAL_FILTER": "1"},       # scratch fallback: the general kernel
    {"MOCAP_CLUSTER": "0"},
])
@pytest.mark.parametrize("lens", ["mild", "barrel_k123"])
def test_tuning_switches(torch_cuda, monkeypatch, env, lens):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    if lens == "mild":
        found = run_case(torch_cuda, 640, 360, [ZERO_DIST, MILD_DIST], pattern=1, shift=15, n=4, edges=True, seed=len(str(env)))
    else:
        lc = case(lens)
        found = run_case(torch_cuda, lc.W, lc.H, [lc.dist], K=lc.K, pattern=0, shift=14, n=3, edges=True, seed=3)
    assert found > 0


# ---- 5. a crowded scene --------------------------------------------------------------------------------------------------
def test_crowded_scene(torch_cuda):
    """32 markers per 1080p frame: on the gray path many tiles go through the wide-tile row pipeline; the gray-less path
    filters them as box items.  Same records."""
    torch = torch_cuda
    W, H = 1920, 1080
    sc = Scene(2, width=W, height=H, dist=MILD_DIST)
    frames = sc.render_batch(seed=11, n_steps=2, n_markers=32)  # [T, C, H, W] gray
    raw = frames.reshape(4, H, W).astype(np.float64)
    raw[:, 0::2, 1::2] *= 0.9
    raw = np.clip(raw, 0, 255).astype(np.uint8)
    ctx, ref = context_pair(W, H, sc.K, [MILD_DIST, MILD_DIST])
    assert check_batch(torch, ctx, ref, torch.from_numpy(raw).cuda(), 2, 3, 15) > 4 * 8


# ---- 6. the trackers ------------------------------------------------------------------------------------------------------
def test_tracker_depth3_from_raw_frames():
    """ReplayTracker / BatchTracker(depth=3, bayer_pattern=3) over several batches = the same tracker fed the oracle's gray
    frames: object points, image points and messages."""
    from mocapv2_amd.engine import GRAY_SHIFT
    from mocapv2_amd.pipeline import scene_arrays
    from mocapv2_amd.replay import ReplayTracker
    sc = Scene(3, width=640, height=360, dist=MILD_DIST)
    T = 14
    gray_scene = sc.render_batch(91, T, 5, radius_range=(14, 19), salt=0.001)  # [T, C, H, W]
    rng = np.random.default_rng(9)
    raw = gray_scene.astype(np.float64)
    raw[:, :, 0::2, 1::2] *= 0.9
    raw[:, :, 1::2, 0::2] *= 0.95
    raw = np.clip(raw + rng.integers(0, 3, raw.shape), 0, 255).astype(np.uint8)
    gray = np.stack([np.stack([oracle.bayer_gray(raw[t, c], 3, GRAY_SHIFT) for c in range(3)]) for t in range(T)])
    arrays = scene_arrays(sc)
    a = list(ReplayTracker(*arrays, 640, 360, batch=3, bayer_pattern=3, depth=3).run(raw))
    b = list(ReplayTracker(*arrays, 640, 360, batch=3, depth=3).run(gray))
    assert len(a) == len(b) == T
    for x, y in zip(a, b):
        assert np.array_equal(x["object_points"], y["object_points"]) and np.array_equal(x["image_points"], y["image_points"])
        assert x["message"] == y["message"]
    assert sum(len(x["object_points"]) > 0 for x in a) >= T - 2
