"""Every remap route of the blob stage on the lens catalogue (tests/lens_cases.py): asymmetric, anisotropic, tangential,
strong and wrapping lenses, the compact table's edge and the product's own lens, against cv.undistort + filter + _find_dot
as restated by the oracle, bit for bit.  Each case first asserts the route mocap_undistort_info reports, so that no case
passes on a path it was not meant to test."""
import warnings

import numpy as np
import pytest

import oracle
from lens_cases import case

pytestmark = pytest.mark.gpu

ROUTE_KEYS = ("compact_table", "early_out_provable", "sparse_path")
SMALL = ["offcentre_fy125", "offcentre_fy080", "tangential", "tangential_w500", "barrel_k123", "pincushion", "int16_wrap",
         "staged_overflow"]
BIG = ["reference_2048x1536", "reference_1920x1080", "compact_1023", "compact_1024"]

# the remap variants of test_gpu_blob.test_filter_mask_remap and the wide tiles' row pipeline, each with what it needs
MODES = {
    "default": ({}, ()),                                                        # the product path of the lens's route
    "box_unstaged": ({"MOCAP_BOX_STAGE_BYTES": "0"}, ("sparse",)),
    "dense": ({"MOCAP_GENERAL_FILTER": "1"}, ()),
    "dense_staged": ({"MOCAP_GENERAL_FILTER": "1", "MOCAP_ROWS_STAGED": "1"}, ("compact", "w16")),  # default stage size
    "dense_smallstage": ({"MOCAP_GENERAL_FILTER": "1", "MOCAP_ROWS_STAGED": "1", "MOCAP_ROWS_STAGE_DW": "600"}, ("compact", "w16")),
    "dense_unstaged": ({"MOCAP_GENERAL_FILTER": "1", "MOCAP_ROWS_STAGED": "1", "MOCAP_ROWS_STAGE_DW": "0"}, ("compact", "w16")),
    "dense_gather": ({"MOCAP_GENERAL_FILTER": "1", "MOCAP_REMAP_PIPELINE": "0"}, ()),
    "dense_boxes": ({"MOCAP_SKIP_DARK": "0", "MOCAP_DENSE_BOXES": "1"}, ("compact",)),
    "wide_rows": ({"MOCAP_WIDE_QUADS": "0,0"}, ("sparse",)),
    "wide_rows_staged": ({"MOCAP_WIDE_QUADS": "0,0", "MOCAP_ROWS_STAGED": "1"}, ("sparse", "w16")),
}


def _takes(c, mode):
    """Whether the lens's route can take the mode at all (a staged form needs W % 16 == 0 and the compact table, the box
    kernel's forms the sparse path ...): the others would silently run another mode's kernel and are not generated."""
    needs, r = MODES[mode][1], c.expected_route
    return not (("sparse" in needs and not r["sparse_path"]) or ("compact" in needs and not r["compact_table"])
                or ("w16" in needs and c.W % 16))


def _cases_and_modes():
    out = []
    for name in SMALL:
        out += [(name, m) for m in MODES if _takes(case(name), m)]
    for name in BIG:  # full-size frames: the default path and two alternatives
        c = case(name)
        alt = "dense_staged" if _takes(c, "dense_staged") else "dense"
        out += [(name, "default"), (name, alt), (name, "dense_gather")]
    return out


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def lens_ctx(c, n_slots=1, lenses=None):
    from mocapv2_amd.engine import MocapContext
    ctx = MocapContext(c.W, c.H, n_slots)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)  # the lenses off the sparse path say so; their route is asserted
        for sl, l in enumerate(lenses or [c]):
            assert not ctx.set_undistort(sl, l.K, l.dist)
    return ctx


def route_of(ctx, slot=0):
    info = ctx.undistort_info(slot)
    assert not info["identity"]
    return {k: info[k] for k in ROUTE_KEYS}


def rand_frames(rng, n, H, W, bright=0.2, blobs=6):
    img = rng.integers(0, 200, (n, H, W), dtype=np.uint8)
    img[rng.random((n, H, W)) < bright] = 255
    for i in range(n):
        for _ in range(blobs):
            cx, cy, r = rng.uniform(-5, W + 5), rng.uniform(-5, H + 5), rng.uniform(3, max(4, min(H, W) / 4))
            y0, y1, x0, x1 = max(0, int(cy - r)), min(H, int(cy + r) + 2), max(0, int(cx - r)), min(W, int(cx + r) + 2)
            yy, xx = np.mgrid[y0:y1, x0:x1]
            img[i, y0:y1, x0:x1][(xx - cx) ** 2 + (yy - cy) ** 2 <= r * r] = 255
    return img


def dark_frames(rng, n, H, W, salt=0.001, noise_max=60):
    """Dark noise, salt, and small anti-aliased discs near each corner, each edge midpoint and the centre."""
    img = rng.integers(0, noise_max, (n, H, W), dtype=np.uint8)
    img[rng.random((n, H, W)) < salt] = 255
    for i in range(n):
        for fx in (0.0, 0.5, 1.0):
            for fy in (0.0, 0.5, 1.0):
                r = rng.uniform(5, 9)
                m = r + rng.uniform(1, 12)  # inset from the border
                cx, cy = m + fx * (W - 2 * m) + rng.uniform(-3, 3), m + fy * (H - 2 * m) + rng.uniform(-3, 3)
                y0, y1, x0, x1 = max(0, int(cy - r - 2)), min(H, int(cy + r + 3)), max(0, int(cx - r - 2)), min(W, int(cx + r + 3))
                yy, xx = np.mgrid[y0:y1, x0:x1]
                d = np.sqrt((xx - cx) ** 2 + (yy - cy) ** 2)
                img[i, y0:y1, x0:x1] = np.maximum(img[i, y0:y1, x0:x1], (np.clip((r + 0.75 - d) / 1.5, 0, 1) * 255).astype(np.uint8))
    return img


@pytest.mark.parametrize("name", SMALL + BIG)
def test_route_and_undistort(torch_cuda, name):
    """The route the device tables take is the one the case is meant for, and the device's cv.undistort (general table)
    equals the oracle's, pixel for pixel."""
    torch = torch_cuda
    c = case(name)
    ctx = lens_ctx(c)
    assert route_of(ctx) == c.expected_route
    frame = np.random.default_rng(c.W + c.H).integers(0, 256, (c.H, c.W), dtype=np.uint8)
    und = ctx.undistort(torch.from_numpy(frame).cuda()).cpu().numpy()
    assert np.array_equal(und, oracle.undistort(frame, c.K, c.dist))


@pytest.mark.parametrize("name,mode", _cases_and_modes())
def test_filter_mask_every_route(torch_cuda, monkeypatch, name, mode):
    """filter_mask = threshold(median(blur(cv.undistort(frame)))) != 0 under every remap mode the lens's route can take."""
    from gpu_util import unpack_mask
    torch = torch_cuda
    c = case(name)
    env = MODES[mode][0]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    ctx = lens_ctx(c)
    r = route_of(ctx)
    assert r["compact_table"] == c.expected_route["compact_table"] and r["early_out_provable"] == c.expected_route["early_out_provable"]
    if not env:
        assert r == c.expected_route
    rng = np.random.default_rng(c.W * 7 + c.H + len(mode))
    n = 2 if name in SMALL else 1
    frames = rand_frames(rng, n, c.H, c.W)
    got, pad = unpack_mask(ctx.filter_mask(torch.from_numpy(frames).cuda()), c.W)
    assert not pad.any()
    for i in range(n):
        exp = oracle.image_filter(oracle.undistort(frames[i], c.K, c.dist), 0) != 0
        assert np.array_equal(got[i], exp), (name, mode, i, np.argwhere(got[i] != exp)[:5])


@pytest.mark.parametrize("name", SMALL + BIG)
def test_centroids_dark_frames(torch_cuda, name):
    """_find_dot on dark frames with salt and small discs at the corners, edge midpoints and centre: the early-out's reach
    and weight bound under asymmetric maps.  Mask and centroids equal the oracle's; the mask is zero everywhere else."""
    from gpu_util import unpack_mask
    torch = torch_cuda
    c = case(name)
    ctx = lens_ctx(c)
    assert route_of(ctx) == c.expected_route
    ctx.set_blob_params(min_area=40.0)
    prm = oracle.default_params(undistort=True)
    prm.min_area = 40.0
    rng = np.random.default_rng(c.W + 3 * c.H)
    n = 2 if name in SMALL else 1
    frames = dark_frames(rng, n, c.H, c.W)
    d = torch.from_numpy(frames).cuda()
    xy, cnt = ctx.record_views(ctx.blob_centroids(d))
    xy, cnt = xy.cpu().numpy(), cnt.cpu().numpy()
    got, _ = unpack_mask(ctx.filter_mask(d), c.W)
    seen = 0
    for i in range(n):
        exp, m = oracle.find_dot(frames[i], c.K, c.dist, params=prm, return_mask=True)
        assert cnt[i] == len(exp) and xy[i, :cnt[i]].tolist() == exp, (name, i, cnt[i], exp)
        assert np.array_equal(got[i], m != 0), (name, i, np.argwhere(got[i] != (m != 0))[:5])
        assert (m == 0).mean() > 0.9
        seen += len(exp)
    assert seen > 0


def test_batch_of_asymmetric_lenses_through_a_strided_view(torch_cuda):
    """One batch, a different asymmetric lens per slot (cam_mod = 5), frames as a view into a wider buffer (pitch > W, base
    offset 16): every image is filtered with its own slot's tables and reach.  Mask and centroids = the oracle's."""
    from gpu_util import unpack_mask
    torch = torch_cuda
    lenses = [case(n) for n in ("offcentre_fy125", "offcentre_fy080", "tangential", "barrel_k123", "pincushion")]
    c0 = lenses[0]
    W, H, C = c0.W, c0.H, len(lenses)
    assert all((l.W, l.H) == (W, H) and l.expected_route["sparse_path"] for l in lenses)
    ctx = lens_ctx(c0, n_slots=C, lenses=lenses)
    for sl, l in enumerate(lenses):
        assert route_of(ctx, sl) == l.expected_route
    ctx.set_blob_params(min_area=40.0)
    prm = oracle.default_params(undistort=True)
    prm.min_area = 40.0
    rng = np.random.default_rng(55)
    frames = dark_frames(rng, 2 * C, H, W, salt=0.002)
    big = np.zeros((2 * C, H, W + 48), np.uint8)
    big[:, :, 16:16 + W] = frames
    big[:, :, :16] = 255  # bright bytes beside the view: never read
    big[:, :, 16 + W:] = 255
    view = torch.from_numpy(big).cuda()[:, :, 16:16 + W]
    assert view.stride(1) == W + 48 and not view.is_contiguous()
    xy, cnt = ctx.record_views(ctx.blob_centroids(view, cam_mod=C))
    xy, cnt = xy.cpu().numpy(), cnt.cpu().numpy()
    got, pad = unpack_mask(ctx.filter_mask(view, cam_mod=C), W)
    assert not pad.any()
    seen = 0
    for i in range(2 * C):
        l = lenses[i % C]
        exp, m = oracle.find_dot(frames[i], l.K, l.dist, params=prm, return_mask=True)
        assert cnt[i] == len(exp) and xy[i, :cnt[i]].tolist() == exp, (i, l.name)
        assert np.array_equal(got[i], m != 0), (i, l.name)
        seen += len(exp)
    assert seen > 0
