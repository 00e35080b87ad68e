"""The forms of the sparse filter's work list that no other test aims at with a small frame: an item that spans 2 x 2 tiles, regions
cut into several parts side by side and one above the other, the wide-tile list with row bands (one of them without rows) and a
routing limit per slot, and the emptying of the boxes an earlier, larger batch left behind.  Everything is bit-exact against the
oracle -- the mask of mocap_filter_mask, and the centroids of mocap_blob_centroids, which go through the context's own mask and
the tiles' occupancy words -- and every case runs two batches on one context, the bright regions in other places the second time,
so that what the first batch left in the mask has to be cleared where the second does not write.  Frames are 512 x 208 at most.

Where a case depends on how settle_tiles_kernel cuts a region, the test derives the region from the frame by the scan's rule for an
identity lens (a saturated 8 x 8 cell is hot; the box = the hot cells widened by 4 pixels, scan_mark.h) and restates choose_split
(blob_settle.hip) at the default constants, and asserts that the cut is the one the case is named for."""
import numpy as np
import pytest

import oracle
from mocapv2_amd.synth import MILD_DIST, ZERO_DIST, Scene

pytestmark = pytest.mark.gpu

MIN_AREA, MIN_CIRC = 20.0, 0.01  # gates that keep bars and small discs alike
BOX_HCAP, BOX_MAX_PARTS = 1536, 4


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def choose_split(nb, h):
    """(nx, ny) of a region nb mask bytes wide and h rows high"""
    best, nx, ny = None, 1, 1
    for cx in range(1, 5):
        Q = 2 * -(-nb // cx) + 2
        if Q > 64:
            continue
        rpw, mr = 64 // Q, BOX_HCAP // Q - 8
        if mr < 1:
            continue
        cy = -(-h // mr)
        if cx * cy > BOX_MAX_PARTS:
            continue
        cost = cx * cy * ((-(-h // cy) + 8 + rpw - 1) // rpw + 8)
        if best is None or cost < best:
            best, nx, ny = cost, cx, cy
    return nx, ny


def region_of(cells_x, cells_y, W, H):
    """(mask bytes, rows) of the box of saturated cells [x0, x1] x [y0, y1] (in cells), identity lens"""
    xa, xb = max(8 * cells_x[0] - 4, 0), min(8 * cells_x[1] + 11, W - 1)
    ya, yb = max(8 * cells_y[0] - 4, 0), min(8 * cells_y[1] + 11, H - 1)
    return ((xb | 7) - (xa & ~7) + 1) // 8, yb - ya + 1


def disc(img, cx, cy, r):
    H, W = img.shape
    yy, xx = np.mgrid[0:H, 0:W]
    d = np.sqrt((xx - cx) ** 2 + (yy - cy) ** 2)
    np.maximum(img, (np.clip((r + 0.75 - d) / 1.5, 0, 1) * 255).astype(np.uint8), out=img)


def make_ctx(W, H, dists, tuning=()):
    from mocapv2_amd.engine import MocapContext
    K = Scene(1, width=W, height=H).K
    ctx = MocapContext(W, H, n_slots=len(dists))
    for s, d in enumerate(dists):
        ctx.set_undistort(s, K, d)
    ctx.set_blob_params(min_area=MIN_AREA, min_circ=MIN_CIRC)
    for name, value in tuning:
        ctx.set_tuning(name, value)
    return ctx, K


_expected = {}


def expected(frames, K, dist, bayer):
    """(mask, centroids) of the oracle per image; computed once per distinct input and shared by the cases that differ in a switch only"""
    prm = oracle.default_params(undistort=True)
    prm.min_area, prm.min_circ = MIN_AREA, MIN_CIRC
    out = []
    for f in frames:
        key = (f.tobytes(), f.shape, tuple(dist), bayer)
        if key not in _expected:
            from mocapv2_amd.engine import GRAY_SHIFT
            gray = oracle.bayer_gray(f, 3, GRAY_SHIFT) if bayer else f
            und = gray if not np.any(dist) else oracle.undistort(gray, K, dist)
            _expected[key] = (oracle.image_filter(und, 0) != 0, oracle.find_dot(gray, K, dist, params=prm))
        out.append(_expected[key])
    return out


def check(torch, ctx, K, dists, batches, bayer=False, masks=True):
    """every batch on the one context: mask (gray input, unless masks=False) and centroids equal the oracle's; returns the centroids seen"""
    from gpu_util import unpack_mask
    seen = 0
    for b, frames in enumerate(batches):
        d = torch.from_numpy(frames).cuda()
        cm = len(dists)
        exp = [expected(frames[i:i + 1], K, np.asarray(dists[i % cm], float), bayer)[0] for i in range(len(frames))]
        if masks and not bayer:
            got, pad = unpack_mask(ctx.filter_mask(d, cam_mod=cm), frames.shape[2])
            assert not pad.any()
            for i in range(len(frames)):
                assert np.array_equal(got[i], exp[i][0]), (b, i, np.argwhere(got[i] != exp[i][0])[:4])
        xy, cnt = ctx.record_views(ctx.blob_centroids(d, cam_mod=cm, bayer_pattern=3 if bayer else None))
        xy, cnt = xy.cpu().numpy(), cnt.cpu().numpy()
        for i in range(len(frames)):
            assert cnt[i] == len(exp[i][1]) and xy[i, :cnt[i]].tolist() == exp[i][1], (b, i, cnt[i], exp[i][1])
            seen += len(exp[i][1])
    return seen


def noise(rng, n, H, W):
    return rng.integers(0, 41, (n, H, W), dtype=np.uint8)


# ---- one item over 2 x 2 tiles ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lens", ["zero", "mild"])
@pytest.mark.parametrize("cluster", [1, 0])
def test_cluster_item_over_four_tiles(torch_cuda, cluster, lens):
    """320 x 136 at 68 rows per tile = 2 strips x 2 chunks (frames lower than 128 rows get lower tiles: a quarter of their height); a
    disc of radius 6 centred on the corner the four tiles share, (240, 68): with `cluster` on the four marked tiles are filtered
    by ONE item over their union, and each tile's occupancy word must still come out right for the contour stage to find that
    disc and the one below it, which lies in the lower two tiles; with `cluster` 0 they are four clipped items.  Second batch: the
    same beside a disc inside a tile, where the first batch had one inside another."""
    W, H = 320, 136
    dists = [ZERO_DIST if lens == "zero" else np.array(MILD_DIST) * 2.0]
    ctx, K = make_ctx(W, H, dists, [("cluster", cluster)])
    rng = np.random.default_rng(1)
    batches = noise(rng, 2, H, W)[:, None].repeat(2, axis=1).copy()  # [batch][image]
    for b in range(2):
        disc(batches[b, 0], 240, 68, 6)
        disc(batches[b, 0], 236, 87, 6)  # in the lower two tiles only: found through their occupancy words alone
        disc(batches[b, 1], 241.5, 66.5, 6.5)
        disc(batches[b, 1 - b], 60 + 100 * b, 30, 7)
    assert check(torch_cuda, ctx, K, dists, list(batches)) == 8


# ---- regions cut into parts ----------------------------------------------------------------------------------------------
def bars_frame(rng, H, W, x_cells, y_cells):
    """two saturated bars one cell high, on the first and the last of the cell rows y_cells, across the cell columns x_cells; discs
    of radius 6 in the gap between them, one every 20 pixels: centroids all along the region, so that a part filtered wrongly or
    left out shows in the records and not only in the mask"""
    f = noise(rng, 1, H, W)[0]
    x0, x1 = 8 * x_cells[0], 8 * x_cells[1] + 8
    for cy in (y_cells[0], y_cells[1]):
        f[8 * cy:8 * cy + 8, x0:x1] = 255
    mid = 4 * (y_cells[0] + y_cells[1]) + 4
    for cx in range(x0 + 10, x1 - 6, 20):
        disc(f, cx + rng.uniform(-1, 1), mid + rng.uniform(-1, 1), 6)
    return f


@pytest.mark.parametrize("path", ["gray", "bayer"])
@pytest.mark.parametrize("lens", ["zero", "mild"])
def test_region_cut_into_parts_side_by_side(torch_cuda, path, lens):
    """Regions as wide as a tile inside one tile, kept away from the wide-tile list (wide_quads 1000; the Bayer path has no wide
    tiles): bars over the cell columns 1..28 and the cell rows 1..6 give 30 mask bytes x 56 rows (the box is the cells + 4 pixels
    each side) in the tile of rows 0..67, cut 2 x 2; in the second batch, in the other image, the cell columns 2..27 give 28 bytes,
    cut into 4 side by side."""
    W, H = 256, 128
    assert region_of((1, 28), (1, 6), W, H) == (30, 56) and choose_split(30, 56) == (2, 2)
    assert region_of((2, 27), (1, 6), W, H) == (28, 56) and choose_split(28, 56) == (4, 1)
    dists = [ZERO_DIST if lens == "zero" else MILD_DIST]
    ctx, K = make_ctx(W, H, dists, [("wide_quads_remap", 1000), ("wide_quads_identity", 1000)])
    rng = np.random.default_rng(2)
    batches = [np.stack([bars_frame(rng, H, W, (1, 28), (1, 6)), noise(rng, 1, H, W)[0]]),
               np.stack([noise(rng, 1, H, W)[0], bars_frame(rng, H, W, (2, 27), (1, 6))])]
    assert check(torch_cuda, ctx, K, dists, batches, bayer=path == "bayer") >= 2 * 10


def test_cluster_item_cut_into_parts_one_above_the_other(torch_cuda):
    """A narrow region is cut into parts one above the other only when it is higher than a tile -- a cluster item, 7 bytes x 96 rows
    here: a column of discs between two bars over the cell columns 10..14 and the cell rows 3..13, rows 24..111 across the tile
    border at row 68; the two tiles' boxes are the same, and so is their union.  Second batch: further right and one cell higher."""
    W, H = 256, 144
    assert region_of((10, 14), (3, 13), W, H) == (7, 96) and choose_split(7, 96) == (1, 2)
    assert region_of((17, 21), (2, 12), W, H) == (7, 96)

    def frame(rng, x_cells, y_cells):
        f = noise(rng, 1, H, W)[0]
        x0, x1 = 8 * x_cells[0], 8 * x_cells[1] + 8
        for cy in (y_cells[0], y_cells[1]):
            f[8 * cy:8 * cy + 8, x0:x1] = 255
        for y in range(8 * y_cells[0] + 22, 8 * y_cells[1] - 13, 20):  # (inside the bars' cell columns: the bars set the box)
            disc(f, (x0 + x1) / 2 + rng.uniform(-6, 6), y, 6)
        return f

    dists = [ZERO_DIST]
    ctx, K = make_ctx(W, H, dists)
    rng = np.random.default_rng(3)
    batches = [np.stack([frame(rng, (10, 14), (3, 13))]), np.stack([frame(rng, (17, 21), (2, 12))])]
    assert check(torch_cuda, ctx, K, dists, batches) == 2 * 5


# ---- the wide-tile list ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("identity_limit", [34, 1000])
def test_wide_tiles_in_bands_for_two_slots(torch_cuda, identity_limit):
    """wide_bands 2 on 512 x 137: the third chunk of tiles is one row high (row 136), so a wide tile there has a band without rows,
    while the 52 rows of the tile above divide into two bands of 26.  cam_mod 2 with a remapped and an identity slot: the routing
    limit is taken per slot -- with wide_quads_identity 1000 the identity slot's regions stay with the box kernel (27 bytes x 52
    rows, cut into 3 side by side; 27 bytes x 1 row) while the remapped slot's go to the row pipeline."""
    W, H = 512, 137
    assert region_of((2, 26), (11, 16), W, H) == (27, 53)  # rows 84..136: 52 in the second chunk's tile, 1 in the third's
    assert choose_split(27, 52) == (3, 1) and choose_split(27, 1) == (1, 1) and 2 * 27 + 2 * 1 >= 34
    dists = [MILD_DIST, ZERO_DIST]
    ctx, K = make_ctx(W, H, dists, [("wide_bands", 2), ("wide_quads_identity", identity_limit)])
    rng = np.random.default_rng(4)

    def frame(x_cells):
        f = bars_frame(rng, H, W, x_cells, (11, 16))
        f[128:, 8 * x_cells[0]:8 * x_cells[1] + 8] = 255  # the lower bar down to the last row of the image, the one-row tile
        return f

    batches = [np.stack([frame((2, 26)) for _ in range(4)]),
               np.stack([frame((32, 57)) if i < 2 else noise(rng, 1, H, W)[0] for i in range(4)])]
    assert check(torch_cuda, ctx, K, dists, batches) >= 6 * 10


# ---- boxes of an earlier, larger batch ------------------------------------------------------------------------------------------
def test_smaller_batch_between_two_larger_ones(torch_cuda):
    """512 x 208 = 3 strips x 4 chunks.  6 images, then 2, then 6 on one context: the boxes the first batch's scan left for images
    2..5 in the array the third batch's scan widens have to be emptied by the second batch's settle (n_clear).  Stale boxes cost
    tiles, never exactness: so besides the results, the early-out must resolve as many tiles as on a fresh context.  (Centroids only:
    a mocap_filter_mask call in between is a batch of its own and would empty the boxes.)"""
    torch = torch_cuda
    W, H = 512, 208
    dists = [MILD_DIST]
    ctx, K = make_ctx(W, H, dists)
    rng = np.random.default_rng(5)

    def frames(n):
        f = noise(rng, n, H, W)
        for i in range(n):
            for _ in range(2):
                disc(f[i], rng.uniform(10, W - 10), rng.uniform(10, H - 10), rng.uniform(4, 9))
        return f

    first, second, third = frames(6), frames(2), frames(6)
    assert check(torch, ctx, K, dists, [first, second, third], masks=False) > 10
    fresh, _ = make_ctx(W, H, dists)
    fresh.blob_centroids(torch.from_numpy(third).cuda())
    stats = ctx.tile_stats()
    assert stats == fresh.tile_stats() and stats[1] > 0.5 * stats[0], (stats, fresh.tile_stats())
