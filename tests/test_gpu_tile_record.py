"""The scan's record of a tile (kernels.h: tile_quad_bits): first and last reachable mask row and a 62-bit mask of the 4-pixel quad
columns, over the window [240 st - 4, 240 st + 243] of strip st, that some hot cell's rectangle overlaps -- written by the three
markers (the scan itself, mark_tiles_kernel behind the hot map, the fused Bayer scan), decoded by settle_tiles_kernel.

Every case asserts, on one context with the excess base pinned: the mask of mocap_filter_mask and the centroids of
mocap_blob_centroids equal the oracle's, and after every call the list counts of mocap_list_stats (items, wide entries, split tiles)
equal a restatement of the scan's and settle's rules for the identity lens that keeps every rectangle's columns to the pixel -- the
record may round them to quads and cut them at the window without changing one routing decision.

What the identity lens allows: a hot cell's rectangle is columns 8 c - 4 .. 8 c + 11 (clamped into the image), so it begins on
the second quad of a mask byte and ends on the first.  A rectangle therefore cannot end exactly at column 240 st - 1, and the gap
between two rectangles is a whole number of bytes, never one quad.  The cases nearest to those are used instead, and they are
the ones a wrong decode would trip over: a rectangle that ends at 240 st + 3 (bits 0 and 1 of tile st alone), one that begins at
240 st + 236 (bits 60 and 61 of tile st alone, beside the bits 0 and 1 it sets in tile st + 1), and a gap of two empty quads that
lie in two different bytes (no byte is empty: no split; a decode that paired quads 2 b, 2 b + 1 would see an empty byte there).

test_inputs_route_as_intended needs no GPU."""
import numpy as np
import pytest

import oracle
from mocapv2_amd.synth import ZERO_DIST
from test_gpu_box_forms import choose_split, disc, expected, make_ctx, noise
from test_gpu_wide_split import runs_of

BASE = 63  # pinned excess base: a cell is hot when 2 * sum(max(0, p - 63)) exceeds the bound of the windows it feeds (abi_blob.hip: scan_bounds)
HOT, HOT_EDGE, HOT_CORNER = (((1024 * 307 * taps - 1) // 1024) // 4 for taps in (25, 15, 9))  # all 25 taps / cut by the border in one axis / in both
LIMIT, MAX_PARTS = 34, 4


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


# ---- the scan's and settle's rules, restated for an identity lens with pixel-exact extents ----------------------------------------------
def tile_boxes(gray):
    """{(chunk, strip): [y0, y1, x0, x1, byte columns]}: the union of the hot cells' rectangles (the cell + 4 pixels) per tile they overlap"""
    Hh, Ww = gray.shape
    rows = 68 if Hh >= 128 else max((Hh + 3) // 4, 8)
    ncy, ncx = -(-Hh // 8), -(-Ww // 8)
    pad = np.zeros((8 * ncy, 8 * ncx), np.int64)
    pad[:Hh, :Ww] = np.maximum(gray.astype(np.int64) - BASE, 0)
    e2 = 2 * pad.reshape(ncy, 8, ncx, 8).sum(axis=(1, 3))
    # a cell with a pixel within 4 of the image border feeds windows the border cuts: in one axis, or (a corner cell) in both
    ye = (np.arange(ncy) == 0) | (np.arange(ncy) >= (Hh - 4) >> 3)
    xe = (np.arange(ncx) == 0) | (np.arange(ncx) >= (Ww - 4) >> 3)
    thr = np.where(ye[:, None] & xe[None, :], HOT_CORNER, np.where(ye[:, None] | xe[None, :], HOT_EDGE, HOT))
    boxes = {}
    for cy, cx in np.argwhere(e2 > thr):
        xa, xb = max(8 * cx - 4, 0), min(min(8 * cx + 7, Ww - 1) + 4, Ww - 1)
        ya, yb = max(8 * cy - 4, 0), min(min(8 * cy + 7, Hh - 1) + 4, Hh - 1)
        for ch in range(ya // rows, yb // rows + 1):
            for st in range(xa // 240, xb // 240 + 1):
                b = boxes.setdefault((ch, st), [1 << 30, -1, 1 << 30, -1, 0])
                b[0], b[1], b[2], b[3] = min(b[0], ya), max(b[1], yb), min(b[2], xa), max(b[3], xb)
                ca, cb = max(xa - 240 * st, 0), min(xb - 240 * st, 239)
                b[4] |= (2 << (cb >> 3)) - (1 << (ca >> 3))
    return boxes, rows


def list_counts(gray, wide_list=True):
    """(items, wide entries, split tiles) settle makes of one image"""
    Hh, Ww = gray.shape
    boxes, rows = tile_boxes(gray)
    n_strips, n_chunks = (Ww + 239) // 240, 4 * -(-Hh // (4 * rows))
    items = wide = split = 0
    for (ch, st), (y0, y1, x0, x1, cols) in boxes.items():
        tx0, tr0 = 240 * st, ch * rows
        tx1, tr1 = min(tx0 + 239, Ww - 1), min(tr0 + rows, Hh) - 1
        out = [max(x0, tx0) & ~7, min(min(x1, tx1) | 7, tx1), max(y0, tr0), min(y1, tr1)]
        if out[0] > out[1] or out[2] > out[3]:
            continue
        cover, emits = out, True
        c0, s0 = ch & ~1, st & ~1
        block = [(c0 + (k >> 1), s0 + (k & 1)) for k in range(4)]
        marked = [k for k, (c, s) in enumerate(block) if c < n_chunks and s < n_strips and c * rows < Hh and (c, s) in boxes]
        if len(marked) >= 2:
            u = [boxes[block[k]] for k in marked]
            uy0, uy1, ux0, ux1 = min(b[0] for b in u), max(b[1] for b in u), min(b[2] for b in u), max(b[3] for b in u)
            e = [max(ux0, 240 * s0) & ~7, min(ux1 | 7, min(240 * (s0 + 2) - 1, Ww - 1)), max(uy0, c0 * rows), min(uy1, min((c0 + 2) * rows, Hh) - 1)]
            if not (((e[1] - e[0] + 8) >> 3) > 13 or e[3] - e[2] + 1 > 100):
                cover, emits = e, marked[0] == (ch - c0) * 2 + (st - s0)
        nb, h = (cover[1] - cover[0] + 8) >> 3, cover[3] - cover[2] + 1
        nx, ny = choose_split(nb, h)
        is_wide = emits and cover == out and wide_list and 2 * nb + 2 * nx >= LIMIT
        if is_wide:
            parts = [choose_split(b1 - b0 + 1, h) + (b1 - b0 + 1,) for b0, b1 in runs_of(cols)]
            if 2 <= len(parts) <= MAX_PARTS and all(2 * n + 2 * px < LIMIT for px, _, n in parts) and sum(px * py for px, py, _ in parts) <= MAX_PARTS:
                split += 1
                items += sum(px * py for px, py, _ in parts)
            else:
                wide += 1
        elif emits:
            items += nx * ny
    return items, wide, split


def quad_bits(gray):
    """{(chunk, strip): quad mask} the records hold, as tile_quad_bits forms it: bit q = columns 240 st - 4 + 4 q .. + 3, q = 0..61 (which
    bits a case exercises, for the routing test below; the hot cells of the inner threshold only, the others lie on the image border)"""
    Hh, Ww = gray.shape
    rows = tile_boxes(gray)[1]
    ncy, ncx = -(-Hh // 8), -(-Ww // 8)
    pad = np.zeros((8 * ncy, 8 * ncx), np.int64)
    pad[:Hh, :Ww] = np.maximum(gray.astype(np.int64) - BASE, 0)
    masks = {}
    for cy, cx in np.argwhere(2 * pad.reshape(ncy, 8, ncx, 8).sum(axis=(1, 3)) > HOT):
        xa, xb = max(8 * cx - 4, 0), min(min(8 * cx + 7, Ww - 1) + 4, Ww - 1)
        ya, yb = max(8 * cy - 4, 0), min(min(8 * cy + 7, Hh - 1) + 4, Hh - 1)
        for ch in range(ya // rows, yb // rows + 1):
            for st in range(xa // 240, xb // 240 + 1):
                qa, qb = max((xa - 240 * st + 4) >> 2, 0), min((xb - 240 * st + 4) >> 2, 61)
                masks[(ch, st)] = masks.get((ch, st), 0) | ((2 << qb) - (1 << qa))
    return masks


# ---- the inputs -------------------------------------------------------------------------------------------------------------------------
def frame(seed, discs=(), blocks=(), shape=(208, 512)):
    """noise below the excess base, discs (cx, cy, r) and saturated blocks of whole cells (first / last cell column, first / last cell row)"""
    f = noise(np.random.default_rng(seed), 1, *shape)[0]
    for cx, cy, r in discs:
        disc(f, cx, cy, r)
    for x0, x1, y0, y1 in blocks:
        f[8 * y0:8 * y1 + 8, 8 * x0:8 * x1 + 8] = 255
    return f


# 512 x 208: strips 0..239, 240..479, 480..511; chunks of 68 rows (the fourth is rows 204..207).  251 x 77: strips 0..239, 240..250; chunks of 20 rows.
FRAMES = {
    # rectangles across quads 31 | 32 (columns 240 st + 120 .. 127) of strip 0 and of strip 1
    "word_seam": frame(1, [(124, 30, 6), (364, 110, 6)]),
    # a disc on the tile edge x = 240; cell column 29 alone (columns 232..239: the rectangle ends at 243, bits 0 and 1 of strip 1); cell
    # column 30 alone (240..247: the rectangle begins at 236, bits 60 and 61 of strip 0)
    "halo_quads": frame(2, [(240, 30, 6)], blocks=[(29, 29, 12, 12), (30, 30, 20, 20)]),
    "image_edges": frame(3, [(3, 100, 6), (508, 100, 6), (5, 4, 6), (506, 203, 6)]),
    "image_edges_251": frame(4, [(2, 40, 5), (248, 40, 5), (244, 8, 4), (120, 60, 5)], shape=(77, 251)),
    # strip 1 (cell column 30 = its first): rectangles columns 252..323 and 340..395 -- byte 11 of the strip is empty: split; below them
    # 252..323 and 332..395 -- two empty quads, one in byte 10 and one in byte 11: no empty byte, no split
    "gap_of_a_byte": frame(5, blocks=[(32, 39, 3, 3), (43, 48, 3, 3)]),
    "gap_of_two_quads_in_two_bytes": frame(6, blocks=[(32, 39, 3, 3), (42, 48, 3, 3)]),
    "hot_everywhere": np.full((208, 512), 255, np.uint8),
    # 2880 x 64 = 12 strips x 4 chunks of 16 rows, 2880 cells: ONE wave of mark_tiles_kernel meets all 48 tiles, 16 more than its table holds
    "tiles_48": frame(7, [(240 * s + 120, 16 * c + 8, 4) for s in range(12) for c in range(4)], shape=(64, 2880)),
}
SPLITS = {"gap_of_a_byte": 1, "gap_of_two_quads_in_two_bytes": 0}
STALE = [[frame(20, blocks=[(2, 25, 3, 3)]), frame(21, [(40, 30, 6), (180, 34, 7)]), frame(22, [(240, 68, 6)])],
         [frame(23, [(300, 120, 6)])],
         [frame(24, [(44, 28, 6), (176, 30, 7)]), frame(25), frame(26, blocks=[(32, 55, 10, 10)])]]


def test_inputs_route_as_intended():
    bit = lambda m, q: (m >> q) & 1
    m = quad_bits(FRAMES["word_seam"])
    assert bit(m[(0, 0)], 31) and bit(m[(0, 0)], 32) and bit(m[(1, 1)], 31) and bit(m[(1, 1)], 32)
    m = quad_bits(FRAMES["halo_quads"])
    assert m[(1, 1)] == 0b11 and m[(2, 0)] == 0b11 << 60 and bit(m[(2, 1)], 0) and bit(m[(0, 0)], 61) and bit(m[(0, 1)], 0)
    m = quad_bits(FRAMES["image_edges"])
    assert bit(m[(1, 0)], 1) and not bit(m[(1, 0)], 0) and bit(m[(1, 2)], 8) and not bit(m[(1, 2)], 9)  # columns 0 and 511: the decode's clamps
    assert len(tile_boxes(FRAMES["image_edges_251"])[0]) >= 4 and any(st == 1 for _, st in tile_boxes(FRAMES["image_edges_251"])[0])
    for name, n in SPLITS.items():
        assert list_counts(FRAMES[name])[2] == n and list_counts(FRAMES[name])[1] == 1 - n, (name, list_counts(FRAMES[name]))
    assert len(tile_boxes(FRAMES["tiles_48"])[0]) == 48
    # the tiles of the two whole strips are wide entries; of the 32 columns of the last strip the upper two chunks are an item each (136
    # rows are too many for a cluster item) and the lower two are one cluster item
    assert list_counts(FRAMES["hot_everywhere"]) == (3, 8, 0)


# ---- on the GPU -------------------------------------------------------------------------------------------------------------------------
def run_batch(torch, ctx, K, frames, bayer=False, masks=True):
    """one batch on `ctx`: the mask (gray frames) and the centroids equal the oracle's, the list counts the restated rules'; returns the counts"""
    from gpu_util import unpack_mask
    from mocapv2_amd.engine import GRAY_SHIFT
    frames = np.stack(frames)
    d = torch.from_numpy(frames).cuda()
    exp = [expected(frames[i:i + 1], K, np.asarray(ZERO_DIST, float), bayer)[0] for i in range(len(frames))]
    calls = []
    if masks and not bayer:
        got, pad = unpack_mask(ctx.filter_mask(d), frames.shape[2])
        assert not pad.any()
        for i in range(len(frames)):
            assert np.array_equal(got[i], exp[i][0]), (i, np.argwhere(got[i] != exp[i][0])[:4])
        calls.append(ctx.list_stats())
    xy, cnt = ctx.record_views(ctx.blob_centroids(d, bayer_pattern=3 if bayer else None, gray=torch.empty_like(d) if bayer else None))
    xy, cnt = xy.cpu().numpy(), cnt.cpu().numpy()
    for i in range(len(frames)):
        assert cnt[i] == len(exp[i][1]) and xy[i, :cnt[i]].tolist() == exp[i][1], (i, cnt[i], xy[i, :cnt[i]].tolist(), exp[i][1])
    calls.append(ctx.list_stats())
    model = [list_counts(oracle.bayer_gray(f, 3, GRAY_SHIFT) if bayer else f) for f in frames]
    want = tuple(sum(m[k] for m in model) for k in range(3))
    print("items, wide, split:", calls, "restated:", want)
    assert all(c == want for c in calls), (calls, want, model)
    return want


def context(shape, tuning=()):
    return make_ctx(shape[1], shape[0], [ZERO_DIST], [("excess_base", BASE)] + list(tuning))


@pytest.mark.gpu
@pytest.mark.parametrize("hotmap", [0, 2])
@pytest.mark.parametrize("name", ["word_seam", "halo_quads", "image_edges", "image_edges_251", "gap_of_a_byte", "gap_of_two_quads_in_two_bytes",
                                  "hot_everywhere", "tiles_48"])
def test_record_through_the_scan_and_the_hot_map(torch_cuda, name, hotmap):
    """scan_hotmap 0: the scan marks the tiles itself (widen_tile_boxes); 2: mark_tiles_kernel does, through its table in LDS"""
    f = FRAMES[name]
    ctx, K = context(f.shape, [("scan_hotmap", hotmap)])
    got = run_batch(torch_cuda, ctx, K, [f])
    if name in SPLITS:
        assert got[2] == SPLITS[name] and got[1] == 1 - SPLITS[name], got


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["word_seam", "halo_quads", "image_edges", "gap_of_a_byte", "gap_of_two_quads_in_two_bytes", "hot_everywhere"])
def test_record_through_the_fused_bayer_scan(torch_cuda, name):
    """the frames as raw Bayer frames with a gray buffer (512 x 208: the fused pass marks the tiles); the rules are restated on the gray frame"""
    f = FRAMES[name]
    ctx, K = context(f.shape)
    run_batch(torch_cuda, ctx, K, [f], bayer=True)


@pytest.mark.gpu
@pytest.mark.parametrize("hotmap", [0, 2])
def test_no_stale_bits_in_either_array(torch_cuda, hotmap):
    """3 images, 1 image, 3 other images on one context (its own mask: the two record arrays alternate, and the second call leaves two
    images' records of the first in one of them -- BoxArgs::n_clear): stale quads or rows would change no result, only the lists, so after
    each call the counts equal the restated rules' -- which is what a fresh context makes of the same frames, asserted too"""
    ctx, K = context(STALE[0][0].shape, [("scan_hotmap", hotmap)])
    for frames in STALE:
        got = run_batch(torch_cuda, ctx, K, frames, masks=False)
        fresh, _ = context(frames[0].shape, [("scan_hotmap", hotmap)])
        assert run_batch(torch_cuda, fresh, K, frames, masks=False) == got
