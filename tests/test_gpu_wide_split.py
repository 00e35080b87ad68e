"""A wide tile with empty mask byte columns between its markers is cut at them into box items, one set per run of marked columns
(settle_tiles_kernel, blob_settle.hip: split_at_gaps), from the column word the scan leaves beside the tile's box (scan_mark.h).

Every case runs on two contexts that differ in `wide_split` alone (1, the default: split unless a probe found the scene crowded --
with the excess base pinned no probe runs -- against 0); on both the mask of mocap_filter_mask (the caller-owned-mask entry
point) and the centroids of mocap_blob_centroids (the context's own mask, kept from batch to batch) must equal the oracle's, and after
every call the list counts of mocap_list_stats (items, wide entries, split tiles) are asserted: under the identity lens against a
restatement of the scan's and settle's rules in this file (the excess base is pinned, so which cells are hot follows from the frame
alone), under the other lenses against the context without the split (a split tile is one wide entry less and 2..4 items more) and the
number of split tiles the case is built for.  Frames are 512 x 208 (3 strips, the last 32 columns wide, x 4 chunks of 68 rows, the
last 4 rows high) and 512 x 137 (the third chunk is the one row 136).

test_inputs_give_the_intended_blobs_and_routing needs no GPU: the oracle alone finds the intended blobs in every input, and the
restated rules route every input the way its case is named for."""
import numpy as np
import pytest

import oracle
from mocapv2_amd.synth import MILD_DIST, MIXED_DISTS, ZERO_DIST
from test_gpu_box_forms import choose_split, disc, expected, make_ctx, noise

BASE, HOT = 63, 1918  # pinned excess base; a cell is hot when 2 * sum(max(0, p - 63)) > ((1024 * 307 * 25 - 1) // 1024) // 4 (abi_blob.hip: scan_bounds)
HOT_CORNER = 690      # ... > ((1024 * 307 * 9 - 1) // 1024) // 4 where it feeds windows the image border cuts in both axes (9 taps), the lowest threshold
LIMIT, MAX_PARTS = 34, 4
W, H = 512, 208


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


# ---- the scan's and settle's rules, restated for an identity lens ---------------------------------------------------------------------
def tile_boxes(gray):
    """{(chunk, strip): [y0, y1, x0, x1, column bits]} as the scan leaves them: every hot cell's rectangle (the cell + 4 pixels)"""
    Hh, Ww = gray.shape
    rows = 68 if Hh >= 128 else max((Hh + 3) // 4, 8)
    pad = np.zeros((-(-Hh // 8) * 8, Ww), np.int64)
    pad[:Hh] = np.maximum(gray.astype(np.int64) - BASE, 0)
    e2 = 2 * pad.reshape(pad.shape[0] // 8, 8, Ww // 8, 8).sum(axis=(1, 3))
    edge = np.ones_like(e2, bool)  # the cells within 4 pixels of the image border: windows the border cuts read them, their thresholds are lower
    edge[1:(Hh - 4) // 8, 1:(Ww - 4) // 8] = False
    assert not np.any(edge & (e2 > HOT_CORNER) & (e2 <= HOT)), "a cell near the image border whose threshold this restatement does not know"
    boxes = {}
    for cy, cx in np.argwhere(e2 > HOT):
        xa, xb = max(8 * cx - 4, 0), min(8 * cx + 11, Ww - 1)
        ya, yb = max(8 * cy - 4, 0), min(min(8 * cy + 7, Hh - 1) + 4, Hh - 1)
        for ch in range(ya // rows, yb // rows + 1):
            for st in range(xa // 240, xb // 240 + 1):
                b = boxes.setdefault((ch, st), [1 << 30, -1, 1 << 30, -1, 0])
                b[0], b[1], b[2], b[3] = min(b[0], ya), max(b[1], yb), min(b[2], xa), max(b[3], xb)
                ca, cb = max(xa - 240 * st, 0), min(xb - 240 * st, 239)
                b[4] |= (2 << (cb >> 3)) - (1 << (ca >> 3))
    return boxes, rows


def runs_of(cols):
    out, b = [], 0
    while cols >> b:
        if (cols >> b) & 1:
            e = b
            while (cols >> (e + 1)) & 1:
                e += 1
            out.append((b, e))
            b = e + 1
        else:
            b += 1
    return out


def list_counts(gray, wide_split, wide_list=True):
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
        marked = [k for k in range(4) if c0 + (k >> 1) < n_chunks and s0 + (k & 1) < n_strips and (c0 + (k >> 1)) * rows < Hh
                  and (c0 + (k >> 1), s0 + (k & 1)) in boxes]
        if len(marked) >= 2:
            u = [boxes[(c0 + (k >> 1), s0 + (k & 1))] for k in marked]
            uy0, uy1, ux0, ux1 = min(b[0] for b in u), max(b[1] for b in u), min(b[2] for b in u), max(b[3] for b in u)
            e = [max(ux0, 240 * s0) & ~7, min(ux1 | 7, min(240 * (s0 + 2) - 1, Ww - 1)), max(uy0, c0 * rows), min(uy1, min((c0 + 2) * rows, Hh) - 1)]
            if not (((e[1] - e[0] + 8) >> 3) > 13 or e[3] - e[2] + 1 > 100):
                cover, emits = e, marked[0] == (ch - c0) * 2 + (st - s0)
        nb, h = (cover[1] - cover[0] + 8) >> 3, cover[3] - cover[2] + 1
        nx, ny = choose_split(nb, h)
        is_wide = emits and cover == out and wide_list and 2 * nb + 2 * nx >= LIMIT
        if is_wide and wide_split:
            parts = [choose_split(b1 - b0 + 1, h) + (b1 - b0 + 1,) for b0, b1 in runs_of(cols)]
            if 2 <= len(parts) <= MAX_PARTS and all(2 * n + 2 * px < LIMIT for px, _, n in parts) and sum(px * py for px, py, _ in parts) <= MAX_PARTS:
                split += 1
                items += sum(px * py for px, py, _ in parts)
                continue
        if is_wide:
            wide += 1
        elif emits:
            items += nx * ny
    return items, wide, split


# ---- the inputs -----------------------------------------------------------------------------------------------------------------------
def frame(seed, discs=(), blocks=(), shape=(H, W)):
    """noise below the excess base, discs (cx, cy, r) and saturated blocks of whole cells (first / last cell column, first / last cell row)"""
    f = noise(np.random.default_rng(seed), 1, *shape)[0]
    for cx, cy, r in discs:
        disc(f, cx, cy, r)
    for x0, x1, y0, y1 in blocks:
        f[8 * y0:8 * y1 + 8, 8 * x0:8 * x1 + 8] = 255
    return f


BAR_A = (2, 9, 3, 3)  # cells 2..9 of cell row 3: rectangle columns 12..83, mask bytes 1..10
# name -> (batches, blobs per image of each batch, split tiles per image of each batch under the identity lens)
CASES = {
    "basic": ([[frame(1, [(40, 30, 6), (180, 34, 7)])]], [[2]], [[1]]),
    # B's rectangle begins 4 pixels left of its first cell: cell 13 -> column 100, byte 12 (byte 11 stays empty); cell 12 -> byte 11,
    # next to A's last byte; cell 11 -> column 84: the rectangles touch and share byte 10
    "gap_of_one_byte": ([[frame(2, blocks=[BAR_A, (13, 17, 3, 3)])]], [[2]], [[1]]),
    "bytes_adjacent": ([[frame(3, blocks=[BAR_A, (12, 17, 3, 3)])]], [[2]], [[0]]),
    "rectangles_touch": ([[frame(4, blocks=[BAR_A, (11, 17, 5, 5)])]], [[2]], [[0]]),
    # strip 1 = columns 240..479: a disc on its left edge and one at its right end; the mirror image, with a disc in the narrow last strip
    "left_edge": ([[frame(5, [(240, 30, 6), (466, 34, 6)])]], [[2]], [[1]]),
    "right_edge": ([[frame(6, [(480, 30, 6), (252, 34, 6), (496, 100, 7)])]], [[3]], [[1]]),
    "three_runs": ([[frame(7, [(30, 30, 6), (120, 28, 6), (210, 33, 6)])]], [[3]], [[1]]),
    "five_runs": ([[frame(8, [(24, 32, 6), (72, 32, 6), (120, 32, 6), (168, 32, 6), (216, 32, 6)])]], [[5]], [[0]]),
    "run_too_wide": ([[frame(9, [(200, 30, 6)], blocks=[(1, 15, 3, 3)])]], [[2]], [[0]]),
    "run_in_two_parts": ([[frame(10, [(200, 30, 6)], blocks=[(2, 11, 0, 7)])]], [[2]], [[1]]),
    # a bar across the later gap, the two discs, the bar again, a dark batch, the discs after the dark one
    "stale_bits": ([[frame(11, blocks=[(2, 25, 3, 3)])], [frame(12, [(40, 30, 6), (180, 34, 7)])], [frame(13, blocks=[(2, 25, 3, 3)])],
                    [frame(14)], [frame(15, [(44, 28, 6), (176, 30, 7)])], [frame(16)]], [[1], [2], [1], [0], [2], [0]], [[0], [1], [0], [0], [1], [0]]),
    # a disc on the corner four tiles share (one cluster item) and a split tile two chunks below
    "cluster": ([[frame(17, [(240, 68, 6), (40, 170, 6), (180, 172, 6)])]], [[3]], [[1]]),
    # 512 x 137: two blocks down to the last row; the tile of row 136 alone is split too
    "one_row_chunk": ([[frame(18, blocks=[(2, 3, 15, 17), (20, 21, 15, 17)], shape=(137, W))]], [[2]], [[2]]),
}


def blobs_of(f, dist=ZERO_DIST, bayer=False):
    K = make_K(f.shape)
    return expected(f[None], K, np.asarray(dist, float), bayer)[0]


def make_K(shape):
    from mocapv2_amd.synth import Scene
    return Scene(1, width=shape[1], height=shape[0]).K


def test_inputs_give_the_intended_blobs_and_routing():
    for name, (batches, blobs, splits) in CASES.items():
        for b, frames in enumerate(batches):
            for i, f in enumerate(frames):
                assert len(blobs_of(f)[1]) == blobs[b][i], (name, b, i, blobs_of(f)[1])
                on, off = list_counts(f, 1), list_counts(f, 0)
                assert on[2] == splits[b][i] and off[2] == 0, (name, b, i, on, off)
                assert on[1] + on[2] == off[1] and 2 * on[2] <= on[0] - off[0] <= MAX_PARTS * on[2], (name, b, i, on, off)
    assert list_counts(CASES["cluster"][0][0][0], 1)[0] == 1 + 2  # the cluster item, the two runs


# ---- on the GPU -----------------------------------------------------------------------------------------------------------------------
def run_case(torch, batches, dist, want_split, tuning=(), bayer=None, masks=True):
    """Both contexts over the batches; bayer: None = gray frames, "direct" = raw frames without a gray buffer, "gray" = with one.
    want_split: split tiles per batch with the split on (None: only the relation to the context without it)."""
    from gpu_util import unpack_mask
    shape = batches[0][0].shape
    identity = not np.any(dist)
    stats = {}
    for ws in (1, 0):
        ctx, K = make_ctx(shape[1], shape[0], [dist], [("wide_split", ws), ("excess_base", BASE)] + list(tuning))
        for b, frames in enumerate(batches):
            frames = np.stack(frames)
            d = torch.from_numpy(frames).cuda()
            exp = [expected(frames[i:i + 1], K, np.asarray(dist, float), bayer is not None)[0] for i in range(len(frames))]
            calls = []
            if masks and bayer is None:
                got, pad = unpack_mask(ctx.filter_mask(d), shape[1])
                assert not pad.any()
                for i in range(len(frames)):
                    assert np.array_equal(got[i], exp[i][0]), (ws, b, i, np.argwhere(got[i] != exp[i][0])[:4])
                calls.append(ctx.list_stats())
            gray = torch.empty_like(d) if bayer == "gray" else None
            xy, cnt = ctx.record_views(ctx.blob_centroids(d, bayer_pattern=None if bayer is None else 3, gray=gray))
            xy, cnt = xy.cpu().numpy(), cnt.cpu().numpy()
            for i in range(len(frames)):
                assert cnt[i] == len(exp[i][1]) and xy[i, :cnt[i]].tolist() == exp[i][1], (ws, b, i, cnt[i], xy[i, :cnt[i]].tolist(), exp[i][1])
            calls.append(ctx.list_stats())
            assert all(c == calls[0] for c in calls), calls  # the caller's mask and the context's own: the same lists
            print("wide_split", ws, "batch", b, "items, wide, split:", calls[0])
            if identity:
                from mocapv2_amd.engine import GRAY_SHIFT
                grays = [oracle.bayer_gray(f, 3, GRAY_SHIFT) if bayer is not None else f for f in frames]
                model = [list_counts(g, ws, wide_list=bayer != "direct") for g in grays]
                assert calls[0] == tuple(sum(m[k] for m in model) for k in range(3)), (ws, b, calls[0], model)
            stats[(ws, b)] = calls[0]
    for b in range(len(batches)):
        on, off = stats[(1, b)], stats[(0, b)]
        assert off[2] == 0 and on[1] + on[2] == off[1] and 2 * on[2] <= on[0] - off[0] <= MAX_PARTS * on[2], (b, on, off)
        if want_split is not None:
            assert on[2] == want_split[b], (b, on, off)
    return stats


LENSES = {"zero": ZERO_DIST, "mild": MILD_DIST, "pincushion": MIXED_DISTS[2], "tangential": MIXED_DISTS[3]}


def splits_of(name):
    return [sum(s) for s in CASES[name][2]]


@pytest.mark.gpu
@pytest.mark.parametrize("lens", ["zero", "mild"])
def test_two_discs_with_a_gap(torch_cuda, lens):
    run_case(torch_cuda, CASES["basic"][0], LENSES[lens], splits_of("basic"))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["gap_of_one_byte", "bytes_adjacent", "rectangles_touch"])
def test_gap_width(torch_cuda, name):
    """identity lens, blocks of whole saturated cells: the rectangles' columns are known to the pixel"""
    run_case(torch_cuda, CASES[name][0], ZERO_DIST, splits_of(name))


@pytest.mark.gpu
@pytest.mark.parametrize("lens", ["zero", "mild", "pincushion", "tangential"])
@pytest.mark.parametrize("name", ["left_edge", "right_edge"])
def test_markers_on_the_tile_edges(torch_cuda, name, lens):
    """a run that holds the tile's first / last byte takes its exact pixels from the box's own extent, into the neighbour's halo; under
    the strong lenses the discs move by pixels, so the number of split tiles is asserted for the identity and the mild lens only"""
    run_case(torch_cuda, CASES[name][0], LENSES[lens], splits_of(name) if lens in ("zero", "mild") else None)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["three_runs", "five_runs", "run_too_wide", "run_in_two_parts"])
def test_run_counts(torch_cuda, name):
    stats = run_case(torch_cuda, CASES[name][0], ZERO_DIST, splits_of(name))
    if name == "run_in_two_parts":
        assert choose_split(12, 68)[0] * choose_split(12, 68)[1] == 2 and stats[(1, 0)][0] == 3
    if name == "five_runs":
        assert stats[(1, 0)][1] == 1


@pytest.mark.gpu
@pytest.mark.parametrize("lens", ["zero", "mild"])
def test_stale_bits_of_the_previous_batch(torch_cuda, lens):
    """the context's own mask from batch to batch: what the bar left in the later gap is cleared (a stale piece would be a blob), and
    what the discs left is cleared under the bar's tile and by the dark batch"""
    run_case(torch_cuda, CASES["stale_bits"][0], LENSES[lens], splits_of("stale_bits"), masks=False)


@pytest.mark.gpu
@pytest.mark.parametrize("hotmap", [0, 2])
def test_marking_by_the_scan_and_by_the_hot_map(torch_cuda, hotmap):
    run_case(torch_cuda, CASES["basic"][0] + CASES["three_runs"][0], ZERO_DIST, splits_of("basic") + splits_of("three_runs"), [("scan_hotmap", hotmap)])


@pytest.mark.gpu
@pytest.mark.parametrize("path", ["gray", "direct"])
def test_bayer_frames(torch_cuda, path):
    """with a gray buffer the fused Bayer scan marks the columns (512 x 208) and the tiles are split as for gray frames; without one
    the box kernel's Bayer form takes every tile: no wide list, nothing to split, the same results"""
    stats = run_case(torch_cuda, CASES["basic"][0], ZERO_DIST, splits_of("basic") if path == "gray" else [0], bayer=path)
    if path == "direct":
        assert stats[(1, 0)] == stats[(0, 0)] and stats[(1, 0)][1] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("bayer", [None, "gray"])
def test_one_row_chunk(torch_cuda, bayer):
    """512 x 137 (height no multiple of 8: the Bayer pass and the scan are two kernels): the tile that is row 136 alone is split too"""
    run_case(torch_cuda, CASES["one_row_chunk"][0], ZERO_DIST, splits_of("one_row_chunk"), bayer=bayer)


@pytest.mark.gpu
def test_cluster_item_beside_a_split_tile(torch_cuda):
    run_case(torch_cuda, CASES["cluster"][0], ZERO_DIST, splits_of("cluster"))
