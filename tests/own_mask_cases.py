"""Inputs of the tests of the context's own mask (test_own_mask_host.py, test_gpu_own_mask.py): which route every tile of a frame
takes through settle_tiles_kernel (blob_settle.hip) and which region it records, restated for the identity lens with the excess base
pinned to 63; the named frames; and the sequences of calls on one context whose batch-to-batch transitions the GPU tests walk through.

The own mask is never zeroed between batches: settle clears what a tile's previous region holds where this batch will not write.
What decides that is the pair (route and region of the previous batch, route and region of this one) per tile, so the sequences are
built to meet the pairs of REQUIRED, and test_own_mask_host.py asserts on the CPU that they do.

Not a test module."""
import numpy as np

import oracle
from mocapv2_amd.synth import MILD_DIST, ZERO_DIST
from test_gpu_box_forms import choose_split
from test_gpu_tile_record import LIMIT, MAX_PARTS, frame, tile_boxes
from test_gpu_wide_split import runs_of

MILD2 = tuple(2.0 * np.array(MILD_DIST))
LENSES = {"zero": ZERO_DIST, "mild2": MILD2}
UNMARKED = (("unmarked",), None)


# ---- the routes ---------------------------------------------------------------------------------------------------------------------------
def routes(gray, wide_split=True, wide_list=True):
    """{(chunk, strip): (route, region)} of the marked tiles of one image on the sparse path.  route: ("item", nx, ny),
    ("cluster_emit", nx, ny) (the tile whose item covers the cluster), ("cluster_member",), ("wide",), ("split", runs) with runs =
    ((first byte, last byte) within the tile, ...).  region = (x0, x1, y0, y1), what the tile records in cur_box: its box clipped to
    the tile in whole mask bytes -- the whole width of the tile for a wide entry, first run to last for a split tile, and for the
    tiles of a cluster each its own clipped piece.  wide_list False: the gray-less Bayer path (items only)."""
    Hh, Ww = gray.shape
    boxes, rows = tile_boxes(gray)
    n_strips, n_chunks = (Ww + 239) // 240, 4 * -(-Hh // (4 * rows))
    out_of = {}
    for (ch, st), (y0, y1, x0, x1, cols) in boxes.items():
        tx0, tr0 = 240 * st, ch * rows
        tx1, tr1 = min(tx0 + 239, Ww - 1), min(tr0 + rows, Hh) - 1
        out = tuple(int(v) for v in (max(x0, tx0) & ~7, min(min(x1, tx1) | 7, tx1), max(y0, tr0), min(y1, tr1)))
        if out[0] <= out[1] and out[2] <= out[3]:
            out_of[(ch, st)] = out
    res = {}
    for (ch, st), out in out_of.items():
        tx0 = 240 * st
        tx1 = min(tx0 + 239, Ww - 1)
        cover, emits, cluster = out, True, False
        c0, s0 = ch & ~1, st & ~1
        block = [(c0 + (k >> 1), s0 + (k & 1)) for k in range(4)]
        # (settle counts the tiles the scan marked: a record whose clipped region comes out empty counts too)
        marked = [k for k, (c, s) in enumerate(block) if c < n_chunks and s < n_strips and c * rows < Hh and (c, s) in boxes]
        if len(marked) >= 2:
            u = [boxes[block[k]] for k in marked]
            uy0, uy1, ux0, ux1 = min(b[0] for b in u), max(b[1] for b in u), min(b[2] for b in u), max(b[3] for b in u)
            e = (max(ux0, 240 * s0) & ~7, min(ux1 | 7, min(240 * (s0 + 2) - 1, Ww - 1)), max(uy0, c0 * rows), min(uy1, min((c0 + 2) * rows, Hh) - 1))
            e = tuple(int(v) for v in e)
            if not (((e[1] - e[0] + 8) >> 3) > 13 or e[3] - e[2] + 1 > 100):
                cover, emits, cluster = e, marked[0] == (ch - c0) * 2 + (st - s0), True
        nb, h = (cover[1] - cover[0] + 8) >> 3, cover[3] - cover[2] + 1
        nx, ny = (int(v) for v in choose_split(nb, h))
        if emits and cover == out and wide_list and 2 * nb + 2 * nx >= LIMIT:
            b0, b1 = (out[0] - tx0) >> 3, (out[1] - tx0) >> 3
            runs = tuple(runs_of(boxes[(ch, st)][4] & ((2 << b1) - (1 << b0))))
            parts = [choose_split(r1 - r0 + 1, h) + (r1 - r0 + 1,) for r0, r1 in runs]
            if (wide_split and 2 <= len(parts) <= MAX_PARTS and all(2 * n + 2 * px < LIMIT for px, _, n in parts)
                    and sum(px * py for px, py, _ in parts) <= MAX_PARTS):
                res[(ch, st)] = (("split", runs), out)
            else:
                res[(ch, st)] = (("wide",), (tx0, tx1, out[2], out[3]))
        elif cluster:
            res[(ch, st)] = (("cluster_emit", nx, ny) if emits else ("cluster_member",), out)
        else:
            res[(ch, st)] = (("item", nx, ny), out)
    return res


def totals(rts):
    """(items, wide entries, split tiles) of mocap_list_stats that follow from the routes of one image"""
    items = wide = split = 0
    for route, (x0, x1, y0, y1) in rts.values():
        if route[0] in ("item", "cluster_emit"):
            items += route[1] * route[2]
        elif route[0] == "wide":
            wide += 1
        elif route[0] == "split":
            split += 1
            items += sum(int(nx * ny) for nx, ny in (choose_split(r1 - r0 + 1, y1 - y0 + 1) for r0, r1 in route[1]))
    return items, wide, split


def relation(prev, cur):
    """how this batch's region lies to the previous one's: same, inside (smaller, within it), covers, disjoint, overlap"""
    if prev is None or cur is None:
        return None
    if prev == cur:
        return "same"
    if prev[0] <= cur[0] and cur[1] <= prev[1] and prev[2] <= cur[2] and cur[3] <= prev[3]:
        return "inside"
    if cur[0] <= prev[0] and prev[1] <= cur[1] and cur[2] <= prev[2] and prev[3] <= cur[3]:
        return "covers"
    if cur[1] < prev[0] or prev[1] < cur[0] or cur[3] < prev[2] or prev[3] < cur[2]:
        return "disjoint"
    return "overlap"


# ---- the frames ---------------------------------------------------------------------------------------------------------------------------
# 512 x 208: strips 0..239, 240..479, 480..511; chunks of 68 rows (the fourth is rows 204..207).  name -> (frame, blobs the oracle finds)
SHAPE, SHAPE_251 = (208, 512), (77, 251)
_F = {
    "dark": (frame(100), 0),
    "disc": (frame(102, [(100, 30, 6)]), 1),
    "disc_small": (frame(103, [(104, 32, 3)]), 0),  # (marked, but too small to set a pixel: its item writes zeros over what `disc` left)
    "disc_else": (frame(104, [(180, 40, 6)]), 1),
    "bar": (frame(105, blocks=[(2, 25, 3, 3)]), 1),
    "two": (frame(106, [(40, 30, 6), (180, 34, 7)]), 2),
    "three": (frame(107, [(40, 30, 6), (120, 34, 6), (200, 30, 6)]), 3),
    "gap_disc": (frame(108, [(110, 30, 6)]), 1),
    "corner": (frame(109, [(240, 68, 6)]), 1),
    "corner_plus": (frame(110, [(240, 68, 6), (100, 30, 6)]), 2),
    "edge_x": (frame(111, [(240, 30, 6)]), 1),
    # a block of saturated cells whose region is cut into two items side by side: 13 mask bytes x 68 rows
    "multi": (frame(112, blocks=[(5, 15, 0, 7)]), 1),
    "hot": (np.full(SHAPE, 255, np.uint8), 1),
    # 251 x 77 (chunks of 20 rows, the last one 17; strips 0..239 and 240..250): discs at the borders
    "edges_a": (frame(113, [(2, 40, 5), (248, 40, 5), (244, 8, 4), (120, 60, 5)], shape=SHAPE_251), None),
    "edges_b": (frame(114, [(4, 5, 4), (246, 72, 4), (120, 38, 5), (237, 40, 5)], shape=SHAPE_251), None),
}
FRAMES = {k: v[0] for k, v in _F.items()}
BLOBS = {k: v[1] for k, v in _F.items() if v[1] is not None}

# what the names promise, for tile (0, 0) unless said otherwise: kind of the route and the recorded region (x0, x1, y0, y1)
NAMED_ROUTES = {
    "dark": {},
    "disc": {(0, 0): ("item", (80, 119, 20, 43))},
    "disc_small": {(0, 0): ("item", (88, 119, 20, 43))},
    "disc_else": {(0, 0): ("item", (168, 199, 28, 51))},
    "bar": {(0, 0): ("wide", (0, 239, 20, 35))},
    "two": {(0, 0): ("split", (24, 199, 20, 51))},
    "three": {(0, 0): ("split", (24, 215, 20, 43))},
    "gap_disc": {(0, 0): ("item", (96, 127, 20, 43))},
    "corner": {(0, 0): "cluster_emit", (0, 1): "cluster_member", (1, 0): "cluster_member", (1, 1): "cluster_member"},
    "corner_plus": {(0, 0): "split", (0, 1): "item", (1, 0): "item", (1, 1): "item"},
    "edge_x": {(0, 0): "cluster_emit", (0, 1): "cluster_member"},
    "multi": {(0, 0): ("item", (32, 135, 0, 67))},
}
NAMED_RUNS = {"two": ((3, 6), (20, 24)), "three": ((3, 6), (13, 16), (23, 26)), "corner_plus": ((10, 14), (28, 29))}


# ---- the sequences ------------------------------------------------------------------------------------------------------------------------
# A sequence is a list of steps on ONE context:
#   ("batch", names)          mocap_blob_centroids of the named frames: the context's own mask
#   ("bayer", names)          the same frames as raw Bayer frames without a gray buffer (the direct path: items only)
#   ("filter_mask", names)    mocap_filter_mask: a caller-owned mask, the external group of tile regions
#   ("image_filter", name)    mocap_image_filter_u8 (order 0, no undistortion): the general kernel over image 0 of the own mask
#   ("tune", name, value)     mocap_set_tuning
#   ("lens", slot, lens)      mocap_set_undistort on the live context
# lenses: the slots' lenses at the start ("run": the lens the test case is parametrised with).
def _seq(steps, lenses=("run",), switches=False, shape=SHAPE):
    return {"steps": steps, "lenses": lenses, "switches": switches, "shape": shape}


def _batches(*names):
    return [("batch", [n]) for n in names]


SEQUENCES = {
    # the same region twice (no clear, cur_box not rewritten), a smaller one inside it, a dark batch, a region elsewhere
    "unmarked_and_items": _seq(_batches("dark", "disc", "disc", "disc_small", "disc", "dark", "disc", "disc_else")),
    # wide <-> item <-> split; two -> three leaves a stale disc half in a gap and half in a run of `three`; gap_disc -> two: the
    # previous region lies inside the gap of `two` only
    "wide_item_split": _seq(_batches("bar", "disc", "bar", "two", "three", "two", "gap_disc", "two", "bar", "two", "dark"), switches=True),
    # the three member tiles clear their own clipped regions; the cluster dissolves (corner_plus) and forms again
    "cluster": _seq(_batches("corner", "disc", "corner", "corner_plus", "corner", "edge_x", "corner", "multi", "corner")),
    # skip_dark 0: the general kernel writes the whole mask (mask_dirty); back on the sparse path the mask is zeroed once
    "dense_kernel": _seq(_batches("two") + [("tune", "skip_dark", 0)] + _batches("disc_else") + [("tune", "skip_dark", 1)] + _batches("disc", "dark")),
    "all_hot": _seq(_batches("dark", "hot", "dark", "hot", "disc"), switches=True),
    # a 3-image context: the zeroing behind mocap_image_filter_u8 must leave images 1 and 2 zero as well
    "image_filter_between": _seq([("batch", ["two", "bar", "corner"]), ("image_filter", "three"), ("batch", ["disc"]), ("batch", ["dark", "two", "disc"])]),
    "lens_swap": _seq(_batches("two") + [("lens", 0, "mild2")] + _batches("disc") + [("lens", 0, "zero")] + _batches("disc_small", "dark"), lenses=("zero",)),
    # images 1 and 2 keep the first batch's mask through the second call
    "batch_sizes": _seq([("batch", ["bar", "two", "corner"]), ("batch", ["disc"]), ("batch", ["three", "disc_else", "dark"])]),
    # slot 0 identity, slot 1 remapped (their routing limits differ): the bright regions swapped between the slots
    "two_slots": _seq([("batch", ["bar", "disc", "two", "corner"]), ("batch", ["disc", "bar", "corner", "two"]), ("batch", ["dark", "two", "bar", "dark"])],
                      lenses=("zero", "mild2")),
    "filter_mask_between": _seq(_batches("two") + [("filter_mask", ["bar"])] + _batches("disc") + [("filter_mask", ["three"])] + _batches("two", "dark")),
    "bayer_direct": _seq([("batch", ["bar"]), ("bayer", ["two"]), ("batch", ["two"]), ("bayer", ["bar"]), ("batch", ["bar"]), ("bayer", ["dark"])]),
    "edges_251": _seq(_batches("edges_a", "edges_b", "edges_a"), shape=SHAPE_251),
}

# (previous kind, this batch's kind, relation of the regions or None = any) that the sequences must meet under the identity lens
REQUIRED = [
    ("unmarked", "item", None), ("item", "item", "same"), ("item", "item", "inside"), ("item", "item", "covers"), ("item", "unmarked", None),
    ("item", "item", "disjoint"),
    ("wide", "item", None), ("item", "wide", None), ("wide", "split", None), ("split", "split", "overlap"), ("split", "split", "inside"),
    ("split", "split", "covers"), ("split", "item", "inside"), ("item", "split", "covers"), ("split", "wide", None), ("split", "unmarked", None),
    ("cluster_emit", "item", None), ("cluster_member", "unmarked", None), ("item", "cluster_emit", None), ("unmarked", "cluster_member", None),
    ("cluster_emit", "split", None), ("cluster_member", "item", "same"), ("split", "cluster_emit", None), ("item", "cluster_member", "same"),
    ("cluster_emit", "cluster_emit", None), ("cluster_member", "cluster_member", None),
    ("wide", "unmarked", None), ("unmarked", "wide", None),
    ("split", "dense", None), ("dense", "item", None), ("dense", "split", None), ("dense", "unmarked", None),
]


def gray_of(name, bayer):
    from mocapv2_amd.engine import GRAY_SHIFT
    return oracle.bayer_gray(FRAMES[name], 3, GRAY_SHIFT) if bayer else FRAMES[name]


def transitions(name, wide_split=True):
    """[(step, image, (chunk, strip), previous (route, region), this batch's (route, region))] over the batches of a sequence into the own
    mask, for the images whose slot holds the identity lens ("run" = identity here).  After the general kernel wrote the mask
    (skip_dark 0, mocap_image_filter_u8) the next sparse batch zeroes all of it: the previous route of every tile is ("dense",) then.
    A batch under another lens leaves routes this restatement does not know: ("unknown",), which no pair of REQUIRED names."""
    seq = SEQUENCES[name]
    Hh, Ww = seq["shape"]
    rows = 68 if Hh >= 128 else max((Hh + 3) // 4, 8)
    tiles = [(ch, st) for ch in range(-(-Hh // rows)) for st in range((Ww + 239) // 240)]
    lens = ["zero" if l == "run" else l for l in seq["lenses"]]
    state, default, dirty, dense, out = {}, UNMARKED, False, False, []
    for s, step in enumerate(seq["steps"]):
        if step[0] == "tune" and step[1] == "skip_dark":
            dense = step[2] == 0
        elif step[0] == "lens":
            lens[step[1]] = step[2]
        elif step[0] == "image_filter":
            dirty = True
        elif step[0] in ("batch", "bayer"):
            if dirty and not dense:
                state, default, dirty = {}, (("dense",), None), False
            for i, n in enumerate(step[1]):
                if dense:
                    cur = {t: (("dense",), None) for t in tiles}
                elif lens[i % len(lens)] != "zero":
                    cur = {t: (("unknown",), None) for t in tiles}
                else:
                    cur = routes(gray_of(n, step[0] == "bayer"), wide_split, wide_list=step[0] == "batch")
                for t in tiles:
                    prev, now = state.get((i, t), default), cur.get(t, UNMARKED)
                    out.append((s, i, t, prev, now))
                    state[(i, t)] = now
            dirty = dirty or dense
    return out


def pair_of(prev, now):
    return prev[0][0], now[0][0], relation(prev[1], now[1])
