"""Constructed masks whose contour tables follow from the construction (plain NumPy, no GPU, no oracle).

Each builder returns (mask uint8 {0,255}, case).  `case` is a dict:
  gates       (min_area, min_circ) the case is meant for
  borders     every border cv.findContours(RETR_TREE, CHAIN_APPROX_SIMPLE) lists, as dicts with is_hole, ox, oy (the start
              pixel: the border's raster-first pixel; for a hole border the foreground pixel left of the hole's first
              pixel), parent (index into this list, -1 = the frame) and -- where the shape is a rectangle -- npts, steps,
              a00, area, perimeter, kept, cx, cy as lib/ImageOperations.py:41-65 would compute them
  kept_xy     the centroids in output order: pre-order over the tree, siblings in reverse raster order of their starts
  candidates  number of pixels that satisfy the local start conditions (what local_candidates counts)

The measurements of a rectangle of w x h pixels: its outer border is the polygon through the corner pixels' centres,
(w-1) x (h-1); the hole border round a w x h hole of background runs through the foreground pixels 4-adjacent to the hole,
an octagon of (w+1) x (h+1) with its four corners cut by one diagonal step.  cv.arcLength adds float32 segment lengths."""
import math

import numpy as np

SQRT2_F32 = float(np.sqrt(np.float32(2.0), dtype=np.float32))


def _select(rec, gates):
    """the area / circularity gate and the truncated centroid (cx, cy given as exact centres by the caller)"""
    min_area, min_circ = gates
    area, per = rec["area"], rec["perimeter"]
    kept = per != 0 and 4 * math.pi * area / (per * per) > min_circ and area > min_area
    rec["kept"] = 1 if kept else 0
    rec["cx"], rec["cy"] = (int(rec["cx"]), int(rec["cy"])) if kept else (0, 0)
    return rec


def outer_rect(x, y, w, h, parent, gates):
    a = (w - 1) * (h - 1)
    return _select(dict(is_hole=0, ox=x, oy=y, parent=parent, npts=4, steps=2 * (w - 1) + 2 * (h - 1), a00=-2 * a,
                        area=float(a), perimeter=float(2 * (w - 1) + 2 * (h - 1)), cx=x + (w - 1) / 2, cy=y + (h - 1) / 2), gates)


def hole_rect(hx, hy, w, h, parent, gates):
    """the border round the w x h background rectangle whose top-left pixel is (hx, hy)"""
    a = (w + 1) * (h + 1) - 2
    straight = 2 * (w - 1) + 2 * (h - 1)
    return _select(dict(is_hole=1, ox=hx - 1, oy=hy, parent=parent, npts=8, steps=straight + 4, a00=2 * a, area=float(a),
                        perimeter=straight + 4 * SQRT2_F32, cx=hx + (w - 1) / 2, cy=hy + (h - 1) / 2), gates)


def _preorder(borders):
    """the borders' indices in tree pre-order, siblings in reverse raster order of their start pixels"""
    kids = {}
    for i, b in enumerate(borders):
        kids.setdefault(b["parent"], []).append(i)
    order, stack = [], [-1]
    while stack:
        i = stack.pop()
        if i >= 0:
            order.append(i)
        # the last pushed is visited first: push in raster order so that the raster-last sibling comes first
        stack.extend(sorted(kids.get(i, []), key=lambda j: (borders[j]["oy"], borders[j]["ox"])))
    return order


def _kept_xy(borders):
    return [[borders[i]["cx"], borders[i]["cy"]] for i in _preorder(borders) if borders[i]["kept"]]


def _case(mask, borders, gates, candidates):
    return (mask * np.uint8(255)).astype(np.uint8), dict(gates=gates, borders=borders, kept_xy=_kept_xy(borders), candidates=candidates)


GRID, BIG, SMALL = 12, 9, 3


def squares(n_big, n_small, H=192, W=384, gates=(20.0, 0.3)):
    """n_big 9 x 9 and n_small 3 x 3 squares on a 12-pixel grid, alternating while both kinds last.  Area (s-1)^2, perimeter
    4 (s-1), circularity pi / 4: the big ones pass min_area = 20, the small ones do not."""
    cols, rows = W // GRID, H // GRID
    assert n_big + n_small <= cols * rows
    kinds, b, s = [], n_big, n_small
    while b or s:
        if b:
            kinds.append(BIG)
            b -= 1
        if s:
            kinds.append(SMALL)
            s -= 1
    mask = np.zeros((H, W), bool)
    borders = []
    for i, side in enumerate(kinds):
        x, y = GRID * (i % cols) + 1, GRID * (i // cols) + 1
        mask[y:y + side, x:x + side] = True
        borders.append(outer_rect(x, y, side, side, -1, gates))
    return _case(mask, borders, gates, len(kinds))


def rings(levels, dot, gates=(20.0, 0.3)):
    """`levels` concentric square rings, walls 2 px thick, 2 px apart, and a dot x dot square (dot = 0: none) in the middle.
    Border 2k is ring k's outer border, 2k + 1 its hole border; each one's parent is the one before it."""
    side0 = 8 * levels + 8  # the innermost hole is 12 x 12
    x0, y0 = 5, 3
    mask = np.zeros((side0 + 7, side0 + 12), bool)
    borders = []
    for k in range(levels):
        x, y, side = x0 + 4 * k, y0 + 4 * k, side0 - 8 * k
        mask[y:y + side, x:x + side] = True
        mask[y + 2:y + side - 2, x + 2:x + side - 2] = False
        borders.append(outer_rect(x, y, side, side, len(borders) - 1, gates))
        borders.append(hole_rect(x + 2, y + 2, side - 4, side - 4, len(borders) - 1, gates))
    if dot:
        x, y = x0 + 4 * levels, y0 + 4 * levels
        mask[y:y + dot, x:x + dot] = True
        borders.append(outer_rect(x, y, dot, dot, len(borders) - 1, gates))
    return _case(mask, borders, gates, len(borders))


TEETH = 93


def combs(n_teeth, gates=(20.0, 0.3)):
    """Combs of up to 93 teeth below one another: a spine 3 rows thick and 185 columns long, on it teeth one pixel wide and
    two rows high on every second column.  Every tooth top has background W, NW, N and NE of it -- a local outer start --
    and no pixel of the row above near it; no background pixel has foreground both W and N of it.  One border per comb
    (started at its first tooth), far too thin to pass min_circ."""
    n_combs = (n_teeth + TEETH - 1) // TEETH
    x0 = 4
    mask = np.zeros((8 * n_combs + 4, 200), bool)
    borders = []
    for i in range(n_combs):
        y, teeth = 3 + 8 * i, min(TEETH, n_teeth - TEETH * i)
        mask[y + 2:y + 5, x0:x0 + 2 * TEETH - 1] = True
        mask[y:y + 2, x0:x0 + 2 * teeth:2] = True
        borders.append(dict(is_hole=0, ox=x0, oy=y, parent=-1, kept=0, cx=0, cy=0))
    return _case(mask, borders, gates, n_teeth)


def ring_column(n, gates=(1.0, 0.05)):
    """One ring 40 columns wide round a column of n 3 x 3 squares.  Scanning left from a square's start ends on the ring's
    inner wall, a pixel inside the bounding boxes of both of the ring's borders: which of the two owns it only a walk tells.
    Every square's parent is the ring's hole border; the ring's own two borders follow from the boxes."""
    Hn = 4 * n + 11
    mask = np.zeros((Hn, 40), bool)
    w, h = 36, 4 * n + 7
    mask[2:2 + h, 2:2 + w] = True
    mask[4:h, 4:w] = False
    borders = [outer_rect(2, 2, w, h, -1, gates), hole_rect(4, 4, w - 4, h - 4, 0, gates)]
    for i in range(n):
        y = 6 + 4 * i
        mask[y:y + 3, 18:21] = True
        borders.append(outer_rect(18, y, 3, 3, 1, gates))
    return _case(mask, borders, gates, n + 2)


def local_candidates(mask):
    """pixels that satisfy the local start conditions: set with W, NW, N, NE clear (outer), clear with W and N set (hole)"""
    m = np.pad(np.asarray(mask) != 0, 1)
    c, w, nw, n, ne = m[1:-1, 1:-1], m[1:-1, :-2], m[:-2, :-2], m[:-2, 1:-1], m[:-2, 2:]
    return int((c & ~w & ~nw & ~n & ~ne).sum() + (~c & w & n).sum())


# ---- one form for a closed-form case, the oracle's table and the kernel's records, so that any two can be compared ----
FIELDS = ("npts", "steps", "a00", "area", "perimeter", "kept", "cx", "cy")


def _start(b):
    return (b["is_hole"], b["ox"], b["oy"])


def normal_form(borders, parent_of, order_of=None):
    """{(is_hole, ox, oy): dict(parent=<start of the parent or None>, order=<position among the kept or None>, fields...)}"""
    out = {}
    kept_seen = 0
    for i, b in enumerate(borders):
        p = parent_of(i, b)
        d = {f: b[f] for f in FIELDS if f in b}
        d["parent"] = None if p < 0 else _start(borders[p])
        if order_of is not None:
            d["order"] = order_of(b) if b["kept"] else None
        else:  # the list is in output order
            d["order"] = kept_seen if b["kept"] else None
            kept_seen += 1 if b["kept"] else 0
        out[_start(b)] = d
    assert len(out) == len(borders)
    return out


def form_of_oracle(table):
    return normal_form(table, lambda i, c: c["parent_order"])


def form_of_records(recs):
    """the kernel's debug records (MocapContext.contours_from_mask with debug_cap)"""
    bs = [dict(r, ox=r["sx"], oy=r["sy"]) for r in recs]
    return normal_form(bs, lambda i, r: r["parent"], lambda r: r["order"])


def form_of_case(case):
    bs = case["borders"]
    pos = {_start(bs[i]): k for k, i in enumerate(i for i in _preorder(bs) if bs[i]["kept"])}
    return normal_form(bs, lambda i, b: b["parent"], lambda b: pos[_start(b)])


def assert_matches_case(case, got):
    """`got` (form_of_oracle / form_of_records) holds exactly the case's borders, with the case's parents, kept order and
    every measurement the case states"""
    exp = form_of_case(case)
    assert set(got) == set(exp), (sorted(set(got) ^ set(exp))[:6], len(got), len(exp))
    for key, e in exp.items():
        g = got[key]
        for f, v in e.items():
            assert g[f] == v, (key, f, g[f], v)
