"""An oracle-free reference for the contour stage (plain Python / NumPy / SciPy / mpmath; no GPU, no C oracle, no line shared
with oracle/blob_oracle.c or the kernels).

Which borders a mask has, where they start and how they nest comes from scipy.ndimage.label alone: one outer border per
8-connected foreground component (start: its raster-first pixel), one hole border per enclosed 4-connected background region
(start: the foreground pixel left of the region's raster-first pixel).  The closed pixel chain of a border is traced from that
start and then certified, so that the trace is not taken on trust: consecutive pixels are 8-adjacent foreground, the chain's
pixel set is the morphological border set, and where no pixel repeats the polygon area obeys Pick's theorem with the pixel
counts of the labelling.  Everything measured on the chain is exact: Python ints and Fractions for the Green's-theorem sums,
one correctly rounded float32 root per diagonal run for cv.arcLength (the sum of such terms is exact in double), mpmath at 40
digits for the circularity gate and for the bound on the perimeter's distance from the true length.

The seeded masks of section 2 (`batch`) carry what the closed-form rectangles of contour_cases.py do not: diagonal runs up to
and beyond the kernel's 64-entry table of run lengths, starts that lie mid-run, hole borders, pixels visited twice, frame
contact, borders wider and taller than a walker's window."""
import functools
import math
from fractions import Fraction

import mpmath
import numpy as np
import scipy.ndimage as ndi

from contour_cases import _preorder, local_candidates

mpmath.mp.dps = 40

EIGHT = np.ones((3, 3), bool)
CROSS = ndi.generate_binary_structure(2, 1)
# the eight neighbours of a pixel as (dx, dy), counter-clockwise on the screen (y grows downwards), from East; odd = diagonal
RING = ((1, 0), (1, -1), (0, -1), (-1, -1), (-1, 0), (-1, 1), (0, 1), (1, 1))
EAST, WEST = 0, 4

MAX_BORDERS, MAX_KEPT, MAX_CANDIDATES, MAX_DEPTH = 384, 256, 1024, 8  # the kernel's documented capacities per image
MARGIN = 1e-6                                                          # circularities and centroid quotients keep this distance


# ---- 1. the reference --------------------------------------------------------------------------------------------------
def trace(fg, x0, y0, behind):
    """The closed chain of the border through (x0, y0) of the padded mask `fg`, as (pixels, moves): moves[i] is the RING index
    of the step from pixels[i] to pixels[i + 1] (cyclically).  Neighbour tracing: from each pixel the walk turns to the first
    foreground neighbour counter-clockwise after the one it came from; at the start it pretends to have come from the
    background neighbour `behind`.  It ends when it is back at the start and about to repeat its first move."""
    def turn(x, y, back):
        for k in range(1, 9):
            j = (back + k) % 8
            if fg[y + RING[j][1], x + RING[j][0]]:
                return j
        return None

    first = turn(x0, y0, behind)
    if first is None:
        return [], []
    pixels, moves = [], []
    x, y, j = x0, y0, first
    while True:
        pixels.append((x, y))
        moves.append(j)
        assert len(pixels) <= 4 * fg.size
        x, y = x + RING[j][0], y + RING[j][1]
        j = turn(x, y, (j + 4) % 8)
        if (x, y) == (x0, y0) and j == first:
            return pixels, moves


def straight_runs(moves):
    """(the maximal straight runs of the closed chain as (RING index, steps), whether position 0 lies inside a run)"""
    n = len(moves)
    if n == 0:
        return [], False
    turns = [i for i in range(n) if moves[i] != moves[i - 1]]
    assert len(turns) >= 2  # a closed chain turns
    ends = turns[1:] + [turns[0] + n]
    return [(moves[a], b - a) for a, b in zip(turns, ends)], turns[0] != 0


def measure(pixels, moves):
    """the statistics of one chain (pixel coordinates unpadded), exact"""
    n = len(pixels)
    a00 = a10 = a01 = 0
    for i in range(n):
        (x, y), (u, v) = pixels[i], pixels[(i + 1) % n]
        assert max(abs(u - x), abs(v - y)) == 1
        cross = x * v - u * y
        a00 += cross
        a10 += cross * (x + u)
        a01 += cross * (y + v)
    runs, mid_run = straight_runs(moves)
    axis = sum(k for d, k in runs if d % 2 == 0)
    diag = [k for d, k in runs if d % 2 == 1]
    assert axis + sum(diag) == n
    perimeter = float(axis) + sum(float(np.sqrt(np.float32(2 * k * k))) for k in diag)  # every term a float32 >= 1: exact in any order
    true_len = axis + mpmath.sqrt(2) * sum(diag)
    assert abs(mpmath.mpf(perimeter) - true_len) <= mpmath.mpf(2) ** -24 * mpmath.sqrt(2) * sum(diag)  # half a float32 ulp per root
    return dict(steps=n, npts=len(runs) if n else 1, a00=a00, a10=a10, a01=a01, area=abs(a00) / 2, perimeter=perimeter,
                mid_run=mid_run, long_diag=sum(1 for k in diag if k > 63), diag_runs=sorted(set(diag)),
                repeats=len(set(pixels)) != n)


def _grown(sl, by=1):
    return tuple(slice(s.start - by, s.stop + by) for s in sl)


def borders_of(mask):
    """Every border of mask != 0 as a dict: is_hole, ox, oy (the start, unpadded), parent (index into the list, -1 = the frame)
    and the gate-free statistics of `measure`.  Each chain is certified against the labelling on the way."""
    P = np.pad(np.asarray(mask) != 0, 1)
    lab_fg, n_fg = ndi.label(P, structure=EIGHT)
    lab_bg, n_bg = ndi.label(~P)  # 4-connected; the region that holds the pad is the frame
    frame = int(lab_bg[0, 0])
    box_fg, box_bg = ndi.find_objects(lab_fg), ndi.find_objects(lab_bg)

    def raster_first(lab, k, box):
        ys, xs = np.nonzero(lab[box] == k)  # row-major: the first hit is the raster-first pixel
        return int(xs[0]) + box[1].start, int(ys[0]) + box[0].start

    borders, outer_of, hole_of = [], {}, {}
    for k in range(1, n_fg + 1):
        x, y = raster_first(lab_fg, k, box_fg[k - 1])
        assert not P[y, x - 1]
        pixels, moves = trace(P, x, y, WEST)
        sl = _grown(box_fg[k - 1])
        comp = lab_fg[sl] == k
        filled = ndi.binary_fill_holes(comp)
        ring = comp & ndi.binary_dilation(~filled, structure=CROSS)
        lattice = int(filled.sum())
        outer_of[k] = len(borders)
        borders.append(dict(is_hole=0, x=x, y=y, pixels=pixels, moves=moves, ring=ring, sl=sl, pick=lambda a, s, L=lattice: a == 2 * L - s - 2))
    for j in range(1, n_bg + 1):
        if j == frame:
            continue
        hx, hy = raster_first(lab_bg, j, box_bg[j - 1])
        x, y = hx - 1, hy
        assert P[y, x]
        pixels, moves = trace(P, x, y, EAST)
        sl = _grown(box_bg[j - 1])
        hole = lab_bg[sl] == j
        # foreground 4-adjacent to the hole -- of the component that encloses it: an island inside the hole touches it too, with
        # its own outer border
        ring = (lab_fg[sl] == lab_fg[y, x]) & ndi.binary_dilation(hole, structure=CROSS)
        lattice = int(ndi.binary_fill_holes(hole, structure=EIGHT).sum())  # the hole's pixels and whatever it encloses
        hole_of[j] = len(borders)
        borders.append(dict(is_hole=1, x=x, y=y, pixels=pixels, moves=moves, ring=ring, sl=sl, pick=lambda a, s, L=lattice: a == 2 * L + s - 2))

    out = []
    for b in borders:
        x, y, pixels = b["x"], b["y"], b["pixels"]
        # certification: foreground (8-adjacency is asserted in measure), the chain's pixel set is the morphological border set
        assert all(P[v, u] for u, v in pixels)
        seen = np.zeros_like(b["ring"])
        for u, v in pixels or [(x, y)]:
            seen[v - b["sl"][0].start, u - b["sl"][1].start] = True
        assert np.array_equal(seen, b["ring"]), ("border set", b["is_hole"], x - 1, y - 1)
        rec = measure([(u - 1, v - 1) for u, v in pixels], b["moves"])
        if not rec["repeats"] and rec["steps"]:  # Pick: area = interior + boundary / 2 - 1 with the labelling's pixel counts
            assert b["pick"](abs(rec["a00"]), rec["steps"]), ("Pick", b["is_hole"], x - 1, y - 1)
        assert rec["a00"] == 0 or (rec["a00"] > 0) == bool(b["is_hole"])
        if b["is_hole"]:
            parent = outer_of[int(lab_fg[y, x])]
        else:
            region = int(lab_bg[y, x - 1])
            parent = -1 if region == frame else hole_of[region]
        out.append(dict(rec, is_hole=b["is_hole"], ox=x - 1, oy=y - 1, parent=parent))
    assert len({(b["is_hole"], b["ox"], b["oy"]) for b in out}) == len(out)
    return out


def gated(borders, min_area, min_circ):
    """The borders with the area / circularity gate and the truncated centroid applied: adds circ_margin, kept, cx, cy,
    exact_rule (the centroid quotient is an integer or within MARGIN of one: the IEEE double recipe decided), gate_tie (likewise
    for a circularity within MARGIN of min_circ; the seeded masks have none) and order (position
    among the kept in output order, None when not kept)."""
    out = []
    for b in borders:
        b = dict(b)
        a00, a10, a01 = b["a00"], b["a10"], b["a01"]
        area, per = Fraction(abs(a00), 2), Fraction(b["perimeter"])
        kept, b["circ_margin"], b["exact_rule"], b["gate_tie"], b["cx"], b["cy"] = False, None, False, False, 0, 0
        if per != 0:
            circ = 4 * mpmath.pi * mpmath.mpf(area.numerator) / area.denominator / (mpmath.mpf(per.numerator) / per.denominator) ** 2
            b["circ_margin"] = float(abs(circ - mpmath.mpf(min_circ)))
            kept = bool(circ > mpmath.mpf(min_circ)) and area > Fraction(min_area) and a00 != 0
            # the same gate as the reference's Python states it, in IEEE double (lib/ImageOperations.py:47-50): where the exact
            # circularity keeps MARGIN from min_circ the two agree; closer than that -- a tie in double -- the double recipe decides
            circ_d = 4 * math.pi * float(area) / (b["perimeter"] * b["perimeter"])
            kept_d = circ_d > min_circ and float(area) > min_area and a00 != 0
            if b["circ_margin"] >= MARGIN:
                assert kept == kept_d
            else:
                kept, b["gate_tie"] = kept_d, True
        if kept:
            # the recipe cv2 and the reference's Python run, in IEEE double
            half, sixth = (0.5, 1 / 6) if a00 > 0 else (-0.5, -(1 / 6))
            m00, m10, m01 = a00 * half, a10 * sixth, a01 * sixth
            cx, cy = int(m10 / m00), int(m01 / m00)
            for q, got in ((Fraction(a10, 3 * a00), cx), (Fraction(a01, 3 * a00), cy)):
                if abs(q - round(q)) >= Fraction(MARGIN):
                    assert int(q) == got, (q, got)  # the exact statement and the double recipe agree
                else:
                    b["exact_rule"] = True
                    assert abs(q - got) < 1 + MARGIN
            b["cx"], b["cy"] = cx, cy
        b["kept"] = 1 if kept else 0
        out.append(b)
    order = [i for i in _preorder(out) if out[i]["kept"]]
    for b in out:
        b["order"] = None
    for pos, i in enumerate(order):
        out[i]["order"] = pos
    return out


def key_of(b):
    return (b["is_hole"], b["ox"], b["oy"])


def depth_of(borders, i):
    d = 0
    while i >= 0:
        d, i = d + 1, borders[i]["parent"]
    return d


# ---- 2. the masks ------------------------------------------------------------------------------------------------------
def _grid(H, W):
    return np.mgrid[0:H, 0:W]


def salt(H, W, seed, p):
    return np.random.default_rng(seed).random((H, W)) < p


def discs_and_rings(H, W, seed, n, rmax=40.0):
    """discs and rings of random radius, some cut by the frame, some nested (the recipe of test_gpu_blob.structured_mask)"""
    rng = np.random.default_rng(seed)
    yy, xx = _grid(H, W)
    m = np.zeros((H, W), bool)
    for _ in range(n):
        cx, cy, r = rng.uniform(0, W), rng.uniform(0, H), rng.uniform(3, rmax)
        d2 = (xx - cx) ** 2 + (yy - cy) ** 2
        m |= d2 <= r * r
        if rng.random() < 0.6:
            m &= ~(d2 <= (0.7 * r) ** 2)
            if rng.random() < 0.6:
                m |= d2 <= (0.4 * r) ** 2
                if rng.random() < 0.5:
                    m &= ~(d2 <= (0.2 * r) ** 2)
    return m


def diamond(m, cx, cy, r, r_in=None):
    """the 45-degree square |x - cx| + |y - cy| <= r (side runs of r diagonal steps), without |..| <= r_in: a diamond ring
    whose hole border runs through |..| = r_in + 1 and starts one step below-left of its top vertex, mid-run"""
    yy, xx = _grid(*m.shape)
    d = np.abs(xx - cx) + np.abs(yy - cy)
    m |= d <= r
    if r_in is not None:
        m &= ~(d <= r_in)


def ragged(m, seed, cx, cy, n):
    """a blob with a ragged rim: small discs along a random walk"""
    rng = np.random.default_rng(seed)
    yy, xx = _grid(*m.shape)
    for _ in range(n):
        cx, cy, r = cx + rng.uniform(-5, 5), cy + rng.uniform(-5, 5), rng.uniform(2, 6)
        m |= (xx - cx) ** 2 + (yy - cy) ** 2 <= r * r


def rect(m, x, y, w, h):
    m[y:y + h, x:x + w] = True


def slim_rects(m, x, y):
    """rectangles 9 rows high whose circularity pi a b / (a + b)^2 (a, b = sides - 1) brackets both gates: 0.785 (1:1), 0.5027
    (4:1), 0.436 (5:1), 0.3103 (8:1), 0.2827 (9:1); one below the other from (x, y)"""
    for i, w in enumerate((9, 33, 41, 65, 73)):
        rect(m, x, y + 11 * i, w, 9)


def thin_parts(m, x, y):
    """one-pixel-wide lines and L shapes (pixels visited twice), a two-pixel diagonal pair, an isolated pixel, a plus, a T and a
    two-pixel-thick bar, within 56 x 40 pixels from (x, y)"""
    m[y + 1, x + 1:x + 20] = True                    # horizontal line
    m[y + 4:y + 22, x + 2] = True                    # vertical line
    m[y + 4, x + 6:x + 20] = True                    # L
    m[y + 4:y + 16, x + 6] = True
    m[y + 8, x + 10] = m[y + 9, x + 11] = True       # diagonal pair
    m[y + 8, x + 16] = True                          # isolated pixel
    for i in range(12):                              # diagonal and anti-diagonal lines
        m[y + 12 + i, x + 10 + i] = True
        m[y + 12 + i, x + 36 - i] = True
    m[y + 30, x + 2:x + 13] = True                   # plus
    m[y + 25:y + 36, x + 7] = True
    m[y + 2, x + 26:x + 41] = True                   # T
    m[y + 2:y + 10, x + 33] = True
    m[y + 36:y + 38, x + 20:x + 50] = True           # bar two pixels thick
    m[y + 14:y + 30, x + 44:x + 46] = True
    m[y + 28, x + 40:x + 53] = True                  # a line crossing it


def frame_contact(m):
    """shapes touching each of the four frame edges, and each corner"""
    H, W = m.shape
    yy, xx = _grid(H, W)
    rect(m, 0, 0, 5, 4)
    rect(m, W - 6, 0, 6, 3)
    rect(m, 0, H - 4, 3, 4)
    m |= (xx - (W - 1)) ** 2 + (yy - (H - 1)) ** 2 <= 7 ** 2                 # a quarter disc in the corner
    m |= (xx - W // 2) ** 2 + (yy + 2) ** 2 <= 8 ** 2                        # cut by the top edge
    m |= (xx - W // 3) ** 2 + (yy - (H + 1)) ** 2 <= 9 ** 2                  # ... the bottom edge
    m |= np.abs(xx + 1) + np.abs(yy - H // 2) <= 9                           # a diamond cut by the left edge
    m |= (np.abs(xx - W) + np.abs(yy - H // 2) <= 10) & ~(np.abs(xx - W) + np.abs(yy - H // 2) <= 6)  # a diamond ring, right edge
    m[H // 2 + 14, 0:9] = True                                               # lines running into the frame
    m[0:7, W // 4] = True


def _masks_64x48():
    H, W = 48, 64
    a = salt(H, W, 11, 0.03)
    b = np.zeros((H, W), bool)
    thin_parts(b, 3, 4)
    c = discs_and_rings(H, W, 5, 5, rmax=15.0)
    d = np.zeros((H, W), bool)
    frame_contact(d)
    e = np.zeros((H, W), bool)
    diamond(e, 20, 23, 19, 12)
    diamond(e, 20, 23, 8)
    diamond(e, 20, 23, 4, 1)
    diamond(e, 51.5, 12, 10)          # centred between two pixels: flat tips
    diamond(e, 52, 35.5, 10, 5)
    f = ~salt(H, W, 12, 0.03)         # nearly full: pinholes, and an outer border round the whole frame
    g = np.ones((H, W), bool)
    h = np.zeros((H, W), bool)
    return [a, b, c, d, e, f, g, h]


def _masks_301x200():
    H, W = 200, 301
    a = discs_and_rings(H, W, 21, 10)
    b = discs_and_rings(H, W, 22, 8)
    ragged(b, 1, 60, 50, 40)
    ragged(b, 2, 220, 140, 60)
    c = np.zeros((H, W), bool)
    diamond(c, 65, 64, 62)                 # side runs of 62: the table's last entry but one
    diamond(c, 232, 100, 65, 63)           # 65 outside; the hole border: 64, start mid-run (the closing merge passes the table's end)
    diamond(c, 232, 100, 20)
    diamond(c, 40, 165, 30, 10)
    diamond(c, 100.5, 165, 25)
    d = np.zeros((H, W), bool)
    diamond(d, 66, 66, 63)                 # 63: the table's last entry
    diamond(d, 225, 100, 64, 61)           # 64 outside (the first run beyond the table); the hole border: 62
    diamond(d, 225, 100, 40, 38)
    slim_rects(d, 5, 140)
    for i in range(70):                    # a one-pixel diagonal line: runs of 69 out and back
        d[125 + i, 100 + i] = True
    e = np.zeros((H, W), bool)
    frame_contact(e)
    thin_parts(e, 30, 30)
    yy, xx = _grid(H, W)
    e |= ((xx - 200) / 90.0) ** 2 + ((yy - 120) / 70.0) ** 2 <= 1  # wider and taller than 64, cut by two edges
    e &= ~(((xx - 210) / 40.0) ** 2 + ((yy - 110) / 33.0) ** 2 <= 1)
    ragged(e, 3, 212, 108, 30)
    return [a, b, c, d, e]


def _masks_640x360():
    H, W = 360, 640
    a = discs_and_rings(H, W, 31, 16)
    b = np.zeros((H, W), bool)
    diamond(b, 135, 135, 130)              # side runs of 130
    diamond(b, 400, 180, 130, 128)         # ... and a hole border with runs of 129, start mid-run
    diamond(b, 400, 180, 100, 35)
    diamond(b, 575, 290, 62)
    c = discs_and_rings(H, W, 32, 12)
    c[:, :300] = False
    diamond(c, 70, 70, 64)
    diamond(c, 210, 80, 65)
    diamond(c, 90, 250, 63, 40)
    diamond(c, 90, 250, 20)
    diamond(c, 220, 260, 66, 64)           # the hole border: 65
    ragged(c, 4, 222, 258, 50)
    d = salt(H, W, 33, 0.0005)
    frame_contact(d)
    thin_parts(d, 300, 40)
    slim_rects(d, 20, 60)
    for k, (x, y, n) in enumerate(((120, 200, 60), (260, 120, 90), (450, 250, 120), (560, 100, 40), (200, 300, 25))):
        ragged(d, 40 + k, x, y, n)
    return [a, b, c, d]


def hand_mask(H=12, W=12):
    """an isolated pixel, a diagonal pair, a line of 5 and a 5 x 5 square with a one-pixel hole, top-left in an H x W frame"""
    m = np.zeros((H, W), np.uint8)
    m[2, 3] = 255
    m[5, 1] = m[6, 2] = 255
    m[8, 4:9] = 255
    m[1:6, 6:11] = 255
    m[3, 8] = 0
    return m


TIE = 4 * math.pi * 16.0 / (16.0 * 16.0)  # that square's circularity as lib/ImageOperations.py:47 computes it: area 16, perimeter 16

SIZES = {"64x48": _masks_64x48, "301x200": _masks_301x200, "640x360": _masks_640x360}
GATES = {"near_0.3": (20.25, 0.3), "near_0.5": (3.25, 0.5)}  # min_area: no polygon area (a multiple of 1/2) equals it
REQUIRED_DIAG_RUNS = (62, 63, 64, 65, 130)


@functools.lru_cache(maxsize=None)
def batch(size):
    """the masks of one size as uint8 {0, 255} [n, H, W], read-only"""
    masks = np.stack([(m * np.uint8(255)).astype(np.uint8) for m in SIZES[size]()])
    w, h = (int(v) for v in size.split("x"))
    assert masks.shape[1:] == (h, w)
    masks.setflags(write=False)
    return masks


@functools.lru_cache(maxsize=None)
def _borders(size):
    return tuple(borders_of(m) for m in batch(size))


@functools.lru_cache(maxsize=None)
def reference(size, gates):
    """per mask of the size: the gated border list (computed once, shared by every test, not to be changed)"""
    return tuple(gated(bs, *GATES[gates]) for bs in _borders(size))


def summary(size, gates):
    """what the GPU test's docstring records, and the conditions of section 2 (asserted by the callers)"""
    ref = reference(size, gates)
    flat = [b for bs in ref for b in bs]
    margins = [b["circ_margin"] for b in flat if b["circ_margin"] is not None]
    return dict(borders=len(flat), holes=sum(b["is_hole"] for b in flat), kept=sum(b["kept"] for b in flat),
                mid_run=sum(b["mid_run"] for b in flat), long_diag=sum(b["long_diag"] for b in flat),
                exact_rule=sum(b["exact_rule"] for b in flat), repeats=sum(b["repeats"] for b in flat),
                min_margin=min(margins), diag_runs=sorted({k for b in flat for k in b["diag_runs"]}),
                per_image=[(len(bs), sum(b["kept"] for b in bs), local_candidates(m), max([0] + [depth_of(bs, i) for i, b in enumerate(bs) if b["kept"]]))
                           for bs, m in zip(ref, batch(size))])


def assert_conditions(size, gates):
    """the reference alone satisfies the conditions under which nothing has to be excluded from a comparison"""
    s = summary(size, gates)
    for n_borders, n_kept, n_cand, kept_depth in s["per_image"]:
        assert n_borders <= MAX_BORDERS and n_kept <= MAX_KEPT and n_cand <= MAX_CANDIDATES and kept_depth <= MAX_DEPTH, s["per_image"]
    assert s["min_margin"] >= MARGIN, s["min_margin"]
    min_area = Fraction(GATES[gates][0])
    assert all(Fraction(abs(b["a00"]), 2) != min_area for bs in reference(size, gates) for b in bs)
    return s
