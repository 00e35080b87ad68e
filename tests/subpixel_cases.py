"""Hand-made frames and records for the sub-pixel centroid tests: full lists of 256 blobs, neighbours that only one lane of one trip
of the neighbour search can find, starts outside the frame, a lens slot's whole frame.  test_subpixel_host asserts from the
restatement (tests/subpixel_ref.py) that each holds what it is meant to hold; test_gpu_subpixel runs them on the device.  Not a test
module."""
import numpy as np

import subpixel_ref as ref
from lens_cases import case

FLOOR = 10
GRID = 16                    # blobs per side: 256, the most an image's record is refined for
W1, H1, PITCH1 = 203, 200, 12  # the dense frame (odd width)
W2, H2, PITCH2, RADIUS2 = 395, 392, 24, 9  # the sparse frame: no blob within another's window of radius 9 ...
PAIRS = ((0, 255), (3, 64), (70, 128))   # ... but these record rows, 8 px apart
PAIR_CELLS = ((2, 2), (7, 5), (4, 11))   # the grid cell (gx, gy) of each pair's first row; the second comes from the cell to its right
W3, H3 = 93, 67              # the frame of the starts outside the image
LENS_W, LENS_H, LENS_RADIUS = 640, 360, 9


def pyramid(img, cx, cy, half=2, peak=250, step=40):
    H, W = img.shape
    for y in range(max(cy - half, 0), min(cy + half, H - 1) + 1):
        for x in range(max(cx - half, 0), min(cx + half, W - 1) + 1):
            img[y, x] = max(int(img[y, x]), peak - step * max(abs(x - cx), abs(y - cy)))


def records_of(point_lists, counts=None, cap=8):
    """int32 records [n, 2 + 2 cap] as blob_centroids writes them; counts overrides the lists' lengths"""
    rec = np.zeros((len(point_lists), 2 + 2 * cap), np.int32)
    for i, pts in enumerate(point_lists):
        rec[i, 0] = len(pts) if counts is None else counts[i]
        for j, (x, y) in enumerate(pts):
            rec[i, 2 + 2 * j], rec[i, 3 + 2 * j] = x, y
    return rec


def noise(H, W, seed):
    """a little noise under every floor used, as in test_gpu_subpixel.hand_made"""
    return np.random.default_rng(seed).integers(0, 9, (H, W), dtype=np.uint8)


def dense_frame():
    """(frame [200, 203], centres [256, 2], pts [256, 2]): a 16 x 16 grid of pyramids of half 2 at pitch 12; the integer centroid
    handed in is the blob's centre moved by -1, 0 or +1 px in x; the rows stand in a seeded permutation"""
    rng = np.random.default_rng(31)
    frame = noise(H1, W1, 32)
    centres = np.array([(10 + PITCH1 * gx, 10 + PITCH1 * gy) for gy in range(GRID) for gx in range(GRID)])[rng.permutation(GRID * GRID)]
    for cx, cy in centres:
        pyramid(frame, cx, cy)
    pts = centres.copy()
    pts[:, 0] += rng.integers(-1, 2, len(pts))
    return frame, centres, pts


def sparse_frame():
    """(frame [392, 395], pts [256, 2]): the grid at pitch 24, the centroids on the blobs' centres, and the second blob of each of
    PAIRS moved to 8 px right of the first.  The rows of a pair are as PAIRS says; all others in a seeded permutation."""
    rng = np.random.default_rng(33)
    cells = [(gx, gy) for gy in range(GRID) for gx in range(GRID)]
    taken = {}
    for (a, b), (gx, gy) in zip(PAIRS, PAIR_CELLS):
        taken[a], taken[b] = (gx, gy), (gx + 1, gy)
    free_cells = [c for c in cells if c not in taken.values()]
    free_rows = [r for r in range(GRID * GRID) if r not in taken]
    for r, k in zip(free_rows, rng.permutation(len(free_cells))):
        taken[r] = free_cells[k]
    pts = np.array([(12 + PITCH2 * taken[r][0], 12 + PITCH2 * taken[r][1]) for r in range(GRID * GRID)])
    for a, b in PAIRS:
        pts[b, 0] = pts[a, 0] + 8
    frame = noise(H2, W2, 34)
    for cx, cy in pts:
        pyramid(frame, cx, cy)
    return frame, pts


# beyond each border, beyond a corner, the ends of the int32 range; then each border once more
OUTSIDE = [(-3, 30), (W3 + 2, 20), (40, -1), (50, H3 + 5), (-7, H3 + 9), (2 ** 31 - 1, -2 ** 31), (-3, 52), (W3 + 2, 50), (70, -1), (20, H3 + 5)]
OUTSIDE_CLAMPED = [(0, 30), (W3 - 1, 20), (40, 0), (50, H3 - 1), (0, H3 - 1), (W3 - 1, 0), (0, 52), (W3 - 1, 50), (70, 0), (20, H3 - 1)]
OUTSIDE_LIT = (0, 1, 2, 3, 4)  # the clamped positions that hold a blob; the windows of the others are empty
# (radius, iters): at radius 2 no window around an unclamped start would reach its blob, and with one window the start shows in
# the sums themselves; at radius 6 the window follows the blob for three rounds
OUTSIDE_WINDOWS = ((6, 3), (2, 3), (2, 1))


def outside_frame():
    """(frame [67, 93], pts [10, 2]): integer centroids beyond the frame, blobs at some of the pixels they are clamped to"""
    frame = noise(H3, W3, 35)
    for k in OUTSIDE_LIT:
        pyramid(frame, *OUTSIDE_CLAMPED[k], half=3, step=30)
    return frame, np.array(OUTSIDE, np.int64)


def lens_frame():
    """(frame [360, 640], pts [256, 2], start pixels [256, 2], clamped [256] bool, lens): barrel_k123, integer centroids on a
    16 x 16 grid that reaches the corners of the undistorted image, rows permuted, a blob at the start pixel of every other row"""
    c = case("barrel_k123")
    assert (c.W, c.H) == (LENS_W, LENS_H)
    rng = np.random.default_rng(36)
    xs, ys = np.round(np.arange(GRID) * (LENS_W - 1) / (GRID - 1)), np.round(np.arange(GRID) * (LENS_H - 1) / (GRID - 1))
    pts = np.array([(x, y) for y in ys for x in xs], np.int64)[rng.permutation(GRID * GRID)]
    uv = np.array([ref.distort_pt(c.K, c.dist, x, y) for x, y in pts])
    start = np.array([(ref._start_index(u, LENS_W), ref._start_index(v, LENS_H)) for u, v in uv])
    clamped = (np.floor(uv + 0.5) != start).any(axis=1)
    frame = noise(LENS_H, LENS_W, 37)
    for cx, cy in start[::2]:
        pyramid(frame, int(cx), int(cy))
    return frame, pts, start, clamped, (c.K, c.dist, False)
