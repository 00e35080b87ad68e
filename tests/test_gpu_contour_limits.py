"""The contour stage's capacity limits at their edges (csrc/contours_dev.h: MAXC 1024 start candidates, MAXR 384 borders,
MAXK 256 kept contours, MAXD 8 nesting levels, MAXA 64 deferred links): at the limit the result is the reference's, one
past it the image carries that limit's MOCAP_BLOB_E_* code and nothing else of the batch changes.  The masks are the
constructions of tests/contour_cases.py (tests/test_contour_cases_host.py pins them against the oracle without a GPU);
every result is checked against the oracle's table and against the construction's closed form, in the three forms the
library ships: the split kernels with links walked in place (the default), with links deferred to the second passes, and
the one-kernel-per-image form.  Through the C-ABI (mocap_contours_from_mask)."""
import functools

import numpy as np
import pytest

import oracle
from contour_cases import assert_matches_case, combs, form_of_records, local_candidates, ring_column, rings, squares

pytestmark = pytest.mark.gpu

FORMS = {"links_in_place": {}, "links_deferred": {"contour_defer": 2}, "one_kernel": {"contours_split": 0}}
SENTINEL = -777

BUILDERS = {
    "squares_256_128": lambda: squares(256, 128),   # MAXR borders, MAXK kept
    "squares_256_0": lambda: squares(256, 0),
    "squares_5_3": lambda: squares(5, 3),
    "rings_4": lambda: rings(4, 0),                 # a kept border at depth MAXD
    "rings_4_dot3": lambda: rings(4, 3),            # a border at depth 9 that is not kept: no error, count 8
    "rings_2_dot3": lambda: rings(2, 3),
    "rings_2_dot7": lambda: rings(2, 7),
    "combs_1024": lambda: combs(1024),              # MAXC candidates (12 borders)
    "combs_100": lambda: combs(100),
    "ring_column_64": lambda: ring_column(64),      # MAXA links that only a walk settles
    "ring_column_65": lambda: ring_column(65),      # ... one and six more: the overflow is walked in place
    "ring_column_70": lambda: ring_column(70),
    "squares_256_129": lambda: squares(256, 129),   # 385 borders
    "squares_257_127": lambda: squares(257, 127),   # 257 kept
    "rings_4_dot7": lambda: rings(4, 7),            # a kept border at depth 9
    "combs_1025": lambda: combs(1025),              # 1025 candidates
}
AT_LIMIT = ["squares_256_128", "rings_4", "rings_4_dot3", "combs_1024", "ring_column_64", "ring_column_65", "ring_column_70"]
OVER_LIMIT = {"squares_256_129": -3, "squares_257_127": -3, "rings_4_dot7": -5, "combs_1025": -2}
# per over-limit case: two good images and an at-limit one for the same batch (embedded top-left into the offender's frame)
NEIGHBOURS = {"squares_256_129": ("squares_5_3", "rings_2_dot3", "squares_256_128"),
              "squares_257_127": ("rings_2_dot7", "squares_5_3", "squares_256_128"),
              "rings_4_dot7": ("rings_2_dot7", "rings_2_dot3", "rings_4"),
              "combs_1025": ("combs_100", "rings_2_dot7", "combs_1024")}


@functools.lru_cache(maxsize=None)
def built(name, H=None, W=None, gates=None):
    """(mask, case, the oracle's table): built once per name; H, W: the mask embedded top-left in a larger frame (no
    coordinate changes); gates: the oracle's table for another batch's gates (the case's closed form then does not apply)"""
    mask, case = BUILDERS[name]()
    if H is not None:
        big = np.zeros((H, W), np.uint8)
        big[:mask.shape[0], :mask.shape[1]] = mask
        mask = big
    g = gates or case["gates"]
    table = oracle.find_contours(mask, min_area=g[0], min_circ=g[1])
    mask.setflags(write=False)
    return mask, (case if gates is None else None), table


def run(masks, gates, form, max_blobs=256, xy_rows=None, tuning=None):
    """the batch through mocap_contours_from_mask -> xy [n, rows, 2] (pre-filled with SENTINEL), count [n], records"""
    import torch
    from gpu_util import pack_mask
    from mocapv2_amd.engine import MocapContext
    assert torch.cuda.is_available(), "these tests need the MI355X"
    H, W = masks[0].shape
    ctx = MocapContext(W, H)
    ctx.set_blob_params(min_area=gates[0], min_circ=gates[1])
    for k, v in {**FORMS[form], **(tuning or {})}.items():
        ctx.set_tuning(k, v)
    xy = torch.full((len(masks), xy_rows or max_blobs, 2), SENTINEL, dtype=torch.int32, device="cuda")
    xy, cnt, recs = ctx.contours_from_mask(pack_mask(np.stack(masks)), max_blobs=max_blobs, debug_cap=384, xy=xy)
    return xy.cpu().numpy(), cnt.cpu().numpy(), recs


def canon(recs):
    """the records without what depends on the order the walks happened to finish in (slot numbers): parents and links by
    their start pixels, sorted by discovery key"""
    def start(j):
        return None if j < 0 else (recs[j]["key"], recs[j]["is_hole"])
    return sorted(tuple(r[f] for f in ("key", "is_hole", "sx", "sy", "npts", "steps", "a00", "a10", "a01", "area", "perimeter",
                                       "kept", "cx", "cy", "order")) + (start(r["parent"]),) for r in recs)


def check_image(mask, case, table, gates, xy, count, recs, max_blobs):
    from gpu_util import check_against_oracle
    check_against_oracle(mask, recs, xy, count, gates[0], gates[1], max_blobs, table=table)
    if case is not None:
        assert_matches_case(case, form_of_records(recs))
        assert count == len(case["kept_xy"])
        assert xy[:min(count, max_blobs)].tolist() == case["kept_xy"][:max_blobs]
    assert (xy[min(count, max_blobs):] == SENTINEL).all()  # nothing is written beyond the centroids


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", AT_LIMIT)
def test_at_the_limit_the_result_is_the_references(name, form):
    mask, case, table = built(name)
    xy, cnt, recs = run([mask], case["gates"], form)
    assert cnt[0] >= 0, (name, form, cnt[0])
    check_image(mask, case, table, case["gates"], xy[0], cnt[0], recs[0], 256)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", OVER_LIMIT)
def test_one_past_the_limit_is_that_limits_code(name, form):
    """... and the over-limit image's neighbours in the batch [good, over-limit, good, at-limit] come out exactly as they
    do in the batch without it: the walk lists are batch-wide, the workspace per image."""
    mask, case, table = built(name)
    H, W = mask.shape
    gates = case["gates"]
    others = [built(n, H, W, None if BUILDERS[n]()[1]["gates"] == gates else gates) for n in NEIGHBOURS[name]]
    # the case exceeds exactly the one limit it is named for
    over = {-3: len(table) > 384 or sum(c["kept"] for c in table) > 256, -2: local_candidates(mask) > 1024,
            -5: any(c["kept"] for c in table[8:]) and [c["parent_order"] for c in table] == list(range(-1, len(table) - 1))}
    assert [code for code, yes in over.items() if yes] == [OVER_LIMIT[name]]
    masks = [others[0][0], mask, others[1][0], others[2][0]]
    xy, cnt, recs = run(masks, gates, form)
    print(name, form, "counts", cnt.tolist())
    assert cnt[1] == OVER_LIMIT[name]
    assert recs[1] == [] and (xy[1] == SENTINEL).all()   # dbg_count == 0, no centroid written
    xy0, cnt0, recs0 = run([masks[0], masks[2], masks[3]], gates, form)
    for i, j in ((0, 0), (2, 1), (3, 2)):
        assert cnt[i] == cnt0[j] and cnt[i] >= 0 and np.array_equal(xy[i], xy0[j]) and canon(recs[i]) == canon(recs0[j]), (name, form, i)
        m, c, t = others[j]
        check_image(m, c, t, gates, xy0[j], cnt0[j], recs0[j], 256)


@pytest.mark.parametrize("form", FORMS)
def test_more_kept_contours_than_max_blobs_are_counted_not_written(form):
    """256 kept contours into max_blobs = 128: the count is the true 256, the first 128 centroids are the reference's
    first 128, and the caller's rows beyond them are not touched (xy buffer of 256 rows per image, pre-filled)."""
    mask, case, table = built("squares_256_0")
    small, case_s, table_s = built("squares_5_3")
    xy, cnt, recs = run([mask, small], case["gates"], form, max_blobs=128, xy_rows=256)
    assert cnt.tolist() == [256, 5]
    assert xy[0, :128].tolist() == case["kept_xy"][:128] and (xy[0, 128:] == SENTINEL).all()
    assert xy[1, :5].tolist() == case_s["kept_xy"] and (xy[1, 5:] == SENTINEL).all()
    check_image(mask, case, table, case["gates"], xy[0], cnt[0], recs[0], 128)
    check_image(small, case_s, table_s, case["gates"], xy[1], cnt[1], recs[1], 128)


@pytest.mark.parametrize("form", ["links_in_place", "links_deferred"])
def test_more_walk_entries_than_the_waves_first_fill(form):
    """A wave of the follow kernel takes its first 32 entries from 32 x its number; only a batch with more than 32 entries per
    wave (4 waves per CU: 128 x CUs) has the counter hand out the rest.  ceil(128 CUs / 1024) + 4 images: combs_1024 (1024
    entries each) with three squares_256_128 (384 each) in between, in one frame size.  Every image is the oracle's."""
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    first_fill = 128 * torch.cuda.get_device_properties(0).multi_processor_count
    n = -(-first_fill // 1024) + 4
    H, W = BUILDERS["squares_256_128"]()[0].shape
    comb, square = built("combs_1024", H, W), built("squares_256_128", H, W)
    gates = comb[1]["gates"]
    assert square[1]["gates"] == gates
    images = [square if i in (n // 4, n // 2, 3 * n // 4) else comb for i in range(n)]
    entries = sum(local_candidates(m) for m, _, _ in images)
    assert local_candidates(comb[0]) == 1024 and entries > first_fill + 1024, (entries, first_fill)
    xy, cnt, recs = run([m for m, _, _ in images], gates, form)
    print("images", n, "walk entries", entries, "first fill", first_fill)
    for i, (mask, case, table) in enumerate(images):
        assert cnt[i] >= 0, (i, cnt[i])
        check_image(mask, case, table, gates, xy[i], cnt[i], recs[i], 256)


# ---- the list of occupancy cells (MAXCELL = 4096), through mocap_blob_centroids ----------------------------------------
def bar_frame(H, W):
    """full-width bars 9 rows thick every 16 rows, 255 on black: blur, threshold and median leave 5 rows of each"""
    img = np.zeros((H, W), np.uint8)
    for y in range(3, H - 9, 16):
        img[y:y + 9] = 255
    return img


def disc_frame(H, W, seed, n=6):
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 40, (H, W), dtype=np.uint8)
    for _ in range(n):
        cx, cy, r = rng.uniform(60, W - 60), rng.uniform(60, H - 60), rng.uniform(18, 30)
        x0, y0 = int(cx) - 40, int(cy) - 40
        yy, xx = np.mgrid[y0:y0 + 80, x0:x0 + 80]
        img[y0:y0 + 80, x0:x0 + 80][(xx - cx) ** 2 + (yy - cy) ** 2 <= r * r] = 255
    return img


def listed_cells(mask, rows=68):
    """How many cells the candidates kernel lists for this mask (blob_contour_image.hip, phase A), restated from the tiling: strips of
    240 columns, chunks of `rows` rows (68; frames lower than 128 rows: a quarter of the height, at least 8) cut into groups of 8
    rows; a group is listed when it, the group above it (the last group of the chunk above for a chunk's first) or the same
    group of the strip left of it holds a set pixel.  (The filter's occupancy words may mark more groups, never fewer.)"""
    H, W = mask.shape
    if H < 128:
        rows = max(8, (H + 3) // 4)
    n_strips, n_chunks, gpc = (W + 239) // 240, -(-H // rows), (rows + 7) // 8
    cols = np.zeros((H, n_strips * 240), bool)
    cols[:, :W] = mask != 0
    row_occ = cols.reshape(H, n_strips, 240).any(axis=2)
    occ = np.zeros((n_chunks * gpc, n_strips), bool)
    exists = np.zeros(n_chunks * gpc, bool)
    for ch in range(n_chunks):
        for g in range(gpc):
            y0, y1 = ch * rows + 8 * g, min(ch * rows + 8 * g + 8, (ch + 1) * rows, H)
            if y0 < y1:
                exists[ch * gpc + g] = True
                occ[ch * gpc + g] = row_occ[y0:y1].any(axis=0)
    scan = occ.copy()
    scan[1:] |= occ[:-1]
    scan[:, 1:] |= occ[:, :-1]
    return int(scan[exists].sum())


def centroids(ctx, frames):
    import torch
    xy, cnt = ctx.record_views(ctx.blob_centroids(torch.from_numpy(np.stack(frames)).cuda()))
    xy, cnt = xy.cpu().numpy(), cnt.cpu().numpy()
    return [xy[i, :max(0, cnt[i])].tolist() for i in range(len(frames))], cnt.tolist()


@pytest.mark.parametrize("W,H,over", [(3840, 2160, True), (1920, 1080, False)], ids=["4k", "1080p_control"])
def test_a_frame_with_every_cell_occupied_is_not_refused(W, H, over):
    """Full-width bars on a 3840 x 2160 frame: 135 borders, none kept -- and a set pixel in every 8-row group of every
    strip, more cells than the candidates kernel's list holds (4096).  That is no documented limit: the frame's answer is
    the reference's (no centroid, count 0), alone and as the middle image of a batch whose other frames (discs) are not
    affected.  The same bars at 1920 x 1080 stay within the list."""
    import torch
    from mocapv2_amd.engine import MocapContext
    assert torch.cuda.is_available(), "these tests need the MI355X"
    K = np.array([[0.7 * W, 0, W / 2.0], [0, 0.7 * W, H / 2.0], [0, 0, 1]])
    bars = bar_frame(H, W)
    frames = [disc_frame(H, W, 1), bars, disc_frame(H, W, 2)]
    ref = [oracle.find_dot(f, K, np.zeros(5)) for f in frames]
    _, mask = oracle.find_dot(bars, K, np.zeros(5), return_mask=True)
    n_listed = listed_cells(mask)
    print(W, H, "listed cells", n_listed, "rows with set pixels", int((mask != 0).any(axis=1).sum()))
    assert (n_listed > 4096) == over
    table = oracle.find_contours(mask)
    assert len(table) == H // 16 and not any(c["kept"] for c in table) and ref[1] == []
    assert len(ref[0]) >= 4 and len(ref[2]) >= 4
    ctx = MocapContext(W, H, 1)
    assert ctx.set_undistort(0, K, np.zeros(5))
    got, cnt = centroids(ctx, frames)
    print("counts", cnt)
    assert cnt == [len(r) for r in ref] and got == ref
    got, cnt = centroids(ctx, [bars])
    assert cnt == [0]


# ---- the per-image kernels as a fixed grid looping over the images (contour_blocks_per_cu > 0, more images than workgroups) ----
LOOP_W, LOOP_H, LOOP_GATES = 96, 64, (1.0, 0.05)


def _dots():
    """an isolated pixel on every second column of every second row: 48 x 32 = 1536 start candidates, one over MAXC and a half"""
    m = np.zeros((LOOP_H, LOOP_W), np.uint8)
    m[1::2, 1::2] = 255
    return m


LOOP_MASKS = [lambda: rings(2, 3)[0], lambda: ring_column(13)[0],   # 13 links that only a walk settles: the wait list, the second passes
              lambda: rings(4, 7)[0],                               # a kept border at depth 9: MOCAP_BLOB_E_DEPTH, from the tree kernel
              lambda: squares(5, 3, H=LOOP_H, W=LOOP_W)[0], lambda: rings(3, 3)[0],
              _dots,                                                # MOCAP_BLOB_E_CANDIDATES, from the candidates kernel
              lambda: np.rot90(ring_column(9)[0]), lambda: rings(3, 0)[0][::-1, ::-1]]
LOOP_CODES = {2: -5, 5: -2}


@functools.lru_cache(maxsize=None)
def loop_masks():
    """the eight masks, embedded top-left in a 96 x 64 frame, and the oracle's table of each for LOOP_GATES"""
    out = []
    for make in LOOP_MASKS:
        big = np.zeros((LOOP_H, LOOP_W), np.uint8)
        m = np.asarray(make())
        big[:m.shape[0], :m.shape[1]] = m
        big.setflags(write=False)
        out.append((big, oracle.find_contours(big, min_area=LOOP_GATES[0], min_circ=LOOP_GATES[1])))
    return out


def looping_batch():
    """(number of workgroups, number of images, which of `k` distinct inputs image i takes): 37 more images than the device has
    CUs, so that with one workgroup per CU the first 37 workgroups take two images and the rest one; the second round is shifted
    by one, so that the two images of a workgroup are never the same input"""
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    grid = torch.cuda.get_device_properties(0).multi_processor_count
    return grid, grid + 37, lambda i, k: (i + i // grid) % k


@pytest.mark.parametrize("defer", [0, 2], ids=["links_in_place", "links_deferred"])
def test_looping_grid_over_a_callers_masks(defer):
    """contour_blocks_per_cu = 1 and more images than CUs: the candidates and the tree kernel run as a fixed grid whose workgroups
    take a second image with the first one's state still in LDS.  Every image equals the oracle's table of its mask (borders,
    measurements, parents, order, centroids); the two over-limit masks carry their codes -- one raised by the candidates kernel,
    one by the tree kernel -- as the first and as the second image of a workgroup, and the image that shares the workgroup with
    them is as good as any other."""
    grid, n, pick = looping_batch()
    cases = loop_masks()
    which = [pick(i, len(cases)) for i in range(n)]
    assert all(which[b] != which[b + grid] for b in range(n - grid))
    for k, code in LOOP_CODES.items():  # an over-limit image first and second in a workgroup, a good one beside it
        assert any(which[b] == k and which[b + grid] not in LOOP_CODES for b in range(n - grid))
        assert any(which[b + grid] == k and which[b] not in LOOP_CODES for b in range(n - grid))
        table = cases[k][1]
        assert (local_candidates(cases[k][0]) > 1024) if code == -2 else any(c["kept"] for c in table[8:]) and len(table) == 9
    nested = [sum(c["parent_order"] >= 0 for c in t) for _, t in cases]
    assert nested[1] >= 14 and nested[0] >= 4  # rings within rings: links that need a walk
    xy, cnt, recs = run([cases[k][0] for k in which], LOOP_GATES, "links_in_place", max_blobs=64,
                        tuning={"contour_blocks_per_cu": 1, "contour_defer": defer})
    print("images", n, "workgroups", grid, "counts of the first 16", cnt[:16].tolist())
    for i, k in enumerate(which):
        mask, table = cases[k]
        if k in LOOP_CODES:
            assert cnt[i] == LOOP_CODES[k] and recs[i] == [] and (xy[i] == SENTINEL).all(), (i, k, cnt[i])
            continue
        assert cnt[i] >= 0, (i, k, cnt[i])
        check_image(mask, None, table, LOOP_GATES, xy[i], cnt[i], recs[i], 64)


def loop_frame(seed):
    """64 x 44: dark noise, one disc large enough to be kept (or, seed 3, none), a small one, and (seed 4) a hole in the large one"""
    rng = np.random.default_rng(900 + seed)
    W, H = 64, 44
    img = rng.integers(0, 50, (H, W), dtype=np.uint8)
    yy, xx = np.mgrid[0:H, 0:W]
    cx, cy, r = 20 + 6 * seed, 20 + (seed % 3), 15 + seed % 2
    if seed != 3:
        img[(xx - cx) ** 2 + (yy - cy) ** 2 <= r * r] = 255
    if seed == 4:
        img[(xx - cx) ** 2 + (yy - cy) ** 2 <= 36] = 0
    sx = 56 if cx < 32 else 6
    img[(xx - sx) ** 2 + (yy - 8 - 5 * seed) ** 2 <= 16] = 255
    return img


@pytest.mark.parametrize("defer", [0, 2], ids=["links_in_place", "links_deferred"])
def test_looping_grid_over_filtered_frames(defer):
    """The same grid on the context's own mask, where the candidates kernel lists the occupied cells (in the LDS its next image
    reuses): five distinct 64 x 44 frames, cycled, against oracle.find_dot."""
    from mocapv2_amd.engine import MocapContext
    grid, n, pick = looping_batch()
    W, H = 64, 44
    K = np.array([[0.7 * W, 0, W / 2.0], [0, 0.7 * W, H / 2.0], [0, 0, 1]])
    distinct = [loop_frame(s) for s in range(5)]
    ref = [oracle.find_dot(f, K, np.zeros(5)) for f in distinct]
    assert sum(len(r) for r in ref) >= 3 and len({str(r) for r in ref}) >= 4
    which = [pick(i, 5) for i in range(n)]
    assert all(which[b] != which[b + grid] for b in range(n - grid))
    ctx = MocapContext(W, H, 1)
    assert ctx.set_undistort(0, K, np.zeros(5))
    ctx.set_tuning("contour_blocks_per_cu", 1)
    ctx.set_tuning("contour_defer", defer)
    got, cnt = centroids(ctx, [distinct[k] for k in which])
    print("images", n, "workgroups", grid, "reference", ref)
    for i, k in enumerate(which):
        assert cnt[i] == len(ref[k]) and got[i] == ref[k], (i, k, cnt[i])
