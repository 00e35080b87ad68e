"""The contour kernels (csrc/blob_contour_image.hip: `follow`; blob_contour_follow.hip: its pair-of-lanes form in contour_follow_kernel; contours_dev.h: select_contour and
the tree passes) held to the oracle-free reference of tests/contour_poly_ref.py -- scipy.ndimage's labelling for which borders
exist, where they start and how they nest; exact integer and rational arithmetic, float32 roots and mpmath for what is measured
on them -- instead of to oracle/blob_oracle.c, which was written beside the kernels from the same reading of OpenCV
(tests/test_contour_poly_host.py holds that oracle to the same reference without a GPU).

Each size's masks go as one batch through mocap_contours_from_mask in the three forms the library ships.  Records are matched
by (is_hole, sx, sy); steps, npts, a00, a10, a01 are compared as integers, area and perimeter as doubles that both sides form
exactly, kept, cx, cy, the parent and the output order as they are: no tolerance anywhere, no border excluded.

Measured on the MI355X (the same in all three forms, and for both gate sets unless two figures are given as 0.3 / 0.5):
    size      masks  borders compared  of them holes  start mid-run  diagonal runs > 63  centroids under the      smallest gate margin
                                                                                          exact-integer rule       |circ - min_circ|
    64x48       8        198               85              5                 0                 9 / 17               0.0589 / 0.0390
    301x200     5         76               19              7                14                23 / 24               0.00352 / 0.00265
    640x360     4        199               18              7                32                24 / 26               0.00130 / 0.00265
All 18 cases and the three tie cases pass, 3 s in all.  With `2 * x + dx` -> `2 * x` in `follow` (a10 from one end of each step
instead of both; built and run once, not part of the tree) the seven one_kernel cases fail at the first record's a10 -- e.g.
((0, 199, 12), 'a10', -2881400, -2885733) -- and the 14 cases of the split forms, which do not run `follow`, pass."""
import numpy as np
import pytest

from contour_poly_ref import GATES, SIZES, TIE, assert_conditions, batch, borders_of, gated, hand_mask, key_of, reference
from test_gpu_contour_limits import FORMS, SENTINEL, run

pytestmark = pytest.mark.gpu

INT_FIELDS = ("steps", "npts", "a00", "a10", "a01", "kept", "cx", "cy")


def compare(ref, recs, xy, count, max_blobs=256):
    """the kernel's records, count and centroids of one image against the reference's gated border list; -> borders compared"""
    exp = {key_of(b): b for b in ref}
    got = {(r["is_hole"], r["sx"], r["sy"]): r for r in recs}
    assert len(got) == len(recs) and set(got) == set(exp), (sorted(set(got) ^ set(exp))[:6], len(recs), len(ref))
    for key, b in exp.items():
        r = got[key]
        for f in INT_FIELDS:
            assert r[f] == b[f], (key, f, r[f], b[f])
        assert r["area"] == b["area"] and r["perimeter"] == b["perimeter"], (key, r["area"], b["area"], r["perimeter"], b["perimeter"])
        parent = None if b["parent"] < 0 else key_of(ref[b["parent"]])
        r_parent = None if r["parent"] < 0 else (recs[r["parent"]]["is_hole"], recs[r["parent"]]["sx"], recs[r["parent"]]["sy"])
        assert r_parent == parent, (key, r_parent, parent)
        if b["kept"]:
            assert r["order"] == b["order"], (key, r["order"], b["order"])
    kept = sorted((b for b in ref if b["kept"]), key=lambda b: b["order"])
    assert count == len(kept) <= max_blobs
    assert xy[:count].tolist() == [[b["cx"], b["cy"]] for b in kept]
    assert (xy[count:] == SENTINEL).all()  # nothing is written beyond the centroids
    return len(exp)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("gates", GATES)
@pytest.mark.parametrize("size", SIZES)
def test_records_equal_the_polygon_reference(size, gates, form):
    s = assert_conditions(size, gates)  # on the CPU, before anything is asked of the GPU
    masks, ref = batch(size), reference(size, gates)
    xy, cnt, recs = run(list(masks), GATES[gates], form)
    assert (cnt >= 0).all(), cnt.tolist()
    compared = sum(compare(ref[i], recs[i], xy[i], cnt[i]) for i in range(len(masks)))
    print(size, gates, form, "borders compared", compared, "holes", s["holes"], "kept", s["kept"], "start mid-run", s["mid_run"],
          "diagonal runs > 63", s["long_diag"], "exact-integer rule", s["exact_rule"], "smallest gate margin", s["min_margin"])
    assert compared == s["borders"] > 0 and s["mid_run"] > 0


@pytest.mark.parametrize("form", FORMS)
def test_a_circularity_equal_to_min_circ_is_not_kept(form):
    """`circularity > min_circ` on doubles: a 5 x 5 square (area 16, perimeter 16) with min_circ its own double circularity is
    dropped, one ulp lower it is kept; its hole border (float32 roots: 2.7e-8 above) is kept both times."""
    mask = hand_mask(48, 64)
    borders = borders_of(mask)
    for min_circ, n_kept in ((TIE, 1), (float(np.nextafter(TIE, 0.0)), 2)):
        ref = gated(borders, 1.25, min_circ)
        assert sum(b["kept"] for b in ref) == n_kept and [b["gate_tie"] for b in ref if key_of(b) == (0, 6, 1)] == [True]
        xy, cnt, recs = run([mask], (1.25, min_circ), form)
        assert compare(ref, recs[0], xy[0], cnt[0]) == 5
