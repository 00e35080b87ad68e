"""The oracle-free contour reference of tests/contour_poly_ref.py, checked where there is no GPU: every chain is certified
against scipy.ndimage's labelling while it is built, the seeded masks satisfy the conditions under which no border has to be
excluded from a comparison, and oracle/blob_oracle.c -- written beside the kernels from the same reading of OpenCV -- gives
the same borders with the same statistics, gates, centroids, parents and order, exactly."""
import numpy as np
import pytest

import oracle
from contour_poly_ref import (GATES, REQUIRED_DIAG_RUNS, SIZES, TIE, assert_conditions, batch, borders_of, gated, hand_mask, key_of,
                              reference)

CASES = [(s, g) for s in SIZES for g in GATES]


@pytest.mark.parametrize("size,gates", CASES)
def test_masks_are_certified_and_within_the_conditions(size, gates):
    """building the reference asserts the certification (8-adjacent foreground chain, morphological border set, Pick where no
    pixel repeats, the half-ulp bound on the perimeter); here: the capacities, the gate margins and what the masks must hold"""
    s = assert_conditions(size, gates)
    print(size, gates, {k: v for k, v in s.items() if k != "per_image"}, "per image (borders, kept, candidates, kept depth)", s["per_image"])
    assert s["borders"] > 0 and s["holes"] > 0 and s["kept"] > 0 and s["repeats"] > 0
    assert s["mid_run"] > 0           # a start that is no vertex: its run is merged into the closing run
    assert s["exact_rule"] > 0        # a shape symmetric about a pixel centre: the double recipe decides its centroid
    flat = [b for bs in reference(size, gates) for b in bs]
    assert any(b["steps"] == 0 for b in flat) and any(b["steps"] == 2 and b["npts"] == 2 for b in flat)  # isolated pixel, pair
    assert any(b["is_hole"] and b["mid_run"] and b["kept"] for b in flat)
    assert 0 < sum(b["kept"] for b in flat) < sum(1 for b in flat if b["steps"] > 0)  # both gates' sides are populated
    if size != "64x48":
        assert s["long_diag"] > 0 and any(b["is_hole"] and b["long_diag"] for b in flat)


def test_the_diagonal_runs_the_table_and_its_fallback_meet():
    runs = {k for size in SIZES for bs in reference(size, "near_0.3") for b in bs for k in b["diag_runs"]}
    assert set(REQUIRED_DIAG_RUNS) <= runs, sorted(runs)
    # ... as hole borders too, and with the start mid-run on a run beyond the table (the merge at the closing step)
    holes = {k for size in SIZES for bs in reference(size, "near_0.3") for b in bs if b["is_hole"] and b["mid_run"] for k in b["diag_runs"]}
    assert {62, 64, 65, 129} <= holes, sorted(holes)


def test_sizes_cover_a_width_that_is_no_multiple_of_32():
    assert [batch(s).shape[2] % 32 for s in SIZES] == [0, 13, 0]
    for s in SIZES:
        assert batch(s).shape[0] <= 8 and set(np.unique(batch(s))) <= {0, 255}


def test_known_shapes_by_hand():
    """the reference on shapes whose numbers are worked out by hand (none taken from any implementation)"""
    m = hand_mask()
    bs = {key_of(b): b for b in gated(borders_of(m), 1.25, 0.3)}
    assert set(bs) == {(0, 3, 2), (0, 1, 5), (0, 4, 8), (0, 6, 1), (1, 7, 3)}
    iso, pair, line, sq, hole = (bs[k] for k in ((0, 3, 2), (0, 1, 5), (0, 4, 8), (0, 6, 1), (1, 7, 3)))
    assert (iso["steps"], iso["npts"], iso["a00"], iso["perimeter"], iso["kept"]) == (0, 1, 0, 0.0, 0)
    assert (pair["steps"], pair["npts"], pair["a00"], pair["kept"]) == (2, 2, 0, 0)
    assert pair["perimeter"] == 2 * float(np.sqrt(np.float32(2)))
    assert (line["steps"], line["npts"], line["a00"], line["perimeter"], line["repeats"]) == (8, 2, 0, 8.0, True)
    # the square: polygon 4 x 4 through the corner pixels' centres, walked with the inside on the left of the screen's y-down axes
    assert (sq["steps"], sq["npts"], sq["a00"], sq["area"], sq["perimeter"], sq["kept"], sq["cx"], sq["cy"]) == (16, 4, -32, 16.0, 16.0, 1, 8, 3)
    assert (sq["a10"], sq["a01"]) == (-32 * 3 * 8, -32 * 3 * 3) and not sq["mid_run"]
    # the hole: the diamond through the four 4-neighbours of (8, 3): area 2, four diagonal steps, start (7, 3) is a vertex
    assert (hole["steps"], hole["npts"], hole["a00"], hole["area"], hole["kept"], hole["cx"], hole["cy"]) == (4, 4, 4, 2.0, 1, 8, 3)
    assert hole["perimeter"] == 4 * float(np.sqrt(np.float32(2))) and hole["parent"] >= 0
    assert all(b["parent"] == -1 for b in (iso, pair, line, sq))


def test_a_circularity_equal_to_min_circ_is_not_kept():
    """The gate is `circularity > min_circ` on IEEE doubles.  With min_circ the square's own double circularity the square is
    dropped (mpmath's pi / 4 lies 3e-17 above that double: only the double recipe can decide, as for centroids on an integer);
    one ulp lower it is kept.  The hole (pi / 4 too, but from float32 roots: 2.7e-8 above) is kept both times."""
    for min_circ, kept in ((TIE, 0), (np.nextafter(TIE, 0.0), 1)):
        ref = {key_of(b): b for b in gated(borders_of(hand_mask()), 1.25, float(min_circ))}
        assert ref[(0, 6, 1)]["gate_tie"] and ref[(0, 6, 1)]["kept"] == kept and ref[(1, 7, 3)]["kept"] == 1
        table = {(c["is_hole"], c["ox"], c["oy"]): c for c in oracle.find_contours(hand_mask(), min_area=1.25, min_circ=float(min_circ))}
        assert set(table) == set(ref)
        for key, b in ref.items():
            assert (table[key]["kept"], table[key]["cx"], table[key]["cy"]) == (b["kept"], b["cx"], b["cy"]), (key, min_circ)


@pytest.mark.parametrize("size,gates", CASES)
def test_the_c_oracle_agrees_with_the_reference(size, gates):
    min_area, min_circ = GATES[gates]
    compared = 0
    for mask, ref in zip(batch(size), reference(size, gates)):
        table = oracle.find_contours(mask, min_area=min_area, min_circ=min_circ)
        got = {(c["is_hole"], c["ox"], c["oy"]): c for c in table}
        exp = {key_of(b): b for b in ref}
        assert len(got) == len(table) and set(got) == set(exp), sorted(set(got) ^ set(exp))[:6]
        for key, b in exp.items():
            c = got[key]
            for f in ("steps", "npts", "a00", "a10", "a01", "area", "perimeter", "kept", "cx", "cy"):
                assert c[f] == b[f] and type(c[f]) is type(b[f]), (key, f, c[f], b[f])
            parent = None if b["parent"] < 0 else key_of(ref[b["parent"]])
            c_parent = None if c["parent_order"] < 0 else (lambda p: (p["is_hole"], p["ox"], p["oy"]))(table[c["parent_order"]])
            assert c_parent == parent, (key, c_parent, parent)
            compared += 1
        # the table is in output order: the kept ones in the reference's order, with its centroids
        kept = [(c["is_hole"], c["ox"], c["oy"]) for c in table if c["kept"]]
        assert kept == [key_of(b) for b in sorted((b for b in ref if b["kept"]), key=lambda b: b["order"])]
    assert compared == sum(len(r) for r in reference(size, gates))
