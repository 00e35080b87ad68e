"""The yardstick of tests/test_gpu_contour_limits.py, checked where there is no GPU: the constructed masks of
tests/contour_cases.py give, through the CPU oracle, exactly the tables their construction states."""
import numpy as np
import pytest

import oracle
from contour_cases import (assert_matches_case, combs, form_of_oracle, local_candidates, ring_column, rings, squares)


def table_of(mask, case):
    return oracle.find_contours(mask, min_area=case["gates"][0], min_circ=case["gates"][1])


def depth(table, i):
    d = 0
    while i >= 0:
        d, i = d + 1, table[i]["parent_order"]
    return d


@pytest.mark.parametrize("n_big,n_small,n_borders,n_kept", [(256, 128, 384, 256), (256, 129, 385, 256), (257, 127, 384, 257), (256, 0, 256, 256)])
def test_squares(n_big, n_small, n_borders, n_kept):
    mask, case = squares(n_big, n_small)
    assert mask.shape == (192, 384)
    table = table_of(mask, case)
    assert len(table) == n_borders and sum(c["kept"] for c in table) == n_kept
    assert_matches_case(case, form_of_oracle(table))
    assert local_candidates(mask) == case["candidates"] == n_borders
    # the closed form itself: an s x s square at (x, y) is the polygon (s-1) x (s-1) through its corner pixels' centres
    for c in table:
        s = 9 if c["kept"] else 3
        assert mask[c["oy"]:c["oy"] + s, c["ox"]:c["ox"] + s].all() and not mask[c["oy"] + s, c["ox"]] and not mask[c["oy"], c["ox"] + s]
        assert c["area"] == (s - 1) ** 2 and c["perimeter"] == 4 * (s - 1) and c["npts"] == 4 and not c["is_hole"]
        if c["kept"]:
            assert (c["cx"], c["cy"]) == (c["ox"] + 4, c["oy"] + 4)
    # kept order = reverse raster order of the start pixels (test_oracle_blob.py::test_contour_order_is_reverse_raster_for_simple_blobs)
    kept = [(c["oy"], c["ox"]) for c in table if c["kept"]]
    assert kept == sorted(kept, reverse=True)
    assert case["kept_xy"] == [[c["cx"], c["cy"]] for c in table if c["kept"]]


@pytest.mark.parametrize("dot,n_borders,n_kept,kept_depth", [(0, 8, 8, 8), (7, 9, 9, 9), (3, 9, 8, 8)])
def test_rings(dot, n_borders, n_kept, kept_depth):
    mask, case = rings(4, dot)
    table = table_of(mask, case)
    assert len(table) == n_borders and sum(c["kept"] for c in table) == n_kept
    assert [c["parent_order"] for c in table] == list(range(-1, n_borders - 1))  # border k's parent is border k - 1
    assert [c["is_hole"] for c in table] == [k % 2 for k in range(n_borders)]
    assert max(depth(table, i) for i, c in enumerate(table) if c["kept"]) == kept_depth
    assert max(depth(table, i) for i in range(len(table))) == n_borders
    assert_matches_case(case, form_of_oracle(table))
    assert case["kept_xy"] == [[c["cx"], c["cy"]] for c in table if c["kept"]]
    assert local_candidates(mask) == case["candidates"]


@pytest.mark.parametrize("n_teeth", [1024, 1025])
def test_combs(n_teeth):
    mask, case = combs(n_teeth)
    table = table_of(mask, case)
    assert len(table) == 12 and not any(c["kept"] for c in table) and not any(c["is_hole"] for c in table)
    assert_matches_case(case, form_of_oracle(table))
    assert local_candidates(mask) == case["candidates"] == n_teeth
    # no foreground run touches the row above near a tooth top: the tops' rows hold nothing but tooth tops, below blank rows
    for c in table:
        assert not mask[c["oy"] - 1].any() and mask[c["oy"]].sum() // 255 in (93, n_teeth - 11 * 93)


@pytest.mark.parametrize("n", [64, 65, 70])
def test_ring_column(n):
    mask, case = ring_column(n)
    assert mask.shape[1] == 40
    table = table_of(mask, case)
    assert len(table) == n + 2 and all(c["kept"] for c in table)
    ring_outer = [i for i, c in enumerate(table) if (c["ox"], c["oy"], c["is_hole"]) == (2, 2, 0)]
    ring_hole = [i for i, c in enumerate(table) if c["is_hole"]]
    assert len(ring_outer) == 1 and len(ring_hole) == 1 and table[ring_hole[0]]["parent_order"] == ring_outer[0]
    squares_ = [c for i, c in enumerate(table) if i not in (ring_outer[0], ring_hole[0])]
    assert len(squares_) == n and all(c["parent_order"] == ring_hole[0] and c["area"] == 4 for c in squares_)
    assert_matches_case(case, form_of_oracle(table))
    assert case["kept_xy"] == [[c["cx"], c["cy"]] for c in table if c["kept"]]
    assert local_candidates(mask) == case["candidates"] == (n + 1) + 1  # n + 1 outer starts, one hole start


def test_local_candidates_on_small_masks():
    m = np.zeros((4, 5), np.uint8)
    assert local_candidates(m) == 0
    m[1, 1] = 255
    assert local_candidates(m) == 1
    m[:] = 255
    assert local_candidates(m) == 1  # the top-left pixel; no background at all
    m[2, 2] = 0
    assert local_candidates(m) == 2  # ... and the hole
