"""The inputs of test_gpu_own_mask.py, checked without a GPU: every named frame of own_mask_cases.py routes through the restated
rules the way its name says, the oracle alone finds the intended blobs in it, and the sequences together meet every pair
(previous route, this batch's route) of own_mask_cases.REQUIRED -- so that no GPU case passes on a transition it was not built for.
test_sequences_meet_the_required_pairs prints the pairs every sequence meets (pytest -s)."""
import collections

import numpy as np

import own_mask_cases as cases
from mocapv2_amd.synth import ZERO_DIST, Scene
from test_gpu_box_forms import choose_split, expected
from test_gpu_tile_record import LIMIT, list_counts


def test_named_frames_route_as_their_names_say():
    for name, want in cases.NAMED_ROUTES.items():
        got = cases.routes(cases.FRAMES[name])
        assert sorted(got) == sorted(want), (name, got)
        for tile, w in want.items():
            kind, region = (w, None) if isinstance(w, str) else w
            assert got[tile][0][0] == kind and (region is None or got[tile][1] == region), (name, tile, got[tile], w)
    for name, runs in cases.NAMED_RUNS.items():
        assert cases.routes(cases.FRAMES[name])[(0, 0)][0] == ("split", runs), (name, cases.routes(cases.FRAMES[name])[(0, 0)])
    # the cluster of `corner` dissolves beside a second disc in tile (0, 0); `edge_x` is a cluster of two tiles
    assert all(r[0] == ("item", 1, 1) for t, r in cases.routes(cases.FRAMES["corner_plus"]).items() if t != (0, 0))
    # the item cut into parts: 13 mask bytes x 68 rows, below the routing limit of the wide list, two parts side by side
    route, (x0, x1, y0, y1) = cases.routes(cases.FRAMES["multi"])[(0, 0)]
    assert ((x1 - x0 + 8) >> 3, y1 - y0 + 1) == (13, 68) and choose_split(13, 68) == (2, 1) and 2 * 13 + 2 * 2 < LIMIT and route == ("item", 2, 1)
    # every tile of the all-bright frame is marked: wide entries in the two whole strips; the 32 columns of the last strip are an
    # item in each of the upper two chunks and one cluster item over the lower two
    hot = cases.routes(cases.FRAMES["hot"])
    assert len(hot) == 12 and all((r[0][0] == "wide") == (st < 2) for (ch, st), r in hot.items()), hot
    assert [hot[(ch, 2)][0][0] for ch in range(4)] == ["item", "item", "cluster_emit", "cluster_member"]
    # without the split the tiles stay wide entries; the Bayer path has no wide list
    assert cases.routes(cases.FRAMES["two"], wide_split=False)[(0, 0)] == (("wide",), (0, 239, 20, 51))
    assert cases.routes(cases.FRAMES["bar"], wide_list=False)[(0, 0)][0][0] == "item"
    assert len(cases.routes(cases.FRAMES["edges_a"])) >= 6 and any(st == 1 for _, st in cases.routes(cases.FRAMES["edges_b"]))


def test_totals_agree_with_the_list_counts_of_the_record_tests():
    """two restatements of one rule: the totals of routes() are list_counts() of test_gpu_tile_record.py on every frame"""
    for name, f in cases.FRAMES.items():
        assert cases.totals(cases.routes(f)) == tuple(int(v) for v in list_counts(f)), name
        assert cases.totals(cases.routes(f, wide_list=False)) == tuple(int(v) for v in list_counts(f, wide_list=False)), name


def test_oracle_finds_the_intended_blobs():
    for name, n in cases.BLOBS.items():
        f = cases.FRAMES[name]
        K = Scene(1, width=f.shape[1], height=f.shape[0]).K
        mask, blobs = expected(f[None], K, np.asarray(ZERO_DIST, float), False)[0]
        assert len(blobs) == n, (name, blobs)
        print(name, "blobs", blobs, "set pixels", int(mask.sum()))
        assert mask.any() == (n > 0), name  # (disc_small: a marked tile whose region holds no set pixel)


def test_stale_pieces_lie_where_the_cases_say():
    """two -> three: the disc `two` leaves at x = 180 lies half in a gap and half in a run of `three`; gap_disc -> two: the previous
    region lies inside the gap between the runs of `two`, so nothing but the split tile's own clearing removes it; corner -> disc:
    the cluster's disc has set pixels in the last byte column of tile (0, 0)'s region"""
    K = Scene(1, width=512, height=208).K
    mask_of = lambda n: expected(cases.FRAMES[n][None], K, np.asarray(ZERO_DIST, float), False)[0][0]  # noqa: E731
    runs = cases.NAMED_RUNS["three"]
    gap, run = slice(8 * runs[1][1] + 8, 8 * runs[2][0]), slice(8 * runs[2][0], 8 * runs[2][1] + 8)
    assert mask_of("two")[:, gap].any() and mask_of("two")[:, run].any()
    (_, r1), (r2, _) = cases.NAMED_RUNS["two"]
    x0, x1, y0, y1 = cases.routes(cases.FRAMES["gap_disc"])[(0, 0)][1]
    assert 8 * r1 + 8 <= x0 and x1 < 8 * r2 and mask_of("gap_disc")[y0:y1 + 1, x0:x1 + 1].any()
    x0, x1, y0, y1 = cases.routes(cases.FRAMES["corner"])[(0, 0)][1]
    assert mask_of("corner")[y0:y1 + 1, x1 - 7:x1 + 1].any()


def test_sequences_meet_the_required_pairs():
    met = collections.Counter()
    for name in cases.SEQUENCES:
        here = collections.Counter()
        for step, image, tile, prev, now in cases.transitions(name):
            if prev[0][0] != "unmarked" or now[0][0] != "unmarked":
                here[cases.pair_of(prev, now)] += 1
                if "unknown" not in (prev[0][0], now[0][0]):
                    print(f"  {name} step {step} image {image} tile {tile}: {prev[0]} {prev[1]} -> {now[0]} {now[1]}")
        print(name + ":", ", ".join(f"{p} -> {q}" + (f" ({rel})" if rel else "") + f" x{n}" for (p, q, rel), n in sorted(here.items(), key=str)))
        met.update(here)
    missing = [(p, q, rel) for p, q, rel in cases.REQUIRED if not any(k[:2] == (p, q) and rel in (None, k[2]) for k in met)]
    assert not missing, missing
    # without the split the same sequences turn the split tiles into wide entries
    off = collections.Counter(cases.pair_of(p, q)[:2] for *_, p, q in cases.transitions("wide_item_split", wide_split=False))
    assert off[("wide", "wide")] >= 4 and not any("split" in k for k in off), off
