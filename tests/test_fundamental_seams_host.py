"""The fundamental-matrix seam cases (tests/fundamental_seam_cases.py), the part that needs no GPU: every case is what its name
says in the restatement (tests/fundamental_ref.py), and lies far from every decision -- no (hypothesis, point) pair within the
relative 1e-6 band of threshold^2, every winner at least 2 inliers ahead, the planted ties tied as planted -- so that
tests/test_gpu_fundamental_seams.py excuses nothing.  The seams themselves are read from csrc/fundamental.hip: a changed
constant fails here, and nothing is silently tested off the seam."""
import os
import re

import numpy as np
import pytest

import fundamental_ref as fr
import fundamental_seam_cases as fs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def lead_of(ref):
    """inliers of the winner minus those of the best other valid hypothesis"""
    counts = ref["counts"].copy()
    counts[ref["best"]] = -1
    return int(ref["n_inliers"] - counts.max())


def test_the_counts_stand_on_the_kernels_seams():
    with open(os.path.join(ROOT, "mocapv2_amd", "csrc", "fundamental.hip")) as f:
        source = f.read()
    constants = {k: int(v) for k, v in re.findall(r"constexpr int (HYP_LANES|SCORE_THREADS|SCORE_CHUNK) = (\d+);", source)}
    assert constants == {"HYP_LANES": 64, "SCORE_THREADS": 256, "SCORE_CHUNK": 1024}
    assert "(a.max_n + 255) / 256" in source and "h += 256" in source  # the mask's block, the arg-max's stride
    chunk, tile, wave = constants["SCORE_CHUNK"], constants["SCORE_THREADS"], constants["HYP_LANES"]
    for seam in (256, chunk, 2 * chunk):
        assert {seam, seam + 1} <= set(fs.POINT_COUNTS)
    assert {255, chunk - 1} <= set(fs.POINT_COUNTS)
    for seam in (wave, tile):
        assert {seam - 1, seam, seam + 1} <= set(fs.HYP_COUNTS)
    assert 2 * tile + 1 in fs.HYP_COUNTS
    assert fs.N_SEAM == chunk + 1 and fs.H_SEAM == tile + 1 and max(fs.POINT_COUNTS) == fs.N_MAX == 2 * chunk + 1
    # the batch of all point counts: the grid has three chunks, so the pairs of up to 1024 points leave two workgroups early and
    # those of up to 2048 one; four pairs end on a chunk or one past it
    assert sorted(-(-n // chunk) for n in fs.POINT_COUNTS) == [1, 1, 1, 1, 1, 2, 2, 3]
    assert sum(n % chunk in (0, 1) for n in fs.POINT_COUNTS) == 4


@pytest.mark.parametrize("n,H", fs.used_cases())
def test_no_pair_in_the_band_and_the_winner_alone_at_the_top(n, H):
    """Measured here: winner 19 in every (1025, H) case with H >= 63 ... 513 (669 inliers, then 626 at the most); the smallest
    lead over all cases is printed below."""
    ref = fs.reference(n, H)
    a, _ = fs.pair(n)
    assert len(a) == n and fs.table(n, H).shape == (H, 8) and fs.table(n, H).max() < n
    assert ref["best"] >= 0 and np.isfinite(ref["F_all"]).all()
    print(f"n {n} H {H}: winner {ref['best']} with {ref['n_inliers']}, lead {lead_of(ref)}, banded {int(ref['banded'].sum())}")
    assert ref["banded"].sum() == 0
    assert lead_of(ref) >= 2
    if n == fs.N_SEAM and H >= 63:
        assert ref["best"] == fs.WINNER and ref["n_inliers"] == 669


@pytest.mark.parametrize("name", sorted(fs.TIES))
def test_planted_ties_are_tied_and_the_lowest_index_wins(name):
    rows, winner = fs.TIES[name]
    plain = fs.reference(fs.N_SEAM, fs.H_TIES)
    assert plain["best"] == fs.WINNER and lead_of(plain) >= 2 and plain["banded"].sum() == 0
    ref = fs.tie_reference(name)
    top = ref["counts"].max()
    assert top == plain["n_inliers"] == 669
    assert tuple(np.flatnonzero(ref["counts"] == top)) == rows and ref["best"] == winner == min(rows)
    assert ref["counts"][fs.WINNER] < top - 1 and ref["banded"].sum() == 0
    others = ref["counts"].copy()
    others[list(rows)] = -1
    assert top - others.max() >= 2
    lanes = [r % 256 for r in rows]
    if name == "first":
        # the lowest index sits in a higher lane than the other two, which share a lane (the strict '>' keeps 259): lane 200's
        # record comes down to lane 0 (200 -> 72 -> 8 -> 0), lane 3's to lane 1, and they meet in the tree's last step
        assert lanes == [200, 3, 3] and winner % 256 > 3
    elif name == "second":
        assert lanes == [44, 45, 44, 44]  # three strides in one lane beside its neighbour
    else:
        # the tree's first step joins lane 72 (holding 328) with lane 72 + 128 (holding 200): the lower index comes from above,
        # the branch `i2 < s_idx[tid]` is taken with equal counts
        assert lanes == [200, 72] and rows[1] > rows[0] and lanes[0] - lanes[1] == 128


def test_not_finite_points_invalidate_their_samples_and_are_no_inliers():
    ref = fs.not_finite_reference()
    S = fs.table(fs.N_SEAM, fs.H_SEAM)
    a, b = fs.not_finite_pair()
    bad = ~(np.isfinite(a).all(1) & np.isfinite(b).all(1))
    assert tuple(np.flatnonzero(bad)) == (5, 9, 700)
    invalid = ~np.isfinite(ref["F_all"]).all((1, 2))
    assert np.array_equal(invalid, np.isin(S, np.flatnonzero(bad)).any(1)) and invalid.sum() == 6
    assert (ref["counts"][invalid] == 0).all()
    assert (ref["best"], ref["n_inliers"]) == (fs.WINNER, 667) and not ref["mask"][bad].any()
    assert ref["banded"].sum() == 0 and lead_of(ref) >= 2
    assert np.isfinite(ref["F_refit"]).all()


@pytest.mark.parametrize("name", sorted(fs.OVERFLOWS))
def test_an_overflowing_point_is_no_inlier_of_the_definition(name):
    """inf / inf is NaN, and NaN <= threshold^2 is false: the definition's mask leaves the point out, for every valid hypothesis.
    The three hypotheses that sample the point are invalid (their normalisation overflows)."""
    ref, refit_without = fs.overflow_reference(name)
    a, b = fs.overflow_pair(name)
    p = fs.OVERFLOW_POINT
    S = fs.table(fs.N_SEAM, fs.H_SEAM)
    invalid = ~np.isfinite(ref["F_all"]).all((1, 2))
    assert np.array_equal(invalid, (S == p).any(1)) and invalid.sum() == 3
    plain = fs.reference(fs.N_SEAM, fs.H_SEAM)
    # the honest point 7 is an outlier of the winner (of 30 % outliers) and an inlier of some other hypotheses; the replaced one is
    # an inlier of none, so every valid hypothesis counts what it counted without the point
    was_inlier = np.array(_inlier_of_all(plain, p))
    assert not plain["mask"][p] and was_inlier.any()
    assert (ref["best"], ref["n_inliers"]) == (fs.WINNER, 669) and not ref["mask"][p]
    assert np.array_equal(ref["counts"][~invalid], (plain["counts"] - was_inlier)[~invalid])
    assert ref["banded"].sum() == 0 and lead_of(ref) >= 2
    assert np.array_equal(ref["F_refit"], refit_without)  # the mask left the point out, so this is the same computation
    if name != "inf":
        assert np.isfinite(a[p]).all() and np.isfinite(b[p]).all()
        with np.errstate(all="ignore"):
            assert not np.isfinite(a[p, 0] * a[p, 0])


def _inlier_of_all(plain, p):
    """whether point p of the plain 1025-point pair is an inlier of each hypothesis"""
    a, b = fs.pair(fs.N_SEAM)
    out = []
    for F in plain["F_all"]:
        out.append(fr.errors(F, a[p:p + 1], b[p:p + 1])[0] <= fs.THRESHOLD ** 2)
    return out
