"""mocap_fundamental_ransac on the GPU at its integer seams (csrc/fundamental.hip), against the restatement
(tests/fundamental_ref.py).  The cases are tests/fundamental_seam_cases.py; tests/test_fundamental_seams_host.py proves on the
CPU that none of them has a (hypothesis, point) pair within the relative 1e-6 band of threshold^2 and that every winner leads by
2 inliers at the least, so nothing is excused here.  Every comparison is compare_with_restatement of tests/test_gpu_fundamental.py,
with its F_TOL = 1e-9 and BAND_CAP = 1e-6: per-hypothesis counts, winner, inlier count and mask equal, both matrices within
F_TOL."""
import numpy as np
import pytest

import fundamental_ref as fr
import fundamental_seam_cases as fs
from test_gpu_fundamental import F_TOL, compare_with_restatement, same_bits

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available()
    from mocapv2_amd.engine import MocapContext
    return MocapContext(1, 1)


def run(ctx, a, b, S):
    return ctx.fundamental_ransac([(a, b)], [S], fs.THRESHOLD, refit=True, with_counts=True)[0]


def test_point_lists_that_end_on_and_one_past_a_chunk_in_one_batch(ctx):
    """Eight pairs of 255, 256, 257, 1023, 1024, 1025, 2048 and 2049 points with 257 hypotheses each, in one call.  The scorer's
    grid has the three chunks of the largest pair, so every shorter pair has whole workgroups that leave early; 1024 and 2048
    end on a chunk, 1025 and 2049 one past it (a chunk of one point), and 256, 257 do the same to the mask's blocks.  Every pair:
    the full comparison with the restatement, and the same bits as the pair run alone.
    The restatement: winners 210, 148, 4, 244, 228, 19, 110, 9 with 178, 179, 177, 718, 712, 669, 1385, 1436 inliers, leads of
    3 to 238, no banded pair.
    Measured on an MI355X: every count, winner and mask equal; |dF_sample| <= 7.4e-15 (256 points), |dF_refit| <= 7.8e-16 (255)
    over the eight."""
    pairs = [fs.pair(n) for n in fs.POINT_COUNTS]
    tables = [fs.table(n, fs.H_SEAM) for n in fs.POINT_COUNTS]
    batch = ctx.fundamental_ransac(pairs, tables, fs.THRESHOLD, refit=True, with_counts=True)
    assert len(batch) == len(fs.POINT_COUNTS)
    for n, got in zip(fs.POINT_COUNTS, batch):
        compare_with_restatement(f"batch n {n} H {fs.H_SEAM}", got, fs.reference(n, fs.H_SEAM), n)
    for n, p, S, got in zip(fs.POINT_COUNTS, pairs, tables, batch):
        assert same_bits(got, run(ctx, *p, S)), n


@pytest.mark.parametrize("H", fs.HYP_COUNTS)
def test_hypothesis_tables_that_end_on_and_one_past_a_wave_and_a_tile(ctx, H):
    """1025 points with 63, 64, 65, 255, 256, 257 and 513 hypotheses: the solver's last wave holds 63, 64 or 1 lanes, the scorer's
    and the arg-max's last tile 255, 256 or 1.  The restatement's winner is hypothesis 19 with 669 inliers in all seven.
    Measured on an MI355X: every count, winner and mask equal; |dF_sample| 1.0e-15, |dF_refit| 1.4e-16 in all seven."""
    a, b = fs.pair(fs.N_SEAM)
    compare_with_restatement(f"n {fs.N_SEAM} H {H}", run(ctx, a, b, fs.table(fs.N_SEAM, H)), fs.reference(fs.N_SEAM, H), fs.N_SEAM)


@pytest.mark.parametrize("name", sorted(fs.TIES))
def test_planted_ties_go_to_the_lowest_index_from_whichever_lane(ctx, name):
    """600 hypotheses over 1025 points; the winner's row (19, 669 inliers) copied to other rows and taken out of its own.
    first: rows 200, 259 and 515 tie -- lane 3 of the arg-max holds 259 then 515, lane 200 holds 200, the lower index in the higher
    lane; 200 wins.  second: rows 44, 45, 300 and 556 -- one lane with three strides beside its neighbour; 44 wins.  third: rows
    200 and 328 -- lane 72 holds 328 and meets lane 200's 200 in the tree's first step, the lower index coming from above.
    The tied sets and winners are the restatement's (asserted on the CPU).
    Measured on an MI355X: winners 200, 44, 200 with 669 inliers, every count equal."""
    rows, winner = fs.TIES[name]
    a, b = fs.pair(fs.N_SEAM)
    ref = fs.tie_reference(name)
    got = run(ctx, a, b, fs.tie_table(name))
    compare_with_restatement(f"ties {name}", got, ref, fs.N_SEAM)
    assert got["best"] == winner and (got["counts"][list(rows)] == got["n_inliers"]).all()
    assert int((got["counts"] == got["n_inliers"]).sum()) == len(rows)


def test_nan_and_inf_points_are_no_inliers_and_their_samples_score_nothing(ctx):
    """The 1025-point pair with a[5] = a[700] = NaN and b[9] = inf.  The restatement: the 6 hypotheses of 257 that sample one of
    the three are invalid, winner 19 with 667 inliers, mask 0 at the three points.
    Measured on an MI355X: the same, the invalid hypotheses' counts 0; |dF_sample| 1.0e-15, |dF_refit| 2.2e-16."""
    a, b = fs.not_finite_pair()
    ref = fs.not_finite_reference()
    got = run(ctx, a, b, fs.table(fs.N_SEAM, fs.H_SEAM))
    compare_with_restatement("NaN and inf points", got, ref, fs.N_SEAM)
    invalid = ~np.isfinite(ref["F_all"]).all((1, 2))
    assert invalid.sum() == 6 and (got["counts"][invalid] == 0).all()
    assert not got["mask"][[5, 9, 700]].any()


@pytest.mark.parametrize("name", sorted(fs.OVERFLOWS))
def test_a_point_whose_products_overflow_is_no_inlier(ctx, name):
    """Point 7 of the 1025-point pair replaced in both lists: (1e200, 1e200) twice; (1e160, 2e160) and (3e160, 1e160); (inf, inf)
    twice.  The definition's error of such a point is inf / inf = NaN, which is not an inlier: the restatement's mask leaves it out
    under every valid hypothesis (winner 19, 669 inliers; the 3 hypotheses that sample the point are invalid), and its refit is the
    refit without the point.
    The inlier test as first written, n^2 <= thr^2 * den without a division, held for the two finite points (inf <= inf).
    Measured on an MI355X before the fix: 75 (1e200) and 99 (1e160) of the 257 hypotheses counted point 7, the winner among them,
    the refit over a mask with that point overflowed, and the whole pair came back as MOCAP_FUND_E_DEGENERATE with an empty mask;
    (inf, inf) passed.  is_inlier now asks for a finite n^2.
    Measured on an MI355X with the fix: every count, winner and mask equal the restatement's in all three; |dF_sample| 1.0e-15,
    |dF_refit| 1.4e-16."""
    a, b = fs.overflow_pair(name)
    ref, refit_without = fs.overflow_reference(name)
    got = run(ctx, a, b, fs.table(fs.N_SEAM, fs.H_SEAM))
    print(f"overflow {name}: best {got['best']} inliers {got['n_inliers']} mask[7] {int(got['mask'][fs.OVERFLOW_POINT])} "
          f"hypotheses counting another number {int((got['counts'] != ref['counts']).sum())} of {fs.H_SEAM}")
    assert got["best"] >= 0, got["best"]
    compare_with_restatement(f"overflow {name}", got, ref, fs.N_SEAM)
    assert got["mask"][fs.OVERFLOW_POINT] == 0
    dF = float(np.abs(fr.align_sign(got["F_refit"], refit_without) - refit_without).max())
    assert dF <= F_TOL
