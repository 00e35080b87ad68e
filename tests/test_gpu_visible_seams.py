"""mocap_correspond_visible on the GPU at its integer seams (csrc/correspond_visible.hip), against the restatement
(tests/correspond_visible_ref.py): exactly `cap` seeds in a pass (the last one in LDS) and one more (the first one in the
context's scratch), a power of two for the bitonic sort (no padding) and one more (the most padding), several time steps side by
side in the scratch, max_hyp at the seed count in scratch, and the output rows running out in a later pass.  The cases are
tests/visible_seam_cases.py (C = 8, P = 32: cap = 2048); tests/test_visible_seams_host.py proves on the CPU that each has the seed
count it is named for and a decision margin above 1e-6.  Every comparison is assert_equals_restatement of
tests/test_gpu_correspond_visible.py: idx, views and n equal, xyz and err within ten times the larger of the restatement's own
deviation from exact_hypotheses and 1e-12, margin > 1e-6."""
import numpy as np
import pytest

import correspond_visible_ref as cv
import visible_seam_cases as vs
from test_gpu_correspond_visible import assert_equals_restatement, run_gpu, run_ref

pytestmark = pytest.mark.gpu

KEYS = ("xyz", "err", "idx", "views")


@pytest.fixture(scope="module")
def ctx():
    from mocapv2_amd.engine import MocapContext
    return MocapContext(1, 1)


def rows_of(gpu, t):
    """the bytes of time step t's result rows (the rows below n[t]; none for an error code)"""
    n = max(int(gpu["n"][t]), 0)
    return (int(gpu["n"][t]),) + tuple(gpu[k][t, :n].tobytes() for k in KEYS)


def check(ctx, pts, counts, what, **kw):
    gpu = run_gpu(ctx, pts, counts, vs.cams(), **kw)
    refs = run_ref(pts, counts, vs.cams(), **kw)
    assert_equals_restatement(gpu, refs, pts, vs.cams(), what=what)
    return gpu, refs


@pytest.mark.parametrize("seed,k", [(1, k) for k in vs.COUNTS] + [(2, k) for k in (2047, 2048, 2049)])
def test_seed_counts_on_and_beside_every_power_of_two(ctx, seed, k):
    """Pass 0 has exactly k seeds, k in {1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097}: with cap = 2048, up to 2048 in
    LDS and from 2049 in scratch; the sort pads 1025 to 2048, 2049 to 4096, 4097 to 8192 and 1024, 2048, 4096 not at all.  Every
    run has a second pass of 11 to 30 seeds in LDS, after a scratch pass over the stale keys of the first 2048.  max_hyp = 8192.
    The restatement: seed 1 gives 34, 34, 34, 35, 35, 35, 35, 35, 35 markers (margin 5.68e-6), seed 2 gives 33 at its three
    counts (6.73e-6).
    Measured on an MI355X: idx, views and n equal in all twelve; xyz and err equal the restatement's bit for bit (deviation 0).
    What these results cannot show, measured with edited kernels: a sort fill that lets index n through is the same code at a
    power of two (n2 = n) and elsewhere sorts in whatever record lies behind the pass's own
    (test_what_an_earlier_call_left_behind_the_records_is_not_sorted_in puts a kept one there); and a kernel that leaves slot
    `cap` in LDS at 2049 seeds loses one seed of 2049, whichever the hardware handed that slot, which changes these markers only
    if it was a marker's single seed (test_513_seeds_each_a_markers_only_seed_around_a_cap_of_512 makes every seed one)."""
    pts, counts, cut, _ = vs.single(seed, k)
    gpu, refs = check(ctx, pts, counts, f"seed {seed}, {k} seeds", cutoff=cut, max_hyp=vs.MAX_HYP)
    assert refs[0]["seeds"][0] == k and gpu["n"][0] == refs[0]["n"] > 0


def test_four_steps_in_lds_and_scratch_side_by_side(ctx):
    """T = 4 at seed 1's cutoff for 2048 seeds (20.27 px): step 0 has exactly cap seeds (LDS), step 1 is seed 2 with 2203
    (scratch), step 2 the 6-marker scene with 151 (LDS), step 3 seed 2 with every list reversed, 2203 again (scratch, at
    scratch + 3 * step_bytes).  Every step equals the restatement, equals byte for byte the same step run alone, and the call
    with the steps in the order 3, 1, 2, 0 gives the same bytes per scene.
    Measured on an MI355X: 35, 35, 6 and 35 markers, deviation 0 in every step."""
    pts, counts, cut = vs.four_steps()
    kw = dict(cutoff=cut, max_hyp=vs.MAX_HYP)
    gpu, refs = check(ctx, pts, counts, "T = 4", **kw)
    assert [r["seeds"][0] for r in refs] == [vs.CAP, 2203, 151, 2203]
    for t in range(4):
        alone = run_gpu(ctx, pts[t:t + 1], counts[t:t + 1], vs.cams(), **kw)
        assert rows_of(alone, 0) == rows_of(gpu, t), t
    order = [3, 1, 2, 0]
    moved = run_gpu(ctx, pts[order], counts[order], vs.cams(), **kw)
    for k, t in enumerate(order):
        assert rows_of(moved, k) == rows_of(gpu, t), (k, t)
    assert rows_of(gpu, 1) != rows_of(gpu, 3)  # the two scratch steps are no copies of each other


def test_max_hyp_equal_to_the_seed_count_in_scratch(ctx):
    """Seed 1 with 2049 seeds as step 0 beside the small scene as step 1.  max_hyp = 2049: the order array starts right behind
    the last record (g_recs + max_hyp * rec) and both steps equal the restatement.  max_hyp = 2048: step 0 is E_GROUPS, step 1
    is byte for byte what it was.
    Measured on an MI355X: 35 and 6 markers, deviation 0; -2 and the same 6."""
    pts, counts, cut = vs.with_neighbour(1, vs.CAP + 1)
    at, refs = check(ctx, pts, counts, "max_hyp = seeds = 2049", cutoff=cut, max_hyp=vs.CAP + 1)
    assert refs[0]["seeds"][0] == vs.CAP + 1 and at["n"][0] > 0
    under, _ = check(ctx, pts, counts, "max_hyp = seeds - 1 = 2048", cutoff=cut, max_hyp=vs.CAP)
    assert under["n"][0] == cv.E_GROUPS and rows_of(under, 1) == rows_of(at, 1) and at["n"][1] > 0


def test_max_hyp_4097_is_no_power_of_two(ctx):
    """4097 seeds with max_hyp = 4097: the records end at 4097 * 24 bytes, the order array behind them takes pow2_at_least(4097)
    = 8192 entries -- the offset and the size of a step's scratch, together; one fewer is E_GROUPS.
    Measured on an MI355X: 35 markers, deviation 0."""
    pts, counts, cut = vs.with_neighbour(1, 4097)
    at, refs = check(ctx, pts, counts, "max_hyp = seeds = 4097", cutoff=cut, max_hyp=4097)
    assert refs[0]["seeds"][0] == 4097 and at["n"][0] > 0
    under, _ = check(ctx, pts, counts, "max_hyp = 4096", cutoff=cut, max_hyp=4096)
    assert under["n"][0] == cv.E_GROUPS and rows_of(under, 1) == rows_of(at, 1)


def test_output_rows_run_out_in_a_later_pass(ctx):
    """Seed 1 with 2049 seeds: pass 0 (scratch) accepts 31 markers, passes 1 and 2 (LDS) bring them to 35.  Q = 35 equals the
    restatement; Q = 34 holds everything pass 0 accepts, so MOCAP_CORR_E_OUTPUT is raised with rows carried over from an
    earlier pass (q >= Q with q starting at nout > 0) -- and the small scene beside it is untouched.
    Measured on an MI355X: 35 and 6 markers, deviation 0; -5 and the same 6."""
    seed, k = vs.LATER_PASS
    n3 = vs.restatement(seed, k, max_passes=3)["n"]
    n1 = vs.restatement(seed, k, max_passes=1)["n"]
    assert n3 - 1 >= n1 > 0
    pts, counts, cut = vs.with_neighbour(seed, k)
    fits, refs = check(ctx, pts, counts, "Q = n", cutoff=cut, Q=n3)
    assert fits["n"][0] == n3 == refs[0]["n"] and fits["xyz"].shape[1] == n3
    one, _ = check(ctx, pts, counts, "one pass, Q = n - 1", cutoff=cut, Q=n3 - 1, max_passes=1)
    assert one["n"][0] == n1                         # pass 0 alone fits the shorter table
    short, _ = check(ctx, pts, counts, "Q = n - 1", cutoff=cut, Q=n3 - 1)
    assert short["n"][0] == cv.E_OUTPUT and rows_of(short, 1) == rows_of(fits, 1) and fits["n"][1] > 0


def test_the_same_call_twice_at_4097_seeds(ctx):
    """Slots are handed out by an integer atomic in whatever order the lanes arrive; the sort's key is a total order, so the
    same call gives the same bytes -- in scratch, with the most padding, as in LDS."""
    pts, counts, cut, _ = vs.single(1, 4097)
    kw = dict(cutoff=cut, max_hyp=vs.MAX_HYP)
    a, b = run_gpu(ctx, pts, counts, vs.cams(), **kw), run_gpu(ctx, pts, counts, vs.cams(), **kw)
    assert a["n"][0] > 0 and rows_of(a, 0) == rows_of(b, 0)


# ---- beyond the sweep: what its results cannot show ----------------------------------------------------------------------------
def test_twelve_steps_two_scratch_scenes_on_every_xcd_that_has_one(ctx):
    """The four steps above land on four XCDs, whose L2s do not show each other's stores to the scratch before the kernel ends:
    measured on an MI355X, that test passes with every step working at the scratch's start.  With T = 12 the workgroups t and
    t + 8 share an XCD: steps 1 and 9, and 3 and 11, are seed 2 and seed 2 reversed, both in scratch at once.  Every step equals
    the restatement and, byte for byte, the same scene in the four-step call.
    Measured on an MI355X: 35, 35, 6, 35 markers per scene, deviation 0 in all twelve steps."""
    pts, counts, cut, order = vs.twelve_steps()
    kw = dict(cutoff=cut, max_hyp=vs.MAX_HYP)
    four_refs = run_ref(*vs.four_steps()[:2], vs.cams(), **kw)
    gpu = run_gpu(ctx, pts, counts, vs.cams(), **kw)
    assert_equals_restatement(gpu, [four_refs[s] for s in order], pts, vs.cams(), what="T = 12")
    four = run_gpu(ctx, *vs.four_steps()[:2], vs.cams(), **kw)
    for t, s in enumerate(order):
        assert rows_of(gpu, t) == rows_of(four, s), (t, s)


def test_what_an_earlier_call_left_behind_the_records_is_not_sorted_in(ctx):
    """A call with 4097 seeds, every one kept as a two-view hypothesis (gate 1e-3 px, max_err 1e30), leaves 4097 kept records
    with free points in the scratch.  The next call has 2049 seeds and keeps none (max_err 1e-9): the sort pads 2049 to 4096 with
    ORD_END, and a fill that let one index past n through would put the earlier call's record 2049, the only kept one, first.
    n must be 0, as the restatement's.
    Measured on an MI355X: 0 markers; with `k <= n` in the fill, 2."""
    _, pts, counts, _, _ = vs.scene(1)
    pts, counts = pts[None], counts[None].astype(np.int32)
    cut_a, _ = vs.cutoff_for(1, vs.POISON["seeds"])
    a = run_gpu(ctx, pts, counts, vs.cams(), cutoff=cut_a, gate=vs.POISON["gate"], max_err=vs.POISON["max_err"], max_passes=1)
    assert a["n"][0] > 0 and (a["views"][0, :a["n"][0]] != 0).all()
    cut_b, _ = vs.cutoff_for(1, vs.DROPPED["seeds"])
    gpu, refs = check(ctx, pts, counts, "2049 seeds, none kept", cutoff=cut_b, max_err=vs.DROPPED["max_err"])
    assert refs[0]["seeds"] == [vs.CAP + 1] and gpu["n"][0] == refs[0]["n"] == 0


def test_513_seeds_each_a_markers_only_seed_around_a_cap_of_512(ctx):
    """C = 32, P = 128: LDS holds 512 records.  513 markers that two cameras each see once give 513 seeds, every one the only seed
    of an accepted two-view marker (proved on the CPU), so the seed that is handed slot 512 -- the first record that lives in
    scratch only, whichever seed the hardware gives it -- decides a marker (max_passes = 1: a second pass would find a lost seed again).  Another scene with no seed key in common runs first
    on the same context, so what that slot held before is no seed of this scene.
    The markers' errors are 1e-10 px^2 and lie 1e-17 apart, so the order of the rows (by error) is not compared: n, the set of
    index rows with their views, and per index row xyz and err within ten times the larger of the restatement's own deviation
    from exact_hypotheses and 1e-12.  The decisions that remain (cutoff, gate, max_err) lie more than 1e-6 off, proved on the CPU.
    Measured on an MI355X: 513 markers, the same rows in the same order, deviation 0; a kernel that leaves slot `cap` in LDS
    returns 512."""
    D = vs.DISJOINT
    other, other_counts, cams = vs.disjoint_scene(D["other_seed"])
    before = run_gpu(ctx, other, other_counts, cams, **vs.disjoint_kw())
    assert before["n"][0] == D["markers"]
    pts, counts, cams = vs.disjoint_scene(D["seed"])
    gpu = run_gpu(ctx, pts, counts, cams, **vs.disjoint_kw())
    ref = run_ref(pts, counts, cams, **vs.disjoint_kw())[0]
    n = int(gpu["n"][0])
    assert ref["seeds"] == [D["cap"] + 1] and n == ref["n"] == D["markers"]
    where = {tuple(row): q for q, row in enumerate(ref["idx"].tolist())}
    rows = [tuple(row) for row in gpu["idx"][0, :n].tolist()]
    assert set(rows) == set(where) and len(set(rows)) == n
    order = [where[row] for row in rows]
    assert np.array_equal(gpu["views"][0, :n], ref["views"][order])
    dev = cv.deviation(ref["xyz"], ref["err"], *cv.exact_hypotheses(pts[0], ref["idx"], *cams))
    got = cv.deviation(gpu["xyz"][0, :n], gpu["err"][0, :n], ref["xyz"][order], ref["err"][order])
    print(f"513 disjoint seeds: n {n} rows in the restatement's order {order == list(range(n))} restatement vs exact {dev:.2e} "
          f"device vs restatement {got:.2e}")
    assert got <= 10 * max(dev, 1e-12), (got, dev)
