"""mocap_fundamental_ransac on the GPU against the NumPy restatement of its definition (tests/fundamental_ref.py), on the
reference's bundled capture and on seeded synthetic pairs with outliers; batch and run independence; the calibration chain
and the tracker fed with estimated matrices."""
import json
import os

import numpy as np
import pytest

import fundamental_ref as fr
import oracle
from mocapv2_amd.synth import Scene

pytestmark = pytest.mark.gpu

SMALL = ["bundled", "s11", "s12", "s13", "s14", "s15"]
F_TOL = 1e-9        # largest entry difference of unit-norm matrices: the worst spread between correct FP64 solvers
BAND_CAP = 1e-6     # share of (hypothesis, point) pairs that may lie within a relative 1e-6 of threshold^2


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available()
    from mocapv2_amd.engine import MocapContext
    return MocapContext(1, 1)


_ref_cache = {}


def reference(name):
    if name not in _ref_cache:
        a, b, S, thr, extras = fr.small_case(name)
        _ref_cache[name] = (a, b, S, thr, extras, fr.ransac(a, b, S, thr))
    return _ref_cache[name]


def compare_with_restatement(tag, got, ref, n_points):
    """The C3 comparison; returns the figures it printed."""
    H = len(ref["counts"])
    diff = np.abs(got["counts"].astype(np.int64) - ref["counts"])
    banded = int(ref["banded"].sum())
    dF_s = float(np.abs(fr.align_sign(got["F_sample"], ref["F_sample"]) - ref["F_sample"]).max())
    dF_r = float(np.abs(fr.align_sign(got["F_refit"], ref["F_refit"]) - ref["F_refit"]).max())
    print(f"{tag}: winner {got['best']} / {ref['best']}  inliers {got['n_inliers']} / {ref['n_inliers']}  hypotheses with "
          f"another count {int((diff > 0).sum())} of {H}  banded pairs {banded}  |dF_sample| {dF_s:.3g}  |dF_refit| {dF_r:.3g}")
    assert banded <= BAND_CAP * H * n_points
    assert (diff <= ref["banded"]).all(), np.flatnonzero(diff > ref["banded"])[:10]
    assert got["best"] == ref["best"] and got["n_inliers"] == ref["n_inliers"]
    assert np.array_equal(got["mask"].astype(bool), ref["mask"]) and int(got["mask"].sum()) == got["n_inliers"]
    assert dF_s <= F_TOL and dF_r <= F_TOL
    return dF_s, dF_r


# ---- C3 ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SMALL)
def test_counts_winner_mask_and_matrices_equal_the_restatement(ctx, name):
    """Same sample table on both sides.  Per-hypothesis inlier counts, winner, inlier count and mask: equal (the restatement
    has no (hypothesis, point) pair within a relative 1e-6 of threshold^2 in any of these cases, so nothing is excused).
    F_sample and F_refit: largest entry difference after aligning the sign <= 1e-9.
    Measured on an MI355X: no hypothesis of any case with another count; largest |dF_sample| 1.07e-14 (s12), largest
    |dF_refit| 1.2e-16 (s11) over the six cases."""
    a, b, S, thr, _, ref = reference(name)
    got = ctx.fundamental_ransac([(a, b)], [S], thr, refit=True, with_counts=True)[0]
    compare_with_restatement(name, got, ref, len(a))


def test_an_odd_number_of_pairs_times_an_odd_number_of_hypotheses(ctx):
    """s11, s13 and s14 in one call, each with the first five rows of its sample table: n_pairs = 3 and n_pairs * H = 15 are odd,
    so the matrices of all hypotheses (72 bytes each) end on an odd multiple of 8 bytes and the counters, the pairs' error words
    and the offsets behind them in the call's scratch start 8 bytes further on than a packed layout would put them.  Every pair:
    the full comparison with the restatement on the same five samples.
    The restatement (CPU) on these: winners 4, 4, 0 with 218, 201, 54 inliers, no (hypothesis, point) pair within the band, and
    every winner ahead of the other four hypotheses (37, 130, 53 at most) -- checked here before the GPU is asked.
    Measured on an MI355X: every count, winner and mask equal; |dF_sample| <= 4.6e-16, |dF_refit| <= 2.3e-16 over the three."""
    names = ("s11", "s13", "s14")
    cases = [reference(n)[:4] for n in names]
    assert all(c[3] == 3.0 for c in cases)
    tables = [np.ascontiguousarray(c[2][:5]) for c in cases]
    refs = [fr.ransac(c[0], c[1], S, 3.0) for c, S in zip(cases, tables)]
    for name, ref in zip(names, refs):
        lead = ref["counts"] + ref["banded"]
        lead[ref["best"]] = -1
        assert ref["best"] >= 0 and ref["counts"][ref["best"]] - ref["banded"][ref["best"]] > lead.max(), name
    res = ctx.fundamental_ransac([(c[0], c[1]) for c in cases], tables, 3.0, refit=True, with_counts=True)
    assert len(res) == 3
    for name, c, got, ref in zip(names, cases, res, refs):
        compare_with_restatement(name + " (5 samples)", got, ref, len(c[0]))


def test_the_restatements_table_of_winners():
    """What the yardstick itself gives on the small cases (CPU arithmetic; here so that a change of the generators shows)."""
    want = {"bundled": (28, 54), "s11": (108, 1398), "s12": (358, 295), "s13": (528, 241), "s14": (0, 54), "s15": (294, 575)}
    for name in SMALL:
        ref = reference(name)[5]
        assert (ref["best"], ref["n_inliers"]) == want[name], name


def test_refit_beats_the_minimal_sample_on_the_noise_free_points(ctx):
    """s11-s15: RMS of sqrt(e_i) of F_refit on the noise-free projections is below that of F_sample (restatement: 0.05-0.33
    against 0.74-1.22 px)."""
    for name in SMALL[1:]:
        a, b, S, thr, (a0, b0, _), _ = reference(name)
        got = ctx.fundamental_ransac([(a, b)], [S], thr)[0]
        r_s, r_r = fr.rms_distance(got["F_sample"], a0, b0), fr.rms_distance(got["F_refit"], a0, b0)
        print(f"{name}: rms on noise-free points: sample {r_s:.3f} refit {r_r:.3f}")
        assert r_r < r_s


# ---- C4 ----------------------------------------------------------------------------------------------------------------
def same_bits(x, y):
    for k in ("F_sample", "F_refit", "mask", "counts"):
        if (x[k] is None) != (y[k] is None):
            return False
        if x[k] is not None and np.asarray(x[k]).tobytes() != np.asarray(y[k]).tobytes():
            return False
    return x["best"] == y["best"] and x["n_inliers"] == y["n_inliers"]


def test_a_pairs_results_do_not_depend_on_the_batch_or_the_run(ctx):
    cases = [reference(n) for n in SMALL]
    pairs, tables = [(c[0], c[1]) for c in cases], [c[2] for c in cases]
    # one threshold per call: the bundled capture's 10 is run at the synthetic cases' 3 here (any value serves this test)
    batch = ctx.fundamental_ransac(pairs, tables, 3.0, with_counts=True)
    again = ctx.fundamental_ransac(pairs, tables, 3.0, with_counts=True)
    singles = [ctx.fundamental_ransac([p], [t], 3.0, with_counts=True)[0] for p, t in zip(pairs, tables)]
    for name, x, y, z in zip(SMALL, batch, again, singles):
        assert x["best"] >= 0, name
        assert same_bits(x, y), ("run", name)
        assert same_bits(x, z), ("batch", name)
    # reversed order, and a batch with a degenerate pair and one with a sample index outside its list
    rev = ctx.fundamental_ransac(pairs[::-1], tables[::-1], 3.0, with_counts=True)[::-1]
    assert all(same_bits(x, y) for x, y in zip(batch, rev))
    flat = np.full((300, 2), 512.25)
    from mocapv2_amd.calibrate import sample_table
    bad = tables[4].copy()
    bad[17, 3] = len(pairs[4][0])  # one past the end
    neg = tables[4].copy()
    neg[999, 0] = -1
    mixed = ctx.fundamental_ransac(pairs[:3] + [(flat, flat), (pairs[4][0], pairs[4][1])] + pairs[3:] + [(pairs[4][0], pairs[4][1])],
                                   tables[:3] + [sample_table(300, 1000, 1), bad] + tables[3:] + [neg], 3.0, with_counts=True)
    assert mixed[3]["best"] == -3 and mixed[3]["F_sample"] is None and mixed[3]["F_refit"] is None and not mixed[3]["mask"].any()
    assert mixed[3]["n_inliers"] == 0 and not mixed[3]["counts"].any()
    for r in (mixed[4], mixed[8]):
        assert r["best"] == -2 and r["F_sample"] is None and not r["mask"].any()
    for x, y in zip(batch, mixed[:3] + mixed[5:8]):
        assert same_bits(x, y)


def test_argument_errors_are_reported(ctx):
    import ctypes as C
    import torch
    from mocapv2_amd import _abi
    a, b, S, thr, _, _ = reference("s14")
    with pytest.raises(ValueError):
        ctx.fundamental_ransac([(a, b[:-1])], [S], thr)
    with pytest.raises(ValueError):
        ctx.fundamental_ransac([(a, b)], [S, S], thr)
    with pytest.raises(_abi.MocapError) as e:
        ctx.fundamental_ransac([(a[:7], b[:7])], [S], thr)
    assert e.value.code == -1 and "8" in str(e.value)
    with pytest.raises(_abi.MocapError):
        ctx.fundamental_ransac([(a, b)], [S], 0.0)
    # offsets that do not increase, H < 1, null pointers: straight at the C-ABI
    d = torch.zeros(64, dtype=torch.float64, device="cuda")
    i32 = torch.zeros(64, dtype=torch.int32, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    off = (C.c_int * 3)(0, 16, 8)
    lib = ctx.lib
    assert lib.mocap_fundamental_ransac(ctx._h, 2, p(d), p(d), off, p(i32), 1, 3.0, 0, p(d), None, p(i32), p(i32), None, None) == -1
    assert b"pair 1" in lib.mocap_last_error()
    off = (C.c_int * 2)(0, 16)
    assert lib.mocap_fundamental_ransac(ctx._h, 1, p(d), p(d), off, p(i32), 0, 3.0, 0, p(d), None, p(i32), p(i32), None, None) == -1
    assert lib.mocap_fundamental_ransac(ctx._h, 1, p(d), p(d), off, p(i32), 1, 3.0, 1, p(d), None, p(i32), p(i32), None, None) == -1
    assert lib.mocap_fundamental_ransac(ctx._h, 1, None, p(d), off, p(i32), 1, 3.0, 0, p(d), None, p(i32), p(i32), None, None) == -1


# ---- C5 ----------------------------------------------------------------------------------------------------------------
def test_the_users_size_fifteen_pairs_of_twenty_thousand_points(ctx):
    """16-camera ring, pairs 0-i, 20 000 points each with 30 % outliers, H = 2048, one call.  Pairs 0-1, 0-8 and 0-15 get
    the full comparison with the restatement.  All 15: the reported count is the number of points with e_i <= threshold^2
    under the returned F_sample (NumPy), at least 98 % of the true inliers are in the mask, and F_refit is closer to the
    noise-free projections than F_sample.
    Measured on an MI355X: 13 924-14 028 inliers per pair of 14 000 true ones, 99.31-100.00 % of them kept, 11-40 false
    ones; refit 0.016-0.066 px against 0.23-0.79 px; the three compared pairs: every count equal (2, 2 and 0 banded pairs
    of 4.1e7), |dF_sample| <= 9.6e-15, |dF_refit| <= 3.5e-15."""
    data = [fr.large_case(i) for i in range(1, 16)]
    res = ctx.fundamental_ransac([(d[0], d[1]) for d in data], [d[2] for d in data], 3.0, with_counts=True)
    for i, (d, got) in enumerate(zip(data, res), start=1):
        a, b, _, thr, (a0, b0, true_inlier) = d
        assert got["best"] >= 0
        with np.errstate(invalid="ignore"):
            recount = int((fr.errors(got["F_sample"], a, b) <= thr ** 2).sum())
        kept = (got["mask"].astype(bool) & true_inlier).sum() / true_inlier.sum()
        r_s, r_r = fr.rms_distance(got["F_sample"], a0, b0), fr.rms_distance(got["F_refit"], a0, b0)
        print(f"pair 0-{i}: winner {got['best']} inliers {got['n_inliers']} (numpy {recount}) true inliers kept {100 * kept:.2f} % "
              f"false {int((got['mask'].astype(bool) & ~true_inlier).sum())} rms noise-free sample {r_s:.3f} refit {r_r:.3f}")
        assert got["n_inliers"] == recount == int(got["mask"].sum()) == int(got["counts"][got["best"]])
        assert kept >= 0.98
        assert r_r < r_s
    for i in (1, 8, 15):
        a, b, S, thr, _ = data[i - 1]
        compare_with_restatement(f"large 0-{i}", res[i - 1], fr.ransac(a, b, S, thr), len(a))


# ---- C6 ----------------------------------------------------------------------------------------------------------------
def test_the_calibration_chain_on_the_references_capture(ctx):
    """calculate_extrinsics on jsons/image_points.json with camera-params-in.json: the cheirality vote is unanimous (108 of
    108), the bundle adjustment ends with status > 0, and its mean residual is at most 1.10 x the one the same bundle
    adjustment reaches from cv2's matrix (fundamentals.json[0]).  Both are measured here.
    Measured on an MI355X: 69.117 from cv2's matrix, 72.095 from the refit (1.0431 x), |R - R(k1_bundled)| 0.0201 -- the
    figures the restatement with the C oracle's residual under SciPy gives on a CPU (69.12, 72.09).
    The rotation after BA is compared with k1_bundled.npz for the record only; the sign of t is left open by the vote."""
    from mocapv2_amd import calibrate as cal
    golden = os.path.join(fr.GOLDEN, "jsons")
    ip = cal.get_points(os.path.join(golden, "image_points.json"))
    with open(os.path.join(golden, "camera-params-in.json")) as f:
        params = json.load(f)
    out = cal.calculate_extrinsics(ip, params, ctx=ctx)
    assert len(out["poses"]) == 2 and len(out["pair_Fs"]) == 1 and out["pair_Fs"][0][2, 2] == 1.0
    assert max(out["votes"][0]) == 2 * len(ip[0]) == 108
    assert out["ba_result"].status > 0
    mean_ours = float(np.mean(out["ba_result"].fun))
    F_cv = fr.bundled_cv2_fundamental()
    initial = cal.extrinsics_from_fundamentals(ip, [F_cv], params, ctx)
    _, res_cv = cal.bundle_adjustment(np.transpose(ip, (1, 0, 2)), initial, params, ctx=ctx)
    mean_cv = float(np.mean(res_cv.fun))
    k1 = np.load(os.path.join(fr.GOLDEN, "k1_bundled.npz"))
    dR = float(np.abs(out["poses"][1]["R"] - k1["R"][1]).max())
    print(f"mean BA residual: from the estimated matrix {mean_ours:.3f}, from cv2's {mean_cv:.3f} (ratio {mean_ours / mean_cv:.4f}); "
          f"|R - R(k1_bundled)| {dR:.4f}; mean reprojection error after BA {out['error']:.3f}; mask {int(out['masks'][0].sum())} of 54")
    assert res_cv.status > 0
    assert mean_ours <= 1.10 * mean_cv
    assert out["object_points"].shape == (54, 3) and np.isfinite(out["error"])


# ---- C7 ----------------------------------------------------------------------------------------------------------------
def test_tracker_runs_on_estimated_fundamentals(ctx):
    """tracker_fundamentals on a 6-camera ring (seed 70, 2000 points, 30 % outliers in every camera but the first, threshold
    3, H = 1000) set through mocap_set_fundamentals; 40 fresh time steps of 8 markers (seeds 700-739), cutoff 10 px.
    (a) roots and groups from the GPU equal oracle.correspond given the same estimated matrices: exact, every step;
    (b) they equal the result with the ground-truth Scene.Fs in at least 36 of the 40 steps -- a cap on what an estimated
    matrix may change (a candidate a hair inside the cutoff under one matrix can be outside under the other), not a
    tolerance.  Measured on an MI355X: 38 of 40 (the restatement's matrices with the C oracle on a CPU: 39 of 40)."""
    import torch
    from mocapv2_amd import calibrate as cal
    sc = Scene(6)
    pts, clean, true_inlier = fr.ring_points(sc, 2000, 70, 0.30)
    res = cal.find_fundamental_matrices(pts, [(0, i) for i in range(1, 6)], threshold=3.0, hypotheses=1000, seed=70, ctx=ctx,
                                        details=True)
    for i, (F, mask, r) in enumerate(res, start=1):
        rms = fr.rms_distance(r["F_refit"], clean[0], clean[i])
        print(f"pair 0-{i}: inliers {r['n_inliers']} of {int(true_inlier[i].sum())} true, refit rms on noise-free points {rms:.3f} px")
        # an estimated matrix must place the noise-free points better than the 0.5 px jitter of one detection; how many inliers
        # the best MINIMAL sample collects depends on that sample (1351-1402 for 1400 true ones here; refit 0.017-0.088 px) and is printed, not bounded
        assert rms < 0.5
    Fs = cal.tracker_fundamentals(pts, threshold=3.0, hypotheses=1000, seed=70, ctx=ctx)
    assert len(Fs) == 5 and all(np.array_equal(F, r[0]) for F, r in zip(Fs, res))
    C, M, T = 6, 8, 40
    K, dist = np.stack([sc.K] * C), np.stack([sc.dist] * C)
    R, t = np.stack([p["R"] for p in sc.poses]), np.stack([p["t"] for p in sc.poses])
    steps = np.zeros((T, C, M, 2), np.int32)
    cnt = np.full((T, C), M, np.int32)
    for s in range(T):
        rng = np.random.default_rng(700 + s)
        cents = sc.centroids(sc.markers(rng, M))
        for c in range(C):
            steps[s, c] = cents[c]
    ctx.set_cameras(K, dist, R, t)

    def run(F):
        ctx.set_fundamentals(np.stack(F))
        out = ctx.correspond(torch.from_numpy(steps).cuda(), torch.from_numpy(cnt).cuda())
        n = out["n"].cpu().numpy()
        assert (n >= 0).all()
        return n, out["root"].cpu().numpy(), out["grp"].cpu().numpy()

    n_e, root_e, grp_e = run(Fs)
    for s in range(T):
        ref = oracle.correspond(steps[s].astype(float), cnt[s], K, dist, R, t, np.stack(Fs))
        assert n_e[s] == len(ref["root"]) and np.array_equal(root_e[s, :n_e[s]], ref["root"])
        assert np.array_equal(grp_e[s, :n_e[s]], ref["groups"])
    n_t, root_t, grp_t = run(sc.Fs)
    same = sum(int(n_e[s] == n_t[s] and np.array_equal(root_e[s, :n_e[s]], root_t[s, :n_t[s]])
                   and np.array_equal(grp_e[s, :n_e[s]], grp_t[s, :n_t[s]])) for s in range(T))
    print(f"steps identical under estimated and ground-truth matrices: {same} of {T}; roots per step {n_t.min()}..{n_t.max()}")
    assert n_t.sum() > 0 and same >= 36
