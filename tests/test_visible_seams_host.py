"""The correspond_visible seam cases (tests/visible_seam_cases.py), the part that needs no GPU: every case has exactly the seed
count it is named for in pass 0, a second pass of 1 to `cap` seeds (the scratch pass is followed by an LDS pass over stale LDS
keys), a decision margin above the suite's MIN_MARGIN, and a cutoff further than that from the nearest seed distance -- so that
tests/test_gpu_visible_seams.py excuses nothing.  The LDS plan is restated from csrc/correspond_visible.hip's own constants: a
changed constant fails here, and nothing is silently tested off the seam.

Measured here (the restatement, 0.1 s a run): seed 1's cutoffs run from 6.45 to 47.75 px, seed 2's from 6.09 to 44.25; the
smallest half gap around a cutoff is 2.57e-4 px (seed 1, 1025 seeds); second passes of 11 to 30 seeds; smallest decision margin
5.68e-6 (seed 1) and 6.73e-6 (seed 2)."""
import os
import re

import numpy as np
import pytest

import correspond_visible_ref as cv
import visible_seam_cases as vs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIN_MARGIN = 1e-6  # tests/test_gpu_correspond_visible.py's (that module needs no GPU to import, but this one asks nothing of it)


def lds_plan_cap(P, C, budget, cam_w, rec_head):
    """vis_lds_plan's `cap` (csrc/correspond_visible.hip), restated"""
    pairs, rec = C * (C - 1) // 2, rec_head + ((C + 7) & ~7)
    o = C * cam_w * 8 + pairs * 72 + C * P * 16 + 32 * 4 + pairs * 2 + C * P
    o = (o + 15) & ~15
    cap = 4096
    while cap > 0 and o + cap * (rec + 2) > budget:
        cap >>= 1
    return cap, rec


def test_the_lds_plan_holds_2048_records_for_this_shape():
    csrc = os.path.join(ROOT, "mocapv2_amd", "csrc")
    with open(os.path.join(csrc, "correspond_visible.hip")) as f:
        source = f.read()
    with open(os.path.join(csrc, "correspond_dev.h")) as f:
        header = f.read()
    cam_row = int(re.search(r"constexpr int .*\bCAM_ROW = (\d+);", header).group(1))
    assert re.search(r"constexpr int oKi = CAM_ROW, CAMW = CAM_ROW \+ 9;", source)
    rec_head = int(re.search(r"constexpr int REC_HEAD = (\d+),", source).group(1))
    m = re.search(r"const int small = (\d+) \* 1024 - (\d+);", source)
    budget = int(m.group(1)) * 1024 - int(m.group(2))
    assert (cam_row + 9, rec_head, budget) == (47, 16, 65472)
    assert "int cap = 4096;" in source and "o + cap * (rec + 2) > budget" in source and "cap >= 2048) return small" in source
    cap, rec = lds_plan_cap(vs.P, vs.C, budget, cam_row + 9, rec_head)
    assert (cap, rec) == (vs.CAP, 24) == (2048, 24)
    # the sweep stands on the seam whichever power of two the plan gives
    for seam in (1024, 2048, 4096):
        assert {seam - 1, seam, seam + 1} <= set(vs.COUNTS)
    assert max(vs.COUNTS) <= vs.MAX_HYP
    scene, pts, counts, _, _ = vs.scene(1)
    assert pts.shape == (vs.C, vs.P, 2) and counts.max() <= vs.P and scene.n_cam == vs.C


def test_first_pass_distances_are_the_restatements_seeds():
    """The count of distances below a cutoff is the restatement's seed count of pass 0, at cutoffs that are no midpoints too."""
    for seed in vs.SEEDS:
        _, pts, counts, _, _ = vs.scene(seed)
        d = vs.distances(seed)
        assert (np.diff(d) >= 0).all() and np.isfinite(d).all() and len(d) > max(vs.COUNTS)
        for cut in (3.0, 10.0, 33.3):
            res = cv.correspond_visible(pts, counts, *vs.cams(), cutoff=cut, max_hyp=1 << 20, max_passes=1)
            assert res["seeds"][0] == int((d < cut).sum()), (seed, cut)
    assert all(np.array_equal(x, y) for x, y in zip(vs.cams(), cv.scene_arrays(vs.scene(2)[0])))  # one rig for every seed


@pytest.mark.parametrize("seed", vs.SEEDS)
@pytest.mark.parametrize("k", vs.COUNTS)
def test_every_count_of_the_sweep_is_its_name(seed, k):
    cut, half_gap = vs.cutoff_for(seed, k)
    res = vs.restatement(seed, k)
    print(f"seed {seed} count {k}: cutoff {cut:.4f} half gap {half_gap:.2e} seeds {res['seeds']} n {res['n']} margin {res['margin']:.2e}")
    assert half_gap > MIN_MARGIN
    assert res["seeds"][0] == k and res["n"] > 0
    assert len(res["seeds"]) >= 2 and 1 <= res["seeds"][1] <= vs.CAP
    assert res["margin"] > MIN_MARGIN
    assert 6.0 < cut < 48.0


def test_four_steps_sit_in_lds_and_scratch_side_by_side():
    pts, counts, cut = vs.four_steps()
    assert pts.shape == (4, vs.C, vs.P, 2) and cut == vs.cutoff_for(1, vs.CAP)[0]
    res = [cv.correspond_visible(pts[t], counts[t], *vs.cams(), cutoff=cut, max_hyp=vs.MAX_HYP) for t in range(4)]
    first = [r["seeds"][0] for r in res]
    print("four steps: seeds", [r["seeds"] for r in res], "n", [r["n"] for r in res], "margins", [f"{r['margin']:.2e}" for r in res])
    assert first[0] == vs.CAP                              # exactly cap: LDS
    assert first[1] == first[3] == 2203 > vs.CAP           # scratch (seed 2's own 2048 lies at 18.54 px)
    assert 0 < first[2] == 151 < vs.CAP                    # few seeds: LDS
    assert all(r["margin"] > MIN_MARGIN and r["n"] > 0 for r in res)
    d2 = vs.distances(2)
    assert min(abs(d2 - cut)) > MIN_MARGIN
    # the reversed lists are the same geometry under other keys: the same markers through other indices
    assert res[3]["n"] == res[1]["n"] and not np.array_equal(res[3]["idx"], res[1]["idx"])
    flipped = np.where(res[3]["idx"] >= 0, counts[3][None, :] - 1 - res[3]["idx"], -1)
    assert {tuple(r) for r in flipped} == {tuple(r) for r in res[1]["idx"]}


def test_max_hyp_at_the_seed_count_in_scratch():
    for k in (vs.CAP + 1, 4097):
        pts, counts, cut = vs.with_neighbour(1, k)
        at = [cv.correspond_visible(pts[t], counts[t], *vs.cams(), cutoff=cut, max_hyp=k) for t in range(2)]
        under = [cv.correspond_visible(pts[t], counts[t], *vs.cams(), cutoff=cut, max_hyp=k - 1) for t in range(2)]
        assert at[0]["seeds"][0] == k and at[0]["n"] > 0 and under[0]["n"] == cv.E_GROUPS
        assert max(at[1]["seeds"]) < k - 1 and under[1]["n"] == at[1]["n"] > 0
        assert all(r["margin"] > MIN_MARGIN for r in at + under)
    assert 4097 & 4096 and 4097 != 4096  # no power of two: the order array's offset and the scratch size differ from the padded count


def test_rows_run_out_in_a_later_pass():
    seed, k = vs.LATER_PASS
    one, three = vs.restatement(seed, k, max_passes=1), vs.restatement(seed, k, max_passes=3)
    n1, n3 = one["n"], three["n"]
    print(f"later pass: n(max_passes=1) {n1}  n(max_passes=3) {n3}  seeds {three['seeds']}")
    assert n3 > n1 > 0 and n3 - 1 >= n1          # Q = n3 - 1 fits pass 0's markers: the refusal comes from pass 2 or later
    assert three["seeds"][0] == k > vs.CAP        # ... after a pass in scratch
    pts, counts, cut = vs.with_neighbour(seed, k)
    fits = [cv.correspond_visible(pts[t], counts[t], *vs.cams(), cutoff=cut, Q=n3) for t in range(2)]
    short = [cv.correspond_visible(pts[t], counts[t], *vs.cams(), cutoff=cut, Q=n3 - 1) for t in range(2)]
    assert fits[0]["n"] == n3 and short[0]["n"] == cv.E_OUTPUT
    assert 0 < fits[1]["n"] == short[1]["n"] <= n3 - 1
    assert all(r["margin"] > MIN_MARGIN for r in fits + short)


# ---- cases beyond the sweep ---------------------------------------------------------------------------------------------------
def test_twelve_steps_pair_different_scratch_scenes_on_one_xcd():
    pts, counts, cut, order = vs.twelve_steps()
    four = vs.four_steps()
    assert len(order) == 12 and cut == four[2] and all(np.array_equal(pts[t], four[0][s]) for t, s in enumerate(order))
    in_scratch = {1, 3}  # four_steps(): asserted above to have 2203 seeds each, the other two 2048 and 151
    shared = [(t, t + 8) for t in range(4) if order[t] in in_scratch]
    assert shared == [(1, 9), (3, 11)]
    for t, u in shared:
        assert order[u] in in_scratch and order[u] != order[t]  # both in scratch at once, with other keys


def test_poison_keeps_every_seed_and_dropped_keeps_none():
    _, pts, counts, _, _ = vs.scene(1)
    cut_a, _ = vs.cutoff_for(1, vs.POISON["seeds"])
    a = cv.correspond_visible(pts, counts, *vs.cams(), cutoff=cut_a, gate=vs.POISON["gate"], max_err=vs.POISON["max_err"], max_passes=1)
    assert a["seeds"] == [4097] and a["n"] > 0 and (a["views"] != 0).all()
    assert all(bin(int(v)).count("1") == 2 for v in a["views"])   # no support: two-view hypotheses only
    # every seed is kept: the accepted ones are a maximal matching, and no seed has two free points left over
    claimed = np.zeros((vs.C, vs.P), bool)
    for row in a["idx"]:
        for c, p in enumerate(row):
            if p >= 0:
                claimed[c, p] = True
    seeds = vs.seeds_in_lane_order(pts, counts, cut_a)
    assert len(seeds) == 4097 and all(claimed[s[1], s[2]] or claimed[s[3], s[4]] for s in seeds)
    cut_b, _ = vs.cutoff_for(1, vs.DROPPED["seeds"])
    b = cv.correspond_visible(pts, counts, *vs.cams(), cutoff=cut_b, max_err=vs.DROPPED["max_err"])
    assert b["seeds"] == [vs.CAP + 1] and b["n"] == 0 and b["margin"] > MIN_MARGIN
    # the GPU test rests on the second call finding the first call's records: equal T and max_hyp ask for the same scratch size, a
    # block that is large enough stays (Buf::reserve), and the entry point neither clears the scratch nor hands out another one
    csrc = os.path.join(ROOT, "mocapv2_amd", "csrc")
    with open(os.path.join(csrc, "ctx.h")) as f:
        assert re.search(r"int reserve\(size_t count, bool zero = false\)\s*\{\s*if \(count <= n\) return 0;", f.read())
    with open(os.path.join(csrc, "abi_geom.hip")) as f:
        geom = f.read()
    entry = geom[geom.index("int mocap_correspond_visible("):]
    entry = entry[:entry.index("launch_correspond_visible(")]
    assert "const size_t need = ((size_t)T * step_bytes + 7) / 8;" in entry and "TRY(c->scratch.reserve(need));" in entry
    assert "a.scratch = (unsigned char*)(double*)c->scratch;" in entry and "emset" not in entry


def test_disjoint_seeds_one_more_than_cap_each_a_markers_only_seed():
    """C = 32, P = 128: the 64 KiB plan holds no record, so the plan takes the 160 KiB budget and holds 512.  513 markers, two views
    each: 513 seeds at the cutoff, every one accepted in the one pass as a two-view marker, every point claimed exactly once -- losing
    any one seed loses a marker.  The scene run before it on the same context shares no seed key with it.
    Measured here: the 513th distance is 4.26e-5 px, the 514th 3.14e-4, the cutoff 1.5e-4; errors up to 2.2e-10 px^2."""
    D = vs.DISJOINT
    csrc = os.path.join(ROOT, "mocapv2_amd", "csrc")
    with open(os.path.join(csrc, "correspond_visible.hip")) as f:
        source = f.read()
    with open(os.path.join(csrc, "correspond.hip")) as f:
        limit_source = f.read()
    with open(os.path.join(csrc, "correspond_dev.h")) as f:
        cam_row = int(re.search(r"constexpr int .*\bCAM_ROW = (\d+);", f.read()).group(1))
    rec_head = int(re.search(r"constexpr int REC_HEAD = (\d+),", source).group(1))
    m = re.search(r"const int small = (\d+) \* 1024 - (\d+);", source)
    small = int(m.group(1)) * 1024 - int(m.group(2))
    m = re.search(r"const int want = (\d+) \* 1024 - (\d+);", limit_source)
    large = int(m.group(1)) * 1024 - int(m.group(2))
    assert (small, large) == (65472, 163776) and "cap >= 2048) return small" in source and "return workgroup_lds_limit(LDS_USER_VISIBLE" in source
    assert lds_plan_cap(D["P"], D["C"], small, cam_row + 9, rec_head)[0] == 0       # below 2048: the plan takes the limit
    cap, rec = lds_plan_cap(D["P"], D["C"], large, cam_row + 9, rec_head)
    assert (cap, rec) == (D["cap"], 48) == (512, 48) and D["markers"] == cap + 1
    pts, counts, cams = vs.disjoint_scene(D["seed"])
    pts, counts = pts[0], counts[0]
    assert pts.shape == (D["C"], D["P"], 2) and counts.max() <= D["P"] and counts.sum() == 2 * D["markers"]
    d = cv.first_pass_distances(pts, counts, *cams)
    print(f"disjoint: distance {cap + 1} is {d[cap]:.2e}, distance {cap + 2} is {d[cap + 1]:.2e}, cutoff {D['cutoff']:.2e}")
    assert D["cutoff"] - d[cap] > MIN_MARGIN and d[cap + 1] - D["cutoff"] > MIN_MARGIN
    res = cv.correspond_visible(pts, counts, *cams, **vs.disjoint_kw())
    assert res["seeds"] == [cap + 1] and res["n"] == cap + 1
    assert all(bin(int(v)).count("1") == 2 for v in res["views"])
    claimed = np.zeros((D["C"], D["P"]), int)
    keys = set()
    for row in res["idx"]:
        (a, b) = np.flatnonzero(row >= 0)
        claimed[a, row[a]] += 1
        claimed[b, row[b]] += 1
        keys.add((int(a), int(row[a]), int(b), int(row[b])))
    assert all((claimed[c, :counts[c]] == 1).all() for c in range(D["C"]))           # every point in exactly one marker
    assert keys == vs.seed_keys(pts, counts, cams, D["cutoff"]) and len(keys) == cap + 1   # every seed is a marker's only seed
    # the other decisions lie far off: errors against max_err = 25, and no foreign point near the gate of 1e-3 px around a projection
    assert res["err"].max() < 1e-6
    c = cv.Cameras(*cams)
    nearest = np.inf
    for cam in range(D["C"]):
        u, v = c.pinhole(cam, res["xyz"])
        others = res["idx"][:, cam] < 0
        d2 = (pts[cam, :counts[cam], 0][None, :] - u[others, None]) ** 2 + (pts[cam, :counts[cam], 1][None, :] - v[others, None]) ** 2
        nearest = min(nearest, float(d2.min()))
    print(f"disjoint: nearest foreign point to a projection {np.sqrt(nearest):.3f} px")
    assert nearest - D["gate"] ** 2 > MIN_MARGIN   # (px^2; measured: the nearest lies 0.81 px off)
    other, other_counts, other_cams = vs.disjoint_scene(D["other_seed"])
    assert all(np.array_equal(x, y) for x, y in zip(cams, other_cams))
    other_keys = vs.seed_keys(other[0], other_counts[0], other_cams, D["cutoff"])
    assert len(other_keys) > cap and not (other_keys & keys)
