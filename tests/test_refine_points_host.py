"""mocap_refine_points, the part that needs no GPU: the NumPy restatement of the definition (tests/refine_points_ref.py) on the
scenes in which correspond_visible's definition is known to miss, on a rig of cameras at unequal distances (accuracy and
covariance), on raw pixels of unequal lenses, through every status and stop an input can reach; the loud failure without a
GPU, the declarations, and the code-object table of the new kernels."""
import importlib.util
import os

import numpy as np
import pytest

import lm_ref
import mixed_rig
import refine_points_cases as cases
import refine_points_ref as rp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pruning_turns_the_wrong_member_rows_into_true_rows_and_touches_no_other():
    """Scenes 6 x 8, 4 x 4 (jitter 0.5 px) and 3 x 4 (0.3 px), p_hide 0.3, seeds 0..19 through correspond_visible and then the
    refinement with pruning at 36 sigma^2 (refine_points_cases.prune_limit: 9 px^2 and 3.24 px^2), one drop per row at most."""
    rows, subsets, became_true, ghosts = 0, 0, [], []
    for name, (C, M, jitter) in cases.WRONG_MEMBER_SCENES.items():
        for seed in range(20):
            cams, pts, truth, res = cases.wrong_member_case(name, seed)
            n = res["n"]
            out = rp.refine_points(res["xyz"][None], [n], res["views"][None], *cams, pts=pts[None], idx=res["idx"][None],
                                   max_res2=cases.prune_limit(jitter), max_drop=1)
            assert (out["status"][0, :n] > 0).all()
            for q in range(n):
                before = tuple(int(v) for v in res["idx"][q])
                left = int(out["views"][0, q])
                after = tuple(p if left >> c & 1 else -1 for c, p in enumerate(before))
                assert left | int(out["dropped"][0, q]) == int(res["views"][q]) and not left & int(out["dropped"][0, q])
                kb, ka = cases.row_kind(before, truth), cases.row_kind(after, truth)
                rows += 1
                subsets += ka == "subset"
                if kb == "true":
                    assert after == before, (name, seed, q, before, after)  # a row that was exactly true has not changed
                if kb == "wrong" and ka == "true":
                    became_true.append((name, seed))
                if ka == "wrong":
                    ghosts.append((name, seed, sum(p >= 0 for p in after), np.sort(out["res2"][0, q][out["res2"][0, q] >= 0])))
    print(f"{rows} rows, {subsets} strict subsets of a true row, wrong -> true: {became_true}, still wrong: {ghosts}")
    assert rows == 304
    assert became_true == [("6x8", 7), ("6x8", 8)]
    # no row has a member that is not its marker's, but for the two-view row of 3 x 4 seed 8 -- which min_views = 2 protects,
    # and whose residuals (12.4 and 14.6 px^2 at a jitter of 0.3 px) a caller can now see
    assert [g[:3] for g in ghosts] == [("3x4", 8, 2)] and (ghosts[0][3] > cases.prune_limit(0.3)).all()
    assert subsets == 2  # the two true markers that lost a point to the wrong-member rows


def test_refined_points_lie_closer_to_the_truth_than_the_dlt_on_cameras_at_unequal_distances():
    s, rows = cases.uneven_scene(), cases.uneven_refined()
    assert all(r["status"] > 0 for r in rows)
    Xr = np.stack([r["xyz"] for r in rows])
    rms_dlt = np.sqrt((np.linalg.norm(s["X0"] - s["truth"], axis=1) ** 2).mean())
    rms_ref = np.sqrt((np.linalg.norm(Xr - s["truth"], axis=1) ** 2).mean())
    iters = np.bincount([r["iters"] for r in rows])
    print(f"rms distance to truth: DLT {rms_dlt * 1e3:.4f} mm, refined {rms_ref * 1e3:.4f} mm, ratio {rms_dlt / rms_ref:.4f}; iterations {iters}")
    assert rms_ref < rms_dlt
    # the rule only accepts decreases: exact
    assert all((np.diff(r["history"][:, 0]) <= 0).all() and r["history"][0, 0] <= r["cost0"] for r in rows)
    assert all(r["err"] == (2.0 * r["history"][-1, 0]) / 12.0 for r in rows)  # err is the cost of the last state: sum r^2 / (2 m)


def test_covariance_is_the_refined_points_scatter():
    """Mean normalised estimation error squared e^T (sigma^2 cov)^-1 e over the 2000 rows: 3 expected, standard error
    sqrt(6 / 2000) = 0.055"""
    s, rows = cases.uneven_scene(), cases.uneven_refined()
    cov = np.stack([r["cov"] for r in rows])
    full = np.zeros((len(rows), 3, 3))
    for k, (a, b) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
        full[:, a, b] = full[:, b, a] = cov[:, k]
    e = np.stack([r["xyz"] for r in rows]) - s["truth"]
    nees = np.einsum("ni,nij,nj->n", e, np.linalg.inv(full * s["sigma"] ** 2), e)
    print(f"mean NEES {nees.mean():.4f}")
    assert abs(nees.mean() - 3.0) < 0.3


def test_raw_pixels_are_matched_through_each_cameras_own_lens():
    """distorted = 1 on a MixedScene: noiseless raw-frame pixels leave no residual at the true point, and camera 0's lens in
    every camera's place moves the refined point -- by 0.087 to 1.7 mm over these markers, where the right lenses return the truth
    to 1e-16 m.  The limit of 1e-6 m lies far above the one and far below the other."""
    sc = mixed_rig.MixedScene(5)
    K, dist, R, t, _ = mixed_rig.arrays(sc)
    mk = sc.markers(np.random.default_rng(3), 12)
    raw = np.stack([sc.pixels(mk, c, distorted=True) for c in range(5)])
    right, wrong = rp.Rig(K, dist, R, t, 1), rp.Rig(K, np.stack([dist[0]] * 5), R, t, 1)
    at_truth = max(np.sqrt(rp.members_pass(right, np.arange(5), raw[:, m], mk[m])["res2"].max()) for m in range(12))
    stay = [np.linalg.norm(rp.refine_row(right, mk[m], 31, lambda c: raw[c, m])["xyz"] - mk[m]) for m in range(12)]
    move = [np.linalg.norm(rp.refine_row(wrong, mk[m], 31, lambda c: raw[c, m])["xyz"] - mk[m]) for m in range(12)]
    print(f"residual at the truth {at_truth:.3g} px; right lenses move the truth by <= {max(stay):.3g} m, camera 0's by {min(move):.3g} .. {max(move):.3g} m")
    assert at_truth < 1e-9
    assert max(stay) < 1e-12 and min(move) > 1e-6
    # and distorted = 0 is the exact pinhole: the same bits as fx x + cx
    flat = rp.Rig(K, dist, R, t, 0)
    ideal = np.stack([sc.pixels(mk, c, distorted=False) for c in range(5)])
    e = rp.members_pass(flat, np.arange(5), ideal[:, 0], mk[0])
    q = [(R[:, i, 0] * mk[0][0] + R[:, i, 1] * mk[0][1]) + R[:, i, 2] * mk[0][2] for i in range(3)]
    pz = q[2] + t[:, 2]
    u = K[:, 0, 0] * ((q[0] + t[:, 0]) / pz) + K[:, 0, 2]
    v = K[:, 1, 1] * ((q[1] + t[:, 1]) / pz) + K[:, 1, 2]
    assert np.array_equal(e["res2"], (u - ideal[:, 0, 0]) * (u - ideal[:, 0, 0]) + (v - ideal[:, 0, 1]) * (v - ideal[:, 0, 1]))


def test_every_status_and_stop_an_input_reaches():
    c = cases.status_case()
    out = rp.refine_points(c["xyz"], c["n"], c["views"], *c["cams"], pts=c["pts"], idx=c["idx"], out=rp.empty_out(1, 12, 6, canary=0xA5))
    assert {q: int(s) for q, s in enumerate(out["status"][0])} == c["want"]
    for q, s in c["want"].items():
        if s < 0:  # an error row: the point and the mask handed in (its other outputs are unspecified)
            assert np.array_equal(out["xyz"][0, q], c["xyz"][0, q], equal_nan=True) and out["views"][0, q] == c["views"][0, q]
        else:
            assert np.linalg.norm(out["xyz"][0, q] - c["markers"][2 if q == 11 else q % 8]) < 5e-3 and out["views"][0, q] == c["views"][0, q]
            assert ((out["res2"][0, q] >= 0) == [bool(int(c["views"][0, q]) >> k & 1) for k in range(6)]).all()
    assert out["iters"][0, 1] >= 2 and out["iters"][0, 9] >= 2
    # the stops, on row 0's marker
    rig = rp.Rig(*c["cams"], 0)
    obs = lambda k: c["pts"][0, k, c["idx"][0, 0, k]]
    X = c["markers"][0]
    one = rp.refine_row(rig, X + 0.01, 63, obs, max_iters=1)
    assert (one["status"], one["iters"]) == (lm_ref.STOP_MAX_ITERS, 1) and one["history"][0, 2] == 1.0
    ftol = rp.refine_row(rig, X + 0.01, 63, obs)
    assert ftol["status"] == lm_ref.STOP_FTOL and ftol["history"][:, 2].all() and 2 <= ftol["iters"] < 10
    # rejected steps: at the largest damping the call takes, the step is too short to lower the cost in FP64 ...
    lam = rp.refine_row(rig, X + 0.01, 63, obs, lambda0=1e16)
    assert (lam["status"], lam["iters"]) == (lm_ref.STOP_LAMBDA, 1) and lam["history"][0, 2] == 0.0 and np.array_equal(lam["xyz"], X + 0.01)
    # ... and at the rounding floor behind six accepted ones (row 11 of the case, from Gauss-Newton's damping): rejected to the end
    near = rp.refine_row(rig, c["xyz"][0, 11], 63, lambda k: c["pts"][0, k, c["idx"][0, 11, k]], lambda0=1e-12)
    acc = near["history"][:, 2]
    print("accepted flags of the start beside camera 0:", acc.astype(int))
    assert near["status"] == lm_ref.STOP_MAX_ITERS and acc[0] == 1.0 and acc[-1] == 0.0 and 0 < acc.sum() < 10
    # a determinant that is not finite, twice: focal lengths of 1e110 px put the determinant at 1e660
    K = np.array(c["cams"][0]).copy()
    K[:, 0, 0] = K[:, 1, 1] = 1e110
    big = rp.refine_row(rp.Rig(K, *c["cams"][1:], 0), X + 0.01, 63, obs)
    assert (big["status"], big["iters"]) == (lm_ref.STOP_CHOLESKY, 2) and np.array_equal(big["xyz"], X + 0.01)
    # pruning's limits: nothing goes with max_drop = 0 or with min_views at the members' number
    cams, pts, truth, res = cases.wrong_member_case("6x8", 7)
    kw = dict(pts=pts[None], idx=res["idx"][None], max_res2=cases.prune_limit(0.5))
    for extra in (dict(max_drop=0), dict(max_drop=1, min_views=6)):
        kept = rp.refine_points(res["xyz"][None], [res["n"]], res["views"][None], *cams, **kw, **extra)
        assert kept["dropped"][0, 0] == 0 and kept["views"][0, 0] == 63
    two = rp.refine_points(res["xyz"][None], [res["n"]], res["views"][None], *cams, **kw, max_drop=2)
    one_drop = rp.refine_points(res["xyz"][None], [res["n"]], res["views"][None], *cams, **kw, max_drop=1)
    assert not rp.specified_equal(two, one_drop) and one_drop["dropped"][0, 0] == 2  # a second drop finds nothing above the limit


def test_without_a_gpu_the_call_fails_loudly():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from mocapv2_amd import _abi
    from mocapv2_amd.engine import MocapContext
    from mocapv2_amd.pipeline import BatchTracker
    assert callable(MocapContext.refine_points)
    with pytest.raises(RuntimeError):
        MocapContext(64, 64)
    c = cases.status_case()
    K, dist, R, t = c["cams"]
    with pytest.raises(RuntimeError):
        BatchTracker(K, dist, R, t, None, 320, 192, 2, visibility="any", refine={})
    with pytest.raises(ValueError):
        BatchTracker(K, dist, R, t, None, 320, 192, 2, visibility="any", refine={"gate": 1.0})
    with pytest.raises(ValueError):
        BatchTracker(K, dist, R, t, None, 320, 192, 2, visibility="any", refine={"max_drop": 1})
    lib = _abi.load()
    args = [None] * 4 + [1, 1, 2, None, 0, 0, 1, 1, None, None, 0, 10, 1e-9, 1e-3, 0.0, 2, 0] + [None] * 9
    assert lib.mocap_refine_points(*args) == -1 and lib.mocap_last_error()


def test_abi_declares_the_entry_point_and_its_status_codes():
    from mocapv2_amd import _abi
    assert _abi.ABI_VERSION == 7 and len(_abi.SIGNATURES["mocap_refine_points"]) == 30
    header = open(os.path.join(ROOT, "include", "mocap_hip.h")).read()
    assert "#define MOCAP_ABI_VERSION 7" in header
    for name, code in (("VIEWS", rp.E_VIEWS), ("INPUT", rp.E_INPUT), ("BEHIND", rp.E_BEHIND)):
        assert f"MOCAP_REFINE_E_{name} = {code}," in header
    kernels = open(os.path.join(ROOT, "mocapv2_amd", "csrc", "kernels.h")).read()
    assert "REFINE_ERR_VIEWS = -2, REFINE_ERR_INPUT = -3, REFINE_ERR_BEHIND = -4" in kernels


def test_new_kernels_use_no_scratch_memory_and_spill_nothing():
    """The compiler's own metadata for refine_points.hip (scratch/kernel_meta.py, no GPU needed), as for every geometry kernel:
    nothing in registers is indexed by a camera number"""
    spec = importlib.util.spec_from_file_location("kernel_meta", os.path.join(ROOT, "scratch", "kernel_meta.py"))
    km = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(km)
    ks = km.kernels_of(os.path.join(km.CSRC, "refine_points.hip"))
    assert len(ks) == 3 and all("refine_points_kernel" in k["name"] for k in ks)  # float64 points, int32 points, groups
    for k in ks:
        print(k)
        assert k["scratch"] == 0 and k["spill"] == 0, k
