"""Fundamental-matrix RANSAC, the part that needs no GPU: the NumPy restatement of the definition
(tests/fundamental_ref.py) against the reference's own cv2 result on its own data, the host-side sample table and argument
checks, the loud failure without a GPU, and the code-object table of the new kernels."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest

import fundamental_ref as fr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- C1: the restatement against cv2's matrix on the bundled capture ---------------------------------------------------
def test_restatement_explains_the_bundled_points_at_least_as_well_as_cv2():
    """tests/golden/jsons/fundamentals.json[0] is what cv.findFundamentalMat returned on image_points.json (reference
    CalculateCameraPoses.py:189): all 54 points within the threshold of 10, RMS of sqrt(e_i) 3.738 px.  The restatement with
    sample_table(54, 1000, 0) finds a 54-inlier winner (hypothesis 28, the first of 14 tied ones) and its refit -- the
    8-point fit over all points -- has RMS 2.451 px.  (The winning minimal sample alone: 3.064; only the refit is held to
    cv2's figure.)"""
    a, b = fr.bundled_pair()
    F_cv = fr.bundled_cv2_fundamental()
    e_cv = fr.errors(F_cv, a, b)
    assert len(a) == 54 and (e_cv <= 100.0).all()
    rms_cv = fr.rms_distance(F_cv, a, b)
    assert abs(rms_cv - 3.738) < 1e-3
    from mocapv2_amd.calibrate import sample_table
    r = fr.ransac(a, b, sample_table(54, 1000, 0), 10.0)
    rms_refit = fr.rms_distance(r["F_refit"], a, b)
    print(f"bundled: winner {r['best']} inliers {r['n_inliers']} tied {(r['counts'] == 54).sum()} rms cv2 {rms_cv:.4f} "
          f"refit {rms_refit:.4f} sample {fr.rms_distance(r['F_sample'], a, b):.4f}")
    assert r["n_inliers"] == 54 and r["mask"].all()
    assert r["best"] == 28 and (r["counts"] == 54).sum() == 14 and r["counts"][:28].max() < 54
    assert rms_refit <= 3.738
    # a unit-norm rank-2 matrix
    assert abs(np.linalg.norm(r["F_refit"]) - 1) < 1e-12 and abs(np.linalg.det(r["F_refit"])) < 1e-12


@pytest.mark.parametrize("name,best,n,tied", [("s13", 528, 241, 2), ("s14", 0, 54, 55)])
def test_restatement_takes_the_lowest_index_among_tied_winners(name, best, n, tied):
    a, b, S, thr, _ = fr.small_case(name)
    r = fr.ransac(a, b, S, thr)
    assert (r["best"], r["n_inliers"], int((r["counts"] == n).sum())) == (best, n, tied)
    assert r["banded"].sum() == 0


def test_restatement_reports_a_degenerate_pair():
    a = np.full((20, 2), 7.0)
    from mocapv2_amd.calibrate import sample_table
    r = fr.ransac(a, a, sample_table(20, 16, 0), 3.0)
    assert r["best"] == -1 and r["F_sample"] is None and not r["mask"].any()


# ---- C2: host logic ---------------------------------------------------------------------------------------------------
def test_sample_table_is_deterministic_in_range_and_distinct():
    from mocapv2_amd.calibrate import sample_table
    for n, H, seed in [(8, 50, 0), (9, 200, 3), (54, 1000, 0), (20000, 2048, 41)]:
        S = sample_table(n, H, seed)
        assert S.dtype == np.int32 and S.shape == (H, 8) and S.flags["C_CONTIGUOUS"]
        assert S.min() >= 0 and S.max() < n
        assert (np.diff(np.sort(S, axis=1), axis=1) > 0).all()
        assert np.array_equal(S, sample_table(n, H, seed))
    assert not np.array_equal(sample_table(54, 100, 0), sample_table(54, 100, 1))
    # rows without a repeated index are the generator's first draw, untouched
    first = np.random.default_rng(5).integers(0, 100, (64, 8))
    keep = (np.diff(np.sort(first, axis=1), axis=1) > 0).all(axis=1)
    assert keep.any() and np.array_equal(sample_table(100, 64, 5)[keep], first[keep])
    with pytest.raises(ValueError):
        sample_table(7, 10, 0)
    with pytest.raises(ValueError):
        sample_table(20, 0, 0)


def test_find_fundamental_matrix_checks_its_arguments():
    from mocapv2_amd import calibrate as cal
    good = np.arange(40, dtype=float).reshape(20, 2)
    for p1, p2, kw in [(good[:7], good[:7], {}),                  # fewer than 8 points
                       (good, good[:19], {}),                     # lists of different length
                       (good.reshape(10, 4), good.reshape(10, 4), {}),
                       (good, good, {"hypotheses": 0}),
                       (good, good, {"threshold": 0.0}),
                       (good, good, {"threshold": float("nan")}),
                       (good, np.where(np.arange(40).reshape(20, 2) == 3, np.nan, good), {})]:
        with pytest.raises(ValueError):
            cal.find_fundamental_matrix(p1, p2, **kw)
    with pytest.raises(ValueError):
        cal.find_fundamental_matrices(np.zeros((3, 20, 2)), [(0, 3)])
    with pytest.raises(ValueError):
        cal.find_fundamental_matrices(np.zeros((3, 20, 2)), [(1, 1)])


def test_without_a_gpu_the_call_fails_loudly():
    """No CPU fallback: without a GPU the Python surface raises and the C entry point returns an error with a text."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from mocapv2_amd import _abi, calibrate as cal
    a, b = fr.bundled_pair()
    with pytest.raises(RuntimeError):
        cal.find_fundamental_matrix(a, b)
    with pytest.raises(RuntimeError):
        cal.tracker_fundamentals(np.stack([a, b]))
    lib = _abi.load()
    rc = lib.mocap_fundamental_ransac(None, 1, None, None, None, None, 1, 3.0, 1, None, None, None, None, None, None)
    assert rc == -1 and lib.mocap_last_error()


def test_abi_declares_the_entry_point_and_its_status_codes():
    from mocapv2_amd import _abi
    assert _abi.ABI_VERSION == 7 and len(_abi.SIGNATURES["mocap_fundamental_ransac"]) == 15
    header = open(os.path.join(ROOT, "include", "mocap_hip.h")).read()
    assert "MOCAP_FUND_E_SAMPLE = -2" in header and "MOCAP_FUND_E_DEGENERATE = -3" in header
    assert "#define MOCAP_ABI_VERSION 7" in header
    assert ctypes.sizeof(ctypes.c_int) == 4


def test_new_kernels_use_no_scratch_memory_and_spill_nothing():
    """The compiler's own metadata for fundamental.hip (scratch/kernel_meta.py, no GPU needed): 0 bytes of scratch and 0
    spilled VGPRs for every kernel, as profiles/r04_code_objects.md records for geom.hip."""
    spec = importlib.util.spec_from_file_location("kernel_meta", os.path.join(ROOT, "scratch", "kernel_meta.py"))
    km = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(km)
    ks = km.kernels_of(os.path.join(km.CSRC, "fundamental.hip"))
    names = " ".join(k["name"] for k in ks)
    for want in ("fund_hypotheses_kernel", "fund_score_kernel", "fund_select_kernel", "fund_mask_kernel", "fund_refit_kernel"):
        assert want in names
    for k in ks:
        print(k)
        assert k["scratch"] == 0 and k["spill"] == 0, k
