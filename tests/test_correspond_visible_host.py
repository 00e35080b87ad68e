"""mocap_correspond_visible, the part that needs no GPU: the NumPy restatement of the definition
(tests/correspond_visible_ref.py) against ground truth from synth.Scene, the loud failure without a GPU, the declarations, and
the code-object table of the new kernel."""
import ctypes
import importlib.util
import os
import re
import subprocess

import numpy as np
import pytest

import correspond_visible_ref as cv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Scenes: ring rigs in 1920 x 1080, markers in a 1 m cube, every view hidden with probability p, Gaussian jitter on the pixels.
# Seeds: 0..19 (camera 0 blinded: 0..4) without those in which the restatement itself does not return exactly the truth -- the
# share of seeds a test may leave out is 0.  Left out: 7 and 8 at 6 x 8 and 8 at 3 x 4, where a seed pair with a narrow
# baseline projects its two-view point within the gate of ANOTHER marker's point in a camera that does not see the marker;
# that hypothesis has one member more than the true one and is ranked first (a limit of the definition).
# worst: the restatement's worst distance to the true marker over the seeds, measured here; the test allows 1.5 times that (a
# property of the jitter, not of the code under test).
SCENES = {
    #               cameras, markers, p, jitter, seeds,                                          kw,            worst (m)
    "6x8":         (6, 8, 0.3, 0.5, [s for s in range(20) if s not in (7, 8)],                    {},            4.00e-3),
    "4x4":         (4, 4, 0.3, 0.5, list(range(20)),                                             {},            3.79e-3),
    "3x4":         (3, 4, 0.3, 0.3, [s for s in range(20) if s != 8],                             {},            2.41e-3),
    "blind0":      (4, 6, 0.2, 0.5, list(range(5)),                                              {"blind": (0,)}, 3.47e-3),
    "two_cameras": (2, 4, 0.0, 0.5, list(range(20)),                                             {},            5.08e-3),
}


@pytest.mark.parametrize("name", sorted(SCENES))
def test_restatement_finds_every_marker_with_two_views_and_nothing_else(name):
    C, M, p, jitter, seeds, kw, worst_measured = SCENES[name]
    total, worst = 0, 0.0
    for seed in seeds:
        scene, pts, counts, truth, markers = cv.scene_case(C, M, p, seed, jitter=jitter, **kw)
        res = cv.correspond_visible(pts, counts, *cv.scene_arrays(scene))
        missed, ghosts, w = cv.check_against_truth(res, truth, markers)
        assert not missed and not ghosts, (name, seed, missed, ghosts)
        assert res["n"] == sum((row >= 0).sum() >= 2 for row in truth)
        assert res["margin"] > 0
        if kw.get("blind"):
            assert (res["idx"][:, 0] == -1).all() and res["n"] > 0
        total += res["n"]
        worst = max(worst, w)
    print(f"{name}: {total} markers over {len(seeds)} seeds, worst distance to truth {worst * 1e3:.3f} mm")
    assert total > 0 and worst <= 1.5 * worst_measured


def test_false_blobs_make_no_ghost_with_three_views():
    """Two false blobs per camera: min_views = 2 must produce ghost points (two random points are often within the cutoff of
    each other's epipolar line), min_views = 3 none -- and no marker with three views is lost."""
    ghosts2 = 0
    for seed in [s for s in range(20) if s not in (7, 8)]:
        scene, pts, counts, truth, markers = cv.scene_case(6, 8, 0.3, seed, false_blobs=2)
        cams = cv.scene_arrays(scene)
        res = cv.correspond_visible(pts, counts, *cams, min_views=3)
        missed, ghosts, _ = cv.check_against_truth(res, truth, markers, min_views=3)
        assert not ghosts and not missed, (seed, missed, ghosts)
        assert (np.array([bin(int(v)).count("1") for v in res["views"]]) >= 3).all()
        ghosts2 += len(cv.check_against_truth(cv.correspond_visible(pts, counts, *cams), truth, markers)[1])
    assert ghosts2 > 0


def test_pair_matrices_are_the_fundamental_matrices_of_the_poses():
    from mocapv2_amd import calibrate, synth
    sc = synth.MixedScene(5)
    K, R, t = np.stack(sc.Ks), np.stack([p["R"] for p in sc.poses]), np.stack([p["t"] for p in sc.poses])
    cams = cv.Cameras(K, np.zeros((5, 5)), R, t)
    assert cams.pairs[:5] == [(0, 1), (0, 2), (0, 3), (0, 4), (1, 2)] and len(cams.pairs) == 10
    for (a, b), F in zip(cams.pairs, cams.F):
        want = synth.fundamental_from_poses(sc.poses[a], sc.poses[b], sc.Ks[a], sc.Ks[b])
        assert np.allclose(F.reshape(3, 3), want, rtol=0, atol=1e-12 * np.abs(want).max())
        assert np.allclose(want, calibrate.poses_to_fundamental_matrix(sc.poses[a], sc.poses[b], sc.Ks[a], sc.Ks[b]), rtol=0,
                           atol=1e-12 * np.abs(want).max())


def test_restatement_shares_its_helpers_results_with_numpy():
    """smallest_eigvec4 against np.linalg.eigh; the undistortion against calibrate.undistort_points, bit for bit."""
    from mocapv2_amd import calibrate, synth
    rng = np.random.default_rng(0)
    A = rng.normal(size=(50, 6, 4))
    B = np.einsum("nij,nik->njk", A, A)
    v = cv.smallest_eigvec4(B)
    for n in range(50):
        ref = np.linalg.eigh(B[n])[1][:, 0]
        assert min(np.abs(v[n] - ref).max(), np.abs(v[n] + ref).max()) < 1e-12
    K = synth.intrinsics(1920, 1080)
    pts = rng.uniform((0, 0), (1920, 1080), (100, 2))
    assert np.array_equal(cv.undistort_points(pts, K, synth.MILD_DIST), calibrate.undistort_points(pts, K, synth.MILD_DIST))


def test_restatement_reports_its_capacities():
    scene, pts, counts, truth, markers = cv.scene_case(4, 5, 0.0, 0)
    cams = cv.scene_arrays(scene)
    good = cv.correspond_visible(pts, counts, *cams)
    assert good["n"] == 5
    over, neg = counts.copy(), counts.copy()
    over[1], neg[2] = 6, -2
    assert cv.correspond_visible(pts, over, *cams)["n"] == cv.E_TRUNCATED
    assert cv.correspond_visible(pts, neg, *cams)["n"] == cv.E_BLOB
    most = max(good["seeds"])
    assert cv.correspond_visible(pts, counts, *cams, max_hyp=most)["n"] == 5
    assert cv.correspond_visible(pts, counts, *cams, max_hyp=most - 1)["n"] == cv.E_GROUPS
    assert cv.correspond_visible(pts, counts, *cams, Q=5)["n"] == 5
    assert cv.correspond_visible(pts, counts, *cams, Q=4)["n"] == cv.E_OUTPUT


def test_without_a_gpu_the_call_fails_loudly():
    """No CPU fallback: without a GPU the Python surface raises and the C entry point returns an error with a text."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from mocapv2_amd import _abi
    from mocapv2_amd.pipeline import BatchTracker
    from mocapv2_amd.synth import Scene
    sc = Scene(3, 320, 192)
    K, dist, R, t = cv.scene_arrays(sc)
    with pytest.raises(RuntimeError):
        BatchTracker(K, dist, R, t, None, 320, 192, 2, visibility="any")
    lib = _abi.load()
    rc = lib.mocap_correspond_visible(None, None, 0, 0, None, 0, 0, 1, 1, 2, 1, 0, 10.0, 10.0, 2, 25.0, 3, 8192, 1, None, None, None,
                                      None, None, None)
    assert rc == -1 and lib.mocap_last_error()


def test_abi_declares_the_entry_point_and_its_status_code():
    from mocapv2_amd import _abi, pipeline
    assert _abi.ABI_VERSION == 7 and len(_abi.SIGNATURES["mocap_correspond_visible"]) == 25
    header = open(os.path.join(ROOT, "include", "mocap_hip.h")).read()
    assert "MOCAP_CORR_E_OUTPUT = -5" in header and "#define MOCAP_ABI_VERSION 7" in header
    assert header.index("MOCAP_CORR_E_BLOB = -4") < header.index("MOCAP_CORR_E_OUTPUT = -5") < header.index("MOCAP_FUND_E_SAMPLE")
    assert "MOCAP_CORR_E_OUTPUT" in pipeline.VIS_STATUS[-5] and "MOCAP_CORR_E_OUTPUT" in pipeline.CORR_STATUS[-5]
    assert str(pipeline.CapacityError(3, -5, pipeline.VIS_STATUS)).startswith("time step 3: more markers accepted")
    assert ctypes.sizeof(ctypes.c_int) == 4


def test_new_kernel_uses_no_scratch_memory_and_spills_nothing():
    """The compiler's own metadata for correspond_visible.hip (scratch/kernel_meta.py, no GPU needed): 0 bytes of scratch and 0
    spilled VGPRs, as for every geometry kernel -- and the seven kernels that were geom.hip's (correspond.hip, geom_batch.hip,
    ba_residuals.hip: exactly those seven) keep theirs with the helpers in geom_dev.h."""
    spec = importlib.util.spec_from_file_location("kernel_meta", os.path.join(ROOT, "scratch", "kernel_meta.py"))
    km = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(km)
    ks = km.kernels_of(os.path.join(km.CSRC, "correspond_visible.hip"))
    assert len(ks) == 2 and all("correspond_visible_kernel" in k["name"] for k in ks)  # the float64 and the int32 points
    geom = [k for f in ("correspond.hip", "geom_batch.hip", "ba_residuals.hip") for k in km.kernels_of(os.path.join(km.CSRC, f))]
    plain = subprocess.run([km.FILT], input="\n".join(k["name"] for k in geom), capture_output=True, text=True, check=True).stdout.split("\n")
    short = sorted(re.sub(r"^void |mocap::|\(.*\)$", "", nm) for nm in plain if nm)
    assert short == ["ba_residuals_kernel", "correspond_kernel<double>", "correspond_kernel<int>", "epipolar_scores_kernel<double>",
                     "epipolar_scores_kernel<int>", "reproject_kernel", "triangulate_kernel"], short
    for k in ks + geom:
        print(k)
        assert k["scratch"] == 0 and k["spill"] == 0, k
