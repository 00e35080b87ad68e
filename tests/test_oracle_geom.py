"""The geometry oracle (oracle/geom_oracle.c) against the fixtures produced by the reference itself."""
import glob
import os

import numpy as np
import pytest

import oracle

TOL_XYZ = 1e-7  # world units (= 1e-4 mm), the bar of BASELINE.json


def load(golden_dir, name):
    return np.load(os.path.join(golden_dir, name + ".npz"), allow_pickle=False)


def test_k1_bundled_dlt(golden_dir):
    g = load(golden_dir, "k1_bundled")
    ident = [0, 1]
    out = np.array([oracle.triangulate(p, ident, ident, g["K"], g["R"], g["t"]) for p in g["image_points"]])
    assert np.abs(out - g["objects_json"]).max() < TOL_XYZ
    assert np.abs(out - g["objects_ref"]).max() < 1e-10


def test_k2_epipolar_distances(golden_dir):
    g = load(golden_dir, "k1_bundled")
    d = []
    for p0, p1 in g["image_points"]:
        line = oracle.epiline(g["F"][0], p0[0], p0[1])
        d.append(oracle.epi_distance(line, p1[0], p1[1]))
    d = np.array(d)
    assert np.array_equal(d, g["epi_dist"])  # same float32 line, same FP64 expression: bit-exact
    assert d.max() < 10.0


def test_reprojection_mse_54(golden_dir):
    g = load(golden_dir, "k1_bundled")
    ident = [0, 1]
    for p, X, e in zip(g["image_points"], g["objects_ref"], g["reproj_mse"]):
        got = oracle.reproj_mse(p, ident, ident, X, g["K"], g["dist"], g["R"], g["t"])
        assert abs(got - e) <= 1e-9 * max(1.0, abs(e))


def test_triangulate_point_with_none(golden_dir):
    g = load(golden_dir, "tri_none")
    for grp, exp in zip(g["groups"], g["out"]):
        valid = ~np.isnan(grp[:, 0])
        pose_idx = np.nonzero(valid)[0]
        k_idx = np.arange(len(pose_idx))  # reference quirk: intrinsics by position after removal
        got = oracle.triangulate(grp[valid], pose_idx, k_idx, g["K"], g["R"], g["t"])
        if np.isnan(exp[0]):
            assert got is None
        else:
            assert np.abs(got - exp).max() < TOL_XYZ


@pytest.mark.parametrize("path", sorted(glob.glob(os.path.join(os.path.dirname(__file__), "golden", "corr_*.npz"))),
                         ids=lambda p: os.path.basename(p)[:-4])
def test_correspondence_cases(path):
    g = np.load(path)
    res = oracle.correspond(g["pts"], g["counts"], g["K"], g["dist"], g["R"], g["t"], g["F"])
    obj, img = oracle.select_objects(res, int(g["obj_count"]))
    exp_obj, exp_img = g["out_obj"], g["out_img"]
    if exp_obj.shape == (0,):
        assert len(obj) == 0 and len(img) == 0
        return
    assert obj.shape == exp_obj.shape and img.shape == exp_img.shape
    assert np.array_equal(img, exp_img)          # marker indices / image points bit-exact
    assert np.abs(obj - exp_obj).max() < TOL_XYZ  # 3-D points within 1e-4 mm


def test_ba_residuals(golden_dir):
    g = load(golden_dir, "ba_residuals")
    ip = g["image_points"]
    valid = np.ones(ip.shape[:2], np.uint8)
    for x, r in zip(g["params"], g["residuals"]):
        got = oracle.ba_residuals(x, 2, ip, valid, g["K"], g["dist"])
        assert got.dtype == np.float32 and got.shape == r.shape
        assert np.allclose(got, r, rtol=2e-5, atol=1e-6)


def test_none_entries_on_unequal_cameras(golden_dir):
    """reproj_none_mixed: triangulate_point and calculate_reprojection_error with [None, None] entries on four cameras that
    differ in K and lens; both take the intrinsics by position after the entries are dropped (lib/Helpers.py:59-61,
    :137-138).  The last assertion shows that the fixture tells the two indexings apart."""
    g = load(golden_dir, "reproj_none_mixed")
    seen = 0
    for grp, exp, X, mse in zip(g["groups"], g["out"], g["obj"], g["mse"]):
        valid = ~np.isnan(grp[:, 0])
        pose_idx = np.nonzero(valid)[0]
        k_idx = np.arange(len(pose_idx))
        got = oracle.triangulate(grp[valid], pose_idx, k_idx, g["K"], g["R"], g["t"])
        e = oracle.reproj_mse(grp[valid], pose_idx, k_idx, X, g["K"], g["dist"], g["R"], g["t"])
        if np.isnan(exp[0]):
            assert got is None and e is None and np.isnan(mse)
            continue
        assert np.abs(got - exp).max() < TOL_XYZ
        assert abs(e - mse) <= 1e-9 * max(1.0, abs(mse))
        if not np.array_equal(pose_idx, k_idx):  # by camera number instead: far off
            wrong = oracle.reproj_mse(grp[valid], pose_idx, pose_idx, X, g["K"], g["dist"], g["R"], g["t"])
            assert abs(wrong - mse) > 1e-3 * mse
            seen += 1
    assert seen == 3


def test_ba_residuals_on_two_unequal_cameras_with_holes(golden_dir):
    g = load(golden_dir, "ba_residuals_mixed")
    ip, valid = np.nan_to_num(g["image_points"]), g["valid"]
    assert ip.shape == (600, 2, 2) and not valid.all(1)[:256].all() and not valid.all(1)[256:512].all() and not valid.all(1)[512:].all()
    assert not np.array_equal(g["K"][0], g["K"][1]) and not np.array_equal(g["dist"][0], g["dist"][1])
    assert (g["params"][2][:3] == 0).all()  # the small-angle branch of Rotation.from_rotvec
    for x, r in zip(g["params"], g["residuals"]):
        got = oracle.ba_residuals(x, 2, ip, valid, g["K"], g["dist"])
        assert got.dtype == np.float32 and got.shape == r.shape and len(r) < valid.all(1).sum()
        assert np.allclose(got, r, rtol=2e-5, atol=1e-6)
        swapped = oracle.ba_residuals(x, 2, ip, valid, g["K"][::-1], g["dist"][::-1])  # the cameras' intrinsics exchanged: far off
        assert not np.allclose(swapped, r, rtol=1e-2, atol=1e-6)


def test_numpy_pairwise_mean():
    rng = np.random.default_rng(0)
    for n in [1, 2, 7, 8, 9, 12, 127, 128, 129, 300, 1000, 4097]:
        a = rng.uniform(0, 100, n)
        assert oracle.np_mean(a) == a.mean()
