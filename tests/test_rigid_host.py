"""The rigid-body definition (tests/rigid_ref.py) on the CPU: what it promises on a noisy scene with hidden
markers and clutter, its exact ties and its capacity, the wire message, the kernel's compiler metadata, and the Python surface's
refusals.

Scene: rigid_ref.rigid_scene -- three bodies of 4, 5 and 6 markers (every two pairwise distances of a body more than 3 tol apart)
on random poses in a 2 m cube, each marker hidden with p = 0.2, 4 clutter points, 0.5 mm Gaussian noise per axis, rows shuffled,
T = 60; tol = 3 mm, gate = 6 mm, min_markers = 3.  Measured with the restatement over seeds 0 and 1 (325 bodies with at least
three visible markers): no wrong label, no lost body, no pose for a body with fewer than three visible markers; the worst pose
against truth is 0.04357 rad (2.5 degrees, a body of which three markers 6 to 9 cm apart are seen) and 1.873 mm in translation.
The bounds below are twice those: the noise draw is fixed by the seed, the margin only absorbs later edits to the scene."""
import importlib.util
import os
import re

import numpy as np
import pytest

import rigid_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEASURED_ANGLE, MEASURED_TRANSLATION = 0.04357, 0.001873  # the worst of seeds 0 and 1 (module docstring)


@pytest.mark.parametrize("seed", [0, 1])
def test_restatement_finds_every_body_of_the_scene(seed):
    sc = rr.rigid_scene(seed)
    tri = [rr.triples_of(m, rr.MIN_AREA) for m in sc["models"]]
    res = rr.rigid_poses(sc["xyz"], sc["n"], sc["models"], tri, rr.TOL, rr.GATE)
    rep = rr.scene_report(sc, res)
    print(seed, rep)
    assert rep["wrong"] == 0 and rep["lost"] == 0 and rep["ghost"] == 0 and rep["found"] >= 150, rep
    assert rep["angle"] <= 2 * MEASURED_ANGLE and rep["translation"] <= 2 * MEASURED_TRANSLATION, rep
    assert set(np.unique(res["status"])) <= {0, rr.LOST}
    found = res["status"] == 0
    assert (res["n_in"][found] >= 3).all() and (res["n_in"][~found] == 0).all() and (res["label"][~found] == -1).all()
    q = res["q"][found]
    assert np.allclose((q * q).sum(axis=1), 1.0, atol=1e-14) and (q[:, 0] >= 0).all()


def test_an_exact_tie_goes_to_the_smaller_candidate():
    """An isosceles triangle seen exactly: the hypothesis and its mirror image both fit with rms 0, and (h, i, j, k) decides --
    whichever way the rows are numbered."""
    iso = np.array([[-0.1, 0, 0], [0.1, 0, 0], [0, 0.15, 0]])
    for det in (iso, iso[[1, 0, 2]]):
        r = rr.solve_body(det, iso, [(0, 1, 2)], rr.TOL, rr.GATE, 3, 64)
        assert r["cand"].tolist() == [[0, 0, 1, 2], [0, 1, 0, 2]] and r["cand_rms2"].tolist() == [0.0, 0.0]
        assert r["status"] == 0 and r["winner"].tolist() == [0, 0, 1, 2] and r["label"].tolist() == [0, 1, 2, -1, -1, -1, -1, -1]


def test_the_candidate_list_is_never_shortened():
    tet, model = rr.lattice_case()
    r = rr.solve_body(tet, model, [(0, 1, 2)], rr.TOL, rr.GATE, 3, 24)
    assert r["status"] == 0 and r["n_cand"] == 24 and r["n_in"] == 3
    assert rr.solve_body(tet, model, [(0, 1, 2)], rr.TOL, rr.GATE, 3, 23)["status"] == rr.E_HYP


def _tri(model):
    return rr.triples_of(model, rr.MIN_AREA)


def test_the_lattice_gives_lists_many_times_the_workgroup():
    """What test_gpu_rigid's long-list cases rely on, from the restatement: on the 4 x 4 x 4 lattice the square has 4 triples of
    864 candidates each (3456 = 13.5 trips of 256 lanes), all with 4 inliers; on the exact lattice 912 of them share the lowest
    rms^2 (0.0) bit for bit and the winner is the fourth in (h, i, j, k) order; with 2e-4 of noise the list is as long, and the
    winner is decided by rms^2 and stands hundreds of places down the ordered list; the triangle has 864 = 3 * 256 + 96; the cube
    has 56 triples and 46 656 candidates, more than the list holds."""
    exact, noisy = rr.lattice(), rr.lattice(rr.LATTICE_NOISE)
    assert exact.shape == (64, 3) and len(np.unique(exact, axis=0)) == 64 and np.array_equal(exact / rr.SPACING, np.round(exact / rr.SPACING))
    assert not np.array_equal(np.lexsort(exact.T), np.arange(64))  # the rows are permuted
    assert np.abs(noisy - exact).max() < 5 * rr.LATTICE_NOISE and (noisy != exact).all()
    for det, slack in ((exact, 1e-12), (noisy, rr.TOL / 2)):  # no distance test is close: a model length, or ten tol off
        d = rr.dist_table(det)[np.triu_indices(64, 1)]
        for L in (rr.SPACING, rr.SPACING * np.sqrt(2.0), rr.SPACING * np.sqrt(3.0)):  # the square's two lengths and the cube's third
            gap = np.abs(d - L)
            assert ((gap < slack) | (gap > 10 * rr.TOL)).all()
    assert len(_tri(rr.SQUARE)) == 4 and len(_tri(rr.TRIANGLE)) == 1 and len(_tri(rr.CUBE)) == 56 == rr.MAX_TRIPLES
    r = rr.solve_body(exact, rr.SQUARE, _tri(rr.SQUARE), rr.TOL, rr.GATE, 3, rr.N_SQUARE)
    assert r["status"] == 0 and r["n_cand"] == rr.N_SQUARE == 3456 and np.bincount(r["cand"][:, 0]).tolist() == [864] * 4
    assert (r["cand_n_in"] == 4).all() and r["n_in"] == 4
    low = r["cand_rms2"].min()
    assert low == 0.0 and int((r["cand_rms2"] == low).sum()) == rr.N_SQUARE_TIES == 912
    assert np.array_equal(r["winner"], r["cand"][3]) and r["cand_rms2"][:3].min() > 0.0
    assert rr.solve_body(exact, rr.SQUARE, _tri(rr.SQUARE), rr.TOL, rr.GATE, 3, rr.N_SQUARE - 1)["status"] == rr.E_HYP
    rn = rr.solve_body(noisy, rr.SQUARE, _tri(rr.SQUARE), rr.TOL, rr.GATE, 3, rr.N_SQUARE)
    assert rn["status"] == 0 and rn["n_cand"] == rr.N_SQUARE and (rn["cand_n_in"] == 4).all()
    place = int(np.flatnonzero((rn["cand"] == rn["winner"]).all(axis=1))[0])
    best = rn["cand_rms2"] == rn["cand_rms2"].min()
    assert place >= 256 and best.sum() < 16 and rn["rms"] > 0.0
    assert not np.array_equal(np.sort(rn["label"][:4]), np.sort(r["label"][:4]))  # it labels other detections than the exact winner
    for model, count in ((rr.TRIANGLE, rr.N_TRIANGLE), (rr.CUBE, rr.N_CUBE)):
        for det in (exact, noisy):
            assert len(rr.candidates(rr.dist_table(det), rr.dist_table(model), _tri(model), rr.TOL)) == count
    assert rr.N_TRIANGLE == 864 == 3 * 256 + 96 and rr.N_CUBE == 46656 > rr.MAX_HYP
    assert rr.solve_body(exact, rr.CUBE, _tri(rr.CUBE), rr.TOL, rr.GATE, 3, rr.MAX_HYP)["status"] == rr.E_HYP


def test_ten_tetrahedra_fill_one_trip_and_eleven_start_a_second():
    """k copies of the tetrahedron 5.0 apart: 24 k candidates, 240 at k = 10 and 264 at k = 11.  Every fit is exact but for
    rounding: rms^2 is 0.0 for five orderings of the copy at the origin (an exact tie that (h, i, j, k) decides) and 1e-33 to
    1e-30 for all others, so the smallest rms^2 decides among near-ties."""
    for k, count in ((10, 240), (11, 264)):
        det, model = rr.tetrahedra(k)
        assert det.shape == (4 * k, 3)
        r = rr.solve_body(det, model, _tri(model), rr.TOL, rr.GATE, 3, count)
        assert r["status"] == 0 and r["n_cand"] == count and r["n_in"] == 3 and (r["cand_n_in"] == 3).all()
        exact = r["cand_rms2"] == 0.0
        assert int(exact.sum()) == 5 and (r["cand"][exact, 1:] < 4).all() and r["cand_rms2"].max() < 1e-29
        assert r["winner"].tolist() == [0, 0, 1, 2] and r["rms"] == 0.0
        assert rr.solve_body(det, model, _tri(model), rr.TOL, rr.GATE, 3, count - 1)["status"] == rr.E_HYP


def test_blind_steps_and_bad_models():
    sc = rr.rigid_scene(2, T=3)
    tri = [rr.triples_of(m, rr.MIN_AREA) for m in sc["models"]]
    n = sc["n"].copy()
    n[0], n[2] = -4, 25  # an upstream failure code; more rows than the step has
    bad = [t.copy() for t in tri]
    bad[1][2] = (1, 1, 3)
    res = rr.rigid_poses(sc["xyz"], n, sc["models"], bad, rr.TOL, rr.GATE)
    assert res["status"][0].tolist() == [rr.E_BLIND] * 3 and res["status"][2].tolist() == [rr.E_CAPACITY] * 3
    assert res["status"][1, 1] == rr.E_MODEL and res["status"][1, 0] in (0, rr.LOST)
    assert (res["n_in"][res["status"] != 0] == 0).all() and (res["label"][res["status"] != 0] == -1).all()


def test_rigid_message_round_trip_and_carry():
    from mocapv2_amd.replay import batch_rigid_messages, rigid_message, unpack_rigid_message, unpack_tracker_message
    rng = np.random.default_rng(0)
    q, t = rng.normal(size=(6, 4)), rng.normal(size=(6, 3))
    one = rigid_message("wand", q[1], t[1])
    assert unpack_rigid_message(one) == ("wand", q[1].tolist(), t[1].tolist())
    # the reference's reader (a map of one key to seven numbers) takes it as it is
    assert unpack_tracker_message(rigid_message("tracker1", q[0], t[0])) == q[0].tolist() + t[0].tolist()
    carry = rigid_message("wand", [0.0] * 4, [0.0] * 3)
    has = np.array([False, True, False, False, True, False])
    for name in ("wand", "a name of more than thirty-one bytes, which msgpack frames differently"):
        msgs = batch_rigid_messages(name, q, t, has, carry)
        want = [rigid_message(name, q[s], t[s]) for s in range(6)]
        assert msgs == [carry, want[1], want[1], want[1], want[4], want[4]]
    assert batch_rigid_messages("wand", q[:0], t[:0], has[:0], carry) == []
    assert batch_rigid_messages("wand", q[:2], t[:2], np.zeros(2, bool), carry) == [carry, carry]


def test_rigid_tables_list_the_triples_and_refuse_bad_models():
    from mocapv2_amd.engine import RIGID_MAX_BODIES, rigid_tables
    sc = rr.rigid_scene(0, T=1)
    tab = rigid_tables(sc["models"], rr.MIN_AREA)
    assert tab["model"].shape == (3, 8, 3) and tab["tri"].shape == (3, 56, 3) and tab["tri"].dtype == np.int32
    assert tab["n_markers"].tolist() == [4, 5, 6] and tab["n_tri"].tolist() == [4, 10, 20]
    for b, m in enumerate(sc["models"]):
        assert np.array_equal(tab["tri"][b, :tab["n_tri"][b]], rr.triples_of(m, rr.MIN_AREA)) and np.array_equal(tab["model"][b, :len(m)], m)
        assert not tab["model"][b, len(m):].any() and not tab["tri"][b, tab["n_tri"][b]:].any()
    line = np.array([[0, 0, 0], [0.1, 0, 0], [0.2, 0, 0], [0.1, 0.1, 0]])
    assert rigid_tables([line])["tri"][0, :3].tolist() == [[0, 1, 3], [0, 2, 3], [1, 2, 3]] and rigid_tables([line])["n_tri"][0] == 3
    for bad, what in (([line[:2]], "3..8"), ([np.zeros((9, 3))], "3..8"), ([line[:3]], "min_area"), ([], "bodies"),
                      ([line] * (RIGID_MAX_BODIES + 1), "bodies"), ([line * np.nan], "finite"), ([np.zeros((4, 2))], "3..8")):
        with pytest.raises(ValueError, match=what):
            rigid_tables(bad)


def test_trackers_refuse_bodies_without_tol_and_gate():
    from mocapv2_amd.pipeline import BatchTracker
    from mocapv2_amd.replay import ReplayTracker
    eye = np.stack([np.eye(3)] * 2)
    args = (eye, np.zeros((2, 5)), eye, np.zeros((2, 3)), None, 64, 64)
    model = rr.rigid_scene(0, T=1)["models"][0]
    for bad in ({"models": [model], "tol": 0.003}, {"models": [model], "gate": 0.006}, {"tol": 0.003, "gate": 0.006},
                {"models": [model], "tol": 0.003, "gate": 0.006, "gait": 1}, {"models": [model[:2]], "tol": 0.003, "gate": 0.006}):
        with pytest.raises(ValueError):
            BatchTracker(*args, 4, visibility="any", bodies=bad)
        with pytest.raises(ValueError):
            ReplayTracker(*args, batch=4, visibility="any", bodies=bad)


def test_header_binding_and_caps_agree():
    from mocapv2_amd import _abi, engine
    text = open(os.path.join(ROOT, "include", "mocap_hip.h")).read()
    decl = re.search(r"MOCAP_API int mocap_rigid_poses\((.*?)\);", text, re.S).group(1)
    decl = re.sub(r"/\*.*?\*/", "", decl, flags=re.S)
    assert len(decl.split(",")) == len(_abi.SIGNATURES["mocap_rigid_poses"]) == 22
    for name, code in (("LOST", rr.LOST), ("E_BLIND", rr.E_BLIND), ("E_CAPACITY", rr.E_CAPACITY), ("E_MODEL", rr.E_MODEL), ("E_HYP", rr.E_HYP)):
        assert f"MOCAP_RIGID_{name} = {code}," in text and getattr(engine, f"RIGID_{name}") == code
    for name, cap in (("DETECTIONS", rr.MAX_DET), ("MARKERS", rr.MAX_MARKERS), ("TRIPLES", rr.MAX_TRIPLES), ("BODIES", rr.MAX_BODIES),
                      ("HYP", rr.MAX_HYP)):
        assert f"#define MOCAP_RIGID_MAX_{name} {cap}\n" in text and getattr(engine, f"RIGID_MAX_{name}") == cap
    assert "#define MOCAP_ABI_VERSION 7\n" in text and _abi.ABI_VERSION == 7


def test_rigid_kernel_uses_no_scratch_memory_and_spills_nothing():
    spec = importlib.util.spec_from_file_location("kernel_meta", os.path.join(ROOT, "scratch", "kernel_meta.py"))
    km = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(km)
    ks = km.kernels_of(os.path.join(km.CSRC, "rigid.hip"))
    assert [k["name"].count("rigid_poses_kernel") for k in ks] == [1]
    for k in ks:
        print(k)
        assert k["scratch"] == 0 and k["spill"] == 0 and k["lds"] <= 65536, k
    make = open(os.path.join(km.CSRC, "Makefile")).read()
    assert "rigid.hip" in make and "abi_rigid.hip" in make
