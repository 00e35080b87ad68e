"""Learning rigid-body models from a tracked capture (tests/rigid_learn_ref.py) on the CPU: what the definition
promises on the seeded take, the grouping's refusal, the constants of header, binding and package, and the kernels' compiler
metadata.

Take: rigid_learn_ref.take -- rigid_ref.rigid_scene (three bodies of 4, 5 and 6 markers on random poses in a 2 m cube, each marker
hidden with p = 0.2, 4 clutter points per step, 0.5 mm Gaussian noise per axis, rows shuffled, T = 60) with the identities of its
`row` truth; spread = 8 mm, min_steps = 10.  Measured with the restatement over seeds 3, 4, 5: same-body pairs spread (max - min)
by at most 0.0050, pairs across bodies by at least 1.37; the three groups come out exactly; every member is averaged over 36 to 54
observations and the learned points lie 0.10 to 0.23 mm from the truth after alignment (one observation: 0.5 mm per axis); without
noise they are exact to 1.2e-16."""
import importlib.util
import os
import re

import numpy as np
import pytest

import rigid_learn_ref as rl
import rigid_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def learned(tk, **kw):
    from mocapv2_amd.engine import rigid_groups
    ids = rl.frequent_ids(tk["n"], tk["id"], rl.MIN_STEPS)
    pairs = rl.pair_stats(tk["xyz"], tk["n"], tk["id"], ids)
    groups, unassigned = rigid_groups(ids, pairs["count"], pairs["dmin"], pairs["dmax"], rl.SPREAD, rl.MIN_STEPS)
    return ids, pairs, groups, unassigned, rl.rigid_learn(tk["xyz"], tk["n"], tk["id"], groups, **kw) if groups else None


@pytest.fixture(scope="module")
def takes():
    return {seed: rl.take(seed) for seed in (3, 4, 5)}


@pytest.fixture(scope="module")
def results(takes):
    return {seed: learned(tk) for seed, tk in takes.items()}


@pytest.mark.parametrize("seed", [3, 4, 5])
def test_the_groups_are_the_bodies_and_the_models_beat_one_observation(takes, results, seed):
    tk = takes[seed]
    ids, pairs, groups, unassigned, res = results[seed]
    assert ids.tolist() == sorted(sum(rl.truth_members(tk), []))  # a clutter identity lives one step
    assert groups == rl.truth_members(tk) and unassigned == []
    body = ids[:, None] // 10 == ids[None, :] // 10
    off = ~np.eye(len(ids), dtype=bool)
    spread = pairs["dmax"] - pairs["dmin"]
    seen = pairs["count"] >= rl.MIN_STEPS
    print(seed, "same-body spread", spread[body & off].max(), "across", spread[~body & seen].min())
    assert spread[body & off].max() <= rl.SPREAD < 1.0 < spread[~body & seen].min()
    assert (res["status"] == 0).all() and (res["ref_step"] >= 0).all()
    for g, truth in enumerate(tk["models"]):
        M = len(truth)
        err = rl.aligned_error(res["model"][g, :M], truth)
        print(seed, g, "error", err.max(), "observations", res["member_count"][g, :M].tolist(), "rms", res["rms"][g])
        assert res["member_count"][g, :M].min() >= 25 and not res["member_count"][g, M:].any() and not res["model"][g, M:].any()
        assert err.max() < rr.NOISE
        assert np.abs(res["model"][g, :M].sum(axis=0)).max() < 1e-15  # the origin is the centroid
        assert 0.0 < res["rms"][g] < 2 * rr.NOISE * np.sqrt(3.0)


@pytest.mark.parametrize("seed", [3, 4, 5])
def test_without_noise_the_models_are_exact(seed):
    tk = rl.take(seed, noise=0.0)
    _, _, groups, _, res = learned(tk)
    assert groups == rl.truth_members(tk) and (res["status"] == 0).all()
    for g, truth in enumerate(tk["models"]):
        err = rl.aligned_error(res["model"][g, :len(truth)], truth)
        print(seed, g, err.max())
        assert err.max() < 1e-12 and res["rms"][g] < 1e-12


@pytest.mark.parametrize("seed", [3, 4])
def test_the_learned_models_pose_as_the_true_ones_do(takes, results, seed):
    tk, res = takes[seed], results[seed][4]
    models = [res["model"][g, :len(m)] for g, m in enumerate(tk["models"])]
    out = []
    for ms in (tk["models"], models):
        tri = [rr.triples_of(m, rr.MIN_AREA) for m in ms]
        out.append(rr.rigid_poses(tk["xyz"][:20], tk["n"][:20], ms, tri, rr.TOL, rr.GATE))
    assert np.array_equal(out[0]["status"], out[1]["status"]) and np.array_equal(out[0]["n_in"], out[1]["n_in"])
    assert (out[0]["status"] == 0).sum() >= 40


def test_bodies_that_never_move_against_one_another_are_refused():
    from mocapv2_amd.engine import rigid_groups
    tk = rl.static_take()
    ids = rl.frequent_ids(tk["n"], tk["id"], rl.MIN_STEPS)
    assert len(ids) == 15
    pairs = rl.pair_stats(tk["xyz"], tk["n"], tk["id"], ids)
    with pytest.raises(ValueError, match=r"\[0, 1, 2, 3, 10, 11, 12, 13, 14, 20, 21, 22, 23, 24, 25\].*more than 8"):
        rigid_groups(ids, pairs["count"], pairs["dmin"], pairs["dmax"], rl.SPREAD, rl.MIN_STEPS)


def test_grouping_walks_the_identities_in_ascending_order():
    from mocapv2_amd.engine import rigid_groups
    ids = [2, 5, 7, 9, 11, 30]
    rigid = np.zeros((6, 6), bool)
    for a, b in ((0, 1), (0, 2), (1, 2), (0, 3), (3, 4)):  # 2-5-7 a triangle; 9 rigid with 2 only; 9-11 a pair; 30 alone
        rigid[a, b] = rigid[b, a] = True
    count = np.where(rigid, 10, 3)
    dmin, dmax = np.zeros((6, 6)), np.where(rigid, 0.001, 0.0)
    assert rigid_groups(ids, count, dmin, dmax, 0.002, 10) == ([[2, 5, 7]], [9, 11, 30])
    assert rigid_groups(ids, count, dmin, dmax, 0.002, 11) == ([], ids)       # too few common steps
    assert rigid_groups(ids, count, dmin, dmax, 0.0005, 10) == ([], ids)      # the distances vary too much
    many = np.ones((51, 51), bool)
    for a in range(51):
        for b in range(51):
            many[a, b] = a // 3 == b // 3
    with pytest.raises(ValueError, match="17 bodies"):
        rigid_groups(range(51), np.where(many, 10, 0), np.zeros((51, 51)), np.zeros((51, 51)), 0.001, 10)


def test_group_statuses_of_the_restatement():
    tk = rl.take(3, T=40)
    res = rl.rigid_learn(tk["xyz"], tk["n"], tk["id"], [[0, 1, 2, 3], [0, 1, 1], [0, 1], [0, 1, 999999], [0, -1, 2], [10, 11, 12]], min_present=3)
    assert res["status"].tolist() == [0, rl.E_MEMBERS, rl.E_MEMBERS, rl.E_INCOMPLETE, rl.E_MEMBERS, 0]
    bad = res["status"] != 0
    assert (res["ref_step"][bad] == -1).all() and not res["member_count"][bad].any() and not res["steps_used"][bad].any()
    assert rl.rigid_learn(tk["xyz"], tk["n"], tk["id"], [[0, 1, 2]], min_present=4)["status"].tolist() == [rl.E_MEMBERS]


def test_header_binding_and_constants_agree():
    """libmocap_learn.so is a library of its own (include/mocap_learn.h, _abi.LEARN_SIGNATURES): the main header and its binding
    stay as they were"""
    from mocapv2_amd import _abi, engine
    text = open(os.path.join(ROOT, "include", "mocap_learn.h")).read()
    declared = sorted(set(re.findall(r"MOCAP_LEARN_API\s+[\w\s\*]+?\b(mocap_learn_\w+)\s*\(", text)))
    assert declared == sorted(_abi.LEARN_SIGNATURES) and len(declared) == 4
    for name, args in (("mocap_learn_marker_pair_stats", 16), ("mocap_learn_rigid_bodies", 21)):
        decl = re.search(r"MOCAP_LEARN_API int %s\((.*?)\);" % name, text, re.S).group(1)
        decl = re.sub(r"/\*.*?\*/", "", decl, flags=re.S)
        assert len(decl.split(",")) == len(_abi.LEARN_SIGNATURES[name]) == args
    for name, code in (("MEMBERS", rl.E_MEMBERS), ("INCOMPLETE", rl.E_INCOMPLETE)):
        assert f"MOCAP_LEARN_E_{name} = {code}," in text.replace(",  ", ", ") or f"MOCAP_LEARN_E_{name} = {code} " in text
        assert getattr(engine, f"LEARN_E_{name}") == code
    for name, cap in (("CHUNK", rl.CHUNK), ("MAX_IDS", rl.MAX_IDS), ("MAX_GROUPS", rl.MAX_GROUPS)):
        assert f"#define MOCAP_LEARN_{name} {cap}\n" in text and getattr(engine, f"LEARN_{name}") == cap
    assert f"#define MOCAP_LEARN_ABI_VERSION {_abi.LEARN_ABI_VERSION}\n" in text
    main = open(os.path.join(ROOT, "include", "mocap_hip.h")).read()
    assert "#define MOCAP_ABI_VERSION 7\n" in main and _abi.ABI_VERSION == 7 and "mocap_learn" not in main
    assert not [k for k in _abi.SIGNATURES if "learn" in k]
    # the workspace macro, evaluated as C would, against the package's arithmetic
    macro = re.search(r"#define MOCAP_LEARN_WORK_BYTES\(T, K, G\)(.*?)\n(?!\s)", text, re.S).group(1).replace("\\\n", " ")
    macro = macro.replace("(size_t)", "").replace("MOCAP_LEARN_CHUNKS(T)", "((T + 31) // 32)").replace("MOCAP_LEARN_PAIRS(K)", "(K * (K + 1) // 2)")
    for T, K, G in ((0, 2, 0), (1, 64, 0), (33, 0, 16), (36000, 64, 0), (8229, 0, 3)):
        assert eval(macro, {"T": T, "K": K, "G": G}) == engine.learn_work_bytes(T, K, G)


def test_the_learn_library_exports_its_header_and_nothing_else():
    import shutil
    import subprocess
    from mocapv2_amd import _abi
    if not os.path.exists(_abi.LEARN_LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = _abi.load_learn()
    assert lib.mocap_learn_abi_version() == _abi.LEARN_ABI_VERSION
    if shutil.which("nm"):
        out = subprocess.run(["nm", "-D", "--defined-only", _abi.LEARN_LIB_PATH], check=True, capture_output=True, text=True).stdout
        exported = sorted(f[2] for f in (line.split() for line in out.splitlines()) if len(f) == 3 and f[1] == "T")
        assert exported == sorted(_abi.LEARN_SIGNATURES)
    # bad arguments are refused before the device is touched: no GPU is needed to see it
    import ctypes
    ids = (ctypes.c_int32 * 3)(3, 2, 1)
    one = ctypes.c_void_p(8)
    assert lib.mocap_learn_marker_pair_stats(0, None, None, None, 0, 4, ctypes.addressof(ids), 3, None, 0, one, one, one, one, one, None) == -1
    assert b"ascending" in lib.mocap_learn_last_error()


def test_learn_kernels_use_no_scratch_memory_and_spill_nothing():
    spec = importlib.util.spec_from_file_location("kernel_meta", os.path.join(ROOT, "scratch", "kernel_meta.py"))
    km = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(km)
    ks = km.kernels_of(os.path.join(km.CSRC, "rigid_learn.hip"))
    names = " ".join(k["name"] for k in ks)
    for want in ("learn_locate_kernel", "pair_chunk_kernel", "pair_total_kernel", "learn_seed_kernel", "learn_pose_kernel", "learn_total_kernel"):
        assert names.count(want) == 1, names
    assert len(ks) == 6
    for k in ks:
        print(k)
        assert k["scratch"] == 0 and k["spill"] == 0 and k["lds"] <= 65536, k
    make = open(os.path.join(km.CSRC, "Makefile")).read()
    assert "rigid_learn.hip" in make and "abi_rigid_learn.hip" in make
    shared = open(os.path.join(km.CSRC, "rigid_dev.h")).read()
    for src in ("rigid.hip", "rigid_learn.hip"):
        text = open(os.path.join(km.CSRC, src)).read()
        assert '#include "rigid_dev.h"' in text and "void horn(" not in text
    assert shared.count("void horn(") == 1
