"""The host layer's parts that need no GPU: the binding against the header argument by argument, the records' layout arithmetic
against values written out by hand, the result-tensor tables, and the input checks of the rig and board problems."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. include/mocap_hip.h against _abi.SIGNATURES ------------------------------------------------------------------------
SCALARS = {"int": ctypes.c_int, "double": ctypes.c_double, "long": ctypes.c_long, "size_t": ctypes.c_size_t,
           "mocap_ctx_t": ctypes.c_void_p}
POINTEES = {"double": ctypes.c_double, "float": ctypes.c_float, "int": ctypes.c_int, "int32_t": ctypes.c_int32,
            "uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64}


def declarations():
    """{name: [(type words without const, is a pointer or an array)]} of every MOCAP_API declaration of the header"""
    text = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "mocap_hip.h")).read(), flags=re.S)
    out = {}
    for name, params in re.findall(r"MOCAP_API\s+[\w\s\*]+?\b(mocap_\w+)\s*\(([^)]*)\)\s*;", text):
        out[name] = []
        for p in (q.strip() for q in params.split(",")):
            if p == "void":
                continue
            pointer = "*" in p or "[" in p
            words = [w for w in re.sub(r"\[[^\]]*\]|\*", " ", p).split() if w != "const"]
            assert len(words) >= 2, (name, p)  # a type and a name
            out[name].append((" ".join(words[:-1]), pointer))
    return out


def test_every_argument_of_the_binding_has_the_headers_class():
    from mocapv2_amd import _abi
    decl = declarations()
    assert sorted(decl) == sorted(_abi.SIGNATURES) and len(decl) == 50
    for name, params in decl.items():
        sig = _abi.SIGNATURES[name]
        assert len(sig) == len(params), (name, len(sig), len(params))
        for k, ((ctype, pointer), bound) in enumerate(zip(params, sig)):
            if not pointer:
                assert ctype in SCALARS, (name, k, ctype)
                assert bound is SCALARS[ctype], (name, k, ctype, bound)
            elif bound not in (ctypes.c_void_p, ctypes.c_char_p):
                assert issubclass(bound, ctypes._Pointer), (name, k, ctype, bound)
                if ctype in POINTEES:
                    assert bound._type_ is POINTEES[ctype], (name, k, ctype, bound._type_)


# ---- 2. the records' layout ------------------------------------------------------------------------------------------------------
REC, PTS = 0x10000, 0x20000   # addresses of the records and of the points block
REC_INTS, CN, T_TOTAL, ROWS = 18, 3, 3, 6   # records of capacity 8 (72 bytes); 6 points rows of 16 bytes per image


def test_record_layout_time_major_default():
    from mocapv2_amd._dev import record_layout
    # the record of (t, c) is record 3 t + c: 54 and 18 ints apart; the points start 8 bytes into the record; P = the capacity
    assert record_layout(REC, REC_INTS, CN) == (REC + 8, 54, 18, REC, 54, 18, 0, 8)
    assert record_layout(REC, REC_INTS, CN, t0=0, stride_t=CN, stride_c=1, P=4) == (REC + 8, 54, 18, REC, 54, 18, 0, 4)
    assert record_layout(REC, 2 + 2 * 100, CN)[7] == 100 and record_layout(REC, 2 + 2 * 300, CN)[7] == 255  # min(255, capacity)
    # from time step 2: 2 * 3 records of 72 bytes further on
    assert record_layout(REC, REC_INTS, CN, t0=2, P=4) == (REC + 432 + 8, 54, 18, REC + 432, 54, 18, 0, 4)


def test_record_layout_camera_major_from_t0():
    from mocapv2_amd._dev import record_layout
    # the record of (t, c) is record T_total c + t: 18 and 54 ints apart; time step 1 starts one record = 72 bytes in
    got = record_layout(REC, REC_INTS, CN, t0=1, stride_t=1, stride_c=T_TOTAL, P=4)
    assert got == (REC + 72 + 8, 18, 54, REC + 72, 18, 54, 0, 4)


def test_record_layout_with_a_points_block_whose_rows_exceed_p():
    from mocapv2_amd._dev import record_layout
    # an image's block is 6 rows x 2 doubles = 12 doubles = 96 bytes; the counts stay the records'
    got = record_layout(REC, REC_INTS, CN, P=4, points=PTS, rows=ROWS)
    assert got == (PTS, 36, 12, REC, 54, 18, 1, 4)
    got = record_layout(REC, REC_INTS, CN, t0=1, stride_t=1, stride_c=T_TOTAL, P=4, points=PTS, rows=ROWS)
    assert got == (PTS + 96, 12, 36, REC + 72, 18, 54, 1, 4)
    assert record_layout(REC, REC_INTS, CN, points=PTS, rows=8) == (PTS, 48, 16, REC, 54, 18, 1, 8)  # P = the records' capacity
    with pytest.raises(AssertionError):
        record_layout(REC, REC_INTS, CN, points=PTS, rows=ROWS)  # 6 rows cannot hold the default P = 8
    with pytest.raises(AssertionError):
        record_layout(REC, REC_INTS, CN, P=7, points=PTS, rows=ROWS)


# ---- 3. outputs ---------------------------------------------------------------------------------------------------------------------
def spec():
    import torch
    from mocapv2_amd._dev import AtLeast
    return {"a": ((2, 3), torch.float64, 0), "b": ((2,), torch.int32, -1), "c": ((2, AtLeast(4), 2), torch.int32, None)}


def test_outputs_allocates_the_tables_shapes_dtypes_and_fills():
    import torch
    from mocapv2_amd._dev import outputs
    out = outputs(spec(), "cpu")
    assert sorted(out) == ["a", "b", "c"]
    assert out["a"].shape == (2, 3) and out["a"].dtype == torch.float64 and (out["a"] == 0).all()
    assert out["b"].shape == (2,) and out["b"].dtype == torch.int32 and (out["b"] == -1).all()
    assert out["c"].shape == (2, 4, 2) and out["c"].dtype == torch.int32
    assert all(t.is_contiguous() and t.device.type == "cpu" for t in out.values())


def test_outputs_passes_a_matching_out_through_and_refuses_any_other():
    import torch
    from mocapv2_amd._dev import outputs
    good = outputs(spec(), "cpu")
    good["c"] = torch.full((2, 6, 2), 9, dtype=torch.int32)  # more rows than the table's: allowed where it says AtLeast
    good["extra"] = torch.zeros(1)                           # the trackers hand in dicts that carry more
    before = dict(good)
    good["a"].fill_(5.0)
    assert outputs(spec(), "cpu", good) is good
    assert list(good) == list(before) and all(good[k] is before[k] for k in before)
    assert (good["a"] == 5.0).all() and (good["b"] == -1).all() and (good["c"] == 9).all()
    for key, bad in (("a", torch.zeros((2, 4), dtype=torch.float64)),           # shape
                     ("a", torch.zeros((6,), dtype=torch.float64)),             # rank
                     ("c", torch.zeros((2, 3, 2), dtype=torch.int32)),          # fewer rows than the table's
                     ("c", torch.zeros((3, 4, 2), dtype=torch.int32)),          # AtLeast frees one dimension only
                     ("a", torch.zeros((2, 3), dtype=torch.float32)),           # dtype
                     ("b", torch.zeros((2,), dtype=torch.int64)),
                     ("a", torch.zeros((3, 2), dtype=torch.float64).t()),       # not contiguous
                     ("b", torch.zeros((4,), dtype=torch.int32)[::2])):
        with pytest.raises(AssertionError):
            outputs(spec(), "cpu", {**good, key: bad})
    with pytest.raises(KeyError):
        outputs(spec(), "cpu", {"a": good["a"], "b": good["b"]})


# ---- 4. rig_problem and board_problem -------------------------------------------------------------------------------------------
def rig_case():
    """3 cameras, 4 points seen by cameras (0, 1, 2), (0, 1), (1, 2), (0, 2)"""
    rng = np.random.default_rng(5)
    return {"obs_offset": np.array([0, 3, 5, 7, 9]), "obs_cam": np.array([0, 1, 2, 0, 1, 1, 2, 0, 2]), "obs_uv": rng.uniform(0, 900, (9, 2)),
            "poses": rng.normal(size=(3, 12)), "points": rng.normal(size=(4, 3))}


def test_rig_problem_returns_the_typed_arrays_and_sizes():
    from mocapv2_amd.engine_calib import rig_problem
    c = rig_case()
    Cn, N, n_obs, off, cam, uv, poses, points = rig_problem(**c)
    assert (Cn, N, n_obs) == (3, 4, 9)
    for got, key, dt in ((off, "obs_offset", np.int32), (cam, "obs_cam", np.int32), (uv, "obs_uv", np.float64),
                         (poses, "poses", np.float64), (points, "points", np.float64)):
        assert got.dtype == dt and got.flags.c_contiguous and np.array_equal(got, c[key]), key
    lists = rig_problem(c["obs_offset"].tolist(), c["obs_cam"].tolist(), c["obs_uv"].reshape(-1), c["poses"].tolist(), c["points"].reshape(-1))
    assert all(np.array_equal(a, b) for a, b in zip(lists[3:], (off, cam, uv, poses, points)))


def spoiled(case, key, fn):
    c = {k: np.array(v, copy=True) for k, v in case.items()}
    c[key] = fn(c[key])
    return c


def at(index, value):
    def put(a):
        a[index] = value
        return a
    return put


RIG_ERRORS = [
    ("poses", lambda p: p[:, :11], "poses must be"),                                    # pose shape
    ("poses", lambda p: p[:1], "poses must be"),                                        # 1 camera
    ("poses", lambda p: np.zeros((33, 12)), "poses must be"),                           # 33 cameras
    ("obs_offset", at(0, 1), "obs_offset must be"),                                     # not from 0
    ("obs_offset", at(-1, 8), "obs_offset must be"),                                    # not to n_obs
    ("obs_offset", lambda o: np.append(o, 9), "obs_offset must be"),                    # not N + 1 entries
    ("obs_uv", lambda u: u[:8], "obs_offset must be"),                                  # not n_obs pixels
    ("obs_offset", lambda o: np.array([0, 1, 3, 6, 9]), "2..C observations"),           # a point with one observation
    ("obs_offset", lambda o: np.array([0, 4, 6, 7, 9]), "2..C observations"),           # a point with four (and one with one)
    ("obs_cam", at(2, 3), "obs_cam outside"),
    ("obs_cam", at(0, -1), "obs_cam outside"),
    ("obs_cam", lambda c: np.array([1, 0, 2, 0, 1, 1, 2, 0, 2]), "strictly ascending"),
    ("obs_cam", lambda c: np.array([0, 1, 2, 0, 1, 1, 2, 2, 2]), "strictly ascending"),  # the same camera twice
    ("obs_uv", at((4, 1), np.nan), "must be finite"),
    ("poses", at((1, 3), np.inf), "must be finite"),
    ("points", at((3, 0), np.nan), "must be finite"),
]


@pytest.mark.parametrize("key,fn,text", RIG_ERRORS, ids=[f"{k}-{i}" for i, (k, _, _) in enumerate(RIG_ERRORS)])
def test_rig_problem_names_what_is_wrong(key, fn, text):
    from mocapv2_amd.engine_calib import rig_problem
    with pytest.raises(ValueError, match=re.escape(text)):
        rig_problem(**spoiled(rig_case(), key, fn))


def test_rig_problem_refuses_more_observations_than_cameras():
    from mocapv2_amd.engine_calib import rig_problem
    c = rig_case()
    c.update(obs_offset=np.array([0, 4, 6, 9]), points=c["points"][:3])  # 4, 2 and 3 observations with 3 cameras
    with pytest.raises(ValueError, match=re.escape("2..C observations")):
        rig_problem(**c)


def board_case():
    """2 cameras, 3 views each, 4 points per view"""
    rng = np.random.default_rng(6)
    return {"view_offset": np.array([0, 3, 6]), "point_offset": np.arange(7) * 4, "obj_xy": rng.uniform(0, 1, (24, 2)),
            "img_uv": rng.uniform(0, 900, (24, 2))}


def test_board_problem_returns_the_typed_arrays_and_sizes():
    from mocapv2_amd.engine_calib import board_problem
    c = board_case()
    n_cams, n_views, voff, poff, obj, img = board_problem(**c)
    assert (n_cams, n_views) == (2, 6)
    for got, key, dt in ((voff, "view_offset", np.int32), (poff, "point_offset", np.int32), (obj, "obj_xy", np.float64),
                         (img, "img_uv", np.float64)):
        assert got.dtype == dt and got.flags.c_contiguous and np.array_equal(got, c[key]), key


BOARD_ERRORS = [
    ("view_offset", at(0, 1), "view_offset must be"),                                   # not from 0
    ("view_offset", lambda v: np.array([0, 4, 3]), "view_offset must be"),              # descending
    ("view_offset", lambda v: v[:1], "view_offset must be"),                            # no camera
    ("view_offset", lambda v: np.zeros(3, int), "point_offset must be"),                # no view
    ("point_offset", lambda p: p[:-1], "point_offset must be"),                         # not n_views + 1 entries
    ("point_offset", at(0, 1), "point_offset must be"),
    ("point_offset", at(3, 2), "point_offset must be"),                                 # descending
    ("obj_xy", lambda o: o[:-1], "obj_xy and img_uv must be"),
    ("img_uv", lambda i: i[:-1], "obj_xy and img_uv must be"),
    ("obj_xy", at((0, 0), np.nan), "must be finite"),
    ("img_uv", at((23, 1), np.inf), "must be finite"),
]


@pytest.mark.parametrize("key,fn,text", BOARD_ERRORS, ids=[f"{k}-{i}" for i, (k, _, _) in enumerate(BOARD_ERRORS)])
def test_board_problem_names_what_is_wrong(key, fn, text):
    from mocapv2_amd.engine_calib import board_problem
    with pytest.raises(ValueError, match=re.escape(text)):
        board_problem(**spoiled(board_case(), key, fn))


# ---- the composed class ---------------------------------------------------------------------------------------------------------
def test_engine_still_exports_what_it_did_and_no_stage_shadows_another():
    from mocapv2_amd import engine
    for name in ("MocapContext", "BAProblem", "default_context", "comm_available", "comm_unique_id", "rigid_tables", "_ptr", "_stream",
                 "MAX_BLOBS", "GRAY_SHIFT", "REC_INTS", "RIG_LOSSES", "SUBPIX_COORDS", "SUBPIX_EMPTY", "SUBPIX_EDGE", "SUBPIX_NEIGHBOUR",
                 "SUBPIX_MOVING", "SUBPIX_CUT", "SUBPIX_FALLBACK", "RIGID_LOST", "RIGID_E_BLIND", "RIGID_E_CAPACITY", "RIGID_E_MODEL",
                 "RIGID_E_HYP", "RIGID_MAX_DETECTIONS", "RIGID_MAX_MARKERS", "RIGID_MAX_TRIPLES", "RIGID_MAX_BODIES", "RIGID_MAX_HYP"):
        assert hasattr(engine, name), name
    owners = {}
    for cls in engine.MocapContext.__mro__[:-1]:
        for attr in vars(cls):
            if not (attr.startswith("__") and attr.endswith("__")):
                assert attr not in owners, (attr, owners[attr], cls.__name__)
                owners[attr] = cls.__name__
    assert callable(engine.MocapContext._vis_out)
