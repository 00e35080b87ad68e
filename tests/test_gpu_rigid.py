"""mocap_rigid_poses on the GPU against its NumPy restatement (tests/rigid_ref.py).

status, n_in and label are compared for EQUALITY everywhere; R, t, q and rms as 64-bit patterns wherever the status is 0 (elsewhere
the floats are unspecified).  The definition fixes every operation and its order, uses + - * / and sqrt only, and the library is
built without fused multiply-adds, so there is no tolerance anywhere.

Candidate lists from none to 56 come from the seeded scene and the hand-made bodies; lists of 240 to 3456 candidates -- up to 14
trips of the workgroup's lanes -- and one of 46 656, beyond the LDS list, from the lattice and the tetrahedra of rigid_ref, whose
counts test_rigid_host asserts.

The trackers (rendered frames, 3 cameras at 640 x 480, one body of 4 discs, sub-pixel centroids) are checked against the scene's
truth.  Measured on the MI355X over the 4 steps, both visibilities alike: the worst pose is 0.0000479 rad and 0.02119 mm from
truth (docstring of test_trackers_find_the_rendered_body); the bounds are twice that."""
import numpy as np
import pytest

import rigid_ref as rr
import subpixel_ref as sref

pytestmark = pytest.mark.gpu

FLOATS, INTS = ("R", "t", "q", "rms"), ("status", "n_in", "label")


@pytest.fixture(scope="module")
def ctx():
    from mocapv2_amd.engine import MocapContext
    return MocapContext(1, 1)


def run_gpu(ctx, xyz, n, models, tol=rr.TOL, gate=rr.GATE, **kw):
    import torch
    bodies = ctx.rigid_bodies(models, rr.MIN_AREA)
    out = ctx.rigid_poses(torch.from_numpy(np.ascontiguousarray(xyz, np.float64)).cuda(),
                          torch.from_numpy(np.ascontiguousarray(n, np.int32)).cuda(), bodies, tol, gate, **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def run_ref(xyz, n, models, tol=rr.TOL, gate=rr.GATE, **kw):
    return rr.rigid_poses(xyz, n, models, [rr.triples_of(m, rr.MIN_AREA) for m in models], tol, gate, **kw)


def assert_same(got, want, what=""):
    for k in INTS:
        bad = np.argwhere(got[k] != want[k])
        assert len(bad) == 0, (what, k, bad[:4].tolist(), got[k][tuple(bad[0])], want[k][tuple(bad[0])])
    ok = want["status"] == 0
    for k in FLOATS:
        g, w = np.ascontiguousarray(got[k][ok]).view(np.uint64), np.ascontiguousarray(want[k][ok]).view(np.uint64)
        bad = np.argwhere(g != w)
        assert len(bad) == 0, (what, k, bad[:4].tolist(), got[k][ok][tuple(bad[0])], want[k][ok][tuple(bad[0])])


def check(ctx, xyz, n, models, what="", **kw):
    got, want = run_gpu(ctx, xyz, n, models, **kw), run_ref(xyz, n, models, **kw)
    assert_same(got, want, what)
    return got


def posed(model, rng, shown=None):
    R, t = rr.random_rotation(rng), rng.uniform(-1, 1, 3)
    pts = model @ R.T + t
    return pts if shown is None else pts[list(shown)]


def steps_of(lists, Q):
    """lists of [k, 3] detections per step -> (xyz [T, Q, 3] with NaN beyond the counts, n [T])"""
    xyz = np.full((len(lists), Q, 3), np.nan)
    for s, d in enumerate(lists):
        xyz[s, :len(d)] = d
    return xyz, np.array([len(d) for d in lists], np.int32)


@pytest.fixture(scope="module")
def scene():
    sc = rr.rigid_scene(3, T=8)
    return sc, run_ref(sc["xyz"], sc["n"], sc["models"])


def test_the_scene_with_nan_beyond_the_counts(ctx, scene):
    """T = 8, B = 3, n <= 20; the rows beyond a step's count hold NaN, and other poison there changes nothing"""
    sc, want = scene
    assert sc["n"].max() <= 20 and np.isnan(sc["xyz"][0, sc["n"][0]:]).all()
    got = run_gpu(ctx, sc["xyz"], sc["n"], sc["models"])
    assert_same(got, want, "scene")
    rep = rr.scene_report(sc, got)
    assert rep["wrong"] == 0 and rep["lost"] == 0 and rep["ghost"] == 0 and rep["found"] >= 20, rep
    for poison in (0.0, 1e300, np.inf):
        assert_same(run_gpu(ctx, np.where(np.isnan(sc["xyz"]), poison, sc["xyz"]), sc["n"], sc["models"]), want, f"poison {poison}")


def test_the_same_call_twice_gives_the_same_bits(ctx, scene):
    sc, _ = scene
    a, b = (run_gpu(ctx, sc["xyz"], sc["n"], sc["models"]) for _ in range(2))
    ok = a["status"] == 0
    for k in FLOATS + INTS:
        assert np.array_equal(a[k][ok].view(np.uint8), b[k][ok].view(np.uint8)) and (k in FLOATS or np.array_equal(a[k], b[k])), k


@pytest.mark.parametrize("B", [1, 16])
def test_one_body_and_sixteen(ctx, scene, B):
    sc, want = scene
    models = [sc["models"][b % 3] for b in range(B)]
    got = run_gpu(ctx, sc["xyz"], sc["n"], models)
    assert_same(got, {k: v[:, [b % 3 for b in range(B)]] for k, v in want.items()}, f"B = {B}")


def test_counts_from_none_to_one_too_many(ctx):
    """n = 0, 1, 2 (nothing to find), 64 (the most a step holds: the body among 60 stray points), 65 and a negative count (blind
    steps), with Q = 66 rows"""
    rng = np.random.default_rng(11)
    model = rr.make_body(rng, 4)
    body = posed(model, rng)
    full = np.concatenate([rng.uniform(-2, 2, (60, 3)), body])[rng.permutation(64)]
    xyz, n = steps_of([body[:0], body[:1], body[:2], full, np.zeros((65, 3)), full], 66)
    n[5] = -3
    got = check(ctx, xyz, n, [model], "counts")
    assert got["status"][:, 0].tolist() == [rr.LOST, rr.LOST, rr.LOST, 0, rr.E_CAPACITY, rr.E_BLIND]
    assert got["n_in"][3, 0] == 4 and np.allclose(full[got["label"][3, 0, :4]], body, atol=0)
    assert (got["n_in"][got["status"] != 0] == 0).all() and (got["label"][got["status"] != 0] == -1).all()
    # Q itself bounds a step as well: the same 64 detections in rows of 40 are one too many
    assert run_gpu(ctx, xyz[:, :40], np.array([0, 1, 2, 41, 40, 3], np.int32), [model])["status"][:, 0].tolist()[3] == rr.E_CAPACITY


def test_three_and_eight_markers_at_and_below_min_markers(ctx):
    """M = 3 and M = 8 side by side; the body of eight with all, with exactly min_markers = 5 and with 4 of its markers visible;
    the triangle with all three and with two"""
    rng = np.random.default_rng(12)
    m3, m8 = rr.make_body(rng, 3), rr.make_body(rng, 8, size=0.5)
    shown8 = [range(8), (0, 2, 3, 5, 7), (1, 2, 4, 6), range(8)]
    shown3 = [range(3), range(3), range(3), (0, 2)]
    lists = []
    for s in range(4):
        pts = np.concatenate([posed(m8, rng, shown8[s]), posed(m3, rng, shown3[s]), rng.uniform(-1.5, 1.5, (3, 3))])
        lists.append(pts[rng.permutation(len(pts))] + rng.normal(scale=rr.NOISE, size=pts.shape))
    xyz, n = steps_of(lists, 16)
    got = check(ctx, xyz, n, [m3, m8], "M", min_markers=5)
    assert got["status"][:, 1].tolist() == [0, 0, rr.LOST, 0] and got["n_in"][:, 1].tolist() == [8, 5, 0, 8]
    assert (got["status"][:, 0] == rr.LOST).all()  # a triangle never has five inliers
    got = check(ctx, xyz, n, [m3, m8], "M", min_markers=3)
    assert got["status"][:, 0].tolist() == [0, 0, 0, rr.LOST] and got["n_in"][:, 1].tolist() == [8, 5, 4, 8]
    assert (got["label"][:, 0, 3:] == -1).all()


def test_an_isosceles_tie_and_duplicate_detections(ctx):
    """Exact ties: an isosceles triangle and its mirror image both fit with rms 0 and (h, i, j, k) decides; a detection reported
    twice (distance 0 to its twin) doubles the candidates, and the lower row is the label"""
    iso = np.array([[-0.1, 0, 0], [0.1, 0, 0], [0, 0.15, 0]])
    xyz, n = steps_of([iso, iso[[1, 0, 2]], iso[[0, 1, 1, 2, 0]]], 6)
    got = check(ctx, xyz, n, [iso], "ties")
    assert got["status"][:, 0].tolist() == [0, 0, 0] and (got["rms"][:, 0] == 0.0).all()
    assert got["label"][:, 0, :3].tolist() == [[0, 1, 2], [0, 1, 2], [0, 1, 3]]
    sc = rr.rigid_scene(4, T=2, hidden=0.0)
    twin = sc["xyz"].copy()
    n2 = sc["n"] + 1
    for s in range(2):
        twin[s, sc["n"][s]] = twin[s, sc["row"][s, 1, 2]]
    got = check(ctx, twin, n2, sc["models"], "twins")
    assert np.array_equal(got["label"], run_ref(sc["xyz"], sc["n"], sc["models"])["label"]) and (got["status"] == 0).all()


def test_exactly_max_hyp_candidates_and_one_more(ctx):
    """A regular tetrahedron holds 24 ordered triples for an equilateral model: max_hyp = 24 is a result, 23 is MOCAP_RIGID_E_HYP for
    that body in that step alone -- the neighbouring bodies and steps are bit for bit what they were"""
    sc = rr.rigid_scene(5, T=3)
    tet, tri_model = rr.lattice_case()
    xyz, n = sc["xyz"].copy(), sc["n"].copy()
    xyz[1, n[1]:n[1] + 4] = tet + 5.0
    n[1] += 4
    models = [sc["models"][0], tri_model, sc["models"][2]]
    fits = check(ctx, xyz, n, models, "24", max_hyp=24)
    assert fits["status"][1, 1] == 0 and fits["n_in"][1, 1] == 3 and fits["status"][[0, 2], 1].tolist() == [rr.LOST, rr.LOST]
    assert (fits["status"][:, [0, 2]] == 0).sum() >= 4
    over = check(ctx, xyz, n, models, "23", max_hyp=23)
    assert over["status"][1, 1] == rr.E_HYP and over["n_in"][1, 1] == 0 and (over["label"][1, 1] == -1).all()
    rest = np.ones((3, 3), bool)
    rest[1, 1] = False
    for k in INTS:
        assert np.array_equal(over[k][rest], fits[k][rest]), k
    ok = rest & (fits["status"] == 0)
    for k in FLOATS:
        assert np.array_equal(over[k][ok].view(np.uint64), fits[k][ok].view(np.uint64)), k


# ---- candidate lists of many trips of the 256 lanes (the constructions and their counts: rigid_ref, test_rigid_host) ---------------
LONG_MODELS = [rr.SQUARE, rr.TRIANGLE]


@pytest.fixture(scope="module")
def lattice_want():
    """The restatement on the exact and the noisy lattice (T = 2) for the square and the triangle: 3456 and 864 candidates each.
    A result does not depend on max_hyp once the list fits, so the tests below share this one."""
    xyz, n = rr.lattice_steps()
    want = run_ref(xyz, n, LONG_MODELS, max_hyp=rr.MAX_HYP)
    assert (want["status"] == 0).all() and want["n_in"].tolist() == [[4, 3], [4, 3]]
    assert (want["rms"][0] == 0.0).all() and (want["rms"][1] > 0.0).all()
    return xyz, n, want


def test_lists_of_3456_and_864_candidates(ctx, lattice_want):
    """Every lane evaluates 13 or 14 candidates of the square and 3 or 4 of the triangle and keeps its best.  Exact lattice: 912
    candidates tie at rms 0 and the winner, the fourth in (h, i, j, k) order, can stand anywhere in the list.  Noisy lattice: rms^2
    decides among candidates that label different detections."""
    xyz, n, want = lattice_want
    assert_same(run_gpu(ctx, xyz, n, LONG_MODELS, max_hyp=rr.MAX_HYP), want, "lattice")


def test_3456_candidates_at_max_hyp_and_one_more(ctx, lattice_want):
    xyz, n, want = lattice_want
    fits = run_gpu(ctx, xyz, n, [rr.SQUARE], max_hyp=rr.N_SQUARE)
    assert_same(fits, {k: v[:, :1] for k, v in want.items()}, "3456")
    over = check(ctx, xyz, n, [rr.SQUARE], "3455", max_hyp=rr.N_SQUARE - 1)
    assert (over["status"] == rr.E_HYP).all() and (over["n_in"] == 0).all() and (over["label"] == -1).all()


@pytest.mark.parametrize("B", [3, 4])
def test_a_list_beyond_the_lds_leaves_its_neighbours_untouched(ctx, lattice_want, B):
    """The cube's 46 656 candidates against max_hyp = 4096, the size of the LDS list itself: MOCAP_RIGID_E_HYP for that body in both
    steps, and every other body and step is bit for bit what it is in a call without the cube (and what the restatement says)."""
    xyz, n, want = lattice_want
    models = [rr.SQUARE, rr.CUBE, rr.TRIANGLE] + [rr.SQUARE] * (B - 3)
    got = run_gpu(ctx, xyz, n, models, max_hyp=rr.MAX_HYP)
    assert (got["status"][:, 1] == rr.E_HYP).all() and (got["n_in"][:, 1] == 0).all() and (got["label"][:, 1] == -1).all()
    keep = [b for b in range(B) if b != 1]
    rest = {k: v[:, keep] for k, v in got.items()}
    alone = run_gpu(ctx, xyz, n, [models[b] for b in keep], max_hyp=rr.MAX_HYP)
    assert (alone["status"] == 0).all()
    for k in INTS + FLOATS:
        assert rest[k].tobytes() == alone[k].tobytes(), k
    assert_same(rest, {k: v[:, [0, 1] + [0] * (B - 3)] for k, v in want.items()}, "beside the cube")  # columns of LONG_MODELS


@pytest.mark.parametrize("k,count", [(10, 240), (11, 264)])
def test_one_trip_of_the_lanes_and_eight_candidates_more(ctx, k, count):
    """10 tetrahedra: 240 candidates, one each for 240 lanes; 11: 264, eight lanes take a second.  max_hyp at the count and one below.
    (Which eight candidates come second is the list's business: a kernel that forgot them fails here only when the winner is among
    them, and fails test_lists_of_3456_and_864_candidates always.)"""
    det, model = rr.tetrahedra(k)
    xyz, n = steps_of([det], 64)
    fits = check(ctx, xyz, n, [model], f"{count}", max_hyp=count)
    assert fits["status"][0, 0] == 0 and fits["label"][0, 0, :3].tolist() == [0, 1, 2] and fits["rms"][0, 0] == 0.0
    over = check(ctx, xyz, n, [model], f"{count - 1}", max_hyp=count - 1)
    assert over["status"][0, 0] == rr.E_HYP and over["n_in"][0, 0] == 0 and (over["label"][0, 0] == -1).all()


def test_the_lists_arrival_order_does_not_show(ctx, lattice_want):
    """The list's order differs from run to run (an LDS atomic hands out its places); no byte of the output may"""
    xyz, n, _ = lattice_want
    a, b = (run_gpu(ctx, xyz[:1], n[:1], [rr.SQUARE], max_hyp=rr.MAX_HYP) for _ in range(2))
    assert (a["status"] == 0).all()
    for k in INTS + FLOATS:
        assert a[k].tobytes() == b[k].tobytes(), k


def test_bad_arguments_launch_nothing_and_bad_tables_are_reported(ctx, scene):
    import torch
    from mocapv2_amd import _abi
    sc, want = scene
    xyz, n = torch.from_numpy(sc["xyz"]).cuda(), torch.from_numpy(sc["n"]).cuda()
    bodies = ctx.rigid_bodies(sc["models"], rr.MIN_AREA)
    out = ctx.rigid_poses(xyz, n, bodies, rr.TOL, rr.GATE)
    out["status"].fill_(77)
    for kw in ({"tol": 0.0}, {"tol": float("nan")}, {"gate": -1.0}, {"gate": float("inf")}, {"min_markers": 2}, {"min_markers": 9},
               {"max_hyp": 0}, {"max_hyp": 4097}):
        with pytest.raises(_abi.MocapError) as e:
            ctx.rigid_poses(xyz, n, bodies, **{"tol": rr.TOL, "gate": rr.GATE, **kw}, out=out)
        assert e.value.code == -1
    many = {k: (torch.cat([v] * 6)[:17].contiguous() if torch.is_tensor(v) else v) for k, v in bodies.items()}
    with pytest.raises(_abi.MocapError) as e:
        ctx.rigid_poses(xyz, n, many, rr.TOL, rr.GATE)
    assert e.value.code == -1
    with pytest.raises(ValueError):
        ctx.rigid_bodies([m[:2] for m in sc["models"]])
    ctx.rigid_poses(xyz[:0], n[:0], bodies, rr.TOL, rr.GATE)  # T = 0: a no-op
    torch.cuda.synchronize()
    assert (out["status"] == 77).all()
    # a table that is no model: the body says so in every step, its neighbours are untouched
    broken = dict(bodies)
    broken["tri"] = bodies["tri"].clone()
    broken["tri"][1, 3, 2] = 5  # body 1 has markers 0..4
    got = {k: v.cpu().numpy() for k, v in ctx.rigid_poses(xyz, n, broken, rr.TOL, rr.GATE).items()}
    assert (got["status"][:, 1] == rr.E_MODEL).all() and (got["n_in"][:, 1] == 0).all() and (got["label"][:, 1] == -1).all()
    keep = {k: v[:, [0, 2]] for k, v in want.items()}
    assert_same({k: v[:, [0, 2]] for k, v in got.items()}, keep, "neighbours")


# ---- trackers ------------------------------------------------------------------------------------------------------------------
PW, PH, PC, PT = 640, 480, 3, 4
SUBPIX = {"radius": 24, "floor": 64}
BODY_TOL, BODY_GATE = 0.002, 0.004
MEASURED_ANGLE, MEASURED_TRANSLATION = 0.0000479, 0.00002119  # rad, world units: the worst of the 4 steps on the MI355X


@pytest.fixture(scope="module")
def rendered_body():
    """One body of 4 markers on 4 poses (a few degrees and centimetres apart), rendered as discs into 3 cameras"""
    from mocapv2_amd import synth
    scene = synth.Scene(PC, PW, PH, dist=synth.MILD_DIST)
    first = sref.place_markers(scene, np.random.default_rng(70), 4, margin=SUBPIX["radius"] + 30, apart=2 * SUBPIX["radius"] + 12)
    centre = first.mean(axis=0)
    model = first - centre
    frames = np.empty((PT, PC, PH, PW), np.uint8)
    Rs, ts = [], []
    for s in range(PT):
        a = 0.03 * s
        R = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])
        t = centre + np.array([0.004 * s, -0.003 * s, 0.002 * s])
        markers = model @ R.T + t
        rng = np.random.default_rng(170 + s)
        for c in range(PC):
            px = scene.pixels(markers, c)
            gaps = np.abs(px[:, None] - px[None]).max(axis=2)[np.triu_indices(4, 1)]
            assert gaps.min() > 2 * SUBPIX["radius"] + 2 and (px > SUBPIX["radius"] + 22).all(), (s, c)
            frames[s, c] = scene.render(rng, markers, c, radius_range=(15.0, 19.0))
        Rs.append(R)
        ts.append(t)
    return scene, frames, model, np.array(Rs), np.array(ts)


def test_trackers_find_the_rendered_body(rendered_body):
    """BatchTracker(bodies=...) and ReplayTracker(bodies=...) with visibility="any" and sub-pixel centroids: the body is found in
    every step with all four markers, its labels are the rows of its markers, its pose is the truth's within twice what was
    measured (per step on the MI355X: 0.0000220, 0.0000345, 0.0000479, 0.0000379 rad and 0.01269, 0.02119, 0.01898, 0.01166 mm; rms
    of the fit at most 0.03552 mm), the device outputs are the
    restatement's on the read-back markers, and the messages carry q and t."""
    import torch
    from mocapv2_amd.pipeline import BatchTracker, scene_arrays
    from mocapv2_amd.replay import ReplayTracker, unpack_rigid_message
    scene, frames, model, Rs, ts = rendered_body
    K, dist, R, t, F = scene_arrays(scene)
    bodies = {"models": [model], "tol": BODY_TOL, "gate": BODY_GATE, "names": ["wand"]}
    trk = BatchTracker(K, dist, R, t, None, PW, PH, PT, visibility="any", subpixel=SUBPIX, bodies=bodies)
    out = trk.step(torch.from_numpy(frames.reshape(PT * PC, PH, PW)).cuda())
    n = trk.finish(out)
    got = {k: v.cpu().numpy() for k, v in out.items()}
    assert n.tolist() == [4] * PT
    assert got["body_status"].tolist() == [[0]] * PT and got["body_n"].tolist() == [[4]] * PT
    want = rr.rigid_poses(got["xyz"], got["n"], [model], [rr.triples_of(model, rr.MIN_AREA)], BODY_TOL, BODY_GATE)
    assert_same({k: got[v] for k, v in BatchTracker.BODY_KEYS.items()}, want, "tracker")
    worst = [0.0, 0.0]
    for s in range(PT):
        lab = got["body_label"][s, 0, :4]
        truth = model @ Rs[s].T + ts[s]
        assert np.abs(got["xyz"][s, lab] - truth).max() < 1e-3, s  # every label is the row of its own marker
        a, d = rr.pose_errors(got["body_R"][s, 0], got["body_t"][s, 0], Rs[s], ts[s])
        worst = [max(worst[0], a), max(worst[1], d)]
    print(f"worst pose against truth: {worst[0]:.6f} rad, {worst[1] * 1e3:.4f} mm; rms {got['body_rms'].max() * 1e3:.4f} mm")
    assert worst[0] <= 2 * MEASURED_ANGLE and worst[1] <= 2 * MEASURED_TRANSLATION, worst

    # the replay: 4 steps in batches of 3 (one padded), host arrays and messages
    kw = dict(batch=3, visibility="any", subpixel=SUBPIX)
    res = list(ReplayTracker(K, dist, R, t, None, PW, PH, bodies=bodies, **kw).run_batches(frames))
    assert [b["n_steps"] for b in res] == [3, 1]
    for key in BatchTracker.BODY_KEYS.values():
        assert np.array_equal(np.concatenate([b[key] for b in res]), got[key]), key
    msgs = [m for b in res for m in b["body_messages"]]
    assert len(msgs) == PT and all(len(m) == 1 for m in msgs)
    for s in range(PT):
        assert unpack_rigid_message(msgs[s][0]) == ("wand", got["body_q"][s, 0].tolist(), got["body_t"][s, 0].tolist())
    # bodies=None is the path as it was: no body_* key anywhere, the same tracker messages
    plain = list(ReplayTracker(K, dist, R, t, None, PW, PH, **kw).run_batches(frames))
    with_none = list(ReplayTracker(K, dist, R, t, None, PW, PH, bodies=None, **kw).run_batches(frames))
    for a, b, c in zip(plain, with_none, res):
        assert not [k for k in list(a) + list(b) if k.startswith("body_")]
        assert a["messages"] == b["messages"] == c["messages"] and sorted(a) == sorted(b)
    one = BatchTracker(K, dist, R, t, None, PW, PH, PT, visibility="any", subpixel=SUBPIX)
    assert not [k for k in one.step(torch.from_numpy(frames.reshape(PT * PC, PH, PW)).cuda()) if k.startswith("body_")]
    steps = list(ReplayTracker(K, dist, R, t, None, PW, PH, bodies=bodies, **kw).run(frames))
    assert [s["body_messages"] for s in steps] == msgs and all(s["body_n"].tolist() == [4] for s in steps)


def test_a_body_that_disappears_repeats_its_message(rendered_body):
    """visibility="all" (the rows are positions in `order`), and frames 2 and 3 black: the body is lost there and its message stays"""
    from mocapv2_amd.pipeline import scene_arrays
    from mocapv2_amd.replay import ReplayTracker, rigid_message
    scene, frames, model, Rs, ts = rendered_body
    K, dist, R, t, F = scene_arrays(scene)
    dark = frames.copy()
    dark[2:] = 0
    bodies = {"models": [model], "tol": BODY_TOL, "gate": BODY_GATE}
    (res,) = list(ReplayTracker(K, dist, R, t, F, PW, PH, batch=4, visibility="all", subpixel=SUBPIX, bodies=bodies).run_batches(dark))
    assert res["body_status"][:, 0].tolist() == [0, 0, rr.LOST, rr.LOST] and res["body_n"][:, 0].tolist() == [4, 4, 0, 0]
    for s in range(2):
        a, d = rr.pose_errors(res["body_R"][s, 0], res["body_t"][s, 0], Rs[s], ts[s])
        assert a <= 2 * MEASURED_ANGLE and d <= 2 * MEASURED_TRANSLATION, (s, a, d)
    m = [b[0] for b in res["body_messages"]]
    assert m[1] == m[2] == m[3] == rigid_message("body1", res["body_q"][1, 0], res["body_t"][1, 0]) and m[0] != m[1]


def test_two_ranks_and_two_batches_in_flight_give_the_single_trackers_poses(rendered_body):
    """bodies with depth = 2 and with world = 2 (each rank solves its own time steps; both ranks run on one GPU here, the all-gather
    replaced by the concatenation it produces): the poses of the one-rank tracker with one batch in flight, bit for bit.  Integer
    centroids (subpixel needs world == 1), hence the wider tol and gate."""
    import torch
    from mocapv2_amd.pipeline import BatchTracker, scene_arrays
    scene, frames, model, _, _ = rendered_body
    arrays = scene_arrays(scene)
    kw = dict(visibility="any", bodies={"models": [model], "tol": 0.03, "gate": 0.03})
    keys = list(BatchTracker.BODY_KEYS.values())
    dev = torch.from_numpy(frames.reshape(PT * PC, PH, PW)).cuda()
    ref = BatchTracker(*arrays, PW, PH, PT, **kw)
    want = {k: v.cpu().numpy() for k, v in ref.step(dev).items()}
    assert want["body_status"].tolist() == [[0]] * PT and want["body_n"].tolist() == [[4]] * PT
    deep = BatchTracker(*arrays, PW, PH, PT, depth=2, **kw)
    outs = [deep.step(dev) for _ in range(2)]
    deep.synchronize()
    for out in outs:
        for k in keys:
            assert out[k].cpu().numpy().tobytes() == want[k].tobytes(), k
    world, T = 2, PT // 2
    ranks = [BatchTracker(*arrays, PW, PH, T, world=world, rank=r, **kw) for r in range(world)]
    recs = [tr.extract(torch.from_numpy(np.stack([frames[t, c] for c, t in tr.local_image_list()])).cuda()).clone() for tr in ranks]
    gathered = torch.cat(recs, dim=0)
    for r, tr in enumerate(ranks):
        out = tr.body_poses(tr.triangulate(gathered))
        for k in keys:
            assert out[k].cpu().numpy().tobytes() == want[k][r * T:(r + 1) * T].tobytes(), (r, k)
