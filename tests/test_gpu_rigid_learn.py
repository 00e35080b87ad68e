"""mocap_learn_marker_pair_stats and mocap_learn_rigid_bodies on the GPU against their NumPy restatement (tests/rigid_learn_ref.py).

Integers are compared for EQUALITY everywhere; the floats as 64-bit patterns -- the pair tables everywhere, the models and their
rms wherever the group's status is 0 (elsewhere they are unspecified).  The definition fixes every operation and the order of every
sum (chunks of 32 steps), uses + - * / and sqrt only, and the library is built without fused multiply-adds, so there is no
tolerance anywhere.

The tracker-level test learns one body of 4 discs from rendered frames (3 cameras at 640 x 480, sub-pixel centroids, 5 poses) and
tracks it with what it learned; its bound against the scene's model is twice what was measured on the MI355X (docstring of
test_a_replay_tracker_learns_the_rendered_body_and_tracks_it)."""
import numpy as np
import pytest

import rigid_learn_ref as rl
import rigid_ref as rr
import subpixel_ref as sref

pytestmark = pytest.mark.gpu

PAIR_KEYS = ("count", "dmin", "dmax", "dsum", "dsum2")
LEARN_INTS, LEARN_FLOATS = ("status", "ref_step", "steps_used", "member_count"), ("model", "rms", "member_rms")
LONG = 32 * 257 + 5


@pytest.fixture(scope="module")
def ctx():
    from mocapv2_amd.engine import MocapContext
    return MocapContext(1, 1)


@pytest.fixture(scope="module")
def tk3():
    return rl.take(3, T=65)


def on_device(tk):
    import torch
    return (torch.from_numpy(np.ascontiguousarray(tk["xyz"], np.float64)).cuda(), torch.from_numpy(np.ascontiguousarray(tk["n"], np.int32)).cuda(),
            torch.from_numpy(np.ascontiguousarray(tk["id"], np.int32)).cuda())


def host(out):
    import torch
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def cut(tk, T):
    return dict(tk, xyz=tk["xyz"][:T].copy(), n=tk["n"][:T].copy(), id=tk["id"][:T].copy())


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def same_pairs(got, want, what=""):
    assert got["count"].dtype == np.int32
    for k in PAIR_KEYS:
        g, w = (got[k], want[k]) if k == "count" else (bits(got[k]), bits(want[k]))
        bad = np.argwhere(g != w)
        assert len(bad) == 0, (what, k, bad[:4].tolist(), got[k][tuple(bad[0])], want[k][tuple(bad[0])])


def same_learn(got, want, what=""):
    for k in LEARN_INTS:
        assert np.array_equal(got[k], want[k]), (what, k, got[k].tolist(), want[k].tolist())
    ok = want["status"] == 0
    for k in LEARN_FLOATS:
        g, w = bits(got[k][ok]), bits(want[k][ok])
        bad = np.argwhere(g != w)
        assert len(bad) == 0, (what, k, bad[:4].tolist(), got[k][ok][tuple(bad[0])], want[k][ok][tuple(bad[0])])


def check_pairs(ctx, tk, ids, what=""):
    got = host(ctx.marker_pair_stats(*on_device(tk), ids))
    same_pairs(got, rl.pair_stats(tk["xyz"], tk["n"], tk["id"], ids), what)
    return got


def check_learn(ctx, tk, members, what="", **kw):
    got = host(ctx.rigid_learn(*on_device(tk), members, **kw))
    same_learn(got, rl.rigid_learn(tk["xyz"], tk["n"], tk["id"], members, **kw), what)
    return got


def body_ids(tk):
    return np.array(sorted(sum(rl.truth_members(tk), [])), np.int32)


def test_the_seeded_take_with_nan_beyond_the_counts(ctx, tk3):
    tk = cut(tk3, 60)
    assert np.isnan(tk["xyz"][0, tk["n"][0]:]).all()
    ids = rl.frequent_ids(tk["n"], tk["id"], rl.MIN_STEPS)
    assert ids.tolist() == body_ids(tk).tolist()
    pairs = check_pairs(ctx, tk, ids)
    assert pairs["count"].max() > 40 and np.isfinite(pairs["dsum2"]).all()
    got = check_learn(ctx, tk, rl.truth_members(tk))
    assert got["status"].tolist() == [0, 0, 0] and np.isfinite(got["model"]).all() and got["member_count"][:, :4].min() >= 25
    # identities beyond the counts are no identities either
    junk = dict(tk, id=tk["id"].copy())
    for s in range(60):
        junk["id"][s, tk["n"][s]:] = 0
    same_pairs(host(ctx.marker_pair_stats(*on_device(junk), ids)), pairs, "junk identities beyond n")
    same_learn(host(ctx.rigid_learn(*on_device(junk), rl.truth_members(tk))), got, "junk identities beyond n")


@pytest.mark.parametrize("T", [1, 31, 32, 33, 65])
def test_the_chunk_seams(ctx, tk3, T):
    tk = cut(tk3, T)
    check_pairs(ctx, tk, body_ids(tk), T)
    got = check_learn(ctx, tk, rl.truth_members(tk), T)
    if T >= 31:
        assert got["status"].tolist() == [0, 0, 0]


def test_a_long_take_of_257_chunks_and_five_steps(ctx, tk3):
    tk = rl.tiled(cut(tk3, 60), LONG)
    assert len(tk["n"]) == LONG == 8229
    pairs = check_pairs(ctx, tk, body_ids(tk), "long")
    assert pairs["count"].max() > 6000
    got = check_learn(ctx, tk, rl.truth_members(tk), "long")
    assert got["status"].tolist() == [0, 0, 0] and got["steps_used"].min() > 6000


def test_two_identities_and_sixty_four_and_bad_lists(ctx, tk3):
    import torch
    from mocapv2_amd import _abi
    tk = cut(tk3, 60)
    check_pairs(ctx, tk, [0, 1], "K=2")
    clutter = np.unique(tk["id"][tk["id"] >= rl.CLUTTER_ID0])
    ids64 = np.concatenate([body_ids(tk), clutter[:49]]).astype(np.int32)
    assert len(ids64) == 64
    got = check_pairs(ctx, tk, ids64, "K=64")
    assert np.diag(got["count"])[15:].tolist() == [1] * 49  # a clutter identity lives one step
    # an identity that never appears: its row and column are zeros
    never = check_pairs(ctx, tk, [0, 1, 2, 999999], "never")
    assert not never["count"][3].any() and not never["dmax"][:, 3].any()
    out = ctx.marker_pair_stats(*on_device(tk), ids64)
    for v in out.values():
        v.fill_(77)
    shaped = lambda K: {k: torch.full((K, K), 77, dtype=v.dtype, device=v.device) for k, v in out.items()}
    for bad in (np.concatenate([ids64, [5000000]]), [3, 2, 1], [1, 1, 2], [-1, 2, 3], [7]):
        o = shaped(len(bad))
        with pytest.raises(_abi.MocapError) as e:
            ctx.marker_pair_stats(*on_device(tk), bad, out=o)
        assert e.value.code == -1
        torch.cuda.synchronize()
        assert all((v == 77).all() for v in o.values())
    # T = 0 zeroes the outputs
    xyz, n, ident = on_device(tk)
    zero = host(ctx.marker_pair_stats(xyz[:0], n[:0], ident[:0], ids64, out=out))
    assert all(not v.any() for v in zero.values())


@pytest.mark.parametrize("G", [1, 16])
def test_one_group_and_sixteen(ctx, tk3, G):
    from itertools import combinations
    tk = cut(tk3, 60)
    members = (rl.truth_members(tk) + [[20 + p for p in c] for c in combinations(range(6), 3)])[:G]
    if G == 1:
        members = [rl.truth_members(tk)[1]]
    got = check_learn(ctx, tk, members, G)
    assert len(got["status"]) == G and (got["status"] == 0).all()


def test_bodies_of_three_and_of_eight_members(ctx):
    tk = rl.take_three_and_eight()
    got = check_learn(ctx, tk, rl.truth_members(tk), "3 and 8")
    assert got["status"].tolist() == [0, 0] and (got["member_count"][1] > 0).all() and not got["model"][0, 3:].any()
    check_pairs(ctx, tk, body_ids(tk), "3 and 8")
    check_learn(ctx, tk, rl.truth_members(tk), "all eight present", min_present=8)


@pytest.mark.parametrize("rounds", [1, 4])
def test_one_round_and_four(ctx, tk3, rounds):
    tk = cut(tk3, 60)
    got = check_learn(ctx, tk, rl.truth_members(tk), rounds, rounds=rounds)
    assert (got["status"] == 0).all()


def test_a_step_one_member_short_is_not_used_and_a_member_seen_once(ctx, tk3):
    tk = cut(tk3, 60)
    six = rl.truth_members(tk)[2]
    present = (rl.locate(tk["n"], tk["id"], six) >= 0).sum(axis=1)
    assert (present == 4).any() and (present >= 5).any()
    got = check_learn(ctx, tk, [six], "min_present 5", min_present=5)
    assert got["steps_used"].tolist() == [int((present >= 5).sum())] and got["steps_used"][0] < int((present >= 4).sum())
    # member 3 of body 0 keeps its identity at the reference step only
    four = rl.truth_members(tk)[0]
    ref = int(np.flatnonzero((rl.locate(tk["n"], tk["id"], four) >= 0).all(axis=1))[0])
    once = dict(tk, id=tk["id"].copy())
    lost = once["id"] == four[3]
    lost[ref] = False
    once["id"][lost] = -1
    got = check_learn(ctx, once, [four], "seen once")
    assert got["status"].tolist() == [0] and got["ref_step"].tolist() == [ref] and got["member_count"][0, :4].tolist()[3] == 1


def test_an_identity_twice_in_a_step_counts_at_its_lower_row(ctx, tk3):
    tk = cut(tk3, 60)
    twice = dict(tk, id=tk["id"].copy())
    moved = 0
    for s in range(60):
        rows = np.flatnonzero(twice["id"][s] == 0)
        stray = np.flatnonzero(twice["id"][s] >= rl.CLUTTER_ID0)
        if len(rows) and len(stray):
            twice["id"][s, stray[0]] = 0
            moved += stray[0] < rows[0]
    assert moved >= 5
    check_pairs(ctx, twice, body_ids(tk), "twice")
    check_learn(ctx, twice, rl.truth_members(tk), "twice")


def test_blind_steps_of_both_kinds(ctx, tk3):
    tk = cut(tk3, 60)
    blind = dict(tk, n=tk["n"].copy())
    members = rl.truth_members(tk)
    first = int(np.flatnonzero((rl.locate(tk["n"], tk["id"], members[0]) >= 0).all(axis=1))[0])
    blind["n"][first], blind["n"][first + 1], blind["n"][40] = -4, tk["xyz"].shape[1] + 1, -2
    pairs = check_pairs(ctx, blind, body_ids(tk), "blind")
    assert pairs["count"][0, 0] < check_pairs(ctx, tk, body_ids(tk))["count"][0, 0]
    got = check_learn(ctx, blind, members, "blind")
    assert got["status"].tolist() == [0, 0, 0] and got["ref_step"][0] > first + 1


def test_group_statuses_leave_the_neighbours_alone(ctx, tk3):
    tk = cut(tk3, 60)
    a, b, c = rl.truth_members(tk)
    plain = check_learn(ctx, tk, [a, b, c])
    got = check_learn(ctx, tk, [a, [0, 1, 999999], b, [10, 11, 11], c, [0, 1], [0, -1, 2]], "statuses")
    assert got["status"].tolist() == [0, rl.E_INCOMPLETE, 0, rl.E_MEMBERS, 0, rl.E_MEMBERS, rl.E_MEMBERS]
    bad = got["status"] != 0
    assert (got["ref_step"][bad] == -1).all() and not got["member_count"][bad].any() and not got["steps_used"][bad].any()
    same_learn({k: v[[0, 2, 4]] for k, v in got.items()}, plain, "neighbours")
    assert check_learn(ctx, tk, [a[:3]], min_present=4)["status"].tolist() == [rl.E_MEMBERS]
    # T = 0: no group has a reference step
    xyz, n, ident = on_device(tk)
    assert host(ctx.rigid_learn(xyz[:0], n[:0], ident[:0], [a, b]))["status"].tolist() == [rl.E_INCOMPLETE] * 2


def test_bad_arguments_launch_nothing(ctx, tk3):
    import torch
    from mocapv2_amd import _abi
    tk = cut(tk3, 60)
    dev, members = on_device(tk), rl.truth_members(tk)
    out = ctx.rigid_learn(*dev, members)
    out["status"].fill_(77)
    for kw in ({"rounds": 0}, {"rounds": 5}, {"min_present": 2}, {"min_present": 9}):
        with pytest.raises(_abi.MocapError) as e:
            ctx.rigid_learn(*dev, members, **kw, out=out)
        assert e.value.code == -1
    for G in (0, 17):
        with pytest.raises(_abi.MocapError) as e:
            ctx.rigid_learn(*dev, [members[0]] * G)
        assert e.value.code == -1
    torch.cuda.synchronize()
    assert (out["status"] == 77).all()


def test_the_same_calls_twice_give_the_same_bits(ctx, tk3):
    tk = rl.tiled(cut(tk3, 60), 300)
    dev, ids, members = on_device(tk), body_ids(tk), rl.truth_members(tk)
    p1, p2 = host(ctx.marker_pair_stats(*dev, ids)), host(ctx.marker_pair_stats(*dev, ids))
    l1, l2 = host(ctx.rigid_learn(*dev, members)), host(ctx.rigid_learn(*dev, members))
    same_pairs(p1, p2)
    for k in LEARN_INTS + LEARN_FLOATS:
        assert np.array_equal(bits(l1[k]) if k in LEARN_FLOATS else l1[k], bits(l2[k]) if k in LEARN_FLOATS else l2[k]), k


@pytest.mark.parametrize("seed", [3, 4])
def test_learn_rigid_bodies_end_to_end(ctx, seed):
    import torch
    tk = rl.take(seed)
    dev = on_device(tk)
    res = ctx.learn_rigid_bodies(*dev, spread=rl.SPREAD, min_steps=rl.MIN_STEPS)
    assert res["members"] == rl.truth_members(tk) and res["unassigned"] == [] and res["names"] == ["body1", "body2", "body3"]
    assert res["status"].tolist() == [0, 0, 0] and res["ids"].tolist() == body_ids(tk).tolist()
    same_pairs(res["pairs"], rl.pair_stats(tk["xyz"], tk["n"], tk["id"], res["ids"]), "e2e")
    want = rl.rigid_learn(tk["xyz"], tk["n"], tk["id"], res["members"])
    for g, m in enumerate(res["models"]):
        assert m.shape == (len(tk["models"][g]), 3) and np.array_equal(bits(m), bits(want["model"][g, :len(m)]))
        assert rl.aligned_error(m, tk["models"][g]).max() < rr.NOISE
    poses = []
    for models in (tk["models"], res["models"]):
        poses.append(host(ctx.rigid_poses(dev[0], dev[1], ctx.rigid_bodies(models, rr.MIN_AREA), rr.TOL, rr.GATE)))
    assert np.array_equal(poses[0]["status"], poses[1]["status"]) and np.array_equal(poses[0]["n_in"], poses[1]["n_in"])
    assert (poses[0]["status"] == 0).sum() > 120
    # the identities may be named, and a static take is refused
    named = ctx.learn_rigid_bodies(*dev, spread=rl.SPREAD, min_steps=rl.MIN_STEPS, ids=[0, 1, 2, 3, 10, 11], names=["wand"])
    assert named["members"] == [[0, 1, 2, 3]] and named["unassigned"] == [10, 11] and named["names"] == ["wand"]
    if seed == 3:
        with pytest.raises(ValueError, match="more than 8"):
            ctx.learn_rigid_bodies(*on_device(rl.static_take()), spread=rl.SPREAD, min_steps=rl.MIN_STEPS)
    torch.cuda.synchronize()


# ---- trackers ------------------------------------------------------------------------------------------------------------------
PW, PH, PC, PT = 640, 480, 3, 5
SUBPIX = {"radius": 24, "floor": 64}
BODY_TOL, BODY_GATE = 0.002, 0.004
TRACK = {"gate": 0.05, "max_tracks": 16}
MEASURED_MODEL = 0.00001043  # world units: the worst learned point against the scene's model on the MI355X


@pytest.fixture(scope="module")
def rendered_take():
    """One body of 4 markers on 5 poses (a few degrees and centimetres apart), rendered as discs into 3 cameras"""
    from mocapv2_amd import synth
    scene = synth.Scene(PC, PW, PH, dist=synth.MILD_DIST)
    first = sref.place_markers(scene, np.random.default_rng(70), 4, margin=SUBPIX["radius"] + 30, apart=2 * SUBPIX["radius"] + 12)
    centre = first.mean(axis=0)
    model = first - centre
    frames = np.empty((PT, PC, PH, PW), np.uint8)
    for s in range(PT):
        a = 0.03 * s
        R = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])
        markers = model @ R.T + centre + np.array([0.004 * s, -0.003 * s, 0.002 * s])
        rng = np.random.default_rng(270 + s)
        for c in range(PC):
            px = scene.pixels(markers, c)
            gaps = np.abs(px[:, None] - px[None]).max(axis=2)[np.triu_indices(4, 1)]
            assert gaps.min() > 2 * SUBPIX["radius"] + 2 and (px > SUBPIX["radius"] + 22).all(), (s, c)
            frames[s, c] = scene.render(rng, markers, c, radius_range=(15.0, 19.0))
    return scene, frames, model


def test_a_replay_tracker_learns_the_rendered_body_and_tracks_it(rendered_take):
    """ReplayTracker.learn_bodies on 5 rendered steps in batches of 3 (the last one padded): one body of four members, every member
    seen in all 5 steps.  Measured on the MI355X: the worst learned point lies 0.01043 mm from the scene's model after alignment
    (rms of the fit 0.02196 mm), far below tol = 2 mm; the bound is twice that.  A second tracker, given the learned model, finds the body
    with all four markers in every step."""
    from mocapv2_amd.pipeline import scene_arrays
    from mocapv2_amd.replay import ReplayTracker
    scene, frames, model = rendered_take
    K, dist, R, t, F = scene_arrays(scene)
    kw = dict(batch=3, visibility="any", subpixel=SUBPIX)
    res = ReplayTracker(K, dist, R, t, None, PW, PH, track=TRACK, **kw).learn_bodies(frames, spread=0.001, min_steps=3)
    assert len(res["models"]) == 1 and len(res["members"][0]) == 4 and res["unassigned"] == [] and res["status"].tolist() == [0]
    assert res["member_count"][0].tolist() == [PT] * 4 + [0] * 4 and res["steps_used"].tolist() == [PT]  # no padding frame took part
    learned = res["models"][0]
    # the members are identities in the order the tracker met the markers: match them to the scene's points by their distances
    best = min((rl.aligned_error(learned, model[list(p)]).max(), p) for p in __import__("itertools").permutations(range(4)))
    print(f"worst learned point against the scene's model: {best[0] * 1e3:.5f} mm; rms of the fit {res['rms'][0] * 1e3:.5f} mm")
    assert MEASURED_MODEL < BODY_TOL and best[0] <= 2 * MEASURED_MODEL, best
    bodies = {"models": res["models"], "tol": BODY_TOL, "gate": BODY_GATE}
    found = list(ReplayTracker(K, dist, R, t, None, PW, PH, bodies=bodies, **kw).run_batches(frames))
    assert [b["n_steps"] for b in found] == [3, 2]
    assert np.concatenate([b["body_status"] for b in found]).tolist() == [[0]] * PT
    assert np.concatenate([b["body_n"] for b in found]).tolist() == [[4]] * PT


def test_a_tracker_without_identities_cannot_learn(rendered_take):
    from mocapv2_amd.pipeline import scene_arrays
    from mocapv2_amd.replay import ReplayTracker
    scene, frames, _ = rendered_take
    K, dist, R, t, F = scene_arrays(scene)
    with pytest.raises(ValueError, match="track"):
        ReplayTracker(K, dist, R, t, None, PW, PH, batch=3, visibility="any", subpixel=SUBPIX).learn_bodies(frames, spread=0.001, min_steps=3)
