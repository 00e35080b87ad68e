"""mocap_track_markers on the GPU against its NumPy restatement (tests/track_ref.py).

Everything is compared for EQUALITY: id, slot, age, status, and the final state byte for byte (pos and vel as 64-bit patterns, the
dead slots' left-over fields included).  The definition fixes every operation and its order and the library is built without
fused multiply-adds, so there is no tolerance anywhere."""
import numpy as np
import pytest

import track_ref as tr

pytestmark = pytest.mark.gpu

GATE = 0.05


@pytest.fixture(scope="module")
def ctx():
    from mocapv2_amd.engine import MocapContext
    return MocapContext(1, 1)


def run_gpu(ctx, xyz, n, state, gate, **kw):
    """state: max_tracks, or the bytes of a state to go on from.  -> (outputs as arrays, the state's bytes after the call)"""
    import torch
    d_state = ctx.track_state(state) if isinstance(state, int) else torch.from_numpy(np.array(state, np.uint8)).cuda()
    out = ctx.track_markers(torch.from_numpy(np.ascontiguousarray(xyz, np.float64)).cuda(),
                            torch.from_numpy(np.ascontiguousarray(n, np.int32)).cuda(), d_state, gate, **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}, d_state.cpu().numpy()


def run_ref(xyz, n, state, gate, **kw):
    st = tr.new_state(state) if isinstance(state, int) else tr.split_state(np.array(state, np.uint8))
    out = tr.track(xyz, n, st, gate, **kw)
    return out, tr.join_state(*st)


def assert_same(got, want, what=""):
    (g, gs), (w, ws) = got, want
    for k in ("status", "id", "slot", "age"):
        bad = np.argwhere(g[k] != w[k])
        assert len(bad) == 0, (what, k, bad[:4].tolist(), g[k][tuple(bad[0])], w[k][tuple(bad[0])])
    if not np.array_equal(gs, ws):
        gh, gsl = tr.split_state(gs)
        wh, wsl = tr.split_state(ws)
        assert gh.tobytes() == wh.tobytes(), (what, gh, wh)
        s = int(np.flatnonzero([a.tobytes() != b.tobytes() for a, b in zip(gsl, wsl)])[0])
        raise AssertionError((what, "slot", s, gsl[s], wsl[s]))


def check(ctx, xyz, n, state, gate, what="", **kw):
    got, want = run_gpu(ctx, xyz, n, state, gate, **kw), run_ref(xyz, n, state, gate, **kw)
    assert_same(got, want, what)
    return got


@pytest.mark.parametrize("seed, speed", [(0, 0.8), (1, 0.5), (2, 0.8)])
def test_host_scenes(ctx, seed, speed):
    xyz, n, who, _, _ = tr.scene(seed, speed)
    out, _ = check(ctx, xyz, n, 16, GATE, what=f"scene {seed}")
    mixed, _ = tr.mixups_and_changes(out["id"], who, 8)
    assert mixed == [] and (out["id"] >= 0).sum() == n.sum()


def test_a_batch_split_into_calls_on_a_carried_state(ctx):
    xyz, n, _, _, _ = tr.scene(5, 0.8, T=300)
    whole, whole_state = check(ctx, xyz, n, 16, GATE, what="whole")
    state, parts, t0 = tr.join_state(*tr.new_state(16)), [], 0
    for T in (64, 1, 0, 235):
        if T == 0:  # a no-op that launches nothing: the state stays as it is, even with no arrays to point at
            import torch
            d_state = torch.from_numpy(state.copy()).cuda()
            empty = torch.empty((0, 16, 3), dtype=torch.float64, device="cuda")
            ctx.track_markers(empty, torch.empty((0,), dtype=torch.int32, device="cuda"), d_state, GATE)
            torch.cuda.synchronize()
            assert np.array_equal(d_state.cpu().numpy(), state)
            continue
        out, state = run_gpu(ctx, xyz[t0:t0 + T], n[t0:t0 + T], state, GATE)
        parts.append(out)
        t0 += T
    for k in ("id", "slot", "age", "status"):
        assert np.array_equal(np.concatenate([p[k] for p in parts]), whole[k]), k
    assert np.array_equal(state, whole_state)
    assert tr.split_state(state)[0]["steps"][0] == 300


@pytest.mark.parametrize("case", ["lattice", "crowd"])
def test_exact_ties_and_several_rounds(ctx, case):
    xyz, n, gate = tr.lattice_case() if case == "lattice" else tr.crowd_case()
    check(ctx, xyz, n, 16, gate, what=case)


def test_rows_beyond_the_count_take_no_part(ctx):
    xyz, n, _, _, _ = tr.scene(4, 0.8, T=64)
    clean = np.where(np.isnan(xyz), 0.0, xyz)
    a, sa = check(ctx, clean, n, 16, GATE, what="clean")
    for poison in (np.nan, 1e300):
        bad = clean.copy()
        for t in range(len(n)):
            bad[t, n[t]:] = poison
        b, sb = run_gpu(ctx, bad, n, 16, GATE)
        assert_same((b, sb), (a, sa), what=f"poison {poison}")
    for t in range(len(n)):
        for k in ("id", "slot", "age"):
            assert (a[k][t, n[t]:] == -1).all() and (a[k][t, :n[t]] >= 0).all()


def test_more_markers_than_slots(ctx):
    """M = 4, six markers: every step is FULL, exactly the two highest rows get -1 (the four first-born keep their tracks,
    whatever the rows' order), and tracking goes on."""
    rng = np.random.default_rng(3)
    base = np.stack([np.arange(6) * 1.0, np.zeros(6), np.zeros(6)], axis=1)
    T = 12
    xyz = np.zeros((T, 8, 3))
    n = np.full(T, 6, np.int32)
    for t in range(T):
        xyz[t, :6] = base + 0.01 * t
    out, _ = check(ctx, xyz, n, 4, 0.2, what="full")
    assert (out["status"] == tr.E_FULL).all()
    for t in range(T):
        assert out["id"][t, :6].tolist() == [0, 1, 2, 3, -1, -1] and out["slot"][t, 4:6].tolist() == [-1, -1]
        assert out["age"][t, :4].tolist() == [t + 1] * 4
    # the rows shuffled from step 1 on: the tracked four keep their identities, the other two rows hold -1
    for t in range(1, T):
        perm = rng.permutation(6)
        xyz[t, :6] = xyz[t, :6][perm]
    out, _ = check(ctx, xyz, n, 4, 0.2, what="full, shuffled")
    assert all(sorted(out["id"][t, :6].tolist()) == [-1, -1, 0, 1, 2, 3] for t in range(T))


def test_blind_steps_carry_their_code_and_the_tracks_coast(ctx):
    xyz, n, _, _, _ = tr.scene(6, 0.5, T=40, Q=300)
    n = n.copy()
    n[10], n[11], n[25] = -2, 257, -5
    out, _ = check(ctx, xyz, n, 16, GATE, what="blind")
    assert out["status"][[10, 11, 25]].tolist() == [tr.E_INPUT, tr.E_COUNT, tr.E_INPUT]
    assert (out["status"][[9, 12, 24, 26]] == 0).all()
    for t in (10, 11, 25):
        assert (out["id"][t] == -1).all() and (out["slot"][t] == -1).all() and (out["age"][t] == -1).all()
    # the tracks coasted through: the step after two blind ones continues identities from before them
    before, after = set(out["id"][9, :n[9]].tolist()), set(out["id"][12, :n[12]].tolist())
    assert len(before & after) >= 5
    # a count above the rows of a step is blind too (Q = 4 < 5)
    small = np.zeros((3, 4, 3))
    out, _ = check(ctx, small, np.array([2, 5, 2], np.int32), 8, GATE, what="n > Q")
    assert out["status"].tolist() == [0, tr.E_COUNT, 0]


def test_the_identity_counter_stops_at_int32_max(ctx):
    head, slots = tr.new_state(8)
    head["next_id"][0] = tr.INT32_MAX - 1
    xyz = np.zeros((3, 4, 3))
    xyz[:, :3, 0] = [0.0, 1.0, 2.0]
    n = np.array([2, 3, 3], np.int32)
    xyz[0, :2, 0] = [0.0, 1.0]
    out, state = check(ctx, xyz, n, tr.join_state(head, slots), GATE, what="ids")
    assert out["id"][0, :2].tolist() == [tr.INT32_MAX - 1, -1] and out["status"].tolist() == [tr.E_IDS] * 3
    assert out["id"][1, :3].tolist() == [tr.INT32_MAX - 1, -1, -1] and out["age"][2, :3].tolist() == [3, -1, -1]
    assert tr.split_state(state)[0]["next_id"][0] == tr.INT32_MAX


def test_the_largest_shape(ctx):
    """M = 256 slots, 256 detections per step, T = 8: four waves, every lane a slot and a detection.  From step 4 on ten markers
    are replaced by new points every step: no slot is free for them (FULL) until the ten tracks have missed three times (step 6:
    deaths come before births), and the tracks born then are in the way again at step 7."""
    rng = np.random.default_rng(9)
    g = np.arange(256)
    base = np.stack([0.1 * (g % 16), 0.1 * (g // 16), 0.03 * (g % 3)], axis=1)
    T = 8
    xyz = np.empty((T, 256, 3))
    for t in range(T):
        pts = base + 0.004 * t + 0.002 * rng.standard_normal(base.shape)
        if t >= 4:
            pts[:10] = rng.uniform(2.0, 3.0, (10, 3))
        xyz[t] = pts[rng.permutation(256)]
    n = np.full(T, 256, np.int32)
    out, _ = check(ctx, xyz, n, 256, 0.03, max_miss=2, what="largest")
    assert out["status"].tolist() == [0, 0, 0, 0, tr.E_FULL, tr.E_FULL, 0, tr.E_FULL]
    assert (out["id"][3] >= 0).all() and sorted(out["slot"][3].tolist()) == list(range(256))


@pytest.mark.parametrize("M", [192, 130])
def test_three_waves(ctx, M):
    """max_tracks in 129 .. 192: 192 threads, so the detections' lanes wrap at 96 and the fourth word of a step's 256
    detections is served by wave 0.  The lattice of test_the_largest_shape, the first count[t] points of it per step in
    permuted rows: more detections than slots from the third step (second: M = 130) on.  Births never come from rows at and
    beyond M, so what the fourth word carries is matched rows and rows that stay -1: both must exist there."""
    rng = np.random.default_rng(9)
    g = np.arange(256)
    base = np.stack([0.1 * (g % 16), 0.1 * (g // 16), 0.03 * (g % 3)], axis=1)
    counts = (120, 180, 256, 256, 230, 256, 256)
    T = len(counts)
    xyz = np.zeros((T, 256, 3))
    for t, c in enumerate(counts):
        pts = (base + 0.004 * t + 0.002 * rng.standard_normal(base.shape))[:c]
        xyz[t, :c] = pts[rng.permutation(c)]
    n = np.array(counts, np.int32)
    out, _ = check(ctx, xyz, n, M, 0.03, max_miss=2, what=f"three waves, M = {M}")
    full = [0, 0] + [tr.E_FULL] * 5 if M == 192 else [0] + [tr.E_FULL] * 6
    assert out["status"].tolist() == full
    for t in np.flatnonzero(n == 256):
        word3 = out["id"][t, 192:256]
        assert (word3 == -1).sum() >= 6 and (word3 >= 0).sum() >= 6, (t, word3.tolist())


@pytest.mark.parametrize("T", [48, 96, 97])
def test_the_chunk_edges(ctx, T):
    """Q = 16: a chunk is 48 steps.  T = 48 is one full chunk with nothing to prefetch, 96 two full chunks (the last step's
    count prefetch has no step beyond T to read), 97 leaves a last chunk of one step."""
    xyz, n, _, _, _ = tr.scene(7, 0.8, T=T)
    out, state = check(ctx, xyz, n, 16, GATE, what=f"T = {T}")
    assert (out["id"] >= 0).sum() == n.sum() and tr.split_state(state)[0]["steps"][0] == T


def test_two_calls_give_the_same_bits(ctx):
    xyz, n, gate = tr.crowd_case()
    a = run_gpu(ctx, xyz, n, 16, gate)
    b = run_gpu(ctx, xyz, n, 16, gate)
    assert_same(a, b, what="twice")


def test_argument_errors_launch_nothing(ctx):
    import torch
    from mocapv2_amd import _abi
    xyz = torch.zeros((2, 4, 3), dtype=torch.float64, device="cuda")
    n = torch.zeros((2,), dtype=torch.int32, device="cuda")
    state = ctx.track_state(4)
    for kw in ({"gate": 0.0}, {"gate": float("inf")}, {"gate": float("nan")}, {"gate": 0.1, "beta": 1.5}, {"gate": 0.1, "beta": -0.1},
               {"gate": 0.1, "max_miss": -1}):
        with pytest.raises(_abi.MocapError) as e:
            ctx.track_markers(xyz, n, state, **kw)
        assert e.value.code == -1
    with pytest.raises(_abi.MocapError) as e:
        ctx.track_markers(xyz, n, torch.zeros(64 * 258, dtype=torch.uint8, device="cuda"), 0.1)
    assert e.value.code == -1 and "max_tracks" in str(e.value)
    with pytest.raises(ValueError):
        ctx.track_state(257)
    torch.cuda.synchronize()
    assert not state.cpu().numpy().any()


# ---- trackers ------------------------------------------------------------------------------------------------------------------
W, H = 320, 192
MARKERS = np.array([[-0.42, -0.30, 0.05], [0.40, 0.32, 0.12]])
TRACK = {"gate": 0.15, "max_tracks": 8}


def marker_positions(t):
    common = np.array([0.06 * np.sin(0.15 * t), 0.05 * np.cos(0.15 * t), 0.04 * np.sin(0.1 * t)])
    return MARKERS + common[None] + np.array([[0.01 * np.sin(0.3 * t + 2 * m), 0.0, 0.0] for m in range(2)])


@pytest.fixture(scope="module")
def moving_discs():
    """[80, 3, H, W]: two discs per camera on slow paths (at most 13 mm per step); every seventh step camera 0 misses marker 0"""
    from mocapv2_amd.synth import ZERO_DIST, Scene
    sc = Scene(3, W, H, dist=ZERO_DIST)
    T = 80
    frames = np.empty((T, 3, H, W), np.uint8)
    for t in range(T):
        mk = marker_positions(t)
        for c in range(3):
            seen = mk[1:] if c == 0 and t % 7 == 3 else mk
            frames[t, c] = sc.render(np.random.default_rng(100 * t + c), seen, c, radius_range=(16.0, 17.0), noise_max=40)
    return sc, frames


def run_batches(arrays, frames, depth, visibility="any", batch=16):
    import torch
    from mocapv2_amd.pipeline import BatchTracker
    K, dist, R, t, F = arrays
    tracker = BatchTracker(K, dist, R, t, F if visibility == "all" else None, W, H, batch, max_points=8, depth=depth,
                           visibility=visibility, track=TRACK)
    res = []
    for b0 in range(0, len(frames), batch):
        out = tracker.step(torch.from_numpy(frames[b0:b0 + batch].reshape(batch * 3, H, W)).cuda())
        if depth == 1:
            tracker.finish(out)
        res.append({k: v.clone() for k, v in out.items()} if depth == 1 else out)
        if depth > 1 and len(res) % depth == 0:  # a lane's outputs are overwritten when the lane comes round again: read them first
            tracker.synchronize()
            res[-depth:] = [{k: v.clone() for k, v in o.items()} for o in res[-depth:]]
    tracker.synchronize()
    torch.cuda.synchronize()
    keys = ("xyz", "n", "id", "slot", "age", "status") + (("order",) if visibility == "all" else ())
    return {k: np.concatenate([o[k].cpu().numpy() for o in res]) for k in keys}, tracker.track_state.cpu().numpy()


def test_batch_tracker_depth_3_and_depth_1_give_the_same_identities(moving_discs):
    from mocapv2_amd.pipeline import scene_arrays
    sc, frames = moving_discs
    arrays = scene_arrays(sc)
    one, s1 = run_batches(arrays, frames, depth=1)
    three, s3 = run_batches(arrays, frames, depth=3)
    assert one["n"].tolist() == [2] * 80
    for k in ("xyz", "n", "id", "slot", "age", "status"):
        rows = one["n"][:, None] > np.arange(one[k].shape[1])[None, :] if one[k].ndim > 1 else None
        a, b = (one[k], three[k]) if rows is None else (one[k][rows], three[k][rows])
        assert np.array_equal(a, b), k
    assert np.array_equal(s1, s3)
    # ... and they are the restatement's on the read-back markers, over the five batches as one run
    want, ws = run_ref(one["xyz"], one["n"], TRACK["max_tracks"], TRACK["gate"])
    assert_same(({k: one[k] for k in ("id", "slot", "age", "status")}, s1), (want, ws), what="tracker")
    # two tracks from the first step to the last, each on its own marker
    assert sorted(one["id"][0, :2].tolist()) == [0, 1] and sorted(one["age"][-1, :2].tolist()) == [80, 80]
    owner = {}
    for t in range(80):
        for r in range(2):
            m = int(np.argmin(np.linalg.norm(marker_positions(t) - one["xyz"][t, r], axis=1)))
            assert owner.setdefault(int(one["id"][t, r]), m) == m, (t, r)


def test_batch_tracker_all_tracks_the_reported_roots_in_their_order(moving_discs):
    from mocapv2_amd.pipeline import scene_arrays
    sc, frames = moving_discs
    got, state = run_batches(scene_arrays(sc), frames[:32], depth=1, visibility="all")
    n, order = got["n"], got["order"]
    assert (n >= 1).all()
    P = got["xyz"].shape[1]
    picked = got["xyz"][np.arange(32)[:, None], np.clip(order, 0, P - 1)]
    want, ws = run_ref(picked, n, TRACK["max_tracks"], TRACK["gate"])
    assert_same(({k: got[k] for k in ("id", "slot", "age", "status")}, state), (want, ws), what="all")


def test_replay_tracker_short_last_batch_equals_one_long_batch(moving_discs):
    from mocapv2_amd.pipeline import scene_arrays
    from mocapv2_amd.replay import ReplayTracker
    sc, frames = moving_discs
    K, dist, R, t, F = scene_arrays(sc)
    frames = frames[:40]
    kw = dict(max_points=8, visibility="any", track=TRACK)
    short = list(ReplayTracker(K, dist, R, t, None, W, H, batch=16, **kw).run_batches(frames))  # 16 + 16 + 8 (padded to 16)
    long = list(ReplayTracker(K, dist, R, t, None, W, H, batch=40, **kw).run_batches(frames))
    assert [b["n_steps"] for b in short] == [16, 16, 8] and [b["n_steps"] for b in long] == [40]
    for key in ("ids", "ages", "kept", "object_points"):
        assert np.array_equal(np.concatenate([b[key] for b in short]), long[0][key]), key
    assert long[0]["ids"].shape == (40, 5) and (long[0]["ids"][:, :2] >= 0).all() and (long[0]["ids"][:, 2:] == -1).all()
    assert sorted(long[0]["ages"][-1, :2].tolist()) == [40, 40]  # the padding of the short run aged nothing either
    steps = list(ReplayTracker(K, dist, R, t, None, W, H, batch=16, **kw).run(frames))
    assert all(np.array_equal(s["ids"], long[0]["ids"][i, :2]) and len(s["object_points"]) == 2 for i, s in enumerate(steps))
    assert all("ids" not in s for s in ReplayTracker(K, dist, R, t, None, W, H, batch=40, max_points=8, visibility="any").run(frames[:2]))
