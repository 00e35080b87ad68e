"""NumPy restatement of the definition of mocap_learn_marker_pair_stats and mocap_learn_rigid_bodies ("Rigid-body models
learned from a capture"): what csrc/rigid_learn.hip must give, bit for bit.  Vectorised over the time steps; every sum over time
is written out in the definition's order -- per chunk of 32 steps in ascending t from 0, then the chunks in ascending order --
and Horn's pose is rigid_ref.horn, the restatement mocap_rigid_poses is held to.  FP64, + - * / and sqrt only, each rounded on its
own.  Also the seeded take the host and GPU tests share.  Not a test module."""
import numpy as np

import rigid_ref as rr

CHUNK, MAX_IDS, MAX_GROUPS, MAX_MARKERS = 32, 64, 16, 8  # MOCAP_LEARN_CHUNK, MOCAP_LEARN_MAX_*, MOCAP_RIGID_MAX_MARKERS
E_MEMBERS, E_INCOMPLETE = -2, -3                         # MOCAP_LEARN_E_*


def locate(n, ident, wanted):
    """row [T, W]: the lowest row r < n[t] with ident[t][r] == wanted[w], -1 = absent; a blind step (n < 0 or n > Q) has no rows"""
    n, ident = np.asarray(n), np.asarray(ident)
    T, Q = ident.shape
    rows = np.where((n[:T] < 0) | (n[:T] > Q), 0, n[:T])
    live = np.arange(Q)[None, :] < rows[:, None]
    out = np.full((T, len(wanted)), -1, np.int64)
    for w, i in enumerate(wanted):
        if i < 0:
            continue
        hit = live & (ident == i)
        out[:, w] = np.where(hit.any(axis=1), hit.argmax(axis=1), -1)
    return out


def positions(xyz, row):
    """[T, W, 3]: the position of each located identity, 0 where it is absent (nothing reads it there)"""
    T = len(row)
    pos = np.asarray(xyz, np.float64)[np.arange(T)[:, None], np.maximum(row, 0)]
    return np.where((row >= 0)[:, :, None], pos, 0.0)


def chunk_sums(val, on):
    """The definition's sum over time of val [T, ...] where on [T, ...] (same shape): per chunk in ascending t from 0, then the
    chunks in ascending order, from 0.  T = 0 gives zeros."""
    T = len(val)
    C = (T + CHUNK - 1) // CHUNK
    pad = C * CHUNK - T
    if pad:
        val = np.concatenate([val, np.zeros((pad,) + val.shape[1:])])
        on = np.concatenate([on, np.zeros((pad,) + on.shape[1:], bool)])
    val, on = val.reshape((C, CHUNK) + val.shape[1:]), on.reshape((C, CHUNK) + on.shape[1:])
    part = np.zeros((C,) + val.shape[2:])
    with np.errstate(invalid="ignore"):
        for s in range(CHUNK):
            part = np.where(on[:, s], part + val[:, s], part)
    total = np.zeros(val.shape[2:])
    for c in range(C):
        total = total + part[c]
    return total


def pair_stats(xyz, n, ident, ids, block=64):
    """mocap_learn_marker_pair_stats: dict of [K, K] arrays count (int32), dmin, dmax, dsum, dsum2.  `block` chunks are held at a time."""
    ids = np.asarray(ids, np.int64)
    K = len(ids)
    assert 2 <= K <= MAX_IDS and (ids >= 0).all() and (np.diff(ids) > 0).all()
    row = locate(n, ident, ids)
    T = len(row)
    has, pos = row >= 0, positions(xyz, row)
    count = np.zeros((K, K), np.int64)
    dmin, dmax = np.full((K, K), np.inf), np.full((K, K), -np.inf)
    dsum, dsum2 = np.zeros((K, K)), np.zeros((K, K))
    step = block * CHUNK
    for t0 in range(0, T, step):
        h, p = has[t0:t0 + step], pos[t0:t0 + step]
        both = h[:, :, None] & h[:, None, :]
        dx, dy, dz = (p[:, :, None, u] - p[:, None, :, u] for u in range(3))
        d = np.sqrt((dx * dx + dy * dy) + dz * dz)
        count += both.sum(axis=0)
        dmin = np.minimum(dmin, np.where(both, d, np.inf).min(axis=0))
        dmax = np.maximum(dmax, np.where(both, d, -np.inf).max(axis=0))
        # (the block's chunks one after the other, onto the running totals: the same chain of additions as over the whole take)
        C = (len(h) + CHUNK - 1) // CHUNK
        for c in range(C):
            sl = slice(c * CHUNK, (c + 1) * CHUNK)
            part, part2 = np.zeros((K, K)), np.zeros((K, K))
            for s in range(len(h[sl])):
                b, ds = both[sl][s], d[sl][s]
                part, part2 = np.where(b, part + ds, part), np.where(b, part2 + ds * ds, part2)
            dsum, dsum2 = dsum + part, dsum2 + part2
    seen = count > 0
    dmin, dmax = np.where(seen, dmin, 0.0), np.where(seen, dmax, 0.0)
    diag = np.eye(K, dtype=bool)
    out = {"count": count.astype(np.int32), "dmin": dmin, "dmax": dmax, "dsum": dsum, "dsum2": dsum2}
    for k in ("dmin", "dmax", "dsum", "dsum2"):
        out[k] = np.where(diag, 0.0, out[k])
    return out


def centred(m):
    """m [M, 3] minus its centroid: the sum over p ascending from 0, divided by M"""
    c = np.zeros(3)
    for p in range(len(m)):
        c = c + m[p]
    return m - c / float(len(m))


def one_pass(model, pos, has, used, residual):
    """One pass over the take for one group.  model [M, 3], pos [T, M, 3], has [T, M], used [T].  -> (sums [M, 3], counts [M]): per
    member the sum of b = R^T (D_p - t) over the used steps it is present in -- with `residual`, of |R m_p + t - D_p|^2 in [:, 0]"""
    T, M = has.shape
    on = has & used[:, None]
    val = np.zeros((T, M, 3))
    idx = np.flatnonzero(used)
    if len(idx):
        det = np.zeros((T, MAX_MARKERS, 3))
        det[:, :M] = pos
        lab = np.full((len(idx), MAX_MARKERS), -1, np.int64)
        lab[:, :M] = np.where(has[idx], idx[:, None] * MAX_MARKERS + np.arange(M)[None, :], -1)
        mod = np.zeros((MAX_MARKERS, 3))
        mod[:M] = model
        R, t, _ = rr.horn(mod, det.reshape(-1, 3), lab)
        for p in range(M):
            D = pos[idx, p]
            if residual:
                e = rr.transform(R, t, mod[p]) - D
                val[idx, p, 0] = (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]
            else:
                e = D - t
                for u in range(3):
                    val[idx, p, u] = (R[:, u] * e[:, 0] + R[:, 3 + u] * e[:, 1]) + R[:, 6 + u] * e[:, 2]
    return chunk_sums(val, np.broadcast_to(on[:, :, None], val.shape)), on.sum(axis=0)


def learn_group(xyz, n, ident, members, rounds, min_present):
    """One group of mocap_learn_rigid_bodies -> dict(model [8, 3], rms, member_rms [8], member_count [8], steps_used, ref_step, status)"""
    out = {"model": np.zeros((MAX_MARKERS, 3)), "rms": 0.0, "member_rms": np.zeros(MAX_MARKERS), "member_count": np.zeros(MAX_MARKERS, np.int32),
           "steps_used": 0, "ref_step": -1, "status": 0}
    members = [int(m) for m in members]
    M = len(members)
    if not (3 <= M <= MAX_MARKERS and M >= min_present) or min(members) < 0 or len(set(members)) != M:
        return dict(out, status=E_MEMBERS)
    row = locate(n, ident, members)
    has, pos = row >= 0, positions(xyz, row)
    complete = np.flatnonzero(has.all(axis=1))
    if not len(complete):
        return dict(out, status=E_INCOMPLETE)
    ref = int(complete[0])
    used = has.sum(axis=1) >= min_present
    model = centred(pos[ref])
    for _ in range(rounds):
        sums, counts = one_pass(model, pos, has, used, False)
        model = centred(sums / counts[:, None].astype(np.float64))
    sums, counts = one_pass(model, pos, has, used, True)
    total, n_total = 0.0, 0
    for p in range(M):
        total, n_total = total + sums[p, 0], n_total + int(counts[p])
    out["model"][:M] = model
    out["member_rms"][:M] = np.sqrt(sums[:, 0] / counts.astype(np.float64))
    out["member_count"][:M] = counts
    out.update(rms=float(np.sqrt(total / float(n_total))), steps_used=int(used.sum()), ref_step=ref)
    return out


def rigid_learn(xyz, n, ident, members, rounds=2, min_present=3):
    """mocap_learn_rigid_bodies: members a list of G lists -> dict of arrays [G, ...] (the floats of a group whose status is not 0 are
    zeros here and unspecified on the device)"""
    groups = [learn_group(xyz, n, ident, m, rounds, min_present) for m in members]
    return {k: np.array([g[k] for g in groups]) for k in groups[0]}


def frequent_ids(n, ident, min_steps):
    """The identities learn_rigid_bodies takes with ids=None: present in at least min_steps steps; more than 64: the 64 with the
    most such steps, ties to the lower identity; ascending"""
    n, ident = np.asarray(n), np.asarray(ident)
    T, Q = ident.shape
    live = (np.arange(Q)[None, :] < np.where((n[:T] < 0) | (n[:T] > Q), 0, n[:T])[:, None]) & (ident >= 0)
    steps = {}
    for t in range(T):
        for i in set(ident[t][live[t]].tolist()):
            steps[i] = steps.get(i, 0) + 1
    keep = sorted((i for i, k in steps.items() if k >= min_steps), key=lambda i: (-steps[i], i))[:MAX_IDS]
    return np.array(sorted(keep), np.int32)


def aligned_error(learned, truth):
    """The distance of every learned point from the truth's after Horn's alignment of the learned model onto it: [M]"""
    M = len(truth)
    mod = np.zeros((MAX_MARKERS, 3))
    mod[:M] = learned
    lab = np.full((1, MAX_MARKERS), -1, np.int64)
    lab[0, :M] = np.arange(M)
    R, t, _ = rr.horn(mod, np.asarray(truth, np.float64), lab)
    return np.array([np.linalg.norm(rr.transform(R, t, mod[p])[0] - truth[p]) for p in range(M)])


# ---- the seeded take -------------------------------------------------------------------------------------------------------------
SPREAD, MIN_STEPS = 0.008, 10
CLUTTER_ID0 = 1000


def take_of(sc):
    """A rigid_ref scene with the identities its `row` truth gives: 10 b + p for marker p of body b, a fresh identity (1000, 1001,
    ...) for every clutter point, -1 beyond n.  -> dict(xyz [T, Q, 3], n [T], id [T, Q] int32, models, sc)"""
    T, Q = sc["xyz"].shape[:2]
    ident = np.full((T, Q), -1, np.int32)
    fresh = CLUTTER_ID0
    for s in range(T):
        owner = {}
        for b in range(sc["row"].shape[1]):
            for p in range(MAX_MARKERS):
                if sc["row"][s, b, p] >= 0:
                    owner[int(sc["row"][s, b, p])] = 10 * b + p
        for r in range(int(sc["n"][s])):
            if r in owner:
                ident[s, r] = owner[r]
            else:
                ident[s, r] = fresh
                fresh += 1
    return {"xyz": sc["xyz"].copy(), "n": sc["n"].copy(), "id": ident, "models": sc["models"], "sc": sc}


def take(seed, T=60, **kw):
    return take_of(rr.rigid_scene(seed, T=T, **kw))


def take_three_and_eight(seed=6, T=40, hidden=0.2, clutter=3, Q=16):
    """A take of a body of 3 and a body of 8 markers (the eight in a cube of edge 0.5: rigid_scene's 0.25 has no room for 28
    distinct distances), otherwise as rigid_scene makes its own"""
    rng = np.random.default_rng(seed)
    models = [rr.make_body(rng, 3), rr.make_body(rng, 8, size=0.5)]
    xyz, n, row = np.full((T, Q, 3), np.nan), np.zeros(T, np.int32), np.full((T, 2, MAX_MARKERS), -1, np.int32)
    for s in range(T):
        pts, owner = [], []
        for b, model in enumerate(models):
            R, t = rr.random_rotation(rng), rng.uniform(-1, 1, 3)
            for p in np.flatnonzero(rng.random(len(model)) >= hidden):
                pts.append(R @ model[p] + t + rng.normal(scale=rr.NOISE, size=3))
                owner.append((b, p))
        pts += list(rng.uniform(-1.2, 1.2, (clutter, 3)))
        n[s] = len(pts)
        for r, k in enumerate(rng.permutation(len(pts))):
            xyz[s, r] = pts[k]
            if k < len(owner):
                row[s, owner[k][0], owner[k][1]] = r
    return take_of({"xyz": xyz, "n": n, "models": models, "row": row})


def truth_members(tk):
    return [[10 * b + p for p in range(len(m))] for b, m in enumerate(tk["models"])]


def tiled(tk, T):
    """The take's steps repeated up to T steps (the identities of the body markers stay; a clutter identity then appears once per
    repetition)"""
    reps = (T + len(tk["n"]) - 1) // len(tk["n"])
    return dict(tk, xyz=np.concatenate([tk["xyz"]] * reps)[:T].copy(), n=np.concatenate([tk["n"]] * reps)[:T].copy(),
                id=np.concatenate([tk["id"]] * reps)[:T].copy())


def static_take(seed=3, T=40):
    """Three bodies that share one pose per step, so they never move against one another: noise-free, nothing hidden, no clutter"""
    rng = np.random.default_rng(seed)
    models = [rr.make_body(rng, M) + off for M, off in ((4, [0.0, 0.0, 0.0]), (5, [0.5, 0.0, 0.0]), (6, [0.0, 0.5, 0.0]))]
    Q = 16
    xyz, ident = np.full((T, Q, 3), np.nan), np.full((T, Q), -1, np.int32)
    for s in range(T):
        R, t = rr.random_rotation(rng), rng.uniform(-1, 1, 3)
        r = 0
        for b, m in enumerate(models):
            for p in range(len(m)):
                xyz[s, r], ident[s, r] = R @ m[p] + t, 10 * b + p
                r += 1
    return {"xyz": xyz, "n": np.full(T, 15, np.int32), "id": ident, "models": models}
