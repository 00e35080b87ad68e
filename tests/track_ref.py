"""The tracker of DESIGN.md section 2 ("Identities across time steps") restated in NumPy: what mocap_track_markers must give,
bit for bit.  All arithmetic is float64 and every operation is rounded on its own (NumPy never fuses a product into a sum), in
the order the definition gives: p = pos + vel;  d = D - p;  d2 = (dx * dx + dy * dy) + dz * dz;  g = gate * (1 + miss);
candidate iff d2 < g * g;  vel = vel + beta * (D - p).  The assignment is carried in both of its forms -- the sorted greedy walk
over (d2, slot, detection) and the rounds of mutually best pairs the kernel runs -- and tests/test_track_host.py shows them equal.

Also here: the scene generator of the host and GPU tests and the two figures they pin (mix-ups, identity changes)."""
import numpy as np

MAX_TRACKS = 256
INT32_MAX = 2 ** 31 - 1
E_FULL, E_IDS, E_INPUT, E_COUNT = -2, -3, -4, -5  # MOCAP_TRACK_E_*

# the state buffer of include/mocap_hip.h: mocap_track_header, then max_tracks mocap_track_slot (64 bytes each)
HEADER = np.dtype([("next_id", "<i4"), ("reserved0", "<i4"), ("steps", "<i8"), ("reserved", "<i8", (6,))])
SLOT = np.dtype([("pos", "<f8", (3,)), ("vel", "<f8", (3,)), ("id", "<i4"), ("miss", "<i4"), ("hits", "<i4"), ("alive", "<i4")])
assert HEADER.itemsize == 64 and SLOT.itemsize == 64


def state_bytes(max_tracks):
    return 64 * (1 + max_tracks)


def new_state(max_tracks):
    """(header [1], slots [max_tracks]) views of one zeroed buffer: the empty tracker"""
    return split_state(np.zeros(state_bytes(max_tracks), np.uint8))


def split_state(buf):
    buf = np.ascontiguousarray(buf).view(np.uint8).reshape(-1)
    return buf[:64].view(HEADER), buf[64:].view(SLOT)


def join_state(head, slots):
    return np.concatenate([head.view(np.uint8).reshape(-1), slots.view(np.uint8).reshape(-1)])


def distances(D, p):
    """d2 [slots, detections] by the definition's operations"""
    d = D[None, :, :] - p[:, None, :]
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def assign_greedy(d2, cand):
    """The candidates in ascending (d2, slot, detection); a pair is accepted when neither side is taken.  -> {slot: detection}"""
    ss, jj = np.nonzero(cand)
    order = np.lexsort((jj, ss, d2[ss, jj]))
    slot_of, det_of = {}, {}
    for k in order:
        s, j = int(ss[k]), int(jj[k])
        if s not in det_of and j not in slot_of:
            det_of[s], slot_of[j] = j, s
    return det_of


def assign_rounds(d2, cand):
    """Rounds of "every pair that is mutually best among what remains is accepted": a row's best is its smallest (d2, detection),
    a column's best its smallest (d2, slot).  -> ({slot: detection}, rounds)"""
    cand = cand.copy()
    det_of, rounds = {}, 0
    while cand.any():
        rounds += 1
        big = np.where(cand, d2, np.inf)
        row_best = np.argmin(big, axis=1)   # argmin: the first of equal values = the lowest index
        col_best = np.argmin(big, axis=0)
        got = [(s, int(row_best[s])) for s in range(d2.shape[0]) if cand[s].any() and col_best[row_best[s]] == s]
        assert got  # the smallest remaining pair is always mutually best
        for s, j in got:
            det_of[s] = j
            cand[s, :] = False
            cand[:, j] = False
    return det_of, rounds


def step(head, slots, D, n, gate, beta=0.5, max_miss=5, Q=None, assign=assign_greedy):
    """One time step on the state (in place).  D [rows, 3], n the count.  -> (id, slot, age [Q] int32, status)"""
    M = len(slots)
    Q = len(D) if Q is None else Q
    ids, slot_out, age = (np.full(Q, -1, np.int32) for _ in range(3))
    blind = n < 0 or n > min(Q, MAX_TRACKS)
    nn = 0 if blind else int(n)
    D = np.asarray(D, np.float64)[:nn]  # rows at and beyond n are never read
    live = slots["alive"] != 0
    p = slots["pos"] + slots["vel"]                                       # 1. predict
    g = gate * (1 + slots["miss"]).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        d2 = distances(D, p)
        cand = live[:, None] & (d2 < (g * g)[:, None])                    # 2. candidates (a NaN compares false)
    det_of = assign(d2, cand)                                             # 3. assignment
    if isinstance(det_of, tuple):
        det_of = det_of[0]
    for s in range(M):
        if not live[s]:
            continue
        if s in det_of:                                                   # 4. matched
            j = det_of[s]
            e = D[j] - p[s]
            slots["vel"][s] = slots["vel"][s] + beta * e
            slots["pos"][s] = D[j]
            slots["miss"][s] = 0
            slots["hits"][s] += 1
            ids[j], slot_out[j], age[j] = slots["id"][s], s, slots["hits"][s]
        else:                                                             # 5. unmatched: coast; deaths come before births
            slots["pos"][s] = p[s]
            slots["miss"][s] += 1
            if slots["miss"][s] > max_miss:
                slots["alive"][s] = 0
    status = (E_INPUT if n < 0 else E_COUNT) if blind else 0
    taken = set(det_of.values())
    for j in range(nn):                                                   # 6. births, in ascending j
        if j in taken:
            continue
        free = np.flatnonzero(slots["alive"] == 0)
        if len(free) == 0:
            status = E_FULL
            continue
        if head["next_id"][0] == INT32_MAX:
            status = E_IDS
            continue
        s = int(free[0])
        slots["id"][s] = head["next_id"][0]
        head["next_id"][0] += 1
        slots["pos"][s], slots["vel"][s], slots["miss"][s], slots["hits"][s], slots["alive"][s] = D[j], 0.0, 0, 1, 1
        ids[j], slot_out[j], age[j] = slots["id"][s], s, 1
    head["steps"][0] += 1
    return ids, slot_out, age, status


def track(xyz, n, state, gate, beta=0.5, max_miss=5, assign=assign_greedy):
    """mocap_track_markers: xyz [T, Q, 3], n [T], state = (header, slots) updated in place.
    -> dict of id, slot, age [T, Q] int32 and status [T] int32"""
    head, slots = state
    T, Q = xyz.shape[:2]
    out = {k: np.full((T, Q), -1, np.int32) for k in ("id", "slot", "age")}
    out["status"] = np.zeros(T, np.int32)
    for t in range(T):
        out["id"][t], out["slot"][t], out["age"][t], out["status"][t] = step(head, slots, xyz[t], int(n[t]), gate, beta, max_miss,
                                                                             Q=Q, assign=assign)
    return out


# ---- scenes ----------------------------------------------------------------------------------------------------------------
def scene(seed, speed=1.0, T=400, markers=8, Q=16, noise=0.0015, p_drop=0.1, p_ghost=0.05):
    """`markers` markers on smooth paths in a 1 m cube (each axis: two sinusoids of amplitude 0.1-0.25 m; `speed` scales their
    frequencies), Gaussian noise per axis, every sighting dropped with p_drop, one burst of 2-4 hidden steps per marker, one
    uniform ghost point per step with p_ghost, rows shuffled per step.
    -> xyz [T, Q, 3] (rows beyond n: NaN), n [T] int32, who [T, Q] (marker of the row, -1 = ghost or empty), seen [T, markers],
    path [T, markers, 3] (the noise-free positions)"""
    rng = np.random.default_rng(seed)
    t = np.arange(T)[:, None, None]
    amp = rng.uniform(0.1, 0.25, (2, markers, 3))
    freq = rng.uniform(0.004, 0.012, (2, markers, 3)) * speed * 2 * np.pi
    phase = rng.uniform(0, 2 * np.pi, (2, markers, 3))
    centre = rng.uniform(0.3, 0.7, (markers, 3))
    path = centre[None] + sum(amp[k][None] * np.sin(freq[k][None] * t + phase[k][None]) for k in range(2))  # [T, markers, 3]
    seen = rng.random((T, markers)) >= p_drop
    for m in range(markers):
        b0, length = rng.integers(10, T - 10), rng.integers(2, 5)
        seen[b0:b0 + length, m] = False
    xyz = np.full((T, Q, 3), np.nan)
    n = np.zeros(T, np.int32)
    who = np.full((T, Q), -1, np.int64)
    for s in range(T):
        rows = [(m, path[s, m] + noise * rng.standard_normal(3)) for m in range(markers) if seen[s, m]]
        if rng.random() < p_ghost:
            rows.append((-1, rng.uniform(0.0, 1.0, 3)))
        for r, k in enumerate(rng.permutation(len(rows))):
            who[s, r], xyz[s, r] = rows[k]
        n[s] = len(rows)
    return xyz, n, who, seen, path


def mixups_and_changes(ids, who, markers):
    """mix-ups: identities that name two markers.  changes: per marker, the steps at which its identity differs from the one it
    had at its previous sighting [(marker, previous sighting, step)]."""
    owner, mixed, changes = {}, set(), []
    last = {}
    T = len(ids)
    for t in range(T):
        for r in np.flatnonzero(who[t] >= 0):
            m, i = int(who[t, r]), int(ids[t, r])
            if i < 0:
                continue
            if owner.setdefault(i, m) != m:
                mixed.add(i)
            if m in last and last[m][1] != i:
                changes.append((m, last[m][0], t))
            last[m] = (t, i)
    return sorted(mixed), changes


def long_gaps(seen, max_miss):
    """[(marker, last sighting, next sighting)] of the gaps with more than max_miss steps without a sighting in between"""
    out = []
    for m in range(seen.shape[1]):
        ts = np.flatnonzero(seen[:, m])
        for a, b in zip(ts[:-1], ts[1:]):
            if b - a - 1 > max_miss:
                out.append((m, int(a), int(b)))
    return out


def lattice_case(Q=16):
    """Exact ties: tracks are born on the even points of an integer lattice, then detections arrive exactly halfway between two
    (d2 = 1) or four (d2 = 2) predictions.  Every coordinate is a small dyadic number, so every d2 is exact and the ties are
    real.  gate = 1.5.  -> xyz [T, Q, 3], n [T], gate"""
    rng = np.random.default_rng(11)
    even = [(2.0 * i, 2.0 * k, 0.0) for i in range(3) for k in range(3)]
    mid = [(1.0, 0.0, 0.0), (3.0, 0.0, 0.0), (1.0, 2.0, 0.0), (3.0, 2.0, 0.0), (1.0, 4.0, 0.0), (3.0, 4.0, 0.0), (1.0, 1.0, 0.0), (3.0, 3.0, 0.0)]
    odd = [(1.0, 1.0, 0.0), (3.0, 1.0, 0.0), (1.0, 3.0, 0.0), (3.0, 3.0, 0.0), (2.0, 2.0, 0.0), (0.0, 4.0, 0.0)]
    steps = [even, mid, odd, mid, even, odd]
    xyz = np.full((len(steps), Q, 3), np.nan)
    n = np.zeros(len(steps), np.int32)
    for t, pts in enumerate(steps):
        pts = np.array(pts)[rng.permutation(len(pts))]
        xyz[t, :len(pts)], n[t] = pts, len(pts)
    return xyz, n, 1.5


def crowd_case(T=24, Q=16, markers=12, seed=5):
    """Markers closer to each other (0.1) than the gate (0.3), jittered by 0.04 and dropped now and then: every slot has several
    candidates and the rounds run several passes.  -> xyz [T, Q, 3], n [T], gate"""
    rng = np.random.default_rng(seed)
    base = np.stack([0.1 * np.arange(markers), 0.05 * (np.arange(markers) % 3), np.zeros(markers)], axis=1)
    xyz = np.full((T, Q, 3), np.nan)
    n = np.zeros(T, np.int32)
    for t in range(T):
        pts = (base + 0.01 * t + 0.04 * rng.standard_normal(base.shape))[rng.random(markers) >= 0.15]
        pts = pts[rng.permutation(len(pts))]
        xyz[t, :len(pts)], n[t] = pts, len(pts)
    return xyz, n, 0.3
