"""NumPy restatement of mocap_rigid_poses' definition ("Rigid-body poses"): what csrc/rigid.hip must give,
bit for bit.  Every (time step, body) is solved on its own; the work inside one is vectorised over the candidates, with masks where
the kernel branches, and every sum is written out in the order the definition gives (FP64, + - * / and sqrt only, each rounded on
its own).  Also the seeded scene the host and GPU tests share.  Not a test module."""
import itertools

import numpy as np

from correspond_visible_ref import smallest_eigvec4

MAX_DET, MAX_MARKERS, MAX_TRIPLES, MAX_BODIES, MAX_HYP = 64, 8, 56, 16, 4096  # MOCAP_RIGID_MAX_*
LOST, E_BLIND, E_CAPACITY, E_MODEL, E_HYP = 1, -2, -3, -4, -5             # MOCAP_RIGID_*


def triples_of(model, min_area):
    """Every model triple (a, b, c), a < b < c, whose triangle area exceeds min_area (MocapContext.rigid_bodies lists the same)"""
    model = np.asarray(model, np.float64)
    out = []
    for a, b, c in itertools.combinations(range(len(model)), 3):
        if 0.5 * np.linalg.norm(np.cross(model[b] - model[a], model[c] - model[a])) > min_area:
            out.append((a, b, c))
    return np.array(out, np.int32).reshape(-1, 3)


def dist_table(P):
    """d_ij = sqrt((dx dx + dy dy) + dz dz); P [n, 3] -> [n, n]"""
    dx, dy, dz = (P[:, None, u] - P[None, :, u] for u in range(3))
    return np.sqrt((dx * dx + dy * dy) + dz * dz)


def candidates(dd, dm, tri, tol):
    """The hypotheses of step 3 in ascending (h, i, j, k): [N, 4] int64.  dd [n, n], dm [M, M]: the distance tables."""
    n = len(dd)
    distinct = np.ones((n, n, n), bool)
    r = np.arange(n)
    distinct[r, r, :] = False
    distinct[r, :, r] = False
    distinct[:, r, r] = False
    out = []
    with np.errstate(invalid="ignore"):
        for h, (a, b, c) in enumerate(tri):
            ab = np.abs(dd - dm[a, b]) < tol
            bc = np.abs(dd - dm[b, c]) < tol
            ac = np.abs(dd - dm[a, c]) < tol
            ijk = np.argwhere(ab[:, :, None] & bc[None, :, :] & ac[:, None, :] & distinct)
            out.append(np.concatenate([np.full((len(ijk), 1), h), ijk], axis=1))
    return np.concatenate(out).astype(np.int64) if out else np.zeros((0, 4), np.int64)


def horn(model, det, lab):
    """Horn's closed-form pose of the pairs (m_p, D_lab[p]) with lab[p] >= 0, taken in ascending p, for N label rows at once:
    lab [N, 8] -> R [N, 9], t [N, 3], q [N, 4].  Rows without a pair give numbers nobody reads."""
    N = len(lab)
    on = lab >= 0
    row = np.where(on, lab, 0)
    cnt = np.zeros(N)
    sm, sd = np.zeros((N, 3)), np.zeros((N, 3))
    for p in range(MAX_MARKERS):
        m = on[:, p]
        cnt = np.where(m, cnt + 1.0, cnt)
        for u in range(3):
            sm[:, u] = np.where(m, sm[:, u] + model[p, u], sm[:, u])
            sd[:, u] = np.where(m, sd[:, u] + det[row[:, p], u], sd[:, u])
    with np.errstate(all="ignore"):
        mb, db = sm / cnt[:, None], sd / cnt[:, None]
        S = np.zeros((N, 3, 3))
        for p in range(MAX_MARKERS):
            m = on[:, p]
            for u in range(3):
                for v in range(3):
                    S[:, u, v] = np.where(m, S[:, u, v] + (model[p, u] - mb[:, u]) * (det[row[:, p], v] - db[:, v]), S[:, u, v])
        Nm = np.empty((N, 4, 4))
        Nm[:, 0, 0] = (S[:, 0, 0] + S[:, 1, 1]) + S[:, 2, 2]
        Nm[:, 1, 1] = (S[:, 0, 0] - S[:, 1, 1]) - S[:, 2, 2]
        Nm[:, 2, 2] = (S[:, 1, 1] - S[:, 0, 0]) - S[:, 2, 2]
        Nm[:, 3, 3] = (S[:, 2, 2] - S[:, 0, 0]) - S[:, 1, 1]
        Nm[:, 0, 1] = Nm[:, 1, 0] = S[:, 1, 2] - S[:, 2, 1]
        Nm[:, 0, 2] = Nm[:, 2, 0] = S[:, 2, 0] - S[:, 0, 2]
        Nm[:, 0, 3] = Nm[:, 3, 0] = S[:, 0, 1] - S[:, 1, 0]
        Nm[:, 1, 2] = Nm[:, 2, 1] = S[:, 0, 1] + S[:, 1, 0]
        Nm[:, 1, 3] = Nm[:, 3, 1] = S[:, 2, 0] + S[:, 0, 2]
        Nm[:, 2, 3] = Nm[:, 3, 2] = S[:, 1, 2] + S[:, 2, 1]
        q = smallest_eigvec4(-Nm)
        nrm = np.sqrt(((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]) + q[:, 3] * q[:, 3])
        q = q / nrm[:, None]
        z = q == 0.0
        neg = (q[:, 0] < 0) | (z[:, 0] & (q[:, 1] < 0)) | (z[:, 0] & z[:, 1] & (q[:, 2] < 0)) | (z[:, 0] & z[:, 1] & z[:, 2] & (q[:, 3] < 0))
        q = np.where(neg[:, None], -q, q)
        w, x, y, zz = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
        ww, xx, yy, z2 = w * w, x * x, y * y, zz * zz
        wx, wy, wz, xy, xz, yz = w * x, w * y, w * zz, x * y, x * zz, y * zz
        R = np.stack([((ww + xx) - yy) - z2, 2.0 * (xy - wz), 2.0 * (xz + wy),
                      2.0 * (xy + wz), ((ww - xx) + yy) - z2, 2.0 * (yz - wx),
                      2.0 * (xz - wy), 2.0 * (yz + wx), ((ww - xx) - yy) + z2], axis=1)
        t = np.stack([db[:, u] - ((R[:, 3 * u] * mb[:, 0] + R[:, 3 * u + 1] * mb[:, 1]) + R[:, 3 * u + 2] * mb[:, 2]) for u in range(3)], axis=1)
    return R, t, q


def transform(R, t, m):
    """R m + t per row: ((R0 m0 + R1 m1) + R2 m2) + t; R [N, 9], t [N, 3], m [3] -> [N, 3]"""
    return np.stack([((R[:, 3 * u] * m[0] + R[:, 3 * u + 1] * m[1]) + R[:, 3 * u + 2] * m[2]) + t[:, u] for u in range(3)], axis=1)


def solve_body(det, model, tri, tol, gate, min_markers, max_hyp):
    """One (time step, body): det [n, 3] (n <= 64), model [M, 3], tri [H, 3] -> dict(status, n_in, label [8], R, t, q, rms)"""
    M = len(model)
    none = {"status": LOST, "n_in": 0, "label": np.full(MAX_MARKERS, -1, np.int32), "R": np.zeros(9), "t": np.zeros(3), "q": np.zeros(4),
            "rms": 0.0}
    tri = np.asarray(tri, np.int64).reshape(-1, 3)
    if not (3 <= M <= MAX_MARKERS and 1 <= len(tri) <= MAX_TRIPLES) or \
            not ((0 <= tri[:, 0]) & (tri[:, 0] < tri[:, 1]) & (tri[:, 1] < tri[:, 2]) & (tri[:, 2] < M)).all():
        return dict(none, status=E_MODEL)
    det = np.asarray(det, np.float64).reshape(-1, 3)
    n = len(det)
    if n < 3:
        return none
    mod = np.zeros((MAX_MARKERS, 3))
    mod[:M] = model
    cand = candidates(dist_table(det), dist_table(mod[:M]), tri, tol)
    N = len(cand)
    if N > max_hyp:
        return dict(none, status=E_HYP)
    if N == 0:
        return none
    lab = np.full((N, MAX_MARKERS), -1, np.int64)
    rows = np.arange(N)
    for s in range(3):
        lab[rows, tri[cand[:, 0], s]] = cand[:, 1 + s]
    R, t, _ = horn(mod, det, lab)
    # labels: the model points in ascending p, each takes the nearest unclaimed detection below gate^2 (ties: the lower row)
    g2 = gate * gate
    claimed = np.zeros((N, n), bool)
    lab = np.full((N, MAX_MARKERS), -1, np.int64)
    with np.errstate(all="ignore"):
        for p in range(M):
            e = det[None, :, :] - transform(R, t, mod[p])[:, None, :]
            d2 = (e[:, :, 0] * e[:, :, 0] + e[:, :, 1] * e[:, :, 1]) + e[:, :, 2] * e[:, :, 2]
            ok = ~claimed & (d2 < g2)
            best = np.argmin(np.where(ok, d2, np.inf), axis=1)  # the first of equal minima
            has = ok[rows, best]
            lab[:, p] = np.where(has, best, -1)
            claimed[rows[has], best[has]] = True
        n_in = (lab >= 0).sum(axis=1)
        R2, t2, q2 = horn(mod, det, lab)
        ssq = np.zeros(N)
        for p in range(M):
            e = det[np.where(lab[:, p] >= 0, lab[:, p], 0)] - transform(R2, t2, mod[p])
            d2 = (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]
            ssq = np.where(lab[:, p] >= 0, ssq + d2, ssq)
        rms2 = ssq / n_in
    good = n_in >= min_markers
    if not good.any():
        return none
    top = n_in[good].max()
    among = good & (n_in == top)
    low = rms2[among].min()
    w = int(np.flatnonzero(among & (rms2 == low))[0])  # the candidates stand in ascending (h, i, j, k)
    return {"status": 0, "n_in": int(n_in[w]), "label": lab[w].astype(np.int32), "R": R2[w], "t": t2[w], "q": q2[w],
            "rms": float(np.sqrt(rms2[w])), "n_cand": N, "winner": cand[w], "cand": cand, "cand_n_in": n_in, "cand_rms2": rms2}


def rigid_poses(xyz, n, models, triples, tol, gate, min_markers=3, max_hyp=1024):
    """xyz [T, Q, 3], n [T]; models / triples: lists per body -> dict of arrays [T, B, ...] as mocap_rigid_poses writes them (the
    floats of a (t, b) whose status is not 0 are zeros here and unspecified on the device)"""
    xyz = np.asarray(xyz, np.float64)
    T, Q, B = len(n), xyz.shape[1], len(models)
    out = {"R": np.zeros((T, B, 9)), "t": np.zeros((T, B, 3)), "q": np.zeros((T, B, 4)), "rms": np.zeros((T, B)),
           "n_in": np.zeros((T, B), np.int32), "label": np.full((T, B, MAX_MARKERS), -1, np.int32), "status": np.zeros((T, B), np.int32)}
    for s in range(T):
        for b in range(B):
            if n[s] < 0:
                out["status"][s, b] = E_BLIND
                continue
            if n[s] > min(Q, MAX_DET):
                out["status"][s, b] = E_CAPACITY
                continue
            r = solve_body(xyz[s, :n[s]], np.asarray(models[b], np.float64), triples[b], tol, gate, min_markers, max_hyp)
            for k in out:
                out[k][s, b] = r[k]
    return out


# ---- the seeded scene ----------------------------------------------------------------------------------------------------------
TOL, GATE, NOISE = 0.003, 0.006, 0.0005  # world units (m): the distance test, the label gate, the noise per axis
MIN_AREA = 1e-4


def random_rotation(rng):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def make_body(rng, M, size=0.25, gap=3 * TOL, min_dist=0.05):
    """M points in a cube of edge `size` about the origin, every two of their pairwise distances more than `gap` apart"""
    pts, dists = [], []
    while len(pts) < M:
        p = rng.uniform(-size / 2, size / 2, 3)
        new = [float(np.linalg.norm(p - q)) for q in pts]
        every = np.sort(np.array(dists + new))
        if all(d > min_dist for d in new) and (len(every) < 2 or np.diff(every).min() > gap):
            pts.append(p)
            dists += new
    pts = np.array(pts)
    return pts - pts.mean(axis=0)


def rigid_scene(seed, T=60, sizes=(4, 5, 6), hidden=0.2, clutter=4, noise=NOISE, Q=24):
    """Seeded bodies on random poses, markers hidden with probability `hidden`, `clutter` stray points, Gaussian noise, rows
    shuffled.  -> dict: xyz [T, Q, 3] (NaN beyond n), n [T], models, truth R [T, B, 3, 3], t [T, B, 3], row [T, B, 8] (the row of
    each marker, -1 = hidden or p >= M)"""
    rng = np.random.default_rng(seed)
    models = [make_body(rng, M) for M in sizes]
    B = len(models)
    xyz = np.full((T, Q, 3), np.nan)
    n = np.zeros(T, np.int32)
    Rt, tt = np.zeros((T, B, 3, 3)), np.zeros((T, B, 3))
    row = np.full((T, B, MAX_MARKERS), -1, np.int32)
    for s in range(T):
        pts, owner = [], []
        for b, model in enumerate(models):
            Rt[s, b], tt[s, b] = random_rotation(rng), rng.uniform(-1, 1, 3)
            seen = rng.random(len(model)) >= hidden
            for p in np.flatnonzero(seen):
                pts.append(Rt[s, b] @ model[p] + tt[s, b] + rng.normal(scale=noise, size=3))
                owner.append((b, p))
        for _ in range(clutter):
            pts.append(rng.uniform(-1.2, 1.2, 3))
            owner.append(None)
        perm = rng.permutation(len(pts))
        n[s] = len(pts)
        assert n[s] <= Q
        for r, k in enumerate(perm):
            xyz[s, r] = pts[k]
            if owner[k] is not None:
                row[s, owner[k][0], owner[k][1]] = r
    return {"xyz": xyz, "n": n, "models": models, "R": Rt, "t": tt, "row": row}


def pose_errors(R, t, R_true, t_true):
    """(angle in radians between the rotations, distance between the translations)"""
    c = (np.trace(np.asarray(R).reshape(3, 3).T @ R_true) - 1.0) / 2.0
    return float(np.arccos(np.clip(c, -1.0, 1.0))), float(np.linalg.norm(np.asarray(t) - t_true))


def scene_report(sc, res, min_markers=3):
    """What the host test asserts and its docstring quotes: wrong labels, lost bodies among those with enough visible markers,
    poses of bodies with fewer, and the worst pose errors"""
    wrong = lost = ghost = found = 0
    ang = tra = 0.0
    T, B = res["status"].shape
    for s in range(T):
        for b in range(B):
            visible = int((sc["row"][s, b] >= 0).sum())
            if res["status"][s, b] != 0:
                lost += visible >= min_markers
                continue
            if visible < min_markers:
                ghost += 1
                continue
            found += 1
            lab = res["label"][s, b]
            wrong += int(((lab >= 0) & (lab != sc["row"][s, b])).sum())
            a, d = pose_errors(res["R"][s, b], res["t"][s, b], sc["R"][s, b], sc["t"][s, b])
            ang, tra = max(ang, a), max(tra, d)
    return {"wrong": wrong, "lost": lost, "ghost": ghost, "found": found, "angle": ang, "translation": tra}


def lattice_case():
    """(detections, model): the four corners of a regular tetrahedron, every two of them exactly sqrt(0.08) apart, and an
    equilateral model triangle of that side -- all 4 * 3 * 2 = 24 ordered triples are candidates of its one model triple"""
    tet = np.array([[1.0, 1.0, 1.0], [1.0, -1.0, -1.0], [-1.0, 1.0, -1.0], [-1.0, -1.0, 1.0]]) * 0.1
    return tet, tet[:3].copy()


# ---- candidate lists longer than the workgroup ------------------------------------------------------------------------------------
# Every detection is an exact lattice or tetrahedron point: the lattice's distances are 0.125 sqrt(m), the nearest two of them
# (0.125 and 0.125 sqrt(2)) 0.05 apart, against TOL = 0.003 and noise of 2e-4 per axis -- no |d - L| < tol is ever close.
SPACING, LATTICE_NOISE = 0.125, 2e-4
SQUARE = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [1.0, 1.0, 0.0], [0.0, 1.0, 0.0]]) * SPACING
TRIANGLE = SQUARE[:3].copy()
CUBE = np.array([[x, y, z] for z in (0.0, 1.0) for y in (0.0, 1.0) for x in (0.0, 1.0)]) * SPACING
N_SQUARE, N_TRIANGLE, N_CUBE, N_SQUARE_TIES = 3456, 864, 46656, 912  # test_rigid_host asserts each from the restatement


def lattice(noise=0.0, seed=22):
    """The 4 x 4 x 4 lattice of spacing 0.125 -- 64 detections, the most a step holds -- with its rows in a seeded permutation
    (the same one with and without noise), and N(0, noise) added per axis"""
    rng = np.random.default_rng(seed)
    g = np.arange(4) * SPACING
    pts = np.array([[x, y, z] for z in g for y in g for x in g])[rng.permutation(64)]
    return pts + rng.normal(scale=noise, size=pts.shape) if noise else pts


def lattice_steps():
    """(xyz [2, 64, 3], n [2]): the exact lattice and the noisy one as the two time steps of one call"""
    return np.stack([lattice(), lattice(LATTICE_NOISE)]), np.array([64, 64], np.int32)


def tetrahedra(k):
    """k copies of lattice_case()'s tetrahedron, 5.0 apart along x and y: 24 k candidates for its equilateral model, all of rms 0"""
    tet, model = lattice_case()
    return np.concatenate([tet + [5.0 * (i % 4), 5.0 * (i // 4), 0.0] for i in range(k)]), model
