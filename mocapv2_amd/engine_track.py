"""The tracking stages of MocapContext (abi_track.hip, abi_rigid.hip): marker identities across time steps and rigid-body
poses per time step, both from the 3-D markers of the correspondence calls."""
import numpy as np
import torch

from . import _abi
from ._dev import _ptr, _stream, marker_rows, outputs

RIGID_LOST, RIGID_E_BLIND, RIGID_E_CAPACITY, RIGID_E_MODEL, RIGID_E_HYP = 1, -2, -3, -4, -5  # MOCAP_RIGID_*
RIGID_MAX_DETECTIONS, RIGID_MAX_MARKERS, RIGID_MAX_TRIPLES, RIGID_MAX_BODIES, RIGID_MAX_HYP = 64, 8, 56, 16, 4096
LEARN_E_MEMBERS, LEARN_E_INCOMPLETE = -2, -3                    # MOCAP_LEARN_E_*
LEARN_CHUNK, LEARN_MAX_IDS, LEARN_MAX_GROUPS = 32, 64, 16      # MOCAP_LEARN_*


def learn_work_bytes(T, K, G):
    """MOCAP_LEARN_WORK_BYTES(T, K, G): the workspace of marker_pair_stats (G = 0) or rigid_learn (K = 0)"""
    chunks = (T + LEARN_CHUNK - 1) // LEARN_CHUNK
    return chunks * (36 * (K * (K + 1) // 2) + 228 * G) + 4 * T * (K + 8 * G) + 200 * G


def rigid_groups(ids, count, dmin, dmax, spread, min_steps):
    """The grouping of learn_rigid_bodies over the K x K pair tables (host arrays): a pair is rigid when count >= min_steps and
    dmax - dmin <= spread; the lowest unassigned identity seeds a group, and each later unassigned identity, in ascending order,
    joins if it is rigid with every current member.  Returns (groups, unassigned): lists of identities per body of 3 to 8
    members, and the identities of the smaller groups.  ValueError: a group of more than 8, or more than 16 bodies."""
    ids = [int(i) for i in ids]
    K = len(ids)
    rigid = (np.asarray(count) >= min_steps) & (np.asarray(dmax) - np.asarray(dmin) <= spread)
    free = [True] * K
    groups, unassigned = [], []
    for a in range(K):
        if not free[a]:
            continue
        members = [a]
        for b in range(a + 1, K):
            if free[b] and all(rigid[m, b] for m in members):
                members.append(b)
        if len(members) > RIGID_MAX_MARKERS:
            raise ValueError(f"identities {[ids[m] for m in members]} keep their distances within spread = {spread}: a body of "
                             f"{len(members)} markers, more than {RIGID_MAX_MARKERS} (did the bodies move against one another?)")
        if len(members) >= 3:
            groups.append([ids[m] for m in members])
            for m in members:
                free[m] = False
        else:
            free[a] = False
            unassigned.append(ids[a])
    if len(groups) > LEARN_MAX_GROUPS:
        raise ValueError(f"{len(groups)} bodies, more than {LEARN_MAX_GROUPS}: {groups}")
    return groups, unassigned


def rigid_tables(models, min_area=1e-4):
    """The padded host tables of mocap_rigid_poses for a list of bodies ([M, 3] model points each): model [B, 8, 3] float64,
    n_markers [B], tri [B, 56, 3] (every triple a < b < c whose triangle area exceeds min_area, in ascending order), n_tri [B]
    int32.  ValueError: no body or more than 16, M outside 3..8, points that are not finite, a body with no such triple."""
    from itertools import combinations
    B = len(models)
    if not 1 <= B <= RIGID_MAX_BODIES:
        raise ValueError(f"{B} bodies: 1..{RIGID_MAX_BODIES}")
    model = np.zeros((B, RIGID_MAX_MARKERS, 3), np.float64)
    tri = np.zeros((B, RIGID_MAX_TRIPLES, 3), np.int32)
    n_markers, n_tri = np.zeros(B, np.int32), np.zeros(B, np.int32)
    for b, m in enumerate(models):
        m = np.asarray(m, np.float64)
        if m.ndim != 2 or m.shape[1] != 3 or not 3 <= m.shape[0] <= RIGID_MAX_MARKERS:
            raise ValueError(f"body {b}: model points of shape {m.shape}; [M, 3] with M in 3..{RIGID_MAX_MARKERS}")
        if not np.isfinite(m).all():
            raise ValueError(f"body {b}: model points that are not finite")
        M = m.shape[0]
        keep = [(a, c, d) for a, c, d in combinations(range(M), 3)
                if 0.5 * np.linalg.norm(np.cross(m[c] - m[a], m[d] - m[a])) > min_area]
        if not keep:
            raise ValueError(f"body {b}: no triple of its {M} points spans a triangle of more than min_area = {min_area}")
        model[b, :M], n_markers[b] = m, M
        tri[b, :len(keep)], n_tri[b] = keep, len(keep)
    return {"model": model, "n_markers": n_markers, "tri": tri, "n_tri": n_tri}


class TrackStage:
    def track_state(self, max_tracks):
        """The state buffer of one tracker for track_markers (MOCAP_TRACK_STATE_BYTES: a 64-byte header and one 64-byte record per
        slot, include/mocap_hip.h), zeroed = the empty tracker.  The caller owns it; NumPy reads a copy of it with a structured dtype."""
        if not 1 <= int(max_tracks) <= 256:
            raise ValueError(f"max_tracks {max_tracks}: 1..256")
        return torch.zeros(64 * (1 + int(max_tracks)), dtype=torch.uint8, device=self.device)

    def track_markers(self, xyz, n, state, gate, beta=0.5, max_miss=5, out=None, steps=None):
        """Marker identities across time steps (mocap_track_markers; the definition is DESIGN.md section 2).  xyz [T, Q, 3] float64
        and n [T] int32 on the GPU (correspond_visible's xyz and n as they are: a negative count is a blind step), state from
        track_state (updated in place; calls on one state must be ordered on the device), gate in world units.  steps: only the
        first `steps` time steps are walked (a batch padded at its end must not age the tracks).  Returns a dict of device
        tensors: id, slot, age [T, Q] int32 (-1 = the row holds no tracked detection) and status [T] int32 (0 or MOCAP_TRACK_E_*);
        the rows of time steps at and beyond `steps` are not written (a fresh `out` holds -1 / 0 there)."""
        T, Q = marker_rows(xyz, n)
        assert state.is_cuda and state.is_contiguous()
        steps = T if steps is None else int(steps)
        if not 0 <= steps <= T:
            raise ValueError(f"steps {steps} outside 0..{T}")
        nbytes = state.numel() * state.element_size()
        max_tracks = nbytes // 64 - 1
        if nbytes % 64 or max_tracks < 1:
            raise ValueError(f"a state of {nbytes} bytes is not one of track_state()")
        out = outputs({**{k: ((T, Q), torch.int32, -1) for k in ("id", "slot", "age")}, "status": ((T,), torch.int32, 0)}, self.device, out)
        _abi.check(self.lib.mocap_track_markers(self._h, _ptr(xyz), _ptr(n), steps, Q, _ptr(state), max_tracks, float(gate), float(beta),
                                                int(max_miss), _ptr(out["id"]), _ptr(out["slot"]), _ptr(out["age"]),
                                                _ptr(out["status"]), _stream()))
        return out

    def rigid_bodies(self, models, min_area=1e-4, names=None):
        """The device tables of rigid bodies for rigid_poses, uploaded once.  models: a list of [M, 3] arrays (3 <= M <= 8 model
        points in the body's own frame, at most 16 bodies).  Every model triple a < b < c whose triangle area exceeds min_area
        (world units squared) is listed: a body whose triples are all degenerate is refused.  Returns the handle dict: model
        [B, 8, 3] float64, n_markers [B], tri [B, 56, 3], n_tri [B] int32 on the GPU, and the host copies `models` and `names`."""
        tables = rigid_tables(models, min_area)
        out = {k: torch.from_numpy(v).to(self.device) for k, v in tables.items()}
        out["models"] = [np.array(m, np.float64).reshape(-1, 3) for m in models]
        out["names"] = list(names) if names is not None else [f"body{b + 1}" for b in range(len(models))]
        if len(out["names"]) != len(models):
            raise ValueError(f"{len(out['names'])} names for {len(models)} bodies")
        return out

    def rigid_poses(self, xyz, n, bodies, tol, gate, min_markers=3, max_hyp=1024, out=None):
        """Rigid-body poses per time step (mocap_rigid_poses; the definition is DESIGN.md section 2).  xyz [T, Q, 3] float64 and
        n [T] int32 on the GPU (correspond_visible's xyz and n as they are: a negative count is a blind step), bodies from
        rigid_bodies, tol (the distance test) and gate (the label gate) in world units.  Returns a dict of device tensors:
        R [T, B, 9], t [T, B, 3], q [T, B, 4] (w, x, y, z), rms [T, B] float64; n_in [T, B], label [T, B, 8] (the detection row of
        each model point or -1), status [T, B] int32 (0, RIGID_LOST = 1, or RIGID_E_* < 0).  Where status is not 0, n_in is 0, the
        labels are -1 and the floats are unspecified and must not be read."""
        T, Q = marker_rows(xyz, n)
        B = int(bodies["model"].shape[0])
        f64, i32 = torch.float64, torch.int32
        out = outputs({"R": ((T, B, 9), f64, 0), "t": ((T, B, 3), f64, 0), "q": ((T, B, 4), f64, 0), "rms": ((T, B), f64, 0),
                       "n_in": ((T, B), i32, 0), "label": ((T, B, 8), i32, -1), "status": ((T, B), i32, 0)}, self.device, out)
        _abi.check(self.lib.mocap_rigid_poses(self._h, _ptr(xyz), _ptr(n), T, Q, B, _ptr(bodies["model"]), _ptr(bodies["n_markers"]),
                                              _ptr(bodies["tri"]), _ptr(bodies["n_tri"]), float(tol), float(gate), int(min_markers),
                                              int(max_hyp), _ptr(out["R"]), _ptr(out["t"]), _ptr(out["q"]), _ptr(out["rms"]),
                                              _ptr(out["n_in"]), _ptr(out["label"]), _ptr(out["status"]), _stream()))
        return out

    def _take(self, xyz, n, id):
        T, Q = marker_rows(xyz, n)
        assert id.is_cuda and id.is_contiguous() and id.dtype == torch.int32 and tuple(id.shape) == (T, Q), (id.shape, T, Q)
        return T, Q

    def marker_pair_stats(self, xyz, n, id, ids, out=None):
        """The distance statistics of every two of K marker identities over a take (mocap_learn_marker_pair_stats, libmocap_learn.so; the definition is
        DESIGN.md section 2).  xyz [T, Q, 3] float64, n [T] int32 and id [T, Q] int32 on the GPU: the markers and track_markers'
        identities as they are.  ids: K host integers, strictly ascending, non-negative, 2 <= K <= 64 (anything else raises
        MocapError before anything is launched).  Returns a dict of device tensors [K, K]: count int32, dmin, dmax, dsum, dsum2
        float64, symmetric; the diagonal's count is the number of steps the identity is present in."""
        T, Q = self._take(xyz, n, id)
        ids = np.ascontiguousarray(ids, np.int32).reshape(-1)
        K = int(ids.size)
        f64 = torch.float64
        out = outputs({"count": ((K, K), torch.int32, 0), **{k: ((K, K), f64, 0) for k in ("dmin", "dmax", "dsum", "dsum2")}}, self.device, out)
        nbytes = learn_work_bytes(T, K, 0) if 2 <= K <= LEARN_MAX_IDS else 8
        work = torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=self.device)
        _abi.check_learn(_abi.load_learn().mocap_learn_marker_pair_stats(self.device.index or 0, _ptr(xyz), _ptr(n), _ptr(id), T, Q, ids.ctypes.data, K, _ptr(work), nbytes,
                                                    _ptr(out["count"]), _ptr(out["dmin"]), _ptr(out["dmax"]), _ptr(out["dsum"]),
                                                    _ptr(out["dsum2"]), _stream()))
        return out

    def rigid_learn(self, xyz, n, id, members, rounds=2, min_present=3, out=None):
        """The model of each of G groups of marker identities, averaged over a take in the group's own frame (mocap_learn_rigid_bodies, libmocap_learn.so; the
        definition is DESIGN.md section 2).  members: a list of G lists of identities (1 <= G <= 16; 3 to 8 distinct non-negative
        identities each, or the group's status says MOCAP_LEARN_E_MEMBERS).  Returns a dict of device tensors: model [G, 8, 3],
        rms [G], member_rms [G, 8] float64; member_count [G, 8], steps_used, ref_step, status [G] int32.  Where status is not 0
        the counts are 0, ref_step is -1 and the floats must not be read.  A model's origin is its centroid, its axes are the
        world's as they stood at ref_step."""
        T, Q = self._take(xyz, n, id)
        G = len(members)
        member_id = np.full((max(G, 1), RIGID_MAX_MARKERS), -1, np.int32)
        n_members = np.zeros(max(G, 1), np.int32)
        for g, m in enumerate(members):
            n_members[g] = len(m)
            member_id[g, :min(len(m), RIGID_MAX_MARKERS)] = list(m)[:RIGID_MAX_MARKERS]
        f64, i32 = torch.float64, torch.int32
        out = outputs({"model": ((G, 8, 3), f64, 0), "rms": ((G,), f64, 0), "member_rms": ((G, 8), f64, 0), "member_count": ((G, 8), i32, 0),
                       "steps_used": ((G,), i32, 0), "ref_step": ((G,), i32, -1), "status": ((G,), i32, 0)}, self.device, out)
        nbytes = learn_work_bytes(T, 0, G) if 1 <= G <= LEARN_MAX_GROUPS else 8
        work = torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=self.device)
        _abi.check_learn(_abi.load_learn().mocap_learn_rigid_bodies(self.device.index or 0, _ptr(xyz), _ptr(n), _ptr(id), T, Q, G, member_id.ctypes.data, n_members.ctypes.data,
                                              int(rounds), int(min_present), _ptr(work), nbytes, _ptr(out["model"]), _ptr(out["rms"]),
                                              _ptr(out["member_rms"]), _ptr(out["member_count"]), _ptr(out["steps_used"]),
                                              _ptr(out["ref_step"]), _ptr(out["status"]), _stream()))
        return out

    def learn_rigid_bodies(self, xyz, n, id, *, spread, min_steps, ids=None, rounds=2, min_present=3, min_area=1e-4, names=None):
        """Rigid-body models from a tracked capture in which the bodies were waved through the volume: the identities that keep
        their mutual distances are a body, and its averaged shape is the model.  xyz, n, id as marker_pair_stats takes them.
        spread (world units): a pair is rigid when it was seen together in at least min_steps steps and its distance varied by at
        most spread (max - min) -- one identity swap breaks a pair, and the tables are returned so the caller sees it.  ids: the
        identities to consider; None = those present in at least min_steps steps (more than 64: the 64 with the most
        detections, ties to the lower identity).  The grouping (rigid_groups) runs on the host; groups of 3 to 8 become bodies.
        Returns a dict: models (a list of [M, 3] arrays, ready for rigid_bodies and for bodies={"models": ...}), members (the
        identities per body), rms, member_rms, member_count, steps_used, ref_step, status (host arrays per body; a body whose
        status is not 0 is reported, not dropped, with a model of zeros), names, unassigned, ids, and pairs (the host copies of
        marker_pair_stats' tables).  ValueError: fewer than two identities, a group of more than 8 identities or more than 16
        bodies (a take in which the bodies never moved against one another), or a learned shape that rigid_tables refuses."""
        T, Q = self._take(xyz, n, id)
        if ids is None:
            nh, idh = n.cpu().numpy()[:T], id.cpu().numpy()
            live = (np.arange(Q)[None, :] < np.where((nh < 0) | (nh > Q), 0, nh)[:, None]) & (idh >= 0)
            # a step counts an identity once, however many rows hold it
            per_step = np.unique(np.stack([np.broadcast_to(np.arange(T)[:, None], idh.shape)[live], idh[live]], axis=1), axis=0)
            seen, steps = np.unique(per_step[:, 1], return_counts=True) if len(per_step) else (np.zeros(0, np.int64), np.zeros(0, np.int64))
            keep = steps >= min_steps
            seen, steps = seen[keep], steps[keep]
            if len(seen) > LEARN_MAX_IDS:
                seen = seen[np.lexsort((seen, -steps))[:LEARN_MAX_IDS]]
            ids = np.sort(seen)
        ids = np.ascontiguousarray(ids, np.int32).reshape(-1)
        if ids.size < 2:
            raise ValueError(f"{ids.size} identities with at least min_steps = {min_steps} steps: a body needs three")
        pairs = {k: v.cpu().numpy() for k, v in self.marker_pair_stats(xyz, n, id, ids).items()}
        groups, unassigned = rigid_groups(ids, pairs["count"], pairs["dmin"], pairs["dmax"], spread, min_steps)
        res = {"members": groups, "unassigned": unassigned, "ids": ids, "pairs": pairs}
        if groups:
            learned = {k: v.cpu().numpy() for k, v in self.rigid_learn(xyz, n, id, groups, rounds, min_present).items()}
        else:
            learned = {"model": np.zeros((0, 8, 3)), "rms": np.zeros(0), "member_rms": np.zeros((0, 8)), "member_count": np.zeros((0, 8), np.int32),
                       "steps_used": np.zeros(0, np.int32), "ref_step": np.zeros(0, np.int32), "status": np.zeros(0, np.int32)}
        res["models"] = [np.where(learned["status"][g] == 0, learned["model"][g, :len(m)], 0.0) for g, m in enumerate(groups)]
        good = [m for g, m in enumerate(res["models"]) if learned["status"][g] == 0]
        if good:
            rigid_tables(good, min_area)  # a degenerate shape is refused with that function's message
        res.update({k: learned[k] for k in ("rms", "member_rms", "member_count", "steps_used", "ref_step", "status")})
        res["names"] = list(names) if names is not None else [f"body{b + 1}" for b in range(len(groups))]
        if len(res["names"]) != len(groups):
            raise ValueError(f"{len(res['names'])} names for {len(groups)} bodies")
        return res
