"""The tracking stages of MocapContext (abi_track.hip, abi_rigid.hip): marker identities across time steps and rigid-body
poses per time step, both from the 3-D markers of the correspondence calls."""
import numpy as np
import torch

from . import _abi
from ._dev import _ptr, _stream, marker_rows, outputs

RIGID_LOST, RIGID_E_BLIND, RIGID_E_CAPACITY, RIGID_E_MODEL, RIGID_E_HYP = 1, -2, -3, -4, -5  # MOCAP_RIGID_*
RIGID_MAX_DETECTIONS, RIGID_MAX_MARKERS, RIGID_MAX_TRIPLES, RIGID_MAX_BODIES, RIGID_MAX_HYP = 64, 8, 56, 16, 4096


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
