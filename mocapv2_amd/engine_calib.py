"""The calibration stage of MocapContext (abi_calib.hip): fundamental matrices by RANSAC, the rig bundle adjustments, intrinsics
from board views.  A problem's layout rules are checked over NumPy (rig_problem, board_problem), before any GPU work."""
import ctypes as C

import numpy as np
import torch

from . import _abi
from ._dev import _ptr, _stream

RIG_LOSSES = {"none": 0, "cauchy": 1}  # MOCAP_RIG_LOSS_*
_IP = C.POINTER(C.c_int)
_FEW_OBS = ", or a camera has fewer observations than twice the lens parameters its mask frees"


def rig_problem(obs_offset, obs_cam, obs_uv, poses, points):
    """A rig problem in the layout of mocap_rig_bundle_adjust, checked: (C, N, n_obs, obs_offset int32 [N + 1], obs_cam int32
    [n_obs], obs_uv [n_obs][2], poses [C][12], points [N][3]) as contiguous host arrays.  ValueError with the reason, where the
    kernel would only say MOCAP_RIG_E_LAYOUT."""
    off = np.ascontiguousarray(obs_offset, np.int32).reshape(-1)
    cam = np.ascontiguousarray(obs_cam, np.int32).reshape(-1)
    uv = np.ascontiguousarray(obs_uv, np.float64).reshape(-1, 2)
    poses = np.ascontiguousarray(poses, np.float64)
    points = np.ascontiguousarray(points, np.float64).reshape(-1, 3)
    Cn, N, n_obs = len(poses), len(points), len(cam)
    if poses.shape != (Cn, 12) or not 2 <= Cn <= 32:
        raise ValueError(f"poses must be [2..32][12] (R row-major, then t), got {poses.shape}")
    if len(off) != N + 1 or off[0] != 0 or off[-1] != n_obs or len(uv) != n_obs or N < 1:
        raise ValueError(f"obs_offset must be [N + 1 = {N + 1}] from 0 to n_obs = {n_obs}, obs_uv [n_obs][2]")
    cnt = np.diff(off)
    if (cnt < 2).any() or (cnt > Cn).any():
        raise ValueError("every point needs 2..C observations")
    if cam.min() < 0 or cam.max() >= Cn:
        raise ValueError(f"obs_cam outside 0..{Cn - 1}")
    inner = np.ones(n_obs, bool)
    inner[off[:-1]] = False
    if (np.diff(cam, prepend=-1)[inner] <= 0).any():
        raise ValueError("a point's observations must come in strictly ascending camera order")
    if not (np.isfinite(uv).all() and np.isfinite(poses).all() and np.isfinite(points).all()):
        raise ValueError("observations, poses and points must be finite")
    return Cn, N, n_obs, off, cam, uv, poses, points


def board_problem(view_offset, point_offset, obj_xy, img_uv):
    """A board-view problem in the layout of mocap_intrinsics_calibrate: (n_cams, n_views, view_offset, point_offset int32,
    obj_xy, img_uv [total][2]) as contiguous host arrays.  Only the shapes are checked here: what a camera or a view lacks
    (3 views, 4 points a view, 2 points >= 9 + 6 views) is that camera's MOCAP_INTR_E_LAYOUT."""
    voff = np.ascontiguousarray(view_offset, np.int32).reshape(-1)
    poff = np.ascontiguousarray(point_offset, np.int32).reshape(-1)
    obj = np.ascontiguousarray(obj_xy, np.float64).reshape(-1, 2)
    img = np.ascontiguousarray(img_uv, np.float64).reshape(-1, 2)
    n_cams = len(voff) - 1
    if n_cams < 1 or voff[0] != 0 or (np.diff(voff) < 0).any():
        raise ValueError("view_offset must be [n_cams + 1], from 0, not descending")
    n_views = int(voff[-1])
    if n_views < 1 or len(poff) != n_views + 1 or poff[0] != 0 or (np.diff(poff) < 0).any():
        raise ValueError(f"point_offset must be [n_views + 1 = {n_views + 1}], from 0, not descending")
    if len(obj) != poff[-1] or len(img) != poff[-1] or len(obj) < 1:
        raise ValueError(f"obj_xy and img_uv must be [{poff[-1]}][2], got {obj.shape} and {img.shape}")
    if not (np.isfinite(obj).all() and np.isfinite(img).all()):
        raise ValueError("board points and pixels must be finite")
    return n_cams, n_views, voff, poff, obj, img


class CalibStage:
    def _upload(self, *arrays):
        return [torch.from_numpy(a).to(self.device) for a in arrays]

    def _zeros(self, *shapes, dtype=torch.float64):
        return [torch.zeros(s, dtype=dtype, device=self.device) for s in shapes]

    def fundamental_ransac(self, pairs, samples, threshold, refit=True, with_counts=False):
        """Fundamental matrices of a batch of camera pairs by RANSAC (mocap_fundamental_ransac; reference
        CalculateCameraPoses.py:189 per pair): one upload, ONE call, one sync.
        pairs: list of (a [N_p, 2], b [N_p, 2]) host arrays, the same markers in the first and the second camera (N_p >= 8);
        samples: int32 [n_pairs, H, 8] (or a list of [H, 8] tables, e.g. calibrate.sample_table): 8 distinct point indices per
        hypothesis, local to the pair.  Returns one dict per pair: F_sample, F_refit (3x3, unit Frobenius norm, x_b^T F x_a =
        0; F_refit None without refit), mask (uint8 [N_p]: inliers of the best sample), best (its index), n_inliers, and counts
        (int32 [H]) with with_counts.  A failed pair has best < 0 (MOCAP_FUND_E_*), no matrices and an all-zero mask."""
        n_pairs = len(pairs)
        if n_pairs < 1:
            raise ValueError("no pairs")
        lists_a, lists_b, offset = [], [], [0]
        for p, (a, b) in enumerate(pairs):
            a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
            if a.ndim != 2 or a.shape[1] != 2 or a.shape != b.shape:
                raise ValueError(f"pair {p}: point lists must both be [N][2], got {a.shape} and {b.shape}")
            lists_a.append(a)
            lists_b.append(b)
            offset.append(offset[-1] + len(a))
        smp = np.ascontiguousarray(np.stack([np.asarray(s) for s in samples]) if isinstance(samples, (list, tuple)) else samples,
                                   np.int32)
        if smp.ndim != 3 or smp.shape[0] != n_pairs or smp.shape[2] != 8:
            raise ValueError(f"samples must be [n_pairs = {n_pairs}][H][8], got {smp.shape}")
        H, offset = smp.shape[1], np.array(offset, np.int32)
        total = int(offset[-1])
        dev = self.device
        d_a, d_b, d_s = self._upload(np.concatenate(lists_a), np.concatenate(lists_b), smp)
        F_s = torch.full((n_pairs, 9), float("nan"), dtype=torch.float64, device=dev)
        F_r = torch.full((n_pairs, 9), float("nan"), dtype=torch.float64, device=dev) if refit else None
        mask = torch.empty((max(total, 1),), dtype=torch.uint8, device=dev)
        status = torch.empty((n_pairs, 2), dtype=torch.int32, device=dev)
        counts = torch.empty((n_pairs, H), dtype=torch.int32, device=dev) if with_counts else None
        _abi.check(self.lib.mocap_fundamental_ransac(self._h, n_pairs, _ptr(d_a), _ptr(d_b), offset.ctypes.data_as(_IP),
                                                     _ptr(d_s), H, float(threshold), int(bool(refit)), _ptr(F_s), _ptr(F_r),
                                                     _ptr(mask), _ptr(status), _ptr(counts), _stream()))
        self.sync()
        F_s, status, mask = F_s.cpu().numpy(), status.cpu().numpy(), mask.cpu().numpy()
        F_r = F_r.cpu().numpy() if refit else None
        counts = counts.cpu().numpy() if with_counts else None
        out = []
        for p in range(n_pairs):
            ok = status[p, 0] >= 0
            r = {"best": int(status[p, 0]), "n_inliers": int(status[p, 1]) if ok else 0,
                 "F_sample": F_s[p].reshape(3, 3).copy() if ok else None,
                 "F_refit": F_r[p].reshape(3, 3).copy() if ok and refit else None,
                 "mask": mask[offset[p]:offset[p + 1]].copy()}
            if with_counts:
                r["counts"] = counts[p].copy()
            out.append(r)
        return out

    @staticmethod
    def _rig_loss(loss, loss_scale):
        """(MOCAP_RIG_LOSS_* number, scale) of the loss keywords: a name of RIG_LOSSES, or a number handed to the library as it
        is (which refuses what it does not know)"""
        if isinstance(loss, str):
            if loss not in RIG_LOSSES:
                raise ValueError(f"loss {loss!r}: one of {sorted(RIG_LOSSES)}")
            loss = RIG_LOSSES[loss]
        return int(loss), 0.0 if loss_scale is None else float(loss_scale)

    def _rig_lenses(self, intrinsics, refine, Cn):
        """(device copy of intrinsics [C][9], host int32 mask [C]) of the entries that refine the lenses.  Only the shapes are
        checked here: what the values lack is the library's MOCAP_E_INVALID."""
        kd = np.ascontiguousarray(intrinsics, np.float64)
        if kd.shape != (Cn, 9):
            raise ValueError(f"intrinsics must be [{Cn}][9] (fx, fy, cx, cy, k1, k2, p1, p2, k3), got {kd.shape}")
        mask = np.ascontiguousarray(np.broadcast_to(np.asarray(refine, np.int32), (Cn,)))
        return torch.from_numpy(kd).to(self.device), mask

    def _rig_setup(self, problem, loss, loss_scale, intrinsics, refine):
        """What the rig entries share before their call: the loss, rig_problem's checks, the upload.  Returns (selfcal, robust, Cn,
        N, n_obs, dev, lens): lenses are given (they are used, not set_cameras', and loss=None is "none"); () or (loss number,
        scale); the sizes; the device copies [obs_offset, obs_cam, obs_uv, poses, points]; None or _rig_lenses' pair"""
        selfcal = intrinsics is not None
        robust = () if loss is None and not selfcal else self._rig_loss(0 if loss is None else loss, loss_scale)
        Cn, N, n_obs, *arrays = rig_problem(*problem)
        if not selfcal and self.n_cam < Cn:
            raise ValueError(f"set_cameras: {self.n_cam} cameras set, {Cn} needed (their K and dist are used)")
        return selfcal, robust, Cn, N, n_obs, self._upload(*arrays), self._rig_lenses(intrinsics, refine, Cn) if selfcal else None

    def _rig_entry(self, name, selfcal, robust, Cn, N, n_obs, dev, lens, own, per_obs=()):
        """The call of the form of entry `name` that _rig_setup's answer names -- plain, _robust (loss and scale follow the entry's
        own arguments, then the per-observation results) or _intrinsics (also: the lenses follow the observations) -- and the sync"""
        lenses = (_ptr(lens[0]), lens[1].ctypes.data_as(_IP)) if selfcal else ()
        fn = getattr(self.lib, name + ("_intrinsics" if selfcal else "_robust" if robust else ""))
        _abi.check(fn(self._h, Cn, N, n_obs, *map(_ptr, dev[:3]), *lenses, *map(_ptr, dev[3:]), *own, *robust, *map(_ptr, per_obs),
                      _stream()))
        self.sync()

    def rig_linearize(self, obs_offset, obs_cam, obs_uv, poses, points, lam, loss=None, loss_scale=None):
        """The pieces of one iteration of rig_bundle_adjust at a given state and damping (mocap_rig_linearize): dict with cost
        (1/2 sum r^2), gradient [6 (C - 1) + 3 N], S [D][D] (damped reduced camera matrix), rhs [D], behind (a point is not
        in front of a camera that sees it).  Arguments as rig_bundle_adjust; K and dist come from set_cameras.  loss,
        loss_scale: as rig_bundle_adjust's (mocap_rig_linearize_robust: cost 1/2 sum rho, the rest from the weighted blocks)."""
        return self._rig_linearize(obs_offset, obs_cam, obs_uv, poses, points, lam, loss, loss_scale)

    def rig_linearize_intrinsics(self, obs_offset, obs_cam, obs_uv, intrinsics, refine, poses, points, lam, loss=None, loss_scale=None):
        """The pieces of one iteration of rig_bundle_adjust_intrinsics at a given state and damping
        (mocap_rig_linearize_intrinsics): dict with cost, gradient [15 C + 3 N] (per camera the 9 lens parameters, then the 6 of
        the pose; then the points), S [15 C][15 C], rhs [15 C], behind.  Arguments as rig_bundle_adjust's."""
        return self._rig_linearize(obs_offset, obs_cam, obs_uv, poses, points, lam, loss, loss_scale, intrinsics, refine)

    def _rig_linearize(self, obs_offset, obs_cam, obs_uv, poses, points, lam, loss, loss_scale, intrinsics=None, refine=None):
        """The one body of rig_linearize and rig_linearize_intrinsics: upload, the entry the arguments name, sync, dict"""
        setup = self._rig_setup((obs_offset, obs_cam, obs_uv, poses, points), loss, loss_scale, intrinsics, refine)
        selfcal, _, Cn, N = setup[:4]
        D = 15 * Cn if selfcal else 6 * (Cn - 1)
        res = self._zeros((1,), (D + 3 * N,), (D, D), (D,)) + self._zeros((2,), dtype=torch.int32)  # cost, gradient, S, rhs, status
        self._rig_entry("mocap_rig_linearize", *setup, (float(lam), *map(_ptr, res)))
        cost, grad, S, rhs, status = (r.cpu().numpy() for r in res)
        if status[0]:
            raise _abi.MocapError(-2, "mocap_rig_linearize" + ("_intrinsics" if selfcal else "") + ": the observation arrays break the "
                                  "layout rules" + (_FEW_OBS if selfcal else "") + " (MOCAP_RIG_E_LAYOUT)")
        return {"cost": float(cost[0]), "gradient": grad, "S": S, "rhs": rhs, "behind": bool(status[1])}

    def rig_bundle_adjust(self, obs_offset, obs_cam, obs_uv, poses, points, max_iters=50, ftol=1e-12, lambda0=1e-3, loss=None,
                          loss_scale=None):
        """Bundle adjustment of a whole rig on the device (mocap_rig_bundle_adjust; the N-camera, partial-visibility
        generalisation of reference lib/Helpers.py:158-176): one upload, ONE call that enqueues every iteration, one sync.
        obs_offset int32 [N + 1], obs_cam int32 [n_obs] (true camera numbers, ascending within a point), obs_uv [n_obs][2]:
        the observations, point-major; poses [C][12] (R row-major, then t; camera 0 is the identity), points [N][3]: the
        start.  K and dist come from set_cameras.  Returns dict: poses [C][12], points [N][3] (|t_1| as at the start),
        status (MOCAP_RIG_STOP_* > 0), iterations, cost_initial, cost (1/2 sum r^2), history [iterations][4] = (cost after
        the iteration, lambda it was solved with, accepted, |step|).  A negative status (MOCAP_RIG_E_*) raises MocapError:
        nothing is returned silently wrong.
        loss: None (mocap_rig_bundle_adjust), or "none" / "cauchy" with loss_scale = c in pixels
        (mocap_rig_bundle_adjust_robust: rho(s) = c^2 log1p(s / c^2) of s = |r|^2 per observation, first-order reweighting,
        costs 1/2 sum rho; "none" gives the bits of loss=None).  The robust call returns two more keys: obs_err [n_obs], the
        length of every observation's unweighted residual at the returned state, and obs_weight [n_obs], its weight
        1 / (1 + s / c^2) there (1 for "none")."""
        return self._rig_bundle_adjust(obs_offset, obs_cam, obs_uv, poses, points, max_iters, ftol, lambda0, loss, loss_scale)

    def rig_bundle_adjust_intrinsics(self, obs_offset, obs_cam, obs_uv, intrinsics, refine, poses, points, max_iters=50, ftol=1e-12,
                                     lambda0=1e-3, loss=None, loss_scale=None):
        """rig_bundle_adjust with the cameras' lenses among the unknowns (mocap_rig_bundle_adjust_intrinsics; K and dist of
        set_cameras are not used).  intrinsics [C][9]: fx, fy, cx, cy, k1, k2, p1, p2, k3 per camera, camera 0 included, the
        start; refine: an int mask for all cameras or one per camera, bit i frees parameter i.  Every other argument as
        rig_bundle_adjust's.  Returns its dict plus intrinsics [C][9], a fixed parameter with the bits it came with, and
        obs_err / obs_weight as the robust call's (loss=None is "none")."""
        return self._rig_bundle_adjust(obs_offset, obs_cam, obs_uv, poses, points, max_iters, ftol, lambda0, loss, loss_scale,
                                       intrinsics, refine)

    def _rig_bundle_adjust(self, obs_offset, obs_cam, obs_uv, poses, points, max_iters, ftol, lambda0, loss, loss_scale,
                           intrinsics=None, refine=None):
        """The one body of rig_bundle_adjust and rig_bundle_adjust_intrinsics: upload, the entry the arguments name, sync, dict"""
        setup = self._rig_setup((obs_offset, obs_cam, obs_uv, poses, points), loss, loss_scale, intrinsics, refine)
        selfcal, robust, _, _, n_obs, (_, _, _, d_poses, d_pts), lens = setup
        hist = torch.empty((int(max_iters), 4), dtype=torch.float64, device=self.device)
        result, = self._zeros((4,))
        per_obs = torch.empty((2, n_obs), dtype=torch.float64, device=self.device) if robust else ()
        self._rig_entry("mocap_rig_bundle_adjust", *setup, (int(max_iters), float(ftol), float(lambda0), _ptr(hist), _ptr(result)), per_obs)
        result = result.cpu().numpy()
        status, iters = int(result[0]), int(result[1])
        if status <= 0:
            what = {-2: "the observation arrays break the layout rules" + (_FEW_OBS if selfcal else "") + " (MOCAP_RIG_E_LAYOUT)",
                    -3: "in the start state a point is not in front of a camera that sees it, or the cost is not finite "
                        "(MOCAP_RIG_E_BEHIND)"}.get(status, f"status {status}")
            raise _abi.MocapError(status, "mocap_rig_bundle_adjust: " + what)
        out = {"poses": d_poses.cpu().numpy(), "points": d_pts.cpu().numpy(), "status": status, "iterations": iters,
               "cost_initial": float(result[2]), "cost": float(result[3]), "history": hist.cpu().numpy()[:iters].copy()}
        if robust:
            out["obs_err"], out["obs_weight"] = (p.copy() for p in per_obs.cpu().numpy())
        if selfcal:
            out["intrinsics"] = lens[0].cpu().numpy()
        return out

    def intrinsics_linearize(self, view_offset, point_offset, obj_xy, img_uv, kd, view_poses, lam):
        """The pieces of one iteration of intrinsics_calibrate at a given state and damping (mocap_intrinsics_linearize): dict
        with cost [n_cams] (1/2 sum r^2), gradient [9 n_cams + 6 n_views] (cameras first), S [n_cams][9][9] (damped reduced
        camera matrix), rhs [n_cams][9], layout [n_cams] (the camera breaks the layout rules: its entries are zero), behind
        [n_cams] (a point is not in front of its view's camera).  Arguments as intrinsics_calibrate."""
        n_cams, n_views, voff, poff, obj, img = board_problem(view_offset, point_offset, obj_xy, img_uv)
        d_obj, d_img, d_kd, d_poses = self._upload(obj, img, np.ascontiguousarray(kd, np.float64).reshape(n_cams, 9),
                                                   np.ascontiguousarray(view_poses, np.float64).reshape(n_views, 12))
        cost, grad, S, rhs = self._zeros((n_cams,), (9 * n_cams + 6 * n_views,), (n_cams, 9, 9), (n_cams, 9))
        status, = self._zeros((n_cams, 2), dtype=torch.int32)
        _abi.check(self.lib.mocap_intrinsics_linearize(self._h, n_cams, voff.ctypes.data_as(_IP), poff.ctypes.data_as(_IP), _ptr(d_obj),
                                                       _ptr(d_img), _ptr(d_kd), _ptr(d_poses), float(lam), _ptr(cost), _ptr(grad), _ptr(S),
                                                       _ptr(rhs), _ptr(status), _stream()))
        self.sync()
        status = status.cpu().numpy()
        return {"cost": cost.cpu().numpy(), "gradient": grad.cpu().numpy(), "S": S.cpu().numpy(), "rhs": rhs.cpu().numpy(),
                "layout": status[:, 0].astype(bool), "behind": status[:, 1].astype(bool)}

    def intrinsics_calibrate(self, view_offset, point_offset, obj_xy, img_uv, image_sizes, start=None, max_iters=50, ftol=1e-12,
                             lambda0=1e-3):
        """Intrinsic calibration of every camera of a rig from planar-board corner lists on the device
        (mocap_intrinsics_calibrate; reference CalculateCameraIntrinsic.py:58, cv2.calibrateCamera, for all cameras at once):
        one upload, ONE call that enqueues every iteration, one sync.
        view_offset int32 [n_cams + 1], point_offset int32 [n_views + 1]: camera c owns views view_offset[c] ..
        view_offset[c + 1] - 1, view v points point_offset[v] .. point_offset[v + 1] - 1; obj_xy [total][2] board coordinates
        (Z = 0), img_uv [total][2] pixels; image_sizes [n_cams][2] (width, height); start: None (the definition's
        initialisation) or (kd [n_cams][9], poses [n_views][12]).
        Returns dict of arrays: kd [n_cams][9] (fx, fy, cx, cy, k1, k2, p1, p2, k3), poses [n_views][12] (R row-major, then
        t), view_rms [n_views], status [n_cams] (MOCAP_RIG_STOP_* > 0, or MOCAP_INTR_E_*: -2 layout, -3 a point behind its
        camera at the start, -4 degenerate views), iterations, cost_initial, cost [n_cams] (1/2 sum r^2), and history: per
        camera [iterations][4] = (cost after the iteration, lambda it was solved with, accepted, |step|).  A failed camera is
        reported by its status, never raised: its kd and poses are the start handed in (NaN when there was none)."""
        n_cams, n_views, voff, poff, obj, img = board_problem(view_offset, point_offset, obj_xy, img_uv)
        d_obj, d_img = self._upload(obj, img)
        size = np.ascontiguousarray(image_sizes, np.int32).reshape(n_cams, 2)
        if (size < 1).any():
            raise ValueError("image sizes must be positive")
        max_iters = int(max_iters)
        dev = self.device
        if start is None:
            d_kd = torch.full((n_cams, 9), float("nan"), dtype=torch.float64, device=dev)
            d_poses = torch.full((n_views, 12), float("nan"), dtype=torch.float64, device=dev)
        else:
            kd = np.ascontiguousarray(start[0], np.float64).reshape(n_cams, 9)
            poses = np.ascontiguousarray(start[1], np.float64).reshape(n_views, 12)
            if not (np.isfinite(kd).all() and np.isfinite(poses).all()):
                raise ValueError("the start must be finite")
            d_kd, d_poses = self._upload(kd, poses)
        rms, result = self._zeros((n_views,), (n_cams, 4))
        hist = torch.empty((n_cams, max_iters, 4), dtype=torch.float64, device=dev)
        _abi.check(self.lib.mocap_intrinsics_calibrate(self._h, n_cams, voff.ctypes.data_as(_IP), poff.ctypes.data_as(_IP), _ptr(d_obj),
                                                       _ptr(d_img), size.ctypes.data_as(_IP), int(start is not None), max_iters,
                                                       float(ftol), float(lambda0), _ptr(d_kd), _ptr(d_poses), _ptr(rms), _ptr(hist),
                                                       _ptr(result), _stream()))
        self.sync()
        result, hist = result.cpu().numpy(), hist.cpu().numpy()
        iters = result[:, 1].astype(np.int64)
        return {"kd": d_kd.cpu().numpy(), "poses": d_poses.cpu().numpy(), "view_rms": rms.cpu().numpy(),
                "status": result[:, 0].astype(np.int64), "iterations": iters, "cost_initial": result[:, 2].copy(),
                "cost": result[:, 3].copy(), "history": [hist[c, :iters[c]].copy() for c in range(n_cams)]}
