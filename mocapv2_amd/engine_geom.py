"""The geometry stage of MocapContext (abi_geom.hip): correspondence and triangulation, marker refinement, batched utilities.
What the reference's callers do around lib.Helpers.find_point_correspondance_and_object_points, for whole batches of time steps."""
import ctypes as C

import numpy as np
import torch

from . import _abi
from ._dev import _ptr, _stream, dense_layout, marker_rows, outputs, records_layout

F64, I32 = torch.float64, torch.int32


class GeomStage:
    def _corr_call(self, lay, T, Cn, P, cutoff, max_groups, out):
        out = outputs({"xyz": ((T, P, 3), F64, None), "err": ((T, P), F64, None), "grp": ((T, P, Cn, 2), F64, None),
                       "root": ((T, P), I32, None), "order": ((T, P), I32, None), "n": ((T,), I32, None)}, self.device, out)
        _abi.check(self.lib.mocap_correspond(self._h, *lay, T, Cn, P, cutoff, max_groups, _ptr(out["xyz"]), _ptr(out["err"]),
                                             _ptr(out["grp"]), _ptr(out["root"]), _ptr(out["order"]), _ptr(out["n"]), _stream()))
        return out

    def correspond(self, pts, counts, cutoff=10.0, max_groups=4096, out=None):
        """pts [T, C, P, 2] (int32 or float64), counts [T, C] int32, both on the GPU -> dict of device tensors."""
        *lay, T, Cn, P = dense_layout(pts, counts)
        return self._corr_call(lay, T, Cn, P, cutoff, max_groups, out)

    def correspond_records(self, records, T, Cn, t0=0, stride_t=None, stride_c=None, P=None, cutoff=10.0, max_groups=4096,
                           out=None, points=None):
        """Correspondence + triangulation straight from centroid records (int32 [..., 2 + 2*max_blobs]) laid out so
        that the record of (time step t0 + t, camera c) sits stride_t*t + stride_c*c records after records[t0 * ...].
        Default layout: records [T_total, C, rec] (time-major).  P limits the points read per camera.
        points: float64 [images, rows >= P, 2] on the GPU, one block per record in the records' order (refine_centroids' xy):
        the points are read from there, the counts still from the records."""
        *lay, P = records_layout(records, Cn, t0, stride_t, stride_c, P, points)
        return self._corr_call(lay, T, Cn, P, cutoff, max_groups, out)

    def _vis_out(self, T, Q, Cn, out=None):
        return outputs({"xyz": ((T, Q, 3), F64, None), "err": ((T, Q), F64, None), "idx": ((T, Q, Cn), I32, None),
                        "views": ((T, Q), I32, None),  # the uint32 masks' bits (bit 31 = the sign)
                        "n": ((T,), I32, None)}, self.device, out)

    def _vis_call(self, lay, T, Cn, P, distorted, cutoff, gate, min_views, max_err, max_passes, max_hyp, Q, out):
        Q = Cn * P // 2 if Q is None else int(Q)  # every marker claims at least two points: these rows can never run out
        out = self._vis_out(T, Q, Cn, out)
        _abi.check(self.lib.mocap_correspond_visible(self._h, *lay, T, Cn, P, int(bool(distorted)), float(cutoff), float(gate),
                                                     int(min_views), float(max_err), int(max_passes), int(max_hyp), Q,
                                                     _ptr(out["xyz"]), _ptr(out["err"]), _ptr(out["idx"]), _ptr(out["views"]),
                                                     _ptr(out["n"]), _stream()))
        return out

    def correspond_visible(self, pts, counts, distorted=False, cutoff=10.0, gate=10.0, min_views=2, max_err=25.0, max_passes=3,
                           max_hyp=8192, Q=None, out=None):
        """Markers that only some cameras see, from any camera pair (mocap_correspond_visible; the definition is DESIGN.md
        section 2).  pts [T, C, P, 2] (int32 or float64), counts [T, C] int32, both on the GPU; needs set_cameras only.
        distorted: the points are pixels of the distorted images (False: of undistorted ones, as blob_centroids delivers).
        Returns a dict of device tensors: n [T] (markers per time step, or MOCAP_CORR_E_* < 0), xyz [T, Q, 3], err [T, Q],
        idx [T, Q, C] (the member point of each camera, -1 = none), views [T, Q] (bit c = camera c is a member; int32 holding
        the uint32's bits).  Only rows below n[t] are results: the rest is unspecified and must not be read.  Q defaults to
        C * P // 2, which the markers of a time step cannot exceed."""
        *lay, T, Cn, P = dense_layout(pts, counts)
        return self._vis_call(lay, T, Cn, P, distorted, cutoff, gate, min_views, max_err, max_passes, max_hyp, Q, out)

    def correspond_visible_records(self, records, T, Cn, t0=0, stride_t=None, stride_c=None, P=None, distorted=False, cutoff=10.0,
                                   gate=10.0, min_views=2, max_err=25.0, max_passes=3, max_hyp=8192, Q=None, out=None, points=None):
        """correspond_visible straight from centroid records, laid out and read as correspond_records reads them (`points`
        included)."""
        *lay, P = records_layout(records, Cn, t0, stride_t, stride_c, P, points)
        return self._vis_call(lay, T, Cn, P, distorted, cutoff, gate, min_views, max_err, max_passes, max_hyp, Q, out)

    def _refine_call(self, xyz, n, views, Cn, lay, P, idx, grp, distorted, max_iters, ftol, lambda0, max_res2, min_views, max_drop, out):
        """lay: a layout tuple of the indexed form (its counts are not read), None for the grouped form"""
        T, Q = marker_rows(xyz, n)
        if int(max_drop) > 0 and max_res2 is None:
            raise ValueError("max_drop > 0 asks for pruning: max_res2 (px^2) has no default, it is the capture's noise")
        for t, shape in ((views, (T, Q)), (idx, (T, Q, Cn))):
            assert t is None or (t.is_cuda and t.is_contiguous() and t.dtype == I32 and t.shape == shape), (t.shape, shape)
        spec = {"xyz": ((T, Q, 3), F64, 0), "err": ((T, Q), F64, 0), "res2": ((T, Q, Cn), F64, 0), "cov": ((T, Q, 6), F64, 0)}
        spec.update({k: ((T, Q), I32, 0) for k in ("views", "dropped", "iters", "status")})  # views, dropped: uint32 masks' bits
        out = outputs(spec, self.device, out)
        pts_ptr, pt_st, pt_sc, f64 = (lay[0], lay[1], lay[2], lay[6]) if lay is not None else (None, 0, 0, 1)
        _abi.check(self.lib.mocap_refine_points(self._h, _ptr(xyz), _ptr(n), _ptr(views), T, Q, Cn, pts_ptr, pt_st, pt_sc, f64, int(P),
                                                _ptr(idx), _ptr(grp), int(bool(distorted)), int(max_iters), float(ftol), float(lambda0),
                                                0.0 if max_res2 is None else float(max_res2), int(min_views), int(max_drop),
                                                _ptr(out["xyz"]), _ptr(out["err"]), _ptr(out["res2"]), _ptr(out["cov"]), _ptr(out["views"]),
                                                _ptr(out["dropped"]), _ptr(out["iters"]), _ptr(out["status"]), _stream()))
        return out

    def refine_points(self, xyz, n, views=None, pts=None, idx=None, grp=None, distorted=False, max_iters=10, ftol=1e-9, lambda0=1e-3,
                      max_res2=None, min_views=2, max_drop=0, out=None):
        """Triangulated markers moved to the minimum of their reprojection error, with the covariance there (mocap_refine_points;
        the definition is DESIGN.md section 2).  xyz [T, Q, 3] float64 and n [T] int32 on the GPU: the points to start from and
        the rows of every step (a count <= 0: none), as the correspondence calls deliver them.  The observations come
          indexed:  pts [T, C, P, 2] (int32 or float64), idx [T, Q, C] int32, views [T, Q] int32 (bit c = camera c is a member)
                    -- correspond_visible's inputs and outputs as they are; or
          grouped:  grp [T, Q, C, 2] float64 -- correspond's grp as it is; views may be None (every camera is a member).
        distorted: the observations are raw-frame pixels and the residual goes through the cameras' lenses (False: ideal
        pixels, an exact pinhole).  max_drop > 0 turns pruning on and needs max_res2 (px^2, no default: it is the capture's
        noise): after a loop, the member with the largest squared residual is dropped when that exceeds max_res2 and more than
        min_views members are left.  Returns a dict of device tensors: xyz [T, Q, 3] (out["xyz"] may be the input), err [T, Q]
        (px^2), res2 [T, Q, C] (-1 = no member), cov [T, Q, 6] (upper triangle 00, 01, 02, 11, 12, 22; world units^2 per px^2),
        views, dropped, iters, status [T, Q] int32 (status: RIG_STOP_* 1..4, 0 = no row, MOCAP_REFINE_E_* < 0 = not refined:
        xyz and views are the input's, the rest of the row must not be read)."""
        if (pts is None) == (grp is None):
            raise ValueError("refine_points: either pts with idx and views (indexed form) or grp (grouped form)")
        if grp is not None:
            assert grp.is_cuda and grp.is_contiguous() and grp.dtype == F64 and grp.dim() == 4 and grp.shape[3] == 2, grp.shape
            assert tuple(grp.shape[:2]) == tuple(xyz.shape[:2]), (grp.shape, xyz.shape)
            return self._refine_call(xyz, n, views, int(grp.shape[2]), None, 0, None, grp, distorted, max_iters, ftol, lambda0, max_res2,
                                     min_views, max_drop, out)
        if idx is None or views is None:
            raise ValueError("refine_points: the indexed form needs idx and views")
        *lay, T, Cn, P = dense_layout(pts)
        assert T == xyz.shape[0], (pts.shape, xyz.shape)
        return self._refine_call(xyz, n, views, Cn, lay, P, idx, None, distorted, max_iters, ftol, lambda0, max_res2, min_views, max_drop, out)

    def refine_points_records(self, xyz, n, views, idx, records, Cn, t0=0, stride_t=None, stride_c=None, P=None, points=None,
                              distorted=False, max_iters=10, ftol=1e-9, lambda0=1e-3, max_res2=None, min_views=2, max_drop=0, out=None):
        """refine_points' indexed form straight from centroid records, laid out and read as correspond_visible_records reads
        them (`points` included)."""
        *lay, P = records_layout(records, Cn, t0, stride_t, stride_c, P, points)
        return self._refine_call(xyz, n, views, Cn, lay, P, idx, None, distorted, max_iters, ftol, lambda0, max_res2, min_views, max_drop, out)

    def epipolar_scores(self, roots, cand, f_index=0, with_lines=False):
        """The scoring step of the correspondence search for one camera pair (reference lib/Helpers.py:205-220): roots [R, 2]
        camera-0 points, cand [N, 2] points of camera f_index + 1 (host arrays, integer or float) -> distances [R, N] float64
        (and the float32 lines [R, 3]) as host arrays.  Requires set_fundamentals."""
        roots, cand = np.asarray(roots), np.asarray(cand)
        f64 = not (roots.dtype.kind in "iu" and cand.dtype.kind in "iu")
        dt = np.float64 if f64 else np.int32
        d_r = torch.from_numpy(np.ascontiguousarray(roots, dt).reshape(-1, 2)).to(self.device)
        d_c = torch.from_numpy(np.ascontiguousarray(cand, dt).reshape(-1, 2)).to(self.device)
        dist = torch.empty((d_r.shape[0], d_c.shape[0]), dtype=F64, device=self.device)
        lines = torch.empty((d_r.shape[0], 3), dtype=torch.float32, device=self.device) if with_lines else None
        _abi.check(self.lib.mocap_epipolar_scores(self._h, _ptr(d_r), d_r.shape[0], _ptr(d_c), d_c.shape[0], int(f64), int(f_index),
                                                  _ptr(dist), _ptr(lines), _stream()))
        return (dist.cpu().numpy(), lines.cpu().numpy()) if with_lines else dist.cpu().numpy()

    def _upload_views(self, pts, valid):
        pts = np.ascontiguousarray(pts, np.float64)
        N, Cn = pts.shape[:2]
        d_val = torch.from_numpy(np.ascontiguousarray(valid, np.uint8).reshape(N, Cn)).to(self.device)
        return N, Cn, torch.from_numpy(pts).to(self.device), d_val, torch.zeros((N,), dtype=I32, device=self.device)

    def triangulate_batch(self, pts, valid, compact_k=True):
        """pts [N, C, 2] float64 host array, valid [N, C] -> (xyz [N,3], ok [N]) host arrays."""
        N, Cn, d_pts, d_val, ok = self._upload_views(pts, valid)
        xyz = torch.zeros((N, 3), dtype=F64, device=self.device)
        _abi.check(self.lib.mocap_triangulate_batch(self._h, _ptr(d_pts), _ptr(d_val), N, Cn, int(compact_k), _ptr(xyz),
                                                    _ptr(ok), _stream()))
        return xyz.cpu().numpy(), ok.cpu().numpy()

    def reproject_batch(self, pts, valid, xyz, compact_k=True):
        N, Cn, d_pts, d_val, ok = self._upload_views(pts, valid)
        d_xyz = torch.from_numpy(np.ascontiguousarray(xyz, np.float64).reshape(N, 3)).to(self.device)
        mse = torch.zeros((N,), dtype=F64, device=self.device)
        _abi.check(self.lib.mocap_reproject_batch(self._h, _ptr(d_pts), _ptr(d_val), _ptr(d_xyz), N, Cn, int(compact_k),
                                                  _ptr(mse), _ptr(ok), _stream()))
        return mse.cpu().numpy(), ok.cpu().numpy()

    def ba_problem(self, pts, valid=None):
        """Bundle-adjustment residuals with the image points resident on the GPU (see BAProblem)."""
        return BAProblem(self, pts, valid)


class BAProblem:
    """The residual function of the reference's bundle adjustment (lib/Helpers.py:161-167) with everything that does not
    change between evaluations kept on the GPU: image points [N, C, 2] and validity [N, C] are uploaded once, the
    intrinsics live in the context's camera table (set_cameras), and an evaluation is one C-ABI call (mocap_ba_residuals:
    one launch -- rotvec -> R, triangulation, reprojection, float32 cast on the device -- and one stream wait)."""

    def __init__(self, ctx, pts, valid=None):
        pts = np.ascontiguousarray(pts, np.float64)
        assert pts.ndim == 3 and pts.shape[2] == 2, pts.shape
        self.ctx, (self.N, self.C) = ctx, pts.shape[:2]
        valid = np.ones((self.N, self.C), np.uint8) if valid is None else np.ascontiguousarray(valid, np.uint8).reshape(self.N, self.C)
        self.d_pts = torch.from_numpy(pts).to(ctx.device)
        self.d_valid = torch.from_numpy(valid).to(ctx.device)
        self._res = np.empty((1, self.N), np.float32)
        self._cnt = np.empty(1, np.int32)

    def residuals(self, params):
        """params: one parameter vector [6 (C - 1)] -> float32 residual vector, or a batch [B, 6 (C - 1)] -> list of
        residual vectors (a vector is shorter than N only when groups hold [None, None] entries, as in the reference)."""
        p = np.ascontiguousarray(params, np.float64)
        single = p.ndim == 1
        p = p.reshape(-1, 6 * (self.C - 1))
        B = p.shape[0]
        if self._res.shape[0] < B:
            self._res = np.empty((B, self.N), np.float32)
            self._cnt = np.empty(B, np.int32)
        ctx = self.ctx
        _abi.check(ctx.lib.mocap_ba_residuals(ctx._h, p.ctypes.data_as(C.POINTER(C.c_double)), B, _ptr(self.d_pts), _ptr(self.d_valid),
                                              self.N, self.C, self._res.ctypes.data_as(C.POINTER(C.c_float)),
                                              self._cnt.ctypes.data_as(C.POINTER(C.c_int)), _stream()))
        if single:
            return self._res[0, :self._cnt[0]].copy()
        return [self._res[b, :self._cnt[b]].copy() for b in range(B)]
