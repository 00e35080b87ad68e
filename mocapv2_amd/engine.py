"""Host side of the hot path: a thin object over the C-ABI context.

PyTorch is used only as the device allocator / stream provider (tensors are passed to the library as raw
pointers); no torch operator touches the data.  Mirrors what the reference's callers do around
lib.ImageOperations._find_dot and lib.Helpers.find_point_correspondance_and_object_points
(reference RealtimeTracking_FLIR.py:95-143,157-209) for whole batches of frames.
"""
import ctypes as C
import threading

import numpy as np
import torch

from . import _abi

MAX_BLOBS = 128       # centroid record capacity per camera image
# Fixed point of cv2.cvtColor(., COLOR_BGR2GRAY) on 8-bit images in the camera loop (RealtimeTracking_FLIR.py:104).
# The reference pins no OpenCV version (README.md:65), so `pip install opencv-python` gives a current 4.x, whose
# RGB2Gray<uchar> works with gray_shift = 15 (RY15 = 9798, GY15 = 19235, BY15 = 3735, + 2^14, >> 15;
# modules/imgproc/src/color.simd_helpers.hpp); OpenCV 2.x / 3.x used the 14-bit set (4899, 9617, 1868).  Both are
# implemented and tested; the default follows the version the reference's users get today.  oracle/check_against_cv2.py
# settles it wherever cv2 can be imported (it cannot in the build container).
GRAY_SHIFT = 15
REC_INTS = 2 + 2 * MAX_BLOBS  # int32 record: count, pad, xy[MAX_BLOBS][2]
RIG_LOSSES = {"none": 0, "cauchy": 1}  # MOCAP_RIG_LOSS_*
SUBPIX_COORDS = {"raw": 0, "ideal": 1}  # mocap_refine_centroids' coords
SUBPIX_EMPTY, SUBPIX_EDGE, SUBPIX_NEIGHBOUR, SUBPIX_MOVING, SUBPIX_CUT = 1, 2, 4, 8, 16  # MOCAP_SUBPIX_*
SUBPIX_FALLBACK = SUBPIX_EMPTY | SUBPIX_EDGE | SUBPIX_NEIGHBOUR | SUBPIX_MOVING  # the point holds its integer centroid

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


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dbl(a, n):
    a = np.ascontiguousarray(a, np.float64).reshape(-1)
    assert a.size == n, (a.size, n)
    return a, a.ctypes.data_as(C.POINTER(C.c_double))


class MocapContext:
    """One GPU, one image geometry.  Not a singleton: one per camera thread or per process is fine."""

    def __init__(self, width, height, n_slots=1, device=0):
        self.lib = _abi.load()
        if not torch.cuda.is_available():
            raise RuntimeError("mocapv2_amd needs a ROCm GPU (torch.cuda.is_available() is False); no CPU fallback")
        self.device = torch.device("cuda", device)
        self.width, self.height, self.n_slots = int(width), int(height), int(n_slots)
        h = C.c_void_p()
        _abi.check(self.lib.mocap_ctx_create(device, self.width, self.height, self.n_slots, C.byref(h)))
        self._h = h
        self._cam_key = None
        self._f_key = None
        self._und_key = {}
        self._warned_dense = set()  # causes set_undistort has warned about
        self.identity = {}

    def close(self):
        if getattr(self, "_h", None):
            self.lib.mocap_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- set-up -------------------------------------------------------------------------------------------
    def set_blob_params(self, thresh=255 * 0.85, min_area=500.0, min_circ=0.5, ksize=5, median=5):
        p = _abi.BlobParams(ksize, median, thresh, min_area, min_circ)
        _abi.check(self.lib.mocap_set_blob_params(self._h, C.byref(p)))

    def set_tuning(self, name, value):
        """One performance switch of this context (mocap_set_tuning; names in include/mocap_hip.h).  None changes a result."""
        _abi.check(self.lib.mocap_set_tuning(self._h, name.encode(), int(value)))

    def set_undistort(self, slot, K, dist, warn_dense=True):
        K, Kp = _dbl(K, 9)
        d, dp = _dbl(dist, 5)
        key = K.tobytes() + d.tobytes()
        if self._und_key.get(slot) == key:
            return self.identity[slot]
        ident = C.c_int(0)
        _abi.check(self.lib.mocap_set_undistort(self._h, slot, Kp, dp, C.byref(ident)))
        self._und_key[slot] = key
        self.identity[slot] = bool(ident.value)
        if warn_dense:
            # Only a table that cannot take the sparse road is worth a warning: sparse_path is also False when a tuning switch
            # (general_filter, skip_dark=0) sends everything down the dense kernel on purpose.  Once per cause and context.
            info = self.undistort_info(slot)
            causes = tuple(k for k in ("compact_table", "early_out_provable") if not info["identity"] and not info[k])
            if causes and causes not in self._warned_dense:
                self._warned_dense.add(causes)
                import warnings
                warnings.warn(f"mocapv2_amd: undistort slot {slot}: the lens table is outside the bounds of the sparse path "
                              f"({', '.join(c + ' = False' for c in causes)}; {info}); its images are filtered by the dense kernel: "
                              "same results, several times slower on dark scenes", RuntimeWarning, stacklevel=2)
        return self.identity[slot]

    def undistort_info(self, slot=0):
        """What set_undistort found out about the slot's table (mocap_undistort_info): dict with identity, compact_table,
        early_out_provable, max_source_weight, sparse_path.  sparse_path False = the slot's images take the dense row
        pipeline (same results, several times slower on a dark scene)."""
        info = _abi.UndistortInfo()
        _abi.check(self.lib.mocap_undistort_info(self._h, int(slot), C.byref(info)))
        return {k: (bool(getattr(info, k)) if k != "max_source_weight" else int(info.max_source_weight)) for k, _ in info._fields_}

    def set_cameras(self, K, dist, R, t):
        n = len(K)
        K, Kp = _dbl(K, 9 * n)
        d, dp = _dbl(dist, 5 * n)
        R, Rp = _dbl(R, 9 * n)
        t, tp = _dbl(t, 3 * n)
        key = K.tobytes() + d.tobytes() + R.tobytes() + t.tobytes()
        if key != self._cam_key:
            _abi.check(self.lib.mocap_set_cameras(self._h, n, Kp, dp, Rp, tp))
            self._cam_key = key
        self.n_cam = n

    def set_fundamentals(self, F):
        F = np.ascontiguousarray(F, np.float64).reshape(-1, 9)
        key = F.tobytes()
        if key != self._f_key:
            _abi.check(self.lib.mocap_set_fundamentals(self._h, len(F), F.ctypes.data_as(C.POINTER(C.c_double))))
            self._f_key = key

    def sync(self):
        _abi.check(self.lib.mocap_sync(self._h, _stream()))

    # ---- blob stage ------------------------------------------------------------------------------------------
    def _frames(self, frames):
        assert frames.is_cuda and frames.dtype == torch.uint8
        assert frames.shape[-2:] == (self.height, self.width), (frames.shape, self.height, self.width)
        assert frames.stride(-1) == 1
        n = int(np.prod(frames.shape[:-2])) if frames.dim() > 2 else 1
        pitch = frames.stride(-2)
        flat = frames.reshape(n, self.height, self.width) if frames.is_contiguous() else frames
        assert flat.dim() == 3
        stride = flat.stride(0) if n > 1 else pitch * self.height
        return flat, n, stride, pitch

    def blob_centroids(self, frames, cam_mod=1, slot_base=0, max_blobs=MAX_BLOBS, records=None, bayer_pattern=None,
                       gray_shift=GRAY_SHIFT, gray=None):
        """_find_dot over uint8 frames [..., H, W] resident on the GPU (image n uses undistort slot
        slot_base + n % cam_mod).  Results land in centroid records, int32 [n, 2 + 2*max_blobs]:
        record[0] = number of image points, record[2:] = (cx, cy) pairs in the reference's contour order.
        Returns the records tensor (use record_views for xy / count views).
        bayer_pattern 0..3 (BG, GB, RG, GR): the frames are raw sensor frames and the camera loop's cvtColor pair
        (RealtimeTracking_FLIR.py:103-104) comes first.  gray=None: no gray frame is allocated or written; the library
        forms the gray values from the Bayer frames where it needs them, or, on geometries that path does not cover
        (width not a multiple of 16, height not of 8, unaligned frames, the dense path), converts into a scratch buffer of
        the context's own.  A tensor passed as `gray` (same shape as frames) is filled with the gray frames.  The records
        are the same either way."""
        flat, n, stride, pitch = self._frames(frames)
        rec_ints = 2 + 2 * max_blobs
        if records is None:
            records = torch.empty((n, rec_ints), dtype=torch.int32, device=self.device)
        assert records.is_contiguous() and records.shape == (n, rec_ints) and records.dtype == torch.int32
        xy_ptr = C.c_void_p(records.data_ptr() + 8)
        if bayer_pattern is None:
            _abi.check(self.lib.mocap_blob_centroids(self._h, _ptr(flat), n, cam_mod, slot_base, stride, pitch, xy_ptr, rec_ints,
                                                     _ptr(records), rec_ints, max_blobs, _stream()))
            return records
        assert gray is None or (gray.dtype == torch.uint8 and gray.is_cuda and gray.reshape(flat.shape).stride() == flat.stride())
        _abi.check(self.lib.mocap_blob_centroids_bayer(self._h, _ptr(flat), _ptr(gray), n, cam_mod, slot_base, stride, pitch,
                                                       bayer_pattern, gray_shift, xy_ptr, rec_ints, _ptr(records), rec_ints,
                                                       max_blobs, _stream()))
        return records

    @staticmethod
    def record_views(records):
        """(xy [n, max_blobs, 2], count [n]) views of a records tensor"""
        n, rec_ints = records.shape
        return records[:, 2:].reshape(n, (rec_ints - 2) // 2, 2), records[:, 0]

    def refine_centroids(self, frames, records, cam_mod=1, slot_base=0, max_blobs=None, *, radius, floor, iters=3, coords="ideal",
                         bayer_pattern=None, gray_shift=GRAY_SHIFT, out=None):
        """Sub-pixel centroids (mocap_refine_centroids; the definition is DESIGN.md section 2): for every integer centroid of
        `records` (blob_centroids' records of the same frames, read in place) the intensity-weighted centroid, weights
        max(0, p - floor), over a window of `radius` pixels (1..31) that follows the blob for at most `iters` windows (1..8).
        radius and floor have no defaults: they depend on the markers' size in the image and on the background.
        coords: "ideal" -- pixels of the undistorted image, a drop-in for the integer centroids (correspond_records and
        correspond_visible_records take them as `points`); "raw" -- pixels of the distorted frame, what
        correspond_visible(distorted=True) takes.  bayer_pattern: the frames are raw Bayer frames (no gray frame is written).
        max_blobs (default: the records' capacity, at most 256): points refined per image.
        Returns {"xy": float64 [n, max_blobs, 2], "weight": int32 [n, max_blobs] (the last window's sum of weights), "flags":
        int32 [n, max_blobs] (SUBPIX_* bits)} as device tensors; weight and flags are views of out["info"].  A point flagged
        EMPTY, EDGE, NEIGHBOUR or MOVING holds its integer centroid in the coordinates asked for.  Rows at and beyond an image's
        count are not written (a fresh `out` holds zeros there)."""
        flat, n, stride, pitch = self._frames(frames)
        rec_ints = records.shape[-1]
        assert records.is_cuda and records.is_contiguous() and records.dtype == torch.int32 and records.numel() == n * rec_ints
        max_blobs = min(256, (rec_ints - 2) // 2) if max_blobs is None else int(max_blobs)
        if coords not in SUBPIX_COORDS:
            raise ValueError(f"coords {coords!r}: one of {sorted(SUBPIX_COORDS)}")
        if out is None:
            out = {"xy": torch.zeros((n, max_blobs, 2), dtype=torch.float64, device=self.device),
                   "info": torch.zeros((n, max_blobs, 2), dtype=torch.int32, device=self.device)}
        xy, info = out["xy"], out["info"]
        assert xy.is_contiguous() and xy.dtype == torch.float64 and xy.shape[0] == n and xy.shape[1] >= max_blobs and xy.shape[2] == 2
        assert info.is_contiguous() and info.dtype == torch.int32 and info.shape[0] == n and info.shape[1] >= max_blobs and info.shape[2] == 2
        _abi.check(self.lib.mocap_refine_centroids(self._h, _ptr(flat), n, cam_mod, slot_base, stride, pitch,
                                                   -1 if bayer_pattern is None else int(bayer_pattern), int(gray_shift),
                                                   C.c_void_p(records.data_ptr() + 8), rec_ints, _ptr(records), rec_ints, max_blobs,
                                                   int(radius), int(floor), int(iters), SUBPIX_COORDS[coords], _ptr(xy),
                                                   2 * xy.shape[1], _ptr(info), 2 * info.shape[1], _stream()))
        out["weight"], out["flags"] = info[:, :, 0], info[:, :, 1]
        return out

    def filter_mask(self, frames, cam_mod=1, slot_base=0, mask=None):
        flat, n, stride, pitch = self._frames(frames)
        wpr = (self.width + 31) // 32
        if mask is None:
            mask = torch.zeros((n, self.height, wpr), dtype=torch.int32, device=self.device)
        _abi.check(self.lib.mocap_filter_mask(self._h, _ptr(flat), n, cam_mod, slot_base, stride, pitch, _ptr(mask), _stream()))
        return mask

    def contours_from_mask(self, mask, max_blobs=MAX_BLOBS, debug_cap=0, xy=None):
        """xy: optional int32 [n, rows >= max_blobs, 2] device tensor to write into (at most max_blobs rows per image are written)."""
        n = mask.shape[0]
        if xy is None:
            xy = torch.empty((n, max_blobs, 2), dtype=torch.int32, device=self.device)
        assert xy.is_cuda and xy.is_contiguous() and xy.dtype == torch.int32 and xy.dim() == 3
        assert xy.shape[0] == n and xy.shape[1] >= max_blobs and xy.shape[2] == 2, (xy.shape, n, max_blobs)
        cnt = torch.empty((n,), dtype=torch.int32, device=self.device)
        dbg = dbg_n = None
        if debug_cap:
            dbg = torch.zeros((n, debug_cap, C.sizeof(_abi.Contour)), dtype=torch.uint8, device=self.device)
            dbg_n = torch.zeros((n,), dtype=torch.int32, device=self.device)
        _abi.check(self.lib.mocap_contours_from_mask(self._h, _ptr(mask), n, _ptr(xy), 2 * xy.shape[1], _ptr(cnt), 1, max_blobs,
                                                     _ptr(dbg), _ptr(dbg_n), debug_cap, _stream()))
        if not debug_cap:
            return xy, cnt
        raw = dbg.cpu().numpy()
        counts = dbg_n.cpu().numpy()
        recs = []
        for i in range(n):
            arr = (_abi.Contour * debug_cap).from_buffer_copy(raw[i].tobytes())
            recs.append([{k: getattr(arr[j], k) for k, _ in _abi.Contour._fields_} for j in range(min(counts[i], debug_cap))])
        return xy, cnt, recs

    def image_filter(self, img, order=0, slot=-1):
        """image_filter_gpu (order 0) / image_filter_cpu (order 1) on one device image -> {0,255} device image."""
        assert img.is_cuda and img.dtype == torch.uint8 and img.shape == (self.height, self.width)
        out = torch.empty_like(img, memory_format=torch.contiguous_format)
        _abi.check(self.lib.mocap_image_filter_u8(self._h, _ptr(img), _ptr(out), img.stride(0), out.stride(0), order, slot,
                                                  _stream()))
        return out

    def undistort(self, img, slot=0):
        assert img.is_cuda and img.dtype == torch.uint8 and img.shape == (self.height, self.width)
        out = torch.empty_like(img, memory_format=torch.contiguous_format)
        _abi.check(self.lib.mocap_undistort_u8(self._h, slot, _ptr(img), _ptr(out), img.stride(0), out.stride(0), _stream()))
        return out

    def box_blur(self, img, ksize=5):
        assert img.is_cuda and img.dtype == torch.uint8 and img.dim() == 2
        out = torch.empty_like(img, memory_format=torch.contiguous_format)
        _abi.check(self.lib.mocap_box_blur_u8(self._h, _ptr(img), _ptr(out), img.shape[0], img.shape[1], img.stride(0),
                                              out.stride(0), ksize, _stream()))
        return out

    def demosaic(self, bayer):
        assert bayer.is_cuda and bayer.dtype == torch.uint8 and bayer.dim() == 2
        out = torch.empty(bayer.shape + (3,), dtype=torch.uint8, device=self.device)
        _abi.check(self.lib.mocap_demosaic_u8(self._h, _ptr(bayer), _ptr(out), bayer.shape[0], bayer.shape[1],
                                              bayer.stride(0), _stream()))
        return out

    def bayer_gray(self, bayer, pattern=3, gray_shift=GRAY_SHIFT, out=None):
        """Raw Bayer frames uint8 [H, W] or [n, H, W] on the GPU -> gray frames of the same shape:
        cv2.cvtColor(cv2.cvtColor(raw, COLOR_BAYER_GR2BGR), COLOR_BGR2GRAY) of the reference's camera loop
        (RealtimeTracking_FLIR.py:103-104) in one pass.  pattern 0..3 = BG, GB, RG, GR."""
        assert bayer.is_cuda and bayer.dtype == torch.uint8 and bayer.dim() in (2, 3) and bayer.stride(-1) == 1
        b3 = bayer if bayer.dim() == 3 else bayer.unsqueeze(0)
        n, H, W = b3.shape
        out = torch.empty((n, H, W), dtype=torch.uint8, device=bayer.device) if out is None else out.reshape(n, H, W)
        assert out.is_contiguous() and out.dtype == torch.uint8
        _abi.check(self.lib.mocap_bayer_gray_u8(self._h, _ptr(b3), _ptr(out), n, H, W, b3.stride(1), W,
                                                b3.stride(0) if n > 1 else H * b3.stride(1), H * W, pattern, gray_shift,
                                                _stream()))
        return out if bayer.dim() == 3 else out[0]

    # ---- geometry stage ----------------------------------------------------------------------------------------
    def _corr_out(self, T, P, Cn):
        dev = self.device
        return {"xyz": torch.empty((T, P, 3), dtype=torch.float64, device=dev),
                "err": torch.empty((T, P), dtype=torch.float64, device=dev),
                "grp": torch.empty((T, P, Cn, 2), dtype=torch.float64, device=dev),
                "root": torch.empty((T, P), dtype=torch.int32, device=dev),
                "order": torch.empty((T, P), dtype=torch.int32, device=dev),
                "n": torch.empty((T,), dtype=torch.int32, device=dev)}

    def correspond(self, pts, counts, cutoff=10.0, max_groups=4096, out=None):
        """pts [T, C, P, 2] (int32 or float64), counts [T, C] int32, both on the GPU -> dict of device tensors."""
        assert pts.is_cuda and pts.is_contiguous() and counts.is_contiguous() and counts.dtype == torch.int32
        T, Cn, P, _ = pts.shape
        f64 = pts.dtype == torch.float64
        assert f64 or pts.dtype == torch.int32
        out = out or self._corr_out(T, P, Cn)
        _abi.check(self.lib.mocap_correspond(self._h, _ptr(pts), Cn * P * 2, P * 2, _ptr(counts), Cn, 1, int(f64), T, Cn, P,
                                             cutoff, max_groups, _ptr(out["xyz"]), _ptr(out["err"]), _ptr(out["grp"]),
                                             _ptr(out["root"]), _ptr(out["order"]), _ptr(out["n"]), _stream()))
        return out

    @staticmethod
    def _record_points(points, records, P, stride_t, stride_c, t0):
        """(pointer, stride_t, stride_c) of float64 points [images, rows >= P, 2] that stand beside the records, image for image
        (refine_centroids' xy), read with pts_f64 = 1 through the records' own layout"""
        assert points.is_cuda and points.is_contiguous() and points.dtype == torch.float64 and points.dim() == 3, points.shape
        assert points.shape[0] == records.numel() // records.shape[-1] and points.shape[1] >= P and points.shape[2] == 2, (points.shape, P)
        row = 2 * points.shape[1]
        return C.c_void_p(points.data_ptr() + 8 * row * stride_t * t0), row * stride_t, row * stride_c

    def correspond_records(self, records, T, Cn, t0=0, stride_t=None, stride_c=None, P=None, cutoff=10.0, max_groups=4096,
                           out=None, points=None):
        """Correspondence + triangulation straight from centroid records (int32 [..., 2 + 2*max_blobs]) laid out so
        that the record of (time step t0 + t, camera c) sits stride_t*t + stride_c*c records after records[t0 * ...].
        Default layout: records [T_total, C, rec] (time-major).  P limits the points read per camera.
        points: float64 [images, rows >= P, 2] on the GPU, one block per record in the records' order (refine_centroids' xy):
        the points are read from there, the counts still from the records."""
        rec_ints = records.shape[-1]
        flat = records.reshape(-1, rec_ints)
        stride_t = Cn if stride_t is None else stride_t
        stride_c = 1 if stride_c is None else stride_c
        P = P or min(255, (rec_ints - 2) // 2)
        out = out or self._corr_out(T, P, Cn)
        base = flat.data_ptr() + 4 * rec_ints * stride_t * t0
        pts = (C.c_void_p(base + 8), rec_ints * stride_t, rec_ints * stride_c) if points is None else \
            self._record_points(points, records, P, stride_t, stride_c, t0)
        _abi.check(self.lib.mocap_correspond(self._h, *pts,
                                             C.c_void_p(base), rec_ints * stride_t, rec_ints * stride_c, int(points is not None), T, Cn, P,
                                             cutoff, max_groups, _ptr(out["xyz"]), _ptr(out["err"]), _ptr(out["grp"]),
                                             _ptr(out["root"]), _ptr(out["order"]), _ptr(out["n"]), _stream()))
        return out

    def _vis_out(self, T, Q, Cn):
        dev = self.device
        return {"xyz": torch.empty((T, Q, 3), dtype=torch.float64, device=dev),
                "err": torch.empty((T, Q), dtype=torch.float64, device=dev),
                "idx": torch.empty((T, Q, Cn), dtype=torch.int32, device=dev),
                "views": torch.empty((T, Q), dtype=torch.int32, device=dev),  # the uint32 masks' bits (bit 31 = the sign)
                "n": torch.empty((T,), dtype=torch.int32, device=dev)}

    def _vis_call(self, pts_ptr, pt_st, pt_sc, cnt_ptr, cnt_st, cnt_sc, f64, T, Cn, P, distorted, cutoff, gate, min_views, max_err,
                  max_passes, max_hyp, Q, out):
        Q = Cn * P // 2 if Q is None else int(Q)  # every marker claims at least two points: these rows can never run out
        out = out or self._vis_out(T, Q, Cn)
        assert out["xyz"].shape == (T, Q, 3) and out["idx"].shape == (T, Q, Cn), (out["xyz"].shape, out["idx"].shape, T, Q, Cn)
        _abi.check(self.lib.mocap_correspond_visible(self._h, pts_ptr, pt_st, pt_sc, cnt_ptr, cnt_st, cnt_sc, int(f64), T, Cn, P,
                                                     int(bool(distorted)), float(cutoff), float(gate), int(min_views), float(max_err),
                                                     int(max_passes), int(max_hyp), Q, _ptr(out["xyz"]), _ptr(out["err"]),
                                                     _ptr(out["idx"]), _ptr(out["views"]), _ptr(out["n"]), _stream()))
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
        assert pts.is_cuda and pts.is_contiguous() and counts.is_contiguous() and counts.dtype == torch.int32
        T, Cn, P, _ = pts.shape
        f64 = pts.dtype == torch.float64
        assert f64 or pts.dtype == torch.int32
        return self._vis_call(_ptr(pts), Cn * P * 2, P * 2, _ptr(counts), Cn, 1, f64, T, Cn, P, distorted, cutoff, gate, min_views,
                              max_err, max_passes, max_hyp, Q, out)

    def correspond_visible_records(self, records, T, Cn, t0=0, stride_t=None, stride_c=None, P=None, distorted=False, cutoff=10.0,
                                   gate=10.0, min_views=2, max_err=25.0, max_passes=3, max_hyp=8192, Q=None, out=None, points=None):
        """correspond_visible straight from centroid records, laid out and read as correspond_records reads them (`points`
        included)."""
        rec_ints = records.shape[-1]
        flat = records.reshape(-1, rec_ints)
        stride_t = Cn if stride_t is None else stride_t
        stride_c = 1 if stride_c is None else stride_c
        P = P or min(255, (rec_ints - 2) // 2)
        base = flat.data_ptr() + 4 * rec_ints * stride_t * t0
        pts = (C.c_void_p(base + 8), rec_ints * stride_t, rec_ints * stride_c) if points is None else \
            self._record_points(points, records, P, stride_t, stride_c, t0)
        return self._vis_call(*pts, C.c_void_p(base), rec_ints * stride_t,
                              rec_ints * stride_c, points is not None, T, Cn, P, distorted, cutoff, gate, min_views, max_err, max_passes,
                              max_hyp, Q, out)

    def _refine_out(self, T, Q, Cn):
        dev = self.device
        out = {"xyz": torch.zeros((T, Q, 3), dtype=torch.float64, device=dev), "err": torch.zeros((T, Q), dtype=torch.float64, device=dev),
               "res2": torch.zeros((T, Q, Cn), dtype=torch.float64, device=dev), "cov": torch.zeros((T, Q, 6), dtype=torch.float64, device=dev)}
        for k in ("views", "dropped", "iters", "status"):  # views, dropped: the uint32 masks' bits (bit 31 = the sign)
            out[k] = torch.zeros((T, Q), dtype=torch.int32, device=dev)
        return out

    def _refine_call(self, xyz, n, views, Cn, pts, P, idx, grp, distorted, max_iters, ftol, lambda0, max_res2, min_views, max_drop, out):
        assert xyz.is_cuda and xyz.is_contiguous() and xyz.dtype == torch.float64 and xyz.dim() == 3 and xyz.shape[2] == 3, xyz.shape
        assert n.is_cuda and n.is_contiguous() and n.dtype == torch.int32
        T, Q = int(xyz.shape[0]), int(xyz.shape[1])
        assert n.numel() >= T, (n.shape, T)
        if int(max_drop) > 0 and max_res2 is None:
            raise ValueError("max_drop > 0 asks for pruning: max_res2 (px^2) has no default, it is the capture's noise")
        if views is not None:
            assert views.is_cuda and views.is_contiguous() and views.dtype == torch.int32 and views.shape == (T, Q), views.shape
        out = out or self._refine_out(T, Q, Cn)
        shapes = {"xyz": (T, Q, 3), "err": (T, Q), "res2": (T, Q, Cn), "cov": (T, Q, 6), "views": (T, Q), "dropped": (T, Q), "iters": (T, Q),
                  "status": (T, Q)}
        assert all(out[k].shape == s and out[k].is_contiguous() for k, s in shapes.items()), {k: out[k].shape for k in shapes}
        pts_ptr, pt_st, pt_sc, f64 = pts if pts is not None else (None, 0, 0, 1)
        _abi.check(self.lib.mocap_refine_points(self._h, _ptr(xyz), _ptr(n), _ptr(views), T, Q, Cn, pts_ptr, pt_st, pt_sc, int(f64), int(P),
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
            assert grp.is_cuda and grp.is_contiguous() and grp.dtype == torch.float64 and grp.dim() == 4 and grp.shape[3] == 2, grp.shape
            assert tuple(grp.shape[:2]) == tuple(xyz.shape[:2]), (grp.shape, xyz.shape)
            return self._refine_call(xyz, n, views, int(grp.shape[2]), None, 0, None, grp, distorted, max_iters, ftol, lambda0, max_res2,
                                     min_views, max_drop, out)
        if idx is None or views is None:
            raise ValueError("refine_points: the indexed form needs idx and views")
        assert pts.is_cuda and pts.is_contiguous() and pts.dim() == 4 and pts.shape[3] == 2 and pts.shape[0] == xyz.shape[0], pts.shape
        f64 = pts.dtype == torch.float64
        assert f64 or pts.dtype == torch.int32
        Cn, P = int(pts.shape[1]), int(pts.shape[2])
        assert idx.is_cuda and idx.is_contiguous() and idx.dtype == torch.int32 and idx.shape == tuple(xyz.shape[:2]) + (Cn,), idx.shape
        return self._refine_call(xyz, n, views, Cn, (_ptr(pts), Cn * P * 2, P * 2, f64), P, idx, None, distorted, max_iters, ftol, lambda0,
                                 max_res2, min_views, max_drop, out)

    def refine_points_records(self, xyz, n, views, idx, records, Cn, t0=0, stride_t=None, stride_c=None, P=None, points=None,
                              distorted=False, max_iters=10, ftol=1e-9, lambda0=1e-3, max_res2=None, min_views=2, max_drop=0, out=None):
        """refine_points' indexed form straight from centroid records, laid out and read as correspond_visible_records reads
        them (`points` included)."""
        rec_ints = records.shape[-1]
        flat = records.reshape(-1, rec_ints)
        stride_t = Cn if stride_t is None else stride_t
        stride_c = 1 if stride_c is None else stride_c
        P = P or min(255, (rec_ints - 2) // 2)
        base = flat.data_ptr() + 4 * rec_ints * stride_t * t0
        pts = (C.c_void_p(base + 8), rec_ints * stride_t, rec_ints * stride_c, False) if points is None else \
            self._record_points(points, records, P, stride_t, stride_c, t0) + (True,)
        assert idx.is_cuda and idx.is_contiguous() and idx.dtype == torch.int32 and idx.shape == tuple(xyz.shape[:2]) + (Cn,), idx.shape
        return self._refine_call(xyz, n, views, Cn, pts, P, idx, None, distorted, max_iters, ftol, lambda0, max_res2, min_views, max_drop, out)

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
        assert xyz.is_cuda and xyz.is_contiguous() and xyz.dtype == torch.float64 and xyz.dim() == 3 and xyz.shape[2] == 3, xyz.shape
        assert n.is_cuda and n.is_contiguous() and n.dtype == torch.int32
        assert state.is_cuda and state.is_contiguous()
        T, Q = int(xyz.shape[0]), int(xyz.shape[1])
        assert n.numel() >= T, (n.shape, T)
        steps = T if steps is None else int(steps)
        if not 0 <= steps <= T:
            raise ValueError(f"steps {steps} outside 0..{T}")
        nbytes = state.numel() * state.element_size()
        max_tracks = nbytes // 64 - 1
        if nbytes % 64 or max_tracks < 1:
            raise ValueError(f"a state of {nbytes} bytes is not one of track_state()")
        if out is None:
            out = {k: torch.full((T, Q), -1, dtype=torch.int32, device=self.device) for k in ("id", "slot", "age")}
            out["status"] = torch.zeros((T,), dtype=torch.int32, device=self.device)
        assert all(out[k].shape == (T, Q) and out[k].is_contiguous() for k in ("id", "slot", "age")) and out["status"].shape == (T,)
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
        assert xyz.is_cuda and xyz.is_contiguous() and xyz.dtype == torch.float64 and xyz.dim() == 3 and xyz.shape[2] == 3, xyz.shape
        assert n.is_cuda and n.is_contiguous() and n.dtype == torch.int32
        T, Q, B = int(xyz.shape[0]), int(xyz.shape[1]), int(bodies["model"].shape[0])
        assert n.numel() >= T, (n.shape, T)
        if out is None:
            out = self._rigid_out(T, B)
        shapes = {"R": (T, B, 9), "t": (T, B, 3), "q": (T, B, 4), "rms": (T, B), "n_in": (T, B), "label": (T, B, 8), "status": (T, B)}
        assert all(out[k].shape == s and out[k].is_contiguous() for k, s in shapes.items()), {k: out[k].shape for k in shapes}
        _abi.check(self.lib.mocap_rigid_poses(self._h, _ptr(xyz), _ptr(n), T, Q, B, _ptr(bodies["model"]), _ptr(bodies["n_markers"]),
                                              _ptr(bodies["tri"]), _ptr(bodies["n_tri"]), float(tol), float(gate), int(min_markers),
                                              int(max_hyp), _ptr(out["R"]), _ptr(out["t"]), _ptr(out["q"]), _ptr(out["rms"]),
                                              _ptr(out["n_in"]), _ptr(out["label"]), _ptr(out["status"]), _stream()))
        return out

    def _rigid_out(self, T, B):
        dev = self.device
        out = {k: torch.zeros((T, B) + s, dtype=torch.float64, device=dev) for k, s in (("R", (9,)), ("t", (3,)), ("q", (4,)), ("rms", ()))}
        out["n_in"] = torch.zeros((T, B), dtype=torch.int32, device=dev)
        out["label"] = torch.full((T, B, 8), -1, dtype=torch.int32, device=dev)
        out["status"] = torch.zeros((T, B), dtype=torch.int32, device=dev)
        return out

    def epipolar_scores(self, roots, cand, f_index=0, with_lines=False):
        """The scoring step of the correspondence search for one camera pair (reference lib/Helpers.py:205-220): roots [R, 2]
        camera-0 points, cand [N, 2] points of camera f_index + 1 (host arrays, integer or float) -> distances [R, N] float64
        (and the float32 lines [R, 3]) as host arrays.  Requires set_fundamentals."""
        roots, cand = np.asarray(roots), np.asarray(cand)
        f64 = not (roots.dtype.kind in "iu" and cand.dtype.kind in "iu")
        dt = np.float64 if f64 else np.int32
        d_r = torch.from_numpy(np.ascontiguousarray(roots, dt).reshape(-1, 2)).to(self.device)
        d_c = torch.from_numpy(np.ascontiguousarray(cand, dt).reshape(-1, 2)).to(self.device)
        dist = torch.empty((d_r.shape[0], d_c.shape[0]), dtype=torch.float64, device=self.device)
        lines = torch.empty((d_r.shape[0], 3), dtype=torch.float32, device=self.device) if with_lines else None
        _abi.check(self.lib.mocap_epipolar_scores(self._h, _ptr(d_r), d_r.shape[0], _ptr(d_c), d_c.shape[0], int(f64), int(f_index),
                                                  _ptr(dist), _ptr(lines), _stream()))
        return (dist.cpu().numpy(), lines.cpu().numpy()) if with_lines else dist.cpu().numpy()

    def triangulate_batch(self, pts, valid, compact_k=True):
        """pts [N, C, 2] float64 host array, valid [N, C] -> (xyz [N,3], ok [N]) host arrays."""
        pts = np.ascontiguousarray(pts, np.float64)
        N, Cn = pts.shape[:2]
        d_pts = torch.from_numpy(pts).to(self.device)
        d_val = torch.from_numpy(np.ascontiguousarray(valid, np.uint8).reshape(N, Cn)).to(self.device)
        xyz = torch.zeros((N, 3), dtype=torch.float64, device=self.device)
        ok = torch.zeros((N,), dtype=torch.int32, device=self.device)
        _abi.check(self.lib.mocap_triangulate_batch(self._h, _ptr(d_pts), _ptr(d_val), N, Cn, int(compact_k), _ptr(xyz),
                                                    _ptr(ok), _stream()))
        return xyz.cpu().numpy(), ok.cpu().numpy()

    def reproject_batch(self, pts, valid, xyz, compact_k=True):
        pts = np.ascontiguousarray(pts, np.float64)
        N, Cn = pts.shape[:2]
        d_pts = torch.from_numpy(pts).to(self.device)
        d_val = torch.from_numpy(np.ascontiguousarray(valid, np.uint8).reshape(N, Cn)).to(self.device)
        d_xyz = torch.from_numpy(np.ascontiguousarray(xyz, np.float64).reshape(N, 3)).to(self.device)
        mse = torch.zeros((N,), dtype=torch.float64, device=self.device)
        ok = torch.zeros((N,), dtype=torch.int32, device=self.device)
        _abi.check(self.lib.mocap_reproject_batch(self._h, _ptr(d_pts), _ptr(d_val), _ptr(d_xyz), N, Cn, int(compact_k),
                                                  _ptr(mse), _ptr(ok), _stream()))
        return mse.cpu().numpy(), ok.cpu().numpy()

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
            a = np.ascontiguousarray(a, np.float64)
            b = np.ascontiguousarray(b, np.float64)
            if a.ndim != 2 or a.shape[1] != 2 or a.shape != b.shape:
                raise ValueError(f"pair {p}: point lists must both be [N][2], got {a.shape} and {b.shape}")
            lists_a.append(a)
            lists_b.append(b)
            offset.append(offset[-1] + len(a))
        smp = np.ascontiguousarray(np.stack([np.asarray(s) for s in samples]) if isinstance(samples, (list, tuple)) else samples,
                                   np.int32)
        if smp.ndim != 3 or smp.shape[0] != n_pairs or smp.shape[2] != 8:
            raise ValueError(f"samples must be [n_pairs = {n_pairs}][H][8], got {smp.shape}")
        H = smp.shape[1]
        offset = np.array(offset, np.int32)
        total = int(offset[-1])
        dev = self.device
        d_a = torch.from_numpy(np.concatenate(lists_a)).to(dev)
        d_b = torch.from_numpy(np.concatenate(lists_b)).to(dev)
        d_s = torch.from_numpy(smp).to(dev)
        F_s = torch.full((n_pairs, 9), float("nan"), dtype=torch.float64, device=dev)
        F_r = torch.full((n_pairs, 9), float("nan"), dtype=torch.float64, device=dev) if refit else None
        mask = torch.empty((max(total, 1),), dtype=torch.uint8, device=dev)
        status = torch.empty((n_pairs, 2), dtype=torch.int32, device=dev)
        counts = torch.empty((n_pairs, H), dtype=torch.int32, device=dev) if with_counts else None
        _abi.check(self.lib.mocap_fundamental_ransac(self._h, n_pairs, _ptr(d_a), _ptr(d_b), offset.ctypes.data_as(C.POINTER(C.c_int)),
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

    def _rig_upload(self, obs_offset, obs_cam, obs_uv, poses, points, need_cameras=True):
        """Device copies of a rig problem in the layout of mocap_rig_bundle_adjust (checked here, so that a mistake is a
        ValueError with a reason and not only the kernel's MOCAP_RIG_E_LAYOUT).  need_cameras=False: the caller hands the
        lenses in itself (the entries that refine them), set_cameras is not asked for."""
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
        if need_cameras and getattr(self, "n_cam", 0) < Cn:
            raise ValueError(f"set_cameras: {getattr(self, 'n_cam', 0)} cameras set, {Cn} needed (their K and dist are used)")
        if not (np.isfinite(uv).all() and np.isfinite(poses).all() and np.isfinite(points).all()):
            raise ValueError("observations, poses and points must be finite")
        dev = self.device
        return (Cn, N, n_obs, torch.from_numpy(off).to(dev), torch.from_numpy(cam).to(dev), torch.from_numpy(uv).to(dev),
                torch.from_numpy(poses).to(dev), torch.from_numpy(points).to(dev))

    @staticmethod
    def _rig_loss(loss, loss_scale):
        """(MOCAP_RIG_LOSS_* number, scale) of the loss keywords: a name of RIG_LOSSES, or a number handed to the library as it
        is (which refuses what it does not know)"""
        if isinstance(loss, str):
            if loss not in RIG_LOSSES:
                raise ValueError(f"loss {loss!r}: one of {sorted(RIG_LOSSES)}")
            loss = RIG_LOSSES[loss]
        return int(loss), 0.0 if loss_scale is None else float(loss_scale)

    def rig_linearize(self, obs_offset, obs_cam, obs_uv, poses, points, lam, loss=None, loss_scale=None):
        """The pieces of one iteration of rig_bundle_adjust at a given state and damping (mocap_rig_linearize): dict with cost
        (1/2 sum r^2), gradient [6 (C - 1) + 3 N], S [D][D] (damped reduced camera matrix), rhs [D], behind (a point is not
        in front of a camera that sees it).  Arguments as rig_bundle_adjust; K and dist come from set_cameras.  loss,
        loss_scale: as rig_bundle_adjust's (mocap_rig_linearize_robust: cost 1/2 sum rho, the rest from the weighted blocks)."""
        robust = () if loss is None else self._rig_loss(loss, loss_scale)
        Cn, N, n_obs, d_off, d_cam, d_uv, d_poses, d_pts = self._rig_upload(obs_offset, obs_cam, obs_uv, poses, points)
        D = 6 * (Cn - 1)
        dev = self.device
        cost = torch.zeros((1,), dtype=torch.float64, device=dev)
        grad = torch.zeros((D + 3 * N,), dtype=torch.float64, device=dev)
        S = torch.zeros((D, D), dtype=torch.float64, device=dev)
        rhs = torch.zeros((D,), dtype=torch.float64, device=dev)
        status = torch.zeros((2,), dtype=torch.int32, device=dev)
        fn = self.lib.mocap_rig_linearize_robust if robust else self.lib.mocap_rig_linearize
        _abi.check(fn(self._h, Cn, N, n_obs, _ptr(d_off), _ptr(d_cam), _ptr(d_uv), _ptr(d_poses), _ptr(d_pts), float(lam), _ptr(cost),
                      _ptr(grad), _ptr(S), _ptr(rhs), _ptr(status), *robust, _stream()))
        self.sync()
        status = status.cpu().numpy()
        if status[0]:
            raise _abi.MocapError(-2, "mocap_rig_linearize: the observation arrays break the layout rules (MOCAP_RIG_E_LAYOUT)")
        return {"cost": float(cost.cpu().numpy()[0]), "gradient": grad.cpu().numpy(), "S": S.cpu().numpy(), "rhs": rhs.cpu().numpy(),
                "behind": bool(status[1])}

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
        selfcal = intrinsics is not None
        robust = () if loss is None and not selfcal else self._rig_loss(loss or 0, loss_scale)
        Cn, N, n_obs, d_off, d_cam, d_uv, d_poses, d_pts = self._rig_upload(obs_offset, obs_cam, obs_uv, poses, points, not selfcal)
        max_iters = int(max_iters)
        hist = torch.empty((max_iters, 4), dtype=torch.float64, device=self.device)
        result = torch.zeros((4,), dtype=torch.float64, device=self.device)
        if selfcal:
            d_kd, mask = self._rig_lenses(intrinsics, refine, Cn)
            per_obs = torch.empty((2, n_obs), dtype=torch.float64, device=self.device)
            _abi.check(self.lib.mocap_rig_bundle_adjust_intrinsics(
                self._h, Cn, N, n_obs, _ptr(d_off), _ptr(d_cam), _ptr(d_uv), _ptr(d_kd), mask.ctypes.data_as(C.POINTER(C.c_int)),
                _ptr(d_poses), _ptr(d_pts), max_iters, float(ftol), float(lambda0), _ptr(hist), _ptr(result), *robust,
                _ptr(per_obs[0]), _ptr(per_obs[1]), _stream()))
        elif robust:
            per_obs = torch.empty((2, n_obs), dtype=torch.float64, device=self.device)
            _abi.check(self.lib.mocap_rig_bundle_adjust_robust(self._h, Cn, N, n_obs, _ptr(d_off), _ptr(d_cam), _ptr(d_uv), _ptr(d_poses),
                                                               _ptr(d_pts), max_iters, float(ftol), float(lambda0), _ptr(hist),
                                                               _ptr(result), *robust, _ptr(per_obs[0]), _ptr(per_obs[1]), _stream()))
        else:
            _abi.check(self.lib.mocap_rig_bundle_adjust(self._h, Cn, N, n_obs, _ptr(d_off), _ptr(d_cam), _ptr(d_uv), _ptr(d_poses),
                                                        _ptr(d_pts), max_iters, float(ftol), float(lambda0), _ptr(hist), _ptr(result),
                                                        _stream()))
        self.sync()
        result = result.cpu().numpy()
        status, iters = int(result[0]), int(result[1])
        if status <= 0:
            what = {-2: "the observation arrays break the layout rules" + (", or a camera has fewer observations than twice the lens "
                                                                                 "parameters its mask frees" if selfcal else "") +
                        " (MOCAP_RIG_E_LAYOUT)",
                    -3: "in the start state a point is not in front of a camera that sees it, or the cost is not finite "
                        "(MOCAP_RIG_E_BEHIND)"}.get(status, f"status {status}")
            raise _abi.MocapError(status, "mocap_rig_bundle_adjust: " + what)
        out = {"poses": d_poses.cpu().numpy(), "points": d_pts.cpu().numpy(), "status": status, "iterations": iters,
               "cost_initial": float(result[2]), "cost": float(result[3]), "history": hist.cpu().numpy()[:iters].copy()}
        if robust:
            per_obs = per_obs.cpu().numpy()
            out["obs_err"], out["obs_weight"] = per_obs[0].copy(), per_obs[1].copy()
        if selfcal:
            out["intrinsics"] = d_kd.cpu().numpy()
        return out

    def _rig_lenses(self, intrinsics, refine, Cn):
        """(device copy of intrinsics [C][9], host int32 mask [C]) of the entries that refine the lenses.  Only the shapes are
        checked here: what the values lack is the library's MOCAP_E_INVALID."""
        kd = np.ascontiguousarray(intrinsics, np.float64)
        if kd.shape != (Cn, 9):
            raise ValueError(f"intrinsics must be [{Cn}][9] (fx, fy, cx, cy, k1, k2, p1, p2, k3), got {kd.shape}")
        mask = np.ascontiguousarray(np.broadcast_to(np.asarray(refine, np.int32), (Cn,)))
        return torch.from_numpy(kd).to(self.device), mask

    def rig_linearize_intrinsics(self, obs_offset, obs_cam, obs_uv, intrinsics, refine, poses, points, lam, loss=None, loss_scale=None):
        """The pieces of one iteration of rig_bundle_adjust_intrinsics at a given state and damping
        (mocap_rig_linearize_intrinsics): dict with cost, gradient [15 C + 3 N] (per camera the 9 lens parameters, then the 6 of
        the pose; then the points), S [15 C][15 C], rhs [15 C], behind.  Arguments as rig_bundle_adjust's."""
        robust = self._rig_loss(loss or 0, loss_scale)
        Cn, N, n_obs, d_off, d_cam, d_uv, d_poses, d_pts = self._rig_upload(obs_offset, obs_cam, obs_uv, poses, points, False)
        d_kd, mask = self._rig_lenses(intrinsics, refine, Cn)
        D = 15 * Cn
        dev = self.device
        cost = torch.zeros((1,), dtype=torch.float64, device=dev)
        grad = torch.zeros((D + 3 * N,), dtype=torch.float64, device=dev)
        S = torch.zeros((D, D), dtype=torch.float64, device=dev)
        rhs = torch.zeros((D,), dtype=torch.float64, device=dev)
        status = torch.zeros((2,), dtype=torch.int32, device=dev)
        _abi.check(self.lib.mocap_rig_linearize_intrinsics(
            self._h, Cn, N, n_obs, _ptr(d_off), _ptr(d_cam), _ptr(d_uv), _ptr(d_kd), mask.ctypes.data_as(C.POINTER(C.c_int)),
            _ptr(d_poses), _ptr(d_pts), float(lam), _ptr(cost), _ptr(grad), _ptr(S), _ptr(rhs), _ptr(status), *robust, _stream()))
        self.sync()
        status = status.cpu().numpy()
        if status[0]:
            raise _abi.MocapError(-2, "mocap_rig_linearize_intrinsics: the observation arrays break the layout rules, or a camera has "
                                      "fewer observations than twice the lens parameters its mask frees (MOCAP_RIG_E_LAYOUT)")
        return {"cost": float(cost.cpu().numpy()[0]), "gradient": grad.cpu().numpy(), "S": S.cpu().numpy(), "rhs": rhs.cpu().numpy(),
                "behind": bool(status[1])}

    def _intr_upload(self, view_offset, point_offset, obj_xy, img_uv):
        """Host offsets and device copies of a board-view problem in the layout of mocap_intrinsics_calibrate.  Only the
        shapes are checked here: what a camera or a view lacks is that camera's MOCAP_INTR_E_LAYOUT."""
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
        dev = self.device
        return n_cams, n_views, voff, poff, torch.from_numpy(obj).to(dev), torch.from_numpy(img).to(dev)

    def intrinsics_linearize(self, view_offset, point_offset, obj_xy, img_uv, kd, view_poses, lam):
        """The pieces of one iteration of intrinsics_calibrate at a given state and damping (mocap_intrinsics_linearize): dict
        with cost [n_cams] (1/2 sum r^2), gradient [9 n_cams + 6 n_views] (cameras first), S [n_cams][9][9] (damped reduced
        camera matrix), rhs [n_cams][9], layout [n_cams] (the camera breaks the layout rules: its entries are zero), behind
        [n_cams] (a point is not in front of its view's camera).  Arguments as intrinsics_calibrate."""
        n_cams, n_views, voff, poff, d_obj, d_img = self._intr_upload(view_offset, point_offset, obj_xy, img_uv)
        kd = np.ascontiguousarray(kd, np.float64).reshape(n_cams, 9)
        poses = np.ascontiguousarray(view_poses, np.float64).reshape(n_views, 12)
        dev = self.device
        d_kd, d_poses = torch.from_numpy(kd).to(dev), torch.from_numpy(poses).to(dev)
        cost = torch.zeros((n_cams,), dtype=torch.float64, device=dev)
        grad = torch.zeros((9 * n_cams + 6 * n_views,), dtype=torch.float64, device=dev)
        S = torch.zeros((n_cams, 9, 9), dtype=torch.float64, device=dev)
        rhs = torch.zeros((n_cams, 9), dtype=torch.float64, device=dev)
        status = torch.zeros((n_cams, 2), dtype=torch.int32, device=dev)
        ip = C.POINTER(C.c_int)
        _abi.check(self.lib.mocap_intrinsics_linearize(self._h, n_cams, voff.ctypes.data_as(ip), poff.ctypes.data_as(ip), _ptr(d_obj),
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
        n_cams, n_views, voff, poff, d_obj, d_img = self._intr_upload(view_offset, point_offset, obj_xy, img_uv)
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
            d_kd, d_poses = torch.from_numpy(kd).to(dev), torch.from_numpy(poses).to(dev)
        rms = torch.zeros((n_views,), dtype=torch.float64, device=dev)
        hist = torch.empty((n_cams, max_iters, 4), dtype=torch.float64, device=dev)
        result = torch.zeros((n_cams, 4), dtype=torch.float64, device=dev)
        ip = C.POINTER(C.c_int)
        _abi.check(self.lib.mocap_intrinsics_calibrate(self._h, n_cams, voff.ctypes.data_as(ip), poff.ctypes.data_as(ip), _ptr(d_obj),
                                                       _ptr(d_img), size.ctypes.data_as(ip), int(start is not None), max_iters,
                                                       float(ftol), float(lambda0), _ptr(d_kd), _ptr(d_poses), _ptr(rms), _ptr(hist),
                                                       _ptr(result), _stream()))
        self.sync()
        result, hist = result.cpu().numpy(), hist.cpu().numpy()
        iters = result[:, 1].astype(np.int64)
        return {"kd": d_kd.cpu().numpy(), "poses": d_poses.cpu().numpy(), "view_rms": rms.cpu().numpy(),
                "status": result[:, 0].astype(np.int64), "iterations": iters, "cost_initial": result[:, 2].copy(),
                "cost": result[:, 3].copy(), "history": [hist[c, :iters[c]].copy() for c in range(n_cams)]}

    def ba_problem(self, pts, valid=None):
        """Bundle-adjustment residuals with the image points resident on the GPU (see BAProblem)."""
        return BAProblem(self, pts, valid)

    # ---- the exchange step (one all-gather of centroid records, RCCL over xGMI) -----------------------------------
    def comm_init(self, unique_id, rank, world):
        """Collective over all ranks: create this context's RCCL communicator from the bytes rank 0 got from
        `comm_unique_id()` (handed around by the host, e.g. through torch.distributed)."""
        buf = (C.c_char * _abi.COMM_ID_BYTES).from_buffer_copy(bytes(unique_id))
        _abi.check(self.lib.mocap_comm_init(self._h, C.cast(buf, C.c_void_p), int(rank), int(world)))
        self.comm_world = int(world)

    def comm_share(self, src):
        """Local: use the communicator of `src` (another context of this rank on the same GPU) -- one communicator per rank,
        whatever the number of batches in flight; the library orders the all-gathers issued through it."""
        _abi.check(self.lib.mocap_comm_share(self._h, src._h))
        self.comm_world = src.comm_world

    def comm_destroy(self):
        _abi.check(self.lib.mocap_comm_destroy(self._h))
        self.comm_world = 1

    def allgather_centroids(self, local, out=None):
        """local: this rank's centroid records (int32, contiguous, on this GPU) -> [world * len(local), ...] on every
        rank, in rank order; asynchronous on the current stream."""
        assert local.is_cuda and local.is_contiguous() and local.dtype == torch.int32
        world = self.comm_world
        if out is None:
            out = torch.empty((world * local.shape[0],) + tuple(local.shape[1:]), dtype=torch.int32, device=local.device)
        assert out.is_contiguous() and out.numel() == world * local.numel() and out.dtype == torch.int32
        _abi.check(self.lib.mocap_allgather_centroids(self._h, _ptr(local), _ptr(out), local.numel(), _stream()))
        return out

    # ---- profiling -----------------------------------------------------------------------------------------------
    def tile_stats(self):
        """(tiles, tiles resolved by the dark-tile early-out) of the most recent blob_centroids batch"""
        a, b = C.c_uint64(0), C.c_uint64(0)
        _abi.check(self.lib.mocap_tile_stats(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def list_stats(self):
        """(box items, wide-tile entries, wide tiles split at their empty columns) of the most recent batch's sparse path"""
        a, b, s = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
        _abi.check(self.lib.mocap_list_stats(self._h, C.byref(a), C.byref(b), C.byref(s)))
        return a.value, b.value, s.value

    def own_mask(self, n):
        """The first n images of the context's own mask -- what blob_centroids filtered into, kept from batch to batch -- as the
        row-major int32 [n, H, ceil(W / 32)] mask of filter_mask (mocap_own_mask).  Reads only; stream-ordered."""
        mask = torch.zeros((int(n), self.height, (self.width + 31) // 32), dtype=torch.int32, device=self.device)
        _abi.check(self.lib.mocap_own_mask(self._h, int(n), _ptr(mask), _stream()))
        return mask

    def profile(self, on=True):
        _abi.check(self.lib.mocap_profile_enable(self._h, int(on)))

    def profile_read(self):
        """Accumulated HIP-event milliseconds / launch counts per kernel since the last read (mocap_hip.h)."""
        ms = (C.c_double * 5)()
        n = (C.c_int * 5)()
        _abi.check(self.lib.mocap_profile_read(self._h, ms, n))
        return {"filter_ms": ms[0], "filter_launches": n[0], "contour_ms": ms[1], "contour_launches": n[1],
                "corr_ms": ms[2], "corr_launches": n[2], "scan_ms": ms[3], "scan_launches": n[3],
                "settle_ms": ms[4], "settle_launches": n[4]}


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


def comm_available():
    """Local check, no communication: can this process load RCCL (mocap_comm_available)?  Raises MocapError when not."""
    _abi.check(_abi.load().mocap_comm_available())
    return True


def comm_unique_id():
    """MOCAP_COMM_ID_BYTES opaque bytes (ncclGetUniqueId) for MocapContext.comm_init; call on rank 0 only."""
    buf = (C.c_char * _abi.COMM_ID_BYTES)()
    _abi.check(_abi.load().mocap_comm_unique_id(C.cast(buf, C.c_void_p)))
    return bytes(buf)


_contexts = threading.local()


def default_context(width=1, height=1, n_slots=1, device=None):
    """Per-thread context cache keyed by geometry (the drop-in modules under mocapv2_amd.lib use it).  A context owns
    per-batch scratch, so its calls must not interleave; the reference runs one `_find_dot` loop per camera thread
    (RealtimeTracking_FLIR.py:307-312) -- each of those threads gets a context of its own here, and its buffers go
    with the thread."""
    if device is None:
        device = torch.cuda.current_device() if torch.cuda.is_available() else 0
    key = (int(width), int(height), int(n_slots), int(device))
    cache = _contexts.__dict__.setdefault("cache", {})
    ctx = cache.get(key)
    if ctx is None:
        ctx = cache[key] = MocapContext(width, height, n_slots, device)
    return ctx
