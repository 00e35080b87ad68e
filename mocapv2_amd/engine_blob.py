"""The blob stage of MocapContext (abi_blob.hip): centroid records from frames, sub-pixel centroids, the mask and contour steps
on their own, the single-image utilities.  What the reference's callers do around lib.ImageOperations._find_dot, for batches."""
import ctypes as C

import numpy as np
import torch

from . import _abi
from ._dev import AtLeast, _ptr, _stream, outputs

MAX_BLOBS = 128       # centroid record capacity per camera image
# Fixed point of cv2.cvtColor(., COLOR_BGR2GRAY) on 8-bit images in the camera loop (RealtimeTracking_FLIR.py:104).
# The reference pins no OpenCV version (README.md:65), so `pip install opencv-python` gives a current 4.x, whose
# RGB2Gray<uchar> works with gray_shift = 15 (RY15 = 9798, GY15 = 19235, BY15 = 3735, + 2^14, >> 15;
# modules/imgproc/src/color.simd_helpers.hpp); OpenCV 2.x / 3.x used the 14-bit set (4899, 9617, 1868).  Both are
# implemented and tested; the default follows the version the reference's users get today.  oracle/check_against_cv2.py
# settles it wherever cv2 can be imported (it cannot in the build container).
GRAY_SHIFT = 15
REC_INTS = 2 + 2 * MAX_BLOBS  # int32 record: count, pad, xy[MAX_BLOBS][2]
SUBPIX_COORDS = {"raw": 0, "ideal": 1}  # mocap_refine_centroids' coords
SUBPIX_EMPTY, SUBPIX_EDGE, SUBPIX_NEIGHBOUR, SUBPIX_MOVING, SUBPIX_CUT = 1, 2, 4, 8, 16  # MOCAP_SUBPIX_*
SUBPIX_FALLBACK = SUBPIX_EMPTY | SUBPIX_EDGE | SUBPIX_NEIGHBOUR | SUBPIX_MOVING  # the point holds its integer centroid


class BlobStage:
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
        into = (C.c_void_p(records.data_ptr() + 8), rec_ints, _ptr(records), rec_ints, max_blobs, _stream())
        if bayer_pattern is None:
            _abi.check(self.lib.mocap_blob_centroids(self._h, _ptr(flat), n, cam_mod, slot_base, stride, pitch, *into))
            return records
        assert gray is None or (gray.dtype == torch.uint8 and gray.is_cuda and gray.reshape(flat.shape).stride() == flat.stride())
        _abi.check(self.lib.mocap_blob_centroids_bayer(self._h, _ptr(flat), _ptr(gray), n, cam_mod, slot_base, stride, pitch,
                                                       bayer_pattern, gray_shift, *into))
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
        rows = (n, AtLeast(max_blobs), 2)  # a caller's tensors may hold more rows per image than are refined
        out = outputs({"xy": (rows, torch.float64, 0), "info": (rows, torch.int32, 0)}, self.device, out)
        xy, info = out["xy"], out["info"]
        _abi.check(self.lib.mocap_refine_centroids(self._h, _ptr(flat), n, cam_mod, slot_base, stride, pitch,
                                                   -1 if bayer_pattern is None else int(bayer_pattern), int(gray_shift),
                                                   C.c_void_p(records.data_ptr() + 8), rec_ints, _ptr(records), rec_ints, max_blobs,
                                                   int(radius), int(floor), int(iters), SUBPIX_COORDS[coords], _ptr(xy),
                                                   2 * xy.shape[1], _ptr(info), 2 * info.shape[1], _stream()))
        out["weight"], out["flags"] = info[:, :, 0], info[:, :, 1]
        return out

    def filter_mask(self, frames, cam_mod=1, slot_base=0, mask=None):
        flat, n, stride, pitch = self._frames(frames)
        if mask is None:
            mask = torch.zeros((n, self.height, (self.width + 31) // 32), dtype=torch.int32, device=self.device)
        _abi.check(self.lib.mocap_filter_mask(self._h, _ptr(flat), n, cam_mod, slot_base, stride, pitch, _ptr(mask), _stream()))
        return mask

    def own_mask(self, n):
        """The first n images of the context's own mask -- what blob_centroids filtered into, kept from batch to batch -- as the
        row-major int32 [n, H, ceil(W / 32)] mask of filter_mask (mocap_own_mask).  Reads only; stream-ordered."""
        mask = torch.zeros((int(n), self.height, (self.width + 31) // 32), dtype=torch.int32, device=self.device)
        _abi.check(self.lib.mocap_own_mask(self._h, int(n), _ptr(mask), _stream()))
        return mask

    def contours_from_mask(self, mask, max_blobs=MAX_BLOBS, debug_cap=0, xy=None):
        """xy: optional int32 [n, rows >= max_blobs, 2] device tensor to write into (at most max_blobs rows per image are written)."""
        n = mask.shape[0]
        assert xy is None or xy.is_cuda
        xy = outputs({"xy": ((n, AtLeast(max_blobs), 2), torch.int32, None)}, self.device, None if xy is None else {"xy": xy})["xy"]
        cnt = torch.empty((n,), dtype=torch.int32, device=self.device)
        dbg = dbg_n = None
        if debug_cap:
            dbg = torch.zeros((n, debug_cap, C.sizeof(_abi.Contour)), dtype=torch.uint8, device=self.device)
            dbg_n = torch.zeros((n,), dtype=torch.int32, device=self.device)
        _abi.check(self.lib.mocap_contours_from_mask(self._h, _ptr(mask), n, _ptr(xy), 2 * xy.shape[1], _ptr(cnt), 1, max_blobs,
                                                     _ptr(dbg), _ptr(dbg_n), debug_cap, _stream()))
        if not debug_cap:
            return xy, cnt
        raw, counts, recs = dbg.cpu().numpy(), dbg_n.cpu().numpy(), []
        for i in range(n):
            arr = (_abi.Contour * debug_cap).from_buffer_copy(raw[i].tobytes())
            recs.append([{k: getattr(arr[j], k) for k, _ in _abi.Contour._fields_} for j in range(min(counts[i], debug_cap))])
        return xy, cnt, recs

    def _image_out(self, img, any_size=False):
        assert img.is_cuda and img.dtype == torch.uint8 and (img.dim() == 2 if any_size else img.shape == (self.height, self.width))
        return torch.empty_like(img, memory_format=torch.contiguous_format)

    def image_filter(self, img, order=0, slot=-1):
        """image_filter_gpu (order 0) / image_filter_cpu (order 1) on one device image -> {0,255} device image."""
        out = self._image_out(img)
        _abi.check(self.lib.mocap_image_filter_u8(self._h, _ptr(img), _ptr(out), img.stride(0), out.stride(0), order, slot, _stream()))
        return out

    def undistort(self, img, slot=0):
        out = self._image_out(img)
        _abi.check(self.lib.mocap_undistort_u8(self._h, slot, _ptr(img), _ptr(out), img.stride(0), out.stride(0), _stream()))
        return out

    def box_blur(self, img, ksize=5):
        out = self._image_out(img, any_size=True)
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
