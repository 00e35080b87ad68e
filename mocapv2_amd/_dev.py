"""What the stage modules of the host side (engine*.py) share: raw pointers, the stream, and the layout and result-tensor helpers
that every entry goes through.  PyTorch is used only as the device allocator / stream provider (tensors are passed to the
library as raw pointers); no torch operator touches the data."""
import ctypes as C

import numpy as np
import torch


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dbl(a, n):
    a = np.ascontiguousarray(a, np.float64).reshape(-1)
    assert a.size == n, (a.size, n)
    return a, a.ctypes.data_as(C.POINTER(C.c_double))


def record_layout(base, rec_ints, Cn, t0=0, stride_t=None, stride_c=None, P=None, points=None, rows=0):
    """The layout arithmetic of the *_records entries, over addresses: centroid records (int32 [rec_ints]: count, pad, xy) from
    `base`, the record of (time step t0 + t, camera c) stride_t * t + stride_c * c records after record stride_t * t0 (default:
    time-major [T_total, Cn]); P points are read per image (default: the records' capacity, at most 255).  points: the address of
    float64 points [images, rows >= P, 2] beside the records, image for image: they are read in the records' place.  Returns (pts_ptr,
    pt_stride_t, pt_stride_c, cnt_ptr, cnt_stride_t, cnt_stride_c, pts_f64, P) as the C entries take them (strides in elements)."""
    stride_t = Cn if stride_t is None else stride_t
    stride_c = 1 if stride_c is None else stride_c
    P = P or min(255, (rec_ints - 2) // 2)
    counts = (base + 4 * rec_ints * stride_t * t0, rec_ints * stride_t, rec_ints * stride_c)  # a record begins with its count
    if points is None:
        return counts[0] + 8, rec_ints * stride_t, rec_ints * stride_c, *counts, 0, P
    assert rows >= P, (rows, P)
    return points + 8 * 2 * rows * stride_t * t0, 2 * rows * stride_t, 2 * rows * stride_c, *counts, 1, P


def records_layout(records, Cn, t0, stride_t, stride_c, P, points):
    """record_layout of a records tensor (int32 [..., rec_ints]) and, optionally, the points tensor beside it (refine_centroids' xy)"""
    rec_ints = records.shape[-1]
    base = records.reshape(-1, rec_ints).data_ptr()
    if points is None:
        return record_layout(base, rec_ints, Cn, t0, stride_t, stride_c, P)
    assert points.is_cuda and points.is_contiguous() and points.dtype == torch.float64 and points.dim() == 3, points.shape
    assert points.shape[0] == records.numel() // rec_ints and points.shape[2] == 2, (points.shape, records.shape)
    return record_layout(base, rec_ints, Cn, t0, stride_t, stride_c, P, points.data_ptr(), points.shape[1])


def dense_layout(pts, counts=None):
    """The dense form, pts [T, C, P, 2] (int32 or float64), counts [T, C] int32 on the GPU: record_layout's tuple, (T, Cn, P) for its P"""
    f64 = pts.dtype == torch.float64
    assert pts.is_cuda and pts.is_contiguous() and pts.dim() == 4 and pts.shape[3] == 2 and (f64 or pts.dtype == torch.int32), pts.shape
    assert counts is None or (counts.is_contiguous() and counts.dtype == torch.int32)
    T, Cn, P = (int(s) for s in pts.shape[:3])
    return pts.data_ptr(), Cn * P * 2, P * 2, counts.data_ptr() if counts is not None else None, Cn, 1, int(f64), T, Cn, P


def marker_rows(xyz, n):
    """(T, Q) of markers xyz [T, Q, 3] float64 and their counts n [T] int32 on the GPU, as the correspondence calls deliver them"""
    assert xyz.is_cuda and xyz.is_contiguous() and xyz.dtype == torch.float64 and xyz.dim() == 3 and xyz.shape[2] == 3, xyz.shape
    assert n.is_cuda and n.is_contiguous() and n.dtype == torch.int32
    T, Q = int(xyz.shape[0]), int(xyz.shape[1])
    assert n.numel() >= T, (n.shape, T)
    return T, Q


class AtLeast(int):
    """A dimension of an `outputs` table that a caller's tensor may exceed"""


def outputs(spec, device, out=None):
    """The result tensors of an entry.  spec: {key: (shape, dtype, fill)}, fill None = uninitialised.  out None: they are
    allocated.  Otherwise every key of the table is checked in `out` for shape (an AtLeast dimension: at least that), dtype and
    contiguity -- the library writes through these pointers -- and other keys are ignored."""
    if not out:
        return {k: torch.empty(s, dtype=dt, device=device) if fill is None else torch.full(s, fill, dtype=dt, device=device)
                for k, (s, dt, fill) in spec.items()}
    for k, (s, dt, _) in spec.items():
        t = out[k]
        fits = t.dim() == len(s) and all(g >= w if isinstance(w, AtLeast) else g == w for g, w in zip(t.shape, s))
        assert fits and t.dtype == dt and t.is_contiguous(), (k, tuple(t.shape), t.dtype, t.stride(), tuple(s), dt)
    return out
