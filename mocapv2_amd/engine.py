"""Host side of the hot path: a thin object over the C-ABI context.

PyTorch is used only as the device allocator / stream provider (tensors are passed to the library as raw
pointers); no torch operator touches the data.  Mirrors what the reference's callers do around
lib.ImageOperations._find_dot and lib.Helpers.find_point_correspondance_and_object_points
(reference RealtimeTracking_FLIR.py:95-143,157-209) for whole batches of frames.
MocapContext is one mixin per stage, each in a module that mirrors the library's abi_*.hip file (engine_blob, _geom, _calib,
_track, _comm); this module holds the context itself (abi_ctx.hip, abi_undistort.hip) and re-exports the stages' names.
"""
import ctypes as C
import threading

import numpy as np
import torch

from . import _abi
from ._dev import _dbl, _ptr, _stream  # noqa: F401
from .engine_blob import (GRAY_SHIFT, MAX_BLOBS, REC_INTS, SUBPIX_COORDS, SUBPIX_CUT, SUBPIX_EDGE, SUBPIX_EMPTY,  # noqa: F401
                          SUBPIX_FALLBACK, SUBPIX_MOVING, SUBPIX_NEIGHBOUR, BlobStage)
from .engine_calib import RIG_LOSSES, CalibStage  # noqa: F401
from .engine_comm import CommStage, comm_available, comm_unique_id  # noqa: F401
from .engine_geom import BAProblem, GeomStage  # noqa: F401
from .engine_track import (LEARN_CHUNK, LEARN_E_INCOMPLETE, LEARN_E_MEMBERS, LEARN_MAX_GROUPS, LEARN_MAX_IDS,  # noqa: F401
                           RIGID_E_BLIND, RIGID_E_CAPACITY, RIGID_E_HYP, RIGID_E_MODEL, RIGID_LOST, RIGID_MAX_BODIES,
                           RIGID_MAX_DETECTIONS, RIGID_MAX_HYP, RIGID_MAX_MARKERS, RIGID_MAX_TRIPLES, TrackStage, learn_work_bytes,
                           rigid_groups, rigid_tables)


class MocapContext(BlobStage, GeomStage, CalibStage, TrackStage, CommStage):
    """One GPU, one image geometry.  Not a singleton: one per camera thread or per process is fine."""

    def __init__(self, width, height, n_slots=1, device=0):
        self.lib = _abi.load()
        if not torch.cuda.is_available():
            raise RuntimeError("mocapv2_amd needs a ROCm GPU (torch.cuda.is_available() is False); no CPU fallback")
        self.device = torch.device("cuda", device)
        self.width, self.height, self.n_slots = int(width), int(height), int(n_slots)
        self._h = C.c_void_p()
        _abi.check(self.lib.mocap_ctx_create(device, self.width, self.height, self.n_slots, C.byref(self._h)))
        self._cam_key = self._f_key = None
        self._und_key = {}
        self._warned_dense = set()  # causes set_undistort has warned about
        self.identity = {}
        self.n_cam, self.comm_world = 0, 1  # cameras of set_cameras; ranks of the communicator (comm_init, comm_share)

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

    def profile(self, on=True):
        _abi.check(self.lib.mocap_profile_enable(self._h, int(on)))

    def profile_read(self):
        """Accumulated HIP-event milliseconds / launch counts per kernel since the last read (mocap_hip.h)."""
        ms = (C.c_double * 5)()
        n = (C.c_int * 5)()
        _abi.check(self.lib.mocap_profile_read(self._h, ms, n))
        return {f"{k}_{what}": v[i] for i, k in enumerate(("filter", "contour", "corr", "scan", "settle"))
                for what, v in (("ms", ms), ("launches", n))}


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
