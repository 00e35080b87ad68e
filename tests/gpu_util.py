"""Helpers shared by the -m gpu parity tests."""
import numpy as np
import torch

import oracle
from contour_cases import local_candidates


def pack_mask(mask):
    """{0,nonzero}[n,H,W] -> int32 [n,H,ceil(W/32)] device tensor, bit b of word k = pixel 32k+b."""
    mask = np.asarray(mask)
    if mask.ndim == 2:
        mask = mask[None]
    n, H, W = mask.shape
    wpr = (W + 31) // 32
    bits = np.zeros((n, H, wpr * 32), np.uint8)
    bits[:, :, :W] = mask != 0
    packed = np.packbits(bits, axis=2, bitorder="little").reshape(n, H, wpr, 4)
    words = np.ascontiguousarray(packed).view(np.uint32).reshape(n, H, wpr)
    return torch.from_numpy(words.view(np.int32).copy()).cuda()


def unpack_mask(words, W):
    """int32 [n,H,wpr] tensor -> (bool [n,H,W], padding bits)"""
    w = np.ascontiguousarray(words.cpu().numpy()).view(np.uint32)
    n, H, wpr = w.shape
    b = np.unpackbits(w.view(np.uint8).reshape(n, H, wpr * 4), axis=2, bitorder="little")
    return b[:, :, :W].astype(bool), b[:, :, W:]


def check_against_oracle(mask, recs, xy, count, min_area, min_circ, max_blobs, table=None):
    """Every border the kernel found == every border cv.findContours would list (per the oracle), with the same
    measurements, the same parent, and the kept ones in the same order.  `table`: the oracle's table of the mask for these
    gates, when the caller has it already."""
    H, W = mask.shape
    table = [dict(c) for c in (oracle.find_contours(mask, min_area=min_area, min_circ=min_circ) if table is None else table)]
    for c in table:  # discovery position: the start pixel, or the background pixel right of it for a hole
        c["key"] = c["oy"] * (W + 1) + c["ox"] + (1 if c["is_hole"] else 0)
    by_key = {(r["key"], r["is_hole"]): r for r in recs}
    assert len(recs) == len(table) == len(by_key)
    for c in table:
        r = by_key[(c["key"], c["is_hole"])]
        for f in ("a00", "a10", "a01", "npts", "steps", "kept", "cx", "cy"):
            assert r[f] == c[f], (f, r, c)
        assert r["area"] == c["area"] and r["perimeter"] == c["perimeter"]
        assert (r["sx"], r["sy"]) == (c["ox"], c["oy"])
        assert (c["a00"] > 0) == bool(c["is_hole"]) or c["a00"] == 0  # orientation tells the border kind
        exp_parent = None if c["parent_order"] < 0 else (table[c["parent_order"]]["key"], table[c["parent_order"]]["is_hole"])
        got_parent = None if r["parent"] < 0 else (recs[r["parent"]]["key"], recs[r["parent"]]["is_hole"])
        assert exp_parent == got_parent, (c, r)
    kept = [c for c in table if c["kept"]]
    assert count == len(kept)
    for j, c in enumerate(kept):
        assert by_key[(c["key"], c["is_hole"])]["order"] == j
        if j < max_blobs:
            assert list(xy[j]) == [c["cx"], c["cy"]]
    return len(table), len(kept)


# the contour stage's documented limits (include/mocap_hip.h, MOCAP_BLOB_E_*)
MAX_BORDERS, MAX_KEPT, MAX_DEPTH, MAX_CANDIDATES = 384, 256, 8, 1024


def allowed_blob_codes(mask, table):
    """The MOCAP_BLOB_E_* codes a negative count may carry for this mask: those of the documented limits that the oracle's
    table (for the gates in use) or the local start conditions show to be exceeded -- none when the mask is within all of
    them, and then the kernel owes the oracle's result.  The kernel drops starts whose run touches the row above within 12
    columns before it counts them, so its candidate count is at most local_candidates: -2 is never accepted below 1025."""
    codes = set()
    if len(table) > MAX_BORDERS or sum(c["kept"] for c in table) > MAX_KEPT:
        codes.add(-3)
    for i, c in enumerate(table):
        depth, j = 0, i
        while j >= 0:
            depth, j = depth + 1, table[j]["parent_order"]
        if c["kept"] and depth > MAX_DEPTH:
            codes.add(-5)
    if local_candidates(mask) > MAX_CANDIDATES:
        codes.add(-2)
    return codes
