"""The records forms of the geometry entries through a layout no other test reaches: camera-major records read from a time
step t0 > 0, with a float64 points block beside them whose rows exceed P.  Both forms reach the same kernel with the same
numbers, so every specified row equals the dense form's bit for bit."""
import numpy as np
import pytest

from mocapv2_amd.pipeline import scene_arrays
from mocapv2_amd.synth import MILD_DIST, Scene

pytestmark = pytest.mark.gpu

C, M, T_TOTAL, T, T0, P, CAP, ROWS = 3, 3, 3, 2, 1, 4, 8, 6
REC_INTS = 2 + 2 * CAP


def layout_case():
    """records int32 [C, T_TOTAL, REC_INTS] (camera-major; their own points are decoys), points float64 [C * T_TOTAL, ROWS, 2]
    beside them, and the same values as dense pts [T, C, P, 2], counts [T, C] of the time steps T0 .. T0 + T - 1"""
    sc = Scene(C, dist=MILD_DIST)
    records = np.zeros((C, T_TOTAL, REC_INTS), np.int32)
    points = np.full((C, T_TOTAL, ROWS, 2), -7.25)  # rows at and beyond a count, and beyond P: never a result
    for s in range(T_TOTAL):
        rng = np.random.default_rng(40 + s)
        markers = sc.markers(rng, M)
        for c in range(C):
            px = sc.pixels(markers, c, distorted=False)[rng.permutation(M)]
            if s == 2 and c == 1:
                px = np.concatenate([px, rng.uniform(0, 1000, (1, 2))])  # a stray point: P rows in use
            records[c, s, 0] = len(px)
            records[c, s, 2:] = rng.integers(0, 1000, 2 * CAP)
            points[c, s, :len(px)] = px
    pts = np.ascontiguousarray(points[:, T0:T0 + T, :P].transpose(1, 0, 2, 3))
    counts = np.ascontiguousarray(records[:, T0:T0 + T, 0].T)
    return sc, records, points.reshape(C * T_TOTAL, ROWS, 2), pts, counts


def assert_rows_equal(got, want, keys, n, what):
    for t in range(T):
        assert n[t] > 0, (what, t, n[t])
        for k in keys:
            a, b = got[k][t, :n[t]].cpu().numpy(), want[k][t, :n[t]].cpu().numpy()
            assert a.tobytes() == b.tobytes(), (what, k, t)


def test_camera_major_records_from_t0_with_a_points_block_equal_the_dense_forms():
    import torch
    from mocapv2_amd.engine import MocapContext
    sc, records, points, pts, counts = layout_case()
    K, dist, R, t, F = scene_arrays(sc)
    ctx = MocapContext(1, 1)
    ctx.set_cameras(K, dist, R, t)
    ctx.set_fundamentals(F)
    d_rec, d_points = torch.from_numpy(records).cuda(), torch.from_numpy(points).cuda()
    d_pts, d_cnt = torch.from_numpy(pts).cuda(), torch.from_numpy(counts).cuda()
    lay = dict(t0=T0, stride_t=1, stride_c=T_TOTAL, P=P, points=d_points)

    dense = ctx.correspond(d_pts, d_cnt)
    rec = ctx.correspond_records(d_rec, T, C, **lay)
    n = dense["n"].cpu().numpy()
    assert np.array_equal(rec["n"].cpu().numpy(), n)
    assert_rows_equal(rec, dense, ("xyz", "err", "grp", "root", "order"), n, "correspond")

    dense = ctx.correspond_visible(d_pts, d_cnt)
    rec = ctx.correspond_visible_records(d_rec, T, C, **lay)
    n = dense["n"].cpu().numpy()
    assert np.array_equal(rec["n"].cpu().numpy(), n)
    assert_rows_equal(rec, dense, ("xyz", "err", "idx", "views"), n, "correspond_visible")

    fine = ctx.refine_points(dense["xyz"], dense["n"], views=dense["views"], pts=d_pts, idx=dense["idx"])
    rec = ctx.refine_points_records(dense["xyz"], dense["n"], dense["views"], dense["idx"], d_rec, C, **lay)
    torch.cuda.synchronize()
    assert all((fine["status"][s, :n[s]] > 0).all() for s in range(T)), fine["status"]
    assert_rows_equal(rec, fine, ("xyz", "err", "res2", "cov", "views", "dropped", "iters", "status"), n, "refine_points")
