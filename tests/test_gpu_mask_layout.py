"""The C-ABI's row-major masks around the kernels' internal mask layout (32-row blocks, kernels.h): what mocap_filter_mask
writes and mocap_contours_from_mask reads is the documented [n][H][ceil(W/32)] mask, at heights that are not multiples of 32,
and the context's own mask is cleared correctly from batch to batch."""
import numpy as np
import pytest

import oracle
from mocapv2_amd.synth import MILD_DIST, Scene
from test_gpu_blob import dark_frames, make_ctx, rand_frames

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


@pytest.mark.parametrize("W,H", [(37, 1), (257, 1), (41, 31), (301, 33), (999, 33), (1921, 1080), (1919, 1081)])
def test_filter_mask_writes_row_major_mask_twice(torch_cuda, W, H):
    from gpu_util import unpack_mask
    torch = torch_cuda
    rng = np.random.default_rng(W * 31 + H)
    ctx, K, ident = make_ctx(W, H)
    assert ident
    wpr = (W + 31) // 32
    buf = torch.zeros((3, H, wpr), dtype=torch.int32, device="cuda")
    for rnd in range(2):  # the second call must replace every bit of the first one's mask
        frames = rand_frames(rng, 3, H, W, bright=0.3 if rnd == 0 else 0.05, blobs=3 if rnd == 0 else 1) if H < 64 else \
            dark_frames(rng, 3, H, W, n_discs=40 if rnd == 0 else 5, salt=0.002 if rnd == 0 else 0.0005)
        out = ctx.filter_mask(torch.from_numpy(frames).cuda(), mask=buf)
        assert out.data_ptr() == buf.data_ptr()
        got, pad = unpack_mask(buf, W)
        assert not pad.any(), rnd
        for i in range(3):
            exp = oracle.image_filter(frames[i], 0) != 0
            assert np.array_equal(got[i], exp), (rnd, i, np.argwhere(got[i] != exp)[:5])


@pytest.mark.parametrize("W,H", [(301, 33), (1921, 1081)])
def test_contours_from_caller_mask_match_oracle(torch_cuda, W, H):
    from gpu_util import check_against_oracle, pack_mask
    rng = np.random.default_rng(H)
    frames = dark_frames(rng, 2, H, W, n_discs=3 if H < 64 else 30, salt=0.001)
    masks = np.stack([oracle.image_filter(f, 0) for f in frames])
    ctx, K, ident = make_ctx(W, H)
    min_area, min_circ = 5.0, 0.3
    ctx.set_blob_params(min_area=min_area, min_circ=min_circ)
    xy, cnt, recs = ctx.contours_from_mask(pack_mask(masks), max_blobs=128, debug_cap=384)
    xy, cnt = xy.cpu().numpy(), cnt.cpu().numpy()
    for i in range(2):
        check_against_oracle(masks[i], recs[i], xy[i], cnt[i], min_area, min_circ, 128)


def test_blob_centroids_two_batches_one_context(torch_cuda):
    """Consecutive batches of different content (and size) on one context: what the first left in the context's own mask is
    cleared where the second does not write."""
    torch = torch_cuda
    from mocapv2_amd.engine import MocapContext
    W, H = 1000, 550
    sc = Scene(3, width=W, height=H, dist=MILD_DIST)
    ctx = MocapContext(W, H, n_slots=3)
    for s in range(3):
        ctx.set_undistort(s, sc.K, sc.dist)
    total = 0
    for seed, steps, markers in ((3, 3, 24), (4, 2, 6), (5, 3, 12)):
        frames = sc.render_batch(seed=seed, n_steps=steps, n_markers=markers, radius_range=(10, 24), salt=0.001)
        xy, cnt = ctx.record_views(ctx.blob_centroids(torch.from_numpy(frames).cuda(), cam_mod=3))
        xy, cnt = xy.cpu().numpy(), cnt.cpu().numpy()
        flat = frames.reshape(-1, H, W)
        for i in range(len(flat)):
            exp = oracle.find_dot(flat[i], sc.K, sc.dist)
            assert cnt[i] == len(exp), (seed, i)
            assert xy[i, :cnt[i]].tolist() == exp, (seed, i)
            total += len(exp)
    assert total >= 60
