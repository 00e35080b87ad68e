"""The context's own mask, read back (mocap_own_mask) and compared bit for bit with the oracle's after EVERY batch of sequences of calls
on one context.  mocap_blob_centroids filters into that mask and never zeroes it between batches: settle_tiles_kernel
(blob_settle.hip) clears what a tile's previous region holds where this batch will not write, and abi_blob.hip zeroes all of it
after the general kernel wrote it whole (mask_dirty).  A stale fragment that touches no blob of the new batch, is smaller than the
area gate or has no contour area changes no centroid -- it is wrong all the same, and turns into a wrong centroid only batches later.

After every mocap_blob_centroids call of a sequence (own_mask_cases.SEQUENCES; excess base pinned, the gates of test_gpu_box_forms):
  (a) every image the own mask holds equals the oracle's mask: the batch's images, and beyond them what the last batch that held them
      left (zeros after the mask was zeroed) -- no tolerance, the first differing pixels are printed;
  (b) the centroids equal the oracle's;
  (c) where every slot holds the identity lens and the sparse path ran, mocap_list_stats equals the totals of own_mask_cases.routes().
The mask is read back before any mocap_filter_mask call on the context, except in the sequence that interleaves the two on purpose.
tests/lens_cases.py has no lens at or below 512 x 208 whose table is not compact (compact_1024 is 4096 x 2160), so the general
kernel is reached through skip_dark 0 and mocap_image_filter_u8 only.

Which pairs (previous route -> this batch's route (how the regions lie)) the sequences meet under the identity lens, as
test_own_mask_host.py prints and asserts them:
  unmarked_and_items    item -> item (covers, disjoint, inside, same), item -> unmarked, unmarked -> item
  wide_item_split       item -> split (covers), item -> wide, split -> item (inside), split -> split (overlap) x2, split -> unmarked,
                        split -> wide, unmarked -> wide, wide -> item, wide -> split x2
  cluster               cluster_emit -> cluster_emit / item / split, cluster_member -> cluster_member / item (same) / unmarked,
                        item -> cluster_emit / cluster_member (same), split -> cluster_emit, unmarked -> cluster_emit / cluster_member
  dense_kernel          split -> dense, unmarked -> dense, dense -> item, dense -> unmarked
  all_hot               unmarked -> wide x16 / item / cluster_emit / cluster_member and back, wide -> item (inside)
  image_filter_between  dense -> item / split / unmarked (33 tiles of 3 images)
  batch_sizes           wide -> item, item -> split, split -> item, cluster -> unmarked (images 1 and 2 across a 1-image batch)
  two_slots             wide -> item, split -> cluster_emit, cluster_emit -> wide on the identity slot
  filter_mask_between   item -> split (covers), split -> item (inside), split -> unmarked
  bayer_direct          wide -> item, item -> split (same), split -> item, item -> wide (covers), wide -> unmarked
  edges_251             item -> item (disjoint, same), split -> split (covers, inside), item -> unmarked

That the cases bite: the library was built four times with one mutation each (stores or a condition removed) and this file run once
against each build; beside it the parent's tests that watch the same mask through centroids (test_gpu_blob.py::
test_context_mask_stays_consistent_across_batches, ::test_batches_of_varying_size_on_one_context,
::test_blob_centroids_two_batches_one_context, test_gpu_box_forms.py, test_gpu_wide_split.py::test_stale_bits_of_the_previous_batch,
test_gpu_tile_record.py::test_no_stale_bits_in_either_array).
  M1  the split override of need_clear dropped (settle_tiles_kernel): 12 of the 42 cases here fail, all on the mask -- wide_item_split
      (every variant but the two with wide_split 0, which never split) at gap_disc -> two, filter_mask_between and batch_sizes at
      disc -> two / three (46 to 62 stale pixels of the disc in the gap), edges_251-zero, test_read_back_reads_only.  The parent's: all pass.
  M2  clear_previous forgets the last byte column: 14 fail -- cluster, batch_sizes and two_slots at corner -> disc / dark (20 to 22
      pixels of the corner disc in columns 232..239 of tile (0, 0)), all_hot in every variant at hot -> dark (columns 232..239, 472..479).
      The parent's: all pass.
  M3  record_region skips the clear whenever the tile is marked: 33 fail (every sequence but dense_kernel and image_filter_between).
      The parent's: test_batches_of_varying_size_on_one_context (both) and test_blob_centroids_two_batches_one_context fail, 18 pass.
  M4  the hipMemsetAsync of the mask_dirty branch skipped: 4 fail -- dense_kernel and image_filter_between under both lenses, at the
      first sparse batch behind the general kernel.  The parent's: all pass.
"""
import numpy as np
import pytest

import oracle
from gpu_util import unpack_mask
from mocapv2_amd._abi import MocapError
from own_mask_cases import FRAMES, LENSES, SEQUENCES, gray_of, routes, totals
from test_gpu_box_forms import expected, make_ctx
from test_gpu_tile_record import BASE

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def same_mask(got, want, what):
    if not np.array_equal(got, want):
        d = np.argwhere(got != want)
        raise AssertionError(f"{what}: {len(d)} pixels differ; first (y, x, bit read): {[(int(y), int(x), int(got[y, x])) for y, x in d[:8]]}")


def centroids(ctx, records):
    xy, cnt = ctx.record_views(records)
    xy, cnt = xy.cpu().numpy(), cnt.cpu().numpy()
    return [(int(cnt[i]), xy[i, :max(int(cnt[i]), 0)].tolist()) for i in range(len(cnt))]


def play(torch, name, lens="zero", tuning=(), read_back=True):
    """the sequence on one context, (a), (b), (c) after every batch; returns what the calls gave: [(step, centroids, list counts)]"""
    seq = SEQUENCES[name]
    Hh, Ww = seq["shape"]
    lens_now = [lens if l == "run" else l for l in seq["lenses"]]
    cm = len(lens_now)
    ctx, K = make_ctx(Ww, Hh, [LENSES[l] for l in lens_now], [("excess_base", BASE)] + list(tuning))
    wide_split = dict(tuning).get("wide_split", 1) != 0
    held, dirty, dense, log = [], False, False, []  # held: the oracle's mask of every image the own mask holds

    def check_own(what):
        if not read_back:
            return
        got, pad = unpack_mask(ctx.own_mask(len(held)), Ww)
        assert not pad.any(), what
        for i, want in enumerate(held):
            same_mask(got[i], want, f"{name} {what} own mask image {i}")

    def oracle_of(names, bayer):
        frames = np.stack([FRAMES[n] for n in names])
        return frames, [expected(frames[i:i + 1], K, np.asarray(LENSES[lens_now[i % cm]], float), bayer)[0] for i in range(len(frames))]

    for s, step in enumerate(seq["steps"]):
        what = f"step {s} {step}"
        if step[0] == "tune":
            ctx.set_tuning(step[1], step[2])
            dense = dense if step[1] != "skip_dark" else step[2] == 0
        elif step[0] == "lens":
            lens_now[step[1]] = step[2]
            ctx.set_undistort(step[1], K, LENSES[step[2]])
        elif step[0] == "image_filter":  # the general kernel over image 0 of the own mask, no undistortion
            f = FRAMES[step[1]]
            want = oracle.image_filter(f, 0) != 0
            same_mask(ctx.image_filter(torch.from_numpy(f).cuda()).cpu().numpy() != 0, want, what)
            held[0], dirty = want, True
            check_own(what)
        elif step[0] == "filter_mask":  # a caller-owned mask: the own one stays what it was
            frames, exp = oracle_of(step[1], False)
            got, pad = unpack_mask(ctx.filter_mask(torch.from_numpy(frames).cuda(), cam_mod=cm), Ww)
            assert not pad.any(), what
            for i in range(len(frames)):
                same_mask(got[i], exp[i][0], f"{name} {what} caller's mask image {i}")
            check_own(what)
        else:
            bayer = step[0] == "bayer"
            frames, exp = oracle_of(step[1], bayer)
            n = len(frames)
            rec = ctx.blob_centroids(torch.from_numpy(frames).cuda(), cam_mod=cm, bayer_pattern=3 if bayer else None)
            if n > len(held):  # the mask group grows: a new, zeroed mask
                held, dirty = [np.zeros((Hh, Ww), bool)] * n, False
            if dirty and not dense:  # back on the sparse path after the general kernel: all of the mask is zeroed first
                held, dirty = [np.zeros((Hh, Ww), bool)] * len(held), False
            held[:n] = [e[0] for e in exp]
            dirty = dirty or dense
            check_own(what)  # (a)
            got = centroids(ctx, rec)
            for i in range(n):  # (b)
                assert got[i] == (len(exp[i][1]), exp[i][1]), (name, what, i, got[i], exp[i][1])
            stats = ctx.list_stats()
            if dense:  # (c) the general kernel has no work lists: none are reported, under any lens (not the previous batch's)
                assert stats == (0, 0, 0), (name, what, stats)
            elif all(l == "zero" for l in lens_now):
                per = [totals(routes(gray_of(nm, bayer), wide_split, wide_list=not bayer)) for nm in step[1]]
                want = tuple(sum(p[k] for p in per) for k in range(3))
                print(name, what, "items, wide, split:", stats, "from the routes:", want)
                assert stats == want, (name, what, stats, want)
            log.append((s, got, stats))
    return ctx, log


SWITCHES = {"default": [], "wide_split0": [("wide_split", 0)], "wide_split2": [("wide_split", 2)], "scan_hotmap0": [("scan_hotmap", 0)],
            "scan_hotmap2": [("scan_hotmap", 2)], "split0_hotmap2": [("wide_split", 0), ("scan_hotmap", 2)]}
CASES = []
for _name, _seq in SEQUENCES.items():
    for _lens in (["zero", "mild2"] if "run" in _seq["lenses"] else ["as_listed"]):
        CASES.append((_name, _lens, "default"))
    if _seq["switches"]:
        CASES += [(_name, "zero", sw) for sw in SWITCHES if sw != "default"] + [(_name, "mild2", "wide_split0"), (_name, "mild2", "scan_hotmap2")]


@pytest.mark.parametrize("name,lens,switch", CASES, ids=["-".join(c) for c in CASES])
def test_own_mask_after_every_batch(torch_cuda, name, lens, switch):
    play(torch_cuda, name, lens, SWITCHES[switch])


# ---- the read-back itself -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lens", ["zero", "mild2"])
@pytest.mark.parametrize("names", [["two", "bar", "corner"], ["edges_a", "edges_b"]], ids=["H208", "H77"])
def test_read_back_equals_filter_mask_of_a_fresh_context(torch_cuda, names, lens):
    """two entry points, two mask buffers, one conversion out of the 32-row blocks: the same words, at heights that are no multiple of 32"""
    torch = torch_cuda
    frames = np.stack([FRAMES[n] for n in names])
    Hh, Ww = frames.shape[1:]
    d = torch.from_numpy(frames).cuda()
    ctx, K = make_ctx(Ww, Hh, [LENSES[lens]], [("excess_base", BASE)])
    ctx.blob_centroids(d)
    own = ctx.own_mask(len(frames))
    fresh, _ = make_ctx(Ww, Hh, [LENSES[lens]], [("excess_base", BASE)])
    other = fresh.filter_mask(d)
    assert own.shape == other.shape == (len(frames), Hh, (Ww + 31) // 32)
    got, pad = unpack_mask(own, Ww)
    assert not pad.any()
    for i in range(len(frames)):
        same_mask(got[i], unpack_mask(other, Ww)[0][i], f"image {i}: own mask against mocap_filter_mask")
        same_mask(got[i], expected(frames[i:i + 1], K, np.asarray(LENSES[lens], float), False)[0][0], f"image {i}: own mask against the oracle")
    assert torch.equal(own, other)
    assert torch.equal(ctx.own_mask(1), own[:1])  # fewer images than the mask holds: the first ones


def test_read_back_reads_only(torch_cuda):
    """read twice: the same bits; and a context that was read back after every batch gives the same centroids, list counts and tile
    counts as one that never was, and ends with the same mask"""
    torch = torch_cuda
    ctx, _ = make_ctx(512, 208, [LENSES["zero"]], [("excess_base", BASE)])
    ctx.blob_centroids(torch.from_numpy(FRAMES["two"][None]).cuda())
    first, second = ctx.own_mask(1), ctx.own_mask(1)
    assert torch.equal(first, second) and bool(first.any())
    read, log_read = play(torch, "wide_item_split")
    never, log_never = play(torch, "wide_item_split", read_back=False)
    assert log_read == log_never
    assert read.tile_stats() == never.tile_stats() and read.list_stats() == never.list_stats()
    n = len(SEQUENCES["wide_item_split"]["steps"][-1][1])
    assert torch.equal(read.own_mask(n), never.own_mask(n))


def test_error_returns(torch_cuda):
    torch = torch_cuda
    ctx, _ = make_ctx(512, 208, [LENSES["zero"]])
    with pytest.raises(MocapError, match="the context's own mask holds 0 images"):  # no batch into the own mask yet
        ctx.own_mask(1)
    ctx.blob_centroids(torch.from_numpy(np.stack([FRAMES["disc"], FRAMES["two"]])).cuda())
    assert ctx.own_mask(2).shape == (2, 208, 16)
    with pytest.raises(MocapError, match="n_images = 3, the context's own mask holds 2 images"):
        ctx.own_mask(3)
    with pytest.raises(MocapError, match="n_images = 0"):
        ctx.own_mask(0)
    rc = ctx.lib.mocap_own_mask(ctx._h, 1, None, None)
    assert rc == -1 and ctx.lib.mocap_last_error() == b"null argument"
    rc = ctx.lib.mocap_own_mask(None, 1, ctx.own_mask(1).data_ptr(), None)
    assert rc == -1 and ctx.lib.mocap_last_error() == b"null argument"
