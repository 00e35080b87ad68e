"""The inputs that put mocap_correspond_visible on its integer seams (csrc/correspond_visible.hip): exactly `cap` seeds in a pass
and one more, a power of two for the sort and one more, several time steps side by side in the scratch, max_hyp at the seed
count in scratch, and the output rows running out in a later pass.  Not a test module: tests/test_visible_seams_host.py proves on
the CPU that every case is what its name says, tests/test_gpu_visible_seams.py compares the device with the restatement.

Every cutoff comes from first_pass_distances: the midpoint between the k-th and the (k+1)-th seed distance of pass 0 gives that
pass exactly k seeds, and half the gap between the two is how far the nearest comparison lies from the cutoff."""
import functools

import numpy as np

import correspond_visible_ref as cv

C, P = 8, 32                 # with CAMW = 47 and 24-byte records the 64 KiB plan holds 2048 records in LDS (the host test restates it)
CAP = 2048
COUNTS = (1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097)
SEEDS = (1, 2)               # seed 3's smallest decision margin is 4.4e-7, below the suite's 1e-6: not used
MAX_HYP = 8192
SMALL = (8, 6, 0.2, 5)       # the few-seed neighbour: scene_case(*SMALL), padded to P


@functools.lru_cache(maxsize=None)
def scene(seed):
    return cv.scene_case(C, P, 0.2, seed)


@functools.lru_cache(maxsize=None)
def cams():
    return cv.scene_arrays(scene(1)[0])  # the rig is the same for every seed: synth.Scene(8, 1920, 1080)


@functools.lru_cache(maxsize=None)
def distances(seed):
    _, pts, counts, _, _ = scene(seed)
    return cv.first_pass_distances(pts, counts, *cams())


def cutoff_for(seed, k):
    """(cutoff, half gap): pass 0 of scene(seed) has exactly k seeds at this cutoff"""
    d = distances(seed)
    return float(0.5 * (d[k - 1] + d[k])), float(0.5 * (d[k] - d[k - 1]))


def padded(case, width=P):
    """pts [C, width, 2] and counts of a case with fewer slots per camera"""
    pts = np.zeros((C, width, 2))
    pts[:, :case[1].shape[1]] = case[1]
    return pts, case[2].astype(np.int32)


def reversed_lists(pts, counts):
    """every camera's list in the opposite order: other keys (i, j) for the same geometry"""
    out = pts.copy()
    for c in range(len(counts)):
        out[c, :counts[c]] = pts[c, :counts[c]][::-1]
    return out


def single(seed, k):
    """(pts [1, C, P, 2], counts [1, C], cutoff, half gap) of one count of the sweep"""
    _, pts, counts, _, _ = scene(seed)
    cut, gap = cutoff_for(seed, k)
    return pts[None].copy(), counts[None].astype(np.int32), cut, gap


@functools.lru_cache(maxsize=None)
def small():
    return padded(cv.scene_case(*SMALL))


def four_steps():
    """(pts [4, C, P, 2], counts [4, C], cutoff): seed 1 with exactly CAP seeds (LDS), seed 2 beyond CAP (scratch), the small
    scene (LDS), seed 2 reversed (scratch) -- all at seed 1's cutoff for CAP seeds"""
    cut, _ = cutoff_for(1, CAP)
    p1, c1 = scene(1)[1], scene(1)[2].astype(np.int32)
    p2, c2 = scene(2)[1], scene(2)[2].astype(np.int32)
    ps, cs = small()
    return np.stack([p1, p2, ps, reversed_lists(p2, c2)]), np.stack([c1, c2, cs, c2]), cut


def with_neighbour(seed, k):
    """(pts [2, C, P, 2], counts [2, C], cutoff): scene(seed) with exactly k seeds as step 0, the small scene as step 1"""
    cut, _ = cutoff_for(seed, k)
    ps, cs = small()
    return np.stack([scene(seed)[1], ps]), np.stack([scene(seed)[2].astype(np.int32), cs]), cut


# rows running out in a later pass: seed 1 at 2049 seeds in pass 0 (scratch), then an LDS pass that accepts more markers
LATER_PASS = (1, 2049)


@functools.lru_cache(maxsize=None)
def restatement(seed, k, **kw):
    """the restatement's result of single(seed, k), computed once"""
    pts, counts, cut, _ = single(seed, k)
    return cv.correspond_visible(pts[0], counts[0], *cams(), cutoff=cut, max_hyp=kw.pop("max_hyp", MAX_HYP), **kw)


# ---- cases beyond the sweep: what the sweep's results cannot show -----------------------------------------------------------
def twelve_steps():
    """(pts [12, C, P, 2], counts [12, C], cutoff, the four_steps() index of every step).  Workgroups are dealt to the eight XCDs
    in turn, and two XCDs do not see each other's stores to the scratch before the kernel ends: the four steps of four_steps()
    sit on four XCDs and could share scratch unnoticed.  Here steps t and t + 8 share an XCD and its L2, and wherever one of
    them works in scratch the other is another scene in scratch: 1 and 9, 3 and 11."""
    pts, counts, cut = four_steps()
    order = [0, 1, 2, 3, 0, 1, 2, 3, 2, 3, 0, 1]
    return pts[order], counts[order], cut, order


def seeds_in_lane_order(pts, counts, cutoff):
    """[(w, a, i, b, j)] of pass 0, ascending in w = pair * Pm^2 + i * Pm + j (Pm the largest count): find_seeds' work items"""
    c = cv.Cameras(*cams())
    Pm = int(counts.max())
    out = []
    with np.errstate(all="ignore"):
        for pr, (a, b) in enumerate(c.pairs):
            d = cv._seed_distances(c.F[pr], pts[a, :counts[a]], pts[b, :counts[b]])
            out += [(pr * Pm * Pm + int(i) * Pm + int(j), a, int(i), b, int(j)) for i, j in zip(*np.nonzero(d < cutoff))]
    return sorted(out)


# what an earlier call leaves behind a pass's records: every seed of POISON is kept as a two-view hypothesis (no support within a
# gate of 1e-3 px, any error below 1e30 px^2), so every scratch record up to 4096 holds a kept hypothesis with free points; DROPPED
# then works on 2049 seeds none of which is kept (no error is below 1e-9 px^2): records 2049.. still hold the earlier call's
POISON = dict(seeds=4097, gate=1e-3, max_err=1e30)
DROPPED = dict(seeds=CAP + 1, max_err=1e-9)


# ---- more than `cap` seeds, each the only seed of a marker of its own ---------------------------------------------------------
# 32 cameras x 128 slots leave the 160 KiB plan room for 512 records (the 64 KiB plan holds none); 513 markers that two cameras
# each see once, almost jitter-free, at a cutoff far below the chance epipolar coincidences and a gate that collects no support:
# 513 seeds, every one accepted as a two-view marker.  Losing any one seed loses a marker.
DISJOINT = dict(C=32, P=128, cap=512, markers=513, jitter=1e-5, cutoff=1.5e-4, gate=1e-3, seed=1, other_seed=3)


@functools.lru_cache(maxsize=None)
def disjoint_scene(seed):
    """(pts [1, 32, 128, 2], counts [1, 32], cams): marker m is seen by two cameras drawn for it, every list shuffled"""
    from mocapv2_amd.synth import ZERO_DIST, Scene
    n_cam, slots, n = DISJOINT["C"], DISJOINT["P"], DISJOINT["markers"]
    rng = np.random.default_rng(seed)
    sc = Scene(n_cam, 1920, 1080, dist=ZERO_DIST)
    markers = sc.markers(rng, n)
    seen = np.array([rng.choice(n_cam, 2, replace=False) for _ in range(n)])
    pts = np.zeros((n_cam, slots, 2))
    counts = np.zeros(n_cam, np.int32)
    for c in range(n_cam):
        mine = np.flatnonzero((seen == c).any(axis=1))
        px = sc.pixels(markers[mine], c, distorted=False) + rng.normal(0, DISJOINT["jitter"], (len(mine), 2))
        px = px[rng.permutation(len(mine))]
        pts[c, :len(mine)] = px
        counts[c] = len(mine)
    return pts[None], counts[None], cv.scene_arrays(sc)


def disjoint_kw():
    """one pass: a second one would find a seed that the first one lost again, its two points still free, and hide the loss"""
    return dict(cutoff=DISJOINT["cutoff"], gate=DISJOINT["gate"], max_hyp=MAX_HYP, max_passes=1)


def seed_keys(pts, counts, cams_, cutoff):
    """{(a, i, b, j)} of pass 0"""
    c = cv.Cameras(*cams_)
    out = set()
    with np.errstate(all="ignore"):
        for pr, (a, b) in enumerate(c.pairs):
            if counts[a] and counts[b]:
                d = cv._seed_distances(c.F[pr], pts[a, :counts[a]], pts[b, :counts[b]])
                out |= {(a, int(i), b, int(j)) for i, j in zip(*np.nonzero(d < cutoff))}
    return out
