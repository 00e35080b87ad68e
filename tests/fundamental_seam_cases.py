"""The inputs that put mocap_fundamental_ransac on its integer seams (csrc/fundamental.hip): point lists that end on, or one
past, the scorer's chunk of 1024 points and the mask's block of 256; hypothesis tables that end on, or one past, the solver's
wave of 64 and the scorer's and the arg-max's tile of 256; tied winners placed so that the lower index sits in the higher lane
of the arg-max's tree; and points that are no honest pixels (NaN, inf, finite values whose products overflow).  Not a test
module: tests/test_fundamental_seams_host.py proves on the CPU that the cases are what their names say,
tests/test_gpu_fundamental_seams.py compares the device with the restatement (tests/fundamental_ref.py)."""
import functools

import numpy as np

import fundamental_ref as fr
from mocapv2_amd import synth
from mocapv2_amd.calibrate import sample_table

SEED, THRESHOLD = 21, 3.0
N_MAX = 2049
POINT_COUNTS = (255, 256, 257, 1023, 1024, 1025, 2048, 2049)  # around the mask's block (256) and the scorer's chunk (1024)
HYP_COUNTS = (63, 64, 65, 255, 256, 257, 513)                # around the solver's wave (64) and the 256-hypothesis tile
N_SEAM, H_SEAM = 1025, 257   # the list and the table the other seams are crossed with
H_TIES, WINNER = 600, 19     # the table the ties are planted in; the restatement's winner of every (1025, H) table used here
# (rows the winner is copied to, the row expected to win): fund_select_kernel's thread `tid` holds the rows tid, tid + 256, ...
#   first: lane 3 holds 259 then 515, lane 200 holds 200 -- the lower index sits in the higher lane
#   second: lane 44 holds 44, 300 and 556 (three strides, the strict '>' keeps the first), its neighbour lane 45 holds 45
#   third: lane 72 holds 328 and lane 72 + 128 holds 200 -- the tree's first step finds the lower index above it
TIES = {"first": ((200, 259, 515), 200), "second": ((44, 45, 300, 556), 44), "third": ((200, 328), 200)}
NOT_FINITE = ((("a", 5), (np.nan, np.nan)), (("a", 700), (np.nan, np.nan)), (("b", 9), (np.inf, np.inf)))
OVERFLOW_POINT = 7
OVERFLOWS = {"1e200": ((1e200, 1e200), (1e200, 1e200)), "1e160": ((1e160, 2e160), (3e160, 1e160)), "inf": ((np.inf, np.inf), (np.inf, np.inf))}


@functools.lru_cache(maxsize=None)
def data():
    """a, b [2049, 2]: 30 % outliers, 0.5 px jitter"""
    a, b, _, _, _ = fr.synthetic_pair(synth.Scene(6), 0, 1, N_MAX, SEED, 0.30)
    a.setflags(write=False)
    b.setflags(write=False)
    return a, b


def pair(n):
    a, b = data()
    return a[:n], b[:n]


@functools.lru_cache(maxsize=None)
def table(n, H):
    S = sample_table(n, H, SEED)
    S.setflags(write=False)
    return S


@functools.lru_cache(maxsize=None)
def reference(n, H):
    """the restatement on the first n points with sample_table(n, H, 21), computed once"""
    a, b = pair(n)
    return fr.ransac(a, b, table(n, H), THRESHOLD)


def used_cases():
    """every (n, H) the GPU tests run on the plain data"""
    return [(n, H_SEAM) for n in POINT_COUNTS] + [(N_SEAM, H) for H in HYP_COUNTS if H != H_SEAM]


@functools.lru_cache(maxsize=None)
def tie_table(name):
    """sample_table(1025, 600, 21) with the winner's row copied to the rows of TIES[name] and the winner's own row overwritten
    with a losing one (the row behind it)"""
    rows, _ = TIES[name]
    S = table(N_SEAM, H_TIES).copy()
    for r in rows:
        S[r] = S[WINNER]
    S[WINNER] = S[WINNER + 1]
    S.setflags(write=False)
    return S


@functools.lru_cache(maxsize=None)
def tie_reference(name):
    a, b = pair(N_SEAM)
    return fr.ransac(a, b, tie_table(name), THRESHOLD)


@functools.lru_cache(maxsize=None)
def not_finite_pair():
    a, b = (x.copy() for x in pair(N_SEAM))
    for (which, i), value in NOT_FINITE:
        (a if which == "a" else b)[i] = value
    return a, b


@functools.lru_cache(maxsize=None)
def not_finite_reference():
    a, b = not_finite_pair()
    with np.errstate(all="ignore"):
        return fr.ransac(a, b, table(N_SEAM, H_SEAM), THRESHOLD)


@functools.lru_cache(maxsize=None)
def overflow_pair(name):
    a, b = (x.copy() for x in pair(N_SEAM))
    a[OVERFLOW_POINT], b[OVERFLOW_POINT] = OVERFLOWS[name]
    return a, b


@functools.lru_cache(maxsize=None)
def overflow_reference(name):
    """(the restatement on the pair, its refit over the winner's inliers with the overflowing point taken out of the lists)"""
    a, b = overflow_pair(name)
    with np.errstate(all="ignore"):
        ref = fr.ransac(a, b, table(N_SEAM, H_SEAM), THRESHOLD)
    keep = ref["mask"].copy()
    keep[OVERFLOW_POINT] = False
    return ref, fr.n_point(a[keep], b[keep])
