"""The oracle's cv.undistort against an independent NumPy restatement, on every lens of the catalogue (tests/lens_cases.py):
asymmetric and anisotropic lenses, tangential-only maps, strong barrel / pincushion, the int16 wrap of cv::remap's integer
parts, the compact table's 11-bit edge and the lens the product ships with.  Also pins what the catalogue claims about
each lens (its route, the staged-band condition), so that the GPU tests in test_gpu_lens.py test what they say they do."""
import numpy as np
import pytest

import oracle
from lens_cases import K1_1023, K1_1024, NAMES, ROWS_STAGE_U, _max_disp, case, catalogue, closed_form_map, \
    compact_disp, compact_fits, int_parts, reference_lens, remap_u8, route, staged_bands
from mocapv2_amd import synth


def test_catalogue_names_and_reference_lens():
    assert [c.name for c in catalogue()] == NAMES
    K, d = reference_lens()
    assert K[0, 0] != K[1, 1] and K[0, 1] == 0 and d[4] > 3 and d[2] < 0 and d[3] < 0
    for name in ("reference_2048x1536", "reference_1920x1080"):
        c = case(name)
        assert 0 <= c.K[0, 2] < c.W and 0 <= c.K[1, 2] < c.H  # the frame holds the principal point
    for name in ("offcentre_fy125", "offcentre_fy080"):
        c = case(name)
        assert abs(c.K[0, 2] / c.W - 0.5) >= 0.15 and abs(c.K[1, 2] / c.H - 0.5) >= 0.15
        assert c.K[1, 1] / c.K[0, 0] in (0.8, 1.25)
    t = case("tangential").dist
    assert not t[[0, 1, 4]].any() and t[2] * t[3] < 0 and 0.01 <= min(abs(t[2]), abs(t[3]))


@pytest.mark.parametrize("name", NAMES)
def test_map_is_the_closed_form_model(name):
    """Every pixel of the quantised map is round(32 u), round(32 v) of the closed-form OpenCV model: catches swapped
    p1 / p2 or fx / fy, a wrong principal point or stripe offset (A[5] = v0 - ys), a sign error in a term."""
    c = case(name)
    iu, iv = oracle.undistort_map(c.H, c.W, c.K, c.dist)
    u, v = closed_form_map(c.H, c.W, c.K, c.dist)
    assert np.abs(iu - 32 * u).max() <= 0.5 + 1e-6
    assert np.abs(iv - 32 * v).max() <= 0.5 + 1e-6


@pytest.mark.parametrize("name", NAMES)
def test_remap_is_integer_bilinear(name):
    """oracle.undistort = cv::remap's fixed-point blend through the oracle's own map, bit for bit."""
    c = case(name)
    rng = np.random.default_rng(sum(map(ord, name)))
    img = rng.integers(0, 256, (c.H, c.W), dtype=np.uint8)
    iu, iv = oracle.undistort_map(c.H, c.W, c.K, c.dist)
    assert np.array_equal(oracle.undistort(img, c.K, c.dist), remap_u8(img, iu, iv))


@pytest.mark.parametrize("name", NAMES)
def test_expected_route_matches_the_table_model(name):
    """The route each case is meant to take, from a NumPy model of the tables mocap_set_undistort builds."""
    c = case(name)
    assert route(c.H, c.W, c.K, c.dist) == c.expected_route


def test_int16_wrap_case_wraps():
    """cv::remap keeps (short)(iu >> 5): corner sources beyond 32767 px wrap, some of them back into the frame."""
    c = case("int16_wrap")
    iu, iv = oracle.undistort_map(c.H, c.W, c.K, c.dist)
    sx, sy = int_parts(iu, iv)
    wrapped = ((iu >> 5) != sx) | ((iv >> 5) != sy)
    assert wrapped.any() and (np.abs(iu >> 5) > 32767).any()
    inside = (sx >= 0) & (sx < c.W) & (sy >= 0) & (sy < c.H)
    assert (wrapped & inside).any()


def test_compact_table_boundary():
    """The compact table holds displacements in [-1024, 1023]: a largest |d| of 1023 fits, 1024 does not.  The two k1 lie
    in the middles of their plateaus, so a rounding difference in a last bit cannot move them across."""
    W, H = 4096, 2160
    K = synth.intrinsics(W, H)
    assert case("compact_1023").dist[0] == K1_1023 and case("compact_1024").dist[0] == K1_1024
    for k1, d, fits in ((K1_1023, 1023, True), (K1_1024, 1024, False)):
        for k in (k1 - 2e-4, k1, k1 + 2e-4):
            assert _max_disp(H, W, K, (k, 0, 0, 0, 0)) == (d, fits), k
    dx4, dy4 = compact_disp(*oracle.undistort_map(H, W, K, (K1_1024, 0, 0, 0, 0)))
    assert dx4.max() == 1024 and not compact_fits(dx4, dy4)


@pytest.mark.parametrize("name", ["staged_overflow", "pincushion"])
def test_staged_overflow_lens_reaches_the_condition(name):
    """filter_rows_staged_kernel stages a band's source rectangle in 576 units of LDS per wave.  These lenses at the
    default buffer size have bands that are not staged (n > 576) and touch the image border (not interior), where the
    staging store's index is only clamped to the rectangle's last inside unit: it would address LDS beyond the wave's
    buffer without the early return in stage_write."""
    c = case(name)
    assert c.W % 16 == 0 and c.expected_route["compact_table"]
    bands = staged_bands(c.H, c.W, c.K, c.dist)
    hit = [b for b in bands if b["n"] > ROWS_STAGE_U and not b["interior"] and b["top_store"] >= ROWS_STAGE_U]
    assert hit and all(not b["staged"] for b in hit)
    assert any(b["staged"] for b in bands)  # ... beside bands that are staged: both forms in one launch


def test_mild_lenses_stay_inside_the_buffer():
    """The band model on the lenses test_filter_mask_remap stages: no band reaches the condition above (why it went unseen)."""
    for W, H in [(64, 48), (960, 540)]:
        K = np.array([[0.7 * W, 0, W / 2.0], [0, 0.7 * W, H / 2.0], [0, 0, 1]])
        for scale in (1.0, 4.0, -3.0):
            bands = staged_bands(H, W, K, np.array(synth.MILD_DIST) * scale)
            assert not [b for b in bands if not b["staged"] and not b["interior"] and b["top_store"] >= ROWS_STAGE_U]
