// contours_dev.h -- what the contour stage's two kernel files share (blob_contour_image.hip: candidates, tree and the one-kernel form;
// blob_contour_follow.hip: the walks of a batch, two lanes per border): limits, mask access, the walk's result, the per-image
// workspace and the walk lists' entries, the contour filter.
//
// Replaces cv.findContours(RETR_TREE, CHAIN_APPROX_SIMPLE) + cv.contourArea + cv.arcLength + cv.moments
// and the filter/centroid loops of reference lib/ImageOperations.py:41-65, for a batch of masks.
//
// The serial raster scan of Suzuki-Abe is replaced by its fixed point: every border is followed exactly
// once, from its raster-first pixel, so
//   * an outer border starts at a foreground pixel whose W, NW, N, NE neighbours are background and that is
//     the raster-minimum of the border it lies on;
//   * a hole border starts at the foreground pixel left of a background pixel whose W and N neighbours are
//     foreground and that is the raster-minimum of the left-side cracks of the border.
// Candidates are found with word-parallel bit tests on the mask, guided by the occupancy words the filter kernels leave
// per tile and by the tiles' boxes (settle_tiles_kernel); a group of 8 lanes holds consecutive words of a mask row.  Every
// candidate becomes one entry of a batch-wide walk list and is followed by a PAIR OF LANES of contour_follow_kernel: one lane
// forwards, one backwards from the same start, until they meet (see there); a lane reads the 3 x 3 neighbourhood of its
// current pixel from a 64 x 64 window of the mask staged in LDS (three 16-bit loads per step, one per row; a lane that reaches the
// window's rim pauses until the window is staged anew around it), the walker state and the integer Green's-theorem sums are
// per-lane registers.  The step itself is literally the reference border-following step
// (same neighbour order, same CHAIN_APPROX_SIMPLE vertex rule); a candidate is dropped as soon as one of its lanes meets an
// earlier pixel of its own border.  The polygon sums are exact integers (int64), the perimeter is a sum of correctly rounded
// float32 square roots held exactly in a double.
// Tree order (parent = enclosing border, siblings in reverse discovery order, pre-order walk) is rebuilt from
// "which border owns the crack left of my start pixel": from the bounding boxes when that is unambiguous, else by
// following that border once -- as one more entry of a (second) walk list.
// The mask is 1/8 B per pixel, in 32-row blocks (kernels.h: mask_word_index): a line holds one word column of 32 rows.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "kernels.h"

namespace mocap {

namespace {

constexpr int MAXC = 1024;  // candidates per image (after the run-level filters)
constexpr int MAXR = 384;   // borders per image
constexpr int MAXK = 256;   // kept contours per image
constexpr int MAXD = 8;     // nesting depth of a kept contour
constexpr int MAXCELL = 4096; // occupancy cells (strip x 8 rows) listed per image; with more, every cell is scanned
constexpr int MAXA = 64;    // links per image whose owner has to be found by a walk that are handed to the packed second pass

struct Mask {
    const uint32_t* w;
    int wpr, H, W;
    int RS; // raster stride W+1, so the virtual background column right of the image has its own index
    __device__ __forceinline__ uint32_t word(int y, int k) const
    {
        return ((unsigned)y < (unsigned)H && (unsigned)k < (unsigned)wpr) ? w[mask_word_index(y, k, wpr)] : 0u;
    }
};

// columns x0 .. x0+63 of row y as a 64-bit word (bit c = column x0 + c), zero outside the image; per lane and
// branch-free: the three words are loaded from clamped in-image positions and zeroed by select
__device__ __forceinline__ uint64_t row64(const Mask& M, int y, int x0)
{
    const int k0 = x0 >> 5; // arithmetic shift = floor for negative x0
    const uint32_t sh = (uint32_t)x0 & 31u;
    const int yc = y < 0 ? 0 : (y > M.H - 1 ? M.H - 1 : y);
    const uint32_t* __restrict__ rowp = M.w + mask_word_index(yc, 0, M.wpr); // the row's word k is rowp[32 k]
    const bool yin = (unsigned)y < (unsigned)M.H;
    uint32_t w[3];
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const int k = k0 + i, kc = k < 0 ? 0 : (k > M.wpr - 1 ? M.wpr - 1 : k);
        const uint32_t keep = (yin && (unsigned)k < (unsigned)M.wpr) ? 0xffffffffu : 0u;
        w[i] = rowp[(uint32_t)kc * 32u] & keep; // an AND, not a select: the load stays unconditional (no branch around it)
    }
    const uint32_t lo = __builtin_amdgcn_alignbit(w[1], w[0], sh), hi = __builtin_amdgcn_alignbit(w[2], w[1], sh);
    return ((uint64_t)hi << 32) | lo;
}

// step of direction code s (0=E 1=NE 2=N 3=NW 4=W 5=SW 6=S 7=SE), from packed 2-bit tables (value + 1) so that the
// scalar walker needs no memory access per step
__device__ __forceinline__ int dir_dx(int s) { return (int)((0x901au >> (2 * s)) & 3u) - 1; }  // 1,1,0,-1,-1,-1,0,1
__device__ __forceinline__ int dir_dy(int s) { return (int)((0xa901u >> (2 * s)) & 3u) - 1; }  // 0,-1,-1,-1,0,1,1,1

// occupancy of the 8 neighbours of a pixel, bit s = direction code s, from columns x-1 .. x+1 (bits 0 .. 2) of the row above it,
// of its own row and of the row below it
__device__ __forceinline__ uint32_t nbr_code(uint32_t up, uint32_t mid, uint32_t dn)
{
    const uint32_t up_rev = (0x73516240u >> (4u * up)) & 7u; // bit order NE, N, NW = columns x+1, x, x-1
    return (mid >> 2) | (up_rev << 1) | ((mid & 1u) << 4) | (dn << 5);
}
// the start's first neighbour: clockwise from direction `first`, which is known to be background; `first` itself = an isolated pixel
__device__ __forceinline__ int first_neighbour(uint32_t n, int first)
{
    int s = first;
    do {
        s = (s - 1) & 7;
    } while (!((n >> s) & 1u) && s != first);
    return s;
}
// the border's next step: the first occupied neighbour counter-clockwise from direction from + 1
__device__ __forceinline__ int next_dir(uint32_t n, int from)
{
    const uint32_t rot = ((n | (n << 8)) >> (from + 1)) & 0xffu;
    return (from + __ffs((int)rot)) & 7;
}

struct Trace {
    int64_t a00, a10, a01; // Green's-theorem sums over the border polygon (exact)
    double per;            // cv.arcLength of the CHAIN_APPROX_SIMPLE polygon (float32 sqrt per segment, exact sum)
    int npts, steps;       // SIMPLE vertex count, border steps
    int min_fg;            // raster-minimum border pixel
    int min_ebg;           // raster-minimum background pixel right of a border pixel whose East side was examined
    int status;            // 0 ok, 1 aborted (not the raster-first start), 2 step limit
    int bx0, by0, bx1, by1; // bounding box of the border pixels
};

// float32 length of a straight run of k unit steps in direction code s, as cv.arcLength computes it
__device__ __forceinline__ double run_length(int s, int k)
{
    float d = (float)k;
    float q = (s & 1) ? __fadd_rn(__fmul_rn(d, d), __fmul_rn(d, d)) : __fmul_rn(d, d);
    // cv.arcLength takes a correctly rounded float32 square root (sqrtss); the device's float32 root (v_sqrt_f32) is good to 1 ulp
    // only, which showed on diagonal runs of a few lengths (tests/test_gpu_blob.py::test_contours_match_oracle_large_masks).  The
    // FP64 root of the (exact, integer-valued) float32 q, rounded to float32, IS the correctly rounded float32 root: sqrt(q) is never
    // within 2^-26 relative of a float32 midpoint for an integer q, and the FP64 root errs by 2^-53.
    return (double)(float)sqrt((double)q);
}

// reference lib/ImageOperations.py:43-65 for one contour
__device__ void select_contour(ContourRec& r, double min_area, double min_circ)
{
    r.kept = 0; r.cx = r.cy = 0;
    double area = r.area, perimeter = r.perimeter;
    if (perimeter != 0.0) {
        double pi4 = 4 * 3.141592653589793;
        double circ = pi4 * area / (perimeter * perimeter);
        if (circ > min_circ && area > min_area) {
            double a00 = (double)r.a00, a10 = (double)r.a10, a01 = (double)r.a01;
            if (fabs(a00) > 1.1920928955078125e-07) {
                double h = 0.5, s = 0.16666666666666666666666666666667;
                if (a00 < 0) { h = -h; s = -s; }
                double m00 = a00 * h, m10 = a10 * s, m01 = a01 * s;
                if (m00 != 0) {
                    r.kept = 1;
                    r.cx = (int)(m10 / m00);
                    r.cy = (int)(m01 / m00);
                }
            }
        }
    }
}


// which border a finished walk was on: its kind from the orientation (hole borders run the other way round) and its discovery key
__device__ __forceinline__ void link_identity(int64_t a00, int min_fg, int min_ebg, int& key, int& type)
{
    type = a00 > 0 ? 1 : 0;
    key = type ? min_ebg : min_fg;
}

// a border's record from its walk's sums, measured and filtered
__device__ __forceinline__ void make_record(ContourRec& r, int key, int is_hole, int sx, int sy, int npts, int steps, int64_t a00, int64_t a10,
                                            int64_t a01, double per, double min_area, double min_circ)
{
    r.key = key; r.is_hole = is_hole;
    r.sx = sx; r.sy = sy;
    r.npts = npts; r.steps = steps;
    r.a00 = a00; r.a10 = a10; r.a01 = a01;
    r.area = fabs((double)a00 * 0.5);
    r.perimeter = npts > 1 ? per : 0.0;
    r.link = -1; r.parent = -1; r.order = -1;
    select_contour(r, min_area, min_circ);
}

// the small per-border fields the tree phases work on, into slot `slot` of the arrays (LDS in the one-kernel form, ContourWork else)
__device__ __forceinline__ void store_small_fields(int slot, const ContourRec& r, int bx0, int by0, int bx1, int by1, int32_t* rkey, int16_t* rsx,
                                                   int16_t* rsy, uint8_t* rhole, uint8_t* rkept, int16_t (*rbox)[4])
{
    rkey[slot] = r.key; rsx[slot] = (int16_t)r.sx; rsy[slot] = (int16_t)r.sy;
    rhole[slot] = (uint8_t)r.is_hole; rkept[slot] = (uint8_t)r.kept;
    rbox[slot][0] = (int16_t)bx0; rbox[slot][1] = (int16_t)by0;
    rbox[slot][2] = (int16_t)bx1; rbox[slot][3] = (int16_t)by1;
}

// a tile's box (tile_box_pack, kernels.h: .x = the recorded region's columns, .z = the scan box's) as the columns [x0, x1] that can hold
// set pixels or a hole start one column right of them; left as they are when the tile recorded nothing
__device__ __forceinline__ void box_columns(uint4 box, int& x0, int& x1)
{
    const int r0 = span_first(box.x), r1 = span_last(box.x), b0 = span_first(box.z) & ~7, b1 = span_last(box.z) | 7;
    if (r0 <= r1) { x0 = r0 > b0 ? r0 : b0; x1 = (r1 < b1 ? r1 : b1) + 1; }
}

} // namespace

// per-image workspace in global memory (L2-resident): the full border records and the ancestor paths of the kept ones
struct ContourWork {
    ContourRec recs[MAXR];
    int32_t kept_path[MAXK][MAXD];
    // hand-over between the kernels of the split form (candidates -> follow -> tree [-> follow the ambiguous links -> tree])
    int32_t st_ncand;        // candidates of the image, or -1: the candidates kernel reported an error for it
    int32_t st_nrec;         // borders recorded by the follow kernel (atomic)
    int32_t st_err;          // follow kernel: 1 = a walk ran into the step limit
    int32_t st_pending;      // tree kernel, first pass: links left to the second follow pass (0 = the image is finished)
    int32_t rkey[MAXR];
    int16_t rsx[MAXR], rsy[MAXR];
    int16_t rbox[MAXR][4];
    uint8_t rhole[MAXR], rkept[MAXR];
    int16_t rlink[MAXR];     // first tree pass -> second: the links found so far (-2 = waits for its walk)
    int32_t link_key[MAXR];  // second follow pass: discovery key of the border that owns border c's link crack
    uint8_t link_type[MAXR]; //   and its kind (1 = hole border)
};

// One entry of the batch-wide walk lists (64 bits): x | y << 15 | kind << 30 | image << 32 | border << 52.
//   kind 0 / 1: a candidate start of an outer / a hole border at scan position (x, y) (contour_candidates_kernel);
//   kind 2 / 3: the link of border `border` of the image: follow the border through pixel (x, y) whose West (2) / East (3)
//               neighbour is background, to learn which border it is (tree kernel, first pass).
__device__ __forceinline__ uint64_t walk_entry(int image, int x, int y, int kind, int border = 0)
{
    return (uint64_t)(uint32_t)x | ((uint64_t)(uint32_t)y << 15) | ((uint64_t)(uint32_t)kind << 30) | ((uint64_t)(uint32_t)image << 32) |
           ((uint64_t)(uint32_t)border << 52);
}
constexpr int MAX_SPLIT_IMAGES = 1 << 20; // image field of a walk entry

} // namespace mocap
