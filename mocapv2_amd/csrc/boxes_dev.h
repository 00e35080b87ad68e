// boxes_dev.h -- device helpers of the box kernel (blob_boxes.hip): small integer helpers, the gray values it forms from raw Bayer
// frames, the geometry of one work item and the box of source pixels the item reads.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "kernels.h"
#include "bayer.h"
#include "filter_dev.h"

namespace mocap {

namespace {

__device__ __forceinline__ int imin(int a, int b) { return a < b ? a : b; }
__device__ __forceinline__ int imax(int a, int b) { return a > b ? a : b; }

// ---- gray values formed from raw Bayer frames (box_filter_kernel<true>) ------------------------------------------------------
// gray(x, y) = site_gray at (clamp(x, 1, W-2), clamp(y, 1, H-2)) -- the arithmetic of orc_bayer_gray_u8 / bayer_gray_any_kernel --
// so that the 3x3 Bayer neighbourhood always lies in the image.  Needs W >= 8, H >= 3.
struct BayerK { int ry, rx; uint32_t cb, cg, cr; int shift; }; // wave-uniform (plain scalars: no struct in scratch)

// The three Bayer rows around row y that the gray quad at columns x..x+3 reads (x % 4 == 0, 0 <= x <= W - 4, W % 4 == 0 and
// 16-byte aligned rows: true on the gray-less path): per row the aligned dwords at x - 4, x and x + 4 (clamped into the row; a
// clamped word is only read for a column whose gray value is replaced by its inner neighbour's).
struct BayerWin { uint32_t w[9]; };
__device__ __forceinline__ void bayer_win_load(BayerWin& b, const uint8_t* __restrict__ img, int pitch, int W, int H, int x, int y)
{
    const int yc = y < 1 ? 1 : (y > H - 2 ? H - 2 : y);
    const uint32_t xl = (uint32_t)imax(x - 4, 0), xr = (uint32_t)imin(x + 4, W - 4);
#pragma unroll
    for (int r = 0; r < 3; r++) {
        const uint32_t o = (uint32_t)(yc - 1 + r) * (uint32_t)pitch;
        b.w[3 * r] = *(const uint32_t*)(img + o + xl);
        b.w[3 * r + 1] = *(const uint32_t*)(img + o + (uint32_t)x);
        b.w[3 * r + 2] = *(const uint32_t*)(img + o + xr);
    }
}
// the gray quad from its window, two pixels of one kind at a time as in bayer_gray_kernel (16-bit fields: e = columns x, x+2,
// o = x+1, x+3, Le / Ro their outer neighbours).  The lanes of a staging round lie in different rows, so which of e / o holds the
// colour sites is a per-lane select of operands (Pc / Pg: colour / green sites, Lx / Rx their left / right neighbours).  Column 0
// repeats column 1, column W - 1 repeats column W - 2.
__device__ __forceinline__ uint32_t bayer_gray4(const BayerWin& b, int W, int H, int x, int y, const BayerK& k)
{
    const int yc = y < 1 ? 1 : (y > H - 2 ? H - 2 : y);
    const bool red_row = (yc & 1) == k.ry;
    const bool eic = (red_row ? k.rx : 1 - k.rx) == 0; // the row's red / blue sites sit on even columns
    uint32_t Pc[3], Lc[3], Rc[3], Pg[3];
    uint32_t Lg = 0, Rg = 0;
#pragma unroll
    for (int r = 0; r < 3; r++) {
        const uint32_t pw = b.w[3 * r], w = b.w[3 * r + 1], nw = b.w[3 * r + 2];
        const uint32_t e = prm(0, w, 0x0c020c00u), o = prm(0, w, 0x0c030c01u);
        const uint32_t Le = prm(pw, w, 0x0c010c07u), Ro = prm(nw, w, 0x0c040c02u);
        Pc[r] = eic ? e : o; Lc[r] = eic ? Le : e; Rc[r] = eic ? o : Ro; Pg[r] = eic ? o : e;
        if (r == 1) { Lg = eic ? e : Le; Rg = eic ? Ro : o; }
    }
    const uint32_t cx = red_row ? k.cr : k.cb, cy = red_row ? k.cb : k.cr;
    const LumaCoef kc{cx, k.cg, cy, cx << 16, k.cg << 16, cy << 16, 1u << (k.shift - 1), k.shift};
    uint32_t ca, cb, ga, gb;
    // colour sites: own value, green from the cross, the other colour from the diagonals
    luma2(Pc[1], mean4(Lc[1], Rc[1], Pc[0], Pc[2]), mean4(Lc[0], Rc[0], Lc[2], Rc[2]), kc, ca, cb);
    // green sites: the row's colour left and right, the other one above and below
    luma2(mean2(Lg, Rg), Pg[1], mean2(Pg[0], Pg[2]), kc, ga, gb);
    uint32_t g0 = eic ? ca : ga, g1 = eic ? ga : ca, g2 = eic ? cb : gb, g3 = eic ? gb : cb;
    if (x == 0) g0 = g1;
    if (x + 3 == W - 1) g3 = g2;
    return g0 | (g1 << 8) | (g2 << 16) | (g3 << 24);
}
// one gray value (0 <= x < W, 0 <= y < H) from its nine Bayer bytes in memory (the taps-from-memory path: rare, only correct)
__device__ __forceinline__ uint32_t bayer_gray1(const uint8_t* __restrict__ img, int pitch, int W, int H, int x, int y, const BayerK& k)
{
    const int yc = y < 1 ? 1 : (y > H - 2 ? H - 2 : y), xc = x < 1 ? 1 : (x > W - 2 ? W - 2 : x);
    const uint32_t c = (uint32_t)yc * (uint32_t)pitch + (uint32_t)xc, u = c - (uint32_t)pitch, d = c + (uint32_t)pitch; // 32-bit offsets
    return site_gray(img[c], img[c - 1], img[c + 1], img[u], img[d], img[u - 1], img[u + 1], img[d - 1], img[d + 1], (yc & 1) == k.ry,
                     (xc & 1) == k.rx, k);
}

// ---- one work item -----------------------------------------------------------------------------------------------------------
// Geometry of one item (all wave-uniform):
//   output region   columns [ox0, ox1] (ox0 a multiple of 8), rows [oy0, oy1]
//   threshold rows  [ty0, ty1] = [oy0 - 2, oy1 + 2] clipped to the image (the median replicates the border rows)
//   patch           columns [px0, px0 + 4 Q) with px0 = ox0 - 4, Q = 2 * bytes + 2 quads; rows [hy0, hy1] = [ty0 - 2, ty1 + 2]
//   exact region    the patch pixels inside the scan's box and the image; every other patch pixel counts as 0, which is
//                   exact for the mask (blob_scan.hip, "dark-tile early-out")
struct BoxGeom { // derived from an item header, wave-uniform
    int image, tile, slot, remap;
    int ox0, ox1, oy0, oy1, Q, px0, ty0, ty1, hy0, hy1, PR, ey0, ey1, eq0, eq1;
    bool valid, exact;
};
__device__ __forceinline__ BoxGeom box_geometry(int H, int W, int cam_mod, uint64_t remap_bits, const BoxItem& it)
{
    const uint4 h0 = it.head, h1 = it.box;
    BoxGeom g;
    g.image = uni((int)h0.x); g.tile = uni((int)h0.y);
    g.ox0 = uni(span_first(h0.z)); g.ox1 = uni(span_last(h0.z)); g.oy0 = uni(span_first(h0.w)); g.oy1 = uni(span_last(h0.w));
    const int bx0 = uni(span_first(h1.x)), bx1 = uni(span_last(h1.x)), by0 = uni(span_first(h1.y)), by1 = uni(span_last(h1.y));
    g.valid = g.ox0 <= g.ox1 && g.oy0 <= g.oy1;
    g.slot = g.image % cam_mod;
    g.remap = (int)((remap_bits >> g.slot) & 1ull);
    const int nb = (g.ox1 - g.ox0 + 8) >> 3;
    g.Q = 2 * nb + 2; g.px0 = g.ox0 - 4;
    g.ty0 = imax(g.oy0 - 2, 0); g.ty1 = imin(g.oy1 + 2, H - 1);
    g.hy0 = g.ty0 - 2; g.hy1 = g.ty1 + 2; g.PR = g.hy1 - g.hy0 + 1;
    g.ey0 = imax(imax(by0, g.hy0), 0); g.ey1 = imin(imin(by1, g.hy1), H - 1);
    g.eq0 = imax((imax(bx0, 0) - g.px0) >> 2, 0); g.eq1 = imin((imin(bx1, W - 1) - g.px0) >> 2, g.Q - 1);
    g.exact = g.valid && g.ey0 <= g.ey1 && g.eq0 <= g.eq1;
    return g;
}
// per-lane partial of the box of source pixels the exact region of `g` reads (union of the per-cell boxes); the caller
// reduces it over the wave when it needs it, so that the loads stay in flight meanwhile
struct SrcBounds { int xa, xb, ya, yb; };
__device__ __forceinline__ SrcBounds source_bounds_partial(const ushort4* __restrict__ srcbox, int H, int W, const BoxGeom& g, int lane)
{
    SrcBounds b{0x7fff, -0x8000, 0x7fff, -0x8000};
    if (!g.exact || !g.remap) return b;
    const int ncx8 = (W + 7) >> 3;
    const ushort4* __restrict__ sbx = srcbox + (size_t)g.slot * ncx8 * ((H + 7) >> 3);
    const int cx0 = imax(g.px0 + 4 * g.eq0, 0) >> 3, cx1 = imin(g.px0 + 4 * g.eq1 + 3, W - 1) >> 3, cy0 = g.ey0 >> 3, cy1 = g.ey1 >> 3;
    const int ncw = cx1 - cx0 + 1, ncells = ncw * (cy1 - cy0 + 1);
    const float rcpw = __builtin_amdgcn_rcpf((float)ncw);
    for (int c0 = 0; c0 < ncells; c0 += 64) {
        const int c = imin(c0 + lane, ncells - 1);
        const int cyi = small_div(c, rcpw), cxi = c - cyi * ncw;
        const ushort4 sb = sbx[(cy0 + cyi) * ncx8 + cx0 + cxi];
        b.xa = imin(b.xa, (int)sb.x - 2); b.xb = imax(b.xb, (int)sb.y - 2); b.ya = imin(b.ya, (int)sb.z - 2); b.yb = imax(b.yb, (int)sb.w - 2);
    }
    return b;
}

} // namespace

} // namespace mocap
