// filter_dev.h -- device helpers of the filter stage (undistort -> 5x5 in-bounds box sum -> threshold -> 5x5 majority) that
// its kernel files share: blob_rows.hip, blob_rows_staged.hip, blob_boxes.hip, blob_setup.hip -- wave shifts and byte sums, the
// general and the compact undistort table's words, the row pipeline's source fetch, the window-count table.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "kernels.h"

namespace mocap {

__device__ __forceinline__ uint32_t lane_from_prev(uint32_t v)
{ // lane L receives lane L-1's value, lane 0 receives 0
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x138 /*wave_shr:1*/, 0xf, 0xf, true);
}
__device__ __forceinline__ uint32_t lane_from_next(uint32_t v)
{ // lane L receives lane L+1's value, lane 63 receives 0
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x130 /*wave_shl:1*/, 0xf, 0xf, true);
}
__device__ __forceinline__ uint32_t dot4(uint32_t a, uint32_t sel, uint32_t acc)
{
    return __builtin_amdgcn_udot4(a, sel, acc, false);
}

__device__ __forceinline__ uint32_t load_u32(const uint8_t* p)
{ // possibly unaligned 4-byte load (the compiler emits one global_load_dword: unaligned access is enabled on amdhsa)
    uint32_t v;
    __builtin_memcpy(&v, p, 4);
    return v;
}
__device__ __forceinline__ uint32_t load_u16(const uint8_t* p)
{
    uint16_t v;
    __builtin_memcpy(&v, p, 2);
    return v;
}

// One undistorted pixel (cv::remap, INTER_LINEAR, BORDER_CONSTANT 0) from the two set-up tables: `m` places the
// 2x2 tap window (already clamped into the image), `w` holds the four blend weights with border handling baked in
// (a tap outside the image weighs 0).  Taps with zero weight are not read.  General form, used off the hot path.
__device__ __forceinline__ uint32_t remap_px(const uint8_t* __restrict__ img, int pitch, uint32_t m, uint32_t w, int x, int y)
{
    int sx = x + (int)(int16_t)(m & 0xffffu), sy = y + ((int)m >> 16);
    uint32_t wx0 = w & 0xffu, wx1 = (w >> 8) & 0xffu, wy1 = (w >> 16) & 0xffu, wy0 = w >> 24;
    const uint8_t* r = img + (size_t)sy * pitch + sx;
    uint32_t p00 = (wx0 && wy0) ? r[0] : 0u, p01 = (wx1 && wy0) ? r[1] : 0u;
    uint32_t p10 = (wx0 && wy1) ? r[pitch] : 0u, p11 = (wx1 && wy1) ? r[pitch + 1] : 0u;
    uint32_t top = p00 * wx0 + p01 * wx1, bot = p10 * wx0 + p11 * wx1;
    return (top * wy0 + bot * wy1 + 512u) >> 10; // == (sum of 32*w*p + 2^14) >> 15
}

// ---- the compact table's word (BoxArgs::map4), in one place -------------------------------------------------------------------
// dx (11 bits, signed) | dy (11, signed) << 11 | x fraction (5) << 22 | y fraction (5) << 27: the 2x2 taps of pixel (x, y) start at
// (x + dx, y + dy); taps outside the image read 0 (cv::remap's BORDER_CONSTANT).
struct Map4 { int dx, dy; uint32_t fa, fb; };
__device__ __forceinline__ Map4 map4_decode(uint32_t w)
{
    return {(int)(w << 21) >> 21, (int)(w << 10) >> 21, (w >> 22) & 31u, w >> 27};
}
// cv::remap's fixed-point blend of the four taps (p00 p01 / p10 p11)
__device__ __forceinline__ uint32_t map4_blend(const Map4& m, uint32_t p00, uint32_t p01, uint32_t p10, uint32_t p11)
{
    const uint32_t wa = 32u - m.fa, wb = 32u - m.fb;
    const uint32_t top = __umul24(p00, wa) + __umul24(p01, m.fa), bot = __umul24(p10, wa) + __umul24(p11, m.fa);
    return (__umul24(top, wb) + __umul24(bot, m.fb) + 512u) >> 10; // == (sum of 32*w*p + 2^14) >> 15
}
// The pixel whose taps start at (sx, sy), the taps taken from memory: each is loaded from the nearest position inside the image
// and zeroed by select where that is not its own (no branch around loads).  px(x, y) fetches one pixel of the image: a gray byte,
// or a gray value formed from its Bayer neighbourhood.
template <class Px>
__device__ __forceinline__ uint32_t map4_blend_from_memory(const Map4& m, int sx, int sy, int W, int H, Px px)
{
    const int sx0 = sx < 0 ? 0 : (sx > W - 1 ? W - 1 : sx), sx1 = sx + 1 < 0 ? 0 : (sx + 1 > W - 1 ? W - 1 : sx + 1);
    const int sy0 = sy < 0 ? 0 : (sy > H - 1 ? H - 1 : sy), sy1 = sy + 1 < 0 ? 0 : (sy + 1 > H - 1 ? H - 1 : sy + 1);
    const uint32_t t00 = px(sx0, sy0), t01 = px(sx1, sy0), t10 = px(sx0, sy1), t11 = px(sx1, sy1);
    const bool c0 = sx0 == sx, c1 = sx1 == sx + 1, r0 = sy0 == sy, r1 = sy1 == sy + 1;
    return map4_blend(m, (c0 && r0) ? t00 : 0u, (c1 && r0) ? t01 : 0u, (c0 && r1) ? t10 : 0u, (c1 && r1) ? t11 : 0u);
}
// Box of the tap coordinates a set of table words reads (srcbox_kernel, rowbox_kernel): they lie in [-2, W + 1] x [-2, H + 1] and
// are stored + 2.
struct TapBox {
    int x0 = 0x7fff, x1 = -0x8000, y0 = 0x7fff, y1 = -0x8000;
    __device__ __forceinline__ void add(uint32_t w, int x, int y)
    {
        const Map4 m = map4_decode(w);
        const int sx = x + m.dx, sy = y + m.dy;
        x0 = sx < x0 ? sx : x0; x1 = sx + 1 > x1 ? sx + 1 : x1; y0 = sy < y0 ? sy : y0; y1 = sy + 1 > y1 ? sy + 1 : y1;
    }
    __device__ __forceinline__ ushort4 stored() const
    {
        return make_ushort4((unsigned short)(x0 + 2), (unsigned short)(x1 + 2), (unsigned short)(y0 + 2), (unsigned short)(y1 + 2));
    }
};

// per-lane column constants of a 4-pixel group starting at column xl
struct LaneCols {
    int addr_x;        // column actually loaded from: clamp(xl, 0, W-4)
    uint32_t shift;    // bits to shift the loaded dword right so that byte k is column xl+k
    uint32_t bytemask; // 0xff for every byte k with 0 <= xl+k < W
    bool interior;     // all four columns inside the image
};

__device__ __forceinline__ LaneCols lane_cols(int xl, int W)
{
    LaneCols c;
    int ax = xl < 0 ? 0 : (xl > W - 4 ? W - 4 : xl);
    if (ax < 0) ax = 0;
    c.addr_x = ax;
    int sh = (xl - ax) * 8;
    c.shift = sh < 0 ? 0u : (sh > 24 ? 24u : (uint32_t)sh);
    c.bytemask = 0;
#pragma unroll
    for (int k = 0; k < 4; k++)
        if ((unsigned)(xl + k) < (unsigned)W) c.bytemask |= 0xffu << (8 * k);
    c.interior = xl >= 0 && xl + 3 < W;
    return c;
}

// Raw fetch of the four source pixels of a lane (columns xl..xl+3 of row y).  For the plain path the dword is
// returned as loaded (row clamped into the image) and finish_src4 applies the column shift/mask and the row
// validity when the value is consumed, several iterations later, so the load stays in flight meanwhile.
template <bool REMAP, bool TINY>
__device__ __forceinline__ uint32_t fetch_src4(const FilterArgs& a, const uint8_t* __restrict__ img,
                                               const uint32_t* __restrict__ map, int y, int xl, const LaneCols& lc)
{
    const int yc = y < 0 ? 0 : (y > a.H - 1 ? a.H - 1 : y); // y is wave-uniform
    if (REMAP) {
        if ((unsigned)y >= (unsigned)a.H) return 0u;
        uint32_t out = 0;
        const uint32_t* mrow = map + (size_t)yc * a.W;
        const uint32_t* wrow = a.mapw + (map - a.map) + (size_t)yc * a.W;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            int x = xl + k;
            if ((unsigned)x < (unsigned)a.W) out |= remap_px(img, a.pitch, mrow[x], wrow[x], x, yc) << (8 * k);
        }
        return out;
    } else {
        // uniform base + 32-bit offset keeps the scalar-base addressing form (and the global address space:
        // a pointer rebuilt from integers would turn these into flat loads, which vmcnt cannot count in order)
        if (!TINY) return load_u32(img + ((uint32_t)yc * (uint32_t)a.pitch + (uint32_t)lc.addr_x)); // needs W >= 4
        const uint8_t* p = img + (size_t)yc * a.pitch;
        uint32_t v = 0;
#pragma unroll
        for (int k = 0; k < 4; k++)
            if ((unsigned)(xl + k) < (unsigned)a.W) v |= (uint32_t)p[xl + k] << (8 * k);
        return v;
    }
}

template <bool REMAP, bool TINY>
__device__ __forceinline__ uint32_t finish_src4(uint32_t raw, bool row_ok, const LaneCols& lc)
{
    if (REMAP) return raw;
    uint32_t v = TINY ? raw : ((raw >> lc.shift) & lc.bytemask);
    return row_ok ? v : 0u;
}

// ---- software-pipelined remap (three stages, each one source row apart in time) -----------------------------
//   A: issue the load of the row's four packed map words          (8 rows ahead of use)
//   B: decode them, issue the 2x2 tap loads and the weight load    (4 rows ahead of use)
//   C: blend the taps                                             (at use)
// so that neither memory latency is exposed.  Border handling lives in the tables (tap window clamped into the
// image, weights of outside taps zero), so the stages contain no image-edge logic at all.
struct MapSlot { uint4 m; };
struct TapSlot { uint32_t t0[4], t1[4], w[4]; };

__device__ __forceinline__ void remap_issue_map(MapSlot& ms, const uint32_t* __restrict__ map, int row, int H, int W,
                                                const LaneCols& lc)
{
    int rc = row < 0 ? 0 : (row > H - 1 ? H - 1 : row);
    __builtin_memcpy(&ms.m, map + ((uint32_t)rc * (uint32_t)W + (uint32_t)lc.addr_x), 16);
}

__device__ __forceinline__ void remap_issue_taps(TapSlot& ts, const MapSlot& ms, const uint8_t* __restrict__ img,
                                                 const uint32_t* __restrict__ mapw, int pitch, int H, int W, int row,
                                                 const int xq[4], const LaneCols& lc)
{
    // Rows outside the image contribute zeros; their loads are simply those of the nearest row (no branch around
    // loads: the compiler's in-flight counts stay exact) and next_row() discards the result.
    row = row < 0 ? 0 : (row > H - 1 ? H - 1 : row);
    const uint32_t mm[4] = {ms.m.x, ms.m.y, ms.m.z, ms.m.w};
    uint4 wv4;
    __builtin_memcpy(&wv4, mapw + ((uint32_t)row * (uint32_t)W + (uint32_t)lc.addr_x), 16);
    ts.w[0] = wv4.x; ts.w[1] = wv4.y; ts.w[2] = wv4.z; ts.w[3] = wv4.w;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        uint32_t m = mm[k];
        int sx = xq[k] + (int)(int16_t)(m & 0xffffu), sy = row + ((int)m >> 16); // inside the image by construction
        uint32_t off0 = __umul24((uint32_t)sy, (uint32_t)pitch) + (uint32_t)sx, off1 = off0 + (uint32_t)pitch;
        ts.t0[k] = load_u16(img + off0);
        ts.t1[k] = load_u16(img + off1);
    }
}

__device__ __forceinline__ uint32_t remap_combine(const TapSlot& ts, const LaneCols& lc)
{
    uint32_t out = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        uint32_t w = ts.w[k];
        uint32_t top = dot4(ts.t0[k], w, 0u), bot = dot4(ts.t1[k], w, 0u); // tap bytes 2,3 are zero
        uint32_t r = __umul24(top, w >> 24) + 512u;
        r += __umul24(bot, (w >> 16) & 0xffu);
        out |= (r >> 10) << (8 * k);
    }
    return out & lc.bytemask; // columns outside the image do not exist
}

// number of in-image taps of a 5-wide window centred on v
__device__ __forceinline__ int taps5(int v, int n)
{
    int lo = v - 2 < 0 ? 0 : v - 2, hi = v + 2 > n - 1 ? n - 1 : v + 2;
    return hi - lo + 1;
}

template <int J> struct IC { static constexpr int value = J; };

// workgroup -> (camera slot, group of 4 chunks, time step); wave w filters chunk 4 * group + w, strip after strip
struct TileId { int slot, cgroup, image; bool valid; };
__device__ __forceinline__ TileId decode_tile(const FilterArgs& a, int b)
{
    TileId t;
    const int groups = a.cam_mod * a.n_cgroups;
    const int grp = b / a.n_steps, tstep = b - grp * a.n_steps;
    t.slot = grp % a.cam_mod;
    t.cgroup = grp / a.cam_mod;
    t.image = tstep * a.cam_mod + t.slot;
    t.valid = grp < groups && t.image < a.n_images;
    return t;
}

// lut[w]: byte k = number of set bits among bits k..k+4 of the 8-bit window w (the horizontal 5-window counts of four
// neighbouring pixels of a thresholded row).  A wave fills the whole table; where several waves share one they all write it
// (identical values), so no workgroup barrier is needed.
__device__ __forceinline__ void fill_window_counts(uint32_t* lut, int lane)
{
#pragma unroll
    for (int e = 0; e < 4; e++) {
        uint32_t i = (uint32_t)(lane + 64 * e), v = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) v |= (uint32_t)__popc((i >> k) & 0x1fu) << (8 * k);
        lut[i] = v;
    }
}

} // namespace mocap
