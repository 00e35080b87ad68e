// bayer.h -- the per-site arithmetic of Bayer -> gray (orc_bayer_gray_u8 in oracle/blob_oracle.c), shared by the Bayer pass
// (bayer_gray.hip) and the box kernel's Bayer form (boxes_dev.h: bayer_gray4 / bayer_gray1, used by blob_boxes.hip), so that both form
// every gray value the same way.
// A = any struct with the luma coefficients cb, cg, cr and the shift (BayerArgs, or the box kernel's scalar copy).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mocap {

template <class A>
__device__ __forceinline__ uint32_t luma(int b, int g, int r, const A& a)
{
    return ((uint32_t)b * a.cb + (uint32_t)g * a.cg + (uint32_t)r * a.cr + (1u << (a.shift - 1))) >> a.shift;
}

// colours at a site from its 3x3 neighbourhood (centre c, l/r/u/d, the four diagonals)
template <class A>
__device__ __forceinline__ uint32_t site_gray(int c, int l, int r_, int u, int d, int ul, int ur, int dl, int dr, bool red_row,
                                              bool red_col, const A& a)
{
    const int horiz = (l + r_ + 1) >> 1, vert = (u + d + 1) >> 1;
    const int cross = (l + r_ + u + d + 2) >> 2, diag = (ul + ur + dl + dr + 2) >> 2;
    int r, g, b;
    if (red_row == red_col) { // a red or a blue site
        g = cross;
        r = red_row ? c : diag;
        b = red_row ? diag : c;
    } else {                  // a green site: its row's colour left and right, the other one above and below
        g = c;
        r = red_row ? horiz : vert;
        b = red_row ? vert : horiz;
    }
    return luma(b, g, r, a);
}

// ---- two pixels of one kind at once (16-bit fields of a dword): the fast Bayer kernels' arithmetic ---------------------------
__device__ __forceinline__ uint32_t prm(uint32_t hi, uint32_t lo, uint32_t sel) { return __builtin_amdgcn_perm(hi, lo, sel); }
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t pk_shr(uint32_t v, int n)
{ // both 16-bit fields shifted right on their own (v_pk_lshrrev_b16): nothing leaks from the upper into the lower field
    return __builtin_bit_cast(uint32_t, (u16x2)(__builtin_bit_cast(u16x2, v) >> (unsigned short)n));
}
__device__ __forceinline__ uint32_t mean2(uint32_t a, uint32_t b) { return pk_shr(a + b + 0x00010001u, 1); }
__device__ __forceinline__ uint32_t mean4(uint32_t a, uint32_t b, uint32_t c, uint32_t d) { return pk_shr(a + b + c + d + 0x00020002u, 2); }

// luma of the two pixels held in the 16-bit fields of (x, g, y): x = the row's own colour, y = the other one.
// v_dot2_u32_u16 against (c, 0) / (0, c) picks the field and multiplies in one instruction.
struct LumaCoef { uint32_t xa, ga, ya, xb, gb, yb, half; int shift; };
__device__ __forceinline__ uint32_t dot2(uint32_t v, uint32_t c, uint32_t acc)
{
    return __builtin_amdgcn_udot2(__builtin_bit_cast(u16x2, v), __builtin_bit_cast(u16x2, c), acc, false);
}
__device__ __forceinline__ void luma2(uint32_t x, uint32_t g, uint32_t y, const LumaCoef& k, uint32_t& out_a, uint32_t& out_b)
{
#ifdef BAYER_LUMA_MUL
    out_a = ((x & 0xffffu) * k.xa + ((g & 0xffffu) * k.ga + ((y & 0xffffu) * k.ya + k.half))) >> k.shift;
    out_b = ((x >> 16) * k.xa + ((g >> 16) * k.ga + ((y >> 16) * k.ya + k.half))) >> k.shift;
#else
    out_a = dot2(x, k.xa, dot2(g, k.ga, dot2(y, k.ya, k.half))) >> k.shift;
    out_b = dot2(x, k.xb, dot2(g, k.gb, dot2(y, k.yb, k.half))) >> k.shift;
#endif
}

} // namespace mocap
