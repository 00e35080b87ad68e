// blob_setup.hip -- the set-up kernels of the undistort tables and the single-image convenience kernels of the filter stage.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "kernels.h"
#include "filter_dev.h"

namespace mocap {

// ---- map construction: cv::initUndistortRectifyMap as called by cv::undistort (stripe by stripe) -------------
// One thread per image row; the _x accumulation along the row is sequential exactly as in OpenCV.
__global__ void undistort_map_kernel(MapArgs m)
{
    int row = blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= m.H) return;
    int stripe0 = 4096 / (m.W > 1 ? m.W : 1);
    if (stripe0 < 1) stripe0 = 1;
    if (stripe0 > m.H) stripe0 = m.H;
    int ys = (row / stripe0) * stripe0, i = row - ys;
    double A[9];
    for (int k = 0; k < 9; k++) A[k] = m.K[k];
    double fx = A[0], fy = A[4], u0 = A[2], v0 = A[5];
    A[5] = v0 - ys;
    double ir[9];
    {
        double det = A[0] * (A[4] * A[8] - A[5] * A[7]) - A[1] * (A[3] * A[8] - A[5] * A[6]) +
                     A[2] * (A[3] * A[7] - A[4] * A[6]);
        double d = 1.0 / det;
        ir[0] = (A[4] * A[8] - A[5] * A[7]) * d;
        ir[1] = (A[2] * A[7] - A[1] * A[8]) * d;
        ir[2] = (A[1] * A[5] - A[2] * A[4]) * d;
        ir[3] = (A[5] * A[6] - A[3] * A[8]) * d;
        ir[4] = (A[0] * A[8] - A[2] * A[6]) * d;
        ir[5] = (A[2] * A[3] - A[0] * A[5]) * d;
        ir[6] = (A[3] * A[7] - A[4] * A[6]) * d;
        ir[7] = (A[1] * A[6] - A[0] * A[7]) * d;
        ir[8] = (A[0] * A[4] - A[1] * A[3]) * d;
    }
    double k1 = m.dist[0], k2 = m.dist[1], p1 = m.dist[2], p2 = m.dist[3], k3 = m.dist[4];
    double _x = i * ir[1] + ir[2], _y = i * ir[4] + ir[5], _w = i * ir[7] + ir[8];
    uint32_t* out = m.map + (size_t)row * m.W;
    uint32_t* outw = m.mapw + (size_t)row * m.W;
    uint32_t* out4 = m.map4 + (size_t)row * m.W;
    uint32_t flags = 0;
    for (int j = 0; j < m.W; j++, _x += ir[0], _y += ir[3], _w += ir[6]) {
        double w = 1. / _w, x = _x * w, y = _y * w;
        double x2 = x * x, y2 = y * y;
        double r2 = x2 + y2, _2xy = 2 * x * y;
        double kr = (1 + ((k3 * r2 + k2) * r2 + k1) * r2);
        double xd = (x * kr + p1 * _2xy + p2 * (r2 + 2 * x2));
        double yd = (y * kr + p1 * (r2 + 2 * y2) + p2 * _2xy);
        double u = fx * xd + u0;
        double v = fy * yd + v0;
        double ru = __builtin_rint(u * 32), rv = __builtin_rint(v * 32); // round half to even (cvRound)
        // saturate_cast<int>, then the (short) casts of the integer parts that cv::remap's fixed-point map applies
        ru = ru > 2147483647.0 ? 2147483647.0 : (ru < -2147483648.0 ? -2147483648.0 : ru);
        rv = rv > 2147483647.0 ? 2147483647.0 : (rv < -2147483648.0 ? -2147483648.0 : rv);
        int iu = (int)ru, iv = (int)rv;
        int sx = (int)(int16_t)(iu >> 5), sy = (int)(int16_t)(iv >> 5);
        uint32_t a = iu & 31, b = iv & 31;
        // 2x2 tap window clamped into the image; taps that fall outside read 0 (BORDER_CONSTANT): weight 0
        int sxc = sx < 0 ? 0 : (sx > m.W - 2 ? m.W - 2 : sx), syc = sy < 0 ? 0 : (sy > m.H - 2 ? m.H - 2 : sy);
        if (sxc < 0) sxc = 0;
        if (syc < 0) syc = 0;
        int ddx = sx - sxc, ddy = sy - syc;
        uint32_t wx0 = ddx == 0 ? 32u - a : (ddx == -1 ? a : 0u), wx1 = ddx == 0 ? a : (ddx == 1 ? 32u - a : 0u);
        uint32_t wy0 = ddy == 0 ? 32u - b : (ddy == -1 ? b : 0u), wy1 = ddy == 0 ? b : (ddy == 1 ? 32u - b : 0u);
        if (sxc + 1 > m.W - 1) wx1 = 0; // one-column / one-row images: the second tap does not exist
        if (syc + 1 > m.H - 1) wy1 = 0;
        int dx = sxc - j, dy = syc - row; // |.| < 32768 because both ends are inside the image
        uint32_t wq = wx0 | (wx1 << 8) | (wy1 << 16) | (wy0 << 24);
        if (iu != 32 * j || iv != 32 * row) flags |= 1u; // anything but the identity map
        out[j] = ((uint32_t)dx & 0xffffu) | ((uint32_t)dy << 16);
        outw[j] = wq;
        // compact table of the box kernel: unclamped tap origin, limited to [-2, W] x [-2, H] (from there on all four
        // taps lie outside the image and read 0 whatever the fractions are), as 11-bit displacements + 5-bit fractions
        const int sx2 = sx < -2 ? -2 : (sx > m.W ? m.W : sx), sy2 = sy < -2 ? -2 : (sy > m.H ? m.H : sy);
        const int dx4 = sx2 - j, dy4 = sy2 - row;
        if (dx4 < -1024 || dx4 > 1023 || dy4 < -1024 || dy4 > 1023) flags |= 2u;
        out4[j] = ((uint32_t)dx4 & 0x7ffu) | (((uint32_t)dy4 & 0x7ffu) << 11) | (a << 22) | (b << 27);
    }
    if (flags) atomicOr(m.flags, flags);
}

// ---- per compact table: the boxes of source pixels that parts of the output read (TapBox, filter_dev.h) ----------------------
// per 8x8 output cell (the box kernel sums them up over an item's exact region)
__global__ void srcbox_kernel(const uint32_t* __restrict__ map4, ushort4* __restrict__ srcbox, int H, int W)
{
    const int ncx = (W + 7) >> 3, ncy = (H + 7) >> 3;
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= ncx * ncy) return;
    const int cy = c / ncx, cx = c - cy * ncx;
    TapBox b;
    for (int y = 8 * cy; y < 8 * cy + 8 && y < H; y++)
        for (int x = 8 * cx; x < 8 * cx + 8 && x < W; x++) b.add(map4[(size_t)y * W + x], x, y);
    srcbox[c] = b.stored();
}
// per (row, strip): the row's pixels of the strip (columns 240 strip - 8 .. + 255), for the bands of the staged row pipeline
__global__ void rowbox_kernel(const uint32_t* __restrict__ map4, ushort4* __restrict__ rowbox, int H, int W, int n_strips)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= H * n_strips) return;
    const int row = i / n_strips, strip = i - row * n_strips;
    const int xa = strip * 240 - 8 > 0 ? strip * 240 - 8 : 0, xb = strip * 240 + 247 < W - 1 ? strip * 240 + 247 : W - 1;
    TapBox b;
    for (int x = xa; x <= xb; x++) b.add(map4[(size_t)row * W + x], x, row);
    rowbox[i] = b.stored();
}

// ---- stand-alone stages (drop-in surface of lib/CudaOperations.py and lib/ImageOperations.py) ---------------

// fast_cuda_blur: floor(S/c) over the in-bounds taps of a ksize x ksize window
__global__ void box_blur_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int H, int W,
                                int spitch, int dpitch, int ksize)
{
    int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y * blockDim.y + threadIdx.y;
    if (x >= W || y >= H) return;
    int k = ksize / 2;
    int y0 = y - k < 0 ? 0 : y - k, y1 = y + k > H - 1 ? H - 1 : y + k;
    int x0 = x - k < 0 ? 0 : x - k, x1 = x + k > W - 1 ? W - 1 : x + k;
    uint32_t s = 0;
    for (int yy = y0; yy <= y1; yy++)
        for (int xx = x0; xx <= x1; xx++) s += src[(size_t)yy * spitch + xx];
    dst[(size_t)y * dpitch + x] = (uint8_t)(s / (uint32_t)((y1 - y0 + 1) * (x1 - x0 + 1)));
}

// cv.undistort of one image through the packed map
__global__ void undistort_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int H, int W,
                                 int spitch, int dpitch, const uint32_t* __restrict__ map,
                                 const uint32_t* __restrict__ mapw)
{
    int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y * blockDim.y + threadIdx.y;
    if (x >= W || y >= H) return;
    dst[(size_t)y * dpitch + x] = (uint8_t)remap_px(src, spitch, map[(size_t)y * W + x], mapw[(size_t)y * W + x], x, y);
}

// bit mask -> {0,255} image
__global__ void mask_expand_kernel(const uint32_t* __restrict__ mask, int words_per_row, uint8_t* __restrict__ dst,
                                   int H, int W, int dpitch)
{
    int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y * blockDim.y + threadIdx.y;
    if (x >= W || y >= H) return;
    uint32_t w = mask[mask_word_index(y, x >> 5, words_per_row)];
    dst[(size_t)y * dpitch + x] = ((w >> (x & 31)) & 1u) ? 255 : 0;
}

// caller row-major masks [n][H][wpr] <-> the internal 32-row blocks (kernels.h), one thread per word in block order: lane = row
__global__ void mask_convert_kernel(const uint32_t* __restrict__ src, uint32_t* __restrict__ dst, int n_images, int H, int wpr,
                                    int to_blocked)
{
    const size_t image_words = mask_image_words(H, wpr);
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (size_t)n_images * image_words) return;
    const size_t n = t / image_words;
    const uint32_t i = (uint32_t)(t - n * image_words);  // = mask_word_index(y, k, wpr)
    const int y = (int)((i >> 5) / (uint32_t)wpr * 32u + (i & 31u)), k = (int)((i >> 5) % (uint32_t)wpr);
    if (y >= H) return; // padding rows: zero from allocation, never written
    const size_t r = ((size_t)n * H + y) * wpr + k;
    if (to_blocked) dst[t] = src[r];
    else dst[r] = src[t];
}

// image_filter_cpu order: exact 5x5 median (BORDER_REPLICATE) then threshold
__global__ void median5_threshold_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int H, int W,
                                         int spitch, int dpitch, int ithresh, int apply_threshold)
{
    int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y * blockDim.y + threadIdx.y;
    if (x >= W || y >= H) return;
    uint8_t v[25];
    int n = 0;
    for (int dy = -2; dy <= 2; dy++) {
        int yy = y + dy;
        yy = yy < 0 ? 0 : (yy > H - 1 ? H - 1 : yy);
        for (int dx = -2; dx <= 2; dx++) {
            int xx = x + dx;
            xx = xx < 0 ? 0 : (xx > W - 1 ? W - 1 : xx);
            v[n++] = src[(size_t)yy * spitch + xx];
        }
    }
    // median = the value with exactly 12 smaller-or-equal-ranked elements before it (rank by value, then index)
    int med = 0;
    for (int i = 0; i < 25; i++) {
        int rank = 0;
        for (int j = 0; j < 25; j++) rank += (v[j] < v[i]) || (v[j] == v[i] && j < i);
        if (rank == 12) med = v[i];
    }
    dst[(size_t)y * dpitch + x] = apply_threshold ? (med > ithresh ? 255 : 0) : (uint8_t)med;
}

// fast_cuda_demosaic (reference lib/CudaOperations.py:43-100)
__global__ void demosaic_kernel(const uint8_t* __restrict__ bayer, uint8_t* __restrict__ bgr, int H, int W,
                                int spitch)
{
    int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y * blockDim.y + threadIdx.y;
    if (x >= W || y >= H) return;
    auto gp = [&](int xx, int yy) -> int {
        return ((unsigned)xx < (unsigned)W && (unsigned)yy < (unsigned)H) ? (int)bayer[(size_t)yy * spitch + xx] : 0;
    };
    int cross = gp(x - 1, y) + gp(x + 1, y) + gp(x, y - 1) + gp(x, y + 1);
    int diag = gp(x - 1, y - 1) + gp(x + 1, y - 1) + gp(x - 1, y + 1) + gp(x + 1, y + 1);
    int horiz = gp(x - 1, y) + gp(x + 1, y), vert = gp(x, y - 1) + gp(x, y + 1);
    int r, g, b, c = gp(x, y);
    if (!(y & 1) && !(x & 1)) { b = c; g = cross / 4; r = diag / 4; }
    else if (!(y & 1)) { g = c; b = horiz / 2; r = vert / 2; }
    else if (!(x & 1)) { g = c; r = horiz / 2; b = vert / 2; }
    else { r = c; g = cross / 4; b = diag / 4; }
    uint8_t* o = bgr + ((size_t)y * W + x) * 3;
    o[0] = (uint8_t)b; o[1] = (uint8_t)g; o[2] = (uint8_t)r;
}

// total blend weight every source pixel carries over all output pixels (scatter), for the dark-tile bound
__global__ void remap_weight_scatter_kernel(StatArgs a)
{
    int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y * blockDim.y + threadIdx.y;
    if (x >= a.W || y >= a.H) return;
    uint32_t m = a.map[(size_t)y * a.W + x], w = a.mapw[(size_t)y * a.W + x];
    int sx = x + (int)(int16_t)(m & 0xffffu), sy = y + ((int)m >> 16);
    uint32_t wx0 = w & 0xffu, wx1 = (w >> 8) & 0xffu, wy1 = (w >> 16) & 0xffu, wy0 = w >> 24;
    uint32_t* p = a.acc + (size_t)sy * a.W + sx;
    if (wx0 * wy0) atomicAdd(p, wx0 * wy0);
    if (wx1 * wy0) atomicAdd(p + 1, wx1 * wy0);
    if (wx0 * wy1) atomicAdd(p + a.W, wx0 * wy1);
    if (wx1 * wy1) atomicAdd(p + a.W + 1, wx1 * wy1);
    // reach of every 8x8 source cell: the bounding box of the output pixels that read it with a nonzero weight
    const int ncx = (a.W + 7) >> 3;
    auto touch = [&](int tx, int ty) {
        int* r = a.reach + 4 * ((ty >> 3) * ncx + (tx >> 3));
        atomicMin(r, x); atomicMax(r + 1, x); atomicMin(r + 2, y); atomicMax(r + 3, y);
    };
    if (wx0 * wy0) touch(sx, sy);
    if (wx1 * wy0) touch(sx + 1, sy);
    if (wx0 * wy1) touch(sx, sy + 1);
    if (wx1 * wy1) touch(sx + 1, sy + 1);
}
__global__ void remap_stats_kernel(StatArgs a)
{
    int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y * blockDim.y + threadIdx.y;
    if (x >= a.W || y >= a.H) return;
    atomicMax(&a.stats[0], a.acc[(size_t)y * a.W + x]);
    int x0 = 0x7fff, x1 = -1, y0 = 0x7fff, y1 = -1; // extent of the nonzero-weight taps of the 5x5 window around (x,y)
    // windows cut by the image border have fewer than 25 taps, hence a smaller bound: their source cells are marked
    const uint32_t cut = ((x < 2 || x >= a.W - 2) ? 1u : 0u) + ((y < 2 || y >= a.H - 2) ? 1u : 0u); // axes cut: 0, 1, 2
    const int ncx = (a.W + 7) >> 3;
    for (int dy = -2; dy <= 2; dy++)
        for (int dx = -2; dx <= 2; dx++) {
            int xx = x + dx, yy = y + dy;
            if ((unsigned)xx >= (unsigned)a.W || (unsigned)yy >= (unsigned)a.H) continue;
            uint32_t m = a.map[(size_t)yy * a.W + xx], w = a.mapw[(size_t)yy * a.W + xx];
            int sx = xx + (int)(int16_t)(m & 0xffffu), sy = yy + ((int)m >> 16);
            bool c0 = (w & 0xffu) != 0, c1 = ((w >> 8) & 0xffu) != 0, r1 = ((w >> 16) & 0xffu) != 0, r0 = (w >> 24) != 0;
            if ((c0 || c1) && (r0 || r1)) {
                int lo = c0 ? sx : sx + 1, hi = c1 ? sx + 1 : sx, lo2 = r0 ? sy : sy + 1, hi2 = r1 ? sy + 1 : sy;
                x0 = lo < x0 ? lo : x0; x1 = hi > x1 ? hi : x1; y0 = lo2 < y0 ? lo2 : y0; y1 = hi2 > y1 ? hi2 : y1;
                if (cut)
                    for (int cy = lo2 >> 3; cy <= hi2 >> 3; cy++)
                        for (int cx = lo >> 3; cx <= hi >> 3; cx++) atomicOr(&a.edge[cy * ncx + cx], cut);
            }
        }
    if (x1 >= x0) { atomicMax(&a.stats[1], (uint32_t)(x1 - x0 + 1)); atomicMax(&a.stats[2], (uint32_t)(y1 - y0 + 1)); }
}

// ---- launchers -------------------------------------------------------------------------------------------------
static inline dim3 grid2d(int W, int H) { return dim3((W + 63) / 64, (H + 3) / 4); }
void launch_remap_stats(const StatArgs& a, hipStream_t s)
{
    hipLaunchKernelGGL(remap_weight_scatter_kernel, grid2d(a.W, a.H), dim3(64, 4), 0, s, a);
    hipLaunchKernelGGL(remap_stats_kernel, grid2d(a.W, a.H), dim3(64, 4), 0, s, a);
}

void launch_undistort_map(const MapArgs& m, hipStream_t s)
{
    hipLaunchKernelGGL(undistort_map_kernel, dim3((m.H + 63) / 64), dim3(64), 0, s, m);
}
void launch_srcbox(const uint32_t* map4, ushort4* srcbox, int H, int W, hipStream_t s)
{
    const int n = ((W + 7) >> 3) * ((H + 7) >> 3);
    hipLaunchKernelGGL(srcbox_kernel, dim3((n + 63) / 64), dim3(64), 0, s, map4, srcbox, H, W);
}
void launch_rowbox(const uint32_t* map4, ushort4* rowbox, int H, int W, int n_strips, hipStream_t s)
{
    const int n = H * n_strips;
    hipLaunchKernelGGL(rowbox_kernel, dim3((n + 63) / 64), dim3(64), 0, s, map4, rowbox, H, W, n_strips);
}
void launch_box_blur(const uint8_t* src, uint8_t* dst, int H, int W, int sp, int dp, int ksize, hipStream_t s)
{
    hipLaunchKernelGGL(box_blur_kernel, grid2d(W, H), dim3(64, 4), 0, s, src, dst, H, W, sp, dp, ksize);
}
void launch_undistort(const uint8_t* src, uint8_t* dst, int H, int W, int sp, int dp, const uint32_t* map, const uint32_t* mapw,
                      hipStream_t s)
{
    hipLaunchKernelGGL(undistort_kernel, grid2d(W, H), dim3(64, 4), 0, s, src, dst, H, W, sp, dp, map, mapw);
}
void launch_mask_convert(const uint32_t* src, uint32_t* dst, int n_images, int H, int wpr, bool to_blocked, hipStream_t s)
{
    const size_t total = (size_t)n_images * mask_image_words(H, wpr);
    if (!total) return;
    hipLaunchKernelGGL(mask_convert_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, src, dst, n_images, H, wpr,
                       to_blocked ? 1 : 0);
}

void launch_mask_expand(const uint32_t* mask, int wpr, uint8_t* dst, int H, int W, int dp, hipStream_t s)
{
    hipLaunchKernelGGL(mask_expand_kernel, grid2d(W, H), dim3(64, 4), 0, s, mask, wpr, dst, H, W, dp);
}
void launch_median5(const uint8_t* src, uint8_t* dst, int H, int W, int sp, int dp, int ithresh, int apply, hipStream_t s)
{
    hipLaunchKernelGGL(median5_threshold_kernel, grid2d(W, H), dim3(64, 4), 0, s, src, dst, H, W, sp, dp, ithresh, apply);
}
void launch_demosaic(const uint8_t* bayer, uint8_t* bgr, int H, int W, int sp, hipStream_t s)
{
    hipLaunchKernelGGL(demosaic_kernel, grid2d(W, H), dim3(64, 4), 0, s, bayer, bgr, H, W, sp);
}

} // namespace mocap
