// subpixel.hip -- sub-pixel marker centroids: back to the frame bytes around every integer centroid of the contour stage, an
// intensity-weighted centroid over a square window that follows the blob (restated by tests/subpixel_ref.py).
//
// The reference has no counterpart (its centroid is int(M["m10"] / M["m00"]), lib/ImageOperations.py).  All sums are integers, so
// their order cannot matter; the few FP64 operations behind them are rounded one by one (the library is built with
// -ffp-contract=off), so the device equals the restatement bit for bit.
//
// Work decomposition: one workgroup per image.  Its threads first map the image's integer centroids into the raw frame (one
// centroid per thread) and leave the start pixels in LDS, where the NEIGHBOUR test reads them; then its four waves stride over the
// centroids.  A window row (at most 63 pixels) is one wavefront's row: a lane per column, a loop over the rows, the three partial
// sums through a butterfly of shuffles.  No atomics, no scratch memory.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "kernels.h"
#include "bayer.h"
#include "geom_dev.h"

namespace mocap {

namespace {

struct WindowSums { uint32_t S, Sx, Sy; bool edge; };

__device__ __forceinline__ uint32_t wave_add(uint32_t v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o, 64);
    return v;
}

// gray value of a site of a raw Bayer frame: bayer_gray_any_kernel's arithmetic (the frame's border repeats its inner neighbours)
__device__ __forceinline__ int bayer_site(const uint8_t* __restrict__ img, const RefineArgs& a, int x, int y)
{
    const int yc = y < 1 ? 1 : (y > a.H - 2 ? a.H - 2 : y), xc = x < 1 ? 1 : (x > a.W - 2 ? a.W - 2 : x);
    const uint8_t* __restrict__ p = img + (size_t)yc * a.pitch + xc;
    const int sp = a.pitch;
    return (int)site_gray(p[0], p[-1], p[1], p[-sp], p[sp], p[-sp - 1], p[-sp + 1], p[sp - 1], p[sp + 1], (yc & 1) == a.ry, (xc & 1) == a.rx, a);
}

// S, Sx, Sy of the window of radius a.radius around (mx, my), clipped to the image ((mx, my) lies inside it), and whether a pixel
// of the unclipped window's outermost ring carries weight.  Every lane gets the sums.
template <bool BAYER>
__device__ __forceinline__ WindowSums window_sums(const uint8_t* __restrict__ img, const RefineArgs& a, int mx, int my, int lane)
{
    const int r = a.radius;
    const int x0 = mx - r > 0 ? mx - r : 0, x1 = mx + r < a.W - 1 ? mx + r : a.W - 1;
    const int y0 = my - r > 0 ? my - r : 0, y1 = my + r < a.H - 1 ? my + r : a.H - 1;
    const int x = x0 + lane;
    const bool on = x <= x1;
    const int xs = on ? x : x1; // lanes beyond the window read its last column and weigh nothing
    const bool ring_col = x == mx - r || x == mx + r;
    uint32_t s = 0, sy = 0, e = 0;
    // ROWS rows per trip, their loads in flight together (a window is latency, not traffic); rows beyond the window read its last
    // row again and weigh nothing, so there is no remainder loop of single loads.  Measured on the benchmark batch, one box: 4, 8
    // and 16 rows per trip take 0.112, 0.112 and 0.130 ms (16 loads 64 rows for a window of 49 and needs 84 registers).
    constexpr int ROWS = BAYER ? 2 : 8;
    for (int yb = y0; yb <= y1; yb += ROWS) {
        int p[ROWS];
#pragma unroll
        for (int k = 0; k < ROWS; k++) {
            const int y = yb + k < y1 ? yb + k : y1;
            p[k] = BAYER ? bayer_site(img, a, xs, y) : (int)img[(size_t)y * a.pitch + xs];
        }
#pragma unroll
        for (int k = 0; k < ROWS; k++) {
            const int y = yb + k;
            const uint32_t w = (on && y <= y1 && p[k] > a.floor) ? (uint32_t)(p[k] - a.floor) : 0u;
            s += w;
            sy += w * (uint32_t)(y - y0);
            e |= (ring_col || y == my - r || y == my + r) ? w : 0u;
        }
    }
    WindowSums o;
    o.S = wave_add(s);
    o.Sx = wave_add(s * (uint32_t)lane);
    o.Sy = wave_add(sy);
    o.edge = __ballot(e != 0u) != 0ull;
    return o;
}

// floor(v + 0.5) as a pixel index clamped into 0 .. n - 1 (a value that is not a number goes to 0)
__device__ __forceinline__ int start_index(double v, int n)
{
    const double f = floor(v + 0.5);
    return !(f >= 0.0) ? 0 : (f > (double)(n - 1) ? n - 1 : (int)f);
}

} // namespace

__global__ __launch_bounds__(256) void refine_centroids_kernel(RefineArgs a)
{
    __shared__ int s_sx[SUBPIX_MAX_BLOBS], s_sy[SUBPIX_MAX_BLOBS];
    __shared__ double s_u[SUBPIX_MAX_BLOBS], s_v[SUBPIX_MAX_BLOBS];
    const int n = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int cnt = a.count[(long)n * a.count_stride];
    if (cnt <= 0) return; // (the whole workgroup: nothing of this image is written)
    if (cnt > a.max_blobs) cnt = a.max_blobs;
    const double* __restrict__ lens = a.lens + (size_t)(n % a.cam_mod) * SUBPIX_LENS;
    const bool ident = lens[14] != 0.0;
    const int32_t* __restrict__ xy = a.xy + (long)n * a.xy_stride;
    const uint8_t* __restrict__ img = a.src + (size_t)n * a.image_stride;
    const int r = a.radius;

    // ---- start pixels: the integer centroid through the forward lens model, rounded, clamped into the image -------------------
    if (tid < cnt) {
        double U = (double)xy[2 * tid], V = (double)xy[2 * tid + 1];
        if (!ident) distort_pt(lens, lens + 9, U, V);
        s_u[tid] = U; s_v[tid] = V;
        s_sx[tid] = start_index(U, a.W); s_sy[tid] = start_index(V, a.H);
    }
    __syncthreads();

    for (int i = wave; i < cnt; i += 4) { // (wave-uniform)
        int mx = __builtin_amdgcn_readfirstlane(s_sx[i]), my = __builtin_amdgcn_readfirstlane(s_sy[i]);
        uint32_t flags = 0;
        WindowSums w;
        double fx_ = 0.0, fy_ = 0.0;
        for (int it = 0;; it++) {
            w = a.bayer ? window_sums<true>(img, a, mx, my, lane) : window_sums<false>(img, a, mx, my, lane);
            if (w.S == 0u) { flags |= SUBPIX_EMPTY; break; }
            const int x0 = mx - r > 0 ? mx - r : 0, y0 = my - r > 0 ? my - r : 0;
            fx_ = (double)x0 + (double)w.Sx / (double)w.S;
            fy_ = (double)y0 + (double)w.Sy / (double)w.S;
            const int nx = (int)floor(fx_ + 0.5), ny = (int)floor(fy_ + 0.5); // inside the clipped window
            if (nx == mx && ny == my) break;
            if (it + 1 >= a.iters) { flags |= SUBPIX_MOVING; break; }
            mx = nx; my = ny;
        }
        // ---- checks on the last window ------------------------------------------------------------------------------------
        if (w.edge) flags |= SUBPIX_EDGE;
        bool nb = false;
        for (int j = lane; j < cnt; j += 64) {
            const int dx = s_sx[j] - mx, dy = s_sy[j] - my;
            nb |= j != i && dx >= -r && dx <= r && dy >= -r && dy <= r;
        }
        if (__ballot(nb) != 0ull) flags |= SUBPIX_NEIGHBOUR;
        if (mx - r < 0 || mx + r > a.W - 1 || my - r < 0 || my + r > a.H - 1) flags |= SUBPIX_CUT;
        // ---- result: the refined point, or the integer centroid, in the coordinates asked for --------------------------------
        if (lane == 0) {
            double ox, oy;
            if (flags & (SUBPIX_EMPTY | SUBPIX_EDGE | SUBPIX_NEIGHBOUR | SUBPIX_MOVING)) {
                ox = a.coords == 1 ? (double)xy[2 * i] : s_u[i];
                oy = a.coords == 1 ? (double)xy[2 * i + 1] : s_v[i];
            } else {
                ox = fx_; oy = fy_;
                if (a.coords == 1 && !ident) undistort_pt(lens, lens + 9, ox, oy);
            }
            double* __restrict__ o = a.out_xy + (long)n * a.out_xy_stride + 2 * i;
            o[0] = ox; o[1] = oy;
            if (a.out_info) {
                int32_t* __restrict__ q = a.out_info + (long)n * a.out_info_stride + 2 * i;
                q[0] = (int32_t)w.S; q[1] = (int32_t)flags;
            }
        }
    }
}

void launch_refine_centroids(const RefineArgs& a, hipStream_t s)
{
    hipLaunchKernelGGL(refine_centroids_kernel, dim3(a.n_images), dim3(256), 0, s, a);
}

} // namespace mocap
