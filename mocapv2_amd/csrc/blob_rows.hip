// blob_rows.hip -- the row pipeline of the filter stage (undistort -> 5x5 in-bounds box sum -> threshold -> 5x5 majority).
//
// The stage replaces, for one batch of camera images resident in HBM, the chain
//   cv.undistort (reference lib/ImageOperations.py:38) -> fast_cuda_blur (lib/CudaOperations.py:5-41)
//   -> cv.threshold (lib/ImageOperations.py:29) -> cv.medianBlur (lib/ImageOperations.py:30)
// and writes the filtered binary image as a bit mask (1 bit / pixel).
//
// Here:
//   filter_mask_kernel   the dense form of the filter (every tile, any image size, any lens model; one wave owns
//                        a strip of 256 source columns and slides down its rows, everything in registers: horizontal
//                        neighbours from DPP wave shifts, byte sums from v_dot4_u32_u8, vertical 5-row windows as
//                        running sums whose history sits in a per-wave LDS ring).  Off the hot path: tiny images, tables
//                        the compact format cannot hold, the single-image entry points.  Its list form works through the
//                        wide tiles of the sparse path.
// The rest of the stage: blob_scan.hip (which tiles can be skipped), blob_settle.hip and blob_boxes.hip (the boxes the scan leaves),
// blob_rows_staged.hip (this pipeline on the compact table; rows_dev.h holds what the two share), blob_setup.hip (undistort tables, single-image kernels).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "kernels.h"
#include "rows_dev.h"

namespace mocap {

// LIST: the waves work through the list of wide tiles instead of every tile of every image (rows_wave_items, rows_dev.h).
#ifndef MOCAP_ROWS_WAVES      // (build-time knob for A/B builds: registers of the row pipeline, scratch/build_variant.sh)
#define MOCAP_ROWS_WAVES 1
#endif
template <bool REMAP, bool TINY, bool PIPE, bool LIST>
__global__ __attribute__((amdgpu_waves_per_eu(MOCAP_ROWS_WAVES))) __launch_bounds__(256) void filter_mask_kernel(FilterArgs a)
{
    __shared__ uint32_t lut[256];
    __shared__ uint2 hring[4][8][64];
    __shared__ uint32_t cring[4][8][64];

    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6); // wave-uniform: keeps the row loop scalar

    RowsItem t;
    uint32_t it_first, it_end, it_step;
    if (!rows_wave_items<LIST>(a, wv, t, it_first, it_end, it_step)) return;
    fill_window_counts(lut, lane);
    for (uint32_t it = it_first; it < it_end; it += it_step) {
        if (!rows_item<LIST>(t, it, a.tiles, a.H, a.rows_per_chunk, a.n_strips, a.n_cgroups, a.cam_mod)) continue;
        const int ks = t.ks, ke = t.ke;

        const uint8_t* __restrict__ img = a.src + (size_t)t.image * a.image_stride;
        const uint32_t* __restrict__ map = REMAP ? a.map + (size_t)t.slot * a.H * a.W : nullptr;
        const uint32_t* __restrict__ mapw = REMAP ? a.mapw + (size_t)t.slot * a.H * a.W : nullptr;
        RowTail rt;
        rt.begin(hring[wv], cring[wv], lut, a.mask, a.words_per_row, lane, t, a.H, a.W, a.thr_mul);
        const int xl = rt.xl;
        const LaneCols lc = lane_cols(xl, a.W);
        // source-row queue, 8 deep.  q[3] holds the first row so that the five set-up slides consume q[3..7] and the
        // steady loop starts at q[0] / ring slot 0 with all indices static.
        uint32_t q[8];
        MapSlot mq[4];
        TapSlot tq[4];
        int xq[4];
    #pragma unroll
        // columns the lane's four table words belong to (lanes outside the image read the nearest in-image group:
        // their taps stay inside the image, their result is masked out)
        for (int k = 0; k < 4; k++) xq[k] = lc.addr_x + k;
        const int y0 = t.kfirst - 2;
        if (PIPE) {
            // slot of source row rho = (rho - (y0 + 5)) & 3, so that the steady loop starts at slot 0
            remap_issue_map(mq[3], map, y0, a.H, a.W, lc);
            remap_issue_map(mq[0], map, y0 + 1, a.H, a.W, lc);
            remap_issue_map(mq[1], map, y0 + 2, a.H, a.W, lc);
            remap_issue_map(mq[2], map, y0 + 3, a.H, a.W, lc);
            remap_issue_taps(tq[3], mq[3], img, mapw, a.pitch, a.H, a.W, y0, xq, lc);
            remap_issue_map(mq[3], map, y0 + 4, a.H, a.W, lc);
            remap_issue_taps(tq[0], mq[0], img, mapw, a.pitch, a.H, a.W, y0 + 1, xq, lc);
            remap_issue_map(mq[0], map, y0 + 5, a.H, a.W, lc);
            remap_issue_taps(tq[1], mq[1], img, mapw, a.pitch, a.H, a.W, y0 + 2, xq, lc);
            remap_issue_map(mq[1], map, y0 + 6, a.H, a.W, lc);
            remap_issue_taps(tq[2], mq[2], img, mapw, a.pitch, a.H, a.W, y0 + 3, xq, lc);
            remap_issue_map(mq[2], map, y0 + 7, a.H, a.W, lc);
        } else {
    #pragma unroll
            for (int j = 0; j < 8; j++) q[j] = fetch_src4<REMAP, TINY>(a, img, map, y0 + ((j + 5) & 7), xl, lc);
        }
        // next source row (row index `row`, queue slot J): its four pixels, and the refill of the pipeline behind it
        auto next_row = [&](auto Jc, int row) -> uint32_t {
            constexpr int J = decltype(Jc)::value;
            if (PIPE) {
                constexpr int S = J & 3;
                uint32_t B = remap_combine(tq[S], lc);
                if ((unsigned)row >= (unsigned)a.H) B = 0u; // wave-uniform select: rows outside the image are zero
                remap_issue_taps(tq[S], mq[S], img, mapw, a.pitch, a.H, a.W, row + 4, xq, lc);
                remap_issue_map(mq[S], map, row + 8, a.H, a.W, lc);
                return B;
            }
            uint32_t B = finish_src4<REMAP, TINY>(q[J], (unsigned)row < (unsigned)a.H, lc);
            // refill 8 rows ahead, unconditionally (rows past the chunk are clamped into the image and simply
            // unused: a branch here would make the compiler drain the whole queue at the join)
            q[J] = fetch_src4<REMAP, TINY>(a, img, map, row + 8, xl, lc);
            return B;
        };
        // ---- set-up: source rows kfirst-2 .. kfirst+2 (ring slots 3..7), first threshold row, replicated top rows ----
        rt.hsum_update(next_row(IC<3>{}, y0), 3, 6);
        rt.hsum_update(next_row(IC<4>{}, y0 + 1), 4, 7);
        rt.hsum_update(next_row(IC<5>{}, y0 + 2), 5, 0);
        rt.hsum_update(next_row(IC<6>{}, y0 + 3), 6, 1);
        rt.hsum_update(next_row(IC<7>{}, y0 + 4), 7, 2);
        rt.top(t);

        // ---- steady state: one source row in, one threshold row, one output row per step; unrolled by 8 so that the
        // queue registers and both ring slots are compile-time constants ----
        auto step = [&](auto Jc, int k) { rt.template step<decltype(Jc)::value>(next_row(Jc, k + 2), k); };
        int k = ks;
        for (; k + 7 <= ke; k += 8) { // hot loop: no guards, every index static
            step(IC<0>{}, k);
            step(IC<1>{}, k + 1);
            step(IC<2>{}, k + 2);
            step(IC<3>{}, k + 3);
            step(IC<4>{}, k + 4);
            step(IC<5>{}, k + 5);
            step(IC<6>{}, k + 6);
            step(IC<7>{}, k + 7);
        }
        if (k <= ke) step(IC<0>{}, k);
        if (k + 1 <= ke) step(IC<1>{}, k + 1);
        if (k + 2 <= ke) step(IC<2>{}, k + 2);
        if (k + 3 <= ke) step(IC<3>{}, k + 3);
        if (k + 4 <= ke) step(IC<4>{}, k + 4);
        if (k + 5 <= ke) step(IC<5>{}, k + 5);
        if (k + 6 <= ke) step(IC<6>{}, k + 6);
        rt.template bottom<LIST>(t, a.cells);
    } // strips / list entries
}

// ---- launchers -------------------------------------------------------------------------------------------------
void launch_filter_mask(const FilterArgs& a, bool remap, hipStream_t s)
{
    const int blocks = a.cam_mod * a.n_cgroups * a.n_steps;
    if (remap && a.staged) {
        launch_filter_rows_staged(a, false, blocks, s);
        return;
    }
    if (remap && a.pipelined)
        hipLaunchKernelGGL((filter_mask_kernel<true, false, true, false>), dim3(blocks), dim3(256), 0, s, a);
    else if (remap)
        hipLaunchKernelGGL((filter_mask_kernel<true, false, false, false>), dim3(blocks), dim3(256), 0, s, a);
    else if (a.W >= 4)
        hipLaunchKernelGGL((filter_mask_kernel<false, false, false, false>), dim3(blocks), dim3(256), 0, s, a);
    else
        hipLaunchKernelGGL((filter_mask_kernel<false, true, false, false>), dim3(blocks), dim3(256), 0, s, a);
}

// the same row pipeline over the list of wide tiles (a.tiles / a.n_tiles): a fixed grid, four entries per workgroup at a time
void launch_filter_tiles(const FilterArgs& a, bool remap, int blocks, hipStream_t s)
{
    if (remap && a.staged) {
        launch_filter_rows_staged(a, true, blocks, s);
        return;
    }
    if (remap && a.pipelined)
        hipLaunchKernelGGL((filter_mask_kernel<true, false, true, true>), dim3(blocks), dim3(256), 0, s, a);
    else if (remap)
        hipLaunchKernelGGL((filter_mask_kernel<true, false, false, true>), dim3(blocks), dim3(256), 0, s, a);
    else
        hipLaunchKernelGGL((filter_mask_kernel<false, false, false, true>), dim3(blocks), dim3(256), 0, s, a);
}

} // namespace mocap
