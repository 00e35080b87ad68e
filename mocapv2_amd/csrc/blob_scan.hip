// blob_scan.hip -- the streaming scan of the filter stage: which tiles of a batch can hold a set mask pixel at all.
//
//   bright_cells_kernel  streams every frame byte once (the algorithmic HBM traffic of the stage) and records, per
//                        filter tile, which mask rows and columns can possibly hold a set pixel -- an exact bound, see
//                        "dark-tile early-out" below.  The boxes it leaves are filtered by blob_boxes.hip;
//   mark_tiles_kernel    turns the hot map the scan wrote into those boxes.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "kernels.h"
#include "scan_mark.h"

namespace mocap {

// ---- dark-tile early-out ---------------------------------------------------------------------------------------
// A thresholded pixel can only be 1 if its 5x5 box sum reaches thr_mul * taps.  Every undistorted pixel is at most
// (sum of weight * tap + 512) >> 10 with weights summing to <= 1024, so with the excess e(p) = max(0, p - 63) of a source
// pixel p (p <= 63 + e(p)):
//     box sum  <=  taps * 63.5  +  (total of weight * e over the source pixels feeding the window) / 1024
// and a source pixel's total weight over ALL output pixels is at most Wmax (measured on the table at set-up; 1024 for
// the identity).  The taps of one 5x5 window span at most 9 source pixels in x and y (checked at set-up), i.e. they
// lie inside some 2x2 block of 8x8-pixel cells of a fixed grid.  Hence: if no such block of the tile's source region
// has an excess sum E with Wmax * 2E >= 1024 * taps * (2 * thr_mul - 127) (2E <= allow, computed on the host with the
// smallest tap count), every threshold bit of the tile is 0, so is the majority, and the tile's mask rows are zero --
// without running the filter.  The test is made per cell: no cell of the region with 2E above hot = allow / 4.
// (A bound on the excess, not on the number of bright pixels: a background at 100 or the 3x3 halo a demosaiced hot
// pixel leaves costs what it weighs, not 192 per pixel.)  The base 63 of this text is a parameter c (BrightArgs::base,
// chosen on the host from the threshold): with e(p) = max(0, p - c) the bound reads box sum <= taps * (c + 0.5) + ...,
// i.e. Wmax * 2E < 1024 * taps * (2 * thr_mul - 2c - 1); |p - c| + |p - 0| = 2 e(p) + c per byte keeps it at two v_sad_u8
// per dword for any c.
// 16 aligned bytes of a frame for the streaming pass: a non-temporal load (global_load_dwordx4 ... nt).  The pass reads every
// pixel exactly once, so nothing is gained by keeping the lines in L2 / the Infinity Cache, and the streaming policy itself
// is faster: 6.37 GB per launch in 0.946 ms instead of 1.02 ms (6.7 against 6.2 TB/s; A/B on one box, profiles/README.md).
__device__ __forceinline__ uint4 load_once16(const uint8_t* p)
{
    typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
    const u32x4 q = __builtin_nontemporal_load((const u32x4*)p);
    return make_uint4(q.x, q.y, q.z, q.w);
}

// One streaming pass over the frames -- the only time a dark tile's pixels are read.  A thread sums the excess over 63
// of two cells of the fixed 8x8-pixel grid (16 eight-byte loads in flight; consecutive lanes take consecutive cells of
// a cell row, so a wave's loads cover 512 contiguous bytes of each of 8 image rows; two v_sad_u8 per dword).  A cell
// whose doubled excess exceeds `hot` (4 * hot <= allow, so four dark cells can never exceed the 2x2-block bound above;
// `hot_edge` and `hot_corner`, from the bounds of the 15- and 9-tap windows, for the cells that feed windows cut by the image
// border in one axis or in both) marks every filter tile its reach touches (reach = the box of output pixels that read
// the cell, tabulated at set-up, + 4 pixels of blur and median) by widening the tile's record: its range of reachable mask rows
// (atomic min / max) and its mask of reachable quad columns (atomic or; kernels.h: tile_quad_bits).  Tiles left unmarked, and rows
// outside the range, provably filter to zeros.
// WIDE (W, pitch, image stride and base multiples of 16): the two cells of a thread are neighbours in one cell row and
// come in with one 16-byte load per image row (8 loads of 16 B instead of 16 of 8 B per thread).
// FULL (H a multiple of 8, wide only): every cell has its 8 rows, no row clamping and no per-row validity test.
// One block of 256 threads of the pass: block `bx` of image `image` (the kernel below deals these to the workgroups).
template <bool WIDE, bool FULL, bool MAP>
__device__ __forceinline__ void bright_cells_block(const BrightArgs& a, const int bx, const int image)
{
    const int ncx = (a.W + 7) >> 3, ncy = (a.H + 7) >> 3, n = ncx * ncy;
    const uint8_t* __restrict__ img = a.src + (size_t)image * a.image_stride;
    uint2 v[2][8];
    int ci[2], cr[2];
    uint32_t sh[2];
    bool in_range[2];
    if (WIDE) {
        const int half = ncx >> 1, np = half * ncy; // cell pairs (ncx is even)
        int p = bx * 256 + threadIdx.x;
        in_range[0] = in_range[1] = p < np;
        p = p < np ? p : np - 1; // threads past the end recount the last pair (and mark the same tiles again)
        const int row = (int)__umulhi((uint32_t)p, a.ncx_magic), cxp = p - row * half; // ncx_magic: for ncx / 2 here
        cr[0] = cr[1] = row;
        ci[0] = row * ncx + 2 * cxp; ci[1] = ci[0] + 1;
        sh[0] = sh[1] = 0;
        if (FULL) {
            const uint32_t off0 = (uint32_t)(8 * row) * (uint32_t)a.pitch + 16u * (uint32_t)cxp;
#pragma unroll
            for (int j = 0; j < 8; j++) {
                const uint4 q = load_once16(img + (off0 + (uint32_t)(j * a.pitch))); // uniform base + 32-bit offset
                v[0][j] = make_uint2(q.x, q.y); v[1][j] = make_uint2(q.z, q.w);
            }
        } else {
#pragma unroll
            for (int j = 0; j < 8; j++) {
                int r = 8 * row + j;
                r = r < a.H ? r : a.H - 1;
                const uint4 q = load_once16(img + ((uint32_t)r * (uint32_t)a.pitch + 16u * (uint32_t)cxp));
                v[0][j] = make_uint2(q.x, q.y); v[1][j] = make_uint2(q.z, q.w);
            }
        }
    } else {
        const int i0 = bx * 512 + threadIdx.x;
#pragma unroll
        for (int u = 0; u < 2; u++) {
            int i = i0 + 256 * u;
            in_range[u] = i < n;
            i = i < n ? i : n - 1; // threads past the end recount the last cell (and mark the same tiles again)
            ci[u] = i;
            cr[u] = a.ncx_magic ? (int)__umulhi((uint32_t)i, a.ncx_magic) : i / ncx; // floor(i / ncx) without the division
            const int cx = i - cr[u] * ncx;
            const int c = 8 * cx, cc = c < a.W - 8 ? c : a.W - 8; // W >= 8 (checked on the host)
            sh[u] = (uint32_t)(8 * (c - cc));
#pragma unroll
            for (int j = 0; j < 8; j++) {
                int r = 8 * cr[u] + j;
                r = r < a.H ? r : a.H - 1;
                __builtin_memcpy(&v[u][j], img + ((uint32_t)r * (uint32_t)a.pitch + (uint32_t)cc), 8);
            }
        }
    }
    const int slot = image % a.cam_mod;
    const uint2* __restrict__ reach = a.reach + (size_t)slot * n;
    const uint8_t* __restrict__ cflags = a.cflags + (size_t)slot * n;
    uint32_t* __restrict__ rec = a.tile_rows + (size_t)image * a.n_chunks * a.n_strips * 4;
    const uint32_t base4 = (uint32_t)a.base * 0x01010101u, c8 = 8u * (uint32_t)a.base;
    uint32_t level[2] = {0u, 0u}, sum[2];
#pragma unroll
    for (int u = 0; u < 2; u++) {
        uint32_t acc = 0;
#pragma unroll
        for (int j = 0; j < 8; j++) {
            if (WIDE) { // cells are whole
                const uint32_t e2 = excess2_row(v[u][j].x, v[u][j].y, base4, c8);
                if (FULL || 8 * cr[u] + j < a.H) acc += e2;
            } else {
                uint64_t vv = (((uint64_t)v[u][j].y << 32) | v[u][j].x) >> sh[u]; // drops the bytes left of the cell at the right edge
                const uint32_t e2 = excess2_row((uint32_t)vv, (uint32_t)(vv >> 32), base4, c8);
                if (8 * cr[u] + j < a.H) acc += e2;
            }
        }
        if (MAP) level[u] = in_range[u] ? hot_level(a, acc) : 0u;
        sum[u] = acc;
        if (a.probe && (image & 15) == 0) { // wave-uniform, rare: which base would leave fewer hot cells?
            const uint32_t alt4 = (uint32_t)a.base_alt * 0x01010101u, alt8 = 8u * (uint32_t)a.base_alt;
            uint32_t acc2 = 0;
#pragma unroll
            for (int j = 0; j < 8; j++) {
                const uint64_t vv = WIDE ? (((uint64_t)v[u][j].y << 32) | v[u][j].x) : ((((uint64_t)v[u][j].y << 32) | v[u][j].x) >> sh[u]);
                const uint32_t e2 = excess2_row((uint32_t)vv, (uint32_t)(vv >> 32), alt4, alt8);
                if (FULL || 8 * cr[u] + j < a.H) acc2 += e2;
            }
            const int n_cur = __popcll(__ballot((int)acc > a.hot)), n_alt = __popcll(__ballot((int)acc2 > a.hot_alt));
            if ((threadIdx.x & 63) == 0) {
                atomicAdd(&a.probe[PROBE_STRIDE * (bx & 127)], (uint32_t)n_cur);
                atomicAdd(&a.probe[PROBE_STRIDE * (bx & 127) + 1], (uint32_t)n_alt);
            }
        }
    }
    // (the hot cells mark their tiles once both sums stand: the frame bytes need no registers beside that rare path's)
    if (!MAP) {
        mark_hot_cell(a, reach, cflags, rec, ci[0], sum[0]);
        mark_hot_cell(a, reach, cflags, rec, ci[1], sum[1]);
    }
    if (MAP) {
        // The hot map: two bits per cell in cell order, so the 128 cells of a wave are 8 whole words (WIDE: consecutive lanes hold
        // consecutive cell pairs) or two runs of 4 (lanes hold cells i and i + 256).  The lanes sharing a word OR their fields
        // together with DPP moves and one of them stores it if it is not zero (the map is all zeros between batches: mark_tiles_kernel
        // clears what it reads) -- no atomics, and a wave without a hot cell, the usual one, issues no memory operation behind its
        // frame loads at all (a store per wave, tried first, made every wave wait for it at its end: 0.99 against 0.95 ms).
        const int lane = threadIdx.x & 63;
        uint32_t* __restrict__ hm = a.hotmap + (size_t)image * a.hot_words;
        if (WIDE) {
            uint32_t w = (level[0] | (level[1] << 2)) << (4 * (lane & 7));
            w |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)w, 0xB1 /*quad_perm 1,0,3,2*/, 0xf, 0xf, true);
            w |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)w, 0x4E /*quad_perm 2,3,0,1*/, 0xf, 0xf, true);
            w |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)w, 0x141 /*row_half_mirror*/, 0xf, 0xf, true);
            if ((lane & 7) == 0 && w != 0u) hm[(bx * 256 + (int)threadIdx.x) >> 3] = w;
        } else {
#pragma unroll
            for (int u = 0; u < 2; u++) {
                uint32_t w = level[u] << (2 * (lane & 15));
                w |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)w, 0xB1, 0xf, 0xf, true);
                w |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)w, 0x4E, 0xf, 0xf, true);
                w |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)w, 0x141, 0xf, 0xf, true);
                w |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)w, 0x140 /*row_mirror*/, 0xf, 0xf, true);
                if ((lane & 15) == 0 && w != 0u) hm[(bx * 512 + (int)threadIdx.x + 256 * u) >> 4] = w;
            }
        }
    }
}

// The hot map of the scan -> tile boxes.  One thread per map word (16 cells); a wave collects its hot cells in a list in LDS
// and works through it one cell per lane: reach and flags of the cell (the tables of the image's undistort slot), the
// threshold its flags ask for, and the boxes of the tiles it reaches -- what the scan used to do behind its own loads, where
// every hot wave then sat through two dependent round trips with no frame loads in flight (0.946 ms for the benchmark batch
// at 8 markers per frame, 1.133 at 32: most scan waves carry a hot cell then).
// The hot cells of a marker lie in the same few waves and reach the same one or two tiles, and a memory atomic costs what
// it costs whether it changes anything or not (the first version issued four per hot cell and tile: 4 M of them per batch
// at 8 markers, 0.29 ms; 0.89 ms at 32): the wave first merges its cells' rectangles, rows and quad columns (tile_quad_bits), per tile in
// a 32-entry table in LDS (tag = tile; a collision goes to memory directly) and then widens each tile it touched once.
__global__ __launch_bounds__(256) void mark_tiles_kernel(BrightArgs a)
{
    __shared__ uint16_t s_list[4][1024];
    __shared__ uint32_t s_tab[4][32][5]; // tile | first row | last row | quad mask, low word | high word
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    // a wave takes 256 consecutive words (4 per lane) of one image at a time; with a fixed grid (a few workgroups per CU) the
    // waves go on to further pieces: few workgroups to place beside another batch's scan, which holds every wave slot of the chip
    const int wpi = (a.hot_words + 255) >> 8; // pieces per image
    const int n_cells = ((a.W + 7) >> 3) * ((a.H + 7) >> 3);
    for (long long piece = (long long)blockIdx.x * 4 + wv; piece < (long long)wpi * a.n_images; piece += (long long)gridDim.x * 4) {
    const int image = (int)(piece / wpi), wave_word0 = (int)(piece - (long long)image * wpi) * 256;
    uint32_t* __restrict__ hm = a.hotmap + (size_t)image * a.hot_words;
    uint32_t wk[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int wi = wave_word0 + 64 * k + lane;
        wk[k] = wi < a.hot_words ? hm[wi] : 0u;
    }
    if (__ballot((wk[0] | wk[1] | wk[2] | wk[3]) != 0u) == 0ull) continue;
#pragma unroll
    for (int k = 0; k < 4; k++)
        if (wk[k] != 0u) hm[wave_word0 + 64 * k + lane] = 0u; // the map is all zeros again for the next batch's scan
    uint32_t (*tab)[5] = s_tab[wv];
    if (lane < 32) { tab[lane][0] = 0xffffffffu; tab[lane][1] = 0xffffffffu; tab[lane][2] = 0u; tab[lane][3] = 0u; tab[lane][4] = 0u; }
    const int slot = image % a.cam_mod;
    const uint2* __restrict__ reach = a.reach + (size_t)slot * n_cells;
    const uint8_t* __restrict__ cflags = a.cflags + (size_t)slot * n_cells;
    uint32_t* __restrict__ rec = a.tile_rows + (size_t)image * a.n_chunks * a.n_strips * 4;
    // widen one tile's record in memory (one 16-byte load; a word that already holds its part of the rectangle needs no atomic)
    auto widen = [&](int t, uint32_t ya, uint32_t yb, uint32_t mlo, uint32_t mhi) __attribute__((always_inline)) {
        const uint4 cur = *(const uint4*)(rec + 4 * t);
        if (cur.x > ya) atomicMin(&rec[4 * t], ya);
        if (cur.y < yb) atomicMax(&rec[4 * t + 1], yb);
        if ((cur.z & mlo) != mlo) atomicOr(&rec[4 * t + 2], mlo);
        if ((cur.w & mhi) != mhi) atomicOr(&rec[4 * t + 3], mhi);
    };
#pragma unroll 1
    for (int k = 0; k < 4; k++) {
        const uint32_t w = k == 0 ? wk[0] : (k == 1 ? wk[1] : (k == 2 ? wk[2] : wk[3]));
        const uint32_t nz = (w | (w >> 1)) & 0x55555555u; // bit 2j: cell j of the word exceeds at least the lowest threshold
        const int cnt = __popc(nz);
        if (__ballot(cnt != 0) == 0ull) continue;
        const int word0 = wave_word0 + 64 * k;
        int incl = cnt; // inclusive prefix sum over the wave
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int o = __shfl_up(incl, d);
            if (lane >= d) incl += o;
        }
        const int total = __builtin_amdgcn_readlane(incl, 63);
        int at = incl - cnt;
        for (uint32_t m = nz; m; m &= m - 1) {
            const int j2 = __ffs((int)m) - 1; // = 2 j
            s_list[wv][at++] = (uint16_t)((lane << 6) | (j2 << 1) | ((w >> j2) & 3u)); // lane | cell of the word | level
        }
        __builtin_amdgcn_s_waitcnt(0xc07f); // lgkmcnt(0): list and table are written (one wave: no barrier needed)
        __builtin_amdgcn_wave_barrier();
        for (int e0 = 0; e0 < total; e0 += 64) {
            const int e = e0 + lane;
            if (e < total) {
                const uint32_t v = s_list[wv][e];
                const int ci = 16 * (word0 + (int)(v >> 6)) + (int)((v >> 2) & 15u);
                if (ci < n_cells) {
                    const uint2 rc = reach[ci];
                    const int x0 = (int)(rc.x & 0xffffu), x1 = (int)(rc.x >> 16), y0 = (int)(rc.y & 0xffffu), y1 = (int)(rc.y >> 16);
                    if (x0 <= x1 && level_is_hot(v & 3u, cflags[ci])) {
                        // (the rectangle and the tiles it overlaps: as widen_tile_boxes, scan_mark.h)
                        const int xa = x0 - 4 > 0 ? x0 - 4 : 0, xb = x1 + 4 < a.W - 1 ? x1 + 4 : a.W - 1;
                        const int ya = y0 - 4 > 0 ? y0 - 4 : 0, yb = y1 + 4 < a.H - 1 ? y1 + 4 : a.H - 1;
                        const int ch0 = (int)(((uint32_t)ya * a.rows_magic) >> 23), ch1 = (int)(((uint32_t)yb * a.rows_magic) >> 23);
                        const int st0 = (int)(((uint32_t)xa * 34953u) >> 23), st1 = (int)(((uint32_t)xb * 34953u) >> 23);
                        for (int ch = ch0; ch <= ch1; ch++)
                            for (int st = st0; st <= st1; st++) {
                                const int t = ch * a.n_strips + st, q = t & 31;
                                const uint64_t m = tile_quad_bits(st, xa, xb);
                                const uint32_t mlo = (uint32_t)m, mhi = (uint32_t)(m >> 32);
                                const uint32_t old = atomicCAS(&tab[q][0], 0xffffffffu, (uint32_t)t);
                                if (old == 0xffffffffu || old == (uint32_t)t) {
                                    atomicMin(&tab[q][1], (uint32_t)ya); atomicMax(&tab[q][2], (uint32_t)yb);
                                    if (mlo) atomicOr(&tab[q][3], mlo);
                                    if (mhi) atomicOr(&tab[q][4], mhi);
                                } else
                                    widen(t, (uint32_t)ya, (uint32_t)yb, mlo, mhi);
                            }
                    }
                }
            }
        }
        __builtin_amdgcn_s_waitcnt(0xc07f);
        __builtin_amdgcn_wave_barrier(); // (the list is rewritten by the next k)
    }
    if (lane < 32 && tab[lane][0] != 0xffffffffu) widen((int)tab[lane][0], tab[lane][1], tab[lane][2], tab[lane][3], tab[lane][4]);
    __builtin_amdgcn_s_waitcnt(0xc07f);
    __builtin_amdgcn_wave_barrier(); // (the table is initialised anew for the wave's next piece)
    }
}

// The grid is one-dimensional: workgroup b takes the blocks b, b + gridDim.x, ... of the batch's blocks_x * n_images blocks
// (block -> image = block / blocks_x).  Launched with as many workgroups as blocks it is the plain form (every workgroup one
// block); launched with a fixed number per CU it is a persistent pass that never holds more than that many wave slots and
// registers of a SIMD, whatever the batch size (BrightArgs::blocks_x, launch_bright_cells).
// MAP: the hot cells go into the hot map (BrightArgs::hotmap) instead of marking their tiles from here.
template <bool WIDE, bool FULL = false, bool MAP = true>
__global__ __launch_bounds__(256) void bright_cells_kernel(BrightArgs a)
{
    if (a.prio == 1) __builtin_amdgcn_s_setprio(1);
    else if (a.prio == 2) __builtin_amdgcn_s_setprio(2);
    else if (a.prio == 3) __builtin_amdgcn_s_setprio(3);
    const uint32_t total = (uint32_t)a.blocks_x * (uint32_t)a.slice_images;
    if (a.zero_counters && blockIdx.x == 0) a.zero_counters[threadIdx.x] = 0u; // the counter block of the kernels behind this one
    if (a.block_ctr == nullptr) {
        for (uint32_t vb = blockIdx.x; vb < total; vb += gridDim.x) {
            const uint32_t image = vb / (uint32_t)a.blocks_x;
            bright_cells_block<WIDE, FULL, MAP>(a, (int)(vb - image * (uint32_t)a.blocks_x), a.image0 + (int)image);
        }
    } else {
        // persistent form: the workgroups take the blocks in the order of a shared counter, as the hardware dispatcher would hand
        // them out -- the blocks in flight stay one contiguous window of the frames (a fixed stride per workgroup lets them drift
        // apart: 1.20 ms against 0.95 at the same occupancy); the next index is fetched while this block's loads are in flight
        __shared__ uint32_t s_next[2];
        constexpr uint32_t CH = 16; // blocks per visit of the counter (one atomic per block would serialise on it: 2.4 ms)
        uint32_t v0 = blockIdx.x * CH;
        for (int it = 0; v0 < total; it++) {
            if (threadIdx.x == 0) s_next[it & 1] = gridDim.x * CH + atomicAdd(a.block_ctr, CH);
            for (uint32_t vb = v0; vb < v0 + CH && vb < total; vb++) {
                const uint32_t image = vb / (uint32_t)a.blocks_x;
                bright_cells_block<WIDE, FULL, MAP>(a, (int)(vb - image * (uint32_t)a.blocks_x), a.image0 + (int)image);
            }
            __syncthreads();
            v0 = s_next[it & 1];
        }
    }
    if (a.mask_words) {
        // caller-owned masks: clear them on the side (16 bytes per thread and round), the filter kernel then only
        // writes the tiles it filters.  The context's own mask needs no clearing (see the filter kernel).
        const size_t nthreads = (size_t)gridDim.x * 256;
        const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
        if (a.mask_aligned16) {
            const size_t quads = a.mask_words >> 2;
            for (size_t q = g; q < quads; q += nthreads) ((uint4*)a.mask)[q] = make_uint4(0u, 0u, 0u, 0u);
            if (g < (a.mask_words & 3)) a.mask[(quads << 2) + g] = 0u;
        } else {
            for (size_t q = g; q < a.mask_words; q += nthreads) a.mask[q] = 0u;
        }
    }
}

// ---- launchers -------------------------------------------------------------------------------------------------
void launch_bright_cells(const BrightArgs& a_, hipStream_t s)
{
    BrightArgs a = a_;
    const int n = ((a.W + 7) >> 3) * ((a.H + 7) >> 3);
    a.blocks_x = a.wide ? (n / 2 + 255) / 256 : (n + 511) / 512;
    // The pass goes out as `slices` launches over consecutive runs of images (1 = one launch).  Between two slices the stream's
    // queue has a kernel boundary: while a slice drains, the short kernels of the other batches in flight get the registers and
    // wave slots that the pass, with its hundreds of thousands of ready workgroups, otherwise holds until its last block.
    const int slices = a.slices > 1 ? (a.slices < a.n_images ? a.slices : a.n_images) : 1;
    const int per = (a.n_images + slices - 1) / slices;
    const size_t mask_words = a.mask_words;
    for (int i0 = 0; i0 < a.n_images; i0 += per) {
        a.image0 = i0;
        a.slice_images = a.n_images - i0 < per ? a.n_images - i0 : per;
        a.mask_words = i0 == 0 ? mask_words : 0; // (the side job of clearing caller-owned masks goes with the first slice)
        const long long total = (long long)a.blocks_x * a.slice_images;
        long long grid = total;
        uint32_t* const ctr = a_.block_ctr;
        a.block_ctr = nullptr;
        if (a.max_blocks > 0 && a.max_blocks < grid) { // persistent form: a fixed number of workgroups
            grid = a.max_blocks;
            a.block_ctr = ctr ? ctr + (i0 / per) : nullptr; // one counter per slice (zeroed by the caller)
        }
        if (grid > 0x7fffffffLL) grid = 0x7fffffffLL;
        const dim3 g((unsigned)grid), b(256);
        if (a.hotmap) {
            if (a.wide && a.H % 8 == 0) hipLaunchKernelGGL((bright_cells_kernel<true, true, true>), g, b, 0, s, a);
            else if (a.wide) hipLaunchKernelGGL((bright_cells_kernel<true, false, true>), g, b, 0, s, a);
            else hipLaunchKernelGGL((bright_cells_kernel<false, false, true>), g, b, 0, s, a);
        } else {
            if (a.wide && a.H % 8 == 0) hipLaunchKernelGGL((bright_cells_kernel<true, true, false>), g, b, 0, s, a);
            else if (a.wide) hipLaunchKernelGGL((bright_cells_kernel<true, false, false>), g, b, 0, s, a);
            else hipLaunchKernelGGL((bright_cells_kernel<false, false, false>), g, b, 0, s, a);
        }
    }
}
int hot_map_words(int H, int W, int wide)
{ // whole waves of the scan write the map: 32 words per block of 256 threads (128 cells per wave either way)
    const int n = ((W + 7) >> 3) * ((H + 7) >> 3);
    return 32 * (wide ? (n / 2 + 255) / 256 : (n + 511) / 512);
}
void launch_mark_tiles(const BrightArgs& a, hipStream_t s)
{
    long long grid = ((long long)((a.hot_words + 255) >> 8) * a.n_images + 3) / 4; // one piece per wave ...
    if (a.mark_grid > 0 && a.mark_grid < grid) grid = a.mark_grid;                  // ... or a fixed grid whose waves loop
    hipLaunchKernelGGL(mark_tiles_kernel, dim3((unsigned)grid), dim3(256), 0, s, a);
}

} // namespace mocap
