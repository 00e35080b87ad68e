// kernels.h -- internal launch interface between the C-ABI (abi_*.hip) and the HIP kernels, and the records the kernels of the
// filter stage pass between them (mask layout, spans, work items, wide-tile entries, the tiles' regions).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mocap {

// The bit masks the kernels pass between them are stored in blocks of 32 rows: word k of row y (bit b = pixel 32k + b) sits
// at word ((y >> 5) * wpr + k) * 32 + (y & 31) of its image, so one 128-byte line holds one word column of 32 rows (32 x 32
// pixels).  Every consumer works on 2-D neighbourhoods some 50-64 pixels across (contour windows, blob boxes, cleared regions):
// a 64 x 64 window is at most 3 x 3 lines, a lane-per-row load of 64 rows touches 2-3 lines.  An image takes
// mask_image_words(H, wpr) words, H padded up to a multiple of 32; the padding rows are zero from allocation and never written.
// (The C-ABI's caller-owned masks stay row-major: abi_blob.hip converts at the boundary.)
__host__ __device__ __forceinline__ uint32_t mask_word_index(int y, int k, int wpr)
{
    return ((uint32_t)(y >> 5) * (uint32_t)wpr + (uint32_t)k) * 32u + (uint32_t)(y & 31);
}
// byte b of row y (pixels 8b .. 8b + 7), for the byte-granular writers
__host__ __device__ __forceinline__ uint32_t mask_byte_index(int y, int b, int wpr)
{
    return mask_word_index(y, b >> 2, wpr) * 4u + (uint32_t)(b & 3);
}
__host__ __device__ __forceinline__ size_t mask_image_words(int H, int wpr) { return (size_t)((H + 31) >> 5) * 32 * (size_t)wpr; }

// a value every lane of the wave holds, moved to scalar registers: addresses formed from it are scalar, loops over it uniform
__device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ unsigned long long uni64(unsigned long long v)
{
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v), hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
    return (unsigned long long)hi << 32 | lo;
}

// floor(n / d) for 0 <= n < 4096, 1 <= d <= 4096 from d's float reciprocal (+0.5 keeps every quotient away from an integer)
__device__ __forceinline__ int small_div(int n, float rcp_d) { return (int)(((float)n + 0.5f) * rcp_d); }

// Sums with a fixed order, for results that must have the same bits on every run (no floating-point atomics): the lanes of a
// wave by shuffles (offsets 32 .. 1; lane 0 holds the sum) ...
__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}
// ... and the 256 threads of a workgroup: wave_sum, then the four waves in order through LDS.  Every thread calls it; every
// thread gets the sum.
__device__ __forceinline__ double block_sum(double v, double* s_part /*[4]*/)
{
    v = wave_sum(v);
    __syncthreads(); // the previous round's readers are done with s_part
    if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = v;
    __syncthreads();
    return (s_part[0] + s_part[1]) + (s_part[2] + s_part[3]);
}

void launch_mask_convert(const uint32_t* src, uint32_t* dst, int n_images, int H, int wpr, bool to_blocked, hipStream_t s);

// The dense filter kernel (any geometry, any lens model): every tile of every image, the undistortion as a gather in the
// row pipeline.  Used when every tile has to be filtered anyway (early-out off or not provable), for images narrower than
// 8 pixels, for undistort tables whose displacements do not fit the compact table of the box kernel, and by the
// single-image convenience entry points.
struct FilterArgs {
    const uint8_t* src;   // images, image_stride bytes apart, rows `pitch` bytes apart
    size_t image_stride;
    int pitch, H, W;
    uint32_t* mask;       // [n_images][mask_image_words(H, words_per_row)] in 32-row blocks (see mask_word_index)
    int words_per_row;
    uint32_t* cells;      // [n_images][n_cgroups*4][n_strips]: bit g = rows 8g..8g+7 of the chunk have set pixels in the strip; bit 31 = tile ran the full filter
    // undistort tables of the first slot used (remap variant only), each [cam_mod][H][W]:
    const uint32_t* map;  //   tap position: (sx - x) | (sy - y) << 16, the 2x2 tap window clamped into the image
    const uint32_t* mapw; //   blend weights 32*(wx0 | wx1<<8 | wy1<<16 | wy0<<24)/32, taps outside the image weigh 0
    const uint4* tiles; const uint32_t* n_tiles; uint32_t cap_tiles; // list form (launch_filter_tiles): entries image, tile (chunk *
                          //   n_strips + strip), first row, last row; their number
    int pipelined;        // 1 = software-pipelined gather (table words 8 rows ahead, taps 4 rows ahead; W % 4 == 0, H >= 2), 0 = per-pixel gather
    int cam_mod;          // undistort slot of image n = n % cam_mod (map already points at the first slot)
    int n_images, n_steps; // n_steps = ceil(n_images / cam_mod)
    int thr_mul;          // floor(thresh)+1: blurred > thresh  <=>  S >= thr_mul * taps
    int rows_per_chunk, n_strips, n_cgroups;
    // the staged form of the row pipeline (filter_rows_staged_kernel): compact table, source pixels through LDS
    int staged = 0;       // 1 = use it (remap variant; W % 16 == 0, H >= 2, every slot's table compact)
    const uint32_t* map4 = nullptr; // compact table of the first slot used (see BoxArgs)
    const ushort4* rowbox = nullptr; // [cam_mod][H][n_strips]: per row and strip, the box of tap coordinates the strip's pixels read, + 2
    int stage_dw = 0;         // dwords of LDS a band's source rectangle may take (ROWS_STAGE_DW; smaller values are a test switch)
};
void launch_rowbox(const uint32_t* map4, ushort4* rowbox, int H, int W, int n_strips, hipStream_t s); // (blob_setup.hip)
int rows_stage_dwords();
// (blob_rows_staged.hip; launch_filter_mask / launch_filter_tiles go through it when a.staged is set)
void launch_filter_rows_staged(const FilterArgs& a, bool list, int blocks, hipStream_t s);

// Bayer -> gray (bayer_gray.hip): red sites at row parity ry / column parity rx, luma coefficients cb, cg, cr >> shift
struct BayerArgs {
    const uint8_t* src; uint8_t* dst;
    int H, W, n_images;
    long spitch, dpitch;
    size_t sstride, dstride;
    int ry, rx;
    uint32_t cb, cg, cr;
    int shift;
};

// The sparse half of the filter stage: tiles, boxes, work items.
// A tile = 240 mask columns x rows_per_chunk rows.  The scan kernel leaves per tile the box of mask rows / columns that
// hot cells can reach (tile_rows); settle_tiles_kernel (blob_settle.hip) turns the boxes into items; box_filter_kernel
// (blob_boxes.hip, its device helpers in boxes_dev.h) consumes them.
#ifndef MOCAP_BOX_HCAP         // (build-time knobs for A/B builds, scratch/build_variant.sh)
#define MOCAP_BOX_HCAP 1536
#define MOCAP_BOX_SCAP 6656
#define MOCAP_BOX_MAX_PARTS 4
#endif
constexpr int BOX_HCAP = MOCAP_BOX_HCAP; // quad-rows (4 pixels x 1 row) of one item's patch (halving it for twice the waves per CU: 0.63 against 0.53 ms)
constexpr int BOX_SCAP = MOCAP_BOX_SCAP; // bytes of source pixels staged in LDS per item (>= (BOX_HCAP + 64) * 4: the counts alias it)
constexpr int BOX_MAX_PARTS = MOCAP_BOX_MAX_PARTS;  // items a tile is cut into at most (a whole 240 x 68 tile: 2 x 2)
constexpr int SPLIT_COUNTER = 12;                   // word of the counter block (BoxArgs::n_items) that counts the split tiles of a batch
// The span records settle writes and the box kernel, the row pipeline's list form and the contour stage read: a closed range
// [a, b] of columns or rows in one word, a | b << 16 (a > b: empty).
__host__ __device__ __forceinline__ uint32_t span_pack(int a, int b) { return (uint32_t)a | ((uint32_t)b << 16); }
__host__ __device__ __forceinline__ int span_first(uint32_t s) { return (int)(s & 0xffffu); }
__host__ __device__ __forceinline__ int span_last(uint32_t s) { return (int)(s >> 16); }
// A tile's record of the scan (BoxArgs::tile_rows): .x / .y the first / last mask row some hot cell's rectangle reaches, .z / .w the low
// and high word of the tile's quad mask.  Bit q (0..61) of the mask: a rectangle overlaps the 4-pixel quad column 240 st - 4 + 4 q .. + 3
// of strip st -- the window [240 st - 4, 240 st + 243], the tile and the 4 pixels a patch reaches beyond it on either side, which is all
// of a rectangle's column extent that a consumer of the tile looks at, and none looks at it more finely than a quad.  Not marked:
// (0xffffffff, 0, 0, 0), first row > last row.
// the quads of strip st that the columns [xa, xb] overlap (the caller has found that they overlap the strip)
__host__ __device__ __forceinline__ uint64_t tile_quad_bits(int st, int xa, int xb)
{
    const int base = 240 * st - 4;
    const int qa = xa > base ? (xa - base) >> 2 : 0, qb = xb - base < 248 ? (xb - base) >> 2 : 61;
    return (2ull << qb) - (1ull << qa);
}
// first and last marked column of the mask `m` (not 0) of strip st, clamped into the image (quad 0 of strip 0 lies left of it)
__host__ __device__ __forceinline__ void tile_quad_columns(int st, uint64_t m, int W, int& x0, int& x1)
{
    const uint32_t lo = (uint32_t)m, hi = (uint32_t)(m >> 32);
#if defined(__HIP_DEVICE_COMPILE__)
    const int q0 = lo ? __ffs((int)lo) - 1 : 31 + __ffs((int)hi), q1 = hi ? 63 - __clz((int)hi) : 31 - __clz((int)lo);
#else
    const int q0 = lo ? __builtin_ctz(lo) : 32 + __builtin_ctz(hi), q1 = hi ? 63 - __builtin_clz(hi) : 31 - __builtin_clz(lo);
#endif
    const int base = 240 * st - 4, a = base + 4 * q0, b = base + 4 * q1 + 3;
    x0 = a > 0 ? a : 0; x1 = b < W - 1 ? b : W - 1;
}
// the mask byte columns of the strip that the marked quads overlap: bit b (0..29, columns 240 st + 8 b .. + 7) = quads 2 b + 1, 2 b + 2
__host__ __device__ __forceinline__ uint32_t tile_quad_bytes(uint64_t m)
{
    uint64_t v = ((m | (m >> 1)) >> 1) & 0x0555555555555555ull; // bit 2 b = quad 2 b + 1 or 2 b + 2; the even bits are pressed together
    v = (v | (v >> 1)) & 0x3333333333333333ull;
    v = (v | (v >> 2)) & 0x0f0f0f0f0f0f0f0full;
    v = (v | (v >> 4)) & 0x00ff00ff00ff00ffull;
    v = (v | (v >> 8)) & 0x0000ffff0000ffffull;
    v = (v | (v >> 16)) & 0x00000000ffffffffull;
    return (uint32_t)v;
}

// One work item of the box kernel, moved as its two 16-byte halves.  head: image, tile (chunk * n_strips + strip), the output region's
// columns and rows as spans (an empty part of a split: columns 1 > 0, the consumer skips it); box: the columns and rows of the scan's
// box the item takes its exact pixels from (not clipped to the tile), two words of padding.
struct BoxItem {
    uint4 head, box;
    static __device__ __forceinline__ BoxItem make(int image, int tile, int x0, int x1, int y0, int y1, int bx0, int bx1, int by0, int by1)
    {
        const bool empty = x0 > x1 || y0 > y1;
        return {make_uint4((uint32_t)image, (uint32_t)tile, empty ? 1u : span_pack(x0, x1), span_pack(y0, y1)),
                make_uint4(span_pack(bx0, bx1), span_pack(by0, by1), 0u, 0u)};
    }
};
static_assert(sizeof(BoxItem) == 32, "two 16-byte halves");
// A tile's record in BoxArgs::cur_box: .x / .y the columns / rows of its output region of this batch (what the mask may hold
// there; empty = none), .z / .w those of the scan's box (not clipped to the tile).
__host__ __device__ __forceinline__ uint4 tile_box_pack(uint32_t out_x, uint32_t out_y, int bx0, int bx1, int by0, int by1)
{
    return make_uint4(out_x, out_y, span_pack(bx0, bx1), span_pack(by0, by1));
}
// An entry of the wide-tile list (BoxArgs::wide_tiles = FilterArgs::tiles): image, tile, rows [y0, y1]; a band without rows
// (y0 > y1) is stored as [y0, y0 - 1] and skipped by the row pipeline.
struct WideTile { int image, tile, y0, y1; };
__host__ __device__ __forceinline__ uint4 wide_tile_pack(int image, int tile, int y0, int y1)
{
    return make_uint4((uint32_t)image, (uint32_t)tile, (uint32_t)y0, (uint32_t)(y0 <= y1 ? y1 : y0 - 1));
}
__host__ __device__ __forceinline__ WideTile wide_tile_unpack(uint4 e) { return {(int)e.x, (int)e.y, (int)e.z, (int)e.w}; }

struct BoxArgs {
    const uint8_t* src; size_t image_stride; int pitch, H, W;
    uint32_t* mask; int words_per_row; // [n_images][mask_image_words(H, words_per_row)] in 32-row blocks (see mask_word_index)
    uint32_t* cells;            // occupancy words [n_images][n_chunks][n_strips] (see FilterArgs)
    const uint32_t* map4;       // compact undistort table of the first slot used, [cam_mod][H][W]: dx (11 bits, signed) |
                                //   dy (11, signed) << 11 | x fraction (5) << 22 | y fraction (5) << 27; the 2x2 taps start at
                                //   (x + dx, y + dy), clamped into [-2, W] x [-2, H] (taps outside the image read 0)
    const ushort4* srcbox;      // [cam_mod][ceil(H/8)][ceil(W/8)]: box of the tap coordinates of an 8x8 output cell, + 2
    uint64_t remap_bits;        // bit s: slot s (relative to the first) is remapped (else the identity)
    int cam_mod, n_images, n_steps;
    int thr_mul;
    int rows_per_chunk, n_strips, n_chunks;
    uint32_t* tile_rows;        // [n_images][n_chunks][n_strips][4]: the scan's records of this batch (first / last row, the quad mask's two
                                //   words: tile_quad_bits; (0xffffffff, 0, 0, 0) = none), read-only for settle
    uint32_t* tile_rows_next;   // the same array for the next batch (the two alternate): emptied by settle
    int wide_split;             // 1 = a wide tile whose byte columns (tile_quad_bytes) have gaps is cut into one set of items per run of columns (the host decides: tuning.def)
    int n_clear;                // images whose boxes tile_rows_next may still hold (an earlier, larger batch): emptied too
    int cluster;                // 1 = a box spanning tiles that all hold it becomes one item (A/B switch)
    uint32_t* cur_box;          // [n_images][n_chunks][n_strips][4]: words 0-1 the tile's output region of this batch
                                //   (x0 | x1 << 16, y0 | y1 << 16; x0 > x1 = none) = what the mask may hold there; words 2-3 the
                                //   scan's box (not clipped to the tile)
    BoxItem* items; uint32_t* n_items; uint32_t cap_items; // n_items[0] = items in the list; n_items[16 + 16 x] = head of run x (box kernel);
                                //   n_items[SPLIT_COUNTER] = wide tiles cut at their column gaps
    uint64_t* timing;           // optional [grid][6] phase clock of the box kernel (MOCAP_BOX_TIMING=1, a debugging aid), else null
    int prio;                   // 1 = raise the wave priority of the box kernel (A/B switch)
    int stage_bytes;            // LDS bytes the source staging may use (BOX_SCAP; smaller values are a test switch)
    uint4* wide_tiles;          // tiles whose box is wider than `wide_quads` patch quads go to this list instead (image, tile, first row,
                                //   last row; counted in n_items[8]) and through the sliding row pipeline of filter_mask_kernel, which
                                //   does less work per pixel on wide regions than the box kernel
    uint32_t cap_wide; int wide_quads_remap, wide_quads_identity, wide_bands;
    uint32_t* zero8;            // not null: 8 words (the contour stage's walk counters) that settle zeroes -- in place of a fill launch
    int dense;                  // 1 = no early-out: every tile is filtered whole
    int ext_mask;               // 1 = caller-owned mask (cleared by the scan kernel, or written whole when dense)
    // gray-less Bayer input (box_filter_kernel<true>): src / pitch / image_stride are the raw Bayer frames', the kernel forms
    // every gray value it reads from their 3x3 neighbourhood (bayer.src / dst are not used; W % 16 == 0, H >= 8)
    BayerArgs bayer;
};
void launch_settle_tiles(const BoxArgs& a, hipStream_t s);                              // blob_settle.hip
void launch_box_filter(const BoxArgs& a, int grid, hipStream_t s, bool bayer = false); // blob_boxes.hip
int box_filter_blocks_per_cu();
void launch_srcbox(const uint32_t* map4, ushort4* srcbox, int H, int W, hipStream_t s); // blob_setup.hip

struct MapArgs {
    double K[9], dist[5];
    int H, W;
    uint32_t* map;   // [H][W] tap positions (see FilterArgs)
    uint32_t* mapw;  // [H][W] blend weights
    uint32_t* map4;  // [H][W] compact table (see BoxArgs)
    uint32_t* flags; // bit0: the table is not the identity; bit1: a displacement does not fit the compact table
};

// one border found by the contour kernel (also the debug record compared with the oracle in tests)
struct ContourRec {
    int32_t key;       // raster index (y*(W+1)+x) of the scan position that discovers the border
    int32_t is_hole;
    int32_t sx, sy;    // first border pixel
    int32_t npts;      // CHAIN_APPROX_SIMPLE vertex count
    int32_t steps;
    int64_t a00, a10, a01;
    double area, perimeter;
    int32_t kept, cx, cy;
    int32_t link;      // rec index of the border owning the crack left of the start (-1 frame), see kernel
    int32_t parent;    // rec index of the parent border, -1 = frame
    int32_t order;     // position among the kept contours in cv.findContours order, -1 if not kept
};

struct ContourArgs {
    const uint32_t* mask;  // [n_images][mask_image_words(H, words_per_row)] in 32-row blocks (see mask_word_index)
    int words_per_row, H, W, n_images;
    int32_t* out_xy;     // image n: out_xy + n*xy_stride, [max_blobs][2]
    int32_t* out_count;  // image n: out_count[n*count_stride]; may exceed max_blobs (truncated), <0 = error
    long xy_stride, count_stride;
    int max_blobs;
    double min_area, min_circ;
    ContourRec* dbg;     // optional [n_images][dbg_cap]
    int32_t* dbg_count;  // optional [n_images]
    int dbg_cap;
    int max_steps;
    const uint32_t* cells; // occupancy written by the filter kernel (see FilterArgs), or null = scan every row
    const uint32_t* boxes; // with cells: per tile [4] the output region and the scan's box (BoxArgs::cur_box), or null = whole strips
    int rows_per_chunk, n_chunks, n_strips;
    uint64_t* timing;      // optional [n_images][8] phase clock (debugging aid), else null
    void* work;            // [n_images] per-image workspace of contour_work_bytes() each
    int prio;              // wave priority (s_setprio 0..3): the walks are serial chains, cheap to favour and costly to delay
    uint64_t* walk_list;   // split form: [n_images * contour_walk_bytes() / 8] candidate walks of the batch (contours_dev.h: walk_entry), or
                           //   null = one kernel per image
    uint64_t* link_list;   // split form: [n_images * contour_link_bytes() / 8] link walks of the batch (second follow pass)
    uint32_t* walk_count;  // split form: [8] entries in walk_list, its head, entries in link_list, its head, entries in wait_list
                           //   (zeroed by launch_contours)
    uint32_t* wait_list;   // split form: [n_images] the images the first tree pass left to the second one
    int follow_grid;       // split form: workgroups (waves) of the follow kernel
    int follow_grid2;      //   ... of its second pass (the link walks: few)
    int counters_zeroed;   // split form: 1 = walk_count was zeroed by an earlier kernel of the stream (settle): no fill launch
    int defer_links;       // split form: 1 = links only a walk can settle go through a second follow + tree pass (two more launches);
                           //   0 = the first tree pass walks them in place (one wave per link) and the second passes are not launched
    int image_grid;        // split form: > 0 = the per-image kernels (candidates, tree) as that many workgroups looping over the images
    int follow_list;       // set by launch_contours: 0 = the follow kernel works through walk_list, 1 = through link_list
    int tree_pass;         // set by launch_contours: 1 / 2 = first / second pass of the tree kernel
    uint64_t* follow_dbg;  // optional [follow_grid][8] phase clock of the follow kernel (follow_timing = 1: first pass, 2: second), else null
    int follow_dbg_list;
};

enum { BLOB_ERR_CANDIDATES = -2, BLOB_ERR_CONTOURS = -3, BLOB_ERR_STEPS = -4, BLOB_ERR_DEPTH = -5 };

void launch_filter_mask(const FilterArgs& a, bool remap, hipStream_t s);
void launch_filter_tiles(const FilterArgs& a, bool remap, int blocks, hipStream_t s);
constexpr int PROBE_STRIDE = 32; // words between two pairs of probe counters: a cache line each
struct BrightArgs {
    const uint8_t* src; size_t image_stride; int pitch, H, W, n_images; // W >= 8
    int cam_mod;                  // undistort slot of image n = n % cam_mod (the tables already point at the first slot)
    uint32_t ncx_magic;           // ceil(2^32 / d), d = ceil(W/8) (wide: d / 2), if that divides every index exactly by multiply-high, else 0
    int wide;                     // 1 = 16-byte loads (W, pitch, image stride, base all multiples of 16; ncx_magic != 0)
    int base;                     // excess base c: a pixel p counts with max(0, p - c)
    int hot, hot_edge, hot_corner; // a cell whose doubled excess sum (2 * sum of max(0, p - c)) exceeds this is hot (4 * hot <= allow); _edge /
                                  //   _corner for cells feeding windows the image border cuts in one axis / in both
    const uint2* reach;           // [cam_mod][cells]: box of the output pixels that read the 8x8 source cell, x0 | x1 << 16, y0 | y1 << 16
    const uint8_t* cflags;        // [cam_mod][cells]: 1 / 2 = the cell feeds windows the image border cuts in one axis / in both
    uint32_t* tile_rows; int n_chunks, n_strips; uint32_t rows_magic; // reachable mask rows / quad columns per tile, see BoxArgs;
                                  //   rows_magic = ceil(2^23 / rows per chunk)
    uint32_t* mask; size_t mask_words; int mask_aligned16; // caller-owned bit masks to clear on the side (mask_words = 0: none)
    // probe (optional): on every 16th image also count the cells that are hot under the current base and under the alternative
    // base `base_alt` / threshold `hot_alt`, into probe[PROBE_STRIDE * (block & 127) + 0 / 1]: the host compares the sums and switches
    uint32_t* probe; int base_alt, hot_alt;
    int prio;                     // wave priority of the scan (s_setprio): its few instructions are loads that keep HBM busy
    int max_blocks;               // > 0: launch at most this many workgroups, each looping over the batch's blocks (persistent form)
    uint32_t* block_ctr;          // persistent form: [slices] zeroed counters the workgroups take their blocks from (else null: fixed stride)
    int blocks_x;                 // blocks of 256 threads per image (set by launch_bright_cells)
    int slices;                   // > 1: the pass goes out as that many launches over consecutive runs of images
    int image0, slice_images;     // set by launch_bright_cells: the images of this launch
    uint32_t* hotmap;             // [n_images][hot_words]: two bits per source cell, cell i of an image at bits 2 (i % 16) of word i / 16: how
                                  //   many of the thresholds hot_corner <= hot_edge <= hot its sum exceeds.  All zeros between batches: the scan
                                  //   stores the words that are not zero, mark_tiles_kernel reads and clears them.  null = the scan marks the tiles itself
    int hot_words;                // words per image: hot_map_words(H, W, wide)
    uint32_t* zero_counters;      // not null: 256 words (the context's counter block) that workgroup 0 of the scan zeroes -- in place of a fill launch
    int mark_grid;                // > 0: workgroups of mark_tiles_kernel (its waves loop over the map); 0 = one piece per wave
};
int hot_map_words(int H, int W, int wide);
void launch_mark_tiles(const BrightArgs& a, hipStream_t s); // hot map -> tile boxes (tile_rows), behind launch_bright_cells
void launch_bright_cells(const BrightArgs& a, hipStream_t s);
// set-up statistics of an undistort table, for the dark-tile bound: stats[0] = largest total blend weight any source
// pixel carries over all output pixels (1024 = one full pixel), stats[1] / stats[2] = largest x / y extent (in source
// pixels) of the taps feeding one 5x5 output window.  acc: H*W zero-initialised scratch words.  edge: zero-initialised
// [ceil(H/8)][ceil(W/8)] words, bit 0 / bit 1 set for the 8x8 source cells read by windows that the image border cuts
// in exactly one axis / in both.  reach: [cells][4] = x0, x1, y0, y1 initialised to (INT_MAX, INT_MIN, INT_MAX, INT_MIN):
// bounding box of the output pixels that read the cell with a nonzero weight.
struct StatArgs { const uint32_t* map; const uint32_t* mapw; uint32_t* acc; uint32_t* stats; int H, W; uint32_t* edge; int* reach; };
void launch_remap_stats(const StatArgs& a, hipStream_t s);
void launch_undistort_map(const MapArgs& m, hipStream_t s);
void launch_contours(const ContourArgs& a, hipStream_t s);
// (blob_contour_follow.hip; launch_contours goes through it for the candidate walks and for the link walks)
void launch_contour_follow(const ContourArgs& a, int grid, hipStream_t s);
size_t contour_work_bytes();
size_t contour_walk_bytes(); // walk list bytes per image (split form of the contour stage)
size_t contour_link_bytes(); // link list bytes per image
void launch_box_blur(const uint8_t* src, uint8_t* dst, int H, int W, int sp, int dp, int ksize, hipStream_t s);
void launch_undistort(const uint8_t* src, uint8_t* dst, int H, int W, int sp, int dp, const uint32_t* map, const uint32_t* mapw,
                      hipStream_t s);
void launch_mask_expand(const uint32_t* mask, int wpr, uint8_t* dst, int H, int W, int dp, hipStream_t s);
void launch_median5(const uint8_t* src, uint8_t* dst, int H, int W, int sp, int dp, int ithresh, int apply, hipStream_t s);
void launch_demosaic(const uint8_t* bayer, uint8_t* bgr, int H, int W, int sp, hipStream_t s);
void launch_bayer_gray(const BayerArgs& a, hipStream_t s);
// the same pass fused with the early-out's scan of the gray frames it writes (bayer_scan_fusable: W % 16 == 0, H % 8 == 0, aligned);
// a.dst == nullptr: the scan alone, no gray frame is written (bayer_scan_direct: only the Bayer side's conditions)
bool bayer_scan_fusable(const BayerArgs& a);
bool bayer_scan_direct(const BayerArgs& a);
void launch_bayer_gray_scan(const BayerArgs& a, const BrightArgs& b, hipStream_t s);

// ---- geometry ----
struct CameraTable {           // device-resident, written by mocap_set_cameras / mocap_set_fundamentals
    double K[32][9], dist[32][5], R[32][9], t[32][3];
    double F[31][9];           // F[i-1]: camera-0 pixel -> epipolar line in camera i
    int n_cam, n_F;
};

struct CorrArgs {
    const CameraTable* cams;
    const void* pts;           // points of (t,c): pts + (t*pt_st + c*pt_sc) elements, [P][2] int32 or float64
    const int32_t* counts;     // count of (t,c): counts[t*cnt_st + c*cnt_sc]
    long pt_st, pt_sc, cnt_st, cnt_sc;
    int pts_f64;
    int T, C, P;               // P = capacity per camera
    double cutoff;
    int max_groups;            // per root
    // per time step, per camera-0 root
    double* root_xyz;          // [T][P][3]
    double* root_err;          // [T][P]  mean reprojection error over the root's groups
    double* root_grp;          // [T][P][C][2] first group
    int32_t* root_idx;         // [T][P]  camera-0 index of the j-th surviving root
    int32_t* order;            // [T][P]  argsort(root_err)
    int32_t* n_roots;          // [T]  (<0 = error)
    int prio;                  // wave priority (s_setprio 0..3), see ContourArgs
    int threads;               // threads per time step: 64 / 128 / 256 (A/B switch; one wave per step measured 0.064 against 0.051 ms)
    double* scratch;           // [T][step_budget] per-group errors, the groups of a time step back to back in root order
    int step_budget;           // groups per time step the scratch holds
    int lds_budget;            // set by launch_correspond: bytes of dynamic LDS the kernel's plan is made for
};

// correspondence from any camera pair, for markers only some cameras see (correspond_visible.hip)
struct VisArgs {
    const CameraTable* cams;   // K, dist, R, t of cameras 0..C-1 (F is not used: the pair matrices are formed on the device)
    const void* pts;           // points and counts through strides, as CorrArgs
    const int32_t* counts;
    long pt_st, pt_sc, cnt_st, cnt_sc;
    int pts_f64;
    int T, C, P;
    int distorted;             // 1 = the points are pixels of the distorted images: mapped to ideal pinhole pixels when loaded
    double cutoff, gate2, max_err; // epipolar limit (px), support limit squared (px^2), error limit (px^2)
    int min_views, max_passes;
    int max_hyp;               // seeds of one pass at most; beyond it the time step reports CORR_ERR_GROUPS
    int Q;                     // output rows per time step
    double* xyz;               // [T][Q][3]
    double* err;               // [T][Q]
    int32_t* idx;              // [T][Q][C] member point per camera, -1 = none
    uint32_t* views;           // [T][Q] bit c: camera c is a member
    int32_t* n;                // [T] markers, or CORR_ERR_*
    unsigned char* scratch;    // [T][correspond_visible_step_bytes(C, max_hyp)] hypothesis records and sort order of the steps that outgrow LDS
    size_t step_bytes;
    int lds_budget;            // set by launch_correspond_visible
};

struct TriArgs {
    const CameraTable* cams;
    const double* pts;         // [N][C][2]
    const uint8_t* valid;      // [N][C]
    int N, C;
    int compact_k;             // intrinsics indexed by position after dropping invalid entries (reference quirk)
    double* xyz;               // [N][3]
    int32_t* ok;               // [N] 1 = triangulated
};

struct ReprojArgs {
    const CameraTable* cams;
    const double* pts;         // [N][C][2]
    const uint8_t* valid;      // [N][C]
    const double* xyz;         // [N][3]
    int N, C, compact_k;
    double* mse;               // [N]
    int32_t* ok;               // [N]
};

struct EpiArgs {
    const CameraTable* cams;
    const void* roots;         // [n_roots][2] camera-0 points (int32 or float64)
    const void* cand;          // [n_cand][2] points of the other camera
    int n_roots, n_cand, pts_f64, f_index;
    double* dist;              // [n_roots][n_cand]
    float* lines;              // optional [n_roots][3]
};

struct BaArgs {
    const CameraTable* cams;   // K and dist of cameras 0..C-1 (R, t come from the parameters)
    const double* params;      // [B][6 (C - 1)] rotvec + t of cameras 1..C-1, device-accessible (pinned host memory is fine)
    const double* pts;         // [N][C][2]
    const uint8_t* valid;      // [N][C]
    int N, C, B;
    double* obj;               // scratch [B][N][3]
    float* res;                // [B][N], the first counts[b] entries of row b are the residual vector
    int32_t* counts;           // [B]
};

// fundamental matrices of n_pairs camera pairs by RANSAC over host-drawn samples (fundamental.hip)
struct FundArgs {
    const double* pts_a;       // [total][2] first camera's points, the pairs' lists one after another
    const double* pts_b;       // [total][2] the same markers in the second camera
    const int32_t* offset;     // [n_pairs + 1] device copy: pair p owns points offset[p] .. offset[p + 1] - 1
    const int32_t* samples;    // [n_pairs][H][8] point indices local to the pair
    int n_pairs, H, max_n;     // max_n: points of the largest pair (sizes the grids)
    double thr2;               // threshold squared
    double* F_all;             // scratch [n_pairs][H][9] every hypothesis' unit-norm matrix (all NaN = invalid)
    int32_t* counts;           // [n_pairs][H] zeroed before the launch: inliers of every hypothesis
    int32_t* pair_err;         // scratch [n_pairs] zeroed before the launch: nonzero = a sample index outside the pair
    double* F_sample;          // [n_pairs][9]
    double* F_refit;           // [n_pairs][9] or null: no refit
    uint8_t* inlier;           // [total]
    int32_t* status;           // [n_pairs][2] (winner, inliers) or (FUND_ERR_*, 0)
};

// The state record of one Levenberg-Marquardt loop (lm.h holds its rule): written by single-workgroup kernels only (the flags
// `behind`, `trial_behind` and, where several workgroups factorise, `chol_fail` also by integer atomicOr), read by every kernel
// of the iterations that follow.
struct LmState {
    double lambda, nu;         // Marquardt damping and Nielsen's growth factor
    double cost, cost0;        // 1/2 sum r^2 of the current state, and of the state handed in
    int32_t stop, status;      // stop != 0: every later kernel of this loop returns at once; status: RIG_STOP_* or the solver's error
    int32_t iters, cur;        // iterations done; which of the two state buffers holds the current state
    int32_t chol_fail, chol_fail_prev, behind, trial_behind;
};

// bundle adjustment of a rig: one loop per call.  Two solvers share this record and every phase but one (rig_lm.h): the plain
// one moves the poses of cameras 1..C-1 (rig_ba.hip: camera blocks 6 wide, camera 0 has none), the other also every camera's
// lens (rig_selfcal.hip: blocks 15 wide -- kd's 9, then the pose's 6 -- for every camera, camera 0 included).  Below, P is the
// block's width, FIRST the first camera that has a block, D = P (C - FIRST) the rows of the reduced system.
struct RigState : LmState {
    double t1_norm;            // |t_1| handed in: the gauge restored on return
    int32_t layout_err, pad;
};
enum { RIG_LIN_COST = 0, RIG_PRED_CAM = 1, RIG_NORM2_CAM = 2, RIG_N_SCALARS = 4 }; // (PRED_CAM, NORM2_CAM: lm_decide's `cam` pair)
enum { RIG_STOP_MAX_ITERS = 1, RIG_STOP_FTOL = 2, RIG_STOP_LAMBDA = 3, RIG_STOP_CHOLESKY = 4, RIG_ERR_LAYOUT = -2, RIG_ERR_BEHIND = -3 };
constexpr int PT_THREADS = 256; // points per workgroup of the point-owning kernels (linearize, update, residuals): n_lin_blocks = ceil(N / PT_THREADS)

struct RigArgs {
    const int32_t* obs_offset; // [N + 1] point n owns observations obs_offset[n] .. obs_offset[n + 1] - 1
    const int32_t* obs_cam;    // [n_obs] ascending within a point
    const double* obs_uv;      // [n_obs][2]
    int C, N, n_obs;
    int n_pairs, n_lin_blocks, n_chunks; // pairs a <= b of cameras that have a block; workgroups of the point kernels; chunks of the Schur kernel
    int loss;                  // LOSS_* of lm.h: which instantiation of the point kernels the launchers pick
    double loss_c2;            // the loss's squared scale c^2 in px^2 (unused by LOSS_NONE)
    double* poses_io;          // [C][12] the caller's: R row-major, then t
    double* points_io;         // [N][3] the caller's
    // the cameras' lenses.  Used by the pose block alone (null otherwise): constant, from the context's table
    const CameraTable* cams;   // K and dist of cameras 0..C-1, by true camera number
    // used by the lens block alone (null / 0 otherwise): the first the caller's, the rest scratch of the context
    double* kd_io;             // [C][9] the caller's: fx, fy, cx, cy, k1, k2, p1, p2, k3
    double* kd;                // [2][C][9] current and trial state (state->cur)
    const int32_t* free_cols;  // [C] device copy: bit i = column i of the camera's block is free (bits 0..8 the caller's mask,
                               //   bits 9..14 the pose: set for cameras 1.., clear for camera 0)
    int32_t* cam_count;        // [C] observations of every camera (zeroed before the init kernel)
    int schur_chunk;           // points of a chunk of its Schur kernel: n_chunks = ceil(N / schur_chunk)
    // scratch of the context
    RigState* state;
    double* poses;             // [2][C][12] current and trial state (state->cur)
    double* points;            // [2][N][3]
    uint32_t* mask;            // [N] bit c: camera c sees the point
    double* W;                 // [n_obs][3 P] W_nc, P x 3 row-major (unused for a camera below FIRST)
    double* Vinv;              // [N][6] damped V^-1, upper triangle
    double* vdiag;             // [N][3] diagonal of the undamped V
    double* gp;                // [N][3] g_n
    double* lin_part;          // [n_lin_blocks][C - FIRST][P (P + 1) / 2 + P] per-workgroup U_c (upper triangle) and g_c
    double* cost_part;         // [n_lin_blocks]
    double* schur_part;        // [n_chunks][n_pairs][P P + P] W_a V*^-1 W_b^T, then W_a V*^-1 g_n
    double* S;                 // [D][D] the damped reduced camera matrix; a fixed column's diagonal entry is 1
    double* rhs;               // [D] reduced right-hand side
    double* gc;                // [D] camera gradient
    double* udiag;             // [D] diagonal of the undamped U
    double* chol;              // [D (D + 1) / 2] the factor when it does not fit LDS
    double* delta_c;           // [D] camera step
    double* upd_part;          // [n_lin_blocks][3] trial cost, predicted reduction, |step|^2 of the points
    double* scalars;           // [RIG_N_SCALARS]
    double* history;           // [max_iters][4] the caller's (or null for a linearisation alone)
    double* result;            // [4] the caller's
    double* obs_err;           // [n_obs] the caller's or null: |r| of every observation at the returned state
    double* obs_weight;        // [n_obs] the caller's or null: the loss's weight there (1 for LOSS_NONE)
};

// What the host needs of a solver: its block's figures, the points of a chunk of its Schur kernel for N points, and its launches
// (rig_lm.h's, instantiated for its block; residuals goes behind finish: obs_err, obs_weight).
struct RigSolver {
    int P, FIRST;
    int (*schur_chunk)(int N);
    void (*init)(const RigArgs& a, double lambda0, hipStream_t s);
    void (*linearize)(const RigArgs& a, hipStream_t s);
    void (*iteration)(const RigArgs& a, int it, int max_iters, double ftol, hipStream_t s);
    void (*finish)(const RigArgs& a, hipStream_t s);
    void (*residuals)(const RigArgs& a, hipStream_t s);
};
RigSolver rig_pose_solver(); // rig_ba.hip
RigSolver rig_lens_solver(); // rig_selfcal.hip

// intrinsic calibration of every camera of a rig from planar-board views (intrinsics.hip): one loop, and one state record, per
// camera; no kernel reads another camera's.  status: RIG_STOP_* / INTR_ERR_*
using IntrState = LmState;
enum { INTR_ERR_LAYOUT = -2, INTR_ERR_BEHIND = -3, INTR_ERR_DEGENERATE = -4 };
// A view's record, in doubles: the 136 sums of [J r]^T [J r] (16 columns: kd's 9, the pose's 6, r; upper triangle row by row),
// then the upper triangle of W V*^-1 W^T (45), W V*^-1 g_v (9), the factor of V* (packed lower triangle, 21)
enum { INTR_REC_SUMS = 0, INTR_REC_T = 136, INTR_REC_YG = 181, INTR_REC_L = 190, INTR_REC = 216 };

struct IntrArgs {
    int n_cams, n_views;
    const int32_t* view_offset;  // [n_cams + 1] camera c owns views view_offset[c] .. view_offset[c + 1] - 1     (device copies
    const int32_t* point_offset; // [n_views + 1] view v owns points point_offset[v] .. point_offset[v + 1] - 1     made by the
    const int32_t* view_cam;     // [n_views] the view's camera                                                      entry point)
    const int32_t* image_size;   // [n_cams][2] width, height (read by the initialisation only)
    const int32_t* cam_bad;      // [n_cams] nonzero: fewer than 3 views, a view with fewer than 4 points, or 2 points < 9 + 6 views
    const double* obj;           // [total][2] board points (X, Y), Z = 0
    const double* img;           // [total][2] their pixels
    double* kd_io;               // [n_cams][9] the caller's: fx, fy, cx, cy, k1, k2, p1, p2, k3
    double* poses_io;            // [n_views][12] the caller's: R row-major, then t (board -> camera)
    double* view_rms;            // [n_views] the caller's
    double* history;             // [n_cams][max_iters][4] the caller's
    double* result;              // [n_cams][4] the caller's
    int32_t* lin_status;         // [n_cams][2] the caller's (mocap_intrinsics_linearize), else null
    int max_iters;
    // scratch of the context
    IntrState* state;            // [n_cams]
    double* kd;                  // [2][n_cams][9] current and trial state (state->cur)
    double* poses;               // [2][n_views][12]
    double* view_cost;           // [2][n_views] sum r^2 of the view in the current and the trial state
    double* H;                   // [n_views][9] the initialisation's homographies
    double* rec;                 // [n_views][INTR_REC]
    double* gv;                  // [n_views][6] the views' gradients
    double* S;                   // [n_cams][81] damped reduced camera matrix
    double* rhs;                 // [n_cams][9]
    double* gc;                  // [n_cams][9] camera gradient
    double* udiag;               // [n_cams][9] diagonal of the undamped U
    double* delta_c;             // [n_cams][9] camera step
    double* lin_cost;            // [n_cams] 1/2 sum r^2 of the linearised state
    double* cam_part;            // [n_cams][2] the camera's part of the predicted reduction and of |step|^2
    double* upd_part;            // [n_views][3] trial sum r^2, predicted reduction, |step|^2 of the view
};
void launch_intr_begin(const IntrArgs& a, int have_start, double lambda0, hipStream_t s);
void launch_intr_linearize(const IntrArgs& a, int it, bool solve, hipStream_t s);
void launch_intr_iteration(const IntrArgs& a, int it, double ftol, hipStream_t s);
void launch_intr_finish(const IntrArgs& a, hipStream_t s);

enum { CORR_ERR_GROUPS = -2, CORR_ERR_TRUNCATED = -3, CORR_ERR_BLOB = -4, CORR_ERR_OUTPUT = -5 };
enum { FUND_ERR_SAMPLE = -2, FUND_ERR_DEGENERATE = -3 };
enum { TRACK_ERR_FULL = -2, TRACK_ERR_IDS = -3, TRACK_ERR_INPUT = -4, TRACK_ERR_COUNT = -5 };

// marker identities across time steps (track.hip).  The caller's state buffer: a 64-byte header, then one
// 64-byte record per slot (include/mocap_hip.h: mocap_track_header / mocap_track_slot; all-zero bytes = the empty tracker).
constexpr int TRACK_MAX = 256; // slots of a tracker and detections of a time step at most
struct TrackHeader { int32_t next_id, reserved0; int64_t steps; int64_t reserved[6]; };
struct TrackSlot { double pos[3], vel[3]; int32_t id, miss, hits, alive; };
static_assert(sizeof(TrackHeader) == 64 && sizeof(TrackSlot) == 64, "the state buffer's layout is part of the ABI");
struct TrackArgs {
    const double* xyz;         // [T][Q][3] detections; rows at and beyond n[t] take no part
    const int32_t* n;          // [T] detections of the step; < 0 or > min(Q, 256): a blind step
    int T, Q, M;
    void* state;               // TrackHeader, then M TrackSlot
    double gate, beta;
    int max_miss;
    int32_t* id;               // [T][Q] each: identity, slot, age of the detection of that row; -1 = none
    int32_t* slot;
    int32_t* age;
    int32_t* status;           // [T] 0 or TRACK_ERR_*
};
void launch_track_markers(const TrackArgs& a, hipStream_t s);

// rigid-body poses per time step (rigid.hip).  The codes and caps are include/mocap_hip.h's MOCAP_RIGID_*.
enum { RIGID_LOST = 1, RIGID_ERR_BLIND = -2, RIGID_ERR_CAPACITY = -3, RIGID_ERR_MODEL = -4, RIGID_ERR_HYP = -5 };
constexpr int RIGID_MAX_DET = 64;      // detections of a time step
constexpr int RIGID_MAX_MARKERS = 8;   // model points of a body
constexpr int RIGID_MAX_TRIPLES = 56;  // model triples of a body: C(8, 3)
constexpr int RIGID_MAX_BODIES = 16;
constexpr int RIGID_MAX_HYP = 4096;    // candidates of one (time step, body): the LDS list's entries
struct RigidArgs {
    const double* xyz;         // [T][Q][3] detections; rows at and beyond n[t] take no part
    const int32_t* n;          // [T] detections of the step; < 0 or > min(Q, 64): a blind step
    int T, Q, B;
    const double* model;       // [B][8][3]
    const int32_t* n_markers;  // [B] 3..8
    const int32_t* tri;        // [B][56][3] model triples a < b < c
    const int32_t* n_tri;      // [B] 1..56
    double tol, gate;
    int min_markers, max_hyp;
    double* R;                 // [T][B][9]
    double* t;                 // [T][B][3]
    double* q;                 // [T][B][4] (w, x, y, z)
    double* rms;               // [T][B]
    int32_t* n_in;             // [T][B]
    int32_t* label;            // [T][B][8] detection row or -1
    int32_t* status;           // [T][B] 0, RIGID_LOST or RIGID_ERR_*
};
void launch_rigid_poses(const RigidArgs& a, hipStream_t s);

// rigid-body models learned from a tracked capture (rigid_learn.hip).  The codes and caps are
// include/mocap_hip.h's MOCAP_LEARN_*.  Every sum over time is formed per chunk of LEARN_CHUNK steps, in ascending t from 0, and
// the chunks' partial sums are added in ascending chunk: the partials live in the caller's workspace, cut up by LearnWork.
enum { LEARN_ERR_MEMBERS = -2, LEARN_ERR_INCOMPLETE = -3 };
constexpr int LEARN_CHUNK = 32;
constexpr int LEARN_MAX_IDS = 64;      // identities of one mocap_learn_marker_pair_stats
constexpr int LEARN_MAX_GROUPS = 16;   // groups of one mocap_learn_rigid_bodies
constexpr int LEARN_MAX_WANTED = LEARN_MAX_GROUPS * RIGID_MAX_MARKERS; // identities either call locates per step
struct LearnWanted { int32_t id[LEARN_MAX_WANTED]; }; // travels by value in the kernel arguments; -1 = a column nobody wants
// the caller's workspace (MOCAP_LEARN_WORK_BYTES): doubles first, then the integers, each array whole
struct LearnWork {
    double *pmin, *pmax, *psum, *psum2; // pair stats: [chunks][P] each, P = K (K + 1) / 2 pairs a <= b
    double *model;                      // rigid learn: [G][8][3] the current model
    double *gsum;                       // [chunks][G][8][3] a pass's partial sums (b per axis; the squared residual in [..][0])
    int32_t *pcnt;                      // [chunks][P]
    int32_t *row;                       // [T][W] the row of each wanted identity in each step, -1 = absent
    int32_t *gcnt;                      // [chunks][G][8] additions per member
    int32_t *gused;                     // [chunks][G] used steps
    int32_t *gstate;                    // [G][2] ref_step, status
    size_t bytes;
    LearnWork() = default;
    // T steps, K identities of the pair statistics (0: none), G groups (0: none); base may be null (only `bytes` counts)
    LearnWork(void* base, long long T, int K, int G)
    {
        const size_t C = (size_t)((T + LEARN_CHUNK - 1) / LEARN_CHUNK), P = (size_t)K * (K + 1) / 2, W = (size_t)K + 8 * (size_t)G;
        double* d = (double*)base;
        pmin = d; pmax = pmin + C * P; psum = pmax + C * P; psum2 = psum + C * P;
        model = psum2 + C * P; gsum = model + 24 * (size_t)G;
        int32_t* i = (int32_t*)(gsum + C * G * 24);
        pcnt = i; row = pcnt + C * P; gcnt = row + (size_t)T * W; gused = gcnt + C * G * 8; gstate = gused + C * G;
        bytes = (size_t)((char*)(gstate + 2 * (size_t)G) - (char*)base);
    }
};
struct PairArgs {
    const double* xyz;         // [T][Q][3]
    const int32_t* n;          // [T]; < 0 or > Q: a blind step
    const int32_t* id;         // [T][Q] identities, -1 = none
    int T, Q, K;
    LearnWanted ids;           // [K] strictly ascending, >= 0 (the host checked)
    LearnWork w;
    int32_t* count;            // [K][K] outputs
    double *dmin, *dmax, *dsum, *dsum2;
};
void launch_marker_pair_stats(const PairArgs& a, hipStream_t s);
struct LearnArgs {
    const double* xyz;
    const int32_t* n;
    const int32_t* id;
    int T, Q, G;
    LearnWanted members;       // [G][8]; -1 from n_members on and in every slot of a group that is not valid
    int32_t n_members[LEARN_MAX_GROUPS];
    uint32_t valid;            // bit g: the group's members are 3..8 distinct identities >= 0, at least min_present of them
    int rounds, min_present;
    LearnWork w;
    double* model;             // [G][8][3]
    double* rms;               // [G]
    double* member_rms;        // [G][8]
    int32_t* member_count;     // [G][8]
    int32_t* steps_used;       // [G]
    int32_t* ref_step;         // [G]
    int32_t* status;           // [G]
};
void launch_rigid_learn(const LearnArgs& a, hipStream_t s);

// sub-pixel centroids from the frames (subpixel.hip): the flag bits are include/mocap_hip.h's MOCAP_SUBPIX_*
enum { SUBPIX_EMPTY = 1, SUBPIX_EDGE = 2, SUBPIX_NEIGHBOUR = 4, SUBPIX_MOVING = 8, SUBPIX_CUT = 16 };
constexpr int SUBPIX_MAX_BLOBS = 256; // centroids of one image at most: one per thread of its workgroup
constexpr int SUBPIX_LENS = 16;       // doubles per slot in `lens`: K (9), dist (5), 1.0 = the slot's table is the identity, padding
struct RefineArgs {
    const uint8_t* src; size_t image_stride; int pitch, H, W; // gray frames, or raw Bayer frames (bayer = 1: ry, rx, cb, cg, cr, shift as BayerArgs)
    int n_images, cam_mod;
    int bayer, ry, rx; uint32_t cb, cg, cr; int shift;
    const double* lens;        // [cam_mod][SUBPIX_LENS] of the first slot used
    const int32_t* xy; long xy_stride;       // integer centroids of image n: xy + n * xy_stride, (cx, cy) pairs
    const int32_t* count; long count_stride; // their number: count[n * count_stride]
    int max_blobs;             // 1..SUBPIX_MAX_BLOBS
    int radius, floor, iters, coords;
    double* out_xy; long out_xy_stride;      // [n_images][max_blobs][2] through the stride (in doubles)
    int32_t* out_info; long out_info_stride; // (S of the last window, flags) per centroid, or null
};
void launch_refine_centroids(const RefineArgs& a, hipStream_t s);

// refinement of triangulated markers by their reprojection error, with covariance (refine_points.hip).  A
// row's status is a RIG_STOP_* code (refined), 0 (no row) or one of these, include/mocap_hip.h's MOCAP_REFINE_E_*
enum { REFINE_ERR_VIEWS = -2, REFINE_ERR_INPUT = -3, REFINE_ERR_BEHIND = -4 };
struct RefinePointsArgs {
    const CameraTable* cams;   // K, dist, R, t of cameras 0..C-1
    const double* xyz;         // [T][Q][3] the points handed in (may be xyz_out)
    const int32_t* n;          // [T] rows of the step; <= 0: none
    const uint32_t* views;     // [T][Q] bit c: camera c is a member; null (grouped form only) = all C cameras
    int T, Q, C;
    // indexed form: the member point of camera c is idx[t][q][c] of the camera's list, read as VisArgs' points are
    const void* pts;
    long pt_st, pt_sc;
    int pts_f64, P;
    const int32_t* idx;        // [T][Q][C]
    // grouped form (pts == null)
    const double* grp;         // [T][Q][C][2]
    int distorted;             // 1 = the points are raw-frame pixels: the residual goes through the camera's five distortion terms
    int max_iters;
    double ftol, lambda0;
    double max_res2;           // > 0: pruning is on
    int min_views, max_drop;
    double* xyz_out;           // [T][Q][3]
    double* err;               // [T][Q]
    double* res2;              // [T][Q][C] squared residual length per member, -1 = no member
    double* cov;               // [T][Q][6] inv_sym3's layout
    uint32_t* views_out;       // [T][Q]
    uint32_t* dropped;         // [T][Q]
    int32_t* iters;            // [T][Q]
    int32_t* status;           // [T][Q]
};
void launch_refine_points(const RefinePointsArgs& a, hipStream_t s);

void launch_fundamental_ransac(const FundArgs& a, hipStream_t s);

enum { LDS_USER_CORRESPOND, LDS_USER_VISIBLE, LDS_USERS };
int workgroup_lds_limit(int user, const void* kernel_f64, const void* kernel_i32); // correspond.hip: bytes of dynamic LDS per workgroup
void launch_correspond(const CorrArgs& a, hipStream_t s);
size_t correspond_smem_bytes(int P, int C);
bool correspond_fits(int P, int C); // the kernel's LDS plan for P points x C cameras fits a workgroup
void launch_correspond_visible(const VisArgs& a, hipStream_t s);
size_t correspond_visible_smem_bytes(int P, int C);
bool correspond_visible_fits(int P, int C);               // the kernel's LDS plan for P points x C cameras fits a workgroup
size_t correspond_visible_step_bytes(int C, int max_hyp); // scratch of one time step
void launch_epipolar_scores(const EpiArgs& a, hipStream_t s);
void launch_ba_residuals(const BaArgs& a, hipStream_t s);
void launch_triangulate(const TriArgs& a, hipStream_t s);
void launch_reproject(const ReprojArgs& a, hipStream_t s);

} // namespace mocap
