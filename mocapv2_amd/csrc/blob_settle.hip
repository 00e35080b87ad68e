// blob_settle.hip -- between the streaming scan and the two filter kernels of the sparse path: settle_tiles_kernel, one thread per
// (tile, image), turns the box the scan left on the tile (reachable mask rows and columns) into work items of a bounded size in ONE
// global list (box_filter_kernel, blob_boxes.hip) -- or, a wide box, into entries of the wide-tile list that the sliding row pipeline
// works through (blob_rows.hip); a wide box with empty columns between its markers is cut at them into items after all --, clears
// what the previous batch left in the mask where this batch will not write, and empties the next batch's tile records.
// The records it writes (items, wide-tile entries, the tiles' regions) are defined in kernels.h.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "kernels.h"

namespace mocap {

namespace {
__device__ __forceinline__ int imin(int a, int b) { return a < b ? a : b; }
__device__ __forceinline__ int imax(int a, int b) { return a > b ? a : b; }
} // namespace

// How a tile's output region (nb mask bytes wide, h rows) is cut into items: nx x ny parts (nx * ny <= BOX_MAX_PARTS) such that a
// part's patch -- (bytes * 2 + 2) quads x (rows + 8) -- fits BOX_HCAP quad-rows, minimising the wave instructions
// ("trips": rows per instruction = 64 / quads) plus a fixed cost per item.
__device__ __forceinline__ void choose_split(int nb, int h, int& nx, int& ny)
{
    int best = 0x7fffffff;
    nx = 1; ny = 1;
    for (int cx = 1; cx <= 4; cx++) {
        const int pb = (nb + cx - 1) / cx, Q = 2 * pb + 2;
        if (Q > 64) continue;
        const int rpw = 64 / Q, mr = BOX_HCAP / Q - 8;
        if (mr < 1) continue;
        const int cy = (h + mr - 1) / mr;
        if (cx * cy > BOX_MAX_PARTS) continue;
        const int ph = (h + cy - 1) / cy;
        const int cost = cx * cy * ((ph + 8 + rpw - 1) / rpw + 8);
        if (cost < best) { best = cost; nx = cx; ny = cy; }
    }
}

namespace {

struct Rect { int x0, x1, y0, y1; }; // columns [x0, x1], rows [y0, y1]; x0 > x1 or y0 > y1: empty
constexpr uint4 NO_BOX = {0xffffffffu, 0u, 0u, 0u}; // a tile of tile_rows the scan did not mark (first row > last row, no quad)

// a tile's record as the box it stands for: its rows, and the first and last marked quad column of strip `st` clamped into the image
__device__ __forceinline__ Rect record_box(uint4 rec, int st, int W)
{
    Rect b{0, 0, (int)rec.x, (int)rec.y};
    tile_quad_columns(st, (uint64_t)rec.w << 32 | rec.z, W, b.x0, b.x1);
    return b;
}

// ---- thread -> (tile, slot, time step) ----------------------------------------------------------------------------------
// Time fastest: the items of one tile of one camera lie together in the list, so the waves that work at the same time share
// undistort-table lines (matters when every tile is filtered).  The grid also covers the images beyond this batch whose boxes
// an earlier, larger batch may have left in the array the next batch's scan will widen (n_clear): n_all images in all.
struct TileOfThread { int image, chunk, strip; size_t idx; bool valid; };
__device__ __forceinline__ TileOfThread tile_of_thread(const BoxArgs& a, int n_all)
{
    const int steps_all = (n_all + a.cam_mod - 1) / a.cam_mod;
    const long long total = (long long)a.n_chunks * a.n_strips * a.cam_mod * steps_all;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    TileOfThread t{0, 0, 0, 0, i < total};
    if (t.valid) {
        const int step = (int)(i % steps_all);
        const long long rest = i / steps_all;
        const int slot = (int)(rest % a.cam_mod), tile = (int)(rest / a.cam_mod);
        t.image = step * a.cam_mod + slot;
        t.chunk = tile / a.n_strips; t.strip = tile - t.chunk * a.n_strips;
        t.valid = t.chunk * a.rows_per_chunk < a.H;
    }
    t.idx = ((size_t)t.image * a.n_chunks + t.chunk) * a.n_strips + t.strip;
    return t;
}

// ---- the scan's box of the tile: where exact pixels are needed / bits can be set -------------------------------------------
// (the scan's records of this batch are only read here: neighbouring tiles look at each other's).  false: the tile is not marked.
// quads: the record's quad mask (0 where there is no record).  The box's columns are the mask's: whole quads inside the tile's window.
__device__ __forceinline__ bool scan_box(const BoxArgs& a, const TileOfThread& t, bool valid, Rect& box, uint64_t& quads)
{
    box = {0, a.W - 1, 0, a.H - 1};
    quads = 0;
    if (!valid || a.dense) return valid;
    const uint4 raw = *(const uint4*)(a.tile_rows + 4 * t.idx);
    if (raw.x > raw.y) return false;
    quads = (uint64_t)raw.w << 32 | raw.z;
    box = record_box(raw, t.strip, a.W);
    return true;
}

// ---- cluster decision ---------------------------------------------------------------------------------------------------
// The marked tiles of an aligned 2 x 2 block of tiles whose boxes together are small (one marker on a tile border, nothing else
// nearby) are filtered ONCE, as the union of their boxes clipped to the block, by the item the first of them emits -- instead of
// one clipped piece per tile, each with its own halo rows, staging and set-up.  Every tile of the block takes the same decision
// from the same read-only data; each still records its own clipped region.
// In: cover = the tile's own region, exact = its scan box.  Out: the region the emitted items cover, the box they take their exact
// pixels from; false: another tile of the block emits them.
__device__ __forceinline__ bool cluster_decision(const BoxArgs& a, const TileOfThread& t, Rect& cover, Rect& exact)
{
    const int c0 = t.chunk & ~1, s0 = t.strip & ~1;
    int n_marked = 0, first = -1;
    Rect u{0x7fffffff, -1, 0x7fffffff, -1};
    for (int k = 0; k < 4; k++) {
        const int cy = c0 + (k >> 1), sx = s0 + (k & 1);
        if (cy >= a.n_chunks || sx >= a.n_strips || cy * a.rows_per_chunk >= a.H) continue;
        const uint4 o = *(const uint4*)(a.tile_rows + 4 * (((size_t)t.image * a.n_chunks + cy) * a.n_strips + sx));
        if (o.x > o.y) continue;
        if (first < 0) first = k;
        n_marked++;
        // (a rectangle that reaches this tile from beyond its window also marks the neighbour it comes from: inside the block's own
        // window, which is all that e and the item's patch look at, the union of the windows' columns is the union of the rectangles')
        const Rect ob = record_box(o, sx, a.W);
        u.y0 = imin(u.y0, ob.y0); u.y1 = imax(u.y1, ob.y1); u.x0 = imin(u.x0, ob.x0); u.x1 = imax(u.x1, ob.x1);
    }
    if (n_marked < 2) return true;
    // the union, clipped to the block and the image, in whole mask bytes
    const int bx_lo = 240 * s0, bx_hi = imin(240 * (s0 + 2) - 1, a.W - 1), by_lo = c0 * a.rows_per_chunk, by_hi = imin((c0 + 2) * a.rows_per_chunk, a.H) - 1;
    const Rect e{imax(u.x0, bx_lo) & ~7, imin(u.x1 | 7, bx_hi), imax(u.y0, by_lo), imin(u.y1, by_hi)};
    if (((e.x1 - e.x0 + 8) >> 3) > 13 || e.y1 - e.y0 + 1 > 100) return true;
    cover = e; exact = u;
    return first == ((t.chunk - c0) * 2 + (t.strip - s0));
}

// ---- record the region, clear the previous one --------------------------------------------------------------------------------
// What the previous batch wrote in this tile of the context's own mask and this batch will not overwrite has to be cleared (the
// mask keeps "zero outside the recorded regions" from batch to batch; a caller-owned mask was cleared by the scan kernel
// instead, or is written whole when every tile is filtered).  Records the tile's region `out` (empty = none) and the scan's box
// in cur_box, resets the tile's occupancy word; true: the previous region (prev_x, prev_y: spans) needs clearing.
__device__ __forceinline__ bool record_region(const BoxArgs& a, const TileOfThread& t, bool marked, const Rect& out, const Rect& box, uint32_t& prev_x,
                                              uint32_t& prev_y)
{
    const uint32_t out_x = span_pack(out.x0, out.x1), out_y = span_pack(out.y0, out.y1);
    uint4* cb = (uint4*)(a.cur_box + 4 * t.idx);
    bool need_clear = false;
    if (!a.ext_mask) {
        const uint4 prev = *cb;
        prev_x = prev.x; prev_y = prev.y;
        const int px0 = span_first(prev.x), px1 = span_last(prev.x), py0 = span_first(prev.y), py1 = span_last(prev.y);
        if (px0 <= px1) need_clear = !(marked && out.x0 <= px0 && px1 <= out.x1 && out.y0 <= py0 && py1 <= out.y1);
        if (prev.x != out_x || prev.y != out_y || marked) *cb = tile_box_pack(out_x, out_y, box.x0, box.x1, box.y0, box.y1);
        if (a.cells[t.idx] != 0u) a.cells[t.idx] = 0u;
    } else {
        *cb = tile_box_pack(out_x, out_y, box.x0, box.x1, box.y0, box.y1);
        a.cells[t.idx] = 0u;
    }
    return need_clear;
}
// the whole wave clears one region after the other
__device__ __forceinline__ void clear_previous(const BoxArgs& a, bool need_clear, uint32_t prev_x, uint32_t prev_y, int image)
{
    const int lane = threadIdx.x & 63;
    for (uint64_t todo = __ballot(need_clear); todo; todo &= todo - 1) {
        const int src = __ffsll((long long)todo) - 1;
        const uint32_t cx = (uint32_t)__builtin_amdgcn_readlane((int)prev_x, src), cy = (uint32_t)__builtin_amdgcn_readlane((int)prev_y, src);
        const int cimage = __builtin_amdgcn_readlane(image, src);
        const int x0 = span_first(cx), x1 = span_last(cx), y0 = span_first(cy), y1 = span_last(cy);
        uint8_t* m = (uint8_t*)(a.mask + (size_t)cimage * mask_image_words(a.H, a.words_per_row));
        // consecutive lanes walk down the rows of one byte column: 32 of them share a line of the blocked mask
        const int b0 = x0 >> 3, nr = y1 - y0 + 1, n = nr * ((x1 >> 3) - b0 + 1); // n <= 30 byte columns x the rows of a tile
        const float rcp_nr = __builtin_amdgcn_rcpf((float)nr);
        for (int i = lane; i < n; i += 64) {
            const int bc = small_div(i, rcp_nr);
            m[mask_byte_index(y0 + (i - bc * nr), b0 + bc, a.words_per_row)] = 0;
        }
    }
}

// ---- wide entries -------------------------------------------------------------------------------------------------------
// The wide tiles of this wave: `wide_bands` slots each in their list (the row pipeline is a serial walk down the rows, so a tile's
// latency, not its work, sets the duration of that short kernel: its rows [y0, y1] are cut into bands for several waves, 8 halo
// rows each).
__device__ __forceinline__ void emit_wide(const BoxArgs& a, bool wide, int image, int tile, int y0, int y1)
{
    const uint64_t wb = __ballot(wide);
    if (!wb) return;
    const int lane = threadIdx.x & 63, nbands = a.wide_bands;
    uint32_t base = 0;
    if (lane == 0) base = atomicAdd(a.n_items + 8, (uint32_t)(__popcll(wb) * nbands));
    base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
    const uint32_t o = base + (uint32_t)(__popcll(wb & ((1ull << lane) - 1ull)) * nbands);
    if (!wide) return;
    const int hb = (y1 - y0 + nbands) / nbands; // rows per band
    for (int b = 0; b < nbands; b++) {
        const int b0 = y0 + b * hb, b1 = imin(b0 + hb - 1, y1);
        if (o + b < a.cap_wide) a.wide_tiles[o + b] = wide_tile_pack(image, tile, b0, b1); // (a band without rows is an entry too)
    }
}

// the split tiles of this wave, counted for the read-back of the list counts (one atomic per wave that has any)
__device__ __forceinline__ void count_split(const BoxArgs& a, bool split)
{
    const uint64_t sb = __ballot(split);
    if (sb && (threadIdx.x & 63) == 0) atomicAdd(a.n_items + SPLIT_COUNTER, (uint32_t)__popcll(sb));
}

// ---- a gapped wide tile, cut at its empty columns ------------------------------------------------------------------------------
// The pieces a thread emits items for, 16 bits each: first and last mask byte column of the piece within its tile (5 bits each),
// then nx and ny of its parts (3 bits each).  A tile that is not split has one piece, of which only nx and ny are used.
__device__ __forceinline__ uint64_t piece_pack(int b0, int b1, int nx, int ny) { return (uint64_t)(b0 | b1 << 5 | nx << 10 | ny << 13); }

// A tile on its way to the wide list whose column word (the byte columns some hot cell's rectangle overlaps: tile_quad_bytes of its record) has empty
// columns inside the region: the maximal runs of set columns become one piece each, IF there are at least two, every run alone
// (its bytes x the region's h rows) would be routed to the box kernel, and the parts of all of them together are at most
// BOX_MAX_PARTS -- what the item list's capacity rests on.  Else the tile stays a wide entry (0 is returned).
// Why a run's items are exact by themselves (exact pixels are needed only within reach + 4, which is what
// the rectangles are): a rectangle marks every byte column it overlaps, so it lies within ONE run; two runs have an empty byte
// column between them, so a rectangle of another run begins at least 8 pixels beyond this run's bytes, while the patch of this
// run's items ends 4 pixels beyond them.  No patch meets another run's rectangles: the run's byte extent (towards the tile's
// edges the box's own extent, which reaches into the neighbour's halo) holds every exact pixel its items need.
// In: cols = the column word, [b0, b1] = the region's byte columns within the tile.  Out: the pieces, their number.
__device__ __forceinline__ int split_at_gaps(uint32_t cols, int b0, int b1, int h, int limit, uint64_t& pieces)
{
    uint32_t w = cols & ((2u << b1) - (1u << b0));
    int n = 0, parts = 0;
    pieces = 0;
    while (w) {
        const int r0 = __ffs((int)w) - 1;
        const uint32_t up = w + (1u << r0);           // the carry runs through the run's bits
        const int r1 = (up ? __ffs((int)up) - 1 : 32) - 1;
        w &= up;                                       // the run is gone
        int nx, ny;
        choose_split(r1 - r0 + 1, h, nx, ny);
        if (n == BOX_MAX_PARTS || 2 * (r1 - r0 + 1) + 2 * nx >= limit) return 0;
        pieces |= piece_pack(r0, r1, nx, ny) << (16 * n);
        n++; parts += nx * ny;
    }
    return (n >= 2 && parts <= BOX_MAX_PARTS) ? n : 0;
}

// ---- items ------------------------------------------------------------------------------------------------------------------
// This thread's pieces (none: n_pieces = 0), each as its nx x ny parts, at consecutive places of the list: one atomic per wave.
// A tile that is not split has one piece: `cover`, with its exact pixels from `exact`.  The pieces of a split tile (split_at_gaps)
// are runs of byte columns of the tile [tile_x0, tile_x1]: a run covers its columns x the rows of `cover` and takes its exact pixels from
// the rows of `exact` and its own byte extent -- where it holds the tile's first / last byte, from the extent of `exact` on that
// side, which is not clipped to the tile: a marker that straddles the tile's edge needs its halo pixels exact.
__device__ __forceinline__ void emit_items(const BoxArgs& a, int n_pieces, uint64_t pieces, bool split, int image, int tile, const Rect& cover,
                                           const Rect& exact, int tile_x0, int tile_x1)
{
    static_assert(BOX_MAX_PARTS <= 4, "a thread's pieces are packed into one 64-bit word");
    const int lane = threadIdx.x & 63;
    int cnt = 0;
    for (int k = 0; k < n_pieces; k++) cnt += (int)((pieces >> (16 * k + 10)) & 7u) * (int)((pieces >> (16 * k + 13)) & 7u);
    int incl = cnt; // inclusive prefix sum over the wave
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_up(incl, d);
        if (lane >= d) incl += o;
    }
    const int wave_total = __builtin_amdgcn_readlane(incl, 63);
    if (wave_total == 0) return;
    uint32_t base = 0;
    if (lane == 0) base = atomicAdd(a.n_items, (uint32_t)wave_total);
    base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
    uint32_t o = base + (uint32_t)(incl - cnt);
    if (!cnt) return;
    for (int k = 0; k < n_pieces; k++) {
        const uint32_t p = (uint32_t)(pieces >> (16 * k)) & 0xffffu;
        const int nx = (int)((p >> 10) & 7u), ny = (int)((p >> 13) & 7u);
        Rect c = cover, e = exact;
        if (split) {
            const int r0 = (int)(p & 31u), r1 = (int)((p >> 5) & 31u);
            c.x0 = tile_x0 + 8 * r0; c.x1 = imin(tile_x0 + 8 * r1 + 7, tile_x1);
            e.x0 = r0 == 0 ? exact.x0 : c.x0; e.x1 = r1 == ((tile_x1 - tile_x0) >> 3) ? exact.x1 : c.x1;
        }
        const int nb = (c.x1 - c.x0 + 8) >> 3, h = c.y1 - c.y0 + 1;
        const int pb = (nb + nx - 1) / nx, ph = (h + ny - 1) / ny;
        for (int jy = 0; jy < ny; jy++)
            for (int jx = 0; jx < nx; jx++, o++) {
                const int x0 = c.x0 + 8 * pb * jx, x1 = imin(x0 + 8 * pb - 1, c.x1);
                const int y0 = c.y0 + ph * jy, y1 = imin(y0 + ph - 1, c.y1);
                if (o >= a.cap_items) continue; // cannot happen: the list holds BOX_MAX_PARTS items per tile
                // (a part may come out empty by the rounding of the split: stored as such, the consumer skips it)
                a.items[o] = BoxItem::make(image, tile, x0, x1, y0, y1, e.x0, e.x1, e.y0, e.y1);
            }
    }
}

} // namespace

// A driver over the steps above: thread -> tile, the scan's box, the cluster decision, the routing (here; the cut of a gapped wide
// tile: split_at_gaps), the record and the clearing of the previous region, the wide entries, the items.
__global__ __launch_bounds__(256) void settle_tiles_kernel(BoxArgs a)
{
    if (a.zero8 && blockIdx.x == 0 && threadIdx.x < 8) a.zero8[threadIdx.x] = 0u; // the contour stage's walk counters
    const int n_all = a.n_clear > a.n_images ? a.n_clear : a.n_images;
    const TileOfThread t = tile_of_thread(a, n_all);
    if (t.valid && !a.dense && t.image < n_all) { // the buffer the NEXT batch's scan will widen -- read by the previous batch's settle -- is emptied
        const uint4 nxt = *(const uint4*)(a.tile_rows_next + 4 * t.idx);
        if (nxt.x <= nxt.y) *(uint4*)(a.tile_rows_next + 4 * t.idx) = NO_BOX;
    }
    const bool valid = t.valid && t.image < a.n_images; // (images beyond the batch: nothing else happens for them)
    const int tile = t.chunk * a.n_strips + t.strip;
    const int tile_r0 = t.chunk * a.rows_per_chunk, tile_r1 = imin(tile_r0 + a.rows_per_chunk, a.H) - 1;
    const int tile_x0 = 240 * t.strip, tile_x1 = imin(tile_x0 + 239, a.W - 1);
    Rect box;
    uint64_t quads;
    bool marked = scan_box(a, t, valid, box, quads);
    // output region of the tile: the box clipped to the tile, whole mask bytes
    Rect out{imax(box.x0, tile_x0) & ~7, imin(imin(box.x1, tile_x1) | 7, tile_x1), imax(box.y0, tile_r0), imin(box.y1, tile_r1)};
    if (marked && (out.x0 > out.x1 || out.y0 > out.y1)) marked = false;
    if (!marked) out = {1, 0, 1, 0};
    Rect cover = out, exact = box; // region the emitted items cover; box they take their exact pixels from
    const bool emits = marked && ((!a.dense && a.cluster) ? cluster_decision(a, t, cover, exact) : true);
    // routing: cut into items for the box kernel, or -- a wide box -- as the tile's rows through the sliding row pipeline, which
    // then writes the whole width of the tile; or, a wide box with empty columns in it, cut at them into items after all
    // (split_at_gaps): the region stays the box's, first run to last, and nobody writes the gaps
    int n_pieces = 0;
    uint64_t pieces = 0;
    bool wide = false, split = false;
    if (marked) {
        int nx, ny;
        const int nb = (cover.x1 - cover.x0 + 8) >> 3, h = cover.y1 - cover.y0 + 1;
        choose_split(nb, h, nx, ny);
        const int limit = ((a.remap_bits >> (t.image % a.cam_mod)) & 1ull) ? a.wide_quads_remap : a.wide_quads_identity;
        const bool own = cover.x0 == out.x0 && cover.x1 == out.x1 && cover.y0 == out.y0 && cover.y1 == out.y1; // no cluster item
        wide = emits && own && a.wide_tiles != nullptr && 2 * nb + 2 * nx >= limit;
        if (wide && a.wide_split && a.wide_bands == 1 && !a.dense) {
            n_pieces = split_at_gaps(tile_quad_bytes(quads), (out.x0 - tile_x0) >> 3, (out.x1 - tile_x0) >> 3, h, limit, pieces);
            split = n_pieces != 0;
            wide = !split;
        }
        if (wide) { out.x0 = tile_x0; out.x1 = tile_x1; cover.x0 = out.x0; cover.x1 = out.x1; }
        else if (emits && !split) { n_pieces = 1; pieces = piece_pack(0, 0, nx, ny); }
    }
    uint32_t prev_x = 1u, prev_y = 1u; // empty
    bool need_clear = valid && record_region(a, t, marked, out, box, prev_x, prev_y);
    // a split tile writes its runs only: what the previous batch left is cleared unless it lies inside ONE run's cover (the items
    // write later on this stream, so clearing the whole previous region is safe)
    if (split && span_first(prev_x) <= span_last(prev_x)) {
        need_clear = true;
        for (int k = 0; k < n_pieces; k++) {
            const uint32_t p = (uint32_t)(pieces >> (16 * k));
            const int x0 = tile_x0 + 8 * (int)(p & 31u), x1 = imin(tile_x0 + 8 * (int)((p >> 5) & 31u) + 7, tile_x1);
            if (x0 <= span_first(prev_x) && span_last(prev_x) <= x1 && out.y0 <= span_first(prev_y) && span_last(prev_y) <= out.y1) need_clear = false;
        }
    }
    clear_previous(a, need_clear, prev_x, prev_y, t.image);
    emit_wide(a, wide, t.image, tile, out.y0, out.y1);
    count_split(a, split);
    emit_items(a, n_pieces, pieces, split, t.image, tile, cover, exact, tile_x0, tile_x1);
}

void launch_settle_tiles(const BoxArgs& a, hipStream_t s)
{
    const int n_all = a.n_clear > a.n_images ? a.n_clear : a.n_images;
    const long long total = (long long)a.n_chunks * a.n_strips * a.cam_mod * ((n_all + a.cam_mod - 1) / a.cam_mod);
    hipLaunchKernelGGL(settle_tiles_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, a);
}

} // namespace mocap
