// rows_dev.h -- what the two row-pipeline kernels of the filter stage share (filter_mask_kernel in blob_rows.hip,
// filter_rows_staged_kernel in blob_rows_staged.hip): which strip or list entry a wave works on, and everything behind the
// remapped row.  How the four pixels of a lane's row come about (the source-row queue and the gathers of the one, the bands staged
// in LDS of the other) stays in each kernel.
#pragma once
#include "filter_dev.h"

namespace mocap {

// One piece of work of a wave: a strip of 256 source columns (240 of output) of one tile, or the band of it a list entry names.
struct RowsItem {
    int image, slot, chunk, strip;
    int tile_r0, tile_r1; // the tile's mask rows [tile_r0, tile_r1)
    int r0, r1;           // the rows filtered
    int kfirst;           // first threshold row: the set-up slides source rows kfirst - 2 .. kfirst + 2
    int ks, ke;           // steady range: every iteration slides one source row
    size_t cell_index;    // the tile's occupancy word
};

// The pieces of wave `wv` of this workgroup: it_first, it_first + it_step, ... below it_end.  Dense form: workgroup -> (camera
// slot, group of 4 chunks, time step), the wave takes one chunk and walks its strips.  LIST: instead of every tile of every image,
// the waves work through a list of (image, tile, first row, last row) entries -- the tiles whose boxes settle_tiles_kernel found
// too wide for the box kernel to be the cheaper way.  false: nothing for this wave.
template <bool LIST>
__device__ __forceinline__ bool rows_wave_items(const FilterArgs& a, int wv, RowsItem& t, uint32_t& it_first, uint32_t& it_end, uint32_t& it_step)
{
    t.slot = 0; t.image = 0; t.chunk = 0;
    uint32_t n_list = 0;
    if (LIST) {
        n_list = *a.n_tiles;
        n_list = n_list < a.cap_tiles ? n_list : a.cap_tiles;
        if ((uint32_t)(blockIdx.x * 4 + wv) >= n_list) return false;
    } else {
        const TileId tid_ = decode_tile(a, blockIdx.x);
        if (!tid_.valid) return false;
        t.slot = tid_.slot; t.image = tid_.image;
        t.chunk = tid_.cgroup * 4 + wv;
        if (t.chunk * a.rows_per_chunk >= a.H) return false;
    }
    it_first = LIST ? (uint32_t)(blockIdx.x * 4 + wv) : 0u; it_end = LIST ? n_list : (uint32_t)a.n_strips;
    it_step = LIST ? gridDim.x * 4u : 1u;
    return true;
}

// Piece `it` of the wave: strip `it` of its chunk, or list entry `it`.  false: an empty band.
// (Kernel arguments come as plain scalars: a struct that the kernels' lambdas capture would be kept in scratch memory.)
template <bool LIST>
__device__ __forceinline__ bool rows_item(RowsItem& t, uint32_t it, const uint4* __restrict__ tiles, int H, int rows_per_chunk, int n_strips,
                                          int n_cgroups, int cam_mod)
{
    t.strip = (int)it;
    int r0e = 0, r1e = 0x7fffffff;
    if (LIST) {
        const WideTile e = wide_tile_unpack(tiles[it]);
        t.image = __builtin_amdgcn_readfirstlane(e.image);
        const int tile = __builtin_amdgcn_readfirstlane(e.tile);
        r0e = __builtin_amdgcn_readfirstlane(e.y0); r1e = __builtin_amdgcn_readfirstlane(e.y1) + 1;
        t.chunk = tile / n_strips; t.strip = tile - t.chunk * n_strips;
        t.slot = t.image % cam_mod;
    }
    t.tile_r0 = t.chunk * rows_per_chunk;
    t.tile_r1 = t.tile_r0 + rows_per_chunk < H ? t.tile_r0 + rows_per_chunk : H;
    t.cell_index = ((size_t)t.image * n_cgroups * 4 + t.chunk) * n_strips + t.strip;
    t.r0 = r0e > t.tile_r0 ? r0e : t.tile_r0; t.r1 = r1e < t.tile_r1 ? r1e : t.tile_r1;
    if (LIST && t.r0 >= t.r1) return false;
    const int Hm1 = H - 1;
    t.kfirst = t.r0 - 2;
    t.kfirst = t.kfirst < 0 ? 0 : (t.kfirst > Hm1 ? Hm1 : t.kfirst);
    t.ks = t.r0 - 1 > 1 ? t.r0 - 1 : 1;
    t.ke = t.r1 + 1 < Hm1 ? t.r1 + 1 : Hm1;
    return true;
}

// Behind the remapped row.  A lane holds four neighbouring pixels of the strip's current source row (columns xl .. xl + 3, one byte
// each); horizontal neighbours come from DPP wave shifts, byte sums from v_dot4_u32_u8, the vertical 5-row windows are running
// sums whose history sits in this wave's LDS rings.  In the order of a strip: begin, five source rows through hsum_update, top,
// one step per source row of the steady range, bottom.
struct RowTail {
    uint2 (*hring)[64];    // this wave's rings in LDS, 8 slots each: the rows' horizontal 5-sums (16-bit fields) ...
    uint32_t (*cring)[64]; // ... and the packed window counts of the thresholded rows
    const uint32_t* lut;   // window-count table (fill_window_counts)
    uint8_t* mrow_base;    // the image's mask
    int wpr, H, thr_mul, r0, tile_r0;
    int lane, xl, lane_r, bit_r, out_byte;
    bool left_edge, right_edge, stores;
    uint32_t cx01, cx23, colmask; // per-lane column constants: in-image taps of the four columns' windows, columns inside the image
    uint32_t V01, V23, Cv, c_cur;
    uint32_t lacc;         // per lane: bit g = this lane's columns have set pixels in output rows tile_r0+8g .. tile_r0+8g+7

    __device__ __forceinline__ void begin(uint2 (*hring_)[64], uint32_t (*cring_)[64], const uint32_t* lut_, uint32_t* mask, int words_per_row,
                                          int lane_, const RowsItem& t, int H_, int W, int thr_mul_)
    {
        hring = hring_; cring = cring_; lut = lut_; lane = lane_;
        wpr = words_per_row; H = H_; thr_mul = thr_mul_; r0 = t.r0; tile_r0 = t.tile_r0;
        mrow_base = (uint8_t*)(mask + (size_t)t.image * mask_image_words(H, wpr));
        const int row_bytes = wpr * 4;
        const int xbase = t.strip * 240 - 8;
        xl = xbase + 4 * lane;
        colmask = 0;
        {
            int c0 = taps5(xl, W), c1 = taps5(xl + 1, W), c2 = taps5(xl + 2, W), c3 = taps5(xl + 3, W);
            cx01 = (uint32_t)(c0 & 0xffff) | ((uint32_t)c1 << 16);
            cx23 = (uint32_t)(c2 & 0xffff) | ((uint32_t)c3 << 16);
#pragma unroll
            for (int k = 0; k < 4; k++)
                if ((unsigned)(xl + k) < (unsigned)W) colmask |= 1u << k;
        }
        left_edge = xbase < 0;
        right_edge = xbase + 255 >= W;
        lane_r = (W - 1 - xbase) >> 2; bit_r = (W - 1 - xbase) & 3; // lane / bit of column W-1
        // byte of the output row written by this (even) lane
        out_byte = t.strip * 30 + ((lane - 2) >> 1);
        stores = ((lane & 1) == 0) && lane >= 2 && lane <= 60 && out_byte < ((W + 7) >> 3) && out_byte < row_bytes;
        V01 = 0; V23 = 0; Cv = 0; c_cur = 0; lacc = 0;
#pragma unroll
        for (int s = 0; s < 8; s++) {
            hring[s][lane] = make_uint2(0u, 0u);
            cring[s][lane] = 0u;
        }
    }
    // horizontal 5-sums of one source row -> vertical running sums (history in the LDS ring)
    __device__ __forceinline__ void hsum_update(uint32_t B, int s_new, int s_old)
    {
        uint32_t A = lane_from_prev(B), C = lane_from_next(B);
        uint32_t sB = dot4(B, 0x01010101u, 0u);
        uint32_t h0 = dot4(A, 0x01010000u, dot4(B, 0x00010101u, 0u));
        uint32_t h1 = dot4(A, 0x01000000u, sB);
        uint32_t h2 = dot4(C, 0x00000001u, sB);
        uint32_t h3 = dot4(C, 0x00000101u, dot4(B, 0x01010100u, 0u));
        uint32_t H01 = h0 | (h1 << 16), H23 = h2 | (h3 << 16);
        uint2 old = hring[s_old][lane];
        hring[s_new][lane] = make_uint2(H01, H23);
        V01 += H01 - old.x; // 16-bit fields never borrow: the window sum always contains the row removed
        V23 += H23 - old.y;
    }
    // threshold row kc from the running sums -> packed horizontal 5-window counts of the thresholded row
    __device__ __forceinline__ uint32_t thresh_counts(int kc)
    {
        uint32_t m = (uint32_t)(thr_mul * taps5(kc, H));
        uint32_t T01 = __umul24(cx01, m), T23 = __umul24(cx23, m);
        uint32_t d01 = (V01 | 0x80008000u) - T01, d23 = (V23 | 0x80008000u) - T23;
        uint32_t t = (d01 >> 15) & 0x10001u, u = (d23 >> 15) & 0x10001u;
        uint32_t w = t | (u << 2);
        uint32_t nib = (w | (w >> 15)) & 0xfu;
        // medianBlur replicates the border: columns outside the image take the edge column's bit
        if (left_edge) {
            uint32_t e = __builtin_amdgcn_readlane(nib, 2) & 1u;
            if (xl < 0) nib = e ? 0xfu : 0u;
        }
        if (right_edge) {
            uint32_t e = (__builtin_amdgcn_readlane(nib, lane_r) >> bit_r) & 1u;
            uint32_t keep = (2u << bit_r) - 1u;
            if (lane > lane_r) nib = e ? 0xfu : 0u;
            else if (lane == lane_r) nib = (nib & keep) | (e ? (0xfu & ~keep) : 0u);
        }
        uint32_t nl = lane_from_prev(nib), nr = lane_from_next(nib);
        uint32_t win = (nl >> 2) | (nib << 2) | ((nr & 3u) << 6);
        return lut[win];
    }
    __device__ __forceinline__ void push_counts(uint32_t c, int s_new, int s_old)
    {
        uint32_t cold = cring[s_old][lane];
        cring[s_new][lane] = c;
        Cv += c - cold;
    }
    // majority (>= 13 of 25) of output row `row`, two lanes -> one byte of the bit mask
    __device__ __forceinline__ void emit(int row, bool on)
    {
        uint32_t mm = ((Cv + 0x73737373u) >> 7) & 0x01010101u;
        uint32_t t1 = mm | (mm >> 7);
        uint32_t mn = (t1 | (t1 >> 14)) & colmask;
        lacc |= (mn != 0u ? 1u : 0u) << (((on ? row : r0) - tile_r0) >> 3); // rows not yet valid have mn from a partial window: harmless superset
        uint32_t odd = lane_from_next(mn);
        uint32_t byte = (mn & 0xfu) | ((odd & 0xfu) << 4);
        // direct byte store: all loads of the two kernels are global-address-space loads, so the compiler keeps counted vmcnt
        // waits around this exec-masked store and the load pipeline stays full
        if (stores && on) mrow_base[mask_byte_index(row, out_byte, wpr)] = (uint8_t)byte;
    }
    // behind the set-up's five source rows (ring slots 3..7): the first threshold row and the replicated rows above the image
    __device__ __forceinline__ void top(const RowsItem& t)
    {
        c_cur = thresh_counts(t.kfirst);
        // count-ring phase chosen so that the steady loop starts at slot 0: pushes so far = 1 (+2 at the image top)
        int cj = (r0 == 0) ? 5 : 7;
        push_counts(c_cur, cj & 7, (cj + 3) & 7);
        cj++;
        for (int kk = r0 - 1; kk < t.ks; ++kk) { // rows above the image replicate row 0 (only the top chunk gets here)
            push_counts(c_cur, cj & 7, (cj + 3) & 7);
            cj++;
            if (kk >= r0 + 2) emit(kk - 2, true);
        }
    }
    // steady state: source row k + 2 in (its pixels B; ring slot J of both rings), threshold row k, output row k - 2
    template <int J>
    __device__ __forceinline__ void step(uint32_t B, int k)
    {
        hsum_update(B, J, (J + 3) & 7);
        c_cur = thresh_counts(k);
        push_counts(c_cur, J, (J + 3) & 7);
        emit(k - 2, k >= r0 + 2);
    }
    // behind the steady range: the replicated rows below the image (only the bottom chunk gets any), then the occupancy word of
    // this (strip, chunk): OR of the output lanes' bits
    template <bool LIST>
    __device__ __forceinline__ void bottom(const RowsItem& t, uint32_t* __restrict__ cells)
    {
        int n_steady = t.ke >= t.ks ? t.ke - t.ks + 1 : 0;
        int cj = n_steady; // slot of the next push (the steady loop started at slot 0)
        int kb = t.ke + 1 > t.ks ? t.ke + 1 : t.ks;
        for (int kk = kb; kk <= t.r1 + 1; ++kk) {
            push_counts(c_cur, cj & 7, (cj + 3) & 7);
            cj++;
            if (kk >= r0 + 2) emit(kk - 2, true);
        }
        const bool out_lane = lane >= 2 && lane <= 61;
        uint32_t cellmask = 0;
        const int groups = (t.tile_r1 - t.tile_r0 + 7) >> 3;
        for (int g = 0; g < groups; g++)
            if (__ballot(out_lane && ((lacc >> g) & 1u)) != 0ull) cellmask |= 1u << g;
        // bit 31 marks a filtered tile; bits 0..16 are the groups (list form: several bands of a tile add their bits)
        if (lane == 0) { if (LIST) atomicOr(&cells[t.cell_index], cellmask | 0x80000000u); else cells[t.cell_index] = cellmask | 0x80000000u; }
    }
};

} // namespace mocap
