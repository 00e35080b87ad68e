// blob_rows_staged.hip -- the row pipeline of the filter stage on the compact undistort table, its source pixels staged in LDS.
//
// filter_mask_kernel<REMAP, PIPE> (blob_rows.hip) reads 8 bytes of table per pixel and gathers every tap pair from memory (ten vector
// memory instructions per 256-pixel row, eight of them 2-byte gathers): 10.6 ms per 3072 1080p images as the dense path, and
// per row just as much for the wide tiles of the sparse path.  This form reads the box kernel's 4-byte table (one 16-byte load
// per lane and row) and takes the taps from LDS: the rows of the strip are worked through in bands of up to 8; the
// rectangle of source pixels a band reads is known from a per-(row, strip) table made at set-up (rowbox), it is staged with
// coalesced dword loads, zeros outside the image (cv::remap's BORDER_CONSTANT), while the previous band is being filtered.
// Everything behind the remapped row -- horizontal sums, running vertical sums, threshold, window counts, majority -- is the
// code of that kernel (RowTail, rows_dev.h).  Requires W % 16 == 0 (16-byte staging units), H >= 2, every slot's table in the compact format.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>
#include "kernels.h"
#include "rows_dev.h"

namespace mocap {

constexpr int ROWS_LOADS = 9;                    // 16-byte staging loads per lane and band (always all of them: see stage_issue)
constexpr int ROWS_STAGE_U = 64 * ROWS_LOADS;    // 16-byte units of source pixels per wave and band (9 KB; 61 KB of LDS per workgroup in all)
constexpr int ROWS_STAGE_DW = 4 * ROWS_STAGE_U;

// source rectangle of a band in 16-byte units: origin (sxa a multiple of 16), pitch SP bytes = q units, SR rows, n units; its part
// inside the image: origin (ux0, iy0), iq units x iSR rows, first / last unit at li0 / llast of the rectangle
typedef uint32_t rows_u32x4 __attribute__((ext_vector_type(4))); // (a native vector: an array of HIP's uint4 filled by memcpy stays in scratch memory)
typedef rows_u32x4 rows_u32x4_any __attribute__((aligned(1)));   // ... at any address (unaligned access is enabled on amdhsa: one global_load_dwordx4)
struct BandRect { int sxa, sya, SP, SR, q, n; int ux0, iy0, iq, in, li0, llast; bool staged, interior; }; // source rectangle of a band: origin, pitch (bytes), rows, dwords per row, dwords

template <bool LIST>
__global__ __launch_bounds__(256) void filter_rows_staged_kernel(FilterArgs a)
{
    __shared__ uint32_t lut[256];
    __shared__ uint2 hring[4][8][64];
    __shared__ uint32_t cring[4][8][64];
    __shared__ rows_u32x4 sbuf[4][ROWS_STAGE_U];

    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6); // wave-uniform: keeps the row loop scalar

    RowsItem t;
    uint32_t it_first, it_end, it_step;
    if (!rows_wave_items<LIST>(a, wv, t, it_first, it_end, it_step)) return;
    fill_window_counts(lut, lane);
    rows_u32x4* const Sb = sbuf[wv];
    const uint8_t* const Sbytes = (const uint8_t*)Sb;
    // kernel arguments as plain scalars (a struct captured by the lambdas below would be kept in scratch memory)
    const int H = a.H, W = a.W, Hm1 = a.H - 1, pitch = a.pitch, stage_units = a.stage_dw >> 2, n_strips = a.n_strips, thr_mul = a.thr_mul;
    const int rows_per_chunk = a.rows_per_chunk, n_cgroups = a.n_cgroups, cam_mod = a.cam_mod, words_per_row = a.words_per_row;
    const uint8_t* __restrict__ const a_src = a.src; const size_t a_image_stride = a.image_stride;
    const uint32_t* __restrict__ const a_map4 = a.map4; const ushort4* __restrict__ const a_rowbox = a.rowbox;
    uint32_t* __restrict__ const a_mask = a.mask; uint32_t* __restrict__ const a_cells = a.cells; const uint4* __restrict__ const a_tiles = a.tiles;
    for (uint32_t it = it_first; it < it_end; it += it_step) {
        if (!rows_item<LIST>(t, it, a_tiles, H, rows_per_chunk, n_strips, n_cgroups, cam_mod)) continue;
        const int ks = t.ks, ke = t.ke;
        const uint8_t* __restrict__ img = a_src + (size_t)t.image * a_image_stride;
        const uint32_t* __restrict__ map4 = a_map4 + (size_t)t.slot * H * W;
        const ushort4* __restrict__ rbox = a_rowbox + (size_t)t.slot * H * n_strips + t.strip; // row r: rbox[r * n_strips]
        RowTail rt;
        rt.begin(hring[wv], cring[wv], lut, a_mask, words_per_row, lane, t, H, W, thr_mul);
        const LaneCols lc = lane_cols(rt.xl, W);
        const int y0 = t.kfirst - 2;

        // ---- bands: rectangle, staging, table words ----------------------------------------------------------------------
        // a lane's share of the rows' boxes (lanes 0..nr-1 hold one row each); reduced when the band is about to be staged
        auto rect_load = [&](int rb, int nr) __attribute__((always_inline)) -> ushort4 {
            int r = rb + (lane < nr ? lane : 0);
            r = r < 0 ? 0 : (r > Hm1 ? Hm1 : r);
            return rbox[(size_t)r * n_strips];
        };
        auto rect_reduce = [&](ushort4 p) __attribute__((always_inline)) -> BandRect {
            int xa = p.x, xb = p.y, ya = p.z, yb = p.w; // lanes beyond the band's rows hold a copy of its first row
#pragma unroll
            for (int d = 1; d <= 4; d <<= 1) {
                const int oxa = __shfl_xor(xa, d), oxb = __shfl_xor(xb, d), oya = __shfl_xor(ya, d), oyb = __shfl_xor(yb, d);
                xa = oxa < xa ? oxa : xa; xb = oxb > xb ? oxb : xb; ya = oya < ya ? oya : ya; yb = oyb > yb ? oyb : yb;
            }
            BandRect R;
            R.sxa = (__builtin_amdgcn_readfirstlane(xa) - 2) & ~15;
            const int sxb = __builtin_amdgcn_readfirstlane(xb) - 2;
            R.sya = __builtin_amdgcn_readfirstlane(ya) - 2;
            const int syb = __builtin_amdgcn_readfirstlane(yb) - 2;
            R.SP = (sxb - R.sxa + 16) & ~15; R.SR = syb - R.sya + 1; R.q = R.SP >> 4; R.n = R.SR * R.q;
            R.staged = R.n < stage_units; // (one unit is kept free: where the loads of a rectangle wholly outside the image end up)
            // the part inside the image: W % 16 == 0 and an origin that is a multiple of 16 put every unit entirely inside or outside
            const int ux1 = R.sxa + R.SP < W ? R.sxa + R.SP : W, iy1 = R.sya + R.SR < H ? R.sya + R.SR : H;
            R.ux0 = R.sxa > 0 ? R.sxa : 0; R.iy0 = R.sya > 0 ? R.sya : 0;
            R.iq = (ux1 - R.ux0) >> 4;
            const int iSR = iy1 - R.iy0;
            R.interior = R.iq == R.q && iSR == R.SR;
            if (R.iq <= 0 || iSR <= 0) { // nothing of it inside the image: one unit from somewhere valid, parked behind the rectangle
                R.iq = 1; R.in = 1; R.ux0 = 0; R.iy0 = 0; R.li0 = R.n; R.llast = R.n;
            } else {
                R.in = R.iq * iSR;
                R.li0 = (R.iy0 - R.sya) * R.q + ((R.ux0 - R.sxa) >> 4);
                R.llast = R.li0 + (iSR - 1) * R.q + R.iq - 1;
            }
            return R;
        };
        // The staging loads of a band: ROWS_LOADS 16-byte loads per lane, ALWAYS all of them and never inside a branch (the
        // counter that orders vector memory operations is counted at compile time: loads inside a branch make every later
        // wait a wait for all of them), all in flight while the previous band is filtered.  Lane -> units lane, lane + 64, ... of
        // the rectangle's part inside the image, row-major; the address and the place in LDS walk on by wave-uniform steps with a
        // carry into the next row (no division, no clamps); units past the end repeat the last one (same address, same place).
        struct StageWalk { int c; uint32_t goff; int li; };
        auto stage_walk = [&](const BandRect& R, StageWalk& w, int& rem, uint32_t& gstep, uint32_t& gcarry, int& lstep, int& lcarry, uint32_t& glast) __attribute__((always_inline)) {
            const float rcpd = __builtin_amdgcn_rcpf((float)R.iq);
            const int qr = (int)(64.5f * rcpd); // 64 = qr * iq + rem
            rem = 64 - qr * R.iq;
            const int r0_ = (int)(((float)lane + 0.5f) * rcpd);
            w.c = lane - r0_ * R.iq;
            w.goff = (uint32_t)(R.iy0 + r0_) * (uint32_t)pitch + (uint32_t)(R.ux0 + 16 * w.c);
            w.li = R.li0 + r0_ * R.q + w.c;
            gstep = (uint32_t)qr * (uint32_t)pitch + 16u * (uint32_t)rem; gcarry = (uint32_t)pitch - 16u * (uint32_t)R.iq;
            lstep = qr * R.q + rem; lcarry = R.q - R.iq;
            const int rl = (R.in - 1) / R.iq; // (scalar)
            glast = (uint32_t)(R.iy0 + rl) * (uint32_t)pitch + (uint32_t)(R.ux0 + 16 * (R.in - 1 - rl * R.iq));
        };
        auto stage_issue = [&](const BandRect& R, rows_u32x4 (&v)[ROWS_LOADS]) __attribute__((always_inline)) {
            StageWalk w; int rem, lstep, lcarry; uint32_t gstep, gcarry, glast;
            stage_walk(R, w, rem, gstep, gcarry, lstep, lcarry, glast);
#pragma unroll
            for (int u = 0; u < ROWS_LOADS; u++) {
                const uint32_t g = w.goff < glast ? w.goff : glast;
                v[u] = *(const rows_u32x4_any*)(img + g);
                w.c += rem; w.goff += gstep;
                if (w.c >= R.iq) { w.c -= R.iq; w.goff += gcarry; }
            }
        };
        auto stage_write = [&](const BandRect& R, const rows_u32x4 (&v)[ROWS_LOADS]) __attribute__((always_inline)) {
            // A band that is not staged takes its taps from memory and never reads Sb.  Its rectangle has R.n >= stage_units
            // units, so the store index below (clamped only to R.llast < R.n) may lie past this wave's buffer -- in the next
            // wave's, or past sbuf for wave 3.  No store then (R.staged is wave-uniform: a scalar branch; clamping the index
            // to ROWS_STAGE_U - 1 instead would still write 9 KB of LDS nobody reads).  The loads in stage_issue stay
            // unconditional.
            if (!R.staged) return;
            if (!R.interior) { // units outside the image read 0 (cv::remap's BORDER_CONSTANT): clear, then the inside part on top
#pragma unroll
                for (int u = 0; u < ROWS_LOADS; u++) Sb[lane + 64 * u] = rows_u32x4{0u, 0u, 0u, 0u};
            }
            StageWalk w; int rem, lstep, lcarry; uint32_t gstep, gcarry, glast;
            stage_walk(R, w, rem, gstep, gcarry, lstep, lcarry, glast);
#pragma unroll
            for (int u = 0; u < ROWS_LOADS; u++) {
                Sb[w.li < R.llast ? w.li : R.llast] = v[u];
                w.c += rem; w.li += lstep;
                if (w.c >= R.iq) { w.c -= R.iq; w.li += lcarry; }
            }
        };
        auto table_issue = [&](uint4& tw, int row) __attribute__((always_inline)) {
            const int rc = row < 0 ? 0 : (row > Hm1 ? Hm1 : row);
            __builtin_memcpy(&tw, map4 + ((uint32_t)rc * (uint32_t)W + (uint32_t)lc.addr_x), 16);
        };
        // one remapped row of the strip: the lane's four pixels, blended exactly as cv::remap's fixed point does
        // (STAGED is a compile-time flag chosen once per band: a branch inside every row would cut the unrolled rows into separate
        // basic blocks, and the tap reads of one row could no longer be scheduled under the arithmetic of the previous one)
        auto blend_row = [&](auto staged_c, const uint4& tw, int row, const BandRect& R) __attribute__((always_inline)) -> uint32_t {
            constexpr bool STAGED = decltype(staged_c)::value;
            const int rc = row < 0 ? 0 : (row > Hm1 ? Hm1 : row);
            const uint32_t ww[4] = {tw.x, tw.y, tw.z, tw.w};
            uint32_t B = 0;
            if (STAGED) {
                const int rowbase = __mul24(rc - R.sya, R.SP) + (lc.addr_x - R.sxa);
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const Map4 m = map4_decode(ww[k]);
                    const int A0 = __mul24(m.dy, R.SP) + (rowbase + k) + m.dx;
                    B |= map4_blend(m, Sbytes[A0], Sbytes[A0 + 1], Sbytes[A0 + R.SP], Sbytes[A0 + R.SP + 1]) << (8 * k);
                }
            } else { // the band's source rectangle outgrew the buffer (strong local distortion): taps from memory
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const Map4 m = map4_decode(ww[k]);
                    const int sx = lc.addr_x + k + m.dx, sy = rc + m.dy;
                    const int sx0 = sx < 0 ? 0 : (sx > W - 1 ? W - 1 : sx), sx1 = sx + 1 < 0 ? 0 : (sx + 1 > W - 1 ? W - 1 : sx + 1);
                    const int sy0 = sy < 0 ? 0 : (sy > Hm1 ? Hm1 : sy), sy1 = sy + 1 < 0 ? 0 : (sy + 1 > Hm1 ? Hm1 : sy + 1);
                    const uint32_t o0 = (uint32_t)sy0 * (uint32_t)pitch, o1 = (uint32_t)sy1 * (uint32_t)pitch;
                    const uint32_t t00 = img[o0 + (uint32_t)sx0], t01 = img[o0 + (uint32_t)sx1], t10 = img[o1 + (uint32_t)sx0], t11 = img[o1 + (uint32_t)sx1];
                    const bool c0 = sx0 == sx, c1 = sx1 == sx + 1, q0 = sy0 == sy, q1 = sy1 == sy + 1;
                    B |= map4_blend(m, (c0 && q0) ? t00 : 0u, (c1 && q0) ? t01 : 0u, (c0 && q1) ? t10 : 0u, (c1 && q1) ? t11 : 0u) << (8 * k);
                }
            }
            return (unsigned)row < (unsigned)H ? (B & lc.bytemask) : 0u; // rows and columns outside the image do not exist
        };
        // ---- band 0: the five rows y0 .. y0 + 4 of the set-up (ring slots 3 .. 7) ------------------------------------------
        uint4 tc[8], tn[8];  // table words of the band being filtered / of the next one
        rows_u32x4 sv[ROWS_LOADS]; // staging loads in flight
        BandRect Rc = rect_reduce(rect_load(y0, 5));
        stage_issue(Rc, sv);
#pragma unroll
        for (int j = 0; j < 5; j++) table_issue(tc[3 + j], y0 + j);
        // band 1 = the first rows of the steady loop: y0 + 5 = ks + 2 onwards
        int nr_next = ke - ks + 1 < 8 ? ke - ks + 1 : 8;
        ushort4 part = rect_load(ks + 2, nr_next > 0 ? nr_next : 1);
        stage_write(Rc, sv);
        // the next band's loads are issued before the current one is filtered, and land in LDS after it.  Every band does this,
        // the last one too (its successor's rows are clamped into the image and never used): no branch around a load
        BandRect Rn = Rc;
        auto prefetch = [&](int first_row, int nr) __attribute__((always_inline)) { // rows first_row .. first_row + nr - 1 -> tn / sv
            Rn = rect_reduce(part);
            stage_issue(Rn, sv);
#pragma unroll
            for (int j = 0; j < 8; j++) table_issue(tn[j], first_row + (j < nr ? j : nr - 1));
        };
        auto commit = [&]() __attribute__((always_inline)) { // the band just filtered has read its last tap: the next one moves in
            stage_write(Rn, sv);
#pragma unroll
            for (int j = 0; j < 8; j++) tc[j] = tn[j];
            Rc = Rn;
        };
        prefetch(ks + 2, nr_next > 0 ? nr_next : 1);
        {
            const int n2 = ke - (ks + 8) + 1 < 8 ? ke - (ks + 8) + 1 : 8;
            part = rect_load(ks + 10, n2 > 0 ? n2 : 1); // (the band after that one: its box loads have a whole band's time)
        }
        auto setup_rows = [&](auto staged_c) __attribute__((always_inline)) {
            rt.hsum_update(blend_row(staged_c, tc[3], y0, Rc), 3, 6);
            rt.hsum_update(blend_row(staged_c, tc[4], y0 + 1, Rc), 4, 7);
            rt.hsum_update(blend_row(staged_c, tc[5], y0 + 2, Rc), 5, 0);
            rt.hsum_update(blend_row(staged_c, tc[6], y0 + 3, Rc), 6, 1);
            rt.hsum_update(blend_row(staged_c, tc[7], y0 + 4, Rc), 7, 2);
        };
        if (Rc.staged) setup_rows(std::true_type{}); else setup_rows(std::false_type{});
        rt.top(t);
        // ---- steady state: bands of 8 rows; one source row in, one threshold row, one output row per step -------------------
        auto step = [&](auto staged_c, auto Jc, int k) __attribute__((always_inline)) {
            constexpr int J = decltype(Jc)::value;
            rt.template step<J>(blend_row(staged_c, tc[J], k + 2, Rc), k);
        };
        auto band_steps = [&](auto staged_c, int k, int nst) __attribute__((always_inline)) {
            if (nst == 8) { // one basic block: the rows' LDS reads and arithmetic interleave
                step(staged_c, IC<0>{}, k); step(staged_c, IC<1>{}, k + 1); step(staged_c, IC<2>{}, k + 2); step(staged_c, IC<3>{}, k + 3);
                step(staged_c, IC<4>{}, k + 4); step(staged_c, IC<5>{}, k + 5); step(staged_c, IC<6>{}, k + 6); step(staged_c, IC<7>{}, k + 7);
            } else {
                step(staged_c, IC<0>{}, k);
                if (nst > 1) step(staged_c, IC<1>{}, k + 1);
                if (nst > 2) step(staged_c, IC<2>{}, k + 2);
                if (nst > 3) step(staged_c, IC<3>{}, k + 3);
                if (nst > 4) step(staged_c, IC<4>{}, k + 4);
                if (nst > 5) step(staged_c, IC<5>{}, k + 5);
                if (nst > 6) step(staged_c, IC<6>{}, k + 6);
            }
        };
        for (int k = ks; k <= ke; k += 8) {
            commit(); // (the band of this iteration)
            const int nst = ke - k + 1 < 8 ? ke - k + 1 : 8;
            {
                const int n1 = ke - (k + 8) + 1 < 8 ? ke - (k + 8) + 1 : 8, n2 = ke - (k + 16) + 1 < 8 ? ke - (k + 16) + 1 : 8;
                prefetch(k + 10, n1 > 0 ? n1 : 1);
                part = rect_load(k + 18, n2 > 0 ? n2 : 1);
            }
            if (Rc.staged) band_steps(std::true_type{}, k, nst); else band_steps(std::false_type{}, k, nst);
        }
        rt.template bottom<LIST>(t, a_cells);
    } // strips / list entries
}

int rows_stage_dwords() { return ROWS_STAGE_DW; }

void launch_filter_rows_staged(const FilterArgs& a, bool list, int blocks, hipStream_t s)
{
    if (list) hipLaunchKernelGGL(filter_rows_staged_kernel<true>, dim3(blocks), dim3(256), 0, s, a);
    else hipLaunchKernelGGL(filter_rows_staged_kernel<false>, dim3(blocks), dim3(256), 0, s, a);
}

} // namespace mocap
