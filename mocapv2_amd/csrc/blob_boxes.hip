// blob_boxes.hip -- the sparse half of the filter stage: undistort -> 5x5 in-bounds box sum -> threshold -> 5x5 majority,
// run only where the streaming scan (bright_cells_kernel, blob_scan.hip) could not prove the mask to be zero.
//
// Replaces, for the boxes of one batch of camera images,
//   cv.undistort (reference lib/ImageOperations.py:38) -> fast_cuda_blur (lib/CudaOperations.py:5-41)
//   -> cv.threshold (lib/ImageOperations.py:29) -> cv.medianBlur (lib/ImageOperations.py:30).
//
// Two kernels per batch, behind the scan:
//   settle_tiles_kernel  (blob_settle.hip) turns the box the scan left on every tile into work items of a bounded size in ONE
//                        global list, or -- a wide box -- into entries for the sliding row pipeline of blob_rows.hip;
//   box_filter_kernel    a fixed grid of single-wave workgroups consumes the list.  One wave owns one item and keeps
//                        everything in LDS: the source pixels its undistortion reads (staged with coalesced row loads,
//                        zero border = cv::remap's BORDER_CONSTANT), the horizontal 5-sums of the undistorted patch, the
//                        packed window counts of the thresholded rows.  Lanes are dealt (row, 4-pixel quad) pairs
//                        compactly -- a 72-pixel-wide box keeps 60 of 64 lanes busy with three rows per instruction --
//                        and horizontal neighbours come from DPP wave shifts.  The undistort table is one 4-byte word per
//                        pixel (11-bit displacements, 5-bit fractions), read with one 16-byte load per quad.
// No workgroup barrier anywhere: a wave never waits for another one; items are taken from the list dynamically (one atomic
// per item on one of 8 per-XCD run heads), so waves with expensive items simply take fewer.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>
#include "boxes_dev.h"

namespace mocap {

#ifndef MOCAP_BOX_GROUP      // (build-time knobs for A/B builds: scratch/build_variant.sh)
#define MOCAP_BOX_GROUP 3
#endif
#ifndef MOCAP_BOX_SU
#define MOCAP_BOX_SU 7
#endif
#ifndef MOCAP_BOX_WAVES
#define MOCAP_BOX_WAVES 4
#endif
constexpr int BOX_GROUP = MOCAP_BOX_GROUP; // trips whose table / frame loads are issued together

namespace {

// ---- the item queue ----------------------------------------------------------------------------------------------------------
// The list is cut into 8 runs of consecutive items, one per XCD (blocks b and b + 8 share an XCD; consecutive items share
// undistort-table lines, see settle).  A wave takes the next item of its run with one atomic add on the run's head word
// -- requested an item ahead, so its latency hides behind the filtering -- and moves on to the next run when its own is
// exhausted: items differ in cost, a fixed deal left the busiest wave with 1.4x the mean.
constexpr uint32_t NO_ITEM = 0xffffffffu;
struct ItemQueue {
    uint32_t* heads; // 8 head words, 64 bytes apart
    uint32_t n_items;
    int shard, tries;
    // the atomic's round trip hides behind an item's work: request now, look later
    __device__ __forceinline__ uint32_t request() const
    {
        uint32_t i = 0;
        if (threadIdx.x == 0 && tries < 8) i = atomicAdd(heads + 16 * shard, 1u);
        return i;
    }
    // index of the item a request got, or NO_ITEM when the list is exhausted; a run that is exhausted: the next ones, synchronously
    // (the tail of the kernel only)
    __device__ __forceinline__ uint32_t resolve(uint32_t i)
    {
        for (;;) {
            if (tries >= 8) return NO_ITEM;
            const uint32_t lo = (uint32_t)(((uint64_t)n_items * (uint32_t)shard) >> 3), hi = (uint32_t)(((uint64_t)n_items * (uint32_t)(shard + 1)) >> 3);
            i = (uint32_t)__builtin_amdgcn_readfirstlane((int)i);
            if (i < hi - lo) return lo + i;
            tries++;
            shard = (shard + 1) & 7;
            i = request();
        }
    }
    __device__ __forceinline__ uint32_t take() { return resolve(request()); }
};

// ---- an item's lanes ---------------------------------------------------------------------------------------------------------
// Lane -> (rsub, q): q = lane % Q the quad, rsub = lane / Q the row of the trip; trip k handles rows k * rpw + rsub.
struct BoxLane {
    int rpw, rsub, q;
    bool lane_on;               // the lane has a row in every trip
    int x;                      // first column of the quad
    uint32_t bytemask, colmask; // columns of the quad inside the image: 0xff per byte / one bit each
};
__device__ __forceinline__ BoxLane box_lane(const BoxGeom& g, int W)
{
    BoxLane L;
    const int lane = threadIdx.x;
    const float rcpQ = __builtin_amdgcn_rcpf((float)g.Q);
    L.rpw = small_div(64, rcpQ);
    L.rsub = small_div(lane, rcpQ); L.q = lane - L.rsub * g.Q;
    L.lane_on = L.rsub < L.rpw;
    L.x = g.px0 + 4 * L.q;
    L.bytemask = 0; L.colmask = 0;
#pragma unroll
    for (int k = 0; k < 4; k++)
        if ((unsigned)(L.x + k) < (unsigned)W) { L.bytemask |= 0xffu << (8 * k); L.colmask |= 1u << k; }
    return L;
}
// Where the exact region lies among the trips of pass A: patch rows outside it are zeros, trips [0, ka0) and [ka1, ntrip) hold
// none of its rows; its trips are worked through in `ngroup` groups of BOX_GROUP.  Lanes outside it load from a quad of it
// (column xc) and drop the result.
struct ExactTrips { int ntrip, ka0, ka1, ngroup, xc; bool q_exact; };
__device__ __forceinline__ ExactTrips exact_trips(const BoxGeom& g, const BoxLane& L)
{
    ExactTrips T;
    T.ntrip = (g.PR + L.rpw - 1) / L.rpw;
    T.ka0 = g.exact ? (g.ey0 - g.hy0) / L.rpw : T.ntrip; T.ka1 = g.exact ? (g.ey1 - g.hy0) / L.rpw + 1 : T.ntrip;
    T.ngroup = (T.ka1 - T.ka0 + BOX_GROUP - 1) / BOX_GROUP;
    T.q_exact = L.q >= g.eq0 && L.q <= g.eq1;
    const int qc = L.q < g.eq0 ? g.eq0 : (L.q > g.eq1 ? g.eq1 : L.q);
    T.xc = imax(g.px0 + 4 * qc, 0);
    return T;
}
// row of the exact region that trip kt's lane reads (clamped into it), and whether the lane's pixels belong to it
__device__ __forceinline__ int exact_row(const BoxGeom& g, int y) { return y < g.ey0 ? g.ey0 : (y > g.ey1 ? g.ey1 : y); }
__device__ __forceinline__ bool in_exact(const BoxGeom& g, const ExactTrips& T, int y) { return T.q_exact && y >= g.ey0 && y <= g.ey1; }

// entry of row r (of nrows, counted from the buffer's first row) and this lane's quad in Hs / Cs; lanes without such a row park
// their store behind the buffer
__device__ __forceinline__ int lane_slot(const BoxGeom& g, const BoxLane& L, int r, int nrows)
{
    return (L.lane_on && r < nrows) ? __mul24(r, g.Q) + L.q : BOX_HCAP + (int)threadIdx.x;
}

// ---- pass A: undistorted patch -> horizontal 5-sums of every patch row, in LDS ----------------------------------------------
// hsum of patch row r's quad B (4 bytes): packed 16-bit sums of the 5 columns around each pixel
__device__ __forceinline__ void store_h(uint2* Hs, const BoxGeom& g, const BoxLane& L, uint32_t B, int r)
{
    const uint32_t A = lane_from_prev(B), C = lane_from_next(B);
    const uint32_t sB = dot4(B, 0x01010101u, 0u);
    const uint32_t h0 = dot4(A, 0x01010000u, dot4(B, 0x00010101u, 0u));
    const uint32_t h1 = dot4(A, 0x01000000u, sB);
    const uint32_t h2 = dot4(C, 0x00000001u, sB);
    const uint32_t h3 = dot4(C, 0x00000101u, dot4(B, 0x01010100u, 0u));
    Hs[lane_slot(g, L, r, g.PR)] = make_uint2(h0 | (h1 << 16), h2 | (h3 << 16));
}
__device__ __forceinline__ void zero_rows_outside(uint2* Hs, const BoxGeom& g, const BoxLane& L, const ExactTrips& T)
{
    for (int k = 0; k < T.ntrip; k++) {
        if (k == T.ka0) k = T.ka1;
        if (k >= T.ntrip) break;
        Hs[lane_slot(g, L, k * L.rpw + L.rsub, g.PR)] = make_uint2(0u, 0u);
    }
}
// Source 1, the identity map: the patch is the frame.  BAYER: the same rows, each lane's gray dword formed from the Bayer rows
// above, at and below it.
template <bool BAYER>
__device__ __forceinline__ void identity_rows(uint2* Hs, const BoxGeom& g, const BoxLane& L, const ExactTrips& T, const uint8_t* __restrict__ img,
                                              int pitch, int W, int H, const BayerK& bk)
{
    using Raw = std::conditional_t<BAYER, BayerWin, uint32_t>;
    const int ax = T.xc > W - 4 ? W - 4 : T.xc; // W >= 4
    const uint32_t sh = (uint32_t)((T.xc - ax) * 8);
    auto load_rows = [&](Raw (&raw)[BOX_GROUP], int gi) __attribute__((always_inline)) {
#pragma unroll
        for (int u = 0; u < BOX_GROUP; u++) {
            const int yc = exact_row(g, g.hy0 + (T.ka0 + gi * BOX_GROUP + u) * L.rpw + L.rsub);
            if constexpr (BAYER) bayer_win_load(raw[u], img, pitch, W, H, ax, yc);
            else __builtin_memcpy(&raw[u], img + ((uint32_t)yc * (uint32_t)pitch + (uint32_t)ax), 4);
        }
    };
    auto use_rows = [&](const Raw (&raw)[BOX_GROUP], int gi) __attribute__((always_inline)) {
#pragma unroll
        for (int u = 0; u < BOX_GROUP; u++) {
            const int kt = T.ka0 + gi * BOX_GROUP + u, r = kt * L.rpw + L.rsub, y = g.hy0 + r;
            uint32_t v = 0;
            if constexpr (BAYER) v = bayer_gray4(raw[u], W, H, ax, exact_row(g, y), bk);
            else v = raw[u];
            store_h(Hs, g, L, in_exact(g, T, y) ? ((v >> sh) & L.bytemask) : 0u, kt < T.ka1 ? r : g.PR);
        }
    };
    if constexpr (BAYER) {
        for (int gi = 0; gi < T.ngroup; gi++) { // (one group's windows in flight: 27 registers per group)
            Raw ra[BOX_GROUP];
            load_rows(ra, gi);
            use_rows(ra, gi);
        }
    } else {
        Raw ra[BOX_GROUP], rb[BOX_GROUP];
        load_rows(ra, 0);
        for (int gi = 0; gi < T.ngroup; gi += 2) {
            load_rows(rb, gi + 1);
            use_rows(ra, gi);
            if (gi + 1 < T.ngroup) {
                load_rows(ra, gi + 2);
                use_rows(rb, gi + 1);
            }
        }
    }
}
// Sources 2 and 3, a remapped slot.  The table words of a group of trips (one 16-byte load per quad and trip):
__device__ __forceinline__ void load_table(uint4 (&tw)[BOX_GROUP], const uint32_t* __restrict__ map4, const BoxGeom& g, const BoxLane& L,
                                           const ExactTrips& T, int W, int gi)
{
#pragma unroll
    for (int u = 0; u < BOX_GROUP; u++) {
        const int yc = exact_row(g, g.hy0 + (T.ka0 + gi * BOX_GROUP + u) * L.rpw + L.rsub);
        __builtin_memcpy(&tw[u], map4 + ((uint32_t)yc * (uint32_t)W + (uint32_t)T.xc), 16);
    }
}
// The rectangle of source pixels the exact region reads: origin (sxa a multiple of 4, sya), SP bytes x SR rows; staged = it is
// in LDS (else it outgrew the buffer -- strong local distortion -- and the taps come from memory).
struct SrcRect { int sxa, sya, SP, SR; bool staged; };
// Reduces the per-lane partial of the rectangle (its loads were issued during the previous item), stages it -- coalesced dword
// loads, zeros outside the image (cv::remap's BORDER_CONSTANT); lane -> (row of the round, dword of the row); all rounds' loads in
// flight together -- and requests the first group's table words into `ta` beside the staging loads.  Three forms: the
// rectangle inside the image (the usual case: no clamps, no masks), leaving it, and BAYER.
template <bool BAYER>
__device__ __forceinline__ SrcRect stage_source(uint8_t* Sbuf, uint4 (&ta)[BOX_GROUP], const SrcBounds& sbp, int stage_bytes,
                                                const uint32_t* __restrict__ map4, const BoxGeom& g, const BoxLane& L, const ExactTrips& T,
                                                const uint8_t* __restrict__ img, int pitch, int W, int H, const BayerK& bk)
{
    const int lane = threadIdx.x, Hm1 = H - 1;
    int sxa = sbp.xa, sxb = sbp.xb, sya = sbp.ya, syb = sbp.yb;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        sxa = imin(sxa, __shfl_xor(sxa, d)); sxb = imax(sxb, __shfl_xor(sxb, d));
        sya = imin(sya, __shfl_xor(sya, d)); syb = imax(syb, __shfl_xor(syb, d));
    }
    sxa = uni(sxa) & ~3; sxb = uni(sxb); sya = uni(sya); syb = uni(syb);
    const int SP = (sxb - sxa + 4) & ~3, SR = syb - sya + 1, dpr = SP >> 2;
    const SrcRect R{sxa, sya, SP, SR, SP * SR <= stage_bytes && dpr <= 64};
    if (!R.staged) {
        load_table(ta, map4, g, L, T, W, 0);
        return R;
    }
    const float rcpd = __builtin_amdgcn_rcpf((float)dpr);
    const int rpi = small_div(64, rcpd), srs = small_div(lane, rcpd), sc = lane - srs * dpr;
    const bool s_on = srs < rpi;
    const int gx = sxa + 4 * sc, ax = gx < 0 ? 0 : (gx > W - 4 ? W - 4 : gx);
    const int sb = (gx - ax) * 8; // > 0 only at the right edge of the image
    uint32_t keep = 0;
#pragma unroll
    for (int k = 0; k < 4; k++)
        if ((unsigned)(gx + k) < (unsigned)W) keep |= 0xffu << (8 * k);
    if (sb >= 32 || sb < 0) keep = 0;
    const uint32_t shs = (uint32_t)(sb < 0 || sb > 31 ? 0 : sb);
    constexpr int SU = MOCAP_BOX_SU;
    const int nround = (SR + rpi - 1) / rpi;
    const bool interior = sya >= 0 && syb <= Hm1 && sxa >= 0 && sxa + SP <= W;
    if (!BAYER && interior) {
        const uint32_t step = (uint32_t)__mul24(rpi, pitch);
        const int scc = sc < dpr ? sc : dpr - 1; // (lanes past the last dword of a row re-read it)
        const uint32_t glast = (uint32_t)__mul24(syb, pitch) + (uint32_t)(sxa + 4 * scc); // same column, last row
        uint32_t goff = (uint32_t)__mul24(sya + (srs < SR ? srs : SR - 1), pitch) + (uint32_t)(sxa + 4 * scc);
        int li = __mul24(srs, dpr) + sc;
        const int lstep = __mul24(rpi, dpr), lend = s_on ? __mul24(SR, dpr) : 0;
        for (int r0 = 0; r0 < nround; r0 += 2 * SU) {
            uint32_t v[2 * SU];
#pragma unroll
            for (int u = 0; u < 2 * SU; u++) {
                // rows past the rectangle re-read its last row: always inside the image
                __builtin_memcpy(&v[u], img + goff, 4);
                goff = goff + step < glast ? goff + step : glast;
            }
            if (r0 == 0) load_table(ta, map4, g, L, T, W, 0);
#pragma unroll
            for (int u = 0; u < 2 * SU; u++) {
                if (li < lend) ((uint32_t*)Sbuf)[li] = v[u];
                li += lstep;
            }
        }
        return R;
    }
    // clamped rows, shifted and masked dwords.  BAYER: each lane's gray dword from the Bayer rows above, at and below it (every read
    // lies in the image); fewer rows in flight than the gray form, whose 14 loads are one dword each against nine here, and the
    // table words after the staging (their 12 registers would spill beside the windows)
    using Raw = std::conditional_t<BAYER, BayerWin, uint32_t>;
    constexpr int NV = BAYER ? 4 : 2 * SU;
    for (int r0 = 0; r0 < nround; r0 += NV) {
        Raw v[NV];
#pragma unroll
        for (int u = 0; u < NV; u++) {
            const int gy = sya + (r0 + u) * rpi + srs, gyc = gy < 0 ? 0 : (gy > Hm1 ? Hm1 : gy);
            if constexpr (BAYER) bayer_win_load(v[u], img, pitch, W, H, ax, gyc);
            else __builtin_memcpy(&v[u], img + ((uint32_t)gyc * (uint32_t)pitch + (uint32_t)ax), 4);
        }
        if (!BAYER && r0 == 0) load_table(ta, map4, g, L, T, W, 0);
#pragma unroll
        for (int u = 0; u < NV; u++) {
            const int r = (r0 + u) * rpi + srs, gy = sya + r, gyc = gy < 0 ? 0 : (gy > Hm1 ? Hm1 : gy);
            uint32_t raw = 0;
            if constexpr (BAYER) raw = bayer_gray4(v[u], W, H, ax, gyc, bk);
            else raw = v[u];
            const uint32_t val = ((unsigned)gy < (unsigned)H) ? ((raw >> shs) & keep) : 0u;
            if (s_on && r < SR) ((uint32_t*)Sbuf)[r * dpr + sc] = val;
        }
    }
    if (BAYER) load_table(ta, map4, g, L, T, W, 0);
    return R;
}
// One group of trips blended exactly as cv::remap's fixed point does, the taps from LDS (STAGED) or from memory.
template <bool STAGED>
__device__ __forceinline__ void blend_rows(uint2* Hs, const uint8_t* Sbuf, const SrcRect& R, const uint4 (&tw)[BOX_GROUP], int gi, const BoxGeom& g,
                                           const BoxLane& L, const ExactTrips& T, const uint8_t* __restrict__ img, int pitch, int W, int H)
{
    auto gray_px = [&](int x, int y) __attribute__((always_inline)) -> uint32_t { return img[(uint32_t)y * (uint32_t)pitch + (uint32_t)x]; };
#pragma unroll
    for (int u = 0; u < BOX_GROUP; u++) {
        const int kt = T.ka0 + gi * BOX_GROUP + u, r = kt * L.rpw + L.rsub, y = g.hy0 + r;
        const int yc = exact_row(g, y);
        // lanes outside the exact region blend a pixel of it (clamped row / quad) and drop the result: no branch,
        // so that the trips of a group overlap their LDS reads
        uint32_t okm = in_exact(g, T, y) ? L.bytemask : 0u;
        asm volatile("" : "+v"(okm));
        const uint32_t ww[4] = {tw[u].x, tw[u].y, tw[u].z, tw[u].w};
        int rowbase = __mul24(yc - R.sya, R.SP) + (T.xc - R.sxa); // LDS offset of (xc, yc)
        asm volatile("" : "+v"(rowbase)); // (keeps dy * SP a 24-bit multiply-add of its own)
        uint32_t B = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const Map4 m = map4_decode(ww[k]);
            uint32_t rr;
            if (STAGED) {
                const int A0 = __mul24(m.dy, R.SP) + (rowbase + k) + m.dx;
                rr = map4_blend(m, Sbuf[A0], Sbuf[A0 + 1], Sbuf[A0 + R.SP], Sbuf[A0 + R.SP + 1]);
            } else
                rr = map4_blend_from_memory(m, T.xc + k + m.dx, yc + m.dy, W, H, gray_px);
            B |= rr << (8 * k);
        }
        store_h(Hs, g, L, B & okm, kt < T.ka1 ? r : g.PR);
    }
}
// all groups: the table words of the next group are requested before the current one is blended (`ta` holds group 0's)
template <bool STAGED>
__device__ __forceinline__ void remap_rows(uint2* Hs, const uint8_t* Sbuf, const SrcRect& R, uint4 (&ta)[BOX_GROUP], const uint32_t* __restrict__ map4,
                                           const BoxGeom& g, const BoxLane& L, const ExactTrips& T, const uint8_t* __restrict__ img, int pitch, int W, int H)
{
    uint4 tb[BOX_GROUP];
    for (int gi = 0; gi < T.ngroup; gi += 2) {
        load_table(tb, map4, g, L, T, W, gi + 1);
        blend_rows<STAGED>(Hs, Sbuf, R, ta, gi, g, L, T, img, pitch, W, H);
        if (gi + 1 < T.ngroup) {
            load_table(ta, map4, g, L, T, W, gi + 2);
            blend_rows<STAGED>(Hs, Sbuf, R, tb, gi + 1, g, L, T, img, pitch, W, H);
        }
    }
}
// BAYER, taps from memory, each tap's gray from its 3x3 Bayer neighbourhood: rare (strong local distortion), only correct.
// One trip at a time and one tap's nine loads in flight: the unrolled groups above would spill here.
__device__ __forceinline__ void bayer_rows_from_memory(uint2* Hs, const uint32_t* __restrict__ map4, const BoxGeom& g, const BoxLane& L,
                                                       const ExactTrips& T, const uint8_t* __restrict__ img, int pitch, int W, int H, const BayerK& bk)
{
    auto bayer_px = [&](int x, int y) __attribute__((always_inline)) -> uint32_t {
        uint32_t t = bayer_gray1(img, pitch, W, H, x, y, bk); asm volatile("" : "+v"(t) : : "memory");
        return t;
    };
    for (int kt = T.ka0; kt < T.ka1; kt++) {
        const int r = kt * L.rpw + L.rsub, y = g.hy0 + r, yc = exact_row(g, y);
        const uint32_t okm = in_exact(g, T, y) ? L.bytemask : 0u;
        uint4 tw;
        __builtin_memcpy(&tw, map4 + ((uint32_t)yc * (uint32_t)W + (uint32_t)T.xc), 16);
        const uint32_t ww[4] = {tw.x, tw.y, tw.z, tw.w};
        uint32_t B = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const Map4 m = map4_decode(ww[k]);
            B |= map4_blend_from_memory(m, T.xc + k + m.dx, yc + m.dy, W, H, bayer_px) << (8 * k);
        }
        store_h(Hs, g, L, B & okm, r);
    }
}

// ---- pass B: vertical 5-sums -> threshold -> horizontal window counts of the threshold bits --------------------------------
// EDGE: the patch sticks out of the image on the left or right
template <bool EDGE>
__device__ __forceinline__ void threshold_rows(const uint2* Hs, uint32_t* Cs, const uint32_t* lut, const BoxGeom& g, const BoxLane& L, int W, int H, int thr_mul)
{
    const int lane = threadIdx.x, q = L.q, Q = g.Q;
    const int c0t = taps5(L.x, W), c1t = taps5(L.x + 1, W), c2t = taps5(L.x + 2, W), c3t = taps5(L.x + 3, W);
    const uint32_t cx01 = (uint32_t)(c0t & 0xffff) | ((uint32_t)c1t << 16), cx23 = (uint32_t)(c2t & 0xffff) | ((uint32_t)c3t << 16);
    const bool left_edge = g.px0 < 0, right_edge = g.px0 + 4 * Q > W;
    const int qe = (W - 1 - g.px0) >> 2, be = (W - 1 - g.px0) & 3; // quad / bit of column W - 1
    const int ntrip = (g.ty1 - g.ty0 + 1 + L.rpw - 1) / L.rpw;
    const int hstep = Q;                                           // Hs entries per patch row
#pragma unroll 2
    for (int k = 0; k < ntrip; k++) {
        const int y = g.ty0 + k * L.rpw + L.rsub, yb = imin(y, g.ty1), rh = yb - g.hy0; // H row of the threshold row (>= 2)
        const uint2* hp = Hs + (__mul24(rh - 2, hstep) + q);
        const uint2 v0 = hp[0], v1 = hp[hstep], v2 = hp[2 * hstep], v3 = hp[3 * hstep], v4 = hp[4 * hstep];
        const uint32_t V01 = v0.x + v1.x + v2.x + v3.x + v4.x, V23 = v0.y + v1.y + v2.y + v3.y + v4.y;
        const uint32_t m = (uint32_t)__mul24(thr_mul, taps5(yb, H));
        const uint32_t T01 = __umul24(cx01, m), T23 = __umul24(cx23, m);
        const uint32_t d01 = (V01 | 0x80008000u) - T01, d23 = (V23 | 0x80008000u) - T23;
        const uint32_t t = (d01 >> 15) & 0x10001u, u = (d23 >> 15) & 0x10001u;
        const uint32_t wv = t | (u << 2);
        uint32_t nib = (wv | (wv >> 15)) & 0xfu;
        if (EDGE) {
            // medianBlur replicates the border: columns outside the image take the edge column's bit
            if (left_edge) { // quad 0 = columns -4..-1, quad 1 starts at column 0
                const uint32_t e = lane_from_next(nib) & 1u;
                if (q == 0) nib = e ? 0xfu : 0u;
            }
            if (right_edge) {
                const uint32_t ne = (uint32_t)__shfl((int)nib, lane - q + qe);
                const uint32_t e = (ne >> be) & 1u, keep = (2u << be) - 1u;
                if (q > qe) nib = e ? 0xfu : 0u;
                else if (q == qe) nib = (nib & keep) | (e ? (0xfu & ~keep) : 0u);
            }
        }
        const uint32_t nl = lane_from_prev(nib), nr = lane_from_next(nib);
        const uint32_t win = (nl >> 2) | (nib << 2) | ((nr & 3u) << 6);
        Cs[lane_slot(g, L, y - g.ty0, g.ty1 - g.ty0 + 1)] = lut[win & 0xffu];
    }
}

// ---- pass C: majority (>= 13 of 25) of every output row, two quads -> one byte of the bit mask -----------------------------
// The item's output region lies in at most 2 x 2 tiles: chunks chunk0 (+1), strips strip0 (+1).  Per lane, bit g of lo / hi:
// rows 8g..8g+7 of chunk0 / chunk0 + 1 hold set pixels in this lane's columns.
struct RowGroups { uint32_t lo, hi; };
__device__ __forceinline__ int box_out_byte(const BoxGeom& g, const BoxLane& L) { return (g.ox0 >> 3) + ((L.q - 1) >> 1); }
// INNER: no row of the item's windows is replicated (rows 0 and H - 1 are further than 2 rows away)
template <bool INNER>
__device__ __forceinline__ RowGroups majority_rows(const uint32_t* Cs, uint8_t* __restrict__ mrow, const BoxGeom& g, const BoxLane& L, int W, int H,
                                                   int words_per_row, int tile_r0, int tile_r1)
{
    const int q = L.q, Q = g.Q, Hm1 = H - 1, hstep = Q;
    const int out_byte = box_out_byte(g, L);
    const bool stores = L.lane_on && (q & 1) && q <= Q - 3 && out_byte < ((W + 7) >> 3) && out_byte < words_per_row * 4;
    RowGroups acc{0u, 0u};
    const int ntrip = (g.oy1 - g.oy0 + 1 + L.rpw - 1) / L.rpw;
#pragma unroll 2
    for (int k = 0; k < ntrip; k++) {
        const int y = g.oy0 + k * L.rpw + L.rsub, yy = imin(y, g.oy1);
        uint32_t Cv = 0;
        if (INNER) {
            const uint32_t* cp = Cs + (__mul24(yy - 2 - g.ty0, hstep) + q);
            Cv = cp[0] + cp[hstep] + cp[2 * hstep] + cp[3 * hstep] + cp[4 * hstep];
        } else {
#pragma unroll
            for (int d = -2; d <= 2; d++) {
                const int yr = yy + d < 0 ? 0 : (yy + d > Hm1 ? Hm1 : yy + d); // BORDER_REPLICATE in y
                Cv += Cs[__mul24(yr - g.ty0, Q) + q];
            }
        }
        const uint32_t mm = ((Cv + 0x73737373u) >> 7) & 0x01010101u;
        const uint32_t t1 = mm | (mm >> 7);
        const uint32_t mn = (t1 | (t1 >> 14)) & L.colmask & 0xfu;
        const uint32_t odd = lane_from_next(mn);
        const uint32_t byte = mn | ((odd & 0xfu) << 4);
        const bool st = stores && y <= g.oy1;
        if (st) mrow[mask_byte_index(y, out_byte, words_per_row)] = (uint8_t)byte;
        const uint32_t hit = (st && byte != 0u) ? 1u : 0u;
        if (yy < tile_r1) acc.lo |= hit << ((yy - tile_r0) >> 3);
        else acc.hi |= hit << ((yy - tile_r1) >> 3);
    }
    return acc;
}
// occupancy words of the item's tiles (read by the contour kernel): OR of every lane's row groups; bit 31 = filtered
__device__ __forceinline__ void mark_occupancy(uint32_t* __restrict__ cells, const BoxGeom& g, const BoxLane& L, RowGroups acc, int chunk0,
                                               int rows_per_chunk, int n_chunks, int n_strips)
{
    const int strip0 = g.ox0 / 240;
    const int lstrip = (box_out_byte(g, L) >= 30 * (strip0 + 1)) ? 1 : 0; // this lane's bytes lie in strip0 or strip0 + 1
    const int chunk1 = g.oy1 / rows_per_chunk, strip1 = (g.ox1 >> 3) / 30;
    for (int cc = 0; cc <= chunk1 - chunk0; cc++)
        for (int ss = 0; ss <= strip1 - strip0; ss++) {
            const uint32_t la = cc ? acc.hi : acc.lo;
            uint32_t cellmask = 0;
            for (int gg = 0; gg < 9; gg++)
                if (__ballot(lstrip == ss && ((la >> gg) & 1u)) != 0ull) cellmask |= 1u << gg;
            const size_t cidx = ((size_t)g.image * n_chunks + chunk0 + cc) * n_strips + strip0 + ss;
            if (threadIdx.x == 0) atomicOr(&cells[cidx], cellmask | 0x80000000u);
        }
}

} // namespace

// ---- the kernel ----------------------------------------------------------------------------------------------------------------
// Registers.  The kernel's 20 KB of LDS per wave allow two waves per SIMD, and left to itself the compiler takes every register
// two waves can have (242; 214 when told to aim at two).  What it does with them is keep loads in flight -- six trips' table words
// twice over, 28 staging dwords -- and a wave that size shuts the other batches' kernels out of its SIMD.
// Round 4: groups of 3 trips and 14 staging loads, compiled for four waves per SIMD: 128 registers, no spills, the same duration
// alone (0.49 ms for the benchmark batch's filters) and +3..7 % for the three-batch pipeline (profiles/history/r4_*.log).
// The phases above are __forceinline__ functions over BoxGeom, BoxLane, ExactTrips and plain scalars: the kernel compiles to the
// registers it had as one body (profiles/README.md, round 18).
constexpr size_t BOX_LDS_BYTES = 1024 + (size_t)(BOX_HCAP + 64) * 8 + BOX_SCAP;
// A driver: take an item, prefetch the next one, pass A -> B -> C.  Global memory latency is taken out of the item loop: the next
// item's header and the box of source pixels it will read are fetched while the current item is filtered, all staging loads of
// an item are in flight together, and the table words of the next group of trips are requested before the current group is blended.
// BAYER = true: a.src holds raw Bayer frames (gray-less input); the three sources of pass A -- identity rows, staged rectangle,
// taps from memory -- form the gray values they read with bayer_gray4 / bayer_gray1, everything after them is the same.
template <bool BAYER>
__global__ __attribute__((amdgpu_waves_per_eu(MOCAP_BOX_WAVES, MOCAP_BOX_WAVES))) __launch_bounds__(64) void box_filter_kernel(BoxArgs a)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t box_lds[];
    uint32_t* const lut = (uint32_t*)box_lds;
    uint2* const Hs = (uint2*)(box_lds + 1024);                         // + 64: where lanes without a row park their store
    uint8_t* const Sbuf = box_lds + 1024 + (size_t)(BOX_HCAP + 64) * 8; // staged source pixels; afterwards the window counts
    uint32_t* const Cs = (uint32_t*)Sbuf;
    static_assert((BOX_HCAP + 64) * 4 <= BOX_SCAP, "counts alias the source buffer");

    const int lane = threadIdx.x;
    const int H = a.H, W = a.W, cam_mod = a.cam_mod;
    const uint64_t remap_bits = a.remap_bits;
    const ushort4* __restrict__ srcbox = a.srcbox;
    const BoxItem* __restrict__ items = a.items;
    uint64_t* const a_timing = a.timing;
    const BayerK bk{a.bayer.ry, a.bayer.rx, a.bayer.cb, a.bayer.cg, a.bayer.cr, a.bayer.shift};
    if (a.prio) __builtin_amdgcn_s_setprio(2); // A/B switch: these waves compute, the scan's waves of the next batch wait on HBM
    fill_window_counts(lut, lane);
    const uint32_t n_listed = *a.n_items;
    ItemQueue queue{a.n_items + 16, n_listed < a.cap_items ? n_listed : a.cap_items, (int)(blockIdx.x & 7), 0};
    uint32_t item = queue.take();
    if (item == NO_ITEM) return;
    uint32_t nitem = queue.take();

    uint64_t tacc[6] = {0, 0, 0, 0, 0, 0}, tlast = a.timing ? __builtin_readcyclecounter() : 0; // phase clock (debugging aid)
    auto tick = [&](int i) __attribute__((always_inline)) { if (a_timing) { const uint64_t now = __builtin_readcyclecounter(); tacc[i] += now - tlast; tlast = now; } };
    BoxGeom g = box_geometry(H, W, cam_mod, remap_bits, items[item]);
    SrcBounds sbp = source_bounds_partial(srcbox, H, W, g, lane);

    while (item != NO_ITEM) {
        // the next item's header and the index of the one after it: requested now, looked at when this item's patch is done /
        // at the end of the iteration
        const BoxItem nit = items[nitem != NO_ITEM ? nitem : item];
        const uint32_t nn_raw = queue.request();
        if (!g.valid) {
            // An empty part of a split.  choose_split (blob_settle.hip) cuts no region into parts of which one is empty at the default
            // BOX_HCAP / BOX_MAX_PARTS (enumerated for every width and height a tile or a cluster can have), so no test reaches this;
            // the build-time knobs can change those constants, hence the skip stays.
            g = box_geometry(H, W, cam_mod, remap_bits, nit);
            sbp = source_bounds_partial(srcbox, H, W, g, lane);
            item = nitem;
            nitem = queue.resolve(nn_raw);
            continue;
        }
        const BoxLane L = box_lane(g, W);
        const ExactTrips T = exact_trips(g, L);
        const uint8_t* __restrict__ img = a.src + (size_t)g.image * a.image_stride;
        __syncthreads(); // (single wave) the previous item's LDS reads are done
        tick(0);

        // ---- pass A -----------------------------------------------------------------------------------------------------------
        zero_rows_outside(Hs, g, L, T);
        if (!g.exact) {
        } else if (!g.remap) {
            identity_rows<BAYER>(Hs, g, L, T, img, a.pitch, W, H, bk);
        } else {
            const uint32_t* __restrict__ map4 = a.map4 + (size_t)g.slot * H * W;
            uint4 ta[BOX_GROUP];
            const SrcRect R = stage_source<BAYER>(Sbuf, ta, sbp, a.stage_bytes, map4, g, L, T, img, a.pitch, W, H, bk);
            if (R.staged) {
                __syncthreads();
                tick(1);
                remap_rows<true>(Hs, Sbuf, R, ta, map4, g, L, T, img, a.pitch, W, H);
            } else if constexpr (!BAYER) remap_rows<false>(Hs, Sbuf, R, ta, map4, g, L, T, img, a.pitch, W, H);
            else bayer_rows_from_memory(Hs, map4, g, L, T, img, a.pitch, W, H, bk);
        }
        __syncthreads();
        tick(2);
        // the next item: its geometry, and the loads of its source box (in flight during passes B and C)
        const BoxGeom gn = box_geometry(H, W, cam_mod, remap_bits, nit);
        const SrcBounds sbn = source_bounds_partial(srcbox, H, W, gn, lane);

        // ---- pass B -----------------------------------------------------------------------------------------------------------
        if (g.px0 < 0 || g.px0 + 4 * g.Q > W) threshold_rows<true>(Hs, Cs, lut, g, L, W, H, a.thr_mul);
        else threshold_rows<false>(Hs, Cs, lut, g, L, W, H, a.thr_mul);
        __syncthreads();
        tick(3);

        // ---- pass C -----------------------------------------------------------------------------------------------------------
        const int chunk0 = g.oy0 / a.rows_per_chunk;
        const int tile_r0 = chunk0 * a.rows_per_chunk, tile_r1 = tile_r0 + a.rows_per_chunk; // first row of chunk0 / of chunk0 + 1
        uint8_t* __restrict__ mrow = (uint8_t*)(a.mask + (size_t)g.image * mask_image_words(H, a.words_per_row));
        const RowGroups acc = (g.oy0 >= 2 && g.oy1 + 2 <= H - 1) ? majority_rows<true>(Cs, mrow, g, L, W, H, a.words_per_row, tile_r0, tile_r1)
                                                                 : majority_rows<false>(Cs, mrow, g, L, W, H, a.words_per_row, tile_r0, tile_r1);
        mark_occupancy(a.cells, g, L, acc, chunk0, a.rows_per_chunk, a.n_chunks, a.n_strips);
        g = gn; sbp = sbn; item = nitem;
        nitem = queue.resolve(nn_raw);
        tick(4);
        tacc[5] += 1;
    }
    if (a_timing && lane == 0)
        for (int i = 0; i < 6; i++) a_timing[(size_t)blockIdx.x * 6 + i] = tacc[i];
}

// resident workgroups of the box kernel per CU (the list is dealt to a grid of exactly the resident workgroups)
int box_filter_blocks_per_cu()
{
    int n = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, box_filter_kernel<false>, 64, BOX_LDS_BYTES) != hipSuccess || n < 1) n = 8;
    return n;
}

void launch_box_filter(const BoxArgs& a, int grid, hipStream_t s, bool bayer)
{
    if (bayer) hipLaunchKernelGGL(box_filter_kernel<true>, dim3(grid), dim3(64), BOX_LDS_BYTES, s, a);
    else hipLaunchKernelGGL(box_filter_kernel<false>, dim3(grid), dim3(64), BOX_LDS_BYTES, s, a);
}

} // namespace mocap
