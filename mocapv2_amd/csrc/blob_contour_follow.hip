// blob_contour_follow.hip -- the border walks of a whole batch (contours_dev.h: the algorithm; blob_contour_image.hip: launch_contours).
#include "contours_dev.h"

namespace mocap {

// The walks of the whole batch, whatever image they belong to, TWO LANES PER BORDER: lane 2i follows the border forwards from
// its start, lane 2i + 1 backwards from the same start (border following is reversible: the backward walk is the forward rule
// on the vertically mirrored neighbourhood), and the pair stops where the two meet -- half the steps of the longest border, which
// is what the kernel's duration comes down to (a merged pair of markers has a border of ~900 steps, ~0.5 us each).  Each lane
// accounts for the forward steps it covers (Green sums, vertices, runs, raster minima, box); the sums add, the two runs that
// straddle the seams (at the start pixel and at the meeting point) are joined before their float32 lengths are taken, exactly
// as the reference measures the whole polygon.
// The waves are PERSISTENT and refill their lane pairs: every FOLLOW_K steps a wave looks at its lanes; pairs whose walk has
// ended store their record (one round of atomics and stores for all of them), walks that have reached the rim of their mask
// window pause until it is staged anew around them, and when enough pairs are idle the wave takes that many new entries from
// the batch-wide list (one atomic on its head).  The windows (64 rows x 64 columns, in LDS, row-major over the lanes:
// bank-conflict-free for lanes at different rows) are staged by the whole wave, lane = row, eight windows per round; a pair
// shares one window until one of its lanes leaves it.  No global memory access happens inside the step loop.
// The step is `follow` (blob_contour_image.hip) cut into resumable, direction-symmetric steps: same neighbour search, same vertex rule, same sums.
#ifndef FOLLOW_K_STEPS
#define FOLLOW_K_STEPS 16
#endif
constexpr int FOLLOW_K = FOLLOW_K_STEPS; // steps between two looks at the lanes
constexpr int FOLLOW_REFILL = 8;  // idle pairs that make a refill worth its three dependent memory round trips
#ifndef STAGE_N
#define STAGE_N 8                 // windows staged per round (3 loads each in flight together)
#endif

__device__ __forceinline__ int pair_swap(int v) { return __builtin_amdgcn_mov_dpp(v, 0xB1 /*quad_perm:[1,0,3,2]*/, 0xf, 0xf, true); }
__device__ __forceinline__ int64_t pair_swap64(int64_t v)
{
    const uint32_t lo = (uint32_t)pair_swap((int)(uint32_t)v), hi = (uint32_t)pair_swap((int)(uint32_t)((uint64_t)v >> 32));
    return (int64_t)(((uint64_t)hi << 32) | lo);
}
__device__ __forceinline__ double pair_swap_f64(double v) { return __longlong_as_double(pair_swap64(__double_as_longlong(v))); }

// A lane is idle, or holds half a walk that is running (`active`), or paused (its pixel lies on the rim of its window: it waits for
// the next look at the lanes), or `finished` (the pair has met, or given up; the record is not stored yet).  These three flags, and
// the wave's `drained` and `first_fill`, are plain locals of the kernel handed to the phases by reference: they decide control flow.
struct Walk { // one lane's half of a walk
    int r, r_ahead;      // raster key y * (W + 1) + x of the current pixel; backward lane: of the pixel ahead of it (the one it came from)
    int64_t a00, a10, a01;
    double diag, pend;
    int sx, sy, x, y, known; // start pixel of the border; current pixel; the direction this lane knows there: the way back
                             //   (forward lane) / the way forward (backward lane)
    int run, head, axis, npts, steps, min_fg, min_ebg, bx0, bx1, by0, by1;
    int wx0, wy0, wslot; // the lane's window: columns wx0 .. wx0 + 63, rows wy0 .. wy0 + 63 of its image's mask, in LDS column wslot
    int abort_lt, key, s0;
    uint32_t n, meta;    // n: neighbourhood (mirrored for the backward lane); meta: kind | border << 2 | image << 11
    bool abort_on_fg, has_head;
    int status;          // 0 closed, 1 aborted, 2 step limit

    // The three rows around the pixel and its left / right neighbour columns must lie inside the window: a lane on the rim pauses.
    __device__ __forceinline__ bool on_rim() const { return (unsigned)(x - wx0 - 1) > 61u || (unsigned)(y - wy0 - 1) > 61u; }
};

// what a lane's steps read beside its Walk
struct FollowCtx {
    const uint8_t* win_bytes; // the windows, [row of the window][window] of 64-bit rows
    const double* diag_len;   // run_length(1, k) for k < 64
    int RS;                   // raster stride W + 1
    bool isB;                 // the backward lane of its pair
    int up_dy;                // the row that plays "up": the backward lane walks the vertically mirrored image

    // what a step in direction d adds to the raster key
    __device__ __forceinline__ int dir_off(int d) const { return __mul24(dir_dy(d), RS) + dir_dx(d); }

    // occupancy of the 8 neighbours of (x,y), bit s = direction code s (0=E 1=NE 2=N 3=NW 4=W 5=SW 6=S 7=SE) -- with up = 1 of the
    // vertically mirrored image (rows swapped: NE <-> SE, N <-> S, NW <-> SW).  Straight from the lane's window: the three columns
    // x-1 .. x+1 of a row lie in the 16 bits at byte (x - 1 - wx0) >> 3 of the window row (one ds_read_u16 each; the pixel is inside
    // the rim, see the pause rule -- a paused lane reads some bytes of the array and does not use them).
    __device__ __forceinline__ uint32_t nbr8(const Walk& w, int x, int y, int up) const
    {
        const int c = x - w.wx0 - 1; // column x-1 at bit 0
        const uint32_t col = (uint32_t)w.wslot * 8u + (((uint32_t)c >> 3) & 7u), sh = (uint32_t)c & 7u;
        const int ly = y - w.wy0;
        uint16_t vu, vm, vd;
        __builtin_memcpy(&vu, win_bytes + ((((uint32_t)(ly + up) & 63u) << 9) + col), 2);
        __builtin_memcpy(&vm, win_bytes + ((((uint32_t)ly & 63u) << 9) + col), 2);
        __builtin_memcpy(&vd, win_bytes + ((((uint32_t)(ly - up) & 63u) << 9) + col), 2);
        return nbr_code(((uint32_t)vu >> sh) & 7u, ((uint32_t)vm >> sh) & 7u, ((uint32_t)vd >> sh) & 7u);
    }

    // one CHAIN_APPROX_SIMPLE segment of `len` steps: its cv.arcLength term
    __device__ __forceinline__ void close_run(Walk& w, int len, int parity) const
    {
        if (parity) w.diag += len < 64 ? diag_len[len] : run_length(1, len);
        else w.axis += len;
    }
};

// optional phase clock (follow_timing = 1, a debugging aid): per wave, 100 MHz ticks in store / refill / walk, wave steps, lane
// steps, walks, refills
struct PhaseClock {
    bool on;
    uint64_t t_prev;
    uint64_t tk[8];
    __device__ __forceinline__ void lap(int i)
    {
        if (on) { const uint64_t t = wall_clock64(); tk[i] += t - t_prev; t_prev = t; }
    }
};

// what the forward lane gathers of the backward lane's half
struct PartnerHalf {
    int64_t a00, a10, a01;
    double diag;
    int axis, npts, steps, run, head, has_head, min_fg, min_ebg, bx0, bx1, by0, by1, status;
};

// (both lanes of a pair are finished together; the exchange runs for the whole wave, idle lanes carry zeros)
__device__ __forceinline__ PartnerHalf exchange_halves(const Walk& w)
{
    PartnerHalf o;
    o.a00 = pair_swap64(w.a00); o.a10 = pair_swap64(w.a10); o.a01 = pair_swap64(w.a01);
    o.diag = pair_swap_f64(w.diag + w.pend);
    o.axis = pair_swap(w.axis); o.npts = pair_swap(w.npts); o.steps = pair_swap(w.steps); o.run = pair_swap(w.run);
    o.head = pair_swap(w.head); o.has_head = pair_swap(w.has_head ? 1 : 0);
    o.min_fg = pair_swap(w.min_fg); o.min_ebg = pair_swap(w.min_ebg);
    o.bx0 = pair_swap(w.bx0); o.bx1 = pair_swap(w.bx1); o.by0 = pair_swap(w.by0); o.by1 = pair_swap(w.by1);
    o.status = pair_swap(w.status);
    return o;
}

// join the halves: sums add; the run through the start pixel = the two heads (or, when a half has no vertex at all, that half's
// whole run as well), the run through the meeting point = the two tails
__device__ __forceinline__ void join_halves(const FollowCtx& cx, Walk& w, const PartnerHalf& o)
{
    w.a00 += o.a00; w.a10 += o.a10; w.a01 += o.a01;
    w.diag += w.pend; w.pend = 0.0; w.diag += o.diag; w.axis += o.axis;
    w.npts += o.npts; w.steps += o.steps;
    w.min_fg = o.min_fg < w.min_fg ? o.min_fg : w.min_fg; w.min_ebg = o.min_ebg < w.min_ebg ? o.min_ebg : w.min_ebg;
    w.bx0 = o.bx0 < w.bx0 ? o.bx0 : w.bx0; w.bx1 = o.bx1 > w.bx1 ? o.bx1 : w.bx1;
    w.by0 = o.by0 < w.by0 ? o.by0 : w.by0; w.by1 = o.by1 > w.by1 ? o.by1 : w.by1;
    const int par0 = w.s0 & 1, par_tail = w.known & 1; // direction parity of the run through the start / of the forward tail
    if (w.has_head && o.has_head) {
        cx.close_run(w, w.head + o.head, par0);
        cx.close_run(w, w.run + o.run, par_tail);
    } else
        cx.close_run(w, (w.has_head ? w.head : 0) + (o.has_head ? o.head : 0) + w.run + o.run, par0);
}

// the pairs whose walk has ended: the forward lane gathers the backward lane's half and stores the record
__device__ __forceinline__ void exchange_and_store_finished(const ContourArgs& a, const FollowCtx& cx, ContourWork* works, Walk& w, bool& finished)
{
    if (!__ballot(finished)) return;
    const PartnerHalf o = exchange_halves(w);
    if (finished && !cx.isB) {
        const int kind = (int)(w.meta & 3u), image = (int)(w.meta >> 11), border = (int)((w.meta >> 2) & 511u);
        ContourWork& work = works[image];
        const bool single = w.npts == 1 && w.steps == 0 && o.steps == 0 && w.status == 0 && w.s0 < 0; // an isolated pixel
        const int status = w.status > o.status ? w.status : o.status;
        if (!single && status == 0) join_halves(cx, w, o);
        if (status == 2) atomicMax(&work.st_err, 1);
        if (kind >= 2) { // a link walk: which border is this?
            if (status == 0) {
                int lkey, ltype;
                link_identity(w.a00, w.min_fg, w.min_ebg, lkey, ltype);
                work.link_key[border] = lkey;
                work.link_type[border] = (uint8_t)ltype;
            } else atomicMax(&work.st_err, 1);
        } else if (status == 0) {
            const int slot = atomicAdd(&work.st_nrec, 1);
            if (slot < MAXR) {
                ContourRec r;
                make_record(r, w.key, kind, w.sx, w.sy, w.npts, w.steps, w.a00, w.a10, w.a01, (double)w.axis + w.diag, a.min_area, a.min_circ);
                work.recs[slot] = r;
                store_small_fields(slot, r, w.bx0, w.by0, w.bx1, w.by1, work.rkey, work.rsx, work.rsy, work.rhole, work.rkept, work.rbox);
            }
        }
    }
    finished = false;
}

// the batch-wide list the wave's entries come from
struct WalkList {
    const uint64_t* list;
    uint32_t total;
    uint32_t* head_ctr;
};

// Refill: when enough pairs are idle (or none is busy) the wave takes that many entries; the k-th idle pair gets the k-th of them.
// The first 32 entries of a wave are those at 32 * its number (no atomic, no round trip); the counter hands out the rest.
// -> this lane's pair took an entry: its start, window and meta are set (both lanes), `kind` and `ex` (the entry's scan column) too
__device__ __forceinline__ bool take_entries(const WalkList& wl, int lane, uint64_t busy, uint64_t busy_pairs, Walk& w, bool& drained, bool& first_fill,
                                             PhaseClock& clock, int& kind, int& ex)
{
    const int n_idle = 32 - __popcll(busy_pairs);
    bool take = false;
    if (!drained && (n_idle >= FOLLOW_REFILL || busy == 0)) {
        uint32_t base = blockIdx.x * 32u;
        if (!first_fill) {
            if (lane == 0) base = atomicAdd(wl.head_ctr, (uint32_t)n_idle);
            base = (uint32_t)uni((int)base) + gridDim.x * 32u;
        }
        first_fill = false;
        const int n_new = base < wl.total ? (int)(wl.total - base < (uint32_t)n_idle ? wl.total - base : (uint32_t)n_idle) : 0;
        drained = n_new < n_idle;
        if (clock.on) { clock.tk[5] += (uint64_t)n_new; clock.tk[6]++; }
        const uint64_t idle_pairs = ~busy_pairs & 0x5555555555555555ull;
        const int rank = __popcll(idle_pairs & ((1ull << (lane & ~1)) - 1ull)); // this pair's number among the idle ones
        take = ((idle_pairs >> (lane & ~1)) & 1ull) != 0 && rank < n_new;
        uint64_t e = 0;
        if (take) e = wl.list[base + (uint32_t)rank];
        ex = (int)(e & 0x7fffu); kind = (int)((e >> 30) & 3u);
        if (take) {
            const int ey = (int)((e >> 15) & 0x7fffu);
            const int sx = ex - (kind == 1 ? 1 : 0); // a hole candidate's border pixel lies left of its scan position
            w.meta = (uint32_t)kind | ((uint32_t)((e >> 52) & 511u) << 2) | ((uint32_t)((e >> 32) & 0xfffffu) << 11);
            w.sx = sx; w.sy = ey; w.x = sx; w.y = ey;
            // an outer border starts at its topmost row: its window reaches down from there; a hole border has pixels one row
            // higher; a link walk starts anywhere on its border
            w.wx0 = sx - 31; w.wy0 = kind == 0 ? ey - 1 : (kind == 1 ? ey - 2 : ey - 31);
            w.wslot = lane & ~1; // the pair shares the forward lane's window until one of the two leaves it
        }
    }
    return take;
}

// a paused lane's window: anew around its current pixel, in the one of the pair's two windows that the partner does not use (both
// paused: each takes its own)
__device__ __forceinline__ void place_windows(Walk& w, int lane, bool paused)
{
    if (paused) { w.wx0 = w.x - 31; w.wy0 = w.y - 31; }
    const int partner_slot = pair_swap(w.wslot), partner_paused = pair_swap(paused ? 1 : 0);
    if (paused) w.wslot = partner_paused ? lane : (partner_slot == (lane & ~1) ? (lane | 1) : (lane & ~1));
}

// the windows of the lanes in `stage`, by the whole wave: lane = row of the window, STAGE_N windows per round so that their loads
// are in flight together.  Ends with the barrier behind which the lanes read their own.
__device__ __forceinline__ void stage_windows(const ContourArgs& a, uint64_t (*win)[64], const Walk& w, uint64_t stage, int lane, uint32_t image_words, int RS)
{
    const int image = (int)(w.meta >> 11);
    for (uint64_t todo = stage; todo;) {
        int cs[STAGE_N];
        uint64_t rows[STAGE_N];
#pragma unroll
        for (int j = 0; j < STAGE_N; j++) {
            cs[j] = todo ? __ffsll((long long)todo) - 1 : -1;
            todo &= todo - 1; // (0 & anything = 0)
        }
#pragma unroll
        for (int j = 0; j < STAGE_N; j++) {
            const int c = cs[j] < 0 ? cs[0] : cs[j]; // a short last round repeats its first window (not stored)
            const int img_c = __builtin_amdgcn_readlane(image, c), x0_c = __builtin_amdgcn_readlane(w.wx0, c), y0_c = __builtin_amdgcn_readlane(w.wy0, c);
            const Mask Mc{a.mask + (size_t)img_c * image_words, a.words_per_row, a.H, a.W, RS};
            rows[j] = row64(Mc, y0_c + lane, x0_c);
        }
#pragma unroll
        for (int j = 0; j < STAGE_N; j++)
            if (cs[j] >= 0) win[lane][__builtin_amdgcn_readlane(w.wslot, cs[j])] = rows[j];
    }
    __syncthreads(); // (one wave) the windows are in LDS before any lane reads its own
}

// both lanes of a pair that took an entry: the start's first neighbour, clockwise from the one known to be background
__device__ __forceinline__ void start_walk(const FollowCtx& cx, Walk& w, int kind, int ex, bool& active, bool& paused, bool& finished)
{
    const uint32_t n0 = cx.nbr8(w, w.x, w.y, -1);
    const int sx = w.sx, ey = w.sy;
    w.key = ey * cx.RS + ex;
    const int first = (kind == 0 || kind == 2) ? 4 : 0; // W (outer start) / E
    w.abort_on_fg = kind == 0;
    w.abort_lt = kind <= 1 ? w.key : -1;  // link walks run all the way round
    w.a00 = w.a10 = w.a01 = 0; w.npts = 0; w.steps = 0; w.axis = 0; w.diag = 0.0; w.pend = 0.0;
    w.run = 0; w.head = 0; w.has_head = false;
    w.min_fg = 0x7fffffff; w.min_ebg = 0x7fffffff;
    w.bx0 = 0x7fffffff; w.bx1 = -1; w.by0 = 0x7fffffff; w.by1 = -1;
    const int s = first_neighbour(n0, first);
    w.status = 0;
    if (s == first) { // isolated pixel: one vertex, zero area, zero perimeter
        w.s0 = -1;
        if (!cx.isB) { w.npts = 1; w.min_fg = ey * cx.RS + sx; w.min_ebg = ey * cx.RS + sx + 1; w.bx0 = w.bx1 = sx; w.by0 = w.by1 = ey; }
        finished = true;
    } else {
        w.s0 = s;
        w.r = ey * cx.RS + sx; w.r_ahead = w.r;
        if (cx.isB) { w.x = sx + dir_dx(s); w.y = ey + dir_dy(s); w.r += cx.dir_off(s); w.known = s ^ 4; } // one step back along the border: the way forward from there
        else w.known = s;
        active = true;
        paused = w.on_rim();
    }
}

// The step, tentatively, and where it leaves the pair.
struct Tentative {
    int srch;        // the direction of the next border pixel
    int r_next;      // its raster key
    bool ends;       // the pair's walk ends here without this step: the lanes have met, or the partner gave up, or (backward lane) the
                     //   forward lane's step of this round completes the cycle
    bool fwd_closes; // the forward lane's step of this round completes the cycle
};

// Search the next border pixel (counter-clockwise from known + 1; the backward lane does the same on its mirrored neighbourhood,
// i.e. clockwise from known - 1), and compare where the two lanes stand on the border's cycle of (pixel, way back) states: the
// forward lane at its own state, the backward lane just behind the state (pixel ahead of it, way back to it) -- pixels as raster keys.
__device__ __forceinline__ Tentative where_the_lanes_stand(const FollowCtx& cx, const Walk& w, bool active, bool go)
{
    const bool isB = cx.isB;
    Tentative t;
    const int kn = isB ? (8 - w.known) & 7 : w.known;
    const int su = next_dir(w.n, kn);
    const int srch = isB ? (8 - su) & 7 : su;
    const int r_next = w.r + cx.dir_off(srch);
    const int st_r = isB ? w.r_ahead : w.r, st_d = isB ? w.known ^ 4 : w.known;
    const int nw_r = isB ? w.r : r_next, nw_d = isB ? srch : srch ^ 4; // ... and after this step
    const int fl = (go ? 1 : 0) | (active ? 2 : 0) | (w.steps > 0 ? 4 : 0) | (w.status << 3);
    const int o_st_r = pair_swap(st_r), o_nw_r = pair_swap(nw_r), o_misc = pair_swap(st_d | (nw_d << 3) | (fl << 6));
    const int o_st_d = o_misc & 7, o_nw_d = (o_misc >> 3) & 7, o_fl = o_misc >> 6;
    const bool o_go = (o_fl & 1) != 0;
    const bool met = active && (o_fl & 2) && st_r == o_st_r && st_d == o_st_d && ((fl | o_fl) & 4);
    // the forward lane's step completes the cycle: the backward lane must not take the same step from the other side
    t.fwd_closes = (isB ? o_nw_r : nw_r) == (isB ? st_r : o_st_r) && (isB ? o_nw_d : nw_d) == (isB ? st_d : o_st_d) && (o_go || !isB);
    const bool partner_gave_up = active && (o_fl >> 3) != 0;
    t.ends = met || partner_gave_up || (isB && active && t.fwd_closes);
    t.srch = srch; t.r_next = r_next;
    return t;
}

// This lane accounts for one forward step of the border -- from its pixel, in direction s, having arrived from s_end -- and moves.
// -> the walk ends with this step
__device__ __forceinline__ bool account_step(const ContourArgs& a, const FollowCtx& cx, Walk& w, const Tentative& t)
{
    const bool isB = cx.isB;
    const int srch = t.srch;
    const int s = isB ? w.known : srch, s_end = isB ? srch : w.known;
    const int r = w.r;
    const bool east_bg = (unsigned)(s - 1) < (unsigned)s_end; // the East neighbour was examined and is background
    const int re = east_bg ? r + 1 : 0x7fffffff;
    w.min_ebg = re < w.min_ebg ? re : w.min_ebg;
    w.min_fg = r < w.min_fg ? r : w.min_fg;
    w.bx0 = w.x < w.bx0 ? w.x : w.bx0; w.bx1 = w.x > w.bx1 ? w.x : w.bx1;
    w.by0 = w.y < w.by0 ? w.y : w.by0; w.by1 = w.y > w.by1 ? w.y : w.by1;
    // (x,y) is a CHAIN_APPROX_SIMPLE vertex when the direction changes there.  Forward lane: the run that ENDS here closes,
    // then this step opens / extends the next one; backward lane: this step extends the run that STARTS here, then it closes.
    const bool vertex = s != (s_end ^ 4);
    w.run += isB ? 1 : 0;
    const int len = vertex ? w.run : 0;
    const bool first_vertex = vertex && !w.has_head; // the lane's first run is joined with the partner's at the end
    w.head = first_vertex ? len : w.head;
    w.has_head = w.has_head || vertex;
    const int kk = first_vertex ? 0 : len;
    const bool odd = ((isB ? s : s_end) & 1) != 0;
    w.axis += odd ? 0 : kk;
    w.diag += w.pend;
    const int kd = odd ? kk : 0;                                  // diag_len[0] = 0
    w.pend = cx.diag_len[kd < 63 ? kd : 63];
    if (kd > 63) w.pend = run_length(1, kd);                      // (a diagonal run longer than the table: rare)
    w.npts += vertex ? 1 : 0;
    w.run = (vertex ? 0 : w.run) + (isB ? 0 : 1);
    const int dx = dir_dx(s), dy = dir_dy(s);
    const int cross = __mul24(w.x, dy) - __mul24(dx, w.y); // x*ny - nx*y (coordinates below 2^15)
    w.a00 += cross;
    w.a10 += (int64_t)cross * (2 * w.x + dx);
    w.a01 += (int64_t)cross * (2 * w.y + dy);
    w.steps++;
    const bool aborted = (w.abort_on_fg ? r : re) < w.abort_lt, limit = w.steps > a.max_steps;
    // the walk ends here when it has left its border's claim (aborted), ran too long, or -- forward lane -- this step completes
    // the cycle (the backward lane sees the same condition and stops as well; known = the way back from the meeting pixel: the
    // direction of the forward tail)
    const bool stop = aborted || limit || (!isB && t.fwd_closes);
    w.status = aborted ? 1 : (limit ? 2 : w.status);
    // move (a lane that stops moves too: nothing reads its position afterwards)
    w.x += dir_dx(srch); w.y += dir_dy(srch); w.known = srch ^ 4;
    w.r_ahead = w.r; w.r = t.r_next;
    return stop;
}

// one step of every running lane (no global load: a lane that steps onto its window's rim pauses until the window is staged anew)
__device__ __forceinline__ void follow_step(const ContourArgs& a, const FollowCtx& cx, Walk& w, bool& active, bool& paused, bool& finished)
{
    const bool go = active && !paused;
    const Tentative t = where_the_lanes_stand(cx, w, active, go);
    if (t.ends) {
        active = false; finished = true; paused = false;
    } else if (go) {
        const bool stop = account_step(a, cx, w, t);
        paused = !stop && w.on_rim();
        w.n = cx.nbr8(w, w.x, w.y, cx.up_dy); // (garbage while paused: read again from the new window)
        active = !stop; finished = stop;
    }
}

__global__ __launch_bounds__(64) void contour_follow_kernel(ContourArgs a)
{
    __shared__ uint64_t win[64][64]; // [row of the window][window]
    __shared__ double diag_len[64];
    const int lane = threadIdx.x;
    diag_len[lane] = run_length(1, lane);
    const WalkList wl{a.follow_list ? a.link_list : a.walk_list, a.walk_count[2 * a.follow_list], &a.walk_count[2 * a.follow_list + 1]};
    ContourWork* const works = (ContourWork*)a.work;
    const uint32_t image_words = (uint32_t)mask_image_words(a.H, a.words_per_row);
    const bool isB = (lane & 1) != 0;
    const FollowCtx cx{(const uint8_t*)&win[0][0], diag_len, a.W + 1, isB, isB ? 1 : -1};
    Walk w;
    w.status = 0; w.meta = 0; w.n = 0; w.known = 0; w.x = 0; w.y = 0; w.wx0 = 0; w.wy0 = 0; w.wslot = lane; w.steps = 0; w.s0 = 0;
    bool active = false, paused = false, finished = false; // (see Walk)
    bool drained = false;                  // (wave-uniform) the list has no more entries
    bool first_fill = true;                // (wave-uniform) the wave has not taken entries yet
    PhaseClock clock{a.follow_dbg != nullptr && a.follow_list == a.follow_dbg_list, 0, {0, 0, 0, 0, 0, 0, 0, 0}};
    clock.t_prev = clock.on ? wall_clock64() : 0;
    __syncthreads();
    for (;;) {
        exchange_and_store_finished(a, cx, works, w, finished);
        clock.lap(0);
        // ---- refill: new walks for the idle pairs; new windows for them and for the paused lanes ----
        const uint64_t busy = __ballot(active);
        const uint64_t busy_pairs = (busy | (busy >> 1)) & 0x5555555555555555ull; // bit 2i: pair i holds a walk
        int kind = 0, ex = 0;
        const bool take = take_entries(wl, lane, busy, busy_pairs, w, drained, first_fill, clock, kind, ex);
        place_windows(w, lane, paused);
        const uint64_t stage = __ballot((take && !isB) || paused);
        if (__ballot(take || paused)) {
            stage_windows(a, win, w, stage, lane, image_words, cx.RS);
            if (take) start_walk(cx, w, kind, ex, active, paused, finished);
            else if (paused) paused = false; // (its window now lies around its pixel)
            if (active && !paused) w.n = cx.nbr8(w, w.x, w.y, cx.up_dy);
        }
        clock.lap(1);
        if (__ballot(active || finished) == 0) break; // nothing in flight (and nothing left in the list, or the refill would have run)
        // ---- FOLLOW_K steps of every running lane ----
        for (int k = 0; k < FOLLOW_K; k++) {
            follow_step(a, cx, w, active, paused, finished);
            if (clock.on) { clock.tk[3]++; clock.tk[4] += (uint64_t)__popcll(__ballot(active && !paused)); }
            if (__ballot(active && !paused) == 0) break;
        }
        clock.lap(2);
    }
    if (clock.on && lane == 0)
        for (int i = 0; i < 8; i++) a.follow_dbg[(size_t)blockIdx.x * 8 + i] = clock.tk[i];
}

void launch_contour_follow(const ContourArgs& a, int grid, hipStream_t s)
{
    hipLaunchKernelGGL(contour_follow_kernel, dim3(grid), dim3(64), 0, s, a);
}

} // namespace mocap
