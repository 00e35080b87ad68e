// blob_contour_image.hip -- the contour stage's per-image kernels: start candidates, the tree of the borders and the ordered
// centroids (contours_kernel<1> / <2>, around the batch-wide walks of blob_contour_follow.hip), and the whole job as one kernel per
// image with the lone-lane walker `follow` (contours_kernel<0>).  The algorithm: contours_dev.h; the launches: launch_contours below.
#include "contours_dev.h"

namespace mocap {

namespace {

// lane L receives lane L - 1's / L + 1's value (0 at the ends of the wave and from lanes that are switched off)
__device__ __forceinline__ uint32_t lane_prev(uint32_t v) { return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x138 /*wave_shr:1*/, 0xf, 0xf, true); }
__device__ __forceinline__ uint32_t lane_next(uint32_t v) { return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x130 /*wave_shl:1*/, 0xf, 0xf, true); }

// Border following by one LANE.  Follows the border through pixel (sx,sy) whose neighbour in direction `first`
// (4 = W for an outer start, 0 = E for a hole start) is background.  Aborts when a border pixel with raster index
// < abort_fg or an East-side background pixel with raster index < abort_ebg is met.  Every lane of a wave follows
// its own border: the walker state, the three 64-column mask rows around the current pixel and all sums live in
// the lane's registers; a vertical move loads one new row (three mask words through L1/L2), a move near the edge of
// the 64-column window re-centres it.
//
// The polygon sums are accumulated per border step: splitting a straight polygon edge at the pixels it passes
// through leaves a00, a10, a01 unchanged (they are exact line integrals), so no vertex list is needed.  The
// perimeter needs the CHAIN_APPROX_SIMPLE segments: axis-parallel runs add their integer length, a diagonal run of
// k steps adds the float32 sqrt(2k^2) -- every term is a float32 >= 1 and the total stays far below 2^29, so the
// double sum is exact in any order.
// `win` (optional): 64 rows of the mask from row sy - 1 down, columns sx - 31 .. sx + 32, staged in LDS by the caller;
// rows are taken from there while the walk stays inside that window's columns.
// WS: distance (in 64-bit words) between consecutive rows of `win` (1: a window of its own; 64: row-major over the 64 windows
// of a wave, so that the lanes' reads fall into different LDS banks).
template <int WS = 1>
__device__ __forceinline__ void follow(const Mask& M, int sx, int sy, int first, int abort_fg, int abort_ebg, int max_steps,
                                       Trace& T, const double* diag_len, const uint64_t* win = nullptr)
{
    int64_t a00 = 0, a10 = 0, a01 = 0;
    int npts = 0, steps = 0;
    int min_fg = sy * M.RS + sx, min_ebg = 0x7fffffff;
    int bx0 = sx, bx1 = sx, by0 = sy, by1 = sy;
    T.status = 0;
    T.per = 0.0;

    int x0 = sx - 31; // window columns x0 .. x0+63
    int x = sx, y = sy;
    const int wy0 = sy - 1;
    bool staged = win != nullptr; // the LDS window still matches x0
    auto fetch = [&](int yy) -> uint64_t {
        const unsigned r = (unsigned)(yy - wy0);
        if (staged && r < 64u) return win[r * WS];
        return row64(M, yy, x0);
    };
    uint64_t rU = fetch(y - 1), rM = fetch(y), rD = fetch(y + 1);

    // occupancy of the 8 neighbours of (x,y), bit s = direction code s (0=E 1=NE 2=N 3=NW 4=W 5=SW 6=S 7=SE)
    auto nbr8 = [&]() -> uint32_t {
        const int c = x - x0 - 1; // column x-1 at bit 0
        return nbr_code((uint32_t)(rU >> c) & 7u, (uint32_t)(rM >> c) & 7u, (uint32_t)(rD >> c) & 7u);
    };

    uint32_t n = nbr8();
    int s = first_neighbour(n, first), s_end;
    if (s == first) { // isolated pixel: one vertex, zero area, zero perimeter
        T.a00 = T.a10 = T.a01 = 0;
        T.npts = 1; T.steps = 0;
        T.min_fg = min_fg; T.min_ebg = sy * M.RS + sx + 1;
        T.bx0 = T.bx1 = sx; T.by0 = T.by1 = sy;
        return;
    }
    const int i1x = sx + dir_dx(s), i1y = sy + dir_dy(s);
    int prev_s = s ^ 4;       // direction of the step that will close the border (arrives at the start)
    int run = 0;              // steps taken in direction prev_s since the last vertex
    int first_len = 0;        // length of the run leaving the start when the start is not a vertex (merged at the end)
    int axis = 0;             // total length of the axis-parallel segments
    double diag = 0.0;        // total length of the diagonal segments
    double pend = 0.0;        // table value fetched in the previous step, added one step later (hides the LDS latency)
    const int abort_lt = abort_fg > abort_ebg ? abort_fg : abort_ebg; // exactly one of the two is armed (the other is -1)
    const bool abort_on_fg = abort_fg >= 0;
    int status = 0;
    // The loop body is written with selects: a lane-divergent branch costs two EXEC updates and their wait states,
    // a select costs one instruction.  Branches remain only for leaving the loop, for re-centring the window and
    // for the two row sources.
    for (;;) {
        s_end = s;
        s = next_dir(n, s_end);
        const int r = y * M.RS + x;
        const bool east_bg = (unsigned)(s - 1) < (unsigned)s_end; // the East neighbour was examined and is background
        const int re = east_bg ? r + 1 : 0x7fffffff;
        min_ebg = re < min_ebg ? re : min_ebg;
        min_fg = r < min_fg ? r : min_fg;
        // (x,y) is a CHAIN_APPROX_SIMPLE vertex when the direction changes: close the run that ends here
        const bool vertex = s != prev_s;
        const bool open_start = vertex && npts == 0 && steps > 0; // the start was not a vertex: its run is closed at the end
        first_len = open_start ? run : first_len;
        const int k = (vertex && !open_start) ? run : 0;
        const bool odd = (prev_s & 1) != 0;
        axis += odd ? 0 : k;
        diag += pend;
        const int kd = odd ? k : 0;                                  // diag_len[0] = 0
        pend = diag_len[kd < 63 ? kd : 63];
        if (kd > 63) pend = run_length(1, kd);                        // (a diagonal run longer than the table: rare)
        npts += vertex ? 1 : 0;
        prev_s = s;
        run = vertex ? 1 : run + 1;
        const int dx = dir_dx(s), dy = dir_dy(s);
        const int nx = x + dx, ny = y + dy;
        const int cross = x * dy - dx * y; // x*ny - nx*y
        a00 += cross;
        a10 += (int64_t)cross * (2 * x + dx);
        a01 += (int64_t)cross * (2 * y + dy);
        steps++;
        const bool aborted = (abort_on_fg ? r : re) < abort_lt;
        const bool closed = nx == sx && ny == sy && x == i1x && y == i1y;
        if (aborted || closed || steps > max_steps) {
            status = aborted ? 1 : (closed ? 0 : 2);
            break;
        }
        bx0 = nx < bx0 ? nx : bx0; bx1 = nx > bx1 ? nx : bx1;
        by0 = ny < by0 ? ny : by0; by1 = ny > by1 ? ny : by1;
        // move, keeping the three cached rows around the current pixel
        const int lx = nx - x0;
        if (lx < 1 || lx > 62) { // left the window: re-centre it on the new pixel (rare), or return to the staged one
            const int wl = nx - (sx - 31); // column of the new pixel in the staged window
            staged = win != nullptr && wl >= 1 && wl <= 62;
            x0 = staged ? sx - 31 : nx - 31;
            rU = fetch(ny - 1); rM = fetch(ny); rD = fetch(ny + 1);
        } else {
            const uint64_t nw = fetch(ny + dy); // (dy = 0: the middle row again, unused)
            const uint64_t oU = rU, oM = rM, oD = rD;
            rU = dy > 0 ? oM : (dy < 0 ? nw : oU);
            rM = dy > 0 ? oD : (dy < 0 ? oU : oM);
            rD = dy > 0 ? nw : (dy < 0 ? oM : oD);
        }
        x = nx; y = ny;
        s = (s + 4) & 7;
        n = nbr8();
    }
    T.status = status;
    if (status) return;
    // the run that arrives at the start, merged with the run that left it when the start is not a vertex
    diag += pend;
    {
        const int k = run + first_len;
        if (prev_s & 1) diag += k < 64 ? diag_len[k] : run_length(1, k);
        else axis += k;
    }
    T.a00 = a00; T.a10 = a10; T.a01 = a01;
    T.npts = npts; T.steps = steps;
    T.min_fg = min_fg; T.min_ebg = min_ebg;
    T.bx0 = bx0; T.bx1 = bx1; T.by0 = by0; T.by1 = by1;
    T.per = (double)axis + diag;
}

} // namespace

constexpr int NTHREADS = 256, NWAVES = NTHREADS / 64;
constexpr int NWIN = 16; // candidates per image whose mask window is staged in LDS

// ---- one image's state in LDS.  Declared by contours_body, piece by piece, so that an instantiation holds only what its phases touch
// (the tree kernel no candidates and no windows, the candidates kernel no borders).  The counters are single words of their own -- n_cell,
// n_cand, n_rec, n_kept, n_open and err (1 = a walk ran into the step limit, 2 = a link without owner, 3 = nesting deeper than MAXD) -- and
// each phase is handed the ones it touches.
struct Borders { // per border, in the order the walks finished: discovery key, start pixel, kind, filter result, links
    int32_t key[MAXR];
    int16_t sx[MAXR], sy[MAXR], link[MAXR], parent[MAXR]; // link: the border that owns the crack left of the start (-1 the frame, -2 waits for its walk)
    uint8_t hole[MAXR], kept[MAXR];
    uint8_t res[MAXR];                                    // 1 = the border's parent follows from the bounding boxes alone (parents_from_boxes)
};
union TreeOrCells { // phase A's list of cells to scan; afterwards the borders' boxes and the kept contours
    uint16_t cell_list[MAXCELL];
    struct {
        alignas(8) int16_t box[MAXR][4];                  // bounding box of each border: x0, y0, x1, y1 (read as one 8-byte word)
        int16_t kept_idx[MAXK];
        int8_t kept_depth[MAXK];
    } tree;
};
union RangesOrWindows { // phase A: first word | words << 12 of each listed cell's column range; phase B: mask windows of the first NWIN candidates (see follow)
    uint16_t cell_rng[MAXCELL];
    uint64_t win[NWIN][64];
};
static_assert(sizeof(TreeOrCells) == sizeof(uint16_t) * MAXCELL && sizeof(RangesOrWindows) == sizeof(uint16_t) * MAXCELL, "the later phases' arrays fit where phase A's lists were");
using Tree = decltype(TreeOrCells::tree);

// What every phase of one image sees besides the LDS state it is handed: the arguments, the image's mask, workspace and count, and which
// thread this is.  The phases are its member functions, in the order contours_body runs them.  Each is entered by the whole workgroup
// behind a barrier and -- unless it says otherwise -- ends with one, so that the next phase may read what it left in LDS.
struct ImageJob {
    const ContourArgs& a;
    const int image;
    const Mask M;
    ContourWork& work;
    int32_t* const out_count;
    uint64_t* const tick; // optional phase clock (MOCAP_CONTOUR_TIMING=1, a debugging aid): 100 MHz ticks at the phase boundaries
    const int tid, lane, wv;

    __device__ __forceinline__ void stamp(int i) const { if (tick && tid == 0) tick[i] = wall_clock64(); }

    // the image ends here with a BLOB_ERR_* code instead of a count (no barrier: the caller returns)
    __device__ __forceinline__ void fail_image(int code) const
    {
        if (tid == 0) { *out_count = code; if (a.dbg_count) a.dbg_count[image] = 0; }
    }

    // Tree kernel's prologue: the follow kernel's records.  Reads the workspace's counts, then the small per-border fields of every
    // border into b and t.box (links: the first pass's for the second pass, else none).  False, before anything is copied, when the
    // follow kernel recorded more borders than MAXR or a walk that hit the step limit (n_rec, err say which).
    __device__ __forceinline__ bool load_follow_records(bool second_pass, int& n_rec, int& err, int& n_open, Borders& b, Tree& t) const
    {
        if (tid == 0) { n_rec = work.st_nrec; err = work.st_err; n_open = 0; }
        __syncthreads();
        if (n_rec > MAXR || err) return false;
        for (int c = tid; c < n_rec; c += NTHREADS) {
            b.key[c] = work.rkey[c]; b.sx[c] = work.rsx[c]; b.sy[c] = work.rsy[c];
            b.hole[c] = work.rhole[c]; b.kept[c] = work.rkept[c];
            b.link[c] = second_pass ? work.rlink[c] : (int16_t)-1; b.parent[c] = -1;
            t.box[c][0] = work.rbox[c][0]; t.box[c][1] = work.rbox[c][1]; t.box[c][2] = work.rbox[c][2]; t.box[c][3] = work.rbox[c][3];
        }
        __syncthreads();
        return true;
    }

    // ---- phase A: candidate starts -------------------------------------------------------------------------------
    // A border can only start where the mask has set pixels.  The filter kernel leaves an occupancy word per
    // (strip, chunk): bit g = rows 8g..8g+7 of the chunk contain set pixels in that 240-column strip.  Occupied
    // cells, plus their right and lower neighbours (a hole can start in an empty cell whose W / N neighbour pixel
    // lies in the occupied one), are scanned row by row with word-parallel bit tests; without the occupancy words
    // (mask supplied by the caller), or when the occupied cells outnumber the list (MAXCELL), every cell is scanned.
    //
    // First half (frames of the context's own mask only): lists the cells to scan in cell_list[0 .. n_cell) -- n_cell may pass MAXCELL,
    // the list does not -- and the mask words to examine in each in cell_rng.  Reads the occupancy words and the tiles' boxes.
    __device__ __forceinline__ void list_cells(const uint32_t* cells, const uint32_t* boxes, int& n_cell, uint16_t* cell_list, uint16_t* cell_rng) const
    {
        const int R = a.rows_per_chunk, NS = a.n_strips, NCH = a.n_chunks;
        const int gpc = (R + 7) >> 3;                       // 8-row groups per chunk
        // one task = one (chunk, strip) occupancy word: its own groups, and the groups its right and lower
        // neighbours must scan because of it
        for (int t = tid; t < NCH * NS; t += NTHREADS) {
            const int ch = t / NS, st = t - ch * NS;
            if (ch * R >= a.H) continue;
            const uint32_t own = cells[t] & 0x7fffffffu;
            const uint32_t left = st > 0 ? cells[t - 1] & 0x7fffffffu : 0u;
            const uint32_t up = ch > 0 ? cells[t - NS] & 0x7fffffffu : 0u;
            const uint32_t upbit = (up >> (gpc - 1)) & 1u;
            uint32_t scan = own | left | (own << 1) | upbit;
            scan &= (1u << gpc) - 1u;
            if (!scan) continue;
            // columns that can hold set pixels: the tile's output region and the scan's box (settle, BoxArgs::cur_box);
            // a hole start lies at most one column right of them
            const int xa = 240 * st, xb = xa + 240 < a.W ? xa + 240 : a.W;
            int ox0 = xa, ox1 = xb - 1, ux0 = xa, ux1 = xb - 1;
            if (boxes) {
                box_columns(*(const uint4*)(boxes + 4 * (size_t)t), ox0, ox1);
                if (upbit) box_columns(*(const uint4*)(boxes + 4 * (size_t)(t - NS)), ux0, ux1);
                ox0 = ox0 < xa ? xa : ox0; ox1 = ox1 > xb - 1 ? xb - 1 : ox1;
                ux0 = ux0 < xa ? xa : ux0; ux1 = ux1 > xb - 1 ? xb - 1 : ux1;
                if (ox0 > ox1) { ox0 = xa; ox1 = xb - 1; }
                if (ux0 > ux1) { ux0 = xa; ux1 = xb - 1; }
            }
            const uint32_t ownish = own | (own << 1);
            while (scan) {
                const int g = __ffs((int)scan) - 1;
                scan &= scan - 1;
                if (ch * R + 8 * g >= a.H || 8 * g >= R) continue;
                const int slot = atomicAdd(&n_cell, 1);
                if (slot >= MAXCELL) continue;
                cell_list[slot] = (uint16_t)((ch * NS + st) * gpc + g);
                int c0 = 0x7fffffff, c1 = -1;
                if ((ownish >> g) & 1u) { c0 = ox0; c1 = ox1; }
                if ((left >> g) & 1u) { c0 = c0 < xa ? c0 : xa; c1 = c1 > xa ? c1 : xa; }
                if (g == 0 && upbit) { c0 = c0 < ux0 ? c0 : ux0; c1 = c1 > ux1 ? c1 : ux1; }
                const int k0 = c0 >> 5, k1 = c1 >> 5;
                cell_rng[slot] = (uint16_t)(k0 | ((k1 - k0 + 1) << 12)); // k0 < 4096 (checked on the host), at most 10 words
            }
        }
        __syncthreads();
    }

    // Second half: scans the listed cells (or every cell: a caller's mask, or more cells than the list holds) and leaves the starts
    // that pass the local tests in cand[0 .. n_cand) as x | hole << 15 | y << 16; n_cand may pass MAXC, the array does not.
    __device__ __forceinline__ void scan_cells(const uint32_t* cells, int n_cell, const uint16_t* cell_list, const uint16_t* cell_rng, int& n_cand, uint32_t* cand) const
    {
        const int R = a.rows_per_chunk, NS = a.n_strips, NCH = a.n_chunks;
        const int gpc = (R + 7) >> 3;
        const int n_cells = NCH * NS * gpc;
        // A frame with more cells to scan than the list holds (MAXCELL; a 3840 x 2160 frame has 16 strips x 286 groups) is no error: like a
        // caller's mask it has every cell scanned, over the whole width of its strip.
        const bool listed = cells != nullptr && n_cell <= MAXCELL; // cell_list / cell_rng hold the cells and the words to examine
        const int ncl = listed ? n_cell : n_cells;
        // One task = one cell, taken by a group of 8 lanes: lane j of the group holds row j of the cell (the lanes of a load lie
        // in one or two lines of the blocked mask) and loads 8 consecutive words of it, kf - 1 + p0 .. kf + p0 + 6 (kf = first
        // word of the cell's column range, see above); the row above comes from lane j - 1 (DPP), lane 0 loads it.  Words
        // 1..6 are tested with their neighbours; ranges longer than 6 words take further passes.
        const int sub = tid & 7, grp8 = tid >> 3;
        for (int ci0 = 0; ci0 < ncl; ci0 += NTHREADS / 8) {
            const int ci = ci0 + grp8;
            const bool cv = ci < ncl;
            const int cell = cv ? (listed ? (int)cell_list[ci] : ci) : 0;
            const int g = cell % gpc, st = (cell / gpc) % NS, ch = cell / (gpc * NS);
            const int y0 = ch * R + 8 * g;
            const int yend = (ch + 1) * R < a.H ? (ch + 1) * R : a.H;
            const int xa = 240 * st, xb = xa + 240 < a.W ? xa + 240 : a.W; // the strip's columns [xa, xb)
            const int ka = xa >> 5, kb = (xb - 1) >> 5;
            int kf = ka, cnt = kb - ka + 1;
            if (listed && cv) { const uint32_t rg = cell_rng[ci]; kf = (int)(rg & 0xfffu); cnt = (int)(rg >> 12); }
            if (!cv) cnt = 0;
            const int y = y0 + sub;
            const bool rowv = y < yend && 8 * g + sub < R;
            for (int p0 = 0; p0 < cnt; p0 += 6) { // (cnt is uniform in the group: its 8 lanes run the same passes)
                uint32_t rw[8], up[8];
#pragma unroll
                for (int i = 0; i < 8; i++) rw[i] = rowv ? M.word(y, kf - 1 + p0 + i) : 0u;
                // the row above: lane j - 1's row, exchanged while every lane of the group is active (before any lane-divergent code)
#pragma unroll
                for (int i = 0; i < 8; i++) up[i] = lane_prev(rw[i]);
                if (sub == 0) {
#pragma unroll
                    for (int i = 0; i < 8; i++) up[i] = M.word(y0 - 1, kf - 1 + p0 + i);
                }
#pragma unroll
                for (int i = 1; i <= 6; i++) {
                    const int k = kf - 1 + p0 + i;
                    if (!rowv || !(k < kf + cnt && k >= ka && k <= kb)) continue;
                    const uint32_t w = rw[i], n = up[i];
                    const uint32_t prev_w = rw[i - 1], prev_n = up[i - 1], next_w = rw[i + 1], next_n = up[i + 1];
                    const uint32_t Wn = (w << 1) | (prev_w >> 31);
                    // Necessary conditions, evaluated on the 64 columns starting at this word (this word + the next):
                    // a raster-first foreground pixel starts a run none of whose pixels touches (8-connectivity) the
                    // row above; a raster-first hole pixel starts a background run none of whose pixels has
                    // background directly above (4-connectivity).  "Touches" are spread leftwards along the run for 12
                    // columns; beyond that the candidate is merely kept -- the follow step decides.
                    const uint64_t w64 = (uint64_t)w | ((uint64_t)next_w << 32), n64 = (uint64_t)n | ((uint64_t)next_n << 32);
                    const uint64_t above64 = n64 | (n64 << 1) | (uint64_t)(prev_n >> 31) | (n64 >> 1); // NE of column 63 unknown: treated as clear
                    uint32_t outer = w & ~Wn & ~(uint32_t)above64;
                    if (outer) {
                        uint64_t touch = w64 & above64;
#pragma unroll
                        for (int i = 0; i < 12; i++) touch |= (touch >> 1) & w64;
                        outer &= ~(uint32_t)touch;
                    }
                    uint32_t hole = ~w & Wn & n;
                    if (hole) {
                        uint64_t bg64 = ~w64, touch = bg64 & ~n64;
#pragma unroll
                        for (int i = 0; i < 12; i++) touch |= (touch >> 1) & bg64;
                        hole &= ~(uint32_t)touch;
                    }
                    // keep only this strip's columns (and, for holes, columns inside the image)
                    const int lo = xa - 32 * k, hi = xb - 32 * k; // bit range [lo, hi)
                    uint32_t m = 0xffffffffu;
                    if (lo > 0) m &= ~((1u << lo) - 1u);
                    if (hi < 32) m &= (1u << hi) - 1u;
                    outer &= m; hole &= m;
                    while (outer) {
                        const int b = __ffs((int)outer) - 1;
                        outer &= outer - 1;
                        const int slot = atomicAdd(&n_cand, 1);
                        if (slot < MAXC) cand[slot] = (uint32_t)(32 * k + b) | ((uint32_t)y << 16);
                    }
                    while (hole) {
                        const int b = __ffs((int)hole) - 1;
                        hole &= hole - 1;
                        const int slot = atomicAdd(&n_cand, 1);
                        if (slot < MAXC) cand[slot] = (uint32_t)(32 * k + b) | ((uint32_t)y << 16) | 0x8000u;
                    }
                }
            }
        }
        __syncthreads();
    }

    // Candidates kernel's epilogue: one self-contained entry per candidate into the batch's walk list, the counts the follow kernel adds
    // to into the workspace.  `wbase` is one LDS word.  Ends without a barrier: the image is finished.
    __device__ __forceinline__ void hand_over_candidates(int n_cand, const uint32_t* cand, uint32_t& wbase) const
    {
        const int nc1 = n_cand;
        if (tid == 0) {
            work.st_ncand = nc1; work.st_nrec = 0; work.st_err = 0; work.st_pending = 0;
            wbase = nc1 ? atomicAdd(&a.walk_count[0], (uint32_t)nc1) : 0u;
        }
        __syncthreads();
        for (int c = tid; c < nc1; c += NTHREADS) {
            const uint32_t v = cand[c];
            a.walk_list[wbase + (uint32_t)c] = walk_entry(image, (int)(v & 0x7fffu), (int)(v >> 16), (int)((v >> 15) & 1u));
        }
    }

    // ---- phase B (one-kernel form): one lane follows one candidate; the raster-first ones become records -------------------------
    // Reads cand; leaves the full records in work.recs and the small fields in b and t.box, n_rec of them (n_rec may pass MAXR, the
    // arrays do not), err = 1 when a walk hit the step limit.  win: this phase's own, diag_len: the table of diagonal run lengths.
    __device__ __forceinline__ void walk_candidates(int n_cand, const uint32_t* cand, uint64_t (*win)[64], const double* diag_len, int& n_rec, int& err, int& dbg_steps, Borders& b, Tree& t) const
    {
        const int nc = n_cand;
        // The walks read the mask rows below each start one at a time.  For the first NWIN candidates (all of them, in a
        // typical frame) the 64 rows from the start downwards are staged in LDS first, one row per lane: one round of
        // parallel loads instead of a dependent L2 round trip per vertical move.
        for (int c = wv; c < nc && c < NWIN; c += NWAVES) {
            const uint32_t v = cand[c];
            const int sx = (int)(v & 0x7fff) - (int)((v >> 15) & 1u), sy = (int)(v >> 16);
            win[c][lane] = row64(M, sy - 1 + lane, sx - 31);
        }
        __syncthreads();
        for (int c = tid; c < nc; c += NTHREADS) {
            const uint32_t v = cand[c];
            const int is_hole = (v >> 15) & 1, x = v & 0x7fff, y = v >> 16;
            const int key = y * M.RS + x;
            Trace T;
            const uint64_t* w = c < NWIN ? win[c] : nullptr;
            if (!is_hole) follow(M, x, y, 4, key, -1, a.max_steps, T, diag_len, w);
            else follow(M, x - 1, y, 0, -1, key, a.max_steps, T, diag_len, w);
            if (T.status == 2) atomicMax(&err, 1);
            if (tick) atomicMax(&dbg_steps, T.status == 0 ? T.steps : 0);
            if (T.status != 0) continue;
            const int slot = atomicAdd(&n_rec, 1);
            if (slot >= MAXR) continue;
            ContourRec r;
            make_record(r, key, is_hole, x - is_hole, y, T.npts, T.steps, T.a00, T.a10, T.a01, T.per, a.min_area, a.min_circ);
            work.recs[slot] = r;
            store_small_fields(slot, r, T.bx0, T.by0, T.bx1, T.by1, b.key, b.sx, b.sy, b.hole, b.kept, t.box);
            b.link[slot] = -1; b.parent[slot] = -1;
        }
        __syncthreads();
    }

    // ---- phase C0: the parents the bounding boxes alone decide (no mask access, no link) ----------------------------
    //   An outer border's parent is the hole border of the hole its component lies in, or the frame; lying in a hole puts every
    //   pixel of the border, its start included, inside that hole border's box: no hole border's box around the start -> the frame.
    //   A hole border's parent is the outer border of its own component, whose box contains every pixel of the component, the
    //   hole's border pixels included: exactly one outer border's box around the hole border's box -> that one.
    //   Everything else (nested rings, boxes that overlap) goes through the link below.  A frame of separate, hole-free markers --
    //   the usual IR frame -- needs nothing more than this.
    // Reads b.hole, b.sx, b.sy, t.box; leaves b.res and, where res is set, b.parent.
    __device__ __forceinline__ void parents_from_boxes(int nr, Borders& b, const Tree& t) const
    {
        for (int c = tid; c < nr; c += NTHREADS) {
            const int me = b.hole[c];
            int hits = 0, found = -1;
            if (!me) {
                const int x = b.sx[c], y = b.sy[c];
                for (int j = 0; j < nr; j++)
                    hits += b.hole[j] && t.box[j][0] <= x && x <= t.box[j][2] && t.box[j][1] <= y && y <= t.box[j][3];
            } else {
                for (int j = 0; j < nr; j++)
                    if (!b.hole[j] && t.box[j][0] <= t.box[c][0] && t.box[c][2] <= t.box[j][2] && t.box[j][1] <= t.box[c][1] && t.box[c][3] <= t.box[j][3]) { hits++; found = j; }
            }
            const bool res = me ? hits == 1 : hits == 0;
            b.res[c] = res ? 1 : 0;
            if (res) b.parent[c] = (int16_t)found;
        }
        __syncthreads();
    }

    // ---- phase C1: link = the border that owns the crack met when scanning left from the start ------------------
    //   outer border: nearest foreground pixel left of the start on the same row -> its East crack
    //   hole border : left end of the foreground run holding the start pixel     -> its West crack
    // One wave per border (wave-uniform control flow).  First pass: leaves b.link of every border that parents_from_boxes left open; with
    // DEFER (tree kernel) and a.defer_links, the first MAXA of n_open links that only a walk settles go into open_link instead (b.link = -2).  Second pass:
    // looks up the borders the link walks have identified.  err: 1 = a walk failed, 2 = a link whose owner is no recorded border.
    template <bool DEFER>
    __device__ __forceinline__ void find_links(int nr, bool second_pass, int& err, uint64_t* open_link, int& n_open, Borders& b, const Tree& t, const double* diag_len) const
    {
        if (second_pass) {
            // the links the first pass left open: the second follow pass has identified the border each of their cracks belongs to
            for (int c = tid; c < nr; c += NTHREADS) {
                if (b.link[c] != -2) continue;
                const int lkey = work.link_key[c], ltype = work.link_type[c];
                int found = -2;
                for (int j = 0; j < nr; j++)
                    if (b.key[j] == lkey && b.hole[j] == ltype) { found = j; break; }
                if (found == -2) atomicMax(&err, 2);
                b.link[c] = (int16_t)found;
            }
        }
        for (int c = wv; c < nr && !second_pass; c += NWAVES) {
            if (b.res[c]) continue; // (wave-uniform)
            const int r_is_hole = b.hole[c], r_sx = b.sx[c], y = b.sy[c];
            // hole: nearest background pixel at/left of the start; outer: nearest foreground pixel left of it.
            // The words of the row up to that column are examined 64 at a time, one per lane, right to left.
            const int xs = r_is_hole ? r_sx : r_sx - 1;
            int qx = r_is_hole ? 0 : -1;
            for (int kbase = xs >> 5; kbase >= 0 && xs >= 0; kbase -= 64) {
                int k = kbase - lane;
                uint32_t w = k >= 0 ? M.word(y, k) : 0u;
                if (r_is_hole) w = k >= 0 ? ~w : 0u;
                if (k == (xs >> 5)) w &= (2u << (xs & 31)) - 1u; // only columns <= xs
                uint64_t bal = __ballot(w != 0u);
                if (bal) {
                    int src = __ffsll((long long)bal) - 1; // lowest lane = rightmost word
                    uint32_t ww = (uint32_t)__builtin_amdgcn_readlane((int)w, src);
                    int px = 32 * (kbase - src) + 31 - __clz((int)ww);
                    qx = r_is_hole ? px + 1 : px;
                    break;
                }
            }
            if (qx < 0) continue; // nothing to the left: the frame (link stays -1)
            // The crack's owner passes through pixel (qx, y), so its bounding box contains it, and it is never this
            // border itself (its pixels are all raster-later than its start).  If exactly one other border's box
            // contains the pixel, that border is the owner; only otherwise is the owner found by following it.
            int found = -2;
            {
                int hits = 0, which = -1;
                for (int jb = 0; jb < nr; jb += 64) {
                    int j = jb + lane;
                    bool in = j < nr && j != c && t.box[j][0] <= qx && qx <= t.box[j][2] && t.box[j][1] <= y && y <= t.box[j][3];
                    uint64_t bal = __ballot(in);
                    hits += __popcll(bal);
                    if (bal && which < 0) which = jb + __ffsll((long long)bal) - 1;
                }
                if (hits == 1) found = which;
            }
            if (DEFER && found == -2 && a.defer_links) {
                // split form: the walk joins the batch's second packed follow pass (one lane there, not a whole wave here)
                int slot = 0;
                if (lane == 0) slot = atomicAdd(&n_open, 1);
                slot = uni(slot);
                if (slot < MAXA) {
                    if (lane == 0) { open_link[slot] = walk_entry(image, qx, y, r_is_hole ? 2 : 3, c); b.link[c] = -2; }
                    continue;
                }
            }
            if (found == -2) {
                Trace T; // every lane walks the same border (uniform arguments): rare path
                follow(M, qx, y, r_is_hole ? 4 : 0, -1, -1, a.max_steps, T, diag_len);
                if (T.status) { if (lane == 0) atomicMax(&err, 1); continue; }
                int lkey, ltype;
                link_identity(T.a00, T.min_fg, T.min_ebg, lkey, ltype);
                for (int jb = 0; jb < nr; jb += 64) {
                    int j = jb + lane;
                    bool hit = j < nr && b.key[j] == lkey && b.hole[j] == ltype;
                    uint64_t bal = __ballot(hit);
                    if (bal) { found = jb + __ffsll((long long)bal) - 1; break; }
                }
            }
            if (lane == 0) {
                if (found == -2) atomicMax(&err, 2);
                b.link[c] = (int16_t)found;
            }
        }
        __syncthreads();
    }

    // Tree kernel, first pass, an image with open links: they join the batch's link list, the image the wait list, the links found so
    // far go to the workspace for the second pass.  `lbase` is one LDS word.  Ends without a barrier: the second tree pass finishes the image.
    __device__ __forceinline__ void hand_over_links(int nr, const uint64_t* open_link, int n_open, const Borders& b, uint32_t& lbase) const
    {
        const int na = n_open < MAXA ? n_open : MAXA;
        if (tid == 0) {
            lbase = atomicAdd(&a.walk_count[2], (uint32_t)na); work.st_pending = na;
            a.wait_list[atomicAdd(&a.walk_count[4], 1u)] = (uint32_t)image; // the second tree pass runs over this list
        }
        __syncthreads();
        for (int i = tid; i < na; i += NTHREADS) a.link_list[lbase + (uint32_t)i] = open_link[i];
        for (int c = tid; c < nr; c += NTHREADS) work.rlink[c] = b.link[c];
    }

    // ---- phase C2: parents (Suzuki's table: same kind -> the link's parent, else the link itself) -----------
    // Leaves b.parent of every border, the kept ones in t.kept_idx / t.kept_depth (n_kept may pass MAXK, the arrays do not) and their
    // ancestor paths, root first, in work.kept_path; err = 3 where a kept border lies deeper than MAXD.
    __device__ __forceinline__ void resolve_parents_and_keep(int nr, int& n_kept, int& err, Borders& b, Tree& t) const
    {
        for (int c = tid; c < nr; c += NTHREADS) {
            if (b.res[c]) continue;
            int me = b.hole[c], j = b.link[c], guard = 0;
            while (j >= 0 && b.hole[j] == me && guard++ < MAXR) {
                if (b.res[j]) { j = b.parent[j]; break; } // a border of my kind whose parent the boxes gave: its parent is mine
                j = b.link[j];
            }
            b.parent[c] = (int16_t)j;
        }
        __syncthreads();
        for (int c = tid; c < nr; c += NTHREADS) {
            if (!b.kept[c]) continue;
            int slot = atomicAdd(&n_kept, 1);
            if (slot >= MAXK) continue;
            t.kept_idx[slot] = (int16_t)c;
            int chain[MAXD], d = 0, j = c;
            while (j >= 0 && d < MAXD) { chain[d++] = b.key[j]; j = b.parent[j]; }
            if (j >= 0) { atomicMax(&err, 3); d = MAXD; }
            t.kept_depth[slot] = (int8_t)d;
            for (int i = 0; i < d; i++) work.kept_path[slot][i] = chain[d - 1 - i]; // root first
        }
        __syncthreads();
    }

    // ---- phase C3: position in the pre-order walk with siblings in reverse discovery order -------------------
    // Writes the centroids in output order, the count, each kept record's order and -- for a caller that asked -- every record with its
    // link and parent.  The image's last phase: no barrier at its end.
    __device__ __forceinline__ void order_and_emit(int nr, int n_kept, const Borders& b, const Tree& t) const
    {
        for (int c = tid; c < n_kept; c += NTHREADS) {
            int rank = 0, da = t.kept_depth[c];
            for (int o = 0; o < n_kept; o++) {
                if (o == c) continue;
                int db = t.kept_depth[o], l = 0;
                while (l < da && l < db && work.kept_path[c][l] == work.kept_path[o][l]) l++;
                bool other_first;
                if (l == db) other_first = true;        // the other one is my ancestor
                else if (l == da) other_first = false;  // I am its ancestor
                else other_first = work.kept_path[o][l] > work.kept_path[c][l]; // later discovery comes first
                rank += other_first;
            }
            ContourRec& r = work.recs[t.kept_idx[c]];
            r.order = rank;
            if (rank < a.max_blobs) {
                int32_t* o = a.out_xy + (size_t)image * a.xy_stride + (size_t)rank * 2;
                o[0] = r.cx; o[1] = r.cy;
            }
        }
        if (tid == 0) *out_count = n_kept;
        stamp(4);
        if (a.dbg) {
            __syncthreads(); // the records' order fields are written by other threads just above
            for (int c = tid; c < nr && c < a.dbg_cap; c += NTHREADS) {
                ContourRec r = work.recs[c];
                r.link = b.link[c]; r.parent = b.parent[c];
                a.dbg[(size_t)image * a.dbg_cap + c] = r;
            }
            if (tid == 0) a.dbg_count[image] = nr;
        }
    }
};

// MODE 0: the whole job for one image (candidates, walks, tree).  MODE 1 / MODE 2: the first and the last part of the split
// form -- candidates only (handed to contour_follow_kernel through the workspace and the batch-wide walk list) / tree only
// (from the records that kernel left).  An image that ends early -- with an error code, handed over, or waiting for its link
// walks -- ends here, by a return between two phases.
template <int MODE>
__device__ __forceinline__ void contours_body(const ContourArgs& a, const int image)
{
    __shared__ int n_cell, n_cand, n_rec, n_kept, err, dbg_steps;
    __shared__ uint32_t cand[MAXC];
    __shared__ TreeOrCells scratch; // (the compiler lays LDS out by the variables' names: under this one the one-kernel form keeps its 90 VGPRs, under others it takes 91)
    __shared__ RangesOrWindows ranges_or_windows;
    __shared__ Borders b;
    __shared__ uint64_t open_link[MAXA]; // MODE 2, first pass: the links left to the second follow pass, n_open of them (the first MAXA are kept)
    __shared__ int n_open;
    __shared__ double diag_len[64]; // float32 length of a diagonal run of k steps, as a double
    __shared__ uint32_t list_base;  // where this image's entries start in the batch's walk list (MODE 1) / link list (MODE 2)
    Tree& t = scratch.tree;

    if (a.prio == 1) __builtin_amdgcn_s_setprio(1);
    else if (a.prio == 2) __builtin_amdgcn_s_setprio(2);
    else if (a.prio == 3) __builtin_amdgcn_s_setprio(3);
    const int tid = threadIdx.x;
    const ImageJob job{a, image,
                       Mask{a.mask + (size_t)image * mask_image_words(a.H, a.words_per_row), a.words_per_row, a.H, a.W, a.W + 1},
                       ((ContourWork*)a.work)[image], a.out_count + (size_t)image * a.count_stride,
                       a.timing ? a.timing + (size_t)image * 8 : nullptr, tid, tid & 63, uni(tid >> 6)};
    if (tid == 0) { n_cand = 0; n_rec = 0; n_kept = 0; err = 0; n_cell = 0; dbg_steps = 0; }
    if (tid < 64) diag_len[tid] = run_length(1, tid);
    job.stamp(0);
    __syncthreads();
    const bool second_pass = MODE == 2 && a.tree_pass == 2;

    if constexpr (MODE == 2) {
        if (job.work.st_ncand < 0) return; // the candidates kernel has reported this image's error
        if (second_pass && job.work.st_pending <= 0) return; // finished by the first pass
        if (!job.load_follow_records(second_pass, n_rec, err, n_open, b, t)) {
            job.fail_image(err ? BLOB_ERR_STEPS : BLOB_ERR_CONTOURS);
            return;
        }
    } else {
        const uint32_t* cells = a.cells ? a.cells + (size_t)image * a.n_chunks * a.n_strips : nullptr;
        const uint32_t* boxes = (a.cells && a.boxes) ? a.boxes + (size_t)image * a.n_chunks * a.n_strips * 4 : nullptr;
        if (cells) job.list_cells(cells, boxes, n_cell, scratch.cell_list, ranges_or_windows.cell_rng);
        job.scan_cells(cells, n_cell, scratch.cell_list, ranges_or_windows.cell_rng, n_cand, cand);
        job.stamp(1);
        if (n_cand > MAXC) {
            job.fail_image(BLOB_ERR_CANDIDATES);
            if (MODE == 1 && tid == 0) job.work.st_ncand = -1;
            return;
        }
    }
    if constexpr (MODE == 1) {
        job.hand_over_candidates(n_cand, cand, list_base);
        return;
    }
    if constexpr (MODE == 0) {
        job.walk_candidates(n_cand, cand, ranges_or_windows.win, diag_len, n_rec, err, dbg_steps, b, t);
        job.stamp(2);
        if (job.tick && tid == 0) { job.tick[5] = (uint64_t)n_cand; job.tick[6] = (uint64_t)dbg_steps; job.tick[7] = (uint64_t)n_rec; }
        if (n_rec > MAXR || err) {
            job.fail_image(err ? BLOB_ERR_STEPS : BLOB_ERR_CONTOURS);
            return;
        }
    }
    if constexpr (MODE != 1) {
        const int nr = n_rec;
        job.parents_from_boxes(nr, b, t);
        job.template find_links<MODE == 2>(nr, second_pass, err, open_link, n_open, b, t, diag_len);
        job.stamp(3);
        if (err) {
            job.fail_image(err == 1 ? BLOB_ERR_STEPS : BLOB_ERR_CONTOURS);
            return;
        }
        if constexpr (MODE == 2) {
            if (!second_pass && n_open > 0) { // this image is finished by the second tree pass
                job.hand_over_links(nr, open_link, n_open, b, list_base);
                return;
            }
        }
        job.resolve_parents_and_keep(nr, n_kept, err, b, t);
        if (err || n_kept > MAXK) {
            job.fail_image(err ? BLOB_ERR_DEPTH : BLOB_ERR_CONTOURS);
            return;
        }
        job.order_and_emit(nr, n_kept, b, t);
    }
}

// One workgroup per image.  The second tree pass runs over the list of the images that wait for link walks (mostly none: its
// workgroups read one counter and leave).  (The kernels as loops over the images, fewer workgroups than images: 19 more registers for
// the candidates kernel, 42 for the tree kernel, 8 us slower each, nothing gained in the pipeline -- profiles/README.md.)
// LOOP: a fixed grid (a few workgroups per CU) works through the images -- workgroup b takes b, b + grid, ... -- instead of one
// workgroup per image.  Alone that is a few microseconds slower (more registers), but beside another batch's streaming scan, which
// holds every wave slot of the chip, each of 3072 four-wave workgroups has to wait for a place of its own: the tree kernel, 12 us
// alone, took 0.34-0.60 ms there, the candidates kernel 0.27-0.52 instead of 0.08 (profiles/history/r4_timeline_depth3.txt).
template <int MODE, bool LOOP>
__global__ __launch_bounds__(NTHREADS) void contours_kernel(ContourArgs a)
{
    if (MODE == 2 && a.tree_pass == 2) { // the images that waited for link walks (mostly none): a small grid over their list
        const uint32_t n = a.walk_count[4];
        for (uint32_t e = blockIdx.x; e < n; e += gridDim.x) {
            contours_body<MODE>(a, uni((int)a.wait_list[e]));
            __syncthreads(); // (the next image reuses the workgroup's LDS)
        }
        return;
    }
    if (!LOOP) {
        contours_body<MODE>(a, blockIdx.x);
        return;
    }
    for (int image = blockIdx.x; image < a.n_images; image += gridDim.x) {
        contours_body<MODE>(a, image);
        __syncthreads();
    }
}

size_t contour_work_bytes() { return sizeof(ContourWork); }
size_t contour_walk_bytes() { return sizeof(uint64_t) * MAXC; }  // candidates of one image in the batch's walk list
size_t contour_link_bytes() { return sizeof(uint64_t) * MAXA; }  // links of one image handed to the second follow pass

// Five launches per batch: contours_kernel<1> = the candidates kernel (one workgroup of 4 waves per image, or a fixed grid looping) -> contour_follow_kernel (persistent
// waves, every walk of the batch whatever image it belongs to) -> contours_kernel<2> (tree and output, one workgroup per image;
// images with an ambiguous link wait) -> contour_follow_kernel (the link walks) -> contours_kernel<2> (the images that waited);
// the hand-over is the per-image global workspace (L2) and the two batch-wide walk lists.  contours_kernel<0> is the same work
// as one kernel per image with the lone-lane walker `follow` above (contours_split = 0, and whenever contour_timing is on).
void launch_contours(const ContourArgs& a_, hipStream_t s)
{
    if (a_.walk_list && !a_.timing && a_.n_images < MAX_SPLIT_IMAGES) {
        // candidates per image -> every walk of the batch -> tree per image; the (few) links whose owner only a walk can tell go
        // through a second, equally packed, follow pass, and the second tree pass finishes the images that waited for them
        ContourArgs a = a_;
        if (!a.counters_zeroed) (void)hipMemsetAsync(a.walk_count, 0, 8 * sizeof(uint32_t), s);
        const bool loop = a.image_grid > 0 && a.image_grid < a.n_images;
        const int pass2_grid = a.n_images < 64 ? a.n_images : 64;
        if (loop) hipLaunchKernelGGL((contours_kernel<1, true>), dim3(a.image_grid), dim3(NTHREADS), 0, s, a);
        else hipLaunchKernelGGL((contours_kernel<1, false>), dim3(a.n_images), dim3(NTHREADS), 0, s, a);
        a.follow_list = 0;
        launch_contour_follow(a, a.follow_grid, s);
        a.tree_pass = 1;
        if (loop) hipLaunchKernelGGL((contours_kernel<2, true>), dim3(a.image_grid), dim3(NTHREADS), 0, s, a);
        else hipLaunchKernelGGL((contours_kernel<2, false>), dim3(a.n_images), dim3(NTHREADS), 0, s, a);
        if (!a.defer_links) return; // every link was settled in the first tree pass (walked in place where the boxes did not decide)
        a.follow_list = 1;
        launch_contour_follow(a, a.follow_grid2, s);
        a.tree_pass = 2;
        hipLaunchKernelGGL((contours_kernel<2, false>), dim3(pass2_grid), dim3(NTHREADS), 0, s, a);
        return;
    }
    hipLaunchKernelGGL((contours_kernel<0, false>), dim3(a_.n_images), dim3(NTHREADS), 0, s, a_);
}

} // namespace mocap
