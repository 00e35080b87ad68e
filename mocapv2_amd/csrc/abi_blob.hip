// abi_blob.hip -- C-ABI host file: the blob stage of a batch (run_filter and its steps, run_contours, the mask and contour
// groups), its entry points, and the single-image utilities that share its helpers.
#include "ctx.h"

static_assert(sizeof(mocap_contour) == sizeof(ContourRec), "debug record layout");

// scan_serial: the scans of all contexts of a device form one chain (each waits for the completion event of the one launched
// before it), so that two batches' scans never share the chip -- a scan alone saturates HBM, two at once only delay each other
struct ScanTurn { std::mutex mu; hipEvent_t done = nullptr; bool have = false; };
static ScanTurn g_scan_turn[64];

extern "C" {

// ---- blob stage ------------------------------------------------------------------------------------------------
static int check_frames(mocap_ctx* c, const void* frames, int n_images, int cam_mod, int slot_base, size_t image_stride, int pitch)
{
    if (!c || !frames) return fail(MOCAP_E_INVALID, "null argument");
    if (n_images < 1) return fail(MOCAP_E_INVALID, "n_images = %d", n_images);
    if (cam_mod < 1 || slot_base < 0 || slot_base + cam_mod > c->n_slots)
        return fail(MOCAP_E_INVALID, "slots %d..%d not in 0..%d", slot_base, slot_base + cam_mod - 1, c->n_slots - 1);
    if (pitch < c->W) return fail(MOCAP_E_INVALID, "pitch %d < width %d", pitch, c->W);
    if (n_images > 1 && image_stride < (size_t)pitch * (c->H - 1) + c->W) return fail(MOCAP_E_INVALID, "image_stride too small");
    for (int s = slot_base; s < slot_base + cam_mod; s++)
        if (c->slot_state[s] == 0) return fail(MOCAP_E_STATE, "mocap_set_undistort was not called for slot %d", s);
    return 0;
}


// Excess base of the scan (BrightArgs::base): pixels count with max(0, p - c).  Exact for any c below the threshold; a
// higher c ignores brighter backgrounds, a lower c lets a cell hold more bright pixels before it is "hot" (tighter boxes
// around the markers).  Two candidates derived from the threshold -- for the reference's 216.75: 63 (tight; a dark IR
// frame) and 150 (backgrounds up to ~150 cost nothing) -- between which the context switches by itself: on its first batch
// and every 32nd one after it the scan also counts the cells that are hot under the other base (on every 16th image); the
// tight one is used whenever it does not leave noticeably more hot cells.  A context starts with the tolerant base (a
// bright scene filtered with the tight one would cost a dense pass).  MOCAP_EXCESS_BASE=c pins the base (A/B switch).
static int excess_base(int thr_mul, int sel)
{
    int c = sel ? thr_mul - 67 : thr_mul - 154;
    if (c > thr_mul - 1) c = thr_mul - 1;
    if (c > 254) c = 254;
    return c < 0 ? 0 : c;
}

static int ensure_gray_scratch(mocap_ctx* c, size_t bytes)
{
    if (bytes <= c->gray_scratch.n) return 0;
    std::lock_guard<std::mutex> lk(c->mu);
    return c->gray_scratch.reserve(bytes);
}

// floor(thresh) + 1: blurred > thresh  <=>  S >= thr_mul * taps
static int threshold_mul(const mocap_ctx* c)
{
    const double ft = floor(c->prm.thresh);
    return ft < -1.0 ? 0 : (ft > 255.0 ? 256 : (int)ft + 1);
}

// The row pipeline's arguments for a batch on the undistort slots from slot_base on (slot_base < 0: no tables): every member defined;
// geometry, tiling, the first slot's tables.  The callers add what differs (the tile list, the staged form, test switches).
static FilterArgs filter_args(const mocap_ctx* c, const void* src, size_t image_stride, int pitch, uint32_t* mask, uint32_t* cells,
                              int slot_base, int cam_mod, int n_images, int thr_mul)
{
    const Tiling tl = tiling(c);
    FilterArgs a{};
    a.src = (const uint8_t*)src; a.image_stride = image_stride; a.pitch = pitch; a.H = c->H; a.W = c->W;
    a.mask = mask; a.words_per_row = c->wpr; a.cam_mod = cam_mod; a.cells = cells;
    a.n_images = n_images; a.n_steps = (n_images + cam_mod - 1) / cam_mod;
    a.thr_mul = thr_mul;
    a.n_strips = tl.n_strips; a.rows_per_chunk = tl.rows; a.n_cgroups = tl.n_cgroups;
    a.pipelined = c->W >= 4 && (c->W & 3) == 0 && c->H >= 2;
    if (slot_base >= 0) {
        a.map = slot_map(c, slot_base); a.mapw = slot_mapw(c, slot_base); a.map4 = slot_map4(c, slot_base);
        a.rowbox = c->rowbox ? c->rowbox + (size_t)slot_base * c->H * tl.n_strips : nullptr;
    }
    return a;
}

// ---- run_filter and its steps, in the order they run ------------------------------------------------------------
// one call's batch, as the steps hand it on
struct Batch {
    int n_images, cam_mod, slot_base;
    size_t image_stride; int pitch;
    uint32_t* mask; uint32_t* cells;
    bool own_mask;       // the context's mask keeps "zero outside the recorded regions" from batch to batch
    hipStream_t s;
};

// the last probe's counts have arrived: which excess base the next scans use (base_sel), who marks the tiles (hot_dense)
static void read_probe(mocap_ctx* c, int thr_mul)
{
    if (!c->probe_pending || hipEventQuery(c->probe_ev) != hipSuccess) return;
    unsigned long long n_cur = 0, n_alt = 0;
    for (int i = 0; i < 128; i++) { n_cur += c->probe_host[PROBE_STRIDE * i]; n_alt += c->probe_host[PROBE_STRIDE * i + 1]; }
    if (c->tune.probe_debug) fprintf(stderr, "[probe] base %d: %llu hot cells, alternative %d: %llu\n", excess_base(thr_mul, c->base_sel), n_cur, excess_base(thr_mul, c->base_sel ^ 1), n_alt);
    // The tight base (sel 0) leaves tighter boxes around the markers for the same number of hot cells (measured: 33k against
    // 45k marked tiles per 3072 images of the benchmark scene), so it is preferred unless the background makes its hot cells
    // explode: use it iff it leaves at most 1.25x the hot cells of the tolerant base.
    const unsigned long long n_lo = c->base_sel == 0 ? n_cur : n_alt, n_hi = c->base_sel == 0 ? n_alt : n_cur;
    c->base_sel = (n_lo * 4 <= n_hi * 5) ? 0 : 1;
    // Who marks the tiles (scan_hotmap = 1: whichever is cheaper).  A hot cell costs the scan two dependent round trips behind
    // its loads; the hot map moves them into mark_tiles_kernel, which costs ~0.04 ms per 3072 images whatever the scene holds.
    // Measured (profiles/history/r4_run7_scan_wide_serial.log): scan + mark + settle 1.03 against 1.00 ms at 8 markers per frame
    // (~190 hot cells per image), 1.07 against 1.21 at 32 (~750): the map pays above a few hundred hot cells per image.
    const unsigned long long n_now = c->base_sel == 0 ? n_lo : n_hi;
    c->hot_dense = c->probe_images > 0 && n_now > 400ull * (unsigned long long)c->probe_images;
    c->probe_pending = false;
}

// dark-tile early-out: largest doubled excess sum 2E (E = sum of max(0, p - base)) per 16x16 block that still proves an
// all-zero mask:   2E * Wmax < 1024 * taps_min * (2 * thr_mul - 2 * base - 1)     (derivation: blob_scan.hip)
struct ScanBounds {
    int thr_mul;
    int fixed_base;      // >= 0: the pinned base (excess_base switch)
    int base, base_alt;  // the excess base in use / the one a probe counts beside it
    int allow, allow_cut1, allow_cut2, allow_alt; // -1 = no early-out
};
static ScanBounds scan_bounds(const mocap_ctx* c, int slot_base, int cam_mod, int thr_mul)
{
    ScanBounds b{thr_mul, c->tune.excess_base, 0, 0, -1, -1, -1, -1};
    if (b.fixed_base >= 0) { if (b.fixed_base > thr_mul - 1) b.fixed_base = thr_mul - 1; if (b.fixed_base > 254) b.fixed_base = 254; if (b.fixed_base < 0) b.fixed_base = 0; }
    b.base = b.fixed_base >= 0 ? b.fixed_base : excess_base(thr_mul, c->base_sel);
    b.base_alt = excess_base(thr_mul, c->base_sel ^ 1);
    long long wmax = 0;
    bool ok = true;
    for (int sl = slot_base; sl < slot_base + cam_mod; sl++) {
        if (c->slot_wmax[sl] == 0) ok = false;
        wmax = c->slot_wmax[sl] > wmax ? c->slot_wmax[sl] : wmax;
    }
    auto t5 = [](int n) { return (n - 1 < 2 ? n - 1 : 2) + 1; }; // taps of a window at the border, per axis
    auto t5full = [](int n) { return n < 5 ? n : 5; };
    const long long per_tap = 1024LL * (2LL * thr_mul - 2LL * b.base - 1), per_tap_alt = 1024LL * (2LL * thr_mul - 2LL * b.base_alt - 1);
    if (!c->tile_rows || !c->reach || !c->cflags) ok = false;
    if (ok && wmax > 0 && per_tap > 0) {
        b.allow = (int)((per_tap * t5full(c->W) * t5full(c->H) - 1) / wmax); // windows with all their taps
        const long long taps1 = t5(c->W) * t5full(c->H) < t5full(c->W) * t5(c->H) ? t5(c->W) * t5full(c->H) : t5full(c->W) * t5(c->H);
        b.allow_cut1 = (int)((per_tap * taps1 - 1) / wmax);                  // smallest window cut in one axis
        b.allow_cut2 = (int)((per_tap * t5(c->W) * t5(c->H) - 1) / wmax);    // smallest window cut in both
        if (per_tap_alt > 0) b.allow_alt = (int)((per_tap_alt * t5full(c->W) * t5full(c->H) - 1) / wmax);
    }
    if (!c->tune.skip_dark) b.allow = -1;
    return b;
}

// Which kernels serve the batch.
// bayer != nullptr: the frames (= bayer->dst) do not exist yet -- the Bayer -> gray pass that writes them runs first, fused
// with the streaming scan where the geometry allows (it has the gray bytes in registers anyway).
// bayer->dst == nullptr (no gray buffer): the gray-less path where it can run -- the fused scan without its write-back, every
// marked tile as items of the box kernel's Bayer form, which forms the gray values it reads from the Bayer frames (no wide tiles:
// the row pipeline has no Bayer form) --, else the gray frames go to the context's scratch buffer and the path above runs.
struct FilterPath {
    bool remap;          // a slot of the batch is remapped
    bool compact;        // the sparse path: scan, settle, box kernel (+ wide tiles); else the dense kernel
    bool rows_staged;    // the row pipeline's staged form (compact table, source pixels through LDS): dense path and wide tiles alike
    bool direct;         // the gray-less path
    bool bayer;          // a Bayer -> gray pass belongs to the batch: `bl`
    uint64_t remap_bits;
    int rows_dw;
    const void* frames;  // what the filter kernels read: gray frames (the caller's, or the scratch buffer), or the Bayer frames (direct)
    BayerArgs bl;
};
static int choose_path(mocap_ctx* c, const Batch& bt, const void* frames, const BayerArgs* bayer, int allow, FilterPath& p)
{
    p = FilterPath{};
    p.compact = c->W >= 8 && bt.cam_mod <= 64;
    for (int sl = bt.slot_base; sl < bt.slot_base + bt.cam_mod; sl++) {
        if (c->slot_state[sl] == 2) { p.remap = true; if (sl - bt.slot_base < 64) p.remap_bits |= 1ull << (sl - bt.slot_base); }
        if (c->slot_state[sl] == 2 && !c->slot_compact[sl]) p.compact = false;
    }
    if (c->tune.general_filter) p.compact = false; // test switch: the general kernel
    p.rows_staged = p.remap && c->tune.rows_staged && c->map4 && c->rowbox && (c->W & 15) == 0 && c->H >= 2; // (16-byte staging units)
    for (int sl = bt.slot_base; sl < bt.slot_base + bt.cam_mod; sl++)
        if (!c->slot_compact[sl]) p.rows_staged = false;
    p.rows_dw = c->tune.rows_stage_dw < 0 || c->tune.rows_stage_dw > rows_stage_dwords() ? rows_stage_dwords() : c->tune.rows_stage_dw;
    // every tile has to be filtered anyway: the dense kernel's sliding row pipeline does that with less work per pixel
    // than the box kernel (MOCAP_DENSE_BOXES=1: the box kernel on whole tiles, a test switch)
    if (allow < 0 && !c->tune.dense_boxes) p.compact = false;
    p.frames = frames;
    p.bayer = bayer != nullptr;
    if (bayer) p.bl = *bayer;
    if (bayer && !bayer->dst) {
        p.direct = p.compact && allow >= 0 && bt.own_mask && bayer_scan_direct(p.bl);
        if (!p.direct) { // the dense path, W % 16 or H % 8 not 0, unaligned frames, MOCAP_SKIP_DARK=0 / MOCAP_GENERAL_FILTER=1
            const size_t bytes = (size_t)(bt.n_images - 1) * bt.image_stride + (size_t)(c->H - 1) * bt.pitch + c->W;
            TRY(ensure_gray_scratch(c, bytes));
            p.bl.dst = c->gray_scratch;
        }
        p.frames = p.direct ? (const void*)p.bl.src : (const void*)p.bl.dst;
    }
    return 0;
}

// general dense kernel (tiny images, tables beyond the compact format): every tile, every mask byte
static int filter_dense(mocap_ctx* c, const Batch& bt, const FilterPath& p, int thr_mul)
{
    FilterArgs a = filter_args(c, p.frames, bt.image_stride, bt.pitch, bt.mask, bt.cells, bt.slot_base, bt.cam_mod, bt.n_images, thr_mul);
    if (!c->tune.remap_pipeline) a.pipelined = 0; // test switch: the per-pixel gather
    a.staged = p.rows_staged; a.stage_dw = p.rows_dw;
    if (p.bayer) { launch_bayer_gray(p.bl, bt.s); HIP_TRY(hipGetLastError()); }
    if (bt.own_mask) c->mask_dirty = true;
    HIP_TRY(hipMemsetAsync(c->n_items, 0, 1024, bt.s)); // no work lists: mocap_list_stats reports none (not the previous batch's)
    EvPair ev; bool on;
    prof_begin(c, bt.s, ev, on);
    launch_filter_mask(a, p.remap, bt.s);
    prof_end(c, PROF_FILTER, bt.s, ev, on);
    HIP_TRY(hipGetLastError());
    return 0;
}

// what settle and the box kernel get (timing and zero8 are added by their steps)
static BoxArgs box_args(const mocap_ctx* c, const Batch& bt, const FilterPath& p, const ScanBounds& sb)
{
    const Tiling tl = tiling(c);
    BoxArgs a{};
    a.src = (const uint8_t*)p.frames; a.image_stride = bt.image_stride; a.pitch = bt.pitch; a.H = c->H; a.W = c->W;
    a.mask = bt.mask; a.words_per_row = c->wpr; a.cells = bt.cells;
    a.map4 = slot_map4(c, bt.slot_base);
    a.srcbox = c->srcbox ? c->srcbox + (size_t)bt.slot_base * source_cells(c) : nullptr;
    a.remap_bits = p.remap_bits;
    a.cam_mod = bt.cam_mod; a.n_images = bt.n_images; a.n_steps = (bt.n_images + bt.cam_mod - 1) / bt.cam_mod;
    a.thr_mul = sb.thr_mul;
    a.rows_per_chunk = tl.rows; a.n_strips = tl.n_strips; a.n_chunks = tl.n_cgroups * 4;
    const size_t tr_words = c->mask_images * cells_per_image(c) * 4;
    a.tile_rows = c->tile_rows + (c->tile_rows_flip ? tr_words : 0);
    a.tile_rows_next = c->tile_rows + (c->tile_rows_flip ? 0 : tr_words);
    a.n_clear = c->tile_rows_hold[c->tile_rows_flip ^ 1];
    a.wide_split = c->tune.wide_split == 2 || (c->tune.wide_split == 1 && !c->hot_dense); // (1: sparse scenes only, as scan_hotmap and contour_defer)
    a.cluster = c->tune.cluster;
    a.cur_box = bt.own_mask ? c->cur_box : c->cur_box_ext;
    a.items = c->items; a.n_items = c->n_items; a.cap_items = (uint32_t)c->items.n;
    a.dense = sb.allow < 0;
    // Boxes wider than this many patch quads go through the sliding row pipeline instead (whole tile width, the box's rows):
    // the box kernel's cost grows with the patch area (~30 cycles per quad-row), the row pipeline's with the rows only
    // (~850 cycles per row with the gather).  Measured optimum on the benchmark scenes (8 and 32 markers, both lens models):
    // 38-46 quads; without the routing the 32-marker scene's filter takes 1.77 ms instead of 1.25, the 8-marker scene's
    // 0.53 instead of 0.49.  MOCAP_WIDE_QUADS="remap,identity" overrides (A/B switch; 1000 = never).
    a.wide_tiles = c->wide_tiles; a.cap_wide = (uint32_t)c->wide_tiles.n; a.wide_quads_remap = c->tune.wide_quads_remap; a.wide_quads_identity = c->tune.wide_quads_identity;
    a.wide_bands = c->tune.wide_bands; // measured: 2 / 4 bands 0.50 / 0.55 ms against 0.475 (8 markers), 1.33 / 1.58 against 1.22 (32 markers): the kernel is work-bound
    if (c->W < 4 || p.direct) a.wide_tiles = nullptr;
    a.bayer = p.direct ? p.bl : BayerArgs{}; // (a.src = the Bayer frames)
    a.stage_bytes = c->tune.box_stage_bytes; // test switch
    a.prio = c->tune.box_prio;
    a.ext_mask = bt.own_mask ? 0 : 1;
    return a;
}

// the scan's arguments, without probe and hot map
static BrightArgs bright_args(const mocap_ctx* c, const Batch& bt, const FilterPath& p, const ScanBounds& sb, uint32_t* tile_rows, bool scan_zeroes)
{
    const Tiling tl = tiling(c);
    // floor(i / ncx) = umulhi(i, ceil(2^32 / ncx)) is exact while i * ncx < 2^32
    uint64_t ncx64 = (uint64_t)((c->W + 7) / 8);
    const uint64_t ncells = ncx64 * (uint64_t)((c->H + 7) / 8);
    int wide = (c->W % 16 == 0) && (bt.pitch % 16 == 0) && (bt.image_stride % 16 == 0) && (((uintptr_t)p.frames & 15) == 0) && ncx64 >= 4;
    if (wide && ncells * (ncx64 / 2) >= (1ull << 32)) wide = 0;
    if (!c->tune.scan_wide) wide = 0; // A/B switch
    if (wide) ncx64 /= 2; // the wide kernel divides pair indices by the pairs per cell row
    const uint32_t ncx_magic = (ncx64 > 1 && ncells * ncx64 < (1ull << 32)) ? (uint32_t)(((1ull << 32) + ncx64 - 1) / ncx64) : 0u;
    BrightArgs b{(const uint8_t*)p.frames, bt.image_stride, bt.pitch, c->H, c->W, bt.n_images, bt.cam_mod, ncx_magic, wide, sb.base, sb.allow / 4, sb.allow_cut1 / 4, sb.allow_cut2 / 4,
                 c->reach + (size_t)bt.slot_base * source_cells(c), c->cflags + (size_t)bt.slot_base * source_cells(c),
                 tile_rows, tl.n_cgroups * 4, tl.n_strips, (uint32_t)(((1u << 23) + tl.rows - 1) / tl.rows),
                 bt.mask, bt.own_mask ? 0 : (size_t)bt.n_images * mask_image_words(c->H, c->wpr), ((uintptr_t)bt.mask & 15) == 0, nullptr, sb.base_alt, sb.allow_alt / 4, 0};
    b.prio = c->tune.scan_prio; // A/B switch
    b.max_blocks = c->tune.scan_blocks_per_cu * c->n_cu; b.blocks_x = 0;
    b.zero_counters = scan_zeroes ? c->n_items.p : nullptr;
    b.block_ctr = c->n_items + 160; // (words 160..223 of the counter block zeroed above: one per slice)
    b.slices = c->tune.scan_slices; b.image0 = 0; b.slice_images = bt.n_images;
    return b;
}

// One streaming pass over the frames marks the tiles (and their boxes) that can hold set pixels.  `b` keeps what it ran with,
// for mark_tiles_kernel when that one has to follow (`mark_after_scan`).
static int scan_tiles(mocap_ctx* c, const Batch& bt, const FilterPath& p, const ScanBounds& sb, uint32_t* tile_rows, bool scan_zeroes, BrightArgs& b, bool& mark_after_scan)
{
    const hipStream_t s = bt.s;
    b = bright_args(c, bt, p, sb, tile_rows, scan_zeroes);
    const bool probe = sb.fixed_base < 0 && !c->probe_pending && sb.allow_alt >= 0 && sb.base_alt != sb.base && !p.bayer &&
                       (c->probe_age == 0 || c->probe_age >= 32);
    if (probe) {
        HIP_TRY(hipMemsetAsync(c->probe_dev, 0, PROBE_BYTES, s));
        b.probe = c->probe_dev;
    }
    c->probe_age = probe ? 1 : c->probe_age + 1;
    const bool fused = p.bayer && bt.own_mask && (p.direct || bayer_scan_fusable(p.bl)); // direct: the scan without the gray write-back
    // the streaming scan leaves a hot map (two bits per cell, no table lookups or atomics behind its loads) that
    // mark_tiles_kernel turns into tile boxes; the fused Bayer pass marks the tiles itself (MOCAP_SCAN_HOTMAP=0: so does the scan)
    const bool two_step = !fused && c->hotmap && (c->tune.scan_hotmap == 2 || (c->tune.scan_hotmap == 1 && c->hot_dense));
    if (two_step) { b.hotmap = c->hotmap; b.hot_words = hot_map_words(c->H, c->W, b.wide); b.mark_grid = c->tune.mark_blocks_per_cu * c->n_cu; }
    ScanTurn* turn = c->tune.scan_serial && c->device >= 0 && c->device < 64 ? &g_scan_turn[c->device] : nullptr;
    std::unique_lock<std::mutex> turn_lock; // held from the wait to the record: the chain's order is the lock's order
    if (turn) {
        turn_lock = std::unique_lock<std::mutex>(turn->mu);
        if (!turn->done) HIP_TRY(hipEventCreateWithFlags(&turn->done, hipEventDisableTiming));
        if (turn->have) HIP_TRY(hipStreamWaitEvent(s, turn->done, 0));
    }
    EvPair ev; bool on;
    prof_begin(c, s, ev, on);
    if (fused) launch_bayer_gray_scan(p.bl, b, s);
    else {
        if (p.bayer) launch_bayer_gray(p.bl, s);
        launch_bright_cells(b, s);
    }
    prof_end(c, PROF_SCAN, s, ev, on);
    HIP_TRY(hipGetLastError());
    if (turn) {
        HIP_TRY(hipEventRecord(turn->done, s));
        turn->have = true;
        turn_lock.unlock();
    }
    mark_after_scan = two_step; // (launched with settle, inside its timer: both turn the scan's output into work lists)
    if (probe) {
        HIP_TRY(hipMemcpyAsync(c->probe_host, c->probe_dev, PROBE_BYTES, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipEventRecord(c->probe_ev, s));
        c->probe_pending = true;
        c->probe_images = (bt.n_images + 15) / 16;
    }
    return 0;
}

// the scan's output becomes work lists: mark_tiles_kernel (when the scan left a hot map) and settle_tiles_kernel
static int settle_tiles(mocap_ctx* c, const BoxArgs& a, const BrightArgs& mark_args, bool mark_after_scan, hipStream_t s)
{
    EvPair ev; bool on;
    prof_begin(c, s, ev, on);
    if (mark_after_scan) {
        launch_mark_tiles(mark_args, s);
        HIP_TRY(hipGetLastError());
    }
    launch_settle_tiles(a, s);
    prof_end(c, PROF_SETTLE, s, ev, on);
    HIP_TRY(hipGetLastError());
    if (!a.dense) { // only now: settle (queued) has emptied the array the next batch's scan will widen
        if (a.n_images > c->tile_rows_hold[c->tile_rows_flip]) c->tile_rows_hold[c->tile_rows_flip] = a.n_images;
        c->tile_rows_hold[c->tile_rows_flip ^ 1] = 0;
        c->tile_rows_flip ^= 1;
    }
    return 0;
}

// debugging aid (box_timing): synchronous, prints the mean duration of the box kernel's phases
static int report_box_timing(mocap_ctx* c, const uint64_t* timing, hipStream_t s)
{
    std::vector<uint64_t> t((size_t)6 * c->box_grid);
    HIP_TRY(hipStreamSynchronize(s));
    HIP_TRY(hipMemcpy(t.data(), timing, sizeof(uint64_t) * t.size(), hipMemcpyDeviceToHost));
    double sum[6] = {0, 0, 0, 0, 0, 0}, mx = 0;
    for (int b = 0; b < c->box_grid; b++) {
        double tot = 0;
        for (int i = 0; i < 6; i++) { sum[i] += (double)t[6 * b + i]; if (i < 5) tot += (double)t[6 * b + i]; }
        mx = tot > mx ? tot : mx;
    }
    const double n = sum[5] > 0 ? sum[5] : 1;
    uint32_t cnt[16];
    HIP_TRY(hipMemcpy(cnt, c->n_items, sizeof(cnt), hipMemcpyDeviceToHost));
    fprintf(stderr, "[box] list: %u items, %u wide-tile entries, %u split tiles\n", cnt[0], cnt[8], cnt[SPLIT_COUNTER]);
    fprintf(stderr, "[box] items %.0f (%.1f per wave) | cycles per item: header+wait %.0f, stage %.0f, patch %.0f, threshold %.0f, majority+next %.0f | busiest wave %.0f cycles\n",
            sum[5], sum[5] / c->box_grid, sum[0] / n, sum[1] / n, sum[2] / n, sum[3] / n, sum[4] / n, mx);
    return 0;
}

// the box kernel over the items, and the row pipeline over the list of tiles with wide boxes
static int filter_boxes(mocap_ctx* c, const Batch& bt, const FilterPath& p, BoxArgs& a)
{
    const hipStream_t s = bt.s;
    Buf<uint64_t> timing;
    if (c->tune.box_timing) {
        TRY(timing.reserve((size_t)6 * c->box_grid));
        HIP_TRY(hipMemsetAsync(timing, 0, sizeof(uint64_t) * 6 * c->box_grid, s));
    }
    a.timing = timing;
    EvPair ev; bool on;
    prof_begin(c, s, ev, on);
    // MOCAP_WIDE_FORK=1: the wide-tile kernel on a side stream beside the box kernel (fork / join by events).  Measured: the pair takes
    // 0.53 ms instead of 0.49 alone and the three-batch pipeline 310k instead of 319k frames/s, so it is off.
    const bool fork_wide = c->tune.wide_fork != 0;
    if (a.wide_tiles) { // the tiles with wide boxes: the row pipeline over their list, beside the box kernel (both only read what
                        // settle left and write disjoint tiles): forked onto the context's side stream, joined before the contours
        FilterArgs f = filter_args(c, a.src, bt.image_stride, bt.pitch, bt.mask, bt.cells, bt.slot_base, bt.cam_mod, bt.n_images, a.thr_mul);
        f.tiles = c->wide_tiles; f.n_tiles = c->n_items + 8; f.cap_tiles = a.cap_wide;
        f.staged = p.rows_staged; f.stage_dw = p.rows_dw;
        hipStream_t ws = s;
        if (fork_wide) {
            HIP_TRY(hipEventRecord(c->ev_fork, s));
            if (!c->side) HIP_TRY(hipStreamCreateWithFlags(&c->side, hipStreamNonBlocking));
            HIP_TRY(hipStreamWaitEvent(c->side, c->ev_fork, 0));
            ws = c->side;
        }
        launch_filter_tiles(f, p.remap, c->tune.wide_blocks_per_cu * c->n_cu, ws);
        HIP_TRY(hipGetLastError());
        if (fork_wide) HIP_TRY(hipEventRecord(c->ev_join, c->side));
    }
    launch_box_filter(a, c->box_grid, s, p.direct);
    HIP_TRY(hipGetLastError());
    if (a.wide_tiles && fork_wide) HIP_TRY(hipStreamWaitEvent(s, c->ev_join, 0));
    prof_end(c, PROF_FILTER, s, ev, on);
    return timing ? report_box_timing(c, timing, s) : 0;
}

// Same-stream invariant: two counter blocks are zeroed by kernels of this stage instead of fills of their own -- n_items by the
// scan's first workgroup (scan_zeroes), walk_count by settle_tiles_kernel (zero8) -- and walk_count_zeroed tells run_contours so.
// That holds only while nothing uses n_items between the scan and settle, and while the run_contours that consumes the flag is the
// very next one of this context, on the stream `s` of this call.  A caller that puts the two stages on different streams must
// leave the flag false (run_contours then clears walk_count itself).
static int run_filter(mocap_ctx* c, const void* frames, int n_images, int cam_mod, int slot_base, size_t image_stride,
                      int pitch, uint32_t* mask, uint32_t* cells, hipStream_t s, const BayerArgs* bayer = nullptr)
{
    const Batch bt{n_images, cam_mod, slot_base, image_stride, pitch, mask, cells, mask == c->mask, s};
    c->walk_count_zeroed = false;
    if (cells == c->cells) c->last_images = n_images;
    const int thr_mul = threshold_mul(c);
    read_probe(c, thr_mul);
    const ScanBounds sb = scan_bounds(c, slot_base, cam_mod, thr_mul);
    FilterPath p;
    TRY(choose_path(c, bt, frames, bayer, sb.allow, p));
    if (!p.compact) return filter_dense(c, bt, p, thr_mul);
    if (bt.own_mask && c->mask_dirty) { // the general kernel wrote the whole mask last time: back to "zero outside the regions"
        HIP_TRY(hipMemsetAsync(c->mask, 0, sizeof(uint32_t) * c->mask_images * mask_image_words(c->H, c->wpr), s));
        std::vector<uint32_t> init(c->mask_images * cells_per_image(c) * 4);
        for (size_t i = 0; i < init.size(); i += 4) { init[i] = 1u; init[i + 1] = 1u; init[i + 2] = 1u; init[i + 3] = 1u; }
        HIP_TRY(hipStreamSynchronize(s));
        HIP_TRY(hipMemcpy(c->cur_box, init.data(), sizeof(uint32_t) * init.size(), hipMemcpyHostToDevice));
        c->mask_dirty = false;
    }
    BoxArgs a = box_args(c, bt, p, sb);
    if ((size_t)n_images * cells_per_image(c) * BOX_MAX_PARTS > c->items.n) return fail(MOCAP_E_STATE, "work list smaller than the batch");
    // the counter block (item counts, run heads) must be zero before settle: the scan's first workgroup does that on its way -- a fill
    // launch of its own is one more tiny kernel that waits for a place beside the other batches' kernels -- unless no plain scan runs
    const bool scan_zeroes = !a.dense && !p.bayer && c->tune.scan_blocks_per_cu == 0 && c->tune.scan_slices <= 1;
    if (!scan_zeroes) HIP_TRY(hipMemsetAsync(c->n_items, 0, 1024, s));
    a.zero8 = bt.own_mask ? c->walk_count.p : nullptr; // (the contour stage of this batch follows on the same stream; null before its first batch)
    c->walk_count_zeroed = a.zero8 != nullptr;
    BrightArgs mark_args{}; bool mark_after_scan = false;
    if (!a.dense) TRY(scan_tiles(c, bt, p, sb, a.tile_rows, scan_zeroes, mark_args, mark_after_scan));
    else if (p.bayer) { // no early-out (not provable for this table, or MOCAP_SKIP_DARK=0): the plain gray pass
        launch_bayer_gray(p.bl, s);
        HIP_TRY(hipGetLastError());
    }
    TRY(settle_tiles(c, a, mark_args, mark_after_scan, s));
    return filter_boxes(c, bt, p, a);
}

// the tiles' output regions / scan boxes of the batch just filtered into the context's mask (settle_tiles_kernel), when the
// sparse path ran (the general dense kernel keeps none); MOCAP_CONTOUR_BOXES=0: whole strips (A/B switch, same results)
static const uint32_t* contour_boxes(mocap_ctx* c)
{
    return (c->mask_dirty || !c->tune.contour_boxes) ? nullptr : c->cur_box;
}

// the contour group: workspace per image, the batch's walk lists (in whole 8-byte words), their counters
static int ensure_contour_work(mocap_ctx* c, size_t n_images)
{
    if (n_images <= c->cwork_images) return 0;
    std::lock_guard<std::mutex> lk(c->mu);
    if (n_images <= c->cwork_images) return 0;
    c->cwork_images = 0;
    int rc = c->cwork.reserve(contour_work_bytes() * n_images);
    if (!rc) rc = c->walk_list.reserve((contour_walk_bytes() * n_images + 7) / 8);
    if (!rc) rc = c->link_list.reserve(((contour_link_bytes() + sizeof(uint32_t)) * n_images + 7) / 8); // + the wait list behind it
    if (!rc) rc = c->walk_count.reserve(64);
    if (rc) { c->cwork.release(); c->walk_list.release(); c->link_list.release(); return rc; } // not half a group: the next call starts over
    c->cwork_images = n_images;
    return 0;
}

// debugging aid (follow_timing): synchronous, the follow kernel's phase clock per wave
static int report_follow_timing(const uint64_t* follow_dbg, int follow_grid, hipStream_t s)
{
    std::vector<uint64_t> t((size_t)8 * follow_grid);
    HIP_TRY(hipStreamSynchronize(s));
    HIP_TRY(hipMemcpy(t.data(), follow_dbg, sizeof(uint64_t) * t.size(), hipMemcpyDeviceToHost));
    double sum[8] = {0, 0, 0, 0, 0, 0, 0, 0}, mx[3] = {0, 0, 0}, mxsteps = 0; int used = 0;
    for (int b = 0; b < follow_grid; b++) {
        if (t[8 * b + 5] == 0) continue;
        used++;
        for (int i = 0; i < 8; i++) sum[i] += (double)t[8 * b + i];
        for (int i = 0; i < 3; i++) mx[i] = (double)t[8 * b + i] > mx[i] ? (double)t[8 * b + i] : mx[i];
        mxsteps = (double)t[8 * b + 3] > mxsteps ? (double)t[8 * b + 3] : mxsteps;
    }
    const double u = used ? used : 1;
    fprintf(stderr, "[follow] %d of %d waves had work | per wave (mean / max us): store %.1f / %.1f, refill %.1f / %.1f, walk %.1f / %.1f | wave steps %.0f (max %.0f), "
                    "lanes alive per step %.1f, walks %.1f, refills %.1f | us per wave step %.3f\n",
            used, follow_grid, sum[0] / u / 100, mx[0] / 100, sum[1] / u / 100, mx[1] / 100, sum[2] / u / 100, mx[2] / 100, sum[3] / u, mxsteps,
            sum[3] > 0 ? sum[4] / sum[3] : 0.0, sum[5] / u, sum[6] / u, sum[3] > 0 ? sum[2] / 100 / sum[3] : 0.0);
    return 0;
}

// debugging aid (contour_timing): synchronous, prints the mean duration of the kernel's phases
static int report_contour_timing(const uint64_t* timing, int n_images, hipStream_t s)
{
    std::vector<uint64_t> t((size_t)8 * n_images);
    HIP_TRY(hipStreamSynchronize(s));
    HIP_TRY(hipMemcpy(t.data(), timing, sizeof(uint64_t) * t.size(), hipMemcpyDeviceToHost));
    double sum[4] = {0, 0, 0, 0}, mx = 0; uint64_t lo = ~0ull, hi = 0;
    for (int i = 0; i < n_images; i++) {
        for (int k = 0; k < 4; k++) sum[k] += (double)(t[8 * i + k + 1] - t[8 * i + k]);
        double tot = (double)(t[8 * i + 4] - t[8 * i]); mx = tot > mx ? tot : mx;
        lo = t[8 * i] < lo ? t[8 * i] : lo; hi = t[8 * i + 4] > hi ? t[8 * i + 4] : hi;
    }
    {
        int worst = 0; double wt = 0, sc = 0, ss = 0;
        for (int i = 0; i < n_images; i++) {
            double tot = (double)(t[8 * i + 4] - t[8 * i]);
            if (tot > wt) { wt = tot; worst = i; }
            sc += (double)t[8 * i + 5]; ss += (double)t[8 * i + 6];
        }
        fprintf(stderr, "[contours] slowest image %d: %.1f us, candidates %llu, longest border %llu steps, borders %llu | mean candidates %.1f, mean longest border %.1f steps\n",
                worst, wt / 100, (unsigned long long)t[8 * worst + 5], (unsigned long long)t[8 * worst + 6], (unsigned long long)t[8 * worst + 7],
                sc / n_images, ss / n_images);
    }
    fprintf(stderr, "[contours] mean us per block: candidates %.1f follow %.1f link %.1f order %.1f | slowest block %.1f | first start to last end %.1f\n",
            sum[0] / n_images / 100, sum[1] / n_images / 100, sum[2] / n_images / 100, sum[3] / n_images / 100, mx / 100, (double)(hi - lo) / 100);
    return 0;
}

// counters_zeroed relies on run_filter's same-stream invariant (see there): it is taken only for the context's own mask, from the
// filter stage just queued on `s`, and the flag is used up here.  mocap_contours_from_mask (mask != c->mask) always gets the fill.
static int run_contours(mocap_ctx* c, const uint32_t* mask, const uint32_t* cells, const uint32_t* boxes, int n_images, int32_t* out_xy, long xy_stride,
                        int32_t* out_count, long count_stride, int max_blobs, mocap_contour* dbg, int32_t* dbg_count, int dbg_cap, hipStream_t s)
{
    ContourArgs a;
    a.mask = mask; a.words_per_row = c->wpr; a.H = c->H; a.W = c->W; a.n_images = n_images;
    a.out_xy = out_xy; a.out_count = out_count; a.max_blobs = max_blobs;
    a.xy_stride = xy_stride; a.count_stride = count_stride;
    a.min_area = c->prm.min_area; a.min_circ = c->prm.min_circ;
    a.dbg = (ContourRec*)dbg; a.dbg_count = dbg_count; a.dbg_cap = dbg_cap;
    long long ms = 4LL * c->H * c->W + 16;
    a.max_steps = ms > (1 << 22) ? (1 << 22) : (int)ms;
    Tiling tl = tiling(c);
    a.cells = cells; a.boxes = boxes; a.rows_per_chunk = tl.rows; a.n_chunks = tl.n_cgroups * 4; a.n_strips = tl.n_strips;
    if ((long long)a.n_chunks * a.n_strips * ((tl.rows + 7) / 8) > 65535 || c->wpr > 4096) a.cells = nullptr; // cell ids are 16-bit, first words 12-bit in the kernel: scan every row instead
    TRY(ensure_contour_work(c, n_images));
    a.work = c->cwork;
    // The split form (candidates per image -> all walks of the batch, 64 to a wave -> tree per image) is the default;
    // MOCAP_CONTOURS_SPLIT=0 runs the one-kernel-per-image form (A/B switch; same results).
    const bool split = c->tune.contours_split != 0;
    a.walk_list = split ? c->walk_list : nullptr; a.link_list = c->link_list; a.walk_count = c->walk_count;
    a.follow_grid = c->n_cu * 4;  // 4 one-wave workgroups per CU (33 KB of LDS each): persistent, they refill their lanes from the list
    a.follow_grid2 = c->n_cu;     // the link walks are few
    a.image_grid = c->tune.contour_blocks_per_cu * c->n_cu;
    a.counters_zeroed = mask == c->mask && c->walk_count_zeroed; // (settle of this batch, same stream)
    c->walk_count_zeroed = false;
    // Links that only a walk can settle (nested rings, overlapping boxes): deferred to a second, packed follow pass + a second tree pass
    // -- two more launches per batch, nearly always empty on frames of separate markers, and beside another batch's scan an empty
    // launch costs up to 0.3 ms (profiles/history/r4_timeline_depth3.txt) -- or walked in place by the first tree pass (one wave per
    // link: 0.1-0.2 ms when a crowded batch holds a long one).  contour_defer = 1: deferred only once a probe found the scene crowded.
    a.defer_links = c->tune.contour_defer == 2 || (c->tune.contour_defer == 1 && c->hot_dense);
    a.wait_list = (uint32_t*)((uint8_t*)c->link_list.p + contour_link_bytes() * c->cwork_images);
    a.follow_list = 0; a.tree_pass = 0; a.follow_dbg_list = c->tune.follow_timing == 2 ? 1 : 0;
    Buf<uint64_t> follow_dbg, timing; // debugging aids: synchronous
    if (c->tune.follow_timing && split) {
        TRY(follow_dbg.reserve((size_t)8 * a.follow_grid));
        HIP_TRY(hipMemsetAsync(follow_dbg, 0, sizeof(uint64_t) * 8 * a.follow_grid, s));
    }
    a.follow_dbg = follow_dbg;
    a.prio = c->tune.contour_prio; // A/B switch (no effect measured)
    if (c->tune.contour_timing) {
        TRY(timing.reserve((size_t)8 * n_images));
        HIP_TRY(hipMemsetAsync(timing, 0, sizeof(uint64_t) * 8 * n_images, s));
    }
    a.timing = timing;
    EvPair p; bool on;
    prof_begin(c, s, p, on);
    launch_contours(a, s);
    prof_end(c, PROF_CONTOURS, s, p, on);
    HIP_TRY(hipGetLastError());
    if (follow_dbg) TRY(report_follow_timing(follow_dbg, a.follow_grid, s));
    if (timing) TRY(report_contour_timing(timing, n_images, s));
    return 0;
}

// The mask group (what the context's own mask needs: occupancy cells, tile boxes, hot map, work lists) for n_images images.
static int grow_mask_group(mocap_ctx* c, size_t n_images)
{
    const size_t tiles = n_images * cells_per_image(c);
    TRY(c->mask.reserve(n_images * mask_image_words(c->H, c->wpr), true));
    TRY(c->cells.reserve(tiles, true));
    // every tile starts with the empty record (0xffffffff, 0, 0, 0) and an empty recorded region (x0 = 1 > x1 = 0)
    std::vector<uint32_t> init(tiles * 4, 0u);
    for (size_t i = 0; i < init.size(); i += 4) init[i] = 0xffffffffu;
    TRY(c->tile_rows.reserve(2 * init.size()));
    HIP_TRY(hipMemcpy(c->tile_rows, init.data(), sizeof(uint32_t) * init.size(), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(c->tile_rows + init.size(), init.data(), sizeof(uint32_t) * init.size(), hipMemcpyHostToDevice));
    // the hot map, sized for either scan form
    const int hw0 = hot_map_words(c->H, c->W, 0), hw1 = hot_map_words(c->H, c->W, 1);
    TRY(c->hotmap.reserve(n_images * (hw0 > hw1 ? hw0 : hw1), true)); // all zeros between batches: the scan stores hot words only, mark_tiles_kernel clears them
    for (size_t i = 0; i < init.size(); i++) init[i] = 1u;
    TRY(c->cur_box.reserve(init.size()));
    HIP_TRY(hipMemcpy(c->cur_box, init.data(), sizeof(uint32_t) * init.size(), hipMemcpyHostToDevice));
    const size_t cap = tiles * BOX_MAX_PARTS; // settle_tiles_kernel cuts a tile into at most that many items
    if (cap > 0xffffffffull) return fail(MOCAP_E_UNSUPPORTED, "batch too large for the work list");
    TRY(c->items.reserve(cap));
    return c->wide_tiles.reserve(4 * tiles); // up to 4 row bands per tile
}
static int ensure_mask(mocap_ctx* c, int n_images)
{
    if ((size_t)n_images <= c->mask_images) return 0;
    std::lock_guard<std::mutex> lk(c->mu);
    if ((size_t)n_images <= c->mask_images) return 0;
    c->mask_images = 0; c->last_images = 0;
    if (int rc = grow_mask_group(c, n_images)) { // not half a group: the error is returned once, the next call starts over
        c->mask.release(); c->cells.release(); c->tile_rows.release(); c->hotmap.release(); c->cur_box.release();
        c->items.release(); c->wide_tiles.release();
        return rc;
    }
    c->tile_rows_flip = 0; c->tile_rows_hold[0] = c->tile_rows_hold[1] = 0;
    c->mask_dirty = false;
    c->mask_images = n_images;
    return 0;
}

// a zeroed mask of the internal layout for n_images (the padding rows stay zero: nothing writes them)
static int ensure_blocked(mocap_ctx* c, Buf<uint32_t>& m, int n_images)
{
    const size_t words = (size_t)n_images * mask_image_words(c->H, c->wpr);
    if (words <= m.n) return 0;
    std::lock_guard<std::mutex> lk(c->mu);
    return m.reserve(words, true);
}

// the external group: occupancy words and tile regions of a caller-owned mask, never mixed with the context's own
static int ensure_ext(mocap_ctx* c, int n_images)
{
    if ((size_t)n_images <= c->cells_ext_images) return 0;
    std::lock_guard<std::mutex> lk(c->mu);
    if ((size_t)n_images <= c->cells_ext_images) return 0;
    c->cells_ext_images = 0;
    int rc = c->cells_ext.reserve((size_t)n_images * cells_per_image(c));
    if (!rc) rc = c->cur_box_ext.reserve(4 * (size_t)n_images * cells_per_image(c));
    if (rc) { c->cells_ext.release(); c->cur_box_ext.release(); return rc; }
    c->cells_ext_images = n_images;
    return 0;
}

int mocap_filter_mask(mocap_ctx_t c, const void* frames, int n_images, int cam_mod, int slot_base, size_t image_stride,
                      int pitch, uint32_t* mask_dev, void* stream)
{
    TRY(check_frames(c, frames, n_images, cam_mod, slot_base, image_stride, pitch));
    if (!mask_dev) return fail(MOCAP_E_INVALID, "null mask");
    if (set_device(c)) return MOCAP_E_HIP;
    TRY(ensure_mask(c, n_images)); // for the tile flags
    TRY(ensure_ext(c, n_images));
    TRY(ensure_blocked(c, c->mask_out, n_images));
    // filtered as a caller-owned mask (cleared by the scan, or written whole), then written whole into the caller's row-major one
    TRY(run_filter(c, frames, n_images, cam_mod, slot_base, image_stride, pitch, c->mask_out, c->cells_ext, (hipStream_t)stream));
    launch_mask_convert(c->mask_out, mask_dev, n_images, c->H, c->wpr, false, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return MOCAP_OK;
}

int mocap_contours_from_mask(mocap_ctx_t c, const uint32_t* mask_dev, int n_images, int32_t* out_xy, long xy_stride,
                             int32_t* out_count, long count_stride, int max_blobs, mocap_contour* dbg, int32_t* dbg_count,
                             int dbg_cap, void* stream)
{
    if (!c || !mask_dev || !out_xy || !out_count) return fail(MOCAP_E_INVALID, "null argument");
    if (n_images < 1 || max_blobs < 1 || xy_stride < 2L * max_blobs || count_stride < 1)
        return fail(MOCAP_E_INVALID, "n_images=%d max_blobs=%d strides %ld %ld", n_images, max_blobs, xy_stride, count_stride);
    if ((dbg != nullptr) != (dbg_count != nullptr) || (dbg && dbg_cap < 1)) return fail(MOCAP_E_INVALID, "inconsistent debug buffers");
    if (set_device(c)) return MOCAP_E_HIP;
    TRY(ensure_blocked(c, c->mask_in, n_images));
    launch_mask_convert(mask_dev, c->mask_in, n_images, c->H, c->wpr, true, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return run_contours(c, c->mask_in, nullptr, nullptr, n_images, out_xy, xy_stride, out_count, count_stride, max_blobs, dbg, dbg_count, dbg_cap,
                        (hipStream_t)stream);
}

int mocap_blob_centroids(mocap_ctx_t c, const void* frames, int n_images, int cam_mod, int slot_base, size_t image_stride,
                         int pitch, int32_t* out_xy, long xy_stride, int32_t* out_count, long count_stride, int max_blobs,
                         void* stream)
{
    TRY(check_frames(c, frames, n_images, cam_mod, slot_base, image_stride, pitch));
    if (!out_xy || !out_count || max_blobs < 1 || xy_stride < 2L * max_blobs || count_stride < 1)
        return fail(MOCAP_E_INVALID, "bad output arguments");
    if (set_device(c)) return MOCAP_E_HIP;
    TRY(ensure_mask(c, n_images));
    TRY(run_filter(c, frames, n_images, cam_mod, slot_base, image_stride, pitch, c->mask, c->cells, (hipStream_t)stream));
    return run_contours(c, c->mask, c->cells, contour_boxes(c), n_images, out_xy, xy_stride, out_count, count_stride, max_blobs, nullptr, nullptr, 0,
                        (hipStream_t)stream);
}

static int bayer_args(BayerArgs& a, const void* bayer, void* gray, int n_images, int H, int W, long spitch, long dpitch,
                      size_t src_image_stride, size_t dst_image_stride, int pattern, int gray_shift, bool gray_optional = false)
{
    if (!bayer || (!gray && !gray_optional)) return fail(MOCAP_E_INVALID, "null argument");
    if (n_images < 1 || n_images > 65535 || H < 3 || W < 3 || spitch < W || dpitch < W)
        return fail(MOCAP_E_INVALID, "bad geometry: n=%d H=%d W=%d pitches %ld %ld (H, W >= 3)", n_images, H, W, spitch, dpitch);
    if (n_images > 1 && (src_image_stride < (size_t)spitch * (H - 1) + W || dst_image_stride < (size_t)dpitch * (H - 1) + W))
        return fail(MOCAP_E_INVALID, "image strides smaller than an image");
    if (pattern < 0 || pattern > 3 || (gray_shift != 14 && gray_shift != 15))
        return fail(MOCAP_E_INVALID, "pattern %d (0..3 = BG, GB, RG, GR) / gray_shift %d (14 or 15)", pattern, gray_shift);
    a = BayerArgs{};
    a.src = (const uint8_t*)bayer; a.dst = (uint8_t*)gray;
    a.H = H; a.W = W; a.n_images = n_images;
    a.spitch = spitch; a.dpitch = dpitch; a.sstride = src_image_stride; a.dstride = dst_image_stride;
    a.ry = pattern >= 2; a.rx = pattern == 1 || pattern == 2;   // red sites: BG (0,0), GB (0,1), RG (1,1), GR (1,0)
    a.cb = gray_shift == 14 ? 1868u : 3735u; a.cg = gray_shift == 14 ? 9617u : 19235u; a.cr = gray_shift == 14 ? 4899u : 9798u;
    a.shift = gray_shift;
    return 0;
}

int mocap_blob_centroids_bayer(mocap_ctx_t c, const void* bayer_frames, void* gray_frames, int n_images, int cam_mod, int slot_base,
                               size_t image_stride, int pitch, int pattern, int gray_shift, int32_t* out_xy, long xy_stride,
                               int32_t* out_count, long count_stride, int max_blobs, void* stream)
{
    TRY(check_frames(c, bayer_frames, n_images, cam_mod, slot_base, image_stride, pitch));
    if (!out_xy || !out_count || max_blobs < 1 || xy_stride < 2L * max_blobs || count_stride < 1)
        return fail(MOCAP_E_INVALID, "bad output arguments");
    BayerArgs b;
    TRY(bayer_args(b, bayer_frames, gray_frames, n_images, c->H, c->W, pitch, pitch, image_stride, image_stride, pattern, gray_shift, true));
    if (set_device(c)) return MOCAP_E_HIP;
    TRY(ensure_mask(c, n_images));
    TRY(run_filter(c, gray_frames, n_images, cam_mod, slot_base, image_stride, pitch, c->mask, c->cells, (hipStream_t)stream, &b));
    return run_contours(c, c->mask, c->cells, contour_boxes(c), n_images, out_xy, xy_stride, out_count, count_stride, max_blobs, nullptr, nullptr, 0,
                        (hipStream_t)stream);
}

// ---- sub-pixel centroids (subpixel.hip) ---------------------------------------------------------------------------------
int mocap_refine_centroids(mocap_ctx_t c, const void* frames, int n_images, int cam_mod, int slot_base, size_t image_stride, int pitch,
                           int pattern, int gray_shift, const int32_t* xy, long xy_stride, const int32_t* count, long count_stride,
                           int max_blobs, int radius, int floor_, int iters, int coords, double* out_xy, long out_xy_stride,
                           int32_t* out_info, long out_info_stride, void* stream)
{
    if (!c || !frames || !xy || !count || !out_xy) return fail(MOCAP_E_INVALID, "null argument");
    if (radius < 1 || radius > 31 || floor_ < 0 || floor_ > 254 || iters < 1 || iters > 8 || (coords != 0 && coords != 1))
        return fail(MOCAP_E_INVALID, "radius %d (1..31), floor %d (0..254), iters %d (1..8), coords %d (0 raw, 1 ideal)", radius, floor_, iters, coords);
    if (max_blobs < 1 || max_blobs > SUBPIX_MAX_BLOBS || xy_stride < 2L * max_blobs || count_stride < 1 || out_xy_stride < 2L * max_blobs ||
        (out_info && out_info_stride < 2L * max_blobs))
        return fail(MOCAP_E_INVALID, "max_blobs %d (1..%d), strides %ld %ld %ld %ld", max_blobs, SUBPIX_MAX_BLOBS, xy_stride, count_stride,
                    out_xy_stride, out_info_stride);
    if (pattern < -1 || pattern > 3 || (pattern >= 0 && gray_shift != 14 && gray_shift != 15))
        return fail(MOCAP_E_INVALID, "pattern %d (-1 = gray frames, 0..3 = BG, GB, RG, GR) / gray_shift %d (14 or 15)", pattern, gray_shift);
    if (pattern >= 0 && (c->H < 3 || c->W < 3)) return fail(MOCAP_E_INVALID, "Bayer frames need H, W >= 3");
    TRY(check_frames(c, frames, n_images, cam_mod, slot_base, image_stride, pitch));
    if (set_device(c)) return MOCAP_E_HIP;
    RefineArgs a{};
    a.src = (const uint8_t*)frames; a.image_stride = image_stride; a.pitch = pitch; a.H = c->H; a.W = c->W;
    a.n_images = n_images; a.cam_mod = cam_mod;
    if (pattern >= 0) { // (the frames are their own gray buffer: bayer_args wants one, nothing is written)
        BayerArgs b;
        TRY(bayer_args(b, frames, nullptr, n_images, c->H, c->W, pitch, pitch, image_stride, image_stride, pattern, gray_shift, true));
        a.bayer = 1; a.ry = b.ry; a.rx = b.rx; a.cb = b.cb; a.cg = b.cg; a.cr = b.cr; a.shift = b.shift;
    }
    a.lens = c->lens + (size_t)SUBPIX_LENS * slot_base;
    a.xy = xy; a.xy_stride = xy_stride; a.count = count; a.count_stride = count_stride; a.max_blobs = max_blobs;
    a.radius = radius; a.floor = floor_; a.iters = iters; a.coords = coords;
    a.out_xy = out_xy; a.out_xy_stride = out_xy_stride; a.out_info = out_info; a.out_info_stride = out_info_stride;
    launch_refine_centroids(a, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return MOCAP_OK;
}

int mocap_undistort_u8(mocap_ctx_t c, int slot, const void* src, void* dst, int spitch, int dpitch, void* stream)
{
    if (!c || !src || !dst) return fail(MOCAP_E_INVALID, "null argument");
    if (slot < 0 || slot >= c->n_slots || c->slot_state[slot] == 0) return fail(MOCAP_E_STATE, "undistort slot %d not set", slot);
    if (spitch < c->W || dpitch < c->W) return fail(MOCAP_E_INVALID, "pitch < width");
    if (set_device(c)) return MOCAP_E_HIP;
    launch_undistort((const uint8_t*)src, (uint8_t*)dst, c->H, c->W, spitch, dpitch, slot_map(c, slot), slot_mapw(c, slot), (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return MOCAP_OK;
}

int mocap_image_filter_u8(mocap_ctx_t c, const void* src, void* dst, int spitch, int dpitch, int order, int slot, void* stream)
{
    if (!c || !src || !dst) return fail(MOCAP_E_INVALID, "null argument");
    if (order != 0 && order != 1) return fail(MOCAP_E_INVALID, "order must be 0 (image_filter_gpu) or 1 (image_filter_cpu)");
    if (spitch < c->W || dpitch < c->W) return fail(MOCAP_E_INVALID, "pitch < width");
    if (slot >= c->n_slots || (slot >= 0 && c->slot_state[slot] == 0)) return fail(MOCAP_E_STATE, "undistort slot %d not set", slot);
    if (set_device(c)) return MOCAP_E_HIP;
    hipStream_t s = (hipStream_t)stream;
    const int thr_mul = threshold_mul(c), ithresh = thr_mul - 1;
    if (order == 1) {
        const uint8_t* in = (const uint8_t*)src;
        int ip = spitch;
        if (slot >= 0 && c->slot_state[slot] == 2) { // undistort into dst, then filter in a second buffer
            return fail(MOCAP_E_UNSUPPORTED, "image_filter_cpu order with undistortion: call mocap_undistort_u8 first");
        }
        launch_median5(in, (uint8_t*)dst, c->H, c->W, ip, dpitch, ithresh, 1, s);
        HIP_TRY(hipGetLastError());
        return MOCAP_OK;
    }
    TRY(ensure_mask(c, 1));
    // the general kernel with a one-image batch; slot < 0 = no undistortion
    const FilterArgs a = filter_args(c, src, 0, spitch, c->mask, c->cells, slot, 1, 1, thr_mul);
    c->mask_dirty = true; c->last_images = 1;
    launch_filter_mask(a, slot >= 0 && c->slot_state[slot] == 2, s);
    HIP_TRY(hipGetLastError());
    launch_mask_expand(c->mask, c->wpr, (uint8_t*)dst, c->H, c->W, dpitch, s);
    HIP_TRY(hipGetLastError());
    return MOCAP_OK;
}

int mocap_box_blur_u8(mocap_ctx_t c, const void* src, void* dst, int H, int W, int spitch, int dpitch, int ksize, void* stream)
{
    if (!c || !src || !dst) return fail(MOCAP_E_INVALID, "null argument");
    if (H < 1 || W < 1 || spitch < W || dpitch < W || ksize < 1 || ksize > 31) return fail(MOCAP_E_INVALID, "bad geometry");
    if (set_device(c)) return MOCAP_E_HIP;
    launch_box_blur((const uint8_t*)src, (uint8_t*)dst, H, W, spitch, dpitch, ksize, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return MOCAP_OK;
}

int mocap_bayer_gray_u8(mocap_ctx_t c, const void* bayer, void* gray, int n_images, int H, int W, long spitch, long dpitch,
                        size_t src_image_stride, size_t dst_image_stride, int pattern, int gray_shift, void* stream)
{
    if (!c) return fail(MOCAP_E_INVALID, "null argument");
    BayerArgs a;
    TRY(bayer_args(a, bayer, gray, n_images, H, W, spitch, dpitch, src_image_stride, dst_image_stride, pattern, gray_shift));
    if (set_device(c)) return MOCAP_E_HIP;
    launch_bayer_gray(a, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return MOCAP_OK;
}

int mocap_demosaic_u8(mocap_ctx_t c, const void* bayer, void* bgr, int H, int W, int spitch, void* stream)
{
    if (!c || !bayer || !bgr) return fail(MOCAP_E_INVALID, "null argument");
    if (H < 1 || W < 1 || spitch < W) return fail(MOCAP_E_INVALID, "bad geometry");
    if (set_device(c)) return MOCAP_E_HIP;
    launch_demosaic((const uint8_t*)bayer, (uint8_t*)bgr, H, W, spitch, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return MOCAP_OK;
}

int mocap_tile_stats(mocap_ctx_t c, uint64_t* tiles, uint64_t* skipped)
{
    if (!c) return fail(MOCAP_E_INVALID, "null context");
    if (set_device(c)) return MOCAP_E_HIP;
    uint64_t total = 0, full = 0;
    if (c->cells && c->last_images > 0) {
        HIP_TRY(hipDeviceSynchronize());
        Tiling t = tiling(c);
        size_t per = cells_per_image(c), n = per * (size_t)c->last_images;
        std::vector<uint32_t> w(n);
        HIP_TRY(hipMemcpy(w.data(), c->cells, sizeof(uint32_t) * n, hipMemcpyDeviceToHost));
        int valid_chunks = (c->H + t.rows - 1) / t.rows; // chunks that start inside the image
        total = (uint64_t)c->last_images * valid_chunks * t.n_strips;
        for (size_t i = 0; i < n; i++) full += w[i] >> 31;
    }
    if (tiles) *tiles = total;
    if (skipped) *skipped = total - full;
    return MOCAP_OK;
}

int mocap_list_stats(mocap_ctx_t c, uint32_t* items, uint32_t* wide, uint32_t* split)
{
    if (!c) return fail(MOCAP_E_INVALID, "null context");
    if (set_device(c)) return MOCAP_E_HIP;
    uint32_t cnt[16] = {0};
    static_assert(SPLIT_COUNTER != 0 && SPLIT_COUNTER != 8 && SPLIT_COUNTER < 16, "a word of its own in the first line of the counter block");
    if (c->n_items) {
        HIP_TRY(hipDeviceSynchronize());
        HIP_TRY(hipMemcpy(cnt, c->n_items, sizeof(cnt), hipMemcpyDeviceToHost));
    }
    if (items) *items = cnt[0];
    if (wide) *wide = cnt[8];
    if (split) *split = cnt[SPLIT_COUNTER];
    return MOCAP_OK;
}

// read-back of the context's own mask (tests): a reader only -- no state of the context changes, no scratch, no synchronisation
int mocap_own_mask(mocap_ctx_t c, int n_images, uint32_t* mask_dev, void* stream)
{
    if (!c) return fail(MOCAP_E_INVALID, "null argument");
    if (n_images < 1) return fail(MOCAP_E_INVALID, "n_images = %d", n_images);
    if (!mask_dev) return fail(MOCAP_E_INVALID, "null argument");
    if ((size_t)n_images > c->mask_images)
        return fail(MOCAP_E_INVALID, "n_images = %d, the context's own mask holds %zu images", n_images, c->mask_images);
    if (set_device(c)) return MOCAP_E_HIP;
    launch_mask_convert(c->mask, mask_dev, n_images, c->H, c->wpr, false, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return MOCAP_OK;
}

} // extern "C"
