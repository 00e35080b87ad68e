// ctx.h -- what the C-ABI's host files (abi_*.hip) share: the error channel, the owners of device memory, the per-GPU context
// and its tiling.  Host-only, included by those files alone; whatever one file uses by itself stays static in that file.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <math.h>
#include <string>
#include <vector>
#include <mutex>
#include <memory>
#include "../../include/mocap_hip.h"
#include "kernels.h"

using namespace mocap;

// sets the calling thread's message for mocap_last_error and returns `code` (abi_ctx.hip)
int fail(int code, const char* fmt, ...);

#define HIP_TRY(expr)                                                                                         \
    do {                                                                                                      \
        hipError_t e_ = (expr);                                                                               \
        if (e_ != hipSuccess) return fail(MOCAP_E_HIP, "%s failed: %s", #expr, hipGetErrorString(e_));        \
    } while (0)
#define TRY(expr) do { if (int rc_ = (expr)) return rc_; } while (0) // for the file's own functions, which return fail()'s code

// The one owner of a block of device memory (Pinned: of page-locked host memory): every allocation and every free of the ABI files happens
// in here.  `n` is what reserve() was last asked for, in elements, and is set only once the block is ready for use.
template <class T, bool Pinned = false>
struct Buf {
    T* p = nullptr;
    size_t n = 0;
    Buf() = default;
    Buf(Buf&& o) : p(o.p), n(o.n) { o.p = nullptr; o.n = 0; }
    Buf& operator=(Buf&& o) { if (this != &o) { release(); p = o.p; n = o.n; o.p = nullptr; o.n = 0; } return *this; }
    ~Buf() { release(); }
    operator T*() const { return p; }
    T* operator->() const { return p; }
    void release()
    {
        if (p) (void)(Pinned ? hipHostFree(p) : hipFree(p));
        p = nullptr; n = 0;
    }
    // Room for `count` elements, zero-filled if asked.  A block that is large enough stays; a smaller one is REPLACED, its contents are
    // not carried over (every caller fills what it reads).  Batches in flight on other streams may still read the old block, hence
    // the device-wide wait before it is freed.  Callers that share a context take c->mu around a growth.
    int reserve(size_t count, bool zero = false)
    {
        if (count <= n) return 0;
        if (p) { HIP_TRY(hipDeviceSynchronize()); release(); }
        HIP_TRY(Pinned ? hipHostMalloc((void**)&p, sizeof(T) * count) : hipMalloc((void**)&p, sizeof(T) * count));
        if (zero) HIP_TRY(hipMemset(p, 0, sizeof(T) * count));
        n = count;
        return 0;
    }
};

struct EvPair { hipEvent_t a, b; };
// the scan's probe counters (BrightArgs::probe): 128 pairs, each pair in a cache line of its own (PROBE_STRIDE words apart) -- packed
// into 8 lines, the ~200 k atomic adds of a probed batch queued up on 8 L2 atomic units: 0.3 ms on top of the scan's 0.95
constexpr size_t PROBE_BYTES = 128 * mocap::PROBE_STRIDE * sizeof(uint32_t);
using mocap::PROBE_STRIDE;

// One RCCL communicator per rank, shared by the rank's contexts (= the batches in flight): RCCL wants the operations of a
// communicator issued one after the other, so every all-gather waits for the event its predecessor recorded (on whatever
// stream that one ran) and records it anew.
struct SharedComm {
    void* comm = nullptr;      // ncclComm_t
    int rank = 0, world = 1, device = 0;
    hipEvent_t last = nullptr; // completion of the most recent all-gather on this communicator
    bool have_last = false;
    std::mutex mu;             // issue order = lock order
    bool (*destroy_comm)(void*) = nullptr; // ncclCommDestroy, bound when the communicator is created
    // the last context sharing the communicator is gone (mocap_comm_destroy, or a context destroyed without it): nothing leaks
    ~SharedComm()
    {
        if (!comm && !last) return;
        (void)hipSetDevice(device);
        if (last) { if (have_last) (void)hipEventSynchronize(last); (void)hipEventDestroy(last); }
        if (comm && destroy_comm) (void)destroy_comm(comm);
    }
};

// Performance switches of a context (A/B measurements, tests of the alternative code paths; none changes a result).  They are
// read from the environment ONCE, by mocap_ctx_create (MOCAP_<NAME IN CAPITALS>), and can be changed per context afterwards
// with mocap_set_tuning: the hot path itself never calls getenv.  -1 = "not set" where 0 is a meaningful value.
// The list is tuning.def: one line per switch with its default and its bounds.
struct Tuning {
#define X(name, def, lo, hi) int name = def;
#include "tuning.def"
#undef X
};
#define X(name, def, lo, hi) static_assert((lo) <= (def) && (def) <= (hi), "tuning.def: the default of " #name " lies outside its bounds");
#include "tuning.def"
#undef X

// The slots of mocap_ctx::ev, in the order of mocap_profile_read's ms[5] / cnt[5] (part of the ABI).
enum ProfSlot { PROF_FILTER, PROF_CONTOURS, PROF_CORRESPOND, PROF_SCAN, PROF_SETTLE, PROF_SLOTS };
static_assert(PROF_SLOTS == 5, "mocap_profile_read hands out five slots");

struct mocap_ctx {
    int device = 0, W = 0, H = 0, n_slots = 0, wpr = 0;
    int box_grid = 2048;      // workgroups of the box kernel: the resident ones (box_filter_blocks_per_cu() per CU)
    int n_cu = 256;           // compute units of the device
    mocap_blob_params prm{5, 5, 255 * 0.85, 500.0, 0.5};
    Tuning tune;
    Buf<uint32_t> maps;       // [2][n_slots][H][W]: tap positions, then blend weights (general form)
    Buf<uint32_t> map4;       // [n_slots][H][W] (+ 4 words): compact table of the box kernel
    Buf<ushort4> srcbox;      // [n_slots][ceil(H/8)][ceil(W/8)]: source box per 8x8 output cell (box kernel)
    Buf<ushort4> rowbox;      // [n_slots][H][n_strips]: source box per row and strip (staged row pipeline)
    Buf<uint32_t> map_flags;  // [n_slots] device
    Buf<double> lens;         // [n_slots][SUBPIX_LENS]: the slot's K, dist and "the table is the identity" (mocap_refine_centroids)
    std::vector<int> slot_state; // 0 unset, 1 identity, 2 remap
    std::vector<int> slot_compact; // 1 = the slot's displacements fit the compact table (identity: always)
    std::vector<uint32_t> slot_wmax; // largest total blend weight of a source pixel (1024 = identity); 0 = early-out not provable
    Buf<uint2> reach;         // [n_slots][ceil(H/8)][ceil(W/8)] per 8x8 source cell: box of the output pixels that read it
    Buf<uint8_t> cflags;      // [n_slots][cells] border-cut window flags per source cell (see BrightArgs)
    // The mask group: grown together by ensure_mask to mask_images images, the count stored once all of them stand.
    Buf<uint32_t> mask; size_t mask_images = 0;
    bool mask_dirty = false;               // the general kernel wrote the mask whole: clear it before the box path runs again
    Buf<uint32_t> cells;                   // occupancy cells written by the filter kernels for c->mask
    int last_images = 0;                   // images of the most recent batch that wrote c->cells
    Buf<uint32_t> hotmap;                  // [mask_images][hot_map_words(H, W, 1)] the scan's hot map (BrightArgs::hotmap)
    Buf<uint32_t> tile_rows;               // [2][mask_images][tiles][4] the scan's record per tile (see BoxArgs): two arrays, alternating
    int tile_rows_flip = 0;                //   per batch: the one the scan widens and settle reads / the one settle empties
    int tile_rows_hold[2] = {0, 0};        //   images whose boxes each of the two may still hold (batches of varying size)
    Buf<uint32_t> cur_box;                 // [mask_images][tiles][4] output region / scan box of the last batch per tile (BoxArgs)
    Buf<BoxItem> items;                    // work list of the box kernel
    Buf<uint4> wide_tiles;                 // list of the tiles with wide boxes (filter_mask_kernel, list form)
    Buf<uint32_t> n_items;                 // item count + the 8 head words of the box kernel's runs (not part of the group: fixed size)
    hipStream_t side = nullptr; hipEvent_t ev_fork = nullptr, ev_join = nullptr; // the wide tiles are filtered beside the box kernel: side stream, fork / join events
    // excess base of the scan, adapted between batches: two candidates (tight / tolerant of bright backgrounds), the current
    // one, and a probe now and then that counts the hot cells both would leave (BrightArgs::probe)
    int base_sel = 1; int probe_age = 0; bool probe_pending = false; Buf<uint32_t> probe_dev; Buf<uint32_t, true> probe_host; hipEvent_t probe_ev = nullptr;
    bool walk_count_zeroed = false;        // the filter stage of the current batch has zeroed walk_count (settle_tiles_kernel)
    int probe_images = 0;                  // images the pending probe counted on (every 16th of its batch)
    bool hot_dense = false;                // the last probe found a crowded scene (many hot cells per image): the scan leaves a hot map
    Buf<uint32_t> cells_ext, cur_box_ext; size_t cells_ext_images = 0; // the external group: the same for caller-owned masks (mocap_filter_mask)
    // the caller's row-major masks pass through masks of the internal layout (kernels.h: mask_word_index), converted at the boundary:
    Buf<uint32_t> mask_out;                // mocap_filter_mask filters into this one (a caller-owned mask for run_filter)
    Buf<uint32_t> mask_in;                 // mocap_contours_from_mask reads the caller's mask from this one
    Buf<uint8_t> gray_scratch;             // mocap_blob_centroids_bayer without a gray buffer, where the gray-less path
                                           //   cannot run: the gray frames go here (grown to the largest batch)
    // The contour group: grown together by run_contours to cwork_images images.
    Buf<uint8_t> cwork; size_t cwork_images = 0; // contour kernel workspace, contour_work_bytes() per image
    Buf<uint64_t> walk_list, link_list;    // contour stage, split form: the batch's border walks / link walks
    Buf<uint32_t> walk_count;              //   their counters (fixed size, allocated with the group's first growth)
    Buf<CameraTable> cams; int n_cam = 0, n_F = 0;
    Buf<double> scratch;                   // error scratch of mocap_correspond
    Buf<double> ba_obj;                    // object points of mocap_ba_residuals, [B][N][3]
    Buf<char> fund_scratch;                // mocap_fundamental_ransac: every hypothesis' matrix, the counters, the pair offsets
    Buf<char> rig_scratch;                 // mocap_rig_bundle_adjust / mocap_rig_linearize: the state record, both state buffers, the blocks and partial sums
    Buf<char> intr_scratch;                // mocap_intrinsics_calibrate / mocap_intrinsics_linearize: the offsets, the state records, both state buffers, the views' records
    Buf<char, true> ba_pinned;             // mocap_ba_residuals' host-side hand-over: parameters in, residuals + counts out (the kernel reads / writes it directly)
    std::shared_ptr<struct SharedComm> comm; // RCCL communicator of mocap_comm_init / mocap_comm_share, else null
    bool profiling = false;
    std::vector<EvPair> ev[PROF_SLOTS];
    std::mutex mu;
};

static int set_device(mocap_ctx* c) { HIP_TRY(hipSetDevice(c->device)); return 0; }

struct Tiling { int rows, n_cgroups, n_strips; };
static Tiling tiling(const mocap_ctx* c)
{
    Tiling t;
    // Rows per tile.  Must be <= 68: settle_tiles_kernel cuts a tile into at most 4 items of BOX_HCAP quad-rows.
    t.rows = c->tune.rows;
    if (c->H < 4 * 32) t.rows = (c->H + 3) / 4 > 8 ? (c->H + 3) / 4 : 8;
    t.n_cgroups = (c->H + 4 * t.rows - 1) / (4 * t.rows);
    t.n_strips = (c->W + 239) / 240;
    return t;
}

static size_t source_cells(const mocap_ctx* c) { return (size_t)((c->H + 7) / 8) * ((c->W + 7) / 8); }
static size_t cells_per_image(const mocap_ctx* c) { Tiling t = tiling(c); return (size_t)t.n_cgroups * 4 * t.n_strips; }
// a slot's part of the undistort tables (null before the first mocap_set_undistort): tap positions, blend weights, compact table
static uint32_t* slot_map(const mocap_ctx* c, int slot) { return c->maps ? c->maps + (size_t)slot * c->H * c->W : nullptr; }
static uint32_t* slot_mapw(const mocap_ctx* c, int slot) { return c->maps ? c->maps + (size_t)(c->n_slots + slot) * c->H * c->W : nullptr; }
static uint32_t* slot_map4(const mocap_ctx* c, int slot) { return c->map4 ? c->map4 + (size_t)slot * c->H * c->W : nullptr; }

// Cuts a scratch block (the solvers' scratch, mocap_ba_residuals' pinned block) into buffers, each rounded up to 16 bytes, in the order of the take() calls.  Over
// a null base it only counts (`used` is the block's size); over the block it sets the pointers.
struct Carver {
    char* base;
    size_t used = 0;
    template <class T> void take(T*& p, size_t count) { p = base ? (T*)(base + used) : nullptr; used += (sizeof(T) * count + 15) & ~(size_t)15; }
};

// profiling (abi_ctx.hip): an event pair around a stage's launches, kept in c->ev[slot] for mocap_profile_read
void prof_begin(mocap_ctx* c, hipStream_t s, EvPair& p, bool& on);
void prof_end(mocap_ctx* c, ProfSlot slot, hipStream_t s, EvPair& p, bool on);
