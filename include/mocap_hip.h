/*
 * mocap_hip.h -- C-ABI of libmocap_hip.so, the MI355X (gfx950) implementation of MocapV2's per-frame hot path.
 *
 * Plain C, pointers and sizes only.  Every entry point returns 0 on success or a negative MOCAP_E_* code;
 * mocap_last_error() returns a thread-local description.  No C++ exception crosses the boundary.  The library
 * never owns caller memory: `*_dev` arguments are raw HIP device pointers supplied by the caller (e.g.
 * torch.Tensor.data_ptr()), `stream` is a hipStream_t passed as void* (NULL = the default stream).  All work is
 * enqueued on `stream` and is asynchronous unless stated otherwise.
 *
 * Each declaration cites the reference interface (RashmikaDushan/MocapV2) it stands in for.
 */
#ifndef MOCAP_HIP_H
#define MOCAP_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MOCAP_ABI_VERSION 7
#define MOCAP_API __attribute__((visibility("default")))

enum {
    MOCAP_OK = 0,
    MOCAP_E_INVALID = -1,     /* bad argument */
    MOCAP_E_HIP = -2,         /* a HIP runtime call failed (no GPU, out of memory, ...) */
    MOCAP_E_UNSUPPORTED = -3, /* parameter outside what the kernels implement */
    MOCAP_E_STATE = -4        /* required set-up call missing */
};

/* per-image status written to out_count by the blob kernels when an internal capacity is exceeded */
enum {
    MOCAP_BLOB_E_CANDIDATES = -2, /* more than 1024 border start candidates in one image (pixels that locally look like the
                                     first pixel of a border; how much of the frame holds set pixels is no limit) */
    MOCAP_BLOB_E_CONTOURS = -3,   /* more than 384 borders or 256 kept contours in one image */
    MOCAP_BLOB_E_STEPS = -4,      /* a border longer than the step limit */
    MOCAP_BLOB_E_DEPTH = -5,      /* a kept contour nested deeper than 8 levels */
    MOCAP_CORR_E_GROUPS = -2,     /* more than 16 candidates for one (root, camera), > max_groups groups for one root, or more
                                     groups in the whole time step than its share of the error scratch holds: max(2 * max_groups,
                                     8192) by default, raised with mocap_set_tuning(ctx, "corr_step_groups", n) */
    MOCAP_CORR_E_TRUNCATED = -3,  /* a camera holds more image points than the P that mocap_correspond was told to read */
    MOCAP_CORR_E_BLOB = -4,       /* a camera's point count is negative: its blob stage reported MOCAP_BLOB_E_* */
    MOCAP_CORR_E_OUTPUT = -5,     /* mocap_correspond_visible: more accepted markers in the time step than the Q output rows */
    MOCAP_TRACK_E_FULL = -2,      /* mocap_track_markers, status[t]: no free slot for a new marker of the step (its rows hold -1) */
    MOCAP_TRACK_E_IDS = -3,       /* the identity counter stands at INT32_MAX: no new marker gets an identity (the counter never wraps) */
    MOCAP_TRACK_E_INPUT = -4,     /* a blind step: its count n[t] is negative (the correspondence's own failure code) */
    MOCAP_TRACK_E_COUNT = -5,     /* a blind step: its count n[t] exceeds 256 or the Q rows of a step */
    MOCAP_RIGID_LOST = 1,         /* mocap_rigid_poses, status[t][b]: no candidate reached min_markers inliers (not an error) */
    MOCAP_RIGID_E_BLIND = -2,     /* a blind step: its count n[t] is negative (the correspondence's own failure code) */
    MOCAP_RIGID_E_CAPACITY = -3,  /* a blind step: its count n[t] exceeds 64 or the Q rows of a step */
    MOCAP_RIGID_E_MODEL = -4,     /* the body's tables are not a model: n_markers outside 3..8, n_tri outside 1..56, or a triple
                                     that is not 0 <= a < b < c < n_markers */
    MOCAP_RIGID_E_HYP = -5,       /* more than max_hyp candidates for the body in the step: it has no result there */
    MOCAP_REFINE_E_VIEWS = -2,    /* mocap_refine_points, status[t][q]: the row has fewer than 2 member cameras */
    MOCAP_REFINE_E_INPUT = -3,    /* the row's point is not finite, a member's index lies outside [0, P), or its mask has bits at or above C */
    MOCAP_REFINE_E_BEHIND = -4,   /* the row's point is not in front of every member camera */
    MOCAP_FUND_E_SAMPLE = -2,     /* mocap_fundamental_ransac: a sample index outside its pair's point list */
    MOCAP_FUND_E_DEGENERATE = -3  /* no valid hypothesis (e.g. coincident points), a winner with fewer than 8 inliers, or
                                     inliers that do not span a model in the refit */
};

typedef struct mocap_ctx* mocap_ctx_t;

/* The literals of reference lib/ImageOperations.py:19-20,28-30,50 as a parameter block (same defaults). */
typedef struct mocap_blob_params {
    int32_t ksize;        /* box blur window, 5   (ImageOperations.py:28)  -- only 5 is implemented */
    int32_t median;       /* median window, 5     (ImageOperations.py:30)  -- only 5 is implemented */
    double thresh;        /* 255*0.85             (ImageOperations.py:29) */
    double min_area;      /* 500                  (ImageOperations.py:50) */
    double min_circ;      /* 0.5                  (ImageOperations.py:50) */
} mocap_blob_params;

/* One border as seen by the contour kernel; used by the parity tests. */
typedef struct mocap_contour {
    int32_t key, is_hole, sx, sy, npts, steps;
    int64_t a00, a10, a01;
    double area, perimeter;
    int32_t kept, cx, cy, link, parent, order;
} mocap_contour;

MOCAP_API int mocap_abi_version(void);
MOCAP_API const char* mocap_last_error(void);

/* Context for one GPU and one image geometry.  n_slots = number of undistortion maps kept resident
 * (one per camera; the reference itself always uses camera 0's, lib/ImageOperations.py:37).
 * A context owns the per-batch scratch of the blob stage (bit mask, occupancy words, patches, contour workspace):
 * its mocap_blob_centroids / mocap_filter_mask / mocap_image_filter_u8 calls must be ordered on one stream.  For
 * several batches in flight use one context per stream. */
MOCAP_API int mocap_ctx_create(int device_id, int width, int height, int n_slots, mocap_ctx_t* out);
MOCAP_API int mocap_ctx_destroy(mocap_ctx_t ctx);
MOCAP_API int mocap_sync(mocap_ctx_t ctx, void* stream); /* hipStreamSynchronize */

MOCAP_API int mocap_set_blob_params(mocap_ctx_t ctx, const mocap_blob_params* p);

/* Performance switches of one context (the reference has none: its tunables are literals).  None of
 * them changes a result; they select between equivalent code paths (A/B measurements, tests of the alternative paths) or
 * size a scratch buffer.  mocap_ctx_create reads each of them ONCE from the environment (MOCAP_<NAME> in capitals; the hot
 * path never calls getenv), this call changes one for the context afterwards.  Names: skip_dark,
 * general_filter, dense_boxes, remap_pipeline, cluster, wide_quads_remap, wide_quads_identity, wide_bands, wide_split, wide_fork,
 * box_prio, scan_prio, contour_prio, corr_prio, box_stage_bytes, box_timing, contour_timing, follow_timing, scan_wide, scan_hotmap, scan_serial, rows_staged, rows_stage_dw, wide_blocks_per_cu, contour_blocks_per_cu, mark_blocks_per_cu, contour_defer,
 * scan_blocks_per_cu, scan_slices, excess_base, probe_debug, contour_boxes, contours_split, corr_threads, corr_step_groups.  (rows, box_blocks_per_cu and base_sel
 * shape the context at creation: environment only.)  Must not race with a batch call on the same context. */
MOCAP_API int mocap_set_tuning(mocap_ctx_t ctx, const char* name, int value);

/* cv.undistort(img, K, dist) set-up (lib/ImageOperations.py:38): builds the quantised remap table of `slot`
 * on the device (synchronous).  identity_out (optional) receives 1 when the table is the identity. */
MOCAP_API int mocap_set_undistort(mocap_ctx_t ctx, int slot, const double K[9], const double dist[5], int* identity_out);

/* What mocap_set_undistort found out about a slot's table -- and with it, which road the slot's images take in
 * mocap_blob_centroids.  The sparse road (one streaming pass that proves most of a dark IR frame's mask zero, then the
 * filter on the marked tiles only) needs (a) a provable early-out: every 5x5 window of the undistorted image reads at most
 * 9 x 9 source pixels, and (b) the compact table: tap displacements within 11 bits.  A lens model outside either bound is
 * still filtered exactly, but every tile of every image goes through the dense row pipeline: the same results at about 7x
 * the time on a dark scene.  This call makes that visible instead of silent (sparse_path = 0). */
typedef struct mocap_undistort_info_t {
    int32_t identity;            /* the table is the identity (zero distortion) */
    int32_t compact_table;       /* displacements fit the box kernel's 4-byte table */
    int32_t early_out_provable;  /* the dark-tile bound holds for this table */
    int32_t max_source_weight;   /* largest total blend weight of one source pixel over all output pixels (1024 = one pixel; 0 = not provable) */
    int32_t sparse_path;         /* 1 = images of this slot take the sparse road (also needs the tuning switches at their defaults) */
} mocap_undistort_info_t;
MOCAP_API int mocap_undistort_info(mocap_ctx_t ctx, int slot, mocap_undistort_info_t* out);

/* camera_params + camera_poses of lib/Helpers.py (K_i, dist_i from jsons/camera-params-in.json :30-40,
 * R_i, t_i from get_extrinsics :282-291); n <= 32.  Synchronous host->device copy. */
MOCAP_API int mocap_set_cameras(mocap_ctx_t ctx, int n, const double* K /*[n][9]*/, const double* dist /*[n][5]*/,
                      const double* R /*[n][9]*/, const double* t /*[n][3]*/);
/* Fs of lib/Helpers.py:22-28: F[i-1] maps a camera-0 pixel to its epipolar line in camera i; n <= 31. */
MOCAP_API int mocap_set_fundamentals(mocap_ctx_t ctx, int n, const double* F /*[n][9]*/);

/* _find_dot over a batch (lib/ImageOperations.py:33-78 without the drawing calls).
 * frames_dev: n_images uint8 images of height x width, rows `pitch` bytes apart, images `image_stride` bytes
 * apart; image n uses undistort slot slot_base + n % cam_mod (frames laid out [time][camera]).
 * Image n writes its (cx, cy) pairs, in the reference's contour order, to out_xy_dev + n*xy_stride (int32
 * [max_blobs][2]) and its number of image points to out_count_dev[n*count_stride] (0 where the reference returns
 * [[None, None]]; values above max_blobs mean truncation; negative = MOCAP_BLOB_E_*).  The strides (in int32
 * elements) let both land in one fixed-size centroid record per image, ready for the all-gather. */
MOCAP_API int mocap_blob_centroids(mocap_ctx_t ctx, const void* frames_dev, int n_images, int cam_mod, int slot_base,
                         size_t image_stride, int pitch, int32_t* out_xy_dev, long xy_stride, int32_t* out_count_dev,
                         long count_stride, int max_blobs, void* stream);

/* The two halves of mocap_blob_centroids, exposed for tests and profiling.
 * mask_dev: [n_images][height][ceil(width/32)] uint32, bit b of word k = pixel 32k+b.  Must be zero-initialised
 * once by the caller (padding bits are never written). */
MOCAP_API int mocap_filter_mask(mocap_ctx_t ctx, const void* frames_dev, int n_images, int cam_mod, int slot_base,
                      size_t image_stride, int pitch, uint32_t* mask_dev, void* stream);
MOCAP_API int mocap_contours_from_mask(mocap_ctx_t ctx, const uint32_t* mask_dev, int n_images, int32_t* out_xy_dev,
                             long xy_stride, int32_t* out_count_dev, long count_stride, int max_blobs,
                             mocap_contour* dbg_dev /*[n_images][dbg_cap] or NULL*/, int32_t* dbg_count_dev,
                             int dbg_cap, void* stream);

/* image_filter_gpu (order 0: blur -> threshold -> median, lib/ImageOperations.py:23-31) and image_filter_cpu
 * (order 1: median -> threshold, :15-21) on one image; slot >= 0 applies that undistortion first (as _find_dot
 * does), slot < 0 filters the image as given.  dst receives the {0,255} image. */
MOCAP_API int mocap_image_filter_u8(mocap_ctx_t ctx, const void* src_dev, void* dst_dev, int spitch, int dpitch, int order,
                          int slot, void* stream);
/* cv.undistort through the table of `slot` (lib/ImageOperations.py:38) */
MOCAP_API int mocap_undistort_u8(mocap_ctx_t ctx, int slot, const void* src_dev, void* dst_dev, int spitch, int dpitch,
                       void* stream);
/* fast_cuda_blur(image, kernel_size) (lib/CudaOperations.py:24-41): uint8 in, uint8 out, any size */
MOCAP_API int mocap_box_blur_u8(mocap_ctx_t ctx, const void* src_dev, void* dst_dev, int height, int width, int spitch,
                      int dpitch, int ksize, void* stream);
/* The two pixel steps in front of _find_dot in the camera loop (RealtimeTracking_FLIR.py:103-104):
 * cv2.cvtColor(raw, cv2.COLOR_BAYER_GR2BGR) then cv2.cvtColor(., cv2.COLOR_BGR2GRAY), fused (no BGR image), for
 * n_images frames per launch.  pattern 0..3 = BG, GB, RG, GR (cv2.COLOR_BayerBG2BGR + pattern; the reference uses GR = 3);
 * gray_shift 14 = OpenCV's R2Y/G2Y/B2Y fixed point (4899, 9617, 1868, >> 14), 15 = its 15-bit set (9798, 19235, 3735).
 * Bilinear demosaic with rounded means; first/last row and column repeat their inner neighbours.  H, W >= 3.
 * Image i starts at bayer_dev + i * src_image_stride / gray_dev + i * dst_image_stride (bytes). */
MOCAP_API int mocap_bayer_gray_u8(mocap_ctx_t ctx, const void* bayer_dev, void* gray_dev, int n_images, int height, int width,
                        long spitch, long dpitch, size_t src_image_stride, size_t dst_image_stride, int pattern,
                        int gray_shift, void* stream);
/* mocap_blob_centroids on raw Bayer frames: the camera loop's cvtColor pair (RealtimeTracking_FLIR.py:103-104) followed by
 * _find_dot (:105) for a batch.  Results equal mocap_bayer_gray_u8 followed by mocap_blob_centroids.  H, W >= 3.
 * gray_frames_dev == NULL (accepted since ABI 6; the normal use): no gray frame is written anywhere.  The early-out's
 * streaming pass reads every Bayer byte once, and the filter forms the gray values it needs from the Bayer frames.
 * That path needs a width that is a multiple of 16, a height that is a multiple of 8, 16-byte aligned frames, pitch and
 * image stride, and the sparse filter path.
 * Otherwise (the dense path, MOCAP_SKIP_DARK=0 and MOCAP_GENERAL_FILTER=1 included) the context converts the frames into
 * a gray scratch buffer of its own, allocated on first use and grown to the largest batch: one frame-sized buffer, and
 * one gray write and read per pixel.
 * gray_frames_dev != NULL: the gray frames are written there (same pitch and image stride as the Bayer frames) and read
 * back by the filter; where the geometry above allows, the conversion is fused with the early-out's streaming pass. */
MOCAP_API int mocap_blob_centroids_bayer(mocap_ctx_t ctx, const void* bayer_frames_dev, void* gray_frames_dev, int n_images,
                               int cam_mod, int slot_base, size_t image_stride, int pitch, int pattern, int gray_shift,
                               int32_t* out_xy_dev, long xy_stride, int32_t* out_count_dev, long count_stride,
                               int max_blobs, void* stream);
/* Sub-pixel centroids: back to the frame bytes around every integer centroid of mocap_blob_centroids.  The reference has no
 * counterpart (its centroid is int(M["m10"] / M["m00"]), which truncates): the contract is the definition of DESIGN.md section 2,
 * restated by tests/subpixel_ref.py; integer sums and FP64 operations rounded one by one, so the device equals the restatement
 * bit for bit.  New symbol, MOCAP_ABI_VERSION stays 7.
 * Frames, cam_mod, slot_base, image_stride and pitch as in mocap_blob_centroids (no alignment demands); pattern -1 = gray
 * frames, 0..3 = raw Bayer frames whose gray values are formed site by site as mocap_bayer_gray_u8 forms them (gray_shift 14
 * or 15; it is not looked at for gray frames; H, W >= 3), no gray frame is written.  xy_dev, count_dev and their strides mean
 * what they mean in mocap_blob_centroids: the records are read in place.  An image with count <= 0 writes nothing, a count above
 * max_blobs (1..256) refines the first max_blobs points, rows at and beyond the count are not written.
 * Per centroid (cx, cy): the start pixel is the centroid mapped into the raw frame by the slot's forward lens model (U, V),
 * rounded and clamped into the image ((cx, cy) itself for an identity slot); over the window of `radius` (1..31) pixels around
 * it, clipped to the image, with the weights w = max(0, p - floor) (floor 0..254): S = sum w and the weighted mean position; the
 * window moves to the mean's pixel and the sums are formed again, `iters` (1..8) windows at most.  Flags of the last window:
 *   MOCAP_SUBPIX_EMPTY      S == 0
 *   MOCAP_SUBPIX_EDGE       a pixel of the unclipped window's outermost ring has w > 0: the blob is wider than the window, or a
 *                           neighbour leaks in
 *   MOCAP_SUBPIX_NEIGHBOUR  the start pixel of another centroid of the image lies inside the window
 *   MOCAP_SUBPIX_MOVING     the last window still wants to move
 *   MOCAP_SUBPIX_CUT        the image border clipped the window (informational)
 * coords 0 (raw): the mean, a pixel of the distorted frame -- what mocap_correspond_visible(distorted = 1) takes; coords 1
 * (ideal): the mean through cv.undistortPoints' five fixed-point rounds -- a drop-in for the integer centroid in mocap_correspond
 * and mocap_correspond_visible(distorted = 0).  A point flagged EMPTY, EDGE, NEIGHBOUR or MOVING falls back to its integer
 * centroid in the coordinates asked for: (cx, cy) for coords 1, (U, V) for coords 0 -- never worse than what the caller had, and
 * never silently.  An identity slot skips both lens maps.
 *   out_xy_dev   float64 [n_images][max_blobs][2], image n at out_xy_dev + n * out_xy_stride (in doubles)
 *   out_info_dev int32 [n_images][max_blobs][2] = (S of the last window, flags), image n at + n * out_info_stride; or NULL
 * Bad arguments are MOCAP_E_INVALID, a slot without mocap_set_undistort is MOCAP_E_STATE; neither launches anything. */
enum { MOCAP_SUBPIX_EMPTY = 1, MOCAP_SUBPIX_EDGE = 2, MOCAP_SUBPIX_NEIGHBOUR = 4, MOCAP_SUBPIX_MOVING = 8, MOCAP_SUBPIX_CUT = 16 };
MOCAP_API int mocap_refine_centroids(mocap_ctx_t ctx, const void* frames_dev, int n_images, int cam_mod, int slot_base,
                                     size_t image_stride, int pitch, int pattern, int gray_shift, const int32_t* xy_dev,
                                     long xy_stride, const int32_t* count_dev, long count_stride, int max_blobs, int radius,
                                     int floor, int iters, int coords, double* out_xy_dev, long out_xy_stride,
                                     int32_t* out_info_dev, long out_info_stride, void* stream);

/* fast_cuda_demosaic(bayer) (lib/CudaOperations.py:84-100): uint8[H][W] -> uint8[H][W][3] (B,G,R) */
MOCAP_API int mocap_demosaic_u8(mocap_ctx_t ctx, const void* bayer_dev, void* bgr_dev, int height, int width, int spitch,
                      void* stream);

/* find_point_correspondance_and_object_points for T time steps (lib/Helpers.py:178-280).
 * The up-to-P points of camera c at time step t start at pts_dev + t*pt_stride_t + c*pt_stride_c (strides in
 * scalars of the point type: int32, or float64 when pts_f64; a point is 2 scalars), their number (sentinel
 * already removed) is counts_dev[t*cnt_stride_t + c*cnt_stride_c].  A dense [T][C][P][2] array has strides
 * (C*P*2, P*2) and (C, 1); centroid records gathered from other GPUs are read in place through other strides.
 * Per time step and surviving camera-0 root o (in root order):
 *   root_xyz [T][P][3]  3-D point of the root's first group          (Helpers.py:272)
 *   root_err [T][P]     mean reprojection error over its groups      (Helpers.py:273)
 *   root_grp [T][P][C][2] the first group's image points             (Helpers.py:268)
 *   root_idx [T][P]     camera-0 index of the root
 *   order    [T][P]     argsort of root_err                          (Helpers.py:274)
 *   n_roots  [T]        number of surviving roots, or MOCAP_CORR_E_* (< 0): the time step has no result.  Nothing is
 *                       ever shortened silently: counts above P or below 0 fail the step (the reference has no
 *                       capacity limits, lib/Helpers.py:191,203-245)
 * The caller applies obj_count (Helpers.py:275-279).  Requires mocap_set_cameras + mocap_set_fundamentals. */
MOCAP_API int mocap_correspond(mocap_ctx_t ctx, const void* pts_dev, long pt_stride_t, long pt_stride_c,
                     const int32_t* counts_dev, long cnt_stride_t, long cnt_stride_c, int pts_f64, int T, int C,
                     int P, double cutoff, int max_groups, double* root_xyz_dev, double* root_err_dev,
                     double* root_grp_dev, int32_t* root_idx_dev, int32_t* order_dev, int32_t* n_roots_dev,
                     void* stream);

/* Correspondence and triangulation of markers that only SOME cameras see, from any camera pair, for T time steps.  The
 * reference has no counterpart: mocap_correspond (its find_point_correspondance_and_object_points) starts from camera 0's
 * points and triangulates only groups in which no camera is missing (lib/Helpers.py:93,178-280), so it reports a marker only
 * when every camera of the rig sees it.  The contract is the definition of DESIGN.md section 2, restated by
 * tests/correspond_visible_ref.py; FP64 throughout, every operation rounded on its own.  New symbol, MOCAP_ABI_VERSION stays 7.
 * Points and counts are read through strides exactly as mocap_correspond reads them (centroid records and all-gathered
 * records work in place).  K, dist, R, t come from mocap_set_cameras; mocap_set_fundamentals is not needed: the pair matrices
 * F_ab = K_b^-T [t]x R K_a^-1 are formed on the device.
 *   distorted   0: the points are pixels of undistorted images (what mocap_blob_centroids delivers); 1: every point is first
 *               mapped to its ideal pinhole pixel (cv.undistortPoints' five fixed-point rounds).  Everything after lives in
 *               ideal pinhole pixels
 *   cutoff      a pair of points of two cameras is a seed when the second lies closer than this (px) to the first's epipolar line
 *   gate        a camera's nearest unclaimed point supports a seed when it lies closer than this (px) to the projection of the
 *               seed's two-view point
 *   min_views   fewest member cameras of an accepted marker, 2..C
 *   max_err     a hypothesis is kept when its error (mean of the squared reprojection residuals over both coordinates of all
 *               members, px^2: root_err's convention) is below this
 *   max_passes  hypotheses are sorted by (more members, smaller error, a, i, b, j) and accepted in that order when none of
 *               their points is claimed yet; passes over the points still unclaimed repeat until one accepts nothing
 *   max_hyp     1..65535: seeds one pass of one time step may hold (in LDS up to a cap, beyond it in scratch the context owns
 *               and grows on demand: calls on one context must be ordered on one stream)
 *   Q           1..65535: output rows per time step
 * Per time step, in acceptance order (more views first, then smaller error, pass by pass):
 *   xyz_dev   float64 [T][Q][3]   the DLT over the members in ascending camera order
 *   err_dev   float64 [T][Q]
 *   idx_dev   int32 [T][Q][C]     index of the member point in each camera, -1 = the camera is no member
 *   views_dev uint32 [T][Q]       bit c set: camera c is a member
 *   n_dev     int32 [T]           markers, or MOCAP_CORR_E_* (< 0): the time step has no result -- a count above P (TRUNCATED),
 *                                 a negative count (BLOB), more than max_hyp seeds in a pass (GROUPS), more than Q markers
 *                                 (OUTPUT).  Nothing is ever shortened silently; the other time steps are unaffected
 * Rows at and beyond n_dev[t] (all rows of a failed step) are UNSPECIFIED: they are not zero-filled and must not be read (a
 * step that fails in its second or a later pass has already written the rows of the passes before).
 * A combination of P and C whose points, camera table and C (C - 1) / 2 pair matrices leave no room for 64 hypotheses in a
 * workgroup's LDS is MOCAP_E_UNSUPPORTED.  Asynchronous on `stream`.  No floating-point atomics: the same call gives the same bits. */
MOCAP_API int mocap_correspond_visible(mocap_ctx_t ctx, const void* pts_dev, long pt_stride_t, long pt_stride_c,
                                       const int32_t* counts_dev, long cnt_stride_t, long cnt_stride_c, int pts_f64, int T, int C,
                                       int P, int distorted, double cutoff, double gate, int min_views, double max_err,
                                       int max_passes, int max_hyp, int Q, double* xyz_dev, double* err_dev, int32_t* idx_dev,
                                       uint32_t* views_dev, int32_t* n_dev, void* stream);

/* Marker identities across time steps.  mocap_correspond and mocap_correspond_visible report every time step's markers in an
 * order of that step alone; this call walks T time steps in order and gives every detection the identity of the track it
 * continues.  The reference has no counterpart (its {"tracker1": object_points[0]} message assumes one marker): the contract is
 * the definition of DESIGN.md section 2, restated by tests/track_ref.py -- FP64 throughout, every operation rounded on its own,
 * so the device equals the restatement bit for bit.  New symbol, MOCAP_ABI_VERSION stays 7.
 * Per step: every live slot predicts p = pos + vel; (slot, detection) is a candidate when |D - p|^2 < (gate * (1 + miss))^2;
 * candidates are accepted in ascending (d2, slot, detection) when neither side is taken; a matched slot takes vel += beta * (D - p),
 * pos = D, miss = 0, hits += 1; an unmatched one coasts (pos = p, miss += 1) and dies once miss > max_miss; then the unmatched
 * detections, in ascending row, take the lowest free slots with identity next_id++ (vel = 0, hits = 1).
 *   xyz_dev     float64 [T][Q][3]  detections (mocap_correspond_visible's xyz_dev as it is); rows at and beyond n_dev[t] take
 *                                  no part in anything and may hold any bytes
 *   n_dev       int32 [T]          detections of the step.  A negative count (MOCAP_CORR_E_*) or one above min(Q, 256) makes the
 *                                  step BLIND: it has no detections, every track coasts, status_dev[t] says why
 *   state_dev   MOCAP_TRACK_STATE_BYTES(max_tracks) bytes the caller owns: a mocap_track_header, then max_tracks mocap_track_slot.
 *               All-zero bytes are the empty tracker.  The call reads it when it starts and writes it when it ends, so calls on
 *               one state must be ordered (one stream, or events between streams); several trackers need nothing from the context
 *   max_tracks  1..256 slots;  gate finite and > 0 (world units);  beta in [0, 1];  max_miss >= 0
 *   id_dev, slot_dev, age_dev  int32 [T][Q] each: identity, slot and age (detections so far) of the track the row's detection
 *               continues or starts; -1 in all three for a detection that found no free slot or identity, and in every row at
 *               and beyond n_dev[t] (all rows of a blind step)
 *   status_dev  int32 [T]  0 or MOCAP_TRACK_E_*: nothing is silent, and the other detections and steps are unaffected
 * T = 0 is a no-op.  Bad arguments are MOCAP_E_INVALID and launch nothing.  Asynchronous on `stream`.  No atomics: the same call
 * on the same state gives the same bits. */
typedef struct mocap_track_header {
    int32_t next_id;      /* the next identity to hand out */
    int32_t reserved0;
    int64_t steps;        /* time steps seen */
    int64_t reserved[6];
} mocap_track_header;     /* 64 bytes */
typedef struct mocap_track_slot {
    double pos[3], vel[3]; /* position; velocity per time step */
    int32_t id;            /* identity */
    int32_t miss;          /* consecutive steps without a detection */
    int32_t hits;          /* detections so far */
    int32_t alive;         /* the slot holds a track (a dead slot keeps the fields of its last track) */
} mocap_track_slot;        /* 64 bytes */
#define MOCAP_TRACK_STATE_BYTES(max_tracks) (64u * (1u + (unsigned)(max_tracks)))
MOCAP_API int mocap_track_markers(mocap_ctx_t ctx, const double* xyz_dev /*[T][Q][3]*/, const int32_t* n_dev /*[T]*/,
                                  int T, int Q, void* state_dev, int max_tracks, double gate, double beta, int max_miss,
                                  int32_t* id_dev, int32_t* slot_dev, int32_t* age_dev /*[T][Q] each*/, int32_t* status_dev /*[T]*/,
                                  void* stream);

/* Rigid-body poses (6-DoF) per time step.  Each of B bodies -- 3 to 8 model points in the body's own frame -- is searched among the
 * unlabelled 3-D detections of every one of T time steps; every (time step, body) is independent (one workgroup each), the call is
 * stateless and neither needs nor changes the tracker.  The reference has no counterpart (nothing optical ever fills the four
 * orientation slots of its {"tracker1": [0, 0, 0, 0, x, y, z]} message): the contract is the definition of DESIGN.md section 2,
 * restated by tests/rigid_ref.py -- FP64 throughout, + - * / and sqrt only, every operation rounded on its own, so the device
 * equals the restatement bit for bit.  New symbol, MOCAP_ABI_VERSION stays 7.
 * Per (step, body): a model triple h = (a, b, c) with an ordered triple (i, j, k) of distinct detections is a candidate when
 * |d_ij - L_ab|, |d_jk - L_bc| and |d_ik - L_ac| are all below tol; each candidate is posed by Horn's closed-form quaternion from
 * its three pairs; the model points, in ascending order, take the nearest unclaimed detection within gate of where the pose puts
 * them (ties: the lower row); with at least min_markers such inliers the pose is refitted once over all of them (no re-labelling)
 * and rms^2 is the mean squared distance after the refit; the result is the candidate smallest in the total order (more inliers,
 * smaller rms^2, h, i, j, k).  Bodies do not know of each other: two bodies may claim the same detection.
 *   xyz_dev       float64 [T][Q][3]  detections (mocap_correspond_visible's xyz_dev as it is); rows at and beyond n_dev[t] take no
 *                                    part and may hold any bytes; the rows below it must be finite
 *   n_dev         int32 [T]          detections of the step.  Negative (MOCAP_CORR_E_*): MOCAP_RIGID_E_BLIND for every body; above
 *                                    min(Q, 64): MOCAP_RIGID_E_CAPACITY for every body
 *   model_dev     float64 [B][8][3]  model points, the first n_markers_dev[b] (3..8) of each body
 *   tri_dev       int32 [B][56][3]   model triples a < b < c, the first n_tri_dev[b] (1..56) of each body: the caller lists those
 *                                    whose triangle is not degenerate
 *   tol, gate     finite and > 0 (world units);  min_markers 3..8;  max_hyp 1..4096: more candidates are MOCAP_RIGID_E_HYP for
 *                 that body in that step -- the list is never shortened -- and leave the other bodies and steps as they are
 *   R_dev [T][B][9] (row-major, D = R m + t), t_dev [T][B][3], q_dev [T][B][4] (w, x, y, z; unit, first non-zero component
 *   positive), rms_dev [T][B], n_in_dev int32 [T][B], label_dev int32 [T][B][8] (the detection row of each model point or -1; -1
 *   from n_markers on), status_dev int32 [T][B]: 0, MOCAP_RIGID_LOST or MOCAP_RIGID_E_*.  On any status other than 0, n_in is 0,
 *   the labels are -1, and the floats are unspecified and must not be read.
 * T = 0 or B = 0 is a no-op.  Bad arguments (B above 16 among them) are MOCAP_E_INVALID and launch nothing.  Asynchronous on
 * `stream`.  No floating-point atomics, and the winner does not depend on the order the lanes found the candidates in: the same
 * call gives the same bits. */
#define MOCAP_RIGID_MAX_DETECTIONS 64
#define MOCAP_RIGID_MAX_MARKERS 8
#define MOCAP_RIGID_MAX_TRIPLES 56
#define MOCAP_RIGID_MAX_BODIES 16
#define MOCAP_RIGID_MAX_HYP 4096
MOCAP_API int mocap_rigid_poses(mocap_ctx_t ctx, const double* xyz_dev /*[T][Q][3]*/, const int32_t* n_dev /*[T]*/, int T, int Q,
                                int B, const double* model_dev /*[B][8][3]*/, const int32_t* n_markers_dev /*[B]*/,
                                const int32_t* tri_dev /*[B][56][3]*/, const int32_t* n_tri_dev /*[B]*/, double tol, double gate,
                                int min_markers, int max_hyp, double* R_dev, double* t_dev, double* q_dev, double* rms_dev,
                                int32_t* n_in_dev, int32_t* label_dev, int32_t* status_dev, void* stream);

/* Refinement of triangulated markers by their reprojection error, with the covariance of the result.  mocap_correspond and
 * mocap_correspond_visible report the DLT, which minimises an algebraic error that weights every view by its depth; this call
 * moves every row's point to the minimum of 1/2 sum |pixel(X) - observation|^2 over the row's member cameras by
 * Levenberg-Marquardt, and reports (J^T J)^-1 there: the point's covariance in world units^2 per px^2 of image noise.  Every
 * (time step, row) is independent (one lane each) and the call is stateless.  The reference has no counterpart: the contract is
 * the definition of DESIGN.md section 2, restated by tests/refine_points_ref.py -- FP64 throughout, + - * / only, every operation
 * rounded on its own, sums in ascending camera order, so the device equals the restatement bit for bit.  New symbol,
 * MOCAP_ABI_VERSION stays 7.
 *   xyz_dev     float64 [T][Q][3]  the points to start from (mocap_correspond_visible's xyz_dev, mocap_correspond's root_xyz)
 *   n_dev       int32 [T]          rows of the step (the correspondence's n / n_roots as it is).  n_dev[t] <= 0: the step has no
 *                                  rows; above Q: Q rows
 *   views_dev   uint32 [T][Q]      bit c set: camera c is a member of the row.  NULL (grouped form only): all C cameras are
 *   Camera c's observation of row (t, q) comes from one of two sources -- exactly one of pts_dev and grp_dev is not NULL:
 *   indexed     point idx_dev[t][q][c] (int32 [T][Q][C]; read for members only) of camera c's list at time step t; the lists
 *               are read through pt_stride_t / pt_stride_c / pts_f64 exactly as mocap_correspond_visible reads them (P = points
 *               a list holds), so centroid records and all-gathered records work in place
 *   grouped     grp_dev[t][q][c], float64 [T][Q][C][2]: mocap_correspond's root_grp as it is
 *   distorted   0: the observations are ideal pinhole pixels (pixels of undistorted images), the model is fx x + cx exactly;
 *               1: they are pixels of the raw frames and the residual is taken there, through the camera's lens (k1, k2, p1, p2,
 *               k3 of mocap_set_cameras) -- no undistortion is involved
 *   max_iters (1..10000), ftol (>= 0), lambda0 (0 < lambda0 <= 1e16): the loop's limits, as mocap_rig_bundle_adjust's; the step
 *               control (gain ratio, Nielsen's damping, the four stops) is the one the rig solvers use
 *   max_res2    > 0 turns pruning on: after a loop has stopped, while the row has more than min_views (2..C) members and has
 *               dropped fewer than max_drop (>= 0), the member with the largest squared residual length r0^2 + r1^2 (px^2; ties:
 *               the lower camera) is dropped when that length exceeds max_res2, and a new loop starts from the current point
 *               with lambda0.  <= 0: no pruning
 * Per row q < n_dev[t]:
 *   xyz_out_dev float64 [T][Q][3]  the refined point (may be xyz_dev itself)
 *   err_dev     float64 [T][Q]     mean of the squared residuals over both coordinates of all members left, px^2 (err_dev's
 *                                  convention in mocap_correspond_visible)
 *   res2_dev    float64 [T][Q][C]  r0^2 + r1^2 of every member left, -1 for a camera that is none
 *   cov_dev     float64 [T][Q][6]  (J^T J)^-1 at the refined point, undamped: upper triangle (00, 01, 02, 11, 12, 22)
 *   views_out_dev, dropped_dev uint32 [T][Q]  the members left, the members dropped
 *   iters_dev   int32 [T][Q]       iterations of all the row's loops
 *   status_dev  int32 [T][Q]       MOCAP_RIG_STOP_* (1..4) of the last loop, or MOCAP_REFINE_E_* (< 0): the row was not refined,
 *                                  xyz_out holds the point handed in, views_out the mask handed in, and the row's other outputs
 *                                  are unspecified.  Nothing is silent, and the other rows are unaffected
 * Rows at and beyond n_dev[t] get status 0 and nothing else is written for them.
 * T = 0 is a no-op.  Bad arguments (C above 32 among them) are MOCAP_E_INVALID and launch nothing.  Requires mocap_set_cameras.
 * Asynchronous on `stream`.  No atomics: the same call gives the same bits. */
MOCAP_API int mocap_refine_points(mocap_ctx_t ctx, const double* xyz_dev, const int32_t* n_dev, const uint32_t* views_dev, int T,
                                  int Q, int C, const void* pts_dev, long pt_stride_t, long pt_stride_c, int pts_f64, int P,
                                  const int32_t* idx_dev, const double* grp_dev, int distorted, int max_iters, double ftol,
                                  double lambda0, double max_res2, int min_views, int max_drop, double* xyz_out_dev,
                                  double* err_dev, double* res2_dev, double* cov_dev, uint32_t* views_out_dev,
                                  uint32_t* dropped_dev, int32_t* iters_dev, int32_t* status_dev, void* stream);

/* The scoring step of find_point_correspondance_and_object_points on its own (lib/Helpers.py:205-220), for one camera
 * pair: the epipolar line of every root point under Fs[f_index] (cv.computeCorrespondEpilines on the float32 point, :207;
 * line coefficients normalised in FP64, rounded to float32) and the distance of every candidate point of camera
 * f_index + 1 to it by the expression of :217, evaluated in FP64 -- the very device functions mocap_correspond scores with.
 * roots_dev [n_roots][2], cand_dev [n_cand][2] (int32, or float64 when pts_f64) -> dist_dev [n_roots][n_cand] float64;
 * lines_dev (optional, may be NULL) [n_roots][3] float32 = (a, b, c).  The caller applies the cutoff (< 10, :219).
 * Requires mocap_set_fundamentals. */
MOCAP_API int mocap_epipolar_scores(mocap_ctx_t ctx, const void* roots_dev, int n_roots, const void* cand_dev, int n_cand,
                                    int pts_f64, int f_index, double* dist_dev, float* lines_dev, void* stream);

/* triangulate_point(s) over N groups (lib/Helpers.py:43-99).  pts_dev [N][C][2] float64, valid_dev [N][C]
 * (0 = [None, None]).  compact_k != 0 reproduces the reference's indexing of the intrinsics by position after
 * the None entries are dropped (:59-61).  ok_dev[n] = 0 where the reference returns [None, None, None]. */
MOCAP_API int mocap_triangulate_batch(mocap_ctx_t ctx, const double* pts_dev, const uint8_t* valid_dev, int N, int C,
                            int compact_k, double* xyz_dev, int32_t* ok_dev, void* stream);
/* calculate_reprojection_error over N (group, object point) pairs (lib/Helpers.py:113-143);
 * ok_dev[n] = 0 where the reference returns None. */
MOCAP_API int mocap_reproject_batch(mocap_ctx_t ctx, const double* pts_dev, const uint8_t* valid_dev, const double* xyz_dev,
                          int N, int C, int compact_k, double* mse_dev, int32_t* ok_dev, void* stream);

/* bundle_adjustment's residual_function (lib/Helpers.py:161-167) with params_to_camera_poses (:145-156) for B parameter
 * vectors in ONE launch: camera 0 at the origin, cameras 1..C-1 from (rotation vector, t) sextuples
 * (Rotation.from_rotvec(.).as_matrix() on the device), every group triangulated from its C views (groups holding a
 * [None, None] are skipped, :93), reprojected into them, per-point MSE cast to float32 (:165); groups and object points are
 * paired positionally as the reference's zip does (:104).  The image points stay resident: pts_dev [N][C][2] float64 and
 * valid_dev [N][C] are device buffers the caller uploads once per problem; K and dist come from mocap_set_cameras.
 * params_host [B][6 (C - 1)], residuals_host [B][N] and counts_host [B] (residuals per vector, <= N) are HOST arrays: the
 * library hands them over through one pinned block the kernel reads and writes directly, so an evaluation costs one launch
 * and one stream wait.  Synchronous.  SciPy's least_squares stays the driver, as in the reference; a forward-difference
 * Jacobian is one call with B = 1 + 6 (C - 1). */
MOCAP_API int mocap_ba_residuals(mocap_ctx_t ctx, const double* params_host, int B, const double* pts_dev,
                                 const uint8_t* valid_dev, int N, int C, float* residuals_host, int32_t* counts_host,
                                 void* stream);

/* cv.findFundamentalMat(p1, p2, cv.FM_RANSAC, threshold, .) (CalculateCameraPoses.py:189) for n_pairs camera pairs in one
 * call.  Not OpenCV's random sequence nor its 7-point solver: the definition of DESIGN.md section 2 (FP64 throughout).
 * The caller draws the samples: hypothesis h of pair p is the normalised 8-point solve (Hartley normalisation, smallest
 * eigenvector of A^T A, rank 2, unit Frobenius norm) over the 8 distinct points samples[p][h][0..7]; a point is an inlier
 * iff the larger of its two squared point-to-epipolar-line distances is <= threshold^2; the valid hypothesis with the most
 * inliers wins, the lowest index on ties.
 *   pts_a_dev, pts_b_dev  float64 [total][2]: the pairs' point lists one after another (a: first camera, b: second;
 *                         x_b^T F x_a = 0)
 *   pair_offset_host      int32 [n_pairs + 1] HOST array, copied before the call returns: pair p owns points
 *                         offset[p] .. offset[p + 1] - 1; at least 8 points per pair
 *   samples_dev, H        int32 [n_pairs][H][8], indices local to the pair
 *   refit                 != 0: F_refit_dev receives the 8-point solve over all inliers of the winner (the mask is NOT
 *                         recomputed under it); 0: F_refit_dev is not written and may be NULL
 *   F_sample_dev, F_refit_dev  float64 [n_pairs][9] row-major, unit norm; not written for a failed pair
 *   inlier_dev            uint8 [total]: 1 = inlier of its pair's winner (0 everywhere in a failed pair)
 *   status_dev            int32 [n_pairs][2] = (winning hypothesis, its inlier count), or (MOCAP_FUND_E_* < 0, 0): the pair
 *                         has no result.  Nothing is ever returned silently wrong
 *   counts_dev            int32 [n_pairs][H] inliers of every hypothesis (0 for an invalid one), or NULL (tests, tuning)
 * Asynchronous on `stream`.  The hypotheses' matrices and counters live in scratch the context owns and grows on demand:
 * calls on one context must be ordered on one stream.  A pair's results do not depend on the rest of the batch. */
MOCAP_API int mocap_fundamental_ransac(mocap_ctx_t ctx, int n_pairs, const double* pts_a_dev, const double* pts_b_dev,
                                       const int32_t* pair_offset_host, const int32_t* samples_dev, int H, double threshold,
                                       int refit, double* F_sample_dev, double* F_refit_dev, uint8_t* inlier_dev,
                                       int32_t* status_dev, int32_t* counts_dev, void* stream);

/* Bundle adjustment of a whole rig: the poses of cameras 1..C-1 and all N 3-D points, over exactly the observations that
 * exist, by sparse Levenberg-Marquardt on the device (Schur complement on the points, analytic Jacobian, Nielsen's damping
 * rule; FP64 throughout; definition in DESIGN.md section 2, restated by tests/rig_ba_ref.py).  Generalises the interface of
 * lib/Helpers.py:158-176 (bundle_adjustment: two cameras, SciPy over 6 parameters, points every camera must have seen); the
 * reference has no N-camera counterpart.  Both entries were added without a change to any existing one, so
 * MOCAP_ABI_VERSION stays 7: a caller built against the earlier header runs unchanged.
 *   C, N, n_obs           2..32 cameras, N points, n_obs observations
 *   obs_offset_dev        int32 [N + 1]: point n owns observations obs_offset[n] .. obs_offset[n + 1] - 1; obs_offset[0] = 0,
 *                         obs_offset[N] = n_obs; every point has 2..C observations
 *   obs_cam_dev           int32 [n_obs]: the TRUE camera number of each observation (K and dist of mocap_set_cameras are
 *                         indexed with it), strictly ascending within a point
 *   obs_uv_dev            float64 [n_obs][2] pixels, distorted as the camera delivers them
 *   poses_dev             float64 [C][12] in / out: R row-major then t, world -> camera; camera 0 is taken as identity, zero
 *   points_dev            float64 [N][3] in / out
 *   max_iters, ftol, lambda0  the stopping rules and the first damping (50, 1e-12, 1e-3 in the Python surface)
 *   history_dev           float64 [max_iters][4], one row per iteration done: cost after it, the lambda it was solved with,
 *                         1 = accepted, length of the step; rows of iterations not done are zero
 *   result_dev            float64 [4]: status, iterations done, cost of the state handed in, final cost (1/2 sum r^2).
 *                         status > 0 names the rule that stopped the loop (MOCAP_RIG_STOP_*); status < 0 (MOCAP_RIG_E_*):
 *                         poses_dev and points_dev are left as they were.  Nothing is ever returned silently wrong
 * On return every t and every point is scaled so that |t_1| is what it was on entry (the scale is free while iterating).
 * Asynchronous on `stream`: all max_iters iterations are enqueued, the kernels of the iterations after the stop return at
 * once, and no array of the iteration crosses to the host.  No floating-point atomics: the same call gives the same bits.
 * The scratch belongs to the context and grows on demand: calls on one context must be ordered on one stream. */
enum {
    MOCAP_RIG_STOP_MAX_ITERS = 1, /* max_iters iterations done */
    MOCAP_RIG_STOP_FTOL = 2,      /* an accepted step lowered the cost by less than ftol, relatively */
    MOCAP_RIG_STOP_LAMBDA = 3,    /* the damping grew beyond 1e16 */
    MOCAP_RIG_STOP_CHOLESKY = 4,  /* the reduced camera matrix was not positive definite twice in a row (once: the step counts as rejected) */
    MOCAP_RIG_E_LAYOUT = -2,      /* the observation arrays break one of the rules above */
    MOCAP_RIG_E_BEHIND = -3       /* in the state handed in, a point is not in front of a camera that sees it, or the cost is not finite */
};
MOCAP_API int mocap_rig_bundle_adjust(mocap_ctx_t ctx, int C, int N, int n_obs, const int32_t* obs_offset_dev,
                                      const int32_t* obs_cam_dev, const double* obs_uv_dev, double* poses_dev, double* points_dev,
                                      int max_iters, double ftol, double lambda0, double* history_dev, double* result_dev,
                                      void* stream);
/* The pieces of one iteration of mocap_rig_bundle_adjust at a given state and damping, for tests and tuning (the residual
 * and Jacobian of lib/Helpers.py:158-176's problem, generalised as above, in normal-equation form): cost_dev [1] = 1/2 sum
 * r^2; gradient_dev [6 (C - 1) + 3 N] = J^T r (cameras 1.., 6 each: rotation, translation; then the points);
 * S_dev [6 (C - 1)][6 (C - 1)] the damped reduced camera matrix U* - sum_n W_n V*_n^-1 W_n^T; rhs_dev [6 (C - 1)] the
 * reduced right-hand side -g_c + sum_n W_n V*_n^-1 g_n; status_dev int32 [2] = (layout error, a point not in front of a
 * camera that sees it), both 0 when all is well.  poses_dev and points_dev are only read.  Asynchronous on `stream`. */
MOCAP_API int mocap_rig_linearize(mocap_ctx_t ctx, int C, int N, int n_obs, const int32_t* obs_offset_dev,
                                  const int32_t* obs_cam_dev, const double* obs_uv_dev, const double* poses_dev,
                                  const double* points_dev, double lambda, double* cost_dev, double* gradient_dev, double* S_dev,
                                  double* rhs_dev, int32_t* status_dev, void* stream);

/* The two entries above with a robust loss on the observations (wand captures carry ghost reflections and wrong-blob picks
 * that no RANSAC mask reaches once the adjustment runs); new symbols, MOCAP_ABI_VERSION stays 7, the entries above keep their
 * signatures and results.  Per observation with residual r: s = rx^2 + ry^2.  MOCAP_RIG_LOSS_CAUCHY with loss_scale = c
 * (pixels, a few sigma of the pixel noise): rho(s) = c^2 log1p(s / c^2), weight w = 1 / (1 + s / c^2), cost 1/2 sum rho;
 * the linearisation is first order (iteratively reweighted: r and the Jacobian rows of the observation times sqrt(w)), the
 * step control is unchanged (restated by tests/rig_robust_ref.py).  MOCAP_RIG_LOSS_NONE is the
 * definition above, bit for bit; loss_scale is then ignored.  Any other loss, or with Cauchy a loss_scale that is not finite
 * or not > 0, is MOCAP_E_INVALID and nothing is launched.
 *   obs_err_dev           float64 [n_obs] or NULL: the length |r| of every observation's UNWEIGHTED residual at the returned state
 *   obs_weight_dev        float64 [n_obs] or NULL: the weight w there (1 for MOCAP_RIG_LOSS_NONE)
 * Both are zero when the status is negative.  Every other argument, the history, the result (costs are 1/2 sum rho) and the
 * rules on streams and scratch are mocap_rig_bundle_adjust's and mocap_rig_linearize's (cost_dev: 1/2 sum rho; gradient, S
 * and rhs from the weighted blocks). */
enum { MOCAP_RIG_LOSS_NONE = 0, MOCAP_RIG_LOSS_CAUCHY = 1 };
MOCAP_API int mocap_rig_bundle_adjust_robust(mocap_ctx_t ctx, int C, int N, int n_obs, const int32_t* obs_offset_dev,
                                             const int32_t* obs_cam_dev, const double* obs_uv_dev, double* poses_dev,
                                             double* points_dev, int max_iters, double ftol, double lambda0, double* history_dev,
                                             double* result_dev, int loss, double loss_scale, double* obs_err_dev,
                                             double* obs_weight_dev, void* stream);
MOCAP_API int mocap_rig_linearize_robust(mocap_ctx_t ctx, int C, int N, int n_obs, const int32_t* obs_offset_dev,
                                         const int32_t* obs_cam_dev, const double* obs_uv_dev, const double* poses_dev,
                                         const double* points_dev, double lambda, double* cost_dev, double* gradient_dev,
                                         double* S_dev, double* rhs_dev, int32_t* status_dev, int loss, double loss_scale,
                                         void* stream);

/* mocap_rig_bundle_adjust_robust with the cameras' lenses among the unknowns: a wand capture, thousands of points through the
 * whole volume seen by many cameras, constrains them far better than the board views mocap_intrinsics_calibrate had (new
 * symbols, MOCAP_ABI_VERSION stays 7; definition in DESIGN.md section 2, restated by tests/rig_selfcal_ref.py).  Every camera,
 * camera 0 included, gains kd = (fx, fy, cx, cy, k1, k2, p1, p2, k3), in mocap_intrinsics_calibrate's order; a camera's block
 * is 15 wide, kd's 9 then the pose's 6, and the reduced system 15 C square.  K and dist of mocap_set_cameras are neither read
 * nor changed, and no cameras need to be set.
 *   kd_dev                float64 [C][9] in / out
 *   refine_mask_host      int32 [C], HOST, copied before the call returns: bit i set = parameter i of kd is free for that
 *                         camera.  A fixed parameter comes back with the bits it had.  Mask 0 for every camera is
 *                         mocap_rig_bundle_adjust_robust's problem at the lenses kd_dev holds
 * A mask with bits above 8, or a kd entry that is not finite or an fx, fy <= 0, is MOCAP_E_INVALID and nothing is launched
 * (kd_dev is read back for the check: the call waits for `stream` once, before it enqueues anything).  A camera whose mask is
 * not 0 needs at least twice as many observations as its mask has bits, else the status is MOCAP_RIG_E_LAYOUT.  A negative
 * status leaves kd_dev, poses_dev and points_dev as they were.  Every other argument, the history, the result, the gauge on
 * return and the rules on streams and scratch are mocap_rig_bundle_adjust_robust's.
 * mocap_rig_linearize_intrinsics, for tests: the pieces of one iteration as mocap_rig_linearize_robust's, with gradient_dev
 * [15 C + 3 N] (the cameras' 15 each, camera 0 first; then the points), S_dev [15 C][15 C] and rhs_dev [15 C].  A fixed
 * parameter's row and column of S are zero but for a 1 on the diagonal, its gradient and rhs entries are 0. */
MOCAP_API int mocap_rig_bundle_adjust_intrinsics(mocap_ctx_t ctx, int C, int N, int n_obs, const int32_t* obs_offset_dev,
                                                 const int32_t* obs_cam_dev, const double* obs_uv_dev, double* kd_dev,
                                                 const int32_t* refine_mask_host, double* poses_dev, double* points_dev,
                                                 int max_iters, double ftol, double lambda0, double* history_dev,
                                                 double* result_dev, int loss, double loss_scale, double* obs_err_dev,
                                                 double* obs_weight_dev, void* stream);
MOCAP_API int mocap_rig_linearize_intrinsics(mocap_ctx_t ctx, int C, int N, int n_obs, const int32_t* obs_offset_dev,
                                             const int32_t* obs_cam_dev, const double* obs_uv_dev, const double* kd_dev,
                                             const int32_t* refine_mask_host, const double* poses_dev, const double* points_dev,
                                             double lambda, double* cost_dev, double* gradient_dev, double* S_dev, double* rhs_dev,
                                             int32_t* status_dev, int loss, double loss_scale, void* stream);

/* Intrinsic calibration of every camera of a rig from planar-board corner lists: per camera fx, fy, cx, cy, k1, k2, p1, p2, k3
 * and one board -> camera pose per view, by Levenberg-Marquardt on the device (Schur complement on the views, analytic
 * Jacobian, Marquardt scaling, Nielsen's damping rule; FP64 throughout; definition in DESIGN.md section 2, restated by
 * tests/intrinsics_ref.py).  Replaces reference CalculateCameraIntrinsic.py:58, cv2.calibrateCamera(objpoints, imgpoints,
 * size, None, None), for all cameras in one call; corner detection stays with the caller.  Both entries were added without a
 * change to any existing one, so MOCAP_ABI_VERSION stays 7.
 *   n_cams                cameras, 1..65536
 *   view_offset_host      int32 [n_cams + 1], HOST: camera c owns views view_offset[c] .. view_offset[c + 1] - 1, from 0,
 *                         not descending; n_views = view_offset[n_cams] (at most 2^20)
 *   point_offset_host     int32 [n_views + 1], HOST: view v owns points point_offset[v] .. point_offset[v + 1] - 1, from 0,
 *                         not descending; total = point_offset[n_views] (at most 2^26).  Both are copied before the call returns
 *   obj_xy_dev            float64 [total][2] board coordinates (X, Y) of every corner, Z = 0
 *   img_uv_dev            float64 [total][2] their pixels
 *   image_size_host       int32 [n_cams][2], HOST: width, height (the initialisation's principal point is ((w - 1) / 2,
 *                         (h - 1) / 2)); may be null with have_start
 *   have_start            0: kd_dev and view_poses_dev are outputs, the start is the definition's initialisation;
 *                         1: they hold the start
 *   max_iters, ftol, lambda0  the stopping rules and the first damping (50, 1e-12, 1e-3 in the Python surface)
 *   kd_dev                float64 [n_cams][9] in / out: fx, fy, cx, cy, k1, k2, p1, p2, k3
 *   view_poses_dev        float64 [n_views][12] in / out: R row-major then t, board -> camera
 *   view_rms_dev          float64 [n_views]: sqrt(sum r^2 of the view / its points), NaN for a failed camera
 *   history_dev           float64 [n_cams][max_iters][4], per camera as mocap_rig_bundle_adjust's
 *   result_dev            float64 [n_cams][4]: status, iterations done, cost at the start (handed in or initialised), final
 *                         cost (1/2 sum r^2 over the camera's points; OpenCV's return value is sqrt(2 cost / points)).
 *                         status > 0: MOCAP_RIG_STOP_*; status < 0: MOCAP_INTR_E_*, and that camera's kd and poses are left
 *                         as they were.  Every camera has its own damping, stop and status: a finished or failed camera
 *                         changes nothing in another, and a camera's results are the bits it gives when calibrated alone
 * A camera needs at least 3 views, a view at least 4 points, and the camera at least as many equations as unknowns, 2 points
 * >= 9 + 6 views (3 views of 4 points fall short: 24 for 27), else the camera reports MOCAP_INTR_E_LAYOUT.  Offsets that
 * descend or sizes outside the ranges are bad arguments (MOCAP_E_INVALID).
 * Asynchronous on `stream`: all max_iters iterations are enqueued (four launches each), the kernels of a camera that has
 * stopped return at once, and no array of the iteration crosses to the host.  No floating-point atomics: the same call gives
 * the same bits.  The scratch belongs to the context and grows on demand: calls on one context must be ordered on one stream. */
enum {
    MOCAP_INTR_E_LAYOUT = -2,     /* fewer than 3 views, a view with fewer than 4 points, or 2 points < 9 + 6 views */
    MOCAP_INTR_E_BEHIND = -3,     /* in the start state a point is not in front of its view's camera, or the cost is not finite */
    MOCAP_INTR_E_DEGENERATE = -4  /* the initialisation cannot tell the focal lengths apart from the views' distances (all views
                                     fronto-parallel, for one): 2x2 determinant <= 1e-10 (trace / 2)^2, or a solution not positive */
};
MOCAP_API int mocap_intrinsics_calibrate(mocap_ctx_t ctx, int n_cams, const int32_t* view_offset_host,
                                         const int32_t* point_offset_host, const double* obj_xy_dev, const double* img_uv_dev,
                                         const int32_t* image_size_host, int have_start, int max_iters, double ftol,
                                         double lambda0, double* kd_dev, double* view_poses_dev, double* view_rms_dev,
                                         double* history_dev, double* result_dev, void* stream);
/* The pieces of one iteration of mocap_intrinsics_calibrate at a given state and damping, for tests: cost_dev [n_cams] = 1/2
 * sum r^2; gradient_dev [9 n_cams + 6 n_views] = J^T r (the cameras' 9 each, then the views' 6 each: rotation, translation);
 * S_dev [n_cams][81] the damped reduced camera matrix U* - sum_v W_v V*_v^-1 W_v^T; rhs_dev [n_cams][9] the reduced
 * right-hand side -g_c + sum_v W_v V*_v^-1 g_v; status_dev int32 [n_cams][2] = (layout error, a point not in front of its
 * view's camera).  The entries of a camera with a layout error are zero.  kd_dev and view_poses_dev are only read.
 * Asynchronous on `stream`. */
MOCAP_API int mocap_intrinsics_linearize(mocap_ctx_t ctx, int n_cams, const int32_t* view_offset_host,
                                         const int32_t* point_offset_host, const double* obj_xy_dev, const double* img_uv_dev,
                                         const double* kd_dev, const double* view_poses_dev, double lambda, double* cost_dev,
                                         double* gradient_dev, double* S_dev, double* rhs_dev, int32_t* status_dev, void* stream);

/* The path's one exchange step: with the cameras sharded over GPUs (one process per GPU), every rank
 * contributes the fixed-size centroid records of its images and receives all ranks' records, in rank order, before
 * correspondence -- one ncclAllGather (RCCL over xGMI) per batch.  The reference has no counterpart: its camera
 * threads hand their image points to the `track` thread through queue.Queue (RealtimeTracking_FLIR.py:107-113,
 * 180-183, 304-312); this is that hand-off across GPUs.  librccl is bound at run time (dlopen), so single-GPU users
 * do not need it.
 *   mocap_comm_unique_id  rank 0 obtains MOCAP_COMM_ID_BYTES opaque bytes (ncclGetUniqueId) and hands them to the
 *                         other ranks by any host-side means (file, socket, MPI, torch.distributed store ...);
 *   mocap_comm_available  0 when librccl can be loaded in this process (no communication: a local check every rank makes
 *                         BEFORE any rank enters the collective mocap_comm_init, so that all take the same road);
 *   mocap_comm_init       every rank, collectively: creates a communicator (ncclCommInitRank) on the context's device;
 *   mocap_comm_share      local: lets another context of the same rank and device (another batch in flight, with its own
 *                         HIP stream) use src's communicator -- ONE communicator per rank; the library orders the
 *                         all-gathers issued through it with an event chain, whatever streams they run on;
 *   mocap_allgather_centroids  asynchronous on `stream`: local_records_dev [ints_per_rank] int32 of every rank
 *                         -> gathered_dev [world][ints_per_rank] on every rank (the records mocap_blob_centroids
 *                         wrote; mocap_correspond then reads them in place through its strides);
 *   mocap_comm_destroy    drops the context's reference; the communicator goes with its last user (mocap_ctx_destroy
 *                         does this too). */
#define MOCAP_COMM_ID_BYTES 128
MOCAP_API int mocap_comm_unique_id(void* id_out /*[MOCAP_COMM_ID_BYTES]*/);
MOCAP_API int mocap_comm_available(void);
MOCAP_API int mocap_comm_init(mocap_ctx_t ctx, const void* id /*[MOCAP_COMM_ID_BYTES]*/, int rank, int world);
MOCAP_API int mocap_comm_share(mocap_ctx_t dst, mocap_ctx_t src);
MOCAP_API int mocap_comm_destroy(mocap_ctx_t ctx);
MOCAP_API int mocap_allgather_centroids(mocap_ctx_t ctx, const int32_t* local_records_dev, int32_t* gathered_dev,
                                        long ints_per_rank, void* stream);

/* Dark-tile early-out of the filter stage: one streaming kernel sums the excess max(0, p - 63) of every 8x8 cell of the
 * frames; a filter tile whose source region provably cannot produce a set mask bit (bound in DESIGN.md 4.1) is then
 * answered with zeros without reading its pixels again.  Results are identical either way; MOCAP_SKIP_DARK=0
 * disables it.  mocap_tile_stats: number of (strip, chunk) tiles of the most recent batch and how many of them were
 * resolved that way.  Synchronises the device. */
MOCAP_API int mocap_tile_stats(mocap_ctx_t ctx, uint64_t* tiles, uint64_t* skipped);
/* The work lists the sparse path made of the most recent batch (any entry point that filters): items of the box kernel,
 * entries of the wide-tile list, and wide tiles that were cut at their empty columns into items instead (wide_split: 0 = never,
 * 2 = always, 1 = unless the context's last probe found the scene crowded; the default).  All 0
 * when the batch took the dense path.  Any pointer may be null.  Synchronises the device. */
MOCAP_API int mocap_list_stats(mocap_ctx_t ctx, uint32_t* items, uint32_t* wide, uint32_t* split);
/* The context's own mask, read back for tests: the first n_images images of the mask mocap_blob_centroids (and its Bayer form)
 * filters into, as the row-major mask of mocap_filter_mask ([n_images][height][ceil(width/32)] uint32; mask_dev zero-initialised by
 * the caller).  That mask is never zeroed between batches.  The invariant it must keep, and this call exposes: after a batch every
 * image of it is exactly that batch's filtered image -- zero outside the regions the batch's tiles recorded, whatever an earlier
 * batch wrote there -- and the images beyond the batch still are what the last batch that held them left.  Reads only (no state of
 * the context changes), ordered on `stream`, does not synchronise.  MOCAP_E_INVALID: n_images < 1, a null pointer, or more
 * images than the own mask holds (0 before the first batch). */
MOCAP_API int mocap_own_mask(mocap_ctx_t ctx, int n_images, uint32_t* mask_dev, void* stream);
/* HIP-event timing of the kernels launched by mocap_blob_centroids / mocap_filter_mask / mocap_correspond / mocap_correspond_visible, recorded
 * on their stream.  mocap_profile_read synchronises, returns accumulated milliseconds and launch counts and resets:
 * index 0 = box_filter_kernel (or the general filter_mask_kernel), 1 = contours_kernel, 2 = correspond_kernel and
 * correspond_visible_kernel,
 * 3 = bright_cells_kernel, 4 = settle_tiles_kernel. */
MOCAP_API int mocap_profile_enable(mocap_ctx_t ctx, int on);
MOCAP_API int mocap_profile_read(mocap_ctx_t ctx, double ms[5], int launches[5]);

#ifdef __cplusplus
}
#endif
#endif /* MOCAP_HIP_H */
