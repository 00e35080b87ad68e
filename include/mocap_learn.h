/*
 * mocap_learn.h -- C-ABI of libmocap_learn.so: rigid-body models learned from a tracked capture, on the MI355X (gfx950).
 *
 * A library of its own beside libmocap_hip.so (include/mocap_hip.h), whose ABI -- version 7, its declarations and its exports --
 * stays exactly as it was: a caller that only tracks loads nothing new.  The two share no state.  This one needs no context: it
 * is told the device, keeps nothing between calls and allocates nothing.
 *
 * Plain C, pointers and sizes only.  Every entry point returns 0 on success or a negative MOCAP_LEARN_E_* code;
 * mocap_learn_last_error() returns a thread-local description.  `*_dev` arguments are raw HIP device pointers supplied by the
 * caller, `stream` is a hipStream_t passed as void* (NULL = the default stream).  All work is enqueued on `stream`.
 */
#ifndef MOCAP_LEARN_H
#define MOCAP_LEARN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MOCAP_LEARN_ABI_VERSION 1
#define MOCAP_LEARN_API __attribute__((visibility("default")))

enum {
    MOCAP_LEARN_OK = 0,
    MOCAP_LEARN_E_INVALID = -1,    /* bad argument */
    MOCAP_LEARN_E_HIP = -2         /* a HIP runtime call failed */
};
/* per-group status of mocap_learn_rigid_bodies */
enum {
    MOCAP_LEARN_E_MEMBERS = -2,    /* status[g]: n_members outside 3..8 or below min_present, or members that are negative or repeated */
    MOCAP_LEARN_E_INCOMPLETE = -3  /* no step of the take shows every member of the group: it has no reference step */
};

MOCAP_LEARN_API int mocap_learn_abi_version(void);
MOCAP_LEARN_API const char* mocap_learn_last_error(void);

/* Rigid-body models learned from a tracked capture: the two calls between mocap_track_markers and mocap_rigid_poses.  Wave the
 * objects through the volume; the identities that keep their mutual distances are a body (mocap_learn_marker_pair_stats gives the
 * caller the table to group them by), and the body's model is its shape averaged over the take (mocap_learn_rigid_bodies).  The
 * reference has no counterpart: the contract is the definition of DESIGN.md section 2, restated by tests/rigid_learn_ref.py -- FP64
 * throughout, + - * / and sqrt only, every operation rounded on its own, so the device equals the restatement bit for bit.
 * Common to both:
 *   xyz_dev  float64 [T][Q][3], n_dev int32 [T], id_dev int32 [T][Q]: the markers, their counts and mocap_track_markers' identities
 *            as they are (-1 = the row has no track).  A step is BLIND when n_dev[t] < 0 or n_dev[t] > Q and is skipped everywhere.
 *            Rows at and beyond n_dev[t] take no part and may hold any bytes.  Identity i is PRESENT in step t at the lowest row
 *            r < n_dev[t] with id_dev[t][r] == i.
 *   Every sum over time is formed per chunk of MOCAP_LEARN_CHUNK = 32 steps (t in [32 c, 32 c + 32)) in ascending t, starting from
 *   0, and the totals add the chunks' partial sums in ascending c.
 *   work_dev  the partial sums: MOCAP_LEARN_WORK_BYTES(T, K, 0) bytes for mocap_learn_marker_pair_stats, MOCAP_LEARN_WORK_BYTES(T, 0, G)
 *            for mocap_learn_rigid_bodies, 8-byte aligned, device memory the caller owns; its contents mean nothing between calls.  So
 *            the calls allocate nothing and are asynchronous on `stream`.
 *   ids, member_id, n_members are HOST arrays: they are checked on the host before anything is launched and are copied by the
 *   call (they may be freed when it returns).  Bad arguments (a workspace too small among them) are MOCAP_LEARN_E_INVALID, launch
 *   nothing and leave the outputs untouched.  No floating-point atomics: the same call gives the same bits.
 *
 * mocap_learn_marker_pair_stats: ids int32 [K], strictly ascending, non-negative, 2 <= K <= 64.  For every pair a < b of them, over the
 * steps where both are present, with d = sqrt((dx dx + dy dy) + dz dz): count, dmin, dmax, dsum (of d) and dsum2 (of d * d), each
 * [K][K] and filled symmetrically.  On the diagonal count is the number of steps where the identity is present and the floats are
 * 0; a pair never seen together has count 0 and floats 0.  T = 0 zeroes the outputs.
 *
 * mocap_learn_rigid_bodies: G groups (1..16) of n_members[g] identities member_id[g][0..n_members[g]) (slots beyond are ignored); rounds
 * 1..4; min_present 3..8.  Per group, independently of the others:
 *   - n_members outside 3..8 or below min_present (no step could ever be used), a negative or a repeated member:
 *     MOCAP_LEARN_E_MEMBERS;
 *   - ref_step is the first step at which every member is present; none: MOCAP_LEARN_E_INCOMPLETE;
 *   - the seed model is m_p = D_p(ref_step) - c, c the centroid (the sum over p ascending, divided by n_members);
 *   - a round: every step with at least min_present members present is USED; its present members, in ascending p, are posed against
 *     the current model by Horn's closed form (mocap_rigid_poses' own), each is mapped back, b = R^T (D_p - t), and added to its
 *     member's sum; afterwards m_p = sum_p / member_count[p], recentred as the seed was;
 *   - after `rounds` rounds a residual pass sums |R m_p + t - D_p|^2 per member over the used steps: member_rms[p] =
 *     sqrt(sum_p / member_count[p]), rms = sqrt((sum_0 + sum_1 + ...) / (count_0 + count_1 + ...)).
 * THE MODEL'S FRAME: its origin is the centroid of the model points, its axes are the world's axes as they stood at ref_step.
 *   model_dev float64 [G][8][3] (zeros from n_members on), rms_dev [G], member_rms_dev [G][8], member_count_dev int32 [G][8],
 *   steps_used_dev, ref_step_dev, status_dev int32 [G]: 0 or MOCAP_LEARN_E_*.  On a status other than 0 the counts are 0, ref_step
 *   is -1 and the floats are unspecified and must not be read; the other groups are unaffected. */
#define MOCAP_LEARN_CHUNK 32
#define MOCAP_LEARN_MAX_IDS 64
#define MOCAP_LEARN_MAX_GROUPS 16
#define MOCAP_LEARN_CHUNKS(T) (((size_t)(T) + MOCAP_LEARN_CHUNK - 1) / MOCAP_LEARN_CHUNK)
#define MOCAP_LEARN_PAIRS(K) ((size_t)(K) * ((size_t)(K) + 1) / 2)
/* per chunk: 4 doubles and a count per pair a <= b, 24 doubles and 9 counts per group; per step a row per identity; a model and two words per group */
#define MOCAP_LEARN_WORK_BYTES(T, K, G)                                                                                          \
    (MOCAP_LEARN_CHUNKS(T) * (36 * MOCAP_LEARN_PAIRS(K) + 228 * (size_t)(G)) + 4 * (size_t)(T) * ((size_t)(K) + 8 * (size_t)(G)) + \
     200 * (size_t)(G))
MOCAP_LEARN_API int mocap_learn_marker_pair_stats(int device, const double* xyz_dev /*[T][Q][3]*/, const int32_t* n_dev /*[T]*/,
                                      const int32_t* id_dev /*[T][Q]*/, int T, int Q, const int32_t* ids /*host [K]*/, int K,
                                      void* work_dev, size_t work_bytes, int32_t* count_dev, double* dmin_dev, double* dmax_dev,
                                      double* dsum_dev, double* dsum2_dev /*[K][K] each*/, void* stream);
MOCAP_LEARN_API int mocap_learn_rigid_bodies(int device, const double* xyz_dev /*[T][Q][3]*/, const int32_t* n_dev /*[T]*/,
                                const int32_t* id_dev /*[T][Q]*/, int T, int Q, int G, const int32_t* member_id /*host [G][8]*/,
                                const int32_t* n_members /*host [G]*/, int rounds, int min_present, void* work_dev, size_t work_bytes,
                                double* model_dev /*[G][8][3]*/, double* rms_dev /*[G]*/, double* member_rms_dev /*[G][8]*/,
                                int32_t* member_count_dev /*[G][8]*/, int32_t* steps_used_dev, int32_t* ref_step_dev,
                                int32_t* status_dev /*[G] each*/, void* stream);

#ifdef __cplusplus
}
#endif
#endif
