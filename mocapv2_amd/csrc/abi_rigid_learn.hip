// abi_rigid_learn.hip -- the C-ABI host file of libmocap_learn.so (include/mocap_learn.h): rigid-body models learned from a tracked
// capture (mocap_learn_marker_pair_stats, mocap_learn_rigid_bodies).  A library of its own: libmocap_hip.so's declarations and
// exports stay as they are, so nothing here comes from ctx.h -- the calls are told the device, and the error channel is this file's.
// Both take their small integer lists (ids, member_id, n_members) from HOST memory: they are checked here, before anything is
// launched, and travel to the kernels by value.  Neither allocates: the partial sums live in the caller's workspace.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include "../../include/mocap_learn.h"
#include "kernels.h"

using namespace mocap;

static thread_local char g_error[512];

// sets the calling thread's message for mocap_learn_last_error and returns `code`
static int fail(int code, const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_error, sizeof g_error, fmt, ap);
    va_end(ap);
    return code;
}

#define HIP_TRY(expr)                                                                                              \
    do {                                                                                                           \
        hipError_t e_ = (expr);                                                                                    \
        if (e_ != hipSuccess) return fail(MOCAP_LEARN_E_HIP, "%s failed: %s", #expr, hipGetErrorString(e_));       \
    } while (0)
#define TRY(expr) do { if (int rc_ = (expr)) return rc_; } while (0)

static_assert(MOCAP_LEARN_E_MEMBERS == LEARN_ERR_MEMBERS && MOCAP_LEARN_E_INCOMPLETE == LEARN_ERR_INCOMPLETE, "the header's codes are the kernel's");
static_assert(MOCAP_LEARN_CHUNK == LEARN_CHUNK && MOCAP_LEARN_MAX_IDS == LEARN_MAX_IDS && MOCAP_LEARN_MAX_GROUPS == LEARN_MAX_GROUPS &&
                  8 == RIGID_MAX_MARKERS, "the header's caps are the kernel's");

// what both calls ask of the take and of the workspace.  -> 0, or fail()'s code
static int check_take(const void* xyz, const void* n, const void* id, int T, int Q, int K, int G, const void* work, size_t work_bytes,
                      LearnWork& w)
{
    if (T < 0 || Q < 1) return fail(MOCAP_LEARN_E_INVALID, "T=%d Q=%d (T >= 0, Q >= 1)", T, Q);
    if ((long long)T * (K + 8 * G) / 256 >= INT_MAX) return fail(MOCAP_LEARN_E_INVALID, "T=%d: more than %d workgroups", T, INT_MAX);
    if (T > 0 && (!xyz || !n || !id)) return fail(MOCAP_LEARN_E_INVALID, "null argument");
    w = LearnWork((void*)work, T, K, G);
    if (w.bytes != MOCAP_LEARN_WORK_BYTES(T, K, G)) return fail(MOCAP_LEARN_E_INVALID, "MOCAP_LEARN_WORK_BYTES(%d, %d, %d) is not the kernels' layout", T, K, G);
    if (w.bytes > 0 && (!work || ((uintptr_t)work & 7) || work_bytes < w.bytes)) // (T = 0 needs no pair workspace: none is read)
        return fail(MOCAP_LEARN_E_INVALID, "a workspace of %zu bytes at %p: MOCAP_LEARN_WORK_BYTES(%d, %d, %d) = %zu, 8-byte aligned", work_bytes, work,
                    T, K, G, w.bytes);
    return 0;
}

extern "C" {

int mocap_learn_abi_version(void) { return MOCAP_LEARN_ABI_VERSION; }
const char* mocap_learn_last_error(void) { return g_error; }

MOCAP_LEARN_API int mocap_learn_marker_pair_stats(int device, const double* xyz, const int32_t* n, const int32_t* id, int T, int Q, const int32_t* ids, int K,
                            void* work, size_t work_bytes, int32_t* count, double* dmin, double* dmax, double* dsum, double* dsum2,
                            void* stream)
{
    if (!ids || !count || !dmin || !dmax || !dsum || !dsum2) return fail(MOCAP_LEARN_E_INVALID, "null argument");
    if (K < 2 || K > LEARN_MAX_IDS) return fail(MOCAP_LEARN_E_INVALID, "K=%d outside 2..%d", K, LEARN_MAX_IDS);
    for (int k = 0; k < K; k++)
        if (ids[k] < 0 || (k > 0 && ids[k] <= ids[k - 1]))
            return fail(MOCAP_LEARN_E_INVALID, "ids[%d]=%d: the identities must be non-negative and strictly ascending", k, ids[k]);
    PairArgs a;
    TRY(check_take(xyz, n, id, T, Q, K, 0, work, work_bytes, a.w));
    HIP_TRY(hipSetDevice(device));
    a.xyz = xyz; a.n = n; a.id = id; a.T = T; a.Q = Q; a.K = K;
    for (int k = 0; k < LEARN_MAX_WANTED; k++) a.ids.id[k] = k < K ? ids[k] : -1;
    a.count = count; a.dmin = dmin; a.dmax = dmax; a.dsum = dsum; a.dsum2 = dsum2;
    launch_marker_pair_stats(a, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return MOCAP_LEARN_OK;
}

MOCAP_LEARN_API int mocap_learn_rigid_bodies(int device, const double* xyz, const int32_t* n, const int32_t* id, int T, int Q, int G, const int32_t* member_id,
                      const int32_t* n_members, int rounds, int min_present, void* work, size_t work_bytes, double* model, double* rms,
                      double* member_rms, int32_t* member_count, int32_t* steps_used, int32_t* ref_step, int32_t* status, void* stream)
{
    if (!member_id || !n_members || !model || !rms || !member_rms || !member_count || !steps_used || !ref_step || !status)
        return fail(MOCAP_LEARN_E_INVALID, "null argument");
    if (G < 1 || G > LEARN_MAX_GROUPS) return fail(MOCAP_LEARN_E_INVALID, "G=%d outside 1..%d", G, LEARN_MAX_GROUPS);
    if (rounds < 1 || rounds > 4) return fail(MOCAP_LEARN_E_INVALID, "rounds=%d outside 1..4", rounds);
    if (min_present < 3 || min_present > RIGID_MAX_MARKERS) return fail(MOCAP_LEARN_E_INVALID, "min_present=%d outside 3..%d", min_present, RIGID_MAX_MARKERS);
    LearnArgs a;
    TRY(check_take(xyz, n, id, T, Q, 0, G, work, work_bytes, a.w));
    HIP_TRY(hipSetDevice(device));
    a.xyz = xyz; a.n = n; a.id = id; a.T = T; a.Q = Q; a.G = G; a.rounds = rounds; a.min_present = min_present;
    a.valid = 0u;
    for (int k = 0; k < LEARN_MAX_WANTED; k++) a.members.id[k] = -1;
    for (int g = 0; g < LEARN_MAX_GROUPS; g++) a.n_members[g] = 0;
    for (int g = 0; g < G; g++) {
        const int M = n_members[g];
        const int32_t* m = member_id + g * RIGID_MAX_MARKERS;
        bool ok = M >= 3 && M <= RIGID_MAX_MARKERS && M >= min_present; // with fewer than min_present members no step is ever used
        for (int p = 0; ok && p < M; p++) {
            ok = m[p] >= 0;
            for (int q = 0; ok && q < p; q++) ok = m[q] != m[p];
        }
        if (!ok) continue; // MOCAP_LEARN_E_MEMBERS: the group wants no identity and reads no slot
        a.valid |= 1u << g;
        a.n_members[g] = M;
        for (int p = 0; p < M; p++) a.members.id[g * RIGID_MAX_MARKERS + p] = m[p];
    }
    a.model = model; a.rms = rms; a.member_rms = member_rms; a.member_count = member_count; a.steps_used = steps_used;
    a.ref_step = ref_step; a.status = status;
    launch_rigid_learn(a, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return MOCAP_LEARN_OK;
}

} // extern "C"
