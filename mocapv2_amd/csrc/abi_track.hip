// abi_track.hip -- C-ABI host file: marker identities across time steps (mocap_track_markers).
#include "ctx.h"

static_assert(sizeof(mocap_track_header) == sizeof(TrackHeader) && sizeof(mocap_track_slot) == sizeof(TrackSlot) &&
                  MOCAP_TRACK_STATE_BYTES(TRACK_MAX) == sizeof(TrackHeader) + TRACK_MAX * sizeof(TrackSlot),
              "the header's state layout is the kernel's");
static_assert(MOCAP_TRACK_E_FULL == TRACK_ERR_FULL && MOCAP_TRACK_E_IDS == TRACK_ERR_IDS && MOCAP_TRACK_E_INPUT == TRACK_ERR_INPUT &&
                  MOCAP_TRACK_E_COUNT == TRACK_ERR_COUNT, "the header's codes are the kernel's");

extern "C" {

int mocap_track_markers(mocap_ctx_t c, const double* xyz, const int32_t* n, int T, int Q, void* state, int max_tracks, double gate,
                        double beta, int max_miss, int32_t* id, int32_t* slot, int32_t* age, int32_t* status, void* stream)
{
    if (!c) return fail(MOCAP_E_INVALID, "null argument");
    if (T < 0 || Q < 1) return fail(MOCAP_E_INVALID, "T=%d Q=%d (T >= 0, Q >= 1)", T, Q);
    if (max_tracks < 1 || max_tracks > TRACK_MAX) return fail(MOCAP_E_INVALID, "max_tracks=%d outside 1..%d", max_tracks, TRACK_MAX);
    if (!(isfinite(gate) && gate > 0)) return fail(MOCAP_E_INVALID, "gate=%g must be finite and > 0", gate);
    if (!(beta >= 0 && beta <= 1)) return fail(MOCAP_E_INVALID, "beta=%g outside [0, 1]", beta);
    if (max_miss < 0) return fail(MOCAP_E_INVALID, "max_miss=%d is negative", max_miss);
    if (T == 0) return MOCAP_OK;
    if (!xyz || !n || !state || !id || !slot || !age || !status) return fail(MOCAP_E_INVALID, "null argument");
    if (set_device(c)) return MOCAP_E_HIP;
    TrackArgs a;
    a.xyz = xyz; a.n = n; a.T = T; a.Q = Q; a.M = max_tracks; a.state = state; a.gate = gate; a.beta = beta; a.max_miss = max_miss;
    a.id = id; a.slot = slot; a.age = age; a.status = status;
    launch_track_markers(a, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return MOCAP_OK;
}

} // extern "C"
