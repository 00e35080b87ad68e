// abi_rigid.hip -- C-ABI host file: rigid-body poses per time step (mocap_rigid_poses).
#include <limits.h>
#include "ctx.h"

static_assert(MOCAP_RIGID_LOST == RIGID_LOST && MOCAP_RIGID_E_BLIND == RIGID_ERR_BLIND && MOCAP_RIGID_E_CAPACITY == RIGID_ERR_CAPACITY &&
                  MOCAP_RIGID_E_MODEL == RIGID_ERR_MODEL && MOCAP_RIGID_E_HYP == RIGID_ERR_HYP, "the header's codes are the kernel's");
static_assert(MOCAP_RIGID_MAX_DETECTIONS == RIGID_MAX_DET && MOCAP_RIGID_MAX_MARKERS == RIGID_MAX_MARKERS &&
                  MOCAP_RIGID_MAX_TRIPLES == RIGID_MAX_TRIPLES && MOCAP_RIGID_MAX_BODIES == RIGID_MAX_BODIES &&
                  MOCAP_RIGID_MAX_HYP == RIGID_MAX_HYP, "the header's caps are the kernel's");

extern "C" {

int mocap_rigid_poses(mocap_ctx_t c, const double* xyz, const int32_t* n, int T, int Q, int B, const double* model,
                      const int32_t* n_markers, const int32_t* tri, const int32_t* n_tri, double tol, double gate, int min_markers,
                      int max_hyp, double* R, double* t, double* q, double* rms, int32_t* n_in, int32_t* label, int32_t* status,
                      void* stream)
{
    if (!c) return fail(MOCAP_E_INVALID, "null argument");
    if (T < 0 || Q < 1 || B < 0 || B > RIGID_MAX_BODIES) return fail(MOCAP_E_INVALID, "T=%d Q=%d B=%d (T >= 0, Q >= 1, B 0..%d)", T, Q, B, RIGID_MAX_BODIES);
    if ((long long)T * B > INT_MAX) return fail(MOCAP_E_INVALID, "T=%d B=%d: more than %d workgroups", T, B, INT_MAX);
    if (!(isfinite(tol) && tol > 0)) return fail(MOCAP_E_INVALID, "tol=%g must be finite and > 0", tol);
    if (!(isfinite(gate) && gate > 0)) return fail(MOCAP_E_INVALID, "gate=%g must be finite and > 0", gate);
    if (min_markers < 3 || min_markers > RIGID_MAX_MARKERS) return fail(MOCAP_E_INVALID, "min_markers=%d outside 3..%d", min_markers, RIGID_MAX_MARKERS);
    if (max_hyp < 1 || max_hyp > RIGID_MAX_HYP) return fail(MOCAP_E_INVALID, "max_hyp=%d outside 1..%d", max_hyp, RIGID_MAX_HYP);
    if (T == 0 || B == 0) return MOCAP_OK;
    if (!xyz || !n || !model || !n_markers || !tri || !n_tri || !R || !t || !q || !rms || !n_in || !label || !status)
        return fail(MOCAP_E_INVALID, "null argument");
    if (set_device(c)) return MOCAP_E_HIP;
    RigidArgs a;
    a.xyz = xyz; a.n = n; a.T = T; a.Q = Q; a.B = B; a.model = model; a.n_markers = n_markers; a.tri = tri; a.n_tri = n_tri;
    a.tol = tol; a.gate = gate; a.min_markers = min_markers; a.max_hyp = max_hyp;
    a.R = R; a.t = t; a.q = q; a.rms = rms; a.n_in = n_in; a.label = label; a.status = status;
    launch_rigid_poses(a, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return MOCAP_OK;
}

} // extern "C"
