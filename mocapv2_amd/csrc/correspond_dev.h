// correspond_dev.h -- what correspond_kernel (correspond.hip) and correspond_visible_kernel (correspond_visible.hip) share: the
// per-camera row in LDS and the one round of loads that begins a time step -- camera rows, points, projection matrices, checked
// counts.  Both kernels run one workgroup per time step; every function here is called by all its threads (tid of nth).
// Device code only, built with -ffp-contract=off like everything that includes it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "kernels.h"
#include "geom_dev.h"

namespace mocap {

// A camera's row in LDS, in doubles: P = K [R|t] (12), K (9), dist (5), R (9), t (3).  A kernel may append to it (row width CW).
constexpr int oP = 0, oK = 12, oD = 21, oR = 26, oT = 35, CAM_ROW = 38;

// element offset (in points) of camera c's list in time step t; strides are given in scalars, a point is 2 scalars
template <typename Args>
__device__ __forceinline__ size_t point_base(const Args& a, int t, int c)
{
    return ((size_t)t * a.pt_st + (size_t)c * a.pt_sc) / 2;
}

// K, dist, R, t of cameras 0..C-1 from the table into their rows (26 doubles behind oK)
template <int CW>
__device__ __forceinline__ void stage_camera_rows(double* cam, const CameraTable* cams, int C, int tid, int nth)
{
    for (int w = tid; w < C * 26; w += nth) {
        const int c = w / 26, k = w - c * 26;
        cam[c * CW + oK + k] = k < 9 ? cams->K[c][k] : (k < 14 ? cams->dist[c][k - 9] : (k < 23 ? cams->R[c][k - 14] : cams->t[c][k - 23]));
    }
}

// every point slot of the time step, up to P per camera (the address does not depend on the count), as doubles: spts[C][P][2]
template <typename PT, typename Args>
__device__ __forceinline__ void stage_step_points(double* spts, const Args& a, int t, int tid, int nth)
{
    const int P = a.P;
    for (int w = tid; w < a.C * P; w += nth) {
        const int c = w / P, p = w - c * P;
        double x, y;
        load_pt<PT>(a.pts, point_base(a, t, c) + p, x, y);
        spts[2 * w] = x; spts[2 * w + 1] = y;
    }
}

// P = K @ [R|t] of every staged row, one entry per lane, the sums in the order of reference lib/Helpers.py:58-62 -- the order
// in which DltAcc::add forms them (geom_dev.h), so that DltAcc::add_rows on a row gives add's bits
template <int CW>
__device__ __forceinline__ void form_projections(double* cam, int C, int tid, int nth)
{
    for (int w = tid; w < C * 12; w += nth) {
        const int c = w / 12, r = (w % 12) / 4, cc = w % 4;
        const double* K = cam + c * CW + oK; const double* R = cam + c * CW + oR; const double* tt = cam + c * CW + oT;
        double sum = 0;
        for (int k = 0; k < 3; k++) sum += K[3 * r + k] * (cc < 3 ? R[3 * k + cc] : tt[k]);
        cam[c * CW + oP + 4 * r + cc] = sum;
    }
}

// The count of camera c as it was loaded.  A count that does not fit the P points read, or a negative one (the blob stage's
// capacity error), fails the time step: the reference has no such limits (lib/Helpers.py:191,203-245), so a shortened list must
// never pass for a result.  *s_err (a word in LDS): 2 = more than P points, 3 = negative count; 1 and 4 are the callers' own.
__device__ __forceinline__ int checked_count(const int* scnt, int c, int P, int* s_err)
{
    const int n = scnt[c];
    if (n < 0) atomicMax(s_err, 3);
    else if (n > P) atomicMax(s_err, 2);
    return n;
}
// what a time step that failed that check reports
__device__ __forceinline__ int count_error_code(int err) { return err == 3 ? CORR_ERR_BLOB : CORR_ERR_TRUNCATED; }

} // namespace mocap
