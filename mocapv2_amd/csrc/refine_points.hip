// refine_points.hip -- refinement of triangulated markers by their reprojection error, with the covariance of the result (FP64).
//
// The reference has no counterpart (its 3-D points are the raw DLT): the contract is the definition of DESIGN.md section 2,
// restated by tests/refine_points_ref.py.  The library is built with -ffp-contract=off: every product and sum below is a
// separately rounded FP64 operation, in the order the definition gives; + - * / only.
//
// Work decomposition: one workgroup per time step, one lane per row (a stride loop lets Q exceed the workgroup).  The camera rows
// are staged in LDS once per step; a lane walks its members in ascending camera order, fetching each observation from memory
// in every pass (a few cache lines per row, read by one lane).  The camera model is lm.h's project, the step control lm.h's
// lm_decide with the state record in registers.  Nothing in registers is indexed by a camera number: the per-member squared
// residuals go straight to memory in the pass behind the loop, the worst member is a running maximum.  No atomics.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "kernels.h"
#include "geom_dev.h"
#include "correspond_dev.h"
#include "lm.h"

namespace mocap {

namespace {

constexpr int RP_THREADS = 128;

// ---- where camera c's observation of a row comes from: the one template parameter of everything below ----
// indexed: point idx[t][q][c] of the camera's list, through the strides and point types of mocap_correspond_visible
template <typename PT>
struct IndexedPoints {
    static __device__ __forceinline__ bool valid(const RefinePointsArgs& a, size_t row, int c)
    {
        const int p = a.idx[row * a.C + c];
        return p >= 0 && p < a.P;
    }
    static __device__ __forceinline__ void load(const RefinePointsArgs& a, int t, size_t row, int c, double& u, double& v)
    {
        load_pt<PT>(a.pts, point_base(a, t, c) + (size_t)a.idx[row * a.C + c], u, v);
    }
};
// grouped: grp[t][q][c], mocap_correspond's root_grp as it is
struct GroupedPoints {
    static __device__ __forceinline__ bool valid(const RefinePointsArgs&, size_t, int) { return true; }
    static __device__ __forceinline__ void load(const RefinePointsArgs& a, int, size_t row, int c, double& u, double& v)
    {
        const double* p = a.grp + 2 * (row * a.C + c);
        u = p[0]; v = p[1];
    }
};

// What one pass over a row's members leaves: S = sum of the squared residual lengths, with JAC the upper triangle of J^T J and
// J^T r, whether X lies in front of every member, and the member with the largest squared residual length (the lower camera of equals)
struct Pass {
    double S, H[6], g[3], worst_r2;
    int worst;
    bool front;
};

// ---- one pass: the members of `mask` in ascending camera order at X.  WRITE: res2[c] goes to memory, -1 for a camera that is no member
template <class SRC, bool JAC, bool WRITE>
__device__ __forceinline__ void pass_members(const RefinePointsArgs& a, const double* cam, int t, size_t row, uint32_t mask, const double X[3], Pass& e)
{
    e.S = 0.;
#pragma unroll
    for (int k = 0; k < 6; k++) e.H[k] = 0.;
    e.g[0] = e.g[1] = e.g[2] = 0.;
    e.worst_r2 = -1.; e.worst = 0; e.front = true;
    for (int c = 0; c < a.C; c++) {
        if (!((mask >> c) & 1u)) {
            if (WRITE) a.res2[row * a.C + c] = -1.;
            continue;
        }
        const double* cr = cam + c * CAM_ROW;
        const double* R = cr + oR;
        const bool lens = a.distorted != 0;
        const Lens m = {cr[oK + 0], cr[oK + 4], cr[oK + 2], cr[oK + 5], lens ? cr[oD + 0] : 0., lens ? cr[oD + 1] : 0., lens ? cr[oD + 2] : 0.,
                        lens ? cr[oD + 3] : 0., lens ? cr[oD + 4] : 0.};
        double u, v;
        SRC::load(a, t, row, c, u, v);
        double q[3], r[2];
#pragma unroll
        for (int i = 0; i < 3; i++) q[i] = (R[3 * i] * X[0] + R[3 * i + 1] * X[1]) + R[3 * i + 2] * X[2];
        Projected o;
        if (!project<JAC>(m, q, cr + oT, u, v, r, o)) e.front = false;
        const double r2 = r[0] * r[0] + r[1] * r[1];
        e.S += r2;
        if (WRITE) a.res2[row * a.C + c] = r2;
        if (r2 > e.worst_r2) { e.worst_r2 = r2; e.worst = c; }
        if (JAC) {
            double J[2][3]; // J = A R_c
#pragma unroll
            for (int i = 0; i < 2; i++)
#pragma unroll
                for (int j = 0; j < 3; j++) J[i][j] = (o.A[i][0] * R[j] + o.A[i][1] * R[3 + j]) + o.A[i][2] * R[6 + j];
            e.H[0] += J[0][0] * J[0][0] + J[1][0] * J[1][0]; e.H[1] += J[0][0] * J[0][1] + J[1][0] * J[1][1];
            e.H[2] += J[0][0] * J[0][2] + J[1][0] * J[1][2]; e.H[3] += J[0][1] * J[0][1] + J[1][1] * J[1][1];
            e.H[4] += J[0][1] * J[0][2] + J[1][1] * J[1][2]; e.H[5] += J[0][2] * J[0][2] + J[1][2] * J[1][2];
#pragma unroll
            for (int j = 0; j < 3; j++) e.g[j] += J[0][j] * r[0] + J[1][j] * r[1];
        }
    }
}

// ---- the trial step at damping lambda from the linearisation e: d = -inv_sym3(H + lambda diag H) g.  false = the determinant
// is not finite or not positive (the control rule's failed factorisation).  part: lm_decide's three sums, but for the trial's cost
__device__ __forceinline__ bool solve_step(const Pass& e, double lambda, const double X[3], double Xt[3], double part[3])
{
    const double Hd[6] = {e.H[0] + lambda * e.H[0], e.H[1], e.H[2], e.H[3] + lambda * e.H[3], e.H[4], e.H[5] + lambda * e.H[5]};
    double inv[6];
    const double det = inv_sym3(Hd, inv);
    if (!(det > 0.0) || !finite(det)) return false;
    const double d[3] = {-((inv[0] * e.g[0] + inv[1] * e.g[1]) + inv[2] * e.g[2]), -((inv[1] * e.g[0] + inv[3] * e.g[1]) + inv[4] * e.g[2]),
                         -((inv[2] * e.g[0] + inv[4] * e.g[1]) + inv[5] * e.g[2])};
    const double diag[3] = {e.H[0], e.H[3], e.H[5]};
    double pred = 0, n2 = 0;
#pragma unroll
    for (int j = 0; j < 3; j++) {
        Xt[j] = X[j] + d[j];
        pred += d[j] * ((lambda * diag[j]) * d[j] - e.g[j]);
        n2 += d[j] * d[j];
    }
    part[1] = pred; part[2] = n2;
    return true;
}

// ---- an error row: the point handed in, the mask handed in, the code
__device__ __forceinline__ void error_row(const RefinePointsArgs& a, size_t row, const double X[3], uint32_t mask, int code)
{
    a.xyz_out[3 * row] = X[0]; a.xyz_out[3 * row + 1] = X[1]; a.xyz_out[3 * row + 2] = X[2];
    a.views_out[row] = mask;
    a.status[row] = code;
}

// ---- one row, by one lane: checks, then loops of (linearise, LM iterations, last pass) with a member dropped between two loops
template <class SRC>
__device__ __forceinline__ void refine_row(const RefinePointsArgs& a, const double* cam, int t, int q)
{
    const size_t row = (size_t)t * a.Q + q;
    const int C = a.C;
    const uint32_t all = C == 32 ? 0xffffffffu : (1u << C) - 1u;
    const uint32_t in_mask = a.views ? a.views[row] : all;
    double X[3] = {a.xyz[3 * row], a.xyz[3 * row + 1], a.xyz[3 * row + 2]};
    bool input_ok = !(in_mask & ~all) && finite(X[0]) && finite(X[1]) && finite(X[2]);
    if (input_ok)
        for (int c = 0; c < C; c++)
            if (((in_mask >> c) & 1u) && !SRC::valid(a, row, c)) input_ok = false;
    if (!input_ok) return error_row(a, row, X, in_mask, REFINE_ERR_INPUT);
    if (__popc(in_mask) < 2) return error_row(a, row, X, in_mask, REFINE_ERR_VIEWS);

    uint32_t mask = in_mask, dropped = 0;
    int total = 0, drops = 0, code = 0;
    const double no_cam[2] = {0., 0.};
    Pass e;
    for (;;) {
        pass_members<SRC, true, false>(a, cam, t, row, mask, X, e);
        if (total == 0 && !e.front) return error_row(a, row, X, in_mask, REFINE_ERR_BEHIND);
        LmState st = {};
        st.lambda = a.lambda0; st.nu = 2.0; st.cost = st.cost0 = 0.5 * e.S;
        for (int it = 0;; it++) {
            double Xt[3] = {X[0], X[1], X[2]}, part[3] = {0., 0., 0.}, h[4];
            if (!solve_step(e, st.lambda, X, Xt, part)) st.chol_fail = 1;
            else {
                Pass tr;
                pass_members<SRC, false, false>(a, cam, t, row, mask, Xt, tr);
                part[0] = tr.S;
                if (!(finite(Xt[0]) && finite(Xt[1]) && finite(Xt[2])) || !tr.front) st.trial_behind = 1;
            }
            lm_decide(&st, part, 1, no_cam, it, a.max_iters, a.ftol, h);
            total++;
            if (st.cur) { // accepted: the trial is the state
                st.cur = 0;
                X[0] = Xt[0]; X[1] = Xt[1]; X[2] = Xt[2];
                if (!st.stop) pass_members<SRC, true, false>(a, cam, t, row, mask, X, e);
            }
            if (st.stop) break;
        }
        code = st.status;
        pass_members<SRC, true, true>(a, cam, t, row, mask, X, e); // res2 to memory, H for the covariance, the worst member
        if (a.max_res2 > 0.0 && __popc(mask) > a.min_views && drops < a.max_drop && e.worst_r2 > a.max_res2) {
            mask &= ~(1u << e.worst); dropped |= 1u << e.worst;
            drops++;
            continue;
        }
        break;
    }
    double cov[6];
    inv_sym3(e.H, cov);
    a.xyz_out[3 * row] = X[0]; a.xyz_out[3 * row + 1] = X[1]; a.xyz_out[3 * row + 2] = X[2];
    a.err[row] = e.S / (double)(2 * __popc(mask));
#pragma unroll
    for (int k = 0; k < 6; k++) a.cov[6 * row + k] = cov[k];
    a.views_out[row] = mask; a.dropped[row] = dropped;
    a.iters[row] = total; a.status[row] = code;
}

} // namespace

// One workgroup per time step; lane q, q + 128, ... owns those rows.  A row at or beyond n[t] (every row of a step with n[t] <= 0)
// gets status 0 and nothing else.
template <class SRC>
__global__ __launch_bounds__(RP_THREADS) void refine_points_kernel(RefinePointsArgs a)
{
    __shared__ double cam[32 * CAM_ROW];
    const int t = blockIdx.x, tid = threadIdx.x;
    const int n = a.n[t], rows = n < a.Q ? n : a.Q;
    if (rows > 0) stage_camera_rows<CAM_ROW>(cam, a.cams, a.C, tid, RP_THREADS);
    __syncthreads();
    for (int q = tid; q < a.Q; q += RP_THREADS) {
        if (q < rows) refine_row<SRC>(a, cam, t, q);
        else a.status[(size_t)t * a.Q + q] = 0;
    }
}

void launch_refine_points(const RefinePointsArgs& a, hipStream_t s)
{
    if (!a.pts)
        hipLaunchKernelGGL(refine_points_kernel<GroupedPoints>, dim3(a.T), dim3(RP_THREADS), 0, s, a);
    else if (a.pts_f64)
        hipLaunchKernelGGL(refine_points_kernel<IndexedPoints<double>>, dim3(a.T), dim3(RP_THREADS), 0, s, a);
    else
        hipLaunchKernelGGL(refine_points_kernel<IndexedPoints<int32_t>>, dim3(a.T), dim3(RP_THREADS), 0, s, a);
}

} // namespace mocap
