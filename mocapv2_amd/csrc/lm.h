// lm.h -- what the Levenberg-Marquardt solvers (the two rig solvers through rig_lm.h, intrinsics.hip) share, each defined once: the camera
// model with its derivatives, the step-control rule over the state record LmState of kernels.h (both: DESIGN.md section 2,
// restated by tests/lm_ref.py), the small index helpers of their packed triangles, and the rig solvers' dense algebra (the
// inverse of a point's 3x3, the packed Cholesky of the reduced camera matrix).
// The library is built with -ffp-contract=off: every product and sum below is rounded on its own, and the restatement forms
// each value by the same operations in the same order.
#pragma once
#include "kernels.h"

namespace mocap {

__device__ __forceinline__ bool finite(double x) { return fabs(x) <= 1.7976931348623157e308; } // false for NaN

__device__ __forceinline__ constexpr int low(int i, int j) { return i * (i + 1) / 2 + j; } // packed lower triangle, j <= i
// position of element (i, j), i <= j, of a symmetric n x n stored as its upper triangle row by row, and the inverse: rank e -> (i, j)
__device__ __forceinline__ constexpr int tri(int i, int j, int n) { return i * n - i * (i - 1) / 2 + (j - i); }
__device__ __forceinline__ void tri_unrank(int e, int n, int& i, int& j)
{
    for (i = 0; e >= n - i; i++) e -= n - i;
    j = i + e;
}

// R <- Exp(w) R by Rodrigues' formula: the local rotation update of both loops
__device__ __forceinline__ void rotate_left(const double w[3], const double R[9], double out[9])
{
    const double th2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2], th = sqrt(th2);
    const double ka = th < 1e-12 ? 1.0 : sin(th) / th, kb = th < 1e-12 ? 0.5 : (1.0 - cos(th)) / th2;
    // E = I + ka K + kb K^2, K = [w]x, K^2 = w w^T - th2 I
    double E[9];
    E[0] = 1.0 + kb * (w[0] * w[0] - th2); E[4] = 1.0 + kb * (w[1] * w[1] - th2); E[8] = 1.0 + kb * (w[2] * w[2] - th2);
    E[1] = kb * (w[0] * w[1]) - ka * w[2]; E[3] = kb * (w[0] * w[1]) + ka * w[2];
    E[2] = kb * (w[0] * w[2]) + ka * w[1]; E[6] = kb * (w[0] * w[2]) - ka * w[1];
    E[5] = kb * (w[1] * w[2]) - ka * w[0]; E[7] = kb * (w[1] * w[2]) + ka * w[0];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) out[3 * i + j] = (E[3 * i] * R[j] + E[3 * i + 1] * R[3 + j]) + E[3 * i + 2] * R[6 + j];
}

// The lens: pinhole + Brown distortion.
struct Lens { double fx, fy, cx, cy, k1, k2, p1, p2, k3; };

// What project() leaves behind for the Jacobians its callers build: the normalised point and its powers, the tangential
// terms tx = r2 + 2 x^2, ty = r2 + 2 y^2, the distorted point, and with JAC the 2x3 A = d pixel / d (q + t).
struct Projected { double x, y, xy, r2, r4, r6, tx, ty, xd, yd, A[2][3]; };

// One point q + t in the camera frame (q = R X, formed by the caller) against its pixel (ou, ov): the residual r.  Returns
// false when the point is not in front of the camera (z <= 0 or NaN).
template <bool JAC>
__device__ __forceinline__ bool project(const Lens& m, const double q[3], const double t[3], double ou, double ov, double r[2], Projected& o)
{
    const double px = q[0] + t[0], py = q[1] + t[1], pz = q[2] + t[2];
    const bool front = pz > 0.0;
    const double x = px / pz, y = py / pz;
    const double xx = x * x, yy = y * y, xy = x * y;
    const double r2 = xx + yy, r4 = r2 * r2, r6 = r4 * r2;
    const double cd = ((1.0 + m.k1 * r2) + m.k2 * r4) + m.k3 * r6;
    const double tx = r2 + 2.0 * xx, ty = r2 + 2.0 * yy;
    const double xd = (x * cd + (2.0 * m.p1) * xy) + m.p2 * tx;
    const double yd = (y * cd + m.p1 * ty) + (2.0 * m.p2) * xy;
    r[0] = (m.fx * xd + m.cx) - ou;
    r[1] = (m.fy * yd + m.cy) - ov;
    if (JAC) {
        o.x = x; o.y = y; o.xy = xy; o.r2 = r2; o.r4 = r4; o.r6 = r6; o.tx = tx; o.ty = ty; o.xd = xd; o.yd = yd;
        const double e = (m.k1 + (2.0 * m.k2) * r2) + (3.0 * m.k3) * r4;
        const double a00 = ((cd + (2.0 * xx) * e) + (2.0 * m.p1) * y) + (6.0 * m.p2) * x;
        const double a01 = ((2.0 * xy) * e + (2.0 * m.p1) * x) + (2.0 * m.p2) * y;
        const double a11 = ((cd + (2.0 * yy) * e) + (6.0 * m.p1) * y) + (2.0 * m.p2) * x;
        const double b00 = m.fx * a00, b01 = m.fx * a01, b10 = m.fy * a01, b11 = m.fy * a11;
        const double iz = 1.0 / pz;
        o.A[0][0] = b00 * iz; o.A[0][1] = b01 * iz; o.A[0][2] = -((b00 * x + b01 * y) * iz);
        o.A[1][0] = b10 * iz; o.A[1][1] = b11 * iz; o.A[1][2] = -((b10 * x + b11 * y) * iz);
    }
    return front;
}

// The lens columns of an observation's Jacobian, d pixel / d (fx, fy, cx, cy, k1, k2, p1, p2, k3), from what project<true> left
// behind: j0[0..8] the row of u, j1[0..8] the row of v
__device__ __forceinline__ void lens_columns(const Lens& m, const Projected& o, double* j0, double* j1)
{
    j0[0] = o.xd; j0[1] = 0.0; j0[2] = 1.0; j0[3] = 0.0;
    j1[0] = 0.0; j1[1] = o.yd; j1[2] = 0.0; j1[3] = 1.0;
    j0[4] = m.fx * (o.x * o.r2); j0[5] = m.fx * (o.x * o.r4); j0[6] = m.fx * (2.0 * o.xy); j0[7] = m.fx * o.tx; j0[8] = m.fx * (o.x * o.r6);
    j1[4] = m.fy * (o.y * o.r2); j1[5] = m.fy * (o.y * o.r4); j1[6] = m.fy * o.ty; j1[7] = m.fy * (2.0 * o.xy); j1[8] = m.fy * (o.y * o.r6);
}

// One row of the pose Jacobian under the local perturbation R <- Exp(w) R, t <- t + dt, from the same row of A: the columns
// w = A (-[q]x), then dt = A
__device__ __forceinline__ void pose_columns(const double A[3], const double q[3], double j[6])
{
    j[0] = A[2] * q[1] - A[1] * q[2];
    j[1] = A[0] * q[2] - A[2] * q[0];
    j[2] = A[1] * q[0] - A[0] * q[1];
    j[3] = A[0]; j[4] = A[1]; j[5] = A[2];
}

// inverse of the symmetric 3x3 with upper triangle v[6] = (00, 01, 02, 11, 12, 22) by the adjugate; same layout out.  Returns
// the determinant it divided by (refine_points.hip's test of a failed factorisation; the rig solvers do not look at it)
__device__ __forceinline__ double inv_sym3(const double v[6], double o[6])
{
    const double c00 = v[3] * v[5] - v[4] * v[4], c01 = v[2] * v[4] - v[1] * v[5], c02 = v[1] * v[4] - v[2] * v[3];
    const double det = (v[0] * c00 + v[1] * c01) + v[2] * c02;
    const double c11 = v[0] * v[5] - v[2] * v[2], c12 = v[1] * v[2] - v[0] * v[4], c22 = v[0] * v[3] - v[1] * v[1];
    o[0] = c00 / det; o[1] = c01 / det; o[2] = c02 / det; o[3] = c11 / det; o[4] = c12 / det; o[5] = c22 / det;
    return det;
}
__device__ __forceinline__ double sym3(const double v[6], int i, int j)
{
    const int a = i < j ? i : j, b = i < j ? j : i;
    return v[a == 0 ? b : (a == 1 ? 2 + b : 5)];
}

// The reduced camera system of the rig solvers (rig_lm.h), by one workgroup of 256 threads.
// In-place Cholesky S = L L^T on the packed lower triangle (right-looking); false when a pivot is not positive
__device__ __forceinline__ bool cholesky_packed(double* L, int D)
{
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    for (int k = 0; k < D; k++) {
        __syncthreads();
        const double d = L[low(k, k)];
        if (!(d > 0.0) || !finite(d)) return false; // uniform: every thread reads the same value
        const double sd = sqrt(d);
        __syncthreads();
        for (int i = k + tid; i < D; i += 256) L[low(i, k)] = i == k ? sd : L[low(i, k)] / sd;
        __syncthreads();
        for (int i = k + 1 + ty; i < D; i += 16) {
            const double lik = L[low(i, k)];
            for (int j = k + 1 + tx; j <= i; j += 16) L[low(i, j)] -= lik * L[low(j, k)];
        }
    }
    __syncthreads();
    return true;
}

// L L^T x = b with b, x in s_x (LDS), column by column
__device__ __forceinline__ void solve_packed(const double* L, int D, double* s_x)
{
    const int tid = threadIdx.x;
    for (int k = 0; k < D; k++) {
        if (tid == 0) s_x[k] = s_x[k] / L[low(k, k)];
        __syncthreads();
        const double xk = s_x[k];
        for (int i = k + 1 + tid; i < D; i += 256) s_x[i] -= L[low(i, k)] * xk;
        __syncthreads();
    }
    for (int k = D - 1; k >= 0; k--) {
        if (tid == 0) s_x[k] = s_x[k] / L[low(k, k)];
        __syncthreads();
        const double xk = s_x[k];
        for (int i = tid; i < k; i += 256) s_x[i] -= L[low(k, i)] * xk;
        __syncthreads();
    }
}

// The robust loss of an observation with squared residual length s = rx^2 + ry^2 and squared scale c2 = c^2 (DESIGN.md
// section 2): Cauchy's rho(s) = c2 log1p(s / c2), whose IRLS weight is rho'(s) = 1 / (1 + s / c2).  A solver scales the
// observation's residual and Jacobian rows by sqrt(weight) and sums rho in place of s for its cost; LOSS_NONE is rho(s) = s.
enum { LOSS_NONE = 0, LOSS_CAUCHY = 1 };
__device__ __forceinline__ double cauchy_weight(double s, double c2) { return 1.0 / (1.0 + s / c2); }
__device__ __forceinline__ double cauchy_rho(double s, double c2) { return c2 * log1p(s / c2); }

// The decision of iteration `it`, by one thread.  part [n][3]: the partials of the trial step (sum r^2 -- under a loss, sum rho -- of the trial state, twice
// the predicted reduction, |step|^2), summed here in ascending order, and only for a step that was solved; cam [2]: the
// camera step's share of the last two.  Gain ratio, accept (flip the buffer index) / reject, Nielsen's damping update, the
// four stops.  h = the history row (cost after the decision, the lambda the step was solved with, accepted, |step|).
__device__ __forceinline__ void lm_decide(LmState* st, const double* part, int n, const double* cam, int it, int max_iters, double ftol, double* h)
{
    const double lambda = st->lambda;
    bool accepted = false;
    double step = 0;
    int stop = 0;
    if (st->chol_fail) {
        if (st->chol_fail_prev) stop = RIG_STOP_CHOLESKY;
        st->chol_fail_prev = 1;
    } else {
        st->chol_fail_prev = 0;
        double c = 0, p = 0, n2 = 0;
        for (int b = 0; b < n; b++) { c += part[3 * (size_t)b]; p += part[3 * (size_t)b + 1]; n2 += part[3 * (size_t)b + 2]; }
        const double trial = 0.5 * c, pred = 0.5 * (p + cam[0]);
        step = sqrt(n2 + cam[1]);
        const double rho = (st->cost - trial) / pred;
        accepted = !st->trial_behind && rho > 0.0; // NaN: rejected
        if (accepted) {
            const double rel = (st->cost - trial) / st->cost, f = 2.0 * rho - 1.0, g = 1.0 - (f * f) * f;
            st->cost = trial; st->cur = 1 - st->cur;
            st->lambda = lambda * (g > 1.0 / 3.0 ? g : 1.0 / 3.0); st->nu = 2.0;
            if (rel < ftol) stop = RIG_STOP_FTOL;
        }
    }
    if (!accepted) {
        st->lambda = lambda * st->nu; st->nu = 2.0 * st->nu;
        if (!stop && st->lambda > 1e16) stop = RIG_STOP_LAMBDA;
    }
    if (!stop && it + 1 == max_iters) stop = RIG_STOP_MAX_ITERS;
    h[0] = st->cost; h[1] = lambda; h[2] = accepted ? 1.0 : 0.0; h[3] = step;
    st->iters = it + 1; st->chol_fail = 0; st->trial_behind = 0;
    if (stop) { st->stop = 1; st->status = stop; }
}

} // namespace mocap
