// intrinsics.hip -- intrinsic calibration of every camera of a rig from planar-board corner lists, on the device (FP64): per
// camera fx, fy, cx, cy, k1, k2, p1, p2, k3 and one pose per view, by Levenberg-Marquardt with a Schur complement on the views.
//
// Replaces reference CalculateCameraIntrinsic.py:58, cv2.calibrateCamera(objpoints, imgpoints, size, None, None), for all
// cameras in one call.  OpenCV's iteration is not reproduced: the contract is the definition of DESIGN.md section 2, restated in
// NumPy by tests/intrinsics_ref.py.  The camera model with its derivatives and the step-control rule are lm.h's, shared with
// rig_ba.hip; a board point is (X, Y, 0), and the third product of R X, an exact zero, is left out.
// The library is built with -ffp-contract=off: every product and sum below is rounded on its own.  No floating-point atomics
// anywhere: a view's sums run over its points in ascending order, a camera's over its views in ascending order, lanes join by
// the fixed shuffle tree of wave_sum.  Two runs give the same bits, and a camera's result does not depend on the cameras it is
// batched with: no kernel reads another camera's state.
//
// The data are small and ragged (3-12 views of 35-99 points per camera), so the unit of work is a view: one wavefront each.
// Initialisation (three launches, skipped when the caller hands a start in):
//   intr_begin_kernel       a workgroup per camera: the state record; the caller's start into buffer 0
//   intr_homography_kernel  a wave per view: Hartley-normalised DLT, the 45 sums of A^T A by the shuffle tree, its smallest
//                           eigenvector by the cyclic Jacobi of jacobi9.h on lane 0
//   intr_start_kernel       a workgroup per camera: 1 / fx^2 and 1 / fy^2 from two orthogonality constraints per view, the
//                           degeneracy test, the poses from K^-1 H
// One iteration is four stream-ordered launches; each returns at once for a camera whose state record says stop, so the host
// enqueues max_iters iterations and never waits between them:
//   intr_linearize_kernel   a wave per view: a lane owns a point, its 2 x 16 rows [J r] go to LDS; then a lane owns up to three
//                           of the 136 sums of [J r]^T [J r] and adds the points in order; V* = L L^T, W V*^-1, the view's
//                           9x9 and 9-vector for the Schur complement
//   intr_solve_kernel       a workgroup per camera: the views' records in ascending order into S and the reduced right-hand
//                           side; Cholesky of S, the camera step, the trial intrinsics
//   intr_update_kernel      a wave per view: back-substitution, the trial pose, the trial cost
//   intr_decide_kernel      a workgroup per camera: lm_decide (gain ratio, accept / reject, Nielsen's update, stops, history)
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "kernels.h"
#include "lm.h"
#include "jacobi9.h"

namespace mocap {

namespace {

__device__ __forceinline__ constexpr int up16(int i, int j) { return tri(i, j, 16); } // the view's 136 sums, i <= j

// In-place Cholesky A = L L^T on the packed lower triangle, column by column; every index a constant, the matrix in registers.
// False when a pivot is not positive and finite (the factor then holds NaN).
template <int N>
__device__ __forceinline__ bool cholesky(double* L)
{
    bool ok = true;
#pragma unroll
    for (int j = 0; j < N; j++) {
        double s = L[low(j, j)];
#pragma unroll
        for (int k = 0; k < j; k++) s = s - L[low(j, k)] * L[low(j, k)];
        ok = ok && s > 0.0 && finite(s);
        const double d = sqrt(s);
        L[low(j, j)] = d;
#pragma unroll
        for (int i = j + 1; i < N; i++) {
            double v = L[low(i, j)];
#pragma unroll
            for (int k = 0; k < j; k++) v = v - L[low(i, k)] * L[low(j, k)];
            L[low(i, j)] = v / d;
        }
    }
    return ok;
}

// L L^T x = b in place
template <int N>
__device__ __forceinline__ void cholesky_solve(const double* L, double* x)
{
#pragma unroll
    for (int i = 0; i < N; i++) {
        double s = x[i];
#pragma unroll
        for (int k = 0; k < i; k++) s = s - L[low(i, k)] * x[k];
        x[i] = s / L[low(i, i)];
    }
#pragma unroll
    for (int i = N - 1; i >= 0; i--) {
        double s = x[i];
#pragma unroll
        for (int k = i + 1; k < N; k++) s = s - L[low(k, i)] * x[k];
        x[i] = s / L[low(i, i)];
    }
}

// One board point under kd = (fx, fy, cx, cy, k1, k2, p1, p2, k3) and the pose P = (R row-major, t): residual r and, with JAC,
// the rows j0, j1 of its 2 x 15 Jacobian (kd's 9 columns, then the local pose perturbation R <- Exp(w) R, t <- t + dt: w, dt).
// Returns false when the point is not in front of the camera (z <= 0 or NaN).
template <bool JAC>
__device__ __forceinline__ bool observe_board(const double* kd, const double* P, double X, double Y, double ou, double ov, double r[2], double* j0, double* j1)
{
    const Lens m{kd[0], kd[1], kd[2], kd[3], kd[4], kd[5], kd[6], kd[7], kd[8]};
    const double q[3] = {P[0] * X + P[1] * Y, P[3] * X + P[4] * Y, P[6] * X + P[7] * Y};
    Projected o;
    const bool front = project<JAC>(m, q, P + 9, ou, ov, r, o);
    if (JAC) {
        lens_columns(m, o, j0, j1);
        pose_columns(o.A[0], q, j0 + 9);
        pose_columns(o.A[1], q, j1 + 9);
    }
    return front;
}

// the sum over the wave, in every lane
__device__ __forceinline__ double wave_sum_all(double v) { return __shfl(wave_sum(v), 0, 64); }

} // namespace

// A workgroup per camera.  The state records were zeroed.
__global__ __launch_bounds__(64) void intr_begin_kernel(IntrArgs a, int have_start, double lambda0)
{
    const int c = blockIdx.x, tid = threadIdx.x;
    IntrState* st = a.state + c;
    const bool bad = a.cam_bad[c] != 0;
    if (tid == 0) {
        st->lambda = lambda0; st->nu = 2.0;
        if (bad) { st->stop = 1; st->status = INTR_ERR_LAYOUT; }
    }
    if (bad || !have_start) return;
    if (tid < 9) a.kd[9 * (size_t)c + tid] = a.kd_io[9 * (size_t)c + tid];
    const int v0 = a.view_offset[c], v1 = a.view_offset[c + 1];
    for (int i = 12 * v0 + tid; i < 12 * v1; i += 64) a.poses[i] = a.poses_io[i];
}

// A wave per view: H with (u, v, 1) ~ H (X, Y, 1), H[2][2] = 1, from all the view's points.
__global__ __launch_bounds__(64) void intr_homography_kernel(IntrArgs a)
{
    __shared__ double s_V[81];
    const int v = blockIdx.x, lane = threadIdx.x;
    if (a.state[a.view_cam[v]].stop) return;
    const int p0 = a.point_offset[v], n = a.point_offset[v + 1] - p0;
    const double* obj = a.obj + 2 * (size_t)p0;
    const double* img = a.img + 2 * (size_t)p0;
    // Hartley's similarities: centroid to the origin, mean distance to it sqrt(2)
    double sx = 0, sy = 0, su = 0, sv = 0;
    for (int p = lane; p < n; p += 64) { sx += obj[2 * p]; sy += obj[2 * p + 1]; su += img[2 * p]; sv += img[2 * p + 1]; }
    const double mx = wave_sum_all(sx) / n, my = wave_sum_all(sy) / n, mu = wave_sum_all(su) / n, mv = wave_sum_all(sv) / n;
    double dso = 0, dsi = 0;
    for (int p = lane; p < n; p += 64) {
        const double dx = obj[2 * p] - mx, dy = obj[2 * p + 1] - my, du = img[2 * p] - mu, dv = img[2 * p + 1] - mv;
        dso += sqrt(dx * dx + dy * dy); dsi += sqrt(du * du + dv * dv);
    }
    const double so = sqrt(2.0) / (wave_sum_all(dso) / n), si = sqrt(2.0) / (wave_sum_all(dsi) / n);
    const double txo = -(so * mx), tyo = -(so * my), txi = -(si * mu), tyi = -(si * mv);
    // the two rows of a point: (-X, -Y, -1, 0, 0, 0, u X, u Y, u) and (0, 0, 0, -X, -Y, -1, v X, v Y, v)
    double B[45];
#pragma unroll
    for (int k = 0; k < 45; k++) B[k] = 0;
    for (int p = lane; p < n; p += 64) {
        const double X = so * obj[2 * p] + txo, Y = so * obj[2 * p + 1] + tyo, u = si * img[2 * p] + txi, w = si * img[2 * p + 1] + tyi;
        const double r0[9] = {-X, -Y, -1.0, 0.0, 0.0, 0.0, u * X, u * Y, u}, r1[9] = {0.0, 0.0, 0.0, -X, -Y, -1.0, w * X, w * Y, w};
#pragma unroll
        for (int i = 0; i < 9; i++)
#pragma unroll
            for (int j = i; j < 9; j++) B[sym9(i, j)] += r0[i] * r0[j] + r1[i] * r1[j];
    }
#pragma unroll
    for (int k = 0; k < 45; k++) B[k] = wave_sum(B[k]);
    if (lane != 0) return; // no barrier below
    double h[9];
    smallest_eigvec9(B, s_V, 1, h);
    // H = T_img^-1 H_n T_obj with T = [[s, 0, tx], [0, s, ty], [0, 0, 1]]
    double M[9], H[9];
#pragma unroll
    for (int i = 0; i < 3; i++) {
        M[3 * i] = h[3 * i] * so; M[3 * i + 1] = h[3 * i + 1] * so;
        M[3 * i + 2] = (h[3 * i] * txo + h[3 * i + 1] * tyo) + h[3 * i + 2];
    }
#pragma unroll
    for (int j = 0; j < 3; j++) {
        H[j] = (M[j] - txi * M[6 + j]) / si; H[3 + j] = (M[3 + j] - tyi * M[6 + j]) / si; H[6 + j] = M[6 + j];
    }
#pragma unroll
    for (int k = 0; k < 9; k++) a.H[9 * (size_t)v + k] = H[k] / H[8];
}

// A workgroup per camera: the start of the definition from the views' homographies, or INTR_ERR_DEGENERATE.
__global__ __launch_bounds__(64) void intr_start_kernel(IntrArgs a)
{
    __shared__ double s_f[2];
    __shared__ int s_ok;
    const int c = blockIdx.x, tid = threadIdx.x;
    IntrState* st = a.state + c;
    if (st->stop) return;
    const int v0 = a.view_offset[c], v1 = a.view_offset[c + 1];
    const double cx = (a.image_size[2 * c] - 1) * 0.5, cy = (a.image_size[2 * c + 1] - 1) * 0.5;
    if (tid == 0) {
        // per view two rows (a0 b0, a1 b1) (1 / fx^2, 1 / fy^2) = -a2 b2: for the first two columns of the centred homography,
        // and for their half-sum and half-difference, each of unit length; the 2x2 normal equations
        double m00 = 0, m01 = 0, m11 = 0, b0 = 0, b1 = 0;
        for (int v = v0; v < v1; v++) {
            const double* H = a.H + 9 * (size_t)v;
            double h[3], w[3], d1[3], d2[3];
            h[0] = H[0] - cx * H[6]; h[1] = H[3] - cy * H[6]; h[2] = H[6];
            w[0] = H[1] - cx * H[7]; w[1] = H[4] - cy * H[7]; w[2] = H[7];
            for (int k = 0; k < 3; k++) { d1[k] = (h[k] + w[k]) * 0.5; d2[k] = (h[k] - w[k]) * 0.5; }
            const double nh = sqrt((h[0] * h[0] + h[1] * h[1]) + h[2] * h[2]), nw = sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]);
            const double n1 = sqrt((d1[0] * d1[0] + d1[1] * d1[1]) + d1[2] * d1[2]), n2 = sqrt((d2[0] * d2[0] + d2[1] * d2[1]) + d2[2] * d2[2]);
            for (int k = 0; k < 3; k++) { h[k] = h[k] / nh; w[k] = w[k] / nw; d1[k] = d1[k] / n1; d2[k] = d2[k] / n2; }
            const double ra[2] = {h[0] * w[0], h[1] * w[1]}, rb[2] = {d1[0] * d2[0], d1[1] * d2[1]};
            const double ya = -(h[2] * w[2]), yb = -(d1[2] * d2[2]);
            m00 += ra[0] * ra[0] + rb[0] * rb[0]; m01 += ra[0] * ra[1] + rb[0] * rb[1]; m11 += ra[1] * ra[1] + rb[1] * rb[1];
            b0 += ra[0] * ya + rb[0] * yb; b1 += ra[1] * ya + rb[1] * yb;
        }
        const double det = m00 * m11 - m01 * m01, half = 0.5 * (m00 + m11);
        const double ia = (m11 * b0 - m01 * b1) / det, ib = (m00 * b1 - m01 * b0) / det;
        const bool ok = det > 1e-10 * (half * half) && finite(ia) && finite(ib) && ia > 0.0 && ib > 0.0;
        s_ok = ok;
        if (ok) {
            s_f[0] = sqrt(1.0 / ia); s_f[1] = sqrt(1.0 / ib);
            double* kd = a.kd + 9 * (size_t)c;
            kd[0] = s_f[0]; kd[1] = s_f[1]; kd[2] = cx; kd[3] = cy;
            for (int k = 4; k < 9; k++) kd[k] = 0.0;
        } else {
            st->stop = 1; st->status = INTR_ERR_DEGENERATE;
        }
    }
    __syncthreads();
    if (!s_ok) return;
    const double fx = s_f[0], fy = s_f[1];
    for (int v = v0 + tid; v < v1; v += 64) {
        // M = K^-1 H = (m1 m2 m3): s = 2 / (|m1| + |m2|) signed for t_z > 0; r1 = s m1, r3 = r1 x (s m2), both of unit length
        const double* H = a.H + 9 * (size_t)v;
        double m[3][3];
        for (int j = 0; j < 3; j++) { m[j][0] = (H[j] - cx * H[6 + j]) / fx; m[j][1] = (H[3 + j] - cy * H[6 + j]) / fy; m[j][2] = H[6 + j]; }
        const double n1 = sqrt((m[0][0] * m[0][0] + m[0][1] * m[0][1]) + m[0][2] * m[0][2]);
        const double n2 = sqrt((m[1][0] * m[1][0] + m[1][1] * m[1][1]) + m[1][2] * m[1][2]);
        double s = 2.0 / (n1 + n2);
        if (s * m[2][2] < 0.0) s = -s;
        double r1[3], b[3], r3[3], r2[3];
        for (int k = 0; k < 3; k++) { r1[k] = s * m[0][k]; b[k] = s * m[1][k]; }
        const double l1 = sqrt((r1[0] * r1[0] + r1[1] * r1[1]) + r1[2] * r1[2]);
        for (int k = 0; k < 3; k++) r1[k] = r1[k] / l1;
        r3[0] = r1[1] * b[2] - r1[2] * b[1]; r3[1] = r1[2] * b[0] - r1[0] * b[2]; r3[2] = r1[0] * b[1] - r1[1] * b[0];
        const double l3 = sqrt((r3[0] * r3[0] + r3[1] * r3[1]) + r3[2] * r3[2]);
        for (int k = 0; k < 3; k++) r3[k] = r3[k] / l3;
        r2[0] = r3[1] * r1[2] - r3[2] * r1[1]; r2[1] = r3[2] * r1[0] - r3[0] * r1[2]; r2[2] = r3[0] * r1[1] - r3[1] * r1[0];
        double* P = a.poses + 12 * (size_t)v;
        for (int k = 0; k < 3; k++) { P[3 * k] = r1[k]; P[3 * k + 1] = r2[k]; P[3 * k + 2] = r3[k]; P[9 + k] = s * m[2][k]; }
    }
}

// A wave per view.  it == 0: also the view's sum r^2 of the start state.
__global__ __launch_bounds__(64) void intr_linearize_kernel(IntrArgs a, int it)
{
    __shared__ double s_A[64][33]; // a point's rows [J r] of u (0..15) and of v (16..31); 33: the lanes' stores spread over the banks
    __shared__ double s_sum[136];
    __shared__ double s_L[21];
    __shared__ double s_Y[54];
    __shared__ int s_fail;
    const int v = blockIdx.x, lane = threadIdx.x, c = a.view_cam[v];
    IntrState* st = a.state + c;
    if (st->stop) return;
    const int cur = st->cur;
    const double lambda = st->lambda;
    const double* kd = a.kd + 9 * ((size_t)cur * a.n_cams + c);
    const double* P = a.poses + 12 * ((size_t)cur * a.n_views + v);
    const int p0 = a.point_offset[v], n = a.point_offset[v + 1] - p0;
    // the (up to) three of the 136 sums this lane owns: entry e = (i, j), i <= j, of the upper triangle row by row
    int ei[3], ej[3];
#pragma unroll
    for (int k = 0; k < 3; k++) tri_unrank(min(lane + 64 * k, 135), 16, ei[k], ej[k]);
    double acc[3] = {0, 0, 0};
    bool behind = false;
    for (int base = 0; base < n; base += 64) {
        const int cnt = n - base < 64 ? n - base : 64;
        __syncthreads(); // the previous chunk's rows have been read
        if (lane < cnt) {
            const size_t p = (size_t)p0 + base + lane;
            double r[2], j0[15], j1[15];
            behind = !observe_board<true>(kd, P, a.obj[2 * p], a.obj[2 * p + 1], a.img[2 * p], a.img[2 * p + 1], r, j0, j1) || behind;
#pragma unroll
            for (int k = 0; k < 15; k++) { s_A[lane][k] = j0[k]; s_A[lane][16 + k] = j1[k]; }
            s_A[lane][15] = r[0]; s_A[lane][31] = r[1];
        }
        __syncthreads();
        for (int p = 0; p < cnt; p++) {
            const double* A = s_A[p];
            acc[0] += A[ei[0]] * A[ej[0]] + A[16 + ei[0]] * A[16 + ej[0]];
            acc[1] += A[ei[1]] * A[ej[1]] + A[16 + ei[1]] * A[16 + ej[1]];
            if (lane < 8) acc[2] += A[ei[2]] * A[ej[2]] + A[16 + ei[2]] * A[16 + ej[2]];
        }
    }
    if (behind) atomicOr(&st->behind, 1);
    s_sum[lane] = acc[0]; s_sum[64 + lane] = acc[1];
    if (lane < 8) s_sum[128 + lane] = acc[2];
    __syncthreads();
    double* rec = a.rec + (size_t)INTR_REC * v;
    for (int e = lane; e < 136; e += 64) rec[INTR_REC_SUMS + e] = s_sum[e];
    if (lane < 6) a.gv[6 * (size_t)v + lane] = s_sum[up16(9 + lane, 15)];
    if (lane == 0) {
        if (it == 0) a.view_cost[(size_t)cur * a.n_views + v] = s_sum[135];
        // V* = V + lambda diag V = L L^T
        double L[21];
#pragma unroll
        for (int i = 0; i < 6; i++)
#pragma unroll
            for (int j = 0; j <= i; j++) {
                const double x = s_sum[up16(9 + j, 9 + i)];
                L[low(i, j)] = i == j ? x + lambda * x : x;
            }
        const bool ok = cholesky<6>(L);
#pragma unroll
        for (int k = 0; k < 21; k++) { s_L[k] = L[k]; rec[INTR_REC_L + k] = L[k]; }
        s_fail = !ok;
    }
    __syncthreads();
    if (s_fail) {
        if (lane == 0) atomicOr(&st->chol_fail, 1);
        return;
    }
    if (lane < 9) { // row `lane` of Y = W V*^-1
        double L[21], y[6];
#pragma unroll
        for (int k = 0; k < 21; k++) L[k] = s_L[k];
        const int row = lane * 16 - lane * (lane - 1) / 2 - lane; // W's row i sits at up16(i, 9 .. 14)
#pragma unroll
        for (int k = 0; k < 6; k++) y[k] = s_sum[row + 9 + k];
        cholesky_solve<6>(L, y);
#pragma unroll
        for (int k = 0; k < 6; k++) s_Y[6 * lane + k] = y[k];
    }
    __syncthreads();
    if (lane < 45) { // entry (i, j), i <= j, of Y W^T
        int i, j;
        tri_unrank(lane, 9, i, j);
        const int row = j * 16 - j * (j - 1) / 2 - j;
        double t = 0;
#pragma unroll
        for (int k = 0; k < 6; k++) t += s_Y[6 * i + k] * s_sum[row + 9 + k];
        rec[INTR_REC_T + lane] = t;
    } else if (lane < 54) { // Y g_v
        const int i = lane - 45;
        double t = 0;
#pragma unroll
        for (int k = 0; k < 6; k++) t += s_Y[6 * i + k] * s_sum[up16(9 + k, 15)];
        rec[INTR_REC_YG + i] = t;
    }
}

// A workgroup per camera.  solve == 0: S, the right-hand side, the gradient and the cost only (mocap_intrinsics_linearize).
__global__ __launch_bounds__(64) void intr_solve_kernel(IntrArgs a, int it, int solve)
{
    __shared__ double s_S[45], s_rhs[9], s_gc[9], s_cost;
    const int c = blockIdx.x, tid = threadIdx.x;
    IntrState* st = a.state + c;
    if (!solve && tid == 0) { a.lin_status[2 * c] = a.cam_bad[c] != 0; a.lin_status[2 * c + 1] = st->behind; }
    if (st->stop) return;
    const int v0 = a.view_offset[c], v1 = a.view_offset[c + 1];
    const double lambda = st->lambda;
    const bool view_fail = st->chol_fail != 0;
    if (tid < 45) { // entry (i, j), i <= j, of S = U* - sum_v W V*^-1 W^T: the views in ascending order
        int i, j;
        tri_unrank(tid, 9, i, j);
        double u = 0, t = 0;
        for (int v = v0; v < v1; v++) {
            const double* rec = a.rec + (size_t)INTR_REC * v;
            u = u + rec[INTR_REC_SUMS + i * 16 - i * (i - 1) / 2 + (j - i)];
            if (!view_fail) t = t + rec[INTR_REC_T + tid];
        }
        const double s = (i == j ? u + lambda * u : u) - t;
        s_S[tid] = s;
        a.S[81 * (size_t)c + 9 * i + j] = s; a.S[81 * (size_t)c + 9 * j + i] = s;
        if (i == j) a.udiag[9 * (size_t)c + i] = u;
    } else if (tid < 54) {
        const int i = tid - 45;
        double g = 0, y = 0;
        for (int v = v0; v < v1; v++) {
            const double* rec = a.rec + (size_t)INTR_REC * v;
            g = g + rec[INTR_REC_SUMS + i * 16 - i * (i - 1) / 2 + (15 - i)];
            if (!view_fail) y = y + rec[INTR_REC_YG + i];
        }
        s_rhs[i] = y - g; s_gc[i] = g;
        a.rhs[9 * (size_t)c + i] = y - g; a.gc[9 * (size_t)c + i] = g;
    } else if (tid == 54) {
        double s = 0;
        for (int v = v0; v < v1; v++) s = s + a.rec[(size_t)INTR_REC * v + INTR_REC_SUMS + 135];
        s_cost = 0.5 * s;
        a.lin_cost[c] = 0.5 * s;
    }
    __syncthreads();
    if (tid != 0) return;
    const double cost = s_cost;
    if (st->behind || !finite(cost)) { // the start (a trial state with this flaw is never accepted)
        if (solve) { st->stop = 1; st->status = INTR_ERR_BEHIND; st->cost = st->cost0 = cost; }
        return;
    }
    if (it == 0) st->cost = st->cost0 = cost;
    if (!solve || view_fail) return;
    double L[45], d[9];
#pragma unroll
    for (int i = 0; i < 9; i++)
#pragma unroll
        for (int j = 0; j <= i; j++) L[low(i, j)] = s_S[tri(j, i, 9)];
    if (!cholesky<9>(L)) { st->chol_fail = 1; return; }
#pragma unroll
    for (int i = 0; i < 9; i++) d[i] = s_rhs[i];
    cholesky_solve<9>(L, d);
    // the camera's part of the predicted reduction 1/2 d^T (lambda diag d - g) and of |d|^2; the trial intrinsics
    const double* kd = a.kd + 9 * ((size_t)st->cur * a.n_cams + c);
    double* trial = a.kd + 9 * ((size_t)(1 - st->cur) * a.n_cams + c);
    double pred = 0, n2 = 0;
#pragma unroll
    for (int i = 0; i < 9; i++) {
        pred += d[i] * ((lambda * a.udiag[9 * (size_t)c + i]) * d[i] - s_gc[i]);
        n2 += d[i] * d[i];
        a.delta_c[9 * (size_t)c + i] = d[i];
        trial[i] = kd[i] + d[i];
    }
    a.cam_part[2 * (size_t)c] = pred; a.cam_part[2 * (size_t)c + 1] = n2;
}

// A wave per view: dp = -V*^-1 (g_v + W^T d_c), the trial pose, the view's points under the trial state.
__global__ __launch_bounds__(64) void intr_update_kernel(IntrArgs a)
{
    __shared__ double s_P[12];
    const int v = blockIdx.x, lane = threadIdx.x, c = a.view_cam[v];
    IntrState* st = a.state + c;
    if (st->stop || st->chol_fail) return;
    const int cur = st->cur;
    const double lambda = st->lambda;
    const double* rec = a.rec + (size_t)INTR_REC * v;
    double pred = 0, n2 = 0;
    if (lane == 0) {
        const double* dc = a.delta_c + 9 * (size_t)c;
        double q[6], L[21];
#pragma unroll
        for (int k = 0; k < 6; k++) q[k] = rec[INTR_REC_SUMS + up16(9 + k, 15)];
#pragma unroll
        for (int i = 0; i < 9; i++)
#pragma unroll
            for (int k = 0; k < 6; k++) q[k] = q[k] + rec[INTR_REC_SUMS + up16(i, 9 + k)] * dc[i];
#pragma unroll
        for (int k = 0; k < 21; k++) L[k] = rec[INTR_REC_L + k];
        cholesky_solve<6>(L, q);
        double dp[6];
#pragma unroll
        for (int k = 0; k < 6; k++) {
            dp[k] = -q[k];
            pred += dp[k] * ((lambda * rec[INTR_REC_SUMS + up16(9 + k, 9 + k)]) * dp[k] - rec[INTR_REC_SUMS + up16(9 + k, 15)]);
            n2 += dp[k] * dp[k];
        }
        const double* P = a.poses + 12 * ((size_t)cur * a.n_views + v);
        double* T = a.poses + 12 * ((size_t)(1 - cur) * a.n_views + v);
        double R[9], Rn[9];
#pragma unroll
        for (int k = 0; k < 9; k++) R[k] = P[k];
        rotate_left(dp, R, Rn);
#pragma unroll
        for (int k = 0; k < 9; k++) { T[k] = Rn[k]; s_P[k] = Rn[k]; }
#pragma unroll
        for (int k = 0; k < 3; k++) { const double t = P[9 + k] + dp[3 + k]; T[9 + k] = t; s_P[9 + k] = t; }
    }
    __syncthreads();
    const double* kd = a.kd + 9 * ((size_t)(1 - cur) * a.n_cams + c);
    const int p0 = a.point_offset[v], n = a.point_offset[v + 1] - p0;
    double cost = 0;
    bool behind = false;
    for (int i = lane; i < n; i += 64) {
        const size_t p = (size_t)p0 + i;
        double r[2];
        behind = !observe_board<false>(kd, s_P, a.obj[2 * p], a.obj[2 * p + 1], a.img[2 * p], a.img[2 * p + 1], r, nullptr, nullptr) || behind;
        cost += r[0] * r[0] + r[1] * r[1];
    }
    if (behind) atomicOr(&st->trial_behind, 1);
    const double total = wave_sum(cost);
    if (lane == 0) {
        a.upd_part[3 * (size_t)v] = total; a.upd_part[3 * (size_t)v + 1] = pred; a.upd_part[3 * (size_t)v + 2] = n2;
        a.view_cost[(size_t)(1 - cur) * a.n_views + v] = total;
    }
}

// A workgroup per camera: one thread decides by lm_decide over the partials of the camera's views.  history[c][it] is its row.
__global__ __launch_bounds__(64) void intr_decide_kernel(IntrArgs a, int it, double ftol)
{
    const int c = blockIdx.x;
    IntrState* st = a.state + c;
    if (st->stop || threadIdx.x != 0) return;
    const int v0 = a.view_offset[c], v1 = a.view_offset[c + 1];
    lm_decide(st, a.upd_part + 3 * (size_t)v0, v1 - v0, a.cam_part + 2 * (size_t)c, it, a.max_iters, ftol, a.history + 4 * ((size_t)c * a.max_iters + it));
}

// The record, and for a camera with a positive status the caller's arrays; a failed camera's stay as they were.
__global__ __launch_bounds__(256) void intr_finish_kernel(IntrArgs a)
{
    const int gid = blockIdx.x * 256 + threadIdx.x, stride = gridDim.x * 256;
    for (int c = gid; c < a.n_cams; c += stride) {
        const IntrState* st = a.state + c;
        double* r = a.result + 4 * (size_t)c;
        r[0] = (double)st->status; r[1] = (double)st->iters; r[2] = st->cost0; r[3] = st->cost;
        if (st->status > 0)
            for (int k = 0; k < 9; k++) a.kd_io[9 * (size_t)c + k] = a.kd[9 * ((size_t)st->cur * a.n_cams + c) + k];
    }
    for (int v = gid; v < a.n_views; v += stride) {
        const IntrState* st = a.state + a.view_cam[v];
        if (st->status > 0) {
            for (int k = 0; k < 12; k++) a.poses_io[12 * (size_t)v + k] = a.poses[12 * ((size_t)st->cur * a.n_views + v) + k];
            a.view_rms[v] = sqrt(a.view_cost[(size_t)st->cur * a.n_views + v] / (a.point_offset[v + 1] - a.point_offset[v]));
        } else {
            a.view_rms[v] = __builtin_nan("");
        }
    }
}

void launch_intr_begin(const IntrArgs& a, int have_start, double lambda0, hipStream_t s)
{
    hipLaunchKernelGGL(intr_begin_kernel, dim3(a.n_cams), dim3(64), 0, s, a, have_start, lambda0);
    if (have_start) return;
    hipLaunchKernelGGL(intr_homography_kernel, dim3(a.n_views), dim3(64), 0, s, a);
    hipLaunchKernelGGL(intr_start_kernel, dim3(a.n_cams), dim3(64), 0, s, a);
}

void launch_intr_linearize(const IntrArgs& a, int it, bool solve, hipStream_t s)
{
    hipLaunchKernelGGL(intr_linearize_kernel, dim3(a.n_views), dim3(64), 0, s, a, it);
    hipLaunchKernelGGL(intr_solve_kernel, dim3(a.n_cams), dim3(64), 0, s, a, it, solve ? 1 : 0);
}

void launch_intr_iteration(const IntrArgs& a, int it, double ftol, hipStream_t s)
{
    launch_intr_linearize(a, it, true, s);
    hipLaunchKernelGGL(intr_update_kernel, dim3(a.n_views), dim3(64), 0, s, a);
    hipLaunchKernelGGL(intr_decide_kernel, dim3(a.n_cams), dim3(64), 0, s, a, it, ftol);
}

void launch_intr_finish(const IntrArgs& a, hipStream_t s)
{
    const int most = a.n_views > a.n_cams ? a.n_views : a.n_cams;
    int g = (most + 255) / 256;
    hipLaunchKernelGGL(intr_finish_kernel, dim3(g > 1024 ? 1024 : g), dim3(256), 0, s, a);
}

} // namespace mocap
