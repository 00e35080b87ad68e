// rig_ba.hip -- bundle adjustment of a whole rig on the device (FP64): the poses of cameras 1..C-1 and every 3-D point over
// exactly the observations that exist, by sparse Levenberg-Marquardt with a Schur complement on the points.
//
// Generalises reference lib/Helpers.py:158-176 (bundle_adjustment: SciPy over the 6 parameters of camera 1, every point
// re-triangulated per evaluation, points any camera missed dropped).  The reference has no N-camera counterpart: the contract
// is the definition of DESIGN.md section 2, restated in NumPy by tests/rig_ba_ref.py.  Observations are point-major
// (obs_offset [N + 1], obs_cam, obs_uv), a point's cameras in ascending order; rig_init_kernel checks that and turns each
// point's camera list into a 32-bit visibility mask, which is all the later kernels index with.
// The camera model with its derivatives and the step-control rule are lm.h's, shared with intrinsics.hip; the inverse of a
// point's 3x3 and the packed Cholesky of the reduced matrix are lm.h's too, shared with rig_selfcal.hip.
// The library is built with -ffp-contract=off: every product and sum below is rounded on its own, and the restatement forms
// every per-observation quantity by the same operations in the same order.  What differs is the order of the sums over
// observations and points, which is fixed here: no floating-point atomics anywhere, a lane sums its own points in order,
// lanes join by a fixed shuffle tree, waves and workgroups in ascending order.  Two runs give the same bits.
//
// One iteration is six stream-ordered launches; each returns at once when the state record says stop, so the host enqueues
// max_iters iterations and never waits between them:
//   rig_linearize_kernel  a lane owns a point: residuals, analytic Jacobian, V_n, g_n and the cost in registers, the W blocks
//                         to scratch; camera blocks U_c, g_c summed per workgroup (shuffle tree, waves through LDS)
//   rig_schur_kernel      grid (camera pair a <= b, chunk of points): the 6x6 blocks W_a V*^-1 W_b^T and, on the diagonal,
//                         W_a V*^-1 g_n, summed per workgroup
//   rig_reduce_kernel     one workgroup per camera pair: the partials in ascending order into S = U* - sum, the reduced
//                         right-hand side, the camera gradient; the cost
//   rig_solve_kernel      one workgroup: Cholesky of S (packed lower triangle: in LDS up to 90 rows, else in global memory),
//                         the camera step, the trial poses
//   rig_update_kernel     a lane owns a point: back-substitution, trial point, trial cost, predicted reduction
//   rig_decide_kernel     one workgroup: lm_decide (gain ratio, accept / reject, Nielsen's damping update, the stops, history)
// The two point-owning kernels take the loss (lm.h) as a template parameter.  With LOSS_CAUCHY an observation's residual and
// Jacobian rows are scaled by sqrt(w), w = 1 / (1 + s / c^2), before anything is formed from them, and the costs sum rho(s) in
// place of s (first-order IRLS); everything downstream reads the scaled blocks and does not know.  LOSS_NONE compiles to the
// code without a loss.  After the loop rig_finish_kernel hands the state back and rig_residuals_kernel (a lane owns a point)
// writes every observation's |r| and weight at that returned state.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "kernels.h"
#include "lm.h"

namespace mocap {

namespace {

constexpr int PT_THREADS = 256;     // points per workgroup of the point-owning kernels (linearize, update)
constexpr int SCHUR_CHUNK = 1024;   // points per workgroup of rig_schur_kernel
constexpr int CHOL_LDS_ROWS = 90;   // 90 * 91 / 2 doubles = 32 760 bytes: C <= 16 factorises in LDS

struct Cam { double R[9], t[3]; Lens lens; };

__device__ __forceinline__ Cam load_cam(const CameraTable* tab, const double* pose, int c)
{
    Cam m;
#pragma unroll
    for (int k = 0; k < 9; k++) m.R[k] = pose[12 * c + k];
#pragma unroll
    for (int k = 0; k < 3; k++) m.t[k] = pose[12 * c + 9 + k];
    m.lens = Lens{tab->K[c][0], tab->K[c][4], tab->K[c][2], tab->K[c][5],
                  tab->dist[c][0], tab->dist[c][1], tab->dist[c][2], tab->dist[c][3], tab->dist[c][4]};
    return m;
}

// One observation: residual r, and with JAC the 2x6 camera Jacobian jc (local pose perturbation R <- Exp(w) R, t <- t + dt:
// columns w, dt) and the 2x3 point Jacobian jp = A R.  Returns false when the point is not in front of the camera (z <= 0 or NaN).
template <bool JAC>
__device__ __forceinline__ bool observe(const Cam& m, const double X[3], double ou, double ov, double r[2], double jc[2][6], double jp[2][3])
{
    const double q[3] = {(m.R[0] * X[0] + m.R[1] * X[1]) + m.R[2] * X[2], (m.R[3] * X[0] + m.R[4] * X[1]) + m.R[5] * X[2],
                         (m.R[6] * X[0] + m.R[7] * X[1]) + m.R[8] * X[2]};
    Projected o;
    const bool front = project<JAC>(m.lens, q, m.t, ou, ov, r, o);
    if (JAC) {
#pragma unroll
        for (int i = 0; i < 2; i++) {
#pragma unroll
            for (int j = 0; j < 3; j++) jp[i][j] = (o.A[i][0] * m.R[j] + o.A[i][1] * m.R[3 + j]) + o.A[i][2] * m.R[6 + j];
            pose_columns(o.A[i], q, jc[i]);
        }
    }
    return front;
}

// The loss's part of an observation: its share of the cost from the unscaled r, and with JAC r, jc, jp scaled by sqrt(weight)
template <int LOSS, bool JAC>
__device__ __forceinline__ double robustify(double c2, double r[2], double jc[2][6], double jp[2][3])
{
    const double s = r[0] * r[0] + r[1] * r[1];
    if (LOSS == LOSS_NONE) return s;
    if (JAC) {
        const double sw = sqrt(cauchy_weight(s, c2));
#pragma unroll
        for (int i = 0; i < 2; i++) {
            r[i] *= sw;
#pragma unroll
            for (int j = 0; j < 6; j++) jc[i][j] *= sw;
#pragma unroll
            for (int j = 0; j < 3; j++) jp[i][j] *= sw;
        }
    }
    return cauchy_rho(s, c2);
}

// the pair of free cameras of a workgroup of the Schur and the reduce kernel: pair index -> (ca, cb), 1 <= ca <= cb < C, row by row
__device__ __forceinline__ void pair_cameras(int pair, int C, int& ca, int& cb) { tri_unrank(pair, C - 1, ca, cb); ca++; cb++; }

__device__ __forceinline__ bool gated(const RigState* st) { return st->stop || st->layout_err; }

} // namespace

// Copies the caller's state into buffer 0, builds the visibility masks and checks the layout (a violation is reported as
// MOCAP_RIG_E_LAYOUT; nothing later reads the observation arrays through an unchecked index).  The state record was zeroed.
__global__ __launch_bounds__(256) void rig_init_kernel(RigArgs a, double lambda0)
{
    const int gid = blockIdx.x * 256 + threadIdx.x, stride = gridDim.x * 256;
    RigState* st = a.state;
    if (gid == 0) {
        st->lambda = lambda0; st->nu = 2.0;
        const double* t1 = a.poses_io + 12 + 9;
        st->t1_norm = sqrt((t1[0] * t1[0] + t1[1] * t1[1]) + t1[2] * t1[2]);
        if (a.obs_offset[0] != 0 || a.obs_offset[a.N] != a.n_obs) atomicOr(&st->layout_err, 1);
    }
    for (int i = gid; i < 12 * a.C; i += stride) a.poses[i] = i < 12 ? ((i == 0 || i == 4 || i == 8) ? 1.0 : 0.0) : a.poses_io[i];
    for (int i = gid; i < 3 * a.N; i += stride) a.points[i] = a.points_io[i];
    for (int n = gid; n < a.N; n += stride) {
        const int o0 = a.obs_offset[n], o1 = a.obs_offset[n + 1];
        uint32_t mask = 0;
        bool ok = o0 >= 0 && o1 <= a.n_obs && o1 - o0 >= 2 && o1 - o0 <= a.C;
        if (ok) {
            int prev = -1;
            for (int o = o0; o < o1; o++) {
                const int c = a.obs_cam[o];
                ok = ok && c > prev && c < a.C;
                prev = c;
                if (ok) mask |= 1u << c;
            }
        }
        a.mask[n] = ok ? mask : 0u;
        if (!ok) atomicOr(&st->layout_err, 1);
    }
}

// A lane owns a point.  Grid: ceil(N / 256).
template <int LOSS>
__global__ __launch_bounds__(PT_THREADS) void rig_linearize_kernel(RigArgs a)
{
    __shared__ double s_red[2][4][27];
    __shared__ double s_part[4];
    RigState* st = a.state;
    if (gated(st)) return;
    const int tid = threadIdx.x, n = blockIdx.x * PT_THREADS + tid, lane = tid & 63, wave = tid >> 6;
    const bool live = n < a.N;
    const double* pose = a.poses + (size_t)st->cur * 12 * a.C;
    const double* pts = a.points + (size_t)st->cur * 3 * a.N;
    const double lambda = st->lambda;
    double X[3] = {0, 0, 0};
    uint32_t mask = 0;
    int o = 0;
    if (live) {
        X[0] = pts[3 * n]; X[1] = pts[3 * n + 1]; X[2] = pts[3 * n + 2];
        mask = a.mask[n]; o = a.obs_offset[n];
    }
    double V[6] = {0, 0, 0, 0, 0, 0}, gp[3] = {0, 0, 0}, cost = 0;
    bool behind = false;
    for (int c = 0; c < a.C; c++) { // uniform over the workgroup
        const bool has = (mask >> c) & 1u;
        double r[2] = {0, 0}, jc[2][6], jp[2][3];
#pragma unroll
        for (int i = 0; i < 2; i++) {
#pragma unroll
            for (int j = 0; j < 6; j++) jc[i][j] = 0;
#pragma unroll
            for (int j = 0; j < 3; j++) jp[i][j] = 0;
        }
        if (has) {
            const Cam m = load_cam(a.cams, pose, c);
            behind = !observe<true>(m, X, a.obs_uv[2 * (size_t)o], a.obs_uv[2 * (size_t)o + 1], r, jc, jp) || behind;
            cost += robustify<LOSS, true>(a.loss_c2, r, jc, jp);
            int k = 0;
#pragma unroll
            for (int i = 0; i < 3; i++) {
                gp[i] += jp[0][i] * r[0] + jp[1][i] * r[1];
#pragma unroll
                for (int j = i; j < 3; j++) V[k++] += jp[0][i] * jp[0][j] + jp[1][i] * jp[1][j];
            }
            if (c > 0) {
                double* W = a.W + 18 * (size_t)o;
#pragma unroll
                for (int i = 0; i < 6; i++)
#pragma unroll
                    for (int j = 0; j < 3; j++) W[3 * i + j] = jc[0][i] * jp[0][j] + jc[1][i] * jp[1][j];
            }
            o++;
        }
        if (c == 0) continue; // camera 0 is fixed
        // U_c (21 sums) and g_c (6) of this workgroup's points; a lane without the camera adds zeros
        double* red = s_red[c & 1][wave];
        {
            int k = 0;
#pragma unroll
            for (int i = 0; i < 6; i++)
#pragma unroll
                for (int j = i; j < 6; j++) {
                    const double v = wave_sum(jc[0][i] * jc[0][j] + jc[1][i] * jc[1][j]);
                    if (lane == 0) red[k] = v;
                    k++;
                }
#pragma unroll
            for (int i = 0; i < 6; i++) {
                const double v = wave_sum(jc[0][i] * r[0] + jc[1][i] * r[1]);
                if (lane == 0) red[21 + i] = v;
            }
        }
        __syncthreads(); // (the buffer of camera c - 1 is free again after this barrier: two buffers, one barrier per camera)
        if (tid < 27)
            a.lin_part[((size_t)blockIdx.x * (a.C - 1) + (c - 1)) * 27 + tid] =
                (s_red[c & 1][0][tid] + s_red[c & 1][1][tid]) + (s_red[c & 1][2][tid] + s_red[c & 1][3][tid]);
    }
    if (live) {
        // damped inverse V*^-1 (V_ii + lambda V_ii on the diagonal), the undamped diagonal and the gradient
        const double Vd[6] = {V[0] + lambda * V[0], V[1], V[2], V[3] + lambda * V[3], V[4], V[5] + lambda * V[5]};
        double inv[6];
        inv_sym3(Vd, inv);
#pragma unroll
        for (int k = 0; k < 6; k++) a.Vinv[6 * (size_t)n + k] = inv[k];
        a.vdiag[3 * (size_t)n] = V[0]; a.vdiag[3 * (size_t)n + 1] = V[3]; a.vdiag[3 * (size_t)n + 2] = V[5];
#pragma unroll
        for (int k = 0; k < 3; k++) a.gp[3 * (size_t)n + k] = gp[k];
    }
    if (behind) atomicOr(&st->behind, 1);
    const double total = block_sum(cost, s_part);
    if (tid == 0) a.cost_part[blockIdx.x] = total;
}

// Grid (pair of free cameras a <= b, chunk of SCHUR_CHUNK points).  A thread walks the points tid, tid + 256, ... of the chunk;
// a point seen by both cameras adds W_a V*^-1 W_b^T (36 sums) and, for a == b, W_a V*^-1 g_n (6).
__global__ __launch_bounds__(256) void rig_schur_kernel(RigArgs a)
{
    __shared__ double s_red[4][42];
    if (gated(a.state)) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, pair = blockIdx.x, chunk = blockIdx.y;
    int ca, cb;
    pair_cameras(pair, a.C, ca, cb);
    const bool diag = ca == cb;
    const uint32_t both = (1u << ca) | (1u << cb);
    double acc[42];
#pragma unroll
    for (int k = 0; k < 42; k++) acc[k] = 0;
    const int n0 = chunk * SCHUR_CHUNK, n1 = n0 + SCHUR_CHUNK < a.N ? n0 + SCHUR_CHUNK : a.N;
    for (int n = n0 + tid; n < n1; n += 256) {
        const uint32_t mask = a.mask[n];
        if ((mask & both) != both) continue;
        const int o0 = a.obs_offset[n];
        const double* Wa = a.W + 18 * (size_t)(o0 + __popc(mask & ((1u << ca) - 1u)));
        const double* Wb = a.W + 18 * (size_t)(o0 + __popc(mask & ((1u << cb) - 1u)));
        double inv[6];
#pragma unroll
        for (int k = 0; k < 6; k++) inv[k] = a.Vinv[6 * (size_t)n + k];
        double wb[18];
#pragma unroll
        for (int k = 0; k < 18; k++) wb[k] = Wb[k];
        const double g0 = a.gp[3 * (size_t)n], g1 = a.gp[3 * (size_t)n + 1], g2 = a.gp[3 * (size_t)n + 2];
#pragma unroll
        for (int i = 0; i < 6; i++) {
            const double w0 = Wa[3 * i], w1 = Wa[3 * i + 1], w2 = Wa[3 * i + 2];
            double Y[3];
#pragma unroll
            for (int j = 0; j < 3; j++) Y[j] = (w0 * sym3(inv, 0, j) + w1 * sym3(inv, 1, j)) + w2 * sym3(inv, 2, j);
#pragma unroll
            for (int j = 0; j < 6; j++) acc[6 * i + j] += (Y[0] * wb[3 * j] + Y[1] * wb[3 * j + 1]) + Y[2] * wb[3 * j + 2];
            if (diag) acc[36 + i] += (Y[0] * g0 + Y[1] * g1) + Y[2] * g2;
        }
    }
#pragma unroll
    for (int k = 0; k < 42; k++) {
        const double v = wave_sum(acc[k]);
        if (lane == 0) s_red[wave][k] = v;
    }
    __syncthreads();
    if (tid < 42)
        a.schur_part[((size_t)chunk * a.n_pairs + pair) * 42 + tid] = (s_red[0][tid] + s_red[1][tid]) + (s_red[2][tid] + s_red[3][tid]);
}

// One workgroup (64 threads) per pair of free cameras: every partial in ascending order.
__global__ __launch_bounds__(64) void rig_reduce_kernel(RigArgs a)
{
    __shared__ double s_u[27];
    __shared__ double s_blk[36];
    if (gated(a.state)) return;
    const int tid = threadIdx.x, pair = blockIdx.x, D = 6 * (a.C - 1);
    int ca, cb;
    pair_cameras(pair, a.C, ca, cb);
    const bool diag = ca == cb;
    const double lambda = a.state->lambda;
    if (diag && tid < 27) {
        double s = 0;
        for (int b = 0; b < a.n_lin_blocks; b++) s += a.lin_part[((size_t)b * (a.C - 1) + (ca - 1)) * 27 + tid];
        s_u[tid] = s;
    }
    double sum = 0;
    if (tid < 42)
        for (int ch = 0; ch < a.n_chunks; ch++) sum += a.schur_part[((size_t)ch * a.n_pairs + pair) * 42 + tid];
    __syncthreads();
    if (tid < 36) {
        const int i = tid / 6, j = tid % 6;
        double u = 0;
        if (diag) {
            u = s_u[i <= j ? tri(i, j, 6) : tri(j, i, 6)];
            if (i == j) u = u + lambda * u;
        }
        s_blk[tid] = u - sum;
    }
    __syncthreads();
    if (tid < 36) {
        const int i = tid / 6, j = tid % 6, ra = 6 * (ca - 1), rb = 6 * (cb - 1);
        if (diag) a.S[(size_t)(ra + i) * D + ra + j] = s_blk[i <= j ? tid : 6 * j + i]; // the upper triangle, mirrored
        else { a.S[(size_t)(ra + i) * D + rb + j] = s_blk[tid]; a.S[(size_t)(rb + j) * D + ra + i] = s_blk[tid]; }
    } else if (tid < 42 && diag) {
        const int i = tid - 36, row = 6 * (ca - 1) + i;
        a.rhs[row] = sum - s_u[21 + i];
        a.gc[row] = s_u[21 + i];
        a.udiag[row] = s_u[tri(i, i, 6)];
    }
    if (pair == 0 && tid == 63) {
        double s = 0;
        for (int b = 0; b < a.n_lin_blocks; b++) s += a.cost_part[b];
        a.scalars[RIG_LIN_COST] = 0.5 * s;
    }
}

// One workgroup.  Also the keeper of the state record's first cost, and of the two failures a linearisation can show.
__global__ __launch_bounds__(256) void rig_solve_kernel(RigArgs a, int it)
{
    __shared__ double s_L[CHOL_LDS_ROWS * (CHOL_LDS_ROWS + 1) / 2];
    __shared__ double s_x[6 * 31];
    RigState* st = a.state;
    if (gated(st)) return;
    const int tid = threadIdx.x, D = 6 * (a.C - 1);
    const double cost = a.scalars[RIG_LIN_COST];
    if (st->behind || !finite(cost)) { // the state handed in (a trial state with this flaw is never accepted)
        __syncthreads();
        if (tid == 0) { st->stop = 1; st->status = RIG_ERR_BEHIND; st->cost = st->cost0 = cost; }
        return;
    }
    if (it == 0 && tid == 0) st->cost = st->cost0 = cost;
    double* L = D <= CHOL_LDS_ROWS ? s_L : a.chol;
    for (int e = tid; e < D * (D + 1) / 2; e += 256) {
        int i = (int)((sqrt(8.0 * e + 1.0) - 1.0) * 0.5);
        while (low(i, 0) > e) i--;
        while (low(i + 1, 0) <= e) i++;
        L[e] = a.S[(size_t)i * D + (e - low(i, 0))];
    }
    for (int i = tid; i < D; i += 256) s_x[i] = a.rhs[i];
    const bool ok = D <= CHOL_LDS_ROWS ? cholesky_packed(s_L, D) : cholesky_packed(a.chol, D);
    if (!ok) {
        if (tid == 0) st->chol_fail = 1;
        return;
    }
    if (D <= CHOL_LDS_ROWS) solve_packed(s_L, D, s_x); else solve_packed(a.chol, D, s_x);
    const double lambda = st->lambda;
    for (int i = tid; i < D; i += 256) a.delta_c[i] = s_x[i];
    if (tid == 0) { // the cameras' part of the predicted reduction 1/2 d^T (lambda diag d - g) and of |d|^2
        double pred = 0, n2 = 0;
        for (int i = 0; i < D; i++) {
            const double d = s_x[i];
            pred += d * ((lambda * a.udiag[i]) * d - a.gc[i]);
            n2 += d * d;
        }
        a.scalars[RIG_PRED_CAM] = pred; a.scalars[RIG_NORM2_CAM] = n2;
    }
    // trial poses into the other buffer
    const double* pose = a.poses + (size_t)st->cur * 12 * a.C;
    double* trial = a.poses + (size_t)(1 - st->cur) * 12 * a.C;
    if (tid < a.C) {
        if (tid == 0) {
            for (int k = 0; k < 12; k++) trial[k] = pose[k];
        } else {
            const double* d = s_x + 6 * (tid - 1);
            double R[9], Rn[9];
            for (int k = 0; k < 9; k++) R[k] = pose[12 * tid + k];
            rotate_left(d, R, Rn);
            for (int k = 0; k < 9; k++) trial[12 * tid + k] = Rn[k];
            for (int k = 0; k < 3; k++) trial[12 * tid + 9 + k] = pose[12 * tid + 9 + k] + d[3 + k];
        }
    }
}

// A lane owns a point: dX = -V*^-1 (g_n + sum_c W_nc^T d_c), the trial point, its observations under the trial poses.
template <int LOSS>
__global__ __launch_bounds__(PT_THREADS) void rig_update_kernel(RigArgs a)
{
    __shared__ double s_d[6 * 31];
    __shared__ double s_part[4];
    RigState* st = a.state;
    if (gated(st) || st->chol_fail) return;
    const int tid = threadIdx.x, n = blockIdx.x * PT_THREADS + tid, D = 6 * (a.C - 1);
    for (int i = tid; i < D; i += PT_THREADS) s_d[i] = a.delta_c[i];
    __syncthreads();
    const double* pts = a.points + (size_t)st->cur * 3 * a.N;
    double* trial_pts = a.points + (size_t)(1 - st->cur) * 3 * a.N;
    const double* trial_pose = a.poses + (size_t)(1 - st->cur) * 12 * a.C;
    const double lambda = st->lambda;
    double cost = 0, pred = 0, n2 = 0;
    bool behind = false;
    if (n < a.N) {
        const uint32_t mask = a.mask[n];
        const int o0 = a.obs_offset[n];
        double q[3], inv[6], X[3];
#pragma unroll
        for (int k = 0; k < 3; k++) q[k] = a.gp[3 * (size_t)n + k];
#pragma unroll
        for (int k = 0; k < 6; k++) inv[k] = a.Vinv[6 * (size_t)n + k];
        int o = o0;
        for (uint32_t m = mask; m; m &= m - 1, o++) {
            const int c = __ffs(m) - 1;
            if (c == 0) continue;
            const double* W = a.W + 18 * (size_t)o;
            const double* d = s_d + 6 * (c - 1);
#pragma unroll
            for (int j = 0; j < 3; j++)
                q[j] += ((((W[j] * d[0] + W[3 + j] * d[1]) + W[6 + j] * d[2]) + W[9 + j] * d[3]) + W[12 + j] * d[4]) + W[15 + j] * d[5];
        }
#pragma unroll
        for (int i = 0; i < 3; i++) {
            const double dx = -((sym3(inv, i, 0) * q[0] + sym3(inv, i, 1) * q[1]) + sym3(inv, i, 2) * q[2]);
            X[i] = pts[3 * n + i] + dx;
            trial_pts[3 * n + i] = X[i];
            pred += dx * ((lambda * a.vdiag[3 * (size_t)n + i]) * dx - a.gp[3 * (size_t)n + i]);
            n2 += dx * dx;
        }
        o = o0;
        for (uint32_t m = mask; m; m &= m - 1, o++) {
            const int c = __ffs(m) - 1;
            const Cam cam = load_cam(a.cams, trial_pose, c);
            double r[2];
            behind = !observe<false>(cam, X, a.obs_uv[2 * (size_t)o], a.obs_uv[2 * (size_t)o + 1], r, nullptr, nullptr) || behind;
            cost += robustify<LOSS, false>(a.loss_c2, r, nullptr, nullptr);
        }
    }
    if (behind) atomicOr(&st->trial_behind, 1);
    const double c_sum = block_sum(cost, s_part), p_sum = block_sum(pred, s_part), n_sum = block_sum(n2, s_part);
    if (tid == 0) {
        a.upd_part[3 * (size_t)blockIdx.x] = c_sum; a.upd_part[3 * (size_t)blockIdx.x + 1] = p_sum; a.upd_part[3 * (size_t)blockIdx.x + 2] = n_sum;
    }
}

// One thread decides by lm_decide over the partials of the point kernel's workgroups.  history[it] is its row.
__global__ __launch_bounds__(64) void rig_decide_kernel(RigArgs a, int it, int max_iters, double ftol)
{
    RigState* st = a.state;
    if (gated(st) || threadIdx.x != 0) return;
    lm_decide(st, a.upd_part, a.n_lin_blocks, a.scalars + RIG_PRED_CAM, it, max_iters, ftol, a.history + 4 * (size_t)it);
}

// The gauge on return (every t and every X scaled so that |t_1| is what it was at the start), the caller's arrays, the record.
__global__ __launch_bounds__(256) void rig_finish_kernel(RigArgs a)
{
    const int gid = blockIdx.x * 256 + threadIdx.x, stride = gridDim.x * 256;
    const RigState* st = a.state;
    if (gid == 0) {
        a.result[0] = st->layout_err ? (double)RIG_ERR_LAYOUT : (double)st->status;
        a.result[1] = (double)st->iters; a.result[2] = st->cost0; a.result[3] = st->cost;
    }
    if (st->layout_err || st->status < 0) return; // the caller's arrays stay as they were
    const double* pose = a.poses + (size_t)st->cur * 12 * a.C;
    const double* pts = a.points + (size_t)st->cur * 3 * a.N;
    const double* t1 = pose + 12 + 9;
    const double now = sqrt((t1[0] * t1[0] + t1[1] * t1[1]) + t1[2] * t1[2]);
    double s = st->t1_norm / now;
    if (!(s > 0.0) || !finite(s)) s = 1.0; // |t_1| = 0 at either end: no scale to restore
    for (int i = gid; i < 12 * a.C; i += stride) a.poses_io[i] = i % 12 < 9 ? pose[i] : pose[i] * s;
    for (int i = gid; i < 3 * a.N; i += stride) a.points_io[i] = pts[i] * s;
}

// A lane owns a point: the length of every observation's unweighted residual and the loss's weight, at the state
// rig_finish_kernel handed back (the caller's arrays; a negative status: nothing is written, the outputs were zeroed).
template <int LOSS>
__global__ __launch_bounds__(PT_THREADS) void rig_residuals_kernel(RigArgs a)
{
    const RigState* st = a.state;
    if (st->layout_err || st->status < 0) return;
    const int n = blockIdx.x * PT_THREADS + threadIdx.x;
    if (n >= a.N) return;
    const double X[3] = {a.points_io[3 * (size_t)n], a.points_io[3 * (size_t)n + 1], a.points_io[3 * (size_t)n + 2]};
    int o = a.obs_offset[n];
    for (uint32_t m = a.mask[n]; m; m &= m - 1, o++) {
        const Cam cam = load_cam(a.cams, a.poses_io, __ffs(m) - 1);
        double r[2];
        observe<false>(cam, X, a.obs_uv[2 * (size_t)o], a.obs_uv[2 * (size_t)o + 1], r, nullptr, nullptr);
        const double s = r[0] * r[0] + r[1] * r[1];
        if (a.obs_err) a.obs_err[o] = sqrt(s);
        if (a.obs_weight) a.obs_weight[o] = LOSS == LOSS_NONE ? 1.0 : cauchy_weight(s, a.loss_c2);
    }
}

static int grid_for(int n) { int g = (n + 255) / 256; return g < 1 ? 1 : (g > 1024 ? 1024 : g); }

void launch_rig_init(const RigArgs& a, double lambda0, hipStream_t s)
{
    const int most = a.N > 4 * a.C ? a.N : 4 * a.C;
    hipLaunchKernelGGL(rig_init_kernel, dim3(grid_for(3 * most)), dim3(256), 0, s, a, lambda0);
}

void launch_rig_linearize(const RigArgs& a, hipStream_t s)
{
    if (a.loss == LOSS_CAUCHY) hipLaunchKernelGGL(rig_linearize_kernel<LOSS_CAUCHY>, dim3(a.n_lin_blocks), dim3(PT_THREADS), 0, s, a);
    else hipLaunchKernelGGL(rig_linearize_kernel<LOSS_NONE>, dim3(a.n_lin_blocks), dim3(PT_THREADS), 0, s, a);
    hipLaunchKernelGGL(rig_schur_kernel, dim3(a.n_pairs, a.n_chunks), dim3(256), 0, s, a);
    hipLaunchKernelGGL(rig_reduce_kernel, dim3(a.n_pairs), dim3(64), 0, s, a);
}

void launch_rig_iteration(const RigArgs& a, int it, int max_iters, double ftol, hipStream_t s)
{
    launch_rig_linearize(a, s);
    hipLaunchKernelGGL(rig_solve_kernel, dim3(1), dim3(256), 0, s, a, it);
    if (a.loss == LOSS_CAUCHY) hipLaunchKernelGGL(rig_update_kernel<LOSS_CAUCHY>, dim3(a.n_lin_blocks), dim3(PT_THREADS), 0, s, a);
    else hipLaunchKernelGGL(rig_update_kernel<LOSS_NONE>, dim3(a.n_lin_blocks), dim3(PT_THREADS), 0, s, a);
    hipLaunchKernelGGL(rig_decide_kernel, dim3(1), dim3(64), 0, s, a, it, max_iters, ftol);
}

void launch_rig_finish(const RigArgs& a, hipStream_t s)
{
    hipLaunchKernelGGL(rig_finish_kernel, dim3(grid_for(3 * a.N)), dim3(256), 0, s, a);
}

void launch_rig_residuals(const RigArgs& a, hipStream_t s)
{
    if (a.loss == LOSS_CAUCHY) hipLaunchKernelGGL(rig_residuals_kernel<LOSS_CAUCHY>, dim3(a.n_lin_blocks), dim3(PT_THREADS), 0, s, a);
    else hipLaunchKernelGGL(rig_residuals_kernel<LOSS_NONE>, dim3(a.n_lin_blocks), dim3(PT_THREADS), 0, s, a);
}

int rig_lin_blocks(int N) { return (N + PT_THREADS - 1) / PT_THREADS; }
int rig_schur_chunks(int N) { return (N + SCHUR_CHUNK - 1) / SCHUR_CHUNK; }

} // namespace mocap
