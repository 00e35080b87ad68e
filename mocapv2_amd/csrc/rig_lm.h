// rig_lm.h -- the phases of the two rig bundle adjustments (rig_ba.hip, rig_selfcal.hip), each written once as a template over
// the camera block B of the solver.  Both minimise the same sum over exactly the observations that exist, by sparse
// Levenberg-Marquardt with a Schur complement on the points (FP64); what a solver's block is made of is all that differs.
//
// Observations are point-major (obs_offset [N + 1], obs_cam, obs_uv), a point's cameras in ascending order; rig_init_kernel
// checks that and turns each point's camera list into a 32-bit visibility mask, which is all the later kernels index with.
// The camera model with its derivatives, the step-control rule, the inverse of a point's 3x3 and the packed Cholesky of the
// reduced matrix are lm.h's.
// The library is built with -ffp-contract=off: every product and sum below is rounded on its own, and the restatements
// (tests/rig_ba_ref.py, tests/rig_selfcal_ref.py) form every per-observation quantity by the same operations in the same
// order.  What differs is the order of the sums over observations and points, which is fixed here: no floating-point atomics
// anywhere, a lane sums its own points in order, lanes join by a fixed shuffle tree, waves and workgroups in ascending order.
// Two runs give the same bits.
//
// One iteration is six stream-ordered launches; each returns at once when the state record says stop, so the host enqueues
// max_iters iterations and never waits between them:
//   rig_linearize_kernel  a lane owns a point: residuals, analytic Jacobian, V_n, g_n and the cost in registers, the W blocks
//                         to scratch; camera blocks U_c, g_c summed per workgroup (shuffle tree, waves through LDS), each sum
//                         through the tree as soon as it is formed, so that none of them stays in a register
//   the Schur kernel      the solver's own (B::launch_schur): per camera pair a <= b and chunk of points, the P x P block
//                         W_a V*^-1 W_b^T and, on the diagonal, W_a V*^-1 g_n, as partials [chunk][pair][BLK]
//   rig_reduce_kernel     one workgroup per camera pair: the partials in ascending order into S = U* - sum, the reduced
//                         right-hand side, the camera gradient; a fixed column's diagonal; the cost
//   rig_solve_kernel      one workgroup: Cholesky of S (packed lower triangle: in LDS up to CHOL_LDS_ROWS rows, else in global
//                         memory), the camera step, the trial cameras
//   rig_update_kernel     a lane owns a point: back-substitution, trial point, trial cost, predicted reduction
//   rig_decide_kernel     one workgroup: lm_decide (gain ratio, accept / reject, Nielsen's damping update, the stops, history)
// The point-owning kernels take the loss (lm.h) as a template parameter.  With LOSS_CAUCHY an observation's residual and
// Jacobian rows are scaled by sqrt(w), w = 1 / (1 + s / c^2), before anything is formed from them, and the costs sum rho(s) in
// place of s (first-order IRLS); everything downstream reads the scaled blocks and does not know.  LOSS_NONE compiles to the
// code without a loss.  Before the loop rig_init_kernel copies the state and builds the masks; after it rig_finish_kernel
// hands the state back and rig_residuals_kernel (a lane owns a point) writes every observation's |r| and weight there.
//
// A block type B states what its solver's camera block is (all members static):
//   P, FIRST                       the block's width, and the first camera that has one (cameras below FIRST are fixed)
//   Lenses, lenses(a, buf), lenses_io(a), lens(l, c)
//                                  where the cameras' lenses live: of state buffer buf, of the state handed back; camera c's
//   columns(a, c, lens, o, q, jc)  the 2 x P camera columns of an observation, from what project<true> left in o
//   init_lenses(a, gid, stride), count(a, mask), launch_check(a, s)
//                                  the block's own work at init: its part of the state, a valid point's cameras, what follows
//   fixed(a, c, i)                 whether column i of camera c is held: the reduce kernel writes 1 on its diagonal of S
//   step_lenses(a, cur, c, d)      camera c's trial lens from its step d [P]
//   return_lenses(a, cur, gid, stride)   the block's part of what rig_finish_kernel hands back
//   launch_schur(a, s), schur_chunk(N)   its Schur kernel, and the points of one of that kernel's chunks
// The pose columns are a block's last six.  Everything else follows from P and FIRST.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "kernels.h"
#include "lm.h"

namespace mocap {

constexpr int CHOL_LDS_ROWS = 90;   // 90 * 91 / 2 doubles = 32 760 bytes: the rows of S that factorise in LDS (6 wide: C <= 16, 15 wide: C <= 6)

template <class B> struct RigDims {
    static constexpr int P = B::P;
    static constexpr int TRI = P * (P + 1) / 2;            // the upper triangle of U_c
    static constexpr int U = TRI + P;                      // a camera's sums of the point kernel: that triangle, then g_c (27 / 135)
    static constexpr int BLK = P * P + P;                  // a pair's sums of the Schur kernel: W_a V*^-1 W_b^T, then W_a V*^-1 g_n (42 / 240)
    static constexpr int MAX_D = P * (32 - B::FIRST);      // rows of the largest reduced system (186 / 480)
    static constexpr int REDUCE_THREADS = (BLK + 63) / 64 * 64; // BLK in whole waves (64 / 256)
};

struct Cam { double R[9], t[3]; Lens lens; };

template <class B>
__device__ __forceinline__ Cam load_cam(typename B::Lenses lenses, const double* pose, int c)
{
    Cam m;
#pragma unroll
    for (int k = 0; k < 9; k++) m.R[k] = pose[12 * c + k];
#pragma unroll
    for (int k = 0; k < 3; k++) m.t[k] = pose[12 * c + 9 + k];
    m.lens = B::lens(lenses, c);
    return m;
}

// One observation of camera c: residual r, and with JAC the 2 x P camera Jacobian jc (B::columns; the pose's are those of the
// local perturbation R <- Exp(w) R, t <- t + dt: w, dt) and the 2x3 point Jacobian jp = A R.  Returns false when the point is
// not in front of the camera (z <= 0 or NaN).
template <class B, bool JAC>
__device__ __forceinline__ bool observe(const RigArgs& a, int c, const Cam& m, const double X[3], double ou, double ov, double r[2],
                                        double jc[2][B::P], double jp[2][3])
{
    const double q[3] = {(m.R[0] * X[0] + m.R[1] * X[1]) + m.R[2] * X[2], (m.R[3] * X[0] + m.R[4] * X[1]) + m.R[5] * X[2],
                         (m.R[6] * X[0] + m.R[7] * X[1]) + m.R[8] * X[2]};
    Projected o;
    const bool front = project<JAC>(m.lens, q, m.t, ou, ov, r, o);
    if (JAC) {
#pragma unroll
        for (int i = 0; i < 2; i++)
#pragma unroll
            for (int j = 0; j < 3; j++) jp[i][j] = (o.A[i][0] * m.R[j] + o.A[i][1] * m.R[3 + j]) + o.A[i][2] * m.R[6 + j];
        B::columns(a, c, m.lens, o, q, jc);
    }
    return front;
}

// The loss's part of an observation: its share of the cost from the unscaled r, and with JAC r, jc, jp scaled by sqrt(weight)
template <int P, int LOSS, bool JAC>
__device__ __forceinline__ double robustify(double c2, double r[2], double jc[2][P], double jp[2][3])
{
    const double s = r[0] * r[0] + r[1] * r[1];
    if (LOSS == LOSS_NONE) return s;
    if (JAC) {
        const double sw = sqrt(cauchy_weight(s, c2));
#pragma unroll
        for (int i = 0; i < 2; i++) {
            r[i] *= sw;
#pragma unroll
            for (int j = 0; j < P; j++) jc[i][j] *= sw;
#pragma unroll
            for (int j = 0; j < 3; j++) jp[i][j] *= sw;
        }
    }
    return cauchy_rho(s, c2);
}

// the pair of cameras of a workgroup of the Schur and the reduce kernel: pair index -> (ca, cb), FIRST <= ca <= cb < C, row by row
template <class B>
__device__ __forceinline__ void pair_cameras(int pair, int C, int& ca, int& cb)
{
    tri_unrank(pair, C - B::FIRST, ca, cb);
    ca += B::FIRST; cb += B::FIRST;
}

__device__ __forceinline__ bool gated(const RigState* st) { return st->stop || st->layout_err; }

// Copies the caller's state into buffer 0, builds the visibility masks and checks the layout (a violation is reported as
// MOCAP_RIG_E_LAYOUT; nothing later reads the observation arrays through an unchecked index).  The state record was zeroed.
template <class B>
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
    B::init_lenses(a, gid, stride);
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
        B::count(a, ok ? mask : 0u);
    }
}

// A lane owns a point.  Grid: ceil(N / PT_THREADS).
template <class B, int LOSS>
__global__ __launch_bounds__(PT_THREADS) void rig_linearize_kernel(RigArgs a)
{
    constexpr int P = B::P, TRI = RigDims<B>::TRI, U = RigDims<B>::U;
    __shared__ double s_red[2][4][U];
    __shared__ double s_part[4];
    RigState* st = a.state;
    if (gated(st)) return;
    const int tid = threadIdx.x, n = blockIdx.x * PT_THREADS + tid, lane = tid & 63, wave = tid >> 6;
    const bool live = n < a.N;
    const typename B::Lenses lenses = B::lenses(a, st->cur);
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
        double r[2] = {0, 0}, jc[2][P], jp[2][3];
#pragma unroll
        for (int i = 0; i < 2; i++) {
#pragma unroll
            for (int j = 0; j < P; j++) jc[i][j] = 0;
#pragma unroll
            for (int j = 0; j < 3; j++) jp[i][j] = 0;
        }
        if (has) {
            const Cam m = load_cam<B>(lenses, pose, c);
            behind = !observe<B, true>(a, c, m, X, a.obs_uv[2 * (size_t)o], a.obs_uv[2 * (size_t)o + 1], r, jc, jp) || behind;
            cost += robustify<P, LOSS, true>(a.loss_c2, r, jc, jp);
            int k = 0;
#pragma unroll
            for (int i = 0; i < 3; i++) {
                gp[i] += jp[0][i] * r[0] + jp[1][i] * r[1];
#pragma unroll
                for (int j = i; j < 3; j++) V[k++] += jp[0][i] * jp[0][j] + jp[1][i] * jp[1][j];
            }
            if (c >= B::FIRST) {
                double* W = a.W + 3 * P * (size_t)o;
#pragma unroll
                for (int i = 0; i < P; i++)
#pragma unroll
                    for (int j = 0; j < 3; j++) W[3 * i + j] = jc[0][i] * jp[0][j] + jc[1][i] * jp[1][j];
            }
            o++;
        }
        if (c < B::FIRST) continue; // a fixed camera
        // U_c (TRI sums) and g_c (P) of this workgroup's points; a lane without the camera adds zeros
        double* red = s_red[c & 1][wave];
        {
            int k = 0;
#pragma unroll
            for (int i = 0; i < P; i++)
#pragma unroll
                for (int j = i; j < P; j++) {
                    const double v = wave_sum(jc[0][i] * jc[0][j] + jc[1][i] * jc[1][j]);
                    if (lane == 0) red[k] = v;
                    k++;
                }
#pragma unroll
            for (int i = 0; i < P; i++) {
                const double v = wave_sum(jc[0][i] * r[0] + jc[1][i] * r[1]);
                if (lane == 0) red[TRI + i] = v;
            }
        }
        __syncthreads(); // (the buffer of camera c - 1 is free again after this barrier: two buffers, one barrier per camera)
        if (tid < U)
            a.lin_part[((size_t)blockIdx.x * (a.C - B::FIRST) + (c - B::FIRST)) * U + tid] =
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

// One workgroup (BLK threads in whole waves) per pair of cameras: every partial in ascending order.
template <class B>
__global__ __launch_bounds__(RigDims<B>::REDUCE_THREADS) void rig_reduce_kernel(RigArgs a)
{
    constexpr int P = B::P, TRI = RigDims<B>::TRI, U = RigDims<B>::U, BLK = RigDims<B>::BLK;
    __shared__ double s_u[U];
    __shared__ double s_blk[P * P];
    if (gated(a.state)) return;
    const int tid = threadIdx.x, pair = blockIdx.x, D = P * (a.C - B::FIRST);
    int ca, cb;
    pair_cameras<B>(pair, a.C, ca, cb);
    const bool diag = ca == cb;
    const double lambda = a.state->lambda;
    if (diag && tid < U) {
        double s = 0;
        for (int b = 0; b < a.n_lin_blocks; b++) s += a.lin_part[((size_t)b * (a.C - B::FIRST) + (ca - B::FIRST)) * U + tid];
        s_u[tid] = s;
    }
    double sum = 0;
    if (tid < BLK)
        for (int ch = 0; ch < a.n_chunks; ch++) sum += a.schur_part[((size_t)ch * a.n_pairs + pair) * BLK + tid];
    __syncthreads();
    if (tid < P * P) {
        const int i = tid / P, j = tid % P;
        double u = 0;
        if (diag) {
            u = s_u[i <= j ? tri(i, j, P) : tri(j, i, P)];
            if (i == j) u = u + lambda * u;
        }
        s_blk[tid] = u - sum;
    }
    __syncthreads();
    if (tid < P * P) {
        const int i = tid / P, j = tid % P, ra = P * (ca - B::FIRST), rb = P * (cb - B::FIRST);
        if (diag) {
            const bool fixed = i == j && B::fixed(a, ca, i);
            a.S[(size_t)(ra + i) * D + ra + j] = fixed ? 1.0 : s_blk[i <= j ? tid : P * j + i]; // the upper triangle, mirrored
        } else { a.S[(size_t)(ra + i) * D + rb + j] = s_blk[tid]; a.S[(size_t)(rb + j) * D + ra + i] = s_blk[tid]; }
    } else if (tid < BLK && diag) {
        const int i = tid - P * P, row = P * (ca - B::FIRST) + i;
        a.rhs[row] = sum - s_u[TRI + i];
        a.gc[row] = s_u[TRI + i];
        a.udiag[row] = s_u[tri(i, i, P)];
    }
    if (pair == 0 && tid == RigDims<B>::REDUCE_THREADS - 1) {
        double s = 0;
        for (int b = 0; b < a.n_lin_blocks; b++) s += a.cost_part[b];
        a.scalars[RIG_LIN_COST] = 0.5 * s;
    }
}

// One workgroup.  Also the keeper of the state record's first cost, and of the two failures a linearisation can show.
template <class B>
__global__ __launch_bounds__(256) void rig_solve_kernel(RigArgs a, int it)
{
    constexpr int P = B::P;
    __shared__ double s_L[CHOL_LDS_ROWS * (CHOL_LDS_ROWS + 1) / 2];
    __shared__ double s_x[RigDims<B>::MAX_D];
    RigState* st = a.state;
    if (gated(st)) return;
    const int tid = threadIdx.x, D = P * (a.C - B::FIRST);
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
    // trial cameras into the other buffer
    const double* pose = a.poses + (size_t)st->cur * 12 * a.C;
    double* trial = a.poses + (size_t)(1 - st->cur) * 12 * a.C;
    if (tid < a.C) {
        if (tid >= B::FIRST) B::step_lenses(a, st->cur, tid, s_x + P * (tid - B::FIRST));
        if (tid == 0) {
            for (int k = 0; k < 12; k++) trial[k] = pose[k];
        } else {
            const double* d = s_x + P * (tid - B::FIRST) + (P - 6);
            double R[9], Rn[9];
            for (int k = 0; k < 9; k++) R[k] = pose[12 * tid + k];
            rotate_left(d, R, Rn);
            for (int k = 0; k < 9; k++) trial[12 * tid + k] = Rn[k];
            for (int k = 0; k < 3; k++) trial[12 * tid + 9 + k] = pose[12 * tid + 9 + k] + d[3 + k];
        }
    }
}

// A lane owns a point: dX = -V*^-1 (g_n + sum_c W_nc^T d_c), the trial point, its observations under the trial cameras.
template <class B, int LOSS>
__global__ __launch_bounds__(PT_THREADS) void rig_update_kernel(RigArgs a)
{
    constexpr int P = B::P;
    __shared__ double s_d[RigDims<B>::MAX_D];
    __shared__ double s_part[4];
    RigState* st = a.state;
    if (gated(st) || st->chol_fail) return;
    const int tid = threadIdx.x, n = blockIdx.x * PT_THREADS + tid, D = P * (a.C - B::FIRST);
    for (int i = tid; i < D; i += PT_THREADS) s_d[i] = a.delta_c[i];
    __syncthreads();
    const double* pts = a.points + (size_t)st->cur * 3 * a.N;
    double* trial_pts = a.points + (size_t)(1 - st->cur) * 3 * a.N;
    const typename B::Lenses trial_lenses = B::lenses(a, 1 - st->cur);
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
            if (c < B::FIRST) continue;
            const double* W = a.W + 3 * P * (size_t)o;
            const double* d = s_d + P * (c - B::FIRST);
#pragma unroll
            for (int j = 0; j < 3; j++) {
                double w = W[j] * d[0]; // W^T d, left-associated from its first term
#pragma unroll
                for (int i = 1; i < P; i++) w = w + W[3 * i + j] * d[i];
                q[j] += w;
            }
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
            const Cam cam = load_cam<B>(trial_lenses, trial_pose, c);
            double r[2];
            behind = !observe<B, false>(a, c, cam, X, a.obs_uv[2 * (size_t)o], a.obs_uv[2 * (size_t)o + 1], r, nullptr, nullptr) || behind;
            cost += robustify<P, LOSS, false>(a.loss_c2, r, nullptr, nullptr);
        }
    }
    if (behind) atomicOr(&st->trial_behind, 1);
    const double c_sum = block_sum(cost, s_part), p_sum = block_sum(pred, s_part), n_sum = block_sum(n2, s_part);
    if (tid == 0) {
        a.upd_part[3 * (size_t)blockIdx.x] = c_sum; a.upd_part[3 * (size_t)blockIdx.x + 1] = p_sum; a.upd_part[3 * (size_t)blockIdx.x + 2] = n_sum;
    }
}

// One thread decides by lm_decide over the partials of the point kernel's workgroups.  history[it] is its row.  It does not
// depend on the block: one plain kernel, which every file that launches it compiles for itself (hence static).
static __global__ __launch_bounds__(64) void rig_decide_kernel(RigArgs a, int it, int max_iters, double ftol)
{
    RigState* st = a.state;
    if (gated(st) || threadIdx.x != 0) return;
    lm_decide(st, a.upd_part, a.n_lin_blocks, a.scalars + RIG_PRED_CAM, it, max_iters, ftol, a.history + 4 * (size_t)it);
}

// The gauge on return (every t and every X scaled so that |t_1| is what it was at the start), the caller's arrays, the record.
template <class B>
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
    B::return_lenses(a, st->cur, gid, stride);
    for (int i = gid; i < 12 * a.C; i += stride) a.poses_io[i] = i % 12 < 9 ? pose[i] : pose[i] * s;
    for (int i = gid; i < 3 * a.N; i += stride) a.points_io[i] = pts[i] * s;
}

// A lane owns a point: the length of every observation's unweighted residual and the loss's weight, at the state
// rig_finish_kernel handed back (the caller's arrays; a negative status: nothing is written, the outputs were zeroed).
template <class B, int LOSS>
__global__ __launch_bounds__(PT_THREADS) void rig_residuals_kernel(RigArgs a)
{
    const RigState* st = a.state;
    if (st->layout_err || st->status < 0) return;
    const int n = blockIdx.x * PT_THREADS + threadIdx.x;
    if (n >= a.N) return;
    const double X[3] = {a.points_io[3 * (size_t)n], a.points_io[3 * (size_t)n + 1], a.points_io[3 * (size_t)n + 2]};
    int o = a.obs_offset[n];
    for (uint32_t m = a.mask[n]; m; m &= m - 1, o++) {
        const int c = __ffs(m) - 1;
        const Cam cam = load_cam<B>(B::lenses_io(a), a.poses_io, c);
        double r[2];
        observe<B, false>(a, c, cam, X, a.obs_uv[2 * (size_t)o], a.obs_uv[2 * (size_t)o + 1], r, nullptr, nullptr);
        const double s = r[0] * r[0] + r[1] * r[1];
        if (a.obs_err) a.obs_err[o] = sqrt(s);
        if (a.obs_weight) a.obs_weight[o] = LOSS == LOSS_NONE ? 1.0 : cauchy_weight(s, a.loss_c2);
    }
}

inline int grid_for(int n) { int g = (n + 255) / 256; return g < 1 ? 1 : (g > 1024 ? 1024 : g); }

// a point-owning kernel in the instantiation of the problem's loss
inline void launch_points(void (*none)(RigArgs), void (*cauchy)(RigArgs), const RigArgs& a, hipStream_t s)
{
    void (*kernel)(RigArgs) = a.loss == LOSS_CAUCHY ? cauchy : none;
    hipLaunchKernelGGL(kernel, dim3(a.n_lin_blocks), dim3(PT_THREADS), 0, s, a);
}

template <class B> void launch_init(const RigArgs& a, double lambda0, hipStream_t s)
{
    const int most = a.N > 4 * a.C ? a.N : 4 * a.C;
    hipLaunchKernelGGL(rig_init_kernel<B>, dim3(grid_for(3 * most)), dim3(256), 0, s, a, lambda0);
    B::launch_check(a, s);
}

template <class B> void launch_linearize(const RigArgs& a, hipStream_t s)
{
    launch_points(rig_linearize_kernel<B, LOSS_NONE>, rig_linearize_kernel<B, LOSS_CAUCHY>, a, s);
    B::launch_schur(a, s);
    hipLaunchKernelGGL(rig_reduce_kernel<B>, dim3(a.n_pairs), dim3(RigDims<B>::REDUCE_THREADS), 0, s, a);
}

template <class B> void launch_iteration(const RigArgs& a, int it, int max_iters, double ftol, hipStream_t s)
{
    launch_linearize<B>(a, s);
    hipLaunchKernelGGL(rig_solve_kernel<B>, dim3(1), dim3(256), 0, s, a, it);
    launch_points(rig_update_kernel<B, LOSS_NONE>, rig_update_kernel<B, LOSS_CAUCHY>, a, s);
    hipLaunchKernelGGL(rig_decide_kernel, dim3(1), dim3(64), 0, s, a, it, max_iters, ftol);
}

template <class B> void launch_finish(const RigArgs& a, hipStream_t s)
{
    hipLaunchKernelGGL(rig_finish_kernel<B>, dim3(grid_for(3 * a.N)), dim3(256), 0, s, a);
}

template <class B> void launch_residuals(const RigArgs& a, hipStream_t s)
{
    launch_points(rig_residuals_kernel<B, LOSS_NONE>, rig_residuals_kernel<B, LOSS_CAUCHY>, a, s);
}

// the record a solver's file exports for the host (kernels.h)
template <class B> constexpr RigSolver rig_solver()
{
    return RigSolver{B::P, B::FIRST, B::schur_chunk, launch_init<B>, launch_linearize<B>, launch_iteration<B>, launch_finish<B>, launch_residuals<B>};
}

} // namespace mocap
