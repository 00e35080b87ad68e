// rig_selfcal.hip -- bundle adjustment of a whole rig that also refines every camera's lens, on the device (FP64): per camera
// fx, fy, cx, cy, k1, k2, p1, p2, k3 (camera 0 included), the poses of cameras 1..C-1 and every 3-D point, over exactly the
// observations that exist, by sparse Levenberg-Marquardt with a Schur complement on the points.
//
// The reference has no counterpart (its intrinsics come from board views alone, CalculateCameraIntrinsic.py:58, and its bundle
// adjustment, lib/Helpers.py:158-176, moves one pose): the contract is the definition of DESIGN.md section 2, restated in NumPy
// by tests/rig_selfcal_ref.py.  The problem, the observation layout, the loss and the phases are rig_ba.hip's; what changes is
// the camera block, 15 wide -- the 9 lens columns of lm.h's lens_columns, then the 6 of pose_columns -- for every camera, so
// the reduced system is 15 C square.  A caller's mask frees lens parameters per camera; a fixed column (a masked lens
// parameter, camera 0's pose) is set to zero in the observation's Jacobian, which zeroes its rows of U, W and g, and the
// reduce kernel writes 1 on its diagonal of S: its step is exactly 0, every block keeps one shape and nothing is compacted.
// The library is built with -ffp-contract=off, and the restatement forms every per-observation quantity by the same
// operations in the same order.  No floating-point atomics: a lane sums its own points in order, lanes join by a fixed
// shuffle tree, a thread of the Schur kernel adds its chunk's points in ascending order, workgroups' partials are added in
// ascending order.  Two runs give the same bits.
//
// One iteration is six stream-ordered launches; each returns at once when the state record says stop:
//   selfcal_linearize_kernel  a lane owns a point: residuals, the 2 x 15 and 2 x 3 Jacobians, V_n, g_n and the cost in
//                             registers, the W blocks (15 x 3) to scratch; U_c (120 sums) and g_c (15) per workgroup, each
//                             sum through the shuffle tree as soon as it is formed, so that none of them stays in a register
//   selfcal_schur_kernel      grid (chunk of points, camera pair a <= b): a THREAD owns one of the 225 entries of W_a V*^-1
//                             W_b^T or, on the diagonal, one of the 15 of W_a V*^-1 g_n, and adds the chunk's points in order
//                             (a lane that owned a point would hold 240 sums: 480 registers)
//   selfcal_reduce_kernel     one workgroup per camera pair: the partials in ascending order into S, the reduced right-hand
//                             side, the camera gradient; the fixed columns' diagonal; the cost
//   selfcal_solve_kernel      one workgroup: Cholesky of S (packed lower triangle: in LDS up to 90 rows, C <= 6, else in
//                             global memory), the camera step, the trial intrinsics and poses
//   selfcal_update_kernel     a lane owns a point: back-substitution, trial point, trial cost, predicted reduction
//   selfcal_decide_kernel     lm_decide
// Before the loop selfcal_init_kernel copies the state, builds the visibility masks, checks the layout and counts every
// camera's observations, and selfcal_check_kernel refuses a camera whose mask frees more than half as many lens parameters as
// it has observations.  After it selfcal_finish_kernel hands the state back and selfcal_residuals_kernel writes every
// observation's |r| and weight there.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "kernels.h"
#include "lm.h"

namespace mocap {

namespace {

constexpr int P = SELFCAL_P;
constexpr int PT_THREADS = 256;     // points per workgroup of the point-owning kernels (linearize, update)
constexpr int SCHUR_CHUNK = 256;    // points per workgroup of selfcal_schur_kernel at least (a thread walks them all), and chunks at most
constexpr int CHOL_LDS_ROWS = 90;   // 90 * 91 / 2 doubles = 32 760 bytes: C <= 6 factorises in LDS
constexpr int MAX_D = P * 32;

struct Cam { double R[9], t[3]; Lens lens; };

__device__ __forceinline__ Cam load_cam(const double* kd, const double* pose, int c)
{
    Cam m;
#pragma unroll
    for (int k = 0; k < 9; k++) m.R[k] = pose[12 * c + k];
#pragma unroll
    for (int k = 0; k < 3; k++) m.t[k] = pose[12 * c + 9 + k];
    const double* k = kd + 9 * c;
    m.lens = Lens{k[0], k[1], k[2], k[3], k[4], k[5], k[6], k[7], k[8]};
    return m;
}

// One observation: residual r, and with JAC the 2x15 camera Jacobian jc (lens columns, then the local pose perturbation's;
// the columns whose bit of `free` is clear set to zero) and the 2x3 point Jacobian jp = A R.  Returns false when the point is
// not in front of the camera (z <= 0 or NaN).
template <bool JAC>
__device__ __forceinline__ bool observe(const Cam& m, int free, const double X[3], double ou, double ov, double r[2], double jc[2][P], double jp[2][3])
{
    const double q[3] = {(m.R[0] * X[0] + m.R[1] * X[1]) + m.R[2] * X[2], (m.R[3] * X[0] + m.R[4] * X[1]) + m.R[5] * X[2],
                         (m.R[6] * X[0] + m.R[7] * X[1]) + m.R[8] * X[2]};
    Projected o;
    const bool front = project<JAC>(m.lens, q, m.t, ou, ov, r, o);
    if (JAC) {
        lens_columns(m.lens, o, jc[0], jc[1]);
#pragma unroll
        for (int i = 0; i < 2; i++) {
#pragma unroll
            for (int j = 0; j < 3; j++) jp[i][j] = (o.A[i][0] * m.R[j] + o.A[i][1] * m.R[3 + j]) + o.A[i][2] * m.R[6 + j];
            pose_columns(o.A[i], q, jc[i] + 9);
#pragma unroll
            for (int j = 0; j < P; j++) jc[i][j] = ((free >> j) & 1) ? jc[i][j] : 0.0;
        }
    }
    return front;
}

// The loss's part of an observation: its share of the cost from the unscaled r, and with JAC r, jc, jp scaled by sqrt(weight)
template <int LOSS, bool JAC>
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

__device__ __forceinline__ bool gated(const RigState* st) { return st->stop || st->layout_err; }

} // namespace

// Copies the caller's state into buffer 0, builds the visibility masks, checks the layout and counts every camera's
// observations (integer atomics).  The state record and the counts were zeroed.
__global__ __launch_bounds__(256) void selfcal_init_kernel(SelfcalArgs a, double lambda0)
{
    const int gid = blockIdx.x * 256 + threadIdx.x, stride = gridDim.x * 256;
    RigState* st = a.state;
    if (gid == 0) {
        st->lambda = lambda0; st->nu = 2.0;
        const double* t1 = a.poses_io + 12 + 9;
        st->t1_norm = sqrt((t1[0] * t1[0] + t1[1] * t1[1]) + t1[2] * t1[2]);
        if (a.obs_offset[0] != 0 || a.obs_offset[a.N] != a.n_obs) atomicOr(&st->layout_err, 1);
    }
    for (int i = gid; i < 9 * a.C; i += stride) a.kd[i] = a.kd_io[i];
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
        for (uint32_t m = ok ? mask : 0u; m; m &= m - 1) atomicAdd(&a.cam_count[__ffs(m) - 1], 1);
    }
}

// One workgroup: a camera whose mask is not 0 needs at least twice as many observations as it has free lens parameters.
__global__ __launch_bounds__(64) void selfcal_check_kernel(SelfcalArgs a)
{
    const int c = threadIdx.x;
    if (c >= a.C) return;
    const int lens = a.free_cols[c] & 0x1ff;
    if (lens != 0 && a.cam_count[c] < 2 * __popc(lens)) atomicOr(&a.state->layout_err, 1);
}

// A lane owns a point.  Grid: ceil(N / 256).
template <int LOSS>
__global__ __launch_bounds__(PT_THREADS) void selfcal_linearize_kernel(SelfcalArgs a)
{
    __shared__ double s_red[2][4][SELFCAL_U];
    __shared__ double s_part[4];
    RigState* st = a.state;
    if (gated(st)) return;
    const int tid = threadIdx.x, n = blockIdx.x * PT_THREADS + tid, lane = tid & 63, wave = tid >> 6;
    const bool live = n < a.N;
    const double* kd = a.kd + (size_t)st->cur * 9 * a.C;
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
            const Cam m = load_cam(kd, pose, c);
            behind = !observe<true>(m, a.free_cols[c], X, a.obs_uv[2 * (size_t)o], a.obs_uv[2 * (size_t)o + 1], r, jc, jp) || behind;
            cost += robustify<LOSS, true>(a.loss_c2, r, jc, jp);
            int k = 0;
#pragma unroll
            for (int i = 0; i < 3; i++) {
                gp[i] += jp[0][i] * r[0] + jp[1][i] * r[1];
#pragma unroll
                for (int j = i; j < 3; j++) V[k++] += jp[0][i] * jp[0][j] + jp[1][i] * jp[1][j];
            }
            double* W = a.W + 3 * P * (size_t)o;
#pragma unroll
            for (int i = 0; i < P; i++)
#pragma unroll
                for (int j = 0; j < 3; j++) W[3 * i + j] = jc[0][i] * jp[0][j] + jc[1][i] * jp[1][j];
            o++;
        }
        // U_c (120 sums) and g_c (15) of this workgroup's points; a lane without the camera adds zeros
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
                if (lane == 0) red[120 + i] = v;
            }
        }
        __syncthreads(); // (the buffer of camera c - 1 is free again after this barrier: two buffers, one barrier per camera)
        if (tid < SELFCAL_U)
            a.lin_part[((size_t)blockIdx.x * a.C + c) * SELFCAL_U + tid] =
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

// Grid (chunk of a.schur_chunk points, pair of cameras a <= b).  Thread e < 225 owns entry (e / 15, e % 15) of W_a V*^-1 W_b^T,
// thread 225 + i entry i of W_a V*^-1 g_n (a == b only); each adds the chunk's points that both cameras see, in ascending order.
__global__ __launch_bounds__(256) void selfcal_schur_kernel(SelfcalArgs a)
{
    if (gated(a.state)) return;
    const int tid = threadIdx.x, pair = blockIdx.y, chunk = blockIdx.x;
    if (tid >= SELFCAL_BLK) return; // (no barrier below)
    int ca, cb;
    tri_unrank(pair, a.C, ca, cb);
    const bool diag = ca == cb, is_g = tid >= P * P;
    const int i = is_g ? tid - P * P : tid / P, j = is_g ? 0 : tid % P;
    const uint32_t both = (1u << ca) | (1u << cb);
    double acc = 0;
    const int n0 = chunk * a.schur_chunk, n1 = n0 + a.schur_chunk < a.N ? n0 + a.schur_chunk : a.N;
    if (!is_g || diag)
        for (int n = n0; n < n1; n++) { // uniform over the workgroup
            const uint32_t mask = a.mask[n];
            if ((mask & both) != both) continue;
            const int o0 = a.obs_offset[n];
            const double* Wa = a.W + 3 * P * (size_t)(o0 + __popc(mask & ((1u << ca) - 1u))) + 3 * i;
            const double* Wb = a.W + 3 * P * (size_t)(o0 + __popc(mask & ((1u << cb) - 1u))) + 3 * j;
            double inv[6];
#pragma unroll
            for (int k = 0; k < 6; k++) inv[k] = a.Vinv[6 * (size_t)n + k];
            const double w0 = Wa[0], w1 = Wa[1], w2 = Wa[2];
            double Y[3];
#pragma unroll
            for (int k = 0; k < 3; k++) Y[k] = (w0 * sym3(inv, 0, k) + w1 * sym3(inv, 1, k)) + w2 * sym3(inv, 2, k);
            if (is_g) acc += (Y[0] * a.gp[3 * (size_t)n] + Y[1] * a.gp[3 * (size_t)n + 1]) + Y[2] * a.gp[3 * (size_t)n + 2];
            else acc += (Y[0] * Wb[0] + Y[1] * Wb[1]) + Y[2] * Wb[2];
        }
    a.schur_part[((size_t)chunk * a.n_pairs + pair) * SELFCAL_BLK + tid] = acc;
}

// One workgroup (256 threads) per pair of cameras: every partial in ascending order.
__global__ __launch_bounds__(256) void selfcal_reduce_kernel(SelfcalArgs a)
{
    __shared__ double s_u[SELFCAL_U];
    __shared__ double s_blk[P * P];
    if (gated(a.state)) return;
    const int tid = threadIdx.x, pair = blockIdx.x, D = P * a.C;
    int ca, cb;
    tri_unrank(pair, a.C, ca, cb);
    const bool diag = ca == cb;
    const double lambda = a.state->lambda;
    if (diag && tid < SELFCAL_U) {
        double s = 0;
        for (int b = 0; b < a.n_lin_blocks; b++) s += a.lin_part[((size_t)b * a.C + ca) * SELFCAL_U + tid];
        s_u[tid] = s;
    }
    double sum = 0;
    if (tid < SELFCAL_BLK)
        for (int ch = 0; ch < a.n_chunks; ch++) sum += a.schur_part[((size_t)ch * a.n_pairs + pair) * SELFCAL_BLK + tid];
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
        const int i = tid / P, j = tid % P, ra = P * ca, rb = P * cb;
        if (diag) {
            const bool fixed = i == j && !((a.free_cols[ca] >> i) & 1);
            a.S[(size_t)(ra + i) * D + ra + j] = fixed ? 1.0 : s_blk[i <= j ? tid : P * j + i]; // the upper triangle, mirrored
        } else { a.S[(size_t)(ra + i) * D + rb + j] = s_blk[tid]; a.S[(size_t)(rb + j) * D + ra + i] = s_blk[tid]; }
    } else if (tid < SELFCAL_BLK && diag) {
        const int i = tid - P * P, row = P * ca + i;
        a.rhs[row] = sum - s_u[120 + i];
        a.gc[row] = s_u[120 + i];
        a.udiag[row] = s_u[tri(i, i, P)];
    }
    if (pair == 0 && tid == 255) {
        double s = 0;
        for (int b = 0; b < a.n_lin_blocks; b++) s += a.cost_part[b];
        a.scalars[RIG_LIN_COST] = 0.5 * s;
    }
}

// One workgroup.  Also the keeper of the state record's first cost, and of the two failures a linearisation can show.
__global__ __launch_bounds__(256) void selfcal_solve_kernel(SelfcalArgs a, int it)
{
    __shared__ double s_L[CHOL_LDS_ROWS * (CHOL_LDS_ROWS + 1) / 2];
    __shared__ double s_x[MAX_D];
    RigState* st = a.state;
    if (gated(st)) return;
    const int tid = threadIdx.x, D = P * a.C;
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
    // trial intrinsics and poses into the other buffer
    const double* kd = a.kd + (size_t)st->cur * 9 * a.C;
    double* trial_kd = a.kd + (size_t)(1 - st->cur) * 9 * a.C;
    const double* pose = a.poses + (size_t)st->cur * 12 * a.C;
    double* trial = a.poses + (size_t)(1 - st->cur) * 12 * a.C;
    if (tid < a.C) {
        const double* d = s_x + P * tid;
        for (int k = 0; k < 9; k++) trial_kd[9 * tid + k] = kd[9 * tid + k] + d[k];
        if (tid == 0) {
            for (int k = 0; k < 12; k++) trial[k] = pose[k];
        } else {
            double R[9], Rn[9];
            for (int k = 0; k < 9; k++) R[k] = pose[12 * tid + k];
            rotate_left(d + 9, R, Rn);
            for (int k = 0; k < 9; k++) trial[12 * tid + k] = Rn[k];
            for (int k = 0; k < 3; k++) trial[12 * tid + 9 + k] = pose[12 * tid + 9 + k] + d[12 + k];
        }
    }
}

// A lane owns a point: dX = -V*^-1 (g_n + sum_c W_nc^T d_c), the trial point, its observations under the trial cameras.
template <int LOSS>
__global__ __launch_bounds__(PT_THREADS) void selfcal_update_kernel(SelfcalArgs a)
{
    __shared__ double s_d[MAX_D];
    __shared__ double s_part[4];
    RigState* st = a.state;
    if (gated(st) || st->chol_fail) return;
    const int tid = threadIdx.x, n = blockIdx.x * PT_THREADS + tid, D = P * a.C;
    for (int i = tid; i < D; i += PT_THREADS) s_d[i] = a.delta_c[i];
    __syncthreads();
    const double* pts = a.points + (size_t)st->cur * 3 * a.N;
    double* trial_pts = a.points + (size_t)(1 - st->cur) * 3 * a.N;
    const double* trial_kd = a.kd + (size_t)(1 - st->cur) * 9 * a.C;
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
            const double* W = a.W + 3 * P * (size_t)o;
            const double* d = s_d + P * c;
#pragma unroll
            for (int j = 0; j < 3; j++) {
                double w = W[j] * d[0];
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
            const Cam cam = load_cam(trial_kd, trial_pose, __ffs(m) - 1);
            double r[2];
            behind = !observe<false>(cam, 0, X, a.obs_uv[2 * (size_t)o], a.obs_uv[2 * (size_t)o + 1], r, nullptr, nullptr) || behind;
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
__global__ __launch_bounds__(64) void selfcal_decide_kernel(SelfcalArgs a, int it, int max_iters, double ftol)
{
    RigState* st = a.state;
    if (gated(st) || threadIdx.x != 0) return;
    lm_decide(st, a.upd_part, a.n_lin_blocks, a.scalars + RIG_PRED_CAM, it, max_iters, ftol, a.history + 4 * (size_t)it);
}

// The gauge on return (every t and every X scaled so that |t_1| is what it was at the start), the caller's arrays, the record.
__global__ __launch_bounds__(256) void selfcal_finish_kernel(SelfcalArgs a)
{
    const int gid = blockIdx.x * 256 + threadIdx.x, stride = gridDim.x * 256;
    const RigState* st = a.state;
    if (gid == 0) {
        a.result[0] = st->layout_err ? (double)RIG_ERR_LAYOUT : (double)st->status;
        a.result[1] = (double)st->iters; a.result[2] = st->cost0; a.result[3] = st->cost;
    }
    if (st->layout_err || st->status < 0) return; // the caller's arrays stay as they were
    const double* kd = a.kd + (size_t)st->cur * 9 * a.C;
    const double* pose = a.poses + (size_t)st->cur * 12 * a.C;
    const double* pts = a.points + (size_t)st->cur * 3 * a.N;
    const double* t1 = pose + 12 + 9;
    const double now = sqrt((t1[0] * t1[0] + t1[1] * t1[1]) + t1[2] * t1[2]);
    double s = st->t1_norm / now;
    if (!(s > 0.0) || !finite(s)) s = 1.0; // |t_1| = 0 at either end: no scale to restore
    for (int i = gid; i < 9 * a.C; i += stride) a.kd_io[i] = kd[i];
    for (int i = gid; i < 12 * a.C; i += stride) a.poses_io[i] = i % 12 < 9 ? pose[i] : pose[i] * s;
    for (int i = gid; i < 3 * a.N; i += stride) a.points_io[i] = pts[i] * s;
}

// A lane owns a point: the length of every observation's unweighted residual and the loss's weight, at the state
// selfcal_finish_kernel handed back (the caller's arrays; a negative status: nothing is written, the outputs were zeroed).
template <int LOSS>
__global__ __launch_bounds__(PT_THREADS) void selfcal_residuals_kernel(SelfcalArgs a)
{
    const RigState* st = a.state;
    if (st->layout_err || st->status < 0) return;
    const int n = blockIdx.x * PT_THREADS + threadIdx.x;
    if (n >= a.N) return;
    const double X[3] = {a.points_io[3 * (size_t)n], a.points_io[3 * (size_t)n + 1], a.points_io[3 * (size_t)n + 2]};
    int o = a.obs_offset[n];
    for (uint32_t m = a.mask[n]; m; m &= m - 1, o++) {
        const Cam cam = load_cam(a.kd_io, a.poses_io, __ffs(m) - 1);
        double r[2];
        observe<false>(cam, 0, X, a.obs_uv[2 * (size_t)o], a.obs_uv[2 * (size_t)o + 1], r, nullptr, nullptr);
        const double s = r[0] * r[0] + r[1] * r[1];
        if (a.obs_err) a.obs_err[o] = sqrt(s);
        if (a.obs_weight) a.obs_weight[o] = LOSS == LOSS_NONE ? 1.0 : cauchy_weight(s, a.loss_c2);
    }
}

static int grid_for(int n) { int g = (n + 255) / 256; return g < 1 ? 1 : (g > 1024 ? 1024 : g); }

void launch_selfcal_init(const SelfcalArgs& a, double lambda0, hipStream_t s)
{
    const int most = a.N > 4 * a.C ? a.N : 4 * a.C;
    hipLaunchKernelGGL(selfcal_init_kernel, dim3(grid_for(3 * most)), dim3(256), 0, s, a, lambda0);
    hipLaunchKernelGGL(selfcal_check_kernel, dim3(1), dim3(64), 0, s, a);
}

void launch_selfcal_linearize(const SelfcalArgs& a, hipStream_t s)
{
    if (a.loss == LOSS_CAUCHY) hipLaunchKernelGGL(selfcal_linearize_kernel<LOSS_CAUCHY>, dim3(a.n_lin_blocks), dim3(PT_THREADS), 0, s, a);
    else hipLaunchKernelGGL(selfcal_linearize_kernel<LOSS_NONE>, dim3(a.n_lin_blocks), dim3(PT_THREADS), 0, s, a);
    hipLaunchKernelGGL(selfcal_schur_kernel, dim3(a.n_chunks, a.n_pairs), dim3(256), 0, s, a);
    hipLaunchKernelGGL(selfcal_reduce_kernel, dim3(a.n_pairs), dim3(256), 0, s, a);
}

void launch_selfcal_iteration(const SelfcalArgs& a, int it, int max_iters, double ftol, hipStream_t s)
{
    launch_selfcal_linearize(a, s);
    hipLaunchKernelGGL(selfcal_solve_kernel, dim3(1), dim3(256), 0, s, a, it);
    if (a.loss == LOSS_CAUCHY) hipLaunchKernelGGL(selfcal_update_kernel<LOSS_CAUCHY>, dim3(a.n_lin_blocks), dim3(PT_THREADS), 0, s, a);
    else hipLaunchKernelGGL(selfcal_update_kernel<LOSS_NONE>, dim3(a.n_lin_blocks), dim3(PT_THREADS), 0, s, a);
    hipLaunchKernelGGL(selfcal_decide_kernel, dim3(1), dim3(64), 0, s, a, it, max_iters, ftol);
}

void launch_selfcal_finish(const SelfcalArgs& a, hipStream_t s)
{
    hipLaunchKernelGGL(selfcal_finish_kernel, dim3(grid_for(3 * a.N)), dim3(256), 0, s, a);
}

void launch_selfcal_residuals(const SelfcalArgs& a, hipStream_t s)
{
    if (a.loss == LOSS_CAUCHY) hipLaunchKernelGGL(selfcal_residuals_kernel<LOSS_CAUCHY>, dim3(a.n_lin_blocks), dim3(PT_THREADS), 0, s, a);
    else hipLaunchKernelGGL(selfcal_residuals_kernel<LOSS_NONE>, dim3(a.n_lin_blocks), dim3(PT_THREADS), 0, s, a);
}

int selfcal_lin_blocks(int N) { return (N + PT_THREADS - 1) / PT_THREADS; }
// points per workgroup of the Schur kernel: SCHUR_CHUNK, or what leaves SCHUR_CHUNK chunks (the partials' memory stays bounded)
int selfcal_schur_chunk(int N) { const int c = (N + SCHUR_CHUNK - 1) / SCHUR_CHUNK; return c > SCHUR_CHUNK ? c : SCHUR_CHUNK; }

} // namespace mocap
