// fundamental.hip -- fundamental matrices from image points by batched RANSAC (FP64): every hypothesis of every camera
// pair of a calibration in one call.
//
// Replaces reference CalculateCameraPoses.py:189, cv.findFundamentalMat(p1, p2, cv.FM_RANSAC, 10, 0.99999), for a batch
// of camera pairs.  OpenCV's random sequence and its 7-point minimal solver are not reproduced: the contract is the
// definition of DESIGN.md section 2 (normalised 8-point solve per sample, symmetric epipolar distance, most inliers wins,
// lowest index on ties, 8-point refit over the winner's inliers), restated in NumPy by tests/fundamental_ref.py.  The
// device draws no random numbers: the sample table comes from the host.
// The library is built with -ffp-contract=off: every product and sum below is rounded on its own.
//
// Five kernels per call, all stream-ordered:
//   fund_hypotheses_kernel  one lane per hypothesis: gather 8 points, normalise, A^T A, smallest eigenvector (cyclic
//                           Jacobi on the 9x9: the matrix in registers, every index a constant, its eigenvector matrix in
//                           LDS, [element][lane]), rank 2, denormalise
//   fund_score_kernel       the hot path, H x N evaluations per pair: one lane holds one hypothesis, the workgroup walks
//                           a chunk of the pair's points staged in LDS; partial counts join by integer atomicAdd
//   fund_select_kernel      per pair: arg-max of the counts over the valid hypotheses, lowest index on ties
//   fund_mask_kernel        one lane per point: the inlier byte under the winner
//   fund_refit_kernel       per pair: normalisation and the 45 sums of A^T A over the inliers by a fixed reduction tree
//                           (no floating-point atomics: same bits on every run and in every batch), then the same solve
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "kernels.h"
#include "jacobi9.h"

namespace mocap {

namespace {

constexpr int HYP_LANES = 64;    // hypotheses per workgroup of fund_hypotheses_kernel (one wave)
constexpr int SCORE_THREADS = 256;
constexpr int SCORE_CHUNK = 1024;  // points staged per workgroup of fund_score_kernel (32 KB)
constexpr int REFIT_THREADS = 256;

__device__ __forceinline__ bool finite(double x) { return fabs(x) <= 1.7976931348623157e308; } // false for NaN

// [x'x, x'y, x', y'x, y'y, y', x, y, 1]: the row of x' F x = 0 for F row-major, (x, y) from list a, (x', y') from list b
__device__ __forceinline__ void epi_row(double x, double y, double xp, double yp, double r[9])
{
    r[0] = xp * x; r[1] = xp * y; r[2] = xp;
    r[3] = yp * x; r[4] = yp * y; r[5] = yp;
    r[6] = x; r[7] = y; r[8] = 1.0;
}
// the 45 unique sums of A^T A, upper triangle row by row.  Fully unrolled: every index is a constant, the sums stay in registers
__device__ __forceinline__ void acc45(double acc[45], const double r[9])
{
    int k = 0;
#pragma unroll
    for (int i = 0; i < 9; i++)
#pragma unroll
        for (int j = i; j < 9; j++) acc[k++] += r[i] * r[j];
}

// Hartley's similarity for a list with centroid (cx, cy) and mean distance d to it: s = sqrt(2) / d
struct Norm { double s, tx, ty; }; // x_n = s x + tx
__device__ __forceinline__ Norm make_norm(double cx, double cy, double d)
{
    Norm n;
    n.s = sqrt(2.0) / d;
    n.tx = -(n.s * cx); n.ty = -(n.s * cy);
    return n;
}

// eigenvector of the smallest eigenvalue of a symmetric 3x3 (cyclic Jacobi, registers only: every index a constant)
__device__ __forceinline__ void smallest_eigvec3(double B[3][3], double v[3])
{
    double V[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
    for (int sweep = 0; sweep < 60; sweep++) {
        double off = 0, diag = 0;
#pragma unroll
        for (int p = 0; p < 3; p++) {
            diag += B[p][p] * B[p][p];
#pragma unroll
            for (int q = p + 1; q < 3; q++) off += B[p][q] * B[p][q];
        }
        if (!(off > 1e-40 * diag)) break; // also ends on NaN
#pragma unroll
        for (int p = 0; p < 2; p++)
#pragma unroll
            for (int q = p + 1; q < 3; q++) {
                const double apq = B[p][q];
                if (apq == 0.0) continue;
                const double theta = (B[q][q] - B[p][p]) / (2.0 * apq);
                const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
#pragma unroll
                for (int k = 0; k < 3; k++) {
                    const double bkp = B[k][p], bkq = B[k][q];
                    B[k][p] = c * bkp - s * bkq; B[k][q] = s * bkp + c * bkq;
                }
#pragma unroll
                for (int k = 0; k < 3; k++) {
                    const double bpk = B[p][k], bqk = B[q][k];
                    B[p][k] = c * bpk - s * bqk; B[q][k] = s * bpk + c * bqk;
                }
#pragma unroll
                for (int k = 0; k < 3; k++) {
                    const double vkp = V[k][p], vkq = V[k][q];
                    V[k][p] = c * vkp - s * vkq; V[k][q] = s * vkp + c * vkq;
                }
            }
    }
    const int m = (B[1][1] < B[0][0]) ? (B[2][2] < B[1][1] ? 2 : 1) : (B[2][2] < B[0][0] ? 2 : 0);
#pragma unroll
    for (int k = 0; k < 3; k++) v[k] = m == 0 ? V[k][0] : (m == 1 ? V[k][1] : V[k][2]);
}

// Steps 3 to 5 of the definition from f, the 9-vector of step 2: rank 2, denormalisation, unit norm.  Writes the matrix to
// F[9]; returns false (and F = NaN) when an entry is not finite.
__device__ __forceinline__ bool finish_model(double f[3][3], const Norm na, const Norm nb, double F[9])
{
    // rank 2: F <- F - (F v) v^T, v = eigenvector of the smallest eigenvalue of F^T F
    double G[3][3], v[3], Fv[3];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) G[i][j] = (f[0][i] * f[0][j] + f[1][i] * f[1][j]) + f[2][i] * f[2][j];
    smallest_eigvec3(G, v);
#pragma unroll
    for (int i = 0; i < 3; i++) Fv[i] = (f[i][0] * v[0] + f[i][1] * v[1]) + f[i][2] * v[2];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) f[i][j] = f[i][j] - Fv[i] * v[j];
    // F <- T_b^T F T_a with T = [[s, 0, tx], [0, s, ty], [0, 0, 1]]
    double M[3][3]; // F T_a
#pragma unroll
    for (int i = 0; i < 3; i++) {
        M[i][0] = f[i][0] * na.s;
        M[i][1] = f[i][1] * na.s;
        M[i][2] = (f[i][0] * na.tx + f[i][1] * na.ty) + f[i][2];
    }
    double o[9];
#pragma unroll
    for (int j = 0; j < 3; j++) {
        o[j] = nb.s * M[0][j];
        o[3 + j] = nb.s * M[1][j];
        o[6 + j] = (nb.tx * M[0][j] + nb.ty * M[1][j]) + M[2][j];
    }
    double n2 = 0;
#pragma unroll
    for (int k = 0; k < 9; k++) n2 += o[k] * o[k];
    const double nrm = sqrt(n2);
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 9; k++) { o[k] = o[k] / nrm; ok = ok && finite(o[k]); }
#pragma unroll
    for (int k = 0; k < 9; k++) F[k] = ok ? o[k] : __builtin_nan("");
    return ok;
}

// Step 2's eigenvector and steps 3 to 5.  B: the 45 unique sums of A^T A of the normalised points (acc45's order = sym9's);
// overwritten.  V: 81 doubles of LDS, st apart (jacobi9.h: st = 64 with one hypothesis per lane, 1 for the refit's single solve).
__device__ __forceinline__ bool solve_from_normal_sums(double B[45], double* V, const int st, const Norm na, const Norm nb, double F[9])
{
    double h[9], f[3][3];
    smallest_eigvec9(B, V, st, h);
#pragma unroll
    for (int k = 0; k < 9; k++) f[k / 3][k % 3] = h[k];
    return finish_model(f, na, nb, F);
}

// Inlier test of the definition: e = max(d'^2, d^2) <= thr2 with d' the distance of (x', y') to the line F (x, y, 1) and d
// that of (x, y) to F^T (x', y', 1).  Each quotient n^2 / den <= thr2 is tested as n^2 <= thr2 * den with den > 0 (no FP64
// division in the hot loop); a NaN anywhere fails every comparison, so a NaN is not an inlier.  A finite point far enough out
// overflows both sides to +inf, where the quotient is inf / inf = NaN and `inf <= inf` would hold: n^2 must be finite (an
// infinite n^2 over any den is inf or NaN, never <= thr2; a finite n^2 over an overflowed den would be 0 <= thr2, which
// the comparison with +inf gives too -- reasoned, not tested: it takes a cancellation in n that no list reaches for a
// whole table).  The scoring kernel and the mask kernel both call this function: the mask's population count is the
// winner's count.
__device__ __forceinline__ bool is_inlier(const double F[9], double x, double y, double xp, double yp, double thr2)
{
    const double l0 = (F[0] * x + F[1] * y) + F[2], l1 = (F[3] * x + F[4] * y) + F[5], l2 = (F[6] * x + F[7] * y) + F[8];
    const double m0 = (F[0] * xp + F[3] * yp) + F[6], m1 = (F[1] * xp + F[4] * yp) + F[7], m2 = (F[2] * xp + F[5] * yp) + F[8];
    const double n1 = (xp * l0 + yp * l1) + l2, n2 = (x * m0 + y * m1) + m2;
    const double d1 = l0 * l0 + l1 * l1, d2 = m0 * m0 + m1 * m1;
    const double q1 = n1 * n1, q2 = n2 * n2;
    return (q1 <= thr2 * d1) && (q2 <= thr2 * d2) && d1 > 0.0 && d2 > 0.0 && finite(q1) && finite(q2);
}

} // namespace

// One lane per hypothesis, one wave per workgroup.
__global__ __launch_bounds__(HYP_LANES) void fund_hypotheses_kernel(FundArgs a)
{
    __shared__ double s_V[81 * HYP_LANES]; // the eigenvector matrices, [element][lane]: 41 KB, three workgroups per CU
    const int lane = threadIdx.x, pair = blockIdx.y, h = blockIdx.x * HYP_LANES + lane;
    if (h >= a.H) return; // no barrier in this kernel: the lanes are independent
    const int p0 = a.offset[pair], n = a.offset[pair + 1] - p0;
    const int32_t* smp = a.samples + ((size_t)pair * a.H + h) * 8;
    double* const Fout = a.F_all + ((size_t)pair * a.H + h) * 9;
    double ax[8], ay[8], bx[8], by[8];
    bool in_range = true;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const int idx = smp[i];
        const bool ok = idx >= 0 && idx < n;
        in_range = in_range && ok;
        const size_t g = (size_t)p0 + (ok ? idx : 0); // an index outside the pair is never dereferenced
        ax[i] = a.pts_a[2 * g]; ay[i] = a.pts_a[2 * g + 1];
        bx[i] = a.pts_b[2 * g]; by[i] = a.pts_b[2 * g + 1];
    }
    if (!in_range) {
        atomicOr(&a.pair_err[pair], 1);
#pragma unroll
        for (int k = 0; k < 9; k++) Fout[k] = __builtin_nan("");
        return;
    }
    // centroids: the eight values summed pairwise (NumPy's order for 8 values), mean distance likewise
    const double cax = (((ax[0] + ax[1]) + (ax[2] + ax[3])) + ((ax[4] + ax[5]) + (ax[6] + ax[7]))) / 8.0;
    const double cay = (((ay[0] + ay[1]) + (ay[2] + ay[3])) + ((ay[4] + ay[5]) + (ay[6] + ay[7]))) / 8.0;
    const double cbx = (((bx[0] + bx[1]) + (bx[2] + bx[3])) + ((bx[4] + bx[5]) + (bx[6] + bx[7]))) / 8.0;
    const double cby = (((by[0] + by[1]) + (by[2] + by[3])) + ((by[4] + by[5]) + (by[6] + by[7]))) / 8.0;
    double da[8], db[8];
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const double ux = ax[i] - cax, uy = ay[i] - cay, wx = bx[i] - cbx, wy = by[i] - cby;
        da[i] = sqrt(ux * ux + uy * uy); db[i] = sqrt(wx * wx + wy * wy);
    }
    const Norm na = make_norm(cax, cay, (((da[0] + da[1]) + (da[2] + da[3])) + ((da[4] + da[5]) + (da[6] + da[7]))) / 8.0);
    const Norm nb = make_norm(cbx, cby, (((db[0] + db[1]) + (db[2] + db[3])) + ((db[4] + db[5]) + (db[6] + db[7]))) / 8.0);
    double acc[45];
#pragma unroll
    for (int k = 0; k < 45; k++) acc[k] = 0.0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        double r[9];
        epi_row(na.s * ax[i] + na.tx, na.s * ay[i] + na.ty, nb.s * bx[i] + nb.tx, nb.s * by[i] + nb.ty, r);
        acc45(acc, r);
    }
    double F[9];
    solve_from_normal_sums(acc, s_V + lane, HYP_LANES, na, nb, F);
#pragma unroll
    for (int k = 0; k < 9; k++) Fout[k] = F[k];
}

// Grid (hypothesis tile, point chunk, pair).  A lane keeps its hypothesis' nine entries in registers; the workgroup stages
// SCORE_CHUNK points of the pair in LDS and every lane walks them (all lanes read the same point: an LDS broadcast).
__global__ __launch_bounds__(SCORE_THREADS) void fund_score_kernel(FundArgs a)
{
    __shared__ double s_pts[SCORE_CHUNK][4];
    const int tid = threadIdx.x, pair = blockIdx.z, h = blockIdx.x * SCORE_THREADS + tid;
    const int p0 = a.offset[pair], n = a.offset[pair + 1] - p0;
    const int c0 = blockIdx.y * SCORE_CHUNK;
    if (c0 >= n) return; // the whole workgroup leaves: the grid's chunk count is that of the largest pair
    const int m = n - c0 < SCORE_CHUNK ? n - c0 : SCORE_CHUNK;
    for (int i = tid; i < m; i += SCORE_THREADS) {
        const size_t g = (size_t)p0 + c0 + i;
        s_pts[i][0] = a.pts_a[2 * g]; s_pts[i][1] = a.pts_a[2 * g + 1];
        s_pts[i][2] = a.pts_b[2 * g]; s_pts[i][3] = a.pts_b[2 * g + 1];
    }
    __syncthreads();
    if (h >= a.H) return;
    double F[9];
    const double* Fh = a.F_all + ((size_t)pair * a.H + h) * 9;
#pragma unroll
    for (int k = 0; k < 9; k++) F[k] = Fh[k];
    if (!(F[0] == F[0])) return; // an invalid hypothesis is all NaN: it scores 0
    const double thr2 = a.thr2;
    int cnt = 0;
#pragma unroll 4
    for (int i = 0; i < m; i++) cnt += is_inlier(F, s_pts[i][0], s_pts[i][1], s_pts[i][2], s_pts[i][3], thr2) ? 1 : 0;
    if (cnt) atomicAdd(&a.counts[(size_t)pair * a.H + h], cnt); // integer: the sum does not depend on the order of arrival
}

// One workgroup per pair: the valid hypothesis with the most inliers, the lowest index on ties.
__global__ __launch_bounds__(256) void fund_select_kernel(FundArgs a)
{
    __shared__ int s_cnt[256], s_idx[256];
    const int tid = threadIdx.x, pair = blockIdx.x;
    int best = -1, bi = -1;
    for (int h = tid; h < a.H; h += 256) { // ascending h, strict '>': the lowest index of this thread's maxima
        const double f0 = a.F_all[((size_t)pair * a.H + h) * 9];
        if (!(f0 == f0)) continue;
        const int c = a.counts[(size_t)pair * a.H + h];
        if (c > best) { best = c; bi = h; }
    }
    s_cnt[tid] = best; s_idx[tid] = bi;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) {
            const int c2 = s_cnt[tid + o], i2 = s_idx[tid + o];
            if (i2 >= 0 && (s_idx[tid] < 0 || c2 > s_cnt[tid] || (c2 == s_cnt[tid] && i2 < s_idx[tid]))) { s_cnt[tid] = c2; s_idx[tid] = i2; }
        }
        __syncthreads();
    }
    const int win = s_idx[0], cnt = s_cnt[0];
    int code = win;
    if (a.pair_err[pair]) code = FUND_ERR_SAMPLE;
    else if (win < 0 || cnt < 8) code = FUND_ERR_DEGENERATE;
    if (tid == 0) { a.status[2 * pair] = code; a.status[2 * pair + 1] = code >= 0 ? cnt : 0; }
    if (code >= 0 && tid < 9) a.F_sample[9 * pair + tid] = a.F_all[((size_t)pair * a.H + win) * 9 + tid];
}

// Grid (point chunk, pair): the inlier byte of every point under the pair's winner (zero for a failed pair).
__global__ __launch_bounds__(256) void fund_mask_kernel(FundArgs a)
{
    const int pair = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    const int p0 = a.offset[pair], n = a.offset[pair + 1] - p0;
    if (i >= n) return;
    const int win = a.status[2 * pair];
    const size_t g = (size_t)p0 + i;
    if (win < 0) { a.inlier[g] = 0; return; }
    double F[9];
#pragma unroll
    for (int k = 0; k < 9; k++) F[k] = a.F_all[((size_t)pair * a.H + win) * 9 + k];
    a.inlier[g] = is_inlier(F, a.pts_a[2 * g], a.pts_a[2 * g + 1], a.pts_b[2 * g], a.pts_b[2 * g + 1], a.thr2) ? 1 : 0;
}

// One workgroup per pair: steps 1-4 of the definition over the winner's inliers.  Three passes over the pair's points, each
// thread over the points tid, tid + 256, ... in order, then block_sum's fixed tree: centroids, mean distances, the 45 sums.
__global__ __launch_bounds__(REFIT_THREADS) void fund_refit_kernel(FundArgs a)
{
    __shared__ double s_part[4];
    __shared__ double s_sum[45], s_V[81];
    __shared__ int s_ok;
    const int tid = threadIdx.x, pair = blockIdx.x;
    if (a.status[2 * pair] < 0) return; // uniform over the workgroup
    const int p0 = a.offset[pair], n = a.offset[pair + 1] - p0;
    const double cnt = (double)a.status[2 * pair + 1];
    double s0 = 0, s1 = 0, s2 = 0, s3 = 0;
    for (int i = tid; i < n; i += REFIT_THREADS) {
        const size_t g = (size_t)p0 + i;
        if (!a.inlier[g]) continue;
        s0 += a.pts_a[2 * g]; s1 += a.pts_a[2 * g + 1]; s2 += a.pts_b[2 * g]; s3 += a.pts_b[2 * g + 1];
    }
    const double cax = block_sum(s0, s_part) / cnt, cay = block_sum(s1, s_part) / cnt;
    const double cbx = block_sum(s2, s_part) / cnt, cby = block_sum(s3, s_part) / cnt;
    s0 = 0; s1 = 0;
    for (int i = tid; i < n; i += REFIT_THREADS) {
        const size_t g = (size_t)p0 + i;
        if (!a.inlier[g]) continue;
        const double ux = a.pts_a[2 * g] - cax, uy = a.pts_a[2 * g + 1] - cay, wx = a.pts_b[2 * g] - cbx, wy = a.pts_b[2 * g + 1] - cby;
        s0 += sqrt(ux * ux + uy * uy); s1 += sqrt(wx * wx + wy * wy);
    }
    const Norm na = make_norm(cax, cay, block_sum(s0, s_part) / cnt);
    const Norm nb = make_norm(cbx, cby, block_sum(s1, s_part) / cnt);
    double acc[45];
#pragma unroll
    for (int k = 0; k < 45; k++) acc[k] = 0.0;
    for (int i = tid; i < n; i += REFIT_THREADS) {
        const size_t g = (size_t)p0 + i;
        if (!a.inlier[g]) continue;
        double r[9];
        epi_row(na.s * a.pts_a[2 * g] + na.tx, na.s * a.pts_a[2 * g + 1] + na.ty, nb.s * a.pts_b[2 * g] + nb.tx,
                nb.s * a.pts_b[2 * g + 1] + nb.ty, r);
        acc45(acc, r);
    }
#pragma unroll
    for (int k = 0; k < 45; k++) {
        const double v = block_sum(acc[k], s_part);
        if (tid == 0) s_sum[k] = v;
    }
    if (tid == 0) { // one lane solves
        double F[9];
#pragma unroll
        for (int k = 0; k < 45; k++) acc[k] = s_sum[k];
        const bool ok = solve_from_normal_sums(acc, s_V, 1, na, nb, F);
        if (ok)
            for (int k = 0; k < 9; k++) a.F_refit[9 * pair + k] = F[k];
        else { // inliers that do not span a model: reported, never returned
            a.status[2 * pair] = FUND_ERR_DEGENERATE; a.status[2 * pair + 1] = 0;
        }
        s_ok = ok ? 1 : 0;
    }
    __syncthreads();
    if (!s_ok) // a failed pair has no mask either
        for (int i = tid; i < n; i += REFIT_THREADS) a.inlier[(size_t)p0 + i] = 0;
}

void launch_fundamental_ransac(const FundArgs& a, hipStream_t s)
{
    hipLaunchKernelGGL(fund_hypotheses_kernel, dim3((a.H + HYP_LANES - 1) / HYP_LANES, a.n_pairs), dim3(HYP_LANES), 0, s, a);
    hipLaunchKernelGGL(fund_score_kernel, dim3((a.H + SCORE_THREADS - 1) / SCORE_THREADS, (a.max_n + SCORE_CHUNK - 1) / SCORE_CHUNK, a.n_pairs),
                       dim3(SCORE_THREADS), 0, s, a);
    hipLaunchKernelGGL(fund_select_kernel, dim3(a.n_pairs), dim3(256), 0, s, a);
    hipLaunchKernelGGL(fund_mask_kernel, dim3((a.max_n + 255) / 256, a.n_pairs), dim3(256), 0, s, a);
    if (a.F_refit) hipLaunchKernelGGL(fund_refit_kernel, dim3(a.n_pairs), dim3(REFIT_THREADS), 0, s, a);
}

} // namespace mocap
