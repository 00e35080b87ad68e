// correspond.hip -- epipolar correspondence of one time step's points, with the triangulation and reprojection error of
// every candidate group (FP64).
//
// Replaces, per time step, reference lib/Helpers.py:178-280 (find_point_correspondance_and_object_points)
// and its callees triangulate_point(s) (:43-99) and calculate_reprojection_error(s) (:102-143), including
// the two OpenCV primitives they use (cv.computeCorrespondEpilines :207, cv.projectPoints :133; geom_dev.h).
// The library is built with -ffp-contract=off: every product and sum below is a separately rounded FP64
// (or, where the reference rounds to float32, FP32) operation, as in the NumPy/OpenCV path.
//
// Work decomposition: one workgroup per time step.  (root, camera) pairs are scored one per lane; the
// candidate groups of all roots of the time step (the reference's cartesian expansion) are flattened into one
// index space and triangulated one group per lane; per-root error means use NumPy's pairwise summation order.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <mutex>
#include "kernels.h"
#include "geom_dev.h"
#include "correspond_dev.h"

namespace mocap {

namespace {

constexpr int MAXM = 16; // candidate matches kept per (root, camera)

// numpy's pairwise_sum for any n, without recursion and without a stack: the leaves (runs of <= 128 values) are visited
// in order -- the leaf holding offset o is found by walking down from the root, which also yields the path (bit d set =
// right child at depth d) --, and a finished subtree's sum is parked IN the array, at the subtree's first offset (those
// values are consumed by then).  A node's left child starts at the node's own offset, so "left + right" of a node whose
// right child has just been finished reads a[offset of the node].  The array is overwritten.  Same additions in the same
// order as numpy's recursion: n2 = (n / 2) rounded down to a multiple of 8, left = [0, n2), right = [n2, n).
__device__ double np_pairwise_sum(double* a, int n)
{
    if (n <= 128) return np_block_sum(a, n);
    int o = 0;
    double ret = 0.;
    while (o < n) {
        int off = 0, len = n, depth = 0;
        uint32_t path = 0;
        while (len > 128) {
            int n2 = len / 2; n2 -= n2 % 8;
            if (o < off + n2) len = n2;
            else { off += n2; len -= n2; path |= 1u << depth; }
            depth++;
        }
        ret = np_block_sum(a + off, len);
        o = off + len;
        // every ancestor this leaf completes as the last leaf of its right subtree: deepest first
        while (depth > 0 && ((path >> (depth - 1)) & 1u)) {
            depth--;
            int poff = 0, plen = n; // the ancestor at `depth`: walk down the same path
            for (int d = 0; d < depth; d++) {
                int n2 = plen / 2; n2 -= n2 % 8;
                if ((path >> d) & 1u) { poff += n2; plen -= n2; } else plen = n2;
            }
            ret = a[poff] + ret;
        }
        if (depth > 0) { // a left child is complete: park its sum where its parent will look for it
            int poff = 0, plen = n;
            for (int d = 0; d < depth - 1; d++) {
                int n2 = plen / 2; n2 -= n2 % 8;
                if ((path >> d) & 1u) { poff += n2; plen -= n2; } else plen = n2;
            }
            a[poff] = ret;
        }
    }
    return ret;
}

} // namespace

// LDS plan of correspond_kernel (dynamic shared memory), the same on host and device.  What the kernel cannot do without
// comes first (camera block, counts, candidate lists); the staged points and the per-group errors take what `budget` leaves
// (both have a fallback: points from global memory, errors in the context's scratch array).
struct CorrLds {
    int cam, F, pts, errs, rerr, ints, nm, midx, total; // byte offsets
    int stage_pts, err_cap;
};
__host__ __device__ inline CorrLds corr_lds_plan(int P, int C, int budget)
{
    CorrLds L;
    int o = 0;
    L.cam = o; o += C * CAM_ROW * 8;            // one row per camera (correspond_dev.h)
    L.F = o; o += (C > 1 ? C - 1 : 0) * 9 * 8;
    L.rerr = o; o += P * 8;
    L.ints = o; o += (3 * P + 2 + 32) * 4;      // G[P], goff[P + 1], slot[P], counts[32]
    L.nm = o; o += P * C;
    L.midx = o; o += P * C * MAXM;
    o = (o + 15) & ~15;
    L.stage_pts = C * P <= 2048 && o + C * P * 16 + 128 * 8 <= budget; // all image points of the time step in LDS (32 KB at most)
    L.pts = o; o += L.stage_pts ? C * P * 16 : 0;
    int cap = (budget - o) / 8;                 // per-group errors in LDS when the time step has no more groups than this
    L.err_cap = cap > 1024 ? 1024 : (cap < 0 ? 0 : cap);
    L.errs = o; o += L.err_cap * 8;
    L.total = (o + 15) & ~15;
    return L;
}

namespace {

// the LDS pointers of one workgroup, from the plan
struct CorrShared {
    double* cam;        // [C][CAM_ROW]
    double (*Fm)[9];    // [C - 1]
    double *spts, *serr, *rerr;
    int *G, *goff, *slot, *scnt; // groups per root, their offsets in the flat group index, output slot per root, counts per camera
    uint8_t *nm, *midx; // [P][C] candidates per (root, camera), [P][C][MAXM] their point indices
    int stage_pts, err_cap;
};
__device__ __forceinline__ CorrShared corr_shared(unsigned char* smem, const CorrArgs& a)
{
    const CorrLds L = corr_lds_plan(a.P, a.C, a.lds_budget);
    CorrShared S;
    S.cam = (double*)(smem + L.cam);
    S.Fm = (double (*)[9])(smem + L.F);
    S.spts = (double*)(smem + L.pts);
    S.serr = (double*)(smem + L.errs);
    S.rerr = (double*)(smem + L.rerr);
    S.G = (int*)(smem + L.ints);
    S.goff = S.G + a.P;
    S.slot = S.goff + a.P + 1;
    S.scnt = S.slot + a.P;
    S.nm = smem + L.nm;
    S.midx = smem + L.midx;
    S.stage_pts = L.stage_pts;
    S.err_cap = L.err_cap;
    return S;
}

// point p of camera c: from LDS when the plan staged the points, else from global memory
template <typename PT>
__device__ __forceinline__ void get_point(const CorrArgs& a, const CorrShared& S, int t, int c, int p, double& x, double& y)
{
    if (S.stage_pts) { x = S.spts[2 * (c * a.P + p)]; y = S.spts[2 * (c * a.P + p) + 1]; }
    else load_pt<PT>(a.pts, point_base(a, t, c) + p, x, y);
}

// ---- the one round of loads: counts, points, cameras, fundamental matrices; then the projection matrices and the count check.
// Leaves *s_err at 0, 2 or 3 (checked_count) behind a barrier.
template <typename PT>
__device__ __forceinline__ void load_step(const CorrArgs& a, const CorrShared& S, int t, int* s_err, int* s_nout)
{
    const int C = a.C, tid = threadIdx.x, nth = blockDim.x;
    if (tid == 0) { *s_err = 0; *s_nout = 0; }
    if (tid < C) S.scnt[tid] = a.counts[(size_t)t * a.cnt_st + (size_t)tid * a.cnt_sc];
    if (S.stage_pts) stage_step_points<PT>(S.spts, a, t, tid, nth);
    stage_camera_rows<CAM_ROW>(S.cam, a.cams, C, tid, nth);
    for (int w = tid; w < (C - 1) * 9; w += nth) S.Fm[w / 9][w % 9] = a.cams->F[w / 9][w % 9];
    __syncthreads();
    form_projections<CAM_ROW>(S.cam, C, tid, nth);
    if (tid < C) checked_count(S.scnt, tid, a.P, s_err);
    __syncthreads();
}

// ---- per (root, camera) candidate lists, sorted by distance to the epipolar line; a 17th candidate raises *s_err = 1 ----------
template <typename PT>
__device__ __forceinline__ void candidate_lists(const CorrArgs& a, const CorrShared& S, int t, int n0, int* s_err)
{
    const int C = a.C;
    for (int w = threadIdx.x; w < n0 * (C - 1); w += blockDim.x) {
        int j = w / (C - 1), i = 1 + w % (C - 1);
        double rx, ry;
        get_point<PT>(a, S, t, 0, j, rx, ry);
        float line[3];
        epiline(S.Fm[i - 1], (float)rx, (float)ry, line);
        // the candidates of (root j, camera i), kept sorted by distance (stable) in their LDS row.  No per-lane arrays: the
        // distance of an entry that has to be compared again is computed again from its point (a handful of operations, the
        // same value), so nothing here lives in scratch memory
        uint8_t* const mrow = S.midx + ((size_t)j * C + i) * MAXM;
        int k = 0;
        const int ni = S.scnt[i];
        bool over = false;
        for (int p = 0; p < ni; p++) {
            double x, y;
            get_point<PT>(a, S, t, i, p, x, y);
            const double d = epi_distance(line, x, y);
            if (d < a.cutoff) {
                if (k == MAXM) { over = true; break; }
                int q = k++; // stable insertion by distance
                while (q > 0) {
                    const int pq = mrow[q - 1];
                    double xq, yq;
                    get_point<PT>(a, S, t, i, pq, xq, yq);
                    if (!(epi_distance(line, xq, yq) > d)) break;
                    mrow[q] = (uint8_t)pq;
                    q--;
                }
                mrow[q] = (uint8_t)p;
            }
        }
        if (over) atomicMax(s_err, 1);
        S.nm[j * C + i] = (uint8_t)k;
    }
}

// ---- groups per root (the product of its candidate counts) and their offsets in the flat group index; *s_nout = roots with
// groups; *s_err = 1 when a root has more than max_groups or the step more than its share of the error scratch.  Ends in a barrier.
__device__ __forceinline__ void group_offsets(const CorrArgs& a, const CorrShared& S, int n0, int* s_err, int* s_nout)
{
    const int C = a.C, tid = threadIdx.x;
    for (int j = tid; j < n0; j += blockDim.x) {
        long g = C >= 2 ? 1 : 0;
        for (int i = 1; i < C; i++) {
            g *= S.nm[j * C + i];
            if (g > a.max_groups) { atomicMax(s_err, 1); g = 0; break; }
        }
        S.G[j] = (int)g;
    }
    __syncthreads();
    if (tid == 0) {
        int acc = 0, no = 0;
        for (int j = 0; j < n0; j++) {
            S.goff[j] = acc; acc += S.G[j];
            S.slot[j] = S.G[j] > 0 ? no++ : -1;
        }
        S.goff[n0] = acc;
        *s_nout = no;
        if (acc > a.step_budget) *s_err = 1;
    }
    __syncthreads();
}

// The root owning flat group index w < goff[n0]: the last root whose offset is <= w.  It has groups: a root without any shares
// its offset with the root behind it, which is then a later root with an offset <= w (and goff[n0] > w behind the last one).
__device__ __forceinline__ int root_of_group(const CorrShared& S, int n0, int w)
{
    int lo = 0, hi = n0 - 1;
    while (lo < hi) {
        int mid = (lo + hi + 1) >> 1;
        if (S.goff[mid] <= w) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// The cameras' points of group g of root j, in camera order: g's mixed-radix digits over the root's candidate counts, camera 1
// the fastest-varying (reference lib/Helpers.py:239-245).  next(i) is the point of camera i; call it for i = 1 .. C - 1 in turn.
struct GroupWalk {
    const uint8_t *nmj, *mj;
    int rem;
    __device__ __forceinline__ GroupWalk(const CorrShared& S, int C, int j, int g) : nmj(S.nm + j * C), mj(S.midx + (size_t)j * C * MAXM), rem(g) {}
    __device__ __forceinline__ int next(int i)
    {
        const int n_i = nmj[i], dgt = rem % n_i;
        rem /= n_i;
        return mj[i * MAXM + dgt];
    }
};

// ---- one candidate group per lane: DLT, then the mean squared reprojection error into errs[]; a root's first group also
// leaves as the root's point, group and camera-0 index ------------------------------------------------------------------
template <typename PT>
__device__ __forceinline__ void triangulate_groups(const CorrArgs& a, const CorrShared& S, int t, int n0, int total, double* errs)
{
    const int C = a.C;
    for (int w = threadIdx.x; w < total; w += blockDim.x) {
        const int j = root_of_group(S, n0, w), g = w - S.goff[j];
        // pass 1 over the cameras: the group's points into the DLT system.  The points are looked up again in pass 2 instead
        // of being kept in per-lane arrays.
        double x0, y0;
        get_point<PT>(a, S, t, 0, j, x0, y0);
        DltAcc acc;
        acc.clear();
        acc.add_rows(S.cam + oP, x0, y0);
        GroupWalk first_walk(S, C, j, g);
        for (int i = 1; i < C; i++) {
            double x, y;
            get_point<PT>(a, S, t, i, first_walk.next(i), x, y);
            acc.add_rows(S.cam + i * CAM_ROW + oP, x, y);
        }
        double X[3];
        acc.solve(X);
        const float Xf[3] = {(float)X[0], (float)X[1], (float)X[2]};
        // pass 2: squared reprojection errors, summed in numpy's order as they come
        const bool first = g == 0;
        const size_t ro = (size_t)t * a.P + (first ? S.slot[j] : 0);
        NpPairStream sum;
        sum.begin(2 * C);
        GroupWalk walk(S, C, j, g);
        for (int i = 0; i < C; i++) {
            double x = x0, y = y0;
            if (i > 0) get_point<PT>(a, S, t, i, walk.next(i), x, y);
            const double* cam = S.cam + i * CAM_ROW;
            double ex, ey;
            reproj_sq(cam + oK, cam + oD, cam + oR, cam + oT, Xf, x, y, ex, ey);
            sum.push2(ex, ey);
            if (first) { a.root_grp[(ro * C + i) * 2] = x; a.root_grp[(ro * C + i) * 2 + 1] = y; }
        }
        errs[S.goff[j] + g] = sum.res / (double)(2 * C);
        if (first) {
            a.root_xyz[ro * 3] = X[0]; a.root_xyz[ro * 3 + 1] = X[1]; a.root_xyz[ro * 3 + 2] = X[2];
            a.root_idx[ro] = j;
        }
    }
}

// ---- per-root mean over its groups (NumPy pairwise order) ------------------------------------------------------------
__device__ __forceinline__ void root_means(const CorrArgs& a, const CorrShared& S, int t, int n0, double* errs)
{
    for (int j = threadIdx.x; j < n0; j += blockDim.x) {
        if (S.G[j] == 0) continue;
        const double m = np_pairwise_sum(errs + S.goff[j], S.G[j]) / (double)S.G[j];
        S.rerr[S.slot[j]] = m;
        a.root_err[(size_t)t * a.P + S.slot[j]] = m;
    }
}

// ---- argsort of the roots' means (stable), one root per lane, and the time step's count ---------------------------------
__device__ __forceinline__ void rank_and_emit(const CorrArgs& a, const CorrShared& S, int t, int nout)
{
    for (int o = threadIdx.x; o < nout; o += blockDim.x) {
        double eo = S.rerr[o];
        int rank = 0;
        for (int q = 0; q < nout; q++) {
            double eq = S.rerr[q];
            rank += (eq < eo) || (eq == eo && q < o);
        }
        a.order[(size_t)t * a.P + rank] = o;
    }
    if (threadIdx.x == 0) a.n_roots[t] = nout;
}

} // namespace

// One workgroup per time step.  Everything the step needs -- the cameras' image points, the camera table (with the
// projection matrices K [R|t] formed once instead of once per group and camera), the fundamental matrices -- comes in with
// ONE round of global loads into LDS; all scoring, triangulation and ranking then runs from LDS and registers, and the
// results leave with one round of stores.  (The first version loaded points and matrices where it used them: ~100 dependent
// global round trips per time step, 47 us alone but 552 us beside the other batches' streaming scans, whose queued loads every
// one of those round trips waits behind.)  s_err: 1 = groups, 2 = more than P points, 3 = negative count.
template <typename PT>
__global__ __launch_bounds__(256) void correspond_kernel(CorrArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ int s_err, s_nout;
    if (a.prio == 1) __builtin_amdgcn_s_setprio(1);
    else if (a.prio == 2) __builtin_amdgcn_s_setprio(2);
    else if (a.prio == 3) __builtin_amdgcn_s_setprio(3);
    const int t = blockIdx.x, tid = threadIdx.x;
    const CorrShared S = corr_shared(smem, a);

    load_step<PT>(a, S, t, &s_err, &s_nout);
    if (s_err) {
        if (tid == 0) a.n_roots[t] = count_error_code(s_err);
        return;
    }
    const int n0 = S.scnt[0];
    candidate_lists<PT>(a, S, t, n0, &s_err);
    __syncthreads();
    group_offsets(a, S, n0, &s_err, &s_nout);
    if (s_err) {
        if (tid == 0) a.n_roots[t] = CORR_ERR_GROUPS;
        return;
    }
    const int total = S.goff[n0];
    double* const errs = total <= S.err_cap ? S.serr : a.scratch + (size_t)t * a.step_budget;
    triangulate_groups<PT>(a, S, t, n0, total, errs);
    __syncthreads(); // the errors are read back by other lanes of this workgroup
    __threadfence_block();
    root_means(a, S, t, n0, errs);
    __syncthreads();
    rank_and_emit(a, S, t, s_nout);
}

// Dynamic LDS a workgroup of a correspondence kernel may use: 64 KiB without asking; the first call on a device asks the runtime
// for gfx950's whole 160 KiB per workgroup on both instantiations (large P x C: correspond_kernel's candidate lists alone are
// P * C * 16 bytes) and remembers the answer.  user: LDS_USER_* (kernels.h), one per kernel pair.
int workgroup_lds_limit(int user, const void* kernel_f64, const void* kernel_i32)
{
    static std::mutex mu;
    static int limit[LDS_USERS][64] = {{0}}; // per device (the attribute belongs to the function on the current device); 0 = not asked yet
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 64 * 1024 - 64;
    std::lock_guard<std::mutex> lk(mu);
    if (limit[user][dev] == 0) {
        const int want = 160 * 1024 - 64; // minus the kernels' static words
        const bool ok = hipFuncSetAttribute(kernel_f64, hipFuncAttributeMaxDynamicSharedMemorySize, want) == hipSuccess &&
                        hipFuncSetAttribute(kernel_i32, hipFuncAttributeMaxDynamicSharedMemorySize, want) == hipSuccess;
        if (!ok) (void)hipGetLastError();
        limit[user][dev] = ok ? want : 64 * 1024 - 64;
    }
    return limit[user][dev];
}
// the budget the plan is made for: 64 KiB when that holds everything (four workgroups per CU stay possible), else the limit
int correspond_lds_budget(int P, int C)
{
    const int small = 64 * 1024 - 64;
    const CorrLds L = corr_lds_plan(P, C, small);
    if (L.total <= small && L.stage_pts == (C * P <= 2048) && L.err_cap == 1024) return small;
    return workgroup_lds_limit(LDS_USER_CORRESPOND, (const void*)correspond_kernel<double>, (const void*)correspond_kernel<int32_t>);
}
size_t correspond_smem_bytes(int P, int C) { return (size_t)corr_lds_plan(P, C, correspond_lds_budget(P, C)).total; }
bool correspond_fits(int P, int C) { return correspond_smem_bytes(P, C) <= (size_t)correspond_lds_budget(P, C); }

void launch_correspond(const CorrArgs& a_, hipStream_t s)
{
    CorrArgs a = a_;
    a.lds_budget = correspond_lds_budget(a.P, a.C);
    size_t sm = (size_t)corr_lds_plan(a.P, a.C, a.lds_budget).total;
    // threads per time step (MOCAP_CORR_THREADS: A/B switch; one wave per step measured 0.064 against 0.051 ms alone and the
    // same in the three-batch pipeline)
    const int threads = (a.threads == 64 || a.threads == 128) ? a.threads : 256;
    if (a.pts_f64)
        hipLaunchKernelGGL(correspond_kernel<double>, dim3(a.T), dim3(threads), sm, s, a);
    else
        hipLaunchKernelGGL(correspond_kernel<int32_t>, dim3(a.T), dim3(threads), sm, s, a);
}

} // namespace mocap
