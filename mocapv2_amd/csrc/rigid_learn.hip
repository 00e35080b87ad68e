// rigid_learn.hip -- rigid-body models learned from a tracked capture: the statistics of the distance between every two of K marker
// identities over a take (mocap_learn_marker_pair_stats), and the model of each of G groups of identities, averaged over the take in the
// group's own frame (mocap_learn_rigid_bodies).  FP64.
//
// The reference has no counterpart: the contract is the definition of DESIGN.md section 2, restated by tests/rigid_learn_ref.py.
// The library is built with -ffp-contract=off: every sum and product below is a separately rounded FP64 operation.  Every sum over
// time is formed per chunk of LEARN_CHUNK = 32 steps in ascending t, starting from 0, and the chunks' partial sums are added in
// ascending chunk: the order is the definition's, not the grid's, so the device and the restatement agree bit for bit.  No
// atomics on global memory at all: counts, minima and maxima travel through the same partials as the sums.
//
// Kernels, each a launch of its own on the caller's stream (the kernel boundary orders a pass behind the one whose model it reads):
//   learn_locate_kernel   one lane per (step, wanted identity): the lowest row below n[t] that holds the identity, or -1
//   pair_chunk_kernel     one workgroup per (chunk, tile of 256 pairs): the chunk's positions staged in LDS ([32][K][3], 48 KB at
//                         K = 64), one lane per pair a <= b walks the 32 steps
//   pair_total_kernel     one lane per pair adds the chunks in order and writes [a][b] and [b][a]
//   learn_seed_kernel     one workgroup per group: the reference step (an LDS integer minimum) and the seed model
//   learn_pose_kernel     one lane per (step, group), a workgroup = one chunk x 4 groups: Horn's pose of the present members
//                         against the current model; then one lane per (group, member, axis) adds the chunk's steps in order
//   learn_total_kernel    one workgroup per group: the chunks in order, then the new model -- or, after the residual pass, the outputs
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <limits.h>
#include "kernels.h"
#include "geom_dev.h"
#include "rigid_dev.h"

namespace mocap {

namespace {

constexpr int THREADS = 256;
constexpr int MM = RIGID_MAX_MARKERS;
constexpr int POSE_GROUPS = 4;                         // groups of a pose workgroup
constexpr int POSE_THREADS = LEARN_CHUNK * POSE_GROUPS;
constexpr int DET_STRIDE = 3 * MM + 1;                 // a lane's detections in LDS: 25 doubles apart, so the lanes spread over the banks
static_assert(MM == 8, "a step's present members are the bits of one byte");
static_assert(3 * MM * POSE_GROUPS <= POSE_THREADS, "one lane per (group, member, axis) adds the chunk's steps");
static_assert(LEARN_MAX_IDS * LEARN_CHUNK * 3 * sizeof(double) + LEARN_MAX_IDS * LEARN_CHUNK <= 65536, "the chunk's positions fit the LDS");

__device__ __forceinline__ bool blind(int n, int Q) { return n < 0 || n > Q; }

// pair p of the K (K + 1) / 2 pairs a <= b, in ascending (a, b)
__device__ __forceinline__ void pair_of(int p, int K, int& a, int& b)
{
    a = 0;
    while (p >= K - a) { p -= K - a; a++; }
    b = a + p;
}

} // namespace

__global__ __launch_bounds__(THREADS) void learn_locate_kernel(const int32_t* __restrict__ n, const int32_t* __restrict__ id, int T, int Q,
                                                               int W, LearnWanted want, int32_t* __restrict__ row)
{
    const long long x = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (x >= (long long)T * W) return;
    const int t = (int)(x / W), k = (int)(x - (long long)t * W);
    const int wanted = want.id[k], rows = n[t];
    int r = -1;
    if (wanted >= 0 && !blind(rows, Q)) {
        const int32_t* ids = id + (size_t)t * Q;
        for (int q = 0; q < rows; q++)
            if (ids[q] == wanted) { r = q; break; }
    }
    row[x] = r;
}

__global__ __launch_bounds__(THREADS) void pair_chunk_kernel(PairArgs a)
{
    __shared__ double s_pos[LEARN_CHUNK * LEARN_MAX_IDS * 3]; // [step][identity][3]
    __shared__ unsigned char s_has[LEARN_CHUNK * LEARN_MAX_IDS];
    const int tid = threadIdx.x, c = blockIdx.x, K = a.K, P = K * (K + 1) / 2;
    const int t0 = c * LEARN_CHUNK;
    for (int x = tid; x < LEARN_CHUNK * K; x += THREADS) {
        const int s = x / K, t = t0 + s;
        const int r = t < a.T ? a.w.row[(size_t)t0 * K + x] : -1;
        s_has[x] = r >= 0;
        if (r >= 0) {
            const double* d = a.xyz + ((size_t)t * a.Q + r) * 3;
            s_pos[3 * x] = d[0]; s_pos[3 * x + 1] = d[1]; s_pos[3 * x + 2] = d[2];
        }
    }
    __syncthreads();
    const int p = blockIdx.y * THREADS + tid;
    if (p >= P) return;
    int ia, ib;
    pair_of(p, K, ia, ib);
    int cnt = 0;
    double lo = 0., hi = 0., sum = 0., sum2 = 0.;
    for (int s = 0; s < LEARN_CHUNK; s++) {
        const int xa = s * K + ia, xb = s * K + ib;
        if (!(s_has[xa] && s_has[xb])) continue;
        if (ia != ib) {
            const double d = dist3(s_pos + 3 * xa, s_pos + 3 * xb);
            if (cnt == 0 || d < lo) lo = d;
            if (cnt == 0 || d > hi) hi = d;
            sum += d;
            sum2 += d * d;
        }
        cnt++;
    }
    const size_t o = (size_t)c * P + p;
    a.w.pcnt[o] = cnt; a.w.pmin[o] = lo; a.w.pmax[o] = hi; a.w.psum[o] = sum; a.w.psum2[o] = sum2;
}

__global__ __launch_bounds__(THREADS) void pair_total_kernel(PairArgs a, int chunks)
{
    const int K = a.K, P = K * (K + 1) / 2;
    const int p = blockIdx.x * THREADS + threadIdx.x;
    if (p >= P) return;
    int ia, ib;
    pair_of(p, K, ia, ib);
    int cnt = 0;
    double lo = 0., hi = 0., sum = 0., sum2 = 0.;
    for (int c = 0; c < chunks; c++) {
        const size_t o = (size_t)c * P + p;
        const int k = a.w.pcnt[o];
        if (k > 0) {
            const double l = a.w.pmin[o], h = a.w.pmax[o];
            if (cnt == 0 || l < lo) lo = l;
            if (cnt == 0 || h > hi) hi = h;
        }
        cnt += k;
        sum += a.w.psum[o];
        sum2 += a.w.psum2[o];
    }
    const int o1 = ia * K + ib, o2 = ib * K + ia;
    a.count[o1] = cnt; a.dmin[o1] = lo; a.dmax[o1] = hi; a.dsum[o1] = sum; a.dsum2[o1] = sum2;
    a.count[o2] = cnt; a.dmin[o2] = lo; a.dmax[o2] = hi; a.dsum[o2] = sum; a.dsum2[o2] = sum2;
}

void launch_marker_pair_stats(const PairArgs& a, hipStream_t s)
{
    const int chunks = (a.T + LEARN_CHUNK - 1) / LEARN_CHUNK, P = a.K * (a.K + 1) / 2, tiles = (P + THREADS - 1) / THREADS;
    if (a.T > 0) {
        const long long cells = (long long)a.T * a.K;
        hipLaunchKernelGGL(learn_locate_kernel, dim3((unsigned)((cells + THREADS - 1) / THREADS)), dim3(THREADS), 0, s, a.n, a.id, a.T, a.Q,
                           a.K, a.ids, a.w.row);
        hipLaunchKernelGGL(pair_chunk_kernel, dim3((unsigned)chunks, (unsigned)tiles), dim3(THREADS), 0, s, a);
    }
    hipLaunchKernelGGL(pair_total_kernel, dim3((unsigned)tiles), dim3(THREADS), 0, s, a, chunks); // T = 0: zeros
}

// the reference step of a group -- the first step at which every member is present -- and the seed model there
__global__ __launch_bounds__(THREADS) void learn_seed_kernel(LearnArgs a)
{
    __shared__ int s_ref;
    const int tid = threadIdx.x, g = blockIdx.x, W = MM * a.G, M = a.n_members[g];
    const bool valid = a.valid >> g & 1u;
    if (tid == 0) s_ref = INT_MAX;
    __syncthreads();
    if (valid)
        for (int t = tid; t < a.T; t += THREADS) {
            const int32_t* r = a.w.row + (size_t)t * W + g * MM;
            bool all = true;
            for (int p = 0; p < M; p++) all = all && r[p] >= 0;
            if (all) { atomicMin(&s_ref, t); break; }
        }
    __syncthreads();
    if (tid != 0) return;
    const int ref = s_ref;
    double* model = a.w.model + g * 3 * MM;
    for (int x = 0; x < 3 * MM; x++) model[x] = 0.;
    a.w.gstate[2 * g] = valid && ref != INT_MAX ? ref : -1;
    a.w.gstate[2 * g + 1] = !valid ? LEARN_ERR_MEMBERS : ref == INT_MAX ? LEARN_ERR_INCOMPLETE : 0;
    if (!valid || ref == INT_MAX) return;
    const int32_t* r = a.w.row + (size_t)ref * W + g * MM;
    double c[3] = {0., 0., 0.};
    for (int p = 0; p < M; p++)
        for (int u = 0; u < 3; u++) c[u] += a.xyz[((size_t)ref * a.Q + r[p]) * 3 + u];
    for (int u = 0; u < 3; u++) c[u] = c[u] / (double)M;
    for (int p = 0; p < M; p++)
        for (int u = 0; u < 3; u++) model[3 * p + u] = a.xyz[((size_t)ref * a.Q + r[p]) * 3 + u] - c[u];
}

// One pass over the take.  residual == 0: a round -- every present member of a used step, mapped back into the model's frame by the
// step's pose, is added to the member's sum.  residual != 0: the squared distance of the posed model point from the member instead.
__global__ __launch_bounds__(POSE_THREADS) void learn_pose_kernel(LearnArgs a, int residual)
{
    __shared__ double s_det[POSE_THREADS * DET_STRIDE];     // a lane's members, [8][3]; then what the lane adds, in their place
    __shared__ double s_model[POSE_GROUPS * 3 * MM];
    __shared__ unsigned char s_on[POSE_THREADS];            // bit p: member p of the lane's (step, group) is added; 0: the step is not used
    const int tid = threadIdx.x, s = tid & (LEARN_CHUNK - 1), gl = tid / LEARN_CHUNK;
    const int c = blockIdx.x, g0 = blockIdx.y * POSE_GROUPS, g = g0 + gl, t = c * LEARN_CHUNK + s, W = MM * a.G;
    if (tid < POSE_GROUPS * 3 * MM) {
        const int gg = g0 + tid / (3 * MM);
        s_model[tid] = gg < a.G ? a.w.model[gg * 3 * MM + tid % (3 * MM)] : 0.;
    }
    double* det = s_det + tid * DET_STRIDE;
    unsigned on = 0u;
    int present = 0;
    if (g < a.G && t < a.T && a.w.gstate[2 * g + 1] == 0) {
        const int32_t* r = a.w.row + (size_t)t * W + g * MM;
#pragma unroll
        for (int p = 0; p < MM; p++) {
            const int q = r[p]; // -1 from n_members on
            if (q < 0) continue;
            const double* d = a.xyz + ((size_t)t * a.Q + q) * 3;
            det[3 * p] = d[0]; det[3 * p + 1] = d[1]; det[3 * p + 2] = d[2];
            on |= 1u << p;
            present++;
        }
    }
    if (present < a.min_present) on = 0u;
    __syncthreads();
    if (on) {
        const double* model = s_model + gl * 3 * MM;
        unsigned long long lab = ~0ull;
#pragma unroll
        for (int p = 0; p < MM; p++)
            if (on >> p & 1u) lab = with_label(lab, p, (unsigned)p);
        Pose o;
        horn(model, det, lab, o);
#pragma unroll
        for (int p = 0; p < MM; p++) {
            if (!(on >> p & 1u)) continue;
            double v[3];
            if (residual) {
                double pr[3];
                transform(o, model + 3 * p, pr);
                const double e0 = pr[0] - det[3 * p], e1 = pr[1] - det[3 * p + 1], e2 = pr[2] - det[3 * p + 2];
                v[0] = (e0 * e0 + e1 * e1) + e2 * e2; v[1] = 0.; v[2] = 0.;
            } else {
                const double e0 = det[3 * p] - o.t[0], e1 = det[3 * p + 1] - o.t[1], e2 = det[3 * p + 2] - o.t[2];
#pragma unroll
                for (int u = 0; u < 3; u++) v[u] = (o.R[u] * e0 + o.R[3 + u] * e1) + o.R[6 + u] * e2; // R^T e
            }
            det[3 * p] = v[0]; det[3 * p + 1] = v[1]; det[3 * p + 2] = v[2];
        }
    }
    s_on[tid] = (unsigned char)on;
    __syncthreads();
    // the chunk's steps in ascending order, one lane per (group, member, axis)
    if (tid >= POSE_GROUPS * 3 * MM) return;
    const int hl = tid / (3 * MM), pu = tid - hl * 3 * MM, p = pu / 3, h = g0 + hl;
    if (h >= a.G) return;
    double sum = 0.;
    int cnt = 0, used = 0;
    for (int k = 0; k < LEARN_CHUNK; k++) {
        const int lane = hl * LEARN_CHUNK + k;
        const unsigned m = s_on[lane];
        used += m != 0u;
        if (!(m >> p & 1u)) continue;
        sum += s_det[lane * DET_STRIDE + pu];
        cnt++;
    }
    const size_t o = (size_t)c * a.G + h;
    a.w.gsum[o * 3 * MM + pu] = sum;
    if (pu % 3 == 0) a.w.gcnt[o * MM + p] = cnt;
    if (pu == 0) a.w.gused[o] = used;
}

// The chunks of a pass in ascending order.  last == 0: the new model, m_p = sum_p / count_p, recentred.  last != 0 (the pass was
// the residual pass): the outputs.
__global__ __launch_bounds__(64) void learn_total_kernel(LearnArgs a, int chunks, int last)
{
    __shared__ double s_sum[3 * MM];
    __shared__ int s_cnt[MM];
    __shared__ int s_used;
    const int tid = threadIdx.x, g = blockIdx.x, M = a.n_members[g];
    const int status = a.w.gstate[2 * g + 1];
    if (tid < 3 * MM) {
        double sum = 0.;
        for (int c = 0; c < chunks; c++) sum += a.w.gsum[((size_t)c * a.G + g) * 3 * MM + tid];
        s_sum[tid] = sum;
    } else if (tid < 4 * MM) {
        int cnt = 0;
        for (int c = 0; c < chunks; c++) cnt += a.w.gcnt[((size_t)c * a.G + g) * MM + tid - 3 * MM];
        s_cnt[tid - 3 * MM] = cnt;
    } else if (tid == 4 * MM) {
        int used = 0;
        for (int c = 0; c < chunks; c++) used += a.w.gused[(size_t)c * a.G + g];
        s_used = used;
    }
    __syncthreads();
    if (tid != 0) return;
    double* model = a.w.model + g * 3 * MM;
    if (!last) {
        if (status != 0) return;
        double c[3] = {0., 0., 0.};
        for (int p = 0; p < M; p++)
            for (int u = 0; u < 3; u++) {
                model[3 * p + u] = s_sum[3 * p + u] / (double)s_cnt[p];
                c[u] += model[3 * p + u];
            }
        for (int u = 0; u < 3; u++) c[u] = c[u] / (double)M;
        for (int p = 0; p < M; p++)
            for (int u = 0; u < 3; u++) model[3 * p + u] = model[3 * p + u] - c[u];
        return;
    }
    a.status[g] = status;
    a.ref_step[g] = a.w.gstate[2 * g];
    a.steps_used[g] = status == 0 ? s_used : 0;
    double all = 0.;
    int n_all = 0;
    for (int p = 0; p < MM; p++) {
        const bool on = status == 0 && p < M;
        a.member_count[g * MM + p] = on ? s_cnt[p] : 0;
        a.member_rms[g * MM + p] = on ? sqrt(s_sum[3 * p] / (double)s_cnt[p]) : 0.;
        for (int u = 0; u < 3; u++) a.model[(g * MM + p) * 3 + u] = on ? model[3 * p + u] : 0.;
        if (on) { all += s_sum[3 * p]; n_all += s_cnt[p]; }
    }
    a.rms[g] = status == 0 ? sqrt(all / (double)n_all) : 0.;
}

void launch_rigid_learn(const LearnArgs& a, hipStream_t s)
{
    const int chunks = (a.T + LEARN_CHUNK - 1) / LEARN_CHUNK, W = MM * a.G;
    const dim3 pose_grid((unsigned)chunks, (unsigned)((a.G + POSE_GROUPS - 1) / POSE_GROUPS));
    if (a.T > 0) {
        const long long cells = (long long)a.T * W;
        hipLaunchKernelGGL(learn_locate_kernel, dim3((unsigned)((cells + THREADS - 1) / THREADS)), dim3(THREADS), 0, s, a.n, a.id, a.T, a.Q,
                           W, a.members, a.w.row);
    }
    hipLaunchKernelGGL(learn_seed_kernel, dim3((unsigned)a.G), dim3(THREADS), 0, s, a); // T = 0: every valid group is incomplete
    for (int pass = 0; pass <= a.rounds; pass++) {
        const int last = pass == a.rounds;
        if (a.T > 0) hipLaunchKernelGGL(learn_pose_kernel, pose_grid, dim3(POSE_THREADS), 0, s, a, last);
        hipLaunchKernelGGL(learn_total_kernel, dim3((unsigned)a.G), dim3(64), 0, s, a, chunks, last);
    }
}

} // namespace mocap
