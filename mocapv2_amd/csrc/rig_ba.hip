// rig_ba.hip -- bundle adjustment of a whole rig on the device (FP64): the poses of cameras 1..C-1 and every 3-D point over
// exactly the observations that exist, by sparse Levenberg-Marquardt with a Schur complement on the points.
//
// Generalises reference lib/Helpers.py:158-176 (bundle_adjustment: SciPy over the 6 parameters of camera 1, every point
// re-triangulated per evaluation, points any camera missed dropped).  The reference has no N-camera counterpart: the contract
// is the definition of DESIGN.md section 2, restated in NumPy by tests/rig_ba_ref.py.
// The observation layout, the loss, the six launches of an iteration and the order of every sum are rig_lm.h's, written once
// for this solver and rig_selfcal.hip's.  This file holds what is this solver's own: its camera block -- the 6 columns of
// lm.h's pose_columns for cameras 1..C-1, camera 0 fixed, every lens constant from the context's camera table, so the reduced
// system is 6 (C - 1) square -- and its Schur kernel:
//   rig_schur_kernel      grid (camera pair a <= b, chunk of points): the 6x6 blocks W_a V*^-1 W_b^T and, on the diagonal,
//                         W_a V*^-1 g_n, a lane walking points with all 42 sums in registers, summed per workgroup
#include "rig_lm.h"

namespace mocap {

constexpr int SCHUR_CHUNK = 1024;   // points per workgroup of rig_schur_kernel

__global__ void rig_schur_kernel(RigArgs a);

struct PoseBlock {
    static constexpr int P = 6, FIRST = 1;
    using Lenses = const CameraTable*;
    static __device__ __forceinline__ Lenses lenses(const RigArgs& a, int) { return a.cams; }
    static __device__ __forceinline__ Lenses lenses_io(const RigArgs& a) { return a.cams; }
    static __device__ __forceinline__ Lens lens(Lenses tab, int c)
    {
        return Lens{tab->K[c][0], tab->K[c][4], tab->K[c][2], tab->K[c][5],
                    tab->dist[c][0], tab->dist[c][1], tab->dist[c][2], tab->dist[c][3], tab->dist[c][4]};
    }
    static __device__ __forceinline__ void columns(const RigArgs&, int, const Lens&, const Projected& o, const double q[3], double jc[2][P])
    {
#pragma unroll
        for (int i = 0; i < 2; i++) pose_columns(o.A[i], q, jc[i]);
    }
    static __device__ __forceinline__ void init_lenses(const RigArgs&, int, int) {}
    static __device__ __forceinline__ void count(const RigArgs&, uint32_t) {}
    static __device__ __forceinline__ bool fixed(const RigArgs&, int, int) { return false; }
    static __device__ __forceinline__ void step_lenses(const RigArgs&, int, int, const double*) {}
    static __device__ __forceinline__ void return_lenses(const RigArgs&, int, int, int) {}
    static void launch_check(const RigArgs&, hipStream_t) {}
    static void launch_schur(const RigArgs& a, hipStream_t s) { hipLaunchKernelGGL(rig_schur_kernel, dim3(a.n_pairs, a.n_chunks), dim3(256), 0, s, a); }
    static int schur_chunk(int) { return SCHUR_CHUNK; }
};

// Grid (pair of free cameras a <= b, chunk of SCHUR_CHUNK points).  A thread walks the points tid, tid + 256, ... of the chunk;
// a point seen by both cameras adds W_a V*^-1 W_b^T (36 sums) and, for a == b, W_a V*^-1 g_n (6).
__global__ __launch_bounds__(256) void rig_schur_kernel(RigArgs a)
{
    __shared__ double s_red[4][42];
    if (gated(a.state)) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, pair = blockIdx.x, chunk = blockIdx.y;
    int ca, cb;
    pair_cameras<PoseBlock>(pair, a.C, ca, cb);
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

RigSolver rig_pose_solver() { return rig_solver<PoseBlock>(); }

} // namespace mocap
