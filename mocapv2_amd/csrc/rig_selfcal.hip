// rig_selfcal.hip -- bundle adjustment of a whole rig that also refines every camera's lens, on the device (FP64): per camera
// fx, fy, cx, cy, k1, k2, p1, p2, k3 (camera 0 included), the poses of cameras 1..C-1 and every 3-D point, over exactly the
// observations that exist, by sparse Levenberg-Marquardt with a Schur complement on the points.
//
// The reference has no counterpart (its intrinsics come from board views alone, CalculateCameraIntrinsic.py:58, and its bundle
// adjustment, lib/Helpers.py:158-176, moves one pose): the contract is the definition of DESIGN.md section 2, restated in NumPy
// by tests/rig_selfcal_ref.py.  The problem, the observation layout, the loss, the phases and the order of every sum are
// rig_lm.h's, shared with rig_ba.hip; what changes is the camera block, 15 wide -- the 9 lens columns of lm.h's lens_columns,
// then the 6 of pose_columns -- for every camera, so the reduced system is 15 C square, and the lenses are part of the state
// (kd, current and trial like the poses).  A caller's mask frees lens parameters per camera; a fixed column (a masked lens
// parameter, camera 0's pose) is set to zero in the observation's Jacobian, which zeroes its rows of U, W and g, and the
// reduce kernel writes 1 on its diagonal of S: its step is exactly 0, every block keeps one shape and nothing is compacted.
// At init the block also counts every camera's observations, and selfcal_check_kernel refuses a camera whose mask frees more
// than half as many lens parameters as it has observations.  Its Schur kernel:
//   selfcal_schur_kernel      grid (chunk of points, camera pair a <= b): a THREAD owns one of the 225 entries of W_a V*^-1
//                             W_b^T or, on the diagonal, one of the 15 of W_a V*^-1 g_n, and adds the chunk's points in order
//                             (a lane that owned a point would hold 240 sums: 480 registers)
#include "rig_lm.h"

namespace mocap {

constexpr int SCHUR_CHUNK = 256;    // points per workgroup of selfcal_schur_kernel at least (a thread walks them all), and chunks at most

__global__ void selfcal_check_kernel(RigArgs a);
__global__ void selfcal_schur_kernel(RigArgs a);

struct LensBlock {
    static constexpr int P = 15, FIRST = 0;
    using Lenses = const double*;
    static __device__ __forceinline__ Lenses lenses(const RigArgs& a, int buf) { return a.kd + (size_t)buf * 9 * a.C; }
    static __device__ __forceinline__ Lenses lenses_io(const RigArgs& a) { return a.kd_io; }
    static __device__ __forceinline__ Lens lens(Lenses kd, int c)
    {
        const double* k = kd + 9 * c;
        return Lens{k[0], k[1], k[2], k[3], k[4], k[5], k[6], k[7], k[8]};
    }
    // the lens columns, then the pose's; the columns whose bit of free_cols[c] is clear set to zero
    static __device__ __forceinline__ void columns(const RigArgs& a, int c, const Lens& lens, const Projected& o, const double q[3], double jc[2][P])
    {
        const int free = a.free_cols[c];
        lens_columns(lens, o, jc[0], jc[1]);
#pragma unroll
        for (int i = 0; i < 2; i++) {
            pose_columns(o.A[i], q, jc[i] + 9);
#pragma unroll
            for (int j = 0; j < P; j++) jc[i][j] = ((free >> j) & 1) ? jc[i][j] : 0.0;
        }
    }
    static __device__ __forceinline__ void init_lenses(const RigArgs& a, int gid, int stride)
    {
        for (int i = gid; i < 9 * a.C; i += stride) a.kd[i] = a.kd_io[i];
    }
    // (integer atomics; the counts were zeroed with the state record)
    static __device__ __forceinline__ void count(const RigArgs& a, uint32_t mask)
    {
        for (uint32_t m = mask; m; m &= m - 1) atomicAdd(&a.cam_count[__ffs(m) - 1], 1);
    }
    static __device__ __forceinline__ bool fixed(const RigArgs& a, int c, int i) { return !((a.free_cols[c] >> i) & 1); }
    static __device__ __forceinline__ void step_lenses(const RigArgs& a, int cur, int c, const double* d)
    {
        const double* kd = lenses(a, cur);
        double* trial_kd = a.kd + (size_t)(1 - cur) * 9 * a.C;
        for (int k = 0; k < 9; k++) trial_kd[9 * c + k] = kd[9 * c + k] + d[k];
    }
    static __device__ __forceinline__ void return_lenses(const RigArgs& a, int cur, int gid, int stride)
    {
        const double* kd = lenses(a, cur);
        for (int i = gid; i < 9 * a.C; i += stride) a.kd_io[i] = kd[i];
    }
    static void launch_check(const RigArgs& a, hipStream_t s) { hipLaunchKernelGGL(selfcal_check_kernel, dim3(1), dim3(64), 0, s, a); }
    static void launch_schur(const RigArgs& a, hipStream_t s) { hipLaunchKernelGGL(selfcal_schur_kernel, dim3(a.n_chunks, a.n_pairs), dim3(256), 0, s, a); }
    // points per workgroup of the Schur kernel: SCHUR_CHUNK, or what leaves SCHUR_CHUNK chunks (the partials' memory stays bounded)
    static int schur_chunk(int N) { const int c = (N + SCHUR_CHUNK - 1) / SCHUR_CHUNK; return c > SCHUR_CHUNK ? c : SCHUR_CHUNK; }
};

// One workgroup: a camera whose mask is not 0 needs at least twice as many observations as it has free lens parameters.
__global__ __launch_bounds__(64) void selfcal_check_kernel(RigArgs a)
{
    const int c = threadIdx.x;
    if (c >= a.C) return;
    const int lens = a.free_cols[c] & 0x1ff;
    if (lens != 0 && a.cam_count[c] < 2 * __popc(lens)) atomicOr(&a.state->layout_err, 1);
}

// Grid (chunk of a.schur_chunk points, pair of cameras a <= b).  Thread e < 225 owns entry (e / 15, e % 15) of W_a V*^-1 W_b^T,
// thread 225 + i entry i of W_a V*^-1 g_n (a == b only); each adds the chunk's points that both cameras see, in ascending order.
__global__ __launch_bounds__(256) void selfcal_schur_kernel(RigArgs a)
{
    constexpr int P = LensBlock::P, BLK = RigDims<LensBlock>::BLK;
    if (gated(a.state)) return;
    const int tid = threadIdx.x, pair = blockIdx.y, chunk = blockIdx.x;
    if (tid >= BLK) return; // (no barrier below)
    int ca, cb;
    pair_cameras<LensBlock>(pair, a.C, ca, cb);
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
    a.schur_part[((size_t)chunk * a.n_pairs + pair) * BLK + tid] = acc;
}

RigSolver rig_lens_solver() { return rig_solver<LensBlock>(); }

} // namespace mocap
