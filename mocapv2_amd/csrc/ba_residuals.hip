// ba_residuals.hip -- the residual vector of the reference's bundle adjustment for a batch of parameter vectors (FP64).
//
// Replaces bundle_adjustment.residual_function (reference lib/Helpers.py:145-167).  Built with -ffp-contract=off like every
// geometry source: each product and sum is rounded on its own, as in the NumPy/SciPy/OpenCV path.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "kernels.h"
#include "geom_dev.h"

namespace mocap {

// scipy Rotation.from_rotvec(v).as_matrix() (reference lib/Helpers.py:152): rotation vector -> unit quaternion -> matrix
__device__ __forceinline__ void rotvec_to_matrix(const double v[3], double Rm[9])
{
    const double angle = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    double scale;
    if (angle <= 1e-3) {
        const double a2 = angle * angle;
        scale = 0.5 - a2 / 48 + a2 * a2 / 3840;
    } else
        scale = sin(angle / 2) / angle;
    const double x = scale * v[0], y = scale * v[1], z = scale * v[2], w = cos(angle / 2);
    const double x2 = x * x, y2 = y * y, z2 = z * z, w2 = w * w;
    const double xy = x * y, zw = z * w, xz = x * z, yw = y * w, yz = y * z, xw = x * w;
    Rm[0] = x2 - y2 - z2 + w2; Rm[1] = 2 * (xy - zw);        Rm[2] = 2 * (xz + yw);
    Rm[3] = 2 * (xy + zw);        Rm[4] = -x2 + y2 - z2 + w2; Rm[5] = 2 * (yz - xw);
    Rm[6] = 2 * (xz - yw);        Rm[7] = 2 * (yz + xw);        Rm[8] = -x2 - y2 + z2 + w2;
}

// bundle_adjustment.residual_function (reference lib/Helpers.py:161-167) for B parameter vectors, one workgroup each:
// params_to_camera_poses (:145-156: camera 0 = identity / zero, cameras 1.. from rotvec + t sextuples) into LDS, then
// triangulate_points (groups holding a None are skipped, :93), then calculate_reprojection_errors, which pairs groups and
// object points POSITIONALLY (:104) and drops pairs seen by fewer than two cameras (:127-128), then the float32 cast (:165).
// Both compactions are block-wide prefix counts, so the residual vector has the reference's length and order.
__global__ __launch_bounds__(256) void ba_residuals_kernel(BaArgs a)
{
    __shared__ double sR[32][9], sT[32][3];
    __shared__ int s_wave[4], s_base;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int C = a.C, N = a.N;
    const CameraTable* cams = a.cams;
    if (tid < C) {
        if (tid == 0) {
            for (int k = 0; k < 9; k++) sR[0][k] = (k % 4 == 0) ? 1.0 : 0.0;
            sT[0][0] = sT[0][1] = sT[0][2] = 0.0;
        } else {
            const double* p = a.params + (size_t)b * 6 * (C - 1) + 6 * (tid - 1);
            const double v[3] = {p[0], p[1], p[2]};
            double Rm[9];
            rotvec_to_matrix(v, Rm);
            for (int k = 0; k < 9; k++) sR[tid][k] = Rm[k];
            sT[tid][0] = p[3]; sT[tid][1] = p[4]; sT[tid][2] = p[5];
        }
    }
    if (tid == 0) s_base = 0;
    __syncthreads();
    double* const obj = a.obj + (size_t)b * N * 3;
    // block-wide exclusive prefix of a flag over the 256 threads of one round; every thread calls it
    auto place = [&](bool flag, int& total) -> int {
        const uint64_t bal = __ballot(flag);
        if (lane == 0) s_wave[wave] = __popcll(bal);
        __syncthreads();
        int off = s_base;
        for (int w = 0; w < wave; w++) off += s_wave[w];
        total = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
        return off + __popcll(bal & ((1ull << lane) - 1ull));
    };
    for (int n0 = 0; n0 < N; n0 += 256) { // triangulate_points: the groups without a None, in order
        const int n = n0 + tid;
        bool full = n < N;
        if (full)
            for (int c = 0; c < C; c++) full = full && a.valid[(size_t)n * C + c] != 0;
        int total;
        const int o = place(full, total);
        if (full) {
            DltAcc acc;
            acc.clear();
            for (int c = 0; c < C; c++)
                acc.add(cams->K[c], sR[c], sT[c], a.pts[((size_t)n * C + c) * 2], a.pts[((size_t)n * C + c) * 2 + 1]);
            double X[3];
            acc.solve(X);
            obj[3 * o] = X[0]; obj[3 * o + 1] = X[1]; obj[3 * o + 2] = X[2];
        }
        __syncthreads();
        if (tid == 0) s_base += total;
        __syncthreads();
    }
    const int nobj = s_base;
    __threadfence_block(); // the object points are read back by other threads of this workgroup
    __syncthreads();
    if (tid == 0) s_base = 0;
    __syncthreads();
    for (int n0 = 0; n0 < nobj; n0 += 256) { // zip(groups, object points): group n with object point n
        const int n = n0 + tid;
        bool has = n < nobj;
        double mse = 0.0;
        if (has) {
            const float Xf[3] = {(float)obj[3 * n], (float)obj[3 * n + 1], (float)obj[3 * n + 2]};
            int nv = 0;
            for (int c = 0; c < C; c++) nv += a.valid[(size_t)n * C + c] != 0;
            has = nv > 1;
            if (has) {
                NpPairStream sum;
                sum.begin(2 * nv);
                int m = 0;
                for (int c = 0; c < C; c++) {
                    if (!a.valid[(size_t)n * C + c]) continue;
                    double ex, ey;
                    reproj_sq(cams->K[m], cams->dist[m], sR[c], sT[c], Xf, a.pts[((size_t)n * C + c) * 2], a.pts[((size_t)n * C + c) * 2 + 1],
                              ex, ey); // intrinsics by position after the None entries are dropped (:121-123,137-138)
                    sum.push2(ex, ey);
                    m++;
                }
                mse = sum.res / (double)(2 * nv);
            }
        }
        int total;
        const int o = place(has, total);
        if (has) a.res[(size_t)b * N + o] = (float)mse;
        __syncthreads();
        if (tid == 0) s_base += total;
        __syncthreads();
    }
    if (tid == 0) a.counts[b] = s_base;
}

void launch_ba_residuals(const BaArgs& a, hipStream_t s)
{
    hipLaunchKernelGGL(ba_residuals_kernel, dim3(a.B), dim3(256), 0, s, a);
}

} // namespace mocap
