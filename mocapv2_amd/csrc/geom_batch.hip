// geom_batch.hip -- the geometry calls over a flat batch, one item per lane (FP64): N-view DLT triangulation, reprojection
// error, and the epipolar distance matrix of one camera pair.
//
// Replaces reference lib/Helpers.py triangulate_point(s) (:43-99), calculate_reprojection_error(s) (:102-143) and the
// distance matrix of :205-220, with the OpenCV primitives they use (geom_dev.h).  Built with -ffp-contract=off like
// every geometry source: each product and sum is rounded on its own, as in the NumPy/OpenCV path.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "kernels.h"
#include "geom_dev.h"

namespace mocap {

// triangulate_point over a batch (reference lib/Helpers.py:43-84): invalid entries dropped, fewer than two
// left -> not triangulated; with compact_k the intrinsics are taken by position after the drop (:59-61)
__global__ void triangulate_kernel(TriArgs a)
{
    int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= a.N) return;
    const CameraTable* cams = a.cams;
    DltAcc acc;
    acc.clear();
    int m = 0;
    for (int c = 0; c < a.C; c++) {
        if (!a.valid[(size_t)n * a.C + c]) continue;
        int ki = a.compact_k ? m : c;
        acc.add(cams->K[ki], cams->R[c], cams->t[c], a.pts[((size_t)n * a.C + c) * 2], a.pts[((size_t)n * a.C + c) * 2 + 1]);
        m++;
    }
    if (m <= 1) { a.ok[n] = 0; return; }
    double X[3];
    acc.solve(X);
    a.xyz[3 * n] = X[0]; a.xyz[3 * n + 1] = X[1]; a.xyz[3 * n + 2] = X[2];
    a.ok[n] = 1;
}

// calculate_reprojection_error over a batch (reference lib/Helpers.py:113-143)
__global__ void reproject_kernel(ReprojArgs a)
{
    int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= a.N) return;
    const CameraTable* cams = a.cams;
    float Xf[3] = {(float)a.xyz[3 * n], (float)a.xyz[3 * n + 1], (float)a.xyz[3 * n + 2]};
    int nv = 0;
    for (int c = 0; c < a.C; c++) nv += a.valid[(size_t)n * a.C + c] != 0;
    if (nv <= 1) { a.ok[n] = 0; return; }
    NpPairStream sum; // the errors of the valid cameras, summed in numpy's order as they come (no per-lane array)
    sum.begin(2 * nv);
    int m = 0;
    for (int c = 0; c < a.C; c++) {
        if (!a.valid[(size_t)n * a.C + c]) continue;
        int ki = a.compact_k ? m : c;
        double ex, ey;
        reproj_sq(cams->K[ki], cams->dist[ki], cams->R[c], cams->t[c], Xf, a.pts[((size_t)n * a.C + c) * 2],
                  a.pts[((size_t)n * a.C + c) * 2 + 1], ex, ey);
        sum.push2(ex, ey);
        m++;
    }
    a.mse[n] = sum.res / (double)(2 * nv);
    a.ok[n] = 1;
}

// The distance matrix of reference lib/Helpers.py:205-220 for one camera pair: line of root r = cv.computeCorrespondEpilines
// of the float32 root point under F (:207), distance of candidate p to it by the expression of :217.  One lane per (root,
// candidate) pair; the same `epiline` / `epi_distance` the correspondence kernel scores with.
template <typename PT>
__global__ __launch_bounds__(256) void epipolar_scores_kernel(EpiArgs a)
{
    const long w = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= (long)a.n_roots * a.n_cand) return;
    const int r = (int)(w / a.n_cand), p = (int)(w - (long)r * a.n_cand);
    double rx, ry, x, y;
    load_pt<PT>(a.roots, (size_t)r, rx, ry);
    load_pt<PT>(a.cand, (size_t)p, x, y);
    float line[3];
    epiline(a.cams->F[a.f_index], (float)rx, (float)ry, line);
    a.dist[w] = epi_distance(line, x, y);
    if (a.lines && p == 0) { a.lines[3 * r] = line[0]; a.lines[3 * r + 1] = line[1]; a.lines[3 * r + 2] = line[2]; }
}

void launch_epipolar_scores(const EpiArgs& a, hipStream_t s)
{
    const long n = (long)a.n_roots * a.n_cand;
    const unsigned blocks = (unsigned)((n + 255) / 256);
    if (a.pts_f64) hipLaunchKernelGGL(epipolar_scores_kernel<double>, dim3(blocks), dim3(256), 0, s, a);
    else hipLaunchKernelGGL(epipolar_scores_kernel<int32_t>, dim3(blocks), dim3(256), 0, s, a);
}
void launch_triangulate(const TriArgs& a, hipStream_t s)
{
    hipLaunchKernelGGL(triangulate_kernel, dim3((a.N + 63) / 64), dim3(64), 0, s, a);
}
void launch_reproject(const ReprojArgs& a, hipStream_t s)
{
    hipLaunchKernelGGL(reproject_kernel, dim3((a.N + 63) / 64), dim3(64), 0, s, a);
}

} // namespace mocap
