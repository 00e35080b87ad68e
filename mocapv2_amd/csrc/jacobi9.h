// jacobi9.h -- the eigenvector of the smallest eigenvalue of a symmetric 9x9 by cyclic Jacobi: the null vector of a DLT's A^T A
// (fundamental.hip: the 8-point solve; intrinsics.hip: a board view's homography).
#pragma once
#include <hip/hip_runtime.h>

namespace mocap {

// position of element (i, j) = (j, i) of a symmetric 9x9 stored as its upper triangle row by row (45 values)
__device__ __forceinline__ constexpr int sym9(int i, int j) { return i <= j ? i * 9 - i * (i - 1) / 2 + (j - i) : j * 9 - j * (j - 1) / 2 + (i - j); }

// B: the 45 unique entries of the matrix (sym9's order); overwritten.  f: the eigenvector.
// Cyclic Jacobi with the eigenvector matrix, the rotations of smallest_eigvec4 in geom_dev.h.  Every loop over matrix indices is
// unrolled, so every index is a constant: B stays in registers, and with it everything a rotation's angle depends on.  The
// eigenvector matrix V (81 doubles) is only ever updated, never looked at before the end: it lives in LDS at V[(9 i + j) * st],
// st = 64 with one problem per lane ([element][lane]: the lanes of a wave never share a bank), st = 1 for a single solve; its
// loads and stores have constant offsets and no rotation waits for them.  (Both matrices in registers need 126 doubles +
// temporaries > the 256 architectural VGPRs: the compiler parks 18 of them in accumulation registers; both in LDS with
// loop-variable indices: 0.90 ms for the 30 720 hypotheses of a 15-pair batch of fundamental matrices, every rotation waiting
// on dependent LDS round trips with one wave per CU.)
__device__ __forceinline__ void smallest_eigvec9(double B[45], double* V, const int st, double f[9])
{
#pragma unroll
    for (int i = 0; i < 9; i++)
#pragma unroll
        for (int j = 0; j < 9; j++) V[(9 * i + j) * st] = i == j ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 60; sweep++) {
        double off = 0, diag = 0;
#pragma unroll
        for (int p = 0; p < 9; p++) {
            diag += B[sym9(p, p)] * B[sym9(p, p)];
#pragma unroll
            for (int q = p + 1; q < 9; q++) off += B[sym9(p, q)] * B[sym9(p, q)];
        }
        if (!(off > 1e-40 * diag)) break; // converged, or NaN
#pragma unroll
        for (int p = 0; p < 8; p++)
#pragma unroll
            for (int q = p + 1; q < 9; q++) {
                const double apq = B[sym9(p, q)];
                if (apq == 0.0) continue;
                const double theta = (B[sym9(q, q)] - B[sym9(p, p)]) / (2.0 * apq);
                const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
#pragma unroll
                for (int k = 0; k < 9; k++) { // rows / columns p and q outside the 2x2 block: (k, p) and (k, q), k != p, q
                    if (k == p || k == q) continue;
                    const double bkp = B[sym9(k, p)], bkq = B[sym9(k, q)];
                    B[sym9(k, p)] = c * bkp - s * bkq; B[sym9(k, q)] = s * bkp + c * bkq;
                }
                { // the 2x2 block: the rotation from the right, then from the left
                    const double bpp = B[sym9(p, p)], bqq = B[sym9(q, q)];
                    const double pp1 = c * bpp - s * apq, pq1 = s * bpp + c * apq, qp1 = c * apq - s * bqq, qq1 = s * apq + c * bqq;
                    B[sym9(p, p)] = c * pp1 - s * qp1; B[sym9(p, q)] = c * pq1 - s * qq1; B[sym9(q, q)] = s * pq1 + c * qq1;
                }
#pragma unroll
                for (int k = 0; k < 9; k++) {
                    const double vkp = V[(9 * k + p) * st], vkq = V[(9 * k + q) * st];
                    V[(9 * k + p) * st] = c * vkp - s * vkq; V[(9 * k + q) * st] = s * vkp + c * vkq;
                }
            }
    }
    int m = 0;
    double best = B[0];
#pragma unroll
    for (int k = 1; k < 9; k++)
        if (B[sym9(k, k)] < best) { best = B[sym9(k, k)]; m = k; }
#pragma unroll
    for (int k = 0; k < 9; k++) f[k] = V[(9 * k + m) * st];
}

} // namespace mocap
