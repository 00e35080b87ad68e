// geom_dev.h -- device helpers the geometry kernels share (geom.hip, correspond_visible.hip): the DLT system of a point seen by
// several cameras, the Jacobi eigen-solver behind it, the lens model of a point in both directions (also subpixel.hip's), and the
// typed load of an image point.  Device code only; the files that
// include it are built with -ffp-contract=off, so every operation here is rounded on its own.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mocap {

// eigenvector of the smallest eigenvalue of a symmetric 4x4 (cyclic Jacobi); same rotations as the oracle
__device__ __forceinline__ void smallest_eigvec4(double B[4][4], double v[4])
{
    double V[4][4] = {{1, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}, {0, 0, 0, 1}};
    for (int sweep = 0; sweep < 60; sweep++) {
        double off = 0, diag = 0;
#pragma unroll
        for (int p = 0; p < 4; p++) {
            diag += B[p][p] * B[p][p];
#pragma unroll
            for (int q = p + 1; q < 4; q++) off += B[p][q] * B[p][q];
        }
        if (off == 0.0 || off <= 1e-40 * diag) break;
#pragma unroll
        for (int p = 0; p < 3; p++)
#pragma unroll
            for (int q = p + 1; q < 4; q++) {
                double apq = B[p][q];
                if (apq == 0.0) continue;
                double theta = (B[q][q] - B[p][p]) / (2.0 * apq);
                double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    double bkp = B[k][p], bkq = B[k][q];
                    B[k][p] = c * bkp - s * bkq;
                    B[k][q] = s * bkp + c * bkq;
                }
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    double bpk = B[p][k], bqk = B[q][k];
                    B[p][k] = c * bpk - s * bqk;
                    B[q][k] = s * bpk + c * bqk;
                }
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    double vkp = V[k][p], vkq = V[k][q];
                    V[k][p] = c * vkp - s * vkq;
                    V[k][q] = s * vkp + c * vkq;
                }
            }
    }
    int m = 0;
    double best = B[0][0];
#pragma unroll
    for (int k = 1; k < 4; k++)
        if (B[k][k] < best) { best = B[k][k]; m = k; }
#pragma unroll
    for (int k = 0; k < 4; k++) v[k] = m == 0 ? V[k][0] : (m == 1 ? V[k][1] : (m == 2 ? V[k][2] : V[k][3]));
}

struct DltAcc {
    double B[4][4];
    __device__ __forceinline__ void clear()
    {
#pragma unroll
        for (int j = 0; j < 4; j++)
#pragma unroll
            for (int k = 0; k < 4; k++) B[j][k] = 0.;
    }
    // rows  y*P[2]-P[1]  and  P[0]-x*P[2]  of the DLT system, P = K @ [R|t]  (reference lib/Helpers.py:58-73)
    __device__ __forceinline__ void add(const double* K, const double* R, const double* t, double x, double y)
    {
        double P[12];
#pragma unroll
        for (int r = 0; r < 3; r++)
#pragma unroll
            for (int c = 0; c < 4; c++) {
                double s = 0;
#pragma unroll
                for (int k = 0; k < 3; k++) s += K[3 * r + k] * (c < 3 ? R[3 * k + c] : t[k]);
                P[4 * r + c] = s;
            }
        double r0[4], r1[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            r0[k] = y * P[8 + k] - P[4 + k];
            r1[k] = P[k] - x * P[8 + k];
        }
#pragma unroll
        for (int j = 0; j < 4; j++)
#pragma unroll
            for (int k = 0; k < 4; k++) B[j][k] += r0[j] * r0[k] + r1[j] * r1[k];
    }
    // the same two rows from a projection matrix formed beforehand (the identical sums, formed once per camera)
    __device__ __forceinline__ void add_rows(const double* P, double x, double y)
    {
        double r0[4], r1[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            r0[k] = y * P[8 + k] - P[4 + k];
            r1[k] = P[k] - x * P[8 + k];
        }
#pragma unroll
        for (int j = 0; j < 4; j++)
#pragma unroll
            for (int k = 0; k < 4; k++) B[j][k] += r0[j] * r0[k] + r1[j] * r1[k];
    }
    __device__ __forceinline__ void solve(double X[3])
    {
        double v[4];
        smallest_eigvec4(B, v);
        X[0] = v[0] / v[3]; X[1] = v[1] / v[3]; X[2] = v[2] / v[3];
    }
};

// cv.undistortPoints(p, K, dist, P=K) by calibrate.undistort_points' five fixed-point rounds, the same operations
// (K row-major [9], dist = k1, k2, p1, p2, k3); used by correspond_visible.hip and subpixel.hip
__device__ __forceinline__ void undistort_pt(const double* K, const double* dist, double& px, double& py)
{
    const double fx = K[0], cx = K[2], fy = K[4], cy = K[5];
    const double k1 = dist[0], k2 = dist[1], p1 = dist[2], p2 = dist[3], k3 = dist[4];
    const double x0 = (px - cx) / fx, y0 = (py - cy) / fy;
    double x = x0, y = y0;
    for (int it = 0; it < 5; it++) {
        const double r2 = x * x + y * y;
        const double icd = 1.0 / (1 + ((k3 * r2 + k2) * r2 + k1) * r2);
        const double dx = 2 * p1 * x * y + p2 * (r2 + 2 * x * x), dy = p1 * (r2 + 2 * y * y) + 2 * p2 * x * y;
        x = (x0 - dx) * icd; y = (y0 - dy) * icd;
    }
    px = fx * x + cx; py = fy * y + cy;
}

// The forward lens model of a pixel of the undistorted image: where it lies in the raw frame (the map undistort_pt inverts, with
// the same tangential sums; DESIGN.md section 2, "sub-pixel centroids")
__device__ __forceinline__ void distort_pt(const double* K, const double* dist, double& px, double& py)
{
    const double fx = K[0], cx = K[2], fy = K[4], cy = K[5];
    const double k1 = dist[0], k2 = dist[1], p1 = dist[2], p2 = dist[3], k3 = dist[4];
    const double x = (px - cx) / fx, y = (py - cy) / fy;
    const double r2 = x * x + y * y;
    const double cd = 1 + ((k3 * r2 + k2) * r2 + k1) * r2;
    const double xd = x * cd + (2 * p1 * x * y + p2 * (r2 + 2 * x * x));
    const double yd = y * cd + (p1 * (r2 + 2 * y * y) + 2 * p2 * x * y);
    px = fx * xd + cx; py = fy * yd + cy;
}

template <typename PT>
__device__ __forceinline__ void load_pt(const void* base, size_t idx, double& x, double& y)
{
    const PT* p = (const PT*)base + 2 * idx;
    x = (double)p[0]; y = (double)p[1];
}

} // namespace mocap
