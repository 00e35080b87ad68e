// geom_dev.h -- device helpers the geometry kernels share (correspond.hip, correspond_visible.hip, geom_batch.hip,
// ba_residuals.hip): the DLT system of a point seen by several cameras, the Jacobi eigen-solver behind it, the lens model of a
// point in both directions (also subpixel.hip's), the typed load of an image point, NumPy's summation order, and the OpenCV
// restatements (epipolar line, projection of a float32 object point).  Device code only; the files that
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
        add_rows(P, x, y);
    }
    // the two rows from a projection matrix formed beforehand (correspond_dev.h: the identical sums, formed once per camera)
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

__device__ __forceinline__ double np_block_sum(const double* a, int n)
{ // numpy pairwise_sum for n <= 128
    if (n < 8) {
        double r = 0.;
        for (int i = 0; i < n; i++) r += a[i];
        return r;
    }
    double r0 = a[0], r1 = a[1], r2 = a[2], r3 = a[3], r4 = a[4], r5 = a[5], r6 = a[6], r7 = a[7];
    int i;
    for (i = 8; i < n - (n % 8); i += 8) {
        r0 += a[i]; r1 += a[i + 1]; r2 += a[i + 2]; r3 += a[i + 3];
        r4 += a[i + 4]; r5 += a[i + 5]; r6 += a[i + 6]; r7 += a[i + 7];
    }
    double res = ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7));
    for (; i < n; i++) res += a[i];
    return res;
}

// numpy's pairwise_sum of n <= 128 values that arrive two at a time, in order, without keeping them (np_block_sum above on
// the fly; n even).  The values are squares (>= +0), so starting the eight partial sums at +0 instead of a[0..7] adds nothing.
struct NpPairStream {
    double r0, r1, r2, r3, r4, r5, r6, r7, res;
    int nfull, i;
    __device__ __forceinline__ void begin(int n)
    {
        nfull = n < 8 ? 0 : n - (n % 8);
        i = 0;
        r0 = r1 = r2 = r3 = r4 = r5 = r6 = r7 = 0.; res = 0.;
    }
    __device__ __forceinline__ void push2(double a, double b)
    {
        if (i < nfull) {
            // value i goes to partial sum i % 8.  The eight sums are rotated by two after every pair instead of being selected by
            // index (a register cannot be indexed; the compiler would move them to scratch memory): the next pair again lands in
            // r0 / r1, and after nfull values -- a multiple of 8 -- every sum is back in its own place
            r0 += a; r1 += b;
            const double t0 = r0, t1 = r1;
            r0 = r2; r1 = r3; r2 = r4; r3 = r5; r4 = r6; r5 = r7; r6 = t0; r7 = t1;
            i += 2;
            if (i == nfull) res = ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7));
        } else {
            res += a; res += b;
            i += 2;
        }
    }
};

// cv.computeCorrespondEpilines for one float32 point
__device__ __forceinline__ void epiline(const double* F, float xf, float yf, float line[3])
{
    double x = xf, y = yf;
    double a = F[0] * x + F[1] * y + F[2];
    double b = F[3] * x + F[4] * y + F[5];
    double c = F[6] * x + F[7] * y + F[8];
    double nu = a * a + b * b;
    nu = nu ? 1. / sqrt(nu) : 1.;
    a *= nu; b *= nu; c *= nu;
    line[0] = (float)a; line[1] = (float)b; line[2] = (float)c;
}

// The FP64 epipolar line of correspond_visible's definition: F (x, y, 1), scaled to a unit normal without a
// rounding to float32 -- another definition than epiline above, not a variant of it.  false: the line has no direction.
__device__ __forceinline__ bool epiline_f64(const double* F, double x, double y, double& la, double& lb, double& lc)
{
    la = F[0] * x + F[1] * y + F[2];
    lb = F[3] * x + F[4] * y + F[5];
    lc = F[6] * x + F[7] * y + F[8];
    const double nu = la * la + lb * lb;
    if (!(nu > 0.)) return false;
    const double sc = 1. / sqrt(nu);
    la *= sc; lb *= sc; lc *= sc;
    return true;
}

__device__ __forceinline__ double epi_distance(const float line[3], double x, double y)
{ // reference lib/Helpers.py:217
    double a = line[0], b = line[1], c = line[2];
    return fabs(a * x + b * y + c) / sqrt(a * a + b * b);
}

// cv.projectPoints for one float32 object point; squared pixel errors against (px,py)
__device__ __forceinline__ void reproj_sq(const double* K, const double* d, const double* R, const double* t, const float Xf[3],
                          double px, double py, double& ex, double& ey)
{
    double X = Xf[0], Y = Xf[1], Z = Xf[2];
    double x = R[0] * X + R[1] * Y + R[2] * Z + t[0];
    double y = R[3] * X + R[4] * Y + R[5] * Z + t[1];
    double z = R[6] * X + R[7] * Y + R[8] * Z + t[2];
    z = z ? 1. / z : 1;
    x *= z; y *= z;
    double r2 = x * x + y * y, r4 = r2 * r2, r6 = r4 * r2;
    double a1 = 2 * x * y, a2 = r2 + 2 * x * x, a3 = r2 + 2 * y * y;
    double cdist = 1 + d[0] * r2 + d[1] * r4 + d[4] * r6;
    double xd = x * cdist + d[2] * a1 + d[3] * a2;
    double yd = y * cdist + d[2] * a3 + d[3] * a1;
    float u = (float)(xd * K[0] + K[2]), v = (float)(yd * K[4] + K[5]);
    double dx = px - (double)u, dy = py - (double)v;
    ex = dx * dx; ey = dy * dy;
}

} // namespace mocap
