// rigid_dev.h -- device code the rigid-body kernels share (rigid.hip, rigid_learn.hip): the packed labels of a body's model points,
// a pose, and Horn's closed-form pose of labelled pairs.  FP64, every operation rounded on its own (-ffp-contract=off), the sums in
// the order DESIGN.md section 2 gives: whoever calls these gets the same bits.
#pragma once
#include <hip/hip_runtime.h>
#include "kernels.h"
#include "geom_dev.h"

namespace mocap {

namespace {

constexpr unsigned NO_LABEL = 0xffu;     // a model point without a detection, in the packed labels (one byte per model point)

struct Pose { double R[9], t[3], q[4]; };

__device__ __forceinline__ unsigned label_of(unsigned long long lab, int p) { return (unsigned)(lab >> (8 * p)) & 0xffu; }
__device__ __forceinline__ unsigned long long with_label(unsigned long long lab, int p, unsigned l)
{
    return (lab & ~(0xffull << (8 * p))) | ((unsigned long long)l << (8 * p));
}

__device__ __forceinline__ double dist3(const double* a, const double* b)
{
    const double dx = a[0] - b[0], dy = a[1] - b[1], dz = a[2] - b[2];
    return sqrt((dx * dx + dy * dy) + dz * dz);
}

// R m + t, each row ((R0 m0 + R1 m1) + R2 m2) + t
__device__ __forceinline__ void transform(const Pose& o, const double* m, double out[3])
{
#pragma unroll
    for (int u = 0; u < 3; u++) out[u] = ((o.R[3 * u] * m[0] + o.R[3 * u + 1] * m[1]) + o.R[3 * u + 2] * m[2]) + o.t[u];
}

// Horn's closed-form pose of the pairs (m_p, D_lab[p]) that have a label, in ascending p
__device__ __forceinline__ void horn(const double* model, const double* det, unsigned long long lab, Pose& o)
{
    double cnt = 0., sm[3] = {0., 0., 0.}, sd[3] = {0., 0., 0.};
#pragma unroll
    for (int p = 0; p < RIGID_MAX_MARKERS; p++) {
        const unsigned l = label_of(lab, p);
        if (l == NO_LABEL) continue;
        cnt += 1.;
#pragma unroll
        for (int u = 0; u < 3; u++) { sm[u] += model[3 * p + u]; sd[u] += det[3 * l + u]; }
    }
    double mb[3], db[3];
#pragma unroll
    for (int u = 0; u < 3; u++) { mb[u] = sm[u] / cnt; db[u] = sd[u] / cnt; }
    double S[3][3] = {{0., 0., 0.}, {0., 0., 0.}, {0., 0., 0.}};
#pragma unroll
    for (int p = 0; p < RIGID_MAX_MARKERS; p++) {
        const unsigned l = label_of(lab, p);
        if (l == NO_LABEL) continue;
#pragma unroll
        for (int u = 0; u < 3; u++)
#pragma unroll
            for (int v = 0; v < 3; v++) S[u][v] += (model[3 * p + u] - mb[u]) * (det[3 * l + v] - db[v]);
    }
    double N[4][4];
    N[0][0] = (S[0][0] + S[1][1]) + S[2][2];
    N[1][1] = (S[0][0] - S[1][1]) - S[2][2];
    N[2][2] = (S[1][1] - S[0][0]) - S[2][2];
    N[3][3] = (S[2][2] - S[0][0]) - S[1][1];
    N[0][1] = N[1][0] = S[1][2] - S[2][1];
    N[0][2] = N[2][0] = S[2][0] - S[0][2];
    N[0][3] = N[3][0] = S[0][1] - S[1][0];
    N[1][2] = N[2][1] = S[0][1] + S[1][0];
    N[1][3] = N[3][1] = S[2][0] + S[0][2];
    N[2][3] = N[3][2] = S[1][2] + S[2][1];
#pragma unroll
    for (int r = 0; r < 4; r++)
#pragma unroll
        for (int c = 0; c < 4; c++) N[r][c] = -N[r][c]; // the largest eigenvalue of N is the smallest of -N
    double q[4];
    smallest_eigvec4(N, q);
    const double nrm = sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]);
#pragma unroll
    for (int k = 0; k < 4; k++) q[k] = q[k] / nrm;
    const bool z0 = q[0] == 0., z1 = q[1] == 0., z2 = q[2] == 0.;
    const bool neg = q[0] < 0. || (z0 && q[1] < 0.) || (z0 && z1 && q[2] < 0.) || (z0 && z1 && z2 && q[3] < 0.);
#pragma unroll
    for (int k = 0; k < 4; k++) o.q[k] = neg ? -q[k] : q[k];
    const double w = o.q[0], x = o.q[1], y = o.q[2], z = o.q[3];
    const double ww = w * w, xx = x * x, yy = y * y, zz = z * z;
    const double wx = w * x, wy = w * y, wz = w * z, xy = x * y, xz = x * z, yz = y * z;
    o.R[0] = ((ww + xx) - yy) - zz; o.R[1] = 2.0 * (xy - wz);       o.R[2] = 2.0 * (xz + wy);
    o.R[3] = 2.0 * (xy + wz);       o.R[4] = ((ww - xx) + yy) - zz; o.R[5] = 2.0 * (yz - wx);
    o.R[6] = 2.0 * (xz - wy);       o.R[7] = 2.0 * (yz + wx);       o.R[8] = ((ww - xx) - yy) + zz;
#pragma unroll
    for (int u = 0; u < 3; u++) o.t[u] = db[u] - ((o.R[3 * u] * mb[0] + o.R[3 * u + 1] * mb[1]) + o.R[3 * u + 2] * mb[2]);
}

} // namespace

} // namespace mocap
