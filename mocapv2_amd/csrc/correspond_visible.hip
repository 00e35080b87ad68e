// correspond_visible.hip -- correspondence and triangulation of markers that only some cameras see, from any camera pair (FP64).
//
// The reference has no counterpart (its find_point_correspondance_and_object_points starts from camera 0's points and
// triangulates only groups without a None, lib/Helpers.py:93,178-280): the contract is the definition of DESIGN.md section 2,
// restated by tests/correspond_visible_ref.py.  The library is built with -ffp-contract=off: every product and sum below is a
// separately rounded FP64 operation, in the order the definition gives.
//
// Work decomposition: one workgroup per time step.  One round of global loads brings counts, points, the camera table into
// LDS; the projection matrices, K^-1 and the pair matrices F_ab are formed there.  A pass scores one (pair, i, j) per lane,
// builds one hypothesis per seed and lane (two Jacobi solves, up to C projections), sorts the hypotheses by their key with a
// bitonic network over 16-bit indices, lets one wave walk the sorted list (lane c owns camera c's claim flags) and writes the
// accepted markers, one per lane.  No floating-point atomics; the only atomics hand out list slots, and the sort's key is a
// total order, so the same call gives the same bits.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <mutex>
#include "kernels.h"
#include "geom_dev.h"

namespace mocap {

namespace {

// per camera in LDS, in doubles: P = K [R|t] (12), K (9), dist (5), R (9), t (3), K^-1 (9)
constexpr int CAMW = 47, oP = 0, oK = 12, oD = 21, oR = 26, oT = 35, oKi = 38;
// A hypothesis record: err (8 bytes), key word a << 24 | i << 16 | b << 8 | j (4), members (1; 0 = dropped), accepted (1),
// output row (2), then the member point of every camera (1 byte each, NONE = the camera has none), padded to 8 bytes.
constexpr int REC_HEAD = 16, NONE = 0xff, ORD_END = 0xffff;
__host__ __device__ inline int vis_rec_bytes(int C) { return REC_HEAD + ((C + 7) & ~7); }
__host__ __device__ inline int pow2_at_least(int n) { int p = 1; while (p < n) p <<= 1; return p; }

// LDS plan (dynamic shared memory), the same on host and device: what the kernel cannot do without, then as many hypothesis
// records (and their sort order) as `budget` leaves, a power of two up to 4096.  A pass with more seeds works in the context's scratch.
struct VisLds {
    int cam, F, pts, cnt, pair, claimed, hyp, ord, total; // byte offsets
    int cap;
};
__host__ __device__ inline VisLds vis_lds_plan(int P, int C, int budget)
{
    VisLds L;
    const int pairs = C * (C - 1) / 2, rec = vis_rec_bytes(C);
    int o = 0;
    L.cam = o; o += C * CAMW * 8;
    L.F = o; o += pairs * 72;
    L.pts = o; o += C * P * 16;
    L.cnt = o; o += 32 * 4;
    L.pair = o; o += pairs * 2;
    L.claimed = o; o += C * P;
    o = (o + 15) & ~15;
    int cap = 4096;
    while (cap > 0 && o + cap * (rec + 2) > budget) cap >>= 1;
    L.cap = cap;
    L.hyp = o; o += cap * rec;
    L.ord = o; o += cap * 2;
    L.total = (o + 15) & ~15;
    return L;
}
constexpr int VIS_MIN_CAP = 64; // fewer records than this in LDS: the combination of P and C is refused

struct Rec {
    unsigned char* r;
    __device__ __forceinline__ double& err() const { return *(double*)r; }
    __device__ __forceinline__ uint32_t& key() const { return *(uint32_t*)(r + 8); }
    __device__ __forceinline__ uint8_t& members() const { return r[12]; }
    __device__ __forceinline__ uint8_t& accepted() const { return r[13]; }
    __device__ __forceinline__ uint16_t& row() const { return *(uint16_t*)(r + 14); }
    __device__ __forceinline__ uint8_t& idx(int c) const { return r[REC_HEAD + c]; }
};

// (R_c X + t_c)_z
__device__ __forceinline__ double depth_of(const double* cam, const double X[3])
{
    return cam[oR + 6] * X[0] + cam[oR + 7] * X[1] + cam[oR + 8] * X[2] + cam[oT + 2];
}
// pinhole projection of X (fx, fy, cx, cy of K, as cv.projectPoints and calibrate.undistort_points use them)
__device__ __forceinline__ void pinhole(const double* cam, const double X[3], double& u, double& v)
{
    const double x = cam[oR + 0] * X[0] + cam[oR + 1] * X[1] + cam[oR + 2] * X[2] + cam[oT + 0];
    const double y = cam[oR + 3] * X[0] + cam[oR + 4] * X[1] + cam[oR + 5] * X[2] + cam[oT + 1];
    const double z = depth_of(cam, X);
    const double xn = x / z, yn = y / z;
    u = cam[oK + 0] * xn + cam[oK + 2];
    v = cam[oK + 4] * yn + cam[oK + 5];
}
__device__ __forceinline__ bool finite3(const double X[3]) { return isfinite(X[0]) && isfinite(X[1]) && isfinite(X[2]); }

// X of a hypothesis: the DLT over its members in ascending camera order; false when X is not finite or not in front of every member
__device__ __forceinline__ bool solve_members(const double* cam, const double* spts, int P, int C, const Rec h, double X[3])
{
    DltAcc acc;
    acc.clear();
    for (int c = 0; c < C; c++) {
        const int p = h.idx(c);
        if (p == NONE) continue;
        acc.add_rows(cam + c * CAMW + oP, spts[2 * (c * P + p)], spts[2 * (c * P + p) + 1]);
    }
    acc.solve(X);
    if (!finite3(X)) return false;
    bool front = true;
    for (int c = 0; c < C; c++)
        if (h.idx(c) != NONE && !(depth_of(cam + c * CAMW, X) > 0.)) front = false;
    return front;
}

} // namespace

template <typename PT>
__global__ __launch_bounds__(256) void correspond_visible_kernel(VisArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int C = a.C, P = a.P, t = blockIdx.x, tid = threadIdx.x, nth = blockDim.x;
    const int pairs = C * (C - 1) / 2, REC = vis_rec_bytes(C);
    const VisLds L = vis_lds_plan(P, C, a.lds_budget);
    double* const cam = (double*)(smem + L.cam);
    double* const Fm = (double*)(smem + L.F);
    double* const spts = (double*)(smem + L.pts);
    int* const scnt = (int*)(smem + L.cnt);
    uint8_t* const pair_ab = smem + L.pair;
    uint8_t* const claimed = smem + L.claimed;
    __shared__ int s_err, s_nseed, s_nout, s_acc, s_pm;

    const CameraTable* cams = a.cams;
    auto pbase = [&](int c) { return ((size_t)t * a.pt_st + (size_t)c * a.pt_sc) / 2; };
    // ---- the one round of loads: counts, points (every slot up to P), cameras ----------------------------------------------
    if (tid == 0) { s_err = 0; s_nout = 0; s_pm = 0; }
    if (tid < 32) scnt[tid] = tid < C ? a.counts[(size_t)t * a.cnt_st + (size_t)tid * a.cnt_sc] : 0;
    for (int w = tid; w < C * P; w += nth) {
        const int c = w / P, p = w - c * P;
        double x, y;
        load_pt<PT>(a.pts, pbase(c) + p, x, y);
        spts[2 * w] = x; spts[2 * w + 1] = y;
        claimed[w] = 0;
    }
    for (int w = tid; w < C * 26; w += nth) {
        const int c = w / 26, k = w - c * 26;
        cam[c * CAMW + oK + k] = k < 9 ? cams->K[c][k] : (k < 14 ? cams->dist[c][k - 9] : (k < 23 ? cams->R[c][k - 14] : cams->t[c][k - 23]));
    }
    for (int w = tid; w < pairs; w += nth) { // pair w = (ca, cb), ca < cb, in the order (0,1), (0,2), ..., (C-2,C-1)
        int ca = 0, rem = w;
        while (rem >= C - 1 - ca) { rem -= C - 1 - ca; ca++; }
        pair_ab[2 * w] = (uint8_t)ca; pair_ab[2 * w + 1] = (uint8_t)(ca + 1 + rem);
    }
    __syncthreads();
    // A count that does not fit the P points read here, or a negative one (the blob stage's capacity error), fails the time step
    if (tid < C) {
        const int n = scnt[tid];
        if (n < 0) atomicMax(&s_err, 3);
        else if (n > P) atomicMax(&s_err, 2);
        else atomicMax(&s_pm, n);
    }
    for (int w = tid; w < C * 12; w += nth) { // P = K [R|t], the sums as DltAcc::add forms them
        const int c = w / 12, r = (w % 12) / 4, cc = w % 4;
        const double* K = cam + c * CAMW + oK; const double* R = cam + c * CAMW + oR; const double* tt = cam + c * CAMW + oT;
        double sum = 0;
        for (int k = 0; k < 3; k++) sum += K[3 * r + k] * (cc < 3 ? R[3 * k + cc] : tt[k]);
        cam[c * CAMW + oP + 4 * r + cc] = sum;
    }
    for (int c = tid; c < C; c += nth) { // K^-1 = adj(K) / det(K)
        const double* K = cam + c * CAMW + oK;
        double* Ki = cam + c * CAMW + oKi;
        const double c00 = K[4] * K[8] - K[5] * K[7], c01 = K[2] * K[7] - K[1] * K[8], c02 = K[1] * K[5] - K[2] * K[4];
        const double c10 = K[5] * K[6] - K[3] * K[8], c11 = K[0] * K[8] - K[2] * K[6], c12 = K[2] * K[3] - K[0] * K[5];
        const double c20 = K[3] * K[7] - K[4] * K[6], c21 = K[1] * K[6] - K[0] * K[7], c22 = K[0] * K[4] - K[1] * K[3];
        const double det = K[0] * c00 + K[1] * c10 + K[2] * c20;
        Ki[0] = c00 / det; Ki[1] = c01 / det; Ki[2] = c02 / det;
        Ki[3] = c10 / det; Ki[4] = c11 / det; Ki[5] = c12 / det;
        Ki[6] = c20 / det; Ki[7] = c21 / det; Ki[8] = c22 / det;
    }
    if (a.distorted)
        for (int w = tid; w < C * P; w += nth) // (geom_dev.h: cv.undistortPoints' five fixed-point rounds)
            undistort_pt(cam + (w / P) * CAMW + oK, cam + (w / P) * CAMW + oD, spts[2 * w], spts[2 * w + 1]);
    __syncthreads();
    if (s_err) {
        if (tid == 0) a.n[t] = s_err == 3 ? CORR_ERR_BLOB : CORR_ERR_TRUNCATED;
        return;
    }
    // ---- pair geometry: F_ab = K_b^-T [t]x R K_a^-1 with R = R_b R_a^T, t = t_b - R t_a, one pair per lane ------------------
    for (int w = tid; w < pairs; w += nth) {
        const double* ca = cam + pair_ab[2 * w] * CAMW; const double* cb = cam + pair_ab[2 * w + 1] * CAMW;
        double Rr[9], tr[3], E[9], M[9];
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 3; j++) {
                double s = 0;
#pragma unroll
                for (int k = 0; k < 3; k++) s += cb[oR + 3 * i + k] * ca[oR + 3 * j + k];
                Rr[3 * i + j] = s;
            }
#pragma unroll
        for (int i = 0; i < 3; i++) {
            double s = 0;
#pragma unroll
            for (int k = 0; k < 3; k++) s += Rr[3 * i + k] * ca[oT + k];
            tr[i] = cb[oT + i] - s;
        }
        const double tx[9] = {0., -tr[2], tr[1], tr[2], 0., -tr[0], -tr[1], tr[0], 0.};
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 3; j++) {
                double s = 0;
#pragma unroll
                for (int k = 0; k < 3; k++) s += tx[3 * i + k] * Rr[3 * k + j];
                E[3 * i + j] = s;
            }
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 3; j++) {
                double s = 0;
#pragma unroll
                for (int k = 0; k < 3; k++) s += cb[oKi + 3 * k + i] * E[3 * k + j];
                M[3 * i + j] = s;
            }
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 3; j++) {
                double s = 0;
#pragma unroll
                for (int k = 0; k < 3; k++) s += M[3 * i + k] * ca[oKi + 3 * k + j];
                Fm[9 * w + 3 * i + j] = s;
            }
    }
    __syncthreads();

    const int Pm = s_pm;
    unsigned char* const lds_recs = smem + L.hyp;
    unsigned char* const g_recs = a.scratch + (size_t)t * a.step_bytes;
    int nout = 0;
    for (int pass = 0; pass < a.max_passes; pass++) {
        if (tid == 0) { s_nseed = 0; s_acc = 0; }
        __syncthreads();
        // ---- seeds: one (pair, i, j) per lane ------------------------------------------------------------------------
        const int tot = pairs * Pm * Pm;
        for (int w = tid; w < tot; w += nth) {
            const int pr = w / (Pm * Pm), r = w - pr * Pm * Pm, i = r / Pm, j = r - i * Pm;
            const int ca = pair_ab[2 * pr], cb = pair_ab[2 * pr + 1];
            if (i >= scnt[ca] || j >= scnt[cb] || claimed[ca * P + i] || claimed[cb * P + j]) continue;
            const double* F = Fm + 9 * pr;
            const double x = spts[2 * (ca * P + i)], y = spts[2 * (ca * P + i) + 1];
            double la = F[0] * x + F[1] * y + F[2];
            double lb = F[3] * x + F[4] * y + F[5];
            double lc = F[6] * x + F[7] * y + F[8];
            const double nu = la * la + lb * lb;
            if (!(nu > 0.)) continue;
            const double sc = 1. / sqrt(nu);
            la *= sc; lb *= sc; lc *= sc;
            const double d = fabs(la * spts[2 * (cb * P + j)] + lb * spts[2 * (cb * P + j) + 1] + lc);
            if (d < a.cutoff) {
                const int s = atomicAdd(&s_nseed, 1);
                if (s < a.max_hyp) {
                    const Rec h{(s < L.cap ? lds_recs : g_recs) + (size_t)s * REC};
                    h.key() = (uint32_t)ca << 24 | (uint32_t)i << 16 | (uint32_t)cb << 8 | (uint32_t)j;
                }
            }
        }
        __syncthreads();
        const int n = s_nseed;
        if (n > a.max_hyp) {
            if (tid == 0) a.n[t] = CORR_ERR_GROUPS;
            return;
        }
        if (n == 0) break;
        const bool in_lds = n <= L.cap;
        if (!in_lds) { // the pass outgrew LDS: its first seeds follow the others into the scratch
            for (int s = tid; s < L.cap; s += nth) Rec{g_recs + (size_t)s * REC}.key() = Rec{lds_recs + (size_t)s * REC}.key();
            __syncthreads();
        }
        unsigned char* const recs = in_lds ? lds_recs : g_recs;
        uint16_t* const ord = in_lds ? (uint16_t*)(smem + L.ord) : (uint16_t*)(g_recs + (size_t)a.max_hyp * REC);
        // ---- hypotheses: one seed per lane ----------------------------------------------------------------------------
        for (int w = tid; w < n; w += nth) {
            const Rec h{recs + (size_t)w * REC};
            const uint32_t key = h.key();
            const int ca = key >> 24, i = (key >> 16) & 255, cb = (key >> 8) & 255, j = key & 255;
            int m = 0;
            bool keep = false;
            double err = 0.;
            DltAcc acc;
            acc.clear();
            acc.add_rows(cam + ca * CAMW + oP, spts[2 * (ca * P + i)], spts[2 * (ca * P + i) + 1]);
            acc.add_rows(cam + cb * CAMW + oP, spts[2 * (cb * P + j)], spts[2 * (cb * P + j) + 1]);
            double v[4];
            smallest_eigvec4(acc.B, v);
            double X2[3] = {v[0] / v[3], v[1] / v[3], v[2] / v[3]};
            if (v[3] != 0. && finite3(X2) && depth_of(cam + ca * CAMW, X2) > 0. && depth_of(cam + cb * CAMW, X2) > 0.) {
                for (int c = 0; c < C; c++) { // members: the seed pair plus, per other camera in front, its nearest free point within the gate
                    int id = NONE;
                    if (c == ca) id = i;
                    else if (c == cb) id = j;
                    else if (depth_of(cam + c * CAMW, X2) > 0.) {
                        double u, vv;
                        pinhole(cam + c * CAMW, X2, u, vv);
                        double best = a.gate2;
                        const int nc = scnt[c];
                        for (int p = 0; p < nc; p++) {
                            if (claimed[c * P + p]) continue;
                            const double du = spts[2 * (c * P + p)] - u, dv = spts[2 * (c * P + p) + 1] - vv;
                            const double d2 = du * du + dv * dv;
                            if (d2 < best) { best = d2; id = p; }
                        }
                    }
                    h.idx(c) = (uint8_t)id;
                    m += id != NONE;
                }
                double X[3];
                if (m >= a.min_views && solve_members(cam, spts, P, C, h, X)) {
                    double s = 0.;
                    for (int c = 0; c < C; c++) {
                        const int p = h.idx(c);
                        if (p == NONE) continue;
                        double u, vv;
                        pinhole(cam + c * CAMW, X, u, vv);
                        const double du = spts[2 * (c * P + p)] - u, dv = spts[2 * (c * P + p) + 1] - vv;
                        s += du * du; s += dv * dv;
                    }
                    err = s / (double)(2 * m);
                    keep = err < a.max_err;
                }
            }
            h.err() = keep ? err : 0.;
            h.members() = keep ? (uint8_t)m : 0;
            h.accepted() = 0;
        }
        // ---- sort ascending by (-members, err, a, i, b, j): bitonic network over the records' indices --------------------
        const int n2 = pow2_at_least(n);
        for (int k = tid; k < n2; k += nth) ord[k] = (uint16_t)(k < n ? k : ORD_END);
        __syncthreads();
        auto less = [&](int p, int q) { // a dropped hypothesis has 0 members and sorts behind every kept one; the padding behind all
            if (p == ORD_END || q == ORD_END) return p != ORD_END;
            const Rec hp{recs + (size_t)p * REC}, hq{recs + (size_t)q * REC};
            if (hp.members() != hq.members()) return hp.members() > hq.members();
            const double ep = hp.err(), eq = hq.err();
            if (ep != eq) return ep < eq;
            return hp.key() < hq.key();
        };
        for (int k = 2; k <= n2; k <<= 1)
            for (int j = k >> 1; j > 0; j >>= 1) {
                for (int x = tid; x < n2; x += nth) {
                    const int y = x ^ j;
                    if (y > x) {
                        const int p = ord[x], q = ord[y];
                        if ((x & k) == 0 ? less(q, p) : less(p, q)) { ord[x] = (uint16_t)q; ord[y] = (uint16_t)p; }
                    }
                }
                __syncthreads();
            }
        // ---- selection: one wave walks the sorted list, lane c owns the claims of camera c ----------------------------------
        if (tid < 64) {
            int q = nout, acc_n = 0;
            for (int k = 0; k < n; k++) {
                const int o = ord[k];
                if (o == ORD_END) break;
                const Rec h{recs + (size_t)o * REC};
                if (h.members() == 0) break;
                const int p = tid < C ? h.idx(tid) : NONE;
                if (__ballot(p != NONE && claimed[tid * P + p])) continue;
                if (q >= a.Q) { if (tid == 0) s_err = 4; break; }
                if (p != NONE) claimed[tid * P + p] = 1;
                if (tid == 0) { h.accepted() = 1; h.row() = (uint16_t)q; }
                q++; acc_n++;
            }
            if (tid == 0) { s_nout = q; s_acc = acc_n; }
        }
        __syncthreads();
        if (s_err) {
            if (tid == 0) a.n[t] = CORR_ERR_OUTPUT;
            return;
        }
        const int accepted = s_acc; // read before the next barrier: the next pass's first store to it comes behind that one
        nout = s_nout;
        // ---- the accepted markers of the pass leave, one per lane (X from the members again: the same operations, the same bits) ----
        for (int w = tid; w < n; w += nth) {
            const Rec h{recs + (size_t)w * REC};
            if (!h.accepted() || h.members() == 0) continue;
            double X[3];
            solve_members(cam, spts, P, C, h, X);
            const size_t ro = (size_t)t * a.Q + h.row();
            a.xyz[3 * ro] = X[0]; a.xyz[3 * ro + 1] = X[1]; a.xyz[3 * ro + 2] = X[2];
            a.err[ro] = h.err();
            uint32_t mask = 0;
            for (int c = 0; c < C; c++) {
                const int p = h.idx(c);
                a.idx[ro * C + c] = p == NONE ? -1 : p;
                if (p != NONE) mask |= 1u << c;
            }
            a.views[ro] = mask;
        }
        __syncthreads();
        if (accepted == 0) break;
    }
    if (tid == 0) a.n[t] = nout;
}

// Dynamic LDS a workgroup may use: 64 KiB without asking; the first call that needs more asks the runtime for gfx950's whole
// 160 KiB per workgroup and remembers the answer (as correspond_kernel does).
static int vis_lds_limit()
{
    static std::mutex mu;
    static int limit[64] = {0};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 64 * 1024 - 64;
    std::lock_guard<std::mutex> lk(mu);
    if (limit[dev] == 0) {
        const int want = 160 * 1024 - 64; // minus the kernel's static words
        const bool ok = hipFuncSetAttribute((const void*)correspond_visible_kernel<double>, hipFuncAttributeMaxDynamicSharedMemorySize, want) == hipSuccess &&
                        hipFuncSetAttribute((const void*)correspond_visible_kernel<int32_t>, hipFuncAttributeMaxDynamicSharedMemorySize, want) == hipSuccess;
        if (!ok) (void)hipGetLastError();
        limit[dev] = ok ? want : 64 * 1024 - 64;
    }
    return limit[dev];
}
// the budget the plan is made for: 64 KiB when that leaves room for 2048 hypotheses (several workgroups per CU stay possible), else the limit
static int vis_lds_budget(int P, int C)
{
    const int small = 64 * 1024 - 64;
    if (vis_lds_plan(P, C, small).cap >= 2048) return small;
    return vis_lds_limit();
}
size_t correspond_visible_smem_bytes(int P, int C)
{ // what the smallest acceptable plan takes (for the refusal's message), or the plan's size when it fits
    const VisLds L = vis_lds_plan(P, C, vis_lds_budget(P, C));
    if (L.cap >= VIS_MIN_CAP) return (size_t)L.total;
    return (size_t)L.hyp + (size_t)VIS_MIN_CAP * (vis_rec_bytes(C) + 2);
}
bool correspond_visible_fits(int P, int C) { return vis_lds_plan(P, C, vis_lds_budget(P, C)).cap >= VIS_MIN_CAP; }
size_t correspond_visible_step_bytes(int C, int max_hyp)
{
    return ((size_t)max_hyp * vis_rec_bytes(C) + (size_t)pow2_at_least(max_hyp) * 2 + 15) & ~(size_t)15;
}

void launch_correspond_visible(const VisArgs& a_, hipStream_t s)
{
    VisArgs a = a_;
    a.lds_budget = vis_lds_budget(a.P, a.C);
    const size_t sm = (size_t)vis_lds_plan(a.P, a.C, a.lds_budget).total;
    if (a.pts_f64)
        hipLaunchKernelGGL(correspond_visible_kernel<double>, dim3(a.T), dim3(256), sm, s, a);
    else
        hipLaunchKernelGGL(correspond_visible_kernel<int32_t>, dim3(a.T), dim3(256), sm, s, a);
}

} // namespace mocap
