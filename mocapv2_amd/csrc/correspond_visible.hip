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
#include "kernels.h"
#include "geom_dev.h"
#include "correspond_dev.h"

namespace mocap {

namespace {

// per camera in LDS, in doubles: the row both correspondence kernels keep (correspond_dev.h), then K^-1 (9)
constexpr int oKi = CAM_ROW, CAMW = CAM_ROW + 9;
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

// the LDS pointers of one workgroup, from the plan, and where the time step's records lie in the context's scratch
struct VisShared {
    double *cam, *Fm, *spts; // [C][CAMW], [pairs][9], [C][P][2]
    int* scnt;               // [32], 0 behind camera C - 1
    uint8_t *pair_ab, *claimed; // [pairs][2] = (ca, cb); [C][P] 1 = the point belongs to an accepted marker
    unsigned char *lds_recs, *g_recs;
    uint16_t* lds_ord;
    int cap, pairs, rec;     // records LDS holds, camera pairs, bytes per record
};
__device__ __forceinline__ VisShared vis_shared(unsigned char* smem, const VisArgs& a, int t)
{
    const VisLds L = vis_lds_plan(a.P, a.C, a.lds_budget);
    VisShared S;
    S.cam = (double*)(smem + L.cam);
    S.Fm = (double*)(smem + L.F);
    S.spts = (double*)(smem + L.pts);
    S.scnt = (int*)(smem + L.cnt);
    S.pair_ab = smem + L.pair;
    S.claimed = smem + L.claimed;
    S.lds_recs = smem + L.hyp;
    S.g_recs = a.scratch + (size_t)t * a.step_bytes;
    S.lds_ord = (uint16_t*)(smem + L.ord);
    S.cap = L.cap;
    S.pairs = a.C * (a.C - 1) / 2;
    S.rec = vis_rec_bytes(a.C);
    return S;
}

// K^-1 = adj(K) / det(K)
__device__ __forceinline__ void invert3(const double* K, double* Ki)
{
    const double c00 = K[4] * K[8] - K[5] * K[7], c01 = K[2] * K[7] - K[1] * K[8], c02 = K[1] * K[5] - K[2] * K[4];
    const double c10 = K[5] * K[6] - K[3] * K[8], c11 = K[0] * K[8] - K[2] * K[6], c12 = K[2] * K[3] - K[0] * K[5];
    const double c20 = K[3] * K[7] - K[4] * K[6], c21 = K[1] * K[6] - K[0] * K[7], c22 = K[0] * K[4] - K[1] * K[3];
    const double det = K[0] * c00 + K[1] * c10 + K[2] * c20;
    Ki[0] = c00 / det; Ki[1] = c01 / det; Ki[2] = c02 / det;
    Ki[3] = c10 / det; Ki[4] = c11 / det; Ki[5] = c12 / det;
    Ki[6] = c20 / det; Ki[7] = c21 / det; Ki[8] = c22 / det;
}

// out = op(A) op(B) for row-major 3x3, op = transpose where TA / TB says so; every sum runs k = 0, 1, 2 from 0
template <bool TA, bool TB>
__device__ __forceinline__ void mat3(const double* A, const double* B, double* out)
{
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) {
            double s = 0;
#pragma unroll
            for (int k = 0; k < 3; k++) s += A[TA ? 3 * k + i : 3 * i + k] * B[TB ? 3 * j + k : 3 * k + j];
            out[3 * i + j] = s;
        }
}

// ---- the one round of loads: counts, points (every slot up to P), cameras; then P = K [R|t], K^-1, the undistorted points and
// the count check.  Leaves *s_err at 0, 2 or 3 (checked_count) and *s_pm at the largest count behind a barrier.
template <typename PT>
__device__ __forceinline__ void load_step(const VisArgs& a, const VisShared& S, int t, int* s_err, int* s_nout, int* s_pm)
{
    const int C = a.C, P = a.P, tid = threadIdx.x, nth = blockDim.x;
    if (tid == 0) { *s_err = 0; *s_nout = 0; *s_pm = 0; }
    if (tid < 32) S.scnt[tid] = tid < C ? a.counts[(size_t)t * a.cnt_st + (size_t)tid * a.cnt_sc] : 0;
    stage_step_points<PT>(S.spts, a, t, tid, nth);
    for (int w = tid; w < C * P; w += nth) S.claimed[w] = 0;
    stage_camera_rows<CAMW>(S.cam, a.cams, C, tid, nth);
    for (int w = tid; w < S.pairs; w += nth) { // pair w = (ca, cb), ca < cb, in the order (0,1), (0,2), ..., (C-2,C-1)
        int ca = 0, rem = w;
        while (rem >= C - 1 - ca) { rem -= C - 1 - ca; ca++; }
        S.pair_ab[2 * w] = (uint8_t)ca; S.pair_ab[2 * w + 1] = (uint8_t)(ca + 1 + rem);
    }
    __syncthreads();
    // (a negative count leaves the maximum alone; one above P fails the time step before the maximum is looked at)
    if (tid < C) atomicMax(s_pm, checked_count(S.scnt, tid, P, s_err));
    form_projections<CAMW>(S.cam, C, tid, nth);
    for (int c = tid; c < C; c += nth) invert3(S.cam + c * CAMW + oK, S.cam + c * CAMW + oKi);
    if (a.distorted)
        for (int w = tid; w < C * P; w += nth) // (geom_dev.h: cv.undistortPoints' five fixed-point rounds)
            undistort_pt(S.cam + (w / P) * CAMW + oK, S.cam + (w / P) * CAMW + oD, S.spts[2 * w], S.spts[2 * w + 1]);
    __syncthreads();
}

// ---- pair geometry: F_ab = K_b^-T [t]x R K_a^-1 with R = R_b R_a^T, t = t_b - R t_a, one pair per lane ------------------
__device__ __forceinline__ void pair_geometry(const VisShared& S)
{
    for (int w = threadIdx.x; w < S.pairs; w += blockDim.x) {
        const double* ca = S.cam + S.pair_ab[2 * w] * CAMW; const double* cb = S.cam + S.pair_ab[2 * w + 1] * CAMW;
        double Rr[9], tr[3], E[9], M[9];
        mat3<false, true>(cb + oR, ca + oR, Rr);
#pragma unroll
        for (int i = 0; i < 3; i++) {
            double s = 0;
#pragma unroll
            for (int k = 0; k < 3; k++) s += Rr[3 * i + k] * ca[oT + k];
            tr[i] = cb[oT + i] - s;
        }
        const double tx[9] = {0., -tr[2], tr[1], tr[2], 0., -tr[0], -tr[1], tr[0], 0.};
        mat3<false, false>(tx, Rr, E);
        mat3<true, false>(cb + oKi, E, M);
        mat3<false, false>(M, ca + oKi, S.Fm + 9 * w);
    }
}

// ---- seeds: one (pair, i, j) per lane; a pair of free points within the cutoff of each other's epipolar line takes a record
// (the first S.cap in LDS, the others in the scratch) and leaves its key there.  *s_nseed counts them, stored or not.
__device__ __forceinline__ void find_seeds(const VisArgs& a, const VisShared& S, int Pm, int* s_nseed)
{
    const int P = a.P, tot = S.pairs * Pm * Pm;
    for (int w = threadIdx.x; w < tot; w += blockDim.x) {
        const int pr = w / (Pm * Pm), r = w - pr * Pm * Pm, i = r / Pm, j = r - i * Pm;
        const int ca = S.pair_ab[2 * pr], cb = S.pair_ab[2 * pr + 1];
        if (i >= S.scnt[ca] || j >= S.scnt[cb] || S.claimed[ca * P + i] || S.claimed[cb * P + j]) continue;
        double la, lb, lc;
        if (!epiline_f64(S.Fm + 9 * pr, S.spts[2 * (ca * P + i)], S.spts[2 * (ca * P + i) + 1], la, lb, lc)) continue;
        const double d = fabs(la * S.spts[2 * (cb * P + j)] + lb * S.spts[2 * (cb * P + j) + 1] + lc);
        if (d < a.cutoff) {
            const int s = atomicAdd(s_nseed, 1);
            if (s < a.max_hyp) {
                const Rec h{(s < S.cap ? S.lds_recs : S.g_recs) + (size_t)s * S.rec};
                h.key() = (uint32_t)ca << 24 | (uint32_t)i << 16 | (uint32_t)cb << 8 | (uint32_t)j;
            }
        }
    }
}

// the pass outgrew LDS: its first seeds follow the others into the scratch.  Ends in a barrier.
__device__ __forceinline__ void seeds_to_scratch(const VisShared& S)
{
    for (int s = threadIdx.x; s < S.cap; s += blockDim.x) Rec{S.g_recs + (size_t)s * S.rec}.key() = Rec{S.lds_recs + (size_t)s * S.rec}.key();
    __syncthreads();
}

// camera c's free point nearest (u, v) within the gate, or NONE
__device__ __forceinline__ int nearest_free_point(const VisShared& S, int P, int c, double u, double v, double gate2)
{
    int id = NONE;
    double best = gate2;
    const int nc = S.scnt[c];
    for (int p = 0; p < nc; p++) {
        if (S.claimed[c * P + p]) continue;
        const double du = S.spts[2 * (c * P + p)] - u, dv = S.spts[2 * (c * P + p) + 1] - v;
        const double d2 = du * du + dv * dv;
        if (d2 < best) { best = d2; id = p; }
    }
    return id;
}

// mean squared pinhole reprojection error of X over the m members of h, the sum in camera order
__device__ __forceinline__ double member_error(const VisShared& S, int P, int C, const Rec h, const double X[3], int m)
{
    double s = 0.;
    for (int c = 0; c < C; c++) {
        const int p = h.idx(c);
        if (p == NONE) continue;
        double u, v;
        pinhole(S.cam + c * CAMW, X, u, v);
        const double du = S.spts[2 * (c * P + p)] - u, dv = S.spts[2 * (c * P + p) + 1] - v;
        s += du * du; s += dv * dv;
    }
    return s / (double)(2 * m);
}

// ---- hypotheses: one seed per lane.  The two-view point of the seed pair collects, per other camera in front of which it
// lies, that camera's nearest free point within the gate; with min_views members or more, X over all members and its error.
__device__ __forceinline__ void build_hypotheses(const VisArgs& a, const VisShared& S, unsigned char* recs, int n)
{
    const int C = a.C, P = a.P;
    for (int w = threadIdx.x; w < n; w += blockDim.x) {
        const Rec h{recs + (size_t)w * S.rec};
        const uint32_t key = h.key();
        const int ca = key >> 24, i = (key >> 16) & 255, cb = (key >> 8) & 255, j = key & 255;
        int m = 0;
        bool keep = false;
        double err = 0.;
        DltAcc acc;
        acc.clear();
        acc.add_rows(S.cam + ca * CAMW + oP, S.spts[2 * (ca * P + i)], S.spts[2 * (ca * P + i) + 1]);
        acc.add_rows(S.cam + cb * CAMW + oP, S.spts[2 * (cb * P + j)], S.spts[2 * (cb * P + j) + 1]);
        double v[4];
        smallest_eigvec4(acc.B, v);
        double X2[3] = {v[0] / v[3], v[1] / v[3], v[2] / v[3]};
        if (v[3] != 0. && finite3(X2) && depth_of(S.cam + ca * CAMW, X2) > 0. && depth_of(S.cam + cb * CAMW, X2) > 0.) {
            for (int c = 0; c < C; c++) {
                int id = NONE;
                if (c == ca) id = i;
                else if (c == cb) id = j;
                else if (depth_of(S.cam + c * CAMW, X2) > 0.) {
                    double u, vv;
                    pinhole(S.cam + c * CAMW, X2, u, vv);
                    id = nearest_free_point(S, P, c, u, vv, a.gate2);
                }
                h.idx(c) = (uint8_t)id;
                m += id != NONE;
            }
            double X[3];
            if (m >= a.min_views && solve_members(S.cam, S.spts, P, C, h, X)) {
                err = member_error(S, P, C, h, X, m);
                keep = err < a.max_err;
            }
        }
        h.err() = keep ? err : 0.;
        h.members() = keep ? (uint8_t)m : 0;
        h.accepted() = 0;
    }
}

// ---- sort ascending by (-members, err, a, i, b, j): bitonic network over the records' indices.  A dropped hypothesis has 0
// members and sorts behind every kept one, the padding up to a power of two behind all.  Ends in a barrier.
__device__ __forceinline__ void sort_hypotheses(const VisShared& S, unsigned char* recs, uint16_t* ord, int n)
{
    const int tid = threadIdx.x, nth = blockDim.x, REC = S.rec;
    const int n2 = pow2_at_least(n);
    for (int k = tid; k < n2; k += nth) ord[k] = (uint16_t)(k < n ? k : ORD_END);
    __syncthreads();
    auto less = [&](int p, int q) {
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
}

// ---- selection: the first wave walks the sorted list, lane c owns the claims of camera c.  A hypothesis none of whose points is
// claimed is accepted, takes output row nout, nout + 1, ... and claims its points; *s_err = 4 when the rows run out.
__device__ __forceinline__ void select_by_one_wave(const VisArgs& a, const VisShared& S, unsigned char* recs, const uint16_t* ord, int n, int nout,
                                                   int* s_err, int* s_nout, int* s_acc)
{
    const int tid = threadIdx.x, C = a.C, P = a.P;
    int q = nout, acc_n = 0;
    for (int k = 0; k < n; k++) {
        const int o = ord[k];
        if (o == ORD_END) break;
        const Rec h{recs + (size_t)o * S.rec};
        if (h.members() == 0) break;
        const int p = tid < C ? h.idx(tid) : NONE;
        if (__ballot(p != NONE && S.claimed[tid * P + p])) continue;
        if (q >= a.Q) { if (tid == 0) *s_err = 4; break; }
        if (p != NONE) S.claimed[tid * P + p] = 1;
        if (tid == 0) { h.accepted() = 1; h.row() = (uint16_t)q; }
        q++; acc_n++;
    }
    if (tid == 0) { *s_nout = q; *s_acc = acc_n; }
}

// ---- the accepted markers of the pass leave, one per lane (X from the members again: the same operations, the same bits) ----
__device__ __forceinline__ void emit_accepted(const VisArgs& a, const VisShared& S, int t, unsigned char* recs, int n)
{
    const int C = a.C;
    for (int w = threadIdx.x; w < n; w += blockDim.x) {
        const Rec h{recs + (size_t)w * S.rec};
        if (!h.accepted() || h.members() == 0) continue;
        double X[3];
        solve_members(S.cam, S.spts, a.P, C, h, X);
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
}

} // namespace

// One workgroup per time step: the loads, the pair matrices, then passes of seeds -> hypotheses -> order -> selection -> output
// until a pass accepts nothing.  s_err: 2 = more than P points, 3 = negative count, 4 = output rows.
template <typename PT>
__global__ __launch_bounds__(256) void correspond_visible_kernel(VisArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ int s_err, s_nseed, s_nout, s_acc, s_pm;
    const int t = blockIdx.x, tid = threadIdx.x;
    const VisShared S = vis_shared(smem, a, t);

    load_step<PT>(a, S, t, &s_err, &s_nout, &s_pm);
    if (s_err) {
        if (tid == 0) a.n[t] = count_error_code(s_err);
        return;
    }
    pair_geometry(S);
    __syncthreads();
    const int Pm = s_pm;
    int nout = 0;
    for (int pass = 0; pass < a.max_passes; pass++) {
        if (tid == 0) { s_nseed = 0; s_acc = 0; }
        __syncthreads();
        find_seeds(a, S, Pm, &s_nseed);
        __syncthreads();
        const int n = s_nseed;
        if (n > a.max_hyp) {
            if (tid == 0) a.n[t] = CORR_ERR_GROUPS;
            return;
        }
        if (n == 0) break;
        const bool in_lds = n <= S.cap;
        if (!in_lds) seeds_to_scratch(S);
        unsigned char* const recs = in_lds ? S.lds_recs : S.g_recs;
        uint16_t* const ord = in_lds ? S.lds_ord : (uint16_t*)(S.g_recs + (size_t)a.max_hyp * S.rec);
        build_hypotheses(a, S, recs, n);
        sort_hypotheses(S, recs, ord, n);
        if (tid < 64) select_by_one_wave(a, S, recs, ord, n, nout, &s_err, &s_nout, &s_acc);
        __syncthreads();
        if (s_err) {
            if (tid == 0) a.n[t] = CORR_ERR_OUTPUT;
            return;
        }
        const int accepted = s_acc; // read before the next barrier: the next pass's first store to it comes behind that one
        nout = s_nout;
        emit_accepted(a, S, t, recs, n);
        __syncthreads();
        if (accepted == 0) break;
    }
    if (tid == 0) a.n[t] = nout;
}

// the budget the plan is made for: 64 KiB when that leaves room for 2048 hypotheses (several workgroups per CU stay possible), else the limit
static int vis_lds_budget(int P, int C)
{
    const int small = 64 * 1024 - 64;
    if (vis_lds_plan(P, C, small).cap >= 2048) return small;
    return workgroup_lds_limit(LDS_USER_VISIBLE, (const void*)correspond_visible_kernel<double>, (const void*)correspond_visible_kernel<int32_t>);
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
