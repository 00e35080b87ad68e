// rigid.hip -- rigid-body poses per time step: each of B bodies (3 to 8 model points) is searched among a step's unlabelled 3-D
// detections by distance-matched triples, posed by Horn's closed-form quaternion, labelled, refitted once and scored (FP64).
//
// The reference has no counterpart (the four orientation slots of its {"tracker1": [0, 0, 0, 0, x, y, z]} message are never
// filled by anything optical): the contract is the definition of DESIGN.md section 2, restated by tests/rigid_ref.py.  The library
// is built with -ffp-contract=off: every sum and product below is a separately rounded FP64 operation, in the order the definition
// gives, so the device and the restatement agree bit for bit.
//
// Work decomposition: every (time step, body) is independent, so the grid is T x B workgroups of 256 threads.  A workgroup keeps in
// LDS the step's detections with their 64 x 64 distance table (32 KB), the body's model with its table and triples, and the
// candidate list (32-bit entries: 6 bits each for h, i, j, k).  Phases: (a) load and build the tables; (b) lanes stride over
// (h, i, j), test the first distance and scan k, appending matches through an LDS integer counter -- the list's order is whatever
// the lanes made it, and nothing below depends on it; (c) lanes stride over the candidates and solve, label, refit and score each,
// keeping their best key; (d) a tree reduction of the key (more inliers, smaller rms^2, smaller (h, i, j, k)) -- a total order, so
// the winner is the same whatever the list's order; (e) lane 0 solves the winner once more (the same operations, the same bits:
// nothing but a key travels through the reduction) and writes it.  No floating-point atomics: the same call gives the same bits.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "kernels.h"
#include "geom_dev.h"
#include "rigid_dev.h"

namespace mocap {

namespace {

constexpr int THREADS = 256;
constexpr int DS = RIGID_MAX_DET;        // row stride of the detections' distance table
static_assert(RIGID_MAX_DET <= 64 && RIGID_MAX_TRIPLES <= 64, "a candidate packs h, i, j, k into 6 bits each");
static_assert(RIGID_MAX_MARKERS == 8, "the labels of a body are the eight bytes of one 64-bit word");

struct Fit { Pose pose; unsigned long long lab; int n_in; double rms2; };

// steps 4 to 6 for one candidate: pose from its three pairs, labels, one refit, rms^2.  n_in < min_markers: no refit, no result.
__device__ __forceinline__ void evaluate(unsigned e, const int* tri, const double* model, const double* det, int M, int n, double g2,
                                         int min_markers, Fit& f)
{
    const int h = e >> 18, i = (e >> 12) & 63, j = (e >> 6) & 63, k = e & 63;
    unsigned long long seed = ~0ull;
    seed = with_label(seed, tri[3 * h], (unsigned)i);
    seed = with_label(seed, tri[3 * h + 1], (unsigned)j);
    seed = with_label(seed, tri[3 * h + 2], (unsigned)k);
    horn(model, det, seed, f.pose);
    unsigned long long claimed = 0ull, lab = ~0ull;
    int n_in = 0;
#pragma unroll
    for (int p = 0; p < RIGID_MAX_MARKERS; p++) {
        if (p >= M) continue;
        double pr[3];
        transform(f.pose, model + 3 * p, pr);
        int best = -1;
        double bd = 0.;
        for (int l = 0; l < n; l++) { // the nearest unclaimed detection below gate^2; ties go to the lower row
            const double e0 = det[3 * l] - pr[0], e1 = det[3 * l + 1] - pr[1], e2 = det[3 * l + 2] - pr[2];
            const double d2 = (e0 * e0 + e1 * e1) + e2 * e2;
            if (!(claimed >> l & 1ull) && d2 < g2 && (best < 0 || d2 < bd)) { bd = d2; best = l; }
        }
        if (best >= 0) { claimed |= 1ull << best; lab = with_label(lab, p, (unsigned)best); n_in++; }
    }
    f.lab = lab; f.n_in = n_in; f.rms2 = 0.;
    if (n_in < min_markers) return;
    horn(model, det, lab, f.pose);
    double ssq = 0.;
#pragma unroll
    for (int p = 0; p < RIGID_MAX_MARKERS; p++) {
        const unsigned l = label_of(lab, p);
        if (l == NO_LABEL) continue;
        double pr[3];
        transform(f.pose, model + 3 * p, pr);
        const double e0 = det[3 * l] - pr[0], e1 = det[3 * l + 1] - pr[1], e2 = det[3 * l + 2] - pr[2];
        ssq += (e0 * e0 + e1 * e1) + e2 * e2;
    }
    f.rms2 = ssq / (double)n_in;
}

// the total order of step 7: more inliers, smaller rms^2, smaller (h, i, j, k); n < 0 = no result, which nothing is worse than
__device__ __forceinline__ bool better(int an, double ar, unsigned ap, int bn, double br, unsigned bp)
{
    return an > bn || (an == bn && (ar < br || (ar == br && ap < bp)));
}

// the workgroup's LDS: the step's detections with their distance table, the body's model with its table and triples, the candidates
struct RigidShared {
    double *dd, *det, *model, *dm; // dd [RIGID_MAX_DET][DS], det [RIGID_MAX_DET][3], model [RIGID_MAX_MARKERS][3], dm [8][8]
    int* tri;
    unsigned* cand;                // h << 18 | i << 12 | j << 6 | k, in no particular order
    double* kr;                    // the reduction's keys: rms^2, inliers, candidate
    int* kn;
    unsigned* kp;
    int *count, *bad;
};

// one (time step, body): what every lane knows of it
struct RigidItem { int tid, t, b, n, M, H, cap; size_t o; };

// (a) inputs and tables.  -> 0 or RIGID_ERR_MODEL, the same in every lane
__device__ __forceinline__ int load_tables(const RigidArgs& a, const RigidItem& it, const RigidShared& sh)
{
    const int tid = it.tid, n = it.n, M = it.M, H = it.H;
    if (tid == 0) { *sh.count = 0; *sh.bad = 0; }
    for (int x = tid; x < 3 * H; x += THREADS) sh.tri[x] = a.tri[(size_t)it.b * RIGID_MAX_TRIPLES * 3 + x];
    if (tid < 3 * M) sh.model[tid] = a.model[(size_t)it.b * RIGID_MAX_MARKERS * 3 + tid];
    for (int x = tid; x < 3 * n; x += THREADS) sh.det[x] = a.xyz[(size_t)it.t * a.Q * 3 + x];
    __syncthreads();
    if (tid < H) {
        const int ta = sh.tri[3 * tid], tb = sh.tri[3 * tid + 1], tc = sh.tri[3 * tid + 2];
        if (!(0 <= ta && ta < tb && tb < tc && tc < M)) *sh.bad = 1;
    }
    for (int x = tid; x < n * n; x += THREADS) {
        const int i = x / n, j = x - i * n;
        sh.dd[i * DS + j] = dist3(sh.det + 3 * i, sh.det + 3 * j);
    }
    if (tid < RIGID_MAX_MARKERS * RIGID_MAX_MARKERS) {
        const int i = tid >> 3, j = tid & 7;
        sh.dm[tid] = i < M && j < M ? dist3(sh.model + 3 * i, sh.model + 3 * j) : 0.;
    }
    __syncthreads();
    return *sh.bad ? RIGID_ERR_MODEL : 0;
}

// (b) candidates: |d_ij - L_ab|, |d_jk - L_bc|, |d_ik - L_ac| all below tol, i, j, k distinct.  -> the list's length (beyond
// it.cap: the list is short of that many)
__device__ __forceinline__ int list_candidates(const RigidArgs& a, const RigidItem& it, const RigidShared& sh)
{
    const int n = it.n, nn = n * n, items = it.H * nn;
    for (int x = it.tid; x < items; x += THREADS) {
        const int h = x / nn, r = x - h * nn, i = r / n, j = r - i * n;
        if (i == j) continue;
        const int ta = sh.tri[3 * h], tb = sh.tri[3 * h + 1], tc = sh.tri[3 * h + 2];
        if (!(fabs(sh.dd[i * DS + j] - sh.dm[ta * 8 + tb]) < a.tol)) continue;
        const double Lbc = sh.dm[tb * 8 + tc], Lac = sh.dm[ta * 8 + tc];
        for (int k = 0; k < n; k++) {
            if (k == i || k == j) continue;
            if (fabs(sh.dd[j * DS + k] - Lbc) < a.tol && fabs(sh.dd[i * DS + k] - Lac) < a.tol) {
                const int pos = atomicAdd(sh.count, 1);
                if (pos < it.cap) sh.cand[pos] = (unsigned)h << 18 | (unsigned)i << 12 | (unsigned)j << 6 | (unsigned)k;
            }
        }
    }
    __syncthreads();
    return *sh.count;
}

struct Key { int n; double r; unsigned p; }; // inliers (-1: no result yet), rms^2, candidate

// (e) the winner's fit leaves
__device__ __forceinline__ void write_pose(const RigidArgs& a, size_t o, const Fit& f)
{
#pragma unroll
    for (int k = 0; k < 9; k++) a.R[o * 9 + k] = f.pose.R[k];
#pragma unroll
    for (int k = 0; k < 3; k++) a.t[o * 3 + k] = f.pose.t[k];
#pragma unroll
    for (int k = 0; k < 4; k++) a.q[o * 4 + k] = f.pose.q[k];
    a.rms[o] = sqrt(f.rms2);
    a.n_in[o] = f.n_in;
#pragma unroll
    for (int p = 0; p < RIGID_MAX_MARKERS; p++) {
        const unsigned l = label_of(f.lab, p);
        a.label[o * RIGID_MAX_MARKERS + p] = l == NO_LABEL ? -1 : (int)l;
    }
    a.status[o] = 0;
}

// THE ONE CALL SITE OF `evaluate`, which is half the kernel inline (a second site: 6 042 -> 13 005 instructions), so it serves
// both of its uses.  search: (c) the lanes stride over the list, each keeping the best key of its candidates.  !search: (e) lane
// 0 solves `winner` once more (the same operations, the same bits: nothing but a key travels through the reduction) and writes it.
__device__ __forceinline__ void evaluate_candidates(const RigidArgs& a, const RigidItem& it, const RigidShared& sh, bool search, int count,
                                                    unsigned winner, Key& best)
{
    const double g2 = a.gate * a.gate;
    const int lo = search ? it.tid : (it.tid == 0 ? 0 : 1), hi = search ? count : 1;
    for (int x = lo; x < hi; x += THREADS) {
        const unsigned e = search ? sh.cand[x] : winner;
        Fit f;
        evaluate(e, sh.tri, sh.model, sh.det, it.M, it.n, g2, a.min_markers, f);
        if (!search) write_pose(a, it.o, f);
        else if (f.n_in >= a.min_markers && better(f.n_in, f.rms2, e, best.n, best.r, best.p)) { best.n = f.n_in; best.r = f.rms2; best.p = e; }
    }
}

// (d) the smallest key of the workgroup.  -> false: no lane has a result
__device__ __forceinline__ bool workgroup_best(const RigidItem& it, const RigidShared& sh, const Key& mine, unsigned& winner)
{
    const int tid = it.tid;
    sh.kn[tid] = mine.n; sh.kr[tid] = mine.r; sh.kp[tid] = mine.p;
    __syncthreads();
    for (int s = THREADS / 2; s > 0; s >>= 1) {
        if (tid < s && better(sh.kn[tid + s], sh.kr[tid + s], sh.kp[tid + s], sh.kn[tid], sh.kr[tid], sh.kp[tid])) {
            sh.kn[tid] = sh.kn[tid + s]; sh.kr[tid] = sh.kr[tid + s]; sh.kp[tid] = sh.kp[tid + s];
        }
        __syncthreads();
    }
    winner = sh.kp[0];
    return sh.kn[0] >= 0;
}

// (c) to (e): the search, the reduction, the winner solved again and written.  -> false: lost, nothing written
__device__ __forceinline__ bool pose_of_the_best_candidate(const RigidArgs& a, const RigidItem& it, const RigidShared& sh, int count)
{
    Key best{-1, 0., 0xffffffffu};
    unsigned winner = 0u;
    for (int pass = 0; pass < 2; pass++) { // (a loop for the sake of evaluate_candidates' one call site)
        evaluate_candidates(a, it, sh, pass == 0, count, winner, best);
        if (pass == 0 && !workgroup_best(it, sh, best, winner)) return false;
    }
    return true;
}

// no result: the status says why, no inliers, no labels; the floats stay as they were
__device__ __forceinline__ void write_no_result(const RigidArgs& a, const RigidItem& it, int code)
{
    if (it.tid == 0) { a.status[it.o] = code; a.n_in[it.o] = 0; }
    if (it.tid < RIGID_MAX_MARKERS) a.label[it.o * RIGID_MAX_MARKERS + it.tid] = -1;
}

} // namespace

__global__ __launch_bounds__(THREADS) void rigid_poses_kernel(RigidArgs a)
{
    __shared__ double s_dd[RIGID_MAX_DET * DS];
    __shared__ double s_det[RIGID_MAX_DET * 3];
    __shared__ double s_model[RIGID_MAX_MARKERS * 3];
    __shared__ double s_dm[RIGID_MAX_MARKERS * RIGID_MAX_MARKERS];
    __shared__ int s_tri[RIGID_MAX_TRIPLES * 3];
    __shared__ unsigned s_cand[RIGID_MAX_HYP];
    __shared__ double s_kr[THREADS];
    __shared__ int s_kn[THREADS];
    __shared__ unsigned s_kp[THREADS];
    __shared__ int s_count, s_bad;
    const RigidShared sh{s_dd, s_det, s_model, s_dm, s_tri, s_cand, s_kr, s_kn, s_kp, &s_count, &s_bad};

    RigidItem it;
    it.tid = threadIdx.x;
    it.t = blockIdx.x / a.B; it.b = blockIdx.x - it.t * a.B;
    it.o = (size_t)it.t * a.B + it.b;
    it.n = a.n[it.t]; it.M = a.n_markers[it.b]; it.H = a.n_tri[it.b];
    it.cap = a.max_hyp < RIGID_MAX_HYP ? a.max_hyp : RIGID_MAX_HYP;
    const int rows = a.Q < RIGID_MAX_DET ? a.Q : RIGID_MAX_DET;

    // every exit below is taken by the whole workgroup: `code` is formed from values all lanes share
    int code = 0;
    if (it.n < 0) code = RIGID_ERR_BLIND;
    else if (it.n > rows) code = RIGID_ERR_CAPACITY;
    else if (it.M < 3 || it.M > RIGID_MAX_MARKERS || it.H < 1 || it.H > RIGID_MAX_TRIPLES) code = RIGID_ERR_MODEL;

    if (code == 0) code = load_tables(a, it, sh);
    int count = 0;
    if (code == 0) {
        count = list_candidates(a, it, sh);
        if (count > it.cap) code = RIGID_ERR_HYP; // never a shortened list
    }
    if (code == 0) {
        if (pose_of_the_best_candidate(a, it, sh, count)) return;
        code = RIGID_LOST;
    }
    write_no_result(a, it, code);
}

void launch_rigid_poses(const RigidArgs& a, hipStream_t s)
{
    hipLaunchKernelGGL(rigid_poses_kernel, dim3((unsigned)(a.T * a.B)), dim3(THREADS), 0, s, a);
}

} // namespace mocap
