// track.hip -- marker identities across time steps: a constant-velocity prediction per track, gated nearest-neighbour
// assignment in the total order (d2, slot, detection), births and deaths (FP64).
//
// The reference has no counterpart (its {"tracker1": object_points[0]} message assumes one marker): the contract is the definition of
// DESIGN.md section 2, restated by tests/track_ref.py.  The library is built with -ffp-contract=off: every sum and product below is a
// separately rounded FP64 operation, in the order the definition gives, so the device and the restatement agree bit for bit.
//
// Work decomposition: the recursion over the time steps is inherent (a prediction needs the step before), so ONE workgroup walks
// the T steps, one lane per slot (one wave per 64 slots, two waves at least), the slot table in registers.  A step touches LDS and
// registers only: the detections live in two chunk buffers in LDS, and while step k of one chunk is worked on, the rows of step k of
// the next chunk are in flight (in registers); they land behind the step, so NO GLOBAL LOAD SITS ON THE STEP-TO-STEP CHAIN
// (prefetch_next_chunk_step, land_prefetch and the two s_waitcnt that say so).  The counts run one chunk further ahead: they tell
// the staging which rows to load, and rows at and beyond a step's count are never read.  No atomics at all, so the same call gives
// the same bits.  Outputs leave as plain stores nothing waits on.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "kernels.h"

namespace mocap {

namespace {

constexpr int CHUNK_DET = 768;              // detections of one chunk buffer, four doubles each: x, y, z, taken (0 / 1)
constexpr int CHUNK_STEPS = 64;             // time steps of a chunk at most (one lane stages one count)
constexpr int MIN_THREADS = 128;            // two waves at least: the slots' lanes and the detections' lanes are different waves
constexpr int PFS = 6;                      // doubles of ONE time step a lane stages at most (two waves: 768 / 128)
static_assert(TRACK_MAX * 3 <= PFS * MIN_THREADS && TRACK_MAX <= CHUNK_DET, "two waves must be able to stage a whole time step");

// the workgroup's LDS
struct TrackShared {
    double (*det)[CHUNK_DET * 4];   // [2] the detections of two chunks: the one walked, the one arriving
    int (*n)[CHUNK_STEPS];          // [3] the counts run one chunk ahead of the detections
    double (*pred)[4];              // per slot: prediction, then gate^2 (-1: the slot is dead or taken, nothing lies below it)
    int* col;                       // per detection: its column's best slot of this round, -1 = none
    int* birth;                     // the k-th unmatched detection
    unsigned long long* live;       // [4] the live slots, 64 per word
    int* more;                      // [2] a round's "some slot still wants a detection", by the round's parity
};

// what a lane is: its slot (tid), its wave, the detections it serves as a column
struct TrackLane {
    int tid, nth, lane, wave, nw;
    int det_lane;                   // detection j's lane sits half a workgroup away from slot j's: with few of both, rows and columns
                                    //   are scanned by different waves at the same time
    unsigned long long below;       // the lanes of the wave below this one
    bool slot_lane;                 // the lane has a slot (tid < max_tracks)
    const double* nowhere;          // what a lane with nothing to load reads instead of branching around its load
};

// the batch: T steps of Q rows, `rows` of them can hold a detection, CH steps per chunk
struct TrackShape { int T, Q, M, rows, per, CH; };

// One slot of the table, in its lane's registers.  Whether the slot is alive travels beside it as a plain bool: it decides control
// flow, and as a struct's byte it would live in a vector register where a plain local is a lane mask.
struct SlotRegs {
    double x0, x1, x2, v0, v1, v2;
    int id, miss, hits;
};

struct Predicted { double p0, p1, p2, g2; };

struct Step { // one time step: its detections in LDS, its rows of the outputs
    int t, k, n_raw, nn, nq;
    bool blind, last; // last: of its chunk
    double* D;
    int32_t *o_id, *o_slot, *o_age;
};

// What sets out at a step's beginning and lands at its end, beside the lane's doubles of the same step of the next chunk: those are
// a plain `double pv[PFS]` of the step loop (as a member of this struct they cost five vector registers more).
struct Prefetch {
    int cnt_nx;     // doubles of that step to bring
    int pn;         // (a chunk's last step) the lane's count of the chunk after the next
};

__device__ __forceinline__ TrackLane lane_of(const TrackArgs& a)
{
    TrackLane L;
    L.tid = threadIdx.x; L.nth = blockDim.x; L.lane = L.tid & 63; L.wave = L.tid >> 6; L.nw = L.nth >> 6;
    L.det_lane = (L.tid + (L.nth >> 1)) % L.nth;
    L.below = (1ull << L.lane) - 1ull;
    L.slot_lane = L.tid < a.M;
    L.nowhere = (const double*)a.state;
    return L;
}

__device__ __forceinline__ TrackShape shape_of(const TrackArgs& a)
{
    TrackShape S;
    S.T = a.T; S.Q = a.Q; S.M = a.M;
    S.rows = S.Q < TRACK_MAX ? S.Q : TRACK_MAX;
    S.per = S.rows * 3;
    S.CH = CHUNK_DET / S.rows;
    if (S.CH > CHUNK_STEPS) S.CH = CHUNK_STEPS;
    return S;
}

__device__ __forceinline__ SlotRegs load_state(const TrackSlot* slots, const TrackLane& L, bool& alive)
{
    SlotRegs r{0., 0., 0., 0., 0., 0., 0, 0, 0};
    alive = false;
    if (L.slot_lane) {
        const TrackSlot s = slots[L.tid];
        r.x0 = s.pos[0]; r.x1 = s.pos[1]; r.x2 = s.pos[2]; r.v0 = s.vel[0]; r.v1 = s.vel[1]; r.v2 = s.vel[2];
        r.id = s.id; r.miss = s.miss; r.hits = s.hits; alive = s.alive != 0;
    }
    return r;
}

__device__ __forceinline__ void store_state(TrackSlot* slots, const TrackLane& L, const SlotRegs& r, bool alive)
{
    if (L.slot_lane) {
        TrackSlot s;
        s.pos[0] = r.x0; s.pos[1] = r.x1; s.pos[2] = r.x2; s.vel[0] = r.v0; s.vel[1] = r.v1; s.vel[2] = r.v2;
        s.id = r.id; s.miss = r.miss; s.hits = r.hits; s.alive = alive ? 1 : 0;
        slots[L.tid] = s;
    }
}

// the wave's live slots, for whoever reads them behind the next barrier
__device__ __forceinline__ void publish_live(const TrackLane& L, const TrackShared& sh, bool alive)
{
    const unsigned long long am = __ballot(alive);
    if (L.lane == 0) sh.live[L.wave] = am;
}

// the counts of the first two chunks, the flags, the live slots, and the first chunk's detections in bulk (once per call)
__device__ __forceinline__ void stage_first_chunk(const TrackArgs& a, const TrackLane& L, const TrackShared& sh, const TrackShape& S, bool alive)
{
    const int tid = L.tid, T = S.T, CH = S.CH, rows = S.rows, per = S.per;
    if (tid < 4) sh.live[tid] = 0;
    if (tid < 2) sh.more[tid] = 0;
    if (tid < CH) {
        sh.n[0][tid] = tid < T ? a.n[tid] : 0;
        sh.n[1][tid] = CH + tid < T ? a.n[CH + tid] : 0;
    }
    __syncthreads();
    publish_live(L, sh, alive);
    const int steps = T < CH ? T : CH, total = steps * per;
#pragma unroll 8
    for (int i = tid; i < total; i += L.nth) {
        const int s = i / per, r = i - s * per, ns = sh.n[0][s];
        const bool ok = ns <= rows && r < 3 * ns;
        const double v = *(ok ? a.xyz + ((size_t)s * S.Q * 3 + r) : L.nowhere);
        const int d = r / 3, comp = r - 3 * d;
        double* const dst = sh.det[0] + (s * rows + d) * 4;
        dst[comp] = ok ? v : 0.;
        if (comp == 0) dst[3] = 0.; // not taken
    }
}

__device__ __forceinline__ Step step_of(const TrackArgs& a, const TrackShared& sh, const TrackShape& S, int c, int k, int steps)
{
    Step st;
    st.k = k; st.t = c * S.CH + k;
    st.n_raw = sh.n[c % 3][k];
    st.blind = st.n_raw < 0 || st.n_raw > S.rows;
    st.nn = st.blind ? 0 : st.n_raw; st.nq = (st.nn + 63) >> 6;
    st.last = k == steps - 1;
    st.D = sh.det[c & 1] + k * S.rows * 4;
    st.o_id = a.id + (size_t)st.t * S.Q;
    st.o_slot = a.slot + (size_t)st.t * S.Q;
    st.o_age = a.age + (size_t)st.t * S.Q;
    return st;
}

// 1. predict; every slot's prediction and gate^2 into LDS.  Ends with the step's first barrier.
__device__ __forceinline__ Predicted predict(const TrackArgs& a, const TrackLane& L, const TrackShared& sh, const SlotRegs& r, bool alive)
{
    Predicted p{0., 0., 0., -1.};
    if (alive) {
        p.p0 = r.x0 + r.v0; p.p1 = r.x1 + r.v1; p.p2 = r.x2 + r.v2;
        const double g = a.gate * (double)(1 + r.miss);
        p.g2 = g * g;
    }
    if (L.slot_lane) { sh.pred[L.tid][0] = p.p0; sh.pred[L.tid][1] = p.p1; sh.pred[L.tid][2] = p.p2; sh.pred[L.tid][3] = p.g2; }
    __syncthreads();
    return p;
}

// Staging: the same step of the next chunk sets out.  Its rows below its count travel while this step is worked on and land
// behind it (land_prefetch).  The chunk's last step brings the counts of the chunk after the next as well.  (Behind the step's
// first barrier: the counts read here landed in the step before.)
__device__ __forceinline__ Prefetch prefetch_next_chunk_step(const TrackArgs& a, const TrackLane& L, const TrackShared& sh, const TrackShape& S,
                                                             const Step& st, int c, double (&pv)[PFS])
{
    Prefetch pf;
    const int tn = st.t + S.CH;
    pf.cnt_nx = 0;
    if (tn < S.T) {
        const int m = sh.n[(c + 1) % 3][st.k];
        pf.cnt_nx = m < 0 || m > S.rows ? 0 : 3 * m;
    }
#pragma unroll
    for (int k2 = 0; k2 < PFS; k2++) {
        pv[k2] = 0.;
        if (k2 * L.nth < pf.cnt_nx) { // (the same in every lane)
            const int i = k2 * L.nth + L.tid;
            pv[k2] = *(i < pf.cnt_nx ? a.xyz + ((size_t)tn * S.Q * 3 + i) : L.nowhere);
        }
    }
    pf.pn = 0;
    if (st.last) {
        const int tc = c * S.CH + 2 * S.CH + L.tid;
        pf.pn = a.n[L.tid < S.CH && tc < S.T ? tc : 0];
    }
    return pf;
}

// one past the highest live slot of the step's beginning: the columns scan no further
__device__ __forceinline__ int highest_live_slot(const TrackLane& L, const TrackShared& sh)
{
    int hi = 0;
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const unsigned long long m = q < L.nw ? uni64(sh.live[q]) : 0ull;
        if (m) hi = q * 64 + 64 - __builtin_clzll(m);
    }
    return hi;
}

// the row's best: smallest (d2, j) among the detections not taken, -1 = none (ascending j, strict comparison)
__device__ __forceinline__ int row_best(const double* D, int nn, const Predicted& p)
{
    int bj = -1;
    double best = 0.;
#pragma unroll 4
    for (int j = 0; j < nn; j++) {
        const double d0 = D[4 * j] - p.p0, d1 = D[4 * j + 1] - p.p1, d2_ = D[4 * j + 2] - p.p2, w = D[4 * j + 3];
        const double d2 = (d0 * d0 + d1 * d1) + d2_ * d2_;
        if (w == 0. && d2 < p.g2 && (bj < 0 || d2 < best)) { best = d2; bj = j; }
    }
    return bj;
}

// the column's best: smallest (d2, s) among the slots not taken, -1 = none
__device__ __forceinline__ int column_best(const double* D, int j, int hi, const TrackShared& sh)
{
    int cs = -1;
    if (D[4 * j + 3] == 0.) {
        const double e0 = D[4 * j], e1 = D[4 * j + 1], e2 = D[4 * j + 2];
        double cb = 0.;
#pragma unroll 4
        for (int s = 0; s < hi; s++) { // (a dead or taken slot's gate^2 is -1: nothing lies below it)
            const double d0 = e0 - sh.pred[s][0], d1 = e1 - sh.pred[s][1], d2_ = e2 - sh.pred[s][2];
            const double d2 = (d0 * d0 + d1 * d1) + d2_ * d2_;
            if (d2 < sh.pred[s][3] && (cs < 0 || d2 < cb)) { cb = d2; cs = s; }
        }
    }
    return cs;
}

// 2., 3. candidates and assignment: rounds of "every pair that is mutually best among what remains is accepted" (with a total
// order the same set as the sorted greedy walk), by broadcast reads of LDS.  -> the detection this slot took, -1 = none
__device__ __forceinline__ int assign_rounds(const TrackLane& L, const TrackShared& sh, const Step& st, const Predicted& p, int hi, bool alive,
                                             int& round)
{
    const int tid = L.tid, nn = st.nn;
    double* const D = st.D;
    int mj = -1;
    bool want = alive && nn > 0; // the slot is untaken and may still have a candidate
    while (nn > 0) {
        const int bj = want ? row_best(D, nn, p) : -1;
        for (int j = L.det_lane; j < nn; j += L.nth) sh.col[j] = column_best(D, j, hi, sh);
        __syncthreads();
        const bool got = bj >= 0 && sh.col[bj] == tid;
        if (got) { mj = bj; D[4 * bj + 3] = 1.; sh.pred[tid][3] = -1.; }
        want = want && bj >= 0 && !got; // a row without a candidate now has none later: the sets only shrink
        // does any slot go on?  The waves tell each other through the flag of the round's parity, which the round before
        // cleared (its last reader has passed a barrier since)
        const bool mine = __ballot(want) != 0ull;
        if (tid == 0) sh.more[(round + 1) & 1] = 0;
        if (L.lane == 0 && mine) sh.more[round & 1] = 1;
        __syncthreads();
        const bool more = sh.more[round & 1] != 0;
        round++;
        if (!more) break;
    }
    return mj;
}

// 4., 5. matched and unmatched slots; deaths come before births
__device__ __forceinline__ void update_matched_and_missed(const TrackArgs& a, SlotRegs& r, bool& alive, const Predicted& p, int mj, const double* D)
{
    if (!alive) return;
    if (mj >= 0) {
        const double e0 = D[4 * mj], e1 = D[4 * mj + 1], e2 = D[4 * mj + 2];
        r.v0 = r.v0 + a.beta * (e0 - p.p0); r.v1 = r.v1 + a.beta * (e1 - p.p1); r.v2 = r.v2 + a.beta * (e2 - p.p2);
        r.x0 = e0; r.x1 = e1; r.x2 = e2;
        r.miss = 0; r.hits += 1;
    } else {
        r.x0 = p.p0; r.x1 = p.p1; r.x2 = p.p2;
        r.miss += 1;
        if (r.miss > a.max_miss) alive = false;
    }
}

// the unmatched detections, 64 per word; every wave forms all of them.  -> how many
__device__ __forceinline__ int unmatched_detections(const TrackLane& L, const Step& st, unsigned long long dm[4])
{
    int U = 0;
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const int j = q * 64 + L.lane;
        dm[q] = q < st.nq ? __ballot(j < st.nn && st.D[4 * j + 3] == 0.) : 0ull;
        U += __popcll(dm[q]);
    }
    return U;
}

// the free slots below M, 64 per word.  -> how many
__device__ __forceinline__ int free_slots(const TrackLane& L, const TrackShared& sh, int M, unsigned long long fr[4])
{
    int F = 0;
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const int left = M - q * 64;
        const unsigned long long valid = left >= 64 ? ~0ull : (left > 0 ? (1ull << left) - 1ull : 0ull);
        fr[q] = q < L.nw ? ~uni64(sh.live[q]) & valid : 0ull;
        F += __popcll(fr[q]);
    }
    return F;
}

// 6. births: the k-th unmatched detection takes the k-th free slot, through ballots, until the detections, the free slots or the
// identities run out; the unmatched detections beyond that get their -1 here.  -> the detection this slot starts a track from, -1 = none
__device__ __forceinline__ int births(const TrackLane& L, const TrackShared& sh, const Step& st, int M, SlotRegs& r, bool& alive, int& next_id, int& code)
{
    int born = -1;
    unsigned long long dm[4];
    const int U = unmatched_detections(L, st, dm);
    if (U == 0) return born; // (the same in every lane)
    publish_live(L, sh, alive);
    __syncthreads();
    unsigned long long fr[4];
    const int F = free_slots(L, sh, M, fr);
    const long long ids_left = (long long)INT32_MAX - (long long)next_id;
    int B = U < F ? U : F;
    if ((long long)B > ids_left) B = ids_left < 0 ? 0 : (int)ids_left;
#pragma unroll
    for (int q = 0; q < 4; q++) {
        if ((q % L.nw) != L.wave) continue; // word q's lanes are this wave's
        const int j = q * 64 + L.lane;
        if (dm[q] >> L.lane & 1) {
            int kth = __popcll(dm[q] & L.below);
            for (int w = 0; w < q; w++) kth += __popcll(dm[w]);
            if (kth < B) sh.birth[kth] = j;
            else { st.o_id[j] = -1; st.o_slot[j] = -1; st.o_age[j] = -1; }
        }
    }
    __syncthreads();
    if (L.slot_lane && !alive) {
        int rank = 0;
#pragma unroll
        for (int q = 0; q < 4; q++) rank += q < L.wave ? __popcll(fr[q]) : (q == L.wave ? __popcll(fr[q] & L.below) : 0);
        if (rank < B) {
            const int j = sh.birth[rank];
            alive = true; r.id = next_id + rank;
            r.x0 = st.D[4 * j]; r.x1 = st.D[4 * j + 1]; r.x2 = st.D[4 * j + 2];
            r.v0 = 0.; r.v1 = 0.; r.v2 = 0.;
            r.miss = 0; r.hits = 1;
            born = j;
        }
    }
    next_id += B;
    if (U > B) code = B == F ? TRACK_ERR_FULL : TRACK_ERR_IDS;
    return born;
}

// What set out at the step's beginning lands (the next step's first barrier stands before its first reader).
__device__ __forceinline__ void land_prefetch(const TrackLane& L, const TrackShared& sh, const TrackShape& S, const Step& st, int c, const Prefetch& pf,
                                              const double (&pv)[PFS])
{
    // Every load of the step has arrived from here on, on every path: said outright (vmcnt(0), the other counters
    // left alone), because the compiler cannot see that whoever loaded also lands, and would otherwise make the NEXT
    // step wait at its top -- behind this step's output stores.
    __builtin_amdgcn_s_waitcnt(0x0f70);
    double* const nx = sh.det[(c & 1) ^ 1] + st.k * S.rows * 4;
#pragma unroll
    for (int k2 = 0; k2 < PFS; k2++)
        if (k2 * L.nth < pf.cnt_nx) {
            const int i = k2 * L.nth + L.tid;
            if (i < pf.cnt_nx) {
                const int d = i / 3, comp = i - 3 * d;
                nx[4 * d + comp] = pv[k2];
                if (comp == 0) nx[4 * d + 3] = 0.; // not taken
            }
        }
    if (st.last && L.tid < S.CH) sh.n[(c + 2) % 3][L.tid] = c * S.CH + 2 * S.CH + L.tid < S.T ? pf.pn : 0;
}

// the step's outputs leave: plain stores nothing waits on
__device__ __forceinline__ void emit_step(const TrackArgs& a, const TrackLane& L, const TrackShape& S, const Step& st, const SlotRegs& r, int row, int code)
{
    if (row >= 0) { st.o_id[row] = r.id; st.o_slot[row] = L.tid; st.o_age[row] = r.hits; }
    for (int q = st.nn + L.tid; q < S.Q; q += L.nth) { st.o_id[q] = -1; st.o_slot[q] = -1; st.o_age[q] = -1; }
    if (L.tid == 0) a.status[st.t] = code;
}

} // namespace

__global__ __launch_bounds__(256) void track_markers_kernel(TrackArgs a)
{
    __shared__ double s_det[2][CHUNK_DET * 4];
    __shared__ int s_n[3][CHUNK_STEPS];
    __shared__ double s_pred[TRACK_MAX][4];
    __shared__ int s_col[TRACK_MAX];
    __shared__ int s_birth[TRACK_MAX];
    __shared__ unsigned long long s_live[4];
    __shared__ int s_more[2];
    const TrackShared sh{s_det, s_n, s_pred, s_col, s_birth, s_live, s_more};

    const TrackLane L = lane_of(a);
    const TrackShape S = shape_of(a);
    const int n_chunks = (S.T + S.CH - 1) / S.CH;

    TrackHeader* const head = (TrackHeader*)a.state;
    TrackSlot* const slots = (TrackSlot*)(head + 1);
    bool alive;
    SlotRegs r = load_state(slots, L, alive);
    int next_id = head->next_id; // every lane keeps the same count
    int round = 0;               // rounds so far, over all steps
    stage_first_chunk(a, L, sh, S, alive);
    __builtin_amdgcn_s_waitcnt(0x0f70); // the state and the first chunk have arrived (vmcnt(0)): no wait for them is left to the loop
    __syncthreads();

    for (int c = 0; c < n_chunks; c++) {
        const int steps = S.T - c * S.CH < S.CH ? S.T - c * S.CH : S.CH;
        for (int k = 0; k < steps; k++) {
            const Step st = step_of(a, sh, S, c, k, steps);
            const Predicted p = predict(a, L, sh, r, alive);
            double pv[PFS];
            const Prefetch pf = prefetch_next_chunk_step(a, L, sh, S, st, c, pv);
            const int hi = highest_live_slot(L, sh);
            const int mj = assign_rounds(L, sh, st, p, hi, alive, round);
            update_matched_and_missed(a, r, alive, p, mj, st.D);
            int code = st.blind ? (st.n_raw < 0 ? TRACK_ERR_INPUT : TRACK_ERR_COUNT) : 0;
            const int born = births(L, sh, st, S.M, r, alive, next_id, code);
            publish_live(L, sh, alive); // the next step's live slots (read behind its first barrier)
            land_prefetch(L, sh, S, st, c, pf, pv);
            emit_step(a, L, S, st, r, mj >= 0 ? mj : born, code);
        }
    }

    store_state(slots, L, r, alive);
    if (L.tid == 0) { head->next_id = next_id; head->steps += S.T; }
}

void launch_track_markers(const TrackArgs& a, hipStream_t s)
{
    int threads = (a.M + 63) / 64 * 64; // one lane per slot, whole waves
    if (threads < MIN_THREADS) threads = MIN_THREADS;
    hipLaunchKernelGGL(track_markers_kernel, dim3(1), dim3(threads), 0, s, a);
}

} // namespace mocap
