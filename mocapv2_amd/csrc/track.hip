// track.hip -- marker identities across time steps: a constant-velocity prediction per track, gated nearest-neighbour
// assignment in the total order (d2, slot, detection), births and deaths (FP64).
//
// The reference has no counterpart (its {"tracker1": object_points[0]} message assumes one marker): the contract is the definition of
// DESIGN.md section 2, restated by tests/track_ref.py.  The library is built with -ffp-contract=off: every sum and product below is a
// separately rounded FP64 operation, in the order the definition gives, so the device and the restatement agree bit for bit.
//
// Work decomposition: the recursion over the time steps is inherent (a prediction needs the step before), so ONE workgroup walks
// the T steps, one lane per slot (one wave per 64 slots, two waves at least).  A step touches LDS and registers only: the detections live in two chunk buffers in LDS,
// and while step k of one chunk is worked on, the rows of step k of the next chunk are in flight (in registers); they land behind
// the step, so no global load sits on the step-to-step chain.  The counts run one chunk further ahead: they tell the staging which
// rows to load, and rows at and beyond a step's count are never read.  The slot table lives in registers.  The assignment runs rounds of "every pair
// that is mutually best among what remains is accepted" (with a total order the same set as the sorted greedy walk): lane s
// scans the detections for its row's best, lane j scans the predictions for its column's best, both by broadcast reads, in
// ascending index with a strict comparison -- no atomics at all, so the same call gives the same bits.  Births hand the k-th
// unmatched detection to the k-th free slot through ballots.  Outputs leave as plain stores nothing waits on.
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

// a value every lane holds, moved to scalar registers: loops over its bits are uniform
__device__ __forceinline__ unsigned long long uniform64(unsigned long long v)
{
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v), hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
    return (unsigned long long)hi << 32 | lo;
}

} // namespace

__global__ __launch_bounds__(256) void track_markers_kernel(TrackArgs a)
{
    __shared__ double s_det[2][CHUNK_DET * 4];   // the detections of two chunks: the one walked, the one arriving
    __shared__ int s_n[3][CHUNK_STEPS];          // the counts run one chunk ahead of the detections: they say which rows to load
    __shared__ double s_pred[TRACK_MAX][4];      // per slot: prediction, then gate^2 (-1: the slot is dead or taken, nothing lies below it)
    __shared__ int s_col[TRACK_MAX];             // per detection: its column's best slot of this round, -1 = none
    __shared__ int s_birth[TRACK_MAX];           // the k-th unmatched detection
    __shared__ unsigned long long s_live[4];     // the live slots, 64 per word
    __shared__ int s_more[2];                    // a round's "some slot still wants a detection", by the round's parity

    const int tid = threadIdx.x, nth = blockDim.x, lane = tid & 63, wave = tid >> 6, nw = nth >> 6;
    const int T = a.T, Q = a.Q, M = a.M;
    const int rows = Q < TRACK_MAX ? Q : TRACK_MAX;  // rows of a time step that can hold a detection
    const int per = rows * 3;
    int CH = CHUNK_DET / rows; // time steps of a chunk
    if (CH > CHUNK_STEPS) CH = CHUNK_STEPS;
    const int n_chunks = (T + CH - 1) / CH;
    const unsigned long long below = (1ull << lane) - 1ull;
    const int det_lane = (tid + (nth >> 1)) % nth;
    const double* const nowhere = (const double*)a.state; // what a lane with nothing to load reads instead of branching around its load

    // ---- the state: one slot per lane, in registers ----------------------------------------------------------------------------
    TrackHeader* const head = (TrackHeader*)a.state;
    TrackSlot* const slots = (TrackSlot*)(head + 1);
    const bool slot_lane = tid < M;
    double x0 = 0., x1 = 0., x2 = 0., v0 = 0., v1 = 0., v2 = 0.;
    int id = 0, miss = 0, hits = 0;
    bool alive = false;
    if (slot_lane) {
        const TrackSlot s = slots[tid];
        x0 = s.pos[0]; x1 = s.pos[1]; x2 = s.pos[2]; v0 = s.vel[0]; v1 = s.vel[1]; v2 = s.vel[2];
        id = s.id; miss = s.miss; hits = s.hits; alive = s.alive != 0;
    }
    int next_id = head->next_id; // every lane keeps the same count
    if (tid < 4) s_live[tid] = 0;
    if (tid < 2) s_more[tid] = 0;
    int round = 0; // rounds so far, over all steps
    if (tid < CH) { // the counts of the first two chunks
        s_n[0][tid] = tid < T ? a.n[tid] : 0;
        s_n[1][tid] = CH + tid < T ? a.n[CH + tid] : 0;
    }
    __syncthreads();
    {
        const unsigned long long am = __ballot(alive);
        if (lane == 0) s_live[wave] = am;
    }
    { // the first chunk's detections, in bulk (once per call)
        const int steps = T < CH ? T : CH, total = steps * per;
#pragma unroll 8
        for (int i = tid; i < total; i += nth) {
            const int s = i / per, r = i - s * per, ns = s_n[0][s];
            const bool ok = ns <= rows && r < 3 * ns;
            const double v = *(ok ? a.xyz + ((size_t)s * Q * 3 + r) : nowhere);
            const int d = r / 3, comp = r - 3 * d;
            double* const dst = s_det[0] + (s * rows + d) * 4;
            dst[comp] = ok ? v : 0.;
            if (comp == 0) dst[3] = 0.; // not taken
        }
    }
    __builtin_amdgcn_s_waitcnt(0x0f70); // the state and the first chunk have arrived (vmcnt(0)): no wait for them is left to the loop
    __syncthreads();

    for (int c = 0; c < n_chunks; c++) {
        const int b = c & 1, t0 = c * CH, steps = T - t0 < CH ? T - t0 : CH;

        for (int k = 0; k < steps; k++) {
            const int t = t0 + k;
            const int n_raw = s_n[c % 3][k];
            const bool blind = n_raw < 0 || n_raw > rows;
            const int nn = blind ? 0 : n_raw, nq = (nn + 63) >> 6;
            double* const D = s_det[b] + k * rows * 4;
            int32_t* const o_id = a.id + (size_t)t * Q;
            int32_t* const o_slot = a.slot + (size_t)t * Q;
            int32_t* const o_age = a.age + (size_t)t * Q;

            // ---- 1. predict ---------------------------------------------------------------------------------------------------
            double p0 = 0., p1 = 0., p2 = 0., g2 = -1.;
            if (alive) {
                p0 = x0 + v0; p1 = x1 + v1; p2 = x2 + v2;
                const double g = a.gate * (double)(1 + miss);
                g2 = g * g;
            }
            if (slot_lane) { s_pred[tid][0] = p0; s_pred[tid][1] = p1; s_pred[tid][2] = p2; s_pred[tid][3] = g2; }
            __syncthreads();
            // ---- staging: the same step of the next chunk sets out.  Its rows below its count (rows at and beyond a count are never
            //      read) travel while this step is worked on and land behind it, so no load sits on the step-to-step chain.  The
            //      chunk's last step brings the counts of the chunk after the next as well.  (Behind the step's first barrier: the
            //      counts read here landed in the step before.)
            const int tn = t + CH;
            int cnt_nx = 0; // doubles to bring
            if (tn < T) {
                const int m = s_n[(c + 1) % 3][k];
                cnt_nx = m < 0 || m > rows ? 0 : 3 * m;
            }
            double pv[PFS];
#pragma unroll
            for (int k2 = 0; k2 < PFS; k2++) {
                pv[k2] = 0.;
                if (k2 * nth < cnt_nx) { // (the same in every lane)
                    const int i = k2 * nth + tid;
                    pv[k2] = *(i < cnt_nx ? a.xyz + ((size_t)tn * Q * 3 + i) : nowhere);
                }
            }
            const bool last = k == steps - 1;
            int pn = 0;
            if (last) {
                const int tc = t0 + 2 * CH + tid;
                pn = a.n[tid < CH && tc < T ? tc : 0];
            }
            int hi = 0; // one past the highest live slot of the step's beginning: the columns scan no further
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const unsigned long long m = q < nw ? uniform64(s_live[q]) : 0ull;
                if (m) hi = q * 64 + 64 - __builtin_clzll(m);
            }

            // ---- 2., 3. candidates and assignment: rounds of mutually best pairs ----------------------------------------------
            int mj = -1;                  // the detection this slot took
            bool want = alive && nn > 0;  // the slot is untaken and may still have a candidate
            while (nn > 0) {
                int bj = -1;
                double best = 0.;
                if (want)
#pragma unroll 4
                    for (int j = 0; j < nn; j++) { // the row's best: smallest (d2, j) among the detections not taken
                        const double d0 = D[4 * j] - p0, d1 = D[4 * j + 1] - p1, d2_ = D[4 * j + 2] - p2, w = D[4 * j + 3];
                        const double d2 = (d0 * d0 + d1 * d1) + d2_ * d2_;
                        if (w == 0. && d2 < g2 && (bj < 0 || d2 < best)) { best = d2; bj = j; }
                    }
                // (detection j's lane sits half a workgroup away from slot j's: with few of both, rows and columns are scanned by
                //  different waves at the same time)
                for (int j = det_lane; j < nn; j += nth) { // the column's best: smallest (d2, s) among the slots not taken
                    int cs = -1;
                    if (D[4 * j + 3] == 0.) {
                        const double e0 = D[4 * j], e1 = D[4 * j + 1], e2 = D[4 * j + 2];
                        double cb = 0.;
#pragma unroll 4
                        for (int s = 0; s < hi; s++) { // (a dead or taken slot's gate^2 is -1: nothing lies below it)
                            const double d0 = e0 - s_pred[s][0], d1 = e1 - s_pred[s][1], d2_ = e2 - s_pred[s][2];
                            const double d2 = (d0 * d0 + d1 * d1) + d2_ * d2_;
                            if (d2 < s_pred[s][3] && (cs < 0 || d2 < cb)) { cb = d2; cs = s; }
                        }
                    }
                    s_col[j] = cs;
                }
                __syncthreads();
                const bool got = bj >= 0 && s_col[bj] == tid;
                if (got) { mj = bj; D[4 * bj + 3] = 1.; s_pred[tid][3] = -1.; }
                want = want && bj >= 0 && !got; // a row without a candidate now has none later: the sets only shrink
                // does any slot go on?  The waves tell each other through the flag of the round's parity, which the round before
                // cleared (its last reader has passed a barrier since)
                const bool mine = __ballot(want) != 0ull;
                if (tid == 0) s_more[(round + 1) & 1] = 0;
                if (lane == 0 && mine) s_more[round & 1] = 1;
                __syncthreads();
                const bool more = s_more[round & 1] != 0;
                round++;
                if (!more) break;
            }

            // ---- 4., 5. matched and unmatched slots; deaths come before births ---------------------------------------------------
            if (alive) {
                if (mj >= 0) {
                    const double e0 = D[4 * mj], e1 = D[4 * mj + 1], e2 = D[4 * mj + 2];
                    v0 = v0 + a.beta * (e0 - p0); v1 = v1 + a.beta * (e1 - p1); v2 = v2 + a.beta * (e2 - p2);
                    x0 = e0; x1 = e1; x2 = e2;
                    miss = 0; hits += 1;
                } else {
                    x0 = p0; x1 = p1; x2 = p2;
                    miss += 1;
                    if (miss > a.max_miss) alive = false;
                }
            }
            // ---- 6. births: the k-th unmatched detection takes the k-th free slot ---------------------------------------------
            int born = -1; // the detection this slot starts a track from
            unsigned long long dm[4]; // the unmatched detections, 64 per word; every wave forms all of them
            int U = 0;
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const int j = q * 64 + lane;
                dm[q] = q < nq ? __ballot(j < nn && D[4 * j + 3] == 0.) : 0ull;
                U += __popcll(dm[q]);
            }
            int code = blind ? (n_raw < 0 ? TRACK_ERR_INPUT : TRACK_ERR_COUNT) : 0;
            if (U > 0) { // (the same in every lane)
                const unsigned long long am = __ballot(alive);
                if (lane == 0) s_live[wave] = am;
                __syncthreads();
                unsigned long long fr[4]; // the free slots
                int F = 0;
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const int left = M - q * 64;
                    const unsigned long long valid = left >= 64 ? ~0ull : (left > 0 ? (1ull << left) - 1ull : 0ull);
                    fr[q] = q < nw ? ~uniform64(s_live[q]) & valid : 0ull;
                    F += __popcll(fr[q]);
                }
                const long long ids_left = (long long)INT32_MAX - (long long)next_id;
                int B = U < F ? U : F; // births: until the detections, the free slots or the identities run out
                if ((long long)B > ids_left) B = ids_left < 0 ? 0 : (int)ids_left;
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    if ((q % nw) != wave) continue; // word q's lanes are this wave's
                    const int j = q * 64 + lane;
                    if (dm[q] >> lane & 1) {
                        int kth = __popcll(dm[q] & below);
                        for (int w = 0; w < q; w++) kth += __popcll(dm[w]);
                        if (kth < B) s_birth[kth] = j;
                        else { o_id[j] = -1; o_slot[j] = -1; o_age[j] = -1; }
                    }
                }
                __syncthreads();
                if (slot_lane && !alive) {
                    int r = 0;
#pragma unroll
                    for (int q = 0; q < 4; q++) r += q < wave ? __popcll(fr[q]) : (q == wave ? __popcll(fr[q] & below) : 0);
                    if (r < B) {
                        const int j = s_birth[r];
                        alive = true; id = next_id + r;
                        x0 = D[4 * j]; x1 = D[4 * j + 1]; x2 = D[4 * j + 2];
                        v0 = 0.; v1 = 0.; v2 = 0.;
                        miss = 0; hits = 1;
                        born = j;
                    }
                }
                next_id += B;
                if (U > B) code = B == F ? TRACK_ERR_FULL : TRACK_ERR_IDS;
            }
            {
                const unsigned long long am = __ballot(alive); // the next step's live slots (read behind its first barrier)
                if (lane == 0) s_live[wave] = am;
            }
            // ---- what set out at the step's beginning lands (the next step's first barrier stands before its first reader) ----
            {
                // Every load of the step has arrived from here on, on every path: said outright (vmcnt(0), the other counters
                // left alone), because the compiler cannot see that whoever loaded also lands, and would otherwise make the NEXT
                // step wait at its top -- behind this step's output stores.
                __builtin_amdgcn_s_waitcnt(0x0f70);
                double* const nx = s_det[b ^ 1] + k * rows * 4;
#pragma unroll
                for (int k2 = 0; k2 < PFS; k2++)
                    if (k2 * nth < cnt_nx) {
                        const int i = k2 * nth + tid;
                        if (i < cnt_nx) {
                            const int d = i / 3, comp = i - 3 * d;
                            nx[4 * d + comp] = pv[k2];
                            if (comp == 0) nx[4 * d + 3] = 0.; // not taken
                        }
                    }
                if (last && tid < CH) s_n[(c + 2) % 3][tid] = t0 + 2 * CH + tid < T ? pn : 0;
            }
            // ---- the step's outputs leave: plain stores nothing waits on ----------------------------------------------------------
            const int row = mj >= 0 ? mj : born;
            if (row >= 0) { o_id[row] = id; o_slot[row] = tid; o_age[row] = hits; }
            for (int r = nn + tid; r < Q; r += nth) { o_id[r] = -1; o_slot[r] = -1; o_age[r] = -1; }
            if (tid == 0) a.status[t] = code;
        }
    }

    if (slot_lane) {
        TrackSlot s;
        s.pos[0] = x0; s.pos[1] = x1; s.pos[2] = x2; s.vel[0] = v0; s.vel[1] = v1; s.vel[2] = v2;
        s.id = id; s.miss = miss; s.hits = hits; s.alive = alive ? 1 : 0;
        slots[tid] = s;
    }
    if (tid == 0) { head->next_id = next_id; head->steps += T; }
}

void launch_track_markers(const TrackArgs& a, hipStream_t s)
{
    int threads = (a.M + 63) / 64 * 64; // one lane per slot, whole waves
    if (threads < MIN_THREADS) threads = MIN_THREADS;
    hipLaunchKernelGGL(track_markers_kernel, dim3(1), dim3(threads), 0, s, a);
}

} // namespace mocap
