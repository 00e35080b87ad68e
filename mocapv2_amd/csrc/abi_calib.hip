// abi_calib.hip -- C-ABI host file: the calibration solvers (fundamental matrices by RANSAC, the rig's bundle adjustment, the
// cameras' intrinsics).
#include <functional>
#include "ctx.h"

extern "C" {

int mocap_fundamental_ransac(mocap_ctx_t c, int n_pairs, const double* pts_a, const double* pts_b, const int32_t* pair_offset_host,
                             const int32_t* samples, int H, double threshold, int refit, double* F_sample, double* F_refit,
                             uint8_t* inlier, int32_t* status, int32_t* counts, void* stream)
{
    if (!c || !pts_a || !pts_b || !pair_offset_host || !samples || !F_sample || !inlier || !status || (refit && !F_refit))
        return fail(MOCAP_E_INVALID, "null argument");
    if (n_pairs < 1 || H < 1 || (long long)n_pairs * H > (1LL << 26)) return fail(MOCAP_E_INVALID, "n_pairs=%d H=%d", n_pairs, H);
    if (n_pairs > 65535) return fail(MOCAP_E_INVALID, "n_pairs=%d: at most 65535 pairs per call", n_pairs);
    if (!(threshold > 0.0) || !(threshold * threshold <= 1.7976931348623157e308)) return fail(MOCAP_E_INVALID, "threshold %g is not a positive finite number", threshold);
    if (pair_offset_host[0] < 0) return fail(MOCAP_E_INVALID, "pair_offset[0] = %d", pair_offset_host[0]);
    int max_n = 0;
    for (int p = 0; p < n_pairs; p++) {
        const long long n = (long long)pair_offset_host[p + 1] - pair_offset_host[p];
        if (n < 8) return fail(MOCAP_E_INVALID, "pair %d: offsets %d .. %d leave %lld points, 8 are needed", p, pair_offset_host[p], pair_offset_host[p + 1], n);
        if (n > (1 << 26)) return fail(MOCAP_E_INVALID, "pair %d: %lld points, at most 2^26 per pair", p, n);
        if (n > max_n) max_n = (int)n;
    }
    if (set_device(c)) return MOCAP_E_HIP;
    std::lock_guard<std::mutex> lk(c->mu);
    // scratch (grown to twice what the call needs; the partition depends on n_pairs and H alone):
    // F_all [n_pairs][H][9] doubles | counts [n_pairs][H] | pair_err [n_pairs] | offset [n_pairs + 1]
    const size_t nh = (size_t)n_pairs * H;
    double* F_all; int32_t *cnt_own, *pair_err, *offset_dev;
    auto carve = [&](char* base) {
        Carver k{base};
        k.take(F_all, 9 * nh);
        k.take(cnt_own, nh); k.take(pair_err, n_pairs); // cleared below as one span up to offset_dev
        k.take(offset_dev, (size_t)n_pairs + 1);
        return k.used;
    };
    const size_t need = carve(nullptr);
    if (need > c->fund_scratch.n) TRY(c->fund_scratch.reserve(need * 2));
    carve(c->fund_scratch);
    hipStream_t s = (hipStream_t)stream;
    // pageable host memory: the copy has left the caller's array when this returns
    HIP_TRY(hipMemcpyAsync(offset_dev, pair_offset_host, sizeof(int32_t) * ((size_t)n_pairs + 1), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemsetAsync(cnt_own, 0, (char*)offset_dev - (char*)cnt_own, s));
    if (counts) HIP_TRY(hipMemsetAsync(counts, 0, sizeof(int32_t) * nh, s));
    FundArgs a{pts_a, pts_b, offset_dev, samples, n_pairs, H, max_n, threshold * threshold, F_all, counts ? counts : cnt_own,
               pair_err, F_sample, refit ? F_refit : nullptr, inlier, status};
    launch_fundamental_ransac(a, s);
    HIP_TRY(hipGetLastError());
    return MOCAP_OK;
}

// The scratch of a rig bundle adjustment by the solver sv, carved out of one block the context owns (grown to twice what a
// call needs; calls on one context are ordered on one stream).  The partition depends on the problem's sizes alone, never on
// the block's: a call's results do not depend on earlier calls.  `own` takes the solver's own buffers, behind the state record.
static int rig_args(mocap_ctx* c, const RigSolver& sv, int C, int N, int n_obs, const int32_t* obs_offset, const int32_t* obs_cam,
                    const double* obs_uv, double* poses, double* points, RigArgs& a, const std::function<void(Carver&)>& own)
{
    if (C < 2 || C > 32 || N < 1 || N > (1 << 24) || n_obs < 2 * (long long)N || n_obs > (long long)N * C)
        return fail(MOCAP_E_INVALID, "C=%d N=%d n_obs=%d: 2..32 cameras, 1..2^24 points, 2..C observations per point", C, N, n_obs);
    a = RigArgs{};
    a.obs_offset = obs_offset; a.obs_cam = obs_cam; a.obs_uv = obs_uv; a.C = C; a.N = N; a.n_obs = n_obs;
    const int blocks = C - sv.FIRST, chunk = sv.schur_chunk(N); // cameras that have a block
    a.n_pairs = blocks * (blocks + 1) / 2; a.n_lin_blocks = (N + PT_THREADS - 1) / PT_THREADS; a.n_chunks = (N + chunk - 1) / chunk;
    a.poses_io = poses; a.points_io = points;
    const size_t P = sv.P, D = P * blocks;
    auto carve = [&](char* base) {
        Carver k{base};
        k.take(a.state, 1); own(k);
        k.take(a.poses, 2 * 12 * (size_t)C); k.take(a.points, 2 * 3 * (size_t)N); k.take(a.mask, N);
        k.take(a.W, 3 * P * (size_t)n_obs); k.take(a.Vinv, 6 * (size_t)N); k.take(a.vdiag, 3 * (size_t)N); k.take(a.gp, 3 * (size_t)N);
        k.take(a.lin_part, (P * (P + 1) / 2 + P) * (size_t)a.n_lin_blocks * blocks); k.take(a.cost_part, a.n_lin_blocks);
        k.take(a.schur_part, (P * P + P) * (size_t)a.n_chunks * a.n_pairs);
        k.take(a.S, D * D); k.take(a.rhs, D); k.take(a.gc, D); k.take(a.udiag, D); k.take(a.chol, D * (D + 1) / 2); k.take(a.delta_c, D);
        k.take(a.upd_part, 3 * (size_t)a.n_lin_blocks); k.take(a.scalars, RIG_N_SCALARS);
        return k.used;
    };
    const size_t need = carve(nullptr);
    if (need > c->rig_scratch.n) TRY(c->rig_scratch.reserve(need * 2));
    carve(c->rig_scratch);
    return 0;
}

// The plain solver's: the lenses are the context's cameras'.  Clears the state record.
static int pose_args(mocap_ctx* c, int C, int N, int n_obs, const int32_t* obs_offset, const int32_t* obs_cam, const double* obs_uv,
                     double* poses, double* points, hipStream_t s, RigArgs& a)
{
    TRY(rig_args(c, rig_pose_solver(), C, N, n_obs, obs_offset, obs_cam, obs_uv, poses, points, a, [](Carver&) {}));
    if (c->n_cam < C) return fail(MOCAP_E_STATE, "mocap_set_cameras: %d cameras set, %d needed (their K and dist are used)", c->n_cam, C);
    a.cams = c->cams;
    HIP_TRY(hipMemsetAsync(a.state, 0, sizeof(RigState), s));
    return 0;
}

// The lens-refining solver's, with the checks that need the caller's mask and a host copy of kd: nothing is launched for a
// mask with bits above 8 or a kd that is not finite or has fx, fy <= 0.  Uploads the cameras' free columns, clears the state
// record and the cameras' counts.
static int lens_args(mocap_ctx* c, int C, int N, int n_obs, const int32_t* obs_offset, const int32_t* obs_cam, const double* obs_uv,
                     double* kd, const int32_t* refine_mask_host, double* poses, double* points, hipStream_t s, RigArgs& a)
{
    int32_t* d_free;
    TRY(rig_args(c, rig_lens_solver(), C, N, n_obs, obs_offset, obs_cam, obs_uv, poses, points, a, [&](Carver& k) {
        k.take(a.cam_count, C); // cleared with the state record as one span up to d_free
        k.take(d_free, C); k.take(a.kd, 2 * 9 * (size_t)C);
    }));
    int32_t free_cols[32];
    for (int k = 0; k < C; k++) {
        if (refine_mask_host[k] < 0 || refine_mask_host[k] > 0x1ff)
            return fail(MOCAP_E_INVALID, "refine_mask[%d] = 0x%x: bits 0..8 (fx, fy, cx, cy, k1, k2, p1, p2, k3)", k, (unsigned)refine_mask_host[k]);
        free_cols[k] = refine_mask_host[k] | (k > 0 ? 0x3f << 9 : 0);
    }
    double kd_host[32 * 9];
    HIP_TRY(hipMemcpyAsync(kd_host, kd, 8 * 9 * (size_t)C, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    for (int k = 0; k < 9 * C; k++)
        if (!(fabs(kd_host[k]) <= 1.7976931348623157e308) || (k % 9 < 2 && !(kd_host[k] > 0.0)))
            return fail(MOCAP_E_INVALID, "kd[%d][%d] = %g: every entry finite, fx and fy > 0", k / 9, k % 9, kd_host[k]);
    a.kd_io = kd; a.free_cols = d_free; a.schur_chunk = rig_lens_solver().schur_chunk(N);
    // pageable host memory: the copy has left `free_cols` when this returns
    HIP_TRY(hipMemcpyAsync(d_free, free_cols, sizeof(int32_t) * C, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemsetAsync(a.state, 0, (char*)d_free - (char*)a.state, s));
    return 0;
}

// The loss of the robust entries, checked before anything is launched: its number, and with Cauchy a finite scale > 0.
static int rig_loss(int loss, double loss_scale)
{
    if (loss != MOCAP_RIG_LOSS_NONE && loss != MOCAP_RIG_LOSS_CAUCHY)
        return fail(MOCAP_E_INVALID, "loss = %d: MOCAP_RIG_LOSS_NONE (0) or MOCAP_RIG_LOSS_CAUCHY (1)", loss);
    if (loss == MOCAP_RIG_LOSS_CAUCHY && (!(loss_scale > 0.0) || !(loss_scale <= 1.7976931348623157e308)))
        return fail(MOCAP_E_INVALID, "loss_scale = %g: the Cauchy loss needs a finite scale > 0 (pixels)", loss_scale);
    return 0;
}

// Linearises the state handed in (it is only read: the init kernel copies it, no finish kernel runs) and copies out what the
// linearize entries return.
static int rig_linearize(const RigSolver& sv, RigArgs& a, double lambda, int loss, double loss_scale, double* cost, double* gradient,
                         double* S, double* rhs, int32_t* status, hipStream_t s)
{
    a.loss = loss; a.loss_c2 = loss_scale * loss_scale;
    const size_t D = sv.P * (size_t)(a.C - sv.FIRST);
    sv.init(a, lambda, s);
    sv.linearize(a, s);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(cost, a.scalars + RIG_LIN_COST, 8, hipMemcpyDeviceToDevice, s));
    HIP_TRY(hipMemcpyAsync(gradient, a.gc, 8 * D, hipMemcpyDeviceToDevice, s));
    HIP_TRY(hipMemcpyAsync(gradient + D, a.gp, 8 * 3 * (size_t)a.N, hipMemcpyDeviceToDevice, s));
    HIP_TRY(hipMemcpyAsync(S, a.S, 8 * D * D, hipMemcpyDeviceToDevice, s));
    HIP_TRY(hipMemcpyAsync(rhs, a.rhs, 8 * D, hipMemcpyDeviceToDevice, s));
    // status: (layout error, a point not in front of a camera that sees it)
    HIP_TRY(hipMemcpyAsync(status, &a.state->layout_err, 4, hipMemcpyDeviceToDevice, s));
    HIP_TRY(hipMemcpyAsync(status + 1, &a.state->behind, 4, hipMemcpyDeviceToDevice, s));
    return MOCAP_OK;
}

// The loop: the caller's outputs cleared, then init, max_iters iterations, finish and, where asked for, the residuals.
static int rig_adjust(const RigSolver& sv, RigArgs& a, int max_iters, double ftol, double lambda0, double* history, double* result,
                      int loss, double loss_scale, double* obs_err, double* obs_weight, hipStream_t s)
{
    a.history = history; a.result = result;
    a.loss = loss; a.loss_c2 = loss_scale * loss_scale; a.obs_err = obs_err; a.obs_weight = obs_weight;
    HIP_TRY(hipMemsetAsync(history, 0, 8 * 4 * (size_t)max_iters, s));
    if (obs_err) HIP_TRY(hipMemsetAsync(obs_err, 0, 8 * (size_t)a.n_obs, s));
    if (obs_weight) HIP_TRY(hipMemsetAsync(obs_weight, 0, 8 * (size_t)a.n_obs, s));
    sv.init(a, lambda0, s);
    // every iteration is enqueued; the kernels of an iteration after the stop return at once
    for (int it = 0; it < max_iters; it++) sv.iteration(a, it, max_iters, ftol, s);
    sv.finish(a, s);
    if (obs_err || obs_weight) sv.residuals(a, s);
    HIP_TRY(hipGetLastError());
    return MOCAP_OK;
}

int mocap_rig_linearize(mocap_ctx_t c, int C, int N, int n_obs, const int32_t* obs_offset, const int32_t* obs_cam, const double* obs_uv,
                        const double* poses, const double* points, double lambda, double* cost, double* gradient, double* S,
                        double* rhs, int32_t* status, void* stream)
{
    return mocap_rig_linearize_robust(c, C, N, n_obs, obs_offset, obs_cam, obs_uv, poses, points, lambda, cost, gradient, S, rhs, status,
                                      MOCAP_RIG_LOSS_NONE, 0.0, stream);
}

int mocap_rig_linearize_robust(mocap_ctx_t c, int C, int N, int n_obs, const int32_t* obs_offset, const int32_t* obs_cam,
                               const double* obs_uv, const double* poses, const double* points, double lambda, double* cost,
                               double* gradient, double* S, double* rhs, int32_t* status, int loss, double loss_scale, void* stream)
{
    if (!c || !obs_offset || !obs_cam || !obs_uv || !poses || !points || !cost || !gradient || !S || !rhs || !status)
        return fail(MOCAP_E_INVALID, "null argument");
    if (!(lambda >= 0.0) || !(lambda <= 1e300)) return fail(MOCAP_E_INVALID, "lambda = %g", lambda);
    TRY(rig_loss(loss, loss_scale));
    if (set_device(c)) return MOCAP_E_HIP;
    std::lock_guard<std::mutex> lk(c->mu);
    hipStream_t s = (hipStream_t)stream;
    RigArgs a;
    TRY(pose_args(c, C, N, n_obs, obs_offset, obs_cam, obs_uv, const_cast<double*>(poses), const_cast<double*>(points), s, a));
    return rig_linearize(rig_pose_solver(), a, lambda, loss, loss_scale, cost, gradient, S, rhs, status, s);
}

int mocap_rig_bundle_adjust(mocap_ctx_t c, int C, int N, int n_obs, const int32_t* obs_offset, const int32_t* obs_cam,
                            const double* obs_uv, double* poses, double* points, int max_iters, double ftol, double lambda0,
                            double* history, double* result, void* stream)
{
    return mocap_rig_bundle_adjust_robust(c, C, N, n_obs, obs_offset, obs_cam, obs_uv, poses, points, max_iters, ftol, lambda0, history,
                                          result, MOCAP_RIG_LOSS_NONE, 0.0, nullptr, nullptr, stream);
}

int mocap_rig_bundle_adjust_robust(mocap_ctx_t c, int C, int N, int n_obs, const int32_t* obs_offset, const int32_t* obs_cam,
                                   const double* obs_uv, double* poses, double* points, int max_iters, double ftol, double lambda0,
                                   double* history, double* result, int loss, double loss_scale, double* obs_err, double* obs_weight,
                                   void* stream)
{
    if (!c || !obs_offset || !obs_cam || !obs_uv || !poses || !points || !history || !result) return fail(MOCAP_E_INVALID, "null argument");
    if (max_iters < 1 || max_iters > 10000 || !(ftol >= 0.0) || !(lambda0 > 0.0) || !(lambda0 <= 1e16))
        return fail(MOCAP_E_INVALID, "max_iters=%d ftol=%g lambda0=%g", max_iters, ftol, lambda0);
    TRY(rig_loss(loss, loss_scale));
    if (set_device(c)) return MOCAP_E_HIP;
    std::lock_guard<std::mutex> lk(c->mu);
    hipStream_t s = (hipStream_t)stream;
    RigArgs a;
    TRY(pose_args(c, C, N, n_obs, obs_offset, obs_cam, obs_uv, poses, points, s, a));
    return rig_adjust(rig_pose_solver(), a, max_iters, ftol, lambda0, history, result, loss, loss_scale, obs_err, obs_weight, s);
}

int mocap_rig_linearize_intrinsics(mocap_ctx_t c, int C, int N, int n_obs, const int32_t* obs_offset, const int32_t* obs_cam,
                                   const double* obs_uv, const double* kd, const int32_t* refine_mask_host, const double* poses,
                                   const double* points, double lambda, double* cost, double* gradient, double* S, double* rhs,
                                   int32_t* status, int loss, double loss_scale, void* stream)
{
    if (!c || !obs_offset || !obs_cam || !obs_uv || !kd || !refine_mask_host || !poses || !points || !cost || !gradient || !S || !rhs || !status)
        return fail(MOCAP_E_INVALID, "null argument");
    if (!(lambda >= 0.0) || !(lambda <= 1e300)) return fail(MOCAP_E_INVALID, "lambda = %g", lambda);
    TRY(rig_loss(loss, loss_scale));
    if (set_device(c)) return MOCAP_E_HIP;
    std::lock_guard<std::mutex> lk(c->mu);
    hipStream_t s = (hipStream_t)stream;
    RigArgs a;
    TRY(lens_args(c, C, N, n_obs, obs_offset, obs_cam, obs_uv, const_cast<double*>(kd), refine_mask_host, const_cast<double*>(poses),
                  const_cast<double*>(points), s, a));
    return rig_linearize(rig_lens_solver(), a, lambda, loss, loss_scale, cost, gradient, S, rhs, status, s);
}

int mocap_rig_bundle_adjust_intrinsics(mocap_ctx_t c, int C, int N, int n_obs, const int32_t* obs_offset, const int32_t* obs_cam,
                                       const double* obs_uv, double* kd, const int32_t* refine_mask_host, double* poses, double* points,
                                       int max_iters, double ftol, double lambda0, double* history, double* result, int loss,
                                       double loss_scale, double* obs_err, double* obs_weight, void* stream)
{
    if (!c || !obs_offset || !obs_cam || !obs_uv || !kd || !refine_mask_host || !poses || !points || !history || !result)
        return fail(MOCAP_E_INVALID, "null argument");
    if (max_iters < 1 || max_iters > 10000 || !(ftol >= 0.0) || !(lambda0 > 0.0) || !(lambda0 <= 1e16))
        return fail(MOCAP_E_INVALID, "max_iters=%d ftol=%g lambda0=%g", max_iters, ftol, lambda0);
    TRY(rig_loss(loss, loss_scale));
    if (set_device(c)) return MOCAP_E_HIP;
    std::lock_guard<std::mutex> lk(c->mu);
    hipStream_t s = (hipStream_t)stream;
    RigArgs a;
    TRY(lens_args(c, C, N, n_obs, obs_offset, obs_cam, obs_uv, kd, refine_mask_host, poses, points, s, a));
    return rig_adjust(rig_lens_solver(), a, max_iters, ftol, lambda0, history, result, loss, loss_scale, obs_err, obs_weight, s);
}

// The scratch of an intrinsic calibration, carved out of one block the context owns (grown to twice what a call needs); the
// partition depends on the problem's sizes alone.  Checks the host-side layout, and uploads it with what it implies: the
// camera of every view, and per camera whether it has its 3 views of 4 points and as many equations as unknowns.
static int intr_args(mocap_ctx* c, int n_cams, const int32_t* view_offset, const int32_t* point_offset, const int32_t* image_size,
                     const double* obj, const double* img, hipStream_t s, IntrArgs& a)
{
    if (n_cams < 1 || n_cams > 65536) return fail(MOCAP_E_INVALID, "n_cams=%d: 1..65536 cameras", n_cams);
    if (view_offset[0] != 0) return fail(MOCAP_E_INVALID, "view_offset[0] = %d", view_offset[0]);
    for (int k = 0; k < n_cams; k++)
        if (view_offset[k + 1] < view_offset[k]) return fail(MOCAP_E_INVALID, "view_offset descends at camera %d", k);
    const int n_views = view_offset[n_cams];
    if (n_views < 1 || n_views > (1 << 20)) return fail(MOCAP_E_INVALID, "%d views: 1..2^20", n_views);
    if (point_offset[0] != 0) return fail(MOCAP_E_INVALID, "point_offset[0] = %d", point_offset[0]);
    for (int v = 0; v < n_views; v++)
        if (point_offset[v + 1] < point_offset[v]) return fail(MOCAP_E_INVALID, "point_offset descends at view %d", v);
    const int total = point_offset[n_views];
    if (total < 1 || total > (1 << 26)) return fail(MOCAP_E_INVALID, "%d points: 1..2^26", total);
    if (image_size)
        for (int k = 0; k < 2 * n_cams; k++)
            if (image_size[k] < 1) return fail(MOCAP_E_INVALID, "camera %d: image size %d x %d", k / 2, image_size[k & ~1], image_size[k | 1]);
    // one host block, one copy: view_offset | point_offset | view_cam | image_size | cam_bad
    const size_t n_int = ((size_t)n_cams + 1) + ((size_t)n_views + 1) + n_views + 2 * (size_t)n_cams + n_cams;
    std::vector<int32_t> host(n_int);
    int32_t* h_voff = host.data(); int32_t* h_poff = h_voff + n_cams + 1; int32_t* h_vcam = h_poff + n_views + 1;
    int32_t* h_size = h_vcam + n_views; int32_t* h_bad = h_size + 2 * (size_t)n_cams;
    memcpy(h_voff, view_offset, sizeof(int32_t) * ((size_t)n_cams + 1));
    memcpy(h_poff, point_offset, sizeof(int32_t) * ((size_t)n_views + 1));
    for (int k = 0; k < n_cams; k++) {
        const int64_t views = view_offset[k + 1] - view_offset[k], points = point_offset[view_offset[k + 1]] - point_offset[view_offset[k]];
        bool bad = views < 3 || 2 * points < 9 + 6 * views; // two equations a point, 9 + 6 views unknowns
        for (int v = view_offset[k]; v < view_offset[k + 1]; v++) { h_vcam[v] = k; bad = bad || point_offset[v + 1] - point_offset[v] < 4; }
        h_bad[k] = bad;
        h_size[2 * k] = image_size ? image_size[2 * k] : 1; h_size[2 * k + 1] = image_size ? image_size[2 * k + 1] : 1;
    }
    a = IntrArgs{};
    a.n_cams = n_cams; a.n_views = n_views; a.obj = obj; a.img = img;
    const size_t nc = n_cams, nv = n_views;
    int32_t* d_int;
    auto carve = [&](char* base) {
        Carver k{base};
        k.take(d_int, n_int); k.take(a.state, nc); k.take(a.kd, 2 * 9 * nc); k.take(a.poses, 2 * 12 * nv); k.take(a.view_cost, 2 * nv);
        k.take(a.H, 9 * nv); k.take(a.rec, (size_t)INTR_REC * nv);
        k.take(a.gc, 9 * nc); k.take(a.gv, 6 * nv); k.take(a.S, 81 * nc); k.take(a.rhs, 9 * nc); // mocap_intrinsics_linearize clears
        k.take(a.udiag, 9 * nc);                                                                 // these four as one span up to udiag
        k.take(a.delta_c, 9 * nc); k.take(a.lin_cost, nc); k.take(a.cam_part, 2 * nc); k.take(a.upd_part, 3 * nv);
        return k.used;
    };
    const size_t need = carve(nullptr);
    if (need > c->intr_scratch.n) TRY(c->intr_scratch.reserve(need * 2));
    carve(c->intr_scratch);
    // pageable host memory: the copy has left `host` when this returns
    HIP_TRY(hipMemcpyAsync(d_int, host.data(), 4 * n_int, hipMemcpyHostToDevice, s));
    a.view_offset = d_int; a.point_offset = d_int + (h_poff - h_voff); a.view_cam = d_int + (h_vcam - h_voff);
    a.image_size = d_int + (h_size - h_voff); a.cam_bad = d_int + (h_bad - h_voff);
    HIP_TRY(hipMemsetAsync(a.state, 0, sizeof(IntrState) * nc, s));
    return 0;
}

int mocap_intrinsics_linearize(mocap_ctx_t c, int n_cams, const int32_t* view_offset_host, const int32_t* point_offset_host,
                               const double* obj_xy, const double* img_uv, const double* kd, const double* view_poses, double lambda,
                               double* cost, double* gradient, double* S, double* rhs, int32_t* status, void* stream)
{
    if (!c || !view_offset_host || !point_offset_host || !obj_xy || !img_uv || !kd || !view_poses || !cost || !gradient || !S || !rhs || !status)
        return fail(MOCAP_E_INVALID, "null argument");
    if (!(lambda >= 0.0) || !(lambda <= 1e300)) return fail(MOCAP_E_INVALID, "lambda = %g", lambda);
    if (set_device(c)) return MOCAP_E_HIP;
    std::lock_guard<std::mutex> lk(c->mu);
    hipStream_t s = (hipStream_t)stream;
    IntrArgs a;
    TRY(intr_args(c, n_cams, view_offset_host, point_offset_host, nullptr, obj_xy, img_uv, s, a));
    // (the state handed in is only read: the begin kernel copies it, no finish kernel runs)
    a.kd_io = const_cast<double*>(kd); a.poses_io = const_cast<double*>(view_poses); a.lin_status = status;
    const size_t nc = n_cams, nv = a.n_views;
    // gc | gv | S | rhs lie one after another in the scratch: a camera with a layout error leaves its entries zero
    HIP_TRY(hipMemsetAsync(a.gc, 0, (char*)a.udiag - (char*)a.gc, s));
    HIP_TRY(hipMemsetAsync(a.lin_cost, 0, 8 * nc, s));
    launch_intr_begin(a, 1, lambda, s);
    launch_intr_linearize(a, 0, false, s);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(cost, a.lin_cost, 8 * nc, hipMemcpyDeviceToDevice, s));
    HIP_TRY(hipMemcpyAsync(gradient, a.gc, 8 * 9 * nc, hipMemcpyDeviceToDevice, s));
    HIP_TRY(hipMemcpyAsync(gradient + 9 * nc, a.gv, 8 * 6 * nv, hipMemcpyDeviceToDevice, s));
    HIP_TRY(hipMemcpyAsync(S, a.S, 8 * 81 * nc, hipMemcpyDeviceToDevice, s));
    HIP_TRY(hipMemcpyAsync(rhs, a.rhs, 8 * 9 * nc, hipMemcpyDeviceToDevice, s));
    return MOCAP_OK;
}

int mocap_intrinsics_calibrate(mocap_ctx_t c, int n_cams, const int32_t* view_offset_host, const int32_t* point_offset_host,
                               const double* obj_xy, const double* img_uv, const int32_t* image_size_host, int have_start, int max_iters,
                               double ftol, double lambda0, double* kd, double* view_poses, double* view_rms, double* history, double* result,
                               void* stream)
{
    if (!c || !view_offset_host || !point_offset_host || !obj_xy || !img_uv || !kd || !view_poses || !view_rms || !history || !result ||
        (!have_start && !image_size_host))
        return fail(MOCAP_E_INVALID, "null argument");
    if (max_iters < 1 || max_iters > 10000 || !(ftol >= 0.0) || !(lambda0 > 0.0) || !(lambda0 <= 1e16))
        return fail(MOCAP_E_INVALID, "max_iters=%d ftol=%g lambda0=%g", max_iters, ftol, lambda0);
    if (set_device(c)) return MOCAP_E_HIP;
    std::lock_guard<std::mutex> lk(c->mu);
    hipStream_t s = (hipStream_t)stream;
    IntrArgs a;
    TRY(intr_args(c, n_cams, view_offset_host, point_offset_host, image_size_host, obj_xy, img_uv, s, a));
    a.kd_io = kd; a.poses_io = view_poses; a.view_rms = view_rms; a.history = history; a.result = result; a.max_iters = max_iters;
    HIP_TRY(hipMemsetAsync(history, 0, 8 * 4 * (size_t)max_iters * n_cams, s));
    launch_intr_begin(a, have_start != 0, lambda0, s);
    // every iteration is enqueued; the kernels of a camera that has stopped return at once
    for (int it = 0; it < max_iters; it++) launch_intr_iteration(a, it, ftol, s);
    launch_intr_finish(a, s);
    HIP_TRY(hipGetLastError());
    return MOCAP_OK;
}

} // extern "C"
