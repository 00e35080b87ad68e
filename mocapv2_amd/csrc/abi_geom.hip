// abi_geom.hip -- C-ABI host file: the per-frame geometry calls (correspondence, epipolar scores, triangulation, reprojection)
// and the residuals of the pairwise bundle adjustment.
#include "ctx.h"

extern "C" {

// ---- geometry stage --------------------------------------------------------------------------------------------
int mocap_correspond(mocap_ctx_t c, const void* pts, long pt_st, long pt_sc, const int32_t* counts, long cnt_st, long cnt_sc,
                     int pts_f64, int T, int C, int P, double cutoff,
                     int max_groups, double* root_xyz, double* root_err, double* root_grp, int32_t* root_idx,
                     int32_t* order, int32_t* n_roots, void* stream)
{
    if (!c || !pts || !counts || !root_xyz || !root_err || !root_grp || !root_idx || !order || !n_roots)
        return fail(MOCAP_E_INVALID, "null argument");
    if ((pt_st | pt_sc) & 1) return fail(MOCAP_E_INVALID, "point strides must be even (whole points)");
    if (T < 1 || C < 1 || C > 32 || P < 1 || P > 255 || max_groups < 1) return fail(MOCAP_E_INVALID, "T=%d C=%d P=%d max_groups=%d", T, C, P, max_groups);
    if (c->n_cam < C) return fail(MOCAP_E_STATE, "mocap_set_cameras: %d cameras set, %d needed", c->n_cam, C);
    if (c->n_F < C - 1) return fail(MOCAP_E_STATE, "mocap_set_fundamentals: %d matrices set, %d needed", c->n_F, C - 1);
    if (set_device(c)) return MOCAP_E_HIP;
    if (!correspond_fits(P, C)) // the plan is adaptive (correspond.hip: corr_lds_plan); what is left are the candidate lists, P * C * 16 bytes
        return fail(MOCAP_E_UNSUPPORTED, "P=%d points x C=%d cameras needs %zu bytes of LDS per time step", P, C, correspond_smem_bytes(P, C));
    // error scratch: the groups of one time step lie back to back, so a step needs room for its total, not P x max_groups;
    // a step with more than max(2 * max_groups, 8192) groups in all reports MOCAP_CORR_E_GROUPS
    size_t budget = 2 * (size_t)max_groups > 8192 ? 2 * (size_t)max_groups : 8192;
    if (c->tune.corr_step_groups > 0) budget = (size_t)c->tune.corr_step_groups; // mocap_set_tuning(ctx, "corr_step_groups", n)
    if (budget > (size_t)P * max_groups) budget = (size_t)P * max_groups;
    if (budget > 0x7fffffff) budget = 0x7fffffff;
    size_t need = (size_t)T * budget;
    if (need > c->scratch.n) {
        std::lock_guard<std::mutex> lk(c->mu);
        TRY(c->scratch.reserve(need));
    }
    CorrArgs a;
    a.cams = c->cams; a.pts = pts; a.counts = counts; a.pts_f64 = pts_f64; a.T = T; a.C = C; a.P = P;
    a.pt_st = pt_st; a.pt_sc = pt_sc; a.cnt_st = cnt_st; a.cnt_sc = cnt_sc;
    a.cutoff = cutoff; a.max_groups = max_groups; a.root_xyz = root_xyz; a.root_err = root_err; a.root_grp = root_grp;
    a.root_idx = root_idx; a.order = order; a.n_roots = n_roots; a.scratch = c->scratch; a.step_budget = (int)budget;
    a.prio = c->tune.corr_prio; // A/B switch (no effect measured)
    a.threads = c->tune.corr_threads;
    EvPair p; bool on;
    prof_begin(c, (hipStream_t)stream, p, on);
    launch_correspond(a, (hipStream_t)stream);
    prof_end(c, PROF_CORRESPOND, (hipStream_t)stream, p, on);
    HIP_TRY(hipGetLastError());
    return MOCAP_OK;
}

int mocap_correspond_visible(mocap_ctx_t c, const void* pts, long pt_st, long pt_sc, const int32_t* counts, long cnt_st, long cnt_sc,
                             int pts_f64, int T, int C, int P, int distorted, double cutoff, double gate, int min_views, double max_err,
                             int max_passes, int max_hyp, int Q, double* xyz, double* err, int32_t* idx, uint32_t* views, int32_t* n,
                             void* stream)
{
    if (!c || !pts || !counts || !xyz || !err || !idx || !views || !n) return fail(MOCAP_E_INVALID, "null argument");
    if ((pt_st | pt_sc) & 1) return fail(MOCAP_E_INVALID, "point strides must be even (whole points)");
    if (T < 1 || C < 2 || C > 32 || P < 1 || P > 255) return fail(MOCAP_E_INVALID, "T=%d C=%d P=%d (C: 2..32, P: 1..255)", T, C, P);
    if (min_views < 2 || min_views > C) return fail(MOCAP_E_INVALID, "min_views=%d outside 2..C=%d", min_views, C);
    if (!(isfinite(cutoff) && cutoff > 0) || !(isfinite(gate) && gate > 0) || !(isfinite(max_err) && max_err > 0))
        return fail(MOCAP_E_INVALID, "cutoff=%g gate=%g max_err=%g must be finite and > 0", cutoff, gate, max_err);
    if (max_passes < 1 || max_hyp < 1 || max_hyp > 65535 || Q < 1 || Q > 65535 || (distorted != 0 && distorted != 1))
        return fail(MOCAP_E_INVALID, "max_passes=%d max_hyp=%d Q=%d distorted=%d (max_passes >= 1, max_hyp and Q: 1..65535, distorted: 0 / 1)",
                    max_passes, max_hyp, Q, distorted);
    if (c->n_cam < C) return fail(MOCAP_E_STATE, "mocap_set_cameras: %d cameras set, %d needed", c->n_cam, C);
    if (set_device(c)) return MOCAP_E_HIP;
    if (!correspond_visible_fits(P, C))
        return fail(MOCAP_E_UNSUPPORTED, "P=%d points x C=%d cameras needs %zu bytes of LDS per time step", P, C, correspond_visible_smem_bytes(P, C));
    // the hypotheses of a pass that outgrows LDS live in the error scratch mocap_correspond uses (the context's calls are ordered on one stream)
    const size_t step_bytes = correspond_visible_step_bytes(C, max_hyp);
    const size_t need = ((size_t)T * step_bytes + 7) / 8;
    if (need > c->scratch.n) {
        std::lock_guard<std::mutex> lk(c->mu);
        TRY(c->scratch.reserve(need));
    }
    VisArgs a;
    a.cams = c->cams; a.pts = pts; a.counts = counts; a.pt_st = pt_st; a.pt_sc = pt_sc; a.cnt_st = cnt_st; a.cnt_sc = cnt_sc;
    a.pts_f64 = pts_f64; a.T = T; a.C = C; a.P = P; a.distorted = distorted; a.cutoff = cutoff; a.gate2 = gate * gate; a.max_err = max_err;
    a.min_views = min_views; a.max_passes = max_passes; a.max_hyp = max_hyp; a.Q = Q;
    a.xyz = xyz; a.err = err; a.idx = idx; a.views = views; a.n = n;
    a.scratch = (unsigned char*)(double*)c->scratch; a.step_bytes = step_bytes; a.lds_budget = 0;
    EvPair p; bool on;
    prof_begin(c, (hipStream_t)stream, p, on);
    launch_correspond_visible(a, (hipStream_t)stream);
    prof_end(c, PROF_CORRESPOND, (hipStream_t)stream, p, on);
    HIP_TRY(hipGetLastError());
    return MOCAP_OK;
}

int mocap_refine_points(mocap_ctx_t c, const double* xyz, const int32_t* n, const uint32_t* views, int T, int Q, int C, const void* pts,
                        long pt_st, long pt_sc, int pts_f64, int P, const int32_t* idx, const double* grp, int distorted, int max_iters,
                        double ftol, double lambda0, double max_res2, int min_views, int max_drop, double* xyz_out, double* err,
                        double* res2, double* cov, uint32_t* views_out, uint32_t* dropped, int32_t* iters, int32_t* status, void* stream)
{
    if (c && T == 0) return MOCAP_OK; // no time step: nothing is read, nothing is launched
    if (!c || !xyz || !n || !xyz_out || !err || !res2 || !cov || !views_out || !dropped || !iters || !status)
        return fail(MOCAP_E_INVALID, "null argument");
    if ((pts != nullptr) == (grp != nullptr)) return fail(MOCAP_E_INVALID, "exactly one of pts_dev (indexed form) and grp_dev (grouped form)");
    if (pts && (!idx || !views)) return fail(MOCAP_E_INVALID, "the indexed form needs idx_dev and views_dev");
    if (pts && ((pt_st | pt_sc) & 1)) return fail(MOCAP_E_INVALID, "point strides must be even (whole points)");
    if (T < 0 || Q < 1 || Q > 65535 || C < 2 || C > 32 || (pts && P < 1))
        return fail(MOCAP_E_INVALID, "T=%d Q=%d C=%d P=%d (T >= 0, Q: 1..65535, C: 2..32, P >= 1)", T, Q, C, P);
    if (max_iters < 1 || max_iters > 10000 || !(ftol >= 0.0) || !(lambda0 > 0.0) || !(lambda0 <= 1e16))
        return fail(MOCAP_E_INVALID, "max_iters=%d ftol=%g lambda0=%g", max_iters, ftol, lambda0);
    if (!isfinite(max_res2) || min_views < 2 || min_views > C || max_drop < 0 || (distorted != 0 && distorted != 1))
        return fail(MOCAP_E_INVALID, "max_res2=%g min_views=%d max_drop=%d distorted=%d (max_res2 finite, min_views: 2..C=%d, max_drop >= 0, distorted: 0 / 1)",
                    max_res2, min_views, max_drop, distorted, C);
    if (c->n_cam < C) return fail(MOCAP_E_STATE, "mocap_set_cameras: %d cameras set, %d needed", c->n_cam, C);
    if (set_device(c)) return MOCAP_E_HIP;
    RefinePointsArgs a;
    a.cams = c->cams; a.xyz = xyz; a.n = n; a.views = views; a.T = T; a.Q = Q; a.C = C;
    a.pts = pts; a.pt_st = pt_st; a.pt_sc = pt_sc; a.pts_f64 = pts_f64; a.P = P; a.idx = idx; a.grp = grp;
    a.distorted = distorted; a.max_iters = max_iters; a.ftol = ftol; a.lambda0 = lambda0; a.max_res2 = max_res2;
    a.min_views = min_views; a.max_drop = max_drop;
    a.xyz_out = xyz_out; a.err = err; a.res2 = res2; a.cov = cov; a.views_out = views_out; a.dropped = dropped; a.iters = iters;
    a.status = status;
    launch_refine_points(a, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return MOCAP_OK;
}

int mocap_epipolar_scores(mocap_ctx_t c, const void* roots, int n_roots, const void* cand, int n_cand, int pts_f64, int f_index,
                          double* dist, float* lines, void* stream)
{
    if (!c || !roots || !cand || !dist) return fail(MOCAP_E_INVALID, "null argument");
    if (n_roots < 1 || n_cand < 1 || (long long)n_roots * n_cand > 0x7fffffffLL) return fail(MOCAP_E_INVALID, "n_roots=%d n_cand=%d", n_roots, n_cand);
    if (f_index < 0 || f_index >= c->n_F) return fail(MOCAP_E_STATE, "mocap_set_fundamentals: %d matrices set, index %d asked", c->n_F, f_index);
    if (set_device(c)) return MOCAP_E_HIP;
    EpiArgs a{c->cams, roots, cand, n_roots, n_cand, pts_f64, f_index, dist, lines};
    launch_epipolar_scores(a, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return MOCAP_OK;
}

int mocap_ba_residuals(mocap_ctx_t c, const double* params_host, int B, const double* pts, const uint8_t* valid, int N, int C,
                       float* residuals_host, int32_t* counts_host, void* stream)
{
    if (!c || !params_host || !pts || !valid || !residuals_host || !counts_host) return fail(MOCAP_E_INVALID, "null argument");
    if (B < 1 || N < 1 || C < 2 || C > 32 || (long long)B * N > (1LL << 28)) return fail(MOCAP_E_INVALID, "B=%d N=%d C=%d", B, N, C);
    if (c->n_cam < C) return fail(MOCAP_E_STATE, "mocap_set_cameras: %d cameras set, %d needed (their K and dist are used)", c->n_cam, C);
    if (set_device(c)) return MOCAP_E_HIP;
    std::lock_guard<std::mutex> lk(c->mu);
    const size_t np_ = (size_t)B * 6 * (C - 1);
    double* params; float* res; int32_t* counts; // the pinned block: parameters | residuals | counts
    auto carve = [&](char* base) {
        Carver k{base};
        k.take(params, np_); k.take(res, (size_t)B * N); k.take(counts, B);
        return k.used;
    };
    const size_t need = carve(nullptr);
    // (grown to twice what the call needs: a series of growing calls allocates a few times, not every time)
    if (need > c->ba_pinned.n) TRY(c->ba_pinned.reserve(need * 2));
    if ((size_t)B * N * 3 > c->ba_obj.n) TRY(c->ba_obj.reserve((size_t)B * N * 3 * 2));
    carve(c->ba_pinned);
    memcpy(params, params_host, sizeof(double) * np_);
    BaArgs a{c->cams, params, pts, valid, N, C, B, c->ba_obj, res, counts};
    launch_ba_residuals(a, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream)); // the one wait of an evaluation: the kernel has written the pinned block
    memcpy(residuals_host, a.res, sizeof(float) * (size_t)B * N);
    memcpy(counts_host, a.counts, sizeof(int32_t) * B);
    return MOCAP_OK;
}

int mocap_triangulate_batch(mocap_ctx_t c, const double* pts, const uint8_t* valid, int N, int C, int compact_k, double* xyz,
                            int32_t* ok, void* stream)
{
    if (!c || !pts || !valid || !xyz || !ok) return fail(MOCAP_E_INVALID, "null argument");
    if (N < 1 || C < 1 || C > 32) return fail(MOCAP_E_INVALID, "N=%d C=%d", N, C);
    if (c->n_cam < C) return fail(MOCAP_E_STATE, "mocap_set_cameras: %d cameras set, %d needed", c->n_cam, C);
    if (set_device(c)) return MOCAP_E_HIP;
    TriArgs a{c->cams, pts, valid, N, C, compact_k, xyz, ok};
    launch_triangulate(a, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return MOCAP_OK;
}

int mocap_reproject_batch(mocap_ctx_t c, const double* pts, const uint8_t* valid, const double* xyz, int N, int C, int compact_k,
                          double* mse, int32_t* ok, void* stream)
{
    if (!c || !pts || !valid || !xyz || !mse || !ok) return fail(MOCAP_E_INVALID, "null argument");
    if (N < 1 || C < 1 || C > 32) return fail(MOCAP_E_INVALID, "N=%d C=%d", N, C);
    if (c->n_cam < C) return fail(MOCAP_E_STATE, "mocap_set_cameras: %d cameras set, %d needed", c->n_cam, C);
    if (set_device(c)) return MOCAP_E_HIP;
    ReprojArgs a{c->cams, pts, valid, xyz, N, C, compact_k, mse, ok};
    launch_reproject(a, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return MOCAP_OK;
}

} // extern "C"
