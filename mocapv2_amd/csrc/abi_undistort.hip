// abi_undistort.hip -- C-ABI host file: the undistort tables of a slot and what the early-out can prove about them.
#include "ctx.h"

extern "C" {

int mocap_set_undistort(mocap_ctx_t c, int slot, const double K[9], const double dist[5], int* identity_out)
{
    if (!c || !K || !dist) return fail(MOCAP_E_INVALID, "null argument");
    if (slot < 0 || slot >= c->n_slots) return fail(MOCAP_E_INVALID, "slot %d out of range", slot);
    if (set_device(c)) return MOCAP_E_HIP;
    std::lock_guard<std::mutex> lk(c->mu);
    size_t per = (size_t)c->H * c->W;
    TRY(c->maps.reserve(per * c->n_slots * 2));
    TRY(c->map4.reserve(per * c->n_slots + 4)); // + 4: a quad load at the last pixel stays inside
    const int ncx_ = (c->W + 7) / 8, ncy_ = (c->H + 7) / 8;
    TRY(c->srcbox.reserve((size_t)ncx_ * ncy_ * c->n_slots));
    const int n_strips_ = tiling(c).n_strips;
    TRY(c->rowbox.reserve((size_t)c->H * n_strips_ * c->n_slots));
    MapArgs m;
    memcpy(m.K, K, sizeof(m.K));
    memcpy(m.dist, dist, sizeof(m.dist));
    m.H = c->H; m.W = c->W;
    m.map = slot_map(c, slot);
    m.mapw = slot_mapw(c, slot);
    m.map4 = slot_map4(c, slot);
    m.flags = c->map_flags + slot;
    HIP_TRY(hipMemset(m.flags, 0, sizeof(uint32_t)));
    launch_undistort_map(m, 0);
    HIP_TRY(hipGetLastError());
    uint32_t flags = 0;
    HIP_TRY(hipMemcpy(&flags, m.flags, sizeof(flags), hipMemcpyDeviceToHost));
    c->slot_state[slot] = (flags & 1u) ? 2 : 1;
    c->slot_compact[slot] = (flags & 2u) ? 0 : 1;
    c->slot_wmax[slot] = c->slot_state[slot] == 1 ? 1024u : 0u; // identity: every source pixel feeds exactly one output pixel
    {   // the lens itself stays on the device too: mocap_refine_centroids maps points through it in both directions
        double lens[SUBPIX_LENS] = {0};
        memcpy(lens, K, 9 * sizeof(double));
        memcpy(lens + 9, dist, 5 * sizeof(double));
        lens[14] = c->slot_state[slot] == 1 ? 1.0 : 0.0;
        TRY(c->lens.reserve((size_t)SUBPIX_LENS * c->n_slots, true));
        HIP_TRY(hipMemcpy(c->lens + (size_t)SUBPIX_LENS * slot, lens, sizeof(lens), hipMemcpyHostToDevice));
    }
    launch_srcbox(m.map4, c->srcbox + (size_t)ncx_ * ncy_ * slot, c->H, c->W, 0);
    HIP_TRY(hipGetLastError());
    launch_rowbox(m.map4, c->rowbox + (size_t)c->H * n_strips_ * slot, c->H, c->W, n_strips_, 0);
    HIP_TRY(hipGetLastError());
    std::vector<uint32_t> edge((size_t)ncx_ * ncy_, 0); // source cells read by windows that the image border cuts: bit 0 one axis, bit 1 both
    std::vector<int> reach32((size_t)ncx_ * ncy_ * 4);  // per source cell: x0, x1, y0, y1 of the output pixels that read it
    for (size_t i = 0; i < reach32.size(); i += 2) { reach32[i] = 0x7fffffff; reach32[i + 1] = -0x7fffffff - 1; }
    if (c->slot_state[slot] == 2) {
        // statistics for the dark-tile early-out (see blob_scan.hip): total weight per source pixel, tap extents
        Buf<uint32_t> tmp; // (released at every return)
        const size_t edge_words = edge.size();
        TRY(tmp.reserve(per + 4 + edge_words + reach32.size()));
        HIP_TRY(hipMemset(tmp, 0, sizeof(uint32_t) * (per + 4 + edge_words)));
        int* reach_dev = (int*)(tmp + per + 4 + edge_words);
        HIP_TRY(hipMemcpy(reach_dev, reach32.data(), sizeof(int) * reach32.size(), hipMemcpyHostToDevice));
        uint32_t st3[3] = {0, 0, 0};
        StatArgs sg{m.map, m.mapw, tmp, tmp + per, c->H, c->W, tmp + per + 4, reach_dev};
        launch_remap_stats(sg, 0);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpy(st3, tmp + per, sizeof(st3), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(edge.data(), tmp + per + 4, sizeof(uint32_t) * edge.size(), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(reach32.data(), reach_dev, sizeof(int) * reach32.size(), hipMemcpyDeviceToHost));
        if (st3[1] <= 9 && st3[2] <= 9 && c->W >= 8) c->slot_wmax[slot] = st3[0];
    }
    {   // Dark-tile early-out tables per 8x8 source cell: the reach (which output pixels read the cell: from the map itself
        // for a remapped camera, the cell's own pixels for the identity) and the border-cut window flags.
        const int H = c->H, W = c->W, ncx = ncx_, ncy = ncy_;
        std::vector<uint2> reach((size_t)ncx * ncy);
        std::vector<uint8_t> cflags((size_t)ncx * ncy);
        for (int cr = 0; cr < ncy; cr++)
            for (int cx = 0; cx < ncx; cx++) {
                const size_t i = (size_t)cr * ncx + cx;
                int x0, x1, y0, y1;
                if (c->slot_state[slot] == 1) {
                    x0 = 8 * cx; x1 = 8 * cx + 7 < W - 1 ? 8 * cx + 7 : W - 1; y0 = 8 * cr; y1 = 8 * cr + 7 < H - 1 ? 8 * cr + 7 : H - 1;
                    // identity: the cut windows lie within 4 pixels of the border
                    const bool xc = 8 * cx < 4 || 8 * cx + 7 >= W - 4, yc = 8 * cr < 4 || 8 * cr + 7 >= H - 4;
                    edge[i] = (xc && yc) ? 2u : (xc || yc) ? 1u : 0u;
                } else {
                    x0 = reach32[4 * i]; x1 = reach32[4 * i + 1]; y0 = reach32[4 * i + 2]; y1 = reach32[4 * i + 3];
                }
                if (x0 > x1 || y0 > y1) reach[i] = make_uint2(1u, 0u); // read by nothing: x0 = 1 > x1 = 0
                else reach[i] = make_uint2((uint32_t)x0 | ((uint32_t)x1 << 16), (uint32_t)y0 | ((uint32_t)y1 << 16));
                cflags[i] = (edge[i] & 2u) ? 2 : (edge[i] & 1u) ? 1 : 0;
            }
        TRY(c->reach.reserve(reach.size() * c->n_slots));
        HIP_TRY(hipMemcpy(c->reach + reach.size() * slot, reach.data(), sizeof(uint2) * reach.size(), hipMemcpyHostToDevice));
        TRY(c->cflags.reserve(cflags.size() * c->n_slots));
        HIP_TRY(hipMemcpy(c->cflags + cflags.size() * slot, cflags.data(), cflags.size(), hipMemcpyHostToDevice));
    }
    if (identity_out) *identity_out = c->slot_state[slot] == 1;
    return MOCAP_OK;
}

int mocap_undistort_info(mocap_ctx_t c, int slot, mocap_undistort_info_t* out)
{
    if (!c || !out) return fail(MOCAP_E_INVALID, "null argument");
    if (slot < 0 || slot >= c->n_slots) return fail(MOCAP_E_INVALID, "slot %d out of range", slot);
    if (c->slot_state[slot] == 0) return fail(MOCAP_E_STATE, "mocap_set_undistort was not called for slot %d", slot);
    out->identity = c->slot_state[slot] == 1;
    out->compact_table = c->slot_compact[slot] != 0 && c->W >= 8;
    out->early_out_provable = c->slot_wmax[slot] != 0 && c->W >= 8;
    out->max_source_weight = (int32_t)c->slot_wmax[slot];
    // the sparse path (streaming scan + box kernel on the marked tiles) needs both; otherwise every tile of every image goes
    // through the dense row pipeline (same results, ~7x the time on a dark IR scene: DESIGN.md 4.1)
    out->sparse_path = out->compact_table && out->early_out_provable && c->tune.skip_dark && !c->tune.general_filter;
    return MOCAP_OK;
}

} // extern "C"
