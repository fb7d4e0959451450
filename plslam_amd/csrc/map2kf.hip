// map2kf.hip -- the map <-> keyframe association drivers of the reference as fused entry points:
// MapHandler::matchMap2KFPoints (src/mapHandler.cpp:532-632) and matchMap2KFLines (:634-752), with and
// without SlamConfig::fastMatching(), without the map mutation (that bookkeeping stays with the
// caller).  Projection / visibility pre-filter, Q/T descriptor matrix construction, the projection of
// the candidates into grid cells, StVO::matchGrid / StVO::match and the epipolar inlier gate all run on
// the MI355X; the host turns the visibility mask into index lists and fills the GridStructure (cell
// lists of the unmatched keyframe features, :580-584 / :683-699) -- the list building the reference's
// callers do with std::vector / std::list.
// This file reserves, uploads, launches and waits: four launch sequences (grid_path, map2kf_once, map2kf_steps, kf2kf_driver)
// behind ten entry points.  What is decided on the host -- checks, early returns, every layout, the staging, the reference's
// conditions -- is in map2kf_plan.hpp; the kernels are in map2kf_kernels.hip (map2kf_dev.hpp).
#include <cstring>
#include <vector>

#include "map2kf_dev.hpp"
#include "map2kf_plan.hpp"
#include "match_grid.hpp"
#include "match_plan.hpp"

namespace plslam {

// (env PLSLAM_MAP2KF_TABLE_IN_PLACE=0: the association table on the device and one copy at the call's end, as before round 6 -- for
// same-box comparisons)
static bool tab_in_place_enabled()
{
    static const bool on = [] { const char* e = getenv("PLSLAM_MAP2KF_TABLE_IN_PLACE"); return !(e && e[0] == '0'); }();
    return on;
}

namespace {
// StVO::matchGrid over projected 3D features, device-resident except the grid fill:
//   d_X3 (device): nq x 3 (points) / nq x 6 (lines) features, projected with T16 into cells * (sx, sy) by K16';
//   feat_curr (HOST): the keyframe features that fill the GridStructure -- item b = feat_curr[sel ? sel[b] : b],
//   2 doubles (pl) or 4 (spl, epl); d_Q / d_T (device): the descriptor matrices; d_m12: nq entries out (device memory, or
//   the device address of page-locked host memory: the caller then has the table without a copy).
// The host-built tables (cell_start, items, directions) and the problem descriptor travel in ONE page-locked image = one
// upload (GridPathLayout); the count comes back through page-locked memory written by the kernel.  Uses ctx->pin_misc,
// ctx->misc_b (tables) and ctx->misc_c (kernel scratch).  Synchronises the stream once, at the end.
int grid_path(plslam_ctx* ctx, int lines, const plslam_cam* K, const double* T16, const double* d_X3, int32_t nq, double sx,
              double sy, const uint8_t* d_Q, const double* feat_curr, const int32_t* sel, int32_t nt, const uint8_t* d_T,
              const plslam_fast_matching* fm, int mutual, int32_t* d_m12, int32_t* matches, const int32_t** deferred = nullptr)
{
    // deferred != nullptr: nothing is waited for here -- the caller has more work for the stream and synchronises itself; then
    // (*deferred)[0] is the count and (*deferred)[1] must be 0 ((*deferred)[0] >= 0): grid_path_check
    hipStream_t s = ctx->stream;
    StreamSyncOnError sg(s);
    int rc;
    const int nc = lines ? 2 : 1;
    const int64_t ncell = (int64_t)fm->grid_cols * fm->grid_rows;
    const GridTables g = fill_grid_tables(lines, feat_curr, sel, nt, fm);
    const GridPathLayout L(lines, nq, nt, GridSizes{g.cs.size(), (size_t)g.n_items, sizeof(GridDesc), grid_aux_words(nt)});
    if ((rc = ctx->pin_misc.reserve(L.image))) return rc;
    if ((rc = ctx->misc_b.reserve(L.bytes))) return rc;
    char* h = ctx->pin_misc.as<char>();
    char* f = ctx->misc_b.as<char>();
    // (the image of a problem the dense one-workgroup kernel takes is read ONCE, into LDS: it is read where it lies in page-locked
    // memory -- ctx option "zero_copy_kb", as plslam_match_grid -- and one copy command leaves the call; the projected cells and
    // the query directions, written by a kernel, stay in device memory: fi = the image's base as the kernels see it)
    const bool dense = grid_dense_ok(nq, nt, ncell, g.n_items, lines != 0, nc);
    const size_t zc_limit = (size_t)(ctx->zero_copy_kb < 0 ? -ctx->zero_copy_kb : ctx->zero_copy_kb) * 1024;
    const bool zero_copy = ctx->pin_misc.dev && zc_limit > 0 && L.image <= zc_limit && (dense || ctx->zero_copy_kb < 0);
    char* fi = zero_copy ? static_cast<char*>(ctx->pin_misc.dev) : f;
    stage_grid_tables(L, h, lines, nt, g);
    // capacity of the candidate store from the grid alone (fullest cell x cells of a window, at most every item, per window
    // centre; rows in blocks of 1024): the projected cells stay on the device, no round trip before the matcher is launched
    const int64_t cap = grid_tables_capacity(g, nq, nc, fm, mutual);
    PLSLAM_REQUIRE(cap < (int64_t(1) << 31) - 1, PLSLAM_ERANGE);
    if ((rc = ctx->misc_c.reserve(grid_scratch_words(nq, nt, ncell, (int32_t)cap) * 4 + 256))) return rc;
    // the count: written by the kernel into the page-locked image when the device can address it (no status word then: it
    // is bumped with an atomic; an overflow also shows as a count of -1)
    int32_t* res_host = (int32_t*)(h + L.oSt);
    int32_t* res_dev = ctx->pin_misc.dev ? (int32_t*)(static_cast<char*>(ctx->pin_misc.dev) + L.oSt) : nullptr;
    const bool in_place = res_dev != nullptr;
    res_host[0] = res_host[1] = 0;
    const plslam_grid_problem q = fill_grid_problem(L, f, fi, lines, d_Q, nq, d_T, nt, g.n_items, fm, mutual, cap, d_m12,
                                                    in_place ? res_dev : (int32_t*)(f + L.oSt));
    if ((rc = grid_prepare_one(q, ctx->misc_c.as<uint32_t>(), in_place ? nullptr : (int32_t*)(f + L.oSt) + 1, (GridDesc*)(h + L.oDesc))))
        return rc;
    grid_aux_fill(h + L.oAux, nt);
    if (!zero_copy) PLSLAM_HIP_CHECK(hipMemcpyAsync(f, h, L.image, hipMemcpyHostToDevice, s));      // (zeroes the device result words too)
    else if (!in_place) PLSLAM_HIP_CHECK(hipMemsetAsync(f + L.oSt, 0, 16, s));
    if ((rc = launch_project_cells(*K, T16, d_X3, nq, lines, sx, sy, (int32_t*)(f + L.oCen),
                                   lines ? (double*)(f + L.oD1) : nullptr, s)))
        return rc;
    if ((rc = grid_launch_single(q, (const GridDesc*)(fi + L.oDesc), s, (uint32_t*)(fi + L.oAux), false, (const GridDesc*)(h + L.oDesc)))) return rc;
    if (!in_place) PLSLAM_HIP_CHECK(hipMemcpyAsync(res_host, f + L.oSt, 8, hipMemcpyDeviceToHost, s));
    if (deferred) {
        sg.dismiss();
        *deferred = res_host;
        return PLSLAM_OK;
    }
    PLSLAM_HIP_CHECK(hipStreamSynchronize(s));
    sg.dismiss();
    PLSLAM_REQUIRE(res_host[1] == 0 && res_host[0] >= 0, PLSLAM_ERANGE);
    *matches = res_host[0];
    return PLSLAM_OK;
}

// The map<->keyframe driver as ONE launch sequence and ONE synchronisation, with fast_matching (fm != nullptr) and without.  The
// candidate list is built on the device (visibility x candidate flags -> stable compaction), so its length nq stays there -- the
// gathers, the projection, the matcher, the gate and the association read it from device memory -- and the one host decision of
// the reference loop that needs it, `|Q| > min && matches < min` (:594-598, :709-713), is taken AFTER the results are back.
//   fast: matchGrid's descriptor is patched with nq behind the upload (its launch geometry follows the upper bound n_map;
//   k_match_grid / k_grid_candidates pick their form from the patched row count).  When matchGrid found too little, the brute-
//   force matcher runs on what is still resident (Q, T, matchGrid's table as the vector it is handed), followed by the gate -- a
//   second, short launch sequence.
//   brute force (:594-598 / :709-713 with an empty matches_12: StVO::match over all of Q): the matcher is a two-launch column-
//   split plan sized for the bound n_map whose kernels read the row count from device memory (SymDesc::n1_dev: workgroups behind
//   the last row leave at once).  When match() would not have run (|Q| <= min_matches) the matcher's table is simply not used:
//   every entry of map_to_kf stays -1.
// Everything the host knows beforehand travels in ONE upload (OnceLayout, stage_once_image).
// *done = 0, nothing staged, uploaded or enqueued: the caller runs the step-by-step form -- fast: the candidate store would have
// to be sized for every landmark of a huge map; brute force: the plan cannot take a device-side row count under the context's
// options, or the problem is not mutual (bf_once_applies, asked FIRST).  Caller holds ctx->mu.
int map2kf_once(plslam_ctx* ctx, int lines, const plslam_cam* K, const double* Twf, const double* LM, const uint8_t* med_desc,
                const uint8_t* candidate, int32_t n_map, const uint8_t* kf_desc, const double* kf_feat, const double* kf_seg,
                const std::vector<int32_t>& ti, float nnr, int mutual, double max_epip, int32_t min_matches,
                const plslam_fast_matching* fm, int32_t* map_to_kf, int32_t* n_matches, int32_t* used_match, bool map_dev, int* done)
{
    *done = 0;
    const bool fast = fm != nullptr;
    const int32_t nt = (int32_t)ti.size();
    if (!fast && !bf_once_applies(mutual, n_map, nt, ctx_takes_device_row_count(ctx))) return PLSLAM_OK;
    hipStream_t s = ctx->stream;
    StreamSyncOnError sg(s);
    int rc;
    const int64_t ncell = fast ? (int64_t)fm->grid_cols * fm->grid_rows : 0;
    GridTables g;
    int64_t cap = 0;
    if (fast) {
        g = fill_grid_tables(lines, lines ? kf_seg : kf_feat, ti.data(), nt, fm);
        cap = grid_tables_capacity(g, n_map, lines ? 2 : 1, fm, mutual);           // (rows: the upper bound)
        if (store_needs_step_form(cap)) {
            sg.dismiss();
            return PLSLAM_OK;
        }
    }
    const GridSizes gs{g.cs.size(), (size_t)g.n_items, sizeof(GridDesc), fast ? grid_aux_words(nt) : 0};
    const OnceLayout L(lines, map_dev, n_map, nt, fast ? &gs : nullptr);
    if ((rc = ctx->misc_a.reserve(L.bytes))) return rc;
    if ((rc = ctx->pin_in.reserve(L.image))) return rc;
    if ((rc = ctx->pin_out.reserve(L.pin_out))) return rc;                // the counters' pages + the table behind them
    if (fast && (rc = ctx->misc_c.reserve(grid_scratch_words(n_map, nt, ncell, (int32_t)cap) * 4 + 256))) return rc;
    char* d = ctx->misc_a.as<char>();
    char* h = ctx->pin_in.as<char>();
    char* ho = ctx->pin_out.as<char>();
    stage_once_image(L, h, lines, map_dev, LM, med_desc, candidate, n_map, kf_desc, kf_feat, ti, fast ? &g : nullptr);
    const double* const d_LM = map_dev ? LM : (const double*)(d + L.oLM);
    const void* const d_MD = map_dev ? (const void*)med_desc : (const void*)(d + L.oMD);
    const uint8_t* const d_cand = map_dev ? candidate : (const uint8_t*)(d + L.oCand);
    int32_t* const res = (int32_t*)(d + L.oRes);                         // [0] gate count, [1] nq, [2] matchGrid's count, [3] publish ticket
    // the association table: written where the host reads it (the page-locked block, mapped) when the device can address it --
    // its -1 fill and the few hundred entries the gate sets cross PCIe as posted writes; the counters follow from the gate's last
    // workgroup: no copy command at the call's end
    const bool tab_in_place = ctx->pin_out.dev != nullptr && tab_in_place_enabled();
    int32_t* const tab = tab_in_place ? (int32_t*)(static_cast<char*>(ctx->pin_out.dev) + L.tab_out) : (int32_t*)(d + L.oMap);
    // the matcher's problem first: the brute-force plan decides whether its form applies at all
    plslam_grid_problem q{};
    plslam_match_problem p{};
    p.d1 = (const uint8_t*)(d + L.oQ); p.d2 = (const uint8_t*)(d + L.oT); p.n2 = nt;
    p.nnr = nnr; p.mutual = mutual ? 1 : 0; p.matches_12 = (int32_t*)(d + L.oM); p.n_matches = nullptr;
    if (fast) {
        q = fill_grid_problem(L, d, d, lines, p.d1, n_map, p.d2, nt, g.n_items, fm, mutual, cap, p.matches_12, res + 2);
        if ((rc = grid_prepare_one(q, ctx->misc_c.as<uint32_t>(), nullptr, (GridDesc*)(h + L.oDesc)))) return rc;
        grid_aux_fill(h + L.oAux, nt);
    }
    PLSLAM_HIP_CHECK(hipMemcpyAsync(d, h, L.image, hipMemcpyHostToDevice, s));
    // ---- the launch sequence (the small steps are fused -- a launch of a microsecond's work costs 4-5 us)
    if ((rc = launch_visible_compact(*K, Twf, d_LM, d_cand, n_map, lines, (int32_t*)(d + L.oQi), res + 1, tab,
                                     fast ? (GridDesc*)(d + L.oDesc) : nullptr, (uint32_t*)(d + L.oPart),
                                     /* zeroed by the image above */ true, s)))
        return rc;
    if ((rc = launch_prepare_rows(*K, Twf, d_MD, d_LM, (const int32_t*)(d + L.oQi), res + 1, n_map, lines, fast ? fm->inv_width : 0.0,
                                  fast ? fm->inv_height : 0.0, d + L.oQ, (double*)(d + L.oQL), fast ? (int32_t*)(d + L.oCen) : nullptr,
                                  fast && lines ? (double*)(d + L.oD1) : nullptr, s)))
        return rc;
    if (fast) {
        if ((rc = grid_launch_single(q, (const GridDesc*)(d + L.oDesc), s, (uint32_t*)(d + L.oAux), true, (const GridDesc*)(h + L.oDesc))))
            return rc;
    } else {
        p.n1 = n_map; p.keep_prior = 0;
        rc = match_problems_on_ctx_stream(ctx, &p, 1, res + 1);          // :597 / :712
        if (rc == PLSLAM_ENOTSUP) {
            // (cannot happen after the test at the top -- the plan's own refusals are the context's options --; if it ever does, what
            // is in flight writes scratch only: wait for it and let the caller take the step-by-step form)
            PLSLAM_HIP_CHECK(hipStreamSynchronize(s));
            sg.dismiss();
            return PLSLAM_OK;
        }
        if (rc) return rc;
    }
    if ((rc = launch_gate_n(lines, *K, Twf, (const double*)(d + L.oQL), (const int32_t*)(d + L.oM), res + 1, n_map,
                            (const double*)(d + L.oTF), max_epip, (uint8_t*)(d + L.oMask), res, (const int32_t*)(d + L.oQi),
                            (const int32_t*)(d + L.oTi), tab, s, tab_in_place ? res + 3 : nullptr, res, (int32_t*)ctx->pin_out.dev,
                            3)))                                          // (res[3]: zero in the image)
        return rc;
    // ---- the counters (from the gate's last workgroup) and, when it is not there already, the table behind them down; one synchronisation
    if (!tab_in_place) PLSLAM_HIP_CHECK(hipMemcpyAsync(ho, d + L.oRes, L.pin_out, hipMemcpyDeviceToHost, s));
    PLSLAM_HIP_CHECK(hipStreamSynchronize(s));
    sg.dismiss();
    *done = 1;
    const int32_t* r = reinterpret_cast<const int32_t*>(ho);
    if (!fast) {
        if (!needs_brute_force(r[1], 0, min_matches)) return PLSLAM_OK;   // match() would not have run: map_to_kf stays -1 everywhere
        if (used_match) *used_match = 1;
    } else {
        PLSLAM_REQUIRE(r[2] >= 0, PLSLAM_ERANGE);                        // (matchGrid's candidate store: the capacity is an upper bound)
        if (needs_brute_force(r[1], r[2], min_matches)) {
            // matchGrid found too little: StVO::match runs over the SAME Q and T with the vector matchGrid filled (keep_prior),
            // then the gate.  Everything it needs is still on the device -- Q, T, their features, the lists, matchGrid's table --
            // and the list's length is known now: no re-staging, no second visibility pass.  The association table and the
            // gate's counter start over.
            StreamSyncOnError sg2(s);
            PLSLAM_HIP_CHECK(hipMemsetAsync(d + L.oMap, 0xFF, (size_t)n_map * 4, s));
            PLSLAM_HIP_CHECK(hipMemsetAsync(res, 0, 4, s));
            p.n1 = r[1]; p.keep_prior = 1;
            if ((rc = match_problems_on_ctx_stream(ctx, &p, 1))) return rc;
            if ((rc = launch_gate_n(lines, *K, Twf, (const double*)(d + L.oQL), (const int32_t*)(d + L.oM), res + 1, n_map,
                                    (const double*)(d + L.oTF), max_epip, (uint8_t*)(d + L.oMask), res, (const int32_t*)(d + L.oQi),
                                    (const int32_t*)(d + L.oTi), (int32_t*)(d + L.oMap), s)))
                return rc;
            PLSLAM_HIP_CHECK(hipMemcpyAsync(ho, d + L.oRes, L.pin_out, hipMemcpyDeviceToHost, s));
            PLSLAM_HIP_CHECK(hipStreamSynchronize(s));
            sg2.dismiss();
            if (used_match) *used_match = 1;
        }
    }
    memcpy(map_to_kf, ho + L.tab_out, (size_t)n_map * 4);
    if (n_matches) *n_matches = r[0];
    return PLSLAM_OK;
}

// The map<->keyframe driver step by step: the visibility flags come back, the host builds the Q list, then gathers, matcher(s),
// gate -- two or three synchronisations.  What map2kf_once hands on (a huge map's candidate store, a plan that cannot take a
// device-side row count, a non-mutual problem).  Caller holds ctx->mu.
int map2kf_steps(plslam_ctx* ctx, int lines, const plslam_cam* K, const double* Twf, const double* LM, const uint8_t* med_desc,
                 const uint8_t* candidate, int32_t n_map, const uint8_t* kf_desc, const double* kf_feat, const double* kf_seg,
                 int32_t n_kf, const std::vector<int32_t>& ti, float nnr, int mutual, double max_epip, int32_t min_matches,
                 const plslam_fast_matching* fm, int32_t* map_to_kf, int32_t* n_matches, int32_t* used_match, bool map_dev)
{
    hipStream_t s = ctx->stream;
    StreamSyncOnError sg(s);
    const int lw = lines ? 6 : 3, fw = lines ? 3 : 2;
    const int32_t nt = (int32_t)ti.size();
    // ---- stage the map and the keyframe on the device (ONE page-locked image, one upload), project + visibility test ----
    const StepLayout L(lines, map_dev, n_map, n_kf, nt);
    int rc;
    if ((rc = ctx->misc_a.reserve(L.bytes))) return rc;
    if ((rc = ctx->pin_in.reserve(L.pin_in))) return rc;
    if ((rc = ctx->pin_out.reserve(L.pin_out))) return rc;
    char* d = ctx->misc_a.as<char>();
    char* h = ctx->pin_in.as<char>();
    char* ho = ctx->pin_out.as<char>();
    if (!map_dev) {
        memcpy(h + L.oLM, LM, (size_t)n_map * lw * 8);
        memcpy(h + L.oMD, med_desc, (size_t)n_map * 32);
    }
    const char* const d_LM = map_dev ? reinterpret_cast<const char*>(LM) : d + L.oLM;          // the map on the device
    const char* const d_MD = map_dev ? reinterpret_cast<const char*>(med_desc) : d + L.oMD;
    memcpy(h + L.oKD, kf_desc, (size_t)n_kf * 32);
    memcpy(h + L.oKF, kf_feat, (size_t)n_kf * fw * 8);
    PLSLAM_HIP_CHECK(hipMemcpyAsync(d, h, L.image1, hipMemcpyHostToDevice, s));
    // the visibility flags come back through page-locked memory the kernel writes (no download command)
    uint8_t* vis_mapped = static_cast<uint8_t*>(mapped_device_pointer(ho));
    rc = map_dev ? launch_visible_cand(*K, Twf, (const double*)d_LM, candidate, n_map, lines, vis_mapped ? vis_mapped : (uint8_t*)(d + L.oVis), s)
                 : launch_visible(*K, Twf, (const double*)d_LM, n_map, lines, vis_mapped ? vis_mapped : (uint8_t*)(d + L.oVis), s);
    if (rc) return rc;
    if (!vis_mapped) PLSLAM_HIP_CHECK(hipMemcpyAsync(ho, d + L.oVis, (size_t)n_map, hipMemcpyDeviceToHost, s));
    PLSLAM_HIP_CHECK(hipStreamSynchronize(s));
    const uint8_t* vis = reinterpret_cast<const uint8_t*>(ho);

    // ---- Q list: candidate landmarks that project inside the image, :545-558 / :647-663 ------
    std::vector<int32_t> qi;
    for (int32_t i = 0; i < n_map; ++i)
        if ((map_dev || candidate[i]) && vis[i]) qi.push_back(i);        // (map_dev: the kernel folded the flags in)
    const int32_t nq = (int32_t)qi.size();
    if (nq == 0) { sg.dismiss(); return PLSLAM_OK; }                      // :571 / :676

    // ---- build the Q / T matrices on the device, match, gate ----------------------------------
    memcpy(h, qi.data(), (size_t)nq * 4);                                  // (image 1 is on the device: the buffer is free)
    memcpy(h + (L.oTi - L.oQi), ti.data(), (size_t)nt * 4);
    PLSLAM_HIP_CHECK(hipMemcpyAsync(d + L.oQi, h, L.image2, hipMemcpyHostToDevice, s));
    if ((rc = launch_gather_rows(d_MD, (int32_t*)(d + L.oQi), nq, 32, d + L.oQ, s))) return rc;
    if ((rc = launch_gather_rows(d + L.oKD, (int32_t*)(d + L.oTi), nt, 32, d + L.oT, s))) return rc;
    if ((rc = launch_gather_rows(d_LM, (int32_t*)(d + L.oQi), nq, lw * 8, d + L.oQL, s))) return rc;
    if ((rc = launch_gather_rows(d + L.oKF, (int32_t*)(d + L.oTi), nt, fw * 8, d + L.oTF, s))) return rc;
    int32_t matches = 0;
    bool have_m12 = false;                       // matches_12.size() != 0: a matcher ran
    if (fm) {                                    // :578-592 / :681-707
        // the grid of the unmatched keyframe features: points :581-584, lines :686-698 (kf_seg = spl, epl)
        if ((rc = grid_path(ctx, lines, K, Twf, (const double*)(d + L.oQL), nq, fm->inv_width, fm->inv_height,
                            (const uint8_t*)(d + L.oQ), lines ? kf_seg : kf_feat, ti.data(), nt, (const uint8_t*)(d + L.oT),
                            fm, mutual, (int32_t*)(d + L.oM), &matches)))
            return rc;
        have_m12 = true;
    }
    if (needs_brute_force(nq, matches, min_matches)) {                   // :594-598 / :709-713
        plslam_match_problem p{};
        p.d1 = (uint8_t*)(d + L.oQ); p.n1 = nq; p.d2 = (uint8_t*)(d + L.oT); p.n2 = nt;
        p.nnr = nnr; p.mutual = mutual ? 1 : 0; p.matches_12 = (int32_t*)(d + L.oM); p.n_matches = nullptr;
        p.keep_prior = have_m12 ? 1 : 0;         // the vector matchGrid filled is handed on (:591 -> :597, :706 -> :712)
        if ((rc = match_problems_on_ctx_stream(ctx, &p, 1))) return rc;   // :597 / :712
        have_m12 = true;
        if (used_match) *used_match = 1;
    }
    if (!have_m12) { PLSLAM_HIP_CHECK(hipStreamSynchronize(s)); sg.dismiss(); return PLSLAM_OK; }
    rc = lines ? launch_line_gate(*K, Twf, (double*)(d + L.oQL), (int32_t*)(d + L.oM), nq, (double*)(d + L.oTF),
                                  max_epip, (uint8_t*)(d + L.oMask), (int32_t*)(d + L.oCnt), s)
               : launch_point_gate(*K, Twf, (double*)(d + L.oQL), (int32_t*)(d + L.oM), nq, (double*)(d + L.oTF),
                                   max_epip, (uint8_t*)(d + L.oMask), (int32_t*)(d + L.oCnt), s);
    if (rc) return rc;
    // table, mask and count lie behind one another: one download
    PLSLAM_HIP_CHECK(hipMemcpyAsync(ho, d + L.oM, L.results, hipMemcpyDeviceToHost, s));
    PLSLAM_HIP_CHECK(hipStreamSynchronize(s));
    sg.dismiss();
    const int32_t* m12 = reinterpret_cast<const int32_t*>(ho);
    const uint8_t* mask = reinterpret_cast<const uint8_t*>(ho + (L.oMask - L.oM));
    for (int32_t a = 0; a < nq; ++a)
        if (mask[a]) map_to_kf[qi[a]] = ti[m12[a]];                       // :614-619 (the association)
    if (n_matches) *n_matches = *reinterpret_cast<const int32_t*>(ho + (L.oCnt - L.oM));
    return PLSLAM_OK;
}

// MapHandler::matchKF2KFPoints / matchKF2KFLines, compute part (src/mapHandler.cpp:246-278 / :378-426)
int kf2kf_driver(plslam_ctx* ctx, int lines, const plslam_cam* K, const double* DT, const double* X_prev,
                 const uint8_t* desc_prev, int32_t n_prev, const double* feat_curr, const uint8_t* desc_curr,
                 int32_t n_curr, float nnr, int mutual, int32_t min_matches, const plslam_fast_matching* fm,
                 int32_t* matches_12, int32_t* n_matches, int32_t* used_match, bool rows_dev = false)
{
    // rows_dev: X_prev, desc_prev and desc_curr are DEVICE pointers (the keyframes' descriptors and the previous keyframe's 3D
    // features stay on the GPU between calls; 16-byte aligned rows): nothing is staged or uploaded but the grid of feat_curr
    Entry e;
    int rc = kf2kf_entry(ctx, K, DT, X_prev, desc_prev, n_prev, feat_curr, desc_curr, n_curr, min_matches, fm, matches_12, rows_dev, e);
    if (!entry_apply(e, matches_12, n_prev, n_matches, used_match)) return rc;
    const bool fast = fast_enabled(fm);
    const bool bf_possible = kf2kf_bf_possible(n_prev, n_curr, min_matches);
    const int xw = lines ? 6 : 3;
    std::lock_guard<std::mutex> lk(ctx->mu);
    DeviceGuard g(ctx->device);
    hipStream_t s = ctx->stream;
    StreamSyncOnError sg(s);
    // ONE page-locked image [desc_prev | desc_curr | X_prev] -> one upload (X only when the windowed matcher runs); the
    // match table comes back through page-locked memory the kernels write (no download on the common path)
    const Kf2kfLayout L(lines, rows_dev, fast, n_prev, n_curr);
    if ((rc = ctx->misc_a.reserve(L.bytes))) return rc;
    if ((rc = ctx->pin_in.reserve(L.image))) return rc;
    if ((rc = ctx->pin_out.reserve(L.pin_out))) return rc;
    char* d = ctx->misc_a.as<char>();
    char* h = ctx->pin_in.as<char>();
    if (!rows_dev) {
        memcpy(h + L.oQ, desc_prev, (size_t)n_prev * 32);
        memcpy(h + L.oT, desc_curr, (size_t)n_curr * 32);
        if (fast) memcpy(h + L.oX, X_prev, (size_t)n_prev * xw * 8);
        PLSLAM_HIP_CHECK(hipMemcpyAsync(d, h, L.image, hipMemcpyHostToDevice, s));
    }
    const uint8_t* const d_Q = rows_dev ? desc_prev : (const uint8_t*)(d + L.oQ);
    const uint8_t* const d_T = rows_dev ? desc_curr : (const uint8_t*)(d + L.oT);
    const double* const d_X = rows_dev ? X_prev : (const double*)(d + L.oX);
    int32_t* tab_host = ctx->pin_out.as<int32_t>();
    int32_t* tab_mapped = static_cast<int32_t*>(ctx->pin_out.dev);
    int32_t* tab_dev = (int32_t*)(d + L.oM);
    int32_t matches = 0;
    bool have = false, on_host = false;            // on_host: the current table is in tab_host (written by a kernel, synchronised)
    const bool both_known = kf2kf_both_known(fast, lines, bf_possible, rows_dev, tab_mapped != nullptr, K, DT, X_prev, n_prev, fm, min_matches);
    const int32_t* grid_res = nullptr;
    if (fast) {
        // points: pj_points = projection * inv (:256); lines: pj_lines = the projected PIXELS (:392-393, as upstream)
        if ((rc = grid_path(ctx, lines, K, DT, d_X, n_prev, lines ? 1.0 : fm->inv_width,
                            lines ? 1.0 : fm->inv_height, d_Q, feat_curr, nullptr, n_curr,
                            d_T, fm, mutual, tab_mapped ? tab_mapped : tab_dev, &matches, both_known ? &grid_res : nullptr)))
            return rc;
        have = true;
        on_host = tab_mapped != nullptr;           // (both_known: "will be" -- the stream's order puts match() behind the kernel that writes it)
    }
    Kf2kfTable t{};
    if (bf_possible && (both_known || matches < min_matches)) {            // :274-278 / :421-425
        t = kf2kf_table(have, on_host, tab_mapped != nullptr);
        plslam_match_problem p{};
        p.d1 = d_Q; p.n1 = n_prev; p.d2 = d_T; p.n2 = n_curr;
        p.nnr = nnr; p.mutual = mutual ? 1 : 0; p.n_matches = (int32_t*)(d + L.oCnt);
        p.keep_prior = have ? 1 : 0;             // the vector matchGrid filled is handed on (:271 -> :277, :418 -> :424)
        p.matches_12 = t.mapped ? tab_mapped : tab_dev;
        if (t.upload_first) PLSLAM_HIP_CHECK(hipMemcpyAsync(tab_dev, tab_host, (size_t)n_prev * 4, hipMemcpyHostToDevice, s));
        if ((rc = match_problems_on_ctx_stream(ctx, &p, 1))) return rc;
        if (!t.on_host) {
            PLSLAM_HIP_CHECK(hipMemcpyAsync(tab_host, tab_dev, (size_t)n_prev * 4, hipMemcpyDeviceToHost, s));
            PLSLAM_HIP_CHECK(hipMemcpyAsync(&matches, d + L.oCnt, 4, hipMemcpyDeviceToHost, s));
        } else if (t.count_only) {
            // (the count: behind the table in the page-locked block, by a one-lane launch -- a small copy command starts ~13 us after
            // the kernel in front of it, a kernel 2-3 us)
            if ((rc = launch_publish_words((const int32_t*)(d + L.oCnt), tab_mapped + n_prev, 1, s))) return rc;
        }
        PLSLAM_HIP_CHECK(hipStreamSynchronize(s));
        if (grid_res) PLSLAM_REQUIRE(grid_res[1] == 0 && grid_res[0] >= 0 && grid_res[0] < min_matches, PLSLAM_ERANGE);   // (the bound held)
        if (t.count_only) matches = tab_host[n_prev];
        have = true;
        if (used_match) *used_match = 1;
    } else if (have && !on_host) {
        PLSLAM_HIP_CHECK(hipMemcpyAsync(tab_host, tab_dev, (size_t)n_prev * 4, hipMemcpyDeviceToHost, s));
        PLSLAM_HIP_CHECK(hipStreamSynchronize(s));
    }
    sg.dismiss();
    if (!have) return PLSLAM_OK;
    memcpy(matches_12, tab_host, (size_t)n_prev * 4);
    if (t.count_entries) {
        matches = 0;
        for (int32_t i = 0; i < n_prev; ++i) matches += matches_12[i] >= 0;
    }
    if (n_matches) *n_matches = matches;
    return PLSLAM_OK;
}

int map2kf_driver(plslam_ctx* ctx, int lines, const plslam_cam* K, const double* Twf, const double* LM,
                  const uint8_t* med_desc, const uint8_t* candidate, int32_t n_map, const uint8_t* kf_desc,
                  const double* kf_feat, const double* kf_seg, const int32_t* kf_idx, int32_t n_kf, float nnr,
                  int mutual, double max_epip, int32_t min_matches, const plslam_fast_matching* fm,
                  int32_t* map_to_kf, int32_t* n_matches, int32_t* used_match, bool map_dev = false)
{
    // map_dev: LM, med_desc and candidate are DEVICE pointers (the local map lives on the GPU across keyframes): nothing of
    // the map is staged or uploaded, the candidate flags are folded into the visibility kernel
    Entry e;
    std::vector<int32_t> ti;                     // the unmatched keyframe features, :563-569 / :668-674
    const int rc = map2kf_entry(ctx, K, Twf, lines, LM, med_desc, candidate, n_map, kf_desc, kf_feat, kf_seg, kf_idx, n_kf, min_matches, fm,
                                map_to_kf, e, ti);
    if (!entry_apply(e, map_to_kf, n_map, n_matches, used_match)) return rc;
    if (!fast_enabled(fm)) fm = nullptr;
    std::lock_guard<std::mutex> lk(ctx->mu);
    DeviceGuard dg_(ctx->device);    // every entry point runs on the context's device, whatever the calling thread's current one
    // one launch sequence, one synchronisation (+ a second, short one on what is resident when the brute-force matcher has to
    // replace matchGrid's table); it asks for the step-by-step form only where its own form does not apply
    int done = 0;
    const int rc1 = map2kf_once(ctx, lines, K, Twf, LM, med_desc, candidate, n_map, kf_desc, kf_feat, kf_seg, ti, nnr, mutual, max_epip,
                                min_matches, fm, map_to_kf, n_matches, used_match, map_dev, &done);
    if (rc1 || done) return rc1;
    return map2kf_steps(ctx, lines, K, Twf, LM, med_desc, candidate, n_map, kf_desc, kf_feat, kf_seg, n_kf, ti, nnr, mutual, max_epip,
                        min_matches, fm, map_to_kf, n_matches, used_match, map_dev);
}
}  // namespace
}  // namespace plslam

extern "C" {

int plslam_map2kf_match_points(plslam_ctx* ctx, const plslam_cam* K, const double* Twf, const double* Xw,
                               const uint8_t* med_desc, const uint8_t* candidate, int32_t n_map,
                               const uint8_t* kf_desc, const double* kf_pl, const int32_t* kf_idx,
                               int32_t n_kf, float nnr, int mutual, double max_epip, int32_t min_matches,
                               int32_t* map_to_kf, int32_t* n_matches)
{
    return plslam::map2kf_driver(ctx, 0, K, Twf, Xw, med_desc, candidate, n_map, kf_desc, kf_pl, nullptr, kf_idx, n_kf,
                                 nnr, mutual, max_epip, min_matches, nullptr, map_to_kf, n_matches, nullptr);
}

int plslam_map2kf_match_lines(plslam_ctx* ctx, const plslam_cam* K, const double* Twf, const double* Lw,
                              const uint8_t* med_desc, const uint8_t* candidate, int32_t n_map,
                              const uint8_t* kf_desc, const double* kf_le, const int32_t* kf_idx,
                              int32_t n_kf, float nnr, int mutual, double max_epip, int32_t min_matches,
                              int32_t* map_to_kf, int32_t* n_matches)
{
    return plslam::map2kf_driver(ctx, 1, K, Twf, Lw, med_desc, candidate, n_map, kf_desc, kf_le, nullptr, kf_idx, n_kf,
                                 nnr, mutual, max_epip, min_matches, nullptr, map_to_kf, n_matches, nullptr);
}

int plslam_map2kf_match_points_fast(plslam_ctx* ctx, const plslam_cam* K, const double* Twf, const double* Xw,
                                    const uint8_t* med_desc, const uint8_t* candidate, int32_t n_map,
                                    const uint8_t* kf_desc, const double* kf_pl, const int32_t* kf_idx, int32_t n_kf,
                                    float nnr, int mutual, double max_epip, int32_t min_matches,
                                    const plslam_fast_matching* fm, int32_t* map_to_kf, int32_t* n_matches,
                                    int32_t* used_match)
{
    return plslam::map2kf_driver(ctx, 0, K, Twf, Xw, med_desc, candidate, n_map, kf_desc, kf_pl, nullptr, kf_idx, n_kf,
                                 nnr, mutual, max_epip, min_matches, fm, map_to_kf, n_matches, used_match);
}

int plslam_map2kf_match_lines_fast(plslam_ctx* ctx, const plslam_cam* K, const double* Twf, const double* Lw,
                                   const uint8_t* med_desc, const uint8_t* candidate, int32_t n_map,
                                   const uint8_t* kf_desc, const double* kf_le, const double* kf_seg,
                                   const int32_t* kf_idx, int32_t n_kf, float nnr, int mutual, double max_epip,
                                   int32_t min_matches, const plslam_fast_matching* fm, int32_t* map_to_kf,
                                   int32_t* n_matches, int32_t* used_match)
{
    return plslam::map2kf_driver(ctx, 1, K, Twf, Lw, med_desc, candidate, n_map, kf_desc, kf_le, kf_seg, kf_idx, n_kf,
                                 nnr, mutual, max_epip, min_matches, fm, map_to_kf, n_matches, used_match);
}

int plslam_map2kf_match_points_dev(plslam_ctx* ctx, const plslam_cam* K, const double* Twf, const double* d_Xw,
                                   const uint8_t* d_med_desc, const uint8_t* d_candidate, int32_t n_map,
                                   const uint8_t* kf_desc, const double* kf_pl, const int32_t* kf_idx, int32_t n_kf,
                                   float nnr, int mutual, double max_epip, int32_t min_matches,
                                   const plslam_fast_matching* fm, int32_t* map_to_kf, int32_t* n_matches,
                                   int32_t* used_match)
{
    PLSLAM_REQUIRE(n_map == 0 || (((uintptr_t)d_Xw & 7) == 0 && ((uintptr_t)d_med_desc & 7) == 0), PLSLAM_EINVAL);
    return plslam::map2kf_driver(ctx, 0, K, Twf, d_Xw, d_med_desc, d_candidate, n_map, kf_desc, kf_pl, nullptr, kf_idx, n_kf,
                                 nnr, mutual, max_epip, min_matches, fm, map_to_kf, n_matches, used_match, true);
}

int plslam_map2kf_match_lines_dev(plslam_ctx* ctx, const plslam_cam* K, const double* Twf, const double* d_Lw,
                                  const uint8_t* d_med_desc, const uint8_t* d_candidate, int32_t n_map,
                                  const uint8_t* kf_desc, const double* kf_le, const double* kf_seg,
                                  const int32_t* kf_idx, int32_t n_kf, float nnr, int mutual, double max_epip,
                                  int32_t min_matches, const plslam_fast_matching* fm, int32_t* map_to_kf,
                                  int32_t* n_matches, int32_t* used_match)
{
    PLSLAM_REQUIRE(n_map == 0 || (((uintptr_t)d_Lw & 7) == 0 && ((uintptr_t)d_med_desc & 7) == 0), PLSLAM_EINVAL);
    return plslam::map2kf_driver(ctx, 1, K, Twf, d_Lw, d_med_desc, d_candidate, n_map, kf_desc, kf_le, kf_seg, kf_idx, n_kf,
                                 nnr, mutual, max_epip, min_matches, fm, map_to_kf, n_matches, used_match, true);
}

int plslam_kf2kf_match_points(plslam_ctx* ctx, const plslam_cam* K, const double* DT, const double* P_prev,
                              const uint8_t* desc_prev, int32_t n_prev, const double* pl_curr, const uint8_t* desc_curr,
                              int32_t n_curr, float nnr, int mutual, int32_t min_matches, const plslam_fast_matching* fm,
                              int32_t* matches_12, int32_t* n_matches, int32_t* used_match)
{
    return plslam::kf2kf_driver(ctx, 0, K, DT, P_prev, desc_prev, n_prev, pl_curr, desc_curr, n_curr, nnr, mutual,
                                min_matches, fm, matches_12, n_matches, used_match);
}

int plslam_kf2kf_match_lines(plslam_ctx* ctx, const plslam_cam* K, const double* DT, const double* sPeP_prev,
                             const uint8_t* desc_prev, int32_t n_prev, const double* seg_curr, const uint8_t* desc_curr,
                             int32_t n_curr, float nnr, int mutual, int32_t min_matches, const plslam_fast_matching* fm,
                             int32_t* matches_12, int32_t* n_matches, int32_t* used_match)
{
    return plslam::kf2kf_driver(ctx, 1, K, DT, sPeP_prev, desc_prev, n_prev, seg_curr, desc_curr, n_curr, nnr, mutual,
                                min_matches, fm, matches_12, n_matches, used_match);
}

int plslam_kf2kf_match_points_dev(plslam_ctx* ctx, const plslam_cam* K, const double* DT, const double* d_P_prev,
                                  const uint8_t* d_desc_prev, int32_t n_prev, const double* pl_curr, const uint8_t* d_desc_curr,
                                  int32_t n_curr, float nnr, int mutual, int32_t min_matches, const plslam_fast_matching* fm,
                                  int32_t* matches_12, int32_t* n_matches, int32_t* used_match)
{
    return plslam::kf2kf_driver(ctx, 0, K, DT, d_P_prev, d_desc_prev, n_prev, pl_curr, d_desc_curr, n_curr, nnr, mutual,
                                min_matches, fm, matches_12, n_matches, used_match, true);
}

int plslam_kf2kf_match_lines_dev(plslam_ctx* ctx, const plslam_cam* K, const double* DT, const double* d_sPeP_prev,
                                 const uint8_t* d_desc_prev, int32_t n_prev, const double* seg_curr, const uint8_t* d_desc_curr,
                                 int32_t n_curr, float nnr, int mutual, int32_t min_matches, const plslam_fast_matching* fm,
                                 int32_t* matches_12, int32_t* n_matches, int32_t* used_match)
{
    return plslam::kf2kf_driver(ctx, 1, K, DT, d_sPeP_prev, d_desc_prev, n_prev, seg_curr, d_desc_curr, n_curr, nnr, mutual,
                                min_matches, fm, matches_12, n_matches, used_match, true);
}

}  // extern "C"
