// match_plan.hip -- the device half of a match plan: plan_decide / plan_tables (match_planner.hpp) say what to launch over
// which tables; plan_build allocates the areas and uploads the packed image, plan_run launches.  The plslam_match_plan_*
// entry points and the plans the library keeps for itself (the context's host-path plan, the loop-closure check's).
#include <string.h>

#include <new>

#include "match_kernels.hpp"   // what plan_run launches; the table shapes the planner is told
#include "match_plan.hpp"

using namespace plslam;

// the plan-relevant options of the context, the CU count and the block-table geometry of the kernels, copied once per plan
static PlanOptions plan_options_of(const plslam_ctx* ctx)
{
    PlanOptions o;
    o.cu_count = ctx->prop.multiProcessorCount;
    o.scan_variant = ctx->scan_variant; o.scan_block = ctx->scan_block; o.sym_rows = ctx->sym_rows; o.group_cap = ctx->group_cap;
    o.mfma_form = ctx->mfma_form; o.col_split = ctx->col_split; o.exact_second = ctx->exact_second;
    o.split_target = ctx->split_target; o.split_min_tiles = ctx->split_min_tiles; o.split_post = ctx->split_post;
    o.post_xcd = ctx->post_xcd; o.post_fuse = ctx->post_fuse; o.fuse = ctx->fuse;
    o.rows_wpq = scan_rows_per_block(PLSLAM_SCAN_WAVE_PER_QUERY, 256);
    o.rows_lpq = scan_rows_per_block(PLSLAM_SCAN_LANE_PER_QUERY, ctx->scan_block ? ctx->scan_block : 256);
    const int lanes[3] = {1, 4, 16};
    for (int k = 0; k < 3; ++k) { o.merge16_cols[k] = merge_partials16_cols(lanes[k]); o.fix16_cols[k] = merge_fix16_cols(lanes[k]); }
    for (int k = 0; k < 2; ++k) { o.sym_block_rows[k] = sym_rows_per_block(lanes[k]); o.sym_partial_rows[k] = sym_rows_per_partial(lanes[k]); }
    return o;
}

// the context-only half of the n1_dev0 test (PlanOptions::takes_device_row_count): callers ask BEFORE they stage or enqueue
// anything for the one-synchronisation form (map2kf.hip)
bool plslam::ctx_takes_device_row_count(const plslam_ctx* ctx) { return plan_options_of(ctx).takes_device_row_count(); }

// plan_decide, the areas it sized, plan_tables over their addresses, one upload of the packed image.
// n1_dev0 (internal; the map<->keyframe driver's one-synchronisation brute-force form): the row count of problem 0 lives on
// the device, probs[0].n1 is its upper bound.  A plan that cannot take it returns PLSLAM_ENOTSUP and the caller takes its
// two-synchronisation form.
int plslam::plan_build(plslam_ctx* ctx, const plslam_match_problem* probs, int32_t nprob,
                       plslam_match_plan* P, const int32_t* n1_dev0)
{
    PlanChoice& c = P->choice;
    PlanTables& t = P->tab;
    P->ctx = ctx;
    P->drop_graph();                   // (a rebuilt plan launches other tables)
    int r = plan_decide(plan_options_of(ctx), probs, nprob, n1_dev0 != nullptr, c);
    if (r) {
        if (c.error) set_last_error("match_planner.hpp: requirement failed: %s", c.error);
        return r;
    }
    P->nprob = nprob;
    P->split_post = c.split_post;

    if ((r = P->keys.reserve(sizeof(uint32_t) * 2 * (size_t)(c.key_rows > 0 ? c.key_rows : 1)))) return r;
    if ((r = P->partials.reserve(sizeof(uint32_t) * 2 * (size_t)(c.part_rows > 0 ? c.part_rows : 1)))) return r;
    if (c.tmp_rows > 0 && (r = P->rowtmp.reserve(sizeof(uint32_t) * 2 * (size_t)c.tmp_rows))) return r;
    if (!c.counts_in_place && (r = P->counts.reserve(sizeof(int32_t) * (size_t)(nprob > 0 ? nprob : 1)))) return r;
    P->d_counts_zero = c.counts_in_place ? probs[0].n_matches : P->counts.as<int32_t>();
    plan_tables(c, probs, {P->keys.as<uint32_t>(), P->partials.as<uint32_t>(), P->rowtmp.as<uint32_t>(), P->d_counts_zero, n1_dev0}, t);

    // every launch table in one host image, uploaded with a single copy
    char* stg = nullptr;
    if (P->pin_tables && t.total <= (size_t(1) << 20)) {
        if ((r = P->staging_pin.reserve(t.total))) return r;
        stg = P->staging_pin.as<char>();
    } else {
        P->staging.resize(t.total);
        stg = P->staging.data();
    }
    for (const PlanTables::Piece& x : t.piece)
        if (x.bytes) memcpy(stg + x.off, x.src, x.bytes);
    // Small plans of the host-pointer path: the kernels read their launch tables (a few hundred bytes per workgroup, once)
    // straight from the page-locked image -- one copy-engine command less in front of the first kernel.  (Those callers
    // synchronise the stream before the context builds its next plan, so the image is not rewritten under a kernel.)
    char* base = nullptr;
    if (stg == P->staging_pin.p && t.total <= (size_t(1) << 14)) base = static_cast<char*>(mapped_device_pointer(stg));
    P->probs_in_place = base != nullptr;
    if (!base) {
        if ((r = P->tables.reserve(t.total))) return r;
        base = P->tables.as<char>();
    }
    auto at = [&](int k) { return base + t.piece[k].off; };
    P->d_scans = reinterpret_cast<ScanDesc*>(at(PlanTables::SCANS));
    P->d_syms = reinterpret_cast<SymDesc*>(at(PlanTables::SYMS));
    P->d_probs = reinterpret_cast<ProblemDesc*>(at(PlanTables::PROBS));
    P->d_scan_blocks = reinterpret_cast<BlockDesc*>(at(PlanTables::SCAN_BLOCKS));
    P->d_sym_blocks = reinterpret_cast<BlockDesc*>(at(PlanTables::SYM_BLOCKS));
    P->d_merge_blocks = reinterpret_cast<BlockDesc*>(at(PlanTables::MERGE_BLOCKS));
    P->d_fin_blocks = reinterpret_cast<BlockDesc*>(at(PlanTables::FIN_BLOCKS));
    P->d_count_dst = reinterpret_cast<int32_t**>(at(PlanTables::COUNT_DST));
    P->d_dirs = reinterpret_cast<SymDesc*>(at(PlanTables::DIRS));
    P->d_dir_blocks = reinterpret_cast<BlockDesc*>(at(PlanTables::DIR_BLOCKS));
    P->ngate_blocks = 0;                 // a rebuilt plan (the context's host-path plan) starts without a gate stage
    P->ngates = 0;

    // P->staging outlives the copy (it is a member), so no synchronisation is needed here; the
    // copy is ordered before the kernels of plan_run when they use the same stream, and the public
    // plan_create synchronises once so that any stream may be used afterwards.
    if (!P->probs_in_place) PLSLAM_HIP_CHECK(hipMemcpyAsync(base, stg, t.total, hipMemcpyHostToDevice, ctx->stream));
    return PLSLAM_OK;
}

// s: the scan kernel(s); sp: the stages behind them (merge of the column partials, finalize, gates, count scatter).  sp == s
// is the plain run.  With two streams the stages behind the scan of one run overlap the scan of the NEXT run on `s` (another
// plan, or this one: its next scan waits for this run's last stage, which reads what that scan overwrites): the scan is
// bound by instruction issue, the stages behind it by HBM, and a workgroup slot the scan frees is taken by either.
int plslam::plan_run(plslam_match_plan* P, hipStream_t s, hipStream_t sp)
{
    const bool split = sp != s;
    if (split) {
        if (!P->scan_done) PLSLAM_HIP_CHECK(hipEventCreateWithFlags(&P->scan_done, hipEventDisableTiming));
        if (!P->post_done) PLSLAM_HIP_CHECK(hipEventCreateWithFlags(&P->post_done, hipEventDisableTiming));
    }
    if (P->post_pending) {            // an earlier split run: its last stage must be over before this scan rewrites its input
        PLSLAM_HIP_CHECK(hipStreamWaitEvent(s, P->post_done, 0));
        P->post_pending = false;
    }
    plslam_match_plan::Ev* ev = nullptr;
    if (P->profiling) {
        if (P->ev_used == P->evs.size()) {
            plslam_match_plan::Ev e{};
            PLSLAM_HIP_CHECK(hipEventCreate(&e.e0));
            PLSLAM_HIP_CHECK(hipEventCreate(&e.e1));
            PLSLAM_HIP_CHECK(hipEventCreate(&e.e2));
            P->evs.push_back(e);
        }
        ev = &P->evs[P->ev_used++];
        PLSLAM_HIP_CHECK(hipEventRecord(ev->e0, s));
    }
    const PlanChoice& c = P->choice;
    const PlanTables& t = P->tab;
    const int nsym_blocks = (int)t.sym_blocks.size(), ndir_blocks = (int)t.dir_blocks.size(), nscan_blocks = (int)t.scan_blocks.size();
    const int nmerge_blocks = (int)t.merge_blocks.size();
    int r;
    bool zeroed = false;               // the first scan kernel that runs zeroes the #matches counters
    if (c.fused) {
        // fused problems STORE their counts from inside the scan kernel, so the counters cannot be zeroed by that kernel's
        // first workgroup: clear them ahead of it (only problems without rows or columns keep the zero)
        PLSLAM_HIP_CHECK(hipMemsetAsync(P->d_counts_zero, 0, sizeof(int32_t) * (size_t)P->nprob, s));
        zeroed = true;
    }
    if (nsym_blocks > 0) {
        r = c.sym_mfma ? launch_scan_mfma_form(c.mfma_form, P->d_syms, P->d_sym_blocks, nsym_blocks, P->d_counts_zero,
                                               zeroed ? 0 : P->nprob, t.sym_mfma_multi, false, s, c.fused)
                       : launch_scan_sym(c.sym_rows, P->d_syms, P->d_sym_blocks, nsym_blocks, P->d_counts_zero, P->nprob, s);
        if (r) return r;
        zeroed = true;
    }
    if (ndir_blocks > 0) {
        r = launch_scan_mfma_form(c.mfma_form, P->d_dirs, P->d_dir_blocks, ndir_blocks, P->d_counts_zero,
                                  zeroed ? 0 : P->nprob, t.dir_multi, true, s, c.fused);
        if (r) return r;
        zeroed = true;
    }
    if (nscan_blocks > 0 || !zeroed) {
        r = launch_scan(P->ctx, c.scan_variant, c.block_threads, P->d_scans, P->d_scan_blocks, nscan_blocks, P->d_counts_zero,
                        zeroed ? 0 : P->nprob, s);
        if (r) return r;
    }
    if (ev) PLSLAM_HIP_CHECK(hipEventRecord(ev->e1, s));   // e0..e1 = the scan kernel(s) alone
    if (split) {
        PLSLAM_HIP_CHECK(hipEventRecord(P->scan_done, s));
        PLSLAM_HIP_CHECK(hipStreamWaitEvent(sp, P->scan_done, 0));
        s = sp;
    }

    if (P->split_post) {
        r = launch_split_post(P->d_syms, P->d_merge_blocks, nmerge_blocks, c.merge_parts, P->d_probs, s);
        if (r) return r;
    } else if (t.post_fused) {
        if (P->ngates > 0 && P->d_gate_counts) PLSLAM_HIP_CHECK(hipMemsetAsync(P->d_gate_counts, 0, sizeof(int32_t) * (size_t)P->ngates, s));
        r = launch_post_fused(P->d_probs, P->nprob, P->ngates > 0 ? P->d_gates : nullptr, t.post_lds, s);
        if (r) return r;
    } else {
        const int grid_cap = split ? P->ctx->post_workgroups : 0;
        r = c.h_tables()     ? launch_merge_fix16(P->d_syms, P->d_merge_blocks, nmerge_blocks, c.merge_parts, c.exact_second, s, grid_cap)
            : c.partials16() ? launch_merge_partials16(P->d_syms, P->d_merge_blocks, nmerge_blocks, c.merge_parts, s)
                             : launch_merge_partials(P->d_syms, P->d_merge_blocks, nmerge_blocks, s);
        if (r) return r;
        // the gate stage: its counters are cleared first; gates over the plan's own tables run inside the finalize kernel
        if (P->ngates > 0 && P->d_gate_counts) PLSLAM_HIP_CHECK(hipMemsetAsync(P->d_gate_counts, 0, sizeof(int32_t) * (size_t)P->ngates, s));
        r = launch_finalize(P->d_probs, P->d_fin_blocks, (int)t.fin_blocks.size(), P->ngates > 0 ? P->d_gates : nullptr, s, grid_cap,
                            P->ctx->post_xcd == 1, t.fin_row);
        if (r) return r;
    }
    if (P->ngate_blocks > 0) {
        r = launch_stereo_gates(P->d_gates, P->d_gate_blocks, P->ngate_blocks, s);
        if (r) return r;
    }
    if (ev) PLSLAM_HIP_CHECK(hipEventRecord(ev->e2, s));
    if (c.scatter_counts && (r = launch_scatter_counts(P->d_counts_zero, P->d_count_dst, P->nprob, s))) return r;
    if (split) {
        PLSLAM_HIP_CHECK(hipEventRecord(P->post_done, s));
        P->post_pending = true;
    }
    return PLSLAM_OK;
}

namespace plslam {
int match_problems_on_ctx_stream(plslam_ctx* ctx, const plslam_match_problem* probs, int32_t nprob, const int32_t* n1_dev0)
{
    if (!ctx->host_plan) ctx->host_plan = new (std::nothrow) plslam_match_plan();
    PLSLAM_REQUIRE(ctx->host_plan != nullptr, PLSLAM_ENOMEM);
    const int r = plan_build(ctx, probs, nprob, ctx->host_plan, n1_dev0);
    if (r == PLSLAM_ENOTSUP && n1_dev0) return r;            // (not an error: the caller has another form; no message)
    return r ? r : plan_run(ctx->host_plan, ctx->stream, ctx->stream);
}

int match_problems_lc(plslam_ctx* ctx, const plslam_match_problem* probs, int32_t nprob)
{
    if (!ctx->lc_plan) ctx->lc_plan = new (std::nothrow) plslam_match_plan();
    PLSLAM_REQUIRE(ctx->lc_plan != nullptr, PLSLAM_ENOMEM);
    const int r = plan_build(ctx, probs, nprob, ctx->lc_plan);
    return r ? r : plan_run(ctx->lc_plan, ctx->stream, ctx->stream);
}

int match_plan_rebuild(plslam_ctx* ctx, plslam_match_plan** slot, const plslam_match_problem* probs, int32_t nprob)
{
    if (!*slot) *slot = new (std::nothrow) plslam_match_plan();
    PLSLAM_REQUIRE(*slot != nullptr, PLSLAM_ENOMEM);
    return plan_build(ctx, probs, nprob, *slot);
}

int match_plan_enqueue(plslam_match_plan* plan, hipStream_t s) { return plan_run(plan, s, s); }

void match_plan_release(plslam_match_plan* plan)
{
    if (!plan) return;
    plan->free_all();
    delete plan;
}
}  // namespace plslam

extern "C" {

// ---- plans ----------------------------------------------------------------------------------
int plslam_match_plan_create(plslam_ctx* ctx, const plslam_match_problem* probs, int32_t nprob,
                             plslam_match_plan** out)
{
    PLSLAM_REQUIRE(ctx && out, PLSLAM_EINVAL);
    *out = nullptr;
    DeviceGuard g(ctx->device);
    plslam_match_plan* P = new (std::nothrow) plslam_match_plan();
    PLSLAM_REQUIRE(P != nullptr, PLSLAM_ENOMEM);
    int r = plan_build(ctx, probs, nprob, P);
    if (!r && hipStreamSynchronize(ctx->stream) != hipSuccess) {
        set_last_error("hipStreamSynchronize failed after the plan upload");
        r = PLSLAM_EHIP;
    }
    if (r) {
        P->free_all();
        delete P;
        return r;
    }
    *out = P;
    return PLSLAM_OK;
}

int plslam_match_plan_add_stereo_gates(plslam_match_plan* plan, const plslam_stereo_gate_problem* gates, int32_t ngates)
{
    PLSLAM_REQUIRE(plan != nullptr && ngates >= 0 && (ngates == 0 || gates != nullptr), PLSLAM_EINVAL);
    DeviceGuard g(plan->ctx->device);
    // ---- validation first: nothing of the plan is touched until the whole request is known to be good -----------------
    // a gate whose input table is the matches_12 of one of the plan's problems (the usual case: the L<->R tables of the
    // batch) is applied by the finalize kernel itself, row by row, the moment the entry is decided (ProblemDesc::gate);
    // any other gate -- and every gate of a fused plan, which has no finalize kernel -- keeps its own workgroups
    std::vector<BlockDesc> blocks;
    std::vector<int32_t> gate_of(plan->tab.probs.size(), -1);
    bool any_cnt = false, all_cnt = true;
    for (int32_t i = 0; i < ngates; ++i) {
        const int rc = check_stereo_gate_problem(gates[i]);
        if (rc) return rc;
        any_cnt = any_cnt || gates[i].n_stereo != nullptr;
        all_cnt = all_cnt && gates[i].n_stereo != nullptr && gates[i].n_stereo == gates[0].n_stereo + i;
        bool in_finalize = false;
        if (!plan->choice.fused && gates[i].n_l > 0)
            for (size_t k = 0; k < plan->tab.probs.size(); ++k) {
                const ProblemDesc& pd = plan->tab.probs[k];
                if (pd.matches_12 == gates[i].matches_12 && pd.n1 == gates[i].n_l && gate_of[k] < 0) {
                    gate_of[k] = i;
                    in_finalize = true;
                    break;
                }
            }
        if (!in_finalize)
            for (int32_t r0 = 0; r0 < gates[i].n_l; r0 += 256) blocks.push_back({i, r0});
    }
    PLSLAM_REQUIRE(!any_cnt || all_cnt, PLSLAM_EINVAL);     // counters: none, or one contiguous array
    // ---- the stage is replaced: its tables and the problem table (ProblemDesc::gate) are rewritten under whatever run is
    // still in flight on whatever stream the caller used -- the call is rare, so it simply waits for the device ------------
    PLSLAM_HIP_CHECK(hipDeviceSynchronize());
    if (plan->graph_exec) plan->drop_graph();               // the captured run has another gate stage
    // from here on every exit leaves the plan consistent: first the state "no gate stage" (host image AND device table) ...
    plan->ngate_blocks = 0;
    plan->ngates = 0;
    plan->d_gate_counts = nullptr;
    plan->d_gates = nullptr;
    plan->split_post = plan->choice.split_post;
    auto upload_probs = [&]() -> int {
        if (plan->tab.probs.empty()) return PLSLAM_OK;
        PLSLAM_HIP_CHECK(hipMemcpyAsync(plan->d_probs, plan->tab.probs.data(), plan->tab.probs.size() * sizeof(ProblemDesc),
                                        plan->probs_in_place ? hipMemcpyHostToHost : hipMemcpyHostToDevice, plan->ctx->stream));
        PLSLAM_HIP_CHECK(hipStreamSynchronize(plan->ctx->stream));
        return PLSLAM_OK;
    };
    bool had = false;
    for (ProblemDesc& pd : plan->tab.probs) { had = had || pd.gate >= 0; pd.gate = -1; }
    if (had) { const int rc = upload_probs(); if (rc) return rc; }
    if (ngates == 0) return PLSLAM_OK;
    // ... then the new stage: its tables first (a failed allocation returns with the consistent "no gate stage" above) ...
    const size_t gbytes = align256((size_t)ngates * sizeof(plslam_stereo_gate_problem));
    const size_t total = gbytes + blocks.size() * sizeof(BlockDesc) + 256;
    plan->gate_staging.assign(total, 0);
    memcpy(plan->gate_staging.data(), gates, (size_t)ngates * sizeof(plslam_stereo_gate_problem));
    if (!blocks.empty()) memcpy(plan->gate_staging.data() + gbytes, blocks.data(), blocks.size() * sizeof(BlockDesc));
    int r = plan->gate_tables.reserve(total);
    if (r) return r;
    PLSLAM_HIP_CHECK(hipMemcpyAsync(plan->gate_tables.p, plan->gate_staging.data(), total, hipMemcpyHostToDevice,
                                    plan->ctx->stream));
    PLSLAM_HIP_CHECK(hipStreamSynchronize(plan->ctx->stream));
    // ... and, last, the gate indices of the problem table together with the counters that make a run use them: a failure of
    // the upload puts the indices back (the device table then still holds -1 everywhere or is rewritten in full next time)
    for (size_t k = 0; k < plan->tab.probs.size(); ++k) plan->tab.probs[k].gate = gate_of[k];
    r = upload_probs();
    if (r) {
        for (ProblemDesc& pd : plan->tab.probs) pd.gate = -1;
        (void)upload_probs();
        return r;
    }
    plan->d_gates = plan->gate_tables.as<plslam_stereo_gate_problem>();
    plan->d_gate_blocks = reinterpret_cast<BlockDesc*>(plan->gate_tables.as<char>() + gbytes);
    plan->ngate_blocks = (int32_t)blocks.size();
    plan->ngates = ngates;
    plan->d_gate_counts = any_cnt ? gates[0].n_stereo : nullptr;
    for (int32_t gk : gate_of)
        if (gk >= 0) plan->split_post = false;              // the finalize kernel applies that gate: merge + finalize it is
    return PLSLAM_OK;
}

int plslam_match_plan_set_wire16(plslam_match_plan* plan, const int32_t* table32, int16_t* table16, size_t n_entries)
{
    PLSLAM_REQUIRE(plan != nullptr && (table16 == nullptr || table32 != nullptr), PLSLAM_EINVAL);
    DeviceGuard g(plan->ctx->device);
    // only the finalize kernel (k_finalize / k_post_fused: finalize_row) stores the mirror: a fused plan decides its entries in
    // the scan kernel, a column-split plan in k_split_post
    if (table16 && (plan->choice.fused || plan->choice.col_split)) {
        set_last_error("plslam_match_plan_set_wire16: this plan's tables are not written by the finalize kernel");
        return PLSLAM_ENOTSUP;
    }
    std::vector<int16_t*> mirror(plan->tab.probs.size(), nullptr);
    if (table16)
        for (size_t k = 0; k < plan->tab.probs.size(); ++k) {
            const ProblemDesc& pd = plan->tab.probs[k];
            if (pd.n1 <= 0 || pd.matches_12 < table32 || pd.matches_12 >= table32 + n_entries) continue;
            PLSLAM_REQUIRE((size_t)(pd.matches_12 - table32) + (size_t)pd.n1 <= n_entries, PLSLAM_EINVAL);
            PLSLAM_REQUIRE(pd.n2 <= 32768, PLSLAM_EINVAL);
            // a kept prior entry of a NON-mutual problem reaches the table unchecked (upstream's resize(); a mutual problem
            // clears whatever lies outside [0, n2)): it could be any int32 and would wrap in the mirror
            if (pd.keep_prior && !pd.mutual) {
                set_last_error("plslam_match_plan_set_wire16: problem %zu keeps prior entries without the mutual check (unbounded values)", k);
                return PLSLAM_ENOTSUP;
            }
            mirror[k] = table16 + (pd.matches_12 - table32);
        }
    PLSLAM_HIP_CHECK(hipDeviceSynchronize());               // (as add_stereo_gates: rare, so it waits for whatever is in flight)
    if (plan->graph_exec) plan->drop_graph();
    for (size_t k = 0; k < plan->tab.probs.size(); ++k) plan->tab.probs[k].matches_16 = mirror[k];
    if (!plan->tab.probs.empty()) {
        PLSLAM_HIP_CHECK(hipMemcpyAsync(plan->d_probs, plan->tab.probs.data(), plan->tab.probs.size() * sizeof(ProblemDesc),
                                        plan->probs_in_place ? hipMemcpyHostToHost : hipMemcpyHostToDevice, plan->ctx->stream));
        PLSLAM_HIP_CHECK(hipStreamSynchronize(plan->ctx->stream));
    }
    return PLSLAM_OK;
}

int plslam_match_plan_run(plslam_match_plan* plan, void* stream)
{
    PLSLAM_REQUIRE(plan != nullptr, PLSLAM_EINVAL);
    DeviceGuard g(plan->ctx->device);
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : plan->ctx->stream;
    // Graph replay (option "graph": 0 = plans of fewer waves than the chip has SIMDs, 1 = never, 2 = always): the run's
    // launches are captured once on the caller's stream and replayed with one hipGraphLaunch.  Not while profiling (the
    // events belong to the run), not for a plan with a split run pending (its ordering event is not part of the graph).
    const int gopt = plan->ctx->graph;
    if (gopt != 1 && (gopt == 2 || plan->choice.small) && !plan->profiling && !plan->post_pending && !plan->graph_failed) {
        if (!plan->graph_exec) {
            hipGraph_t gr = nullptr;
            if (hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal) == hipSuccess) {
                const int r = plan_run(plan, s, s);
                const hipError_t e = hipStreamEndCapture(s, &gr);
                if (r == PLSLAM_OK && e == hipSuccess && gr && hipGraphInstantiate(&plan->graph_exec, gr, nullptr, nullptr, 0) != hipSuccess)
                    plan->graph_exec = nullptr;
                if (gr) (void)hipGraphDestroy(gr);
            }
            (void)hipGetLastError();
            if (!plan->graph_exec) plan->graph_failed = true;       // (this device / runtime cannot: plain launches from now on)
        }
        if (plan->graph_exec) {
            PLSLAM_HIP_CHECK(hipGraphLaunch(plan->graph_exec, s));
            return PLSLAM_OK;
        }
    }
    return plan_run(plan, s, s);
}

int plslam_match_plan_run_split(plslam_match_plan* plan, void* scan_stream, void* post_stream)
{
    PLSLAM_REQUIRE(plan != nullptr, PLSLAM_EINVAL);
    DeviceGuard g(plan->ctx->device);
    hipStream_t s = scan_stream ? static_cast<hipStream_t>(scan_stream) : plan->ctx->stream;
    // A fused plan (option "fuse" = 2) writes matches_12 and the counts from inside its scan kernel: there is no stage behind
    // the scan whose completion could order the caller's consumers against the plan's NEXT scan, so such a plan is not
    // split -- everything goes to the scan stream, where stream order does it.
    if (plan->choice.fused) return plan_run(plan, s, s);
    return plan_run(plan, s, post_stream ? static_cast<hipStream_t>(post_stream) : s);
}

int plslam_match_plan_set_profiling(plslam_match_plan* plan, int enable)
{
    PLSLAM_REQUIRE(plan != nullptr, PLSLAM_EINVAL);
    plan->profiling = enable != 0;
    return PLSLAM_OK;
}

int plslam_match_plan_elapsed(plslam_match_plan* plan, double* scan_ms, double* finalize_ms,
                              int64_t* runs)
{
    PLSLAM_REQUIRE(plan != nullptr, PLSLAM_EINVAL);
    DeviceGuard g(plan->ctx->device);
    for (size_t i = 0; i < plan->ev_used; ++i) {
        auto& e = plan->evs[i];
        PLSLAM_HIP_CHECK(hipEventSynchronize(e.e2));
        float a = 0.f, b = 0.f;
        PLSLAM_HIP_CHECK(hipEventElapsedTime(&a, e.e0, e.e1));
        PLSLAM_HIP_CHECK(hipEventElapsedTime(&b, e.e1, e.e2));
        plan->acc_scan_ms += a;
        plan->acc_fin_ms += b;
        plan->acc_runs += 1;
    }
    plan->ev_used = 0;
    if (scan_ms) *scan_ms = plan->acc_scan_ms;
    if (finalize_ms) *finalize_ms = plan->acc_fin_ms;
    if (runs) *runs = plan->acc_runs;
    plan->acc_scan_ms = plan->acc_fin_ms = 0;
    plan->acc_runs = 0;
    return PLSLAM_OK;
}

int plslam_match_plan_info(plslam_match_plan* plan, plslam_plan_info* info)
{
    PLSLAM_REQUIRE(plan && info, PLSLAM_EINVAL);
    *info = plan->tab.info;
    return PLSLAM_OK;
}

// diagnostics: raw copies of a plan's key table and the symmetric scan's column partials (see the header)
int plslam_match_plan_dump(plslam_match_plan* plan, void* keys_out, size_t keys_cap, void* part_out, size_t part_cap,
                           size_t* keys_bytes, size_t* part_bytes)
{
    if (!plan || !keys_bytes || !part_bytes) return PLSLAM_EINVAL;
    DeviceGuard g(plan->ctx->device);
    (void)hipDeviceSynchronize();
    if (plan->split_post) {            // the two-launch form leaves the rows' merged pairs unwritten: complete them here
        (void)launch_split_rows_dump(plan->d_probs, plan->d_fin_blocks, (int)plan->tab.fin_blocks.size(), plan->ctx->stream);
        (void)hipDeviceSynchronize();
    }
    *keys_bytes = plan->keys.cap;
    *part_bytes = plan->partials.cap;
    if (keys_out && keys_cap >= plan->keys.cap && plan->keys.p) (void)hipMemcpy(keys_out, plan->keys.p, plan->keys.cap, hipMemcpyDeviceToHost);
    if (part_out && part_cap >= plan->partials.cap && plan->partials.p) (void)hipMemcpy(part_out, plan->partials.p, plan->partials.cap, hipMemcpyDeviceToHost);
    return PLSLAM_OK;
}

void plslam_match_plan_destroy(plslam_match_plan* plan)
{
    if (!plan) return;
    DeviceGuard g(plan->ctx->device);
    (void)hipDeviceSynchronize();
    plan->free_all();
    delete plan;
}

int plslam_match_plan_key_state(plslam_match_plan* plan, int32_t* flags)
{
    if (!plan || !flags) return PLSLAM_EINVAL;
    *flags = (plan->choice.lazy_keys() ? PLSLAM_KEYS_ROW_SECOND_INDEX_INEXACT | PLSLAM_KEYS_COLUMN_SECOND_LAZY : 0) |
             (plan->tab.post_fused ? PLSLAM_KEYS_COLUMNS_NOT_IN_MEMORY : 0);
    return PLSLAM_OK;
}

}  // extern "C"
