// match_plan.hpp -- the match plan object (match_plan.hip) as the other translation units of the library see it: the
// host-pointer calls, the pipeline and the gather build and run plans of their own or step a caller's.  Internal.
#pragma once

#include "common.hpp"
#include "match_planner.hpp"

struct plslam_match_plan {
    plslam_ctx* ctx = nullptr;
    int32_t nprob = 0;
    plslam::PlanChoice choice;         // what the planner decided (match_planner.hpp): scan kernels, table family, area sizes
    plslam::PlanTables tab;            // the launch tables it filled; tab.probs is the host image of d_probs (the gate stage patches it)
    bool split_post = false;           // choice.split_post, until a gate applied by the finalize kernel switches it off
    plslam::DevBuf keys, counts, partials;
    plslam::DevBuf rowtmp;             // column-split plans: the per-range row results (merged by the finalize kernel)
    plslam::DevBuf tables;             // all launch tables, packed, uploaded with ONE copy
    std::vector<char> staging;         // host image of `tables` (kept alive: the copy is async)
    plslam::HostBuf staging_pin;       // ... in pinned memory when pin_tables (the context's host-path plan)
    bool pin_tables = false;
    plslam::ScanDesc* d_scans = nullptr; plslam::SymDesc *d_syms = nullptr, *d_dirs = nullptr; plslam::ProblemDesc* d_probs = nullptr;
    plslam::BlockDesc *d_scan_blocks = nullptr, *d_sym_blocks = nullptr, *d_dir_blocks = nullptr, *d_merge_blocks = nullptr, *d_fin_blocks = nullptr;
    int32_t** d_count_dst = nullptr;
    int32_t* d_counts_zero = nullptr;  // contiguous int32 counters zeroed by the first scan kernel
    // optional last stage: the stereo gates over the L<->R tables of the batch (plslam_match_plan_add_stereo_gates)
    plslam::DevBuf gate_tables;
    std::vector<char> gate_staging;
    bool probs_in_place = false;       // d_probs IS the page-locked image
    plslam_stereo_gate_problem* d_gates = nullptr;
    plslam::BlockDesc* d_gate_blocks = nullptr;
    int32_t ngate_blocks = 0, ngates = 0;
    int32_t* d_gate_counts = nullptr;  // contiguous counters of the gate problems (or nullptr)
    bool profiling = false;
    // a run on one stream, captured once and replayed as a HIP graph (latency plans: a few small kernels whose launch
    // overheads are the run; option "graph")
    hipGraphExec_t graph_exec = nullptr;
    bool graph_failed = false;
    void drop_graph() { if (graph_exec) (void)hipGraphExecDestroy(graph_exec); graph_exec = nullptr; graph_failed = false; }
    struct Ev { hipEvent_t e0, e1, e2; };
    std::vector<Ev> evs;
    // split runs (plslam_match_plan_run_split): the scan on one stream, everything behind it on another
    hipEvent_t scan_done = nullptr, post_done = nullptr;
    bool post_pending = false;
    // plslam_match_plan_step_gather: the gather of this plan's table (and the root's widening) is over
    hipEvent_t gather_done = nullptr;
    bool gather_pending = false;
    size_t ev_used = 0;
    double acc_scan_ms = 0, acc_fin_ms = 0;
    int64_t acc_runs = 0;
    void free_all()
    {
        keys.release(); counts.release(); partials.release(); tables.release(); staging_pin.release();
        gate_tables.release(); rowtmp.release();
        for (auto& e : evs) { (void)hipEventDestroy(e.e0); (void)hipEventDestroy(e.e1); (void)hipEventDestroy(e.e2); }
        evs.clear();
        if (scan_done) (void)hipEventDestroy(scan_done);
        if (post_done) (void)hipEventDestroy(post_done);
        if (gather_done) (void)hipEventDestroy(gather_done);
        scan_done = post_done = gather_done = nullptr;
        post_pending = gather_pending = false;
        drop_graph();
    }
};

namespace plslam {

// The device half of a plan: plan_decide, the areas it sized, plan_tables over their addresses, one upload of the packed image
// on the context's stream (no synchronisation).  n1_dev0: see match_problems_on_ctx_stream.
int plan_build(plslam_ctx* ctx, const plslam_match_problem* probs, int32_t nprob, plslam_match_plan* P,
               const int32_t* n1_dev0 = nullptr);
// s: the scan kernel(s); sp: the stages behind them.  sp == s is the plain run.
int plan_run(plslam_match_plan* P, hipStream_t s, hipStream_t sp);

// builds the plan for `probs` (DEVICE pointers) into the context's persistent host-path plan and
// enqueues it on the context stream; no synchronisation.  Caller holds ctx->mu.
// n1_dev0: the row count of problem 0 on the device (probs[0].n1 = its bound); PLSLAM_ENOTSUP when the plan cannot take it
int match_problems_on_ctx_stream(plslam_ctx* ctx, const plslam_match_problem* probs, int32_t nprob, const int32_t* n1_dev0 = nullptr);
// whether the context's options allow the n1_dev0 form at all (asked before anything is staged or enqueued for it)
bool ctx_takes_device_row_count(const plslam_ctx* ctx);
// the loop-closure check's match problems (device pointers) as one plan on the context's stream: ctx->lc_plan, whose
// buffers only grow and whose tables are staged in pageable memory
int match_problems_lc(plslam_ctx* ctx, const plslam_match_problem* probs, int32_t nprob);
// a plan kept by its owner across calls (plslam_lc_batch): (re)built for `probs` (DEVICE pointers) into *slot, its tables
// uploaded on the context's stream without a synchronisation; run on `s`; freed with its buffers
int match_plan_rebuild(plslam_ctx* ctx, plslam_match_plan** slot, const plslam_match_problem* probs, int32_t nprob);
int match_plan_enqueue(plslam_match_plan* plan, hipStream_t s);
void match_plan_release(plslam_match_plan* plan);
}  // namespace plslam
