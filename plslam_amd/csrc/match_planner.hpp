// match_planner.hpp -- the host half of a match plan that needs no device: which scan every problem takes, how large the
// key / partial / row-temp areas are (plan_decide), and the launch tables over given base addresses (plan_tables).
// Standard library only: arithmetic on (options, CU count, problem shapes), so tests/cpp/test_match_planner.cpp runs it
// without a GPU.  match_plan.hip (plan_build) allocates between the two calls and uploads the packed image.
#pragma once

#include <algorithm>
#include <vector>

#include "match_tables.hpp"

namespace plslam {

// the plan-relevant context options (plslam_ctx_set_option; meanings in plslam_hip.h) and facts of the device and the kernels
struct PlanOptions {
    int cu_count = 0;
    int scan_variant = PLSLAM_SCAN_AUTO, scan_block = 0, sym_rows = 0, group_cap = 0, mfma_form = 0, col_split = 0, exact_second = 0;
    int split_target = 0, split_min_tiles = 0, split_post = 0, post_xcd = 2, post_fuse = 0, fuse = 0;
    // rows / column slots one block-table entry stands for, as the kernels' translation units report them:
    int rows_wpq = 0, rows_lpq = 0;             // scan_rows_per_block(wave per query, 256) / (lane per query, scan_block or 256)
    int sym_block_rows[2] = {0, 0};             // sym_rows_per_block(1), (4)
    int sym_partial_rows[2] = {0, 0};           // sym_rows_per_partial(1), (4)
    int merge16_cols[3] = {0, 0, 0};            // merge_partials16_cols(1), (4), (16)
    int fix16_cols[3] = {0, 0, 0};              // merge_fix16_cols(1), (4), (16)

    // the row count of problem 0 may live on the device (n1_dev0): only as a two-launch column-split plan of ONE mutual
    // problem (K1f + k_split_post, which read the count themselves) -- these are the options such a plan cannot honour
    bool takes_device_row_count() const
    {
        return (scan_variant == PLSLAM_SCAN_AUTO || scan_variant == PLSLAM_SCAN_MFMA) && (mfma_form == 0 || mfma_form == 2) &&
               col_split != 1 && split_post != 1 && fuse != 2;
    }
};

enum class ProblemPath : int32_t {
    empty,      // no rows: nothing is scanned (the finalize kernel has no block of it either)
    scan,       // directed scan(s) on the popcount kernels: d1 -> d2, and d2 -> d1 when mutual (lane or wave per query)
    sym,        // one symmetric scan feeds both directions (XOR + popcount, or the matrix cores)
    directed,   // the directed form of the matrix-core scan (non-mutual; mfma_form 3: both directions of a mutual problem)
    split,      // matrix-core scan with the columns cut into `nsplit` ranges of `cstep`, each a sub-problem
};

struct ProblemPlan {
    ProblemPath path;
    int32_t nsplit, cstep;                      // path split only (else 1, 0)
    int64_t key_row, part_row, tmp_row;         // where the problem's slices of the three areas start, in units of two words
};

struct PlanChoice {
    PlanOptions opts;
    const char* error = nullptr;                // the requirement that failed (plan_decide returned EINVAL / ERANGE)
    bool small = false;                         // fewer waves than the chip has SIMDs
    int scan_variant = 0, block_threads = 0;    // the directed popcount scan: lane or wave per query
    int rows_scan = 0;                          // ... its rows per block-table entry
    bool sym_mfma = false;                      // symmetric / directed problems run on the matrix cores
    bool dpair = false;                         // mfma_form 3: a mutual problem is TWO directed matrix-core scans, no column direction
    int mfma_form = 0;                          // option "mfma_form"; AUTO (0 = K1i) becomes 2 (K1f) for a column-split plan
    int sym_rows = 1;                           // rows of d1 per lane of the XOR symmetric scan (the matrix cores: its 256-row tables)
    int rows_sym = 0, rows_partial = 0;         // a-rows per workgroup / per column partial of the symmetric scan
    bool fused = false;                         // K1f, one workgroup per problem: merge + ratio + mutual inside the scan kernel
    bool col_split = false;                     // K1f on a FEW LARGE problems: columns cut into ranges scanned as sub-problems
    bool split_post = false;                    // ... and everything behind the scan in ONE kernel (k_split_post): two launches
    bool exact_second = false;                  // K1h / K1i: exact key tables; else the finalize kernel completes keys21 lazily
    int merge_parts = 1;                        // lanes per column in the partial merge (tall problems: many row blocks, few columns)
    int merge_cols = 0;                         // column slots per entry of the merge kernel's block table
    size_t group_cap = 2;                       // blocks of one problem kept together on one XCD
    int64_t key_rows = 0, part_rows = 0, tmp_rows = 0;   // the three areas, in units of two words
    // #matches counters: accumulated with atomics by the finalize kernel, zeroed by the scan kernel.  The callers' n_matches
    // pointers form one contiguous array: count in place; else in an array of the plan, scattered to whoever gave a pointer
    bool counts_in_place = false, scatter_counts = false;
    std::vector<ProblemPlan> per;               // one per problem

    // THE place where the table family is decided.  K1h's tables (K1h and K1i, what AUTO takes for throughput plans): one
    // column partial word per (256-row block, column slot), merged by launch_merge_fix16.  Else, every matrix-core form but
    // K1e (K1f, which AUTO takes for column-split plans; K1g): 16-bit partials per (64-row block, column slot).
    bool h_tables() const { return sym_mfma && mfma_form_is_h(mfma_form) && !fused; }
    bool partials16() const { return sym_mfma && mfma_form != 1; }
    bool lazy_keys() const { return h_tables() && !exact_second; }      // (plslam_match_plan_key_state)
    // column partials of an n1 x n2 (sub-)problem on the matrix cores, rows padded to 256 slots
    int64_t part_units(int32_t n1, int32_t n2) const
    {
        if (h_tables()) return (int64_t)((n1 + 255) / 256) * ((n2 + 255) / 256) * (exact_second ? 256 : 128);
        return (int64_t)((n1 + 63) / 64) * ((n2 + 255) / 256) * 128;
    }
};

#define PLSLAM_PLAN_REQUIRE(cond, code)   \
    do {                                  \
        if (!(cond)) {                    \
            c.error = #cond;              \
            return (code);                \
        }                                 \
    } while (0)

// Validates the problems and decides.  PLSLAM_ENOTSUP (no message): has_n1_dev0 and the plan cannot take a device row count.
inline int plan_decide(const PlanOptions& o, const plslam_match_problem* probs, int32_t nprob, bool has_n1_dev0, PlanChoice& c)
{
    c.error = nullptr;
    c.per.clear();
    c.opts = o;
    PLSLAM_PLAN_REQUIRE(nprob >= 0, PLSLAM_EINVAL);
    PLSLAM_PLAN_REQUIRE(nprob == 0 || probs != nullptr, PLSLAM_EINVAL);
    const bool variant_auto = o.scan_variant == PLSLAM_SCAN_AUTO;
    const bool variant_mfma = variant_auto || o.scan_variant == PLSLAM_SCAN_MFMA;

    // AUTO: mutual problems take the symmetric scan (one distance feeds both directions) on the matrix cores (K1i), the others
    // its directed form (row direction only).  A forced variant applies to every problem (SYMMETRIC = the XOR + popcount form).
    // A plan too small to put one wave on every SIMD under those (e.g. ONE StVO::match call of the SLAM loop) takes the
    // wave-per-query scan instead: 16 queries per workgroup, train tile in LDS.
    // A plan of a FEW LARGE problems (C3: one local map against one frame, 10 000 x 1500 + 2 000 x 200, mapHandler.cpp:532-752)
    // has too few 256-row blocks to fill the chip, but far too much work for the latency kernel (50 us there): the
    // matrix-core scan takes it with the COLUMNS cut into ranges, one workgroup per (row block, range).
    int64_t thr_waves = 0;      // waves the throughput kernels would launch: one per 64 rows of d1
    int64_t sym_evals = 0, mf_row_blocks = 0;
    for (int32_t i = 0; i < nprob; ++i) {
        thr_waves += (probs[i].n1 + 63) / 64;
        if (probs[i].n1 > 0 && probs[i].n2 > 0) {
            sym_evals += (int64_t)probs[i].n1 * probs[i].n2;
            mf_row_blocks += (probs[i].n1 + 255) / 256;
        }
    }
    c.small = thr_waves < (int64_t)o.cu_count * 4;
    const bool split_auto = variant_auto && c.small && sym_evals >= (int64_t(6) << 20) && o.mfma_form != 1;
    const bool split_forced = o.col_split == 2 && o.mfma_form != 1 && variant_mfma;
    bool col_split = o.col_split != 1 && (split_auto || split_forced);
    if (has_n1_dev0) {
        const bool can = nprob == 1 && probs[0].mutual && !probs[0].keep_prior && probs[0].n1 > 0 && probs[0].n2 > 0 &&
                         o.takes_device_row_count();
        if (!can) return PLSLAM_ENOTSUP;
        col_split = true;
    }
    const bool use_wpq = o.scan_variant == PLSLAM_SCAN_WAVE_PER_QUERY || (variant_auto && c.small && !col_split);
    const bool allow_sym = !use_wpq && (variant_mfma || o.scan_variant == PLSLAM_SCAN_SYMMETRIC);
    c.dpair = allow_sym && o.mfma_form == 3 && variant_mfma;
    c.sym_mfma = allow_sym && variant_mfma;
    auto is_sym = [&](const plslam_match_problem& p) { return allow_sym && !c.dpair && p.mutual && p.n1 > 0 && p.n2 > 0; };

    // sym_rows 0 = auto: 4 rows of d1 per lane (4x fewer column partials, slightly faster) once the
    // plan has enough 256-row waves for >= 6 full rounds of the chip (17 single-wave workgroups fit a
    // CU's LDS); below that the 4x coarser work units lose more to tail quantisation than they gain
    // (measured: 266k vs 320k pairs/s at 512 pairs, 347k vs 344k at 2048, 364k vs 347k at 4096).
    c.sym_rows = c.sym_mfma ? 4 : o.sym_rows;      // the matrix-core scans use the 256-row tables of K1b'
    if (c.sym_rows == 0) {
        int64_t waves4 = 0;
        for (int32_t i = 0; i < nprob; ++i)
            if (is_sym(probs[i])) waves4 += (probs[i].n1 + 255) / 256;
        c.sym_rows = waves4 >= 6 * 17 * (int64_t)o.cu_count ? 4 : 1;
    }
    c.rows_partial = o.sym_partial_rows[c.sym_rows == 4];
    c.rows_sym = o.sym_block_rows[c.sym_rows == 4];
    c.mfma_form = o.mfma_form;
    c.exact_second = o.exact_second != 0;
    // Fused form (K1f only): one workgroup per problem walks all row blocks and finishes the problem (column merge, ratio
    // test, mutual check, count) -- ONE kernel per plan run, no merge / finalize kernels, no keys21 round trip.  Measured
    // at C2 / 4096 pairs per step: 4.05 ms against 3.48 + 0.52 ms unfused -- the merge's VALU work (+5 %), which the
    // separate merge kernel hides under its HBM time, and the serial tail of every workgroup cost what the two launches
    // cost -- so AUTO does not select it; "fuse" = 2 does (it needs many more problems than the chip has workgroup slots,
    // 3 per CU, or the 6x coarser work units lose to tail quantisation).  Mutual problems keep their merged column keys in
    // LDS: n2 <= PLSLAM_K1F_FUSED_MAX_N2.
    bool fits = true;
    for (int32_t i = 0; i < nprob; ++i) {
        if (probs[i].n1 <= 0 || probs[i].n2 <= 0) continue;
        if (probs[i].mutual && probs[i].n2 > PLSLAM_K1F_FUSED_MAX_N2) fits = false;
        if (probs[i].keep_prior) fits = false;          // the in-kernel finalize always writes every row
    }
    c.fused = c.partials16() && fits && o.fuse == 2 && !col_split && !c.dpair;
    c.col_split = col_split && c.partials16() && mf_row_blocks > 0 && !c.dpair;
    // AUTO form: K1i for throughput plans; a column-split plan (a few large problems, e.g. C3's one map against one frame) is
    // latency-bound -- 4-5 tiles per workgroup -- and K1f's lighter per-workgroup prologue / row finish wins there
    // (measured at C3: 22.4 us per run against 27.4 us)
    if (o.mfma_form == 0 && c.col_split) c.mfma_form = 2;
    {   // partial merge: share a column among several lanes when the plan has long columns and too few of them
        int64_t cols = 0;
        int32_t max_nwb = 0;
        for (int32_t i = 0; i < nprob; ++i)
            if (is_sym(probs[i])) { cols += probs[i].n2; max_nwb = std::max(max_nwb, (probs[i].n1 + 63) / 64); }
        const int64_t lanes = 64 * 4 * (int64_t)o.cu_count * 4;      // ~4 waves per SIMD in flight
        c.merge_parts = (max_nwb >= 64 && cols * 16 <= lanes) ? 16 : (max_nwb >= 32 && cols * 4 <= lanes) ? 4 : 1;
    }
    const int parts_k = c.merge_parts >= 16 ? 2 : c.merge_parts >= 4 ? 1 : 0;
    c.merge_cols = c.h_tables() ? o.fix16_cols[parts_k] : o.merge16_cols[parts_k];
    c.scan_variant = use_wpq ? PLSLAM_SCAN_WAVE_PER_QUERY : PLSLAM_SCAN_LANE_PER_QUERY;
    c.block_threads = use_wpq ? 256 : (o.scan_block ? o.scan_block : 256);
    c.rows_scan = use_wpq ? o.rows_wpq : o.rows_lpq;
    // group_cap: measured on MI355X (512 / 2048 pairs per step): 1 -> 321k / 343k pairs/s with 2.55 GB of
    // HBM reads per 2048-pair launch; 2 -> 317k / 343k; >= 3 -> 310k / 335k (many waves streaming the same
    // rows at the same moment contend for the same cache lines) with 0.67 GB of reads.  Default 2.
    // For the 4-rows-per-lane kernel the cap is speed-neutral (364.7k / 364.9k / 364.4k / 365.9k pairs/s at
    // cap 1 / 2 / 3 / 6), so its groups keep a whole problem together.  0 = auto.
    c.group_cap = o.group_cap > 0 ? (size_t)o.group_cap : (c.sym_rows == 4 ? 8 : 2);

    // column split (K1f only): ranges of `cstep` columns per problem so that the launch has about 3 workgroups per CU
    // (option "split_target"), at least 4 tiles = 128 columns per range (option "split_min_tiles")
    const int64_t want = c.col_split ? ((o.split_target > 0 ? o.split_target : 3) * (int64_t)o.cu_count + mf_row_blocks - 1) / mf_row_blocks : 1;
    const int32_t min_tiles = o.split_min_tiles > 0 ? o.split_min_tiles : 4;
    // A column-split plan of mutual K1f problems runs in TWO launches: k_split_post merges the column partials and decides the
    // matches from the column side (match_post.hip); rows without a match keep the -1 the scan's first column range
    // writes.  Not with kept entries (keep_prior: a rejected row's old entry goes through the consistency loop) and not with a
    // stereo gate behind the table (add_stereo_gates switches back to merge + finalize).  Option "split_post": 0 = auto, 1 = never.
    c.split_post = c.col_split && !c.h_tables() && !c.fused && o.split_post != 1 && nprob > 0;
    c.key_rows = c.part_rows = c.tmp_rows = 0;
    c.counts_in_place = nprob > 0;
    bool any_counter = false;
    for (int32_t i = 0; i < nprob; ++i) {
        const plslam_match_problem& p = probs[i];
        PLSLAM_PLAN_REQUIRE(p.n1 >= 0 && p.n2 >= 0, PLSLAM_EINVAL);
        PLSLAM_PLAN_REQUIRE(p.n1 == 0 || p.d1 != nullptr, PLSLAM_EINVAL);
        PLSLAM_PLAN_REQUIRE(p.n2 == 0 || p.d2 != nullptr, PLSLAM_EINVAL);
        PLSLAM_PLAN_REQUIRE(p.n1 == 0 || p.matches_12 != nullptr, PLSLAM_EINVAL);
        PLSLAM_PLAN_REQUIRE((reinterpret_cast<uintptr_t>(p.d1) & 3) == 0, PLSLAM_EINVAL);
        PLSLAM_PLAN_REQUIRE((reinterpret_cast<uintptr_t>(p.d2) & 3) == 0, PLSLAM_EINVAL);
        PLSLAM_PLAN_REQUIRE(p.n2 <= PLSLAM_MAX_TRAIN_ROWS, PLSLAM_ERANGE);
        PLSLAM_PLAN_REQUIRE(!p.mutual || p.n1 <= PLSLAM_MAX_TRAIN_ROWS, PLSLAM_ERANGE);
        ProblemPlan q{ProblemPath::empty, 1, 0, c.key_rows, c.part_rows, c.tmp_rows};
        const bool both = p.n1 > 0 && p.n2 > 0;
        if (c.col_split && both) {
            const int32_t tiles = (p.n2 + 31) / 32;
            const int32_t per = std::max((int32_t)((tiles + want - 1) / want), min_tiles);
            const int32_t ns = (tiles + per - 1) / per;
            if (ns > 1) { q.nsplit = ns; q.cstep = per * 32; }
        }
        q.path = q.nsplit > 1 ? ProblemPath::split : is_sym(p) ? ProblemPath::sym : c.sym_mfma && both ? ProblemPath::directed
                 : p.n1 > 0 ? ProblemPath::scan : ProblemPath::empty;
        c.key_rows += p.n1 + (p.mutual ? p.n2 : 0);
        if (q.path == ProblemPath::split) {     // one partial area per column range (mutual problems), one row table per range
            for (int32_t s = 0; p.mutual && s < q.nsplit; ++s) c.part_rows += c.part_units(p.n1, std::min(q.cstep, p.n2 - s * q.cstep));
            c.tmp_rows += (int64_t)q.nsplit * p.n1;
        } else if (q.path == ProblemPath::sym) {
            // K1e and the XOR form: one (best, second) pair per (row block, column)
            c.part_rows += c.partials16() ? c.part_units(p.n1, p.n2) : (int64_t)((p.n1 + c.rows_partial - 1) / c.rows_partial) * p.n2;
        }
        c.split_post = c.split_post && is_sym(p) && !p.keep_prior;
        any_counter = any_counter || p.n_matches != nullptr;
        c.counts_in_place = c.counts_in_place && p.n_matches != nullptr && p.n_matches == probs[0].n_matches + i;
        c.per.push_back(q);
    }
    c.scatter_counts = any_counter && !c.counts_in_place;
    PLSLAM_PLAN_REQUIRE(c.key_rows < (int64_t(1) << 31), PLSLAM_ERANGE);
    if (has_n1_dev0 && !c.split_post) return PLSLAM_ENOTSUP;
    return PLSLAM_OK;
}
#undef PLSLAM_PLAN_REQUIRE

// base addresses of the areas plan_decide sized (device memory to the caller, plain addresses here)
struct PlanBases {
    uint32_t* keys = nullptr;           // 2 x key_rows words
    uint32_t* partials = nullptr;       // 2 x part_rows words
    uint32_t* rowtmp = nullptr;         // 2 x tmp_rows words
    int32_t* counts = nullptr;          // one #matches counter per problem (counts_in_place: the callers' own array)
    const int32_t* n1_dev0 = nullptr;   // the device row count of problem 0, or nullptr
};

struct PlanTables {
    std::vector<ScanDesc> scans;
    std::vector<int32_t> scan_problem;      // scans[k] belongs to problem scan_problem[k]
    std::vector<SymDesc> syms, dirs;
    std::vector<ProblemDesc> probs;
    std::vector<BlockDesc> scan_blocks, sym_blocks, dir_blocks, merge_blocks, fin_blocks;
    std::vector<int32_t*> user_counts;      // the callers' n_matches pointers (uploaded when they are not one contiguous array)
    bool sym_mfma_multi = false, dir_multi = false;    // some (sub-)problem of the launch has n2 > 2048 (multi-window instantiation)
    bool post_fused = false;                // merge + finalize + gates in ONE kernel, a workgroup per problem (k_post_fused)
    size_t post_lds = 0;                    // ... its dynamic LDS: 8 bytes per column of the widest problem
    int32_t fin_row = 0;                    // > 0: the finalize table is dealt to the XCDs, 8 rows of this length (option post_xcd 2)
    plslam_plan_info info{};
    // the packed image: every table at a 256-byte aligned offset of one upload
    enum { SCANS, SYMS, PROBS, SCAN_BLOCKS, SYM_BLOCKS, MERGE_BLOCKS, FIN_BLOCKS, COUNT_DST, DIRS, DIR_BLOCKS, NPIECES };
    struct Piece { const void* src; size_t bytes, off; } piece[NPIECES] = {};
    size_t total = 0;
    // (scratch of the dealing)
    struct Group { int64_t cost; int32_t first, count; size_t xcd, at; };
    std::vector<Group> groups;
    std::vector<BlockDesc> dealt;
};

// XCD-striped block tables.  Hardware places workgroup b on XCD b % 8 and dispatches in increasing b, and the kernels read
// table entry (b % 8) * L + b / 8, so row x of the table (L entries) is XCD x's work in dispatch order.  Blocks are dealt
// out in GROUPS (runs of at most `cap` blocks with one key: they stream the same descriptor sets, so they should share one
// XCD's L2 at the same time), groups in descending cost, ties in table order: round-robin over the XCDs, but the shortest
// row among the next candidates first.  Rows are padded to equal length with no-op entries (item = -1).  Returns L.
// (Dealing the SHORT groups -- the LBD problems of a stereo batch, seven tiles of mostly memory latency -- evenly among the
// long ones instead of running them together at the end measured 1-3 % SLOWER, 2.62-2.70 against 2.60-2.64 ms per
// 4096-pair scan.)
template <class KeyOf, class CostOf>
inline size_t deal_to_xcds(PlanTables& t, std::vector<BlockDesc>& blocks, size_t cap, KeyOf key_of, CostOf cost_of)
{
    t.groups.clear();
    for (size_t i = 0; i < blocks.size();) {
        size_t j = i;
        while (j < blocks.size() && j - i < cap && key_of(blocks[j]) == key_of(blocks[i])) ++j;
        t.groups.push_back({cost_of(blocks[i]), (int32_t)i, (int32_t)(j - i), 0, 0});
        i = j;
    }
    std::stable_sort(t.groups.begin(), t.groups.end(), [](const PlanTables::Group& a, const PlanTables::Group& b) { return a.cost > b.cost; });
    size_t len[8] = {0, 0, 0, 0, 0, 0, 0, 0}, x = 0;
    for (PlanTables::Group& g : t.groups) {
        size_t best = x;
        for (size_t k = 0; k < 8; ++k) {
            const size_t cand = (x + k) & 7;
            if (len[cand] < len[best]) best = cand;
        }
        g.xcd = best;
        g.at = len[best];
        len[best] += (size_t)g.count;
        x = (best + 1) & 7;
    }
    const size_t L = *std::max_element(len, len + 8);
    t.dealt.assign(8 * L, BlockDesc{-1, 0});
    for (const PlanTables::Group& g : t.groups)
        for (int32_t k = 0; k < g.count; ++k) t.dealt[g.xcd * L + g.at + (size_t)k] = blocks[(size_t)g.first + k];
    blocks.swap(t.dealt);
    return L;
}

// Fills the descriptors and block tables of the choice over `b`, deals them to the XCDs and lays out the packed image.
// plan_info counters (plslam_hip.h): distance_evals = n1 n2 per scan executed (a symmetric scan serves two directions with
// one); directed_evals = n1 n2 per direction; algorithmic_bytes = 32 (Q + T) + 16 Q per DIRECTED scan, however executed.
inline void plan_tables(const PlanChoice& c, const plslam_match_problem* probs, const PlanBases& b, PlanTables& t)
{
    const int32_t nprob = (int32_t)c.per.size();
    t.scans.clear(); t.scan_problem.clear(); t.syms.clear(); t.dirs.clear(); t.probs.clear(); t.user_counts.clear();
    t.scan_blocks.clear(); t.sym_blocks.clear(); t.dir_blocks.clear(); t.merge_blocks.clear(); t.fin_blocks.clear();
    t.sym_mfma_multi = t.dir_multi = false;
    int64_t evals = 0, devals = 0, abytes = 0;
    auto blocks_of = [](std::vector<BlockDesc>& tab, size_t item, int32_t n, int32_t step) {
        for (int32_t r0 = 0; r0 < n; r0 += step) tab.push_back({(int32_t)item, r0});
    };
    for (int32_t i = 0; i < nprob; ++i) {
        const plslam_match_problem& p = probs[i];
        const ProblemPlan& q = c.per[(size_t)i];
        ProblemDesc pd{};
        pd.n1 = p.n1; pd.n2 = p.n2; pd.nnr = p.nnr; pd.mutual = p.mutual ? 1 : 0;
        pd.keep_prior = p.keep_prior ? 1 : 0;
        pd.matches_12 = p.matches_12;
        pd.n_matches = b.counts + i;
        t.user_counts.push_back(p.n_matches);
        uint32_t* k12 = b.keys + 2 * q.key_row;
        uint32_t* k21 = p.mutual ? k12 + 2 * (int64_t)p.n1 : nullptr;
        pd.keys12 = k12;
        pd.keys21 = k21;
        pd.d1 = p.d1; pd.d2 = p.d2;
        pd.gate = -1;
        const int64_t nn = (int64_t)p.n1 * p.n2;
        const bool on_mfma = q.path == ProblemPath::split || (c.sym_mfma && (q.path == ProblemPath::sym || q.path == ProblemPath::directed));
        // (finalize blocks start at multiples of 256 rows and run all 256 lanes: the lazy completion of K1h's / K1i's column keys
        // rotates the neighbouring rows' keys through DPP within aligned groups of 16 lanes -- match_post.hip, finalize_row)
        if (!(c.fused && on_mfma)) blocks_of(t.fin_blocks, (size_t)i, p.n1, 256);
        SymDesc y{};
        y.flags = c.exact_second ? 1 : 0;
        switch (q.path) {
        case ProblemPath::split: {
            // one sub-problem per column range: its own row results (relative column indices, merged by the finalize
            // kernel), its own partial area, its slice of keys21
            uint32_t* tmp = b.rowtmp + 2 * q.tmp_row;
            pd.split_tmp = tmp; pd.keys12_out = k12; pd.nsplit = q.nsplit; pd.cstep = q.cstep;
            pd.lazy21 = p.mutual && c.lazy_keys();
            std::vector<SymDesc>& dst = p.mutual ? t.syms : t.dirs;
            int64_t part_row = q.part_row;
            for (int32_t s = 0; s < q.nsplit; ++s) {
                const int32_t c0 = s * q.cstep, n2s = std::min(q.cstep, p.n2 - c0);
                y.a = p.d1; y.b = p.d2 + (size_t)c0 * 32;
                y.keys12 = tmp + 2 * (int64_t)s * p.n1;
                y.n1 = p.n1; y.n2 = n2s;
                if (c.split_post) { y.mutual = i + 1; y.matches_12 = s == 0 ? p.matches_12 : nullptr; y.n1_dev = b.n1_dev0; }
                if (p.mutual) {
                    y.keys21 = k21 + 2 * (size_t)c0;
                    y.part21 = b.partials + 2 * part_row;
                    y.n_iblk = (p.n1 + c.rows_partial - 1) / c.rows_partial;
                    part_row += c.part_units(p.n1, n2s);
                    // (the merge walks column SLOTS, 32 per tile: the table covers n2 rounded up to a tile)
                    blocks_of(t.merge_blocks, dst.size(), (n2s + 31) & ~31, c.merge_cols);
                }
                blocks_of(p.mutual ? t.sym_blocks : t.dir_blocks, dst.size(), p.n1, 256);
                if (n2s > 2048) (p.mutual ? t.sym_mfma_multi : t.dir_multi) = true;
                dst.push_back(y);
            }
            evals += nn;
            devals += (p.mutual ? 2 : 1) * nn;
            abytes += p.mutual ? 2 * 32LL * (p.n1 + p.n2) + 16LL * (p.n1 + p.n2) : 32LL * (p.n1 + p.n2) + 16LL * p.n1;
            break;
        }
        case ProblemPath::sym:
            pd.lazy21 = c.lazy_keys();
            y.a = p.d1; y.b = p.d2; y.keys12 = k12; y.keys21 = k21;
            y.part21 = b.partials + 2 * q.part_row;
            pd.part21 = y.part21;
            y.n1 = p.n1; y.n2 = p.n2; y.n_iblk = (p.n1 + c.rows_partial - 1) / c.rows_partial;
            if (c.split_post) { y.mutual = i + 1; y.matches_12 = p.matches_12; y.n1_dev = b.n1_dev0; }     // (a problem of one column range)
            if (c.fused) {
                y.mutual = 1; y.matches_12 = p.matches_12; y.n_matches = pd.n_matches; y.nnr = p.nnr;
                t.sym_blocks.push_back({(int32_t)t.syms.size(), 0});
            } else {
                blocks_of(t.sym_blocks, t.syms.size(), p.n1, c.rows_sym);
                if (c.partials16()) blocks_of(t.merge_blocks, t.syms.size(), (p.n2 + 31) & ~31, c.merge_cols);
                else blocks_of(t.merge_blocks, t.syms.size(), p.n2, 256);
            }
            if (c.sym_mfma && p.n2 > 2048) t.sym_mfma_multi = true;
            t.syms.push_back(y);
            evals += nn;
            devals += 2 * nn;
            abytes += 2 * 32LL * (p.n1 + p.n2) + 16LL * (p.n1 + p.n2);
            break;
        case ProblemPath::directed:
            // non-mutual problem on the matrix cores: the directed form (row direction only); mfma_form 3: also the two
            // directions of a mutual problem
            for (int dir = 0; dir < (p.mutual ? 2 : 1); ++dir) {
                y.a = dir ? p.d2 : p.d1; y.b = dir ? p.d1 : p.d2; y.keys12 = dir ? k21 : k12;
                y.n1 = dir ? p.n2 : p.n1; y.n2 = dir ? p.n1 : p.n2;
                if (c.fused && !p.mutual) {
                    y.mutual = 0; y.matches_12 = p.matches_12; y.n_matches = pd.n_matches; y.nnr = p.nnr;
                    t.dir_blocks.push_back({(int32_t)t.dirs.size(), 0});
                } else {
                    blocks_of(t.dir_blocks, t.dirs.size(), y.n1, 256);
                }
                if (y.n2 > 2048) t.dir_multi = true;
                t.dirs.push_back(y);
                evals += nn;
                devals += nn;
                abytes += 32LL * (p.n1 + p.n2) + 16LL * y.n1;
            }
            break;
        case ProblemPath::scan:
            for (int dir = 0; dir < (p.mutual && p.n2 > 0 ? 2 : 1); ++dir) {
                const ScanDesc sc = dir ? ScanDesc{p.d2, p.d1, k21, p.n2, p.n1} : ScanDesc{p.d1, p.d2, k12, p.n1, p.n2};
                blocks_of(t.scan_blocks, t.scans.size(), sc.nq, c.rows_scan);
                t.scans.push_back(sc);
                t.scan_problem.push_back(i);
                evals += nn;
                devals += nn;
                abytes += 32LL * (p.n1 + p.n2) + 16LL * sc.nq;
            }
            break;
        case ProblemPath::empty:
            break;
        }
        t.probs.push_back(pd);
    }
    // scan tables: the blocks of one problem, at most group_cap, make a group; groups in descending train-stream length so
    // that every XCD runs its long blocks (ORB) first and the short ones (LBD) fill the drain phase
    // (fused: one entry per problem, so a group is one workgroup and its cost the whole distance matrix)
    auto item_of = [](const BlockDesc& e) { return e.item; };
    auto stream_cost = [&c](const std::vector<SymDesc>& d) {
        return [&c, &d](const BlockDesc& e) { return (int64_t)d[(size_t)e.item].n2 * (c.fused ? d[(size_t)e.item].n1 : 1); };
    };
    if (!t.sym_blocks.empty()) deal_to_xcds(t, t.sym_blocks, c.group_cap, item_of, stream_cost(t.syms));
    if (!t.dir_blocks.empty()) deal_to_xcds(t, t.dir_blocks, c.group_cap, item_of, stream_cost(t.dirs));
    if (c.scan_variant != PLSLAM_SCAN_WAVE_PER_QUERY && !t.scan_blocks.empty())   // the two directed scans of a mutual problem are adjacent: same group key
        deal_to_xcds(t, t.scan_blocks, c.group_cap, [&t](const BlockDesc& e) { return t.scan_problem[(size_t)e.item]; },
                     [&t](const BlockDesc& e) { return (int64_t)t.scans[(size_t)e.item].nt; });
    // option "post_xcd" = 2: the finalize table dealt PROBLEM BY PROBLEM, in table order (a problem's row blocks gather its column
    // keys through one L2, and consecutive problems sit on different XCDs, so the eight of them sweep memory together)
    t.fin_row = 0;
    if (c.opts.post_xcd == 2 && t.fin_blocks.size() >= 64)
        t.fin_row = (int32_t)deal_to_xcds(t, t.fin_blocks, (size_t)-1, item_of, [](const BlockDesc&) { return (int64_t)0; });

    // The stage behind the scan as ONE kernel (k_post_fused): every problem a mutual one on K1h / K1i with lazy column keys,
    // few row blocks, columns that fit the workgroup's LDS (option "post_fuse": 0 = auto, 1 = never, 2 = whenever the plan is
    // eligible).  AUTO does NOT select it: measured at C2 / 4096 pairs it moves 0.8 GB less per step (no merged column table
    // written and gathered back) but takes 0.335 ms against the separate kernels' 0.276 ms, and the step 2.78 against 2.71 ms --
    // a workgroup per problem is a chain of round trips (partials -> LDS -> rows -> gates) with 2 048 problems in flight,
    // where the separate kernels keep 8x as many independent lanes busy; the scan leaves no free registers beside it
    // (3 x 168 of 512 per lane), so whatever runs behind it displaces scan workgroups one for one and only its own
    // duration counts.
    bool pf = c.opts.post_fuse == 2 && c.lazy_keys() && !c.col_split && nprob > 0;
    int32_t max_n2 = 0;
    for (int32_t i = 0; pf && i < nprob; ++i) {
        pf = c.per[(size_t)i].path == ProblemPath::sym && t.probs[(size_t)i].part21 != nullptr && probs[i].n2 <= POST_FUSED_MAX_N2 &&
             (probs[i].n1 + 255) / 256 <= POST_FUSED_MAX_ROW_BLOCKS;
        max_n2 = std::max(max_n2, probs[i].n2);
    }
    t.post_fused = pf;
    t.post_lds = pf ? sizeof(uint32_t) * 2 * (size_t)((max_n2 + 63) & ~63) : 0;

    const int32_t nsym = (int32_t)t.syms.size(), ndir = (int32_t)t.dirs.size();
    t.info.distance_evals = evals;
    t.info.directed_evals = devals;
    t.info.algorithmic_bytes = abytes;
    t.info.n_scans = (int32_t)t.scans.size() + 2 * nsym + ndir;
    t.info.scan_blocks = (int32_t)(t.scan_blocks.size() + t.sym_blocks.size() + t.dir_blocks.size());
    t.info.scan_variant = nsym ? (c.sym_mfma ? PLSLAM_SCAN_MFMA : PLSLAM_SCAN_SYMMETRIC) : (ndir ? PLSLAM_SCAN_MFMA : c.scan_variant);
    t.info.scan_block_threads = nsym ? (c.sym_rows == 4 && !c.sym_mfma ? 64 : 256) : (ndir ? 256 : c.block_threads);

    auto put = [&t](int k, const auto& v, size_t n) { t.piece[k] = {v.data(), n * sizeof(v[0]), 0}; };
    put(PlanTables::SCANS, t.scans, t.scans.size());
    put(PlanTables::SYMS, t.syms, t.syms.size());
    put(PlanTables::PROBS, t.probs, t.probs.size());
    put(PlanTables::SCAN_BLOCKS, t.scan_blocks, t.scan_blocks.size());
    put(PlanTables::SYM_BLOCKS, t.sym_blocks, t.sym_blocks.size());
    put(PlanTables::MERGE_BLOCKS, t.merge_blocks, t.merge_blocks.size());
    put(PlanTables::FIN_BLOCKS, t.fin_blocks, t.fin_blocks.size());
    put(PlanTables::COUNT_DST, t.user_counts, c.scatter_counts ? t.user_counts.size() : 0);
    put(PlanTables::DIRS, t.dirs, t.dirs.size());
    put(PlanTables::DIR_BLOCKS, t.dir_blocks, t.dir_blocks.size());
    t.total = 0;
    for (PlanTables::Piece& x : t.piece) { x.off = t.total; t.total += align256(x.bytes); }
    if (t.total == 0) t.total = 256;
}

}  // namespace plslam
