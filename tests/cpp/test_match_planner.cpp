// The match planner (plslam_amd/csrc/match_planner.hpp) on the CPU: no device, no HIP header.  One plan per branch of
// plan_decide, the smallest shapes that reach it, on a 256-CU device with made-up base addresses; for each the invariants the
// kernels rely on are checked.  Prints "PASS <case>" or "FAIL <case>: <what>" per case; exit status 1 when any failed.
//   g++ -std=c++17 -I include -I plslam_amd/csrc tests/cpp/test_match_planner.cpp
#include <cstdio>
#include <cstring>
#include <functional>
#include <map>
#include <string>
#include <tuple>

#include "match_planner.hpp"

using namespace plslam;

namespace {

std::string g_fail;     // first failure of the running case
#define CHECK(cond)                                                                          \
    do {                                                                                     \
        if (!(cond) && g_fail.empty()) g_fail = std::string(#cond) + " (line " + std::to_string(__LINE__) + ")"; \
    } while (0)

template <class T> T* fake(uint64_t addr) { return reinterpret_cast<T*>(static_cast<uintptr_t>(addr)); }
uintptr_t addr(const void* p) { return reinterpret_cast<uintptr_t>(p); }

// distinct, 256-byte aligned, far apart: an address of one area can never be taken for one of another
const uint64_t KEYS = 0x100000000000, PARTS = 0x200000000000, TMP = 0x300000000000, COUNTS = 0x400000000000, N1DEV = 0x480000000000,
               DESC = 0x500000000000, OUT = 0x600000000000;

PlanOptions options()
{
    PlanOptions o;
    o.cu_count = 256;
    // what the kernels' translation units report (hamming.hip, hamming_mfma_g.hip, hamming_mfma_h.hip)
    o.rows_wpq = 16; o.rows_lpq = 256;
    o.sym_block_rows[0] = o.sym_block_rows[1] = 256;
    o.sym_partial_rows[0] = 64; o.sym_partial_rows[1] = 256;
    o.merge16_cols[0] = 256; o.merge16_cols[1] = 64; o.merge16_cols[2] = 16;
    o.fix16_cols[0] = 1024; o.fix16_cols[1] = 64; o.fix16_cols[2] = 16;
    return o;
}

plslam_match_problem problem(int i, int32_t n1, int32_t n2, int mutual, int keep_prior = 0)
{
    plslam_match_problem p{};
    p.d1 = fake<uint8_t>(DESC + (uint64_t)i * 0x200000000);
    p.d2 = fake<uint8_t>(DESC + (uint64_t)i * 0x200000000 + 0x100000000);
    p.n1 = n1; p.n2 = n2; p.nnr = 0.8f; p.mutual = mutual; p.keep_prior = keep_prior;
    p.matches_12 = fake<int32_t>(OUT + (uint64_t)i * 0x100000000);
    p.n_matches = nullptr;
    return p;
}

struct Interval { uintptr_t lo, hi; };
void inside_and_disjoint(std::vector<Interval>& v, uintptr_t base, int64_t units)
{
    std::sort(v.begin(), v.end(), [](const Interval& a, const Interval& b) { return a.lo < b.lo; });
    for (size_t k = 0; k < v.size(); ++k) {
        CHECK(v[k].lo >= base && v[k].hi <= base + (uintptr_t)units * 8);
        if (k) CHECK(v[k - 1].hi <= v[k].lo);
    }
}

// a block table: every (item, row0) once, together [0, n) of the item in steps of `step`; padding is {-1, 0}; with L > 0 the
// table is 8 rows of L and every group (a run of at most `cap` blocks with one key, in undealt order) sits in one row
void check_table(const std::vector<BlockDesc>& tab, size_t L, size_t nitems, const std::function<int32_t(int32_t)>& rows_of, int32_t step,
                 const std::function<int32_t(int32_t)>& key_of, size_t cap)
{
    if (L) CHECK(tab.size() == 8 * L && tab.size() % 8 == 0);
    std::map<std::pair<int32_t, int32_t>, size_t> where;       // (item, row0) -> position
    for (size_t k = 0; k < tab.size(); ++k) {
        if (tab[k].item < 0) { CHECK(L > 0 && tab[k].item == -1 && tab[k].row0 == 0); continue; }
        CHECK((size_t)tab[k].item < nitems);
        CHECK(where.emplace(std::make_pair(tab[k].item, tab[k].row0), k).second);
    }
    size_t expected = 0;
    std::map<int32_t, std::vector<size_t>> by_key;              // group key -> positions in undealt order (item, then row0)
    for (int32_t it = 0; it < (int32_t)nitems; ++it)
        for (int32_t r0 = 0; r0 < rows_of(it); r0 += step, ++expected) {
            auto f = where.find({it, r0});
            CHECK(f != where.end());
            if (f != where.end()) by_key[key_of(it)].push_back(f->second);
        }
    CHECK(where.size() == expected);
    if (L)
        for (auto& kv : by_key)
            for (size_t k = 0; k < kv.second.size(); ++k)
                if (k % cap) CHECK(kv.second[k] == kv.second[k - 1] + 1 && kv.second[k] / L == kv.second[k - 1] / L);
}

struct Case {
    PlanChoice c;
    PlanTables t;
    std::vector<plslam_match_problem> probs;
    int rc = 0;
};

// plan_decide + plan_tables + every invariant that holds for any plan
void plan(Case& k, const PlanOptions& o, bool n1_dev0 = false)
{
    const int32_t nprob = (int32_t)k.probs.size();
    k.rc = plan_decide(o, k.probs.data(), nprob, n1_dev0, k.c);
    if (k.rc) return;
    const PlanChoice& c = k.c;
    PlanTables& t = k.t;
    CHECK((int32_t)c.per.size() == nprob);
    plan_tables(c, k.probs.data(), {fake<uint32_t>(KEYS), fake<uint32_t>(PARTS), fake<uint32_t>(TMP), fake<int32_t>(COUNTS),
                                    n1_dev0 ? fake<const int32_t>(N1DEV) : nullptr}, t);
    CHECK((int32_t)t.probs.size() == nprob);
    // block tables
    const bool dealt_scan = c.scan_variant != PLSLAM_SCAN_WAVE_PER_QUERY;
    auto same = [](int32_t it) { return it; };
    check_table(t.scan_blocks, dealt_scan ? t.scan_blocks.size() / 8 : 0, t.scans.size(), [&](int32_t it) { return t.scans[it].nq; }, c.rows_scan,
                [&](int32_t it) { return t.scan_problem[it]; }, c.group_cap);
    check_table(t.sym_blocks, t.sym_blocks.size() / 8, t.syms.size(), [&](int32_t it) { return c.fused ? 1 : t.syms[it].n1; }, c.rows_sym, same, c.group_cap);
    check_table(t.dir_blocks, t.dir_blocks.size() / 8, t.dirs.size(), [&](int32_t it) { return c.fused && !t.dirs[it].mutual && t.dirs[it].matches_12 ? 1 : t.dirs[it].n1; },
                256, same, c.group_cap);
    check_table(t.fin_blocks, (size_t)t.fin_row, (size_t)nprob, [&](int32_t it) {
        const ProblemPath p = c.per[it].path;
        return c.fused && (p == ProblemPath::split || (c.sym_mfma && (p == ProblemPath::sym || p == ProblemPath::directed))) ? 0 : k.probs[it].n1; },
                256, same, (size_t)-1);
    CHECK((t.fin_row > 0) == (c.opts.post_xcd == 2 && t.fin_blocks.size() >= 64));
    check_table(t.merge_blocks, 0, t.syms.size(), [&](int32_t it) { return c.fused ? 0 : c.partials16() ? (t.syms[it].n2 + 31) & ~31 : t.syms[it].n2; },
                c.partials16() ? c.merge_cols : 256, same, 1);
    // the areas: what the scans write is pairwise disjoint and inside what plan_decide sized
    std::vector<Interval> keys, parts, tmp;
    for (const ScanDesc& s : t.scans) keys.push_back({addr(s.keys), addr(s.keys) + (uintptr_t)s.nq * 8});
    for (const std::vector<SymDesc>* v : {&t.syms, &t.dirs})
        for (const SymDesc& y : *v) {
            (addr(y.keys12) >= TMP ? tmp : keys).push_back({addr(y.keys12), addr(y.keys12) + (uintptr_t)y.n1 * 8});
            if (y.keys21) keys.push_back({addr(y.keys21), addr(y.keys21) + (uintptr_t)y.n2 * 8});
            if (y.part21) parts.push_back({addr(y.part21), addr(y.part21) + 8 * (uintptr_t)(c.partials16() ? c.part_units(y.n1, y.n2) : (int64_t)y.n_iblk * y.n2)});
        }
    int64_t devals = 0, abytes = 0;
    for (int32_t i = 0; i < nprob; ++i) {
        const plslam_match_problem& p = k.probs[i];
        const ProblemDesc& pd = t.probs[i];
        CHECK(pd.n1 == p.n1 && pd.n2 == p.n2 && pd.matches_12 == p.matches_12 && pd.gate == -1 && pd.n_matches == fake<int32_t>(COUNTS) + i);
        CHECK(addr(pd.keys12) >= KEYS && addr(pd.keys12) + (uintptr_t)p.n1 * 8 <= KEYS + (uintptr_t)c.key_rows * 8);
        CHECK((pd.keys21 != nullptr) == (p.mutual != 0));
        if (pd.keys21) CHECK(addr(pd.keys21) == addr(pd.keys12) + (uintptr_t)p.n1 * 8 && addr(pd.keys21) + (uintptr_t)p.n2 * 8 <= KEYS + (uintptr_t)c.key_rows * 8);
        CHECK((pd.nsplit > 1) == (c.per[i].path == ProblemPath::split));
        if (pd.nsplit > 1) {       // the ranges tile [0, n2); the finalize kernel merges [nsplit][n1] row results into keys12_out
            CHECK(pd.cstep % 32 == 0 && (int64_t)(pd.nsplit - 1) * pd.cstep < p.n2 && (int64_t)pd.nsplit * pd.cstep >= p.n2);
            CHECK(pd.keys12_out == pd.keys12);
            CHECK(addr(pd.split_tmp) >= TMP && addr(pd.split_tmp) + (uintptr_t)pd.nsplit * p.n1 * 8 <= TMP + (uintptr_t)c.tmp_rows * 8);
        }
        // plslam_plan_info: n1 n2 per direction; 32 (Q + T) + 16 Q per directed scan -- d1 -> d2 whenever there are rows,
        // d2 -> d1 when the problem is mutual and has columns
        if (p.n1 > 0) {
            devals += (int64_t)p.n1 * p.n2;
            abytes += 32LL * (p.n1 + p.n2) + 16LL * p.n1;
            if (p.mutual && p.n2 > 0) { devals += (int64_t)p.n1 * p.n2; abytes += 32LL * (p.n1 + p.n2) + 16LL * p.n2; }
        }
    }
    inside_and_disjoint(keys, KEYS, c.key_rows);
    inside_and_disjoint(parts, PARTS, c.part_rows);
    inside_and_disjoint(tmp, TMP, c.tmp_rows);
    CHECK(t.info.directed_evals == devals);
    CHECK(t.info.algorithmic_bytes == abytes);
    CHECK(t.info.n_scans == (int32_t)(t.scans.size() + 2 * t.syms.size() + t.dirs.size()));
    CHECK(t.info.scan_blocks == (int32_t)(t.scan_blocks.size() + t.sym_blocks.size() + t.dir_blocks.size()));
    // the packed image: pieces in order, 256-byte aligned, not overlapping
    size_t end = 0;
    for (const PlanTables::Piece& x : t.piece) { CHECK(x.off % 256 == 0 && x.off >= end); end = x.off + x.bytes; }
    CHECK(t.total >= end && t.total % 256 == 0 && t.total > 0);
    CHECK(t.piece[PlanTables::PROBS].bytes == (size_t)nprob * sizeof(ProblemDesc));
    CHECK(t.piece[PlanTables::COUNT_DST].bytes == (c.scatter_counts ? (size_t)nprob * sizeof(int32_t*) : 0));
}

std::vector<plslam_match_problem> c3(int keep_prior_on_second = 0)
{
    return {problem(0, 10000, 1500, 1), problem(1, 2000, 200, 1, keep_prior_on_second)};
}

int n_failed = 0;
void run(const char* name, const std::function<void(Case&)>& body)
{
    g_fail.clear();
    Case* k = new Case();       // (a fresh planner state per case)
    body(*k);
    delete k;
    if (g_fail.empty()) std::printf("PASS %s\n", name);
    else { std::printf("FAIL %s: %s\n", name, g_fail.c_str()); ++n_failed; }
}

}  // namespace

int main()
{
    run("small_plan_wave_per_query", [](Case& k) {
        k.probs = {problem(0, 300, 300, 1)};
        plan(k, options());
        CHECK(k.rc == PLSLAM_OK && k.c.small && k.c.scan_variant == PLSLAM_SCAN_WAVE_PER_QUERY && !k.c.sym_mfma && !k.c.col_split);
        CHECK(k.c.per[0].path == ProblemPath::scan && k.t.scans.size() == 2 && k.t.scan_blocks.size() == 2 * 19 && k.t.syms.empty());
        CHECK(k.t.info.scan_variant == PLSLAM_SCAN_WAVE_PER_QUERY && k.t.info.scan_block_threads == 256 && k.t.info.distance_evals == 2 * 300 * 300);
    });
    for (int form : {2, 5})
        run(form == 2 ? "mfma_forced_form_2" : "mfma_forced_form_5", [form](Case& k) {
            PlanOptions o = options();
            o.scan_variant = PLSLAM_SCAN_MFMA; o.mfma_form = form;
            k.probs = {problem(0, 300, 300, 1)};
            plan(k, o);
            CHECK(k.rc == PLSLAM_OK && k.c.sym_mfma && k.c.partials16() && k.c.h_tables() == (form == 5) && k.c.lazy_keys() == (form == 5));
            CHECK(k.c.per[0].path == ProblemPath::sym && k.t.syms.size() == 1 && k.t.scans.empty() && k.t.sym_blocks.size() == 8 * 2);
            CHECK(k.c.part_rows == (form == 5 ? 2 * 2 * 128 : 5 * 2 * 128) && k.t.probs[0].lazy21 == (form == 5));
            CHECK(k.t.info.scan_variant == PLSLAM_SCAN_MFMA && k.t.info.distance_evals == 300 * 300 && !k.t.sym_mfma_multi);
        });
    run("auto_column_split_two_launches", [](Case& k) {
        k.probs = c3();
        plan(k, options());
        // 40 + 8 row blocks; 3 x 256 workgroups aimed at: 16 ranges wanted, at least 4 tiles each
        CHECK(k.rc == PLSLAM_OK && k.c.small && k.c.col_split && k.c.mfma_form == 2 && !k.c.h_tables() && k.c.split_post && !k.c.fused);
        CHECK(k.c.per[0].path == ProblemPath::split && k.c.per[0].nsplit == 12 && k.c.per[0].cstep == 128);
        CHECK(k.c.per[1].path == ProblemPath::split && k.c.per[1].nsplit == 2 && k.c.per[1].cstep == 128);      // 7 tiles: 4 + 3
        CHECK(k.t.syms.size() == 14 && k.c.tmp_rows == 12 * 10000 + 2 * 2000 && k.c.merge_parts == 16 && k.t.syms[13].n2 == 72);
        for (size_t s = 0; s < k.t.syms.size(); ++s) CHECK(k.t.syms[s].mutual == (s < 12 ? 1 : 2) && (k.t.syms[s].matches_12 != nullptr) == (s == 0 || s == 12));
    });
    run("column_split_keep_prior_three_launches", [](Case& k) {
        k.probs = c3(1);
        plan(k, options());
        CHECK(k.rc == PLSLAM_OK && k.c.col_split && k.c.mfma_form == 2 && !k.c.split_post && k.c.per[0].nsplit == 12);
        for (const SymDesc& y : k.t.syms) CHECK(y.mutual == 0 && y.matches_12 == nullptr);
    });
    run("col_split_1_no_split", [](Case& k) {
        PlanOptions o = options();
        o.col_split = 1;
        k.probs = c3();
        plan(k, o);
        CHECK(k.rc == PLSLAM_OK && !k.c.col_split && !k.c.split_post && k.c.tmp_rows == 0 && k.c.scan_variant == PLSLAM_SCAN_WAVE_PER_QUERY);
        CHECK(k.c.per[0].path == ProblemPath::scan && k.c.per[0].nsplit == 1 && k.t.scans.size() == 4);
    });
    run("throughput_plan_dealt_finalize", [](Case& k) {
        for (int i = 0; i < 600; ++i) k.probs.push_back(i % 2 ? problem(i, 200, 200, 1) : problem(i, 1500, 1500, 1));
        plan(k, options());
        CHECK(k.rc == PLSLAM_OK && !k.c.small && k.c.h_tables() && k.c.mfma_form == 0 && k.c.sym_rows == 4 && k.c.group_cap == 8 && k.c.merge_parts == 1);
        CHECK(k.t.syms.size() == 600 && k.t.fin_row > 0 && k.t.fin_blocks.size() == 8 * (size_t)k.t.fin_row && !k.t.post_fused);
        // 2100 blocks dealt problem by problem, each to the shortest row: no row exceeds the shortest by more than one problem's 6
        CHECK(k.t.fin_row >= (2100 + 7) / 8 && k.t.fin_row <= 2100 / 8 + 6);
        CHECK(k.t.info.scan_variant == PLSLAM_SCAN_MFMA && k.t.info.n_scans == 1200);
        // longest first: the first entry of every XCD's row belongs to a 1500-row problem
        const size_t L = k.t.sym_blocks.size() / 8;
        for (size_t x = 0; x < 8; ++x) CHECK(k.t.syms[k.t.sym_blocks[x * L].item].n2 == 1500);
    });
    run("directed_multi_window", [](Case& k) {
        PlanOptions o = options();
        o.scan_variant = PLSLAM_SCAN_MFMA;
        k.probs = {problem(0, 1500, 2100, 0)};
        plan(k, o);
        CHECK(k.rc == PLSLAM_OK && k.c.per[0].path == ProblemPath::directed && k.t.dirs.size() == 1 && k.t.dir_multi && !k.t.sym_mfma_multi);
        CHECK(k.t.syms.empty() && k.c.part_rows == 0 && k.t.dirs[0].part21 == nullptr && k.t.info.scan_variant == PLSLAM_SCAN_MFMA);
    });
    run("no_rows_no_columns_no_problems", [](Case& k) {
        PlanOptions o = options();
        o.scan_variant = PLSLAM_SCAN_MFMA;
        k.probs = {problem(0, 0, 300, 1), problem(1, 300, 0, 1), problem(2, 300, 300, 1)};
        plan(k, o);
        CHECK(k.rc == PLSLAM_OK && k.c.per[0].path == ProblemPath::empty && k.c.per[1].path == ProblemPath::scan && k.c.per[2].path == ProblemPath::sym);
        CHECK(k.t.scans.size() == 1 && k.t.scans[0].nt == 0 && k.t.fin_blocks.size() == 4 && k.c.key_rows == 300 + 300 + 600);
        Case e;
        plan(e, options());
        CHECK(e.rc == PLSLAM_OK && e.c.key_rows == 0 && e.t.total == 256 && e.t.probs.empty() && e.t.info.n_scans == 0 && !e.c.split_post && !e.t.post_fused);
        CHECK(plan_decide(options(), nullptr, 1, false, e.c) == PLSLAM_EINVAL && e.c.error != nullptr);
        CHECK(plan_decide(options(), nullptr, -1, false, e.c) == PLSLAM_EINVAL);
    });
    for (int n2 : {4096, 4097})
        run(n2 == 4096 ? "fuse_2_columns_fit" : "fuse_2_columns_too_many", [n2](Case& k) {
            PlanOptions o = options();
            o.scan_variant = PLSLAM_SCAN_MFMA; o.mfma_form = 2; o.fuse = 2;
            k.probs = {problem(0, 300, n2, 1), problem(1, 300, 100, 0)};
            plan(k, o);
            CHECK(k.rc == PLSLAM_OK && k.c.fused == (n2 == PLSLAM_K1F_FUSED_MAX_N2) && k.t.sym_mfma_multi);
            CHECK(k.t.fin_blocks.size() == (k.c.fused ? 0u : 4u) && k.t.merge_blocks.empty() == k.c.fused);
            CHECK((k.t.syms[0].matches_12 != nullptr) == k.c.fused && (k.t.dirs[0].matches_12 != nullptr) == k.c.fused);
        });
    for (int n1 : {4096, 4097})
        run(n1 == 4096 ? "post_fuse_2_16_row_blocks" : "post_fuse_2_17_row_blocks", [n1](Case& k) {
            PlanOptions o = options();
            o.scan_variant = PLSLAM_SCAN_MFMA; o.post_fuse = 2;
            k.probs = {problem(0, n1, 300, 1), problem(1, 100, 70, 1)};
            plan(k, o);
            CHECK(k.rc == PLSLAM_OK && k.c.h_tables() && k.t.post_fused == (n1 == 256 * POST_FUSED_MAX_ROW_BLOCKS));
            CHECK(k.t.post_lds == (k.t.post_fused ? 8u * 320u : 0u) && k.t.probs[0].part21 == k.t.syms[0].part21);
        });
    run("device_row_count", [](Case& k) {
        k.probs = {problem(0, 10000, 1500, 1)};
        plan(k, options(), true);
        CHECK(k.rc == PLSLAM_OK && k.c.col_split && k.c.split_post && k.t.syms.size() > 1);
        for (const SymDesc& y : k.t.syms) CHECK(y.n1_dev == fake<const int32_t>(N1DEV));
        Case small;     // forced to split although AUTO would not
        small.probs = {problem(0, 300, 300, 1)};
        plan(small, options(), true);
        CHECK(small.rc == PLSLAM_OK && small.c.col_split && small.c.split_post);
        // ineligible: two problems; a non-mutual one; kept entries; options the two-launch plan cannot honour
        PlanChoice c;
        CHECK(plan_decide(options(), c3().data(), 2, true, c) == PLSLAM_ENOTSUP && c.error == nullptr);
        plslam_match_problem p = problem(0, 10000, 1500, 0);
        CHECK(plan_decide(options(), &p, 1, true, c) == PLSLAM_ENOTSUP);
        p = problem(0, 10000, 1500, 1, 1);
        CHECK(plan_decide(options(), &p, 1, true, c) == PLSLAM_ENOTSUP);
        p = problem(0, 10000, 1500, 1);
        for (int which = 0; which < 4; ++which) {
            PlanOptions o = options();
            (which == 0 ? o.col_split : which == 1 ? o.split_post : which == 2 ? o.mfma_form : o.scan_variant) = which == 2 ? 5 : which == 3 ? PLSLAM_SCAN_SYMMETRIC : 1;
            CHECK(plan_decide(o, &p, 1, true, c) == PLSLAM_ENOTSUP);
        }
        CHECK(plan_decide(options(), &p, 1, true, c) == PLSLAM_OK);
    });
    run("limits_and_arguments", [](Case&) {
        PlanChoice c;
        plslam_match_problem p = problem(0, 300, PLSLAM_MAX_TRAIN_ROWS + 1, 0);
        CHECK(plan_decide(options(), &p, 1, false, c) == PLSLAM_ERANGE && c.error != nullptr);
        p = problem(0, 300, PLSLAM_MAX_TRAIN_ROWS, 0);
        CHECK(plan_decide(options(), &p, 1, false, c) == PLSLAM_OK);
        p = problem(0, PLSLAM_MAX_TRAIN_ROWS + 1, 300, 1);
        CHECK(plan_decide(options(), &p, 1, false, c) == PLSLAM_ERANGE);
        p = problem(0, PLSLAM_MAX_TRAIN_ROWS + 1, 300, 0);        // (only a TRAIN set is bounded)
        CHECK(plan_decide(options(), &p, 1, false, c) == PLSLAM_OK);
        p = problem(0, -1, 300, 1);
        CHECK(plan_decide(options(), &p, 1, false, c) == PLSLAM_EINVAL);
        p = problem(0, 300, 300, 1); p.d1 = nullptr;
        CHECK(plan_decide(options(), &p, 1, false, c) == PLSLAM_EINVAL);
        p = problem(0, 300, 300, 1); p.matches_12 = nullptr;
        CHECK(plan_decide(options(), &p, 1, false, c) == PLSLAM_EINVAL);
        p = problem(0, 300, 300, 1); p.d2 = fake<uint8_t>(DESC + 2);
        CHECK(plan_decide(options(), &p, 1, false, c) == PLSLAM_EINVAL);
        // an invalid argument is reported before a size beyond the limit of a LATER problem, and EINVAL of problem 0 before ERANGE of problem 0
        plslam_match_problem two[2] = {problem(0, -1, 300, 1), problem(1, 300, PLSLAM_MAX_TRAIN_ROWS + 1, 0)};
        CHECK(plan_decide(options(), two, 2, false, c) == PLSLAM_EINVAL);
        // 2^31 key rows in all
        std::vector<plslam_match_problem> many;
        for (int i = 0; i < 257; ++i) many.push_back(problem(i, PLSLAM_MAX_TRAIN_ROWS, 1, 0));
        CHECK(plan_decide(options(), many.data(), 256, false, c) == PLSLAM_ERANGE);
        CHECK(plan_decide(options(), many.data(), 255, false, c) == PLSLAM_OK);
        // counters: one contiguous array is counted in place; anything else is scattered
        std::vector<plslam_match_problem> ps = {problem(0, 300, 300, 1), problem(1, 300, 300, 1)};
        ps[0].n_matches = fake<int32_t>(COUNTS + 0x1000); ps[1].n_matches = ps[0].n_matches + 1;
        CHECK(plan_decide(options(), ps.data(), 2, false, c) == PLSLAM_OK && c.counts_in_place && !c.scatter_counts);
        ps[1].n_matches = ps[0].n_matches + 2;
        CHECK(plan_decide(options(), ps.data(), 2, false, c) == PLSLAM_OK && !c.counts_in_place && c.scatter_counts);
        ps[0].n_matches = ps[1].n_matches = nullptr;
        CHECK(plan_decide(options(), ps.data(), 2, false, c) == PLSLAM_OK && !c.counts_in_place && !c.scatter_counts);
    });
    return n_failed ? 1 : 0;
}
