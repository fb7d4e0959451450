// The pure host planner of the vocabulary training (plslam_amd/csrc/bow_train_plan.hpp, bow_train_draw.h) on the CPU: no
// device, no HIP header, no library.  Hand cases whose expectations come from include/plslam_bow_train.h, from trees drawn in
// the comments here and from DBoW2's creation order, not from the code under test: one "PASS <case>" or "FAIL <case>: <what>"
// line each, exit status 1 when any failed.  With the argument "draws" it prints the draw function on the tuples read from
// standard input instead (seed, path length, path ..., j, t per line) for tests/test_bow_train_cpu.py.
//   g++ -std=c++17 -I plslam_amd/csrc -I include tests/cpp/test_bow_train_plan.cpp
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include "bow_train_plan.hpp"

using namespace plslam;

namespace {

std::string g_fail;
#define CHECK(cond)                                                                          \
    do {                                                                                     \
        if (!(cond) && g_fail.empty()) g_fail = std::string(#cond) + " (line " + std::to_string(__LINE__) + ")"; \
    } while (0)

int n_failed = 0;
void run(const char* name, const std::function<void()>& body)
{
    g_fail.clear();
    body();
    if (g_fail.empty()) std::printf("PASS %s\n", name);
    else { std::printf("FAIL %s: %s\n", name, g_fail.c_str()); ++n_failed; }
}

template <class T> const T* fake(uintptr_t a) { return reinterpret_cast<const T*>(a); }
bool has(const char* s, const char* part) { return s && strstr(s, part); }

plslam_bow_train_params params(int k, int L)
{
    plslam_bow_train_params p;
    memset(&p, 0, sizeof(p));
    p.k = k; p.L = L; p.weighting_type = PLSLAM_BOW_TF_IDF; p.scoring_type = PLSLAM_BOW_L1_NORM; p.seed = 7;
    return p;
}

int draws_mode()
{
    unsigned long long seed;
    int len;
    while (std::scanf("%llu %d", &seed, &len) == 2) {
        uint64_t key = bt_root_key(seed);
        for (int i = 0; i < len; ++i) {
            int c;
            if (std::scanf("%d", &c) != 1) return 2;
            key = bt_child_key(key, c);
        }
        unsigned j, t;
        if (std::scanf("%u %u", &j, &t) != 2) return 2;
        std::printf("%" PRIu64 " %u\n", key, bt_draw(key, j, t));
    }
    return 0;
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc > 1 && !strcmp(argv[1], "draws")) return draws_mode();
    const uint8_t* D = fake<uint8_t>(0x1000);
    run("check_refusals_in_the_headers_order", [&] {
        BowTrainPlan P;
        const int32_t off[3] = {0, 2, 5};
        plslam_bow_train_params p = params(3, 2);
        CHECK(bow_train_check(&p, D, off, 2, true, 0, &P) == PLSLAM_OK && P.N == 5 && P.n_docs == 2 && P.max_iters == 1000);
        CHECK(bow_train_check(nullptr, D, off, 2, true, 0, &P) == PLSLAM_EINVAL);
        CHECK(bow_train_check(&p, nullptr, off, 2, true, 0, &P) == PLSLAM_EINVAL);
        p = params(1, 2); CHECK(bow_train_check(&p, D, off, 2, true, 0, &P) == PLSLAM_EINVAL && P.why.a == 1 && P.why.b == 2);
        p = params(2, 0); CHECK(bow_train_check(&p, D, off, 2, true, 0, &P) == PLSLAM_EINVAL);
        p = params(257, 2); CHECK(bow_train_check(&p, D, off, 2, true, 0, &P) == PLSLAM_ERANGE);
        p = params(2, 17); CHECK(bow_train_check(&p, D, off, 2, true, 0, &P) == PLSLAM_ERANGE);
        p = params(3, 2); p.scoring_type = 1; CHECK(bow_train_check(&p, D, off, 2, true, 0, &P) == PLSLAM_ENOTSUP && P.why.a == 1);
        p = params(3, 2); p.weighting_type = 4; CHECK(bow_train_check(&p, D, off, 2, true, 0, &P) == PLSLAM_EINVAL);
        p = params(3, 2); p.max_iters = -1; CHECK(bow_train_check(&p, D, off, 2, true, 0, &P) == PLSLAM_EINVAL);
        p = params(3, 2); p.max_iters = 5; CHECK(bow_train_check(&p, D, off, 2, true, 0, &P) == PLSLAM_OK && P.max_iters == 5);
        CHECK(bow_train_check(&p, D, off, 0, true, 0, &P) == PLSLAM_EINVAL);
    });
    run("check_offsets_first_nonzero_decreasing_empty_documents_and_n_zero", [&] {
        BowTrainPlan P;
        plslam_bow_train_params p = params(2, 2);
        const int32_t bad0[3] = {1, 2, 5}, dec[4] = {0, 3, 2, 5}, empties[5] = {0, 0, 4, 4, 4}, none[3] = {0, 0, 0};
        CHECK(bow_train_check(&p, D, bad0, 2, true, 0, &P) == PLSLAM_EINVAL && has(P.why.fmt, "start") && P.why.a == 1);
        CHECK(bow_train_check(&p, D, dec, 3, true, 0, &P) == PLSLAM_EINVAL && has(P.why.fmt, "decrease") && P.why.a == 1);
        CHECK(bow_train_check(&p, D, empties, 4, true, 0, &P) == PLSLAM_OK && P.N == 4 && P.n_docs == 4);
        CHECK(bow_train_check(&p, D, none, 2, true, 0, &P) == PLSLAM_EINVAL && has(P.why.fmt, "no descriptor"));
    });
    run("check_dev_form_takes_n_total_and_the_alignment_and_the_largest_n", [&] {
        BowTrainPlan P;
        plslam_bow_train_params p = params(10, 5);
        const int32_t* off = fake<int32_t>(0x2000);
        CHECK(bow_train_check(&p, D, off, 3, false, 100, &P) == PLSLAM_OK && P.N == 100 && P.oDesc == P.oOff);   // nothing of the caller's is copied
        CHECK(bow_train_check(&p, fake<uint8_t>(0x1008), off, 3, false, 100, &P) == PLSLAM_EINVAL);
        CHECK(bow_train_check(&p, D, off, 3, false, 0, &P) == PLSLAM_EINVAL);
        CHECK(bow_train_check(&p, D, off, 3, false, PLSLAM_BOW_TRAIN_MAX_N, &P) == PLSLAM_OK);
        CHECK(bow_train_check(&p, D, off, 3, false, PLSLAM_BOW_TRAIN_MAX_N + 1, &P) == PLSLAM_ERANGE);
        p = params(256, 16);                                            // 2^23 nodes x 256 centres = 2^31 entries
        CHECK(bow_train_check(&p, D, off, 3, false, PLSLAM_BOW_TRAIN_MAX_N, &P) == PLSLAM_ERANGE && has(P.why.fmt, "centre table"));
    });
    run("sizes_of_a_million_rows_k_10_L_5", [&] {
        BowTrainPlan P;
        plslam_bow_train_params p = params(10, 5);
        CHECK(bow_train_check(&p, D, fake<int32_t>(0x2000), 1, false, 1000000, &P) == PLSLAM_OK);
        CHECK(P.max_visited == 10000);                                  // k^(L-1) = 10^4 < N / 2
        CHECK(P.max_slots == 10000);                                    // < N / 11 = 90909
        CHECK(P.max_items == 100000);
        CHECK(P.tree_cap == 1 + 10 + 100 + 1000 + 10000 + 100000);
        CHECK(P.counter_bytes == (size_t)10000 * 10 * 257 * 4);         // the nodes that iterate, not the level's rows
        p = params(2, 16);                                              // k^15 = 32768 > N / 2 = 50: rows bound the nodes
        CHECK(bow_train_check(&p, D, fake<int32_t>(0x2000), 1, false, 100, &P) == PLSLAM_OK);
        CHECK(P.max_visited == 50 && P.max_slots == 33 && P.tree_cap == 1 + 2 + 4 + 8 + 16 + 32 + 64 + 10 * 100);
        p = params(5, 3);                                               // one row: the root alone
        CHECK(bow_train_check(&p, D, fake<int32_t>(0x2000), 1, false, 1, &P) == PLSLAM_OK);
        CHECK(P.max_visited == 1 && P.max_slots == 0 && P.counter_bytes == (size_t)5 * 257 * 4 && P.tree_cap == 4);
    });
    run("carving_slices_on_256_bytes_in_order_and_disjoint", [&] {
        BowTrainPlan P;
        plslam_bow_train_params p = params(3, 3);
        const int32_t off[2] = {0, 1000};
        CHECK(bow_train_check(&p, D, off, 1, true, 0, &P) == PLSLAM_OK);
        const size_t o[] = {P.oDesc, P.oOff, P.oDoc, P.oPermA, P.oPermB, P.oPnode, P.oAsg, P.oMind, P.oPsum, P.oTot, P.oKey, P.oKeyA,
                            P.oKeyB, P.oIdTmp, P.oTable, P.oIds, P.oLeaf, P.oWord, P.oNbegA, P.oNbegB, P.oNkeyA, P.oNkeyB, P.oNcl,
                            P.oNrun, P.oNround, P.oNchg, P.oNcap, P.oNempty, P.oSnode, P.oSflag, P.oSscan, P.oCent, P.oCnt, P.oCsize,
                            P.oCitem, P.oCscan, P.oTree, P.oNi, P.oStat, P.bytes};
        for (size_t i = 0; i + 1 < sizeof(o) / sizeof(o[0]); ++i) CHECK(o[i] % 256 == 0 && o[i] < o[i + 1]);
        CHECK(P.oOff - P.oDesc == 32000 + 0 && P.oDoc - P.oOff == 256);      // 1000 x 32 is a multiple of 256; 2 offsets
        CHECK(P.oPsum - P.oMind == 4096 && P.oTot - P.oPsum == 8192);        // N x 4 and N x 8 rounded up to 256
        CHECK(P.max_visited == 9 && P.oCsize - P.oCnt == 27904);   // 9 x 3 x 257 x 4 = 27756 -> 109 x 256
        CHECK(P.oCent + 27 * 32 <= P.oCnt);
    });
    run("geometry_blocks_tiles_and_waves", [] {
        CHECK(bt_blocks(0) == 0 && bt_blocks(1) == 1 && bt_blocks(256) == 1 && bt_blocks(257) == 2);
        CHECK(bt_scan_tiles(1024) == 1 && bt_scan_tiles(1025) == 2 && bt_scan_tiles(1 << 24) == 16384);
        CHECK(bt_wave_blocks(4) == 1 && bt_wave_blocks(5) == 2);
        CHECK(bt_pow_capped(10, 4, 1000000) == 10000 && bt_pow_capped(10, 7, 1000000) == 1000000 && bt_pow_capped(2, 62, INT64_MAX) == (int64_t)1 << 62);
        CHECK(bt_pow_capped(256, 15, 1 << 23) == 1 << 23 && bt_pow_capped(3, 0, 5) == 1);
    });
    // The tree of the next three cases, k = 3, L = 3, 20 rows:
    //   root: 3 clusters of 9, 1, 10 rows        level-order 1 2 3        DBoW2 ids 1 2 3
    //     child 1 (9 rows): 2 clusters of 4, 5   level-order 4 5          DBoW2 ids 4 5     (seeding stopped early)
    //       child 4 (4 rows): 3 clusters 2 1 1   level-order 9 10 11      DBoW2 ids 6 7 8
    //       child 5 (5 rows): 3 clusters 0 3 2   level-order 12 13 14     DBoW2 ids 9 10 11 (an empty group: a leaf with no row)
    //     child 2 (1 row): never visited
    //     child 3 (10 rows): 3 clusters 3 3 4    level-order 6 7 8        DBoW2 ids 12 13 14
    //       child 6, 7 (3 rows each, k = 3): trivial, 3 children each     level-order 15 16 17, 18 19 20   DBoW2 15 16 17, 18 19 20
    //       child 8 (4 rows): 3 clusters 2 1 1   level-order 21 22 23     DBoW2 ids 21 22 23
    auto build = [](BowTrainTree* T) {
        BowTrainLevel lv = bow_train_begin(T, 3, 3, 20);
        if (!(lv.level == 1 && lv.n_visited == 1 && lv.n_rows == 20 && lv.n_slots == 1 && lv.base == 1)) return false;
        const int32_t ncl1[1] = {3}, cs1[3] = {9, 1, 10}, r1[1] = {4}, z1[1] = {0};
        lv = bow_train_add_level(T, lv, ncl1, cs1, r1, z1, z1);
        if (!(lv.level == 2 && lv.n_visited == 2 && lv.n_rows == 19 && lv.n_slots == 2 && lv.base == 4)) return false;
        const int32_t ncl2[2] = {2, 3}, cs2[6] = {4, 5, 77, 3, 3, 4}, r2[2] = {2, 7}, cap2[2] = {0, 1}, e2[2] = {0, 0};
        lv = bow_train_add_level(T, lv, ncl2, cs2, r2, cap2, e2);        // (the 77 lies behind ncl: not a child)
        if (!(lv.level == 3 && lv.n_visited == 5 && lv.n_rows == 19 && lv.n_slots == 3 && lv.base == 9)) return false;
        const int32_t ncl3[5] = {3, 3, 3, 3, 3}, cs3[15] = {2, 1, 1, 0, 3, 2, 1, 1, 1, 1, 1, 1, 2, 1, 1}, r3[5] = {3, 5, 0, 0, 2},
                      z3[5] = {0, 0, 0, 0, 0}, e3[5] = {0, 2, 0, 0, 0};
        lv = bow_train_add_level(T, lv, ncl3, cs3, r3, z3, e3);          // level L: nobody is visited, whatever the sizes
        return lv.n_visited == 0 && lv.base == 24 && lv.n_rows == 0;
    };
    run("tree_levels_visited_nodes_rows_slots_and_statistics", [&] {
        BowTrainTree T;
        CHECK(build(&T));
        CHECK(T.parent.size() == 24 && T.levels == 3);
        CHECK(T.rounds == 4 + 2 + 7 + 3 + 5 + 2 && T.rounds_max == 7 && T.capped == 1 && T.empty == 2);
        CHECK((T.parent == std::vector<int32_t>{0, 0, 0, 0, 1, 1, 3, 3, 3, 4, 4, 4, 5, 5, 5, 6, 6, 6, 7, 7, 7, 8, 8, 8}));
        CHECK(T.n_child[0] == 3 && T.n_child[1] == 2 && T.n_child[2] == 0 && T.n_child[3] == 3 && T.first_child[3] == 6 && T.first_child[5] == 12);
    });
    run("renumbering_is_dbow2s_creation_order", [&] {
        BowTrainTree T;
        CHECK(build(&T));
        const std::vector<int32_t> d = bow_train_renumber(T);
        CHECK((d == std::vector<int32_t>{0, 1, 2, 3, 4, 5, 12, 13, 14, 6, 7, 8, 9, 10, 11, 15, 16, 17, 18, 19, 20, 21, 22, 23}));
    });
    run("export_ascending_ids_parents_words_over_the_leaves_and_weights", [&] {
        BowTrainTree T;
        CHECK(build(&T));
        std::vector<uint8_t> desc(24 * 32, 0);
        for (int i = 0; i < 24; ++i) desc[32 * i] = (uint8_t)(100 + i);          // byte 0 = 100 + level-order id
        BowTrainExport E;
        bow_train_export(T, desc.data(), &E);
        CHECK(E.nodes.size() == 23 && E.words.size() == 16);
        for (int d = 1; d <= 23; ++d) CHECK(E.nodes[d - 1].node_id == d);
        CHECK(E.nodes[5].parent_id == 4 && E.nodes[5].descriptor[0] == 109);     // id 6 = level-order 9, under id 4
        CHECK(E.nodes[11].parent_id == 3 && E.nodes[11].descriptor[0] == 106);   // id 12 = level-order 6, under id 3
        CHECK(E.nodes[14].parent_id == 12 && E.nodes[14].descriptor[0] == 115);  // id 15 = level-order 15, under level-order 6 = id 12
        CHECK(E.words[0].word_id == 0 && E.words[0].node_id == 2);               // the leaves by node id: 2, 6, 7, 8, 9, ...
        CHECK(E.words[1].node_id == 6 && E.words[4].node_id == 9 && E.words[15].word_id == 15 && E.words[15].node_id == 23);
        CHECK(E.word_of[2] == 0 && E.word_of[1] == -1 && E.word_of[9] == 1 && E.word_of[23] == 15);
        std::vector<int32_t> ni(16, 1);
        ni[0] = 4; ni[1] = 0; ni[2] = 3;
        bow_train_weights(&E, PLSLAM_BOW_IDF, 4, ni.data());
        CHECK(E.nodes[1].weight == 0.0);                                         // log(4 / 4)
        CHECK(E.nodes[5].weight == 0.0 && E.nodes[0].weight == 0.0);             // Ni = 0; an inner node
        CHECK(E.nodes[6].weight == std::log(4.0 / 3.0) && E.nodes[7].weight == std::log(4.0));
        bow_train_weights(&E, PLSLAM_BOW_BINARY, 4, ni.data());
        CHECK(E.nodes[5].weight == 1.0 && E.nodes[1].weight == 1.0 && E.nodes[0].weight == 0.0);
    });
    run("a_single_row_is_the_roots_one_child", [] {
        BowTrainTree T;
        BowTrainLevel lv = bow_train_begin(&T, 4, 2, 1);
        CHECK(lv.n_slots == 0 && lv.n_rows == 1);
        const int32_t ncl[1] = {1}, cs[4] = {1, 0, 0, 0}, z[1] = {0};
        lv = bow_train_add_level(&T, lv, ncl, cs, z, z, z);
        CHECK(lv.n_visited == 0 && T.parent.size() == 2);
        const uint8_t desc[64] = {0};
        BowTrainExport E;
        bow_train_export(T, desc, &E);
        CHECK(E.nodes.size() == 1 && E.words.size() == 1 && E.nodes[0].parent_id == 0 && E.words[0].node_id == 1);
    });
    run("path_keys_and_draws_known_answers", [] {
        CHECK(bt_mix64(0) == 0 && bt_mix64(1) == 0x5692161D100B05E5ull);     // the splitmix64 finaliser
        CHECK(bt_root_key(7) == bt_mix64(7) && bt_child_key(5, 2) == bt_mix64(8));
        CHECK(bt_draw(0, 0, 0) == (uint32_t)(bt_mix64(0x9E3779B97F4A7C15ull) >> 33) && bt_draw(0, 0, 0) < 0x80000000u);
        CHECK(bt_draw(3, 2, 1) == (uint32_t)(bt_mix64(3 + 0x9E3779B97F4A7C15ull * 0x200000002ull) >> 33));
        CHECK(bt_cut_of(0, 123.0) == 0.0 && bt_cut_of(2147483647u, 123.0) == 123.0 && bt_cut_of(1, 2147483647.0) == 1.0);
        CHECK(bt_first_index(bt_root_key(1), 1) == 0);
        for (int n : {2, 7, 1000}) { const int32_t i = bt_first_index(bt_root_key(9), n); CHECK(i >= 0 && i < n); }
        CHECK(bt_cut(bt_root_key(5), 3, 10.0) > 0.0 && bt_cut(bt_root_key(5), 3, 10.0) <= 10.0);
    });
    return n_failed ? 1 : 0;
}
