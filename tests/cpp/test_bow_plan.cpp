// The pure host planner of the bag of words (plslam_amd/csrc/bow_plan.hpp) on the CPU: no device, no HIP header, no library.
// Hand cases whose expectations come from include/plslam_hip.h, from trees whose layout is known by construction and from the
// comments here, not from the code under test: one "PASS <case>" or "FAIL <case>: <what>" line each, exit status 1 when any
// failed.
//   g++ -std=c++17 -I plslam_amd/csrc -I include tests/cpp/test_bow_plan.cpp
#include <climits>
#include <cstdio>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include "bow_plan.hpp"

using namespace plslam;

namespace {

std::string g_fail;     // first failure of the running case
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

// addresses that are never read through
template <class T> const T* fake(uintptr_t a) { return reinterpret_cast<const T*>(a); }

bool starts(const char* s, const char* prefix) { return s && strncmp(s, prefix, strlen(prefix)) == 0; }
bool has(const char* s, const char* part) { return s && strstr(s, part); }

// ---- vocabularies --------------------------------------------------------------------------------------------------------
// node `id`: weight id * 1.5, descriptor bytes {id & 255, id >> 8, 0xA5, 0, ...}
plslam_bow_node node(int32_t id, int32_t parent)
{
    plslam_bow_node n;
    memset(&n, 0, sizeof(n));
    n.node_id = id; n.parent_id = parent; n.weight = id * 1.5;
    n.descriptor[0] = (uint8_t)(id & 255); n.descriptor[1] = (uint8_t)(id >> 8); n.descriptor[2] = 0xA5;
    return n;
}
struct Voc {
    std::vector<plslam_bow_node> nodes;
    std::vector<plslam_bow_word> words;
    int32_t scoring = PLSLAM_BOW_L1_NORM, weighting = PLSLAM_BOW_TF_IDF;
    int flatten(BowVocabFlat* F) const
    {
        plslam_bow_vocab_desc d;
        memset(&d, 0, sizeof(d));
        d.k = 2; d.L = 2; d.scoring_type = scoring; d.weighting_type = weighting;
        d.n_nodes = (int32_t)nodes.size(); d.n_words = (int32_t)words.size();
        d.nodes = nodes.empty() ? nullptr : nodes.data();
        d.words = words.empty() ? nullptr : words.data();
        return bow_vocab_flatten(&d, F);
    }
};
// the rule of the layout for breadth-first position i holding node id: its descriptor, its weight
bool holds(const BowVocabFlat& F, int32_t i, int32_t id)
{
    const uint8_t* d = &F.desc[32 * (size_t)i];
    for (int b = 3; b < 32; ++b) if (d[b]) return false;
    if (id == 0) return d[0] == 0 && d[1] == 0 && d[2] == 0 && F.node_w[i] == 0.0;
    return d[0] == (uint8_t)(id & 255) && d[1] == (uint8_t)(id >> 8) && d[2] == 0xA5 && F.node_w[i] == id * 1.5;
}
bool link_is(const BowVocabFlat& F, int32_t i, int32_t first, int32_t count)
{
    return F.links[2 * (size_t)i] == first && F.links[2 * (size_t)i + 1] == count;
}

// tests/test_gpu_bow.py::_tiny: root -> {1 -> {3}, 2}; word 0 is node 2, word 1 is node 3
Voc tiny()
{
    Voc v;
    v.nodes = {node(1, 0), node(2, 0), node(3, 1)};
    v.nodes[0].weight = 0.0; v.nodes[1].weight = 1.0; v.nodes[2].weight = 2.0;
    v.words = {{0, 2}, {1, 3}};
    return v;
}

// The complete k-ary tree of n_total nodes numbered breadth first (node j > 0 hangs off (j - 1) / k), records in id order: the
// breadth-first layout is the identity.  Leaves get the word ids 0, 1, ... in ascending node order.
Voc complete_tree(int32_t k, int32_t n_total)
{
    Voc v;
    for (int32_t j = 1; j < n_total; ++j) v.nodes.push_back(node(j, (j - 1) / k));
    for (int32_t j = 1; j < n_total; ++j)
        if ((int64_t)k * j + 1 >= n_total) v.words.push_back({(int32_t)v.words.size(), j});
    return v;
}
void check_complete_tree(int32_t k, int32_t n_total)
{
    const Voc v = complete_tree(k, n_total);
    BowVocabFlat F;
    CHECK(v.flatten(&F) == PLSLAM_OK);
    CHECK(F.n == n_total && F.n_words == (int32_t)v.words.size() && F.n_stage == (n_total < 1228 ? n_total : 1228));
    CHECK(F.links.size() == 2 * (size_t)n_total && F.desc.size() == 32 * (size_t)n_total && F.node_w.size() == (size_t)n_total);
    CHECK(F.word_w.size() == v.words.size());
    if (!g_fail.empty()) return;
    int32_t word = 0;
    for (int32_t i = 0; i < n_total; ++i) {
        const int64_t c0 = (int64_t)k * i + 1;
        const int32_t cnt = c0 >= n_total ? 0 : (int32_t)std::min<int64_t>(k, n_total - c0);
        CHECK(holds(F, i, i));
        if (cnt) CHECK(link_is(F, i, (int32_t)c0, cnt));
        else {
            CHECK(i > 0 && link_is(F, i, word, 0) && F.word_w[word] == i * 1.5);
            ++word;
        }
    }
    CHECK(word == F.n_words);
}

// ---- databases -----------------------------------------------------------------------------------------------------------
BowDbState fresh_db(int32_t hint, int mode)
{
    BowDbState S;
    S.mode = mode;
    bow_db_commit(S, bow_db_initial(hint, mode), nullptr);
    return S;
}
// check + plan + commit, as a call does; the counts go through the check
int insert(BowDbState& S, int32_t kf, int32_t n_p, int32_t n_l, BowInsertPlan* out = nullptr, bool host = true)
{
    static const plslam_bow_pl_stats st = {1, 1, 1.0, 1.0};
    std::vector<uint8_t> alive((size_t)kf + 1, 0);
    double row = 0;
    BowInsertPlan P;
    int rc = bow_insert_check(S, kf, fake<uint8_t>(0x1000), n_p, fake<uint8_t>(0x2000), n_l, &st, alive.data(), &row, host, &P);
    if (!rc) rc = bow_db_plan_insert(S, kf, n_p, n_l, host, &P);
    if (!rc) bow_db_commit(S, P, &st);
    if (out) *out = P;
    return rc;
}
bool same(const BowDbState& a, const BowDbState& b)
{
    const auto st_eq = [](const plslam_bow_pl_stats& x, const plslam_bow_pl_stats& y) {
        return x.n_pt == y.n_pt && x.n_ls == y.n_ls && x.std_pt == y.std_pt && x.std_ls == y.std_ls;
    };
    return a.mode == b.mode && a.size == b.size && a.cap_kf == b.cap_kf && a.p.cap == b.p.cap && a.p.used == b.p.used &&
           a.l.cap == b.l.cap && a.l.used == b.l.used && a.res_p == b.res_p && a.res_l == b.res_l && a.inserted == b.inserted &&
           a.stats.size() == b.stats.size() && std::equal(a.stats.begin(), a.stats.end(), b.stats.begin(), st_eq);
}
bool same(const BowGrow& a, const BowGrow& b) { return a.cap == b.cap && a.keep == b.keep; }
bool same(const BowInsertPlan& a, const BowInsertPlan& b)
{
    return a.kf_idx == b.kf_idx && a.n_p == b.n_p && a.n_l == b.n_l && a.off_p == b.off_p && a.off_l == b.off_l &&
           same(a.tab, b.tab) && same(a.p, b.p) && same(a.l, b.l) && a.oP == b.oP && a.oL == b.oL && a.oA == b.oA && a.up == b.up &&
           a.oW == b.oW && a.oR == b.oR && a.scratch_bytes == b.scratch_bytes && a.pin_in_bytes == b.pin_in_bytes &&
           a.pin_out_bytes == b.pin_out_bytes && a.sets_lds == b.sets_lds && a.score_lds == b.score_lds;
}

}  // namespace

int main()
{
    // ================================================ flatten ================================================
    run("flatten_the_three_node_tree_written_out_by_hand", [] {
        BowVocabFlat F;
        CHECK(tiny().flatten(&F) == PLSLAM_OK);
        CHECK(F.n == 4 && F.n_words == 2 && F.n_stage == 4);
        // breadth first: root, 1, 2, 3
        CHECK((F.links == std::vector<int32_t>{1, 2, /* node 1 */ 3, 1, /* node 2: word 0 */ 0, 0, /* node 3: word 1 */ 1, 0}));
        CHECK((F.node_w == std::vector<double>{0.0, 0.0, 1.0, 2.0}));
        CHECK((F.word_w == std::vector<double>{1.0, 2.0}));
        std::vector<uint8_t> desc(128, 0);
        for (int id = 1; id <= 3; ++id) { desc[32 * id] = (uint8_t)id; desc[32 * id + 2] = 0xA5; }
        CHECK(F.desc == desc);
    });
    run("flatten_refuses_what_the_gpu_validation_test_refuses", [] {
        BowVocabFlat F;
        Voc v = tiny();
        v.nodes[2].node_id = 4;                                       // id out of range
        CHECK(v.flatten(&F) == PLSLAM_EINVAL && starts(F.why.fmt, "bow vocabulary") && has(F.why.fmt, "out of range") && F.why.a == 4 && F.why.b == 3);
        v = tiny(); v.nodes[2].node_id = 2;                           // duplicate node id
        CHECK(v.flatten(&F) == PLSLAM_EINVAL && starts(F.why.fmt, "bow vocabulary") && has(F.why.fmt, "duplicate node id") && F.why.a == 2);
        v = tiny(); v.nodes[2].parent_id = 7;                         // parent not a node
        CHECK(v.flatten(&F) == PLSLAM_EINVAL && starts(F.why.fmt, "bow vocabulary") && has(F.why.fmt, "is not a node") && F.why.a == 7 && F.why.b == 3);
        v = tiny(); v.nodes[0].parent_id = 3;                         // 1 -> 3 -> 1: both off the root
        CHECK(v.flatten(&F) == PLSLAM_EINVAL && starts(F.why.fmt, "bow vocabulary") && has(F.why.fmt, "not reachable") && F.why.a == 2 && F.why.b == 3);
        v = tiny(); v.words[0].node_id = 2; v.words[1].node_id = 1;   // leaf 3 without a word
        CHECK(v.flatten(&F) == PLSLAM_EINVAL && starts(F.why.fmt, "bow vocabulary") && has(F.why.fmt, "has no word") && F.why.a == 3);
        CHECK(F.links.empty() && F.desc.empty() && F.node_w.empty() && F.word_w.empty() && F.n == 0);   // the last rule: still nothing left behind
        v = tiny(); v.words[1].word_id = 5;                           // word id out of range
        CHECK(v.flatten(&F) == PLSLAM_EINVAL && starts(F.why.fmt, "bow vocabulary") && has(F.why.fmt, "word id") && F.why.a == 5 && F.why.b == 1);
        CHECK(Voc().flatten(&F) == PLSLAM_EINVAL && starts(F.why.fmt, "bow vocabulary: empty"));
        v = tiny(); v.scoring = 1;                                    // L2
        CHECK(v.flatten(&F) == PLSLAM_ENOTSUP && starts(F.why.fmt, "bow vocabulary") && has(F.why.fmt, "scoring type") && F.why.a == 1);
        CHECK(F.links.empty() && F.desc.empty() && F.n == 0);         // a refusal leaves nothing behind
    });
    run("flatten_refusals_no_gpu_test_reaches", [] {
        BowVocabFlat F;
        Voc v = tiny();
        for (int32_t nid : {0, 4, -1}) {                              // a word names a non-node
            v = tiny(); v.words[1].node_id = nid;
            CHECK(v.flatten(&F) == PLSLAM_EINVAL && starts(F.why.fmt, "bow vocabulary") && has(F.why.fmt, "not a node") && F.why.a == 1 && F.why.b == nid);
        }
        v = tiny(); v.words[1].word_id = 0;                           // duplicate word id
        CHECK(v.flatten(&F) == PLSLAM_EINVAL && starts(F.why.fmt, "bow vocabulary") && has(F.why.fmt, "duplicate word id") && F.why.a == 0);
        v = tiny(); v.words[1].node_id = 2;                           // node 2 carries words 0 and 1
        CHECK(v.flatten(&F) == PLSLAM_EINVAL && starts(F.why.fmt, "bow vocabulary") && has(F.why.fmt, "carries two words") && F.why.a == 2);
        v = tiny(); v.nodes[1].parent_id = 2;                         // self-parent
        CHECK(v.flatten(&F) == PLSLAM_EINVAL && starts(F.why.fmt, "bow vocabulary") && has(F.why.fmt, "its own parent") && F.why.a == 2);
        for (int32_t w : {-1, 4}) {                                   // weighting out of range
            v = tiny(); v.weighting = w;
            CHECK(v.flatten(&F) == PLSLAM_EINVAL && starts(F.why.fmt, "bow vocabulary") && has(F.why.fmt, "weighting type") && F.why.a == w);
        }
        for (int32_t w : {PLSLAM_BOW_TF_IDF, PLSLAM_BOW_TF, PLSLAM_BOW_IDF, PLSLAM_BOW_BINARY}) {
            v = tiny(); v.weighting = w;
            CHECK(v.flatten(&F) == PLSLAM_OK);
        }
        v = tiny(); v.nodes[0].parent_id = -1;                        // a negative parent
        CHECK(v.flatten(&F) == PLSLAM_EINVAL && has(F.why.fmt, "is not a node"));
        v = tiny(); v.nodes[0].node_id = 0;                           // the root has no record
        CHECK(v.flatten(&F) == PLSLAM_EINVAL && has(F.why.fmt, "out of range"));
        plslam_bow_vocab_desc d;                                      // counts without arrays; no descriptor at all
        memset(&d, 0, sizeof(d));
        d.n_nodes = 3; d.n_words = 2;
        CHECK(bow_vocab_flatten(&d, &F) == PLSLAM_EINVAL);
        CHECK(bow_vocab_flatten(nullptr, &F) == PLSLAM_EINVAL);
    });
    run("flatten_shuffled_records_keep_children_in_record_order_not_id_order", [] {
        // root -> {5, 6}; 5 -> {2, 1, 3}; 6 -> {4}, the records in this order:
        Voc v;
        v.nodes = {node(5, 0), node(2, 5), node(6, 0), node(1, 5), node(4, 6), node(3, 5)};
        v.words = {{0, 4}, {1, 1}, {2, 3}, {3, 2}};
        BowVocabFlat F;
        CHECK(v.flatten(&F) == PLSLAM_OK && F.n == 7 && F.n_words == 4 && F.n_stage == 7);
        const int32_t order[7] = {0, 5, 6, 2, 1, 3, 4};               // breadth first, lists in record order
        for (int i = 0; i < 7; ++i) CHECK(holds(F, i, order[i]));
        CHECK(link_is(F, 0, 1, 2) && link_is(F, 1, 3, 3) && link_is(F, 2, 6, 1));
        CHECK(link_is(F, 3, 3, 0) && link_is(F, 4, 1, 0) && link_is(F, 5, 2, 0) && link_is(F, 6, 0, 0));
        CHECK((F.word_w == std::vector<double>{4 * 1.5, 1 * 1.5, 3 * 1.5, 2 * 1.5}));
    });
    run("flatten_records_in_reverse_order", [] {
        // the complete binary tree 0 -> {1, 2}, 1 -> {3, 4}, 2 -> {5, 6}, records 6, 5, ..., 1: every list comes out reversed
        Voc v;
        for (int32_t j = 6; j >= 1; --j) v.nodes.push_back(node(j, (j - 1) / 2));
        v.words = {{0, 3}, {1, 4}, {2, 5}, {3, 6}};
        BowVocabFlat F;
        CHECK(v.flatten(&F) == PLSLAM_OK && F.n == 7);
        const int32_t order[7] = {0, 2, 1, 6, 5, 4, 3};
        for (int i = 0; i < 7; ++i) CHECK(holds(F, i, order[i]));
        CHECK(link_is(F, 0, 1, 2) && link_is(F, 1, 3, 2) && link_is(F, 2, 5, 2));
        CHECK(link_is(F, 3, 3, 0) && link_is(F, 4, 2, 0) && link_is(F, 5, 1, 0) && link_is(F, 6, 0, 0));
        CHECK((F.word_w == std::vector<double>{4.5, 6.0, 7.5, 9.0}));
    });
    run("flatten_complete_trees_of_1227_1228_1229_nodes_stage_min_of_n_and_1228", [] {
        CHECK(STAGE_NODES == 1228);
        for (int32_t n_total : {1227, 1228, 1229}) check_complete_tree(10, n_total);      // ragged last levels
        check_complete_tree(3, 1229);
        check_complete_tree(1, 5);                                                         // a chain
        check_complete_tree(7, 2);                                                         // the root and one leaf
    });
    run("flatten_a_parents_children_straddle_position_1228", [] {
        // k = 10: position 122's children are 1221 .. 1230, on both sides of the last staged position 1227
        check_complete_tree(10, 1235);
        BowVocabFlat F;
        CHECK(complete_tree(10, 1235).flatten(&F) == PLSLAM_OK && F.n_stage == 1228);
        CHECK(link_is(F, 122, 1221, 10) && 1221 < F.n_stage && F.n_stage <= 1230);
        CHECK(link_is(F, 123, 1231, 4) && link_is(F, 124, 0, 0));
    });
    run("flatten_a_two_node_cycle_off_the_root_is_refused_by_the_count", [] {
        Voc v;
        v.nodes = {node(1, 0), node(2, 0), node(3, 4), node(4, 3)};
        v.words = {{0, 1}, {1, 2}};
        BowVocabFlat F;
        CHECK(v.flatten(&F) == PLSLAM_EINVAL && starts(F.why.fmt, "bow vocabulary") && has(F.why.fmt, "not reachable from the root"));
        CHECK(F.why.a == 2 && F.why.b == 4);                           // 2 of 4 nodes
    });
    // ================================================ transform ================================================
    run("transform_offsets_first_nonzero_decreasing_and_the_largest_set", [] {
        BowTransformCheck C;
        const uint8_t* desc = fake<uint8_t>(0x1000);
        int32_t len[4];
        const int32_t a[3] = {1, 5, 9};
        CHECK(bow_transform_check_host(desc, a, 2, len, &C) == PLSLAM_EINVAL);
        const int32_t b[4] = {0, 5, 4, 9};
        CHECK(bow_transform_check_host(desc, b, 3, len, &C) == PLSLAM_EINVAL);
        const int32_t c[4] = {0, 7, 7, 7 + PLSLAM_BOW_MAX_SET};
        CHECK(bow_transform_check_host(desc, c, 3, len, &C) == PLSLAM_OK);
        CHECK(C.nsets == 3 && C.max_set == PLSLAM_BOW_MAX_SET && C.total == 7 + PLSLAM_BOW_MAX_SET);
        const int32_t d[3] = {0, 7, 8 + PLSLAM_BOW_MAX_SET};
        CHECK(bow_transform_check_host(desc, d, 2, len, &C) == PLSLAM_ERANGE && starts(C.why.fmt, "bow transform") &&
              C.why.a == PLSLAM_BOW_MAX_SET + 1 && C.why.b == PLSLAM_BOW_MAX_SET);
        const int32_t e[3] = {0, 0, 0};                                // empty sets need no descriptors; rows do
        CHECK(bow_transform_check_host(nullptr, e, 2, len, &C) == PLSLAM_OK && C.total == 0 && C.max_set == 0 && C.nsets == 2);
        CHECK(bow_transform_check_host(nullptr, c, 3, len, &C) == PLSLAM_EINVAL);
        CHECK(bow_transform_check_host(desc, nullptr, 3, len, &C) == PLSLAM_EINVAL);
        CHECK(bow_transform_check_host(desc, c, 3, nullptr, &C) == PLSLAM_EINVAL);
        const int32_t f[3] = {0, INT32_MAX, INT32_MIN};               // sizes are taken in 64 bits
        CHECK(bow_transform_check_host(desc, f, 1, len, &C) == PLSLAM_ERANGE && C.why.a == INT32_MAX);
        CHECK(bow_transform_check_host(desc, f, 2, len, &C) == PLSLAM_ERANGE);     // (the first set refuses; the second is negative)
    });
    run("transform_nsets_zero_is_ok_and_reads_nothing", [] {
        BowTransformCheck C;
        CHECK(bow_transform_check_host(nullptr, nullptr, 0, nullptr, &C) == PLSLAM_OK && C.nsets == 0);
        CHECK(bow_transform_check_dev(nullptr, nullptr, 0, 0, 0, nullptr, nullptr, nullptr, nullptr, &C) == PLSLAM_OK && C.nsets == 0);
        CHECK(bow_transform_check_host(nullptr, nullptr, -1, nullptr, &C) == PLSLAM_EINVAL);
        CHECK(bow_transform_check_dev(nullptr, nullptr, -1, 0, 0, nullptr, nullptr, nullptr, nullptr, &C) == PLSLAM_EINVAL);
    });
    run("transform_layout_slices_on_256_bytes_in_order_and_disjoint", [] {
        for (const auto& nt : std::vector<std::pair<int32_t, int32_t>>{{3, 1000}, {1, 0}, {64, 96000}, {5, 1}}) {
            const int32_t nsets = nt.first, total = nt.second;
            const BowTransformLayout L = bow_transform_layout(nsets, total);
            const size_t off[7] = {L.oD, L.oO, L.oW, L.oV, L.oBW, L.oBV, L.oL};
            const size_t bytes[7] = {(size_t)total * 32, ((size_t)nsets + 1) * 4, (size_t)total * 4, (size_t)total * 8,
                                     (size_t)total * 4,  (size_t)total * 8,       (size_t)nsets * 4};
            size_t end = 0;
            for (int i = 0; i < 7; ++i) {
                CHECK(off[i] % 256 == 0 && off[i] >= end);
                end = off[i] + bytes[i];
            }
            CHECK(L.oD == 0 && L.bytes >= end && L.bytes % 256 == 0 && L.bytes < end + 256);
        }
    });
    run("transform_dev_argument_and_alignment_rules", [] {
        BowTransformCheck C;
        const int32_t* i32 = fake<int32_t>(0x2000);
        const double* f64 = fake<double>(0x3000);
        CHECK(bow_transform_check_dev(fake<uint8_t>(0x1000), i32, 4, 100, 50, i32, i32, f64, i32, &C) == PLSLAM_OK);
        CHECK(C.nsets == 4 && C.total == 100 && C.max_set == 50);
        CHECK(bow_transform_check_dev(fake<uint8_t>(0x1010), i32, 4, 100, 50, i32, i32, f64, i32, &C) == PLSLAM_OK);
        CHECK(bow_transform_check_dev(fake<uint8_t>(0x1008), i32, 4, 100, 50, i32, i32, f64, i32, &C) == PLSLAM_EINVAL);
        CHECK(bow_transform_check_dev(fake<uint8_t>(0x1001), i32, 4, 100, 50, i32, i32, f64, i32, &C) == PLSLAM_EINVAL);
        CHECK(bow_transform_check_dev(nullptr, i32, 4, 100, 50, i32, i32, f64, i32, &C) == PLSLAM_EINVAL);
        CHECK(bow_transform_check_dev(nullptr, i32, 4, 0, 0, i32, i32, f64, i32, &C) == PLSLAM_OK);
        CHECK(bow_transform_check_dev(fake<uint8_t>(0x1000), nullptr, 4, 100, 50, i32, i32, f64, i32, &C) == PLSLAM_EINVAL);
        CHECK(bow_transform_check_dev(fake<uint8_t>(0x1000), i32, 4, 100, 50, nullptr, i32, f64, i32, &C) == PLSLAM_EINVAL);
        CHECK(bow_transform_check_dev(fake<uint8_t>(0x1000), i32, 4, 100, 50, i32, nullptr, f64, i32, &C) == PLSLAM_EINVAL);
        CHECK(bow_transform_check_dev(fake<uint8_t>(0x1000), i32, 4, 100, 50, i32, i32, nullptr, i32, &C) == PLSLAM_EINVAL);
        CHECK(bow_transform_check_dev(fake<uint8_t>(0x1000), i32, 4, 100, 50, i32, i32, f64, nullptr, &C) == PLSLAM_EINVAL);
        CHECK(bow_transform_check_dev(fake<uint8_t>(0x1000), i32, 4, -1, 50, i32, i32, f64, i32, &C) == PLSLAM_EINVAL);
        CHECK(bow_transform_check_dev(fake<uint8_t>(0x1000), i32, 4, 100, PLSLAM_BOW_MAX_SET, i32, i32, f64, i32, &C) == PLSLAM_OK);
        CHECK(bow_transform_check_dev(fake<uint8_t>(0x1000), i32, 4, 100, PLSLAM_BOW_MAX_SET + 1, i32, i32, f64, i32, &C) == PLSLAM_ERANGE &&
              starts(C.why.fmt, "bow transform") && C.why.a == PLSLAM_BOW_MAX_SET + 1);
        // the bound is refused ahead of the early return for no sets
        CHECK(bow_transform_check_dev(nullptr, nullptr, 0, 0, PLSLAM_BOW_MAX_SET + 1, nullptr, nullptr, nullptr, nullptr, &C) == PLSLAM_ERANGE);
    });
    run("geometry_lds_bytes_grids_and_their_limits", [] {
        // K20: the keys padded to a power of two (at least one) and one scan word per lane of 1024
        CHECK(bow_set_lds(0) == 4 + 4096 && bow_set_lds(1) == 4 + 4096 && bow_set_lds(2) == 8 + 4096 && bow_set_lds(3) == 16 + 4096);
        CHECK(bow_set_lds(1024) == 4096 + 4096 && bow_set_lds(1025) == 8192 + 4096);
        CHECK(bow_set_lds(PLSLAM_BOW_MAX_SET) == 65536 + 4096 && bow_set_lds(PLSLAM_BOW_MAX_SET) <= SET_LDS_MAX);
        // K21: both query vectors' word ids, never zero bytes
        CHECK(bow_score_lds(0, 0) == 16 && bow_score_lds(3, 0) == 16 && bow_score_lds(3, 2) == 20 && bow_score_lds(1500, 200) == 6800);
        CHECK(bow_score_lds(PLSLAM_BOW_MAX_SET, PLSLAM_BOW_MAX_SET) == SCORE_LDS_MAX && SCORE_LDS_MAX == 131072);
        CHECK(bow_score_grid_x(1) == 1 && bow_score_grid_x(4) == 1 && bow_score_grid_x(5) == 2 && bow_score_grid_x(10001) == 2501);
        // K19: a lane per descriptor, 256 a block; 40 bytes per staged node, inside the 48 KB a kernel has without asking
        CHECK(bow_descend_blocks(0) == 0 && bow_descend_blocks(1) == 1 && bow_descend_blocks(256) == 1 && bow_descend_blocks(257) == 2);
        CHECK(bow_stage_bytes(STAGE_NODES) == 49120 && bow_stage_bytes(STAGE_NODES) <= 48 * 1024 && bow_stage_bytes(STAGE_NODES + 1) > 48 * 1024);
        CHECK(DESCEND_THREADS == 256 && SET_THREADS == 1024 && NO_WORD == 0xFFFFFFFFu);
    });
    // ================================================ database ================================================
    run("db_initial_capacities_for_hints_0_4_16_17", [] {
        const int32_t hint[4] = {0, 4, 16, 17}, kf[4] = {16, 16, 16, 17};
        for (int i = 0; i < 4; ++i) {
            const BowInsertPlan P = bow_db_initial(hint[i], 3);
            CHECK(P.kf_idx == -1 && P.tab.cap == kf[i] && P.p.cap == kf[i] * 256 && P.l.cap == kf[i] * 64);
            CHECK(P.tab.keep == 0 && P.p.keep == 0 && P.l.keep == 0);
            const BowDbState S = fresh_db(hint[i], 3);
            CHECK(S.mode == 3 && S.size == 0 && S.cap_kf == kf[i] && S.p.cap == kf[i] * 256 && S.l.cap == kf[i] * 64);
            CHECK(S.p.used == 0 && S.l.used == 0 && S.inserted.empty() && S.res_p.empty() && S.res_l.empty() && S.stats.empty());
        }
        CHECK(bow_db_initial(16, 1).l.cap == 0 && bow_db_initial(16, 1).p.cap == 4096);
        CHECK(bow_db_initial(16, 2).p.cap == 0 && bow_db_initial(16, 2).l.cap == 1024);
    });
    run("db_an_insert_that_grows_nothing", [] {
        BowDbState S = fresh_db(16, 3);
        BowInsertPlan P;
        CHECK(insert(S, 0, 100, 20, &P) == PLSLAM_OK);
        CHECK(P.kf_idx == 0 && P.n_p == 100 && P.n_l == 20 && P.off_p == 0 && P.off_l == 0);
        CHECK(P.tab.cap == 16 && P.p.cap == 4096 && P.l.cap == 1024);
        CHECK(S.size == 1 && S.p.used == 100 && S.l.used == 20 && S.cap_kf == 16 && S.p.cap == 4096 && S.l.cap == 1024);
        CHECK(S.res_p[0] == 100 && S.res_l[0] == 20 && S.inserted[0] == 1 && S.stats[0].n_pt == 1);
        CHECK(insert(S, 1, 7, 0, &P) == PLSLAM_OK && P.off_p == 100 && P.off_l == 20);
        CHECK(S.size == 2 && S.p.used == 107 && S.l.used == 20 && S.cap_kf == 16 && S.p.cap == 4096 && S.l.cap == 1024);
    });
    run("db_the_table_grows_at_kf_idx_equal_to_cap_kf", [] {
        BowDbState S = fresh_db(16, 3);
        BowInsertPlan P;
        for (int32_t k = 0; k < 16; ++k) {
            CHECK(insert(S, k, 1, 1, &P) == PLSLAM_OK);
            CHECK(P.tab.cap == 16);
        }
        CHECK(insert(S, 16, 1, 1, &P) == PLSLAM_OK);
        CHECK(P.tab.cap == 32 && P.tab.keep == 16);                    // max(17, 2 x 16); the 16 rows in use
        CHECK(P.p.cap == 4096 && P.l.cap == 1024);                     // and nothing else
        CHECK(S.cap_kf == 32 && S.size == 17);
    });
    run("db_a_pool_is_full_at_used_plus_n_equal_cap_and_grows_one_beyond", [] {
        for (int kind = 0; kind < 2; ++kind) {                         // 0 the point pool, 1 the line pool
            const int64_t cap = kind ? 1024 : 4096;
            const int32_t fill = (int32_t)cap - 100;
            BowDbState S = fresh_db(16, 3);
            BowInsertPlan P;
            CHECK(insert(S, 0, kind ? 3 : fill, kind ? fill : 3) == PLSLAM_OK);
            BowDbState T = S;
            CHECK(insert(T, 1, kind ? 3 : 100, kind ? 100 : 3, &P) == PLSLAM_OK);      // used + n == cap
            CHECK(P.tab.cap == 16 && P.p.cap == 4096 && P.l.cap == 1024);
            CHECK((kind ? T.l.used : T.p.used) == cap);
            T = S;
            CHECK(insert(T, 1, kind ? 3 : 101, kind ? 101 : 3, &P) == PLSLAM_OK);      // one beyond: 2 x cap > need
            const BowGrow& g = kind ? P.l : P.p;
            const BowGrow& other = kind ? P.p : P.l;
            CHECK(g.cap == 2 * cap && g.keep == fill && other.cap == (kind ? 4096 : 1024) && P.tab.cap == 16);
            CHECK((kind ? T.l.cap : T.p.cap) == 2 * cap && (kind ? T.p.cap : T.l.cap) == (kind ? 4096 : 1024) && T.cap_kf == 16);
            T = S;
            CHECK(insert(T, 1, kind ? 3 : PLSLAM_BOW_MAX_SET, kind ? PLSLAM_BOW_MAX_SET : 3, &P) == PLSLAM_OK);   // need > 2 x cap
            CHECK((kind ? P.l : P.p).cap == fill + PLSLAM_BOW_MAX_SET && (kind ? P.l : P.p).keep == fill);
        }
        CHECK(bow_grow_to(16, 17) == 32 && bow_grow_to(16, 32) == 32 && bow_grow_to(16, 33) == 33 && bow_grow_to(0, 5) == 5);
    });
    run("db_kf_idx_jumps_from_3_to_1000", [] {
        BowDbState S = fresh_db(4, 1);
        BowInsertPlan P;
        for (int32_t k = 0; k < 4; ++k) CHECK(insert(S, k, 10, 0) == PLSLAM_OK);
        CHECK(insert(S, 1000, 10, 0, &P) == PLSLAM_OK);
        CHECK(P.tab.cap == 1001 && P.tab.keep == 4 && P.off_p == 40);
        CHECK(S.size == 1001 && S.cap_kf == 1001 && S.inserted.size() == 1001 && S.res_p.size() == 1001 && S.stats.size() == 1001);
        CHECK(S.inserted[3] == 1 && S.inserted[4] == 0 && S.inserted[999] == 0 && S.inserted[1000] == 1 && S.res_p[500] == 0);
        // a live keyframe in the gap was never inserted: the host call says which
        std::vector<uint8_t> alive(1001, 0);
        alive[2] = 1; alive[1000] = 1;
        int32_t n_p = 1, n_l = 0;
        double row = 0;
        CHECK(bow_insert_check(S, 1001, fake<uint8_t>(0x1000), n_p, nullptr, n_l, nullptr, alive.data(), &row, true, &P) == PLSLAM_OK);
        alive[777] = 1;
        CHECK(bow_insert_check(S, 1001, fake<uint8_t>(0x1000), n_p, nullptr, n_l, nullptr, alive.data(), &row, true, &P) == PLSLAM_EINVAL &&
              starts(P.why.fmt, "bow insert") && has(P.why.fmt, "never inserted") && P.why.a == 777);
        CHECK(bow_insert_check(S, 1001, fake<uint8_t>(0x1000), n_p, nullptr, n_l, nullptr, alive.data(), &row, false, &P) == PLSLAM_OK);
    });
    run("db_a_mode_without_points_zeroes_n_p_and_never_plans_a_point_pool", [] {
        BowDbState S = fresh_db(0, 2);
        CHECK(S.p.cap == 0 && S.l.cap == 1024);
        int32_t n_p = 77, n_l = 2000;
        double row = 0;
        BowInsertPlan P;
        CHECK(bow_insert_check(S, 0, nullptr, n_p, fake<uint8_t>(0x1000), n_l, nullptr, nullptr, &row, true, &P) == PLSLAM_OK);
        CHECK(n_p == 0 && n_l == 2000);
        CHECK(bow_db_plan_insert(S, 0, n_p, n_l, true, &P) == PLSLAM_OK);
        CHECK(P.p.cap == 0 && P.p.keep == 0 && P.n_p == 0 && P.l.cap == 2048 && P.oL == P.oP);
        bow_db_commit(S, P, nullptr);
        CHECK(S.p.cap == 0 && S.p.used == 0 && S.res_p[0] == 0 && S.l.used == 2000 && S.res_l[0] == 2000);
        // and the other way round
        BowDbState T = fresh_db(0, 1);
        n_p = 5; n_l = -3;
        CHECK(bow_insert_check(T, 0, fake<uint8_t>(0x1000), n_p, nullptr, n_l, nullptr, nullptr, &row, true, &P) == PLSLAM_OK && n_l == 0);
        CHECK(bow_db_plan_insert(T, 0, n_p, n_l, true, &P) == PLSLAM_OK && P.l.cap == 0 && P.p.cap == 4096);
    });
    run("db_a_plan_leaves_the_state_untouched_until_commit", [] {
        BowDbState S = fresh_db(4, 3);
        CHECK(insert(S, 0, 4000, 1000) == PLSLAM_OK);
        const BowDbState before = S;
        BowInsertPlan P, Q;
        CHECK(bow_db_plan_insert(S, 40, 500, 500, true, &P) == PLSLAM_OK);       // grows all three
        CHECK(P.tab.cap == 41 && P.p.cap == 8192 && P.l.cap == 2048);
        CHECK(same(S, before));
        P = BowInsertPlan{};                                                     // the plan is dropped
        CHECK(bow_db_plan_insert(S, 40, 500, 500, true, &P) == PLSLAM_OK && bow_db_plan_insert(S, 40, 500, 500, true, &Q) == PLSLAM_OK);
        CHECK(same(P, Q) && same(S, before));
        bow_db_commit(S, P, nullptr);
        CHECK(!same(S, before) && S.cap_kf == 41 && S.p.cap == 8192 && S.l.cap == 2048 && S.p.used == 4500 && S.l.used == 1500);
    });
    run("db_the_2_31_refusal_plans_no_growth", [] {
        BowDbState S = fresh_db(16, 3);
        S.p.used = (int64_t)INT32_MAX - 10;                            // (a state no test can reach by inserting)
        S.p.cap = S.p.used;
        const BowDbState before = S;
        BowInsertPlan P;
        CHECK(bow_db_plan_insert(S, 5, 11, 1, true, &P) == PLSLAM_ERANGE && starts(P.why.fmt, "bow database") && has(P.why.fmt, "2^31"));
        CHECK(P.kf_idx == -1 && P.tab.cap == 0 && P.p.cap == 0 && P.l.cap == 0 && P.scratch_bytes == 0);
        CHECK(same(S, before));
        CHECK(bow_db_plan_insert(S, 5, 10, 1, true, &P) == PLSLAM_OK && P.p.cap == 2 * S.p.cap && P.off_p == S.p.used);
        S = before;
        S.l.used = (int64_t)INT32_MAX;
        CHECK(bow_db_plan_insert(S, 5, 0, 1, false, &P) == PLSLAM_ERANGE && P.l.cap == 0);
        CHECK(bow_db_plan_insert(S, 5, 0, 0, false, &P) == PLSLAM_OK);
    });
    run("db_keep_is_what_is_in_use_not_the_capacity", [] {
        BowDbState S = fresh_db(16, 3);
        CHECK(insert(S, 0, 10, 3) == PLSLAM_OK);
        BowInsertPlan P;
        CHECK(bow_db_plan_insert(S, 20, PLSLAM_BOW_MAX_SET, PLSLAM_BOW_MAX_SET, true, &P) == PLSLAM_OK);
        CHECK(P.p.cap == 10 + PLSLAM_BOW_MAX_SET && P.p.keep == 10 && P.l.cap == 3 + PLSLAM_BOW_MAX_SET && P.l.keep == 3);
        CHECK(P.tab.cap == 32 && P.tab.keep == 1);
    });
    run("db_inserting_an_index_again_overwrites_its_reservation_and_advances_used", [] {
        BowDbState S = fresh_db(16, 3);
        BowInsertPlan P;
        CHECK(insert(S, 2, 50, 5) == PLSLAM_OK);
        CHECK(insert(S, 2, 30, 9, &P) == PLSLAM_OK);
        CHECK(P.off_p == 50 && P.off_l == 5);
        CHECK(S.res_p[2] == 30 && S.res_l[2] == 9 && S.p.used == 80 && S.l.used == 14 && S.size == 3);
        CHECK(S.inserted[0] == 0 && S.inserted[1] == 0 && S.inserted[2] == 1);
    });
    run("db_score_plan_capacities_are_the_maximum_over_the_queries", [] {
        BowDbState S = fresh_db(16, 3);
        const int32_t np[4] = {10, 50, 30, 0}, nl[4] = {5, 2, 9, 0};
        for (int32_t k = 0; k < 3; ++k) {
            int32_t a = np[k], b = nl[k];
            double row = 0;
            const plslam_bow_pl_stats st = {k + 100, k + 200, k + 0.5, k + 0.25};
            std::vector<uint8_t> alive(8, 0);
            BowInsertPlan P;
            const int32_t kf = k == 2 ? 4 : k;                         // 0, 1 and 4: 2 and 3 are never inserted
            CHECK(bow_insert_check(S, kf, fake<uint8_t>(0x1000), a, fake<uint8_t>(0x2000), b, &st, alive.data(), &row, true, &P) == PLSLAM_OK);
            CHECK(bow_db_plan_insert(S, kf, a, b, true, &P) == PLSLAM_OK);
            bow_db_commit(S, P, &st);
        }
        double out = 0;
        BowScorePlan P;
        const int32_t q04[2] = {0, 4}, q1[1] = {1}, q2[2] = {1, 2}, q5[1] = {5}, qn[1] = {-1};
        CHECK(bow_score_plan(S, q04, 2, &out, &P) == PLSLAM_OK);
        CHECK(P.nq == 2 && P.n == 5 && P.cap_p == 30 && P.cap_l == 9 && P.score_lds == 39 * 4);
        CHECK(P.st.size() == 2 && P.st[0].n_pt == 100 && P.st[1].n_pt == 102 && P.st[1].std_ls == 2.25);
        CHECK(P.oQ == 0 && P.oS == 256 && P.oO == 512 && P.bytes == 512 + 256);          // 8, 48 and 2 x 5 x 8 bytes
        CHECK(bow_score_plan(S, q1, 1, &out, &P) == PLSLAM_OK && P.cap_p == 50 && P.cap_l == 2);
        CHECK(bow_score_plan(S, q2, 2, &out, &P) == PLSLAM_EINVAL && starts(P.why.fmt, "bow score") && P.why.a == 1 && P.why.b == 2);
        CHECK(bow_score_plan(S, q5, 1, &out, &P) == PLSLAM_EINVAL && P.why.a == 0 && P.why.b == 5);      // >= size
        CHECK(bow_score_plan(S, qn, 1, &out, &P) == PLSLAM_EINVAL);
        CHECK(bow_score_plan(S, nullptr, 1, &out, &P) == PLSLAM_EINVAL && bow_score_plan(S, q1, 1, nullptr, &P) == PLSLAM_EINVAL);
        CHECK(bow_score_plan(S, q1, -1, &out, &P) == PLSLAM_EINVAL);
        CHECK(bow_score_plan(S, nullptr, 0, nullptr, &P) == PLSLAM_OK && P.nq == 0);                     // nothing to do
        CHECK(bow_score_plan(fresh_db(16, 3), q1, 1, nullptr, &P) == PLSLAM_OK && P.n == 0);             // an empty database
        // a P database ignores what the line side holds
        BowDbState T = fresh_db(16, 1);
        CHECK(insert(T, 0, 12, 999) == PLSLAM_OK);
        const int32_t q0[1] = {0};
        CHECK(bow_score_plan(T, q0, 1, &out, &P) == PLSLAM_OK && P.cap_p == 12 && P.cap_l == 0);
    });
    run("db_host_insert_layout_alive_bytes_upload_before_the_words_row_of_doubles", [] {
        const BowDbState S = fresh_db(16, 3);
        BowInsertPlan P;
        CHECK(bow_db_plan_insert(S, 7, 100, 3, true, &P) == PLSLAM_OK);
        // 3200 | 96 | 8 bytes uploaded, then 412 bytes of words and 8 doubles
        CHECK(P.oP == 0 && P.oL == 3328 && P.oA == 3584 && P.up == 3840 && P.oW == 3840 && P.oR == 4352 && P.scratch_bytes == 4608);
        CHECK(P.oL >= P.oP + 100 * 32 && P.oA >= P.oL + 3 * 32 && P.up >= P.oA + 8 && P.up <= P.oW);
        CHECK(P.oR >= P.oW + 103 * 4 && P.scratch_bytes >= P.oR + 8 * 8 && P.pin_in_bytes == P.up && P.pin_out_bytes == 8 * 8);
        CHECK(P.sets_lds == 128 * 4 + 4096 && P.score_lds == 103 * 4);
        for (int32_t kf : {0, 255, 256, 100000}) {
            CHECK(bow_db_plan_insert(S, kf, 1500, 200, true, &P) == PLSLAM_OK);
            CHECK(P.up >= P.oA + (size_t)kf + 1 && P.up <= P.oW && P.scratch_bytes >= P.oR + ((size_t)kf + 1) * 8);
            CHECK(P.pin_out_bytes == ((size_t)kf + 1) * 8 && P.oP % 256 == 0 && P.oL % 256 == 0 && P.oA % 256 == 0 && P.oW % 256 == 0 && P.oR % 256 == 0);
        }
        // the device-pointer call stages nothing: the words alone
        CHECK(bow_db_plan_insert(S, 7, 100, 3, false, &P) == PLSLAM_OK);
        CHECK(P.oW == 0 && P.scratch_bytes == 103 * 4 + 16 && P.pin_in_bytes == 0 && P.pin_out_bytes == 0 && P.up == 0);
        CHECK(P.sets_lds == 128 * 4 + 4096 && P.score_lds == 103 * 4);
    });
    run("db_insert_argument_rules", [] {
        const BowDbState S = fresh_db(16, 3);
        const plslam_bow_pl_stats st = {1, 1, 1.0, 1.0};
        const uint8_t* pd = fake<uint8_t>(0x1000);
        const uint8_t* ld = fake<uint8_t>(0x2000);
        const uint8_t alive[4] = {0, 0, 0, 0};
        double row = 0;
        BowInsertPlan P;
        const auto chk = [&](int32_t kf, const uint8_t* p, int32_t n_p, const uint8_t* l, int32_t n_l, const plslam_bow_pl_stats* s,
                             const uint8_t* al, const double* r, bool host) {
            return bow_insert_check(S, kf, p, n_p, l, n_l, s, al, r, host, &P);
        };
        CHECK(chk(3, pd, 5, ld, 5, &st, alive, &row, true) == PLSLAM_OK);
        CHECK(chk(-1, pd, 5, ld, 5, &st, alive, &row, true) == PLSLAM_EINVAL);
        CHECK(chk(INT32_MAX, pd, 5, ld, 5, &st, alive, &row, false) == PLSLAM_EINVAL);
        CHECK(chk(3, pd, 5, ld, 5, &st, alive, nullptr, true) == PLSLAM_EINVAL);
        CHECK(chk(3, pd, 5, ld, 5, &st, nullptr, &row, true) == PLSLAM_EINVAL);
        CHECK(chk(0, pd, 5, ld, 5, &st, nullptr, &row, true) == PLSLAM_OK);                 // the first keyframe has no earlier one
        CHECK(chk(3, pd, -1, ld, 5, &st, alive, &row, true) == PLSLAM_EINVAL);
        CHECK(chk(3, nullptr, 5, ld, 5, &st, alive, &row, true) == PLSLAM_EINVAL);
        CHECK(chk(3, nullptr, 0, nullptr, 0, &st, alive, &row, true) == PLSLAM_OK);
        CHECK(chk(3, pd, 5, ld, 5, nullptr, alive, &row, true) == PLSLAM_EINVAL);           // PL reads the stats
        CHECK(chk(3, pd, PLSLAM_BOW_MAX_SET, ld, PLSLAM_BOW_MAX_SET, &st, alive, &row, true) == PLSLAM_OK);
        CHECK(chk(3, pd, PLSLAM_BOW_MAX_SET + 1, ld, 5, &st, alive, &row, true) == PLSLAM_ERANGE && starts(P.why.fmt, "bow insert") &&
              P.why.a == PLSLAM_BOW_MAX_SET + 1 && P.why.b == 5);
        CHECK(chk(3, pd, 5, ld, PLSLAM_BOW_MAX_SET + 1, &st, alive, &row, true) == PLSLAM_ERANGE);
        const uint8_t live[4] = {0, 1, 0, 0};                                               // nothing was inserted yet
        CHECK(chk(3, pd, 5, ld, 5, &st, live, &row, true) == PLSLAM_EINVAL && has(P.why.fmt, "never inserted") && P.why.a == 1);
        // the device-pointer call: 16-byte descriptors, an 8-byte row; alive is not read
        CHECK(chk(3, pd, 5, ld, 5, &st, fake<uint8_t>(0x3001), fake<double>(0x4008), false) == PLSLAM_OK);
        CHECK(chk(3, fake<uint8_t>(0x1008), 5, ld, 5, &st, fake<uint8_t>(0x3000), fake<double>(0x4000), false) == PLSLAM_EINVAL);
        CHECK(chk(3, pd, 5, fake<uint8_t>(0x2004), 5, &st, fake<uint8_t>(0x3000), fake<double>(0x4000), false) == PLSLAM_EINVAL);
        CHECK(chk(3, pd, 5, ld, 5, &st, fake<uint8_t>(0x3000), fake<double>(0x4004), false) == PLSLAM_EINVAL);
    });
    return n_failed ? 1 : 0;
}
