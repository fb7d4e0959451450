// bow_train_plan.hpp -- the pure host half of the vocabulary training (bow_train.hip, K111-K130; the contract is in
// include/plslam_bow_train.h): every argument check, the sizes and the carving of the trainer's one device block, the launch
// shapes, the root's path key, the bookkeeping of the tree level by level, the renumbering from level order to DBoW2's node ids
// and the export.  A refusal returns its code and leaves `why`.  No HIP in here: tests/cpp/test_bow_train_plan.cpp compiles it
// with the host compiler alone and runs it under the sanitizers.
//
// Level order: the root is node 0; the children made at level l are numbered on in (visited node, cluster) order.  A node is
// VISITED when HKmeansStep runs on it: the root, and a child with more than one descriptor above level L (TemplatedVocabulary.h
// :774, :791).
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "bow_train_draw.h"
#include "match_tables.hpp"   // Carver
#include "plslam_bow_train.h"

namespace plslam {

constexpr int BT_THREADS = 256;                 // lanes per workgroup of every per-position / per-node kernel
constexpr int BT_SCAN_TILE = 1024;              // items per workgroup of the prefix sum (4 per lane)
constexpr int BT_SCAN_NT = 1024;                // the one workgroup that sums the tiles
constexpr int BT_CNT_STRIDE = 257;              // per (node, cluster): 256 bit counters and the group's size
constexpr int BT_DIST_TILE = 1024;              // distribute_dev.hpp: DIST_TILE (asserted in bow_train.hip)

struct BtWhy {
    const char* fmt = "";
    long a = 0, b = 0;
};
#define BT_REFUSE(cond, code, ...)     \
    do {                               \
        if (cond) {                    \
            P->why = BtWhy{__VA_ARGS__}; \
            return code;               \
        }                              \
    } while (0)
#define BT_REQUIRE(cond) BT_REFUSE(!(cond), PLSLAM_EINVAL, "bow train: requirement failed: " #cond)

inline int32_t bt_blocks(int64_t n) { return (int32_t)((n + BT_THREADS - 1) / BT_THREADS); }
inline int32_t bt_scan_tiles(int64_t n) { return (int32_t)((n + BT_SCAN_TILE - 1) / BT_SCAN_TILE); }
inline int32_t bt_wave_blocks(int64_t waves) { return (int32_t)((waves + BT_THREADS / 64 - 1) / (BT_THREADS / 64)); }

// min(k^e, cap) without overflow
inline int64_t bt_pow_capped(int64_t k, int e, int64_t cap)
{
    int64_t p = 1;
    for (int i = 0; i < e; ++i) {
        if (p > cap / k) return cap;
        p *= k;
    }
    return std::min(p, cap);
}

// ---- the checks and the sizes ---------------------------------------------------------------------------------------------
struct BowTrainPlan {
    int32_t k = 0, L = 0, weighting = 0, max_iters = 0, N = 0, n_docs = 0;
    uint64_t seed = 0, root_key = 0;
    int64_t max_visited = 0;       // visited nodes of one level: the root alone, else at most N / 2 and k^(L-1)
    int64_t max_slots = 0;         // nodes of one level that run k-means (more than k descriptors): at most N / (k + 1)
    int64_t max_items = 0;         // max_visited x k: (node, cluster) pairs of one level
    int64_t tree_cap = 0;          // level-order nodes incl. the root: 1 + sum over l of min(N, k^l)
    size_t counter_bytes = 0;      // the counter table: max_slots x k x BT_CNT_STRIDE words, for the nodes that iterate
    // the device block
    size_t oDesc = 0, oOff = 0, oDoc = 0, oPermA = 0, oPermB = 0, oPnode = 0, oAsg = 0, oMind = 0, oPsum = 0, oTot = 0, oKey = 0,
           oKeyA = 0, oKeyB = 0, oIdTmp = 0, oTable = 0, oIds = 0, oLeaf = 0, oWord = 0, oNbegA = 0, oNbegB = 0, oNkeyA = 0,
           oNkeyB = 0, oNcl = 0, oNrun = 0, oNround = 0, oNchg = 0, oNcap = 0, oNempty = 0, oSnode = 0, oSflag = 0, oSscan = 0,
           oCent = 0, oCnt = 0, oCsize = 0, oCitem = 0, oCscan = 0, oTree = 0, oNi = 0, oStat = 0;
    size_t bytes = 0;
    BtWhy why;
};

inline void bow_train_carve(BowTrainPlan* P, bool own_desc)
{
    const size_t N = (size_t)P->N, V = (size_t)P->max_visited, I = (size_t)P->max_items, k = (size_t)P->k;
    const size_t scan_n = std::max(N, I);
    Carver c;
    P->oDesc = c.take(own_desc ? N * 32 : 0);
    P->oOff = c.take(own_desc ? ((size_t)P->n_docs + 1) * 4 : 0);
    P->oDoc = c.take(N * 4);
    P->oPermA = c.take(N * 4);
    P->oPermB = c.take(N * 4);
    P->oPnode = c.take(N * 4);
    P->oAsg = c.take(N * 4);
    P->oMind = c.take(N * 4);
    P->oPsum = c.take(N * 8);
    P->oTot = c.take(((size_t)bt_scan_tiles((int64_t)scan_n) + 1) * 8);
    P->oKey = c.take(N * 4);
    P->oKeyA = c.take(N * 4);
    P->oKeyB = c.take(N * 4);
    P->oIdTmp = c.take(N * 4);
    P->oTable = c.take((size_t)256 * ((N + BT_DIST_TILE - 1) / BT_DIST_TILE) * 4);
    P->oIds = c.take(N * 4);
    P->oLeaf = c.take(N * 4);
    P->oWord = c.take(N * 4);
    P->oNbegA = c.take((V + 1) * 4);
    P->oNbegB = c.take((V + 1) * 4);
    P->oNkeyA = c.take(V * 8);
    P->oNkeyB = c.take(V * 8);
    P->oNcl = c.take(V * 4);
    P->oNrun = c.take(V * 4);
    P->oNround = c.take(V * 4);
    P->oNchg = c.take(V * 4);
    P->oNcap = c.take(V * 4);
    P->oNempty = c.take(V * 4);
    P->oSnode = c.take(V * 4);
    P->oSflag = c.take(V * 8);
    P->oSscan = c.take(V * 8);
    P->oCent = c.take(I * 32);
    P->counter_bytes = std::max<size_t>(1, (size_t)P->max_slots) * k * BT_CNT_STRIDE * 4;
    P->oCnt = c.take(P->counter_bytes);
    P->oCsize = c.take(I * 4);
    P->oCitem = c.take(I * 8);
    P->oCscan = c.take(I * 8);
    P->oTree = c.take((size_t)P->tree_cap * 32);
    P->oNi = c.take((size_t)P->tree_cap * 4);
    P->oStat = c.take(64);
    P->bytes = c.off;
}

// host_call: the offsets are read (they start at 0, never decrease, N = offsets[n_docs]); else N = n_total and the alignment
inline int bow_train_check(const plslam_bow_train_params* prm, const uint8_t* desc, const int32_t* off, int32_t n_docs,
                           bool host_call, int32_t n_total, BowTrainPlan* P)
{
    *P = BowTrainPlan{};
    BT_REQUIRE(prm && desc && off);
    BT_REFUSE(prm->scoring_type != PLSLAM_BOW_L1_NORM, PLSLAM_ENOTSUP,
              "bow train: scoring type %ld is not supported (only L1_NORM = 0)", prm->scoring_type);
    BT_REFUSE(prm->k < 2 || prm->L < 1, PLSLAM_EINVAL, "bow train: k = %ld (>= 2), L = %ld (>= 1)", prm->k, prm->L);
    BT_REFUSE(prm->k > PLSLAM_BOW_TRAIN_MAX_K || prm->L > PLSLAM_BOW_TRAIN_MAX_L, PLSLAM_ERANGE,
              "bow train: k = %ld, L = %ld beyond PLSLAM_BOW_TRAIN_MAX_K / _MAX_L", prm->k, prm->L);
    BT_REFUSE(prm->weighting_type < PLSLAM_BOW_TF_IDF || prm->weighting_type > PLSLAM_BOW_BINARY, PLSLAM_EINVAL,
              "bow train: weighting type %ld out of range", prm->weighting_type);
    BT_REQUIRE(prm->max_iters >= 0 && n_docs >= 1);
    int64_t N = n_total;
    if (host_call) {
        BT_REFUSE(off[0] != 0, PLSLAM_EINVAL, "bow train: the document offsets start at %ld, not 0", off[0]);
        for (int32_t d = 0; d < n_docs; ++d)
            BT_REFUSE(off[d + 1] < off[d], PLSLAM_EINVAL, "bow train: the offsets decrease behind document %ld", d);
        N = off[n_docs];
    } else {
        BT_REQUIRE(((uintptr_t)desc & 15) == 0 && ((uintptr_t)off & 3) == 0);
    }
    BT_REFUSE(N <= 0, PLSLAM_EINVAL, "bow train: no descriptor to train on (N = %ld)", (long)N);
    BT_REFUSE(N > PLSLAM_BOW_TRAIN_MAX_N, PLSLAM_ERANGE, "bow train: %ld descriptors > PLSLAM_BOW_TRAIN_MAX_N (%ld)", (long)N,
              (long)PLSLAM_BOW_TRAIN_MAX_N);
    P->k = prm->k;
    P->L = prm->L;
    P->weighting = prm->weighting_type;
    P->max_iters = prm->max_iters ? prm->max_iters : PLSLAM_BOW_TRAIN_DEFAULT_MAX_ITERS;
    P->seed = prm->seed;
    P->root_key = bt_root_key(prm->seed);
    P->N = (int32_t)N;
    P->n_docs = n_docs;
    P->max_visited = std::max<int64_t>(1, bt_pow_capped(P->k, P->L - 1, N / 2));
    P->max_slots = std::min<int64_t>(P->max_visited, N / (P->k + 1));
    P->max_items = P->max_visited * P->k;
    BT_REFUSE(P->max_items >= (int64_t)1 << 31, PLSLAM_ERANGE, "bow train: a level's centre table would hold %ld entries (2^31 or more)",
              (long)P->max_items);
    P->tree_cap = 1;
    for (int l = 1; l <= P->L; ++l) P->tree_cap += bt_pow_capped(P->k, l, N);
    bow_train_carve(P, host_call);
    return PLSLAM_OK;
}

// ---- the tree, level by level ----------------------------------------------------------------------------------------------
struct BowTrainLevel {             // what the next pass clusters
    int32_t level = 1;             // 1 .. L
    int32_t n_visited = 1;         // nodes
    int32_t n_rows = 0;            // descriptors in them (the permutation's live length)
    int32_t n_slots = 0;           // nodes with more than k descriptors: the ones that run k-means
    int32_t base = 1;              // level-order id of the level's first child
};

struct BowTrainTree {
    int32_t k = 0, L = 0;
    std::vector<int32_t> parent;       // per level-order node; parent[0] = 0
    std::vector<int32_t> first_child;  // level-order id of the first child, children are contiguous
    std::vector<int32_t> n_child;
    std::vector<int32_t> visited_ids;  // the level-order ids of the CURRENT level's visited nodes, in node-table order
    int64_t rounds = 0, empty = 0, capped = 0;
    int32_t rounds_max = 0, levels = 0;
};

inline BowTrainLevel bow_train_begin(BowTrainTree* T, int32_t k, int32_t L, int32_t N)
{
    *T = BowTrainTree{};
    T->k = k;
    T->L = L;
    T->parent.assign(1, 0);
    T->first_child.assign(1, 0);
    T->n_child.assign(1, 0);
    T->visited_ids.assign(1, 0);
    BowTrainLevel lv;
    lv.n_rows = N;
    lv.n_slots = N > k ? 1 : 0;
    return lv;
}

// Takes a finished level's per-node tables as the device left them (ncl: clusters per visited node; csize: n_visited x k group
// sizes; nround / ncap / nempty: rounds, capped flag and empty-group count per node) and returns the next level.  n_visited == 0
// in the result: the tree is complete.
inline BowTrainLevel bow_train_add_level(BowTrainTree* T, const BowTrainLevel& lv, const int32_t* ncl, const int32_t* csize,
                                         const int32_t* nround, const int32_t* ncap, const int32_t* nempty)
{
    BowTrainLevel nx;
    nx.level = lv.level + 1;
    nx.n_visited = 0;
    std::vector<int32_t> next_ids;
    int32_t id = lv.base;
    for (int32_t v = 0; v < lv.n_visited; ++v) {
        const int32_t me = T->visited_ids[(size_t)v];
        T->first_child[(size_t)me] = id;
        T->n_child[(size_t)me] = ncl[v];
        T->rounds += nround[v];
        T->rounds_max = std::max(T->rounds_max, nround[v]);
        T->capped += ncap[v];
        T->empty += nempty[v];
        for (int32_t c = 0; c < ncl[v]; ++c, ++id) {
            const int32_t n = csize[(size_t)v * T->k + c];
            T->parent.push_back(me);
            T->first_child.push_back(0);
            T->n_child.push_back(0);
            if (lv.level < T->L && n > 1) {
                next_ids.push_back(id);
                nx.n_rows += n;
                nx.n_slots += n > T->k;
            }
        }
    }
    nx.base = id;
    nx.n_visited = (int32_t)next_ids.size();
    T->visited_ids.swap(next_ids);
    T->levels = lv.level;
    return nx;
}

// DBoW2's node ids: a node's children get consecutive ids when the node is clustered, then each child that is clustered is
// walked in order (HKmeansStep's recursion).  dbow[level-order id] = node id; the root stays 0.
inline std::vector<int32_t> bow_train_renumber(const BowTrainTree& T)
{
    const size_t n = T.parent.size();
    std::vector<int32_t> dbow(n, 0);
    std::vector<std::pair<int32_t, int32_t>> stack;   // (node, the next child to walk)
    int32_t next = 1;
    for (int32_t c = 0; c < T.n_child[0]; ++c) dbow[(size_t)T.first_child[0] + c] = next++;
    stack.push_back({0, 0});
    while (!stack.empty()) {
        auto& top = stack.back();
        if (top.second >= T.n_child[(size_t)top.first]) {
            stack.pop_back();
            continue;
        }
        const int32_t ch = T.first_child[(size_t)top.first] + top.second++;
        if (T.n_child[(size_t)ch] == 0) continue;
        for (int32_t c = 0; c < T.n_child[(size_t)ch]; ++c) dbow[(size_t)T.first_child[(size_t)ch] + c] = next++;
        stack.push_back({ch, 0});
    }
    return dbow;
}

// The records in ascending node id, without the root (weights 0), the words ascending over the leaves by node id
// (createWords), and word_of[level-order id] (-1: an inner node).  tree_desc: 32 bytes per level-order node.
struct BowTrainExport {
    std::vector<plslam_bow_node> nodes;
    std::vector<plslam_bow_word> words;
    std::vector<int32_t> dbow, word_of;
};
inline void bow_train_export(const BowTrainTree& T, const uint8_t* tree_desc, BowTrainExport* E)
{
    const size_t n = T.parent.size();
    E->dbow = bow_train_renumber(T);
    E->nodes.assign(n - 1, plslam_bow_node{});
    E->word_of.assign(n, -1);
    E->words.clear();
    std::vector<int32_t> lo_of(n, 0);
    for (size_t i = 1; i < n; ++i) lo_of[(size_t)E->dbow[i]] = (int32_t)i;
    for (size_t d = 1; d < n; ++d) {
        const size_t i = (size_t)lo_of[d];
        plslam_bow_node& r = E->nodes[d - 1];
        r.node_id = (int32_t)d;
        r.parent_id = E->dbow[(size_t)T.parent[i]];
        r.weight = 0.0;
        std::memcpy(r.descriptor, tree_desc + 32 * i, 32);
        if (T.n_child[i] == 0) {
            E->word_of[i] = (int32_t)E->words.size();
            E->words.push_back(plslam_bow_word{(int32_t)E->words.size(), (int32_t)d});
        }
    }
}

// setNodeWeights (:923-976): TF and BINARY 1; IDF and TF_IDF log(NDocs / Ni) where Ni > 0, else 0 (libm's log on the host)
inline void bow_train_weights(BowTrainExport* E, int32_t weighting, int32_t n_docs, const int32_t* ni)
{
    for (const plslam_bow_word& w : E->words) {
        double x = 1.0;
        if (weighting == PLSLAM_BOW_TF_IDF || weighting == PLSLAM_BOW_IDF)
            x = ni[w.word_id] > 0 ? std::log((double)n_docs / (double)ni[w.word_id]) : 0.0;
        E->nodes[(size_t)w.node_id - 1].weight = x;
    }
}

#undef BT_REQUIRE
#undef BT_REFUSE

}  // namespace plslam
