// bow_plan.hpp -- the pure host half of the bag-of-words entry points (bow.hip, K19-K21; the contract is in
// include/plslam_hip.h): every argument check, the flattening of a caller's vocabulary tree into the arrays the kernels read,
// the launch geometry and LDS sizes, the layouts of the staged blocks, and the bookkeeping of a database (sizes, capacities,
// what each keyframe reserved) with the growth rule.  A refusal returns its code and leaves `why` in the plan: the text
// set_last_error gets, with its two arguments.  No HIP in here: tests/cpp/test_bow_plan.cpp compiles it with the host
// compiler alone and runs it under the sanitizers.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#include "match_tables.hpp"   // Carver, align256
#include "plslam_hip.h"

namespace plslam {

// ---- constants and geometry ------------------------------------------------------------------------------------------
constexpr int STAGE_NODES = 1228;          // 1228 x (32 + 8) B = 48 KB of LDS: no dynamic-LDS attribute needed for K19
constexpr int DESCEND_THREADS = 256;
constexpr int SET_THREADS = 1024;
constexpr uint32_t NO_WORD = 0xFFFFFFFFu;  // sorts behind every word id (< 2^31)
constexpr size_t SET_LDS_MAX = (size_t)PLSLAM_BOW_MAX_SET * 4 + SET_THREADS * 4 + 16;
constexpr size_t SCORE_LDS_MAX = (size_t)2 * PLSLAM_BOW_MAX_SET * 4;

inline size_t bow_stage_bytes(int32_t n_stage) { return (size_t)n_stage * 40; }                       // K19: desc + links
inline int32_t bow_descend_blocks(int32_t n) { return (n + DESCEND_THREADS - 1) / DESCEND_THREADS; }  // K19: a lane per row
inline size_t bow_set_lds(int32_t max_set)                                                            // K20: keys + the scan
{
    int P = 1;
    while (P < max_set) P <<= 1;
    return (size_t)P * 4 + SET_THREADS * 4;
}
inline size_t bow_score_lds(int32_t cap_p, int32_t cap_l) { return std::max<size_t>(16, ((size_t)cap_p + (size_t)cap_l) * 4); }
inline unsigned bow_score_grid_x(int32_t ntarget) { return (unsigned)((ntarget + 3) / 4); }           // K21: a wave per target

struct BowWhy {                            // what was refused: set_last_error(fmt, a, b)
    const char* fmt = "";
    long a = 0, b = 0;
};
#define BOW_REFUSE(cond, code, ...)        \
    do {                                   \
        if (cond) {                        \
            P->why = BowWhy{__VA_ARGS__};  \
            return code;                   \
        }                                  \
    } while (0)
#define BOW_REQUIRE(cond) BOW_REFUSE(!(cond), PLSLAM_EINVAL, "bow: requirement failed: " #cond)

// ---- the vocabulary ----------------------------------------------------------------------------------------------------
struct BowVocabFlat {                      // the four arrays as they are uploaded (bow.hip: Layout)
    int32_t n = 0, n_words = 0, n_stage = 0;
    std::vector<int32_t> links;            // n x {first child, count}; a leaf {word id, 0}
    std::vector<uint8_t> desc;             // n x 32
    std::vector<double> node_w, word_w;    // n, n_words
    BowWhy why;
};

// Validates load()'s records and re-orders the nodes breadth first, every parent's children contiguous in RECORD order.
// PLSLAM_OK, PLSLAM_EINVAL or PLSLAM_ENOTSUP.
inline int bow_vocab_flatten(const plslam_bow_vocab_desc* d, BowVocabFlat* P)
{
    *P = BowVocabFlat{};
    BOW_REQUIRE(d);
    const int32_t N = d->n_nodes, W = d->n_words;
    BOW_REFUSE(N <= 0 || W <= 0, PLSLAM_EINVAL, "bow vocabulary: empty (%ld nodes, %ld words)", N, W);
    BOW_REQUIRE(d->nodes && d->words);
    BOW_REFUSE(d->scoring_type != PLSLAM_BOW_L1_NORM, PLSLAM_ENOTSUP,
               "bow vocabulary: scoring type %ld is not supported (only L1_NORM = 0)", d->scoring_type);
    BOW_REFUSE(d->weighting_type < PLSLAM_BOW_TF_IDF || d->weighting_type > PLSLAM_BOW_BINARY, PLSLAM_EINVAL,
               "bow vocabulary: weighting type %ld out of range", d->weighting_type);
    // children lists in file order (TemplatedVocabulary.h:1470 m_nodes[pid].children.push_back(nid)), as CSR
    std::vector<int32_t> rec_of((size_t)N + 1, -1), nchild((size_t)N + 2, 0);
    for (int32_t r = 0; r < N; ++r) {
        const int32_t id = d->nodes[r].node_id, pid = d->nodes[r].parent_id;
        BOW_REFUSE(id < 1 || id > N, PLSLAM_EINVAL, "bow vocabulary: node id %ld out of range 1..%ld", id, N);
        BOW_REFUSE(rec_of[id] >= 0, PLSLAM_EINVAL, "bow vocabulary: duplicate node id %ld", id);
        BOW_REFUSE(pid < 0 || pid > N, PLSLAM_EINVAL, "bow vocabulary: parent %ld of node %ld is not a node", pid, id);
        BOW_REFUSE(pid == id, PLSLAM_EINVAL, "bow vocabulary: node %ld is its own parent (cycle)", id);
        rec_of[id] = r;
        ++nchild[pid + 1];
    }
    std::vector<int32_t> first((size_t)N + 2, 0);
    for (int32_t i = 0; i <= N; ++i) first[i + 1] = first[i] + nchild[i + 1];
    std::vector<int32_t> kids((size_t)N), fill(first.begin(), first.end() - 1);
    for (int32_t r = 0; r < N; ++r) kids[fill[d->nodes[r].parent_id]++] = d->nodes[r].node_id;
    // words
    std::vector<int32_t> word_of((size_t)N + 1, -1), node_of_word((size_t)W, -1);
    for (int32_t r = 0; r < W; ++r) {
        const int32_t wid = d->words[r].word_id, nid = d->words[r].node_id;
        BOW_REFUSE(wid < 0 || wid >= W, PLSLAM_EINVAL, "bow vocabulary: word id %ld out of range 0..%ld", wid, W - 1);
        BOW_REFUSE(nid < 1 || nid > N, PLSLAM_EINVAL, "bow vocabulary: word %ld names node %ld, not a node", wid, nid);
        BOW_REFUSE(node_of_word[wid] >= 0, PLSLAM_EINVAL, "bow vocabulary: duplicate word id %ld", wid);
        BOW_REFUSE(word_of[nid] >= 0, PLSLAM_EINVAL, "bow vocabulary: node %ld carries two words", nid);
        node_of_word[wid] = nid;
        word_of[nid] = wid;
    }
    // breadth-first order from the root: every parent's children contiguous, in list order.  Every node is in exactly one
    // children list, so the walk visits at most N + 1 nodes; those on a cycle hang off no list the root reaches.
    std::vector<int32_t> order;
    order.reserve((size_t)N + 1);
    order.push_back(0);
    for (size_t h = 0; h < order.size(); ++h) {
        const int32_t u = order[h];
        for (int32_t c = first[u]; c < first[u + 1]; ++c) order.push_back(kids[c]);
    }
    BOW_REFUSE(order.size() != (size_t)N + 1, PLSLAM_EINVAL,
               "bow vocabulary: %ld of %ld nodes are not reachable from the root (a cycle)", (long)N + 1 - (long)order.size(), N);
    std::vector<int32_t> pos((size_t)N + 1);
    for (int32_t i = 0; i <= N; ++i) {
        const int32_t u = order[i];
        BOW_REFUSE(first[u + 1] == first[u] && word_of[u] < 0, PLSLAM_EINVAL, "bow vocabulary: leaf node %ld has no word", u);
        pos[u] = i;
    }
    P->links.assign((size_t)2 * ((size_t)N + 1), 0);
    P->desc.assign((size_t)32 * ((size_t)N + 1), 0);
    P->node_w.assign((size_t)N + 1, 0.0);
    P->word_w.assign((size_t)W, 0.0);
    for (int32_t i = 0; i <= N; ++i) {
        const int32_t u = order[i], nc = first[u + 1] - first[u];
        P->links[2 * (size_t)i] = nc ? pos[kids[first[u]]] : word_of[u];
        P->links[2 * (size_t)i + 1] = nc;
        if (u > 0) {
            std::memcpy(&P->desc[32 * (size_t)i], d->nodes[rec_of[u]].descriptor, 32);
            P->node_w[i] = d->nodes[rec_of[u]].weight;
        }
    }
    for (int32_t w = 0; w < W; ++w) P->word_w[w] = d->nodes[rec_of[node_of_word[w]]].weight;
    P->n = N + 1;
    P->n_words = W;
    P->n_stage = std::min(N + 1, STAGE_NODES);
    return PLSLAM_OK;
}

// ---- transform -----------------------------------------------------------------------------------------------------------
struct BowTransformCheck {
    int32_t nsets = 0, max_set = 0, total = 0;   // nsets == 0: nothing to do
    BowWhy why;
};

// the host call: the offsets scan
inline int bow_transform_check_host(const uint8_t* desc, const int32_t* offsets, int32_t nsets, const int32_t* bow_len,
                                    BowTransformCheck* P)
{
    *P = BowTransformCheck{};
    BOW_REQUIRE(nsets >= 0);
    if (nsets == 0) return PLSLAM_OK;
    BOW_REQUIRE(offsets && bow_len && offsets[0] == 0);
    for (int32_t s = 0; s < nsets; ++s) {
        const int64_t n = (int64_t)offsets[s + 1] - offsets[s];
        BOW_REQUIRE(n >= 0);
        BOW_REFUSE(n > PLSLAM_BOW_MAX_SET, PLSLAM_ERANGE, "bow transform: set of %ld descriptors > PLSLAM_BOW_MAX_SET (%ld)",
                   (long)n, PLSLAM_BOW_MAX_SET);
        P->max_set = std::max<int32_t>(P->max_set, (int32_t)n);
    }
    P->total = offsets[nsets];
    BOW_REQUIRE(P->total == 0 || desc);
    P->nsets = nsets;
    return PLSLAM_OK;
}

// the device-pointer call: sizes from the caller, nothing is read through a pointer
inline int bow_transform_check_dev(const uint8_t* desc, const int32_t* offsets, int32_t nsets, int32_t total, int32_t max_set,
                                   const int32_t* word_id, const int32_t* bow_word, const double* bow_weight,
                                   const int32_t* bow_len, BowTransformCheck* P)
{
    *P = BowTransformCheck{};
    BOW_REQUIRE(nsets >= 0 && total >= 0 && max_set >= 0);
    BOW_REFUSE(max_set > PLSLAM_BOW_MAX_SET, PLSLAM_ERANGE, "bow transform: max_set %ld > PLSLAM_BOW_MAX_SET (%ld)", max_set,
               PLSLAM_BOW_MAX_SET);
    if (nsets == 0) return PLSLAM_OK;
    BOW_REQUIRE(offsets && word_id && bow_word && bow_weight && bow_len && (total == 0 || desc));
    BOW_REQUIRE(((uintptr_t)desc & 15) == 0);
    P->nsets = nsets;
    P->total = total;
    P->max_set = max_set;
    return PLSLAM_OK;
}

struct BowTransformLayout {                // the host call's slices of the context's staging buffer
    size_t oD = 0, oO = 0;                 // uploaded: descriptors, offsets
    size_t oW = 0, oV = 0, oBW = 0, oBV = 0, oL = 0;   // per descriptor word / weight; per set the vector's words / weights, its length
    size_t bytes = 0;
};
inline BowTransformLayout bow_transform_layout(int32_t nsets, int32_t total)
{
    BowTransformLayout L;
    Carver c;
    L.oD = c.take((size_t)total * 32);
    L.oO = c.take(((size_t)nsets + 1) * 4);
    L.oW = c.take((size_t)total * 4);
    L.oV = c.take((size_t)total * 8);
    L.oBW = c.take((size_t)total * 4);
    L.oBV = c.take((size_t)total * 8);
    L.oL = c.take((size_t)nsets * 4);
    L.bytes = c.off;
    return L;
}

// ---- the database --------------------------------------------------------------------------------------------------------
struct BowPool {                           // one pool of stored vectors: two device arrays (word ids, weights), ONE capacity
    int64_t cap = 0, used = 0;             // entries
};
struct BowDbState {                        // the bookkeeping of a database, without any buffer
    int mode = 0;                          // 1 P, 2 L, 3 PL
    int32_t size = 0;                      // 1 + the largest keyframe index inserted
    int64_t cap_kf = 0;                    // rows of the keyframe table
    BowPool p, l;
    std::vector<int32_t> res_p, res_l;     // entries reserved per keyframe
    std::vector<uint8_t> inserted;
    std::vector<plslam_bow_pl_stats> stats;
};

// the doubling rule, stated once
inline int64_t bow_grow_to(int64_t have, int64_t need) { return std::max(need, 2 * have); }

struct BowGrow {                           // one array set across an insert
    int64_t cap = 0;                       // the capacity after it; equal to the state's: no growth
    int64_t keep = 0;                      // entries carried over into a grown array (what is in use, not the old capacity)
};
struct BowInsertPlan {
    int32_t kf_idx = -1;                   // -1: the plan of bow_db_initial, no keyframe
    int32_t n_p = 0, n_l = 0;
    int64_t off_p = 0, off_l = 0;          // where the keyframe's vectors go in the pools
    BowGrow tab, p, l;
    // the host call's staged block in `scratch`: uploaded [descriptors P | L | alive], then the words and the row; the
    // device-pointer call has the words alone (oW = 0)
    size_t oP = 0, oL = 0, oA = 0, up = 0, oW = 0, oR = 0;
    size_t scratch_bytes = 0, pin_in_bytes = 0, pin_out_bytes = 0;
    size_t sets_lds = 0, score_lds = 0;    // K20, K21
    BowWhy why;
};

// The capacities a new database allocates: max(hint, 16) keyframes, x 256 point entries, x 64 line entries.
inline BowInsertPlan bow_db_initial(int32_t capacity_hint, int mode)
{
    BowInsertPlan P;
    const int64_t cap = std::max<int32_t>(capacity_hint, 16);
    P.tab.cap = cap;
    if (mode & 1) P.p.cap = cap * 256;
    if (mode & 2) P.l.cap = cap * 64;
    return P;
}

// The argument rules of both insert calls; the counts of an absent modality become 0.  host_call: alive is host memory and
// every live earlier keyframe must have been inserted; else the alignment the kernels need of the device pointers.
inline int bow_insert_check(const BowDbState& S, int32_t kf_idx, const uint8_t* pdesc, int32_t& n_p, const uint8_t* ldesc,
                            int32_t& n_l, const plslam_bow_pl_stats* stats, const uint8_t* alive, const double* row,
                            bool host_call, BowInsertPlan* P)
{
    BOW_REQUIRE(kf_idx >= 0 && kf_idx < INT32_MAX && row && (kf_idx == 0 || alive));
    if (!(S.mode & 1)) n_p = 0;
    if (!(S.mode & 2)) n_l = 0;
    BOW_REQUIRE(n_p >= 0 && n_l >= 0 && (n_p == 0 || pdesc) && (n_l == 0 || ldesc));
    BOW_REQUIRE(S.mode != 3 || stats);
    BOW_REFUSE(n_p > PLSLAM_BOW_MAX_SET || n_l > PLSLAM_BOW_MAX_SET, PLSLAM_ERANGE,
               "bow insert: %ld point / %ld line descriptors; at most PLSLAM_BOW_MAX_SET each", n_p, n_l);
    if (!host_call) {
        BOW_REQUIRE(((uintptr_t)pdesc & 15) == 0 && ((uintptr_t)ldesc & 15) == 0 && ((uintptr_t)row & 7) == 0);
        return PLSLAM_OK;
    }
    for (int32_t i = 0; i < kf_idx; ++i)
        BOW_REFUSE(alive[i] && (i >= (int32_t)S.inserted.size() || !S.inserted[i]), PLSLAM_EINVAL,
                   "bow insert: keyframe %ld is alive but was never inserted", i);
    return PLSLAM_OK;
}

// What one insert needs of the device half; S is not modified (bow_db_commit does that, after the device half is through).
inline int bow_db_plan_insert(const BowDbState& S, int32_t kf_idx, int32_t n_p, int32_t n_l, bool host_call, BowInsertPlan* P)
{
    *P = BowInsertPlan{};
    BOW_REFUSE(S.p.used + n_p > INT32_MAX || S.l.used + n_l > INT32_MAX, PLSLAM_ERANGE,
               "bow database: more than 2^31 stored entries");
    P->kf_idx = kf_idx;
    P->n_p = n_p;
    P->n_l = n_l;
    P->off_p = S.p.used;
    P->off_l = S.l.used;
    const auto grown = [](int64_t cap, int64_t need, int64_t used) {
        return BowGrow{need <= cap ? cap : bow_grow_to(cap, need), used};
    };
    P->tab = grown(S.cap_kf, (int64_t)kf_idx + 1, S.size);
    P->p = (S.mode & 1) ? grown(S.p.cap, S.p.used + n_p, S.p.used) : BowGrow{S.p.cap, 0};
    P->l = (S.mode & 2) ? grown(S.l.cap, S.l.used + n_l, S.l.used) : BowGrow{S.l.cap, 0};
    const size_t row_bytes = ((size_t)kf_idx + 1) * 8, words_bytes = ((size_t)n_p + (size_t)n_l) * 4;
    if (host_call) {
        Carver c;
        P->oP = c.take((size_t)n_p * 32);
        P->oL = c.take((size_t)n_l * 32);
        P->oA = c.take((size_t)kf_idx + 1);
        P->up = c.off;
        P->oW = c.take(words_bytes);
        P->oR = c.take(row_bytes);
        P->scratch_bytes = c.off;
        P->pin_in_bytes = P->up;
        P->pin_out_bytes = row_bytes;
    } else {
        P->scratch_bytes = words_bytes + 16;
    }
    P->sets_lds = bow_set_lds(std::max(n_p, n_l));
    P->score_lds = bow_score_lds(n_p, n_l);
    return PLSLAM_OK;
}

// Records a plan the device half has carried out: the capacities (every grown array replaced, both arrays of a pool), and
// for a keyframe what it reserved.  An index inserted again overwrites its reservation and still advances `used`.
inline void bow_db_commit(BowDbState& S, const BowInsertPlan& P, const plslam_bow_pl_stats* stats)
{
    S.cap_kf = P.tab.cap;
    S.p.cap = P.p.cap;
    S.l.cap = P.l.cap;
    if (P.kf_idx < 0) return;
    const size_t k = (size_t)P.kf_idx;
    if (S.inserted.size() <= k) {
        S.res_p.resize(k + 1, 0);
        S.res_l.resize(k + 1, 0);
        S.inserted.resize(k + 1, 0);
        S.stats.resize(k + 1, plslam_bow_pl_stats{0, 0, 0.0, 0.0});
    }
    if (S.mode & 1) { S.res_p[k] = P.n_p; S.p.used += P.n_p; }
    if (S.mode & 2) { S.res_l[k] = P.n_l; S.l.used += P.n_l; }
    S.inserted[k] = 1;
    S.stats[k] = stats ? *stats : plslam_bow_pl_stats{0, 0, 0.0, 0.0};
    S.size = std::max(S.size, P.kf_idx + 1);
}

struct BowScorePlan {
    int32_t nq = 0, n = 0;                 // either 0: nothing to do
    int32_t cap_p = 0, cap_l = 0;          // the longest query vectors: K21's LDS entries
    std::vector<plslam_bow_pl_stats> st;   // per query
    size_t oQ = 0, oS = 0, oO = 0, bytes = 0;      // `scratch`: the queries, their stats, the nq x n scores
    size_t score_lds = 0;
    BowWhy why;
};
inline int bow_score_plan(const BowDbState& S, const int32_t* queries, int32_t nq, const double* out, BowScorePlan* P)
{
    *P = BowScorePlan{};
    BOW_REQUIRE(nq >= 0);
    if (nq == 0 || S.size == 0) return PLSLAM_OK;
    BOW_REQUIRE(queries && out);
    P->st.resize((size_t)nq);
    for (int32_t q = 0; q < nq; ++q) {
        const int32_t k = queries[q];
        BOW_REFUSE(k < 0 || k >= S.size || !S.inserted[k], PLSLAM_EINVAL, "bow score: query %ld (keyframe %ld) was never inserted",
                   q, k);
        P->cap_p = std::max(P->cap_p, (S.mode & 1) ? S.res_p[k] : 0);
        P->cap_l = std::max(P->cap_l, (S.mode & 2) ? S.res_l[k] : 0);
        P->st[q] = S.stats[k];
    }
    P->nq = nq;
    P->n = S.size;
    Carver c;
    P->oQ = c.take((size_t)nq * 4);
    P->oS = c.take((size_t)nq * sizeof(plslam_bow_pl_stats));
    P->oO = c.take((size_t)nq * P->n * 8);
    P->bytes = c.off;
    P->score_lds = bow_score_lds(P->cap_p, P->cap_l);
    return PLSLAM_OK;
}

#undef BOW_REQUIRE
#undef BOW_REFUSE

}  // namespace plslam
