// K19-K21 -- bag of words on the device: DBoW2 vocabulary transform and the keyframe confusion-matrix row.
//
// Reference: MapHandler::insertKFBowVector{P,L,PL}, src/mapHandler.cpp:3007-3128, called on every keyframe from
// addKeyFrame (:196-201):
//   TemplatedVocabulary<FORB>::transform(features, BowVector&)   3rdparty/DBoW2/include/DBoW2/TemplatedVocabulary.h:1046-1100
//     per feature: descend from the root; at each node the child with the smallest FORB::distance wins, strict '<' over
//     the children list in load() order, so the FIRST child wins a tie                                          :1198-1240
//     stopped words (`w > 0` fails) are dropped; TF / TF_IDF: BowVector::addWeight, IDF / BINARY: addIfNotExist
//     (src/DBoW2/BowVector.cpp:33-59); then normalize(L1): norm = sum of fabs in ascending word id order, divide only if
//     norm > 0 (BowVector.cpp:62-84)
//   L1Scoring::score(v1, v2)   src/DBoW2/ScoringObject.cpp:23-67: over the common words in ascending id order
//     score += fabs(vi - wi) - fabs(vi) - fabs(wi); then -score / 2.0
//   PL: score = 0.0; score += (sp*n_pt + sl*n_ls)/n_pl; score += (sp*std_pt + sl*std_ls)/std_pl   mapHandler.cpp:3100-3127
//
// Layout (plslam_bow_vocab): the nodes re-ordered breadth first, each parent's children contiguous IN LIST ORDER (never
// sorted by id): links[i] = {first child, child count}, a leaf {word id, 0}; desc[i] = 32 bytes; node_w[i]; word_w[word].
// The first STAGE_NODES nodes (the top levels: root + k + k^2 + k^3 for k = 10) are staged in LDS by every workgroup of K19.
//
// K19 k_bow_descend   one lane per descriptor, descriptor in 8 VGPRs; level 1 is uniform across lanes (LDS broadcast), deeper
//                     levels read k x 32 contiguous bytes per step, from LDS while staged, then global (L2 / Infinity Cache).
// K20 k_bow_sets      one 1024-lane workgroup per set: LDS bitonic sort of the word ids (stopped words as +inf), runs by a
//                     block scan, per run the sequential fold w + w + ... + w (TF, TF_IDF) or w (IDF, BINARY), the L1 norm
//                     summed sequentially in ascending word order by one wave, then the division.
// K21 k_bow_score     one wave per (query, stored keyframe): the query's word ids in LDS, the stored vector streamed 64 entries
//                     at a time, each lane binary-searches its word; the common words' terms are added in lane order (=
//                     ascending word id) through ballot + shuffles.  All three folds run in the reference's order: the
//                     results are bit-identical to it (-ffp-contract=off).
// One keyframe insert = 1 H2D copy, K19, K20, K21, 1 D2H copy, 1 synchronisation (DESIGN.md section "Bag of words").
//
// The kernels, the handles with their buffers and the launches are here.  Every check, the flattening of the vocabulary tree,
// the database's bookkeeping, the staged layouts and the LDS sizes are in bow_plan.hpp (pure host): an entry point reads
// check (planner) -> lock and guard -> reserve and stage by the plan -> launch -> commit.
#include "common.hpp"

#include <cstring>

#include "bow_plan.hpp"   // STAGE_NODES, DESCEND_THREADS, SET_THREADS, NO_WORD, the LDS sizes; the planner

namespace plslam {
namespace {

struct VocabDev {                          // what the kernels read of one vocabulary
    const int32_t* links;                  // n x {first, count}
    const uint32_t* desc;                  // n x 8 words
    const double* node_w;                  // n
    const double* word_w;                  // n_words
    int32_t n_stage;
};

struct DescendJob {
    VocabDev v;
    const uint32_t* q;                     // n x 8 words
    int32_t n, nblocks;
    int32_t* word;
    double* weight;                        // may be nullptr
};

__device__ __forceinline__ int dist8(const uint32_t (&q)[8], gvec4_t a, gvec4_t b)
{
    return __popc(q[0] ^ a.x) + __popc(q[1] ^ a.y) + __popc(q[2] ^ a.z) + __popc(q[3] ^ a.w) + __popc(q[4] ^ b.x) +
           __popc(q[5] ^ b.y) + __popc(q[6] ^ b.z) + __popc(q[7] ^ b.w);
}

__global__ __launch_bounds__(DESCEND_THREADS) void k_bow_descend(DescendJob j0, DescendJob j1)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
    const bool second = (int)blockIdx.x >= j0.nblocks;
    const DescendJob J = second ? j1 : j0;
    const int blk = second ? (int)blockIdx.x - j0.nblocks : (int)blockIdx.x;
    const int ns = J.v.n_stage;
    gvec4_t* s_desc = reinterpret_cast<gvec4_t*>(smem);                       // ns x 2
    int32_t* s_links = reinterpret_cast<int32_t*>(smem + (size_t)ns * 8);     // ns x 2
    for (int i = threadIdx.x; i < ns * 2; i += DESCEND_THREADS) {
        s_desc[i] = g_(reinterpret_cast<const gvec4_t*>(J.v.desc))[i];
        s_links[i] = g_(J.v.links)[i];
    }
    __syncthreads();
    const int t = blk * DESCEND_THREADS + (int)threadIdx.x;
    if (t >= J.n) return;
    uint32_t q[8];
    {
        const gvec4_t a = g_(reinterpret_cast<const gvec4_t*>(J.q))[(size_t)t * 2];
        const gvec4_t b = g_(reinterpret_cast<const gvec4_t*>(J.q))[(size_t)t * 2 + 1];
        q[0] = a.x; q[1] = a.y; q[2] = a.z; q[3] = a.w; q[4] = b.x; q[5] = b.y; q[6] = b.z; q[7] = b.w;
    }
    const gvec4_t* gd = reinterpret_cast<const gvec4_t*>(J.v.desc);
    int node = 0, first, count;
    for (;;) {
        if (node < ns) { first = s_links[2 * node]; count = s_links[2 * node + 1]; }
        else { first = g_(J.v.links)[2 * (size_t)node]; count = g_(J.v.links)[2 * (size_t)node + 1]; }
        if (count == 0) break;                                     // a leaf: `first` is its word id
        int best = first, best_d = 1 << 30;
        for (int c = first; c < first + count; ++c) {
            const int d = c < ns ? dist8(q, s_desc[2 * c], s_desc[2 * c + 1])
                                 : dist8(q, g_(gd)[2 * (size_t)c], g_(gd)[2 * (size_t)c + 1]);
            if (d < best_d) { best_d = d; best = c; }             // strict '<': the first child of the list wins a tie
        }
        node = best;
    }
    g_(J.word)[t] = first;
    if (J.weight) g_(J.weight)[t] = g_(J.v.node_w)[node];
}

struct SetJob {
    const int32_t* off;                    // nsets + 1 device offsets, or nullptr: one set of n rows
    int32_t n, nsets, max_set, weighting;
    const int32_t* dword;                  // per-descriptor word ids (K19)
    const double* word_w;
    int32_t* out_word;                     // set s: entries off[s] ..
    double* out_w;
    int32_t* out_len;                      // nsets entries, or nullptr
    int32_t* kf_slot;                      // database: {offset, length} of this keyframe's vector, or nullptr
    int32_t kf_off;
};

__global__ __launch_bounds__(SET_THREADS) void k_bow_sets(SetJob j0, SetJob j1)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
    __shared__ double s_norm;
    const bool second = (int)blockIdx.x >= j0.nsets;
    const SetJob J = second ? j1 : j0;
    const int s = second ? (int)blockIdx.x - j0.nsets : (int)blockIdx.x;
    const int tid = threadIdx.x;
    const int32_t base = J.off ? g_(J.off)[s] : 0;
    const int32_t n = J.off ? g_(J.off)[s + 1] - base : J.n;
    if (n < 0 || n > J.max_set) {                                  // the caller's bound was wrong: no vector
        if (tid == 0) {
            if (J.out_len) g_(J.out_len)[s] = -1;
            if (J.kf_slot) { g_(J.kf_slot)[0] = J.kf_off; g_(J.kf_slot)[1] = -1; }
        }
        return;
    }
    int P = 1;
    while (P < n) P <<= 1;
    uint32_t* key = smem;                                          // P
    int32_t* scan = reinterpret_cast<int32_t*>(smem + P);          // SET_THREADS
    for (int i = tid; i < P; i += SET_THREADS) {
        uint32_t k = NO_WORD;
        if (i < n) {
            const int32_t w = g_(J.dword)[base + i];
            if (g_(J.word_w)[w] > 0) k = (uint32_t)w;              // TemplatedVocabulary.h:1074,1093: `if(w > 0)`
        }
        key[i] = k;
    }
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < P; i += SET_THREADS) {
                const int ixj = i ^ j;
                if (ixj > i) {
                    const uint32_t a = key[i], b = key[ixj];
                    if ((a > b) == ((i & k) == 0)) { key[i] = b; key[ixj] = a; }
                }
            }
            __syncthreads();
        }
    // runs: each lane owns a contiguous chunk of the sorted keys and counts the run starts in it
    const int chunk = (P + SET_THREADS - 1) / SET_THREADS;
    const int c0 = tid * chunk, c1 = min(c0 + chunk, P);
    int starts = 0;
    for (int i = c0; i < c1; ++i) starts += key[i] != NO_WORD && (i == 0 || key[i] != key[i - 1]);
    scan[tid] = starts;
    __syncthreads();
    for (int d = 1; d < SET_THREADS; d <<= 1) {                    // inclusive Hillis-Steele scan
        const int v = tid >= d ? scan[tid - d] : 0;
        __syncthreads();
        scan[tid] += v;
        __syncthreads();
    }
    const int R = scan[SET_THREADS - 1];
    int r = scan[tid] - starts;
    const bool tf = J.weighting == PLSLAM_BOW_TF_IDF || J.weighting == PLSLAM_BOW_TF;
    for (int i = c0; i < c1; ++i) {
        const uint32_t w = key[i];
        if (w == NO_WORD || (i > 0 && key[i - 1] == w)) continue;
        const double ww = g_(J.word_w)[w];
        double acc = ww;                                           // BowVector::insert of the first hit
        if (tf)
            for (int e = i + 1; e < P && key[e] == w; ++e) acc += ww;   // addWeight: vit->second += v, hit by hit
        g_(J.out_word)[base + r] = (int32_t)w;
        g_(J.out_w)[base + r] = acc;
        ++r;
    }
    __syncthreads();
    // normalize(L1): norm += fabs(w) in ascending word order (one wave, lane order through shuffles)
    if (tid < 64) {
        double norm = 0.0;
        for (int b = 0; b < R; b += 64) {
            const double v = b + tid < R ? fabs(g_(J.out_w)[base + b + tid]) : 0.0;
            const int cnt = min(64, R - b);
            for (int e = 0; e < cnt; ++e) norm += __shfl(v, e);
        }
        if (tid == 0) s_norm = norm;
    }
    __syncthreads();
    const double norm = s_norm;
    if (norm > 0.0)
        for (int i = tid; i < R; i += SET_THREADS) g_(J.out_w)[base + i] = g_(J.out_w)[base + i] / norm;
    if (tid == 0) {
        if (J.out_len) g_(J.out_len)[s] = R;
        if (J.kf_slot) { g_(J.kf_slot)[0] = J.kf_off; g_(J.kf_slot)[1] = R; }
    }
}

struct ScoreArgs {
    const int32_t* tab;                    // per keyframe {off_p, len_p, off_l, len_l}; len < 0: not stored
    const int32_t* pw;                     // point pool
    const double* pv;
    const int32_t* lw;                     // line pool
    const double* lv;
    int32_t mode;                          // 1 points, 2 lines, 3 both
    int32_t ntarget;                       // stored keyframes looked at: 0 .. ntarget-1
    int32_t cap_p, cap_l;                  // LDS entries reserved for the query's vectors
    const int32_t* queries;                // nq device entries, or nullptr: the one query `query0`
    const plslam_bow_pl_stats* stats;      // nq device entries, or nullptr: `stats0`
    int32_t query0, pad;
    plslam_bow_pl_stats stats0;
    const uint8_t* alive;                  // insert: i < query with alive[i], and i == query; nullptr: every i (NaN if unstored)
    double* out;
    int64_t out_stride;
};

// L1Scoring::score(v1 = the query, v2 = keyframe i), ScoringObject.cpp:23-67; v1's word ids in LDS (s_w1)
__device__ double l1_score(const int32_t* s_w1, int32_t len1, const double* v1, const int32_t* w2, const double* v2,
                           int32_t len2, int lane)
{
    double score = 0;
    for (int b = 0; b < len2; b += 64) {
        const int j = b + lane;
        const bool have = j < len2;
        const int32_t w = have ? g_(w2)[j] : -1;
        int lo = 0, hi = len1;
        while (lo < hi) {                                          // lower_bound
            const int mid = (lo + hi) >> 1;
            if (s_w1[mid] < w) lo = mid + 1; else hi = mid;
        }
        const bool common = have && lo < len1 && s_w1[lo] == w;
        double t = 0.0;
        if (common) {
            const double vi = g_(v1)[lo], wi = g_(v2)[j];
            t = fabs(vi - wi) - fabs(vi) - fabs(wi);
        }
        uint64_t m = __ballot(common);
        while (m) {                                                // ascending lanes = ascending word ids
            const int src = __ffsll((unsigned long long)m) - 1;
            score += __shfl(t, src);
            m &= m - 1;
        }
    }
    score = -score / 2.0;
    return score;
}

__global__ __launch_bounds__(256) void k_bow_score(ScoreArgs a)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
    int32_t* s_p = reinterpret_cast<int32_t*>(smem);
    int32_t* s_l = s_p + a.cap_p;
    const int qi = blockIdx.y;
    const int32_t q = a.queries ? g_(a.queries)[qi] : a.query0;
    const int32_t qoff_p = g_(a.tab)[4 * (size_t)q], qlen_p = max(g_(a.tab)[4 * (size_t)q + 1], 0);
    const int32_t qoff_l = g_(a.tab)[4 * (size_t)q + 2], qlen_l = max(g_(a.tab)[4 * (size_t)q + 3], 0);
    const int np = (a.mode & 1) ? min(qlen_p, a.cap_p) : 0, nl = (a.mode & 2) ? min(qlen_l, a.cap_l) : 0;
    for (int i = threadIdx.x; i < np; i += 256) s_p[i] = g_(a.pw)[qoff_p + i];
    for (int i = threadIdx.x; i < nl; i += 256) s_l[i] = g_(a.lw)[qoff_l + i];
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= a.ntarget) return;
    const int32_t* e = a.tab + 4 * (size_t)i;
    const int32_t off_p = g_(e)[0], len_p = g_(e)[1], off_l = g_(e)[2], len_l = g_(e)[3];
    const bool stored = ((a.mode & 1) == 0 || len_p >= 0) && ((a.mode & 2) == 0 || len_l >= 0);
    double* out = a.out + (int64_t)qi * a.out_stride + i;
    if (a.alive) {
        if (!(i == q || (i < q && g_(a.alive)[i] != 0 && stored))) return;
    } else if (!stored) {
        if (lane == 0) g_(out)[0] = __builtin_nan("");
        return;
    }
    double sp = 0.0, sl = 0.0;
    if (a.mode & 1) sp = l1_score(s_p, np, a.pv + qoff_p, a.pw + off_p, a.pv + off_p, len_p, lane);
    if (a.mode & 2) sl = l1_score(s_l, nl, a.lv + qoff_l, a.lw + off_l, a.lv + off_l, len_l, lane);
    double score;
    if (a.mode == 3) {
        plslam_bow_pl_stats st = a.stats0;
        if (a.stats) st = a.stats[qi];
        const int n_pl = st.n_pt + st.n_ls;
        const double std_pl = st.std_ls + st.std_pt;
        score = 0.0;
        score += (sp * st.n_pt + sl * st.n_ls) / n_pl;             // strategy#1 (mapHandler.cpp:3103, int -> double as in C++)
        score += (sp * st.std_pt + sl * st.std_ls) / std_pl;       // strategy#2
    } else {
        score = (a.mode & 1) ? sp : sl;
    }
    if (lane == 0) g_(out)[0] = score;
}

}  // namespace
}  // namespace plslam

using namespace plslam;

struct plslam_bow_vocab {
    plslam_ctx* ctx = nullptr;
    int32_t k = 0, L = 0, weighting = 0, n = 0, n_words = 0, n_stage = 0;
    DevBuf links, desc, node_w, word_w;
    VocabDev dev() const
    {
        return VocabDev{links.as<int32_t>(), desc.as<uint32_t>(), node_w.as<double>(), word_w.as<double>(), n_stage};
    }
};

struct plslam_bow_db {
    plslam_ctx* ctx = nullptr;
    plslam_bow_vocab* vp = nullptr;
    plslam_bow_vocab* vl = nullptr;
    BowDbState st;                                   // sizes, capacities, reservations: written by bow_db_commit alone
    DevBuf tab, pw, pv, lw, lv;                      // keyframe table; the pools of stored vectors (entries)
    DevBuf scratch;                                  // insert: descriptors, alive, words, the row
    HostBuf pin_in, pin_out;
};

namespace {

int refuse(int code, const BowWhy& why)
{
    set_last_error(why.fmt, why.a, why.b);
    return code;
}

struct FreshBlock {                                  // a new device block until a DevBuf takes it
    void* p = nullptr;
    ~FreshBlock()
    {
        if (p) (void)hipFree(p);
    }
};

// Carries out the planned growth of one set of arrays with ONE capacity (now `have` entries): a pool's word ids and weights
// (`ea` / `eb` bytes per entry), or the keyframe table alone (b == nullptr).  Every new array is allocated first, the g.keep
// entries in use are copied and the rest filled with `fill` bytes (< 0: left as is) on `s`, one synchronisation, then every old
// array is released and replaced: a failure leaves all of them as they were, and the caller's capacity with them.
int grow_pool(int64_t have, const BowGrow& g, DevBuf& a, size_t ea, DevBuf* b, size_t eb, int fill, hipStream_t s)
{
    if (g.cap == have) return PLSLAM_OK;
    DevBuf* const buf[2] = {&a, b};
    const size_t elem[2] = {ea, eb};
    FreshBlock fresh[2];
    for (int i = 0; i < 2 && buf[i]; ++i) PLSLAM_HIP_CHECK(hipMalloc(&fresh[i].p, (size_t)g.cap * elem[i]));
    for (int i = 0; i < 2 && buf[i]; ++i) {
        const size_t kept = (size_t)g.keep * elem[i];
        if (kept) PLSLAM_HIP_CHECK(hipMemcpyAsync(fresh[i].p, buf[i]->p, kept, hipMemcpyDeviceToDevice, s));
        if (fill >= 0) PLSLAM_HIP_CHECK(hipMemsetAsync((char*)fresh[i].p + kept, fill, (size_t)g.cap * elem[i] - kept, s));
    }
    PLSLAM_HIP_CHECK(hipStreamSynchronize(s));      // the old blocks may still be read by enqueued work
    for (int i = 0; i < 2 && buf[i]; ++i) {
        buf[i]->release();
        buf[i]->p = fresh[i].p;
        buf[i]->cap = (size_t)g.cap * elem[i];
        fresh[i].p = nullptr;
    }
    return PLSLAM_OK;
}

// the growth of a plan: the table, then each pool; the capacities are recorded by bow_db_commit once all of it is through
int db_grow(plslam_bow_db* db, const BowInsertPlan& P, hipStream_t s)
{
    int rc;
    if ((rc = grow_pool(db->st.cap_kf, P.tab, db->tab, 16, nullptr, 0, 0xFF, s))) return rc;
    if ((rc = grow_pool(db->st.p.cap, P.p, db->pw, 4, &db->pv, 8, -1, s))) return rc;
    return grow_pool(db->st.l.cap, P.l, db->lw, 4, &db->lv, 8, -1, s);
}

DescendJob descend_job(const plslam_bow_vocab* v, const uint8_t* q, int32_t n, int32_t* word, double* weight)
{
    return DescendJob{v->dev(), reinterpret_cast<const uint32_t*>(q), n, bow_descend_blocks(n), word, weight};
}

int launch_descend(const DescendJob& j0, const DescendJob& j1, size_t lds, hipStream_t s)
{
    const int nb = j0.nblocks + j1.nblocks;
    if (nb == 0) return PLSLAM_OK;
    hipLaunchKernelGGL(k_bow_descend, dim3(nb), dim3(DESCEND_THREADS), lds, s, j0, j1);
    PLSLAM_HIP_CHECK(hipGetLastError());
    return PLSLAM_OK;
}

int launch_sets(const SetJob& j0, const SetJob& j1, size_t lds, hipStream_t s)
{
    const int nb = j0.nsets + j1.nsets;
    if (nb == 0) return PLSLAM_OK;
    hipLaunchKernelGGL(k_bow_sets, dim3(nb), dim3(SET_THREADS), lds, s, j0, j1);
    PLSLAM_HIP_CHECK(hipGetLastError());
    return PLSLAM_OK;
}

int launch_score(const ScoreArgs& a, int32_t nq, size_t lds, hipStream_t s)
{
    if (nq == 0 || a.ntarget == 0) return PLSLAM_OK;
    hipLaunchKernelGGL(k_bow_score, dim3(bow_score_grid_x(a.ntarget), nq), dim3(256), lds, s, a);
    PLSLAM_HIP_CHECK(hipGetLastError());
    return PLSLAM_OK;
}

// what K21 reads of a database whichever call launches it
ScoreArgs score_args(const plslam_bow_db* db)
{
    ScoreArgs a{};
    a.tab = db->tab.as<int32_t>();
    a.pw = db->pw.as<int32_t>();
    a.pv = db->pv.as<double>();
    a.lw = db->lw.as<int32_t>();
    a.lv = db->lv.as<double>();
    a.mode = db->st.mode;
    return a;
}

// the dynamic-LDS limits of K20 / K21 on the CURRENT device (asked for every vocabulary / database: a process-wide once would
// miss a second device)
int raise_lds_limits()
{
    PLSLAM_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_bow_sets), hipFuncAttributeMaxDynamicSharedMemorySize,
                                         (int)SET_LDS_MAX));
    PLSLAM_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_bow_score), hipFuncAttributeMaxDynamicSharedMemorySize,
                                         (int)SCORE_LDS_MAX));
    return PLSLAM_OK;
}

int upload(DevBuf& b, const void* src, size_t bytes)
{
    int rc;
    if ((rc = b.reserve(bytes))) return rc;
    if (hipMemcpy(b.p, src, bytes, hipMemcpyHostToDevice) != hipSuccess) {
        set_last_error("bow vocabulary: upload failed");
        return PLSLAM_EHIP;
    }
    return PLSLAM_OK;
}

}  // namespace

namespace plslam {
// K19 alone over n device rows, for the vocabulary training (bow_train.hip): word[i] = the word of row i
int bow_descend_enqueue(plslam_bow_vocab* v, const uint8_t* q, int32_t n, int32_t* word, hipStream_t s)
{
    if (n <= 0) return PLSLAM_OK;
    return launch_descend(descend_job(v, q, n, word, nullptr), DescendJob{}, bow_stage_bytes(v->n_stage), s);
}
}  // namespace plslam

extern "C" {

int plslam_bow_vocab_create(plslam_ctx* ctx, const plslam_bow_vocab_desc* d, plslam_bow_vocab** out)
{
    PLSLAM_REQUIRE(ctx && d && out, PLSLAM_EINVAL);
    *out = nullptr;
    BowVocabFlat F;
    int rc;
    if ((rc = bow_vocab_flatten(d, &F))) return refuse(rc, F.why);
    std::lock_guard<std::mutex> lk(ctx->mu);
    DeviceGuard g(ctx->device);
    if ((rc = raise_lds_limits())) return rc;
    plslam_bow_vocab* v = new plslam_bow_vocab();
    v->ctx = ctx;
    v->k = d->k;
    v->L = d->L;
    v->weighting = d->weighting_type;
    v->n = F.n;
    v->n_words = F.n_words;
    v->n_stage = F.n_stage;
    if ((rc = upload(v->links, F.links.data(), F.links.size() * 4)) || (rc = upload(v->desc, F.desc.data(), F.desc.size())) ||
        (rc = upload(v->node_w, F.node_w.data(), F.node_w.size() * 8)) ||
        (rc = upload(v->word_w, F.word_w.data(), F.word_w.size() * 8))) {
        plslam_bow_vocab_destroy(v);
        return rc;
    }
    *out = v;
    return PLSLAM_OK;
}

void plslam_bow_vocab_destroy(plslam_bow_vocab* v)
{
    if (!v) return;
    {
        DeviceGuard g(v->ctx->device);
        v->links.release();
        v->desc.release();
        v->node_w.release();
        v->word_w.release();
    }
    delete v;
}

static int transform_enqueue(plslam_bow_vocab* v, const uint8_t* desc, const int32_t* off, const BowTransformCheck& C,
                             int32_t* word, double* weight, int32_t* bow_word, double* bow_w, int32_t* bow_len, hipStream_t s)
{
    DescendJob none{};
    if (C.total > 0) {
        const DescendJob j = descend_job(v, desc, C.total, word, weight);
        int rc = launch_descend(j, none, bow_stage_bytes(v->n_stage), s);
        if (rc) return rc;
    }
    SetJob sj{off, 0, C.nsets, C.max_set, v->weighting, word, v->word_w.as<double>(), bow_word, bow_w, bow_len, nullptr, 0};
    SetJob sn{};
    return launch_sets(sj, sn, bow_set_lds(C.max_set), s);
}

int plslam_bow_transform_dev(plslam_bow_vocab* v, const uint8_t* desc, const int32_t* offsets, int32_t nsets, int32_t total,
                             int32_t max_set, int32_t* word_id, double* word_weight, int32_t* bow_word, double* bow_weight,
                             int32_t* bow_len, void* stream)
{
    PLSLAM_REQUIRE(v, PLSLAM_EINVAL);
    BowTransformCheck C;
    int rc;
    if ((rc = bow_transform_check_dev(desc, offsets, nsets, total, max_set, word_id, bow_word, bow_weight, bow_len, &C)))
        return refuse(rc, C.why);
    if (C.nsets == 0) return PLSLAM_OK;
    DeviceGuard g(v->ctx->device);
    return transform_enqueue(v, desc, offsets, C, word_id, word_weight, bow_word, bow_weight, bow_len,
                             stream ? static_cast<hipStream_t>(stream) : v->ctx->stream);
}

int plslam_bow_transform(plslam_bow_vocab* v, const uint8_t* desc, const int32_t* offsets, int32_t nsets, int32_t* word_id,
                         double* word_weight, int32_t* bow_word, double* bow_weight, int32_t* bow_len)
{
    PLSLAM_REQUIRE(v, PLSLAM_EINVAL);
    BowTransformCheck C;
    int rc;
    if ((rc = bow_transform_check_host(desc, offsets, nsets, bow_len, &C))) return refuse(rc, C.why);
    if (C.nsets == 0) return PLSLAM_OK;
    const BowTransformLayout L = bow_transform_layout(C.nsets, C.total);
    const size_t total = (size_t)C.total;
    plslam_ctx* ctx = v->ctx;
    std::lock_guard<std::mutex> lk(ctx->mu);
    DeviceGuard g(ctx->device);
    if ((rc = ctx->in_a.reserve(L.bytes))) return rc;
    char* d = ctx->in_a.as<char>();
    hipStream_t s = ctx->stream;
    StreamSyncOnError guard(s);
    if (total) PLSLAM_HIP_CHECK(hipMemcpyAsync(d + L.oD, desc, total * 32, hipMemcpyHostToDevice, s));
    PLSLAM_HIP_CHECK(hipMemcpyAsync(d + L.oO, offsets, ((size_t)C.nsets + 1) * 4, hipMemcpyHostToDevice, s));
    if ((rc = transform_enqueue(v, (const uint8_t*)(d + L.oD), (const int32_t*)(d + L.oO), C, (int32_t*)(d + L.oW),
                                (double*)(d + L.oV), (int32_t*)(d + L.oBW), (double*)(d + L.oBV), (int32_t*)(d + L.oL), s)))
        return rc;
    if (total && word_id) PLSLAM_HIP_CHECK(hipMemcpyAsync(word_id, d + L.oW, total * 4, hipMemcpyDeviceToHost, s));
    if (total && word_weight) PLSLAM_HIP_CHECK(hipMemcpyAsync(word_weight, d + L.oV, total * 8, hipMemcpyDeviceToHost, s));
    if (total && bow_word) PLSLAM_HIP_CHECK(hipMemcpyAsync(bow_word, d + L.oBW, total * 4, hipMemcpyDeviceToHost, s));
    if (total && bow_weight) PLSLAM_HIP_CHECK(hipMemcpyAsync(bow_weight, d + L.oBV, total * 8, hipMemcpyDeviceToHost, s));
    PLSLAM_HIP_CHECK(hipMemcpyAsync(bow_len, d + L.oL, (size_t)C.nsets * 4, hipMemcpyDeviceToHost, s));
    PLSLAM_HIP_CHECK(hipStreamSynchronize(s));
    guard.dismiss();
    return PLSLAM_OK;
}

int plslam_bow_db_create(plslam_ctx* ctx, plslam_bow_vocab* vocab_p, plslam_bow_vocab* vocab_l, int32_t capacity_hint,
                         plslam_bow_db** out)
{
    PLSLAM_REQUIRE(ctx && out && capacity_hint >= 0 && (vocab_p || vocab_l), PLSLAM_EINVAL);
    PLSLAM_REQUIRE((!vocab_p || vocab_p->ctx == ctx) && (!vocab_l || vocab_l->ctx == ctx), PLSLAM_EINVAL);
    *out = nullptr;
    std::lock_guard<std::mutex> lk(ctx->mu);
    DeviceGuard g(ctx->device);
    int rc;
    if ((rc = raise_lds_limits())) return rc;
    plslam_bow_db* db = new plslam_bow_db();
    db->ctx = ctx;
    db->vp = vocab_p;
    db->vl = vocab_l;
    db->st.mode = (vocab_p ? 1 : 0) | (vocab_l ? 2 : 0);
    const BowInsertPlan P = bow_db_initial(capacity_hint, db->st.mode);
    if ((rc = db_grow(db, P, ctx->stream))) {
        plslam_bow_db_destroy(db);
        return rc;
    }
    bow_db_commit(db->st, P, nullptr);
    *out = db;
    return PLSLAM_OK;
}

void plslam_bow_db_destroy(plslam_bow_db* db)
{
    if (!db) return;
    {
        DeviceGuard g(db->ctx->device);
        (void)hipStreamSynchronize(db->ctx->stream);
        for (DevBuf* b : {&db->tab, &db->pw, &db->pv, &db->lw, &db->lv, &db->scratch}) b->release();
        db->pin_in.release();
        db->pin_out.release();
    }
    delete db;
}

int plslam_bow_db_size(plslam_bow_db* db, int32_t* n)
{
    PLSLAM_REQUIRE(db && n, PLSLAM_EINVAL);
    *n = db->st.size;
    return PLSLAM_OK;
}

// K19 + K20 + K21 of one planned insert on `s`; pdesc / ldesc / alive / row / words are device pointers
static int db_enqueue_insert(plslam_bow_db* db, const BowInsertPlan& P, const uint8_t* pdesc, const uint8_t* ldesc,
                             const plslam_bow_pl_stats* stats, const uint8_t* alive, double* row, int32_t* words, hipStream_t s)
{
    DescendJob jp{}, jl{};
    SetJob sp{}, sl{};
    int32_t* tab = db->tab.as<int32_t>() + 4 * (size_t)P.kf_idx;
    if (db->st.mode & 1) {
        jp = descend_job(db->vp, pdesc, P.n_p, words, nullptr);
        sp = SetJob{nullptr, P.n_p, 1, P.n_p, db->vp->weighting, words, db->vp->word_w.as<double>(),
                    db->pw.as<int32_t>() + P.off_p, db->pv.as<double>() + P.off_p, nullptr, tab, (int32_t)P.off_p};
    }
    if (db->st.mode & 2) {
        jl = descend_job(db->vl, ldesc, P.n_l, words + P.n_p, nullptr);
        sl = SetJob{nullptr, P.n_l, 1, P.n_l, db->vl->weighting, words + P.n_p, db->vl->word_w.as<double>(),
                    db->lw.as<int32_t>() + P.off_l, db->lv.as<double>() + P.off_l, nullptr, tab + 2, (int32_t)P.off_l};
    }
    int rc;
    const size_t lds = std::max(db->vp ? bow_stage_bytes(db->vp->n_stage) : 0, db->vl ? bow_stage_bytes(db->vl->n_stage) : 0);
    if ((rc = launch_descend(jp.n ? jp : DescendJob{}, jl.n ? jl : DescendJob{}, lds, s))) return rc;
    if ((rc = launch_sets(sp, sl, P.sets_lds, s))) return rc;
    ScoreArgs a = score_args(db);
    a.ntarget = P.kf_idx + 1;
    a.cap_p = P.n_p;
    a.cap_l = P.n_l;
    a.query0 = P.kf_idx;
    a.stats0 = stats ? *stats : plslam_bow_pl_stats{0, 0, 0.0, 0.0};
    a.alive = alive;
    a.out = row;
    a.out_stride = 0;
    return launch_score(a, 1, P.score_lds, s);
}

int plslam_bow_db_insert(plslam_bow_db* db, int32_t kf_idx, const uint8_t* pdesc, int32_t n_pdesc, const uint8_t* ldesc,
                         int32_t n_ldesc, const plslam_bow_pl_stats* stats, const uint8_t* alive, double* conf_row)
{
    PLSLAM_REQUIRE(db, PLSLAM_EINVAL);
    BowInsertPlan P;
    int rc;
    if ((rc = bow_insert_check(db->st, kf_idx, pdesc, n_pdesc, ldesc, n_ldesc, stats, alive, conf_row, true, &P)))
        return refuse(rc, P.why);
    plslam_ctx* ctx = db->ctx;
    std::lock_guard<std::mutex> lk(ctx->mu);
    DeviceGuard g(ctx->device);
    hipStream_t s = ctx->stream;
    StreamSyncOnError guard(s);
    if ((rc = bow_db_plan_insert(db->st, kf_idx, n_pdesc, n_ldesc, true, &P))) return refuse(rc, P.why);
    if ((rc = db_grow(db, P, s)) || (rc = db->scratch.reserve(P.scratch_bytes)) || (rc = db->pin_in.reserve(P.pin_in_bytes)) ||
        (rc = db->pin_out.reserve(P.pin_out_bytes)))
        return rc;
    char* h = db->pin_in.as<char>();
    if (P.n_p) std::memcpy(h + P.oP, pdesc, (size_t)P.n_p * 32);
    if (P.n_l) std::memcpy(h + P.oL, ldesc, (size_t)P.n_l * 32);
    if (kf_idx) std::memcpy(h + P.oA, alive, (size_t)kf_idx);
    char* d = db->scratch.as<char>();
    PLSLAM_HIP_CHECK(hipMemcpyAsync(d, h, P.up, hipMemcpyHostToDevice, s));
    if ((rc = db_enqueue_insert(db, P, (const uint8_t*)(d + P.oP), (const uint8_t*)(d + P.oL), stats, (const uint8_t*)(d + P.oA),
                                (double*)(d + P.oR), (int32_t*)(d + P.oW), s)))
        return rc;
    PLSLAM_HIP_CHECK(hipMemcpyAsync(db->pin_out.p, d + P.oR, P.pin_out_bytes, hipMemcpyDeviceToHost, s));
    PLSLAM_HIP_CHECK(hipStreamSynchronize(s));
    guard.dismiss();
    bow_db_commit(db->st, P, stats);
    const double* r = db->pin_out.as<double>();
    for (int32_t i = 0; i < kf_idx; ++i)
        if (alive[i]) conf_row[i] = r[i];
    conf_row[kf_idx] = r[kf_idx];
    return PLSLAM_OK;
}

int plslam_bow_db_insert_dev(plslam_bow_db* db, int32_t kf_idx, const uint8_t* pdesc, int32_t n_pdesc, const uint8_t* ldesc,
                             int32_t n_ldesc, const plslam_bow_pl_stats* stats, const uint8_t* alive, double* conf_row)
{
    PLSLAM_REQUIRE(db, PLSLAM_EINVAL);
    BowInsertPlan P;
    int rc;
    if ((rc = bow_insert_check(db->st, kf_idx, pdesc, n_pdesc, ldesc, n_ldesc, stats, alive, conf_row, false, &P)) ||
        (rc = bow_db_plan_insert(db->st, kf_idx, n_pdesc, n_ldesc, false, &P)))
        return refuse(rc, P.why);
    DeviceGuard g(db->ctx->device);
    hipStream_t s = db->ctx->stream;
    if ((rc = db_grow(db, P, s)) || (rc = db->scratch.reserve(P.scratch_bytes))) return rc;
    if ((rc = db_enqueue_insert(db, P, pdesc, ldesc, stats, alive, conf_row, db->scratch.as<int32_t>(), s))) return rc;
    bow_db_commit(db->st, P, stats);
    return PLSLAM_OK;
}

int plslam_bow_db_score(plslam_bow_db* db, const int32_t* queries, int32_t nq, double* out)
{
    PLSLAM_REQUIRE(db, PLSLAM_EINVAL);
    BowScorePlan P;
    int rc;
    if ((rc = bow_score_plan(db->st, queries, nq, out, &P))) return refuse(rc, P.why);
    if (P.nq == 0 || P.n == 0) return PLSLAM_OK;
    plslam_ctx* ctx = db->ctx;
    std::lock_guard<std::mutex> lk(ctx->mu);
    DeviceGuard g(ctx->device);
    hipStream_t s = ctx->stream;
    StreamSyncOnError guard(s);
    if ((rc = db->scratch.reserve(P.bytes))) return rc;
    char* d = db->scratch.as<char>();
    PLSLAM_HIP_CHECK(hipMemcpyAsync(d + P.oQ, queries, (size_t)P.nq * 4, hipMemcpyHostToDevice, s));
    PLSLAM_HIP_CHECK(hipMemcpyAsync(d + P.oS, P.st.data(), (size_t)P.nq * sizeof(plslam_bow_pl_stats), hipMemcpyHostToDevice, s));
    ScoreArgs a = score_args(db);
    a.ntarget = P.n;
    a.cap_p = P.cap_p;
    a.cap_l = P.cap_l;
    a.queries = (const int32_t*)(d + P.oQ);
    a.stats = (const plslam_bow_pl_stats*)(d + P.oS);
    a.alive = nullptr;
    a.out = (double*)(d + P.oO);
    a.out_stride = P.n;
    if ((rc = launch_score(a, P.nq, P.score_lds, s))) return rc;
    PLSLAM_HIP_CHECK(hipMemcpyAsync(out, d + P.oO, (size_t)P.nq * P.n * 8, hipMemcpyDeviceToHost, s));
    PLSLAM_HIP_CHECK(hipStreamSynchronize(s));
    guard.dismiss();
    return PLSLAM_OK;
}

}  // extern "C"
