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
#include "common.hpp"

#include <algorithm>
#include <cstring>

namespace plslam {
namespace {

constexpr int STAGE_NODES = 1228;          // 1228 x (32 + 8) B = 48 KB of LDS: no dynamic-LDS attribute needed for K19
constexpr int DESCEND_THREADS = 256;
constexpr int SET_THREADS = 1024;
constexpr uint32_t NO_WORD = 0xFFFFFFFFu;  // sorts behind every word id (< 2^31)
constexpr size_t SET_LDS_MAX = (size_t)PLSLAM_BOW_MAX_SET * 4 + SET_THREADS * 4 + 16;
constexpr size_t SCORE_LDS_MAX = (size_t)2 * PLSLAM_BOW_MAX_SET * 4;

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
    size_t stage_bytes() const { return (size_t)n_stage * 40; }
};

struct plslam_bow_db {
    plslam_ctx* ctx = nullptr;
    plslam_bow_vocab* vp = nullptr;
    plslam_bow_vocab* vl = nullptr;
    int mode = 0;                                    // 1 P, 2 L, 3 PL
    int32_t cap_kf = 0, size = 0;
    int64_t cap_p = 0, used_p = 0, cap_l = 0, used_l = 0;
    DevBuf tab, pw, pv, lw, lv;                      // keyframe table; the pools of stored vectors (entries)
    DevBuf scratch;                                  // insert: descriptors, alive, words, the row
    HostBuf pin_in, pin_out;
    std::vector<int32_t> res_p, res_l;               // entries reserved per keyframe
    std::vector<uint8_t> inserted;
    std::vector<plslam_bow_pl_stats> stats;
};

namespace {

int fail(int code, const char* msg, long a = 0, long b = 0)
{
    set_last_error(msg, a, b);
    return code;
}

// grows a device array of `elem`-byte entries from `have` to at least `need` entries, keeping the first `keep` entries
// (copied on `s`); new space filled with `fill` bytes
int grow(DevBuf& b, size_t elem, int64_t& have, int64_t need, int64_t keep, int fill, hipStream_t s)
{
    if (need <= have) return PLSLAM_OK;
    const int64_t want = std::max(need, have * 2);
    void* p = nullptr;
    PLSLAM_HIP_CHECK(hipMalloc(&p, (size_t)want * elem));
    if (keep > 0) PLSLAM_HIP_CHECK(hipMemcpyAsync(p, b.p, (size_t)keep * elem, hipMemcpyDeviceToDevice, s));
    if (fill >= 0) PLSLAM_HIP_CHECK(hipMemsetAsync((char*)p + keep * elem, fill, (size_t)(want - keep) * elem, s));
    PLSLAM_HIP_CHECK(hipStreamSynchronize(s));      // the old block may still be read by enqueued work
    b.release();
    b.p = p;
    b.cap = (size_t)want * elem;
    have = want;
    return PLSLAM_OK;
}

DescendJob descend_job(const plslam_bow_vocab* v, const uint8_t* q, int32_t n, int32_t* word, double* weight)
{
    return DescendJob{v->dev(), reinterpret_cast<const uint32_t*>(q), n, (n + DESCEND_THREADS - 1) / DESCEND_THREADS, word,
                      weight};
}

int launch_descend(const DescendJob& j0, const DescendJob& j1, size_t lds, hipStream_t s)
{
    const int nb = j0.nblocks + j1.nblocks;
    if (nb == 0) return PLSLAM_OK;
    hipLaunchKernelGGL(k_bow_descend, dim3(nb), dim3(DESCEND_THREADS), lds, s, j0, j1);
    PLSLAM_HIP_CHECK(hipGetLastError());
    return PLSLAM_OK;
}

size_t set_lds(int32_t max_set)
{
    int P = 1;
    while (P < max_set) P <<= 1;
    return (size_t)P * 4 + SET_THREADS * 4;
}

int launch_sets(const SetJob& j0, const SetJob& j1, size_t lds, hipStream_t s)
{
    const int nb = j0.nsets + j1.nsets;
    if (nb == 0) return PLSLAM_OK;
    hipLaunchKernelGGL(k_bow_sets, dim3(nb), dim3(SET_THREADS), lds, s, j0, j1);
    PLSLAM_HIP_CHECK(hipGetLastError());
    return PLSLAM_OK;
}

int launch_score(const ScoreArgs& a, int32_t nq, hipStream_t s)
{
    if (nq == 0 || a.ntarget == 0) return PLSLAM_OK;
    const size_t lds = std::max<size_t>(16, (size_t)(a.cap_p + a.cap_l) * 4);
    hipLaunchKernelGGL(k_bow_score, dim3((a.ntarget + 3) / 4, nq), dim3(256), lds, s, a);
    PLSLAM_HIP_CHECK(hipGetLastError());
    return PLSLAM_OK;
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

}  // namespace

extern "C" {

int plslam_bow_vocab_create(plslam_ctx* ctx, const plslam_bow_vocab_desc* d, plslam_bow_vocab** out)
{
    PLSLAM_REQUIRE(ctx && d && out, PLSLAM_EINVAL);
    *out = nullptr;
    const int32_t N = d->n_nodes, W = d->n_words;
    if (N <= 0 || W <= 0) return fail(PLSLAM_EINVAL, "bow vocabulary: empty (%ld nodes, %ld words)", N, W);
    PLSLAM_REQUIRE(d->nodes && d->words, PLSLAM_EINVAL);
    if (d->scoring_type != PLSLAM_BOW_L1_NORM)
        return fail(PLSLAM_ENOTSUP, "bow vocabulary: scoring type %ld is not supported (only L1_NORM = 0)", d->scoring_type);
    if (d->weighting_type < PLSLAM_BOW_TF_IDF || d->weighting_type > PLSLAM_BOW_BINARY)
        return fail(PLSLAM_EINVAL, "bow vocabulary: weighting type %ld out of range", d->weighting_type);
    // children lists in file order (TemplatedVocabulary.h:1470 m_nodes[pid].children.push_back(nid)), as CSR
    std::vector<int32_t> rec_of((size_t)N + 1, -1), nchild((size_t)N + 2, 0);
    for (int32_t r = 0; r < N; ++r) {
        const int32_t id = d->nodes[r].node_id, pid = d->nodes[r].parent_id;
        if (id < 1 || id > N) return fail(PLSLAM_EINVAL, "bow vocabulary: node id %ld out of range 1..%ld", id, N);
        if (rec_of[id] >= 0) return fail(PLSLAM_EINVAL, "bow vocabulary: duplicate node id %ld", id);
        if (pid < 0 || pid > N) return fail(PLSLAM_EINVAL, "bow vocabulary: parent %ld of node %ld is not a node", pid, id);
        if (pid == id) return fail(PLSLAM_EINVAL, "bow vocabulary: node %ld is its own parent (cycle)", id);
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
        if (wid < 0 || wid >= W) return fail(PLSLAM_EINVAL, "bow vocabulary: word id %ld out of range 0..%ld", wid, W - 1);
        if (nid < 1 || nid > N) return fail(PLSLAM_EINVAL, "bow vocabulary: word %ld names node %ld, not a node", wid, nid);
        if (node_of_word[wid] >= 0) return fail(PLSLAM_EINVAL, "bow vocabulary: duplicate word id %ld", wid);
        if (word_of[nid] >= 0) return fail(PLSLAM_EINVAL, "bow vocabulary: node %ld carries two words", nid);
        node_of_word[wid] = nid;
        word_of[nid] = wid;
    }
    // breadth-first order from the root: every parent's children contiguous, in list order
    std::vector<int32_t> order;
    order.reserve((size_t)N + 1);
    order.push_back(0);
    for (size_t h = 0; h < order.size(); ++h) {
        const int32_t u = order[h];
        for (int32_t c = first[u]; c < first[u + 1]; ++c) order.push_back(kids[c]);
        if (order.size() > (size_t)N + 1) break;
    }
    if (order.size() != (size_t)N + 1)
        return fail(PLSLAM_EINVAL, "bow vocabulary: %ld of %ld nodes are not reachable from the root (a cycle)",
                    (long)N + 1 - (long)order.size(), N);
    std::vector<int32_t> pos((size_t)N + 1);
    for (int32_t i = 0; i <= N; ++i) pos[order[i]] = i;
    std::vector<int32_t> links((size_t)2 * (N + 1));
    std::vector<uint8_t> desc((size_t)32 * (N + 1), 0);
    std::vector<double> node_w((size_t)N + 1, 0.0), word_w((size_t)W, 0.0);
    for (int32_t i = 0; i <= N; ++i) {
        const int32_t u = order[i], nc = first[u + 1] - first[u];
        if (nc == 0 && word_of[u] < 0) return fail(PLSLAM_EINVAL, "bow vocabulary: leaf node %ld has no word", u);
        links[2 * (size_t)i] = nc ? pos[kids[first[u]]] : word_of[u];
        links[2 * (size_t)i + 1] = nc;
        if (u > 0) {
            std::memcpy(&desc[32 * (size_t)i], d->nodes[rec_of[u]].descriptor, 32);
            node_w[i] = d->nodes[rec_of[u]].weight;
        }
    }
    for (int32_t w = 0; w < W; ++w) word_w[w] = d->nodes[rec_of[node_of_word[w]]].weight;

    std::lock_guard<std::mutex> lk(ctx->mu);
    DeviceGuard g(ctx->device);
    int rc;
    if ((rc = raise_lds_limits())) return rc;
    plslam_bow_vocab* v = new plslam_bow_vocab();
    v->ctx = ctx;
    v->k = d->k;
    v->L = d->L;
    v->weighting = d->weighting_type;
    v->n = N + 1;
    v->n_words = W;
    v->n_stage = std::min(N + 1, STAGE_NODES);
    if ((rc = v->links.reserve(links.size() * 4)) || (rc = v->desc.reserve(desc.size())) ||
        (rc = v->node_w.reserve(node_w.size() * 8)) || (rc = v->word_w.reserve(word_w.size() * 8))) {
        plslam_bow_vocab_destroy(v);
        return rc;
    }
    if (hipMemcpy(v->links.p, links.data(), links.size() * 4, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(v->desc.p, desc.data(), desc.size(), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(v->node_w.p, node_w.data(), node_w.size() * 8, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(v->word_w.p, word_w.data(), word_w.size() * 8, hipMemcpyHostToDevice) != hipSuccess) {
        set_last_error("bow vocabulary: upload failed");
        plslam_bow_vocab_destroy(v);
        return PLSLAM_EHIP;
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

static int transform_enqueue(plslam_bow_vocab* v, const uint8_t* desc, const int32_t* off, int32_t nsets, int32_t total,
                             int32_t max_set, int32_t* word, double* weight, int32_t* bow_word, double* bow_w, int32_t* bow_len,
                             hipStream_t s)
{
    DescendJob none{};
    if (total > 0) {
        const DescendJob j = descend_job(v, desc, total, word, weight);
        int rc = launch_descend(j, none, v->stage_bytes(), s);
        if (rc) return rc;
    }
    SetJob sj{off, 0, nsets, max_set, v->weighting, word, v->word_w.as<double>(), bow_word, bow_w, bow_len, nullptr, 0};
    SetJob sn{};
    return launch_sets(sj, sn, set_lds(max_set), s);
}

int plslam_bow_transform_dev(plslam_bow_vocab* v, const uint8_t* desc, const int32_t* offsets, int32_t nsets, int32_t total,
                             int32_t max_set, int32_t* word_id, double* word_weight, int32_t* bow_word, double* bow_weight,
                             int32_t* bow_len, void* stream)
{
    PLSLAM_REQUIRE(v && nsets >= 0 && total >= 0 && max_set >= 0, PLSLAM_EINVAL);
    if (max_set > PLSLAM_BOW_MAX_SET) return fail(PLSLAM_ERANGE, "bow transform: max_set %ld > PLSLAM_BOW_MAX_SET (%ld)", max_set,
                                                  PLSLAM_BOW_MAX_SET);
    if (nsets == 0) return PLSLAM_OK;
    PLSLAM_REQUIRE(offsets && word_id && bow_word && bow_weight && bow_len && (total == 0 || desc), PLSLAM_EINVAL);
    PLSLAM_REQUIRE(((uintptr_t)desc & 15) == 0, PLSLAM_EINVAL);
    DeviceGuard g(v->ctx->device);
    return transform_enqueue(v, desc, offsets, nsets, total, max_set, word_id, word_weight, bow_word, bow_weight, bow_len,
                             stream ? static_cast<hipStream_t>(stream) : v->ctx->stream);
}

int plslam_bow_transform(plslam_bow_vocab* v, const uint8_t* desc, const int32_t* offsets, int32_t nsets, int32_t* word_id,
                         double* word_weight, int32_t* bow_word, double* bow_weight, int32_t* bow_len)
{
    PLSLAM_REQUIRE(v && nsets >= 0, PLSLAM_EINVAL);
    if (nsets == 0) return PLSLAM_OK;
    PLSLAM_REQUIRE(offsets && bow_len && offsets[0] == 0, PLSLAM_EINVAL);
    int32_t max_set = 0;
    for (int32_t s = 0; s < nsets; ++s) {
        const int64_t n = (int64_t)offsets[s + 1] - offsets[s];
        PLSLAM_REQUIRE(n >= 0, PLSLAM_EINVAL);
        if (n > PLSLAM_BOW_MAX_SET)
            return fail(PLSLAM_ERANGE, "bow transform: set of %ld descriptors > PLSLAM_BOW_MAX_SET (%ld)", (long)n,
                        PLSLAM_BOW_MAX_SET);
        max_set = std::max<int32_t>(max_set, (int32_t)n);
    }
    const int32_t total = offsets[nsets];
    PLSLAM_REQUIRE(total == 0 || desc, PLSLAM_EINVAL);
    plslam_ctx* ctx = v->ctx;
    std::lock_guard<std::mutex> lk(ctx->mu);
    DeviceGuard g(ctx->device);
    Carver c;
    const size_t oD = c.take((size_t)total * 32), oO = c.take((size_t)(nsets + 1) * 4), oW = c.take((size_t)total * 4),
                 oV = c.take((size_t)total * 8), oBW = c.take((size_t)total * 4), oBV = c.take((size_t)total * 8),
                 oL = c.take((size_t)nsets * 4);
    int rc;
    if ((rc = ctx->in_a.reserve(c.off))) return rc;
    char* d = ctx->in_a.as<char>();
    hipStream_t s = ctx->stream;
    StreamSyncOnError guard(s);
    if (total) PLSLAM_HIP_CHECK(hipMemcpyAsync(d + oD, desc, (size_t)total * 32, hipMemcpyHostToDevice, s));
    PLSLAM_HIP_CHECK(hipMemcpyAsync(d + oO, offsets, (size_t)(nsets + 1) * 4, hipMemcpyHostToDevice, s));
    if ((rc = transform_enqueue(v, (const uint8_t*)(d + oD), (const int32_t*)(d + oO), nsets, total, max_set, (int32_t*)(d + oW),
                                (double*)(d + oV), (int32_t*)(d + oBW), (double*)(d + oBV), (int32_t*)(d + oL), s)))
        return rc;
    if (total && word_id) PLSLAM_HIP_CHECK(hipMemcpyAsync(word_id, d + oW, (size_t)total * 4, hipMemcpyDeviceToHost, s));
    if (total && word_weight) PLSLAM_HIP_CHECK(hipMemcpyAsync(word_weight, d + oV, (size_t)total * 8, hipMemcpyDeviceToHost, s));
    if (total && bow_word) PLSLAM_HIP_CHECK(hipMemcpyAsync(bow_word, d + oBW, (size_t)total * 4, hipMemcpyDeviceToHost, s));
    if (total && bow_weight) PLSLAM_HIP_CHECK(hipMemcpyAsync(bow_weight, d + oBV, (size_t)total * 8, hipMemcpyDeviceToHost, s));
    PLSLAM_HIP_CHECK(hipMemcpyAsync(bow_len, d + oL, (size_t)nsets * 4, hipMemcpyDeviceToHost, s));
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
    db->mode = (vocab_p ? 1 : 0) | (vocab_l ? 2 : 0);
    const int64_t cap = std::max<int32_t>(capacity_hint, 16);
    int64_t c0 = 0;
    rc = grow(db->tab, 16, c0, cap, 0, 0xFF, ctx->stream);
    db->cap_kf = (int32_t)c0;
    if (!rc && vocab_p) rc = grow(db->pw, 4, db->cap_p, cap * 256, 0, -1, ctx->stream);
    if (!rc && vocab_p) { int64_t c = 0; rc = grow(db->pv, 8, c, db->cap_p, 0, -1, ctx->stream); }
    if (!rc && vocab_l) rc = grow(db->lw, 4, db->cap_l, cap * 64, 0, -1, ctx->stream);
    if (!rc && vocab_l) { int64_t c = 0; rc = grow(db->lv, 8, c, db->cap_l, 0, -1, ctx->stream); }
    if (rc) {
        plslam_bow_db_destroy(db);
        return rc;
    }
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
    *n = db->size;
    return PLSLAM_OK;
}

// host-side bookkeeping and growth in front of an insert; the caller holds the context lock (host path) or owns the db (dev)
static int db_prepare(plslam_bow_db* db, int32_t kf_idx, int32_t n_p, int32_t n_l, int64_t& off_p, int64_t& off_l)
{
    hipStream_t s = db->ctx->stream;
    int rc;
    int64_t cap_kf = db->cap_kf;
    if ((rc = grow(db->tab, 16, cap_kf, (int64_t)kf_idx + 1, db->size, 0xFF, s))) return rc;
    db->cap_kf = (int32_t)cap_kf;
    off_p = db->used_p;
    off_l = db->used_l;
    if (db->mode & 1) {
        int64_t c = db->cap_p;
        if ((rc = grow(db->pw, 4, db->cap_p, db->used_p + n_p, db->used_p, -1, s))) return rc;
        if ((rc = grow(db->pv, 8, c, db->cap_p, db->used_p, -1, s))) return rc;
    }
    if (db->mode & 2) {
        int64_t c = db->cap_l;
        if ((rc = grow(db->lw, 4, db->cap_l, db->used_l + n_l, db->used_l, -1, s))) return rc;
        if ((rc = grow(db->lv, 8, c, db->cap_l, db->used_l, -1, s))) return rc;
    }
    if ((int32_t)db->res_p.size() <= kf_idx) {
        db->res_p.resize((size_t)kf_idx + 1, 0);
        db->res_l.resize((size_t)kf_idx + 1, 0);
        db->inserted.resize((size_t)kf_idx + 1, 0);
        db->stats.resize((size_t)kf_idx + 1, plslam_bow_pl_stats{0, 0, 0.0, 0.0});
    }
    if ((off_p + n_p) > INT32_MAX || (off_l + n_l) > INT32_MAX)
        return fail(PLSLAM_ERANGE, "bow database: more than 2^31 stored entries");
    return PLSLAM_OK;
}

static void db_commit(plslam_bow_db* db, int32_t kf_idx, int32_t n_p, int32_t n_l, const plslam_bow_pl_stats* stats)
{
    if (db->mode & 1) { db->res_p[kf_idx] = n_p; db->used_p += n_p; }
    if (db->mode & 2) { db->res_l[kf_idx] = n_l; db->used_l += n_l; }
    db->inserted[kf_idx] = 1;
    db->stats[kf_idx] = stats ? *stats : plslam_bow_pl_stats{0, 0, 0.0, 0.0};
    db->size = std::max(db->size, kf_idx + 1);
}

// K19 + K20 + K21 of one insert on `s`; pdesc / ldesc / alive / row are device pointers
static int db_enqueue_insert(plslam_bow_db* db, int32_t kf_idx, const uint8_t* pdesc, int32_t n_p, const uint8_t* ldesc,
                             int32_t n_l, const plslam_bow_pl_stats* stats, const uint8_t* alive, double* row, int32_t* words,
                             int64_t off_p, int64_t off_l, hipStream_t s)
{
    DescendJob jp{}, jl{};
    SetJob sp{}, sl{};
    int32_t* tab = db->tab.as<int32_t>() + 4 * (size_t)kf_idx;
    if (db->mode & 1) {
        jp = descend_job(db->vp, pdesc, n_p, words, nullptr);
        sp = SetJob{nullptr, n_p, 1, n_p, db->vp->weighting, words, db->vp->word_w.as<double>(), db->pw.as<int32_t>() + off_p,
                    db->pv.as<double>() + off_p, nullptr, tab, (int32_t)off_p};
    }
    if (db->mode & 2) {
        jl = descend_job(db->vl, ldesc, n_l, words + n_p, nullptr);
        sl = SetJob{nullptr, n_l, 1, n_l, db->vl->weighting, words + n_p, db->vl->word_w.as<double>(),
                    db->lw.as<int32_t>() + off_l, db->lv.as<double>() + off_l, nullptr, tab + 2, (int32_t)off_l};
    }
    int rc;
    size_t lds = std::max(db->vp ? db->vp->stage_bytes() : 0, db->vl ? db->vl->stage_bytes() : 0);
    if ((rc = launch_descend(jp.n ? jp : DescendJob{}, jl.n ? jl : DescendJob{}, lds, s))) return rc;
    if ((rc = launch_sets(sp, sl, set_lds(std::max(n_p, n_l)), s))) return rc;
    ScoreArgs a{};
    a.tab = db->tab.as<int32_t>();
    a.pw = db->pw.as<int32_t>();
    a.pv = db->pv.as<double>();
    a.lw = db->lw.as<int32_t>();
    a.lv = db->lv.as<double>();
    a.mode = db->mode;
    a.ntarget = kf_idx + 1;
    a.cap_p = (db->mode & 1) ? n_p : 0;
    a.cap_l = (db->mode & 2) ? n_l : 0;
    a.query0 = kf_idx;
    a.stats0 = stats ? *stats : plslam_bow_pl_stats{0, 0, 0.0, 0.0};
    a.alive = alive;
    a.out = row;
    a.out_stride = 0;
    return launch_score(a, 1, s);
}

static int check_insert(plslam_bow_db* db, int32_t kf_idx, const uint8_t* pdesc, int32_t& n_p, const uint8_t* ldesc,
                        int32_t& n_l, const plslam_bow_pl_stats* stats, const uint8_t* alive, const double* row)
{
    PLSLAM_REQUIRE(db && kf_idx >= 0 && kf_idx < INT32_MAX && row && (kf_idx == 0 || alive), PLSLAM_EINVAL);
    if (!(db->mode & 1)) n_p = 0;
    if (!(db->mode & 2)) n_l = 0;
    PLSLAM_REQUIRE(n_p >= 0 && n_l >= 0 && (n_p == 0 || pdesc) && (n_l == 0 || ldesc), PLSLAM_EINVAL);
    PLSLAM_REQUIRE(db->mode != 3 || stats, PLSLAM_EINVAL);
    if (n_p > PLSLAM_BOW_MAX_SET || n_l > PLSLAM_BOW_MAX_SET)
        return fail(PLSLAM_ERANGE, "bow insert: %ld point / %ld line descriptors; at most PLSLAM_BOW_MAX_SET each", n_p, n_l);
    return PLSLAM_OK;
}

int plslam_bow_db_insert(plslam_bow_db* db, int32_t kf_idx, const uint8_t* pdesc, int32_t n_pdesc, const uint8_t* ldesc,
                         int32_t n_ldesc, const plslam_bow_pl_stats* stats, const uint8_t* alive, double* conf_row)
{
    int rc;
    if ((rc = check_insert(db, kf_idx, pdesc, n_pdesc, ldesc, n_ldesc, stats, alive, conf_row))) return rc;
    for (int32_t i = 0; i < kf_idx; ++i)
        if (alive[i] && (i >= (int32_t)db->inserted.size() || !db->inserted[i]))
            return fail(PLSLAM_EINVAL, "bow insert: keyframe %ld is alive but was never inserted", i);
    plslam_ctx* ctx = db->ctx;
    std::lock_guard<std::mutex> lk(ctx->mu);
    DeviceGuard g(ctx->device);
    hipStream_t s = ctx->stream;
    StreamSyncOnError guard(s);
    int64_t off_p, off_l;
    if ((rc = db_prepare(db, kf_idx, n_pdesc, n_ldesc, off_p, off_l))) return rc;
    Carver c;
    const size_t oP = c.take((size_t)n_pdesc * 32), oL = c.take((size_t)n_ldesc * 32), oA = c.take((size_t)kf_idx + 1);
    const size_t up = c.off;
    const size_t oW = c.take((size_t)(n_pdesc + n_ldesc) * 4), oR = c.take((size_t)(kf_idx + 1) * 8);
    if ((rc = db->scratch.reserve(c.off)) || (rc = db->pin_in.reserve(up)) || (rc = db->pin_out.reserve((size_t)(kf_idx + 1) * 8)))
        return rc;
    char* h = db->pin_in.as<char>();
    if (n_pdesc) std::memcpy(h + oP, pdesc, (size_t)n_pdesc * 32);
    if (n_ldesc) std::memcpy(h + oL, ldesc, (size_t)n_ldesc * 32);
    if (kf_idx) std::memcpy(h + oA, alive, (size_t)kf_idx);
    char* d = db->scratch.as<char>();
    PLSLAM_HIP_CHECK(hipMemcpyAsync(d, h, up, hipMemcpyHostToDevice, s));
    if ((rc = db_enqueue_insert(db, kf_idx, (const uint8_t*)(d + oP), n_pdesc, (const uint8_t*)(d + oL), n_ldesc, stats,
                                (const uint8_t*)(d + oA), (double*)(d + oR), (int32_t*)(d + oW), off_p, off_l, s)))
        return rc;
    PLSLAM_HIP_CHECK(hipMemcpyAsync(db->pin_out.p, d + oR, (size_t)(kf_idx + 1) * 8, hipMemcpyDeviceToHost, s));
    PLSLAM_HIP_CHECK(hipStreamSynchronize(s));
    guard.dismiss();
    db_commit(db, kf_idx, n_pdesc, n_ldesc, stats);
    const double* r = db->pin_out.as<double>();
    for (int32_t i = 0; i < kf_idx; ++i)
        if (alive[i]) conf_row[i] = r[i];
    conf_row[kf_idx] = r[kf_idx];
    return PLSLAM_OK;
}

int plslam_bow_db_insert_dev(plslam_bow_db* db, int32_t kf_idx, const uint8_t* pdesc, int32_t n_pdesc, const uint8_t* ldesc,
                             int32_t n_ldesc, const plslam_bow_pl_stats* stats, const uint8_t* alive, double* conf_row)
{
    int rc;
    if ((rc = check_insert(db, kf_idx, pdesc, n_pdesc, ldesc, n_ldesc, stats, alive, conf_row))) return rc;
    PLSLAM_REQUIRE(((uintptr_t)pdesc & 15) == 0 && ((uintptr_t)ldesc & 15) == 0 && ((uintptr_t)conf_row & 7) == 0, PLSLAM_EINVAL);
    DeviceGuard g(db->ctx->device);
    hipStream_t s = db->ctx->stream;
    int64_t off_p, off_l;
    if ((rc = db_prepare(db, kf_idx, n_pdesc, n_ldesc, off_p, off_l))) return rc;
    if ((rc = db->scratch.reserve((size_t)(n_pdesc + n_ldesc) * 4 + 16))) return rc;
    if ((rc = db_enqueue_insert(db, kf_idx, pdesc, n_pdesc, ldesc, n_ldesc, stats, alive, conf_row, db->scratch.as<int32_t>(),
                                off_p, off_l, s)))
        return rc;
    db_commit(db, kf_idx, n_pdesc, n_ldesc, stats);
    return PLSLAM_OK;
}

int plslam_bow_db_score(plslam_bow_db* db, const int32_t* queries, int32_t nq, double* out)
{
    PLSLAM_REQUIRE(db && nq >= 0, PLSLAM_EINVAL);
    if (nq == 0 || db->size == 0) return PLSLAM_OK;
    PLSLAM_REQUIRE(queries && out, PLSLAM_EINVAL);
    int32_t cap_p = 0, cap_l = 0;
    std::vector<plslam_bow_pl_stats> st((size_t)nq);
    for (int32_t q = 0; q < nq; ++q) {
        const int32_t k = queries[q];
        if (k < 0 || k >= db->size || !db->inserted[k])
            return fail(PLSLAM_EINVAL, "bow score: query %ld (keyframe %ld) was never inserted", q, k);
        cap_p = std::max(cap_p, (db->mode & 1) ? db->res_p[k] : 0);
        cap_l = std::max(cap_l, (db->mode & 2) ? db->res_l[k] : 0);
        st[q] = db->stats[k];
    }
    const int32_t n = db->size;
    plslam_ctx* ctx = db->ctx;
    std::lock_guard<std::mutex> lk(ctx->mu);
    DeviceGuard g(ctx->device);
    hipStream_t s = ctx->stream;
    StreamSyncOnError guard(s);
    Carver c;
    const size_t oQ = c.take((size_t)nq * 4), oS = c.take((size_t)nq * sizeof(plslam_bow_pl_stats));
    const size_t oO = c.take((size_t)nq * n * 8);
    int rc;
    if ((rc = db->scratch.reserve(c.off))) return rc;
    char* d = db->scratch.as<char>();
    PLSLAM_HIP_CHECK(hipMemcpyAsync(d + oQ, queries, (size_t)nq * 4, hipMemcpyHostToDevice, s));
    PLSLAM_HIP_CHECK(hipMemcpyAsync(d + oS, st.data(), (size_t)nq * sizeof(plslam_bow_pl_stats), hipMemcpyHostToDevice, s));
    ScoreArgs a{};
    a.tab = db->tab.as<int32_t>();
    a.pw = db->pw.as<int32_t>();
    a.pv = db->pv.as<double>();
    a.lw = db->lw.as<int32_t>();
    a.lv = db->lv.as<double>();
    a.mode = db->mode;
    a.ntarget = n;
    a.cap_p = cap_p;
    a.cap_l = cap_l;
    a.queries = (const int32_t*)(d + oQ);
    a.stats = (const plslam_bow_pl_stats*)(d + oS);
    a.alive = nullptr;
    a.out = (double*)(d + oO);
    a.out_stride = n;
    if ((rc = launch_score(a, nq, s))) return rc;
    PLSLAM_HIP_CHECK(hipMemcpyAsync(out, d + oO, (size_t)nq * n * 8, hipMemcpyDeviceToHost, s));
    PLSLAM_HIP_CHECK(hipStreamSynchronize(s));
    guard.dismiss();
    return PLSLAM_OK;
}

}  // extern "C"
