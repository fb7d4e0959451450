// K111-K130 -- training a DBoW2 vocabulary on the device: TemplatedVocabulary::create's hierarchical k-means++
// (3rdparty/DBoW2/include/DBoW2/TemplatedVocabulary.h:536-976), one whole tree level per pass.  The contract, with the three
// departures from the reference, is in include/plslam_bow_train.h; the draws are bow_train_draw.h's.
//
// State: the descriptors stay where they are.  perm[0 .. M) lists the rows that are still being clustered, grouped by node and
// in their original order inside a node; nbeg[v] .. nbeg[v + 1] is node v's range.  Every kernel is launched over the positions
// of perm (or over the nodes, or over the (node, cluster) pairs): the root -- one node of N rows -- and the deepest level -- many
// nodes of a few rows -- run through the same launches.
//
//   K111 k_bt_rows         identity permutation; the document of every row (bisection of the offsets)
//   K112 k_bt_node_flags   per node: does it run k-means (more than k rows)      -> K114-K116 -> its counter slot
//   K113 k_bt_level_init   per position: its node; a node of at most k rows gets one cluster per row, in order (:638-648)
//   K114-K116 k_bt_scan_*  inclusive int64 prefix sum: tiles of 1024, the tiles' totals by one workgroup, the add
//   K117 k_bt_node_init    per node: cluster count, the first centre int((r / 2^31) n) (:835)
//   K118 k_bt_seed_dist    seeding round j, per position: min distance to the centres so far (:852-860)
//   K119 k_bt_seed_pick    per node: the cut from its own sum; the first position whose inclusive sum is >= the cut, found by
//                          bisection of the prefix sums; that row is centre j.  A node whose sum is 0 stops seeding (:865-889)
//   K120 k_bt_assign       Lloyd, per position of a running node: the first minimum over its centres by strict '<' (:712-723);
//                          a changed assignment raises the node's flag
//   K121 k_bt_round_end    per node: converged (no change), capped (max_iters), or on -- and then the word the host reads
//   K122 k_bt_count        per position of a running node: ballots restricted to the lanes of the same (node, cluster) count
//                          each of the 256 bits, one relaxed integer atomic add per bit and wave into the cluster's counters
//   K123 k_bt_centres      one wave per (running node, cluster): bit b set iff count_b >= n / 2 + n % 2 (FORB::meanValue); an
//                          empty group keeps its centre and is counted; the counters are left zeroed
//   K124 k_bt_sizes        per position: the final groups' sizes
//   K125 k_bt_child_flags  per (node, cluster): is it a child, is the child clustered on the next level   -> K114-K116
//   K126 k_bt_children     per child: its descriptor into the tree (level order), its path key into the next node table
//   K127 k_bt_keys         per position: the distribution key (the next level's node, or -1: the row is done and gets its leaf)
//                          -> K75-K78 (distribute_dev.hpp): the stable regrouping and the next level's nbeg
//   K128 k_bt_perm         the next permutation
//   K129 k_bt_ni           per position of the rows sorted stably by word (K75-K78): a word's documents ascend, so Ni[word] is
//                          the count of positions whose document differs from the predecessor's
// The descent behind K129 is K19 (bow.hip) over the training rows with the finished tree.
//
// Integer sums are the same in any order of arrival: the atomics are relaxed, no fence anywhere, kernel boundaries order the
// passes, and the result is the same bytes on every run.  The host reads one word per Lloyd round and five small tables per level.
#include "common.hpp"

#include <cstring>

#include "bow_train_plan.hpp"
#include "distribute_dev.hpp"

static_assert(plslam::BT_DIST_TILE == plslam::DIST_TILE, "the planner sizes the distribution's table by DIST_TILE");

namespace plslam {
namespace {

struct TrainDev {                          // what the kernels read of one trainer at one level
    const uint32_t* desc;                  // N x 8 words
    const int32_t* doc_off;
    int32_t N, n_docs, k, L, level, max_iters;
    int32_t M, nV, nS;                     // live positions, visited nodes, nodes that run k-means
    int32_t level_base, tree_cap, max_visited;
    int32_t *doc, *perm, *perm_next, *pnode, *asg, *mind;
    int64_t* psum;
    int32_t* nbeg;
    uint64_t *nkey, *nkey_next;
    int32_t *ncl, *nrun, *nround, *nchg, *ncap, *nempty, *snode;
    int64_t *sflag, *sscan;
    uint32_t* cent;                        // nV x k x 8 words
    int32_t* cnt;                          // nS x k x BT_CNT_STRIDE
    int32_t* csize;                        // nV x k
    int64_t *citem, *cscan;
    uint32_t* tree;                        // tree_cap x 8 words
    int32_t *key, *ids, *leaf, *word, *ni;
    int32_t* stat;                         // [0]: does any node go on
};

__device__ __forceinline__ void load_row(const uint32_t* desc, int32_t row, uint32_t (&q)[8])
{
    const gvec4_t a = g_(reinterpret_cast<const gvec4_t*>(desc))[(size_t)row * 2];
    const gvec4_t b = g_(reinterpret_cast<const gvec4_t*>(desc))[(size_t)row * 2 + 1];
    q[0] = a.x; q[1] = a.y; q[2] = a.z; q[3] = a.w; q[4] = b.x; q[5] = b.y; q[6] = b.z; q[7] = b.w;
}
__device__ __forceinline__ void copy_desc(uint32_t* dst, const uint32_t* src)       // 8 words, both 32-byte aligned
{
    g_(reinterpret_cast<gvec4_t*>(dst))[0] = g_(reinterpret_cast<const gvec4_t*>(src))[0];
    g_(reinterpret_cast<gvec4_t*>(dst))[1] = g_(reinterpret_cast<const gvec4_t*>(src))[1];
}
__device__ __forceinline__ int dist_to(const uint32_t (&q)[8], const uint32_t* c)
{
    const gvec4_t a = g_(reinterpret_cast<const gvec4_t*>(c))[0], b = g_(reinterpret_cast<const gvec4_t*>(c))[1];
    return __popc(q[0] ^ a.x) + __popc(q[1] ^ a.y) + __popc(q[2] ^ a.z) + __popc(q[3] ^ a.w) + __popc(q[4] ^ b.x) +
           __popc(q[5] ^ b.y) + __popc(q[6] ^ b.z) + __popc(q[7] ^ b.w);
}
__device__ __forceinline__ uint32_t* centre_of(const TrainDev& T, int32_t node, int32_t c)
{
    return T.cent + ((size_t)node * T.k + c) * 8;
}

__global__ __launch_bounds__(BT_THREADS) void k_bt_rows(TrainDev T)
{
    const int64_t i = (int64_t)blockIdx.x * BT_THREADS + threadIdx.x;
    if (i >= T.N) return;
    g_(T.perm)[i] = (int32_t)i;
    g_(T.leaf)[i] = 0;
    int32_t lo = 0, hi = T.n_docs - 1;                             // the document d with off[d] <= i < off[d + 1]
    while (lo < hi) {
        const int32_t mid = lo + ((hi - lo) >> 1);
        if (g_(T.doc_off)[mid + 1] > (int32_t)i) hi = mid;
        else lo = mid + 1;
    }
    g_(T.doc)[i] = lo;
}

__global__ __launch_bounds__(BT_THREADS) void k_bt_node_flags(TrainDev T)
{
    const int64_t v = (int64_t)blockIdx.x * BT_THREADS + threadIdx.x;
    if (v >= T.nV) return;
    g_(T.sflag)[v] = g_(T.nbeg)[v + 1] - g_(T.nbeg)[v] > T.k ? 1 : 0;
}

__global__ __launch_bounds__(BT_THREADS) void k_bt_level_init(TrainDev T)
{
    const int64_t p = (int64_t)blockIdx.x * BT_THREADS + threadIdx.x;
    if (p >= T.M) return;
    int32_t lo = 0, hi = T.nV - 1;                                 // the node v with nbeg[v] <= p < nbeg[v + 1]
    while (lo < hi) {
        const int32_t mid = lo + ((hi - lo) >> 1);
        if (g_(T.nbeg)[mid + 1] > (int32_t)p) hi = mid;
        else lo = mid + 1;
    }
    const int32_t beg = g_(T.nbeg)[lo], n = g_(T.nbeg)[lo + 1] - beg;
    g_(T.pnode)[p] = lo;
    g_(T.mind)[p] = 0;
    if (n <= T.k) {                                                // trivial case: one cluster per feature, in order
        const int32_t c = (int32_t)p - beg;
        g_(T.asg)[p] = c;
        copy_desc(centre_of(T, lo, c), T.desc + (size_t)g_(T.perm)[p] * 8);
    } else {
        g_(T.asg)[p] = -1;
    }
}

// ---- the prefix sum ---------------------------------------------------------------------------------------------------------
template <class TIn>
__global__ __launch_bounds__(BT_THREADS) void k_bt_scan_tiles(const TIn* in, int64_t* out, int64_t* totals, int32_t n)
{
    __shared__ int64_t s_w[BT_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int64_t i0 = (int64_t)blockIdx.x * BT_SCAN_TILE + tid * 4;
    int64_t v[4], sum = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        v[e] = i0 + e < n ? (int64_t)g_(in)[i0 + e] : 0;
        sum += v[e];
    }
    int64_t incl = sum;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int64_t t = __shfl_up((long long)incl, o);
        if (lane >= o) incl += t;
    }
    if (lane == 63) s_w[wv] = incl;
    __syncthreads();
    int64_t before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < BT_THREADS / 64; ++w) {
        const int64_t c = s_w[w];
        before += w < wv ? c : 0;
        all += c;
    }
    int64_t run = before + incl - sum;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        run += v[e];
        if (i0 + e < n) g_(out)[i0 + e] = run;
    }
    if (tid == 0) g_(totals)[blockIdx.x] = all;
}

__global__ __launch_bounds__(BT_SCAN_NT) void k_bt_scan_totals(int64_t* totals, int32_t ntiles)      // -> exclusive, in place
{
    __shared__ int64_t s_w[BT_SCAN_NT / 64];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    int64_t carry = 0;
    for (int32_t base = 0; base < ntiles; base += BT_SCAN_NT) {
        const int32_t i = base + tid;
        const int64_t v = i < ntiles ? g_(totals)[i] : 0;
        int64_t incl = v;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int64_t t = __shfl_up((long long)incl, o);
            if (lane >= o) incl += t;
        }
        if (lane == 63) s_w[wv] = incl;
        __syncthreads();
        int64_t before = 0, all = 0;
#pragma unroll
        for (int w = 0; w < BT_SCAN_NT / 64; ++w) {
            const int64_t c = s_w[w];
            before += w < wv ? c : 0;
            all += c;
        }
        if (i < ntiles) g_(totals)[i] = carry + before + incl - v;
        carry += all;
        __syncthreads();
    }
}

__global__ __launch_bounds__(BT_THREADS) void k_bt_scan_add(int64_t* out, const int64_t* totals, int32_t n)
{
    const int64_t i = (int64_t)blockIdx.x * BT_THREADS + threadIdx.x;
    if (i < n) g_(out)[i] += g_(totals)[i / BT_SCAN_TILE];
}

// ---- seeding ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BT_THREADS) void k_bt_node_init(TrainDev T)
{
    const int64_t v = (int64_t)blockIdx.x * BT_THREADS + threadIdx.x;
    if (v >= T.nV) return;
    const int32_t beg = g_(T.nbeg)[v], n = g_(T.nbeg)[v + 1] - beg;
    g_(T.nround)[v] = 0;
    g_(T.nchg)[v] = 0;
    g_(T.ncap)[v] = 0;
    g_(T.nempty)[v] = 0;
    if (n <= T.k) {
        g_(T.ncl)[v] = n;
        g_(T.nrun)[v] = 0;
        return;
    }
    g_(T.ncl)[v] = 1;
    g_(T.nrun)[v] = 1;
    const int64_t slot = g_(T.sscan)[v] - 1;
    if (slot >= 0 && slot < T.nS) g_(T.snode)[slot] = (int32_t)v;
    int32_t i = bt_first_index(g_(T.nkey)[v], n);
    i = min(max(i, 0), n - 1);
    copy_desc(centre_of(T, (int32_t)v, 0), T.desc + (size_t)g_(T.perm)[beg + i] * 8);
}

__global__ __launch_bounds__(BT_THREADS) void k_bt_seed_dist(TrainDev T, int32_t j)
{
    const int64_t p = (int64_t)blockIdx.x * BT_THREADS + threadIdx.x;
    if (p >= T.M) return;
    const int32_t v = g_(T.pnode)[p];
    if (!g_(T.nrun)[v] || g_(T.ncl)[v] != j) return;               // (a node that stopped seeding keeps ncl < j)
    uint32_t q[8];
    load_row(T.desc, g_(T.perm)[p], q);
    const int d = dist_to(q, centre_of(T, v, j - 1));
    g_(T.mind)[p] = j == 1 ? d : min(g_(T.mind)[p], d);
}

__global__ __launch_bounds__(BT_THREADS) void k_bt_seed_pick(TrainDev T, int32_t j)
{
    const int64_t v = (int64_t)blockIdx.x * BT_THREADS + threadIdx.x;
    if (v >= T.nV) return;
    if (!g_(T.nrun)[v] || g_(T.ncl)[v] != j) return;
    const int32_t beg = g_(T.nbeg)[v], end = g_(T.nbeg)[v + 1];
    const int64_t base = beg > 0 ? g_(T.psum)[beg - 1] : 0;
    const int64_t sum = g_(T.psum)[end - 1] - base;
    if (sum <= 0) return;                                          // every row lies on a centre: fewer than k clusters
    const double cut = bt_cut(g_(T.nkey)[v], (uint32_t)j, (double)sum);
    int32_t lo = beg, hi = end - 1;                                // the first position with d_up_now >= cut_d, else the last
    while (lo < hi) {
        const int32_t mid = lo + ((hi - lo) >> 1);
        if ((double)(g_(T.psum)[mid] - base) >= cut) hi = mid;
        else lo = mid + 1;
    }
    copy_desc(centre_of(T, (int32_t)v, j), T.desc + (size_t)g_(T.perm)[lo] * 8);
    g_(T.ncl)[v] = j + 1;
}

// ---- a Lloyd round ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BT_THREADS) void k_bt_assign(TrainDev T)
{
    const int64_t p = (int64_t)blockIdx.x * BT_THREADS + threadIdx.x;
    if (p >= T.M) return;
    const int32_t v = g_(T.pnode)[p];
    if (!g_(T.nrun)[v]) return;
    uint32_t q[8];
    load_row(T.desc, g_(T.perm)[p], q);
    const int32_t m = g_(T.ncl)[v];
    const uint32_t* c0 = centre_of(T, v, 0);
    int best = 0, best_d = dist_to(q, c0);
    for (int c = 1; c < m; ++c) {
        const int d = dist_to(q, c0 + (size_t)c * 8);
        if (d < best_d) { best_d = d; best = c; }
    }
    if (best != g_(T.asg)[p]) {
        g_(T.asg)[p] = best;
        g_(T.nchg)[v] = 1;
    }
}

__global__ __launch_bounds__(BT_THREADS) void k_bt_round_end(TrainDev T)
{
    const int64_t v = (int64_t)blockIdx.x * BT_THREADS + threadIdx.x;
    if (v >= T.nV || !g_(T.nrun)[v]) return;
    const int32_t r = g_(T.nround)[v] + 1;
    g_(T.nround)[v] = r;
    if (!g_(T.nchg)[v]) {
        g_(T.nrun)[v] = 0;                                         // the assignment equals the previous one
    } else if (r >= T.max_iters) {
        g_(T.nrun)[v] = 0;
        g_(T.ncap)[v] = 1;
    } else {
        g_(T.nchg)[v] = 0;
        g_(T.stat)[0] = 1;
    }
}

__global__ __launch_bounds__(BT_THREADS) void k_bt_count(TrainDev T)
{
    const int64_t p = (int64_t)blockIdx.x * BT_THREADS + threadIdx.x;
    const int lane = threadIdx.x & 63;
    bool run = p < T.M;
    int32_t gkey = -1;
    uint32_t q[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (run) {
        const int32_t v = g_(T.pnode)[p];
        run = g_(T.nrun)[v] != 0;
        if (run) {
            const int64_t slot = g_(T.sscan)[v] - 1;
            const int32_t c = g_(T.asg)[p];
            run = slot >= 0 && slot < T.nS && c >= 0 && c < T.k;
            if (run) {
                gkey = (int32_t)slot * T.k + c;
                load_row(T.desc, g_(T.perm)[p], q);
            }
        }
    }
    uint64_t todo = __ballot(run);
    while (todo) {                                                 // one pass per (node, cluster) present in the wave
        const int leader = __ffsll((unsigned long long)todo) - 1;
        const int32_t lk = __shfl(gkey, leader);
        const bool mine = run && gkey == lk;
        const uint64_t group = __ballot(mine);
        todo &= ~group;
        int32_t* base = T.cnt + (size_t)lk * BT_CNT_STRIDE;
#pragma unroll
        for (int h = 0; h < 4; ++h) {                              // counters 64 h .. 64 h + 63: words 2 h and 2 h + 1
            int my = 0;
#pragma unroll
            for (int b = 0; b < 64; ++b) {
                const uint64_t m = __ballot(mine && ((q[2 * h + (b >> 5)] >> (b & 31)) & 1u));
                if (lane == b) my = __popcll(m);
            }
            if (my) atomic_add_global(base + h * 64 + lane, my);
        }
        if (lane == leader) atomic_add_global(base + 256, __popcll(group));
    }
}

__global__ __launch_bounds__(BT_THREADS) void k_bt_centres(TrainDev T)
{
    const int lane = threadIdx.x & 63;
    const int64_t w = (int64_t)blockIdx.x * (BT_THREADS / 64) + (threadIdx.x >> 6);
    if (w >= (int64_t)T.nS * T.k) return;
    const int32_t slot = (int32_t)(w / T.k), c = (int32_t)(w % T.k);
    const int32_t v = g_(T.snode)[slot];
    if (v < 0 || v >= T.nV || !g_(T.nrun)[v] || c >= g_(T.ncl)[v]) return;
    int32_t* base = T.cnt + (size_t)w * BT_CNT_STRIDE;
    const int32_t n = g_(base)[256];
    if (n == 0) {                                                  // departure 2: the centre stays
        if (lane == 0) atomic_add_global(T.nempty + v, 1);
        return;
    }
    const int32_t need = n / 2 + n % 2;
    uint32_t* cen = centre_of(T, v, c);
#pragma unroll
    for (int h = 0; h < 4; ++h) {
        const uint64_t m = __ballot(g_(base)[h * 64 + lane] >= need);
        g_(base)[h * 64 + lane] = 0;
        if (lane == 0) {
            g_(cen)[2 * h] = (uint32_t)m;
            g_(cen)[2 * h + 1] = (uint32_t)(m >> 32);
        }
    }
    if (lane == 0) g_(base)[256] = 0;
}

// ---- ending a level ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BT_THREADS) void k_bt_sizes(TrainDev T)
{
    const int64_t p = (int64_t)blockIdx.x * BT_THREADS + threadIdx.x;
    if (p >= T.M) return;
    const int32_t c = g_(T.asg)[p];
    if (c < 0 || c >= T.k) return;
    atomic_add_global(T.csize + (size_t)g_(T.pnode)[p] * T.k + c, 1);
}

__global__ __launch_bounds__(BT_THREADS) void k_bt_child_flags(TrainDev T)
{
    const int64_t it = (int64_t)blockIdx.x * BT_THREADS + threadIdx.x;
    if (it >= (int64_t)T.nV * T.k) return;
    const int32_t v = (int32_t)(it / T.k), c = (int32_t)(it % T.k);
    const bool has = c < g_(T.ncl)[v];
    const bool vis = has && T.level < T.L && g_(T.csize)[it] > 1;
    g_(T.citem)[it] = ((int64_t)(has ? 1 : 0) << 32) | (int64_t)(vis ? 1 : 0);
}

__global__ __launch_bounds__(BT_THREADS) void k_bt_children(TrainDev T)
{
    const int64_t it = (int64_t)blockIdx.x * BT_THREADS + threadIdx.x;
    if (it >= (int64_t)T.nV * T.k) return;
    const int32_t v = (int32_t)(it / T.k), c = (int32_t)(it % T.k);
    if (c >= g_(T.ncl)[v]) return;
    const int64_t S = g_(T.cscan)[it];
    const int64_t id = (int64_t)T.level_base + (S >> 32) - 1;
    if (id >= 1 && id < T.tree_cap) copy_desc(T.tree + (size_t)id * 8, centre_of(T, v, c));
    if (T.level < T.L && g_(T.csize)[it] > 1) {
        const int64_t ci = (S & 0xFFFFFFFFll) - 1;
        if (ci >= 0 && ci < T.max_visited) g_(T.nkey_next)[ci] = bt_child_key(g_(T.nkey)[v], c);
    }
}

__global__ __launch_bounds__(BT_THREADS) void k_bt_keys(TrainDev T)
{
    const int64_t p = (int64_t)blockIdx.x * BT_THREADS + threadIdx.x;
    if (p >= T.M) return;
    const int32_t c = g_(T.asg)[p];
    const int64_t it = (int64_t)g_(T.pnode)[p] * T.k + (c < 0 ? 0 : c);
    const int64_t S = g_(T.cscan)[it];
    if (T.level < T.L && g_(T.csize)[it] > 1) {
        g_(T.key)[p] = (int32_t)(S & 0xFFFFFFFFll) - 1;
    } else {
        g_(T.key)[p] = -1;
        g_(T.leaf)[g_(T.perm)[p]] = T.level_base + (int32_t)(S >> 32) - 1;
    }
}

__global__ __launch_bounds__(BT_THREADS) void k_bt_perm(TrainDev T, int32_t n_next)
{
    const int64_t i = (int64_t)blockIdx.x * BT_THREADS + threadIdx.x;
    if (i >= n_next) return;
    const int32_t p = g_(T.ids)[i];
    if (p >= 0 && p < T.M) g_(T.perm_next)[i] = g_(T.perm)[p];
}

__global__ __launch_bounds__(BT_THREADS) void k_bt_ni(TrainDev T, const int32_t* sorted_word, int32_t n_words)
{
    const int64_t i = (int64_t)blockIdx.x * BT_THREADS + threadIdx.x;
    if (i >= T.N) return;
    const int32_t w = g_(sorted_word)[i];
    if (w < 0 || w >= n_words) return;
    const int32_t d = g_(T.doc)[g_(T.ids)[i]];
    if (i == 0 || g_(sorted_word)[i - 1] != w || g_(T.doc)[g_(T.ids)[i - 1]] != d) atomic_add_global(T.ni + w, 1);
}

}  // namespace
}  // namespace plslam

using namespace plslam;

struct plslam_bow_trainer {
    plslam_ctx* ctx = nullptr;
    BowTrainPlan P;
    DevBuf buf;
    const uint8_t* desc = nullptr;         // device: the trainer's copy or the caller's block
    const int32_t* doc_off = nullptr;
    bool done = false;
    BowTrainTree tree;
    BowTrainExport ex;
    std::vector<int32_t> leaf, word;       // per descriptor: the training partition's node id, the descent's word
    plslam_bow_train_stats stats{};
};

namespace {

int refuse(int code, const BtWhy& why)
{
    set_last_error(why.fmt, why.a, why.b);
    return code;
}

template <class TIn> int scan_enqueue(const TIn* in, int64_t* out, int64_t* totals, int32_t n, hipStream_t s)
{
    if (n <= 0) return PLSLAM_OK;
    const int32_t tiles = bt_scan_tiles(n);
    hipLaunchKernelGGL(k_bt_scan_tiles<TIn>, dim3(tiles), dim3(BT_THREADS), 0, s, in, out, totals, n);
    hipLaunchKernelGGL(k_bt_scan_totals, dim3(1), dim3(BT_SCAN_NT), 0, s, totals, tiles);
    hipLaunchKernelGGL(k_bt_scan_add, dim3(bt_blocks(n)), dim3(BT_THREADS), 0, s, out, (const int64_t*)totals, n);
    PLSLAM_HIP_CHECK(hipGetLastError());
    return PLSLAM_OK;
}

TrainDev train_dev(const plslam_bow_trainer* t)
{
    const BowTrainPlan& P = t->P;
    char* b = t->buf.as<char>();
    TrainDev T{};
    T.desc = reinterpret_cast<const uint32_t*>(t->desc);
    T.doc_off = t->doc_off;
    T.N = P.N; T.n_docs = P.n_docs; T.k = P.k; T.L = P.L; T.max_iters = P.max_iters;
    T.tree_cap = (int32_t)P.tree_cap;
    T.max_visited = (int32_t)P.max_visited;
    T.doc = (int32_t*)(b + P.oDoc);
    T.perm = (int32_t*)(b + P.oPermA); T.perm_next = (int32_t*)(b + P.oPermB);
    T.pnode = (int32_t*)(b + P.oPnode); T.asg = (int32_t*)(b + P.oAsg); T.mind = (int32_t*)(b + P.oMind);
    T.psum = (int64_t*)(b + P.oPsum);
    T.nbeg = (int32_t*)(b + P.oNbegA);
    T.nkey = (uint64_t*)(b + P.oNkeyA); T.nkey_next = (uint64_t*)(b + P.oNkeyB);
    T.ncl = (int32_t*)(b + P.oNcl); T.nrun = (int32_t*)(b + P.oNrun); T.nround = (int32_t*)(b + P.oNround);
    T.nchg = (int32_t*)(b + P.oNchg); T.ncap = (int32_t*)(b + P.oNcap); T.nempty = (int32_t*)(b + P.oNempty);
    T.snode = (int32_t*)(b + P.oSnode); T.sflag = (int64_t*)(b + P.oSflag); T.sscan = (int64_t*)(b + P.oSscan);
    T.cent = (uint32_t*)(b + P.oCent); T.cnt = (int32_t*)(b + P.oCnt); T.csize = (int32_t*)(b + P.oCsize);
    T.citem = (int64_t*)(b + P.oCitem); T.cscan = (int64_t*)(b + P.oCscan);
    T.tree = (uint32_t*)(b + P.oTree);
    T.key = (int32_t*)(b + P.oKey); T.ids = (int32_t*)(b + P.oIds); T.leaf = (int32_t*)(b + P.oLeaf);
    T.word = (int32_t*)(b + P.oWord); T.ni = (int32_t*)(b + P.oNi);
    T.stat = (int32_t*)(b + P.oStat);
    return T;
}

#define BT_LAUNCH(kernel, blocks, ...)                                                          \
    do {                                                                                        \
        if ((blocks) > 0) hipLaunchKernelGGL(kernel, dim3(blocks), dim3(BT_THREADS), 0, s, __VA_ARGS__); \
    } while (0)

// the tree: every level clustered on the context's stream; fills t->tree and the level-order leaf of every row (device)
int train_tree(plslam_bow_trainer* t, hipStream_t s)
{
    const BowTrainPlan& P = t->P;
    TrainDev T = train_dev(t);
    char* b = t->buf.as<char>();
    int64_t* totals = (int64_t*)(b + P.oTot);
    const DistScratch ds{(int32_t*)(b + P.oKeyA), (int32_t*)(b + P.oKeyB), (int32_t*)(b + P.oIdTmp), (uint32_t*)(b + P.oTable)};
    int rc;
    BowTrainLevel lv = bow_train_begin(&t->tree, P.k, P.L, P.N);
    BT_LAUNCH(k_bt_rows, bt_blocks(P.N), T);
    const int32_t nbeg0[2] = {0, P.N};
    PLSLAM_HIP_CHECK(hipMemcpyAsync(T.nbeg, nbeg0, 8, hipMemcpyHostToDevice, s));
    PLSLAM_HIP_CHECK(hipMemcpyAsync(T.nkey, &P.root_key, 8, hipMemcpyHostToDevice, s));
    PLSLAM_HIP_CHECK(hipStreamSynchronize(s));                    // (the two host words above are this frame's)
    std::vector<int32_t> h_ncl, h_csize, h_round, h_cap, h_empty;
    int32_t* nbeg_next = (int32_t*)(b + P.oNbegB);
    while (lv.n_visited > 0) {
        if (lv.n_visited > P.max_visited || lv.n_slots > P.max_slots || lv.n_rows > P.N || lv.level > P.L) {
            set_last_error("bow train: level %d outgrew the plan (%d nodes, %d slots)", lv.level, lv.n_visited, lv.n_slots);
            return PLSLAM_ERANGE;
        }
        T.level = lv.level; T.M = lv.n_rows; T.nV = lv.n_visited; T.nS = lv.n_slots; T.level_base = lv.base;
        const int32_t pb = bt_blocks(T.M), vb = bt_blocks(T.nV), items = T.nV * T.k, ib = bt_blocks(items);
        BT_LAUNCH(k_bt_node_flags, vb, T);
        if ((rc = scan_enqueue(T.sflag, T.sscan, totals, T.nV, s))) return rc;
        BT_LAUNCH(k_bt_level_init, pb, T);
        BT_LAUNCH(k_bt_node_init, vb, T);
        if (T.nS > 0) {
            PLSLAM_HIP_CHECK(hipMemsetAsync(T.cnt, 0, (size_t)T.nS * T.k * BT_CNT_STRIDE * 4, s));
            for (int32_t j = 1; j < T.k; ++j) {
                BT_LAUNCH(k_bt_seed_dist, pb, T, j);
                if ((rc = scan_enqueue(T.mind, T.psum, totals, T.M, s))) return rc;
                BT_LAUNCH(k_bt_seed_pick, vb, T, j);
            }
            for (;;) {
                int32_t goon = 0;
                PLSLAM_HIP_CHECK(hipMemsetAsync(T.stat, 0, 4, s));
                BT_LAUNCH(k_bt_assign, pb, T);
                BT_LAUNCH(k_bt_round_end, vb, T);
                PLSLAM_HIP_CHECK(hipMemcpyAsync(&goon, T.stat, 4, hipMemcpyDeviceToHost, s));
                PLSLAM_HIP_CHECK(hipStreamSynchronize(s));
                if (!goon) break;
                BT_LAUNCH(k_bt_count, pb, T);
                BT_LAUNCH(k_bt_centres, bt_wave_blocks((int64_t)T.nS * T.k), T);
            }
        }
        PLSLAM_HIP_CHECK(hipMemsetAsync(T.csize, 0, (size_t)items * 4, s));
        BT_LAUNCH(k_bt_sizes, pb, T);
        BT_LAUNCH(k_bt_child_flags, ib, T);
        if ((rc = scan_enqueue(T.citem, T.cscan, totals, items, s))) return rc;
        BT_LAUNCH(k_bt_children, ib, T);
        BT_LAUNCH(k_bt_keys, pb, T);
        PLSLAM_HIP_CHECK(hipGetLastError());
        h_ncl.resize((size_t)T.nV); h_round.resize((size_t)T.nV); h_cap.resize((size_t)T.nV); h_empty.resize((size_t)T.nV);
        h_csize.resize((size_t)items);
        PLSLAM_HIP_CHECK(hipMemcpyAsync(h_ncl.data(), T.ncl, (size_t)T.nV * 4, hipMemcpyDeviceToHost, s));
        PLSLAM_HIP_CHECK(hipMemcpyAsync(h_round.data(), T.nround, (size_t)T.nV * 4, hipMemcpyDeviceToHost, s));
        PLSLAM_HIP_CHECK(hipMemcpyAsync(h_cap.data(), T.ncap, (size_t)T.nV * 4, hipMemcpyDeviceToHost, s));
        PLSLAM_HIP_CHECK(hipMemcpyAsync(h_empty.data(), T.nempty, (size_t)T.nV * 4, hipMemcpyDeviceToHost, s));
        PLSLAM_HIP_CHECK(hipMemcpyAsync(h_csize.data(), T.csize, (size_t)items * 4, hipMemcpyDeviceToHost, s));
        PLSLAM_HIP_CHECK(hipStreamSynchronize(s));
        for (int32_t v = 0; v < T.nV; ++v)
            if (h_ncl[(size_t)v] < 1 || h_ncl[(size_t)v] > T.k) {
                set_last_error("bow train: node %d of level %d came back with %d clusters", v, lv.level, h_ncl[(size_t)v]);
                return PLSLAM_EHIP;
            }
        const BowTrainLevel nx = bow_train_add_level(&t->tree, lv, h_ncl.data(), h_csize.data(), h_round.data(), h_cap.data(),
                                                     h_empty.data());
        if ((int64_t)t->tree.parent.size() > P.tree_cap) {
            set_last_error("bow train: the tree outgrew the plan (%ld nodes)", (long)t->tree.parent.size());
            return PLSLAM_ERANGE;
        }
        if (nx.n_visited > 0) {
            dist_enqueue(s, T.key, T.M, nx.n_visited, T.ids, nbeg_next, ds);
            BT_LAUNCH(k_bt_perm, bt_blocks(nx.n_rows), T, nx.n_rows);
            PLSLAM_HIP_CHECK(hipGetLastError());
            std::swap(T.perm, T.perm_next);
            std::swap(T.nkey, T.nkey_next);
            std::swap(T.nbeg, nbeg_next);
        }
        lv = nx;
    }
    return PLSLAM_OK;
}

}  // namespace

namespace plslam {
int bow_descend_enqueue(plslam_bow_vocab* v, const uint8_t* q, int32_t n, int32_t* word, hipStream_t s);   // bow.hip: K19
}

namespace {

int create_common(plslam_ctx* ctx, const BowTrainPlan& P, const uint8_t* desc, const int32_t* off, bool host_call,
                  plslam_bow_trainer** out)
{
    plslam_bow_trainer* t = new plslam_bow_trainer();
    t->ctx = ctx;
    t->P = P;
    int rc = t->buf.reserve(P.bytes);
    if (rc == PLSLAM_OK && host_call) {
        char* b = t->buf.as<char>();
        if (hipMemcpy(b + P.oDesc, desc, (size_t)P.N * 32, hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(b + P.oOff, off, ((size_t)P.n_docs + 1) * 4, hipMemcpyHostToDevice) != hipSuccess) {
            set_last_error("bow train: upload failed");
            rc = PLSLAM_EHIP;
        }
        t->desc = (const uint8_t*)(b + P.oDesc);
        t->doc_off = (const int32_t*)(b + P.oOff);
    } else {
        t->desc = desc;
        t->doc_off = off;
    }
    if (rc) {
        t->buf.release();
        delete t;
        return rc;
    }
    *out = t;
    return PLSLAM_OK;
}

}  // namespace

extern "C" {

int plslam_bow_train_create(plslam_ctx* ctx, const plslam_bow_train_params* params, const uint8_t* desc,
                            const int32_t* doc_offsets, int32_t n_docs, plslam_bow_trainer** out)
{
    PLSLAM_REQUIRE(ctx && out, PLSLAM_EINVAL);
    *out = nullptr;
    BowTrainPlan P;
    int rc;
    if ((rc = bow_train_check(params, desc, doc_offsets, n_docs, true, 0, &P))) return refuse(rc, P.why);
    std::lock_guard<std::mutex> lk(ctx->mu);
    DeviceGuard g(ctx->device);
    return create_common(ctx, P, desc, doc_offsets, true, out);
}

int plslam_bow_train_create_dev(plslam_ctx* ctx, const plslam_bow_train_params* params, const uint8_t* desc,
                                const int32_t* doc_offsets, int32_t n_docs, int32_t n_total, plslam_bow_trainer** out)
{
    PLSLAM_REQUIRE(ctx && out, PLSLAM_EINVAL);
    *out = nullptr;
    BowTrainPlan P;
    int rc;
    if ((rc = bow_train_check(params, desc, doc_offsets, n_docs, false, n_total, &P))) return refuse(rc, P.why);
    std::lock_guard<std::mutex> lk(ctx->mu);
    DeviceGuard g(ctx->device);
    return create_common(ctx, P, desc, doc_offsets, false, out);
}

int plslam_bow_train_run(plslam_bow_trainer* t, plslam_bow_train_stats* stats)
{
    PLSLAM_REQUIRE(t, PLSLAM_EINVAL);
    plslam_ctx* ctx = t->ctx;
    const BowTrainPlan& P = t->P;
    hipStream_t s = ctx->stream;
    t->done = false;
    int rc;
    std::vector<uint8_t> tree_desc;
    {
        std::lock_guard<std::mutex> lk(ctx->mu);
        DeviceGuard g(ctx->device);
        StreamSyncOnError guard(s);
        if ((rc = train_tree(t, s))) return rc;
        tree_desc.assign(t->tree.parent.size() * 32, 0);
        PLSLAM_HIP_CHECK(hipMemcpyAsync(tree_desc.data(), t->buf.as<char>() + P.oTree, tree_desc.size(), hipMemcpyDeviceToHost, s));
        t->leaf.resize((size_t)P.N);
        PLSLAM_HIP_CHECK(hipMemcpyAsync(t->leaf.data(), t->buf.as<char>() + P.oLeaf, (size_t)P.N * 4, hipMemcpyDeviceToHost, s));
        PLSLAM_HIP_CHECK(hipStreamSynchronize(s));
        guard.dismiss();
    }
    bow_train_export(t->tree, tree_desc.data(), &t->ex);
    for (int32_t& l : t->leaf) l = l >= 0 && (size_t)l < t->ex.dbow.size() ? t->ex.dbow[(size_t)l] : -1;
    // the descent of every training row through the finished tree (K19), then Ni
    const int32_t n_nodes = (int32_t)t->ex.nodes.size(), n_words = (int32_t)t->ex.words.size();
    const plslam_bow_vocab_desc vd{P.k, P.L, PLSLAM_BOW_L1_NORM, P.weighting, n_nodes, n_words, t->ex.nodes.data(), t->ex.words.data()};
    plslam_bow_vocab* voc = nullptr;
    if ((rc = plslam_bow_vocab_create(ctx, &vd, &voc))) return rc;
    std::vector<int32_t> ni((size_t)n_words, 0);
    {
        std::lock_guard<std::mutex> lk(ctx->mu);
        DeviceGuard g(ctx->device);
        TrainDev T = train_dev(t);
        char* b = t->buf.as<char>();
        const DistScratch ds{(int32_t*)(b + P.oKeyA), (int32_t*)(b + P.oKeyB), (int32_t*)(b + P.oIdTmp), (uint32_t*)(b + P.oTable)};
        rc = bow_descend_enqueue(voc, t->desc, P.N, T.word, s);
        if (rc == PLSLAM_OK && (P.weighting == PLSLAM_BOW_TF_IDF || P.weighting == PLSLAM_BOW_IDF)) {
            const int32_t* sorted = dist_sort_enqueue(s, T.word, P.N, n_words, T.ids, ds);
            if (hipMemsetAsync(T.ni, 0, (size_t)n_words * 4, s) != hipSuccess) rc = PLSLAM_EHIP;
            BT_LAUNCH(k_bt_ni, bt_blocks(P.N), T, sorted, n_words);
            if (hipMemcpyAsync(ni.data(), T.ni, (size_t)n_words * 4, hipMemcpyDeviceToHost, s) != hipSuccess) rc = PLSLAM_EHIP;
        }
        t->word.resize((size_t)P.N);
        if (hipMemcpyAsync(t->word.data(), T.word, (size_t)P.N * 4, hipMemcpyDeviceToHost, s) != hipSuccess) rc = PLSLAM_EHIP;
        if (hipStreamSynchronize(s) != hipSuccess || hipGetLastError() != hipSuccess) rc = rc ? rc : PLSLAM_EHIP;
    }
    plslam_bow_vocab_destroy(voc);
    if (rc) {
        if (rc == PLSLAM_EHIP) set_last_error("bow train: the descent or the document counts failed on the device");
        return rc;
    }
    bow_train_weights(&t->ex, P.weighting, P.n_docs, ni.data());
    t->stats = plslam_bow_train_stats{n_nodes, n_words, t->tree.rounds, t->tree.empty, t->tree.capped, t->tree.rounds_max,
                                      t->tree.levels};
    t->done = true;
    if (stats) *stats = t->stats;
    return PLSLAM_OK;
}

int plslam_bow_train_sizes(plslam_bow_trainer* t, int32_t* n_nodes, int32_t* n_words)
{
    PLSLAM_REQUIRE(t && n_nodes && n_words && t->done, PLSLAM_EINVAL);
    *n_nodes = t->stats.n_nodes;
    *n_words = t->stats.n_words;
    return PLSLAM_OK;
}

int plslam_bow_train_export(plslam_bow_trainer* t, plslam_bow_node* nodes, plslam_bow_word* words)
{
    PLSLAM_REQUIRE(t && nodes && words && t->done, PLSLAM_EINVAL);
    std::memcpy(nodes, t->ex.nodes.data(), t->ex.nodes.size() * sizeof(plslam_bow_node));
    std::memcpy(words, t->ex.words.data(), t->ex.words.size() * sizeof(plslam_bow_word));
    return PLSLAM_OK;
}

int plslam_bow_train_download(plslam_bow_trainer* t, int32_t* leaf_node, int32_t* word)
{
    PLSLAM_REQUIRE(t && t->done, PLSLAM_EINVAL);
    if (leaf_node) std::memcpy(leaf_node, t->leaf.data(), t->leaf.size() * 4);
    if (word) std::memcpy(word, t->word.data(), t->word.size() * 4);
    return PLSLAM_OK;
}

void plslam_bow_train_destroy(plslam_bow_trainer* t)
{
    if (!t) return;
    {
        std::lock_guard<std::mutex> lk(t->ctx->mu);
        DeviceGuard g(t->ctx->device);
        (void)hipStreamSynchronize(t->ctx->stream);
        t->buf.release();
    }
    delete t;
}

}  // extern "C"
