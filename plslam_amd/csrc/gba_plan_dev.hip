// gba_plan_dev.hip -- the GBA plan built ON THE DEVICE from device columns (plslam_gba_plan_create_dev): what
// plslam_local_map_form_all + plslam_local_map_gather leave on the device goes into the plan without crossing PCIe, and the plan
// keeps no host copy of any list but kf_list.  The lists are those of gba_lists_build (gba_lists.hpp), entry for entry:
//   K89 k_gbp_columns       a lane per Vector6i row and per kf_list entry: the checks of gba_lists_build (a status word; what is
//                           stored is made safe, so no later kernel follows a bad index); plm / pkf / llm / lkf, the slot column
//                           of the inner LBA plan, the keys of the two landmark lists (-1 where the keyframe is not optimised)
//   K75-K78                 the stable distribution (distribute.hip), four times: lpp / lpo, llp / llo, kpp / kpo, klp / klo
//   K90 k_gbp_pair_count    a lane per position of lpo / llo: the pairs (o1, .) it starts, kf(o1) >= kf(o2); their sum in 64 bits
//   K91 k_gbp_publish       status, the four list lengths and the pair total to the page-locked block the host reads
//   K92 k_gbp_pair_emit     enumeration offsets (the look-back of lookback_dev.hpp over K90's counts), then key
//                           2 (k1 nkf + k2) + kind and pair of every (o1, o2), in gba_lists_build's enumeration order
//   K75-K77                 the distribution's passes over the pairs' keys (no ptr over all 2 nkf^2 keys)
//   K93 k_gbp_heads         a lane per sorted pair and per diagonal key: the first pair of each block (neighbour compare) and the
//                           diagonal blocks no pair falls in (bisection), each compacted in order behind a look-back
//   K94 k_gbp_block_info    a lane per block: its place in the merge of the two compacted lists (bisection of the other one), its
//                           first pair, its point and line pair counts
//   K95 k_gbp_block_scan    a lane per block in order: the exclusive sum of the blocks' chunk counts (look-back) -> GbaBlock; the
//                           block and chunk totals to the host
//   K96 k_gbp_layout        a lane per chunk (its block by bisection of the chunk offsets) and per pair (the pair the
//                           distribution put there): GbaChunk and the compact pair list
// No order comes from where an atomic lands (the only atomics: the status word's OR, the 64-bit pair total, the look-back's
// words and the distribution's LDS histogram), no device-scope fence, no flat access.
// Synchronisations: the inner LBA plan's own (plslam_lba_plan_create_dev: one), plus TWO here -- the counts behind K91 (the pair
// scratch is carved from them) and the block and chunk totals behind K95 (pairbuf and work are carved from them).  K96 and the
// copy of the blocks are enqueued behind the second one, on the stream every later call of the plan uses.
#include <cstring>
#include <new>

#include "distribute_dev.hpp"
#include "gba_plan.hpp"
#include "lookback_dev.hpp"

using namespace plslam;

namespace plslam {
namespace {

constexpr int GBP_NT = 256;
constexpr int GBP_NW = GBP_NT / 64;
// the page-locked words the builders' last kernels write
enum { W_STATUS = 0, W_LPO, W_LLO, W_KPO, W_KLO, W_PAIRS_LO, W_PAIRS_HI, W_NBLK, W_NCHUNK, W_WORDS = 16 };
// the device words (aux): the status, then the 64-bit pair total at an 8-byte boundary; (aux_pairs) the compactions' totals
enum { D_STATUS = 0, D_PAIRS = 2, D_WORDS = 64 };
enum { D_NPH = 0, D_NAD = 1 };
// status bits
enum { BAD_COLUMN = 1, BAD_KF_LOCAL = 2, BAD_KF_LIST = 4 };

unsigned wgs(int64_t n, int per) { return (unsigned)((n + per - 1) / per); }

struct GbpColumnArgs {
    const int32_t *pt_obs, *ls_obs, *kf_list;             // the caller's columns
    int32_t *plm, *pkf, *pslot, *pkey, *llm, *lkf, *lslot, *lkey, *status;
    int32_t np, nl, npt, nls, nkf, n_map;
};

__global__ void __launch_bounds__(GBP_NT)
k_gbp_columns(const GbpColumnArgs A)
{
    const int64_t t = (int64_t)blockIdx.x * GBP_NT + threadIdx.x;
    const int64_t nobs = (int64_t)A.np + A.nl;
    if (t >= nobs + A.nkf) return;
    if (t >= nobs) {                                        // kf_list names a slot out of range
        const int32_t v = g_(A.kf_list)[t - nobs];
        if (v < 0 || v >= A.n_map) atomicOr(A.status, BAD_KF_LIST);
        return;
    }
    const bool lines = t >= A.np;
    const int32_t o = (int32_t)(lines ? t - A.np : t);
    const int32_t* v = (lines ? A.ls_obs : A.pt_obs) + 6 * (size_t)o;
    int32_t lm = g_(v)[1], slot = g_(v)[3], kf = g_(v)[4];
    const int32_t nlm = lines ? A.nls : A.npt;
    int bad = 0;
    if (!(lm >= 0 && lm < nlm && slot >= 0 && slot < A.n_map && kf >= -1 && kf < A.nkf)) bad = BAD_COLUMN;
    else if (kf >= 0 && g_(A.kf_list)[kf] != slot) bad = BAD_KF_LOCAL;
    if (bad) {
        atomicOr(A.status, bad);
        lm = 0; kf = -1; slot = 0;                          // (in range: the host has refused observations without landmarks or slots)
    }
    g_(lines ? A.llm : A.plm)[o] = lm;
    g_(lines ? A.lkf : A.pkf)[o] = kf;
    g_(lines ? A.lslot : A.pslot)[o] = slot;                // (the inner LBA plan rewrites the points' slots: first_estimate_slot)
    g_(lines ? A.lkey : A.pkey)[o] = kf >= 0 ? lm : -1;     // the landmark lists leave out keyframes that are not optimised
}

// the lists as the pair kernels read them
struct GbpLists {
    const int32_t *lpp, *lpo, *plm, *pkf, *llp, *llo, *llm, *lkf;
    int32_t np, nl, npt, nls, nkf;
};

// K90: position i1 of a landmark's list starts the pairs (o1, o2), o2 over the landmark's whole list, with kf(o1) >= kf(o2)
// (gba_lists_build's add_pairs); cnt[t]: the points' positions, then the lines'
__global__ void __launch_bounds__(GBP_NT)
k_gbp_pair_count(const GbpLists L, int32_t* __restrict__ cnt, unsigned long long* __restrict__ total)
{
    const int64_t t = (int64_t)blockIdx.x * GBP_NT + threadIdx.x;
    int32_t c = 0;
    if (t < (int64_t)L.np + L.nl) {
        const bool lines = t >= L.np;
        const int32_t i1 = (int32_t)(lines ? t - L.np : t);
        const int32_t* __restrict__ ptr = lines ? L.llp : L.lpp;
        const int32_t* __restrict__ ids = lines ? L.llo : L.lpo;
        const int32_t* __restrict__ kf = lines ? L.lkf : L.pkf;
        const int32_t nobs = lines ? L.nl : L.np;
        const int32_t kept0 = g_(ptr)[lines ? L.nls : L.npt], kept = kept0 < nobs ? kept0 : nobs;
        if (i1 < kept) {
            const int32_t o1 = g_(ids)[i1];
            if ((uint32_t)o1 < (uint32_t)nobs) {            // (ids are item numbers: in range)
                const int32_t k1 = g_(kf)[o1], j = g_(lines ? L.llm : L.plm)[o1];       // (validated by K89)
                const int32_t e = g_(ptr)[j + 1] < kept ? g_(ptr)[j + 1] : kept;
                for (int32_t i2 = g_(ptr)[j] > 0 ? g_(ptr)[j] : 0; i2 < e; ++i2) {
                    const int32_t o2 = g_(ids)[i2];
                    c += (uint32_t)o2 < (uint32_t)nobs && g_(kf)[o2] <= k1 && g_(kf)[o2] >= 0 ? 1 : 0;
                }
                if (k1 < 0) c = 0;
            }
        }
        cnt[t] = c;
    }
    unsigned long long sum = (unsigned long long)c;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sum += (unsigned long long)__shfl_xor((long long)sum, o);
    if ((threadIdx.x & 63) == 0 && sum) atomicAdd(total, sum);
}

// K91: one lane; the last kernel in front of the first synchronisation
__global__ void __launch_bounds__(64)
k_gbp_publish(const int32_t* __restrict__ lpp, int32_t npt, const int32_t* __restrict__ llp, int32_t nls, const int32_t* __restrict__ kpp,
              const int32_t* __restrict__ klp, int32_t nkf, const int32_t* __restrict__ words, int32_t* __restrict__ pinned)
{
    if (threadIdx.x != 0) return;
    pinned[W_STATUS] = words[D_STATUS];
    pinned[W_LPO] = lpp[npt];
    pinned[W_LLO] = llp[nls];
    pinned[W_KPO] = kpp[nkf];
    pinned[W_KLO] = klp[nkf];
    pinned[W_PAIRS_LO] = words[D_PAIRS];
    pinned[W_PAIRS_HI] = words[D_PAIRS + 1];
}

// K92: the enumeration offset of every position (the exclusive sum of K90's counts: a look-back chain over tiles of GBP_NT
// positions), then the position's pairs in list order.  n_enum: the arrays' length.
__global__ void __launch_bounds__(GBP_NT)
k_gbp_pair_emit(const GbpLists L, const int32_t* __restrict__ cnt, uint32_t* __restrict__ part, int32_t n_enum,
                int32_t* __restrict__ key, int2* __restrict__ pair)
{
    __shared__ uint32_t s_w[GBP_NW], s_before;
    const int tid = (int)threadIdx.x, b = (int)blockIdx.x;
    const int64_t t = (int64_t)b * GBP_NT + tid;
    const bool in = t < (int64_t)L.np + L.nl;
    const uint32_t c = in ? (uint32_t)cnt[t] : 0u;
    uint32_t pos = lookback_offset<GBP_NW>(c, part, b, s_w, &s_before).pos;
    if (!in || c == 0) return;
    const bool lines = t >= L.np;
    const int32_t i1 = (int32_t)(lines ? t - L.np : t);
    const int32_t* __restrict__ ptr = lines ? L.llp : L.lpp;
    const int32_t* __restrict__ ids = lines ? L.llo : L.lpo;
    const int32_t* __restrict__ kf = lines ? L.lkf : L.pkf;
    const int32_t nobs = lines ? L.nl : L.np;
    const int32_t kept0 = g_(ptr)[lines ? L.nls : L.npt], kept = kept0 < nobs ? kept0 : nobs;
    const int32_t o1 = g_(ids)[i1], k1 = g_(kf)[o1];        // (c > 0: K90 found o1 in range and its keyframe optimised)
    const int32_t j = g_(lines ? L.llm : L.plm)[o1];
    const int32_t e = g_(ptr)[j + 1] < kept ? g_(ptr)[j + 1] : kept;
    for (int32_t i2 = g_(ptr)[j] > 0 ? g_(ptr)[j] : 0; i2 < e; ++i2) {
        const int32_t o2 = g_(ids)[i2];
        if ((uint32_t)o2 >= (uint32_t)nobs) continue;
        const int32_t k2 = g_(kf)[o2];
        if (k2 > k1 || k2 < 0) continue;
        if (pos < (uint32_t)n_enum) {
            key[pos] = 2 * (k1 * L.nkf + k2) + (lines ? 1 : 0);
            pair[pos] = make_int2(o1, o2);
        }
        ++pos;
    }
}

// the first position of the ascending keys[lo .. hi) whose value is at least x
__device__ __forceinline__ int32_t lower_bound_key(const int32_t* __restrict__ keys, int32_t lo, int32_t hi, int32_t x)
{
    while (lo < hi) {
        const int32_t mid = lo + ((hi - lo) >> 1);
        if (keys[mid] < x) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// K93: lanes 0 .. n_enum-1 are the sorted pairs -- a pair whose block differs from its predecessor's is its block's first -- and
// lanes n_enum .. n_enum+nkf-1 the diagonal keys k (nkf + 1) -- one that no pair carries is a block of its own (c0 == c1).
// Two stable compactions (two look-back chains): heads[r] = the position of the r-th first pair, diag[r] = the r-th such k.
__global__ void __launch_bounds__(GBP_NT)
k_gbp_heads(const int32_t* __restrict__ sorted, int32_t n_enum, int32_t nkf, uint32_t* __restrict__ part_h, uint32_t* __restrict__ part_d,
            int32_t* __restrict__ heads, int32_t* __restrict__ diag, int32_t* __restrict__ words)
{
    __shared__ uint32_t s_h[GBP_NW], s_d[GBP_NW], s_before_h, s_before_d;
    const int tid = (int)threadIdx.x, lane = tid & 63, wv = tid >> 6, b = (int)blockIdx.x;
    const int64_t t = (int64_t)b * GBP_NT + tid;
    bool fh = false, fd = false;
    if (t < n_enum) fh = t == 0 || (sorted[t] >> 1) != (sorted[t - 1] >> 1);
    else if (t < (int64_t)n_enum + nkf) {
        const int32_t bk = (int32_t)(t - n_enum) * (nkf + 1);
        const int32_t p = lower_bound_key(sorted, 0, n_enum, 2 * bk);
        fd = !(p < n_enum && (sorted[p] >> 1) == bk);
    }
    const uint64_t mh = __ballot(fh), md = __ballot(fd);
    if (lane == 0) { s_h[wv] = (uint32_t)__popcll(mh); s_d[wv] = (uint32_t)__popcll(md); }
    __syncthreads();                                        // (one barrier for the two chains)
    uint32_t in_h, own_h, in_d, own_d;
    waves_before_and_all<GBP_NW>(s_h, wv, in_h, own_h);
    waves_before_and_all<GBP_NW>(s_d, wv, in_d, own_d);
    const uint32_t before_h = lookback_exclusive(part_h, b, own_h, &s_before_h);
    const uint32_t before_d = lookback_exclusive(part_d, b, own_d, &s_before_d);
    const uint64_t below = (1ull << lane) - 1ull;
    if (fh) heads[before_h + in_h + (uint32_t)__popcll(mh & below)] = (int32_t)t;
    if (fd) diag[before_d + in_d + (uint32_t)__popcll(md & below)] = (int32_t)(t - n_enum);
    if (b == (int)gridDim.x - 1 && tid == 0) {
        words[D_NPH] = (int32_t)(before_h + own_h);
        words[D_NAD] = (int32_t)(before_d + own_d);
    }
}

struct GbpBlockInfo { int32_t key, p0, npp, nlp; };         // block key k1 nkf + k2, first pair, point pairs, line pairs

// K94: the blocks are the merge of the two compacted lists by block key (no key is in both).  A lane per entry of either list:
// its place is its rank in its own list plus the entries of the OTHER list in front of it (bisection).
__global__ void __launch_bounds__(GBP_NT)
k_gbp_block_info(const int32_t* __restrict__ sorted, int32_t n_enum, int32_t nkf, const int32_t* __restrict__ heads,
                 const int32_t* __restrict__ diag, const int32_t* __restrict__ words, int32_t nblk_cap, GbpBlockInfo* __restrict__ info)
{
    const int64_t t = (int64_t)blockIdx.x * GBP_NT + threadIdx.x;
    const int32_t nph = words[D_NPH], nad = words[D_NAD];
    if (t >= (int64_t)nph + nad) return;
    GbpBlockInfo B{};
    int32_t at;
    if (t < nph) {
        const int32_t r = (int32_t)t, p0 = heads[r], p1 = r + 1 < nph ? heads[r + 1] : n_enum;
        B.key = sorted[p0] >> 1;
        int32_t lo = 0, hi = nad;                           // the diagonal blocks without pairs in front of this key
        while (lo < hi) {
            const int32_t mid = lo + ((hi - lo) >> 1);
            if (diag[mid] * (nkf + 1) < B.key) lo = mid + 1;
            else hi = mid;
        }
        const int32_t split = lower_bound_key(sorted, p0, p1, 2 * B.key + 1);
        B.p0 = p0; B.npp = split - p0; B.nlp = p1 - split;
        at = r + lo;
    } else {
        const int32_t r = (int32_t)t - nph;
        B.key = diag[r] * (nkf + 1);
        int32_t lo = 0, hi = nph;                           // the blocks with pairs in front of this key
        while (lo < hi) {
            const int32_t mid = lo + ((hi - lo) >> 1);
            if ((sorted[heads[mid]] >> 1) < B.key) lo = mid + 1;
            else hi = mid;
        }
        B.p0 = lo < nph ? heads[lo] : n_enum;
        at = r + lo;
    }
    if (at >= 0 && at < nblk_cap) info[at] = B;            // (a merge of nph + nad entries: in range; checked all the same)
}

// K95: a lane per block in order: chunks of at most GBA_CHUNK pairs, the points' before the lines'; c0 = the exclusive sum
__global__ void __launch_bounds__(GBP_NT)
k_gbp_block_scan(const GbpBlockInfo* __restrict__ info, const int32_t* __restrict__ words, int32_t nkf, int32_t nblk_cap,
                 uint32_t* __restrict__ part, GbaBlock* __restrict__ blk, int32_t* __restrict__ c0, int32_t* __restrict__ pinned)
{
    __shared__ uint32_t s_w[GBP_NW], s_before;
    const int tid = (int)threadIdx.x, b = (int)blockIdx.x;
    const int64_t t = (int64_t)b * GBP_NT + tid;
    const int32_t nall = words[D_NPH] + words[D_NAD], nblk = nall < nblk_cap ? nall : nblk_cap;      // (a merge of distinct lower blocks: within the room)
    uint32_t c = 0;
    GbpBlockInfo B{};
    if (t < nblk) {
        B = info[t];
        c = (uint32_t)((B.npp + GBA_CHUNK - 1) / GBA_CHUNK + (B.nlp + GBA_CHUNK - 1) / GBA_CHUNK);
    }
    const TileScan sc = lookback_offset<GBP_NW>(c, part, b, s_w, &s_before);
    if (t < nblk) {
        blk[t] = GbaBlock{B.key / nkf, B.key % nkf, (int32_t)sc.pos, (int32_t)(sc.pos + c)};
        c0[t] = (int32_t)sc.pos;
    }
    if (b == (int)gridDim.x - 1 && tid == 0) {
        c0[nblk] = (int32_t)sc.upto;
        pinned[W_NBLK] = nblk;
        pinned[W_NCHUNK] = (int32_t)sc.upto;
    }
}

// K96: chunk c belongs to the block whose chunk range holds it (blocks without chunks share an offset with their successor: the
// last one at or below c is the owner); pair s of the compact list is the pair the distribution put at s
__global__ void __launch_bounds__(GBP_NT)
k_gbp_layout(const GbpBlockInfo* __restrict__ info, const int32_t* __restrict__ c0, int32_t nblk, int32_t nchunk,
             const int32_t* __restrict__ ids, const int2* __restrict__ src, int32_t n_enum, GbaChunk* __restrict__ chk, int2* __restrict__ pair)
{
    const int64_t t = (int64_t)blockIdx.x * GBP_NT + threadIdx.x;
    if (t < nchunk) {
        const int32_t c = (int32_t)t, B = segment_of(c0, nblk, c), r = c - c0[B];
        const GbpBlockInfo I = info[B];
        const int32_t ncp = (I.npp + GBA_CHUNK - 1) / GBA_CHUNK;
        GbaChunk q;
        q.blk = B;
        if (r < ncp) { q.line = 0; q.p0 = I.p0 + GBA_CHUNK * r; q.np = I.npp - GBA_CHUNK * r; }
        else { q.line = 1; q.p0 = I.p0 + I.npp + GBA_CHUNK * (r - ncp); q.np = I.nlp - GBA_CHUNK * (r - ncp); }
        q.np = q.np < GBA_CHUNK ? (q.np > 0 ? q.np : 0) : GBA_CHUNK;
        if (q.p0 < 0 || q.p0 + q.np > n_enum) { q.p0 = 0; q.np = 0; }      // (cannot happen: K29 never reads outside the pair list)
        chk[c] = q;
    } else if (t < (int64_t)nchunk + n_enum) {
        const int32_t s = (int32_t)(t - nchunk), e = ids[s];
        pair[s] = e >= 0 && e < n_enum ? src[e] : make_int2(0, 0);
    }
}

// the build's first scratch (aux): the device words, the columns that are not the plan's own, the distribution's buffers for the
// longer of the two observation lists, and -- kept for the emit -- the pair counts
struct ColScratch { int32_t *words, *pslot, *lslot, *pkey, *lkey, *pair_cnt; DistScratch dist; size_t bytes; };
ColScratch col_scratch(char* base, size_t np, size_t nl)
{
    ArrCarver c{base};
    ColScratch w{};
    const size_t cap = np > nl ? np : nl;
    w.words = c.take<int32_t>(D_WORDS * 4);
    w.pslot = c.take<int32_t>(np * 4); w.lslot = c.take<int32_t>(nl * 4);
    w.pkey = c.take<int32_t>(np * 4); w.lkey = c.take<int32_t>(nl * 4);
    w.dist.key_a = c.take<int32_t>(cap * 4); w.dist.key_b = c.take<int32_t>(cap * 4); w.dist.id_tmp = c.take<int32_t>(cap * 4);
    w.dist.table = c.take<uint32_t>((size_t)DIST_RADIX * (size_t)dist_tiles((int64_t)cap) * 4);
    w.pair_cnt = c.take<int32_t>((np + nl) * 4);
    w.bytes = c.size();
    return w;
}

// the second (aux_pairs): the look-back words of K92 / K93 (two chains) / K95 in ONE slice (cleared in one go), the emitted pairs
// and keys, the distribution's buffers, the compacted lists, the blocks
struct PairScratch {
    uint32_t *part_emit, *part_h, *part_d, *part_scan;
    int32_t* words;
    size_t zero_bytes;
    int2* pair;
    int32_t *key, *ids, *heads, *diag, *c0;
    GbpBlockInfo* info;
    GbaBlock* blk;
    DistScratch dist;
    size_t bytes;
};
PairScratch pair_scratch(char* base, size_t nobs, size_t n_enum, size_t nkf, size_t nblk_cap)
{
    ArrCarver c{base};
    PairScratch w{};
    w.part_emit = c.take<uint32_t>((size_t)wgs((int64_t)nobs, GBP_NT) * 4);
    w.part_h = c.take<uint32_t>((size_t)wgs((int64_t)(n_enum + nkf), GBP_NT) * 4);
    w.part_d = c.take<uint32_t>((size_t)wgs((int64_t)(n_enum + nkf), GBP_NT) * 4);
    w.part_scan = c.take<uint32_t>((size_t)wgs((int64_t)nblk_cap, GBP_NT) * 4);
    w.words = c.take<int32_t>(D_WORDS * 4);
    w.zero_bytes = c.size();
    w.pair = c.take<int2>(n_enum * sizeof(int2));
    w.key = c.take<int32_t>(n_enum * 4); w.ids = c.take<int32_t>(n_enum * 4);
    w.dist.key_a = c.take<int32_t>(n_enum * 4); w.dist.key_b = c.take<int32_t>(n_enum * 4); w.dist.id_tmp = c.take<int32_t>(n_enum * 4);
    w.dist.table = c.take<uint32_t>((size_t)DIST_RADIX * (size_t)dist_tiles((int64_t)n_enum) * 4);
    w.heads = c.take<int32_t>(nblk_cap * 4); w.diag = c.take<int32_t>(nkf * 4); w.c0 = c.take<int32_t>((nblk_cap + 1) * 4);
    w.info = c.take<GbpBlockInfo>(nblk_cap * sizeof(GbpBlockInfo));
    w.blk = c.take<GbaBlock>(nblk_cap * sizeof(GbaBlock));
    w.bytes = c.size();
    return w;
}

}  // namespace
}  // namespace plslam

extern "C" int plslam_gba_plan_create_dev(plslam_ctx* ctx, const plslam_cam* K, double homog_th, int32_t n_map_kf, int32_t nkf,
                                          const int32_t* d_kf_list, int32_t npt, int32_t nls, const int32_t* d_pt_obs,
                                          const double* d_pt_obs_uv, int32_t n_pt_obs, const int32_t* d_ls_obs, const double* d_ls_l_obs,
                                          int32_t n_ls_obs, plslam_gba_plan** out)
{
    int rc = gba_plan_args_ok(ctx, K, homog_th, n_map_kf, nkf, d_kf_list, npt, nls, d_pt_obs, d_pt_obs_uv, n_pt_obs, d_ls_obs, d_ls_l_obs,
                              n_ls_obs, out);
    if (rc) return rc;
    // (a kf_list entry, and an observation's landmark, cannot be in range where there is no slot or no landmark: what the host
    // builder refuses row by row is refused here before anything is launched)
    PLSLAM_REQUIRE(n_map_kf >= 1 && (n_pt_obs == 0 || npt > 0) && (n_ls_obs == 0 || nls > 0), PLSLAM_EINVAL);
    plslam_gba_plan* G = new (std::nothrow) plslam_gba_plan();
    PLSLAM_REQUIRE(G != nullptr, PLSLAM_ENOMEM);
    gba_plan_dims(G, ctx, n_map_kf, nkf, npt, nls, n_pt_obs, n_ls_obs);
    const size_t np = (size_t)n_pt_obs, nl = (size_t)n_ls_obs, nobs = np + nl;
    GbaListRoom room{np, nl, np, nl, 0, 0, 0};
    ColScratch w{};
    const int32_t* h = nullptr;
    int64_t n_enum = 0;
    {
        std::lock_guard<std::mutex> lk(ctx->mu);
        DeviceGuard dg_(ctx->device);
        hipStream_t s = ctx->stream;
        if ((rc = G->stat.reserve(gba_carve_stat(G, room, nullptr) + 256)) || (rc = G->aux.reserve(col_scratch(nullptr, np, nl).bytes + 256)) ||
            (rc = G->pin_cnt.reserve(W_WORDS * 4)))
            return gba_fail(G, rc);
        if (!G->pin_cnt.dev) return gba_fail(G, PLSLAM_ENOTSUP);   // the counts are written where the host reads them
        gba_carve_stat(G, room, G->stat.as<char>());
        w = col_scratch(G->aux.as<char>(), np, nl);
        const GbaStatView& S = G->st;
        G->kf_list.resize((size_t)nkf);
        auto build = [&]() -> int {
            PLSLAM_HIP_CHECK(hipMemsetAsync(w.words, 0, D_WORDS * 4, s));
            PLSLAM_HIP_CHECK(hipMemcpyAsync(G->kf_list.data(), d_kf_list, (size_t)nkf * 4, hipMemcpyDeviceToHost, s));   // (downloaded once)
            const GbpColumnArgs A{d_pt_obs, d_ls_obs, d_kf_list, S.plm, S.pkf, w.pslot, w.pkey, S.llm, S.lkf, w.lslot, w.lkey,
                                  w.words + D_STATUS, n_pt_obs, n_ls_obs, npt, nls, nkf, n_map_kf};
            hipLaunchKernelGGL(k_gbp_columns, dim3(wgs((int64_t)nobs + nkf, GBP_NT)), dim3(GBP_NT), 0, s, A);
            dist_enqueue(s, w.pkey, n_pt_obs, npt, S.lpo, S.lpp, w.dist);
            dist_enqueue(s, w.lkey, n_ls_obs, nls, S.llo, S.llp, w.dist);
            dist_enqueue(s, S.pkf, n_pt_obs, nkf, S.kpo, S.kpp, w.dist);
            dist_enqueue(s, S.lkf, n_ls_obs, nkf, S.klo, S.klp, w.dist);
            if (nobs) {
                const GbpLists L{S.lpp, S.lpo, S.plm, S.pkf, S.llp, S.llo, S.llm, S.lkf, n_pt_obs, n_ls_obs, npt, nls, nkf};
                hipLaunchKernelGGL(k_gbp_pair_count, dim3(wgs((int64_t)nobs, GBP_NT)), dim3(GBP_NT), 0, s, L, w.pair_cnt,
                                   reinterpret_cast<unsigned long long*>(w.words + D_PAIRS));
            }
            hipLaunchKernelGGL(k_gbp_publish, dim3(1), dim3(64), 0, s, (const int32_t*)S.lpp, npt, (const int32_t*)S.llp, nls,
                               (const int32_t*)S.kpp, (const int32_t*)S.klp, nkf, (const int32_t*)w.words, static_cast<int32_t*>(G->pin_cnt.dev));
            PLSLAM_HIP_CHECK(hipGetLastError());
            PLSLAM_HIP_CHECK(hipStreamSynchronize(s));      // the first synchronisation: status, list lengths, the pair total
            return PLSLAM_OK;
        };
        if ((rc = build())) return gba_fail(G, rc);
        h = G->pin_cnt.as<int32_t>();
        if (h[W_STATUS] != 0) {
            set_last_error("plslam_gba_plan_create_dev: %s", (h[W_STATUS] & BAD_KF_LIST) ? "kf_list names a slot out of range"
                                                             : (h[W_STATUS] & BAD_COLUMN) ? "a column out of range"
                                                                                          : "an observation's local keyframe is not its map keyframe");
            return gba_fail(G, PLSLAM_EINVAL);
        }
        if (h[W_LPO] < 0 || (size_t)h[W_LPO] > np || h[W_KPO] != h[W_LPO] || h[W_LLO] < 0 || (size_t)h[W_LLO] > nl || h[W_KLO] != h[W_LLO])
            return gba_fail(G, PLSLAM_EHIP);
        n_enum = (int64_t)(((uint64_t)(uint32_t)h[W_PAIRS_HI] << 32) | (uint32_t)h[W_PAIRS_LO]);
    }
    // (the pair list stays below 2^30 entries: the look-back's sums are 30-bit words.  The host builder's limit is INT32_MAX pairs,
    // PLSLAM_EINVAL; here PLSLAM_ERANGE at 2^30, as for the LBA plan's device-built lists -- refused before anything is emitted)
    if (n_enum < 0 || n_enum >= ((int64_t)1 << 30)) {
        set_last_error("plslam_gba_plan_create_dev: %lld observation pairs (at most 2^30 - 1)", (long long)n_enum);
        return gba_fail(G, PLSLAM_ERANGE);
    }
    // the inner LBA plan from the same columns: n_map_kf + nkf pose slots, the points of optimised keyframes read slot
    // n_map_kf + kf_loc (its own synchronisation; it takes the context's lock itself)
    rc = plslam_lba_plan_create_dev(ctx, K, homog_th, n_map_kf + nkf, nkf, npt, nls, G->st.plm, w.pslot, G->st.pkf, d_pt_obs_uv, n_pt_obs,
                                    G->st.llm, w.lslot, G->st.lkf, d_ls_l_obs, n_ls_obs, nullptr, nullptr, n_map_kf, &G->lba);
    if (rc) return gba_fail(G, rc);
    std::lock_guard<std::mutex> lk(ctx->mu);
    DeviceGuard dg_(ctx->device);
    hipStream_t s = ctx->stream;
    GbaStatView& S = G->st;
    S.lpo.bytes = (size_t)h[W_LPO] * 4; S.llo.bytes = (size_t)h[W_LLO] * 4; S.kpo.bytes = (size_t)h[W_KPO] * 4; S.klo.bytes = (size_t)h[W_KLO] * 4;
    const int64_t tri = (int64_t)nkf * (nkf + 1) / 2;
    const size_t nblk_cap = (size_t)(n_enum + nkf < tri ? n_enum + nkf : tri);
    if ((rc = G->aux_pairs.reserve(pair_scratch(nullptr, nobs, (size_t)n_enum, (size_t)nkf, nblk_cap).bytes + 256))) return gba_fail(G, rc);
    const PairScratch q = pair_scratch(G->aux_pairs.as<char>(), nobs, (size_t)n_enum, (size_t)nkf, nblk_cap);
    const int32_t* sorted = nullptr;
    auto blocks = [&]() -> int {
        PLSLAM_HIP_CHECK(hipMemsetAsync(q.part_emit, 0, q.zero_bytes, s));
        if (n_enum > 0) {
            const GbpLists L{S.lpp, S.lpo, S.plm, S.pkf, S.llp, S.llo, S.llm, S.lkf, n_pt_obs, n_ls_obs, npt, nls, nkf};
            hipLaunchKernelGGL(k_gbp_pair_emit, dim3(wgs((int64_t)nobs, GBP_NT)), dim3(GBP_NT), 0, s, L, (const int32_t*)w.pair_cnt, q.part_emit,
                               (int32_t)n_enum, q.key, q.pair);
        }
        sorted = dist_sort_enqueue(s, q.key, (int32_t)n_enum, 2 * nkf * nkf, q.ids, q.dist);
        hipLaunchKernelGGL(k_gbp_heads, dim3(wgs(n_enum + nkf, GBP_NT)), dim3(GBP_NT), 0, s, sorted, (int32_t)n_enum, nkf, q.part_h, q.part_d,
                           q.heads, q.diag, q.words);
        hipLaunchKernelGGL(k_gbp_block_info, dim3(wgs((int64_t)nblk_cap, GBP_NT)), dim3(GBP_NT), 0, s, sorted, (int32_t)n_enum, nkf,
                           (const int32_t*)q.heads, (const int32_t*)q.diag, (const int32_t*)q.words, (int32_t)nblk_cap, q.info);
        hipLaunchKernelGGL(k_gbp_block_scan, dim3(wgs((int64_t)nblk_cap, GBP_NT)), dim3(GBP_NT), 0, s, (const GbpBlockInfo*)q.info,
                           (const int32_t*)q.words, nkf, (int32_t)nblk_cap, q.part_scan, q.blk, q.c0, static_cast<int32_t*>(G->pin_cnt.dev));
        PLSLAM_HIP_CHECK(hipGetLastError());
        PLSLAM_HIP_CHECK(hipStreamSynchronize(s));          // the second synchronisation: the block and chunk totals
        return PLSLAM_OK;
    };
    if ((rc = blocks())) return gba_fail(G, rc);
    const int32_t nblk = h[W_NBLK], nchunk = h[W_NCHUNK];
    if (nblk < nkf || (size_t)nblk > nblk_cap || nchunk < 0 || (int64_t)nchunk > n_enum) return gba_fail(G, PLSLAM_EHIP);
    // chunk partials (36 doubles each) are indexed with int32: the host builder's limit and its code
    if ((int64_t)nchunk * 36 >= (int64_t)INT32_MAX) {
        set_last_error("plslam_gba_plan_create_dev: more chunks than int32 indexes");
        return gba_fail(G, PLSLAM_EINVAL);
    }
    G->nblk = nblk; G->nchunk = nchunk; G->npair = n_enum;
    room.nblk = (size_t)nblk; room.nchunk = (size_t)nchunk; room.npair = (size_t)n_enum;
    if ((rc = G->pairbuf.reserve(gba_carve_pairs(G, room, nullptr) + 256)) || (rc = G->work.reserve(gba_carve_work(G, nullptr) + 256)) ||
        (rc = G->Sbuf.reserve((size_t)G->npad * (size_t)G->npad * 8)))
        return gba_fail(G, rc);
    gba_carve_pairs(G, room, G->pairbuf.as<char>());
    gba_carve_work(G, G->work.as<char>());
    auto layout = [&]() -> int {
        PLSLAM_HIP_CHECK(hipMemcpyAsync(S.blk, q.blk, S.blk.bytes, hipMemcpyDeviceToDevice, s));
        if ((int64_t)nchunk + n_enum > 0)
            hipLaunchKernelGGL(k_gbp_layout, dim3(wgs((int64_t)nchunk + n_enum, GBP_NT)), dim3(GBP_NT), 0, s, (const GbpBlockInfo*)q.info,
                               (const int32_t*)q.c0, nblk, nchunk, (const int32_t*)q.ids, (const int2*)q.pair, (int32_t)n_enum, S.chk.p, S.pair.p);
        PLSLAM_HIP_CHECK(hipGetLastError());
        return PLSLAM_OK;
    };
    // (the scratch stays with the plan: the layout reads it behind this call, on the stream every later call of the plan uses)
    if ((rc = layout())) return gba_fail(G, rc);
    *out = G;
    return PLSLAM_OK;
}

extern "C" int plslam_gba_plan_list_sizes(plslam_gba_plan* G, plslam_gba_list_sizes* out)
{
    PLSLAM_REQUIRE(G && out, PLSLAM_EINVAL);
    const GbaStatView& S = G->st;
    out->nkf = G->nkf; out->npt = G->npt; out->nls = G->nls; out->n_pt_obs = G->np; out->n_ls_obs = G->nl;
    out->nblk = G->nblk; out->nchunk = G->nchunk; out->n_pairs = (int32_t)G->npair;
    out->n_lpo = (int32_t)(S.lpo.bytes / 4); out->n_llo = (int32_t)(S.llo.bytes / 4);
    out->n_kpo = (int32_t)(S.kpo.bytes / 4); out->n_klo = (int32_t)(S.klo.bytes / 4);
    return PLSLAM_OK;
}

extern "C" int plslam_gba_plan_lists(plslam_gba_plan* G, const plslam_gba_lists* host)
{
    PLSLAM_REQUIRE(G && host, PLSLAM_EINVAL);
    plslam_ctx* ctx = G->ctx;
    std::lock_guard<std::mutex> lk(ctx->mu);
    DeviceGuard dg_(ctx->device);
    const GbaStatView& S = G->st;
    const DownloadItem items[] = {
        {host->blk, S.blk, S.blk.bytes}, {host->chk, S.chk, S.chk.bytes}, {host->pair, S.pair, S.pair.bytes},
        {host->plm, S.plm, S.plm.bytes}, {host->pkf, S.pkf, S.pkf.bytes}, {host->llm, S.llm, S.llm.bytes}, {host->lkf, S.lkf, S.lkf.bytes},
        {host->kpp, S.kpp, S.kpp.bytes}, {host->kpo, S.kpo, S.kpo.bytes}, {host->klp, S.klp, S.klp.bytes}, {host->klo, S.klo, S.klo.bytes},
        {host->lpp, S.lpp, S.lpp.bytes}, {host->lpo, S.lpo, S.lpo.bytes}, {host->llp, S.llp, S.llp.bytes}, {host->llo, S.llo, S.llo.bytes}};
    return download_items(items, ctx->stream);
}
