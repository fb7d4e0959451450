// distribute_dev.hpp -- the stable distribution the device-built plans make their lists with (lba_plan_dev.hip: landmarks by
// lm_loc, the keyframe list by kf_loc, the Schur pairs by block; gba_plan_dev.hip: the four CSR lists, the covisible pairs by
// block and kind).  One copy: a change here moves every list that is built with it.
//
// Items 0 .. n-1 carry integer keys in [-1, nkeys).  The result is build_csr's inner by(...) (lba_lists.hpp): ids[ptr[k] .. ptr[k+1])
// are the items of key k IN THEIR ORIGINAL ORDER, items of key -1 are left out.  A key of -1 sorts as the value nkeys, behind
// every real key, so ptr[nkeys] is the number of items kept and whatever lies behind it in ids is not part of the list.
//
// Least-significant-digit passes over 8-bit digits, dist_passes(nkeys) of them; a pass is three launches:
//   hist     a workgroup per tile of DIST_TILE items: the tile's count of every digit -> table[digit][tile]
//   scan     ONE workgroup: the exclusive sum of the table in (digit, tile) order, in place -- where each tile's items of each
//            digit start in the pass's output
//   scatter  a workgroup per tile: every item to table[digit][tile] + its rank among the tile's EARLIER items of the same digit
// and dist_ptr_of() reads ptr off the sorted keys by bisection.  Nothing is exchanged between workgroups inside a launch: a pass's
// order comes from the ranks (ballots inside a wave, per-wave counts in LDS), never from the order in which atomics land; the
// only atomics are the histogram's LDS counts, whose sum is the same in any order.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "common.hpp"

namespace plslam {

constexpr int DIST_NT = 256;                          // lanes per workgroup of hist / scatter
constexpr int DIST_NW = DIST_NT / 64;
constexpr int DIST_ITEMS = 4;                         // items per lane
constexpr int DIST_TILE = DIST_NT * DIST_ITEMS;       // items per tile (plslam_amd/capi.py: LbaPlan.DIST_TILE)
constexpr int DIST_RADIX = 256;                       // 8-bit digits: one table row per lane of a workgroup
constexpr int DIST_SCAN_NT = 1024;                    // the scan's one workgroup

// passes that sort the values 0 .. nkeys (nkeys itself: the place of key -1)
inline int dist_passes(int32_t nkeys)
{
    int p = 1;
    while (p < 4 && ((uint32_t)nkeys >> (8 * p)) != 0) ++p;
    return p;
}
inline int32_t dist_tiles(int64_t n) { return (int32_t)((n + DIST_TILE - 1) / DIST_TILE); }

struct DistPass {
    const int32_t* key_in;     // n keys in [-1, nkeys)
    const int32_t* id_in;      // the items' ids so far; nullptr (the first pass): item i is id i
    int32_t *key_out, *id_out;
    uint32_t* table;           // DIST_RADIX x ntiles words
    int32_t n, ntiles, nkeys, shift;
};

// the distribution's scratch: two key buffers and an id buffer of `cap` items, the table for dist_tiles(cap) tiles
struct DistScratch { int32_t *key_a, *key_b, *id_tmp; uint32_t* table; };

// (distribute.hip: the kernels K75-K78 and their launches)
// ids_out[ptr_out[k] .. ptr_out[k + 1]): the items of key k in their order; ptr_out: nkeys + 1 words.  Enqueued on s.
void dist_enqueue(hipStream_t s, const int32_t* key_in, int32_t n, int32_t nkeys, int32_t* ids_out, int32_t* ptr_out, const DistScratch& w);
// The passes alone, for a caller that reads the segments off the sorted keys itself (no ptr over all nkeys keys): ids_out as
// above; returns where the n sorted keys lie -- key_in itself (n == 0) or one of the scratch's key buffers.
const int32_t* dist_sort_enqueue(hipStream_t s, const int32_t* key_in, int32_t n, int32_t nkeys, int32_t* ids_out, const DistScratch& w);

#if defined(__HIPCC__)

__device__ __forceinline__ uint32_t dist_value(int32_t key, int32_t nkeys) { return (uint32_t)(key < 0 ? nkeys : key); }
__device__ __forceinline__ uint32_t dist_digit(int32_t key, int32_t nkeys, int shift) { return (dist_value(key, nkeys) >> shift) & 255u; }

// hist: called by every thread of workgroup `tile` (DIST_NT lanes); s_cnt: DIST_RADIX words of LDS
__device__ __forceinline__ void dist_hist_tile(const DistPass& A, int tile, uint32_t* s_cnt)
{
    const int tid = (int)threadIdx.x;
    s_cnt[tid] = 0;
    __syncthreads();
#pragma unroll
    for (int j = 0; j < DIST_ITEMS; ++j) {
        const int64_t i = (int64_t)tile * DIST_TILE + j * DIST_NT + tid;
        if (i < A.n) atomicAdd(&s_cnt[dist_digit(g_(A.key_in)[i], A.nkeys, A.shift)], 1u);
    }
    __syncthreads();
    g_(A.table)[(size_t)tid * A.ntiles + tile] = s_cnt[tid];
}

// scan: called by every thread of the ONE workgroup (DIST_SCAN_NT lanes); s_w: DIST_SCAN_NT / 64 + 1 words of LDS.  The table's
// total is n < 2^31.
__device__ __forceinline__ void dist_scan_table(uint32_t* __restrict__ table, int64_t words, uint32_t* s_w)
{
    constexpr int NW = DIST_SCAN_NT / 64;
    const int tid = (int)threadIdx.x, lane = tid & 63, wv = tid >> 6;
    uint32_t carry = 0;
    for (int64_t base = 0; base < words; base += DIST_SCAN_NT) {
        const int64_t i = base + tid;
        const uint32_t v = i < words ? g_(table)[i] : 0u;
        uint32_t incl = v;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t t = (uint32_t)__shfl_up((int)incl, o);
            if (lane >= o) incl += t;
        }
        if (lane == 63) s_w[wv] = incl;
        __syncthreads();
        uint32_t before = 0, all = 0;
#pragma unroll
        for (int w = 0; w < NW; ++w) {
            const uint32_t c = s_w[w];
            before += w < wv ? c : 0u;
            all += c;
        }
        if (i < words) g_(table)[i] = carry + before + incl - v;
        carry += all;
        __syncthreads();                                    // (s_w is rewritten by the next round)
    }
}

// scatter: called by every thread of workgroup `tile` (DIST_NT lanes); s_cnt: DIST_NW x DIST_RADIX words, s_base: DIST_RADIX words.
// Item order inside the tile: wave, then round j, then lane -- ascending item index.
__device__ __forceinline__ void dist_scatter_tile(const DistPass& A, int tile, uint32_t (*s_cnt)[DIST_RADIX], uint32_t* s_base)
{
    const int tid = (int)threadIdx.x, lane = tid & 63, wv = tid >> 6;
#pragma unroll
    for (int w = 0; w < DIST_NW; ++w) s_cnt[w][tid] = 0;
    s_base[tid] = g_(A.table)[(size_t)tid * A.ntiles + tile];
    __syncthreads();
    int32_t key[DIST_ITEMS];
    uint32_t rank[DIST_ITEMS];
    const uint64_t below = (1ull << lane) - 1ull;
#pragma unroll
    for (int j = 0; j < DIST_ITEMS; ++j) {
        const int64_t i = (int64_t)tile * DIST_TILE + (wv * DIST_ITEMS + j) * 64 + lane;
        const bool live = i < A.n;
        key[j] = live ? g_(A.key_in)[i] : 0;
        const uint32_t d = dist_digit(key[j], A.nkeys, A.shift);
        uint64_t same = __ballot(live);                    // the live lanes of the wave with this lane's digit
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const bool bit = (d >> b) & 1u;
            const uint64_t m = __ballot(bit);
            same &= bit ? m : ~m;
        }
        const uint32_t prev = live ? s_cnt[wv][d] : 0u;    // the wave's earlier rounds
        rank[j] = prev + (uint32_t)__popcll(same & below);
        // (the digit's first lane counts the round in AFTER every lane has read: the LDS unit serves a wave's instructions in order;
        // the fences are for the compiler, they emit nothing)
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        if (live && (same & below) == 0) s_cnt[wv][d] = prev + (uint32_t)__popcll(same);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    }
    __syncthreads();
    {                                                       // per-wave counts -> the waves' offsets inside the tile
        uint32_t run = 0;
#pragma unroll
        for (int w = 0; w < DIST_NW; ++w) {
            const uint32_t c = s_cnt[w][tid];
            s_cnt[w][tid] = run;
            run += c;
        }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < DIST_ITEMS; ++j) {
        const int64_t i = (int64_t)tile * DIST_TILE + (wv * DIST_ITEMS + j) * 64 + lane;
        if (i >= A.n) continue;
        const uint32_t d = dist_digit(key[j], A.nkeys, A.shift);
        const uint32_t pos = s_base[d] + s_cnt[wv][d] + rank[j];
        if (pos >= (uint32_t)A.n) continue;                 // (cannot happen with a table of these keys: no store outside the arrays)
        g_(A.key_out)[pos] = key[j];
        g_(A.id_out)[pos] = A.id_in ? g_(A.id_in)[i] : (int32_t)i;
    }
}

// ptr[k], k in [0, nkeys]: the first position of the sorted keys whose value is at least k
__device__ __forceinline__ int32_t dist_ptr_of(const int32_t* __restrict__ sorted_key, int32_t n, int32_t nkeys, int32_t k)
{
    int32_t lo = 0, hi = n;                                 // the answer is in [lo, hi]
    while (lo < hi) {
        const int32_t mid = lo + ((hi - lo) >> 1);
        if (dist_value(g_(sorted_key)[mid], nkeys) < (uint32_t)k) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

#endif  // __HIPCC__

}  // namespace plslam
