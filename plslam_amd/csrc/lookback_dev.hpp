// lookback_dev.hpp -- the decoupled look-back the stable compactions and offset scans share, the tile scan that stands in front of
// it, and the bisection that finds an item's segment in the offsets such a scan leaves.  Its users: map2kf_kernels.hip k_visible_compact;
// local_map.hip K59 (the keyframe list), K60 (the landmark lists and their observation offsets); map_insert.hip K63 (events, new
// landmarks, pairs), K64 (the new obs_ptr); lc_fuse.hip K70 (the new obs_ptr); lba_plan_dev.hip K81 (the pair enumeration; K82
// uses the tile scan alone).  One copy: a change here moves every list that is built with it.
//
// A launch's workgroups chain their counts through part[b], one word per workgroup, ZERO when the kernel starts: bit 30 = "my own
// count is here", bit 31 = "the count of everything up to and including me is here", the low 30 bits the count (sums stay below
// 2^30).  A workgroup publishes its own count at once; its first wave then looks back 64 predecessors at a time -- the nearest
// one that already knows its inclusive sum ends the walk, the ones in between contribute their own counts -- and publishes its
// inclusive sum.  Normally one or two loads per lane.  It waits only for workgroups dispatched before it (a word without either
// bit), which were started earlier: the chain cannot wait on itself.  The values travel IN the words (relaxed agent-scope atomics):
// nothing else is exchanged between workgroups, so no fence is needed.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace plslam {

constexpr uint32_t LB_INCL = 0x80000000u, LB_AGG = 0x40000000u, LB_VAL = 0x3FFFFFFFu;

// Called by EVERY thread of workgroup b (at least one full wave; it holds two barriers' worth of synchronisation: the second one
// inside).  own: the workgroup's count (the same value in every thread); s_before: one LDS word of the caller, a word of its own per call
// (a kernel that chains two counts: the fast wave of the second call must not overwrite what a slow wave still reads).  Returns the sum of
// the counts of workgroups 0 .. b-1 to every thread.
__device__ __forceinline__ uint32_t lookback_exclusive(uint32_t* __restrict__ part, int b, uint32_t own, uint32_t* s_before)
{
    const int tid = (int)threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (tid == 0) __hip_atomic_store(part + b, own | (b == 0 ? LB_INCL : LB_AGG), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (wv == 0) {
        uint32_t before = 0;                                // the count in front of this workgroup
        for (int base = b - 1; base >= 0; base -= 64) {
            const int p = base - lane;                      // lane 0 looks at the nearest predecessor
            uint32_t x = LB_INCL;                           // (in front of workgroup 0: an inclusive sum of nothing)
            if (p >= 0)
                while (!((x = __hip_atomic_load(part + p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) & (LB_INCL | LB_AGG))) __builtin_amdgcn_s_sleep(1);
            const uint64_t incl = __ballot((x & LB_INCL) != 0);
            const int first = incl ? (int)__builtin_ctzll(incl) : 64;        // the nearest predecessor that knows its inclusive sum
            uint32_t t = lane <= first ? (x & LB_VAL) : 0u;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) t += (uint32_t)__shfl_xor((int)t, o);
            before += t;
            if (incl) break;
        }
        if (lane == 0) {
            *s_before = before;
            if (b > 0) __hip_atomic_store(part + b, (before + own) | LB_INCL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    __syncthreads();
    return *s_before;
}

// ---- the tile scan in front of the look-back ----
// A workgroup of NW waves is one tile.  Every chain of a kernel goes: a value per lane -> wave_inclusive_sum or a ballot -> the wave's
// total into the chain's NW LDS words -> ONE __syncthreads for all chains of the kernel -> waves_before_and_all -> lookback_exclusive.

// the sum of c over the lanes of this wave up to and including the caller's
__device__ __forceinline__ uint32_t wave_inclusive_sum(uint32_t c)
{
    const int lane = (int)threadIdx.x & 63;
    uint32_t incl = c;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t t = (uint32_t)__shfl_up((int)incl, o);
        if (lane >= o) incl += t;
    }
    return incl;
}
// from the waves' totals s_w[NW] (written in front of the caller's barrier): in = the total of the waves in front of wave wv,
// all = of every wave
template <int NW>
__device__ __forceinline__ void waves_before_and_all(const uint32_t* s_w, int wv, uint32_t& in, uint32_t& all)
{
    in = all = 0;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
        in += w < wv ? s_w[w] : 0u;
        all += s_w[w];
    }
}

// The kernels with ONE chain.  Called by EVERY thread of workgroup b (NW full waves; two barriers: one here, one in the look-back);
// s_w: NW LDS words, s_before: one more.  pos: the lane's place in the launch-wide list; tile: the workgroup's total; upto: the
// total of workgroups 0 .. b -- in the last workgroup, of the launch.
struct TileScan { uint32_t pos, tile, upto; };
// a stable compaction: the rank of a lane with `flag` among all lanes with it (pos means nothing for a lane without)
template <int NW>
__device__ __forceinline__ TileScan lookback_rank(bool flag, uint32_t* __restrict__ part, int b, uint32_t* s_w, uint32_t* s_before)
{
    const int lane = (int)threadIdx.x & 63, wv = (int)threadIdx.x >> 6;
    const uint64_t m = __ballot(flag);
    if (lane == 0) s_w[wv] = (uint32_t)__popcll(m);
    __syncthreads();
    uint32_t in, all;
    waves_before_and_all<NW>(s_w, wv, in, all);
    const uint32_t before = lookback_exclusive(part, b, all, s_before);
    return TileScan{before + in + (uint32_t)__popcll(m & ((1ull << lane) - 1ull)), all, before + all};
}
// an exclusive sum: the total of `count` over all lanes in front of the caller
template <int NW>
__device__ __forceinline__ TileScan lookback_offset(uint32_t count, uint32_t* __restrict__ part, int b, uint32_t* s_w, uint32_t* s_before)
{
    const int lane = (int)threadIdx.x & 63, wv = (int)threadIdx.x >> 6;
    const uint32_t incl = wave_inclusive_sum(count);
    if (lane == 63) s_w[wv] = incl;
    __syncthreads();
    uint32_t in, all;
    waves_before_and_all<NW>(s_w, wv, in, all);
    const uint32_t before = lookback_exclusive(part, b, all, s_before);
    return TileScan{before + in + incl - count, all, before + all};
}

// the largest k in [0, n) with ptr[k] <= x (ptr ascending, ptr[0] <= x): the segment an item of a CSR list belongs to
__device__ __forceinline__ int segment_of(const int32_t* __restrict__ ptr, int n, int32_t x)
{
    int lo = 0, hi = n;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (ptr[mid] <= x) lo = mid;
        else hi = mid;
    }
    return lo;
}

}  // namespace plslam
