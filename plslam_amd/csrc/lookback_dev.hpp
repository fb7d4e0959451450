// lookback_dev.hpp -- the decoupled look-back the stable compactions share (lba.hip: k_visible_compact; local_map.hip: the
// local-map lists and the observation offsets; map_insert.hip: the event list and the new obs_ptr), and the bisection that finds
// an item's segment in the offsets such a scan leaves.  One copy: a change here moves every list that is built with it.
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
