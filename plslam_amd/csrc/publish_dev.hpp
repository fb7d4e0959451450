// publish_dev.hpp -- the counters of a call's LAST kernel (map2kf_kernels.hip: the gates of the map <-> keyframe drivers; local_map.hip: K57,
// K62, K84): every wave adds its ballot to a device word and WAITS for the atomic (a returning one) before the workgroup's barrier;
// one lane then counts the workgroup in, and the workgroup that finishes last copies the words to the page-locked block the host
// reads -- a launch less at the end of a call that is bound by its launches.  One copy: the memory order of this ticket (relaxed
// throughout) is decided here.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace plslam {

struct Publish { int32_t* done; const int32_t* src; int32_t* dst; int32_t n; };     // done: a ZERO device word

// a wave adds the number of its lanes with `ok` to *count and waits for the atomic
__device__ __forceinline__ void wave_count_and_wait(bool ok, int32_t* __restrict__ count)
{
    const unsigned long long b = __ballot(ok);
    if ((threadIdx.x & 63) == 0 && b) {
        const int old = atomicAdd(count, (int)__popcll(b));
        asm volatile("" ::"v"(old));                        // (the atomic has been performed when the wave passes here)
    }
}

// Called by EVERY thread of every workgroup, behind the waves' counts: the last workgroup to arrive copies pub.n words
__device__ __forceinline__ void publish_from_last_workgroup(const Publish& pub)
{
    __syncthreads();
    if (threadIdx.x == 0) {
        const int prev = atomicAdd(pub.done, 1);
        if (prev == (int)gridDim.x - 1)
            for (int w = 0; w < pub.n; ++w) pub.dst[w] = __hip_atomic_load(pub.src + w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

}  // namespace plslam
