// median_desc_dev.hpp -- one row of MapPoint::updateAverageDescDir's confusion matrix (src/mapFeatures.cpp:57-82), shared by K12
// (median_desc.hip: every landmark of a map) and K87 (map_lists.hip: the landmarks a carry touched).  One copy: the order
// statistic, the row-cache split and the key are written here once.
//
// Row i of conf of a landmark with n >= 2 observations: the distances d(i, j), j = 0 .. n - 1 (d(i, i) = 0).  The reference sorts
// the row and takes element k = int(1 + 0.5 (n - 1)); here the k-th order statistic is found by bisection on the value range
// [0, 256]: the smallest v with #{j : d(i, j) <= v} >= k + 1.  Lists of up to MEDIAN_ROW_CACHE observations keep the row in a
// lane-private LDS column (no barrier); longer ones recompute the distances per probe: 9 x n XOR + popcount distances per lane.
// The row's key (value << 23 | i) folded with an atomic minimum is "smallest value, then smallest i" in any execution order.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace plslam {

constexpr uint32_t MEDIAN_IDX_BITS = 23, MEDIAN_IDX_MASK = (1u << MEDIAN_IDX_BITS) - 1u;
constexpr int MEDIAN_ROW_CACHE = 16;      // lists up to this long keep their distance row in LDS
constexpr int MEDIAN_NT = 256;            // lanes per workgroup of the kernels that call median_row_key

// (not mfma_h_common.hpp's hamming256 of four vector registers: the builtin, so that the compiler selects the popcount for a
// row it reads from memory -- the asm form pins v_bcnt_u32_b32 and its operand order)
__device__ __forceinline__ int median_hamming256(const uint32_t (&q)[8], const uint32_t* __restrict__ t)
{
    int d = 0;
#pragma unroll
    for (int w = 0; w < 8; ++w) d += __popc(q[w] ^ t[w]);
    return d;
}

// The key of row i of the landmark whose n >= 2 descriptors start at row s of desc (8 words per row).  row_cache: the calling
// workgroup's MEDIAN_ROW_CACHE x MEDIAN_NT LDS block; the caller's lane owns column threadIdx.x.
__device__ __forceinline__ uint32_t median_row_key(const uint32_t* __restrict__ desc, int64_t s, int32_t n, int32_t i,
                                                   uint16_t (*row_cache)[MEDIAN_NT])
{
    const int32_t k = 1 + ((n - 1) >> 1);          // == int(1 + 0.5*(n-1)) for n >= 1
    uint32_t q[8];
#pragma unroll
    for (int w = 0; w < 8; ++w) q[w] = desc[(s + i) * 8 + w];
    const uint32_t* rows = desc + s * 8;
    // smallest v with #{j : d(i,j) <= v} >= k+1  ==  sorted(row)[k]
    int32_t vlo = 0, vhi = 256;
    if (n <= MEDIAN_ROW_CACHE) {
        // the usual case: the row of conf lives in this lane's LDS column (lane-private, no barrier)
        for (int32_t j = 0; j < n; ++j) row_cache[j][threadIdx.x] = (uint16_t)median_hamming256(q, rows + (int64_t)j * 8);
        while (vlo < vhi) {
            const int32_t mid = (vlo + vhi) >> 1;
            int32_t cnt = 0;
            for (int32_t j = 0; j < n; ++j) cnt += (int32_t)row_cache[j][threadIdx.x] <= mid;
            if (cnt >= k + 1) vhi = mid; else vlo = mid + 1;
        }
    } else {
        // long lists: recompute the distances per probe instead of storing n of them
        while (vlo < vhi) {
            const int32_t mid = (vlo + vhi) >> 1;
            int32_t cnt = 0;
            for (int32_t j = 0; j < n; ++j) cnt += median_hamming256(q, rows + (int64_t)j * 8) <= mid;
            if (cnt >= k + 1) vhi = mid; else vlo = mid + 1;
        }
    }
    return ((uint32_t)vlo << MEDIAN_IDX_BITS) | (uint32_t)i;
}

}  // namespace plslam
