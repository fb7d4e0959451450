// distribute.hip -- the kernels of the stable distribution (distribute_dev.hpp) and the host code that enqueues them: ONE copy for
// every list that is built with it (lba_plan_dev.hip: the LBA plan's lists and its Schur pairs; gba_plan_dev.hip: the GBA plan's
// four CSR lists and its covisible pairs).
//   K75 k_dist_hist / K76 k_dist_scan / K77 k_dist_scatter   a pass over one 8-bit digit
//   K78 k_dist_ptr                                           ptr off the sorted keys, by bisection
#include "distribute_dev.hpp"

namespace plslam {
namespace {

constexpr int DIST_PTR_NT = 256;

__global__ void __launch_bounds__(DIST_NT)
k_dist_hist(const DistPass A)
{
    __shared__ uint32_t s_cnt[DIST_RADIX];
    dist_hist_tile(A, (int)blockIdx.x, s_cnt);
}

__global__ void __launch_bounds__(DIST_SCAN_NT)
k_dist_scan(uint32_t* __restrict__ table, int64_t words)
{
    __shared__ uint32_t s_w[DIST_SCAN_NT / 64 + 1];
    dist_scan_table(table, words, s_w);
}

__global__ void __launch_bounds__(DIST_NT)
k_dist_scatter(const DistPass A)
{
    __shared__ uint32_t s_cnt[DIST_NW][DIST_RADIX], s_base[DIST_RADIX];
    dist_scatter_tile(A, (int)blockIdx.x, s_cnt, s_base);
}

__global__ void __launch_bounds__(DIST_PTR_NT)
k_dist_ptr(const int32_t* __restrict__ sorted_key, int32_t n, int32_t nkeys, int32_t* __restrict__ ptr)
{
    const int64_t k = (int64_t)blockIdx.x * DIST_PTR_NT + threadIdx.x;
    if (k <= nkeys) ptr[k] = dist_ptr_of(sorted_key, n, nkeys, (int32_t)k);
}

}  // namespace

const int32_t* dist_sort_enqueue(hipStream_t s, const int32_t* key_in, int32_t n, int32_t nkeys, int32_t* ids_out, const DistScratch& w)
{
    const int passes = dist_passes(nkeys);
    const int32_t ntiles = dist_tiles(n);
    const int32_t* sorted = key_in;
    if (n > 0) {
        const int32_t* ids_in = nullptr;
        for (int p = 0; p < passes; ++p) {
            DistPass A{};
            A.key_in = sorted; A.id_in = ids_in;
            A.key_out = (p & 1) ? w.key_b : w.key_a;
            A.id_out = ((passes - 1 - p) & 1) ? w.id_tmp : ids_out;        // the last pass writes the list itself
            A.table = w.table; A.n = n; A.ntiles = ntiles; A.nkeys = nkeys; A.shift = 8 * p;
            hipLaunchKernelGGL(k_dist_hist, dim3(ntiles), dim3(DIST_NT), 0, s, A);
            hipLaunchKernelGGL(k_dist_scan, dim3(1), dim3(DIST_SCAN_NT), 0, s, w.table, (int64_t)DIST_RADIX * ntiles);
            hipLaunchKernelGGL(k_dist_scatter, dim3(ntiles), dim3(DIST_NT), 0, s, A);
            sorted = A.key_out; ids_in = A.id_out;
        }
    }
    return sorted;
}

void dist_enqueue(hipStream_t s, const int32_t* key_in, int32_t n, int32_t nkeys, int32_t* ids_out, int32_t* ptr_out, const DistScratch& w)
{
    const int32_t* sorted = dist_sort_enqueue(s, key_in, n, nkeys, ids_out, w);
    hipLaunchKernelGGL(k_dist_ptr, dim3((unsigned)(((int64_t)nkeys + 1 + DIST_PTR_NT - 1) / DIST_PTR_NT)), dim3(DIST_PTR_NT), 0, s, sorted, n,
                       nkeys, ptr_out);
}

}  // namespace plslam
