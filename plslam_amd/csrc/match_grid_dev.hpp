// match_grid_dev.hpp -- what the device kernels of the windowed matcher (match_grid.hip, match_grid_listers.hip,
// match_grid_dense.hip) share: the address-space pointer types, the problem's tables as one struct, the walk over a
// row's window cells and the device-only constants.
#pragma once

#include "match_grid.hpp"

namespace plslam {

constexpr uint32_t REC_D_BITS = 9, REC_D_MASK = 511u;                  // column state: i1 << 9 | d
constexpr int CB = 4;                                                  // candidates per batch
constexpr uint32_t GRID_TAIL = 256;                                   // candidates left when one wave finishes the passes alone
constexpr int PB_BATCH = 8;                                            // stored candidates per batch of a record pass
constexpr uint32_t GRID_RUNS_PER_COLUMN = 4;                           // k_grid_records' list is bucketed by column while a column has at most this many runs on average

// Pointers read out of the problem table are generic to the compiler (it would emit FLAT instructions and, for the
// mode-dependent ones, could not tell LDS from global memory): every pointer below carries its address space.
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));   // a builtin vector (HIP's uint4 class cannot live behind an address space)
#define PLSLAM_AS_GLOBAL __attribute__((address_space(1)))
#define PLSLAM_AS_LDS __attribute__((address_space(3)))
template <class T, bool IN_LDS> struct as_ptr { using type = PLSLAM_AS_GLOBAL T*; };
template <class T> struct as_ptr<T, true> { using type = PLSLAM_AS_LDS T*; };

template <int MODE>   // 0: every table in global scratch; 1: cell_start + column / row words in LDS; 2: items and desc2 rows too
struct GridPtrs {
    typename as_ptr<const uint32_t, (MODE >= 1)>::type cs;      // cell_start
    typename as_ptr<const int32_t, (MODE == 2)>::type items;    // cell_items
    typename as_ptr<const u32x4, (MODE == 2)>::type d2;         // desc2 rows, 2 x 16 bytes
    typename as_ptr<uint32_t, (MODE >= 1)>::type state, next, row_k1, row_k2;
    PLSLAM_AS_GLOBAL const int32_t* centres;
    PLSLAM_AS_GLOBAL const double* dir1;
    typename as_ptr<const double, (MODE == 2)>::type dir2;      // directions of the desc2 lines
};

__device__ __forceinline__ void best2_fold(uint32_t& k1, uint32_t& k2, uint32_t key)
{   // idempotent insertion into the two smallest DISTINCT keys (k1 <= k2) -- which is why it is not merge2 / pk_push2 of
    // mfma_h_common.hpp, where a key met twice takes both places; value selects only -- a branchy form makes
    // the compiler address k1 / k2 through private memory
    const uint32_t lo = key < k1 ? key : k1, hi = key < k1 ? k1 : key;
    k2 = key == k1 ? k2 : (hi < k2 ? hi : k2);
    k1 = lo;
}

// Slot k of lane `tid` in the transposed candidate store of a round: row k of a [depth][NT] array, rotated by one
// wave per row -- a wave's successive slots then fall into different 256-byte channels of L2 / HBM instead of all
// into the same one (row pitch 4 KB = 16 channels x 256 B)
template <int NT>
__device__ __forceinline__ size_t slot_index(uint32_t k, int tid)
{
    return (size_t)k * NT + ((uint32_t)(tid + (k << 6)) & (uint32_t)(NT - 1));
}

struct RowWindows {     // GridStructure::get ranges of one window centre (clamped to the grid: they fit 32 bits)
    int32_t min_x, max_x, min_y, max_y;
};
__device__ __forceinline__ RowWindows window_of(const GridDesc& g, PLSLAM_AS_GLOBAL const int32_t* p)
{
    const int64_t x = p[0], y = p[1];
    RowWindows r;   // the sums in 64 bits: centres and windows may be any int32
    r.min_x = (int32_t)(x - g.w[0] > 0 ? (x - g.w[0] < g.cols ? x - g.w[0] : g.cols) : 0);
    r.max_x = (int32_t)(x + g.w[1] + 1 < g.cols ? (x + g.w[1] + 1 > 0 ? x + g.w[1] + 1 : 0) : g.cols);
    r.min_y = (int32_t)(y - g.w[2] > 0 ? (y - g.w[2] < g.rows ? y - g.w[2] : g.rows) : 0);
    r.max_y = (int32_t)(y + g.w[3] + 1 < g.rows ? (y + g.w[3] + 1 > 0 ? y + g.w[3] + 1 : 0) : g.rows);
    return r;
}

// number of grid items inside row i1's windows (duplicates, out-of-range items and candidates the direction test
// will drop included): the upper bound its slots in the candidate store are sized by
template <int MODE>
__device__ __forceinline__ uint32_t count_items(const GridDesc& g, const GridPtrs<MODE>& P, int32_t i1)
{
    uint32_t n = 0;
    for (int32_t c = 0; c < g.n_centres; ++c) {
        const RowWindows r = window_of(g, P.centres + ((int64_t)i1 * g.n_centres + c) * 2);
        if (r.min_y >= r.max_y) continue;
        for (int32_t x_ = r.min_x; x_ < r.max_x; ++x_) n += P.cs[x_ * g.rows + r.max_y] - P.cs[x_ * g.rows + r.min_y];
    }
    return n;
}

// GridStructure::get over every window centre of row i1, in batches: f(i2[CB]) with i2[j] = -1 for the slots
// that are empty or fail `if (i2 < 0 || i2 >= desc2.rows) continue;` / the direction test of the line overload
// (part, split): only the window columns min_x + part, + split, ... -- a row's window shared out over `split` lanes
template <int MODE, class F>
__device__ __forceinline__ void for_candidates(const GridDesc& g, const GridPtrs<MODE>& P, int32_t i1, F&& f, int32_t part = 0,
                                               int32_t split = 1)
{
    double a0 = 0.0, a1 = 0.0;
    const bool dirs = g.dir1 != nullptr && g.dir2 != nullptr;
    if (dirs) {
        a0 = P.dir1[2 * (int64_t)i1];
        a1 = P.dir1[2 * (int64_t)i1 + 1];
    }
    for (int32_t c = 0; c < g.n_centres; ++c) {
        const RowWindows r = window_of(g, P.centres + ((int64_t)i1 * g.n_centres + c) * 2);
        if (r.min_y >= r.max_y) continue;
        for (int32_t x_ = r.min_x + part; x_ < r.max_x; x_ += split) {
            // cells (x_, min_y .. max_y-1) are adjacent in the CSR order (id = x*rows + y)
            const int32_t s = (int32_t)P.cs[x_ * g.rows + r.min_y], e = (int32_t)P.cs[x_ * g.rows + r.max_y];
            for (int32_t k = s; k < e; k += CB) {
                int32_t i2[CB];
#pragma unroll
                for (int j = 0; j < CB; ++j) {
                    i2[j] = k + j < e ? P.items[k + j] : -1;
                    if ((uint32_t)i2[j] >= (uint32_t)g.n2) i2[j] = -1;
                }
                if (dirs) {
                    double b0[CB], b1[CB];
#pragma unroll
                    for (int j = 0; j < CB; ++j) {
                        const int64_t t = i2[j] < 0 ? 0 : i2[j];
                        b0[j] = P.dir2[2 * t];
                        b1[j] = P.dir2[2 * t + 1];
                    }
#pragma unroll
                    for (int j = 0; j < CB; ++j) {
                        const double dot = a0 * b0[j] + a1 * b1[j];
                        if (fabs(dot) < g.sim_th) i2[j] = -1;     // NaN (zero-length direction) compares false: kept
                    }
                }
                f(i2);
            }
        }
    }
}

}  // namespace plslam
