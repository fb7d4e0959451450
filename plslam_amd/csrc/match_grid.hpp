// match_grid.hpp -- StVO::matchGrid, the windowed matcher (K14): what the other translation units see of it, and below the
// divider what its own files (match_grid.hip, match_grid_listers.hip, match_grid_dense.hip, match_grid_api.hip) share.
#pragma once

#include "common.hpp"
#include "match_grid_layout.hpp"   // grid_scratch_words, grid_store_capacity_bound, ...: the sizes a caller provides

namespace plslam {

struct GridDesc {              // one matchGrid problem; every pointer is a device pointer
    const uint8_t* d1;         // n1 x 32
    const uint8_t* d2;         // n2 x 32
    const int32_t* centres;    // n1 x n_centres x 2 window centres (x, y)
    const int32_t* cell_start; // cols*rows + 1   GridStructure in CSR form, cell id = x*rows + y
    const int32_t* cell_items;
    const double* dir1;        // n1 x 2 or nullptr (points)
    const double* dir2;        // n2 x 2 or nullptr
    int32_t* matches_12;       // n1
    int32_t* n_matches;        // 1 or nullptr
    uint32_t* scratch;         // grid_scratch_words() words: [tables when they do not fit LDS |] pair list
    int32_t* status;           // incremented when the pair list does not fit pair_cap; may be nullptr
    double sim_th, nnr;
    int32_t n1, n2, n_centres, cols, rows, mutual;
    int32_t w[4];              // width.first, width.second, height.first, height.second
    int32_t pair_cap;
    int32_t n_items;           // entries of cell_items the caller declared (cell_start[cols*rows] must not exceed it)
};
extern int g_grid_dense;       // ctx option "grid_dense" (process-wide): 1 = a small lone problem runs on k_match_grid_dense
// the dense one-workgroup kernel takes the problem (when it is alone and the host has its descriptor)
bool grid_dense_ok(int32_t n1, int32_t n2, int64_t ncell, int32_t n_items, bool dirs, int32_t n_centres);
// the device words the two launches of a large lone problem share, prefilled by grid_aux_fill in the caller's upload image
size_t grid_aux_words(int32_t n2);
void grid_aux_fill(void* host_image, int32_t n2);
// one problem with DEVICE pointers on `s` (scratch: grid_scratch_words() words; status: one zeroed int32 or nullptr), in two
// steps -- the descriptor travels inside a larger upload of the caller: host-side check + fill, then the launch
int grid_prepare_one(const plslam_grid_problem& q, uint32_t* scratch, int32_t* status, GridDesc* h_desc_slot);
int grid_launch_single(const plslam_grid_problem& q, const GridDesc* d_desc, hipStream_t s, uint32_t* aux, bool n1_upper_bound,
                       const GridDesc* h_desc);

// ---- the matcher's own files only ------------------------------------------------------------------------------------------
// match_grid.hip.  Table order: the n[3] problems of group 3, then n[2], n[1], n[0] (grid_group)
int launch_match_grid(const GridDesc* d_probs, const int32_t n[4], const size_t lds_bytes[4], hipStream_t s);
int launch_match_grid_listed(const GridDesc* d_desc, size_t lds_bytes, hipStream_t s, const uint32_t* pre, uint32_t pre_slots,
                             const GridDesc* h_desc, const int32_t* n1_dev);
// match_grid_listers.hip
int launch_grid_candidates(const GridDesc* d_desc, uint32_t* aux, int split, unsigned workgroups, hipStream_t s);
int launch_grid_records(const GridDesc& h_desc, uint32_t* aux, const int32_t* n1_dev, unsigned n_groups, hipStream_t s);
// match_grid_dense.hip
int launch_match_grid_dense(const GridDesc& h_desc, hipStream_t s);

}  // namespace plslam
