// match_kernels.hpp -- how the matcher's kernels are launched: the scans (hamming.hip, hamming_mfma*.hip) and the stages behind
// a scan (match_post.hip), with the table-shape functions the planner's options are filled from and the column layout K1h /
// K1i share with their merge.  Seen by the scan sources (through mfma_h_common.hpp), match_post.hip, match_plan.hip,
// context.hip and host_calls.hip -- not by the rest of the library.  Every launch is asynchronous on `s`.  Internal.
#pragma once

#include "common.hpp"

namespace plslam {

// ---- K1h / K1i: the layout of b over (tile, class): class-major inside groups of 16 tiles of 32 rows ---------------------
// full groups: 512 rows each; the ragged rest (n2 mod 512 rows) is one more group of S = ceil(rest / 32) tiles with S rows per
// class.  Column slot of the partial table = 32 tile + class.
struct MhLayout {
    int n2, nfull, ntiles, rag_s;       // nfull: tiles of full groups (a multiple of 16); rag_s: tiles (= rows per class) of the ragged group
    __host__ __device__ explicit MhLayout(int n2_) : n2(n2_)
    {
        const int full = n2_ / 512, rest = n2_ - full * 512;
        nfull = full * 16;
        rag_s = (rest + 31) / 32;
        ntiles = nfull + rag_s;
    }
    __host__ __device__ int stride(int t) const { return t < nfull ? 16 : rag_s; }
    __host__ __device__ int row_of(int t, int cls) const { return (t >> 4) * 512 + stride(t) * cls + (t & 15); }   // may be >= n2
    __host__ __device__ int slot_of(int j) const
    {
        const int G = j >> 9, off = j & 511;
        const int s = G * 16 < nfull ? 16 : rag_s;
        // off / s for off < 512, 1 <= s <= 16 without a division: floor(off * ceil(2^16 / s) / 2^16), exact while off < 2^16 / s
        constexpr uint32_t recip[17] = {0, 65536, 32768, 21846, 16384, 13108, 10923, 9363, 8192, 7282, 6554, 5958, 5462, 5042,
                                        4682, 4370, 4096};
        const int cls = (int)(((uint32_t)off * recip[s]) >> 16), tt = off - cls * s;
        return 32 * (G * 16 + tt) + cls;
    }
    __host__ __device__ int slots_padded() const { return (32 * ntiles + 255) & ~255; }     // slots per row of the partial table
};

// ---- the scans -----------------------------------------------------------------------------------------------------------
// the popcount forms (hamming.hip).  K1a / K1d: directed scans; scan_rows_per_block() = query rows covered by one BlockDesc
int scan_rows_per_block(int variant, int block_threads);
int launch_scan(const plslam_ctx* ctx, int variant, int block_threads, const ScanDesc* d_scans,
                const BlockDesc* d_blocks, int nblocks, int32_t* d_zero, int nzero, hipStream_t s);
// rows_per_lane: 1 (K1b: 256-thread workgroups, 64 a-rows per wave) or 4 (K1b': 64-thread
// workgroups, 256 a-rows per wave).  sym_rows_per_block() = a-rows covered by one BlockDesc.
int sym_rows_per_block(int rows_per_lane);
int sym_rows_per_partial(int rows_per_lane);
int launch_scan_sym(int rows_per_lane, const SymDesc* d_sym, const BlockDesc* d_blocks, int nblocks,
                    int32_t* d_zero, int nzero, hipStream_t s);
// K1e: the symmetric scan on the matrix cores (hamming_mfma.hip); block tables / partials as for
// launch_scan_sym(rows_per_lane = 4): 256 a-rows per workgroup and per column partial
// multi_window: some problem of the launch has n2 > 2048 (row keys hold 64 tiles of 32 columns per window)
// directed: only keys12 of every SymDesc is produced (keys21 / part21 unused): non-mutual problems, knnMatch
int launch_scan_sym_mfma(const SymDesc* d_sym, const BlockDesc* d_blocks, int nblocks, int32_t* d_zero,
                         int nzero, bool multi_window, bool directed, hipStream_t s);
// K1f (hamming_mfma_g.hip): same contract and tables as K1e; row direction = group minima + second best by recomputation
// fused: one block-table entry per PROBLEM (row0 = 0); the workgroup walks the problem's row blocks itself, then merges the
// column partials and applies the ratio test + mutual check (SymDesc::matches_12 / n_matches / nnr / mutual): no merge
// kernel, no finalize kernel, no counter zeroing for these problems.  Mutual problems need n2 <= PLSLAM_K1F_FUSED_MAX_N2.
// (Column split of a large problem: the columns are cut into ranges scanned as sub-problems of their own -- more
// workgroups than 256-row blocks alone give; the per-range row results are merged by the finalize kernel: ProblemDesc.)
int launch_scan_sym_mfma_g(const SymDesc* d_sym, const BlockDesc* d_blocks, int nblocks, int32_t* d_zero,
                           int nzero, bool multi_window, bool directed, bool fused, hipStream_t s);
// K1g (hamming_mfma_d.hip): the directed scan, one item per (directed scan, 256-row block of a); any n2 (windows inside)
int launch_scan_dir_mfma(const SymDesc* d_sym, const BlockDesc* d_blocks, int nblocks, int32_t* d_zero, int nzero, hipStream_t s);
// K1h (hamming_mfma_h.hip): K1f's contract and partial table; minimum-only bookkeeping in both directions, class-major layouts;
// its partials need launch_merge_fix16 (merge + second-best recomputation), same block table as launch_merge_partials16
int launch_scan_sym_mfma_h(const SymDesc* d_sym, const BlockDesc* d_blocks, int nblocks, int32_t* d_zero, int nzero,
                           bool directed, hipStream_t s);
// K1i (hamming_mfma_i.hip): K1h with the two M-tiles of a wave pipelined against each other; same tables, same merge kernel
int launch_scan_sym_mfma_i(const SymDesc* d_sym, const BlockDesc* d_blocks, int nblocks, int32_t* d_zero, int nzero,
                           bool directed, hipStream_t s);
// the matrix-core scan of `form` (context.hip: the one place that knows which generations the build carries)
int launch_scan_mfma_form(int form, const SymDesc* d_sym, const BlockDesc* d_blocks, int nblocks, int32_t* d_zero,
                          int nzero, bool multi_window, bool directed, hipStream_t s, bool fused = false);

// ---- the stages behind a scan (match_post.hip), in the order plan_run chooses among them ---------------------------------
// K1c'' + K2 behind a column-split K1f scan in one kernel (two-launch plan runs); the dump's row completion.
// parts: lanes sharing one column (1, 4 or 16); d_blocks: the merge kernel's table (launch_merge_partials16)
int launch_split_post(const SymDesc* d_sym, const BlockDesc* d_blocks, int nblocks, int parts, const ProblemDesc* d_probs, hipStream_t s);
int launch_split_rows_dump(const ProblemDesc* d_probs, const BlockDesc* d_fin_blocks, int nblocks, hipStream_t s);
// K2': merge of K1h's / K1i's column partials + finalize + gates, one workgroup per problem; lds_bytes = 8 x the
// largest n2 of the plan (POST_FUSED_MAX_*: match_tables.hpp)
int launch_post_fused(const ProblemDesc* d_probs, int nprob, const plslam_stereo_gate_problem* d_gates, size_t lds_bytes,
                      hipStream_t s);
// the column merges, one per table family.  K1h / K1i: the block table has one entry per merge_fix16_cols(parts) column slots;
// K1f: one per merge_partials16_cols(parts) columns; K1b / K1b' / K1e: one per 256 columns
int merge_fix16_cols(int parts);
int launch_merge_fix16(const SymDesc* d_sym, const BlockDesc* d_blocks, int nblocks, int parts, bool fix, hipStream_t s, int grid_cap = 0);
int merge_partials16_cols(int parts);
int launch_merge_partials16(const SymDesc* d_sym, const BlockDesc* d_blocks, int nblocks, int parts, hipStream_t s);
int launch_merge_partials(const SymDesc* d_sym, const BlockDesc* d_blocks, int nblocks, hipStream_t s);
// K2: ratio test + mutual check (+ the stereo gate of the row just decided) behind any merge
int launch_finalize(const ProblemDesc* d_probs, const BlockDesc* d_blocks, int nblocks,
                    const plslam_stereo_gate_problem* d_gates, hipStream_t s, int grid_cap = 0, bool xcd_chunks = false, int dealt_row = 0);
int launch_scatter_counts(const int32_t* d_src, int32_t* const* d_dst, int32_t n, hipStream_t s);
int launch_unpack_keys(const uint32_t* d_keys, int32_t n, int32_t* d_idx, int32_t* d_dist,
                       hipStream_t s);

}  // namespace plslam
