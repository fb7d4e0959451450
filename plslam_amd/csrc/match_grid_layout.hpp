// match_grid_layout.hpp -- the arithmetic of the windowed matcher (K14, StVO::matchGrid): every sizing constant, the packed
// ("flat") candidate word's bit split, the layout of a problem's global scratch and of its LDS, the choice of mode and launch
// group, the capacity of the candidate store and the path a lone problem takes.  Pure arithmetic: no HIP header, no device, no
// context (tests/cpp/test_grid_layout.cpp compiles it with g++ alone).  What a kernel shares with the host is marked
// PLSLAM_GRID_HD and written in the kernels' own expression order, so that it inlines to the instructions they had before.
// The kernels are in match_grid.hip, match_grid_listers.hip and match_grid_dense.hip; the launches in match_grid_api.hip.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <algorithm>

#if defined(__HIPCC__)
#define PLSLAM_GRID_HD __host__ __device__ __forceinline__
#else
#define PLSLAM_GRID_HD inline
#endif

namespace plslam {

constexpr int GRID_THREADS = 1024;
constexpr size_t GRID_LDS_MAX_BYTES = 152 * 1024;                      // dynamic LDS of the LDS instantiations
constexpr size_t GRID_LDS_FIXED_MAX_BYTES = 144 * 1024;                // tables that MUST fit for MODE 1
constexpr int GRID_SMALL_ROWS = 256;       // problems of at most this many rows run on 256-lane workgroups (MODE 2 only)
constexpr int GRID_SPLIT = 4;              // flat PA: at most this many lanes share a row's window columns
constexpr int GRID_SPLIT_MAX = 16;         // k_grid_candidates: at most this many lanes per row (one per window column)
constexpr int GRID_SPLIT_MIN_ROWS = 128;   // one problem alone: from this many rows on PA runs as its own many-workgroup launch
constexpr uint32_t REC_SLOT = 8;                    // k_grid_records: list words per item of the grid
constexpr int REC_G = 8;                            // k_grid_records: cells per workgroup, same grid column x, consecutive y
constexpr int REC_ROWS_MAX = 16384;                 // rows of a problem that takes k_grid_records (the row lists of a group: 48 KB of LDS)
constexpr int64_t REC_GROUPS_MAX = 1 << 16;         // beyond this k_grid_candidates lists the pairs
constexpr int DENSE_MAX = 256, DENSE_NT = 1024, DENSE_CHUNK = 16;      // k_match_grid_dense: rows / columns at most, lanes, rows per chunk
constexpr size_t DENSE_LDS_MAX_BYTES = 128 * 1024;

// ---- the packed candidate word d << (fb1 + fb2) | i1 << fb2 | i2 ("flat" mode) ------------------------------------------------
// fb2 = bits of a column number (at least 1), fb1 = what is left of 23, at most 14: a column's record needs 9 bits for its pass
// number above i1 << 9 | d.  A problem is flat when it is mutual, n2 fits fb2 bits and n1 fits fb1 bits.  The bits of a column
// number exist in two forms: the loop stops at 22 (its users then test n2 against 1 << fb2), the clz form does not (its user
// tests fb2 <= 22); min(clz form, 22) == loop form for every n2, so the two tests agree (test_grid_layout.cpp: exhaustively).
PLSLAM_GRID_HD uint32_t grid_col_bits(uint32_t n2)
{
    uint32_t fb2 = 1;
    while (fb2 < 22 && (1u << fb2) < n2) ++fb2;
    return fb2;
}
PLSLAM_GRID_HD uint32_t grid_col_bits_clz(int32_t n2)
{
    return n2 > 1 ? 32u - (uint32_t)__builtin_clz((uint32_t)n2 - 1u) : 1u;
}
PLSLAM_GRID_HD uint32_t grid_row_bits(uint32_t fb2) { return 23u - fb2 > 14u ? 14u : 23u - fb2; }
// (the kernels restate this test on the bits they hold -- as a function it compiles to other instructions there --,
// k_grid_records with `fb2 <= 22u`, fb2 from the clz form, for `n2 <= 1 << fb2`)
PLSLAM_GRID_HD bool grid_flat(int mutual, int32_t n1, int32_t n2)
{
    const uint32_t fb2 = grid_col_bits((uint32_t)n2), fb1 = grid_row_bits(fb2);
    return mutual && (uint32_t)n2 <= (1u << fb2) && (uint32_t)n1 <= (1u << fb1);
}

// ---- LDS -----------------------------------------------------------------------------------------------------------------------
// words of the tables that live in LDS when they fit: state n2 | next n2 | row_k1 n1 | row_k2 n1 | cell_start copy ncell + 1
// (W: uint32_t in the kernel -- the launcher guarantees the fit --, size_t on the host)
template <class W>
PLSLAM_GRID_HD W grid_fixed_words_of(int32_t n1, int32_t n2, W ncell)
{
    return (ncell + 1) + 2 * (W)n2 + 2 * (W)n1;
}
inline size_t grid_fixed_words(int32_t n1, int32_t n2, int64_t ncell) { return grid_fixed_words_of<size_t>(n1, n2, (size_t)ncell); }
inline bool grid_fits_lds(int32_t n1, int32_t n2, int64_t ncell) { return grid_fixed_words(n1, n2, ncell) * 4 <= GRID_LDS_FIXED_MAX_BYTES; }

// MODE 2, word offsets: the column / row words first (what lies behind them is free once PA is done), the cell_start copy, the
// items at the next 16-byte boundary, the desc2 rows (2 x 16 bytes each) at the next, the directions of the desc2 lines when
// the problem has them (2 doubles each; 16-byte aligned: d2_off is), flat mode's best (d, row) seen per column while PA runs.
// (colbest and end as functions: the kernel asks for them where it knows `dirs`, and nowhere earlier)
template <class W>
struct GridLds2 {
    W cs, items_off, d2_off, dir2, n2;
    PLSLAM_GRID_HD W colbest(bool dirs) const { return d2_off + 8 * n2 + (dirs ? 4 * n2 : 0); }
    PLSLAM_GRID_HD W end(bool dirs) const { return colbest(dirs) + n2; }
};
template <class W>
PLSLAM_GRID_HD GridLds2<W> grid_lds2(int32_t n1, int32_t n2, W ncell, W n_items)
{
    GridLds2<W> l;
    const W fixed_words = grid_fixed_words_of<W>(n1, n2, ncell);
    l.n2 = (W)n2;
    l.cs = 2 * ((W)n2 + (W)n1);
    l.items_off = (fixed_words + 3) & ~(W)3;
    l.d2_off = (l.items_off + n_items + 3) & ~(W)3;
    l.dir2 = l.d2_off + 8 * (W)n2;
    return l;
}
// LDS bytes of a problem in each mode (0: every table in global scratch; 1: the tables; 2: items and desc2 rows too)
inline size_t grid_lds_bytes(int mode, int32_t n1, int32_t n2, int64_t ncell, int32_t n_items, bool dirs)
{
    if (mode == 0) return 0;
    if (mode == 2) return grid_lds2<size_t>(n1, n2, (size_t)ncell, (size_t)n_items).end(dirs) * 4;
    return grid_fixed_words(n1, n2, ncell) * 4;
}
inline int grid_mode(int32_t n1, int32_t n2, int64_t ncell, int32_t n_items, bool dirs)
{
    if (grid_lds_bytes(2, n1, n2, ncell, n_items, dirs) <= GRID_LDS_MAX_BYTES) return 2;
    return grid_fits_lds(n1, n2, ncell) ? 1 : 0;
}
// launch groups: 0 = tables in global scratch, 1 = tables in LDS, 2 = everything in LDS / 1024 lanes, 3 = everything in
// LDS / 256 lanes (n1 <= GRID_SMALL_ROWS)
inline int grid_group(int32_t n1, int32_t n2, int64_t ncell, int32_t n_items, bool dirs)
{
    const int mode = grid_mode(n1, n2, ncell, n_items, dirs);
    return mode == 2 && n1 <= GRID_SMALL_ROWS ? 3 : mode;
}
// dynamic LDS a problem of the group asks for: group 2 takes everything (one workgroup per CU either way: the spare LDS
// holds the candidates); group 3 adds room for the candidate runs (64 per row) so that several problems share a CU
inline size_t grid_group_lds_bytes(int group, int32_t n1, int32_t n2, int64_t ncell, int32_t n_items, bool dirs)
{
    if (group == 0) return 0;
    if (group == 2) return GRID_LDS_MAX_BYTES;
    size_t b = grid_lds_bytes(group == 3 ? 2 : 1, n1, n2, ncell, n_items, dirs);
    if (group == 3) {
        b += 4 * (2 * (size_t)n1 + 1 + 64 * (size_t)n1);
        b = (b + 4095) & ~size_t(4095);
        if (b > GRID_LDS_MAX_BYTES) b = GRID_LDS_MAX_BYTES;
    }
    return b;
}

// ---- global scratch of one problem, word offsets ---------------------------------------------------------------------------
// [tables when they do not fit LDS |] slot counts n1 | round depths | candidate store 2 x pair_cap; the listers (k_grid_candidates,
// k_grid_records) write their list into the store's second half.  Rows go in rounds of `threads`: GRID_THREADS, and 256 for the
// 256-lane workgroups of k_match_grid, which is the same for the problems they take (n1 <= GRID_SMALL_ROWS: one round).
// Carved from a base: word offsets from 0 on the host, addresses from the problem's scratch pointer in a kernel.
template <class B>
struct GridScratch {
    B tables, rcnt, round_k, store, listed, total;
};
template <class B, class T>
PLSLAM_GRID_HD GridScratch<B> grid_scratch_carve(B base, T table_words, int32_t n1, int32_t pair_cap, int threads = GRID_THREADS)
{
    GridScratch<B> l;
    l.tables = base;
    l.rcnt = base + table_words;
    l.round_k = l.rcnt + n1;
    l.store = l.round_k + (n1 + threads - 1) / threads;
    l.listed = l.store + (uint32_t)pair_cap;
    l.total = l.listed + (uint32_t)pair_cap;
    return l;
}
inline GridScratch<size_t> grid_scratch(int32_t n1, int32_t n2, int64_t ncell, int32_t pair_cap)
{
    return grid_scratch_carve(size_t(0), grid_fits_lds(n1, n2, ncell) ? size_t(0) : 2 * (size_t)n2 + 2 * (size_t)n1, n1, pair_cap);
}
inline size_t grid_scratch_words(int32_t n1, int32_t n2, int64_t ncell, int32_t pair_cap) { return grid_scratch(n1, n2, ncell, pair_cap).total; }

// ---- the candidate store's capacity ---------------------------------------------------------------------------------------------
// (host-side data) rows go in blocks of 1024, a block needs 1024 slots per grid item inside the windows of its fullest row
// (mutual only; without it nothing is stored).  (The 256-lane workgroups of small problems use blocks of 256: never more
// than this.)
inline int64_t grid_store_capacity_host(const int32_t* centres, int32_t n1, int32_t n_centres, const int32_t* cell_start,
                                        int32_t cols, int32_t rows, const int32_t window[4], int mutual)
{
    if (!mutual) return 0;
    int64_t total = 0, depth = 0;
    for (int32_t i1 = 0; i1 < n1; ++i1) {
        int64_t cnt = 0;
        for (int32_t c = 0; c < n_centres; ++c) {
            const int64_t k = (int64_t)i1 * n_centres + c;
            const int64_t x = centres[2 * k], y = centres[2 * k + 1];
            const int64_t min_x = x - window[0] > 0 ? x - window[0] : 0;
            const int64_t max_x = x + window[1] + 1 < cols ? x + window[1] + 1 : cols;
            const int64_t min_y = y - window[2] > 0 ? y - window[2] : 0;
            const int64_t max_y = y + window[3] + 1 < rows ? y + window[3] + 1 : rows;
            if (min_y >= max_y) continue;
            for (int64_t x_ = min_x; x_ < max_x; ++x_) cnt += cell_start[x_ * rows + max_y] - cell_start[x_ * rows + min_y];
        }
        if (cnt > depth) depth = cnt;
        if ((i1 & (GRID_THREADS - 1)) == GRID_THREADS - 1 || i1 == n1 - 1) {
            total += depth * GRID_THREADS;
            depth = 0;
        }
    }
    return total;
}
// upper bound of grid_store_capacity_host() from the grid alone: fullest cell x cells of a window, at most every item, per
// window centre; rows in blocks of 1024
inline int64_t grid_store_capacity_bound(int32_t n1, int32_t n_centres, const int32_t* cell_start, int32_t cols, int32_t rows,
                                         const int32_t window[4], int mutual)
{
    if (!mutual || n1 <= 0) return 0;
    const int64_t ncell = (int64_t)cols * rows;
    int64_t fullest = 0;
    for (int64_t c = 0; c < ncell; ++c) fullest = std::max<int64_t>(fullest, (int64_t)cell_start[c + 1] - cell_start[c]);
    const int64_t wx = std::min<int64_t>((int64_t)window[0] + window[1] + 1, cols);
    const int64_t wy = std::min<int64_t>((int64_t)window[2] + window[3] + 1, rows);
    const int64_t per_row = std::min<int64_t>(fullest * wx * wy, cell_start[ncell]) * n_centres;
    return per_row * GRID_THREADS * ((n1 + GRID_THREADS - 1) / GRID_THREADS);
}

// ---- the dense one-workgroup kernel ------------------------------------------------------------------------------------------
// LDS words: d1 8 n1 | d2 8 n2 | member 8 n1 | live 8 n1 | any n1 | memberT 8 n2 | m21 n2 | centres 2 nc n1 | R | (dirs: 4 n1 + 4 n2
// doubles' words, 8-byte aligned)
// R is one region with three lives: the grid (cell_start ncell + 1, items) while A runs; the chunk minima of the columns
// (nchunk n2) while B runs; the rows' per-word best pairs (16 n1) while C runs
PLSLAM_GRID_HD int64_t dense_region_words(int32_t n1, int32_t n2, int64_t ncell, int32_t n_items)
{
    const int32_t nchunk = (n1 + DENSE_CHUNK - 1) / DENSE_CHUNK;
    return std::max<int64_t>(ncell + 1 + n_items, std::max<int64_t>((int64_t)nchunk * n2, 16 * (int64_t)n1));
}
inline size_t grid_dense_lds_bytes(int32_t n1, int32_t n2, int64_t ncell, int32_t n_items, bool dirs, int32_t n_centres)
{
    size_t w = (size_t)(25 + 2 * n_centres) * (size_t)n1 + (size_t)17 * (size_t)n2 + (size_t)dense_region_words(n1, n2, ncell, n_items) + 2;
    if (dirs) w += 4 * ((size_t)n1 + (size_t)n2);
    return w * 4;
}
// the size half of grid_dense_ok() (match_grid.hpp), which also asks the run-time switch g_grid_dense
inline bool grid_dense_fits(int32_t n1, int32_t n2, int64_t ncell, int32_t n_items, bool dirs, int32_t n_centres)
{
    return n1 > 0 && n1 <= DENSE_MAX && n2 > 0 && n2 <= DENSE_MAX && n_centres >= 1 && n_centres <= 4 &&
           grid_dense_lds_bytes(n1, n2, ncell, n_items, dirs, n_centres) <= DENSE_LDS_MAX_BYTES;
}

// ---- the path of ONE problem on a stream (grid_launch_single) ------------------------------------------------------------------
// A small problem whose row count the host knows runs dense on one workgroup.  A mutual problem that runs LDS-resident with
// packed candidate words (what k_match_grid decides for itself) and has enough rows to be worth a second launch gets its
// distances from a many-workgroup launch first -- the records of each column, found cell by cell (k_grid_records: the
// descriptor goes by value, so the host must have it), or every candidate pair (k_grid_candidates) -- and then runs
// k_match_grid<2, 1024> over that list; everything else is one launch of its group.
struct GridShape {
    int32_t n1, n2, n_centres, cols, rows, n_items, pair_capacity;
    int32_t window[4];
    int mutual;
    bool dirs;
};
enum GridPath { GRID_PATH_DENSE, GRID_PATH_RECORDS, GRID_PATH_CANDIDATES, GRID_PATH_SINGLE };
struct GridRoute {
    GridPath path;
    int group;              // SINGLE: the launch group; the two-launch paths: 2
    int split;              // CANDIDATES: lanes per row
    unsigned workgroups;    // of the first launch (RECORDS: n_groups; CANDIDATES: 256 (row, window column) tasks each)
    int64_t n_groups;       // RECORDS / CANDIDATES: groups of REC_G cells the grid has
};
// k_grid_records can list the problem: its workgroups (one per group of REC_G cells; never more than the cells, and those fit
// LDS here: a guard), the rows a group's lists hold, and REC_SLOT words of the store's half for every item of the grid
inline bool grid_records_ok(int64_t n_groups, int32_t n1, int32_t n_items, int32_t pair_capacity)
{
    return n_groups <= REC_GROUPS_MAX && n1 <= REC_ROWS_MAX && (int64_t)n_items * REC_SLOT <= (int64_t)pair_capacity;
}
// dense_allowed: the run-time switch; has_aux: the caller provided the words the two launches share; has_h_desc: the host's
// copy of the descriptor is at hand; n1_upper_bound: q.n1 is an upper bound (the descriptor's n1 is patched on the device):
// both launches go out whenever the problem runs LDS-resident at the bound -- the kernels decide for themselves whether the
// row count admits the packed words.
inline GridRoute grid_route(const GridShape& q, bool dense_allowed, bool has_aux, bool has_h_desc, bool n1_upper_bound)
{
    GridRoute r{GRID_PATH_SINGLE, 0, 1, 0u, 0};
    const int64_t ncell = (int64_t)q.cols * q.rows;
    if (has_h_desc && !n1_upper_bound && dense_allowed && grid_dense_fits(q.n1, q.n2, ncell, q.n_items, q.dirs, q.n_centres)) {
        r.path = GRID_PATH_DENSE;
        r.workgroups = 1u;
        return r;
    }
    r.group = grid_group(q.n1, q.n2, ncell, q.n_items, q.dirs);
    // ONE problem: nothing shares the CU, and a mutual problem of <= 256 rows still has up to 1024 (row, window part) tasks
    if (r.group == 3 && q.mutual && q.n1 * GRID_SPLIT > GRID_SMALL_ROWS) r.group = 2;
    if (r.group == 2 && (grid_flat(q.mutual, q.n1, q.n2) || (n1_upper_bound && q.mutual)) && has_aux && q.n1 >= GRID_SPLIT_MIN_ROWS &&
        q.n2 > 0 && q.pair_capacity > 0) {
        const int64_t wx = std::min<int64_t>((int64_t)q.window[0] + q.window[1] + 1, q.cols);
        r.split = (int)std::max<int64_t>(1, std::min<int64_t>(wx, GRID_SPLIT_MAX));
        r.n_groups = (int64_t)q.cols * ((q.rows + REC_G - 1) / REC_G);
        if (has_h_desc && grid_records_ok(r.n_groups, q.n1, q.n_items, q.pair_capacity)) {
            r.path = GRID_PATH_RECORDS;
            r.workgroups = (unsigned)r.n_groups;
        } else {
            r.path = GRID_PATH_CANDIDATES;
            r.workgroups = (unsigned)(((int64_t)q.n1 * r.split + 255) / 256);
        }
    }
    return r;
}

}  // namespace plslam
