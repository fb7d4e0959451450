// match_grid_listers.hip -- the two kernels that evaluate the distances of ONE large LDS-resident mutual matchGrid problem on the
// whole chip, in front of k_match_grid<2, 1024> (match_grid.hip), which does the bookkeeping over the list they leave in the
// second half of the problem's candidate store: k_grid_candidates lists every candidate pair, k_grid_records each column's
// records only.  Which of them a problem gets: grid_route() (match_grid_layout.hpp).
#include "match_grid_dev.hpp"

namespace plslam {
namespace {

// PA of ONE LDS-resident mutual problem spread over the chip (k_match_grid with `pre` does the rest): a lane per (row, window
// column) -- `split` = the window's width in cells, at most GRID_SPLIT_MAX: a lane's chain of dependent reads is centre -> cell
// offsets -> items -> desc2 rows, once --, 256 tasks per workgroup, every table read from global memory (the grid and the desc2 rows are
// a few tens of KB: L2).  A single workgroup spends two thirds of its time here -- a few 10^4 distances behind scattered
// reads, with the lanes of a wave unevenly loaded -- while 255 CUs idle.  The candidate words (d << (b1 + b2) | i1 << b2 | i2,
// as in the flat mode) of a workgroup are collected in LDS and appended to the list in the SECOND half of the problem's
// candidate store (one global atomic per workgroup; aux[0] = the list's length, zero when the kernel starts); their order in the
// list is whatever the scheduling made it -- nothing downstream depends on it (every combination is a min of keys).
constexpr uint32_t GRID_CAND_BUF = 6144;            // candidate words a workgroup collects before they go out (24 KB)
__global__ __launch_bounds__(256) void k_grid_candidates(const GridDesc* __restrict__ probs, uint32_t* __restrict__ aux, int split)
{
    __shared__ uint32_t s_buf[GRID_CAND_BUF];
    __shared__ uint32_t s_n, s_base;
    const GridDesc g = probs[0];
    const int tid = (int)threadIdx.x;
    const int32_t n1 = g.n1, n2 = g.n2;
    const int32_t ncell = g.cols * g.rows;
    const uint32_t fb2 = grid_col_bits((uint32_t)n2), fb1 = grid_row_bits(fb2);
    GridPtrs<0> P;
    P.cs = (PLSLAM_AS_GLOBAL const uint32_t*)g.cell_start;
    P.items = (PLSLAM_AS_GLOBAL const int32_t*)g.cell_items;
    P.d2 = (PLSLAM_AS_GLOBAL const u32x4*)g.d2;
    P.centres = (PLSLAM_AS_GLOBAL const int32_t*)g.centres;
    P.dir1 = (PLSLAM_AS_GLOBAL const double*)g.dir1;
    P.dir2 = (PLSLAM_AS_GLOBAL const double*)g.dir2;
    P.state = P.next = P.row_k1 = P.row_k2 = nullptr;
    // the scratch layout of k_match_grid<2, 1024> (no tables: they are in LDS): the list goes to the store's second half
    PLSLAM_AS_GLOBAL uint32_t* raw = grid_scratch_carve((PLSLAM_AS_GLOBAL uint32_t*)g.scratch, 0, n1, g.pair_cap).listed;
    PLSLAM_AS_GLOBAL const u32x4* g_d1 = (PLSLAM_AS_GLOBAL const u32x4*)g.d1;
    uint32_t* const counter = aux;
    if (!(g.mutual && (uint32_t)n2 <= (1u << fb2) && (uint32_t)n1 <= (1u << fb1))) return;   // grid_flat(): k_match_grid evaluates its own otherwise
    if (tid == 0) s_n = 0u;
    __syncthreads();
    const int64_t task = (int64_t)blockIdx.x * 256 + tid;
    if (task < (int64_t)n1 * split && (uint32_t)P.cs[ncell] <= (uint32_t)g.n_items) {      // (an inconsistent grid: k_match_grid reports it)
        const int32_t i1 = (int32_t)(task / split), part = (int32_t)(task - (int64_t)i1 * split);
        const u32x4 qa = g_d1[2 * (int64_t)i1], qb = g_d1[2 * (int64_t)i1 + 1];
        for_candidates(g, P, i1, [&](const int32_t (&i2)[CB]) {
            u32x4 ta[CB], tb[CB];
#pragma unroll
            for (int j = 0; j < CB; ++j) {
                const int64_t t = i2[j] < 0 ? 0 : i2[j];
                ta[j] = P.d2[2 * t];
                tb[j] = P.d2[2 * t + 1];
            }
            uint32_t n_keep = 0;
#pragma unroll
            for (int j = 0; j < CB; ++j) n_keep += i2[j] >= 0 ? 1u : 0u;
            if (n_keep) {
                uint32_t pos = atomicAdd(&s_n, n_keep);               // one claim per batch
#pragma unroll
                for (int j = 0; j < CB; ++j)
                    if (i2[j] >= 0) {
                        const uint32_t d = (uint32_t)(__popc(qa.x ^ ta[j].x) + __popc(qa.y ^ ta[j].y) + __popc(qa.z ^ ta[j].z) +
                                                      __popc(qa.w ^ ta[j].w) + __popc(qb.x ^ tb[j].x) + __popc(qb.y ^ tb[j].y) +
                                                      __popc(qb.z ^ tb[j].z) + __popc(qb.w ^ tb[j].w));
                        const uint32_t word = (d << (fb1 + fb2)) | ((uint32_t)i1 << fb2) | (uint32_t)i2[j];
                        if (pos < GRID_CAND_BUF) s_buf[pos] = word;
                        else {                                        // (a very dense grid) straight to the list
                            const uint32_t gp = (uint32_t)atomic_add_global(counter, 1);
                            if (gp < (uint32_t)g.pair_cap) raw[gp] = word;
                        }
                        ++pos;
                    }
            }
        }, part, split);
    }
    __syncthreads();
    const uint32_t n = s_n < GRID_CAND_BUF ? s_n : GRID_CAND_BUF;
    if (tid == 0) s_base = n ? (uint32_t)atomic_add_global(counter, (int)n) : 0u;
    __syncthreads();
    for (uint32_t k = (uint32_t)tid; k < n; k += 256u)
        if (s_base + k < (uint32_t)g.pair_cap) raw[s_base + k] = s_buf[k];
}


// The same list, pre-filtered, COLUMN-wise: a workgroup per REC_G vertically adjacent grid cells.  The rows whose windows
// touch the group come out of one sweep over every row's window centres (a few KB from L2; each wave sweeps a quarter of the
// rows and compacts its finds IN ROW ORDER, each with the mask of the group's cells its windows hold); a wave then takes a
// column (an item of one of the cells), evaluates its distance to those rows -- lane j the j-th row -- and a prefix minimum
// across the lanes says which of them are the column's records (d below every earlier row's): those words alone are kept.  A
// column of ~19 candidates has ~3 records, so what k_match_grid bookkeeps shrinks from ~28 k to ~4 k words for a keyframe
// pair, and no lane walks the dependent chain centre -> cell offsets -> items -> desc2 rows of k_grid_candidates.
// What k_match_grid needs: every live candidate, and candidates only.  A column whose item sits in SEVERAL cells (line
// segments) gets the records of each cell's row set -- a superset of its records (a record of the union is a record of any
// subset that holds it), and the bookkeeping downstream drops the rest: a dead candidate has an earlier RECORD at or below its
// distance, and every record is kept.
// Where they go: item k of the grid's CSR list (one (cell, column) run) owns words k * REC_SLOT ... + REC_SLOT - 1 of the list,
// records first, KEY_NONE behind them -- no counter to claim, nothing returns to the wave (a round trip of a global atomic is
// ~1 us here, and every workgroup of the launch wanted the same word).  The records a run has beyond REC_SLOT (a column in a
// hundred) are listed from the END of the store downwards, aux[0] counting them (their place does not depend on the grid).  The FIRST word of an item's slots is a record
// exactly when the run has any: k_match_grid counts those per column to see whether a column has one run (the list then holds
// its records and nothing else) or several.
// The descriptor comes BY VALUE (kernel arguments): one dependent round trip less in front of everything.
constexpr int REC_NT = 256;
__global__ __launch_bounds__(REC_NT) void k_grid_records(const GridDesc g, uint32_t* __restrict__ aux, const int32_t* __restrict__ n1_dev)
{
    // n1_dev: where the row count lives when a kernel upstream decides it (g.n1 is then its upper bound, and still what the
    // scratch layout is counted by)
    constexpr int NW = REC_NT / 64, PER_WAVE = REC_ROWS_MAX / NW, SWEEP_UN = 16;
    static_assert(REC_G <= 8, "a row's cells fit an 8-bit mask");
    __shared__ uint16_t s_rows[NW][PER_WAVE];         // wave w's finds among rows [w * q, (w + 1) * q), ascending
    __shared__ uint8_t s_mask[NW][PER_WAVE];
    __shared__ int32_t s_cs[REC_G + 1];
    __shared__ uint32_t s_wn[NW];
    const int tid = (int)threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    int32_t n1 = g.n1;
    if (n1_dev) {
        const int32_t n1_now = *(PLSLAM_AS_GLOBAL const int32_t*)n1_dev;
        n1 = n1_now >= 0 && n1_now < n1 ? n1_now : n1;
    }
    const int32_t n2 = g.n2;
    const int32_t ncell = g.cols * g.rows;
    const uint32_t fb2 = grid_col_bits_clz(n2), fb1 = grid_row_bits(fb2);
    if (!(g.mutual && fb2 <= 22u && (uint32_t)n1 <= (1u << fb1)) || n1 > REC_ROWS_MAX) return;   // !grid_flat() (launcher: never)
    PLSLAM_AS_GLOBAL const int32_t* cs = (PLSLAM_AS_GLOBAL const int32_t*)g.cell_start;
    PLSLAM_AS_GLOBAL const int32_t* items = (PLSLAM_AS_GLOBAL const int32_t*)g.cell_items;
    PLSLAM_AS_GLOBAL const int32_t* centres = (PLSLAM_AS_GLOBAL const int32_t*)g.centres;
    PLSLAM_AS_GLOBAL const u32x4* g_d1 = (PLSLAM_AS_GLOBAL const u32x4*)g.d1;
    PLSLAM_AS_GLOBAL const u32x4* g_d2 = (PLSLAM_AS_GLOBAL const u32x4*)g.d2;
    PLSLAM_AS_GLOBAL const double* dir1 = (PLSLAM_AS_GLOBAL const double*)g.dir1;
    PLSLAM_AS_GLOBAL const double* dir2 = (PLSLAM_AS_GLOBAL const double*)g.dir2;
    const bool dirs = g.dir1 != nullptr && g.dir2 != nullptr;
    // (the layout k_grid_candidates writes, counted by the descriptor's row count)
    PLSLAM_AS_GLOBAL uint32_t* raw = grid_scratch_carve((PLSLAM_AS_GLOBAL uint32_t*)g.scratch, 0, g.n1, g.pair_cap).listed;
    const int32_t gpc = (g.rows + REC_G - 1) / REC_G;                   // groups per grid column
    const int32_t cx = (int32_t)blockIdx.x / gpc, cy0 = ((int32_t)blockIdx.x - cx * gpc) * REC_G;
    if (cx >= g.cols) return;
    const int32_t ng = g.rows - cy0 < REC_G ? g.rows - cy0 : REC_G, cell0 = cx * g.rows + cy0;
    // the group's slice of the CSR list and this wave's first rows' centres: requested together
    const int32_t it_all = cs[ncell], it_begin = cs[cell0], it_end = cs[cell0 + ng];
    const int32_t my_cs = tid <= ng ? cs[cell0 + tid] : 0;
    const int32_t q = (n1 + NW - 1) / NW, r_begin = wv * q, r_end = r_begin + q < n1 ? r_begin + q : n1;
    const bool one_centre = g.n_centres == 1;
    int32_t cxy[SWEEP_UN][2];
    if (one_centre) {
#pragma unroll
        for (int k = 0; k < SWEEP_UN; ++k) {
            const int32_t r = r_begin + k * 64 + lane;
            cxy[k][0] = cxy[k][1] = 0;
            if (r < r_end) {
                cxy[k][0] = centres[2 * (int64_t)r];
                cxy[k][1] = centres[2 * (int64_t)r + 1];
            }
        }
    }
    if ((uint32_t)it_all > (uint32_t)g.n_items || it_begin >= it_end) return;    // (an inconsistent grid: k_match_grid reports it)
    if (tid <= ng) s_cs[tid] = my_cs;
    // this wave's first columns: their numbers now (under the sweep below), their descriptors together once those are here --
    // two round trips for IT_UN columns, not two each (a group holds ~3 items, a wave takes every fourth)
    constexpr int IT_UN = 4;
    const int32_t k_first = it_begin + wv;
    int32_t i2_un[IT_UN];
#pragma unroll
    for (int t = 0; t < IT_UN; ++t) i2_un[t] = k_first + t * NW < it_end ? items[k_first + t * NW] : -1;

    // ---- the rows whose windows touch the group, each with the mask of the cells it reaches ----
    // (cell (cx, cy) of the grid lies in a centre's clamped window [min, max) exactly when cx - x is in [-w0, w1] and cy - y in
    // [-w2, w3]: the clamps of window_of only cut what no cell index reaches)
    auto cells_of = [&](int64_t x, int64_t y) -> uint32_t {
        const int64_t dx = (int64_t)cx - x;
        int64_t lo = y - g.w[2], hi = y + g.w[3];
        lo = lo > cy0 ? lo : cy0;
        hi = hi < cy0 + ng - 1 ? hi : cy0 + ng - 1;
        if (dx >= -(int64_t)g.w[0] && dx <= (int64_t)g.w[1] && lo <= hi)
            return ((2u << (uint32_t)(hi - cy0)) - 1u) & ~((1u << (uint32_t)(lo - cy0)) - 1u);
        return 0u;
    };
    const uint64_t below = (1ull << lane) - 1ull;
    uint32_t found = 0;                               // (uniform) this wave's finds so far
    auto keep = [&](int32_t r, uint32_t mask) {
        const uint64_t b = __ballot(mask != 0u);
        if (mask) {
            const uint32_t pos = found + (uint32_t)__popcll(b & below);
            s_rows[wv][pos] = (uint16_t)r;
            s_mask[wv][pos] = (uint8_t)mask;
        }
        found += (uint32_t)__popcll(b);
    };
    if (one_centre) {
#pragma unroll
        for (int k = 0; k < SWEEP_UN; ++k) {
            if (r_begin + k * 64 >= r_end) break;
            const int32_t r = r_begin + k * 64 + lane;
            keep(r, r < r_end ? cells_of(cxy[k][0], cxy[k][1]) : 0u);
        }
    }
    for (int32_t r0 = r_begin + (one_centre ? SWEEP_UN * 64 : 0); r0 < r_end; r0 += 64) {      // (many rows, or several centres a row)
        const int32_t r = r0 + lane;
        uint32_t mask = 0;
        if (r < r_end)
            for (int32_t c = 0; c < g.n_centres; ++c) {
                PLSLAM_AS_GLOBAL const int32_t* p = centres + ((int64_t)r * g.n_centres + c) * 2;
                mask |= cells_of(p[0], p[1]);
            }
        keep(r, mask);
    }
    if (lane == 0) s_wn[wv] = found;
    __syncthreads();
    uint32_t first_of[NW + 1];                        // the waves' finds, concatenated: row j of the group
    first_of[0] = 0u;
#pragma unroll
    for (int w = 0; w < NW; ++w) first_of[w + 1] = first_of[w] + s_wn[w];
    const uint32_t n_rows = first_of[NW];
    auto row_at = [&](uint32_t j, uint32_t& row, uint32_t& mk) {
        uint32_t w = 0;
#pragma unroll
        for (int t = 1; t < NW; ++t) w += j >= first_of[t] ? 1u : 0u;
        uint32_t base = 0;
#pragma unroll
        for (int t = 1; t < NW; ++t) base = w == (uint32_t)t ? first_of[t] : base;
        row = j < n_rows ? s_rows[w][j - base] : 0u;
        mk = j < n_rows ? s_mask[w][j - base] : 0u;
    };

    // ---- a wave per column; lane j holds the j-th row (the first 64 rows' descriptors are loaded once) ----
    uint32_t row_0, mask_0;
    row_at((uint32_t)lane, row_0, mask_0);
    const u32x4 qa_0 = g_d1[2 * (int64_t)row_0], qb_0 = g_d1[2 * (int64_t)row_0 + 1];
    auto run_column = [&](int32_t k, int32_t i2, const u32x4& ta, const u32x4& tb, double b0, double b1) {
        PLSLAM_AS_GLOBAL uint32_t* slot = raw + (uint64_t)(uint32_t)k * REC_SLOT;
        const bool room = ((uint64_t)(uint32_t)k + 1u) * REC_SLOT <= (uint64_t)(uint32_t)g.pair_cap;    // (launcher: always)
        uint32_t n_rec = 0;                            // (uniform) records of this run so far
        if ((uint32_t)i2 < (uint32_t)n2) {
            uint32_t cq = 0;                           // the cell of item k: how many of the group's inner boundaries lie at or below k
            for (int32_t t = 1; t < ng; ++t) cq += k >= s_cs[t] ? 1u : 0u;
            const uint32_t bit = 1u << cq;
            uint32_t carry = REC_D_MASK + 1u;          // the smallest distance of the rows before this chunk
            for (uint32_t j0 = 0; j0 < n_rows && carry; j0 += 64) {
                uint32_t row = row_0, mk = mask_0;
                u32x4 qa = qa_0, qb = qb_0;
                if (j0) {
                    row_at(j0 + (uint32_t)lane, row, mk);
                    qa = g_d1[2 * (int64_t)row];
                    qb = g_d1[2 * (int64_t)row + 1];
                }
                bool valid = (mk & bit) != 0u;
                const uint32_t d = (uint32_t)(__popc(qa.x ^ ta.x) + __popc(qa.y ^ ta.y) + __popc(qa.z ^ ta.z) + __popc(qa.w ^ ta.w) +
                                              __popc(qb.x ^ tb.x) + __popc(qb.y ^ tb.y) + __popc(qb.z ^ tb.z) + __popc(qb.w ^ tb.w));
                if (dirs) {
                    const double a0 = dir1[2 * (int64_t)row], a1 = dir1[2 * (int64_t)row + 1];
                    const double dot = a0 * b0 + a1 * b1;
                    if (fabs(dot) < g.sim_th) valid = false;     // NaN (zero-length direction) compares false: kept
                }
                const uint32_t dm = valid ? d : REC_D_MASK + 1u;
                uint32_t incl = dm;
#pragma unroll
                for (int o = 1; o < 64; o <<= 1) {
                    const uint32_t t = (uint32_t)__shfl_up((int)incl, o);
                    if (lane >= o) incl = t < incl ? t : incl;
                }
                uint32_t excl = (uint32_t)__shfl_up((int)incl, 1);
                if (lane == 0) excl = REC_D_MASK + 1u;
                excl = excl < carry ? excl : carry;
                const bool rec = valid && d < excl;
                const uint32_t all = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
                carry = all < carry ? all : carry;
                const uint64_t m = __ballot(rec);
                if (rec) {
                    const uint32_t pos = n_rec + (uint32_t)__popcll(m & below);
                    const uint32_t word = (d << (fb1 + fb2)) | (row << fb2) | (uint32_t)i2;
                    if (pos < REC_SLOT) {
                        if (room) slot[pos] = word;
                    } else {                                      // beyond the run's own words: from the store's end downwards
                        const uint32_t gp = (uint32_t)atomic_add_global(aux, 1);
                        if ((uint64_t)(uint32_t)it_all * REC_SLOT + gp < (uint64_t)(uint32_t)g.pair_cap)
                            raw[(uint32_t)g.pair_cap - 1u - gp] = word;
                    }
                }
                n_rec += (uint32_t)__popcll(m);
            }
        }
        if (room && (uint32_t)lane < REC_SLOT && (uint32_t)lane >= n_rec) slot[lane] = KEY_NONE;
    };
    {
        u32x4 ta[IT_UN], tb[IT_UN];
        double b0[IT_UN], b1[IT_UN];
#pragma unroll
        for (int t = 0; t < IT_UN; ++t) {
            const int32_t i2 = __builtin_amdgcn_readfirstlane(i2_un[t]);
            const int64_t at = (uint32_t)i2 < (uint32_t)n2 ? i2 : 0;
            ta[t] = g_d2[2 * at];
            tb[t] = g_d2[2 * at + 1];
            b0[t] = dirs ? dir2[2 * at] : 0.0;
            b1[t] = dirs ? dir2[2 * at + 1] : 0.0;
        }
#pragma unroll
        for (int t = 0; t < IT_UN; ++t) {
            if (k_first + t * NW >= it_end) break;
            run_column(k_first + t * NW, __builtin_amdgcn_readfirstlane(i2_un[t]), ta[t], tb[t], b0[t], b1[t]);
        }
    }
    for (int32_t k = k_first + IT_UN * NW; k < it_end; k += NW) {       // (a dense group)
        const int32_t i2 = __builtin_amdgcn_readfirstlane(items[k]);
        const int64_t at = (uint32_t)i2 < (uint32_t)n2 ? i2 : 0;
        const u32x4 ta = g_d2[2 * at], tb = g_d2[2 * at + 1];
        run_column(k, i2, ta, tb, dirs ? dir2[2 * at] : 0.0, dirs ? dir2[2 * at + 1] : 0.0);
    }
}

}  // namespace

// workgroups of 256 (row, window column) tasks; d_desc: the problem's descriptor on the device; aux[0]: zero, then the list's length
int launch_grid_candidates(const GridDesc* d_desc, uint32_t* aux, int split, unsigned workgroups, hipStream_t s)
{
    hipLaunchKernelGGL(k_grid_candidates, dim3(workgroups), dim3(256), 0, s, d_desc, aux, split);
    PLSLAM_HIP_CHECK(hipGetLastError());
    return PLSLAM_OK;
}

// a workgroup per group of REC_G cells; the descriptor by value (n1_dev: see the kernel); aux[0]: zero, then the records that
// did not fit their items' words
int launch_grid_records(const GridDesc& h_desc, uint32_t* aux, const int32_t* n1_dev, unsigned n_groups, hipStream_t s)
{
    hipLaunchKernelGGL(k_grid_records, dim3(n_groups), dim3(REC_NT), 0, s, h_desc, aux, n1_dev);
    PLSLAM_HIP_CHECK(hipGetLastError());
    return PLSLAM_OK;
}

}  // namespace plslam
