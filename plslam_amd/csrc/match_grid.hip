// K14 -- StVO::matchGrid, the windowed ("fast_matching") matcher, as ONE kernel launch per batch of problems.
//
// Reference: stvo-pl matching.cpp::matchGrid (both overloads) + gridStructure.cpp::GridStructure::get -- the
// un-vendored dependency, [RECALL]; call sites src/mapHandler.cpp:271 (points KF<->KF), :418 (lines), :591 (map
// points <-> KF), :706 (map lines <-> KF); grids filled by the callers at :258-264, :395-411, :580-584, :683-699.
//
// Upstream is a sequential loop over the rows i1 of desc1: the candidates of row i1 are the grid items inside the
// window(s) around its cell(s); with Config::bestLRMatches() a candidate (i1, i2) is SKIPPED unless its distance is
// strictly below the smallest distance any earlier row had to i2 (`if (d < distances[i2]) {...} else continue;`),
// and matches_21[i2] follows the rows that lowered distances[i2].  That loop-carried dependence has an order-free
// form, which is what runs here:
//     (i1, i2) takes part in row i1's best / second best   <=>   no row i1' < i1 has d(i1', i2) <= d(i1, i2),
// i.e. the live entries of a column are its strict prefix minima in row order (its "records": rows ascending,
// distances strictly descending, ending in the column's lexicographic minimum (d, i1) = matches_21[i2]).  The
// tests check this form against a literal restatement of the sequential loop.  Ties between equally distant best
// candidates go to the lowest i2 (upstream: the iteration order of a std::unordered_set<int>, implementation-
// defined).
//
// One workgroup of 1024 lanes per problem (256 for problems of at most 256 rows).  A problem is a few 10^4 distances:
// what costs is the length of dependent memory chains and the address rate of scattered loads, so the grid's cell_start,
// its items, the desc2 rows (and line directions) and the per-column / per-row words live in LDS whenever they fit
// (64 x 48 cells, 1500 + 1500 rows: 96 KB); the same code runs on global scratch when they do not.
//   PA  a lane per row: candidates in batches of 4, d = popcount(desc1[i1] ^ desc2[i2]).  Without bestLRMatches the
//       best two (d << 23 | i2) keys are folded on the spot.  With it every candidate proposes itself as its column's
//       first record (atomic min of i1 << 9 | d: the smallest row wins) and is kept for the record passes:
//       * FLAT mode (everything in LDS and row + column numbers of at most 23 bits together -- 4096 x 2048, 8192 x 1024 ..:
//         the shipped sizes): a candidate is one word that names its row, d << (b1 + b2) | i1 << b2 | i2, appended to the region of the wave that found it in the LDS that is still free
//         (its share of the global store takes what does not fit).  colbest[i2] = the smallest (d, i1) shown for the column
//         so far: a candidate that an EARLIER row matches or beats is dead whatever happens later and is never stored.
//       * otherwise: one word per candidate in the lane's slots of a transposed global store -- slot k of lane t at
//         [k][t], every access coalesced.
//   PB  record passes (bestLRMatches only).  A candidate that IS its column's newest record is live: it joins its row's
//       best two and leaves; one that is still below the record's distance proposes itself as the next record (the
//       smallest ROW below the last record's distance) and stays; the others are dropped.  About ln(candidates per column)
//       + 2 passes over geometrically shrinking lists; the last record of a column is its lexicographic minimum
//       (d, i1) = matches_21.
//       * FLAT mode: candidate-parallel -- each wave streams its own region and compacts the survivors in place (ballot +
//         prefix), so the lanes are evenly loaded whatever the rows' list lengths; records carry their pass number in the
//         top bits and alternate between two arrays, so nothing is cleared or installed between passes (one barrier per
//         pass); rows' best two via two LDS atomic mins; when at most 256 candidates are left one wave finishes alone.
//       * otherwise: a lane streams its rows' slots (row-private best two), a sweep over the columns installs the
//         proposals between passes.
//   PC  per row: ratio test `best_d < best_d2 * nnr` in fp64 (int * double upstream; best_d2 = INT_MAX when absent,
//       so a lone live candidate passes), mutual check against the column's final state, count.
// Fences: every exchange through global memory in this kernel (candidate store, the scratch tables of the modes that do not
// fit LDS) is between lanes of ONE workgroup, so the fences are workgroup-scope (__threadfence_block).  A device-scope fence
// is an L2 write-back + invalidate on this chip (buffer_wbl2 / buffer_inv), whose cost grows with what every OTHER workgroup
// on the die has written: with it a problem took 107 us among 127 others against 66 us alone.
// Duplicated candidates (an item sitting in several cells of the window, the two windows of a line overlapping) are
// harmless: the atomic min and the best-two fold are idempotent.
#include "match_grid_dev.hpp"

namespace plslam {
namespace {

// NT lanes per workgroup: 1024, or 256 for problems of at most 256 rows (a 200-line problem would leave 12 of 16 waves
// idle at every barrier -- and, in a batch, occupy a whole CU)
template <int MODE, int NT, bool BYVAL = false>
__global__ __launch_bounds__(NT) void k_match_grid(const GridDesc* __restrict__ probs, uint32_t lds_words, const uint32_t* __restrict__ pre_arg,
                                                   uint32_t pre_slots, const GridDesc one, const int32_t* __restrict__ n1_dev)
{
    // BYVAL: ONE problem, its descriptor by value in `one` (a dependent round trip less in front of everything; a run-time
    // choice between the two copies a 152-byte struct through private memory).  n1_dev (BYVAL only): where the row count lives
    // when a kernel upstream decides it -- one.n1 is then its upper bound, and still what the scratch layout is counted by.
    // pre_slots > 0: the list is k_grid_records': pre_slots words per item of the grid's CSR list (records first, KEY_NONE behind
    // them), then pre[0] more words; 0: k_grid_candidates' dense list of pre[0] words.
    // pre != nullptr (one LDS-resident mutual problem alone on the chip, MODE 2): PA's distances were evaluated by
    // k_grid_candidates on many workgroups -- every candidate word lies in the second half of the problem's candidate store,
    // pre[0] = their number --, this kernel does the bookkeeping over them (candidate-parallel: first records, the filter of
    // candidates an earlier row matches or beats, the waves' shares), then runs the record passes and PC.
    // (The two per-column atomic minima of the bookkeeping as GLOBAL atomics in k_grid_candidates instead: that kernel 10.5 ->
    // 16.1 us, this one 42.6 -> 39.4 us -- device-scope atomics are slower than one CU's LDS pipe is busy.)
    constexpr bool LDS = MODE >= 1;
    extern __shared__ u32x4 s_dyn4[];
    __shared__ uint32_t s_part[NT];
    __shared__ uint32_t s_max2[2];
    __shared__ uint32_t s_tail[GRID_TAIL];
    __shared__ uint32_t s_cur[NT / 64];              // flat mode: candidates appended to each wave's region
    __shared__ uint32_t s_seg[NT / 64 + 1];          // flat mode: first LDS word of each wave's region
    PLSLAM_AS_LDS uint32_t* s_dyn = (PLSLAM_AS_LDS uint32_t*)reinterpret_cast<uint32_t*>(s_dyn4);

    GridDesc g = BYVAL ? one : probs[blockIdx.x];
    const int tid = (int)threadIdx.x, lane = tid & 63;
    const int32_t n1_layout = g.n1;
    if (BYVAL && n1_dev) {
        const int32_t n1_now = *(PLSLAM_AS_GLOBAL const int32_t*)n1_dev;
        g.n1 = n1_now >= 0 && n1_now < n1_layout ? n1_now : n1_layout;
    }
    const int32_t n1 = g.n1, n2 = g.n2;
    const int32_t ncell = g.cols * g.rows;
    const int32_t n_rounds = (n1 + NT - 1) / NT;
    PLSLAM_AS_GLOBAL uint32_t* gscratch = (PLSLAM_AS_GLOBAL uint32_t*)g.scratch;
    PLSLAM_AS_GLOBAL const int32_t* g_cell_start = (PLSLAM_AS_GLOBAL const int32_t*)g.cell_start;
    PLSLAM_AS_GLOBAL const int32_t* g_items = (PLSLAM_AS_GLOBAL const int32_t*)g.cell_items;
    PLSLAM_AS_GLOBAL const u32x4* g_d1 = (PLSLAM_AS_GLOBAL const u32x4*)g.d1;
    PLSLAM_AS_GLOBAL const u32x4* g_d2 = (PLSLAM_AS_GLOBAL const u32x4*)g.d2;
    PLSLAM_AS_GLOBAL int32_t* g_matches = (PLSLAM_AS_GLOBAL int32_t*)g.matches_12;
    // tables: state n2 | next n2 | row_k1 n1 | row_k2 n1 | [cell_start copy (LDS only)]; in global scratch when not in LDS
    const uint32_t table_words = 2u * (uint32_t)n2 + 2u * (uint32_t)n1;
    // MODE 2: items at the next 16-byte boundary behind the tables, desc2 rows behind them -- grid_lds2()'s carving (the
    // launcher guarantees the fit)
    GridLds2<uint32_t> L2{};
    if constexpr (MODE == 2) L2 = grid_lds2<uint32_t>(n1, n2, (uint32_t)ncell, (uint32_t)g.n_items);
    const uint32_t items_off = L2.items_off, d2_off = L2.d2_off;
    GridPtrs<MODE> P;
    P.centres = (PLSLAM_AS_GLOBAL const int32_t*)g.centres;
    P.dir1 = (PLSLAM_AS_GLOBAL const double*)g.dir1;
    const bool has_dirs = g.dir1 != nullptr && g.dir2 != nullptr;
    if constexpr (LDS) {    // column / row words first: what lies behind them is free once PA is done
        P.state = s_dyn;
        P.cs = s_dyn + 2 * (n2 + n1);         // (GridLds2::cs)
    } else {
        P.cs = (PLSLAM_AS_GLOBAL const uint32_t*)g.cell_start;
        P.state = gscratch;
    }
    P.next = P.state + n2;                                  // this pass's proposals; state = newest record i1 << 9 | d
    P.row_k1 = P.next + n2;                                 // (d << 23 | i2) best live candidate of the row
    P.row_k2 = P.row_k1 + n1;                               // second best
    if constexpr (MODE == 2) {
        P.items = (PLSLAM_AS_LDS const int32_t*)(s_dyn + items_off);
        P.d2 = (PLSLAM_AS_LDS const u32x4*)(s_dyn + d2_off);
        P.dir2 = (PLSLAM_AS_LDS const double*)(s_dyn + d2_off + 8u * (uint32_t)n2);    // L2.dir2, restated; 16-byte aligned: d2_off is
    } else {
        P.items = g_items;
        P.d2 = g_d2;
        P.dir2 = (PLSLAM_AS_GLOBAL const double*)g.dir2;
    }
    // global scratch behind the tables: per-row slot counts (n1), per-round slot depth (n_rounds), the candidate store (2 x
    // pair_cap words; round r at NT * sum_{r' < r} round_k)
    // (grid_scratch_carve() of match_grid_layout.hpp, restated -- as a call it compiles to other instructions here -- with
    // rounds of NT rows: the same offsets, a 256-lane workgroup's problem being one round either way; test_grid_layout.cpp
    // pins both)
    PLSLAM_AS_GLOBAL uint32_t* rcnt = gscratch + (LDS ? 0u : table_words);   // n1
    PLSLAM_AS_GLOBAL uint32_t* round_k = rcnt + n1_layout;                   // n_rounds
    PLSLAM_AS_GLOBAL uint32_t* store = round_k + (n1_layout + NT - 1) / NT;  // 2 x pair_cap words; round r at NT * sum_{r' < r} round_k

    // ---- "flat" mode (everything in LDS, bestLRMatches, row and column numbers of at most 23 bits together): a candidate is ONE
    // word that names its row, d << (fb1 + fb2) | i1 << fb2 | i2 (fb2 = bits of a column number, fb1 = what is left, at most
    // 14: a column's record needs 9 bits for its pass number above i1 << 9 | d); PA appends the candidates of a wave's rows to the wave's own region of the
    // LDS that is still free (spilling into its share of the global store if it must), the record passes run on those
    // regions.  colbest[i2] = the smallest (d, i1) any row has shown for the column so far: a candidate that some EARLIER row
    // matches or beats is dead whatever else happens and is never stored.
    constexpr uint32_t NW = NT / 64;
    const uint32_t wv = (uint32_t)tid >> 6;
    bool flat = false;
    uint32_t fb1 = 11, fb2 = 11;                    // bits of a row / column number in the flat words
    uint32_t seg_words = 0, tail_cap = 0, reg_off = 0;
    PLSLAM_AS_LDS uint32_t* colbest = nullptr;
    // (the launcher may know an upper bound of n1 only -- the row count then comes from the device, GridDesc::n1 patched behind
    // the upload --: whether the candidates were listed by k_grid_candidates is decided here, by the same test as there)
    const uint32_t* pre = pre_arg;
    if constexpr (MODE == 2) {
        fb2 = grid_col_bits((uint32_t)n2);
        fb1 = grid_row_bits(fb2);
        flat = g.mutual && (uint32_t)n2 <= (1u << fb2) && (uint32_t)n1 <= (1u << fb1);     // grid_flat()
        if (!flat) pre = nullptr;
        // (pre: neither the items nor the desc2 rows are needed here -- their LDS goes to the candidates)
        const uint32_t pa_end = pre ? items_off : L2.colbest(has_dirs);
        colbest = s_dyn + pa_end;
        reg_off = pa_end + (uint32_t)n2;
        tail_cap = (uint32_t)g.pair_cap / NW;
    }
    // The free LDS is shared out in proportion to the (row, window part) tasks a wave owns (task t belongs to lane t % NT).
    // seg_at(w) = first word of wave w's region, seg_at(NW) = end.
    const uint32_t free_words = flat && lds_words > reg_off ? lds_words - reg_off : 0u;
    // flat PA: a row's window columns go to 4 lanes (GRID_SPLIT).  Measured against 1 and 2 and against a choice by row count
    // (1500 x 1500 points: PA 40 -> 47 us but the passes 21 -> 16.5 us, because the stored candidates spread evenly over the
    // waves' regions; 200 x 200 lines: PA 48 -> 30 us; batched +6 % / +5 %)
    constexpr int32_t split_log = 2;
    static_assert((1 << split_log) == GRID_SPLIT, "");
    const int32_t n_tasks = n1 << split_log;
    auto seg_at = [&](uint32_t w) -> uint32_t {
        uint32_t before = 0;
        for (int32_t r = 0; r * NT < n_tasks; ++r) {
            const int32_t left = n_tasks - r * NT;                        // tasks of round r
            before += (uint32_t)(left < (int32_t)(64u * w) ? left : (int32_t)(64u * w));
        }
        return reg_off + free_words * before / (uint32_t)(n_tasks > 0 ? n_tasks : 1);   // < 2^16 words x <= 8192 tasks: 32 bits do
    };
    // (read behind P0's barrier; a listed problem that takes the column-bucketed bookkeeping never needs them -- the loop
    // and its divisions on 17 lanes would hold the other waves at that barrier --: it fills them in if it falls back)
    uint32_t seg_first = 0;
    // candidate k of this wave: its LDS region first, then its share of the global store
    auto cand_load = [&](uint32_t k) -> uint32_t {
        return k < seg_words ? s_dyn[seg_first + k] : store[(size_t)wv * tail_cap + (k - seg_words)];
    };
    auto cand_store = [&](uint32_t k, uint32_t v) {
        if (k < seg_words) s_dyn[seg_first + k] = v;
        else store[(size_t)wv * tail_cap + (k - seg_words)] = v;
    };

    // ---- P0: tables ----
    // A listed problem whose PC never counts rows without candidates (nnr <= 1) reads nothing of the grid here: the column-
    // bucketed bookkeeping below takes the LDS behind the row words, cell_start copy included.  Its list's length, the first
    // COLS_EARLY words per lane of the list and the grid's item count are requested NOW: one round trip under the table
    // initialisation instead of three behind it.
    constexpr uint32_t COLS_HOLD = 32, COLS_EARLY = 12;
    const bool count_empty = 2147483647.0 < 2147483647.0 * g.nnr;     // PC's nnr > 1 rule
    const bool cols_maybe = MODE == 2 && NT == 1024 && pre != nullptr && !count_empty;
    const uint32_t col_off = 2u * (uint32_t)(n2 + n1);
    // (k_grid_records' list: the words of item tid and item tid + NT, and the first two words per lane of the records that
    // did not fit their items' -- those are listed from the END of the store downwards, so their place is known now)
    constexpr uint32_t ITEMS_EARLY = 2;
    uint32_t c_early[COLS_EARLY], total_early = 0, items_end_early = 0;
    u32x4 it_early[ITEMS_EARLY][REC_SLOT / 4];
    uint32_t ov_early[ITEMS_EARLY];
    const bool slots_early = cols_maybe && pre_slots == REC_SLOT;
    if (cols_maybe) {
        total_early = ((PLSLAM_AS_GLOBAL const uint32_t*)pre)[0];
        items_end_early = (uint32_t)g_cell_start[ncell];
        PLSLAM_AS_GLOBAL const uint32_t* raw = store + (uint32_t)g.pair_cap;
        if (slots_early) {
#pragma unroll
            for (uint32_t j = 0; j < ITEMS_EARLY; ++j) {
                const uint32_t item = (uint32_t)tid + j * NT;
                const bool in = ((uint64_t)item + 1u) * REC_SLOT <= (uint64_t)(uint32_t)g.pair_cap;
#pragma unroll
                for (uint32_t v = 0; v < REC_SLOT / 4; ++v) {
                    const u32x4 none4 = {KEY_NONE, KEY_NONE, KEY_NONE, KEY_NONE};
                    it_early[j][v] = in ? *(PLSLAM_AS_GLOBAL const u32x4*)(raw + (size_t)item * REC_SLOT + 4u * v) : none4;
                }
                ov_early[j] = item < (uint32_t)g.pair_cap ? raw[(uint32_t)g.pair_cap - 1u - item] : KEY_NONE;
            }
        } else {
#pragma unroll
            for (uint32_t j = 0; j < COLS_EARLY; ++j) {
                const uint32_t k = (uint32_t)tid + j * NT;
                c_early[j] = k < (uint32_t)g.pair_cap ? raw[k] : KEY_NONE;      // (words behind the list's end: masked later)
            }
        }
    }
    if (LDS && !cols_maybe) {
        for (int32_t j = tid; j <= ncell; j += NT) s_dyn[2 * (n2 + n1) + j] = (uint32_t)g_cell_start[j];
    }
    if (MODE == 2 && !pre) {
        PLSLAM_AS_LDS int32_t* li = (PLSLAM_AS_LDS int32_t*)(s_dyn + items_off);
        for (int32_t j = tid; j < g.n_items; j += NT) li[j] = g_items[j];
        PLSLAM_AS_LDS u32x4* lt = (PLSLAM_AS_LDS u32x4*)(s_dyn + d2_off);
        for (int32_t j = tid; j < 2 * n2; j += NT) lt[j] = g_d2[j];
        if (has_dirs) {     // a candidate's direction test sits between its item and its descriptor: not a global round trip
            PLSLAM_AS_LDS double* ld = (PLSLAM_AS_LDS double*)(s_dyn + d2_off + 8u * (uint32_t)n2);
            PLSLAM_AS_GLOBAL const double* gd = (PLSLAM_AS_GLOBAL const double*)g.dir2;
            for (int32_t j = tid; j < 2 * n2; j += NT) ld[j] = gd[j];
        }
    }
    for (int32_t j = tid; j < n2; j += NT) {
        P.state[j] = KEY_NONE;
        P.next[j] = KEY_NONE;
        if (flat && !cols_maybe) colbest[j] = KEY_NONE;
    }
    if (cols_maybe)
        for (int32_t j = tid; j <= n2; j += NT) s_dyn[col_off + j] = 0u;          // the columns' counts
    if (tid < (int)NW) s_cur[tid] = 0u;
    for (int32_t i = tid; i < n1; i += NT) {
        P.row_k1[i] = KEY_NONE;
        P.row_k2[i] = KEY_NONE;
    }
    if (!cols_maybe && tid <= (int)NW) s_seg[tid] = seg_at((uint32_t)tid);
    __syncthreads();
    if (!cols_maybe) {
        seg_first = s_seg[wv];
        seg_words = s_seg[wv + 1] - seg_first;              // this wave's region
    }
    if ((cols_maybe ? items_end_early : (uint32_t)P.cs[ncell]) > (uint32_t)g.n_items) {      // the grid holds more items than the caller declared
        for (int32_t i = tid; i < n1; i += NT) g_matches[i] = -1;
        if (tid == 0) {
            if (g.n_matches) *g_(g.n_matches) = -1;
            if (g.status) (void)atomic_add_global(g.status, 1);
        }
        return;
    }

    // ---- PA: distances ----
    uint32_t store_words = 0;        // slots claimed so far (uniform)
    uint32_t has_items = 0;          // bit r: this lane's row of round r has grid items inside its windows (mutual only)
    bool cols_done = false;          // (uniform) the column-bucketed path has produced the records and the rows' best two
    bool cols_fast = false;          // (uniform) ... straight from k_grid_records' list: a column's state is d << fb1 | row
    if (flat) {
        if (count_empty)                                                  // PC's nnr > 1 rule needs to know (cell_start is gone by then)
            for (int32_t r = 0; r < n_rounds && r < 32; ++r)
                if (r * NT + tid < n1 && count_items(g, P, r * NT + tid) > 0u) has_items |= 1u << r;
        if (pre) {
            // the candidate words of k_grid_candidates: bookkeeping in two candidate-parallel sweeps.  First every candidate
            // proposes itself as its column's first record and shows its (d, row) to colbest; then, colbest being final, a
            // candidate that an earlier row matches or beats is dropped and the others go to the waves' regions, evenly.
            // (the grid's item count has been checked against the caller's n_items, at most 2^31, by now)
            const uint32_t n_slots = pre_slots * (cols_maybe ? items_end_early : pre_slots ? (uint32_t)P.cs[ncell] : 0u);
            const uint64_t total64 = (uint64_t)n_slots + (cols_maybe ? total_early : *(PLSLAM_AS_GLOBAL const uint32_t*)pre);
            const uint32_t total = total64 > (uint64_t)(uint32_t)g.pair_cap ? (uint32_t)g.pair_cap + 1u : (uint32_t)total64;
            PLSLAM_AS_GLOBAL const uint32_t* raw = store + (uint32_t)g.pair_cap;
            // word k of the list: the items' words, then (from the end of the store downwards) what did not fit them
            auto list_at = [&](uint32_t k) -> uint32_t { return k < n_slots || !pre_slots ? raw[k] : raw[(uint32_t)g.pair_cap - 1u - (k - n_slots)]; };
            if (total > (uint32_t)g.pair_cap) {                         // (uniform) the list did not fit: report, match nothing
                for (int32_t i = tid; i < n1; i += NT) g_matches[i] = -1;
                if (tid == 0) {
                    if (g.n_matches) *g_(g.n_matches) = -1;
                    if (g.status) (void)atomic_add_global(g.status, 1);
                }
                return;
            }
            const uint32_t mk1 = (1u << fb1) - 1u, mk2 = (1u << fb2) - 1u;
            // ---- the list fits LDS whole (a keyframe pair's ~28 k candidates do; the ~5 k records k_grid_records leaves of them
            // easily): bucket it by COLUMN and read each column's records off its own segment, no passes over the whole list.
            // A column's records are, by the definition the passes implement, r_1 = min (i1 << 9 | d) over its candidates,
            // r_{k+1} = that min over the candidates with d below r_k's; its live candidates are exactly its records (they join
            // their rows' best two), its final state is the last one.  The counting sort: per-column counts by LDS atomics, an
            // exclusive scan, a second round of atomics for the places; the list itself is read ONCE, into registers
            // (COLS_HOLD words per lane).  The segments lie over the cell_start copy's place and everything behind it.
            // ---- the shortest way: the list is k_grid_records', and no column has two runs (every item of the grid in one
            // cell: points).  The list then holds each column's records and nothing else -- no liveness to settle: every word
            // joins its row's best two, a column's state is its smallest (d, row).  A lane takes an item's words (records first:
            // the first is one iff the run has any -- the counts P0 zeroed take those, and a column counted twice has two runs:
            // the tables are wiped and the bucketed bookkeeping below runs).  The returning atomics of a lane go out together.
            const uint32_t n_over = total - n_slots;                    // (total <= pair_cap here)
            if (slots_early && items_end_early <= ITEMS_EARLY * NT && n_over <= ITEMS_EARLY * NT) {
                PLSLAM_AS_LDS uint32_t* off = s_dyn + col_off;
                bool dup = false;
                auto fold = [&](uint32_t w, bool first, uint32_t& was_) {           // a record word: column state, row's best
                    const uint32_t i2 = w & mk2, i1 = (w >> fb2) & mk1, d = w >> (fb1 + fb2);
                    if (first) dup = dup || atomicAdd((uint32_t*)&off[i2], 1u) != 0u;
                    atomicMin((uint32_t*)&P.state[i2], (d << fb1) | i1);
                    was_ = atomicMin((uint32_t*)&P.row_k1[i1], (d << KEY_IDX_BITS) | i2);
                };
                auto fold2 = [&](uint32_t w, uint32_t was_) {                       // ... whichever lost goes to the second best
                    const uint32_t i2 = w & mk2, i1 = (w >> fb2) & mk1, d = w >> (fb1 + fb2), key = (d << KEY_IDX_BITS) | i2;
                    if (was_ != key) atomicMin((uint32_t*)&P.row_k2[i1], was_ > key ? was_ : key);
                };
#pragma unroll
                for (uint32_t j = 0; j < ITEMS_EARLY; ++j) {
                    if (j * NT >= items_end_early) break;
                    uint32_t w[REC_SLOT], was[REC_SLOT];
                    const bool mine = (uint32_t)tid + j * NT < items_end_early;
#pragma unroll
                    for (uint32_t v = 0; v < REC_SLOT; ++v) w[v] = mine ? it_early[j][v / 4][v % 4] : KEY_NONE;
#pragma unroll
                    for (uint32_t v = 0; v < REC_SLOT; ++v) {
                        if (!__any(w[v] != KEY_NONE)) break;                          // (records first: no lane has a later one either)
                        was[v] = 0u;
                        if (w[v] != KEY_NONE) fold(w[v], v == 0u, was[v]);
                    }
#pragma unroll
                    for (uint32_t v = 0; v < REC_SLOT; ++v) {
                        if (!__any(w[v] != KEY_NONE)) break;
                        if (w[v] != KEY_NONE) fold2(w[v], was[v]);
                    }
                }
#pragma unroll
                for (uint32_t j = 0; j < ITEMS_EARLY; ++j) {
                    if (j * NT >= n_over) break;
                    if ((uint32_t)tid + j * NT < n_over) {
                        uint32_t was_ = 0u;
                        fold(ov_early[j], false, was_);
                        fold2(ov_early[j], was_);
                    }
                }
                if (__syncthreads_or(dup)) {
                    for (int32_t j = tid; j < n2; j += NT) P.state[j] = KEY_NONE;
                    for (int32_t j = tid; j <= n2; j += NT) off[j] = 0u;
                    for (int32_t i = tid; i < n1; i += NT) {
                        P.row_k1[i] = KEY_NONE;
                        P.row_k2[i] = KEY_NONE;
                    }
                    __syncthreads();
                } else {
                    cols_done = true;
                    cols_fast = true;
                }
            }
            // (a lane per column: worth it while the columns are many and short -- 200 columns of 100 candidates each, a map's
            // lines against a keyframe's, took 107 us this way against ~30 us of record passes)
            // (k_grid_records' list holds records only: a few per run whatever the windows)
            if (!cols_done && cols_maybe && total <= COLS_HOLD * NT &&
                (pre_slots > 0u ? (uint64_t)items_end_early <= (uint64_t)GRID_RUNS_PER_COLUMN * (uint32_t)n2 : (uint64_t)total <= 24ull * (uint32_t)n2) &&
                (uint64_t)col_off + (uint32_t)n2 + 1u + total <= (uint64_t)lds_words) {
                PLSLAM_AS_LDS uint32_t* off = s_dyn + col_off;              // n2 + 1: counts (zeroed by P0), then the segments' first words
                PLSLAM_AS_LDS uint32_t* seg = off + n2 + 1;
                uint32_t c[COLS_HOLD];
                const uint32_t nj = (total + NT - 1) / NT;                  // (uniform) words per lane that exist at all: the unrolled
                                                                           // steps behind them are skipped, not predicated away
#pragma unroll
                for (uint32_t j = 0; j < COLS_HOLD; ++j) c[j] = KEY_NONE;
                if (!slots_early) {
#pragma unroll
                    for (uint32_t j = 0; j < COLS_EARLY; ++j) c[j] = (uint32_t)tid + j * NT < total ? c_early[j] : KEY_NONE;
                }
                if (slots_early || total > COLS_EARLY * NT) {
#pragma unroll
                    for (uint32_t j = 0; j < COLS_HOLD; ++j) {
                        if (j * NT >= total) break;
                        const uint32_t k = (uint32_t)tid + j * NT;
                        if (slots_early || j >= COLS_EARLY) c[j] = k < total ? list_at(k) : KEY_NONE;
                    }
                }
#pragma unroll
                for (uint32_t j = 0; j < COLS_HOLD; ++j)
                    if (j < nj && c[j] != KEY_NONE) atomicAdd((uint32_t*)&off[c[j] & mk2], 1u);
                __syncthreads();
                {   // exclusive scan of the counts: a run of columns per lane, wave scans, the waves' totals through s_part
                    const int32_t per = (n2 + NT - 1) / NT, b = tid * per, e = b + per < n2 ? b + per : n2;
                    uint32_t sum = 0;
                    for (int32_t j = b; j < e; ++j) sum += off[j];
                    uint32_t incl = sum;
#pragma unroll
                    for (int o = 1; o < 64; o <<= 1) {
                        const uint32_t t = (uint32_t)__shfl_up((int)incl, o);
                        if (lane >= o) incl += t;
                    }
                    if (lane == 63) s_part[wv] = incl;
                    __syncthreads();
                    uint32_t run = incl - sum;
                    for (uint32_t w = 0; w < wv; ++w) run += s_part[w];
                    for (int32_t j = b; j < e; ++j) {
                        const uint32_t k = off[j];
                        off[j] = run;
                        P.next[j] = run;                                  // the column's cursor
                        run += k;
                    }
                    if (tid == NT - 1) off[n2] = run;                     // every word that is not KEY_NONE (lanes behind the last column: all of them)
                    __syncthreads();
                }
#pragma unroll
                for (uint32_t j = 0; j < COLS_HOLD; ++j)
                    if (j < nj && c[j] != KEY_NONE) {
                        const uint32_t i2 = c[j] & mk2, i1 = (c[j] >> fb2) & mk1, d = c[j] >> (fb1 + fb2);
                        seg[atomicAdd((uint32_t*)&P.next[i2], 1u)] = (i1 << REC_D_BITS) | d;
                    }
                __syncthreads();
                // A lane per column; the segment goes to registers once (REG_N words, chunks of 8 that no lane of the wave
                // needs are skipped).
                constexpr int REG_N = 32, CHUNK = 8;
                for (int32_t base2 = 0; base2 < n2; base2 += NT) {
                    const int32_t i2 = base2 + tid;
                    const bool act = i2 < n2;
                    const uint32_t b = act ? off[i2] : 0u, e = act ? off[i2 + 1] : 0u, len = e - b;
                    uint32_t longest = len;                            // (uniform) the wave's longest segment
#pragma unroll
                    for (int o = 32; o > 0; o >>= 1) {
                        const uint32_t t = (uint32_t)__shfl_xor((int)longest, o);
                        longest = t > longest ? t : longest;
                    }
                    longest = (uint32_t)__builtin_amdgcn_readfirstlane((int)longest);
#define need_chunk(q) (longest > (uint32_t)((q) * CHUNK))
                    uint32_t w[REG_N];
#pragma unroll
                    for (int q = 0; q < REG_N / CHUNK; ++q) {
                        if (need_chunk(q)) {
#pragma unroll
                            for (int j = q * CHUNK; j < (q + 1) * CHUNK; ++j) {
                                const uint32_t v = seg[b + ((uint32_t)j < len ? (uint32_t)j : 0u)];   // (len 0: any word, unused)
                                w[j] = (uint32_t)j < len ? v : KEY_NONE;
                            }
                        } else {
#pragma unroll
                            for (int j = q * CHUNK; j < (q + 1) * CHUNK; ++j) w[j] = KEY_NONE;
                        }
                    }
                    uint32_t last = KEY_NONE;
                    if (!need_chunk(1)) {
                        // (uniform) segments of at most 8 words -- what k_grid_records leaves: sort them (w = row << 9 | d orders
                        // by row; 19 compare-exchanges, a min and a max each), then a word is a record iff its distance is below
                        // every earlier word's.  No sweeps, and the records' atomics go out together: two LDS round trips.
#define GRID_CE(a, b) do { const uint32_t lo_ = w[a] < w[b] ? w[a] : w[b], hi_ = w[a] < w[b] ? w[b] : w[a]; w[a] = lo_; w[b] = hi_; } while (0)
                        GRID_CE(0, 1); GRID_CE(2, 3); GRID_CE(4, 5); GRID_CE(6, 7);
                        GRID_CE(0, 2); GRID_CE(1, 3); GRID_CE(4, 6); GRID_CE(5, 7);
                        GRID_CE(1, 2); GRID_CE(5, 6);
                        GRID_CE(0, 4); GRID_CE(1, 5); GRID_CE(2, 6); GRID_CE(3, 7);
                        GRID_CE(2, 4); GRID_CE(3, 5);
                        GRID_CE(1, 2); GRID_CE(3, 4); GRID_CE(5, 6);
#undef GRID_CE
                        uint32_t run = REC_D_MASK + 1u, was[CHUNK], dd[CHUNK];
                        bool live[CHUNK];
#pragma unroll
                        for (int j = 0; j < CHUNK; ++j) {
                            const uint32_t dj = w[j] == KEY_NONE ? REC_D_MASK + 1u : w[j] & REC_D_MASK;
                            live[j] = dj < run;
                            if (live[j]) last = w[j];                                         // (the last record: the last live word)
                            run = dj < run ? dj : run;
                            dd[j] = dj;
                        }
#pragma unroll
                        for (int j = 0; j < CHUNK; ++j) {
                            const uint32_t key = (dd[j] << KEY_IDX_BITS) | (uint32_t)i2;
                            was[j] = key;
                            if (live[j]) was[j] = atomicMin((uint32_t*)&P.row_k1[w[j] >> REC_D_BITS], key);
                        }
#pragma unroll
                        for (int j = 0; j < CHUNK; ++j) {
                            const uint32_t key = (dd[j] << KEY_IDX_BITS) | (uint32_t)i2;
                            if (live[j] && was[j] != key) atomicMin((uint32_t*)&P.row_k2[w[j] >> REC_D_BITS], was[j] > key ? was[j] : key);
                        }
                    } else {
                        // a sweep is a mask, a compare, a select and a min per word; lanes whose column is done idle until the
                        // wave's last column is (a column of ~19 candidates has ~3.5 records, the worst of 64 about 8)
                        uint32_t cur_d = len ? REC_D_MASK + 1u : 0u;
                        while (__any(cur_d != 0u)) {
                            uint32_t best = KEY_NONE;
#pragma unroll
                            for (int q = 0; q < REG_N / CHUNK; ++q) {
                                if (need_chunk(q)) {
#pragma unroll
                                    for (int j = q * CHUNK; j < (q + 1) * CHUNK; ++j) {
                                        const uint32_t t = (w[j] & REC_D_MASK) < cur_d && w[j] != KEY_NONE ? w[j] : KEY_NONE;
                                        best = t < best ? t : best;
                                    }
                                }
                            }
                            if (len > (uint32_t)REG_N && cur_d)                               // (long columns) the rest from LDS, 8 reads in flight
                                for (uint32_t k = b + REG_N; k < e; k += CHUNK) {
                                    uint32_t v[CHUNK];
#pragma unroll
                                    for (int j = 0; j < CHUNK; ++j) v[j] = seg[k + j < e ? k + j : b];        // (a repeat changes no minimum)
#pragma unroll
                                    for (int j = 0; j < CHUNK; ++j)
                                        if ((v[j] & REC_D_MASK) < cur_d && v[j] < best) best = v[j];
                                }
                            if (best != KEY_NONE) {
                                cur_d = best & REC_D_MASK;
                                last = best;
                                const uint32_t key = (cur_d << KEY_IDX_BITS) | (uint32_t)i2, i1 = best >> REC_D_BITS;
                                const uint32_t was = atomicMin((uint32_t*)&P.row_k1[i1], key);
                                if (was != key) atomicMin((uint32_t*)&P.row_k2[i1], was > key ? was : key);
                            } else
                                cur_d = 0u;
                        }
                    }
                    if (act) P.state[i2] = last;
                }
#undef need_chunk
                cols_done = true;
                __syncthreads();
            } else if (cols_maybe && !cols_done) {                        // (uniform) the passes after all: what P0 left out
                __syncthreads();
                for (int32_t j = tid; j < n2; j += NT) colbest[j] = KEY_NONE;
                if (tid <= (int)NW) s_seg[tid] = seg_at((uint32_t)tid);
                __syncthreads();
                seg_first = s_seg[wv];
                seg_words = s_seg[wv + 1] - seg_first;
            }
            // (the list comes from L2: PRE_UN independent loads in flight per lane -- one load per loop trip made the two sweeps
            // 18 us of dependent round trips)
            constexpr int PRE_UN = 8;
            for (uint32_t k0 = (uint32_t)tid; k0 < (cols_done ? 0u : total); k0 += NT * PRE_UN) {
                uint32_t c[PRE_UN];
#pragma unroll
                for (int j = 0; j < PRE_UN; ++j) c[j] = k0 + (uint32_t)j * NT < total ? list_at(k0 + (uint32_t)j * NT) : KEY_NONE;
#pragma unroll
                for (int j = 0; j < PRE_UN; ++j)
                    if (c[j] != KEY_NONE) {
                        const uint32_t i2 = c[j] & mk2, i1 = (c[j] >> fb2) & mk1, d = c[j] >> (fb1 + fb2);
                        atomicMin((uint32_t*)&P.next[i2], (i1 << REC_D_BITS) | d);
                        atomicMin((uint32_t*)&colbest[i2], (d << fb1) | i1);
                    }
            }
            __syncthreads();
            const uint32_t lo = cols_done ? 0u : (uint32_t)((uint64_t)total * wv / NW);
            const uint32_t hi = cols_done ? 0u : (uint32_t)((uint64_t)total * (wv + 1) / NW);
            const uint64_t below_ = (1ull << lane) - 1ull;
            uint32_t out = 0;
            for (uint32_t base = lo; base < hi; base += 64 * PRE_UN) {
                uint32_t c[PRE_UN];
#pragma unroll
                for (int j = 0; j < PRE_UN; ++j) {
                    const uint32_t k = base + 64u * (uint32_t)j + (uint32_t)lane;
                    c[j] = k < hi ? list_at(k) : KEY_NONE;
                }
#pragma unroll
                for (int j = 0; j < PRE_UN; ++j) {
                    bool keep_ = false;
                    if (c[j] != KEY_NONE) {
                        const uint32_t i2 = c[j] & mk2, i1 = (c[j] >> fb2) & mk1, d = c[j] >> (fb1 + fb2), cb = colbest[i2];
                        keep_ = !((cb >> fb1) <= d && (cb & mk1) < i1);
                    }
                    const uint64_t m = __ballot(keep_);
                    if (keep_) {
                        const uint32_t pos = out + (uint32_t)__popcll(m & below_);
                        if (pos < seg_words + tail_cap) cand_store(pos, c[j]);
                    }
                    out += (uint32_t)__popcll(m);
                }
            }
            if (lane == 0) s_cur[wv] = out;
        }
        // a lane per (row, part of the row's window columns): rows differ a lot in their number of candidates, quarters of
        // rows much less, and there are four times as many of them to even out the lanes of a wave
        for (int32_t task = tid; task < (pre ? 0 : n_tasks); task += NT) {
            const int32_t i1 = task >> split_log;
            const u32x4 qa = g_d1[2 * (int64_t)i1], qb = g_d1[2 * (int64_t)i1 + 1];
            for_candidates(g, P, i1, [&](const int32_t (&i2)[CB]) {
                u32x4 ta[CB], tb[CB];
#pragma unroll
                for (int j = 0; j < CB; ++j) {
                    const int64_t t = i2[j] < 0 ? 0 : i2[j];
                    ta[j] = P.d2[2 * t];
                    tb[j] = P.d2[2 * t + 1];
                }
                uint32_t d[CB], was[CB];
#pragma unroll
                for (int j = 0; j < CB; ++j)
                    d[j] = (uint32_t)(__popc(qa.x ^ ta[j].x) + __popc(qa.y ^ ta[j].y) + __popc(qa.z ^ ta[j].z) +
                                      __popc(qa.w ^ ta[j].w) + __popc(qb.x ^ tb[j].x) + __popc(qb.y ^ tb[j].y) +
                                      __popc(qb.z ^ tb[j].z) + __popc(qb.w ^ tb[j].w));
#pragma unroll
                for (int j = 0; j < CB; ++j) {                        // the batch's atomics back to back, one wait
                    was[j] = 0u;                                      // (row 0 at distance 0 beats everything: "dead")
                    if (i2[j] >= 0) {
                        // the first record pass, fused: the smallest row of a column is its first record
                        atomicMin((uint32_t*)&P.next[i2[j]], ((uint32_t)i1 << REC_D_BITS) | d[j]);
                        was[j] = atomicMin((uint32_t*)&colbest[i2[j]], (d[j] << fb1) | (uint32_t)i1);
                    }
                }
                bool keep[CB];
                uint32_t n_keep = 0;
#pragma unroll
                for (int j = 0; j < CB; ++j) {
                    // stored unless an earlier row is known to match or beat it (or the slot is empty)
                    keep[j] = i2[j] >= 0 && !((was[j] >> fb1) <= d[j] && (was[j] & ((1u << fb1) - 1u)) < (uint32_t)i1);
                    n_keep += keep[j] ? 1u : 0u;
                }
                if (n_keep) {
                    uint32_t pos = atomicAdd(&s_cur[wv], n_keep);     // one claim per batch
#pragma unroll
                    for (int j = 0; j < CB; ++j)
                        if (keep[j]) {
                            if (pos < seg_words + tail_cap) cand_store(pos, (d[j] << (fb1 + fb2)) | ((uint32_t)i1 << fb2) | (uint32_t)i2[j]);
                            ++pos;
                        }
                }
            }, task & ((1 << split_log) - 1), 1 << split_log);
        }
        __threadfence_block();
        if (__syncthreads_or(s_cur[wv] > seg_words + tail_cap)) {       // a wave's share of the store does not fit: report, match nothing
            for (int32_t i = tid; i < n1; i += NT) g_matches[i] = -1;
            if (tid == 0) {
                if (g.n_matches) *g_(g.n_matches) = -1;
                if (g.status) (void)atomic_add_global(g.status, 1);
            }
            return;
        }
    }
    for (int32_t r = 0; r < (flat ? 0 : n_rounds); ++r) {
        const int32_t i1 = r * NT + tid;
        uint32_t depth = 0;
        if (g.mutual) {              // slot depth of this round = the largest item count of one of its rows
            uint32_t c = i1 < n1 ? count_items(g, P, i1) : 0u;
            if (c && r < 32) has_items |= 1u << r;      // for PC: the cell_start copy may be gone by then
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                const uint32_t o = (uint32_t)__shfl_xor((int)c, off);
                c = c > o ? c : o;
            }
            uint32_t& s_max = s_max2[r & 1];     // alternating slots: no barrier needed after the read below
            if (tid == 0) s_max = 0u;
            __syncthreads();
            if (lane == 0) atomicMax(&s_max, c);
            __syncthreads();
            depth = s_max;
            if (tid == 0) round_k[r] = depth;
            if ((uint64_t)store_words + (uint64_t)depth * NT > (uint64_t)(uint32_t)g.pair_cap) {
                // the store does not fit: report, match nothing
                for (int32_t i = tid; i < n1; i += NT) g_matches[i] = -1;
                if (tid == 0) {
                    if (g.n_matches) *g_(g.n_matches) = -1;
                    if (g.status) (void)atomic_add_global(g.status, 1);
                }
                return;
            }
        }
        if (i1 < n1) {
            const u32x4 qa = g_d1[2 * (int64_t)i1], qb = g_d1[2 * (int64_t)i1 + 1];
            uint32_t k1 = KEY_NONE, k2 = KEY_NONE, kout = 0;
            PLSLAM_AS_GLOBAL uint32_t* slot = store + store_words;
            for_candidates(g, P, i1, [&](const int32_t (&i2)[CB]) {
                u32x4 ta[CB], tb[CB];
#pragma unroll
                for (int j = 0; j < CB; ++j) {
                    const int64_t t = i2[j] < 0 ? 0 : i2[j];
                    ta[j] = P.d2[2 * t];
                    tb[j] = P.d2[2 * t + 1];
                }
#pragma unroll
                for (int j = 0; j < CB; ++j) {
                    const uint32_t d = (uint32_t)(__popc(qa.x ^ ta[j].x) + __popc(qa.y ^ ta[j].y) + __popc(qa.z ^ ta[j].z) +
                                                  __popc(qa.w ^ ta[j].w) + __popc(qb.x ^ tb[j].x) + __popc(qb.y ^ tb[j].y) +
                                                  __popc(qb.z ^ tb[j].z) + __popc(qb.w ^ tb[j].w));
                    const uint32_t key = (d << KEY_IDX_BITS) | (uint32_t)i2[j];
                    if (i2[j] >= 0) {
                        if (g.mutual) {
                            // the first record pass, fused: no column has a record yet, so every candidate proposes
                            atomicMin((uint32_t*)&P.next[i2[j]], ((uint32_t)i1 << REC_D_BITS) | d);
                            slot[slot_index<NT>(kout, tid)] = key;
                            ++kout;
                        } else
                            best2_fold(k1, k2, key);
                    }
                }
            });
            if (g.mutual)
                rcnt[i1] = kout;
            else {
                P.row_k1[i1] = k1;
                P.row_k2[i1] = k2;
            }
        }
        store_words += depth * NT;
    }
    __threadfence_block();
    __syncthreads();

    // ---- PB: record passes ----
    if (g.mutual && !cols_done) {
        // one row's share of a pass: stream its remaining candidates from `slot` (stride apart), keep the survivors
        // in `out`; returns how many
        auto pass_row = [&](int32_t i1, auto slot, auto out, auto at, uint32_t cnt) -> uint32_t {
            uint32_t k1 = P.row_k1[i1], k2 = P.row_k2[i1], kout = 0;
            for (uint32_t k0 = 0; k0 < cnt; k0 += PB_BATCH) {         // PB_BATCH independent loads in flight
                uint32_t key[PB_BATCH], st[PB_BATCH];
#pragma unroll
                for (int j = 0; j < PB_BATCH; ++j) key[j] = k0 + j < cnt ? slot[at(k0 + j)] : KEY_NONE;
#pragma unroll
                for (int j = 0; j < PB_BATCH; ++j) st[j] = P.state[key[j] == KEY_NONE ? 0u : key[j] & KEY_IDX_MASK];
#pragma unroll
                for (int j = 0; j < PB_BATCH; ++j) {
                    const uint32_t i2 = key[j] & KEY_IDX_MASK, d = key[j] >> KEY_IDX_BITS;
                    const uint32_t me = ((uint32_t)i1 << REC_D_BITS) | d;
                    // installed by the previous sweep: live
                    if (key[j] != KEY_NONE && st[j] == me) best2_fold(k1, k2, key[j]);
                    const uint32_t cur = st[j] == KEY_NONE ? 512u : st[j] & REC_D_MASK;
                    if (key[j] != KEY_NONE && d < cur) {             // still below the newest record: propose, keep
                        atomicMin((uint32_t*)&P.next[i2], me);
                        out[at(kout)] = key[j];
                        ++kout;
                    }
                }
            }
            P.row_k1[i1] = k1;
            P.row_k2[i1] = k2;
            return kout;
        };
        auto sweep = [&]() -> int {       // install the proposals; workgroup-wide "anything new?"
            if (!LDS) __threadfence_block();
            __syncthreads();
            int any = 0;
            for (int32_t i2 = tid; i2 < n2; i2 += NT) {
                const uint32_t nx = P.next[i2];
                if (nx != KEY_NONE) {
                    P.state[i2] = nx;
                    P.next[i2] = KEY_NONE;
                    any = 1;
                }
            }
            if (!LDS) __threadfence_block();
            return __syncthreads_or(any);
        };

        int more = sweep();               // installs the proposals PA made: every column's first record
        if (flat) {
            // ---- candidate-parallel passes: each wave works on its own region and compacts the survivors of a pass in
            // place (ballot + prefix: no other wave touches the region).
            // A column's record carries its pass number in the top bits, newest = smallest:
            //     rec(t, i1, d) = (TMAX - t) << (9 + fb1) | i1 << 9 | d     (TMAX = all ones of the 23 - fb1 >= 9 bits above),
            // pass t reads the records of pass t-1 from one array and proposes with an atomic min into the other: a proposal
            // of pass t beats whatever pass t-2 left there, so nothing is cleared and nothing is installed -- one barrier per
            // pass.  (Every candidate that survives pass t-1 proposed in it: its column's word in the array pass t reads IS
            // a pass t-1 record.  A column has at most 257 records: the pass number fits.)  Live candidates join their
            // row's best two with two LDS atomic mins: k1 takes the key, whichever of (old k1, key) lost goes to k2 -- every
            // key of the row except the final minimum reaches k2 exactly once.
            const uint32_t t_shift = REC_D_BITS + fb1, t_max = (1u << (32u - t_shift)) - 1u;
            const uint32_t m1 = (1u << fb1) - 1u, m2 = (1u << fb2) - 1u;
            for (int32_t i2 = tid; i2 < n2; i2 += NT) {                // the first records: pass 0
                const uint32_t v = P.state[i2];
                if (v != KEY_NONE) P.state[i2] = (t_max << t_shift) | v;
            }
            __syncthreads();
            constexpr int UN = 4;                                      // chunks of 64 candidates in flight per lane
            const uint64_t below = (1ull << lane) - 1ull;
            // one pass over the `alive` candidates of wave w's region (s_tail when w == NW); returns the survivors
            auto run_pass = [&](uint32_t w, uint32_t alive, uint32_t t) -> uint32_t {
                auto rd = (t & 1) ? P.state : P.next;
                auto wr = (t & 1) ? P.next : P.state;
                const uint32_t tag_rd = (t_max - (t - 1)) << t_shift, tag_wr = (t_max - t) << t_shift;
                uint32_t out = 0;
                for (uint32_t base = 0; base < alive; base += 64 * UN) {
                    uint32_t c[UN], rec[UN];
                    bool keep[UN];
                    // (uniform) the whole step inside the LDS region: plain LDS traffic, all loads in flight together
                    const bool in_lds = w != NW && base + 64 * UN <= seg_words;
                    PLSLAM_AS_LDS uint32_t* reg = s_dyn + seg_first;        // (in_lds: w is this wave)
#pragma unroll
                    for (int j = 0; j < UN; ++j) {
                        const uint32_t k = base + 64 * j + lane;
                        c[j] = k >= alive ? KEY_NONE : in_lds ? reg[k] : w == NW ? s_tail[k] : cand_load(k);
                    }
#pragma unroll
                    for (int j = 0; j < UN; ++j) rec[j] = rd[c[j] == KEY_NONE ? 0u : c[j] & m2];
#pragma unroll
                    for (int j = 0; j < UN; ++j) {
                        const uint32_t i2 = c[j] & m2, i1 = (c[j] >> fb2) & m1, d = c[j] >> (fb1 + fb2);
                        const uint32_t me = (i1 << REC_D_BITS) | d;
                        keep[j] = false;
                        if (c[j] != KEY_NONE) {
                            if (rec[j] == (tag_rd | me)) {                    // the record of the last pass: live
                                const uint32_t key = (d << KEY_IDX_BITS) | i2;
                                const uint32_t was = atomicMin((uint32_t*)&P.row_k1[i1], key);
                                // (a duplicate of the key -- an item in two cells of the window -- changes nothing)
                                if (was != key) atomicMin((uint32_t*)&P.row_k2[i1], was > key ? was : key);
                            } else if (d < (rec[j] & REC_D_MASK)) {           // still below it: propose, stay
                                atomicMin((uint32_t*)&wr[i2], tag_wr | me);
                                keep[j] = true;
                            }
                        }
                    }
#pragma unroll
                    for (int j = 0; j < UN; ++j) {                           // every read of this step is done: in place
                        const uint64_t m = __ballot(keep[j]);
                        if (keep[j]) {
                            const uint32_t k = out + (uint32_t)__popcll(m & below);
                            if (in_lds) reg[k] = c[j];
                            else if (w == NW) s_tail[k] = c[j];
                            else cand_store(k, c[j]);
                        }
                        out += (uint32_t)__popcll(m);
                    }
                }
                return out;
            };
            uint32_t alive = s_cur[wv], t = 1;
            bool tail = false;
            while (more) {
                alive = run_pass(wv, alive, t);
                ++t;
                PLSLAM_AS_LDS uint32_t* left_of = (PLSLAM_AS_LDS uint32_t*)s_part + (t & 1u) * NW;   // alternating: one barrier per pass
                if (lane == 0) left_of[wv] = alive;
                if (alive > seg_words) __threadfence_block();                // survivors in the global share: wave 0 may gather them
                __syncthreads();
                uint32_t left = 0;
                for (uint32_t w = 0; w < NW; ++w) left += left_of[w];
                more = left != 0u;
                if (left != 0u && left <= GRID_TAIL) {                   // few survivors: no more workgroup barriers
                    tail = true;
                    break;
                }
            }
            if (tail) {
                // the last passes of a problem carry a handful of candidates each: wave 0 gathers them and finishes alone
                // (its LDS operations are ordered; the other waves wait at the barrier below)
                if (wv == 0) {
                    uint32_t n_tail = 0;
                    PLSLAM_AS_LDS const uint32_t* left_of = (PLSLAM_AS_LDS const uint32_t*)s_part + (t & 1u) * NW;
                    for (uint32_t w = 0; w < NW; ++w) {
                        const uint32_t cw = left_of[w], first = s_seg[w], words = s_seg[w + 1] - first;
                        for (uint32_t k = lane; k < cw; k += 64)
                            s_tail[n_tail + k] = k < words ? s_dyn[first + k] : store[(size_t)w * tail_cap + (k - words)];
                        n_tail += cw;
                    }
                    while (n_tail) {
                        n_tail = run_pass(NW, n_tail, t);
                        ++t;
                    }
                }
                __syncthreads();
            }
            for (int32_t i2 = tid; i2 < n2; i2 += NT) {                  // the newest record of either array, untagged
                const uint32_t a = P.state[i2], b = P.next[i2], v = a < b ? a : b;
                P.state[i2] = v == KEY_NONE ? KEY_NONE : v & ((1u << t_shift) - 1u);
            }
            __syncthreads();
        }
        if (!flat) {
            int flip = 0;
            while (more) {
                // survivors of a pass go to the other half of the store: reads and writes never alias, so a batch's
                // loads do not wait for the previous batch's stores
                PLSLAM_AS_GLOBAL const uint32_t* __restrict__ src = store + (flip ? (uint32_t)g.pair_cap : 0u);
                PLSLAM_AS_GLOBAL uint32_t* __restrict__ dst = store + (flip ? 0u : (uint32_t)g.pair_cap);
                flip ^= 1;
                uint32_t off = 0;
                for (int32_t r = 0; r < n_rounds; ++r) {
                    const int32_t i1 = r * NT + tid;
                    if (i1 < n1) {
                        const uint32_t cnt = rcnt[i1];
                        if (cnt)
                            rcnt[i1] = pass_row(i1, src + off, dst + off, [tid](uint32_t k) { return slot_index<NT>(k, tid); }, cnt);
                    }
                    off += round_k[r] * NT;
                }
                more = sweep();
            }
        }
    }

    // ---- PC: ratio test, mutual check, count ----
    uint32_t cnt = 0;
    for (int32_t i1 = tid; i1 < n1; i1 += NT) {
        const uint32_t k1 = P.row_k1[i1], k2 = P.row_k2[i1];
        int32_t m = -1;
        if (k1 != KEY_NONE) {
            const double best_d = (double)(int32_t)(k1 >> KEY_IDX_BITS);
            const double best_d2 = k2 == KEY_NONE ? 2147483647.0 : (double)(int32_t)(k2 >> KEY_IDX_BITS);
            if (best_d < best_d2 * g.nnr) {
                const int32_t i2 = (int32_t)(k1 & KEY_IDX_MASK);
                if (!g.mutual || (cols_fast ? P.state[i2] & ((1u << fb1) - 1u) : P.state[i2] >> REC_D_BITS) == (uint32_t)i1) m = i2;
            }
        }
        else if (2147483647.0 < 2147483647.0 * g.nnr &&
                 ((g.mutual && i1 / NT < 32) ? ((has_items >> (i1 / NT)) & 1u) != 0u : count_items(g, P, i1) > 0u))
            cnt += 1;   // upstream, nnr > 1 only: a row whose candidates all fail keeps best_d = best_d2 = INT_MAX, passes
                        // `best_d < best_d2 * nnr`, gets matches_12 = best_idx = -1 and is COUNTED
        g_matches[i1] = m;
        cnt += m >= 0;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += (uint32_t)__shfl_xor((int)cnt, o);
    __syncthreads();                                         // (s_part may still be read as the scan's wave totals)
    if (lane == 0) s_part[tid >> 6] = cnt;
    __syncthreads();
    if (tid == 0 && g.n_matches) {
        uint32_t all = 0;
        for (int w = 0; w < NT / 64; ++w) all += s_part[w];
        *g_(g.n_matches) = (int32_t)all;
    }
}

}  // namespace

// one: the descriptor of a lone problem by value (d_probs is not read then); pre / pre_slots: its listed candidates
template <int MODE, int NT>
static int launch_group(const GridDesc* d_probs, int32_t n, size_t lds_bytes, hipStream_t s, const uint32_t* pre = nullptr,
                        uint32_t pre_slots = 0, const GridDesc* one = nullptr, const int32_t* n1_dev = nullptr)
{
    if (n <= 0) return PLSLAM_OK;
    if (MODE > 0) {
        static std::once_flag once;
        static hipError_t attr = hipSuccess;
        std::call_once(once, [] {
            attr = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_match_grid<MODE, NT, false>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)GRID_LDS_MAX_BYTES);
            if (attr == hipSuccess && MODE == 2 && NT == 1024)
                attr = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_match_grid<2, 1024, true>),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)GRID_LDS_MAX_BYTES);
        });
        PLSLAM_HIP_CHECK(attr);
    }
    static const GridDesc none{};
    if (one && MODE == 2 && NT == 1024)
        hipLaunchKernelGGL((k_match_grid<2, 1024, true>), dim3(1), dim3(1024), lds_bytes, s, nullptr, (uint32_t)(lds_bytes / 4), pre,
                           pre_slots, *one, n1_dev);
    else
        hipLaunchKernelGGL((k_match_grid<MODE, NT, false>), dim3((unsigned)n), dim3(NT), lds_bytes, s, d_probs,
                           (uint32_t)(lds_bytes / 4), pre, pre_slots, none, nullptr);
    PLSLAM_HIP_CHECK(hipGetLastError());
    return PLSLAM_OK;
}

// d_probs: the problems of group 3 first, then group 2, 1, 0; lds_bytes[g] = the largest grid_group_lds_bytes() in group g
int launch_match_grid(const GridDesc* d_probs, const int32_t n[4], const size_t lds_bytes[4], hipStream_t s)
{
    int rc;
    if ((rc = launch_group<2, 256>(d_probs, n[3], lds_bytes[3], s))) return rc;
    if ((rc = launch_group<2, 1024>(d_probs + n[3], n[2], lds_bytes[2], s))) return rc;
    if ((rc = launch_group<1, 1024>(d_probs + n[3] + n[2], n[1], lds_bytes[1], s))) return rc;
    return launch_group<0, 1024>(d_probs + n[3] + n[2] + n[1], n[0], 0, s);
}

// ONE LDS-resident problem whose candidates a lister launch in front of this one wrote (pre[0] = the list's length, pre_slots:
// see k_match_grid); h_desc (k_grid_records' list): the host's copy of the descriptor, which then goes by value
int launch_match_grid_listed(const GridDesc* d_desc, size_t lds_bytes, hipStream_t s, const uint32_t* pre, uint32_t pre_slots,
                             const GridDesc* h_desc, const int32_t* n1_dev)
{
    return launch_group<2, 1024>(d_desc, 1, lds_bytes, s, pre, pre_slots, h_desc, n1_dev);
}

}  // namespace plslam
