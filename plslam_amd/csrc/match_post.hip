// match_post.hip -- the stages behind a scan, for gfx950: the column merges (K1c), the ratio test with the mutual check (K2),
// their fused forms, and the two small utility kernels.  A scan (hamming.hip, hamming_mfma*.hip) leaves the row results
// keys12 complete and the column direction as partials per row block; what turns them into matches_12 and the match count is
// here (stvo-pl matchNNR() / match() behind cv::BFMatcher::knnMatch).  The launch interface: match_kernels.hpp.
//
// Which stage follows which scan -- plan_run (match_plan.hip) picks, in this order:
//
//   the plan (match_planner.hpp)    scan and table family                          behind it
//   split_post                      K1f, column split; 16-bit key pairs per        k_split_post<PARTS>: merge + ratio + the one row a column
//                                   64-row block                                   can match, two launches per run (k_split_rows_dump: dumps)
//   PlanTables::post_fused          K1h / K1i; one word per 256-row block          K2' k_post_fused: merge into LDS + finalize + gates, one
//                                                                                  workgroup per problem (option "post_fuse" 2, never AUTO)
//   PlanChoice::h_tables()          K1h / K1i (K1i: the DEFAULT), the same words   K1c'' k_merge_fix16<PARTS, FIX>, then K2 k_finalize
//   PlanChoice::partials16()        K1f; 16-bit key pairs per 64-row block         K1c' k_merge_partials16<PARTS>, then K2 k_finalize
//   neither                         K1b / K1b' (popcount), K1e; 32-bit key pairs   K1c k_merge_partials, then K2 k_finalize
//                                   per 64- / 256-row block
//   (directed scans: K1a, K1d, the matrix-core forms) no column direction          K2 k_finalize alone
//
// k_finalize also applies the stereo gate of the row it has just decided (stereo_gates_dev.hpp); k_scatter_counts copies the
// counters to caller pointers that are not one array; k_unpack_keys serves plslam_knn2_hamming256.  A fused K1f scan
// (hamming_mfma_g.hip, FUSED) finishes its problems itself and has no stage here.
// The file's order: the split form, the three merges, K2 (its row function, then the kernel), K2' (which calls the row function),
// the utilities; the launchers at the end in the same order.
//
// Three pieces of text exist more than once, on purpose -- a shared form changed register allocation and schedule of the
// kernels that took it: the 16-bit-partial merge loop (k_merge_partials16, k_split_post), the ratio test (ratio_pick here, the
// lambdas of k_split_post and of K1f's fused scan) and the per-range row merge (finalize_row, k_split_post, k_split_rows_dump).
#include "mfma_h_common.hpp"
#include "stereo_gates_dev.hpp"

namespace plslam {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4), aligned(4)));

// K1c'' + K2 in ONE kernel behind a column-split K1f scan (C3: one local map against one frame; mapHandler.cpp:532-752): the
// plan run is two launches.  The column side decides.  A workgroup merges the partials of its columns exactly as
// k_merge_partials16 does; the lane that then holds column j's pair applies the column's ratio test -> i* (the only row that can
// be consistent with j), merges row i*'s per-range results (the finalize kernel's best2 over `nsplit` tables, column indices
// relative to ranges of `cstep` columns), applies the row's ratio test -> m, and writes matches_12[i*] = j iff m == j: the set
// {(i, m) : m21[m] == i} of stvo-pl's match() read from the other side (every row has at most one m, every column at most
// one i*).  Rows without a match hold the -1 the scan's first column range left there; the count is the number of pairs.
// Only for mutual problems without keep_prior and without a stereo gate (plan_build / add_stereo_gates decide).
// SymDesc::mutual - 1 = the problem's index; the range's first column = (sd.b - p.d2) / 32.
template <int PARTS>
__global__ void __launch_bounds__(256)
k_split_post(const SymDesc* __restrict__ syms, const BlockDesc* __restrict__ blocks, const ProblemDesc* __restrict__ probs)
{
    constexpr int COLS = 256 / PARTS;
    __shared__ uint32_t red[PARTS > 1 ? 512 : 2];
    const BlockDesc bd = blocks[blockIdx.x];
    const SymDesc sd = syms[bd.item];
    const ProblemDesc p = probs[sd.mutual - 1];
    const int jl = (int)threadIdx.x % COLS, part_id = (int)threadIdx.x / COLS;
    const int j = bd.row0 + jl;
    const gcu32_t part = (gcu32_t) sd.part21;
    const int n1 = sd.n1_dev ? min(sd.n1, *(const PLSLAM_GLOBAL int32_t*) sd.n1_dev) : sd.n1;   // (the scan wrote the partials of these rows only)
    const int nwb = (n1 + 63) >> 6;
    const int n2p = (sd.n2 + 255) & ~255;
    uint32_t b0 = KEY_NONE, b1 = KEY_NONE;
    const uint32_t tw = ((uint32_t)j >> 5) & 63u;
    // (the merge loop of k_merge_partials16, kept apart: one shared function changed all six instantiations)
    if (j < sd.n2) {
        auto wide = [](uint32_t k16, uint32_t wb) -> uint32_t { return ((k16 << 16) & 0xFF800000u) | ((k16 & 63u) + 64u * wb); };
        const uint32_t tw2 = tw | (tw << 16);
        uint32_t s0 = 0xFFFFFFFFu;
#pragma unroll 8
        for (int wb = part_id; wb < nwb; wb += PARTS) {
            const uint32_t e = part[(size_t)wb * n2p + j] - tw2;
            const uint32_t k = wide(e & 0xFFFFu, (uint32_t)wb);
            s0 = k < b0 ? e : s0;
            b1 = umin_(b1, umax_(b0, k));
            b0 = umin_(b0, k);
        }
        if (b0 < (257u << KEY_IDX_BITS)) {
            b1 = umin_(b1, wide(s0 >> 16, (b0 & KEY_IDX_MASK) >> 6));
            if (b1 >= (257u << KEY_IDX_BITS)) b1 = KEY_NONE;
        } else {
            b0 = b1 = KEY_NONE;
        }
    }
    if (PARTS > 1) {
        red[2 * threadIdx.x] = b0;
        red[2 * threadIdx.x + 1] = b1;
        __syncthreads();
        if (part_id == 0) {
#pragma unroll
            for (int q = 1; q < PARTS; ++q) merge2(b0, b1, red[2 * (q * COLS + jl)], red[2 * (q * COLS + jl) + 1]);
        }
    }
    // stvo-pl matchNNR: accept iff (float)d0 < (float)d1 * nnr (one fp32 multiply); fewer than two neighbours: no match
    // (ratio_pick below and the lambda of K1f's fused scan, kept apart: the function in their place changed this kernel and that scan)
    auto ratio_pick = [&](uint32_t q0, uint32_t q1) -> int {
        if (q1 == KEY_NONE) return -1;
        const float d0 = (float)(q0 >> KEY_IDX_BITS);
        const float d1n = __fmul_rn((float)(q1 >> KEY_IDX_BITS), p.nnr);
        return d0 < d1n ? (int)(q0 & KEY_IDX_MASK) : -1;
    };
    bool pair = false;
    if (part_id == 0 && j < sd.n2) {
        ((gu2_t) reinterpret_cast<u32x2_t*>(sd.keys21))[j] = u32x2_t{b0, b1};          // diagnostics (plslam_match_plan_dump)
        const int istar = ratio_pick(b0, b1);
        if (istar >= 0) {
            const int jg = j + (int)((sd.b - p.d2) >> 5);                               // the column within the problem
            const int ns = p.nsplit > 1 ? p.nsplit : 1;
            const auto tmp = (const PLSLAM_GLOBAL u32x2_t*) reinterpret_cast<const u32x2_t*>(p.nsplit > 1 ? p.split_tmp : p.keys12);
            uint32_t r0 = KEY_NONE, r1 = KEY_NONE;
            // (the per-range row merge of finalize_row and k_split_rows_dump, kept apart: for one row, unrolled by four)
#pragma unroll 4
            for (int s = 0; s < ns; ++s) {
                const u32x2_t q = tmp[(size_t)s * p.n1 + istar];
                const uint32_t off = (uint32_t)(s * p.cstep);
                merge2(r0, r1, q.x == KEY_NONE ? KEY_NONE : q.x + off, q.y == KEY_NONE ? KEY_NONE : q.y + off);
            }
            pair = ratio_pick(r0, r1) == jg;
            if (pair) ((PLSLAM_GLOBAL int32_t*) p.matches_12)[istar] = jg;
        }
    }
    if (p.n_matches) {
        const int found = (int)__popcll(__ballot(pair));
        if ((threadIdx.x & 63) == 0 && found) (void)atomic_add_global(p.n_matches, found);
    }
}

// plslam_match_plan_dump of a two-launch column-split plan: the rows' merged pairs (what the finalize kernel of the three-launch
// form stores to keys12_out on its way), a lane per row
__global__ void __launch_bounds__(256)
k_split_rows_dump(const ProblemDesc* __restrict__ probs, const BlockDesc* __restrict__ blocks)
{
    const BlockDesc bd = blocks[blockIdx.x];
    if (bd.item < 0) return;                               // (padding entry of a dealt table)
    const ProblemDesc p = probs[bd.item];
    const int i1 = bd.row0 + (int)threadIdx.x;
    if (i1 >= p.n1 || p.nsplit <= 1) return;
    const auto tmp = (const PLSLAM_GLOBAL u32x2_t*) reinterpret_cast<const u32x2_t*>(p.split_tmp);
    uint32_t r0 = KEY_NONE, r1 = KEY_NONE;
    // (the per-range row merge of finalize_row and k_split_post, kept apart: a kernel of its own for the dump)
    for (int s = 0; s < p.nsplit; ++s) {
        const u32x2_t q = tmp[(size_t)s * p.n1 + i1];
        const uint32_t off = (uint32_t)(s * p.cstep);
        merge2(r0, r1, q.x == KEY_NONE ? KEY_NONE : q.x + off, q.y == KEY_NONE ? KEY_NONE : q.y + off);
    }
    ((gu2_t) reinterpret_cast<u32x2_t*>(p.keys12_out))[i1] = u32x2_t{r0, r1};
}

// K1c''  merge of K1h's column partials + the second-best recomputation: keys21[j] = best-2 over all rows of a.
// part[256-row block][slot] = (d0 << 17 | row0 << 9 | d1): the block's best row and the distance of its best row OUTSIDE
// row0's aligned group of 16 rows (FIX: the pair of words (d0 << 8 | row0, d1 << 8 | row1)).  Over the blocks: K0 = the best
// row, K1 = the best of (every other block's best row, the winner block's second entry) = the best row outside K0's group of 16.
// FIX = false: keys21[j] = (K0, K1) as they are -- K1's index is not a row then (all ones) -- and the finalize kernel completes
// the second best for the columns it needs (ProblemDesc::lazy21); FIX = true (exact key tables asked for): the 15 other
// rows of K0's group are recomputed here for every column (512 contiguous bytes of a).  PARTS lanes share a column (tall
// problems: see K1f).
template <int PARTS, bool FIX>
__global__ void __launch_bounds__(256)
k_merge_fix16(const SymDesc* __restrict__ syms, const BlockDesc* __restrict__ blocks, int nblocks)
{
  // (a capped grid walks the block table: plslam_ctx option "post_workgroups")
  for (int blk = blockIdx.x; blk < nblocks; blk += gridDim.x) {
    constexpr int COLS = 256 / PARTS;
    // PARTS == 1: a lane takes SPT slots, 256 apart (one block-table entry per 1024 slots): the kernel is a chain of dependent
    // round trips (block entry -> descriptor -> partials -> store) with a few loads at its end, and four slots' loads
    // share the chain
    constexpr int SPT = PARTS == 1 ? MH_MERGE_SPT : 1;
    __shared__ uint32_t red[PARTS > 1 ? 512 : 2];
    const BlockDesc bd = blocks[blk];
    const SymDesc sd = syms[bd.item];
    // lanes walk the partial table in SLOT order (coalesced reads of every block's row); the slot's column is where the result goes
    const int jl = (int)threadIdx.x % COLS, part_id = (int)threadIdx.x / COLS;
    const MhLayout L(sd.n2);
    const gcu32_t part = (gcu32_t) sd.part21;
    const int nwb = (sd.n1 + 255) >> 8;
    const int n2p = (MH_TILE_N * L.ntiles + 255) & ~255;
    int slot[SPT], j[SPT];
    uint32_t b0[SPT], b1[SPT], s0[SPT];     // s0: the winner block's second entry, kept raw: it joins at the end
#pragma unroll
    for (int q = 0; q < SPT; ++q) {
        slot[q] = bd.row0 + jl + 256 * q;
        j[q] = slot[q] < MH_TILE_N * L.ntiles ? L.row_of(slot[q] >> 5, slot[q] & 31) : sd.n2;     // >= n2: the slot holds no column
        if (j[q] >= sd.n2) slot[q] = 0;       // (reads a valid word, drops the result)
        b0[q] = b1[q] = KEY_NONE;
        s0[q] = 0xFFFFFFFFu;
    }
    auto wide = [](uint32_t k17, uint32_t wb) -> uint32_t {         // (d << 8 | row in block) -> (d << 23 | row)
        return ((k17 >> 8) << KEY_IDX_BITS) | ((k17 & 255u) + 256u * wb);
    };
    // only a block's BEST key is widened and merged per entry
    // the default form (one word per entry, a lane per slot): the words of MH_MERGE_WB row blocks are requested together
    if (PARTS == 1 && !FIX) {
        constexpr int WB = MH_MERGE_WB;
        for (int wb0 = 0; wb0 < nwb; wb0 += WB) {
            uint32_t e[WB][SPT];
#pragma unroll
            for (int u = 0; u < WB; ++u) {
                if (wb0 + u < nwb) {                  // (uniform)
#pragma unroll
                    for (int q = 0; q < SPT; ++q)
                        e[u][q] = __builtin_nontemporal_load(&part[(size_t)(wb0 + u) * n2p + slot[q]]);
                }
            }
#pragma unroll
            for (int u = 0; u < WB; ++u) {
                if (wb0 + u < nwb) {
#pragma unroll
                    for (int q = 0; q < SPT; ++q) {
                        const uint32_t k = wide(e[u][q] >> 9, (uint32_t)(wb0 + u)), e1 = ((e[u][q] & 511u) << 8) | 255u;
                        s0[q] = k < b0[q] ? e1 : s0[q];
                        b1[q] = umin_(b1[q], umax_(b0[q], k));
                        b0[q] = umin_(b0[q], k);
                    }
                }
            }
        }
    } else
#pragma unroll 2
    for (int wb = part_id; wb < nwb; wb += PARTS) {
        uint32_t e0[SPT], e1[SPT];
#pragma unroll
        for (int q = 0; q < SPT; ++q) {
            if (FIX) {
                const gu2c_t pp = (gu2c_t) part + ((size_t)wb * n2p + slot[q]);
                const u32x2_t e = __builtin_nontemporal_load(pp);
                e0[q] = e.x; e1[q] = e.y;
            } else {
                const uint32_t e = __builtin_nontemporal_load(&part[(size_t)wb * n2p + slot[q]]);
                e0[q] = e >> 9; e1[q] = ((e & 511u) << 8) | 255u;     // the second entry's row is not in the word
            }
        }
#pragma unroll
        for (int q = 0; q < SPT; ++q) {
            const uint32_t k = wide(e0[q], (uint32_t)wb);
            s0[q] = k < b0[q] ? e1[q] : s0[q];
            b1[q] = umin_(b1[q], umax_(b0[q], k));
            b0[q] = umin_(b0[q], k);
        }
    }
#pragma unroll
    for (int q = 0; q < SPT; ++q) {
        if (j[q] < sd.n2 && b0[q] < (257u << KEY_IDX_BITS)) {
            const uint32_t k1 = FIX ? wide(s0[q], (b0[q] & KEY_IDX_MASK) >> 8) : (((s0[q] >> 8) << KEY_IDX_BITS) | KEY_IDX_MASK);
            b1[q] = umin_(b1[q], k1);
            if (b1[q] >= (257u << KEY_IDX_BITS)) b1[q] = KEY_NONE;
        } else {
            b0[q] = b1[q] = KEY_NONE;
        }
    }
    if (PARTS > 1) {
        // the parts' pairs: each is (best of its blocks, best outside THAT best's group): the overall best's pair partner is
        // still "outside its group", and any other part's best is outside it too (another block, or the same block's
        // other group only if it came as a second entry -- which is also outside) -- merge2 keeps exactly that
        if (blk != (int)blockIdx.x) __syncthreads();          // the entry before: every lane is past its reads of red[]
        red[2 * threadIdx.x] = b0[0];
        red[2 * threadIdx.x + 1] = b1[0];
        __syncthreads();
        if (part_id == 0) {
#pragma unroll
            for (int q = 1; q < PARTS; ++q) merge2(b0[0], b1[0], red[2 * (q * COLS + jl)], red[2 * (q * COLS + jl) + 1]);
        }
    }
#pragma unroll
    for (int q = 0; q < SPT; ++q) {
        if (part_id == 0 && j[q] < sd.n2) {
            if (FIX && b0[q] != KEY_NONE) {
                const gcu32_t araw = (gcu32_t) reinterpret_cast<const uint32_t*>(sd.a);
                const gcu32x4_t bp = (gcu32x4_t)((gcu32_t) reinterpret_cast<const uint32_t*>(sd.b) + (size_t)j[q] * 8);
                const u32x4_t b_lo = bp[0], b_hi = bp[1];
                const uint32_t i0 = b0[q] & KEY_IDX_MASK, ibase = i0 & ~15u;
#pragma unroll
                for (int k = 0; k < 16; ++k) {
                    const uint32_t i = ibase + (uint32_t)k;
                    const bool ok = i != i0 && i < (uint32_t)sd.n1;
                    const gcu32x4_t ap = (gcu32x4_t)(araw + (size_t)(ok ? i : i0) * 8);
                    const u32x4_t a_lo = ap[0], a_hi = ap[1];
                    const uint32_t d = hamming256(a_lo, a_hi, b_lo, b_hi);
                    b1[q] = umin_(b1[q], ok ? ((d << KEY_IDX_BITS) | i) : KEY_NONE);
                }
            }
            ((gu2_t) reinterpret_cast<u32x2_t*>(sd.keys21))[j[q]] = u32x2_t{b0[q], b1[q]};
        }
    }
  }
}

// K1c'  merge of K1f's column partials: keys21[j] = best-2 over the 64-row blocks of part16[block][j] (16-bit keys
// (d << 7 | row within the block), best | second << 16), widened to (d << 23 | row).  PARTS lanes share a column (each
// takes every PARTS-th row block, then LDS): a batch of 1500-row problems has 24 row blocks per column and thousands of
// columns (PARTS = 1: HBM-bound), ONE 10 000-row local map has 157 row blocks and 1500 columns -- a serial chain of 157
// loads per lane on 6 workgroups took longer (13.6 us) than the scan itself.
template <int PARTS>
__global__ void __launch_bounds__(256)
k_merge_partials16(const SymDesc* __restrict__ syms, const BlockDesc* __restrict__ blocks)
{
    constexpr int COLS = 256 / PARTS;
    __shared__ uint32_t red[PARTS > 1 ? 512 : 2];
    const BlockDesc bd = blocks[blockIdx.x];
    const SymDesc sd = syms[bd.item];
    const int jl = (int)threadIdx.x % COLS, part_id = (int)threadIdx.x / COLS;
    const int j = bd.row0 + jl;
    const gcu32_t part = (gcu32_t) sd.part21;
    const int nwb = (sd.n1 + 63) >> 6;
    const int n2p = (sd.n2 + 255) & ~255;                  // padded row of the partial table
    uint32_t b0 = KEY_NONE, b1 = KEY_NONE;
    const uint32_t tw = ((uint32_t)j >> 5) & 63u;          // the keys still carry + tile within the 64-tile window
    // (k_split_post holds the same merge loop, kept apart: one shared function changed all six instantiations)
    if (j < sd.n2) {
        // Only a block's BEST key is widened and merged; the second best overall is either the best of another block (b1)
        // or the second key of the block that holds the overall best (kept raw in s0, widened once at the end): half the
        // instructions per entry -- they matter because this kernel runs under the next step's instruction-bound scan.
        // A "none" half (0xFFFF - tw) widens to a key with d >= 257: it loses every comparison and is mapped to KEY_NONE
        // at the end.
        auto wide = [](uint32_t k16, uint32_t wb) -> uint32_t {         // (d << 7 | row in block) -> (d << 23 | row)
            return ((k16 << 16) & 0xFF800000u) | ((k16 & 63u) + 64u * wb);
        };
        const uint32_t tw2 = tw | (tw << 16);
        uint32_t s0 = 0xFFFFFFFFu;
#pragma unroll 8
        for (int wb = part_id; wb < nwb; wb += PARTS) {
            const uint32_t e = __builtin_nontemporal_load(&part[(size_t)wb * n2p + j]) - tw2;    // both halves >= tw: no borrow between them
            const uint32_t k = wide(e & 0xFFFFu, (uint32_t)wb);
            s0 = k < b0 ? e : s0;
            b1 = umin_(b1, umax_(b0, k));
            b0 = umin_(b0, k);
        }
        if (b0 < (257u << KEY_IDX_BITS)) {
            b1 = umin_(b1, wide(s0 >> 16, (b0 & KEY_IDX_MASK) >> 6));
            if (b1 >= (257u << KEY_IDX_BITS)) b1 = KEY_NONE;
        } else {
            b0 = b1 = KEY_NONE;
        }
    }
    if (PARTS > 1) {
        red[2 * threadIdx.x] = b0;
        red[2 * threadIdx.x + 1] = b1;
        __syncthreads();
        if (part_id == 0) {
#pragma unroll
            for (int q = 1; q < PARTS; ++q) merge2(b0, b1, red[2 * (q * COLS + jl)], red[2 * (q * COLS + jl) + 1]);
        }
    }
    if (part_id == 0 && j < sd.n2) ((gu2_t) reinterpret_cast<u32x2_t*>(sd.keys21))[j] = u32x2_t{b0, b1};
}

// K1c  merge the per-block column partials of K1b: keys21[j] = best-2 over iblk of part21[iblk][j]
__global__ void __launch_bounds__(256)
k_merge_partials(const SymDesc* __restrict__ syms, const BlockDesc* __restrict__ blocks)
{
    const BlockDesc bd = blocks[blockIdx.x];
    const SymDesc sd = syms[bd.item];
    const int j = bd.row0 + (int)threadIdx.x;
    if (j >= sd.n2) return;
    const auto part = g_(reinterpret_cast<const gvec2_t*>(sd.part21));
    uint32_t b0 = KEY_NONE, b1 = KEY_NONE;
    for (int ib = 0; ib < sd.n_iblk; ++ib) {
        const gvec2_t p = part[(size_t)ib * sd.n2 + j];
        merge2(b0, b1, p.x, p.y);
    }
    g_(reinterpret_cast<gvec2_t*>(sd.keys21))[j] = gvec2_t{b0, b1};
}

// ---------------------------------------------------------------------------------------------
// K2  finalize: ratio test (fp32, one multiply) + mutual consistency -> matches_12, #matches.
// stvo-pl matchNNR: accept iff (float)d0 < (float)d1 * nnr; match(): keep i1->i2 iff m21[i2]==i1.
// ---------------------------------------------------------------------------------------------
// (the lambdas of k_split_post and of K1f's fused scan are this function, kept apart: see there)
__device__ __forceinline__ int ratio_pick(uint32_t k0, uint32_t k1, float nnr)
{
    if (k1 == KEY_NONE) return -1;  // fewer than two neighbours: defined as "no match"
    const float d0 = (float)(k0 >> KEY_IDX_BITS);
    const float d1n = __fmul_rn((float)(k1 >> KEY_IDX_BITS), nnr);
    return d0 < d1n ? (int)(k0 & KEY_IDX_MASK) : -1;
}

// One row of a problem: ratio test on its scan result, the mutual check against the candidate column's pair kb = fetch_kb(m)
// (K1h / K1i plans: completed lazily, see below), the table entry, the count and the stereo gate.  EVERY lane of the workgroup
// calls it (DPP row rotations inside); the workgroup's 256 lanes are 256 consecutive rows starting at a multiple of 16.
// `pre`: the row's pair of keys12 if the caller has loaded it already (problems that are not column-split), else nullptr.
template <class FetchKb>
__device__ __forceinline__ void finalize_row(const ProblemDesc& p, const int i1, const plslam_stereo_gate_problem* __restrict__ gates,
                                             FetchKb fetch_kb, const gvec2_t* pre = nullptr)
{
    int m = -1;
    bool accepted = false, cleared = false;
    uint2 k = make_uint2(KEY_NONE, KEY_NONE);            // this row's scan result (rows past n1: none)
    uint2 kb = make_uint2(KEY_NONE, KEY_NONE);           // the candidate column's keys21 pair
    bool check = false;                                  // this row has a candidate whose consistency must be checked
    if (i1 < p.n1) {
        if (p.nsplit > 1) {
            // column-split problem: best-2 over the ranges' row results; keys are (d << 23 | j) with j relative to the
            // range, so its first column is added first -- (d, j) order holds within and across ranges
            // (k_split_post and k_split_rows_dump hold the same merge, kept apart: see there)
            const auto tmp = g_(reinterpret_cast<const gvec2_t*>(p.split_tmp));
            uint32_t b0 = KEY_NONE, b1 = KEY_NONE;
            for (int s = 0; s < p.nsplit; ++s) {
                const gvec2_t q = tmp[(size_t)s * p.n1 + i1];
                const uint32_t off = (uint32_t)(s * p.cstep);
                merge2(b0, b1, q.x == KEY_NONE ? KEY_NONE : q.x + off, q.y == KEY_NONE ? KEY_NONE : q.y + off);
            }
            k = make_uint2(b0, b1);
            g_(reinterpret_cast<gvec2_t*>(p.keys12_out))[i1] = gvec2_t{k.x, k.y};          // diagnostics (plslam_match_plan_dump)
        } else if (pre) {
            k = make_uint2(pre->x, pre->y);
        } else {
            // (read once: non-temporal, like the table written below -- they must not push the scan's rows out of L2)
            const gvec2_t kv = __builtin_nontemporal_load(g_(reinterpret_cast<const gvec2_t*>(p.keys12)) + i1);
            k = make_uint2(kv.x, kv.y);
        }
        m = ratio_pick(k.x, k.y, p.nnr);
        accepted = m >= 0;
        // [RECALL] stvo-pl matchNNR resize()s the table it is given: an entry already there survives a rejected row, then
        // goes through the consistency loop like any other (an entry outside [0, n2) -- an out-of-bounds read upstream --
        // is defined as failing it)
        if (!accepted && p.keep_prior) m = g_(p.matches_12)[i1];
        if (m >= 0 && p.mutual) {
            check = m < p.n2;
            if (check) kb = fetch_kb(m);
            else { m = -1; cleared = true; }
        }
    }
    bool ok = true;
    if (!p.lazy21) {
        if (check) ok = ratio_pick(kb.x, kb.y, p.nnr) == i1;
    } else {
        // K1h plans.  kb.x = column m's best row (exact); kb.y = its best row OUTSIDE kb.x's aligned group of 16 rows of d1: an
        // upper bound of the true second best.  The consistency check can only hold if the best row is THIS row; then the
        // other 15 rows of this row's group are what kb.y has not seen.  Row r's own scan result bounds its distance to
        // column m from below: it IS r's best distance if m is r's best column, and it is at least r's second-best distance
        // otherwise.  Those results sit in the neighbouring lanes (a group = 16 aligned lanes: DPP row rotation).  With the
        // lower bound lo = min(kb.y's distance, the 15 bounds) and the upper bound hi = kb.y's distance on the same side of
        // the ratio threshold the test is decided; only between them are the 15 distances recomputed (XOR + popcount).
        const uint32_t mm = check ? (uint32_t)m : 0xFFFFFFFFu;
        uint32_t lb = 0xFFFFFFFFu;                       // min over the other rows of the group of their bound (a distance)
#define PLSLAM_FIN_ROT(S)                                                                           \
        {                                                                                          \
            const uint32_t px = (uint32_t)__builtin_amdgcn_update_dpp(-1, (int)k.x, 0x120 + (S), 0xf, 0xf, false); \
            const uint32_t py = (uint32_t)__builtin_amdgcn_update_dpp(-1, (int)k.y, 0x120 + (S), 0xf, 0xf, false); \
            const uint32_t b = (px != KEY_NONE && (px & KEY_IDX_MASK) == mm) ? (px >> KEY_IDX_BITS)  \
                                                                           : (py == KEY_NONE ? 0xFFFFFFFFu : (py >> KEY_IDX_BITS)); \
            lb = lb < b ? lb : b;                                                                  \
        }
        PLSLAM_FIN_ROT(1) PLSLAM_FIN_ROT(2) PLSLAM_FIN_ROT(3) PLSLAM_FIN_ROT(4) PLSLAM_FIN_ROT(5)
        PLSLAM_FIN_ROT(6) PLSLAM_FIN_ROT(7) PLSLAM_FIN_ROT(8) PLSLAM_FIN_ROT(9) PLSLAM_FIN_ROT(10)
        PLSLAM_FIN_ROT(11) PLSLAM_FIN_ROT(12) PLSLAM_FIN_ROT(13) PLSLAM_FIN_ROT(14) PLSLAM_FIN_ROT(15)
#undef PLSLAM_FIN_ROT
        if (check) {
            ok = kb.x != KEY_NONE && (int)(kb.x & KEY_IDX_MASK) == i1;
            if (ok) {
                const float d0 = (float)(kb.x >> KEY_IDX_BITS);
                const uint32_t hi = kb.y == KEY_NONE ? 0xFFFFFFFFu : (kb.y >> KEY_IDX_BITS);
                const uint32_t lo = hi < lb ? hi : lb;
                if (hi != 0xFFFFFFFFu && !(d0 < __fmul_rn((float)hi, p.nnr))) {
                    ok = false;                                      // fails even against the upper bound
                } else if (lo != 0xFFFFFFFFu && d0 < __fmul_rn((float)lo, p.nnr)) {
                    ok = true;                                       // holds even against the lower bound (a second row exists)
                } else {
                    uint32_t second = kb.y;
                    const auto b = g_(reinterpret_cast<const u32x4*>(p.d2 + (size_t)m * 32));
                    const u32x4 b_lo = b[0], b_hi = b[1];
                    const int base = i1 & ~15;
                    for (int q = 0; q < 16; ++q) {
                        const int i = base + q;
                        const bool use = i != i1 && i < p.n1;
                        const auto a = g_(reinterpret_cast<const u32x4*>(p.d1 + (size_t)(use ? i : i1) * 32));
                        const u32x4 a_lo = a[0], a_hi = a[1];
                        const uint32_t d = __popc(a_lo.x ^ b_lo.x) + __popc(a_lo.y ^ b_lo.y) + __popc(a_lo.z ^ b_lo.z) +
                                           __popc(a_lo.w ^ b_lo.w) + __popc(a_hi.x ^ b_hi.x) + __popc(a_hi.y ^ b_hi.y) +
                                           __popc(a_hi.z ^ b_hi.z) + __popc(a_hi.w ^ b_hi.w);
                        const uint32_t cand = use ? ((d << KEY_IDX_BITS) | (uint32_t)i) : KEY_NONE;
                        second = second < cand ? second : cand;
                    }
                    ok = ratio_pick(kb.x, second, p.nnr) == i1;
                }
            }
        }
    }
    if (check && !ok) { m = -1; cleared = true; }
    if (i1 < p.n1) {
        __builtin_nontemporal_store(m, g_(p.matches_12) + i1);
        // the gather's wire table (plslam_match_plan_set_wire16): the same entry as int16 (m < n2 <= 32768)
        if (p.matches_16) g_(p.matches_16)[i1] = (int16_t)m;
    }
    if (p.n_matches) {
        // the reference's arithmetic: +1 per row the ratio test accepts, -1 per entry the consistency loop clears (equal
        // to the number of entries >= 0 unless kept entries are involved)
        const int delta = (int)__popcll(__ballot(accepted)) - (int)__popcll(__ballot(cleared));
        if ((threadIdx.x & 63) == 0 && delta) (void)atomic_add_global(p.n_matches, delta);
    }
    if (gates && p.gate >= 0) {           // (a plan without a gate stage passes no table: never read through a stale index)
        // StereoFrame's gate over this L<->R table (stereo_gates_dev.hpp), on the entry just decided.  (Requesting the gate's
        // descriptor and the row's left feature ahead of the keys -- two links off the chain of dependent accesses -- measured
        // 2.5 % SLOWER for the stages behind the scan, 0.298 against 0.290 ms per 4096-pair step.)
        const plslam_stereo_gate_problem q = gates[p.gate];
        const int kept = i1 < p.n1 ? stereo_gate_row(q, i1, m) : 0;
        const unsigned long long bal = __ballot(kept);
        if (q.n_stereo && (threadIdx.x & 63) == 0 && bal) (void)atomic_add_global(q.n_stereo, (int)__popcll(bal));
    }
}

__global__ void __launch_bounds__(256)
k_finalize(const ProblemDesc* __restrict__ probs, const BlockDesc* __restrict__ blocks,
           const plslam_stereo_gate_problem* __restrict__ gates, int nblocks, int per_xcd)
{
  // per_xcd > 0: workgroup b runs on XCD b % 8 and takes table entry (b % 8) * per_xcd + b / 8, so that the (<= 6) row blocks of
  // one problem gather their column pairs keys21[m] through ONE L2 -- in table order they sit on six XCDs and each fetches
  // the problem's whole column table (round-4 counters: FETCH_SIZE 488 k KiB per 4096-pair step against 174 k; tools/
  // fetch_gather_calib.hip reproduces the pattern and the factor).  Option "post_xcd" 2 (default): plan_build deals the table
  // to the XCDs problem by problem (rows of per_xcd entries, padding item = -1) -- consecutive problems on different XCDs, the
  // eight sweep memory together: step time equal to 1 % better, the stage alone 2 % slower.  Option 1: per_xcd = ceil(nblocks /
  // 8) over the table in problem order, i.e. a contiguous eighth per XCD: the same bytes but 8 % SLOWER for the stage (0.302
  // against 0.280 ms per step) -- eight distant regions of memory at a time.
  // (a capped grid walks the block table: plslam_ctx option "post_workgroups")
  const int nslots = per_xcd > 0 ? 8 * per_xcd : nblocks;
  for (int b = blockIdx.x; b < nslots; b += gridDim.x) {
    const int blk = per_xcd > 0 ? (b & 7) * per_xcd + (b >> 3) : b;
    if (blk >= nblocks) continue;                      // (the whole workgroup: finalize_row's DPP rotations see all lanes or none)
    const BlockDesc bd = blocks[blk];
    if (bd.item < 0) continue;                         // padding entry of a table dealt to the XCDs (option "post_xcd" 2)
    const ProblemDesc p = probs[bd.item];
    finalize_row(p, bd.row0 + (int)threadIdx.x, gates, [&](int m) {
        const gvec2_t kv = g_(reinterpret_cast<const gvec2_t*>(p.keys21))[m];
        return make_uint2(kv.x, kv.y);
    });
  }
}

// K2'  everything behind a K1h / K1i scan in ONE kernel, one workgroup per problem: the column partials of the problem's <= 16
// row blocks are merged into LDS (what k_merge_fix16<1, false> writes to keys21: best row, distance of the best row outside
// its group of 16), then the problem's rows are finalized from there (+ gates).  No merged column table in HBM: the separate
// kernels write it once (8 B per column) and gather it back through up to six L2s with 8-byte reads (round 3 PMC: 1.0 GB
// fetched to write 0.16 GB).  Throughput plans only (plan_build: every problem mutual, on K1h / K1i, n2 <= POST_FUSED_MAX_N2,
// lazy keys): a plan of a few large problems has too few workgroups for this.
template <int NT>
__global__ void __launch_bounds__(NT)
k_post_fused(const ProblemDesc* __restrict__ probs, const plslam_stereo_gate_problem* __restrict__ gates, int nprob)
{
    extern __shared__ __attribute__((aligned(16))) uint2 kb_lds[];           // [n2]: the merged pair of every column
    for (int pi = blockIdx.x; pi < nprob; pi += gridDim.x) {
        const ProblemDesc p = probs[pi];
        const MhLayout L(p.n2);
        const int nwb = (p.n1 + 255) >> 8, n2p = L.slots_padded(), nslots = 32 * L.ntiles;
        const auto part = g_(p.part21);
        if (pi != (int)blockIdx.x) __syncthreads();        // the problem before: every lane is past its reads of kb_lds
        // the first 256 rows of keys12 now: their latency passes under the merge
        const auto k12 = g_(reinterpret_cast<const gvec2_t*>(p.keys12));
        gvec2_t kcur = gvec2_t{KEY_NONE, KEY_NONE};
        if ((int)threadIdx.x < p.n1) kcur = __builtin_nontemporal_load(k12 + threadIdx.x);
        // merge: a lane takes slots 256 apart, PF at a time (their nwb words each are requested together: one round trip)
        constexpr int PF = NT >= 1024 ? 2 : 4;
        for (int s0_ = (int)threadIdx.x; s0_ < nslots; s0_ += NT * PF) {
            uint32_t b0[PF], b1[PF], sx[PF];
            int j[PF];
#pragma unroll
            for (int q = 0; q < PF; ++q) {
                const int slot = s0_ + NT * q;
                j[q] = slot < nslots ? L.row_of(slot >> 5, slot & 31) : p.n2;
                b0[q] = b1[q] = KEY_NONE;
                sx[q] = 0xFFFFFFFFu;
            }
            for (int wb = 0; wb < nwb; ++wb) {
                uint32_t e[PF];
#pragma unroll
                for (int q = 0; q < PF; ++q) e[q] = j[q] < p.n2 ? __builtin_nontemporal_load(&part[(size_t)wb * n2p + s0_ + NT * q]) : 0xFFFFFFFFu;
#pragma unroll
                for (int q = 0; q < PF; ++q) {
                    const uint32_t e0 = e[q] >> 9, e1 = ((e[q] & 511u) << 8) | 255u;     // (d0 << 8 | row0), the second entry's distance
                    const uint32_t k = ((e0 >> 8) << KEY_IDX_BITS) | ((e0 & 255u) + 256u * (uint32_t)wb);
                    sx[q] = k < b0[q] ? e1 : sx[q];
                    b1[q] = umin_(b1[q], umax_(b0[q], k));
                    b0[q] = umin_(b0[q], k);
                }
            }
#pragma unroll
            for (int q = 0; q < PF; ++q) {
                if (j[q] >= p.n2) continue;                // the slot holds no column
                if (b0[q] < (257u << KEY_IDX_BITS)) {
                    b1[q] = umin_(b1[q], ((sx[q] >> 8) << KEY_IDX_BITS) | KEY_IDX_MASK);
                    if (b1[q] >= (257u << KEY_IDX_BITS)) b1[q] = KEY_NONE;
                } else {
                    b0[q] = b1[q] = KEY_NONE;
                }
                kb_lds[j[q]] = make_uint2(b0[q], b1[q]);
            }
        }
        __syncthreads();
        // rows: the next block's keys are requested before this block's are consumed
#pragma unroll 1
        for (int r0 = 0; r0 < p.n1; r0 += NT) {
            const int inext = r0 + NT + (int)threadIdx.x;
            gvec2_t knext = gvec2_t{KEY_NONE, KEY_NONE};
            if (inext < p.n1) knext = __builtin_nontemporal_load(k12 + inext);
            finalize_row(p, r0 + (int)threadIdx.x, gates, [&](int m) { return kb_lds[m]; }, &kcur);
            kcur = knext;
        }
    }
}

// copies the per-problem counters to caller pointers that are not one contiguous array
__global__ void __launch_bounds__(256)
k_scatter_counts(const int32_t* __restrict__ src, int32_t* const* __restrict__ dst, int32_t n)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n && g_(dst)[i]) *g_(g_(dst)[i]) = g_(src)[i];
}

// keys -> (idx, dist) pairs of the knnMatch ABI
__global__ void __launch_bounds__(256)
k_unpack_keys(const uint32_t* __restrict__ keys, int32_t n, int32_t* __restrict__ idx,
              int32_t* __restrict__ dist)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint32_t k = g_(keys)[i];
    idx[i] = k == KEY_NONE ? -1 : (int32_t)(k & KEY_IDX_MASK);
    dist[i] = k == KEY_NONE ? INT32_MAX : (int32_t)(k >> KEY_IDX_BITS);
}

// ---------------------------------------------------------------------------------------------
// host-side launchers, in the kernels' order.  The order is part of the machine code: the kernel templates are instantiated
// where their launchers stand, and with k_post_fused instantiated in front of a merge kernel the compiler lays k_finalize's
// blocks out differently (tools/isa_same.py against the commit that gathered these stages here).
// ---------------------------------------------------------------------------------------------
int merge_partials16_cols(int parts) { return 256 / (parts >= 16 ? 16 : parts >= 4 ? 4 : 1); }

// d_blocks: the merge kernel's table, one entry per (sub-problem, merge_partials16_cols(parts) columns)
int launch_split_post(const SymDesc* d_sym, const BlockDesc* d_blocks, int nblocks, int parts, const ProblemDesc* d_probs, hipStream_t s)
{
    if (nblocks <= 0) return PLSLAM_OK;
    if (parts >= 16) hipLaunchKernelGGL((k_split_post<16>), dim3(nblocks), dim3(256), 0, s, d_sym, d_blocks, d_probs);
    else if (parts >= 4) hipLaunchKernelGGL((k_split_post<4>), dim3(nblocks), dim3(256), 0, s, d_sym, d_blocks, d_probs);
    else hipLaunchKernelGGL((k_split_post<1>), dim3(nblocks), dim3(256), 0, s, d_sym, d_blocks, d_probs);
    PLSLAM_HIP_CHECK(hipGetLastError());
    return PLSLAM_OK;
}

int launch_split_rows_dump(const ProblemDesc* d_probs, const BlockDesc* d_fin_blocks, int nblocks, hipStream_t s)
{
    if (nblocks <= 0) return PLSLAM_OK;
    hipLaunchKernelGGL(k_split_rows_dump, dim3(nblocks), dim3(256), 0, s, d_probs, d_fin_blocks);
    PLSLAM_HIP_CHECK(hipGetLastError());
    return PLSLAM_OK;
}

int merge_fix16_cols(int parts) { return parts >= 16 ? 16 : parts >= 4 ? 64 : 256 * MH_MERGE_SPT; }

// d_blocks: one entry per (problem, merge_fix16_cols(parts) column slots)
int launch_merge_fix16(const SymDesc* d_sym, const BlockDesc* d_blocks, int nblocks, int parts, bool fix, hipStream_t s, int grid_cap)
{
    if (nblocks <= 0) return PLSLAM_OK;
    const int grid = grid_cap > 0 && grid_cap < nblocks ? grid_cap : nblocks;
#define PLSLAM_MH_MERGE(P) { if (fix) hipLaunchKernelGGL((k_merge_fix16<P, true>), dim3(grid), dim3(256), 0, s, d_sym, d_blocks, nblocks); \
                             else hipLaunchKernelGGL((k_merge_fix16<P, false>), dim3(grid), dim3(256), 0, s, d_sym, d_blocks, nblocks); }
    if (parts >= 16) PLSLAM_MH_MERGE(16)
    else if (parts >= 4) PLSLAM_MH_MERGE(4)
    else PLSLAM_MH_MERGE(1)
#undef PLSLAM_MH_MERGE
    PLSLAM_HIP_CHECK(hipGetLastError());
    return PLSLAM_OK;
}

// d_blocks: one entry per (problem, merge_partials16_cols(parts) columns)
int launch_merge_partials16(const SymDesc* d_sym, const BlockDesc* d_blocks, int nblocks, int parts, hipStream_t s)
{
    if (nblocks <= 0) return PLSLAM_OK;
    if (parts >= 16) hipLaunchKernelGGL((k_merge_partials16<16>), dim3(nblocks), dim3(256), 0, s, d_sym, d_blocks);
    else if (parts >= 4) hipLaunchKernelGGL((k_merge_partials16<4>), dim3(nblocks), dim3(256), 0, s, d_sym, d_blocks);
    else hipLaunchKernelGGL((k_merge_partials16<1>), dim3(nblocks), dim3(256), 0, s, d_sym, d_blocks);
    PLSLAM_HIP_CHECK(hipGetLastError());
    return PLSLAM_OK;
}

int launch_merge_partials(const SymDesc* d_sym, const BlockDesc* d_blocks, int nblocks, hipStream_t s)
{
    if (nblocks <= 0) return PLSLAM_OK;
    hipLaunchKernelGGL(k_merge_partials, dim3(nblocks), dim3(256), 0, s, d_sym, d_blocks);
    PLSLAM_HIP_CHECK(hipGetLastError());
    return PLSLAM_OK;
}

int launch_finalize(const ProblemDesc* d_probs, const BlockDesc* d_blocks, int nblocks,
                    const plslam_stereo_gate_problem* d_gates, hipStream_t s, int grid_cap, bool xcd_chunks, int dealt_row)
{
    if (nblocks <= 0) return PLSLAM_OK;
    // xcd_chunks: contiguous table entries per XCD (k_finalize; option post_xcd 1, measured slower); pointless below a few entries
    // per XCD.  dealt_row > 0: the table is already dealt to the XCDs in 8 rows of that length (plan_build, option post_xcd 2).
    const int per_xcd = dealt_row > 0 ? dealt_row : (xcd_chunks && nblocks >= 64 ? (nblocks + 7) / 8 : 0);
    const int nslots = per_xcd > 0 ? 8 * per_xcd : nblocks;
    int grid = grid_cap > 0 && grid_cap < nslots ? grid_cap : nslots;
    if (per_xcd > 0 && grid < nslots) grid = grid >= 8 ? grid & ~7 : 8;   // a walking workgroup stays on its XCD's chunk
    hipLaunchKernelGGL(k_finalize, dim3(grid), dim3(256), 0, s, d_probs, d_blocks, d_gates, nblocks, per_xcd);
    PLSLAM_HIP_CHECK(hipGetLastError());
    return PLSLAM_OK;
}

constexpr int POST_FUSED_THREADS = 256;
int launch_post_fused(const ProblemDesc* d_probs, int nprob, const plslam_stereo_gate_problem* d_gates, size_t lds_bytes,
                      hipStream_t s)
{
    if (nprob <= 0) return PLSLAM_OK;
    // (measured per 16 384-problem step at C2, exclusive: this kernel with 256 lanes per problem 0.335 ms, with 1024 lanes
    // 0.65 ms, the separate merge + finalize kernels 0.276 ms -- see match_planner.hpp plan_decide, option "post_fuse")
    hipLaunchKernelGGL(k_post_fused<POST_FUSED_THREADS>, dim3(nprob), dim3(POST_FUSED_THREADS), lds_bytes, s, d_probs, d_gates, nprob);
    PLSLAM_HIP_CHECK(hipGetLastError());
    return PLSLAM_OK;
}

int launch_scatter_counts(const int32_t* d_src, int32_t* const* d_dst, int32_t n, hipStream_t s)
{
    if (n <= 0) return PLSLAM_OK;
    hipLaunchKernelGGL(k_scatter_counts, dim3((n + 255) / 256), dim3(256), 0, s, d_src, d_dst, n);
    PLSLAM_HIP_CHECK(hipGetLastError());
    return PLSLAM_OK;
}

int launch_unpack_keys(const uint32_t* d_keys, int32_t n, int32_t* d_idx, int32_t* d_dist,
                       hipStream_t s)
{
    if (n <= 0) return PLSLAM_OK;
    hipLaunchKernelGGL(k_unpack_keys, dim3((n + 255) / 256), dim3(256), 0, s, d_keys, n, d_idx,
                       d_dist);
    PLSLAM_HIP_CHECK(hipGetLastError());
    return PLSLAM_OK;
}

}  // namespace plslam
