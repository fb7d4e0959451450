// match_tables.hpp -- the launch tables of the matcher as the kernels read them, and the few constants and predicates the
// host needs to fill them.  No HIP header: the planner (match_planner.hpp) and its CPU test compile this with a plain C++
// compiler.  common.hpp includes it for the kernels.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "plslam_hip.h"

namespace plslam {

struct ScanDesc {       // one directed scan: every query row against every train row
    const uint8_t* q;   // nq x 32
    const uint8_t* t;   // nt x 32
    uint32_t* keys;     // nq x 2 composite keys (best, second best)
    int32_t nq, nt;
};

struct ProblemDesc {    // one StVO::match problem = scan12 (+ scan21 when mutual)
    const uint32_t* keys12;
    const uint32_t* keys21;  // nullptr when !mutual
    int32_t* matches_12;
    int32_t* n_matches;      // may be nullptr
    int32_t n1, n2;
    float nnr;
    int32_t mutual;
    // column-split problems (K1f, match_planner.hpp): the row results arrive as `nsplit` tables [nsplit][n1][2] with column
    // indices relative to ranges of `cstep` columns; the finalize kernel merges them on the fly (and stores the merged pair to
    // keys12_out for diagnostics).  nsplit <= 1: keys12 is final.
    const uint32_t* split_tmp;
    uint32_t* keys12_out;
    int32_t nsplit, cstep;
    // plslam_match_problem.keep_prior: rows the ratio test rejects keep what matches_12 holds (stvo-pl's resize())
    int32_t keep_prior;
    // K1h plans: keys21[j] = (best row, best row OUTSIDE the best row's aligned group of 16 rows of d1): the exact second best
    // is recomputed here, and only for the columns a row actually points at (15 XOR + popcount distances from d1 / d2)
    int32_t lazy21;
    const uint8_t* d1;
    const uint8_t* d2;
    // index of the stereo-gate problem that consumes this table (plslam_match_plan_add_stereo_gates), or -1: the finalize
    // kernel applies the gate to a row's match the moment it is decided -- no second launch, no second pass over the table
    int32_t gate, pad2;
    // K1h / K1i plans with the fused stage behind the scan (k_post_fused): the problem's column partials -- [row block][slot]
    // words, SymDesc::part21 -- or nullptr
    const uint32_t* part21;
    // plslam_match_plan_set_wire16: the int16 mirror of matches_12 (the gather's wire format), or nullptr
    int16_t* matches_16;
};

struct BlockDesc {      // one workgroup's slice of a scan / problem
    int32_t item;       // scan or problem index
    int32_t row0;       // first query row of this workgroup
};

// symmetric scan: one mutual problem = one (a x b) distance matrix feeding both directions
struct SymDesc {
    const uint8_t* a;       // n1 rows: one per lane
    const uint8_t* b;       // n2 rows: streamed
    uint32_t* keys12;       // n1 x 2   row results (complete)
    uint32_t* keys21;       // n2 x 2   column results (written by the merge kernel)
    uint32_t* part21;       // [n_iblk][n2][2] column partials per 64-row block of a
    int32_t n1, n2;
    int32_t n_iblk;
    int32_t mutual;         // fused form (K1f, one workgroup per problem): ratio + mutual finalize happen in the scan kernel
    int32_t* matches_12;    //   n1 match-table entries (nullptr: not fused)
    int32_t* n_matches;     //   one counter, STORED (not accumulated) by the problem's workgroup; may be nullptr
    float nnr;
    int32_t flags;          // bit 0 (K1h): the INDEX of the second-best row key must be exact too (knnMatch output, key dumps)
    // K1f, two-launch column-split plans only (the brute-force map<->keyframe driver in one synchronisation, map2kf.hip): the
    // number of rows of a lives on the DEVICE (*n1_dev <= n1; n1 is the bound the tables and the launch are sized for), or nullptr
    const int32_t* n1_dev;
};

// every area and every packed table starts on a multiple of 256 bytes
constexpr size_t align256(size_t bytes) { return (bytes + 255) & ~size_t(255); }
// carve several arrays out of one scratch buffer (slices aligned as align256 says)
struct Carver {
    size_t off = 0;
    size_t take(size_t bytes) { const size_t o = off; off += align256(bytes); return o; }
};

// the kernels index these tables with fixed strides: a reordered or resized field must not slip through
static_assert(sizeof(ScanDesc) == 32, "ScanDesc layout");
static_assert(sizeof(SymDesc) == 88, "SymDesc layout");
static_assert(sizeof(ProblemDesc) == 120, "ProblemDesc layout");
static_assert(sizeof(BlockDesc) == 8, "BlockDesc layout");

// K2' (match_post.hip, k_post_fused): merge of K1h's / K1i's column partials + finalize + gates, one workgroup per problem
constexpr int POST_FUSED_MAX_N2 = 4096;
constexpr int POST_FUSED_MAX_ROW_BLOCKS = 16;
// K1f fused (hamming_mfma_g.hip): a mutual problem keeps its merged column keys in LDS
constexpr int PLSLAM_K1F_FUSED_MAX_N2 = 4096;

// K1h's tables (one column partial per 256-row block, launch_merge_fix16 behind the scan): K1h and K1i; 0 = auto (= 5)
inline bool mfma_form_is_h(int form) { return form == 0 || form == 4 || form == 5; }
// PLSLAM_BUILD_LEGACY_SCANS (plslam_amd/build.py; default 0): the earlier generations of the matrix-core scan -- K1e
// (hamming_mfma.hip, mfma_form 1), K1g (hamming_mfma_d.hip, 3) and K1h (hamming_mfma_h.hip, 4) -- are compiled in, each a source
// of the legacy library alone; the one translation unit that sees the macro is context.hip.
// AUTO never picks them; without them plslam_ctx_set_option("mfma_form", 1 | 3 | 4) returns PLSLAM_ENOTSUP.
#ifndef PLSLAM_BUILD_LEGACY_SCANS
#define PLSLAM_BUILD_LEGACY_SCANS 0
#endif
inline bool mfma_form_built(int form) { return PLSLAM_BUILD_LEGACY_SCANS || form == 0 || form == 2 || form == 5; }

}  // namespace plslam
