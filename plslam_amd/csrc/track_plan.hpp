// track_plan.hpp -- the pure host half of the tracker (track.hip, include/plslam_track.h): the argument checks, the row
// capacities, the one block every buffer of the object is carved from, and the three launches' shapes.  No HIP in here, no
// context, no device: tests/cpp/test_track_plan.cpp compiles it with g++ alone and runs it under the sanitizers.  Addresses
// called "device" are only added to, never read through.
#pragma once

#include <cstdint>

#include "match_tables.hpp"   // Carver
#include "plslam_track.h"

namespace plslam {

#ifndef PLSLAM_REQUIRE
#define PLSLAM_REQUIRE(cond, code) do { if (!(cond)) return (code); } while (0)
#endif

constexpr int TRACK_THREADS = 256;      // K108, K109 and K110 alike

// one kind of one pair: the prev arrays where prev has rows, the curr arrays where both frames have
inline int track_check_kind(const int32_t* m, const int32_t* st_prev, const double* disp_prev, const float* f_prev,
                            const int32_t* st_curr, const float* f_curr, int32_t n_prev, int32_t n_curr)
{
    PLSLAM_REQUIRE(n_prev >= 0 && n_curr >= 0, PLSLAM_EINVAL);
    PLSLAM_REQUIRE(n_prev == 0 || (m && st_prev && disp_prev && f_prev), PLSLAM_EINVAL);
    PLSLAM_REQUIRE(n_prev == 0 || n_curr == 0 || (st_curr && f_curr), PLSLAM_EINVAL);
    PLSLAM_REQUIRE(n_prev <= PLSLAM_LC_MAX_FEATURES && n_curr <= PLSLAM_LC_MAX_FEATURES, PLSLAM_ERANGE);
    return PLSLAM_OK;
}

inline int track_check_pair(const plslam_track_pair* p)
{
    int rc;
    PLSLAM_REQUIRE(p != nullptr, PLSLAM_EINVAL);
    if ((rc = track_check_kind(p->m_pt, p->st_pt_prev, p->disp_pt_prev, p->kp_prev, p->st_pt_curr, p->kp_curr, p->n_pt_prev, p->n_pt_curr))) return rc;
    return track_check_kind(p->m_ls, p->st_ls_prev, p->disp_ls_prev, p->seg_prev, p->st_ls_curr, p->seg_curr, p->n_ls_prev, p->n_ls_curr);
}

// the rows the packed arrays hold at most: every prev row of the batch a correspondence
struct TrackCaps { int64_t pt = 0, ls = 0; };

// everything plslam_track_batch_create refuses, but the params' iteration counts (lc_plan.hpp: lc_check_params); caps: out
inline int track_check(const void* ctx, const plslam_lc_params* params, const plslam_track_pair* pairs, int32_t B, const void* out,
                       TrackCaps& caps)
{
    int rc;
    caps = TrackCaps{};
    PLSLAM_REQUIRE(ctx && params && out, PLSLAM_EINVAL);
    PLSLAM_REQUIRE(B >= 0, PLSLAM_EINVAL);
    PLSLAM_REQUIRE(B <= PLSLAM_LC_MAX_BATCH, PLSLAM_ERANGE);
    PLSLAM_REQUIRE(B == 0 || pairs, PLSLAM_EINVAL);
    for (int32_t b = 0; b < B; ++b) {
        if ((rc = track_check_pair(pairs + b))) return rc;
        caps.pt += pairs[b].n_pt_prev;
        caps.ls += pairs[b].n_ls_prev;
    }
    PLSLAM_REQUIRE(caps.pt < (int64_t(1) << 31) && caps.ls < (int64_t(1) << 31), PLSLAM_ERANGE);   // the offsets are int32
    return PLSLAM_OK;
}

// ---- the buffer table: every array of the object, in the order it is carved from ONE device block (each on a multiple of
// 256 bytes).  A row array of a kind without rows keeps one row, so that no address of the table is null or shared.
enum TrackBuf {
    TB_PAIRS,      // B plslam_track_pair: what K108 and K110 read
    TB_COUNTS,     // 2 B int32: K108's counts, points then lines
    TB_PT_OFF, TB_LS_OFF,
    TB_PT_ROWS, TB_LS_ROWS,
    TB_P, TB_PL, TB_SPEP, TB_LE,
    TB_PT_INL, TB_LS_INL,
    TB_RESULTS,
    TB_COUNT
};

struct TrackLayout {
    size_t off[TB_COUNT] = {};
    size_t bytes_of[TB_COUNT] = {};     // the data bytes of each array (what a download copies)
    size_t bytes = 0;                   // of the block; 0 for B = 0
};

inline TrackLayout track_layout(int32_t B, const TrackCaps& caps)
{
    TrackLayout L;
    if (B <= 0) return L;
    const size_t nb = (size_t)B, np = (size_t)caps.pt, nl = (size_t)caps.ls;
    const size_t row[TB_COUNT] = {sizeof(plslam_track_pair), 4, 4, 4, 8, 8, 24, 16, 48, 24, 1, 1, sizeof(plslam_lc_result)};
    const size_t n[TB_COUNT] = {nb, 2 * nb, nb + 1, nb + 1, np, nl, np, np, nl, nl, np, nl, nb};
    Carver c;
    for (int i = 0; i < TB_COUNT; ++i) {
        L.bytes_of[i] = n[i] * row[i];
        L.off[i] = c.take((n[i] ? n[i] : 1) * row[i]);
    }
    L.bytes = c.off;
    return L;
}

// the object's public view of its block at device address `base`
inline plslam_track_buffers track_buffers(const TrackLayout& L, char* base, int32_t B, const TrackCaps& caps)
{
    plslam_track_buffers o{};
    o.B = B;
    o.pt_capacity = caps.pt;
    o.ls_capacity = caps.ls;
    if (B <= 0 || !base) return o;
    o.pt_off = reinterpret_cast<const int32_t*>(base + L.off[TB_PT_OFF]);
    o.ls_off = reinterpret_cast<const int32_t*>(base + L.off[TB_LS_OFF]);
    o.pt_rows = reinterpret_cast<const int32_t*>(base + L.off[TB_PT_ROWS]);
    o.ls_rows = reinterpret_cast<const int32_t*>(base + L.off[TB_LS_ROWS]);
    o.P = reinterpret_cast<const double*>(base + L.off[TB_P]);
    o.pl_obs = reinterpret_cast<const double*>(base + L.off[TB_PL]);
    o.sPeP = reinterpret_cast<const double*>(base + L.off[TB_SPEP]);
    o.le_obs = reinterpret_cast<const double*>(base + L.off[TB_LE]);
    o.pt_inlier = reinterpret_cast<const uint8_t*>(base + L.off[TB_PT_INL]);
    o.ls_inlier = reinterpret_cast<const uint8_t*>(base + L.off[TB_LS_INL]);
    o.results = reinterpret_cast<const plslam_lc_result*>(base + L.off[TB_RESULTS]);
    return o;
}

// ---- the launches of one run, in order: K108 and K110 one workgroup per (pair, kind), K109 one workgroup
struct TrackLaunch { uint32_t gx, gy, threads; };
struct TrackLaunches { TrackLaunch count, scan, write; int n; };   // n: launches in front of K54 (0: the run launches nothing)
inline TrackLaunches track_launches(int32_t B)
{
    TrackLaunches t{};
    if (B <= 0) return t;
    t.count = t.write = TrackLaunch{(uint32_t)B, 2u, (uint32_t)TRACK_THREADS};
    t.scan = TrackLaunch{1u, 1u, (uint32_t)TRACK_THREADS};
    t.n = 3;
    return t;
}

// K109: lane t of the one workgroup sums and then writes the offsets of this many consecutive pairs
inline int32_t track_scan_chunk(int32_t B) { return (B + TRACK_THREADS - 1) / TRACK_THREADS; }

}  // namespace plslam
