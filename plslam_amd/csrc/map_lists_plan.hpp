// map_lists_plan.hpp -- the pure host part of plslam_map_lists_refresh / plslam_map_insert_carry / plslam_lc_fuse_carry
// (map_lists.hip; the contract is in include/plslam_hip.h): every argument check that needs no device, the launch geometry and
// the carving of the scratch that holds the list of touched landmarks.  No HIP in here: tests/cpp/test_map_lists_plan.cpp compiles
// it with the host compiler alone.
#pragma once

#include <cstddef>
#include <cstdint>

#include "map_image.hpp"      // MAP_TILE; ListsRecords: what the handle's last insert / run left for a carry
#include "match_tables.hpp"   // Carver
#include "plslam_hip.h"

struct plslam_map_insert;
struct plslam_lc_fuse;

namespace plslam {

constexpr int LISTS_TILE = MAP_TILE;     // lanes per workgroup of K85-K88: the map kernels' one tile (map_image.hpp)
constexpr int LISTS_LANES_PER_OBS = 8;   // K85: lanes 0-1 the descriptor (2 x 16 bytes), 2-4 the direction (3 x 8), 5-6 pts (2 x 16)

// the rows of one kind, whichever call they belong to (plslam_map_insert_rows / plslam_lc_fuse_rows have this layout)
struct ListsRows {
    const uint8_t* desc[2] = {nullptr, nullptr};
    const double* pts[2] = {nullptr, nullptr};
};

struct ListsKindPlan {
    int32_t src_n = 0, src_obs = 0, dst_n = 0, dst_obs = 0;
    bool with_pts = false;
    unsigned g_carry = 0, g_lm = 0, g_rows = 0;          // workgroups of K85, of K86 / K88, of K87; 0 = not launched
    size_t o_part = 0, o_cnt = 0, o_tl = 0, o_toff = 0;  // in the scratch: 2 g_lm chain words, 2 counters, dst_n, dst_n + 1 int32
};
struct ListsPlan {
    ListsKindPlan k[2];
    size_t zero_bytes = 0, scratch_bytes = 0;            // the front of the scratch that is cleared; all of it
    const char* why = "";
};

inline unsigned lists_tiles(int64_t n) { return (unsigned)((n + LISTS_TILE - 1) / LISTS_TILE); }
inline bool lists_aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

// one kind of a lists struct: every array its counts need is there and aligned
inline bool lists_kind_ok(const plslam_map_lists_kind& L, int32_t n, int32_t n_obs)
{
    if (!lists_aligned(L.desc, 16) || !lists_aligned(L.med_desc, 16) || !lists_aligned(L.pts, 16) || !lists_aligned(L.dir, 8) ||
        !lists_aligned(L.med_idx, 4))
        return false;
    return (n_obs == 0 || (L.desc && L.dir)) && (n == 0 || (L.med_idx && L.med_desc));
}

// plslam_map_lists_refresh
inline int lists_refresh_check(const plslam_map_index* map, const plslam_map_lists* lists, const char** why)
{
    *why = "";
    if (!map || !lists) { *why = "a NULL argument"; return PLSLAM_EINVAL; }
    const plslam_map_landmarks* M[2] = {&map->points, &map->lines};
    const plslam_map_lists_kind* L[2] = {&lists->points, &lists->lines};
    for (int k = 0; k < 2; ++k) {
        if (M[k]->n < 0 || M[k]->n_obs < 0 || M[k]->n_obs >= (1 << 30) || (M[k]->n > 0 && !M[k]->obs_ptr)) { *why = "the image's counts"; return PLSLAM_EINVAL; }
        if (!lists_kind_ok(*L[k], M[k]->n, M[k]->n_obs)) { *why = "a list pointer is missing or misaligned"; return PLSLAM_EINVAL; }
    }
    return PLSLAM_OK;
}

// plslam_map_insert_carry / plslam_lc_fuse_carry: R = the handle's records, rows[k] = the caller's rows of kind k (all NULL where
// it gave no struct).  On PLSLAM_OK *P holds the geometry and the scratch layout.
inline int lists_carry_plan(const ListsRecords& R, const plslam_map_index* src_map, const plslam_map_lists* src_lists,
                            const plslam_map_index* dst_map, const plslam_map_lists* dst_lists, const ListsRows rows[2], ListsPlan* P)
{
    *P = ListsPlan{};
#define LISTS_REFUSE(cond, text) do { if (cond) { P->why = text; return PLSLAM_EINVAL; } } while (0)
    LISTS_REFUSE(!src_map || !src_lists || !dst_map || !dst_lists, "a NULL argument");
    LISTS_REFUSE(!R.valid, "no successful insert / run on the handle");
    const plslam_map_landmarks *SM[2] = {&src_map->points, &src_map->lines}, *DM[2] = {&dst_map->points, &dst_map->lines};
    const plslam_map_lists_kind *SL[2] = {&src_lists->points, &src_lists->lines}, *DL[2] = {&dst_lists->points, &dst_lists->lines};
    for (int k = 0; k < 2; ++k) {
        const ListsKindRecords& r = R.k[k];
        LISTS_REFUSE(SM[k]->n != r.src_n || SM[k]->n_obs != r.src_obs, "src_map is not the image the handle's last call read");
        LISTS_REFUSE(DM[k]->n != r.dst_n || DM[k]->n_obs != r.dst_obs, "dst_map is not the image the handle's last call produced");
        LISTS_REFUSE(r.src_n < 0 || r.dst_n < r.src_n || r.src_obs < 0 || r.dst_obs < 0 || r.dst_obs >= (1 << 30), "the records' counts");
        LISTS_REFUSE((r.src_n > 0 && (!SM[k]->obs_ptr || !SM[k]->valid)) || (r.dst_n > 0 && (!DM[k]->obs_ptr || !DM[k]->valid)),
                     "an image without obs_ptr / valid");
        LISTS_REFUSE(!lists_kind_ok(*SL[k], r.src_n, r.src_obs), "a source list pointer is missing or misaligned");
        LISTS_REFUSE(!lists_kind_ok(*DL[k], r.dst_n, r.dst_obs), "a destination list pointer is missing or misaligned");
        LISTS_REFUSE(r.dst_obs > 0 && !r.obs_src, "the records hold no obs_src");
        const bool ev = r.n_ev > 0;
        LISTS_REFUSE(ev && (!r.dir || (r.ev_stride && !r.ev)), "the records hold no events");
        LISTS_REFUSE(ev && (!rows[k].desc[1] || (r.need_side0 && !rows[k].desc[0])), "a kind has events but lacks its rows");
        LISTS_REFUSE(!lists_aligned(rows[k].desc[0], 16) || !lists_aligned(rows[k].desc[1], 16) || !lists_aligned(rows[k].pts[0], 16) ||
                         !lists_aligned(rows[k].pts[1], 16), "a misaligned row pointer");
        ListsKindPlan& K = P->k[k];
        if (k == 1) {
            // pts: by all or by none (where the kind has no events the rows' pts are not looked at)
            const bool s = SL[k]->pts != nullptr, d = DL[k]->pts != nullptr;
            LISTS_REFUSE(s != d, "pts in one of src_lists / dst_lists only");
            if (ev) {
                const bool r1 = rows[k].pts[1] != nullptr, r0 = r.need_side0 ? rows[k].pts[0] != nullptr : r1;
                LISTS_REFUSE(r0 != r1 || r1 != d, "pts missing on one side");
            }
            K.with_pts = d;
        }
        // a destination list is never a source list (of either kind)
        const void* dp[] = {DL[k]->desc, DL[k]->dir, DL[k]->pts, DL[k]->med_idx, DL[k]->med_desc, DL[k]->refreshed};
        for (const void* p : dp) {
            if (!p) continue;
            for (int q = 0; q < 2; ++q) {
                const void* sp[] = {SL[q]->desc, SL[q]->dir, SL[q]->pts, SL[q]->med_idx, SL[q]->med_desc, SL[q]->refreshed};
                for (const void* x : sp) LISTS_REFUSE(p == x, "a destination list is a source list");
            }
        }
        K.src_n = r.src_n; K.src_obs = r.src_obs; K.dst_n = r.dst_n; K.dst_obs = r.dst_obs;
    }
#undef LISTS_REFUSE
    // ---- the geometry and the scratch: [cleared: per kind the two chains' words and the two counters] [per kind tl, toff] ----
    Carver c;
    for (int k = 0; k < 2; ++k) {
        ListsKindPlan& K = P->k[k];
        K.g_carry = K.dst_obs > 0 ? lists_tiles((int64_t)K.dst_obs * LISTS_LANES_PER_OBS) : 0;
        K.g_lm = K.dst_n > 0 ? lists_tiles(K.dst_n) : 0;
        K.g_rows = K.dst_n > 0 && K.dst_obs > 0 ? lists_tiles(K.dst_obs) : 0;
        K.o_part = c.take(2 * (size_t)K.g_lm * 4 + 4);
        K.o_cnt = c.take(2 * 4);
    }
    P->zero_bytes = c.off;
    for (int k = 0; k < 2; ++k) {
        ListsKindPlan& K = P->k[k];
        K.o_tl = c.take((size_t)K.dst_n * 4 + 4);
        K.o_toff = c.take((size_t)K.dst_n * 4 + 8);
    }
    P->scratch_bytes = c.off;
    return PLSLAM_OK;
}

// the records of a handle (nullptr for a NULL handle) and its context: map_insert.hip / lc_fuse.hip
const ListsRecords* map_insert_lists_records(plslam_map_insert* mi, plslam_ctx** ctx);
const ListsRecords* lc_fuse_lists_records(plslam_lc_fuse* lf, plslam_ctx** ctx);

}  // namespace plslam
