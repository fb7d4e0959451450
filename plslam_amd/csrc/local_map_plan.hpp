// local_map_plan.hpp -- the pure host part of the plslam_local_map_* calls (local_map.hip; the contract is in include/plslam_hip.h):
// the counter words, the image check, the carving of the handle's buffer, the handle's state with the check every entry point
// makes and the transitions it goes through, and the one table of the buffers a caller sees.  No HIP in here:
// tests/cpp/test_local_map_plan.cpp compiles it with the host compiler alone.
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstring>

#include "map_image.hpp"
#include "match_tables.hpp"   // Carver
#include "plslam_hip.h"

namespace plslam {

// the call counters (device words, mirrored in the page-locked block): plslam_local_map_counts' order, then the tickets
enum { C_KF_LOCAL = 0, C_PT_LOCAL, C_LS_LOCAL, C_NKF, C_NPT, C_NLS, C_PT_OBS, C_LS_OBS, C_PT_REM, C_LS_REM, C_CULL_DONE, C_FORM_DONE, C_PT_MOVED, C_LS_MOVED, C_APPLY_DONE, C_WORDS = 16 };

// an image the local-map calls read: complete, and X_aux's 6 nk + 3 np + 6 nl doubles are indexed by an int32
inline bool local_map_image_ok(const plslam_map_index* m)
{
    return m && m->n_map_kf >= 1 && m->kf_valid && m->x_kf_w && map_src_kind_ok(m->points) && map_src_kind_ok(m->lines) &&
           6 * (int64_t)m->n_map_kf + 3 * (int64_t)m->points.n + 6 * (int64_t)m->lines.n < (int64_t)1 << 31;
}

// the five counts of an image a handle's buffer is carved for
struct LocalMapSizes {
    int32_t n_map_kf = 0, npt = 0, nls = 0, n_pt_obs = 0, n_ls_obs = 0;
    bool operator==(const LocalMapSizes& o) const
    {
        return n_map_kf == o.n_map_kf && npt == o.npt && nls == o.nls && n_pt_obs == o.n_pt_obs && n_ls_obs == o.n_ls_obs;
    }
};
inline LocalMapSizes local_map_sizes(const plslam_map_index& m)
{
    return LocalMapSizes{m.n_map_kf, m.points.n, m.lines.n, m.points.n_obs, m.lines.n_obs};
}

// The slices of the handle's buffer, in the order they are carved.  LM_KF_LOCAL ... LM_CNT are the cleared front: the flags and
// the counters, cleared by form in one go.  LM_PT_OFF / LM_LS_OFF: the listed landmarks' observation offsets (n + 1 words).
enum LocalMapSlot {
    LM_KF_LOCAL = 0, LM_PT_LOCAL, LM_LS_LOCAL, LM_CNT,
    LM_PT_CANDIDATE, LM_LS_CANDIDATE, LM_PT_REMOVED, LM_LS_REMOVED, LM_PT_MOVED, LM_LS_MOVED,
    LM_KF_LIST, LM_KF_INV, LM_ROW, LM_PT_LIST, LM_LS_LIST, LM_PT_OFF, LM_LS_OFF, LM_PT_OBS, LM_LS_OBS,
    LM_PT_LM_LOC, LM_PT_KF_LOC, LM_PT_POSE_SLOT, LM_LS_LM_LOC, LM_LS_KF_LOC, LM_LS_POSE_SLOT,
    LM_PT_OBS_UV, LM_LS_L_OBS, LM_X_AUX, LM_PART, LM_SLOTS
};
// the five look-back chains inside LM_PART: map_tiles(n) words each
enum { LM_CHAIN_KF = 0, LM_CHAIN_PT, LM_CHAIN_PT_OBS, LM_CHAIN_LS, LM_CHAIN_LS_OBS, LM_CHAINS };

struct LocalMapLayout {
    size_t off[LM_SLOTS] = {}, bytes[LM_SLOTS] = {};     // bytes: what the slice holds (the carver pads it to 256)
    size_t zero_bytes = 0;                               // the cleared front, from offset 0 to the end of LM_CNT's slice
    size_t chain_off[LM_CHAINS] = {}, chain_words[LM_CHAINS] = {}, part_words = 0;       // chain_off: in words, inside LM_PART
    size_t total = 0;                                    // the end of the last slice
    size_t pin_bytes = 0;                                // page-locked: the counters, then the staged graph row

    explicit LocalMapLayout(const LocalMapSizes& z = LocalMapSizes{})
    {
        const size_t nk = (size_t)z.n_map_kf, np = (size_t)z.npt, nl = (size_t)z.nls, op = (size_t)z.n_pt_obs, ol = (size_t)z.n_ls_obs;
        const size_t tiles[LM_CHAINS] = {map_tiles((int64_t)nk), map_tiles((int64_t)np), map_tiles((int64_t)np), map_tiles((int64_t)nl),
                                         map_tiles((int64_t)nl)};
        for (int c = 0; c < LM_CHAINS; ++c) {
            chain_off[c] = part_words;
            chain_words[c] = tiles[c];
            part_words += tiles[c];
        }
        bytes[LM_KF_LOCAL] = nk; bytes[LM_PT_LOCAL] = np; bytes[LM_LS_LOCAL] = nl; bytes[LM_CNT] = C_WORDS * 4;
        bytes[LM_PT_CANDIDATE] = bytes[LM_PT_REMOVED] = bytes[LM_PT_MOVED] = np;
        bytes[LM_LS_CANDIDATE] = bytes[LM_LS_REMOVED] = bytes[LM_LS_MOVED] = nl;
        bytes[LM_KF_LIST] = bytes[LM_KF_INV] = bytes[LM_ROW] = nk * 4;
        bytes[LM_PT_LIST] = np * 4; bytes[LM_LS_LIST] = nl * 4; bytes[LM_PT_OFF] = (np + 1) * 4; bytes[LM_LS_OFF] = (nl + 1) * 4;
        bytes[LM_PT_OBS] = op * 24; bytes[LM_LS_OBS] = ol * 24;
        bytes[LM_PT_LM_LOC] = bytes[LM_PT_KF_LOC] = bytes[LM_PT_POSE_SLOT] = op * 4;
        bytes[LM_LS_LM_LOC] = bytes[LM_LS_KF_LOC] = bytes[LM_LS_POSE_SLOT] = ol * 4;
        bytes[LM_PT_OBS_UV] = op * 16; bytes[LM_LS_L_OBS] = ol * 24; bytes[LM_X_AUX] = (6 * nk + 3 * np + 6 * nl) * 8;
        bytes[LM_PART] = part_words * 4;
        Carver c;
        for (int s = 0; s < LM_SLOTS; ++s) {
            off[s] = c.take(bytes[s]);
            if (s == LM_CNT) zero_bytes = c.off;
        }
        total = c.off;
        pin_bytes = (C_WORDS + nk) * 4;
    }
};

// ---- the buffers a caller sees (plslam_local_map_buffers): each named once ------------------------------------------------------
// what scales a buffer's download: a count of the image the handle was formed on, or a count of the last gather
enum LocalMapScale { LM_BY_MAP_KF, LM_BY_MAP_PT, LM_BY_MAP_LS, LM_BY_NKF, LM_BY_NPT, LM_BY_NLS, LM_BY_PT_OBS, LM_BY_LS_OBS, LM_BY_X_AUX };
// the call a buffer's download needs to have run
enum LocalMapAfter { LM_AFTER_FORM, LM_AFTER_GATHER, LM_AFTER_APPLY };
struct LocalMapBuffer {
    size_t field;                        // offsetof(plslam_local_map_buffers, <member>): every member is one pointer
    LocalMapSlot slot;
    size_t elem_bytes;                   // per unit of `scale`
    LocalMapScale scale;
    LocalMapAfter after;
};
#define LM_BUF(member, slot, elem, scale, after) {offsetof(plslam_local_map_buffers, member), slot, elem, scale, after}
constexpr LocalMapBuffer LOCAL_MAP_BUFFERS[] = {
    LM_BUF(kf_local, LM_KF_LOCAL, 1, LM_BY_MAP_KF, LM_AFTER_FORM),
    LM_BUF(pt_local, LM_PT_LOCAL, 1, LM_BY_MAP_PT, LM_AFTER_FORM),
    LM_BUF(ls_local, LM_LS_LOCAL, 1, LM_BY_MAP_LS, LM_AFTER_FORM),
    LM_BUF(pt_candidate, LM_PT_CANDIDATE, 1, LM_BY_MAP_PT, LM_AFTER_FORM),
    LM_BUF(ls_candidate, LM_LS_CANDIDATE, 1, LM_BY_MAP_LS, LM_AFTER_FORM),
    LM_BUF(pt_removed, LM_PT_REMOVED, 1, LM_BY_MAP_PT, LM_AFTER_FORM),
    LM_BUF(ls_removed, LM_LS_REMOVED, 1, LM_BY_MAP_LS, LM_AFTER_FORM),
    LM_BUF(kf_list, LM_KF_LIST, 4, LM_BY_NKF, LM_AFTER_GATHER),
    LM_BUF(pt_list, LM_PT_LIST, 4, LM_BY_NPT, LM_AFTER_GATHER),
    LM_BUF(ls_list, LM_LS_LIST, 4, LM_BY_NLS, LM_AFTER_GATHER),
    LM_BUF(pt_obs, LM_PT_OBS, 24, LM_BY_PT_OBS, LM_AFTER_GATHER),
    LM_BUF(ls_obs, LM_LS_OBS, 24, LM_BY_LS_OBS, LM_AFTER_GATHER),
    LM_BUF(pt_lm_loc, LM_PT_LM_LOC, 4, LM_BY_PT_OBS, LM_AFTER_GATHER),
    LM_BUF(pt_kf_loc, LM_PT_KF_LOC, 4, LM_BY_PT_OBS, LM_AFTER_GATHER),
    LM_BUF(pt_pose_slot, LM_PT_POSE_SLOT, 4, LM_BY_PT_OBS, LM_AFTER_GATHER),
    LM_BUF(ls_lm_loc, LM_LS_LM_LOC, 4, LM_BY_LS_OBS, LM_AFTER_GATHER),
    LM_BUF(ls_kf_loc, LM_LS_KF_LOC, 4, LM_BY_LS_OBS, LM_AFTER_GATHER),
    LM_BUF(ls_pose_slot, LM_LS_POSE_SLOT, 4, LM_BY_LS_OBS, LM_AFTER_GATHER),
    LM_BUF(pt_obs_uv, LM_PT_OBS_UV, 16, LM_BY_PT_OBS, LM_AFTER_GATHER),
    LM_BUF(ls_l_obs, LM_LS_L_OBS, 24, LM_BY_LS_OBS, LM_AFTER_GATHER),
    LM_BUF(X_aux, LM_X_AUX, 8, LM_BY_X_AUX, LM_AFTER_GATHER),
    LM_BUF(pt_moved, LM_PT_MOVED, 1, LM_BY_NPT, LM_AFTER_APPLY),
    LM_BUF(ls_moved, LM_LS_MOVED, 1, LM_BY_NLS, LM_AFTER_APPLY),
};
#undef LM_BUF
constexpr int LOCAL_MAP_N_BUFFERS = (int)(sizeof(LOCAL_MAP_BUFFERS) / sizeof(LOCAL_MAP_BUFFERS[0]));

// the pointer member of the struct a table row names
inline void* local_map_buffer_get(const plslam_local_map_buffers& b, const LocalMapBuffer& e)
{
    void* p;
    memcpy(&p, (const char*)&b + e.field, sizeof p);
    return p;
}
inline void local_map_buffer_set(plslam_local_map_buffers& b, const LocalMapBuffer& e, void* p)
{
    memcpy((char*)&b + e.field, &p, sizeof p);
}
// the struct of device pointers: every buffer at its slice of the handle's buffer
inline void local_map_fill_buffers(plslam_local_map_buffers& b, const LocalMapLayout& L, char* base, void* stream)
{
    for (const LocalMapBuffer& e : LOCAL_MAP_BUFFERS) local_map_buffer_set(b, e, base + L.off[e.slot]);
    b.stream = stream;
}

// ---- the handle's state: what has run on it, on which image, with which counts -------------------------------------------------
struct LocalMapState {
    LocalMapSizes z;                             // the image of the last form
    bool formed = false, gathered = false, applied = false;
    int32_t h_cnt[C_WORDS] = {};                 // the counts of the last calls (download sizes)

    bool same_map(const plslam_map_index* m) const { return formed && z == local_map_sizes(*m); }

    // -- one check per entry point (the handle itself is the entry point's to test): the code the call returns --
    static int check_form(const plslam_map_index* map, int32_t anchor_kf, const int32_t* row, const plslam_local_map_counts* counts)
    {
        return local_map_image_ok(map) && row && counts && anchor_kf >= 0 && anchor_kf < map->n_map_kf ? PLSLAM_OK : PLSLAM_EINVAL;
    }
    static int check_form_all(const plslam_map_index* map, const plslam_local_map_counts* counts)
    {
        return local_map_image_ok(map) && counts ? PLSLAM_OK : PLSLAM_EINVAL;
    }
    int check_candidates(const plslam_map_index* map) const { return local_map_image_ok(map) && same_map(map) ? PLSLAM_OK : PLSLAM_EINVAL; }
    int check_gather(const plslam_map_index* map, const plslam_local_map_counts* counts) const
    {
        return local_map_image_ok(map) && counts && same_map(map) ? PLSLAM_OK : PLSLAM_EINVAL;
    }
    int check_cull(const plslam_map_index* map, const plslam_local_map_counts* counts) const { return check_gather(map, counts); }
    // the plan's facts as plain values: its context is the handle's, its list lengths, its state resident (no plan type in here)
    int check_apply_lba(bool same_ctx, int32_t plan_npt, int32_t plan_nls, bool state_valid, const plslam_local_map_lba_dst* dst,
                        const plslam_local_map_counts* counts) const
    {
        if (!dst || !counts || !same_ctx || !formed || !gathered) return PLSLAM_EINVAL;
        const int32_t npt_l = h_cnt[C_NPT], nls_l = h_cnt[C_NLS];
        if (plan_npt != npt_l || plan_nls != nls_l || !state_valid) return PLSLAM_EINVAL;
        return (npt_l == 0 || (dst->pt_X && dst->pt_inlier)) && (nls_l == 0 || (dst->ls_X && dst->ls_inlier)) ? PLSLAM_OK : PLSLAM_EINVAL;
    }
    // (the write-back of the global BA copies only: dst's inlier pointers are not looked at)
    int check_apply_gba(bool same_ctx, int32_t plan_npt, int32_t plan_nls, bool optimized, const plslam_local_map_lba_dst* dst) const
    {
        if (!dst || !same_ctx || !formed || !gathered) return PLSLAM_EINVAL;
        const int32_t npt_l = h_cnt[C_NPT], nls_l = h_cnt[C_NLS];
        if (plan_npt != npt_l || plan_nls != nls_l || !optimized) return PLSLAM_EINVAL;
        return (npt_l == 0 || dst->pt_X) && (nls_l == 0 || dst->ls_X) ? PLSLAM_OK : PLSLAM_EINVAL;
    }
    int check_device_buffers(const plslam_local_map_buffers* out) const { return out && formed ? PLSLAM_OK : PLSLAM_EINVAL; }
    // a list needs the gather, a moved mask the write-back: by the table
    int check_download(const plslam_local_map_buffers* host) const
    {
        if (!host || !formed) return PLSLAM_EINVAL;
        for (const LocalMapBuffer& e : LOCAL_MAP_BUFFERS) {
            if (!local_map_buffer_get(*host, e)) continue;
            if ((e.after == LM_AFTER_GATHER && !gathered) || (e.after == LM_AFTER_APPLY && !applied)) return PLSLAM_EINVAL;
        }
        return PLSLAM_OK;
    }

    // -- the transitions: what a call clears before it runs, what it sets after success --
    void begin_form(const plslam_map_index& map)
    {
        formed = gathered = applied = false;
        z = local_map_sizes(map);
    }
    void end_form(const int32_t* pinned, plslam_local_map_counts* counts)
    {
        memset(h_cnt, 0, sizeof h_cnt);
        for (int k = C_KF_LOCAL; k <= C_LS_LOCAL; ++k) h_cnt[k] = pinned[k];
        counts->n_kf_local = h_cnt[C_KF_LOCAL]; counts->n_pt_local = h_cnt[C_PT_LOCAL]; counts->n_ls_local = h_cnt[C_LS_LOCAL];
        formed = true;
    }
    void begin_gather() { gathered = applied = false; }
    void end_gather(const int32_t* pinned, plslam_local_map_counts* counts)
    {
        for (int k = C_NKF; k <= C_LS_OBS; ++k) h_cnt[k] = pinned[k];
        counts->nkf = h_cnt[C_NKF]; counts->npt = h_cnt[C_NPT]; counts->nls = h_cnt[C_NLS];
        counts->n_pt_obs = h_cnt[C_PT_OBS]; counts->n_ls_obs = h_cnt[C_LS_OBS];
        counts->empty = (int64_t)h_cnt[C_PT_OBS] + h_cnt[C_LS_OBS] == 0;
        gathered = true;
    }
    void begin_cull(plslam_local_map_counts* counts) { counts->n_pt_removed = counts->n_ls_removed = h_cnt[C_PT_REM] = h_cnt[C_LS_REM] = 0; }
    void end_cull(const int32_t* pinned, plslam_local_map_counts* counts)
    {
        counts->n_pt_removed = h_cnt[C_PT_REM] = pinned[C_PT_REM];
        counts->n_ls_removed = h_cnt[C_LS_REM] = pinned[C_LS_REM];
    }
    // (applied before the launch: a write-back of two empty lists launches nothing and has run all the same)
    void begin_apply_lba(plslam_local_map_counts* counts)
    {
        counts->n_pt_moved = counts->n_ls_moved = h_cnt[C_PT_MOVED] = h_cnt[C_LS_MOVED] = 0;
        applied = true;
    }
    void end_apply_lba(const int32_t* pinned, plslam_local_map_counts* counts)
    {
        counts->n_pt_moved = h_cnt[C_PT_MOVED] = pinned[C_PT_MOVED];
        counts->n_ls_moved = h_cnt[C_LS_MOVED] = pinned[C_LS_MOVED];
    }

    // the bytes a download of one buffer copies
    size_t download_bytes(const LocalMapBuffer& e) const
    {
        const size_t nkf = (size_t)h_cnt[C_NKF], npt = (size_t)h_cnt[C_NPT], nls = (size_t)h_cnt[C_NLS];
        size_t n = 0;
        switch (e.scale) {
        case LM_BY_MAP_KF: n = (size_t)z.n_map_kf; break;
        case LM_BY_MAP_PT: n = (size_t)z.npt; break;
        case LM_BY_MAP_LS: n = (size_t)z.nls; break;
        case LM_BY_NKF: n = nkf; break;
        case LM_BY_NPT: n = npt; break;
        case LM_BY_NLS: n = nls; break;
        case LM_BY_PT_OBS: n = (size_t)h_cnt[C_PT_OBS]; break;
        case LM_BY_LS_OBS: n = (size_t)h_cnt[C_LS_OBS]; break;
        case LM_BY_X_AUX: n = 6 * nkf + 3 * npt + 6 * nls; break;
        }
        return n * e.elem_bytes;
    }
};

}  // namespace plslam
