// map_insert_plan.hpp -- the pure host half of plslam_map_insert_kf2kf / _map2kf (map_insert.hip; the contract is in
// include/plslam_hip.h): every argument check, the growth bounds the tables give, the launch geometry, the layout of the handle's
// device buffer with its fill regions, and the packing of the call's tables into the block that is staged to the device.  No HIP
// in here: tests/cpp/test_map_insert_plan.cpp compiles it with the host compiler alone.
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstring>

#include "map_image.hpp"
#include "match_tables.hpp"   // Carver, align256
#include "plslam_hip.h"

namespace plslam {

enum { MAP_INSERT_KF2KF = 0, MAP_INSERT_MAP2KF = 1 };
constexpr int MAP_INSERT_COUNTER_WORDS = 8;      // the call counters: four per kind (map_insert.hip: W_WORDS)

struct MapInsertKindPlan {                       // one kind of one call
    const plslam_map_insert_kind* in = nullptr;  // nullptr: no table
    int32_t n_tab = 0, n_prev = 0, n_curr = 0;
    int32_t m = 0;                               // table entries >= 0: the bound on the events
    int32_t dl = 3, dv = 2;                      // doubles per feature position (3 / 6) and per observation (2 / 3)
    int64_t need_lm = 0, need_obs = 0;           // n + m (kf2kf) or n; n_obs + 2 m (kf2kf) or n_obs + m
    unsigned w_tab = 1, w_lm = 1;                // tiles of the table, of need_lm landmarks
    // the device buffer: zeroed (part: 3 w_tab + w_lm chain words) | 0x7f | staged | scratch | last
    size_t o_app = 0, o_win = 0, o_part = 0, o_head = 0;
    size_t o_tab = 0, o_P1 = 0, o_o1 = 0, o_P2 = 0, o_o2 = 0;
    size_t o_i1lm = 0, o_ev = 0, o_dir = 0, o_pair = 0, o_new = 0, o_osrc = 0;
};
struct MapInsertPlan {
    int32_t mode = 0, nk = 0, kf1 = -1, kf2 = 0;
    MapInsertKindPlan k[2];
    size_t o_cnt = 0, o_row = 0, o_T = 0;        // the counters, row_delta (zeroed); T_kf1_w, T_kf2_w (staged: 2 x 16 doubles)
    FillRegion fill[2] = {};                     // zero, then 0x7f (the heads: above every event number)
    size_t stage_off = 0, stage_bytes = 0;       // the staged block inside the device buffer
    size_t total = 0;                            // the end of the last slice
    size_t res_bytes = 0;                        // page-locked: the counters and row_delta the last kernel writes; the staged block follows
    const char* why = "";                        // what was refused
};

inline bool map_insert_kind_args_ok(const plslam_map_insert_kind* k, int mode)
{
    if (!k || !k->table || k->n_table == 0) return !k || k->n_table >= 0;
    if (k->n_table < 0 || k->n_curr < 0 || (k->n_curr > 0 && (!k->P2 || !k->obs2))) return false;
    return mode == MAP_INSERT_MAP2KF || (k->n_prev >= 0 && (k->n_prev == 0 || (k->P1 && k->obs1)));
}

// Validates everything the host can and fills the plan.  PLSLAM_OK, PLSLAM_EINVAL or PLSLAM_ERANGE (P->why says which rule).
inline int map_insert_plan(int mode, const plslam_map_index* src, const plslam_map_insert_dst* dst, int32_t kf1, int32_t kf2,
                           const double* T1, const double* T2, const plslam_map_insert_kind* points, const plslam_map_insert_kind* lines,
                           MapInsertPlan* P)
{
#define MI_REFUSE(cond, code, text) \
    do {                            \
        if (cond) {                 \
            P->why = text;          \
            return code;            \
        }                           \
    } while (0)
    *P = MapInsertPlan{};
    const bool kf2kf = mode == MAP_INSERT_KF2KF;
    MI_REFUSE(!src || !dst || !T2 || (kf2kf && !T1), PLSLAM_EINVAL, "a NULL argument");
    MI_REFUSE(src->n_map_kf < 1 || !src->kf_valid || !src->x_kf_w || !map_src_kind_ok(src->points) || !map_src_kind_ok(src->lines),
              PLSLAM_EINVAL, "the source image is incomplete");
    const int32_t nk = src->n_map_kf;
    MI_REFUSE(kf2 < 0 || kf2 >= nk || (kf2kf && (kf1 < 0 || kf1 >= nk || kf1 == kf2)), PLSLAM_EINVAL,
              "a keyframe slot is out of range, or kf1 == kf2");
    MI_REFUSE(!dst->map.kf_valid || !dst->map.x_kf_w || !map_dst_kind_ok(dst->map.points, src->points) ||
                  !map_dst_kind_ok(dst->map.lines, src->lines),
              PLSLAM_EINVAL, "a destination array is NULL or is a source array");
    MI_REFUSE(!map_insert_kind_args_ok(points, mode) || !map_insert_kind_args_ok(lines, mode), PLSLAM_EINVAL,
              "a kind with a table and a negative count or a NULL array");
    P->mode = mode; P->nk = nk; P->kf1 = kf2kf ? kf1 : -1; P->kf2 = kf2;
    const plslam_map_insert_kind* in[2] = {points, lines};
    const plslam_map_landmarks* S[2] = {&src->points, &src->lines};
    const int32_t cap[2] = {dst->pt_cap, dst->ls_cap}, obs_cap[2] = {dst->pt_obs_cap, dst->ls_obs_cap};
    for (int k = 0; k < 2; ++k) {
        MapInsertKindPlan& K = P->k[k];
        K.dl = k ? 6 : 3;
        K.dv = k ? 3 : 2;
        if (in[k] && in[k]->table && in[k]->n_table > 0) {
            K.in = in[k];
            K.n_tab = K.in->n_table; K.n_prev = kf2kf ? K.in->n_prev : 0; K.n_curr = K.in->n_curr;
            MI_REFUSE(!kf2kf && K.n_tab > S[k]->n, PLSLAM_EINVAL, "a map_to_kf table longer than the map");
            MI_REFUSE(kf2kf && K.n_tab > PLSLAM_MAP_INSERT_MAX_TABLE, PLSLAM_ERANGE, "a table beyond PLSLAM_MAP_INSERT_MAX_TABLE");
            for (int32_t i = 0; i < K.n_tab; ++i) K.m += K.in->table[i] >= 0;
        }
        K.need_lm = (int64_t)S[k]->n + (kf2kf ? K.m : 0);
        K.need_obs = (int64_t)S[k]->n_obs + (kf2kf ? 2 : 1) * (int64_t)K.m;
        MI_REFUSE(cap[k] < K.need_lm, PLSLAM_ERANGE, "a landmark capacity below what the table can add");
        MI_REFUSE(obs_cap[k] < K.need_obs, PLSLAM_ERANGE, "an observation capacity below what the table can add");
        MI_REFUSE(K.need_obs >= (1 << 30), PLSLAM_ERANGE, "n_obs beyond 2^30");
    }
#undef MI_REFUSE
    // ---- the layout: [zeroed: counters, row_delta, per kind app_cnt / feat_win / part] [0x7f: head] [staged] [the rest] [obs_src] ----
    Carver c;
    P->o_cnt = c.take(MAP_INSERT_COUNTER_WORDS * 4);
    P->o_row = c.take((size_t)nk * 4);
    for (int k = 0; k < 2; ++k) {
        MapInsertKindPlan& K = P->k[k];
        K.w_tab = map_tiles(K.n_tab);
        K.w_lm = map_tiles((int64_t)S[k]->n + K.m);
        K.o_app = c.take((size_t)S[k]->n * 4 + 4);
        K.o_win = c.take((size_t)K.n_curr * 4 + 4);
        K.o_part = c.take((3 * (size_t)K.w_tab + K.w_lm) * 4);
    }
    P->fill[0] = FillRegion{0, c.off, 0};
    for (int k = 0; k < 2; ++k) P->k[k].o_head = c.take((size_t)S[k]->n * 4 + 4);
    P->fill[1] = FillRegion{P->fill[0].bytes, c.off - P->fill[0].bytes, 0x7f};
    P->stage_off = c.off;
    P->o_T = c.take(32 * 8);
    for (int k = 0; k < 2; ++k) {
        MapInsertKindPlan& K = P->k[k];
        K.o_tab = c.take((size_t)K.n_tab * 4 + 4);
        K.o_P1 = c.take((size_t)K.n_prev * K.dl * 8 + 8);
        K.o_o1 = c.take((size_t)K.n_prev * K.dv * 8 + 8);
        K.o_P2 = c.take((size_t)K.n_curr * K.dl * 8 + 8);
        K.o_o2 = c.take((size_t)K.n_curr * K.dv * 8 + 8);
    }
    P->stage_bytes = c.off - P->stage_off;
    for (int k = 0; k < 2; ++k) {
        MapInsertKindPlan& K = P->k[k];
        const size_t m = (size_t)K.m;
        K.o_i1lm = c.take((size_t)K.n_tab * 4 + 4);
        K.o_ev = c.take(m * 16 + 16);
        K.o_dir = c.take(m * 48 + 48);
        K.o_pair = c.take(m * 4 + 4);
        K.o_new = c.take(m * 4 + 4);
    }
    for (int k = 0; k < 2; ++k) P->k[k].o_osrc = c.take((size_t)P->k[k].need_obs * 4 + 4);   // (behind everything else)
    P->total = c.off;
    P->res_bytes = align256((MAP_INSERT_COUNTER_WORDS + (size_t)nk) * 4);
    return PLSLAM_OK;
}

// Fills the staged block (P.stage_bytes bytes at `staged`; its offsets are the device layout's, from P.stage_off) from the
// caller's arrays.  T1: NULL in map <-> KF mode, its 16 doubles stay zero.
inline void map_insert_pack(const MapInsertPlan& P, const double* T1, const double* T2, char* staged)
{
    const auto to = [&](size_t o) { return staged + (o - P.stage_off); };
    memset(staged, 0, P.stage_bytes);
    if (T1) memcpy(to(P.o_T), T1, 128);
    memcpy(to(P.o_T) + 128, T2, 128);
    for (int k = 0; k < 2; ++k) {
        const MapInsertKindPlan& K = P.k[k];
        if (!K.in) continue;
        memcpy(to(K.o_tab), K.in->table, (size_t)K.n_tab * 4);
        if (K.n_prev) {
            memcpy(to(K.o_P1), K.in->P1, (size_t)K.n_prev * K.dl * 8);
            memcpy(to(K.o_o1), K.in->obs1, (size_t)K.n_prev * K.dv * 8);
        }
        if (K.n_curr) {
            memcpy(to(K.o_P2), K.in->P2, (size_t)K.n_curr * K.dl * 8);
            memcpy(to(K.o_o2), K.in->obs2, (size_t)K.n_curr * K.dv * 8);
        }
    }
}

}  // namespace plslam
