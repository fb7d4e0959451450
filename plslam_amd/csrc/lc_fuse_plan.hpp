// lc_fuse_plan.hpp -- the pure host half of plslam_lc_fuse_run (lc_fuse.hip): the validation of the arguments, the growth bounds
// the tuples alone give, the layout of the handle's device buffer with its fill regions, and the packing of the call's tables into
// the one block that is staged to the device.  No HIP in here: tests/cpp/test_lc_fuse_pack.cpp compiles it on its own and runs it
// under the sanitizers.
#pragma once

#include <cstdint>
#include <cstring>

#include "map_image.hpp"
#include "match_tables.hpp"   // Carver, align256
#include "plslam_hip.h"

namespace plslam {

constexpr int LC_FUSE_COUNTER_WORDS = 20;        // the call counters: eight per kind, then the status word (lc_fuse.hip: W_WORDS)

struct LcFuseKindPlan {
    const plslam_lc_fuse_kind* in = nullptr;     // nullptr: no tuple of this kind
    int32_t m = 0, cC = 0, cAB = 0;              // tuples; among those of flagged entries: (-1, -1), exactly one -1
    int32_t dl = 3, dv = 2;                      // doubles per feature position (3 / 6) and per observation (2 / 3)
    int64_t need_lm = 0, need_obs = 0;
    size_t o_tup = 0, o_eptr = 0, o_P0 = 0, o_o0 = 0, o_P1 = 0, o_o1 = 0;      // in the staged block
    // the device buffer: zeroed (win, part: w_lm chain words) | 0x7f (head) | 0xff (killer) | behind the staged block the rest
    unsigned w_lm = 1;                           // tiles of need_lm landmarks
    size_t d_win = 0, d_part = 0, d_head = 0, d_killer = 0;
    size_t d_len = 0, d_sc = 0, d_fw0 = 0, d_fw1 = 0, d_ev = 0, d_off = 0, d_pair = 0, d_nev = 0, d_dir = 0, d_osrc = 0;
};
struct LcFusePlan {
    int32_t n_lc = 0, nk = 0;
    LcFuseKindPlan k[2];
    size_t o_lc = 0, o_T = 0, stage_bytes = 0;
    size_t d_cnt = 0, d_graph = 0;               // the device buffer: the counters, the dense nk x nk graph delta (zeroed)
    FillRegion fill[3] = {};                     // zero, 0x7f (the heads: above every event number), 0xff (the killers: -1)
    size_t stage_off = 0;                        // the staged block inside the device buffer
    size_t total = 0;                            // the end of the last slice
    const char* why = "";                        // what was refused
    // page-locked: the counters, the graph where the caller asked for it; the staged block follows
    size_t res_bytes(bool with_graph) const { return align256((LC_FUSE_COUNTER_WORDS + (with_graph ? (size_t)nk * nk : 0)) * 4); }
};

inline size_t lc_fuse_align(size_t bytes) { return (bytes + 255) & ~(size_t)255; }

// Validates everything the host can and fills the plan.  PLSLAM_OK, PLSLAM_EINVAL or PLSLAM_ERANGE (P->why says which rule).
inline int lc_fuse_plan(const plslam_map_index* src, const plslam_map_insert_dst* dst, int32_t n_lc, const int32_t* lc_idx,
                        const double* T_kf_w, const plslam_lc_fuse_kind* points, const plslam_lc_fuse_kind* lines, LcFusePlan* P)
{
#define LCF_REFUSE(cond, code, text) \
    do {                             \
        if (cond) {                  \
            P->why = text;           \
            return code;             \
        }                            \
    } while (0)
    LCF_REFUSE(!src || !dst || !lc_idx || !T_kf_w, PLSLAM_EINVAL, "a NULL argument");
    LCF_REFUSE(n_lc <= 0, PLSLAM_EINVAL, "n_lc <= 0");
    LCF_REFUSE(src->n_map_kf < 1 || !src->kf_valid || !src->x_kf_w || !map_src_kind_ok(src->points) || !map_src_kind_ok(src->lines),
               PLSLAM_EINVAL, "the source image is incomplete");
    LCF_REFUSE((int64_t)src->n_map_kf * src->n_map_kf >= (1 << 28), PLSLAM_ERANGE, "n_map_kf^2 beyond 2^28");
    LCF_REFUSE(!dst->map.kf_valid || !dst->map.x_kf_w || !map_dst_kind_ok(dst->map.points, src->points) ||
                   !map_dst_kind_ok(dst->map.lines, src->lines),
               PLSLAM_EINVAL, "a destination array is NULL or is a source array");
    const int32_t nk = src->n_map_kf;
    for (int32_t i = 0; i < n_lc; ++i) {
        const int32_t kp = lc_idx[3 * i], kc = lc_idx[3 * i + 1];
        if (lc_idx[3 * i + 2] != 1) continue;                    // already optimised: contributes nothing, names nothing
        LCF_REFUSE(kp < 0 || kp >= nk || kc < 0 || kc >= nk, PLSLAM_EINVAL, "an entry's slot is out of range");
        LCF_REFUSE(kp == kc, PLSLAM_EINVAL, "an entry with kf_prev == kf_curr");
    }
    P->n_lc = n_lc;
    P->nk = nk;
    const plslam_lc_fuse_kind* in[2] = {points, lines};
    const plslam_map_landmarks* S[2] = {&src->points, &src->lines};
    const int32_t cap[2] = {dst->pt_cap, dst->ls_cap}, obs_cap[2] = {dst->pt_obs_cap, dst->ls_obs_cap};
    for (int k = 0; k < 2; ++k) {
        LcFuseKindPlan& K = P->k[k];
        K = LcFuseKindPlan();
        K.dl = k ? 6 : 3;
        K.dv = k ? 3 : 2;
        if (in[k] && in[k]->entry_ptr) {
            const int32_t* ep = in[k]->entry_ptr;
            LCF_REFUSE(ep[0] != 0, PLSLAM_EINVAL, "entry_ptr[0] != 0");
            for (int32_t i = 0; i < n_lc; ++i) LCF_REFUSE(ep[i + 1] < ep[i], PLSLAM_EINVAL, "entry_ptr decreases");
            LCF_REFUSE(ep[n_lc] > PLSLAM_LC_FUSE_MAX_TUPLES, PLSLAM_ERANGE, "more than PLSLAM_LC_FUSE_MAX_TUPLES tuples");
            K.m = ep[n_lc];
            if (K.m > 0) {
                LCF_REFUSE(!in[k]->tuples || !in[k]->P0 || !in[k]->obs0 || !in[k]->P1 || !in[k]->obs1, PLSLAM_EINVAL,
                           "a kind with tuples and a NULL array");
                K.in = in[k];
                for (int32_t i = 0; i < n_lc; ++i) {
                    if (lc_idx[3 * i + 2] != 1) continue;
                    for (int32_t t = ep[i]; t < ep[i + 1]; ++t) {
                        const bool a = K.in->tuples[4 * (size_t)t] == -1, b = K.in->tuples[4 * (size_t)t + 2] == -1;
                        K.cC += a && b;
                        K.cAB += a != b;
                    }
                }
            }
        }
        K.need_lm = (int64_t)S[k]->n + K.cC;
        K.need_obs = (int64_t)S[k]->n_obs + K.cAB + 2 * (int64_t)K.cC;
        LCF_REFUSE(K.need_obs >= (1 << 30), PLSLAM_ERANGE, "n_obs beyond 2^30");
        LCF_REFUSE(cap[k] < K.need_lm, PLSLAM_ERANGE, "a landmark capacity below n + cC");
        LCF_REFUSE(obs_cap[k] < K.need_obs, PLSLAM_ERANGE, "an observation capacity below n_obs + cAB + 2 cC");
    }
#undef LCF_REFUSE
    // the staged block: lc_idx, T_kf_w, then per kind the tuples, entry_ptr and the four feature arrays
    size_t off = 0;
    auto take = [&off](size_t bytes) { const size_t o = off; off += lc_fuse_align(bytes); return o; };
    P->o_lc = take((size_t)n_lc * 12);
    P->o_T = take((size_t)nk * 128);
    for (int k = 0; k < 2; ++k) {
        LcFuseKindPlan& K = P->k[k];
        K.o_tup = take((size_t)K.m * 16 + 16);
        K.o_eptr = take(((size_t)n_lc + 1) * 4);
        K.o_P0 = take((size_t)K.m * K.dl * 8 + 8);
        K.o_o0 = take((size_t)K.m * K.dv * 8 + 8);
        K.o_P1 = take((size_t)K.m * K.dl * 8 + 8);
        K.o_o1 = take((size_t)K.m * K.dv * 8 + 8);
    }
    P->stage_bytes = off;
    // ---- the device layout: [zeroed: counters, graph, per kind feat_win / part] [0x7f: head] [0xff: killer] [staged] [the rest] ----
    Carver c;
    P->d_cnt = c.take(LC_FUSE_COUNTER_WORDS * 4);
    P->d_graph = c.take((size_t)nk * nk * 4);
    for (int k = 0; k < 2; ++k) {
        LcFuseKindPlan& K = P->k[k];
        K.w_lm = map_tiles(K.need_lm);
        K.d_win = c.take((size_t)S[k]->n_feat * 4 + 4);
        K.d_part = c.take((size_t)K.w_lm * 4);
    }
    P->fill[0] = FillRegion{0, c.off, 0};
    for (int k = 0; k < 2; ++k) P->k[k].d_head = c.take((size_t)S[k]->n * 4 + 4);
    P->fill[1] = FillRegion{P->fill[0].bytes, c.off - P->fill[0].bytes, 0x7f};
    for (int k = 0; k < 2; ++k) P->k[k].d_killer = c.take((size_t)S[k]->n * 4 + 4);
    P->fill[2] = FillRegion{P->fill[1].off + P->fill[1].bytes, c.off - (P->fill[1].off + P->fill[1].bytes), 0xff};
    P->stage_off = c.take(P->stage_bytes);
    for (int k = 0; k < 2; ++k) {
        LcFuseKindPlan& K = P->k[k];
        const size_t m = (size_t)K.m;
        K.d_len = c.take((size_t)K.need_lm * 4 + 4);
        K.d_sc = c.take(m * 4 + 4); K.d_fw0 = c.take(m * 4 + 4); K.d_fw1 = c.take(m * 4 + 4);
        K.d_ev = c.take(m * 24 + 24); K.d_off = c.take(m * 4 + 4); K.d_pair = c.take(m * 4 + 8);
        K.d_nev = c.take((size_t)K.cC * 4 + 4); K.d_dir = c.take(m * 48 + 48);
        K.d_osrc = c.take((size_t)obs_cap[k] * 4 + 4);       // (the destination's capacity: K71 clamps to it)
    }
    P->total = c.off;
    return PLSLAM_OK;
}

// Fills the staged block (P.stage_bytes bytes at `stage`) from the caller's arrays; a kind without tuples gets an all-zero
// entry_ptr.
inline void lc_fuse_pack(const LcFusePlan& P, const int32_t* lc_idx, const double* T_kf_w, char* stage)
{
    memset(stage, 0, P.stage_bytes);
    memcpy(stage + P.o_lc, lc_idx, (size_t)P.n_lc * 12);
    memcpy(stage + P.o_T, T_kf_w, (size_t)P.nk * 128);
    for (int k = 0; k < 2; ++k) {
        const LcFuseKindPlan& K = P.k[k];
        if (!K.in) continue;
        const size_t m = (size_t)K.m;
        memcpy(stage + K.o_tup, K.in->tuples, m * 16);
        memcpy(stage + K.o_eptr, K.in->entry_ptr, ((size_t)P.n_lc + 1) * 4);
        memcpy(stage + K.o_P0, K.in->P0, m * K.dl * 8);
        memcpy(stage + K.o_o0, K.in->obs0, m * K.dv * 8);
        memcpy(stage + K.o_P1, K.in->P1, m * K.dl * 8);
        memcpy(stage + K.o_o1, K.in->obs1, m * K.dv * 8);
    }
}

}  // namespace plslam
