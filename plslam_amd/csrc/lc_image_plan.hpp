// lc_image_plan.hpp -- the pure host half of plslam_lc_correct_image (lc_correct_image.hip): the validation of the arguments and
// the packing of T_corr, the corrected flags and the new x_kf_w rows into the one block that is staged to the device.  No HIP in
// here: tests/cpp/test_lc_image_plan.cpp compiles it on its own and runs it under the sanitizers.
#pragma once

#include <cstdint>
#include <cstring>

#include "map_image.hpp"
#include "plslam_hip.h"

namespace plslam {

struct LcImagePlan {
    int32_t nk = 0;
    bool with_x = false;                         // x_kf_w_new and dst->x_kf_w are both given: corrected slots take their new row
    bool with_dir[2] = {false, false}, with_med[2] = {false, false};
    size_t o_T = 0, o_x = 0, o_corr = 0, stage_bytes = 0;      // in the staged block
    const char* why = "";                        // what was refused
};

inline size_t lc_image_align(size_t bytes) { return (bytes + 255) & ~(size_t)255; }
inline bool lc_image_aligned8(const void* p) { return ((uintptr_t)p & 7) == 0; }

// Validates everything the host can and fills the plan.  PLSLAM_OK or PLSLAM_EINVAL (P->why says which rule).
inline int lc_image_plan(const plslam_map_index* map, const double* T_corr, const uint8_t* corrected, const double* x_kf_w_new,
                         const plslam_lc_image_dst* dst, LcImagePlan* P)
{
#define LCI_REFUSE(cond, text)       \
    do {                             \
        if (cond) {                  \
            P->why = text;           \
            return PLSLAM_EINVAL;    \
        }                            \
    } while (0)
    *P = LcImagePlan();
    LCI_REFUSE(!map || !T_corr || !corrected || !dst, "a NULL argument");
    LCI_REFUSE(map->n_map_kf < 1, "n_map_kf < 1");
    LCI_REFUSE(!map_src_kind_ok(map->points) || !map_src_kind_ok(map->lines), "the image is incomplete");
    LCI_REFUSE((map->points.n > 0 && !dst->pt_X) || (map->lines.n > 0 && !dst->ls_X), "a kind with landmarks and a NULL X");
    const void* d[] = {dst->pt_X, dst->pt_dir, dst->pt_med_dir, dst->ls_X, dst->ls_dir, dst->ls_med_dir, dst->x_kf_w};
    for (const void* p : d) LCI_REFUSE(!lc_image_aligned8(p), "a destination array is not 8-byte aligned");
#undef LCI_REFUSE
    P->nk = map->n_map_kf;
    P->with_x = x_kf_w_new && dst->x_kf_w;
    P->with_dir[0] = dst->pt_dir && map->points.n_obs > 0;
    P->with_dir[1] = dst->ls_dir && map->lines.n_obs > 0;
    P->with_med[0] = dst->pt_med_dir && map->points.n > 0;
    P->with_med[1] = dst->ls_med_dir && map->lines.n > 0;
    size_t off = 0;
    auto take = [&off](size_t bytes) { const size_t o = off; off += lc_image_align(bytes); return o; };
    P->o_T = take((size_t)P->nk * 128);
    P->o_x = take(P->with_x ? (size_t)P->nk * 48 : 0);
    P->o_corr = take((size_t)P->nk);
    P->stage_bytes = off;
    return PLSLAM_OK;
}

// Fills the staged block (P.stage_bytes bytes at `stage`) from the caller's arrays; the flags become 0 / 1.
inline void lc_image_pack(const LcImagePlan& P, const double* T_corr, const uint8_t* corrected, const double* x_kf_w_new, char* stage)
{
    memset(stage, 0, P.stage_bytes);
    memcpy(stage + P.o_T, T_corr, (size_t)P.nk * 128);
    if (P.with_x) memcpy(stage + P.o_x, x_kf_w_new, (size_t)P.nk * 48);
    for (int32_t k = 0; k < P.nk; ++k) stage[P.o_corr + (size_t)k] = corrected[k] ? 1 : 0;
}

}  // namespace plslam
