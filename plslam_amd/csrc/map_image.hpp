// map_image.hpp -- the pure host part of the device-resident map image (plslam_map_index, include/plslam_hip.h): the argument
// checks every call that reads an image, or writes one out of place, makes before it launches anything (local_map.hip,
// map_insert.hip, lc_fuse_plan.hpp).  No HIP in here: tests/cpp/test_lc_fuse_pack.cpp compiles it without hipcc.
#pragma once

#include <cstdint>

#include "plslam_hip.h"

namespace plslam {

// one landmark kind of an image a call READS: the counts in range, every array its counts need is there
inline bool map_src_kind_ok(const plslam_map_landmarks& L)
{
    return L.n >= 0 && L.n_obs >= 0 && L.n_obs < (1 << 30) && L.n_feat >= 0 &&
           (L.n == 0 || (L.valid && L.inlier && L.X && L.obs_ptr)) && (L.n_obs == 0 || (L.n > 0 && L.obs_kf && L.obs_val)) &&
           (L.n_feat == 0 || (L.feat_ptr && L.feat_idx));
}
// ... of an image a call WRITES out of place: every destination array is there and none of them is an array of the source
// (feat_ptr may be the source's).  This is what keeps a kernel from writing through a source pointer.
inline bool map_dst_kind_ok(const plslam_map_landmarks& D, const plslam_map_landmarks& S)
{
    const void* d[] = {D.valid, D.inlier, D.X, D.obs_ptr, D.obs_kf, D.obs_val, D.feat_idx};
    const void* s[] = {S.valid, S.inlier, S.X, S.obs_ptr, S.obs_kf, S.obs_val, S.feat_idx, S.feat_ptr};
    for (const void* p : d) {
        if (!p) return false;
        for (const void* q : s)
            if (p == q) return false;
    }
    return D.feat_ptr != nullptr;
}

}  // namespace plslam
