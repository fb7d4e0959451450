// map_image_dev.hpp -- the device view of one landmark kind of the map image (plslam_map_landmarks) and the guarded accessors the
// map kernels share (local_map.hip K55-K62, map_insert.hip K63-K67, lc_fuse.hip K68-K73).  One copy: the rule "an index read from
// the image is range-checked before it is used as an address" is written here once.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "map_image.hpp"

namespace plslam {

constexpr int MAP_NW = MAP_TILE / 64;   // waves per workgroup (MAP_TILE and map_tiles: map_image.hpp, shared with the host planners)

struct MapKindSrc {                     // one landmark kind of an image a kernel READS
    int32_t n, n_obs, n_feat, dl, dv;   // dl: doubles per landmark / feature position (3 / 6), dv: doubles per observation (2 / 3)
    const uint8_t *valid, *inlier;
    const double* X;
    const int32_t *obs_ptr, *obs_kf;
    const double* obs_val;
    const int32_t *feat_ptr, *feat_idx;
};
struct MapKindDst {                     // ... of the destination of an out-of-place call, with its two capacities
    uint8_t *valid, *inlier;
    double* X;
    int32_t *obs_ptr, *obs_kf;
    double* obs_val;
    int32_t* feat_idx;
    int32_t cap, obs_cap;
};

inline MapKindSrc map_kind_src(const plslam_map_landmarks& L, int lines)
{
    return MapKindSrc{L.n, L.n_obs, L.n_feat, lines ? 6 : 3, lines ? 3 : 2, L.valid, L.inlier, L.X, L.obs_ptr, L.obs_kf, L.obs_val, L.feat_ptr, L.feat_idx};
}
// (the ABI struct is const where a READING call needs no more; map_dst_kind_ok has told these arrays from the source's)
inline MapKindDst map_kind_dst(const plslam_map_landmarks& L, int32_t cap, int32_t obs_cap)
{
    return MapKindDst{L.valid, (uint8_t*)L.inlier, (double*)L.X, (int32_t*)L.obs_ptr, (int32_t*)L.obs_kf, (double*)L.obs_val, L.feat_idx, cap, obs_cap};
}

// the length of a landmark's list in the source image, 0 where obs_ptr is not a list inside obs_kf
__device__ __forceinline__ int32_t old_len(const MapKindSrc& S, int32_t lm)
{
    const int32_t b = S.obs_ptr[lm], e = S.obs_ptr[lm + 1];
    return b >= 0 && e > b && e <= S.n_obs ? e - b : 0;
}
// the features of a slot: [f0, f0 + nf) inside feat_idx, empty where feat_ptr is not
__device__ __forceinline__ void slot_features(const MapKindSrc& S, int32_t kf, int32_t& f0, int32_t& nf)
{
    f0 = nf = 0;
    if (S.n_feat <= 0) return;
    const int32_t b = S.feat_ptr[kf], e = S.feat_ptr[kf + 1];
    if (b >= 0 && e > b && e <= S.n_feat) { f0 = b; nf = e - b; }
}
// Eigen's normalized(): v / sqrt(squaredNorm) where the squared norm is positive, else v itself; (x^2 + y^2) + z^2
__device__ __forceinline__ void normalized3(const double v[3], double o[3])
{
    const double z = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2];
    if (z > 0.0) {
        const double s = sqrt(z);
        o[0] = v[0] / s; o[1] = v[1] / s; o[2] = v[2] / s;
    } else {
        o[0] = v[0]; o[1] = v[1]; o[2] = v[2];
    }
}
// v / v.norm(): no guard (src/mapHandler.cpp:311, :4436, :4474)
__device__ __forceinline__ void over_norm3(const double v[3], double o[3])
{
    const double s = sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
    o[0] = v[0] / s; o[1] = v[1] / s; o[2] = v[2] / s;
}

}  // namespace plslam
