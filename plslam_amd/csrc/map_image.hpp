// map_image.hpp -- the pure host part of the device-resident map image (plslam_map_index, include/plslam_hip.h): the tile every map
// kernel and every host planner counts in; the argument checks every call that reads an image, or writes one out of place, makes
// before it launches anything (local_map_plan.hpp, map_insert_plan.hpp, lc_fuse_plan.hpp); and what the two out-of-place calls
// (map_insert.hip, lc_fuse.hip) share on the host: the typed pointer into a carved buffer and the commit after a successful run.
// No HIP in here: the planners' tests under tests/cpp compile it without hipcc.
#pragma once

#include <cstddef>
#include <cstdint>

#include "plslam_hip.h"

namespace plslam {

constexpr int MAP_TILE = 256;           // lanes per workgroup = items per look-back tile (plslam_amd/local_map.py: LOOKBACK_TILE)
inline unsigned map_tiles(int64_t n) { return (unsigned)(n > 0 ? (n + MAP_TILE - 1) / MAP_TILE : 1); }

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

// the slice at `off` of a carved buffer, typed: the one place an offset of a planner's layout becomes a pointer
template <class T> inline T* slice_at(char* base, size_t off) { return reinterpret_cast<T*>(base + off); }
template <class T> inline const T* slice_at(const char* base, size_t off) { return reinterpret_cast<const T*>(base + off); }

// one memset of a call's device buffer: the planners list them in the order they are issued
struct FillRegion { size_t off, bytes; int byte; };

// What the last successful insert / run of a handle left for a carry (map_lists.hip), per kind: the counts it read and produced,
// and its records on the device.  Written by map_commit below, read through map_lists_plan.hpp.
struct ListsKindRecords {
    int32_t src_n = 0, src_obs = 0, dst_n = 0, dst_obs = 0;
    int32_t n_ev = 0;                    // rows of ev / dir: the insert's events, the fuse's tuples
    int32_t bound[2] = {0, 0};           // rows of the caller's arrays side w may name: n_prev, n_curr / m, m
    int32_t ev_stride = 0;               // insert: 4, the row of side w is ev[4 e + 1 + w]; fuse: 0, the row is e
    int32_t need_side0 = 0;              // insert: kf2kf (side 0 rows exist); fuse: 1
    const int32_t* ev = nullptr;
    const double* dir = nullptr;
    const int32_t* obs_src = nullptr;
};
struct ListsRecords {
    bool valid = false;
    ListsKindRecords k[2];
};

// The commit of an out-of-place call that ran: per kind the destination's counts, the three event pointers in the handle's
// buffers struct (plslam_map_insert_events / plslam_lc_fuse_buffers) and the records a carry reads; then the image's n_map_kf.
struct MapCommitKind {
    int32_t n_new, n_obs;                // landmarks made; observations of the destination
    int32_t n_ev, bound[2];              // as ListsKindRecords
    int32_t* ev;
    double* dir;
    int32_t* obs_src;
};
template <class Events>
inline void map_commit(const plslam_map_index& src, plslam_map_index& dst, const MapCommitKind (&K)[2], int32_t ev_stride,
                       int32_t need_side0, Events& d, ListsRecords& lists)
{
    const plslam_map_landmarks* S[2] = {&src.points, &src.lines};
    plslam_map_landmarks* D[2] = {&dst.points, &dst.lines};
    for (int k = 0; k < 2; ++k) {
        D[k]->n = S[k]->n + K[k].n_new;
        D[k]->n_obs = K[k].n_obs;
        D[k]->n_feat = S[k]->n_feat;
        (k ? d.ls_ev : d.pt_ev) = K[k].ev;
        (k ? d.ls_dir : d.pt_dir) = K[k].dir;
        (k ? d.ls_obs_src : d.pt_obs_src) = K[k].obs_src;
        ListsKindRecords& R = lists.k[k];
        R = ListsKindRecords{};
        R.src_n = S[k]->n; R.src_obs = S[k]->n_obs; R.dst_n = D[k]->n; R.dst_obs = D[k]->n_obs;
        R.n_ev = K[k].n_ev; R.bound[0] = K[k].bound[0]; R.bound[1] = K[k].bound[1]; R.ev_stride = ev_stride; R.need_side0 = need_side0;
        R.ev = K[k].ev; R.dir = K[k].dir; R.obs_src = K[k].obs_src;
    }
    dst.n_map_kf = src.n_map_kf;
    lists.valid = true;
}

}  // namespace plslam
