// local_map.hpp -- header-only packer for the local map on the device (plslam_local_map_*, include/plslam_hip.h): LocalMapIndex
// turns containers shaped like the reference's map_keyframes / map_points / map_lines into the device-resident CSR image
// (plslam_map_index) and offers MapHandler's formLocalMap(), formLocalMap(kf), the gather of localBundleAdjustment() and
// removeBadMapLandmarks() (src/mapHandler.cpp:836-968, :1225-1321, :2705-2786) under the reference's names, returning the
// reference's containers.  No PL-SLAM type here; the HIP runtime is used for the image's device memory only.
#pragma once

#include <hip/hip_runtime_api.h>

#include <array>
#include <stdexcept>
#include <string>
#include <vector>

#include "plslam_hip.h"

namespace PLSLAM {
namespace local_map {

typedef std::array<int, 6> Vector6i;
struct Feature { bool present = true; int idx = -1; };                // stereo_pt[i] / stereo_ls[i]; present == false: NULL
struct KeyFrame {                                                       // map_keyframes[i]; present == false: NULL
    bool present = true, local = false;
    double x_kf_w[6] = {0, 0, 0, 0, 0, 0};
    std::vector<Feature> stereo_pt, stereo_ls;
};
struct Landmark {                                                       // map_points[i] / map_lines[i]; present == false: NULL
    bool present = true, inlier = true, local = false;
    double X[6] = {0, 0, 0, 0, 0, 0};                                   // point3D (3) or line3D (6)
    std::vector<int> kf_obs_list;
    std::vector<double> obs_list;                                       // 2 (points) or 3 (lines) doubles per observation
};
struct LbaLists {                                                       // what :1225-1321 hands to levMarquardtOptimizationLBA
    std::vector<double> X_aux;
    std::vector<int> kf_list, pt_list, ls_list;
    std::vector<Vector6i> pt_obs_list, ls_obs_list;
    std::vector<double> pt_obs_uv, ls_l_obs;                            // and the observations, as plslam_lba_plan_create takes them
};

inline void check(int rc, const char* where)
{
    if (rc != PLSLAM_OK) throw std::runtime_error(std::string("[local_map] ") + where + ": " + plslam_strerror(rc) + "; " + plslam_last_error());
}
inline void hip_check(hipError_t e, const char* where)
{
    if (e != hipSuccess) throw std::runtime_error(std::string("[local_map] ") + where + ": " + hipGetErrorString(e));
}

class LocalMapIndex {
public:
    explicit LocalMapIndex(plslam_ctx* ctx) { check(plslam_local_map_create(ctx, &lm_), "create"); }
    ~LocalMapIndex()
    {
        plslam_local_map_destroy(lm_);
        for (void* p : blocks_) (void)hipFree(p);
    }
    LocalMapIndex(const LocalMapIndex&) = delete;
    LocalMapIndex& operator=(const LocalMapIndex&) = delete;

    // (re)builds the image from the containers and uploads it
    void pack(const std::vector<KeyFrame>& kfs, const std::vector<Landmark>& pts, const std::vector<Landmark>& lns)
    {
        for (void* p : blocks_) (void)hipFree(p);
        blocks_.clear();
        const size_t n = kfs.size();
        std::vector<uint8_t> kv(n);
        std::vector<double> x(6 * n, 0.0);
        for (size_t i = 0; i < n; ++i) {
            kv[i] = kfs[i].present ? 1 : 0;
            for (int a = 0; a < 6; ++a) x[6 * i + a] = kfs[i].x_kf_w[a];
        }
        map_.n_map_kf = (int32_t)n;
        map_.kf_valid = up(kv);
        map_.x_kf_w = up(x);
        map_.points = kind(kfs, pts, false);
        map_.lines = kind(kfs, lns, true);
    }
    const plslam_map_index& index() const { return map_; }
    plslam_local_map* handle() const { return lm_; }

    // formLocalMap() (:836-902): full_graph_row = full_graph[full_graph.size() - 1]; the local flags go into the containers
    void formLocalMap(const std::vector<int32_t>& full_graph_row, int minLMCovGraph, int minKFLocalMap, std::vector<KeyFrame>& kfs,
                      std::vector<Landmark>& pts, std::vector<Landmark>& lns)
    {
        formLocalMap(map_.n_map_kf - 1, full_graph_row, minLMCovGraph, minKFLocalMap, kfs, pts, lns);
    }
    // formLocalMap(kf) (:904-968): kf_idx = kf->kf_idx; the row is STILL the last one (:946)
    void formLocalMap(int kf_idx, const std::vector<int32_t>& full_graph_row, int minLMCovGraph, int minKFLocalMap,
                      std::vector<KeyFrame>& kfs, std::vector<Landmark>& pts, std::vector<Landmark>& lns)
    {
        if ((int32_t)full_graph_row.size() != map_.n_map_kf) throw std::runtime_error("[local_map] formLocalMap: row length");
        check(plslam_local_map_form(lm_, &map_, kf_idx, full_graph_row.data(), minLMCovGraph, minKFLocalMap, &counts_), "form");
        std::vector<uint8_t> a(kfs.size()), b(pts.size()), c(lns.size());
        plslam_local_map_buffers h{};
        h.kf_local = a.data(); h.pt_local = b.data(); h.ls_local = c.data();
        check(plslam_local_map_download(lm_, &h), "download");
        for (size_t i = 0; i < kfs.size(); ++i) kfs[i].local = a[i] != 0;
        for (size_t i = 0; i < pts.size(); ++i) pts[i].local = b[i] != 0;
        for (size_t i = 0; i < lns.size(); ++i) lns[i].local = c[i] != 0;
    }
    // the candidate masks of matchMap2KFPoints / Lines (:547, :649), left on the device for the _dev drivers
    plslam_local_map_buffers candidates(int kf2_idx)
    {
        check(plslam_local_map_candidates(lm_, &map_, kf2_idx), "candidates");
        plslam_local_map_buffers b{};
        check(plslam_local_map_device_buffers(lm_, &b), "device_buffers");
        return b;
    }
    // the gather of localBundleAdjustment() (:1225-1321); returns -1 where the reference does (:1327), else 0
    int localBundleAdjustment(LbaLists& o)
    {
        check(plslam_local_map_gather(lm_, &map_, &counts_), "gather");
        const plslam_local_map_counts& c = counts_;
        std::vector<int32_t> p6(6 * (size_t)c.n_pt_obs), l6(6 * (size_t)c.n_ls_obs), kl(c.nkf), pl(c.npt), ll(c.nls);
        o.X_aux.assign(6 * (size_t)c.nkf + 3 * (size_t)c.npt + 6 * (size_t)c.nls, 0.0);
        o.pt_obs_uv.assign(2 * (size_t)c.n_pt_obs, 0.0);
        o.ls_l_obs.assign(3 * (size_t)c.n_ls_obs, 0.0);
        plslam_local_map_buffers h{};
        h.kf_list = kl.data(); h.pt_list = pl.data(); h.ls_list = ll.data(); h.pt_obs = p6.data(); h.ls_obs = l6.data();
        h.X_aux = o.X_aux.data(); h.pt_obs_uv = o.pt_obs_uv.data(); h.ls_l_obs = o.ls_l_obs.data();
        check(plslam_local_map_download(lm_, &h), "download");
        o.kf_list.assign(kl.begin(), kl.end()); o.pt_list.assign(pl.begin(), pl.end()); o.ls_list.assign(ll.begin(), ll.end());
        auto rows = [](const std::vector<int32_t>& v, std::vector<Vector6i>& out) {
            out.resize(v.size() / 6);
            for (size_t j = 0; j < out.size(); ++j)
                for (int a = 0; a < 6; ++a) out[j][a] = v[6 * j + a];
        };
        rows(p6, o.pt_obs_list);
        rows(l6, o.ls_obs_list);
        return c.empty ? -1 : 0;
    }
    // removeBadMapLandmarks() (:2705-2786): the image is culled in place; the containers follow (present = false, the first
    // observer's first feature that named the landmark = -1); returns the number of landmarks removed
    int removeBadMapLandmarks(int max_kf_idx, int minLMObs, std::vector<KeyFrame>& kfs, std::vector<Landmark>& pts,
                              std::vector<Landmark>& lns)
    {
        check(plslam_local_map_cull(lm_, &map_, max_kf_idx, minLMObs, &counts_), "cull");
        std::vector<uint8_t> rp(pts.size()), rl(lns.size());
        plslam_local_map_buffers h{};
        h.pt_removed = rp.data(); h.ls_removed = rl.data();
        check(plslam_local_map_download(lm_, &h), "download");
        auto apply = [&](std::vector<Landmark>& lms, const std::vector<uint8_t>& r, bool lines) {
            for (size_t i = 0; i < lms.size(); ++i) {
                if (!r[i]) continue;
                lms[i].present = false;
                const int k = lms[i].kf_obs_list[0];
                if (k < 0 || k >= (int)kfs.size() || !kfs[k].present) continue;
                for (Feature& f : lines ? kfs[k].stereo_ls : kfs[k].stereo_pt)
                    if (f.present && f.idx == (int)i) { f.idx = -1; break; }
            }
        };
        apply(pts, rp, false);
        apply(lns, rl, true);
        return counts_.n_pt_removed + counts_.n_ls_removed;
    }
    // the write-back of localBundleAdjustment() (:1828-1855) from the plan's resident landmarks into the image, in place, after
    // localBundleAdjustment() / plslam_local_map_gather on this handle: point3D / line3D <- the estimate, inlier = false where it
    // moved by more than moved_th (the reference's literal: 0.01).  The image's X and inlier arrays are this object's own device
    // memory, so it may write them.  Returns the number of landmarks flagged; the containers follow from the masks where the
    // caller keeps them (plslam_local_map_download: pt_moved / ls_moved).
    int applyLba(plslam_lba_plan* plan, double moved_th = 0.01)
    {
        const plslam_local_map_lba_dst d = writeBackDst();
        check(plslam_local_map_apply_lba(lm_, plan, &d, moved_th, &counts_), "apply_lba");
        return counts_.n_pt_moved + counts_.n_ls_moved;
    }
    // The gather of globalBundleAdjustment() (:1995-2092) left ON THE DEVICE: every non-NULL keyframe but slot 0, every non-NULL
    // landmark with all its observations.  formAll() overwrites the flags of the last formLocalMap(): removeBadMapLandmarks() or
    // candidates() afterwards need a new formLocalMap().  The lists stay in the handle's device buffers (deviceBuffers()) for
    // plslam_gba_plan_create_dev -- PLSLAM::gba::runResident (host/gba.hpp) takes them from there.
    void formAll() { check(plslam_local_map_form_all(lm_, &map_, &counts_), "form_all"); }
    void gatherResident() { check(plslam_local_map_gather(lm_, &map_, &counts_), "gather"); }
    plslam_local_map_buffers deviceBuffers()
    {
        plslam_local_map_buffers b{};
        check(plslam_local_map_device_buffers(lm_, &b), "device_buffers");
        return b;
    }
    // where the write-backs put the landmarks: the image's own X (and inlier) arrays, this object's device memory
    plslam_local_map_lba_dst writeBackDst() const
    {
        plslam_local_map_lba_dst d{};
        d.pt_X = const_cast<double*>(map_.points.X); d.pt_inlier = const_cast<uint8_t*>(map_.points.inlier);
        d.ls_X = const_cast<double*>(map_.lines.X); d.ls_inlier = const_cast<uint8_t*>(map_.lines.inlier);
        return d;
    }
    // the write-back of globalBundleAdjustment() (:2681-2697) from the GBA plan's resident landmarks into the image, in place,
    // after gatherResident() on this handle: point3D / line3D <- the estimate; no moved test, inlier untouched
    void applyGba(plslam_gba_plan* plan)
    {
        const plslam_local_map_lba_dst d = writeBackDst();
        check(plslam_local_map_apply_gba(lm_, plan, &d), "apply_gba");
    }
    // the image's landmarks, device -> host (n x 3 points, n x 6 lines): what a write-back left there
    void downloadLandmarks(std::vector<double>& pts_X, std::vector<double>& lns_X) const
    {
        pts_X.assign(3 * (size_t)map_.points.n, 0.0);
        lns_X.assign(6 * (size_t)map_.lines.n, 0.0);
        if (!pts_X.empty()) hip_check(hipMemcpy(pts_X.data(), map_.points.X, pts_X.size() * 8, hipMemcpyDeviceToHost), "hipMemcpy");
        if (!lns_X.empty()) hip_check(hipMemcpy(lns_X.data(), map_.lines.X, lns_X.size() * 8, hipMemcpyDeviceToHost), "hipMemcpy");
    }
    const plslam_local_map_counts& counts() const { return counts_; }

private:
    template <class T> T* up(const std::vector<T>& v)
    {
        void* d = nullptr;
        hip_check(hipMalloc(&d, v.size() * sizeof(T) + 8), "hipMalloc");
        blocks_.push_back(d);
        if (!v.empty()) hip_check(hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice), "hipMemcpy");
        return static_cast<T*>(d);
    }
    plslam_map_landmarks kind(const std::vector<KeyFrame>& kfs, const std::vector<Landmark>& lms, bool lines)
    {
        const int dl = lines ? 6 : 3;
        std::vector<uint8_t> valid, inl;
        std::vector<double> X, val;
        std::vector<int32_t> optr(1, 0), okf, fptr(1, 0), fidx;
        for (const Landmark& m : lms) {
            valid.push_back(m.present ? 1 : 0);
            inl.push_back(m.inlier ? 1 : 0);
            X.insert(X.end(), m.X, m.X + dl);
            okf.insert(okf.end(), m.kf_obs_list.begin(), m.kf_obs_list.end());
            val.insert(val.end(), m.obs_list.begin(), m.obs_list.end());
            optr.push_back((int32_t)okf.size());
        }
        for (const KeyFrame& k : kfs) {
            if (k.present)
                for (const Feature& f : lines ? k.stereo_ls : k.stereo_pt) fidx.push_back(f.present ? f.idx : PLSLAM_FEAT_NULL);
            fptr.push_back((int32_t)fidx.size());
        }
        plslam_map_landmarks L{};
        L.n = (int32_t)lms.size(); L.n_obs = (int32_t)okf.size(); L.n_feat = (int32_t)fidx.size();
        L.valid = up(valid); L.inlier = up(inl); L.X = up(X); L.obs_ptr = up(optr); L.obs_kf = up(okf); L.obs_val = up(val);
        L.feat_ptr = up(fptr); L.feat_idx = up(fidx);
        return L;
    }
    plslam_local_map* lm_ = nullptr;
    plslam_map_index map_{};
    plslam_local_map_counts counts_{};
    std::vector<void*> blocks_;
};

}  // namespace local_map
}  // namespace PLSLAM
