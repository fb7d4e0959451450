// pgo.hpp -- header-only drop-in for the body of MapHandler::loopClosureOptimizationCovGraphG2O (src/mapHandler.cpp:4185-4398,
// up to loopClosureFuseLandmarks()) on the C ABI's loop-closure correction (plslam_pgo_*, plslam_lc_correct_map,
// plslam_lc_correct_image, include/plslam_hip.h).  The caller describes its map with plain arrays (no PL-SLAM or g2o types here);
// pgo::run builds and optimises the pose graph, writes T_kf_w / x_kf_w back as :4298-4304 and :4358-4362 do, and re-anchors every
// landmark of a corrected keyframe as :4306-4355 / :4364-4397 do; pgo::runResident does the same on a device-resident map image, in
// place, without the map_*_kf_idx containers.  Marking the LC entries optimised ((2) = 0) and the landmark fusion stay with the
// caller.
#pragma once

#include <algorithm>
#include <stdexcept>
#include <string>
#include <vector>

#include "plslam_hip.h"

namespace PLSLAM {
namespace pgo {

struct Keyframe {                 // map_keyframes[i]; present == false for a NULL entry
    bool present = true;
    double T_kf_w[16];            // row-major
    double x_kf_w[6];
};
struct Landmark {                 // map_points[i] / map_lines[i]; present == false for a NULL entry
    bool present = true;
    double X[6];                  // point3D (3) or line3D (6)
    double med_obs_dir[3];
    std::vector<double> dir_list; // 3 doubles per entry
};
struct Params {
    int min_lm_ess_graph = 75, min_lm_cov_graph = 75, max_iters_pgo = 100, max_trials = 10;
    double lambda_init = 1e-10;
};

inline void check(int rc, const char* where)
{
    if (rc != PLSLAM_OK) throw std::runtime_error(std::string("[pgo] ") + where + ": " + plslam_strerror(rc) + "; " + plslam_last_error());
}

namespace detail {
struct Kind {                     // one landmark kind as the C ABI takes it, and the write-back
    std::vector<int32_t> ptr, idx, dptr;
    std::vector<uint8_t> valid;
    std::vector<double> X, med, dirs;
    plslam_lc_landmarks view{};
    void build(std::vector<Landmark>& lms, const std::vector<std::vector<int>>& kf_idx, int dl)
    {
        ptr.assign(1, 0);
        for (const auto& l : kf_idx) { for (int j : l) idx.push_back(j); ptr.push_back((int32_t)idx.size()); }
        dptr.assign(1, 0);
        for (auto& m : lms) {
            valid.push_back(m.present ? 1 : 0);
            X.insert(X.end(), m.X, m.X + dl);
            med.insert(med.end(), m.med_obs_dir, m.med_obs_dir + 3);
            dirs.insert(dirs.end(), m.dir_list.begin(), m.dir_list.end());
            dptr.push_back((int32_t)(dirs.size() / 3));
        }
        view = {(int32_t)lms.size(), (int32_t)idx.size(), (int32_t)(dirs.size() / 3), ptr.data(), idx.data(), valid.data(), X.data(),
                med.data(), dptr.data(), dirs.data()};
    }
    void store(std::vector<Landmark>& lms, int dl) const
    {
        for (size_t j = 0; j < lms.size(); ++j) {
            for (int a = 0; a < dl; ++a) lms[j].X[a] = X[dl * j + a];
            for (int a = 0; a < 3; ++a) lms[j].med_obs_dir[a] = med[3 * j + a];
            for (size_t d = 0; d < lms[j].dir_list.size(); ++d) lms[j].dir_list[d] = dirs[3 * (size_t)dptr[j] + d];
        }
    }
};
}  // namespace detail

namespace detail {
struct Correction {               // what the optimise half leaves for the map correction
    std::vector<double> T_corr, x_out;
    std::vector<uint8_t> corrected;
    plslam_pgo_result res{};
};
// The plan and optimise half of run / runResident: builds and optimises the pose graph and writes T_kf_w / x_kf_w of the corrected
// slots back into the Keyframes (:4298-4304, :4358-4362).
inline Correction optimize(plslam_ctx* ctx, const Params& prm, std::vector<Keyframe>& kfs, const std::vector<int32_t>& full_graph,
                           const std::vector<int32_t>& lc_idx, const std::vector<double>& lc_pose, std::vector<plslam_pgo_trial>* trace)
{
    const size_t n = kfs.size();
    const int32_t n_lc = (int32_t)(lc_idx.size() / 3);
    std::vector<uint8_t> valid(n);
    std::vector<double> T(n * 16, 0.0), x(n * 6, 0.0);
    for (size_t i = 0; i < n; ++i) {
        valid[i] = kfs[i].present ? 1 : 0;
        if (!kfs[i].present) continue;
        for (int a = 0; a < 16; ++a) T[16 * i + a] = kfs[i].T_kf_w[a];
        for (int a = 0; a < 6; ++a) x[6 * i + a] = kfs[i].x_kf_w[a];
    }
    const plslam_pgo_params p{prm.min_lm_ess_graph, prm.min_lm_cov_graph, prm.max_iters_pgo, prm.max_trials, prm.lambda_init};
    plslam_pgo_plan* plan = nullptr;
    check(plslam_pgo_plan_create(ctx, &p, (int32_t)n, valid.data(), full_graph.data(), n_lc, lc_idx.data(), &plan), "plan_create");
    Correction c;
    std::vector<double> To(n * 16);
    c.T_corr.resize(n * 16); c.x_out.resize(n * 6); c.corrected.resize(n);
    std::vector<plslam_pgo_trial> tr((size_t)prm.max_iters_pgo * prm.max_trials + 1);
    const int rc = plslam_pgo_optimize(plan, T.data(), x.data(), lc_pose.data(), To.data(), c.x_out.data(), c.T_corr.data(),
                                       c.corrected.data(), tr.data(), (int32_t)tr.size(), &c.res);
    plslam_pgo_plan_destroy(plan);
    check(rc, "optimize");
    if (trace) trace->assign(tr.begin(), tr.begin() + std::min<size_t>(tr.size(), (size_t)c.res.trials));
    for (size_t i = 0; i < n; ++i) {
        if (!c.corrected[i]) continue;
        for (int a = 0; a < 16; ++a) kfs[i].T_kf_w[a] = To[16 * i + a];
        for (int a = 0; a < 6; ++a) kfs[i].x_kf_w[a] = c.x_out[6 * i + a];
    }
    return c;
}
}  // namespace detail

// lc_idx: n_lc rows of (kf_prev, kf_curr, flag) as lc_idx_list; lc_pose: n_lc x 6 as lc_pose_list; full_graph: n_kf x n_kf
// row-major; map_points_kf_idx / map_lines_kf_idx: the anchor list of every keyframe slot.  Returns the optimiser's result;
// trace (optional) receives one record per trial.
inline plslam_pgo_result run(plslam_ctx* ctx, const Params& prm, std::vector<Keyframe>& kfs, const std::vector<int32_t>& full_graph,
                             const std::vector<int32_t>& lc_idx, const std::vector<double>& lc_pose, std::vector<Landmark>& pts,
                             const std::vector<std::vector<int>>& map_points_kf_idx, std::vector<Landmark>& lns,
                             const std::vector<std::vector<int>>& map_lines_kf_idx, std::vector<plslam_pgo_trial>* trace = nullptr)
{
    const detail::Correction c = detail::optimize(ctx, prm, kfs, full_graph, lc_idx, lc_pose, trace);
    detail::Kind P, L;
    P.build(pts, map_points_kf_idx, 3);
    L.build(lns, map_lines_kf_idx, 6);
    check(plslam_lc_correct_map(ctx, (int32_t)kfs.size(), c.T_corr.data(), c.corrected.data(), &P.view, &L.view), "correct_map");
    P.store(pts, 3);
    L.store(lns, 6);
    return c.res;
}

// The same on a device-resident map: `index` is the image (local_map::LocalMapIndex::index(), map_insert::MapImages::index()) whose
// keyframe slots are `kfs`, `lists` (may be NULL) the side lists that go with it (map_lists::MapLists::lists()).  The landmarks, the
// dir rows and the image's x_kf_w are corrected IN PLACE on the device by plslam_lc_correct_image: a landmark's anchor is its first
// observer, so no map_points_kf_idx / map_lines_kf_idx is taken and no landmark leaves the device.  counts (optional): what the
// correction touched.  The one condition: the caller's port never removes a landmark's first observation (the reference's live
// code does not); one that does keeps the containers and calls run.
inline plslam_pgo_result runResident(plslam_ctx* ctx, const Params& prm, std::vector<Keyframe>& kfs, const std::vector<int32_t>& full_graph,
                                     const std::vector<int32_t>& lc_idx, const std::vector<double>& lc_pose, const plslam_map_index& index,
                                     const plslam_map_lists* lists = nullptr, plslam_lc_image_counts* counts = nullptr,
                                     std::vector<plslam_pgo_trial>* trace = nullptr)
{
    if ((size_t)index.n_map_kf != kfs.size()) throw std::runtime_error("[pgo] runResident: the image has other keyframe slots than kfs");
    const detail::Correction c = detail::optimize(ctx, prm, kfs, full_graph, lc_idx, lc_pose, trace);
    const plslam_lc_image_dst dst{const_cast<double*>(index.points.X), lists ? lists->points.dir : nullptr, nullptr,
                                  const_cast<double*>(index.lines.X), lists ? lists->lines.dir : nullptr, nullptr,
                                  const_cast<double*>(index.x_kf_w)};
    check(plslam_lc_correct_image(ctx, &index, c.T_corr.data(), c.corrected.data(), c.x_out.data(), &dst, counts), "correct_image");
    return c.res;
}

}  // namespace pgo
}  // namespace PLSLAM
