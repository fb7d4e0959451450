// gba.hpp -- header-only drop-in for MapHandler::globalBundleAdjustment (src/mapHandler.cpp:1995-2099) on the C ABI's
// global bundle adjustment (plslam_gba_*, include/plslam_hip.h).  The caller describes its map with plain arrays (no PL-SLAM
// types here); gba::run builds the lists as :1995-2099 does, runs levMarquardtOptimizationGBA on the device and writes back
// as :2674-2702 does (T_kf_w of every optimised keyframe, point3D, line3D; no inlier marking).  gba::runResident is the same
// optimisation on a map that lives on the device (plslam_map_index): gather, plan, loop and write-back without the host.
#pragma once

#include <stdexcept>
#include <string>
#include <vector>

#include "plslam_hip.h"

namespace PLSLAM {
namespace gba {

struct Keyframe {                 // map_keyframes[i]; present == false for a NULL entry
    bool present = true;
    int kf_idx = 0;               // keyframe 0 stays fixed
    double T_kf_w[16];            // row-major
    double x_kf_w[6];
};
struct Landmark {                 // map_points[i] / map_lines[i]; present == false for a NULL entry
    bool present = true;
    double X[6];                  // point3D (3) or line3D (6)
    std::vector<int> kf_obs;      // kf_obs_list: map index of the observing keyframe
    std::vector<double> obs;      // obs_list: 2 (points) or 3 (lines) doubles per observation
};
struct Params {
    double homog_th = 1e-7, lambda_lba_lm = 0.00001, lambda_lba_k = 10.0;
    int max_iters_lba = 15;
};

inline void check(int rc, const char* where)
{
    if (rc != PLSLAM_OK) throw std::runtime_error(std::string("[gba] ") + where + ": " + plslam_strerror(rc) + "; " + plslam_last_error());
}

// returns the number of solves; trace (optional) receives one record per solve
inline int run(plslam_ctx* ctx, const plslam_cam& cam, const Params& prm, std::vector<Keyframe>& kfs, std::vector<Landmark>& pts,
               std::vector<Landmark>& lns, std::vector<plslam_gba_solve>* trace = nullptr)
{
    std::vector<int32_t> kf_list, loc_of(kfs.size(), -1);
    std::vector<double> x_kf, T_all(kfs.size() * 16, 0.0);
    for (size_t i = 0; i < kfs.size(); ++i) {
        if (!kfs[i].present) continue;
        for (int a = 0; a < 16; ++a) T_all[16 * i + a] = kfs[i].T_kf_w[a];
        if (kfs[i].kf_idx == 0) continue;
        loc_of[i] = (int32_t)kf_list.size();
        kf_list.push_back((int32_t)i);
        x_kf.insert(x_kf.end(), kfs[i].x_kf_w, kfs[i].x_kf_w + 6);
    }
    auto lists = [&](std::vector<Landmark>& lms, int dl, int dobs, std::vector<int32_t>& rows, std::vector<double>& ob,
                     std::vector<double>& X, std::vector<int>& map_of) {
        int32_t loc = 0;
        for (size_t j = 0; j < lms.size(); ++j) {
            if (!lms[j].present) continue;
            X.insert(X.end(), lms[j].X, lms[j].X + dl);
            for (size_t i = 0; i < lms[j].kf_obs.size(); ++i) {
                const int k = lms[j].kf_obs[i];
                if (k < 0 || (size_t)k >= kfs.size() || !kfs[k].present) continue;    // the reference skips NULL keyframes
                const int32_t r[6] = {(int32_t)j, loc, (int32_t)i, k, loc_of[k], 1};
                rows.insert(rows.end(), r, r + 6);
                ob.insert(ob.end(), lms[j].obs.begin() + dobs * i, lms[j].obs.begin() + dobs * (i + 1));
            }
            map_of.push_back((int)j);
            ++loc;
        }
    };
    std::vector<int32_t> prow, lrow;
    std::vector<double> puv, ll, Xw, Lw;
    std::vector<int> pmap, lmap;
    lists(pts, 3, 2, prow, puv, Xw, pmap);
    lists(lns, 6, 3, lrow, ll, Lw, lmap);
    const int32_t nkf = (int32_t)kf_list.size(), npt = (int32_t)pmap.size(), nls = (int32_t)lmap.size();
    plslam_gba_plan* plan = nullptr;
    check(plslam_gba_plan_create(ctx, &cam, prm.homog_th, (int32_t)kfs.size(), nkf, kf_list.data(), npt, nls, prow.data(),
                                 puv.data(), (int32_t)(prow.size() / 6), lrow.data(), ll.data(), (int32_t)(lrow.size() / 6), &plan),
          "plslam_gba_plan_create");
    std::vector<double> x_out(x_kf.size()), T_out((size_t)nkf * 16), X_out(Xw.size()), L_out(Lw.size());
    std::vector<plslam_gba_solve> tr((size_t)(prm.max_iters_lba > 1 ? prm.max_iters_lba : 1));
    plslam_gba_result res{};
    const int rc = plslam_gba_optimize(plan, prm.lambda_lba_lm, prm.lambda_lba_k, prm.max_iters_lba, T_all.data(), x_kf.data(),
                                       Xw.data(), Lw.data(), x_out.data(), T_out.data(), X_out.data(), L_out.data(), tr.data(), &res);
    plslam_gba_plan_destroy(plan);
    check(rc, "plslam_gba_optimize");
    // write-back (:2674-2702): T_kf_w = expmap_se3(X) of every optimised keyframe, point3D / line3D = X
    for (int32_t k = 0; k < nkf; ++k)
        for (int a = 0; a < 16; ++a) kfs[kf_list[k]].T_kf_w[a] = T_out[16 * (size_t)k + a];
    for (int32_t j = 0; j < npt; ++j)
        for (int a = 0; a < 3; ++a) pts[pmap[j]].X[a] = X_out[3 * (size_t)j + a];
    for (int32_t j = 0; j < nls; ++j)
        for (int a = 0; a < 6; ++a) lns[lmap[j]].X[a] = L_out[6 * (size_t)j + a];
    if (trace) trace->assign(tr.begin(), tr.begin() + res.n_solves);
    return res.n_solves;
}

// The resident route: the same optimisation for a caller whose map lives on the device as a plslam_map_index (host/local_map.hpp:
// LocalMapIndex).  Nothing but the poses crosses to the host: the gather (plslam_local_map_form_all + _gather), the plan
// (plslam_gba_plan_create_dev), the loop (plslam_gba_optimize_dev) and the write-back of the landmarks into the image
// (plslam_local_map_apply_gba) run on the device.  form_all overwrites the handle's local flags: a cull or a candidate mask
// afterwards needs a new form.
//   T_all    the stored T_kf_w of every map slot (n_map_kf x 16, row-major; NULL slots: anything) -- poses stay with the host
//   dst      where the landmarks go: the image's own X arrays (LocalMapIndex::writeBackDst())
//   kf_list  out: the map index of every optimised keyframe; T_out (nkf x 16): what :2676-2680 store as T_kf_w; x_out (nkf x 6)
// returns the number of solves; trace (optional) receives one record per solve
inline int runResident(plslam_ctx* ctx, const plslam_cam& cam, const Params& prm, plslam_local_map* lm, const plslam_map_index& map,
                       const plslam_local_map_lba_dst& dst, const std::vector<double>& T_all, std::vector<int32_t>& kf_list,
                       std::vector<double>& T_out, std::vector<double>& x_out, std::vector<plslam_gba_solve>* trace = nullptr)
{
    if (T_all.size() != (size_t)map.n_map_kf * 16) throw std::runtime_error("[gba] runResident: T_all is n_map_kf x 16");
    plslam_local_map_counts c{};
    check(plslam_local_map_form_all(lm, &map, &c), "plslam_local_map_form_all");
    check(plslam_local_map_gather(lm, &map, &c), "plslam_local_map_gather");
    plslam_local_map_buffers b{};
    check(plslam_local_map_device_buffers(lm, &b), "plslam_local_map_device_buffers");
    plslam_gba_plan* plan = nullptr;
    check(plslam_gba_plan_create_dev(ctx, &cam, prm.homog_th, map.n_map_kf, c.nkf, b.kf_list, c.npt, c.nls, b.pt_obs, b.pt_obs_uv, c.n_pt_obs,
                                     b.ls_obs, b.ls_l_obs, c.n_ls_obs, &plan),
          "plslam_gba_plan_create_dev");
    kf_list.assign((size_t)c.nkf, 0);
    x_out.assign((size_t)c.nkf * 6, 0.0);
    T_out.assign((size_t)c.nkf * 16, 0.0);
    std::vector<plslam_gba_solve> tr((size_t)(prm.max_iters_lba > 1 ? prm.max_iters_lba : 1));
    plslam_gba_result res{};
    const double* X = b.X_aux;
    int rc = plslam_gba_optimize_dev(plan, prm.lambda_lba_lm, prm.lambda_lba_k, prm.max_iters_lba, T_all.data(), X, X + 6 * (size_t)c.nkf,
                                     X + 6 * (size_t)c.nkf + 3 * (size_t)c.npt, x_out.data(), T_out.data(), tr.data(), &res);
    const char* where = "plslam_gba_optimize_dev";
    if (rc == PLSLAM_OK) { rc = plslam_local_map_apply_gba(lm, plan, &dst); where = "plslam_local_map_apply_gba"; }
    plslam_gba_plan_destroy(plan);
    check(rc, where);
    plslam_local_map_buffers h{};
    h.kf_list = kf_list.data();
    check(plslam_local_map_download(lm, &h), "plslam_local_map_download");
    if (trace) trace->assign(tr.begin(), tr.begin() + res.n_solves);
    return res.n_solves;
}

}  // namespace gba
}  // namespace PLSLAM
