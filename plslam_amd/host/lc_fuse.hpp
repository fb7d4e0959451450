// lc_fuse.hpp -- header-only client of the loop-closure landmark fusion on the device (plslam_lc_fuse_*, include/plslam_hip.h):
// MapHandler::loopClosureFuseLandmarks (src/mapHandler.cpp:4412-4687) over the pair of device images map_insert.hpp's MapImages
// keeps.  pack() turns lc_idx_list / lc_pt_idxs / lc_ls_idxs and the keyframes' features, as the reference holds them, into the
// call's arrays; Fuser::run() fuses from the current image into the other one; apply() brings the caller's own containers up to
// date from the records: full_graph, map_points_kf_idx / map_lines_kf_idx and, by one gather, any per-observation list the
// caller still keeps on the host (desc_list, dir_list, pts_list on the device: map_lists.hpp's MapLists::carry).  No PL-SLAM type here.
#pragma once

#include <algorithm>
#include <array>

#include "map_insert.hpp"

namespace PLSLAM {
namespace lc_fuse {

using map_insert::check;
using map_insert::MapImages;

// the features of every keyframe of one kind, laid out as the image's feat_ptr / feat_idx are: feature i of keyframe k is entry
// feat_ptr[k] + i.  P: PointFeature::P (x 3) or LineFeature::sP, eP (x 6); obs: pl (x 2) or le (x 3).  A NULL feature's values
// are never read by the call.
struct KindFeatures {
    std::vector<int32_t> feat_ptr;
    std::vector<double> P, obs;
};
using Tuple = std::array<int32_t, 4>;                                   // lm_idx0, lm_ldx0, lm_idx1, lm_ldx1
struct Packed {                                                         // one kind of plslam_lc_fuse_run's arguments
    std::vector<int32_t> tuples, entry_ptr;
    std::vector<double> P0, obs0, P1, obs1;
    plslam_lc_fuse_kind arg() const { return plslam_lc_fuse_kind{tuples.data(), entry_ptr.data(), P0.data(), obs0.data(), P1.data(), obs1.data()}; }
};
struct KindRecords {
    std::vector<int32_t> ev;                                            // m x 6
    std::vector<double> dir;                                            // m x 6
    std::vector<int32_t> obs_src;                                       // the destination's n_obs
};
struct Fused {
    KindRecords points, lines;
    std::vector<int32_t> graph_delta;                                   // n_map_kf^2
    plslam_lc_fuse_counts counts;
};

// lc_idx_list -> n_lc x 3
inline std::vector<int32_t> pack_entries(const std::vector<std::array<int, 3>>& lc_idx_list)
{
    std::vector<int32_t> out;
    for (const auto& e : lc_idx_list) out.insert(out.end(), {e[0], e[1], e[2]});
    return out;
}
// lc_pt_idxs / lc_ls_idxs (per entry the tuples) with the two features' values gathered per tuple; dl / dv: 3, 2 or 6, 3.  A
// feature the entry's keyframe does not have gives zeros (the call skips such a tuple where it would read it).
inline Packed pack(const std::vector<std::array<int, 3>>& lc_idx_list, const std::vector<std::vector<Tuple>>& idxs,
                   const KindFeatures& feats, int dl, int dv)
{
    Packed p;
    p.entry_ptr.push_back(0);
    const int32_t nk = (int32_t)feats.feat_ptr.size() - 1;
    auto gather = [&](int32_t kf, int32_t ldx, std::vector<double>& P, std::vector<double>& o) {
        int64_t f = -1;
        if (kf >= 0 && kf < nk && ldx >= 0 && ldx < feats.feat_ptr[kf + 1] - feats.feat_ptr[kf]) f = (int64_t)feats.feat_ptr[kf] + ldx;
        for (int a = 0; a < dl; ++a) P.push_back(f < 0 ? 0.0 : feats.P[(size_t)dl * f + a]);
        for (int a = 0; a < dv; ++a) o.push_back(f < 0 ? 0.0 : feats.obs[(size_t)dv * f + a]);
    };
    for (size_t e = 0; e < lc_idx_list.size(); ++e) {
        if (e < idxs.size())
            for (const Tuple& t : idxs[e]) {
                p.tuples.insert(p.tuples.end(), t.begin(), t.end());
                gather(lc_idx_list[e][0], t[1], p.P0, p.obs0);
                gather(lc_idx_list[e][1], t[3], p.P1, p.obs1);
            }
        p.entry_ptr.push_back((int32_t)(p.tuples.size() / 4));
    }
    return p;
}

class Fuser {
public:
    explicit Fuser(plslam_ctx* ctx) { check(plslam_lc_fuse_create(ctx, &lf_), "lc_fuse_create"); }
    ~Fuser() { plslam_lc_fuse_destroy(lf_); }
    Fuser(const Fuser&) = delete;
    Fuser& operator=(const Fuser&) = delete;

    // loopClosureFuseLandmarks() from maps' current image into its other one; T_kf_w: n_map_kf x 16, as plslam_pgo_optimize
    // writes T_out.  Marking the entries optimised (:4401-4402) stays with the caller, AFTER this.
    Fused run(MapImages& maps, const std::vector<int32_t>& lc_idx, const std::vector<double>& T_kf_w, const Packed& pts, const Packed& lns)
    {
        const plslam_map_index& m = maps.index();
        const int32_t n_lc = (int32_t)(lc_idx.size() / 3);
        int32_t grow[2][2];                                             // per kind: cC, cAB among the flagged entries
        const Packed* K[2] = {&pts, &lns};
        for (int k = 0; k < 2; ++k) {
            grow[k][0] = grow[k][1] = 0;
            for (int32_t e = 0; e < n_lc && (size_t)e + 1 < K[k]->entry_ptr.size(); ++e) {
                if (lc_idx[3 * (size_t)e + 2] != 1) continue;
                for (int32_t t = K[k]->entry_ptr[e]; t < K[k]->entry_ptr[e + 1]; ++t) {
                    const bool a = K[k]->tuples[4 * (size_t)t] == -1, b = K[k]->tuples[4 * (size_t)t + 2] == -1;
                    grow[k][0] += a && b;
                    grow[k][1] += a != b;
                }
            }
        }
        Fused out;
        out.graph_delta.assign((size_t)m.n_map_kf * m.n_map_kf, 0);
        const plslam_lc_fuse_kind ap = pts.arg(), al = lns.arg();
        maps.pingpong(m.points.n + grow[0][0], m.points.n_obs + grow[0][1] + 2 * grow[0][0], m.lines.n + grow[1][0],
                      m.lines.n_obs + grow[1][1] + 2 * grow[1][0], [&](const plslam_map_index& src, plslam_map_insert_dst& dst) {
                          check(plslam_lc_fuse_run(lf_, &src, &dst, n_lc, lc_idx.data(), T_kf_w.data(), pts.entry_ptr.empty() ? nullptr : &ap,
                                                   lns.entry_ptr.empty() ? nullptr : &al, out.graph_delta.data(), &out.counts),
                                "lc_fuse_run");
                      });
        const plslam_map_index& d = maps.index();
        out.points.ev.resize(pts.tuples.size() / 4 * 6); out.points.dir.resize(pts.tuples.size() / 4 * 6);
        out.lines.ev.resize(lns.tuples.size() / 4 * 6); out.lines.dir.resize(lns.tuples.size() / 4 * 6);
        out.points.obs_src.resize((size_t)d.points.n_obs); out.lines.obs_src.resize((size_t)d.lines.n_obs);
        plslam_lc_fuse_buffers h{};
        h.pt_ev = out.points.ev.data(); h.pt_dir = out.points.dir.data(); h.pt_obs_src = out.points.obs_src.data();
        h.ls_ev = out.lines.ev.data(); h.ls_dir = out.lines.dir.data(); h.ls_obs_src = out.lines.obs_src.data();
        check(plslam_lc_fuse_download(lf_, &h), "lc_fuse_download");
        return out;
    }
    plslam_lc_fuse* handle() const { return lf_; }              // (whose records describe the last run: map_lists.hpp)

private:
    plslam_lc_fuse* lf_ = nullptr;
};

// full_graph += graph_delta (a dense n x n container of ints)
template <class Graph> inline void apply_graph(const Fused& f, Graph& full_graph)
{
    const size_t n = full_graph.size();
    for (size_t i = 0; i < n; ++i)
        for (size_t j = 0; j < n; ++j) full_graph[i][j] += f.graph_delta[i * n + j];
}
// map_points_kf_idx / map_lines_kf_idx: a new landmark goes to its anchor's list (:4477, :4619), a fused one leaves the list of
// its first observer (:4521-4529), in event order.  Only for a caller that still keeps the containers: pgo::runResident
// (plslam_lc_correct_image) reads the anchor from the image and needs none.
inline void apply_kf_idx(const KindRecords& r, std::vector<std::vector<int>>& map_kf_idx)
{
    for (size_t t = 0; t < r.ev.size() / 6; ++t) {
        const int32_t* e = r.ev.data() + 6 * t;
        if (e[3] < 0 || (size_t)e[3] >= map_kf_idx.size()) continue;
        std::vector<int>& l = map_kf_idx[(size_t)e[3]];
        if (e[0] == 3) l.push_back(e[1]);
        else if (e[0] == 4) {
            auto it = std::find(l.begin(), l.end(), e[2]);
            if (it != l.end()) l.erase(it);
        }
    }
}
// one per-observation list (desc_list, dir_list, pts_list flattened in the image's order) after the fusion: position j takes
// old[obs_src[j]], or made(t, w) for the observation tuple t made on side w (0 kf_prev's, 1 kf_curr's)
template <class T, class Made> inline std::vector<T> gather(const KindRecords& r, const std::vector<T>& old, Made made)
{
    std::vector<T> out;
    out.reserve(r.obs_src.size());
    for (int32_t s : r.obs_src) {
        if (s >= 0) out.push_back(old[(size_t)s]);
        else out.push_back(made((-1 - s) >> 1, (-1 - s) & 1));
    }
    return out;
}

}  // namespace lc_fuse
}  // namespace PLSLAM
