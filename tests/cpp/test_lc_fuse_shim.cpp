// A C++ client of plslam_amd/host/lc_fuse.hpp: reads a map image, lc_idx_list, lc_pt_idxs / lc_ls_idxs, the keyframes' features
// and the caller-side containers (map_*_kf_idx, a per-observation list) written by the Python test, uploads the image once,
// fuses on the device as the end of loopClosureOptimizationCovGraphG2O would, applies the records to the containers, and writes
// the image, the records and the containers for the test to compare with the sequential restatement.
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "../../plslam_amd/host/lc_fuse.hpp"

using namespace PLSLAM::map_insert;
using namespace PLSLAM::lc_fuse;

template <class T> static std::vector<T> rd(const std::string& dir, const std::string& name)
{
    std::ifstream f(dir + "/" + name + ".bin", std::ios::binary | std::ios::ate);
    if (!f) throw std::runtime_error("missing " + name);
    std::vector<T> v((size_t)f.tellg() / sizeof(T));
    f.seekg(0);
    f.read(reinterpret_cast<char*>(v.data()), (std::streamsize)(v.size() * sizeof(T)));
    return v;
}
template <class T> static void wr(const std::string& dir, const std::string& name, const std::vector<T>& v)
{
    std::ofstream f(dir + "/" + name + ".bin", std::ios::binary);
    f.write(reinterpret_cast<const char*>(v.data()), (std::streamsize)(v.size() * sizeof(T)));
}
static HostKind kind_in(const std::string& d, const std::string& k)
{
    HostKind h;
    h.valid = rd<uint8_t>(d, k + "_valid"); h.inlier = rd<uint8_t>(d, k + "_inlier"); h.X = rd<double>(d, k + "_X");
    h.obs_val = rd<double>(d, k + "_obs_val"); h.obs_ptr = rd<int32_t>(d, k + "_obs_ptr"); h.obs_kf = rd<int32_t>(d, k + "_obs_kf");
    h.feat_ptr = rd<int32_t>(d, k + "_feat_ptr"); h.feat_idx = rd<int32_t>(d, k + "_feat_idx");
    return h;
}
static void kind_out(const std::string& d, const std::string& k, const HostKind& h)
{
    wr(d, "out_" + k + "_valid", h.valid); wr(d, "out_" + k + "_inlier", h.inlier); wr(d, "out_" + k + "_X", h.X);
    wr(d, "out_" + k + "_obs_val", h.obs_val); wr(d, "out_" + k + "_obs_ptr", h.obs_ptr); wr(d, "out_" + k + "_obs_kf", h.obs_kf);
    wr(d, "out_" + k + "_feat_ptr", h.feat_ptr); wr(d, "out_" + k + "_feat_idx", h.feat_idx);
}
// the reference's nested containers from the flat files
static std::vector<std::vector<Tuple>> idxs_in(const std::string& d, const std::string& k)
{
    const auto t = rd<int32_t>(d, k + "_tuples"), ep = rd<int32_t>(d, k + "_entry_ptr");
    std::vector<std::vector<Tuple>> out(ep.size() - 1);
    for (size_t e = 0; e + 1 < ep.size(); ++e)
        for (int32_t i = ep[e]; i < ep[e + 1]; ++i) out[e].push_back(Tuple{t[4 * (size_t)i], t[4 * (size_t)i + 1], t[4 * (size_t)i + 2], t[4 * (size_t)i + 3]});
    return out;
}
static std::vector<std::vector<int>> lists_in(const std::string& d, const std::string& k)
{
    const auto p = rd<int32_t>(d, k + "_kf_idx_ptr"), v = rd<int32_t>(d, k + "_kf_idx");
    std::vector<std::vector<int>> out(p.size() - 1);
    for (size_t i = 0; i + 1 < p.size(); ++i) out[i].assign(v.begin() + p[i], v.begin() + p[i + 1]);
    return out;
}
static void lists_out(const std::string& d, const std::string& k, const std::vector<std::vector<int>>& l)
{
    std::vector<int32_t> p{0}, v;
    for (const auto& x : l) {
        v.insert(v.end(), x.begin(), x.end());
        p.push_back((int32_t)v.size());
    }
    wr(d, "out_" + k + "_kf_idx_ptr", p);
    wr(d, "out_" + k + "_kf_idx", v);
}

int main(int argc, char** argv)
{
    if (argc < 2) return 2;
    const std::string d = argv[1];
    try {
        const auto lc = rd<int32_t>(d, "lc_idx");
        const auto T = rd<double>(d, "T_kf_w");
        std::vector<std::array<int, 3>> lc_idx_list;
        for (size_t e = 0; e < lc.size() / 3; ++e) lc_idx_list.push_back({lc[3 * e], lc[3 * e + 1], lc[3 * e + 2]});
        HostImage h;
        h.kf_valid = rd<uint8_t>(d, "kf_valid");
        h.x_kf_w = rd<double>(d, "x_kf_w");
        h.points = kind_in(d, "pt");
        h.lines = kind_in(d, "ls");
        const KindFeatures fp{h.points.feat_ptr, rd<double>(d, "pt_feat_P"), rd<double>(d, "pt_feat_obs")};
        const KindFeatures fl{h.lines.feat_ptr, rd<double>(d, "ls_feat_P"), rd<double>(d, "ls_feat_obs")};
        const Packed pts = pack(lc_idx_list, idxs_in(d, "pt"), fp, 3, 2), lns = pack(lc_idx_list, idxs_in(d, "ls"), fl, 6, 3);
        const size_t nk = h.kf_valid.size();
        std::vector<std::vector<int>> full_graph(nk, std::vector<int>(nk, 1)), pt_kf_idx = lists_in(d, "pt"), ls_kf_idx = lists_in(d, "ls");
        plslam_ctx* ctx = nullptr;
        check(plslam_ctx_create(0, &ctx), "ctx_create");
        {
            MapImages maps(ctx);
            maps.upload(h);
            Fuser fuser(ctx);
            const Fused f = fuser.run(maps, pack_entries(lc_idx_list), T, pts, lns);
            for (auto& e : lc_idx_list) e[2] = 0;                       // :4401-4402, the caller's
            apply_graph(f, full_graph);
            apply_kf_idx(f.points, pt_kf_idx);
            apply_kf_idx(f.lines, ls_kf_idx);
            // a per-observation list of the caller's (a stand-in for desc_list / dir_list): the old entries 1000 + their index, a made
            // one 2 t + w
            std::vector<int32_t> old((size_t)h.points.obs_kf.size());
            for (size_t j = 0; j < old.size(); ++j) old[j] = 1000 + (int32_t)j;
            wr(d, "out_pt_list", gather(f.points, old, [](int32_t t, int32_t w) { return 2 * t + w; }));
            wr(d, "out_pt_ev", f.points.ev); wr(d, "out_pt_dir", f.points.dir); wr(d, "out_pt_obs_src", f.points.obs_src);
            wr(d, "out_ls_ev", f.lines.ev); wr(d, "out_ls_dir", f.lines.dir); wr(d, "out_ls_obs_src", f.lines.obs_src);
            const plslam_lc_fuse_kind_counts &a = f.counts.points, &b = f.counts.lines;
            wr(d, "out_counts", std::vector<int32_t>{a.n_a, a.n_b, a.n_c, a.n_d, a.n_new, a.n_dead, a.n_skipped,
                                                     b.n_a, b.n_b, b.n_c, b.n_d, b.n_new, b.n_dead, b.n_skipped});
            std::vector<int32_t> g;
            for (const auto& row : full_graph) g.insert(g.end(), row.begin(), row.end());
            wr(d, "out_full_graph", g);
            lists_out(d, "pt", pt_kf_idx);
            lists_out(d, "ls", ls_kf_idx);
            HostImage o;
            maps.download(o);
            wr(d, "out_kf_valid", o.kf_valid); wr(d, "out_x_kf_w", o.x_kf_w);
            kind_out(d, "pt", o.points);
            kind_out(d, "ls", o.lines);
        }
        plslam_ctx_destroy(ctx);
    } catch (const std::exception& e) {
        std::cerr << e.what() << "\n";
        return 1;
    }
    return 0;
}
