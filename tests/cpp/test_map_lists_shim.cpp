// A C++ client of plslam_amd/host/map_lists.hpp: reads a map image, its side lists and either a keyframe's tables and rows
// ("insert": the KF <-> KF insertion, then the map <-> KF insertion, a carry behind each) or a loop closure's tuples and rows
// ("fuse": one fusion and its carry) written by the Python test; image and lists stay on the device throughout, the
// representatives of the uploaded lists are computed there (plslam_map_lists_refresh); writes the final lists for the test to
// compare with the Python route.
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "../../plslam_amd/host/map_lists.hpp"

using namespace PLSLAM;
using map_insert::check;

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

static map_insert::HostKind kind_in(const std::string& d, const std::string& k)
{
    map_insert::HostKind h;
    h.valid = rd<uint8_t>(d, k + "_valid"); h.inlier = rd<uint8_t>(d, k + "_inlier"); h.X = rd<double>(d, k + "_X");
    h.obs_val = rd<double>(d, k + "_obs_val"); h.obs_ptr = rd<int32_t>(d, k + "_obs_ptr"); h.obs_kf = rd<int32_t>(d, k + "_obs_kf");
    h.feat_ptr = rd<int32_t>(d, k + "_feat_ptr"); h.feat_idx = rd<int32_t>(d, k + "_feat_idx");
    return h;
}
static map_lists::HostKind lists_in(const std::string& d, const std::string& k, bool lines)
{
    map_lists::HostKind h;
    h.desc = rd<uint8_t>(d, k + "_desc"); h.dir = rd<double>(d, k + "_dir");
    if (lines) h.pts = rd<double>(d, k + "_pts");
    return h;
}
static void lists_out(const std::string& d, const std::string& k, const map_lists::HostKind& h)
{
    wr(d, "out_" + k + "_desc", h.desc); wr(d, "out_" + k + "_dir", h.dir); wr(d, "out_" + k + "_pts", h.pts);
    wr(d, "out_" + k + "_med_idx", h.med_idx); wr(d, "out_" + k + "_med_desc", h.med_desc); wr(d, "out_" + k + "_refreshed", h.refreshed);
}
static map_insert::KindMatches matches(const std::string& d, const std::string& k, bool map2kf)
{
    map_insert::KindMatches m;
    m.table = rd<int32_t>(d, k + (map2kf ? "_map_to_kf" : "_matches_12"));
    m.P2 = rd<double>(d, k + "_P2"); m.obs2 = rd<double>(d, k + "_obs2");
    if (!map2kf) { m.P1 = rd<double>(d, k + "_P1"); m.obs1 = rd<double>(d, k + "_obs1"); }
    return m;
}
// a / b: the names of the two sides' files ("1", "2" for an insert, "0", "1" for a fusion); an empty a: side b only
static map_lists::Rows rows_in(const std::string& d, const std::string& k, const std::string& a, const std::string& b, bool lines)
{
    map_lists::Rows r;
    if (!a.empty()) r.desc_a = rd<uint8_t>(d, k + "_desc" + a);
    r.desc_b = rd<uint8_t>(d, k + "_desc" + b);
    if (lines) {
        if (!a.empty()) r.pts_a = rd<double>(d, k + "_pts" + a);
        r.pts_b = rd<double>(d, k + "_pts" + b);
    }
    return r;
}
static lc_fuse::Packed packed_in(const std::string& d, const std::string& k)
{
    lc_fuse::Packed p;
    p.tuples = rd<int32_t>(d, k + "_tuples"); p.entry_ptr = rd<int32_t>(d, k + "_entry_ptr");
    p.P0 = rd<double>(d, k + "_P0"); p.obs0 = rd<double>(d, k + "_obs0"); p.P1 = rd<double>(d, k + "_P1"); p.obs1 = rd<double>(d, k + "_obs1");
    return p;
}

int main(int argc, char** argv)
{
    if (argc < 3) return 2;
    const std::string d = argv[1], mode = argv[2];
    try {
        map_insert::HostImage h;
        h.kf_valid = rd<uint8_t>(d, "kf_valid");
        h.x_kf_w = rd<double>(d, "x_kf_w");
        h.points = kind_in(d, "pt");
        h.lines = kind_in(d, "ls");
        map_lists::HostLists hl;
        hl.points = lists_in(d, "pt", false);
        hl.lines = lists_in(d, "ls", true);
        plslam_ctx* ctx = nullptr;
        check(plslam_ctx_create(0, &ctx), "ctx_create");
        {
            map_insert::MapImages maps(ctx);
            map_lists::MapLists lists(ctx);
            maps.upload(h);
            lists.upload(hl, maps.index(), true);
            if (mode == "insert") {
                const auto p = rd<int32_t>(d, "params");       // kf1, kf2
                const auto T = rd<double>(d, "T");             // T_kf1_w, T_kf2_w
                maps.insertKF2KF(p[0], p[1], T.data(), T.data() + 16, matches(d, "pt", false), matches(d, "ls", false));
                lists.carry(maps, rows_in(d, "pt", "1", "2", false), rows_in(d, "ls", "1", "2", true));
                maps.insertMap2KF(p[1], T.data() + 16, matches(d, "pt", true), matches(d, "ls", true));
                lists.carry(maps, rows_in(d, "pt", "", "2", false), rows_in(d, "ls", "", "2", true));
            } else {
                lc_fuse::Fuser fuser(ctx);
                fuser.run(maps, rd<int32_t>(d, "lc_idx"), rd<double>(d, "T_kf_w"), packed_in(d, "pt"), packed_in(d, "ls"));
                lists.carry(fuser, maps, rows_in(d, "pt", "0", "1", false), rows_in(d, "ls", "0", "1", true));
            }
            map_lists::HostLists out;
            lists.download(out, maps.index());
            lists_out(d, "pt", out.points);
            lists_out(d, "ls", out.lines);
            wr(d, "out_counts", std::vector<int32_t>{maps.index().points.n, maps.index().points.n_obs, maps.index().lines.n, maps.index().lines.n_obs});
        }
        plslam_ctx_destroy(ctx);
    } catch (const std::exception& e) {
        std::cerr << e.what() << "\n";
        return 1;
    }
    return 0;
}
