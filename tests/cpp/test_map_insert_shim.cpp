// A C++ client of plslam_amd/host/map_insert.hpp: reads a map image and a keyframe's tables written by the Python test, uploads
// the image once and runs the KF <-> KF insertion and then the map <-> KF insertion as MapHandler::addKeyFrame would, the image
// staying on the device in between; writes the final image, the events and row_delta for the test to compare with the
// sequential restatement.
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "../../plslam_amd/host/map_insert.hpp"

using namespace PLSLAM::map_insert;

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
static KindMatches matches(const std::string& d, const std::string& k, bool map2kf)
{
    KindMatches m;
    m.table = rd<int32_t>(d, k + (map2kf ? "_map_to_kf" : "_matches_12"));
    m.P2 = rd<double>(d, k + "_P2"); m.obs2 = rd<double>(d, k + "_obs2");
    if (!map2kf) { m.P1 = rd<double>(d, k + "_P1"); m.obs1 = rd<double>(d, k + "_obs1"); }
    return m;
}
static void events_out(const std::string& d, const std::string& name, const std::vector<Event>& ev)
{
    std::vector<int32_t> e;
    std::vector<double> dir;
    for (const Event& v : ev) {
        e.insert(e.end(), {v.lm, v.i1, v.i2, v.is_new ? 1 : 0});
        dir.insert(dir.end(), v.dir_first, v.dir_first + 3);
        dir.insert(dir.end(), v.dir, v.dir + 3);
    }
    wr(d, "out_" + name + "_ev", e);
    wr(d, "out_" + name + "_dir", dir);
}

int main(int argc, char** argv)
{
    if (argc < 2) return 2;
    const std::string d = argv[1];
    try {
        const auto p = rd<int32_t>(d, "params");       // kf1, kf2
        const auto T = rd<double>(d, "T");             // T_kf1_w, T_kf2_w
        HostImage h;
        h.kf_valid = rd<uint8_t>(d, "kf_valid");
        h.x_kf_w = rd<double>(d, "x_kf_w");
        h.points = kind_in(d, "pt");
        h.lines = kind_in(d, "ls");
        plslam_ctx* ctx = nullptr;
        check(plslam_ctx_create(0, &ctx), "ctx_create");
        {
            MapImages maps(ctx);
            maps.upload(h);
            const Inserted a = maps.insertKF2KF(p[0], p[1], T.data(), T.data() + 16, matches(d, "pt", false), matches(d, "ls", false));
            const Inserted b = maps.insertMap2KF(p[1], T.data() + 16, matches(d, "pt", true), matches(d, "ls", true));
            events_out(d, "a_pt", a.pt_events); events_out(d, "a_ls", a.ls_events);
            events_out(d, "b_pt", b.pt_events); events_out(d, "b_ls", b.ls_events);
            wr(d, "out_a_row_delta", a.row_delta); wr(d, "out_b_row_delta", b.row_delta);
            wr(d, "out_counts", std::vector<int32_t>{a.counts.points.n_events, a.counts.points.n_new, a.counts.points.n_skipped,
                                                     a.counts.lines.n_events, a.counts.lines.n_new, a.counts.lines.n_skipped,
                                                     b.counts.points.n_events, b.counts.points.n_skipped, b.counts.lines.n_events,
                                                     b.counts.lines.n_skipped});
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
