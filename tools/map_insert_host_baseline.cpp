// map_insert_host_baseline.cpp -- what a caller does WITHOUT plslam_map_insert_* to keep the device image of the map current over
// one keyframe: mutate the host containers with the insertion loops (src/mapHandler.cpp:280-360, :428-527; :601-629, :716-749;
// the landmark positions are computed, the observation directions are not: the baseline does a little less than the reference),
// then re-pack and upload the WHOLE image with plslam_amd/host/local_map.hpp (LocalMapIndex::pack) -- once after the KF <-> KF
// pass (plslam_local_map_candidates must see it) and once after the map <-> KF pass.  tools/map_insert_bench.py writes the inputs,
// builds and runs this program and reports its medians next to the device calls'.
//   usage: map_insert_host_baseline <dir> <reps>      one JSON line: medians in microseconds
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <vector>

#include "../plslam_amd/host/local_map.hpp"

using namespace PLSLAM::local_map;

template <class T> static std::vector<T> rd(const std::string& dir, const std::string& name)
{
    std::ifstream f(dir + "/" + name + ".bin", std::ios::binary | std::ios::ate);
    if (!f) throw std::runtime_error("missing " + name);
    std::vector<T> v((size_t)f.tellg() / sizeof(T));
    f.seekg(0);
    f.read(reinterpret_cast<char*>(v.data()), (std::streamsize)(v.size() * sizeof(T)));
    return v;
}
struct Tables { std::vector<int32_t> m12, m2k; std::vector<double> P1, o1, o2; };

static std::vector<Landmark> landmarks(const std::string& d, const std::string& k, int dl, int dv)
{
    const auto valid = rd<uint8_t>(d, k + "_valid"), inl = rd<uint8_t>(d, k + "_inlier");
    const auto X = rd<double>(d, k + "_X"), val = rd<double>(d, k + "_obs_val");
    const auto ptr = rd<int32_t>(d, k + "_obs_ptr"), okf = rd<int32_t>(d, k + "_obs_kf");
    std::vector<Landmark> out(valid.size());
    for (size_t i = 0; i < out.size(); ++i) {
        out[i].present = valid[i] != 0;
        out[i].inlier = inl[i] != 0;
        for (int a = 0; a < dl; ++a) out[i].X[a] = X[dl * i + a];
        out[i].kf_obs_list.assign(okf.begin() + ptr[i], okf.begin() + ptr[i + 1]);
        out[i].obs_list.assign(val.begin() + (size_t)dv * ptr[i], val.begin() + (size_t)dv * ptr[i + 1]);
    }
    return out;
}
static void xf(const double* T, const double* p, double* o)
{
    for (int i = 0; i < 3; ++i) o[i] = (T[4 * i] * p[0] + T[4 * i + 1] * p[1] + T[4 * i + 2] * p[2]) + T[4 * i + 3];
}
static void append(Landmark& m, int kf2, const double* obs, int dv, std::vector<int32_t>& graph)
{
    m.kf_obs_list.push_back(kf2);
    m.obs_list.insert(m.obs_list.end(), obs, obs + dv);
    for (int o : m.kf_obs_list)
        if (o != kf2) graph[o]++;
}
static void kf2kf(std::vector<Feature>& prev, std::vector<Feature>& curr, std::vector<Landmark>& lms, const Tables& t, int dl, int dv,
                  int kf1, int kf2, const double* T1, std::vector<int32_t>& graph)
{
    for (size_t i1 = 0; i1 < t.m12.size(); ++i1) {
        const int i2 = t.m12[i1];
        if (i2 < 0 || !prev[i1].present || !curr[i2].present) continue;
        if (prev[i1].idx == -1) {
            prev[i1].idx = curr[i2].idx = (int)lms.size();
            Landmark m;
            xf(T1, &t.P1[dl * i1], m.X);
            if (dl == 6) xf(T1, &t.P1[dl * i1 + 3], m.X + 3);
            m.kf_obs_list = {kf1, kf2};
            m.obs_list.assign(&t.o1[dv * i1], &t.o1[dv * i1] + dv);
            m.obs_list.insert(m.obs_list.end(), &t.o2[dv * i2], &t.o2[dv * i2] + dv);
            lms.push_back(std::move(m));
            graph[kf1]++;
        } else if (prev[i1].idx >= 0 && prev[i1].idx < (int)lms.size() && lms[prev[i1].idx].present) {
            curr[i2].idx = prev[i1].idx;
            append(lms[prev[i1].idx], kf2, &t.o2[dv * i2], dv, graph);
        }
    }
}
static void map2kf(std::vector<Feature>& curr, std::vector<Landmark>& lms, const Tables& t, int dv, int kf2, std::vector<int32_t>& graph)
{
    for (size_t lm = 0; lm < t.m2k.size(); ++lm) {
        const int i2 = t.m2k[lm];
        if (i2 < 0 || !curr[i2].present) continue;
        curr[i2].idx = (int)lm;
        append(lms[lm], kf2, &t.o2[dv * i2], dv, graph);
    }
}
static double median(std::vector<double> v)
{
    std::sort(v.begin(), v.end());
    return v[v.size() / 2];
}

int main(int argc, char** argv)
{
    if (argc < 3) return 2;
    const std::string d = argv[1];
    const int reps = std::atoi(argv[2]);
    try {
        const auto p = rd<int32_t>(d, "params");       // kf1, kf2
        const auto T = rd<double>(d, "T");
        const auto kv = rd<uint8_t>(d, "kf_valid");
        const auto x = rd<double>(d, "x_kf_w");
        std::vector<KeyFrame> kfs0(kv.size());
        const auto pfp = rd<int32_t>(d, "pt_feat_ptr"), pfi = rd<int32_t>(d, "pt_feat_idx"), lfp = rd<int32_t>(d, "ls_feat_ptr"),
                   lfi = rd<int32_t>(d, "ls_feat_idx");
        for (size_t i = 0; i < kfs0.size(); ++i) {
            kfs0[i].present = kv[i] != 0;
            for (int a = 0; a < 6; ++a) kfs0[i].x_kf_w[a] = x[6 * i + a];
            for (int32_t f = pfp[i]; f < pfp[i + 1]; ++f) kfs0[i].stereo_pt.push_back(Feature{pfi[f] != PLSLAM_FEAT_NULL, pfi[f]});
            for (int32_t f = lfp[i]; f < lfp[i + 1]; ++f) kfs0[i].stereo_ls.push_back(Feature{lfi[f] != PLSLAM_FEAT_NULL, lfi[f]});
        }
        const std::vector<Landmark> pts0 = landmarks(d, "pt", 3, 2), lns0 = landmarks(d, "ls", 6, 3);
        Tables tp{rd<int32_t>(d, "pt_matches_12"), rd<int32_t>(d, "pt_map_to_kf"), rd<double>(d, "pt_P1"), rd<double>(d, "pt_obs1"), rd<double>(d, "pt_obs2")};
        Tables tl{rd<int32_t>(d, "ls_matches_12"), rd<int32_t>(d, "ls_map_to_kf"), rd<double>(d, "ls_P1"), rd<double>(d, "ls_obs1"), rd<double>(d, "ls_obs2")};
        plslam_ctx* ctx = nullptr;
        check(plslam_ctx_create(0, &ctx), "ctx_create");
        std::vector<double> t_mut_a, t_pack_a, t_mut_b, t_pack_b;
        {
            LocalMapIndex ix(ctx);
            using clk = std::chrono::steady_clock;
            auto us = [](clk::time_point a, clk::time_point b) { return std::chrono::duration<double, std::micro>(b - a).count(); };
            for (int r = 0; r < reps + 2; ++r) {
                std::vector<KeyFrame> kfs = kfs0;
                std::vector<Landmark> pts = pts0, lns = lns0;
                std::vector<int32_t> graph(kfs.size(), 0);
                const auto t0 = clk::now();
                kf2kf(kfs[p[0]].stereo_pt, kfs[p[1]].stereo_pt, pts, tp, 3, 2, p[0], p[1], T.data(), graph);
                kf2kf(kfs[p[0]].stereo_ls, kfs[p[1]].stereo_ls, lns, tl, 6, 3, p[0], p[1], T.data(), graph);
                const auto t1 = clk::now();
                ix.pack(kfs, pts, lns);
                const auto t2 = clk::now();
                map2kf(kfs[p[1]].stereo_pt, pts, tp, 2, p[1], graph);
                map2kf(kfs[p[1]].stereo_ls, lns, tl, 3, p[1], graph);
                const auto t3 = clk::now();
                ix.pack(kfs, pts, lns);
                const auto t4 = clk::now();
                if (r < 2) continue;                   // warm-up
                t_mut_a.push_back(us(t0, t1)); t_pack_a.push_back(us(t1, t2)); t_mut_b.push_back(us(t2, t3)); t_pack_b.push_back(us(t3, t4));
            }
        }
        plslam_ctx_destroy(ctx);
        std::printf("{\"kf2kf_mutate_us\": %.1f, \"kf2kf_repack_upload_us\": %.1f, \"map2kf_mutate_us\": %.1f, \"map2kf_repack_upload_us\": %.1f}\n",
                    median(t_mut_a), median(t_pack_a), median(t_mut_b), median(t_pack_b));
    } catch (const std::exception& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
