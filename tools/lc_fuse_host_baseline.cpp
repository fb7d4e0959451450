// What a caller does for loopClosureFuseLandmarks (src/mapHandler.cpp:4412-4687) WITHOUT plslam_lc_fuse_run when its map image
// lives on the device: download the image, fuse on the host containers, re-pack and upload the whole image.  Compiled and run by
// tools/lc_fuse_bench.py; reads the files that tool writes, prints one JSON line of medians in microseconds.
// The host fusion works on vectors per landmark (kf_obs_list, obs_list) and per keyframe (the features' idx), as the reference
// does; it keeps the documented deviations of the call (skips instead of undefined behaviour) and leaves out the directions.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "../plslam_amd/host/lc_fuse.hpp"

using namespace PLSLAM::map_insert;
using namespace PLSLAM::lc_fuse;
using Clock = std::chrono::steady_clock;

template <class T> static std::vector<T> rd(const std::string& dir, const std::string& name)
{
    std::ifstream f(dir + "/" + name + ".bin", std::ios::binary | std::ios::ate);
    if (!f) throw std::runtime_error("missing " + name);
    std::vector<T> v((size_t)f.tellg() / sizeof(T));
    f.seekg(0);
    f.read(reinterpret_cast<char*>(v.data()), (std::streamsize)(v.size() * sizeof(T)));
    return v;
}
static HostKind kind_in(const std::string& d, const std::string& k)
{
    HostKind h;
    h.valid = rd<uint8_t>(d, k + "_valid"); h.inlier = rd<uint8_t>(d, k + "_inlier"); h.X = rd<double>(d, k + "_X");
    h.obs_val = rd<double>(d, k + "_obs_val"); h.obs_ptr = rd<int32_t>(d, k + "_obs_ptr"); h.obs_kf = rd<int32_t>(d, k + "_obs_kf");
    h.feat_ptr = rd<int32_t>(d, k + "_feat_ptr"); h.feat_idx = rd<int32_t>(d, k + "_feat_idx");
    return h;
}
struct KindArgs { std::vector<int32_t> tuples, entry_ptr; std::vector<double> P0, obs0, P1, obs1; };
static KindArgs args_in(const std::string& d, const std::string& k)
{
    return KindArgs{rd<int32_t>(d, k + "_tuples"), rd<int32_t>(d, k + "_entry_ptr"), rd<double>(d, k + "_P0"), rd<double>(d, k + "_obs0"),
                    rd<double>(d, k + "_P1"), rd<double>(d, k + "_obs1")};
}
static void xform(const double* T, const double* p, double* o)
{
    for (int i = 0; i < 3; ++i) o[i] = ((T[4 * i] * p[0] + T[4 * i + 1] * p[1]) + T[4 * i + 2] * p[2]) + T[4 * i + 3];
}

// one kind: the image's arrays -> containers, the loop of :4417-4537, containers -> arrays
static void fuse_kind(HostKind& h, const std::vector<uint8_t>& kf_valid, const std::vector<int32_t>& lc, const std::vector<double>& T,
                      const KindArgs& a, int dl, int dv, std::vector<int32_t>& graph)
{
    const int32_t n = (int32_t)h.valid.size(), nk = (int32_t)kf_valid.size();
    struct Lm { std::vector<int32_t> kf; std::vector<double> obs; };
    std::vector<Lm> L((size_t)n);
    for (int32_t x = 0; x < n; ++x) {
        L[x].kf.assign(h.obs_kf.begin() + h.obs_ptr[x], h.obs_kf.begin() + h.obs_ptr[x + 1]);
        L[x].obs.assign(h.obs_val.begin() + (size_t)dv * h.obs_ptr[x], h.obs_val.begin() + (size_t)dv * h.obs_ptr[x + 1]);
    }
    auto inc = [&](int32_t i, int32_t j) {
        if (i >= 0 && i < nk && j >= 0 && j < nk) { ++graph[(size_t)i * nk + j]; ++graph[(size_t)j * nk + i]; }
    };
    auto feat = [&](int32_t kf, int32_t ldx) -> int32_t* {
        return ldx >= 0 && ldx < h.feat_ptr[kf + 1] - h.feat_ptr[kf] ? &h.feat_idx[(size_t)h.feat_ptr[kf] + ldx] : nullptr;
    };
    auto ok = [&](int32_t x) { return x >= 0 && x < n; };
    for (size_t e = 0; e + 1 < a.entry_ptr.size(); ++e) {
        const int32_t kp = lc[3 * e], kc = lc[3 * e + 1];
        if (lc[3 * e + 2] != 1 || !kf_valid[kp] || !kf_valid[kc]) continue;
        for (int32_t t = a.entry_ptr[e]; t < a.entry_ptr[e + 1]; ++t) {
            const int32_t la = a.tuples[4 * (size_t)t], l0 = a.tuples[4 * (size_t)t + 1], lb = a.tuples[4 * (size_t)t + 2], l1 = a.tuples[4 * (size_t)t + 3];
            if ((la != -1 && !ok(la)) || (lb != -1 && !ok(lb))) continue;
            int32_t *f0 = feat(kp, l0), *f1 = feat(kc, l1);
            if (la == -1 && lb != -1) {
                if (!f0 || *f0 == PLSLAM_FEAT_NULL || !h.valid[lb]) continue;
                *f0 = lb;
                L[lb].kf.push_back(kp);
                L[lb].obs.insert(L[lb].obs.end(), a.obs0.begin() + (size_t)dv * t, a.obs0.begin() + (size_t)dv * (t + 1));
                for (int32_t k : L[lb].kf) inc(k, kc);
            } else if (la != -1 && lb == -1) {
                if (!f1 || *f1 == PLSLAM_FEAT_NULL || !h.valid[la]) continue;
                *f1 = la;
                L[la].kf.push_back(kc);
                L[la].obs.insert(L[la].obs.end(), a.obs1.begin() + (size_t)dv * t, a.obs1.begin() + (size_t)dv * (t + 1));
                for (int32_t k : L[la].kf) inc(k, kp);
            } else if (la == -1) {
                if (!f0 || !f1 || *f0 == PLSLAM_FEAT_NULL || *f1 == PLSLAM_FEAT_NULL) continue;
                *f0 = *f1 = (int32_t)L.size();
                Lm lm;
                lm.kf = {kp, kc};
                lm.obs.insert(lm.obs.end(), a.obs0.begin() + (size_t)dv * t, a.obs0.begin() + (size_t)dv * (t + 1));
                lm.obs.insert(lm.obs.end(), a.obs1.begin() + (size_t)dv * t, a.obs1.begin() + (size_t)dv * (t + 1));
                L.push_back(std::move(lm));
                h.valid.push_back(1);
                h.inlier.push_back(1);
                double X[6];
                xform(&T[16 * (size_t)kp], &a.P0[(size_t)dl * t], X);
                if (dl == 6) xform(&T[16 * (size_t)kp], &a.P0[(size_t)dl * t + 3], X + 3);
                h.X.insert(h.X.end(), X, X + dl);
                inc(kp, kc);
            } else {
                if (!f1 || *f1 == PLSLAM_FEAT_NULL || !h.valid[la] || !h.valid[lb] || la == lb || L[lb].kf.empty()) continue;
                const size_t n_prev = L[la].kf.size();
                for (int32_t j : L[lb].kf)
                    for (size_t i = 0; i < n_prev; ++i) inc(L[la].kf[i], j);
                L[la].kf.insert(L[la].kf.end(), L[lb].kf.begin(), L[lb].kf.end());
                L[la].obs.insert(L[la].obs.end(), L[lb].obs.begin(), L[lb].obs.end());
                *f1 = la;
                h.valid[lb] = 0;
                L[lb] = Lm();
            }
        }
    }
    h.obs_ptr.assign(L.size() + 1, 0);
    h.obs_kf.clear();
    h.obs_val.clear();
    for (size_t x = 0; x < L.size(); ++x) {
        h.obs_kf.insert(h.obs_kf.end(), L[x].kf.begin(), L[x].kf.end());
        h.obs_val.insert(h.obs_val.end(), L[x].obs.begin(), L[x].obs.end());
        h.obs_ptr[x + 1] = (int32_t)h.obs_kf.size();
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
    const int reps = std::max(1, atoi(argv[2]));
    try {
        const auto lc = rd<int32_t>(d, "lc_idx");
        const auto T = rd<double>(d, "T_kf_w");
        HostImage h0;
        h0.kf_valid = rd<uint8_t>(d, "kf_valid");
        h0.x_kf_w = rd<double>(d, "x_kf_w");
        h0.points = kind_in(d, "pt");
        h0.lines = kind_in(d, "ls");
        const KindArgs ap = args_in(d, "pt"), al = args_in(d, "ls");
        plslam_ctx* ctx = nullptr;
        check(plslam_ctx_create(0, &ctx), "ctx_create");
        std::vector<double> t_down, t_fuse, t_up;
        int64_t n_after = 0, n_obs_after = 0, g_sum = 0;
        {
            MapImages maps(ctx);
            for (int r = 0; r < reps + 2; ++r) {
                maps.upload(h0);                                        // the state before the loop closure (not timed)
                hip_check(hipDeviceSynchronize(), "sync");
                HostImage h;
                const auto t0 = Clock::now();
                maps.download(h);
                const auto t1 = Clock::now();
                std::vector<int32_t> graph(h.kf_valid.size() * h.kf_valid.size(), 0);
                fuse_kind(h.points, h.kf_valid, lc, T, ap, 3, 2, graph);
                fuse_kind(h.lines, h.kf_valid, lc, T, al, 6, 3, graph);
                const auto t2 = Clock::now();
                maps.upload(h);
                hip_check(hipDeviceSynchronize(), "sync");
                const auto t3 = Clock::now();
                if (r >= 2) {
                    t_down.push_back(std::chrono::duration<double, std::micro>(t1 - t0).count());
                    t_fuse.push_back(std::chrono::duration<double, std::micro>(t2 - t1).count());
                    t_up.push_back(std::chrono::duration<double, std::micro>(t3 - t2).count());
                }
                n_after = (int64_t)h.points.valid.size();
                n_obs_after = (int64_t)h.points.obs_kf.size();
                g_sum = 0;
                for (int32_t v : graph) g_sum += v;
            }
        }
        plslam_ctx_destroy(ctx);
        std::cout << "{\"download_us\": " << median(t_down) << ", \"fuse_us\": " << median(t_fuse) << ", \"upload_us\": " << median(t_up)
                  << ", \"n_pt_after\": " << n_after << ", \"n_pt_obs_after\": " << n_obs_after << ", \"graph_sum\": " << g_sum << "}\n";
    } catch (const std::exception& e) {
        std::cerr << e.what() << "\n";
        return 1;
    }
    return 0;
}
