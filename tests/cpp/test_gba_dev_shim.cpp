// A C++ client of the resident route (plslam_amd/host/gba.hpp: runResident over plslam_amd/host/local_map.hpp's LocalMapIndex): reads
// a map written by tests/test_gpu_gba_dev_shim.py (meta.txt and raw .bin arrays, the files of test_gba_shim.cpp), runs the host
// route PLSLAM::gba::run and the resident route on the same map and compares them bit for bit.  Exit status 0: identical.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <vector>

#include "../../plslam_amd/host/gba.hpp"
#include "../../plslam_amd/host/local_map.hpp"

template <class T> static std::vector<T> rd(const std::string& p)
{
    std::ifstream f(p, std::ios::binary | std::ios::ate);
    const size_t n = (size_t)f.tellg();
    std::vector<T> v(n / sizeof(T));
    f.seekg(0);
    f.read((char*)v.data(), (std::streamsize)n);
    return v;
}
static bool same(const std::vector<double>& a, const std::vector<double>& b, const char* what)
{
    const bool ok = a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * 8) == 0);
    if (!ok) std::printf("DIFFERENT: %s\n", what);
    return ok;
}

int main(int argc, char** argv)
{
    if (argc < 2) return 2;
    const std::string d = argv[1];
    int n_kf = 0, npt = 0, nls = 0;
    double fx, fy, cx, cy;
    std::FILE* m = std::fopen((d + "/meta.txt").c_str(), "r");
    if (!m || std::fscanf(m, "%d %d %d %lf %lf %lf %lf", &n_kf, &npt, &nls, &fx, &fy, &cx, &cy) != 7) return 2;
    std::fclose(m);
    const auto T = rd<double>(d + "/T.bin"), x = rd<double>(d + "/x.bin"), Xw = rd<double>(d + "/Xw.bin"), Lw = rd<double>(d + "/Lw.bin");
    const auto po = rd<int32_t>(d + "/pt_obs.bin"), lo = rd<int32_t>(d + "/ls_obs.bin");
    const auto uv = rd<double>(d + "/pt_uv.bin"), ll = rd<double>(d + "/ls_l.bin");
    namespace G = PLSLAM::gba;
    namespace M = PLSLAM::local_map;
    // the same map in the containers of the two headers
    std::vector<G::Keyframe> kfs(n_kf);
    std::vector<M::KeyFrame> mkfs(n_kf);
    for (int k = 0; k < n_kf; ++k) {
        kfs[k].kf_idx = k;
        for (int a = 0; a < 16; ++a) kfs[k].T_kf_w[a] = T[16 * k + a];
        for (int a = 0; a < 6; ++a) mkfs[k].x_kf_w[a] = kfs[k].x_kf_w[a] = k ? x[6 * (k - 1) + a] : 0.0;
    }
    std::vector<G::Landmark> pts(npt), lns(nls);
    std::vector<M::Landmark> mpts(npt), mlns(nls);
    for (int j = 0; j < npt; ++j) for (int a = 0; a < 3; ++a) mpts[j].X[a] = pts[j].X[a] = Xw[3 * j + a];
    for (int j = 0; j < nls; ++j) for (int a = 0; a < 6; ++a) mlns[j].X[a] = lns[j].X[a] = Lw[6 * j + a];
    for (size_t o = 0; o < po.size() / 6; ++o) {
        const int j = po[6 * o + 1];
        pts[j].kf_obs.push_back(po[6 * o + 3]);
        pts[j].obs.insert(pts[j].obs.end(), &uv[2 * o], &uv[2 * o] + 2);
        mpts[j].kf_obs_list = pts[j].kf_obs;
        mpts[j].obs_list = pts[j].obs;
    }
    for (size_t o = 0; o < lo.size() / 6; ++o) {
        const int j = lo[6 * o + 1];
        lns[j].kf_obs.push_back(lo[6 * o + 3]);
        lns[j].obs.insert(lns[j].obs.end(), &ll[3 * o], &ll[3 * o] + 3);
        mlns[j].kf_obs_list = lns[j].kf_obs;
        mlns[j].obs_list = lns[j].obs;
    }
    plslam_ctx* ctx = nullptr;
    if (plslam_ctx_create(0, &ctx) != PLSLAM_OK) return 3;
    const plslam_cam cam{fx, fy, cx, cy, 0.0, 0, 0};
    int rc = 0;
    try {
        std::vector<plslam_gba_solve> tr_host, tr_dev;
        G::run(ctx, cam, G::Params{}, kfs, pts, lns, &tr_host);
        std::vector<int32_t> kf_list;
        std::vector<double> T_out, x_out, Xp, Xl;
        {
            M::LocalMapIndex ix(ctx);
            ix.pack(mkfs, mpts, mlns);
            G::runResident(ctx, cam, G::Params{}, ix.handle(), ix.index(), ix.writeBackDst(), T, kf_list, T_out, x_out, &tr_dev);
            ix.downloadLandmarks(Xp, Xl);
        }
        std::vector<double> To, Xo, Lo, th, tdv;
        for (int k = 1; k < n_kf; ++k) To.insert(To.end(), kfs[k].T_kf_w, kfs[k].T_kf_w + 16);
        for (auto& p : pts) Xo.insert(Xo.end(), p.X, p.X + 3);
        for (auto& l : lns) Lo.insert(Lo.end(), l.X, l.X + 6);
        for (auto& t : tr_host) { th.push_back(t.lambda); th.push_back(t.err_raw); th.push_back(t.err); th.push_back(t.dx_norm); th.push_back(t.n_singular); th.push_back(t.accepted); }
        for (auto& t : tr_dev) { tdv.push_back(t.lambda); tdv.push_back(t.err_raw); tdv.push_back(t.err); tdv.push_back(t.dx_norm); tdv.push_back(t.n_singular); tdv.push_back(t.accepted); }
        bool ok = (int)kf_list.size() == n_kf - 1;
        for (size_t k = 0; ok && k < kf_list.size(); ++k) ok = kf_list[k] == (int32_t)k + 1;
        if (!ok) std::printf("DIFFERENT: kf_list\n");
        ok = same(T_out, To, "T_kf_w") && ok;
        ok = same(Xp, Xo, "point3D") && ok;
        ok = same(Xl, Lo, "line3D") && ok;
        ok = same(tdv, th, "trace") && ok;
        std::printf("solves %zu %zu\n", tr_host.size(), tr_dev.size());
        rc = ok && !tr_host.empty() ? 0 : 1;
    } catch (const std::exception& e) {
        std::printf("%s\n", e.what());
        rc = 4;
    }
    plslam_ctx_destroy(ctx);
    return rc;
}
