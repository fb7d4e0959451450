// A C++ client of plslam_amd/host/gba.hpp: reads a map written by tests/test_gpu_gba_shim.py (meta.txt and raw .bin arrays),
// runs PLSLAM::gba::run and writes the keyframe poses, the landmarks and the per-solve trace back as raw arrays.
#include <cstdio>
#include <fstream>
#include <vector>

#include "../../plslam_amd/host/gba.hpp"

template <class T> static std::vector<T> rd(const std::string& p)
{
    std::ifstream f(p, std::ios::binary | std::ios::ate);
    const size_t n = (size_t)f.tellg();
    std::vector<T> v(n / sizeof(T));
    f.seekg(0);
    f.read((char*)v.data(), (std::streamsize)n);
    return v;
}
template <class T> static void wr(const std::string& p, const std::vector<T>& v)
{
    std::ofstream(p, std::ios::binary).write((const char*)v.data(), (std::streamsize)(v.size() * sizeof(T)));
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
    std::vector<PLSLAM::gba::Keyframe> kfs(n_kf);
    for (int k = 0; k < n_kf; ++k) {
        kfs[k].kf_idx = k;
        for (int a = 0; a < 16; ++a) kfs[k].T_kf_w[a] = T[16 * k + a];
        for (int a = 0; a < 6; ++a) kfs[k].x_kf_w[a] = k ? x[6 * (k - 1) + a] : 0.0;
    }
    std::vector<PLSLAM::gba::Landmark> pts(npt), lns(nls);
    for (int j = 0; j < npt; ++j) for (int a = 0; a < 3; ++a) pts[j].X[a] = Xw[3 * j + a];
    for (int j = 0; j < nls; ++j) for (int a = 0; a < 6; ++a) lns[j].X[a] = Lw[6 * j + a];
    for (size_t o = 0; o < po.size() / 6; ++o) {
        pts[po[6 * o + 1]].kf_obs.push_back(po[6 * o + 3]);
        pts[po[6 * o + 1]].obs.insert(pts[po[6 * o + 1]].obs.end(), &uv[2 * o], &uv[2 * o + 2]);
    }
    for (size_t o = 0; o < lo.size() / 6; ++o) {
        lns[lo[6 * o + 1]].kf_obs.push_back(lo[6 * o + 3]);
        lns[lo[6 * o + 1]].obs.insert(lns[lo[6 * o + 1]].obs.end(), &ll[3 * o], &ll[3 * o + 3]);
    }
    plslam_ctx* ctx = nullptr;
    if (plslam_ctx_create(0, &ctx) != PLSLAM_OK) return 3;
    const plslam_cam cam{fx, fy, cx, cy, 0.0, 0, 0};
    std::vector<plslam_gba_solve> trace;
    PLSLAM::gba::run(ctx, cam, PLSLAM::gba::Params{}, kfs, pts, lns, &trace);
    plslam_ctx_destroy(ctx);
    std::vector<double> To, Xo, Lo, tr;
    for (int k = 1; k < n_kf; ++k) To.insert(To.end(), kfs[k].T_kf_w, kfs[k].T_kf_w + 16);
    for (auto& p : pts) Xo.insert(Xo.end(), p.X, p.X + 3);
    for (auto& l : lns) Lo.insert(Lo.end(), l.X, l.X + 6);
    for (auto& t : trace) { tr.push_back(t.lambda); tr.push_back(t.err_raw); tr.push_back(t.dx_norm); }
    wr(d + "/T_out.bin", To); wr(d + "/Xw_out.bin", Xo); wr(d + "/Lw_out.bin", Lo); wr(d + "/trace.bin", tr);
    std::printf("solves %zu\n", trace.size());
    return 0;
}
