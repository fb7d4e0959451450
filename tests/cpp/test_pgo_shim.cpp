// A C++ client of plslam_amd/host/pgo.hpp: reads a drifted map written by tests/test_gpu_pgo_shim.py (meta.txt and raw .bin
// arrays), runs PLSLAM::pgo::run and writes the keyframe poses, the points and the per-trial chi' back as raw arrays.
#include <cstdio>
#include <fstream>
#include <vector>

#include "../../plslam_amd/host/pgo.hpp"

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
    int n_kf = 0, npt = 0;
    std::FILE* m = std::fopen((d + "/meta.txt").c_str(), "r");
    if (!m || std::fscanf(m, "%d %d", &n_kf, &npt) != 2) return 2;
    std::fclose(m);
    const auto T = rd<double>(d + "/T.bin"), x = rd<double>(d + "/x.bin"), lc_pose = rd<double>(d + "/lc_pose.bin");
    const auto valid = rd<uint8_t>(d + "/valid.bin");
    const auto fg = rd<int32_t>(d + "/fg.bin"), lc_idx = rd<int32_t>(d + "/lc_idx.bin");
    const auto aptr = rd<int32_t>(d + "/aptr.bin"), aidx = rd<int32_t>(d + "/aidx.bin"), dptr = rd<int32_t>(d + "/dptr.bin");
    const auto pvalid = rd<uint8_t>(d + "/pvalid.bin");
    const auto X = rd<double>(d + "/X.bin"), med = rd<double>(d + "/med.bin"), dirs = rd<double>(d + "/dirs.bin");
    std::vector<PLSLAM::pgo::Keyframe> kfs(n_kf);
    for (int k = 0; k < n_kf; ++k) {
        kfs[k].present = valid[k] != 0;
        for (int a = 0; a < 16; ++a) kfs[k].T_kf_w[a] = T[16 * k + a];
        for (int a = 0; a < 6; ++a) kfs[k].x_kf_w[a] = x[6 * k + a];
    }
    std::vector<PLSLAM::pgo::Landmark> pts(npt), lns;
    for (int j = 0; j < npt; ++j) {
        pts[j].present = pvalid[j] != 0;
        for (int a = 0; a < 3; ++a) { pts[j].X[a] = X[3 * j + a]; pts[j].med_obs_dir[a] = med[3 * j + a]; }
        pts[j].dir_list.assign(dirs.begin() + 3 * dptr[j], dirs.begin() + 3 * dptr[j + 1]);
    }
    std::vector<std::vector<int>> pk(n_kf), lk(n_kf);
    for (int k = 0; k < n_kf; ++k) pk[k].assign(aidx.begin() + aptr[k], aidx.begin() + aptr[k + 1]);
    plslam_ctx* ctx = nullptr;
    if (plslam_ctx_create(0, &ctx) != PLSLAM_OK) return 3;
    std::vector<plslam_pgo_trial> trace;
    const plslam_pgo_result r = PLSLAM::pgo::run(ctx, PLSLAM::pgo::Params{}, kfs, fg, lc_idx, lc_pose, pts, pk, lns, lk, &trace);
    plslam_ctx_destroy(ctx);
    std::vector<double> To, xo, Xo, mo, dout, tr;
    for (auto& k : kfs) { To.insert(To.end(), k.T_kf_w, k.T_kf_w + 16); xo.insert(xo.end(), k.x_kf_w, k.x_kf_w + 6); }
    for (auto& p : pts) {
        Xo.insert(Xo.end(), p.X, p.X + 3);
        mo.insert(mo.end(), p.med_obs_dir, p.med_obs_dir + 3);
        dout.insert(dout.end(), p.dir_list.begin(), p.dir_list.end());
    }
    for (auto& t : trace) tr.push_back(t.chi_new);
    wr(d + "/T_out.bin", To); wr(d + "/x_out.bin", xo); wr(d + "/X_out.bin", Xo); wr(d + "/med_out.bin", mo);
    wr(d + "/dirs_out.bin", dout); wr(d + "/trace.bin", tr);
    std::printf("trials %d iterations %d\n", r.trials, r.iterations);
    return 0;
}
