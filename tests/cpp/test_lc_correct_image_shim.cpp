// A C++ client of plslam_amd/host/pgo.hpp's two routes on the same packed map, written by tests/test_gpu_lc_correct_image_shim.py
// (meta.txt and raw .bin arrays): PLSLAM::pgo::run on containers with the map_*_kf_idx lists, and PLSLAM::pgo::runResident on the
// device-resident image (local_map.hpp's LocalMapIndex) with its dir lists (map_lists.hpp's MapLists), which takes no list.  Both
// results are written back as raw arrays: keyframes, landmarks and dir lists of each route.
#include <cstdio>
#include <fstream>
#include <vector>

#include "../../plslam_amd/host/local_map.hpp"
#include "../../plslam_amd/host/map_lists.hpp"
#include "../../plslam_amd/host/pgo.hpp"

using namespace PLSLAM;

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

struct KindIn {
    std::vector<uint8_t> valid;
    std::vector<double> X, obs_val, dir;
    std::vector<int32_t> obs_ptr, obs_kf, aptr, aidx;
    KindIn(const std::string& d, const std::string& t)
        : valid(rd<uint8_t>(d + "/" + t + "_valid.bin")), X(rd<double>(d + "/" + t + "_X.bin")), obs_val(rd<double>(d + "/" + t + "_obs_val.bin")),
          dir(rd<double>(d + "/" + t + "_dir.bin")), obs_ptr(rd<int32_t>(d + "/" + t + "_obs_ptr.bin")),
          obs_kf(rd<int32_t>(d + "/" + t + "_obs_kf.bin")), aptr(rd<int32_t>(d + "/" + t + "_aptr.bin")), aidx(rd<int32_t>(d + "/" + t + "_aidx.bin"))
    {
    }
};

int main(int argc, char** argv)
{
    if (argc < 2) return 2;
    const std::string d = argv[1];
    int n_kf = 0;
    std::FILE* m = std::fopen((d + "/meta.txt").c_str(), "r");
    if (!m || std::fscanf(m, "%d", &n_kf) != 1) return 2;
    std::fclose(m);
    const auto T = rd<double>(d + "/T.bin"), x = rd<double>(d + "/x.bin"), lc_pose = rd<double>(d + "/lc_pose.bin");
    const auto valid = rd<uint8_t>(d + "/valid.bin");
    const auto fg = rd<int32_t>(d + "/fg.bin"), lc_idx = rd<int32_t>(d + "/lc_idx.bin");
    const KindIn in[2] = {KindIn(d, "pt"), KindIn(d, "ls")};

    std::vector<pgo::Keyframe> kfs(n_kf);
    std::vector<local_map::KeyFrame> lkfs(n_kf);
    for (int k = 0; k < n_kf; ++k) {
        kfs[k].present = lkfs[k].present = valid[k] != 0;
        for (int a = 0; a < 16; ++a) kfs[k].T_kf_w[a] = T[16 * k + a];
        for (int a = 0; a < 6; ++a) kfs[k].x_kf_w[a] = lkfs[k].x_kf_w[a] = x[6 * k + a];
    }
    std::vector<pgo::Keyframe> kfs_res = kfs;
    // the same landmarks as the containers of the host route and as the image of the resident one
    std::vector<pgo::Landmark> lms[2];
    std::vector<local_map::Landmark> llms[2];
    std::vector<std::vector<int>> kf_idx[2];
    map_lists::HostLists hl;
    for (int k = 0; k < 2; ++k) {
        const KindIn& K = in[k];
        const int dl = k ? 6 : 3, dv = k ? 3 : 2;
        const size_t n = K.valid.size();
        lms[k].resize(n);
        llms[k].resize(n);
        for (size_t j = 0; j < n; ++j) {
            lms[k][j].present = llms[k][j].present = K.valid[j] != 0;
            for (int a = 0; a < dl; ++a) lms[k][j].X[a] = llms[k][j].X[a] = K.X[dl * j + a];
            for (int a = 0; a < 3; ++a) lms[k][j].med_obs_dir[a] = 0.0;
            lms[k][j].dir_list.assign(K.dir.begin() + 3 * K.obs_ptr[j], K.dir.begin() + 3 * K.obs_ptr[j + 1]);
            llms[k][j].kf_obs_list.assign(K.obs_kf.begin() + K.obs_ptr[j], K.obs_kf.begin() + K.obs_ptr[j + 1]);
            llms[k][j].obs_list.assign(K.obs_val.begin() + dv * K.obs_ptr[j], K.obs_val.begin() + dv * K.obs_ptr[j + 1]);
        }
        kf_idx[k].resize(n_kf);
        for (int s = 0; s < n_kf; ++s) kf_idx[k][s].assign(K.aidx.begin() + K.aptr[s], K.aidx.begin() + K.aptr[s + 1]);
        map_lists::HostKind& H = k ? hl.lines : hl.points;
        H.dir = K.dir;
        H.desc.assign(32 * K.obs_kf.size(), 0);
        if (k) H.pts.assign(4 * K.obs_kf.size(), 0.0);
        H.med_idx.assign(n, 0);
        H.med_desc.assign(32 * n, 0);
    }

    plslam_ctx* ctx = nullptr;
    if (plslam_ctx_create(0, &ctx) != PLSLAM_OK) return 3;
    int rc = 0;
    try {
        const plslam_pgo_result r0 = pgo::run(ctx, pgo::Params{}, kfs, fg, lc_idx, lc_pose, lms[0], kf_idx[0], lms[1], kf_idx[1]);
        plslam_lc_image_counts counts{};
        std::vector<double> Xr[2], xr((size_t)n_kf * 6);
        map_lists::HostLists out;
        plslam_pgo_result r1{};
        {
            local_map::LocalMapIndex image(ctx);
            image.pack(lkfs, llms[0], llms[1]);
            map_lists::MapLists lists(ctx);
            lists.upload(hl, image.index(), false);
            r1 = pgo::runResident(ctx, pgo::Params{}, kfs_res, fg, lc_idx, lc_pose, image.index(), &lists.lists(), &counts);
            image.downloadLandmarks(Xr[0], Xr[1]);
            lists.download(out, image.index());
            local_map::hip_check(hipMemcpy(xr.data(), image.index().x_kf_w, xr.size() * 8, hipMemcpyDeviceToHost), "hipMemcpy");
        }
        std::vector<double> To, xo, Tr, xo_r;
        for (auto& k : kfs) { To.insert(To.end(), k.T_kf_w, k.T_kf_w + 16); xo.insert(xo.end(), k.x_kf_w, k.x_kf_w + 6); }
        for (auto& k : kfs_res) { Tr.insert(Tr.end(), k.T_kf_w, k.T_kf_w + 16); xo_r.insert(xo_r.end(), k.x_kf_w, k.x_kf_w + 6); }
        wr(d + "/run_T.bin", To); wr(d + "/run_x.bin", xo); wr(d + "/res_T.bin", Tr); wr(d + "/res_x.bin", xo_r); wr(d + "/res_image_x.bin", xr);
        for (int k = 0; k < 2; ++k) {
            const std::string t = k ? "ls" : "pt";
            std::vector<double> Xo, dout;
            for (auto& p : lms[k]) {
                Xo.insert(Xo.end(), p.X, p.X + (k ? 6 : 3));
                dout.insert(dout.end(), p.dir_list.begin(), p.dir_list.end());
            }
            wr(d + "/run_" + t + "_X.bin", Xo); wr(d + "/run_" + t + "_dir.bin", dout);
            wr(d + "/res_" + t + "_X.bin", Xr[k]); wr(d + "/res_" + t + "_dir.bin", k ? out.lines.dir : out.points.dir);
        }
        wr(d + "/counts.bin", std::vector<int32_t>{counts.n_pt, counts.n_ls, counts.n_pt_dirs, counts.n_ls_dirs});
        std::printf("trials %d %d iterations %d %d\n", r0.trials, r1.trials, r0.iterations, r1.iterations);
        if (r0.trials != r1.trials || r0.iterations != r1.iterations) rc = 4;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "%s\n", e.what());
        rc = 5;
    }
    plslam_ctx_destroy(ctx);
    return rc;
}
