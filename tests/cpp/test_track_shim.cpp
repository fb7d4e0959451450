// A C++ client of plslam_amd/host/track.hpp (tests/test_gpu_track.py::test_cpp_client_tracks_two_pairs): reads the tables of
// the pairs the test wrote (meta.txt: B, then per pair n_pt_prev n_pt_curr n_ls_prev n_ls_curr; p<b>_<field>.bin; params.txt),
// uploads them, runs PLSLAM::TrackBatch on a stream of its own and prints, per pair:
//   pair b <point rows> <line rows> / the point rows (i1 i2) / "P0" and the first point's P / the line rows / "T" and T_inc
// with %.17g, so that the test sees every bit.
#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <vector>

#include "track.hpp"

namespace {

std::vector<void*> g_blocks;

template <class T>
const T* upload(const std::string& path, size_t n)
{
    if (n == 0) return nullptr;
    std::vector<T> v(n);
    std::ifstream f(path, std::ios::binary);
    if (!f.read(reinterpret_cast<char*>(v.data()), (std::streamsize)(n * sizeof(T)))) { std::fprintf(stderr, "short file %s\n", path.c_str()); std::exit(2); }
    void* d = nullptr;
    if (hipMalloc(&d, n * sizeof(T)) != hipSuccess || hipMemcpy(d, v.data(), n * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) {
        std::fprintf(stderr, "upload of %s failed\n", path.c_str());
        std::exit(3);
    }
    g_blocks.push_back(d);
    return static_cast<const T*>(d);
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc < 2) return 2;
    const std::string dir = argv[1];
    std::ifstream meta(dir + "/meta.txt"), prm(dir + "/params.txt");
    int B = 0;
    meta >> B;
    plslam_lc_params p{};
    prm >> p.cam.fx >> p.cam.fy >> p.cam.cx >> p.cam.cy >> p.cam.b >> p.homog_th >> p.max_iters >> p.max_iters_ref >> p.lc_res >> p.lc_unc >>
        p.lc_inl >> p.lc_trs >> p.lc_rot;
    p.has_points = p.has_lines = 1;
    if (!prm) { std::fprintf(stderr, "params.txt\n"); return 2; }
    plslam_ctx* ctx = nullptr;
    if (plslam_ctx_create(0, &ctx) != PLSLAM_OK) { std::fprintf(stderr, "ctx: %s\n", plslam_last_error()); return 3; }
    std::vector<plslam_track_pair> pairs((size_t)B);
    for (int b = 0; b < B; ++b) {
        plslam_track_pair& q = pairs[(size_t)b];
        meta >> q.n_pt_prev >> q.n_pt_curr >> q.n_ls_prev >> q.n_ls_curr;
        const std::string pre = dir + "/p" + std::to_string(b) + "_";
        const size_t np0 = (size_t)q.n_pt_prev, np1 = (size_t)q.n_pt_curr, nl0 = (size_t)q.n_ls_prev, nl1 = (size_t)q.n_ls_curr;
        q.m_pt = upload<int32_t>(pre + "m_pt.bin", np0);
        q.st_pt_prev = upload<int32_t>(pre + "st_pt_prev.bin", np0);
        q.disp_pt_prev = upload<double>(pre + "disp_pt_prev.bin", np0);
        q.kp_prev = upload<float>(pre + "kp_prev.bin", 2 * np0);
        q.st_pt_curr = upload<int32_t>(pre + "st_pt_curr.bin", np1);
        q.kp_curr = upload<float>(pre + "kp_curr.bin", 2 * np1);
        q.m_ls = upload<int32_t>(pre + "m_ls.bin", nl0);
        q.st_ls_prev = upload<int32_t>(pre + "st_ls_prev.bin", nl0);
        q.disp_ls_prev = upload<double>(pre + "disp_ls_prev.bin", 2 * nl0);
        q.seg_prev = upload<float>(pre + "seg_prev.bin", 4 * nl0);
        q.st_ls_curr = upload<int32_t>(pre + "st_ls_curr.bin", nl1);
        q.seg_curr = upload<float>(pre + "seg_curr.bin", 4 * nl1);
    }
    int rc = 0;
    hipStream_t s = nullptr;
    if (hipStreamCreate(&s) != hipSuccess) return 3;
    try {
        PLSLAM::TrackBatch track(ctx, p, pairs);
        track.run(s);
        if (hipStreamSynchronize(s) != hipSuccess) { std::fprintf(stderr, "synchronise failed\n"); return 3; }
        const PLSLAM::TrackBatch::Host h = track.download();
        for (int b = 0; b < B; ++b) {
            const int32_t p0 = h.pt_off[(size_t)b], p1 = h.pt_off[(size_t)b + 1], l0 = h.ls_off[(size_t)b], l1 = h.ls_off[(size_t)b + 1];
            std::printf("pair %d %d %d\n", b, p1 - p0, l1 - l0);
            for (int32_t k = p0; k < p1; ++k) std::printf("%d %d\n", h.pt_rows[2 * (size_t)k], h.pt_rows[2 * (size_t)k + 1]);
            std::printf("P0");
            for (int q = 0; q < 3; ++q) std::printf(" %.17g", p1 > p0 ? h.P[3 * (size_t)p0 + q] : 0.0);
            std::printf("\n");
            for (int32_t k = l0; k < l1; ++k) std::printf("%d %d\n", h.ls_rows[2 * (size_t)k], h.ls_rows[2 * (size_t)k + 1]);
            std::printf("T");
            for (int q = 0; q < 16; ++q) std::printf(" %.17g", h.results[(size_t)b].T_inc[q]);
            std::printf("\n");
        }
    } catch (const std::exception& e) {
        std::fprintf(stderr, "%s\n", e.what());
        rc = 1;
    }
    (void)hipStreamDestroy(s);
    for (void* d : g_blocks) (void)hipFree(d);
    plslam_ctx_destroy(ctx);
    return rc;
}
