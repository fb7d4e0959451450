// PLSLAM::LbaPlanSolver::optimizeResident on a plan built from DEVICE copies of the observation columns
// (plslam_lba_plan_create_dev) against LbaPlanSolver::optimize on the host-built plan of the same problem: the trace, x_kf and the
// final landmarks must be equal to the bit.  The problem file is the one tests/test_gpu_lba_lm.py writes for test_lm_loop.cpp
// from tests/golden/lba_lm_golden.npz; the SE(3) maps are the checker's restatements, as there.
// usage: test_lm_loop_dev <problem.bin>      exit 0: equal; 1: a difference (printed)
#include <hip/hip_runtime_api.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../oracle/plslam_oracle.h"
#include "../../plslam_amd/host/lba_rows.hpp"

template <class T>
static void rd(FILE* f, std::vector<T>& v, size_t n)
{
    v.resize(n);
    if (n && fread(v.data(), sizeof(T), n, f) != n) { std::fprintf(stderr, "short problem file\n"); std::exit(2); }
}
static std::vector<void*> g_dev;
template <class T>
static const T* up(const std::vector<T>& v)
{
    void* d = nullptr;
    if (hipMalloc(&d, v.size() * sizeof(T) + 8) != hipSuccess) { std::fprintf(stderr, "hipMalloc failed\n"); std::exit(3); }
    g_dev.push_back(d);
    if (!v.empty() && hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) { std::fprintf(stderr, "hipMemcpy failed\n"); std::exit(3); }
    return static_cast<const T*>(d);
}
template <class T>
static int same(const char* what, const std::vector<T>& a, const std::vector<T>& b)
{
    if (a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0)) return 0;
    std::fprintf(stderr, "%s differs (%zu against %zu entries)\n", what, a.size(), b.size());
    return 1;
}

int main(int argc, char** argv)
{
    if (argc != 2) { std::fprintf(stderr, "usage: %s <problem.bin>\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { std::perror(argv[1]); return 2; }
    std::vector<int32_t> hdr;
    rd(f, hdr, 6);
    const int nkf = hdr[0], n_kf_map = hdr[1], npt = hdr[2], nls = hdr[3], npo = hdr[4], nlo = hdr[5];
    std::vector<double> cfg, cam4, T_map, x_kf0, Xw, Lw, pt_uv, ls_l;
    std::vector<int32_t> pt_lm, pt_kf_map, pt_kf_loc, ls_lm, ls_kf_map, ls_kf_loc;
    rd(f, cfg, 6); rd(f, cam4, 4);
    rd(f, T_map, (size_t)n_kf_map * 16); rd(f, x_kf0, (size_t)nkf * 6); rd(f, Xw, (size_t)npt * 3); rd(f, Lw, (size_t)nls * 6);
    rd(f, pt_lm, npo); rd(f, pt_kf_map, npo); rd(f, pt_kf_loc, npo); rd(f, pt_uv, (size_t)npo * 2);
    rd(f, ls_lm, nlo); rd(f, ls_kf_map, nlo); rd(f, ls_kf_loc, nlo); rd(f, ls_l, (size_t)nlo * 3);
    fclose(f);

    // the host-built plan's problem, as test_lm_loop.cpp lays it out: slots [0, n_kf_map) the stored poses, then the estimates
    PLSLAM::LbaProblem p;
    p.Nkf = nkf;
    p.poses_T_kf_w.assign(T_map.begin(), T_map.end());
    p.poses_T_kf_w.resize((size_t)(n_kf_map + nkf) * 16, 0.0);
    p.points = Xw; p.lines = Lw; p.pt_obs = pt_uv; p.ls_obs = ls_l;
    std::vector<int> seen_p(npt, 0), seen_l(nls, 0);
    for (int o = 0; o < npo; ++o) {
        p.pt_obs_list.push_back({pt_lm[o], pt_lm[o], seen_p[pt_lm[o]]++, pt_kf_map[o], pt_kf_loc[o], 1});
        p.pt_pose_slot.push_back(pt_kf_loc[o] >= 0 ? n_kf_map + pt_kf_loc[o] : pt_kf_map[o]);
    }
    for (int o = 0; o < nlo; ++o) {
        p.ls_obs_list.push_back({ls_lm[o], ls_lm[o], seen_l[ls_lm[o]]++, ls_kf_map[o], ls_kf_loc[o], 1});
        p.ls_pose_slot.push_back(ls_kf_map[o]);
    }
    plslam_ctx* ctx = nullptr;
    if (plslam_ctx_create(0, &ctx) != PLSLAM_OK) { std::fprintf(stderr, "plslam_ctx_create: %s\n", plslam_last_error()); return 3; }
    plslam_cam cam{};
    cam.fx = cam4[0]; cam.fy = cam4[1]; cam.cx = cam4[2]; cam.cy = cam4[3];
    int rc = 0;
    try {
        typedef PLSLAM::LbaPlanSolver Solver;
        Solver::LmParams prm;
        prm.lambda_lba_lm = cfg[1]; prm.lambda_lba_k = cfg[2]; prm.max_iters_lba = (int)cfg[3];
        prm.min_error_change = cfg[4]; prm.min_error = cfg[5];
        const Solver::Se3Maps maps = {plo_expmap_se3, plo_logmap_se3, plo_inverse_se3};
        Solver::LmTrace ta, tb;
        std::vector<double> xa = x_kf0, xb = x_kf0, Xb, Lb;
        {
            Solver host(ctx, cam, cfg[0], p);
            host.optimize(p, xa, n_kf_map, prm, maps, &ta);
        }
        {
            // the device columns as the gather leaves them: the pose slot is the key frame's index; the rewrite is the call's
            Solver::DeviceColumns c;
            c.pt_lm_loc = up(pt_lm); c.pt_pose_slot = up(pt_kf_map); c.pt_kf_loc = up(pt_kf_loc); c.pt_obs_uv = up(pt_uv); c.n_pt_obs = npo;
            c.ls_lm_loc = up(ls_lm); c.ls_pose_slot = up(ls_kf_map); c.ls_kf_loc = up(ls_kf_loc); c.ls_l_obs = up(ls_l); c.n_ls_obs = nlo;
            c.Xw = up(Xw); c.Lw = up(Lw);
            Solver dev(ctx, cam, cfg[0], n_kf_map + nkf, nkf, npt, nls, c, n_kf_map);
            std::vector<double> T_slots(T_map.begin(), T_map.end());
            T_slots.resize((size_t)(n_kf_map + nkf) * 16, 0.0);
            dev.optimizeResident(xb, T_slots, n_kf_map, prm, maps, &tb);
            dev.landmarks(Xb, Lb);
        }
        rc |= same("err", ta.err, tb.err) | same("lambda", ta.lambda, tb.lambda) | same("applied", ta.applied, tb.applied);
        if (ta.iters != tb.iters || ta.stop != tb.stop || ta.n_singular != tb.n_singular) { std::fprintf(stderr, "iters / stop / n_singular differ\n"); rc = 1; }
        rc |= same("x_kf", xa, xb) | same("Xw", p.points, Xb) | same("Lw", p.lines, Lb);
        if (same("Xw moved", Xw, Xb) == 0 && npt) { std::fprintf(stderr, "the loop did not move the points\n"); rc = 1; }
        std::printf("optimizeResident against optimize: %d builds, iters %d, stop %d: %s\n", (int)ta.err.size(), ta.iters, ta.stop,
                    rc ? "DIFFERENT" : "equal to the bit");
    } catch (const std::exception& e) {
        std::fprintf(stderr, "%s\n", e.what());
        rc = 4;
    }
    for (void* d : g_dev) (void)hipFree(d);
    plslam_ctx_destroy(ctx);
    return rc;
}
