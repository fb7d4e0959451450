// PLSLAM::LbaPlanSolver::optimizeOnDevice (plslam_lba_plan_optimize_dev: the whole LM loop in one call, one synchronisation)
// against LbaPlanSolver::optimizeResident (two calls and two synchronisations per iteration, the host's LDL^T and SE(3) maps) on
// the same host-built plan.  The problem file is the one tests/test_gpu_lba_lm.py writes from tests/golden/lba_lm_golden.npz.
// usage: test_lm_loop_ondev <problem.bin>
//            control flow (builds, applied pattern, iters, stop) exact; lambda to 1e-12, err to 1e-9 relative, x_kf and the
//            landmarks to 1e-9 of their scale (the solves and the SE(3) maps differ by rounding and libm).  exit 0: agree
//        test_lm_loop_ondev <problem.bin> --bench <calls>
//            times both routes host to host, <calls> calls each in the order parent / new / parent within this process (the
//            landmarks go up again before every call, outside the timed region); one line "BENCH {json}"
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
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
static double max_abs(const std::vector<double>& a)
{
    double m = 0.0;
    for (double v : a) m = std::max(m, std::fabs(v));
    return m;
}
static int close_to(const char* what, const std::vector<double>& a, const std::vector<double>& b, double rel, bool scale)
{
    if (a.size() != b.size()) { std::fprintf(stderr, "%s: %zu against %zu entries\n", what, a.size(), b.size()); return 1; }
    const double s = scale ? std::max(1.0, max_abs(b)) : 0.0;
    for (size_t i = 0; i < a.size(); ++i) {
        if (std::isinf(a[i]) && std::isinf(b[i])) continue;
        const double tol = scale ? rel * s : rel * std::fabs(b[i]);
        if (!(std::fabs(a[i] - b[i]) <= tol)) { std::fprintf(stderr, "%s[%zu]: %.17g against %.17g\n", what, i, a[i], b[i]); return 1; }
    }
    return 0;
}
struct Series { std::vector<double> us; double med() const { return q(0.5); } double q(double f) const { std::vector<double> s = us; std::sort(s.begin(), s.end()); return s[(size_t)(f * (s.size() - 1) + 0.5)]; } };

int main(int argc, char** argv)
{
    const bool bench = argc == 4 && std::string(argv[2]) == "--bench";
    if (argc != 2 && !bench) { std::fprintf(stderr, "usage: %s <problem.bin> [--bench <calls>]\n", argv[0]); return 2; }
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

    // slots [0, n_kf_map): the stored poses; then the estimate slots, which hold the stored poses of the optimised key frames on entry
    PLSLAM::LbaProblem p;
    p.Nkf = nkf;
    p.poses_T_kf_w.assign(T_map.begin(), T_map.end());
    p.poses_T_kf_w.insert(p.poses_T_kf_w.end(), T_map.begin() + 16, T_map.begin() + 16 * (size_t)(1 + nkf));
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
        const std::vector<double> T0 = p.poses_T_kf_w;
        Solver solver(ctx, cam, cfg[0], p);
        Solver::LmTrace ta, tb;
        std::vector<double> xa, xb, Xa, La, Xb, Lb, Ts;
        auto parent = [&]() { xa = x_kf0; Ts = T0; solver.optimizeResident(xa, Ts, n_kf_map, prm, maps, &ta); };
        auto fresh = [&]() { xb = x_kf0; solver.optimizeOnDevice(xb, T0, n_kf_map, prm, &tb); };
        auto reset = [&]() { solver.iterate(p, false); };          // the landmarks (and poses) of the start go up again
        if (!bench) {
            reset(); parent(); solver.landmarks(Xa, La);
            reset(); fresh(); solver.landmarks(Xb, Lb);
            if (ta.applied != tb.applied || ta.iters != tb.iters || ta.stop != tb.stop || ta.n_singular != tb.n_singular) {
                std::fprintf(stderr, "control flow differs: builds %zu / %zu, iters %d / %d, stop %d / %d\n", ta.applied.size(), tb.applied.size(),
                             ta.iters, tb.iters, ta.stop, tb.stop);
                rc = 1;
            }
            rc |= close_to("lambda", tb.lambda, ta.lambda, 1e-12, false) | close_to("err", tb.err, ta.err, 1e-9, false);
            rc |= close_to("x_kf", xb, xa, 1e-9, true) | close_to("Xw", Xb, Xa, 1e-9, true) | close_to("Lw", Lb, La, 1e-9, true);
            if (npt && Xb == Xw) { std::fprintf(stderr, "the loop did not move the points\n"); rc = 1; }
            std::printf("optimizeOnDevice against optimizeResident: %d builds, iters %d, stop %d: %s\n", (int)tb.err.size(), tb.iters, tb.stop,
                        rc ? "DIFFERENT" : "agree");
        } else {
            const int calls = std::atoi(argv[3]);
            Series s[3];
            for (int w = 0; w < 2; ++w) { reset(); parent(); reset(); fresh(); }      // warm: buffers, the pair lists, code objects
            for (int k = 0; k < 3; ++k)
                for (int i = 0; i < calls; ++i) {
                    reset();
                    const auto t0 = std::chrono::steady_clock::now();
                    if (k == 1) fresh(); else parent();
                    const auto t1 = std::chrono::steady_clock::now();
                    s[k].us.push_back(std::chrono::duration<double, std::micro>(t1 - t0).count());
                }
            const plslam_lba_result& r = solver.lastDeviceResult();
            std::printf("BENCH {\"nkf\": %d, \"npt\": %d, \"nls\": %d, \"calls\": %d, \"builds\": %d, \"iters\": %d, \"stop\": %d, "
                        "\"builds_parent\": %d, \"n_enqueued_passes\": %d, ", nkf, npt, nls, calls, r.n_builds, r.iters, r.stop_reason,
                        (int)ta.err.size(), r.n_enqueued_passes);
            const char* names[3] = {"parent_1", "new", "parent_2"};
            for (int k = 0; k < 3; ++k)
                std::printf("\"%s_us\": {\"median\": %.1f, \"p10\": %.1f, \"p90\": %.1f}%s", names[k], s[k].med(), s[k].q(0.1), s[k].q(0.9), k < 2 ? ", " : "}\n");
        }
    } catch (const std::exception& e) {
        std::fprintf(stderr, "%s\n", e.what());
        rc = 4;
    }
    plslam_ctx_destroy(ctx);
    return rc;
}
