// A C++ client of plslam_amd/host/loop_closure.hpp's batch form: reads keyframe pairs written by
// tests/test_gpu_lc_batch_shim.py, runs them through LoopClosureBatch::isLoopClosure in ONE call and then one by one through
// LoopClosure::isLoopClosure, and prints what each leaves: the return value, pose_inc and the rows of lc_pt_idx / lc_ls_idx.
//   test_lc_batch_shim <dir>   (dir/meta.txt: B, then per pair n_pt0 n_ls0 n_pt1 n_ls1 and whether kf1 is pair 0's;
//                               dir/p<b>_k{0,1}_{pdesc,P,pl,pt_idx,ldesc,sPeP,le,ls_idx}.bin; dir/params.txt)
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <memory>
#include <string>
#include <vector>

#include "../../plslam_amd/host/loop_closure.hpp"

struct V {                                          // a stand-in for Eigen's small vectors
    double d[6] = {0, 0, 0, 0, 0, 0};
    double& operator()(int i) { return d[i]; }
    double operator()(int i) const { return d[i]; }
};
struct I4 {
    int v[4] = {0, 0, 0, 0};
    int& operator()(int i) { return v[i]; }
};
struct Pt { V P, pl; int idx; };
struct Ls { V sP, eP, le; int idx; };
struct Desc {                                       // cv::Mat-like: ptr<uchar>(row)
    std::vector<uint8_t> b;
    template <class T> const T* ptr(int r) const { return reinterpret_cast<const T*>(b.data() + (size_t)r * 32); }
};
struct Frame {
    std::vector<std::unique_ptr<Pt>> stereo_pt;
    std::vector<std::unique_ptr<Ls>> stereo_ls;
    Desc pdesc_l, ldesc_l;
};

template <class T> static std::vector<T> load(const std::string& path, size_t n)
{
    std::vector<T> v(n);
    std::ifstream f(path, std::ios::binary);
    if (n) f.read(reinterpret_cast<char*>(v.data()), (std::streamsize)(n * sizeof(T)));
    if (!f && n) { std::fprintf(stderr, "cannot read %s\n", path.c_str()); std::exit(2); }
    return v;
}

static void read_frame(const std::string& d, int b, int q, int np, int nl, Frame& f)
{
    const std::string p = d + "/p" + std::to_string(b) + "_k" + std::to_string(q) + "_";
    f.pdesc_l.b = load<uint8_t>(p + "pdesc.bin", (size_t)np * 32);
    f.ldesc_l.b = load<uint8_t>(p + "ldesc.bin", (size_t)nl * 32);
    auto P = load<double>(p + "P.bin", (size_t)np * 3), pl = load<double>(p + "pl.bin", (size_t)np * 2);
    auto S = load<double>(p + "sPeP.bin", (size_t)nl * 6), le = load<double>(p + "le.bin", (size_t)nl * 3);
    auto pi = load<int32_t>(p + "pt_idx.bin", (size_t)np), li = load<int32_t>(p + "ls_idx.bin", (size_t)nl);
    for (int i = 0; i < np; ++i) {
        auto s = std::make_unique<Pt>();
        for (int k = 0; k < 3; ++k) s->P(k) = P[(size_t)i * 3 + k];
        for (int k = 0; k < 2; ++k) s->pl(k) = pl[(size_t)i * 2 + k];
        s->idx = pi[(size_t)i];
        f.stereo_pt.push_back(std::move(s));
    }
    for (int i = 0; i < nl; ++i) {
        auto s = std::make_unique<Ls>();
        for (int k = 0; k < 3; ++k) { s->sP(k) = S[(size_t)i * 6 + k]; s->eP(k) = S[(size_t)i * 6 + 3 + k]; s->le(k) = le[(size_t)i * 3 + k]; }
        s->idx = li[(size_t)i];
        f.stereo_ls.push_back(std::move(s));
    }
}

static void print(const char* tag, size_t b, bool is, const V& pose, std::vector<I4>& pt, std::vector<I4>& ls)
{
    std::printf("%s %zu is_lc %d\npose_inc", tag, b, is ? 1 : 0);
    for (int k = 0; k < 6; ++k) std::printf(" %.17g", pose(k));
    std::printf("\npt %zu\n", pt.size());
    for (auto& r : pt) std::printf("%d %d %d %d\n", r(0), r(1), r(2), r(3));
    std::printf("ls %zu\n", ls.size());
    for (auto& r : ls) std::printf("%d %d %d %d\n", r(0), r(1), r(2), r(3));
}

int main(int argc, char** argv)
{
    if (argc < 2) return 2;
    const std::string d = argv[1];
    std::ifstream m(d + "/meta.txt");
    int B = 0;
    m >> B;
    std::vector<std::unique_ptr<Frame>> own;
    std::vector<const Frame*> kf0, kf1;
    for (int b = 0; b < B; ++b) {
        int n[4], shared = 0;
        m >> n[0] >> n[1] >> n[2] >> n[3] >> shared;
        own.push_back(std::make_unique<Frame>());
        read_frame(d, b, 0, n[0], n[1], *own.back());
        kf0.push_back(own.back().get());
        if (shared) {
            kf1.push_back(kf1[0]);
        } else {
            own.push_back(std::make_unique<Frame>());
            read_frame(d, b, 1, n[2], n[3], *own.back());
            kf1.push_back(own.back().get());
        }
    }
    plslam_ctx* ctx = nullptr;
    if (plslam_ctx_create(0, &ctx) != PLSLAM_OK) return 3;
    plslam_lc_params p = {};
    std::ifstream pm(d + "/params.txt");
    pm >> p.cam.fx >> p.cam.fy >> p.cam.cx >> p.cam.cy >> p.homog_th >> p.min_ratio_12_p >> p.min_ratio_12_l >> p.mutual >>
        p.has_points >> p.has_lines >> p.max_iters >> p.max_iters_ref >> p.lc_inlier_ratio >> p.lc_res >> p.lc_unc >> p.lc_inl >>
        p.lc_trs >> p.lc_rot;
    int rc = 0;
    try {
        {
            plslam::LoopClosureBatch batch(ctx, p, B);
            std::vector<V> pose;
            std::vector<std::vector<I4>> pt, ls;
            std::vector<bool> is;
            batch.isLoopClosure(kf0, kf1, pose, pt, ls, is);
            for (size_t b = 0; b < (size_t)B; ++b) print("batch", b, is[b], pose[b], pt[b], ls[b]);
        }
        plslam::LoopClosure lc(ctx, p);
        for (size_t b = 0; b < (size_t)B; ++b) {
            V pose;
            std::vector<I4> pt, ls;
            const bool is = lc.isLoopClosure(*kf0[b], *kf1[b], pose, pt, ls);
            print("single", b, is, pose, pt, ls);
        }
    } catch (const std::exception& e) {
        std::fprintf(stderr, "%s\n", e.what());
        rc = 1;
    }
    plslam_ctx_destroy(ctx);
    return rc;
}
