// The pure host half of plslam_lc_correct_image (plslam_amd/csrc/lc_image_plan.hpp): the argument checks and the packing of the
// staged block, on heap arrays of exactly the documented sizes.  A stand-alone program: tests/test_lc_correct_image_cpu.py builds it
// with -fsanitize=address,undefined and runs it; it prints "lc_image_plan: ok" and returns 0, or says which check failed.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "lc_image_plan.hpp"

using namespace plslam;

#define CHECK(cond)                                                   \
    do {                                                              \
        if (!(cond)) {                                                \
            printf("%s:%d: check failed: %s\n", __FILE__, __LINE__, #cond); \
            return 1;                                                 \
        }                                                             \
    } while (0)

namespace {

// an image whose pointers are never dereferenced by the host half: distinct non-NULL addresses are all it needs
struct Image {
    std::vector<double> mem;
    plslam_map_index ix;
    Image(int32_t nk, int32_t n_pt, int32_t n_ls, int32_t obs_pt, int32_t obs_ls) : mem(64)
    {
        char* p = (char*)mem.data();
        ix.n_map_kf = nk;
        ix.kf_valid = (const uint8_t*)(p++);
        ix.x_kf_w = (const double*)(p++);
        plslam_map_landmarks* L[2] = {&ix.points, &ix.lines};
        const int32_t n[2] = {n_pt, n_ls}, no[2] = {obs_pt, obs_ls};
        for (int k = 0; k < 2; ++k) {
            L[k]->n = n[k]; L[k]->n_obs = no[k]; L[k]->n_feat = 10;
            L[k]->valid = (uint8_t*)(p++); L[k]->inlier = (const uint8_t*)(p++); L[k]->X = (const double*)(p++);
            L[k]->obs_ptr = (const int32_t*)(p++); L[k]->obs_kf = (const int32_t*)(p++); L[k]->obs_val = (const double*)(p++);
            L[k]->feat_ptr = (const int32_t*)(p++); L[k]->feat_idx = (int32_t*)(p++);
        }
    }
};

}  // namespace

int main()
{
    const int32_t nk = 5;
    Image im(nk, 100, 40, 300, 90);
    std::vector<double> T((size_t)nk * 16), x((size_t)nk * 6), arrays(7 * 4);
    for (size_t i = 0; i < T.size(); ++i) T[i] = 0.25 * i;
    for (size_t i = 0; i < x.size(); ++i) x[i] = -1.5 * i;
    std::vector<uint8_t> co = {1, 0, 7, 0, 255};                  // any non-zero byte is "corrected"
    double* a = arrays.data();
    const plslam_lc_image_dst full{a, a + 4, a + 8, a + 12, a + 16, a + 20, a + 24};
    LcImagePlan P;

    // everything given: every array is carried, the block holds T_corr, the new rows and the flags as 0 / 1
    CHECK(lc_image_plan(&im.ix, T.data(), co.data(), x.data(), &full, &P) == PLSLAM_OK);
    CHECK(P.nk == nk && P.with_x && P.with_dir[0] && P.with_dir[1] && P.with_med[0] && P.with_med[1]);
    CHECK(P.o_T % 256 == 0 && P.o_x % 256 == 0 && P.o_corr % 256 == 0 && P.o_corr + (size_t)nk <= P.stage_bytes);
    {
        std::vector<char> stage(P.stage_bytes, (char)0x5a);
        lc_image_pack(P, T.data(), co.data(), x.data(), stage.data());
        CHECK(!memcmp(stage.data() + P.o_T, T.data(), T.size() * 8) && !memcmp(stage.data() + P.o_x, x.data(), x.size() * 8));
        const char want[5] = {1, 0, 1, 0, 1};
        CHECK(!memcmp(stage.data() + P.o_corr, want, 5) && stage[P.o_corr + 5] == 0 && stage[P.o_T + T.size() * 8] == 0);
    }
    // x_kf_w: both sides or nothing
    {
        plslam_lc_image_dst d = full;
        CHECK(lc_image_plan(&im.ix, T.data(), co.data(), nullptr, &d, &P) == PLSLAM_OK && !P.with_x);
        std::vector<char> stage(P.stage_bytes);
        lc_image_pack(P, T.data(), co.data(), nullptr, stage.data());
        d.x_kf_w = nullptr;
        CHECK(lc_image_plan(&im.ix, T.data(), co.data(), x.data(), &d, &P) == PLSLAM_OK && !P.with_x);
        std::vector<char> stage2(P.stage_bytes);
        lc_image_pack(P, T.data(), co.data(), x.data(), stage2.data());
    }
    // NULL dir / med_dir: not carried
    {
        plslam_lc_image_dst d = full;
        d.pt_dir = d.ls_med_dir = nullptr;
        CHECK(lc_image_plan(&im.ix, T.data(), co.data(), x.data(), &d, &P) == PLSLAM_OK);
        CHECK(!P.with_dir[0] && P.with_dir[1] && P.with_med[0] && !P.with_med[1]);
    }
    // a kind without landmarks needs no X; its dir and med_dir are not carried whatever is given
    {
        Image none(nk, 0, 40, 0, 90);
        plslam_lc_image_dst d = full;
        d.pt_X = nullptr;
        CHECK(lc_image_plan(&none.ix, T.data(), co.data(), x.data(), &d, &P) == PLSLAM_OK && !P.with_dir[0] && !P.with_med[0] && P.with_dir[1]);
    }
    // the refusals
    CHECK(lc_image_plan(nullptr, T.data(), co.data(), x.data(), &full, &P) == PLSLAM_EINVAL);
    CHECK(lc_image_plan(&im.ix, nullptr, co.data(), x.data(), &full, &P) == PLSLAM_EINVAL);
    CHECK(lc_image_plan(&im.ix, T.data(), nullptr, x.data(), &full, &P) == PLSLAM_EINVAL);
    CHECK(lc_image_plan(&im.ix, T.data(), co.data(), x.data(), nullptr, &P) == PLSLAM_EINVAL && P.why[0] != 0);
    for (int bad = 0; bad < 7; ++bad) {
        Image b(nk, 100, 40, 300, 90);
        plslam_lc_image_dst d = full;
        if (bad == 0) b.ix.n_map_kf = 0;
        if (bad == 1) b.ix.points.n = -1;
        if (bad == 2) b.ix.lines.obs_kf = nullptr;               // observations without their array
        if (bad == 3) b.ix.points.obs_ptr = nullptr;
        if (bad == 4) d.pt_X = nullptr;                          // a kind with landmarks and no X
        if (bad == 5) d.ls_X = nullptr;
        if (bad == 6) d.ls_dir = (double*)((char*)d.ls_dir + 4); // misaligned
        CHECK(lc_image_plan(&b.ix, T.data(), co.data(), x.data(), &d, &P) == PLSLAM_EINVAL);
    }
    {
        Image b(nk, 0, 40, 3, 90);                               // observations of a kind without landmarks
        CHECK(lc_image_plan(&b.ix, T.data(), co.data(), x.data(), &full, &P) == PLSLAM_EINVAL);
    }
    printf("lc_image_plan: ok\n");
    return 0;
}
