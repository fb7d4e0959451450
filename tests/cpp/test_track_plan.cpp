// The pure host planner of the tracker (plslam_amd/csrc/track_plan.hpp) on the CPU: no device, no HIP header, no library.
// Hand cases whose expectations come from include/plslam_track.h and from the comments here, not from the code under test:
// one "PASS <case>" or "FAIL <case>: <what>" line each, exit status 1 when any failed.
//   g++ -std=c++17 -I plslam_amd/csrc -I include tests/cpp/test_track_plan.cpp
#include <cstdio>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include "track_plan.hpp"

using namespace plslam;

namespace {

std::string g_fail;     // first failure of the running case
#define CHECK(cond)                                                                          \
    do {                                                                                     \
        if (!(cond) && g_fail.empty()) g_fail = std::string(#cond) + " (line " + std::to_string(__LINE__) + ")"; \
    } while (0)

int n_failed = 0;
void run(const char* name, const std::function<void()>& body)
{
    g_fail.clear();
    body();
    if (g_fail.empty()) std::printf("PASS %s\n", name);
    else { std::printf("FAIL %s: %s\n", name, g_fail.c_str()); ++n_failed; }
}

// addresses that are never read through
template <class T> const T* fake(uintptr_t a) { return reinterpret_cast<const T*>(a); }

plslam_track_pair full_pair(int32_t np0, int32_t np1, int32_t nl0, int32_t nl1)
{
    plslam_track_pair p;
    memset(&p, 0, sizeof(p));
    p.m_pt = fake<int32_t>(0x1000); p.st_pt_prev = fake<int32_t>(0x2000); p.disp_pt_prev = fake<double>(0x3000);
    p.kp_prev = fake<float>(0x4000); p.st_pt_curr = fake<int32_t>(0x5000); p.kp_curr = fake<float>(0x6000);
    p.m_ls = fake<int32_t>(0x7000); p.st_ls_prev = fake<int32_t>(0x8000); p.disp_ls_prev = fake<double>(0x9000);
    p.seg_prev = fake<float>(0xa000); p.st_ls_curr = fake<int32_t>(0xb000); p.seg_curr = fake<float>(0xc000);
    p.n_pt_prev = np0; p.n_pt_curr = np1; p.n_ls_prev = nl0; p.n_ls_curr = nl1;
    return p;
}

int check(const std::vector<plslam_track_pair>& pairs, TrackCaps* caps = nullptr, int32_t B = -12345)
{
    plslam_lc_params prm;
    memset(&prm, 0, sizeof(prm));
    int ctx = 0;
    void* out = nullptr;
    TrackCaps c;
    const int rc = track_check(&ctx, &prm, pairs.empty() ? nullptr : pairs.data(), B == -12345 ? (int32_t)pairs.size() : B, &out, c);
    if (caps) *caps = c;
    return rc;
}

}  // namespace

int main()
{
    run("capacities_are_the_sums_of_the_prev_counts", [] {
        TrackCaps c;
        CHECK(check({full_pair(5, 9, 2, 1), full_pair(0, 4, 7, 7), full_pair(11, 0, 0, 0)}, &c) == PLSLAM_OK);
        CHECK(c.pt == 16 && c.ls == 9);
    });
    run("b_zero_is_ok_and_plans_nothing", [] {
        TrackCaps c;
        CHECK(check({}, &c) == PLSLAM_OK && c.pt == 0 && c.ls == 0);
        const TrackLayout L = track_layout(0, c);
        CHECK(L.bytes == 0);
        CHECK(track_launches(0).n == 0);
        const plslam_track_buffers o = track_buffers(L, nullptr, 0, c);
        CHECK(o.B == 0 && !o.pt_off && !o.results && o.pt_capacity == 0);
    });
    run("null_arguments_and_negative_sizes_are_einval", [] {
        plslam_lc_params prm;
        memset(&prm, 0, sizeof(prm));
        int ctx = 0;
        void* out = nullptr;
        TrackCaps c;
        plslam_track_pair p = full_pair(1, 1, 1, 1);
        CHECK(track_check(nullptr, &prm, &p, 1, &out, c) == PLSLAM_EINVAL);
        CHECK(track_check(&ctx, nullptr, &p, 1, &out, c) == PLSLAM_EINVAL);
        CHECK(track_check(&ctx, &prm, nullptr, 1, &out, c) == PLSLAM_EINVAL);
        CHECK(track_check(&ctx, &prm, &p, 1, nullptr, c) == PLSLAM_EINVAL);
        CHECK(track_check(&ctx, &prm, &p, -1, &out, c) == PLSLAM_EINVAL);
        CHECK(track_check(&ctx, &prm, nullptr, 0, &out, c) == PLSLAM_OK);
        for (int f = 0; f < 4; ++f) {
            plslam_track_pair q = full_pair(3, 3, 3, 3);
            (f == 0 ? q.n_pt_prev : f == 1 ? q.n_pt_curr : f == 2 ? q.n_ls_prev : q.n_ls_curr) = -1;
            CHECK(check({q}) == PLSLAM_EINVAL);
        }
    });
    run("a_null_array_is_refused_only_where_rows_exist", [] {
        // every one of the twelve arrays: refused with rows on both sides
        for (int f = 0; f < 12; ++f) {
            plslam_track_pair q = full_pair(3, 3, 3, 3);
            const void** slot[12] = {(const void**)&q.m_pt, (const void**)&q.st_pt_prev, (const void**)&q.disp_pt_prev, (const void**)&q.kp_prev,
                                     (const void**)&q.st_pt_curr, (const void**)&q.kp_curr, (const void**)&q.m_ls, (const void**)&q.st_ls_prev,
                                     (const void**)&q.disp_ls_prev, (const void**)&q.seg_prev, (const void**)&q.st_ls_curr, (const void**)&q.seg_curr};
            *slot[f] = nullptr;
            CHECK(check({q}) == PLSLAM_EINVAL);
        }
        // a kind without prev rows needs nothing; with prev rows but an empty curr frame it needs the prev arrays alone
        plslam_track_pair q;
        memset(&q, 0, sizeof(q));
        CHECK(check({q}) == PLSLAM_OK);
        q.n_pt_curr = 50; q.n_ls_curr = 50;
        CHECK(check({q}) == PLSLAM_OK);
        q = full_pair(4, 0, 4, 0);
        q.st_pt_curr = nullptr; q.kp_curr = nullptr; q.st_ls_curr = nullptr; q.seg_curr = nullptr;
        CHECK(check({q}) == PLSLAM_OK);
        q.kp_prev = nullptr;
        CHECK(check({q}) == PLSLAM_EINVAL);
    });
    run("counts_and_batch_over_the_limits_are_erange", [] {
        CHECK(check({full_pair(PLSLAM_LC_MAX_FEATURES, 1, 1, 1)}) == PLSLAM_OK);
        CHECK(check({full_pair(PLSLAM_LC_MAX_FEATURES + 1, 1, 1, 1)}) == PLSLAM_ERANGE);
        CHECK(check({full_pair(1, PLSLAM_LC_MAX_FEATURES + 1, 1, 1)}) == PLSLAM_ERANGE);
        CHECK(check({full_pair(1, 1, PLSLAM_LC_MAX_FEATURES + 1, 1)}) == PLSLAM_ERANGE);
        CHECK(check({full_pair(1, 1, 1, PLSLAM_LC_MAX_FEATURES + 1)}) == PLSLAM_ERANGE);
        std::vector<plslam_track_pair> one(1, full_pair(1, 1, 1, 1));
        CHECK(check(one, nullptr, PLSLAM_LC_MAX_BATCH + 1) == PLSLAM_ERANGE);      // refused before a record is read
    });
    run("the_largest_batch_of_the_largest_pairs_stays_under_2_31_rows", [] {
        // 65536 pairs of 16384 rows are 2^30 rows: the largest batch of the largest pairs fits
        std::vector<plslam_track_pair> v((size_t)PLSLAM_LC_MAX_BATCH, full_pair(PLSLAM_LC_MAX_FEATURES, 1, 0, 0));
        TrackCaps c;
        CHECK(check(v, &c) == PLSLAM_OK && c.pt == (int64_t(1) << 30) && c.ls == 0);
        // (no batch the other two limits admit reaches 2^31 rows: the rule on the sums guards the int32 offsets should a
        // limit ever be raised)
    });
    run("layout_every_array_on_256_bytes_in_order_without_overlap", [] {
        TrackCaps c;
        c.pt = 1000; c.ls = 77;
        const int32_t B = 5;
        const TrackLayout L = track_layout(B, c);
        const size_t want[TB_COUNT] = {5 * sizeof(plslam_track_pair), 40, 24, 24, 8000, 616, 24000, 16000, 3696, 1848, 1000, 77,
                                       5 * sizeof(plslam_lc_result)};
        size_t end = 0;
        for (int i = 0; i < TB_COUNT; ++i) {
            CHECK(L.bytes_of[i] == want[i]);
            CHECK(L.off[i] % 256 == 0 && L.off[i] >= end);
            end = L.off[i] + L.bytes_of[i];
        }
        CHECK(L.bytes >= end && L.bytes % 256 == 0 && L.bytes < end + 256);
        char* base = reinterpret_cast<char*>(uintptr_t(0x10000000));
        const plslam_track_buffers o = track_buffers(L, base, B, c);
        CHECK(reinterpret_cast<const char*>(o.pt_off) == base + L.off[TB_PT_OFF] && reinterpret_cast<const char*>(o.ls_off) == base + L.off[TB_LS_OFF]);
        CHECK(reinterpret_cast<const char*>(o.pt_rows) == base + L.off[TB_PT_ROWS] && reinterpret_cast<const char*>(o.ls_rows) == base + L.off[TB_LS_ROWS]);
        CHECK(reinterpret_cast<const char*>(o.P) == base + L.off[TB_P] && reinterpret_cast<const char*>(o.pl_obs) == base + L.off[TB_PL]);
        CHECK(reinterpret_cast<const char*>(o.sPeP) == base + L.off[TB_SPEP] && reinterpret_cast<const char*>(o.le_obs) == base + L.off[TB_LE]);
        CHECK(reinterpret_cast<const char*>(o.pt_inlier) == base + L.off[TB_PT_INL] && reinterpret_cast<const char*>(o.ls_inlier) == base + L.off[TB_LS_INL]);
        CHECK(reinterpret_cast<const char*>(o.results) == base + L.off[TB_RESULTS]);
        CHECK(o.B == 5 && o.pt_capacity == 1000 && o.ls_capacity == 77 && o.reserved == 0);
    });
    run("layout_a_kind_without_rows_keeps_distinct_addresses", [] {
        TrackCaps c;
        c.pt = 0; c.ls = 3;
        const TrackLayout L = track_layout(2, c);
        CHECK(L.bytes_of[TB_P] == 0 && L.bytes_of[TB_PT_ROWS] == 0 && L.bytes_of[TB_PT_INL] == 0);
        for (int i = 1; i < TB_COUNT; ++i) CHECK(L.off[i] >= L.off[i - 1] + 256);       // one row's room each: no two arrays share an address
    });
    run("launches_one_workgroup_per_pair_and_kind_one_for_the_scan", [] {
        const TrackLaunches t = track_launches(600);
        CHECK(t.n == 3);
        CHECK(t.count.gx == 600 && t.count.gy == 2 && t.count.threads == 256);
        CHECK(t.write.gx == 600 && t.write.gy == 2 && t.write.threads == 256);
        CHECK(t.scan.gx == 1 && t.scan.gy == 1 && t.scan.threads == 256);
    });
    run("scan_chunks_cover_every_pair_once", [] {
        // lane t of 256 takes pairs [t chunk, min((t + 1) chunk, B)): together exactly [0, B)
        for (int32_t B : {1, 2, 255, 256, 257, 600, 65535, 65536}) {
            const int32_t ch = track_scan_chunk(B);
            CHECK(ch >= 1 && (int64_t)ch * 256 >= B && (int64_t)(ch - 1) * 256 < B);
        }
        CHECK(track_scan_chunk(256) == 1 && track_scan_chunk(257) == 2 && track_scan_chunk(65536) == 256);
    });
    return n_failed ? 1 : 0;
}
