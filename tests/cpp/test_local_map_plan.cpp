// The pure host part of the local-map calls (plslam_amd/csrc/local_map_plan.hpp) on the CPU: no device, no HIP header, no library.
// Hand cases whose expectations are worked out in the comments here -- the carving of the handle's buffer at the tile's edges, the
// image check at its bounds, every call against every state it refuses, the table of the buffers: one "PASS <case>" or
// "FAIL <case>: <what>" line each, exit status 1 when any failed.
//   g++ -std=c++17 -I plslam_amd/csrc -I include tests/cpp/test_local_map_plan.cpp
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <functional>
#include <string>
#include <utility>
#include <vector>

#include "local_map_plan.hpp"

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

// A world of fake addresses: the planner never dereferences an image pointer, it tests them against NULL.
alignas(256) unsigned char g_arena[64 * 256];
template <class T> T* slot(int i) { return (T*)(g_arena + 256 * (size_t)i); }

// an image of 30 keyframes, 1000 points with 4000 observations, 200 lines with 700
plslam_map_index image()
{
    plslam_map_index m;
    memset(&m, 0, sizeof m);
    int s = 0;
    m.n_map_kf = 30; m.kf_valid = slot<uint8_t>(s++); m.x_kf_w = slot<double>(s++);
    plslam_map_landmarks* L[2] = {&m.points, &m.lines};
    const int32_t n[2][3] = {{1000, 4000, 5000}, {200, 700, 900}};
    for (int k = 0; k < 2; ++k) {
        L[k]->n = n[k][0]; L[k]->n_obs = n[k][1]; L[k]->n_feat = n[k][2];
        L[k]->valid = slot<uint8_t>(s++); L[k]->inlier = slot<uint8_t>(s++); L[k]->X = slot<double>(s++);
        L[k]->obs_ptr = slot<int32_t>(s++); L[k]->obs_kf = slot<int32_t>(s++); L[k]->obs_val = slot<double>(s++);
        L[k]->feat_ptr = slot<int32_t>(s++); L[k]->feat_idx = slot<int32_t>(s++);
    }
    return m;
}

size_t pad(size_t b) { return (b + 255) & ~(size_t)255; }

// what every layout must satisfy, whatever its sizes
void check_layout(const LocalMapSizes& z, const size_t (&want_tiles)[LM_CHAINS])
{
    const LocalMapLayout Y(z);
    // aligned as the carver aligns: a slice starts where the one before it ended, padded to 256
    size_t end = 0;
    for (int s = 0; s < LM_SLOTS; ++s) {
        CHECK(Y.off[s] % 256 == 0 && Y.off[s] == end);
        end = Y.off[s] + pad(Y.bytes[s]);
    }
    CHECK(Y.total == end && Y.total == Y.off[LM_PART] + pad(Y.bytes[LM_PART]));
    // no two slices overlap: sorted by offset, each ends at or before the next one starts
    std::vector<std::pair<size_t, size_t>> v;
    for (int s = 0; s < LM_SLOTS; ++s) v.emplace_back(Y.off[s], Y.bytes[s]);
    std::sort(v.begin(), v.end());
    for (size_t i = 0; i + 1 < v.size(); ++i) CHECK(v[i].first + v[i].second <= v[i + 1].first);
    CHECK(v.back().first + v.back().second <= Y.total);
    // the cleared front: kf_local ... cnt, one run from 0 that ends exactly where cnt's slice does (64 bytes, padded)
    CHECK(Y.off[LM_KF_LOCAL] == 0 && Y.bytes[LM_CNT] == C_WORDS * 4 && Y.zero_bytes == Y.off[LM_CNT] + 256);
    for (int s = 0; s < LM_SLOTS; ++s) CHECK((s <= LM_CNT) == (Y.off[s] + Y.bytes[s] <= Y.zero_bytes && Y.off[s] < Y.zero_bytes));
    // the five chains
    size_t words = 0;
    for (int c = 0; c < LM_CHAINS; ++c) {
        CHECK(Y.chain_words[c] == want_tiles[c] && Y.chain_off[c] == words);
        words += Y.chain_words[c];
    }
    CHECK(Y.part_words == words && Y.bytes[LM_PART] == 4 * words);
    CHECK(Y.bytes[LM_X_AUX] == 8 * (6 * (size_t)z.n_map_kf + 3 * (size_t)z.npt + 6 * (size_t)z.nls));
    CHECK(Y.pin_bytes == 4 * (C_WORDS + (size_t)z.n_map_kf));
}

// the handle after form (and gather, and apply) on image(), with the gather's counts written by hand
LocalMapState state(bool gathered, bool applied)
{
    LocalMapState st;
    const plslam_map_index m = image();
    st.begin_form(m);
    int32_t pinned[C_WORDS] = {};
    pinned[C_KF_LOCAL] = 9; pinned[C_PT_LOCAL] = 400; pinned[C_LS_LOCAL] = 80;
    plslam_local_map_counts c;
    memset(&c, 0, sizeof c);
    st.end_form(pinned, &c);
    if (gathered) {
        st.begin_gather();
        pinned[C_NKF] = 7; pinned[C_NPT] = 11; pinned[C_NLS] = 5; pinned[C_PT_OBS] = 40; pinned[C_LS_OBS] = 9;
        st.end_gather(pinned, &c);
    }
    if (applied) st.begin_apply_lba(&c);
    return st;
}

}  // namespace

int main()
{
    run("layout_one_keyframe_both_kinds_empty", [] {
        // 1 keyframe, nothing else.  kf_local: 1 byte at 0 -> 256; pt_local, ls_local: empty at 256; cnt: 64 bytes at 256 -> 512 = the
        // cleared front.  The six masks: empty at 512.  kf_list, kf_inv, row: 4 bytes each at 512, 768, 1024 -> 1280.  pt_list,
        // ls_list: empty at 1280; pt_off, ls_off: one word each at 1280, 1536 -> 1792.  Everything per observation: empty at 1792.
        // X_aux: 6 doubles at 1792 -> 2048.  part: five chains of one tile each = 20 bytes at 2048 -> 2304.
        const LocalMapSizes z{1, 0, 0, 0, 0};
        const size_t one[LM_CHAINS] = {1, 1, 1, 1, 1};
        check_layout(z, one);
        const LocalMapLayout Y(z);
        CHECK(Y.off[LM_PT_LOCAL] == 256 && Y.off[LM_LS_LOCAL] == 256 && Y.off[LM_CNT] == 256 && Y.zero_bytes == 512);
        CHECK(Y.off[LM_PT_CANDIDATE] == 512 && Y.off[LM_LS_MOVED] == 512);
        CHECK(Y.off[LM_KF_LIST] == 512 && Y.off[LM_KF_INV] == 768 && Y.off[LM_ROW] == 1024 && Y.off[LM_PT_LIST] == 1280);
        CHECK(Y.off[LM_PT_OFF] == 1280 && Y.bytes[LM_PT_OFF] == 4 && Y.off[LM_LS_OFF] == 1536 && Y.off[LM_PT_OBS] == 1792);
        CHECK(Y.off[LM_X_AUX] == 1792 && Y.bytes[LM_X_AUX] == 48 && Y.off[LM_PART] == 2048 && Y.bytes[LM_PART] == 20);
        CHECK(Y.total == 2304 && Y.pin_bytes == 68);
    });
    run("layout_at_the_tile_edges", [] {
        // each of the five sizes at 0, 1, 255, 256, 257 beside 30 / 1000 / 200 / 4000 / 700.  A chain has one word per tile of 256,
        // at least one: 0, 1, 255, 256 -> 1; 257 -> 2; 30 -> 1, 1000 -> 4, 200 -> 1.  The observation counts size no chain.
        const int32_t edge[] = {0, 1, 255, 256, 257};
        const size_t edge_tiles[] = {1, 1, 1, 1, 2};
        for (int which = 0; which < 5; ++which)
            for (int e = 0; e < 5; ++e) {
                LocalMapSizes z{30, 1000, 200, 4000, 700};
                size_t tiles[LM_CHAINS] = {1, 4, 4, 1, 1};
                int32_t* field[5] = {&z.n_map_kf, &z.npt, &z.nls, &z.n_pt_obs, &z.n_ls_obs};
                *field[which] = edge[e];
                if (which == 0) tiles[LM_CHAIN_KF] = edge_tiles[e];
                if (which == 1) tiles[LM_CHAIN_PT] = tiles[LM_CHAIN_PT_OBS] = edge_tiles[e];
                if (which == 2) tiles[LM_CHAIN_LS] = tiles[LM_CHAIN_LS_OBS] = edge_tiles[e];
                check_layout(z, tiles);
            }
        // and the sizes of the slices of one of them: 257 lines, 700 line observations
        const LocalMapLayout Y(LocalMapSizes{30, 1000, 257, 4000, 700});
        CHECK(Y.bytes[LM_LS_LOCAL] == 257 && Y.bytes[LM_LS_LIST] == 1028 && Y.bytes[LM_LS_OFF] == 1032 && Y.bytes[LM_LS_OBS] == 16800);
        CHECK(Y.bytes[LM_LS_KF_LOC] == 2800 && Y.bytes[LM_LS_L_OBS] == 16800 && Y.bytes[LM_PT_OBS_UV] == 64000 && Y.bytes[LM_KF_INV] == 120);
        CHECK(Y.bytes[LM_X_AUX] == 8 * (180 + 3000 + 1542) && Y.part_words == 1 + 4 + 4 + 2 + 2);
    });
    run("image_ok_bounds", [] {
        plslam_map_index m = image();
        CHECK(local_map_image_ok(&m) && !local_map_image_ok(nullptr));
        // X_aux's doubles: 6 nk + 3 np + 6 nl < 2^31.  With 1 keyframe and no lines: 6 + 3 * 715827880 = 2^31 - 2 is in,
        // 6 + 3 * 715827881 = 2^31 + 1 is out
        m.n_map_kf = 1; m.lines.n = m.lines.n_obs = 0;
        m.points.n = 715827880;
        CHECK(local_map_image_ok(&m));
        m.points.n = 715827881;
        CHECK(!local_map_image_ok(&m));
        // ... through the lines: 6 + 6 * 357913940 = 2^31 - 2 is in, one more line (2^31 + 4) is out
        m.points.n = m.points.n_obs = 0; m.lines.n = 357913940;
        CHECK(local_map_image_ok(&m));
        m.lines.n = 357913941;
        CHECK(!local_map_image_ok(&m));
        m = image();
        m.points.n_obs = (1 << 30) - 1;
        CHECK(local_map_image_ok(&m));
        m.points.n_obs = 1 << 30;
        CHECK(!local_map_image_ok(&m));
        m = image();
        m.lines.n_obs = 1 << 30;
        CHECK(!local_map_image_ok(&m));
        // an array a non-zero count needs
        m = image(); m.points.X = nullptr;
        CHECK(!local_map_image_ok(&m));
        m.points.n = m.points.n_obs = 0;                          // ... no landmark needs it
        CHECK(local_map_image_ok(&m));
        m = image(); m.lines.obs_kf = nullptr;
        CHECK(!local_map_image_ok(&m));
        m = image(); m.lines.feat_idx = nullptr;
        CHECK(!local_map_image_ok(&m));
        m.lines.n_feat = 0;
        CHECK(local_map_image_ok(&m));
        m = image(); m.kf_valid = nullptr;
        CHECK(!local_map_image_ok(&m));
        m = image(); m.x_kf_w = nullptr;
        CHECK(!local_map_image_ok(&m));
        m = image(); m.n_map_kf = 0;
        CHECK(!local_map_image_ok(&m));
        m = image(); m.points.n = -1;
        CHECK(!local_map_image_ok(&m));
    });
    run("form_arguments", [] {
        const plslam_map_index m = image();
        plslam_local_map_counts c;
        int32_t row[30] = {};
        CHECK(LocalMapState::check_form(&m, 29, row, &c) == PLSLAM_OK && LocalMapState::check_form(&m, 0, row, &c) == PLSLAM_OK);
        CHECK(LocalMapState::check_form(&m, 30, row, &c) == PLSLAM_EINVAL && LocalMapState::check_form(&m, -1, row, &c) == PLSLAM_EINVAL);
        CHECK(LocalMapState::check_form(&m, 29, nullptr, &c) == PLSLAM_EINVAL && LocalMapState::check_form(&m, 29, row, nullptr) == PLSLAM_EINVAL);
        CHECK(LocalMapState::check_form(nullptr, 29, row, &c) == PLSLAM_EINVAL);
        CHECK(LocalMapState::check_form_all(&m, &c) == PLSLAM_OK && LocalMapState::check_form_all(&m, nullptr) == PLSLAM_EINVAL);
        CHECK(LocalMapState::check_form_all(nullptr, &c) == PLSLAM_EINVAL);
    });
    run("calls_before_form", [] {
        const plslam_map_index m = image();
        plslam_local_map_counts c;
        plslam_local_map_buffers b;
        memset(&b, 0, sizeof b);
        const LocalMapState fresh;
        CHECK(fresh.check_candidates(&m) == PLSLAM_EINVAL && fresh.check_gather(&m, &c) == PLSLAM_EINVAL && fresh.check_cull(&m, &c) == PLSLAM_EINVAL);
        CHECK(fresh.check_device_buffers(&b) == PLSLAM_EINVAL && fresh.check_download(&b) == PLSLAM_EINVAL);
        LocalMapState begun;                                      // a form that did not finish (its layout or a launch failed)
        begun.begin_form(m);
        CHECK(begun.check_candidates(&m) == PLSLAM_EINVAL && begun.check_gather(&m, &c) == PLSLAM_EINVAL);
        const LocalMapState st = state(false, false);
        CHECK(st.check_candidates(&m) == PLSLAM_OK && st.check_gather(&m, &c) == PLSLAM_OK && st.check_cull(&m, &c) == PLSLAM_OK);
        CHECK(st.check_device_buffers(&b) == PLSLAM_OK && st.check_device_buffers(nullptr) == PLSLAM_EINVAL);
        CHECK(st.check_gather(&m, nullptr) == PLSLAM_EINVAL && st.check_cull(&m, nullptr) == PLSLAM_EINVAL && st.check_candidates(nullptr) == PLSLAM_EINVAL);
    });
    run("calls_on_a_changed_image", [] {
        const LocalMapState st = state(false, false);
        plslam_local_map_counts c;
        for (int which = 0; which < 5; ++which)
            for (int step = -1; step <= 1; step += 2) {
                plslam_map_index m = image();
                int32_t* field[5] = {&m.n_map_kf, &m.points.n, &m.lines.n, &m.points.n_obs, &m.lines.n_obs};
                *field[which] += step;
                CHECK(local_map_image_ok(&m));                    // (a good image, only another one)
                CHECK(st.check_candidates(&m) == PLSLAM_EINVAL && st.check_gather(&m, &c) == PLSLAM_EINVAL && st.check_cull(&m, &c) == PLSLAM_EINVAL);
            }
        plslam_map_index m = image();                             // n_feat is not one of the five
        m.points.n_feat += 1;
        CHECK(st.check_candidates(&m) == PLSLAM_OK);
    });
    run("apply_checks", [] {
        // the gather listed 11 points and 5 lines
        double X[1];
        uint8_t in[1];
        const plslam_local_map_lba_dst dst{X, in, X, in};
        plslam_local_map_counts c;
        const LocalMapState formed = state(false, false), st = state(true, false);
        CHECK(st.check_apply_lba(true, 11, 5, true, &dst, &c) == PLSLAM_OK && st.check_apply_gba(true, 11, 5, true, &dst) == PLSLAM_OK);
        CHECK(formed.check_apply_lba(true, 11, 5, true, &dst, &c) == PLSLAM_EINVAL);           // before gather
        CHECK(formed.check_apply_gba(true, 11, 5, true, &dst) == PLSLAM_EINVAL);
        CHECK(LocalMapState().check_apply_lba(true, 0, 0, true, &dst, &c) == PLSLAM_EINVAL);   // before form
        for (int d = -1; d <= 1; d += 2) {                                                     // the plan's counts off by one
            CHECK(st.check_apply_lba(true, 11 + d, 5, true, &dst, &c) == PLSLAM_EINVAL && st.check_apply_lba(true, 11, 5 + d, true, &dst, &c) == PLSLAM_EINVAL);
            CHECK(st.check_apply_gba(true, 11 + d, 5, true, &dst) == PLSLAM_EINVAL && st.check_apply_gba(true, 11, 5 + d, true, &dst) == PLSLAM_EINVAL);
        }
        CHECK(st.check_apply_lba(true, 11, 5, false, &dst, &c) == PLSLAM_EINVAL);              // state_valid
        CHECK(st.check_apply_gba(true, 11, 5, false, &dst) == PLSLAM_EINVAL);                  // optimized
        CHECK(st.check_apply_lba(false, 11, 5, true, &dst, &c) == PLSLAM_EINVAL);              // another context's plan
        CHECK(st.check_apply_gba(false, 11, 5, true, &dst) == PLSLAM_EINVAL);
        CHECK(st.check_apply_lba(true, 11, 5, true, nullptr, &c) == PLSLAM_EINVAL && st.check_apply_lba(true, 11, 5, true, &dst, nullptr) == PLSLAM_EINVAL);
        CHECK(st.check_apply_gba(true, 11, 5, true, nullptr) == PLSLAM_EINVAL);
        // the destination's arrays: X and inlier for the local BA, X alone for the global one; none for an empty list
        const plslam_local_map_lba_dst no_inl{X, nullptr, X, nullptr}, no_lsX{X, in, nullptr, in}, none{nullptr, nullptr, nullptr, nullptr};
        CHECK(st.check_apply_lba(true, 11, 5, true, &no_inl, &c) == PLSLAM_EINVAL && st.check_apply_gba(true, 11, 5, true, &no_inl) == PLSLAM_OK);
        CHECK(st.check_apply_lba(true, 11, 5, true, &no_lsX, &c) == PLSLAM_EINVAL && st.check_apply_gba(true, 11, 5, true, &no_lsX) == PLSLAM_EINVAL);
        LocalMapState empty = st;
        empty.h_cnt[C_NPT] = empty.h_cnt[C_NLS] = 0;
        CHECK(empty.check_apply_lba(true, 0, 0, true, &none, &c) == PLSLAM_OK && empty.check_apply_gba(true, 0, 0, true, &none) == PLSLAM_OK);
    });
    run("download_preconditions", [] {
        alignas(8) unsigned char host_mem[8];
        const LocalMapState formed = state(false, false), gathered = state(true, false), applied = state(true, true);
        CHECK(formed.check_download(nullptr) == PLSLAM_EINVAL);
        for (const LocalMapBuffer& e : LOCAL_MAP_BUFFERS) {       // one buffer asked for at a time
            plslam_local_map_buffers h;
            memset(&h, 0, sizeof h);
            local_map_buffer_set(h, e, host_mem);
            CHECK(LocalMapState().check_download(&h) == PLSLAM_EINVAL);
            CHECK(formed.check_download(&h) == (e.after == LM_AFTER_FORM ? PLSLAM_OK : PLSLAM_EINVAL));
            CHECK(gathered.check_download(&h) == (e.after == LM_AFTER_APPLY ? PLSLAM_EINVAL : PLSLAM_OK));
            CHECK(applied.check_download(&h) == PLSLAM_OK);
        }
        // by name: a list before the gather, pt_moved before the write-back, a flag array at once
        plslam_local_map_buffers h;
        memset(&h, 0, sizeof h);
        CHECK(formed.check_download(&h) == PLSLAM_OK);            // nothing asked for
        h.kf_local = host_mem; h.pt_candidate = host_mem; h.ls_removed = host_mem;
        CHECK(formed.check_download(&h) == PLSLAM_OK);
        h.pt_list = (int32_t*)host_mem;
        CHECK(formed.check_download(&h) == PLSLAM_EINVAL && gathered.check_download(&h) == PLSLAM_OK);
        h.pt_list = nullptr; h.X_aux = (double*)host_mem;
        CHECK(formed.check_download(&h) == PLSLAM_EINVAL && gathered.check_download(&h) == PLSLAM_OK);
        h.pt_moved = host_mem;
        CHECK(gathered.check_download(&h) == PLSLAM_EINVAL && applied.check_download(&h) == PLSLAM_OK);
        h.pt_moved = nullptr; h.ls_moved = host_mem;
        CHECK(gathered.check_download(&h) == PLSLAM_EINVAL && applied.check_download(&h) == PLSLAM_OK);
        h.stream = host_mem;                                      // ignored
        CHECK(applied.check_download(&h) == PLSLAM_OK);
    });
    run("transitions", [] {
        const plslam_map_index m = image();
        plslam_local_map_counts c;
        memset(&c, 0x55, sizeof c);
        LocalMapState st = state(true, true);
        CHECK(st.formed && st.gathered && st.applied && st.h_cnt[C_NPT] == 11 && st.h_cnt[C_KF_LOCAL] == 9);
        st.begin_gather();                                        // gather clears applied (and gathered, until it is through)
        CHECK(st.formed && !st.gathered && !st.applied);
        int32_t pinned[C_WORDS] = {};
        pinned[C_NKF] = 3; pinned[C_NPT] = 4; pinned[C_NLS] = 0; pinned[C_PT_OBS] = 0; pinned[C_LS_OBS] = 0;
        st.end_gather(pinned, &c);
        CHECK(st.gathered && !st.applied && c.nkf == 3 && c.npt == 4 && c.nls == 0 && c.n_pt_obs == 0 && c.n_ls_obs == 0 && c.empty == 1);
        CHECK(st.h_cnt[C_NKF] == 3 && st.h_cnt[C_NPT] == 4 && st.h_cnt[C_KF_LOCAL] == 9);
        pinned[C_LS_OBS] = 2;
        st.end_gather(pinned, &c);
        CHECK(c.empty == 0 && c.n_ls_obs == 2);
        st.begin_apply_lba(&c);
        CHECK(st.applied && c.n_pt_moved == 0 && c.n_ls_moved == 0);
        pinned[C_PT_MOVED] = 2; pinned[C_LS_MOVED] = 1;
        st.end_apply_lba(pinned, &c);
        CHECK(c.n_pt_moved == 2 && c.n_ls_moved == 1 && st.h_cnt[C_PT_MOVED] == 2 && st.h_cnt[C_LS_MOVED] == 1);
        pinned[C_PT_REM] = 6; pinned[C_LS_REM] = 7;
        st.begin_cull(&c);
        CHECK(c.n_pt_removed == 0 && c.n_ls_removed == 0 && st.gathered && st.applied);
        st.end_cull(pinned, &c);
        CHECK(c.n_pt_removed == 6 && c.n_ls_removed == 7 && st.h_cnt[C_PT_REM] == 6 && st.h_cnt[C_LS_REM] == 7);
        plslam_map_index small = m;                               // form clears gathered and applied, and takes the new sizes
        small.points.n = 10; small.points.n_obs = 20;
        st.begin_form(small);
        CHECK(!st.formed && !st.gathered && !st.applied && st.z.npt == 10 && st.z.n_pt_obs == 20 && st.z.nls == 200);
        pinned[C_KF_LOCAL] = 1; pinned[C_PT_LOCAL] = 2; pinned[C_LS_LOCAL] = 3;
        st.end_form(pinned, &c);
        CHECK(st.formed && !st.gathered && !st.applied && c.n_kf_local == 1 && c.n_pt_local == 2 && c.n_ls_local == 3);
        for (int k = C_NKF; k < C_WORDS; ++k) CHECK(st.h_cnt[k] == 0);   // the counts of the calls before it are gone
        CHECK(st.same_map(&small) && !st.same_map(&m));
    });
    run("buffer_table", [] {
        // plslam_local_map_buffers: 24 pointers, `stream` among them; the table names the other 23, each once, each with a slice of
        // its own that is none of the handle's private ones
        CHECK(LOCAL_MAP_N_BUFFERS == 23 && sizeof(plslam_local_map_buffers) == 24 * sizeof(void*));
        std::vector<int> seen_field(24, 0), seen_slot(LM_SLOTS, 0);
        for (const LocalMapBuffer& e : LOCAL_MAP_BUFFERS) {
            CHECK(e.field % sizeof(void*) == 0 && e.field < sizeof(plslam_local_map_buffers) && e.field != offsetof(plslam_local_map_buffers, stream));
            seen_field[e.field / sizeof(void*)] += 1;
            seen_slot[e.slot] += 1;
        }
        for (size_t i = 0; i < 24; ++i) CHECK(seen_field[i] == (i == offsetof(plslam_local_map_buffers, stream) / sizeof(void*) ? 0 : 1));
        for (int s = 0; s < LM_SLOTS; ++s) {
            const bool priv = s == LM_CNT || s == LM_KF_INV || s == LM_ROW || s == LM_PT_OFF || s == LM_LS_OFF || s == LM_PART;
            CHECK(seen_slot[s] == (priv ? 0 : 1));
        }
        // filled: every member at its slice
        const LocalMapLayout Y(LocalMapSizes{30, 1000, 200, 4000, 700});
        plslam_local_map_buffers b;
        memset(&b, 0, sizeof b);
        char* base = (char*)g_arena;                              // (only offsets are added to it)
        local_map_fill_buffers(b, Y, base, g_arena + 8);
        CHECK((char*)b.kf_local == base && (char*)b.pt_local == base + Y.off[LM_PT_LOCAL] && (char*)b.ls_candidate == base + Y.off[LM_LS_CANDIDATE]);
        CHECK((char*)b.pt_removed == base + Y.off[LM_PT_REMOVED] && (char*)b.kf_list == base + Y.off[LM_KF_LIST] && (char*)b.ls_obs == base + Y.off[LM_LS_OBS]);
        CHECK((char*)b.pt_pose_slot == base + Y.off[LM_PT_POSE_SLOT] && (char*)b.ls_lm_loc == base + Y.off[LM_LS_LM_LOC]);
        CHECK((char*)b.pt_obs_uv == base + Y.off[LM_PT_OBS_UV] && (char*)b.X_aux == base + Y.off[LM_X_AUX] && (char*)b.ls_moved == base + Y.off[LM_LS_MOVED]);
        CHECK(b.stream == g_arena + 8);
    });
    run("download_bytes", [] {
        // formed on 30 keyframes / 1000 points / 200 lines; the gather listed 7 keyframes, 11 points, 5 lines, 40 + 9 observations
        const LocalMapState st = state(true, true);
        struct Want { size_t field, bytes; };
#define W(member, bytes) {offsetof(plslam_local_map_buffers, member), bytes}
        const Want want[] = {W(kf_local, 30), W(pt_local, 1000), W(ls_local, 200), W(pt_candidate, 1000), W(ls_candidate, 200),
                             W(pt_removed, 1000), W(ls_removed, 200), W(kf_list, 7 * 4), W(pt_list, 11 * 4), W(ls_list, 5 * 4),
                             W(pt_obs, 40 * 24), W(ls_obs, 9 * 24), W(pt_lm_loc, 40 * 4), W(pt_kf_loc, 40 * 4), W(pt_pose_slot, 40 * 4),
                             W(ls_lm_loc, 9 * 4), W(ls_kf_loc, 9 * 4), W(ls_pose_slot, 9 * 4), W(pt_obs_uv, 40 * 16), W(ls_l_obs, 9 * 24),
                             W(X_aux, (6 * 7 + 3 * 11 + 6 * 5) * 8), W(pt_moved, 11), W(ls_moved, 5)};
#undef W
        int found = 0;
        for (const Want& w : want)
            for (const LocalMapBuffer& e : LOCAL_MAP_BUFFERS)
                if (e.field == w.field) {
                    CHECK(st.download_bytes(e) == w.bytes);
                    ++found;
                }
        CHECK(found == 23);
        // no download is larger than its slice
        const LocalMapLayout Y(st.z);
        for (const LocalMapBuffer& e : LOCAL_MAP_BUFFERS) CHECK(st.download_bytes(e) <= Y.bytes[e.slot]);
    });
    return n_failed ? 1 : 0;
}
