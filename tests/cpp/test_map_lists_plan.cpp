// The pure host planner of the map-lists calls (plslam_amd/csrc/map_lists_plan.hpp) on the CPU: no device, no HIP header, no
// library.  Hand cases whose expectations are worked out in the comments here -- every refusal of include/plslam_hip.h that needs
// no device, the launch geometry at the tile's edges, the scratch layout: one "PASS <case>" or "FAIL <case>: <what>" line each,
// exit status 1 when any failed.
//   g++ -std=c++17 -I plslam_amd/csrc -I include tests/cpp/test_map_lists_plan.cpp
#include <cstdio>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include "map_lists_plan.hpp"

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

// A world of fake addresses: the planner never dereferences a list or an image pointer, it compares and checks alignment.
// Every array gets 4 KB of an aligned arena of its own.
alignas(256) unsigned char g_arena[64 * 4096];
void* slot(int i) { return g_arena + 4096 * (size_t)i; }

struct World {
    plslam_map_index src, dst;
    plslam_map_lists sl, dl;
    ListsRecords R;
    ListsRows rows[2];
};

// an insert (kf2kf) that read 10 points / 30 observations and 4 lines / 9 observations and produced 12 / 35 and 5 / 12, with 3
// point events and 2 line events
World world()
{
    World w;
    memset(&w.src, 0, sizeof(w.src));
    memset(&w.dst, 0, sizeof(w.dst));
    memset(&w.sl, 0, sizeof(w.sl));
    memset(&w.dl, 0, sizeof(w.dl));
    int s = 0;
    const int32_t n[2][4] = {{10, 30, 12, 35}, {4, 9, 5, 12}};
    plslam_map_landmarks* SM[2] = {&w.src.points, &w.src.lines};
    plslam_map_landmarks* DM[2] = {&w.dst.points, &w.dst.lines};
    plslam_map_lists_kind* SL[2] = {&w.sl.points, &w.sl.lines};
    plslam_map_lists_kind* DL[2] = {&w.dl.points, &w.dl.lines};
    for (int k = 0; k < 2; ++k) {
        SM[k]->n = n[k][0]; SM[k]->n_obs = n[k][1]; DM[k]->n = n[k][2]; DM[k]->n_obs = n[k][3];
        SM[k]->obs_ptr = (const int32_t*)slot(s++); SM[k]->valid = (uint8_t*)slot(s++);
        DM[k]->obs_ptr = (const int32_t*)slot(s++); DM[k]->valid = (uint8_t*)slot(s++);
        for (plslam_map_lists_kind* L : {SL[k], DL[k]}) {
            L->desc = (uint8_t*)slot(s++); L->dir = (double*)slot(s++); L->pts = k ? (double*)slot(s++) : nullptr;
            L->med_idx = (int32_t*)slot(s++); L->med_desc = (uint8_t*)slot(s++); L->refreshed = (uint8_t*)slot(s++);
        }
        ListsKindRecords& r = w.R.k[k];
        r.src_n = n[k][0]; r.src_obs = n[k][1]; r.dst_n = n[k][2]; r.dst_obs = n[k][3];
        r.n_ev = k ? 2 : 3; r.bound[0] = 20; r.bound[1] = 25; r.ev_stride = 4; r.need_side0 = 1;
        r.ev = (const int32_t*)slot(s++); r.dir = (const double*)slot(s++); r.obs_src = (const int32_t*)slot(s++);
        w.rows[k].desc[0] = (const uint8_t*)slot(s++); w.rows[k].desc[1] = (const uint8_t*)slot(s++);
        if (k) { w.rows[k].pts[0] = (const double*)slot(s++); w.rows[k].pts[1] = (const double*)slot(s++); }
    }
    w.R.valid = true;
    return w;
}

int plan(const World& w, ListsPlan* P = nullptr)
{
    ListsPlan local;
    return lists_carry_plan(w.R, &w.src, &w.sl, &w.dst, &w.dl, w.rows, P ? P : &local);
}

}  // namespace

int main()
{
    run("accepts_the_plain_call", [] {
        World w = world();
        ListsPlan P;
        CHECK(plan(w, &P) == PLSLAM_OK);
        CHECK(P.k[0].dst_n == 12 && P.k[0].dst_obs == 35 && P.k[1].src_n == 4 && P.k[1].src_obs == 9);
        CHECK(!P.k[0].with_pts && P.k[1].with_pts);
    });
    run("null_arguments", [] {
        World w = world();
        ListsPlan P;
        CHECK(lists_carry_plan(w.R, nullptr, &w.sl, &w.dst, &w.dl, w.rows, &P) == PLSLAM_EINVAL);
        CHECK(lists_carry_plan(w.R, &w.src, nullptr, &w.dst, &w.dl, w.rows, &P) == PLSLAM_EINVAL);
        CHECK(lists_carry_plan(w.R, &w.src, &w.sl, nullptr, &w.dl, w.rows, &P) == PLSLAM_EINVAL);
        CHECK(lists_carry_plan(w.R, &w.src, &w.sl, &w.dst, nullptr, w.rows, &P) == PLSLAM_EINVAL);
        CHECK(std::string(P.why) == "a NULL argument");
        w.dl.points.med_desc = nullptr;                           // 12 landmarks need it
        CHECK(plan(w) == PLSLAM_EINVAL);
        w = world();
        w.sl.lines.dir = nullptr;                                 // 9 observations need it
        CHECK(plan(w) == PLSLAM_EINVAL);
        w = world();
        w.dl.points.refreshed = nullptr;                          // optional
        CHECK(plan(w) == PLSLAM_OK);
    });
    run("no_successful_call_on_the_handle", [] {
        World w = world();
        w.R.valid = false;
        ListsPlan P;
        CHECK(plan(w, &P) == PLSLAM_EINVAL && std::string(P.why).find("no successful") == 0);
    });
    run("counts_of_another_image", [] {
        for (int which = 0; which < 8; ++which) {
            World w = world();
            plslam_map_landmarks* M[4] = {&w.src.points, &w.src.lines, &w.dst.points, &w.dst.lines};
            (which & 1 ? M[which >> 1]->n_obs : M[which >> 1]->n) += 1;
            CHECK(plan(w) == PLSLAM_EINVAL);
        }
    });
    run("events_without_rows", [] {
        World w = world();
        w.rows[0].desc[1] = nullptr;
        CHECK(plan(w) == PLSLAM_EINVAL);
        w = world();
        w.rows[0].desc[0] = nullptr;                              // kf2kf reads side 0 ...
        CHECK(plan(w) == PLSLAM_EINVAL);
        w.R.k[0].need_side0 = 0;                                  // ... map2kf does not
        CHECK(plan(w) == PLSLAM_OK);
        w = world();
        w.rows[0] = ListsRows{};
        w.R.k[0].n_ev = 0;                                        // no events: no rows needed
        CHECK(plan(w) == PLSLAM_OK);
    });
    run("pts_by_all_or_by_none", [] {
        World w = world();
        w.rows[1].pts[0] = nullptr;                               // one side of the rows
        CHECK(plan(w) == PLSLAM_EINVAL);
        w = world();
        w.rows[1].pts[1] = nullptr;
        CHECK(plan(w) == PLSLAM_EINVAL);
        w = world();
        w.dl.lines.pts = nullptr;                                 // one of the two lists
        CHECK(plan(w) == PLSLAM_EINVAL);
        w = world();
        w.sl.lines.pts = nullptr;
        CHECK(plan(w) == PLSLAM_EINVAL);
        w = world();
        w.sl.lines.pts = w.dl.lines.pts = nullptr;                // none: pts is not carried
        w.rows[1].pts[0] = w.rows[1].pts[1] = nullptr;
        ListsPlan P;
        CHECK(plan(w, &P) == PLSLAM_OK && !P.k[1].with_pts);
        w.rows[1].pts[1] = (const double*)slot(60);               // ... but then the rows may not bring it either
        CHECK(plan(w) == PLSLAM_EINVAL);
    });
    run("destination_is_a_source", [] {
        World w = world();
        w.dl.points.desc = w.sl.points.desc;
        CHECK(plan(w) == PLSLAM_EINVAL);
        w = world();
        w.dl.lines.med_idx = w.sl.lines.med_idx;
        CHECK(plan(w) == PLSLAM_EINVAL);
        w = world();
        w.dl.lines.med_desc = w.sl.points.med_desc;               // across the kinds too
        ListsPlan P;
        CHECK(plan(w, &P) == PLSLAM_EINVAL && std::string(P.why) == "a destination list is a source list");
    });
    run("alignment", [] {
        World w = world();
        w.dl.points.desc += 8;                                    // 16 bytes wanted
        CHECK(plan(w) == PLSLAM_EINVAL);
        w = world();
        w.sl.lines.pts += 1;                                      // 8 bytes off
        w.dl.lines.pts += 1;
        CHECK(plan(w) == PLSLAM_EINVAL);
        w = world();
        w.dl.points.dir = (double*)((char*)w.dl.points.dir + 4);
        CHECK(plan(w) == PLSLAM_EINVAL);
        w = world();
        w.dl.points.dir += 1;                                     // 8 bytes are enough for dir
        CHECK(plan(w) == PLSLAM_OK);
        w = world();
        w.rows[0].desc[1] += 4;
        CHECK(plan(w) == PLSLAM_EINVAL);
    });
    run("geometry_at_the_tile_edges", [] {
        // K85: 8 lanes per observation, 256 per workgroup: 32 observations per workgroup; K86 / K88: a lane per landmark; K87: a
        // lane per observation
        const int32_t obs[] = {0, 1, 32, 33, 255, 256, 257, 8192}, want_carry[] = {0, 1, 1, 2, 8, 8, 9, 256}, want_rows[] = {0, 1, 1, 1, 1, 1, 2, 32};
        for (int i = 0; i < 8; ++i) {
            World w = world();
            w.dst.points.n_obs = w.R.k[0].dst_obs = obs[i];
            ListsPlan P;
            CHECK(plan(w, &P) == PLSLAM_OK);
            CHECK(P.k[0].g_carry == (unsigned)want_carry[i] && P.k[0].g_rows == (unsigned)want_rows[i] && P.k[0].g_lm == 1);
        }
        const int32_t lm[] = {10, 255, 256, 257, 1000000}, want_lm[] = {1, 1, 1, 2, 3907};
        for (int i = 0; i < 5; ++i) {
            World w = world();
            w.dst.points.n = w.R.k[0].dst_n = lm[i];
            ListsPlan P;
            CHECK(plan(w, &P) == PLSLAM_OK && P.k[0].g_lm == (unsigned)want_lm[i]);
        }
        World w = world();                                        // an empty kind launches nothing
        w.src.lines.n = w.src.lines.n_obs = w.dst.lines.n = w.dst.lines.n_obs = 0;
        w.R.k[1].src_n = w.R.k[1].src_obs = w.R.k[1].dst_n = w.R.k[1].dst_obs = w.R.k[1].n_ev = 0;
        w.sl.lines = plslam_map_lists_kind{};
        w.dl.lines = plslam_map_lists_kind{};
        ListsPlan P;
        CHECK(plan(w, &P) == PLSLAM_OK && P.k[1].g_carry == 0 && P.k[1].g_lm == 0 && P.k[1].g_rows == 0);
    });
    run("scratch_layout", [] {
        // 257 point landmarks: 2 workgroups -> 2 x 2 chain words; 5 line landmarks: 1 -> 2.  Slices are 256-byte aligned, the
        // cleared front holds the chain words and the counters of both kinds, the lists follow and overlap nothing.
        World w = world();
        w.dst.points.n = w.R.k[0].dst_n = 257;
        ListsPlan P;
        CHECK(plan(w, &P) == PLSLAM_OK);
        struct Piece { size_t off, bytes; };
        const Piece pieces[] = {{P.k[0].o_part, 16}, {P.k[0].o_cnt, 8}, {P.k[1].o_part, 8}, {P.k[1].o_cnt, 8},
                                {P.k[0].o_tl, 257 * 4}, {P.k[0].o_toff, 258 * 4}, {P.k[1].o_tl, 5 * 4}, {P.k[1].o_toff, 6 * 4}};
        size_t end = 0;
        for (int i = 0; i < 8; ++i) {
            CHECK(pieces[i].off % 256 == 0 && pieces[i].off >= end);
            end = pieces[i].off + pieces[i].bytes;
            CHECK((i < 4) == (end <= P.zero_bytes));
        }
        CHECK(end <= P.scratch_bytes && P.zero_bytes == 4 * 256);
    });
    run("refresh_check", [] {
        World w = world();
        const char* why;
        CHECK(lists_refresh_check(&w.src, &w.sl, &why) == PLSLAM_OK);
        CHECK(lists_refresh_check(nullptr, &w.sl, &why) == PLSLAM_EINVAL && lists_refresh_check(&w.src, nullptr, &why) == PLSLAM_EINVAL);
        w.sl.points.med_idx = nullptr;
        CHECK(lists_refresh_check(&w.src, &w.sl, &why) == PLSLAM_EINVAL);
        w = world();
        w.src.points.obs_ptr = nullptr;
        CHECK(lists_refresh_check(&w.src, &w.sl, &why) == PLSLAM_EINVAL);
        w = world();
        w.sl.lines.desc += 4;
        CHECK(lists_refresh_check(&w.src, &w.sl, &why) == PLSLAM_EINVAL);
    });
    return n_failed ? 1 : 0;
}
