// The pure host half of plslam_map_insert_kf2kf / _map2kf (plslam_amd/csrc/map_insert_plan.hpp) on the CPU: no device, no HIP
// header, no library.  Hand cases whose expectations are worked out in the comments here -- every refusal one rule away from an
// accepted call, their precedence, the bounds the tables give, the device layout at the tile's edges, the packing of the staged
// block into a buffer of exactly its size: one "PASS <case>" or "FAIL <case>: <what>" line each, exit status 1 when any failed.
//   g++ -std=c++17 -I plslam_amd/csrc -I include tests/cpp/test_map_insert_plan.cpp
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include "map_insert_plan.hpp"

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

// A world of fake addresses for the two images: the planner never dereferences an image pointer, it compares them.  The tables
// and the feature arrays ARE read (the count of entries >= 0, the packing): those are heap arrays of exactly their documented sizes.
alignas(256) unsigned char g_arena[64 * 256];
template <class T> T* slot(int i) { return (T*)(g_arena + 256 * (size_t)i); }

void fake_image(plslam_map_index& m, int& s, int32_t nk, const int32_t (&n)[2][3])
{
    memset(&m, 0, sizeof m);
    m.n_map_kf = nk; m.kf_valid = slot<uint8_t>(s++); m.x_kf_w = slot<double>(s++);
    plslam_map_landmarks* L[2] = {&m.points, &m.lines};
    for (int k = 0; k < 2; ++k) {
        L[k]->n = n[k][0]; L[k]->n_obs = n[k][1]; L[k]->n_feat = n[k][2];
        L[k]->valid = slot<uint8_t>(s++); L[k]->inlier = slot<uint8_t>(s++); L[k]->X = slot<double>(s++);
        L[k]->obs_ptr = slot<int32_t>(s++); L[k]->obs_kf = slot<int32_t>(s++); L[k]->obs_val = slot<double>(s++);
        L[k]->feat_ptr = slot<int32_t>(s++); L[k]->feat_idx = slot<int32_t>(s++);
    }
}

struct Kind {                            // a table of n_tab entries, n_prev / n_curr feature rows
    std::vector<int32_t> tab;
    std::vector<double> P1, o1, P2, o2;
    plslam_map_insert_kind k;
    Kind(const std::vector<int32_t>& table, int32_t n_prev, int32_t n_curr, int dl, int dv, double seed) : tab(table)
    {
        for (int i = 0; i < n_prev * dl; ++i) P1.push_back(seed + i);
        for (int i = 0; i < n_prev * dv; ++i) o1.push_back(seed + 0.25 + i);
        for (int i = 0; i < n_curr * dl; ++i) P2.push_back(-seed - i);
        for (int i = 0; i < n_curr * dv; ++i) o2.push_back(-seed - 0.5 - i);
        bind(n_prev, n_curr);
    }
    Kind(const Kind& o) : tab(o.tab), P1(o.P1), o1(o.o1), P2(o.P2), o2(o.o2) { bind(o.k.n_prev, o.k.n_curr); }
    void bind(int32_t n_prev, int32_t n_curr)
    {
        k = plslam_map_insert_kind{tab.data(), (int32_t)tab.size(), n_prev, n_curr, P1.data(), o1.data(), P2.data(), o2.data()};
    }
};

std::vector<int32_t> table(int32_t n_tab, int32_t m)         // the first m entries name a feature, the rest none
{
    std::vector<int32_t> t((size_t)n_tab, -1);
    for (int32_t i = 0; i < m; ++i) t[(size_t)i] = i % 7;
    return t;
}

// 5 keyframes; 100 points with 300 observations, 40 lines with 90.  Point table: 12 entries, 5 of them >= 0; line table: 6, 2.
struct World {
    plslam_map_index src;
    plslam_map_insert_dst dst;
    Kind pts, lns;
    std::vector<double> T1, T2;
    World() : pts(table(12, 5), 12, 9, 3, 2, 1.0), lns(table(6, 2), 6, 8, 6, 3, 100.0), T1(16), T2(16)
    {
        int s = 0;
        const int32_t n[2][3] = {{100, 300, 50}, {40, 90, 20}}, none[2][3] = {{0, 0, 0}, {0, 0, 0}};
        fake_image(src, s, 5, n);
        fake_image(dst.map, s, 0, none);
        dst.pt_cap = 105; dst.pt_obs_cap = 310; dst.ls_cap = 42; dst.ls_obs_cap = 94;      // exactly what kf2kf can need
        for (int i = 0; i < 16; ++i) { T1[(size_t)i] = 0.5 + i; T2[(size_t)i] = -0.5 - i; }
    }
    int kf2kf(MapInsertPlan* P = nullptr, int32_t kf1 = 3, int32_t kf2 = 4)
    {
        MapInsertPlan local;
        return map_insert_plan(MAP_INSERT_KF2KF, &src, &dst, kf1, kf2, T1.data(), T2.data(), &pts.k, &lns.k, P ? P : &local);
    }
    int map2kf(MapInsertPlan* P = nullptr, int32_t kf2 = 4)
    {
        MapInsertPlan local;
        return map_insert_plan(MAP_INSERT_MAP2KF, &src, &dst, -1, kf2, nullptr, T2.data(), &pts.k, &lns.k, P ? P : &local);
    }
};

size_t pad(size_t b) { return (b + 255) & ~(size_t)255; }

// what every layout must satisfy.  The pieces in the order they are carved, with the bytes each holds.
void check_layout(const MapInsertPlan& P, const plslam_map_index& src)
{
    const plslam_map_landmarks* S[2] = {&src.points, &src.lines};
    struct Piece { size_t off, bytes; int region; };         // region: 0 zeroed, 1 0x7f, 2 staged, 3 scratch, 4 obs_src
    std::vector<Piece> v = {{P.o_cnt, 32, 0}, {P.o_row, (size_t)P.nk * 4, 0}};
    for (int k = 0; k < 2; ++k) {
        const MapInsertKindPlan& K = P.k[k];
        v.push_back({K.o_app, (size_t)S[k]->n * 4 + 4, 0});
        v.push_back({K.o_win, (size_t)K.n_curr * 4 + 4, 0});
        v.push_back({K.o_part, (3 * (size_t)K.w_tab + K.w_lm) * 4, 0});
    }
    for (int k = 0; k < 2; ++k) v.push_back({P.k[k].o_head, (size_t)S[k]->n * 4 + 4, 1});
    v.push_back({P.o_T, 256, 2});
    for (int k = 0; k < 2; ++k) {
        const MapInsertKindPlan& K = P.k[k];
        v.push_back({K.o_tab, (size_t)K.n_tab * 4 + 4, 2});
        v.push_back({K.o_P1, (size_t)K.n_prev * K.dl * 8 + 8, 2});
        v.push_back({K.o_o1, (size_t)K.n_prev * K.dv * 8 + 8, 2});
        v.push_back({K.o_P2, (size_t)K.n_curr * K.dl * 8 + 8, 2});
        v.push_back({K.o_o2, (size_t)K.n_curr * K.dv * 8 + 8, 2});
    }
    for (int k = 0; k < 2; ++k) {
        const MapInsertKindPlan& K = P.k[k];
        v.push_back({K.o_i1lm, (size_t)K.n_tab * 4 + 4, 3});
        v.push_back({K.o_ev, (size_t)K.m * 16 + 16, 3});
        v.push_back({K.o_dir, (size_t)K.m * 48 + 48, 3});
        v.push_back({K.o_pair, (size_t)K.m * 4 + 4, 3});
        v.push_back({K.o_new, (size_t)K.m * 4 + 4, 3});
    }
    for (int k = 0; k < 2; ++k) v.push_back({P.k[k].o_osrc, (size_t)P.k[k].need_obs * 4 + 4, 4});
    // carved in this order, aligned as the carver aligns: each starts where the one before it ended, padded to 256
    size_t end = 0;
    for (const Piece& p : v) {
        CHECK(p.off % 256 == 0 && p.off == end);
        end = p.off + pad(p.bytes);
    }
    CHECK(P.total == end);                                    // obs_src is last
    // no two overlap: sorted by offset, each ends at or before the next one starts
    std::vector<Piece> w = v;
    std::sort(w.begin(), w.end(), [](const Piece& a, const Piece& b) { return a.off < b.off; });
    for (size_t i = 0; i + 1 < w.size(); ++i) CHECK(w[i].off + w[i].bytes <= w[i + 1].off);
    // the zeroed, the 0x7f and the staged regions: contiguous, in that order, and each holds exactly its pieces
    CHECK(P.fill[0].off == 0 && P.fill[0].byte == 0 && P.fill[1].off == P.fill[0].bytes && P.fill[1].byte == 0x7f);
    CHECK(P.stage_off == P.fill[1].off + P.fill[1].bytes && P.stage_off == P.o_T);
    const size_t lo[3] = {0, P.fill[1].off, P.stage_off}, hi[3] = {P.fill[0].bytes, P.stage_off, P.stage_off + P.stage_bytes};
    for (const Piece& p : v)
        for (int r = 0; r < 3; ++r) CHECK((p.region == r) == (p.off >= lo[r] && p.off + p.bytes <= hi[r] && p.off < hi[r]));
    CHECK(P.k[0].o_i1lm == P.stage_off + P.stage_bytes);
    CHECK(P.res_bytes == pad((8 + (size_t)P.nk) * 4));
}

}  // namespace

int main()
{
    run("accepts_both_modes", [] {
        World w;
        MapInsertPlan P;
        CHECK(w.kf2kf(&P) == PLSLAM_OK && P.mode == MAP_INSERT_KF2KF && P.nk == 5 && P.kf1 == 3 && P.kf2 == 4);
        CHECK(P.k[0].in == &w.pts.k && P.k[0].n_tab == 12 && P.k[0].n_prev == 12 && P.k[0].n_curr == 9 && P.k[1].n_tab == 6);
        CHECK(w.map2kf(&P) == PLSLAM_OK && P.mode == MAP_INSERT_MAP2KF && P.kf1 == -1 && P.k[0].n_prev == 0 && P.k[1].n_prev == 0);
    });
    run("null_arguments", [] {
        World w;
        MapInsertPlan P;
        const double *T1 = w.T1.data(), *T2 = w.T2.data();
        CHECK(map_insert_plan(MAP_INSERT_KF2KF, nullptr, &w.dst, 3, 4, T1, T2, &w.pts.k, &w.lns.k, &P) == PLSLAM_EINVAL);
        CHECK(map_insert_plan(MAP_INSERT_KF2KF, &w.src, nullptr, 3, 4, T1, T2, &w.pts.k, &w.lns.k, &P) == PLSLAM_EINVAL);
        CHECK(map_insert_plan(MAP_INSERT_KF2KF, &w.src, &w.dst, 3, 4, T1, nullptr, &w.pts.k, &w.lns.k, &P) == PLSLAM_EINVAL);
        CHECK(map_insert_plan(MAP_INSERT_KF2KF, &w.src, &w.dst, 3, 4, nullptr, T2, &w.pts.k, &w.lns.k, &P) == PLSLAM_EINVAL);
        CHECK(std::string(P.why) == "a NULL argument");
        CHECK(map_insert_plan(MAP_INSERT_MAP2KF, nullptr, &w.dst, -1, 4, nullptr, T2, &w.pts.k, &w.lns.k, &P) == PLSLAM_EINVAL);
        CHECK(map_insert_plan(MAP_INSERT_MAP2KF, &w.src, nullptr, -1, 4, nullptr, T2, &w.pts.k, &w.lns.k, &P) == PLSLAM_EINVAL);
        CHECK(map_insert_plan(MAP_INSERT_MAP2KF, &w.src, &w.dst, -1, 4, nullptr, nullptr, &w.pts.k, &w.lns.k, &P) == PLSLAM_EINVAL);
        CHECK(map_insert_plan(MAP_INSERT_MAP2KF, &w.src, &w.dst, -1, 4, nullptr, T2, &w.pts.k, &w.lns.k, &P) == PLSLAM_OK);   // no T1 there
        CHECK(map_insert_plan(MAP_INSERT_KF2KF, &w.src, &w.dst, 3, 4, T1, T2, nullptr, nullptr, &P) == PLSLAM_OK);          // no kind at all
        w.src.kf_valid = nullptr;                                 // an incomplete source image
        CHECK(w.kf2kf() == PLSLAM_EINVAL && w.map2kf() == PLSLAM_EINVAL);
        World v;
        v.src.lines.obs_val = nullptr;
        CHECK(v.kf2kf(&P) == PLSLAM_EINVAL && std::string(P.why) == "the source image is incomplete" && v.map2kf() == PLSLAM_EINVAL);
    });
    run("slots_out_of_range", [] {
        World w;                                                  // 5 keyframes: slots 0 .. 4
        CHECK(w.kf2kf(nullptr, 0, 4) == PLSLAM_OK && w.kf2kf(nullptr, 4, 0) == PLSLAM_OK);
        CHECK(w.kf2kf(nullptr, 3, 5) == PLSLAM_EINVAL && w.kf2kf(nullptr, 3, -1) == PLSLAM_EINVAL);
        CHECK(w.kf2kf(nullptr, 5, 4) == PLSLAM_EINVAL && w.kf2kf(nullptr, -1, 4) == PLSLAM_EINVAL);
        CHECK(w.kf2kf(nullptr, 4, 4) == PLSLAM_EINVAL);           // kf1 == kf2
        CHECK(w.map2kf(nullptr, 0) == PLSLAM_OK && w.map2kf(nullptr, 4) == PLSLAM_OK);
        CHECK(w.map2kf(nullptr, 5) == PLSLAM_EINVAL && w.map2kf(nullptr, -1) == PLSLAM_EINVAL);
        MapInsertPlan P;                                          // map <-> KF has no keyframe 1: whatever is passed is not looked at
        CHECK(map_insert_plan(MAP_INSERT_MAP2KF, &w.src, &w.dst, 99, 4, nullptr, w.T2.data(), &w.pts.k, &w.lns.k, &P) == PLSLAM_OK && P.kf1 == -1);
    });
    run("destination_is_a_source", [] {
        for (int mode = 0; mode < 2; ++mode) {
            auto call = [mode](World& w) { return mode ? w.map2kf() : w.kf2kf(); };
            World w;
            w.dst.map.points.obs_kf = w.src.points.obs_kf;
            CHECK(call(w) == PLSLAM_EINVAL);
            World x;
            x.dst.map.lines.feat_idx = x.src.lines.feat_idx;
            CHECK(call(x) == PLSLAM_EINVAL);
            World y;
            y.dst.map.lines.X = nullptr;                          // a destination array that is not there
            CHECK(call(y) == PLSLAM_EINVAL);
            World z;
            z.dst.map.x_kf_w = nullptr;
            CHECK(call(z) == PLSLAM_EINVAL);
            World a;                                              // these three may be the source's
            a.dst.map.kf_valid = a.src.kf_valid; a.dst.map.x_kf_w = a.src.x_kf_w; a.dst.map.points.feat_ptr = a.src.points.feat_ptr;
            CHECK(call(a) == PLSLAM_OK);
        }
    });
    run("kind_arguments", [] {
        World w;
        w.pts.k.n_table = -1;
        CHECK(w.kf2kf() == PLSLAM_EINVAL && w.map2kf() == PLSLAM_EINVAL);
        World a;
        a.lns.k.n_curr = -1;
        CHECK(a.kf2kf() == PLSLAM_EINVAL && a.map2kf() == PLSLAM_EINVAL);
        World b;
        b.lns.k.obs2 = nullptr;                                   // 8 current features need it
        CHECK(b.kf2kf() == PLSLAM_EINVAL && b.map2kf() == PLSLAM_EINVAL);
        b.lns.k.n_curr = 0;                                       // ... none does
        CHECK(b.kf2kf() == PLSLAM_OK && b.map2kf() == PLSLAM_OK);
        World c;
        c.pts.k.P1 = nullptr;                                     // keyframe 1's rows: KF <-> KF only
        CHECK(c.kf2kf() == PLSLAM_EINVAL && c.map2kf() == PLSLAM_OK);
        World d;
        d.pts.k.n_prev = -1;
        CHECK(d.kf2kf() == PLSLAM_EINVAL && d.map2kf() == PLSLAM_OK);
        World e;                                                  // a kind without a table is not looked at any further
        e.pts.k.table = nullptr; e.pts.k.n_curr = -5; e.pts.k.P2 = nullptr;
        CHECK(e.kf2kf() == PLSLAM_OK && e.map2kf() == PLSLAM_OK);
    });
    run("table_length", [] {
        // map <-> KF: the table is indexed by the landmark: at most S.n entries (EINVAL).  KF <-> KF: at most
        // PLSLAM_MAP_INSERT_MAX_TABLE (ERANGE), and it may be longer than the map.
        World w;
        w.pts.tab = table(100, 0); w.pts.bind(12, 9);
        CHECK(w.map2kf() == PLSLAM_OK);
        w.pts.tab = table(101, 0); w.pts.bind(12, 9);
        MapInsertPlan P;
        CHECK(w.map2kf(&P) == PLSLAM_EINVAL && std::string(P.why) == "a map_to_kf table longer than the map");
        CHECK(w.kf2kf() == PLSLAM_OK);
        World x;
        x.lns.tab = table(PLSLAM_MAP_INSERT_MAX_TABLE, 0); x.lns.bind(6, 8);
        CHECK(x.kf2kf() == PLSLAM_OK);
        x.lns.tab = table(PLSLAM_MAP_INSERT_MAX_TABLE + 1, 0); x.lns.bind(6, 8);
        CHECK(x.kf2kf(&P) == PLSLAM_ERANGE && std::string(P.why) == "a table beyond PLSLAM_MAP_INSERT_MAX_TABLE");
    });
    run("capacities", [] {
        // KF <-> KF needs n + m landmarks and n_obs + 2 m observations: 105 / 310 and 42 / 94; map <-> KF n and n_obs + m:
        // 100 / 305 and 40 / 92
        World w;
        int32_t* caps[4] = {&w.dst.pt_cap, &w.dst.pt_obs_cap, &w.dst.ls_cap, &w.dst.ls_obs_cap};
        const int32_t need_b[4] = {100, 305, 40, 92};
        for (int i = 0; i < 4; ++i) {
            --*caps[i];
            CHECK(w.kf2kf() == PLSLAM_ERANGE);
            ++*caps[i];
        }
        CHECK(w.kf2kf() == PLSLAM_OK);
        for (int i = 0; i < 4; ++i) *caps[i] = need_b[i];
        CHECK(w.map2kf() == PLSLAM_OK && w.kf2kf() == PLSLAM_ERANGE);
        for (int i = 0; i < 4; ++i) {
            --*caps[i];
            CHECK(w.map2kf() == PLSLAM_ERANGE);
            ++*caps[i];
        }
        // need_obs < 2^30 whatever the capacity: the source holds 2^30 - 11 point observations, the 5 events of a KF <-> KF
        // insert bring 10 (2^30 - 1: in); one observation more in the source (2^30: out).  map <-> KF brings 5.
        World x;
        x.dst.pt_obs_cap = INT32_MAX;
        x.src.points.n_obs = (1 << 30) - 11;
        MapInsertPlan P;
        CHECK(x.kf2kf(&P) == PLSLAM_OK && P.k[0].need_obs == (1 << 30) - 1);
        x.src.points.n_obs = (1 << 30) - 10;
        CHECK(x.kf2kf(&P) == PLSLAM_ERANGE && std::string(P.why) == "n_obs beyond 2^30");
        CHECK(x.map2kf() == PLSLAM_OK);
        x.src.points.n_obs = (1 << 30) - 5;
        CHECK(x.map2kf() == PLSLAM_ERANGE);
    });
    run("precedence", [] {
        // every EINVAL rule on the whole call is tested before any ERANGE rule; inside the kinds the rules run kind by kind
        World w;
        w.dst.pt_cap -= 1;                                        // ERANGE on its own ...
        CHECK(w.kf2kf() == PLSLAM_ERANGE);
        CHECK(w.kf2kf(nullptr, 4, 4) == PLSLAM_EINVAL);           // ... with kf1 == kf2
        w.dst.map.lines.valid = w.src.lines.valid;                // ... with a destination array that is a source array
        CHECK(w.kf2kf() == PLSLAM_EINVAL && w.map2kf() == PLSLAM_EINVAL);
        World x;                                                  // ... with a bad kind argument of the OTHER kind
        x.dst.pt_cap -= 1;
        x.lns.k.n_curr = -1;
        CHECK(x.kf2kf() == PLSLAM_EINVAL);
        World y;                                                  // a table beyond the limit (ERANGE) of a call with a bad slot
        y.pts.tab = table(PLSLAM_MAP_INSERT_MAX_TABLE + 1, 0); y.pts.bind(12, 9);
        CHECK(y.kf2kf() == PLSLAM_ERANGE && y.kf2kf(nullptr, 3, 7) == PLSLAM_EINVAL);
        World z;                                                  // map <-> KF, one kind: the table's length (EINVAL) before its capacity
        z.pts.tab = table(101, 3); z.pts.bind(12, 9);
        z.dst.pt_obs_cap = 0;
        CHECK(z.map2kf() == PLSLAM_EINVAL);
        World u;                                                  // kind by kind: the points' capacity (ERANGE) is met before the
        u.dst.pt_obs_cap = 0;                                     // lines' table length (EINVAL)
        u.lns.tab = table(41, 0); u.lns.bind(6, 8);
        CHECK(u.map2kf() == PLSLAM_ERANGE);
        u.dst.pt_obs_cap = 310;
        CHECK(u.map2kf() == PLSLAM_EINVAL);
    });
    run("events_and_bounds", [] {
        // m = the entries >= 0.  n = 100 / 40, n_obs = 300 / 90.
        struct Case { int32_t n_tab, m; } cases[] = {{12, 0}, {12, 1}, {12, 12}};
        for (const Case& c : cases) {
            World w;
            w.dst.pt_cap = 200; w.dst.pt_obs_cap = 400;
            w.pts.tab = table(c.n_tab, c.m); w.pts.bind(12, 9);
            MapInsertPlan P;
            CHECK(w.kf2kf(&P) == PLSLAM_OK && P.k[0].m == c.m && P.k[0].need_lm == 100 + c.m && P.k[0].need_obs == 300 + 2 * c.m);
            CHECK(w.map2kf(&P) == PLSLAM_OK && P.k[0].m == c.m && P.k[0].need_lm == 100 && P.k[0].need_obs == 300 + c.m);
            CHECK(P.k[1].m == 2 && P.k[1].need_lm == 40 && P.k[1].need_obs == 92);
        }
        World w;                                                  // an entry that is not first: {-1, 3, -1, -1, 0}: 2
        w.pts.tab = {-1, 3, -1, -1, 0}; w.pts.bind(12, 9);
        MapInsertPlan P;
        CHECK(w.kf2kf(&P) == PLSLAM_OK && P.k[0].m == 2 && P.k[0].n_tab == 5);
        // a kind with no table: a NULL struct, a NULL table, an empty table -- nothing to add, nothing staged
        for (int how = 0; how < 3; ++how) {
            World v;
            if (how == 1) v.lns.k.table = nullptr;
            if (how == 2) v.lns.k.n_table = 0;
            const int rc = map_insert_plan(MAP_INSERT_KF2KF, &v.src, &v.dst, 3, 4, v.T1.data(), v.T2.data(), &v.pts.k, how ? &v.lns.k : nullptr, &P);
            CHECK(rc == PLSLAM_OK && !P.k[1].in && P.k[1].m == 0 && P.k[1].n_tab == 0 && P.k[1].n_curr == 0 && P.k[1].need_lm == 40 && P.k[1].need_obs == 90);
            CHECK(P.k[0].in == &v.pts.k && P.k[0].m == 5);
        }
    });
    run("layout_at_the_tile_edges", [] {
        // tiles of 256: w_tab = the table's, w_lm = those of S.n + m landmarks, at least one each: 0, 255, 256 -> 1; 257 -> 2.
        // The table's length, S.n + m and n_obs + 2 m each at 0, 255, 256, 257 (m = 3 wherever there is a table).
        const int32_t edge[] = {0, 255, 256, 257};
        const unsigned tiles[] = {1, 1, 1, 2};
        for (int e = 0; e < 4; ++e) {
            World w;                                              // the table's length
            w.dst.pt_cap = 200; w.dst.pt_obs_cap = 400;
            w.pts.tab = table(edge[e], edge[e] ? 3 : 0); w.pts.bind(12, 9);
            MapInsertPlan P;
            CHECK(w.kf2kf(&P) == PLSLAM_OK && P.k[0].w_tab == tiles[e] && P.k[0].n_tab == edge[e] && P.k[0].w_lm == 1 && P.k[1].w_tab == 1);
            check_layout(P, w.src);
        }
        for (int e = 0; e < 4; ++e) {
            World w;                                              // S.n + m: no table where the sum is 0
            if (edge[e] == 0) { w.pts.k.table = nullptr; w.src.points.n_obs = 0; }
            w.pts.tab = table(12, 3); if (edge[e]) w.pts.bind(12, 9);
            w.src.points.n = edge[e] ? edge[e] - 3 : 0;
            w.dst.pt_cap = 300; w.dst.pt_obs_cap = 400;
            MapInsertPlan P;
            CHECK(w.kf2kf(&P) == PLSLAM_OK && P.k[0].need_lm == edge[e] && P.k[0].w_lm == tiles[e]);
            check_layout(P, w.src);
            if (edge[e]) {                                        // map <-> KF makes no landmark: S.n alone counts there, the
                w.src.points.n = edge[e];                         // kernel is launched over S.n + m all the same
                CHECK(w.map2kf(&P) == PLSLAM_OK && P.k[0].need_lm == edge[e] && P.k[0].w_lm == (edge[e] + 3 > 256 ? 2u : 1u));
                check_layout(P, w.src);
            }
        }
        for (int e = 0; e < 4; ++e) {
            World w;                                              // n_obs + 2 m
            if (edge[e] == 0) { w.pts.k.table = nullptr; w.src.points.n = 0; }
            w.pts.tab = table(12, 3); if (edge[e]) w.pts.bind(12, 9);
            w.src.points.n_obs = edge[e] ? edge[e] - 6 : 0;
            w.dst.pt_cap = 300; w.dst.pt_obs_cap = 400;
            MapInsertPlan P;
            CHECK(w.kf2kf(&P) == PLSLAM_OK && P.k[0].need_obs == edge[e]);
            check_layout(P, w.src);
        }
        // part: three chains over the table's tiles and one over the landmarks': 257 entries, 255 + 3 landmarks -> 3 * 2 + 2 words
        World w;
        w.pts.tab = table(257, 3); w.pts.bind(12, 9);
        w.src.points.n = 255;
        w.dst.pt_cap = 300; w.dst.pt_obs_cap = 400;
        MapInsertPlan P;
        CHECK(w.kf2kf(&P) == PLSLAM_OK && P.k[0].w_tab == 2 && P.k[0].w_lm == 2 && P.k[1].o_app == P.k[0].o_part + 256);
        check_layout(P, w.src);
    });
    run("pack_into_an_exact_buffer", [] {
        World w;
        const Kind* K[2] = {&w.pts, &w.lns};
        for (int mode = 0; mode < 2; ++mode) {
            MapInsertPlan P;
            CHECK((mode ? w.map2kf(&P) : w.kf2kf(&P)) == PLSLAM_OK);
            std::vector<char> stage(P.stage_bytes, (char)0x5a);   // exactly stage_bytes: a byte beyond is the sanitizer's to catch
            map_insert_pack(P, mode ? nullptr : w.T1.data(), w.T2.data(), stage.data());
            const char* st = stage.data();
            auto at = [&](size_t off) { return st + (off - P.stage_off); };
            const std::vector<double> zero(16, 0.0);
            CHECK(!memcmp(at(P.o_T), mode ? zero.data() : w.T1.data(), 128));      // T1 is absent in map <-> KF mode
            CHECK(!memcmp(at(P.o_T) + 128, w.T2.data(), 128));
            for (int k = 0; k < 2; ++k) {
                const MapInsertKindPlan& Q = P.k[k];
                CHECK(!memcmp(at(Q.o_tab), K[k]->tab.data(), K[k]->tab.size() * 4) && at(Q.o_tab)[K[k]->tab.size() * 4] == 0);
                if (mode == 0) {
                    CHECK(!memcmp(at(Q.o_P1), K[k]->P1.data(), K[k]->P1.size() * 8) && !memcmp(at(Q.o_o1), K[k]->o1.data(), K[k]->o1.size() * 8));
                } else {
                    CHECK(Q.n_prev == 0 && at(Q.o_P1)[0] == 0 && at(Q.o_o1)[0] == 0);   // keyframe 1's rows are not staged
                }
                CHECK(!memcmp(at(Q.o_P2), K[k]->P2.data(), K[k]->P2.size() * 8) && !memcmp(at(Q.o_o2), K[k]->o2.data(), K[k]->o2.size() * 8));
                CHECK(Q.o_o2 - P.stage_off + K[k]->o2.size() * 8 + 8 <= P.stage_bytes);
            }
        }
        // a call without any table stages the transforms alone
        MapInsertPlan P;
        CHECK(map_insert_plan(MAP_INSERT_KF2KF, &w.src, &w.dst, 3, 4, w.T1.data(), w.T2.data(), nullptr, nullptr, &P) == PLSLAM_OK);
        std::vector<char> stage(P.stage_bytes, (char)0x5a);
        map_insert_pack(P, w.T1.data(), w.T2.data(), stage.data());
        CHECK(!memcmp(stage.data(), w.T1.data(), 128) && stage[256] == 0 && stage[P.stage_bytes - 1] == 0);
    });
    return n_failed ? 1 : 0;
}
