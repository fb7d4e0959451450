// The host half of the loop-closure pose graph (plslam_amd/csrc/pgo_graph.hpp) on the CPU: no device, no HIP header, no library.
// Hand cases whose expectations are worked out in the comments here (not taken from the code under test), one "PASS <case>" or
// "FAIL <case>: <what>" line each, exit status 1 when any failed; and a dump mode (--dump FILE) that reads one case from a text
// file and prints every list of the PgoGraph for tests/test_pgo_graph_cpu.py to compare with tests/pgo_ref.py.
//   g++ -std=c++17 -I plslam_amd/csrc -I include tests/cpp/test_pgo_graph.cpp
#include <cstdio>
#include <cstring>
#include <fstream>
#include <functional>
#include <string>

#include "pgo_graph.hpp"

using namespace plslam;

namespace {

std::string g_fail;     // first failure of the running case
#define CHECK(cond)                                                                          \
    do {                                                                                     \
        if (!(cond) && g_fail.empty()) g_fail = std::string(#cond) + " (line " + std::to_string(__LINE__) + ")"; \
    } while (0)

const plslam_pgo_params PRM{75, 75, 100, 10, 1e-10};

struct Input {
    int32_t n = 0;
    std::vector<uint8_t> valid;
    std::vector<int32_t> fg, lc;
    explicit Input(int32_t n_, std::initializer_list<int32_t> null_slots = {}) : n(n_), valid(n_, 1), fg((size_t)n_ * n_, 0)
    {
        for (int32_t k : null_slots) valid[k] = 0;
    }
    void cov(int32_t i, int32_t j, int32_t c) { fg[(size_t)i * n + j] = fg[(size_t)j * n + i] = c; }
    void loop(int32_t a, int32_t b, int32_t flag = 1) { lc.push_back(a); lc.push_back(b); lc.push_back(flag); }
    int build(PgoGraph& G, const plslam_pgo_params& p = PRM) const
    {
        static const int32_t none[3] = {0, 0, 0};          // no entry: still a list, so that n_lc = 0 is what is refused
        return pgo_graph_build(&p, n, valid.data(), fg.data(), (int32_t)lc.size() / 3, lc.empty() ? none : lc.data(), &G);
    }
};

bool edges_are(const PgoGraph& G, const std::vector<std::vector<int32_t>>& want)     // {x, y, elc} per edge
{
    if (G.ev.size() != want.size() || G.elc.size() != want.size() || G.ne != (int32_t)want.size()) return false;
    for (size_t e = 0; e < want.size(); ++e)
        if (G.ev[e].x != want[e][0] || G.ev[e].y != want[e][1] || G.elc[e] != want[e][2]) return false;
    return true;
}
bool tree_is(const PgoGraph& G, const std::vector<std::vector<int32_t>>& want)      // {v, u, e, first} per entry
{
    if (G.tree.size() != want.size()) return false;
    for (size_t k = 0; k < want.size(); ++k)
        if (G.tree[k].v != want[k][0] || G.tree[k].u != want[k][1] || G.tree[k].e != want[k][2] || G.tree[k].first != want[k][3]) return false;
    return true;
}
std::vector<int32_t> block_starts(const PgoGraph& G)       // cs of the first row of every 6-row block, all six rows checked equal
{
    std::vector<int32_t> s;
    for (int32_t r = 0; r < G.N; ++r) {
        if (r % 6 == 0) s.push_back(G.env.cs[r]);
        else if (G.env.cs[r] != s.back()) s.push_back(-1000);
    }
    return s;
}
using V = std::vector<int32_t>;

int n_failed = 0;
void run(const char* name, const std::function<void()>& body)
{
    g_fail.clear();
    body();
    if (g_fail.empty()) std::printf("PASS %s\n", name);
    else { std::printf("FAIL %s: %s\n", name, g_fail.c_str()); ++n_failed; }
}
void refused(const char* name, int code, const Input& in, const plslam_pgo_params& p = PRM)
{
    run(name, [&] {
        PgoGraph G;
        CHECK(in.build(G, p) == code);
        CHECK(G.why[0] != 0);
    });
}

void hand_cases()
{
    run("two_keyframes", [] {
        // edges: (0, 1) because j - i == 1, then the LC entry's (0, 1).  Vertex 1 is the one active vertex: N = 6, every row
        // starts at column 0, the widest (row 5) is 5 wide.  Both edges have the active vertex as their second end: codes
        // 4 e + 1 into target (0, 0), 2 e + 1 into its right-hand side.
        Input in(2);
        in.loop(0, 1);
        PgoGraph G;
        CHECK(in.build(G) == PLSLAM_OK);
        CHECK(G.nv == 2 && G.ne == 2 && G.na == 1 && G.N == 6 && G.env.bw == 5 && G.kf_curr == 1 && G.nlvl == 1);
        CHECK(edges_are(G, {{0, 1, -1}, {0, 1, 0}}));
        CHECK(G.vslot == V({0, 1}) && G.vcol == V({-1, 0}) && G.ord == V({0}));
        CHECK(G.tg.size() == 1 && G.tg[0].row == 0 && G.tg[0].col == 0 && G.tg[0].c0 == 0 && G.tg[0].c1 == 2);
        CHECK(G.contrib == V({1, 5}) && G.rptr == V({0, 2}) && G.rlist == V({1, 3}));
        CHECK(tree_is(G, {{1, 0, 0, 1}}) && G.lvl_ptr == V({0, 1}));
        CHECK(G.env.cs == V(6, 0) && G.env.reach == V(6, 5));
        CHECK(G.env.off == std::vector<int64_t>({0, 1, 3, 6, 10, 15, 21}));
        // vertex 0 is the entry's (0)-end: no init entry; vertex 1 its (1)-end: entry 0
        CHECK(G.vinit.size() == 2 && G.vinit[0].x == 0 && G.vinit[0].y == -1 && G.vinit[1].x == 1 && G.vinit[1].y == 0);
    });
    run("null_keyframe_inside_the_range", [] {
        // slots 0 1 [2 NULL] 3: vertices 0, 1, 2 (slot 3).  Slots 1 and 3 are two apart: j - i == 1 does not join them over the
        // NULL slot, so vertex 2 hangs on the LC entry alone ...
        Input in(4, {2});
        in.loop(0, 3);
        PgoGraph G;
        CHECK(in.build(G) == PLSLAM_OK);
        CHECK(G.nv == 3 && G.vslot == V({0, 1, 3}) && edges_are(G, {{0, 1, -1}, {0, 2, 0}}));
        in.cov(1, 3, 74);                    // ... below both thresholds: still no edge
        CHECK(in.build(G) == PLSLAM_OK && G.ne == 2);
        in.cov(1, 3, 75);                    // ... or on full_graph: created between (0, 1) and the LC edge
        CHECK(in.build(G) == PLSLAM_OK && edges_are(G, {{0, 1, -1}, {1, 2, -1}, {0, 2, 0}}));
        in.cov(1, 2, 500);                   // covisibility with the NULL slot itself makes nothing
        CHECK(in.build(G) == PLSLAM_OK && G.ne == 3 && G.nv == 3);
    });
    run("vinit_break_rule", [] {
        // entries (2, 4), (0, 2), (1, 5): slot 2 is entry 0's (0)-end, met before entry 1 names it as a (1)-end: the scan
        // breaks, no init entry.  Slots 0 and 1 are (0)-ends of entries 1 and 2 and nobody's (1)-end before that.
        Input in(6);
        in.loop(2, 4); in.loop(0, 2); in.loop(1, 5);
        PgoGraph G;
        CHECK(in.build(G) == PLSLAM_OK && G.nv == 6 && G.kf_curr == 5);
        const int32_t want[6] = {-1, -1, -1, -1, 0, 2};
        for (int v = 0; v < 6 && G.nv == 6; ++v) CHECK(G.vinit[v].x == v && G.vinit[v].y == want[v]);
        // the other order, (0, 2) first: slot 2 is a (1)-end first -> entry 0; kf_curr falls to 4
        Input in2(6);
        in2.loop(0, 2); in2.loop(2, 4);
        CHECK(in2.build(G) == PLSLAM_OK && G.nv == 5 && G.kf_curr == 4);
        const int32_t want2[5] = {-1, -1, 0, -1, 1};
        for (int v = 0; v < 5 && G.nv == 5; ++v) CHECK(G.vinit[v].y == want2[v]);
    });
    run("bfs_tie_by_incident_edge_order", [] {
        // e0 (0,1) e1 (0,2) e2 (1,2) e3 (1,3) e4 (2,3) e5 (3,4), LC e6 (1,4), e7 (3,0).  From 0 in incident order e0, e1, e7:
        // 1, 2, then 3 through e7 whose FIRST vertex is 3, not the parent 0 (first = 0).  Vertex 4 is one step from 1 (e6) and
        // from 3 (e5): 1 left the queue first, so e6 sets it although e5 was created earlier.
        Input in(5);
        in.cov(0, 2, 100); in.cov(1, 3, 100);
        in.loop(1, 4); in.loop(3, 0);
        PgoGraph G;
        CHECK(in.build(G) == PLSLAM_OK);
        CHECK(edges_are(G, {{0, 1, -1}, {0, 2, -1}, {1, 2, -1}, {1, 3, -1}, {2, 3, -1}, {3, 4, -1}, {1, 4, 0}, {3, 0, 1}}));
        CHECK(tree_is(G, {{1, 0, 0, 1}, {2, 0, 1, 1}, {3, 0, 7, 0}, {4, 1, 6, 1}}));
        CHECK(G.lvl_ptr == V({0, 3, 4}) && G.nlvl == 2);
    });
    run("two_chains_meeting_at_vertex_0", [] {
        // slots 0 1 2 3 [4 NULL] 5 6, full_graph(0, 5), LC (0, 6): vertices v0..v5 = slots 0 1 2 3 5 6; edges e0 (v0,v1)
        // e1 (v0,v4) e2 (v1,v2) e3 (v2,v3) e4 (v4,v5) e5 LC (v0,v5).  Active a0..a4 = v1..v5; their adjacency has the components
        // a0-a1-a2 and a3-a4 (vertex 0 is not in it).  Degrees 1 2 1 1 1: RCM starts at a0, walks a1, a2, restarts at a3 (the
        // unseen vertex of least degree and lowest index), a4; reversed: 4 3 2 1 0.
        Input in(7, {4});
        in.cov(0, 5, 80);
        in.loop(0, 6);
        PgoGraph G;
        CHECK(in.build(G) == PLSLAM_OK);
        CHECK(edges_are(G, {{0, 1, -1}, {0, 4, -1}, {1, 2, -1}, {2, 3, -1}, {4, 5, -1}, {0, 5, 0}}));
        CHECK(G.na == 5 && G.ord == V({4, 3, 2, 1, 0}) && G.vcol == V({-1, 4, 3, 2, 1, 0}));
        // block p starts at the lowest position among itself and its neighbours: a4|a3 -> 0, 0; a2 (nb a1 at 3) -> 2;
        // a1 (nbs a0 at 4, a2 at 2) -> 2; a0 (nb a1 at 3) -> 3
        CHECK(block_starts(G) == V({0, 0, 12, 12, 18}) && G.env.bw == 11 && G.env.off[G.N] == 21 + 57 + 21 + 57 + 57);
    });
    run("star_neighbours_by_degree_then_index", [] {
        // slots 0 1 [2] 3 4 5 [6] 7 [8] 9; full_graph (1,3) (3,7) (3,9); LC (0, 9).  Vertices v0..v6 = slots 0 1 3 4 5 7 9; edges
        // e0 (v0,v1) e1 (v1,v2) e2 (v2,v3) e3 (v2,v5) e4 (v2,v6) e5 (v3,v4) e6 LC (v0,v6).  Active a0..a5 = v1..v6: a1 is the
        // centre with neighbours a0, a2, a4, a5; a2 has a3 behind it.  Degrees 1 4 2 1 1 1.  RCM starts at a0, then a1, whose
        // unseen neighbours come by ascending degree, then index: a4, a5 (degree 1) before a2 (degree 2) although a2 has the
        // lowest index; then a3.  Reversed: 3 2 5 4 1 0.
        Input in(10, {2, 6, 8});
        in.cov(1, 3, 80); in.cov(3, 7, 80); in.cov(3, 9, 80);
        in.loop(0, 9);
        PgoGraph G;
        CHECK(in.build(G) == PLSLAM_OK);
        CHECK(edges_are(G, {{0, 1, -1}, {1, 2, -1}, {2, 3, -1}, {2, 5, -1}, {2, 6, -1}, {3, 4, -1}, {0, 6, 0}}));
        CHECK(G.ord == V({3, 2, 5, 4, 1, 0}) && G.vcol == V({-1, 5, 4, 1, 0, 3, 2}));
        // positions: a3 0, a2 1, a5 2, a4 3, a1 4, a0 5.  Starts: a3 (nb a2) 0; a2 (nbs a1, a3) 0; a5 (nb a1) 2; a4 (nb a1) 3;
        // a1 (nbs at 5, 1, 3, 2) 1; a0 (nb a1) 4.  Widest row: the last of block 4, 29 - 6.
        CHECK(block_starts(G) == V({0, 0, 12, 18, 6, 24}) && G.env.bw == 23);
    });

    // ---- the refusals of tests/test_gpu_pgo.py::test_refusals, and the argument checks in front of them
    { Input in(30); in.loop(5, 29); in.valid[5] = 0; refused("refuse_lc_entry_names_a_null_keyframe", PLSLAM_EINVAL, in); }
    { Input in(30); in.loop(0, 30); refused("refuse_lc_entry_out_of_range", PLSLAM_EINVAL, in); }
    { Input in(30); in.loop(-1, 4); refused("refuse_lc_entry_negative", PLSLAM_EINVAL, in); }
    { Input in(30, {0}); in.loop(5, 29); refused("refuse_keyframe_0_null", PLSLAM_EINVAL, in); }
    { Input in(30); refused("refuse_no_lc_entry", PLSLAM_EINVAL, in); }
    { Input in(30); in.loop(7, 7); refused("refuse_lc_entry_of_one_keyframe", PLSLAM_EINVAL, in); }
    { Input in(30, {10, 11, 12, 13, 14}); in.loop(16, 25); refused("refuse_no_path_to_vertex_0", PLSLAM_EINVAL, in); }
    { Input in(8); in.loop(0, 7); plslam_pgo_params p = PRM; p.max_iters_pgo = -1; refused("refuse_negative_max_iters", PLSLAM_EINVAL, in, p); }
    { Input in(8); in.loop(0, 7); plslam_pgo_params p = PRM; p.max_trials = 0; refused("refuse_zero_max_trials", PLSLAM_EINVAL, in, p); }
    run("refuse_null_arguments", [] {
        Input in(8);
        in.loop(0, 7);
        PgoGraph G;
        const int32_t n_lc = 1;
        CHECK(pgo_graph_build(nullptr, 8, in.valid.data(), in.fg.data(), n_lc, in.lc.data(), &G) == PLSLAM_EINVAL);
        CHECK(pgo_graph_build(&PRM, 8, nullptr, in.fg.data(), n_lc, in.lc.data(), &G) == PLSLAM_EINVAL);
        CHECK(pgo_graph_build(&PRM, 8, in.valid.data(), nullptr, n_lc, in.lc.data(), &G) == PLSLAM_EINVAL);
        CHECK(pgo_graph_build(&PRM, 8, in.valid.data(), in.fg.data(), n_lc, nullptr, &G) == PLSLAM_EINVAL);
        CHECK(pgo_graph_build(&PRM, 0, in.valid.data(), in.fg.data(), n_lc, in.lc.data(), &G) == PLSLAM_EINVAL);
        CHECK(in.build(G) == PLSLAM_OK);
    });
    run("refuse_more_than_4096_active_vertices", [] {
        // a plain chain: keyframes 1 .. n - 1 are active.  4097 keyframes: 4096 active, the last size taken; 4098: refused
        static_assert(PLSLAM_GBA_MAX_KEYFRAMES == 4096, "the case is built for this bound");
        PgoGraph G;
        Input big(4098);
        big.loop(0, 4097);
        CHECK(big.build(G) == PLSLAM_ERANGE);
        Input last(4097);
        last.loop(0, 4096);
        CHECK(last.build(G) == PLSLAM_OK && G.na == 4096 && G.N == 6 * 4096 && G.ne == 4097);
    });
}

template <class T> void line(const char* key, const std::vector<T>& v)
{
    std::printf("%s", key);
    for (const T& x : v) std::printf(" %lld", (long long)x);
    std::printf("\n");
}

// FILE: n_map_kf n_lc min_lm_ess_graph min_lm_cov_graph | kf_valid (n) | lc_idx (3 n_lc) | nnz | nnz x (i j count)
int dump(const char* path)
{
    std::ifstream f(path);
    int32_t n = 0, n_lc = 0, nnz = 0;
    plslam_pgo_params p = PRM;
    if (!(f >> n >> n_lc >> p.min_lm_ess_graph >> p.min_lm_cov_graph) || n < 0 || n_lc < 0) return 2;
    std::vector<uint8_t> valid(n);
    std::vector<int32_t> lc(3 * (size_t)n_lc), fg((size_t)n * n, 0);
    for (auto& v : valid) { int x; if (!(f >> x)) return 2; v = (uint8_t)x; }
    for (auto& v : lc) if (!(f >> v)) return 2;
    if (!(f >> nnz)) return 2;
    for (int32_t k = 0; k < nnz; ++k) {
        int32_t i, j, c;
        if (!(f >> i >> j >> c) || i < 0 || i >= n || j < 0 || j >= n) return 2;
        fg[(size_t)i * n + j] = c;
    }
    PgoGraph G;
    const int rc = pgo_graph_build(&p, n, valid.data(), fg.data(), n_lc, lc.data(), &G);
    std::printf("rc %d\n", rc);
    if (rc) return 0;
    std::printf("counts %d %d %d %d %d %d %d %d\n", G.n_map, G.kf_curr, G.nv, G.ne, G.na, G.N, G.nlvl, G.env.bw);
    std::vector<int32_t> ev, tree, tg, vinit;
    for (const PgoPair& e : G.ev) { ev.push_back(e.x); ev.push_back(e.y); }
    for (const PgoLevel& l : G.tree) { tree.push_back(l.v); tree.push_back(l.u); tree.push_back(l.e); tree.push_back(l.first); }
    for (const PgoTarget& t : G.tg) { tg.push_back(t.row); tg.push_back(t.col); tg.push_back(t.c0); tg.push_back(t.c1); }
    for (const PgoPair& v : G.vinit) { vinit.push_back(v.x); vinit.push_back(v.y); }
    line("vslot", G.vslot); line("ev", ev); line("elc", G.elc); line("tree", tree); line("lvl_ptr", G.lvl_ptr);
    line("ord", G.ord); line("vcol", G.vcol); line("cs", G.env.cs); line("off", G.env.off); line("reach", G.env.reach);
    line("tg", tg); line("contrib", G.contrib); line("rptr", G.rptr); line("rlist", G.rlist); line("vinit", vinit);
    return 0;
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc == 3 && !std::strcmp(argv[1], "--dump")) return dump(argv[2]);
    hand_cases();
    return n_failed ? 1 : 0;
}
