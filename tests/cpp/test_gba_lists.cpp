// The host-built lists of the global bundle adjustment (plslam_amd/csrc/gba_lists.hpp) on the CPU: no device, no HIP header, no
// library.  Hand cases whose expectations come from the comments here and from a brute-force restatement (a triple loop over
// landmarks and their observation pairs), not from the code under test: one "PASS <case>" or "FAIL <case>: <what>" line each,
// exit status 1 when any failed; and a dump mode (--dump FILE) that reads one problem from a text file and prints every list for
// tests/test_gba_lists_cpu.py to compare with tests/test_gba_cpu.py::plan_layout.
//   g++ -std=c++17 -I plslam_amd/csrc -I include tests/cpp/test_gba_lists.cpp
#include <cstdio>
#include <cstring>
#include <fstream>
#include <functional>
#include <map>
#include <string>
#include <utility>

#include "gba_lists.hpp"

using namespace plslam;

namespace {

std::string g_fail;     // first failure of the running case
#define CHECK(cond)                                                                          \
    do {                                                                                     \
        if (!(cond) && g_fail.empty()) g_fail = std::string(#cond) + " (line " + std::to_string(__LINE__) + ")"; \
    } while (0)

using V = std::vector<int32_t>;

// optimised keyframe k (local index) is map slot kf_list[k]; local -1 stands for the fixed keyframe in map slot 0
struct Problem {
    int32_t n_map = 0, npt = 0, nls = 0;
    V kf_list, pt, ls;                        // Vector6i rows
    explicit Problem(int32_t nkf) : n_map(nkf + 1) { for (int32_t k = 0; k < nkf; ++k) kf_list.push_back(k + 1); }
    int32_t nkf() const { return (int32_t)kf_list.size(); }
    void obs(bool line, int32_t lm, int32_t local)
    {
        V& rows = line ? ls : pt;
        const int32_t o = (int32_t)rows.size() / 6;
        const int32_t row[6] = {1000 + lm, lm, o, local < 0 ? 0 : kf_list[local], local, 1};
        rows.insert(rows.end(), row, row + 6);
    }
    // landmark of a new index seen by the given local keyframes, in that list order
    void point(std::initializer_list<int32_t> kfs) { for (int32_t k : kfs) obs(false, npt, k); ++npt; }
    void line(std::initializer_list<int32_t> kfs) { for (int32_t k : kfs) obs(true, nls, k); ++nls; }
    int build(GbaLists& L) const
    {
        return gba_lists_build(n_map, nkf(), kf_list.data(), npt, nls, pt.data(), (int32_t)pt.size() / 6, ls.data(),
                               (int32_t)ls.size() / 6, &L);
    }
};

// the brute-force restatement: per lower block (k1, k2) the point pairs and the line pairs, landmark after landmark, o1 and o2
// in list order; every diagonal block exists
struct Want { std::vector<std::pair<int32_t, int32_t>> kind[2]; };
std::map<std::pair<int32_t, int32_t>, Want> brute(const Problem& p)
{
    std::map<std::pair<int32_t, int32_t>, Want> w;
    for (int32_t k = 0; k < p.nkf(); ++k) w[{k, k}];
    for (int line = 0; line < 2; ++line) {
        const V& rows = line ? p.ls : p.pt;
        const int32_t n = (int32_t)rows.size() / 6;
        for (int32_t j = 0; j < (line ? p.nls : p.npt); ++j)
            for (int32_t o1 = 0; o1 < n; ++o1)
                for (int32_t o2 = 0; o2 < n; ++o2) {
                    const int32_t k1 = rows[6 * o1 + 4], k2 = rows[6 * o2 + 4];
                    if (rows[6 * o1 + 1] == j && rows[6 * o2 + 1] == j && k2 >= 0 && k1 >= k2) w[{k1, k2}].kind[line].push_back({o1, o2});
                }
    }
    return w;
}

// every list of L against the restatement; returns the chunk sizes per block, in block order
std::vector<V> check(const Problem& p, const GbaLists& L)
{
    std::vector<V> sizes;
    const int32_t np = (int32_t)p.pt.size() / 6, nl = (int32_t)p.ls.size() / 6, nkf = p.nkf();
    CHECK((int32_t)L.plm.size() == np && (int32_t)L.pkf.size() == np && (int32_t)L.pslot.size() == np);
    CHECK((int32_t)L.llm.size() == nl && (int32_t)L.lkf.size() == nl && (int32_t)L.lslot.size() == nl);
    if (!g_fail.empty()) return sizes;
    for (int32_t o = 0; o < np; ++o) {        // a point of an optimised keyframe reads the estimate slot behind the map's
        const int32_t* v = &p.pt[6 * (size_t)o];
        CHECK(L.plm[o] == v[1] && L.pkf[o] == v[4] && L.pslot[o] == (v[4] >= 0 ? p.n_map + v[4] : v[3]));
    }
    for (int32_t o = 0; o < nl; ++o) {        // a line always reads the stored pose
        const int32_t* v = &p.ls[6 * (size_t)o];
        CHECK(L.llm[o] == v[1] && L.lkf[o] == v[4] && L.lslot[o] == v[3]);
    }
    // the four CSR lists: observations by optimised keyframes only, in list order
    auto csr_is = [&](const V& ptr, const V& ids, const V& key, const V& kf, int32_t nkeys) {
        CHECK((int32_t)ptr.size() == nkeys + 1 && ptr[0] == 0 && (int32_t)ids.size() == ptr[nkeys]);
        for (int32_t k = 0; k < nkeys && g_fail.empty(); ++k) {
            V want;
            for (size_t o = 0; o < key.size(); ++o) if (key[o] == k && kf[o] >= 0) want.push_back((int32_t)o);
            CHECK(V(ids.begin() + ptr[k], ids.begin() + ptr[k + 1]) == want);
        }
    };
    csr_is(L.lpp, L.lpo, L.plm, L.pkf, p.npt);
    csr_is(L.llp, L.llo, L.llm, L.lkf, p.nls);
    csr_is(L.kpp, L.kpo, L.pkf, L.pkf, nkf);
    csr_is(L.klp, L.klo, L.lkf, L.lkf, nkf);
    // blocks sorted by (k1, k2); a block's chunks: its point pairs, then its line pairs, at most GBA_CHUNK of one kind each
    const auto want = brute(p);
    CHECK(L.blks.size() == want.size());
    size_t b = 0, c = 0, q = 0;
    for (const auto& kv : want) {
        if (!g_fail.empty() || b >= L.blks.size()) break;
        const GbaBlock& B = L.blks[b];
        CHECK(B.k1 == kv.first.first && B.k2 == kv.first.second && B.k1 >= B.k2 && B.c0 == (int32_t)c);
        V sz;
        for (int line = 0; line < 2; ++line) {
            const auto& pr = kv.second.kind[line];
            for (size_t i = 0; i < pr.size(); i += GBA_CHUNK) {
                const int32_t n = (int32_t)std::min<size_t>(GBA_CHUNK, pr.size() - i);
                CHECK(c < L.chks.size());
                if (!g_fail.empty()) return sizes;
                const GbaChunk& C = L.chks[c++];
                CHECK(C.blk == (int32_t)b && C.line == line && C.p0 == (int32_t)q && C.np == n);
                for (int32_t u = 0; u < n; ++u, ++q) {
                    CHECK(q < L.pairs.size());
                    if (!g_fail.empty()) return sizes;
                    CHECK(L.pairs[q].o1 == pr[i + u].first && L.pairs[q].o2 == pr[i + u].second);
                }
                sz.push_back(n);
            }
        }
        CHECK(B.c1 == (int32_t)c);
        sizes.push_back(sz);
        ++b;
    }
    CHECK(c == L.chks.size() && q == L.pairs.size());
    return sizes;
}

int n_failed = 0;
void run(const char* name, const std::function<void()>& body)
{
    g_fail.clear();
    body();
    if (g_fail.empty()) std::printf("PASS %s\n", name);
    else { std::printf("FAIL %s: %s\n", name, g_fail.c_str()); ++n_failed; }
}
void refused(const char* name, const std::function<void(Problem&)>& spoil)
{
    run(name, [&] {
        Problem p(3);
        p.point({0, 1}); p.point({-1, 2}); p.line({1, 2}); p.line({2, -1, 0});
        GbaLists L;
        CHECK(p.build(L) == PLSLAM_OK);
        spoil(p);
        CHECK(p.build(L) == PLSLAM_EINVAL && L.why[0] != 0);
    });
}

void hand_cases()
{
    run("one_keyframe_no_observation", [] {
        Problem p(1);
        GbaLists L;
        CHECK(p.build(L) == PLSLAM_OK);
        CHECK(L.blks.size() == 1 && L.blks[0].k1 == 0 && L.blks[0].k2 == 0 && L.blks[0].c0 == 0 && L.blks[0].c1 == 0);
        CHECK(L.chks.empty() && L.pairs.empty() && L.kpp == V({0, 0}) && L.klp == V({0, 0}) && L.lpp == V({0}) && L.llp == V({0}));
        check(p, L);
    });
    run("landmark_seen_by_keyframe_0_only", [] {
        // point 0 and line 1 are seen by the fixed keyframe alone: an empty range of the landmark lists, no pair, and their rows
        // read map slot 0
        Problem p(2);
        p.point({-1}); p.point({0, 1}); p.line({1, 0}); p.line({-1});
        GbaLists L;
        CHECK(p.build(L) == PLSLAM_OK);
        CHECK(L.lpp == V({0, 0, 2}) && L.lpo == V({1, 2}) && L.llp == V({0, 2, 2}) && L.llo == V({0, 1}));
        CHECK(L.pslot == V({0, 3 + 0, 3 + 1}) && L.lslot == V({2, 1, 0}) && L.pkf == V({-1, 0, 1}));
        CHECK(L.kpp == V({0, 1, 2}) && L.kpo == V({1, 2}) && L.klp == V({0, 1, 2}) && L.klo == V({1, 0}));
        const std::vector<V> sz = check(p, L);
        CHECK(sz == std::vector<V>({{1, 1}, {1, 1}, {1, 1}}));       // (0,0), (1,0), (1,1): one point pair and one line pair each
        // block (1, 0): the point's pair is (the observation by keyframe 1, the one by keyframe 0) = (2, 1); the line's (0, 1)
        CHECK(L.pairs.size() == 6 && L.pairs[2].o1 == 2 && L.pairs[2].o2 == 1 && L.pairs[3].o1 == 0 && L.pairs[3].o2 == 1);
    });
    run("chunk_boundaries", [] {
        // 64 points and 65 lines seen by keyframes 0 and 1, 65 points by 0 and 2, one point by 1 and 2; the two observations of
        // a landmark in either list order.  Block (1,0): exactly 64 point pairs -- the point run ends on the chunk boundary --
        // then 65 line pairs; (2,0): 65 point pairs; (2,1): a single pair.  Diagonals: (0,0) 129 points + 65 lines; (1,1) 65
        // points + 65 lines; (2,2) 66 points.
        Problem p(3);
        for (int j = 0; j < 64; ++j) { if (j % 2) p.point({1, 0}); else p.point({0, 1}); }
        for (int j = 0; j < 65; ++j) { if (j % 3) p.line({0, 1}); else p.line({1, -1, 0}); }
        for (int j = 0; j < 65; ++j) { if (j % 2) p.point({0, 2}); else p.point({2, 0}); }
        p.point({2, 1});
        GbaLists L;
        CHECK(p.build(L) == PLSLAM_OK);
        const std::vector<V> sz = check(p, L);
        CHECK(sz == std::vector<V>({{64, 64, 1, 64, 1}, {64, 64, 1}, {64, 1, 64, 1}, {64, 1}, {1}, {64, 2}}));
        CHECK(L.blks.size() == 6 && L.blks[1].k1 == 1 && L.blks[1].k2 == 0 && L.blks[4].k1 == 2 && L.blks[4].k2 == 1);
        if (g_fail.empty()) {
            const GbaChunk* c = &L.chks[L.blks[1].c0];
            CHECK(c[0].line == 0 && c[1].line == 1 && c[2].line == 1);
            // pairs of one kind inside a block are in landmark order, (higher keyframe's observation, lower one's)
            for (int32_t i = 0; i < 64; ++i) {
                const GbaPair q = L.pairs[c[0].p0 + i];
                CHECK(L.plm[q.o1] == i && L.plm[q.o2] == i && L.pkf[q.o1] == 1 && L.pkf[q.o2] == 0);
            }
            for (int32_t i = 0; i < 65; ++i) {
                const GbaPair q = L.pairs[c[1].p0 + i];
                CHECK(L.llm[q.o1] == i && L.llm[q.o2] == i && L.lkf[q.o1] == 1 && L.lkf[q.o2] == 0);
            }
            const GbaChunk& one = L.chks[L.blks[4].c0];
            CHECK(one.np == 1 && L.plm[L.pairs[one.p0].o1] == 129 && L.pkf[L.pairs[one.p0].o1] == 2 && L.pkf[L.pairs[one.p0].o2] == 1);
        }
    });

    // ---- every column refusal: rows 0 .. of the valid problem of refused() spoilt one at a time
    refused("refuse_point_landmark_index_past_the_end", [](Problem& p) { p.pt[6 * 1 + 1] = p.npt; });
    refused("refuse_point_landmark_index_negative", [](Problem& p) { p.pt[6 * 0 + 1] = -1; });
    refused("refuse_line_landmark_index_past_the_end", [](Problem& p) { p.ls[6 * 2 + 1] = p.nls; });
    refused("refuse_point_local_keyframe_below_minus_one", [](Problem& p) { p.pt[6 * 2 + 4] = -2; });
    refused("refuse_line_local_keyframe_below_minus_one", [](Problem& p) { p.ls[6 * 3 + 4] = -2; });
    refused("refuse_point_local_keyframe_past_the_end", [](Problem& p) { p.pt[6 * 0 + 4] = 3; });
    refused("refuse_point_map_keyframe_out_of_range", [](Problem& p) { p.pt[6 * 2 + 3] = p.n_map; });
    refused("refuse_point_local_keyframe_is_not_its_map_keyframe", [](Problem& p) { p.pt[6 * 1 + 3] = 3; });    // kf_list[1] = 2
    refused("refuse_line_local_keyframe_is_not_its_map_keyframe", [](Problem& p) { p.ls[6 * 0 + 4] = 0; });     // its map slot is 2
    refused("refuse_kf_list_out_of_range", [](Problem& p) { p.kf_list[2] = p.n_map; });
}

void line_out(const char* key, const V& v)
{
    std::printf("%s", key);
    for (int32_t x : v) std::printf(" %d", x);
    std::printf("\n");
}

// FILE: n_map_kf nkf npt nls n_pt_obs n_ls_obs | kf_list (nkf) | point rows (6 each) | line rows (6 each)
int dump(const char* path)
{
    std::ifstream f(path);
    int32_t n_map, nkf, npt, nls, np, nl;
    if (!(f >> n_map >> nkf >> npt >> nls >> np >> nl) || nkf < 0 || np < 0 || nl < 0) return 2;
    V kf_list(nkf), pt(6 * (size_t)np), ls(6 * (size_t)nl);
    for (auto& v : kf_list) if (!(f >> v)) return 2;
    for (auto& v : pt) if (!(f >> v)) return 2;
    for (auto& v : ls) if (!(f >> v)) return 2;
    GbaLists L;
    const int rc = gba_lists_build(n_map, nkf, kf_list.data(), npt, nls, pt.data(), np, ls.data(), nl, &L);
    std::printf("rc %d\n", rc);
    if (rc) return 0;
    V blks, chks, pairs;
    for (const GbaBlock& b : L.blks) { blks.push_back(b.k1); blks.push_back(b.k2); blks.push_back(b.c0); blks.push_back(b.c1); }
    for (const GbaChunk& c : L.chks) { chks.push_back(c.blk); chks.push_back(c.line); chks.push_back(c.p0); chks.push_back(c.np); }
    for (const GbaPair& q : L.pairs) { pairs.push_back(q.o1); pairs.push_back(q.o2); }
    line_out("blks", blks); line_out("chks", chks); line_out("pairs", pairs);
    line_out("plm", L.plm); line_out("pkf", L.pkf); line_out("pslot", L.pslot);
    line_out("llm", L.llm); line_out("lkf", L.lkf); line_out("lslot", L.lslot);
    line_out("lpp", L.lpp); line_out("lpo", L.lpo); line_out("llp", L.llp); line_out("llo", L.llo);
    line_out("kpp", L.kpp); line_out("kpo", L.kpo); line_out("klp", L.klp); line_out("klo", L.klo);
    return 0;
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc == 3 && !std::strcmp(argv[1], "--dump")) return dump(argv[2]);
    hand_cases();
    return n_failed ? 1 : 0;
}
