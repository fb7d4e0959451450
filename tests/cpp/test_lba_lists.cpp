// The host-built lists of the local BA (plslam_amd/csrc/lba_lists.hpp) on the CPU: no device, no HIP header, no library.  The
// smallest shapes that reach each branch of build_csr, pose_max_chunks and build_schur_pairs; what is expected comes from a
// brute-force restatement here (a triple loop over landmarks and their observation pairs), not from the code under test.
// Prints "PASS <case>" or "FAIL <case>: <what>" per case; exit status 1 when any failed.
//   g++ -std=c++17 -I plslam_amd/csrc tests/cpp/test_lba_lists.cpp
#include <cstdio>
#include <functional>
#include <string>

#include "lba_lists.hpp"

using namespace plslam;

namespace {

std::string g_fail;     // first failure of the running case
#define CHECK(cond)                                                                          \
    do {                                                                                     \
        if (!(cond) && g_fail.empty()) g_fail = std::string(#cond) + " (line " + std::to_string(__LINE__) + ")"; \
    } while (0)

struct Problem {
    int32_t nkf = 0, npt = 0, nls = 0;
    std::vector<int32_t> pt_lm, pt_kf, ls_lm, ls_kf;       // per observation: its landmark, its keyframe (-1: a fixed one)
    void point(int32_t lm, int32_t kf) { pt_lm.push_back(lm); pt_kf.push_back(kf); }
    void line(int32_t lm, int32_t kf) { ls_lm.push_back(lm); ls_kf.push_back(kf); }
};
struct Result {
    CsrLists csr;
    SchurLists sch;
    int32_t nulls = 0, max_block_chunks = 0;
};

bool same(const SchurPair& a, const SchurPair& b) { return a.o1 == b.o1 && a.o2 == b.o2 && a.lm == b.lm && a.line == b.line; }

// the observations with key[o] == k, ascending: what a stable list of them holds
std::vector<int32_t> having(const std::vector<int32_t>& key, int32_t k, int32_t offset = 0)
{
    std::vector<int32_t> v;
    for (size_t o = 0; o < key.size(); ++o)
        if (key[o] == k) v.push_back((int32_t)o + offset);
    return v;
}
void check_list(const std::vector<int32_t>& ptr, const std::vector<int32_t>& ids, int32_t k, const std::vector<int32_t>& want)
{
    CHECK(ptr[k + 1] - ptr[k] == (int32_t)want.size());
    for (size_t i = 0; i < want.size() && g_fail.empty(); ++i) CHECK(ids[ptr[k] + i] == want[i]);
}

Result check(const Problem& p)
{
    Result r;
    const int32_t np = (int32_t)p.pt_lm.size(), nl = (int32_t)p.ls_lm.size(), nkf = p.nkf;
    build_csr(p.pt_lm.data(), p.pt_kf.data(), np, p.ls_lm.data(), p.ls_kf.data(), nl, nkf, p.npt, p.nls, r.csr);
    const CsrLists& c = r.csr;
    // landmark lists: every observation of the landmark, fixed keyframes included, in observation order
    CHECK((int32_t)c.ptp.size() == p.npt + 1 && c.ptp[0] == 0 && c.ptp[p.npt] == np && (int32_t)c.pti.size() == np);
    CHECK((int32_t)c.lsp.size() == p.nls + 1 && c.lsp[0] == 0 && c.lsp[p.nls] == nl && (int32_t)c.lsi.size() == nl);
    for (int32_t j = 0; j < p.npt; ++j) check_list(c.ptp, c.pti, j, having(p.pt_lm, j));
    for (int32_t j = 0; j < p.nls; ++j) check_list(c.lsp, c.lsi, j, having(p.ls_lm, j));
    // keyframe lists: points first, then lines offset by np; nothing of a fixed keyframe
    int32_t n_opt = 0, want_pose_chunks = 0;
    for (int32_t o = 0; o < np; ++o) n_opt += p.pt_kf[o] >= 0;
    for (int32_t o = 0; o < nl; ++o) n_opt += p.ls_kf[o] >= 0;
    CHECK((int32_t)c.kfp.size() == nkf + 1 && c.kfp[0] == 0 && c.kfp[nkf] == n_opt && (int32_t)c.kfi.size() == n_opt);
    for (int32_t k = 0; k < nkf; ++k) {
        std::vector<int32_t> want = having(p.pt_kf, k), ls = having(p.ls_kf, k, np);
        want.insert(want.end(), ls.begin(), ls.end());
        check_list(c.kfp, c.kfi, k, want);
        want_pose_chunks = std::max(want_pose_chunks, ((int32_t)want.size() + POSE_CHUNK - 1) / POSE_CHUNK);
    }
    CHECK(pose_max_chunks(c.kfp) == want_pose_chunks);

    // the pairs, brute force: blocks numbered by walking the upper triangle row by row; per block the point pairs and the line
    // pairs in landmark-then-list order
    std::vector<std::vector<int32_t>> blk((size_t)nkf, std::vector<int32_t>((size_t)nkf, -1));
    int32_t nblk = 0;
    for (int32_t k1 = 0; k1 < nkf; ++k1)
        for (int32_t k2 = k1; k2 < nkf; ++k2) blk[k1][k2] = nblk++;
    std::vector<std::vector<SchurPair>> want_pt((size_t)nblk), want_ls((size_t)nblk);
    for (int line = 0; line < 2; ++line) {
        const std::vector<int32_t>& lm = line ? p.ls_lm : p.pt_lm;
        const std::vector<int32_t>& kf = line ? p.ls_kf : p.pt_kf;
        for (int32_t j = 0; j < (line ? p.nls : p.npt); ++j)
            for (int32_t o1 = 0; o1 < (int32_t)lm.size(); ++o1)
                for (int32_t o2 = 0; o2 < (int32_t)lm.size(); ++o2)
                    if (lm[o1] == j && lm[o2] == j && 0 <= kf[o1] && kf[o1] <= kf[o2])
                        (line ? want_ls : want_pt)[(size_t)blk[kf[o1]][kf[o2]]].push_back(SchurPair{o1, o2, j, line});
    }
    r.sch = build_schur_pairs(c, p.pt_kf, p.ls_kf, nkf);
    const SchurLists& s = r.sch;
    CHECK((int32_t)s.cnt.size() == nblk + 1 && s.cnt[0] == 0 && (int32_t)s.pairs.size() == s.cnt[nblk]);
    for (int32_t B = 0; B < nblk && g_fail.empty(); ++B) {
        const std::vector<SchurPair>&wp = want_pt[(size_t)B], &wl = want_ls[(size_t)B];
        const int32_t npp = (int32_t)wp.size(), nlp = (int32_t)wl.size();
        // the line pairs start on a chunk boundary exactly when the block has both kinds; null pairs fill the gap
        const int32_t line0 = nlp && npp ? (npp + SCH_CHUNK - 1) / SCH_CHUNK * SCH_CHUNK : npp;
        CHECK(s.cnt[B + 1] - s.cnt[B] == line0 + nlp);
        if (!g_fail.empty()) break;
        const SchurPair* q = s.pairs.data() + s.cnt[B];
        for (int32_t i = 0; i < npp; ++i) CHECK(same(q[i], wp[(size_t)i]));
        for (int32_t i = npp; i < line0; ++i) { CHECK(q[i].line == 2); ++r.nulls; }
        for (int32_t i = 0; i < nlp; ++i) CHECK(same(q[line0 + i], wl[(size_t)i]));
        if (nlp && npp) CHECK(line0 % SCH_CHUNK == 0);
        r.max_block_chunks = std::max(r.max_block_chunks, (line0 + nlp + SCH_CHUNK - 1) / SCH_CHUNK);
    }
    CHECK(s.schur_chunks == r.max_block_chunks);
    return r;
}

// `nobs` observations per landmark, observation i of landmark j by keyframe kf(j, i); the landmarks' observations interleaved
// (observation order is i-major), so that a stable list is not the order of arrival by accident
void observe(Problem& p, bool lines, int32_t nlm, int32_t nobs, const std::function<int32_t(int32_t, int32_t)>& kf)
{
    (lines ? p.nls : p.npt) = nlm;
    for (int32_t i = 0; i < nobs; ++i)
        for (int32_t j = 0; j < nlm; ++j) lines ? p.line(j, kf(j, i)) : p.point(j, kf(j, i));
}

int n_failed = 0;
void run(const char* name, const std::function<void()>& body)
{
    g_fail.clear();
    body();
    if (g_fail.empty()) std::printf("PASS %s\n", name);
    else { std::printf("FAIL %s: %s\n", name, g_fail.c_str()); ++n_failed; }
}

}  // namespace

int main()
{
    run("empty", [] {
        Problem p; p.nkf = 3;
        const Result r = check(p);
        CHECK(r.sch.pairs.empty() && r.sch.cnt.size() == 7 && r.sch.schur_chunks == 0 && pose_max_chunks(r.csr.kfp) == 0);
    });
    run("points_only", [] {                  // 3 keyframes, 10 points, 2 observations each
        Problem p; p.nkf = 3;
        observe(p, false, 10, 2, [](int32_t j, int32_t i) { return (j + i) % 3; });
        const Result r = check(p);
        CHECK(r.nulls == 0 && r.sch.pairs.size() == 30 && r.sch.schur_chunks == 1);     // per point: (a, a), (b, b) and one of (a, b), (b, a)
    });
    run("lines_only", [] {                   // 3 keyframes, 7 lines, 3 observations each
        Problem p; p.nkf = 3;
        observe(p, true, 7, 3, [](int32_t j, int32_t i) { return (j + 2 * i) % 3; });
        const Result r = check(p);
        CHECK(r.nulls == 0 && r.sch.pairs.size() == 7 * 6 && r.sch.cnt[1] == 7);        // three keyframes, one observation each: 6 ordered pairs
    });
    run("both_kinds_null_padding", [] {      // every block: 5 point pairs, then 59 null pairs, then 3 line pairs
        Problem p; p.nkf = 2;
        observe(p, false, 5, 2, [](int32_t, int32_t i) { return 1 - i; });          // (list order against keyframe order)
        observe(p, true, 3, 2, [](int32_t, int32_t i) { return i; });
        const Result r = check(p);
        CHECK(r.nulls == 3 * 59 && r.sch.cnt[1] == 67 && r.sch.schur_chunks == 2);
    });
    run("exactly_one_chunk_of_points_no_padding", [] {
        Problem p; p.nkf = 2;
        observe(p, false, 64, 1, [](int32_t, int32_t) { return 0; });               // block (0, 0): 64 point pairs (o, o)
        observe(p, true, 2, 2, [](int32_t, int32_t i) { return i; });
        const Result r = check(p);
        CHECK(r.nulls == 0 && r.sch.cnt[1] == 66 && r.sch.pairs[64].line == 1 && r.sch.schur_chunks == 2);
    });
    run("more_than_one_chunk_of_a_kind", [] {
        Problem p; p.nkf = 2;
        observe(p, false, 70, 1, [](int32_t, int32_t) { return 0; });               // block (0, 0): 70 point pairs, 58 nulls, 65 line pairs
        observe(p, true, 65, 2, [](int32_t, int32_t i) { return i; });
        const Result r = check(p);
        CHECK(r.nulls == 58 && r.sch.cnt[1] == 128 + 65 && r.sch.schur_chunks == 4 && pose_max_chunks(r.csr.kfp) == 3);
    });
    run("fixed_keyframes", [] {              // keyframe -1: in the landmark lists, in no keyframe list, in no pair
        Problem p; p.nkf = 3;
        observe(p, false, 6, 3, [](int32_t j, int32_t i) { return j == 4 ? -1 : (j + i) % 4 - 1; });    // point 4: fixed keyframes only
        observe(p, true, 4, 3, [](int32_t j, int32_t i) { return 2 - (j + i) % 4; });
        const Result r = check(p);
        for (const SchurPair& q : r.sch.pairs)
            CHECK(q.line == 2 || ((q.line ? p.ls_kf : p.pt_kf)[q.o1] >= 0 && (q.line ? p.ls_kf : p.pt_kf)[q.o2] >= 0));
        // fixed: point 4's three observations and (j + i) % 4 == 0 at (0, 0), (2, 2), (3, 1); lines: (j + i) % 4 == 3 at (1, 2), (2, 1), (3, 0)
        CHECK(r.csr.ptp[5] - r.csr.ptp[4] == 3 && r.csr.kfp[3] == (18 - 6) + (12 - 3));
    });
    return n_failed ? 1 : 0;
}
