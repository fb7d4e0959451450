// The pure host planner of the loop-closure check (plslam_amd/csrc/lc_plan.hpp) on the CPU: no device, no HIP header, no library.
// Hand cases whose expectations come from the comments here, from the public header's description of the calls and from a
// literal restatement of the single call's host code as it stood before the planner existed (old_enqueue_verify) -- not from
// the code under test: one "PASS <case>" or "FAIL <case>: <what>" line each, exit status 1 when any failed.
//   g++ -std=c++17 -I plslam_amd/csrc -I include tests/cpp/test_lc_plan.cpp
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <functional>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "lc_plan.hpp"

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

// every field another value, so that a swapped pair of fields shows
plslam_lc_params params(int has_points, int has_lines)
{
    plslam_lc_params p;
    memset(&p, 0, sizeof(p));
    p.cam.fx = 435.25; p.cam.fy = 436.5; p.cam.cx = 367.75; p.cam.cy = 252.125;
    p.homog_th = 1e-7;
    p.min_ratio_12_p = 0.9f; p.min_ratio_12_l = 0.8f;
    p.mutual = 7;                                   // any non-zero value is "true": the problems carry 1
    p.has_points = has_points; p.has_lines = has_lines;
    p.max_iters = 5; p.max_iters_ref = 10;
    p.lc_inlier_ratio = 30.0; p.lc_res = 1.5; p.lc_unc = 0.25; p.lc_inl = 0.375; p.lc_trs = 0.625; p.lc_rot = 35.0;
    return p;
}

// a keyframe with arrays of its own (contents from a seed); a kind without rows has null arrays, as the checks allow
struct Kf {
    std::vector<uint8_t> pdesc, ldesc;
    std::vector<double> P, pl, sPeP, le;
    std::vector<int32_t> pt_idx, ls_idx;
    plslam_lc_keyframe rec;
    Kf(int32_t np, int32_t nl, uint32_t seed, bool with_idx = true)
    {
        uint32_t s = seed * 2654435761u + 12345u;
        auto next = [&s] { s = s * 1664525u + 1013904223u; return s >> 8; };
        pdesc.resize((size_t)np * 32); P.resize((size_t)np * 3); pl.resize((size_t)np * 2); pt_idx.resize((size_t)np);
        ldesc.resize((size_t)nl * 32); sPeP.resize((size_t)nl * 6); le.resize((size_t)nl * 3); ls_idx.resize((size_t)nl);
        for (auto& v : pdesc) v = (uint8_t)next();
        for (auto& v : P) v = (double)next() / 64.0;
        for (auto& v : pl) v = (double)next() / 32.0;
        for (auto& v : pt_idx) v = (int32_t)(next() % 1000) - 1;
        for (auto& v : ldesc) v = (uint8_t)next();
        for (auto& v : sPeP) v = (double)next() / 16.0;
        for (auto& v : le) v = (double)next() / 8.0;
        for (auto& v : ls_idx) v = (int32_t)(next() % 1000) - 1;
        memset(&rec, 0, sizeof(rec));
        rec.n_pt = np; rec.n_ls = nl;
        if (np) { rec.pdesc = pdesc.data(); rec.P = P.data(); rec.pl = pl.data(); rec.pt_idx = with_idx ? pt_idx.data() : nullptr; }
        if (nl) { rec.ldesc = ldesc.data(); rec.sPeP = sPeP.data(); rec.le = le.data(); rec.ls_idx = with_idx ? ls_idx.data() : nullptr; }
    }
    Kf(const Kf&) = delete;
};

// room for the output arrays of a call (the planner only forms addresses inside them)
struct OutRoom {
    std::vector<plslam_lc_result> res;
    std::vector<int32_t> pc, lc;
    std::vector<uint8_t> pi, li;
    OutRoom(size_t B, size_t sp, size_t sl) : res(B), pc(4 * sp + 4), lc(4 * sl + 4), pi(sp + 1), li(sl + 1) {}
    LcOut out() { return {res.data(), pc.data(), pi.data(), lc.data(), li.data()}; }
};

// ---- the single call's host code before the planner, word for word (its Carver spelt out; the launch and the match call left
// out): a comes in with res and the four output fields set, as both callers did
size_t old_take(size_t& off, size_t bytes) { const size_t o = off; off += (bytes + 255) & ~size_t(255); return o; }
struct OldFill { static void args(LcArgs& a, const plslam_lc_params* p)
{
    a.K = GnCam{p->cam.fx, p->cam.fy, p->cam.cx, p->cam.cy};
    a.th = p->homog_th;
    a.has_points = p->has_points ? 1 : 0;
    a.has_lines = p->has_lines ? 1 : 0;
    a.max_iters = p->max_iters;
    a.max_iters_ref = p->max_iters_ref;
    a.lc_inlier_ratio = p->lc_inlier_ratio;
    a.lc_res = p->lc_res;
    a.lc_unc = p->lc_unc;
    a.lc_inl = p->lc_inl;
    a.lc_trs = p->lc_trs;
    a.lc_rot = p->lc_rot;
} };
int old_enqueue_verify(const plslam_lc_params* p, const plslam_lc_keyframe* k0, const plslam_lc_keyframe* k1, char* tb,
                       size_t& tab_bytes, plslam_match_problem pr[2], LcArgs& a)
{
    const bool mp = p->has_points && k0->n_pt > 0 && k1->n_pt > 0;
    const bool ml = p->has_lines && k0->n_ls > 0 && k1->n_ls > 0;
    size_t off = 0;
    const size_t oP = old_take(off, (size_t)k0->n_pt * 4), oL = old_take(off, (size_t)k0->n_ls * 4), oC = old_take(off, 8);
    tab_bytes = off;
    memset(pr, 0, 2 * sizeof(plslam_match_problem));
    int np = 0;
    if (mp) {
        pr[np].d1 = k0->pdesc; pr[np].d2 = k1->pdesc; pr[np].n1 = k0->n_pt; pr[np].n2 = k1->n_pt;
        pr[np].nnr = p->min_ratio_12_p; pr[np].mutual = p->mutual ? 1 : 0;
        pr[np].matches_12 = (int32_t*)(tb + oP); pr[np].n_matches = (int32_t*)(tb + oC);
        ++np;
    }
    if (ml) {
        pr[np].d1 = k0->ldesc; pr[np].d2 = k1->ldesc; pr[np].n1 = k0->n_ls; pr[np].n2 = k1->n_ls;
        pr[np].nnr = p->min_ratio_12_l; pr[np].mutual = p->mutual ? 1 : 0;
        pr[np].matches_12 = (int32_t*)(tb + oL); pr[np].n_matches = (int32_t*)(tb + oC) + 1;
        ++np;
    }
    OldFill::args(a, p);
    a.P = k0->P; a.pl = k1->pl; a.pt_idx0 = k0->pt_idx; a.pt_idx1 = k1->pt_idx;
    a.sPeP = k0->sPeP; a.le = k1->le; a.ls_idx0 = k0->ls_idx; a.ls_idx1 = k1->ls_idx;
    a.m12_p = mp ? (const int32_t*)(tb + oP) : nullptr;
    a.m12_l = ml ? (const int32_t*)(tb + oL) : nullptr;
    a.n_pt0 = k0->n_pt; a.n_pt1 = k1->n_pt; a.n_ls0 = k0->n_ls; a.n_ls1 = k1->n_ls;
    a.identity = 0;
    return np;
}

// every member of the record, one by one
void same_args(const LcArgs& a, const LcArgs& w)
{
    CHECK(a.K.fx == w.K.fx && a.K.fy == w.K.fy && a.K.cx == w.K.cx && a.K.cy == w.K.cy && a.th == w.th);
    CHECK(a.P == w.P && a.pl == w.pl && a.pt_idx0 == w.pt_idx0 && a.pt_idx1 == w.pt_idx1);
    CHECK(a.sPeP == w.sPeP && a.le == w.le && a.ls_idx0 == w.ls_idx0 && a.ls_idx1 == w.ls_idx1);
    CHECK(a.m12_p == w.m12_p && a.m12_l == w.m12_l);
    CHECK(a.n_pt0 == w.n_pt0 && a.n_pt1 == w.n_pt1 && a.n_ls0 == w.n_ls0 && a.n_ls1 == w.n_ls1 && a.identity == w.identity);
    CHECK(a.has_points == w.has_points && a.has_lines == w.has_lines && a.max_iters == w.max_iters && a.max_iters_ref == w.max_iters_ref);
    CHECK(a.lc_inlier_ratio == w.lc_inlier_ratio && a.lc_res == w.lc_res && a.lc_unc == w.lc_unc && a.lc_inl == w.lc_inl);
    CHECK(a.lc_trs == w.lc_trs && a.lc_rot == w.lc_rot);
    CHECK(a.pt_corr == w.pt_corr && a.pt_inl == w.pt_inl && a.ls_corr == w.ls_corr && a.ls_inl == w.ls_inl && a.res == w.res);
}

// B = 1: the planner against the restatement -- the table block's size, the problems (all but the counter slot, which is the
// problem's position in the list) and every field of the record.  Returns the number of problems.
int single_is_old(int has_points, int has_lines, int32_t np0, int32_t nl0, int32_t np1, int32_t nl1)
{
    const plslam_lc_params p = params(has_points, has_lines);
    Kf k0(np0, nl0, 1), k1(np1, nl1, 2);
    OutRoom room(1, (size_t)np0, (size_t)nl0);
    LcArgs want;
    memset(&want, 0, sizeof(want));
    want.res = room.res.data();
    want.pt_corr = room.pc.data(); want.pt_inl = room.pi.data(); want.ls_corr = room.lc.data(); want.ls_inl = room.li.data();
    size_t want_bytes = 0;
    plslam_match_problem want_pr[2], pr[2];
    std::vector<char> tab(align256((size_t)np0 * 4) + align256((size_t)nl0 * 4) + 256);
    const int want_n = old_enqueue_verify(&p, &k0.rec, &k1.rec, tab.data(), want_bytes, want_pr, want);

    const LcTables T = lc_tables(&k0.rec, 1);
    CHECK(T.bytes == want_bytes && T.bytes == tab.size());
    LcArgs a;
    const int32_t n = lc_plan_pairs(&p, &k0.rec, &k1.rec, 1, T, tab.data(), room.out(), pr, &a);
    CHECK(n == want_n);
    for (int k = 0; k < n && k < want_n; ++k) {
        CHECK(pr[k].d1 == want_pr[k].d1 && pr[k].d2 == want_pr[k].d2 && pr[k].n1 == want_pr[k].n1 && pr[k].n2 == want_pr[k].n2);
        CHECK(pr[k].nnr == want_pr[k].nnr && pr[k].mutual == want_pr[k].mutual && pr[k].mutual == 1);
        CHECK(pr[k].matches_12 == want_pr[k].matches_12 && pr[k].keep_prior == 0 && pr[k].reserved == 0);
        CHECK(pr[k].n_matches == (int32_t*)(tab.data() + T.oC) + k);
    }
    same_args(a, want);
    return n;
}

// the bytes [o, o + n) of every array of the laid-out records, for the overlap check
struct Span { size_t o, n; };

void hand_cases()
{
    // ---- 1. the single call is the planner with B = 1
    run("b1_points_and_lines", [] { CHECK(single_is_old(1, 1, 300, 41, 257, 3) == 2); });
    run("b1_points_only", [] { CHECK(single_is_old(1, 0, 300, 41, 257, 3) == 1); });
    run("b1_lines_only", [] { CHECK(single_is_old(0, 1, 300, 41, 257, 3) == 1); });
    run("b1_has_points_0_with_points_present", [] { CHECK(single_is_old(0, 0, 64, 64, 64, 64) == 0); });
    run("b1_n_pt1_zero", [] { CHECK(single_is_old(1, 1, 300, 41, 0, 3) == 1); });

    // ---- 2. three pairs with ragged counts.  Pair 0: 5 x 4 points, 2 x 0 lines (lines not matched); pair 1: no kf0 point (points
    // not matched), 7 x 1 lines; pair 2: 300 x 3 points, no kf0 line.  Rows: points 0, 5, 5; lines 0, 2, 9.
    run("b3_ragged_counts", [] {
        const plslam_lc_params p = params(1, 1);
        Kf a0(5, 2, 1), a1(0, 7, 2), a2(300, 0, 3), b0(4, 0, 4), b1(6, 1, 5), b2(3, 9, 6);
        const plslam_lc_keyframe kf0[3] = {a0.rec, a1.rec, a2.rec}, kf1[3] = {b0.rec, b1.rec, b2.rec};
        const LcTables T = lc_tables(kf0, 3);
        CHECK(T.oP == 0 && T.oL == 1280 && T.oC == 1280 + 256 && T.bytes == 1280 + 256 + 256);      // 305 x 4 -> 1280; 9 x 4; 3 x 8
        std::vector<char> tab(T.bytes);
        OutRoom room(3, 305, 9);
        plslam_match_problem pr[6];
        LcArgs a[3];
        CHECK(lc_plan_pairs(&p, kf0, kf1, 3, T, tab.data(), room.out(), pr, a) == 3);
        int32_t *mP = (int32_t*)tab.data(), *mL = (int32_t*)(tab.data() + T.oL), *cnt = (int32_t*)(tab.data() + T.oC);
        CHECK(pr[0].d1 == a0.rec.pdesc && pr[0].d2 == b0.rec.pdesc && pr[0].n1 == 5 && pr[0].n2 == 4 && pr[0].matches_12 == mP);
        CHECK(pr[1].d1 == a1.rec.ldesc && pr[1].d2 == b1.rec.ldesc && pr[1].n1 == 7 && pr[1].n2 == 1 && pr[1].matches_12 == mL + 2);
        CHECK(pr[2].d1 == a2.rec.pdesc && pr[2].d2 == b2.rec.pdesc && pr[2].n1 == 300 && pr[2].n2 == 3 && pr[2].matches_12 == mP + 5);
        CHECK(pr[0].nnr == 0.9f && pr[1].nnr == 0.8f && pr[2].nnr == 0.9f);
        CHECK(pr[0].n_matches == cnt && pr[1].n_matches == cnt + 1 && pr[2].n_matches == cnt + 2);     // each its own
        const size_t rp[3] = {0, 5, 5}, rl[3] = {0, 2, 9};
        for (int b = 0; b < 3; ++b) {
            CHECK(a[b].res == room.res.data() + b && a[b].identity == 0);
            CHECK(a[b].pt_corr == room.pc.data() + 4 * rp[b] && a[b].pt_inl == room.pi.data() + rp[b]);
            CHECK(a[b].ls_corr == room.lc.data() + 4 * rl[b] && a[b].ls_inl == room.li.data() + rl[b]);
            CHECK(a[b].n_pt0 == kf0[b].n_pt && a[b].n_pt1 == kf1[b].n_pt && a[b].n_ls0 == kf0[b].n_ls && a[b].n_ls1 == kf1[b].n_ls);
            CHECK(a[b].P == kf0[b].P && a[b].pl == kf1[b].pl && a[b].sPeP == kf0[b].sPeP && a[b].le == kf1[b].le);
            CHECK(a[b].pt_idx0 == kf0[b].pt_idx && a[b].pt_idx1 == kf1[b].pt_idx && a[b].ls_idx0 == kf0[b].ls_idx && a[b].ls_idx1 == kf1[b].ls_idx);
        }
        CHECK(a[0].m12_p == mP && a[0].m12_l == nullptr);
        CHECK(a[1].m12_p == nullptr && a[1].m12_l == mL + 2);
        CHECK(a[2].m12_p == mP + 5 && a[2].m12_l == nullptr);
    });

    // ---- 3. null output bases give null fields, in every pair
    run("null_output_bases_give_null_fields", [] {
        const plslam_lc_params p = params(1, 1);
        Kf a0(5, 2, 1), a1(9, 7, 2), b0(4, 3, 4);
        const plslam_lc_keyframe kf0[2] = {a0.rec, a1.rec}, kf1[2] = {b0.rec, b0.rec};
        const LcTables T = lc_tables(kf0, 2);
        std::vector<char> tab(T.bytes);
        OutRoom room(2, 14, 9);
        plslam_match_problem pr[4];
        LcArgs a[2];
        CHECK(lc_plan_pairs(&p, kf0, kf1, 2, T, tab.data(), LcOut{room.res.data(), nullptr, nullptr, nullptr, nullptr}, pr, a) == 4);
        for (int b = 0; b < 2; ++b)
            CHECK(a[b].res == room.res.data() + b && !a[b].pt_corr && !a[b].pt_inl && !a[b].ls_corr && !a[b].ls_inl && a[b].m12_p && a[b].m12_l);
        // one at a time
        CHECK(lc_plan_pairs(&p, kf0, kf1, 2, T, tab.data(), LcOut{room.res.data(), nullptr, room.pi.data(), room.lc.data(), nullptr}, pr, a) == 4);
        CHECK(!a[1].pt_corr && a[1].pt_inl == room.pi.data() + 5 && a[1].ls_corr == room.lc.data() + 4 * 2 && !a[1].ls_inl);
    });

    // ---- 4. the keyframe image
    run("kf_image_of_eight_pairs_sharing_kf1", [] {
        // kf0: eight records of their own -- one without any feature, one without landmark indices, one whose record differs from
        // another's in pdesc alone (an equal copy of the descriptors elsewhere); kf1: one record eight times
        std::vector<std::unique_ptr<Kf>> own;
        const int32_t np[8] = {5, 0, 300, 1, 64, 5, 17, 8}, nl[8] = {2, 0, 0, 9, 64, 2, 3, 1};
        plslam_lc_keyframe kf0[8], kf1[8];
        for (int b = 0; b < 8; ++b) {
            own.emplace_back(new Kf(np[b], nl[b], 10 + (uint32_t)b, b != 3));
            kf0[b] = own.back()->rec;
        }
        std::vector<uint8_t> pdesc_copy(own[0]->pdesc);
        kf0[5] = kf0[0];
        kf0[5].pdesc = pdesc_copy.data();
        Kf shared(40, 6, 99);
        for (int b = 0; b < 8; ++b) kf1[b] = shared.rec;
        LcKfImage L;
        lc_kf_layout(kf0, kf1, 8, L);
        CHECK(L.first.size() == 16 && L.off.size() == 16 * 8);
        for (size_t q = 0; q < 16 && q < L.first.size(); ++q) CHECK(L.first[q] == (q <= 8 ? q : 8));     // kf1 once; kf0[5] on its own
        // aligned, inside the block, no two arrays of the laid-out records overlap
        std::vector<Span> spans;
        for (size_t q = 0; q <= 8; ++q) {
            const plslam_lc_keyframe& k = q < 8 ? kf0[q] : kf1[0];
            const size_t rows[8] = {(size_t)k.n_pt, (size_t)k.n_pt, (size_t)k.n_pt, (size_t)k.n_pt, (size_t)k.n_ls, (size_t)k.n_ls, (size_t)k.n_ls, (size_t)k.n_ls};
            const size_t stride[8] = {32, 24, 16, 4, 32, 48, 24, 4};          // pdesc, P, pl, pt_idx, ldesc, sPeP, le, ls_idx
            for (int i = 0; i < 8; ++i) {
                const size_t o = L.off[q * 8 + i];
                CHECK(o % 256 == 0 && o + rows[i] * stride[i] <= L.bytes);
                if (rows[i]) spans.push_back({o, rows[i] * stride[i]});
            }
        }
        std::sort(spans.begin(), spans.end(), [](const Span& x, const Span& y) { return x.o < y.o; });
        for (size_t i = 1; i < spans.size(); ++i) CHECK(spans[i - 1].o + spans[i - 1].n <= spans[i].o);
        // the filled block holds the inputs byte for byte; what nothing is copied to keeps the sentinel
        std::vector<char> h(L.bytes, (char)0xA5);
        lc_kf_fill(kf0, kf1, L, h.data());
        size_t copied = 0;
        for (size_t q = 0; q <= 8; ++q) {
            const plslam_lc_keyframe& k = q < 8 ? kf0[q] : kf1[0];
            const size_t n = (size_t)k.n_pt, m = (size_t)k.n_ls;
            const size_t* o = &L.off[q * 8];
            if (n) {
                CHECK(!memcmp(&h[o[0]], k.pdesc, n * 32) && !memcmp(&h[o[1]], k.P, n * 24) && !memcmp(&h[o[2]], k.pl, n * 16));
                copied += n * 72;
                if (k.pt_idx) { CHECK(!memcmp(&h[o[3]], k.pt_idx, n * 4)); copied += n * 4; }
            }
            if (m) {
                CHECK(!memcmp(&h[o[4]], k.ldesc, m * 32) && !memcmp(&h[o[5]], k.sPeP, m * 48) && !memcmp(&h[o[6]], k.le, m * 24));
                copied += m * 104;
                if (k.ls_idx) { CHECK(!memcmp(&h[o[7]], k.ls_idx, m * 4)); copied += m * 4; }
            }
        }
        // record 3 has no indices: its two index areas (1 x 4 and 9 x 4 bytes) are untouched
        CHECK(h[L.off[3 * 8 + 3]] == (char)0xA5 && h[L.off[3 * 8 + 7]] == (char)0xA5 && h[L.off[3 * 8 + 7] + 35] == (char)0xA5);
        size_t touched = 0;
        std::vector<char> h2(L.bytes, (char)0x5A);
        lc_kf_fill(kf0, kf1, L, h2.data());
        for (size_t i = 0; i < L.bytes; ++i) touched += h[i] == h2[i];          // a byte both fills agree on was written
        CHECK(touched == copied);
        // the device records over a copy at d
        std::vector<char> dev(L.bytes);
        char* d = dev.data();
        plslam_lc_keyframe D[16];
        lc_kf_device(kf0, kf1, L, d, D);
        for (size_t q = 0; q < 16; ++q) {
            const plslam_lc_keyframe& k = q < 8 ? kf0[q] : kf1[q - 8];
            const size_t* o = &L.off[L.first[q] * 8];
            CHECK(D[q].n_pt == k.n_pt && D[q].n_ls == k.n_ls);
            CHECK((const char*)D[q].pdesc == d + o[0] && (const char*)D[q].P == d + o[1] && (const char*)D[q].pl == d + o[2]);
            CHECK((const char*)D[q].ldesc == d + o[4] && (const char*)D[q].sPeP == d + o[5] && (const char*)D[q].le == d + o[6]);
            CHECK(k.pt_idx ? (const char*)D[q].pt_idx == d + o[3] : D[q].pt_idx == nullptr);
            CHECK(k.ls_idx ? (const char*)D[q].ls_idx == d + o[7] : D[q].ls_idx == nullptr);
        }
        CHECK(D[3].pt_idx == nullptr && D[3].ls_idx == nullptr && D[1].pt_idx == nullptr);      // no indices; no feature at all
        CHECK(!memcmp(&D[9], &D[8], sizeof(D[8])) && !memcmp(&D[15], &D[8], sizeof(D[8])));
    });
    run("kf_image_same_record_twice_is_laid_out_once", [] {
        // the single host call with kf0 == kf1: n = 2 records, one image
        Kf k(257, 3, 5);
        LcKfImage L, one;
        lc_kf_layout(&k.rec, &k.rec, 1, L);
        CHECK(L.first.size() == 2 && L.first[0] == 0 && L.first[1] == 0);
        CHECK(L.bytes == align256(257 * 32) + align256(257 * 24) + align256(257 * 16) + align256(257 * 4) + 4 * 256);
        Kf other(257, 3, 5);                       // equal contents in other arrays: a record of its own
        lc_kf_layout(&k.rec, &other.rec, 1, one);
        CHECK(one.first[1] == 1 && one.bytes == 2 * L.bytes);
        std::vector<char> dev(L.bytes);
        plslam_lc_keyframe D[2];
        lc_kf_device(&k.rec, &k.rec, L, dev.data(), D);
        CHECK(!memcmp(&D[0], &D[1], sizeof(D[0])) && (const char*)D[1].le == dev.data() + L.off[6]);
    });
    run("kf_image_of_records_without_features", [] {
        Kf e0(0, 0, 1), e1(0, 0, 2), pts(3, 0, 3);
        LcKfImage L;
        lc_kf_layout(&e0.rec, &e1.rec, 1, L);      // two all-null records are equal: one (empty) layout
        CHECK(L.bytes == 0 && L.first[1] == 0);
        lc_kf_fill(&e0.rec, &e1.rec, L, nullptr);  // nothing to copy: h is not touched
        plslam_lc_keyframe D[2];
        lc_kf_device(&e0.rec, &e1.rec, L, nullptr, D);
        CHECK(D[0].n_pt == 0 && D[0].n_ls == 0 && D[0].pt_idx == nullptr && D[0].ls_idx == nullptr);
        lc_kf_layout(&e0.rec, &pts.rec, 1, L);
        CHECK(L.first[1] == 1 && L.bytes == 4 * 256 && L.off[8 + 4] == L.bytes && L.off[8 + 7] == L.bytes);
        std::vector<char> h(L.bytes, (char)0xA5);
        lc_kf_fill(&e0.rec, &pts.rec, L, h.data());
        CHECK(!memcmp(&h[L.off[8 + 1]], pts.rec.P, 72) && h[L.off[8 + 1] + 72] == (char)0xA5);
    });

    // ---- 5. the output block.  Three pairs with capacities 5, 0, 7 points and 2, 3, 0 lines; K25 reported 3, 0, 7 common
    // points and 0, 3, 0 common lines
    run("out_block_scatter_copies_the_common_rows_only", [] {
        plslam_lc_keyframe kf0[3];
        memset(kf0, 0, sizeof(kf0));
        const int32_t cp[3] = {5, 0, 7}, cl[3] = {2, 3, 0}, ncp[3] = {3, 0, 7}, ncl[3] = {0, 3, 0};
        for (int b = 0; b < 3; ++b) { kf0[b].n_pt = cp[b]; kf0[b].n_ls = cl[b]; }
        const LcOutBlock L = lc_out_block(kf0, 3);
        const size_t R = align256(3 * sizeof(plslam_lc_result));
        CHECK(L.oR == 0 && L.oPC == R && L.oPI == R + 256 && L.oLC == R + 512 && L.oLI == R + 768 && L.bytes == R + 1024);
        std::vector<char> ho(L.bytes);
        for (size_t i = 0; i < ho.size(); ++i) ho[i] = (char)(i * 7 + 1);
        plslam_lc_result* hr = (plslam_lc_result*)ho.data();
        for (int b = 0; b < 3; ++b) { hr[b].common_pt = ncp[b]; hr[b].common_ls = ncl[b]; }
        const LcOut bases = lc_out_bases(L, ho.data());
        CHECK((char*)bases.res == ho.data() && (char*)bases.pt_corr == ho.data() + L.oPC && (char*)bases.pt_inl == ho.data() + L.oPI);
        CHECK((char*)bases.ls_corr == ho.data() + L.oLC && (char*)bases.ls_inl == ho.data() + L.oLI);
        plslam_lc_result res[3];
        std::vector<int32_t> pc(4 * 12, -77), lc(4 * 5, -77);
        std::vector<uint8_t> pi(12, 0xEE), li(5, 0xEE);
        lc_out_scatter(L, ho.data(), kf0, 3, res, pc.data(), pi.data(), lc.data(), li.data());
        CHECK(!memcmp(res, ho.data(), sizeof(res)));
        const int32_t* bpc = (const int32_t*)(ho.data() + L.oPC);
        const int32_t* blc = (const int32_t*)(ho.data() + L.oLC);
        const uint8_t* bpi = (const uint8_t*)(ho.data() + L.oPI);
        const uint8_t* bli = (const uint8_t*)(ho.data() + L.oLI);
        size_t rp = 0, rl = 0;
        std::vector<int> pt_row_written(12, 0), ls_row_written(5, 0);
        for (int b = 0; b < 3; ++b) {
            for (int k = 0; k < ncp[b]; ++k) pt_row_written[rp + (size_t)k] = 1;
            for (int k = 0; k < ncl[b]; ++k) ls_row_written[rl + (size_t)k] = 1;
            rp += (size_t)cp[b]; rl += (size_t)cl[b];
        }
        for (size_t r = 0; r < 12; ++r) {
            for (int c = 0; c < 4; ++c) CHECK(pc[4 * r + c] == (pt_row_written[r] ? bpc[4 * r + c] : -77));
            CHECK(pi[r] == (pt_row_written[r] ? bpi[r] : 0xEE));
        }
        for (size_t r = 0; r < 5; ++r) {
            for (int c = 0; c < 4; ++c) CHECK(lc[4 * r + c] == (ls_row_written[r] ? blc[4 * r + c] : -77));
            CHECK(li[r] == (ls_row_written[r] ? bli[r] : 0xEE));
        }
        CHECK(pt_row_written[3] == 0 && pt_row_written[5] == 1 && ls_row_written[0] == 0 && ls_row_written[2] == 1);
    });
    run("out_block_scatter_skips_null_arrays", [] {
        // the relative-pose call's use: one problem, masks and no correspondence rows; then no optional array at all
        plslam_lc_keyframe rows;
        memset(&rows, 0, sizeof(rows));
        rows.n_pt = 6; rows.n_ls = 4;
        const LcOutBlock L = lc_out_block(&rows, 1);
        std::vector<char> ho(L.bytes);
        for (size_t i = 0; i < ho.size(); ++i) ho[i] = (char)(i * 5 + 3);
        ((plslam_lc_result*)ho.data())->common_pt = 6;
        ((plslam_lc_result*)ho.data())->common_ls = 4;
        plslam_lc_result res;
        std::vector<uint8_t> pi(7, 0xEE), li(5, 0xEE);
        lc_out_scatter(L, ho.data(), &rows, 1, &res, nullptr, pi.data(), nullptr, li.data());
        CHECK(!memcmp(&res, ho.data(), sizeof(res)) && !memcmp(pi.data(), ho.data() + L.oPI, 6) && pi[6] == 0xEE);
        CHECK(!memcmp(li.data(), ho.data() + L.oLI, 4) && li[4] == 0xEE);
        memset(&res, 0, sizeof(res));
        lc_out_scatter(L, ho.data(), &rows, 1, &res, nullptr, nullptr, nullptr, nullptr);
        CHECK(!memcmp(&res, ho.data(), sizeof(res)));
    });

    // ---- 6. the checks: every rule and its code
    run("check_params_refusals", [] {
        plslam_lc_params p = params(1, 1);
        CHECK(lc_check_params(&p) == PLSLAM_OK);
        CHECK(lc_check_params(nullptr) == PLSLAM_EINVAL);
        p.max_iters = -1; CHECK(lc_check_params(&p) == PLSLAM_EINVAL);
        p.max_iters = PLSLAM_LC_MAX_ITERS + 1; CHECK(lc_check_params(&p) == PLSLAM_EINVAL);
        p.max_iters = PLSLAM_LC_MAX_ITERS; CHECK(lc_check_params(&p) == PLSLAM_OK);
        p.max_iters_ref = -1; CHECK(lc_check_params(&p) == PLSLAM_EINVAL);
        p.max_iters_ref = PLSLAM_LC_MAX_ITERS + 1; CHECK(lc_check_params(&p) == PLSLAM_EINVAL);
        p.max_iters_ref = 0; p.max_iters = 0; CHECK(lc_check_params(&p) == PLSLAM_OK);
    });
    run("check_kf_refusals", [] {
        Kf k(4, 3, 1);
        auto code = [](plslam_lc_keyframe r) { return lc_check_kf(&r); };
        auto with = [&k](const std::function<void(plslam_lc_keyframe&)>& spoil) { plslam_lc_keyframe r = k.rec; spoil(r); return r; };
        CHECK(code(k.rec) == PLSLAM_OK);
        CHECK(lc_check_kf(nullptr) == PLSLAM_EINVAL);
        CHECK(code(with([](plslam_lc_keyframe& r) { r.n_pt = -1; })) == PLSLAM_EINVAL);
        CHECK(code(with([](plslam_lc_keyframe& r) { r.n_ls = -1; })) == PLSLAM_EINVAL);
        CHECK(code(with([](plslam_lc_keyframe& r) { r.pdesc = nullptr; })) == PLSLAM_EINVAL);
        CHECK(code(with([](plslam_lc_keyframe& r) { r.P = nullptr; })) == PLSLAM_EINVAL);
        CHECK(code(with([](plslam_lc_keyframe& r) { r.pl = nullptr; })) == PLSLAM_EINVAL);
        CHECK(code(with([](plslam_lc_keyframe& r) { r.ldesc = nullptr; })) == PLSLAM_EINVAL);
        CHECK(code(with([](plslam_lc_keyframe& r) { r.sPeP = nullptr; })) == PLSLAM_EINVAL);
        CHECK(code(with([](plslam_lc_keyframe& r) { r.le = nullptr; })) == PLSLAM_EINVAL);
        CHECK(code(with([](plslam_lc_keyframe& r) { r.pt_idx = nullptr; r.ls_idx = nullptr; })) == PLSLAM_OK);      // optional
        CHECK(code(with([](plslam_lc_keyframe& r) { r.n_pt = PLSLAM_LC_MAX_FEATURES; r.n_ls = PLSLAM_LC_MAX_FEATURES; })) == PLSLAM_OK);
        CHECK(code(with([](plslam_lc_keyframe& r) { r.n_pt = PLSLAM_LC_MAX_FEATURES + 1; })) == PLSLAM_ERANGE);
        CHECK(code(with([](plslam_lc_keyframe& r) { r.n_ls = PLSLAM_LC_MAX_FEATURES + 1; })) == PLSLAM_ERANGE);
        // the codes in the order of the rules: a missing array is reported before the range
        CHECK(code(with([](plslam_lc_keyframe& r) { r.n_pt = PLSLAM_LC_MAX_FEATURES + 1; r.P = nullptr; })) == PLSLAM_EINVAL);
        plslam_lc_keyframe none;
        memset(&none, 0, sizeof(none));
        CHECK(code(none) == PLSLAM_OK);                                             // no feature: no array needed
    });
    run("check_batch_refusals", [] {
        Kf k(4, 3, 1);
        plslam_lc_keyframe kf[3] = {k.rec, k.rec, k.rec}, bad[3] = {k.rec, k.rec, k.rec};
        const int32_t max_pairs = 3;
        CHECK(lc_check_batch(&max_pairs, kf, kf, 3) == PLSLAM_OK);
        CHECK(lc_check_batch(nullptr, kf, kf, 1) == PLSLAM_EINVAL);           // no batch object
        CHECK(lc_check_batch(&max_pairs, kf, kf, -1) == PLSLAM_EINVAL);
        CHECK(lc_check_batch(&max_pairs, kf, kf, max_pairs + 1) == PLSLAM_EINVAL);
        CHECK(lc_check_batch(&max_pairs, nullptr, nullptr, 0) == PLSLAM_OK);  // B = 0 needs no record
        CHECK(lc_check_batch(&max_pairs, nullptr, kf, 1) == PLSLAM_EINVAL);
        CHECK(lc_check_batch(&max_pairs, kf, nullptr, 1) == PLSLAM_EINVAL);
        bad[2].n_ls = PLSLAM_LC_MAX_FEATURES + 1;
        CHECK(lc_check_batch(&max_pairs, bad, kf, 3) == PLSLAM_ERANGE);
        CHECK(lc_check_batch(&max_pairs, kf, bad, 3) == PLSLAM_ERANGE);
        CHECK(lc_check_batch(&max_pairs, kf, bad, 2) == PLSLAM_OK);           // only the B records of the call are looked at
        bad[2] = k.rec; bad[1].le = nullptr;
        CHECK(lc_check_batch(&max_pairs, kf, bad, 3) == PLSLAM_EINVAL);
    });

    // ---- 7. the identity record: the single call gives counts and every output, the batched call counts of 0 (the device has
    // them) and no rows; given the same arguments both get the same record, and the batch changes res alone
    run("identity_record_of_the_two_relpose_forms", [] {
        const plslam_lc_params p = params(0, 0);
        Kf k(6, 4, 1);
        OutRoom room(3, 6, 4);
        LcArgs one, tab[3], base;
        lc_identity_args(one, &p, k.rec.P, k.rec.pl, 6, k.rec.sPeP, k.rec.le, 4, room.out());
        CHECK(one.identity == 1 && one.n_pt0 == 6 && one.n_pt1 == 6 && one.n_ls0 == 4 && one.n_ls1 == 4);
        CHECK(one.P == k.rec.P && one.pl == k.rec.pl && one.sPeP == k.rec.sPeP && one.le == k.rec.le);
        CHECK(!one.m12_p && !one.m12_l && !one.pt_idx0 && !one.pt_idx1 && !one.ls_idx0 && !one.ls_idx1);
        CHECK(one.res == room.res.data() && one.pt_corr == room.pc.data() && one.pt_inl == room.pi.data());
        CHECK(one.ls_corr == room.lc.data() && one.ls_inl == room.li.data());
        LcArgs filled;
        memset(&filled, 0, sizeof(filled));
        OldFill::args(filled, &p);
        CHECK(one.K.fx == filled.K.fx && one.K.cy == filled.K.cy && one.th == filled.th && one.max_iters == 5 && one.max_iters_ref == 10);
        CHECK(one.has_points == 0 && one.has_lines == 0 && one.lc_res == 1.5 && one.lc_unc == 0.25 && one.lc_trs == 0.625 && one.lc_rot == 35.0);
        // the batched form: the same filler, then res per record
        lc_identity_args(base, &p, k.rec.P, k.rec.pl, 6, k.rec.sPeP, k.rec.le, 4, room.out());
        for (int b = 0; b < 3; ++b) { tab[b] = base; tab[b].res = room.res.data() + b; }
        for (int b = 0; b < 3; ++b) {
            LcArgs w = tab[b];
            CHECK(w.res == room.res.data() + b);
            w.res = one.res;
            CHECK(!memcmp(&w, &one, sizeof(LcArgs)));
        }
        // as plslam_relpose_robust_gn_batched_dev calls it
        lc_identity_args(base, &p, k.rec.P, k.rec.pl, 0, nullptr, nullptr, 0, LcOut{nullptr, nullptr, room.pi.data(), nullptr, nullptr});
        CHECK(base.identity == 1 && base.n_pt0 == 0 && base.n_ls1 == 0 && !base.pt_corr && !base.ls_corr && !base.sPeP && !base.ls_inl);
        CHECK(base.pt_inl == room.pi.data() && base.P == k.rec.P && base.res == nullptr);
    });
}

}  // namespace

int main()
{
    hand_cases();
    return n_failed ? 1 : 0;
}
