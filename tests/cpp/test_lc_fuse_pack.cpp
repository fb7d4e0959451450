// The pure host half of plslam_lc_fuse_run (plslam_amd/csrc/lc_fuse_plan.hpp): validation, the growth bounds, the packing of
// the staged block on heap arrays of exactly the documented sizes, and the layout of the handle's device buffer at the tile's
// edges.  A stand-alone program: tests/test_lc_fuse_cpu.py builds it with -fsanitize=address,undefined and runs it; it prints
// "lc_fuse_layout: ok" and "lc_fuse_pack: ok" and returns 0, or says which check failed.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "lc_fuse_plan.hpp"

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
    std::vector<char> mem;
    plslam_map_index ix;
    explicit Image(int32_t nk, int32_t n_pt, int32_t n_ls, int32_t obs_pt, int32_t obs_ls) : mem(64)
    {
        char* p = mem.data();
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

struct Kind {                            // exactly m rows of everything, n_lc + 1 offsets
    std::vector<int32_t> tup, eptr;
    std::vector<double> P0, o0, P1, o1;
    plslam_lc_fuse_kind k;
    Kind(const std::vector<std::vector<int32_t>>& per_entry, int dl, int dv)
    {
        eptr.push_back(0);
        for (const auto& e : per_entry) {
            tup.insert(tup.end(), e.begin(), e.end());
            eptr.push_back((int32_t)(tup.size() / 4));
        }
        const size_t m = tup.size() / 4;
        for (size_t i = 0; i < m * dl; ++i) { P0.push_back(1.0 + i); P1.push_back(-1.0 - i); }
        for (size_t i = 0; i < m * dv; ++i) { o0.push_back(0.5 + i); o1.push_back(-0.5 - i); }
        k = plslam_lc_fuse_kind{tup.data(), eptr.data(), P0.data(), o0.data(), P1.data(), o1.data()};
    }
};

size_t pad(size_t b) { return (b + 255) & ~(size_t)255; }

// What every device layout must satisfy.  The pieces in the order they are carved, with the bytes each holds:
// [zeroed: counters, graph, per kind feat_win / part] [0x7f: head] [0xff: killer] [staged] [the rest, per kind]
int device_layout_ok(const LcFusePlan& P, const plslam_map_index& src, const plslam_map_insert_dst& dst)
{
    const plslam_map_landmarks* S[2] = {&src.points, &src.lines};
    const int32_t obs_cap[2] = {dst.pt_obs_cap, dst.ls_obs_cap};
    struct Piece { size_t off, bytes; int region; };         // region: 0 zeroed, 1 0x7f, 2 0xff, 3 staged, 4 the rest
    std::vector<Piece> v = {{P.d_cnt, 80, 0}, {P.d_graph, (size_t)P.nk * P.nk * 4, 0}};
    for (int k = 0; k < 2; ++k) {
        v.push_back({P.k[k].d_win, (size_t)S[k]->n_feat * 4 + 4, 0});
        v.push_back({P.k[k].d_part, (size_t)P.k[k].w_lm * 4, 0});
    }
    for (int k = 0; k < 2; ++k) v.push_back({P.k[k].d_head, (size_t)S[k]->n * 4 + 4, 1});
    for (int k = 0; k < 2; ++k) v.push_back({P.k[k].d_killer, (size_t)S[k]->n * 4 + 4, 2});
    v.push_back({P.stage_off, P.stage_bytes, 3});
    for (int k = 0; k < 2; ++k) {
        const LcFuseKindPlan& K = P.k[k];
        const size_t m = (size_t)K.m;
        v.push_back({K.d_len, (size_t)K.need_lm * 4 + 4, 4});
        v.push_back({K.d_sc, m * 4 + 4, 4});
        v.push_back({K.d_fw0, m * 4 + 4, 4});
        v.push_back({K.d_fw1, m * 4 + 4, 4});
        v.push_back({K.d_ev, m * 24 + 24, 4});
        v.push_back({K.d_off, m * 4 + 4, 4});
        v.push_back({K.d_pair, m * 4 + 8, 4});
        v.push_back({K.d_nev, (size_t)K.cC * 4 + 4, 4});
        v.push_back({K.d_dir, m * 48 + 48, 4});
        v.push_back({K.d_osrc, (size_t)obs_cap[k] * 4 + 4, 4});
    }
    // carved in this order, aligned as the carver aligns: each starts where the one before it ended, padded to 256
    size_t end = 0;
    for (const Piece& p : v) {
        CHECK(p.off % 256 == 0 && p.off == end);
        end = p.off + pad(p.bytes);
    }
    CHECK(P.total == end);                                    // the total is the last slice's end
    // no two overlap: sorted by offset, each ends at or before the next one starts
    std::vector<Piece> w = v;
    std::sort(w.begin(), w.end(), [](const Piece& a, const Piece& b) { return a.off < b.off; });
    for (size_t i = 0; i + 1 < w.size(); ++i) CHECK(w[i].off + w[i].bytes <= w[i + 1].off);
    // the three fill regions and the staged block: contiguous, in that order, and each holds exactly its pieces
    CHECK(P.fill[0].off == 0 && P.fill[0].byte == 0 && P.fill[1].byte == 0x7f && P.fill[2].byte == 0xff);
    CHECK(P.fill[1].off == P.fill[0].bytes && P.fill[2].off == P.fill[1].off + P.fill[1].bytes);
    CHECK(P.stage_off == P.fill[2].off + P.fill[2].bytes);
    const size_t lo[4] = {0, P.fill[1].off, P.fill[2].off, P.stage_off};
    const size_t hi[4] = {P.fill[1].off, P.fill[2].off, P.stage_off, P.stage_off + pad(P.stage_bytes)};
    for (const Piece& p : v)
        for (int r = 0; r < 4; ++r) CHECK((p.region == r) == (p.off >= lo[r] && p.off + p.bytes <= hi[r] && p.off < hi[r]));
    // page-locked: 20 counter words, nk^2 more where the caller takes the graph
    CHECK(P.res_bytes(false) == 256 && P.res_bytes(true) == pad((20 + (size_t)P.nk * P.nk) * 4));
    return 0;
}

// the layout of a call on `n` point landmarks with `n_feat` features and `m` point tuples, `c` of them (-1, -1): one flagged entry
int layout_case(int32_t n, int32_t n_feat, int32_t m, int32_t c)
{
    const int32_t nk = 7;
    Image src(nk, n, 40, n ? 300 : 0, 90), dsti(nk, 0, 0, 0, 0);
    src.ix.points.n_feat = n_feat;
    plslam_map_insert_dst dst{dsti.ix, 1000, 2000, 100, 200};
    std::vector<int32_t> lc = {1, 5, 1}, tup;
    std::vector<double> T((size_t)nk * 16, 1.0);
    for (int32_t i = 0; i < m; ++i) {
        const int32_t t[4] = {i < c ? -1 : 0, i, i < c ? -1 : 1, i};
        tup.insert(tup.end(), t, t + 4);
    }
    Kind pts({tup}, 3, 2), lns({{-1, 1, -1, 2}}, 6, 3);
    LcFusePlan P;
    CHECK(lc_fuse_plan(&src.ix, &dst, 1, lc.data(), T.data(), &pts.k, &lns.k, &P) == PLSLAM_OK);
    CHECK(P.k[0].m == m && P.k[0].cC == c && P.k[0].need_lm == n + c && P.k[0].w_lm == (unsigned)(n + c > 256 ? 2 : 1));
    CHECK(P.k[1].m == 1 && P.k[1].need_lm == 41 && P.k[1].w_lm == 1);
    return device_layout_ok(P, src.ix, dst);
}

}  // namespace

int main()
{
    const int32_t nk = 7;
    Image src(nk, 100, 40, 300, 90), dsti(nk, 0, 0, 0, 0);
    plslam_map_insert_dst dst{dsti.ix, 0, 0, 0, 0};
    std::vector<int32_t> lc = {1, 5, 1, 2, 6, 0, 0, 4, 1};       // the second entry is already optimised
    std::vector<double> T((size_t)nk * 16);
    for (size_t i = 0; i < T.size(); ++i) T[i] = 0.25 * i;
    // entry 0: A, B, C, D; entry 1 (flag 0): C, C, A; entry 2: C, A
    Kind pts({{-1, 0, 7, 1, 8, 2, -1, 3, -1, 4, -1, 5, 9, 6, 10, 7}, {-1, 0, -1, 0, -1, 0, -1, 0, -1, 0, 3, 0}, {-1, 1, -1, 2, -1, 3, 4, 5}}, 3, 2);
    Kind lns({{}, {}, {-1, 1, -1, 2}}, 6, 3);
    LcFusePlan P;
    // the bounds: cC = 2, cAB = 3 for the points (the flag-0 entry asks for nothing), cC = 1 for the lines
    dst.pt_cap = 102; dst.pt_obs_cap = 300 + 3 + 4; dst.ls_cap = 41; dst.ls_obs_cap = 92;
    CHECK(lc_fuse_plan(&src.ix, &dst, 3, lc.data(), T.data(), &pts.k, &lns.k, &P) == PLSLAM_OK);
    CHECK(P.k[0].m == 9 && P.k[0].cC == 2 && P.k[0].cAB == 3 && P.k[0].need_lm == 102 && P.k[0].need_obs == 307);
    CHECK(P.k[1].m == 1 && P.k[1].cC == 1 && P.k[1].cAB == 0 && P.k[1].need_lm == 41 && P.k[1].need_obs == 92);
    // each capacity one below its bound
    int32_t* caps[4] = {&dst.pt_cap, &dst.pt_obs_cap, &dst.ls_cap, &dst.ls_obs_cap};
    for (int32_t* c : caps) {
        --*c;
        CHECK(lc_fuse_plan(&src.ix, &dst, 3, lc.data(), T.data(), &pts.k, &lns.k, &P) == PLSLAM_ERANGE);
        ++*c;
    }
    // the packing: an exact-size block, every array where the plan says, the padding zero
    CHECK(lc_fuse_plan(&src.ix, &dst, 3, lc.data(), T.data(), &pts.k, &lns.k, &P) == PLSLAM_OK);
    {
        std::vector<char> stage(P.stage_bytes, (char)0x5a);
        lc_fuse_pack(P, lc.data(), T.data(), stage.data());
        CHECK(!memcmp(stage.data() + P.o_lc, lc.data(), lc.size() * 4) && !memcmp(stage.data() + P.o_T, T.data(), T.size() * 8));
        const Kind* K[2] = {&pts, &lns};
        for (int k = 0; k < 2; ++k) {
            const LcFuseKindPlan& Q = P.k[k];
            CHECK(!memcmp(stage.data() + Q.o_tup, K[k]->tup.data(), K[k]->tup.size() * 4));
            CHECK(!memcmp(stage.data() + Q.o_eptr, K[k]->eptr.data(), K[k]->eptr.size() * 4));
            CHECK(!memcmp(stage.data() + Q.o_P0, K[k]->P0.data(), K[k]->P0.size() * 8));
            CHECK(!memcmp(stage.data() + Q.o_o0, K[k]->o0.data(), K[k]->o0.size() * 8));
            CHECK(!memcmp(stage.data() + Q.o_P1, K[k]->P1.data(), K[k]->P1.size() * 8));
            CHECK(!memcmp(stage.data() + Q.o_o1, K[k]->o1.data(), K[k]->o1.size() * 8));
            CHECK(Q.o_tup % 256 == 0 && Q.o_P0 % 256 == 0 && Q.o_o1 + K[k]->o1.size() * 8 <= P.stage_bytes);
        }
        CHECK(stage[P.o_lc + lc.size() * 4] == 0);
    }
    // a NULL kind, and a kind with no tuple at all
    CHECK(lc_fuse_plan(&src.ix, &dst, 3, lc.data(), T.data(), &pts.k, nullptr, &P) == PLSLAM_OK && P.k[1].m == 0 && !P.k[1].in);
    {
        Kind none({{}, {}, {}}, 3, 2);
        none.k.tuples = nullptr; none.k.P0 = none.k.obs0 = none.k.P1 = none.k.obs1 = nullptr;
        CHECK(lc_fuse_plan(&src.ix, &dst, 3, lc.data(), T.data(), &none.k, nullptr, &P) == PLSLAM_OK && P.k[0].m == 0);
        std::vector<char> stage(P.stage_bytes);
        lc_fuse_pack(P, lc.data(), T.data(), stage.data());
    }
    // the refusals
    CHECK(lc_fuse_plan(nullptr, &dst, 3, lc.data(), T.data(), &pts.k, &lns.k, &P) == PLSLAM_EINVAL);
    CHECK(lc_fuse_plan(&src.ix, nullptr, 3, lc.data(), T.data(), &pts.k, &lns.k, &P) == PLSLAM_EINVAL);
    CHECK(lc_fuse_plan(&src.ix, &dst, 3, nullptr, T.data(), &pts.k, &lns.k, &P) == PLSLAM_EINVAL);
    CHECK(lc_fuse_plan(&src.ix, &dst, 3, lc.data(), nullptr, &pts.k, &lns.k, &P) == PLSLAM_EINVAL);
    CHECK(lc_fuse_plan(&src.ix, &dst, 0, lc.data(), T.data(), &pts.k, &lns.k, &P) == PLSLAM_EINVAL);
    for (int bad = 0; bad < 4; ++bad) {
        std::vector<int32_t> l2 = lc;
        if (bad == 0) l2[0] = l2[1];                             // kf_prev == kf_curr
        if (bad == 1) l2[0] = -1;
        if (bad == 2) l2[7] = nk;
        if (bad == 3) { l2[3] = l2[4] = nk + 3; }                // an entry already optimised is not validated
        CHECK(lc_fuse_plan(&src.ix, &dst, 3, l2.data(), T.data(), &pts.k, &lns.k, &P) == (bad == 3 ? PLSLAM_OK : PLSLAM_EINVAL));
    }
    {
        plslam_map_insert_dst same = dst;                        // a destination array that is a source array
        same.map.points.obs_kf = src.ix.points.obs_kf;
        CHECK(lc_fuse_plan(&src.ix, &same, 3, lc.data(), T.data(), &pts.k, &lns.k, &P) == PLSLAM_EINVAL);
        same = dst;
        same.map.kf_valid = src.ix.kf_valid;                     // (these may alias)
        same.map.lines.feat_ptr = src.ix.lines.feat_ptr;
        CHECK(lc_fuse_plan(&src.ix, &same, 3, lc.data(), T.data(), &pts.k, &lns.k, &P) == PLSLAM_OK);
    }
    {
        Kind k2 = pts;                                           // offsets that do not start at 0 / that decrease
        k2.k = plslam_lc_fuse_kind{k2.tup.data(), k2.eptr.data(), k2.P0.data(), k2.o0.data(), k2.P1.data(), k2.o1.data()};
        k2.eptr[0] = 1;
        CHECK(lc_fuse_plan(&src.ix, &dst, 3, lc.data(), T.data(), &k2.k, &lns.k, &P) == PLSLAM_EINVAL);
        k2.eptr[0] = 0; k2.eptr[2] = 3;
        CHECK(lc_fuse_plan(&src.ix, &dst, 3, lc.data(), T.data(), &k2.k, &lns.k, &P) == PLSLAM_EINVAL);
        k2.eptr[2] = 7; k2.k.P1 = nullptr;
        CHECK(lc_fuse_plan(&src.ix, &dst, 3, lc.data(), T.data(), &k2.k, &lns.k, &P) == PLSLAM_EINVAL);
    }
    {
        std::vector<int32_t> ep = {0, 0, 0, PLSLAM_LC_FUSE_MAX_TUPLES + 1};   // beyond the limit: refused before a tuple is read
        plslam_lc_fuse_kind huge{nullptr, ep.data(), nullptr, nullptr, nullptr, nullptr};
        CHECK(lc_fuse_plan(&src.ix, &dst, 3, lc.data(), T.data(), &huge, nullptr, &P) == PLSLAM_ERANGE);
    }
    // ---- the device layout: the tuples, the landmarks it can end with and the features each at 0, 255, 256 and 257 ----
    CHECK(lc_fuse_plan(&src.ix, &dst, 3, lc.data(), T.data(), &pts.k, &lns.k, &P) == PLSLAM_OK);
    CHECK(device_layout_ok(P, src.ix, dst) == 0);
    // 102 point landmarks at most: one tile, one chain word; the staged block sits behind the three fill regions
    CHECK(P.k[0].w_lm == 1 && P.k[1].w_lm == 1 && P.k[0].d_part == P.k[0].d_win + 256 && P.k[1].d_win == P.k[0].d_part + 256);
    const int32_t edge[4] = {0, 255, 256, 257};
    for (int e = 0; e < 4; ++e) {
        CHECK(layout_case(100, 10, edge[e], 0) == 0);                            // m
        CHECK(layout_case(edge[e] ? edge[e] - 5 : 0, 10, edge[e] ? 9 : 0, edge[e] ? 5 : 0) == 0);   // need_lm = n + cC
        CHECK(layout_case(100, edge[e], 9, 5) == 0);                             // n_feat
    }
    printf("lc_fuse_layout: ok\n");
    printf("lc_fuse_pack: ok\n");
    return 0;
}
