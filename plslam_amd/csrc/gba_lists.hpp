// gba_lists.hpp -- the host-built lists of the global bundle adjustment (gba.hip): the checks on the Vector6i observation columns,
// the per-observation index arrays, the four CSR lists and the covisible blocks with their ragged chunks of observation pairs.
// Pure host code: no HIP header, no device, no context (tests/cpp/test_gba_lists.cpp compiles it with g++ alone and runs it under
// the sanitizers).  The kernels that walk these lists are K28-K31 and K37 of gba.hip.
#pragma once

#include <stdint.h>

#include <algorithm>
#include <vector>

#include "lba_lists.hpp"
#include "plslam_hip.h"

namespace plslam {

constexpr int GBA_CHUNK = 64;   // observation pairs per chunk of K29

struct GbaBlock { int32_t k1, k2, c0, c1; };          // covisible block (k1 >= k2) and its chunk range
struct GbaChunk { int32_t blk, line, p0, np; };       // chunk: block, kind (1 = lines), first pair, pair count
struct GbaPair { int32_t o1, o2; };                   // observation ids within their own list; the kernels read it as an int2

struct GbaLists {
    // per observation: its landmark (local index), its optimised keyframe (-1: not optimised) and the pose slot its rows read
    std::vector<int32_t> plm, pkf, pslot, llm, lkf, lslot;
    // landmark -> its observations by optimised keyframes (lpp / lpo points, llp / llo lines); optimised keyframe -> its
    // observations (kpp / kpo, klp / klo); all in list order
    std::vector<int32_t> lpp, lpo, llp, llo, kpp, kpo, klp, klo;
    std::vector<GbaBlock> blks;
    std::vector<GbaChunk> chks;
    std::vector<GbaPair> pairs;
    const char* why = "";                             // what was refused
};

// Vector6i columns: 0 landmark map index, 1 landmark local index, 2 observation index, 3 keyframe map index, 4 keyframe
// local index (-1: keyframe 0, not optimised), 5 inlier flag.  PLSLAM_OK or PLSLAM_EINVAL (L->why says which rule).
inline int gba_lists_build(int32_t n_map_kf, int32_t nkf, const int32_t* kf_list, int32_t npt, int32_t nls, const int32_t* pt_obs,
                           int32_t n_pt_obs, const int32_t* ls_obs, int32_t n_ls_obs, GbaLists* L)
{
#define GBA_REFUSE(cond, text)       \
    do {                             \
        if (cond) {                  \
            L->why = text;           \
            return PLSLAM_EINVAL;    \
        }                            \
    } while (0)
    GBA_REFUSE(!kf_list || nkf < 1 || n_map_kf < 0 || npt < 0 || nls < 0 || n_pt_obs < 0 || n_ls_obs < 0, "a NULL list or a negative count");
    GBA_REFUSE((n_pt_obs > 0 && !pt_obs) || (n_ls_obs > 0 && !ls_obs), "observations without their columns");
    for (int32_t k = 0; k < nkf; ++k) GBA_REFUSE(kf_list[k] < 0 || kf_list[k] >= n_map_kf, "kf_list names a slot out of range");
    L->plm.resize(n_pt_obs); L->pkf.resize(n_pt_obs); L->pslot.resize(n_pt_obs);
    L->llm.resize(n_ls_obs); L->lkf.resize(n_ls_obs); L->lslot.resize(n_ls_obs);
    for (int32_t o = 0; o < n_pt_obs; ++o) {
        const int32_t* v = pt_obs + 6 * (size_t)o;
        GBA_REFUSE(!(v[1] >= 0 && v[1] < npt && v[3] >= 0 && v[3] < n_map_kf && v[4] >= -1 && v[4] < nkf), "a point column out of range");
        GBA_REFUSE(!(v[4] < 0 || kf_list[v[4]] == v[3]), "a point's local keyframe is not its map keyframe");
        L->plm[o] = v[1]; L->pkf[o] = v[4];
        L->pslot[o] = v[4] >= 0 ? n_map_kf + v[4] : v[3];   // points of optimised keyframes read the estimate (:2411-2416)
    }
    for (int32_t o = 0; o < n_ls_obs; ++o) {
        const int32_t* v = ls_obs + 6 * (size_t)o;
        GBA_REFUSE(!(v[1] >= 0 && v[1] < nls && v[3] >= 0 && v[3] < n_map_kf && v[4] >= -1 && v[4] < nkf), "a line column out of range");
        GBA_REFUSE(!(v[4] < 0 || kf_list[v[4]] == v[3]), "a line's local keyframe is not its map keyframe");
        L->llm[o] = v[1]; L->lkf[o] = v[4];
        L->lslot[o] = v[3];                                  // lines always read the stored pose (:2523)
    }
    // landmark -> its observations by optimised keyframes, list order; keyframe -> its observations, list order
    csr_by_key(L->plm.data(), n_pt_obs, npt, L->lpp, L->lpo, L->pkf.data());
    csr_by_key(L->llm.data(), n_ls_obs, nls, L->llp, L->llo, L->lkf.data());
    csr_by_key(L->pkf.data(), n_pt_obs, nkf, L->kpp, L->kpo, L->pkf.data());
    csr_by_key(L->lkf.data(), n_ls_obs, nkf, L->klp, L->klo, L->lkf.data());

    // covisible blocks: every ordered pair (o1, o2) of a landmark's observations with kf(o1) >= kf(o2) falls in lower block
    // (kf(o1), kf(o2)); blocks sorted by (k1, k2), a block's point pairs before its line pairs, each in landmark order
    struct Pr { int64_t key; int32_t line, o1, o2; };
    std::vector<Pr> prs;
    auto add_pairs = [&](const std::vector<int32_t>& ptr, const std::vector<int32_t>& ids, const std::vector<int32_t>& kf, int line,
                         int32_t nlm) {
        for (int32_t j = 0; j < nlm; ++j)
            for (int32_t a = ptr[j]; a < ptr[j + 1]; ++a)
                for (int32_t b = ptr[j]; b < ptr[j + 1]; ++b) {
                    const int32_t o1 = ids[a], o2 = ids[b];
                    if (kf[o1] >= kf[o2]) prs.push_back({(int64_t)kf[o1] * nkf + kf[o2], line, o1, o2});
                }
    };
    add_pairs(L->lpp, L->lpo, L->pkf, 0, npt);
    add_pairs(L->llp, L->llo, L->lkf, 1, nls);
    for (int32_t k = 0; k < nkf; ++k) prs.push_back({(int64_t)k * nkf + k, 2, -1, -1});   // every diagonal block exists
    std::stable_sort(prs.begin(), prs.end(), [](const Pr& x, const Pr& y) { return x.key != y.key ? x.key < y.key : x.line < y.line; });
    std::vector<GbaBlock>& blks = L->blks;
    std::vector<GbaChunk>& chks = L->chks;
    std::vector<GbaPair>& pairs = L->pairs;
    blks.clear(); chks.clear(); pairs.clear();
    pairs.reserve(prs.size());
    for (size_t i = 0; i < prs.size();) {
        size_t e = i;
        while (e < prs.size() && prs[e].key == prs[i].key) ++e;
        GbaBlock B{(int32_t)(prs[i].key / nkf), (int32_t)(prs[i].key % nkf), (int32_t)chks.size(), 0};
        for (size_t q = i; q < e;) {
            if (prs[q].line == 2) { ++q; continue; }
            size_t r = q;
            while (r < e && prs[r].line == prs[q].line && r - q < (size_t)GBA_CHUNK) ++r;
            chks.push_back({(int32_t)blks.size(), prs[q].line, (int32_t)pairs.size(), (int32_t)(r - q)});
            for (size_t u = q; u < r; ++u) pairs.push_back({prs[u].o1, prs[u].o2});
            q = r;
        }
        B.c1 = (int32_t)chks.size();
        blks.push_back(B);
        i = e;
    }
    // pairs and chunk partials (36 doubles each) are indexed with int32
    GBA_REFUSE(pairs.size() >= (size_t)INT32_MAX || chks.size() * 36 >= (size_t)INT32_MAX, "more pairs or chunks than int32 indexes");
#undef GBA_REFUSE
    return PLSLAM_OK;
}

}  // namespace plslam
