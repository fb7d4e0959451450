// lc_plan.hpp -- the pure host half of the loop-closure check's six calls (loop_closure.hip): the argument checks, the record a
// workgroup of K25 / K54 runs on, the rule that turns candidate pairs into match problems and records, and the layouts of the
// two staged blocks of the host-pointer forms (the keyframe image that goes up, the output block that comes down).  No HIP in
// here, no context, no device: tests/cpp/test_lc_plan.cpp compiles it with g++ alone and runs it under the sanitizers.
// Addresses called "device" are only added to, never read through.
#pragma once

#include <cstdint>
#include <cstring>
#include <vector>

#include "gn_cam.hpp"
#include "match_tables.hpp"   // align256
#include "plslam_hip.h"

namespace plslam {
namespace {      // (K25's and K54's symbol names carry their parameter type: it stays in the namespace the kernels are in)

struct LcArgs {
    GnCam K;
    double th;
    const double* P;          // kf0 stereo_pt[i]->P  (n_pt0 x 3)   [identity: lc_points[k]->P]
    const double* pl;         // kf1 stereo_pt[i]->pl (n_pt1 x 2)   [identity: ->pl_obs]
    const int32_t* pt_idx0;   // may be null (-1)
    const int32_t* pt_idx1;
    const double* sPeP;       // kf0 (n_ls0 x 6)
    const double* le;         // kf1 (n_ls1 x 3)
    const int32_t* ls_idx0;
    const int32_t* ls_idx1;
    const int32_t* m12_p;     // the match tables (n_pt0 / n_ls0 entries); null: the kind was not matched
    const int32_t* m12_l;
    int32_t n_pt0, n_pt1, n_ls0, n_ls1;
    int32_t identity;         // plslam_relpose_robust_gn: correspondence k is (k, k), no gate
    int32_t has_points, has_lines, max_iters, max_iters_ref;
    double lc_inlier_ratio, lc_res, lc_unc, lc_inl, lc_trs, lc_rot;
    int32_t* pt_corr;         // n_pt0 x 4
    uint8_t* pt_inl;
    int32_t* ls_corr;
    uint8_t* ls_inl;
    plslam_lc_result* res;
};

static_assert(sizeof(LcArgs) % 8 == 0, "K54 copies its record in 8-byte words");

}  // namespace

// ---- the checks.  Inside the library PLSLAM_REQUIRE is common.hpp's, which also records the refused rule as the last error;
// compiled without it (the CPU test) a refusal is its code alone
#ifndef PLSLAM_REQUIRE
#define PLSLAM_REQUIRE(cond, code) do { if (!(cond)) return (code); } while (0)
#endif

inline int lc_check_params(const plslam_lc_params* p)
{
    PLSLAM_REQUIRE(p != nullptr, PLSLAM_EINVAL);
    PLSLAM_REQUIRE(p->max_iters >= 0 && p->max_iters <= PLSLAM_LC_MAX_ITERS, PLSLAM_EINVAL);
    PLSLAM_REQUIRE(p->max_iters_ref >= 0 && p->max_iters_ref <= PLSLAM_LC_MAX_ITERS, PLSLAM_EINVAL);
    return PLSLAM_OK;
}

inline int lc_check_kf(const plslam_lc_keyframe* k)
{
    PLSLAM_REQUIRE(k != nullptr && k->n_pt >= 0 && k->n_ls >= 0, PLSLAM_EINVAL);
    PLSLAM_REQUIRE(k->n_pt == 0 || (k->pdesc && k->P && k->pl), PLSLAM_EINVAL);
    PLSLAM_REQUIRE(k->n_ls == 0 || (k->ldesc && k->sPeP && k->le), PLSLAM_EINVAL);
    PLSLAM_REQUIRE(k->n_pt <= PLSLAM_LC_MAX_FEATURES && k->n_ls <= PLSLAM_LC_MAX_FEATURES, PLSLAM_ERANGE);
    return PLSLAM_OK;
}

// max_pairs: the batch object's, nullptr where there is no batch object
inline int lc_check_batch(const int32_t* max_pairs, const plslam_lc_keyframe* kf0, const plslam_lc_keyframe* kf1, int32_t B)
{
    int rc;
    PLSLAM_REQUIRE(max_pairs != nullptr, PLSLAM_EINVAL);
    PLSLAM_REQUIRE(B >= 0 && B <= *max_pairs, PLSLAM_EINVAL);
    PLSLAM_REQUIRE(B == 0 || (kf0 && kf1), PLSLAM_EINVAL);
    for (int32_t b = 0; b < B; ++b)
        if ((rc = lc_check_kf(kf0 + b)) || (rc = lc_check_kf(kf1 + b))) return rc;
    return PLSLAM_OK;
}

// ---- the records
inline void lc_fill_args(LcArgs& a, const plslam_lc_params* p)
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
}

// where a call's outputs go (device addresses): record b at res + b; rows as the pair planner and the output block say
struct LcOut { plslam_lc_result* res; int32_t* pt_corr; uint8_t* pt_inl; int32_t* ls_corr; uint8_t* ls_inl; };

// The record of computeRelativePoseRobustGN alone on the caller's correspondences: correspondence k is (k, k), no match table,
// no gate.  plslam_relpose_robust_gn gives its counts and all of `out`; the batched form gives counts of 0 (K54 reads them from
// the device) and no correspondence rows, and sets res per record.
inline void lc_identity_args(LcArgs& a, const plslam_lc_params* p, const double* P, const double* pl, int32_t npt,
                             const double* sPeP, const double* le, int32_t nls, const LcOut& out)
{
    memset(&a, 0, sizeof(a));
    lc_fill_args(a, p);
    a.P = P; a.pl = pl; a.sPeP = sPeP; a.le = le;
    a.n_pt0 = a.n_pt1 = npt; a.n_ls0 = a.n_ls1 = nls;
    a.identity = 1;
    a.res = out.res;
    a.pt_corr = out.pt_corr; a.pt_inl = out.pt_inl;
    a.ls_corr = out.ls_corr; a.ls_inl = out.ls_inl;
}

struct LcTake {       // slices of one block in the order they are taken, each on a multiple of 256 bytes
    size_t off = 0;
    size_t take(size_t bytes) { const size_t o = off; off += align256(bytes); return o; }
};

// ---- the pairs: match problems + records
// the match-table block of B pairs: the point tables (sum of kf0[b].n_pt entries), the line tables, 2 B match counters
struct LcTables { size_t oP, oL, oC, bytes; };
inline LcTables lc_tables(const plslam_lc_keyframe* kf0, int32_t B)
{
    size_t sp = 0, sl = 0;
    for (int32_t b = 0; b < B; ++b) { sp += (size_t)kf0[b].n_pt; sl += (size_t)kf0[b].n_ls; }
    LcTake t;
    LcTables T;
    T.oP = t.take(sp * 4); T.oL = t.take(sl * 4); T.oC = t.take((size_t)B * 8);
    T.bytes = t.off;
    return T;
}

// The match problems of :3222-3223 / :3248-3249 for every pair (kf0[b], kf1[b]) -- a kind is matched only where the source calls
// match(): has_points && n_pt0 > 0 && n_pt1 > 0, likewise the lines; a skipped kind has no problem and null m12_p / m12_l --
// and the B records K25 (B = 1) / K54 run on.  The records' arrays are device arrays already; tab: the device address of the
// block lc_tables() sized.  Pair b's rows start at row sum_{b' < b} kf0[b'].n_pt (n_ls) of the point (line) tables, of pt_corr
// (x 4 int32) and of the masks; a null base of `out` gives null fields.  The k-th problem of the list counts its matches in
// counter k, so a lines-only single call counts in counter 0 (no kernel reads the counters).
// probs: room for 2 B problems; args: B records.  Returns the number of problems.
inline int32_t lc_plan_pairs(const plslam_lc_params* p, const plslam_lc_keyframe* kf0, const plslam_lc_keyframe* kf1, int32_t B,
                             const LcTables& T, void* tab, const LcOut& out, plslam_match_problem* probs, LcArgs* args)
{
    int32_t* const mP = reinterpret_cast<int32_t*>(static_cast<char*>(tab) + T.oP);
    int32_t* const mL = reinterpret_cast<int32_t*>(static_cast<char*>(tab) + T.oL);
    int32_t* const cnt = reinterpret_cast<int32_t*>(static_cast<char*>(tab) + T.oC);
    int32_t n = 0;
    size_t rp = 0, rl = 0;
    for (int32_t b = 0; b < B; ++b) {
        const plslam_lc_keyframe *k0 = kf0 + b, *k1 = kf1 + b;
        const bool mp = p->has_points && k0->n_pt > 0 && k1->n_pt > 0;
        const bool ml = p->has_lines && k0->n_ls > 0 && k1->n_ls > 0;
        plslam_match_problem q;
        memset(&q, 0, sizeof(q));
        q.mutual = p->mutual ? 1 : 0;
        if (mp) {
            q.d1 = k0->pdesc; q.d2 = k1->pdesc; q.n1 = k0->n_pt; q.n2 = k1->n_pt; q.nnr = p->min_ratio_12_p;
            q.matches_12 = mP + rp; q.n_matches = cnt + n;
            probs[n++] = q;
        }
        if (ml) {
            q.d1 = k0->ldesc; q.d2 = k1->ldesc; q.n1 = k0->n_ls; q.n2 = k1->n_ls; q.nnr = p->min_ratio_12_l;
            q.matches_12 = mL + rl; q.n_matches = cnt + n;
            probs[n++] = q;
        }
        LcArgs& a = args[b];
        memset(&a, 0, sizeof(a));
        lc_fill_args(a, p);
        a.P = k0->P; a.pl = k1->pl; a.pt_idx0 = k0->pt_idx; a.pt_idx1 = k1->pt_idx;
        a.sPeP = k0->sPeP; a.le = k1->le; a.ls_idx0 = k0->ls_idx; a.ls_idx1 = k1->ls_idx;
        a.m12_p = mp ? mP + rp : nullptr;
        a.m12_l = ml ? mL + rl : nullptr;
        a.n_pt0 = k0->n_pt; a.n_pt1 = k1->n_pt; a.n_ls0 = k0->n_ls; a.n_ls1 = k1->n_ls;
        a.identity = 0;
        a.res = out.res + b;
        a.pt_corr = out.pt_corr ? out.pt_corr + 4 * rp : nullptr; a.pt_inl = out.pt_inl ? out.pt_inl + rp : nullptr;
        a.ls_corr = out.ls_corr ? out.ls_corr + 4 * rl : nullptr; a.ls_inl = out.ls_inl ? out.ls_inl + rl : nullptr;
        rp += (size_t)k0->n_pt;
        rl += (size_t)k0->n_ls;
    }
    return n;
}

// ---- the keyframe image: the page-locked block the host-pointer forms upload in one copy
// A record's eight arrays in the order of its fields -- pdesc, P, pl, pt_idx | ldesc, sPeP, le, ls_idx -- and their bytes per
// row; the fourth of each kind (the landmark indices) may be null.
constexpr int LC_KF_ARRAYS = 8;
constexpr size_t LC_KF_STRIDE[LC_KF_ARRAYS] = {32, 24, 16, 4, 32, 48, 24, 4};
struct LcKfArray { const void* src; size_t bytes; bool optional; };
inline void lc_kf_arrays(const plslam_lc_keyframe& k, LcKfArray a[LC_KF_ARRAYS])
{
    const void* src[LC_KF_ARRAYS] = {k.pdesc, k.P, k.pl, k.pt_idx, k.ldesc, k.sPeP, k.le, k.ls_idx};
    for (int i = 0; i < LC_KF_ARRAYS; ++i) a[i] = {src[i], (size_t)(i < 4 ? k.n_pt : k.n_ls) * LC_KF_STRIDE[i], (i & 3) == 3};
}

// The 2 B records of a call are kf0[0..B) then kf1[0..B).  A record is laid out once: first[q] is the first record with the
// same pdesc and memcmp-equal contents (q itself: laid out, its eight offsets at off[8 q ...]) -- every pair of a top-K
// verification has the same kf1.
struct LcKfImage {
    int32_t B = 0;
    std::vector<size_t> first, off;
    size_t bytes = 0;
    const plslam_lc_keyframe& rec(const plslam_lc_keyframe* k0, const plslam_lc_keyframe* k1, size_t q) const { return q < (size_t)B ? k0[q] : k1[q - (size_t)B]; }
};

inline void lc_kf_layout(const plslam_lc_keyframe* kf0, const plslam_lc_keyframe* kf1, int32_t B, LcKfImage& L)
{
    const size_t n2 = 2 * (size_t)B;
    L.B = B;
    L.first.assign(n2, 0);
    L.off.assign(n2 * LC_KF_ARRAYS, 0);
    LcTake t;
    for (size_t q = 0; q < n2; ++q) {
        const plslam_lc_keyframe& k = L.rec(kf0, kf1, q);
        L.first[q] = q;
        for (size_t r = 0; r < q; ++r) {
            const plslam_lc_keyframe& kr = L.rec(kf0, kf1, r);
            if (L.first[r] == r && kr.pdesc == k.pdesc && memcmp(&kr, &k, sizeof(plslam_lc_keyframe)) == 0) { L.first[q] = r; break; }
        }
        if (L.first[q] != q) continue;
        LcKfArray a[LC_KF_ARRAYS];
        lc_kf_arrays(k, a);
        for (int i = 0; i < LC_KF_ARRAYS; ++i) L.off[q * LC_KF_ARRAYS + i] = t.take(a[i].bytes);
    }
    L.bytes = t.off;
}

// fills the L.bytes at h (the slack between arrays, and an optional array that is null, are left as they are)
inline void lc_kf_fill(const plslam_lc_keyframe* kf0, const plslam_lc_keyframe* kf1, const LcKfImage& L, char* h)
{
    for (size_t q = 0; q < L.first.size(); ++q) {
        if (L.first[q] != q) continue;
        LcKfArray a[LC_KF_ARRAYS];
        lc_kf_arrays(L.rec(kf0, kf1, q), a);
        for (int i = 0; i < LC_KF_ARRAYS; ++i)
            if (a[i].bytes && a[i].src) memcpy(h + L.off[q * LC_KF_ARRAYS + i], a[i].src, a[i].bytes);
    }
}

// the 2 B records over the image's copy at device address d: D[q] for record q; an optional array that is null stays null
inline void lc_kf_device(const plslam_lc_keyframe* kf0, const plslam_lc_keyframe* kf1, const LcKfImage& L, char* d,
                         plslam_lc_keyframe* D)
{
    for (size_t q = 0; q < L.first.size(); ++q) {
        if (L.first[q] != q) { D[q] = D[L.first[q]]; continue; }
        const plslam_lc_keyframe& k = L.rec(kf0, kf1, q);
        LcKfArray a[LC_KF_ARRAYS];
        lc_kf_arrays(k, a);
        const void* at[LC_KF_ARRAYS];
        for (int i = 0; i < LC_KF_ARRAYS; ++i) at[i] = a[i].optional && !a[i].src ? nullptr : d + L.off[q * LC_KF_ARRAYS + i];
        D[q].n_pt = k.n_pt; D[q].n_ls = k.n_ls;
        D[q].pdesc = static_cast<const uint8_t*>(at[0]); D[q].P = static_cast<const double*>(at[1]);
        D[q].pl = static_cast<const double*>(at[2]); D[q].pt_idx = static_cast<const int32_t*>(at[3]);
        D[q].ldesc = static_cast<const uint8_t*>(at[4]); D[q].sPeP = static_cast<const double*>(at[5]);
        D[q].le = static_cast<const double*>(at[6]); D[q].ls_idx = static_cast<const int32_t*>(at[7]);
    }
}

// ---- the output block of the host-pointer forms: B result records, then pt_corr (16 bytes a row), pt_inlier (1), ls_corr,
// ls_inlier with the rows the pair planner gives pair b (capacity kf0[b].n_pt / n_ls)
struct LcOutBlock { size_t oR, oPC, oPI, oLC, oLI, bytes; };
inline LcOutBlock lc_out_block(const plslam_lc_keyframe* kf0, int32_t B)
{
    size_t sp = 0, sl = 0;
    for (int32_t b = 0; b < B; ++b) { sp += (size_t)kf0[b].n_pt; sl += (size_t)kf0[b].n_ls; }
    LcTake t;
    LcOutBlock L;
    L.oR = t.take((size_t)B * sizeof(plslam_lc_result));
    L.oPC = t.take(sp * 16); L.oPI = t.take(sp); L.oLC = t.take(sl * 16); L.oLI = t.take(sl);
    L.bytes = t.off;
    return L;
}

inline LcOut lc_out_bases(const LcOutBlock& L, char* base)
{
    return {reinterpret_cast<plslam_lc_result*>(base + L.oR), reinterpret_cast<int32_t*>(base + L.oPC),
            reinterpret_cast<uint8_t*>(base + L.oPI), reinterpret_cast<int32_t*>(base + L.oLC),
            reinterpret_cast<uint8_t*>(base + L.oLI)};
}

// from the block's host copy into the caller's arrays: the B records, and of pair b its common_pt / common_ls rows (what K25
// wrote) at the pair's row offset; a null array is skipped, rows beyond a pair's count are not touched
inline void lc_out_scatter(const LcOutBlock& L, const char* ho, const plslam_lc_keyframe* kf0, int32_t B,
                           plslam_lc_result* results, int32_t* pt_corr, uint8_t* pt_inlier, int32_t* ls_corr, uint8_t* ls_inlier)
{
    memcpy(results, ho + L.oR, (size_t)B * sizeof(plslam_lc_result));
    size_t rp = 0, rl = 0;
    for (int32_t b = 0; b < B; ++b) {
        const size_t ncp = (size_t)results[b].common_pt, ncl = (size_t)results[b].common_ls;
        if (pt_corr && ncp) memcpy(pt_corr + 4 * rp, ho + L.oPC + 16 * rp, ncp * 16);
        if (pt_inlier && ncp) memcpy(pt_inlier + rp, ho + L.oPI + rp, ncp);
        if (ls_corr && ncl) memcpy(ls_corr + 4 * rl, ho + L.oLC + 16 * rl, ncl * 16);
        if (ls_inlier && ncl) memcpy(ls_inlier + rl, ho + L.oLI + rl, ncl);
        rp += (size_t)kf0[b].n_pt;
        rl += (size_t)kf0[b].n_ls;
    }
}

}  // namespace plslam
