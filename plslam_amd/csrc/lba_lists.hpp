// lba_lists.hpp -- the host-built lists of the local BA: which observations every sum of the block assembly and of the Schur step
// runs over, and in which order.  Pure host code: no HIP header, no device, no context (tests/cpp/test_lba_lists.cpp compiles it
// with g++ alone).  The kernels that walk these lists are in lba_assemble_rows.hip, lba_plan.hip and lba_schur.hip.
#pragma once

#include <stdint.h>

#include <algorithm>
#include <vector>

namespace plslam {

// entry e of keyframe k: e < 36 -> H_pp[k][e/6][e%6]; e >= 36 -> g_p[k][e-36].
// Two-level, fixed-shape (deterministic) summation: chunk c of keyframe k sums observations
// [c*POSE_CHUNK, (c+1)*POSE_CHUNK) of the keyframe's list sequentially in list order, then the chunk
// partials are summed sequentially in chunk order.  (A single sequential chain over the ~6700
// observations of a C3 keyframe is bit-identical to the reference's dense accumulation but takes
// 1.9 ms on 9 workgroups; this takes microseconds and differs from it by rounding only.)
constexpr int POSE_CHUNK = 64;

// stable CSR lists (host, O(nobs)): observations per landmark and per keyframe, list order; keyframe
// lists hold points first, then lines (global ids: points [0, n_pt_obs), lines n_pt_obs + o)
struct CsrLists { std::vector<int32_t> ptp, pti, lsp, lsi, kfp, kfi; };
// one stable list: the observations o < n by key[o] in [0, nkeys), list order; keep != nullptr: only those with keep[o] >= 0
// (the global BA's lists, gba_lists.hpp: the observations by optimised keyframes)
inline void csr_by_key(const int32_t* key, int32_t n, int32_t nkeys, std::vector<int32_t>& ptr, std::vector<int32_t>& ids,
                       const int32_t* keep = nullptr)
{
    ptr.assign((size_t)nkeys + 1, 0);
    for (int32_t o = 0; o < n; ++o) if (!keep || keep[o] >= 0) ++ptr[key[o] + 1];
    for (int32_t k = 0; k < nkeys; ++k) ptr[k + 1] += ptr[k];
    ids.assign((size_t)ptr[nkeys], 0);
    std::vector<int32_t> pos(ptr.begin(), ptr.end() - 1);
    for (int32_t o = 0; o < n; ++o) if (!keep || keep[o] >= 0) ids[pos[key[o]]++] = o;
}
inline void build_csr(const int32_t* pt_lm, const int32_t* pt_kf, int32_t np, const int32_t* ls_lm,
                      const int32_t* ls_kf, int32_t nl, int32_t nkf, int32_t npt, int32_t nls, CsrLists& c)
{
    csr_by_key(pt_lm, np, npt, c.ptp, c.pti);
    csr_by_key(ls_lm, nl, nls, c.lsp, c.lsi);
    c.kfp.assign((size_t)nkf + 1, 0);
    for (int32_t o = 0; o < np; ++o) if (pt_kf[o] >= 0) ++c.kfp[pt_kf[o] + 1];
    for (int32_t o = 0; o < nl; ++o) if (ls_kf[o] >= 0) ++c.kfp[ls_kf[o] + 1];
    for (int32_t k = 0; k < nkf; ++k) c.kfp[k + 1] += c.kfp[k];
    c.kfi.assign((size_t)c.kfp[nkf], 0);
    std::vector<int32_t> pos(c.kfp.begin(), c.kfp.end() - 1);
    for (int32_t o = 0; o < np; ++o) if (pt_kf[o] >= 0) c.kfi[pos[pt_kf[o]]++] = o;
    for (int32_t o = 0; o < nl; ++o) if (ls_kf[o] >= 0) c.kfi[pos[ls_kf[o]]++] = np + o;
}

inline int32_t pose_max_chunks(const std::vector<int32_t>& kfp)
{
    int32_t m = 0;
    for (size_t k = 0; k + 1 < kfp.size(); ++k) m = std::max(m, (kfp[k + 1] - kfp[k] + POSE_CHUNK - 1) / POSE_CHUNK);
    return m;
}

constexpr int SCH_CHUNK = 64;
struct SchurPair { int32_t o1, o2, lm, line; };     // observation ids within their own list (points / lines), the landmark

// the pair lists of the Schur step: every ordered pair (o1, o2) of observations of ONE landmark by OPTIMISED keyframes
// with kf(o1) <= kf(o2), sorted by block (k1, k2) -- stable: landmark order, then list order.  Block (k1 <= k2) is number
// k1 * nkf - k1 * (k1 - 1) / 2 + (k2 - k1): row-major over the upper triangle; its pairs are pairs[cnt[B] .. cnt[B + 1]).
struct SchurLists {
    std::vector<SchurPair> pairs;
    std::vector<int32_t> cnt;          // nblk + 1 offsets into pairs
    int32_t schur_chunks = 0;          // the largest block's count of SCH_CHUNK-pair chunks
};
inline SchurLists build_schur_pairs(const CsrLists& csr, const std::vector<int32_t>& pt_kf, const std::vector<int32_t>& ls_kf, int32_t nkf)
{
    const int32_t nblk = nkf * (nkf + 1) / 2;
    auto blk_of = [nkf](int32_t k1, int32_t k2) { return k1 * nkf - k1 * (k1 - 1) / 2 + (k2 - k1); };
    SchurLists L;
    std::vector<int32_t>& cnt = L.cnt;
    cnt.assign((size_t)nblk + 1, 0);
    auto each_pair = [&](auto&& fn) {
        for (int line = 0; line < 2; ++line) {
            const std::vector<int32_t>& ptr = line ? csr.lsp : csr.ptp;
            const std::vector<int32_t>& ids = line ? csr.lsi : csr.pti;
            const std::vector<int32_t>& kf = line ? ls_kf : pt_kf;
            const int32_t nlm = (int32_t)ptr.size() - 1;
            for (int32_t j = 0; j < nlm; ++j)
                for (int32_t i1 = ptr[j]; i1 < ptr[j + 1]; ++i1) {
                    const int32_t o1 = ids[i1], k1 = kf[o1];
                    if (k1 < 0) continue;
                    for (int32_t i2 = ptr[j]; i2 < ptr[j + 1]; ++i2) {
                        const int32_t o2 = ids[i2], k2 = kf[o2];
                        if (k2 < k1) continue;             // (k2 < 0 included)
                        fn(blk_of(k1, k2), SchurPair{o1, o2, j, line});
                    }
                }
        }
    };
    // a block's point pairs, then its line pairs starting at a CHUNK boundary (null pairs -- line = 2: no contribution -- fill the last
    // point chunk of a block that has both kinds): every chunk is of one kind, and the wave fetches its rows together
    std::vector<int32_t> npt_pairs((size_t)nblk, 0), nls_pairs((size_t)nblk, 0);
    each_pair([&](int32_t B, const SchurPair& q) { ++(q.line ? nls_pairs : npt_pairs)[(size_t)B]; });
    auto pt_room = [&](int32_t B) {
        const int32_t np_ = npt_pairs[(size_t)B];
        return nls_pairs[(size_t)B] ? (np_ + SCH_CHUNK - 1) / SCH_CHUNK * SCH_CHUNK : np_;
    };
    for (int32_t B = 0; B < nblk; ++B) cnt[(size_t)B + 1] = cnt[B] + pt_room(B) + nls_pairs[(size_t)B];
    L.pairs.assign((size_t)cnt[nblk], SchurPair{0, 0, 0, 2});
    std::vector<int32_t> pos_pt(cnt.begin(), cnt.end() - 1), pos_ls((size_t)nblk);
    for (int32_t B = 0; B < nblk; ++B) pos_ls[(size_t)B] = cnt[B] + pt_room(B);
    each_pair([&](int32_t B, const SchurPair& q) { L.pairs[(size_t)(q.line ? pos_ls : pos_pt)[(size_t)B]++] = q; });
    for (int32_t B = 0; B < nblk; ++B) L.schur_chunks = std::max(L.schur_chunks, (cnt[(size_t)B + 1] - cnt[B] + SCH_CHUNK - 1) / SCH_CHUNK);
    return L;
}

}  // namespace plslam
