// loop_closure.hpp -- C++ host shim: MapHandler::isLoopClosure / computeRelativePoseRobustGN on top of the C ABI
// (plslam_loop_closure_verify, plslam_relpose_robust_gn; K25), and LoopClosureBatch: the same check for several candidate
// pairs in one call (plslam_lc_batch_verify; K54).
//
// Mirrors   bool MapHandler::isLoopClosure(const KeyFrame* kf0, const KeyFrame* kf1, Vector6d& pose_inc,
//                                          vector<Vector4i>& lc_pt_idx, vector<Vector4i>& lc_ls_idx, ...)   src/mapHandler.cpp:3192
//           bool MapHandler::computeRelativePoseRobustGN(...)                                                 :3566
// The keyframe is a template argument: any view with the stereo frame's members works unchanged --
//   pdesc_l / ldesc_l   descriptor blocks (rows, ptr<uchar>(), continuous N x 32), and
//   stereo_pt[i]->P (3), ->pl (2), ->idx;  stereo_ls[i]->sP, ->eP (3), ->le (3), ->idx   (operator() / operator[] indexing).
// Vec6 / Idx4 are templates as well (Eigen's Vector6d / Vector4i, or any type with operator()(int) / operator[]).
// Header-only; link with libplslam_hip.so.  Errors throw std::runtime_error.
#pragma once

#include <stdint.h>

#include <map>
#include <stdexcept>
#include <string>
#include <vector>

#include "plslam_hip.h"

namespace plslam {

class LoopClosure {
public:
    LoopClosure(plslam_ctx* ctx, const plslam_lc_params& p) : ctx_(ctx), p_(p) {}

    // isLoopClosure: returns its value, writes pose_inc on success (untouched otherwise, as the reference), and fills
    // lc_pt_idx / lc_ls_idx as :3914-3946 leave them (the inlier rows on success, every match otherwise)
    template <class Frame, class Vec6, class Idx4>
    bool isLoopClosure(const Frame& kf0, const Frame& kf1, Vec6& pose_inc, std::vector<Idx4>& lc_pt_idx,
                       std::vector<Idx4>& lc_ls_idx)
    {
        Packed a, b;
        pack(kf0, a);
        pack(kf1, b);
        plslam_lc_keyframe k0 = a.record(), k1 = b.record();
        std::vector<int32_t> pc((size_t)k0.n_pt * 4), lc((size_t)k0.n_ls * 4);
        std::vector<uint8_t> pi((size_t)k0.n_pt), li((size_t)k0.n_ls);
        check(plslam_loop_closure_verify(ctx_, &p_, &k0, &k1, &last_, pc.data(), pi.data(), lc.data(), li.data()),
              "plslam_loop_closure_verify");
        rows(pc, pi, last_.common_pt, last_.is_lc != 0, lc_pt_idx);
        rows(lc, li, last_.common_ls, last_.is_lc != 0, lc_ls_idx);
        if (last_.is_lc)
            for (int k = 0; k < 6; ++k) pose_inc(k) = last_.pose_inc[k];
        return last_.is_lc != 0;
    }

    // computeRelativePoseRobustGN on caller-built correspondences (lc_points / lc_lines as flat arrays)
    bool computeRelativePoseRobustGN(const std::vector<double>& P, const std::vector<double>& pl_obs, const std::vector<double>& sPeP,
                                     const std::vector<double>& le_obs, double pose_inc[6], std::vector<uint8_t>* pt_inlier = nullptr,
                                     std::vector<uint8_t>* ls_inlier = nullptr)
    {
        const int32_t np = (int32_t)(P.size() / 3), nl = (int32_t)(sPeP.size() / 6);
        if (pt_inlier) pt_inlier->assign((size_t)np, 0);
        if (ls_inlier) ls_inlier->assign((size_t)nl, 0);
        check(plslam_relpose_robust_gn(ctx_, &p_, P.data(), pl_obs.data(), np, sPeP.data(), le_obs.data(), nl, &last_,
                                       pt_inlier ? pt_inlier->data() : nullptr, ls_inlier ? ls_inlier->data() : nullptr),
              "plslam_relpose_robust_gn");
        if (last_.is_lc)
            for (int k = 0; k < 6; ++k) pose_inc[k] = last_.pose_inc[k];
        return last_.is_lc != 0;
    }

    const plslam_lc_result& last() const { return last_; }

private:
    friend class LoopClosureBatch;
    struct Packed {
        std::vector<uint8_t> pdesc, ldesc;
        std::vector<double> P, pl, sPeP, le;
        std::vector<int32_t> pt_idx, ls_idx;
        plslam_lc_keyframe record() const
        {
            plslam_lc_keyframe k;
            k.pdesc = pdesc.data(); k.P = P.data(); k.pl = pl.data(); k.pt_idx = pt_idx.data(); k.n_pt = (int32_t)pt_idx.size();
            k.ldesc = ldesc.data(); k.sPeP = sPeP.data(); k.le = le.data(); k.ls_idx = ls_idx.data(); k.n_ls = (int32_t)ls_idx.size();
            return k;
        }
    };

    static void check(int rc, const char* where)
    {
        if (rc != PLSLAM_OK)
            throw std::runtime_error(std::string(where) + ": " + plslam_strerror(rc) + "; " + plslam_last_error());
    }

    template <class Desc>
    static void desc_rows(const Desc& d, size_t n, std::vector<uint8_t>& out)
    {
        out.resize(n * 32);
        for (size_t i = 0; i < n; ++i)
            for (int b = 0; b < 32; ++b) out[i * 32 + b] = d.template ptr<unsigned char>((int)i)[b];
    }

    template <class Frame>
    static void pack(const Frame& f, Packed& o)
    {
        const size_t np = f.stereo_pt.size(), nl = f.stereo_ls.size();
        desc_rows(f.pdesc_l, np, o.pdesc);
        desc_rows(f.ldesc_l, nl, o.ldesc);
        o.P.resize(np * 3); o.pl.resize(np * 2); o.pt_idx.resize(np);
        for (size_t i = 0; i < np; ++i) {
            const auto& s = *f.stereo_pt[i];
            for (int k = 0; k < 3; ++k) o.P[i * 3 + k] = s.P(k);
            for (int k = 0; k < 2; ++k) o.pl[i * 2 + k] = s.pl(k);
            o.pt_idx[i] = s.idx;
        }
        o.sPeP.resize(nl * 6); o.le.resize(nl * 3); o.ls_idx.resize(nl);
        for (size_t i = 0; i < nl; ++i) {
            const auto& s = *f.stereo_ls[i];
            for (int k = 0; k < 3; ++k) { o.sPeP[i * 6 + k] = s.sP(k); o.sPeP[i * 6 + 3 + k] = s.eP(k); o.le[i * 3 + k] = s.le(k); }
            o.ls_idx[i] = s.idx;
        }
    }

    template <class Idx4>
    static void rows(const std::vector<int32_t>& c, const std::vector<uint8_t>& inl, int32_t n, bool only_inliers,
                     std::vector<Idx4>& out)
    {
        out.clear();
        for (int32_t k = 0; k < n; ++k) {
            if (only_inliers && !inl[(size_t)k]) continue;
            Idx4 v;
            for (int q = 0; q < 4; ++q) v(q) = c[(size_t)k * 4 + q];
            out.push_back(v);
        }
    }

    plslam_ctx* ctx_;
    plslam_lc_params p_;
    plslam_lc_result last_{};
};

// isLoopClosure for several (kf0, kf1) pairs in one call -- e.g. the best K candidates of lookForLoopCandidates against
// the current keyframe.  Pair b's outputs are what LoopClosure::isLoopClosure(*kf0[b], *kf1[b], ...) leaves, bit for bit.
class LoopClosureBatch {
public:
    LoopClosureBatch(plslam_ctx* ctx, const plslam_lc_params& p, int max_pairs) : max_pairs_(max_pairs)
    {
        LoopClosure::check(plslam_lc_batch_create(ctx, &p, max_pairs, &h_), "plslam_lc_batch_create");
    }
    ~LoopClosureBatch() { plslam_lc_batch_destroy(h_); }
    LoopClosureBatch(const LoopClosureBatch&) = delete;
    LoopClosureBatch& operator=(const LoopClosureBatch&) = delete;

    // kf0[b], kf1[b]: the reference's KeyFrame* pairs (a keyframe that appears several times is packed and uploaded once).
    // is_lc[b]: isLoopClosure's value; pose_inc[b] written on success only (resized, earlier entries kept);
    // lc_pt_idx[b] / lc_ls_idx[b] as :3914-3946 leave them
    template <class Frame, class Vec6, class Idx4>
    void isLoopClosure(const std::vector<const Frame*>& kf0, const std::vector<const Frame*>& kf1, std::vector<Vec6>& pose_inc,
                       std::vector<std::vector<Idx4>>& lc_pt_idx, std::vector<std::vector<Idx4>>& lc_ls_idx,
                       std::vector<bool>& is_lc)
    {
        if (kf0.size() != kf1.size() || kf0.size() > (size_t)max_pairs_)
            throw std::runtime_error("LoopClosureBatch::isLoopClosure: kf0 and kf1 differ in length, or exceed max_pairs");
        const size_t B = kf0.size();
        std::map<const Frame*, LoopClosure::Packed> packed;
        for (size_t q = 0; q < 2 * B; ++q) {
            const Frame* f = q < B ? kf0[q] : kf1[q - B];
            if (!packed.count(f)) LoopClosure::pack(*f, packed[f]);
        }
        std::vector<plslam_lc_keyframe> r0(B), r1(B);
        size_t sp = 0, sl = 0;
        for (size_t b = 0; b < B; ++b) {
            r0[b] = packed[kf0[b]].record();
            r1[b] = packed[kf1[b]].record();
            sp += (size_t)r0[b].n_pt;
            sl += (size_t)r0[b].n_ls;
        }
        std::vector<int32_t> pc(sp * 4), lc(sl * 4);
        std::vector<uint8_t> pi(sp), li(sl);
        last_.assign(B, plslam_lc_result{});
        LoopClosure::check(plslam_lc_batch_verify(h_, r0.data(), r1.data(), (int32_t)B, last_.data(), pc.data(), pi.data(), lc.data(),
                                                  li.data()), "plslam_lc_batch_verify");
        pose_inc.resize(B);
        lc_pt_idx.resize(B);
        lc_ls_idx.resize(B);
        is_lc.assign(B, false);
        sp = sl = 0;
        for (size_t b = 0; b < B; ++b) {
            const plslam_lc_result& r = last_[b];
            rows(pc, pi, sp, r.common_pt, r.is_lc != 0, lc_pt_idx[b]);
            rows(lc, li, sl, r.common_ls, r.is_lc != 0, lc_ls_idx[b]);
            if (r.is_lc)
                for (int k = 0; k < 6; ++k) pose_inc[b](k) = r.pose_inc[k];
            is_lc[b] = r.is_lc != 0;
            sp += (size_t)r0[b].n_pt;
            sl += (size_t)r0[b].n_ls;
        }
    }

    const std::vector<plslam_lc_result>& last() const { return last_; }

private:
    template <class Idx4>
    static void rows(const std::vector<int32_t>& c, const std::vector<uint8_t>& inl, size_t row0, int32_t n, bool only_inliers,
                     std::vector<Idx4>& out)
    {
        out.clear();
        for (size_t k = row0; k < row0 + (size_t)n; ++k) {
            if (only_inliers && !inl[k]) continue;
            Idx4 v;
            for (int q = 0; q < 4; ++q) v(q) = c[k * 4 + q];
            out.push_back(v);
        }
    }

    plslam_lc_batch* h_ = nullptr;
    int max_pairs_;
    std::vector<plslam_lc_result> last_;
};

}  // namespace plslam
