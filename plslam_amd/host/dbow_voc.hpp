// dbow_voc.hpp -- C++ host shim: the reference's bag-of-words calls on top of the C ABI (plslam_bow_*).
//
// Mirrors, for PL-SLAM's Vocabulary = DBoW2::TemplatedVocabulary<FORB::TDescriptor, FORB> with L1 scoring:
//   void Vocabulary::transform(const std::vector<cv::Mat>& features, BowVector& v) const
//        3rdparty/DBoW2/include/DBoW2/TemplatedVocabulary.h:1046-1100
//   double Vocabulary::score(const BowVector& v1, const BowVector& v2) const   -> L1Scoring::score, ScoringObject.cpp:23-67
//   MapHandler::insertKFBowVector{P,L,PL}(KeyFrame*)   src/mapHandler.cpp:3007-3128 (conf_matrix filled symmetrically)
//   void Vocabulary::create(const std::vector<std::vector<cv::Mat>>& training_features, int k, int L, WeightingType, ScoringType)
//        TemplatedVocabulary.h:536-976 -> PlslamBow::train (include/plslam_bow_train.h: the three departures from create)
// The BowVector is a template argument: DBoW2::BowVector (a std::map<WordId, WordValue>) or any map with clear() and
// operator[] works unchanged.  Descriptor blocks are templates too (cv::Mat or StVO::DescMat: rows, ptr<uchar>(), continuous
// N x 32 rows).  Header-only; link with libplslam_hip.so.  Errors throw std::runtime_error.
#pragma once

#include <stdint.h>

#include <cmath>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "plslam_bow_train.h"
#include "plslam_hip.h"

namespace PlslamBow {

inline void check(int rc, const char* where)
{
    if (rc != PLSLAM_OK)
        throw std::runtime_error(std::string(where) + ": " + plslam_strerror(rc) + "; " + plslam_last_error());
}

class Vocabulary {
public:
    // desc: the records of TemplatedVocabulary::load (plslam_bow_vocab_desc); copied to the device
    Vocabulary(plslam_ctx* ctx, const plslam_bow_vocab_desc& desc) { check(plslam_bow_vocab_create(ctx, &desc, &v_), "plslam_bow_vocab_create"); }
    ~Vocabulary() { plslam_bow_vocab_destroy(v_); }
    Vocabulary(const Vocabulary&) = delete;
    Vocabulary& operator=(const Vocabulary&) = delete;
    plslam_bow_vocab* handle() const { return v_; }

    // TemplatedVocabulary::transform(features, v): one descriptor row per element (FORB::TDescriptor = a 1 x 32 CV_8U Mat)
    template <class Mat, class BowVector>
    void transform(const std::vector<Mat>& features, BowVector& v) const
    {
        v.clear();
        const int32_t n = (int32_t)features.size();
        buf_.resize((size_t)n * PLSLAM_DESC_BYTES);
        for (int32_t i = 0; i < n; ++i)
            std::memcpy(&buf_[(size_t)i * PLSLAM_DESC_BYTES], features[i].template ptr<uint8_t>(), PLSLAM_DESC_BYTES);
        transform_rows(buf_.data(), n, v);
    }

    // the same for a contiguous N x 32 block (what insertKFBowVector* split into rows, mapHandler.cpp:3010-3013)
    template <class BowVector>
    void transform_rows(const uint8_t* rows, int32_t n, BowVector& v) const
    {
        v.clear();
        const int32_t off[2] = {0, n};
        words_.resize((size_t)n + 1);
        weights_.resize((size_t)n + 1);
        int32_t len = 0;
        check(plslam_bow_transform(v_, rows, off, 1, nullptr, nullptr, words_.data(), weights_.data(), &len), "plslam_bow_transform");
        for (int32_t j = 0; j < len; ++j) v[words_[j]] = weights_[j];
    }

    // L1Scoring::score(v1, v2) of one pair: the reference's walk over the common words (ScoringObject.cpp:23-67).  The
    // confusion-matrix rows themselves are computed on the device (KFBowDatabase).
    template <class BowVector>
    static double score(const BowVector& v1, const BowVector& v2)
    {
        auto a = v1.begin(), b = v2.begin();
        double s = 0;
        while (a != v1.end() && b != v2.end()) {
            if (a->first == b->first) {
                const double vi = a->second, wi = b->second;
                s += std::fabs(vi - wi) - std::fabs(vi) - std::fabs(wi);
                ++a;
                ++b;
            } else if (a->first < b->first) {
                a = v1.lower_bound(b->first);
            } else {
                b = v2.lower_bound(a->first);
            }
        }
        s = -s / 2.0;
        return s;
    }

private:
    plslam_bow_vocab* v_ = nullptr;
    mutable std::vector<uint8_t> buf_;
    mutable std::vector<int32_t> words_;
    mutable std::vector<double> weights_;
};

// A trained vocabulary: the records of TemplatedVocabulary::save in ascending node id.  desc() is what Vocabulary is
// constructed from (valid as long as this object is).
struct Trained {
    int32_t k = 0, L = 0, weighting = 0;
    std::vector<plslam_bow_node> nodes;
    std::vector<plslam_bow_word> words;
    plslam_bow_train_stats stats{};
    plslam_bow_vocab_desc desc() const
    {
        return plslam_bow_vocab_desc{k, L, PLSLAM_BOW_L1_NORM, weighting, (int32_t)nodes.size(), (int32_t)words.size(), nodes.data(), words.data()};
    }
};

// TemplatedVocabulary::create(training_features, k, L, weighting, L1_NORM) on the device.  rows: the documents' descriptors
// one after the other (N x 32 bytes); doc_offsets: n_docs + 1 row offsets from 0.  max_iters = 0: the default cap.
inline Trained train(plslam_ctx* ctx, const uint8_t* rows, const int32_t* doc_offsets, int32_t n_docs, int32_t k, int32_t L,
                     int32_t weighting, uint64_t seed, int32_t max_iters = 0)
{
    const plslam_bow_train_params prm{k, L, weighting, PLSLAM_BOW_L1_NORM, seed, max_iters, 0};
    plslam_bow_trainer* t = nullptr;
    check(plslam_bow_train_create(ctx, &prm, rows, doc_offsets, n_docs, &t), "plslam_bow_train_create");
    Trained out;
    out.k = k;
    out.L = L;
    out.weighting = weighting;
    int rc = plslam_bow_train_run(t, &out.stats);
    if (rc == PLSLAM_OK) {
        out.nodes.resize((size_t)out.stats.n_nodes);
        out.words.resize((size_t)out.stats.n_words);
        rc = plslam_bow_train_export(t, out.nodes.data(), out.words.data());
    }
    plslam_bow_train_destroy(t);
    check(rc, "plslam_bow_train_run");
    return out;
}

// the same over one vector of descriptor rows per document (cv::Mat or any type with ptr<uint8_t>())
template <class Mat>
inline Trained train(plslam_ctx* ctx, const std::vector<std::vector<Mat>>& training_features, int32_t k, int32_t L, int32_t weighting,
                     uint64_t seed, int32_t max_iters = 0)
{
    std::vector<uint8_t> rows;
    std::vector<int32_t> off(1, 0);
    for (const auto& doc : training_features) {
        for (const Mat& f : doc) rows.insert(rows.end(), f.template ptr<uint8_t>(), f.template ptr<uint8_t>() + PLSLAM_DESC_BYTES);
        off.push_back((int32_t)(rows.size() / PLSLAM_DESC_BYTES));
    }
    return train(ctx, rows.data(), off.data(), (int32_t)training_features.size(), k, L, weighting, seed, max_iters);
}

// MapHandler's keyframe BowVectors + conf_matrix rows (src/mapHandler.cpp:3007-3128) on the device.  vocab_p or vocab_l may
// be null: the mode of mapHandler.cpp:196-201.  The vocabularies must outlive the database.
class KFBowDatabase {
public:
    KFBowDatabase(plslam_ctx* ctx, const Vocabulary* vocab_p, const Vocabulary* vocab_l, int capacity_hint = 0)
    {
        check(plslam_bow_db_create(ctx, vocab_p ? vocab_p->handle() : nullptr, vocab_l ? vocab_l->handle() : nullptr,
                                   capacity_hint, &db_),
              "plslam_bow_db_create");
    }
    ~KFBowDatabase() { plslam_bow_db_destroy(db_); }
    KFBowDatabase(const KFBowDatabase&) = delete;
    KFBowDatabase& operator=(const KFBowDatabase&) = delete;
    plslam_bow_db* handle() const { return db_; }

    // insertKFBowVectorP(kf): pdesc_l = kf->stereo_frame->pdesc_l; map_keyframes[i] != NULL marks the live keyframes
    template <class Mat, class KeyFrames>
    void insertKFBowVectorP(int kf_idx, const Mat& pdesc_l, const KeyFrames& map_keyframes,
                            std::vector<std::vector<double>>& conf_matrix)
    {
        insert(kf_idx, &pdesc_l, (const Mat*)nullptr, nullptr, map_keyframes, conf_matrix);
    }
    template <class Mat, class KeyFrames>
    void insertKFBowVectorL(int kf_idx, const Mat& ldesc_l, const KeyFrames& map_keyframes,
                            std::vector<std::vector<double>>& conf_matrix)
    {
        insert(kf_idx, (const Mat*)nullptr, &ldesc_l, nullptr, map_keyframes, conf_matrix);
    }
    // insertKFBowVectorPL(kf): n_pt / n_ls = the stereo feature counts, std_pt / std_ls = vector_stdv(x) + vector_stdv(y) of
    // their image positions (mapHandler.cpp:3063-3091; vector_stdv is stvo-pl's)
    template <class Mat, class KeyFrames>
    void insertKFBowVectorPL(int kf_idx, const Mat& pdesc_l, const Mat& ldesc_l, int n_pt, int n_ls, double std_pt,
                             double std_ls, const KeyFrames& map_keyframes, std::vector<std::vector<double>>& conf_matrix)
    {
        const plslam_bow_pl_stats st{n_pt, n_ls, std_pt, std_ls};
        insert(kf_idx, &pdesc_l, &ldesc_l, &st, map_keyframes, conf_matrix);
    }

private:
    template <class Mat, class KeyFrames>
    void insert(int kf_idx, const Mat* p, const Mat* l, const plslam_bow_pl_stats* st, const KeyFrames& map_keyframes,
                std::vector<std::vector<double>>& conf_matrix)
    {
        if (kf_idx < 0 || (size_t)kf_idx >= conf_matrix.size()) throw std::runtime_error("insertKFBowVector: kf_idx outside conf_matrix");
        alive_.assign((size_t)kf_idx + 1, 0);
        for (int i = 0; i < kf_idx; ++i) alive_[i] = map_keyframes[i] != nullptr;
        row_.resize((size_t)kf_idx + 1);
        for (int i = 0; i <= kf_idx; ++i) row_[i] = conf_matrix[kf_idx][i];
        check(plslam_bow_db_insert(db_, kf_idx, p ? p->template ptr<uint8_t>() : nullptr, p ? (int32_t)p->rows : 0,
                                   l ? l->template ptr<uint8_t>() : nullptr, l ? (int32_t)l->rows : 0, st, alive_.data(),
                                   row_.data()),
              "plslam_bow_db_insert");
        for (int i = 0; i < kf_idx; ++i)
            if (alive_[i]) {                                   // conf_matrix[idx][i] = conf_matrix[i][idx] = score
                conf_matrix[kf_idx][i] = row_[i];
                conf_matrix[i][kf_idx] = row_[i];
            }
        conf_matrix[kf_idx][kf_idx] = row_[kf_idx];
    }

    plslam_bow_db* db_ = nullptr;
    std::vector<uint8_t> alive_;
    std::vector<double> row_;
};

}  // namespace PlslamBow
