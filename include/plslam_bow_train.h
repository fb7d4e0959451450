/* plslam_bow_train.h -- training a DBoW2 vocabulary on the device: TemplatedVocabulary::create's hierarchical k-means++
 * (3rdparty/DBoW2/include/DBoW2/TemplatedVocabulary.h:536-976) over 256-bit descriptors, one whole tree level per pass.
 * Part of libplslam_hip.so; the records it exports (plslam_bow_node, plslam_bow_word) are plslam_hip.h's and feed
 * plslam_bow_vocab_create as they stand.
 *
 * The tree, the partition, the tie rules, the node and word ids and the weights are the reference's.  Three departures
 * ("Training a vocabulary"):
 *   1. every random draw is a function of (seed, node path, centre index, retry) -- plslam_amd/csrc/bow_train_draw.h -- not
 *      the next value of one rand() stream;
 *   2. a group that is empty when the centres are recomputed keeps its centre (the reference reads a released matrix);
 *   3. a node runs at most max_iters rounds (the seeding pass included) and then keeps its last centres and assignment.
 * The same arguments give the same bytes on every run. */
#ifndef PLSLAM_BOW_TRAIN_H
#define PLSLAM_BOW_TRAIN_H

#include "plslam_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct plslam_bow_trainer plslam_bow_trainer;

#define PLSLAM_BOW_TRAIN_MAX_N 16777216 /* descriptors of one training set (2^24) */
#define PLSLAM_BOW_TRAIN_MAX_K 256      /* branching factor */
#define PLSLAM_BOW_TRAIN_MAX_L 16       /* depth */
#define PLSLAM_BOW_TRAIN_DEFAULT_MAX_ITERS 1000

typedef struct plslam_bow_train_params {
    int32_t k;              /* >= 2 */
    int32_t L;              /* >= 1 */
    int32_t weighting_type; /* PLSLAM_BOW_TF_IDF .. PLSLAM_BOW_BINARY */
    int32_t scoring_type;   /* PLSLAM_BOW_L1_NORM; any other: PLSLAM_ENOTSUP */
    uint64_t seed;
    int32_t max_iters;      /* rounds per node; 0 = PLSLAM_BOW_TRAIN_DEFAULT_MAX_ITERS */
    int32_t reserved;       /* 0 */
} plslam_bow_train_params;

typedef struct plslam_bow_train_stats {
    int32_t n_nodes;          /* without the root */
    int32_t n_words;
    int64_t lloyd_rounds;     /* over all nodes that ran k-means */
    int64_t empty_groups;     /* departure 2: (node, round, cluster) triples whose group was empty at a recomputation */
    int64_t capped_nodes;     /* departure 3 */
    int32_t lloyd_rounds_max; /* the most rounds of one node */
    int32_t levels;           /* tree levels that were clustered */
} plslam_bow_train_stats;

/* desc: n_total x 32 bytes, document d owns rows [doc_offsets[d], doc_offsets[d + 1]); doc_offsets: n_docs + 1 entries from 0,
 * not decreasing; empty documents are allowed and count in NDocs.  Host memory, copied.
 * EINVAL: a NULL argument, k < 2, L < 1, a weighting out of range, max_iters < 0, n_docs < 1, offsets that do not start at 0 or
 *         decrease, no descriptor at all (N = 0);
 * ENOTSUP: a scoring other than L1;  ERANGE: N > PLSLAM_BOW_TRAIN_MAX_N, k > PLSLAM_BOW_TRAIN_MAX_K, L > PLSLAM_BOW_TRAIN_MAX_L,
 *         or a level's centre table of 2^31 entries or more.
 * A failed create frees what it allocated and leaves *out NULL. */
int plslam_bow_train_create(plslam_ctx* ctx, const plslam_bow_train_params* params, const uint8_t* desc,
                            const int32_t* doc_offsets, int32_t n_docs, plslam_bow_trainer** out);
/* The same over device memory that stays where it is (desc 16-byte aligned, both valid until the trainer is destroyed);
 * n_total = doc_offsets[n_docs], stated by the caller: nothing is read through the pointers by the host. */
int plslam_bow_train_create_dev(plslam_ctx* ctx, const plslam_bow_train_params* params, const uint8_t* desc,
                                const int32_t* doc_offsets, int32_t n_docs, int32_t n_total, plslam_bow_trainer** out);
/* Trains on the context's stream and waits; stats may be NULL.  Running a trainer again repeats the training. */
int plslam_bow_train_run(plslam_bow_trainer* t, plslam_bow_train_stats* stats);
/* The counts of the last run (EINVAL before the first). */
int plslam_bow_train_sizes(plslam_bow_trainer* t, int32_t* n_nodes, int32_t* n_words);
/* nodes: n_nodes records in ascending node id (DBoW2's creation order), without the root; words: n_words records in ascending
 * word id.  Together with k, L, the weighting and the scoring they are a plslam_bow_vocab_desc. */
int plslam_bow_train_export(plslam_bow_trainer* t, plslam_bow_node* nodes, plslam_bow_word* words);
/* Per training descriptor (n_total entries each, either may be NULL): the node id of the leaf the training partition left it
 * in, and the word id TemplatedVocabulary::transform gives it in the finished tree. */
int plslam_bow_train_download(plslam_bow_trainer* t, int32_t* leaf_node, int32_t* word);
void plslam_bow_train_destroy(plslam_bow_trainer* t);

#ifdef __cplusplus
}
#endif

#endif /* PLSLAM_BOW_TRAIN_H */
