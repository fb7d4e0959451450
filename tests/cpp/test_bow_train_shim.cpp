// Client of PlslamBow::train (plslam_amd/host/dbow_voc.hpp): reads a fixture written by tests/test_gpu_bow_train_shim.py --
// int32 {k, L, weighting, max_iters, n_docs}, uint64 seed, n_docs + 1 int32 offsets, N x 32 descriptor bytes --, trains both
// through the flat rows and through per-document vectors of rows, builds a PlslamBow::Vocabulary from the result, and writes
// int64 {n_nodes, n_words, rounds, rounds_max, empty, capped}, the node records and the word records for the test to compare.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../plslam_amd/host/dbow_voc.hpp"

struct Row {                                   // what the shim asks of a descriptor row: ptr<uint8_t>()
    const uint8_t* p;
    template <class T> const T* ptr() const { return reinterpret_cast<const T*>(p); }
};

int main(int argc, char** argv)
{
    if (argc < 3) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t head[5];
    uint64_t seed;
    if (std::fread(head, 4, 5, f) != 5 || std::fread(&seed, 8, 1, f) != 1) return 2;
    const int32_t k = head[0], L = head[1], weighting = head[2], max_iters = head[3], n_docs = head[4];
    std::vector<int32_t> off((size_t)n_docs + 1);
    if (std::fread(off.data(), 4, off.size(), f) != off.size()) return 2;
    std::vector<uint8_t> rows((size_t)off.back() * 32);
    if (std::fread(rows.data(), 1, rows.size(), f) != rows.size()) return 2;
    std::fclose(f);
    plslam_ctx* ctx = nullptr;
    if (plslam_ctx_create(0, &ctx) != PLSLAM_OK) { std::printf("no context: %s\n", plslam_last_error()); return 1; }
    int bad = 0;
    try {
        const PlslamBow::Trained a = PlslamBow::train(ctx, rows.data(), off.data(), n_docs, k, L, weighting, seed, max_iters);
        std::vector<std::vector<Row>> docs((size_t)n_docs);
        for (int32_t d = 0; d < n_docs; ++d)
            for (int32_t i = off[d]; i < off[d + 1]; ++i) docs[(size_t)d].push_back(Row{rows.data() + (size_t)i * 32});
        const PlslamBow::Trained b = PlslamBow::train(ctx, docs, k, L, weighting, seed, max_iters);
        if (a.nodes.size() != b.nodes.size() || a.words.size() != b.words.size() ||
            std::memcmp(a.nodes.data(), b.nodes.data(), a.nodes.size() * sizeof(plslam_bow_node)) ||
            std::memcmp(a.words.data(), b.words.data(), a.words.size() * sizeof(plslam_bow_word))) {
            std::printf("FAIL the two forms of train differ\n");
            bad = 1;
        }
        {
            PlslamBow::Vocabulary voc(ctx, a.desc());              // the result is what a Vocabulary is constructed from
            if (!voc.handle()) bad = 1;
        }
        FILE* o = std::fopen(argv[2], "wb");
        if (!o) return 2;
        const int64_t st[6] = {a.stats.n_nodes, a.stats.n_words, a.stats.lloyd_rounds, a.stats.lloyd_rounds_max, a.stats.empty_groups,
                               a.stats.capped_nodes};
        std::fwrite(st, 8, 6, o);
        std::fwrite(a.nodes.data(), sizeof(plslam_bow_node), a.nodes.size(), o);
        std::fwrite(a.words.data(), sizeof(plslam_bow_word), a.words.size(), o);
        std::fclose(o);
    } catch (const std::exception& e) {
        std::printf("FAIL %s\n", e.what());
        bad = 1;
    }
    plslam_ctx_destroy(ctx);
    if (!bad) std::printf("all checks passed\n");
    return bad;
}
