// The arithmetic of the windowed matcher (plslam_amd/csrc/match_grid_layout.hpp) on the CPU: no device, no HIP header, no
// library.  Every expected value is a literal worked out by hand from the kernels' carving and comments (the sums are written
// out beside them), never the function under test called a second way.
// Prints "PASS <case>" or "FAIL <case>: <what>" per case; exit status 1 when any failed.
//   g++ -std=c++17 -I plslam_amd/csrc tests/cpp/test_grid_layout.cpp
#include <cstdio>
#include <functional>
#include <string>
#include <vector>

#include "match_grid_layout.hpp"

using namespace plslam;

namespace {

std::string g_fail;     // first failure of the running case
void fail(const char* what, int line)
{
    if (g_fail.empty()) g_fail = std::string(what) + " (line " + std::to_string(line) + ")";
}
#define CHECK(cond)                          \
    do {                                     \
        if (!(cond)) fail(#cond, __LINE__);  \
    } while (0)

int n_failed = 0;
void run(const char* name, const std::function<void()>& body)
{
    g_fail.clear();
    body();
    if (g_fail.empty()) std::printf("PASS %s\n", name);
    else { std::printf("FAIL %s: %s\n", name, g_fail.c_str()); ++n_failed; }
}

// k_grid_records' own test of the packed word, on the clz form of the column bits (match_grid_listers.hip)
bool flat_as_records(int mutual, int32_t n1, int32_t n2)
{
    const uint32_t fb2 = grid_col_bits_clz(n2), fb1 = grid_row_bits(fb2);
    return mutual && fb2 <= 22u && (uint32_t)n1 <= (1u << fb1);
}

GridShape shape(int32_t n1, int32_t n2, int32_t cols, int32_t rows, int32_t n_items, int32_t n_centres, int32_t wx0, int32_t wx1,
                int mutual, bool dirs, int32_t pair_capacity)
{
    GridShape s{};
    s.n1 = n1; s.n2 = n2; s.cols = cols; s.rows = rows; s.n_items = n_items; s.n_centres = n_centres;
    s.window[0] = wx0; s.window[1] = wx1; s.window[2] = 3; s.window[3] = 3;
    s.mutual = mutual; s.dirs = dirs; s.pair_capacity = pair_capacity;
    return s;
}

}  // namespace

int main()
{
    run("flat_bits", [] {
        // the two forms of a column number's bits, exhaustively: the loop stops at 22, where the clz form goes on -- and the
        // tests built on them (n2 <= 1 << fb2 on the loop form, fb2 <= 22 on the clz form) say the same of every n2
        for (uint32_t n2 = 1; n2 <= (1u << 23) + 1u && g_fail.empty(); ++n2) {
            const uint32_t a = grid_col_bits(n2), b = grid_col_bits_clz((int32_t)n2);
            CHECK((b < 22u ? b : 22u) == a);
            CHECK(n2 > (1u << 22) || a == b);
            CHECK((n2 <= (1u << a)) == (b <= 22u));
        }
        const struct { int32_t n2; uint32_t bits; } want[] = {{1, 1}, {2, 1}, {3, 2}, {4, 2}, {5, 3}, {8, 3}, {9, 4}, {1024, 10},
                                                              {1025, 11}, {2048, 11}, {2049, 12}, {1 << 22, 22}};
        for (const auto& w : want) CHECK(grid_col_bits((uint32_t)w.n2) == w.bits && grid_col_bits_clz(w.n2) == w.bits);
        CHECK(grid_col_bits((1u << 22) + 1u) == 22 && grid_col_bits_clz((1 << 22) + 1) == 23);
        // the row bits: what is left of 23, at most 14
        CHECK(grid_row_bits(1) == 14 && grid_row_bits(8) == 14 && grid_row_bits(9) == 14 && grid_row_bits(10) == 13);
        CHECK(grid_row_bits(11) == 12 && grid_row_bits(22) == 1);
        // flat flips at n1 = 2^fb1 -> + 1: 1500 columns are 11 bits, 12 are left; 100 columns are 7 bits, the cap of 14 holds
        CHECK(grid_flat(1, 4096, 1500) && !grid_flat(1, 4097, 1500));
        CHECK(grid_flat(1, 16384, 100) && !grid_flat(1, 16385, 100));
        // ... and at n2 = 2^22 -> + 1 (one bit is left for the rows: two of them)
        CHECK(grid_flat(1, 2, 1 << 22) && !grid_flat(1, 3, 1 << 22) && !grid_flat(1, 1, (1 << 22) + 1));
        // the records kernel's test agrees on both sides of every flip
        const int32_t n2s[] = {1, 2, 100, 511, 512, 513, 1500, 2048, 2049, 1 << 21, (1 << 21) + 1, 1 << 22, (1 << 22) + 1, 1 << 23};
        const int32_t n1s[] = {0, 1, 2, 3, 4, 5, 2048, 4096, 4097, 8192, 8193, 16384, 16385};
        for (int32_t n2 : n2s)
            for (int32_t n1 : n1s) CHECK(grid_flat(1, n1, n2) == flat_as_records(1, n1, n2));
        // a problem without bestLRMatches is never flat
        CHECK(!grid_flat(0, 1, 1) && !grid_flat(0, 100, 100) && !flat_as_records(0, 100, 100));
    });

    run("scratch_layout", [] {
        // tables in LDS: 64 x 48 cells + 1, 2 x 1500 + 2 x 1500 words = 9073 words = 36 292 bytes of 147 456
        CHECK(grid_fits_lds(1500, 1500, 3072));
        GridScratch<size_t> l = grid_scratch(1500, 1500, 3072, 5000);
        CHECK(l.tables == 0 && l.rcnt == 0 && l.round_k == 1500 && l.store == 1502 && l.listed == 6502 && l.total == 11502);
        CHECK(l.total == 1500 + 2 + 2 * 5000 && l.listed == l.store + 5000);
        CHECK(grid_scratch_words(1500, 1500, 3072, 5000) == 11502);
        // tables in scratch: 3073 + 18000 + 20000 = 41073 words > 36864; 10 rounds of 1024 rows
        CHECK(!grid_fits_lds(10000, 9000, 3072));
        l = grid_scratch(10000, 9000, 3072, 7);
        CHECK(l.tables == 0 && l.rcnt == 38000 && l.round_k == 48000 && l.store == 48010 && l.listed == 48017 && l.total == 48024);
        CHECK(l.total == 38000 + 10000 + 10 + 2 * 7 && l.listed == l.store + 7);
        CHECK(l.tables <= l.rcnt && l.rcnt < l.round_k && l.round_k < l.store && l.store < l.listed && l.listed < l.total);
        // tables appear exactly when the fixed words do not fit: 3072 + 2 x 16896 = 36864 words fit, two words more do not
        CHECK(grid_fits_lds(8448, 8448, 3071) && grid_scratch(8448, 8448, 3071, 1).rcnt == 0);
        CHECK(!grid_fits_lds(8449, 8448, 3071) && grid_scratch(8449, 8448, 3071, 1).rcnt == 2 * 8448 + 2 * 8449);
        // rounds of 256 rows and of 1024 are the same count -- one -- for what the 256-lane workgroups take: they share the layout
        for (int32_t n1 = 0; n1 <= GRID_SMALL_ROWS; ++n1) {
            CHECK((n1 + 255) / 256 == (n1 + 1023) / 1024);
            const GridScratch<size_t> a = grid_scratch_carve(size_t(0), size_t(0), n1, 77), b = grid_scratch_carve(size_t(0), size_t(0), n1, 77, 256);
            CHECK(a.round_k == b.round_k && a.store == b.store && a.listed == b.listed && a.total == b.total);
        }
        CHECK((257 + 255) / 256 == 2 && (257 + 1023) / 1024 == 1);
        // carved from a pointer (the kernels): the same places
        std::vector<uint32_t> buf(11502);
        const GridScratch<uint32_t*> p = grid_scratch_carve(buf.data(), 0, 1500, 5000);
        CHECK(p.tables == buf.data() && p.rcnt == buf.data() && p.round_k - buf.data() == 1500 && p.store - buf.data() == 1502);
        CHECK(p.listed - buf.data() == 6502 && p.total - buf.data() == 11502);
    });

    run("lds_mode2", [] {
        // n1 = 10, n2 = 7, 5 cells: the tables are 6 + 14 + 20 = 40 words, the cell_start copy behind the 34 column / row words;
        // desc2 rows 8 x 7 = 56 words, directions 4 x 7 = 28, colbest 7
        const struct { int32_t n_items; size_t d2_off; } want[] = {{0, 40}, {1, 44}, {3, 44}, {4, 44}, {5, 48}};
        for (const auto& w : want) {
            const GridLds2<size_t> l = grid_lds2<size_t>(10, 7, 5, (size_t)w.n_items);
            CHECK(l.cs == 34 && l.items_off == 40 && l.d2_off == w.d2_off && l.dir2 == w.d2_off + 56);
            CHECK(l.colbest(false) == w.d2_off + 56 && l.end(false) == w.d2_off + 63);
            CHECK(l.colbest(true) == w.d2_off + 84 && l.end(true) == w.d2_off + 91);
            CHECK(l.items_off % 4 == 0 && l.d2_off % 4 == 0 && (l.dir2 * 4) % 8 == 0);
            CHECK(grid_lds_bytes(2, 10, 7, 5, w.n_items, false) == 4 * (w.d2_off + 63));
            CHECK(grid_lds_bytes(2, 10, 7, 5, w.n_items, true) == 4 * (w.d2_off + 91));
            const GridLds2<uint32_t> k = grid_lds2<uint32_t>(10, 7, 5u, (uint32_t)w.n_items);      // the kernel's width
            CHECK(k.cs == l.cs && k.items_off == l.items_off && k.d2_off == l.d2_off && k.dir2 == l.dir2 && k.end(true) == l.end(true));
        }
        CHECK(grid_lds_bytes(2, 10, 7, 5, 0, false) == 412 && grid_lds_bytes(2, 10, 7, 5, 5, true) == 556);
        // 6 cells: 41 words of tables, the items at 44; 5 items: desc2 rows at (44 + 5 + 3) & ~3 = 52
        const GridLds2<size_t> l = grid_lds2<size_t>(10, 7, 6, 5);
        CHECK(l.items_off == 44 && l.d2_off == 52 && l.dir2 == 108 && l.colbest(true) == 136 && l.end(true) == 143 && l.end(false) == 115);
        CHECK(grid_lds_bytes(2, 10, 7, 6, 5, true) == 572 && grid_lds_bytes(2, 10, 7, 6, 5, false) == 460);
        CHECK(grid_lds_bytes(1, 10, 7, 6, 5, true) == 164 && grid_lds_bytes(0, 10, 7, 6, 5, true) == 0 && grid_fixed_words(10, 7, 6) == 41);
    });

    run("modes_and_groups", [] {
        // GRID_LDS_MAX_BYTES = 38912 words.  Tables of 7072 words (a multiple of 4), n_items a multiple of 4, no directions:
        // end = 7072 + n_items + 9 n2
        CHECK(GRID_LDS_MAX_BYTES == 38912 * 4 && GRID_LDS_FIXED_MAX_BYTES == 36864 * 4);
        CHECK(grid_fixed_words(1000, 999, 3073) == 7072 && grid_fixed_words(1000, 1000, 3071) == 7072 && grid_fixed_words(1000, 1001, 3069) == 7072);
        CHECK(grid_lds_bytes(2, 1000, 999, 3073, 22848, false) == 38911 * 4 && grid_mode(1000, 999, 3073, 22848, false) == 2);
        CHECK(grid_lds_bytes(2, 1000, 1000, 3071, 22840, false) == 38912 * 4 && grid_mode(1000, 1000, 3071, 22840, false) == 2);
        CHECK(grid_lds_bytes(2, 1000, 1001, 3069, 22832, false) == 38913 * 4 && grid_mode(1000, 1001, 3069, 22832, false) == 1);
        // GRID_LDS_FIXED_MAX_BYTES = 36864 words = cells + 1 + 2 x 16896
        CHECK(grid_mode(8448, 8448, 3070, 100, false) == 1 && grid_mode(8448, 8448, 3071, 100, false) == 1 && grid_mode(8448, 8448, 3072, 100, false) == 0);
        // the 256-lane group
        CHECK(grid_group(256, 100, 12, 50, false) == 3 && grid_group(257, 100, 12, 50, false) == 2);
        CHECK(grid_group(1000, 1001, 3069, 22832, false) == 1 && grid_group(8448, 8448, 3072, 100, false) == 0);
        // group 3 asks for its mode-2 bytes + 4 (2 n1 + 1 + 64 n1), rounded up to 4096, at most the maximum
        CHECK(grid_group_lds_bytes(3, 10, 7, 6, 5, true) == 4096);                       // 572 + 2644 = 3216
        // 200 x 200 lines on 64 x 48 cells, 200 items: tables 3873 -> items at 3876, desc2 rows at 4076, end 4076 + 1600 + 800 + 200
        CHECK(grid_lds_bytes(2, 200, 200, 3072, 200, true) == 26704);
        CHECK(grid_group_lds_bytes(3, 200, 200, 3072, 200, true) == 81920);              // 26704 + 52804 = 79508 -> 20 x 4096
        // 256 x 2000: tables 7585 -> 7588, rows at 9588, end 27588 words = 110352 bytes; + 67588 is over the maximum
        CHECK(grid_group(256, 2000, 3072, 2000, false) == 3 && grid_lds_bytes(2, 256, 2000, 3072, 2000, false) == 110352);
        CHECK(grid_group_lds_bytes(3, 256, 2000, 3072, 2000, false) == 155648);
        CHECK(grid_group_lds_bytes(2, 10, 7, 6, 5, true) == 155648 && grid_group_lds_bytes(2, 1500, 1500, 3072, 1500, false) == 155648);
        CHECK(grid_group_lds_bytes(1, 10, 7, 6, 5, true) == 164 && grid_group_lds_bytes(0, 10, 7, 6, 5, true) == 0);
    });

    run("dense_layout", [] {
        // d1 8 n1 | d2 8 n2 | member 8 n1 | live 8 n1 | any n1 | memberT 8 n2 | m21 n2 | centres 2 nc n1 | R | 2 (| dirs 4 n1 + 4 n2)
        // the grid is the largest life: 3073 + 400 against 13 x 200 and 16 x 200
        CHECK(dense_region_words(200, 200, 3072, 400) == 3473);
        CHECK(grid_dense_lds_bytes(200, 200, 3072, 400, true, 2) == 4 * (1600 + 1600 + 1600 + 1600 + 200 + 1600 + 200 + 800 + 3473 + 2 + 1600));
        CHECK(grid_dense_lds_bytes(200, 200, 3072, 400, true, 2) == 57100);
        // the chunk minima are: 16 chunks x 256 columns against 16 x 250 and 101 + 50
        CHECK(dense_region_words(250, 256, 100, 50) == 4096);
        CHECK(grid_dense_lds_bytes(250, 256, 100, 50, false, 1) == 4 * (2000 + 2048 + 2000 + 2000 + 250 + 2048 + 256 + 500 + 4096 + 2));
        CHECK(grid_dense_lds_bytes(250, 256, 100, 50, false, 1) == 60800);
        // the rows' best pairs are: 16 x 100 against 7 x 10 and 21 + 5
        CHECK(dense_region_words(100, 10, 20, 5) == 1600);
        CHECK(grid_dense_lds_bytes(100, 10, 20, 5, false, 4) == 4 * (800 + 80 + 800 + 800 + 100 + 80 + 10 + 800 + 1600 + 2));
        CHECK(grid_dense_lds_bytes(100, 10, 20, 5, false, 4) == 20288);
        // the size test
        CHECK(grid_dense_fits(256, 10, 20, 5, false, 1) && !grid_dense_fits(257, 10, 20, 5, false, 1) && !grid_dense_fits(0, 10, 20, 5, false, 1));
        CHECK(grid_dense_fits(10, 256, 20, 5, false, 1) && !grid_dense_fits(10, 257, 20, 5, false, 1) && !grid_dense_fits(10, 0, 20, 5, false, 1));
        CHECK(!grid_dense_fits(10, 10, 20, 5, false, 0) && grid_dense_fits(10, 10, 20, 5, false, 1) && grid_dense_fits(10, 10, 20, 5, false, 4) &&
              !grid_dense_fits(10, 10, 20, 5, false, 5));
        // 128 KB = 32768 words = 29 x 256 + 17 x 256 + 2 + R: R = 20990 = 3073 + 17917 items
        CHECK(DENSE_LDS_MAX_BYTES == 32768 * 4);
        CHECK(grid_dense_lds_bytes(256, 256, 3072, 17917, false, 2) == 131072 && grid_dense_fits(256, 256, 3072, 17917, false, 2));
        CHECK(grid_dense_lds_bytes(256, 256, 3072, 17918, false, 2) == 131076 && !grid_dense_fits(256, 256, 3072, 17918, false, 2));
    });

    run("store_capacity", [] {
        {   // 3 x 2 cells (id = x * 2 + y) holding 1 2 | 0 3 | 1 1 items; windows x +- 1, y exact; one centre a row
            const int32_t cs[] = {0, 1, 3, 3, 6, 7, 8}, win[4] = {1, 1, 0, 0};
            const int32_t cen[] = {0, 0, 1, 1, 2, 1};
            // row 0 at (0, 0), clamped at the left border: cells (0, 0) (1, 0) = 1 + 0; row 1 at (1, 1): 2 + 3 + 1; row 2 at
            // (2, 1), clamped at the right border: 3 + 1.  One block of rows, its fullest row has 6
            CHECK(grid_store_capacity_host(cen, 3, 1, cs, 3, 2, win, 1) == 6 * 1024);
            CHECK(grid_store_capacity_host(cen, 1, 1, cs, 3, 2, win, 1) == 1 * 1024 && grid_store_capacity_host(cen + 4, 1, 1, cs, 3, 2, win, 1) == 4 * 1024);
            // the bound: fullest cell 3 x 3 x 1 cells of a window = 9, at most the 8 items
            CHECK(grid_store_capacity_bound(3, 1, cs, 3, 2, win, 1) == 8 * 1024);
            CHECK(grid_store_capacity_host(cen, 3, 1, cs, 3, 2, win, 0) == 0 && grid_store_capacity_bound(3, 1, cs, 3, 2, win, 0) == 0);
            CHECK(grid_store_capacity_bound(0, 1, cs, 3, 2, win, 1) == 0);
        }
        {   // 2 x 3 cells (id = x * 3 + y) holding 2 0 1 | 1 4 0; windows x exact, y +- 1; two centres a row; 1025 rows = 2 blocks
            const int32_t cs[] = {0, 2, 2, 3, 4, 8, 8}, win[4] = {0, 0, 1, 1};
            std::vector<int32_t> cen;
            // rows 0 .. 1023: (0, 0), clamped at the top: cells (0, 0) (0, 1) = 2, and (1, 2), clamped at the bottom: (1, 1)
            // (1, 2) = 4; row 1024: (1, 1): 1 + 4 + 0 = 5, and (0, 5), whose window lies below the grid
            for (int i = 0; i < 1024; ++i) cen.insert(cen.end(), {0, 0, 1, 2});
            cen.insert(cen.end(), {1, 1, 0, 5});
            CHECK(grid_store_capacity_host(cen.data(), 1025, 2, cs, 2, 3, win, 1) == 6 * 1024 + 5 * 1024);
            CHECK(grid_store_capacity_host(cen.data(), 1024, 2, cs, 2, 3, win, 1) == 6 * 1024);
            // the bound: fullest cell 4 x 1 x 3 cells = 12, at most the 8 items, x 2 centres, x 2 blocks
            CHECK(grid_store_capacity_bound(1025, 2, cs, 2, 3, win, 1) == 16 * 1024 * 2 && grid_store_capacity_bound(1024, 2, cs, 2, 3, win, 1) == 16 * 1024);
        }
        // the bound is one: small pseudo-random grids, centres inside and outside the grid
        uint32_t lcg = 12345u;
        auto next = [&](uint32_t n) { lcg = lcg * 1664525u + 1013904223u; return (int32_t)((lcg >> 8) % n); };
        for (int t = 0; t < 400 && g_fail.empty(); ++t) {
            const int32_t cols = 1 + next(6), rows = 1 + next(6), nc = 1 + next(2), n1 = t % 50 == 0 ? 1030 : 1 + next(40);
            std::vector<int32_t> cs(1, 0), cen;
            for (int32_t c = 0; c < cols * rows; ++c) cs.push_back(cs.back() + next(4));
            for (int32_t i = 0; i < n1 * nc; ++i) { cen.push_back(next((uint32_t)cols + 4) - 2); cen.push_back(next((uint32_t)rows + 4) - 2); }
            const int32_t win[4] = {next(3), next(3), next(3), next(3)};
            const int64_t exact = grid_store_capacity_host(cen.data(), n1, nc, cs.data(), cols, rows, win, 1);
            CHECK(exact % 1024 == 0 && exact <= (int64_t)cs.back() * nc * 1024 * ((n1 + 1023) / 1024));
            CHECK(grid_store_capacity_bound(n1, nc, cs.data(), cols, rows, win, 1) >= exact);
        }
    });

    run("route", [] {
        // a keyframe pair: 1500 x 1500 points on 64 x 48 cells, windows of 7 columns, one item per column, the store exactly
        // REC_SLOT words per item: mode 2 (24076 words of LDS), flat (11 + 12 bits) -> records on 64 x 6 groups of 8 cells
        const GridShape kf = shape(1500, 1500, 64, 48, 1500, 1, 3, 3, 1, false, 12000);
        GridRoute r = grid_route(kf, true, true, true, false);
        CHECK(r.path == GRID_PATH_RECORDS && r.group == 2 && r.n_groups == 384 && r.workgroups == 384u && r.split == 7);
        // one word less in the store: every pair is listed, 1500 x 7 tasks in workgroups of 256
        GridShape q = kf; q.pair_capacity = 11999;
        r = grid_route(q, true, true, true, false);
        CHECK(r.path == GRID_PATH_CANDIDATES && r.group == 2 && r.split == 7 && r.workgroups == 42u && r.n_groups == 384);
        q.pair_capacity = 0;
        CHECK(grid_route(q, true, true, true, false).path == GRID_PATH_SINGLE);
        // no shared words: one launch; no host descriptor: the pairs
        r = grid_route(kf, true, false, true, false);
        CHECK(r.path == GRID_PATH_SINGLE && r.group == 2);
        CHECK(grid_route(kf, true, true, false, false).path == GRID_PATH_CANDIDATES);
        // GRID_SPLIT_MIN_ROWS (the one-launch problem of 127 rows runs on 1024 lanes: 127 x 4 tasks > 256)
        q = kf; q.n1 = 127;
        r = grid_route(q, false, true, true, false);
        CHECK(r.path == GRID_PATH_SINGLE && r.group == 2);
        q.n1 = 128;
        CHECK(grid_route(q, false, true, true, false).path == GRID_PATH_RECORDS);
        // the records kernel's limits (a grid whose cell_start fits LDS has fewer groups than REC_GROUPS_MAX: the predicate alone)
        CHECK(REC_GROUPS_MAX == 65536 && REC_ROWS_MAX == 16384 && REC_SLOT == 8);
        CHECK(grid_records_ok(65536, 1500, 1500, 12000) && !grid_records_ok(65537, 1500, 1500, 12000));
        CHECK(grid_records_ok(384, 16384, 1500, 12000) && !grid_records_ok(384, 16385, 1500, 12000));
        CHECK(grid_records_ok(384, 1500, 1500, 12000) && !grid_records_ok(384, 1500, 1501, 12000) && !grid_records_ok(384, 1500, 1500, 11999));
        // REC_ROWS_MAX through the route: 16384 x 100 on 4 x 3 cells is mode 2 (33936 words) and flat (7 + 14 bits); a row more
        // is not flat -- one launch --, unless it is an upper bound: both launches, and the pairs, since the records' rows are full
        q = shape(16384, 100, 4, 3, 50, 1, 3, 3, 1, false, 400);
        CHECK(grid_mode(16384, 100, 12, 50, false) == 2 && grid_lds_bytes(2, 16384, 100, 12, 50, false) == 33936 * 4);
        CHECK(grid_route(q, true, true, true, false).path == GRID_PATH_RECORDS && grid_route(q, true, true, true, true).path == GRID_PATH_RECORDS);
        q.n1 = 16385;
        r = grid_route(q, true, true, true, false);
        CHECK(!grid_flat(1, 16385, 100) && r.path == GRID_PATH_SINGLE && r.group == 2);
        r = grid_route(q, true, true, true, true);
        CHECK(r.path == GRID_PATH_CANDIDATES && r.split == 4 && r.workgroups == 257u);      // (16385 x 4 + 255) / 256
        q.mutual = 0;
        CHECK(grid_route(q, true, true, true, true).path == GRID_PATH_SINGLE);
        // group 3 -> 2 for a lone mutual problem of more than 64 rows (64 x 4 tasks fill 256 lanes)
        q = shape(64, 100, 8, 8, 100, 1, 3, 3, 1, false, 5000);
        r = grid_route(q, false, true, true, false);
        CHECK(r.path == GRID_PATH_SINGLE && r.group == 3);
        q.n1 = 65;
        r = grid_route(q, false, true, true, false);
        CHECK(r.path == GRID_PATH_SINGLE && r.group == 2);
        q.mutual = 0;
        CHECK(grid_route(q, false, true, true, false).group == 3);
        // the 200 x 200 line problem: dense when allowed and the host has the descriptor and the row count
        q = shape(200, 200, 64, 48, 400, 2, 3, 3, 1, true, 400 * 8);
        CHECK(grid_route(q, true, true, true, false).path == GRID_PATH_DENSE && grid_route(q, true, false, true, false).path == GRID_PATH_DENSE);
        CHECK(grid_route(q, false, true, true, false).path == GRID_PATH_RECORDS);
        CHECK(grid_route(q, true, true, false, false).path == GRID_PATH_CANDIDATES);
        CHECK(grid_route(q, true, true, true, true).path == GRID_PATH_RECORDS);
        // lanes per row = the window's columns, at most the grid's 16 and GRID_SPLIT_MAX
        q = shape(1500, 1500, 16, 8, 1500, 1, 0, 0, 1, false, 12000);
        r = grid_route(q, true, true, false, false);
        CHECK(r.path == GRID_PATH_CANDIDATES && r.split == 1 && r.workgroups == 6u && r.n_groups == 16);         // 1755 / 256
        q.window[0] = q.window[1] = 2;
        r = grid_route(q, true, true, false, false);
        CHECK(r.split == 5 && r.workgroups == 30u);                                                              // 7755 / 256
        q.window[0] = 20; q.window[1] = 19;
        r = grid_route(q, true, true, false, false);
        CHECK(r.split == 16 && r.workgroups == 94u);                                                             // 24255 / 256
    });
    return n_failed ? 1 : 0;
}
