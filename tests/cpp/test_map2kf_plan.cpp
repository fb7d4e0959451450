// The pure host planner of the map <-> keyframe and keyframe <-> keyframe drivers (plslam_amd/csrc/map2kf_plan.hpp) on the CPU:
// no device, no HIP header, no library.  Hand cases whose expectations come from the comments here (cells worked out by hand),
// from the project's own restatement of the reference (oracle/plslam_oracle.c: plo_get_line_coords, plo_grid_fill_points) and
// from a literal restatement of the drivers' carving as it stood before the planner existed (old_fast_once, old_bf_once) --
// not from the code under test: one "PASS <case>" or "FAIL <case>: <what>" line each, exit status 1 when any failed.
//   g++ -std=c++17 -I plslam_amd/csrc -I include -I oracle tests/cpp/test_map2kf_plan.cpp oracle/plslam_oracle.c
#include <cmath>
#include <cstdio>
#include <cstring>
#include <functional>
#include <limits>
#include <string>
#include <vector>

#include "map2kf_plan.hpp"
#include "plslam_oracle.h"

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

using V = std::vector<int32_t>;
const double NaN = std::numeric_limits<double>::quiet_NaN();

V cells_of(double x1, double y1, double x2, double y2)
{
    V xy{7, 7};                                    // (line_cells clears what it is given)
    line_cells(x1, y1, x2, y2, xy);
    return xy;
}

plslam_fast_matching grid(int32_t cols, int32_t rows, double inv_w, double inv_h, int32_t ws = 1)
{
    plslam_fast_matching fm;
    memset(&fm, 0, sizeof(fm));
    fm.enabled = 1; fm.grid_cols = cols; fm.grid_rows = rows; fm.ws = ws; fm.inv_width = inv_w; fm.inv_height = inv_h;
    fm.nnr_grid = 0.75; fm.line_sim_th = 0.5;
    return fm;
}

// ---- the carving of the two one-synchronisation forms before the planner, word for word (Carver spelt out)
size_t old_take(size_t& off, size_t bytes) { const size_t o = off; off += (bytes + 255) & ~size_t(255); return o; }
struct OldOnce {
    size_t oLM, oMD, oCand, oT, oTF, oTi, oCs, oIt, oD2, oDesc, oAux, oRes, oPart, image, oMap, oQi, oQ, oQL, oCen, oD1, oM, oMask, off,
        pin_out;
};
size_t old_part_words(int32_t n) { return (size_t)(n > 0 ? (n + 256 - 1) / 256 : 1); }
OldOnce old_fast_once(int lines, bool map_dev, int32_t n_map, int32_t nt, size_t cs_size, int32_t n_items, size_t desc_bytes,
                      size_t aux_words)
{
    OldOnce o;
    const int lw = lines ? 6 : 3, fw = lines ? 3 : 2, nc = lines ? 2 : 1;
    size_t c = 0;
    o.oLM = old_take(c, map_dev ? 0 : (size_t)n_map * lw * 8); o.oMD = old_take(c, map_dev ? 0 : (size_t)n_map * 32);
    o.oCand = old_take(c, map_dev ? 0 : (size_t)n_map); o.oT = old_take(c, (size_t)nt * 32); o.oTF = old_take(c, (size_t)nt * fw * 8);
    o.oTi = old_take(c, (size_t)nt * 4); o.oCs = old_take(c, cs_size * 4); o.oIt = old_take(c, (size_t)(n_items + 1) * 4);
    o.oD2 = old_take(c, lines ? (size_t)nt * 16 : 0); o.oDesc = old_take(c, desc_bytes); o.oAux = old_take(c, aux_words * 4);
    o.oRes = old_take(c, 16);
    o.oPart = old_take(c, old_part_words(n_map) * 4);
    o.image = c;
    o.oMap = old_take(c, (size_t)n_map * 4);
    o.oQi = old_take(c, (size_t)n_map * 4); o.oQ = old_take(c, (size_t)n_map * 32);
    o.oQL = old_take(c, (size_t)n_map * lw * 8); o.oCen = old_take(c, (size_t)n_map * nc * 8);
    o.oD1 = old_take(c, lines ? (size_t)n_map * 16 : 0); o.oM = old_take(c, (size_t)n_map * 4); o.oMask = old_take(c, (size_t)n_map);
    o.off = c;
    o.pin_out = (o.oMap - o.oRes) + (size_t)n_map * 4;
    return o;
}
OldOnce old_bf_once(int lines, bool map_dev, int32_t n_map, int32_t nt)
{
    OldOnce o;
    memset(&o, 0, sizeof(o));
    const int lw = lines ? 6 : 3, fw = lines ? 3 : 2;
    size_t c = 0;
    o.oLM = old_take(c, map_dev ? 0 : (size_t)n_map * lw * 8); o.oMD = old_take(c, map_dev ? 0 : (size_t)n_map * 32);
    o.oCand = old_take(c, map_dev ? 0 : (size_t)n_map); o.oT = old_take(c, (size_t)nt * 32); o.oTF = old_take(c, (size_t)nt * fw * 8);
    o.oTi = old_take(c, (size_t)nt * 4);
    o.oRes = old_take(c, 16);
    o.oPart = old_take(c, old_part_words(n_map) * 4);
    o.image = c;
    o.oMap = old_take(c, (size_t)n_map * 4);
    o.oQi = old_take(c, (size_t)n_map * 4); o.oQ = old_take(c, (size_t)n_map * 32); o.oQL = old_take(c, (size_t)n_map * lw * 8);
    o.oM = old_take(c, (size_t)n_map * 4); o.oMask = old_take(c, (size_t)n_map);
    o.off = c;
    o.pin_out = (o.oMap - o.oRes) + (size_t)n_map * 4;
    return o;
}

// slices in the order given: each starts on a multiple of 256 bytes, not before the end of the one in front of it
struct Slice { size_t off, bytes; };
bool in_order(const std::vector<Slice>& s, size_t end)
{
    size_t at = 0;
    for (const Slice& x : s) {
        if (x.off % 256 != 0 || x.off < at) return false;
        at = x.off + x.bytes;
    }
    return at <= end && end % 256 == 0;
}

const int32_t N_MAP[] = {1, 255, 256, 257};
const int32_t N_T[] = {1, 40};

// dummy arguments of the entry checks: only their being null or not matters
char dummy[64];
int32_t three_idx[3] = {4, -1, -1};

}  // namespace

int main()
{
    // ---- line_cells: x from (int)x1 up to, not including, (int)x2 after the swaps; y follows the error term
    run("line_cells_steep", [] {
        // (0.5, 0.5) -> (1.5, 3.5): steep, walked along y = 0, 1, 2 with x stepping up after the second cell
        CHECK((cells_of(0.5, 0.5, 1.5, 3.5) == V{0, 0, 0, 1, 1, 2}));
    });
    run("line_cells_right_to_left", [] {
        // (5.5, 2.5) -> (1.5, 0.5) is walked from its left end: x = 1 .. 4, y up after every second cell
        CHECK((cells_of(5.5, 2.5, 1.5, 0.5) == V{1, 0, 2, 0, 3, 1, 4, 1}));
        CHECK(cells_of(5.5, 2.5, 1.5, 0.5) == cells_of(1.5, 0.5, 5.5, 2.5));
    });
    run("line_cells_horizontal_last_x_excluded", [] {
        CHECK((cells_of(1.0, 2.7, 4.0, 2.7) == V{1, 2, 2, 2, 3, 2}));       // cell x = 4, where the segment ends, is not listed
    });
    run("line_cells_zero_length", [] {
        CHECK(cells_of(3.3, 3.3, 3.3, 3.3).empty());
        CHECK(cells_of(3.2, 1.0, 3.9, 1.0).empty());                         // both ends in one cell column: no cell either
    });
    run("line_cells_negative_coordinates", [] {
        // the conversions truncate toward zero: y = (int)-0.5 = 0, x from (int)-2.5 = -2 to (int)1.5 = 1
        CHECK((cells_of(-2.5, -0.5, 1.5, -0.5) == V{-2, 0, -1, 0, 0, 0}));
    });
    run("line_cells_diagonal_against_oracle", [] {
        const double seg[3][4] = {{0.2, 0.3, 7.9, 6.1}, {7.9, 0.3, 0.2, 6.1}, {1.5, 9.75, 4.25, -3.5}};
        for (const auto& s : seg) {
            const V got = cells_of(s[0], s[1], s[2], s[3]);
            V want(64, 0);
            const int32_t n = plo_get_line_coords(s[0], s[1], s[2], s[3], want.data(), 32);
            CHECK(n > 3 && n <= 32);
            want.resize(2 * (size_t)n);
            CHECK(got == want);
        }
    });

    // ---- point cells (fill_grid_tables without lines): a 4 x 3 grid of unit cells
    run("point_cells_nan_and_huge_are_dropped", [] {
        CHECK(cvtt_x86(NaN) == INT32_MIN && cvtt_x86(1e10) == INT32_MIN && cvtt_x86(-1e10) == INT32_MIN);
        CHECK(cvtt_x86(2147483648.0) == INT32_MIN && cvtt_x86(2147483647.5) == 2147483647 && cvtt_x86(-2147483648.5) == INT32_MIN);
        CHECK(cvtt_x86(-0.75) == 0 && cvtt_x86(2.99) == 2);
        const plslam_fast_matching fm = grid(4, 3, 1.0, 1.0);
        const double p[] = {NaN, 1.0, 1e10, 1.0, -1e10, 1.0, 1.5, NaN, 1.5, 1.5};
        const GridTables g = fill_grid_tables(0, p, nullptr, 5, &fm);
        CHECK(g.n_items == 1 && g.items.size() == 2 && g.items[0] == 4);
        CHECK(g.cs[1 * 3 + 1] == 0 && g.cs[1 * 3 + 2] == 1 && g.cs.back() == 1);
    });
    run("point_cells_border_column_and_row_dropped", [] {
        const plslam_fast_matching fm = grid(4, 3, 1.0, 1.0);
        const double p[] = {4.0, 1.0, 1.0, 3.0, 4.5, 3.5};                  // column `cols`, row `rows`, both
        const GridTables g = fill_grid_tables(0, p, nullptr, 3, &fm);
        CHECK(g.n_items == 0 && g.items.size() == 1 && g.cs == V(13, 0));
    });
    run("point_cells_corner_cells_kept", [] {
        const plslam_fast_matching fm = grid(4, 3, 1.0, 1.0);
        const double p[] = {0.9, 0.9, 3.99, 2.99, -0.5, 1.2};                // (0, 0), (3, 2) and -- truncation toward zero -- (0, 1)
        const GridTables g = fill_grid_tables(0, p, nullptr, 3, &fm);
        V cs(13, 3);
        cs[0] = 0; cs[1] = 1;
        for (int c = 2; c <= 11; ++c) cs[c] = 2;
        CHECK(g.cs == cs);
        CHECK((g.items == V{0, 2, 1, 0}));
    });
    run("csr_fill_push_order_and_sizes", [] {
        V cs, items;
        csr_fill(V{0, 1, 2, 3, 4}, V{1, 0, 1, 1, 0}, V{1, 0, 1, 1, 0}, 2, 2, cs, items);
        CHECK((cs == V{0, 2, 2, 2, 5}));                                      // cols * rows + 1 entries; cell id = x * rows + y
        CHECK((items == V{1, 4, 0, 2, 3, 0}));                                // n_items + 1 entries, a cell's items in push order
        csr_fill(V{}, V{}, V{}, 3, 2, cs, items);
        CHECK(cs == V(7, 0) && items == V(1, 0));
    });

    // ---- fill_grid_tables
    run("grid_tables_points_with_and_without_sel", [] {
        const plslam_fast_matching fm = grid(8, 6, 0.5, 0.25);                 // a cell is 2 x 4 pixels
        const double p[] = {3.0, 9.0, 15.9, 23.9, 3.5, 11.0, 100.0, 1.0};     // cells (1, 2), (7, 5), (1, 2), out
        const GridTables a = fill_grid_tables(0, p, nullptr, 4, &fm);
        CHECK(a.n_items == 3 && a.cs.size() == 49 && a.items.size() == 4 && a.dir2.empty());
        CHECK(a.cs[8] == 0 && a.cs[9] == 2 && a.cs[47] == 2 && a.cs[48] == 3);
        CHECK((a.items == V{0, 2, 1, 0}));
        const int32_t sel[] = {2, 3, 1};                                      // item b is feature sel[b]
        const GridTables b = fill_grid_tables(0, p, sel, 3, &fm);
        CHECK(b.n_items == 2 && b.cs[9] == 1 && b.cs[48] == 2);
        CHECK((b.items == V{0, 2, 0}));
    });
    run("grid_tables_lines_dir2_and_three_cells", [] {
        const plslam_fast_matching fm = grid(8, 6, 0.5, 0.5);
        const double sg[] = {2.0, 2.0, 2.0, 2.0, 1.0, 1.0, 7.0, 1.0};         // a zero-length segment; grid (0.5, 0.5) -> (3.5, 0.5)
        const GridTables a = fill_grid_tables(1, sg, nullptr, 2, &fm);
        CHECK(a.dir2.size() == 4 && std::isnan(a.dir2[0]) && std::isnan(a.dir2[1]) && a.dir2[2] == 1.0 && a.dir2[3] == 0.0);
        CHECK(a.n_items == 3 && a.items.size() == 4);
        CHECK(a.cs[0] == 0 && a.cs[1] == 1 && a.cs[6] == 1 && a.cs[7] == 2 && a.cs[12] == 2 && a.cs[13] == 3 && a.cs[48] == 3);
        CHECK((a.items == V{1, 1, 1, 0}));                                    // cells (0, 0), (1, 0), (2, 0) each list the segment
        const int32_t sel[] = {1, 0};
        const GridTables b = fill_grid_tables(1, sg, sel, 2, &fm);
        CHECK(b.cs == a.cs && (b.items == V{0, 0, 0, 0}));
        CHECK(b.dir2[0] == 1.0 && b.dir2[1] == 0.0 && std::isnan(b.dir2[2]) && std::isnan(b.dir2[3]));
    });
    run("grid_tables_points_against_oracle", [] {
        const plslam_fast_matching fm = grid(8, 6, 8.0 / 752.0, 6.0 / 480.0);
        const int32_t n = 60;
        std::vector<double> p(2 * (size_t)n);
        V xy(2 * (size_t)n);
        uint32_t s = 12345u;
        for (size_t k = 0; k < p.size(); ++k) {
            s = s * 1664525u + 1013904223u;
            p[k] = (double)(s >> 8) / 16777216.0 * ((k & 1) ? 560.0 : 860.0) - 40.0;   // some outside on every side
            xy[k] = (int32_t)(p[k] * ((k & 1) ? fm.inv_height : fm.inv_width));
        }
        V cs(49, -1), items((size_t)n, -1);
        plo_grid_fill_points(xy.data(), n, 8, 6, cs.data(), items.data());
        const GridTables g = fill_grid_tables(0, p.data(), nullptr, n, &fm);
        CHECK(g.cs == cs && g.n_items == cs.back() && g.n_items > 20 && g.n_items < n);
        CHECK(g.items.size() == (size_t)g.n_items + 1);
        CHECK(std::equal(g.items.begin(), g.items.end() - 1, items.begin()));
    });

    // ---- kf2kf_line_grid_bound: a 64 x 48 grid, ws = 1 -> reach 3; K and DT the identity, so (u, v) = (X / Z, Y / Z)
    run("line_grid_bound_cases", [] {
        const plslam_fast_matching fm = grid(64, 48, 1.0, 1.0, 1);
        plslam_cam K;
        memset(&K, 0, sizeof(K));
        K.fx = K.fy = 1.0;
        const double DT[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
        const double out_both[6] = {-10, 5, 1, 70, 60, 1}, one_in[6] = {-10, 5, 1, 10, 10, 1}, near_border[6] = {-2.5, 5, 1, -10, 5, 1},
                     near_far_border[6] = {-10, 5, 1, 66.9, 50.9, 1}, just_out[6] = {-3.5, 5, 1, 67.5, 5, 1}, nan_proj[6] = {0, 0, 0, -10, 5, 1};
        CHECK(kf2kf_line_grid_bound(&K, DT, out_both, 1, &fm) == 0);
        CHECK(kf2kf_line_grid_bound(&K, DT, one_in, 1, &fm) == 1);
        CHECK(kf2kf_line_grid_bound(&K, DT, near_border, 1, &fm) == 1);
        CHECK(kf2kf_line_grid_bound(&K, DT, near_far_border, 1, &fm) == 1);
        CHECK(kf2kf_line_grid_bound(&K, DT, just_out, 1, &fm) == 0);
        CHECK(kf2kf_line_grid_bound(&K, DT, nan_proj, 1, &fm) == 1);          // P[2] == 0 with P[0] == 0: not a number counts as "may"
        double all[36];
        const double* rows[] = {out_both, one_in, near_border, near_far_border, just_out, nan_proj};
        for (int i = 0; i < 6; ++i) memcpy(all + 6 * i, rows[i], 48);
        CHECK(kf2kf_line_grid_bound(&K, DT, all, 6, &fm) == 4);
        CHECK(kf2kf_line_grid_bound(&K, DT, all, 0, &fm) == 0);
    });

    // ---- the layouts
    run("once_layout_sweep", [] {
        const GridSizes gs{13, 40, 136, 10};
        for (int lines = 0; lines < 2; ++lines)
            for (int map_dev = 0; map_dev < 2; ++map_dev)
                for (int32_t n_map : N_MAP)
                    for (int32_t nt : N_T)
                        for (int fast = 0; fast < 2; ++fast) {
                            const OnceLayout L(lines, map_dev != 0, n_map, nt, fast ? &gs : nullptr);
                            const size_t lw = lines ? 6 : 3, fw = lines ? 3 : 2, nc = lines ? 2 : 1, nm = (size_t)n_map, n2 = (size_t)nt;
                            const size_t gr = fast ? 1 : 0;                        // the grid slices: only in the fast form
                            const std::vector<Slice> up = {
                                {L.oLM, map_dev ? 0 : nm * lw * 8}, {L.oMD, map_dev ? 0 : nm * 32}, {L.oCand, map_dev ? 0 : nm},
                                {L.oT, n2 * 32}, {L.oTF, n2 * fw * 8}, {L.oTi, n2 * 4}, {L.oCs, gr * 13 * 4},
                                {L.oIt, gr * 41 * 4}, {L.oD2, fast && lines ? n2 * 16 : 0}, {L.oDesc, gr * 136},
                                {L.oAux, gr * 40}, {L.oRes, 16}, {L.oPart, (nm + 255) / 256 * 4}};
                            std::vector<Slice> all = up;
                            const std::vector<Slice> dev = {{L.oMap, nm * 4}, {L.oQi, nm * 4}, {L.oQ, nm * 32}, {L.oQL, nm * lw * 8},
                                                            {L.oCen, fast ? nm * nc * 8 : 0}, {L.oD1, fast && lines ? nm * 16 : 0},
                                                            {L.oM, nm * 4}, {L.oMask, nm}};
                            all.insert(all.end(), dev.begin(), dev.end());
                            CHECK(in_order(up, L.image));
                            CHECK(in_order(all, L.bytes));
                            CHECK(L.image == L.oMap);                              // the first device-only slice: the table
                            CHECK(L.tab_out == L.oMap - L.oRes && L.pin_out == (L.oMap - L.oRes) + 4 * nm);
                            CHECK(L.part_bytes == (nm + 255) / 256 * 4);
                            if (map_dev) CHECK(L.oLM == 0 && L.oMD == 0 && L.oCand == 0 && L.oT == 0);
                            else CHECK(L.oT > L.oCand && L.oCand > L.oMD && L.oMD > L.oLM);
                            if (!fast) CHECK(L.oCs == L.oRes && L.oIt == L.oRes && L.oD2 == L.oRes && L.oDesc == L.oRes && L.oAux == L.oRes &&
                                             L.oCen == L.oM && L.oD1 == L.oM);
                        }
    });
    run("once_layout_is_the_carving_it_replaces", [] {
        const GridSizes gs{3073, 77, 136, 19};
        for (int lines = 0; lines < 2; ++lines)
            for (int map_dev = 0; map_dev < 2; ++map_dev)
                for (int32_t n_map : N_MAP)
                    for (int32_t nt : N_T) {
                        const OnceLayout F(lines, map_dev != 0, n_map, nt, &gs), B(lines, map_dev != 0, n_map, nt, nullptr);
                        const OldOnce f = old_fast_once(lines, map_dev != 0, n_map, nt, 3073, 77, 136, 19), b = old_bf_once(lines, map_dev != 0, n_map, nt);
                        CHECK(F.oLM == f.oLM && F.oMD == f.oMD && F.oCand == f.oCand && F.oT == f.oT && F.oTF == f.oTF && F.oTi == f.oTi);
                        CHECK(F.oCs == f.oCs && F.oIt == f.oIt && F.oD2 == f.oD2 && F.oDesc == f.oDesc && F.oAux == f.oAux);
                        CHECK(F.oRes == f.oRes && F.oPart == f.oPart && F.image == f.image && F.oMap == f.oMap && F.oQi == f.oQi);
                        CHECK(F.oQ == f.oQ && F.oQL == f.oQL && F.oCen == f.oCen && F.oD1 == f.oD1 && F.oM == f.oM && F.oMask == f.oMask);
                        CHECK(F.bytes == f.off && F.pin_out == f.pin_out);
                        // the brute-force form: the fast form without its grid slices, offset for offset
                        CHECK(B.oLM == b.oLM && B.oMD == b.oMD && B.oCand == b.oCand && B.oT == b.oT && B.oTF == b.oTF && B.oTi == b.oTi);
                        CHECK(B.oRes == b.oRes && B.oPart == b.oPart && B.image == b.image && B.oMap == b.oMap && B.oQi == b.oQi);
                        CHECK(B.oQ == b.oQ && B.oQL == b.oQL && B.oM == b.oM && B.oMask == b.oMask && B.bytes == b.off && B.pin_out == b.pin_out);
                    }
    });
    run("once_layout_written_down", [] {
        // points, map not resident, 257 landmarks x 40 features; sizes rounded up to 256 by hand:
        //   map 6168 -> 6400 | med 8224 -> 8448 | cand 257 -> 512 | T 1280 | TF 640 -> 768 | ti 160 -> 256 | res 256 | part 8 -> 256
        //   table 1028 -> 1280 | qi 1280 | Q 8448 | QL 6400 | M 1280 | mask 512
        const OnceLayout B(0, false, 257, 40, nullptr);
        CHECK(B.oLM == 0 && B.oMD == 6400 && B.oCand == 14848 && B.oT == 15360 && B.oTF == 16640 && B.oTi == 17408);
        CHECK(B.oRes == 17664 && B.oPart == 17920 && B.image == 18176 && B.oMap == 18176 && B.oQi == 19456 && B.oQ == 20736);
        CHECK(B.oQL == 29184 && B.oM == 35584 && B.oMask == 36864 && B.bytes == 37376 && B.tab_out == 512 && B.pin_out == 1540);
        // the same with a 4 x 3 grid of 40 items, a 128-byte descriptor, 10 shared words: cs 52, items 164, desc, aux -> 256 each;
        // window centres 2056 -> 2304
        const GridSizes gs{13, 40, 128, 10};
        const OnceLayout F(0, false, 257, 40, &gs);
        CHECK(F.oTi == 17408 && F.oCs == 17664 && F.oIt == 17920 && F.oD2 == 18176 && F.oDesc == 18176 && F.oAux == 18432);
        CHECK(F.oRes == 18688 && F.oPart == 18944 && F.image == 19200 && F.oMap == 19200 && F.oQi == 20480 && F.oQ == 21760);
        CHECK(F.oQL == 30208 && F.oCen == 36608 && F.oD1 == 38912 && F.oM == 38912 && F.oMask == 40192 && F.bytes == 40704);
        CHECK(F.tab_out == 512 && F.pin_out == 1540);
        // lines, map resident, one landmark, one feature
        const OnceLayout R(1, true, 1, 1, nullptr);
        CHECK(R.oT == 0 && R.oTF == 256 && R.oTi == 512 && R.oRes == 768 && R.oPart == 1024 && R.image == 1280 && R.oMask == 2560 &&
              R.bytes == 2816 && R.pin_out == 516);
    });
    run("step_layout", [] {
        for (int lines = 0; lines < 2; ++lines)
            for (int map_dev = 0; map_dev < 2; ++map_dev)
                for (int32_t n_map : N_MAP)
                    for (int32_t nt : N_T) {
                        const int32_t n_kf = nt + 7;
                        const StepLayout L(lines, map_dev != 0, n_map, n_kf, nt);
                        const size_t lw = lines ? 6 : 3, fw = lines ? 3 : 2, nm = (size_t)n_map, nk = (size_t)n_kf, n2 = (size_t)nt;
                        CHECK(in_order({{L.oLM, map_dev ? 0 : nm * lw * 8}, {L.oMD, map_dev ? 0 : nm * 32}, {L.oKD, nk * 32}, {L.oKF, nk * fw * 8}}, L.image1));
                        CHECK(in_order({{L.oLM, 0}, {L.oKF, nk * fw * 8}, {L.oQi, nm * 4}, {L.oTi, n2 * 4}, {L.oVis, nm}, {L.oQ, nm * 32},
                                        {L.oT, n2 * 32}, {L.oQL, nm * lw * 8}, {L.oTF, n2 * fw * 8}, {L.oM, nm * 4}, {L.oMask, nm}, {L.oCnt, 8}}, L.bytes));
                        CHECK(L.oQi == L.image1 && L.image2 == L.oVis - L.oQi && L.results == L.bytes - L.oM);
                        CHECK(L.pin_in == std::max(L.image1, L.image2) && L.pin_out == std::max(L.results, nm));
                        if (map_dev) CHECK(L.oKD == 0);
                    }
        const StepLayout L(0, false, 257, 47, 40);     // map 6400 | med 8448 | kd 1504 -> 1536 | kf 752 -> 768
        CHECK(L.oMD == 6400 && L.oKD == 14848 && L.oKF == 16384 && L.image1 == 17152 && L.oTi == 18432 && L.image2 == 1536 && L.oVis == 18688);
        CHECK(L.oM == 36096 && L.oMask == 37376 && L.oCnt == 37888 && L.results == 2048 && L.bytes == 38144);
    });
    run("grid_path_layout", [] {
        for (int lines = 0; lines < 2; ++lines)
            for (int32_t nq : N_MAP)
                for (int32_t nt : N_T) {
                    const GridPathLayout L(lines, nq, nt, GridSizes{3073, 77, 136, 19});
                    const size_t nc = lines ? 2 : 1;
                    CHECK(L.oSt == 0);
                    CHECK(in_order({{L.oSt, 16}, {L.oCs, 3073 * 4}, {L.oIt, 78 * 4}, {L.oD2, lines ? (size_t)nt * 16 : 0}, {L.oDesc, 136}, {L.oAux, 76}},
                                   L.image));
                    CHECK(L.oCen == L.image && in_order({{L.oCen, (size_t)nq * nc * 8}, {L.oD1, lines ? (size_t)nq * 16 : 0}}, L.bytes));
                }
        const GridPathLayout L(1, 257, 40, GridSizes{13, 40, 128, 10});
        CHECK(L.oCs == 256 && L.oIt == 512 && L.oD2 == 768 && L.oDesc == 1536 && L.oAux == 1792 && L.image == 2048 && L.oD1 == 6400 && L.bytes == 10752);
    });
    run("kf2kf_layout", [] {
        for (int lines = 0; lines < 2; ++lines)
            for (int rows_dev = 0; rows_dev < 2; ++rows_dev)
                for (int fast = 0; fast < 2; ++fast)
                    for (int32_t n_prev : N_MAP)
                        for (int32_t n_curr : N_T) {
                            const Kf2kfLayout L(lines, rows_dev != 0, fast != 0, n_prev, n_curr);
                            const size_t xw = lines ? 6 : 3, np = (size_t)n_prev;
                            CHECK(in_order({{L.oQ, rows_dev ? 0 : np * 32}, {L.oT, rows_dev ? 0 : (size_t)n_curr * 32},
                                            {L.oX, fast && !rows_dev ? np * xw * 8 : 0}}, L.image));
                            CHECK(L.oM == L.image && in_order({{L.oM, np * 4}, {L.oCnt, 16}}, L.bytes) && L.pin_out == np * 4 + 256);
                            if (rows_dev) CHECK(L.image == 0);
                        }
        const Kf2kfLayout L(1, false, true, 257, 40);   // Q 8448 | T 1280 | X 12336 -> 12544
        CHECK(L.oT == 8448 && L.oX == 9728 && L.image == 22272 && L.oCnt == 23552 && L.bytes == 23808 && L.pin_out == 1284);
    });

    // ---- staging and the problem record
    run("stage_once_image_contents", [] {
        for (int map_dev = 0; map_dev < 2; ++map_dev) {
            const int lines = 1;
            const int32_t n_map = 3;                                               // and five keyframe features, two of them unmatched
            std::vector<double> LM(18), feat(15);
            std::vector<uint8_t> med(96), cand{1, 0, 1}, kd(160);
            for (size_t k = 0; k < LM.size(); ++k) LM[k] = 100.0 + (double)k;
            for (size_t k = 0; k < feat.size(); ++k) feat[k] = 0.5 + (double)k;
            for (size_t k = 0; k < med.size(); ++k) med[k] = (uint8_t)(k + 1);
            for (size_t k = 0; k < kd.size(); ++k) kd[k] = (uint8_t)(200 - k);
            const V ti{1, 4};
            const plslam_fast_matching fm = grid(8, 6, 0.5, 0.5);
            const double sg[] = {0, 0, 0, 0, 1.0, 1.0, 7.0, 1.0, 0, 0, 0, 0, 0, 0, 0, 0, 2.0, 2.0, 2.0, 9.0};
            const GridTables g = fill_grid_tables(lines, sg, ti.data(), 2, &fm);
            const GridSizes gs{g.cs.size(), (size_t)g.n_items, 136, 10};
            const OnceLayout L(lines, map_dev != 0, n_map, 2, &gs);
            std::vector<char> h(L.image, (char)0x5A);                              // exactly the image: the sanitizers watch its end
            stage_once_image(L, h.data(), lines, map_dev != 0, map_dev ? nullptr : LM.data(), map_dev ? nullptr : med.data(),
                             map_dev ? nullptr : cand.data(), n_map, kd.data(), feat.data(), ti, &g);
            if (!map_dev) CHECK(!memcmp(h.data() + L.oLM, LM.data(), 144) && !memcmp(h.data() + L.oMD, med.data(), 96) && !memcmp(h.data() + L.oCand, cand.data(), 3));
            CHECK(!memcmp(h.data() + L.oT, kd.data() + 32, 32) && !memcmp(h.data() + L.oT + 32, kd.data() + 128, 32));
            CHECK(!memcmp(h.data() + L.oTF, feat.data() + 3, 24) && !memcmp(h.data() + L.oTF + 24, feat.data() + 12, 24));
            CHECK(!memcmp(h.data() + L.oTi, ti.data(), 8));
            CHECK(!memcmp(h.data() + L.oCs, g.cs.data(), 49 * 4) && !memcmp(h.data() + L.oIt, g.items.data(), ((size_t)g.n_items + 1) * 4));
            CHECK(!memcmp(h.data() + L.oD2, g.dir2.data(), 32));
            const char zero[16] = {0};
            CHECK(!memcmp(h.data() + L.oRes, zero, 16) && !memcmp(h.data() + L.oPart, zero, 4) && L.part_bytes == 4);
            CHECK(h[L.oDesc] == 0x5A && h[L.oAux] == 0x5A && h[L.oRes + 16] == 0x5A);   // the matcher's slices and the slack: not touched
            // the brute-force form: no grid slices
            const OnceLayout B(lines, map_dev != 0, n_map, 2, nullptr);
            std::vector<char> hb(B.image, (char)0x5A);
            stage_once_image(B, hb.data(), lines, map_dev != 0, map_dev ? nullptr : LM.data(), map_dev ? nullptr : med.data(),
                             map_dev ? nullptr : cand.data(), n_map, kd.data(), feat.data(), ti, nullptr);
            CHECK(!memcmp(hb.data() + B.oT, kd.data() + 32, 32) && !memcmp(hb.data() + B.oTi, ti.data(), 8) && !memcmp(hb.data() + B.oRes, zero, 16));
        }
    });
    run("fill_grid_problem_fields", [] {
        static char dev[1 << 16], img[1 << 16];
        const plslam_fast_matching fm = grid(64, 48, 0.1, 0.2, 3);
        const GridPathLayout L(1, 300, 40, GridSizes{3073, 77, 136, 19});
        const uint8_t* d1 = (const uint8_t*)dummy;
        const uint8_t* d2 = (const uint8_t*)dummy + 32;
        int32_t m12 = 0, cnt = 0;
        const plslam_grid_problem q = fill_grid_problem(L, dev, img, 1, d1, 300, d2, 40, 77, &fm, 5, 123456, &m12, &cnt);
        CHECK(q.d1 == d1 && q.d2 == d2 && q.n1 == 300 && q.n2 == 40 && q.n_centres == 2 && q.grid_cols == 64 && q.grid_rows == 48 && q.n_items == 77);
        CHECK((const char*)q.centres1 == dev + L.oCen && (const char*)q.dir1 == dev + L.oD1);                // what a kernel writes: device
        CHECK((const char*)q.cell_start == img + L.oCs && (const char*)q.cell_items == img + L.oIt && (const char*)q.dir2 == img + L.oD2);
        CHECK(q.window[0] == 3 && q.window[1] == 3 && q.window[2] == 3 && q.window[3] == 3 && q.sim_th == 0.5 && q.nnr == 0.75);
        CHECK(q.mutual == 1 && q.pair_capacity == 123456 && q.matches_12 == &m12 && q.n_matches == &cnt);
        const OnceLayout O(0, false, 300, 40, nullptr);
        const plslam_grid_problem p = fill_grid_problem(O, dev, dev, 0, d1, 300, d2, 40, 0, &fm, 0, 0, &m12, nullptr);
        CHECK(p.n_centres == 1 && p.dir1 == nullptr && p.dir2 == nullptr && p.mutual == 0 && p.n_matches == nullptr);
    });

    // ---- argument checks and early returns
    run("map2kf_entry_table", [] {
        const plslam_fast_matching fast = grid(64, 48, 0.1, 0.1);
        plslam_fast_matching bad = fast, disabled = bad;
        bad.grid_cols = 0;
        disabled.grid_cols = 0; disabled.enabled = 0;                          // not enabled: its fields are not looked at
        plslam_cam K;
        const double* Twf = (const double*)dummy;
        const void* p = dummy;
        Entry e;
        V ti;
        auto call = [&](const void* ctx, int lines, const void* LM, int32_t n_map, const void* kd, const void* seg, const int32_t* idx,
                        int32_t n_kf, int32_t min_matches, const plslam_fast_matching* fm, const void* out) {
            return map2kf_entry(ctx, &K, Twf, lines, LM, p, p, n_map, kd, p, seg, idx, n_kf, min_matches, fm, out, e, ti);
        };
        auto is = [&](EntryDo what, bool zero, bool fill) { return e.what == what && e.zero_counts == zero && e.fill_table == fill; };
        // refusals before anything is written
        CHECK(call(nullptr, 0, p, 5, p, p, three_idx, 3, 10, nullptr, p) == PLSLAM_EINVAL && is(ENTRY_REFUSE, false, false));
        CHECK(call(p, 0, p, -1, p, p, three_idx, 3, 10, nullptr, p) == PLSLAM_EINVAL && is(ENTRY_REFUSE, false, false));
        CHECK(call(p, 0, p, 5, p, p, three_idx, -1, 10, nullptr, p) == PLSLAM_EINVAL && is(ENTRY_REFUSE, false, false));
        CHECK(call(p, 0, p, 5, p, p, three_idx, 3, 10, &bad, p) == PLSLAM_EINVAL && is(ENTRY_REFUSE, false, false));
        CHECK(call(p, 0, p, 0, p, p, three_idx, 3, 10, &bad, p) == PLSLAM_EINVAL && is(ENTRY_REFUSE, false, false));   // (before n_map == 0)
        CHECK(call(p, 1, p, 5, p, nullptr, three_idx, 3, 10, &fast, p) == PLSLAM_EINVAL && is(ENTRY_REFUSE, false, false));
        // n_map == 0: the counters are zeroed, the table is not touched; no array is needed
        CHECK(call(p, 0, nullptr, 0, nullptr, nullptr, nullptr, 3, 10, nullptr, nullptr) == PLSLAM_OK && is(ENTRY_RETURN, true, false));
        CHECK(call(p, 1, nullptr, 0, nullptr, nullptr, nullptr, 0, 10, &fast, nullptr) == PLSLAM_OK && is(ENTRY_RETURN, true, false));   // (lines without kf_seg: n_kf == 0)
        // refusals after the counters are zeroed
        CHECK(call(p, 0, nullptr, 5, p, p, three_idx, 3, 10, nullptr, p) == PLSLAM_EINVAL && is(ENTRY_REFUSE, true, false));
        CHECK(call(p, 0, p, 5, p, p, three_idx, 3, 10, nullptr, nullptr) == PLSLAM_EINVAL && is(ENTRY_REFUSE, true, false));
        CHECK(call(p, 0, p, 5, nullptr, p, three_idx, 3, 10, nullptr, p) == PLSLAM_EINVAL && is(ENTRY_REFUSE, true, false));
        CHECK(call(p, 0, p, 5, p, p, nullptr, 3, 10, nullptr, p) == PLSLAM_EINVAL && is(ENTRY_REFUSE, true, false));
        // no unmatched feature: the table is filled, nothing runs
        const int32_t matched[3] = {0, 7, 2};
        CHECK(call(p, 0, p, 5, p, p, matched, 3, 10, &fast, p) == PLSLAM_OK && is(ENTRY_FILL_RETURN, true, true) && ti.empty());
        CHECK(call(p, 0, p, 5, nullptr, p, nullptr, 0, 10, nullptr, p) == PLSLAM_OK && is(ENTRY_FILL_RETURN, true, true));
        // brute force with min_matches <= 0: no matcher would run
        CHECK(call(p, 0, p, 5, p, p, three_idx, 3, 0, nullptr, p) == PLSLAM_OK && is(ENTRY_FILL_RETURN, true, true));
        CHECK(call(p, 0, p, 5, p, p, three_idx, 3, -1, &disabled, p) == PLSLAM_OK && is(ENTRY_FILL_RETURN, true, true));
        // run
        CHECK(call(p, 0, p, 5, p, p, three_idx, 3, 1, nullptr, p) == PLSLAM_OK && is(ENTRY_RUN, true, true) && (ti == V{1, 2}));
        CHECK(call(p, 0, p, 5, p, p, three_idx, 3, 1, &disabled, p) == PLSLAM_OK && is(ENTRY_RUN, true, true));
        CHECK(call(p, 0, p, 5, p, p, three_idx, 3, 0, &fast, p) == PLSLAM_OK && is(ENTRY_RUN, true, true));            // matchGrid runs whatever min_matches is
        CHECK(call(p, 1, p, 5, p, p, three_idx, 3, 10, &fast, p) == PLSLAM_OK && is(ENTRY_RUN, true, true));
        CHECK(call(p, 1, p, 5, p, nullptr, three_idx, 3, 10, nullptr, p) == PLSLAM_OK && is(ENTRY_RUN, true, true));   // brute-force lines need no kf_seg
    });
    run("kf2kf_entry_table", [] {
        const plslam_fast_matching fast = grid(64, 48, 0.1, 0.1);
        plslam_fast_matching bad = fast;
        bad.ws = -1;
        plslam_cam K;
        const double* DT = (const double*)dummy;
        const void* p = dummy;                                               // (64-byte aligned below)
        Entry e;
        auto call = [&](const void* ctx, const void* X, const void* dp, int32_t n_prev, const void* dc, int32_t n_curr, int32_t min_matches,
                        const plslam_fast_matching* fm, const void* out, bool rows_dev) {
            return kf2kf_entry(ctx, &K, DT, X, dp, n_prev, p, dc, n_curr, min_matches, fm, out, rows_dev, e);
        };
        auto is = [&](EntryDo what, bool zero, bool fill) { return e.what == what && e.zero_counts == zero && e.fill_table == fill; };
        CHECK(call(nullptr, p, p, 30, p, 30, 20, nullptr, p, false) == PLSLAM_EINVAL && is(ENTRY_REFUSE, false, false));
        CHECK(call(p, p, p, -1, p, 30, 20, nullptr, p, false) == PLSLAM_EINVAL && is(ENTRY_REFUSE, false, false));
        CHECK(call(p, p, p, 30, p, -1, 20, nullptr, p, false) == PLSLAM_EINVAL && is(ENTRY_REFUSE, false, false));
        CHECK(call(p, p, p, 0, p, 30, 20, &bad, p, false) == PLSLAM_EINVAL && is(ENTRY_REFUSE, false, false));
        CHECK(call(p, nullptr, nullptr, 0, nullptr, 30, 20, nullptr, nullptr, false) == PLSLAM_OK && is(ENTRY_RETURN, true, false));   // n_prev == 0
        CHECK(call(p, p, p, 30, p, 30, 20, nullptr, nullptr, false) == PLSLAM_EINVAL && is(ENTRY_REFUSE, true, false));
        CHECK(call(p, nullptr, nullptr, 30, nullptr, 0, 20, nullptr, p, false) == PLSLAM_OK && is(ENTRY_FILL_RETURN, true, true));     // n_curr == 0: table -1, OK
        CHECK(call(p, nullptr, p, 30, p, 30, 20, nullptr, p, false) == PLSLAM_EINVAL && is(ENTRY_REFUSE, true, true));                 // (the table is filled by then)
        CHECK(call(p, p, p, 30, nullptr, 30, 20, nullptr, p, false) == PLSLAM_EINVAL && is(ENTRY_REFUSE, true, true));
        alignas(64) static char al[64];
        CHECK(call(p, al, al + 16, 30, al + 32, 30, 20, &fast, p, true) == PLSLAM_OK && is(ENTRY_RUN, true, true));
        CHECK(call(p, al, al + 8, 30, al + 32, 30, 20, &fast, p, true) == PLSLAM_EINVAL && is(ENTRY_REFUSE, true, true));
        CHECK(call(p, al, al + 16, 30, al + 40, 30, 20, &fast, p, true) == PLSLAM_EINVAL && is(ENTRY_REFUSE, true, true));
        CHECK(call(p, al + 4, al + 16, 30, al + 32, 30, 20, &fast, p, true) == PLSLAM_EINVAL && is(ENTRY_REFUSE, true, true));
        CHECK(call(p, al + 4, al + 8, 30, al + 40, 30, 20, &fast, p, false) == PLSLAM_OK && is(ENTRY_RUN, true, true));                 // host rows: any alignment
        // !fast && !(bf_possible && 0 < min_matches): no matcher would run
        CHECK(call(p, p, p, 20, p, 30, 20, nullptr, p, false) == PLSLAM_OK && is(ENTRY_FILL_RETURN, true, true));
        CHECK(call(p, p, p, 30, p, 20, 20, nullptr, p, false) == PLSLAM_OK && is(ENTRY_FILL_RETURN, true, true));
        CHECK(call(p, p, p, 30, p, 30, 0, nullptr, p, false) == PLSLAM_OK && is(ENTRY_FILL_RETURN, true, true));
        CHECK(call(p, p, p, 21, p, 21, 20, nullptr, p, false) == PLSLAM_OK && is(ENTRY_RUN, true, true));
        CHECK(call(p, p, p, 20, p, 20, 20, &fast, p, false) == PLSLAM_OK && is(ENTRY_RUN, true, true));                                // matchGrid runs either way
        CHECK(kf2kf_bf_possible(21, 21, 20) && !kf2kf_bf_possible(21, 20, 20) && !kf2kf_bf_possible(20, 21, 20));
    });
    run("entry_apply_writes_what_the_entry_says", [] {
        for (int zero = 0; zero < 2; ++zero)
            for (int fill = 0; fill < 2; ++fill)
                for (int what = 0; what < 4; ++what) {
                    Entry e;
                    e.what = (EntryDo)what; e.zero_counts = zero != 0; e.fill_table = fill != 0;
                    int32_t tab[4] = {9, 9, 9, 9}, n = 5, used = 6;
                    CHECK(entry_apply(e, tab, 3, &n, &used) == (what == ENTRY_RUN));
                    CHECK(n == (zero ? 0 : 5) && used == (zero ? 0 : 6));
                    CHECK(tab[0] == (fill ? -1 : 9) && tab[2] == (fill ? -1 : 9) && tab[3] == 9);
                    CHECK(entry_apply(e, fill ? tab : nullptr, 3, nullptr, nullptr) == (what == ENTRY_RUN));   // the counters are optional
                }
    });

    // ---- decisions
    run("kf2kf_table_all_combinations", [] {
        for (int keep = 0; keep < 2; ++keep)
            for (int host = 0; host < 2; ++host)
                for (int mapped = 0; mapped < 2; ++mapped) {
                    // the ladder the driver had in the middle of its launches, word for word
                    bool on_host = host != 0, count_only = false, count_entries = false, upload = false, in_mapped;
                    if (keep && on_host && mapped) { in_mapped = true; count_only = true; }
                    else if (keep) { if (on_host) upload = true; in_mapped = false; on_host = false; }
                    else { in_mapped = mapped != 0; on_host = mapped != 0; count_entries = on_host; }
                    const Kf2kfTable t = kf2kf_table(keep != 0, host != 0, mapped != 0);
                    CHECK(t.mapped == in_mapped && t.upload_first == upload && t.count_only == count_only && t.count_entries == count_entries &&
                          t.on_host == on_host);
                    CHECK(!(t.count_only && t.count_entries) && !(t.mapped && !mapped) && (!t.count_only || t.on_host));
                }
        // the common paths: matchGrid's table in the mapped block is finished in place; a fresh table in the block is counted on the host
        const Kf2kfTable a = kf2kf_table(true, true, true), b = kf2kf_table(false, false, true), c = kf2kf_table(false, false, false);
        CHECK(a.mapped && a.count_only && !a.upload_first && b.mapped && b.count_entries && b.on_host && !c.mapped && !c.on_host && !c.count_entries);
    });
    run("decisions_thresholds", [] {
        CHECK(needs_brute_force(11, 9, 10) && !needs_brute_force(11, 10, 10) && !needs_brute_force(10, 0, 10) && !needs_brute_force(10, 9, 10));
        CHECK(needs_brute_force(1, 0, 0) == false && needs_brute_force(11, 0, 10));
        CHECK(!store_needs_step_form((int64_t(1) << 28) - 1) && store_needs_step_form(int64_t(1) << 28) && !store_needs_step_form(0));
        CHECK(bf_once_applies(1, 300, 40, true) && !bf_once_applies(0, 300, 40, true) && !bf_once_applies(1, 300, 40, false));
        CHECK(!bf_once_applies(1, 0, 40, true) && !bf_once_applies(1, 300, 0, true));
        CHECK(bf_once_applies(1, PLSLAM_MAX_TRAIN_ROWS, 40, true) && !bf_once_applies(1, PLSLAM_MAX_TRAIN_ROWS + 1, 40, true));
        CHECK(visible_compact_part_words(0) == 1 && visible_compact_part_words(1) == 1 && visible_compact_part_words(256) == 1 &&
              visible_compact_part_words(257) == 2 && VC_NT == 256);
        const plslam_fast_matching ok = grid(64, 48, 0.1, 0.1);
        plslam_fast_matching b1 = ok, b2 = ok, b3 = ok, b4 = ok;
        b1.grid_cols = 0; b2.grid_rows = 0; b3.ws = -1; b4.grid_cols = 1 << 15; b4.grid_rows = 1 << 15;
        CHECK(fast_ok(&ok) && !fast_ok(&b1) && !fast_ok(&b2) && !fast_ok(&b3) && !fast_ok(&b4));
        CHECK(fast_enabled(&ok) && !fast_enabled(nullptr));
        const int32_t idx[] = {-1, 3, -1, -2, 0};
        CHECK((unmatched_features(idx, 5) == V{0, 2}) && unmatched_features(idx, 0).empty());
    });
    run("both_known_needs_every_condition", [] {
        const plslam_fast_matching fm = grid(64, 48, 1.0, 1.0, 1);
        plslam_cam K;
        memset(&K, 0, sizeof(K));
        K.fx = K.fy = 1.0;
        const double DT[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
        const double X[12] = {-10, 5, 1, 70, 60, 1, 10, 10, 1, -10, 5, 1};      // bound: 1 of 2 lines may have candidates
        CHECK(kf2kf_both_known(true, 1, true, false, true, &K, DT, X, 2, &fm, 2));
        CHECK(!kf2kf_both_known(true, 1, true, false, true, &K, DT, X, 2, &fm, 1));     // the bound is not below min_matches
        CHECK(!kf2kf_both_known(false, 1, true, false, true, &K, DT, X, 2, &fm, 2));
        CHECK(!kf2kf_both_known(true, 0, true, false, true, &K, DT, X, 2, &fm, 2));
        CHECK(!kf2kf_both_known(true, 1, false, false, true, &K, DT, X, 2, &fm, 2));
        CHECK(!kf2kf_both_known(true, 1, true, true, true, &K, DT, nullptr, 2, &fm, 2));  // resident rows: the host has no copy to look at
        CHECK(!kf2kf_both_known(true, 1, true, false, false, &K, DT, X, 2, &fm, 2));
    });
    return n_failed ? 1 : 0;
}
