// map2kf_plan.hpp -- the pure host half of the map <-> keyframe and keyframe <-> keyframe drivers (map2kf.hip): the GridStructure
// of the keyframe features in CSR form, the argument checks and early returns of the two drivers, the layout of every staged
// block (each offset named once), the host staging of the one-synchronisation forms, the one filler of plslam_grid_problem and
// the reference's decisions as functions.  No HIP in here, no context, no device: tests/cpp/test_map2kf_plan.cpp compiles it
// with g++ alone and runs it under the sanitizers.  Addresses called "device" are only added to, never read through; sizes that
// HIP-side code decides (sizeof(GridDesc), grid_aux_words, the dense kernel's answer) come in as numbers.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "match_grid_layout.hpp"
#include "match_tables.hpp"   // align256, Carver
#include "plslam_hip.h"

namespace plslam {

// ---- the GridStructure of the keyframe features -------------------------------------------------------------------------------
// getLineCoords of stvo-pl ([RECALL]; the callers' grid fill :693-697): Bresenham cells, the last x excluded
inline void line_cells(double x1, double y1, double x2, double y2, std::vector<int32_t>& xy)
{
    xy.clear();
    const bool steep = std::fabs(y2 - y1) > std::fabs(x2 - x1);
    if (steep) { std::swap(x1, y1); std::swap(x2, y2); }
    if (x1 > x2) { std::swap(x1, x2); std::swap(y1, y2); }
    const double dx = x2 - x1, dy = std::fabs(y2 - y1);
    double error = dx / 2.0;
    const int ystep = (y1 < y2) ? 1 : -1;
    int y = (int)y1;
    const int maxX = (int)x2;
    for (int x = (int)x1; x < maxX; x++) {
        xy.push_back(steep ? y : x);
        xy.push_back(steep ? x : y);
        error -= dy;
        if (error < 0) { y += ystep; error += dx; }
    }
}

// GridStructure fill in CSR form: `cells` lists (item, x, y) in push_back order
inline void csr_fill(const std::vector<int32_t>& item, const std::vector<int32_t>& cx, const std::vector<int32_t>& cy,
                     int32_t cols, int32_t rows, std::vector<int32_t>& cs, std::vector<int32_t>& items)
{
    cs.assign((size_t)cols * rows + 1, 0);
    for (size_t k = 0; k < item.size(); ++k)
        if (cx[k] >= 0 && cx[k] < cols && cy[k] >= 0 && cy[k] < rows) ++cs[(size_t)cx[k] * rows + cy[k] + 1];
    for (size_t c = 0; c < (size_t)cols * rows; ++c) cs[c + 1] += cs[c];
    items.assign((size_t)cs.back() + 1, 0);
    std::vector<int32_t> fill(cs.begin(), cs.end() - 1);
    for (size_t k = 0; k < item.size(); ++k)
        if (cx[k] >= 0 && cx[k] < cols && cy[k] >= 0 && cy[k] < rows) items[(size_t)fill[(size_t)cx[k] * rows + cy[k]]++] = item[k];
}

inline int32_t cvtt_x86(double v)   // as the reference's x86 build converts (cvttsd2si): NaN / out of range -> INT_MIN
{
    return (v > -2147483649.0 && v < 2147483648.0) ? (int32_t)v : INT32_MIN;
}

// the GridStructure of the keyframe features feat_curr[sel ? sel[b] : b], b < nt, in CSR form (points: the feature's cell,
// :581-584; lines: the Bresenham cells of (spl, epl), :686-698) and, for lines, their directions
struct GridTables {
    std::vector<int32_t> cs, items;     // cols * rows + 1 cell starts; n_items + 1 items
    std::vector<double> dir2;           // lines: nt x 2
    int32_t n_items = 0;
};
inline GridTables fill_grid_tables(int lines, const double* feat_curr, const int32_t* sel, int32_t nt, const plslam_fast_matching* fm)
{
    GridTables g;
    const int32_t cols = fm->grid_cols, rows = fm->grid_rows;
    std::vector<int32_t> it, cx, cy, xy;
    if (!lines) {
        for (int32_t b = 0; b < nt; ++b) {
            const double* p = feat_curr + 2 * (size_t)(sel ? sel[b] : b);
            it.push_back(b);
            cx.push_back(cvtt_x86(p[0] * fm->inv_width));
            cy.push_back(cvtt_x86(p[1] * fm->inv_height));
        }
    } else {
        g.dir2.resize((size_t)nt * 2);
        for (int32_t b = 0; b < nt; ++b) {
            const double* sg = feat_curr + 4 * (size_t)(sel ? sel[b] : b);
            double vx = (sg[2] - sg[0]) * fm->inv_width, vy = (sg[3] - sg[1]) * fm->inv_height;
            const double magnitude = std::sqrt(vx * vx + vy * vy);
            g.dir2[2 * (size_t)b] = vx / magnitude;
            g.dir2[2 * (size_t)b + 1] = vy / magnitude;
            line_cells(sg[0] * fm->inv_width, sg[1] * fm->inv_height, sg[2] * fm->inv_width, sg[3] * fm->inv_height, xy);
            for (size_t k = 0; k + 1 < xy.size(); k += 2) {
                it.push_back(b);
                cx.push_back(xy[k]);
                cy.push_back(xy[k + 1]);
            }
        }
    }
    csr_fill(it, cx, cy, cols, rows, g.cs, g.items);
    g.n_items = g.cs.back();
    return g;
}

// capacity of matchGrid's candidate store from the grid alone (match_grid_layout.hpp), every window fm->ws wide
inline int64_t grid_tables_capacity(const GridTables& g, int32_t n1, int32_t n_centres, const plslam_fast_matching* fm, int mutual)
{
    const int32_t win[4] = {fm->ws, fm->ws, fm->ws, fm->ws};
    return grid_store_capacity_bound(n1, n_centres, g.cs.data(), fm->grid_cols, fm->grid_rows, win, mutual);
}

// ---- other pure helpers ---------------------------------------------------------------------------------------------------------
// An upper bound of what the windowed matcher can find for the KF<->KF LINE call, from the host's copy of the previous key frame's
// lines: a row can only match if one of its two window centres has a grid cell in its window.  The reference hands matchGrid the
// projected end points in PIXELS there (:392-393; the point call scales by the grid, :256), so on a 752 x 480 image nearly every
// window lies outside the 64 x 48 grid and the windowed pass finds next to nothing -- StVO::match runs behind it (:421-425) in
// practically every call.  When this bound is below min_matches that is KNOWN before anything is launched, and the driver
// enqueues both matchers and waits once.  Conservative: the host's projection may differ from the device's in the last bit, so a
// centre within two cells of the window's reach, or not finite, counts as "may have candidates".
inline int32_t kf2kf_line_grid_bound(const plslam_cam* K, const double* DT, const double* sPeP, int32_t n, const plslam_fast_matching* fm)
{
    const double reach = (double)fm->ws + 2.0;
    int32_t may = 0;
    for (int32_t i = 0; i < n; ++i) {
        bool any = false;
        for (int e = 0; e < 2 && !any; ++e) {
            const double* X = sPeP + 6 * (size_t)i + 3 * e;
            double P[3];
            for (int r = 0; r < 3; ++r) P[r] = DT[4 * r] * X[0] + DT[4 * r + 1] * X[1] + DT[4 * r + 2] * X[2] + DT[4 * r + 3];
            const double u = K->cx + K->fx * P[0] / P[2], v = K->cy + K->fy * P[1] / P[2];
            const bool out = u < -reach || u > (double)fm->grid_cols + reach || v < -reach || v > (double)fm->grid_rows + reach;
            any = !out;                            // (NaN compares false everywhere: "may")
        }
        may += any;
    }
    return may;
}

inline bool fast_ok(const plslam_fast_matching* fm)
{
    return fm->grid_cols >= 1 && fm->grid_rows >= 1 && fm->ws >= 0 && (int64_t)fm->grid_cols * fm->grid_rows < (int64_t(1) << 30);
}

// T list (host only): unmatched keyframe features, :563-569 / :668-674
inline std::vector<int32_t> unmatched_features(const int32_t* kf_idx, int32_t n_kf)
{
    std::vector<int32_t> ti;
    for (int32_t i = 0; i < n_kf; ++i)
        if (kf_idx[i] == -1) ti.push_back(i);
    return ti;
}

// k_visible_compact (map2kf_kernels.hip): landmarks per workgroup, and the zeroed device words its workgroups chain their counts
// through
constexpr int VC_NT = 256;
inline size_t visible_compact_part_words(int32_t n) { return (size_t)(n > 0 ? (n + VC_NT - 1) / VC_NT : 1); }

// ---- the argument checks and early returns of the two drivers ----------------------------------------------------------------
// Inside the library PLSLAM_REQUIRE is common.hpp's, which also records the refused rule as the last error; compiled without it
// (the CPU test) a refusal is its code alone
#ifndef PLSLAM_REQUIRE
#define PLSLAM_REQUIRE(cond, code) do { if (!(cond)) return (code); } while (0)
#endif

// What a driver does with its arguments: refuse (the code is not PLSLAM_OK), return with nothing written to the table, fill the
// table with -1 and return, or run.  The counters (n_matches, used_match) are zeroed and the table is filled in the order the
// checks stand in: zero_counts / fill_table say what has happened when a later rule refuses.
enum EntryDo { ENTRY_REFUSE, ENTRY_RETURN, ENTRY_FILL_RETURN, ENTRY_RUN };
struct Entry {
    EntryDo what = ENTRY_REFUSE;
    bool zero_counts = false, fill_table = false;
};
// true: run
inline bool entry_apply(const Entry& e, int32_t* table, int32_t n, int32_t* n_matches, int32_t* used_match)
{
    if (e.zero_counts) {
        if (n_matches) *n_matches = 0;
        if (used_match) *used_match = 0;
    }
    if (e.fill_table)
        for (int32_t i = 0; i < n; ++i) table[i] = -1;
    return e.what == ENTRY_RUN;
}

inline bool fast_enabled(const plslam_fast_matching* fm) { return fm && fm->enabled; }

// MapHandler::matchMap2KFPoints / Lines; ti: the unmatched keyframe features (filled when the checks get that far)
inline int map2kf_entry(const void* ctx, const plslam_cam* K, const double* Twf, int lines, const void* LM, const void* med_desc,
                        const void* candidate, int32_t n_map, const void* kf_desc, const void* kf_feat, const void* kf_seg,
                        const int32_t* kf_idx, int32_t n_kf, int32_t min_matches, const plslam_fast_matching* fm,
                        const void* map_to_kf, Entry& e, std::vector<int32_t>& ti)
{
    e = Entry{};
    PLSLAM_REQUIRE(ctx && K && Twf && n_map >= 0 && n_kf >= 0, PLSLAM_EINVAL);
    if (fast_enabled(fm)) {
        PLSLAM_REQUIRE(fast_ok(fm), PLSLAM_EINVAL);
        PLSLAM_REQUIRE(!lines || kf_seg || n_kf == 0, PLSLAM_EINVAL);
    }
    e.zero_counts = true;
    if (n_map == 0) { e.what = ENTRY_RETURN; return PLSLAM_OK; }
    PLSLAM_REQUIRE(LM && med_desc && candidate && map_to_kf, PLSLAM_EINVAL);
    PLSLAM_REQUIRE(n_kf == 0 || (kf_desc && kf_feat && kf_idx), PLSLAM_EINVAL);
    e.fill_table = true;
    e.what = ENTRY_FILL_RETURN;
    ti = unmatched_features(kf_idx, n_kf);
    if (ti.empty()) return PLSLAM_OK;                                     // :571 / :676
    // no matcher would run at all (:594 / :709 with no table from matchGrid: matches = 0 < min_matches is the condition)
    if (!fast_enabled(fm) && !(0 < min_matches)) return PLSLAM_OK;
    e.what = ENTRY_RUN;
    return PLSLAM_OK;
}

// StVO::match behind (or instead of) matchGrid can run at all, :274 / :421
inline bool kf2kf_bf_possible(int32_t n_prev, int32_t n_curr, int32_t min_matches) { return n_curr > min_matches && n_prev > min_matches; }

// MapHandler::matchKF2KFPoints / Lines; rows_dev: X_prev, desc_prev and desc_curr are device pointers (16-byte aligned rows)
inline int kf2kf_entry(const void* ctx, const plslam_cam* K, const double* DT, const void* X_prev, const void* desc_prev,
                       int32_t n_prev, const void* feat_curr, const void* desc_curr, int32_t n_curr, int32_t min_matches,
                       const plslam_fast_matching* fm, const void* matches_12, bool rows_dev, Entry& e)
{
    e = Entry{};
    PLSLAM_REQUIRE(ctx && K && DT && n_prev >= 0 && n_curr >= 0, PLSLAM_EINVAL);
    if (fast_enabled(fm)) PLSLAM_REQUIRE(fast_ok(fm), PLSLAM_EINVAL);
    e.zero_counts = true;
    if (n_prev == 0) { e.what = ENTRY_RETURN; return PLSLAM_OK; }
    PLSLAM_REQUIRE(matches_12 != nullptr, PLSLAM_EINVAL);
    e.fill_table = true;
    if (n_curr == 0) { e.what = ENTRY_FILL_RETURN; return PLSLAM_OK; }    // :243 / :368
    PLSLAM_REQUIRE(X_prev && desc_prev && feat_curr && desc_curr, PLSLAM_EINVAL);
    if (rows_dev)
        PLSLAM_REQUIRE((reinterpret_cast<uintptr_t>(desc_prev) & 15) == 0 && (reinterpret_cast<uintptr_t>(desc_curr) & 15) == 0 &&
                           (reinterpret_cast<uintptr_t>(X_prev) & 7) == 0,
                       PLSLAM_EINVAL);
    e.what = ENTRY_FILL_RETURN;
    if (!fast_enabled(fm) && !(kf2kf_bf_possible(n_prev, n_curr, min_matches) && 0 < min_matches)) return PLSLAM_OK;   // no matcher would run
    e.what = ENTRY_RUN;
    return PLSLAM_OK;
}

// ---- the layouts: every slice on a multiple of 256 bytes, in the order named ----------------------------------------------------
// sizes of the grid slices of an image: what fill_grid_tables gave and what the matcher's own code says
struct GridSizes { size_t cs_words, n_items, desc_bytes, aux_words; };

// The one-synchronisation forms of the map <-> keyframe driver.  One image up:
//   [map | med_desc | cand, unless the map is resident] | T rows | their features | ti | [cell_start | items | directions |
//   matchGrid's descriptor | its shared words] | counters (gate count, nq, matchGrid's count, publish ticket) | k_visible_compact's
//   chain (zero)
// and behind it, device only: the association table -- directly behind the counters' pages, so that counters + table come down
// in ONE copy of pin_out bytes, the table at tab_out of it -- | the list | Q | its landmarks | [window centres | directions] |
// the matcher's table | the gate's mask.  grid = nullptr: the brute-force form, which is the fast form without its grid slices.
struct OnceLayout {
    size_t oLM, oMD, oCand, oT, oTF, oTi, oCs, oIt, oD2, oDesc, oAux, oRes, oPart, image;
    size_t oMap, oQi, oQ, oQL, oCen, oD1, oM, oMask, bytes;
    size_t part_bytes, tab_out, pin_out;
    OnceLayout(int lines, bool map_dev, int32_t n_map, int32_t nt, const GridSizes* grid)
    {
        const size_t lw = lines ? 6 : 3, fw = lines ? 3 : 2, nc = lines ? 2 : 1, nm = (size_t)n_map, n2 = (size_t)nt;
        Carver c;
        oLM = c.take(map_dev ? 0 : nm * lw * 8); oMD = c.take(map_dev ? 0 : nm * 32); oCand = c.take(map_dev ? 0 : nm);
        oT = c.take(n2 * 32); oTF = c.take(n2 * fw * 8); oTi = c.take(n2 * 4);
        oCs = c.take(grid ? grid->cs_words * 4 : 0); oIt = c.take(grid ? (grid->n_items + 1) * 4 : 0);
        oD2 = c.take(grid && lines ? n2 * 16 : 0); oDesc = c.take(grid ? grid->desc_bytes : 0);
        oAux = c.take(grid ? grid->aux_words * 4 : 0);
        oRes = c.take(16);
        part_bytes = visible_compact_part_words(n_map) * 4;
        oPart = c.take(part_bytes);
        image = c.off;
        oMap = c.take(nm * 4); oQi = c.take(nm * 4); oQ = c.take(nm * 32); oQL = c.take(nm * lw * 8);
        oCen = c.take(grid ? nm * nc * 8 : 0); oD1 = c.take(grid && lines ? nm * 16 : 0);
        oM = c.take(nm * 4); oMask = c.take(nm);
        bytes = c.off;
        tab_out = oMap - oRes;
        pin_out = tab_out + nm * 4;
    }
};

// The step-by-step form: image 1 [map | med_desc, unless resident] | keyframe descriptors | features; image 2 (the two lists,
// staged in the same page-locked block once image 1 is on the device) qi | ti; device only: visibility flags | Q | T | their
// landmarks / features; one results block: the matcher's table | the gate's mask | its count
struct StepLayout {
    size_t oLM, oMD, oKD, oKF, image1, oQi, oTi, image2, oVis, oQ, oT, oQL, oTF, oM, oMask, oCnt, results, bytes;
    size_t pin_in, pin_out;
    StepLayout(int lines, bool map_dev, int32_t n_map, int32_t n_kf, int32_t nt)
    {
        const size_t lw = lines ? 6 : 3, fw = lines ? 3 : 2, nm = (size_t)n_map, nk = (size_t)n_kf, n2 = (size_t)nt;
        Carver c;
        oLM = c.take(map_dev ? 0 : nm * lw * 8); oMD = c.take(map_dev ? 0 : nm * 32); oKD = c.take(nk * 32); oKF = c.take(nk * fw * 8);
        image1 = c.off;
        oQi = c.take(nm * 4); oTi = c.take(n2 * 4);
        image2 = c.off - oQi;
        oVis = c.take(nm); oQ = c.take(nm * 32); oT = c.take(n2 * 32); oQL = c.take(nm * lw * 8); oTF = c.take(n2 * fw * 8);
        oM = c.take(nm * 4); oMask = c.take(nm); oCnt = c.take(8);
        results = c.off - oM;
        bytes = c.off;
        pin_in = std::max(image1, image2);
        pin_out = std::max(results, nm);       // (the visibility flags come back through it first)
    }
};

// grid_path's image (host -> device in one copy): result words | cell_start | items | directions | descriptor | shared words;
// behind it, device only: the projected cells and the query directions
struct GridPathLayout {
    size_t oSt, oCs, oIt, oD2, oDesc, oAux, image, oCen, oD1, bytes;
    GridPathLayout(int lines, int32_t nq, int32_t nt, const GridSizes& g)
    {
        const size_t nc = lines ? 2 : 1;
        Carver c;
        oSt = c.take(16); oCs = c.take(g.cs_words * 4); oIt = c.take((g.n_items + 1) * 4);
        oD2 = c.take(lines ? (size_t)nt * 16 : 0); oDesc = c.take(g.desc_bytes); oAux = c.take(g.aux_words * 4);
        image = c.off;
        oCen = c.take((size_t)nq * nc * 8); oD1 = c.take(lines ? (size_t)nq * 16 : 0);
        bytes = c.off;
    }
};

// kf2kf_driver: ONE image [desc_prev | desc_curr | X_prev] (X only when the windowed matcher runs; nothing when the rows are
// resident); device only: the match table | its count.  pin_out: the table and, behind it, the count
struct Kf2kfLayout {
    size_t oQ, oT, oX, image, oM, oCnt, bytes, pin_out;
    Kf2kfLayout(int lines, bool rows_dev, bool fast, int32_t n_prev, int32_t n_curr)
    {
        const size_t xw = lines ? 6 : 3;
        Carver c;
        oQ = c.take(rows_dev ? 0 : (size_t)n_prev * 32); oT = c.take(rows_dev ? 0 : (size_t)n_curr * 32);
        oX = c.take(fast && !rows_dev ? (size_t)n_prev * xw * 8 : 0);
        image = c.off;
        oM = c.take((size_t)n_prev * 4); oCnt = c.take(16);
        bytes = c.off;
        pin_out = (size_t)n_prev * 4 + 256;
    }
};

// ---- staging ------------------------------------------------------------------------------------------------------------------
// the host-built grid tables into the image at h (L: a layout with oCs, oIt, oD2)
template <class L>
inline void stage_grid_tables(const L& l, char* h, int lines, int32_t nt, const GridTables& g)
{
    memcpy(h + l.oCs, g.cs.data(), g.cs.size() * 4);
    memcpy(h + l.oIt, g.items.data(), (size_t)(g.n_items + 1) * 4);
    if (lines) memcpy(h + l.oD2, g.dir2.data(), (size_t)nt * 16);
}

// the image of the one-synchronisation forms at h: the map unless it is resident, the T matrix and its features gathered by ti
// (:563-569), ti, the grid tables (g = nullptr: the brute-force form), zeroed counters and chain words.  (The matcher's own
// slices -- descriptor, shared words -- are filled by its code.)
inline void stage_once_image(const OnceLayout& l, char* h, int lines, bool map_dev, const double* LM, const uint8_t* med_desc,
                             const uint8_t* candidate, int32_t n_map, const uint8_t* kf_desc, const double* kf_feat,
                             const std::vector<int32_t>& ti, const GridTables* g)
{
    const size_t lw = lines ? 6 : 3, fw = lines ? 3 : 2;
    const int32_t nt = (int32_t)ti.size();
    if (!map_dev) {
        memcpy(h + l.oLM, LM, (size_t)n_map * lw * 8);
        memcpy(h + l.oMD, med_desc, (size_t)n_map * 32);
        memcpy(h + l.oCand, candidate, (size_t)n_map);
    }
    for (int32_t b = 0; b < nt; ++b) {
        memcpy(h + l.oT + (size_t)b * 32, kf_desc + (size_t)ti[b] * 32, 32);
        memcpy(h + l.oTF + (size_t)b * fw * 8, kf_feat + (size_t)ti[b] * fw, fw * 8);
    }
    memcpy(h + l.oTi, ti.data(), (size_t)nt * 4);
    if (g) stage_grid_tables(l, h, lines, nt, *g);
    memset(h + l.oRes, 0, 16);
    memset(h + l.oPart, 0, l.part_bytes);
}

// The one filler of plslam_grid_problem (L: a layout with oCs, oIt, oD2, oCen, oD1).  dev: the device block; img: the base the
// kernels see the uploaded image at (dev itself, or the page-locked block read in place); the slices a kernel writes (window
// centres, query directions) are always in dev.  d1 / d2: the descriptor matrices (device), n1 rows (or their upper bound) x nt.
template <class L>
inline plslam_grid_problem fill_grid_problem(const L& l, char* dev, char* img, int lines, const uint8_t* d1, int32_t n1,
                                             const uint8_t* d2, int32_t nt, int32_t n_items, const plslam_fast_matching* fm,
                                             int mutual, int64_t cap, int32_t* matches_12, int32_t* n_matches)
{
    plslam_grid_problem q{};
    q.d1 = d1; q.d2 = d2; q.centres1 = (int32_t*)(dev + l.oCen);
    q.cell_start = (int32_t*)(img + l.oCs); q.cell_items = (int32_t*)(img + l.oIt);
    q.dir1 = lines ? (double*)(dev + l.oD1) : nullptr; q.dir2 = lines ? (double*)(img + l.oD2) : nullptr;
    q.n1 = n1; q.n2 = nt; q.n_centres = lines ? 2 : 1; q.grid_cols = fm->grid_cols; q.grid_rows = fm->grid_rows; q.n_items = n_items;
    for (int k = 0; k < 4; ++k) q.window[k] = fm->ws;
    q.sim_th = fm->line_sim_th; q.nnr = fm->nnr_grid; q.mutual = mutual ? 1 : 0;
    q.pair_capacity = (int32_t)cap;
    q.matches_12 = matches_12; q.n_matches = n_matches;
    return q;
}

// ---- the reference's decisions ------------------------------------------------------------------------------------------------
// :594-598 / :709-713 (and :274 / :421 per keyframe pair): matchGrid found too little (or did not run: matches = 0) and there are
// enough rows: StVO::match runs
inline bool needs_brute_force(int32_t nq, int32_t matches, int32_t min_matches) { return nq > min_matches && matches < min_matches; }

// a candidate store sized for every landmark of a huge map: the step-by-step form sizes it for the list
inline bool store_needs_step_form(int64_t cap) { return cap >= (int64_t(1) << 28); }

// the brute-force one-synchronisation form applies: its plan is sized for the bound n_map, not for |Q|, and must take a device-
// side row count (takes_row_count: the context's answer; the form is mutual only)
inline bool bf_once_applies(int mutual, int32_t n_map, int32_t nt, bool takes_row_count)
{
    return mutual && n_map <= PLSLAM_MAX_TRAIN_ROWS && takes_row_count && n_map > 0 && nt > 0;
}

// KF<->KF lines: the windowed pass provably stays below min_matches (kf2kf_line_grid_bound), so StVO::match is enqueued behind it
// at once: one synchronisation for the call instead of two
inline bool kf2kf_both_known(bool fast, int lines, bool bf_possible, bool rows_dev, bool has_mapped, const plslam_cam* K,
                             const double* DT, const double* X_prev, int32_t n_prev, const plslam_fast_matching* fm, int32_t min_matches)
{
    return fast && lines && bf_possible && !rows_dev && has_mapped && kf2kf_line_grid_bound(K, DT, X_prev, n_prev, fm) < min_matches;
}

// Where StVO::match of the KF<->KF driver writes its table.  keep_prior: matchGrid filled a table that is handed on (:271 -> :277,
// :418 -> :424); on_host: that table is in the page-locked block; has_mapped: the device can address the block.
//   mapped: matches_12 is the block's device address (else the device table); upload_first: the block's table goes to the device
//   table first; count_only: the table stays in the block and only the counter comes back (by a one-lane launch behind it);
//   count_entries: StVO::match on a fresh vector in the block: the count is the number of entries; on_host: where the table is
//   once the matcher is enqueued.
// (keep_prior && on_host && has_mapped: the finalize kernel reads the earlier entry of a rejected row and writes every row: a few
// hundred to a few thousand 4-byte accesses to page-locked memory cost less than moving the table to the device and back.)
struct Kf2kfTable { bool mapped, upload_first, count_only, count_entries, on_host; };
inline Kf2kfTable kf2kf_table(bool keep_prior, bool on_host, bool has_mapped)
{
    if (keep_prior && on_host && has_mapped) return {true, false, true, false, true};
    if (keep_prior) return {false, on_host, false, false, false};
    return {has_mapped, false, false, has_mapped, has_mapped};
}

}  // namespace plslam
