// pgo_graph.hpp -- the host half of the loop-closure pose graph (pgo.hip): the refusals of plslam_pgo_plan_create, the vertices and
// edges of MapHandler::loopClosureOptimizationCovGraphG2O (src/mapHandler.cpp:4198-4290) in creation order, computeInitialGuess's
// BFS tree by levels, the reverse Cuthill-McKee order of the active vertices, the envelope of the reordered system, the H targets
// with their contribution ranges, the right-hand-side lists and the vertex-init rule.  Pure host code: no HIP header, no device, no
// context (tests/cpp/test_pgo_graph.cpp compiles it with g++ alone and runs it under the sanitizers).  The envelope alone
// (envelope_from) also serves plslam_envelope_ldlt_solve (env_ldlt.hip).
#pragma once

#include <stdint.h>

#include <algorithm>
#include <numeric>
#include <vector>

#include "plslam_hip.h"

namespace plslam {

struct PgoPair { int32_t x, y; };             // two int32 the kernels read as one int2 (an edge's vertices; a vertex's init rule)
struct PgoLevel { int32_t v, u, e, first; };  // BFS tree: vertex v set from parent u through edge e (first: u is the edge's first vertex)
struct PgoTarget { int32_t row, col, c0, c1; };  // envelope block (row block >= col block) and its contribution range

// ---- the envelope: first column of every row, offsets, reach --------------------------------------------------------------
struct Envelope {
    std::vector<int64_t> off;     // N + 1
    std::vector<int32_t> cs, reach;
    int32_t bw = 0;               // max over rows of r - cs[r]
};
inline Envelope envelope_from(const std::vector<int32_t>& cs)
{
    Envelope E;
    const int32_t N = (int32_t)cs.size();
    E.cs = cs;
    E.off.assign((size_t)N + 1, 0);
    E.reach.assign(N, 0);
    for (int32_t r = 0; r < N; ++r) {
        E.off[r + 1] = E.off[r] + (r - cs[r] + 1);
        E.bw = std::max(E.bw, r - cs[r]);
    }
    // reach[k] = max { r : cs[r] <= k } (>= k)
    int32_t run = -1;
    std::vector<int32_t> best(N, -1);
    for (int32_t r = 0; r < N; ++r) best[cs[r]] = std::max(best[cs[r]], r);
    for (int32_t k = 0; k < N; ++k) { run = std::max(run, std::max(best[k], k)); E.reach[k] = run; }
    return E;
}

// reverse Cuthill-McKee over the active vertices (adjacency without duplicates): every component from a vertex of least
// degree (lowest index on ties), neighbours by ascending degree (then index); the whole order reversed
inline std::vector<int32_t> rcm_order(const std::vector<std::vector<int32_t>>& adj)
{
    const int32_t n = (int32_t)adj.size();
    std::vector<int32_t> order, deg(n);
    for (int32_t i = 0; i < n; ++i) deg[i] = (int32_t)adj[i].size();
    std::vector<char> seen(n, 0);
    std::vector<int32_t> byd(n);
    std::iota(byd.begin(), byd.end(), 0);
    std::stable_sort(byd.begin(), byd.end(), [&](int32_t a, int32_t b) { return deg[a] < deg[b]; });
    for (int32_t s0 : byd) {
        if (seen[s0]) continue;
        seen[s0] = 1;
        size_t h = order.size();
        order.push_back(s0);
        while (h < order.size()) {
            const int32_t u = order[h++];
            std::vector<int32_t> nb;
            for (int32_t v : adj[u]) if (!seen[v]) { seen[v] = 1; nb.push_back(v); }
            std::stable_sort(nb.begin(), nb.end(), [&](int32_t a, int32_t b) { return deg[a] != deg[b] ? deg[a] < deg[b] : a < b; });
            order.insert(order.end(), nb.begin(), nb.end());
        }
    }
    std::reverse(order.begin(), order.end());
    return order;
}

// everything plslam_pgo_plan_create computes before its first HIP call
struct PgoGraph {
    int32_t n_map = 0, kf_curr = 0, n_lc = 0;
    int32_t nv = 0, ne = 0, na = 0, N = 0, nlvl = 0;    // vertices, edges, active vertices, unknowns (6 na), BFS levels
    std::vector<int32_t> vslot;               // vertex -> map slot
    std::vector<PgoPair> ev;                  // edge -> its two vertices, creation order
    std::vector<int32_t> elc;                 // edge -> its LC entry, -1 for a covisibility edge
    std::vector<PgoLevel> tree;               // the BFS tree from vertex 0, level after level
    std::vector<int32_t> lvl_ptr;             // nlvl + 1 offsets into tree
    std::vector<int32_t> ord;                 // position in the reordered system -> active vertex number (RCM)
    std::vector<int32_t> vcol;                // vertex -> its block column in the reordered system, -1: not active
    Envelope env;
    std::vector<PgoTarget> tg;                // sorted by (row, col)
    std::vector<int32_t> contrib;             // 4 edge + kind, a target's in edge order (K43)
    std::vector<int32_t> rptr, rlist;         // per block column: 2 edge + side, in edge order (K44)
    std::vector<PgoPair> vinit;               // vertex -> (map slot, LC entry that initialises it or -1) (K41)
    const char* why = "";                     // what was refused
};

// PLSLAM_OK, PLSLAM_EINVAL or PLSLAM_ERANGE (G->why says which rule)
inline int pgo_graph_build(const plslam_pgo_params* params, int32_t n_map_kf, const uint8_t* kf_valid, const int32_t* full_graph,
                           int32_t n_lc, const int32_t* lc_idx, PgoGraph* G)
{
#define PGO_REFUSE(cond, code, text) \
    do {                             \
        if (cond) {                  \
            G->why = text;           \
            return code;             \
        }                            \
    } while (0)
    PGO_REFUSE(!params || n_map_kf < 1 || !kf_valid || !full_graph || !lc_idx, PLSLAM_EINVAL, "a NULL argument or no keyframe");
    PGO_REFUSE(n_lc < 1 || params->max_iters_pgo < 0 || params->max_trials < 1, PLSLAM_EINVAL, "no LC entry, or a negative limit");
    PGO_REFUSE(!kf_valid[0], PLSLAM_EINVAL, "keyframe 0 is NULL");
    for (int32_t k = 0; k < n_lc; ++k) {
        const int32_t a = lc_idx[3 * k], b = lc_idx[3 * k + 1];
        PGO_REFUSE(!(a >= 0 && a < n_map_kf && b >= 0 && b < n_map_kf && kf_valid[a] && kf_valid[b] && a != b), PLSLAM_EINVAL,
                   "an LC entry names a NULL or out-of-range keyframe, or one keyframe twice");
    }
    *G = PgoGraph();
    G->n_map = n_map_kf;
    G->n_lc = n_lc;
    int32_t kf_curr = -1;
    for (int32_t k = 0; k < n_lc; ++k) kf_curr = std::max(kf_curr, lc_idx[3 * k + 1]);
    G->kf_curr = kf_curr;
    // vertices: every non-NULL keyframe 0 .. kf_curr (:4210-4249)
    std::vector<int32_t>& vslot = G->vslot;
    std::vector<int32_t> vof(n_map_kf, -1);
    for (int32_t i = 0; i <= kf_curr; ++i) if (kf_valid[i]) { vof[i] = (int32_t)vslot.size(); vslot.push_back(i); }
    const int32_t nv = (int32_t)vslot.size();
    // edges in creation order (:4252-4290): covisibility i ascending, j > i ascending, then one per LC entry
    std::vector<PgoPair>& ev = G->ev;
    std::vector<int32_t>& elc = G->elc;
    const int64_t nm = n_map_kf;
    for (int32_t i = 0; i <= kf_curr; ++i) {
        if (!kf_valid[i]) continue;
        for (int32_t j = i + 1; j <= kf_curr; ++j) {
            const int32_t c = full_graph[(int64_t)i * nm + j];
            if (kf_valid[j] && (c >= params->min_lm_ess_graph || c >= params->min_lm_cov_graph || j - i == 1)) {
                ev.push_back({vof[i], vof[j]});
                elc.push_back(-1);
            }
        }
    }
    for (int32_t k = 0; k < n_lc; ++k) { ev.push_back({vof[lc_idx[3 * k]], vof[lc_idx[3 * k + 1]]}); elc.push_back(k); }
    const int32_t ne = (int32_t)ev.size();
    // incident edges per vertex in creation order; active vertices: not vertex 0, at least one edge
    std::vector<std::vector<int32_t>> inc(nv);
    for (int32_t e = 0; e < ne; ++e) { inc[ev[e].x].push_back(e); inc[ev[e].y].push_back(e); }
    std::vector<int32_t> act;
    for (int32_t v = 1; v < nv; ++v) if (!inc[v].empty()) act.push_back(v);
    PGO_REFUSE(act.empty(), PLSLAM_EINVAL, "no active vertex");
    PGO_REFUSE((int64_t)act.size() > PLSLAM_GBA_MAX_KEYFRAMES, PLSLAM_ERANGE, "more than PLSLAM_GBA_MAX_KEYFRAMES active vertices");
    // computeInitialGuess's BFS tree from vertex 0 (slot 0 is vertex 0), by levels
    std::vector<int32_t> level(nv, -1);
    std::vector<PgoLevel>& tree = G->tree;
    std::vector<int32_t>& lvl_ptr = G->lvl_ptr;
    lvl_ptr.assign(1, 0);
    {
        std::vector<int32_t> q{0};
        level[0] = 0;
        std::vector<std::vector<PgoLevel>> bylvl;
        for (size_t h = 0; h < q.size(); ++h) {
            const int32_t u = q[h];
            for (int32_t e : inc[u]) {
                const int32_t z = ev[e].x == u ? ev[e].y : ev[e].x;
                if (level[z] >= 0) continue;
                level[z] = level[u] + 1;
                if ((int32_t)bylvl.size() < level[z]) bylvl.resize(level[z]);
                bylvl[level[z] - 1].push_back({z, u, e, ev[e].x == u ? 1 : 0});
                q.push_back(z);
            }
        }
        for (auto& L : bylvl) { tree.insert(tree.end(), L.begin(), L.end()); lvl_ptr.push_back((int32_t)tree.size()); }
    }
    for (int32_t v : act) PGO_REFUSE(level[v] < 0, PLSLAM_EINVAL, "an active vertex has no path to vertex 0");   // a singular system
    // the reordered system
    const int32_t na = (int32_t)act.size();
    std::vector<int32_t> aof(nv, -1);
    for (int32_t k = 0; k < na; ++k) aof[act[k]] = k;
    std::vector<std::vector<int32_t>> adj(na);
    for (int32_t e = 0; e < ne; ++e) {
        const int32_t a = aof[ev[e].x], b = aof[ev[e].y];
        if (a >= 0 && b >= 0) { adj[a].push_back(b); adj[b].push_back(a); }
    }
    for (auto& l : adj) { std::sort(l.begin(), l.end()); l.erase(std::unique(l.begin(), l.end()), l.end()); }
    G->ord = rcm_order(adj);
    const std::vector<int32_t>& ord = G->ord;
    std::vector<int32_t> pos(na);
    std::vector<int32_t>& vcol = G->vcol;
    vcol.assign(nv, -1);
    for (int32_t p = 0; p < na; ++p) pos[ord[p]] = p;
    for (int32_t k = 0; k < na; ++k) vcol[act[k]] = pos[k];
    std::vector<int32_t> sblk(na);
    for (int32_t p = 0; p < na; ++p) {
        int32_t s = p;
        for (int32_t nb : adj[ord[p]]) s = std::min(s, pos[nb]);
        sblk[p] = s;
    }
    const int32_t N = 6 * na;
    std::vector<int32_t> cs(N);
    for (int32_t r = 0; r < N; ++r) cs[r] = 6 * sblk[r / 6];
    G->env = envelope_from(cs);
    // H targets: every diagonal block and every (row block > col block) pair an edge joins; contributions in edge order
    struct Ct { int64_t key; int32_t code; };
    std::vector<Ct> cts;
    std::vector<std::vector<int32_t>> rl(na);
    for (int32_t e = 0; e < ne; ++e) {
        const int32_t ci = vcol[ev[e].x], cj = vcol[ev[e].y];
        if (ci >= 0) { cts.push_back({(int64_t)ci * na + ci, 4 * e + 0}); rl[ci].push_back(2 * e + 0); }
        if (cj >= 0) { cts.push_back({(int64_t)cj * na + cj, 4 * e + 1}); rl[cj].push_back(2 * e + 1); }
        if (ci >= 0 && cj >= 0 && ci != cj) {
            if (ci > cj) cts.push_back({(int64_t)ci * na + cj, 4 * e + 2});
            else cts.push_back({(int64_t)cj * na + ci, 4 * e + 3});
        }
    }
    std::stable_sort(cts.begin(), cts.end(), [](const Ct& a, const Ct& b) { return a.key < b.key; });
    std::vector<PgoTarget>& tg = G->tg;
    std::vector<int32_t>& contrib = G->contrib;
    contrib.assign(cts.size(), 0);
    for (size_t i = 0; i < cts.size();) {
        size_t j = i;
        while (j < cts.size() && cts[j].key == cts[i].key) { contrib[j] = cts[j].code; ++j; }
        tg.push_back({(int32_t)(cts[i].key / na), (int32_t)(cts[i].key % na), (int32_t)i, (int32_t)j});
        i = j;
    }
    G->rptr.assign((size_t)na + 1, 0);
    for (int32_t p = 0; p < na; ++p) { G->rlist.insert(G->rlist.end(), rl[p].begin(), rl[p].end()); G->rptr[p + 1] = (int32_t)G->rlist.size(); }
    // vertex init: the LC entry whose (1)-end the vertex is, unless an earlier entry names it as (0) (:4220-4231, break)
    G->vinit.resize(nv);
    for (int32_t v = 0; v < nv; ++v) {
        int32_t id = -1;
        for (int32_t k = 0; k < n_lc; ++k) {
            if (lc_idx[3 * k] == vslot[v]) break;
            if (lc_idx[3 * k + 1] == vslot[v]) { id = k; break; }
        }
        G->vinit[v] = {vslot[v], id};
    }
    G->nv = nv; G->ne = ne; G->na = na; G->N = N; G->nlvl = (int32_t)lvl_ptr.size() - 1;
#undef PGO_REFUSE
    return PLSLAM_OK;
}

}  // namespace plslam
