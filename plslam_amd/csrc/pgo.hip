// pgo.hip -- the loop-closure correction of the reference (MapHandler::loopClosureOptimizationCovGraphG2O,
// src/mapHandler.cpp:4185-4410, up to loopClosureFuseLandmarks()) on the device: the SE(3) pose graph over keyframes 0 ..
// kf_curr_idx optimised with g2o's Levenberg-Marquardt (as restated in tests/pgo_ref.py) and the write-back
// of the poses.  The graph itself is host work (pgo_graph.hpp), g2o's maps are in g2o_dev.hpp, the linear solve in env_ldlt.hip
// (K45-K46; the dense comparison path: ldlt_dense.hip), the re-anchoring of the landmarks in lc_correct.hip (K50-K53).
//   K40 k_pgo_meas             a lane per edge: Z = SE3Quat::exp(reverse_se3(logmap_se3(T_i^-1 T_j))) or of the LC pose
//   K41 k_pgo_init             one workgroup: the :4220-4249 estimates, then computeInitialGuess along the host's BFS tree,
//                              level after level
//   K42 k_pgo_edges<JAC>       a lane per edge: e = toVectorMQT(Z^-1 X_i^-1 X_j), chi2_e, and (JAC) the exact Jacobians
//   K43 k_pgo_hblocks          a workgroup per envelope block: the sum of J^T J over its edges, in edge order
//   K44 k_pgo_rhs              a lane per unknown: b = -sum J^T e over the vertex's edges, in edge order
//   K47 k_pgo_update           a lane per vertex: X' = X fromVectorMQT(dx) (active vertices), X' = X otherwise
//   K48 k_pgo_reduce           one workgroup: chi (fixed order), dx.(lambda dx + b), the bad-pivot flag: what crosses per trial
//   K49 k_pgo_writeback        a lane per vertex: log, expmap_se3, logmap_se3, T_corr; then the keyframes after kf_curr_idx
// Every sum has a fixed order (no floating-point atomics): two runs give the same bits.  Phases are ordered by kernel
// boundaries and, inside the one-workgroup kernels, by workgroup barriers only.
//
// The plan's buffers are named ONCE: each is carved in one function (carve_stat, carve_work), which fills a view of typed
// pointers with the bytes behind each; every launch site, upload and download reads the views.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <limits>
#include <vector>

#include "common.hpp"
#include "env_ldlt.hpp"
#include "g2o_dev.hpp"
#include "ldlt_dense.hpp"
#include "pgo_graph.hpp"

namespace plslam {
namespace {

// the host lists hold pairs of int32 (pgo_graph.hpp has no HIP type); the kernels read the same bytes as int2
static_assert(sizeof(PgoPair) == sizeof(int2) && alignof(PgoPair) <= alignof(int2), "PgoPair is uploaded as int2");

struct PgoStats { double chi, scale; int32_t bad, pad; };
// the two PgoStats the host fetches per trial: the trial's (chi', dx.(lambda dx + b), bad pivots) and the chi of the state
enum : int { PGO_STAT_TRIAL = 0, PGO_STAT_STATE = 1, PGO_N_STATS = 2 };

// ---- K40: measurements ------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
k_pgo_meas(const int2* __restrict__ ev, const int32_t* __restrict__ elc, int32_t ne, const int32_t* __restrict__ vslot,
           const double* __restrict__ T, const double* __restrict__ lc_pose, double* __restrict__ Z)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= ne) return;
    double x[6], u[6];
    if (elc[e] < 0) {
        double Ti[16], Tj[16], Tii[16], Tij[16];
        const int2 p = ev[e];                       // vertices; their map slots index the stored poses
        const size_t si = (size_t)vslot[p.x], sj = (size_t)vslot[p.y];
#pragma unroll
        for (int a = 0; a < 16; ++a) { Ti[a] = T[16 * si + a]; Tj[a] = T[16 * sj + a]; }
        inverse_se3(Ti, Tii);
        mat4_mul(Tii, Tj, Tij);
        logmap_se3(Tij, x);
    } else {
#pragma unroll
        for (int a = 0; a < 6; ++a) x[a] = lc_pose[6 * (size_t)elc[e] + a];
    }
    rev6(x, u);
    Iso Zi;
    se3quat_exp(u, Zi);
    iso_store(Zi, Z + 12 * (size_t)e);
}

// ---- K41: the initial estimates and computeInitialGuess -------------------------------------------------------------------
// vinit[v] = (map slot, LC entry whose (0)-end this vertex is not but whose (1)-end it is, else -1)
__global__ void __launch_bounds__(256)
k_pgo_init(const int2* __restrict__ vinit, int32_t nv, const double* __restrict__ T, const double* __restrict__ x_kf,
           const int32_t* __restrict__ lc_idx, const double* __restrict__ lc_pose, const PgoLevel* __restrict__ tree,
           const int32_t* __restrict__ lvl_ptr, int32_t nlvl, const double* __restrict__ Z, double* __restrict__ X0,
           double* __restrict__ X)
{
    const int t = threadIdx.x;
    for (int v = t; v < nv; v += 256) {
        const int2 vi = vinit[v];
        double x[6], u[6];
        if (vi.y >= 0) {
            double E[16], Ta[16], P[16];
            expmap_se3(lc_pose + 6 * (size_t)vi.y, E);
            const int a = lc_idx[3 * vi.y];
#pragma unroll
            for (int k = 0; k < 16; ++k) Ta[k] = T[16 * (size_t)a + k];
            mat4_mul(E, Ta, P);
            logmap_se3(P, x);
        } else {
#pragma unroll
            for (int k = 0; k < 6; ++k) x[k] = x_kf[6 * (size_t)vi.x + k];
        }
        rev6(x, u);
        Iso Xv;
        se3quat_exp(u, Xv);
        iso_store(Xv, X0 + 12 * (size_t)v);
        iso_store(Xv, X + 12 * (size_t)v);
    }
    for (int l = 0; l < nlvl; ++l) {
        __syncthreads();
        for (int k = lvl_ptr[l] + t; k < lvl_ptr[l + 1]; k += 256) {
            const PgoLevel L = tree[k];
            Iso Xu, Ze, Zi, Xv;
            iso_load(X + 12 * (size_t)L.u, Xu);
            iso_load(Z + 12 * (size_t)L.e, Ze);
            if (L.first) iso_mul(Xu, Ze, Xv);
            else { iso_inv(Ze, Zi); iso_mul(Xu, Zi, Xv); }
            iso_store(Xv, X + 12 * (size_t)L.v);
        }
    }
}

// ---- K42: edge errors and Jacobians ------------------------------------------------------------------------------------------
// J layout per edge: J_i (6 x 6 row-major), then J_j
template <bool JAC>
__global__ void __launch_bounds__(256)
k_pgo_edges(const int2* __restrict__ evs, int32_t ne, const double* __restrict__ Z, const double* __restrict__ X,
            double* __restrict__ err, double* __restrict__ J, double* __restrict__ chi2)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= ne) return;
    const int2 p = evs[e];
    Iso Ze, Xi, Xj, A, Xii, AX, E;
    iso_load(Z + 12 * (size_t)e, Ze);
    iso_load(X + 12 * (size_t)p.x, Xi);
    iso_load(X + 12 * (size_t)p.y, Xj);
    iso_inv(Ze, A);
    iso_inv(Xi, Xii);
    iso_mul(A, Xii, AX);
    iso_mul(AX, Xj, E);
    double q[4];
    unit_quat(E.R, q);
    const double ev[6] = {E.t[0], E.t[1], E.t[2], q[1], q[2], q[3]};
    double c = 0.0;
#pragma unroll
    for (int a = 0; a < 6; ++a) c += ev[a] * ev[a];
    chi2[e] = c;
    if (!JAC) return;
#pragma unroll
    for (int a = 0; a < 6; ++a) err[6 * (size_t)e + a] = ev[a];
    Iso B, EB;
    iso_mul(Xii, Xj, B);
    iso_mul(A, B, EB);
    double qb[4];
    unit_quat(EB.R, qb);
    const double w = qb[0], v[3] = {qb[1], qb[2], qb[3]};
    double S[9], Sb[9];
    skew3(v, S);
    skew3(B.t, Sb);
    double Ji[36], Jj[36];
#pragma unroll
    for (int k = 0; k < 36; ++k) { Ji[k] = 0.0; Jj[k] = 0.0; }
    double RS[9], M[9], Mr[9];
    mat3_mul(A.R, Sb, RS);
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        const double id = (k % 4 == 0) ? 1.0 : 0.0;
        M[k] = w * id + S[k];      // w I + [v]x
        Mr[k] = w * id - S[k];     // w I - [v]x
    }
    double MA[9];
    mat3_mul(Mr, A.R, MA);
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c2 = 0; c2 < 3; ++c2) {
            Jj[6 * r + c2] = EB.R[3 * r + c2];
            Jj[6 * (r + 3) + 3 + c2] = M[3 * r + c2];
            Ji[6 * r + c2] = -A.R[3 * r + c2];
            Ji[6 * r + 3 + c2] = 2.0 * RS[3 * r + c2];
            Ji[6 * (r + 3) + 3 + c2] = -MA[3 * r + c2];
        }
    double* o = J + 72 * (size_t)e;
#pragma unroll
    for (int k = 0; k < 36; ++k) { o[k] = Ji[k]; o[36 + k] = Jj[k]; }
}

// ---- K43: Hessian blocks in the envelope ------------------------------------------------------------------------------------
// contribution code c: edge = c >> 2, kind = c & 3: 0 J_i^T J_i, 1 J_j^T J_j, 2 J_i^T J_j, 3 J_j^T J_i
__global__ void __launch_bounds__(64)
k_pgo_hblocks(const PgoTarget* __restrict__ tg, const int32_t* __restrict__ contrib, const double* __restrict__ J,
              const int64_t* __restrict__ off, const int32_t* __restrict__ cs, double* __restrict__ H)
{
    const PgoTarget T = tg[blockIdx.x];
    const int t = threadIdx.x;
    if (t >= 36) return;
    const int r = t / 6, c = t % 6;
    const int64_t gr = 6 * (int64_t)T.row + r, gc = 6 * (int64_t)T.col + c;
    if (gc > gr) return;
    double acc = 0.0;
    for (int k = T.c0; k < T.c1; ++k) {
        const int32_t code = contrib[k];
        const int kind = code & 3;
        const double* Je = J + 72 * (size_t)(code >> 2);
        const double* Ja = Je + ((kind == 1 || kind == 3) ? 36 : 0);
        const double* Jb = Je + ((kind == 1 || kind == 2) ? 36 : 0);
        double s = 0.0;
#pragma unroll
        for (int m = 0; m < 6; ++m) s += Ja[6 * m + r] * Jb[6 * m + c];
        acc += s;
    }
    H[off[gr] + (gc - cs[gr])] = acc;
}

// ---- K44: b = -sum J^T e -----------------------------------------------------------------------------------------------------
// rhs_list entry: edge << 1 | side (0: the vertex is the edge's first end)
__global__ void __launch_bounds__(256)
k_pgo_rhs(const int32_t* __restrict__ rptr, const int32_t* __restrict__ rlist, int32_t na, const double* __restrict__ J,
          const double* __restrict__ err, double* __restrict__ b)
{
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= 6 * na) return;
    const int p = g / 6, r = g % 6;
    double acc = 0.0;
    for (int k = rptr[p]; k < rptr[p + 1]; ++k) {
        const int32_t code = rlist[k];
        const int e = code >> 1;
        const double* Jv = J + 72 * (size_t)e + 36 * (code & 1);
        double s = 0.0;
#pragma unroll
        for (int m = 0; m < 6; ++m) s += Jv[6 * m + r] * err[6 * (size_t)e + m];
        acc -= s;
    }
    b[g] = acc;
}

// ---- K47: the trial update ---------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
k_pgo_update(const int32_t* __restrict__ vcol, int32_t nv, const double* __restrict__ dx, const int32_t* __restrict__ nbad,
             const double* __restrict__ X, double* __restrict__ Y)
{
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= nv) return;
    Iso Xv, D, Yv;
    iso_load(X + 12 * (size_t)v, Xv);
    const int c = vcol[v];
    if (c < 0 || *nbad) { iso_store(Xv, Y + 12 * (size_t)v); return; }
    double d[6];
#pragma unroll
    for (int a = 0; a < 6; ++a) d[a] = dx[6 * (size_t)c + a];
    from_vector_mqt(d, D);
    iso_mul(Xv, D, Yv);
    iso_store(Yv, Y + 12 * (size_t)v);
}

// ---- K48: the scalars of a trial -------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
k_pgo_reduce(const double* __restrict__ chi2, int32_t ne, const double* __restrict__ dx, const double* __restrict__ b, int32_t N,
             double lambda, const int32_t* __restrict__ nbad, PgoStats* __restrict__ out)
{
    __shared__ double rc[256], rs[256];
    const int t = threadIdx.x;
    double c = 0.0, s = 0.0;
    for (int e = t; e < ne; e += 256) c += chi2[e];
    if (dx && !*nbad)
        for (int k = t; k < N; k += 256) s += dx[k] * (lambda * dx[k] + b[k]);
    rc[t] = c; rs[t] = s;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (t < h) { rc[t] += rc[t + h]; rs[t] += rs[t + h]; }
        __syncthreads();
    }
    if (t == 0) { out->chi = rc[0]; out->scale = rs[0]; out->bad = nbad ? *nbad : 0; out->pad = 0; }
}

// ---- K49: write-back ---------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
k_pgo_writeback(const int32_t* __restrict__ vslot, const int32_t* __restrict__ vcol, int32_t nv, const double* __restrict__ X,
                const double* __restrict__ X0, const double* __restrict__ T, double* __restrict__ T_out, double* __restrict__ x_out,
                double* __restrict__ T_corr)
{
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= nv) return;
    const size_t k = (size_t)vslot[v];
    Iso Xv;
    iso_load((vcol[v] >= 0 ? X : X0) + 12 * (size_t)v, Xv);
    double u[6], x[6], Tk[16], Tp[16], Tpi[16], Tc[16];
    se3quat_log(Xv, u);
    rev6(u, x);
    expmap_se3(x, Tk);
    logmap_se3(Tk, u);
#pragma unroll
    for (int a = 0; a < 16; ++a) Tp[a] = T[16 * k + a];
    inverse_se3(Tp, Tpi);
    mat4_mul(Tk, Tpi, Tc);
#pragma unroll
    for (int a = 0; a < 16; ++a) { T_out[16 * k + a] = Tk[a]; T_corr[16 * k + a] = Tc[a]; }
#pragma unroll
    for (int a = 0; a < 6; ++a) x_out[6 * k + a] = u[a];
}
__global__ void __launch_bounds__(256)
k_pgo_later(const uint8_t* __restrict__ valid, int32_t k0, int32_t n, int32_t last, const double* __restrict__ T,
            double* __restrict__ T_out, double* __restrict__ x_out, double* __restrict__ T_corr, uint8_t* __restrict__ corrected)
{
    const int k = k0 + blockIdx.x * 256 + threadIdx.x;
    if (k >= n || !valid[k]) return;
    double C[16], Tk[16], To[16], u[6];
#pragma unroll
    for (int a = 0; a < 16; ++a) { C[a] = T_corr[16 * (size_t)last + a]; Tk[a] = T[16 * (size_t)k + a]; }
    mat4_mul(C, Tk, To);
    logmap_se3(To, u);
#pragma unroll
    for (int a = 0; a < 16; ++a) { T_out[16 * (size_t)k + a] = To[a]; T_corr[16 * (size_t)k + a] = C[a]; }
#pragma unroll
    for (int a = 0; a < 6; ++a) x_out[6 * (size_t)k + a] = u[a];
    corrected[k] = 1;
}

struct PgoStatView {               // `stat`: the graph's lists (pgo_graph.hpp: PgoGraph) -- uploaded once
    Arr<int2> ev;
    Arr<int32_t> elc;
    Arr<int2> vinit;
    Arr<int32_t> lc_idx;
    Arr<PgoLevel> tree;
    Arr<int32_t> lvl_ptr;
    Arr<PgoTarget> tg;
    Arr<int32_t> contrib, rptr, rlist;
    Arr<int64_t> off;
    Arr<int32_t> cs, reach, vcol, vslot;
    Arr<uint8_t> valid;
};
struct PgoWorkView {               // `work`: a call's inputs, the state and everything an iteration computes, the outputs
    Arr<double> T, x_in, lc_pose;                     // the stored poses (per map slot) and the LC poses, as given
    Arr<double> Z, X0, Xa, Xb;                        // measurements; the :4220-4249 estimates; the state and the trial state
    Arr<double> err, J, chi2, H, b;                   // the linearisation
    Arr<double> L, z, zg, dx;                         // the solve (z, dx: npad doubles -- the dense path writes them too)
    Arr<int32_t> nbad;
    Arr<PgoStats> stats;                              // PGO_N_STATS of them
    Arr<double> T_out, x_out, T_corr;
    Arr<uint8_t> corrected;
    Arr<double> P, w;                                 // the dense comparison path only (ldlt_dense.hpp)
    Arr<int32_t> badp;
};

}  // namespace
}  // namespace plslam

using namespace plslam;

struct plslam_pgo_plan {
    plslam_ctx* ctx = nullptr;
    plslam_pgo_params prm{};
    PgoGraph g;                               // the host-built graph; its counts size every launch
    int64_t npad = 0;
    bool dense = false;                       // the tool-only dense comparison path (context option "pgo_solver" = 1)
    DevBuf stat, work, Sbuf;
    PgoStatView st;
    PgoWorkView wk;

    EnvDev env() const { return EnvDev{st.off, st.cs, st.reach, g.N, g.env.bw}; }
    void release() { stat.release(); work.release(); Sbuf.release(); }
};

namespace {

size_t carve_stat(plslam_pgo_plan* P, char* base)
{
    const PgoGraph& g = P->g;
    PgoStatView& v = P->st;
    ArrCarver c{base};
    v.ev = c.take<int2>(g.ev.size() * sizeof(int2));
    v.elc = c.take<int32_t>(g.elc.size() * 4);
    v.vinit = c.take<int2>(g.vinit.size() * sizeof(int2));
    v.lc_idx = c.take<int32_t>((size_t)g.n_lc * 12);
    v.tree = c.take<PgoLevel>(g.tree.size() * sizeof(PgoLevel), 16);
    v.lvl_ptr = c.take<int32_t>(g.lvl_ptr.size() * 4);
    v.tg = c.take<PgoTarget>(g.tg.size() * sizeof(PgoTarget), 16);
    v.contrib = c.take<int32_t>(g.contrib.size() * 4, 4);
    v.rptr = c.take<int32_t>(g.rptr.size() * 4);
    v.rlist = c.take<int32_t>(g.rlist.size() * 4, 4);
    v.off = c.take<int64_t>(g.env.off.size() * 8);
    v.cs = c.take<int32_t>((size_t)g.N * 4);
    v.reach = c.take<int32_t>((size_t)g.N * 4);
    v.vcol = c.take<int32_t>((size_t)g.nv * 4);
    v.vslot = c.take<int32_t>((size_t)g.nv * 4);
    v.valid = c.take<uint8_t>((size_t)g.n_map, 8);
    return c.size();
}

size_t carve_work(plslam_pgo_plan* P, char* base)
{
    const PgoGraph& g = P->g;
    PgoWorkView& v = P->wk;
    ArrCarver c{base};
    const size_t nm = (size_t)g.n_map, nv = (size_t)g.nv, ne = (size_t)g.ne, N = (size_t)g.N, npad = (size_t)P->npad;
    const size_t entries = (size_t)g.env.off[g.N];
    v.T = c.take<double>(nm * 128);
    v.x_in = c.take<double>(nm * 48);
    v.lc_pose = c.take<double>((size_t)g.n_lc * 48);
    v.Z = c.take<double>(ne * 96);
    v.X0 = c.take<double>(nv * 96);
    v.Xa = c.take<double>(nv * 96);
    v.Xb = c.take<double>(nv * 96);
    v.err = c.take<double>(ne * 48);
    v.J = c.take<double>(ne * 576);
    v.chi2 = c.take<double>(ne * 8);
    v.H = c.take<double>(entries * 8);
    v.b = c.take<double>(N * 8);
    v.L = c.take<double>(entries * 8);
    v.z = c.take<double>(npad * 8);
    v.zg = c.take<double>(N * 8);
    v.dx = c.take<double>(npad * 8);
    v.nbad = c.take<int32_t>(4, 4);
    v.stats = c.take<PgoStats>(PGO_N_STATS * sizeof(PgoStats));
    v.T_out = c.take<double>(nm * 128);
    v.x_out = c.take<double>(nm * 48);
    v.T_corr = c.take<double>(nm * 128);
    v.corrected = c.take<uint8_t>(nm, 8);
    if (P->dense) {
        v.P = c.take<double>(npad * LT * 8);
        v.w = c.take<double>(npad * 8);
        v.badp = c.take<int32_t>((npad / LT) * 4, 4);
    }
    return c.size();
}

int pgo_fail(plslam_pgo_plan* P, int rc)
{
    P->release();
    delete P;
    return rc;
}

// chi of the state X into the stats' PGO_STAT_STATE (JAC: with the errors and Jacobians of a linearisation at X)
template <bool JAC>
void pgo_state_chi_enqueue(plslam_pgo_plan* P, const double* X, hipStream_t s)
{
    const PgoStatView& st = P->st;
    const PgoWorkView& wk = P->wk;
    const int32_t ne = P->g.ne;
    hipLaunchKernelGGL(k_pgo_edges<JAC>, dim3((ne + 255) / 256), dim3(256), 0, s, (const int2*)st.ev, ne, (const double*)wk.Z, X,
                       wk.err.p, wk.J.p, wk.chi2.p);
    hipLaunchKernelGGL(k_pgo_reduce, dim3(1), dim3(256), 0, s, (const double*)wk.chi2, ne, (const double*)nullptr,
                       (const double*)nullptr, 0, 0.0, (const int32_t*)nullptr, wk.stats.p + PGO_STAT_STATE);
}

// one trial: factor and solve (H + lambda I) dx = b, X' = X fromVectorMQT(dx), chi' and dx.(lambda dx + b)
int pgo_trial_enqueue(plslam_pgo_plan* P, double lambda, const double* X, double* Y, hipStream_t s)
{
    const PgoGraph& g = P->g;
    const PgoStatView& st = P->st;
    const PgoWorkView& wk = P->wk;
    const EnvDev E = P->env();
    int rc;
    if (!P->dense) {
        if ((rc = env_solve_enqueue(E, wk.H, lambda, wk.b, wk.L, wk.z, wk.zg, wk.dx, wk.nbad, s))) return rc;
    } else {
        double* S = P->Sbuf.as<double>();
        PLSLAM_HIP_CHECK(hipMemsetAsync(S, 0, (size_t)P->npad * (size_t)P->npad * 8, s));
        PLSLAM_HIP_CHECK(hipMemsetAsync(wk.w, 0, wk.w.bytes, s));
        env_to_dense_enqueue(E, wk.H, P->npad, lambda, wk.b, S, wk.w, s);
        if ((rc = ldlt_enqueue(S, P->npad, g.N, wk.P, wk.w, wk.z, wk.dx, wk.badp, s))) return rc;
        ldlt_count_bad_enqueue(wk.badp, (int32_t)(P->npad / LT), wk.nbad, s);
    }
    hipLaunchKernelGGL(k_pgo_update, dim3((g.nv + 255) / 256), dim3(256), 0, s, (const int32_t*)st.vcol, g.nv, (const double*)wk.dx,
                       (const int32_t*)wk.nbad, X, Y);
    hipLaunchKernelGGL(k_pgo_edges<false>, dim3((g.ne + 255) / 256), dim3(256), 0, s, (const int2*)st.ev, g.ne, (const double*)wk.Z,
                       (const double*)Y, wk.err.p, wk.J.p, wk.chi2.p);
    hipLaunchKernelGGL(k_pgo_reduce, dim3(1), dim3(256), 0, s, (const double*)wk.chi2, g.ne, (const double*)wk.dx,
                       (const double*)wk.b, g.N, lambda, (const int32_t*)wk.nbad, wk.stats.p + PGO_STAT_TRIAL);
    PLSLAM_HIP_CHECK(hipGetLastError());
    return PLSLAM_OK;
}

// the linearisation at X: errors, Jacobians, chi, H blocks, b
int pgo_linearise_enqueue(plslam_pgo_plan* P, const double* X, hipStream_t s)
{
    const PgoGraph& g = P->g;
    const PgoStatView& st = P->st;
    const PgoWorkView& wk = P->wk;
    pgo_state_chi_enqueue<true>(P, X, s);
    if (!g.tg.empty())
        hipLaunchKernelGGL(k_pgo_hblocks, dim3((unsigned)g.tg.size()), dim3(64), 0, s, (const PgoTarget*)st.tg, (const int32_t*)st.contrib,
                           (const double*)wk.J, (const int64_t*)st.off, (const int32_t*)st.cs, wk.H.p);
    hipLaunchKernelGGL(k_pgo_rhs, dim3((6 * g.na + 255) / 256), dim3(256), 0, s, (const int32_t*)st.rptr, (const int32_t*)st.rlist,
                       g.na, (const double*)wk.J, (const double*)wk.err, wk.b.p);
    PLSLAM_HIP_CHECK(hipGetLastError());
    return PLSLAM_OK;
}

}  // namespace

extern "C" {

// check the pointers, plan (pgo_graph.hpp), carve and upload, return
int plslam_pgo_plan_create(plslam_ctx* ctx, const plslam_pgo_params* params, int32_t n_map_kf, const uint8_t* kf_valid,
                           const int32_t* full_graph, int32_t n_lc, const int32_t* lc_idx, plslam_pgo_plan** out)
{
    PLSLAM_REQUIRE(ctx && out, PLSLAM_EINVAL);
    *out = nullptr;
    plslam_pgo_plan* P = new (std::nothrow) plslam_pgo_plan();
    PLSLAM_REQUIRE(P != nullptr, PLSLAM_ENOMEM);
    int rc = pgo_graph_build(params, n_map_kf, kf_valid, full_graph, n_lc, lc_idx, &P->g);
    if (rc) {
        set_last_error("plslam_pgo_plan_create: %s", P->g.why);
        return pgo_fail(P, rc);
    }
    const PgoGraph& g = P->g;
    P->ctx = ctx; P->prm = *params;
    P->dense = ctx->pgo_solver == 1; P->npad = pad_to_tile(g.N);
    if ((rc = P->stat.reserve(carve_stat(P, nullptr) + 256)) || (rc = P->work.reserve(carve_work(P, nullptr) + 256)) ||
        (P->dense && (rc = P->Sbuf.reserve((size_t)P->npad * (size_t)P->npad * 8))))
        return pgo_fail(P, rc);
    carve_stat(P, P->stat.as<char>());
    carve_work(P, P->work.as<char>());
    {
        std::lock_guard<std::mutex> lk(ctx->mu);
        DeviceGuard dg_(ctx->device);
        hipStream_t s = ctx->stream;
        const PgoStatView& st = P->st;
        const UploadItem ups[] = {{st.ev, g.ev.data()}, {st.elc, g.elc.data()}, {st.vinit, g.vinit.data()}, {st.lc_idx, lc_idx},
                                  {st.tree, g.tree.data()}, {st.lvl_ptr, g.lvl_ptr.data()}, {st.tg, g.tg.data()},
                                  {st.contrib, g.contrib.data()}, {st.rptr, g.rptr.data()}, {st.rlist, g.rlist.data()},
                                  {st.off, g.env.off.data()}, {st.cs, g.env.cs.data()}, {st.reach, g.env.reach.data()},
                                  {st.vcol, g.vcol.data()}, {st.vslot, g.vslot.data()}, {st.valid, kf_valid}};
        rc = upload_items(ups, s);
        if (hipStreamSynchronize(s) != hipSuccess && !rc) rc = PLSLAM_EHIP;
        if (rc) return pgo_fail(P, rc);
    }
    *out = P;
    return PLSLAM_OK;
}

int plslam_pgo_optimize(plslam_pgo_plan* P, const double* T_kf_w, const double* x_kf_w, const double* lc_pose, double* T_out,
                        double* x_out, double* T_corr, uint8_t* corrected, plslam_pgo_trial* trace, int32_t trace_cap,
                        plslam_pgo_result* result)
{
    PLSLAM_REQUIRE(P && T_kf_w && x_kf_w && lc_pose && T_out && x_out && T_corr && corrected && trace_cap >= 0 &&
                   (trace_cap == 0 || trace), PLSLAM_EINVAL);
    plslam_ctx* ctx = P->ctx;
    std::lock_guard<std::mutex> lk(ctx->mu);
    DeviceGuard dg_(ctx->device);
    hipStream_t s = ctx->stream;
    StreamSyncOnError guard(s);
    const PgoGraph& g = P->g;
    const PgoStatView& st = P->st;
    const PgoWorkView& wk = P->wk;
    const size_t nm = (size_t)g.n_map;
    {
        const UploadItem in[] = {{wk.T, T_kf_w}, {wk.x_in, x_kf_w}, {wk.lc_pose, lc_pose}};
        int r = upload_items(in, s);
        if (r) return r;
    }
    hipLaunchKernelGGL(k_pgo_meas, dim3((g.ne + 255) / 256), dim3(256), 0, s, (const int2*)st.ev, (const int32_t*)st.elc, g.ne,
                       (const int32_t*)st.vslot, (const double*)wk.T, (const double*)wk.lc_pose, wk.Z.p);
    hipLaunchKernelGGL(k_pgo_init, dim3(1), dim3(256), 0, s, (const int2*)st.vinit, g.nv, (const double*)wk.T,
                       (const double*)wk.x_in, (const int32_t*)st.lc_idx, (const double*)wk.lc_pose, (const PgoLevel*)st.tree,
                       (const int32_t*)st.lvl_ptr, g.nlvl, (const double*)wk.Z, wk.X0.p, wk.Xa.p);
    PLSLAM_HIP_CHECK(hipMemsetAsync(wk.H, 0, wk.H.bytes, s));
    PLSLAM_HIP_CHECK(hipGetLastError());
    double* Xs[2] = {wk.Xa, wk.Xb};
    int cur = 0;
    PgoStats stats[PGO_N_STATS];
    auto fetch = [&]() -> int {
        PLSLAM_HIP_CHECK(hipMemcpyAsync(stats, wk.stats, sizeof(stats), hipMemcpyDeviceToHost, s));
        PLSLAM_HIP_CHECK(hipStreamSynchronize(s));
        return PLSLAM_OK;
    };
    int rc;
    pgo_state_chi_enqueue<false>(P, Xs[cur], s);          // chi of the initial guess
    if ((rc = fetch())) return rc;
    const double chi_initial = stats[PGO_STAT_STATE].chi;
    double lambda = P->prm.lambda_init, ni = 2.0;
    int32_t iters = 0, trials = 0, stop = PLSLAM_PGO_STOP_MAX_ITERS;
    for (int32_t it = 0; it < P->prm.max_iters_pgo; ++it) {
        if ((rc = pgo_linearise_enqueue(P, Xs[cur], s))) return rc;
        if (it == 0) { lambda = P->prm.lambda_init; ni = 2.0; }
        int32_t q = 0;
        double rho = 0.0;
        iters = it + 1;
        do {
            if ((rc = pgo_trial_enqueue(P, lambda, Xs[cur], Xs[cur ^ 1], s)) || (rc = fetch())) return rc;
            const PgoStats& tr = stats[PGO_STAT_TRIAL];
            const double chi = stats[PGO_STAT_STATE].chi;
            const bool ok = tr.bad == 0;
            const double chi_new = ok ? tr.chi : DBL_MAX;
            const double scale = tr.scale + 1e-3;
            rho = (chi - chi_new) / scale;
            const double lam_used = lambda;
            const bool acc = rho > 0 && std::isfinite(chi_new);
            if (acc) {
                const double a = 1.0 - std::pow(2.0 * rho - 1.0, 3);
                lambda *= std::max(1.0 / 3.0, std::min(a, 2.0 / 3.0));
                ni = 2.0;
                cur ^= 1;
            } else {
                lambda *= ni;
                ni *= 2.0;
            }
            if (trials < trace_cap) {
                plslam_pgo_trial& t = trace[trials];
                t.iteration = it; t.trial = q; t.lambda = lam_used; t.chi = chi; t.chi_new = chi_new; t.scale = scale; t.rho = rho;
                t.ok = ok ? 1 : 0; t.accepted = acc ? 1 : 0;
            }
            ++trials;
            ++q;
        } while (rho < 0 && q < P->prm.max_trials);
        if (q == P->prm.max_trials || rho == 0) { stop = PLSLAM_PGO_STOP_TERMINATE; break; }
    }
    // chi of the final state, then the write-back (:4298-4304) and the keyframes after kf_curr (:4358-4362)
    pgo_state_chi_enqueue<false>(P, Xs[cur], s);
    {
        std::vector<double> I(nm * 16, 0.0);
        for (size_t k = 0; k < nm; ++k) for (int a = 0; a < 4; ++a) I[16 * k + 5 * a] = 1.0;
        std::vector<uint8_t> cflag(nm, 0);
        for (int32_t v : g.vslot) cflag[v] = 1;
        const UploadItem start[] = {{wk.T_out, T_kf_w}, {wk.x_out, x_kf_w}, {wk.T_corr, I.data()}, {wk.corrected, cflag.data()}};
        if ((rc = upload_items(start, s))) return rc;
        hipLaunchKernelGGL(k_pgo_writeback, dim3((g.nv + 255) / 256), dim3(256), 0, s, (const int32_t*)st.vslot,
                           (const int32_t*)st.vcol, g.nv, (const double*)Xs[cur], (const double*)wk.X0, (const double*)wk.T,
                           wk.T_out.p, wk.x_out.p, wk.T_corr.p);
        const int32_t k0 = g.kf_curr + 1;
        if (k0 < g.n_map)
            hipLaunchKernelGGL(k_pgo_later, dim3((g.n_map - k0 + 255) / 256), dim3(256), 0, s, (const uint8_t*)st.valid, k0, g.n_map,
                               g.kf_curr, (const double*)wk.T, wk.T_out.p, wk.x_out.p, wk.T_corr.p, wk.corrected.p);
        PLSLAM_HIP_CHECK(hipGetLastError());
        const DownloadItem back[] = {{T_out, wk.T_out, wk.T_out.bytes}, {x_out, wk.x_out, wk.x_out.bytes},
                                     {T_corr, wk.T_corr, wk.T_corr.bytes}, {corrected, wk.corrected, wk.corrected.bytes}};
        for (const DownloadItem& d : back) PLSLAM_HIP_CHECK(hipMemcpyAsync(d.dst, d.src, d.bytes, hipMemcpyDeviceToHost, s));
        if ((rc = fetch())) return rc;
    }
    guard.dismiss();
    if (result) {
        result->iterations = iters; result->trials = trials; result->stop_reason = stop; result->n_vertices = g.nv;
        result->n_active = g.na; result->n_edges = g.ne; result->n_lc_edges = g.n_lc; result->env_width = g.env.bw;
        result->env_entries = g.env.off[g.N]; result->chi_initial = chi_initial; result->chi_final = stats[PGO_STAT_STATE].chi;
        result->lambda = lambda;
    }
    return PLSLAM_OK;
}

void plslam_pgo_plan_destroy(plslam_pgo_plan* P)
{
    if (!P) return;
    {
        std::lock_guard<std::mutex> lk(P->ctx->mu);
        DeviceGuard dg_(P->ctx->device);
        (void)hipStreamSynchronize(P->ctx->stream);
        P->release();
    }
    delete P;
}

}  // extern "C"
