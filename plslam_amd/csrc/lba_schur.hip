// lba_schur.hip -- the Schur step on the resident blocks (round 5) -- the consumer of plslam_lba_plan_iterate_dev / _resident.
//
// The reference solves the damped normal equations whole: H(i,i) += lambda * H(i,i), H.sparseView(), SimplicialLDLT
// (src/mapHandler.cpp:1552-1556; :1779-1783 in the loop) -- N = 6 Nkf + 3 Npt + 6 Nls unknowns, 42 054 at C3.  H has the block
// structure the plan's iteration already produces, and the landmark blocks are independent of each other, so the same system is
//     S dp = b,   S = Hpp' - sum_j Wj^T Vj'^-1 Wj,   b = gp - sum_j Wj^T Vj'^-1 gj,   dxj = Vj'^-1 (gj - Wj dp)
// with Hpp' / Vj' the damped pose / landmark blocks and Wj the cross blocks of landmark j's observations: 6 Nkf unknowns (60 at
// C3) for the host's dense LDLT, everything else stays on the device.  What crosses PCIe per iteration is S and b down (29 kB at
// C3) and dp up (480 B) instead of 11.5 MB of blocks.  Algebraically the reference's solve; numerically equal to rounding
// (tests/test_gpu_lba.py compares with a dense solve of the assembled system).
//
// No atomics, nothing scheduling-dependent (as everywhere in this file): the pairs (o1, o2) of observations of one landmark that
// fall into block (k1 <= k2) of S are listed ONCE per plan on the host, sorted by block; a block's sum is a fixed-shape two-level
// sum -- chunks of SCH_CHUNK pairs sequentially in list order, then the chunk partials in chunk order -- and the lower triangle
// is the mirror of the upper one, block by block (inside a DIAGONAL block all 36 entries are summed, each over its own products:
// S(a,b) and S(b,a) there agree to rounding, not to the bit).  A sequential program in this order reproduces every word of S, b,
// the steps and their sum of squares: tests/lba_schur_ref.py is one, tests/test_gpu_lba_schur_edges.py compares with it.
//   K19 k_schur_landmarks       a lane per landmark: Vj' inverse (Gauss-Jordan without pivoting, 3x3 and 6x6 alike: schur_landmark
//                               in lba_blocks_dev.hpp), tj = Vj'^-1 gj
//   K20 k_schur_partials        a lane per (block, chunk, entry of the 6x6 block): sum over the chunk's pairs of W1^T Vinv W2
//   K21 (in K20's launch)       a lane per (keyframe, chunk, entry of b): sum over the chunk's observations of W^T tj
//   K22 k_schur_finish          a lane per (block, entry) / (keyframe, entry): chunk partials -> S (both triangles), b
//   K23 k_schur_backsub         a lane per (landmark, row): dxj = tj - Vinv_j sum_o W_o dp[kf(o)]  (+ the update of Xw / Lw in place)
//   K24 k_lba_diag_max          max |H(i,i)| over all diagonal entries (the reference's lambda *= Hmax, :1544-1550)
#include <algorithm>
#include <cstring>

#include "lba_plan.hpp"

using namespace plslam;

namespace plslam {

// one launch for both kinds: workgroups [0, nb3) take the points, the rest the lines
__global__ void __launch_bounds__(256)
k_schur_landmarks(const double* __restrict__ H_pt, const double* __restrict__ g_pt, int32_t npt, const double* __restrict__ H_ls,
                  const double* __restrict__ g_ls, int32_t nls, int32_t nb3, double lambda, double* __restrict__ Vp,
                  double* __restrict__ tp, double* __restrict__ Vl, double* __restrict__ tl, int32_t* __restrict__ nsing)
{
    if ((int)blockIdx.x < nb3) {
        const int j = blockIdx.x * 256 + threadIdx.x;
        if (j < npt) schur_landmark<3>(H_pt, g_pt, j, lambda, Vp, tp, nsing);
    } else {
        const int j = ((int)blockIdx.x - nb3) * 256 + threadIdx.x;
        if (j < nls) schur_landmark<6>(H_ls, g_ls, j, lambda, Vl, tl, nsing);
    }
}

// (plslam_lba_plan_optimize_dev, lba_lm_dev.hip: the same kernels behind the loop's stop word, the damping read from its control block)
__global__ void __launch_bounds__(256)
k_schur_landmarks_lm(const double* __restrict__ H_pt, const double* __restrict__ g_pt, int32_t npt, const double* __restrict__ H_ls,
                     const double* __restrict__ g_ls, int32_t nls, int32_t nb3, const LbaLmCtl* __restrict__ ctl, double* __restrict__ Vp,
                     double* __restrict__ tp, double* __restrict__ Vl, double* __restrict__ tl, int32_t* __restrict__ nsing)
{
    if (ctl->stop != LM_RUNNING) return;
    const double lambda = ctl->lambda;
    if ((int)blockIdx.x < nb3) {
        const int j = blockIdx.x * 256 + threadIdx.x;
        if (j < npt) schur_landmark<3>(H_pt, g_pt, j, lambda, Vp, tp, nsing);
    } else {
        const int j = ((int)blockIdx.x - nb3) * 256 + threadIdx.x;
        if (j < nls) schur_landmark<6>(H_ls, g_ls, j, lambda, Vl, tl, nsing);
    }
}

// W_pt[o]: 3 x 6 (landmark row x, pose column a), W_ls[o]: 6 x 6.  Entry (a, b) of W1^T Vinv W2 = sum_x sum_y W1[x][a] Vinv[x][y] W2[y][b].
// A workgroup = one chunk of SCH_CHUNK pairs: lane i computes the whole 6 x 6 contribution of pair i (its loads are one round
// trip: a first form with a lane per entry walking the chunk was a chain of 64 dependent round trips, 177 us per call at C3),
// parks it in LDS, and lane e < 36 adds the 64 values of entry e SEQUENTIALLY in pair order -- the same sum, term for term.
template <int DL>
__device__ __forceinline__ void schur_pair_product(const double (&w1)[DL * 6], const double (&w2)[DL * 6], const double (&v)[DL * DL],
                                                   double* __restrict__ out /* [36], stride 1 */)
{
#pragma unroll
    for (int b = 0; b < 6; ++b) {
        double u[DL];
#pragma unroll
        for (int x = 0; x < DL; ++x) {
            double t = 0.0;
#pragma unroll
            for (int y = 0; y < DL; ++y) t += v[x * DL + y] * w2[y * 6 + b];
            u[x] = t;
        }
#pragma unroll
        for (int a = 0; a < 6; ++a) {
            double sacc = 0.0;
#pragma unroll
            for (int x = 0; x < DL; ++x) sacc += w1[x * 6 + a] * u[x];
            out[a * 6 + b] = sacc;
        }
    }
}
template <int DL>
__device__ __forceinline__ void schur_pair_block(const double* __restrict__ W1, const double* __restrict__ W2,
                                                 const double* __restrict__ V, double* __restrict__ out /* [36], stride 1 */)
{
    double w1[DL * 6], w2[DL * 6], v[DL * DL];
#pragma unroll
    for (int i = 0; i < DL * 6; ++i) { w1[i] = W1[i]; w2[i] = W2[i]; }
#pragma unroll
    for (int i = 0; i < DL * DL; ++i) v[i] = V[i];
    schur_pair_product<DL>(w1, w2, v, out);
}

// 64 rows of NE doubles, row r at base + NE * id(r) where lane r holds id(r): fetched by the WAVE in runs (consecutive lanes read
// consecutive words of a row: 4-8 cache lines per instruction; a lane reading its own row word by word touches 64), parked in
// the tile, and every lane takes its own row out of it.  One wave per workgroup: the barriers are the wave's own.
// One chunk per workgroup of one wave.  Measured at C3: two or four chunks
// per workgroup, a wave each with its own tile and wave-level synchronisation, are SLOWER (24.0 / 24.9 us against 19.8: a
// workgroup's LDS and registers stay taken until its slowest wave is through), and so is the wave-level form at one wave (22.3: the
// scheduler takes the weaker barrier as leave to spread the gathers' loads over 285 registers).
__device__ __forceinline__ void wave_sync()
{
    __syncthreads();
}
// (fetch: the loads, into registers -- several gathers' loads can be in flight together; park: through the tile, one at a time)
template <int NE>
__device__ __forceinline__ void gather_fetch(const double* __restrict__ base, int id, double (&flat)[NE])
{
    const int lane = threadIdx.x & 63;
    typedef double f64x2 __attribute__((ext_vector_type(2)));
    if constexpr (NE % 2 == 0) {
        constexpr int H = NE / 2;
#pragma unroll
        for (int j = 0; j < H; ++j) {
            const int idx = j * 64 + lane, r = idx / H, c2 = idx - r * H;
            const int rid = __shfl(id, r);
            // (a 32-bit byte offset from the uniform base: the load takes it beside the base in scalar registers -- a 64-bit
            // address per load was two more registers for each of the 18 loads in flight; lba_schur_prepare bounds the tables)
            const uint32_t boff = ((uint32_t)rid * NE + 2 * c2) * 8u;
            const f64x2 v = *reinterpret_cast<const f64x2*>(reinterpret_cast<const char*>(base) + boff);
            flat[2 * j] = v.x;
            flat[2 * j + 1] = v.y;
        }
    } else {
#pragma unroll
        for (int j = 0; j < NE; ++j) {
            const int idx = j * 64 + lane, r = idx / NE, c = idx - r * NE;
            const int rid = __shfl(id, r);
            const uint32_t boff = ((uint32_t)rid * NE + c) * 8u;
            flat[j] = *reinterpret_cast<const double*>(reinterpret_cast<const char*>(base) + boff);
        }
    }
}
// (park_only: the rows stay in the tile -- every lane reads its own row from there as it goes; the caller synchronises before the
// tile's next use)
template <int NE>
__device__ __forceinline__ void gather_park_only(double (*tile)[37], const double (&flat)[NE])
{
    static_assert(NE <= 36 && NE % 2 == 0, "the tile is 37 doubles wide");
    const int lane = threadIdx.x & 63;
    constexpr int H = NE / 2;
#pragma unroll
    for (int j = 0; j < H; ++j) {
        const int idx = j * 64 + lane, r = idx / H, c2 = idx - r * H;
        tile[r][2 * c2] = flat[2 * j];
        tile[r][2 * c2 + 1] = flat[2 * j + 1];
    }
    wave_sync();
}
template <int NE>
__device__ __forceinline__ void gather_park(double (*tile)[37], const double (&flat)[NE], double (&row_out)[NE])
{
    static_assert(NE <= 36, "the tile is 37 doubles wide");
    const int lane = threadIdx.x & 63;
    if constexpr (NE % 2 == 0) {
        constexpr int H = NE / 2;
#pragma unroll
        for (int j = 0; j < H; ++j) {
            const int idx = j * 64 + lane, r = idx / H, c2 = idx - r * H;
            tile[r][2 * c2] = flat[2 * j];
            tile[r][2 * c2 + 1] = flat[2 * j + 1];
        }
    } else {
#pragma unroll
        for (int j = 0; j < NE; ++j) {
            const int idx = j * 64 + lane, r = idx / NE, c = idx - r * NE;
            tile[r][c] = flat[j];
        }
    }
    wave_sync();
#pragma unroll
    for (int e = 0; e < NE; ++e) row_out[e] = tile[lane][e];
    wave_sync();
}
template <int NE>
__device__ __forceinline__ void gather_rows(double (*tile)[37], const double* __restrict__ base, int id, double (&row_out)[NE])
{
    double flat[NE];
    gather_fetch<NE>(base, id, flat);
    gather_park<NE>(tile, flat, row_out);
}

__device__ __forceinline__ void
schur_partials_wg(double (*tile)[37], int B, int c, const SchurPair* __restrict__ pairs, const int32_t* __restrict__ blk_ptr,
                  const double* __restrict__ W_pt, const double* __restrict__ W_ls, const double* __restrict__ Vp,
                  const double* __restrict__ Vl, int32_t max_chunks, double* __restrict__ part /* [nblk][max_chunks][36] */)
{
    const int i = threadIdx.x & 63;
    const int beg = blk_ptr[B] + c * SCH_CHUNK;
    const int end = beg + SCH_CHUNK < blk_ptr[B + 1] ? beg + SCH_CHUNK : blk_ptr[B + 1];
    const int n = end - beg;                       // <= 0: the block has fewer chunks than the grid is wide
    if (n <= 0) return;
    SchurPair q = pairs[beg + (i < n ? i : n - 1)];           // (lanes past the chunk's end replay its last pair: their block is dropped)
    // the chunk's kind (lba_schur_prepare: one kind per chunk, null pairs -- line = 2 -- behind a block's last point pairs); a null
    // pair fetches what the chunk's first pair fetches and contributes zeros
    const bool null_pair = q.line == 2;
    if (null_pair) { q.o1 = __shfl(q.o1, 0); q.o2 = __shfl(q.o2, 0); q.lm = __shfl(q.lm, 0); }
    const bool line_chunk = __shfl(q.line, 0) == 1;
    // The wave fetches its 64 pairs' rows together (gather_*), each lane takes its own out of the tile, and the pair's 6 x 6 block
    // goes straight back into the tile (the sums are schur_pair_product's, term for term).  Registers: what a lane holds at once
    // decides how many waves a SIMD keeps (a first form with all operands and the block in registers: 256 and one wave; this one: two).
    if (!line_chunk) {
        double w1[18], w2[18], v[9];
        {
            double f1[18], f2[18], fv[9];
            gather_fetch<18>(W_pt, q.o1, f1);      // (the three gathers' loads: one round trip)
            gather_fetch<18>(W_pt, q.o2, f2);
            gather_fetch<9>(Vp, q.lm, fv);
            gather_park<18>(tile, f1, w1);
            gather_park<18>(tile, f2, w2);
            gather_park<9>(tile, fv, v);
        }
#pragma unroll
        for (int b = 0; b < 6; ++b) {
            double u[3];
#pragma unroll
            for (int x = 0; x < 3; ++x) {
                double t = 0.0;
#pragma unroll
                for (int y = 0; y < 3; ++y) t += v[x * 3 + y] * w2[y * 6 + b];
                u[x] = t;
            }
#pragma unroll
            for (int a = 0; a < 6; ++a) {
                double sacc = 0.0;
#pragma unroll
                for (int x = 0; x < 3; ++x) sacc += w1[x * 6 + a] * u[x];
                tile[i][a * 6 + b] = null_pair ? 0.0 : sacc;
            }
        }
    } else {
        // W2, then Y = Vinv W2 (column b of a lane's W2 row is dead once Y's column b is known: Y overwrites W2 in place), then W1,
        // and entry (a, b) = sum_x W1[x][a] Y[x][b] lands where W1[b][a] was (column a of W1 is dead by then): the block sits
        // TRANSPOSED in the tile, and the lanes that add the chunk's blocks read it so
        {
            double v[36];
            {
                double fv[36], f2[36];
                gather_fetch<36>(Vl, q.lm, fv);
                gather_fetch<36>(W_ls, q.o2, f2);
                gather_park<36>(tile, fv, v);
                gather_park_only<36>(tile, f2);
            }
#pragma unroll
            for (int b = 0; b < 6; ++b) {
                double w2c[6], yc[6];
#pragma unroll
                for (int y = 0; y < 6; ++y) w2c[y] = tile[i][y * 6 + b];
#pragma unroll
                for (int x = 0; x < 6; ++x) {
                    double t = 0.0;
#pragma unroll
                    for (int y = 0; y < 6; ++y) t += v[x * 6 + y] * w2c[y];
                    yc[x] = t;                     // u[x] of column b
                }
#pragma unroll
                for (int x = 0; x < 6; ++x) tile[i][x * 6 + b] = yc[x];
            }
        }
        double Y[36];
#pragma unroll
        for (int e = 0; e < 36; ++e) Y[e] = tile[i][e];
        {
            double f1[36];
            gather_fetch<36>(W_ls, q.o1, f1);
            wave_sync();                       // (every lane has taken its Y)
            gather_park_only<36>(tile, f1);
        }
#pragma unroll
        for (int a = 0; a < 6; ++a) {
            double w1c[6], oc[6];
#pragma unroll
            for (int x = 0; x < 6; ++x) w1c[x] = tile[i][x * 6 + a];
#pragma unroll
            for (int b = 0; b < 6; ++b) {
                double sacc = 0.0;
#pragma unroll
                for (int x = 0; x < 6; ++x) sacc += w1c[x] * Y[x * 6 + b];
                oc[b] = sacc;
            }
#pragma unroll
            for (int b = 0; b < 6; ++b) tile[i][b * 6 + a] = null_pair ? 0.0 : oc[b];
        }
    }
    wave_sync();
    if (i < 36) {                                  // (eight LDS reads in flight, added in pair order)
        const int slot = line_chunk ? (i % 6) * 6 + i / 6 : i;
        double acc = 0.0;
        for (int k0 = 0; k0 < n; k0 += 8) {
            double v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = tile[k0 + u < n ? k0 + u : n - 1][slot];
#pragma unroll
            for (int u = 0; u < 8; ++u) if (k0 + u < n) acc += v[u];
        }
        part[((size_t)B * max_chunks + c) * 36 + i] = acc;
    }
}

// b's share of keyframe k: sum over its observations (the keyframe lists of the assembly: points first, then lines) of W_o^T t_lm
// -- a lane per observation of the chunk, then six lanes add the chunk's terms sequentially in list order
__device__ __forceinline__ void
schur_b_partials_wg(double (*tile)[37], int k, int c, const int32_t* __restrict__ kf_ptr, const int32_t* __restrict__ kf_obs,
                    int32_t n_pt_obs, const int32_t* __restrict__ pt_lm, const int32_t* __restrict__ ls_lm,
                    const double* __restrict__ W_pt, const double* __restrict__ W_ls, const double* __restrict__ tp,
                    const double* __restrict__ tl, int32_t max_chunks, double* __restrict__ part /* [nkf][max_chunks][6] */)
{
    const int i = threadIdx.x & 63;
    const int beg = kf_ptr[k] + c * POSE_CHUNK;
    const int end = beg + POSE_CHUNK < kf_ptr[k + 1] ? beg + POSE_CHUNK : kf_ptr[k + 1];
    const int n = end - beg;
    if (n <= 0) return;
    if (i < n) {
        const int o = kf_obs[beg + i];
        if (o < n_pt_obs) {
            const double* W = W_pt + (size_t)o * 18;
            const double* t = tp + (size_t)pt_lm[o] * 3;
            const double t0 = t[0], t1 = t[1], t2 = t[2];
#pragma unroll
            for (int a = 0; a < 6; ++a) tile[i][a] = W[0 * 6 + a] * t0 + W[1 * 6 + a] * t1 + W[2 * 6 + a] * t2;
        } else {
            const int ol = o - n_pt_obs;
            const double* W = W_ls + (size_t)ol * 36;
            const double* t = tl + (size_t)ls_lm[ol] * 6;
            double tt[6];
#pragma unroll
            for (int x = 0; x < 6; ++x) tt[x] = t[x];
#pragma unroll
            for (int a = 0; a < 6; ++a) {
                double sacc = 0.0;
#pragma unroll
                for (int x = 0; x < 6; ++x) sacc += W[x * 6 + a] * tt[x];
                tile[i][a] = sacc;
            }
        }
    }
    wave_sync();
    if (i < 6) {
        double acc = 0.0;
        for (int q0 = 0; q0 < n; q0 += 8) {
            double v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = tile[q0 + u < n ? q0 + u : n - 1][i];
#pragma unroll
            for (int u = 0; u < 8; ++u) if (q0 + u < n) acc += v[u];
        }
        part[((size_t)k * max_chunks + c) * 6 + i] = acc;
    }
}

// both kinds of chunk partials in ONE launch (they need the landmark inverses and nothing of each other): workgroups
// [0, nblk * schur_chunks) take the (block, chunk) pairs of S, the rest the (keyframe, chunk) pairs of b
struct SchurPartArgs {
    const SchurPair* pairs; const int32_t* blk_ptr; const int32_t* kf_ptr; const int32_t* kf_obs; const int32_t* pt_lm; const int32_t* ls_lm;
    const double *W_pt, *W_ls, *Vp, *Vl, *tp, *tl;
    double *spart, *bpart;
    int32_t nblk, schur_chunks, nkf, pose_chunks, n_pt_obs;
};
static_assert(SCH_CHUNK == POSE_CHUNK, "one workgroup shape for both kinds of chunk");
// (one chunk, one wave and one tile per workgroup: see wave_sync.  The tile is static LDS: 20.8 us against 26.8 with the same tile as
// dynamic LDS -- the register allocator sees what the workgroup's LDS allows and keeps two waves.  The kernels still index the
// tile by the wave's number, which is 0: taking that out changes their code, so it waits for the next change to them.)
constexpr int SCH_WAVES = 1;
constexpr size_t SCH_TILE_DOUBLES = (size_t)SCH_CHUNK * 37;
__device__ __forceinline__ void schur_partials_item(double (*tile)[37], const SchurPartArgs& A, int w, int npart)
{
    const int nS = A.nblk * A.schur_chunks;
    if (w < nS)
        schur_partials_wg(tile, w / A.schur_chunks, w % A.schur_chunks, A.pairs, A.blk_ptr, A.W_pt, A.W_ls, A.Vp, A.Vl, A.schur_chunks, A.spart);
    else if (w < npart)
        schur_b_partials_wg(tile, (w - nS) / A.pose_chunks, (w - nS) % A.pose_chunks, A.kf_ptr, A.kf_obs, A.n_pt_obs, A.pt_lm, A.ls_lm,
                            A.W_pt, A.W_ls, A.tp, A.tl, A.pose_chunks, A.bpart);
}
__global__ void __launch_bounds__(SCH_CHUNK * SCH_WAVES)
k_schur_partials(SchurPartArgs A, int32_t npart)
{
    __shared__ __attribute__((aligned(16))) double sch_lds[SCH_WAVES * SCH_TILE_DOUBLES];
    const int wv = (int)threadIdx.x >> 6;
    schur_partials_item(reinterpret_cast<double (*)[37]>(sch_lds + wv * SCH_TILE_DOUBLES), A, (int)blockIdx.x * SCH_WAVES + wv, npart);
}

__global__ void __launch_bounds__(SCH_CHUNK * SCH_WAVES)
k_schur_partials_lm(SchurPartArgs A, int32_t npart, const LbaLmCtl* __restrict__ ctl)
{
    __shared__ __attribute__((aligned(16))) double sch_lds[SCH_WAVES * SCH_TILE_DOUBLES];
    if (ctl->stop != LM_RUNNING) return;
    const int wv = (int)threadIdx.x >> 6;
    schur_partials_item(reinterpret_cast<double (*)[37]>(sch_lds + wv * SCH_TILE_DOUBLES), A, (int)blockIdx.x * SCH_WAVES + wv, npart);
}

// plslam_lba_plan_iterate_schur: the Schur partials and, in the SAME launch, the iteration's last stage (K10: keyframe blocks and err
// from their partials) -- the two are independent (the partials read W and the landmark inverses, K22 behind them reads H_pose /
// g_pose), so the iteration's third launch rides in the Schur step's second.  The last stage's workgroups come FIRST (a wave each;
// chains of round trips: at the grid's end they would be the launch's tail).
__global__ void __launch_bounds__(SCH_CHUNK * SCH_WAVES)
k_schur_partials_lba_finish(SchurPartArgs A, const LbaBlockArgs B, int32_t npart)
{
    __shared__ __attribute__((aligned(16))) double sch_lds[SCH_WAVES * SCH_TILE_DOUBLES];
    const int wv = (int)threadIdx.x >> 6;
    const int nF = B.nkf + 1;
    if ((int)blockIdx.x < nF) {
        if (wv == 0) lba_finish_wg<SCH_CHUNK>(B, (int)blockIdx.x, sch_lds);
        return;
    }
    schur_partials_item(reinterpret_cast<double (*)[37]>(sch_lds + wv * SCH_TILE_DOUBLES), A, ((int)blockIdx.x - nF) * SCH_WAVES + wv, npart);
}

__global__ void __launch_bounds__(SCH_CHUNK * SCH_WAVES)
k_schur_partials_lba_finish_lm(SchurPartArgs A, const LbaBlockArgs B, int32_t npart, const LbaLmCtl* __restrict__ ctl)
{
    __shared__ __attribute__((aligned(16))) double sch_lds[SCH_WAVES * SCH_TILE_DOUBLES];
    if (ctl->stop != LM_RUNNING) return;
    const int wv = (int)threadIdx.x >> 6;
    const int nF = B.nkf + 1;
    if ((int)blockIdx.x < nF) {
        if (wv == 0) lba_finish_wg<SCH_CHUNK>(B, (int)blockIdx.x, sch_lds);
        return;
    }
    schur_partials_item(reinterpret_cast<double (*)[37]>(sch_lds + wv * SCH_TILE_DOUBLES), A, ((int)blockIdx.x - nF) * SCH_WAVES + wv, npart);
}

// block B = (k1 <= k2) in row-major upper-triangle order; S is (6 nkf) x (6 nkf) row-major, b follows it
__device__ __forceinline__ void
schur_finish_wg(const int32_t* __restrict__ blk_ptr, const int32_t* __restrict__ kf_ptr, const double* __restrict__ spart,
               const double* __restrict__ bpart, const double* __restrict__ H_pose, const double* __restrict__ g_pose,
               int32_t nkf, int32_t nblk, int32_t schur_chunks, int32_t pose_chunks, double lambda, double* __restrict__ S,
               double* __restrict__ bvec, int32_t* __restrict__ next_sing, const double* __restrict__ err_src, double* __restrict__ err_dst,
               const int32_t* __restrict__ sing_cur, int32_t* __restrict__ sing_out)
{
    const int B = blockIdx.x, e = threadIdx.x;
    const int n6 = 6 * nkf;
    if (B == 0 && e == 0) {
        *next_sing = 0;                            // the NEXT call's counter of singular landmarks (this call's: the other word)
        *err_dst = *err_src;                       // the iteration's err beside S and b: plslam_lba_plan_iterate_schur's ONE copy
        if (sing_out) *sing_out = *sing_cur;       // (S, b written in place in the host's image: this call's counter beside them)
    }
    if (B < nblk) {
        if (e >= 36) return;
        int k1 = 0, rem = B;                       // B = offset(k1) + (k2 - k1), offset(k1) = sum_{i < k1} (nkf - i)
        while (rem >= nkf - k1) { rem -= nkf - k1; ++k1; }
        const int k2 = k1 + rem, a = e / 6, b = e % 6;
        const int nch = (blk_ptr[B + 1] - blk_ptr[B] + SCH_CHUNK - 1) / SCH_CHUNK;
        // (the chunk partials are added in chunk order; their loads go out eight at a time -- one by one they are a chain of
        // round trips)
        double acc = 0.0;
        for (int c0 = 0; c0 < nch; c0 += 32) {
            double v[32];
#pragma unroll
            for (int u = 0; u < 32; ++u) v[u] = c0 + u < nch ? spart[((size_t)B * schur_chunks + c0 + u) * 36 + e] : 0.0;
#pragma unroll
            for (int u = 0; u < 32; ++u) if (c0 + u < nch) acc += v[u];
        }
        double h = 0.0;
        if (k1 == k2) {
            h = H_pose[(size_t)k1 * 36 + e];
            if (a == b) h += lambda * h;
        }
        const double v = h - acc;
        S[(size_t)(6 * k1 + a) * n6 + 6 * k2 + b] = v;
        if (k1 != k2) S[(size_t)(6 * k2 + b) * n6 + 6 * k1 + a] = v;
    } else {
        const int k = B - nblk;
        if (e >= 6) return;
        const int nch = (kf_ptr[k + 1] - kf_ptr[k] + POSE_CHUNK - 1) / POSE_CHUNK;
        double acc = 0.0;
        for (int c0 = 0; c0 < nch; c0 += 32) {
            double v[32];
#pragma unroll
            for (int u = 0; u < 32; ++u) v[u] = c0 + u < nch ? bpart[((size_t)k * pose_chunks + c0 + u) * 6 + e] : 0.0;
#pragma unroll
            for (int u = 0; u < 32; ++u) if (c0 + u < nch) acc += v[u];
        }
        bvec[6 * k + e] = g_pose[6 * k + e] - acc;
    }
}
__global__ void __launch_bounds__(64)
k_schur_finish(const int32_t* __restrict__ blk_ptr, const int32_t* __restrict__ kf_ptr, const double* __restrict__ spart,
               const double* __restrict__ bpart, const double* __restrict__ H_pose, const double* __restrict__ g_pose,
               int32_t nkf, int32_t nblk, int32_t schur_chunks, int32_t pose_chunks, double lambda, double* __restrict__ S,
               double* __restrict__ bvec, int32_t* __restrict__ next_sing, const double* __restrict__ err_src, double* __restrict__ err_dst,
               const int32_t* __restrict__ sing_cur, int32_t* __restrict__ sing_out)
{
    schur_finish_wg(blk_ptr, kf_ptr, spart, bpart, H_pose, g_pose, nkf, nblk, schur_chunks, pose_chunks, lambda, S, bvec, next_sing, err_src,
                    err_dst, sing_cur, sing_out);
}
__global__ void __launch_bounds__(64)
k_schur_finish_lm(const int32_t* __restrict__ blk_ptr, const int32_t* __restrict__ kf_ptr, const double* __restrict__ spart,
                  const double* __restrict__ bpart, const double* __restrict__ H_pose, const double* __restrict__ g_pose,
                  int32_t nkf, int32_t nblk, int32_t schur_chunks, int32_t pose_chunks, const LbaLmCtl* __restrict__ ctl,
                  double* __restrict__ S, double* __restrict__ bvec, int32_t* __restrict__ next_sing, const double* __restrict__ err_src,
                  double* __restrict__ err_dst, const int32_t* __restrict__ sing_cur)
{
    if (ctl->stop != LM_RUNNING) return;
    schur_finish_wg(blk_ptr, kf_ptr, spart, bpart, H_pose, g_pose, nkf, nblk, schur_chunks, pose_chunks, ctl->lambda, S, bvec, next_sing,
                    err_src, err_dst, sing_cur, nullptr);
}

// A lane per (landmark, row x of its step): the row's share of sum_o W_o dp[kf(o)] in list order, the DL shares of a landmark
// exchanged through LDS, then row x of Vinv times them.  192 lanes = 64 points or 32 lines per workgroup; points' workgroups
// first, lines' behind them: ONE launch (a lane per landmark was 8 workgroups for C3's 2 000 lines: 15 + 9 us in two launches).
constexpr int BACK_WG = 192;
template <int DL>
__device__ __forceinline__ void
schur_backsub_wg(double* __restrict__ sh, int wg, const int32_t* __restrict__ lm_ptr, const int32_t* __restrict__ lm_obs,
                 const int32_t* __restrict__ kf_loc, int32_t n, const double* __restrict__ W, const double* __restrict__ Vinv,
                 const double* __restrict__ t, const double* __restrict__ dp, double* __restrict__ dx, double* __restrict__ X,
                 double* __restrict__ part)
{
    constexpr int PER_WG = BACK_WG / DL;
    const int q = (int)threadIdx.x / DL, x = (int)threadIdx.x % DL;
    const int j = wg * PER_WG + q;
    double acc = 0.0;
    if (j < n) {
        for (int i = lm_ptr[j]; i < lm_ptr[j + 1]; ++i) {
            const int o = lm_obs[i], k = kf_loc[o];
            if (k < 0) continue;                       // a fixed keyframe: no cross block, no step
            const double* Wo = W + (size_t)o * DL * 6 + x * 6;
            double s = 0.0;
#pragma unroll
            for (int a = 0; a < 6; ++a) s += Wo[a] * dp[6 * k + a];
            acc += s;
        }
    }
    sh[threadIdx.x] = acc;
    __syncthreads();
    double d = 0.0;
    if (j < n) {
        double s = 0.0;
#pragma unroll
        for (int y = 0; y < DL; ++y) s += Vinv[(size_t)j * DL * DL + x * DL + y] * sh[q * DL + y];
        d = t[(size_t)j * DL + x] - s;
        dx[(size_t)j * DL + x] = d;
        if (X) X[(size_t)j * DL + x] += d;             // :1570-1575 "update point / line LMs": X(i) += DX(i)
    }
    // the workgroup's share of sum DX^2 (the loop's ||DX|| test, :1808), summed in a fixed tree: the same bits on every run
    __syncthreads();
    sh[threadIdx.x] = d * d;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w && (int)threadIdx.x + w < BACK_WG) sh[threadIdx.x] += sh[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) *part = sh[0];
}

struct SchurBackArgs {
    const int32_t *pt_ptr, *pt_obs, *pt_kf, *ls_ptr, *ls_obs, *ls_kf;
    const double *W_pt, *W_ls, *Vp, *Vl, *tp, *tl, *dp;
    double *dx_pt, *dx_ls, *X, *L, *part;              // X / L = nullptr: do not apply; part: a sum of squares per workgroup
    int32_t npt, nls, nwg_pt;
};
__device__ __forceinline__ void schur_backsub_item(const SchurBackArgs& A)
{
    __shared__ double sh[BACK_WG];
    if ((int)blockIdx.x < A.nwg_pt)
        schur_backsub_wg<3>(sh, (int)blockIdx.x, A.pt_ptr, A.pt_obs, A.pt_kf, A.npt, A.W_pt, A.Vp, A.tp, A.dp, A.dx_pt, A.X, A.part + blockIdx.x);
    else
        schur_backsub_wg<6>(sh, (int)blockIdx.x - A.nwg_pt, A.ls_ptr, A.ls_obs, A.ls_kf, A.nls, A.W_ls, A.Vl, A.tl, A.dp, A.dx_ls, A.L, A.part + blockIdx.x);
}

__global__ void __launch_bounds__(BACK_WG)
k_schur_backsub(SchurBackArgs A)
{
    schur_backsub_item(A);
}
// the step is taken only when the control block says so: a rejected step leaves Xw / Lw untouched
__global__ void __launch_bounds__(BACK_WG)
k_schur_backsub_lm(SchurBackArgs A, const LbaLmCtl* __restrict__ ctl)
{
    if (ctl->stop != LM_RUNNING) return;
    if (ctl->apply != 1) { A.X = nullptr; A.L = nullptr; }
    schur_backsub_item(A);
}

// max over all diagonal entries of |H(i,i)| (a maximum: exact whatever the order)
__global__ void __launch_bounds__(256)
k_lba_diag_max(const double* __restrict__ H_pose, int32_t nkf, const double* __restrict__ H_pt, int32_t npt,
               const double* __restrict__ H_ls, int32_t nls, double* __restrict__ out)
{
    __shared__ double red[256];
    double m = 0.0;
    const int total = 6 * nkf + 3 * npt + 6 * nls;
    for (int i = threadIdx.x; i < total; i += 256) {
        double v;
        if (i < 6 * nkf) v = H_pose[(size_t)(i / 6) * 36 + (i % 6) * 7];
        else if (i < 6 * nkf + 3 * npt) { const int q = i - 6 * nkf; v = H_pt[(size_t)(q / 3) * 9 + (q % 3) * 4]; }
        else { const int q = i - 6 * nkf - 3 * npt; v = H_ls[(size_t)(q / 6) * 36 + (q % 6) * 7]; }
        v = fabs(v);
        m = v > m ? v : m;
    }
    red[threadIdx.x] = m;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] = red[threadIdx.x] > red[threadIdx.x + s] ? red[threadIdx.x] : red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = red[0];
}


// workgroups of the back-substitution: 64 points or 32 lines each
static size_t backsub_wgs(const plslam_lba_plan* P)
{
    return (size_t)(P->npt + BACK_WG / 3 - 1) / (BACK_WG / 3) + (size_t)(P->nls + BACK_WG / 6 - 1) / (BACK_WG / 6);
}

// The Schur buffer is laid out HERE and nowhere else (base = nullptr: only the size is wanted).
static size_t carve_schur(plslam_lba_plan* P, char* base, size_t npairs)
{
    ArrCarver c{base};
    const size_t n6 = 6 * (size_t)P->nkf, npt = (size_t)P->npt, nls = (size_t)P->nls;
    LbaSchurView& V = P->sc;
    V.pairs = c.take<SchurPair>(npairs * sizeof(SchurPair), 16); V.blk_ptr = c.take<int32_t>(((size_t)P->nblk + 1) * 4);
    V.Vp = c.take<double>(npt * 72, 8); V.Vl = c.take<double>(nls * 288, 8);
    V.tp = c.take<double>(npt * 24, 8); V.tl = c.take<double>(nls * 48, 8);
    V.spart = c.take<double>((size_t)P->nblk * (size_t)P->schur_chunks * 36 * 8, 8);
    V.bpart = c.take<double>((size_t)P->nkf * (size_t)P->max_chunks * 6 * 8, 8);
    V.tail = SchurTail(c.take<double>(SchurTail::bytes(n6), 16), n6);
    V.dp = c.take<double>(n6 * 8, 8);
    V.dx = c.take<double>((3 * npt + 6 * nls) * 8, 8);
    // (then a partial sum of squares per workgroup of the back-substitution, and their sum)
    V.dx_part = c.take<double>((backsub_wgs(P) + 2) * 8);
    c.take<char>(8);                               // (a word nothing uses: the buffer keeps its size)
    return c.size();
}

int lba_schur_reserve(plslam_lba_plan* P, size_t npairs)
{
    const size_t n6 = 6 * (size_t)P->nkf;
    int rc;
    if ((rc = P->schur.reserve(carve_schur(P, nullptr, npairs) + 256)) ||
        (rc = P->schur_pin.reserve(std::max(SchurTail::bytes(n6), (3 * (size_t)P->npt + 6 * (size_t)P->nls) * 8) + n6 * 8 +
                                   ((size_t)P->npt / (BACK_WG / 3) + (size_t)P->nls / (BACK_WG / 6) + 2) * 8 + 256)))
        return rc;
    carve_schur(P, P->schur.as<char>(), npairs);
    P->simg = SchurImage(P->schur_pin.as<double>(), n6);
    P->schur_mapped = P->schur_pin.dev != nullptr;
    if (P->schur_mapped) P->simg_dev = SchurImage(static_cast<double*>(P->schur_pin.dev), n6);
    PLSLAM_HIP_CHECK(hipMemsetAsync(P->sc.tail.sing, 0, 8, P->ctx->stream));      // both counters of singular landmarks
    P->schur_parity = 0;
    return PLSLAM_OK;
}

int lba_schur_prepare(plslam_lba_plan* P)
{
    if (P->schur_ready) return PLSLAM_OK;
    // (the partials address the cross blocks and the landmark inverses by 32-bit byte offsets: 288 bytes per line row)
    PLSLAM_REQUIRE((size_t)P->np * 144 < (size_t(1) << 32) && (size_t)P->nl * 288 < (size_t(1) << 32) &&
                   (size_t)P->npt * 72 < (size_t(1) << 32) && (size_t)P->nls * 288 < (size_t(1) << 32), PLSLAM_EINVAL);
    if (P->dev_lists) return lba_schur_prepare_dev(P);      // (the lists are on the device already, and no host copy exists)
    const SchurLists L = build_schur_pairs(P->csr, P->h_pt_kf, P->h_ls_kf, P->nkf);
    P->nblk = (int32_t)L.cnt.size() - 1;
    P->schur_chunks = L.schur_chunks;
    int rc = lba_schur_reserve(P, L.pairs.size());
    if (rc) return rc;
    hipStream_t s = P->ctx->stream;
    const LbaSchurView& V = P->sc;
    if (V.pairs.bytes) PLSLAM_HIP_CHECK(hipMemcpyAsync(V.pairs, L.pairs.data(), V.pairs.bytes, hipMemcpyHostToDevice, s));
    PLSLAM_HIP_CHECK(hipMemcpyAsync(V.blk_ptr, L.cnt.data(), V.blk_ptr.bytes, hipMemcpyHostToDevice, s));
    PLSLAM_HIP_CHECK(hipStreamSynchronize(s));          // (the staging vectors die here)
    P->schur_ready = true;
    return PLSLAM_OK;
}

}  // namespace plslam

extern "C" int plslam_lba_plan_diag_max(plslam_lba_plan* P, double* hmax)
{
    PLSLAM_REQUIRE(P && hmax, PLSLAM_EINVAL);
    plslam_ctx* ctx = P->ctx;
    std::lock_guard<std::mutex> lk(ctx->mu);               // (the plan's state flags are read under the lock: ADVICE r5)
    DeviceGuard dg_(ctx->device);
    PLSLAM_REQUIRE(P->blocks_valid, PLSLAM_EINVAL);        // one plslam_lba_plan_iterate* first
    int rc = lba_schur_prepare(P);
    if (rc) return rc;
    hipStream_t s = ctx->stream;
    const LbaOutView& O = P->o;
    hipLaunchKernelGGL(k_lba_diag_max, dim3(1), dim3(256), 0, s, O.H_pose, P->nkf, O.H_pt, P->npt, O.H_ls, P->nls, P->sc.tail.hmax);
    PLSLAM_HIP_CHECK(hipGetLastError());
    PLSLAM_HIP_CHECK(hipMemcpyAsync(P->simg.tail.hmax, P->sc.tail.hmax, 8, hipMemcpyDeviceToHost, s));
    PLSLAM_HIP_CHECK(hipStreamSynchronize(s));
    *hmax = *P->simg.tail.hmax;
    return PLSLAM_OK;
}

// the Schur step's three launches on the blocks of the last iteration (no copy, no synchronisation); *par = the counter word of
// singular landmarks this call counts in
namespace plslam {
int lba_schur_enqueue(plslam_lba_plan* P, double lambda, int* par_out, bool fused, const LbaLmCtl* ctl)
{
    int rc = lba_schur_prepare(P);
    if (rc) return rc;
    hipStream_t s = P->ctx->stream;
    const LbaStatView& S = P->st; const LbaOutView& O = P->o; const LbaSchurView& C = P->sc;
    const size_t n6 = 6 * (size_t)P->nkf;
    // two counters of singular landmarks behind S, b and the diagonal maximum (ONE copy brings S, b and them back): a call counts
    // in one of them and its last kernel clears the other for the next call (both cleared at plan creation) -- no memset launch
    int32_t* sing2 = C.tail.sing;
    const int par = P->schur_parity;
    const int32_t nb3 = (P->npt + 255) / 256, nb6 = (P->nls + 255) / 256;
    if (nb3 + nb6 > 0 && !fused && ctl)
        hipLaunchKernelGGL(k_schur_landmarks_lm, dim3(nb3 + nb6), dim3(256), 0, s, O.H_pt, O.g + n6, P->npt, O.H_ls,
                           O.g + n6 + 3 * (size_t)P->npt, P->nls, nb3, ctl, C.Vp, C.tp, C.Vl, C.tl, sing2 + par);
    else if (nb3 + nb6 > 0 && !fused)                     // (fused: the iteration's blocks launch has written them)
        hipLaunchKernelGGL(k_schur_landmarks, dim3(nb3 + nb6), dim3(256), 0, s, O.H_pt, O.g + n6, P->npt, O.H_ls,
                           O.g + n6 + 3 * (size_t)P->npt, P->nls, nb3, lambda, C.Vp, C.tp, C.Vl, C.tl, sing2 + par);
    SchurPartArgs A{};
    A.pairs = C.pairs; A.blk_ptr = C.blk_ptr; A.kf_ptr = S.kf_ptr; A.kf_obs = S.kf_ids; A.pt_lm = S.pt_lm; A.ls_lm = S.ls_lm;
    A.W_pt = O.W_pt; A.W_ls = O.W_ls; A.Vp = C.Vp; A.Vl = C.Vl; A.tp = C.tp; A.tl = C.tl;
    A.spart = C.spart; A.bpart = C.bpart;
    A.nblk = P->nblk; A.schur_chunks = P->schur_chunks; A.nkf = P->nkf; A.pose_chunks = P->max_chunks; A.n_pt_obs = P->np;
    const int32_t npart_wgs = P->nblk * P->schur_chunks + P->nkf * P->max_chunks;
    if (fused && ctl)
        hipLaunchKernelGGL(k_schur_partials_lba_finish_lm, dim3(npart_wgs + P->nkf + 1), dim3(SCH_CHUNK), 0, s, A, lba_block_args(P), npart_wgs, ctl);
    else if (fused)
        hipLaunchKernelGGL(k_schur_partials_lba_finish, dim3(npart_wgs + P->nkf + 1), dim3(SCH_CHUNK), 0, s, A, lba_block_args(P), npart_wgs);
    else if (npart_wgs > 0 && ctl)
        hipLaunchKernelGGL(k_schur_partials_lm, dim3(npart_wgs), dim3(SCH_CHUNK), 0, s, A, npart_wgs, ctl);
    else if (npart_wgs > 0)
        hipLaunchKernelGGL(k_schur_partials, dim3(npart_wgs), dim3(SCH_CHUNK), 0, s, A, npart_wgs);
    // S, b, err and this call's counter: written where the host reads them (the page-locked image, mapped) when it can be -- no
    // copy behind the kernel; otherwise beside the partials on the device, and lba_schur_fetch copies
    const SchurTail& to = P->schur_mapped && !ctl ? P->simg_dev.tail : C.tail;
    if (ctl)
        hipLaunchKernelGGL(k_schur_finish_lm, dim3(P->nblk + P->nkf), dim3(64), 0, s, C.blk_ptr, S.kf_ptr, C.spart, C.bpart, O.H_pose, O.g,
                           P->nkf, P->nblk, P->schur_chunks, P->max_chunks, ctl, to.S, to.b, sing2 + (par ^ 1), O.err, to.err, sing2 + par);
    else
    hipLaunchKernelGGL(k_schur_finish, dim3(P->nblk + P->nkf), dim3(64), 0, s, C.blk_ptr, S.kf_ptr, C.spart, C.bpart, O.H_pose, O.g, P->nkf,
                       P->nblk, P->schur_chunks, P->max_chunks, lambda, to.S, to.b, sing2 + (par ^ 1), O.err, to.err, sing2 + par,
                       P->schur_mapped ? to.sing + par : nullptr);
    PLSLAM_HIP_CHECK(hipGetLastError());
    P->schur_parity = par ^ 1;        // (only now: the kernel that clears the other counter is in the stream)
    *par_out = par;
    return PLSLAM_OK;
}
}  // namespace plslam

// S, b and the counter behind them: one copy, one synchronisation
static int lba_schur_fetch(plslam_lba_plan* P, int par, double* S, double* b, int32_t* n_singular, double* err = nullptr)
{
    hipStream_t s = P->ctx->stream;
    const size_t n6 = 6 * (size_t)P->nkf;
    const SchurTail& h = P->simg.tail;
    if (!P->schur_mapped) PLSLAM_HIP_CHECK(hipMemcpyAsync(h.S, P->sc.tail.S, SchurTail::bytes(n6), hipMemcpyDeviceToHost, s));
    PLSLAM_HIP_CHECK(hipStreamSynchronize(s));
    memcpy(S, h.S, n6 * n6 * 8);
    memcpy(b, h.b, n6 * 8);
    if (n_singular) *n_singular = h.sing[par];
    if (err) *err = *h.err;
    P->schur_done = true;
    return PLSLAM_OK;
}

extern "C" int plslam_lba_plan_schur(plslam_lba_plan* P, double lambda, double* S, double* b, int32_t* n_singular)
{
    PLSLAM_REQUIRE(P && S && b && lambda >= 0.0, PLSLAM_EINVAL);
    plslam_ctx* ctx = P->ctx;
    std::lock_guard<std::mutex> lk(ctx->mu);
    DeviceGuard dg_(ctx->device);
    PLSLAM_REQUIRE(P->blocks_valid && P->nkf > 0, PLSLAM_EINVAL);
    // the cross blocks must be the local BA's (landmark rows x pose columns): an iteration run with PLSLAM_LBA_COMPAT_GBA wrote the
    // pose x line blocks transposed, as the reference's GBA does (:2341-2352) -- a defect this step does not reproduce
    PLSLAM_REQUIRE(!P->blocks_gba, PLSLAM_EINVAL);
    int par = 0;
    int rc = lba_schur_enqueue(P, lambda, &par);
    if (rc) { (void)hipStreamSynchronize(ctx->stream); return rc; }
    return lba_schur_fetch(P, par, S, b, n_singular);
}

// One LM iteration's device half in ONE call and ONE synchronisation (round 6): H, g, err on the RESIDENT state
// (plslam_lba_plan_iterate_resident) and, straight behind it, the Schur step for `lambda` (plslam_lba_plan_schur) -- the
// reference's :1587-1783 for a lambda the caller already knows (every iteration but the first, whose lambda needs Hmax).
extern "C" int plslam_lba_plan_iterate_schur(plslam_lba_plan* P, int compat_flags, double lambda, double* err, double* S, double* b,
                                             int32_t* n_singular)
{
    PLSLAM_REQUIRE(P && err && S && b && lambda >= 0.0, PLSLAM_EINVAL);
    PLSLAM_REQUIRE(!(compat_flags & PLSLAM_LBA_COMPAT_GBA), PLSLAM_EINVAL);
    plslam_ctx* ctx = P->ctx;
    std::lock_guard<std::mutex> lk(ctx->mu);
    DeviceGuard dg_(ctx->device);
    PLSLAM_REQUIRE(P->state_valid && P->nkf > 0, PLSLAM_EINVAL);
    hipStream_t s = ctx->stream;
    // four launches for the iteration and its Schur step: rows + cross blocks | landmark blocks AND their damped inverses, keyframe
    // chunk partials | Schur partials AND the keyframe blocks + err | S, b (+ err beside them); the separate calls make seven
    int rc = lba_schur_prepare(P);
    if (!rc) rc = lba_plan_enqueue(P, nullptr, nullptr, nullptr, compat_flags, false, lambda);
    int par = 0;
    if (!rc) rc = lba_schur_enqueue(P, lambda, &par, true);
    if (rc) { (void)hipStreamSynchronize(s); return rc; }
    return lba_schur_fetch(P, par, S, b, n_singular, err);    // (err rides behind S and b: k_schur_finish put it there)
}

// the back-substitution's arguments from the plan's views
static SchurBackArgs backsub_args(plslam_lba_plan* P, int apply, double* part_out)
{
    const LbaStatView& S = P->st; const LbaOutView& O = P->o; const LbaSchurView& C = P->sc;
    SchurBackArgs A{};
    A.pt_ptr = S.pt_ptr; A.pt_obs = S.pt_ids; A.pt_kf = S.pt_kf; A.ls_ptr = S.ls_ptr; A.ls_obs = S.ls_ids; A.ls_kf = S.ls_kf;
    A.W_pt = O.W_pt; A.W_ls = O.W_ls; A.Vp = C.Vp; A.Vl = C.Vl; A.tp = C.tp; A.tl = C.tl;
    A.dp = C.dp; A.dx_pt = C.dx; A.dx_ls = C.dx + 3 * (size_t)P->npt; A.part = part_out ? part_out : C.dx_part.p;
    A.X = apply ? P->x.Xw.p : nullptr; A.L = apply ? P->x.Lw.p : nullptr;
    A.npt = P->npt; A.nls = P->nls; A.nwg_pt = (P->npt + BACK_WG / 3 - 1) / (BACK_WG / 3);
    return A;
}

namespace plslam {
int lba_backsub_enqueue_lm(plslam_lba_plan* P, const LbaLmCtl* ctl)
{
    const SchurBackArgs A = backsub_args(P, 1, nullptr);
    const int32_t nwg = (int32_t)backsub_wgs(P);
    if (nwg > 0) hipLaunchKernelGGL(k_schur_backsub_lm, dim3(nwg), dim3(BACK_WG), 0, P->ctx->stream, A, ctl);
    PLSLAM_HIP_CHECK(hipGetLastError());
    return PLSLAM_OK;
}
int lba_backsub_wgs(const plslam_lba_plan* P) { return (int)backsub_wgs(P); }
}  // namespace plslam

// dp up, the back-substitution (and the landmark update when `apply`) into the stream; no synchronisation
static int lba_backsub_enqueue(plslam_lba_plan* P, const double* dpose, int apply, double* part_out = nullptr)
{
    hipStream_t s = P->ctx->stream;
    const LbaSchurView& C = P->sc;
    memcpy(P->simg.dp, dpose, C.dp.bytes);
    PLSLAM_HIP_CHECK(hipMemcpyAsync(C.dp, P->simg.dp, C.dp.bytes, hipMemcpyHostToDevice, s));
    const SchurBackArgs A = backsub_args(P, apply, part_out);
    const int32_t nwg = (int32_t)backsub_wgs(P);
    if (nwg > 0) hipLaunchKernelGGL(k_schur_backsub, dim3(nwg), dim3(BACK_WG), 0, s, A);
    PLSLAM_HIP_CHECK(hipGetLastError());
    if (apply) P->schur_done = false;                      // (a second application of the same step would be a bug of the caller)
    return PLSLAM_OK;
}

extern "C" int plslam_lba_plan_backsub(plslam_lba_plan* P, const double* dpose, int apply, double* dX_pt, double* dX_ls)
{
    PLSLAM_REQUIRE(P && dpose, PLSLAM_EINVAL);
    plslam_ctx* ctx = P->ctx;
    std::lock_guard<std::mutex> lk(ctx->mu);
    DeviceGuard dg_(ctx->device);
    PLSLAM_REQUIRE(P->schur_done, PLSLAM_EINVAL);          // plslam_lba_plan_schur on the blocks of the last iteration first
    PLSLAM_REQUIRE(!apply || P->state_valid, PLSLAM_EINVAL);
    hipStream_t s = ctx->stream;
    int rc = lba_backsub_enqueue(P, dpose, apply);
    if (rc) { (void)hipStreamSynchronize(s); return rc; }
    if (dX_pt || dX_ls) {
        const Arr<double>& dx = P->sc.dx;
        const double* hdx = P->simg.dx;
        if (dx.bytes) PLSLAM_HIP_CHECK(hipMemcpyAsync(P->simg.dx, dx, dx.bytes, hipMemcpyDeviceToHost, s));
        PLSLAM_HIP_CHECK(hipStreamSynchronize(s));
        if (dX_pt && P->npt) memcpy(dX_pt, hdx, (size_t)P->npt * 24);
        if (dX_ls && P->nls) memcpy(dX_ls, hdx + 3 * (size_t)P->npt, (size_t)P->nls * 48);
    } else {
        PLSLAM_HIP_CHECK(hipStreamSynchronize(s));         // (the page-locked image of dp is the caller's to rewrite next)
    }
    return PLSLAM_OK;
}

// The rest of an LM iteration in ONE call and ONE synchronisation (round 6): the back-substitution of `dpose` (and X(i) += DX(i)
// when `apply`, :1570-1575 / :1801-1806), the pose slots for the next iteration (T_kf_w: n_slots x 16 or NULL to leave them --
// a rejected step), and sum_i DX_landmark(i)^2 for the loop's ||DX|| test (:1808) -- 8 bytes come back instead of the steps.
extern "C" int plslam_lba_plan_apply_step(plslam_lba_plan* P, const double* dpose, const double* T_kf_w, int apply, double* dx_sumsq)
{
    PLSLAM_REQUIRE(P && dpose, PLSLAM_EINVAL);
    plslam_ctx* ctx = P->ctx;
    std::lock_guard<std::mutex> lk(ctx->mu);
    DeviceGuard dg_(ctx->device);
    PLSLAM_REQUIRE(P->schur_done, PLSLAM_EINVAL);
    PLSLAM_REQUIRE(P->state_valid || (!apply && !T_kf_w), PLSLAM_EINVAL);
    hipStream_t s = ctx->stream;
    // (the per-workgroup sums of squares: written in place behind dp's image when the image is mapped)
    const bool in_place = dx_sumsq && P->schur_mapped;
    int rc = lba_backsub_enqueue(P, dpose, apply, in_place ? P->simg_dev.dx_part : nullptr);
    if (rc) { (void)hipStreamSynchronize(s); return rc; }
    if (T_kf_w && P->n_slots) {
        memcpy(P->hx.T, T_kf_w, P->hx.T.bytes);
        PLSLAM_HIP_CHECK(hipMemcpyAsync(P->x.T, P->hx.T, P->x.T.bytes, hipMemcpyHostToDevice, s));
    }
    // the back-substitution left one sum of squares per workgroup (220 at C3): they come down and are added here in workgroup
    // order -- a fixed order, and no launch for it
    const size_t nwg = backsub_wgs(P);
    if (dx_sumsq && nwg && !in_place)
        PLSLAM_HIP_CHECK(hipMemcpyAsync(P->simg.dx_part, P->sc.dx_part, nwg * 8, hipMemcpyDeviceToHost, s));
    PLSLAM_HIP_CHECK(hipStreamSynchronize(s));
    if (dx_sumsq) {
        const double* part = P->simg.dx_part;
        double acc = 0.0;
        for (size_t i = 0; i < nwg; ++i) acc += part[i];
        *dx_sumsq = acc;
    }
    return PLSLAM_OK;
}
