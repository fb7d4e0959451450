// lba_blocks_dev.hpp -- what the fused iteration kernels of the LBA plan (lba_plan.hip) and the Schur step's kernels (lba_schur.hip)
// share: the block kernels' arguments, the iteration's last stage as a workgroup's work (it rides in the Schur partials' launch
// of plslam_lba_plan_iterate_schur) and a landmark's damped inverse (the blocks' launch computes it from its registers there).
// POSE_CHUNK, SCH_CHUNK and SchurPair come from lba_lists.hpp, where the host builds the lists the chunks run over.
#pragma once

#include "lba_lists.hpp"
#include "lba_rows_dev.hpp"

namespace plslam {

struct LbaBlockArgs {
    const int32_t *pt_ptr, *pt_ids, *ls_ptr, *ls_ids, *kf_ptr, *kf_ids;
    const double *pJp, *pJl, *pr, *pw, *lJp, *lJl, *lr, *lw;
    double *H_pt, *g_pt, *H_ls, *g_ls, *pose_part, *H_pose, *g_pose, *err;
    const double* err_part;
    int32_t npt, nls, nkf, np, nb3, nb6, max_chunks, nerr;
    // the Schur step's landmark inverses in the same launch (Vp = nullptr: not asked for)
    double lambda = 0.0;
    double *Vp = nullptr, *tp = nullptr, *Vl = nullptr, *tl = nullptr;
    int32_t* nsing = nullptr;
};

// NT = 256: a lane per partial-sum slot; NT = 64 (inside the Schur partials' launch): a lane plays the four lanes e, e + 64,
// e + 128, e + 192 of the 256-lane form and adds them as its tree's first two levels do -- the same sums in the same order
template <int NT>
__device__ __forceinline__ void lba_finish_wg(const LbaBlockArgs& A, int k, double* __restrict__ red /* [NT] */)
{
    static_assert(NT == 256 || NT == 64, "256 lanes, or 64 lanes playing four each");
    const int e = threadIdx.x;
    if (k < A.nkf) {
        if (e >= 42) return;
        const int nchunks = (A.kf_ptr[k + 1] - A.kf_ptr[k] + POSE_CHUNK - 1) / POSE_CHUNK;
        double acc = 0.0;
        constexpr int PB = 32;                     // (loads in flight per round trip: C3's 105 chunks were 14 round trips at 8)
        for (int c0 = 0; c0 < nchunks; c0 += PB) {
            double v[PB];
#pragma unroll
            for (int j = 0; j < PB; ++j) v[j] = A.pose_part[((size_t)k * A.max_chunks + (c0 + j < nchunks ? c0 + j : nchunks - 1)) * 42 + e];
#pragma unroll
            for (int j = 0; j < PB; ++j)
                if (c0 + j < nchunks) acc += v[j];
        }
        if (e < 36) A.H_pose[(size_t)k * 36 + e] = acc;
        else A.g_pose[(size_t)k * 6 + (e - 36)] = acc;
        return;
    }
    // err: lane e sums the row workgroups' partials e, e + 256, ... in that order, then a tree over the lanes
    constexpr int Q = 256 / NT;
    double acc[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        acc[q] = 0.0;
        for (int i = e + q * NT; i < A.nerr; i += 256) acc[q] += A.err_part[i];
    }
    if constexpr (Q == 4) { acc[0] += acc[2]; acc[1] += acc[3]; acc[0] += acc[1]; }      // the tree's levels 128 and 64
    auto sync = [] { __syncthreads(); };
    red[e] = acc[0];
    sync();
    for (int s = NT / 2; s > 0; s >>= 1) {
        if (e < s) red[e] += red[e + s];
        sync();
    }
    if (e == 0) A.err[0] = red[0];
}

// a landmark's damped block inverted and t = Vinv g (K19 / K20's work): H, g indexed by j; Vinv, t written at j
template <int DL>
__device__ __forceinline__ void schur_landmark(const double* __restrict__ H, const double* __restrict__ g, int j, double lambda,
                                               double* __restrict__ Vinv, double* __restrict__ t, int32_t* __restrict__ nsing)
{
    double A[DL][DL], I[DL][DL];
#pragma unroll
    for (int a = 0; a < DL; ++a)
#pragma unroll
        for (int b = 0; b < DL; ++b) {
            const double h = H[(size_t)j * DL * DL + a * DL + b];
            A[a][b] = a == b ? h + lambda * h : h;
            I[a][b] = a == b ? 1.0 : 0.0;
        }
    // Gauss-Jordan without pivoting (the damped block is symmetric positive definite whenever its diagonal is positive);
    // a pivot that is not positive marks the landmark as singular: no step, no contribution (Vinv = 0, t = 0)
    bool ok = true;
#pragma unroll
    for (int c = 0; c < DL; ++c) {
        const double piv = A[c][c];
        ok = ok && piv > 0.0;
        const double ip = 1.0 / (piv > 0.0 ? piv : 1.0);
#pragma unroll
        for (int b = 0; b < DL; ++b) { A[c][b] *= ip; I[c][b] *= ip; }
#pragma unroll
        for (int a = 0; a < DL; ++a) {
            if (a == c) continue;
            const double f = A[a][c];
#pragma unroll
            for (int b = 0; b < DL; ++b) { A[a][b] -= f * A[c][b]; I[a][b] -= f * I[c][b]; }
        }
    }
    double gj[DL];
#pragma unroll
    for (int a = 0; a < DL; ++a) gj[a] = g[(size_t)j * DL + a];
#pragma unroll
    for (int a = 0; a < DL; ++a) {
        double acc = 0.0;
#pragma unroll
        for (int b = 0; b < DL; ++b) {
            const double v = ok ? I[a][b] : 0.0;
            Vinv[(size_t)j * DL * DL + a * DL + b] = v;
            acc += v * gj[b];
        }
        t[(size_t)j * DL + a] = acc;
    }
    if (!ok && nsing) atomicAdd(nsing, 1);     // (a count only: no sum depends on it)
}

}  // namespace plslam
