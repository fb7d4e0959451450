// ldlt_dense.hpp -- the dense right-looking fp64 L D L^T of the global bundle adjustment (ldlt_dense.hip, K32-K36) as gba.hip
// and, for the comparison path of the loop-closure pose graph, pgo.hip use it.  Internal.
#pragma once

#include "common.hpp"

namespace plslam {

constexpr int LT = 32;          // LDL^T tile edge
inline int64_t pad_to_tile(int64_t n) { return (n + LT - 1) / LT * LT; }   // the npad of ldlt_enqueue

// The matrix S (npad x npad, row-major, lower triangle read) is factored in place and S x = b solved; w, z: npad doubles of
// workspace (w holds b on entry and is overwritten); P: npad x 32 doubles; n <= npad: the order of the system itself, whose bad
// pivots badp counts per tile (npad / LT int32)
int ldlt_enqueue(double* S, int64_t npad, int32_t n, double* P, double* w, double* z, double* x, int32_t* badp, hipStream_t s);
// the padding of S beyond n: identity, so that every tile is full (nothing is launched when npad == n)
void ldlt_pad_diag_enqueue(double* S, int64_t npad, int32_t n, hipStream_t s);
// *nbad = the sum of the nt per-tile counts
void ldlt_count_bad_enqueue(const int32_t* badp, int32_t nt, int32_t* nbad, hipStream_t s);

}  // namespace plslam
