// env_ldlt.hpp -- the envelope L D L^T of the loop-closure pose graph (env_ldlt.hip, K45-K46) as pgo.hip uses it.  Internal.
#pragma once

#include "common.hpp"

namespace plslam {

// the envelope on the device (pgo_graph.hpp: Envelope): row r holds columns cs[r] .. r at off[r]; reach[k] = the last row whose
// envelope reaches column k; bw = the widest row
struct EnvDev { const int64_t* off; const int32_t* cs; const int32_t* reach; int32_t N, bw; };

// one damped envelope solve: L D L^T of H + lambda I and x with it; nbad: the count of zero / non-finite pivots.  Lo: as many
// doubles as H; z, zg, x: N doubles each
int env_solve_enqueue(const EnvDev& E, const double* H, double lambda, const double* b, double* Lo, double* z, double* zg,
                      double* x, int32_t* nbad, hipStream_t s);
// the dense comparison path: the envelope into a zero-padded npad x npad S (+ lambda, unit padding), b into w
void env_to_dense_enqueue(const EnvDev& E, const double* H, int64_t npad, double lambda, const double* b, double* S, double* w,
                          hipStream_t s);

}  // namespace plslam
