// pose_step_dev.hpp -- the pose update both bundle adjustments run per optimised keyframe (src/mapHandler.cpp:1560-1566 /
// :1793-1799 in the local one, :2371-2377 / :2650-2655 in the global one), one copy: K38 (gba.hip) and the local BA's solve
// kernels (lba_lm_dev.hip) call it.  stvo-pl's maps: se3_dev.hpp.
#pragma once

#include "se3_dev.hpp"

namespace plslam {

// x <- logmap(expmap(x) * inverse(expmap(d))); Tp <- expmap(x), what the keyframe's estimate slot holds from then on
__device__ __forceinline__ void pose_step_se3(const double (&d)[6], double (&x)[6], double (&Tp)[16])
{
    double E[16], Ei[16], Tc[16];
    expmap_se3(x, Tp);
    expmap_se3(d, E);
    inverse_se3(E, Ei);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int c = 0; c < 4; ++c)
            Tc[4 * i + c] = Tp[4 * i] * Ei[c] + Tp[4 * i + 1] * Ei[4 + c] + Tp[4 * i + 2] * Ei[8 + c] + Tp[4 * i + 3] * Ei[12 + c];
    logmap_se3(Tc, x);
    expmap_se3(x, Tp);
}

}  // namespace plslam
