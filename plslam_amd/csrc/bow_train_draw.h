// bow_train_draw.h -- the random draws of the vocabulary training (bow_train.hip, K111-K130), stated ONCE for the host planner
// (bow_train_plan.hpp) and the kernels.  tests/bow_train_ref.py states the same function independently (CounterDraws).
//
// The reference draws from one rand() stream in depth-first order; a build that clusters a whole level at once cannot follow
// that stream, so every draw is a function of (seed, node path, centre index j, retry t):
//   key(root) = mix(seed),  key(child c of a node) = mix(key(node) + c + 1),  mix = the splitmix64 finaliser
//   r(key, j, t) = mix(key + 0x9E3779B97F4A7C15 * ((j << 32) + t + 1)) >> 33          a 31-bit integer in place of rand()
// and the arithmetic on r is the reference's (DUtils::Random::RandomInt, Random.cpp:49; RandomValue<double>, Random.h:57):
//   first centre  int((r / 2147483648.0) * n)                               j = 0, t = 0
//   cut           (r / 2147483647.0) * dist_sum, again with t + 1 while it is 0.0   j = the centre being chosen, 1 .. k-1
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define BT_HD __host__ __device__ inline
#else
#define BT_HD inline
#endif

namespace plslam {

BT_HD uint64_t bt_mix64(uint64_t z)
{
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
BT_HD uint64_t bt_root_key(uint64_t seed) { return bt_mix64(seed); }
BT_HD uint64_t bt_child_key(uint64_t key, int32_t c) { return bt_mix64(key + (uint64_t)c + 1ull); }
BT_HD uint32_t bt_draw(uint64_t key, uint32_t j, uint32_t t)
{
    return (uint32_t)(bt_mix64(key + 0x9E3779B97F4A7C15ull * (((uint64_t)j << 32) + (uint64_t)t + 1ull)) >> 33);
}
BT_HD int32_t bt_first_index(uint64_t key, int32_t n) { return (int32_t)(((double)bt_draw(key, 0, 0) / 2147483648.0) * (double)n); }
BT_HD double bt_cut_of(uint32_t r, double dist_sum) { return ((double)r / 2147483647.0) * dist_sum; }
// dist_sum > 0: the cut is 0.0 only for r == 0, so the loop ends (a run of 2^32 zero draws does not exist in a bijection's image)
BT_HD double bt_cut(uint64_t key, uint32_t j, double dist_sum)
{
    double c;
    uint32_t t = 0;
    do c = bt_cut_of(bt_draw(key, j, t++), dist_sum);
    while (c == 0.0);
    return c;
}

}  // namespace plslam
