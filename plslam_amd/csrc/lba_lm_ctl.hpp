// lba_lm_ctl.hpp -- the control flow of levMarquardtOptimizationLBA's loop (src/mapHandler.cpp:1334-1812) as a pure function of
// its state: what plslam_lba_plan_optimize_dev's control kernels (lba_lm_dev.hip, K98-K104) run on one lane, and what
// tests/cpp/test_lba_lm_ctl.cpp replays on the CPU against the reference's recorded runs.  No HIP in here.
//
// One H / g build ("pass") calls, in this order:
//   lm_on_hmax    the first pass only: lambda0 = lambdaLbaLM * max |H(i,i)| (:1544-1550; Hmax is a double here)
//   lm_on_err     err as the text normalises it -- the first pass by the two counters it never increments (:1541: +inf, or NaN for
//                 a zero sum), every later pass by Npt + Nls (:1773) -- and the first stop test (:1775); says whether the solve runs
//                 and whether its step is to be applied (:1786: rejected when err > err_prev; the first one always applied)
//   lm_on_pivots  a pivot of the reduced system that is <= 0 or not finite: the loop ends, the step is NOT applied
//   lm_on_step    the lambda schedule (:1786-1806: lambda GROWS on an applied step), the ||DX|| test over all N unknowns, for a
//                 rejected step too (:1808), err_prev = err after a rejected step too (:1811), ++iters, the loop's bound
#pragma once

#include <stdint.h>

#include "plslam_hip.h"

#if defined(__HIPCC__)
#define PLSLAM_LM_HD __host__ __device__
#else
#define PLSLAM_LM_HD
#endif

namespace plslam {

constexpr int32_t LM_RUNNING = -1;       // the stop word while the loop runs; PLSLAM_LBA_STOP_* once it has ended

struct LbaLmPrm {
    double lambda_lm, lambda_k, min_error_change, min_error;
    double n_lm;                         // Npt + Nls: LANDMARKS, not observations (:1773)
    int32_t max_iters, reserved;
};

struct LbaLmCtl {
    double lambda, err, err_prev, err_raw, hmax;
    double dp_sumsq;                     // the pose part of ||DX||^2 of the current solve (the landmarks' part: lm_on_step's argument)
    int32_t iters, n_builds;
    int32_t stop;                        // LM_RUNNING, or why the loop ended
    int32_t apply;                       // the current build's solve: 1 applied, 0 rejected, -1 the loop ended before it
    int32_t n_singular, n_bad_pivots;    // running counts over the solves
};

PLSLAM_LM_HD inline void lm_init(LbaLmCtl& c)
{
    c.lambda = c.err = c.err_prev = c.err_raw = c.hmax = c.dp_sumsq = 0.0;
    c.iters = c.n_builds = 0;
    c.stop = LM_RUNNING;
    c.apply = -1;
    c.n_singular = c.n_bad_pivots = 0;
}

PLSLAM_LM_HD inline void lm_on_hmax(LbaLmCtl& c, const LbaLmPrm& p, double hmax)
{
    c.hmax = hmax;
    c.lambda = p.lambda_lm * hmax;
}

// -> true: the build's solve runs (c.apply says whether its step is taken)
PLSLAM_LM_HD inline bool lm_on_err(LbaLmCtl& c, const LbaLmPrm& p, double err_raw)
{
    const bool first = c.n_builds == 0;
    const double n_obs_counted = 0.0;    // Npt_obs + Nls_obs as the text leaves them
    c.err_raw = err_raw;
    c.err = err_raw / (first ? n_obs_counted : p.n_lm);
    ++c.n_builds;
    c.dp_sumsq = 0.0;
    if (first) {
        c.apply = 1;
        return true;
    }
    if (__builtin_fabs(c.err - c.err_prev) < p.min_error_change || c.err < p.min_error) {
        c.stop = PLSLAM_LBA_STOP_ERR;
        c.apply = -1;
        return false;
    }
    c.apply = c.err > c.err_prev ? 0 : 1;
    return true;
}

PLSLAM_LM_HD inline void lm_on_pivots(LbaLmCtl& c, int32_t n_bad)
{
    c.n_bad_pivots += n_bad;
    if (n_bad > 0) {
        c.stop = PLSLAM_LBA_STOP_NOT_PD;
        c.apply = 0;
    }
}

PLSLAM_LM_HD inline void lm_on_step(LbaLmCtl& c, const LbaLmPrm& p, double dx_sumsq_landmarks)
{
    // (selects, no early return: with the test as a branch that returns, the gfx950 code of the one-lane control kernel stored the
    // old err_prev on the path behind the first pass -- read in its assembly, seen on the device as a loop that never rejects)
    const bool later = c.n_builds > 1;                 // the first pass: no schedule, no ||DX|| test (:1552-1578)
    if (later) c.lambda = c.apply ? c.lambda * p.lambda_k : c.lambda / p.lambda_k;
    const bool small_step = later && __builtin_sqrt(c.dp_sumsq + dx_sumsq_landmarks) < p.min_error_change;
    const int32_t iters = c.iters + 1;
    c.err_prev = small_step ? c.err_prev : c.err;
    c.iters = small_step ? c.iters : iters;
    c.stop = small_step ? (int32_t)PLSLAM_LBA_STOP_DX : iters >= p.max_iters ? (int32_t)PLSLAM_LBA_STOP_MAX_ITERS : c.stop;
}

}  // namespace plslam
