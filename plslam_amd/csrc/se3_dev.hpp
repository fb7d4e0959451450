// se3_dev.hpp -- the one copy of the small fp64 device math: std::max / std::min as the reference orders the comparison, the
// rigid transform of a point, 3x3 products, the inverse of a pose, and stvo-pl's SE(3) maps (expmap_se3 / logmap_se3 /
// inverse_se3, auxiliar.cpp), their theta < 1e-6 branches included.  Every includer is built with -ffp-contract=off and every
// expression keeps the reference's order of operations (sums left to right).  Used by the row kernels (pose_gn_dev.hpp,
// lba_rows_dev.hpp, lba.hip, map2kf_kernels.hip), the stereo gates, K25 (loop_closure.hip), the global BA (gba.hip), the pose graph
// (pgo.hip, under g2o's maps in g2o_dev.hpp) and the map correction (lc_correct.hip).
#pragma once

#include <hip/hip_runtime.h>

namespace plslam {

// std::max / std::min of libstdc++: the SECOND argument is taken only when the comparison holds, so a NaN in either place
// and the sign of a zero come out as in the reference
__device__ __forceinline__ double dmax_std(double a, double b) { return a < b ? b : a; }
__device__ __forceinline__ double dmin_std(double a, double b) { return b < a ? b : a; }

// o = R X + t, ((r0 x + r1 y) + r2 z) + t per row; o may be X
__device__ __forceinline__ void xform(const double R[9], const double t[3], const double* X, double o[3])
{
    const double x = X[0], y = X[1], z = X[2];
#pragma unroll
    for (int i = 0; i < 3; ++i) o[i] = (R[3 * i] * x + R[3 * i + 1] * y + R[3 * i + 2] * z) + t[i];
}
// the same with R | t as rows 0..2 of a row-major 4x4 (12 or 16 doubles)
__device__ __forceinline__ void xform(const double* T, const double* X, double o[3])
{
    const double x = X[0], y = X[1], z = X[2];
#pragma unroll
    for (int i = 0; i < 3; ++i) o[i] = (T[4 * i] * x + T[4 * i + 1] * y + T[4 * i + 2] * z) + T[4 * i + 3];
}
__device__ __forceinline__ void mv3(const double R[9], const double v[3], double o[3])
{
#pragma unroll
    for (int i = 0; i < 3; ++i) o[i] = R[3 * i] * v[0] + R[3 * i + 1] * v[1] + R[3 * i + 2] * v[2];
}

__device__ __forceinline__ void skew3(const double w[3], double s[9])
{
    s[0] = 0.0;   s[1] = -w[2]; s[2] = w[1];
    s[3] = w[2];  s[4] = 0.0;   s[5] = -w[0];
    s[6] = -w[1]; s[7] = w[0];  s[8] = 0.0;
}

__device__ __forceinline__ void mat3_mul(const double a[9], const double b[9], double c[9])
{
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) c[3 * i + j] = a[3 * i] * b[j] + a[3 * i + 1] * b[3 + j] + a[3 * i + 2] * b[6 + j];
}

// inverse_se3 (stvo-pl): [R^T, -R^T t] of the row-major 4x4 at T (its first 12 doubles are read)
__device__ __forceinline__ void inv_pose(const double* __restrict__ T, double R[9], double t[3])
{
    double m[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) m[i] = T[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        R[3 * i] = m[i];
        R[3 * i + 1] = m[4 + i];
        R[3 * i + 2] = m[8 + i];
        t[i] = (-m[i]) * m[3] + (-m[4 + i]) * m[7] + (-m[8 + i]) * m[11];
    }
}
// the same as a row-major 4x4, the same operations in the same order.  Written out, not a call of inv_pose plus a copy: that
// form leaves k_pgo_meas and k_pgo_writeback with another instruction stream
__device__ __forceinline__ void inverse_se3(const double T[16], double o[16])
{
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) o[4 * i + j] = T[4 * j + i];
#pragma unroll
    for (int i = 0; i < 3; ++i) o[4 * i + 3] = (-T[4 * 0 + i]) * T[3] + (-T[4 * 1 + i]) * T[7] + (-T[4 * 2 + i]) * T[11];
    o[12] = 0.0; o[13] = 0.0; o[14] = 0.0; o[15] = 1.0;
}

__device__ __forceinline__ void expmap_se3(const double x[6], double T[16])
{
    double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    double tt[3] = {x[0], x[1], x[2]};
    const double theta = sqrt(x[3] * x[3] + x[4] * x[4] + x[5] * x[5]);
    if (!(theta < 0.000001)) {
        double s[9], s2[9], V[9];
        const double wn[3] = {x[3] / theta, x[4] / theta, x[5] / theta};
        skew3(wn, s);
        mat3_mul(s, s, s2);
        const double sn = sin(theta), cs = cos(theta);
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            const double id = (k % 4 == 0) ? 1.0 : 0.0;
            R[k] = id + s[k] * sn + s2[k] * (1.0 - cs);
            V[k] = id + s[k] * (1.0 - cs) / theta + s2[k] * (theta - sn) / theta;
        }
#pragma unroll
        for (int i = 0; i < 3; ++i) tt[i] = V[3 * i] * x[0] + V[3 * i + 1] * x[1] + V[3 * i + 2] * x[2];
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) T[4 * i + j] = R[3 * i + j];
        T[4 * i + 3] = tt[i];
    }
    T[12] = 0.0; T[13] = 0.0; T[14] = 0.0; T[15] = 1.0;
}

__device__ __forceinline__ void logmap_se3(const double T[16], double x[6])
{
    double R[9], V[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, w[3] = {0, 0, 0};
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) R[3 * i + j] = T[4 * i + j];
    double cosine = (R[0] + R[4] + R[8] - 1.0) / 2.0;
    if (cosine > 1.0) cosine = 1.0; else if (cosine < -1.0) cosine = -1.0;
    double sine = sqrt(1.0 - cosine * cosine);
    if (sine > 1.0) sine = 1.0; else if (sine < -1.0) sine = -1.0;
    const double theta = acos(cosine);
    if (theta > 0.000001) {
        w[0] = theta * (R[7] - R[5]) / (2.0 * sine);
        w[1] = theta * (R[2] - R[6]) / (2.0 * sine);
        w[2] = theta * (R[3] - R[1]) / (2.0 * sine);
        double s[9], s2[9];
        const double wn[3] = {w[0] / theta, w[1] / theta, w[2] / theta};
        skew3(wn, s);
        mat3_mul(s, s, s2);
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            const double id = (k % 4 == 0) ? 1.0 : 0.0;
            V[k] = id + s[k] * (1.0 - cosine) / theta + s2[k] * (theta - sine) / theta;
        }
    }
    double Vi[9];
    const double c0 = V[4] * V[8] - V[5] * V[7];
    const double c1 = V[5] * V[6] - V[3] * V[8];
    const double c2 = V[3] * V[7] - V[4] * V[6];
    const double det = V[0] * c0 + V[1] * c1 + V[2] * c2;
    if (det == 0.0) {
#pragma unroll
        for (int k = 0; k < 9; ++k) Vi[k] = V[k];
    } else {
        const double id = 1.0 / det;
        Vi[0] = c0 * id; Vi[1] = (V[2] * V[7] - V[1] * V[8]) * id; Vi[2] = (V[1] * V[5] - V[2] * V[4]) * id;
        Vi[3] = c1 * id; Vi[4] = (V[0] * V[8] - V[2] * V[6]) * id; Vi[5] = (V[2] * V[3] - V[0] * V[5]) * id;
        Vi[6] = c2 * id; Vi[7] = (V[1] * V[6] - V[0] * V[7]) * id; Vi[8] = (V[0] * V[4] - V[1] * V[3]) * id;
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) x[i] = Vi[3 * i] * T[3] + Vi[3 * i + 1] * T[7] + Vi[3 * i + 2] * T[11];
    x[3] = w[0]; x[4] = w[1]; x[5] = w[2];
}

}  // namespace plslam
