// se3_dev.hpp -- stvo-pl's SE(3) maps (expmap_se3 / logmap_se3 / inverse_se3, auxiliar.cpp) restated in fp64 for the device,
// their theta < 1e-6 branches included.  Shared by K25 (loop_closure.hip) and the pose update of the global BA (gba.hip).
#pragma once

#include <hip/hip_runtime.h>

namespace plslam {

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
