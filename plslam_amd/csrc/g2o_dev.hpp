// g2o_dev.hpp -- g2o's SE(3) and quaternion maps as the loop-closure pose graph needs them on the device (pgo.hip, K40-K49):
// isometries (R row-major, t), Eigen's Quaternion(Matrix3) and toRotationMatrix, SE3Quat::exp / log, fromVectorMQT.  The constants
// are those of tests/pgo_ref.py (G2O).  Built with -ffp-contract=off like se3_dev.hpp, on whose small products it rests.
#pragma once

#include "se3_dev.hpp"

namespace plslam {

// ---- isometries (R row-major, t) and g2o's maps -----------------------------------------------------------------------------
struct Iso { double R[9], t[3]; };

__device__ __forceinline__ void iso_load(const double* __restrict__ p, Iso& X)
{
#pragma unroll
    for (int a = 0; a < 9; ++a) X.R[a] = p[a];
#pragma unroll
    for (int a = 0; a < 3; ++a) X.t[a] = p[9 + a];
}
__device__ __forceinline__ void iso_store(const Iso& X, double* __restrict__ p)
{
#pragma unroll
    for (int a = 0; a < 9; ++a) p[a] = X.R[a];
#pragma unroll
    for (int a = 0; a < 3; ++a) p[9 + a] = X.t[a];
}
__device__ __forceinline__ void iso_mul(const Iso& A, const Iso& B, Iso& C)
{
    mat3_mul(A.R, B.R, C.R);
    double u[3];
    mv3(A.R, B.t, u);         // (not xform(A.R, A.t, B.t, C.t): the same sums, but the kernels' instruction streams change)
#pragma unroll
    for (int i = 0; i < 3; ++i) C.t[i] = u[i] + A.t[i];
}
// (not inv_pose: that one negates the factors, this one the finished sum, as g2o's Isometry3::inverse does)
__device__ __forceinline__ void iso_inv(const Iso& A, Iso& C)
{
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) C.R[3 * i + j] = A.R[3 * j + i];
    double u[3];
    mv3(C.R, A.t, u);
#pragma unroll
    for (int i = 0; i < 3; ++i) C.t[i] = -u[i];
}
// Eigen's Quaternion(const Matrix3&) -> (w, x, y, z)
__device__ __forceinline__ void quat_from_R(const double R[9], double q[4])
{
    const double tr = R[0] + R[4] + R[8];
    if (tr > 0.0) {
        double t = sqrt(tr + 1.0);
        q[0] = 0.5 * t;
        t = 0.5 / t;
        q[1] = (R[7] - R[5]) * t;
        q[2] = (R[2] - R[6]) * t;
        q[3] = (R[3] - R[1]) * t;
    } else {
        int i = 0;
        if (R[4] > R[0]) i = 1;
        if (R[8] > R[4 * i]) i = 2;
        const int j = (i + 1) % 3, k = (j + 1) % 3;
        double t = sqrt(R[4 * i] - R[4 * j] - R[4 * k] + 1.0);
        q[1 + i] = 0.5 * t;
        t = 0.5 / t;
        q[0] = (R[3 * k + j] - R[3 * j + k]) * t;
        q[1 + j] = (R[3 * j + i] + R[3 * i + j]) * t;
        q[1 + k] = (R[3 * k + i] + R[3 * i + k]) * t;
    }
}
__device__ __forceinline__ void unit_quat(const double R[9], double q[4])
{
    quat_from_R(R, q);
    const double n = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
#pragma unroll
    for (int a = 0; a < 4; ++a) q[a] /= n;
    if (q[0] < 0.0) {
#pragma unroll
        for (int a = 0; a < 4; ++a) q[a] = -q[a];
    }
}
__device__ __forceinline__ void R_from_quat(const double q[4], double R[9])
{
    const double w = q[0], x = q[1], y = q[2], z = q[3];
    const double tx = 2.0 * x, ty = 2.0 * y, tz = 2.0 * z;
    const double twx = tx * w, twy = ty * w, twz = tz * w, txx = tx * x, txy = ty * x, txz = tz * x, tyy = ty * y, tyz = tz * y,
                 tzz = tz * z;
    R[0] = 1.0 - (tyy + tzz); R[1] = txy - twz;         R[2] = txz + twy;
    R[3] = txy + twz;         R[4] = 1.0 - (txx + tzz); R[5] = tyz - twx;
    R[6] = txz - twy;         R[7] = tyz + twx;         R[8] = 1.0 - (txx + tyy);
}
// SE3Quat::exp([omega; upsilon]) as an isometry (constants: tests/pgo_ref.py G2O)
__device__ __forceinline__ void se3quat_exp(const double u[6], Iso& X)
{
    const double w[3] = {u[0], u[1], u[2]};
    const double theta = sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
    double Om[9], Om2[9], R[9], V[9];
    skew3(w, Om);
    mat3_mul(Om, Om, Om2);
    if (theta < 1e-5) {
#pragma unroll
        for (int k = 0; k < 9; ++k) { R[k] = ((k % 4 == 0) ? 1.0 : 0.0) + Om[k] + Om2[k]; V[k] = R[k]; }
    } else {
        const double t2 = theta * theta, s = sin(theta), c = cos(theta);
        const double a = s / theta, b = (1.0 - c) / t2, d = (theta - s) / (t2 * theta);
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            const double id = (k % 4 == 0) ? 1.0 : 0.0;
            R[k] = id + a * Om[k] + b * Om2[k];
            V[k] = id + b * Om[k] + d * Om2[k];
        }
    }
    double q[4];
    unit_quat(R, q);
    R_from_quat(q, X.R);
    mv3(V, u + 3, X.t);
}
// SE3Quat(estimate()).log() -> [omega; V^-1 t]
__device__ __forceinline__ void se3quat_log(const Iso& X, double u[6])
{
    double q[4], R[9];
    unit_quat(X.R, q);
    R_from_quat(q, R);
    const double d = 0.5 * (R[0] + R[4] + R[8] - 1.0);
    const double dR[3] = {R[7] - R[5], R[2] - R[6], R[3] - R[1]};
    double w[3], Om[9], Om2[9], Vi[9];
    if (d > 0.99999) {
#pragma unroll
        for (int a = 0; a < 3; ++a) w[a] = 0.5 * dR[a];
        skew3(w, Om);
        mat3_mul(Om, Om, Om2);
#pragma unroll
        for (int k = 0; k < 9; ++k) Vi[k] = ((k % 4 == 0) ? 1.0 : 0.0) - 0.5 * Om[k] + Om2[k] / 12.0;
    } else {
        const double theta = acos(d);
        const double f = theta / (2.0 * sqrt(1.0 - d * d));
#pragma unroll
        for (int a = 0; a < 3; ++a) w[a] = f * dR[a];
        skew3(w, Om);
        mat3_mul(Om, Om, Om2);
        const double g = (1.0 - theta / (2.0 * tan(theta / 2.0))) / (theta * theta);
#pragma unroll
        for (int k = 0; k < 9; ++k) Vi[k] = ((k % 4 == 0) ? 1.0 : 0.0) - 0.5 * Om[k] + g * Om2[k];
    }
    u[0] = w[0]; u[1] = w[1]; u[2] = w[2];
    mv3(Vi, X.t, u + 3);
}
__device__ __forceinline__ void from_vector_mqt(const double v[6], Iso& X)
{
    const double n = 1.0 - (v[3] * v[3] + v[4] * v[4] + v[5] * v[5]);
    if (n < 0.0) {
#pragma unroll
        for (int k = 0; k < 9; ++k) X.R[k] = (k % 4 == 0) ? 1.0 : 0.0;
    } else {
        const double q[4] = {sqrt(n), v[3], v[4], v[5]};
        R_from_quat(q, X.R);
    }
    X.t[0] = v[0]; X.t[1] = v[1]; X.t[2] = v[2];
}
__device__ __forceinline__ void mat4_mul(const double a[16], const double b[16], double c[16])
{
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
            c[4 * i + j] = a[4 * i] * b[j] + a[4 * i + 1] * b[4 + j] + a[4 * i + 2] * b[8 + j] + a[4 * i + 3] * b[12 + j];
}
__device__ __forceinline__ void rev6(const double x[6], double u[6])
{
    u[0] = x[3]; u[1] = x[4]; u[2] = x[5]; u[3] = x[0]; u[4] = x[1]; u[5] = x[2];
}

}  // namespace plslam
