// pose_gn_dev.hpp -- the row math of the loop-closure pose-only Gauss-Newton system, shared by K17 (pose_gn.hip) and K25
// (loop_closure.hip): one point / line observation of MapHandler::computeRelativePoseRobustGN (src/mapHandler.cpp:3595-3689)
// evaluated at T_inc and folded into a lane's partial sums.  fp64, the source's operation order inside a row (the
// translation units are built with -ffp-contract=off).
#pragma once

#include <hip/hip_runtime.h>

#include "gn_cam.hpp"   // GnCam
#include "se3_dev.hpp"

namespace plslam {

constexpr int GN_TERMS = 21 + 6 + 1;       // upper triangle of H, g, e

__device__ __forceinline__ void jac6(double fgz2, double a, double b, double gx, double gy, double gz, double J[6])
{
    J[0] = +fgz2 * a * gz;
    J[1] = +fgz2 * b * gz;
    J[2] = -fgz2 * (gx * a + gy * b);
    J[3] = -fgz2 * (gx * gy * a + gy * gy * b + gz * gz * b);
    J[4] = +fgz2 * (gx * gx * a + gz * gz * a + gx * gy * b);
    J[5] = +fgz2 * (gx * gz * b - gy * gz * a);
}

__device__ __forceinline__ void accumulate(double acc[GN_TERMS], const double J[6], double r, double w)
{
    int k = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = i; j < 6; ++j) acc[k++] += J[i] * J[j] * w;     // (J J^T) w, evaluated as Eigen does: product, then * w
#pragma unroll
    for (int i = 0; i < 6; ++i) acc[21 + i] += J[i] * r * w;
    acc[27] += r * r * w;
}

// a point: X = lc_points[i]->P, (ox, oy) = pl_obs.  Returns ||err_i|| (:3600-3603; the outlier test of :3728-3738 uses it)
__device__ __forceinline__ double gn_point_residual(const GnCam& K, const double Tm[12], const double X[3], double ox, double oy,
                                                    double G[3], double& dx, double& dy)
{
    xform(Tm, X, G);
    const double u = K.cx + K.fx * G[0] / G[2], v = K.cy + K.fy * G[1] / G[2];
    dx = u - ox;
    dy = v - oy;
    return sqrt(dx * dx + dy * dy);
}

__device__ __forceinline__ void gn_point_row(const GnCam& K, double th, const double Tm[12], const double X[3], double ox, double oy,
                                             double acc[GN_TERMS])
{
    double G[3], J[6], dx, dy;
    const double r = gn_point_residual(K, Tm, X, ox, oy, G, dx, dy);
    const double fgz2 = K.fx / dmax_std(th, G[2] * G[2]);
    jac6(fgz2, dx, dy, G[0], G[1], G[2], J);
    const double den = dmax_std(th, r);
#pragma unroll
    for (int k = 0; k < 6; ++k) J[k] = J[k] / den;
    accumulate(acc, J, r, 1.0 / (1.0 + r * r));
}

// a line: SE = (sP, eP) of lc_lines[i], l = le_obs.  Returns ||err_i|| (:3631-3640, :3740-3756)
__device__ __forceinline__ double gn_line_residual(const GnCam& K, const double Tm[12], const double SE[6], const double l[3],
                                                   double S[3], double E[3], double& ds, double& de)
{
    xform(Tm, SE, S);
    xform(Tm, SE + 3, E);
    const double su = K.cx + K.fx * S[0] / S[2], sv = K.cy + K.fy * S[1] / S[2];
    const double eu = K.cx + K.fx * E[0] / E[2], ev = K.cy + K.fy * E[1] / E[2];
    ds = l[0] * su + l[1] * sv + l[2];
    de = l[0] * eu + l[1] * ev + l[2];
    return sqrt(ds * ds + de * de);
}

__device__ __forceinline__ void gn_line_row(const GnCam& K, double th, const double Tm[12], const double SE[6], const double l[3],
                                            double acc[GN_TERMS])
{
    double S[3], E[3], Js[6], Je[6], J[6], ds, de;
    const double r = gn_line_residual(K, Tm, SE, l, S, E, ds, de);
    jac6(K.fx / dmax_std(th, S[2] * S[2]), l[0], l[1], S[0], S[1], S[2], Js);
    jac6(K.fx / dmax_std(th, E[2] * E[2]), l[0], l[1], E[0], E[1], E[2], Je);
    const double den = dmax_std(th, r);
#pragma unroll
    for (int k = 0; k < 6; ++k) J[k] = (Js[k] * ds + Je[k] * de) / den;
    accumulate(acc, J, r, 1.0 / (1.0 + r * r));
}

}  // namespace plslam
