// The lift of a pixel onto the normalised image plane through a camera's distortion model (cv::undistortPoints without R and P; contract:
// include/pmv_hip.h, pmv_undistort_points). lift_point below is the ONE device statement of the arithmetic: k_undistort_points
// (frontend_lift.hip), k_klt_observe[_many] and k_klt_lift_f[_many] (frontend_klt.hip) call it. Double, IEEE + - * / in the order written,
// no contraction (the library is built with -ffp-contract=off). The CPU restatement the tests hold the bits to is tests/twin/lift_twin.cpp.
// project_point is the way back: a point of the camera frame through the forward model onto the image (cv::projectPoints without rvec and
// tvec; pmv_project_points), stated once in the same manner; its CPU restatement is tests/twin/project_twin.cpp.
// A camera is of one of two models (LiftCam::model, the same for every lane of a launch, so the branch is uniform): the eight-coefficient
// radial-tangential one, and the equidistant one of cv::fisheye (Kannala-Brandt; pmv_camera_create_fisheye), whose two directions are
// fisheye_lift and fisheye_project below. Those need atan and tan, which are stated here too, in + - * / on literals (pmv_atan, pmv_tan: no
// math library's atan / tan is the same on the device and the host), and a square root, which is the correctly rounded one on both sides.
// They are __host__ __device__: pmv_fisheye_map_build (fisheye_map, frontend_remap.hip) runs fisheye_project on the host. Their CPU restatement is
// tests/twin/fisheye_twin.cpp; the constants come from scripts/derive_atan_tan.py.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pmv {

// A camera as the kernels read it, one entry of the context's device table (PMV_MAX_CAMERAS entries; the entry is the same for every lane,
// so its loads are uniform). ifx = 1.0 / fx and ify = 1.0 / fy are computed once on the host; fx and fy are the caller's own values.
struct LiftCam {
    double cx, cy, ifx, ify;
    double k1, k2, p1, p2, k3, k4, k5, k6;
    int iters, model;   // model: LIFT_RADTAN or LIFT_FISHEYE; a fisheye camera keeps its k[0..3] in k1, k2, k3, k4 and reads no other coefficient
    double fx, fy;
};
enum { LIFT_RADTAN = 0, LIFT_FISHEYE = 1 };

// atan on [0, inf), relative error below 2^-50. The argument is brought into |t| <= 7/16 by atan x = atan c + atan((x - c) /
// (1 + c x)) for c = 0.5, 1, 1.5 and by atan x = pi/2 - atan(1 / x); the five cases differ in operands only, so there is one division and no
// divergent branch. There atan t = t - t (z A(z)), z = t t, A of degree 13; the constant atan c comes in two parts.
__host__ __device__ __forceinline__ double pmv_atan(double x) {
    double num = x, den = 1.0, hi = 0.0, lo = 0.0;
    if (x >= 0.4375) { num = 2.0 * x - 1.0; den = 2.0 + x; hi = 0x1.dac670561bb4fp-2; lo = 0x1.a2b7f222f65e2p-56; }
    if (x >= 0.6875) { num = x - 1.0; den = x + 1.0; hi = 0x1.921fb54442d18p-1; lo = 0x1.1a62633145c07p-55; }
    if (x >= 1.1875) { num = x - 1.5; den = 1.0 + 1.5 * x; hi = 0x1.f730bd281f69bp-1; lo = 0x1.007887af0cbbdp-56; }
    if (x >= 2.4375) { num = -1.0; den = x; hi = 0x1.921fb54442d18p+0; lo = 0x1.1a62633145c07p-54; }
    const double t = num / den, z = t * t;
    double a = -0x1.5d5faa4833839p-7;
    a = a * z + 0x1.a6bf351c93cbap-6; a = a * z - 0x1.2af8fb9b78149p-5; a = a * z + 0x1.5e0521f3326b2p-5; a = a * z - 0x1.852a8f9a22e39p-5;
    a = a * z + 0x1.af0eddd1736b8p-5; a = a * z - 0x1.e1dfee494f386p-5; a = a * z + 0x1.111103b1c1bf8p-4; a = a * z - 0x1.3b13b0be2c090p-4;
    a = a * z + 0x1.745d1742db484p-4; a = a * z - 0x1.c71c71c711a64p-4; a = a * z + 0x1.24924924923eep-3; a = a * z - 0x1.9999999999999p-3;
    a = a * z + 0x1.5555555555555p-2;
    return hi + (lo + (t - t * (z * a)));
}

// tan on [0, pi/2] (pi/2 the double 0x1.921fb54442d18p+0), relative error below 2^-50. Up to pi/4: tan x = x + x (z T(z)), z = x x, T of degree
// 16. Beyond: the reciprocal of the tangent of the complement, which is formed with a two-part pi/2 (the first difference is exact).
__host__ __device__ __forceinline__ double pmv_tan(double x) {
    const bool upper = x > 0x1.921fb54442d18p-1;
    const double w = upper ? (0x1.921fb54442d18p+0 - x) + 0x1.1a62633145c07p-54 : x, z = w * w;
    double a = 0x1.ed9a40629b5cap-20;
    a = a * z - 0x1.5689e9cdf429fp-18; a = a * z + 0x1.5eb0f15cba348p-17; a = a * z - 0x1.f488308cecb1dp-18; a = a * z + 0x1.d24e2f91cdbe0p-17;
    a = a * z + 0x1.91536255d67b4p-17; a = a * z + 0x1.5677978a5ce77p-15; a = a * z + 0x1.949cfc61c6fcbp-14; a = a * z + 0x1.f5b10588249cfp-13;
    a = a * z + 0x1.35561ee6aaab9p-11; a = a * z + 0x1.7da3816c2c352p-10; a = a * z + 0x1.d6d3cfbf1a15ep-9; a = a * z + 0x1.226e35622425cp-7;
    a = a * z + 0x1.664f4882b24afp-6; a = a * z + 0x1.ba1ba1ba1bc09p-5; a = a * z + 0x1.1111111111110p-3; a = a * z + 0x1.5555555555555p-2;
    const double t = w + w * (z * a);
    return upper ? 1.0 / t : t;
}

// finite, in arithmetic that is the same statement on the host and the device (inf - inf and NaN - NaN are NaN)
__host__ __device__ __forceinline__ bool lift_fin(double x) { return x - x == 0.0; }
__host__ __device__ __forceinline__ bool lift_fin(float x) { return x - x == 0.f; }

// the equidistant model, inverse (cv::fisheye::undistortPoints without R / P): Newton on theta (1 + k1 theta^2 + ..) = theta_d from theta_d, at
// most 10 steps, a plain loop with a per-lane exit. A point that did not converge, or whose angle left [0, pi/2], is refused.
__host__ __device__ __forceinline__ bool fisheye_lift(const LiftCam& c, float u, float v, double* xd, double* yd) {
    const double PI_2 = 0x1.921fb54442d18p+0;
    const double px = ((double)u - c.cx) * c.ifx, py = ((double)v - c.cy) * c.ify;
    double td = sqrt(px * px + py * py);
    if (td > PI_2) td = PI_2;
    double s = 1.0;
    bool good = true;
    if (td > 1e-8) {
        double t = td;
        bool converged = false;
#pragma unroll 1
        for (int it = 0; it < 10; it++) {
            const double t2 = t * t, t4 = t2 * t2, t6 = t4 * t2, t8 = t4 * t4;
            const double fix = (t * (1 + c.k1 * t2 + c.k2 * t4 + c.k3 * t6 + c.k4 * t8) - td) / (1 + 3 * c.k1 * t2 + 5 * c.k2 * t4 + 7 * c.k3 * t6 + 9 * c.k4 * t8);
            t = t - fix;
            if (fix > -1e-8 && fix < 1e-8) { converged = true; break; }
        }
        good = converged && t >= 0.0 && t <= PI_2;
        if (good) s = pmv_tan(t) / td;
    }
    const double x = px * s, y = py * s;
    *xd = x; *yd = y;
    return good && lift_fin(x) && lift_fin(y);
}

// the equidistant model, forward (cv::fisheye::projectPoints without rvec / tvec, skew 0); ok and the refusal as project_point, and r finite
__host__ __device__ __forceinline__ bool fisheye_project(const LiftCam& c, double X, double Y, double Z, float* uf, float* vf) {
    bool ok = lift_fin(X) && lift_fin(Y) && lift_fin(Z) && Z > 0.0;
    const double a = X / Z, b = Y / Z, r2 = a * a + b * b, r = sqrt(r2);
    ok = ok && lift_fin(r);
    const double t = pmv_atan(r);   // (a point that is refused may give any t: nothing of it is written)
    const double t2 = t * t, t4 = t2 * t2, t6 = t4 * t2, t8 = t4 * t4;
    const double td = t * (1 + c.k1 * t2 + c.k2 * t4 + c.k3 * t6 + c.k4 * t8);
    const double s = r > 1e-8 ? td / r : 1.0;
    const double ud = c.fx * (a * s) + c.cx, vd = c.fy * (b * s) + c.cy;
    const float u = (float)ud, v = (float)vd;
    ok = ok && lift_fin(ud) && lift_fin(vd) && lift_fin(u) && lift_fin(v) && u >= -1e6f && u <= 1e6f && v >= -1e6f && v <= 1e6f;
    *uf = ok ? u : 0.f; *vf = ok ? v : 0.f;
    return ok;
}

// (u, v) -> (*xd, *yd), the doubles before their rounding to float; true iff both are finite
__device__ __forceinline__ bool lift_point(const LiftCam& c, float u, float v, double* xd, double* yd) {
    if (c.model == LIFT_FISHEYE) return fisheye_lift(c, u, v, xd, yd);
    const double x0 = ((double)u - c.cx) * c.ifx, y0 = ((double)v - c.cy) * c.ify;
    double x = x0, y = y0;
    for (int it = 0; it < c.iters; it++) {
        const double r2 = x * x + y * y;
        const double icdist = (1 + ((c.k6 * r2 + c.k5) * r2 + c.k4) * r2) / (1 + ((c.k3 * r2 + c.k2) * r2 + c.k1) * r2);
        const double dX = 2 * c.p1 * x * y + c.p2 * (r2 + 2 * x * x);
        const double dY = c.p1 * (r2 + 2 * y * y) + 2 * c.p2 * x * y;
        x = (x0 - dX) * icdist; y = (y0 - dY) * icdist;
    }
    *xd = x; *yd = y;
    return isfinite(x) && isfinite(y);
}
// the lift as the calls return it: rounded to float, ok iff finite before and after the rounding; a refused point is (0, 0) - no NaN is written
__device__ __forceinline__ bool lift_point_f(const LiftCam& c, float u, float v, float* xf, float* yf) {
    double xd, yd;
    bool ok = lift_point(c, u, v, &xd, &yd);
    const float x = (float)xd, y = (float)yd;
    ok = ok && isfinite(x) && isfinite(y);
    *xf = ok ? x : 0.f; *yf = ok ? y : 0.f;
    return ok;
}

// (X, Y, Z) of the camera frame -> the pixel (*uf, *vf): ok iff X, Y, Z are finite, Z > 0, u and v are finite before and after their rounding
// to float and within 1e6 in magnitude (the bound pmv_lk_track_ex puts on an initial flow); a refused point is (0, 0)
__device__ __forceinline__ bool project_point(const LiftCam& c, double X, double Y, double Z, float* uf, float* vf) {
    if (c.model == LIFT_FISHEYE) return fisheye_project(c, X, Y, Z, uf, vf);
    bool ok = isfinite(X) && isfinite(Y) && isfinite(Z) && Z > 0.0;
    const double x = X / Z, y = Y / Z, r2 = x * x + y * y;
    const double kr = (1 + ((c.k3 * r2 + c.k2) * r2 + c.k1) * r2) / (1 + ((c.k6 * r2 + c.k5) * r2 + c.k4) * r2);
    const double xd = x * kr + (2 * c.p1 * x * y + c.p2 * (r2 + 2 * x * x));
    const double yd = y * kr + (c.p1 * (r2 + 2 * y * y) + 2 * c.p2 * x * y);
    const double ud = c.fx * xd + c.cx, vd = c.fy * yd + c.cy;
    const float u = (float)ud, v = (float)vd;
    ok = ok && isfinite(ud) && isfinite(vd) && isfinite(u) && isfinite(v) && fabsf(u) <= 1e6f && fabsf(v) <= 1e6f;
    *uf = ok ? u : 0.f; *vf = ok ? v : 0.f;
    return ok;
}

// k_undistort_points: n points of camera `cam` (a device table entry), one lane per point; d_xy, d_out_xy: 2 n floats, d_ok: n bytes, all
// device-visible. One launch on s.
hipError_t launch_undistort_points(hipStream_t s, const LiftCam* cam, const float* d_xy, int n, float* d_out_xy, uint8_t* d_ok);
// k_project_points: the same for n camera-frame points d_xyz (3 n doubles) -> pixels
hipError_t launch_project_points(hipStream_t s, const LiftCam* cam, const double* d_xyz, int n, float* d_out_xy, uint8_t* d_ok);

}  // namespace pmv
