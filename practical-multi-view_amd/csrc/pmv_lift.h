// The lift of a pixel onto the normalised image plane through a camera's distortion model (cv::undistortPoints without R and P; contract:
// include/pmv_hip.h, pmv_undistort_points). lift_point below is the ONE device statement of the arithmetic: k_undistort_points
// (frontend_lift.hip), k_klt_observe[_many] and k_klt_lift_f[_many] (frontend_klt.hip) call it. Double, IEEE + - * / in the order written,
// no contraction (the library is built with -ffp-contract=off). The CPU restatement the tests hold the bits to is tests/twin/lift_twin.cpp.
// project_point is the way back: a point of the camera frame through the forward model onto the image (cv::projectPoints without rvec and
// tvec; pmv_project_points), stated once in the same manner; its CPU restatement is tests/twin/project_twin.cpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pmv {

// A camera as the kernels read it, one entry of the context's device table (PMV_MAX_CAMERAS entries; the entry is the same for every lane,
// so its loads are uniform). ifx = 1.0 / fx and ify = 1.0 / fy are computed once on the host; fx and fy are the caller's own values.
struct LiftCam {
    double cx, cy, ifx, ify;
    double k1, k2, p1, p2, k3, k4, k5, k6;
    int iters, pad;
    double fx, fy;
};

// (u, v) -> (*xd, *yd), the doubles before their rounding to float; true iff both are finite
__device__ __forceinline__ bool lift_point(const LiftCam& c, float u, float v, double* xd, double* yd) {
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
