// CPU restatement of the equidistant (cv::fisheye) camera model of include/pmv_hip.h (pmv_camera_create_fisheye): pmv_atan and pmv_tan, the
// inverse (pmv_undistort_points) and the forward direction (pmv_project_points), pmv_fisheye_map_build, and - for a camera of either model -
// the stage-9 rule of the tracker step (pmv_klt_set_observe) and the virtual-camera points of stage 3 with undistorted_f. The yardstick for
// bits: double, IEEE + - * / in the order the header writes them and the correctly rounded square root; built with -ffp-contract=off
// -fno-fast-math (tests/fisheye_common.py). The device statement is in practical-multi-view_amd/csrc/pmv_lift.h.
// A camera is 14 doubles: fx, fy, cx, cy, then 8 coefficients, iters, model. Model 0 is the radial-tangential camera of
// tests/twin/lift_twin.cpp (coefficients k1, k2, p1, p2, k3, k4, k5, k6); model 1 is the fisheye camera (k1, k2, k3, k4 and four zeros; iters
// is not read).
#include <cmath>
#include <cstddef>
#include <cstdint>

namespace {

const double PI_2 = 0x1.921fb54442d18p+0;

double tw_atan(double x) {
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

double tw_tan(double x) {
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

struct Cam { double fx, fy, cx, cy, ifx, ify, k1, k2, p1, p2, k3, k4, k5, k6; int iters, model; };

Cam cam_of(const double* c) {
    Cam m;
    m.fx = c[0]; m.fy = c[1]; m.ifx = 1.0 / c[0]; m.ify = 1.0 / c[1]; m.cx = c[2]; m.cy = c[3];
    m.iters = (int)c[12]; m.model = (int)c[13];
    if (m.model == 1) { m.k1 = c[4]; m.k2 = c[5]; m.k3 = c[6]; m.k4 = c[7]; m.p1 = m.p2 = m.k5 = m.k6 = 0.0; }
    else { m.k1 = c[4]; m.k2 = c[5]; m.p1 = c[6]; m.p2 = c[7]; m.k3 = c[8]; m.k4 = c[9]; m.k5 = c[10]; m.k6 = c[11]; }
    return m;
}

bool fisheye_lift_d(const Cam& c, float u, float v, double* xd, double* yd) {
    const double px = ((double)u - c.cx) * c.ifx, py = ((double)v - c.cy) * c.ify;
    double td = std::sqrt(px * px + py * py);
    if (td > PI_2) td = PI_2;
    double s = 1.0;
    bool good = true;
    if (td > 1e-8) {
        double t = td;
        bool converged = false;
        for (int it = 0; it < 10; it++) {
            const double t2 = t * t, t4 = t2 * t2, t6 = t4 * t2, t8 = t4 * t4;
            const double fix = (t * (1 + c.k1 * t2 + c.k2 * t4 + c.k3 * t6 + c.k4 * t8) - td) / (1 + 3 * c.k1 * t2 + 5 * c.k2 * t4 + 7 * c.k3 * t6 + 9 * c.k4 * t8);
            t = t - fix;
            if (std::fabs(fix) < 1e-8) { converged = true; break; }
        }
        good = converged && t >= 0.0 && t <= PI_2;
        if (good) s = tw_tan(t) / td;
    }
    const double x = px * s, y = py * s;
    *xd = x; *yd = y;
    return good && std::isfinite(x) && std::isfinite(y);
}

// the radial-tangential lift, as tests/twin/lift_twin.cpp states it
bool radtan_lift_d(const Cam& c, float u, float v, double* xd, double* yd) {
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
    return std::isfinite(x) && std::isfinite(y);
}

bool lift_d(const Cam& c, float u, float v, double* xd, double* yd) {
    return c.model == 1 ? fisheye_lift_d(c, u, v, xd, yd) : radtan_lift_d(c, u, v, xd, yd);
}

bool lift_f(const Cam& c, float u, float v, float* xf, float* yf) {
    double xd, yd;
    bool ok = lift_d(c, u, v, &xd, &yd);
    const float x = (float)xd, y = (float)yd;
    ok = ok && std::isfinite(x) && std::isfinite(y);
    *xf = ok ? x : 0.f; *yf = ok ? y : 0.f;
    return ok;
}

bool fisheye_project_f(const Cam& c, double X, double Y, double Z, float* uf, float* vf) {
    bool ok = std::isfinite(X) && std::isfinite(Y) && std::isfinite(Z) && Z > 0.0;
    const double a = X / Z, b = Y / Z, r2 = a * a + b * b, r = std::sqrt(r2);
    ok = ok && std::isfinite(r);
    const double t = tw_atan(r);
    const double t2 = t * t, t4 = t2 * t2, t6 = t4 * t2, t8 = t4 * t4;
    const double td = t * (1 + c.k1 * t2 + c.k2 * t4 + c.k3 * t6 + c.k4 * t8);
    const double s = r > 1e-8 ? td / r : 1.0;
    const double ud = c.fx * (a * s) + c.cx, vd = c.fy * (b * s) + c.cy;
    const float u = (float)ud, v = (float)vd;
    ok = ok && std::isfinite(ud) && std::isfinite(vd) && std::isfinite(u) && std::isfinite(v) && std::fabs(u) <= 1e6f && std::fabs(v) <= 1e6f;
    *uf = ok ? u : 0.f; *vf = ok ? v : 0.f;
    return ok;
}

// the radial-tangential projection, as tests/twin/project_twin.cpp states it
bool radtan_project_f(const Cam& c, double X, double Y, double Z, float* uf, float* vf) {
    bool ok = std::isfinite(X) && std::isfinite(Y) && std::isfinite(Z) && Z > 0.0;
    const double x = X / Z, y = Y / Z, r2 = x * x + y * y;
    const double kr = (1 + ((c.k3 * r2 + c.k2) * r2 + c.k1) * r2) / (1 + ((c.k6 * r2 + c.k5) * r2 + c.k4) * r2);
    const double xd = x * kr + (2 * c.p1 * x * y + c.p2 * (r2 + 2 * x * x));
    const double yd = y * kr + (c.p1 * (r2 + 2 * y * y) + 2 * c.p2 * x * y);
    const double ud = c.fx * xd + c.cx, vd = c.fy * yd + c.cy;
    const float u = (float)ud, v = (float)vd;
    ok = ok && std::isfinite(ud) && std::isfinite(vd) && std::isfinite(u) && std::isfinite(v) && std::fabs(u) <= 1e6f && std::fabs(v) <= 1e6f;
    *uf = ok ? u : 0.f; *vf = ok ? v : 0.f;
    return ok;
}

}  // namespace

extern "C" {

void fisheye_twin_atan(const double* x, int n, double* out) { for (int i = 0; i < n; i++) out[i] = tw_atan(x[i]); }
void fisheye_twin_tan(const double* x, int n, double* out) { for (int i = 0; i < n; i++) out[i] = tw_tan(x[i]); }

// pmv_undistort_points
int fisheye_twin_points(const double* cam14, const float* xy, int n, float* out_xy, uint8_t* out_ok) {
    const Cam c = cam_of(cam14);
    for (int i = 0; i < n; i++) out_ok[i] = lift_f(c, xy[2 * i], xy[2 * i + 1], out_xy + 2 * i, out_xy + 2 * i + 1) ? 1 : 0;
    return 0;
}

// the clamped theta_d of a pixel, and what the Newton loop made of it: out3 = {td, t after the loop, converged}; (td, td, 1) when td <= 1e-8
int fisheye_twin_newton(const double* cam14, float u, float v, double* out3) {
    const Cam c = cam_of(cam14);
    const double px = ((double)u - c.cx) * c.ifx, py = ((double)v - c.cy) * c.ify;
    double td = std::sqrt(px * px + py * py);
    if (td > PI_2) td = PI_2;
    double t = td;
    bool converged = !(td > 1e-8);
    if (td > 1e-8)
        for (int it = 0; it < 10; it++) {
            const double t2 = t * t, t4 = t2 * t2, t6 = t4 * t2, t8 = t4 * t4;
            const double fix = (t * (1 + c.k1 * t2 + c.k2 * t4 + c.k3 * t6 + c.k4 * t8) - td) / (1 + 3 * c.k1 * t2 + 5 * c.k2 * t4 + 7 * c.k3 * t6 + 9 * c.k4 * t8);
            t = t - fix;
            if (std::fabs(fix) < 1e-8) { converged = true; break; }
        }
    out3[0] = td; out3[1] = t; out3[2] = converged ? 1.0 : 0.0;
    return 0;
}

// pmv_project_points
int fisheye_twin_project(const double* cam14, const double* xyz, int n, float* out_xy, uint8_t* out_ok) {
    const Cam c = cam_of(cam14);
    for (int i = 0; i < n; i++) {
        float* o = out_xy + 2 * i;
        out_ok[i] = (c.model == 1 ? fisheye_project_f(c, xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], o, o + 1) : radtan_project_f(c, xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], o, o + 1)) ? 1 : 0;
    }
    return 0;
}

// pmv_fisheye_map_build; 1: newK R is singular, nothing written
int fisheye_twin_map(const double* K, const double* k4, const double* R, const double* newK, int w, int h, float* map_x, float* map_y) {
    const double I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    const double* Rm = R ? R : I;
    const double* N = newK ? newK : K;
    double A[9];
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) A[3 * r + c] = N[3 * r] * Rm[c] + N[3 * r + 1] * Rm[3 + c] + N[3 * r + 2] * Rm[6 + c];
    const double c00 = A[4] * A[8] - A[5] * A[7], c01 = A[5] * A[6] - A[3] * A[8], c02 = A[3] * A[7] - A[4] * A[6];
    const double det = A[0] * c00 + A[1] * c01 + A[2] * c02;
    if (!(std::fabs(det) > 0.0) || !std::isfinite(det)) return 1;
    const double iR[9] = {c00 / det, (A[2] * A[7] - A[1] * A[8]) / det, (A[1] * A[5] - A[2] * A[4]) / det,
                          c01 / det, (A[0] * A[8] - A[2] * A[6]) / det, (A[2] * A[3] - A[0] * A[5]) / det,
                          c02 / det, (A[1] * A[6] - A[0] * A[7]) / det, (A[0] * A[4] - A[1] * A[3]) / det};
    const double cam14[14] = {K[0], K[4], K[2], K[5], k4[0], k4[1], k4[2], k4[3], 0, 0, 0, 0, 10, 1};
    const Cam cam = cam_of(cam14);
    for (int i = 0; i < h; i++)
        for (int j = 0; j < w; j++) {
            const double X = iR[0] * j + iR[1] * i + iR[2], Y = iR[3] * j + iR[4] * i + iR[5], W = iR[6] * j + iR[7] * i + iR[8];
            float u, v;
            const bool ok = fisheye_project_f(cam, X, Y, W, &u, &v);
            map_x[(size_t)i * w + j] = ok ? u : -1.f;
            map_y[(size_t)i * w + j] = ok ? v : -1.f;
        }
    return 0;
}

// stage 9 on a step's outputs; rcam14 null (or right_xy null): no right observations - right ok all 0, right xy untouched
int fisheye_twin_observe(const double* cam14, const double* rcam14, double dt, const int* ages, const float* xy, const float* prev_xy, const float* right_xy,
                         const uint8_t* right_status, int n, float* out_un, float* out_vel, uint8_t* out_ok, float* out_run, uint8_t* out_rok) {
    const Cam c = cam_of(cam14);
    for (int i = 0; i < n; i++) {
        float ux, uy, px, py;
        const bool ok = lift_f(c, xy[2 * i], xy[2 * i + 1], &ux, &uy), pok = lift_f(c, prev_xy[2 * i], prev_xy[2 * i + 1], &px, &py);
        out_un[2 * i] = ux; out_un[2 * i + 1] = uy; out_ok[i] = ok ? 1 : 0;
        float vx = 0.f, vy = 0.f;
        if (ages[i] > 1 && ok && pok) {
            const float dx = ux - px, dy = uy - py;
            vx = (float)((double)dx / dt); vy = (float)((double)dy / dt);
        }
        out_vel[2 * i] = vx; out_vel[2 * i + 1] = vy;
    }
    if (rcam14 && right_xy) {
        const Cam r = cam_of(rcam14);
        for (int i = 0; i < n; i++) {
            const bool rok = lift_f(r, right_xy[2 * i], right_xy[2 * i + 1], out_run + 2 * i, out_run + 2 * i + 1);
            out_rok[i] = right_status[i] && rok ? 1 : 0;
        }
    } else {
        for (int i = 0; i < n; i++) out_rok[i] = 0;
    }
    return 0;
}

// stage 3's two point sets with undistorted_f: the virtual-camera points of the survivors' previous and current positions
int fisheye_twin_f_points(const double* cam14, double f_focal, int w, int h, const float* prev_xy, const float* cur_xy, int n, float* p1, float* p2) {
    const Cam c = cam_of(cam14);
    for (int i = 0; i < n; i++) {
        double ax, ay, bx, by;
        const bool oka = lift_d(c, prev_xy[2 * i], prev_xy[2 * i + 1], &ax, &ay), okb = lift_d(c, cur_xy[2 * i], cur_xy[2 * i + 1], &bx, &by);
        const bool ok = oka && okb;
        p1[2 * i] = ok ? (float)(f_focal * ax + w / 2.0) : 0.f; p1[2 * i + 1] = ok ? (float)(f_focal * ay + h / 2.0) : 0.f;
        p2[2 * i] = ok ? (float)(f_focal * bx + w / 2.0) : 0.f; p2[2 * i + 1] = ok ? (float)(f_focal * by + h / 2.0) : 0.f;
    }
    return 0;
}

}  // extern "C"
