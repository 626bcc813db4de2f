// CPU restatement of the lift onto the normalised image plane (include/pmv_hip.h: pmv_undistort_points), of the stage-9 rule of the
// tracker step (pmv_klt_set_observe) and of the virtual-camera points of stage 3 with undistorted_f. The yardstick for bits: double, IEEE
// + - * / in the order the header writes them; built with -ffp-contract=off -fno-fast-math (tests/lift_common.py).
// A camera is 13 doubles: fx, fy, cx, cy, k1, k2, p1, p2, k3, k4, k5, k6, iters.
#include <cmath>
#include <cstdint>

namespace {

struct Cam { double cx, cy, ifx, ify, k1, k2, p1, p2, k3, k4, k5, k6; int iters; };

Cam cam_of(const double* c) {
    Cam m;
    m.ifx = 1.0 / c[0]; m.ify = 1.0 / c[1]; m.cx = c[2]; m.cy = c[3];
    m.k1 = c[4]; m.k2 = c[5]; m.p1 = c[6]; m.p2 = c[7]; m.k3 = c[8]; m.k4 = c[9]; m.k5 = c[10]; m.k6 = c[11];
    m.iters = (int)c[12];
    return m;
}

// the doubles before their rounding to float; true iff both are finite
bool lift_d(const Cam& c, float u, float v, double* xd, double* yd) {
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

bool lift_f(const Cam& c, float u, float v, float* xf, float* yf) {
    double xd, yd;
    bool ok = lift_d(c, u, v, &xd, &yd);
    const float x = (float)xd, y = (float)yd;
    ok = ok && std::isfinite(x) && std::isfinite(y);
    *xf = ok ? x : 0.f; *yf = ok ? y : 0.f;
    return ok;
}

}  // namespace

extern "C" {

// pmv_undistort_points
int lift_twin_points(const double* cam13, const float* xy, int n, float* out_xy, uint8_t* out_ok) {
    const Cam c = cam_of(cam13);
    for (int i = 0; i < n; i++) out_ok[i] = lift_f(c, xy[2 * i], xy[2 * i + 1], out_xy + 2 * i, out_xy + 2 * i + 1) ? 1 : 0;
    return 0;
}

// stage 9 on a step's outputs; rcam13 null (or right_xy null): no right observations - right ok all 0, right xy untouched
int lift_twin_observe(const double* cam13, const double* rcam13, double dt, const int* ages, const float* xy, const float* prev_xy, const float* right_xy,
                      const uint8_t* right_status, int n, float* out_un, float* out_vel, uint8_t* out_ok, float* out_run, uint8_t* out_rok) {
    const Cam c = cam_of(cam13);
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
    if (rcam13 && right_xy) {
        const Cam r = cam_of(rcam13);
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
int lift_twin_f_points(const double* cam13, double f_focal, int w, int h, const float* prev_xy, const float* cur_xy, int n, float* p1, float* p2) {
    const Cam c = cam_of(cam13);
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
