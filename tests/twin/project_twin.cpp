// CPU restatement of the projection of camera-frame points onto the image (include/pmv_hip.h: pmv_project_points; the device statement is
// project_point in pmv_lift.h). The yardstick for bits: double, IEEE + - * / in the order the header writes them; built with
// -ffp-contract=off -fno-fast-math (tests/predict_common.py).
// A camera is 13 doubles: fx, fy, cx, cy, k1, k2, p1, p2, k3, k4, k5, k6, iters (as tests/twin/lift_twin.cpp; iters is not used here).
#include <cmath>
#include <cstdint>

namespace {

bool project_f(const double* c, double X, double Y, double Z, float* uf, float* vf) {
    const double fx = c[0], fy = c[1], cx = c[2], cy = c[3], k1 = c[4], k2 = c[5], p1 = c[6], p2 = c[7], k3 = c[8], k4 = c[9], k5 = c[10], k6 = c[11];
    bool ok = std::isfinite(X) && std::isfinite(Y) && std::isfinite(Z) && Z > 0.0;
    const double x = X / Z, y = Y / Z, r2 = x * x + y * y;
    const double kr = (1 + ((k3 * r2 + k2) * r2 + k1) * r2) / (1 + ((k6 * r2 + k5) * r2 + k4) * r2);
    const double xd = x * kr + (2 * p1 * x * y + p2 * (r2 + 2 * x * x));
    const double yd = y * kr + (p1 * (r2 + 2 * y * y) + 2 * p2 * x * y);
    const double ud = fx * xd + cx, vd = fy * yd + cy;
    const float u = (float)ud, v = (float)vd;
    ok = ok && std::isfinite(ud) && std::isfinite(vd) && std::isfinite(u) && std::isfinite(v) && std::fabs(u) <= 1e6f && std::fabs(v) <= 1e6f;
    *uf = ok ? u : 0.f; *vf = ok ? v : 0.f;
    return ok;
}

}  // namespace

extern "C" {

// pmv_project_points
int project_twin_points(const double* cam13, const double* xyz, int n, float* out_xy, uint8_t* out_ok) {
    for (int i = 0; i < n; i++) out_ok[i] = project_f(cam13, xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], out_xy + 2 * i, out_xy + 2 * i + 1) ? 1 : 0;
    return 0;
}

}  // extern "C"
