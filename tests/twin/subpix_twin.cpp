// TEST INFRASTRUCTURE ONLY. CPU restatement of pmv_corner_subpix (include/pmv_hip.h): cv::cornerSubPix on level 0 of a gray frame.
// PARITY UNPINNED like the rest of the front end [mem: OpenCV 3.4 cornersubpix.cpp, samplers.cpp getRectSubPix_8u32f / getRectSubPix_Cn_ /
// adjustRect]; this file fixes the arithmetic the product follows:
//   - weight table: mask[i][j] = (float)(vy * expf(-x*x)), x = (float)(j - win_w) / win_w, vy = expf(-y*y), y likewise, libm's expf; the
//     zero zone is cleared only when it lies strictly inside the window, otherwise it is ignored;
//   - patch per iteration: getRectSubPix(src, (2 win_w + 3) x (2 win_h + 3), cI), u8 -> f32. Interior fast path (0 <= ip.x, ip.x + W < cols,
//     the same for y): a = max(a, 0.0001f), dst[j] = prev + t[j] with t[j] = a12*src[j+1] + a22*src[j+1+step], prev = (float)(t[j-1] * s),
//     s = (1. - a) / a in double, and for j = 0 prev = (1 - a)*(b1*src[0] + b2*src[step]). General path: rows and columns replicate-clamped to
//     the w x h image; four float weights a11..a22 added left to right; where both sample columns clamp to the same column (x0 < 0 or
//     x0 >= cols - 1) the two-weight form src*b1 + src2*b2;
//   - normal equations: tgx, tgy float differences of patch neighbours, gxx = tgx*tgx*m etc. in double, five double sums, stop when
//     fabs(det) <= DBL_EPSILON^2, cI2 = (float)(cI + ...) with scale = 1.0 / det, err = the squared float step, stop outside
//     [0, cols) x [0, rows), while (++iter < max_iter && err > eps*eps), revert when |cI - cT| > win;
//   - order of the five sums. `order` = 0: cv's serial raster order. `order` = 1, the kernel's: lane l of 64 adds the window pixels
//     k = l, l + 64, l + 128, ... (k = i * (2 win_w + 1) + j, rows outer) in ascending k into five accumulators that start at +0.0; the 64
//     lane values are then added as a binary tree of neighbours: lanes (0,1), (2,3), ... then pairs of pairs, up to (0..31) + (32..63).
// Self-contained: no header of this repository. Build: g++ -O2 -std=c++17 -fPIC -shared -ffp-contract=off -fno-fast-math.
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

namespace {

int cv_floor(float v) { const int i = (int)v; return i - ((float)i > v); }
int clampi(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }

void table(int win_w, int win_h, int zero_w, int zero_h, float* mask) {
    const int WW = 2 * win_w + 1, WH = 2 * win_h + 1;
    for (int i = 0; i < WH; i++) {
        const float y = (float)(i - win_h) / win_h;
        const float vy = expf(-y * y);
        for (int j = 0; j < WW; j++) {
            const float x = (float)(j - win_w) / win_w;
            mask[i * WW + j] = (float)(vy * expf(-x * x));
        }
    }
    if (zero_w >= 0 && zero_h >= 0 && 2 * zero_w + 1 < WW && 2 * zero_h + 1 < WH)
        for (int i = win_h - zero_h; i <= win_h + zero_h; i++)
            for (int j = win_w - zero_w; j <= win_w + zero_w; j++) mask[i * WW + j] = 0.f;
}

// returns 1 when the interior fast path was taken, 0 for the general one
int patch(const uint8_t* img, int cols, int rows, float cx, float cy, int PW, int PH, float* dst) {
    cx -= (PW - 1) * 0.5f;
    cy -= (PH - 1) * 0.5f;
    const int ipx = cv_floor(cx), ipy = cv_floor(cy);
    if (0 <= ipx && ipx + PW < cols && 0 <= ipy && ipy + PH < rows) {
        float a = cx - ipx;
        const float b = cy - ipy;
        a = a > 0.0001f ? a : 0.0001f;
        const float a12 = a * (1.f - b), a22 = a * b, b1 = 1.f - b, b2 = b;
        const double s = (1. - a) / a;
        for (int i = 0; i < PH; i++) {
            const uint8_t* src = img + (size_t)(ipy + i) * cols + ipx;
            float prev = (1 - a) * (b1 * src[0] + b2 * src[cols]);
            for (int j = 0; j < PW; j++) {
                const float t = a12 * src[j + 1] + a22 * src[j + 1 + cols];
                dst[i * PW + j] = prev + t;
                prev = (float)(t * s);
            }
        }
        return 1;
    }
    const float a = cx - ipx, b = cy - ipy;
    const float a11 = (1.f - a) * (1.f - b), a12 = a * (1.f - b), a21 = (1.f - a) * b, a22 = a * b, b1 = 1.f - b, b2 = b;
    for (int i = 0; i < PH; i++) {
        const uint8_t* r0 = img + (size_t)clampi(ipy + i, 0, rows - 1) * cols;
        const uint8_t* r1 = img + (size_t)clampi(ipy + i + 1, 0, rows - 1) * cols;
        for (int j = 0; j < PW; j++) {
            const int x0 = ipx + j;
            if (x0 < 0 || x0 >= cols - 1) {
                const int xc = x0 < 0 ? 0 : cols - 1;
                dst[i * PW + j] = r0[xc] * b1 + r1[xc] * b2;
            } else
                dst[i * PW + j] = r0[x0] * a11 + r0[x0 + 1] * a12 + r1[x0] * a21 + r1[x0 + 1] * a22;
        }
    }
    return 0;
}

struct Sums { double a, b, c, bb1, bb2; };

inline void term(const float* P, const float* mask, int PW, int WW, int win_w, int win_h, int i, int j, Sums& S) {
    const float* sp = P + (i + 1) * PW + (j + 1);
    const double m = mask[i * WW + j];
    const double tgx = sp[1] - sp[-1];
    const double tgy = sp[PW] - sp[-PW];
    const double gxx = tgx * tgx * m, gxy = tgx * tgy * m, gyy = tgy * tgy * m;
    const double px = j - win_w, py = i - win_h;
    S.a += gxx; S.b += gxy; S.c += gyy;
    S.bb1 += gxx * px + gxy * py;
    S.bb2 += gxy * px + gyy * py;
}

Sums sums(const float* P, const float* mask, int win_w, int win_h, int order) {
    const int WW = 2 * win_w + 1, WH = 2 * win_h + 1, PW = WW + 2;
    if (!order) {
        Sums S{0, 0, 0, 0, 0};
        for (int i = 0; i < WH; i++)
            for (int j = 0; j < WW; j++) term(P, mask, PW, WW, win_w, win_h, i, j, S);
        return S;
    }
    Sums L[64];
    for (int l = 0; l < 64; l++) {
        L[l] = Sums{0, 0, 0, 0, 0};
        for (int k = l; k < WW * WH; k += 64) term(P, mask, PW, WW, win_w, win_h, k / WW, k % WW, L[l]);
    }
    for (int s = 1; s < 64; s *= 2)
        for (int l = 0; l < 64; l += 2 * s) {
            L[l].a += L[l + s].a; L[l].b += L[l + s].b; L[l].c += L[l + s].c; L[l].bb1 += L[l + s].bb1; L[l].bb2 += L[l + s].bb2;
        }
    return L[0];
}

}  // namespace

extern "C" {

void subpix_twin_table(int win_w, int win_h, int zero_w, int zero_h, float* out) { table(win_w, win_h, zero_w, zero_h, out); }

int subpix_twin_patch(const uint8_t* img, int w, int h, float cx, float cy, int win_w, int win_h, float* out) {
    return patch(img, w, h, cx, cy, 2 * win_w + 3, 2 * win_h + 3, out);
}

// xy: n * 2, in/out. out_iters / out_flags may be null. out_fast (may be null): per point, iterations that took the interior path.
void subpix_twin_refine(const uint8_t* img, int w, int h, float* xy, int n, int win_w, int win_h, int zero_w, int zero_h, int max_iter, double eps,
                        int order, uint8_t* out_iters, uint8_t* out_flags, int* out_fast) {
    const int WW = 2 * win_w + 1, WH = 2 * win_h + 1, PW = WW + 2, PH = WH + 2;
    std::vector<float> mask((size_t)WW * WH), P((size_t)PW * PH);
    table(win_w, win_h, zero_w, zero_h, mask.data());
    eps *= eps;
    for (int p = 0; p < n; p++) {
        const float tx = xy[2 * p], ty = xy[2 * p + 1];
        float cx = tx, cy = ty;
        int iter = 0, updates = 0, flags = 0, fast = 0;
        double err = 0;
        bool broke = false;
        do {
            fast += patch(img, w, h, cx, cy, PW, PH, P.data());
            const Sums S = sums(P.data(), mask.data(), win_w, win_h, order);
            const double det = S.a * S.c - S.b * S.b;
            if (fabs(det) <= DBL_EPSILON * DBL_EPSILON) { flags |= 1; broke = true; break; }
            const double scale = 1.0 / det;
            const float nx = (float)(cx + S.c * scale * S.bb1 - S.b * scale * S.bb2);
            const float ny = (float)(cy - S.b * scale * S.bb1 + S.a * scale * S.bb2);
            err = (nx - cx) * (nx - cx) + (ny - cy) * (ny - cy);
            cx = nx; cy = ny;
            updates++;
            if (cx < 0 || cx >= w || cy < 0 || cy >= h) { flags |= 2; broke = true; break; }
        } while (++iter < max_iter && err > eps);
        if (!broke && err > eps) flags |= 4;
        if (fabs(cx - tx) > win_w || fabs(cy - ty) > win_h) { cx = tx; cy = ty; flags |= 8; }
        xy[2 * p] = cx; xy[2 * p + 1] = cy;
        if (out_iters) out_iters[p] = (uint8_t)updates;
        if (out_flags) out_flags[p] = (uint8_t)flags;
        if (out_fast) out_fast[p] = fast;
    }
}

}  // extern "C"
