// TEST INFRASTRUCTURE ONLY. CPU restatement of pmv_lk_track_ex and pmv_lk_track_fb (include/pmv_hip.h): cv::calcOpticalFlowPyrLK with
// OPTFLOW_USE_INITIAL_FLOW and OPTFLOW_LK_GET_MIN_EIGENVALS, and the forward-backward check as a composition of two such calls.
// PARITY UNPINNED like the rest of LK (OpenCV 3.4 video/lkpyramid.cpp from memory); this file fixes the choices the product follows:
//   - window sums are exact integers (int64) rounded once to float32, as oracle/orc_lk.cpp does it;
//   - USE_INITIAL_FLOW: at the top level the search starts at next_xy * 2^-level; next_xy is read, then overwritten;
//   - GET_MIN_EIGENVALS: err = minEig at every level whose template window passes the bounds test, stored before the threshold test;
//     the final residual is not computed. The final bounds test on the tracked position stays, so positions and status are those of the
//     call without the flag (cv skips that test together with the residual);
//   - at flags 0 the three outputs are those of orc_lk_track, byte for byte (tests/test_lkx_twin.py holds it to that).
// Self-contained: no header of this repository, its own pyramid and Scharr. Build: g++ -O2 -std=c++17 -fPIC -shared -ffp-contract=off -fno-fast-math.
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

namespace {

enum { USE_INITIAL_FLOW = 4, GET_MIN_EIGENVALS = 8 };

struct Img {
    int w = 0, h = 0;
    std::vector<uint8_t> px;
    std::vector<int16_t> gx, gy;   // Scharr derivatives of the whole level (filled for template images only)
};

int mirror(int p, int len) {   // BORDER_REFLECT_101, applied as often as needed
    if (len == 1) return 0;
    while (p < 0 || p >= len) p = p < 0 ? -p : 2 * len - 2 - p;
    return p;
}
int pix(const Img& I, int x, int y) { return I.px[(size_t)mirror(y, I.h) * I.w + mirror(x, I.w)]; }

// cv::pyrDown, 8-bit: the separable [1 4 6 4 1] kernel on the mirrored image, (sum + 128) >> 8
Img half_size(const Img& s) {
    Img d;
    d.w = (s.w + 1) / 2; d.h = (s.h + 1) / 2;
    d.px.resize((size_t)d.w * d.h);
    static const int kern[5] = {1, 4, 6, 4, 1};
    for (int y = 0; y < d.h; y++)
        for (int x = 0; x < d.w; x++) {
            int sum = 0;
            for (int i = -2; i <= 2; i++) {
                int row = 0;
                for (int j = -2; j <= 2; j++) row += kern[j + 2] * pix(s, 2 * x + j, 2 * y + i);
                sum += kern[i + 2] * row;
            }
            d.px[(size_t)y * d.w + x] = (uint8_t)((sum + 128) >> 8);
        }
    return d;
}

// buildOpticalFlowPyramid's level rule: after level k is kept, stop if level k + 1 would be <= win in either dimension
std::vector<Img> pyramid(const uint8_t* p, int w, int h, int win, int max_level) {
    std::vector<Img> v(1);
    v[0].w = w; v[0].h = h; v[0].px.assign(p, p + (size_t)w * h);
    for (int lv = 0; lv < max_level; lv++) {
        const Img& top = v.back();
        if ((top.w + 1) / 2 <= win || (top.h + 1) / 2 <= win) break;
        v.push_back(half_size(top));
    }
    return v;
}

// calcSharrDeriv: 3/10/3 smoothing across, central difference along, mirrored inside the image
void scharr(Img& I) {
    I.gx.assign((size_t)I.w * I.h, 0); I.gy.assign((size_t)I.w * I.h, 0);
    for (int y = 0; y < I.h; y++)
        for (int x = 0; x < I.w; x++) {
            int sm[3], df[3];   // per column x-1 .. x+1: vertical smoothing, vertical difference
            for (int k = -1; k <= 1; k++) {
                const int a = pix(I, x + k, y - 1), b = pix(I, x + k, y), c = pix(I, x + k, y + 1);
                sm[k + 1] = 3 * (a + c) + 10 * b;
                df[k + 1] = c - a;
            }
            I.gx[(size_t)y * I.w + x] = (int16_t)(sm[2] - sm[0]);
            I.gy[(size_t)y * I.w + x] = (int16_t)(3 * (df[0] + df[2]) + 10 * df[1]);
        }
}
int grad(const Img& I, const std::vector<int16_t>& g, int x, int y) { return (x < 0 || x >= I.w || y < 0 || y >= I.h) ? 0 : g[(size_t)y * I.w + x]; }

struct Weights { int w00, w01, w10, w11; };
Weights bilinear(float a, float b) {   // 14-bit integer weights, the fourth takes the rounding
    Weights q;
    q.w00 = (int)lrintf((1.f - a) * (1.f - b) * 16384.f);
    q.w01 = (int)lrintf(a * (1.f - b) * 16384.f);
    q.w10 = (int)lrintf((1.f - a) * b * 16384.f);
    q.w11 = 16384 - q.w00 - q.w01 - q.w10;
    return q;
}
int rshift_round(int v, int n) { return (v + (1 << (n - 1))) >> n; }
int sample_px(const Img& I, int x, int y, const Weights& q) {   // 5 fractional bits
    return rshift_round(pix(I, x, y) * q.w00 + pix(I, x + 1, y) * q.w01 + pix(I, x, y + 1) * q.w10 + pix(I, x + 1, y + 1) * q.w11, 9);
}
int sample_grad(const Img& I, const std::vector<int16_t>& g, int x, int y, const Weights& q) {
    return rshift_round(grad(I, g, x, y) * q.w00 + grad(I, g, x + 1, y) * q.w01 + grad(I, g, x, y + 1) * q.w10 + grad(I, g, x + 1, y + 1) * q.w11, 14);
}

struct Params { int win, max_iter; double eps; float min_eig; };
struct Track { float x, y; uint8_t status; float err; };   // x, y: the running position, in the coordinates of the level being processed

bool outside(int ix, int iy, int W, const Img& I) { return ix < -W || ix >= I.w || iy < -W || iy >= I.h; }

// one level of one point; `first` = the top level of the pyramid
void level_step(const Img& I, const Img& J, int level, bool first, const Params& P, int flags, float px0, float py0, float ix0, float iy0, Track& t) {
    const int W = P.win;
    const float half = (W - 1) * 0.5f;
    const float scale = (float)(1. / (1 << level));
    if (first) {
        if (flags & USE_INITIAL_FLOW) { t.x = ix0 * scale; t.y = iy0 * scale; }
        else { t.x = px0 * scale; t.y = py0 * scale; }
    } else { t.x = t.x * 2.f; t.y = t.y * 2.f; }
    const float tx = px0 * scale - half, ty = py0 * scale - half;
    const int itx = (int)floorf(tx), ity = (int)floorf(ty);
    if (outside(itx, ity, W, I)) {
        if (level == 0) { t.status = 0; t.err = 0.f; }
        return;
    }
    const Weights qt = bilinear(tx - itx, ty - ity);
    std::vector<int> tI((size_t)W * W), tX((size_t)W * W), tY((size_t)W * W);
    int64_t sxx = 0, sxy = 0, syy = 0;
    for (int y = 0; y < W; y++)
        for (int x = 0; x < W; x++) {
            const size_t k = (size_t)y * W + x;
            tI[k] = sample_px(I, itx + x, ity + y, qt);
            tX[k] = sample_grad(I, I.gx, itx + x, ity + y, qt);
            tY[k] = sample_grad(I, I.gy, itx + x, ity + y, qt);
            sxx += (int64_t)tX[k] * tX[k]; sxy += (int64_t)tX[k] * tY[k]; syy += (int64_t)tY[k] * tY[k];
        }
    const float S = 1.f / (1 << 20);
    const float A11 = (float)sxx * S, A12 = (float)sxy * S, A22 = (float)syy * S;
    float D = A11 * A22 - A12 * A12;
    const float min_eig = (A22 + A11 - std::sqrt((A11 - A22) * (A11 - A22) + 4.f * A12 * A12)) / (2 * W * W);
    if (flags & GET_MIN_EIGENVALS) t.err = min_eig;
    if (min_eig < P.min_eig || D < FLT_EPSILON) {
        if (level == 0) t.status = 0;
        return;
    }
    D = 1.f / D;
    float sx = t.x - half, sy = t.y - half;   // the search window's origin
    float last_dx = 0.f, last_dy = 0.f;
    const double eps2 = P.eps * P.eps;
    for (int it = 0; it < P.max_iter; it++) {
        const int isx = (int)floorf(sx), isy = (int)floorf(sy);
        if (outside(isx, isy, W, J)) {
            if (level == 0) t.status = 0;
            break;
        }
        const Weights q = bilinear(sx - isx, sy - isy);
        int64_t b1 = 0, b2 = 0;
        for (int y = 0; y < W; y++)
            for (int x = 0; x < W; x++) {
                const size_t k = (size_t)y * W + x;
                const int d = sample_px(J, isx + x, isy + y, q) - tI[k];
                b1 += (int64_t)d * tX[k]; b2 += (int64_t)d * tY[k];
            }
        const float fb1 = (float)b1 * S, fb2 = (float)b2 * S;
        const float dx = (A12 * fb2 - A22 * fb1) * D, dy = (A12 * fb1 - A11 * fb2) * D;
        sx += dx; sy += dy;
        t.x = sx + half; t.y = sy + half;
        if ((double)dx * dx + (double)dy * dy <= eps2) break;
        if (it > 0 && std::abs(dx + last_dx) < 0.01 && std::abs(dy + last_dy) < 0.01) {
            t.x -= dx * 0.5f; t.y -= dy * 0.5f;
            break;
        }
        last_dx = dx; last_dy = dy;
    }
    if (t.status && level == 0) {
        const float fx = t.x - half, fy = t.y - half;
        const int ifx = (int)floorf(fx), ify = (int)floorf(fy);
        if (outside(ifx, ify, W, J)) { t.status = 0; return; }
        if (flags & GET_MIN_EIGENVALS) return;
        const Weights q = bilinear(fx - ifx, fy - ify);
        int64_t e = 0;
        for (int y = 0; y < W; y++)
            for (int x = 0; x < W; x++) {
                const int d = sample_px(J, ifx + x, ify + y, q) - tI[(size_t)y * W + x];
                e += d < 0 ? -d : d;
            }
        t.err = (float)e * (1.f / (32 * W * W));
    }
}

// next_xy in/out; A's levels carry their Scharr maps
void track_all(const std::vector<Img>& A, const std::vector<Img>& B, const float* prev_xy, int n, const Params& P, int flags, float* next_xy, uint8_t* status, float* err) {
    const int top = (int)A.size() - 1;
    for (int i = 0; i < n; i++) {
        Track t{0.f, 0.f, 1, 0.f};
        for (int lv = top; lv >= 0; lv--) level_step(A[lv], B[lv], lv, lv == top, P, flags, prev_xy[2 * i], prev_xy[2 * i + 1], next_xy[2 * i], next_xy[2 * i + 1], t);
        next_xy[2 * i] = t.x; next_xy[2 * i + 1] = t.y; status[i] = t.status; err[i] = t.err;
    }
}

}  // namespace

extern "C" {

// returns the top level's index (levels built - 1), -1 on a bad argument
int lkx_track(const uint8_t* prev, const uint8_t* next, int w, int h, const float* prev_xy, int n, int win, int max_level, int max_iter, double eps, float min_eig,
              int flags, float* next_xy, uint8_t* status, float* err) {
    if (flags & ~(USE_INITIAL_FLOW | GET_MIN_EIGENVALS)) return -1;
    std::vector<Img> A = pyramid(prev, w, h, win, max_level), B = pyramid(next, w, h, win, max_level);
    for (Img& I : A) scharr(I);
    const Params P{win, max_iter, eps, min_eig};
    track_all(A, B, prev_xy, n, P, flags, next_xy, status, err);
    return (int)A.size() - 1;
}

// the composition pmv_lk_track_fb is defined as
int lkx_track_fb(const uint8_t* prev, const uint8_t* next, int w, int h, const float* prev_xy, int n, int win, int max_level, int max_iter, double eps, float min_eig,
                 int flags, float* next_xy, uint8_t* status, float* err, float* back_xy, uint8_t* back_status, float* back_err) {
    if (flags & ~(USE_INITIAL_FLOW | GET_MIN_EIGENVALS)) return -1;
    std::vector<Img> A = pyramid(prev, w, h, win, max_level), B = pyramid(next, w, h, win, max_level);
    for (Img& I : A) scharr(I);
    for (Img& I : B) scharr(I);
    const Params P{win, max_iter, eps, min_eig};
    track_all(A, B, prev_xy, n, P, flags, next_xy, status, err);
    for (int i = 0; i < n; i++) {
        back_xy[2 * i] = next_xy[2 * i]; back_xy[2 * i + 1] = next_xy[2 * i + 1]; back_status[i] = 0; back_err[i] = 0.f;
        if (!status[i]) continue;
        float b[2] = {prev_xy[2 * i], prev_xy[2 * i + 1]};   // initial flow = where the track came from
        track_all(B, A, next_xy + 2 * i, 1, P, USE_INITIAL_FLOW | (flags & GET_MIN_EIGENVALS), b, back_status + i, back_err + i);
        back_xy[2 * i] = b[0]; back_xy[2 * i + 1] = b[1];
    }
    return (int)A.size() - 1;
}
}
