// TEST INFRASTRUCTURE ONLY. CPU restatement of pmv_detect_gftt_ex (include/pmv_hip.h): cv::goodFeaturesToTrack on a grid cell that is a
// sub-view of a gray frame, with the caller's mask, blockSize, useHarrisDetector and k (gradientSize stays 3).
// PARITY UNPINNED like the rest of the detector [mem: OpenCV 3.4 cornerEigenValsVecs, calcMinEigenVal, calcHarris, goodFeaturesToTrack];
// this file fixes the choices the product follows:
//   - Sobel 3x3, u8 -> f32, the scale 1 / (4 * blockSize * 255) folded into the smoothing kernel [1 2 1] as floats; its border is
//     REFLECT_101 of the PARENT frame (the cell is a non-isolated ROI); cov = (dx^2, dx dy, dy^2) in float;
//   - un-normalised blockSize x blockSize box, anchor blockSize / 2 (offsets -b/2 .. b-1-b/2), REFLECT_101 of the CELL coordinate as often
//     as needed; the sum is a b*b-term DOUBLE sum in raster order (rows outer), cast to float once;
//   - min-eigenvalue: a = s0 * 0.5f, b = s1, c = s2 * 0.5f, (a + c) - sqrt((a - c)^2 + b^2) in float;
//     Harris: a = s0, b = s1, c = s2, (float)(a*c - b*b - k*(a + c)*(a + c)) with C++'s types for that expression;
//   - mask: the maximum for the threshold is taken over the allowed pixels (NaN never wins; no allowed pixel: maximum 0); the 3x3
//     non-maximum test looks at every neighbour; a pixel is a candidate only if its own mask byte is non-zero;
//   - threshold (float)(max * quality) TOZERO, order (value desc, address desc), greedy minDistance, maxCorners: as oracle/orc_detect.cpp.
//   At (3, no Harris, no mask) corners and map are those of orc_gftt_cell, byte for byte (tests/test_gftt_twin.py holds it to that).
// Self-contained: no header of this repository. Build: g++ -O2 -std=c++17 -fPIC -shared -ffp-contract=off -fno-fast-math.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

namespace {

int mirror(int p, int len) {   // BORDER_REFLECT_101, applied as often as needed
    if (len == 1) return 0;
    while (p < 0 || p >= len) p = p < 0 ? -p : 2 * len - 2 - p;
    return p;
}

void response(const uint8_t* img, int W, int H, int cx0, int cy0, int cw, int ch, int bs, int harris, double k, float* out) {
    const double dscale = 1.0 / ((double)(1 << 2) * bs * 255.0);
    const float k1 = (float)(1.0 * dscale), k2 = (float)(2.0 * dscale);
    auto P = [&](int x, int y) -> float { return (float)img[(size_t)mirror(y, H) * W + mirror(x, W)]; };
    std::vector<float> cov((size_t)cw * ch * 3);
    for (int y = 0; y < ch; y++)
        for (int x = 0; x < cw; x++) {
            const int gx = cx0 + x, gy = cy0 + y;
            const float rt = P(gx + 1, gy - 1) - P(gx - 1, gy - 1);
            const float rm = P(gx + 1, gy) - P(gx - 1, gy);
            const float rb = P(gx + 1, gy + 1) - P(gx - 1, gy + 1);
            const float dx = (rt + rb) * k1 + rm * k2;
            float st = k1 * P(gx - 1, gy - 1); st += k2 * P(gx, gy - 1); st += k1 * P(gx + 1, gy - 1);
            float sb = k1 * P(gx - 1, gy + 1); sb += k2 * P(gx, gy + 1); sb += k1 * P(gx + 1, gy + 1);
            const float dy = sb - st;
            float* c = &cov[((size_t)y * cw + x) * 3];
            c[0] = dx * dx; c[1] = dx * dy; c[2] = dy * dy;
        }
    const int an = bs / 2;
    for (int y = 0; y < ch; y++)
        for (int x = 0; x < cw; x++) {
            double s[3] = {0, 0, 0};
            for (int j = -an; j < bs - an; j++)
                for (int i = -an; i < bs - an; i++) {
                    const float* c = &cov[((size_t)mirror(y + j, ch) * cw + mirror(x + i, cw)) * 3];
                    s[0] += c[0]; s[1] += c[1]; s[2] += c[2];
                }
            float e;
            if (harris) {
                const float a = (float)s[0], b = (float)s[1], c = (float)s[2];
                e = (float)(a * c - b * b - k * (a + c) * (a + c));
            } else {
                const float a = (float)s[0] * 0.5f, b = (float)s[1], c = (float)s[2] * 0.5f;
                e = (float)((a + c) - std::sqrt((a - c) * (a - c) + b * b));
            }
            out[(size_t)y * cw + x] = e;
        }
}

}  // namespace

extern "C" {

// the response map alone: cw * ch floats
int gftt_twin_response(const uint8_t* img, int W, int H, int cx0, int cy0, int cw, int ch, int block_size, int use_harris, double k, float* out) {
    if (block_size < 1 || cw < 1 || ch < 1) return -1;
    response(img, W, H, cx0, cy0, cw, ch, block_size, use_harris, k, out);
    return 0;
}

// mask: null, or the FRAME's mask (W x H, mask_stride bytes per row): the cell sees its own rectangle of it. max_corners <= 0: no limit.
// Returns the number of corners (at most out_cap are written; a larger count means out_xy was too small), or -2 if a selected value is
// not above 0 (the invariant the device's selection pass relies on). info (optional, 2 doubles): the masked maximum, and the number of
// records that pass the non-maximum test, their own mask byte and the threshold.
int gftt_twin_cell(const uint8_t* img, int W, int H, int cx0, int cy0, int cw, int ch, int max_corners, double quality, double min_dist, int block_size,
                   int use_harris, double k, const uint8_t* mask, int mask_stride, int* out_xy, int out_cap, float* resp_out, double* info) {
    if (block_size < 1 || cw < 3 || ch < 3) return -1;
    std::vector<float> eig((size_t)cw * ch);
    response(img, W, H, cx0, cy0, cw, ch, block_size, use_harris, k, eig.data());
    if (resp_out) memcpy(resp_out, eig.data(), eig.size() * sizeof(float));
    auto allowed = [&](int x, int y) { return !mask || mask[(size_t)(cy0 + y) * mask_stride + cx0 + x] != 0; };
    bool any = false;
    double maxVal = 0.0;   // no allowed pixel: 0
    for (int y = 0; y < ch; y++)
        for (int x = 0; x < cw; x++) {
            const float v = eig[(size_t)y * cw + x];
            if (!allowed(x, y) || v != v) continue;
            if (!any || (double)v > maxVal) { maxVal = v; any = true; }
        }
    const float thr = (float)(maxVal * quality);
    for (float& v : eig) v = v > thr ? v : 0.f;   // THRESH_TOZERO, on every pixel: the neighbours of the non-maximum test are not masked
    struct Cand { float v; int idx; };
    std::vector<Cand> cand;
    for (int y = 1; y < ch - 1; y++)
        for (int x = 1; x < cw - 1; x++) {
            const float v = eig[(size_t)y * cw + x];
            if (v == 0.f || !allowed(x, y)) continue;
            float m = v;
            for (int j = -1; j <= 1; j++)
                for (int i = -1; i <= 1; i++) m = std::max(m, eig[(size_t)(y + j) * cw + x + i]);
            if (v == m) cand.push_back({v, y * cw + x});
        }
    if (info) { info[0] = maxVal; info[1] = (double)cand.size(); }
    std::sort(cand.begin(), cand.end(), [](const Cand& a, const Cand& b) { return (a.v > b.v) ? true : (a.v < b.v) ? false : (a.idx > b.idx); });
    std::vector<std::pair<int, int>> acc;
    const bool use_dist = min_dist >= 1;
    const double md2 = min_dist * min_dist;
    for (const Cand& c : cand) {
        const int y = c.idx / cw, x = c.idx - y * cw;
        bool good = true;
        if (use_dist)
            for (const auto& a : acc) {
                const float dx = (float)(x - a.first), dy = (float)(y - a.second);
                if (dx * dx + dy * dy < md2) { good = false; break; }
            }
        if (!good) continue;
        if (!(c.v > 0.f)) return -2;
        if ((int)acc.size() < out_cap) { out_xy[2 * acc.size()] = x; out_xy[2 * acc.size() + 1] = y; }
        acc.push_back({x, y});
        if (max_corners > 0 && (int)acc.size() == max_corners) break;
    }
    return (int)acc.size();
}
}
