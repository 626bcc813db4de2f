// TEST INFRASTRUCTURE ONLY. CPU restatement of the mask half of pmv_detect_gftt_refill (include/pmv_hip.h): FeatureTracker::setMask of a
// VINS-style KLT loop - sort the tracks, walk them, keep a track whose mask byte is still 255, clear a filled cv::circle around it.
// PARITY UNPINNED [mem: OpenCV 3.4 drawing.cpp, Circle() with fill, LINE_8, shift 0; cvRound; Point2f -> Point]; this file fixes the
// choices the product follows:
//   - position: (cvRound(x), cvRound(y)), round half to even (lrintf in the default rounding mode);
//   - order: priority descending, then index ascending - one of the orders std::sort may give setMask among equal priorities; a null
//     priority list = all equal;
//   - walk: keep track i iff mask(y, x) == 255 at its turn; then circle(mask, (x, y), radius, 0, -1);
//   - circle: the Circle() loop below, literally: err / plus / minus, `while (dx >= dy)`, two span pairs per step, the clipped branch;
//   - start: every byte 255, or the base mask's bytes.
// The corner half of the call is gftt_twin_cell (gftt_twin.cpp) with this file's mask. Self-contained: no header of this repository.
// Build: g++ -O2 -std=c++17 -fPIC -shared -ffp-contract=off -fno-fast-math.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <numeric>
#include <vector>

namespace {

void hline(uint8_t* row, int xl, int xr, uint8_t color) {   // ICV_HLINE: both ends included
    for (int x = xl; x <= xr; x++) row[x] = color;
}

// Circle(img, center, radius, color, fill = 1) of drawing.cpp on a one-channel 8-bit image of `step` bytes per row
void circle_filled(uint8_t* ptr, int width, int height, size_t step, int cx, int cy, int radius, uint8_t color) {
    int err = 0, dx = radius, dy = 0, plus = 1, minus = (radius << 1) - 1;
    const int inside = cx >= radius && cx < width - radius && cy >= radius && cy < height - radius;
    while (dx >= dy) {
        int mask;
        int y11 = cy - dy, y12 = cy + dy, y21 = cy - dx, y22 = cy + dx;
        int x11 = cx - dx, x12 = cx + dx, x21 = cx - dy, x22 = cx + dy;
        if (inside) {
            uint8_t* tptr0 = ptr + y11 * step;
            uint8_t* tptr1 = ptr + y12 * step;
            hline(tptr0, x11, x12, color);
            hline(tptr1, x11, x12, color);
            tptr0 = ptr + y21 * step;
            tptr1 = ptr + y22 * step;
            hline(tptr0, x21, x22, color);
            hline(tptr1, x21, x22, color);
        } else if (x11 < width && x12 >= 0 && y21 < height && y22 >= 0) {
            x11 = std::max(x11, 0);
            x12 = std::min(x12, width - 1);
            if ((unsigned)y11 < (unsigned)height) hline(ptr + y11 * step, x11, x12, color);
            if ((unsigned)y12 < (unsigned)height) hline(ptr + y12 * step, x11, x12, color);
            if (x21 < width && x22 >= 0) {
                x21 = std::max(x21, 0);
                x22 = std::min(x22, width - 1);
                if ((unsigned)y21 < (unsigned)height) hline(ptr + y21 * step, x21, x22, color);
                if ((unsigned)y22 < (unsigned)height) hline(ptr + y22 * step, x21, x22, color);
            }
        }
        dy++;
        err += plus;
        plus += 2;
        mask = (err <= 0) - 1;
        err -= minus & mask;
        dx += mask;
        minus -= mask & 2;
    }
}

}  // namespace

extern "C" {

// diagnostic for the tests: the literal painting on the caller's image
void refill_twin_circle(uint8_t* img, int w, int h, int step, int cx, int cy, int radius, int color) {
    circle_filled(img, w, h, (size_t)step, cx, cy, radius, (uint8_t)color);
}

// out[d], d = 0 .. radius: the widest span the loop paints at row offset d, as a half width (the table the product's kernels test against)
void refill_twin_halfwidths(int radius, int* out) {
    for (int d = 0; d <= radius; d++) out[d] = -1;
    int err = 0, dx = radius, dy = 0, plus = 1, minus = (radius << 1) - 1;
    while (dx >= dy) {
        out[dy] = std::max(out[dy], dx);
        out[dx] = std::max(out[dx], dy);
        dy++;
        err += plus;
        plus += 2;
        const int mask = (err <= 0) - 1;
        err -= minus & mask;
        dx += mask;
        minus -= mask & 2;
    }
}

// the rounded positions: (n, 2) ints
void refill_twin_positions(const float* xy, int n, int* out) {
    for (int i = 0; i < 2 * n; i++) out[i] = (int)lrintf(xy[i]);
}

// setMask. out_keep: n bytes; out_mask: w * h bytes, tight. base: null or a w x h view of base_stride bytes per row.
// Returns the number of kept tracks, or -1 - (index of the first track whose rounded position lies outside the frame), nothing written.
int refill_twin_mask(int w, int h, const float* xy, const int* prio_or_null, int n, int radius, const uint8_t* base, int base_stride, uint8_t* out_keep,
                     uint8_t* out_mask) {
    std::vector<int> px(n), py(n);
    for (int i = 0; i < n; i++) {
        px[i] = (int)lrintf(xy[2 * i]); py[i] = (int)lrintf(xy[2 * i + 1]);
        if (px[i] < 0 || px[i] >= w || py[i] < 0 || py[i] >= h) return -1 - i;
    }
    for (int y = 0; y < h; y++) {
        if (base) memcpy(out_mask + (size_t)y * w, base + (size_t)y * base_stride, (size_t)w);
        else memset(out_mask + (size_t)y * w, 255, (size_t)w);
    }
    std::vector<int> order(n);
    std::iota(order.begin(), order.end(), 0);
    if (prio_or_null)
        std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return prio_or_null[a] > prio_or_null[b]; });
    int kept = 0;
    for (int o = 0; o < n; o++) {
        const int i = order[o];
        out_keep[i] = 0;
        if (out_mask[(size_t)py[i] * w + px[i]] == 255) {
            out_keep[i] = 1;
            kept++;
            circle_filled(out_mask, w, h, (size_t)w, px[i], py[i], radius, 0);
        }
    }
    return kept;
}

}  // extern "C"
