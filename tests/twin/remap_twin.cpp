// CPU twin of pmv_frames_remap (include/pmv_hip.h): cv::remap(src, dst, map_x, map_y, INTER_LINEAR, BORDER_CONSTANT, border) for a
// CV_8UC1 image and a pair of CV_32FC1 maps of the image's own size, restated serially: the conversion of the float maps into cv's
// fixed-point form (INTER_BITS 5), then the bilinear blend in integers. It fixes the bits the device kernel is held to. Compiled with
// -ffp-contract=off (the one float product, map * 32.0f, is exact anyway).
// Beside the image it reports what the maps reach: how many destination pixels have all four taps inside the image, all outside, or some of
// each (and for those, which sides of the image the outside taps lie beyond), and how often every (fy, fx) pair occurs.
#include <climits>
#include <cmath>
#include <cstdint>

namespace {

// cvRound(float) as SSE's cvtss2si gives it: to nearest, ties to even; NaN and values that do not fit an int32 give INT_MIN
int cv_round(float v) {
    if (std::isnan(v) || v >= 2147483648.0f || v < -2147483648.0f) return INT_MIN;
    return (int)std::lrintf(v);
}

short saturate_s16(int v) { return (short)(v < SHRT_MIN ? SHRT_MIN : v > SHRT_MAX ? SHRT_MAX : v); }

}  // namespace

// stats: 8 + 1024 ints. [0] pixels with all four taps inside, [1] all outside, [2] mixed; of the mixed ones, [3] with a tap left of the
// image, [4] right of it, [5] above it, [6] below it (a pixel at a corner counts for both of its sides); [7] unused; [8 + 32 fy + fx] the
// number of pixels with that pair of fractions.
extern "C" int remap_twin_apply(const uint8_t* src, int w, int h, const float* map_x, const float* map_y, int border, uint8_t* dst, int32_t* stats) {
    if (!src || !map_x || !map_y || !dst || !stats || w < 1 || h < 1 || border < 0 || border > 255) return -1;
    for (int i = 0; i < 8 + 1024; i++) stats[i] = 0;
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
            const int sx = cv_round(map_x[(long)y * w + x] * 32.0f);
            const int sy = cv_round(map_y[(long)y * w + x] * 32.0f);
            const int ix = saturate_s16(sx >> 5), iy = saturate_s16(sy >> 5);   // arithmetic shifts
            const int fx = sx & 31, fy = sy & 31;
            stats[8 + 32 * fy + fx]++;
            int tap[2][2], n_in = 0;
            bool left = false, right = false, above = false, below = false;
            for (int dy = 0; dy < 2; dy++)
                for (int dx = 0; dx < 2; dx++) {
                    const int tx = ix + dx, ty = iy + dy;
                    const bool in = tx >= 0 && tx < w && ty >= 0 && ty < h;
                    tap[dy][dx] = in ? src[(long)ty * w + tx] : border;
                    n_in += in;
                    left |= tx < 0; right |= tx >= w; above |= ty < 0; below |= ty >= h;
                }
            if (n_in == 4) stats[0]++;
            else if (n_in == 0) stats[1]++;
            else { stats[2]++; stats[3] += left; stats[4] += right; stats[5] += above; stats[6] += below; }
            const int sum = (32 - fy) * (32 - fx) * tap[0][0] + (32 - fy) * fx * tap[0][1] + fy * (32 - fx) * tap[1][0] + fy * fx * tap[1][1];
            dst[(long)y * w + x] = (uint8_t)((sum + 512) >> 10);
        }
    return 0;
}
