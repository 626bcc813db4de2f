// CPU twin of pmv_frames_clahe: cv::CLAHE::apply for 8-bit images, restated from OpenCV 3.4 clahe.cpp [mem], serially and in cv's own
// order of statements. It FIXES the arithmetic of the contract in include/pmv_hip.h: the GPU tests compare the slots with this file's
// output byte for byte. Build: g++ -O2 -ffp-contract=off -fno-fast-math (tests/clahe_common.py).
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

namespace {

int reflect101(int p, int len) {
    if (len == 1) return 0;
    while (p < 0 || p >= len) p = p < 0 ? -p : 2 * len - 2 - p;
    return p;
}
uint8_t sat_u8(float v) {   // saturate_cast<uchar>(float): cvRound = round half to even (the default rounding mode), then the clamp
    const int q = (int)std::nearbyintf(v);
    return (uint8_t)(q < 0 ? 0 : q > 255 ? 255 : q);
}

}  // namespace

// stats (int[8 + 257], may be null): [0] columns added on the right, [1] rows added at the bottom, [2] tile width, [3] tile height, [4] cl,
// [5] tiles with clipped > 0, [6] tiles with residual > 0, [7] unused, [8 + s] = 1 when the redistribution ran with step s (1..256)
extern "C" int clahe_twin_apply(const uint8_t* img, int w, int h, double clip_limit, int tiles_x, int tiles_y, uint8_t* out, int* stats) {
    if (!img || !out || w < 1 || h < 1 || tiles_x < 1 || tiles_y < 1 || !(clip_limit >= 0.0)) return -1;
    const int hist_size = 256;
    // the image CLAHE_CalcLut_Body sees: the source, or copyMakeBorder(src, 0, ty - h % ty, 0, tx - w % tx, BORDER_REFLECT_101)
    int right = 0, bottom = 0;
    if (w % tiles_x != 0 || h % tiles_y != 0) {
        right = tiles_x - w % tiles_x;
        bottom = tiles_y - h % tiles_y;
    }
    const int ew = w + right, eh = h + bottom;
    std::vector<uint8_t> ext((size_t)ew * eh);
    for (int y = 0; y < eh; y++)
        for (int x = 0; x < ew; x++) ext[(size_t)y * ew + x] = img[(size_t)reflect101(y, h) * w + reflect101(x, w)];
    const int tile_w = ew / tiles_x, tile_h = eh / tiles_y;
    const int area = tile_w * tile_h;
    const float lut_scale = static_cast<float>(hist_size - 1) / area;
    int cl = 0;
    if (clip_limit > 0.0) {
        double c = clip_limit * area / hist_size;
        if (c > (double)area) c = (double)area;   // (no bin exceeds area: the same result, and the cast cannot overflow)
        cl = static_cast<int>(c);
        cl = cl > 1 ? cl : 1;
    }
    if (stats) {
        memset(stats, 0, sizeof(int) * (8 + 257));
        stats[0] = right; stats[1] = bottom; stats[2] = tile_w; stats[3] = tile_h; stats[4] = cl;
    }
    std::vector<uint8_t> lut((size_t)tiles_x * tiles_y * hist_size);
    for (int k = 0; k < tiles_x * tiles_y; k++) {
        const int ty = k / tiles_x, tx = k % tiles_x;
        int hist[256];
        memset(hist, 0, sizeof(hist));
        for (int y = 0; y < tile_h; y++) {
            const uint8_t* row = &ext[(size_t)(ty * tile_h + y) * ew + (size_t)tx * tile_w];
            for (int x = 0; x < tile_w; x++) hist[row[x]]++;
        }
        if (cl > 0) {
            int clipped = 0;
            for (int i = 0; i < hist_size; i++)
                if (hist[i] > cl) { clipped += hist[i] - cl; hist[i] = cl; }
            const int batch = clipped / hist_size;
            int residual = clipped - batch * hist_size;
            for (int i = 0; i < hist_size; i++) hist[i] += batch;
            if (stats && clipped > 0) stats[5]++;
            if (residual != 0) {
                const int step = (hist_size / residual) > 1 ? hist_size / residual : 1;
                if (stats) { stats[6]++; stats[8 + step] = 1; }
                for (int i = 0; i < hist_size && residual > 0; i += step, residual--) hist[i]++;
            }
        }
        int sum = 0;
        for (int i = 0; i < hist_size; i++) {
            sum += hist[i];
            lut[(size_t)k * hist_size + i] = sat_u8(sum * lut_scale);
        }
    }
    // CLAHE_Interpolation_Body on the w x h source
    const float inv_tw = 1.0f / tile_w, inv_th = 1.0f / tile_h;
    for (int y = 0; y < h; y++) {
        const float tyf = y * inv_th - 0.5f;
        int ty1 = (int)std::floor(tyf);
        int ty2 = ty1 + 1;
        const float ya = tyf - ty1, ya1 = 1.0f - ya;
        ty1 = ty1 > 0 ? ty1 : 0;
        ty2 = ty2 < tiles_y - 1 ? ty2 : tiles_y - 1;
        const uint8_t* plane1 = &lut[(size_t)ty1 * tiles_x * hist_size];
        const uint8_t* plane2 = &lut[(size_t)ty2 * tiles_x * hist_size];
        for (int x = 0; x < w; x++) {
            const float txf = x * inv_tw - 0.5f;
            int tx1 = (int)std::floor(txf);
            int tx2 = tx1 + 1;
            const float xa = txf - tx1, xa1 = 1.0f - xa;
            tx1 = tx1 > 0 ? tx1 : 0;
            tx2 = tx2 < tiles_x - 1 ? tx2 : tiles_x - 1;
            const int v = img[(size_t)y * w + x];
            const int ind1 = tx1 * hist_size + v, ind2 = tx2 * hist_size + v;
            const float res = (plane1[ind1] * xa1 + plane1[ind2] * xa) * ya1 + (plane2[ind1] * xa1 + plane2[ind2] * xa) * ya;
            out[(size_t)y * w + x] = sat_u8(res);
        }
    }
    return 0;
}
