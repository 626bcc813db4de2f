// pmv_frames_remap / pmv_batch_frame_upload_remap: cv::remap(INTER_LINEAR, BORDER_CONSTANT) on level 0 of frame slots (contract:
// include/pmv_hip.h; the arithmetic, statement by statement: tests/twin/remap_twin.cpp), and the two host helpers behind the maps.
// A gather cannot run in place, so k_remap reads the raw INTERIOR of level 0 (never the slot's own border: a staged slot has none yet) and
// writes a tight w x h frame into a scratch area; the existing list-form k_pad_level0 launch, with that frame as its source, then writes level
// 0 and its REFLECT_101 frame, and the existing k_pyrdown launches build the levels above. A record per frame (RemapRec, pmv_device.h)
// names the slot, the frame's entry of a geometry table, its packed map, the border value and where its frame starts in the scratch, so one
// launch serves frames of any sizes and maps.
// The packed map (remap_pack, once per camera) is two planes over the LINEAR pixel index p = y w + x, each padded to a multiple of four
// entries: a dword (ix & 0xffff) | iy << 16 and a halfword fx | fy << 5 - 6 bytes per pixel. The tight destination is linear in p as well, so
// a thread takes p = 4 t .. 4 t + 3: one 16-byte and one 8-byte map load, both aligned and coalesced, and one aligned dword store, whatever w
// is; with w % 4 != 0 its four pixels may sit on two rows, which only the row / column split below has to know. The 2 x 2 taps are plain
// cached byte loads. Vector loads and stores only, no LDS.
// pmv_set_frame_preproc (the feeder, ingest_batch.hip) runs the same gather as k_remap_src: its taps come from the round's landing buffer,
// not from a slot, so it writes level 0 of the slot directly and needs neither the scratch frame nor the list-form level-0 pass.
#include "pmv_device.h"
#include "pmv_lift.h"
#include "pmv_prof.h"
#include <climits>
#include <cmath>

namespace pmv {

namespace {

constexpr int RM_T = 256, RM_PX = 4;           // threads per workgroup, pixels per thread

__global__ __launch_bounds__(RM_T) void k_remap(const uint8_t* __restrict__ slots, const PyrLayout* __restrict__ geom, const RemapRec* __restrict__ recs,
                                                 uint8_t* __restrict__ scratch) {
    const RemapRec r = recs[blockIdx.y];
    GeomEntry& L = geom_entry(geom, r.geom);
    const int w = L.w[0], h = L.h[0], stride = L.stride[0];
    const unsigned npix = (unsigned)w * (unsigned)h;
    const unsigned p0 = (blockIdx.x * (unsigned)RM_T + threadIdx.x) * RM_PX;
    if (p0 >= npix) return;                    // (the grid is sized for the largest frame of the list; no barrier in this kernel)
    const uint8_t* img = slots + (size_t)__builtin_amdgcn_readfirstlane(r.slot) * L.slot_bytes + L.gray_off;
    const unsigned n4 = (npix + 3u) & ~3u;     // entries per plane of the packed map
    const uint32_t* plane_xy = r.map;
    const uint16_t* plane_f = (const uint16_t*)(r.map + n4);
    const uint4 cq = *(const uint4*)(plane_xy + p0);   // p0 is a multiple of 4 and the planes are padded to one: inside the map
    const uint2 fq = *(const uint2*)(plane_f + p0);
    const uint32_t c[RM_PX] = {cq.x, cq.y, cq.z, cq.w};
    const uint32_t f[RM_PX] = {fq.x & 0xffffu, fq.x >> 16, fq.y & 0xffffu, fq.y >> 16};
    const int bv = r.border;
    uint32_t out = 0;
#pragma unroll
    for (int k = 0; k < RM_PX; k++) {
        if (p0 + k >= npix) break;             // (the padding entries of the last dword)
        const int ix = (int)(short)(c[k] & 0xffffu), iy = (int)(short)(c[k] >> 16);
        const int fx = (int)(f[k] & 31u), fy = (int)((f[k] >> 5) & 31u);
        // a tap is read only where it lies inside the w x h interior; everywhere else it is the border value
        const bool x0 = (unsigned)ix < (unsigned)w, x1 = (unsigned)(ix + 1) < (unsigned)w;
        const bool y0 = (unsigned)iy < (unsigned)h, y1 = (unsigned)(iy + 1) < (unsigned)h;
        const uint8_t* t = img + (ptrdiff_t)iy * (ptrdiff_t)stride + (ptrdiff_t)ix;
        const int t00 = (x0 && y0) ? (int)t[0] : bv;
        const int t01 = (x1 && y0) ? (int)t[1] : bv;
        const int t10 = (x0 && y1) ? (int)t[stride] : bv;
        const int t11 = (x1 && y1) ? (int)t[stride + 1] : bv;
        const int d = ((32 - fy) * (32 - fx) * t00 + (32 - fy) * fx * t01 + fy * (32 - fx) * t10 + fy * fx * t11 + 512) >> 10;
        out |= (uint32_t)d << (8 * k);
    }
    uint8_t* dst = scratch + r.dst_off + p0;   // dst_off is a multiple of 256: a dword-aligned address
    if (p0 + RM_PX <= npix) *(uint32_t*)dst = out;
    else for (unsigned k = 0; p0 + k < npix; k++) dst[k] = (uint8_t)(out >> (8 * k));   // byte tail of a frame with w h % 4 != 0
}

// The feeder's form: k_remap's arithmetic, statement for statement, on a tight source frame (gray bytes, or BGR triples converted per tap)
// with the interior of level 0 as the destination. The thread / pixel assignment stays linear in p, so the map loads stay one aligned 16-byte
// and one aligned 8-byte load per four pixels whatever w is. The destination is NOT linear in p any more (row pitch stride[0] >= w + 128), so
// the stores split: a thread whose four pixels lie in one row at a column that is a multiple of 4 (every thread when w % 4 == 0; with an
// odd w the rows y with y w % 4 == 0, one in four) makes ONE aligned dword store - interior rows start 64-byte aligned; every other thread,
// including the one that straddles a row end and the tail of a frame with w h % 4 != 0, makes up to four byte stores.
template <bool BGR>
__device__ __forceinline__ int remap_src_tap(const uint8_t* __restrict__ src, ptrdiff_t o) {
    if (!BGR) return (int)src[o];
    const uint8_t* q = src + 3 * o;            // cvtColor(BGR2GRAY), as k_pad_level0_bgr stores it
    return ((int)q[0] * 1868 + (int)q[1] * 9617 + (int)q[2] * 4899 + 8192) >> 14;
}
template <bool BGR>
__device__ __forceinline__ void remap_src_body(uint8_t* __restrict__ slots, GeomEntry& L, const RemapSrcRec& r) {
    const int w = L.w[0], h = L.h[0], stride = L.stride[0];
    const unsigned npix = (unsigned)w * (unsigned)h;
    const unsigned p0 = (blockIdx.x * (unsigned)RM_T + threadIdx.x) * RM_PX;
    if (p0 >= npix) return;                    // (the grid is sized for the largest frame of the list; no barrier in this kernel)
    const uint8_t* __restrict__ src = r.src;
    const unsigned n4 = (npix + 3u) & ~3u;     // entries per plane of the packed map
    const uint32_t* plane_xy = r.map;
    const uint16_t* plane_f = (const uint16_t*)(r.map + n4);
    const uint4 cq = *(const uint4*)(plane_xy + p0);   // p0 is a multiple of 4 and the planes are padded to one: inside the map
    const uint2 fq = *(const uint2*)(plane_f + p0);
    const uint32_t c[RM_PX] = {cq.x, cq.y, cq.z, cq.w};
    const uint32_t f[RM_PX] = {fq.x & 0xffffu, fq.x >> 16, fq.y & 0xffffu, fq.y >> 16};
    const int bv = r.border;
    uint32_t out = 0;
#pragma unroll
    for (int k = 0; k < RM_PX; k++) {
        if (p0 + k >= npix) break;             // (the padding entries of the last dword)
        const int ix = (int)(short)(c[k] & 0xffffu), iy = (int)(short)(c[k] >> 16);
        const int fx = (int)(f[k] & 31u), fy = (int)((f[k] >> 5) & 31u);
        // a tap is read only where it lies inside the w x h frame; everywhere else it is the border value
        const bool x0 = (unsigned)ix < (unsigned)w, x1 = (unsigned)(ix + 1) < (unsigned)w;
        const bool y0 = (unsigned)iy < (unsigned)h, y1 = (unsigned)(iy + 1) < (unsigned)h;
        const ptrdiff_t o = (ptrdiff_t)iy * (ptrdiff_t)w + (ptrdiff_t)ix;   // the source is tight: its row pitch is w pixels
        const int t00 = (x0 && y0) ? remap_src_tap<BGR>(src, o) : bv;
        const int t01 = (x1 && y0) ? remap_src_tap<BGR>(src, o + 1) : bv;
        const int t10 = (x0 && y1) ? remap_src_tap<BGR>(src, o + w) : bv;
        const int t11 = (x1 && y1) ? remap_src_tap<BGR>(src, o + w + 1) : bv;
        const int d = ((32 - fy) * (32 - fx) * t00 + (32 - fy) * fx * t01 + fy * (32 - fx) * t10 + fy * fx * t11 + 512) >> 10;
        out |= (uint32_t)d << (8 * k);
    }
    uint8_t* img = slots + (size_t)__builtin_amdgcn_readfirstlane(r.slot) * L.slot_bytes + L.gray_off;
    const unsigned y = p0 / (unsigned)w, x = p0 - y * (unsigned)w;
    if (p0 + RM_PX <= npix && x + RM_PX <= (unsigned)w && (x & 3u) == 0u) {
        *(uint32_t*)(img + (size_t)y * (size_t)stride + x) = out;
    } else {
        for (unsigned k = 0; k < RM_PX && p0 + k < npix; k++) {
            unsigned xk = x + k, yk = y;
            if (xk >= (unsigned)w) { xk -= (unsigned)w; yk++; }   // (w >= 40: four pixels cross one row end at most)
            img[(size_t)yk * (size_t)stride + xk] = (uint8_t)(out >> (8 * k));
        }
    }
}
__global__ __launch_bounds__(RM_T) void k_remap_src(uint8_t* __restrict__ slots, const PyrLayout* __restrict__ geom, const RemapSrcRec* __restrict__ recs) {
    const RemapSrcRec r = recs[blockIdx.y];
    GeomEntry& L = geom_entry(geom, r.geom);
    if (__builtin_amdgcn_readfirstlane(r.bgr)) remap_src_body<true>(slots, L, r);   // (the record is the workgroup's: a uniform branch)
    else remap_src_body<false>(slots, L, r);
}

// cvRound of a float as cvtss2si does it: half to even, and the "integer indefinite" INT_MIN for a NaN or a value beyond int32
inline int cv_round_f32(float v) {
    if (!(v >= -2147483648.0f && v < 2147483648.0f)) return INT_MIN;
    return (int)nearbyintf(v);                 // (the default rounding mode: to nearest, ties to even)
}
inline int sat_s16(int v) { return v < -32768 ? -32768 : v > 32767 ? 32767 : v; }

}  // namespace

size_t remap_map_bytes(int w, int h) { return ((((size_t)w * (size_t)h) + 3) & ~(size_t)3) * 6; }

void remap_pack(const float* map_x, const float* map_y, int w, int h, uint8_t* out) {
    const size_t n = (size_t)w * (size_t)h, n4 = (n + 3) & ~(size_t)3;
    uint32_t* a = (uint32_t*)out;
    uint16_t* b = (uint16_t*)(a + n4);
    for (size_t p = 0; p < n4; p++) {
        if (p >= n) { a[p] = 0; b[p] = 0; continue; }
        const int sx = cv_round_f32(map_x[p] * 32.0f), sy = cv_round_f32(map_y[p] * 32.0f);
        const int ix = sat_s16(sx >> 5), iy = sat_s16(sy >> 5);   // (arithmetic shifts: floor)
        a[p] = ((uint32_t)ix & 0xffffu) | ((uint32_t)iy << 16);
        b[p] = (uint16_t)((sx & 31) | ((sy & 31) << 5));
    }
}

// (newK R)^-1 by adjugate and determinant, for the two map builders; false when newK R is singular
static bool map_ray_matrix(const double* K, const double* R, const double* newK, double* iR) {
    const double I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    const double* Rm = R ? R : I;
    const double* N = newK ? newK : K;
    double A[9];
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) A[3 * r + c] = N[3 * r] * Rm[c] + N[3 * r + 1] * Rm[3 + c] + N[3 * r + 2] * Rm[6 + c];
    // the inverse by adjugate and determinant
    const double c00 = A[4] * A[8] - A[5] * A[7], c01 = A[5] * A[6] - A[3] * A[8], c02 = A[3] * A[7] - A[4] * A[6];
    const double det = A[0] * c00 + A[1] * c01 + A[2] * c02;
    if (!(std::fabs(det) > 0.0) || !std::isfinite(det)) return false;
    const double inv[9] = {c00 / det, (A[2] * A[7] - A[1] * A[8]) / det, (A[1] * A[5] - A[2] * A[4]) / det,
                           c01 / det, (A[0] * A[8] - A[2] * A[6]) / det, (A[2] * A[3] - A[0] * A[5]) / det,
                           c02 / det, (A[1] * A[6] - A[0] * A[7]) / det, (A[0] * A[4] - A[1] * A[3]) / det};
    for (int k = 0; k < 9; k++) iR[k] = inv[k];
    return true;
}

bool undistort_map(const double* K, const double* dist, const double* R, const double* newK, int w, int h, float* map_x, float* map_y) {
    double iR[9];
    if (!map_ray_matrix(K, R, newK, iR)) return false;
    const double fx = K[0], fy = K[4], cx = K[2], cy = K[5];
    const double k1 = dist[0], k2 = dist[1], p1 = dist[2], p2 = dist[3], k3 = dist[4], k4 = dist[5], k5 = dist[6], k6 = dist[7];
    for (int i = 0; i < h; i++)
        for (int j = 0; j < w; j++) {
            const double X = iR[0] * j + iR[1] * i + iR[2], Y = iR[3] * j + iR[4] * i + iR[5], W = iR[6] * j + iR[7] * i + iR[8];
            const double x = X / W, y = Y / W;
            const double x2 = x * x, y2 = y * y, r2 = x2 + y2, xy2 = 2 * x * y;
            const double kr = (1 + ((k3 * r2 + k2) * r2 + k1) * r2) / (1 + ((k6 * r2 + k5) * r2 + k4) * r2);
            const double xd = x * kr + p1 * xy2 + p2 * (r2 + 2 * x2);
            const double yd = y * kr + p1 * (r2 + 2 * y2) + p2 * xy2;
            map_x[(size_t)i * w + j] = (float)(fx * xd + cx);
            map_y[(size_t)i * w + j] = (float)(fy * yd + cy);
        }
    return true;
}

// cv::fisheye::initUndistortRectifyMap: the ray of every pixel as above, then fisheye_project (pmv_lift.h, the one statement of the forward
// model, here on the host); a pixel it refuses gets (-1, -1), the border under pmv_frames_remap
bool fisheye_map(const double* K, const double* k4, const double* R, const double* newK, int w, int h, float* map_x, float* map_y) {
    double iR[9];
    if (!map_ray_matrix(K, R, newK, iR)) return false;
    LiftCam c{};
    c.fx = K[0]; c.fy = K[4]; c.cx = K[2]; c.cy = K[5]; c.ifx = 1.0 / c.fx; c.ify = 1.0 / c.fy;
    c.k1 = k4[0]; c.k2 = k4[1]; c.k3 = k4[2]; c.k4 = k4[3];
    c.iters = 10; c.model = LIFT_FISHEYE;
    for (int i = 0; i < h; i++)
        for (int j = 0; j < w; j++) {
            const double X = iR[0] * j + iR[1] * i + iR[2], Y = iR[3] * j + iR[4] * i + iR[5], W = iR[6] * j + iR[7] * i + iR[8];
            float u, v;
            const bool ok = fisheye_project(c, X, Y, W, &u, &v);
            map_x[(size_t)i * w + j] = ok ? u : -1.f;
            map_y[(size_t)i * w + j] = ok ? v : -1.f;
        }
    return true;
}

hipError_t launch_remap(hipStream_t s, const uint8_t* slots, const PyrLayout* d_geom, const RemapRec* d_recs, int n, int max_w, int max_h, uint8_t* d_scratch) {
    if (!slots || !d_geom || !d_recs || !d_scratch || n < 1 || n > 65535 || max_w < 1 || max_h < 1) return hipErrorInvalidValue;
    const size_t per_block = (size_t)RM_T * RM_PX;
    const size_t gx = ((size_t)max_w * (size_t)max_h + per_block - 1) / per_block;
    if (gx > 0x7fffffffu / per_block) return hipErrorInvalidValue;   // (the kernel's pixel index is 32 bits)
    ProfScope ps(K_PAD0, s);
    hipLaunchKernelGGL(k_remap, dim3((unsigned)gx, n), dim3(RM_T), 0, s, slots, d_geom, d_recs, d_scratch);
    return hipGetLastError();
}

hipError_t launch_remap_src(hipStream_t s, uint8_t* slots, const PyrLayout* d_geom, const RemapSrcRec* d_recs, int n, int max_w, int max_h) {
    if (!slots || !d_geom || !d_recs || n < 1 || n > 65535 || max_w < 1 || max_h < 1) return hipErrorInvalidValue;
    const size_t per_block = (size_t)RM_T * RM_PX;
    const size_t gx = ((size_t)max_w * (size_t)max_h + per_block - 1) / per_block;
    if (gx > 0x7fffffffu / per_block) return hipErrorInvalidValue;   // (the kernel's pixel index is 32 bits)
    ProfScope ps(K_PAD0, s);
    hipLaunchKernelGGL(k_remap_src, dim3((unsigned)gx, n), dim3(RM_T), 0, s, slots, d_geom, d_recs);
    return hipGetLastError();
}

}  // namespace pmv
