// pmv_frames_clahe / pmv_batch_frame_upload_clahe: cv::CLAHE::apply on level 0 of frame slots, in place (contract: include/pmv_hip.h; the
// arithmetic, statement by statement: tests/twin/clahe_twin.cpp).
// Two list-driven launches, because a pixel needs the LUTs of four tiles: k_clahe_lut makes the 256-byte LUT of every tile of every frame
// of the list (integer histogram, clip, redistribution, prefix sum, one rounding per bin), k_clahe_apply interpolates between the four
// LUTs around each pixel and writes the interior of level 0 back where it was read. A record per frame (ClaheRec, pmv_device.h) names the
// slot, the frame's entry of a geometry table, the tile grid and the host's constants, so one pair of launches serves frames of any sizes
// and parameters. Both kernels read the INTERIOR of level 0 only: the extension cv makes for sizes that are no multiple of the grid is
// taken from it with reflect101 (a staged slot has no border yet), and the border is rebuilt afterwards by the in-place k_pad_level0.
// LDS atomics and vector stores only.
#include "pmv_device.h"
#include "pmv_prof.h"

namespace pmv {

namespace {

constexpr int CL_WAVES = 4, CL_T = 64 * CL_WAVES;
constexpr int CA_PX = 4;                       // pixels per thread of k_clahe_apply: one dword of a 64-byte aligned interior row
constexpr int CA_ROW = 64 * CA_PX;             // pixels of a row per wavefront

__device__ __forceinline__ int cl_u(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ float cl_uf(float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); }
__device__ __forceinline__ int cl_u8(float v) { const int q = (int)rintf(v); return q < 0 ? 0 : q > 255 ? 255 : q; }   // saturate_cast<uchar>(float): cvRound, half to even

// One workgroup per (tile, frame). Each wavefront counts into its own 256 bins, so the wavefronts of a workgroup never meet on an address;
// then one thread per bin.
__global__ __launch_bounds__(CL_T) void k_clahe_lut(const uint8_t* __restrict__ slots, const PyrLayout* __restrict__ geom, const ClaheRec* __restrict__ recs,
                                                     uint8_t* __restrict__ lut) {
    __shared__ int hist[CL_WAVES][256];
    __shared__ int part[2][CL_WAVES];
    const ClaheRec r = recs[blockIdx.y];
    const int tiles_x = cl_u(r.tiles_x), tiles_y = cl_u(r.tiles_y);
    const int tile = blockIdx.x;
    if (tile >= tiles_x * tiles_y) return;     // (the grid is sized for the largest grid of the list: before the first load or barrier)
    GeomEntry& L = geom_entry(geom, r.geom);
    const int w = L.w[0], h = L.h[0], stride = L.stride[0];
    const int tile_w = cl_u(r.tile_w), tile_h = cl_u(r.tile_h), clip = cl_u(r.clip);
    const float lut_scale = cl_uf(r.lut_scale);
    const uint8_t* img = slots + (size_t)cl_u(r.slot) * L.slot_bytes + L.gray_off;
    const int wave = cl_u((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63, bin = threadIdx.x;
#pragma unroll
    for (int k = 0; k < CL_WAVES; k++) hist[k][bin] = 0;
    __syncthreads();
    const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
    const int x0 = tx * tile_w, y0 = ty * tile_h;
    for (int ry = wave; ry < tile_h; ry += CL_WAVES) {
        const uint8_t* row = img + (size_t)reflect101(y0 + ry, h) * (size_t)stride;   // rows and columns past the image: cv's REFLECT_101 extension
        for (int cx = lane; cx < tile_w; cx += 64) atomicAdd(&hist[wave][row[reflect101(x0 + cx, w)]], 1);
    }
    __syncthreads();
    int v = 0;
#pragma unroll
    for (int k = 0; k < CL_WAVES; k++) v += hist[k][bin];
    if (clip > 0) {                            // (the same for the whole workgroup)
        const int excess = v > clip ? v - clip : 0;
        v = v > clip ? clip : v;
        const int ws = wave_sum_i32(excess);
        if (lane == 0) part[0][wave] = ws;
        __syncthreads();
        int clipped = 0;
#pragma unroll
        for (int k = 0; k < CL_WAVES; k++) clipped += part[0][k];
        const int batch = clipped >> 8, residual = clipped & 255;
        v += batch;
        if (residual != 0) {
            // cv's loop `for (i = 0; i < 256 && residual > 0; i += step, residual--) hist[i]++` visits i = 0, step, .. (residual - 1) step,
            // all below 256 because step = 256 / residual rounds down
            const int step = 256 / residual;   // >= 1: residual <= 255
            const int q = bin / step;
            if (bin - q * step == 0 && q < residual) v++;
        }
    }
    // prefix sum over the 256 bins: a scan inside each wavefront, then the sums of the wavefronts before it
    int s = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(s, o, 64);
        if (lane >= o) s += t;
    }
    if (lane == 63) part[1][wave] = s;
    __syncthreads();
    for (int k = 0; k < wave; k++) s += part[1][k];
    lut[(size_t)r.lut_off + (size_t)tile * 256 + bin] = (uint8_t)cl_u8((float)s * lut_scale);
}

// A wavefront equalises CA_ROW consecutive pixels of one row, a workgroup CL_WAVES rows. Every thread reads one dword of its row, looks its
// four pixels up and writes the dword back: a pixel is read once and written once, by the same thread, so the kernel works in place. The
// last dword of a row may reach into the right border; those bytes go back as they were read.
__global__ __launch_bounds__(CL_T) void k_clahe_apply(uint8_t* __restrict__ slots, const PyrLayout* __restrict__ geom, const ClaheRec* __restrict__ recs,
                                                       const uint8_t* __restrict__ lut) {
    const ClaheRec r = recs[blockIdx.z];
    GeomEntry& L = geom_entry(geom, r.geom);
    const int w = L.w[0], h = L.h[0], stride = L.stride[0];
    if ((int)blockIdx.y * CL_WAVES >= h || (int)blockIdx.x * CA_ROW >= w) return;   // (the grid is sized for the largest frame of the list)
    const int wave = cl_u((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    const int y = blockIdx.y * CL_WAVES + wave, x = (blockIdx.x * 64 + lane) * CA_PX;
    if (y >= h || x >= w) return;              // (no barrier in this kernel)
    const int tiles_x = cl_u(r.tiles_x), tiles_y = cl_u(r.tiles_y);
    const float inv_tw = cl_uf(r.inv_tw), inv_th = cl_uf(r.inv_th);
    const float tyf = (float)y * inv_th - 0.5f;
    const float fy = floorf(tyf);
    int ty1 = (int)fy, ty2 = ty1 + 1;
    const float ya = tyf - fy, ya1 = 1.0f - ya;
    ty1 = ty1 < 0 ? 0 : ty1;
    ty2 = ty2 > tiles_y - 1 ? tiles_y - 1 : ty2;
    const uint8_t* lut1 = lut + (size_t)r.lut_off + (size_t)(ty1 * tiles_x) * 256;
    const uint8_t* lut2 = lut + (size_t)r.lut_off + (size_t)(ty2 * tiles_x) * 256;
    uint32_t* p = (uint32_t*)(slots + (size_t)cl_u(r.slot) * L.slot_bytes + L.gray_off + (size_t)y * (size_t)stride + (size_t)x);
    const uint32_t in = *p;
    uint32_t out = 0;
#pragma unroll
    for (int k = 0; k < CA_PX; k++) {
        const int val = (int)((in >> (8 * k)) & 0xffu);
        int res = val;
        if (x + k < w) {
            const float txf = (float)(x + k) * inv_tw - 0.5f;
            const float fx = floorf(txf);
            int tx1 = (int)fx, tx2 = tx1 + 1;
            const float xa = txf - fx, xa1 = 1.0f - xa;
            tx1 = tx1 < 0 ? 0 : tx1;
            tx2 = tx2 > tiles_x - 1 ? tiles_x - 1 : tx2;
            const int i1 = tx1 * 256 + val, i2 = tx2 * 256 + val;
            const float top = (float)lut1[i1] * xa1 + (float)lut1[i2] * xa;
            const float bot = (float)lut2[i1] * xa1 + (float)lut2[i2] * xa;
            res = cl_u8(top * ya1 + bot * ya);
        }
        out |= (uint32_t)res << (8 * k);
    }
    *p = out;
}

}  // namespace

ClaheRec clahe_record(int slot, int geom, int w, int h, double clip_limit, int tiles_x, int tiles_y) {
    int ew = w, eh = h;
    if (w % tiles_x != 0 || h % tiles_y != 0) {   // cv extends BOTH directions then, a direction that divides by a whole tile count
        ew = w + (tiles_x - w % tiles_x);
        eh = h + (tiles_y - h % tiles_y);
    }
    ClaheRec r{};
    r.slot = slot; r.geom = geom; r.tiles_x = tiles_x; r.tiles_y = tiles_y;
    r.tile_w = ew / tiles_x; r.tile_h = eh / tiles_y;
    const int area = r.tile_w * r.tile_h;
    r.lut_scale = (float)255 / area;
    r.clip = 0;
    if (clip_limit > 0.0) {
        double c = clip_limit * area / 256;
        if (c > (double)area) c = (double)area;   // no bin exceeds area: the same result, and the cast cannot overflow
        r.clip = (int)c > 1 ? (int)c : 1;
    }
    r.inv_tw = 1.0f / r.tile_w; r.inv_th = 1.0f / r.tile_h;
    return r;
}

hipError_t launch_clahe(hipStream_t s, uint8_t* slots, const PyrLayout* d_geom, const ClaheRec* d_recs, int n, int max_tiles, int max_w, int max_h, uint8_t* d_lut) {
    if (!slots || !d_geom || !d_recs || !d_lut || n < 1 || n > 65535 || max_tiles < 1 || max_tiles > CLAHE_MAX_TILES * CLAHE_MAX_TILES || max_w < 1 || max_h < 1)
        return hipErrorInvalidValue;
    {
        ProfScope ps(K_PAD0, s);
        hipLaunchKernelGGL(k_clahe_lut, dim3(max_tiles, n), dim3(CL_T), 0, s, slots, d_geom, d_recs, d_lut);
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    {
        ProfScope ps(K_PAD0, s);
        hipLaunchKernelGGL(k_clahe_apply, dim3((max_w + CA_ROW - 1) / CA_ROW, (max_h + CL_WAVES - 1) / CL_WAVES, n), dim3(CL_T), 0, s, slots, d_geom, d_recs, d_lut);
    }
    return hipGetLastError();
}

}  // namespace pmv
