// pmv_corner_subpix / pmv_batch_corner_subpix: cv::cornerSubPix on level 0 of a frame slot (contract: include/pmv_hip.h; the arithmetic,
// statement by statement: tests/twin/subpix_twin.cpp with order = 1).
// One wavefront per corner, four corners per workgroup. The (2 win_w + 3) x (2 win_h + 3) float patch of getRectSubPix lives in the
// wavefront's own LDS area and is rebuilt from the 8-bit level 0 in every iteration; the weight table (host, libm) is read once per
// workgroup. The loop is wave-uniform: the position, the determinant and the stop tests are the same bits in every lane, so a corner that
// converges leaves the loop as a whole wavefront and no workgroup barrier sits inside it. Nothing but the level-0 bytes is read from HBM
// inside the loop, nothing is written before the end, and there are no atomics.
#include "pmv_ctx.h"
#include "pmv_prof.h"
#include <float.h>
#include <string.h>

namespace pmv {

namespace {

constexpr int SP_WAVES = 4, SP_T = 64 * SP_WAVES;

__device__ __forceinline__ float sp_uniform(float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); }
__device__ __forceinline__ int sp_floor(float v) { const int i = (int)v; return i - ((float)i > v); }   // cvFloor
__device__ __forceinline__ int sp_clamp(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }
// The patch is written and read by the lanes of ONE wavefront, whose LDS operations complete in program order: what is needed is that the
// compiler keeps that order (a workgroup barrier here would wait for wavefronts that have left the loop).
__device__ __forceinline__ void sp_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// getRectSubPix(src, PW x PH, (cx, cy)) from 8-bit to float into P, both of cv's paths. img: pixel (0, 0) of the REAL cols x rows image
// (row pitch st); the REFLECT_101 frame stored around it is never sampled: every index below lies inside the image.
__device__ __forceinline__ void sp_patch(const uint8_t* __restrict__ img, int st, int cols, int rows, float cx, float cy, int PW, int PH, float* __restrict__ P, int lane) {
    cx -= (PW - 1) * 0.5f;
    cy -= (PH - 1) * 0.5f;
    const int ipx = sp_floor(cx), ipy = sp_floor(cy);
    int i = 0, j = lane;
    while (j >= PW) { j -= PW; i++; }
    if (0 <= ipx && ipx + PW < cols && 0 <= ipy && ipy + PH < rows) {
        float a = cx - ipx;
        const float b = cy - ipy;
        a = a > 0.0001f ? a : 0.0001f;
        const float a12 = a * (1.f - b), a22 = a * b, b1 = 1.f - b, b2 = b;
        const double s = (1. - a) / a;
        const uint8_t* base = img + (ptrdiff_t)ipy * st + ipx;
        for (int k = lane; k < PW * PH; k += 64) {
            const uint8_t* src = base + (ptrdiff_t)i * st;
            const float t = a12 * src[j + 1] + a22 * src[j + 1 + st];
            // element j needs t[j] and t[j - 1] only: cv's running `prev` is no serial chain
            float prev;
            if (j == 0) prev = (1 - a) * (b1 * src[0] + b2 * src[st]);
            else { const float tp = a12 * src[j] + a22 * src[j + st]; prev = (float)(tp * s); }
            P[k] = prev + t;
            j += 64;
            while (j >= PW) { j -= PW; i++; }
        }
        return;
    }
    const float a = cx - ipx, b = cy - ipy;
    const float a11 = (1.f - a) * (1.f - b), a12 = a * (1.f - b), a21 = (1.f - a) * b, a22 = a * b, b1 = 1.f - b, b2 = b;
    for (int k = lane; k < PW * PH; k += 64) {
        const uint8_t* r0 = img + (ptrdiff_t)sp_clamp(ipy + i, 0, rows - 1) * st;
        const uint8_t* r1 = img + (ptrdiff_t)sp_clamp(ipy + i + 1, 0, rows - 1) * st;
        const int x0 = ipx + j;
        float v;
        if (x0 < 0 || x0 >= cols - 1) {   // both sample columns clamp to the same column
            const int xc = x0 < 0 ? 0 : cols - 1;
            v = r0[xc] * b1 + r1[xc] * b2;
        } else
            v = r0[x0] * a11 + r0[x0 + 1] * a12 + r1[x0] * a21 + r1[x0 + 1] * a22;
        P[k] = v;
        j += 64;
        while (j >= PW) { j -= PW; i++; }
    }
}

struct SpResult { float x, y; int updates, flags; };

template <class LRef>
__device__ __forceinline__ SpResult sp_refine(const uint8_t* __restrict__ slot, LRef L, float tx, float ty, const SubpixArgs& A, const float* __restrict__ sM,
                                              float* __restrict__ P, int lane) {
    const int WW = 2 * A.win_w + 1, WH = 2 * A.win_h + 1, PW = WW + 2, PH = WH + 2;
    const int cols = L.w[0], rows = L.h[0], st = L.stride[0];
    const uint8_t* img = level_origin(slot, L, 0);
    float cx = tx, cy = ty;
    int iter = 0, updates = 0, flags = 0;
    double err = 0;
    bool broke = false;
    do {
        sp_wave_sync();   // (the previous iteration's reads of P are done)
        sp_patch(img, st, cols, rows, cx, cy, PW, PH, P, lane);
        sp_wave_sync();
        // the five sums: lane l adds the window pixels k = l, l + 64, ... in ascending k, then one tree over the lanes (wave_sum_f64:
        // neighbours, pairs of pairs, ... halves) - the order of the twin, whatever n, the point's place in the launch or the call's form
        double sa = 0, sb = 0, sc = 0, s1 = 0, s2 = 0;
        int i = 0, j = lane;
        while (j >= WW) { j -= WW; i++; }
        for (int k = lane; k < WW * WH; k += 64) {
            const float* sp = P + (i + 1) * PW + (j + 1);
            const double m = sM[k];
            const double tgx = sp[1] - sp[-1];
            const double tgy = sp[PW] - sp[-PW];
            const double gxx = tgx * tgx * m, gxy = tgx * tgy * m, gyy = tgy * tgy * m;
            const double px = j - A.win_w, py = i - A.win_h;
            sa += gxx; sb += gxy; sc += gyy;
            s1 += gxx * px + gxy * py;
            s2 += gxy * px + gyy * py;
            j += 64;
            while (j >= WW) { j -= WW; i++; }
        }
        sa = wave_sum_f64(sa); sb = wave_sum_f64(sb); sc = wave_sum_f64(sc); s1 = wave_sum_f64(s1); s2 = wave_sum_f64(s2);
        const double det = sa * sc - sb * sb;
        if (fabs(det) <= DBL_EPSILON * DBL_EPSILON) { flags |= 1; broke = true; break; }
        const double scale = 1.0 / det;
        const float nx = (float)(cx + sc * scale * s1 - sb * scale * s2);
        const float ny = (float)(cy - sb * scale * s1 + sa * scale * s2);
        err = (nx - cx) * (nx - cx) + (ny - cy) * (ny - cy);
        cx = nx; cy = ny;
        updates++;
        if (cx < 0 || cx >= cols || cy < 0 || cy >= rows) { flags |= 2; broke = true; break; }
    } while (++iter < A.max_iter && err > A.eps2);
    if (!broke && err > A.eps2) flags |= 4;
    if (fabs(cx - tx) > A.win_w || fabs(cy - ty) > A.win_h) { cx = tx; cy = ty; flags |= 8; }
    return SpResult{cx, cy, updates, flags};
}

// TABLE: the records' geometry is an entry of the context's table (the batch engine: one launch for points of any slots and frame sizes);
// otherwise every record has the geometry L1 (the single call). The same function does the work: the bytes are the same.
// GROUP (a group of trackers): blockIdx.y is the request - its count word n_dev[request], its frame slot req_slots[request], its share of n
// points in ixy and in the outputs. Every other form is the one request it was, and its code is what it was.
template <bool TABLE, bool GROUP = false>
__global__ __launch_bounds__(SP_T) void k_corner_subpix(const uint8_t* __restrict__ slots, const PyrLayout* __restrict__ geom, PyrLayout L1,
                                                        const SubpixRec* __restrict__ recs, int n, const float* __restrict__ table, SubpixArgs A,
                                                        float* __restrict__ out_xy, uint8_t* __restrict__ out_iters, uint8_t* __restrict__ out_flags,
                                                        const int* __restrict__ n_dev, const int* __restrict__ ixy, int ixy_slot,
                                                        const int* __restrict__ req_slots) {
    extern __shared__ float sp_lds[];
    BACKEND_PRIO();
    const int WW = 2 * A.win_w + 1, WH = 2 * A.win_h + 1;
    float* sM = sp_lds;                                          // [WW * WH] the weight table
    for (int i = threadIdx.x; i < WW * WH; i += SP_T) sM[i] = table[i];
    __syncthreads();                                             // the only workgroup barrier, before any wavefront can leave
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    // n_dev / ixy (launch_corner_subpix_dev): the count comes from device memory, clamped to the grid's n, and the points are int corners
    const int in_req = blockIdx.x * SP_WAVES + wave;
    int n_pts = n;
    if (n_dev) { const int c = GROUP ? n_dev[blockIdx.y] : *n_dev; n_pts = c < 0 ? 0 : (c < n ? c : n); }
    if (in_req >= n_pts) return;
    const size_t pt = GROUP ? (size_t)blockIdx.y * n + in_req : (size_t)in_req;
    float* P = sp_lds + WW * WH + wave * (WW + 2) * (WH + 2);    // [(WW + 2) * (WH + 2)] this wavefront's patch
    const SubpixRec r = ixy ? SubpixRec{(float)ixy[2 * pt], (float)ixy[2 * pt + 1], GROUP ? req_slots[blockIdx.y] : ixy_slot, 0} : recs[pt];
    const float tx = sp_uniform(r.x), ty = sp_uniform(r.y);
    const int slot = __builtin_amdgcn_readfirstlane(r.slot);
    SpResult R;
    if constexpr (TABLE) {
        GeomEntry& L = geom_entry(geom, r.geom);
        R = sp_refine<GeomEntry&>(slots + (size_t)slot * L.slot_bytes, L, tx, ty, A, sM, P, lane);
    } else
        R = sp_refine<const PyrLayout&>(slots + (size_t)slot * L1.slot_bytes, L1, tx, ty, A, sM, P, lane);
    if (lane == 0) {
        out_xy[2 * pt] = R.x; out_xy[2 * pt + 1] = R.y;
        out_iters[pt] = (uint8_t)R.updates; out_flags[pt] = (uint8_t)R.flags;
    }
}

size_t sp_lds_bytes(const SubpixArgs& A) {
    const size_t WW = 2 * (size_t)A.win_w + 1, WH = 2 * (size_t)A.win_h + 1;
    return (WW * WH + SP_WAVES * (WW + 2) * (WH + 2)) * sizeof(float);
}
bool sp_args_ok(const SubpixArgs& A) {
    return A.win_w >= 1 && A.win_w <= SUBPIX_MAX_WIN && A.win_h >= 1 && A.win_h <= SUBPIX_MAX_WIN && A.max_iter >= 1 && A.max_iter <= 100 && A.eps2 >= 0.0;
}

}  // namespace

void subpix_table(int win_w, int win_h, int zero_w, int zero_h, float* out) {
    const int WW = 2 * win_w + 1, WH = 2 * win_h + 1;
    for (int i = 0; i < WH; i++) {
        const float y = (float)(i - win_h) / win_h;
        const float vy = expf(-y * y);
        for (int j = 0; j < WW; j++) {
            const float x = (float)(j - win_w) / win_w;
            out[i * WW + j] = (float)(vy * expf(-x * x));
        }
    }
    if (zero_w >= 0 && zero_h >= 0 && 2 * zero_w + 1 < WW && 2 * zero_h + 1 < WH)
        for (int i = win_h - zero_h; i <= win_h + zero_h; i++)
            for (int j = win_w - zero_w; j <= win_w + zero_w; j++) out[i * WW + j] = 0.f;
}

// The context's weight table (d_subpix_tab) for p, and the launch arguments that go with it. The table is kept with the window and the
// (effective) zero zone it was computed for: a caller keeps its parameters, so it crosses the bus once. On another key the front-end stream is
// waited for first - the pinned mirror may still be on its way from the last change, and a launch in flight may still read the old table.
hipError_t subpix_table_ready(pmv_ctx* ctx, const pmv_subpix_params* p, SubpixArgs* A) {
    hipError_t e = ctx->h_subpix_tab.ensure(SUBPIX_TABLE_MAX * sizeof(float));
    if (!e) e = ctx->d_subpix_tab.ensure(SUBPIX_TABLE_MAX * sizeof(float));
    int zw, zh;
    subpix_zero_zone(p, &zw, &zh);
    const int key[4] = {p->win_w, p->win_h, zw, zh};
    *A = SubpixArgs{p->win_w, p->win_h, p->max_iter, p->eps * p->eps};
    if (e != hipSuccess || memcmp(key, ctx->subpix_tab_key, sizeof(key)) == 0) return e;
    if ((e = hipStreamSynchronize(ctx->s_front)) != hipSuccess) return e;
    subpix_table(p->win_w, p->win_h, zw, zh, ctx->h_subpix_tab);
    e = hipMemcpyAsync(ctx->d_subpix_tab, ctx->h_subpix_tab, (size_t)(2 * p->win_w + 1) * (2 * p->win_h + 1) * sizeof(float), hipMemcpyHostToDevice, ctx->s_front);
    if (e == hipSuccess) memcpy(ctx->subpix_tab_key, key, sizeof(key));
    return e;
}

hipError_t launch_corner_subpix(hipStream_t s, const uint8_t* slots, const PyrLayout& L, const SubpixRec* d_recs, int n, const float* d_table, const SubpixArgs& A,
                                float* d_out_xy, uint8_t* d_out_iters, uint8_t* d_out_flags) {
    if (!slots || !d_recs || !d_table || !d_out_xy || !d_out_iters || !d_out_flags || n < 1 || !sp_args_ok(A)) return hipErrorInvalidValue;
    ProfScope ps(K_GFTT_PICK, s);
    hipLaunchKernelGGL(k_corner_subpix<false>, dim3((n + SP_WAVES - 1) / SP_WAVES), dim3(SP_T), sp_lds_bytes(A), s, slots, (const PyrLayout*)nullptr, L, d_recs, n, d_table, A,
                       d_out_xy, d_out_iters, d_out_flags, (const int*)nullptr, (const int*)nullptr, 0, (const int*)nullptr);
    return hipGetLastError();
}

hipError_t launch_corner_subpix_geom(hipStream_t s, const uint8_t* slots, const PyrLayout* d_geom, const SubpixRec* d_recs, int n, const float* d_table, const SubpixArgs& A,
                                     float* d_out_xy, uint8_t* d_out_iters, uint8_t* d_out_flags) {
    if (!slots || !d_geom || !d_recs || !d_table || !d_out_xy || !d_out_iters || !d_out_flags || n < 1 || !sp_args_ok(A)) return hipErrorInvalidValue;
    ProfScope ps(K_GFTT_PICK, s);
    hipLaunchKernelGGL(k_corner_subpix<true>, dim3((n + SP_WAVES - 1) / SP_WAVES), dim3(SP_T), sp_lds_bytes(A), s, slots, d_geom, PyrLayout{}, d_recs, n, d_table, A,
                       d_out_xy, d_out_iters, d_out_flags, (const int*)nullptr, (const int*)nullptr, 0, (const int*)nullptr);
    return hipGetLastError();
}

hipError_t launch_corner_subpix_dev(hipStream_t s, const uint8_t* slots, const PyrLayout& L, const int* d_ixy, int slot, int n_cap, const int* d_n, const float* d_table,
                                    const SubpixArgs& A, float* d_out_xy, uint8_t* d_out_iters, uint8_t* d_out_flags, const int* d_req_slots, int n_req) {
    if (!slots || !d_ixy || !d_n || !d_table || !d_out_xy || !d_out_iters || !d_out_flags || n_cap < 1 || (!d_req_slots && slot < 0) || n_req < 1 || n_req > 65535 ||
        (n_req > 1 && !d_req_slots) || !sp_args_ok(A)) return hipErrorInvalidValue;
    ProfScope ps(K_GFTT_PICK, s);
    if (d_req_slots)
        hipLaunchKernelGGL((k_corner_subpix<false, true>), dim3((n_cap + SP_WAVES - 1) / SP_WAVES, n_req), dim3(SP_T), sp_lds_bytes(A), s, slots, (const PyrLayout*)nullptr, L,
                           (const SubpixRec*)nullptr, n_cap, d_table, A, d_out_xy, d_out_iters, d_out_flags, d_n, d_ixy, slot, d_req_slots);
    else
        hipLaunchKernelGGL(k_corner_subpix<false>, dim3((n_cap + SP_WAVES - 1) / SP_WAVES), dim3(SP_T), sp_lds_bytes(A), s, slots, (const PyrLayout*)nullptr, L,
                           (const SubpixRec*)nullptr, n_cap, d_table, A, d_out_xy, d_out_iters, d_out_flags, d_n, d_ixy, slot, (const int*)nullptr);
    return hipGetLastError();
}

}  // namespace pmv
