// gfx950 front-end kernels: padded pyramid build, per-track pyramidal Lucas–Kanade, fused corner detectors.
// Replaces the OpenCV calls behind BaseFeatureMatcher / BaseFeatureExtractor (see include/pmv_hip.h for file:line).
// All integer results (track coordinates after truncation, status bytes, corner lists) are bit-exact with oracle/:
//   * LK: every window sum is an exact integer (per-lane int32 partials, 64-bit wave reduction), rounded once to f32;
//   * GFTT: float32 ops in a fixed order, compiled with -ffp-contract=off; the 3x3 box sum is a 9-term double sum.
//     pmv_detect_gftt_ex (block size 1..15, Harris, mask): the b*b-term double sum in raster order of tests/twin/gftt_twin.cpp.
#include "pmv_device.h"
#include "pmv_prof.h"
#include "pmv_gfsort.h"
#include <float.h>

namespace pmv {

// =========================================================================================================
// Pyramid
// =========================================================================================================
// Both kernels work on ONE padded output row per workgroup (grid = (1, padded rows, frames)) and touch global memory only with
// coalesced dword / 16-byte accesses; the byte-granular REFLECT_101 gather happens in LDS. (The first version read 25 bytes per
// output pixel straight from global memory: 0.6 TB/s; this one moves each source row once per output row that needs it.)

// NB valid bytes starting at byte `off` of a 4-byte-aligned LDS row as packed little-endian dwords (see k_lk)
template <int NB>
__device__ inline void lds_bytes_aligned(const uint8_t* row, int off, uint32_t (&e)[(NB + 3) / 4]) {
    constexpr int ND = (NB + 3 + 3) / 4, NE = (NB + 3) / 4;
    const uint32_t* w = (const uint32_t*)row + (off >> 2);
    const uint32_t sh = (uint32_t)off & 3u;
    uint32_t d[ND];
#pragma unroll
    for (int j = 0; j < ND; j++) d[j] = w[j];
#pragma unroll
    for (int j = 0; j < NE; j++) e[j] = __builtin_amdgcn_alignbyte(j + 1 < ND ? d[j + 1] : 0u, d[j], sh);
}

// One padded REFLECT_101 row from an unpadded row of `w` bytes that sits in LDS at byte `lead` of a 4-byte-aligned buffer (with >= 24
// bytes of slack behind it): 16 bytes per thread and step. Interior groups are aligned gathers; the left and right borders are
// byte-reversed runs of the row (PAD % 16 == 0, so only the group that straddles the right edge mixes both). Rows narrower than
// PAD + 48 take the per-byte path everywhere.
template <int T>
__device__ inline void write_padded_row(const uint8_t* lrow, int lead, int w, uint8_t* dst) {
    const int pw = w + 2 * PAD;
    const bool wide = w >= PAD + 48;   // block-uniform
    for (int x16 = threadIdx.x * 16; x16 < pw; x16 += T * 16) {   // (strides are multiples of 64: a 16-byte store never leaves the row)
        uint32_t v[4];
        const int sx0 = x16 - PAD;
        if (sx0 >= 0 && sx0 + 15 < w) {
            lds_bytes_aligned<16>(lrow, lead + sx0, v);
        } else if (wide && (sx0 < 0 || sx0 >= w)) {
            // dst[x16 + k] = row[s - k]: left border s = PAD - x16 (>= 16), right border s = 2w - 2 - sx0
            const int s = sx0 < 0 ? -sx0 : 2 * w - 2 - sx0;
            uint32_t e[4];
            lds_bytes_aligned<16>(lrow, lead + s - 15, e);
#pragma unroll
            for (int q = 0; q < 4; q++) v[q] = __builtin_bswap32(e[3 - q]);
        } else if (wide) {
            // the group that straddles the right edge: the first n_in bytes run forward, the rest is the reversed run
            const int n_in = w - sx0;   // 1 .. 15
            uint32_t a[4], e[4];
            lds_bytes_aligned<16>(lrow, lead + sx0, a);
            lds_bytes_aligned<16>(lrow, lead + 2 * w - 2 - sx0 - 15, e);
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const int lo = n_in - 4 * q;
                const uint32_t m = lo >= 4 ? 0xffffffffu : (lo <= 0 ? 0u : ((1u << (8 * lo)) - 1u));
                v[q] = (a[q] & m) | (__builtin_bswap32(e[3 - q]) & ~m);
            }
        } else {
#pragma unroll
            for (int q = 0; q < 4; q++) {
                uint32_t t = 0;
#pragma unroll
                for (int k = 0; k < 4; k++) t |= (uint32_t)lrow[lead + reflect101(sx0 + 4 * q + k, w)] << (8 * k);
                v[q] = t;
            }
        }
        *(uint4*)(dst + x16) = make_uint4(v[0], v[1], v[2], v[3]);
    }
}

// level 0: the gray frame sits in the interior of its padded buffer (staged there row by row); this kernel adds the REFLECT_101 frame
// IN PLACE: every padded row is rebuilt from the interior row it mirrors (an interior row from itself: same bytes; a border row from
// another row's interior, which no block changes).
constexpr int PAD0_T = 128, PAD0_R = 4;   // rows per workgroup: their loads are in flight together
__host__ __device__ inline int pad0_row_lds(int w) { return ((w + 3 + 24 + 3) / 4) * 4; }
// Workgroup column z builds one slot. Range form (list == nullptr): slot first_slot + z, level 0 from tight gray frame z at `tight` (staging
// / upload: the 256-byte aligned landing area) or, with `tight` null too, from the level's own interior. List form (the feeder, ingest_batch.hip):
// slot list[z].slot, level 0 from list[z].src (the HBM landing area or mapped pinned host memory, at any alignment), in place when that is null.
// Tight rows are generally unaligned: they are fetched as the aligned dwords that hold the row's bytes and no others, so a source that ends at
// the end of a host page is never over-read.
// (LRef: const PyrLayout& = the launch's own geometry, GeomEntry& = the frame's entry of the geometry table; the grid of a list launch is
// sized for the tallest frame of the round, so a workgroup below its own frame leaves before its first load or barrier)
// `pitch`: bytes from one source row to the next (block-uniform; w for a tight frame). The fetch rule holds for any pitch and base: the lead
// offset is kept per row, and the last row's last dword is the one that holds its last byte.
template <class LRef>
__device__ __forceinline__ void pad_level0_rows(uint8_t* slots, LRef L, int s, const uint8_t* __restrict__ frame, size_t pitch) {
    extern __shared__ __attribute__((aligned(16))) uint8_t srow_all[];   // PAD0_R x row_lds bytes
    const int w = L.w[0], h = L.h[0], stride = L.stride[0];
    uint8_t* slot = slots + (size_t)s * L.slot_bytes;
    const int row_lds = pad0_row_lds(w);
    const int ph = h + 2 * PAD;
    const int py0 = blockIdx.y * PAD0_R;
    if (py0 >= ph) return;
    unsigned lead[PAD0_R];
#pragma unroll
    for (int r = 0; r < PAD0_R; r++) {
        const int py = py0 + r < ph ? py0 + r : ph - 1;     // (rows past the end repeat the last one; they are not stored)
        const int sy = reflect101(py - PAD, h);
        const uint32_t* src;
        int nd;
        if (frame) {
            const uintptr_t a = (uintptr_t)(frame + (size_t)sy * pitch);
            lead[r] = (unsigned)(a & 3u);
            src = (const uint32_t*)(a & ~(uintptr_t)3);
            nd = (int)((lead[r] + (unsigned)w + 3u) >> 2);
        } else {
            lead[r] = 0u;                                   // interior rows start 64-byte aligned (PAD and the stride are multiples of 64)
            src = (const uint32_t*)(slot + L.gray_off + (size_t)sy * (size_t)stride);
            nd = (w + 3) >> 2;                              // (the last dword may reach into the right border: inside the buffer)
        }
        uint32_t* srow = (uint32_t*)(srow_all + r * row_lds);
        for (int d = threadIdx.x; d < nd; d += PAD0_T) srow[d] = src[d];
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < PAD0_R; r++) {
        if (py0 + r >= ph) break;
        write_padded_row<PAD0_T>(srow_all + r * row_lds, (int)lead[r], w, slot + L.off[0] + (size_t)(py0 + r) * stride);
    }
}
__global__ __launch_bounds__(PAD0_T) void k_pad_level0(uint8_t* slots, PyrLayout L, int first_slot, const uint8_t* __restrict__ tight) {
    // tight source frame z, or null: in place (block-uniform)
    pad_level0_rows<const PyrLayout&>(slots, L, first_slot + (int)blockIdx.z, tight ? tight + (size_t)blockIdx.z * (size_t)L.w[0] * (size_t)L.h[0] : nullptr, (size_t)L.w[0]);
}
__global__ __launch_bounds__(PAD0_T) void k_pad_level0_list(uint8_t* slots, const PyrLayout* __restrict__ geom, const PyrListEntry* __restrict__ list) {
    const PyrListEntry e = list[blockIdx.z];
    GeomEntry& L = geom_entry(geom, e.geom);
    pad_level0_rows<GeomEntry&>(slots, L, __builtin_amdgcn_readfirstlane(e.slot), e.src, (size_t)L.w[0]);
}
// Pitched list form (the upload class of a batch session, batch_session.hip): the source is read IN PLACE - a camera buffer with aligned
// rows, an ROI view into a larger image, a hipMallocPitch surface - so the entry carries the bytes from row to row. The entry is the same
// for the whole workgroup: slot and pitch go through readfirstlane and stay in scalar registers.
__global__ __launch_bounds__(PAD0_T) void k_pad_level0_pitched(uint8_t* slots, const PyrLayout* __restrict__ geom, const PyrPitchEntry* __restrict__ list) {
    const PyrPitchEntry e = list[blockIdx.z];
    pad_level0_rows<GeomEntry&>(slots, geom_entry(geom, e.geom), __builtin_amdgcn_readfirstlane(e.slot), e.src, (size_t)(unsigned)__builtin_amdgcn_readfirstlane((int)e.pitch));
}

// level l-1 (padded) -> level l (padded): cv::pyrDown [1 4 6 4 1]^2, (sum+128)>>8. A workgroup produces PYR_R padded output rows: per
// row the vertical taps straight from coalesced dword loads of the five source rows (source columns -4 .. 2*dw+3: the level origin
// is 4-byte aligned) as packed 16-bit sums into LDS, then the horizontal taps of the dw INTERIOR pixels in packed 16-bit arithmetic
// (every intermediate <= 16 * 4080 + 128 < 2^16), then the padded row as mirrored runs of that interior row (the pyrDown value at a
// REFLECT_101-mapped destination coordinate IS the interior pixel at that coordinate). Integer sums: the order does not matter.
typedef unsigned short pk_u16 __attribute__((ext_vector_type(2)));
__device__ inline pk_u16 as_pk(uint32_t x) { union { uint32_t u; pk_u16 p; } c; c.u = x; return c.p; }
__device__ inline uint32_t as_u32(pk_u16 x) { union { uint32_t u; pk_u16 p; } c; c.p = x; return c.u; }
constexpr int PYR_T = 256, PYR_R = 4;   // output rows per workgroup
__host__ __device__ inline int pyr_vs_row(int dw) { return (2 * dw + 24 + 3) & ~3; }        // uint16 entries
__host__ __device__ inline int pyr_out_row(int dw) { return ((dw + 3 + 24 + 3) / 4) * 4; }  // bytes
// (slot of workgroup column z and LRef as in k_pad_level0; in a list launch a frame whose pyramid has no level ld - 640x200 builds levels
// 0-2, the KITTI sizes 0-3 - is skipped by all its workgroups, again before the first load or barrier)
template <class LRef>
__device__ __forceinline__ void pyrdown_rows(uint8_t* slots, LRef L, int ld, int s) {
    extern __shared__ __attribute__((aligned(16))) uint8_t pyr_lds[];
    if (ld >= L.n_levels) return;
    uint8_t* slot = slots + (size_t)s * L.slot_bytes;
    const int ls = ld - 1;
    const uint8_t* src = level_origin((const uint8_t*)slot, L, ls);
    const int ss = L.stride[ls];
    const int dw = L.w[ld], dh = L.h[ld], ds = L.stride[ld];
    const int ph = dh + 2 * PAD;
    const int py0 = blockIdx.y * PYR_R;
    if (py0 >= ph) return;
    const int nd = (2 * dw + 8) >> 2;
    const int vs_row = pyr_vs_row(dw), out_row = pyr_out_row(dw);
    uint8_t* orow_all = pyr_lds + (size_t)PYR_R * vs_row * 2;
#pragma unroll
    for (int r = 0; r < PYR_R; r++) {
        const int py = py0 + r < ph ? py0 + r : ph - 1;
        const int ry = reflect101(py - PAD, dh);
        const uint8_t* r0 = src + (ptrdiff_t)(2 * ry - 2) * ss - 4;
        uint16_t* vs = (uint16_t*)pyr_lds + r * vs_row;      // vs[c + 4] = vertical sum of source column c
        for (int d = threadIdx.x; d < nd; d += PYR_T) {
            const uint32_t a = *(const uint32_t*)(r0 + 4 * d), b = *(const uint32_t*)(r0 + ss + 4 * d), c = *(const uint32_t*)(r0 + 2 * ss + 4 * d),
                           e = *(const uint32_t*)(r0 + 3 * ss + 4 * d), f = *(const uint32_t*)(r0 + 4 * ss + 4 * d);
            // bytes 0,2 and bytes 1,3 of each row as 16-bit pairs; (a + f) + 4 (b + e) + 6 c <= 4080
            const uint32_t M = 0x00ff00ffu;
            const pk_u16 lo = (as_pk(a & M) + as_pk(f & M)) + (pk_u16)(4) * (as_pk(b & M) + as_pk(e & M)) + (pk_u16)(6) * as_pk(c & M);
            const pk_u16 hi = (as_pk((a >> 8) & M) + as_pk((f >> 8) & M)) + (pk_u16)(4) * (as_pk((b >> 8) & M) + as_pk((e >> 8) & M)) + (pk_u16)(6) * as_pk((c >> 8) & M);
            const uint32_t l = as_u32(lo), hh = as_u32(hi);   // l = (col0, col2), hh = (col1, col3)
            *(uint2*)(vs + 4 * d) = make_uint2((l & 0xffffu) | (hh << 16), (l >> 16) | (hh & 0xffff0000u));
        }
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < PYR_R; r++) {
        // D[j] = (E[j], O[j]) = vertical sums of source columns 2j, 2j+1 = dword j + 2 of the row; output pixel i:
        // E[i-1] + E[i+1] + 4 (O[i-1] + O[i]) + 6 E[i]
        const uint32_t* vsd = (const uint32_t*)((const uint16_t*)pyr_lds + r * vs_row) + 2;
        uint32_t* orow = (uint32_t*)(orow_all + r * out_row);
        for (int i = threadIdx.x * 4; i < dw; i += PYR_T * 4) {
            uint32_t D[7];
#pragma unroll
            for (int q = 0; q < 7; q++) D[q] = vsd[i - 1 + q];   // D[q] = pair i - 1 + q
            uint32_t res[2];
#pragma unroll
            for (int half = 0; half < 2; half++) {
                const int o = 2 * half;   // outputs i + o, i + o + 1
                const pk_u16 Em = as_pk(__builtin_amdgcn_perm(D[o + 1], D[o], 0x05040100u)), E0 = as_pk(__builtin_amdgcn_perm(D[o + 2], D[o + 1], 0x05040100u)),
                             Ep = as_pk(__builtin_amdgcn_perm(D[o + 3], D[o + 2], 0x05040100u));
                const pk_u16 Om = as_pk(__builtin_amdgcn_perm(D[o + 1], D[o], 0x07060302u)), O0 = as_pk(__builtin_amdgcn_perm(D[o + 2], D[o + 1], 0x07060302u));
                const pk_u16 t = ((Em + Ep) + (pk_u16)(4) * (Om + O0) + (pk_u16)(6) * E0 + (pk_u16)(128)) >> (pk_u16)(8);
                res[half] = as_u32(t);   // two bytes in the 16-bit lanes
            }
            orow[i >> 2] = (res[0] & 0xffu) | ((res[0] >> 8) & 0xff00u) | ((res[1] & 0xffu) << 16) | ((res[1] & 0xff0000u) << 8);
        }
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < PYR_R; r++) {
        if (py0 + r >= ph) break;
        write_padded_row<PYR_T>(orow_all + r * out_row, 0, dw, slot + L.off[ld] + (size_t)(py0 + r) * ds);
    }
}
__global__ __launch_bounds__(PYR_T) void k_pyrdown(uint8_t* slots, PyrLayout L, int ld, int first_slot) {
    pyrdown_rows<const PyrLayout&>(slots, L, ld, first_slot + (int)blockIdx.z);
}
__global__ __launch_bounds__(PYR_T) void k_pyrdown_list(uint8_t* slots, const PyrLayout* __restrict__ geom, int ld, const PyrListEntry* __restrict__ list) {
    const PyrListEntry e = list[blockIdx.z];
    pyrdown_rows<GeomEntry&>(slots, geom_entry(geom, e.geom), ld, __builtin_amdgcn_readfirstlane(e.slot));
}

// cv::cvtColor(BGR2GRAY) for 8-bit images (Frame::init, Frame.cpp:40-41): gray = (B * 1868 + G * 9617 + R * 4899 + 8192) >> 14, the 14-bit
// fixed-point form of 0.114 B + 0.587 G + 0.299 R [mem: OpenCV 3.4 color.cpp]; identity for B = G = R (KITTI's gray PNGs, quirk Q2).
// One thread per 4 output pixels: 12 source bytes as three dword loads when the row is 4-byte aligned, byte loads otherwise.
__global__ __launch_bounds__(256) void k_bgr2gray(const uint8_t* __restrict__ bgr, int w, int h, int stride, uint8_t* __restrict__ gray) {
    const int x4 = (blockIdx.x * 256 + threadIdx.x) * 4, y = blockIdx.y;
    if (x4 >= w || y >= h) return;
    const uint8_t* row = bgr + (size_t)y * stride + 3 * (size_t)x4;
    uint8_t out[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        if (x4 + k >= w) { out[k] = 0; continue; }
        const int b = row[3 * k], g = row[3 * k + 1], r = row[3 * k + 2];
        out[k] = (uint8_t)((b * 1868 + g * 9617 + r * 4899 + 8192) >> 14);
    }
    uint8_t* dst = gray + (size_t)y * w + x4;
#pragma unroll
    for (int k = 0; k < 4; k++) if (x4 + k < w) dst[k] = out[k];
}
hipError_t launch_bgr2gray(hipStream_t s, const uint8_t* d_bgr, int w, int h, int stride, uint8_t* d_gray) {
    if (!d_bgr || !d_gray || w < 1 || h < 1 || stride < 3 * w) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_bgr2gray, dim3((w + 1023) / 1024, h), dim3(256), 0, s, d_bgr, w, h, stride, d_gray);
    return hipGetLastError();
}

// Level 0 straight from a COLOUR frame (Frame::Frame / Frame::init, Frame.cpp:33,40-41: imread(IMREAD_COLOR) gives BGR, cvtColor(BGR2GRAY) the
// u8 image everything else works on): k_bgr2gray followed by k_pad_level0 in one pass, no gray frame in HBM in between. The source is tight
// BGR (3 w bytes per row, 3 w h per frame) in the HBM landing area, in mapped pinned host memory at any alignment or in the staging buffer;
// the range and slot-list forms are those of k_pad_level0, except that there is no in-place form (an entry without a source is left alone).
// Per padded output row: the source row as the aligned dwords that hold its 3 w bytes and no others (so a source that ends at the end of a
// host page is never over-read) into LDS, each source byte once; then a thread converts 4 pixels = 12 bytes = the four LDS dwords around them
// (lanes are 3 dwords apart: an odd stride, no bank conflicts) into one dword of the gray LDS row; then write_padded_row as for gray.
// gray = (B * 1868 + G * 9617 + R * 4899 + 8192) >> 14 as two v_dot4_u32_u8 per pixel on the packed (B, G, R, next B) bytes: the weights
// do not fit in 8 bits, so they are split into high and low bytes (1868 = 7 * 256 + 76, 9617 = 37 * 256 + 145, 4899 = 19 * 256 + 35; the
// fourth byte's weight is 0). Integer arithmetic: the bits are those of k_bgr2gray.
constexpr int PAD0C_T = 256, PAD0C_R = 4;   // rows per workgroup: their loads are in flight together (1 for frames too wide for 4 rows of LDS)
constexpr uint32_t BGR_W_HI = 7u | (37u << 8) | (19u << 16), BGR_W_LO = 76u | (145u << 8) | (35u << 16);
static_assert(7 * 256 + 76 == 1868 && 37 * 256 + 145 == 9617 && 19 * 256 + 35 == 4899, "split BGR2GRAY weights");
// bytes of one raw BGR row in LDS: the dwords that hold lead (<= 3) + 3 w bytes, and 16 more so that the last thread's four dwords exist
__host__ __device__ inline int pad0c_raw_lds(int w) { return ((3 + 3 * w + 3) / 4) * 4 + 16; }
__device__ inline uint32_t bgr_gray(uint32_t p) {   // p = B | G << 8 | R << 16 | (any byte) << 24
    return ((__builtin_amdgcn_udot4(p, BGR_W_HI, 0u, false) << 8) + __builtin_amdgcn_udot4(p, BGR_W_LO, 8192u, false)) >> 14;
}
template <int R, class LRef>   // (LRef as in k_pad_level0; `frame`: the BGR source frame, `pitch` bytes from row to row (3 w: tight), both block-uniform)
__device__ __forceinline__ void pad_level0_bgr_rows(uint8_t* slots, LRef L, int s, const uint8_t* __restrict__ frame, size_t pitch) {
    extern __shared__ __attribute__((aligned(16))) uint8_t crow_all[];   // R x raw_lds bytes of BGR, then R x row_lds bytes of gray
    const int w = L.w[0], h = L.h[0], stride = L.stride[0];
    if (!frame) return;
    uint8_t* slot = slots + (size_t)s * L.slot_bytes;
    const int raw_lds = pad0c_raw_lds(w), row_lds = pad0_row_lds(w);
    uint8_t* gray_all = crow_all + R * raw_lds;
    const int ph = h + 2 * PAD;
    const int py0 = blockIdx.y * R;
    if (py0 >= ph) return;
    unsigned lead[R];
    const uint32_t* src[R];
    int nd[R], nd_max = 0;
#pragma unroll
    for (int r = 0; r < R; r++) {
        const int py = py0 + r < ph ? py0 + r : ph - 1;     // (rows past the end repeat the last one; they are not stored)
        const int sy = reflect101(py - PAD, h);
        const uintptr_t a = (uintptr_t)(frame + (size_t)sy * pitch);
        lead[r] = (unsigned)(a & 3u);
        src[r] = (const uint32_t*)(a & ~(uintptr_t)3);
        nd[r] = (int)((lead[r] + 3u * (unsigned)w + 3u) >> 2);   // the aligned dwords that hold the row's bytes and no others
        nd_max = nd[r] > nd_max ? nd[r] : nd_max;
    }
    for (int d = threadIdx.x; d < nd_max; d += PAD0C_T) {   // the loads of the R rows are issued together, then stored
        uint32_t v[R];
#pragma unroll
        for (int r = 0; r < R; r++) v[r] = d < nd[r] ? src[r][d] : 0u;
#pragma unroll
        for (int r = 0; r < R; r++)
            if (d < nd[r]) ((uint32_t*)(crow_all + r * raw_lds))[d] = v[r];
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < R; r++) {
        const uint8_t* raw = crow_all + r * raw_lds;
        uint32_t* grow = (uint32_t*)(gray_all + r * row_lds);
        for (int x4 = threadIdx.x * 4; x4 < w; x4 += PAD0C_T * 4) {
            uint32_t e[3];   // B0 G0 R0 B1 | G1 R1 B2 G2 | R2 B3 G3 R3 (pixels past w: bytes nobody reads, their results land in the row's slack)
            lds_bytes_aligned<12>(raw, (int)lead[r] + 3 * x4, e);
            const uint32_t g0 = bgr_gray(e[0]), g1 = bgr_gray(__builtin_amdgcn_alignbyte(e[1], e[0], 3)),
                           g2 = bgr_gray(__builtin_amdgcn_alignbyte(e[2], e[1], 2)), g3 = bgr_gray(e[2] >> 8);
            grow[x4 >> 2] = g0 | (g1 << 8) | (g2 << 16) | (g3 << 24);
        }
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < R; r++) {
        if (py0 + r >= ph) break;
        write_padded_row<PAD0C_T>(gray_all + r * row_lds, 0, w, slot + L.off[0] + (size_t)(py0 + r) * stride);
    }
}
template <int R>
__global__ __launch_bounds__(PAD0C_T) void k_pad_level0_bgr(uint8_t* slots, PyrLayout L, int first_slot, const uint8_t* __restrict__ tight) {
    pad_level0_bgr_rows<R, const PyrLayout&>(slots, L, first_slot + (int)blockIdx.z, tight ? tight + (size_t)blockIdx.z * 3 * (size_t)L.w[0] * (size_t)L.h[0] : nullptr, 3 * (size_t)L.w[0]);
}
template <int R>
__global__ __launch_bounds__(PAD0C_T) void k_pad_level0_bgr_list(uint8_t* slots, const PyrLayout* __restrict__ geom, const PyrListEntry* __restrict__ list) {
    const PyrListEntry e = list[blockIdx.z];
    GeomEntry& L = geom_entry(geom, e.geom);
    pad_level0_bgr_rows<R, GeomEntry&>(slots, L, __builtin_amdgcn_readfirstlane(e.slot), e.src, 3 * (size_t)L.w[0]);
}
// Pitched list form, as k_pad_level0_pitched: with a pitch that is no multiple of 4 the lead offset differs from row to row (lead[r] above).
template <int R>
__global__ __launch_bounds__(PAD0C_T) void k_pad_level0_bgr_pitched(uint8_t* slots, const PyrLayout* __restrict__ geom, const PyrPitchEntry* __restrict__ list) {
    const PyrPitchEntry e = list[blockIdx.z];
    pad_level0_bgr_rows<R, GeomEntry&>(slots, geom_entry(geom, e.geom), __builtin_amdgcn_readfirstlane(e.slot), e.src, (size_t)(unsigned)__builtin_amdgcn_readfirstlane((int)e.pitch));
}

hipError_t launch_pad_level0(hipStream_t s, uint8_t* slots, const PyrLayout& L, int first_slot, int n, const uint8_t* tight) {
    if (!slots || n < 1 || first_slot < 0 || L.n_levels < 1) return hipErrorInvalidValue;
    dim3 grid(1, (L.h[0] + 2 * PAD + PAD0_R - 1) / PAD0_R, n);
    const size_t shm = (size_t)pad0_row_lds(L.w[0]) * PAD0_R;
    ProfScope ps(K_PAD0, s);
    hipLaunchKernelGGL(k_pad_level0, grid, dim3(PAD0_T), shm, s, slots, L, first_slot, tight);
    return hipGetLastError();
}
// colour form: level 0 of n slots from n tight BGR frames at `tight`
hipError_t launch_pad_level0_bgr(hipStream_t s, uint8_t* slots, const PyrLayout& L, int first_slot, int n, const uint8_t* tight) {
    if (!slots || n < 1 || first_slot < 0 || !tight || L.n_levels < 1) return hipErrorInvalidValue;
    const size_t row = (size_t)pad0c_raw_lds(L.w[0]) + (size_t)pad0_row_lds(L.w[0]);
    const int ph = L.h[0] + 2 * PAD;
    ProfScope ps(K_PAD0_BGR, s);
    if (row * PAD0C_R <= (64u << 10))
        hipLaunchKernelGGL(k_pad_level0_bgr<PAD0C_R>, dim3(1, (ph + PAD0C_R - 1) / PAD0C_R, n), dim3(PAD0C_T), row * PAD0C_R, s, slots, L, first_slot, tight);
    else if (row <= (64u << 10))   // frames wider than 4 k pixels: one row per workgroup
        hipLaunchKernelGGL(k_pad_level0_bgr<1>, dim3(1, ph, n), dim3(PAD0C_T), row, s, slots, L, first_slot, tight);
    else
        return hipErrorInvalidValue;
    return hipGetLastError();
}
hipError_t launch_pyrdown(hipStream_t s, uint8_t* slots, const PyrLayout& L, int ld, int first_slot, int n) {
    if (!slots || n < 1 || first_slot < 0 || ld < 1 || ld >= L.n_levels) return hipErrorInvalidValue;
    dim3 grid(1, (L.h[ld] + 2 * PAD + PYR_R - 1) / PYR_R, n);
    const size_t shm = ((size_t)pyr_vs_row(L.w[ld]) * 2 + (size_t)pyr_out_row(L.w[ld])) * PYR_R;
    ProfScope ps(K_PYRDOWN, s);
    hipLaunchKernelGGL(k_pyrdown, grid, dim3(PYR_T), shm, s, slots, L, ld, first_slot);
    return hipGetLastError();
}
// List forms: n device-visible entries, geometry per entry from the table; grid and dynamic LDS from Lmax (pmv_device.h)
hipError_t launch_pad_level0_list(hipStream_t s, uint8_t* slots, const PyrLayout* d_geom, const PyrLayout& Lmax, const PyrListEntry* list, int n) {
    if (!slots || !d_geom || !list || n < 1 || n > 65535 || Lmax.n_levels < 1) return hipErrorInvalidValue;
    dim3 grid(1, (Lmax.h[0] + 2 * PAD + PAD0_R - 1) / PAD0_R, n);
    const size_t shm = (size_t)pad0_row_lds(Lmax.w[0]) * PAD0_R;
    ProfScope ps(K_PAD0, s);
    hipLaunchKernelGGL(k_pad_level0_list, grid, dim3(PAD0_T), shm, s, slots, d_geom, list);
    return hipGetLastError();
}
hipError_t launch_pad_level0_bgr_list(hipStream_t s, uint8_t* slots, const PyrLayout* d_geom, const PyrLayout& Lmax, const PyrListEntry* list, int n) {
    if (!slots || !d_geom || !list || n < 1 || n > 65535 || Lmax.n_levels < 1) return hipErrorInvalidValue;
    const size_t row = (size_t)pad0c_raw_lds(Lmax.w[0]) + (size_t)pad0_row_lds(Lmax.w[0]);
    const int ph = Lmax.h[0] + 2 * PAD;
    ProfScope ps(K_PAD0_BGR, s);
    if (row * PAD0C_R <= (64u << 10))
        hipLaunchKernelGGL(k_pad_level0_bgr_list<PAD0C_R>, dim3(1, (ph + PAD0C_R - 1) / PAD0C_R, n), dim3(PAD0C_T), row * PAD0C_R, s, slots, d_geom, list);
    else if (row <= (64u << 10))   // frames wider than 4 k pixels: one row per workgroup
        hipLaunchKernelGGL(k_pad_level0_bgr_list<1>, dim3(1, ph, n), dim3(PAD0C_T), row, s, slots, d_geom, list);
    else
        return hipErrorInvalidValue;
    return hipGetLastError();
}
// Pitched list forms: as the two above, every entry with a source and its own row pitch (the caller checks pitch >= w, or 3 w, per entry)
hipError_t launch_pad_level0_pitched(hipStream_t s, uint8_t* slots, const PyrLayout* d_geom, const PyrLayout& Lmax, const PyrPitchEntry* list, int n) {
    if (!slots || !d_geom || !list || n < 1 || n > 65535 || Lmax.n_levels < 1 || Lmax.w[0] < 1 || Lmax.h[0] < 1) return hipErrorInvalidValue;
    dim3 grid(1, (Lmax.h[0] + 2 * PAD + PAD0_R - 1) / PAD0_R, n);
    const size_t shm = (size_t)pad0_row_lds(Lmax.w[0]) * PAD0_R;
    if (shm > (64u << 10)) return hipErrorInvalidValue;
    ProfScope ps(K_PAD0, s);
    hipLaunchKernelGGL(k_pad_level0_pitched, grid, dim3(PAD0_T), shm, s, slots, d_geom, list);
    return hipGetLastError();
}
hipError_t launch_pad_level0_bgr_pitched(hipStream_t s, uint8_t* slots, const PyrLayout* d_geom, const PyrLayout& Lmax, const PyrPitchEntry* list, int n) {
    if (!slots || !d_geom || !list || n < 1 || n > 65535 || Lmax.n_levels < 1 || Lmax.w[0] < 1 || Lmax.h[0] < 1) return hipErrorInvalidValue;
    const size_t row = (size_t)pad0c_raw_lds(Lmax.w[0]) + (size_t)pad0_row_lds(Lmax.w[0]);
    const int ph = Lmax.h[0] + 2 * PAD;
    ProfScope ps(K_PAD0_BGR, s);
    if (row * PAD0C_R <= (64u << 10))
        hipLaunchKernelGGL(k_pad_level0_bgr_pitched<PAD0C_R>, dim3(1, (ph + PAD0C_R - 1) / PAD0C_R, n), dim3(PAD0C_T), row * PAD0C_R, s, slots, d_geom, list);
    else if (row <= (64u << 10))   // frames wider than 4 k pixels: one row per workgroup
        hipLaunchKernelGGL(k_pad_level0_bgr_pitched<1>, dim3(1, ph, n), dim3(PAD0C_T), row, s, slots, d_geom, list);
    else
        return hipErrorInvalidValue;
    return hipGetLastError();
}
hipError_t launch_pyrdown_list(hipStream_t s, uint8_t* slots, const PyrLayout* d_geom, const PyrLayout& Lmax, int ld, const PyrListEntry* list, int n) {
    if (!slots || !d_geom || !list || n < 1 || n > 65535 || ld < 1 || ld >= Lmax.n_levels) return hipErrorInvalidValue;
    dim3 grid(1, (Lmax.h[ld] + 2 * PAD + PYR_R - 1) / PYR_R, n);
    const size_t shm = ((size_t)pyr_vs_row(Lmax.w[ld]) * 2 + (size_t)pyr_out_row(Lmax.w[ld])) * PYR_R;
    ProfScope ps(K_PYRDOWN, s);
    hipLaunchKernelGGL(k_pyrdown_list, grid, dim3(PYR_T), shm, s, slots, d_geom, ld, list);
    return hipGetLastError();
}

// =========================================================================================================
// Pyramidal Lucas–Kanade: one 256-thread block (4 wavefronts) per track, all levels inside one launch.
//   thread = window row (tid >> 3), 4 consecutive columns; its (I, Ix, Iy) samples live in registers for the level.
//   LDS per block: 35x35 u8 tile of the previous image (-> Scharr on the fly, no derivative image in HBM),
//   33x33 (dx,dy) int16 pairs, and a 64x64 u8 search tile of the next image that is re-staged only when the
//   window walks out of it.
// =========================================================================================================
constexpr int SI_STRIDE = 40;   // 40 staged bytes per row: 35 tile columns + up to 3 bytes of dword-alignment slack
constexpr int SD_STRIDE = 33;
constexpr int SJ_STRIDE = 68;

__device__ inline int descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

__device__ inline void bilinear_weights(float a, float b, int& w00, int& w01, int& w10, int& w11) {
    w00 = __float2int_rn((1.f - a) * (1.f - b) * 16384.f);
    w01 = __float2int_rn(a * (1.f - b) * 16384.f);
    w10 = __float2int_rn((1.f - a) * b * 16384.f);
    w11 = 16384 - w00 - w01 - w10;
}

// Block-wide EXACT sums of per-thread int32 partials (4 wavefronts). A wavefront's total leaves wave_sum_i32_exact as a double: every
// sum of these integers stays far below 2^53 (<= 1024 pixels x 8160 x 4080 = 3.4e10), so double addition is exact in any order.
// Each wavefront leaves its total in LDS and after ONE barrier every thread adds the four totals. `slot` alternates between calls that are not separated by another barrier (iteration parity),
// so the next write never overtakes a pending read. (float)(total) rounds the exact integer once, like (float)(int64).
// T = threads per track: 256 (four wavefronts: the shortest chain per track, used when one sequence's ~300 tracks are all there is)
// or 64 (one wavefront: no barrier in the reduction and four times as many tracks resident per CU — the throughput form used by the
// batched launch, where thousands of tracks are in flight). Integer sums are exact, so both give the same bits.
constexpr int LK_T = 256;
// One wavefront's exact sum of int32 partials as a double: the partial is split into its low 16 bits (unsigned) and the rest (signed),
// each half summed with six DPP steps folded into v_add_u32 and read from lane 63 (no half can overflow: 64 x 65535 and
// 64 x 2^15), total = 65536 * H + L, exact in double. The double-precision DPP form this replaces cost 23 dependent vector instructions
// per value (1.4 k clk per LK iteration for two values: a fifth of a track's time in the batched launch).
// The halves of all N values go through each step TOGETHER: 2N independent instructions per step fill the wait states a DPP or swap
// result needs before its next use (one chain after the other spent more slots on s_nop than on adds).
template <int N>
__device__ __forceinline__ void wave_sum_i32_exact(const int (&part)[N], double (&out)[N]) {
    int h[2 * N];
#pragma unroll
    for (int k = 0; k < N; k++) { h[2 * k] = part[k] & 0xffff; h[2 * k + 1] = part[k] >> 16; }
#pragma unroll
    for (int k = 0; k < 2 * N; k++) h[k] += __builtin_amdgcn_update_dpp(0, h[k], 0xB1, 0xf, 0xf, false);    // quad_perm [1,0,3,2]
#pragma unroll
    for (int k = 0; k < 2 * N; k++) h[k] += __builtin_amdgcn_update_dpp(0, h[k], 0x4E, 0xf, 0xf, false);    // quad_perm [2,3,0,1]
#pragma unroll
    for (int k = 0; k < 2 * N; k++) h[k] += __builtin_amdgcn_update_dpp(0, h[k], 0x141, 0xf, 0xf, false);   // row_half_mirror
#pragma unroll
    for (int k = 0; k < 2 * N; k++) h[k] += __builtin_amdgcn_update_dpp(0, h[k], 0x140, 0xf, 0xf, false);   // row_mirror: the 16-lane row's sum in every lane
    // across the four rows: lane 15 of a row into the next row (rows 1 and 3), then lane 31 into rows 2 and 3 - lane 63 holds the total
#pragma unroll
    for (int k = 0; k < 2 * N; k++) h[k] += __builtin_amdgcn_update_dpp(0, h[k], 0x142, 0xa, 0xf, false);   // row_bcast:15
#pragma unroll
    for (int k = 0; k < 2 * N; k++) h[k] += __builtin_amdgcn_update_dpp(0, h[k], 0x143, 0xc, 0xf, false);   // row_bcast:31
#pragma unroll
    for (int k = 0; k < N; k++) out[k] = (double)__builtin_amdgcn_readlane(h[2 * k + 1], 63) * 65536.0 + (double)__builtin_amdgcn_readlane(h[2 * k], 63);
}
template <int N, int T>
__device__ inline void block_sum_exact(const int (&part)[N], double (&out)[N], double* sred /* [2][T/64][4] */, int slot) {
    constexpr int NW = T / 64;
    if (NW == 1) { wave_sum_i32_exact<N>(part, out); return; }
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    double v[N];
    wave_sum_i32_exact<N>(part, v);
#pragma unroll
    for (int k = 0; k < N; k++)
        if (lane == 0) sred[(slot * NW + wv) * 4 + k] = v[k];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < N; k++) {
        double a = sred[(slot * NW + 0) * 4 + k];
#pragma unroll
        for (int w = 1; w < NW; w++) a += sred[(slot * NW + w) * 4 + k];
        out[k] = a;
    }
}

// NB consecutive bytes that start at byte `off` (any alignment) of an LDS row whose base is 4-byte aligned, fetched as aligned dword
// loads and shifted into place: e[j] holds bytes 4j .. 4j+3 of the run. A byte load serves one pixel per LDS instruction; this serves
// four, and with lanes = distinct rows of an odd dword stride the dword loads are free of bank conflicts. `off & 3` must be
// wave-uniform in practice (it is: tile origin + a multiple of 4), but nothing here depends on it.
template <int NB>
__device__ inline void lds_row_bytes(const uint8_t* row, int off, uint32_t (&e)[(NB + 3) / 4]) {
    constexpr int ND = (NB + 3 + 3) / 4, NE = (NB + 3) / 4;
    const uint32_t* w = (const uint32_t*)row + (off >> 2);
    const uint32_t sh = (uint32_t)off & 3u;
    uint32_t d[ND];
#pragma unroll
    for (int j = 0; j < ND; j++) d[j] = w[j];
#pragma unroll
    for (int j = 0; j < NE; j++) e[j] = __builtin_amdgcn_alignbyte(j + 1 < ND ? d[j + 1] : 0u, d[j], sh);
}
#define PACKED_BYTE(e, k) ((int)(((e)[(k) >> 2] >> (((k) & 3) * 8)) & 0xffu))

// Bilinear sample as two packed dot products (v_dot2_i32_i16): the pixel of the upper row and the pixel of the lower row of one column
// share a register as two 16-bit lanes, the weights of that column likewise: w00*p0 + w10*p1 is ONE instruction, the neighbouring
// column adds w01*p0n + w11*p1n. Same integer as the four 24-bit products (|terms| < 2^28).
typedef short pk_s16 __attribute__((ext_vector_type(2)));
__device__ inline pk_s16 as_s16x2(uint32_t x) { union { uint32_t u; pk_s16 p; } c; c.u = x; return c.p; }
__device__ inline uint32_t pack_weights(int lo, int hi) { return ((uint32_t)lo & 0xffffu) | ((uint32_t)hi << 16); }
// column k of two packed byte rows -> (top | bottom << 16)
#define PACKED_COLUMN(top, bot, k) __builtin_amdgcn_perm((bot)[(k) >> 2], (top)[(k) >> 2], 0x0c040c00u | ((uint32_t)((k) & 3) << 16) | (uint32_t)((k) & 3))
__device__ inline int dot2_acc(uint32_t a, uint32_t w, int acc) { return __builtin_amdgcn_sdot2(as_s16x2(a), as_s16x2(w), acc, false); }

// 64x64-byte search tile (stride % 64 == 0, PAD % 4 == 0, tx0 % 4 == 0) in two halves: `tile_issue` starts the global loads (16 bytes
// per lane and load, 256 / T of them) into registers, `tile_commit` writes them to LDS. The caller puts independent work between the
// two - the iterations of the level above - so that the round trip to HBM (7 us per tile in a batched launch, a third of a track's
// time when it was waited for in place) overlaps it.
struct __attribute__((packed, aligned(4))) U4A { uint32_t x, y, z, w; };   // 16 bytes at a 4-byte-aligned address: one global_load_dwordx4
struct __attribute__((packed, aligned(4))) U2A { uint32_t x, y; };
template <int T>
__device__ __forceinline__ void tile_issue(U4A (&reg)[256 / T], const uint8_t* Jorg, int js, int tx0, int ty0, int tid) {
#pragma unroll
    for (int q = 0; q < 256 / T; q++) {
        const int idx = tid + q * T, row = idx >> 2, x4 = idx & 3;
        reg[q] = *(const U4A*)(Jorg + (ptrdiff_t)(ty0 + row) * js + tx0 + 16 * x4);
    }
}
template <int T>
__device__ __forceinline__ void tile_commit(uint8_t* sJ, const U4A (&reg)[256 / T], int tid) {
#pragma unroll
    for (int q = 0; q < 256 / T; q++) {
        const int idx = tid + q * T, row = idx >> 2, x4 = idx & 3;
        uint32_t* d = (uint32_t*)(sJ + row * SJ_STRIDE) + 4 * x4;
        d[0] = reg[q].x; d[1] = reg[q].y; d[2] = reg[q].z; d[3] = reg[q].w;
    }
}
template <int T>
__device__ inline void stage_J(uint8_t* sJ, const uint8_t* Jorg, int js, int tx0, int ty0, int tid) {
    U4A reg[256 / T];
    tile_issue<T>(reg, Jorg, js, tx0, ty0, tid);
    tile_commit<T>(sJ, reg, tid);
}

// One 256-thread block (4 wavefronts) per track: thread = window row (tid >> 3) and 4 consecutive columns ((tid & 7) * 4); its
// (I, Ix, Iy) samples live in registers for the whole level. A single wavefront per track is VALU-issue-bound (2.2 k cycles per
// iteration for 16 pixels per lane); four wavefronts on the four SIMDs of a CU cut the per-iteration chain to 4 pixels per lane
// plus one barrier. All sums are integers (order-free), so the result is bit-identical to the sequential algorithm.
// One track through all pyramid levels; executed by one whole 256-thread block (every thread gets the same results). `stamp_on`:
// this block feeds the diagnostic phase timers.
struct LKResult { float x, y, err; int status, n_iter, n_lev; };
// LRef: const PyrLayout& (k_lk: the launch's by-value geometry) or GeomEntry& (k_lk_batch: the track's entry of the geometry table)
// EX (pmv_lk_track_ex / _fb, the k_lk*_ex kernels): `flags` of LKX_INIT - the top level's search starts at (ix0, iy0) * 2^-level instead of
// the template position - and LKX_EIG - err = the level's minEig, stored before the threshold test, and no final residual.
// `top` (EX only; pmv_lk_track_fb_levels): the walk starts at level min(top, n_levels - 1) instead of the slot's top level, -1 = no cap: cv's
// maxLevel argument on a pyramid that is already built (levels 0 .. top are the same images whatever depth was built).
// The plain instantiations (EX = false) never look at the four arguments: they generate the code they generated without them.
template <int T, bool STAMPS, class LRef, bool EX = false>
__device__ __forceinline__ LKResult lk_track_block(const uint8_t* __restrict__ prevS, const uint8_t* __restrict__ nextS, LRef L,
                                                   const float px0, const float py0, const LKParams& P, const bool stamp_on,
                                                   const float ix0 = 0.f, const float iy0 = 0.f, const int flags = 0, const int top = -1) {
    constexpr int NPRE = 4;                       // I tiles staged per group (all levels of a 4-level pyramid at once)
    constexpr int SI_BYTES = 35 * SI_STRIDE + 8;   // + two dwords: the aligned loads of the last row may touch the first
    __shared__ __attribute__((aligned(16))) uint8_t sIall[NPRE * SI_BYTES];
    __shared__ __attribute__((aligned(16))) short2 sD[33 * SD_STRIDE];
    __shared__ __attribute__((aligned(16))) uint8_t sJ[64 * SJ_STRIDE];
    __shared__ double sred[2 * (T / 64) * 4];
    constexpr int TPR = T / 32, PP = 32 / TPR;   // threads per window row, pixels per thread (256 -> 8 x 4, 64 -> 2 x 16)
    constexpr int NIQ = (35 * 5 + T - 1) / T;     // 8-byte loads per thread of one I tile (35 rows x 40 bytes)
    const int tid = threadIdx.x;
    // 32 consecutive lanes = the 32 window rows of one column group: their LDS rows differ, and with the odd dword strides of sJ (17)
    // and sD (33) they fall into 32 different banks (the sums are exact integers, so the pixel-to-lane assignment is free)
    const int r = tid & 31, c0 = (tid >> 5) * PP;
    const int W = LK_WIN;
    const float half = 15.5f;
    const float FLT_SCALE = 1.f / (1 << 20);
    float outx = 0.f, outy = 0.f, err = 0.f;
    int status = 1;
    int slot = 0;
    int n_iter = 0, n_lev = 0;   // work counters for the roofline's measured OPS_lk
    int ml = L.n_levels - 1;
    if constexpr (EX) { if (top >= 0 && top < ml) ml = top; }   // workgroup-uniform
    unsigned long long t_prev = __builtin_readcyclecounter();
    const unsigned long long wall0 = (STAMPS && P.stamps && stamp_on) ? wall_clock64() : 0ull;   // 100 MHz: calibrates the cycle counter of the stamps
#define LSTAMP(k) do { if (STAMPS && P.stamps && stamp_on && tid == 0) { const unsigned long long t_ = __builtin_readcyclecounter(); atomicAdd(&P.stamps[k], t_ - t_prev); t_prev = t_; } } while (0)

    // where the template window of a level sits: known for every level before anything is tracked (only the search side depends on the
    // level above), so the I tiles of all levels are fetched at once - one round trip to memory instead of one per level
    auto template_origin = [&](int level, float& fx, float& fy, int& ipx, int& ipy) -> bool {
        const float lscale = __int_as_float((127 - level) << 23);   // 2^-level, the value of (float)(1. / (1 << level))
        fx = px0 * lscale - half; fy = py0 * lscale - half;
        ipx = (int)floorf(fx); ipy = (int)floorf(fy);
        return !(ipx < -W || ipx >= L.w[level] || ipy < -W || ipy >= L.h[level]);
    };
    // 35x35 I tiles (rows ipy-1 .. ipy+33, cols ipx-1 .. ipx+33, always inside the padded buffer) of levels top .. top-3 as 8-byte copies
    // of 40-byte rows that start at the 4-byte-aligned column below ipx-1 (35 + 3 <= 40 columns stay inside the 64-pixel frame)
    int tx0 = 0, ty0 = 0, tile_level = -1;   // the search tile in sJ: origin and the level it was cut from
    auto stage_I_group = [&](int top, bool with_search_tile) {
        U2A ireg[NPRE][NIQ];
        U4A jreg[256 / T];
        bool j_ok = false;
#pragma unroll
        for (int g = 0; g < NPRE; g++) {
            const int lv = top - g;
            float fx, fy; int ipx, ipy;
            if (lv < 0 || !template_origin(lv, fx, fy, ipx, ipy)) continue;   // block-uniform
            const uint8_t* Iorg = level_origin(prevS, L, lv);
            const int ls = L.stride[lv], ax0 = (ipx - 1) & ~3;
#pragma unroll
            for (int q = 0; q < NIQ; q++) {
                const int idx = tid + q * T, y = idx / 5, xw = idx - y * 5;
                if (idx < 35 * 5) ireg[g][q] = *(const U2A*)(Iorg + (ptrdiff_t)(ipy - 1 + y) * ls + ax0 + 8 * xw);
            }
        }
        if (with_search_tile) {   // the top level's search starts at the template position: its tile rides along
            float fx, fy; int inx, iny;
            bool first_ok = template_origin(top, fx, fy, inx, iny);
            if constexpr (EX) {
                if (flags & LKX_INIT) {   // ... or at the caller's guess, wherever that lies: the first iteration's own position and bounds test
                    const float lscale = __int_as_float((127 - top) << 23);
                    inx = (int)floorf(ix0 * lscale - half); iny = (int)floorf(iy0 * lscale - half);
                    first_ok = first_ok && !(inx < -W || inx >= L.w[top] || iny < -W || iny >= L.h[top]);
                }
            }
            if (first_ok) {
                tx0 = (inx - 16) & ~3; ty0 = iny - 16;
                tile_issue<T>(jreg, level_origin(nextS, L, top), L.stride[top], tx0, ty0, tid);
                j_ok = true;
            }
        }
#pragma unroll
        for (int g = 0; g < NPRE; g++) {
            const int lv = top - g;
            float fx, fy; int ipx, ipy;
            if (lv < 0 || !template_origin(lv, fx, fy, ipx, ipy)) continue;
            uint8_t* dst = sIall + (lv & (NPRE - 1)) * SI_BYTES;
#pragma unroll
            for (int q = 0; q < NIQ; q++) {
                const int idx = tid + q * T, y = idx / 5, xw = idx - y * 5;
                if (idx < 35 * 5) { uint32_t* d = (uint32_t*)(dst + y * SI_STRIDE) + 2 * xw; d[0] = ireg[g][q].x; d[1] = ireg[g][q].y; }
            }
        }
        if (j_ok) { tile_commit<T>(sJ, jreg, tid); tile_level = top; }
    };
    stage_I_group(ml, true);
    LSTAMP(1);

    for (int level = ml; level >= 0; level--) {
        LSTAMP(0);
        const int lw = L.w[level], lh = L.h[level], ls = L.stride[level];
        const uint8_t* Jorg = level_origin(nextS, L, level);
        __syncthreads();
        if (level != ml && ((ml - level) & (NPRE - 1)) == 0) {   // pyramids deeper than NPRE levels: the next group of template tiles
            stage_I_group(level, false);
            __syncthreads();
            LSTAMP(1);
        }
        const uint8_t* sI = sIall + (level & (NPRE - 1)) * SI_BYTES;
        float prevx, prevy;
        int ipx, ipy;
        const bool inside = template_origin(level, prevx, prevy, ipx, ipy);
        float nx, ny;
        if (level == ml) {
            const float lscale = __int_as_float((127 - level) << 23);
            if (EX && (flags & LKX_INIT)) { nx = ix0 * lscale; ny = iy0 * lscale; }
            else { nx = px0 * lscale; ny = py0 * lscale; }
        }
        else { nx = outx * 2.f; ny = outy * 2.f; }
        outx = nx; outy = ny;
        if (!inside) {   // block-uniform
            if (level == 0) { status = 0; err = 0.f; }
            continue;
        }
        int iw00, iw01, iw10, iw11;
        bilinear_weights(prevx - ipx, prevy - ipy, iw00, iw01, iw10, iw11);
        const int aoff = (ipx - 1) - ((ipx - 1) & ~3);
        // (tile origin (ipx-1, ipy-1) = byte aoff of row 0)
        LSTAMP(1);
        // ---- Scharr (calcSharrDeriv) at the 33x33 sample positions; constant 0 outside the image. Task = (row y, run of SEG columns):
        // three rows of SEG + 2 tile bytes through aligned dword loads, then the 3x3 stencil slides along the run in registers.
        {
            constexpr int SEG = (T >= 256) ? 5 : 11, NSEG = (33 + SEG - 1) / SEG;
            for (int idx = tid; idx < 33 * NSEG; idx += T) {
                const int sg = idx / 33, y = idx - sg * 33, x0 = sg * SEG;
                uint32_t ra[(SEG + 2 + 3) / 4], rb[(SEG + 2 + 3) / 4], rc[(SEG + 2 + 3) / 4];
                lds_row_bytes<SEG + 2>(sI + y * SI_STRIDE, aoff + x0, ra);
                lds_row_bytes<SEG + 2>(sI + (y + 1) * SI_STRIDE, aoff + x0, rb);
                lds_row_bytes<SEG + 2>(sI + (y + 2) * SI_STRIDE, aoff + x0, rc);
                const int gy = ipy + y;
                const bool row_in = gy >= 0 && gy < lh;
                // per tile column: the vertical smoothing 3*(a + c) + 10*b (for d/dx) and the vertical difference c - a (for d/dy) once,
                // then dx = S[x+2] - S[x], dy = 3*(V[x] + V[x+2]) + 10*V[x+1]: the same integers as the 3x3 stencil per pixel
                int S[SEG + 2], V[SEG + 2];
#pragma unroll
                for (int k = 0; k < SEG + 2; k++) {
                    const int a = PACKED_BYTE(ra, k), b = PACKED_BYTE(rb, k), c = PACKED_BYTE(rc, k);
                    S[k] = (a + c) * 3 + b * 10;
                    V[k] = c - a;
                }
#pragma unroll
                for (int k = 0; k < SEG; k++) {
                    const int x = x0 + k;
                    if (x < 33) {
                        const int gx = ipx + x;
                        short2 d = make_short2(0, 0);
                        if (row_in && gx >= 0 && gx < lw) {
                            d.x = (short)(S[k + 2] - S[k]);
                            d.y = (short)((V[k + 2] + V[k]) * 3 + V[k + 1] * 10);
                        }
                        sD[y * SD_STRIDE + x] = d;
                    }
                }
            }
        }
        __syncthreads();
        LSTAMP(2);
        // ---- this thread's PP window samples (I with 5 fractional bits, Ix, Iy) + exact A sums
        // Ix / Iy of two neighbouring pixels share a register as 16-bit halves (|derivative sample| <= 4080): the window sums then take one
        // v_dot2_i32_i16 per pixel PAIR instead of a 24-bit multiply and an add per pixel - the same exact integers
        int Iv[PP];
        uint32_t IxP[PP / 2], IyP[PP / 2];
        int apart[3] = {0, 0, 0};
        {
            uint32_t ia[(PP + 1 + 3) / 4], ib[(PP + 1 + 3) / 4];
            lds_row_bytes<PP + 1>(sI + (r + 1) * SI_STRIDE, aoff + c0 + 1, ia);
            lds_row_bytes<PP + 1>(sI + (r + 2) * SI_STRIDE, aoff + c0 + 1, ib);
            const uint32_t* d0 = (const uint32_t*)&sD[r * SD_STRIDE + c0];   // (dx | dy << 16) per pixel
            const uint32_t W0 = pack_weights(iw00, iw10), W1 = pack_weights(iw01, iw11);   // (upper, lower) weights of a column / of its right neighbour
            uint32_t pc = PACKED_COLUMN(ia, ib, 0);
            uint32_t q0 = d0[0], q1 = d0[SD_STRIDE];
            uint32_t xc = __builtin_amdgcn_perm(q1, q0, 0x05040100u), yc = __builtin_amdgcn_perm(q1, q0, 0x07060302u);   // (upper.dx, lower.dx), (upper.dy, lower.dy)
#pragma unroll
            for (int k = 0; k < PP; k++) {
                const uint32_t pn = PACKED_COLUMN(ia, ib, k + 1);
                const uint32_t q0n = d0[k + 1], q1n = d0[SD_STRIDE + k + 1];
                const uint32_t xn = __builtin_amdgcn_perm(q1n, q0n, 0x05040100u), yn = __builtin_amdgcn_perm(q1n, q0n, 0x07060302u);
                // kept as 256 - 512*I: the accumulator start of the search-side sample, so that (J_sum + 256 - 512*I) >> 9 = descale(J_sum, 9) - I
                // needs neither the rounding constant nor the subtraction per pixel and iteration (512*I is a multiple of 2^9: exact)
                Iv[k] = (1 << 8) - ((dot2_acc(pn, W1, dot2_acc(pc, W0, 1 << 8)) >> 9) << 9);
                const int ixv = dot2_acc(xn, W1, dot2_acc(xc, W0, 1 << 13)) >> 14;
                const int iyv = dot2_acc(yn, W1, dot2_acc(yc, W0, 1 << 13)) >> 14;
                if (k & 1) {
                    IxP[k >> 1] = __builtin_amdgcn_perm((uint32_t)ixv, IxP[k >> 1], 0x05040100u);   // (even pixel | odd pixel << 16)
                    IyP[k >> 1] = __builtin_amdgcn_perm((uint32_t)iyv, IyP[k >> 1], 0x05040100u);
                    apart[0] = dot2_acc(IxP[k >> 1], IxP[k >> 1], apart[0]);
                    apart[1] = dot2_acc(IxP[k >> 1], IyP[k >> 1], apart[1]);
                    apart[2] = dot2_acc(IyP[k >> 1], IyP[k >> 1], apart[2]);
                } else { IxP[k >> 1] = (uint32_t)ixv; IyP[k >> 1] = (uint32_t)iyv; }
                pc = pn; xc = xn; yc = yn;
            }
        }
        double sA[3];
        block_sum_exact<3, T>(apart, sA, sred, slot); slot ^= 1;
        const float A11 = (float)sA[0] * FLT_SCALE, A12 = (float)sA[1] * FLT_SCALE, A22 = (float)sA[2] * FLT_SCALE;
        float D = A11 * A22 - A12 * A12;
        const float minEig = (A22 + A11 - sqrtf((A11 - A22) * (A11 - A22) + 4.f * A12 * A12)) / (2 * W * W);
        if (EX && (flags & LKX_EIG)) err = minEig;
        if (minEig < P.min_eig || D < FLT_EPSILON) {   // block-uniform (computed from block-wide sums)
            if (level == 0) status = 0;
            continue;
        }
        D = 1.f / D;
        LSTAMP(3);
        nx -= half; ny -= half;
        float pdx = 0.f, pdy = 0.f;
        n_lev++;
        // Speculative fetch of the NEXT level's search tile around twice this level's start: the loads fly while this level iterates
        // and are written to LDS after the loop. The iterations of a level move the window by a pixel or two, the 64-pixel tile has
        // 15 pixels of slack on every side; when the guess misses, the loop below re-stages as before - the result never depends on it.
        U4A jreg[256 / T];
        bool pre = false;
        int ptx0 = 0, pty0 = 0;
        if (level > 0) {
            const float gx = (nx + half) * 2.f - half, gy = (ny + half) * 2.f - half;
            const int pinx = (int)floorf(gx), piny = (int)floorf(gy);
            if (!(pinx < -W || pinx >= L.w[level - 1] || piny < -W || piny >= L.h[level - 1])) {
                ptx0 = (pinx - 16) & ~3; pty0 = piny - 16;
                tile_issue<T>(jreg, level_origin(nextS, L, level - 1), L.stride[level - 1], ptx0, pty0, tid);
                pre = true;
            }
        }

        for (int j = 0; j < P.max_iter; j++) {
            const int inx = (int)floorf(nx), iny = (int)floorf(ny);
            if (inx < -W || inx >= lw || iny < -W || iny >= lh) {
                if (level == 0) status = 0;
                break;
            }
            int wx = inx - tx0, wy = iny - ty0;
            if (tile_level != level || wx < 0 || wx > 31 || wy < 0 || wy > 31) {
                tx0 = (inx - 16) & ~3; ty0 = iny - 16;
                __syncthreads();
                stage_J<T>(sJ, Jorg, ls, tx0, ty0, tid);
                __syncthreads();
                tile_level = level;
                wx = inx - tx0; wy = iny - ty0;
                if (STAMPS && P.stamps && stamp_on && tid == 0) atomicAdd(&P.stamps[14], 1ull);   // diagnostic: tiles waited for in place
            }
            LSTAMP(9);
            bilinear_weights(nx - inx, ny - iny, iw00, iw01, iw10, iw11);
            int bpart[2] = {0, 0};
            {
                uint32_t ja[(PP + 1 + 3) / 4], jb[(PP + 1 + 3) / 4];
                lds_row_bytes<PP + 1>(sJ + (wy + r) * SJ_STRIDE, wx + c0, ja);
                lds_row_bytes<PP + 1>(sJ + (wy + r + 1) * SJ_STRIDE, wx + c0, jb);
                const uint32_t W0 = pack_weights(iw00, iw10), W1 = pack_weights(iw01, iw11);
                uint32_t pc = PACKED_COLUMN(ja, jb, 0);
#pragma unroll
                for (int k = 0; k < PP; k += 2) {   // |diff| <= 8160: two of them per register, one dot product per sum and pixel pair
                    const uint32_t p1 = PACKED_COLUMN(ja, jb, k + 1), p2 = PACKED_COLUMN(ja, jb, k + 2);
                    const int diff0 = dot2_acc(p1, W1, dot2_acc(pc, W0, Iv[k])) >> 9;
                    const int diff1 = dot2_acc(p2, W1, dot2_acc(p1, W0, Iv[k + 1])) >> 9;
                    const uint32_t dp = __builtin_amdgcn_perm((uint32_t)diff1, (uint32_t)diff0, 0x05040100u);
                    bpart[0] = dot2_acc(dp, IxP[k >> 1], bpart[0]); bpart[1] = dot2_acc(dp, IyP[k >> 1], bpart[1]);
                    pc = p2;
                }
            }
            LSTAMP(10);
            double sB[2];
            block_sum_exact<2, T>(bpart, sB, sred, slot); slot ^= 1;
            LSTAMP(11);
            const float fb1 = (float)sB[0] * FLT_SCALE, fb2 = (float)sB[1] * FLT_SCALE;
            const float dx = (A12 * fb2 - A22 * fb1) * D;
            const float dy = (A12 * fb1 - A11 * fb2) * D;
            nx += dx; ny += dy;
            outx = nx + half; outy = ny + half;
            n_iter++;
            if (STAMPS && P.stamps && stamp_on && tid == 0) atomicAdd(&P.stamps[8], 1ull);
            if ((double)dx * dx + (double)dy * dy <= P.eps2d) break;
            if (j > 0 && fabsf(dx + pdx) < 0.01 && fabsf(dy + pdy) < 0.01) {
                outx -= dx * 0.5f; outy -= dy * 0.5f;
                break;
            }
            pdx = dx; pdy = dy;
            LSTAMP(12);
        }
        if (pre) {   // block-uniform
            __syncthreads();
            tile_commit<T>(sJ, jreg, tid);
            tx0 = ptx0; ty0 = pty0; tile_level = level - 1;
        }
        LSTAMP(4);

        if (status && level == 0) {
            const float fx = outx - half, fy = outy - half;
            const int inx = (int)floorf(fx), iny = (int)floorf(fy);
            if (inx < -W || inx >= lw || iny < -W || iny >= lh) {
                status = 0;
            } else if (!(EX && (flags & LKX_EIG))) {
                int wx = inx - tx0, wy = iny - ty0;
                if (tile_level != 0 || wx < 0 || wx > 31 || wy < 0 || wy > 31) {
                    tx0 = (inx - 16) & ~3; ty0 = iny - 16;
                    __syncthreads();
                    stage_J<T>(sJ, Jorg, ls, tx0, ty0, tid);
                    __syncthreads();
                    tile_level = 0;
                    wx = inx - tx0; wy = iny - ty0;
                }
                bilinear_weights(fx - inx, fy - iny, iw00, iw01, iw10, iw11);
                int epart[1] = {0};
                uint32_t ja[(PP + 1 + 3) / 4], jb[(PP + 1 + 3) / 4];
                lds_row_bytes<PP + 1>(sJ + (wy + r) * SJ_STRIDE, wx + c0, ja);
                lds_row_bytes<PP + 1>(sJ + (wy + r + 1) * SJ_STRIDE, wx + c0, jb);
                const uint32_t W0 = pack_weights(iw00, iw10), W1 = pack_weights(iw01, iw11);
                uint32_t pc = PACKED_COLUMN(ja, jb, 0);
#pragma unroll
                for (int k = 0; k < PP; k++) {
                    const uint32_t pn = PACKED_COLUMN(ja, jb, k + 1);
                    const int diff = dot2_acc(pn, W1, dot2_acc(pc, W0, Iv[k])) >> 9;
                    epart[0] += diff < 0 ? -diff : diff;
                    pc = pn;
                }
                double sE[1];
                block_sum_exact<1, T>(epart, sE, sred, slot); slot ^= 1;
                err = (float)sE[0] * (1.f / (32 * W * W));
            }
        }
    }
    LSTAMP(5);
    if (STAMPS && P.stamps && stamp_on && tid == 0) atomicAdd(&P.stamps[15], wall_clock64() - wall0);
#undef LSTAMP
    LKResult res;
    res.x = outx; res.y = outy; res.err = err; res.status = status; res.n_iter = n_iter; res.n_lev = n_lev;
    return res;
}

__device__ __forceinline__ void lk_store(const LKResult& r, int t, float* __restrict__ out_xy, uint8_t* __restrict__ out_status,
                                         float* __restrict__ out_err, uint16_t* __restrict__ out_work) {
    if (threadIdx.x == 0) {
        out_xy[2 * t] = r.x; out_xy[2 * t + 1] = r.y;
        out_status[t] = (uint8_t)r.status;
        out_err[t] = r.err;
        if (out_work) out_work[t] = (uint16_t)(r.n_iter | (r.n_lev << 8));   // <= 5 x 30 iterations, <= 5 levels
    }
}

template <bool STAMPS>   // STAMPS: the diagnostic build with phase timers (PMV_LK_STAMPS=1); the product launch carries none of that code
__global__ __launch_bounds__(LK_T) void k_lk(const uint8_t* __restrict__ prevS, const uint8_t* __restrict__ nextS,
                                             PyrLayout L, const float* __restrict__ prev_xy, const int* __restrict__ order, int n, LKParams P,
                                             float* __restrict__ out_xy, uint8_t* __restrict__ out_status,
                                             float* __restrict__ out_err, uint16_t* __restrict__ out_work) {
    const int t = order[blockIdx.x];   // block -> track (XCD-aware order built by the host; -1 = no track)
    if (t < 0 || t >= n) return;
    const LKResult r = lk_track_block<LK_T, STAMPS, const PyrLayout&>(prevS, nextS, L, prev_xy[2 * t], prev_xy[2 * t + 1], P, t == 0);
    lk_store(r, t, out_xy, out_status, out_err, out_work);
}

// Batched form ("same kernels with a leading batch dimension"): the blocks of several independent sequences in one
// launch. blocks[b] = the byte offsets of the track's prev / next frame slots inside `slots`, its position, its index into the
// concatenated result arrays and the index of its frames' geometry in the table `geom` (pmv_device.h): the tracks of one launch may
// belong to sequences of different frame sizes. The index is workgroup-uniform, the table is read with scalar loads.
constexpr int LKB_T = 64;   // one wavefront per track: throughput form (see block_sum_exact)
template <bool STAMPS>
__global__ __launch_bounds__(LKB_T) __attribute__((amdgpu_waves_per_eu(3, 3))) void k_lk_batch(const uint8_t* __restrict__ slots, const LKBlock* __restrict__ blocks,
                                                   int n_blocks, const PyrLayout* __restrict__ geom, LKParams P, float* __restrict__ out_xy,
                                                   uint8_t* __restrict__ out_status, float* __restrict__ out_err, uint16_t* __restrict__ out_work) {
    // grid-stride over the track list: the launcher may cap the grid (PMV_LK_BATCH_BLOCKS) so that the tracks of a round do not occupy
    // every register-file slot of the chip while the short launches of the back-end chains wait for one
    for (int b = blockIdx.x; b < n_blocks; b += gridDim.x) {
        const LKBlock bk = blocks[b];   // (every record is a real track: the host drops padding entries)
        const int2 bt = make_int2(0, bk.track);
        const LKResult r = lk_track_block<LKB_T, STAMPS, GeomEntry&>(slots + bk.prev_off, slots + bk.next_off, geom_entry(geom, bk.geom), bk.x, bk.y, P, (b & 63) == 17);
        if (STAMPS && P.stamps && (b & 63) == 17 && threadIdx.x == 0) atomicAdd(&P.stamps[13], 1ull);   // diagnostic: sampled tracks
        lk_store(r, bt.y, out_xy, out_status, out_err, out_work);   // (out_work: what this track cost - the next launch's ordering hint, and OPS_lk)
        __syncthreads();
    }
}

// ---- the general form: any square window 3 .. 63 (pmv_set_lk_params) ------------------------------------------------------------------
// k_lk / k_lk_batch above are built around 32 window rows: thread = row, samples in registers, tiles of fixed size. A caller's
// cv::calcOpticalFlowPyrLK arguments (OpenCV's default is 21 x 21) go through this form instead. The window side is a RUNTIME value: one
// code object serves all 61 sides, and a round of the batch engine needs no kernel per window. The price is that a lane's samples cannot
// live in registers (their count per lane, ceil(win^2 / T), would have to be a compile-time array bound): I (5 fractional bits) and the
// packed (Ix, Iy) of the window are kept in LDS for the level, next to the tiles.
//   Pixel-to-lane mapping: window pixel p = y * win + x goes to lane p % T, in steps of T (x and y advance incrementally: no division per
//   pixel). Every window sum is an exact integer, so the mapping cannot change a bit.
//   int32 partials: a lane adds at most ceil(63^2 / 64) = 63 products of |diff| <= 8160 and |Ix| <= 4080: 63 * 8160 * 4080 = 2 097 446 400
//   < 2^31 = 2 147 483 648. 64 products would still fit, 65 would not - the window cap of 63 and T >= 64 are what keeps this true
//   (static_assert below). The wave / block totals are formed exactly (wave_sum_i32_exact: doubles) and rounded once to float, like the
//   oracle's (float)int64; that also covers the err sum, which passes 2^24 at win = 63 (3969 * 8160 = 3.2e7).
//   Tiles (LDS, dynamic, sized by win - lkg_lds): the template tile of (win + 3)^2 bytes and the (win + 1)^2 Scharr pairs are dead once the
//   samples are taken, so the search tile of TS x TS bytes (TS = win + 28 rounded up to 16: 64 at win = 32 as in k_lk, 96 at 63) shares
//   their space. It is re-staged when the window walks out of it; its origin is clamped so that it never leaves the padded level buffer
//   (the window itself reaches at most 63 pixels outside the image: one pixel beyond a window of 63 is column w + 63 of a 64-pixel frame).
constexpr int LKG_MIN_WIN = 3, LKG_MAX_WIN = 63;
static_assert((long long)((LKG_MAX_WIN * LKG_MAX_WIN + 63) / 64) * 8160 * 4080 < (1ll << 31), "a lane's int32 partial of diff * Ix at the largest window, one wavefront per track");
struct LKGLds { int si_stride, sd_stride, ts, sj_stride, off_tiles, off_iw, off_dw, total; };
__host__ __device__ inline LKGLds lkg_lds(int win) {
    LKGLds G;
    G.si_stride = ((win + 9) >> 2) << 2;          // the dwords that hold (<= 3 bytes of alignment) + win + 3 tile columns
    G.sd_stride = (win + 1) | 1;                   // (dx, dy) pairs per row: odd
    G.ts = (win + 28 + 15) & ~15;
    G.sj_stride = G.ts + 4;
    const int tmpl = (win + 3) * G.si_stride + (win + 1) * G.sd_stride * 4, srch = G.ts * G.sj_stride;
    G.off_tiles = 2 * 4 * 4 * 8;                   // behind sred[2][<= 4 wavefronts][4] doubles
    G.off_iw = G.off_tiles + (((tmpl > srch ? tmpl : srch) + 3) & ~3);
    G.off_dw = G.off_iw + ((win * win * 2 + 3) & ~3);
    G.total = G.off_dw + win * win * 4;
    return G;
}
// One track through all pyramid levels, executed by one whole T-thread workgroup (T = 256: k_lk_general, T = 64: k_lk_batch_general);
// every thread returns the same results. The arithmetic is orc_lk.cpp:92-209 with W = P.win.
// EX, ix0, iy0, flags, top: as lk_track_block.
template <int T, class LRef, bool EX = false>
__device__ __forceinline__ LKResult lk_track_general(const uint8_t* __restrict__ prevS, const uint8_t* __restrict__ nextS, LRef L,
                                                     const float px0, const float py0, const LKParams& P,
                                                     const float ix0 = 0.f, const float iy0 = 0.f, const int flags = 0, const int top = -1) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lkg_smem[];
    const int W = __builtin_amdgcn_readfirstlane(P.win);
    const LKGLds G = lkg_lds(W);
    double* sred = (double*)lkg_smem;
    uint8_t* sI = lkg_smem + G.off_tiles;
    short2* sD = (short2*)(sI + (W + 3) * G.si_stride);
    uint8_t* sJ = lkg_smem + G.off_tiles;                    // shares the space of sI and sD (see above)
    short* sIw = (short*)(lkg_smem + G.off_iw);
    uint32_t* sDw = (uint32_t*)(lkg_smem + G.off_dw);      // Ix | Iy << 16
    const int tid = threadIdx.x;
    const int npix = W * W, TS = G.ts;
    const int step_y = T / W, step_x = T - step_y * W;       // pixel p + T from pixel p
    const int y_first = tid / W, x_first = tid - y_first * W;
    const int slack = (TS - W - 4) >> 1;                     // search-tile columns left of the window when a tile is cut
    const float half = (float)(W - 1) * 0.5f;
    const float FLT_SCALE = 1.f / (1 << 20);
    float outx = 0.f, outy = 0.f, err = 0.f;
    int status = 1, slot = 0, n_iter = 0, n_lev = 0;
    int ml = L.n_levels - 1;
    if constexpr (EX) { if (top >= 0 && top < ml) ml = top; }   // workgroup-uniform
    int tx0 = 0, ty0 = 0, tile_level = -1;

    for (int level = ml; level >= 0; level--) {
        const int lw = L.w[level], lh = L.h[level], ls = L.stride[level];
        const uint8_t* Iorg = level_origin(prevS, L, level);
        const uint8_t* Jorg = level_origin(nextS, L, level);
        const float lscale = __int_as_float((127 - level) << 23);   // 2^-level, the value of (float)(1. / (1 << level))
        const float prevx = px0 * lscale - half, prevy = py0 * lscale - half;
        const int ipx = (int)floorf(prevx), ipy = (int)floorf(prevy);
        float nx, ny;
        if (level == ml) {
            if (EX && (flags & LKX_INIT)) { nx = ix0 * lscale; ny = iy0 * lscale; }
            else { nx = px0 * lscale; ny = py0 * lscale; }
        }
        else { nx = outx * 2.f; ny = outy * 2.f; }
        outx = nx; outy = ny;
        if (ipx < -W || ipx >= lw || ipy < -W || ipy >= lh) {   // block-uniform
            if (level == 0) { status = 0; err = 0.f; }
            continue;
        }
        // search tile of level `level` with the window origin (inx, iny) `slack` pixels inside, clamped into the padded buffer: columns
        // -PAD .. stride - PAD - 1 and rows -PAD .. lh + PAD - 1 exist (stride >= lw + 2 PAD, a multiple of 64; TS <= 96 <= 2 PAD, so
        // the upper clamp is never below the lower one). A window origin in -W .. lw - 1 keeps its W + 1 columns inside either way.
        auto stage_search = [&](int inx, int iny) {
            int x0 = (inx - slack) & ~3, y0 = iny - slack;
            x0 = x0 < -PAD ? -PAD : x0; x0 = x0 > ls - PAD - TS ? ls - PAD - TS : x0;
            y0 = y0 < -PAD ? -PAD : y0; y0 = y0 > lh + PAD - TS ? lh + PAD - TS : y0;
            tx0 = x0; ty0 = y0; tile_level = level;
            const int per_row = TS >> 4;
            __syncthreads();
            for (int idx = tid; idx < TS * per_row; idx += T) {
                const int row = idx / per_row, x16 = idx - row * per_row;
                const U4A v = *(const U4A*)(Jorg + (ptrdiff_t)(y0 + row) * ls + x0 + 16 * x16);
                uint32_t* d = (uint32_t*)(sJ + row * G.sj_stride) + 4 * x16;
                d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
            }
            __syncthreads();
        };
        auto in_tile = [&](int inx, int iny) {
            const int wx = inx - tx0, wy = iny - ty0;
            return tile_level == level && wx >= 0 && wy >= 0 && wx + W + 1 <= TS && wy + W + 1 <= TS;
        };
        __syncthreads();   // the level above is done with the search tile, whose space the template tile takes
        tile_level = -1;
        // ---- template tile: rows ipy - 1 .. ipy + W + 1, columns ipx - 1 .. ipx + W + 1 (>= -PAD and <= lw + PAD - 1 for W <= 63), as the
        // aligned dwords that hold them and no others
        const int ax0 = (ipx - 1) & ~3, aoff = (ipx - 1) - ax0;
        {
            const int ndw = (aoff + W + 3 + 3) >> 2;   // <= si_stride / 4
            for (int idx = tid; idx < (W + 3) * ndw; idx += T) {
                const int y = idx / ndw, d = idx - y * ndw;
                ((uint32_t*)(sI + y * G.si_stride))[d] = *(const uint32_t*)(Iorg + (ptrdiff_t)(ipy - 1 + y) * ls + ax0 + 4 * d);
            }
        }
        __syncthreads();
        // ---- Scharr (calcSharrDeriv) at the (W + 1)^2 sample positions: REFLECT_101 inside the image comes with the padded buffer, constant 0
        // outside the image
        for (int idx = tid; idx < (W + 1) * (W + 1); idx += T) {
            const int y = idx / (W + 1), x = idx - y * (W + 1);
            const int gx = ipx + x, gy = ipy + y;
            short2 d = make_short2(0, 0);
            if (gx >= 0 && gx < lw && gy >= 0 && gy < lh) {
                const uint8_t* a = sI + y * G.si_stride + aoff + x;
                const uint8_t* b = a + G.si_stride;
                const uint8_t* c = b + G.si_stride;
                const int S0 = (a[0] + c[0]) * 3 + b[0] * 10, S2 = (a[2] + c[2]) * 3 + b[2] * 10;
                const int V0 = c[0] - a[0], V1 = c[1] - a[1], V2 = c[2] - a[2];
                d.x = (short)(S2 - S0);
                d.y = (short)((V2 + V0) * 3 + V1 * 10);
            }
            sD[y * G.sd_stride + x] = d;
        }
        __syncthreads();
        // ---- window samples (I with 5 fractional bits, Ix, Iy) into LDS + exact A sums
        int iw00, iw01, iw10, iw11;
        bilinear_weights(prevx - ipx, prevy - ipy, iw00, iw01, iw10, iw11);
        int apart[3] = {0, 0, 0};
        for (int p = tid, x = x_first, y = y_first; p < npix; p += T) {
            const uint8_t* i0 = sI + (y + 1) * G.si_stride + aoff + x + 1;
            const uint8_t* i1 = i0 + G.si_stride;
            const short2 d00 = sD[y * G.sd_stride + x], d01 = sD[y * G.sd_stride + x + 1], d10 = sD[(y + 1) * G.sd_stride + x], d11 = sD[(y + 1) * G.sd_stride + x + 1];
            const int iv = descale(i0[0] * iw00 + i0[1] * iw01 + i1[0] * iw10 + i1[1] * iw11, 9);
            const int ixv = descale(d00.x * iw00 + d01.x * iw01 + d10.x * iw10 + d11.x * iw11, 14);
            const int iyv = descale(d00.y * iw00 + d01.y * iw01 + d10.y * iw10 + d11.y * iw11, 14);
            sIw[p] = (short)iv;
            sDw[p] = ((uint32_t)ixv & 0xffffu) | ((uint32_t)iyv << 16);
            apart[0] += ixv * ixv; apart[1] += ixv * iyv; apart[2] += iyv * iyv;   // <= 63 x 4080^2 per lane
            x += step_x; y += step_y;
            if (x >= W) { x -= W; y++; }
        }
        double sA[3];
        block_sum_exact<3, T>(apart, sA, sred, slot); slot ^= 1;
        const float A11 = (float)sA[0] * FLT_SCALE, A12 = (float)sA[1] * FLT_SCALE, A22 = (float)sA[2] * FLT_SCALE;
        float D = A11 * A22 - A12 * A12;
        const float minEig = (A22 + A11 - sqrtf((A11 - A22) * (A11 - A22) + 4.f * A12 * A12)) / (float)(2 * W * W);
        if (EX && (flags & LKX_EIG)) err = minEig;
        if (minEig < P.min_eig || D < FLT_EPSILON) {   // block-uniform (computed from block-wide sums)
            if (level == 0) status = 0;
            continue;
        }
        D = 1.f / D;
        nx -= half; ny -= half;
        float pdx = 0.f, pdy = 0.f;
        n_lev++;
        // sum over the window of f(diff, Ix | Iy << 16) with diff = the search-side sample at window origin (wx, wy) of the tile minus I
        auto window_pass = [&](int wx, int wy, auto&& f) {
            for (int p = tid, x = x_first, y = y_first; p < npix; p += T) {
                const uint8_t* j0 = sJ + (wy + y) * G.sj_stride + wx + x;
                const uint8_t* j1 = j0 + G.sj_stride;
                const int diff = descale(j0[0] * iw00 + j0[1] * iw01 + j1[0] * iw10 + j1[1] * iw11, 9) - sIw[p];
                f(diff, sDw[p]);
                x += step_x; y += step_y;
                if (x >= W) { x -= W; y++; }
            }
        };
        for (int j = 0; j < P.max_iter; j++) {
            const int inx = (int)floorf(nx), iny = (int)floorf(ny);
            if (inx < -W || inx >= lw || iny < -W || iny >= lh) {
                if (level == 0) status = 0;
                break;
            }
            if (!in_tile(inx, iny)) stage_search(inx, iny);   // block-uniform
            bilinear_weights(nx - inx, ny - iny, iw00, iw01, iw10, iw11);
            int bpart[2] = {0, 0};
            window_pass(inx - tx0, iny - ty0, [&](int diff, uint32_t d) { bpart[0] += diff * (int)(short)(d & 0xffffu); bpart[1] += diff * ((int)d >> 16); });
            double sB[2];
            block_sum_exact<2, T>(bpart, sB, sred, slot); slot ^= 1;
            const float fb1 = (float)sB[0] * FLT_SCALE, fb2 = (float)sB[1] * FLT_SCALE;
            const float dx = (A12 * fb2 - A22 * fb1) * D;
            const float dy = (A12 * fb1 - A11 * fb2) * D;
            nx += dx; ny += dy;
            outx = nx + half; outy = ny + half;
            n_iter++;
            if ((double)dx * dx + (double)dy * dy <= P.eps2d) break;
            if (j > 0 && fabsf(dx + pdx) < 0.01 && fabsf(dy + pdy) < 0.01) {
                outx -= dx * 0.5f; outy -= dy * 0.5f;
                break;
            }
            pdx = dx; pdy = dy;
        }
        if (status && level == 0) {
            const float fx = outx - half, fy = outy - half;
            const int inx = (int)floorf(fx), iny = (int)floorf(fy);
            if (inx < -W || inx >= lw || iny < -W || iny >= lh) {
                status = 0;
            } else if (!(EX && (flags & LKX_EIG))) {
                if (!in_tile(inx, iny)) stage_search(inx, iny);
                bilinear_weights(fx - inx, fy - iny, iw00, iw01, iw10, iw11);
                int epart[1] = {0};
                window_pass(inx - tx0, iny - ty0, [&](int diff, uint32_t) { epart[0] += diff < 0 ? -diff : diff; });
                double sE[1];
                block_sum_exact<1, T>(epart, sE, sred, slot); slot ^= 1;
                err = (float)sE[0] * (1.f / (float)(32 * W * W));
            }
        }
    }
    LKResult res;
    // the per-track work word has 8 bits for the iterations (lk_store): up to 5 x 100 here, so the count saturates
    res.x = outx; res.y = outy; res.err = err; res.status = status; res.n_iter = n_iter > 255 ? 255 : n_iter; res.n_lev = n_lev;
    return res;
}

__global__ __launch_bounds__(LK_T) void k_lk_general(const uint8_t* __restrict__ prevS, const uint8_t* __restrict__ nextS, PyrLayout L,
                                                     const float* __restrict__ prev_xy, const int* __restrict__ order, int n, LKParams P,
                                                     float* __restrict__ out_xy, uint8_t* __restrict__ out_status, float* __restrict__ out_err,
                                                     uint16_t* __restrict__ out_work) {
    const int t = order[blockIdx.x];   // as k_lk
    if (t < 0 || t >= n) return;
    const LKResult r = lk_track_general<LK_T, const PyrLayout&>(prevS, nextS, L, prev_xy[2 * t], prev_xy[2 * t + 1], P);
    lk_store(r, t, out_xy, out_status, out_err, out_work);
}
__global__ __launch_bounds__(LKB_T) void k_lk_batch_general(const uint8_t* __restrict__ slots, const LKBlock* __restrict__ blocks, int n_blocks,
                                                            const PyrLayout* __restrict__ geom, LKParams P, float* __restrict__ out_xy,
                                                            uint8_t* __restrict__ out_status, float* __restrict__ out_err, uint16_t* __restrict__ out_work) {
    for (int b = blockIdx.x; b < n_blocks; b += gridDim.x) {   // as k_lk_batch
        const LKBlock bk = blocks[b];
        const LKResult r = lk_track_general<LKB_T, GeomEntry&>(slots + bk.prev_off, slots + bk.next_off, geom_entry(geom, bk.geom), bk.x, bk.y, P);
        lk_store(r, bk.track, out_xy, out_status, out_err, out_work);
        __syncthreads();
    }
}
// ---- the extended calls (pmv_lk_track_ex, pmv_lk_track_fb and their session forms) -----------------------------------------------------
// The same two device functions with EX = true: an initial flow, minEig as the error measure, and - LKX_FB - the forward-backward check as a
// mode: the workgroup that took the track forward takes the result back into the first frame, slot pointers swapped, the original position
// as its initial flow. ONE call site of the tracker in a two-trip loop; the second trip is a workgroup-uniform decision (flags and the
// forward status are the same in every lane). A track whose forward status is 0 makes no second trip: back status 0, back err 0, back
// position = the bits of its forward position. top_f / top_b: the level cap (`top` of the two device functions) of the forward and of the
// backward trip; -1 = the slot's top level. pred_slot / pred_mode (a predicted tracker step, pmv_device.h: LKP_*): the (successes, successes
// wanted) pair O.pred[2 slot ..] - a gated workgroup reads it before anything else and leaves when the first pass had successes enough (the
// same words in every lane: a workgroup-uniform decision, like the count of k_lk_ex_dev); a counting one adds its forward status, an integer
// atomic by one lane, whose sum does not depend on the order of the workgroups.
struct LKExOut { float* xy; uint8_t* status; float* err; uint16_t* work; float* back_xy; uint8_t* back_status; float* back_err; int* pred; int n_pred; };
__device__ __forceinline__ float uniform_f32(float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); }
template <int T, bool GENERAL, class LRef>
__device__ __forceinline__ void lk_track_ex(const uint8_t* a, const uint8_t* b, LRef L, float px, float py, float ix, float iy, int flags,
                                            const LKParams& P, const int t, const LKExOut& O, const int top_f = -1, const int top_b = -1,
                                            const int pred_slot = -1, const int pred_mode = LKP_NONE) {
    const bool pred_on = pred_mode != LKP_NONE && O.pred && pred_slot >= 0 && pred_slot < O.n_pred;   // (a slot outside the table serves nobody)
    if (pred_on && pred_mode == LKP_GATE) {
        const int* const g = O.pred + 2 * pred_slot;
        if (__builtin_amdgcn_readfirstlane(g[0]) >= __builtin_amdgcn_readfirstlane(g[1])) return;
    }
    const bool fb = (flags & LKX_FB) != 0;
    int n_iter = 0, n_lev = 0, top = top_f;
#pragma nounroll
    for (int trip = 0; trip < 2; trip++) {
        LKResult r;
        if constexpr (GENERAL) r = lk_track_general<T, LRef, true>(a, b, L, px, py, P, ix, iy, flags, top);
        else r = lk_track_block<T, false, LRef, true>(a, b, L, px, py, P, false, ix, iy, flags, top);
        n_iter += r.n_iter; n_lev += r.n_lev;
        if (trip == 1) {
            if (threadIdx.x == 0) { O.back_xy[2 * t] = r.x; O.back_xy[2 * t + 1] = r.y; O.back_status[t] = (uint8_t)r.status; O.back_err[t] = r.err; }
            break;
        }
        if (threadIdx.x == 0) {
            O.xy[2 * t] = r.x; O.xy[2 * t + 1] = r.y; O.status[t] = (uint8_t)r.status; O.err[t] = r.err;
            if (fb && !r.status) { O.back_xy[2 * t] = r.x; O.back_xy[2 * t + 1] = r.y; O.back_status[t] = 0; O.back_err[t] = 0.f; }
            if (pred_on && pred_mode == LKP_COUNT && r.status) atomicAdd(O.pred + 2 * pred_slot, 1);
        }
        if (!fb || !r.status) break;   // workgroup-uniform
        const uint8_t* const a0 = a; a = b; b = a0;
        ix = px; iy = py; px = r.x; py = r.y;
        flags = LKX_INIT | (flags & LKX_EIG);
        top = top_b;
        __syncthreads();   // the forward trip is done with the tiles
    }
    // both directions in the track's one work word: 8 bits of iterations (saturating), <= 10 level passes
    if (threadIdx.x == 0 && O.work) O.work[t] = (uint16_t)((n_iter > 255 ? 255 : n_iter) | (n_lev << 8));
}
// init_xy is read only with LKX_INIT; back_* only written with LKX_FB
template <bool GENERAL>
__global__ __launch_bounds__(LK_T) void k_lk_ex(const uint8_t* __restrict__ prevS, const uint8_t* __restrict__ nextS, PyrLayout L,
                                                const float* __restrict__ prev_xy, const float* __restrict__ init_xy, const int* __restrict__ order,
                                                int n, int flags, LKParams P, LKExOut O, int top_f, int top_b, int pred_mode) {
    const int t = order[blockIdx.x];   // as k_lk
    if (t < 0 || t >= n) return;
    float ix = 0.f, iy = 0.f;
    if (flags & LKX_INIT) { ix = init_xy[2 * t]; iy = init_xy[2 * t + 1]; }
    lk_track_ex<LK_T, GENERAL, const PyrLayout&>(prevS, nextS, L, uniform_f32(prev_xy[2 * t]), uniform_f32(prev_xy[2 * t + 1]), uniform_f32(ix), uniform_f32(iy), flags, P, t, O, top_f, top_b, 0, pred_mode);
}
// the device-counted form (stage 8 of a stereo KLT step): the launch is sized by a bound n_cap, the count is a word an earlier kernel of the
// chain left in device memory. Identity order, no initial flow; a block at or beyond the count leaves before it touches LDS or the frames.
template <bool GENERAL>
__global__ __launch_bounds__(LK_T) void k_lk_ex_dev(const uint8_t* __restrict__ prevS, const uint8_t* __restrict__ nextS, PyrLayout L,
                                                    const float* __restrict__ prev_xy, const int* __restrict__ n_dev, int n_cap, int flags, LKParams P, LKExOut O) {
    const int t = blockIdx.x, n = __builtin_amdgcn_readfirstlane(*n_dev);
    if (t >= n || t >= n_cap) return;   // (a negative count serves nobody)
    lk_track_ex<LK_T, GENERAL, const PyrLayout&>(prevS, nextS, L, uniform_f32(prev_xy[2 * t]), uniform_f32(prev_xy[2 * t + 1]), 0.f, 0.f, flags, P, t, O);
}
// the batched form: ext[b] belongs to blocks[b]
template <bool GENERAL>
__global__ __launch_bounds__(LKB_T) void k_lk_batch_ex(const uint8_t* __restrict__ slots, const LKBlock* __restrict__ blocks, const LKExt* __restrict__ ext,
                                                       int n_blocks, const PyrLayout* __restrict__ geom, LKParams P, LKExOut O) {
    for (int b = blockIdx.x; b < n_blocks; b += gridDim.x) {   // as k_lk_batch
        const LKBlock bk = blocks[b];
        const LKExt ex = ext[b];
        if (__builtin_amdgcn_readfirstlane(ex.flags) & LKX_VOID) continue;   // workgroup-uniform: a record beyond its list's device-side count
        const int opt = __builtin_amdgcn_readfirstlane(ex.opt);   // lkext_opt(..): 0 = no cap, no pair
        lk_track_ex<LKB_T, GENERAL, GeomEntry&>(slots + bk.prev_off, slots + bk.next_off, geom_entry(geom, bk.geom), uniform_f32(bk.x), uniform_f32(bk.y),
                                                uniform_f32(ex.ix), uniform_f32(ex.iy), __builtin_amdgcn_readfirstlane(ex.flags), P,
                                                __builtin_amdgcn_readfirstlane(bk.track), O, (opt & 15) - 1, ((opt >> 4) & 15) - 1, ((opt >> 8) & 0xfffff) - 1,
                                                (opt >> 28) & 3);
        __syncthreads();
    }
}
// which form a launch takes: the tuned kernels serve the window they were built for unless the diagnostic asks for the general form
static bool lk_use_general(const LKParams& P) { return P.win != LK_WIN || P.general; }
static bool lk_params_ok(const LKParams& P) {
    return P.win >= LKG_MIN_WIN && P.win <= LKG_MAX_WIN && P.max_iter >= 1 && P.eps2d >= 0.0 && P.min_eig >= 0.f && lkg_lds(P.win).total <= (64 << 10);
}

hipError_t launch_lk(hipStream_t s, const uint8_t* prev_slot, const uint8_t* next_slot, const PyrLayout& L,
                     const float* d_prev_xy, const int* d_order, int n_blocks, int n, const LKParams& P, float* d_out_xy,
                     uint8_t* d_status, float* d_err, uint16_t* d_work) {
    if (n <= 0) return hipSuccess;
    if (lk_use_general(P)) {
        if (!prev_slot || !next_slot || !d_prev_xy || !d_order || !d_out_xy || !d_status || !d_err || n_blocks < n || L.n_levels < 1 || L.n_levels > MAX_LEVELS || !lk_params_ok(P)) return hipErrorInvalidValue;
        ProfScope ps(K_LK, s);
        hipLaunchKernelGGL(k_lk_general, dim3(n_blocks), dim3(LK_T), (size_t)lkg_lds(P.win).total, s, prev_slot, next_slot, L, d_prev_xy, d_order, n, P, d_out_xy, d_status, d_err, d_work);
        return hipGetLastError();
    }
    // every pointer the kernel dereferences: a null base must come back as an error code, never reach a launch
    if (!prev_slot || !next_slot || !d_prev_xy || !d_order || !d_out_xy || !d_status || !d_err || n_blocks < n || L.n_levels < 1 || L.n_levels > MAX_LEVELS) return hipErrorInvalidValue;
    ProfScope ps(K_LK, s);
    if (P.stamps) hipLaunchKernelGGL(k_lk<true>, dim3(n_blocks), dim3(LK_T), 0, s, prev_slot, next_slot, L, d_prev_xy, d_order, n, P, d_out_xy, d_status, d_err, d_work);
    else hipLaunchKernelGGL(k_lk<false>, dim3(n_blocks), dim3(LK_T), 0, s, prev_slot, next_slot, L, d_prev_xy, d_order, n, P, d_out_xy, d_status, d_err, d_work);
    return hipGetLastError();
}

hipError_t launch_lk_batch(hipStream_t s, const uint8_t* slots, const LKBlock* d_blocks, int n_blocks, const PyrLayout* d_geom,
                           const LKParams& P, float* d_out_xy, uint8_t* d_status, float* d_err, uint16_t* d_work) {
    if (n_blocks <= 0) return hipSuccess;
    if (!slots || !d_blocks || !d_out_xy || !d_status || !d_err || !d_geom) return hipErrorInvalidValue;
    static const int cap = getenv("PMV_LK_BATCH_BLOCKS") ? atoi(getenv("PMV_LK_BATCH_BLOCKS")) : 0;
    if (lk_use_general(P)) {   // (its own LDS, 6 .. 46 KB by window, already bounds the workgroups per CU: no padding on top)
        if (!lk_params_ok(P)) return hipErrorInvalidValue;
        ProfScope ps(K_LK, s);
        hipLaunchKernelGGL(k_lk_batch_general, dim3(cap > 0 && cap < n_blocks ? cap : n_blocks), dim3(LKB_T), (size_t)lkg_lds(P.win).total, s, slots, d_blocks, n_blocks, d_geom, P,
                           d_out_xy, d_status, d_err, d_work);
        return hipGetLastError();
    }
    // Occupancy cap of the bulk kernel: 13.9 KB of LDS per one-wavefront workgroup lets 11 of them share a CU (160 KB; the prefetch
    // registers of a track, ~150 per lane, allow 12), and then every short kernel of the other classes - the 23 launches of an LM solve,
    // the PnP stages, the detector - waits for LK wavefronts to drain before its workgroups fit anywhere. Unused dynamic LDS on top caps it:
    // 5 000 B = 8 per CU. B = 192, same box, profiles/r03_batch_exp_ae/af.log (after the per-track atomics were gone, which had made
    // the cap look far more valuable than it is: with them every extra resident wavefront was one more contender for three L2 lines):
    // no cap 64.8 k, 2 000 B 63.4 k, 3 000 B 65.6 k, 4 000 B 62.7-68.7 k, 5 000 B 69.0 k, 6 500 B 68.3 k frames/s (run-to-run spread of one
    // setting: +-3 k). PMV_LK_LDS_PAD overrides (0 = no cap).
    static const int lds_pad = getenv("PMV_LK_LDS_PAD") ? atoi(getenv("PMV_LK_LDS_PAD")) : 5000;
    ProfScope ps(K_LK, s);
    const dim3 grid(cap > 0 && cap < n_blocks ? cap : n_blocks);
    const size_t pad = (size_t)(lds_pad > 0 ? lds_pad : 0);
    if (P.stamps) hipLaunchKernelGGL(k_lk_batch<true>, grid, dim3(LKB_T), pad, s, slots, d_blocks, n_blocks, d_geom, P, d_out_xy, d_status, d_err, d_work);
    else hipLaunchKernelGGL(k_lk_batch<false>, grid, dim3(LKB_T), pad, s, slots, d_blocks, n_blocks, d_geom, P, d_out_xy, d_status, d_err, d_work);
    return hipGetLastError();
}

static bool lk_ex_args_ok(int flags, const float* d_xy, const uint8_t* d_status, const float* d_err, const float* d_back_xy, const uint8_t* d_back_status, const float* d_back_err) {
    return !(flags & ~(LKX_INIT | LKX_EIG | LKX_FB)) && d_xy && d_status && d_err && (!(flags & LKX_FB) || (d_back_xy && d_back_status && d_back_err));
}
hipError_t launch_lk_ex(hipStream_t s, const uint8_t* prev_slot, const uint8_t* next_slot, const PyrLayout& L, const float* d_prev_xy, const float* d_init_xy,
                        const int* d_order, int n_blocks, int n, int flags, const LKParams& P, float* d_out_xy, uint8_t* d_status, float* d_err, uint16_t* d_work,
                        float* d_back_xy, uint8_t* d_back_status, float* d_back_err, int top_f, int top_b, int* d_pred, int pred_mode) {
    if (n <= 0) return hipSuccess;
    if (!prev_slot || !next_slot || !d_prev_xy || !d_order || n_blocks < n || L.n_levels < 1 || L.n_levels > MAX_LEVELS || ((flags & LKX_INIT) && !d_init_xy) ||
        top_f < -1 || top_f >= MAX_LEVELS || top_b < -1 || top_b >= MAX_LEVELS || pred_mode < LKP_NONE || pred_mode > LKP_GATE || (pred_mode != LKP_NONE && !d_pred) ||
        !lk_ex_args_ok(flags, d_out_xy, d_status, d_err, d_back_xy, d_back_status, d_back_err)) return hipErrorInvalidValue;
    const LKExOut O{d_out_xy, d_status, d_err, d_work, d_back_xy, d_back_status, d_back_err, d_pred, d_pred ? 1 : 0};
    if (lk_use_general(P)) {
        if (!lk_params_ok(P)) return hipErrorInvalidValue;
        ProfScope ps(K_LK, s);
        hipLaunchKernelGGL(k_lk_ex<true>, dim3(n_blocks), dim3(LK_T), (size_t)lkg_lds(P.win).total, s, prev_slot, next_slot, L, d_prev_xy, d_init_xy, d_order, n, flags, P, O, top_f, top_b, pred_mode);
        return hipGetLastError();
    }
    ProfScope ps(K_LK, s);
    hipLaunchKernelGGL(k_lk_ex<false>, dim3(n_blocks), dim3(LK_T), 0, s, prev_slot, next_slot, L, d_prev_xy, d_init_xy, d_order, n, flags, P, O, top_f, top_b, pred_mode);
    return hipGetLastError();
}
hipError_t launch_lk_ex_dev(hipStream_t s, const uint8_t* prev_slot, const uint8_t* next_slot, const PyrLayout& L, const float* d_prev_xy, const int* d_n, int n_cap,
                            int flags, const LKParams& P, float* d_out_xy, uint8_t* d_status, float* d_err, float* d_back_xy, uint8_t* d_back_status, float* d_back_err) {
    if (n_cap <= 0) return hipSuccess;
    if (!prev_slot || !next_slot || !d_prev_xy || !d_n || L.n_levels < 1 || L.n_levels > MAX_LEVELS || (flags & ~LKX_FB) ||
        !lk_ex_args_ok(flags, d_out_xy, d_status, d_err, d_back_xy, d_back_status, d_back_err)) return hipErrorInvalidValue;
    const bool general = lk_use_general(P);
    if (general && !lk_params_ok(P)) return hipErrorInvalidValue;
    const LKExOut O{d_out_xy, d_status, d_err, nullptr, d_back_xy, d_back_status, d_back_err, nullptr, 0};
    ProfScope ps(K_LK, s);
    if (general) {
        hipLaunchKernelGGL(k_lk_ex_dev<true>, dim3(n_cap), dim3(LK_T), (size_t)lkg_lds(P.win).total, s, prev_slot, next_slot, L, d_prev_xy, d_n, n_cap, flags, P, O);
    } else hipLaunchKernelGGL(k_lk_ex_dev<false>, dim3(n_cap), dim3(LK_T), 0, s, prev_slot, next_slot, L, d_prev_xy, d_n, n_cap, flags, P, O);
    return hipGetLastError();
}
hipError_t launch_lk_batch_ex(hipStream_t s, const uint8_t* slots, const LKBlock* d_blocks, const LKExt* d_ext, int n_blocks, const PyrLayout* d_geom, const LKParams& P,
                              float* d_out_xy, uint8_t* d_status, float* d_err, uint16_t* d_work, float* d_back_xy, uint8_t* d_back_status, float* d_back_err,
                              int* d_pred, int n_pred) {
    if (n_blocks <= 0) return hipSuccess;
    // (the records carry the flags: a launch that may hold LKX_FB records needs the three back arrays)
    if (!slots || !d_blocks || !d_ext || !d_geom || !lk_ex_args_ok(LKX_FB, d_out_xy, d_status, d_err, d_back_xy, d_back_status, d_back_err)) return hipErrorInvalidValue;
    const LKExOut O{d_out_xy, d_status, d_err, d_work, d_back_xy, d_back_status, d_back_err, d_pred, d_pred && n_pred > 0 ? n_pred : 0};
    ProfScope ps(K_LK, s);
    if (lk_use_general(P)) {
        if (!lk_params_ok(P)) return hipErrorInvalidValue;
        hipLaunchKernelGGL(k_lk_batch_ex<true>, dim3(n_blocks), dim3(LKB_T), (size_t)lkg_lds(P.win).total, s, slots, d_blocks, d_ext, n_blocks, d_geom, P, O);
    } else hipLaunchKernelGGL(k_lk_batch_ex<false>, dim3(n_blocks), dim3(LKB_T), 0, s, slots, d_blocks, d_ext, n_blocks, d_geom, P, O);
    return hipGetLastError();
}

// =========================================================================================================
// goodFeaturesToTrack per grid cell
// =========================================================================================================
__device__ inline unsigned f32_key(float v) {   // order-preserving map float -> uint32
    const unsigned b = __float_as_uint(v);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ inline float f32_unkey(unsigned k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}
__device__ inline unsigned long long f64_key(double v) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ inline double f64_unkey(unsigned long long k) {
    return __longlong_as_double((long long)((k >> 63) ? (k & 0x7fffffffffffffffull) : ~k));
}

// Phase 1: min-eigenvalue response, 32x32 outputs per 256-thread workgroup.
// grid = (tiles_x, tiles_y, n_cells). cov at the 34x34 halo positions is evaluated at the REFLECT_101-mapped CELL
// coordinate (box filter border = cell), from pixels of the PARENT image with REFLECT_101 on the parent (Sobel border).
__global__ __launch_bounds__(256) void k_gftt_eig(const uint8_t* __restrict__ slots, PyrLayout L,
                                                  const int* __restrict__ cells, float* __restrict__ eig,
                                                  unsigned* __restrict__ cellmax) {
    __shared__ float sC[34 * 34 * 3];
    __shared__ unsigned smax[4];
    const int cell = blockIdx.z;
    const int cx0 = cells[CELL_STRIDE * cell], cy0 = cells[CELL_STRIDE * cell + 1], cw = cells[CELL_STRIDE * cell + 2], ch = cells[CELL_STRIDE * cell + 3];
    const int tx0 = blockIdx.x * 32, ty0 = blockIdx.y * 32;
    if (tx0 >= cw || ty0 >= ch) return;
    const uint8_t* img = level_origin(slots + (size_t)cells[CELL_STRIDE * cell + 4] * L.slot_bytes, L, 0);   // the cell's frame slot
    const int st = L.stride[0];
    const float k1 = (float)(1.0 / 3060.0), k2 = (float)(2.0 / 3060.0);
    for (int idx = threadIdx.x; idx < 34 * 34; idx += 256) {
        const int hy = idx / 34, hx = idx - hy * 34;
        const int lx = reflect101(tx0 - 1 + hx, cw), ly = reflect101(ty0 - 1 + hy, ch);
        // padded level 0 == REFLECT_101 of the parent image, so +-1 neighbours are plain loads
        const uint8_t* p = img + (ptrdiff_t)(cy0 + ly) * st + (cx0 + lx);
        const float p00 = p[-st - 1], p01 = p[-st], p02 = p[-st + 1];
        const float p10 = p[-1], p12 = p[1];
        const float p20 = p[st - 1], p21 = p[st], p22 = p[st + 1];
        const float rt = p02 - p00, rm = p12 - p10, rb = p22 - p20;
        const float dx = (rt + rb) * k1 + rm * k2;
        float s_t = k1 * p00; s_t += k2 * p01; s_t += k1 * p02;
        float s_b = k1 * p20; s_b += k2 * p21; s_b += k1 * p22;
        const float dy = s_b - s_t;
        sC[idx * 3 + 0] = dx * dx; sC[idx * 3 + 1] = dx * dy; sC[idx * 3 + 2] = dy * dy;
    }
    __syncthreads();
    unsigned mk = 0;   // key 0 is below every real float key
    for (int idx = threadIdx.x; idx < 32 * 32; idx += 256) {
        const int oy = idx >> 5, ox = idx & 31;
        const int x = tx0 + ox, y = ty0 + oy;
        if (x >= cw || y >= ch) continue;
        double s0 = 0, s1 = 0, s2 = 0;
#pragma unroll
        for (int j = 0; j < 3; j++)
#pragma unroll
            for (int i = 0; i < 3; i++) {
                const float* c = &sC[((oy + j) * 34 + (ox + i)) * 3];
                s0 += c[0]; s1 += c[1]; s2 += c[2];
            }
        const float a = (float)s0 * 0.5f, b = (float)s1, c2 = (float)s2 * 0.5f;
        const float e = (a + c2) - sqrtf((a - c2) * (a - c2) + b * b);
        eig[(size_t)cell * CELL_PIX + y * cw + x] = e;
        if (e == e) { const unsigned k = f32_key(e); mk = k > mk ? k : mk; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const unsigned t = __shfl_xor(mk, o, 64); mk = t > mk ? t : mk; }
    if ((threadIdx.x & 63) == 0) smax[threadIdx.x >> 6] = mk;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned m = smax[0];
        for (int i = 1; i < 4; i++) m = smax[i] > m ? smax[i] : m;
        atomicMax(&cellmax[cell], m);
    }
}

// ---- the detector pass proper: no response map in HBM -------------------------------------------------------------------------------
// cov = (dx^2, dx dy, dy^2) at one cell position (the Sobel arithmetic of k_gftt_eig, shared)
__device__ inline void gftt_cov(const uint8_t* __restrict__ p, int st, float& c0, float& c1, float& c2) {
    const float k1 = (float)(1.0 / 3060.0), k2 = (float)(2.0 / 3060.0);
    const float p00 = p[-st - 1], p01 = p[-st], p02 = p[-st + 1];
    const float p10 = p[-1], p12 = p[1];
    const float p20 = p[st - 1], p21 = p[st], p22 = p[st + 1];
    const float rt = p02 - p00, rm = p12 - p10, rb = p22 - p20;
    const float dx = (rt + rb) * k1 + rm * k2;
    float s_t = k1 * p00; s_t += k2 * p01; s_t += k1 * p02;
    float s_b = k1 * p20; s_b += k2 * p21; s_b += k1 * p22;
    const float dy = s_b - s_t;
    c0 = dx * dx; c1 = dx * dy; c2 = dy * dy;
}
// Pass 1, grid = (tiles_x, tiles_y, n_cells), 256 threads, 32x32 cell pixels per workgroup: covariances on the 36x36 halo, min-eigenvalue
// on 34x34, then the 3x3 non-maximum test on the RAW response and one (value, pixel) record per surviving pixel. The reference's order is
// threshold -> dilate -> compare; for a pixel above the threshold the thresholded neighbours exceed it exactly when the raw ones do
// (a neighbour at or below the threshold became 0), so the test needs no threshold - which is only known once the whole cell has been
// seen (0.01 x the cell's maximum, cellinfo[2 cell] by atomicMax). Pass 2 drops the records at or below it. Only values > 0 can ever be
// selected. HBM traffic: the cell's pixels once (+ halo), 8 B per local maximum - no 4 W H map.
// The work of one 32x32 tile at (tx0, ty0) of the cell (cx0, cy0, cw, ch) of `img` (level 0 of the cell's slot, row stride st), shared by
// k_gftt_cand (a cell of the grid) and k_gftt_cand_frame (a region of any size). list_val / list_idx: the cell's record list; info: its
// (maximum key, record count) pair; sC [36 * 36 * 3], sE [34 * 34], smax [4]: the workgroup's LDS.
__device__ __forceinline__ void gftt_cand_tile(const uint8_t* __restrict__ img, int st, int cx0, int cy0, int cw, int ch, int tx0, int ty0,
                                               float* __restrict__ list_val, unsigned* __restrict__ list_idx, unsigned* __restrict__ info, double quality,
                                               float* sC, float* sE, unsigned* smax) {
    for (int idx = threadIdx.x; idx < 36 * 36; idx += 256) {
        const int hy = idx / 36, hx = idx - hy * 36;
        // the box filter's border is the CELL's (REFLECT_101 of the cell coordinate); the Sobel's is the parent image's (= the padded level)
        const int lx = reflect101(tx0 - 2 + hx, cw), ly = reflect101(ty0 - 2 + hy, ch);
        gftt_cov(img + (ptrdiff_t)(cy0 + ly) * st + (cx0 + lx), st, sC[idx * 3], sC[idx * 3 + 1], sC[idx * 3 + 2]);
    }
    __syncthreads();
    unsigned mk = 0;   // key 0 is below every real float key
    for (int idx = threadIdx.x; idx < 34 * 34; idx += 256) {
        const int ey = idx / 34, ex = idx - ey * 34;
        const int x = tx0 - 1 + ex, y = ty0 - 1 + ey;
        float e = -1.f;   // outside the cell: never consulted (only interior pixels are tested), never counted in the maximum
        if (x >= 0 && y >= 0 && x < cw && y < ch) {
            double s0 = 0, s1 = 0, s2 = 0;
#pragma unroll
            for (int j = 0; j < 3; j++)
#pragma unroll
                for (int i = 0; i < 3; i++) {
                    const float* c = &sC[((ey + j) * 36 + (ex + i)) * 3];
                    s0 += c[0]; s1 += c[1]; s2 += c[2];
                }
            const float a = (float)s0 * 0.5f, b = (float)s1, c2 = (float)s2 * 0.5f;
            e = (a + c2) - sqrtf((a - c2) * (a - c2) + b * b);
            if (ex >= 1 && ex <= 32 && ey >= 1 && ey <= 32 && e == e) { const unsigned k = f32_key(e); mk = k > mk ? k : mk; }   // every cell pixel once
        }
        sE[idx] = e;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const unsigned t = __shfl_xor(mk, o, 64); mk = t > mk ? t : mk; }
    if ((threadIdx.x & 63) == 0) smax[threadIdx.x >> 6] = mk;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned m = smax[0];
        for (int i = 1; i < 4; i++) m = smax[i] > m ? smax[i] : m;
        atomicMax(&info[0], m);
    }
    // the tile's records are collected in LDS first (sC is free now), then ONE global atomic per workgroup reserves their place in the
    // cell's list (640 workgroups bumping 10 counters per wavefront and turn serialised in L2: 82 us per launch instead of 15)
    // A record at or below quality x (the largest response seen so far) can be dropped here already: the cell's maximum only grows, the
    // threshold with it (the same (float)((double)max * quality) as pass 2 uses, monotone in max), so pass 2 would drop it anyway. "So far" =
    // this tile's own maximum (reading what the other tiles have published - one more global load per thread behind the atomicMax - cost
    // 15 us per launch, measured): fewer records written, read back and compacted, at no cost.
    unsigned seen = smax[0];
    for (int i = 1; i < 4; i++) seen = smax[i] > seen ? smax[i] : seen;
    const float thr_now = seen ? (float)((double)f32_unkey(seen) * quality) : 0.f;
    unsigned* s_cnt = smax;                          // [0] tile count, [1] base in the cell's list
    float* lv = sC;                                  // up to 1024 values ...
    unsigned* li = (unsigned*)(sC + 1024);           // ... and pixel indices
    __syncthreads();
    if (threadIdx.x == 0) s_cnt[0] = 0;
    __syncthreads();
    for (int idx = threadIdx.x; idx < 32 * 32; idx += 256) {   // (every lane takes all four turns: the ballot below is wave-wide)
        const int oy = idx >> 5, ox = idx & 31;
        const int x = tx0 + ox, y = ty0 + oy;
        bool cand = false;
        float v = 0.f;
        if (x >= 1 && y >= 1 && x < cw - 1 && y < ch - 1) {
            v = sE[(oy + 1) * 34 + ox + 1];
            cand = v > 0.f && v > thr_now;
#pragma unroll
            for (int j = 0; j < 3; j++)
#pragma unroll
                for (int i = 0; i < 3; i++) cand = cand && !(sE[(oy + j) * 34 + ox + i] > v);
        }
        const unsigned long long bal = __ballot(cand);
        if (bal) {   // one LDS atomic per wavefront
            const int lane = threadIdx.x & 63;
            unsigned base = 0;
            if (lane == 0) base = atomicAdd(&s_cnt[0], (unsigned)__popcll(bal));
            base = __shfl(base, 0, 64);
            if (cand) {
                const unsigned slot = base + (unsigned)__popcll(bal & ((1ull << lane) - 1ull));
                lv[slot] = v; li[slot] = (unsigned)(y * cw + x);
            }
        }
    }
    __syncthreads();
    const unsigned nt = s_cnt[0];
    if (nt == 0) return;
    if (threadIdx.x == 0) s_cnt[1] = atomicAdd(&info[1], nt);
    __syncthreads();
    const unsigned gbase = s_cnt[1];
    float* cv = list_val + gbase;
    unsigned* ci = list_idx + gbase;
    for (unsigned i = threadIdx.x; i < nt; i += 256) { cv[i] = lv[i]; ci[i] = li[i]; }
}
__global__ __launch_bounds__(256) void k_gftt_cand(const uint8_t* __restrict__ slots, PyrLayout L, const int* __restrict__ cells,
                                                   float* __restrict__ cand_val, unsigned* __restrict__ cand_idx, unsigned* __restrict__ cellinfo, double quality) {
    __shared__ float sC[36 * 36 * 3];
    __shared__ float sE[34 * 34];
    __shared__ unsigned smax[4];
    BACKEND_PRIO();   // a short pass between two LK launches of its sequence: ahead of the bulk LK waves it shares SIMDs with
    const int cell = blockIdx.z;
    const int cx0 = cells[CELL_STRIDE * cell], cy0 = cells[CELL_STRIDE * cell + 1], cw = cells[CELL_STRIDE * cell + 2], ch = cells[CELL_STRIDE * cell + 3];
    // Consecutive workgroup ids go round the 8 XCDs, each with its own L2: blockIdx.x (8 values = the XCD) is the tile ROW, so the eight
    // tiles that share the 128-byte lines of a 32-row band of the image run on ONE XCD and the band is fetched from HBM once (with
    // blockIdx.x as the tile column every line was fetched by four XCDs: 2.75 MB of HBM reads per 0.47 MB frame by the PMC counters)
    const int tx0 = blockIdx.y * 32, ty0 = blockIdx.x * 32;
    if (tx0 >= cw || ty0 >= ch) return;
    const uint8_t* img = level_origin(slots + (size_t)cells[CELL_STRIDE * cell + 4] * L.slot_bytes, L, 0);
    gftt_cand_tile(img, L.stride[0], cx0, cy0, cw, ch, tx0, ty0, cand_val + (size_t)cell * CELL_PIX, cand_idx + (size_t)cell * CELL_PIX, cellinfo + 2 * cell,
                   quality, sC, sE, smax);
}

// Pass 2, one 256-thread workgroup per cell: records above the threshold are compacted into LDS and dealt to the lanes' REGISTERS; the
// greedy selection of cv::goodFeaturesToTrack ("walk the list sorted by (value, address) descending, accept a corner unless an accepted
// one is closer than minDistance") runs as: repeat {arg-max over the live records; accept; kill every record closer than minDistance} -
// identical result, max_corners rounds of register work with one 4-wavefront exchange each, no sort. A cell with more than GP_REG records
// above the threshold (a periodic texture can make every pixel a local maximum) takes the same rounds over its list in HBM.
// Four wavefronts per cell. Measured alternatives (shader-clock stamps, PMV_GFTT_DBG=1; one cell = 2740 raw records, 742 above the threshold):
// a round is a serial chain (arg-max -> accept -> kill) and costs ~2.9 k cycles whatever the operand width (64-bit keys: 3.4 k) - a lone or
// nearly lone wavefront issues one DEPENDENT instruction every 10-30 cycles, so the chain's instruction count is what matters; ONE wavefront
// per cell (no exchange, no barrier, 12 slots per lane) takes 9.6 k cycles per round: the slots' instructions do not overlap, they queue.
// SORTING the records once (bitonic network over the LDS list, 55 stages for 1024 records) and letting one wavefront walk the sorted list 64
// records at a time (accept in list order unless an accepted corner is closer than minDistance: OpenCV's loop verbatim, bit-exact in every
// test) took 84 us per launch instead of 60: a stage with its barrier costs ~1 us, not the 200 cycles of its instruction count.
constexpr int GP_T = 256, GP_SLOTS = 16, GP_REG = GP_T * GP_SLOTS, GP_MAXOUT = 4096;   // GP_MAXOUT = MAX_PER_CELL of pmv_ctx.h
__global__ __launch_bounds__(GP_T) void k_gftt_pick(const int* __restrict__ cells, float* __restrict__ cand_val, unsigned* __restrict__ cand_idx,
                                                    const unsigned* __restrict__ cellinfo, int max_corners, double quality, double min_dist,
                                                    int unlimited, int* __restrict__ out_xy, int* __restrict__ out_count, int* __restrict__ flags) {
    __shared__ unsigned long long lkey[GP_REG];
    __shared__ __attribute__((aligned(16))) unsigned long long wbest[2][4];
    // accepted corners, (y << 16) | x, written to HBM once at the end: a global store per round sits in front of the next round's barrier
    // (__syncthreads waits for the wavefront's outstanding stores: 1-2 us each - 80 of the 93 us this kernel took with the store inside the loop)
    __shared__ unsigned s_acc[GP_MAXOUT];
    BACKEND_PRIO();
    const unsigned long long dbg_t0 = __builtin_readcyclecounter();
    const int cell = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int cw = cells[CELL_STRIDE * cell + 2];
    float* cv = cand_val + (size_t)cell * CELL_PIX;
    unsigned* ci = cand_idx + (size_t)cell * CELL_PIX;
    const int nraw = (int)cellinfo[2 * cell + 1];
    const double maxVal = (double)f32_unkey(cellinfo[2 * cell]);
    const float thr = (float)(maxVal * quality);
    // compaction of the records above the threshold: key = (value bits, pixel index), 0 = dead. The first GP_REG go to LDS, the rest
    // stay in the HBM list, compacted in place (a record only moves to a lower position, behind every record already read)
    int n = 0;
    constexpr int CPT = 4;   // records per thread and chunk: a quarter of the barriers
    for (int base = 0; base < nraw; base += GP_T * CPT) {
        float v[CPT]; unsigned px[CPT]; bool keep[CPT];
#pragma unroll
        for (int q = 0; q < CPT; q++) {
            const int i = base + q * GP_T + tid;
            v[q] = 0.f; px[q] = 0;
            if (i < nraw) { v[q] = cv[i]; px[q] = ci[i]; }
            keep[q] = i < nraw && v[q] > thr;
        }
        __syncthreads();   // (all reads of this chunk before any in-place write into it)
        // place in the compacted list = records kept so far + those of the wavefronts before + those of this wavefront's earlier turns + rank
        // in the ballot (any order will do, the selection is order-free; every target position lies inside the part already read)
        int wave_tot = 0;
#pragma unroll
        for (int q = 0; q < CPT; q++) wave_tot += __popcll(__ballot(keep[q]));
        int off = n, tot = wave_tot;
        if (GP_T > 64) {
            if (lane == 0) wbest[0][wave] = (unsigned long long)wave_tot;
            __syncthreads();
            for (int w2 = 0; w2 < wave; w2++) off += (int)wbest[0][w2];
            tot = (int)(wbest[0][0] + wbest[0][1] + wbest[0][2] + wbest[0][3]);
        }
        int run = 0;
#pragma unroll
        for (int q = 0; q < CPT; q++) {
            const unsigned long long bal = __ballot(keep[q]);
            if (keep[q]) {
                const int slot = off + run + __popcll(bal & ((1ull << lane) - 1ull));
                if (slot < GP_REG) lkey[slot] = ((unsigned long long)__float_as_uint(v[q]) << 32) | px[q];
                else { cv[slot] = v[q]; ci[slot] = px[q]; }
            }
            run += __popcll(bal);
        }
        n += tot;
    }
    __syncthreads();
    const unsigned long long dbg_t1 = __builtin_readcyclecounter();
    const bool use_dist = min_dist >= 1.0;
    const double md2 = min_dist * min_dist;
    // dx*dx + dy*dy is an integer: (double)d2 < md2  <=>  d2 < ceil(md2)
    const int md2i = (int)(md2 < 2.0e9 ? ceil(md2) : 2.0e9);
    const int n_reg = n < GP_REG ? n : GP_REG;
    // A record in registers = (value bits, (y << 16) | x): the pair orders like (value, pixel index = y * cw + x), the coordinates need no
    // division by the cell width in the rounds, and every comparison is a full-rate 32-bit one (v_cmp / v_cndmask on 64-bit keys are not)
    unsigned kv[GP_SLOTS], kp[GP_SLOTS];   // kv == 0: dead / empty (live values are > 0)
#pragma unroll
    for (int s2 = 0; s2 < GP_SLOTS; s2++) {
        const int i = s2 * GP_T + tid;
        const unsigned long long k = i < n_reg ? lkey[i] : 0ull;
        kv[s2] = (unsigned)(k >> 32);
        const int px = (int)(k & 0x7fffffffu);
        const int y = px / cw;
        kp[s2] = ((unsigned)y << 16) | (unsigned)(px - y * cw);
    }
    unsigned* wv = (unsigned*)&wbest[0][0];   // [2][4] values, then [2][4] positions
    unsigned* wp = wv + 8;
    int naccepted = 0;
    const unsigned long long dbg_t2 = __builtin_readcyclecounter();
    const int nslots = (n_reg + GP_T - 1) / GP_T;   // slots in use (uniform): a typical cell keeps ~750 records = 3 of the 16
    unsigned bv = 0, bp = 0;                        // this lane's best live record; recomputed only after one of its records died
#pragma unroll
    for (int s2 = 0; s2 < GP_SLOTS; s2++) { const bool g = kv[s2] > bv || (kv[s2] == bv && kp[s2] > bp); bv = g ? kv[s2] : bv; bp = g ? kp[s2] : bp; }
    for (int it = 0; it < max_corners; it++) {
        unsigned tv = bv, tp = bp;
        for (int i = GP_REG + tid; i < n; i += GP_T) {   // (only for cells beyond the register capacity: records in HBM, bit 31 of the index = dead)
            const unsigned px = ci[i];
            if (px >> 31) continue;
            const unsigned v = __float_as_uint(cv[i]);
            const int y = (int)px / cw;
            const unsigned pp = ((unsigned)y << 16) | (unsigned)((int)px - y * cw);
            const bool g = v > tv || (v == tv && pp > tp);
            tv = g ? v : tv; tp = g ? pp : tp;
        }
        // arg-max over the workgroup: first the value, then the position among the lanes that hold that value
        const unsigned mv = wave_max_u32(tv);
        // the position: almost always ONE lane holds the maximum value - read its position directly; a second reduction only on a tie
        const unsigned long long holders = __ballot(tv == mv);
        unsigned mp;
        if (__popcll(holders) == 1) mp = (unsigned)__builtin_amdgcn_readlane((int)tp, __builtin_ctzll(holders));
        else mp = wave_max_u32(tv == mv ? tp : 0u);
        unsigned V = mv, P = mp;
        if (GP_T > 64) {   // several wavefronts per cell: one exchange through LDS per round (the buffer alternates)
            if (lane == 0) { wv[(it & 1) * 4 + wave] = mv; wp[(it & 1) * 4 + wave] = mp; }
            __syncthreads();
            const uint4 v4 = *(const uint4*)&wv[(it & 1) * 4], p4 = *(const uint4*)&wp[(it & 1) * 4];
            V = max(max(v4.x, v4.y), max(v4.z, v4.w));
            P = max(max(v4.x == V ? p4.x : 0u, v4.y == V ? p4.y : 0u), max(v4.z == V ? p4.z : 0u, v4.w == V ? p4.w : 0u));
        }
        if (V == 0) break;
        const int bx = (int)(P & 0xffffu), by = (int)(P >> 16);
        if (tid == 0) s_acc[naccepted] = P;
        naccepted++;
        bool died = false;
#pragma unroll
        for (int s2 = 0; s2 < GP_SLOTS; s2++) {
            if (s2 < nslots) {   // uniform (no break: the loop has to unroll, the slots are registers)
                bool kill;
                if (use_dist) {
                    const int dx = (int)(kp[s2] & 0xffffu) - bx, dy = (int)(kp[s2] >> 16) - by;
                    kill = dx * dx + dy * dy < md2i;
                } else kill = kp[s2] == P;
                kill = kill && kv[s2] != 0;
                if (kill) kv[s2] = 0;
                died = died || kill;
            }
        }
        if (died) {
            bv = 0; bp = 0;
#pragma unroll
            for (int s2 = 0; s2 < GP_SLOTS; s2++) {
                if (s2 < nslots) {
                    const bool g = kv[s2] > bv || (kv[s2] == bv && kp[s2] > bp);
                    bv = g ? kv[s2] : bv; bp = g ? kp[s2] : bp;
                }
            }
        }
        for (int i = GP_REG + tid; i < n; i += GP_T) {
            const unsigned u = ci[i];
            if (u >> 31) continue;
            bool kill;
            const int y = (int)u / cw, x = (int)u - y * cw;
            if (use_dist) {
                const int dx = x - bx, dy = y - by;
                kill = dx * dx + dy * dy < md2i;
            } else kill = x == bx && y == by;
            if (kill) ci[i] = u | 0x80000000u;
        }
    }
    // cv::goodFeaturesToTrack(maxCorners <= 0) has no limit; here the caller's buffer holds max_corners: more corners than that
    // is reported (bit 2), not silently truncated
    if (unlimited && naccepted == max_corners) {
        int live = 0;
#pragma unroll
        for (int s2 = 0; s2 < GP_SLOTS; s2++) live |= kv[s2] != 0;
        for (int i = GP_REG + tid; i < n; i += GP_T) live |= !(ci[i] >> 31);
        if (live) atomicOr(flags, 4);
    }
    if (cell == 0 && tid == 0 && (flags[0] & 0x40000000)) {   // diagnostic (PMV_GFTT_DBG=1): cycles of compaction / key set-up / rounds, record counts
        const unsigned long long dbg_t3 = __builtin_readcyclecounter();
        flags[1] = (int)(dbg_t1 - dbg_t0); flags[2] = (int)(dbg_t2 - dbg_t1); flags[3] = (int)(dbg_t3 - dbg_t2);
        flags[0] = 0x40000000 | (nraw & 0xffff) | ((n & 0x3fff) << 16);
    }
    __syncthreads();
    for (int i = tid; i < naccepted; i += GP_T) {
        const unsigned a = s_acc[i];   // (y << 16) | x
        *(int2*)&out_xy[((size_t)cell * max_corners + i) * 2] = make_int2((int)(a & 0xffffu), (int)(a >> 16));
    }
    if (tid == 0) out_count[cell] = naccepted;
}

hipError_t launch_gftt(hipStream_t s, const uint8_t* slots, const PyrLayout& L, const int* d_cells, int n_cells,
                       int max_per_cell, double quality, double min_dist, int unlimited, float* d_eig, unsigned* d_cellmax,
                       int* d_out_xy, int* d_out_count, int* d_flags, unsigned* d_spill) {
    if (!slots || !d_cells || !d_eig || !d_cellmax || !d_out_xy || !d_out_count || !d_flags || !d_spill || n_cells < 1 || max_per_cell < 1 || max_per_cell > GP_MAXOUT) return hipErrorInvalidValue;
    // d_eig / d_spill: the cells' candidate records (value / pixel index, CELL_PIX each); d_cellmax: (maximum key, record count) per cell
    hipError_t e = hipMemsetAsync(d_cellmax, 0, 2 * sizeof(unsigned) * n_cells, s);
    if (e != hipSuccess) return e;
    { ProfScope ps(K_GFTT_CAND, s);
    hipLaunchKernelGGL(k_gftt_cand, dim3(8, 8, n_cells), dim3(256), 0, s, slots, L, d_cells, d_eig, d_spill, d_cellmax, quality); }
    ProfScope ps2(K_GFTT_PICK, s);
    hipLaunchKernelGGL(k_gftt_pick, dim3(n_cells), dim3(GP_T), 0, s, d_cells, d_eig, d_spill, d_cellmax, max_per_cell,
                       quality, min_dist, unlimited, d_out_xy, d_out_count, d_flags);
    return hipGetLastError();
}
// diagnostic / parity: the response map itself (pmv_debug_gftt_response), which the detector pass no longer writes
hipError_t launch_gftt_response(hipStream_t s, const uint8_t* slots, const PyrLayout& L, const int* d_cells, int n_cells, float* d_eig, unsigned* d_cellmax) {
    if (!slots || !d_cells || !d_eig || !d_cellmax || n_cells < 1) return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(d_cellmax, 0, 2 * sizeof(unsigned) * n_cells, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_gftt_eig, dim3(8, 8, n_cells), dim3(256), 0, s, slots, L, d_cells, d_eig, d_cellmax);
    return hipGetLastError();
}

// ---- the caller's goodFeaturesToTrack arguments (pmv_detect_gftt_ex): blockSize 1..15, Harris response, mask ------------------------
// The general kernels keep k_gftt_cand's shape - a 32x32 tile per workgroup, the tile row on blockIdx.x, the response on 34x34, the
// non-maximum test on the raw response, ballot-compacted records, one global atomic per workgroup - with the block size, the response
// kind and the mask as RUNTIME arguments (one code object, no spills: the b x b sum is a plain nested loop over LDS). cov lives on a
// (34 + b - 1)^2 halo in dynamic LDS as three PLANES, not as float3 records: consecutive lanes then read consecutive dwords of a plane
// whatever the halo width, and a 32-lane group spans at most two halo rows (a gap of b - 1 dwords: at worst two lanes on one bank).
// Window of the box filter: anchor b / 2, so offsets -b/2 .. b-1-b/2 (an even size leans to the upper left), REFLECT_101 of the CELL
// coordinate as often as needed; the sum is the b*b-term double sum in raster order that tests/twin/gftt_twin.cpp states.
// mask (optional): the cells' mask sub-views, cw*ch bytes each at byte offset cells[.. + 5], indexed with the y*cw+x of a record. Only
// allowed pixels count in the tile's and the cell's maximum and only they become records; the 3x3 test looks at every neighbour.
__device__ inline void gftt_cov_k(const uint8_t* __restrict__ p, int st, float k1, float k2, float& c0, float& c1, float& c2) {
    const float p00 = p[-st - 1], p01 = p[-st], p02 = p[-st + 1];
    const float p10 = p[-1], p12 = p[1];
    const float p20 = p[st - 1], p21 = p[st], p22 = p[st + 1];
    const float rt = p02 - p00, rm = p12 - p10, rb = p22 - p20;
    const float dx = (rt + rb) * k1 + rm * k2;
    float s_t = k1 * p00; s_t += k2 * p01; s_t += k1 * p02;
    float s_b = k1 * p20; s_b += k2 * p21; s_b += k1 * p22;
    const float dy = s_b - s_t;
    c0 = dx * dx; c1 = dx * dy; c2 = dy * dy;
}
// cov planes of the tile at (tx0, ty0): halo position (hx, hy) = cell position (tx0 - 1 - b/2 + hx, ty0 - 1 - b/2 + hy), reflected
__device__ inline void gfttg_fill(const uint8_t* __restrict__ img, int st, int cx0, int cy0, int cw, int ch, int tx0, int ty0, const GfttExt& X,
                                  float* __restrict__ sC0, float* __restrict__ sC1, float* __restrict__ sC2) {
    const int HS = 34 + X.bs - 1, org = 1 + X.bs / 2;
    for (int idx = threadIdx.x; idx < HS * HS; idx += 256) {
        const int hy = idx / HS, hx = idx - hy * HS;
        const int lx = reflect101(tx0 - org + hx, cw), ly = reflect101(ty0 - org + hy, ch);   // inside the cell, whatever b: the loads stay in the frame
        gftt_cov_k(img + (ptrdiff_t)(cy0 + ly) * st + (cx0 + lx), st, X.k1, X.k2, sC0[idx], sC1[idx], sC2[idx]);
    }
}
// response at position (ex, ey) of the 34x34 grid (cell position (tx0 - 1 + ex, ty0 - 1 + ey)): its window starts at halo (ex, ey)
__device__ inline float gfttg_resp(const float* __restrict__ sC0, const float* __restrict__ sC1, const float* __restrict__ sC2, int ex, int ey, const GfttExt& X) {
    const int HS = 34 + X.bs - 1;
    double s0 = 0, s1 = 0, s2 = 0;
    for (int j = 0; j < X.bs; j++) {
        const int row = (ey + j) * HS + ex;
        for (int i = 0; i < X.bs; i++) { s0 += sC0[row + i]; s1 += sC1[row + i]; s2 += sC2[row + i]; }
    }
    if (X.harris) {   // (float)(a*c - b*b - k*(a + c)*(a + c)) with C++'s types: float products and difference, the k term and the last subtraction in double
        const float a = (float)s0, b = (float)s1, c = (float)s2;
        return (float)(a * c - b * b - X.k * (a + c) * (a + c));
    }
    const float a = (float)s0 * 0.5f, b = (float)s1, c2 = (float)s2 * 0.5f;
    return (a + c2) - sqrtf((a - c2) * (a - c2) + b * b);
}
// gftt_cand_tile's counterpart for the general kernels (k_gftt_cand_general, k_gftt_cand_general_frame). cmask: null, or the cell's packed
// mask sub-view; lds: the workgroup's dynamic LDS (gfttg_lds_bytes).
__device__ __forceinline__ void gfttg_cand_tile(const uint8_t* __restrict__ img, int st, int cx0, int cy0, int cw, int ch, int tx0, int ty0, const GfttExt& X,
                                                const uint8_t* __restrict__ cmask, float* __restrict__ list_val, unsigned* __restrict__ list_idx,
                                                unsigned* __restrict__ info, double quality, float* lds) {
    const int HP = (34 + X.bs - 1) * (34 + X.bs - 1);
    float* sC0 = lds; float* sC1 = sC0 + HP; float* sC2 = sC1 + HP;
    float* sE = sC2 + HP;                            // [34 * 34]
    unsigned* smax = (unsigned*)(sE + 34 * 34);      // [4]
    gfttg_fill(img, st, cx0, cy0, cw, ch, tx0, ty0, X, sC0, sC1, sC2);
    __syncthreads();
    unsigned mk = 0;   // key 0 is below every real float key
    for (int idx = threadIdx.x; idx < 34 * 34; idx += 256) {
        const int ey = idx / 34, ex = idx - ey * 34;
        const int x = tx0 - 1 + ex, y = ty0 - 1 + ey;
        float e = -1.f;   // outside the cell: never consulted, never counted
        if (x >= 0 && y >= 0 && x < cw && y < ch) {
            e = gfttg_resp(sC0, sC1, sC2, ex, ey, X);
            // every cell pixel once, and only the allowed ones: the threshold follows the MASKED maximum (cv::minMaxLoc with the mask)
            if (ex >= 1 && ex <= 32 && ey >= 1 && ey <= 32 && e == e && (!cmask || cmask[y * cw + x])) { const unsigned k = f32_key(e); mk = k > mk ? k : mk; }
        }
        sE[idx] = e;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const unsigned t = __shfl_xor(mk, o, 64); mk = t > mk ? t : mk; }
    if ((threadIdx.x & 63) == 0) smax[threadIdx.x >> 6] = mk;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned m = smax[0];
        for (int i = 1; i < 4; i++) m = smax[i] > m ? smax[i] : m;
        if (m) atomicMax(&info[0], m);   // (a tile without an allowed pixel has nothing to publish)
    }
    // the early drop of k_gftt_cand, against the tile's own MASKED maximum: the cell's masked maximum is at least that
    unsigned seen = smax[0];
    for (int i = 1; i < 4; i++) seen = smax[i] > seen ? smax[i] : seen;
    const float thr_now = seen ? (float)((double)f32_unkey(seen) * quality) : 0.f;
    unsigned* s_cnt = smax;                          // [0] tile count, [1] base in the cell's list
    float* lv = sC0;                                 // up to 1024 values and pixel indices: 2048 dwords of the >= 3 * 34 * 34 of the planes
    unsigned* li = (unsigned*)(sC0 + 1024);
    __syncthreads();
    if (threadIdx.x == 0) s_cnt[0] = 0;
    __syncthreads();
    for (int idx = threadIdx.x; idx < 32 * 32; idx += 256) {   // (every lane takes all four turns: the ballot below is wave-wide)
        const int oy = idx >> 5, ox = idx & 31;
        const int x = tx0 + ox, y = ty0 + oy;
        bool cand = false;
        float v = 0.f;
        if (x >= 1 && y >= 1 && x < cw - 1 && y < ch - 1) {
            v = sE[(oy + 1) * 34 + ox + 1];
            cand = v > 0.f && v > thr_now && (!cmask || cmask[y * cw + x]);
#pragma unroll
            for (int j = 0; j < 3; j++)
#pragma unroll
                for (int i = 0; i < 3; i++) cand = cand && !(sE[(oy + j) * 34 + ox + i] > v);
        }
        const unsigned long long bal = __ballot(cand);
        if (bal) {   // one LDS atomic per wavefront
            const int lane = threadIdx.x & 63;
            unsigned base = 0;
            if (lane == 0) base = atomicAdd(&s_cnt[0], (unsigned)__popcll(bal));
            base = __shfl(base, 0, 64);
            if (cand) {
                const unsigned slot = base + (unsigned)__popcll(bal & ((1ull << lane) - 1ull));
                lv[slot] = v; li[slot] = (unsigned)(y * cw + x);
            }
        }
    }
    __syncthreads();
    const unsigned nt = s_cnt[0];
    if (nt == 0) return;
    if (threadIdx.x == 0) s_cnt[1] = atomicAdd(&info[1], nt);
    __syncthreads();
    const unsigned gbase = s_cnt[1];
    float* cv = list_val + gbase;
    unsigned* ci = list_idx + gbase;
    for (unsigned i = threadIdx.x; i < nt; i += 256) { cv[i] = lv[i]; ci[i] = li[i]; }
}
__global__ __launch_bounds__(256) void k_gftt_cand_general(const uint8_t* __restrict__ slots, PyrLayout L, const int* __restrict__ cells,
                                                           float* __restrict__ cand_val, unsigned* __restrict__ cand_idx, unsigned* __restrict__ cellinfo,
                                                           double quality, GfttExt X, const uint8_t* __restrict__ mask) {
    extern __shared__ float gfttg_lds[];
    BACKEND_PRIO();
    const int cell = blockIdx.z;
    const int cx0 = cells[CELL_STRIDE * cell], cy0 = cells[CELL_STRIDE * cell + 1], cw = cells[CELL_STRIDE * cell + 2], ch = cells[CELL_STRIDE * cell + 3];
    const int tx0 = blockIdx.y * 32, ty0 = blockIdx.x * 32;   // blockIdx.x = the tile ROW: see k_gftt_cand
    if (tx0 >= cw || ty0 >= ch) return;
    const uint8_t* img = level_origin(slots + (size_t)cells[CELL_STRIDE * cell + 4] * L.slot_bytes, L, 0);
    const uint8_t* cmask = mask ? mask + (size_t)cells[CELL_STRIDE * cell + 5] : nullptr;
    gfttg_cand_tile(img, L.stride[0], cx0, cy0, cw, ch, tx0, ty0, X, cmask, cand_val + (size_t)cell * CELL_PIX, cand_idx + (size_t)cell * CELL_PIX,
                    cellinfo + 2 * cell, quality, gfttg_lds);
}
// diagnostic / parity (pmv_debug_gftt_response_ex): the response map of the same arithmetic, the only general launch that writes one
__global__ __launch_bounds__(256) void k_gftt_eig_general(const uint8_t* __restrict__ slots, PyrLayout L, const int* __restrict__ cells,
                                                          float* __restrict__ eig, GfttExt X) {
    extern __shared__ float gfttg_lds[];
    const int HP = (34 + X.bs - 1) * (34 + X.bs - 1);
    float* sC0 = gfttg_lds; float* sC1 = sC0 + HP; float* sC2 = sC1 + HP;
    const int cell = blockIdx.z;
    const int cx0 = cells[CELL_STRIDE * cell], cy0 = cells[CELL_STRIDE * cell + 1], cw = cells[CELL_STRIDE * cell + 2], ch = cells[CELL_STRIDE * cell + 3];
    const int tx0 = blockIdx.y * 32, ty0 = blockIdx.x * 32;
    if (tx0 >= cw || ty0 >= ch) return;
    const uint8_t* img = level_origin(slots + (size_t)cells[CELL_STRIDE * cell + 4] * L.slot_bytes, L, 0);
    gfttg_fill(img, L.stride[0], cx0, cy0, cw, ch, tx0, ty0, X, sC0, sC1, sC2);
    __syncthreads();
    for (int idx = threadIdx.x; idx < 32 * 32; idx += 256) {
        const int oy = idx >> 5, ox = idx & 31;
        const int x = tx0 + ox, y = ty0 + oy;
        if (x < cw && y < ch) eig[(size_t)cell * CELL_PIX + y * cw + x] = gfttg_resp(sC0, sC1, sC2, ox + 1, oy + 1, X);
    }
}
static size_t gfttg_lds_bytes(int bs) { const size_t hs = 34 + (size_t)bs - 1; return (3 * hs * hs + 34 * 34 + 4) * sizeof(float); }
static bool gftt_ext_ok(const GfttExt& X) { return X.bs >= 1 && X.bs <= GFTT_MAX_BLOCK && (!X.harris || std::isfinite(X.k)); }

hipError_t launch_gftt_ex(hipStream_t s, const uint8_t* slots, const PyrLayout& L, const int* d_cells, int n_cells, int max_per_cell, double quality,
                          double min_dist, int unlimited, const GfttExt& X, const uint8_t* d_mask, float* d_eig, unsigned* d_cellmax, int* d_out_xy,
                          int* d_out_count, int* d_flags, unsigned* d_spill) {
    if (!slots || !d_cells || !d_eig || !d_cellmax || !d_out_xy || !d_out_count || !d_flags || !d_spill || n_cells < 1 || max_per_cell < 1 || max_per_cell > GP_MAXOUT ||
        !gftt_ext_ok(X)) return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(d_cellmax, 0, 2 * sizeof(unsigned) * n_cells, s);
    if (e != hipSuccess) return e;
    { ProfScope ps(K_GFTT_CAND, s);
    hipLaunchKernelGGL(k_gftt_cand_general, dim3(8, 8, n_cells), dim3(256), gfttg_lds_bytes(X.bs), s, slots, L, d_cells, d_eig, d_spill, d_cellmax, quality, X, d_mask); }
    // the selection does not depend on the block size, the response kind or the mask: only values > 0 reach it (quality in (0, 1])
    ProfScope ps2(K_GFTT_PICK, s);
    hipLaunchKernelGGL(k_gftt_pick, dim3(n_cells), dim3(GP_T), 0, s, d_cells, d_eig, d_spill, d_cellmax, max_per_cell,
                       quality, min_dist, unlimited, d_out_xy, d_out_count, d_flags);
    return hipGetLastError();
}
hipError_t launch_gftt_response_ex(hipStream_t s, const uint8_t* slots, const PyrLayout& L, const int* d_cells, int n_cells, const GfttExt& X, float* d_eig) {
    if (!slots || !d_cells || !d_eig || n_cells < 1 || !gftt_ext_ok(X)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_gftt_eig_general, dim3(8, 8, n_cells), dim3(256), gfttg_lds_bytes(X.bs), s, slots, L, d_cells, d_eig, X);
    return hipGetLastError();
}

// ---- cv::goodFeaturesToTrack on a region of any size (pmv_detect_gftt_frame) ---------------------------------------------------------
// A request record is a cell record (x0, y0, w, h, slot, byte offset of the region's packed mask) whose ints 6 and 7 hold the first entry
// of the request's record list, low and high word: the lists of a launch lie one after the other, each as long as its region has pixels (a
// flat positive plateau makes every pixel a record). info: (maximum key, record count) per request, as cellinfo.
// Pass 1 is gftt_cand_tile / gfttg_cand_tile over ceil(h / 32) x ceil(w / 32) tiles. The tiles of one 32-row band share the band's cache
// lines, so they should run on one XCD (the measurement above k_gftt_cand); consecutive workgroup ids go round the 8 XCDs, and with more
// than 8 tile rows blockIdx.x = tile row no longer says which. The launch is (8 * ceil(tiles_y / 8) * tiles_x, requests): its x extent is a
// multiple of 8, so workgroup (b, r) runs on XCD b % 8 whatever r, and the k = b / 8-th workgroup of XCD x takes tile row x + 8 * (k /
// tiles_x), column k % tiles_x: row t of every request lands on XCD t % 8. Workgroups past a request's last row leave at once.
constexpr int GF_CAP = GFTT_FRAME_ONCHIP;   // records it sorts on chip: 128 KiB of the CU's 160 KiB of LDS as 64-bit keys
constexpr size_t GF_LDS = (size_t)GF_CAP * 8 + (size_t)(2 * GF_T + 32) * 4;   // keys | survivors of a chunk | its accepted corners | counters
__device__ __forceinline__ size_t gf_list_off(const int* __restrict__ r) { return (size_t)(unsigned)r[6] | ((size_t)(unsigned)r[7] << 32); }
__device__ __forceinline__ bool gf_tile_of_block(int cw, int ch, int& tx0, int& ty0) {
    const int tiles_x = (cw + 31) >> 5, tiles_y = (ch + 31) >> 5;
    const int xcd = blockIdx.x & 7, k = blockIdx.x >> 3;
    const int band = k / tiles_x;
    tx0 = (k - band * tiles_x) * 32; ty0 = (xcd + 8 * band) * 32;
    return xcd + 8 * band < tiles_y;
}
__global__ __launch_bounds__(256) void k_gftt_cand_frame(const uint8_t* __restrict__ slots, PyrLayout L, const int* __restrict__ recs,
                                                         float* __restrict__ cand_val, unsigned* __restrict__ cand_idx, unsigned* __restrict__ info, double quality) {
    __shared__ float sC[36 * 36 * 3];
    __shared__ float sE[34 * 34];
    __shared__ unsigned smax[4];
    BACKEND_PRIO();
    const int* __restrict__ r = recs + CELL_STRIDE * blockIdx.y;
    const int cw = r[2], ch = r[3];
    int tx0, ty0;
    if (!gf_tile_of_block(cw, ch, tx0, ty0)) return;
    const uint8_t* img = level_origin(slots + (size_t)r[4] * L.slot_bytes, L, 0);
    const size_t off = gf_list_off(r);
    gftt_cand_tile(img, L.stride[0], r[0], r[1], cw, ch, tx0, ty0, cand_val + off, cand_idx + off, info + 2 * blockIdx.y, quality, sC, sE, smax);
}
__global__ __launch_bounds__(256) void k_gftt_cand_general_frame(const uint8_t* __restrict__ slots, PyrLayout L, const int* __restrict__ recs,
                                                                 float* __restrict__ cand_val, unsigned* __restrict__ cand_idx, unsigned* __restrict__ info,
                                                                 double quality, GfttExt X, const uint8_t* __restrict__ mask) {
    extern __shared__ float gfttg_lds[];
    BACKEND_PRIO();
    const int* __restrict__ r = recs + CELL_STRIDE * blockIdx.y;
    const int cw = r[2], ch = r[3];
    int tx0, ty0;
    if (!gf_tile_of_block(cw, ch, tx0, ty0)) return;
    const uint8_t* img = level_origin(slots + (size_t)r[4] * L.slot_bytes, L, 0);
    const uint8_t* cmask = mask ? mask + (size_t)(unsigned)r[5] : nullptr;
    const size_t off = gf_list_off(r);
    gfttg_cand_tile(img, L.stride[0], r[0], r[1], cw, ch, tx0, ty0, X, cmask, cand_val + off, cand_idx + off, info + 2 * blockIdx.y, quality, gfttg_lds);
}

// Pass 2, ONE launch, one 1024-thread workgroup per request, no host round trip and nothing another workgroup writes is waited for.
//   1. The records above the threshold become 64-bit keys (value bits << 32 | y << 16 | x): for values > 0 and x < w the key orders like cv's
//      (value, address y * w + x), and it is unique, so the order of the keys is total and the place a record had in the list (which depends
//      on the order the tiles of pass 1 finished in) cannot show in the result. Up to GF_CAP keys stay in LDS.
//   2. The keys are sorted, descending, by a bitonic network whose comparators all point the same way (each merge begins with the mirrored
//      "flip" step), so a partner index beyond n stands for a key below every real one and is skipped: any n, no padding. A stage with its
//      barrier costs ~1 us whatever its instruction count (the measurement above k_gftt_pick) - of the 105 stages of 16 k keys the 95 whose
//      comparators span at most 1024 keys are run by ONE wavefront per 1024-key block, with no workgroup barrier between them: the LDS
//      operations of a wavefront complete in order. 10 stages keep their barrier.
//   3. min_dist < 1: the first `cap` keys are cv's answer (its loop accepts every record then). Otherwise the sorted list is walked in
//      chunks of 1024 records, one per thread: (a) every thread tests its record against all corners accepted from earlier chunks; (b) the
//      survivors are compacted in order; (c) wavefront 0 takes them 64 at a time - each against the corners accepted earlier in this chunk,
//      then the wavefront accepts the first live lane and kills the lanes within min_dist of it until none is left. That IS cv's loop
//      (walk the list in order, accept a record unless an accepted corner is closer than min_dist): a record is dropped only because of a
//      corner that precedes it in the order and was accepted, and every such corner is seen in (a), in (c)'s test or in (c)'s in-wave loop
//      before the record's turn. Stated as the fixed point: the accepted set is the set of records that outrank every ACCEPTED record within
//      min_dist of them; accepting at once every live record that outranks all LIVE records within min_dist of it and killing their
//      neighbourhoods reaches the same set, because the top live record is always such a record and a kill is only ever made by an accepted
//      one - the in-wave loop is that step on 64 records. The first `cap` accepted, in rank order, are the answer: the walk stops there.
//      Accepted corners are kept in the memory of the keys themselves (32-bit slot a lies inside key a / 2, and a <= the number of records
//      already held in registers), written to the caller's list once at the end - no global store in front of a barrier.
//   More than GF_CAP records above the threshold (noise at block size 1): the same steps over the key list in HBM (gkeys, as long as the
//   record list) with a workgroup barrier after every stage - exact, slower, reported in stats[1].
//   distances: dx * dx + dy * dy is an integer, (double)d2 < min_dist^2 <=> d2 < ceil(min_dist^2); frames up to 32767 x 32767 keep it in an int.
// out_count[request]: the number of corners, or -1 for a no-limit request (cap + 1 corners were looked for) that has more than cap.
// stats: (records above the threshold, of those kept in HBM) per request.
// step 3 for min_dist >= 1; returns the number of accepted corners (<= limit), their (y << 16) | x in ((unsigned*)keys)[0 .. ), visible to all
__device__ __forceinline__ int gf_walk(unsigned long long* keys, int n, int limit, int md2i, unsigned* s_surv, unsigned* s_new, unsigned* s_w, int tid) {
    const int lane = tid & 63, wave = tid >> 6;
    typedef unsigned __attribute__((may_alias)) acc_t;   // (32-bit slots inside the memory of the 64-bit keys)
    acc_t* acc = (acc_t*)keys;
    int na = 0;
    for (int base = 0; base < n && na < limit; base += GF_T) {
        const int i = base + tid;
        bool alive = i < n;
        const unsigned p = alive ? (unsigned)keys[i] : 0u;
        const int px = (int)(p & 0xffffu), py = (int)(p >> 16);
        for (int a = 0; a < na; a++) {               // (a) every lane reads the same word
            const unsigned q = acc[a];
            const int dx = (int)(q & 0xffffu) - px, dy = (int)(q >> 16) - py;
            alive = alive && !(dx * dx + dy * dy < md2i);
        }
        const unsigned long long bal = __ballot(alive);   // (b)
        if (lane == 0) s_w[wave] = (unsigned)__popcll(bal);
        __syncthreads();
        int off = 0, tot = 0;
        for (int w2 = 0; w2 < GF_T / 64; w2++) { const int c = (int)s_w[w2]; off += w2 < wave ? c : 0; tot += c; }
        if (alive) s_surv[off + __popcll(bal & ((1ull << lane) - 1ull))] = p;
        __syncthreads();
        if (wave == 0) {                             // (c)
            int nn = 0;                              // corners accepted in this chunk: s_new[0 .. nn)
            for (int sub = 0; sub < tot && na + nn < limit; sub += 64) {
                const bool valid = sub + lane < tot;
                const unsigned sp = valid ? s_surv[sub + lane] : 0u;
                const int sx = (int)(sp & 0xffffu), sy = (int)(sp >> 16);
                bool live = valid;
                for (int a = 0; a < nn; a++) {
                    const unsigned q = s_new[a];
                    const int dx = (int)(q & 0xffffu) - sx, dy = (int)(q >> 16) - sy;
                    live = live && !(dx * dx + dy * dy < md2i);
                }
                unsigned long long lm = __ballot(live);
                while (lm && na + nn < limit) {
                    const int j = __builtin_ctzll(lm);
                    const unsigned pj = (unsigned)__shfl((int)sp, j, 64);
                    if (lane == 0) { s_new[nn] = pj; acc[na + nn] = pj; }
                    nn++;
                    const int dx = (int)(pj & 0xffffu) - sx, dy = (int)(pj >> 16) - sy;
                    lm &= ~__ballot(dx * dx + dy * dy < md2i);   // (lane j itself: distance 0, min_dist >= 1)
                }
                gf_wave_sync();
            }
            if (lane == 0) s_w[GF_T / 64] = (unsigned)(na + nn);
        }
        __syncthreads();
        na = (int)s_w[GF_T / 64];
    }
    return na;
}

// PER_REQ (a group of trackers, more than one request with cap_dev): cap_dev holds one word per request; otherwise the one word of the
// single request - the form every single call and a lone tracker's step launch, whose code is what it was
template <bool PER_REQ>
__global__ __launch_bounds__(GF_T) void k_gftt_pick_frame(const int* __restrict__ recs, const float* __restrict__ cand_val, const unsigned* __restrict__ cand_idx,
                                                          const unsigned* __restrict__ info, unsigned long long* __restrict__ gkeys, int cap, double quality,
                                                          double min_dist, int unlimited, int* __restrict__ out_xy, int* __restrict__ out_count,
                                                          int* __restrict__ stats, const int* __restrict__ cap_dev) {
    extern __shared__ unsigned long long gf_lds[];
    unsigned long long* lkey = gf_lds;                    // [GF_CAP]
    unsigned* s_surv = (unsigned*)(lkey + GF_CAP);        // [GF_T]
    unsigned* s_new = s_surv + GF_T;                      // [GF_T]
    unsigned* s_w = s_new + GF_T;                         // [32]: per-wavefront counts, [16] accepted so far, [20] keys
    BACKEND_PRIO();
    const int req = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const int* __restrict__ r = recs + CELL_STRIDE * req;
    const int cw = r[2];
    const size_t off = gf_list_off(r);
    const float* __restrict__ cv = cand_val + off;
    const unsigned* __restrict__ ci = cand_idx + off;
    unsigned long long* gk = gkeys + off;
    const int nraw = (int)info[2 * req + 1];
    const float thr = (float)((double)f32_unkey(info[2 * req]) * quality);
    if (tid == 0) s_w[20] = 0;
    __syncthreads();
    for (int base = 0; base < nraw; base += GF_T) {   // step 1; the place of a key among the keys is whatever the atomic gives: the sort follows
        const int i = base + tid;
        float v = 0.f; unsigned px = 0;
        if (i < nraw) { v = cv[i]; px = ci[i]; }
        const bool keep = i < nraw && v > thr;
        const unsigned long long bal = __ballot(keep);
        if (bal) {
            unsigned b0 = 0;
            if (lane == 0) b0 = atomicAdd(&s_w[20], (unsigned)__popcll(bal));
            b0 = __shfl(b0, 0, 64);
            if (keep) {
                const unsigned slot = b0 + (unsigned)__popcll(bal & ((1ull << lane) - 1ull));
                const int y = (int)px / cw;
                const unsigned long long key = ((unsigned long long)__float_as_uint(v) << 32) | ((unsigned)y << 16) | (unsigned)((int)px - y * cw);
                if (slot < (unsigned)GF_CAP) lkey[slot] = key; else gk[slot] = key;
            }
        }
    }
    __syncthreads();
    const int n = (int)s_w[20];
    const bool use_dist = min_dist >= 1.0;
    const double md2 = min_dist * min_dist;
    const int md2i = (int)(md2 < 2.0e9 ? ceil(md2) : 2.0e9);
    // cap_dev (the tracker's chain): the number of corners wanted is known only on the device - clamped to the list's capacity `cap`, which
    // still places the list; 0 selects nothing
    int want = cap;
    if (cap_dev) { const int c = PER_REQ ? cap_dev[req] : *cap_dev; want = c < 0 ? 0 : (c < cap ? c : cap); }
    const int limit = unlimited ? want + 1 : want;
    int na;
    if (n <= GF_CAP) {
        if (n > 1) gf_sort<true>(lkey, n, tid);
        na = use_dist ? gf_walk(lkey, n, limit, md2i, s_surv, s_new, s_w, tid) : (n < limit ? n : limit);
    } else {
        for (int i = tid; i < GF_CAP; i += GF_T) gk[i] = lkey[i];
        __syncthreads();
        gf_sort<false>(gk, n, tid);
        na = use_dist ? gf_walk(gk, n, limit, md2i, s_surv, s_new, s_w, tid) : (n < limit ? n : limit);
    }
    const unsigned long long* keys = n <= GF_CAP ? lkey : gk;
    const bool over = unlimited && na > want;
    if (!over)
        for (int i = tid; i < na; i += GF_T) {
            typedef unsigned __attribute__((may_alias)) acc_t;
            const unsigned a = use_dist ? ((const acc_t*)keys)[i] : (unsigned)keys[i];   // (y << 16) | x
            *(int2*)&out_xy[((size_t)req * cap + i) * 2] = make_int2((int)(a & 0xffffu), (int)(a >> 16));
        }
    if (tid == 0) { out_count[req] = over ? -1 : na; stats[2 * req] = n; stats[2 * req + 1] = n > GF_CAP ? n : 0; }
}

int gftt_frame_grid_x(int w, int h) { const int tx = (w + 31) / 32, ty = (h + 31) / 32; return 8 * ((ty + 7) / 8) * tx; }
hipError_t launch_gftt_frame(hipStream_t s, const uint8_t* slots, const PyrLayout& L, const int* d_recs, int n_req, int grid_x, int cap, double quality,
                             double min_dist, int unlimited, const GfttExt* X, const uint8_t* d_mask, float* d_val, unsigned* d_idx, unsigned* d_info,
                             unsigned long long* d_keys, int* d_out_xy, int* d_out_count, int* d_stats, const int* d_cap) {
    if (!slots || !d_recs || !d_val || !d_idx || !d_info || !d_keys || !d_out_xy || !d_out_count || !d_stats || n_req < 1 || n_req > 65535 || grid_x < 8 || (grid_x & 7) ||
        cap < 1 || cap > GF_CAP || (X && !gftt_ext_ok(*X)) || (d_mask && !X)) return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(d_info, 0, 2 * sizeof(unsigned) * n_req, s);
    if (e != hipSuccess) return e;
    { ProfScope ps(K_GFTT_CAND, s);
    if (X) hipLaunchKernelGGL(k_gftt_cand_general_frame, dim3(grid_x, n_req), dim3(256), gfttg_lds_bytes(X->bs), s, slots, L, d_recs, d_val, d_idx, d_info, quality, *X, d_mask);
    else hipLaunchKernelGGL(k_gftt_cand_frame, dim3(grid_x, n_req), dim3(256), 0, s, slots, L, d_recs, d_val, d_idx, d_info, quality); }
    ProfScope ps2(K_GFTT_PICK, s);
    if (d_cap && n_req > 1)
        hipLaunchKernelGGL(k_gftt_pick_frame<true>, dim3(n_req), dim3(GF_T), GF_LDS, s, d_recs, d_val, d_idx, d_info, d_keys, cap, quality, min_dist, unlimited, d_out_xy,
                           d_out_count, d_stats, d_cap);
    else
        hipLaunchKernelGGL(k_gftt_pick_frame<false>, dim3(n_req), dim3(GF_T), GF_LDS, s, d_recs, d_val, d_idx, d_info, d_keys, cap, quality, min_dist, unlimited, d_out_xy,
                           d_out_count, d_stats, d_cap);
    return hipGetLastError();
}

// =========================================================================================================
// ShiTomasiFeatureExtractor (in-repo arithmetic, float64)
// =========================================================================================================
__global__ __launch_bounds__(256) void k_st_resp(const uint8_t* __restrict__ slots, PyrLayout L,
                                                 const int* __restrict__ cells, double* __restrict__ resp,
                                                 unsigned long long* __restrict__ cellmax) {
    __shared__ double sH[34 * 34 * 3];
    __shared__ unsigned long long smax[4];
    const int cell = blockIdx.z;
    const int cx0 = cells[CELL_STRIDE * cell], cy0 = cells[CELL_STRIDE * cell + 1], cw = cells[CELL_STRIDE * cell + 2], ch = cells[CELL_STRIDE * cell + 3];
    const int tx0 = blockIdx.x * 32, ty0 = blockIdx.y * 32;
    if (tx0 >= cw || ty0 >= ch) return;
    const uint8_t* img = level_origin(slots + (size_t)cells[CELL_STRIDE * cell + 4] * L.slot_bytes, L, 0);
    const int st = L.stride[0];
    for (int idx = threadIdx.x; idx < 34 * 34; idx += 256) {
        const int hy = idx / 34, hx = idx - hy * 34;
        const int lx = reflect101(tx0 - 1 + hx, cw), ly = reflect101(ty0 - 1 + hy, ch);
        double gx = 0.0, gy = 0.0;   // Frame.cpp:58-86: zero on the cell border
        if (lx >= 1 && lx < cw - 1 && ly >= 1 && ly < ch - 1) {
            const uint8_t* p = img + (ptrdiff_t)(cy0 + ly) * st + (cx0 + lx);
            gx = 1. / 2. * (double)(int8_t)p[1] - 1. / 2. * (double)(int8_t)p[-1];     // quirk Q1: signed char view
            gy = 1. / 2. * (double)(int8_t)p[st] - 1. / 2. * (double)(int8_t)p[-st];
        }
        sH[idx * 3 + 0] = gx * gx; sH[idx * 3 + 1] = gy * gy; sH[idx * 3 + 2] = gx * gy;
    }
    __syncthreads();
    unsigned long long mk = 0;
    const double inv9 = 1.0 / 9.0;
    for (int idx = threadIdx.x; idx < 32 * 32; idx += 256) {
        const int oy = idx >> 5, ox = idx & 31;
        const int x = tx0 + ox, y = ty0 + oy;
        if (x >= cw || y >= ch) continue;
        double R = 0.0;
        if (x < cw - 1) {   // ShiTomasiFeatureExtractor.cpp:58 skips the last column
            double s0 = 0, s1 = 0, s2 = 0;
#pragma unroll
            for (int j = 0; j < 3; j++)
#pragma unroll
                for (int i = 0; i < 3; i++) {
                    const double* h = &sH[((oy + j) * 34 + (ox + i)) * 3];
                    s0 += h[0]; s1 += h[1]; s2 += h[2];
                }
            const double Ixx = s0 * inv9, Iyy = s1 * inv9, Ixy = s2 * inv9;
            const double B = -Ixx - Iyy;
            const double C = Ixx * Iyy - Ixy * Ixy;
            const double disc = sqrt(B * B - 4 * C);
            const double l1 = (-B + disc) / 2, l2 = (-B - disc) / 2;
            R = (l2 < l1) ? l2 : l1;   // std::min(l1, l2)
        }
        resp[(size_t)cell * CELL_PIX + y * cw + x] = R;
        if (R == R) { const unsigned long long k = f64_key(R); mk = k > mk ? k : mk; }
    }
    mk = wave_max_u64(mk);
    if ((threadIdx.x & 63) == 0) smax[threadIdx.x >> 6] = mk;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long m = smax[0];
        for (int i = 1; i < 4; i++) m = smax[i] > m ? smax[i] : m;
        atomicMax(&cellmax[cell], m);
    }
}

constexpr int ST_CAP = 8192;
constexpr size_t ST_SELECT_SHM = ST_CAP * 12 + 16 * 12 + 16;
__global__ __launch_bounds__(1024) void k_st_select(const int* __restrict__ cells, const double* __restrict__ resp,
                                                    const unsigned long long* __restrict__ cellmax, int max_feats,
                                                    double quality, int* __restrict__ out_xy,
                                                    double* __restrict__ out_score, int* __restrict__ out_count,
                                                    int* __restrict__ flags, unsigned* __restrict__ spill_all) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned* spill = spill_all + (size_t)blockIdx.x * CELL_PIX;   // candidates beyond ST_CAP: pixel indices in HBM (bit 31 = taken), see k_gftt_select
    unsigned long long* ckey = (unsigned long long*)smem;              // ST_CAP: ordered score key, 0 = dead
    unsigned* cidx = (unsigned*)(smem + ST_CAP * 8);                   // ST_CAP
    unsigned long long* wk = (unsigned long long*)(smem + ST_CAP * 12);// 16
    unsigned* wi = (unsigned*)(smem + ST_CAP * 12 + 16 * 8);           // 16
    int* scount = (int*)(smem + ST_CAP * 12 + 16 * 12);
    const int cell = blockIdx.x;
    const int cw = cells[CELL_STRIDE * cell + 2], ch = cells[CELL_STRIDE * cell + 3];
    const double* R = resp + (size_t)cell * CELL_PIX;
    const int tid = threadIdx.x;
    if (tid == 0) *scount = 0;
    __syncthreads();
    const double rmax = f64_unkey(cellmax[cell]);
    const double thr = rmax * quality;
    for (int idx = tid; idx < cw * ch; idx += 1024) {
        const double v = R[idx];
        if (v > thr) {
            const int slot = atomicAdd(scount, 1);
            if (slot < ST_CAP) { ckey[slot] = f64_key(v); cidx[slot] = (unsigned)idx; }
            else spill[slot - ST_CAP] = (unsigned)idx;
        }
    }
    __threadfence_block();
    __syncthreads();
    const int ncand = *scount;
    int nacc = 0;
    for (int it = 0; it < max_feats; it++) {
        // best = highest score, ties -> lowest raster index (stable sort of a raster-ordered list)
        unsigned long long bk = 0; unsigned bi = 0xffffffffu;
        for (int i = tid; i < ncand; i += 1024) {
            unsigned long long k; unsigned ci;
            if (i < ST_CAP) { k = ckey[i]; ci = cidx[i]; }
            else { ci = spill[i - ST_CAP]; k = (ci >> 31) ? 0ull : f64_key(R[ci]); }
            if (k > bk || (k == bk && k != 0 && ci < bi)) { bk = k; bi = ci; }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned long long tk = __shfl_xor(bk, o, 64);
            const unsigned ti = __shfl_xor(bi, o, 64);
            if (tk > bk || (tk == bk && ti < bi)) { bk = tk; bi = ti; }
        }
        if ((tid & 63) == 0) { wk[tid >> 6] = bk; wi[tid >> 6] = bi; }
        __syncthreads();
        bk = wk[0]; bi = wi[0];
#pragma unroll
        for (int i = 1; i < 16; i++)
            if (wk[i] > bk || (wk[i] == bk && wi[i] < bi)) { bk = wk[i]; bi = wi[i]; }
        if (bk == 0) break;
        if (tid == 0) {
            out_xy[((size_t)cell * max_feats + nacc) * 2] = (int)(bi % (unsigned)cw);
            out_xy[((size_t)cell * max_feats + nacc) * 2 + 1] = (int)(bi / (unsigned)cw);
            out_score[(size_t)cell * max_feats + nacc] = f64_unkey(bk);
        }
        nacc++;
        for (int i = tid; i < ncand; i += 1024) {
            if (i < ST_CAP) { if (cidx[i] == bi) ckey[i] = 0; }
            else if (spill[i - ST_CAP] == bi) spill[i - ST_CAP] = bi | 0x80000000u;
        }
        __threadfence_block();
        __syncthreads();
    }
    if (tid == 0) out_count[cell] = nacc;
}

hipError_t launch_shitomasi(hipStream_t s, const uint8_t* slots, const PyrLayout& L, const int* d_cells, int n_cells,
                            int max_per_cell, double quality, double* d_resp, unsigned long long* d_cellmax,
                            int* d_out_xy, double* d_out_score, int* d_out_count, int* d_flags, unsigned* d_spill) {
    if (!slots || !d_cells || !d_resp || !d_cellmax || !d_out_xy || !d_out_score || !d_out_count || !d_flags || !d_spill || n_cells < 1 || max_per_cell < 1) return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(d_cellmax, 0, sizeof(unsigned long long) * n_cells, s);
    if (e != hipSuccess) return e;
    { ProfScope ps(K_ST_RESP, s);
    hipLaunchKernelGGL(k_st_resp, dim3(8, 8, n_cells), dim3(256), 0, s, slots, L, d_cells, d_resp, d_cellmax); }
    ProfScope ps2(K_ST_SELECT, s);
    const size_t shm = ST_SELECT_SHM;
    hipLaunchKernelGGL(k_st_select, dim3(n_cells), dim3(1024), shm, s, d_cells, d_resp, d_cellmax, max_per_cell,
                       quality, d_out_xy, d_out_score, d_out_count, d_flags, d_spill);
    return hipGetLastError();
}

// Kernels that need more than the default 64 KB of dynamic LDS opt in per DEVICE (function attributes are per device in HIP):
// called by pmv_ctx_create after hipSetDevice, so a second context on another GPU of the same process is set up as well.
hipError_t frontend_prepare_device() {
    if (hipError_t e = hipFuncSetAttribute((const void*)k_st_select, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ST_SELECT_SHM)) return e;
    if (hipError_t e = hipFuncSetAttribute((const void*)k_gftt_pick_frame<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)GF_LDS)) return e;
    return hipFuncSetAttribute((const void*)k_gftt_pick_frame<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)GF_LDS);
}

}  // namespace pmv
