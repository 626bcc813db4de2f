// pmv_detect_gftt_refill / pmv_batch_detect_gftt_refill: FeatureTracker::setMask of a KLT loop on the device (contract: include/pmv_hip.h;
// statement by statement: tests/twin/refill_twin.cpp). The tracks are ordered (priority descending, index ascending), walked, and a track is
// kept when its position is allowed by the base mask and lies in no filled cv::circle of a track kept before it; the kept tracks' discs are
// cleared in the region's packed mask, which the general pass-1 kernel of pmv_detect_gftt_frame then reads. Two kernels, no atomics on
// global memory, every global byte written once by one thread.
//   The disc is cv's Circle() with fill, not x^2 + y^2 <= r^2: pixel (x, y) lies in the disc of c iff |y - cy| <= r and
//   |x - cx| <= hw[|y - cy|], hw = the half-width table the HOST computes with the literal loop (refill_halfwidths).
#include "pmv_device.h"
#include "pmv_prof.h"
#include "pmv_gfsort.h"

namespace pmv {

namespace {

constexpr int RS_CAP = REFILL_MAX_TRACKS;
// keys | positions, later the kept list | keep bytes | survivors of a chunk (index << 32 | position) | its accepted positions | half-widths | counters
constexpr size_t RS_LDS = (size_t)RS_CAP * 8 + (size_t)RS_CAP * 4 + (size_t)RS_CAP + (size_t)GF_T * 8 + (size_t)GF_T * 4 + (size_t)REFILL_HW * 4 + 64 * 4;
constexpr int RS_CHUNK = 256, RS_PARTS = GF_T / RS_CHUNK;   // ranks per step of the walk; the threads that share one rank in (a)
constexpr unsigned RS_DEAD = 0xffffffffu;   // the position of a track on a base byte other than 255: no frame has a row 65535

// a in disc(b) <=> b in disc(a): the test looks at |dx| and |dy| only. Almost every pair of a frame is further apart than the radius in x
// or in y: the table in LDS is read only when some lane of the wavefront has a pair inside the (2r + 1)^2 box, a wave-uniform branch -
// call it from code that the wavefront runs together. Nothing short-circuits, so the compiler can batch the loads of an unrolled loop.
__device__ __forceinline__ bool rf_in_disc(unsigned a, unsigned b, int r, const int* __restrict__ hw) {
    int dx = (int)(a & 0xffffu) - (int)(b & 0xffffu), dy = (int)(a >> 16) - (int)(b >> 16);
    dx = dx < 0 ? -dx : dx; dy = dy < 0 ? -dy : dy;
    const bool box = dx <= r && dy <= r;
    bool hit = false;
    if (__ballot(box)) hit = box && dx <= hw[dy & (REFILL_HW - 1)];
    return hit;
}
// b against the n positions at list (16-byte aligned), four at a time
__device__ __forceinline__ bool rf_in_any(const unsigned* __restrict__ list, int n, unsigned b, int r, const int* __restrict__ hw) {
    int hit = 0, a = 0;   // (an int, so that the four tests are joined without a short-circuit)
    for (; a + 4 <= n; a += 4) {
        const uint4 q = *(const uint4*)(list + a);
        hit |= (int)rf_in_disc(q.x, b, r, hw) | (int)rf_in_disc(q.y, b, r, hw) | (int)rf_in_disc(q.z, b, r, hw) | (int)rf_in_disc(q.w, b, r, hw);
    }
    for (; a < n; a++) hit |= (int)rf_in_disc(list[a], b, r, hw);
    return hit != 0;
}

// One 1024-thread workgroup per request.
//   1. Track i becomes the key (priority biased to unsigned) << 32 | (0xffffffff - i): unique, and its descending order is priority
//      descending, then index ascending. Keys and packed positions (y << 16 | x) live in LDS.
//   2. gf_sort, the network of k_gftt_pick_frame: any n, no padding. Then key i is replaced by (index << 32 | position) of rank i.
//   3. The walk of k_gftt_pick_frame's step 3 with the disc test in the place of the distance test and no limit: chunks of 256 ranks,
//      (a) every record against the tracks kept from earlier chunks - four threads a record, a quarter of the kept list each, their
//      verdicts joined through the wavefronts' ballots -, (b) the survivors compacted in order, (c) wavefront 0 takes them 64 at a
//      time - each against the tracks kept earlier in this chunk, then it accepts the first live lane and kills the lanes in its disc until
//      none is left. (c) is the serial part, one wavefront: the chunk is short so that most tests are made in (a), by all sixteen.
//      setMask keeps a track iff no track kept BEFORE it holds it in its disc; the fixed-point argument written above
//      k_gftt_pick_frame carries over unchanged because the relation is symmetric ("i lies in disc(j)" depends on |dx| and |dy| only, so it
//      is "j lies in disc(i)"): the kept set is the set of records that outrank every KEPT record whose disc they lie in, the top live
//      record is always such a record, and a kill is only ever made by a kept one. A track on a base byte other than 255 is never live and
//      kills nothing.
//   The keep bytes (input order) are gathered in LDS and written once, as dwords; the kept positions go to HBM in rank order.
__global__ __launch_bounds__(GF_T) void k_track_select(const RefillRec* __restrict__ recs, const unsigned* __restrict__ pos, const int* __restrict__ prio,
                                                       const uint8_t* __restrict__ flag, const uint8_t* __restrict__ hwtab, uint8_t* __restrict__ keep,
                                                       unsigned* __restrict__ kept, int* __restrict__ nkept) {
    extern __shared__ unsigned long long rs_lds[];
    unsigned long long* keys = rs_lds;                         // [RS_CAP]
    unsigned* s_pos = (unsigned*)(keys + RS_CAP);              // [RS_CAP] positions by index; after step 2 the kept list
    uint8_t* s_keep = (uint8_t*)(s_pos + RS_CAP);              // [RS_CAP]
    unsigned long long* s_surv = (unsigned long long*)(s_keep + RS_CAP);   // [GF_T]
    unsigned* s_new = (unsigned*)(s_surv + GF_T);              // [GF_T]
    int* s_hw = (int*)(s_new + GF_T);                          // [REFILL_HW]
    unsigned* s_w = (unsigned*)(s_hw + REFILL_HW);             // [64]: per-wavefront counts, [16] kept so far, [32 ..) the wavefronts' ballots of (a)
    unsigned long long* s_bal = (unsigned long long*)(s_w + 32);   // [GF_T / 64]
    BACKEND_PRIO();
    const int req = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const RefillRec R = recs[req];
    const int n = R.n < RS_CAP ? R.n : RS_CAP, radius = R.radius;
    const size_t off = (size_t)R.trk_off;
    for (int i = tid; i < REFILL_HW; i += GF_T) s_hw[i] = i <= radius ? (int)hwtab[(size_t)req * REFILL_HW + i] : -1;
    for (int i = tid; i < (n + 3) / 4; i += GF_T) ((unsigned*)s_keep)[i] = 0u;
    for (int i = tid; i < n; i += GF_T) {
        keys[i] = ((unsigned long long)((unsigned)prio[off + i] ^ 0x80000000u) << 32) | (0xffffffffu - (unsigned)i);
        s_pos[i] = flag[off + i] ? pos[off + i] : RS_DEAD;
    }
    __syncthreads();
    if (n > 1) gf_sort<true>(keys, n, tid);
    for (int i = tid; i < n; i += GF_T) {
        const unsigned idx = 0xffffffffu - (unsigned)keys[i];
        keys[i] = ((unsigned long long)idx << 32) | s_pos[idx];
    }
    __syncthreads();
    unsigned* acc = s_pos;                                     // (every position has moved into its key)
    int na = 0;
    constexpr int CW = RS_CHUNK / 64;                          // wavefronts that hold one copy of the chunk
    for (int base = 0; base < n; base += RS_CHUNK) {
        const int i = base + (tid & (RS_CHUNK - 1)), part = tid / RS_CHUNK;
        const unsigned long long rec = i < n ? keys[i] : (unsigned long long)RS_DEAD;
        const unsigned p = (unsigned)rec;
        const int share = ((na + 4 * RS_PARTS - 1) / (4 * RS_PARTS)) * 4, a0 = part * share;   // (a): this part's quarter of the kept list
        const bool hit = rf_in_any(acc + a0, na - a0 < share ? (na - a0 < 0 ? 0 : na - a0) : share, p, radius, s_hw);
        const unsigned long long hb = __ballot(hit);
        if (lane == 0) s_bal[wave] = hb;
        __syncthreads();
        bool alive = false;
        if (wave < CW) {                                       // (b)
            unsigned long long dead = 0;
            for (int q = 0; q < RS_PARTS; q++) dead |= s_bal[wave + q * CW];
            alive = p != RS_DEAD && !((dead >> lane) & 1ull);
        }
        const unsigned long long bal = __ballot(alive);
        if (lane == 0 && wave < CW) s_w[wave] = (unsigned)__popcll(bal);
        __syncthreads();
        int o = 0, tot = 0;
        for (int w2 = 0; w2 < CW; w2++) { const int c = (int)s_w[w2]; o += w2 < wave ? c : 0; tot += c; }
        if (alive) s_surv[o + __popcll(bal & ((1ull << lane) - 1ull))] = rec;
        __syncthreads();
        if (wave == 0) {                                       // (c)
            int nn = 0;                                        // tracks kept in this chunk: s_new[0 .. nn)
            for (int sub = 0; sub < tot; sub += 64) {
                const bool valid = sub + lane < tot;
                const unsigned long long sr = valid ? s_surv[sub + lane] : (unsigned long long)RS_DEAD;
                const unsigned sp = (unsigned)sr, si = (unsigned)(sr >> 32);
                const bool held = rf_in_any(s_new, nn, sp, radius, s_hw);   // (every lane: the test has a wave-uniform branch)
                unsigned long long lm = __ballot(valid && !held);
                while (lm) {
                    const int j = __builtin_ctzll(lm);
                    const unsigned pj = (unsigned)__builtin_amdgcn_readlane((int)sp, j);
                    if (lane == j) { s_new[nn] = sp; acc[na + nn] = sp; s_keep[si] = 1; }
                    nn++;
                    lm &= ~__ballot(rf_in_disc(pj, sp, radius, s_hw));   // (lane j itself: offsets 0, 0 <= hw[0])
                }
                gf_wave_sync();
            }
            if (lane == 0) s_w[GF_T / 64] = (unsigned)(na + nn);
        }
        __syncthreads();
        na = (int)s_w[GF_T / 64];
    }
    for (int i = tid; i < (n + 3) / 4; i += GF_T) ((unsigned*)(keep + off))[i] = ((const unsigned*)s_keep)[i];
    for (int i = tid; i < na; i += GF_T) kept[off + i] = acc[i];
    if (tid == 0) nkept[req] = na;
}

// The region's packed mask, cw * ch tight bytes at mask_off: a thread owns aligned dwords of it (mask_off is a multiple of 4 and the index
// is the linear index over the tight sub-view, so this holds for any cw) and writes each once - from 255 or from the uploaded base bytes,
// with the bytes inside a kept disc cleared. The up to three bytes behind the region's last one belong to the same request's padding.
// A workgroup owns RP_BYTES consecutive bytes, a band of rows; it first bins the kept tracks whose disc reaches the band into LDS (their
// order does not matter: a byte is cleared if ANY disc holds it), so a byte is tested against tens of tracks, not all of them.
constexpr int RP_T = 256, RP_DW = 4, RP_BYTES = RP_T * RP_DW * 4;
__global__ __launch_bounds__(RP_T) void k_track_paint(const RefillRec* __restrict__ recs, const uint8_t* __restrict__ hwtab, const unsigned* __restrict__ kept,
                                                      const int* __restrict__ nkept, uint8_t* __restrict__ mask) {
    __shared__ unsigned s_bin[REFILL_MAX_TRACKS];
    __shared__ int s_hw[REFILL_HW];
    __shared__ unsigned s_n;
    BACKEND_PRIO();
    const int req = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
    const RefillRec R = recs[req];
    // (a region has fewer than 2^31 bytes - gftt_frame_check - and the grid covers the largest region of the launch: 32-bit indices)
    const unsigned total = (unsigned)R.cw * (unsigned)R.ch, b0 = blockIdx.x * (unsigned)RP_BYTES, cw = (unsigned)R.cw;
    if (b0 >= total) return;                                   // (the whole workgroup, before its first barrier)
    const unsigned b1 = (total - b0 > (unsigned)RP_BYTES ? b0 + RP_BYTES : total) - 1u;
    const int radius = R.radius, ylo = R.y0 + (int)(b0 / cw) - radius, yhi = R.y0 + (int)(b1 / cw) + radius;
    for (int i = tid; i < REFILL_HW; i += RP_T) s_hw[i] = i <= radius ? (int)hwtab[(size_t)req * REFILL_HW + i] : -1;
    if (tid == 0) s_n = 0;
    __syncthreads();
    const int nk = nkept[req];
    const unsigned* __restrict__ kl = kept + (size_t)R.trk_off;
    for (int base = 0; base < nk; base += RP_T) {
        const int i = base + tid;
        const unsigned k = i < nk ? kl[i] : 0u;
        const int ky = (int)(k >> 16);
        const bool reach = i < nk && ky >= ylo && ky <= yhi;
        const unsigned long long bal = __ballot(reach);
        if (bal) {
            unsigned s0 = 0;
            if (lane == 0) s0 = atomicAdd(&s_n, (unsigned)__popcll(bal));
            s0 = __shfl(s0, 0, 64);
            if (reach) s_bin[s0 + (unsigned)__popcll(bal & ((1ull << lane) - 1ull))] = k;
        }
    }
    __syncthreads();
    const int nb = (int)s_n;
    unsigned* __restrict__ m32 = (unsigned*)(mask + (size_t)R.mask_off);
    for (int e = 0; e < RP_DW; e++) {
        const unsigned li = b0 + 4u * (unsigned)(e * RP_T + tid);   // linear index of the dword's first byte
        if (li >= total) break;
        unsigned v = R.has_base ? m32[li >> 2] : 0xffffffffu;
        unsigned q[4];
        unsigned ly = li / cw, lx = li - ly * cw;
#pragma unroll
        for (int b = 0; b < 4; b++) {                          // (a byte behind the region's end gets a position too; it is padding)
            q[b] = ((unsigned)R.y0 + ly) << 16 | ((unsigned)R.x0 + lx);
            if (++lx == cw) { lx = 0; ly++; }
        }
        for (int t = 0; t < nb; t++) {
            const unsigned k = s_bin[t];
#pragma unroll
            for (int b = 0; b < 4; b++)
                if (rf_in_disc(k, q[b], radius, s_hw)) v &= ~(0xffu << (8 * b));
        }
        m32[li >> 2] = v;
    }
}

}  // namespace

void refill_halfwidths(int radius, uint8_t out[REFILL_HW]) {
    int hw[REFILL_HW];
    for (int d = 0; d < REFILL_HW; d++) hw[d] = d <= radius ? 0 : 255;
    // Circle() of drawing.cpp: at every step it paints rows cy -+ dy with the span cx -+ dx and rows cy -+ dx with the span cx -+ dy
    int err = 0, dx = radius, dy = 0, plus = 1, minus = (radius << 1) - 1;
    while (dx >= dy) {
        hw[dy] = hw[dy] > dx ? hw[dy] : dx;
        hw[dx] = hw[dx] > dy ? hw[dx] : dy;
        dy++;
        err += plus;
        plus += 2;
        const int mask = (err <= 0) - 1;
        err -= minus & mask;
        dx += mask;
        minus -= mask & 2;
    }
    for (int d = 0; d < REFILL_HW; d++) out[d] = (uint8_t)hw[d];
}

hipError_t launch_track_refill(hipStream_t s, const RefillRec* d_recs, int n_req, size_t max_bytes, const unsigned* d_pos, const int* d_prio, const uint8_t* d_flag,
                               const uint8_t* d_hw, uint8_t* d_keep, unsigned* d_kept, int* d_nkept, uint8_t* d_mask) {
    const size_t gx = (max_bytes + RP_BYTES - 1) / RP_BYTES;
    if (!d_recs || !d_pos || !d_prio || !d_flag || !d_hw || !d_keep || !d_kept || !d_nkept || !d_mask || n_req < 1 || n_req > 65535 || max_bytes < 1 || gx > 0x7fffffffu)
        return hipErrorInvalidValue;
    { ProfScope ps(K_GFTT_PICK, s);
    hipLaunchKernelGGL(k_track_select, dim3(n_req), dim3(GF_T), RS_LDS, s, d_recs, d_pos, d_prio, d_flag, d_hw, d_keep, d_kept, d_nkept); }
    ProfScope ps2(K_GFTT_CAND, s);
    hipLaunchKernelGGL(k_track_paint, dim3((unsigned)gx, n_req), dim3(RP_T), 0, s, d_recs, d_hw, d_kept, d_nkept, d_mask);
    return hipGetLastError();
}

hipError_t refill_prepare_device() {
    return hipFuncSetAttribute((const void*)k_track_select, hipFuncAttributeMaxDynamicSharedMemorySize, (int)RS_LDS);
}

}  // namespace pmv
