// Shared declarations for the gfx950 kernels of the VO hot path (internal; the public boundary is include/pmv_hip.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pmv {

// ---- frame slot layout in HBM -------------------------------------------------------------------------
// Every pyramid level is stored with a PAD-pixel BORDER_REFLECT_101 frame on all four sides (cv::buildOpticalFlowPyramid
// pads by winSize=32; we pad by 64 so that the 64x64 LDS search tile of the LK kernel never leaves the buffer) and a
// row stride that is a multiple of 64 bytes, so every tile row starts dword-aligned and no kernel needs a border branch.
constexpr int PAD = 64;
constexpr int MAX_LEVELS = 5;   // maxLevel 4 -> levels 0..4
constexpr int LK_WIN = 32;       // the window k_lk / k_lk_batch are built around, and the default of pmv_set_lk_params

struct PyrLayout {
    int n_levels;                 // levels actually built = maxLevel + 1
    int w[MAX_LEVELS], h[MAX_LEVELS], stride[MAX_LEVELS];
    uint32_t off[MAX_LEVELS];     // byte offset of the padded level buffer inside the slot
    uint32_t gray_off;            // byte offset of pixel (0,0) of level 0: a frame is staged straight into the interior of its padded level 0 (row pitch stride[0])
    uint32_t slot_bytes;
};

static_assert(sizeof(PyrLayout) == 92, "PyrLayout: 23 dwords, the entry of a geometry table");

// ---- geometry table ---------------------------------------------------------------------------------------
// A batch may hold sequences of different frame sizes (the reference takes whatever cv::imread returns, Frame.cpp:31-42). Its batched
// launches then carry no PyrLayout of their own: the context keeps a small array of them in device memory, one entry per distinct frame
// size of the run (slot_bytes = the capacity pitch in every entry), written before the sequence threads start, and every track / request /
// frame record carries the index of its entry. The index is the same for the whole workgroup; it goes through readfirstlane, and the
// table is read through the constant address space, so the level dimensions, strides and offsets arrive by scalar loads and stay in
// scalar registers, exactly as the fields of a by-value kernel argument do (which is itself a scalar load from the kernarg segment).
typedef const __attribute__((address_space(4))) PyrLayout GeomEntry;
__device__ __forceinline__ GeomEntry& geom_entry(const PyrLayout* __restrict__ table, int index) {
#if defined(__HIP_DEVICE_COMPILE__)
    index = __builtin_amdgcn_readfirstlane(index);
#endif
    return ((GeomEntry*)(uintptr_t)table)[index];
}

__host__ __device__ inline int reflect101(int p, int len) {
    if (len == 1) return 0;
    while (p < 0 || p >= len) {
        if (p < 0) p = -p;
        else p = 2 * len - 2 - p;
    }
    return p;
}

// pointer to pixel (0,0) of a padded level
__host__ __device__ inline const uint8_t* level_origin(const uint8_t* slot, const PyrLayout& L, int l) {
    return slot + L.off[l] + (size_t)PAD * L.stride[l] + PAD;
}
__host__ __device__ inline uint8_t* level_origin(uint8_t* slot, const PyrLayout& L, int l) {
    return slot + L.off[l] + (size_t)PAD * L.stride[l] + PAD;
}

// (the same for an entry of the geometry table)
__host__ __device__ inline const uint8_t* level_origin(const uint8_t* slot, GeomEntry& L, int l) {
    return slot + L.off[l] + (size_t)PAD * L.stride[l] + PAD;
}
__host__ __device__ inline uint8_t* level_origin(uint8_t* slot, GeomEntry& L, int l) {
    return slot + L.off[l] + (size_t)PAD * L.stride[l] + PAD;
}

// ---- wave64 helpers -------------------------------------------------------------------------------------
__device__ inline long long wave_sum_i64(long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
// DPP all-reduce of an int32 over the wavefront (EXEC must be full): quad butterflies, half-row mirror, row mirror leave the
// 16-lane row sum in every lane of the row; the four row sums are combined on the scalar unit. ~10 instructions instead of
// six ds_bpermute round trips.
__device__ inline int wave_sum_i32(int v) {
    v += __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xf, 0xf, false);    // quad_perm [1,0,3,2]
    v += __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xf, 0xf, false);    // quad_perm [2,3,0,1]
    v += __builtin_amdgcn_update_dpp(0, v, 0x141, 0xf, 0xf, false);   // row_half_mirror
    v += __builtin_amdgcn_update_dpp(0, v, 0x140, 0xf, 0xf, false);   // row_mirror
    return __builtin_amdgcn_readlane(v, 0) + __builtin_amdgcn_readlane(v, 16) + __builtin_amdgcn_readlane(v, 32) +
           __builtin_amdgcn_readlane(v, 48);
}
// exact 64-bit sum of per-lane int32 partials: v = (v >> 16) * 65536 + (v & 0xffff), both halves summed in int32
__device__ inline long long wave_sum_i32_wide(int v) {
    const int hi = wave_sum_i32(v >> 16), lo = wave_sum_i32(v & 0xffff);
    return (long long)hi * 65536 + lo;
}
// Wavefront all-reduce of doubles on DPP row operations (a ds_bpermute shuffle of an f64 costs ~160 clk per step, a DPP move
// ~10): quad butterflies, row_half_mirror, row_mirror give every lane its 16-lane row sum; the four row sums are fetched with
// lane reads and added in a fixed order. Every lane receives the same bits.
__device__ inline double dpp_f64(double v, const int ctrl_sel) {
    int lo = __double2loint(v), hi = __double2hiint(v);
    switch (ctrl_sel) {   // the DPP control must be an immediate
    case 0: lo = __builtin_amdgcn_update_dpp(0, lo, 0xB1, 0xf, 0xf, false); hi = __builtin_amdgcn_update_dpp(0, hi, 0xB1, 0xf, 0xf, false); break;
    case 1: lo = __builtin_amdgcn_update_dpp(0, lo, 0x4E, 0xf, 0xf, false); hi = __builtin_amdgcn_update_dpp(0, hi, 0x4E, 0xf, 0xf, false); break;
    case 2: lo = __builtin_amdgcn_update_dpp(0, lo, 0x141, 0xf, 0xf, false); hi = __builtin_amdgcn_update_dpp(0, hi, 0x141, 0xf, 0xf, false); break;
    default: lo = __builtin_amdgcn_update_dpp(0, lo, 0x140, 0xf, 0xf, false); hi = __builtin_amdgcn_update_dpp(0, hi, 0x140, 0xf, 0xf, false); break;
    }
    return __hiloint2double(hi, lo);
}
__device__ inline double readlane_f64_c(double v, int l) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), l), __builtin_amdgcn_readlane(__double2loint(v), l));
}
__device__ inline double wave_sum_f64(double v) {
    v += dpp_f64(v, 0);   // quad_perm [1,0,3,2]
    v += dpp_f64(v, 1);   // quad_perm [2,3,0,1]
    v += dpp_f64(v, 2);   // row_half_mirror
    v += dpp_f64(v, 3);   // row_mirror
    return (readlane_f64_c(v, 0) + readlane_f64_c(v, 16)) + (readlane_f64_c(v, 32) + readlane_f64_c(v, 48));
}
// Wavefront all-reduce maximum of 64-bit keys on the same DPP row operations (the __shfl_xor form was six dependent pairs of ds_bpermute,
// ~1.5 k clk per call: most of a selection round of k_gftt_pick). Every lane receives the maximum.
__device__ inline unsigned long long dpp_u64(unsigned long long v, const int ctrl_sel) {
    int lo = (int)(unsigned)(v & 0xffffffffull), hi = (int)(unsigned)(v >> 32);
    switch (ctrl_sel) {
    case 0: lo = __builtin_amdgcn_update_dpp(0, lo, 0xB1, 0xf, 0xf, false); hi = __builtin_amdgcn_update_dpp(0, hi, 0xB1, 0xf, 0xf, false); break;
    case 1: lo = __builtin_amdgcn_update_dpp(0, lo, 0x4E, 0xf, 0xf, false); hi = __builtin_amdgcn_update_dpp(0, hi, 0x4E, 0xf, 0xf, false); break;
    case 2: lo = __builtin_amdgcn_update_dpp(0, lo, 0x141, 0xf, 0xf, false); hi = __builtin_amdgcn_update_dpp(0, hi, 0x141, 0xf, 0xf, false); break;
    default: lo = __builtin_amdgcn_update_dpp(0, lo, 0x140, 0xf, 0xf, false); hi = __builtin_amdgcn_update_dpp(0, hi, 0x140, 0xf, 0xf, false); break;
    }
    return ((unsigned long long)(unsigned)hi << 32) | (unsigned long long)(unsigned)lo;
}
// the same for 32-bit keys: one DPP move + v_max_u32 per step
__device__ inline unsigned wave_max_u32(unsigned v) {
    v = max(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xf, 0xf, false));
    v = max(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xf, 0xf, false));
    v = max(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x141, 0xf, 0xf, false));
    v = max(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x140, 0xf, 0xf, false));
    const unsigned a = (unsigned)__builtin_amdgcn_readlane((int)v, 0), b = (unsigned)__builtin_amdgcn_readlane((int)v, 16),
                   c = (unsigned)__builtin_amdgcn_readlane((int)v, 32), d = (unsigned)__builtin_amdgcn_readlane((int)v, 48);
    return max(max(a, b), max(c, d));
}
__device__ inline unsigned long long readlane_u64(unsigned long long v, int l) {
    return ((unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), l) << 32) |
           (unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v & 0xffffffffull), l);
}
__device__ inline unsigned long long wave_max_u64(unsigned long long v) {
    unsigned long long t;
    t = dpp_u64(v, 0); v = t > v ? t : v;   // quad_perm [1,0,3,2]
    t = dpp_u64(v, 1); v = t > v ? t : v;   // quad_perm [2,3,0,1]
    t = dpp_u64(v, 2); v = t > v ? t : v;   // row_half_mirror
    t = dpp_u64(v, 3); v = t > v ? t : v;   // row_mirror: every lane holds its 16-lane row's maximum
    const unsigned long long a = readlane_u64(v, 0), b = readlane_u64(v, 16), c = readlane_u64(v, 32), d = readlane_u64(v, 48);
    const unsigned long long ab = a > b ? a : b, cd = c > d ? c : d;
    return ab > cd ? ab : cd;
}

// ---- launch entry points (frontend.hip) -------------------------------------------------------------------
struct LKParams {
    int max_iter;     // 30
    float eps2;       // not used in float: see eps2d
    double eps2d;     // epsilon^2 = 1e-4
    float min_eig;    // 1e-4
    unsigned long long* stamps;   // optional (diagnostic): 16 shader-clock phase timers accumulated by the block of track 0
    int win;          // square window side (pmv_set_lk_params); k_lk / k_lk_batch are built for LK_WIN and serve only that
    int general;      // diagnostic (pmv_debug_lk_general): the general kernels also at win == LK_WIN
};

// one workgroup of k_lk_batch: everything it needs to start in ONE 32-byte record (the records sit in mapped pinned host memory: a wave's
// first load is a round trip over PCIe, and it used to make three dependent ones - block -> sequence -> coordinates)
struct __attribute__((aligned(32))) LKBlock {
    unsigned long long prev_off, next_off;   // byte offsets of the sequence's prev / next frame slot
    float x, y;                              // the track's position in the prev frame
    int track;                               // index into the concatenated result arrays
    int geom;                                // the sequence's entry of the geometry table
};
static_assert(sizeof(LKBlock) == 32, "LKBlock: one 32-byte record per workgroup");
// The extended calls (pmv_lk_track_ex / _fb): the two cv flag values, and the forward-backward mode as an internal third bit. A workgroup of
// the extended batch kernels reads, next to its LKBlock, the record of the same index in a second array: LKBlock keeps its 32 bytes and
// k_lk_batch its records. An LKX_FB record's back results go to index `track` of the launch's three back arrays.
// LKX_VOID (k_lk_batch_ex only): the record is beyond its list's count, which only the device knew when the launch was sized - its
// workgroup leaves without a load from the frames or a store. Set by k_klt_stereo_records alone.
constexpr int LKX_INIT = 4, LKX_EIG = 8, LKX_FB = 0x100, LKX_VOID = 0x200;
// `opt` of a record, 0 = none of it: the level caps of the two trips (pmv_lk_track_fb_levels' top levels, -1 = the slot's top) and the record's
// part in a predicted tracker step (pmv_klt_set_prediction) - `slot` names a (successes, successes wanted) pair of the launch's table d_pred:
// an LKP_COUNT record adds its forward status to the pair's first word, an LKP_GATE record reads the pair first and leaves at once when the
// first word has reached the second.
constexpr int LKP_NONE = 0, LKP_COUNT = 1, LKP_GATE = 2;
constexpr int lkext_opt(int top_f, int top_b, int slot, int mode) { return (top_f + 1) | ((top_b + 1) << 4) | ((slot + 1) << 8) | (mode << 28); }
struct __attribute__((aligned(16))) LKExt {
    float ix, iy;      // where the top level's search starts (level-0 coordinates), read with LKX_INIT
    int flags;         // LKX_*
    int opt;           // lkext_opt(..)
};
static_assert(sizeof(LKExt) == 16, "LKExt: one 16-byte record per workgroup");
static_assert(MAX_LEVELS + 1 <= 16, "lkext_opt: four bits per level cap");
// d_geom: the geometry table in device memory; every record's `geom` is an entry of it (the caller's business, on the host)
hipError_t launch_lk_batch(hipStream_t s, const uint8_t* slots, const LKBlock* d_blocks, int n_blocks, const PyrLayout* d_geom, const LKParams& P,
                           float* d_out_xy, uint8_t* d_status, float* d_err, uint16_t* d_work = nullptr);
// d_pred: n_pred (successes, successes wanted) pairs in device memory, named by the records' `opt`; null: no record names one
hipError_t launch_lk_batch_ex(hipStream_t s, const uint8_t* slots, const LKBlock* d_blocks, const LKExt* d_ext, int n_blocks, const PyrLayout* d_geom, const LKParams& P,
                              float* d_out_xy, uint8_t* d_status, float* d_err, uint16_t* d_work, float* d_back_xy, uint8_t* d_back_status, float* d_back_err,
                              int* d_pred = nullptr, int n_pred = 0);
hipError_t launch_bgr2gray(hipStream_t s, const uint8_t* d_bgr, int w, int h, int stride, uint8_t* d_gray);   // cv::cvtColor(BGR2GRAY), 8-bit
// one entry of a slot-list pyramid build (the feeder): destination slot and, for level 0, the device-visible address of the tight gray
// frame (HBM landing area or mapped pinned host memory), null = already staged in the slot; `geom` = the frame's entry of the geometry table
struct PyrListEntry { const uint8_t* src; int slot; int geom; };
// Range form: pyramid stages of the n consecutive slots first_slot .. first_slot + n - 1, all of ONE geometry L (level 0 from n tight gray
// frames at `tight`, null: in place).
hipError_t launch_pad_level0(hipStream_t s, uint8_t* slots, const PyrLayout& L, int first_slot, int n, const uint8_t* tight = nullptr);
// The same level 0 from tight BGR frames (3 w h bytes each), converted on the way (k_pad_level0_bgr).
hipError_t launch_pad_level0_bgr(hipStream_t s, uint8_t* slots, const PyrLayout& L, int first_slot, int n, const uint8_t* tight);
hipError_t launch_pyrdown(hipStream_t s, uint8_t* slots, const PyrLayout& L, int level_dst, int first_slot, int n);
// List form (the feeder): the n entries of a device-visible `list`, each with its own geometry d_geom[list[i].geom] (device memory). Lmax: a
// layout whose level count and level dimensions are, level by level, at least those of every entry in the list - it sizes the grid and the
// dynamic LDS; a workgroup whose rows lie outside its own frame returns as a whole before its first load or barrier, and so does every
// workgroup of k_pyrdown whose frame has no level `level_dst`. Every entry of a BGR list has a source.
hipError_t launch_pad_level0_list(hipStream_t s, uint8_t* slots, const PyrLayout* d_geom, const PyrLayout& Lmax, const PyrListEntry* list, int n);
hipError_t launch_pad_level0_bgr_list(hipStream_t s, uint8_t* slots, const PyrLayout* d_geom, const PyrLayout& Lmax, const PyrListEntry* list, int n);
hipError_t launch_pyrdown_list(hipStream_t s, uint8_t* slots, const PyrLayout* d_geom, const PyrLayout& Lmax, int level_dst, const PyrListEntry* list, int n);
// One entry of a PITCHED level-0 list (the upload class of a batch session): the source is read in place, `pitch` bytes from one row to the
// next (>= w for gray, >= 3 w for BGR; any value, any base alignment - rows are fetched as the aligned dwords that hold their bytes and no
// others, so nothing past the last row's last byte is read). Every entry has a source. The level-0 kernels take the list; the levels above
// are built by launch_pyrdown_list from a PyrListEntry list of the same slots.
struct PyrPitchEntry { const uint8_t* src; unsigned pitch; int slot; int geom; int reserved; };
static_assert(sizeof(PyrPitchEntry) == 24, "PyrPitchEntry: one 24-byte record per frame");
hipError_t launch_pad_level0_pitched(hipStream_t s, uint8_t* slots, const PyrLayout* d_geom, const PyrLayout& Lmax, const PyrPitchEntry* list, int n);
hipError_t launch_pad_level0_bgr_pitched(hipStream_t s, uint8_t* slots, const PyrLayout* d_geom, const PyrLayout& Lmax, const PyrPitchEntry* list, int n);
hipError_t launch_lk(hipStream_t s, const uint8_t* prev_slot, const uint8_t* next_slot, const PyrLayout& L,
                     const float* d_prev_xy, const int* d_order, int n_blocks, int n, const LKParams& P, float* d_out_xy,
                     uint8_t* d_status, float* d_err, uint16_t* d_work = nullptr);
// One launch of the extended form: `flags` (LKX_*) holds for every track, d_init_xy is read with LKX_INIT, the back arrays are written with LKX_FB.
// top_f / top_b (pmv_lk_track_fb_levels): the forward / backward trip starts at level min(top, L.n_levels - 1); -1 = the slot's top level.
// pred_mode (LKP_*; a predicted tracker step): d_pred is one (successes, successes wanted) pair - LKP_COUNT: every track adds its forward status
// to the first word; LKP_GATE: every workgroup reads the pair first and leaves at once when the first word has reached the second.
hipError_t launch_lk_ex(hipStream_t s, const uint8_t* prev_slot, const uint8_t* next_slot, const PyrLayout& L, const float* d_prev_xy, const float* d_init_xy,
                        const int* d_order, int n_blocks, int n, int flags, const LKParams& P, float* d_out_xy, uint8_t* d_status, float* d_err, uint16_t* d_work,
                        float* d_back_xy, uint8_t* d_back_status, float* d_back_err, int top_f = -1, int top_b = -1, int* d_pred = nullptr,
                        int pred_mode = LKP_NONE);
// The same launch sized by a bound: n_cap workgroups, of which those below *d_n (device memory, read by every workgroup) track d_prev_xy[i] in
// identity order; flags: LKX_FB or 0. The count never reaches the host.
hipError_t launch_lk_ex_dev(hipStream_t s, const uint8_t* prev_slot, const uint8_t* next_slot, const PyrLayout& L, const float* d_prev_xy, const int* d_n, int n_cap,
                            int flags, const LKParams& P, float* d_out_xy, uint8_t* d_status, float* d_err, float* d_back_xy, uint8_t* d_back_status, float* d_back_err);
// d_work (optional), per track: LK iterations executed over all levels | (level passes that iterated) << 8 - what the track cost. The
// roofline's OPS_lk is summed from these on the host (three atomics per track on shared counters cost the batched launch 14 % of the
// whole run's throughput: every wavefront of the chip ended on the same three L2 lines).

// Detector cells on the device: CELL_STRIDE ints per cell = (x0, y0, w, h, frame slot index, 0, 0, 0) — the slot index lets one
// launch serve cells of different frames (several sequences in one batch); `slots` is the base of the frame-slot array.
constexpr int CELL_STRIDE = 8;
// The back-end chains (PnP hypotheses + refit, the ~23 launches of an LM solve, two-view DLT) and the detector's selection pass are short,
// serially dependent launches whose waves share SIMDs with thousands of LK waves that keep the vector ALU issuing: in the mix every k_bamB_*
// kernel ran 3-4x longer than alone (kernel trace of a B = 128 run: campoint 64 vs 18 us, backsub 69 vs 15 us, no dispatch gap between them).
// s_setprio raises the issue priority of the wave that executes it, so the few waves of a chain get the instruction slots they ask for and the
// LK waves fill the rest.
#define BACKEND_PRIO() __builtin_amdgcn_s_setprio(3)
// GFTT: eig maps (n_cells * 255*255 floats), cell max (n_cells uint32 ordered keys), outputs
hipError_t launch_gftt(hipStream_t s, const uint8_t* slots, const PyrLayout& L, const int* d_cells, int n_cells,
                       int max_per_cell, double quality, double min_dist, int unlimited, float* d_eig, unsigned* d_cellmax,
                       int* d_out_xy, int* d_out_count, int* d_flags, unsigned* d_spill /* n_cells * CELL_PIX candidate overflow area */);
hipError_t launch_shitomasi(hipStream_t s, const uint8_t* slots, const PyrLayout& L, const int* d_cells, int n_cells,
                            int max_per_cell, double quality, double* d_resp, unsigned long long* d_cellmax,
                            int* d_out_xy, double* d_out_score, int* d_out_count, int* d_flags, unsigned* d_spill);

// ---- the reference's alternative plugins (frontend_alt.hip) ------------------------------------------------------
// One request of a kNN matcher round: n source features of the frame at byte offset src_off of the slot array against m candidates of
// the frame at cmp_off. The coordinate lists ((x, y) int pairs) are in device memory, the results may be mapped pinned host memory.
struct __attribute__((aligned(64))) KnnRound {
    unsigned long long src_off, cmp_off;
    const int* src_xy; const int* cmp_xy;
    int* out_best; float* out_err;       // per source feature: candidate index or -1 (the default Feature at (0,0)), its window error
    int n, m;
    int nn_window;                       // n_nn (1..8) | window (1..63) << 8: knn_pack
    int geom;                            // the request's entry of the geometry table (table form)
};
static_assert(sizeof(KnnRound) == 64, "KnnRound: one 64-byte record per request");
inline int knn_pack(int n_nn, int window) { return n_nn | (window << 8); }
// k_knn_round over n_requests records in device memory; max_n = the largest n among them. Both frames of a request have the geometry L
// (pmv_knn_match: a round of one) or, table form, d_geom[record.geom] (the batch engine: a round may hold any sizes).
hipError_t launch_knn_round(hipStream_t s, const uint8_t* slots, const PyrLayout& L, const KnnRound* d_recs, int n_requests, int max_n);
hipError_t launch_knn_round_geom(hipStream_t s, const uint8_t* slots, const PyrLayout* d_geom, const KnnRound* d_recs, int n_requests, int max_n);
// k_fast_score + k_fast_select over n_cells cell records (x0, y0, w, h, slot, byte offset of the cell's score map in d_score, 0, 0) in
// device-visible memory; a "cell" may be as large as the frame. max_pix = the largest w * h among them. Outputs per cell: max_per_cell
// (x, y) pairs, as many float responses, one count.
hipError_t launch_fast(hipStream_t s, const uint8_t* slots, const PyrLayout& L, const int* d_cells, int n_cells, int max_pix, int max_per_cell, int threshold,
                       int nonmax, uint8_t* d_score, int* d_out_xy, float* d_out_resp, int* d_out_count);

hipError_t launch_gftt_response(hipStream_t s, const uint8_t* slots, const PyrLayout& L, const int* d_cells, int n_cells, float* d_eig, unsigned* d_cellmax);
constexpr int CELL_MAX = 255;                 // OdometryPipeline.h:31 grid_size
constexpr int CELL_PIX = CELL_MAX * CELL_MAX;

// pmv_detect_gftt_ex: cv::goodFeaturesToTrack's blockSize, useHarrisDetector and k as the general kernels take them. k1, k2 = the taps of
// the Sobel smoothing kernel [1 2 1] with the scale 1 / (4 * blockSize * 255) folded in, as floats (gftt_ext computes them on the host
// the way tests/twin/gftt_twin.cpp does; at blockSize 3 they are k_gftt_cand's 1/3060 and 2/3060).
constexpr int GFTT_MAX_BLOCK = 15;
struct GfttExt { int bs, harris; double k; float k1, k2; };
inline GfttExt gftt_ext(int block_size, int use_harris, double k) {
    const double dscale = 1.0 / ((double)(1 << 2) * block_size * 255.0);
    return GfttExt{block_size, use_harris ? 1 : 0, use_harris ? k : 0.0, (float)(1.0 * dscale), (float)(2.0 * dscale)};
}
// launch_gftt through k_gftt_cand_general. d_mask: null, or the cells' packed mask sub-views (cw * ch bytes per cell at the byte offset in
// int 5 of its cell record, non-zero = allowed). Booked under the same two profiling classes.
hipError_t launch_gftt_ex(hipStream_t s, const uint8_t* slots, const PyrLayout& L, const int* d_cells, int n_cells, int max_per_cell, double quality,
                          double min_dist, int unlimited, const GfttExt& X, const uint8_t* d_mask, float* d_eig, unsigned* d_cellmax, int* d_out_xy,
                          int* d_out_count, int* d_flags, unsigned* d_spill);
hipError_t launch_gftt_response_ex(hipStream_t s, const uint8_t* slots, const PyrLayout& L, const int* d_cells, int n_cells, const GfttExt& X, float* d_eig);
// pmv_detect_gftt_frame: k_gftt_cand_frame (X null) or k_gftt_cand_general_frame, then k_gftt_pick_frame, over n_req request records in
// device-visible memory: (x0, y0, w, h, slot, byte offset of the region's packed mask in d_mask, first entry of the request's record list as
// low and high word). d_val / d_idx / d_keys: the record lists and the key lists of the slower path, each as long as the regions have
// pixels; d_info: 2 words per request. grid_x = the largest gftt_frame_grid_x(w, h) among the requests. Outputs per request: cap (x, y)
// pairs, a count (-1: a no-limit request with more than cap corners) and (records above the threshold, of those kept in HBM). Booked under
// K_GFTT_CAND and K_GFTT_PICK. The packing (y << 16) | x and the int distances need w, h <= GFTT_FRAME_MAX_SIDE.
constexpr int GFTT_FRAME_MAX_SIDE = 32767;
int gftt_frame_grid_x(int w, int h);
constexpr int GFTT_FRAME_ONCHIP = 16384;   // records the selection kernel sorts on chip (= PMV_GFTT_FRAME_MAX_CORNERS, capi.hip)
hipError_t launch_gftt_frame(hipStream_t s, const uint8_t* slots, const PyrLayout& L, const int* d_recs, int n_req, int grid_x, int cap, double quality,
                             double min_dist, int unlimited, const GfttExt* X, const uint8_t* d_mask, float* d_val, unsigned* d_idx, unsigned* d_info,
                             unsigned long long* d_keys, int* d_out_xy, int* d_out_count, int* d_stats, const int* d_cap = nullptr);
// d_cap (the tracker's chain): one word per request, the number of corners wanted, read by the selection from device memory and clamped to
// 0 .. cap; `cap` stays the capacity of every request's list. Null: cap itself, as ever.

// ---- keep-away mask of a track list (frontend_refill.hip) ----------------------------------------------------------
// pmv_detect_gftt_refill / pmv_batch_detect_gftt_refill: FeatureTracker::setMask on the device. One record per request; the tables of a
// launch (positions, priorities, flags, keep bytes, kept lists) hold the requests' tracks one after the other, each request's share
// starting at a multiple of four entries (refill_pad(n) entries long).
constexpr int REFILL_MAX_TRACKS = 8192;    // = PMV_REFILL_MAX_TRACKS: keys and positions of a request stay in LDS
constexpr int REFILL_MAX_RADIUS = 255;     // = PMV_REFILL_MAX_RADIUS: a half-width fits a byte
constexpr int REFILL_HW = 256;             // bytes of a request's half-width table
struct __attribute__((aligned(16))) RefillRec {
    int n, radius;                // tracks, cv::circle's radius
    int trk_off;                  // first entry of the request in the launch's per-track tables (a multiple of 4)
    int x0, y0, cw, ch;           // the region that is painted (frame coordinates)
    unsigned mask_off;            // byte offset of the region's packed mask (cw * ch bytes) in the mask buffer, a multiple of 4
    int has_base;                 // the packed mask holds the caller's base bytes (else it is painted from 255)
    int reserved[3];
};
static_assert(sizeof(RefillRec) == 48, "RefillRec: one 48-byte record per request");
inline size_t refill_pad(int n) { return ((size_t)n + 3) & ~(size_t)3; }
// cv::circle(.., radius, .., -1)'s rows as half-widths: out[d], d = 0 .. radius, is the widest span Circle()'s loop paints at row offset d;
// out[d] for d above the radius = 255 (never read as a width: the kernels test the row offset first). Computed on the HOST by the literal
// loop (OpenCV 3.4 drawing.cpp, fill, LINE_8, shift 0) and handed to the kernels, the policy of subpix_table.
void refill_halfwidths(int radius, uint8_t out[REFILL_HW]);
// k_track_select (one workgroup per request) then k_track_paint (grid over the largest packed region x requests) over n_req records in
// device-visible memory. d_pos: (y << 16) | x per track; d_prio: int priorities; d_flag: non-zero = the base byte under the track is 255;
// d_hw: REFILL_HW bytes per request. Outputs: d_keep (one byte per track, input order; device-visible), d_kept / d_nkept (the kept
// positions in rank order and their number: HBM, read by the painting) and the requests' packed masks in d_mask (which holds the base
// bytes of the requests that have some). max_bytes = the largest cw * ch among the requests. Booked under K_GFTT_PICK and K_GFTT_CAND.
hipError_t launch_track_refill(hipStream_t s, const RefillRec* d_recs, int n_req, size_t max_bytes, const unsigned* d_pos, const int* d_prio, const uint8_t* d_flag,
                               const uint8_t* d_hw, uint8_t* d_keep, unsigned* d_kept, int* d_nkept, uint8_t* d_mask);
hipError_t refill_prepare_device();   // LDS opt-in of k_track_select, per device (see frontend_prepare_device)

// ---- corner sub-pixel refinement (frontend_subpix.hip) -----------------------------------------------------------
// pmv_corner_subpix / pmv_batch_corner_subpix: one point of a launch names its frame slot and, in the table form, its entry of the geometry
// table, as LK's track records do: one launch serves points of several slots and frame sizes. Results go to the record's own index.
constexpr int SUBPIX_MAX_WIN = 15;
constexpr int SUBPIX_TABLE_MAX = (2 * SUBPIX_MAX_WIN + 1) * (2 * SUBPIX_MAX_WIN + 1);
struct __attribute__((aligned(16))) SubpixRec { float x, y; int slot; int geom; };
static_assert(sizeof(SubpixRec) == 16, "SubpixRec: one 16-byte record per point");
struct SubpixArgs { int win_w, win_h, max_iter; double eps2; };   // cv's half sizes, TermCriteria COUNT, EPS squared (in double)
// cv::cornerSubPix's weight table, (2 win_h + 1) rows of (2 win_w + 1) floats, with the zero zone cleared where cv clears it: computed on the
// HOST with libm (a device expf does not have libm's bits) and handed to the kernel
void subpix_table(int win_w, int win_h, int zero_w, int zero_h, float* out);
// k_corner_subpix over n records in device-visible memory. Every record has the geometry L (the single call) or d_geom[record.geom] (the
// batch engine). d_table: subpix_table's floats in device-visible memory. Booked under the detector's selection class.
hipError_t launch_corner_subpix(hipStream_t s, const uint8_t* slots, const PyrLayout& L, const SubpixRec* d_recs, int n, const float* d_table, const SubpixArgs& A,
                                float* d_out_xy, uint8_t* d_out_iters, uint8_t* d_out_flags);
// The tracker's chain: the grid is sized for n_cap points, the point count is read from *d_n (clamped to 0 .. n_cap; a wavefront beyond it
// leaves at once) and point i is the detector's corner ((float)d_ixy[2 i], (float)d_ixy[2 i + 1]) of frame slot `slot`.
// With d_req_slots (a group of trackers): n_req requests of n_cap points each, one after the other in d_ixy and in the outputs; request r reads
// its count from d_n[r] and its frame slot from d_req_slots[r] (`slot` is ignored). Null, n_req = 1: the one request above.
hipError_t launch_corner_subpix_dev(hipStream_t s, const uint8_t* slots, const PyrLayout& L, const int* d_ixy, int slot, int n_cap, const int* d_n, const float* d_table,
                                    const SubpixArgs& A, float* d_out_xy, uint8_t* d_out_iters, uint8_t* d_out_flags, const int* d_req_slots = nullptr, int n_req = 1);
hipError_t launch_corner_subpix_geom(hipStream_t s, const uint8_t* slots, const PyrLayout* d_geom, const SubpixRec* d_recs, int n, const float* d_table,
                                     const SubpixArgs& A, float* d_out_xy, uint8_t* d_out_iters, uint8_t* d_out_flags);

// ---- contrast-limited equalisation of level 0 (frontend_clahe.hip) -------------------------------------------------
// pmv_frames_clahe / pmv_batch_frame_upload_clahe: cv::CLAHE::apply on the interior of level 0, in place. One record per frame names its
// slot, its entry of a geometry table, its tile grid and the constants of include/pmv_hip.h (computed once on the host: clahe_record), and
// where its LUT block starts in the launch's LUT scratch, so ONE pair of launches serves any number of frames of any sizes and parameters.
constexpr int CLAHE_MAX_TILES = 16;                                        // per direction
constexpr size_t CLAHE_LUT_MAX = (size_t)CLAHE_MAX_TILES * CLAHE_MAX_TILES * 256;   // bytes of a frame's LUT block at most
struct __attribute__((aligned(16))) ClaheRec {
    int slot, geom;               // frame slot, entry of the launch's geometry table
    int tiles_x, tiles_y;         // cv's tileGridSize
    int tile_w, tile_h;           // tile size on the extended image
    int clip;                     // cl: the bins' ceiling, 0 = no clipping
    float lut_scale;              // (float)255 / (tile_w * tile_h)
    float inv_tw, inv_th;         // 1.0f / tile_w, 1.0f / tile_h
    unsigned lut_off;             // byte offset of the frame's tiles_x * tiles_y * 256 LUT bytes in the LUT scratch
    int reserved;
};
static_assert(sizeof(ClaheRec) == 48, "ClaheRec: one 48-byte record per frame");
// the record of a w x h frame (lut_off left 0): cv's extension rule and constants, in the contract's arithmetic
ClaheRec clahe_record(int slot, int geom, int w, int h, double clip_limit, int tiles_x, int tiles_y);
// k_clahe_lut then k_clahe_apply over n records in device-visible memory; d_geom[record.geom] (device memory) is the record's frame.
// max_tiles, max_w, max_h: the largest tiles_x * tiles_y, level-0 width and height among the records - they size the grids; a workgroup
// beyond its own frame's tiles or rows leaves before its first load or barrier. d_lut: the LUT scratch (device memory) that holds every
// record's block. Both launches are booked under the level-0 profiling class.
hipError_t launch_clahe(hipStream_t s, uint8_t* slots, const PyrLayout* d_geom, const ClaheRec* d_recs, int n, int max_tiles, int max_w, int max_h, uint8_t* d_lut);

// ---- cv::remap of level 0 (frontend_remap.hip) ----------------------------------------------------------------------
// pmv_frames_remap / pmv_batch_frame_upload_remap: bilinear, constant border, cv's fixed-point arithmetic. One record per frame names its
// slot, its entry of a geometry table, its packed map (device memory, remap_pack's layout), the border value and the byte offset of its
// tight w x h destination frame in the launch's scratch area (a multiple of 256), so ONE launch serves any number of frames of any sizes
// and maps. The kernel reads the interior of level 0 and writes the scratch frame; the list-form level-0 launch with that frame as its
// source and the k_pyrdown launches finish the slot.
struct __attribute__((aligned(16))) RemapRec {
    const uint32_t* map;          // the packed map of the frame's size
    unsigned long long dst_off;   // byte offset of the frame in the scratch area
    int slot, geom;               // frame slot, entry of the launch's geometry table
    int border;                   // cv's borderValue, 0..255
    int reserved;
};
static_assert(sizeof(RemapRec) == 32, "RemapRec: one 32-byte record per frame");
// bytes of a frame in a remap scratch area: the tight frame rounded up, so that every frame starts 256-byte aligned and the dword fetches of
// the level-0 kernel behind it (the aligned dwords that hold a row's bytes) stay inside the frame's own block
inline size_t remap_frame_bytes(int w, int h) { return ((size_t)w * (size_t)h + 255) & ~(size_t)255; }
// the packed form of a w x h pair of CV_32FC1 maps: two planes over the linear pixel index, each padded to a multiple of four entries -
// (ix & 0xffff) | iy << 16 as dwords, then fx | fy << 5 as halfwords; 6 bytes per pixel. remap_pack converts on the host (cv's conversion,
// include/pmv_hip.h) into `out` (remap_map_bytes(w, h) bytes, 4-byte aligned).
size_t remap_map_bytes(int w, int h);
void remap_pack(const float* map_x, const float* map_y, int w, int h, uint8_t* out);
// cv::initUndistortRectifyMap(K, dist8, R or identity, newK or K, (w, h), CV_32FC1), evaluated per pixel in double; false: newK R is singular
bool undistort_map(const double* K, const double* dist8, const double* R, const double* newK, int w, int h, float* map_x, float* map_y);
// cv::fisheye::initUndistortRectifyMap(K, k4, R or identity, newK or K, (w, h), CV_32FC1) in the same manner, through fisheye_project
// (pmv_lift.h) on the host; a pixel the projection refuses gets (-1, -1); false: newK R is singular
bool fisheye_map(const double* K, const double* k4, const double* R, const double* newK, int w, int h, float* map_x, float* map_y);
// k_remap over n records in device-visible memory; d_geom[record.geom] (device memory) is the record's frame. max_w, max_h: the largest
// level-0 width and height among the records - they size the grid; a thread beyond its own frame leaves before its first load. Booked under
// the level-0 profiling class.
hipError_t launch_remap(hipStream_t s, const uint8_t* slots, const PyrLayout* d_geom, const RemapRec* d_recs, int n, int max_w, int max_h, uint8_t* d_scratch);
// The feeder's form (pmv_set_frame_preproc): the same gather with its taps in a TIGHT source frame at a device address - the round's
// landing buffer in HBM - instead of a slot, and the interior of level 0 of the slot as its destination (row pitch stride[0], base gray_off),
// so source and destination are different memory and no scratch frame exists. bgr != 0: the source is tight BGR (3 w h bytes) and every tap
// is converted with cvtColor's integer rule before the weights - the value k_pad_level0_bgr would have stored. The in-place level-0 launch
// behind it adds the REFLECT_101 frame.
struct __attribute__((aligned(16))) RemapSrcRec {
    const uint32_t* map;          // the packed map of the frame's size
    const uint8_t* src;           // the tight source frame (device memory)
    int slot, geom;               // destination slot, entry of the launch's geometry table
    int border;                   // cv's borderValue, 0..255
    int bgr;                      // 0: w h gray bytes, else 3 w h BGR bytes
};
static_assert(sizeof(RemapSrcRec) == 32, "RemapSrcRec: one 32-byte record per frame");
// k_remap_src over n records in device-visible memory; max_w, max_h as for launch_remap. Booked under the level-0 profiling class.
hipError_t launch_remap_src(hipStream_t s, uint8_t* slots, const PyrLayout* d_geom, const RemapSrcRec* d_recs, int n, int max_w, int max_h);

}  // namespace pmv
