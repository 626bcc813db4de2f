// C-ABI implementation (include/pmv_hip.h): context, frame slots, launches, D2H staging.
#include "pmv_ctx.h"
#include "ingest_batch.h"
#include <algorithm>
#include <vector>
#include <cstdarg>
#include <cfloat>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <cstdlib>

using namespace pmv;

static thread_local char g_create_err[512] = "";
thread_local pmv::Profiler* pmv::tl_prof = nullptr;

// The message goes to the calling thread's own buffer first (what ck() of hip_pipeline.hip and the batch engine's sequence threads
// report: a failing sequence must not pick up another sequence's text) and then, under a mutex, to the context's buffer that
// pmv_last_error() hands to the caller of the entry point.
static thread_local char tl_err[512] = "";
const char* pmv::thread_error() { return tl_err; }
void pmv::set_err(pmv_ctx* c, const char* fmt, ...) {
    char tmp[512];   // (the arguments may point into tl_err or c->err themselves)
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(tmp, sizeof(tmp), fmt, ap);
    va_end(ap);
    memcpy(tl_err, tmp, sizeof(tmp));
    if (!c) { memcpy(g_create_err, tmp, sizeof(tmp)); return; }
    std::lock_guard<std::mutex> lk(c->err_mu);
    memcpy(c->err, tmp, sizeof(tmp));
}

PyrLayout pmv::make_layout(int w, int h, int win, int max_level) {
    PyrLayout L;
    memset(&L, 0, sizeof(L));
    // cv::buildOpticalFlowPyramid(img, pyr, Size(win,win), maxLevel): stop when the next level would be <= winSize (the reference: 32, 4)
    int lw = w, lh = h, n = 0;
    uint32_t off = 0;
    for (int level = 0; level <= max_level && level < MAX_LEVELS; level++) {
        L.w[level] = lw; L.h[level] = lh;
        L.stride[level] = (lw + 2 * PAD + 63) & ~63;
        L.off[level] = off;
        off += (uint32_t)L.stride[level] * (uint32_t)(lh + 2 * PAD);
        n = level + 1;
        lw = (lw + 1) / 2; lh = (lh + 1) / 2;
        if (lw <= win || lh <= win) break;
    }
    L.n_levels = n;
    // No separate copy of the gray frame: staging writes its rows into the interior of the padded level 0 and k_pad_level0 adds the
    // REFLECT_101 frame around them in place (1.11 MB per 1241x376 slot instead of 1.58 MB: 192 sequences of the metric configuration
    // fit the 288 GB instead of 128)
    L.gray_off = L.off[0] + (uint32_t)PAD * (uint32_t)L.stride[0] + (uint32_t)PAD;
    L.slot_bytes = (off + 4095) & ~4095u;
    return L;
}

LKParams pmv::lk_launch_params(const pmv_ctx* ctx) {
    LKParams P;
    P.max_iter = ctx->lk.max_iter; P.eps2d = ctx->lk.eps * ctx->lk.eps; P.eps2 = (float)P.eps2d; P.min_eig = ctx->lk.min_eig;
    P.stamps = nullptr;
    P.win = ctx->lk.win; P.general = ctx->lk_general;
    return P;
}

extern "C" {

const char* pmv_last_error(pmv_ctx* ctx) { return ctx ? ctx->err : g_create_err; }
const char* pmv_thread_error(void) { return tl_err; }

int pmv_ctx_create(pmv_ctx** out, int device, int max_w, int max_h, int n_slots, int max_tracks, int max_ba_cams,
                   int max_ba_points, int max_ba_obs) {
    if (!out || max_w < 40 || max_h < 40 || n_slots < 1 || max_tracks < 1) {
        set_err(nullptr, "pmv_ctx_create: invalid argument");
        return PMV_ERR_INVALID;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device >= ndev) {
        set_err(nullptr, "pmv_ctx_create: no HIP device %d (count %d) — this library has no CPU fallback", device, ndev);
        return PMV_ERR_NO_DEVICE;
    }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) { set_err(nullptr, "hipGetDeviceProperties failed"); return PMV_ERR_HIP; }
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        set_err(nullptr, "pmv_ctx_create: device %d is %s; kernels are built for gfx950 only", device, prop.gcnArchName);
        return PMV_ERR_NO_DEVICE;
    }
    pmv_ctx* c = new pmv_ctx();
    c->device = device;
    c->max_w = max_w; c->max_h = max_h; c->n_slots = n_slots; c->max_tracks = max_tracks;
    c->max_ba_cams = max_ba_cams; c->max_ba_points = max_ba_points; c->max_ba_obs = max_ba_obs;
    c->cap = make_layout(max_w, max_h, c->lk.win, c->lk.max_level);
    c->slot_layout.assign(n_slots, PyrLayout());
    c->slot_state.assign(n_slots, SLOT_EMPTY);
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { set_err(nullptr, "%s: %s", #x, hipGetErrorString(e_)); pmv_ctx_destroy(c); return PMV_ERR_HIP; } } while (0)
    CK(hipSetDevice(device));
    CK(frontend_prepare_device());
    CK(refill_prepare_device());
    CK(backend_prepare_device());
    CK(hipStreamCreateWithFlags(&c->s_front, hipStreamNonBlocking));
    CK(hipStreamCreateWithFlags(&c->s_back, hipStreamNonBlocking));
    const size_t nt = (size_t)max_tracks;
    // THE list of the context's fixed buffers (the lazily made ones are an ensure() at their first use; the back-end's own table: backend_alloc)
    const MemRow rows[] = {
        {&c->d_slots, (size_t)c->cap.slot_bytes * n_slots, MEM_DEVICE},
        {&c->d_tight, (size_t)pmv_ctx::TIGHT_FRAMES * max_w * max_h + 256, MEM_DEVICE},
        {&c->d_prev_xy, nt * 12 + 64, MEM_DEVICE},   // track coordinates followed by the block -> track order
        {&c->d_out_xy, nt * 8, MEM_DEVICE},
        {&c->d_status, nt, MEM_DEVICE},
        {&c->d_err, nt * 4, MEM_DEVICE},
        {&c->h_prev_xy, nt * 12 + 64, MEM_PINNED},
        // LK results: 13 bytes per track, written by the kernel through the device aliases of these mapped pinned buffers (no D2H copies)
        {&c->h_out_xy, nt * 8, MEM_MAPPED},
        {&c->h_status, nt, MEM_MAPPED},
        {&c->h_err, nt * 4, MEM_MAPPED},
        {&c->d_knn, nt * 16 + 64, MEM_DEVICE},
        {&c->h_knn, nt * 16 + 64, MEM_PINNED},
        {&c->h_work, nt * 2, MEM_MAPPED},
        {&c->d_geom, sizeof(PyrLayout) * pmv_ctx::MAX_GEOM, MEM_DEVICE},
        {&c->d_cells, MAX_CELLS * CELL_STRIDE * 4, MEM_DEVICE},
        {&c->h_cells, MAX_CELLS * CELL_STRIDE * 4, MEM_PINNED},
        {&c->d_eig, (size_t)MAX_CELLS * CELL_PIX * sizeof(double), MEM_DEVICE},   // shared by GFTT (f32) and ShiTomasi (f64)
        {&c->d_cellmax, MAX_CELLS * 8, MEM_DEVICE},
        {&c->d_spill, (size_t)MAX_CELLS * CELL_PIX * 4, MEM_DEVICE},
        {&c->d_det_xy, (size_t)MAX_CELLS * MAX_PER_CELL * 8, MEM_DEVICE},
        {&c->d_det_score, (size_t)MAX_CELLS * MAX_PER_CELL * 8, MEM_DEVICE},
        {&c->d_det_count, MAX_CELLS * 4, MEM_DEVICE},
        {&c->d_flags, 16, MEM_DEVICE},
        {&c->h_det_xy, (size_t)MAX_CELLS * MAX_PER_CELL * 8, MEM_PINNED},
        {&c->h_det_score, (size_t)MAX_CELLS * MAX_PER_CELL * 8, MEM_PINNED},
        {&c->h_det_count, MAX_CELLS * 4 + 16, MEM_PINNED},
    };
    CK(mem_alloc_table(rows, sizeof(rows) / sizeof(rows[0])));
    CK(hipMemset(c->d_geom, 0, sizeof(PyrLayout) * pmv_ctx::MAX_GEOM));
    CK(hipMemset(c->d_flags, 0, 16));
    for (auto& a : c->lk_work) a.store(0);
    for (auto& a : c->batch_launches) a.store(0);
    for (auto& a : c->whole_rounds) a.store(0);
    for (auto& a : c->homography_launches) a.store(0);
    for (auto& a : c->tri_tracks_launches) a.store(0);
    for (auto& a : c->subpix_launches) a.store(0);
    for (auto& a : c->clahe_launches) a.store(0);
    for (auto& a : c->remap_launches) a.store(0);
    for (auto& a : c->preproc_launches) a.store(0);
    for (auto& a : c->klt_stats) a.store(0);
    for (auto& a : c->klt_many_stats) a.store(0);
    for (auto& a : c->klt_stereo_stats) a.store(0);
    for (auto& a : c->klt_observe_stats) a.store(0);
    int rc = backend_create(c);
    if (rc != PMV_OK) { snprintf(g_create_err, sizeof(g_create_err), "%s", c->err); pmv_ctx_destroy(c); return rc; }
#undef CK
    *out = c;
    return PMV_OK;
}

void pmv_ctx_destroy(pmv_ctx* c) {
    if (!c) return;
    hipSetDevice(c->device);
    batch_session_destroy(c);
    batch_engine_destroy(c);
    batch_ingest_destroy(c->ingest);
    batch_ingest_destroy(c->bingest);
    if (c->s_front) hipStreamSynchronize(c->s_front);
    if (c->s_back) hipStreamSynchronize(c->s_back);
    klt_destroy_all(c);
    backend_destroy(c);
    c->prof.destroy();
    if (c->s_front) hipStreamDestroy(c->s_front);
    if (c->s_back) hipStreamDestroy(c->s_back);
    delete c;   // the buffers go with it: every stream that could use one was synchronised above
}

#define CKC(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { set_err(ctx, "%s: %s", #x, hipGetErrorString(e_)); return PMV_ERR_HIP; } } while (0)
#define REQ(cond, code, ...) do { if (!(cond)) { set_err(ctx, __VA_ARGS__); return code; } } while (0)

int pmv_debug_mem_live(long long* out2) {
    pmv_ctx* ctx = nullptr;
    REQ(out2, PMV_ERR_INVALID, "pmv_debug_mem_live: null argument");
    for (int i = 0; i < 2; i++) out2[i] = g_mem_live[i].load();
    return PMV_OK;
}

int pmv_sync(pmv_ctx* ctx) {
    REQ(ctx, PMV_ERR_INVALID, "null ctx");
    CKC(hipStreamSynchronize(ctx->s_front));
    CKC(hipStreamSynchronize(ctx->s_back));
    return PMV_OK;
}

}  // extern "C"
// pyramid levels of `n` consecutive slots with identical geometry L on `stream`; tight != nullptr: level 0 comes from n tight gray frames
// at `tight` (device) instead of from the levels' own interior
static int build_levels_on(pmv_ctx* ctx, hipStream_t stream, int first_slot, int n, const PyrLayout& L, const uint8_t* tight = nullptr) {
    CKC(launch_pad_level0(stream, ctx->d_slots, L, first_slot, n, tight));
    for (int l = 1; l < L.n_levels; l++) CKC(launch_pyrdown(stream, ctx->d_slots, L, l, first_slot, n));
    return PMV_OK;
}

// build_levels_on over slots [first_slot, first_slot + n): consecutive slots of equal geometry go into one launch per level. With `who`, an
// empty slot is that call's PMV_ERR_INVALID and every built run is marked SLOT_BUILT at once.
static int build_runs_on(pmv_ctx* ctx, hipStream_t stream, int first_slot, int n, const char* who = nullptr) {
    int i = 0;
    while (i < n) {
        const PyrLayout& L = ctx->slot_layout[first_slot + i];
        if (who) REQ(ctx->slot_state[first_slot + i] != SLOT_EMPTY, PMV_ERR_INVALID, "%s: slot %d was never staged", who, first_slot + i);
        int j = i + 1;
        while (j < n && ctx->slot_layout[first_slot + j].w[0] == L.w[0] && ctx->slot_layout[first_slot + j].h[0] == L.h[0]) j++;
        if (const int rc = build_levels_on(ctx, stream, first_slot + i, j - i, L)) return rc;
        if (who) for (int k = i; k < j; k++) ctx->slot_state[first_slot + k] = SLOT_BUILT;
        i = j;
    }
    return PMV_OK;
}

// the tail pmv_frame_upload and pmv_frame_upload_bgr share once the gray frame is in the landing area
static int upload_from_tight(pmv_ctx* ctx, int slot, const PyrLayout& L) {
    if (const int rc = build_levels_on(ctx, ctx->s_front, slot, 1, L, ctx->d_tight)) return rc;
    CKC(hipStreamSynchronize(ctx->s_front));   // the host buffer may be reused by the caller
    ctx->slot_layout[slot] = L;
    ctx->slot_state[slot] = SLOT_BUILT;
    return PMV_OK;
}

// NOTE: slots are addressed with the CAPACITY slot size (ctx->cap.slot_bytes); a frame smaller than max_w x max_h
// uses its own level geometry inside the slot but the same slot pitch.
PyrLayout pmv::layout_for(pmv_ctx* ctx, int w, int h) {
    PyrLayout L = make_layout(w, h, ctx->lk.win, ctx->lk.max_level);
    L.slot_bytes = ctx->cap.slot_bytes;
    return L;
}
int pmv::geom_table_set(pmv_ctx* ctx, const int* w, const int* h, int B) {
    ctx->geom.clear();
    for (int b = 0; b < B; b++)
        if (ctx->geom_index(w[b], h[b]) < 0) {
            REQ((int)ctx->geom.size() < pmv_ctx::MAX_GEOM, PMV_ERR_CAPACITY, "more than %d distinct frame sizes in one batch", pmv_ctx::MAX_GEOM);
            ctx->geom.push_back(layout_for(ctx, w[b], h[b]));
        }
    CKC(hipSetDevice(ctx->device));
    CKC(hipMemcpy(ctx->d_geom, ctx->geom.data(), sizeof(PyrLayout) * ctx->geom.size(), hipMemcpyHostToDevice));
    return PMV_OK;
}
extern "C" {

int pmv_frames_stage(pmv_ctx* ctx, int first_slot, int n, const uint8_t* gray, int w, int h) {
    REQ(ctx && gray, PMV_ERR_INVALID, "pmv_frames_stage: null argument");
    REQ(first_slot >= 0 && n >= 1 && first_slot + n <= ctx->n_slots, PMV_ERR_CAPACITY, "pmv_frames_stage: slots [%d,%d) out of range (n_slots %d)", first_slot, first_slot + n, ctx->n_slots);
    REQ(w >= 40 && h >= 40 && w <= ctx->max_w && h <= ctx->max_h, PMV_ERR_CAPACITY, "pmv_frames_stage: frame %dx%d outside capacity %dx%d", w, h, ctx->max_w, ctx->max_h);
    tl_prof = &ctx->prof;
    CKC(hipSetDevice(ctx->device));
    PyrLayout L = layout_for(ctx, w, h);
    // contiguous copies into the landing area, then level 0 (interior + REFLECT_101 frame) written by k_pad_level0 from there. Colour frames
    // (tight BGR, pmv_set_frame_format) land as they are, a third as many per chunk, and k_pad_level0_bgr converts them on the way: the slot
    // then holds what staging the converted image would have left.
    const bool bgr = ctx->frame_format == PMV_FRAMES_BGR;
    const size_t fb = (size_t)w * h * (bgr ? 3 : 1);
    const int chunk = bgr ? pmv_ctx::TIGHT_FRAMES / 3 : pmv_ctx::TIGHT_FRAMES;
    for (int i0 = 0; i0 < n; i0 += chunk) {
        const int nb = std::min(chunk, n - i0);
        CKC(hipMemcpyAsync(ctx->d_tight, gray + (size_t)i0 * fb, (size_t)nb * fb, hipMemcpyHostToDevice, ctx->s_front));
        if (bgr) CKC(launch_pad_level0_bgr(ctx->s_front, ctx->d_slots, L, first_slot + i0, nb, ctx->d_tight));
        else CKC(launch_pad_level0(ctx->s_front, ctx->d_slots, L, first_slot + i0, nb, ctx->d_tight));
    }
    CKC(hipStreamSynchronize(ctx->s_front));
    for (int i = 0; i < n; i++) { ctx->slot_layout[first_slot + i] = L; ctx->slot_state[first_slot + i] = SLOT_STAGED; }
    return PMV_OK;
}

// What the host frames of pmv_frames_stage, pmv_frames_stream_begin, pmv_pipeline_run_streamed and pmv_pipeline_run_batch_streamed hold: the
// reference never sees a gray image on input (Frame.cpp:33,40-41). Not while a feed reads frames of the other format.
int pmv_set_frame_format(pmv_ctx* ctx, int format) {
    REQ(ctx, PMV_ERR_INVALID, "null ctx");
    REQ(format == PMV_FRAMES_GRAY || format == PMV_FRAMES_BGR, PMV_ERR_INVALID, "pmv_set_frame_format: unknown format %d (PMV_FRAMES_GRAY = 0, PMV_FRAMES_BGR = 1)", format);
    REQ(!batch_ingest_active(ctx->ingest), PMV_ERR_INVALID, "pmv_set_frame_format: a pmv_frames_stream_begin bracket is open (pmv_frames_stream_end first)");
    REQ(!ctx->batch_open.load() && !batch_ingest_active(ctx->bingest), PMV_ERR_INVALID, "pmv_set_frame_format: a batched run is open on this context");
    ctx->frame_format = format;
    return PMV_OK;
}

// cv::calcOpticalFlowPyrLK's winSize, maxLevel, criteria and minEigThreshold (and buildOpticalFlowPyramid's winSize, maxLevel) for every
// pyramid built and every LK call made on the context from now on. Not while a feeder, a batched run or a session holds layouts made
// under the old values.
int pmv_set_lk_params(pmv_ctx* ctx, const pmv_lk_params* p) {
    REQ(ctx && p, PMV_ERR_INVALID, "pmv_set_lk_params: null argument");
    REQ(p->win >= 3 && p->win <= 63, PMV_ERR_INVALID, "pmv_set_lk_params: win = %d outside 3..63", p->win);
    REQ(p->max_level >= 0 && p->max_level <= MAX_LEVELS - 1, PMV_ERR_INVALID, "pmv_set_lk_params: max_level = %d outside 0..%d", p->max_level, MAX_LEVELS - 1);
    REQ(p->max_iter >= 1 && p->max_iter <= 100, PMV_ERR_INVALID, "pmv_set_lk_params: max_iter = %d outside 1..100", p->max_iter);
    REQ(p->eps >= 0.0 && p->eps <= 10.0, PMV_ERR_INVALID, "pmv_set_lk_params: eps = %g outside 0..10", p->eps);   // (a NaN fails the comparison too)
    REQ(p->min_eig >= 0.f && p->min_eig <= FLT_MAX, PMV_ERR_INVALID, "pmv_set_lk_params: min_eig = %g is negative or not finite", (double)p->min_eig);
    REQ(!batch_ingest_active(ctx->ingest), PMV_ERR_INVALID, "pmv_set_lk_params: a pmv_frames_stream_begin bracket is open (pmv_frames_stream_end first)");
    std::lock_guard<std::mutex> own(ctx->owner_mu);
    REQ(ctx->session_state.load() == 0, PMV_ERR_INVALID, "pmv_set_lk_params: a batch session is open on this context (set the parameters before pmv_batch_open)");
    REQ(!ctx->batch_open.load() && !batch_ingest_active(ctx->bingest), PMV_ERR_INVALID, "pmv_set_lk_params: a batched run is open on this context");
    if (p->win != ctx->lk.win || p->max_level != ctx->lk.max_level) {
        // every layout changes: the slots go back to what they were after pmv_ctx_create, on a pitch sized for the new depth
        CKC(hipSetDevice(ctx->device));
        CKC(hipStreamSynchronize(ctx->s_front));
        CKC(hipStreamSynchronize(ctx->s_back));
        const PyrLayout cap = make_layout(ctx->max_w, ctx->max_h, p->win, p->max_level);
        const size_t need = (size_t)cap.slot_bytes * ctx->n_slots;
        if (need > ctx->d_slots.cap) {   // new before old, not ensure(): a failed allocation leaves storage, pitch and setting as they were
            Buf<uint8_t> d;
            CKC(d.ensure(need));
            ctx->d_slots = std::move(d);
        }
        ctx->cap = cap;
        ctx->slot_layout.assign(ctx->n_slots, PyrLayout());
        ctx->slot_state.assign(ctx->n_slots, SLOT_EMPTY);
    }
    ctx->lk = *p;
    return PMV_OK;
}
int pmv_get_lk_params(pmv_ctx* ctx, pmv_lk_params* out) {
    REQ(ctx && out, PMV_ERR_INVALID, "pmv_get_lk_params: null argument");
    *out = ctx->lk;
    return PMV_OK;
}
// diagnostic: the default window through the general kernels as well (a test compares the two code paths; no result changes)
int pmv_debug_lk_general(pmv_ctx* ctx, int on) {
    REQ(ctx, PMV_ERR_INVALID, "null ctx");
    ctx->lk_general = on != 0;
    return PMV_OK;
}

int pmv_frames_build(pmv_ctx* ctx, int first_slot, int n) {
    REQ(ctx, PMV_ERR_INVALID, "null ctx");
    tl_prof = &ctx->prof;
    REQ(first_slot >= 0 && n >= 1 && first_slot + n <= ctx->n_slots, PMV_ERR_CAPACITY, "pmv_frames_build: slot range");
    CKC(hipSetDevice(ctx->device));
    return build_runs_on(ctx, ctx->s_front, first_slot, n, "pmv_frames_build");
}

int pmv_frame_upload(pmv_ctx* ctx, int slot, const uint8_t* gray, int w, int h, int stride) {
    REQ(ctx && gray, PMV_ERR_INVALID, "pmv_frame_upload: null argument");
    REQ(slot >= 0 && slot < ctx->n_slots, PMV_ERR_CAPACITY, "pmv_frame_upload: slot %d out of range", slot);
    REQ(w >= 40 && h >= 40 && w <= ctx->max_w && h <= ctx->max_h && stride >= w, PMV_ERR_CAPACITY, "pmv_frame_upload: frame %dx%d outside capacity %dx%d", w, h, ctx->max_w, ctx->max_h);
    tl_prof = &ctx->prof;
    CKC(hipSetDevice(ctx->device));
    PyrLayout L = layout_for(ctx, w, h);
    CKC(hipMemcpy2DAsync(ctx->d_tight, (size_t)w, gray, stride, w, h, hipMemcpyHostToDevice, ctx->s_front));
    return upload_from_tight(ctx, slot, L);
}

// Frame::Frame(file) + Frame::init for a COLOUR image (Frame.cpp:33,40-41: imread(IMREAD_COLOR) gives BGR, cvtColor(BGR2GRAY) the u8 `bw`
// everything else works on): the conversion runs on the device, in front of the landing area.
int pmv_frame_upload_bgr(pmv_ctx* ctx, int slot, const uint8_t* bgr, int w, int h, int stride) {
    REQ(ctx && bgr, PMV_ERR_INVALID, "pmv_frame_upload_bgr: null argument");
    REQ(slot >= 0 && slot < ctx->n_slots, PMV_ERR_CAPACITY, "pmv_frame_upload_bgr: slot %d out of range", slot);
    REQ(w >= 40 && h >= 40 && w <= ctx->max_w && h <= ctx->max_h && stride >= 3 * w, PMV_ERR_CAPACITY, "pmv_frame_upload_bgr: frame %dx%d outside capacity %dx%d", w, h, ctx->max_w, ctx->max_h);
    tl_prof = &ctx->prof;
    CKC(hipSetDevice(ctx->device));
    PyrLayout L = layout_for(ctx, w, h);
    // landing area: frame 0 receives the gray image, frames 1..3 hold the three bytes per pixel on their way in (TIGHT_FRAMES >= 4)
    uint8_t* d_bgr = ctx->d_tight + (size_t)ctx->max_w * ctx->max_h;
    CKC(hipMemcpy2DAsync(d_bgr, (size_t)3 * w, bgr, stride, (size_t)3 * w, h, hipMemcpyHostToDevice, ctx->s_front));
    CKC(launch_bgr2gray(ctx->s_front, d_bgr, w, h, 3 * w, ctx->d_tight));
    return upload_from_tight(ctx, slot, L);
}

}  // extern "C"

int pmv::clahe_check(pmv_ctx* ctx, const char* who, const pmv_clahe_params* p) {
    REQ(p, PMV_ERR_INVALID, "%s: null argument", who);
    REQ(p->tiles_x >= 1 && p->tiles_x <= CLAHE_MAX_TILES && p->tiles_y >= 1 && p->tiles_y <= CLAHE_MAX_TILES, PMV_ERR_INVALID, "%s: tiles = (%d, %d) is outside 1..%d", who,
        p->tiles_x, p->tiles_y, CLAHE_MAX_TILES);
    REQ(p->clip_limit >= 0.0 && std::isfinite(p->clip_limit), PMV_ERR_INVALID, "%s: clip_limit = %g is negative or not finite", who, p->clip_limit);   // (a NaN fails the comparison too)
    return PMV_OK;
}

extern "C" {

// cv::CLAHE::apply on level 0 of the slots, in place, then the REFLECT_101 frame and the levels above through pmv_frames_build's launches.
// A chunk of CLAHE_CHUNK frames is ONE pair of launches whatever its sizes: every record names its entry of the chunk's own geometry table.
int pmv_frames_clahe(pmv_ctx* ctx, int first_slot, int n, const pmv_clahe_params* p) {
    REQ(ctx, PMV_ERR_INVALID, "pmv_frames_clahe: null argument");
    if (const int rc_ = clahe_check(ctx, "pmv_frames_clahe", p)) return rc_;
    REQ(first_slot >= 0 && n >= 1 && first_slot <= ctx->n_slots - n, PMV_ERR_CAPACITY, "pmv_frames_clahe: slots [%d,%d) out of range (n_slots %d)", first_slot, first_slot + n, ctx->n_slots);
    REQ(!batch_ingest_active(ctx->ingest), PMV_ERR_INVALID, "pmv_frames_clahe: a pmv_frames_stream_begin bracket is open (pmv_frames_stream_end first)");
    REQ(!ctx->batch_open.load() && !batch_ingest_active(ctx->bingest), PMV_ERR_INVALID, "pmv_frames_clahe: a batched run is open on this context");
    for (int i = 0; i < n; i++) REQ(ctx->slot_state[first_slot + i] != SLOT_EMPTY, PMV_ERR_INVALID, "pmv_frames_clahe: slot %d is empty (never staged or uploaded)", first_slot + i);
    tl_prof = &ctx->prof;
    CKC(hipSetDevice(ctx->device));
    constexpr int CH = pmv_ctx::CLAHE_CHUNK;
    constexpr size_t tab_bytes = (size_t)CH * (sizeof(ClaheRec) + sizeof(PyrLayout));
    CKC(ctx->h_clahe.ensure(tab_bytes)); CKC(ctx->d_clahe.ensure(tab_bytes)); CKC(ctx->d_clahe_lut.ensure((size_t)CH * CLAHE_LUT_MAX));
    Carve c(ctx->h_clahe.p, ctx->d_clahe.p, tab_bytes);   // chunk tables, pinned mirror and HBM copy: [records | the chunk's geometry table]
    const Carved<ClaheRec> c_recs = c.take<ClaheRec>(CH);
    const Carved<PyrLayout> c_tab = c.take<PyrLayout>(CH);
    ClaheRec* recs = c_recs.h;
    PyrLayout* tab = c_tab.h;
    for (int i0 = 0; i0 < n; i0 += CH) {
        const int nb = std::min(CH, n - i0);
        int n_geom = 0, max_tiles = 0, max_w = 0, max_h = 0;
        unsigned lut_off = 0;
        for (int i = 0; i < nb; i++) {
            const int slot = first_slot + i0 + i;
            const PyrLayout& L = ctx->slot_layout[slot];
            int g = 0;
            while (g < n_geom && (tab[g].w[0] != L.w[0] || tab[g].h[0] != L.h[0])) g++;
            if (g == n_geom) tab[n_geom++] = L;
            recs[i] = clahe_record(slot, g, L.w[0], L.h[0], p->clip_limit, p->tiles_x, p->tiles_y);
            recs[i].lut_off = lut_off;
            lut_off += (unsigned)(p->tiles_x * p->tiles_y) * 256u;
            max_tiles = p->tiles_x * p->tiles_y; max_w = std::max(max_w, L.w[0]); max_h = std::max(max_h, L.h[0]);
        }
        CKC(hipMemcpyAsync(ctx->d_clahe, ctx->h_clahe, tab_bytes, hipMemcpyHostToDevice, ctx->s_front));
        CKC(launch_clahe(ctx->s_front, ctx->d_slots, c_tab.d, c_recs.d, nb, max_tiles, max_w, max_h, ctx->d_clahe_lut));
        ctx->clahe_launches[0]++;
        CKC(hipStreamSynchronize(ctx->s_front));   // (the next chunk rewrites the pinned tables)
    }
    // the REFLECT_101 frame of level 0 in place and the levels above
    if (const int rc_ = build_runs_on(ctx, ctx->s_front, first_slot, n)) return rc_;
    CKC(hipStreamSynchronize(ctx->s_front));
    for (int k = 0; k < n; k++) ctx->slot_state[first_slot + k] = SLOT_BUILT;
    return PMV_OK;
}
int pmv_debug_clahe_launches(pmv_ctx* ctx, long long* out3) {
    REQ(ctx && out3, PMV_ERR_INVALID, "pmv_debug_clahe_launches: null argument");
    for (int i = 0; i < 3; i++) out3[i] = ctx->clahe_launches[i].load();
    return PMV_OK;
}

}  // extern "C"

int pmv::remap_check(pmv_ctx* ctx, const char* who, int map_id, int border_value, pmv_ctx::RemapMap* map) {
    REQ(border_value >= 0 && border_value <= 255, PMV_ERR_INVALID, "%s: border_value = %d is outside 0..255", who, border_value);
    std::lock_guard<std::mutex> lk(ctx->remap_mu);
    REQ(map_id >= 0 && map_id < pmv_ctx::MAX_REMAP_MAPS && ctx->remap_maps[map_id].d, PMV_ERR_INVALID, "%s: map %d does not exist (pmv_remap_map_create)", who, map_id);
    *map = ctx->remap_maps[map_id];
    return PMV_OK;
}

extern "C" {

// cv's fixed-point form of a pair of CV_32FC1 maps, converted ONCE on the host and kept in HBM (remap_pack, pmv_device.h: 6 bytes per pixel)
int pmv_remap_map_create(pmv_ctx* ctx, int w, int h, const float* map_x, const float* map_y, int* out_id) {
    REQ(ctx, PMV_ERR_INVALID, "pmv_remap_map_create: null argument");
    REQ(map_x && map_y && out_id, PMV_ERR_INVALID, "pmv_remap_map_create: null argument");
    REQ(w >= 1 && h >= 1 && w <= ctx->max_w && h <= ctx->max_h, PMV_ERR_INVALID, "pmv_remap_map_create: a %dx%d map is outside the context's %dx%d", w, h, ctx->max_w, ctx->max_h);
    std::lock_guard<std::mutex> lk(ctx->remap_mu);
    int id = 0;
    while (id < pmv_ctx::MAX_REMAP_MAPS && ctx->remap_maps[id].d) id++;
    REQ(id < pmv_ctx::MAX_REMAP_MAPS, PMV_ERR_CAPACITY, "pmv_remap_map_create: the context holds %d maps already (pmv_remap_map_destroy one)", pmv_ctx::MAX_REMAP_MAPS);
    CKC(hipSetDevice(ctx->device));
    const size_t bytes = remap_map_bytes(w, h);
    std::vector<uint32_t> packed(bytes / 4);
    remap_pack(map_x, map_y, w, h, (uint8_t*)packed.data());
    Buf<uint8_t>& d = ctx->remap_mem[id];
    CKC(d.ensure(bytes));
    const hipError_t e = hipMemcpy(d, packed.data(), bytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) { (void)d.release(); set_err(ctx, "pmv_remap_map_create: %s", hipGetErrorString(e)); return PMV_ERR_HIP; }
    ctx->remap_maps[id].w = w; ctx->remap_maps[id].h = h; ctx->remap_maps[id].d = d;
    *out_id = id;
    return PMV_OK;
}

int pmv_remap_map_destroy(pmv_ctx* ctx, int id) {
    REQ(ctx, PMV_ERR_INVALID, "pmv_remap_map_destroy: null argument");
    // a session's upload rounds read the maps of their requests: none may go while one is open
    std::lock_guard<std::mutex> own(ctx->owner_mu);
    REQ(ctx->session_state.load() == 0, PMV_ERR_INVALID, "pmv_remap_map_destroy: a batch session is open on this context (pmv_batch_close first)");
    std::lock_guard<std::mutex> lk(ctx->remap_mu);
    REQ(id >= 0 && id < pmv_ctx::MAX_REMAP_MAPS && ctx->remap_maps[id].d, PMV_ERR_INVALID, "pmv_remap_map_destroy: map %d does not exist", id);
    // the feeders resolve the setting's maps whenever a feed begins
    for (int k = 0; k < ctx->preproc.n_maps; k++)
        REQ(ctx->preproc.map_ids[k] != id, PMV_ERR_INVALID, "pmv_remap_map_destroy: map %d is named by the frame preprocessing setting (clear it with pmv_set_frame_preproc first)", id);
    CKC(hipSetDevice(ctx->device));
    CKC(hipStreamSynchronize(ctx->s_front));
    CKC(ctx->remap_mem[id].release());
    ctx->remap_maps[id] = pmv_ctx::RemapMap();
    return PMV_OK;
}

// cv::remap on level 0 of the slots: k_remap from the slots' interiors into the chunk's scratch frames, the list-form level-0 launch from
// there, the k_pyrdown launches. A chunk of REMAP_CHUNK frames is ONE k_remap launch whatever its sizes (one map size per call, though:
// every slot must have it).
int pmv_frames_remap(pmv_ctx* ctx, int first_slot, int n, int map_id, int border_value) {
    REQ(ctx, PMV_ERR_INVALID, "pmv_frames_remap: null argument");
    pmv_ctx::RemapMap map;
    if (const int rc_ = remap_check(ctx, "pmv_frames_remap", map_id, border_value, &map)) return rc_;
    REQ(first_slot >= 0 && n >= 1 && first_slot <= ctx->n_slots - n, PMV_ERR_CAPACITY, "pmv_frames_remap: slots [%d,%d) out of range (n_slots %d)", first_slot, first_slot + n, ctx->n_slots);
    REQ(!batch_ingest_active(ctx->ingest), PMV_ERR_INVALID, "pmv_frames_remap: a pmv_frames_stream_begin bracket is open (pmv_frames_stream_end first)");
    REQ(!ctx->batch_open.load() && !batch_ingest_active(ctx->bingest), PMV_ERR_INVALID, "pmv_frames_remap: a batched run is open on this context");
    for (int i = 0; i < n; i++) REQ(ctx->slot_state[first_slot + i] != SLOT_EMPTY, PMV_ERR_INVALID, "pmv_frames_remap: slot %d is empty (never staged or uploaded)", first_slot + i);
    for (int i = 0; i < n; i++) {
        const PyrLayout& L = ctx->slot_layout[first_slot + i];
        REQ(L.w[0] == map.w && L.h[0] == map.h, PMV_ERR_INVALID, "pmv_frames_remap: slot %d holds a %dx%d frame, map %d is %dx%d", first_slot + i, L.w[0], L.h[0], map_id, map.w, map.h);
    }
    tl_prof = &ctx->prof;
    CKC(hipSetDevice(ctx->device));
    constexpr int CH = pmv_ctx::REMAP_CHUNK;
    constexpr size_t tab_bytes = (size_t)CH * (sizeof(RemapRec) + sizeof(PyrListEntry) + sizeof(PyrLayout));
    CKC(ctx->h_remap.ensure(tab_bytes)); CKC(ctx->d_remap.ensure(tab_bytes)); CKC(ctx->d_remap_scratch.ensure((size_t)CH * remap_frame_bytes(ctx->max_w, ctx->max_h)));
    Carve c(ctx->h_remap.p, ctx->d_remap.p, tab_bytes);   // chunk tables, pinned mirror and HBM copy: [records | list entries | geometry table]
    const Carved<RemapRec> c_recs = c.take<RemapRec>(CH);
    const Carved<PyrListEntry> c_list = c.take<PyrListEntry>(CH);
    const Carved<PyrLayout> c_tab = c.take<PyrLayout>(CH);
    RemapRec* recs = c_recs.h; PyrListEntry* list = c_list.h; PyrLayout* tab = c_tab.h;
    const RemapRec* d_recs = c_recs.d; const PyrListEntry* d_list = c_list.d; const PyrLayout* d_tab = c_tab.d;
    const PyrLayout L = ctx->slot_layout[first_slot];   // (one size per call: the map's)
    const size_t fb = remap_frame_bytes(L.w[0], L.h[0]);
    tab[0] = L;
    for (int i0 = 0; i0 < n; i0 += CH) {
        const int nb = std::min(CH, n - i0);
        for (int i = 0; i < nb; i++) {
            recs[i].map = (const uint32_t*)map.d; recs[i].dst_off = (unsigned long long)((size_t)i * fb);
            recs[i].slot = first_slot + i0 + i; recs[i].geom = 0; recs[i].border = border_value; recs[i].reserved = 0;
            list[i].src = ctx->d_remap_scratch + (size_t)i * fb; list[i].slot = first_slot + i0 + i; list[i].geom = 0;
        }
        CKC(hipMemcpyAsync(ctx->d_remap, ctx->h_remap, tab_bytes, hipMemcpyHostToDevice, ctx->s_front));
        CKC(launch_remap(ctx->s_front, ctx->d_slots, d_tab, d_recs, nb, L.w[0], L.h[0], ctx->d_remap_scratch));
        ctx->remap_launches[0]++;
        CKC(launch_pad_level0_list(ctx->s_front, ctx->d_slots, d_tab, L, d_list, nb));
        for (int l = 1; l < L.n_levels; l++) CKC(launch_pyrdown_list(ctx->s_front, ctx->d_slots, d_tab, L, l, d_list, nb));
        CKC(hipStreamSynchronize(ctx->s_front));   // (the next chunk rewrites the pinned tables and the scratch frames)
    }
    for (int k = 0; k < n; k++) ctx->slot_state[first_slot + k] = SLOT_BUILT;
    return PMV_OK;
}
int pmv_debug_remap_launches(pmv_ctx* ctx, long long* out3) {
    REQ(ctx && out3, PMV_ERR_INVALID, "pmv_debug_remap_launches: null argument");
    for (int i = 0; i < 3; i++) out3[i] = ctx->remap_launches[i].load();
    return PMV_OK;
}

// Remap and / or CLAHE of every host frame that a feeder moves into a slot (ingest_batch.hip): validated here, read by batch_ingest_begin.
// Not while a feed is open: a feed works from its own snapshot, and the maps it reads must stay.
int pmv_set_frame_preproc(pmv_ctx* ctx, const pmv_frame_preproc* p) {
    REQ(ctx, PMV_ERR_INVALID, "pmv_set_frame_preproc: null ctx");
    pmv_frame_preproc q = {};
    if (p) {
        REQ(p->n_maps >= 0 && p->n_maps <= PMV_PREPROC_MAX_MAPS, PMV_ERR_INVALID, "pmv_set_frame_preproc: n_maps = %d is outside 0..%d", p->n_maps, PMV_PREPROC_MAX_MAPS);
        REQ(p->border_value >= 0 && p->border_value <= 255, PMV_ERR_INVALID, "pmv_set_frame_preproc: border_value = %d is outside 0..255", p->border_value);
        if (p->clahe) {
            if (const int rc_ = clahe_check(ctx, "pmv_set_frame_preproc", &p->clahe_params)) return rc_;
            q.clahe = 1; q.clahe_params = p->clahe_params;
        }
        std::lock_guard<std::mutex> lk(ctx->remap_mu);
        for (int k = 0; k < p->n_maps; k++) {
            const int id = p->map_ids[k];
            REQ(id >= 0 && id < pmv_ctx::MAX_REMAP_MAPS && ctx->remap_maps[id].d, PMV_ERR_INVALID, "pmv_set_frame_preproc: map %d does not exist (pmv_remap_map_create)", id);
            for (int j = 0; j < k; j++) {
                const pmv_ctx::RemapMap &a = ctx->remap_maps[p->map_ids[j]], &b = ctx->remap_maps[id];
                REQ(a.w != b.w || a.h != b.h, PMV_ERR_INVALID, "pmv_set_frame_preproc: maps %d and %d are both %dx%d: one map per frame size", p->map_ids[j], id, b.w, b.h);
            }
            q.map_ids[k] = id;
        }
        q.n_maps = p->n_maps;
        q.border_value = p->border_value;
    }
    REQ(!batch_ingest_active(ctx->ingest), PMV_ERR_INVALID, "pmv_set_frame_preproc: a pmv_frames_stream_begin bracket is open (pmv_frames_stream_end first)");
    REQ(!ctx->batch_open.load() && !batch_ingest_active(ctx->bingest), PMV_ERR_INVALID, "pmv_set_frame_preproc: a batched run is open on this context");
    std::lock_guard<std::mutex> lk(ctx->remap_mu);   // (pmv_remap_map_destroy reads the setting under it)
    ctx->preproc = q;
    return PMV_OK;
}
int pmv_get_frame_preproc(pmv_ctx* ctx, pmv_frame_preproc* out) {
    REQ(ctx && out, PMV_ERR_INVALID, "pmv_get_frame_preproc: null argument");
    *out = ctx->preproc;
    return PMV_OK;
}
int pmv_debug_preproc_launches(pmv_ctx* ctx, long long* out4) {
    REQ(ctx && out4, PMV_ERR_INVALID, "pmv_debug_preproc_launches: null argument");
    for (int i = 0; i < 4; i++) out4[i] = ctx->preproc_launches[i].load();
    return PMV_OK;
}

// cv::initUndistortRectifyMap(.., CV_32FC1) on the host; no context (the message goes where pmv_last_error(NULL) finds it)
int pmv_undistort_map_build(const double* K9, const double* dist8, const double* R9_or_null, const double* newK9_or_null, int w, int h, float* map_x, float* map_y) {
    pmv_ctx* ctx = nullptr;
    REQ(K9 && dist8 && map_x && map_y, PMV_ERR_INVALID, "pmv_undistort_map_build: null argument");
    REQ(w >= 1 && h >= 1, PMV_ERR_INVALID, "pmv_undistort_map_build: size %dx%d", w, h);
    REQ(undistort_map(K9, dist8, R9_or_null, newK9_or_null, w, h, map_x, map_y), PMV_ERR_INVALID, "pmv_undistort_map_build: newK R is singular");
    return PMV_OK;
}
// cv::fisheye::initUndistortRectifyMap(.., CV_32FC1) on the host, in the same shape
int pmv_fisheye_map_build(const double* K9, const double* k4, const double* R9_or_null, const double* newK9_or_null, int w, int h, float* map_x, float* map_y) {
    pmv_ctx* ctx = nullptr;
    REQ(K9 && k4 && map_x && map_y, PMV_ERR_INVALID, "pmv_fisheye_map_build: null argument");
    REQ(w >= 1 && h >= 1, PMV_ERR_INVALID, "pmv_fisheye_map_build: size %dx%d", w, h);
    REQ(fisheye_map(K9, k4, R9_or_null, newK9_or_null, w, h, map_x, map_y), PMV_ERR_INVALID, "pmv_fisheye_map_build: newK R is singular");
    return PMV_OK;
}

}  // extern "C"

extern "C" {

int pmv_frame_num_levels(pmv_ctx* ctx, int slot) {
    if (!ctx || slot < 0 || slot >= ctx->n_slots) return PMV_ERR_INVALID;
    return ctx->slot_state[slot] == SLOT_BUILT ? ctx->slot_layout[slot].n_levels - 1 : PMV_ERR_INVALID;
}

int pmv_frame_get_level(pmv_ctx* ctx, int slot, int level, uint8_t* out, int* w, int* h) {
    REQ(ctx && out, PMV_ERR_INVALID, "null argument");
    REQ(slot >= 0 && slot < ctx->n_slots, PMV_ERR_CAPACITY, "slot out of range");
    const PyrLayout& L = ctx->slot_layout[slot];
    REQ(ctx->slot_state[slot] == SLOT_BUILT && level >= 0 && level < L.n_levels, PMV_ERR_INVALID, "level %d not built for slot %d", level, slot);
    CKC(hipSetDevice(ctx->device));
    CKC(hipStreamSynchronize(ctx->s_front));
    const uint8_t* org = level_origin((const uint8_t*)ctx->d_slots + (size_t)slot * L.slot_bytes, L, level);
    CKC(hipMemcpy2D(out, L.w[level], org, L.stride[level], L.w[level], L.h[level], hipMemcpyDeviceToHost));
    if (w) *w = L.w[level];
    if (h) *h = L.h[level];
    return PMV_OK;
}

int pmv_frame_get_level_padded(pmv_ctx* ctx, int slot, int level, uint8_t* out, int* pw, int* ph) {
    REQ(ctx && out, PMV_ERR_INVALID, "null argument");
    REQ(slot >= 0 && slot < ctx->n_slots, PMV_ERR_CAPACITY, "slot out of range");
    const PyrLayout& L = ctx->slot_layout[slot];
    REQ(ctx->slot_state[slot] == SLOT_BUILT && level >= 0 && level < L.n_levels, PMV_ERR_INVALID, "level %d not built for slot %d", level, slot);
    static_assert(PAD == PMV_PYR_PAD, "header constant");
    CKC(hipSetDevice(ctx->device));
    CKC(hipStreamSynchronize(ctx->s_front));
    const uint8_t* base = (const uint8_t*)ctx->d_slots + (size_t)slot * L.slot_bytes + L.off[level];
    const int w = L.w[level] + 2 * PAD, h = L.h[level] + 2 * PAD;
    CKC(hipMemcpy2D(out, w, base, L.stride[level], w, h, hipMemcpyDeviceToHost));
    if (pw) *pw = w;
    if (ph) *ph = h;
    return PMV_OK;
}

int pmv_lk_track(pmv_ctx* ctx, int prev_slot, int next_slot, const float* prev_xy, int n, float* out_xy,
                 uint8_t* out_status, float* out_err) {
    REQ(ctx, PMV_ERR_INVALID, "pmv_lk_track: null argument");
    if (const int rc_ = lk_check(ctx, true, prev_slot, next_slot, prev_xy, n, out_xy, out_status, out_err)) return rc_;
    const PyrLayout& L = ctx->slot_layout[prev_slot];
    if (n == 0) return PMV_OK;
    tl_prof = &ctx->prof;
    CKC(hipSetDevice(ctx->device));
    memcpy(ctx->h_prev_xy, prev_xy, (size_t)n * 8);
    const int nb = (n + 7) / 8 * 8;
    lk_xcd_order(prev_xy, n, (int*)(ctx->h_prev_xy + (size_t)2 * n));
    CKC(hipMemcpyAsync(ctx->d_prev_xy, ctx->h_prev_xy, (size_t)n * 8 + (size_t)nb * 4, hipMemcpyHostToDevice, ctx->s_front));
    LKParams P = lk_launch_params(ctx);
    static const bool lk_stamps = getenv("PMV_LK_STAMPS") != nullptr;   // read once per process
    if (!ctx->d_lk_stamps && lk_stamps) { CKC(ctx->d_lk_stamps.ensure(16 * 8)); CKC(hipMemset(ctx->d_lk_stamps, 0, 16 * 8)); }
    P.stamps = ctx->d_lk_stamps;
    CKC(launch_lk(ctx->s_front, ctx->d_slots + (size_t)prev_slot * L.slot_bytes, ctx->d_slots + (size_t)next_slot * L.slot_bytes,
                  L, ctx->d_prev_xy, (const int*)(ctx->d_prev_xy + (size_t)2 * n), nb, n, P, ctx->h_out_xy.dm(), ctx->h_status.dm(), ctx->h_err.dm(), ctx->h_work.dm()));
    CKC(hipStreamSynchronize(ctx->s_front));   // the kernel wrote positions / status / err straight into mapped pinned memory
    memcpy(out_xy, ctx->h_out_xy, (size_t)n * 8);
    memcpy(out_status, ctx->h_status, (size_t)n);
    memcpy(out_err, ctx->h_err, (size_t)n * 4);
    ctx->add_lk_work(ctx->h_work, (size_t)n);
    return PMV_OK;
}

// pmv_lk_track_ex, pmv_lk_track_fb and pmv_lk_track_fb_levels: pmv_lk_track's steps around ONE launch of the extended kernels; top_f / top_b:
// the level caps of the two trips, -1 = the slot's top level
static int lk_single_ex(pmv_ctx* ctx, const char* who, int prev_slot, int next_slot, const float* prev_xy, int n, float* next_xy, int flags, uint8_t* out_status, float* out_err,
                        bool fb, float* back_xy, uint8_t* back_status, float* back_err, int top_f = -1, int top_b = -1) {
    REQ(ctx, PMV_ERR_INVALID, "%s: null argument", who);
    REQ(top_f >= -1 && top_f < MAX_LEVELS && top_b >= -1 && top_b < MAX_LEVELS, PMV_ERR_INVALID, "%s: fwd_top_level = %d, back_top_level = %d: outside -1..%d", who, top_f,
        top_b, MAX_LEVELS - 1);
    if (const int rc_ = lkx_check(ctx, who, true, prev_slot, next_slot, prev_xy, n, next_xy, flags, out_status, out_err, fb, back_xy, back_status, back_err)) return rc_;
    const PyrLayout& L = ctx->slot_layout[prev_slot];
    if (n == 0) return PMV_OK;
    tl_prof = &ctx->prof;
    CKC(hipSetDevice(ctx->device));
    const size_t nt = (size_t)ctx->max_tracks;
    // [initial flow of max_tracks tracks | their back block]
    Carved<float> init; LkBackBlock back;
    auto lkx_block = [&](Carve c) { init = c.take<float>(2 * nt); back = lk_back_block(c, nt); return c.bytes(); };
    CKC(ctx->h_lkx.ensure(lkx_block(Carve()) + 64));
    lkx_block(carve_of(ctx->h_lkx));
    if (flags & PMV_LK_USE_INITIAL_FLOW) memcpy(init.h, next_xy, (size_t)n * 8);
    memcpy(ctx->h_prev_xy, prev_xy, (size_t)n * 8);
    const int nb = (n + 7) / 8 * 8;
    lk_xcd_order(prev_xy, n, (int*)(ctx->h_prev_xy + (size_t)2 * n));
    CKC(hipMemcpyAsync(ctx->d_prev_xy, ctx->h_prev_xy, (size_t)n * 8 + (size_t)nb * 4, hipMemcpyHostToDevice, ctx->s_front));
    const LKParams P = lk_launch_params(ctx);
    CKC(launch_lk_ex(ctx->s_front, ctx->d_slots + (size_t)prev_slot * L.slot_bytes, ctx->d_slots + (size_t)next_slot * L.slot_bytes, L, ctx->d_prev_xy,
                     init.d, (const int*)(ctx->d_prev_xy + (size_t)2 * n), nb, n, flags | (fb ? LKX_FB : 0), P, ctx->h_out_xy.dm(), ctx->h_status.dm(),
                     ctx->h_err.dm(), ctx->h_work.dm(), back.xy.d, back.status.d, back.err.d, top_f, top_b));
    CKC(hipStreamSynchronize(ctx->s_front));
    memcpy(next_xy, ctx->h_out_xy, (size_t)n * 8);
    memcpy(out_status, ctx->h_status, (size_t)n);
    memcpy(out_err, ctx->h_err, (size_t)n * 4);
    if (fb) {
        memcpy(back_xy, back.xy.h, (size_t)n * 8);
        memcpy(back_status, back.status.h, (size_t)n);
        memcpy(back_err, back.err.h, (size_t)n * 4);
    }
    ctx->add_lk_work(ctx->h_work, (size_t)n);
    return PMV_OK;
}
int pmv_lk_track_ex(pmv_ctx* ctx, int prev_slot, int next_slot, const float* prev_xy, int n, float* next_xy, int flags, uint8_t* out_status, float* out_err) {
    return lk_single_ex(ctx, "pmv_lk_track_ex", prev_slot, next_slot, prev_xy, n, next_xy, flags, out_status, out_err, false, nullptr, nullptr, nullptr);
}
int pmv_lk_track_fb(pmv_ctx* ctx, int prev_slot, int next_slot, const float* prev_xy, int n, float* next_xy, int flags, uint8_t* out_status, float* out_err,
                    float* back_xy, uint8_t* back_status, float* back_err) {
    return lk_single_ex(ctx, "pmv_lk_track_fb", prev_slot, next_slot, prev_xy, n, next_xy, flags, out_status, out_err, true, back_xy, back_status, back_err);
}
int pmv_lk_track_fb_levels(pmv_ctx* ctx, int prev_slot, int next_slot, const float* prev_xy, int n, float* next_xy, int flags, int fwd_top_level, int back_top_level,
                           uint8_t* out_status, float* out_err, float* back_xy_or_null, uint8_t* back_status_or_null, float* back_err_or_null) {
    REQ(ctx, PMV_ERR_INVALID, "pmv_lk_track_fb_levels: null argument");
    const int n_back = (back_xy_or_null ? 1 : 0) + (back_status_or_null ? 1 : 0) + (back_err_or_null ? 1 : 0);
    REQ(n_back == 0 || n_back == 3, PMV_ERR_INVALID, "pmv_lk_track_fb_levels: %d of the three back outputs are null (all three: forward only; none: the back check)", 3 - n_back);
    return lk_single_ex(ctx, "pmv_lk_track_fb_levels", prev_slot, next_slot, prev_xy, n, next_xy, flags, out_status, out_err, n_back == 3, back_xy_or_null, back_status_or_null,
                        back_err_or_null, fwd_top_level, back_top_level);
}

}  // extern "C"
int pmv::lk_check(pmv_ctx* ctx, bool bracket, int prev_slot, int next_slot, const float* prev_xy, int n, const float* out_xy, const uint8_t* out_status, const float* out_err) {
    REQ(n == 0 || (prev_xy && out_xy && out_status && out_err), PMV_ERR_INVALID, "pmv_lk_track: null argument");
    REQ(n >= 0 && n <= ctx->max_tracks, PMV_ERR_CAPACITY, "pmv_lk_track: n=%d exceeds max_tracks=%d", n, ctx->max_tracks);
    REQ(prev_slot >= 0 && prev_slot < ctx->n_slots && next_slot >= 0 && next_slot < ctx->n_slots, PMV_ERR_CAPACITY, "pmv_lk_track: slot out of range");
    for (int s : {prev_slot, next_slot}) { int rc_ = bracket ? slot_ready(ctx, s, ctx->ingest, 0, ctx->s_front) : slot_ready(ctx, s); if (rc_) return rc_; }
    const PyrLayout& L = ctx->slot_layout[prev_slot];
    const PyrLayout& L2 = ctx->slot_layout[next_slot];
    REQ(L.w[0] == L2.w[0] && L.h[0] == L2.h[0], PMV_ERR_INVALID, "pmv_lk_track: frame sizes differ");
    return PMV_OK;
}
int pmv::lkx_check(pmv_ctx* ctx, const char* who, bool bracket, int prev_slot, int next_slot, const float* prev_xy, int n, const float* next_xy, int flags,
                   const uint8_t* out_status, const float* out_err, bool fb, const float* back_xy, const uint8_t* back_status, const float* back_err) {
    static_assert(PMV_LK_USE_INITIAL_FLOW == LKX_INIT && PMV_LK_GET_MIN_EIGENVALS == LKX_EIG, "the kernels take cv's flag values as they are");
    REQ(n <= 0 || !fb || (back_xy && back_status && back_err), PMV_ERR_INVALID, "%s: null argument", who);
    if (const int rc_ = lk_check(ctx, bracket, prev_slot, next_slot, prev_xy, n, next_xy, out_status, out_err)) return rc_;
    REQ(!(flags & ~(PMV_LK_USE_INITIAL_FLOW | PMV_LK_GET_MIN_EIGENVALS)), PMV_ERR_INVALID, "%s: flags = 0x%x has bits other than PMV_LK_USE_INITIAL_FLOW (4) and PMV_LK_GET_MIN_EIGENVALS (8)", who, (unsigned)flags);
    if (flags & PMV_LK_USE_INITIAL_FLOW)
        for (int i = 0; i < 2 * n; i++)   // (a NaN fails the comparison too)
            REQ(fabsf(next_xy[i]) <= 1e6f, PMV_ERR_INVALID, "%s: initial flow of point %d (%g, %g) is not finite or beyond 1e6", who, i / 2, (double)next_xy[i & ~1], (double)next_xy[i | 1]);
    return PMV_OK;
}
int pmv::detect_check(pmv_ctx* ctx, bool bracket, int slot, const int* cells, int n_cells, int max_per_cell) {
    REQ(cells, PMV_ERR_INVALID, "detect: null argument");
    REQ(slot >= 0 && slot < ctx->n_slots, PMV_ERR_CAPACITY, "detect: slot out of range");
    REQ(n_cells >= 1 && n_cells <= MAX_CELLS, PMV_ERR_CAPACITY, "detect: n_cells=%d (max %d)", n_cells, MAX_CELLS);
    REQ(max_per_cell >= 1 && max_per_cell <= MAX_PER_CELL, PMV_ERR_CAPACITY, "detect: max_per_cell=%d (max %d)", max_per_cell, MAX_PER_CELL);
    int rc = bracket ? slot_ready(ctx, slot, ctx->ingest, 0, ctx->s_front) : slot_ready(ctx, slot);
    if (rc) return rc;
    const PyrLayout& L = ctx->slot_layout[slot];
    for (int i = 0; i < n_cells; i++) {
        const int* c = cells + 4 * i;
        REQ(c[2] >= 3 && c[3] >= 3 && c[2] <= CELL_MAX && c[3] <= CELL_MAX && c[0] >= 0 && c[1] >= 0 && c[0] + c[2] <= L.w[0] && c[1] + c[3] <= L.h[0],
            PMV_ERR_INVALID, "detect: cell %d (%d,%d,%d,%d) invalid for %dx%d frame", i, c[0], c[1], c[2], c[3], L.w[0], L.h[0]);
    }
    return PMV_OK;
}
int pmv::gftt_ex_check(pmv_ctx* ctx, const char* who, const pmv_gftt_params* p, const int* out_xy, const int* out_count) {
    REQ(p && out_xy && out_count, PMV_ERR_INVALID, "%s: null argument", who);
    REQ(p->block_size >= 1 && p->block_size <= GFTT_MAX_BLOCK, PMV_ERR_INVALID, "%s: block_size = %d is outside 1..%d", who, p->block_size, GFTT_MAX_BLOCK);
    REQ(p->quality > 0.0 && p->quality <= 1.0, PMV_ERR_INVALID, "%s: quality = %g is outside (0, 1]", who, p->quality);   // (a NaN fails the comparison too)
    REQ(p->min_dist >= 0.0 && std::isfinite(p->min_dist), PMV_ERR_INVALID, "%s: min_dist = %g is negative or not finite", who, p->min_dist);
    REQ(!p->use_harris || std::isfinite(p->k), PMV_ERR_INVALID, "%s: k = %g is not finite", who, p->k);
    return PMV_OK;
}
int pmv::gftt_mask_check(pmv_ctx* ctx, const char* who, int slot, const uint8_t* mask, int mask_stride) {   // after detect_check: the slot is valid
    REQ(!mask || mask_stride >= ctx->slot_layout[slot].w[0], PMV_ERR_CAPACITY, "%s: mask_stride = %d is below the frame width %d", who, mask_stride, ctx->slot_layout[slot].w[0]);
    return PMV_OK;
}
// The record of a corner, (y << 16) | x, the 31-bit pixel index y * w + x of a pass-1 record and the int distances of the selection hold
// for every region this check lets through: sides up to GFTT_FRAME_MAX_SIDE, fewer than 2^31 pixels.
int pmv::gftt_frame_check(pmv_ctx* ctx, const char* who, bool bracket, int slot, const int* roi4_or_null, int max_corners, const pmv_gftt_params* p, const uint8_t* mask,
                          int mask_stride, const int* out_xy, int out_cap, const int* out_count, int* roi4, int* cap) {
    static_assert(PMV_GFTT_FRAME_MAX_CORNERS == GFTT_FRAME_ONCHIP, "a call may return as many corners as the selection kernel sorts on chip");
    static_assert(GFTT_FRAME_MAX_SIDE <= 0xffff && 2ll * GFTT_FRAME_MAX_SIDE * GFTT_FRAME_MAX_SIDE <= INT_MAX, "(y << 16) | x; dx * dx + dy * dy in an int");
    if (const int rc = gftt_ex_check(ctx, who, p, out_xy, out_count)) return rc;
    REQ(slot >= 0 && slot < ctx->n_slots, PMV_ERR_CAPACITY, "%s: slot out of range", who);
    *cap = max_corners > 0 ? max_corners : out_cap;
    REQ(*cap >= 1 && *cap <= out_cap && *cap <= PMV_GFTT_FRAME_MAX_CORNERS, PMV_ERR_CAPACITY, "%s: max_corners = %d with out_cap = %d: the list must hold 1..%d corners",
        who, max_corners, out_cap, PMV_GFTT_FRAME_MAX_CORNERS);
    if (const int rc = bracket ? slot_ready(ctx, slot, ctx->ingest, 0, ctx->s_front) : slot_ready(ctx, slot)) return rc;
    const PyrLayout& L = ctx->slot_layout[slot];
    if (roi4_or_null) memcpy(roi4, roi4_or_null, 4 * sizeof(int));
    else { roi4[0] = 0; roi4[1] = 0; roi4[2] = L.w[0]; roi4[3] = L.h[0]; }
    REQ(roi4[2] >= 3 && roi4[3] >= 3 && roi4[0] >= 0 && roi4[1] >= 0 && roi4[2] <= L.w[0] - roi4[0] && roi4[3] <= L.h[0] - roi4[1], PMV_ERR_INVALID,
        "%s: region (%d,%d,%d,%d) is smaller than 3x3 or not inside the %dx%d frame", who, roi4[0], roi4[1], roi4[2], roi4[3], L.w[0], L.h[0]);
    REQ(L.w[0] <= GFTT_FRAME_MAX_SIDE && L.h[0] <= GFTT_FRAME_MAX_SIDE && (long long)ctx->max_w * ctx->max_h <= INT_MAX, PMV_ERR_CAPACITY,
        "%s: a %dx%d frame is beyond the %d pixels a side (2^31 a frame) the corner records hold", who, L.w[0], L.h[0], GFTT_FRAME_MAX_SIDE);
    return gftt_mask_check(ctx, who, slot, mask, mask_stride);
}
size_t pmv::gftt_frame_record(int* rec, const int* roi4, int slot, size_t list_off, uint8_t* dst, size_t pos, const uint8_t* mask, int mask_stride) {
    pack_cells(rec, roi4, 1, slot);
    rec[6] = (int)(unsigned)(list_off & 0xffffffffu); rec[7] = (int)(unsigned)(list_off >> 32);
    return mask ? gftt_pack_mask(dst, pos, rec, roi4, 1, mask, mask_stride) : pos;
}
int pmv::refill_check(pmv_ctx* ctx, const char* who, int slot, const float* track_xy, int n_tracks, int radius, const uint8_t* out_keep) {   // after gftt_frame_check: the slot is valid
    static_assert(PMV_REFILL_MAX_TRACKS == REFILL_MAX_TRACKS && PMV_REFILL_MAX_RADIUS == REFILL_MAX_RADIUS, "the header's limits are the kernels'");
    REQ(out_keep && (track_xy || n_tracks <= 0), PMV_ERR_INVALID, "%s: null argument", who);
    REQ(radius >= 0 && radius <= PMV_REFILL_MAX_RADIUS, PMV_ERR_INVALID, "%s: radius = %d is outside 0..%d", who, radius, PMV_REFILL_MAX_RADIUS);
    const int max_n = std::min(ctx->max_tracks, PMV_REFILL_MAX_TRACKS);
    REQ(n_tracks >= 0 && n_tracks <= max_n, PMV_ERR_CAPACITY, "%s: n_tracks = %d is outside 0..%d (max_tracks, PMV_REFILL_MAX_TRACKS)", who, n_tracks, max_n);
    const PyrLayout& L = ctx->slot_layout[slot];
    for (int i = 0; i < n_tracks; i++) {   // (a NaN fails the comparison too)
        const float x = track_xy[2 * i], y = track_xy[2 * i + 1];
        REQ(fabsf(x) <= 1e6f && fabsf(y) <= 1e6f, PMV_ERR_INVALID, "%s: track %d (%g, %g) is not finite or beyond 1e6", who, i, (double)x, (double)y);
        const long px = lrintf(x), py = lrintf(y);   // cvRound: half to even
        REQ(px >= 0 && px < L.w[0] && py >= 0 && py < L.h[0], PMV_ERR_INVALID, "%s: track %d rounds to the point (%ld, %ld), outside the %dx%d frame", who, i, px, py, L.w[0], L.h[0]);
    }
    return PMV_OK;
}
void pmv::refill_fill(const RefillBlock& B, size_t i, size_t trk_off, const int* roi4, size_t mask_off, const float* track_xy, const int* track_prio_or_null, int n_tracks,
                      int radius, const uint8_t* base_mask_or_null, int base_stride) {
    RefillRec& R = B.rec.h[i];
    R = RefillRec{n_tracks, radius, (int)trk_off, roi4[0], roi4[1], roi4[2], roi4[3], (unsigned)mask_off, base_mask_or_null ? 1 : 0, {0, 0, 0}};
    unsigned* pos = B.pos.h + trk_off; int* prio = B.prio.h + trk_off; uint8_t* flag = B.flag.h + trk_off;
    for (int t = 0; t < n_tracks; t++) {
        const int x = (int)lrintf(track_xy[2 * t]), y = (int)lrintf(track_xy[2 * t + 1]);
        pos[t] = ((unsigned)y << 16) | (unsigned)x;
        prio[t] = track_prio_or_null ? track_prio_or_null[t] : 0;
        flag[t] = base_mask_or_null ? base_mask_or_null[(size_t)y * (size_t)base_stride + x] == 255 : 1;   // setMask tests `== 255`
    }
    refill_halfwidths(radius, B.hw.h + i * REFILL_HW);
}
int pmv::shitomasi_nothing(pmv_ctx* ctx, const int* cells, int n_cells, int* out_count) {   // ShiTomasiFeatureExtractor.cpp:37-44: `if (i >= max) break` before the first feature
    REQ(cells && out_count && n_cells >= 1 && n_cells <= MAX_CELLS, PMV_ERR_INVALID, "pmv_detect_shitomasi: bad argument");
    for (int i = 0; i < n_cells; i++) out_count[i] = 0;
    return PMV_OK;
}
void pmv::pack_cells(int* dst, const int* cells, int n_cells, int slot) {
    for (int i = 0; i < n_cells; i++) {
        int* d = dst + (size_t)i * CELL_STRIDE;
        d[0] = cells[4 * i]; d[1] = cells[4 * i + 1]; d[2] = cells[4 * i + 2]; d[3] = cells[4 * i + 3]; d[4] = slot; d[5] = d[6] = d[7] = 0;
    }
}
// the cells' mask sub-views one after the other (cw * ch bytes each); the byte offset of each goes into int 5 of its device cell record
size_t pmv::gftt_pack_mask(uint8_t* dst, size_t pos, int* cell_recs, const int* cells, int n_cells, const uint8_t* mask, int mask_stride) {
    for (int i = 0; i < n_cells; i++) {
        const int* c = cells + 4 * i;
        cell_recs[(size_t)i * CELL_STRIDE + 5] = (int)pos;
        for (int y = 0; y < c[3]; y++, pos += (size_t)c[2]) memcpy(dst + pos, mask + (size_t)(c[1] + y) * (size_t)mask_stride + c[0], (size_t)c[2]);
    }
    return pos;
}
int pmv::subpix_params_check(pmv_ctx* ctx, const char* who, const pmv_subpix_params* p) {
    REQ(p->win_w >= 1 && p->win_w <= SUBPIX_MAX_WIN && p->win_h >= 1 && p->win_h <= SUBPIX_MAX_WIN, PMV_ERR_INVALID, "%s: win = (%d, %d) is outside 1..%d", who, p->win_w, p->win_h, SUBPIX_MAX_WIN);
    REQ(p->max_iter >= 1 && p->max_iter <= 100, PMV_ERR_INVALID, "%s: max_iter = %d is outside 1..100", who, p->max_iter);
    REQ(p->eps >= 0.0 && std::isfinite(p->eps), PMV_ERR_INVALID, "%s: eps = %g is negative or not finite", who, p->eps);   // (a NaN fails the comparison too)
    return PMV_OK;
}
int pmv::subpix_check(pmv_ctx* ctx, const char* who, bool bracket, int slot, const float* xy, int n, const pmv_subpix_params* p) {
    REQ(p && (n == 0 || xy), PMV_ERR_INVALID, "%s: null argument", who);
    if (const int rc_ = subpix_params_check(ctx, who, p)) return rc_;
    REQ(n >= 0 && n <= ctx->max_tracks, PMV_ERR_CAPACITY, "%s: n=%d exceeds max_tracks=%d", who, n, ctx->max_tracks);
    REQ(slot >= 0 && slot < ctx->n_slots, PMV_ERR_CAPACITY, "%s: slot out of range", who);
    if (const int rc_ = bracket ? slot_ready(ctx, slot, ctx->ingest, 0, ctx->s_front) : slot_ready(ctx, slot)) return rc_;
    for (int i = 0; i < 2 * n; i++)   // (a NaN fails the comparison too)
        REQ(fabsf(xy[i]) <= 1e6f, PMV_ERR_INVALID, "%s: point %d (%g, %g) is not finite or beyond 1e6", who, i / 2, (double)xy[i & ~1], (double)xy[i | 1]);
    return PMV_OK;
}
static int check_cells(pmv_ctx* ctx, int slot, const int* cells, int n_cells, int max_per_cell) {   // max_per_cell: already >= 1
    REQ(ctx, PMV_ERR_INVALID, "detect: null argument");
    return detect_check(ctx, true, slot, cells, n_cells, max_per_cell);
}
// What the three detector entry points do around their launch: the packed cell records (ctx->h_cells) go up, the overflow bits are cleared
// (they are per call: one overflow must not poison later calls), `launch` enqueues the kernels, then lists, counts and flags come back in one
// wait. out_score may be null. overflow_who: the call whose "no limit" form fails with PMV_ERR_OVERFLOW, outputs untouched.
template <class Launch>
static int detect_run(pmv_ctx* ctx, int n_cells, int per_cell, Launch launch, const char* overflow_who, int* out_xy, double* out_score, int* out_count) {
    CKC(hipMemcpyAsync(ctx->d_cells, ctx->h_cells, (size_t)n_cells * CELL_STRIDE * 4, hipMemcpyHostToDevice, ctx->s_front));
    CKC(hipMemsetAsync(ctx->d_flags, 0, 16, ctx->s_front));
    CKC(launch());
    const size_t nxy = (size_t)n_cells * per_cell * 8;
    CKC(hipMemcpyAsync(ctx->h_det_xy, ctx->d_det_xy, nxy, hipMemcpyDeviceToHost, ctx->s_front));
    if (out_score) CKC(hipMemcpyAsync(ctx->h_det_score, ctx->d_det_score, nxy, hipMemcpyDeviceToHost, ctx->s_front));
    CKC(hipMemcpyAsync(ctx->h_det_count, ctx->d_det_count, (size_t)n_cells * 4, hipMemcpyDeviceToHost, ctx->s_front));
    CKC(hipMemcpyAsync(ctx->h_det_count + MAX_CELLS, ctx->d_flags, 4, hipMemcpyDeviceToHost, ctx->s_front));
    CKC(hipStreamSynchronize(ctx->s_front));
    REQ(!overflow_who || (ctx->h_det_count[MAX_CELLS] & 4) == 0, PMV_ERR_OVERFLOW, "%s: more than %d corners in a cell with max_per_cell <= 0 (no limit)", overflow_who, MAX_PER_CELL);
    memcpy(out_xy, ctx->h_det_xy, nxy);
    if (out_score) memcpy(out_score, ctx->h_det_score, nxy);
    memcpy(out_count, ctx->h_det_count, (size_t)n_cells * 4);
    return PMV_OK;
}

extern "C" {

int pmv_detect_gftt(pmv_ctx* ctx, int slot, const int* cells, int n_cells, int max_per_cell, double quality,
                    double min_dist, int* out_xy, int* out_count) {
    // cv::goodFeaturesToTrack: maxCorners <= 0 means "no limit" (the reference gets there when min_tracked_features < number of
    // grid cells, OdometryPipeline.cpp:438 integer division). The caller's out_xy then holds PMV_GFTT_UNLIMITED_CAP corners per cell.
    const int unlimited = max_per_cell <= 0;
    if (unlimited) max_per_cell = MAX_PER_CELL;
    int rc = check_cells(ctx, slot, cells, n_cells, max_per_cell);
    if (rc) return rc;
    REQ(out_xy && out_count, PMV_ERR_INVALID, "pmv_detect_gftt: null output");
    tl_prof = &ctx->prof;
    CKC(hipSetDevice(ctx->device));
    const PyrLayout& L = ctx->slot_layout[slot];
    pack_cells(ctx->h_cells, cells, n_cells, slot);
    static const bool gftt_dbg = getenv("PMV_GFTT_DBG") != nullptr;
    rc = detect_run(ctx, n_cells, max_per_cell, [&] {
        if (gftt_dbg) { static const int on = 0x40000000; if (hipError_t e = hipMemcpyAsync(ctx->d_flags, &on, 4, hipMemcpyHostToDevice, ctx->s_front)) return e; }
        return launch_gftt(ctx->s_front, ctx->d_slots, L, ctx->d_cells, n_cells, max_per_cell, quality, min_dist, unlimited, (float*)ctx->d_eig, (unsigned*)ctx->d_cellmax,
                           ctx->d_det_xy, ctx->d_det_count, ctx->d_flags, ctx->d_spill);
    }, "pmv_detect_gftt", out_xy, nullptr, out_count);
    if (gftt_dbg && (rc == PMV_OK || rc == PMV_ERR_OVERFLOW)) {
        int f[4];
        CKC(hipMemcpy(f, ctx->d_flags, 16, hipMemcpyDeviceToHost));
        fprintf(stderr, "[gftt-dbg] cell 0: %d raw records, %d above the threshold; cycles: compaction %d, key set-up %d, rounds %d\n", f[0] & 0xffff, (f[0] >> 16) & 0x3fff, f[1], f[2], f[3]);
    }
    return rc;
}

// cv::goodFeaturesToTrack with the caller's mask, blockSize, useHarrisDetector and k. The reference's arguments (3, false, no mask) are
// pmv_detect_gftt itself - the tuned kernels - unless pmv_debug_gftt_general sends them through the general ones.
int pmv_detect_gftt_ex(pmv_ctx* ctx, int slot, const int* cells, int n_cells, int max_per_cell, const pmv_gftt_params* p, const uint8_t* mask,
                       int mask_stride, int* out_xy, int* out_count) {
    REQ(ctx, PMV_ERR_INVALID, "pmv_detect_gftt_ex: null argument");
    int rc = gftt_ex_check(ctx, "pmv_detect_gftt_ex", p, out_xy, out_count);
    if (rc) return rc;
    const int unlimited = max_per_cell <= 0;
    const int cap = unlimited ? MAX_PER_CELL : max_per_cell;
    rc = check_cells(ctx, slot, cells, n_cells, cap);
    if (rc) return rc;
    rc = gftt_mask_check(ctx, "pmv_detect_gftt_ex", slot, mask, mask_stride);
    if (rc) return rc;
    if (p->block_size == 3 && !p->use_harris && !mask && !ctx->gftt_general)
        return pmv_detect_gftt(ctx, slot, cells, n_cells, max_per_cell, p->quality, p->min_dist, out_xy, out_count);
    tl_prof = &ctx->prof;
    CKC(hipSetDevice(ctx->device));
    const PyrLayout& L = ctx->slot_layout[slot];
    pack_cells(ctx->h_cells, cells, n_cells, slot);
    if (mask) {
        CKC(ctx->h_gmask.ensure((size_t)MAX_CELLS * CELL_PIX)); CKC(ctx->d_gmask.ensure((size_t)MAX_CELLS * CELL_PIX));
        const size_t nb = gftt_pack_mask(ctx->h_gmask, 0, ctx->h_cells, cells, n_cells, mask, mask_stride);
        CKC(hipMemcpyAsync(ctx->d_gmask, ctx->h_gmask, nb, hipMemcpyHostToDevice, ctx->s_front));
    }
    return detect_run(ctx, n_cells, cap, [&] {
        return launch_gftt_ex(ctx->s_front, ctx->d_slots, L, ctx->d_cells, n_cells, cap, p->quality, p->min_dist, unlimited, gftt_ext(p->block_size, p->use_harris, p->k),
                              mask ? ctx->d_gmask.get() : nullptr, (float*)ctx->d_eig, (unsigned*)ctx->d_cellmax, ctx->d_det_xy, ctx->d_det_count, ctx->d_flags, ctx->d_spill);
    }, "pmv_detect_gftt_ex", out_xy, nullptr, out_count);
}
// cv::goodFeaturesToTrack on one region of any size: ONE request of the frame kernels (k_gftt_cand_frame or k_gftt_cand_general_frame, then
// k_gftt_pick_frame). Record, count, statistics and the corner list live in one mapped pinned block: one wait, no copy calls.
int pmv_detect_gftt_frame(pmv_ctx* ctx, int slot, const int* roi4_or_null, int max_corners, const pmv_gftt_params* p, const uint8_t* mask, int mask_stride,
                          int* out_xy, int out_cap, int* out_count) {
    REQ(ctx, PMV_ERR_INVALID, "pmv_detect_gftt_frame: null argument");
    int roi[4], cap;
    if (const int rc = gftt_frame_check(ctx, "pmv_detect_gftt_frame", true, slot, roi4_or_null, max_corners, p, mask, mask_stride, out_xy, out_cap, out_count, roi, &cap)) return rc;
    tl_prof = &ctx->prof;
    CKC(hipSetDevice(ctx->device));
    const PyrLayout& L = ctx->slot_layout[slot];
    const size_t pix = (size_t)ctx->max_w * ctx->max_h;
    Carve need;
    gftt_frame_block(need, 1, PMV_GFTT_FRAME_MAX_CORNERS);
    FrameDetScratch& S = ctx->fds;
    CKC(S.lists(pix, 1, need.bytes()));
    if (mask) CKC(S.masks(pix, pix));
    Carve c = carve_of(S.h_gfr);
    const GfttFrameBlock B = gftt_frame_block(c, 1, (size_t)cap);
    const size_t nb = gftt_frame_record(B.rec.h, roi, slot, 0, S.h_gfr_mask, 0, mask, mask_stride);
    if (mask) CKC(hipMemcpyAsync(S.d_gfr_mask, S.h_gfr_mask, nb, hipMemcpyHostToDevice, ctx->s_front));
    const bool general = p->block_size != 3 || p->use_harris || mask || ctx->gftt_general;
    const GfttExt X = gftt_ext(p->block_size, p->use_harris, p->k);
    CKC(launch_gftt_frame(ctx->s_front, ctx->d_slots, L, B.rec.d, 1, gftt_frame_grid_x(roi[2], roi[3]), cap, p->quality, p->min_dist, max_corners <= 0, general ? &X : nullptr,
                          mask ? S.d_gfr_mask.get() : nullptr, S.d_gfr_val, S.d_gfr_idx, S.d_gfr_info, S.d_gfr_keys, B.xy.d, B.count.d, B.stats.d));
    CKC(hipStreamSynchronize(ctx->s_front));
    ctx->gftt_frame_stats[0]++; ctx->gftt_frame_stats[3] = B.stats.h[0]; ctx->gftt_frame_stats[4] = B.stats.h[1];
    const int n = B.count.h[0];
    REQ(n >= 0, PMV_ERR_OVERFLOW, "pmv_detect_gftt_frame: more than out_cap = %d corners with max_corners <= 0 (no limit)", out_cap);
    memcpy(out_xy, B.xy.h, (size_t)n * 8);
    *out_count = n;
    return PMV_OK;
}
int pmv_debug_gftt_frame_stats(pmv_ctx* ctx, long long* out6) {
    REQ(ctx && out6, PMV_ERR_INVALID, "pmv_debug_gftt_frame_stats: null argument");
    for (int i = 0; i < 5; i++) out6[i] = ctx->gftt_frame_stats[i].load();
    out6[5] = GFTT_FRAME_ONCHIP;
    return PMV_OK;
}
// pmv_detect_gftt_frame with the mask made on the device from the caller's tracks: k_track_select and k_track_paint in front of the frame
// kernels (the general pass 1: there is a mask), one wait. Only a base mask crosses the bus, packed as gftt_frame_record packs a mask.
int pmv_detect_gftt_refill(pmv_ctx* ctx, int slot, const int* roi4_or_null, int max_corners, const pmv_gftt_params* p, const float* track_xy,
                           const int* track_prio_or_null, int n_tracks, int radius, const uint8_t* base_mask_or_null, int base_stride, uint8_t* out_keep,
                           int* out_xy, int out_cap, int* out_count) {
    REQ(ctx, PMV_ERR_INVALID, "pmv_detect_gftt_refill: null argument");
    int roi[4], cap;
    if (const int rc = gftt_frame_check(ctx, "pmv_detect_gftt_refill", true, slot, roi4_or_null, max_corners, p, base_mask_or_null, base_stride, out_xy, out_cap, out_count, roi, &cap)) return rc;
    if (const int rc = refill_check(ctx, "pmv_detect_gftt_refill", slot, track_xy, n_tracks, radius, out_keep)) return rc;
    tl_prof = &ctx->prof;
    CKC(hipSetDevice(ctx->device));
    const PyrLayout& L = ctx->slot_layout[slot];
    const size_t pix = (size_t)ctx->max_w * ctx->max_h, rpix = (size_t)roi[2] * roi[3];
    Carve need, rneed;
    gftt_frame_block(need, 1, PMV_GFTT_FRAME_MAX_CORNERS);
    refill_block(rneed, 1, PMV_REFILL_MAX_TRACKS);
    FrameDetScratch& S = ctx->fds;
    CKC(S.lists(pix, 1, need.bytes()));
    CKC(S.masks(pix + S.PAINT_SLACK, base_mask_or_null ? pix : 0));
    CKC(S.refill(PMV_REFILL_MAX_TRACKS, 1, rneed.bytes()));
    Carve c = carve_of(S.h_gfr), rc2 = carve_of(S.h_refill);
    const GfttFrameBlock B = gftt_frame_block(c, 1, (size_t)cap);
    const RefillBlock T = refill_block(rc2, 1, refill_pad(n_tracks));
    const size_t nb = gftt_frame_record(B.rec.h, roi, slot, 0, S.h_gfr_mask, 0, base_mask_or_null, base_stride);   // (mask offset 0 either way)
    refill_fill(T, 0, 0, roi, 0, track_xy, track_prio_or_null, n_tracks, radius, base_mask_or_null, base_stride);
    if (base_mask_or_null) { CKC(hipMemcpyAsync(S.d_gfr_mask, S.h_gfr_mask, nb, hipMemcpyHostToDevice, ctx->s_front)); ctx->refill_stats[3] += (long long)nb; }
    CKC(launch_track_refill(ctx->s_front, T.rec.d, 1, rpix, T.pos.d, T.prio.d, T.flag.d, T.hw.d, T.keep.d, S.d_refill_kept, S.d_refill_nkept, S.d_gfr_mask));
    const GfttExt X = gftt_ext(p->block_size, p->use_harris, p->k);
    CKC(launch_gftt_frame(ctx->s_front, ctx->d_slots, L, B.rec.d, 1, gftt_frame_grid_x(roi[2], roi[3]), cap, p->quality, p->min_dist, max_corners <= 0, &X, S.d_gfr_mask.get(),
                          S.d_gfr_val, S.d_gfr_idx, S.d_gfr_info, S.d_gfr_keys, B.xy.d, B.count.d, B.stats.d));
    CKC(hipStreamSynchronize(ctx->s_front));
    ctx->refill_stats[0]++; ctx->refill_last[0] = roi[2]; ctx->refill_last[1] = roi[3];
    const int n = B.count.h[0];
    REQ(n >= 0, PMV_ERR_OVERFLOW, "pmv_detect_gftt_refill: more than out_cap = %d corners with max_corners <= 0 (no limit)", out_cap);
    memcpy(out_keep, T.keep.h, (size_t)n_tracks);
    memcpy(out_xy, B.xy.h, (size_t)n * 8);
    *out_count = n;
    return PMV_OK;
}
// diagnostic: the packed region mask the last pmv_detect_gftt_refill of this context painted (w * h tight bytes)
int pmv_debug_refill_mask(pmv_ctx* ctx, uint8_t* out, long long cap, int* w, int* h) {
    REQ(ctx && out && w && h, PMV_ERR_INVALID, "pmv_debug_refill_mask: null argument");
    const long long nb = (long long)ctx->refill_last[0] * ctx->refill_last[1];
    REQ(nb > 0, PMV_ERR_INVALID, "pmv_debug_refill_mask: no pmv_detect_gftt_refill call has been made on this context");
    REQ(cap >= nb, PMV_ERR_CAPACITY, "pmv_debug_refill_mask: cap = %lld is below the %dx%d region's %lld bytes", cap, ctx->refill_last[0], ctx->refill_last[1], nb);
    CKC(hipSetDevice(ctx->device));
    CKC(hipStreamSynchronize(ctx->s_front));
    CKC(hipMemcpy(out, ctx->fds.d_gfr_mask, (size_t)nb, hipMemcpyDeviceToHost));
    *w = ctx->refill_last[0]; *h = ctx->refill_last[1];
    return PMV_OK;
}
int pmv_debug_refill_stats(pmv_ctx* ctx, long long* out4) {
    REQ(ctx && out4, PMV_ERR_INVALID, "pmv_debug_refill_stats: null argument");
    for (int i = 0; i < 4; i++) out4[i] = ctx->refill_stats[i].load();
    return PMV_OK;
}
// diagnostic: on != 0 sends the default arguments of pmv_detect_gftt_ex through the general kernels as well (no result changes)
int pmv_debug_gftt_general(pmv_ctx* ctx, int on) {
    REQ(ctx, PMV_ERR_INVALID, "null ctx");
    ctx->gftt_general = on != 0;
    return PMV_OK;
}

// cv::cornerSubPix on level 0 of the slot: point records and results in one mapped pinned block, ONE launch
int pmv_corner_subpix(pmv_ctx* ctx, int slot, float* xy, int n, const pmv_subpix_params* p, uint8_t* out_iters, uint8_t* out_flags) {
    REQ(ctx, PMV_ERR_INVALID, "pmv_corner_subpix: null argument");
    if (const int rc_ = subpix_check(ctx, "pmv_corner_subpix", true, slot, xy, n, p)) return rc_;
    if (n == 0) return PMV_OK;
    tl_prof = &ctx->prof;
    CKC(hipSetDevice(ctx->device));
    const size_t nt = (size_t)ctx->max_tracks;
    Carve spx_need, spx;
    subpix_block(spx_need, nt);
    CKC(ctx->h_subpix.ensure(spx_need.bytes() + 64));
    SubpixArgs A;
    CKC(subpix_table_ready(ctx, p, &A));
    spx = carve_of(ctx->h_subpix);
    const SubpixBlock S = subpix_block(spx, nt);   // at max_tracks points (the engine's round carves the same block at its round's points)
    SubpixRec* rec = S.rec.h;
    for (int i = 0; i < n; i++) rec[i] = SubpixRec{xy[2 * i], xy[2 * i + 1], slot, 0};
    CKC(launch_corner_subpix(ctx->s_front, ctx->d_slots, ctx->slot_layout[slot], S.rec.d, n, ctx->d_subpix_tab, A, S.xy.d, S.iters.d, S.flags.d));
    ctx->subpix_launches[0]++;
    CKC(hipStreamSynchronize(ctx->s_front));
    memcpy(xy, S.xy.h, (size_t)n * 8);
    if (out_iters) memcpy(out_iters, S.iters.h, (size_t)n);
    if (out_flags) memcpy(out_flags, S.flags.h, (size_t)n);
    return PMV_OK;
}
int pmv_debug_subpix_launches(pmv_ctx* ctx, long long* out3) {
    REQ(ctx && out3, PMV_ERR_INVALID, "pmv_debug_subpix_launches: null argument");
    for (int i = 0; i < 3; i++) out3[i] = ctx->subpix_launches[i].load();
    return PMV_OK;
}

int pmv_detect_shitomasi(pmv_ctx* ctx, int slot, const int* cells, int n_cells, int max_per_cell, double quality,
                         int* out_xy, double* out_score, int* out_count) {
    if (max_per_cell <= 0) {
        REQ(ctx, PMV_ERR_INVALID, "pmv_detect_shitomasi: bad argument");
        return shitomasi_nothing(ctx, cells, n_cells, out_count);
    }
    int rc = check_cells(ctx, slot, cells, n_cells, max_per_cell);
    if (rc) return rc;
    REQ(out_xy && out_score && out_count, PMV_ERR_INVALID, "pmv_detect_shitomasi: null output");
    tl_prof = &ctx->prof;
    CKC(hipSetDevice(ctx->device));
    const PyrLayout& L = ctx->slot_layout[slot];
    pack_cells(ctx->h_cells, cells, n_cells, slot);
    return detect_run(ctx, n_cells, max_per_cell, [&] {
        return launch_shitomasi(ctx->s_front, ctx->d_slots, L, ctx->d_cells, n_cells, max_per_cell, quality, ctx->d_eig, (unsigned long long*)ctx->d_cellmax, ctx->d_det_xy,
                                ctx->d_det_score, ctx->d_det_count, ctx->d_flags, ctx->d_spill);
    }, nullptr, out_xy, out_score, out_count);
}

// ---- per-kernel HIP-event timing -------------------------------------------------------------------------------------
int pmv_prof_enable(pmv_ctx* ctx, int on) {
    REQ(ctx, PMV_ERR_INVALID, "null ctx");
    CKC(hipSetDevice(ctx->device));
    CKC(hipStreamSynchronize(ctx->s_front));
    CKC(hipStreamSynchronize(ctx->s_back));
    if (on) for (int i = 0; i < K_COUNT; i++) { ctx->prof.used[i] = 0; ctx->prof.dropped[i] = 0; }
    ctx->prof.enabled = on != 0;
    ctx->prof.mask = ~0u;
    ctx->prof.chain_detail = false;
    return PMV_OK;
}
// restrict recording to the classes whose bit is set (events cost host time and a queue barrier each: the timed region of the
// bench records only the kernel its roofline object reports)
int pmv_prof_select(pmv_ctx* ctx, unsigned mask) {
    REQ(ctx, PMV_ERR_INVALID, "null ctx");
    ctx->prof.mask = mask;
    ctx->prof.chain_detail = (((mask >> K_BAM_EVAL0) & 0x3fu) != 0 || ((mask >> K_BAM_SOLVEBACK) & 3u) != 0) && mask != ~0u;
    return PMV_OK;
}
// diagnostic: phase timers of k_lk for track 0 (PMV_LK_STAMPS=1): [0] level entry, [1] I tile, [2] Scharr, [3] samples + A, [4] iterations
// (+ J tiles), [5] error pass; [8] iteration count
int pmv_debug_lk_stamps(pmv_ctx* ctx, unsigned long long* out16) {
    REQ(ctx && out16, PMV_ERR_INVALID, "null argument");
    memset(out16, 0, 16 * 8);
    if (!ctx->d_lk_stamps) return PMV_OK;
    CKC(hipSetDevice(ctx->device));
    CKC(hipStreamSynchronize(ctx->s_front));
    CKC(hipMemcpy(out16, ctx->d_lk_stamps, 16 * 8, hipMemcpyDeviceToHost));
    return PMV_OK;
}
// work counters of k_lk accumulated since the context was created or since the last reset: [0] LK iterations executed, [1] (track,
// level) pairs that entered the iteration loop, [2] tracks. bench.py turns them into SURVEY.md §8(d)'s OPS_lk = sum over tracks and
// levels of 1024 * (40 + 14 * iterations).
int pmv_lk_counters(pmv_ctx* ctx, unsigned long long* out3, int reset) {
    REQ(ctx && out3, PMV_ERR_INVALID, "null argument");
    CKC(hipSetDevice(ctx->device));
    CKC(hipStreamSynchronize(ctx->s_front));
    for (int i = 0; i < 3; i++) out3[i] = reset ? ctx->lk_work[i].exchange(0) : ctx->lk_work[i].load();
    return PMV_OK;
}
int pmv_prof_kernel_count(void) { return K_COUNT; }
const char* pmv_prof_kernel_name(int id) { return kernel_name(id); }
int pmv_prof_read(pmv_ctx* ctx, int id, int* launches, double* total_ms, double* max_ms) {
    REQ(ctx && id >= 0 && id < K_COUNT && launches && total_ms && max_ms, PMV_ERR_INVALID, "pmv_prof_read: bad argument");
    CKC(hipSetDevice(ctx->device));
    CKC(hipStreamSynchronize(ctx->s_front));
    CKC(hipStreamSynchronize(ctx->s_back));
    double tot = 0, mx = 0;
    const int n = ctx->prof.used[id] / 2;
    for (int i = 0; i < n; i++) {
        float ms = 0;
        CKC(hipEventElapsedTime(&ms, ctx->prof.ev[id][2 * i], ctx->prof.ev[id][2 * i + 1]));
        tot += ms;
        if (ms > mx) mx = ms;
    }
    *launches = n; *total_ms = tot; *max_ms = mx;
    return PMV_OK;
}

int pmv_debug_gftt_response(pmv_ctx* ctx, int slot, const int* cell, float* out) {
    int rc = check_cells(ctx, slot, cell, 1, 1);
    if (rc) return rc;
    REQ(out, PMV_ERR_INVALID, "null output");
    CKC(hipSetDevice(ctx->device));
    pack_cells(ctx->h_cells, cell, 1, slot);
    CKC(hipMemcpyAsync(ctx->d_cells, ctx->h_cells, (size_t)CELL_STRIDE * 4, hipMemcpyHostToDevice, ctx->s_front));
    CKC(launch_gftt_response(ctx->s_front, ctx->d_slots, ctx->slot_layout[slot], ctx->d_cells, 1, (float*)ctx->d_eig, (unsigned*)ctx->d_cellmax));
    CKC(hipStreamSynchronize(ctx->s_front));
    CKC(hipMemcpy(out, ctx->d_eig, (size_t)cell[2] * cell[3] * sizeof(float), hipMemcpyDeviceToHost));
    return PMV_OK;
}

int pmv_debug_gftt_response_ex(pmv_ctx* ctx, int slot, const int* cell, const pmv_gftt_params* p, float* out) {
    REQ(ctx, PMV_ERR_INVALID, "pmv_debug_gftt_response_ex: null argument");
    int dummy = 0;
    int rc = gftt_ex_check(ctx, "pmv_debug_gftt_response_ex", p, &dummy, &dummy);
    if (rc) return rc;
    rc = check_cells(ctx, slot, cell, 1, 1);
    if (rc) return rc;
    REQ(out, PMV_ERR_INVALID, "null output");
    CKC(hipSetDevice(ctx->device));
    pack_cells(ctx->h_cells, cell, 1, slot);
    CKC(hipMemcpyAsync(ctx->d_cells, ctx->h_cells, (size_t)CELL_STRIDE * 4, hipMemcpyHostToDevice, ctx->s_front));
    CKC(launch_gftt_response_ex(ctx->s_front, ctx->d_slots, ctx->slot_layout[slot], ctx->d_cells, 1, gftt_ext(p->block_size, p->use_harris, p->k), (float*)ctx->d_eig));
    CKC(hipStreamSynchronize(ctx->s_front));
    CKC(hipMemcpy(out, ctx->d_eig, (size_t)cell[2] * cell[3] * sizeof(float), hipMemcpyDeviceToHost));
    return PMV_OK;
}

int pmv_debug_shitomasi_response(pmv_ctx* ctx, int slot, const int* cell, double* out) {
    int rc = check_cells(ctx, slot, cell, 1, 1);
    if (rc) return rc;
    REQ(out, PMV_ERR_INVALID, "null output");
    int xy[2], cnt; double sc;
    rc = pmv_detect_shitomasi(ctx, slot, cell, 1, 1, 0.4, xy, &sc, &cnt);
    if (rc) return rc;
    CKC(hipMemcpy(out, ctx->d_eig, (size_t)cell[2] * cell[3] * sizeof(double), hipMemcpyDeviceToHost));
    return PMV_OK;
}

}  // extern "C"
