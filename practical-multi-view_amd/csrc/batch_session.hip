// Batch sessions (include/pmv_hip.h, pmv_batch_*): the batch engine for callers who keep their own orchestrator - the reference's real
// OdometryPipeline behind the INTEGRATION.md adapters, a live camera loop, a Python experiment. Their frames arrive one at a time and the
// length of a sequence is not known in advance, so nothing here is declared up front except the frame sizes (the geometry table).
//
//   * The plugin calls are the engine's request entry points (batch_engine.h), which run the argument checks of the single-sequence call of
//     the same name; a wrapper here adds the session, the seq index and the seq's lock: the combiners merge whatever requests have accumulated into one launch per kernel class, exactly as for the sequences
//     of pmv_pipeline_run_batch.
//   * Uploads are one more kernel class: the UPLOAD thread (one thread, one HIP stream, one completion word) takes whatever upload requests
//     accumulated while its previous round ran and issues the round as at most one gray and one BGR level-0 launch (pitched list forms,
//     frontend.hip) and one k_pyrdown_list launch per level, whatever the number of requests and the mix of sizes; then it stores
//     slot_layout / slot_state of the round's slots and wakes exactly the callers it served. A request returns only after its round's
//     completion word was seen, so the slot may be read by any session call from any thread without further ordering - the argument the
//     feeder's release rule uses (ingest_batch.hip).
//     A request of pmv_batch_frame_upload_clahe rides in the same round: behind the level-0 launches the round makes ONE k_clahe_lut and ONE
//     k_clahe_apply launch for all such requests (frontend_clahe.hip: a record per frame names its size and parameters) and ONE in-place
//     k_pad_level0_list launch over their slots, in front of the k_pyrdown launches. A round without such a request launches what it always did.
//     A request of pmv_batch_frame_upload_remap rides there too: behind the level-0 launches (which leave the gray image in the slot, colour
//     sources converted) the round makes ONE k_remap launch for all such requests, from the slots into the session's remap scratch
//     (frontend_remap.hip: a record per frame names its size, map and border value), and ONE k_pad_level0_list launch from that scratch back
//     into the slots; then the CLAHE stage, which also serves the remap requests that carry parameters, then the k_pyrdown launches.
//   * Sources. Pinned memory mapped at its host address and device memory of the context's device are read in place by the kernel, with the
//     caller's row stride as the entry's pitch. Anything else is copied by the CALLING thread, row by row and tight, into a block of the
//     session's pinned staging pool; the kernel reads it from there. The callers' threads launch nothing and wait for no stream: their one
//     runtime call is the address-range lookup that classifies the source (hipPointerGetAttributes, as batch_ingest_begin does).
#include "pmv_ctx.h"
#include "backend.h"
#include "batch_engine.h"
#include "ingest_batch.h"
#include "vo_pipeline.h"
#include "pmv_block.h"
#include "pmv_wait.h"
#include <sys/prctl.h>
#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstring>
#include <memory>
#include <thread>

namespace pmv {

namespace {

struct UpReq {
    int slot = 0, geom = 0, format = 0;
    const uint8_t* dsrc = nullptr;   // the address the kernel reads: the caller's own buffer (in place) or a staging block
    unsigned pitch = 0;
    bool in_place = false;           // dsrc is the caller's own buffer
    bool clahe = false;              // pmv_batch_frame_upload_clahe: level 0 is equalised with `cp` inside the round
    pmv_clahe_params cp = {0.0, 0, 0};
    const uint8_t* remap = nullptr;  // pmv_batch_frame_upload_remap: the packed map (device memory) level 0 is gathered through inside the round
    int border = 0;
    int rc = PMV_OK;
    char err[200] = "";
    std::atomic<int> done{0};        // completion word of the request: the owner sleeps on it (futex), as in batch_engine.hip
};

}  // namespace

struct BatchSession {
    static constexpr int ROUND = 1024;     // upload requests per round at most (the rest wait for the next one)
    pmv_ctx* ctx = nullptr;
    BatchEngine* eng = nullptr;
    int n_seq = 0;
    std::unique_ptr<std::mutex[]> seq_mu;  // one outstanding back-end call per seq: the four calls share the seq's pinned block
    // the upload class
    std::thread th;
    hipStream_t stream = nullptr;
    RoundSignal sig;                       // completion word of a round (pmv_wait.h)
    int linger_us = 0;                     // diagnostic (PMV_BATCH_LINGER_US, as the engine's combiners): a round with fewer than n_seq requests waits that long for more
    std::mutex mu;
    std::condition_variable cv;
    std::vector<UpReq*> pending;
    bool stop = false;
    // round tables in mapped pinned memory (round_tables; the last four are written only by a round with such requests)
    Buf<char> h_tab{MEM_MAPPED};
    // LUT blocks of a round's CLAHE requests (HBM): made by the first such round, grown to the largest round seen
    Buf<uint8_t> d_lut;
    // tight destination frames of a round's remap requests (HBM): made by the first such round, grown to the largest round seen
    Buf<uint8_t> d_rscratch;
    // staging pool: n_blk blocks of blk_bytes (the largest BGR frame of the declared sizes), pinned + mapped
    Buf<uint8_t> h_pool{MEM_MAPPED};
    size_t blk_bytes = 0;
    std::mutex pool_mu;
    std::condition_variable pool_cv;
    std::vector<int> free_blk;
    std::atomic<long long> rounds{0}, frames{0}, l0_launches{0}, pyr_launches{0};   // launches: counted where they are made
    // diagnostic (pmv_batch_upload_rounds): what each round held and launched, the first ROUND_LOG rounds of the session
    static constexpr size_t ROUND_LOG = 1 << 16;
    struct RoundRec { int by_levels[MAX_LEVELS]; int l0_launches, pyr_launches, in_place; };   // by_levels[i]: frames whose pyramid has i + 1 levels
    std::mutex log_mu;
    std::vector<RoundRec> log;
};

namespace {

void fail_round(std::vector<UpReq*>& batch, const char* what, hipError_t e) {
    for (UpReq* r : batch) { r->rc = PMV_ERR_HIP; snprintf(r->err, sizeof(r->err), "pmv_batch_frame_upload: %s: %s", what, hipGetErrorString(e)); }
}

// The seven tables of a round, ROUND entries each, host side and device side in step: level-0 entries of the gray and of the BGR requests, the
// list entries of all requests, the slots and records of the CLAHE requests, the slots (sources: their scratch frames) and records of the
// remap requests. A dry run gives the block's size.
struct RoundTables {
    Carved<PyrPitchEntry> gray, bgr;
    Carved<PyrListEntry> all, clahe_slots; Carved<ClaheRec> clahe;
    Carved<PyrListEntry> remap_slots; Carved<RemapRec> remap;
    size_t bytes;
};
RoundTables round_tables(Carve c) {
    constexpr size_t N = BatchSession::ROUND;
    RoundTables T{c.take<PyrPitchEntry>(N), c.take<PyrPitchEntry>(N), c.take<PyrListEntry>(N), c.take<PyrListEntry>(N), c.take<ClaheRec>(N),
                  c.take<PyrListEntry>(N), c.take<RemapRec>(N), 0};
    T.bytes = c.bytes();
    return T;
}

// one round: every request of `batch` (distinct slots, <= ROUND of them)
void upload_round(BatchSession* S, std::vector<UpReq*>& batch) {
    pmv_ctx* ctx = S->ctx;
    const RoundTables T = round_tables(Carve(S->h_tab.p, S->h_tab.dev, S->h_tab.cap));
    PyrPitchEntry* tg = T.gray.h; PyrPitchEntry* tc = T.bgr.h; PyrListEntry* ta = T.all.h;
    PyrListEntry* te = T.clahe_slots.h; ClaheRec* tr = T.clahe.h;   // the slots of the round's CLAHE requests (in-place entries)
    PyrListEntry* tm = T.remap_slots.h; RemapRec* tq = T.remap.h;   // the slots of the round's remap requests (sources: their scratch frames)
    const PyrPitchEntry* dg = T.gray.d; const PyrPitchEntry* dc = T.bgr.d; const PyrListEntry* da = T.all.d;
    const PyrListEntry* de = T.clahe_slots.d; const ClaheRec* dr = T.clahe.d;
    const PyrListEntry* dm = T.remap_slots.d; const RemapRec* dq = T.remap.d;
    // grid and LDS of a launch from the largest geometry among ITS entries, level by level
    PyrLayout Lg{}, Lc{}, La{}, Le{}, Lm{};
    auto widen = [](PyrLayout& M, const PyrLayout& L) {
        M.n_levels = std::max(M.n_levels, L.n_levels);
        for (int l = 0; l < L.n_levels; l++) { M.w[l] = std::max(M.w[l], L.w[l]); M.h[l] = std::max(M.h[l], L.h[l]); }
    };
    int ng = 0, nc = 0, na = 0, ne = 0, max_tiles = 0, nm = 0;
    size_t lut_bytes = 0, rscratch_bytes = 0;
    for (UpReq* r : batch) {
        const PyrLayout& L = ctx->geom[(size_t)r->geom];
        PyrPitchEntry& e = r->format == PMV_FRAMES_BGR ? tc[nc++] : tg[ng++];
        e.src = r->dsrc; e.pitch = r->pitch; e.slot = r->slot; e.geom = r->geom; e.reserved = 0;
        widen(r->format == PMV_FRAMES_BGR ? Lc : Lg, L);
        widen(La, L);
        ta[na].src = nullptr; ta[na].slot = r->slot; ta[na].geom = r->geom;
        na++;
        if (r->clahe) {
            tr[ne] = clahe_record(r->slot, r->geom, L.w[0], L.h[0], r->cp.clip_limit, r->cp.tiles_x, r->cp.tiles_y);
            tr[ne].lut_off = (unsigned)lut_bytes;
            lut_bytes += (size_t)(r->cp.tiles_x * r->cp.tiles_y) * 256;
            max_tiles = std::max(max_tiles, r->cp.tiles_x * r->cp.tiles_y);
            te[ne].src = nullptr; te[ne].slot = r->slot; te[ne].geom = r->geom;
            widen(Le, L);
            ne++;
        }
        if (r->remap) {
            tq[nm].map = (const uint32_t*)r->remap; tq[nm].dst_off = (unsigned long long)rscratch_bytes;
            tq[nm].slot = r->slot; tq[nm].geom = r->geom; tq[nm].border = r->border; tq[nm].reserved = 0;
            tm[nm].src = nullptr; tm[nm].slot = r->slot; tm[nm].geom = r->geom;   // (src: below, once the scratch is there)
            rscratch_bytes += remap_frame_bytes(L.w[0], L.h[0]);
            widen(Lm, L);
            nm++;
        }
    }
    // A round that fails after its first launch must not hand the sources back while a kernel still reads them: wait for the stream first.
    auto fail = [&](const char* what, hipError_t err) { (void)hipStreamSynchronize(S->stream); fail_round(batch, what, err); };
    BatchSession::RoundRec rec{};
    hipError_t e = hipSuccess;
    if (ng) {
        if ((e = launch_pad_level0_pitched(S->stream, ctx->d_slots, ctx->d_geom, Lg, dg, ng)) != hipSuccess) { fail("k_pad_level0_pitched", e); return; }
        rec.l0_launches++;
    }
    if (nc) {
        if ((e = launch_pad_level0_bgr_pitched(S->stream, ctx->d_slots, ctx->d_geom, Lc, dc, nc)) != hipSuccess) { fail("k_pad_level0_bgr_pitched", e); return; }
        rec.l0_launches++;
    }
    if (nm) {
        // level 0 of the round's remap requests is gathered from where the launches above left it into the scratch, then written back with its
        // REFLECT_101 frame by the list form, whose sources are the scratch frames
        // (growing frees the old block: the stream is idle between rounds, the previous round was waited for)
        if ((e = S->d_rscratch.ensure(rscratch_bytes)) != hipSuccess) { fail("the remap scratch", e); return; }
        for (int i = 0; i < nm; i++) tm[i].src = S->d_rscratch + tq[i].dst_off;
        if ((e = launch_remap(S->stream, ctx->d_slots, ctx->d_geom, dq, nm, Lm.w[0], Lm.h[0], S->d_rscratch)) != hipSuccess) { fail("k_remap", e); return; }
        ctx->remap_launches[2]++;
        if ((e = launch_pad_level0_list(S->stream, ctx->d_slots, ctx->d_geom, Lm, dm, nm)) != hipSuccess) { fail("k_pad_level0_list", e); return; }
        rec.l0_launches++;
    }
    if (ne) {
        // level 0 of the round's CLAHE requests is equalised where the launches above left it, then its REFLECT_101 frame is rebuilt in place
        if ((e = S->d_lut.ensure(lut_bytes)) != hipSuccess) { fail("the LUT scratch", e); return; }   // (as above)
        if ((e = launch_clahe(S->stream, ctx->d_slots, ctx->d_geom, dr, ne, max_tiles, Le.w[0], Le.h[0], S->d_lut)) != hipSuccess) { fail("k_clahe_lut / k_clahe_apply", e); return; }
        ctx->clahe_launches[2]++;
        if ((e = launch_pad_level0_list(S->stream, ctx->d_slots, ctx->d_geom, Le, de, ne)) != hipSuccess) { fail("k_pad_level0_list", e); return; }
        rec.l0_launches++;
    }
    for (int l = 1; l < La.n_levels; l++) {
        if ((e = launch_pyrdown_list(S->stream, ctx->d_slots, ctx->d_geom, La, l, da, na)) != hipSuccess) { fail("k_pyrdown", e); return; }
        rec.pyr_launches++;
    }
    if ((e = S->sig.signal_and_wait<false>(S->stream, true)) != hipSuccess) { fail("waiting for the round", e); return; }
    for (UpReq* r : batch) {
        ctx->slot_layout[(size_t)r->slot] = ctx->geom[(size_t)r->geom];
        ctx->slot_state[(size_t)r->slot] = SLOT_BUILT;
        rec.by_levels[ctx->geom[(size_t)r->geom].n_levels - 1]++;
        rec.in_place += r->in_place ? 1 : 0;
    }
    if (ne) ctx->clahe_launches[1]++;
    if (nm) ctx->remap_launches[1]++;
    S->rounds++; S->frames += na; S->l0_launches += rec.l0_launches; S->pyr_launches += rec.pyr_launches;
    std::lock_guard<std::mutex> lk(S->log_mu);
    if (S->log.size() < BatchSession::ROUND_LOG) S->log.push_back(rec);
}

void upload_loop(BatchSession* S) {
    (void)hipSetDevice(S->ctx->device);
    tl_prof = &S->ctx->prof;
    (void)prctl(PR_SET_TIMERSLACK, 1000UL, 0, 0, 0);   // 1 us: the timed sleeps of RoundSignal
    std::vector<UpReq*> carry;   // requests put off by a round: a second upload into a slot of the round, or more than ROUND requests
    for (;;) {
        std::vector<UpReq*> got;
        {
            std::unique_lock<std::mutex> lk(S->mu);
            if (carry.empty()) S->cv.wait(lk, [&] { return !S->pending.empty() || S->stop; });
            if (S->pending.empty() && carry.empty() && S->stop) return;
            if (S->linger_us > 0 && (int)S->pending.size() < S->n_seq && !S->stop) {
                lk.unlock();
                std::this_thread::sleep_for(std::chrono::microseconds(S->linger_us));
                lk.lock();
            }
            got.swap(S->pending);
        }
        std::vector<UpReq*> batch, later;
        carry.insert(carry.end(), got.begin(), got.end());
        for (UpReq* r : carry) {
            bool dup = (int)batch.size() >= BatchSession::ROUND;
            for (size_t i = 0; i < batch.size() && !dup; i++) dup = batch[i]->slot == r->slot;
            (dup ? later : batch).push_back(r);
        }
        carry.swap(later);
        upload_round(S, batch);
        for (UpReq* r : batch) {
            std::atomic<int>* w = &r->done;   // (after the store the owner may return and the request, which lives on its stack, is gone)
            w->store(1, std::memory_order_release);
            futex_wake_one(w);
        }
    }
}

void session_free(BatchSession* S) {
    if (!S) return;
    { std::lock_guard<std::mutex> lk(S->mu); S->stop = true; }
    S->cv.notify_all();
    if (S->th.joinable()) S->th.join();
    if (S->stream) { (void)hipStreamSynchronize(S->stream); (void)hipStreamDestroy(S->stream); }
    delete S;
}

}  // namespace

void batch_session_destroy(pmv_ctx* ctx) {
    session_free(ctx->session);
    ctx->session = nullptr;
    ctx->session_state.store(0);
}

}  // namespace pmv

using namespace pmv;

#define CKC(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { set_err(ctx, "%s: %s", #x, hipGetErrorString(e_)); return PMV_ERR_HIP; } } while (0)
#define REQ(cond, code, ...) do { if (!(cond)) { set_err(ctx, __VA_ARGS__); return code; } } while (0)

namespace {

// A session call in flight: counted so that pmv_batch_close can refuse while one is outstanding. Either the call sees the session closing
// (and fails) or pmv_batch_close sees the call (and fails): both sides use sequentially consistent atomics.
struct InCall {
    pmv_ctx* ctx; bool ok;
    InCall(pmv_ctx* c, const char* who) : ctx(c), ok(false) {
        if (!ctx) { set_err(nullptr, "%s: null ctx", who); return; }
        ctx->session_calls.fetch_add(1);
        int st;
        while ((st = ctx->session_state.load()) == 2) std::this_thread::yield();   // a pmv_batch_close is deciding: it sees this call, or it wins
        ok = st == 1;
        if (!ok) { ctx->session_calls.fetch_sub(1); set_err(ctx, "%s: no batch session is open on this context (pmv_batch_open first)", who); }
    }
    ~InCall() { if (ok) ctx->session_calls.fetch_sub(1); }
};
#define SESSION(who) InCall in_(ctx, who); if (!in_.ok) return PMV_ERR_INVALID; BatchSession* S = ctx->session; (void)S

int seq_check(pmv_ctx* ctx, BatchSession* S, const char* who, int seq) {
    REQ(seq >= 0 && seq < S->n_seq, PMV_ERR_INVALID, "%s: seq %d outside 0..%d (n_seq of pmv_batch_open)", who, seq, S->n_seq - 1);
    return PMV_OK;
}

}  // namespace

extern "C" {

int pmv_batch_open(pmv_ctx* ctx, int n_seq, const int* sizes_wh, int n_sizes) {
    REQ(ctx && sizes_wh, PMV_ERR_INVALID, "pmv_batch_open: null argument");
    REQ(n_seq >= 1 && n_seq <= 256, PMV_ERR_INVALID, "pmv_batch_open: n_seq = %d (1..256)", n_seq);
    REQ(n_sizes >= 1 && n_sizes <= pmv_ctx::MAX_GEOM, PMV_ERR_INVALID, "pmv_batch_open: n_sizes = %d (1..%d)", n_sizes, pmv_ctx::MAX_GEOM);
    std::vector<int> ws((size_t)n_sizes), hs((size_t)n_sizes);
    size_t max_fb = 0;
    for (int i = 0; i < n_sizes; i++) {
        const int w = sizes_wh[2 * i], h = sizes_wh[2 * i + 1];
        REQ(w >= 40 && h >= 40 && w <= ctx->max_w && h <= ctx->max_h, PMV_ERR_CAPACITY, "pmv_batch_open: size %d: frame %dx%d outside capacity %dx%d", i, w, h, ctx->max_w, ctx->max_h);
        for (int j = 0; j < i; j++) REQ(ws[(size_t)j] != w || hs[(size_t)j] != h, PMV_ERR_INVALID, "pmv_batch_open: size %dx%d is named twice (entries %d and %d)", w, h, j, i);
        ws[(size_t)i] = w; hs[(size_t)i] = h;
        max_fb = std::max(max_fb, (size_t)3 * w * h);
    }
    // the engine and the geometry table have one owner at a time: a session, or a batched run
    std::lock_guard<std::mutex> own(ctx->owner_mu);
    REQ(ctx->session_state.load() == 0, PMV_ERR_INVALID, "pmv_batch_open: a batch session is already open on this context (pmv_batch_close first)");
    REQ(ctx->batch_open.load() == 0 && !batch_ingest_active(ctx->bingest), PMV_ERR_INVALID, "pmv_batch_open: a batched run (pmv_pipeline_run_batch / _streamed) is open on this context");
    CKC(hipSetDevice(ctx->device));
    BatchEngine* eng = nullptr;
    int rc = batch_engine_get(ctx, n_seq, &eng);
    if (rc != PMV_OK) return rc;
    if ((rc = pmv_sync(ctx)) != PMV_OK) return rc;
    if ((rc = geom_table_set(ctx, ws.data(), hs.data(), n_sizes)) != PMV_OK) return rc;
    BatchSession* S = new BatchSession();
    S->ctx = ctx; S->eng = eng; S->n_seq = n_seq;
    S->seq_mu.reset(new std::mutex[(size_t)n_seq]);
    if (const char* e = getenv("PMV_BATCH_LINGER_US")) S->linger_us = atoi(e);
    hipError_t e = hipSuccess;
    const size_t tab_bytes = round_tables(Carve()).bytes;
    S->blk_bytes = (max_fb + 255) & ~(size_t)255;
    // two blocks per sequence (frames k - 1 and k on their way), within 4 .. 64 blocks and 256 MB; an uploader without a block waits for one
    const int n_blk = (int)std::max<size_t>(2, std::min<size_t>({(size_t)64, std::max<size_t>(4, 2 * (size_t)n_seq), ((size_t)256 << 20) / S->blk_bytes}));
    if ((e = hipStreamCreateWithFlags(&S->stream, hipStreamNonBlocking)) == hipSuccess &&
        (e = S->sig.init()) == hipSuccess && (e = S->h_tab.ensure(tab_bytes)) == hipSuccess)
        e = S->h_pool.ensure((size_t)n_blk * S->blk_bytes);
    if (e != hipSuccess) { set_err(ctx, "pmv_batch_open: %s", hipGetErrorString(e)); session_free(S); return PMV_ERR_HIP; }
    for (int i = n_blk - 1; i >= 0; i--) S->free_blk.push_back(i);
    S->th = std::thread(upload_loop, S);
    ctx->session = S;
    ctx->session_state.store(1);
    return PMV_OK;
}

int pmv_batch_close(pmv_ctx* ctx) {
    REQ(ctx, PMV_ERR_INVALID, "pmv_batch_close: null ctx");
    std::lock_guard<std::mutex> own(ctx->owner_mu);
    REQ(ctx->session_state.load() == 1, PMV_ERR_INVALID, "pmv_batch_close: no batch session is open on this context");
    ctx->session_state.store(2);   // closing: new session calls are refused from here on
    const int n = ctx->session_calls.load();
    if (n != 0) {
        ctx->session_state.store(1);
        set_err(ctx, "pmv_batch_close: %d session call%s still outstanding", n, n == 1 ? " is" : "s are");
        return PMV_ERR_INVALID;
    }
    (void)hipSetDevice(ctx->device);
    batch_session_destroy(ctx);
    return PMV_OK;
}

int pmv_batch_upload_stats(pmv_ctx* ctx, long long* out4) {
    SESSION("pmv_batch_upload_stats");
    REQ(out4, PMV_ERR_INVALID, "pmv_batch_upload_stats: null argument");
    out4[0] = S->rounds.load(); out4[1] = S->frames.load(); out4[2] = S->l0_launches.load(); out4[3] = S->pyr_launches.load();
    return PMV_OK;
}

int pmv_batch_upload_rounds(pmv_ctx* ctx, int* out8, int capacity) {
    SESSION("pmv_batch_upload_rounds");
    REQ(capacity >= 0 && (out8 || capacity == 0), PMV_ERR_INVALID, "pmv_batch_upload_rounds: null argument");
    std::lock_guard<std::mutex> lk(S->log_mu);
    static_assert(sizeof(BatchSession::RoundRec) == 8 * sizeof(int) && MAX_LEVELS == 5, "a round's record is the 8 ints the header names");
    const size_t n = std::min(S->log.size(), (size_t)capacity);
    if (n) memcpy(out8, S->log.data(), n * sizeof(BatchSession::RoundRec));
    return (int)S->log.size();
}

// pmv_batch_frame_upload and, with cp, pmv_batch_frame_upload_clahe, with map, pmv_batch_frame_upload_remap (cp, map, border: checked by the
// caller): one request of the upload class
static int session_upload(pmv_ctx* ctx, int slot, const uint8_t* pixels, int w, int h, int stride, int format, const pmv_clahe_params* cp,
                          const pmv_ctx::RemapMap* map = nullptr, int map_id = 0, int border = 0) {
    SESSION("pmv_batch_frame_upload");
    REQ(pixels, PMV_ERR_INVALID, "pmv_batch_frame_upload: null argument");
    REQ(slot >= 0 && slot < ctx->n_slots, PMV_ERR_CAPACITY, "pmv_batch_frame_upload: slot %d out of range", slot);
    REQ(format == PMV_FRAMES_GRAY || format == PMV_FRAMES_BGR, PMV_ERR_INVALID, "pmv_batch_frame_upload: unknown format %d (PMV_FRAMES_GRAY = 0, PMV_FRAMES_BGR = 1)", format);
    UpReq r;
    r.slot = slot; r.format = format;
    if (cp) { r.clahe = true; r.cp = *cp; }
    if (map) {
        REQ(w == map->w && h == map->h, PMV_ERR_INVALID, "pmv_batch_frame_upload_remap: slot %d: a %dx%d frame, map %d is %dx%d", slot, w, h, map_id, map->w, map->h);
        r.remap = map->d; r.border = border;
    }
    r.geom = ctx->geom_index(w, h);
    REQ(r.geom >= 0, PMV_ERR_INVALID, "pmv_batch_frame_upload: a %dx%d frame: that size was not declared at pmv_batch_open", w, h);
    const size_t row = (size_t)w * (format == PMV_FRAMES_BGR ? 3 : 1);
    REQ(stride >= 0 && (size_t)stride >= row, PMV_ERR_CAPACITY, "pmv_batch_frame_upload: stride %d below the %zu bytes of a %s row of %d pixels", stride, row,
        format == PMV_FRAMES_BGR ? "BGR" : "gray", w);
    // A kernel is never handed a pageable address. Device memory of this device and pinned memory mapped at its host address are read in place;
    // anything else - pageable, registered under another device address, managed - goes through the staging pool.
    bool in_place = false;
    {
        hipPointerAttribute_t attr;
        const hipError_t e = hipPointerGetAttributes(&attr, pixels);
        (void)hipGetLastError();   // (a malloc'ed pointer may make the lookup fail: that is the "pageable" answer)
        if (e == hipSuccess && attr.type == hipMemoryTypeDevice) {
            REQ(attr.device == ctx->device, PMV_ERR_INVALID, "pmv_batch_frame_upload: the frame is in memory of device %d, the context is on device %d", attr.device, ctx->device);
            void* base = nullptr; size_t size = 0;   // the whole frame lies inside its allocation
            if (hipMemGetAddressRange((hipDeviceptr_t*)&base, &size, (hipDeviceptr_t)pixels) == hipSuccess)
                REQ((const uint8_t*)pixels + (size_t)(h - 1) * (size_t)stride + row <= (const uint8_t*)base + size, PMV_ERR_INVALID,
                    "pmv_batch_frame_upload: a %dx%d frame with stride %d reaches past the end of its device allocation", w, h, stride);
            (void)hipGetLastError();
            in_place = true;
        } else if (e == hipSuccess && attr.type == hipMemoryTypeHost && attr.hostPointer == (const void*)pixels && attr.devicePointer == attr.hostPointer)
            in_place = true;
    }
    int blk = -1;
    r.in_place = in_place;
    if (in_place) { r.dsrc = pixels; r.pitch = (unsigned)stride; }
    else {
        {
            std::unique_lock<std::mutex> lk(S->pool_mu);
            S->pool_cv.wait(lk, [&] { return !S->free_blk.empty(); });
            blk = S->free_blk.back();
            S->free_blk.pop_back();
        }
        uint8_t* dst = S->h_pool + (size_t)blk * S->blk_bytes;   // (row * h <= blk_bytes: the size is a declared one)
        if ((size_t)stride == row) memcpy(dst, pixels, row * (size_t)h);
        else for (int y = 0; y < h; y++) memcpy(dst + (size_t)y * row, pixels + (size_t)y * (size_t)stride, row);
        r.dsrc = S->h_pool.dm() + (size_t)blk * S->blk_bytes;
        r.pitch = (unsigned)row;
    }
    {
        std::lock_guard<std::mutex> lk(S->mu);
        S->pending.push_back(&r);
    }
    S->cv.notify_one();
    futex_wait_while(&r.done, 0);
    if (blk >= 0) {
        { std::lock_guard<std::mutex> lk(S->pool_mu); S->free_blk.push_back(blk); }
        S->pool_cv.notify_one();
    }
    if (r.rc != PMV_OK) set_err(ctx, "%s", r.err);
    return r.rc;
}

int pmv_batch_frame_upload(pmv_ctx* ctx, int slot, const uint8_t* pixels, int w, int h, int stride, int format) {
    return session_upload(ctx, slot, pixels, w, h, stride, format, nullptr);
}

int pmv_batch_frame_upload_clahe(pmv_ctx* ctx, int slot, const uint8_t* pixels, int w, int h, int stride, int format, const pmv_clahe_params* p) {
    if (!ctx) { set_err(nullptr, "pmv_batch_frame_upload_clahe: null ctx"); return PMV_ERR_INVALID; }
    if (const int rc = clahe_check(ctx, "pmv_batch_frame_upload_clahe", p)) return rc;
    return session_upload(ctx, slot, pixels, w, h, stride, format, p);
}

int pmv_batch_frame_upload_remap(pmv_ctx* ctx, int slot, const uint8_t* pixels, int w, int h, int stride, int format, int map_id, int border_value,
                                 const pmv_clahe_params* clahe_or_null) {
    if (!ctx) { set_err(nullptr, "pmv_batch_frame_upload_remap: null ctx"); return PMV_ERR_INVALID; }
    pmv_ctx::RemapMap map;
    if (const int rc = remap_check(ctx, "pmv_batch_frame_upload_remap", map_id, border_value, &map)) return rc;
    if (clahe_or_null)
        if (const int rc = clahe_check(ctx, "pmv_batch_frame_upload_remap", clahe_or_null)) return rc;
    return session_upload(ctx, slot, pixels, w, h, stride, format, clahe_or_null, &map, map_id, border_value);
}

// ---- front-end calls: a request of the class's combiner; the engine entry runs the checks of the single call (batch_engine.h) ----------
int pmv_batch_lk_track(pmv_ctx* ctx, int prev_slot, int next_slot, const float* prev_xy, int n, float* out_xy, uint8_t* out_status, float* out_err) {
    SESSION("pmv_batch_lk_track");
    return engine_lk(S->eng, prev_slot, next_slot, prev_xy, n, out_xy, out_status, out_err);
}

int pmv_batch_lk_track_ex(pmv_ctx* ctx, int prev_slot, int next_slot, const float* prev_xy, int n, float* next_xy, int flags, uint8_t* out_status, float* out_err) {
    SESSION("pmv_batch_lk_track_ex");
    return engine_lk_ex(S->eng, "pmv_batch_lk_track_ex", prev_slot, next_slot, prev_xy, n, next_xy, flags, out_status, out_err, false, nullptr, nullptr, nullptr);
}
int pmv_batch_lk_track_fb(pmv_ctx* ctx, int prev_slot, int next_slot, const float* prev_xy, int n, float* next_xy, int flags, uint8_t* out_status, float* out_err,
                          float* back_xy, uint8_t* back_status, float* back_err) {
    SESSION("pmv_batch_lk_track_fb");
    return engine_lk_ex(S->eng, "pmv_batch_lk_track_fb", prev_slot, next_slot, prev_xy, n, next_xy, flags, out_status, out_err, true, back_xy, back_status, back_err);
}

int pmv_batch_knn_match(pmv_ctx* ctx, int src_slot, int cmp_slot, const int* src_xy, int n, const int* cmp_xy, int m, int n_neighbours, int window,
                        int* out_best, float* out_err) {
    SESSION("pmv_batch_knn_match");
    return engine_knn(S->eng, src_slot, cmp_slot, src_xy, n, cmp_xy, m, n_neighbours, window, out_best, out_err);
}

int pmv_batch_detect_gftt(pmv_ctx* ctx, int slot, const int* cells, int n_cells, int max_per_cell, double quality, double min_dist, int* out_xy, int* out_count) {
    SESSION("pmv_batch_detect_gftt");
    return engine_detect(S->eng, Q_GFTT, slot, cells, n_cells, max_per_cell, quality, min_dist, out_xy, nullptr, out_count);
}

int pmv_batch_detect_gftt_ex(pmv_ctx* ctx, int slot, const int* cells, int n_cells, int max_per_cell, const pmv_gftt_params* p, const uint8_t* mask,
                             int mask_stride, int* out_xy, int* out_count) {
    SESSION("pmv_batch_detect_gftt_ex");
    return engine_detect_gftt_ex(S->eng, "pmv_batch_detect_gftt_ex", slot, cells, n_cells, max_per_cell, p, mask, mask_stride, out_xy, out_count);
}

int pmv_batch_detect_gftt_frame(pmv_ctx* ctx, int slot, const int* roi4_or_null, int max_corners, const pmv_gftt_params* p, const uint8_t* mask, int mask_stride,
                                int* out_xy, int out_cap, int* out_count) {
    SESSION("pmv_batch_detect_gftt_frame");
    return engine_detect_gftt_frame(S->eng, "pmv_batch_detect_gftt_frame", slot, roi4_or_null, max_corners, p, mask, mask_stride, out_xy, out_cap, out_count);
}

int pmv_batch_detect_gftt_refill(pmv_ctx* ctx, int slot, const int* roi4_or_null, int max_corners, const pmv_gftt_params* p, const float* track_xy,
                                 const int* track_prio_or_null, int n_tracks, int radius, const uint8_t* base_mask_or_null, int base_stride, uint8_t* out_keep,
                                 int* out_xy, int out_cap, int* out_count) {
    SESSION("pmv_batch_detect_gftt_refill");
    return engine_detect_gftt_refill(S->eng, "pmv_batch_detect_gftt_refill", slot, roi4_or_null, max_corners, p, track_xy, track_prio_or_null, n_tracks, radius,
                                     base_mask_or_null, base_stride, out_keep, out_xy, out_cap, out_count);
}

int pmv_batch_corner_subpix(pmv_ctx* ctx, int slot, float* xy, int n, const pmv_subpix_params* p, uint8_t* out_iters, uint8_t* out_flags) {
    SESSION("pmv_batch_corner_subpix");
    return engine_corner_subpix(S->eng, "pmv_batch_corner_subpix", slot, xy, n, p, out_iters, out_flags);
}

int pmv_batch_detect_shitomasi(pmv_ctx* ctx, int slot, const int* cells, int n_cells, int max_per_cell, double quality, int* out_xy, double* out_score,
                               int* out_count) {
    SESSION("pmv_batch_detect_shitomasi");
    return engine_detect(S->eng, Q_SHITOMASI, slot, cells, n_cells, max_per_cell, quality, 0.0, out_xy, out_score, out_count);
}

int pmv_batch_detect_fast(pmv_ctx* ctx, int slot, const int* cells, int n_cells, int max_per_cell, int threshold, int nonmax, int* out_xy, float* out_response,
                          int* out_count) {
    SESSION("pmv_batch_detect_fast");
    return engine_detect_fast(S->eng, slot, cells, n_cells, max_per_cell, threshold, nonmax, out_xy, out_response, out_count);
}

// ---- back-end calls: seq selects the workspace set; its four calls share one pinned block, so they take turns ---------------------------
int pmv_batch_pnp_ransac(pmv_ctx* ctx, int seq, const float* obj_xyz, const float* img_xy, int m, const double* K, double* rvec, double* tvec, int iterations,
                         float reproj_err, double confidence, int* out_inliers, int* out_n_inliers) {
    SESSION("pmv_batch_pnp_ransac");
    if (const int rc = seq_check(ctx, S, "pmv_batch_pnp_ransac", seq)) return rc;
    std::lock_guard<std::mutex> lk(S->seq_mu[(size_t)seq]);
    return engine_pnp(S->eng, seq, obj_xyz, img_xy, m, K, rvec, tvec, iterations, reproj_err, confidence, out_inliers, out_n_inliers);
}

int pmv_batch_ba_solve(pmv_ctx* ctx, int seq, double* cams, int nc, double* pts, int np, const double* obs_xy, const int* cam_idx, const int* pt_idx, int n_obs,
                       const double* K, double huber_delta, int max_iterations, pmv_ba_summary* summary) {
    SESSION("pmv_batch_ba_solve");
    if (const int rc = seq_check(ctx, S, "pmv_batch_ba_solve", seq)) return rc;
    std::lock_guard<std::mutex> lk(S->seq_mu[(size_t)seq]);
    return engine_ba(S->eng, seq, cams, nc, pts, np, obs_xy, cam_idx, pt_idx, n_obs, K, huber_delta, max_iterations, summary);
}

int pmv_batch_triangulate_candidates(pmv_ctx* ctx, int seq, const double* q1, const double* q2, int n, const double* P1x4, const uint8_t* mask_in, double* out_Q,
                                     uint8_t* out_mask, int* out_good) {
    SESSION("pmv_batch_triangulate_candidates");
    if (const int rc = seq_check(ctx, S, "pmv_batch_triangulate_candidates", seq)) return rc;
    std::lock_guard<std::mutex> lk(S->seq_mu[(size_t)seq]);
    return engine_dlt(S->eng, seq, q1, q2, n, P1x4, mask_in, out_Q, out_mask, out_good);
}

// N-view triangulation of a seq: one row of workgroups of the round's k_tri_tracks_batch launch (engine_tri_tracks)
int pmv_batch_triangulate_tracks(pmv_ctx* ctx, int seq, const double* P3x4, int nc, const double* obs_xy, const int* cam_idx, const int* pt_idx, int n_obs,
                                 int np, const pmv_tri_params* p_or_null, double* out_xyz, uint8_t* out_status, double* out_err_or_null, int* out_good) {
    SESSION("pmv_batch_triangulate_tracks");
    if (const int rc = seq_check(ctx, S, "pmv_batch_triangulate_tracks", seq)) return rc;
    std::lock_guard<std::mutex> lk(S->seq_mu[(size_t)seq]);
    return engine_tri_tracks(S->eng, seq, P3x4, nc, obs_xy, cam_idx, pt_idx, n_obs, np, p_or_null, out_xyz, out_status, out_err_or_null, out_good);
}

int pmv_batch_fivepoint_hypotheses(pmv_ctx* ctx, int seq, const double* q1, const double* q2, int n, const int* samples, int n_hyp, float thr, double* models,
                                   int* n_models, int* counts) {
    SESSION("pmv_batch_fivepoint_hypotheses");
    if (const int rc = seq_check(ctx, S, "pmv_batch_fivepoint_hypotheses", seq)) return rc;
    std::lock_guard<std::mutex> lk(S->seq_mu[(size_t)seq]);
    return engine_fivepoint(S->eng, seq, q1, q2, n, samples, n_hyp, thr, models, n_models, counts);
}

// The whole two-view step of a seq: findEssentialMat as one workgroup of the round's k_essential_ransac launch (the call returns when ITS
// request is done, not when the round is), recoverPose as the host half of the single call around a request of the DLT combiner.
int pmv_batch_find_essential_mat(pmv_ctx* ctx, int seq, const double* p1_xy, const double* p2_xy, int n, const double* K, double prob, double threshold,
                                 double* E9, uint8_t* mask, int* out_found, int* out_samples_drawn) {
    SESSION("pmv_batch_find_essential_mat");
    if (const int rc = seq_check(ctx, S, "pmv_batch_find_essential_mat", seq)) return rc;
    std::lock_guard<std::mutex> lk(S->seq_mu[(size_t)seq]);
    return engine_essential(S->eng, seq, p1_xy, p2_xy, n, K, prob, threshold, E9, mask, out_found, out_samples_drawn);
}

// rejectWithF of a seq's KLT loop: findFundamentalMat as one workgroup of the round's k_fundamental_ransac launch (engine_fundamental)
int pmv_batch_find_fundamental_mat(pmv_ctx* ctx, int seq, const float* p1_xy, const float* p2_xy, int n, double threshold, double confidence, double* F9,
                                   uint8_t* mask, int* out_found, int* out_samples_drawn) {
    SESSION("pmv_batch_find_fundamental_mat");
    if (const int rc = seq_check(ctx, S, "pmv_batch_find_fundamental_mat", seq)) return rc;
    std::lock_guard<std::mutex> lk(S->seq_mu[(size_t)seq]);
    return engine_fundamental(S->eng, seq, p1_xy, p2_xy, n, threshold, confidence, F9, mask, out_found, out_samples_drawn);
}

// findHomography of a seq: one workgroup of the round's k_homography_ransac launch (engine_homography)
int pmv_batch_find_homography(pmv_ctx* ctx, int seq, const float* p1_xy, const float* p2_xy, int n, double threshold, double confidence, int max_iters, double* H9,
                              uint8_t* mask, int* out_found, int* out_samples_drawn) {
    SESSION("pmv_batch_find_homography");
    if (const int rc = seq_check(ctx, S, "pmv_batch_find_homography", seq)) return rc;
    std::lock_guard<std::mutex> lk(S->seq_mu[(size_t)seq]);
    return engine_homography(S->eng, seq, p1_xy, p2_xy, n, threshold, confidence, max_iters, H9, mask, out_found, out_samples_drawn);
}

int pmv_batch_recover_pose(pmv_ctx* ctx, int seq, const double* E9, const double* p1_xy, const double* p2_xy, int n, const double* K, double* R9, double* t3,
                           uint8_t* mask, double* tri4n, int* out_good) {
    SESSION("pmv_batch_recover_pose");
    if (const int rc = seq_check(ctx, S, "pmv_batch_recover_pose", seq)) return rc;
    if (const int rc = recover_pose_check(ctx, "pmv_recover_pose", E9, p1_xy, p2_xy, n, K, R9, t3, mask, tri4n, out_good)) return rc;
    std::lock_guard<std::mutex> lk(S->seq_mu[(size_t)seq]);
    struct Tri : vo::FivePointTri {
        BatchEngine* eng; int seq; int rc = PMV_OK;
        void dlt_candidates(const double* q1, const double* q2, int n, const double* P1x4, const uint8_t* mask_in, double* out_Q, uint8_t* out_mask, int* out_good) override {
            if (n > 0) rc = engine_dlt(eng, seq, q1, q2, n, P1x4, mask_in, out_Q, out_mask, out_good);
        }
    } tri;
    tri.eng = S->eng; tri.seq = seq;
    std::vector<uint8_t> m(mask, mask + n);
    std::vector<double> q;
    double R[9], t[3];
    const int good = vo::recover_pose(&tri, E9, p1_xy, p2_xy, n, K, R, t, m, q);
    if (tri.rc != PMV_OK) return tri.rc;
    memcpy(R9, R, 72); memcpy(t3, t, 24);
    if (n > 0) { memcpy(mask, m.data(), (size_t)n); memcpy(tri4n, q.data(), (size_t)4 * n * 8); }
    *out_good = good;
    return PMV_OK;
}

}  // extern "C"
