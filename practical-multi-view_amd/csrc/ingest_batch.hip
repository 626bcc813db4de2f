// Streamed ingest of a batched run (pmv_pipeline_run_batch_streamed). The reference loads one image per front-end iteration
// (Frame::Frame / Frame::init, Frame.cpp:31-42; featureExtractionThread, OdometryPipeline.cpp:212-229) and tracking touches only frames
// k-1 and k, so a sequence needs a short RING of device slots instead of one slot per frame: frame f of sequence b lives in slot
// first_slot[b] + f % ring. One ingest thread on its own HIP stream fills the rings of all B sequences:
//
//   * Release. After addFrame(image i) has returned, the sequence's front-end thread reports (OdometryPipeline::on_frame_added) that
//     frames below i are dead. Their kernels have finished: a request returns to its sequence only after the combiner has seen the
//     completion word of its round, so the ingest stream may overwrite those slots without any GPU-side dependency.
//   * Rounds. A round takes up to F frames from every sequence with room, most-starved first (fewest frames landed ahead of its
//     release point), up to ROUND_FRAMES frames. It is one table + frames block in a pinned staging buffer, and then
//       copy:   one hipMemcpyAsync of the block into an HBM landing buffer; level 0 is read from there;
//       mapped: no copy call; k_pad_level0_list reads level 0 straight from mapped pinned host memory (the staging buffer for a
//               pageable source, the caller's own pinned buffer through its device address otherwise);
//     then one k_pad_level0_list and one k_pyrdown_list launch per level for the whole round, and an event.
//   * Acquire. Each slot carries (frame, round) of its last enqueued build, published with release / acquire atomics. Before an LK or
//     detect request, the sequence thread waits on the host until the frame it needs is in the slot's record; the combiner then makes
//     its stream wait for that round's event once per launch.
//
// A sequence is served when it has room for F frames, or has no more than LOW frames landed ahead, or only its last frames remain, or its
// thread is waiting for a frame: a round per released frame would be 5 launches per frame (the launch volume DESIGN §5 suspects behind
// the bimodal throughput).
#include "pmv_ctx.h"
#include "ingest_batch.h"
#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstring>
#include <memory>
#include <mutex>
#include <thread>

namespace pmv {

struct BatchIngest {
    static constexpr int NBUF = 4;                      // staging (and landing) buffers: rounds in flight
    static constexpr int NEV = 64;                      // round events (round % NEV): a combiner waits on its own round's, not on a later one's
    static constexpr int ROUND_FRAMES = 64;             // frames per round at most ...
    static constexpr size_t ROUND_BYTES = 32u << 20;    // ... and no more bytes than this (1241x376: 64 frames = 29.9 MB)
    static constexpr size_t HDR = 4096;                 // the round's slot table in front of its frames
    static constexpr int LOW = 2;                       // frames landed ahead of the release point below which a sequence is served at once
    // kept across calls
    hipStream_t stream = nullptr;
    hipEvent_t ev[NEV] = {};
    uint8_t* h_stage = nullptr;   // NBUF x buf_bytes, pinned + mapped
    uint8_t* dm_stage = nullptr;  // its device address
    uint8_t* d_land = nullptr;    // NBUF x buf_bytes in HBM (copy mode only)
    size_t buf_bytes = 0, land_bytes = 0;
    std::unique_ptr<std::atomic<long long>[]> slot_state;   // per slot: (frame << 32) | round of its last enqueued build, -1 = none
    std::mutex ev_mu;             // hipEventRecord (ingest thread) vs hipStreamWaitEvent (combiners) on the same event
    // one call
    struct Seq {
        int first = 0, n = 0;
        const uint8_t* src = nullptr;   // host address of frame 0
        const uint8_t* dev = nullptr;   // device address of frame 0 when the source is pinned, else null
        std::atomic<int> released{0};   // frames below this are dead
        std::atomic<int> finished{0};
        std::atomic<int> waiting{0};    // its thread is blocked in batch_ingest_acquire
        int next = 0;                   // next frame to ingest (ingest thread only)
    };
    std::unique_ptr<Seq[]> seq;
    pmv_ctx* ctx = nullptr;
    int B = 0, ring = 0, F = 1, w = 0, h = 0, frames_per_round = 1;
    size_t fb = 0;
    PyrLayout L{};
    bool copy_mode = false;
    std::thread th;
    std::atomic<bool> stop{false};
    std::atomic<int> error{0};
    char err[256] = "";
    std::mutex mu;                // sequence threads waiting for frames
    std::condition_variable cv;
    std::atomic<int> waiters{0};
    // statistics of the call (pmv_batch_ingest_stats)
    long long rounds = 0, frames = 0, bytes = 0;
    double t_memcpy = 0, t_room = 0;
    std::atomic<long long> wait_ns{0};
};

namespace {

void fail(BatchIngest* g, int code, const char* what, hipError_t e) {
    {
        std::lock_guard<std::mutex> lk(g->mu);
        if (!g->error.load()) snprintf(g->err, sizeof(g->err), "batch ingest: %s: %s", what, hipGetErrorString(e));
        g->error.store(code);
    }
    g->cv.notify_all();
}

void ingest_loop(pmv_ctx* ctx, BatchIngest* g) {
    tl_prof = &ctx->prof;
    hipError_t e = hipSetDevice(ctx->device);
    if (e != hipSuccess) { fail(g, PMV_ERR_HIP, "hipSetDevice", e); return; }
    std::vector<std::pair<int, int>> cand;        // (frames landed ahead of the release point, sequence)
    std::vector<std::pair<int, int>> take;        // (sequence, frame) of this round
    for (long long round = 0;; ) {
        if (g->stop.load() || g->error.load()) return;
        cand.clear();
        bool all_done = true;
        for (int b = 0; b < g->B; b++) {
            BatchIngest::Seq& S = g->seq[b];
            if (S.finished.load() || S.next >= S.n) continue;
            all_done = false;
            const int rel = S.released.load();
            const int room = std::min(rel + g->ring, S.n) - S.next;
            if (room <= 0) continue;
            const int ahead = S.next - rel;
            if (room >= g->F || ahead <= BatchIngest::LOW || S.next + room == S.n || S.waiting.load()) cand.push_back({ahead, b});
        }
        if (all_done) return;
        if (cand.empty()) {   // no sequence has room: the only place this thread sleeps
            const auto t0 = std::chrono::steady_clock::now();
            std::this_thread::sleep_for(std::chrono::microseconds(50));
            g->t_room += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
            continue;
        }
        std::stable_sort(cand.begin(), cand.end());   // most-starved first
        take.clear();
        for (auto& c : cand) {
            BatchIngest::Seq& S = g->seq[c.second];
            const int room = std::min(S.released.load() + g->ring, S.n) - S.next;
            const int k = std::min({room, g->F, g->frames_per_round - (int)take.size()});
            for (int i = 0; i < k; i++) take.push_back({c.second, S.next + i});
            S.next += std::max(k, 0);
            if ((int)take.size() >= g->frames_per_round) break;
        }
        const int n = (int)take.size(), buf = (int)(round % BatchIngest::NBUF);
        // the buffer's previous round (round - NBUF) has finished reading it (its event is not re-recorded before round - NBUF + NEV)
        if (round >= BatchIngest::NBUF && (e = hipEventSynchronize(g->ev[(round - BatchIngest::NBUF) % BatchIngest::NEV])) != hipSuccess) {
            fail(g, PMV_ERR_HIP, "hipEventSynchronize", e); return;
        }
        uint8_t* blk = g->h_stage + (size_t)buf * g->buf_bytes;
        PyrListEntry* tab = (PyrListEntry*)blk;
        // device address of the round's block as the kernels see it: the landing buffer (copy) or the mapped staging buffer
        const uint8_t* dblk = g->copy_mode ? g->d_land + (size_t)buf * g->buf_bytes : g->dm_stage + (size_t)buf * g->buf_bytes;
        const auto tm0 = std::chrono::steady_clock::now();
        bool copied = false;
        for (int i = 0; i < n; i++) {
            const BatchIngest::Seq& S = g->seq[take[(size_t)i].first];
            const int f = take[(size_t)i].second;
            tab[i].slot = S.first + f % g->ring;
            tab[i].pad = 0;
            if (!g->copy_mode && S.dev) { tab[i].src = S.dev + (size_t)f * g->fb; continue; }   // the caller's pinned frame, in place
            memcpy(blk + BatchIngest::HDR + (size_t)i * g->fb, S.src + (size_t)f * g->fb, g->fb);
            tab[i].src = dblk + BatchIngest::HDR + (size_t)i * g->fb;
            copied = true;
        }
        if (copied) g->t_memcpy += std::chrono::duration<double>(std::chrono::steady_clock::now() - tm0).count();
        if (g->copy_mode && (e = hipMemcpyAsync((void*)dblk, blk, BatchIngest::HDR + (size_t)n * g->fb, hipMemcpyHostToDevice, g->stream)) != hipSuccess) {
            fail(g, PMV_ERR_HIP, "hipMemcpyAsync", e); return;
        }
        const PyrListEntry* dtab = (const PyrListEntry*)dblk;
        if ((e = launch_pad_level0_list(g->stream, ctx->d_slots, g->L, dtab, n)) != hipSuccess) { fail(g, PMV_ERR_HIP, "k_pad_level0_list", e); return; }
        for (int l = 1; l < g->L.n_levels; l++)
            if ((e = launch_pyrdown_list(g->stream, ctx->d_slots, g->L, l, dtab, n)) != hipSuccess) { fail(g, PMV_ERR_HIP, "k_pyrdown_list", e); return; }
        {
            std::lock_guard<std::mutex> lk(g->ev_mu);
            if ((e = hipEventRecord(g->ev[round % BatchIngest::NEV], g->stream)) != hipSuccess) { fail(g, PMV_ERR_HIP, "hipEventRecord", e); return; }
        }
        for (auto& t : take) {
            const BatchIngest::Seq& S = g->seq[t.first];
            g->slot_state[(size_t)(S.first + t.second % g->ring)].store(((long long)t.second << 32) | round);   // (seq_cst: see acquire)
        }
        g->rounds++; g->frames += n; g->bytes += (long long)n * (long long)g->fb;
        round++;
        if (g->waiters.load() > 0) { std::lock_guard<std::mutex> lk(g->mu); g->cv.notify_all(); }
    }
}

}  // namespace

#define CKC(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { set_err(ctx, "%s: %s", #x, hipGetErrorString(e_)); return PMV_ERR_HIP; } } while (0)

int batch_ingest_begin(pmv_ctx* ctx, int B, const int* first_slot, const int* n_frames, const uint8_t* const* host_frames, int ring, int w, int h,
                       BatchIngest** out) {
    CKC(hipSetDevice(ctx->device));
    if (!ctx->bingest) {
        BatchIngest* g = new BatchIngest();
        ctx->bingest = g;
        CKC(hipStreamCreateWithFlags(&g->stream, hipStreamNonBlocking));
        for (auto& ev : g->ev) CKC(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        g->slot_state.reset(new std::atomic<long long>[(size_t)ctx->n_slots]);
    }
    BatchIngest* g = ctx->bingest;
    g->fb = (size_t)w * h;
    g->frames_per_round = (int)std::max<size_t>(1, std::min<size_t>(BatchIngest::ROUND_FRAMES, BatchIngest::ROUND_BYTES / g->fb));
    const size_t need = (BatchIngest::HDR + (size_t)g->frames_per_round * g->fb + 4095) & ~(size_t)4095;
    static_assert(BatchIngest::ROUND_FRAMES * sizeof(PyrListEntry) <= BatchIngest::HDR, "the slot table fits its header block");
    const char* mode = getenv("PMV_BATCH_INGEST");   // diagnostic: copy | mapped (default); no result depends on it
    g->copy_mode = mode && !strcmp(mode, "copy");
    if (g->buf_bytes < need) {
        if (g->h_stage) { CKC(hipHostFree(g->h_stage)); g->h_stage = nullptr; }
        if (g->d_land) { CKC(hipFree(g->d_land)); g->d_land = nullptr; g->land_bytes = 0; }
        g->buf_bytes = 0;
        CKC(hipHostMalloc(&g->h_stage, BatchIngest::NBUF * need, hipHostMallocMapped | hipHostMallocCoherent));
        CKC(hipHostGetDevicePointer((void**)&g->dm_stage, g->h_stage, 0));
        g->buf_bytes = need;
    }
    if (g->copy_mode && g->land_bytes < g->buf_bytes) {
        CKC(hipMalloc(&g->d_land, BatchIngest::NBUF * g->buf_bytes));
        g->land_bytes = g->buf_bytes;
    }
    g->seq.reset(new BatchIngest::Seq[(size_t)B]);
    g->ctx = ctx; g->B = B; g->ring = ring; g->w = w; g->h = h;
    g->F = std::max(1, std::min(8, ring / 2));
    g->L = layout_for(ctx, w, h);
    for (int b = 0; b < B; b++) {
        BatchIngest::Seq& S = g->seq[b];
        S.first = first_slot[b]; S.n = n_frames[b]; S.src = host_frames[b]; S.dev = nullptr;
        // A kernel is never handed a pageable address (XNACK is off). Pinned memory whose device address is its host address (hipHostMalloc'ed,
        // torch's pin_memory) is read in place; anything else - pageable, or registered under another device address - is copied into staging.
        hipPointerAttribute_t attr;
        if (hipPointerGetAttributes(&attr, S.src) == hipSuccess && attr.type == hipMemoryTypeHost && attr.hostPointer == (const void*)S.src &&
            attr.devicePointer == attr.hostPointer)
            S.dev = S.src;
        (void)hipGetLastError();   // (a malloc'ed pointer makes hipPointerGetAttributes fail: that is the "pageable" answer)
        for (int i = 0; i < ring; i++) g->slot_state[(size_t)(S.first + i)].store(-1);
    }
    g->stop.store(false); g->error.store(0); g->err[0] = 0; g->waiters.store(0);
    g->rounds = g->frames = g->bytes = 0; g->t_memcpy = g->t_room = 0; g->wait_ns.store(0);
    g->th = std::thread(ingest_loop, ctx, g);
    *out = g;
    return PMV_OK;
}

int batch_ingest_acquire(BatchIngest* g, int seq, int slot, int* round) {
    BatchIngest::Seq& S = g->seq[seq];
    const int pos = slot - S.first, rel = S.released.load(std::memory_order_relaxed);   // (this thread is the only writer of `released`)
    // the one frame of [rel, rel + ring) that lives in this slot
    const int f = rel + ((pos - rel % g->ring) % g->ring + g->ring) % g->ring;
    if (pos < 0 || pos >= g->ring || f >= S.n) {
        set_err(g->ctx, "batch ingest: sequence %d asked for slot %d (frame %d): outside its ring [%d, %d) or past its %d frames", seq, slot, f, S.first, S.first + g->ring, S.n);
        return PMV_ERR_INVALID;
    }
    auto have = [&](long long st) { return st >= 0 && (int)(st >> 32) == f; };
    long long st = g->slot_state[(size_t)slot].load();
    if (!have(st)) {
        const auto t0 = std::chrono::steady_clock::now();
        std::unique_lock<std::mutex> lk(g->mu);
        S.waiting.store(1);   // served in the next round whatever its room (initialise() may need more frames than F at once)
        g->waiters.fetch_add(1);
        // (seq_cst on both sides: either this load sees the round's record, or the ingest thread sees the waiter and notifies)
        while (!have(st = g->slot_state[(size_t)slot].load()) && !g->error.load()) g->cv.wait_for(lk, std::chrono::milliseconds(2));
        g->waiters.fetch_sub(1);
        S.waiting.store(0);
        lk.unlock();
        g->wait_ns += (long long)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count();
        if (!have(st)) { set_err(g->ctx, "%s", g->err); return g->error.load(); }
    }
    *round = (int)(st & 0xffffffffll);
    return PMV_OK;
}

hipError_t batch_ingest_wait_gpu(void* arg, hipStream_t s, int round) {
    BatchIngest* g = (BatchIngest*)arg;
    // The round's event: recorded for this round or, NEV rounds later, for a later round of the same in-order stream (already enqueued, and
    // dependent on nothing but that stream): waiting for it waits at least for `round`.
    std::lock_guard<std::mutex> lk(g->ev_mu);
    return hipStreamWaitEvent(s, g->ev[round % BatchIngest::NEV], 0);
}

void batch_ingest_release(BatchIngest* g, int seq, int frame) {
    BatchIngest::Seq& S = g->seq[seq];
    if (frame > S.released.load(std::memory_order_relaxed)) S.released.store(frame);
}

void batch_ingest_finish(BatchIngest* g, int seq) {
    g->seq[seq].released.store(g->seq[seq].n);
    g->seq[seq].finished.store(1);
}

int batch_ingest_end(pmv_ctx* ctx, BatchIngest* g) {
    g->stop.store(true);
    if (g->th.joinable()) g->th.join();
    const hipError_t e = hipStreamSynchronize(g->stream);
    for (int b = 0; b < g->B; b++)
        for (int i = 0; i < g->ring; i++) {
            const int s = g->seq[b].first + i;
            ctx->slot_layout[(size_t)s] = g->L;
            if (g->slot_state[(size_t)s].load() < 0) ctx->slot_layout[(size_t)s].n_levels = 0;   // never received a frame
        }
    if (g->error.load()) { set_err(ctx, "%s", g->err); return g->error.load(); }
    if (e != hipSuccess) { set_err(ctx, "batch ingest: hipStreamSynchronize: %s", hipGetErrorString(e)); return PMV_ERR_HIP; }
    return PMV_OK;
}

void batch_ingest_stats(const BatchIngest* g, double* out) {
    out[0] = (double)g->rounds; out[1] = (double)g->frames; out[2] = (double)g->bytes;
    out[3] = g->t_memcpy; out[4] = g->t_room; out[5] = 1e-9 * (double)g->wait_ns.load();
}

void batch_ingest_destroy(pmv_ctx* ctx) {
    BatchIngest* g = ctx->bingest;
    if (!g) return;
    g->stop.store(true);
    if (g->th.joinable()) g->th.join();
    if (g->stream) { (void)hipStreamSynchronize(g->stream); (void)hipStreamDestroy(g->stream); }
    for (auto& ev : g->ev) if (ev) (void)hipEventDestroy(ev);
    if (g->h_stage) (void)hipHostFree(g->h_stage);
    if (g->d_land) (void)hipFree(g->d_land);
    delete g;
    ctx->bingest = nullptr;
}

}  // namespace pmv
