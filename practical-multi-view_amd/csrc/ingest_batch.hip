// The feeder: every background pyramid build of frame slots. The reference loads one image per front-end iteration (Frame::Frame /
// Frame::init, Frame.cpp:31-42; featureExtractionThread, OdometryPipeline.cpp:212-229) and tracking touches only frames k-1 and k. Here a
// FEED of B sequences is built on a HIP stream of its own while the sequences already track. Frame f of sequence b lives in slot
// first + f % ring; its source is host memory or the slot itself (staged):
//   * pmv_pipeline_run_batch_streamed: host frames, a short ring per sequence whose slots are recycled;
//   * pmv_pipeline_run_batch: the sequences with build_pyramids, staged in place, ring = n_frames;
//   * pmv_frames_stream_begin .. _end: one sequence of host frames, ring = n.
//
//   * Release. After addFrame(image i) has returned, the sequence's front-end thread reports (OdometryPipeline::on_frame_added) that
//     frames below i are dead. Their kernels have finished: a request returns to its sequence only after the combiner has seen the
//     completion word of its round, so the feeder's stream may overwrite those slots without any GPU-side dependency.
//   * Rounds. A round takes up to F frames from every sequence with room, most-starved first (fewest frames landed ahead of its
//     release point), up to a round's capacity. It is one table + frames block in a pinned staging buffer, and then for host frames
//       copy:   one hipMemcpyAsync of the block into an HBM landing buffer; level 0 is read from there;
//       mapped: no copy call; k_pad_level0 reads level 0 straight from mapped pinned host memory (the staging buffer for a pageable
//               source, the caller's own pinned buffer through its device address otherwise);
//     then one k_pad_level0 and one k_pyrdown launch per level for the whole round, and an event. The sequences of a feed may differ in frame
//     size: a frame's bytes, its place in the staging block and its source address are its sequence's, and its entry of the slot table names
//     its geometry in the context's table (pmv_device.h); grid and LDS of the round's launches are sized for the largest geometry in it. A feed of COLOUR frames (tight BGR, Frame.cpp:33,40-41;
//     pmv_set_frame_format) differs in two things only: a frame is 3 w h bytes, so a round under ROUND_BYTES holds about a third as many, and
//     level 0 is written by k_pad_level0_bgr, which converts on the way - from the same three sources. The launches read the round's slot
//     table (list form), unless the round is consecutive slots from consecutive frames (range form, as every round of a bracket). A bracket
//     (copy form by default) DMAs a pinned source straight into HBM; a staged feed copies only its slot tables into HBM.
//   * Acquire. Each slot carries (frame, round) of its last enqueued build, published with release / acquire atomics. Before a kernel
//     reads a slot, its caller waits in slot_ready on the host until the frame it needs is in the slot's record; the stream of the kernel
//     then waits for that round's event (a combiner once per launch).
//
//   * Preprocessing (pmv_set_frame_preproc; a snapshot per feed, host sources only). A round of such a feed carries, in its header block
//     behind the slot table, a second slot table without sources, its RemapSrcRec and ClaheRec records and - in a bracket, which has no
//     geometry table - the one-entry table they index. With a remap every host frame lands in HBM first (the copy form, whatever
//     PMV_BATCH_INGEST says and for a caller's pinned buffer too: a 2 x 2 byte gather across the host link is a link transaction per tap), and
//     ONE k_remap_src launch takes the place of the level-0 launch: it gathers from the landing buffer straight into level 0 of the slots.
//     With CLAHE, ONE k_clahe_lut + k_clahe_apply pair follows over the round's slots. Then ONE in-place k_pad_level0 launch (no source)
//     builds the REFLECT_101 frame, and the k_pyrdown launches follow as always. A feed without preprocessing launches what it always did.
//
// A sequence is served when it has room for F frames, or has no more than LOW frames landed ahead, or only its last frames remain, or its
// thread is waiting for a frame: a round per released frame would be 5 launches per frame (the launch volume DESIGN §5 suspects behind
// the bimodal throughput). A ring that is not recycled (ring >= n) has all its frames as room from the start: its sequence is fed CHUNK
// frames per round until every frame is built, whether the sequence still runs or not.
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
    // Round events. A feed that recycles slots keeps a ring of NEV (round % NEV): its rounds wait for releases, so a combiner waits on its own
    // round's event, not on a later one's. A feed that does not recycle (every ring >= n) may run any number of rounds ahead of its readers:
    // it has one event per round (`per_round`), created as the rounds come and kept for later feeds.
    static constexpr int NEV = 64;
    static constexpr int ROUND_FRAMES = 64;             // host frames per round at most ...
    static constexpr size_t ROUND_BYTES = 32u << 20;    // ... and no more bytes than this (1241x376: 64 frames = 29.9 MB)
    static constexpr size_t HDR = 16384;                // the round's slot table in front of its frames ...
    static constexpr int TABLE = (int)(HDR / sizeof(PyrListEntry));   // ... and so the frames of a round of staged sources at most
    // a preprocessing round (host frames: ROUND_FRAMES at most) keeps behind its slot table: the same slots without sources (the in-place
    // border launch of a list round), the gather records, the CLAHE records, a bracket's one-entry geometry table
    static constexpr size_t OFF_INPLACE = (size_t)ROUND_FRAMES * sizeof(PyrListEntry);
    static constexpr size_t OFF_REMAP = OFF_INPLACE + (size_t)ROUND_FRAMES * sizeof(PyrListEntry);
    static constexpr size_t OFF_CLAHE = OFF_REMAP + (size_t)ROUND_FRAMES * sizeof(RemapSrcRec);
    static constexpr size_t OFF_GEOM = OFF_CLAHE + (size_t)ROUND_FRAMES * sizeof(ClaheRec);
    static constexpr size_t HDR_PRE = OFF_GEOM + sizeof(PyrLayout);   // bytes of a preprocessing round's header that are in use
    static_assert(HDR_PRE <= HDR && OFF_REMAP % 16 == 0 && OFF_CLAHE % 16 == 0 && OFF_GEOM % 4 == 0, "a preprocessing round's tables fit its header block");
    static constexpr int LOW = 2;                       // frames landed ahead of the release point below which a sequence is served at once
    static constexpr int BRACKET_CHUNK = 16, STAGED_CHUNK = 32;   // frames of a sequence per round: bracket, staged batch (as before the feeder)
    // slot_rec values besides (frame << 32) | round: no feed covers the slot / not built yet, by sequence b of the feed
    static constexpr long long NONE = -1;
    static long long pending(int b) { return -2 - (long long)b; }
    // kept across calls
    hipStream_t stream = nullptr;
    std::vector<hipEvent_t> ev;
    hipEvent_t copied[NBUF] = {};   // copy form: the round's DMA out of its staging buffer is done
    Buf<uint8_t> h_stage{MEM_MAPPED};   // NBUF x buf_bytes, pinned + mapped
    Buf<uint8_t> d_land;                // NBUF x buf_bytes in HBM (copy form and staged feeds: made by the first that needs it)
    size_t buf_bytes = 0;
    Buf<uint8_t> d_lut;                 // CLAHE of a preprocessing feed: frames_per_round LUT blocks (made by the first such feed)
    std::unique_ptr<std::atomic<long long>[]> slot_rec;   // per slot: (frame << 32) | round of its last enqueued build, or NONE / pending(b)
    std::mutex ev_mu;             // hipEventRecord / growth of `ev` (feeder thread) vs hipStreamWaitEvent (readers)
    // one feed
    struct Seq {
        int first = 0, n = 0, ring = 0, F = 1;
        const uint8_t* src = nullptr;   // host address of frame 0, null = staged in the slots
        const uint8_t* dev = nullptr;   // device address of frame 0 when the source is pinned, else null
        std::atomic<int> released{0};   // frames below this are dead
        std::atomic<int> finished{0};
        std::atomic<int> waiting{0};    // its thread is blocked in acquire
        int next = 0;                   // next frame to feed (feeder thread only)
        int w = 0, h = 0, geom = 0;     // its frame size and that size's entry of the context's geometry table (0 in a bracket, which has no list rounds)
        size_t fb = 0;                  // bytes of one of its host frames: w h (gray) or 3 w h (BGR)
        PyrLayout L{};
        const uint32_t* map = nullptr;  // preprocessing with a remap: the packed map of its size (device memory)
    };
    std::unique_ptr<Seq[]> seq;
    pmv_ctx* ctx = nullptr;
    int B = 0, frames_per_round = 1;
    size_t max_fb = 0;            // bytes of the largest host frame of the feed
    bool bgr = false;             // the host frames are tight BGR: level 0 through k_pad_level0_bgr
    // the feed's snapshot of pmv_set_frame_preproc (host sources only; a feed with either has nothing but host sources)
    bool remap = false, clahe = false;
    int border = 0;
    pmv_clahe_params cp{};
    bool table = false;           // the sequences' geometries are in the context's table: list rounds are possible
    bool count_launches = false;  // the feed of a batched run: its launches go into pmv_debug_batch_launches
    bool copy_mode = false, per_round = false, open = false;
    bool dma_release = false;   // copy form of a bracket or staged feed: a staging buffer is free once its DMA is done (else: once its round is)
    std::atomic<int> front_waited{-1};   // newest round the synchronous callers' stream already waits for (slot_ready)
    std::thread th;
    std::atomic<bool> stop{false};
    std::atomic<int> error{0};
    char err[256] = "";
    std::mutex mu;                // sequence threads waiting for frames
    std::condition_variable cv;
    std::atomic<int> waiters{0};
    // statistics of the feed (pmv_batch_ingest_stats)
    long long rounds = 0, frames = 0, bytes = 0;
    double t_memcpy = 0, t_room = 0;
    std::atomic<long long> wait_ns{0};
    size_t ev_index(long long round) const { return (size_t)(per_round ? round : round % NEV); }
};

namespace {

void fail(BatchIngest* g, int code, const char* what, hipError_t e) {
    {
        std::lock_guard<std::mutex> lk(g->mu);
        if (!g->error.load()) snprintf(g->err, sizeof(g->err), "feeder: %s: %s", what, hipGetErrorString(e));
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
            if ((S.ring < S.n && S.finished.load()) || S.next >= S.n) continue;
            all_done = false;
            const int rel = S.released.load();
            const int room = std::min(rel + S.ring, S.n) - S.next;
            if (room <= 0) continue;
            const int ahead = S.next - rel;
            if (room >= S.F || ahead <= BatchIngest::LOW || S.next + room == S.n || S.waiting.load()) cand.push_back({ahead, b});
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
            const int end = std::min(S.released.load() + S.ring, S.n);
            for (int k = std::min(S.F, g->frames_per_round - (int)take.size()); k > 0 && S.next < end; ) {
                const int f = S.next++;
                // a slot that several sequences of a non-recycled feed cover (overlapping staged ranges) is built once, by the first of them
                if (S.ring >= S.n && g->slot_rec[(size_t)(S.first + f)].load() != BatchIngest::pending(c.second)) continue;
                take.push_back({c.second, f});
                k--;
            }
            if ((int)take.size() >= g->frames_per_round) break;
        }
        if (take.empty()) continue;
        const int n = (int)take.size(), buf = (int)(round % BatchIngest::NBUF);
        // The buffer's previous round (round - NBUF) has finished with it: its round is done (a ring event is not re-recorded before
        // round - NBUF + NEV) or, with dma_release, its DMA has read the staging buffer (the landing buffer is overwritten by a later DMA on
        // the same in-order stream, after that round's kernels).
        if (round >= BatchIngest::NBUF &&
            (e = hipEventSynchronize(g->dma_release ? g->copied[buf] : g->ev[g->ev_index(round - BatchIngest::NBUF)])) != hipSuccess) {
            fail(g, PMV_ERR_HIP, "hipEventSynchronize", e); return;
        }
        uint8_t* blk = g->h_stage + (size_t)buf * g->buf_bytes;
        PyrListEntry* tab = (PyrListEntry*)blk;
        // device address of the round's block as the kernels see it: the landing buffer (copy) or the mapped staging buffer
        const uint8_t* dblk = g->copy_mode ? g->d_land + (size_t)buf * g->buf_bytes : g->h_stage.dm() + (size_t)buf * g->buf_bytes;
        // Consecutive slots, all in place or one sequence's consecutive frames (every round of a bracket): the range form, no table lookup in
        // the kernels; in the copy form a pinned source is then DMA'd straight into the landing buffer.
        const BatchIngest::Seq& S0 = g->seq[take[0].first];
        bool range = true;
        for (int i = 1; i < n && range; i++) {
            const BatchIngest::Seq& S = g->seq[take[(size_t)i].first];
            range = S.first + take[(size_t)i].second % S.ring == S0.first + take[0].second % S0.ring + i && S.geom == S0.geom &&
                    (S0.src ? take[(size_t)i].first == take[0].first && take[(size_t)i].second == take[0].second + i : !S.src);
        }
        const bool direct = range && g->dma_release && S0.dev;
        const auto tm0 = std::chrono::steady_clock::now();
        const bool pre = g->remap || g->clahe;
        int nc = 0;                  // frames copied into staging
        size_t cb = 0, hb = 0;       // their bytes (frame after frame, each of its own size); bytes of all frames from host memory
        for (int i = 0; i < n; i++) {
            const BatchIngest::Seq& S = g->seq[take[(size_t)i].first];
            const int f = take[(size_t)i].second;
            tab[i].slot = S.first + f % S.ring;
            tab[i].geom = S.geom;
            tab[i].src = nullptr;   // staged: level 0 in place
            if (!S.src) continue;
            hb += S.fb;
            if (direct) { tab[i].src = dblk + BatchIngest::HDR + (size_t)i * S.fb; continue; }   // (range form: the frames of one sequence)
            if (!g->copy_mode && S.dev) { tab[i].src = S.dev + (size_t)f * S.fb; continue; }   // the caller's pinned frame, in place
            memcpy(blk + BatchIngest::HDR + cb, S.src + (size_t)f * S.fb, S.fb);   // (cb + fb <= frames_per_round * max_fb: the buffer's size)
            tab[i].src = dblk + BatchIngest::HDR + cb;
            cb += S.fb;
            nc++;
        }
        if (nc) g->t_memcpy += std::chrono::duration<double>(std::chrono::steady_clock::now() - tm0).count();
        int pre_w = 0, pre_h = 0;    // preprocessing: the largest level 0 of the round
        if (pre) {   // the round's extra tables, behind its slot table
            PyrListEntry* inplace = (PyrListEntry*)(blk + BatchIngest::OFF_INPLACE);
            RemapSrcRec* rr = (RemapSrcRec*)(blk + BatchIngest::OFF_REMAP);
            ClaheRec* cr = (ClaheRec*)(blk + BatchIngest::OFF_CLAHE);
            const unsigned lut_block = (unsigned)(g->cp.tiles_x * g->cp.tiles_y) * 256u;
            for (int i = 0; i < n; i++) {
                const BatchIngest::Seq& S = g->seq[take[(size_t)i].first];
                inplace[i].src = nullptr; inplace[i].slot = tab[i].slot; inplace[i].geom = tab[i].geom;
                if (g->remap) { rr[i].map = S.map; rr[i].src = tab[i].src; rr[i].slot = tab[i].slot; rr[i].geom = tab[i].geom; rr[i].border = g->border; rr[i].bgr = g->bgr ? 1 : 0; }
                if (g->clahe) {
                    cr[i] = clahe_record(tab[i].slot, tab[i].geom, S.w, S.h, g->cp.clip_limit, g->cp.tiles_x, g->cp.tiles_y);
                    cr[i].lut_off = (unsigned)i * lut_block;   // (i < frames_per_round: inside d_lut)
                }
                pre_w = std::max(pre_w, S.w); pre_h = std::max(pre_h, S.h);
            }
            if (!g->table) memcpy(blk + BatchIngest::OFF_GEOM, &S0.L, sizeof(PyrLayout));   // a bracket: its records name entry 0 of this table
        }
        if (g->copy_mode) {   // frames only for the range form; the table (+ frames) for the list form and for a preprocessing round
            const bool whole = !range || (pre && !direct);   // header and frames in one copy (a preprocessing round has host frames only: nc > 0 unless direct)
            if (pre && direct && (e = hipMemcpyAsync((void*)dblk, blk, BatchIngest::HDR_PRE, hipMemcpyHostToDevice, g->stream)) != hipSuccess) { fail(g, PMV_ERR_HIP, "hipMemcpyAsync", e); return; }
            const uint8_t* from = direct ? S0.src + (size_t)take[0].second * S0.fb : whole ? blk : blk + BatchIngest::HDR;
            const size_t off = whole ? 0 : BatchIngest::HDR;
            const size_t bytes = whole ? (nc ? BatchIngest::HDR + cb : (size_t)n * sizeof(PyrListEntry)) : direct ? (size_t)n * S0.fb : cb;
            if (bytes && (e = hipMemcpyAsync((void*)(dblk + off), from, bytes, hipMemcpyHostToDevice, g->stream)) != hipSuccess) { fail(g, PMV_ERR_HIP, "hipMemcpyAsync", e); return; }
            if ((e = hipEventRecord(g->copied[buf], g->stream)) != hipSuccess) { fail(g, PMV_ERR_HIP, "hipEventRecord", e); return; }
        }
        // Preprocessing: the gather in place of the level-0 launch, then the CLAHE pair, then the border in place - each ONE launch for the whole
        // round, whatever sizes and maps it holds (the records name them). Their geometry table: the context's, or a bracket's own single entry.
        const PyrLayout* pre_geom = g->table ? (const PyrLayout*)ctx->d_geom : (const PyrLayout*)(dblk + BatchIngest::OFF_GEOM);
        auto gather = [&]() {   // level 0's interior from the landing buffer through the maps (counted where the level-0 launch it replaces is)
            if ((e = launch_remap_src(g->stream, ctx->d_slots, pre_geom, (const RemapSrcRec*)(dblk + BatchIngest::OFF_REMAP), n, pre_w, pre_h)) != hipSuccess) {
                fail(g, PMV_ERR_HIP, "k_remap_src", e); return false;
            }
            ctx->preproc_launches[1]++;
            return true;
        };
        auto finish_level0 = [&](const PyrLayout* Lmax) {   // level 0's interior is in the slots; Lmax: of a list round, null: a range round
            if (g->clahe) {
                if ((e = launch_clahe(g->stream, ctx->d_slots, pre_geom, (const ClaheRec*)(dblk + BatchIngest::OFF_CLAHE), n, g->cp.tiles_x * g->cp.tiles_y, pre_w, pre_h,
                                      g->d_lut)) != hipSuccess) { fail(g, PMV_ERR_HIP, "k_clahe_lut / k_clahe_apply", e); return false; }
                ctx->preproc_launches[2]++;
            }
            e = Lmax ? launch_pad_level0_list(g->stream, ctx->d_slots, pre_geom, *Lmax, (const PyrListEntry*)(dblk + BatchIngest::OFF_INPLACE), n)
                     : launch_pad_level0(g->stream, ctx->d_slots, S0.L, tab[0].slot, n, nullptr);
            if (e != hipSuccess) { fail(g, PMV_ERR_HIP, "k_pad_level0 (in place)", e); return false; }
            ctx->preproc_launches[0]++; ctx->preproc_launches[3]++;
            return true;
        };
        int n_levels;
        if (range) {   // one geometry, by value
            const int first = tab[0].slot;
            n_levels = S0.L.n_levels;
            if (g->remap) { if (!gather()) return; }
            else {
                e = g->bgr ? launch_pad_level0_bgr(g->stream, ctx->d_slots, S0.L, first, n, tab[0].src)   // (every frame of a colour feed has a source)
                           : launch_pad_level0(g->stream, ctx->d_slots, S0.L, first, n, tab[0].src);
                if (e != hipSuccess) { fail(g, PMV_ERR_HIP, g->bgr ? "k_pad_level0_bgr" : "k_pad_level0", e); return; }
            }
            if (pre && !finish_level0(nullptr)) return;
            for (int l = 1; l < n_levels; l++)
                if ((e = launch_pyrdown(g->stream, ctx->d_slots, S0.L, l, first, n)) != hipSuccess) { fail(g, PMV_ERR_HIP, "k_pyrdown", e); return; }
        } else {       // geometry per entry; grid, LDS and the levels launched from the largest geometry of THIS round
            if (!g->table) { fail(g, PMV_ERR_INVALID, "a list round in a feed without a geometry table", hipSuccess); return; }
            PyrLayout Lmax{};
            for (int i = 0; i < n; i++) {
                const PyrLayout& Ls = g->seq[take[(size_t)i].first].L;
                Lmax.n_levels = std::max(Lmax.n_levels, Ls.n_levels);
                for (int l = 0; l < Ls.n_levels; l++) { Lmax.w[l] = std::max(Lmax.w[l], Ls.w[l]); Lmax.h[l] = std::max(Lmax.h[l], Ls.h[l]); }
            }
            n_levels = Lmax.n_levels;
            const PyrListEntry* dtab = (const PyrListEntry*)dblk;
            if (g->remap) { if (!gather()) return; }
            else {
                e = g->bgr ? launch_pad_level0_bgr_list(g->stream, ctx->d_slots, ctx->d_geom, Lmax, dtab, n)
                           : launch_pad_level0_list(g->stream, ctx->d_slots, ctx->d_geom, Lmax, dtab, n);
                if (e != hipSuccess) { fail(g, PMV_ERR_HIP, g->bgr ? "k_pad_level0_bgr" : "k_pad_level0", e); return; }
            }
            if (pre && !finish_level0(&Lmax)) return;
            for (int l = 1; l < n_levels; l++)
                if ((e = launch_pyrdown_list(g->stream, ctx->d_slots, ctx->d_geom, Lmax, l, dtab, n)) != hipSuccess) { fail(g, PMV_ERR_HIP, "k_pyrdown", e); return; }
        }
        if (g->count_launches) { ctx->batch_launches[2]++; ctx->batch_launches[3] += n_levels - 1; }
        {
            std::lock_guard<std::mutex> lk(g->ev_mu);
            const size_t k = g->ev_index(round);
            if (k == g->ev.size()) {   // (per_round only: the ring's NEV events exist)
                hipEvent_t ev;
                if ((e = hipEventCreateWithFlags(&ev, hipEventDisableTiming)) != hipSuccess) { fail(g, PMV_ERR_HIP, "hipEventCreateWithFlags", e); return; }
                g->ev.push_back(ev);
            }
            if ((e = hipEventRecord(g->ev[k], g->stream)) != hipSuccess) { fail(g, PMV_ERR_HIP, "hipEventRecord", e); return; }
        }
        for (auto& t : take) {
            const BatchIngest::Seq& S = g->seq[t.first];
            g->slot_rec[(size_t)(S.first + t.second % S.ring)].store(((long long)t.second << 32) | round);   // (seq_cst: see acquire)
        }
        g->rounds++; g->frames += n; g->bytes += (long long)hb;
        round++;
        if (g->waiters.load() > 0) { std::lock_guard<std::mutex> lk(g->mu); g->cv.notify_all(); }
    }
}

// Before a kernel reads `slot` (covered by the feed): waits on the host until its build has been enqueued, and returns the round that builds
// it. A feed that recycles slots: the frame sequence `seq` (the caller's own thread) needs in that slot. Otherwise every slot is built once,
// and any reader may wait for it.
int acquire(BatchIngest* g, int seq, int slot, int* round) {
    BatchIngest::Seq* S = seq >= 0 && seq < g->B ? &g->seq[seq] : nullptr;
    int f = -1;   // the frame needed, -1 = any
    if (!g->per_round) {
        if (!S || slot < S->first || slot >= S->first + S->ring) {
            set_err(g->ctx, "feeder: sequence %d asked for slot %d outside its ring", seq, slot);
            return PMV_ERR_INVALID;
        }
        const int pos = slot - S->first, rel = S->released.load(std::memory_order_relaxed);   // (this thread is the only writer of `released`)
        f = rel + ((pos - rel % S->ring) % S->ring + S->ring) % S->ring;   // the one frame of [rel, rel + ring) that lives in this slot
        if (f >= S->n) {
            set_err(g->ctx, "feeder: sequence %d asked for slot %d (frame %d): past its %d frames", seq, slot, f, S->n);
            return PMV_ERR_INVALID;
        }
    }
    auto have = [&](long long st) { return st >= 0 && (f < 0 || (int)(st >> 32) == f); };
    long long st = g->slot_rec[(size_t)slot].load();
    if (!have(st)) {
        const auto t0 = std::chrono::steady_clock::now();
        std::unique_lock<std::mutex> lk(g->mu);
        if (S) S->waiting.store(1);   // served in the next round whatever its room (initialise() may need more frames than F at once)
        g->waiters.fetch_add(1);
        // (seq_cst on both sides: either this load sees the round's record, or the feeder thread sees the waiter and notifies)
        while (!have(st = g->slot_rec[(size_t)slot].load()) && !g->error.load()) g->cv.wait_for(lk, std::chrono::milliseconds(2));
        g->waiters.fetch_sub(1);
        if (S) S->waiting.store(0);
        lk.unlock();
        g->wait_ns += (long long)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count();
        if (!have(st)) { set_err(g->ctx, "%s", g->err); return g->error.load(); }
    }
    *round = (int)(st & 0xffffffffll);
    return PMV_OK;
}

}  // namespace

#define CKC(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { set_err(ctx, "%s: %s", #x, hipGetErrorString(e_)); return PMV_ERR_HIP; } } while (0)
#define REQ(cond, code, ...) do { if (!(cond)) { set_err(ctx, __VA_ARGS__); return code; } } while (0)

int batch_ingest_begin(pmv_ctx* ctx, BatchIngest*& gp, FeedKind kind, const std::vector<FeedSeq>& seqs, int format, const pmv_frame_preproc* pre) {
    CKC(hipSetDevice(ctx->device));
    // The preprocessing snapshot: every sequence with a host source finds the map of its size, before anything of the feed exists. (The
    // setting's maps have pairwise different sizes and cannot be destroyed while it names them.)
    std::vector<const uint32_t*> maps(seqs.size(), nullptr);
    const bool pre_remap = pre && pre->n_maps > 0, pre_clahe = pre && pre->clahe != 0;
    if (pre_remap) {
        std::lock_guard<std::mutex> lk(ctx->remap_mu);
        for (size_t b = 0; b < seqs.size(); b++) {
            if (!seqs[b].src) continue;
            for (int k = 0; k < pre->n_maps; k++) {
                const pmv_ctx::RemapMap& m = ctx->remap_maps[pre->map_ids[k]];
                if (m.d && m.w == seqs[b].w && m.h == seqs[b].h) maps[b] = (const uint32_t*)m.d;
            }
            REQ(maps[b], PMV_ERR_INVALID, "feeder: sequence %d: its frames are %dx%d and the frame preprocessing setting has no remap map of that size (pmv_set_frame_preproc)",
                (int)b, seqs[b].w, seqs[b].h);
        }
    }
    if (!gp) {
        BatchIngest* g = new BatchIngest();
        gp = g;
        CKC(hipStreamCreateWithFlags(&g->stream, hipStreamNonBlocking));
        g->ev.resize(BatchIngest::NEV);
        for (auto& ev : g->ev) CKC(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        for (auto& ev : g->copied) CKC(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        g->slot_rec.reset(new std::atomic<long long>[(size_t)ctx->n_slots]);
        for (int s = 0; s < ctx->n_slots; s++) g->slot_rec[(size_t)s].store(BatchIngest::NONE);
    }
    BatchIngest* g = gp;
    const int B = (int)seqs.size();
    g->seq.reset(new BatchIngest::Seq[(size_t)B]);
    bool host = false;
    int sum_F = 0;
    g->per_round = true;
    g->table = kind != FEED_BRACKET;   // (a bracket is one sequence whose rounds are all ranges)
    g->count_launches = kind != FEED_BRACKET;
    for (int b = 0; b < B; b++) {
        BatchIngest::Seq& S = g->seq[b];
        const FeedSeq& q = seqs[(size_t)b];
        S.first = q.first; S.n = q.n; S.ring = q.ring; S.src = q.src; S.dev = nullptr; S.map = maps[(size_t)b];
        S.w = q.w; S.h = q.h; S.L = layout_for(ctx, q.w, q.h);
        S.geom = g->table ? ctx->geom_index(q.w, q.h) : 0;
        REQ(S.geom >= 0, PMV_ERR_INVALID, "feeder: sequence %d: no entry for %dx%d frames in the geometry table", b, q.w, q.h);
        S.F = kind == FEED_BRACKET ? BatchIngest::BRACKET_CHUNK : kind == FEED_STAGED ? BatchIngest::STAGED_CHUNK : std::max(1, std::min(8, S.ring / 2));
        sum_F += S.F;
        g->per_round = g->per_round && S.ring >= S.n;
        if (S.src) {
            host = true;
            // A kernel is never handed a pageable address (XNACK is off). Pinned memory whose device address is its host address (hipHostMalloc'ed,
            // torch's pin_memory) is read in place; anything else - pageable, or registered under another device address - is copied into staging.
            hipPointerAttribute_t attr;
            if (hipPointerGetAttributes(&attr, S.src) == hipSuccess && attr.type == hipMemoryTypeHost && attr.hostPointer == (const void*)S.src &&
                attr.devicePointer == attr.hostPointer)
                S.dev = S.src;
            (void)hipGetLastError();   // (a malloc'ed pointer makes hipPointerGetAttributes fail: that is the "pageable" answer)
        }
    }
    g->bgr = host && format == PMV_FRAMES_BGR;
    g->remap = host && pre_remap; g->clahe = host && pre_clahe;   // (a feed with host sources has no others)
    g->border = g->remap ? pre->border_value : 0;
    if (g->clahe) g->cp = pre->clahe_params;
    g->max_fb = 1;
    for (int b = 0; b < B; b++) {
        g->seq[b].fb = (size_t)g->seq[b].w * g->seq[b].h * (g->bgr ? 3 : 1);
        g->max_fb = std::max(g->max_fb, g->seq[b].fb);
    }
    // a round's frames and its buffer's bytes: both from the largest frame of the feed, so every round of frames_per_round frames fits
    g->frames_per_round = host ? (int)std::max<size_t>(1, std::min<size_t>({(size_t)BatchIngest::ROUND_FRAMES, BatchIngest::ROUND_BYTES / g->max_fb, (size_t)sum_F}))
                               : BatchIngest::TABLE;
    const size_t need = (BatchIngest::HDR + (host ? (size_t)g->frames_per_round * g->max_fb : 0) + 4095) & ~(size_t)4095;
    static_assert(BatchIngest::ROUND_FRAMES <= BatchIngest::TABLE, "a round's slot table fits its header block");
    // How host frames reach level 0: PMV_BATCH_INGEST=copy | mapped; by default mapped for a streamed batch and copy for a bracket
    // (the DMA into HBM the single-sequence path has always used). A staged feed's slot tables are always copied into HBM, so its kernels do
    // not read them across the link. No result depends on it.
    const char* mode = getenv("PMV_BATCH_INGEST");
    // A remap gathers 2 x 2 bytes per pixel: never across the host link, so such a feed lands every frame in HBM first.
    g->copy_mode = !host || g->remap || (mode ? !strcmp(mode, "copy") : kind == FEED_BRACKET);
    g->dma_release = g->copy_mode && kind != FEED_STREAMED;   // (a streamed batch keeps the form it was measured with)
    if (g->buf_bytes < need) {   // both buffers are NBUF x buf_bytes: a landing area of the old size goes with the old staging
        g->buf_bytes = 0;
        CKC(g->d_land.release());
        CKC(g->h_stage.ensure(BatchIngest::NBUF * need));
        g->buf_bytes = need;
    }
    if (g->copy_mode) CKC(g->d_land.ensure(BatchIngest::NBUF * g->buf_bytes));
    if (g->clahe) CKC(g->d_lut.ensure((size_t)g->frames_per_round * (size_t)(g->cp.tiles_x * g->cp.tiles_y) * 256));
    g->ctx = ctx; g->B = B;
    // every slot of the feed carries its sequence's geometry and counts as built from here on: its readers wait for its round in slot_ready.
    // The first sequence that covers a slot builds it.
    for (int b = 0; b < B; b++)
        for (int i = 0; i < g->seq[b].ring; i++) {
            const size_t s = (size_t)(g->seq[b].first + i);
            ctx->slot_layout[s] = g->seq[b].L;
            ctx->slot_state[s] = SLOT_BUILT;
            if (g->slot_rec[s].load() == BatchIngest::NONE) g->slot_rec[s].store(BatchIngest::pending(b));
        }
    g->stop.store(false); g->error.store(0); g->err[0] = 0; g->waiters.store(0); g->front_waited.store(-1);
    g->rounds = g->frames = g->bytes = 0; g->t_memcpy = g->t_room = 0; g->wait_ns.store(0);
    g->open = true;
    g->th = std::thread(ingest_loop, ctx, g);
    return PMV_OK;
}

bool batch_ingest_active(const BatchIngest* g) { return g && g->open; }

hipError_t batch_ingest_wait_gpu(BatchIngest* g, hipStream_t s, int round) {
    // The round's event: recorded for this round or, in a ring, NEV rounds later for a later round of the same in-order stream (already
    // enqueued, and dependent on nothing but that stream): waiting for it waits at least for `round`.
    std::lock_guard<std::mutex> lk(g->ev_mu);
    return hipStreamWaitEvent(s, g->ev[g->ev_index(round)], 0);
}

int slot_ready(pmv_ctx* ctx, int slot, BatchIngest* g, int seq, hipStream_t s, int* round) {
    int r = -1;
    if (g && g->open && g->slot_rec[(size_t)slot].load() != BatchIngest::NONE) {   // a slot of the feed
        const int rc = acquire(g, seq, slot, &r);
        if (rc != PMV_OK) return rc;
        if (s && r > g->front_waited.load()) {   // (in-order stream: a wait for round r covers every earlier one)
            CKC(batch_ingest_wait_gpu(g, s, r));
            g->front_waited.store(r);
        }
    }
    if (round) *round = r;
    const uint8_t st = ctx->slot_state[(size_t)slot];
    REQ(st == SLOT_BUILT, PMV_ERR_INVALID, "slot %d %s", slot, st == SLOT_EMPTY ? "holds no frame" : "was staged but its pyramid was never built");
    return PMV_OK;
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
    if (g->th.joinable()) g->th.join();
    const hipError_t e = hipStreamSynchronize(g->stream);
    for (int b = 0; b < g->B; b++)
        for (int i = 0; i < g->seq[b].ring; i++) {
            const int s = g->seq[b].first + i;
            const long long rec = g->slot_rec[(size_t)s].exchange(BatchIngest::NONE);
            if (rec != BatchIngest::NONE && rec < 0) ctx->slot_state[(size_t)s] = g->seq[b].src ? SLOT_EMPTY : SLOT_STAGED;   // never received its frame
        }
    g->open = false;
    if (g->error.load()) { set_err(ctx, "%s", g->err); return g->error.load(); }
    if (e != hipSuccess) { set_err(ctx, "feeder: hipStreamSynchronize: %s", hipGetErrorString(e)); return PMV_ERR_HIP; }
    return PMV_OK;
}

void batch_ingest_stats(const BatchIngest* g, double* out) {
    out[0] = (double)g->rounds; out[1] = (double)g->frames; out[2] = (double)g->bytes;
    out[3] = g->t_memcpy; out[4] = g->t_room; out[5] = 1e-9 * (double)g->wait_ns.load();
}

void batch_ingest_destroy(BatchIngest*& g) {
    if (!g) return;
    g->stop.store(true);
    if (g->th.joinable()) g->th.join();
    if (g->stream) { (void)hipStreamSynchronize(g->stream); (void)hipStreamDestroy(g->stream); }
    for (auto& ev : g->ev) if (ev) (void)hipEventDestroy(ev);
    for (auto& ev : g->copied) if (ev) (void)hipEventDestroy(ev);
    delete g;
    g = nullptr;
}

}  // namespace pmv

using namespace pmv;

extern "C" {

// A bracket is a feed of one sequence from host memory whose ring is not recycled. `gray`: n frames in the context's frame format.
int pmv_frames_stream_begin(pmv_ctx* ctx, int first_slot, int n, const uint8_t* gray, int w, int h) {
    REQ(ctx && gray, PMV_ERR_INVALID, "pmv_frames_stream_begin: null argument");
    REQ(first_slot >= 0 && n >= 1 && first_slot + n <= ctx->n_slots, PMV_ERR_CAPACITY, "pmv_frames_stream_begin: slots [%d,%d) out of range (n_slots %d)", first_slot, first_slot + n, ctx->n_slots);
    REQ(w >= 40 && h >= 40 && w <= ctx->max_w && h <= ctx->max_h, PMV_ERR_CAPACITY, "pmv_frames_stream_begin: frame %dx%d outside capacity %dx%d", w, h, ctx->max_w, ctx->max_h);
    REQ(!batch_ingest_active(ctx->ingest), PMV_ERR_INVALID, "pmv_frames_stream_begin: a stream is already open (pmv_frames_stream_end first)");
    CKC(hipSetDevice(ctx->device));
    // frames in the slots about to be overwritten may still be read by work in flight on the front-end stream
    CKC(hipStreamSynchronize(ctx->s_front));
    return batch_ingest_begin(ctx, ctx->ingest, FEED_BRACKET, {FeedSeq{first_slot, n, n, gray, w, h}}, ctx->frame_format, &ctx->preproc);
}

int pmv_frames_stream_end(pmv_ctx* ctx) {
    REQ(ctx, PMV_ERR_INVALID, "null ctx");
    if (!batch_ingest_active(ctx->ingest)) return PMV_OK;
    CKC(hipSetDevice(ctx->device));
    return batch_ingest_end(ctx, ctx->ingest);
}

}  // extern "C"
