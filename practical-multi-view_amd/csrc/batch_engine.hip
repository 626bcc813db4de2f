// Batch engine (several independent sequences per GPU through "the same kernels with a leading batch dimension").
//
// A single sequence can never fill 256 CUs: frame k+1's tracks depend on frame k's result (~300 workgroups in flight) and the
// back-end is a serial chain of small solves. Sequences, however, are independent (the path shards by sequence). Here every
// sequence keeps the reference's own host structure — a front-end and a back-end thread running the unchanged adapters of
// host/vo_pipeline.cpp — but its plugin calls do not launch anything themselves: they hand a request to the COMBINER thread of
// their kernel class (LK, detectors, PnP, BA, two-view DLT; one HIP stream each, so the classes overlap on the GPU) and sleep. A
// combiner takes whatever requests have accumulated while its previous launch was running, issues ONE batched launch for all of
// them (k_lk_batch, k_gftt_* / k_st_* over the cells of several frames, k_pnp_*_batch, the k_bamB_* chain with the problem index
// in blockIdx.y, k_tri_dlt_batch), synchronises once and wakes exactly the callers it served. Only the five combiner threads talk
// to the HIP runtime: no runtime-lock contention, no per-sequence stream; the batch size adapts to the load by itself. Inputs that
// the callers prepared in their pinned blocks are pulled into HBM by one gather kernel per batch (k_stage_in) instead of one DMA
// per request. Every block of a batched launch executes exactly the code and the block index of the single-sequence launch, so
// each sequence's results are bit-identical to its own single run (tests/test_batch_gpu.py).
#include "pmv_ctx.h"
#include "backend.h"
#include "batch_engine.h"
#include "ingest_batch.h"
#include "pmv_block.h"
#include "pmv_wait.h"
#include <sys/prctl.h>
#include <algorithm>
#include <atomic>
#include <chrono>
#include <climits>
#include <condition_variable>
#include <cstring>
#include <memory>
#include <thread>
#include <time.h>

namespace pmv {

namespace {

struct Req {
    int kind = Q_LK;   // a ReqKind (batch_engine.h)
    int rc = PMV_OK;
    // completion word: the owner sleeps on it (futex), the combiner stores 1 and wakes that one sleeper. No lock is involved: with a
    // condition variable under the queue's mutex the 50-70 owners of a round woke up one by one into a fight for that mutex, while the
    // next requests were waiting to get in through the same mutex.
    std::atomic<int> done{0};
    char err[200] = "";
    virtual ~Req() {}
};
struct LKReq : Req {
    int prev_slot, next_slot, n;
    const float* prev_xy; float* out_xy; uint8_t* status; float* err_out;
    uint8_t* iters_out = nullptr;   // optional: LK iterations each track took (the caller's ordering hint for its next request)
    std::vector<int> order;   // block -> track order of THIS request (local indices, -1 = padding), built by the caller
    int base = 0;             // filled by the combiner: first index in the concatenated arrays
    int geom = 0;             // filled by the combiner: the geometry-table entry of its two frames
    int ring_round = -1;      // the feed round that builds the two frames (-1 = nothing to wait for)
    // Q_LK_EX (pmv_lk_track_ex / _fb): out_xy is in/out, flags = LKX_*; with LKX_FB the three back outputs
    int flags = 0;
    float* back_xy = nullptr; uint8_t* back_status = nullptr; float* back_err = nullptr;
};
struct KnnReq : Req {         // Q_KNN: one kNNFeatureMatcher call (pmv_knn_match's contract)
    int src_slot, cmp_slot, n, m, n_nn, window;
    const int* src_xy; const int* cmp_xy; int* out_best; float* err_out;
    int base = 0;             // filled by the combiner: first index in the round's result arrays (shared with the LK requests)
    int geom = 0;             // filled by the combiner: the geometry-table entry of its two frames
    int ring_round = -1;
};
struct DetReq : Req {
    int slot, n_cells, max_per_cell, unlimited;
    const int* cells; double quality, min_dist;   // FAST: quality = threshold, min_dist = the non-max flag
    int* out_xy; double* out_score; int* out_count;
    float* out_resp = nullptr;                    // FAST: KeyPoint::response per keypoint
    int cell_base = 0;
    int ring_round = -1;      // as LKReq::ring_round
    // GFTT through the general kernels (pmv_batch_detect_gftt_ex): the caller's block size, response kind and k, and the optional host mask
    int ext = 0, block_size = 3, use_harris = 0; double k = 0.0;
    const uint8_t* mask = nullptr; int mask_stride = 0;
    // Q_GFTT_FRAME (pmv_batch_detect_gftt_frame): the region (cells points at it, n_cells = 1, max_per_cell = the capacity of the corner list);
    // filled by the combiner: the first entry of its record list among the round's, its index in its group
    int roi[4] = {0, 0, 0, 0};
    size_t list_off = 0;
    // pmv_batch_detect_gftt_refill: a frame request whose mask is painted on the device from these tracks (`mask` = the base mask or null);
    // filled by the combiner: the first entry of its tracks in the round's refill block
    int refill = 0, n_trk = 0, radius = 0;
    const float* trk_xy = nullptr; const int* trk_prio = nullptr; uint8_t* out_keep = nullptr;
    size_t trk_off = 0;
    bool has_mask() const { return mask != nullptr || refill != 0; }
};
struct SubpixReq : Req {      // Q_SUBPIX: one pmv_batch_corner_subpix call; p's zero zone is the effective one (subpix_zero_zone)
    int slot, n;
    float* xy; uint8_t* iters_out; uint8_t* flags_out;
    pmv_subpix_params p;
    int base = 0;             // filled by the combiner: first index in the round's record and result arrays
    int geom = 0;             // filled by the combiner: the geometry-table entry of its frame
};
struct PnPReq : Req { BackendBuffers* b; PnPProblem P; PnPLayout L; };
struct BAReq : Req { BackendBuffers* b; BAArgs A; BaIoLayout L; int max_iterations; };
struct DltReq : Req { BackendBuffers* b; DltProblem P; DltLayout L; };
struct TriTracksReq : Req { BackendBuffers* b; TriTracksProblem P; TriTracksLayout L; };
struct FPReq : Req { BackendBuffers* b; FivePointProblem P; FivePointLayout L; };
// Q_ESSENTIAL, Q_FUNDAMENTAL, Q_HOMOGRAPHY: a whole findEssentialMat / findFundamentalMat / findHomography. Its caller returns as soon as the kernel's completion word of ITS request is seen, which may be long
// before the round's launch ends (a round ends with its slowest request) - so the record cannot live on the caller's stack like the others:
// the combiner's store into `done` after its stream sync would land in a dead frame. The engine owns one record per seq and kind; `inflight` is 1
// from the submit until the combiner has released the record after the round, and the seq's next call of that kind waits for that before it
// fills the record again.
struct WholeReq : Req { BackendBuffers* b = nullptr; WholeLayout L{}; std::atomic<int> inflight{0}; };
template <class Pt> struct WholeReqOf : WholeReq { WholeProblem<Pt> P; };
using EssReq = WholeReqOf<double>;
using FundReq = WholeReqOf<float>;   // (Q_FUNDAMENTAL and Q_HOMOGRAPHY: the same record)

// per-round scratch of a combiner: grows with slack (GROW_SLACK), in HBM or in mapped pinned memory (.dev = the address kernels use)
struct DScratch : Growable { DScratch() : Growable(MEM_DEVICE, GROW_SLACK) {} };
struct HScratch : Growable { HScratch() : Growable(MEM_MAPPED, GROW_SLACK) {} };

enum Role { R_LK = 0, R_DET, R_PNP, R_BA, R_DLT, R_FP, R_COUNT };
struct Queue {   // pending requests of one kernel class
    std::mutex mu;
    std::condition_variable cv_new;
    std::vector<Req*> pending;
    std::chrono::steady_clock::time_point first_arrival;   // when `pending` last went from empty to non-empty
    int min_batch = 0;     // copy of BatchEngine::min_batch of the class: submit() wakes a combiner at the first and at the min_batch-th request only
    bool stop = false;
};
constexpr int MAX_LANES = 4;
// One combiner = one thread + one HIP stream + its staging buffers. A class may have several (PMV_BATCH_LANES, default 1): while
// one waits for its launch, the next takes the requests that have arrived meanwhile instead of letting them sit for a whole round.
struct Combiner {
    std::thread th;
    hipStream_t s = nullptr;           // this combiner's stream (lanes of a class may share one: BatchEngine::streams)
    bool owns_stream = true;
    hipEvent_t ev = nullptr;           // blocking-sync event for the interrupt-driven wait
    HScratch h_desc; DScratch d_desc;   // per-batch descriptors (+ stage-in jobs), pinned mirror and device copy
    long batches = 0, requests = 0;
    double t_idle = 0, t_work = 0, t_sync = 0;   // seconds: waiting for requests / processing a batch / inside hipStreamSynchronize
    double t_cpu = 0;                            // CPU seconds of the combiner thread itself
    // LK staging + mapped pinned result blocks; detector buffers (only used by combiners of those classes)
    HScratch h_front, h_cells, h_det; DScratch d_front, d_cells, d_eig, d_cellmax, d_spill, d_det_xy, d_det_score, d_det_count;
    // masks of the extended GFTT requests of a round (detector combiner, made by the first round that has one): the cells' mask sub-views
    // packed one after the other, pinned mirror and HBM copy
    HScratch h_gmask; DScratch d_gmask;
    // whole-frame GFTT and refill requests of a round (detector combiner, made by the first round that has one, grown to the largest round
    // seen): the groups' blocks one after the other, one list entry per pixel of the round's regions
    FrameDetScratch fds{GROW_SLACK, MEM_MAPPED};
    // corner sub-pixel requests of a round (detector combiner, made by the first round that has one): [point records | positions | updates |
    // flags] in one mapped pinned block; the weight tables of the round's parameter groups, pinned mirror and HBM copy
    HScratch h_spx, h_spx_tab; DScratch d_spx_tab;
    // kNN matcher rounds (LK combiners): [stage-in job | request records | coordinate lists], pinned mirror and HBM copy; FAST score maps (detector combiner)
    HScratch h_knn; DScratch d_knn, d_fast_score;
    // extended LK requests (LK combiners, made by the first round that has one): [LKBlock | LKExt] records of a round; back results of
    // cap_tracks tracks as [positions | err | status], indexed like the forward results
    HScratch h_lkx, h_back;
    // results of cap_tracks tracks (LK combiners; mapped pinned, the kernels write them through .dm()); the detector combiner's overflow bits
    Buf<float> h_out_xy{MEM_MAPPED}, h_err{MEM_MAPPED}; Buf<uint8_t> h_status{MEM_MAPPED}; Buf<uint16_t> h_work{MEM_MAPPED};
    Buf<int> d_flags;
    RoundSignal sig;                   // completion word of the "flag" wait (pmv_wait.h)
    RoundSignal::Diag sig_diag;        // diagnostic (PMV_BATCH_TIMING=1, printed when the engine goes)
};

// one input block to pull from mapped pinned host memory into HBM (16-byte granules; both buffers have >= 16 B of slack)
struct StageJob { const char* src; char* dst; unsigned bytes, pad; };
__global__ __launch_bounds__(256) void k_stage_in(const StageJob* __restrict__ jobs) { BACKEND_PRIO();
    const StageJob j = jobs[blockIdx.y];
    const unsigned n16 = (j.bytes + 15u) >> 4;
    const uint4* __restrict__ src = (const uint4*)j.src;
    uint4* __restrict__ dst = (uint4*)j.dst;
    for (unsigned i = blockIdx.x * 256 + threadIdx.x; i < n16; i += gridDim.x * 256) dst[i] = src[i];
}

}  // namespace

struct BatchEngine {
    pmv_ctx* ctx = nullptr;
    int B = 0;
    int linger_us = 0;
    // Round-forming policy: a combiner that finds fewer than min_batch[class] requests waiting gives the others up to max_linger_us
    // (counted from the arrival of the oldest one) to join. Without it the classes have a second, stable operating point - lanes firing as
    // soon as anything is pending, rounds of a third of the size, the fixed cost of a round (launches, completion signal, wake-ups) paid
    // three times as often: the same binary then ran at 53 k instead of 65-69 k frames/s in one run out of five (profiles/r03_batch_exp_af.log).
    int min_batch[R_COUNT] = {0, 0, 0, 0, 0, 0};
    int max_linger_us = 300;
    int wait_mode = 3;   // 0 spin (hipStreamSynchronize), 1 query + yield, 2 blocking event, 3 completion word + timed sleeps
    std::vector<BackendBuffers*> slots;   // one back-end workspace set per concurrent sequence
    std::unique_ptr<EssReq[]> ess;        // one whole-findEssentialMat request record per concurrent sequence (see WholeReq)
    std::unique_ptr<FundReq[]> fund;      // ... and one whole-findFundamentalMat record
    std::unique_ptr<FundReq[]> homog;     // ... and one whole-findHomography record
    // combiners (thread + stream) per class. Round 2, host-bound: 2 and 3 per class cost more host CPU (smaller batches) than they won in
    // latency (25.7k -> 23.3k -> 19.5k frames/s at B = 64). Round 3, with the track tables the host has headroom and the LK class is the one
    // that is busy all the time - a launch ends with its slowest track, so a single LK stream idles most SIMDs during every tail: PMV_BATCH_LANES
    // sets all classes, PMV_BATCH_LANES_LK / _PNP / _BA one class.
    int lanes[R_COUNT] = {1, 1, 1, 1, 1, 1};
    // HIP streams per class (<= lanes): lane l launches on stream l % streams. Lanes that share a stream overlap their HOST halves (forming a
    // round, scattering its results, waking the owners) with each other's kernels while the kernels themselves run one after the other
    // with every wave slot of the class to themselves; lanes on different streams also overlap their kernels.
    int streams[R_COUNT] = {0, 0, 0, 0, 0, 0};   // 0 = one per lane
    Queue queue[R_COUNT];
    Combiner comb[R_COUNT][MAX_LANES];
    size_t cap_tracks = 0;
    bool lk_lpt = true;       // PMV_LK_LPT=0: the round-2 block order (x-sorted stripes per XCD, request after request)
    bool exclusive = false;
    std::mutex exclusive_mu;
    // The frames of a batched run are built by the context's batch feeder (ctx->bingest) WHILE the sequences already track. A request
    // carries the feed round that builds its frames (its caller has waited in slot_ready until that round was enqueued); the combiner of
    // the launch makes its stream wait for the newest such round on the GPU. Before this the 1.1 ms of pyramid kernels per sequence ran back
    // to back in front of everything: 141 ms of a 3 s pass at B = 128 with nothing else on the GPU.
};

namespace {

void fail_all(std::vector<Req*>& batch, int code, const char* what, hipError_t e) {
    for (Req* r : batch) { r->rc = code; snprintf(r->err, sizeof(r->err), "batch engine: %s: %s", what, hipGetErrorString(e)); }
}
#define EK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fail_all(batch, PMV_ERR_HIP, #x, e_); return; } } while (0)

// Waiting for a batch: hipStreamSynchronize spins on a host core; with five combiners and 2 B sequence threads on a 16-core share
// the cores are better spent on the sequences' host work, so the default is an interrupt-driven wait on a blocking event
// (PMV_BATCH_WAIT=spin | yield | block).
hipError_t wait_stream(BatchEngine* E, Combiner& C);
#define SYNC_TIMED(C) do { const auto t0_ = std::chrono::steady_clock::now(); EK(wait_stream(E, (C))); (C).t_sync += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0_).count(); } while (0)

hipError_t wait_stream(BatchEngine* E, Combiner& C) {
    if (E->wait_mode == 0) return hipStreamSynchronize(C.s);
    if (E->wait_mode == 1) {
        for (;;) {
            const hipError_t e = hipStreamQuery(C.s);
            if (e != hipErrorNotReady) return e;
            std::this_thread::yield();
        }
    }
    if (E->wait_mode == 2) {
        // (measured: with a blocking-sync event the runtime still spins 100 + 200 us before it sleeps in the driver - for rounds of
        // 0.15-1.4 ms the five combiner threads burned 17 of the 59 CPU-seconds of a B = 128 run)
        hipError_t e = hipEventRecord(C.ev, C.s);
        if (e != hipSuccess) return e;
        return hipEventSynchronize(C.ev);
    }
    // completion word (the signal kernel raises its priority as the back-end kernels do). It tells US that the round is over; the runtime has
    // not been asked anything about this stream since the launches: one query per round lets it retire the round's commands now.
    static const bool query_each_round = !(getenv("PMV_BATCH_QUERY") && atoi(getenv("PMV_BATCH_QUERY")) == 0);
    return C.sig.signal_and_wait<true>(C.s, query_each_round, &C.sig_diag);
}

// Admission of a request into a round: its frame (slot_b < 0) or frame pair still holds built pyramids, a pair agrees in size, and - where
// the launch takes the geometry from the context's table (geom given) - the size is one the batch declared. On refusal the request carries
// rc and err, and the round goes on without it. `what` names the kernel class in the message.
bool admit_frames(pmv_ctx* ctx, Req* r, const char* what, int slot_a, int slot_b, int* geom) {
    const PyrLayout& a = ctx->slot_layout[slot_a];
    r->rc = PMV_ERR_INVALID;
    if (slot_b < 0) {
        if (slot_ready(ctx, slot_a)) { snprintf(r->err, sizeof(r->err), "batch %s: slot %d holds no built pyramid", what, slot_a); return false; }
    } else {
        const PyrLayout& b = ctx->slot_layout[slot_b];
        if (slot_ready(ctx, slot_a) || slot_ready(ctx, slot_b) || a.w[0] != b.w[0] || a.h[0] != b.h[0]) { snprintf(r->err, sizeof(r->err), "batch %s: slot has no pyramid / sizes differ", what); return false; }
    }
    if (geom && (*geom = ctx->geom_index(a.w[0], a.h[0])) < 0) {
        snprintf(r->err, sizeof(r->err), "batch %s: slot %d holds a %dx%d frame, which is %s", what, slot_a, a.w[0], a.h[0],
                 slot_b < 0 ? "no declared size of this session" : "no sequence's size in this batch");
        return false;
    }
    r->rc = PMV_OK;
    return true;
}

// ---- LK -------------------------------------------------------------------------------------------------------------------------
// back results of a round's forward-backward tracks: lk_back_block over the lane's h_back at cap_tracks tracks
size_t back_bytes(size_t cap) { Carve c; lk_back_block(c, cap); return c.bytes() + 64; }
LkBackBlock back_block(const Combiner& C, size_t cap) { Carve c = carve_of(C.h_back); return lk_back_block(c, cap); }
void process_lk(BatchEngine* E, Combiner& C, std::vector<Req*>& batch) {
    pmv_ctx* ctx = E->ctx;
    hipStream_t s = C.s;
    std::vector<LKReq*> lk;
    std::vector<KnnReq*> knn;   // (sequences that run the kNN matcher: the same role, the same round)
    std::vector<LKReq*> lkx;    // (extended LK requests: one more launch for all of them)
    for (Req* r : batch) { if (r->kind == Q_KNN) knn.push_back((KnnReq*)r); else if (r->kind == Q_LK_EX) lkx.push_back((LKReq*)r); else lk.push_back((LKReq*)r); }
    // ---- LK: one launch for the tracks of every requesting sequence, whatever their frame sizes: a request's geometry is the one staged in
    // its prev slot (prev and next of ONE request must agree), carried by each of its track records as an index into the context's table
    const unsigned long long pitch = ctx->cap.slot_bytes;
    int total_tracks = 0, total_blocks = 0, need_ring = -1;
    for (LKReq* r : lk) {
        if (!admit_frames(ctx, r, "LK", r->prev_slot, r->next_slot, &r->geom)) continue;
        r->base = total_tracks;
        total_tracks += r->n;
        total_blocks += (int)r->order.size();
        need_ring = std::max(need_ring, r->ring_round);
    }
    // ---- kNN matcher: one k_knn_round launch for the requests of the round. Its results use the indices behind the LK tracks in the same
    // mapped pinned result blocks (best index: the first n ints of the request's 2 n coordinate floats; window error: the error block).
    // The round block, pinned mirror and HBM copy: [stage-in job | at byte 64: KnnRound x requests | src list, cmp list of every live request,
    // each a multiple of 16 bytes]. The same two functions size it (dry run) and carve it.
    int knn_tracks = 0, knn_max_n = 0;
    auto knn_head = [&](Carve& c) { c.take<StageJob>(1); return c.take<KnnRound>(knn.size(), 64); };
    auto knn_lists = [](Carve& c, const KnnReq* r, Carved<int>* src, Carved<int>* cmp) {
        *src = c.take<int>(2 * (size_t)r->n, 16); *cmp = c.take<int>(2 * (size_t)r->m, 16); c.skip_to(16);
    };
    Carved<int> l_src, l_cmp;
    Carve knn_need;
    knn_head(knn_need);
    for (KnnReq* r : knn) {
        if (!admit_frames(ctx, r, "kNN", r->src_slot, r->cmp_slot, &r->geom)) continue;
        r->base = total_tracks + knn_tracks;
        knn_tracks += r->n;
        knn_max_n = std::max(knn_max_n, r->n);
        knn_lists(knn_need, r, &l_src, &l_cmp);
        need_ring = std::max(need_ring, r->ring_round);
    }
    bool ring_waited = false;
    if (knn_tracks > 0) {
        if (need_ring >= 0) { EK(batch_ingest_wait_gpu(ctx->bingest, s, need_ring)); ring_waited = true; }
        if ((size_t)total_tracks + (size_t)knn_tracks > E->cap_tracks) { fail_all(batch, PMV_ERR_CAPACITY, "more tracks than B * max_tracks", hipSuccess); return; }
        EK(C.h_knn.ensure(knn_need.bytes() + 64)); EK(C.d_knn.ensure(knn_need.bytes() + 64));
        Carve c(C.h_knn.p, C.d_knn.p, C.h_knn.cap);
        const Carved<KnnRound> rec = knn_head(c);
        int n_rec = 0;
        for (KnnReq* r : knn) {
            if (r->rc != PMV_OK) continue;
            KnnRound& k = rec.h[n_rec++];
            k.src_off = (unsigned long long)r->src_slot * pitch; k.cmp_off = (unsigned long long)r->cmp_slot * pitch;
            knn_lists(c, r, &l_src, &l_cmp);
            k.src_xy = l_src.d; memcpy(l_src.h, r->src_xy, (size_t)r->n * 8);
            k.cmp_xy = l_cmp.d; if (r->m) memcpy(l_cmp.h, r->cmp_xy, (size_t)r->m * 8);
            k.out_best = (int*)C.h_out_xy.dm() + 2 * (size_t)r->base; k.out_err = C.h_err.dm() + r->base;
            k.n = r->n; k.m = r->m; k.nn_window = knn_pack(r->n_nn, r->window); k.geom = r->geom;
        }
        // one gather pulls records and lists into HBM (every workgroup of a request scans its whole candidate list): no DMA call
        *(StageJob*)C.h_knn.p = StageJob{C.h_knn.dev + rec.off, (char*)rec.d, (unsigned)(c.bytes() - rec.off), 0};
        hipLaunchKernelGGL(k_stage_in, dim3(64, 1), dim3(256), 0, s, (const StageJob*)C.h_knn.dev);
        EK(hipGetLastError());
        EK(launch_knn_round_geom(s, ctx->d_slots, ctx->d_geom, rec.d, n_rec, knn_max_n));
        ctx->batch_launches[1]++;
    }
    if (total_tracks > 0) {
        if (need_ring >= 0 && !ring_waited) EK(batch_ingest_wait_gpu(ctx->bingest, s, need_ring));
        if ((size_t)total_tracks > E->cap_tracks) { fail_all(batch, PMV_ERR_CAPACITY, "more tracks than B * max_tracks", hipSuccess); return; }
        const size_t bytes = sizeof(LKBlock) * (size_t)total_blocks;
        EK(C.h_front.ensure(bytes + 64));
        LKBlock* hblk = (LKBlock*)C.h_front.p;
        int bpos = 0;
        std::vector<LKReq*> live;
        auto put = [&](const LKReq* r, int o) {
            if (o < 0) return;   // (padding entries of the striped order: the launch carries real tracks only)
            LKBlock& k = hblk[bpos++];
            k.prev_off = (unsigned long long)r->prev_slot * pitch;
            k.next_off = (unsigned long long)r->next_slot * pitch;
            k.track = r->base + o;
            k.x = r->prev_xy[2 * (size_t)o]; k.y = r->prev_xy[2 * (size_t)o + 1];
            k.geom = r->geom;
        };
        for (LKReq* r : lk) {
            if (r->rc != PMV_OK) continue;
            if (!E->lk_lpt) for (int o : r->order) put(r, o);
            live.push_back(r);
        }
        if (E->lk_lpt) {
            // longest-predicted tracks first, over the WHOLE round: every request's order is "most expensive first" (engine_lk), the
            // launch takes the k-th track of every request before any (k + 1)-th. Workgroups start in index order, so the tracks that
            // will iterate longest start first and the launch does not end with one of them started last (a launch ends with its slowest
            // track: makespan <= work / slots + longest track for an arbitrary order).
            size_t kmax = 0;
            for (LKReq* r : live) kmax = std::max(kmax, r->order.size());
            for (size_t k = 0; k < kmax; k++)
                for (LKReq* r : live)
                    if (k < r->order.size()) put(r, r->order[k]);
        }
        LKParams P = lk_launch_params(ctx);
        static const bool lk_stamps = getenv("PMV_LK_STAMPS") != nullptr;   // diagnostic: phase timers of every 64th track (pmv_debug_lk_stamps)
        if (lk_stamps) {
            static std::mutex stamps_mu;   // two LK lanes
            std::lock_guard<std::mutex> lk_(stamps_mu);
            if (!ctx->d_lk_stamps && ctx->d_lk_stamps.ensure(16 * 8) == hipSuccess) (void)hipMemset(ctx->d_lk_stamps, 0, 16 * 8);
        }
        P.stamps = lk_stamps ? ctx->d_lk_stamps : nullptr;
        // mapped pinned: every workgroup reads its 32-byte record once, no copy launch
        EK(launch_lk_batch(s, ctx->d_slots, (const LKBlock*)C.h_front.dev, bpos, ctx->d_geom, P, C.h_out_xy.dm(), C.h_status.dm(), C.h_err.dm(), C.h_work.dm()));
        ctx->batch_launches[0]++;
    }
    // ---- extended LK: the round's pmv_lk_track_ex / _fb requests in ONE launch of the extended batch kernels; their results take the
    // indices behind the plain tracks and the matcher's in the same result blocks, the back results the same indices of the back block
    int ext_tracks = 0;
    for (LKReq* r : lkx) {
        if (!admit_frames(ctx, r, "LK", r->prev_slot, r->next_slot, &r->geom)) continue;
        r->base = total_tracks + knn_tracks + ext_tracks;
        ext_tracks += r->n;
    }
    if (ext_tracks > 0) {
        const size_t cap = E->cap_tracks;
        if ((size_t)total_tracks + (size_t)knn_tracks + (size_t)ext_tracks > cap) { fail_all(batch, PMV_ERR_CAPACITY, "more tracks than B * max_tracks", hipSuccess); return; }
        EK(C.h_lkx.ensure((sizeof(LKBlock) + sizeof(LKExt)) * (size_t)ext_tracks + 64));
        EK(C.h_back.ensure(back_bytes(cap)));
        Carve cx = carve_of(C.h_lkx);   // [LKBlock | LKExt] records of the round, read through the mapped alias
        const Carved<LKBlock> blk = cx.take<LKBlock>((size_t)ext_tracks);
        const Carved<LKExt> ext = cx.take<LKExt>((size_t)ext_tracks);
        LKBlock* hblk = blk.h;
        LKExt* hext = ext.h;
        int bpos = 0;
        size_t kmax = 0;
        for (LKReq* r : lkx) if (r->rc == PMV_OK) kmax = std::max(kmax, (size_t)r->n);
        for (size_t k = 0; k < kmax; k++)   // the engine's default order: track k of every request before any track k + 1
            for (LKReq* r : lkx) {
                if (r->rc != PMV_OK || k >= (size_t)r->n) continue;
                LKBlock& b = hblk[bpos];
                b.prev_off = (unsigned long long)r->prev_slot * pitch; b.next_off = (unsigned long long)r->next_slot * pitch;
                b.track = r->base + (int)k; b.x = r->prev_xy[2 * k]; b.y = r->prev_xy[2 * k + 1]; b.geom = r->geom;
                LKExt& x = hext[bpos++];
                const bool init = (r->flags & LKX_INIT) != 0;
                x.ix = init ? r->out_xy[2 * k] : 0.f; x.iy = init ? r->out_xy[2 * k + 1] : 0.f; x.flags = r->flags; x.opt = 0;
            }
        const LKParams P = lk_launch_params(ctx);
        const LkBackBlock back = back_block(C, cap);
        EK(launch_lk_batch_ex(s, ctx->d_slots, blk.d, ext.d, bpos, ctx->d_geom, P, C.h_out_xy.dm(),
                              C.h_status.dm(), C.h_err.dm(), C.h_work.dm(), back.xy.d, back.status.d, back.err.d));
        ctx->batch_launches[0]++;
    }
    SYNC_TIMED(C);
    for (LKReq* r : lkx) {
        if (r->rc != PMV_OK) continue;
        memcpy(r->out_xy, C.h_out_xy + (size_t)2 * r->base, (size_t)r->n * 8);
        memcpy(r->status, C.h_status + r->base, (size_t)r->n);
        memcpy(r->err_out, C.h_err + r->base, (size_t)r->n * 4);
        if (r->flags & LKX_FB) {
            const LkBackBlock back = back_block(C, E->cap_tracks);
            memcpy(r->back_xy, back.xy.h + (size_t)2 * r->base, (size_t)r->n * 8);
            memcpy(r->back_err, back.err.h + r->base, (size_t)r->n * 4);
            memcpy(r->back_status, back.status.h + r->base, (size_t)r->n);
        }
        ctx->add_lk_work(C.h_work + r->base, (size_t)r->n);
    }
    for (LKReq* r : lk) {
        if (r->rc != PMV_OK) continue;
        memcpy(r->out_xy, C.h_out_xy + (size_t)2 * r->base, (size_t)r->n * 8);
        memcpy(r->status, C.h_status + r->base, (size_t)r->n);
        memcpy(r->err_out, C.h_err + r->base, (size_t)r->n * 4);
        if (r->iters_out) for (int i = 0; i < r->n; i++) r->iters_out[i] = (uint8_t)(C.h_work[(size_t)r->base + i] & 0xffu);
        ctx->add_lk_work(C.h_work + r->base, (size_t)r->n);
    }
    for (KnnReq* r : knn) {
        if (r->rc != PMV_OK) continue;
        memcpy(r->out_best, (const int*)C.h_out_xy + 2 * (size_t)r->base, (size_t)r->n * 4);
        memcpy(r->err_out, C.h_err + r->base, (size_t)r->n * 4);
    }
}

// ---- detectors --------------------------------------------------------------------------------------------------------------------
// result block of a round's detector launches, written by the kernels through the mapped alias: [xy | score | count | overflow flags]
struct DetBlock { Carved<int> xy; Carved<double> score; Carved<int> count, flags; };
// The detector role serves three request families in one round: they share the stream and the round's one wait, nothing else. Each family
// forms its groups, sizes its scratch and enqueues its launches (enqueue: false after a failed runtime call, which has failed the whole
// batch - EKF), keeps what it carved, and scatters its results after the wait (collect). A family without a request adds nothing.
#define EKF(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fail_all(batch, PMV_ERR_HIP, #x, e_); return false; } } while (0)

// ---- cell detectors: requests with the same parameters AND the same frame geometry share a launch (cells of several frames); the
// geometry is the one actually staged in each request's slot (KITTI 00-02, 03 and 04-10 have three different sizes)
// FAST (grouped by threshold, non-max flag and max_per_cell) keeps a score byte per pixel of its cells, which may be whole frames:
// its score maps are sized by the pixels of the round (d_fast_score), the cell record's offset into them stays within int.
// Extended GFTT requests (ext) also agree in block size, response kind, k and has-mask; a round without one launches what it always did.
struct DetCells {
    struct Group { int kind, max_per_cell, unlimited; double quality, min_dist; PyrLayout L; std::vector<DetReq*> reqs; int n_cells = 0; size_t out_off = 0; int max_pix = 0;
                   int ext = 0, block_size = 3, use_harris = 0; double k = 0.0; bool has_mask = false; };
    std::vector<DetReq*> reqs; std::vector<Group> groups;
    DetBlock D{};
    bool enqueue(BatchEngine* E, Combiner& C, std::vector<Req*>& batch) {
        pmv_ctx* ctx = E->ctx; hipStream_t s = C.s;
        size_t fast_pix = 0, mask_bytes = 0;
        for (DetReq* r : reqs) {
            if (!admit_frames(ctx, r, "detect", r->slot, -1, nullptr)) continue;
            const PyrLayout& Lr = ctx->slot_layout[r->slot];
            if (r->kind == Q_FAST) {
                size_t pix = 0;
                for (int i = 0; i < r->n_cells; i++) pix += (size_t)r->cells[4 * i + 2] * r->cells[4 * i + 3];
                if (fast_pix + pix > (size_t)INT_MAX) { r->rc = PMV_ERR_CAPACITY; snprintf(r->err, sizeof(r->err), "batch FAST: the cells of the round cover more than 2^31 pixels"); continue; }
                fast_pix += pix;
            }
            size_t mask_pix = 0;
            if (r->mask) for (int i = 0; i < r->n_cells; i++) mask_pix += (size_t)r->cells[4 * i + 2] * r->cells[4 * i + 3];
            if (mask_bytes + mask_pix > (size_t)INT_MAX) { r->rc = PMV_ERR_CAPACITY; snprintf(r->err, sizeof(r->err), "batch GFTT: the masks of the round cover more than 2^31 pixels"); continue; }
            mask_bytes += mask_pix;
            Group* g = nullptr;
            for (Group& x : groups)
                if (x.kind == r->kind && x.max_per_cell == r->max_per_cell && x.unlimited == r->unlimited && x.quality == r->quality && x.min_dist == r->min_dist &&
                    x.ext == r->ext && (!r->ext || (x.block_size == r->block_size && x.use_harris == r->use_harris && x.k == r->k && x.has_mask == (r->mask != nullptr))) &&
                    x.L.w[0] == Lr.w[0] && x.L.h[0] == Lr.h[0] && x.L.n_levels == Lr.n_levels) { g = &x; break; }
            if (!g) {
                groups.push_back(Group{r->kind, r->max_per_cell, r->unlimited, r->quality, r->min_dist, Lr, {}, 0, 0});
                g = &groups.back();
                if (r->ext) { g->ext = 1; g->block_size = r->block_size; g->use_harris = r->use_harris; g->k = r->k; g->has_mask = r->mask != nullptr; }
            }
            r->cell_base = g->n_cells; g->n_cells += r->n_cells; g->reqs.push_back(r);
        }
        if (reqs.empty()) return true;   // (a round of frame or sub-pixel requests alone has no cell launch)
        size_t tot_cells = 0, tot_out = 0;
        size_t eig_cells = 0;   // cells of the GFTT / ShiTomasi groups: the response, cell-maximum and spill areas are theirs alone
        for (Group& g : groups) { g.out_off = tot_out; tot_cells += g.n_cells; tot_out += (size_t)g.n_cells * g.max_per_cell; if (g.kind != Q_FAST) eig_cells += g.n_cells; }
        const size_t cells_bytes = tot_cells * CELL_STRIDE * 4;
        EKF(C.h_cells.ensure(cells_bytes + 64));   // (+ the stage-in job of a round with FAST cells)
        EKF(C.d_eig.ensure(eig_cells * CELL_PIX * sizeof(double))); EKF(C.d_cellmax.ensure(eig_cells * 8)); EKF(C.d_spill.ensure(eig_cells * CELL_PIX * 4));
        EKF(C.h_det.ensure(tot_out * 16 + tot_cells * 4 + 64));   // (det_block)
        if (mask_bytes) { EKF(C.h_gmask.ensure(mask_bytes + 64)); EKF(C.d_gmask.ensure(mask_bytes + 64)); }
        int* hc = (int*)C.h_cells.p;
        size_t cpos = 0, fpos = 0, mpos = 0;
        for (Group& g : groups)
            for (DetReq* r : g.reqs) {
                int* recs = hc + cpos * CELL_STRIDE;
                pack_cells(recs, r->cells, r->n_cells, r->slot);
                // int 5 of a record: the offset of a masked cell's mask bytes, of a FAST cell's score bytes
                if (r->mask) mpos = gftt_pack_mask((uint8_t*)C.h_gmask.p, mpos, recs, r->cells, r->n_cells, r->mask, r->mask_stride);
                if (g.kind == Q_FAST)
                    for (int* d = recs; d < recs + (size_t)r->n_cells * CELL_STRIDE; d += CELL_STRIDE) { d[5] = (int)fpos; fpos += (size_t)d[2] * d[3]; g.max_pix = std::max(g.max_pix, d[2] * d[3]); }
                cpos += (size_t)r->n_cells;
            }
        if (mask_bytes) EKF(hipMemcpyAsync(C.d_gmask.p, C.h_gmask.p, mask_bytes, hipMemcpyHostToDevice, s));
        if (fast_pix > 0) {
            // every thread of k_fast_score reads its cell record: the records of the round go to HBM by one gather (no DMA call)
            EKF(C.d_cells.ensure(cells_bytes + 64)); EKF(C.d_fast_score.ensure(fast_pix + 64));
            StageJob* job = (StageJob*)((char*)C.h_cells.p + ((cells_bytes + 15) & ~(size_t)15));
            *job = StageJob{C.h_cells.dev, (char*)C.d_cells.p, (unsigned)cells_bytes, 0};
            hipLaunchKernelGGL(k_stage_in, dim3(1, 1), dim3(256), 0, s, (const StageJob*)(C.h_cells.dev + ((cells_bytes + 15) & ~(size_t)15)));
            EKF(hipGetLastError());
        }
        EKF(hipMemsetAsync(C.d_flags, 0, 16, s));
        int need_ring = -1;
        for (DetReq* r : reqs) if (r->rc == PMV_OK) need_ring = std::max(need_ring, r->ring_round);
        if (need_ring >= 0) EKF(batch_ingest_wait_gpu(ctx->bingest, s, need_ring));
        size_t c0 = 0, e0 = 0;   // first cell of the group among all cells of the round / among those with a response area (c0 = e0 in a round without FAST)
        Carve c = carve_of(C.h_det);
        D = DetBlock{c.take<int>(2 * tot_out), c.take<double>(tot_out), c.take<int>(tot_cells), c.take<int>(1)};
        for (Group& g : groups) {
            const int* dc = (const int*)C.h_cells.dev + c0 * CELL_STRIDE;
            int* dxy = D.xy.d + g.out_off * 2;
            double* dsc = D.score.d + g.out_off;
            int* dcnt = D.count.d + c0;
            if (g.kind == Q_GFTT && g.ext)
                EKF(launch_gftt_ex(s, ctx->d_slots, g.L, dc, g.n_cells, g.max_per_cell, g.quality, g.min_dist, g.unlimited, gftt_ext(g.block_size, g.use_harris, g.k),
                                   g.has_mask ? (const uint8_t*)C.d_gmask.p : nullptr, (float*)C.d_eig.p + e0 * CELL_PIX, (unsigned*)C.d_cellmax.p + 2 * e0, dxy, dcnt,
                                   C.d_flags, (unsigned*)C.d_spill.p + e0 * CELL_PIX));
            else if (g.kind == Q_GFTT)
                EKF(launch_gftt(s, ctx->d_slots, g.L, dc, g.n_cells, g.max_per_cell, g.quality, g.min_dist, g.unlimited, (float*)C.d_eig.p + e0 * CELL_PIX,
                                (unsigned*)C.d_cellmax.p + 2 * e0, dxy, dcnt, C.d_flags, (unsigned*)C.d_spill.p + e0 * CELL_PIX));
            else if (g.kind == Q_SHITOMASI)
                EKF(launch_shitomasi(s, ctx->d_slots, g.L, dc, g.n_cells, g.max_per_cell, g.quality, (double*)C.d_eig.p + e0 * CELL_PIX,
                                     (unsigned long long*)C.d_cellmax.p + e0, dxy, dsc, dcnt, C.d_flags, (unsigned*)C.d_spill.p + e0 * CELL_PIX));
            else   // FAST: records from HBM, float responses in the group's share of the score block
                EKF(launch_fast(s, ctx->d_slots, g.L, (const int*)C.d_cells.p + c0 * CELL_STRIDE, g.n_cells, g.max_pix, g.max_per_cell, (int)g.quality, (int)g.min_dist,
                                (uint8_t*)C.d_fast_score.p, dxy, (float*)dsc, dcnt));
            c0 += g.n_cells;
            if (g.kind != Q_FAST) e0 += g.n_cells;
        }
        EKF(hipMemcpyAsync(D.flags.h, C.d_flags, 4, hipMemcpyDeviceToHost, s));   // (the kernels set the bits with atomics: device memory)
        return true;
    }
    void collect() {
        if (reqs.empty()) return;
        const int flags = *D.flags.h;
        size_t c0 = 0;
        for (Group& g : groups) {
            for (DetReq* r : g.reqs) {
                if (g.kind == Q_GFTT && (flags & 4)) { r->rc = PMV_ERR_OVERFLOW; snprintf(r->err, sizeof(r->err), "more corners than the no-limit capacity in a cell (batched launch)"); continue; }
                const size_t o = g.out_off + (size_t)r->cell_base * g.max_per_cell;
                memcpy(r->out_xy, D.xy.h + o * 2, (size_t)r->n_cells * g.max_per_cell * 8);
                if (r->out_score) memcpy(r->out_score, D.score.h + o, (size_t)r->n_cells * g.max_per_cell * 8);
                if (g.kind == Q_FAST) memcpy(r->out_resp, (const float*)(D.score.h + g.out_off) + (size_t)r->cell_base * g.max_per_cell, (size_t)r->n_cells * g.max_per_cell * 4);
                memcpy(r->out_count, D.count.h + c0 + r->cell_base, (size_t)r->n_cells * 4);
            }
            c0 += g.n_cells;
        }
    }
};

// ---- whole-frame GFTT and refill: requests that agree in every argument but the slot, the region and the mask's bytes, on frames of one
// layout, share ONE pass-1 and ONE pass-2 launch (launch_gftt_frame); the round's refill requests share ONE select and ONE paint launch in
// front of them. The scratch is the combiner's FrameDetScratch.
struct DetFrames {
    struct Group { DetReq* key; PyrLayout L; std::vector<DetReq*> reqs; int grid_x = 0; size_t info_base = 0; GfttFrameBlock B{}; };
    std::vector<DetReq*> reqs; std::vector<Group> groups;
    RefillBlock T{}; pmv_ctx* ctx = nullptr;   // T: the round's refill tables (a round with a refill request)
    bool enqueue(BatchEngine* E, Combiner& C, std::vector<Req*>& batch) {
        ctx = E->ctx; hipStream_t s = C.s; FrameDetScratch& S = C.fds;
        size_t f_pix = 0, f_mask = 0, f_n = 0;
        // refill requests: their number, their track entries, the bytes of the regions that are painted from 255 (they lie behind the uploaded
        // masks and are not copied), the largest region
        size_t rf_n = 0, rf_trk = 0, rf_plain = 0, rf_max = 0;
        for (DetReq* r : reqs) {
            if (!admit_frames(ctx, r, "detect", r->slot, -1, nullptr)) continue;
            const PyrLayout& Lr = ctx->slot_layout[r->slot];
            if (r->roi[0] + r->roi[2] > Lr.w[0] || r->roi[1] + r->roi[3] > Lr.h[0]) {   // (the slot was re-used since the call's check)
                r->rc = PMV_ERR_INVALID; snprintf(r->err, sizeof(r->err), "batch GFTT: region (%d,%d,%d,%d) is not inside the %dx%d frame", r->roi[0], r->roi[1], r->roi[2], r->roi[3], Lr.w[0], Lr.h[0]);
                continue;
            }
            const size_t pix = (size_t)r->roi[2] * r->roi[3];
            if (r->has_mask() && f_mask + rf_plain + pix + (r->refill ? 8 : 0) > (size_t)INT_MAX) { r->rc = PMV_ERR_CAPACITY; snprintf(r->err, sizeof(r->err), "batch GFTT: the masks of the round cover more than 2^31 pixels"); continue; }
            if (r->mask) f_mask += pix + (r->refill ? 6 : 0);   // (a refill request's bytes begin and end at a multiple of 4)
            else if (r->refill) rf_plain += (pix + 3) & ~(size_t)3;
            if (r->refill) { r->trk_off = rf_trk; rf_trk += refill_pad(r->n_trk); rf_n++; rf_max = std::max(rf_max, pix); }
            Group* g = nullptr;
            for (Group& x : groups) {
                const DetReq* k = x.key;
                if (k->max_per_cell == r->max_per_cell && k->unlimited == r->unlimited && k->quality == r->quality && k->min_dist == r->min_dist && k->ext == r->ext &&
                    k->block_size == r->block_size && k->use_harris == r->use_harris && k->k == r->k && k->has_mask() == r->has_mask() &&
                    x.L.w[0] == Lr.w[0] && x.L.h[0] == Lr.h[0] && x.L.n_levels == Lr.n_levels) { g = &x; break; }
            }
            if (!g) { groups.push_back(Group{r, Lr, {}}); g = &groups.back(); }
            r->list_off = f_pix; f_pix += pix; f_n++;
            g->grid_x = std::max(g->grid_x, gftt_frame_grid_x(r->roi[2], r->roi[3]));
            g->reqs.push_back(r);
        }
        if (groups.empty()) return true;
        Carve need, rneed;
        for (Group& g : groups) gftt_frame_block(need, g.reqs.size(), (size_t)g.key->max_per_cell);
        EKF(S.lists(f_pix, f_n, need.bytes()));
        // (the round's bytes with this engine's 64 of slack behind every scratch block; the painting owns whole dwords)
        EKF(S.masks(f_mask || rf_plain ? f_mask + rf_plain + (rf_n ? 4 : 0) + 64 : 0, f_mask ? f_mask + 64 : 0));
        if (rf_n) {
            refill_block(rneed, rf_n, rf_trk);
            EKF(S.refill(rf_trk + 4, rf_n, rneed.bytes()));
            Carve rc = carve_of(S.h_refill);
            T = refill_block(rc, rf_n, rf_trk);
        }
        Carve c = carve_of(S.h_gfr);
        size_t mpos = 0, ibase = 0;
        for (Group& g : groups) {
            g.B = gftt_frame_block(c, g.reqs.size(), (size_t)g.key->max_per_cell);
            g.info_base = ibase; ibase += g.reqs.size();
            for (size_t i = 0; i < g.reqs.size(); i++) {
                DetReq* r = g.reqs[i];
                if (r->refill && r->mask) mpos = (mpos + 3) & ~(size_t)3;   // (the painting owns aligned dwords of a refill request's bytes)
                const size_t m0 = mpos;
                mpos = gftt_frame_record(g.B.rec.h + i * CELL_STRIDE, r->roi, r->slot, r->list_off, S.h_gfr_mask, mpos, r->mask, r->mask_stride);
                if (r->refill && r->mask) { ctx->refill_stats[3] += (long long)(mpos - m0); mpos = (mpos + 3) & ~(size_t)3; }
            }
        }
        if (mpos) EKF(hipMemcpyAsync(S.d_gfr_mask, S.h_gfr_mask, mpos, hipMemcpyHostToDevice, s));
        if (rf_n) {   // the regions painted from 255 follow the uploaded bytes; then ONE select and ONE paint launch for the round's refill requests
            size_t ppos = (mpos + 3) & ~(size_t)3, ri = 0;
            for (Group& g : groups)
                for (size_t i = 0; i < g.reqs.size(); i++) {
                    DetReq* r = g.reqs[i];
                    if (!r->refill) continue;
                    int* rec = g.B.rec.h + i * CELL_STRIDE;
                    if (!r->mask) { rec[5] = (int)ppos; ppos += ((size_t)r->roi[2] * r->roi[3] + 3) & ~(size_t)3; }
                    refill_fill(T, ri++, r->trk_off, r->roi, (size_t)(unsigned)rec[5], r->trk_xy, r->trk_prio, r->n_trk, r->radius, r->mask, r->mask_stride);
                }
            EKF(launch_track_refill(s, T.rec.d, (int)rf_n, rf_max, T.pos.d, T.prio.d, T.flag.d, T.hw.d, T.keep.d, S.d_refill_kept, S.d_refill_nkept, S.d_gfr_mask));
            ctx->refill_stats[1]++; ctx->refill_stats[2]++;
        }
        for (Group& g : groups) {
            const DetReq* k = g.key;
            const GfttExt X = gftt_ext(k->block_size, k->use_harris, k->k);
            EKF(launch_gftt_frame(s, ctx->d_slots, g.L, g.B.rec.d, (int)g.reqs.size(), g.grid_x, k->max_per_cell, k->quality, k->min_dist, k->unlimited, k->ext ? &X : nullptr,
                                  k->has_mask() ? S.d_gfr_mask.get() : nullptr, S.d_gfr_val, S.d_gfr_idx, S.d_gfr_info + 2 * g.info_base, S.d_gfr_keys, g.B.xy.d, g.B.count.d,
                                  g.B.stats.d));
            ctx->gftt_frame_stats[2]++;
        }
        ctx->gftt_frame_stats[1]++;
        return true;
    }
    void collect() {
        for (Group& g : groups)
            for (size_t i = 0; i < g.reqs.size(); i++) {
                DetReq* r = g.reqs[i];
                const int n = g.B.count.h[i];
                ctx->gftt_frame_stats[3] = g.B.stats.h[2 * i]; ctx->gftt_frame_stats[4] = g.B.stats.h[2 * i + 1];   // (of the last request served)
                if (n < 0) { r->rc = PMV_ERR_OVERFLOW; snprintf(r->err, sizeof(r->err), "%s: more than out_cap = %d corners with max_corners <= 0 (no limit)", r->refill ? "pmv_batch_detect_gftt_refill" : "pmv_batch_detect_gftt_frame", r->max_per_cell); continue; }
                if (r->refill) memcpy(r->out_keep, T.keep.h + r->trk_off, (size_t)r->n_trk);
                memcpy(r->out_xy, g.B.xy.h + i * (size_t)r->max_per_cell * 2, (size_t)n * 8);
                *r->out_count = n;
            }
    }
};

// ---- corner sub-pixel refinement: requests that agree in the six parameters share ONE launch, whatever their slots and frame sizes -
// every point's record names its slot and its entry of the geometry table. The round's weight tables are its own (one per group).
struct DetSubpix {
    struct Group { pmv_subpix_params p; std::vector<SubpixReq*> reqs; int n = 0, base = 0; };
    std::vector<SubpixReq*> reqs; std::vector<Group> groups;
    SubpixBlock S{};
    bool enqueue(BatchEngine* E, Combiner& C, std::vector<Req*>& batch) {
        pmv_ctx* ctx = E->ctx; hipStream_t s = C.s;
        size_t total = 0;
        for (SubpixReq* r : reqs) {
            if (!admit_frames(ctx, r, "corner subpix", r->slot, -1, &r->geom)) continue;
            if (total + (size_t)r->n > E->cap_tracks) { r->rc = PMV_ERR_CAPACITY; snprintf(r->err, sizeof(r->err), "batch corner subpix: more points than n_seq * max_tracks in a round"); continue; }
            Group* g = nullptr;
            for (Group& x : groups)
                if (x.p.win_w == r->p.win_w && x.p.win_h == r->p.win_h && x.p.zero_w == r->p.zero_w && x.p.zero_h == r->p.zero_h && x.p.max_iter == r->p.max_iter && x.p.eps == r->p.eps) { g = &x; break; }
            if (!g) { groups.push_back(Group{r->p, {}, 0, 0}); g = &groups.back(); }
            g->reqs.push_back(r); g->n += r->n; total += (size_t)r->n;
        }
        if (total == 0) { groups.clear(); return true; }
        const size_t tab_bytes = groups.size() * SUBPIX_TABLE_MAX * sizeof(float);
        Carve spx_need;
        subpix_block(spx_need, total);
        EKF(C.h_spx.ensure(spx_need.bytes() + 64)); EKF(C.h_spx_tab.ensure(tab_bytes)); EKF(C.d_spx_tab.ensure(tab_bytes));
        Carve c = carve_of(C.h_spx);
        S = subpix_block(c, total);
        SubpixRec* rec = S.rec.h;
        int pos = 0;
        for (size_t gi = 0; gi < groups.size(); gi++) {
            Group& g = groups[gi];
            g.base = pos;
            for (SubpixReq* r : g.reqs) {
                r->base = pos;
                for (int i = 0; i < r->n; i++) rec[pos++] = SubpixRec{r->xy[2 * i], r->xy[2 * i + 1], r->slot, r->geom};
            }
            subpix_table(g.p.win_w, g.p.win_h, g.p.zero_w, g.p.zero_h, (float*)C.h_spx_tab.p + gi * SUBPIX_TABLE_MAX);
        }
        EKF(hipMemcpyAsync(C.d_spx_tab.p, C.h_spx_tab.p, tab_bytes, hipMemcpyHostToDevice, s));
        for (size_t gi = 0; gi < groups.size(); gi++) {
            const Group& g = groups[gi];
            const SubpixArgs A{g.p.win_w, g.p.win_h, g.p.max_iter, g.p.eps * g.p.eps};
            EKF(launch_corner_subpix_geom(s, ctx->d_slots, ctx->d_geom, S.rec.d + g.base, g.n, (const float*)C.d_spx_tab.p + gi * SUBPIX_TABLE_MAX, A,
                                          S.xy.d + 2 * (size_t)g.base, S.iters.d + g.base, S.flags.d + g.base));
            ctx->subpix_launches[2]++;
        }
        ctx->subpix_launches[1]++;
        return true;
    }
    void collect() {
        for (Group& g : groups)
            for (SubpixReq* r : g.reqs) {
                memcpy(r->xy, S.xy.h + (size_t)2 * r->base, (size_t)r->n * 8);
                if (r->iters_out) memcpy(r->iters_out, S.iters.h + r->base, (size_t)r->n);
                if (r->flags_out) memcpy(r->flags_out, S.flags.h + r->base, (size_t)r->n);
            }
    }
};
#undef EKF

void process_det(BatchEngine* E, Combiner& C, std::vector<Req*>& batch) {
    DetCells cells; DetFrames frames; DetSubpix subpix;
    for (Req* r : batch) { if (r->kind == Q_SUBPIX) subpix.reqs.push_back((SubpixReq*)r); else if (r->kind == Q_GFTT_FRAME) frames.reqs.push_back((DetReq*)r); else cells.reqs.push_back((DetReq*)r); }
    if (!cells.enqueue(E, C, batch) || !frames.enqueue(E, C, batch) || !subpix.enqueue(E, C, batch)) return;
    SYNC_TIMED(C);
    subpix.collect();
    frames.collect();   // (gftt_frame_stats[3..4]: the last request served)
    cells.collect();
}

// ---- back-end classes: the callers prepared their inputs in their slot's pinned block; one gather kernel pulls them into HBM ----
// Descriptor block of a batch in mapped pinned memory: [problem records | problem records of a second kind (process_whole) | stage-in jobs],
// each part at a multiple of 256 bytes. No DMA call is made: k_stage_in reads
// its job list through the host alias; job 0 copies the problem records into device memory (the back-end chains read them in every
// launch), jobs 1..n pull the requests' input blocks. (A hipMemcpyAsync is a blit kernel of its own: 83 k of them, 15 us each in
// stream time, in a B = 64 run before this.)
template <class A, class B> struct DescBlock { Carved<A> a; Carved<B> b; Carved<StageJob> jobs; size_t rec_bytes, bytes; };   // .d: records in d_desc, jobs through the mapped alias
template <class A, class B> DescBlock<A, B> desc_carve(Carve c, size_t na, size_t nb) {
    DescBlock<A, B> D;
    D.a = c.take<A>(na); D.rec_bytes = c.bytes();
    D.b = c.take<B>(nb, 256); if (nb) D.rec_bytes = c.bytes();   // (the end of the last record: what job 0 copies)
    D.jobs = c.take<StageJob>(1 + na + nb, 256);
    D.bytes = c.bytes();
    return D;
}
template <class A, class B = char>
hipError_t desc_block(Combiner& C, size_t na, size_t nb, DescBlock<A, B>& D) {
    D = desc_carve<A, B>(Carve(), na, nb);   // (dry run: the sizes)
    hipError_t e = C.h_desc.ensure(D.bytes + 256);
    if (e != hipSuccess) return e;
    e = C.d_desc.ensure(D.jobs.off + 256);
    if (e != hipSuccess) return e;
    D = desc_carve<A, B>(Carve(C.h_desc.p, C.d_desc.p, C.h_desc.cap), na, nb);
    D.jobs.d = (StageJob*)(C.h_desc.dev + D.jobs.off);
    D.jobs.h[0] = StageJob{C.h_desc.dev, (char*)C.d_desc.p, (unsigned)D.rec_bytes, 0};   // job 0: the records themselves
    D.jobs.h += 1;   // the callers fill jobs 1..n
    return hipSuccess;
}
template <class A, class B>
hipError_t stage_in(Combiner& C, const DescBlock<A, B>& D, size_t n, int blocks_per_job) {
    hipLaunchKernelGGL(k_stage_in, dim3(blocks_per_job, (unsigned)(n + 1)), dim3(256), 0, C.s, D.jobs.d);
    return hipGetLastError();
}

void process_pnp(BatchEngine* E, Combiner& C, std::vector<Req*>& batch) {
    DescBlock<PnPProblem, char> D;
    EK(desc_block(C, batch.size(), 0, D));
    int max_hyp = 0;
    for (size_t i = 0; i < batch.size(); i++) {
        PnPReq* r = (PnPReq*)batch[i];
        D.a.h[i] = r->P;
        D.jobs.h[i] = StageJob{(const char*)r->b->h_stage.dm(), r->b->d_pnp_in, (unsigned)r->L.in_bytes, 0};
        max_hyp = std::max(max_hyp, r->P.n_hyp);
    }
    EK(stage_in(C, D, batch.size(), 2));
    EK(launch_pnp_batch(C.s, D.a.d, (int)batch.size(), max_hyp));
    SYNC_TIMED(C);   // the refit kernel wrote every result straight into the request's pinned block
}

void process_ba(BatchEngine* E, Combiner& C, std::vector<Req*>& batch) {
    if (E->ctx->ba_mode == 1) {   // one workgroup per problem: ONE launch for the whole round (pmv_set_ba_mode)
        DescBlock<BAArgs, char> D;
        EK(desc_block(C, batch.size(), 0, D));
        int max_m = 6;
        for (size_t i = 0; i < batch.size(); i++) {
            BAReq* r = (BAReq*)batch[i];
            D.a.h[i] = r->A;
            D.jobs.h[i] = StageJob{(const char*)r->b->h_stage.dm(), r->b->d_ba_io, (unsigned)r->L.io_bytes, 0};
            max_m = std::max(max_m, 6 * r->A.nc);
        }
        EK(stage_in(C, D, batch.size(), 8));
        EK(launch_ba_lm_batch(C.s, D.a.d, (int)batch.size(), max_m));
        SYNC_TIMED(C);
        return;
    }
    // one launch chain per distinct iteration cap (in practice one)
    std::vector<int> iters;
    for (Req* q : batch) { const int it = ((BAReq*)q)->max_iterations; if (std::find(iters.begin(), iters.end(), it) == iters.end()) iters.push_back(it); }
    std::vector<BAReq*> sorted;
    for (int it : iters) for (Req* q : batch) if (((BAReq*)q)->max_iterations == it) sorted.push_back((BAReq*)q);
    DescBlock<BAProb, char> D;
    EK(desc_block(C, sorted.size(), 0, D));
    for (size_t i = 0; i < sorted.size(); i++) {
        BAReq* r = sorted[i];
        ba_fill_prob(D.a.h[i], r->A, r->b->d_bastate, r->b->d_bapart);
        D.jobs.h[i] = StageJob{(const char*)r->b->h_stage.dm(), r->b->d_ba_io, (unsigned)r->L.io_bytes, 0};
    }
    EK(stage_in(C, D, sorted.size(), 8));
    size_t i0 = 0;
    for (int it : iters) {
        BABatchDims dims{0, 0, 0, 0, 0, 0, it};
        size_t i1 = i0;
        while (i1 < sorted.size() && sorted[i1]->max_iterations == it) {
            const BAProb& P = D.a.h[i1];
            dims.max_eval_blocks = std::max(dims.max_eval_blocks, P.nbo + P.clear_blocks);
            dims.max_nc = std::max(dims.max_nc, P.A.nc); dims.max_nbp = std::max(dims.max_nbp, P.nbp); dims.max_tiles = std::max(dims.max_tiles, P.tiles);
            dims.max_m = std::max(dims.max_m, 6 * P.A.nc);
            i1++;
        }
        dims.n_probs = (int)(i1 - i0);
        EK(launch_ba_multi_batch(C.s, D.a.d + i0, dims));
        i0 = i1;
    }
    SYNC_TIMED(C);
}

// The two-view requests of a round share ONE k_tri_dlt_batch launch, its N-view requests (Q_TRI_TRACKS) ONE k_tri_tracks_batch launch behind
// it, both behind one k_stage_in launch: the descriptor block is desc_block's with both kinds of records.
void process_dlt(BatchEngine* E, Combiner& C, std::vector<Req*>& batch) {
    std::vector<DltReq*> dlt; std::vector<TriTracksReq*> tt;
    for (Req* r : batch) { if (r->kind == Q_TRI_TRACKS) tt.push_back((TriTracksReq*)r); else dlt.push_back((DltReq*)r); }
    const size_t nd = dlt.size(), nt = tt.size();
    DescBlock<DltProblem, TriTracksProblem> D;
    EK(desc_block(C, nd, nt, D));
    int max_n = 0, max_np = 0;
    for (size_t i = 0; i < nd; i++) {
        DltReq* r = dlt[i];
        D.a.h[i] = r->P;
        D.jobs.h[i] = StageJob{(const char*)r->b->h_stage.dm(), r->b->d_tri_in, (unsigned)r->L.in_bytes, 0};
        max_n = std::max(max_n, r->P.n);
    }
    for (size_t i = 0; i < nt; i++) {
        TriTracksReq* r = tt[i];
        D.b.h[i] = r->P;
        D.jobs.h[nd + i] = StageJob{(const char*)r->b->h_stage.dm(), r->b->d_tt_in, (unsigned)r->L.in_bytes, 0};
        max_np = std::max(max_np, r->P.np);
    }
    EK(stage_in(C, D, nd + nt, 2));
    EK(launch_tri_dlt_batch(C.s, D.a.d, (int)nd, max_n));
    EK(launch_tri_tracks_batch(C.s, D.b.d, (int)nt, max_np));
    if (nt) { E->ctx->tri_tracks_launches[0]++; E->ctx->tri_tracks_launches[1] += (long long)nt; }
    SYNC_TIMED(C);
}

void process_fp_rounds(BatchEngine* E, Combiner& C, std::vector<Req*>& batch) {
    DescBlock<FivePointProblem, char> D;
    EK(desc_block(C, batch.size(), 0, D));
    int max_hyp = 0;
    for (size_t i = 0; i < batch.size(); i++) {
        FPReq* r = (FPReq*)batch[i];
        D.a.h[i] = r->P;
        D.jobs.h[i] = StageJob{(const char*)r->b->h_stage.dm(), r->b->d_tri_in, (unsigned)r->L.in_bytes, 0};
        max_hyp = std::max(max_hyp, r->P.n_hyp);
    }
    EK(stage_in(C, D, batch.size(), 2));
    EK(launch_fivepoint_batch(C.s, D.a.d, (int)batch.size(), max_hyp));
    SYNC_TIMED(C);
}

// whole findEssentialMat and findFundamentalMat calls: ONE k_essential_ransac launch for the round's requests of the first kind, ONE
// k_fundamental_ransac launch for those of the second, one workgroup per request, behind one k_stage_in launch for both. The descriptor block
// is desc_block's with both kinds of records. The fundamental launch goes first: its requests take a fraction
// of a five-point request's time and would otherwise wait on the stream behind all of them. Each workgroup signals its own caller; the sync
// below is the fallback (a failed launch releases everyone with an error) and what makes the records reusable.
// The round's findHomography requests have the fundamental requests' record and blocks: they stand behind them in the same array and get
// ONE k_homography_ransac launch, between the other two.
void process_whole(BatchEngine* E, Combiner& C, std::vector<Req*>& batch) {
    std::vector<EssReq*> ess; std::vector<FundReq*> fund, homog;
    for (Req* r : batch) { if (r->kind == Q_ESSENTIAL) ess.push_back((EssReq*)r); else (r->kind == Q_HOMOGRAPHY ? homog : fund).push_back((FundReq*)r); }
    const size_t ne = ess.size(), nf = fund.size(), nh = homog.size();
    fund.insert(fund.end(), homog.begin(), homog.end());
    DescBlock<EssentialProblem, FundamentalProblem> D;
    EK(desc_block(C, ne, nf + nh, D));
    for (size_t i = 0; i < ne; i++) {
        D.a.h[i] = ess[i]->P;
        D.jobs.h[i] = StageJob{(const char*)ess[i]->b->h_stage.dm(), ess[i]->b->d_ess_in, (unsigned)ess[i]->L.in_bytes, 0};
    }
    for (size_t i = 0; i < nf + nh; i++) {
        D.b.h[i] = fund[i]->P;
        D.jobs.h[ne + i] = StageJob{(const char*)fund[i]->b->h_stage.dm(), fund[i]->b->d_fund_in, (unsigned)fund[i]->L.in_bytes, 0};
    }
    EK(stage_in(C, D, ne + nf + nh, 2));
    EK(launch_fundamental_ransac(C.s, D.b.d, (int)nf));
    EK(launch_homography_ransac(C.s, D.b.d + nf, (int)nh));
    EK(launch_essential_ransac(C.s, D.a.d, (int)ne));
    if (nh) { E->ctx->homography_launches[0]++; E->ctx->homography_launches[1] += (long long)nh; }
    if (nf) E->ctx->whole_rounds[0]++;
    if (ne) E->ctx->whole_rounds[1]++;
    if (nf && ne) E->ctx->whole_rounds[2]++;
    SYNC_TIMED(C);
}

void process_fp(BatchEngine* E, Combiner& C, std::vector<Req*>& batch) {
    std::vector<Req*> rounds, whole;   // (the forms share the class; a round that holds both serves them one after the other)
    for (Req* r : batch) (r->kind >= Q_WHOLE_FIRST ? whole : rounds).push_back(r);
    if (!rounds.empty()) process_fp_rounds(E, C, rounds);
    if (!whole.empty()) process_whole(E, C, whole);
}

// The result blocks of a lane hold cap_tracks = B * max_tracks tracks (LK, kNN) or points (sub-pixel). The B sequences of a batched run never
// ask for more; the callers of a batch session may (any number of threads): a round takes the requests that fit, in arrival order, and the
// rest stay at the head of the queue for the next round (one request is at most max_tracks, so a round is never empty). weight(r): what a
// request takes of the block. Called under Q's mutex.
template <class Weight> void take_what_fits(Queue* Q, std::vector<Req*>& batch, size_t cap, Weight weight) {
    size_t total = 0, k = 0;
    for (; k < batch.size(); k++) {
        const size_t n = weight(batch[k]);
        if (total + n > cap) break;
        total += n;
    }
    if (k == batch.size()) return;
    Q->pending.assign(batch.begin() + (long)k, batch.end());
    batch.resize(k);
    Q->first_arrival = std::chrono::steady_clock::now();
    Q->cv_new.notify_all();   // (another lane of the class may take them at once)
}

void combiner_loop(BatchEngine* E, int role, int lane) {
    Combiner* C = &E->comb[role][lane];
    Queue* Q = &E->queue[role];
    (void)hipSetDevice(E->ctx->device);
    tl_prof = &E->ctx->prof;
    (void)prctl(PR_SET_TIMERSLACK, 1000UL, 0, 0, 0);   // 1 us instead of the default 50 us: the timed sleeps of wait_stream
    for (;;) {
        std::vector<Req*> batch;
        const auto ti = std::chrono::steady_clock::now();
        {
            std::unique_lock<std::mutex> lk(Q->mu);
            Q->cv_new.wait(lk, [&] { return !Q->pending.empty() || Q->stop; });
            if (Q->pending.empty() && Q->stop) return;
            if (E->min_batch[role] > 1 && (int)Q->pending.size() < E->min_batch[role] && !Q->stop) {
                const auto deadline = Q->first_arrival + std::chrono::microseconds(E->max_linger_us);
                Q->cv_new.wait_until(lk, deadline, [&] { return (int)Q->pending.size() >= E->min_batch[role] || Q->stop; });
                if (Q->pending.empty()) { if (Q->stop) return; continue; }   // another lane of the class took them meanwhile
            }
            if (E->linger_us > 0 && (int)Q->pending.size() < E->B) {   // optional: give stragglers a moment to join the batch
                lk.unlock();
                std::this_thread::sleep_for(std::chrono::microseconds(E->linger_us));
                lk.lock();
                if (Q->pending.empty()) { if (Q->stop) return; continue; }   // another lane of the class lingered too and took them: no empty round
            }
            batch.swap(Q->pending);
            if (role == R_LK) take_what_fits(Q, batch, E->cap_tracks, [](Req* r) { return r->kind == Q_KNN ? (size_t)((KnnReq*)r)->n : (size_t)((LKReq*)r)->n; });
            if (role == R_DET) take_what_fits(Q, batch, E->cap_tracks, [](Req* r) { return r->kind == Q_SUBPIX ? (size_t)((SubpixReq*)r)->n : (size_t)0; });
        }
        const auto tw = std::chrono::steady_clock::now();
        C->t_idle += std::chrono::duration<double>(tw - ti).count();
        // diagnostic (PMV_BATCH_EXCLUSIVE=1): one class on the GPU at a time, so a round's duration is that of its kernels alone
        std::unique_lock<std::mutex> excl(E->exclusive_mu, std::defer_lock);
        if (E->exclusive) excl.lock();
        switch (role) {
        case R_LK: process_lk(E, *C, batch); break;
        case R_DET: process_det(E, *C, batch); break;
        case R_PNP: process_pnp(E, *C, batch); break;
        case R_BA: process_ba(E, *C, batch); break;
        case R_DLT: process_dlt(E, *C, batch); break;
        default: process_fp(E, *C, batch); break;
        }
        if (E->exclusive) excl.unlock();
        C->batches++; C->requests += (long)batch.size();
        for (Req* r : batch) {
            std::atomic<int>* w = &r->done;   // (after the store the owner may return and the request, which lives on its stack, is gone)
            const bool engine_owned = r->kind >= Q_WHOLE_FIRST && r->kind <= Q_WHOLE_LAST;
            w->store(1, std::memory_order_release);
            futex_wake_one(w);
            if (engine_owned) {   // the record may be filled again from here on
                std::atomic<int>* f = &((WholeReq*)r)->inflight;
                f->store(0, std::memory_order_release);
                futex_wake_one(f);
            }
        }
        C->t_work += std::chrono::duration<double>(std::chrono::steady_clock::now() - tw).count();
        { timespec ts; clock_gettime(CLOCK_THREAD_CPUTIME_ID, &ts); C->t_cpu = ts.tv_sec + 1e-9 * ts.tv_nsec; }
    }
}

void enqueue(Queue& Q, Req* r) {
    std::lock_guard<std::mutex> lk(Q.mu);
    if (Q.pending.empty()) Q.first_arrival = std::chrono::steady_clock::now();
    Q.pending.push_back(r);
    const int sz = (int)Q.pending.size();
    if (sz == 1) Q.cv_new.notify_one();
    else if (Q.min_batch <= 1 || sz == Q.min_batch) Q.cv_new.notify_all();   // (a lingering combiner is waiting for exactly this)
}

int submit(pmv_ctx* ctx, Queue& Q, Req* r) {
    enqueue(Q, r);
    futex_wait_while(&r->done, 0);
    if (r->rc != PMV_OK) set_err(ctx, "%s", r->err);
    return r->rc;
}

}  // namespace

#define CKC(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { set_err(ctx, "%s: %s", #x, hipGetErrorString(e_)); return PMV_ERR_HIP; } } while (0)
#define REQ(cond, code, ...) do { if (!(cond)) { set_err(ctx, __VA_ARGS__); return code; } } while (0)

void batch_engine_destroy(pmv_ctx* ctx) {
    BatchEngine* E = ctx->engine;
    if (!E) return;
    for (Queue& Q : E->queue) {
        { std::lock_guard<std::mutex> lk(Q.mu); Q.stop = true; }
        Q.cv_new.notify_all();
    }
    for (auto& role : E->comb)
        for (Combiner& C : role)
            if (C.th.joinable()) C.th.join();   // all of them first: lanes of a class may share a stream
    for (auto& role : E->comb)
        for (Combiner& C : role) {
            if (getenv("PMV_BATCH_TIMING") && C.batches)
                fprintf(stderr, "[batch-timing] class %d lane %d: %ld rounds, %.1f req/round, per round: work %.0f us, sync %.0f us (first sleep %.0f us, then %.1f polls), cpu %.0f us, ema %.0f us\n",
                        (int)(&role - &E->comb[0]), (int)(&C - &role[0]), C.batches, (double)C.requests / C.batches, C.t_work / C.batches * 1e6, C.t_sync / C.batches * 1e6,
                        C.sig_diag.t_first_sleep / C.batches * 1e6, (double)C.sig_diag.n_polls / C.batches, C.t_cpu / C.batches * 1e6, C.sig.ema_us);
            if (C.s && C.owns_stream) { (void)hipStreamSynchronize(C.s); (void)hipStreamDestroy(C.s); }
            if (C.ev) (void)hipEventDestroy(C.ev);
        }
    for (BackendBuffers* b : E->slots) backend_free(b);
    delete E;   // the combiners' buffers go with it: their threads are joined and their streams idle
    ctx->engine = nullptr;
}

int batch_engine_get(pmv_ctx* ctx, int B, BatchEngine** out) {
    REQ(B >= 1 && B <= 256, PMV_ERR_CAPACITY, "batch size %d (1..256)", B);
    if (ctx->engine && ctx->engine->B >= B) { *out = ctx->engine; return PMV_OK; }
    batch_engine_destroy(ctx);
    CKC(hipSetDevice(ctx->device));
    BatchEngine* E = new BatchEngine();
    ctx->engine = E;
    E->ctx = ctx; E->B = B;
    if (const char* e = getenv("PMV_BATCH_LINGER_US")) E->linger_us = atoi(e);
    {
        const double frac = getenv("PMV_BATCH_MIN_FRAC") ? atof(getenv("PMV_BATCH_MIN_FRAC")) : 0.12;   // of the B sequences, per class with long rounds
        if (const char* e = getenv("PMV_BATCH_MAX_LINGER_US")) E->max_linger_us = atoi(e);
        for (int r : {(int)R_LK, (int)R_PNP, (int)R_BA}) { E->min_batch[r] = (int)(frac * B); E->queue[r].min_batch = E->min_batch[r]; }
    }
    for (int i = 0; i < B; i++) {
        BackendBuffers* b = nullptr;
        const int rc = backend_alloc(ctx, &b);
        if (b) E->slots.push_back(b);
        if (rc != PMV_OK) { batch_engine_destroy(ctx); return rc; }
    }
    E->ess.reset(new EssReq[(size_t)B]);
    E->fund.reset(new FundReq[(size_t)B]);
    E->homog.reset(new FundReq[(size_t)B]);
    E->cap_tracks = (size_t)B * ctx->max_tracks;
    if (const char* e = getenv("PMV_BATCH_EXCLUSIVE")) E->exclusive = atoi(e) != 0;
    if (const char* e = getenv("PMV_LK_LPT")) E->lk_lpt = atoi(e) != 0;
    E->lanes[R_LK] = 2;   // (measured, B = 128: see DESIGN.md §5)
    E->lanes[R_BA] = 2;   // (B = 192, profiles/r03_batch_exp_ae.log: 64.8 k -> 67.6 k frames/s; three lanes: 52 k)
    if (const char* e = getenv("PMV_BATCH_LANES")) for (int& l : E->lanes) l = std::max(1, std::min(MAX_LANES, atoi(e)));
    if (const char* e = getenv("PMV_BATCH_LANES_LK")) E->lanes[R_LK] = std::max(1, std::min(MAX_LANES, atoi(e)));
    if (const char* e = getenv("PMV_BATCH_LANES_PNP")) E->lanes[R_PNP] = std::max(1, std::min(MAX_LANES, atoi(e)));
    if (const char* e = getenv("PMV_BATCH_LANES_BA")) E->lanes[R_BA] = std::max(1, std::min(MAX_LANES, atoi(e)));
    if (const char* e = getenv("PMV_BATCH_LANES_FP")) E->lanes[R_FP] = std::max(1, std::min(MAX_LANES, atoi(e)));
    if (const char* e = getenv("PMV_BATCH_STREAMS_LK")) E->streams[R_LK] = atoi(e);
    if (const char* e = getenv("PMV_BATCH_STREAMS_BA")) E->streams[R_BA] = atoi(e);
    if (const char* e = getenv("PMV_BATCH_STREAMS_PNP")) E->streams[R_PNP] = atoi(e);
    if (const char* e = getenv("PMV_BATCH_WAIT")) E->wait_mode = !strcmp(e, "spin") ? 0 : !strcmp(e, "yield") ? 1 : !strcmp(e, "block") ? 2 : 3;
    for (int r = 0; r < R_COUNT; r++)
        for (int l = 0; l < E->lanes[r]; l++) {
            Combiner& C = E->comb[r][l];
            // the back-end classes are chains of small launches (a BA solve: 23 of them): they get the higher stream priority so their
            // workgroups are not queued behind the thousands of LK / detector waves of the front-end classes (PMV_BATCH_PRIO=0: all equal)
            int prio_lo = 0, prio_hi = 0;
            (void)hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);   // numerically lower = higher priority
            static const bool use_prio = !(getenv("PMV_BATCH_PRIO") && atoi(getenv("PMV_BATCH_PRIO")) == 0);
            const int prio = !use_prio ? prio_lo : (r == R_BA || r == R_PNP || r == R_DLT) ? prio_hi : prio_lo;
            // (measured and dropped: confining the back-end classes to 64 / 96 CUs with hipExtStreamCreateWithCUMask: 25.4 k -> 16.2 k / 21.3 k
            // frames/s at B = 64 - the PnP hypotheses need the whole chip; equal priorities: no difference either)
            const int n_streams = E->streams[r] > 0 ? std::min(E->streams[r], E->lanes[r]) : E->lanes[r];
            if (l < n_streams) CKC(hipStreamCreateWithPriority(&C.s, hipStreamNonBlocking, prio));
            else { C.s = E->comb[r][l % n_streams].s; C.owns_stream = false; }
            CKC(hipEventCreateWithFlags(&C.ev, hipEventBlockingSync | hipEventDisableTiming));
            CKC(C.sig.init());
            if (r == R_LK) { CKC(C.h_out_xy.ensure(E->cap_tracks * 8)); CKC(C.h_status.ensure(E->cap_tracks)); CKC(C.h_err.ensure(E->cap_tracks * 4)); CKC(C.h_work.ensure(E->cap_tracks * 2)); }
            if (r == R_DET) CKC(C.d_flags.ensure(16));
        }
    for (int r = 0; r < R_COUNT; r++)
        for (int l = 0; l < E->lanes[r]; l++) E->comb[r][l].th = std::thread(combiner_loop, E, r, l);
    *out = E;
    return PMV_OK;
}

void batch_engine_stats(BatchEngine* E, long long* counts10, double* times15) {
    for (int r = 0; r < 5; r++) {   // the five classes every run uses; the optional five-point class is reported separately

        counts10[2 * r] = counts10[2 * r + 1] = 0;
        if (times15) times15[3 * r] = times15[3 * r + 1] = times15[3 * r + 2] = 0;
        for (int l = 0; l < E->lanes[r]; l++) {   // summed over the class's combiners
            const Combiner& C = E->comb[r][l];
            counts10[2 * r] += C.batches; counts10[2 * r + 1] += C.requests;
            if (times15) { times15[3 * r] += C.t_cpu; times15[3 * r + 1] += C.t_work; times15[3 * r + 2] += C.t_sync; }
        }
    }
}

// ---- request entry points (called from the sequences' own host threads) ---------------------------------------------------------
int engine_lk(BatchEngine* E, int prev_slot, int next_slot, const float* prev_xy, int n, float* out_xy, uint8_t* status, float* err,
              const uint8_t* predicted_iters, uint8_t* iters_out, int ring_round) {
    pmv_ctx* ctx = E->ctx;
    if (const int rc = lk_check(ctx, false, prev_slot, next_slot, prev_xy, n, out_xy, status, err)) return rc;
    if (n == 0) return PMV_OK;
    LKReq r;
    r.kind = Q_LK; r.prev_slot = prev_slot; r.next_slot = next_slot; r.n = n; r.prev_xy = prev_xy; r.out_xy = out_xy; r.status = status; r.err_out = err;
    r.iters_out = iters_out;
    r.ring_round = ring_round;
    if (E->lk_lpt) {
        // most expensive first: a counting sort on the predicted iteration count (255 .. 0), ties in track order
        r.order.resize((size_t)n);
        int cnt[257] = {0};
        for (int i = 0; i < n; i++) cnt[256 - (predicted_iters ? predicted_iters[i] : 0)]++;   // bucket b = 255 - pred, offset by one for the prefix
        for (int b = 1; b <= 256; b++) cnt[b] += cnt[b - 1];
        for (int i = 0; i < n; i++) r.order[(size_t)cnt[255 - (predicted_iters ? predicted_iters[i] : 0)]++] = i;
        return submit(ctx, E->queue[R_LK], &r);
    }
    // the same XCD-aware dealing as pmv_lk_track (stripe s of the x-sorted tracks -> blocks 8k + s); a request's block range starts at
    // a multiple of 8 in the concatenated launch, so block % 8 (= XCD) is preserved
    r.order.resize((size_t)((n + 7) / 8 * 8));
    lk_xcd_order(prev_xy, n, r.order.data());
    return submit(ctx, E->queue[R_LK], &r);
}

int engine_lk_ex(BatchEngine* E, const char* who, int prev_slot, int next_slot, const float* prev_xy, int n, float* next_xy, int flags, uint8_t* status,
                 float* err, bool fb, float* back_xy, uint8_t* back_status, float* back_err) {
    pmv_ctx* ctx = E->ctx;
    if (const int rc = lkx_check(ctx, who, false, prev_slot, next_slot, prev_xy, n, next_xy, flags, status, err, fb, back_xy, back_status, back_err)) return rc;
    if (n == 0) return PMV_OK;
    LKReq r;
    r.kind = Q_LK_EX; r.prev_slot = prev_slot; r.next_slot = next_slot; r.n = n; r.prev_xy = prev_xy; r.out_xy = next_xy; r.status = status; r.err_out = err;
    r.flags = (flags & (LKX_INIT | LKX_EIG)) | (fb ? LKX_FB : 0);
    r.back_xy = back_xy; r.back_status = back_status; r.back_err = back_err;
    return submit(ctx, E->queue[R_LK], &r);
}

// a GFTT or ShiTomasi request as every form of the call makes it; max_per_cell <= 0: no limit (GFTT)
static void det_fill(DetReq& r, ReqKind kind, int slot, const int* cells, int n_cells, int max_per_cell, double quality, double min_dist, int* out_xy,
                     double* out_score, int* out_count, int ring_round) {
    r.kind = kind; r.slot = slot; r.cells = cells; r.n_cells = n_cells; r.unlimited = max_per_cell <= 0;
    r.max_per_cell = r.unlimited ? MAX_PER_CELL : max_per_cell;
    r.quality = quality; r.min_dist = min_dist; r.out_xy = out_xy; r.out_score = out_score; r.out_count = out_count;
    r.ring_round = ring_round;
}

int engine_detect(BatchEngine* E, ReqKind kind, int slot, const int* cells, int n_cells, int max_per_cell, double quality, double min_dist, int* out_xy,
                  double* out_score, int* out_count, int ring_round) {
    pmv_ctx* ctx = E->ctx;
    const bool st = kind == Q_SHITOMASI;
    if (st && max_per_cell <= 0) return shitomasi_nothing(ctx, cells, n_cells, out_count);
    if (const int rc = detect_check(ctx, false, slot, cells, n_cells, max_per_cell <= 0 ? MAX_PER_CELL : max_per_cell)) return rc;
    REQ(out_xy && out_count && (out_score || !st), PMV_ERR_INVALID, "%s: null output", st ? "pmv_detect_shitomasi" : "pmv_detect_gftt");
    DetReq r;
    det_fill(r, kind, slot, cells, n_cells, max_per_cell, quality, min_dist, out_xy, out_score, out_count, ring_round);
    return submit(ctx, E->queue[R_DET], &r);
}

int engine_detect_gftt_ex(BatchEngine* E, const char* who, int slot, const int* cells, int n_cells, int max_per_cell, const pmv_gftt_params* p,
                          const uint8_t* mask, int mask_stride, int* out_xy, int* out_count) {
    pmv_ctx* ctx = E->ctx;
    if (const int rc = gftt_ex_check(ctx, who, p, out_xy, out_count)) return rc;
    if (const int rc = detect_check(ctx, false, slot, cells, n_cells, max_per_cell <= 0 ? MAX_PER_CELL : max_per_cell)) return rc;
    if (const int rc = gftt_mask_check(ctx, who, slot, mask, mask_stride)) return rc;
    DetReq r;
    det_fill(r, Q_GFTT, slot, cells, n_cells, max_per_cell, p->quality, p->min_dist, out_xy, nullptr, out_count, -1);
    if (p->block_size != 3 || p->use_harris || mask || ctx->gftt_general) {   // (else: a plain GFTT request)
        r.ext = 1; r.block_size = p->block_size; r.use_harris = p->use_harris ? 1 : 0; r.k = p->use_harris ? p->k : 0.0;
        r.mask = mask; r.mask_stride = mask_stride;
    }
    return submit(ctx, E->queue[R_DET], &r);
}

int engine_detect_gftt_frame(BatchEngine* E, const char* who, int slot, const int* roi4_or_null, int max_corners, const pmv_gftt_params* p, const uint8_t* mask,
                             int mask_stride, int* out_xy, int out_cap, int* out_count) {
    pmv_ctx* ctx = E->ctx;
    DetReq r;
    int cap = 0;
    if (const int rc = gftt_frame_check(ctx, who, false, slot, roi4_or_null, max_corners, p, mask, mask_stride, out_xy, out_cap, out_count, r.roi, &cap)) return rc;
    r.kind = Q_GFTT_FRAME; r.slot = slot; r.cells = r.roi; r.n_cells = 1; r.unlimited = max_corners <= 0; r.max_per_cell = cap;
    r.quality = p->quality; r.min_dist = p->min_dist; r.out_xy = out_xy; r.out_score = nullptr; r.out_count = out_count; r.ring_round = -1;
    r.ext = p->block_size != 3 || p->use_harris || mask || ctx->gftt_general;   // the general pass-1 kernel, as in the single call
    r.block_size = p->block_size; r.use_harris = p->use_harris ? 1 : 0; r.k = p->use_harris ? p->k : 0.0;
    r.mask = mask; r.mask_stride = mask_stride;
    return submit(ctx, E->queue[R_DET], &r);
}

int engine_detect_gftt_refill(BatchEngine* E, const char* who, int slot, const int* roi4_or_null, int max_corners, const pmv_gftt_params* p, const float* track_xy,
                              const int* track_prio_or_null, int n_tracks, int radius, const uint8_t* base_mask_or_null, int base_stride, uint8_t* out_keep,
                              int* out_xy, int out_cap, int* out_count) {
    pmv_ctx* ctx = E->ctx;
    DetReq r;
    int cap = 0;
    if (const int rc = gftt_frame_check(ctx, who, false, slot, roi4_or_null, max_corners, p, base_mask_or_null, base_stride, out_xy, out_cap, out_count, r.roi, &cap)) return rc;
    if (const int rc = refill_check(ctx, who, slot, track_xy, n_tracks, radius, out_keep)) return rc;
    r.kind = Q_GFTT_FRAME; r.slot = slot; r.cells = r.roi; r.n_cells = 1; r.unlimited = max_corners <= 0; r.max_per_cell = cap;
    r.quality = p->quality; r.min_dist = p->min_dist; r.out_xy = out_xy; r.out_score = nullptr; r.out_count = out_count; r.ring_round = -1;
    r.ext = 1;   // there is a mask: the general pass-1 kernel, as in the single call
    r.block_size = p->block_size; r.use_harris = p->use_harris ? 1 : 0; r.k = p->use_harris ? p->k : 0.0;
    r.mask = base_mask_or_null; r.mask_stride = base_stride;
    r.refill = 1; r.n_trk = n_tracks; r.radius = radius; r.trk_xy = track_xy; r.trk_prio = track_prio_or_null; r.out_keep = out_keep;
    return submit(ctx, E->queue[R_DET], &r);
}

int engine_corner_subpix(BatchEngine* E, const char* who, int slot, float* xy, int n, const pmv_subpix_params* p, uint8_t* out_iters, uint8_t* out_flags) {
    pmv_ctx* ctx = E->ctx;
    if (const int rc = subpix_check(ctx, who, false, slot, xy, n, p)) return rc;
    if (n == 0) return PMV_OK;
    SubpixReq r;
    r.kind = Q_SUBPIX; r.slot = slot; r.n = n; r.xy = xy; r.iters_out = out_iters; r.flags_out = out_flags;
    r.p = *p;
    subpix_zero_zone(p, &r.p.zero_w, &r.p.zero_h);
    return submit(ctx, E->queue[R_DET], &r);
}

int engine_detect_fast(BatchEngine* E, int slot, const int* cells, int n_cells, int max_per_cell, int threshold, int nonmax, int* out_xy, float* out_response,
                       int* out_count, int ring_round) {
    pmv_ctx* ctx = E->ctx;
    int rc = fast_counts(ctx, cells, n_cells, max_per_cell, out_count);
    if (rc || max_per_cell <= 0) return rc;
    if ((rc = fast_check(ctx, false, slot, cells, n_cells, max_per_cell, out_xy, out_response))) return rc;
    DetReq r;
    r.kind = Q_FAST; r.slot = slot; r.cells = cells; r.n_cells = n_cells; r.unlimited = 0; r.max_per_cell = max_per_cell;
    r.quality = threshold; r.min_dist = nonmax ? 1 : 0;   // (the group key of process_det)
    r.out_xy = out_xy; r.out_score = nullptr; r.out_resp = out_response; r.out_count = out_count;
    r.ring_round = ring_round;
    return submit(ctx, E->queue[R_DET], &r);
}

int engine_knn(BatchEngine* E, int src_slot, int cmp_slot, const int* src_xy, int n, const int* cmp_xy, int m, int n_neighbours, int window, int* out_best,
               float* out_err, int ring_round) {
    pmv_ctx* ctx = E->ctx;
    if (const int rc = knn_check(ctx, false, src_slot, cmp_slot, src_xy, n, cmp_xy, m, n_neighbours, window, out_best, out_err)) return rc;
    if (n == 0) return PMV_OK;
    KnnReq r;
    r.kind = Q_KNN; r.src_slot = src_slot; r.cmp_slot = cmp_slot; r.n = n; r.m = m; r.n_nn = n_neighbours; r.window = window;
    r.src_xy = src_xy; r.cmp_xy = cmp_xy; r.out_best = out_best; r.err_out = out_err;
    r.ring_round = ring_round;
    return submit(ctx, E->queue[R_LK], &r);
}

int engine_pnp(BatchEngine* E, int seq, const float* obj_xyz, const float* img_xy, int m, const double* K, double* rvec, double* tvec, int iterations,
               float reproj_err, double confidence, int* out_inliers, int* out_n_inliers) {
    pmv_ctx* ctx = E->ctx;
    int rc = pnp_check(ctx, obj_xyz, img_xy, m, K, rvec, tvec, iterations, confidence, out_inliers, out_n_inliers);
    if (rc) return rc;
    PnPReq r;
    r.kind = Q_PNP; r.b = E->slots[seq];
    if ((rc = pnp_prepare(ctx, r.b, obj_xyz, img_xy, m, K, iterations, reproj_err, confidence, &r.P, &r.L))) return rc;
    rc = submit(ctx, E->queue[R_PNP], &r);
    if (rc) return rc;
    pnp_finish(ctx, r.b, obj_xyz, img_xy, m, K, rvec, tvec, iterations, reproj_err, confidence, r.L, out_inliers, out_n_inliers);
    return PMV_OK;
}

int engine_ba(BatchEngine* E, int seq, double* cams, int nc, double* pts, int np, const double* obs_xy, const int* cam_idx, const int* pt_idx, int n_obs,
              const double* K, double huber, int max_iterations, pmv_ba_summary* summary) {
    pmv_ctx* ctx = E->ctx;
    int rc = ba_check(ctx, cams, nc, pts, np, obs_xy, cam_idx, pt_idx, n_obs, K, huber, max_iterations);
    if (rc) return rc;
    if (max_iterations == 0) {   // as pmv_ba_solve: the parameters stay untouched
        if (summary) { summary->initial_cost = summary->final_cost = 0.0; summary->iterations = 0; summary->successful_steps = 0; summary->termination = 0; }
        return PMV_OK;
    }
    BAReq r;
    r.kind = Q_BA; r.b = E->slots[seq]; r.max_iterations = max_iterations;
    rc = ba_prepare(ctx, r.b, cams, nc, pts, np, obs_xy, cam_idx, pt_idx, n_obs, K, huber, max_iterations, ctx->ba_mode != 1, &r.A, &r.L);
    if (rc) return rc;
    if (ctx->ba_mode == 1) r.A.out = (double*)r.b->h_stage.dm();   // k_ba_lm_batch copies [summary | cams | pts] into the request's pinned block
    rc = submit(ctx, E->queue[R_BA], &r);
    if (rc) return rc;
    ba_finish(ctx, r.b, cams, nc, pts, np, obs_xy, cam_idx, pt_idx, n_obs, K, huber, max_iterations, r.L, summary);
    return PMV_OK;
}

int engine_dlt(BatchEngine* E, int seq, const double* q1, const double* q2, int n, const double* P1x4, const uint8_t* mask_in, double* out_Q,
               uint8_t* out_mask, int* out_good) {
    pmv_ctx* ctx = E->ctx;
    int rc = dlt_check(ctx, "pmv_triangulate_candidates", q1, q2, n, P1x4, mask_in, out_Q, out_mask, out_good);
    if (rc) return rc;
    DltReq r;
    r.kind = Q_DLT; r.b = E->slots[seq];
    rc = dlt_prepare(ctx, r.b, q1, q2, n, P1x4, mask_in, &r.P, &r.L);
    if (rc) return rc;
    rc = submit(ctx, E->queue[R_DLT], &r);
    if (rc) return rc;
    dlt_finish(ctx, r.b, q1, q2, n, P1x4, mask_in, r.L, out_Q, out_mask, out_good);
    return PMV_OK;
}

int engine_tri_tracks(BatchEngine* E, int seq, const double* P3x4, int nc, const double* obs_xy, const int* cam_idx, const int* pt_idx, int n_obs, int np,
                      const pmv_tri_params* p_or_null, double* out_xyz, uint8_t* out_status, double* out_err_or_null, int* out_good) {
    pmv_ctx* ctx = E->ctx;
    int rc = tri_tracks_check(ctx, "pmv_triangulate_tracks", P3x4, nc, obs_xy, cam_idx, pt_idx, n_obs, np, p_or_null, out_xyz, out_status, out_good);
    if (rc) return rc;
    if (np == 0 || n_obs == 0) { tri_tracks_empty(np, out_xyz, out_status, out_err_or_null, out_good); return PMV_OK; }
    TriTracksReq r;
    r.kind = Q_TRI_TRACKS; r.b = E->slots[seq];
    rc = tri_tracks_prepare(ctx, r.b, P3x4, nc, obs_xy, cam_idx, pt_idx, n_obs, np, p_or_null, &r.P, &r.L);
    if (rc) return rc;
    rc = submit(ctx, E->queue[R_DLT], &r);
    if (rc) return rc;
    tri_tracks_finish(r.b, np, r.L, out_xyz, out_status, out_err_or_null, out_good);
    return PMV_OK;
}

int engine_fivepoint(BatchEngine* E, int seq, const double* q1, const double* q2, int n, const int* samples, int n_hyp, float thr, double* models,
                     int* n_models, int* counts) {
    pmv_ctx* ctx = E->ctx;
    int rc = fivepoint_check(ctx, models, n_models, counts);
    if (rc) return rc;
    FPReq r;
    r.kind = Q_FIVEPOINT; r.b = E->slots[seq];
    rc = fivepoint_prepare(ctx, r.b, q1, q2, n, samples, n_hyp, thr, &r.P, &r.L);
    if (rc) return rc;
    rc = submit(ctx, E->queue[R_FP], &r);
    if (rc) return rc;
    fivepoint_finish(r.b, n_hyp, r.L, models, n_models, counts);
    return PMV_OK;
}

}  // namespace pmv

namespace pmv {

// The wait of a whole-RANSAC request: whichever comes first, the completion word that its own workgroup stores last into the seq's pinned
// result block, or the combiner's done flag after the round's stream sync (the only one a failed launch gives).
static int wait_whole(pmv_ctx* ctx, WholeReq& r, volatile unsigned* word, unsigned want) {
    for (;;) {
        if (__atomic_load_n(word, __ATOMIC_ACQUIRE) == want) return PMV_OK;
        if (r.done.load(std::memory_order_acquire)) {   // the round is over
            if (__atomic_load_n(word, __ATOMIC_ACQUIRE) == want) return PMV_OK;
            const int rc = r.rc != PMV_OK ? r.rc : PMV_ERR_HIP;
            set_err(ctx, "%s", r.rc != PMV_OK ? r.err : "batch engine: the round ended without the request's completion word");
            return rc;
        }
        std::this_thread::sleep_for(std::chrono::microseconds(20));
    }
}

// pmv_find_essential_mat's or pmv_find_fundamental_mat's contract through the five-point combiner, behind the call's argument check: the
// request is one workgroup of the round's launch of its kind. The caller waits for whichever comes first: the completion word that
// its own workgroup stores last into the seq's pinned result block, or the combiner's done flag after the round's stream sync (the only
// one a failed launch gives). After the word the workgroup touches nothing of the seq's blocks any more, so the seq's next call may use them
// while the round's other workgroups are still running; only the request record stays taken until the combiner has released it.
// prepare: either *_prepare, bound to the call's arguments.
template <class Pt, class Prepare>
static int engine_whole(BatchEngine* E, WholeReqOf<Pt>& r, int kind, int seq, Prepare prepare, int n, double* M9, uint8_t* mask, int* out_found, int* out_samples_drawn) {
    futex_wait_while(&r.inflight, 1);   // the round of this seq's previous call is still in flight: its combiner has yet to release the record
    r.kind = kind; r.rc = PMV_OK; r.err[0] = 0; r.b = E->slots[(size_t)seq];
    if (const int rc = prepare(r.b, &r.P, &r.L)) return rc;
    r.done.store(0, std::memory_order_relaxed);
    r.inflight.store(1, std::memory_order_release);
    enqueue(E->queue[R_FP], &r);
    if (const int rc = wait_whole(E->ctx, r, whole_done_word(r.b, r.L), r.P.done_seq)) return rc;
    whole_finish(r.b, n, r.L, M9, mask, out_found, out_samples_drawn);
    return PMV_OK;
}

int engine_essential(BatchEngine* E, int seq, const double* p1_xy, const double* p2_xy, int n, const double* K, double prob, double threshold, double* E9,
                     uint8_t* mask, int* out_found, int* out_samples_drawn) {
    pmv_ctx* ctx = E->ctx;
    if (const int rc = essential_check(ctx, "pmv_find_essential_mat", p1_xy, p2_xy, n, K, prob, threshold, E9, mask, out_found, out_samples_drawn)) return rc;
    *out_found = 0; *out_samples_drawn = 0;
    if (n < 5) { memset(mask, 0, (size_t)n); return PMV_OK; }
    const auto prepare = [&](BackendBuffers* b, EssentialProblem* P, WholeLayout* L) { return essential_prepare(ctx, b, p1_xy, p2_xy, n, K, prob, threshold, P, L); };
    return engine_whole(E, E->ess[(size_t)seq], Q_ESSENTIAL, seq, prepare, n, E9, mask, out_found, out_samples_drawn);
}

int engine_fundamental(BatchEngine* E, int seq, const float* p1_xy, const float* p2_xy, int n, double threshold, double confidence, double* F9, uint8_t* mask,
                       int* out_found, int* out_samples_drawn) {
    pmv_ctx* ctx = E->ctx;
    if (const int rc = fundamental_check(ctx, "pmv_find_fundamental_mat", p1_xy, p2_xy, n, threshold, confidence, F9, mask, out_found, out_samples_drawn)) return rc;
    const auto prepare = [&](BackendBuffers* b, FundamentalProblem* P, WholeLayout* L) { return fundamental_prepare(ctx, b, p1_xy, p2_xy, n, threshold, confidence, P, L); };
    return engine_whole(E, E->fund[(size_t)seq], Q_FUNDAMENTAL, seq, prepare, n, F9, mask, out_found, out_samples_drawn);
}

int engine_homography(BatchEngine* E, int seq, const float* p1_xy, const float* p2_xy, int n, double threshold, double confidence, int max_iters, double* H9,
                      uint8_t* mask, int* out_found, int* out_samples_drawn) {
    pmv_ctx* ctx = E->ctx;
    if (const int rc = homography_check(ctx, "pmv_find_homography", p1_xy, p2_xy, n, threshold, confidence, max_iters, H9, mask, out_found, out_samples_drawn)) return rc;
    const auto prepare = [&](BackendBuffers* b, HomographyProblem* P, WholeLayout* L) { return homography_prepare(ctx, b, p1_xy, p2_xy, n, threshold, confidence, max_iters, P, L); };
    return engine_whole(E, E->homog[(size_t)seq], Q_HOMOGRAPHY, seq, prepare, n, H9, mask, out_found, out_samples_drawn);
}

}  // namespace pmv
