// HIP plugin set: the reference's five plugin roles served by this library - through its C ABI or, for the sequences of a batched run,
// through the batch engine (Route) - plugged into the host pipeline mirror (host/vo_pipeline.*). This is the drop-in: OdometryPipeline/addFrame/estimatePose stay host C++,
// every numerically heavy call crosses into the gfx950 kernels. No CPU fallback exists on this path (the triangulator,
// which the north star does not move to the device, is the host implementation in host/vo_fivepoint.cpp).
#include "pmv_ctx.h"
#include "batch_engine.h"
#include "ingest_batch.h"
#include <mutex>
#include <thread>
#include "vo_capi_impl.h"
#include <algorithm>
#include <cstring>
#include <stdexcept>
#include <string>
#include <malloc.h>

namespace {
using namespace vo;

struct HipError : std::runtime_error { int code; HipError(int c, const char* m) : std::runtime_error(m), code(c) {} };
inline void ck(pmv_ctx* ctx, int rc) { (void)ctx; if (rc != PMV_OK) throw HipError(rc, pmv::thread_error()); }   // this thread's own message

static void cells_of(const std::vector<ImageView>& cells, std::vector<int>& out) {
    out.clear();
    for (auto& c : cells) { out.push_back(c.x0); out.push_back(c.y0); out.push_back(c.w); out.push_back(c.h); }
}

// The frames a request of the batch engine reads: slot_ready on the sequence's own thread (for a fed sequence it waits until the feeder has
// enqueued their build); the request carries the feed round the combiner's stream must wait for.
struct RingFrames {
    pmv::BatchIngest* feed = nullptr; int seq = -1;   // seq: the sequence's index in the feed, -1 = not fed (it may still read fed slots)
    int round(pmv_ctx* ctx, int slot_a, int slot_b = -1) {
        int ra = -1, rb = -1;
        ck(ctx, pmv::slot_ready(ctx, slot_a, feed, seq, nullptr, &ra));
        if (slot_b >= 0) ck(ctx, pmv::slot_ready(ctx, slot_b, feed, seq, nullptr, &rb));
        return std::max(ra, rb);
    }
};
// How a plugin call travels: as the single call of the C ABI (eng null: pmv_pipeline_run), or as a request of the batch engine
// (batch_engine.hip: several sequences per launch) for sequence `seq` of a batched run, whose frames `ring` waits for. Each member has
// the contract of the pmv_* call it names and returns its status.
struct Route {
    pmv_ctx* ctx = nullptr; pmv::BatchEngine* eng = nullptr; RingFrames ring; int seq = 0;
    int gftt(int slot, const int* cells, int n_cells, int max, double quality, double min_dist, int* xy, int* cnt) {
        return eng ? pmv::engine_detect(eng, pmv::Q_GFTT, slot, cells, n_cells, max, quality, min_dist, xy, nullptr, cnt, ring.round(ctx, slot))
                   : pmv_detect_gftt(ctx, slot, cells, n_cells, max, quality, min_dist, xy, cnt);
    }
    int shitomasi(int slot, const int* cells, int n_cells, int max, double quality, int* xy, double* score, int* cnt) {
        return eng ? pmv::engine_detect(eng, pmv::Q_SHITOMASI, slot, cells, n_cells, max, quality, 0.0, xy, score, cnt, ring.round(ctx, slot))
                   : pmv_detect_shitomasi(ctx, slot, cells, n_cells, max, quality, xy, score, cnt);
    }
    int fast(int slot, const int* cells, int n_cells, int max, int threshold, int nonmax, int* xy, float* response, int* cnt) {
        return eng ? pmv::engine_detect_fast(eng, slot, cells, n_cells, max, threshold, nonmax, xy, response, cnt, ring.round(ctx, slot))
                   : pmv_detect_fast(ctx, slot, cells, n_cells, max, threshold, nonmax, xy, response, cnt);
    }
    int knn(int src_slot, int cmp_slot, const int* src_xy, int n, const int* cmp_xy, int m, int neighbours, int window, int* best, float* err) {
        return eng ? pmv::engine_knn(eng, src_slot, cmp_slot, src_xy, n, cmp_xy, m, neighbours, window, best, err, ring.round(ctx, src_slot, cmp_slot))
                   : pmv_knn_match(ctx, src_slot, cmp_slot, src_xy, n, cmp_xy, m, neighbours, window, best, err);
    }
    // predicted, iters: the engine's ordering hint (batch_engine.h); the single call deals its tracks by position alone
    int lk(int prev_slot, int next_slot, const float* prev_xy, int n, float* next_xy, uint8_t* status, float* err, const uint8_t* predicted, uint8_t* iters) {
        return eng ? pmv::engine_lk(eng, prev_slot, next_slot, prev_xy, n, next_xy, status, err, predicted, iters, ring.round(ctx, prev_slot, next_slot))
                   : pmv_lk_track(ctx, prev_slot, next_slot, prev_xy, n, next_xy, status, err);
    }
    int pnp(const float* obj, const float* img, int m, const double* K, double* rvec, double* tvec, int iterations, float reproj_err, double confidence,
            int* inliers, int* n_inliers) {
        return eng ? pmv::engine_pnp(eng, seq, obj, img, m, K, rvec, tvec, iterations, reproj_err, confidence, inliers, n_inliers)
                   : pmv_pnp_ransac(ctx, obj, img, m, K, rvec, tvec, iterations, reproj_err, confidence, inliers, n_inliers);
    }
    int ba(double* cams, int nc, double* pts, int np, const double* obs_xy, const int* cam_idx, const int* pt_idx, int n_obs, const double* K, double huber,
           int max_iterations) {
        return eng ? pmv::engine_ba(eng, seq, cams, nc, pts, np, obs_xy, cam_idx, pt_idx, n_obs, K, huber, max_iterations)
                   : pmv_ba_solve(ctx, cams, nc, pts, np, obs_xy, cam_idx, pt_idx, n_obs, K, huber, max_iterations, nullptr);
    }
    int dlt(const double* q1, const double* q2, int n, const double* P1x4, const uint8_t* mask_in, double* out_Q, uint8_t* out_mask, int* out_good) {
        return eng ? pmv::engine_dlt(eng, seq, q1, q2, n, P1x4, mask_in, out_Q, out_mask, out_good)
                   : pmv_triangulate_candidates(ctx, q1, q2, n, P1x4, mask_in, out_Q, out_mask, out_good);
    }
    int fivepoint(const double* q1, const double* q2, int n, const int* samples, int n_hyp, float thr, double* models, int* n_models, int* counts) {
        return eng ? pmv::engine_fivepoint(eng, seq, q1, q2, n, samples, n_hyp, thr, models, n_models, counts)
                   : pmv_fivepoint_hypotheses(ctx, q1, q2, n, samples, n_hyp, thr, models, n_models, counts);
    }
    int essential(const double* p1, const double* p2, int n, const double* K, double prob, double threshold, double* E, uint8_t* mask, int* found, int* samples_drawn) {
        return eng ? pmv::engine_essential(eng, seq, p1, p2, n, K, prob, threshold, E, mask, found, samples_drawn)
                   : pmv_find_essential_mat(ctx, p1, p2, n, K, prob, threshold, E, mask, found, samples_drawn);
    }
};

// per-cell lists of a detector call: `per` entries per cell, cnt[c] of them filled; val (with vals) runs beside xy
template <class T>
static void lists_of(size_t n_cells, size_t per, const std::vector<int>& xy, const std::vector<int>& cnt, std::vector<std::vector<std::pair<int, int>>>& out,
                     const std::vector<T>* val = nullptr, std::vector<std::vector<T>>* vals = nullptr) {
    for (size_t c = 0; c < n_cells; c++)
        for (int i = 0; i < cnt[c]; i++) {
            out[c].push_back({xy[(c * per + i) * 2], xy[(c * per + i) * 2 + 1]});
            if (vals) (*vals)[c].push_back((*val)[c * per + i]);
        }
}

struct HipGftt : GoodFeatureExtractorBase {
    Route via;
    std::vector<int> rect, xy, cnt;
    void gftt(const std::vector<ImageView>& cells, int max, std::vector<std::vector<std::pair<int, int>>>& out) override {
        out.assign(cells.size(), {});
        if (cells.empty()) return;
        cells_of(cells, rect);
        const size_t cap = max > 0 ? (size_t)max : (size_t)PMV_GFTT_UNLIMITED_CAP;   // max <= 0: no limit (cv::goodFeaturesToTrack)
        xy.resize(cells.size() * cap * 2);
        cnt.resize(cells.size());
        ck(via.ctx, via.gftt(cells[0].slot, rect.data(), (int)cells.size(), max, quality, min_distance, xy.data(), cnt.data()));
        lists_of<int>(cells.size(), cap, xy, cnt, out);
    }
};
struct HipShiTomasi : ShiTomasiExtractorBase {
    Route via;
    std::vector<int> rect, xy, cnt;
    std::vector<double> sc;
    void shitomasi(const std::vector<ImageView>& cells, int max, std::vector<std::vector<std::pair<int, int>>>& out,
                   std::vector<std::vector<double>>& score) override {
        out.assign(cells.size(), {});
        score.assign(cells.size(), {});
        if (cells.empty() || max < 1) return;
        cells_of(cells, rect);
        xy.resize(cells.size() * (size_t)max * 2);
        sc.resize(cells.size() * (size_t)max);
        cnt.resize(cells.size());
        ck(via.ctx, via.shitomasi(cells[0].slot, rect.data(), (int)cells.size(), max, quality, xy.data(), sc.data(), cnt.data()));
        lists_of(cells.size(), (size_t)max, xy, cnt, out, &sc, &score);
    }
};
struct HipFast : FastExtractorBase {
    Route via;
    std::vector<int> rect, xy, cnt;
    std::vector<float> rs;
    void fast(const std::vector<ImageView>& cells, int max, std::vector<std::vector<std::pair<int, int>>>& out,
              std::vector<std::vector<float>>& response) override {
        out.assign(cells.size(), {});
        response.assign(cells.size(), {});
        if (cells.empty() || max < 1) return;
        cells_of(cells, rect);
        xy.resize(cells.size() * (size_t)max * 2); rs.resize(cells.size() * (size_t)max); cnt.resize(cells.size());
        ck(via.ctx, via.fast(cells[0].slot, rect.data(), (int)cells.size(), max, threshold, nonmax ? 1 : 0, xy.data(), rs.data(), cnt.data()));
        lists_of(cells.size(), (size_t)max, xy, cnt, out, &rs, &response);
    }
};
struct HipKnn : KnnFeatureMatcherBase {   // (`extractor` = the sequence's HipFast: matchFeatures calls it on the whole next frame)
    Route via;
    void knn(const ImageView& src, const ImageView& next, const int* src_xy, int n, const int* cmp_xy, int m, int* best, float* err) override {
        ck(via.ctx, via.knn(src.slot, next.slot, src_xy, n, cmp_xy, m, neighbours, window, best, err));
    }
};
struct HipLK : LucasKanadeFMBase {
    Route via;
    // Ordering hint for the batched launch (engine route only; no effect on any result): a track that needed many LK iterations in the last
    // frame pair tends to need many again (weak texture, an edge along the motion), and a launch ends with its slowest track - so the engine
    // starts the expensive ones first. The cost of a track is remembered under the integer pixel it was tracked TO, which is where the next call
    // starts it from (the adapter truncates exactly like this: OpenCVLucasKanadeFM.cpp:25); re-detected features are new: default cost.
    static constexpr int TBL = 2048, DEFAULT_COST = 24;   // open addressing, > 2 x the tracks of a frame (1024 max)
    std::vector<uint32_t> tkey = std::vector<uint32_t>(TBL, 0xffffffffu);
    std::vector<uint8_t> tval = std::vector<uint8_t>(TBL, 0);
    std::vector<uint8_t> pred, iters;
    static uint32_t key_of(float x, float y) { return ((uint32_t)(int)y << 16) ^ (uint32_t)(int)x; }
    static uint32_t slot_of(uint32_t k) { return (k * 2654435761u) >> 21; }   // 11 bits
    void pyrlk(const ImageView& prev, const ImageView& next, const float* prev_xy, int n, float* next_xy, uint8_t* status,
               float* err) override {
        if (!via.eng) { ck(via.ctx, via.lk(prev.slot, next.slot, prev_xy, n, next_xy, status, err, nullptr, nullptr)); return; }
        pred.resize((size_t)n); iters.resize((size_t)n);
        const bool use = n <= TBL / 2;
        for (int i = 0; i < n; i++) {
            uint8_t c = DEFAULT_COST;
            if (use) {
                const uint32_t k = key_of(prev_xy[2 * i], prev_xy[2 * i + 1]);
                for (uint32_t h = slot_of(k);; h = (h + 1) & (TBL - 1)) {
                    if (tkey[h] == k) { c = tval[h]; break; }
                    if (tkey[h] == 0xffffffffu) break;
                }
            }
            pred[(size_t)i] = c;
        }
        ck(via.ctx, via.lk(prev.slot, next.slot, prev_xy, n, next_xy, status, err, pred.data(), iters.data()));
        std::fill(tkey.begin(), tkey.end(), 0xffffffffu);
        if (!use) return;
        for (int i = 0; i < n; i++) {
            if (!status[i]) continue;
            const uint32_t k = key_of(next_xy[2 * i], next_xy[2 * i + 1]);
            uint32_t h = slot_of(k);
            while (tkey[h] != 0xffffffffu && tkey[h] != k) h = (h + 1) & (TBL - 1);
            if (tkey[h] == k) { if (iters[(size_t)i] > tval[h]) tval[h] = iters[(size_t)i]; }   // two tracks on one pixel: the dearer one
            else { tkey[h] = k; tval[h] = iters[(size_t)i]; }
        }
    }
};
struct HipPnP : EPnPSolverBase {
    Route via;
    bool pnp_ransac(const float* obj, const float* img, int m, const double* K, double* rvec, double* tvec,
                    std::vector<int>& inliers) override {
        inliers.assign(m > 0 ? m : 1, 0);
        int n = 0;
        const int rc = via.pnp(obj, img, m, K, rvec, tvec, 100, 8.f, .99, inliers.data(), &n);
        if (rc == PMV_ERR_DEGENERATE) { inliers.clear(); return false; }   // cv::Exception in the reference
        ck(via.ctx, rc);
        inliers.resize(n);
        return n > 0;
    }
};
struct HipTri : vo::FivePointTri {   // five-point RANSAC on host threads (default), its hypotheses round by round or the whole loop on the GPU; recoverPose's DLT + cheirality on the GPU
    Route via;
    bool essential_hypotheses(const double* q1, const double* q2, int n, const int* samples, int n_hyp, float thr, double* models, int* n_models,
                              int* counts) override {
        ck(via.ctx, via.fivepoint(q1, q2, n, samples, n_hyp, thr, models, n_models, counts));
        return true;
    }
    bool essential_whole(const double* p1, const double* p2, int n, const double* K, double prob, double threshold, double* E, uint8_t* mask, bool* found,
                         int* samples_drawn) override {
        int f = 0;
        ck(via.ctx, via.essential(p1, p2, n, K, prob, threshold, E, mask, &f, samples_drawn));
        *found = f != 0;
        return true;
    }
    void dlt_candidates(const double* q1, const double* q2, int n, const double* P1x4, const uint8_t* mask_in, double* out_Q,
                        uint8_t* out_mask, int* out_good) override {
        ck(via.ctx, via.dlt(q1, q2, n, P1x4, mask_in, out_Q, out_mask, out_good));
    }
    // (single route only: the context's auxiliary lane. A sequence of a batched run has no prefetch helpers.)
    void dlt_candidates_ahead(const double* q1, const double* q2, int n, const double* P1x4, const uint8_t* mask_in, double* out_Q,
                              uint8_t* out_mask, int* out_good) override {
        if (via.eng) { FivePointTri::dlt_candidates_ahead(q1, q2, n, P1x4, mask_in, out_Q, out_mask, out_good); return; }
        ck(via.ctx, pmv_triangulate_candidates_ahead(via.ctx, q1, q2, n, P1x4, mask_in, out_Q, out_mask, out_good));
    }
};
struct HipBA : BundleAdjustmentBase {
    Route via;
    void ba_solve(double* cams, int nc, double* pts, int np, const double* obs_xy, const int* cam_idx, const int* pt_idx, int n_obs,
                  const double* K, double huber, int max_iterations) override {
        ck(via.ctx, via.ba(cams, nc, pts, np, obs_xy, cam_idx, pt_idx, n_obs, K, huber, max_iterations));
    }
};

vo::PipelineParams params_of(const pmv_pipeline_params* P, int n_threads) {
    vo::PipelineParams vp;
    vp.n_frames = P->n_frames; vp.w = P->w; vp.h = P->h;
    vp.min_tracked_features = P->min_tracked_features; vp.tracked_features_tol = P->tracked_features_tol;
    vp.init_frames = P->init_frames; vp.bundle_size = P->bundle_size; vp.ba_iterations = P->ba_iterations;
    vp.extractor = P->extractor; vp.threaded = P->threaded; vp.n_threads = n_threads; vp.reserved = 0; vp.matcher = P->matcher;
    return vp;
}

// The five plugins of a run, all travelling `via`, wired into run.pipe (after pipeline_setup). tri_workers: threads of the host five-point
// RANSAC; the two-thread single pipeline also gets its prefetch helpers.
void plug_in(vo::PipelineRun& run, const pmv_pipeline_params* P, const Route& via, int tri_workers) {
    vo::BaseFeatureExtractor* ex;
    if (P->extractor == 1) { auto* e = new HipShiTomasi(); e->via = via; ex = e; }
    else if (P->extractor == 2) { auto* e = new HipFast(); e->via = via; ex = e; }
    else { auto* e = new HipGftt(); e->via = via; ex = e; }
    run.owned_ex.push_back(ex);
    vo::BaseFeatureMatcher* lk;
    if (P->matcher == 1) {   // kNNFeatureMatcher(extractor): the reference's alternative matcher; it calls the extractor on whole frames
        if (P->extractor != 2) throw std::runtime_error("the kNN matcher needs an extractor that accepts whole frames: extractor = 2 (FAST)");   // (a batch: check_params)
        auto* k = new HipKnn(); k->via = via; k->extractor = ex; lk = k;
    } else { auto* l = new HipLK(); l->via = via; lk = l; }
    auto* pnp = new HipPnP(); pnp->via = via; pnp->tracker = &run.pipe;
    auto* tri = new HipTri(); tri->via = via; tri->tracker = &run.pipe; tri->workers = tri_workers;
    tri->use_whole_hook = P->device_fivepoint == 2;   // the whole findEssentialMat: one launch, or one request of the five-point combiner
    tri->use_hypothesis_hook = P->device_fivepoint != 0 && !tri->use_whole_hook;
    tri->prefetch_threads = (!via.eng && P->n_threads > 1 && P->device_fivepoint == 0) ? 2 : 0;   // only the two-thread pipeline calls prefetch()
    auto* ba = new HipBA(); ba->via = via; ba->tracker = &run.pipe;
    run.m = lk; run.p = pnp; run.tr = tri; run.b = ba;
    run.pipe.extractor = ex; run.pipe.matcher = lk; run.pipe.pnpsolver = pnp; run.pipe.triangulator = tri; run.pipe.ba = ba;
}
}  // namespace

struct pmv_pipeline_result { vo::PipelineRun run; };

// The host threads of a run allocate and free per-frame tables all the time, each in its own glibc arena; with the default tunables an
// arena gives its top back as soon as 128 KB are free and grows again a frame later - mprotect / madvise calls that take the process's
// address-space lock. Sampled on a B = 192 run (scripts/hostprof): 30 % of the host CPU time of the timed region in mprotect,
// __default_morecore, madvise and malloc itself. Keep freed memory in the arenas instead (once per process; PMV_KEEP_MALLOC_DEFAULTS=1
// leaves the process's settings alone).
static void host_allocator_setup() {
    static std::once_flag once;
    std::call_once(once, [] {
        if (getenv("PMV_KEEP_MALLOC_DEFAULTS")) return;
        mallopt(M_TRIM_THRESHOLD, 1 << 30);
        mallopt(M_TOP_PAD, 16 << 20);
        mallopt(M_MMAP_THRESHOLD, 32 << 20);
    });
}

// Sequence b of a batched run, on the calling thread: the reference's pipeline with the batch engine's plugin set. Frame i lives in slot
// first_slot + i % ring. A fed sequence (fed = its index in the feed `ing`, else -1) reports every frame it has finished with
// (OdometryPipeline::on_frame_added) and its end.
static void run_batch_sequence(pmv_ctx* ctx, pmv::BatchEngine* eng, int b, const pmv_pipeline_params* P, const double* K9, const double* gt_poses12,
                               int first_slot, pmv::BatchIngest* ing, int fed, int ring, pmv_pipeline_result** out, int& code, std::string& msg) {
    auto* res = new pmv_pipeline_result();
    vo::PipelineRun& run = res->run;
    const vo::PipelineParams vp = params_of(P, 1);
    try {
        vo::pipeline_setup(run, vp, nullptr, K9, gt_poses12);
        for (auto& im : run.pipe.images) im.slot = first_slot + im.slot % ring;
        if (fed >= 0) {
            // on_frame_added(k) follows addFrame of frames[k] = image k + init_offset (initialise() keeps image init_offset as frames[0]):
            // every image below that one is dead - addFrame(i + 1) reads images i and i + 1 only
            vo::OdometryPipeline* pipe = &run.pipe;
            run.pipe.on_frame_added = [ing, fed, pipe](int k) { pmv::batch_ingest_release(ing, fed, k + pipe->init_offset); };
        }
        plug_in(run, P, Route{ctx, eng, RingFrames{ing, fed}, b}, 1);
        vo::pipeline_execute(run, vp);
        *out = res;
    } catch (const HipError& e) {
        code = e.code; msg = e.what(); delete res;
    } catch (const std::exception& e) {
        code = PMV_ERR_INVALID; msg = e.what(); delete res;
    }
    if (fed >= 0) pmv::batch_ingest_finish(ing, fed);   // finished or failed: its whole ring is free
}

// The parameter rules the entry points share: bundle_size, and for a batch the sequence's own frame size (within the context's capacity) and
// the plugin pairs (those of the single run).
static int check_params(pmv_ctx* ctx, const char* who, const pmv_pipeline_params& P, bool batch) {
    if (P.bundle_size != 0 && P.bundle_size < 3) { pmv::set_err(ctx, "%s: bundle_size 1..2 divides by zero in the reference (OdometryPipeline.cpp:407)", who); return PMV_ERR_INVALID; }
    if (P.bundle_size > ctx->max_ba_cams) { pmv::set_err(ctx, "%s: bundle_size exceeds max_ba_cams", who); return PMV_ERR_CAPACITY; }
    if (!batch) return PMV_OK;
    if (P.w < 40 || P.h < 40 || P.w > ctx->max_w || P.h > ctx->max_h) { pmv::set_err(ctx, "%s: frame %dx%d outside capacity %dx%d", who, P.w, P.h, ctx->max_w, ctx->max_h); return PMV_ERR_CAPACITY; }
    // the plugin pairs pmv_pipeline_run serves, refused here before any sequence thread or feed starts (the single run finds the last one by exception)
    if (P.extractor < 0 || P.extractor > 2) { pmv::set_err(ctx, "%s: extractor = %d: the extractor is 0 (GFTT), 1 (ShiTomasi) or 2 (FAST)", who, P.extractor); return PMV_ERR_INVALID; }
    if (P.matcher < 0 || P.matcher > 1) { pmv::set_err(ctx, "%s: matcher = %d: the matcher is 0 (LK) or 1 (kNN)", who, P.matcher); return PMV_ERR_INVALID; }
    if (P.matcher == 1 && P.extractor != 2) {
        pmv::set_err(ctx, "%s: matcher = 1 needs extractor = 2: the kNN matcher calls the extractor on whole frames, which only FAST accepts (got extractor = %d)", who, P.extractor);
        return PMV_ERR_INVALID;
    }
    return PMV_OK;
}

// Everything the two batched entry points share once each has validated its slots: sequence b reads slots first_slot[b] .. + ring[b] - 1,
// fed from host_frames[b] (streamed batch), staged in place (host_frames null: the sequences with build_pyramids), or not at all.
static int run_batch(pmv_ctx* ctx, const char* who, int B, const pmv_pipeline_params* params, const double* K9, const double* const* gt_poses12,
                     const uint8_t* const* host_frames, const int* first_slot, const int* ring, pmv_pipeline_result** out) {
    // every sequence has its own frame size (the reference takes whatever cv::imread returns, Frame.cpp:31-42; KITTI odometry comes in three)
    for (int b = 0; b < B; b++)
        if (const int rc = check_params(ctx, who, params[b], true)) return rc;
    // The run owns the engine and the geometry table until it returns: not while a batch session (pmv_batch_open) holds them. The count also
    // keeps pmv_set_frame_format and pmv_batch_open away for the duration of the run.
    struct Open {
        pmv_ctx* c; bool ok;
        Open(pmv_ctx* c_) : c(c_) { std::lock_guard<std::mutex> own(c->owner_mu); ok = c->session_state.load() == 0; if (ok) c->batch_open++; }
        ~Open() { if (ok) c->batch_open--; }
    } open(ctx);
    if (!open.ok) { pmv::set_err(ctx, "%s: a batch session is open on this context (pmv_batch_close first): it owns the batch engine and the geometry table", who); return PMV_ERR_INVALID; }
    pmv::BatchEngine* eng = nullptr;
    int rc = pmv::batch_engine_get(ctx, B, &eng);
    if (rc != PMV_OK) return rc;
    rc = pmv_sync(ctx);
    if (rc != PMV_OK) return rc;
    {   // the geometry table of the run's batched launches: one entry per distinct frame size, before any feeder or sequence thread exists
        std::vector<int> ws((size_t)B), hs((size_t)B);
        for (int b = 0; b < B; b++) { ws[(size_t)b] = params[b].w; hs[(size_t)b] = params[b].h; }
        if ((rc = pmv::geom_table_set(ctx, ws.data(), hs.data(), B)) != PMV_OK) return rc;
    }
    std::vector<pmv::FeedSeq> feed;
    std::vector<int> fed((size_t)B, -1);
    for (int b = 0; b < B; b++)
        if (host_frames || params[b].build_pyramids) {
            fed[(size_t)b] = (int)feed.size();
            feed.push_back({first_slot[b], params[b].n_frames, ring[b], host_frames ? host_frames[b] : nullptr, params[b].w, params[b].h});
        }
    if (!feed.empty() && (rc = pmv::batch_ingest_begin(ctx, ctx->bingest, host_frames ? pmv::FEED_STREAMED : pmv::FEED_STAGED, feed, host_frames ? ctx->frame_format : PMV_FRAMES_GRAY,
                                                       host_frames ? &ctx->preproc : nullptr)) != PMV_OK)
        return rc;
    std::vector<int> codes(B, PMV_OK);
    std::vector<std::string> msgs(B);
    std::vector<std::thread> th;
    for (int b = 0; b < B; b++)
        th.emplace_back([&, b] { run_batch_sequence(ctx, eng, b, &params[b], K9 + 9 * b, gt_poses12[b], first_slot[b], ctx->bingest, fed[(size_t)b], ring[b], &out[b], codes[b], msgs[b]); });
    for (auto& t : th) t.join();
    if (!feed.empty()) {
        rc = pmv::batch_ingest_end(ctx, ctx->bingest);   // joins the feeder thread (also after a failed sequence: the sources are the caller's)
        if (host_frames) pmv::batch_ingest_stats(ctx->bingest, ctx->bingest_stats);
        if (rc != PMV_OK) { for (int k = 0; k < B; k++) { delete out[k]; out[k] = nullptr; } return rc; }
    }
    for (int b = 0; b < B; b++)
        if (codes[b] != PMV_OK) {
            pmv::set_err(ctx, "%s: sequence %d: %s", who, b, msgs[b].c_str());
            for (int k = 0; k < B; k++) { delete out[k]; out[k] = nullptr; }
            return codes[b];
        }
    return PMV_OK;
}

extern "C" {

// Same run from HOST frames (n_frames frames of w * h gray or 3 * w * h BGR bytes, pmv_set_frame_format; pageable or pinned): the frames are streamed into slots 0..n_frames-1 by
// the feeder (a pmv_frames_stream_begin bracket, ingest_batch.hip) while the pipeline is already tracking the first ones. Results are identical to
// pmv_frames_stage + pmv_pipeline_run(build_pyramids = 1).
int pmv_pipeline_run_streamed(pmv_ctx* ctx, const pmv_pipeline_params* P, const double* K9, const double* gt_poses12,
                              const uint8_t* host_frames, pmv_pipeline_result** out) {
    if (!ctx || !P || !host_frames) { pmv::set_err(ctx, "pmv_pipeline_run_streamed: null argument"); return PMV_ERR_INVALID; }
    if (P->n_frames > ctx->n_slots) { pmv::set_err(ctx, "pmv_pipeline_run_streamed: n_frames=%d exceeds the %d frame slots", P->n_frames, ctx->n_slots); return PMV_ERR_CAPACITY; }
    int rc = pmv_frames_stream_begin(ctx, 0, P->n_frames, host_frames, P->w, P->h);
    if (rc != PMV_OK) return rc;
    pmv_pipeline_params Q = *P;
    Q.build_pyramids = 0;   // the feeder builds them round by round
    rc = pmv_pipeline_run(ctx, &Q, K9, gt_poses12, out);
    const int rc2 = pmv_frames_stream_end(ctx);   // joins the feeder thread (also after a failed run: the source buffer is the caller's)
    if (rc == PMV_OK && rc2 != PMV_OK) { pmv_pipeline_free(*out); *out = nullptr; return rc2; }
    return rc;
}

int pmv_pipeline_run(pmv_ctx* ctx, const pmv_pipeline_params* P, const double* K9, const double* gt_poses12,
                     pmv_pipeline_result** out) {
    if (!ctx || !P || !K9 || !gt_poses12 || !out) { pmv::set_err(ctx, "pmv_pipeline_run: null argument"); return PMV_ERR_INVALID; }
    host_allocator_setup();
    if (P->n_frames < P->init_frames + 2 || P->n_frames > ctx->n_slots || P->init_frames < 1) {
        pmv::set_err(ctx, "pmv_pipeline_run: n_frames=%d (slots %d, init_frames %d)", P->n_frames, ctx->n_slots, P->init_frames);
        return PMV_ERR_CAPACITY;
    }
    if (const int rc = check_params(ctx, "pmv_pipeline_run", *P, false)) return rc;
    auto* res = new pmv_pipeline_result();
    vo::PipelineRun& run = res->run;
    const vo::PipelineParams vp = params_of(P, P->n_threads);
    try {
        if (P->build_pyramids) ck(ctx, pmv_frames_build(ctx, 0, P->n_frames));
        vo::pipeline_setup(run, vp, nullptr, K9, gt_poses12);
        plug_in(run, P, Route{ctx}, std::max(1, P->n_threads));
        vo::pipeline_execute(run, vp);
    } catch (const HipError& e) {
        pmv::set_err(ctx, "pmv_pipeline_run: %s", e.what());
        const int code = e.code;
        delete res;
        return code;
    } catch (const std::exception& e) {
        pmv::set_err(ctx, "pmv_pipeline_run: %s", e.what());
        delete res;
        return PMV_ERR_INVALID;
    }
    *out = res;
    return PMV_OK;
}
// B independent sequences in one go. Sequence b uses frame slots first_slot[b] .. first_slot[b] + params[b].n_frames - 1
// (staged with pmv_frames_stage, each sequence in its own frame size params[b].w x h), its own K9 (9 doubles at K9 + 9 b) and ground-truth rows.
// Every sequence runs the reference's two host threads (front-end / back-end) with the unchanged adapters; their plugin calls are
// merged by the context's batch engine into batched launches. out[b] receives sequence b's result, bit-identical to its own
// pmv_pipeline_run. On error every result that exists is freed and the first error is returned.
int pmv_pipeline_run_batch(pmv_ctx* ctx, int B, const pmv_pipeline_params* params, const double* K9, const double* const* gt_poses12,
                           const int* first_slot, pmv_pipeline_result** out) {
    if (!ctx || !params || !K9 || !gt_poses12 || !first_slot || !out || B < 1) { pmv::set_err(ctx, "pmv_pipeline_run_batch: bad argument"); return PMV_ERR_INVALID; }
    if (ctx->session_state.load() != 0) { pmv::set_err(ctx, "pmv_pipeline_run_batch: a batch session is open on this context (pmv_batch_close first): it owns the batch engine and the geometry table"); return PMV_ERR_INVALID; }
    host_allocator_setup();
    std::vector<int> ring((size_t)B);
    for (int b = 0; b < B; b++) {
        const pmv_pipeline_params& P = params[b];
        out[b] = nullptr;
        if (P.n_frames < P.init_frames + 2 || P.init_frames < 1 || first_slot[b] < 0 || first_slot[b] + P.n_frames > ctx->n_slots) {
            pmv::set_err(ctx, "pmv_pipeline_run_batch: sequence %d: frames [%d, %d) outside the %d slots / too short", b, first_slot[b], first_slot[b] + P.n_frames, ctx->n_slots);
            return PMV_ERR_CAPACITY;
        }
        if (P.w < 40 || P.h < 40 || P.w > ctx->max_w || P.h > ctx->max_h) {   // (before the slots are looked at: a size no slot can hold)
            pmv::set_err(ctx, "pmv_pipeline_run_batch: sequence %d: frame %dx%d outside capacity %dx%d", b, P.w, P.h, ctx->max_w, ctx->max_h);
            return PMV_ERR_CAPACITY;
        }
        for (int i = 0; i < P.n_frames; i++) {   // the geometry actually staged in the slots, not only the parameter structs
            const pmv::PyrLayout& Ls = ctx->slot_layout[first_slot[b] + i];
            const bool empty = ctx->slot_state[first_slot[b] + i] == pmv::SLOT_EMPTY;
            // (also what makes overlapping ranges agree: a shared slot holds one size, which every sequence over it must name)
            if (empty || Ls.w[0] != P.w || Ls.h[0] != P.h) {
                pmv::set_err(ctx, "pmv_pipeline_run_batch: sequence %d: slot %d holds %s (%dx%d), the sequence is %dx%d", b, first_slot[b] + i,
                             empty ? "no frame" : "a frame of another size", Ls.w[0], Ls.h[0], P.w, P.h);
                return PMV_ERR_INVALID;
            }
        }
        ring[(size_t)b] = P.n_frames;
    }
    // the pyramids of the sequences with build_pyramids are built by the feeder, round by round, while the sequences already track
    return run_batch(ctx, "pmv_pipeline_run_batch", B, params, K9, gt_poses12, nullptr, first_slot, ring.data(), out);
}
// The same B sequences from HOST memory through per-sequence rings of `ring` slots (ingest_batch.hip): sequence b owns slots
// first_slot[b] .. first_slot[b] + ring - 1, frame f lives in first_slot[b] + f % ring. Validation as in pmv_pipeline_run_batch, plus the
// ring rules of include/pmv_hip.h. out[b] is bit-identical to the staged batch's and to the sequence's own pmv_pipeline_run.
int pmv_pipeline_run_batch_streamed(pmv_ctx* ctx, int B, const pmv_pipeline_params* params, const double* K9, const double* const* gt_poses12,
                                    const uint8_t* const* host_frames, const int* first_slot, int ring, pmv_pipeline_result** out) {
    if (!ctx || !params || !K9 || !gt_poses12 || !host_frames || !first_slot || !out || B < 1) { pmv::set_err(ctx, "pmv_pipeline_run_batch_streamed: bad argument"); return PMV_ERR_INVALID; }
    if (ctx->session_state.load() != 0) { pmv::set_err(ctx, "pmv_pipeline_run_batch_streamed: a batch session is open on this context (pmv_batch_close first): it owns the batch engine and the geometry table"); return PMV_ERR_INVALID; }
    if (pmv::batch_ingest_active(ctx->ingest)) { pmv::set_err(ctx, "pmv_pipeline_run_batch_streamed: a pmv_frames_stream_begin bracket is open on this context"); return PMV_ERR_INVALID; }
    host_allocator_setup();
    for (int b = 0; b < B; b++) out[b] = nullptr;
    std::vector<std::pair<int, int>> ranges;
    for (int b = 0; b < B; b++) {
        const pmv_pipeline_params& P = params[b];
        if (!host_frames[b] || !gt_poses12[b]) { pmv::set_err(ctx, "pmv_pipeline_run_batch_streamed: sequence %d: null frames / poses", b); return PMV_ERR_INVALID; }
        if (P.n_frames < P.init_frames + 2 || P.init_frames < 1) { pmv::set_err(ctx, "pmv_pipeline_run_batch_streamed: sequence %d: %d frames, init_frames %d: too short", b, P.n_frames, P.init_frames); return PMV_ERR_CAPACITY; }
        // initialise() holds frames 0 .. init_frames - 1, and the first addFrame may need frame init_frames while frame init_offset is live
        if (ring < P.init_frames + 1) { pmv::set_err(ctx, "pmv_pipeline_run_batch_streamed: ring %d < init_frames + 1 = %d", ring, P.init_frames + 1); return PMV_ERR_INVALID; }
        if (first_slot[b] < 0 || first_slot[b] > ctx->n_slots - ring) {
            pmv::set_err(ctx, "pmv_pipeline_run_batch_streamed: sequence %d: ring [%d, %d) outside the %d slots", b, first_slot[b], first_slot[b] + ring, ctx->n_slots);
            return PMV_ERR_CAPACITY;
        }
        ranges.push_back({first_slot[b], b});
        hipPointerAttribute_t attr;
        const bool device_mem = hipPointerGetAttributes(&attr, host_frames[b]) == hipSuccess && attr.type == hipMemoryTypeDevice;
        (void)hipGetLastError();
        if (device_mem) { pmv::set_err(ctx, "pmv_pipeline_run_batch_streamed: sequence %d: the frames are in device memory, not host memory", b); return PMV_ERR_INVALID; }
    }
    std::sort(ranges.begin(), ranges.end());
    for (size_t i = 1; i < ranges.size(); i++)
        if (ranges[i].first < ranges[i - 1].first + ring) {
            pmv::set_err(ctx, "pmv_pipeline_run_batch_streamed: the rings of sequences %d and %d overlap", ranges[i - 1].second, ranges[i].second);
            return PMV_ERR_INVALID;
        }
    const std::vector<int> rings((size_t)B, ring);
    return run_batch(ctx, "pmv_pipeline_run_batch_streamed", B, params, K9, gt_poses12, host_frames, first_slot, rings.data(), out);
}
// diagnostic: launches of the batched legs since the context was created (pmv_ctx::batch_launches)
int pmv_debug_batch_launches(pmv_ctx* ctx, long long* out4) {
    if (!ctx || !out4) return PMV_ERR_INVALID;
    for (int i = 0; i < 4; i++) out4[i] = ctx->batch_launches[i].load();
    return PMV_OK;
}
int pmv_debug_whole_rounds(pmv_ctx* ctx, long long* out3) {
    if (!ctx || !out3) return PMV_ERR_INVALID;
    for (int i = 0; i < 3; i++) out3[i] = ctx->whole_rounds[i].load();
    return PMV_OK;
}
int pmv_batch_ingest_stats(pmv_ctx* ctx, double* out) {
    if (!out) return pmv::BATCH_INGEST_STATS;
    if (!ctx) return PMV_ERR_INVALID;
    for (int i = 0; i < pmv::BATCH_INGEST_STATS; i++) out[i] = ctx->bingest_stats[i];
    return pmv::BATCH_INGEST_STATS;
}
// diagnostic: what the five combiners (LK, detectors, PnP, BA, DLT) have served so far
int pmv_batch_stats(pmv_ctx* ctx, long long* counts10, double* times15) {
    if (!ctx || !counts10) return PMV_ERR_INVALID;
    for (int i = 0; i < 10; i++) counts10[i] = 0;
    if (times15) for (int i = 0; i < 15; i++) times15[i] = 0;
    if (ctx->engine) pmv::batch_engine_stats(ctx->engine, counts10, times15);
    return PMV_OK;
}
void pmv_pipeline_free(pmv_pipeline_result* r) { delete r; }
// Tearing down ~10^6 host container nodes of a 1100-frame run takes ~40 ms and is not part of the path: a result can be
// handed to a background thread instead. pmv_pipeline_drain() waits for all outstanding releases.
static std::mutex g_release_mu;
static std::vector<std::thread> g_release_threads;
void pmv_pipeline_release(pmv_pipeline_result* r) {
    if (!r) return;
    std::lock_guard<std::mutex> lk(g_release_mu);
    g_release_threads.emplace_back([r] { delete r; });
}
void pmv_pipeline_drain(void) {
    std::vector<std::thread> th;
    { std::lock_guard<std::mutex> lk(g_release_mu); th.swap(g_release_threads); }
    for (auto& t : th) t.join();
}
int pmv_pipeline_num_poses(const pmv_pipeline_result* r) { return vo::pipeline_num_poses(r->run); }
void pmv_pipeline_get_poses(const pmv_pipeline_result* r, double* out) { vo::pipeline_get_poses(r->run, out); }
int pmv_pipeline_num_frames(const pmv_pipeline_result* r) { return vo::pipeline_num_frames(r->run); }
int pmv_pipeline_frame_feature_count(const pmv_pipeline_result* r, int k) { return vo::pipeline_frame_feature_count(r->run, k); }
void pmv_pipeline_get_frame_features(const pmv_pipeline_result* r, int k, int* out) { vo::pipeline_get_frame_features(r->run, k, out); }
int pmv_pipeline_stats_count(void) { return vo::PIPELINE_STATS_COUNT; }
void pmv_pipeline_get_stats(const pmv_pipeline_result* r, double* out25) { vo::pipeline_get_stats(r->run, out25); }
}
