// C-ABI entry points of the back-end stream: pmv_pnp_ransac, pmv_ba_residuals, pmv_ba_solve (include/pmv_hip.h).
#include "pmv_ctx.h"
#include "backend.h"
#include "pmv_wait.h"
#include "vo_pipeline.h"
#include <cmath>
#include <cstring>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include <algorithm>

namespace pmv {

// Input block of a solve from mapped pinned host memory into HBM: a copy launch on the solve's own stream instead of a DMA-engine
// transfer (hipMemcpyAsync of ~50 KB goes through SDMA: 10-15 us until the first kernel of the chain may start; this is ~5).
__global__ __launch_bounds__(256) void k_stage_block(const uint4* __restrict__ src, uint4* __restrict__ dst, unsigned n16) { BACKEND_PRIO();
    for (unsigned i = blockIdx.x * 256 + threadIdx.x; i < n16; i += gridDim.x * 256) dst[i] = src[i];
}
hipError_t stage_block(hipStream_t s, const void* mapped_src, void* dst, size_t bytes, unsigned max_blocks) {
    const unsigned n16 = (unsigned)((bytes + 15) >> 4);
    hipLaunchKernelGGL(k_stage_block, dim3(std::min(max_blocks, (n16 + 255u) / 256u)), dim3(256), 0, s, (const uint4*)mapped_src, (uint4*)dst, n16);
    return hipGetLastError();
}
// PMV_BA_STAGE=dma: PnP and BA stage their input block with hipMemcpyAsync instead (read once per process)
static bool stage_by_kernel() { static const bool on = !(getenv("PMV_BA_STAGE") && !strcmp(getenv("PMV_BA_STAGE"), "dma")); return on; }

static int round_up(int a, int b) { return (a + b - 1) / b * b; }

int backend_alloc(pmv_ctx* c, BackendBuffers** out) {
    BackendBuffers* b = new BackendBuffers();
    *out = b;
    const size_t nc = (size_t)std::max(c->max_ba_cams, 1), np = (size_t)std::max(c->max_ba_points, 1), no = (size_t)std::max(c->max_ba_obs, 1);
    const size_t n = 6 * nc + 3 * np, m = 6 * nc;
    const size_t ldw = (size_t)round_up((int)m + 1, 16), krows = (size_t)round_up((int)(3 * np), 16);
    b->ydwd_elems = krows * ldw;
    b->gpart_elems = (size_t)8 * ldw * ldw;   // up to 8 K-slices of an (ldw x ldw) tile grid
    const size_t mt = (size_t)c->max_tracks;
    const BackendCaps caps = backend_caps(c->max_tracks, c->max_ba_cams, c->max_ba_points, c->max_ba_obs);   // the staging blocks: the layouts at capacity
    // THE list of a workspace set's buffers
    const MemRow rows[] = {
        {&b->d_cams, nc * 6 * 8, MEM_DEVICE}, {&b->d_pts, np * 3 * 8, MEM_DEVICE}, {&b->d_obs, no * 2 * 8, MEM_DEVICE}, {&b->d_K, 9 * 8, MEM_DEVICE},
        {&b->d_cam_idx, no * 4, MEM_DEVICE}, {&b->d_pt_idx, no * 4, MEM_DEVICE},
        {&b->d_pobs_start, (np + 1) * 4, MEM_DEVICE}, {&b->d_pobs_list, no * 4, MEM_DEVICE},
        {&b->d_cobs_start, (nc + 1) * 4, MEM_DEVICE}, {&b->d_cobs_list, no * 4, MEM_DEVICE},
        {&b->d_x, 2 * n * 8, MEM_DEVICE}, {&b->d_cand, n * 8, MEM_DEVICE}, {&b->d_scale, n * 8, MEM_DEVICE}, {&b->d_diag, n * 8, MEM_DEVICE},
        {&b->d_D2, n * 8, MEM_DEVICE}, {&b->d_step, n * 8, MEM_DEVICE},
        {&b->d_res, 2 * no * 2 * 8, MEM_DEVICE}, {&b->d_J, 2 * no * 18 * 8, MEM_DEVICE},   // two buffers: current point / candidate
        {&b->d_Einv, np * 9 * 8, MEM_DEVICE}, {&b->d_gp, np * 3 * 8, MEM_DEVICE},
        {&b->d_Yd, 2 * b->ydwd_elems * 8, MEM_DEVICE},   // Yt | [Wt | g] adjacent: one clear per solve (multi-kernel LM)
        {&b->d_Wd, b->ydwd_elems * 8, MEM_DEVICE},       // [Wt | g] of the single-workgroup LM
        {&b->d_S, m * m * 8, MEM_DEVICE}, {&b->d_rhs, m * 8, MEM_DEVICE},
        {&b->d_Gpart, b->gpart_elems * 8, MEM_DEVICE},
        {&b->d_summary, 8 * 8, MEM_DEVICE},
        {&b->d_stamps, 32 * 8, MEM_DEVICE},
        {&b->d_bastate, 512 + 4 * BA_MAX_ITERATIONS, MEM_DEVICE},
        {&b->d_bapart, ((size_t)(no + 255) / 256 + 5 * ((size_t)(np + 63) / 64) + 64 * (size_t)nc + 3 * (size_t)no + 64) * 8, MEM_DEVICE},
        {&b->d_obj, mt * 12, MEM_DEVICE}, {&b->d_img, mt * 8, MEM_DEVICE},
        {&b->d_samples, MAX_HYP * 5 * 4, MEM_DEVICE}, {&b->d_counts, MAX_HYP * 4, MEM_DEVICE},
        {&b->d_inliers, mt * 4, MEM_DEVICE}, {&b->d_info, 16, MEM_DEVICE},
        {&b->d_models, MAX_HYP * 6 * 8, MEM_DEVICE}, {&b->d_rt, 6 * 8, MEM_DEVICE}, {&b->d_Kp, 9 * 8, MEM_DEVICE},
        {&b->d_masks, (size_t)MAX_HYP * mt, MEM_DEVICE},
        {&b->d_ba_io, caps.ba_io, MEM_DEVICE},
        {&b->d_pnp_in, caps.pnp_in, MEM_DEVICE}, {&b->d_pnp_out, caps.pnp_out, MEM_DEVICE},
        {&b->d_tri_in, caps.tri_in, MEM_DEVICE}, {&b->d_tri_out, caps.tri_out, MEM_DEVICE},
        {&b->d_fp_work, (size_t)FP_MAX_HYP * (90 * 8 + 4) + 64, MEM_DEVICE},
        {&b->d_ess_in, caps.ess_in, MEM_DEVICE},
        {&b->d_tt_in, caps.tt_in, MEM_DEVICE},
        {&b->h_stage, caps.h_stage, MEM_MAPPED},
    };
    hipError_t e = mem_alloc_table(rows, sizeof(rows) / sizeof(rows[0]));
    if (e == hipSuccess) e = hipMemset(b->d_stamps, 0, 32 * 8);
    if (e != hipSuccess) { set_err(c, "backend_alloc: %s", hipGetErrorString(e)); return PMV_ERR_HIP; }
    return PMV_OK;
}
int backend_create(pmv_ctx* c) { return backend_alloc(c, &c->be); }

void backend_free(BackendBuffers* b) { delete b; }
void backend_destroy(pmv_ctx* c) {
    if (c->s_ahead) { (void)hipStreamSynchronize(c->s_ahead); (void)hipStreamDestroy(c->s_ahead); c->s_ahead = nullptr; }   // (before its workspaces go)
    backend_free(c->be); c->be = nullptr;
    backend_free(c->be_ahead); c->be_ahead = nullptr;
}

// cv::RNG (multiply-with-carry) and RANSACPointSetRegistrator::getSubset (5 distinct indices)
struct CvRNG {
    uint64_t state;
    explicit CvRNG(uint64_t s) : state(s ? s : 0xffffffffULL) {}
    unsigned next() { state = (uint64_t)(unsigned)state * 4164903690U + (unsigned)(state >> 32); return (unsigned)state; }
    int uniform(int a, int b) { return a == b ? a : (int)(next() % (unsigned)(b - a) + a); }
};

}  // namespace pmv

using namespace pmv;

#define CKC(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { set_err(ctx, "%s: %s", #x, hipGetErrorString(e_)); return PMV_ERR_HIP; } } while (0)
#define REQ(cond, code, ...) do { if (!(cond)) { set_err(ctx, __VA_ARGS__); return code; } } while (0)

// ---- PnP: prepare (host slab + device problem record) / finish (results out of the pinned block), shared by the single call
// and by the batch engine (several sequences' calls in one launch) ------------------------------------------------------------
int pmv::pnp_check(pmv_ctx* ctx, const float* obj_xyz, const float* img_xy, int m, const double* K, double* rvec, double* tvec, int iterations,
                   double confidence, int* out_inliers, int* out_n_inliers) {
    REQ(ctx && obj_xyz && img_xy && K && rvec && tvec && out_inliers && out_n_inliers, PMV_ERR_INVALID, "pmv_pnp_ransac: null argument");
    *out_n_inliers = 0;
    REQ(m <= ctx->max_tracks, PMV_ERR_CAPACITY, "pmv_pnp_ransac: m=%d exceeds max_tracks=%d", m, ctx->max_tracks);
    // cv::solvePnPRansac asserts npoints >= 4; with 4 points it switches to P3P, with 5 it runs the kernel once (not built: the
    // reference only calls it with >= tracked_features_tol points)
    REQ(m >= 6, PMV_ERR_DEGENERATE, "pmv_pnp_ransac: %d correspondences (need >= 6)", m);
    REQ(iterations >= 1 && iterations <= MAX_HYP, PMV_ERR_CAPACITY, "pmv_pnp_ransac: iterations=%d (1..%d)", iterations, MAX_HYP);
    REQ(confidence > 0 && confidence < 1, PMV_ERR_INVALID, "pmv_pnp_ransac: confidence must be in (0,1)");
    return PMV_OK;
}
// packs pnp_layout's in-block [K 10 doubles, 10^k for k = -16..16 (CvLevMarq's lambda) | obj 3m floats | img 2m floats | samples 5*iterations
// ints] into b's pinned block and describes the problem with b's device buffers; L->in_bytes = bytes to copy h_stage -> d_pnp_in
int pmv::pnp_prepare(pmv_ctx* ctx, BackendBuffers* b, const float* obj_xyz, const float* img_xy, int m, const double* K, int iterations, float reproj_err,
                     double confidence, PnPProblem* P, PnPLayout* Lout) {
    const PnPLayout L = pnp_layout((size_t)m, (size_t)iterations);
    REQ(L.total <= b->h_stage.cap && L.in_bytes <= b->d_pnp_in.cap && L.total - L.out <= b->d_pnp_out.cap, PMV_ERR_CAPACITY,
        "pmv_pnp_ransac: m=%d with %d iterations does not fit the staging blocks", m, iterations);
    char* hs = (char*)b->h_stage;
    double* h_K = (double*)(hs + L.K);
    int* h_samples = (int*)(hs + L.samples);
    memcpy(h_K, K, 72);
    for (int k = -16; k <= 16; k++) h_K[10 + 16 + k] = std::exp(k * std::log(10.));   // as CvLevMarq::step evaluates it (host libm)
    memcpy(hs + L.obj, obj_xyz, (size_t)m * 12);
    memcpy(hs + L.img, img_xy, (size_t)m * 8);
    CvRNG rng((uint64_t)-1);
    for (int it = 0; it < iterations; it++) {
        int* idx = h_samples + it * 5;
        for (int i = 0; i < 5;) {
            int idx_i;
            for (;;) {
                idx_i = idx[i] = rng.uniform(0, m);
                int j = 0;
                for (; j < i; j++) if (idx_i == idx[j]) break;
                if (j == i) break;
            }
            i++;
        }
    }
    P->K = (const double*)(b->d_pnp_in + L.K);
    P->obj = (const float*)(b->d_pnp_in + L.obj);
    P->img = (const float*)(b->d_pnp_in + L.img);
    P->samples = (const int*)(b->d_pnp_in + L.samples);
    P->models = b->d_models; P->masks = b->d_masks; P->counts = b->d_counts;
    P->rt_out = (double*)b->d_pnp_out;
    P->info = (int*)(b->d_pnp_out + PNP_OUT_INFO);
    P->inliers = (int*)(b->d_pnp_out + PNP_OUT_INLIERS);
    P->host_out = b->h_stage.dm() + L.out;   // the refit kernel writes [PnPResultHdr | inliers] straight into the pinned block
    P->m = m; P->n_hyp = iterations;
    P->thr = (float)((double)reproj_err * (double)reproj_err);
    P->confidence = confidence;
    *Lout = L;
    return PMV_OK;
}
void pmv::pnp_finish(pmv_ctx* ctx, BackendBuffers* b, const float* obj_xyz, const float* img_xy, int m, const double* K, double* rvec, double* tvec,
                     int iterations, float reproj_err, double confidence, const PnPLayout& L, int* out_inliers, int* out_n_inliers) {
    const PnPResultHdr* R = (const PnPResultHdr*)((const char*)b->h_stage + L.out);
    const double* h_rt = R->rt;
    const int* h_inl = (const int*)((const char*)b->h_stage + L.inliers);
    const int n = R->info[0];
    if (ctx->log.on) {   // [kind 0, m, iterations, n_inliers | obj 3m f32 | img 2m f32 | K 9, rvec_in 3, tvec_in 3, reproj_err, confidence f64 | rvec_out 3, tvec_out 3 f64 | inliers]
        std::lock_guard<std::mutex> lk(ctx->log.mu);
        ctx->log.blobs.emplace_back();
        std::vector<char>& bl = ctx->log.blobs.back();
        const int hdr[4] = {0, m, iterations, n};
        const double opt[2] = {(double)reproj_err, confidence};
        pmv_call_log::put(bl, hdr, 16); pmv_call_log::put(bl, obj_xyz, (size_t)m * 12); pmv_call_log::put(bl, img_xy, (size_t)m * 8);
        pmv_call_log::put(bl, K, 72); pmv_call_log::put(bl, rvec, 24); pmv_call_log::put(bl, tvec, 24); pmv_call_log::put(bl, opt, 16);
        pmv_call_log::put(bl, h_rt, 48); pmv_call_log::put(bl, h_inl, (size_t)(n > 0 ? n : 0) * 4);
    }
    for (int i = 0; i < 3; i++) { rvec[i] = h_rt[i]; tvec[i] = h_rt[3 + i]; }
    *out_n_inliers = n;
    if (n > 0) memcpy(out_inliers, h_inl, (size_t)n * 4);
}

// Waits for a kernel's last store, the call's sequence number in its result block (spin_for_word), or, with by_word false, for the stream
static int wait_done_word(pmv_ctx* ctx, hipStream_t s, volatile unsigned* done_word, unsigned done_seq, bool by_word) {
    if (by_word) CKC(spin_for_word(s, done_word, done_seq));
    else CKC(hipStreamSynchronize(s));
    return PMV_OK;
}

extern "C" {

static bool stamps_on() { static const bool on = getenv("PMV_BA_STAMPS") != nullptr; return on; }

int pmv_pnp_ransac(pmv_ctx* ctx, const float* obj_xyz, const float* img_xy, int m, const double* K, double* rvec, double* tvec,
                   int iterations, float reproj_err, double confidence, int* out_inliers, int* out_n_inliers) {
    int rc = pnp_check(ctx, obj_xyz, img_xy, m, K, rvec, tvec, iterations, confidence, out_inliers, out_n_inliers);
    if (rc) return rc;
    tl_prof = &ctx->prof;
    CKC(hipSetDevice(ctx->device));
    static const char* const dump = getenv("PMV_DUMP_PNP");   // (the diagnostic switches are read once per process: getenv walks the whole environment)
    if (dump) {   // debug: append the inputs of every call to a file
        if (FILE* f = fopen(dump, "ab")) {
            fwrite(&m, 4, 1, f); fwrite(obj_xyz, 12, m, f); fwrite(img_xy, 8, m, f); fwrite(K, 8, 9, f); fwrite(rvec, 8, 3, f); fwrite(tvec, 8, 3, f);
            fclose(f);
        }
    }
    BackendBuffers* b = ctx->be;
    hipStream_t s = ctx->s_back;
    PnPProblem P;
    PnPLayout L;
    if ((rc = pnp_prepare(ctx, b, obj_xyz, img_xy, m, K, iterations, reproj_err, confidence, &P, &L))) return rc;
    if (stage_by_kernel()) CKC(stage_block(s, b->h_stage.dm(), b->d_pnp_in, L.in_bytes, 8));
    else CKC(hipMemcpyAsync(b->d_pnp_in, b->h_stage, L.in_bytes, hipMemcpyHostToDevice, s));
    // the refit kernel writes [PnPResultHdr | inliers] straight into the pinned block and, last, this call's sequence number into the
    // header's done word: the result is read as soon as that store lands (PMV_BACK_WAIT=sync: hipStreamSynchronize instead)
    const bool flag_wait = back_wait_by_word();
    volatile unsigned* done_word = (volatile unsigned*)((char*)b->h_stage + L.done);
    if (++b->done_seq == 0) b->done_seq = 1;
    *done_word = 0;
    CKC(launch_pnp(s, P.obj, P.img, m, P.K, P.samples, iterations, P.thr, confidence, P.models, P.masks, P.counts,
                   P.rt_out, P.inliers, P.info, P.host_out, stamps_on() ? b->d_stamps : nullptr, flag_wait ? b->done_seq : 0u));
    if ((rc = wait_done_word(ctx, s, done_word, b->done_seq, flag_wait))) return rc;
    pnp_finish(ctx, b, obj_xyz, img_xy, m, K, rvec, tvec, iterations, reproj_err, confidence, L, out_inliers, out_n_inliers);
    return PMV_OK;
}

// ---- call log (teacher-forced replay of a pipeline run's back-end calls through another implementation) ----------------
int pmv_record_enable(pmv_ctx* ctx, int on) {
    REQ(ctx, PMV_ERR_INVALID, "null ctx");
    if (on) ctx->log.blobs.clear();
    ctx->log.on = on != 0;
    return PMV_OK;
}
int pmv_record_count(pmv_ctx* ctx) { return ctx ? (int)ctx->log.blobs.size() : PMV_ERR_INVALID; }
long long pmv_record_size(pmv_ctx* ctx, int i) {
    if (!ctx || i < 0 || i >= (int)ctx->log.blobs.size()) return PMV_ERR_INVALID;
    return (long long)ctx->log.blobs[i].size();
}
int pmv_record_get(pmv_ctx* ctx, int i, void* out, long long capacity) {
    REQ(ctx && out && i >= 0 && i < (int)ctx->log.blobs.size(), PMV_ERR_INVALID, "pmv_record_get: bad argument");
    REQ(capacity >= (long long)ctx->log.blobs[i].size(), PMV_ERR_CAPACITY, "pmv_record_get: buffer too small");
    memcpy(out, ctx->log.blobs[i].data(), ctx->log.blobs[i].size());
    return PMV_OK;
}

// diagnostic: accumulated per-phase shader-clock counters of k_ba_lm (enabled by PMV_BA_STAMPS=1), 32 values
int pmv_debug_ba_stamps(pmv_ctx* ctx, unsigned long long* out32) {
    REQ(ctx && out32, PMV_ERR_INVALID, "null argument");
    CKC(hipSetDevice(ctx->device));
    CKC(hipStreamSynchronize(ctx->s_back));
    CKC(hipMemcpy(out32, ctx->be->d_stamps, 256, hipMemcpyDeviceToHost));
    return PMV_OK;
}

// debug/parity: models (n x 6) and inlier counts of the hypotheses evaluated by the last pmv_pnp_ransac call
int pmv_debug_pnp_hypotheses(pmv_ctx* ctx, int n, double* models, int* counts) {
    REQ(ctx && models && counts && n >= 1 && n <= MAX_HYP, PMV_ERR_INVALID, "pmv_debug_pnp_hypotheses: bad argument");
    CKC(hipSetDevice(ctx->device));
    CKC(hipStreamSynchronize(ctx->s_back));
    CKC(hipMemcpy(models, ctx->be->d_models, (size_t)n * 48, hipMemcpyDeviceToHost));
    CKC(hipMemcpy(counts, ctx->be->d_counts, (size_t)n * 4, hipMemcpyDeviceToHost));
    return PMV_OK;
}

int pmv_ba_residuals(pmv_ctx* ctx, const double* cams, int nc, const double* pts, int np, const double* obs_xy, const int* cam_idx,
                     const int* pt_idx, int n_obs, const double* K, double* out_r, double* out_J) {
    REQ(ctx && cams && pts && obs_xy && cam_idx && pt_idx && K && out_r && out_J, PMV_ERR_INVALID, "pmv_ba_residuals: null argument");
    REQ(nc >= 1 && nc <= ctx->max_ba_cams && np >= 1 && np <= ctx->max_ba_points && n_obs >= 0 && n_obs <= ctx->max_ba_obs, PMV_ERR_CAPACITY,
        "pmv_ba_residuals: nc=%d np=%d n_obs=%d exceed capacity %d/%d/%d", nc, np, n_obs, ctx->max_ba_cams, ctx->max_ba_points, ctx->max_ba_obs);
    for (int i = 0; i < n_obs; i++) REQ(cam_idx[i] >= 0 && cam_idx[i] < nc && pt_idx[i] >= 0 && pt_idx[i] < np, PMV_ERR_INVALID, "pmv_ba_residuals: index out of range at observation %d", i);
    if (n_obs == 0) return PMV_OK;
    tl_prof = &ctx->prof;
    CKC(hipSetDevice(ctx->device));
    BackendBuffers* b = ctx->be;
    hipStream_t s = ctx->s_back;
    CKC(hipMemcpyAsync(b->d_cams, cams, (size_t)nc * 48, hipMemcpyHostToDevice, s));
    CKC(hipMemcpyAsync(b->d_pts, pts, (size_t)np * 24, hipMemcpyHostToDevice, s));
    CKC(hipMemcpyAsync(b->d_obs, obs_xy, (size_t)n_obs * 16, hipMemcpyHostToDevice, s));
    CKC(hipMemcpyAsync(b->d_cam_idx, cam_idx, (size_t)n_obs * 4, hipMemcpyHostToDevice, s));
    CKC(hipMemcpyAsync(b->d_pt_idx, pt_idx, (size_t)n_obs * 4, hipMemcpyHostToDevice, s));
    CKC(hipMemcpyAsync(b->d_K, K, 72, hipMemcpyHostToDevice, s));
    CKC(launch_ba_residuals(s, b->d_cams, b->d_pts, b->d_obs, b->d_cam_idx, b->d_pt_idx, n_obs, b->d_K, b->d_res, b->d_J));
    CKC(hipMemcpyAsync(out_r, b->d_res, (size_t)n_obs * 16, hipMemcpyDeviceToHost, s));
    CKC(hipMemcpyAsync(out_J, b->d_J, (size_t)n_obs * 144, hipMemcpyDeviceToHost, s));
    CKC(hipStreamSynchronize(s));
    return PMV_OK;
}

}  // extern "C"

// ---- BA: check / prepare (pinned io block, observation lists, BAArgs over b's workspaces) / finish -------------------------------
int pmv::ba_check(pmv_ctx* ctx, const double* cams, int nc, const double* pts, int np, const double* obs_xy, const int* cam_idx, const int* pt_idx,
                  int n_obs, const double* K, double huber_delta, int max_iterations) {
    REQ(ctx && cams && pts && obs_xy && cam_idx && pt_idx && K, PMV_ERR_INVALID, "pmv_ba_solve: null argument");
    REQ(nc >= 1 && nc <= ctx->max_ba_cams && np >= 1 && np <= ctx->max_ba_points && n_obs >= 1 && n_obs <= ctx->max_ba_obs, PMV_ERR_CAPACITY,
        "pmv_ba_solve: nc=%d np=%d n_obs=%d exceed capacity %d/%d/%d", nc, np, n_obs, ctx->max_ba_cams, ctx->max_ba_points, ctx->max_ba_obs);
    REQ(max_iterations >= 0 && max_iterations <= BA_MAX_ITERATIONS && huber_delta > 0, PMV_ERR_INVALID, "pmv_ba_solve: bad options");
    for (int i = 0; i < n_obs; i++)
        REQ(cam_idx[i] >= 0 && cam_idx[i] < nc && pt_idx[i] >= 0 && pt_idx[i] < np, PMV_ERR_INVALID, "pmv_ba_solve: index out of range at observation %d", i);
    const int m = 6 * nc;
    REQ(((size_t)(m + 1) * m + (size_t)m) * 8 <= 150 * 1024, PMV_ERR_CAPACITY, "pmv_ba_solve: %d cameras exceed the LDS-resident reduced system (max 22)", nc);
    return PMV_OK;
}
int pmv::ba_prepare(pmv_ctx* ctx, BackendBuffers* b, const double* cams, int nc, const double* pts, int np, const double* obs_xy, const int* cam_idx,
                    const int* pt_idx, int n_obs, const double* K, double huber_delta, int max_iterations, bool multi, BAArgs* Aout, BaIoLayout* Lout) {
    // one pinned block mirrors the device block (ba_io_layout)
    const BaIoLayout L = ba_io_layout((size_t)nc, (size_t)np, (size_t)n_obs);
    REQ(L.total <= b->d_ba_io.cap && L.total <= b->h_stage.cap, PMV_ERR_CAPACITY, "pmv_ba_solve: io block too small");
    char* hs = (char*)b->h_stage;
    double* h_cams = (double*)(hs + L.cams); double* h_pts = (double*)(hs + L.pts); double* h_obs = (double*)(hs + L.obs); double* h_K = (double*)(hs + L.K);
    int* h_ci = (int*)(hs + L.cam_idx); int* h_pi = (int*)(hs + L.pt_idx);
    int* pstart = (int*)(hs + L.pstart); int* plist = (int*)(hs + L.plist); int* cstart = (int*)(hs + L.cstart); int* clist = (int*)(hs + L.clist);
    int* odup = (int*)(hs + L.erec);
    memcpy(h_cams, cams, (size_t)nc * 48); memcpy(h_pts, pts, (size_t)np * 24); memcpy(h_obs, obs_xy, (size_t)n_obs * 16);
    memcpy(h_K, K, 72); memcpy(h_ci, cam_idx, (size_t)n_obs * 4); memcpy(h_pi, pt_idx, (size_t)n_obs * 4);
    // observation lists per point / per camera (counting sort, observation order preserved)
    std::fill(pstart, pstart + np + 1, 0);
    std::fill(cstart, cstart + nc + 1, 0);
    for (int i = 0; i < n_obs; i++) { pstart[pt_idx[i] + 1]++; cstart[cam_idx[i] + 1]++; }
    for (int p = 0; p < np; p++) pstart[p + 1] += pstart[p];
    for (int c = 0; c < nc; c++) cstart[c + 1] += cstart[c];
    {
        std::vector<int> pf(pstart, pstart + np), cf(cstart, cstart + nc);
        for (int i = 0; i < n_obs; i++) { plist[pf[pt_idx[i]]++] = i; clist[cf[cam_idx[i]]++] = i; }
    }
    // a point seen twice by the same camera (the reference's feat_corr duplicates): the first entry carries the group
    for (int p = 0; p < np; p++) {
        for (int e = pstart[p]; e < pstart[p + 1]; e++) {
            const int c = cam_idx[plist[e]];
            bool earlier = false, later = false;
            for (int e2 = pstart[p]; e2 < e; e2++) earlier = earlier || cam_idx[plist[e2]] == c;
            for (int e2 = e + 1; e2 < pstart[p + 1]; e2++) later = later || cam_idx[plist[e2]] == c;
            odup[4 * e] = plist[e]; odup[4 * e + 1] = c; odup[4 * e + 2] = p; odup[4 * e + 3] = earlier ? 2 : (later ? 1 : 0);
        }
    }
    const int m = 6 * nc;
    const int tiles_r = (m + 15) / 16, tiles_c = (m + 1 + 15) / 16;
    char* dio = b->d_ba_io;
    BAArgs A;
    A.cams = (double*)(dio + L.cams); A.pts = (double*)(dio + L.pts); A.obs = (const double*)(dio + L.obs); A.K = (const double*)(dio + L.K);
    A.cam_idx = (const int*)(dio + L.cam_idx); A.pt_idx = (const int*)(dio + L.pt_idx);
    A.pobs_start = (const int*)(dio + L.pstart); A.pobs_list = (const int*)(dio + L.plist); A.cobs_start = (const int*)(dio + L.cstart); A.cobs_list = (const int*)(dio + L.clist);
    A.erec = (const int4*)(dio + L.erec);
    A.nc = nc; A.np = np; A.nobs = n_obs; A.max_iterations = max_iterations; A.huber = huber_delta;
    A.x = b->d_x; A.cand = b->d_cand; A.scale = b->d_scale; A.diag = b->d_diag; A.D2 = b->d_D2; A.step = b->d_step; A.res = b->d_res; A.J = b->d_J;
    A.Einv = b->d_Einv; A.gp = b->d_gp; A.Yd = b->d_Yd; A.Wd = b->d_Wd; A.S = b->d_S; A.rhs = b->d_rhs; A.Gpart = b->d_Gpart; A.summary = (double*)(dio + L.summary);
    A.stamps = stamps_on() ? b->d_stamps : nullptr;
    A.out = nullptr;
    A.done_seq = 0;
    A.tiles_r = tiles_r; A.tiles_c = tiles_c;
    A.ldw = A.tiles_c * 16;
    A.krows = round_up(3 * np, 16);
    A.gp_rows = A.tiles_r * 16;
    int ks = 8 / (A.tiles_r * A.tiles_c);
    if (ks < 1) ks = 1;
    if (ks > 8) ks = 8;
    if (multi) ks = 8;   // multi-kernel paths: one wavefront per (tile, K-slice) anywhere on the chip
    A.kper = round_up((A.krows + ks - 1) / ks, 16);
    A.kslices = (A.krows + A.kper - 1) / A.kper;
    REQ((size_t)A.krows * A.ldw <= b->ydwd_elems && (size_t)A.kslices * A.gp_rows * A.ldw <= b->gpart_elems, PMV_ERR_CAPACITY, "pmv_ba_solve: workspace too small");
    if (multi) {
        A.Wd = A.Yd + (size_t)A.krows * A.ldw;
        A.out = (double*)b->h_stage.dm();   // [summary | cams | pts] of the result, straight into the pinned block
    }
    *Aout = A;
    *Lout = L;
    return PMV_OK;
}
void pmv::ba_finish(pmv_ctx* ctx, BackendBuffers* b, double* cams, int nc, double* pts, int np, const double* obs_xy, const int* cam_idx,
                    const int* pt_idx, int n_obs, const double* K, double huber_delta, int max_iterations, const BaIoLayout& L, pmv_ba_summary* summary) {
    const char* hs = (const char*)b->h_stage;
    const double* h_out = (const double*)(hs + L.summary);
    const double* h_cams = (const double*)(hs + L.cams);
    static const bool ba_trace = getenv("PMV_BA_TRACE") != nullptr;
    if (ba_trace) {   // diagnostic: first / last camera before and after the solve
        fprintf(stderr, "[ba-trace] nc=%d np=%d nobs=%d cost %.15g -> %.15g it %d ok %d\n", nc, np, n_obs, h_out[0], h_out[1], (int)h_out[2], (int)h_out[3]);
        for (int c : {0, nc - 1}) {
            fprintf(stderr, "[ba-trace]   cam %d in ", c);
            for (int k = 0; k < 6; k++) fprintf(stderr, " %.15g", cams[6 * c + k]);
            fprintf(stderr, "\n[ba-trace]   cam %d out", c);
            for (int k = 0; k < 6; k++) fprintf(stderr, " %.15g", h_cams[6 * c + k]);
            fprintf(stderr, "\n");
        }
    }
    if (ctx->log.on) {   // [kind 1, nc, np, n_obs, max_iterations | cams_in 6nc, pts_in 3np, obs 2n_obs, K 9, huber f64 | cam_idx, pt_idx i32 | cams_out, pts_out, summary 5 f64]
        std::lock_guard<std::mutex> lk(ctx->log.mu);
        ctx->log.blobs.emplace_back();
        std::vector<char>& bl = ctx->log.blobs.back();
        const int hdr[5] = {1, nc, np, n_obs, max_iterations};
        pmv_call_log::put(bl, hdr, 20); pmv_call_log::put(bl, cams, (size_t)nc * 48); pmv_call_log::put(bl, pts, (size_t)np * 24);
        pmv_call_log::put(bl, obs_xy, (size_t)n_obs * 16); pmv_call_log::put(bl, K, 72); pmv_call_log::put(bl, &huber_delta, 8);
        pmv_call_log::put(bl, cam_idx, (size_t)n_obs * 4); pmv_call_log::put(bl, pt_idx, (size_t)n_obs * 4);
        pmv_call_log::put(bl, h_cams, L.out_bytes - L.cams); pmv_call_log::put(bl, h_out, 40);
    }
    memcpy(cams, h_cams, (size_t)nc * 48);
    memcpy(pts, hs + L.pts, (size_t)np * 24);
    if (summary) {
        summary->initial_cost = h_out[0]; summary->final_cost = h_out[1]; summary->iterations = (int)h_out[2];
        summary->successful_steps = (int)h_out[3]; summary->termination = (int)h_out[4];
    }
}

extern "C" {

int pmv_set_ba_mode(pmv_ctx* ctx, int mode) {
    if (!ctx || (mode != 0 && mode != 1)) { set_err(ctx, "pmv_set_ba_mode: mode must be 0 (launch chain) or 1 (one workgroup per solve)"); return PMV_ERR_INVALID; }
    ctx->ba_mode = mode;
    return PMV_OK;
}

int pmv_ba_solve(pmv_ctx* ctx, double* cams, int nc, double* pts, int np, const double* obs_xy, const int* cam_idx, const int* pt_idx,
                 int n_obs, const double* K, double huber_delta, int max_iterations, pmv_ba_summary* summary) {
    int rc = ba_check(ctx, cams, nc, pts, np, obs_xy, cam_idx, pt_idx, n_obs, K, huber_delta, max_iterations);
    if (rc) return rc;
    if (max_iterations == 0) {   // ceres::Solve with max_num_iterations = 0 leaves the parameters untouched (costs are not evaluated here)
        if (summary) { summary->initial_cost = summary->final_cost = 0.0; summary->iterations = 0; summary->successful_steps = 0; summary->termination = 0; }
        return PMV_OK;
    }
    tl_prof = &ctx->prof;
    CKC(hipSetDevice(ctx->device));
    BackendBuffers* b = ctx->be;
    hipStream_t s = ctx->s_back;
    // launch mode: multi (one launch per LM phase, default) | single (one persistent workgroup); PMV_BA_MODE overrides
    static const int mode = [] { const char* e = getenv("PMV_BA_MODE"); if (getenv("PMV_BA_SINGLE")) return 0;
                                 return (e && !strcmp(e, "single")) ? 0 : 1; }();
    const bool single = mode == 0 || ctx->ba_mode == 1;
    BAArgs A;
    BaIoLayout L;
    rc = ba_prepare(ctx, b, cams, nc, pts, np, obs_xy, cam_idx, pt_idx, n_obs, K, huber_delta, max_iterations, !single, &A, &L);
    if (rc) return rc;
    const size_t io_bytes = L.io_bytes;
    char* hs = (char*)b->h_stage;
    static const bool check = getenv("PMV_BA_CHECK") != nullptr;
    // multi-kernel chain: the finish kernel writes the result into hs and, last, this call's sequence number into the low word of summary
    // slot BA_SUM_DONE; the result is read as soon as that store lands (PMV_BACK_WAIT=sync: hipStreamSynchronize instead; see pmv_pnp_ransac)
    const bool flag_wait = back_wait_by_word() && !single && !check;
    volatile unsigned* done_word = (volatile unsigned*)(hs + L.done);
    if (flag_wait) {
        if (++b->done_seq == 0) b->done_seq = 1;
        *(double*)(hs + L.done) = 0.0;
        A.done_seq = b->done_seq;
    }
    if (stage_by_kernel() && !check) CKC(stage_block(s, b->h_stage.dm(), b->d_ba_io, io_bytes, 64));   // (h_stage and d_ba_io are 16-byte aligned and have >= 16 B of slack)
    else CKC(hipMemcpyAsync(b->d_ba_io, hs, io_bytes, hipMemcpyHostToDevice, s));
    std::vector<char> saved;
    if (check) saved.assign(hs, hs + io_bytes);
    if (single) CKC(launch_ba_lm(s, A));
    else CKC(launch_ba_multi(s, A, b->d_bastate, b->d_bapart));
    const size_t out_bytes = L.out_bytes;
    if (single) CKC(hipMemcpyAsync(hs, b->d_ba_io, out_bytes, hipMemcpyDeviceToHost, s));   // (multi: the finish kernel wrote into hs)
    if ((rc = wait_done_word(ctx, s, done_word, b->done_seq, flag_wait))) return rc;
    const double* h_out = (const double*)hs;
    if (!single && check) {   // diagnostic: the same problem through the one-workgroup kernel, differences to stderr
        std::vector<double> got(h_out, h_out + out_bytes / 8);
        CKC(hipMemcpyAsync(b->d_ba_io, saved.data(), io_bytes, hipMemcpyHostToDevice, s));
        A.Wd = b->d_Wd;
        CKC(launch_ba_lm(s, A));
        CKC(hipMemcpyAsync(hs, b->d_ba_io, out_bytes, hipMemcpyDeviceToHost, s));
        CKC(hipStreamSynchronize(s));
        double dmax = 0;
        for (size_t i = BA_SUM_SLOTS; i < out_bytes / 8; i++) dmax = std::max(dmax, fabs(got[i] - h_out[i]));
        fprintf(stderr, "[ba-check] nc=%d np=%d nobs=%d multi: cost %.12g -> %.12g it %d ok %d term %d | single: %.12g -> %.12g it %d ok %d term %d | max|dx| %.3e\n",
                nc, np, n_obs, got[0], got[1], (int)got[2], (int)got[3], (int)got[4], h_out[0], h_out[1], (int)h_out[2], (int)h_out[3],
                (int)h_out[4], dmax);
        {   // sensitivity: the same problem with the cameras perturbed by 1e-9 (how much does one solve amplify?)
            std::vector<double> base(h_out, h_out + out_bytes / 8);
            std::vector<char> pert(saved);
            double* pc = (double*)(pert.data() + L.cams);
            for (int i = 0; i < 6 * nc; i++) pc[i] += 1e-9 * ((i * 2654435761u >> 7) % 3 - 1.0);
            CKC(hipMemcpyAsync(b->d_ba_io, pert.data(), io_bytes, hipMemcpyHostToDevice, s));
            CKC(launch_ba_lm(s, A));
            CKC(hipMemcpyAsync(hs, b->d_ba_io, out_bytes, hipMemcpyDeviceToHost, s));
            CKC(hipStreamSynchronize(s));
            double d2 = 0;
            for (size_t i = BA_SUM_SLOTS; i < out_bytes / 8; i++) d2 = std::max(d2, fabs(base[i] - h_out[i]));
            fprintf(stderr, "[ba-check]    input perturbed by 1e-9 -> single-kernel output moves by %.3e\n", d2);
        }
        memcpy(hs, got.data(), out_bytes);
    }
    ba_finish(ctx, b, cams, nc, pts, np, obs_xy, cam_idx, pt_idx, n_obs, K, huber_delta, max_iterations, L, summary);
    return PMV_OK;
}

}  // extern "C"

// ---- five-point RANSAC round: prepare / finish ----------------------------------------------------------------------------------
int pmv::fivepoint_check(pmv_ctx* ctx, const double* models, const int* n_models, const int* counts) {
    REQ(models && n_models && counts, PMV_ERR_INVALID, "pmv_fivepoint_hypotheses: null argument");
    return PMV_OK;
}
int pmv::fivepoint_prepare(pmv_ctx* ctx, BackendBuffers* b, const double* q1, const double* q2, int n, const int* samples, int n_hyp, float thr,
                           FivePointProblem* P, FivePointLayout* Lout) {
    REQ(q1 && q2 && samples && n >= 5 && n <= ctx->max_tracks && n_hyp >= 1 && n_hyp <= FP_MAX_HYP, PMV_ERR_INVALID,
        "five-point round: n=%d (5..max_tracks=%d), n_hyp=%d (1..%d)", n, ctx->max_tracks, n_hyp, FP_MAX_HYP);
    const FivePointLayout L = fivepoint_layout((size_t)n, (size_t)n_hyp);
    REQ(L.in_bytes <= b->d_tri_in.cap && L.total <= b->h_stage.cap, PMV_ERR_CAPACITY, "five-point round: input block too small");
    char* hs = (char*)b->h_stage;
    memcpy(hs + L.q1, q1, (size_t)n * 16); memcpy(hs + L.q2, q2, (size_t)n * 16); memcpy(hs + L.samples, samples, (size_t)5 * n_hyp * 4);
    P->q1 = (const double*)(b->d_tri_in + L.q1);
    P->q2 = (const double*)(b->d_tri_in + L.q2);
    P->samples = (const int*)(b->d_tri_in + L.samples);
    P->models_d = (double*)b->d_fp_work;
    P->n_models_d = (int*)(b->d_fp_work + (size_t)FP_MAX_HYP * 90 * 8);
    char* dh = b->h_stage.dm();
    P->models_h = (double*)(dh + L.models);
    P->n_models_h = (int*)(dh + L.n_models);
    P->counts_h = (int*)(dh + L.counts);
    P->n = n; P->n_hyp = n_hyp; P->thr = thr;
    // hypotheses whose sample is degenerate write no models: clear the counts the host will read
    memset(hs + L.n_models, 0, L.total - L.n_models);
    *Lout = L;
    return PMV_OK;
}
void pmv::fivepoint_finish(BackendBuffers* b, int n_hyp, const FivePointLayout& L, double* models, int* n_models, int* counts) {
    const char* hs = (const char*)b->h_stage;
    memcpy(models, hs + L.models, (size_t)n_hyp * 90 * 8);
    memcpy(n_models, hs + L.n_models, (size_t)n_hyp * 4);
    memcpy(counts, hs + L.counts, (size_t)n_hyp * 40);
}

// ---- two-view DLT: prepare / finish -------------------------------------------------------------------------------------------
int pmv::dlt_check(pmv_ctx* ctx, const char* who, const double* q1, const double* q2, int n, const double* P1x4, const uint8_t* mask_in, const double* out_Q,
                   const uint8_t* out_mask, const int* out_good) {
    REQ(q1 && q2 && P1x4 && mask_in && out_Q && out_mask && out_good, PMV_ERR_INVALID, "%s: null argument", who);
    REQ(n >= 1 && n <= ctx->max_tracks, PMV_ERR_CAPACITY, "%s: n=%d (1..max_tracks=%d)", who, n, ctx->max_tracks);
    return PMV_OK;
}
int pmv::dlt_prepare(pmv_ctx* ctx, BackendBuffers* b, const double* q1, const double* q2, int n, const double* P1x4, const uint8_t* mask_in, DltProblem* P,
                     DltLayout* Lout) {
    const DltLayout L = dlt_layout((size_t)n);
    REQ(L.in_bytes <= b->d_tri_in.cap && L.total <= b->h_stage.cap, PMV_ERR_CAPACITY, "pmv_triangulate_candidates: n=%d does not fit the staging blocks", n);
    char* hs = (char*)b->h_stage;
    memcpy(hs + L.P, P1x4, 48 * 8); memcpy(hs + L.q1, q1, (size_t)n * 16); memcpy(hs + L.q2, q2, (size_t)n * 16); memcpy(hs + L.mask_in, mask_in, (size_t)n);
    P->P1x4 = (const double*)(b->d_tri_in + L.P);
    P->q1 = (const double*)(b->d_tri_in + L.q1);
    P->q2 = (const double*)(b->d_tri_in + L.q2);
    P->mask_in = (const uint8_t*)(b->d_tri_in + L.mask_in);
    P->Q = (double*)(b->h_stage.dm() + L.Q);   // results go straight into the pinned block (coalesced 8-byte stores)
    P->mask = (uint8_t*)(b->h_stage.dm() + L.mask);
    P->n = n;
    *Lout = L;
    return PMV_OK;
}
void pmv::dlt_finish(pmv_ctx* ctx, BackendBuffers* b, const double* q1, const double* q2, int n, const double* P1x4, const uint8_t* mask_in,
                     const DltLayout& L, double* out_Q, uint8_t* out_mask, int* out_good) {
    const char* hs = (const char*)b->h_stage;
    memcpy(out_Q, hs + L.Q, (size_t)16 * n * 8);
    memcpy(out_mask, hs + L.mask, (size_t)4 * n);
    for (int c = 0; c < 4; c++) {
        int g = 0;
        for (int i = 0; i < n; i++) g += out_mask[(size_t)c * n + i];
        out_good[c] = g;
    }
    if (ctx->log.on) {   // [kind 2, n | q1 2n, q2 2n, P 48 f64 | mask_in n u8 | Q 16n f64 | mask 4n u8 | good 4 i32]
        std::lock_guard<std::mutex> lk(ctx->log.mu);
        ctx->log.blobs.emplace_back();
        std::vector<char>& bl = ctx->log.blobs.back();
        const int hdr[2] = {2, n};
        pmv_call_log::put(bl, hdr, 8); pmv_call_log::put(bl, q1, (size_t)n * 16); pmv_call_log::put(bl, q2, (size_t)n * 16); pmv_call_log::put(bl, P1x4, 384);
        pmv_call_log::put(bl, mask_in, (size_t)n); pmv_call_log::put(bl, out_Q, (size_t)n * 128); pmv_call_log::put(bl, out_mask, (size_t)n * 4);
        pmv_call_log::put(bl, out_good, 16);
    }
}

extern "C" {

// one round of cv::findEssentialMat's RANSAC (OpenCVFivePointTri.cpp:24) on the device: see include/pmv_hip.h
int pmv_fivepoint_hypotheses(pmv_ctx* ctx, const double* q1, const double* q2, int n, const int* samples, int n_hyp, float thr, double* models,
                             int* n_models, int* counts) {
    REQ(ctx, PMV_ERR_INVALID, "pmv_fivepoint_hypotheses: null argument");
    if (const int rc = fivepoint_check(ctx, models, n_models, counts)) return rc;
    tl_prof = &ctx->prof;
    CKC(hipSetDevice(ctx->device));
    BackendBuffers* b = ctx->be;
    hipStream_t s = ctx->s_back;
    FivePointProblem P;
    FivePointLayout L;
    int rc = fivepoint_prepare(ctx, b, q1, q2, n, samples, n_hyp, thr, &P, &L);
    if (rc) return rc;
    CKC(hipMemcpyAsync(b->d_tri_in, b->h_stage, L.in_bytes, hipMemcpyHostToDevice, s));
    CKC(hipMemcpyAsync(b->d_tri_out, &P, sizeof(P), hipMemcpyHostToDevice, s));   // the problem record (d_tri_out is free during a five-point round)
    CKC(launch_fivepoint_batch(s, (const FivePointProblem*)b->d_tri_out, 1, n_hyp));
    CKC(hipStreamSynchronize(s));
    fivepoint_finish(b, n_hyp, L, models, n_models, counts);
    return PMV_OK;
}

// the per-point part of cv::recoverPose (OpenCVFivePointTri.cpp:27): DLT triangulation + cheirality for the four candidates
static int triangulate_on(pmv_ctx* ctx, BackendBuffers* b, hipStream_t s, const double* q1, const double* q2, int n, const double* P1x4,
                          const uint8_t* mask_in, double* out_Q, uint8_t* out_mask, int* out_good) {
    DltProblem P;
    DltLayout L;
    if (const int rc = dlt_prepare(ctx, b, q1, q2, n, P1x4, mask_in, &P, &L)) return rc;
    CKC(hipMemcpyAsync(b->d_tri_in, b->h_stage, L.in_bytes, hipMemcpyHostToDevice, s));
    CKC(launch_tri_dlt(s, P.P1x4, P.q1, P.q2, P.mask_in, n, P.Q, P.mask));
    CKC(hipStreamSynchronize(s));
    dlt_finish(ctx, b, q1, q2, n, P1x4, mask_in, L, out_Q, out_mask, out_good);
    return PMV_OK;
}

int pmv_triangulate_candidates(pmv_ctx* ctx, const double* q1, const double* q2, int n, const double* P1x4, const uint8_t* mask_in,
                               double* out_Q, uint8_t* out_mask, int* out_good) {
    REQ(ctx, PMV_ERR_INVALID, "pmv_triangulate_candidates: null argument");
    if (const int rc = dlt_check(ctx, "pmv_triangulate_candidates", q1, q2, n, P1x4, mask_in, out_Q, out_mask, out_good)) return rc;
    tl_prof = &ctx->prof;
    CKC(hipSetDevice(ctx->device));
    return triangulate_on(ctx, ctx->be, ctx->s_back, q1, q2, n, P1x4, mask_in, out_Q, out_mask, out_good);
}

int pmv_triangulate_candidates_ahead(pmv_ctx* ctx, const double* q1, const double* q2, int n, const double* P1x4, const uint8_t* mask_in,
                                     double* out_Q, uint8_t* out_mask, int* out_good) {
    REQ(ctx, PMV_ERR_INVALID, "pmv_triangulate_candidates_ahead: null argument");
    if (const int rc = dlt_check(ctx, "pmv_triangulate_candidates_ahead", q1, q2, n, P1x4, mask_in, out_Q, out_mask, out_good)) return rc;
    std::lock_guard<std::mutex> lk(ctx->ahead_mu);   // one call at a time on the auxiliary lane (its callers are helper threads)
    CKC(hipSetDevice(ctx->device));
    if (!ctx->be_ahead) {
        BackendBuffers* b = nullptr;
        const int rc = backend_alloc(ctx, &b);
        if (rc != PMV_OK) { if (b) backend_free(b); return rc; }
        ctx->be_ahead = b;
        CKC(hipStreamCreateWithFlags(&ctx->s_ahead, hipStreamNonBlocking));
    }
    return triangulate_on(ctx, ctx->be_ahead, ctx->s_ahead, q1, q2, n, P1x4, mask_in, out_Q, out_mask, out_good);
}

}  // extern "C"

// ---- the two whole-RANSAC calls (pmv_ransac.h): what their prepare halves and their single calls share --------------------------------------
// The tail of either *_prepare, once the points and the iteration table stand in b's pinned block by L: the record points into the device
// in-block d_in and at the mapped result block, takes the set's next sequence number, whose word it clears, and goes into the in-block
template <class Pt> static void whole_record(BackendBuffers* b, char* d_in, const WholeLayout& L, int n, double threshold, int max_iters, WholeProblem<Pt>* P) {
    if (++b->done_seq == 0) b->done_seq = 1;
    *P = whole_problem((const Pt*)(d_in + L.p1), (const Pt*)(d_in + L.p2), (const double*)(d_in + L.iters), b->h_stage.dm() + L.out, n, threshold, max_iters, b->done_seq);
    *whole_done_word(b, L) = 0;
    *(WholeProblem<Pt>*)((char*)b->h_stage + L.rec) = *P;
}
// A checked single call on the context's own set: prepare (either *_prepare, bound to the call's arguments), stage-in into the set's d_in,
// one workgroup of `launch`, the wait for the request's completion word, the copy-out
template <class Pt, class Prepare>
static int whole_single(pmv_ctx* ctx, Prepare prepare, Buf<char> BackendBuffers::*d_in, hipError_t (*launch)(hipStream_t, const WholeProblem<Pt>*, int), int n,
                        double* M9, uint8_t* mask, int* out_found, int* out_samples_drawn) {
    tl_prof = &ctx->prof;
    CKC(hipSetDevice(ctx->device));
    BackendBuffers* b = ctx->be;
    hipStream_t s = ctx->s_back;
    WholeProblem<Pt> P;
    WholeLayout L;
    if (const int rc = prepare(b, &P, &L)) return rc;
    char* d = b->*d_in;
    CKC(stage_block(s, b->h_stage.dm(), d, L.in_bytes, 8));
    CKC(launch(s, (const WholeProblem<Pt>*)d, 1));
    if (const int rc = wait_done_word(ctx, s, whole_done_word(b, L), P.done_seq, back_wait_by_word())) return rc;
    whole_finish(b, n, L, M9, mask, out_found, out_samples_drawn);
    return PMV_OK;
}

// ---- whole findEssentialMat RANSAC on the device (k_essential_ransac): check / prepare / finish -----------------------------------------
int pmv::essential_check(pmv_ctx* ctx, const char* who, const double* p1_xy, const double* p2_xy, int n, const double* K, double prob, double threshold,
                         double* E9, uint8_t* mask, int* out_found, int* out_samples_drawn) {
    REQ(ctx && p1_xy && p2_xy && K && E9 && mask && out_found && out_samples_drawn, PMV_ERR_INVALID, "%s: null argument", who);
    REQ(prob >= 0 && prob <= 1, PMV_ERR_INVALID, "%s: prob = %g outside [0, 1]", who, prob);
    REQ(threshold > 0 && std::isfinite(threshold), PMV_ERR_INVALID, "%s: threshold = %g (a positive finite number of pixels)", who, threshold);
    REQ(n >= 0 && n <= ctx->max_tracks, PMV_ERR_CAPACITY, "%s: n=%d (0..max_tracks=%d)", who, n, ctx->max_tracks);
    return PMV_OK;
}
// essential_layout: pinned in-block [EssentialProblem | q1 2n | q2 2n | log(1 - prob), n + 1 denominators], out-block [WholeResultHdr | mask]
int pmv::essential_prepare(pmv_ctx* ctx, BackendBuffers* b, const double* p1, const double* p2, int n, const double* K, double prob, double threshold,
                           EssentialProblem* P, WholeLayout* Lout) {
    const WholeLayout L = essential_layout((size_t)n);
    REQ(L.in_bytes <= b->d_ess_in.cap && L.total <= b->h_stage.cap, PMV_ERR_CAPACITY, "pmv_find_essential_mat: n=%d does not fit the staging blocks", n);
    char* hs = (char*)b->h_stage;
    double* h_q1 = (double*)(hs + L.p1);
    double* h_q2 = (double*)(hs + L.p2);
    double* h_it = (double*)(hs + L.iters);
    // the normalisation of vo_fivepoint.cpp:find_essential_mat, expression for expression
    const double fx = K[0], fy = K[4], cx = K[2], cy = K[5];
    for (int i = 0; i < n; i++) {
        h_q1[2 * i] = (p1[2 * i] - cx) / fx; h_q1[2 * i + 1] = (p1[2 * i + 1] - cy) / fy;
        h_q2[2 * i] = (p2[2 * i] - cx) / fx; h_q2[2 * i + 1] = (p2[2 * i + 1] - cy) / fy;
    }
    threshold /= (fx + fy) / 2;
    vo::five_point_iters_table(n, prob, h_it + 1, h_it);
    whole_record(b, b->d_ess_in, L, n, threshold, WHOLE_MAX_ITERS, P);
    *Lout = L;
    return PMV_OK;
}
volatile unsigned* pmv::whole_done_word(BackendBuffers* b, const WholeLayout& L) { return (volatile unsigned*)((char*)b->h_stage + L.done); }
void pmv::whole_finish(BackendBuffers* b, int n, const WholeLayout& L, double* M9, uint8_t* mask, int* out_found, int* out_samples_drawn) {
    const WholeResultHdr* R = (const WholeResultHdr*)((const char*)b->h_stage + L.out);
    *out_found = R->found; *out_samples_drawn = R->samples_drawn;
    if (R->found) memcpy(M9, R->M, 72);
    memcpy(mask, (const char*)b->h_stage + L.mask, (size_t)n);
}
int pmv::recover_pose_check(pmv_ctx* ctx, const char* who, const double* E9, const double* p1_xy, const double* p2_xy, int n, const double* K, double* R9,
                            double* t3, uint8_t* mask, double* tri4n, int* out_good) {
    REQ(ctx && E9 && p1_xy && p2_xy && K && R9 && t3 && mask && tri4n && out_good, PMV_ERR_INVALID, "%s: null argument", who);
    REQ(n >= 0 && n <= ctx->max_tracks, PMV_ERR_CAPACITY, "%s: n=%d (0..max_tracks=%d)", who, n, ctx->max_tracks);
    return PMV_OK;
}

// ---- whole findFundamentalMat RANSAC on the device (k_fundamental_ransac): check / prepare / finish -------------------------------------
int pmv::fundamental_check(pmv_ctx* ctx, const char* who, const float* p1_xy, const float* p2_xy, int n, double threshold, double confidence, double* F9,
                           uint8_t* mask, int* out_found, int* out_samples_drawn) {
    REQ(ctx && p1_xy && p2_xy && F9 && mask && out_found && out_samples_drawn, PMV_ERR_INVALID, "%s: null argument", who);
    REQ(threshold > 0 && std::isfinite(threshold), PMV_ERR_INVALID, "%s: threshold = %g (a positive finite number of pixels)", who, threshold);
    REQ(confidence > 0 && confidence < 1, PMV_ERR_INVALID, "%s: confidence = %g outside (0, 1)", who, confidence);   // (a NaN fails the comparison too)
    REQ(n >= 0 && n <= ctx->max_tracks, PMV_ERR_CAPACITY, "%s: n=%d (0..max_tracks=%d)", who, n, ctx->max_tracks);
    // cv::findFundamentalMat runs RANSAC only from 15 points on: LMedS for 8..14, up to three stacked matrices for 7 - neither is built
    REQ(n >= 15, PMV_ERR_DEGENERATE, "%s: %d correspondences (the RANSAC needs >= 15; cv switches to LMedS or the plain 7-point result below, which are not built)", who, n);
    for (int k = 0; k < 2; k++) {
        const float* p = k ? p2_xy : p1_xy;
        for (int i = 0; i < 2 * n; i++)
            REQ(fabsf(p[i]) <= 1e6f, PMV_ERR_INVALID, "%s: point %d of image %d (%g, %g) is not finite or beyond 1e6", who, i / 2, k + 1, (double)p[i & ~1], (double)p[i | 1]);
    }
    return PMV_OK;
}
// fundamental_layout: pinned in-block [FundamentalProblem | p1 2n floats | p2 2n floats | log(1 - confidence), n + 1 denominators], out-block
// as essential_prepare's with F in the place of E
// (for the model points and the iteration cap of either call on float points)
static int float_points_prepare(pmv_ctx* ctx, BackendBuffers* b, const char* who, const float* p1, const float* p2, int n, double threshold, double confidence,
                                int model_points, int max_iters, WholeProblem<float>* P, WholeLayout* Lout) {
    const size_t fund_in_bytes = fund_in_cap((size_t)ctx->max_tracks);
    if (b->d_fund_in.cap < fund_in_bytes) {   // the set's first such call: a session caller's thread has not chosen the context's device yet
        CKC(hipSetDevice(ctx->device));
        CKC(b->d_fund_in.ensure(fund_in_bytes));
    }
    const WholeLayout L = fundamental_layout((size_t)n);
    REQ(L.in_bytes <= b->d_fund_in.cap && L.total <= b->h_stage.cap, PMV_ERR_CAPACITY, "%s: n=%d does not fit the staging blocks", who, n);
    char* hs = (char*)b->h_stage;
    double* h_it = (double*)(hs + L.iters);
    memcpy(hs + L.p1, p1, (size_t)n * 8);
    memcpy(hs + L.p2, p2, (size_t)n * 8);
    vo::ransac_iters_table(n, confidence, model_points, h_it + 1, h_it);
    whole_record(b, b->d_fund_in, L, n, threshold, max_iters, P);
    *Lout = L;
    return PMV_OK;
}
int pmv::fundamental_prepare(pmv_ctx* ctx, BackendBuffers* b, const float* p1, const float* p2, int n, double threshold, double confidence,
                             FundamentalProblem* P, WholeLayout* Lout) {
    return float_points_prepare(ctx, b, "pmv_find_fundamental_mat", p1, p2, n, threshold, confidence, 7, WHOLE_MAX_ITERS, P, Lout);
}

// ---- whole findHomography RANSAC and refit on the device (k_homography_ransac): check / prepare; the blocks and whole_finish are F's ---------
int pmv::homography_args_check(int max_tracks, const char* who, const float* p1_xy, const float* p2_xy, int n, double threshold, double confidence, int max_iters,
                               const double* H9, const uint8_t* mask, const int* out_found, const int* out_samples_drawn, char* err) {
#define HREQ(cond, code, ...) do { if (!(cond)) { snprintf(err, 256, __VA_ARGS__); return code; } } while (0)
    HREQ(p1_xy && p2_xy && H9 && mask && out_found && out_samples_drawn, PMV_ERR_INVALID, "%s: null argument", who);
    HREQ(threshold > 0 && std::isfinite(threshold), PMV_ERR_INVALID, "%s: threshold = %g (a positive finite number of pixels)", who, threshold);
    HREQ(confidence > 0 && confidence < 1, PMV_ERR_INVALID, "%s: confidence = %g outside (0, 1)", who, confidence);   // (a NaN fails the comparison too)
    HREQ(max_iters >= 1 && max_iters <= HG_MAX_ITERS, PMV_ERR_INVALID, "%s: max_iters = %d outside 1..%d", who, max_iters, HG_MAX_ITERS);
    HREQ(n >= 0 && n <= max_tracks, PMV_ERR_CAPACITY, "%s: n=%d (0..max_tracks=%d)", who, n, max_tracks);
    HREQ(n >= 4, PMV_ERR_DEGENERATE, "%s: %d correspondences (a homography needs >= 4; cv asserts)", who, n);
    for (int k = 0; k < 2; k++) {
        const float* p = k ? p2_xy : p1_xy;
        for (int i = 0; i < 2 * n; i++)
            HREQ(fabsf(p[i]) <= 1e6f, PMV_ERR_INVALID, "%s: point %d of image %d (%g, %g) is not finite or beyond 1e6", who, i / 2, k + 1, (double)p[i & ~1], (double)p[i | 1]);
    }
#undef HREQ
    return PMV_OK;
}
int pmv::homography_check(pmv_ctx* ctx, const char* who, const float* p1_xy, const float* p2_xy, int n, double threshold, double confidence, int max_iters,
                          double* H9, uint8_t* mask, int* out_found, int* out_samples_drawn) {
    REQ(ctx, PMV_ERR_INVALID, "%s: null argument", who);
    char err[256];
    const int rc = homography_args_check(ctx->max_tracks, who, p1_xy, p2_xy, n, threshold, confidence, max_iters, H9, mask, out_found, out_samples_drawn, err);
    if (rc != PMV_OK) set_err(ctx, "%s", err);
    return rc;
}
int pmv::homography_prepare(pmv_ctx* ctx, BackendBuffers* b, const float* p1, const float* p2, int n, double threshold, double confidence, int max_iters,
                            HomographyProblem* P, WholeLayout* Lout) {
    return float_points_prepare(ctx, b, "pmv_find_homography", p1, p2, n, threshold, confidence, 4, max_iters, P, Lout);
}

// ---- N-view triangulation of track landmarks (k_tri_tracks, backend_tritracks.hip): check / prepare / finish ------------------------------
pmv_tri_params pmv::tri_tracks_defaults() { return pmv_tri_params{2, 0, 0.1, HUGE_VAL, HUGE_VAL, 0.0}; }
// the centre C = -M^-1 p4 of one camera by the adjugate (the statement of tests/twin/tri_tracks_twin.cpp); false: det M == 0, C3 untouched
static bool tri_centre(const double* p, double* C3) {
    const double m00 = p[0], m01 = p[1], m02 = p[2], m10 = p[4], m11 = p[5], m12 = p[6], m20 = p[8], m21 = p[9], m22 = p[10];
    const double a00 = m11 * m22 - m12 * m21, a01 = m02 * m21 - m01 * m22, a02 = m01 * m12 - m02 * m11;
    const double a10 = m12 * m20 - m10 * m22, a11 = m00 * m22 - m02 * m20, a12 = m02 * m10 - m00 * m12;
    const double a20 = m10 * m21 - m11 * m20, a21 = m01 * m20 - m00 * m21, a22 = m00 * m11 - m01 * m10;
    const double det = m00 * a00 + m01 * a10 + m02 * a20;
    if (det == 0) return false;
    C3[0] = -(a00 * p[3] + a01 * p[7] + a02 * p[11]) / det;
    C3[1] = -(a10 * p[3] + a11 * p[7] + a12 * p[11]) / det;
    C3[2] = -(a20 * p[3] + a21 * p[7] + a22 * p[11]) / det;
    return true;
}
int pmv::tri_tracks_args_check(int max_cams, int max_points, int max_obs, const char* who, const double* P3x4, int nc, const double* obs_xy, const int* cam_idx,
                               const int* pt_idx, int n_obs, int np, const pmv_tri_params* p_or_null, const double* out_xyz, const uint8_t* out_status,
                               const int* out_good, char* err) {
#define TREQ(cond, code, ...) do { if (!(cond)) { snprintf(err, 256, __VA_ARGS__); return code; } } while (0)
    TREQ(P3x4 && out_good && (n_obs <= 0 || (obs_xy && cam_idx && pt_idx)) && (np <= 0 || (out_xyz && out_status)), PMV_ERR_INVALID, "%s: null argument", who);
    const pmv_tri_params p = p_or_null ? *p_or_null : tri_tracks_defaults();
    TREQ(p.min_views >= 2, PMV_ERR_INVALID, "%s: min_views = %d (at least 2)", who, p.min_views);
    TREQ(p.refine_iters >= 0 && p.refine_iters <= TT_MAX_REFINE, PMV_ERR_INVALID, "%s: refine_iters = %d outside 0..%d", who, p.refine_iters, TT_MAX_REFINE);
    TREQ(std::isfinite(p.min_depth), PMV_ERR_INVALID, "%s: min_depth = %g is not finite", who, p.min_depth);
    TREQ(p.max_depth >= p.min_depth, PMV_ERR_INVALID, "%s: max_depth = %g below min_depth = %g", who, p.max_depth, p.min_depth);   // (a NaN fails the comparison too)
    TREQ(p.max_reproj > 0, PMV_ERR_INVALID, "%s: max_reproj = %g (positive, +inf = no gate)", who, p.max_reproj);
    TREQ(p.min_parallax_deg >= 0 && p.min_parallax_deg < 180, PMV_ERR_INVALID, "%s: min_parallax_deg = %g outside [0, 180)", who, p.min_parallax_deg);
    TREQ(nc >= 1, PMV_ERR_INVALID, "%s: nc = %d (at least one camera)", who, nc);
    TREQ(nc <= max_cams && np >= 0 && np <= max_points && n_obs >= 0 && n_obs <= max_obs, PMV_ERR_CAPACITY, "%s: nc=%d np=%d n_obs=%d exceed capacity %d/%d/%d", who,
         nc, np, n_obs, max_cams, max_points, max_obs);
    for (int i = 0; i < n_obs; i++)
        TREQ(cam_idx[i] >= 0 && cam_idx[i] < nc && pt_idx[i] >= 0 && pt_idx[i] < np, PMV_ERR_INVALID, "%s: index out of range at observation %d (camera %d of %d, landmark %d of %d)",
             who, i, cam_idx[i], nc, pt_idx[i], np);
    for (int i = 0; i < 12 * nc; i++) TREQ(std::isfinite(P3x4[i]), PMV_ERR_INVALID, "%s: entry %d of the projection matrix of camera %d is not finite", who, i % 12, i / 12);
    for (int i = 0; i < 2 * n_obs; i++) TREQ(std::isfinite(obs_xy[i]), PMV_ERR_INVALID, "%s: observation %d (%g, %g) is not finite", who, i / 2, obs_xy[i & ~1], obs_xy[i | 1]);
    if (p.min_parallax_deg > 0)
        for (int c = 0; c < nc; c++) {
            double C3[3];
            TREQ(tri_centre(P3x4 + 12 * c, C3), PMV_ERR_INVALID, "%s: camera %d has a singular left 3x3 block (det M == 0): no centre for the parallax gate", who, c);
        }
#undef TREQ
    return PMV_OK;
}
int pmv::tri_tracks_check(pmv_ctx* ctx, const char* who, const double* P3x4, int nc, const double* obs_xy, const int* cam_idx, const int* pt_idx, int n_obs, int np,
                          const pmv_tri_params* p_or_null, double* out_xyz, uint8_t* out_status, int* out_good) {
    REQ(ctx, PMV_ERR_INVALID, "%s: null argument", who);
    char err[256];
    const int rc = tri_tracks_args_check(ctx->max_ba_cams, ctx->max_ba_points, ctx->max_ba_obs, who, P3x4, nc, obs_xy, cam_idx, pt_idx, n_obs, np, p_or_null, out_xyz,
                                         out_status, out_good, err);
    if (rc != PMV_OK) set_err(ctx, "%s", err);
    return rc;
}
void pmv::tri_tracks_empty(int np, double* out_xyz, uint8_t* out_status, double* out_err_or_null, int* out_good) {
    for (int p = 0; p < np; p++) {
        out_xyz[3 * p] = out_xyz[3 * p + 1] = out_xyz[3 * p + 2] = 0; out_status[p] = PMV_TRI_FEW_VIEWS;
        if (out_err_or_null) out_err_or_null[p] = HUGE_VAL;
    }
    *out_good = 0;
}
// tri_tracks_layout: the record, P, the centres (zeros with the gate off), the observations in per-landmark runs, the run starts, the counter
int pmv::tri_tracks_prepare(pmv_ctx* ctx, BackendBuffers* b, const double* P3x4, int nc, const double* obs_xy, const int* cam_idx, const int* pt_idx, int n_obs,
                            int np, const pmv_tri_params* p_or_null, TriTracksProblem* P, TriTracksLayout* Lout) {
    const pmv_tri_params p = p_or_null ? *p_or_null : tri_tracks_defaults();
    const TriTracksLayout L = tri_tracks_layout((size_t)nc, (size_t)np, (size_t)n_obs);
    REQ(L.in_bytes <= b->d_tt_in.cap && L.total <= b->h_stage.cap, PMV_ERR_CAPACITY, "pmv_triangulate_tracks: nc=%d np=%d n_obs=%d do not fit the staging blocks", nc, np, n_obs);
    char* hs = (char*)b->h_stage;
    double* h_C = (double*)(hs + L.C); double* h_obs = (double*)(hs + L.obs);
    int* h_cam = (int*)(hs + L.cam); int* start = (int*)(hs + L.start);
    memcpy(hs + L.P, P3x4, (size_t)nc * 96);
    const bool parallax_on = p.min_parallax_deg > 0;
    for (int c = 0; c < nc; c++) {
        h_C[3 * c] = h_C[3 * c + 1] = h_C[3 * c + 2] = 0;
        if (parallax_on) REQ(tri_centre(P3x4 + 12 * c, h_C + 3 * c), PMV_ERR_INVALID, "pmv_triangulate_tracks: camera %d has a singular left 3x3 block", c);
    }
    // the observations of a landmark, in order of appearance (stable counting sort)
    std::fill(start, start + np + 1, 0);
    for (int i = 0; i < n_obs; i++) start[pt_idx[i] + 1]++;
    for (int q = 0; q < np; q++) start[q + 1] += start[q];
    {
        std::vector<int> fill(start, start + np);
        for (int i = 0; i < n_obs; i++) {
            const int o = fill[pt_idx[i]]++;
            h_obs[2 * o] = obs_xy[2 * i]; h_obs[2 * o + 1] = obs_xy[2 * i + 1]; h_cam[o] = cam_idx[i];
        }
    }
    memset(hs + L.counter, 0, 16);
    char* d = b->d_tt_in;
    if (++b->done_seq == 0) b->done_seq = 1;
    P->P = (const double*)(d + L.P); P->C = (const double*)(d + L.C); P->obs = (const double*)(d + L.obs); P->cam = (const int*)(d + L.cam);
    P->start = (const int*)(d + L.start); P->counter = (unsigned*)(d + L.counter);
    P->out = b->h_stage.dm() + L.out;
    P->min_depth = p.min_depth; P->max_depth = p.max_depth; P->max_reproj = p.max_reproj;
    P->cos_thr = parallax_on ? std::cos(p.min_parallax_deg * M_PI / 180.0) : 1.0;
    P->nc = nc; P->np = np; P->min_views = p.min_views; P->refine_iters = p.refine_iters; P->parallax_on = parallax_on ? 1 : 0;
    P->done_seq = b->done_seq;
    *(volatile unsigned*)(hs + L.done) = 0;
    memset(hs + L.rec, 0, TT_HDR);
    *(TriTracksProblem*)(hs + L.rec) = *P;
    *Lout = L;
    return PMV_OK;
}
void pmv::tri_tracks_finish(BackendBuffers* b, int np, const TriTracksLayout& L, double* out_xyz, uint8_t* out_status, double* out_err_or_null, int* out_good) {
    const char* hs = (const char*)b->h_stage;
    memcpy(out_xyz, hs + L.xyz, (size_t)np * 24);
    memcpy(out_status, hs + L.status, (size_t)np);
    if (out_err_or_null) memcpy(out_err_or_null, hs + L.err, (size_t)np * 8);
    int good = 0;
    for (int q = 0; q < np; q++) good += out_status[q] == 0;
    *out_good = good;
}

extern "C" {

int pmv_triangulate_tracks(pmv_ctx* ctx, const double* P3x4, int nc, const double* obs_xy, const int* cam_idx, const int* pt_idx, int n_obs, int np,
                           const pmv_tri_params* p_or_null, double* out_xyz, uint8_t* out_status, double* out_err_or_null, int* out_good) {
    if (const int rc = tri_tracks_check(ctx, "pmv_triangulate_tracks", P3x4, nc, obs_xy, cam_idx, pt_idx, n_obs, np, p_or_null, out_xyz, out_status, out_good)) return rc;
    if (np == 0 || n_obs == 0) { tri_tracks_empty(np, out_xyz, out_status, out_err_or_null, out_good); return PMV_OK; }
    tl_prof = &ctx->prof;
    CKC(hipSetDevice(ctx->device));
    BackendBuffers* b = ctx->be;
    hipStream_t s = ctx->s_back;
    TriTracksProblem P;
    TriTracksLayout L;
    if (const int rc = tri_tracks_prepare(ctx, b, P3x4, nc, obs_xy, cam_idx, pt_idx, n_obs, np, p_or_null, &P, &L)) return rc;
    CKC(stage_block(s, b->h_stage.dm(), b->d_tt_in, L.in_bytes, 8));
    CKC(launch_tri_tracks(s, (const TriTracksProblem*)(b->d_tt_in + L.rec), np));
    ctx->tri_tracks_launches[0]++; ctx->tri_tracks_launches[1]++;
    if (const int rc = wait_done_word(ctx, s, (volatile unsigned*)((char*)b->h_stage + L.done), P.done_seq, back_wait_by_word())) return rc;
    tri_tracks_finish(b, np, L, out_xyz, out_status, out_err_or_null, out_good);
    return PMV_OK;
}

int pmv_debug_tri_tracks_check(int max_cams, int max_points, int max_obs, const double* P3x4, int nc, const double* obs_xy, const int* cam_idx, const int* pt_idx,
                               int n_obs, int np, const pmv_tri_params* p_or_null, const double* out_xyz, const uint8_t* out_status, const double* out_err_or_null,
                               const int* out_good, char* err256) {
    (void)out_err_or_null;
    char err[256] = "";
    const int rc = tri_tracks_args_check(max_cams, max_points, max_obs, "pmv_triangulate_tracks", P3x4, nc, obs_xy, cam_idx, pt_idx, n_obs, np, p_or_null, out_xyz,
                                         out_status, out_good, err);
    if (err256) memcpy(err256, err, 256);
    return rc;
}

int pmv_debug_tri_tracks_launches(pmv_ctx* ctx, long long* out2) {
    if (!ctx || !out2) return PMV_ERR_INVALID;
    for (int i = 0; i < 2; i++) out2[i] = ctx->tri_tracks_launches[i].load();
    return PMV_OK;
}

int pmv_find_essential_mat(pmv_ctx* ctx, const double* p1_xy, const double* p2_xy, int n, const double* K, double prob, double threshold, double* E9,
                           uint8_t* mask, int* out_found, int* out_samples_drawn) {
    if (const int rc = essential_check(ctx, "pmv_find_essential_mat", p1_xy, p2_xy, n, K, prob, threshold, E9, mask, out_found, out_samples_drawn)) return rc;
    *out_found = 0; *out_samples_drawn = 0;
    if (n < 5) { memset(mask, 0, (size_t)n); return PMV_OK; }   // fewer points than a sample: no model
    const auto prepare = [&](BackendBuffers* b, EssentialProblem* P, WholeLayout* L) { return essential_prepare(ctx, b, p1_xy, p2_xy, n, K, prob, threshold, P, L); };
    return whole_single(ctx, prepare, &BackendBuffers::d_ess_in, launch_essential_ransac, n, E9, mask, out_found, out_samples_drawn);
}

int pmv_recover_pose(pmv_ctx* ctx, const double* E9, const double* p1_xy, const double* p2_xy, int n, const double* K, double* R9, double* t3, uint8_t* mask,
                     double* tri4n, int* out_good) {
    if (const int rc = recover_pose_check(ctx, "pmv_recover_pose", E9, p1_xy, p2_xy, n, K, R9, t3, mask, tri4n, out_good)) return rc;
    tl_prof = &ctx->prof;
    CKC(hipSetDevice(ctx->device));
    struct Tri : vo::FivePointTri {   // the host half of cv::recoverPose (vo_fivepoint.cpp:recover_pose) around the context's DLT kernel
        pmv_ctx* ctx; int rc = PMV_OK;
        void dlt_candidates(const double* q1, const double* q2, int n, const double* P1x4, const uint8_t* mask_in, double* out_Q, uint8_t* out_mask, int* out_good) override {
            if (n > 0) rc = triangulate_on(ctx, ctx->be, ctx->s_back, q1, q2, n, P1x4, mask_in, out_Q, out_mask, out_good);
        }
    } tri;
    tri.ctx = ctx;
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

int pmv_find_fundamental_mat(pmv_ctx* ctx, const float* p1_xy, const float* p2_xy, int n, double threshold, double confidence, double* F9, uint8_t* mask,
                             int* out_found, int* out_samples_drawn) {
    if (const int rc = fundamental_check(ctx, "pmv_find_fundamental_mat", p1_xy, p2_xy, n, threshold, confidence, F9, mask, out_found, out_samples_drawn)) return rc;
    const auto prepare = [&](BackendBuffers* b, FundamentalProblem* P, WholeLayout* L) { return fundamental_prepare(ctx, b, p1_xy, p2_xy, n, threshold, confidence, P, L); };
    return whole_single(ctx, prepare, &BackendBuffers::d_fund_in, launch_fundamental_ransac, n, F9, mask, out_found, out_samples_drawn);
}

int pmv_find_homography(pmv_ctx* ctx, const float* p1_xy, const float* p2_xy, int n, double threshold, double confidence, int max_iters, double* H9, uint8_t* mask,
                        int* out_found, int* out_samples_drawn) {
    if (const int rc = homography_check(ctx, "pmv_find_homography", p1_xy, p2_xy, n, threshold, confidence, max_iters, H9, mask, out_found, out_samples_drawn)) return rc;
    const auto prepare = [&](BackendBuffers* b, HomographyProblem* P, WholeLayout* L) { return homography_prepare(ctx, b, p1_xy, p2_xy, n, threshold, confidence, max_iters, P, L); };
    const int rc = whole_single(ctx, prepare, &BackendBuffers::d_fund_in, launch_homography_ransac, n, H9, mask, out_found, out_samples_drawn);
    if (rc == PMV_OK) { ctx->homography_launches[0]++; ctx->homography_launches[1]++; }
    return rc;
}

int pmv_debug_homography_iters_table(int n, double confidence, double* out_denoms, double* out_num) {
    if (n < 0 || !out_denoms || !out_num) return PMV_ERR_INVALID;
    vo::ransac_iters_table(n, confidence, 4, out_denoms, out_num);
    return PMV_OK;
}

int pmv_debug_homography_check(int max_tracks, const float* p1_xy, const float* p2_xy, int n, double threshold, double confidence, int max_iters, const double* H9,
                               const uint8_t* mask, const int* out_found, const int* out_samples_drawn, char* out_message256) {
    char err[256] = "";
    const int rc = homography_args_check(max_tracks, "pmv_find_homography", p1_xy, p2_xy, n, threshold, confidence, max_iters, H9, mask, out_found, out_samples_drawn, err);
    if (out_message256) memcpy(out_message256, err, 256);
    return rc;
}

int pmv_debug_homography_launches(pmv_ctx* ctx, long long* out2) {
    if (!ctx || !out2) return PMV_ERR_INVALID;
    for (int i = 0; i < 2; i++) out2[i] = ctx->homography_launches[i].load();
    return PMV_OK;
}

int pmv_debug_fundamental_iters_table(int n, double confidence, double* out_denoms, double* out_num) {
    if (n < 0 || !out_denoms || !out_num) return PMV_ERR_INVALID;
    vo::ransac_iters_table(n, confidence, 7, out_denoms, out_num);
    return PMV_OK;
}

int pmv_debug_fundamental_r(void) { return fundamental_round_width(); }

int pmv_debug_set_fundamental_r(int r) {
    if (r < 0 || r > FUND_MAX_R) return PMV_ERR_INVALID;
    fundamental_set_round_width(r);
    return PMV_OK;
}

int pmv_debug_essential_iters_table(int n, double prob, double* out_denoms, double* out_num) {
    if (n < 0 || !out_denoms || !out_num) return PMV_ERR_INVALID;
    vo::five_point_iters_table(n, prob, out_denoms, out_num);
    return PMV_OK;
}

}  // extern "C"
