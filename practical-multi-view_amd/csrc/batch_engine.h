// Batch engine interface (batch_engine.hip): the request entry points behind the batched pipelines' plugin set (hip_pipeline.hip) and the
// session calls (batch_session.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/pmv_hip.h"
struct pmv_ctx;
namespace pmv {
struct BatchEngine;
int batch_engine_get(pmv_ctx* ctx, int B, BatchEngine** out);   // creates (or grows) the context's engine for B concurrent sequences
void batch_engine_destroy(pmv_ctx* ctx);
// per combiner (LK, detectors, PnP, BA, DLT): counts10 = {launch rounds, requests} x 5; times15 (may be null) = seconds spent
// {CPU time of the combiner thread, wall time processing batches, of that waiting for the GPU} x 5
void batch_engine_stats(BatchEngine* E, long long* counts10, double* times15);
// What a request asks for. Callers name Q_GFTT or Q_SHITOMASI as the `kind` of engine_detect; from Q_WHOLE_FIRST to Q_WHOLE_LAST the engine
// owns the request record.
enum ReqKind {
    Q_LK = 0, Q_GFTT = 1 /* plain or, with the caller's goodFeaturesToTrack arguments, extended */, Q_SHITOMASI = 2, Q_FAST = 3,
    Q_KNN = 4, Q_LK_EX = 5 /* both served by the LK combiners */, Q_SUBPIX = 6, Q_GFTT_FRAME = 7 /* the detector combiner */,
    Q_PNP = 10, Q_BA = 11, Q_DLT = 12, Q_FIVEPOINT = 13, Q_ESSENTIAL = 14, Q_FUNDAMENTAL = 15, Q_HOMOGRAPHY = 16, Q_WHOLE_FIRST = Q_ESSENTIAL,
    Q_WHOLE_LAST = Q_HOMOGRAPHY, Q_TRI_TRACKS = 17 /* served by the DLT combiner */
};
// ---- request entry points: one per plugin call, with the contract of the single call of the same name (include/pmv_hip.h) -------------
// Who checks what. Each entry runs the check function of its single call (pmv_ctx.h, backend.h; bracket = false) and then forms its
// request, so the single call, the session call and the batched pipelines refuse the same arguments with the same status code and text.
// `who` is the name the check's messages carry. A session wrapper (batch_session.hip) adds only what the session owns: that one is open,
// the seq index and the seq's lock. The combiners look at a request's frames once more when they form a round (admit_frames): a slot may
// have been re-used since, and the frame size must be one the batch declared.
// Blocking; safe to call from many threads at once (one outstanding call per seq and stream role). `seq` selects the sequence's back-end
// workspace set. ring_round: the round of the context's batch feeder (ctx->bingest) that builds the request's frames, from slot_ready;
// -1 = none.
// predicted_iters (optional): how many LK iterations the caller expects each track to take (0..255) - the launch starts the expensive
// tracks first; iters_out (optional): what each track took. Neither changes a result.
int engine_lk(BatchEngine* E, int prev_slot, int next_slot, const float* prev_xy, int n, float* out_xy, uint8_t* status, float* err,
              const uint8_t* predicted_iters = nullptr, uint8_t* iters_out = nullptr, int ring_round = -1);
// pmv_lk_track_ex's / pmv_lk_track_fb's (fb) contract: a request of the LK combiners. A round serves all its extended requests with one
// launch of the extended batch kernels, next to the k_lk_batch launch of its plain ones; an fb request counts n tracks against the round's
// capacity. Tracks go in the engine's default order. next_xy: in (with PMV_LK_USE_INITIAL_FLOW) and out.
int engine_lk_ex(BatchEngine* E, const char* who, int prev_slot, int next_slot, const float* prev_xy, int n, float* next_xy, int flags, uint8_t* status,
                 float* err, bool fb, float* back_xy, uint8_t* back_status, float* back_err);
// pmv_detect_gftt's (kind = Q_GFTT; out_score null) or pmv_detect_shitomasi's (Q_SHITOMASI) contract
int engine_detect(BatchEngine* E, ReqKind kind, int slot, const int* cells, int n_cells, int max_per_cell, double quality, double min_dist, int* out_xy,
                  double* out_score, int* out_count, int ring_round = -1);
// pmv_detect_gftt_ex's contract: a GFTT request that carries the caller's block size, response kind, k and optional mask (host memory,
// read by the combiner before the call returns). The reference's arguments without a mask are a plain GFTT request unless
// pmv_debug_gftt_general is on.
int engine_detect_gftt_ex(BatchEngine* E, const char* who, int slot, const int* cells, int n_cells, int max_per_cell, const pmv_gftt_params* p,
                          const uint8_t* mask, int mask_stride, int* out_xy, int* out_count);
// pmv_detect_gftt_frame's contract: a request of the detector combiner (the mask is read by the combiner before the call returns). The frame
// requests of a round that agree in block size, response kind, k, has-mask, quality, min_dist, capacity, the no-limit flag and the frame
// layout share ONE pass-1 and ONE pass-2 launch: each has its own record list, pass 2 runs one workgroup per request.
int engine_detect_gftt_frame(BatchEngine* E, const char* who, int slot, const int* roi4_or_null, int max_corners, const pmv_gftt_params* p, const uint8_t* mask,
                             int mask_stride, int* out_xy, int out_cap, int* out_count);
// pmv_detect_gftt_refill's contract: a frame request that carries a track list (read, like the base mask, by the combiner before the call
// returns). It joins the frame groups with has-mask = true; the refill requests of a round share ONE k_track_select and ONE k_track_paint
// launch in front of the frame launches.
int engine_detect_gftt_refill(BatchEngine* E, const char* who, int slot, const int* roi4_or_null, int max_corners, const pmv_gftt_params* p, const float* track_xy,
                              const int* track_prio_or_null, int n_tracks, int radius, const uint8_t* base_mask_or_null, int base_stride, uint8_t* out_keep,
                              int* out_xy, int out_cap, int* out_count);
// pmv_corner_subpix's contract: a request of the detector combiner. Requests of a round that agree in the six parameters share one
// launch, whatever their slots and frame sizes.
int engine_corner_subpix(BatchEngine* E, const char* who, int slot, float* xy, int n, const pmv_subpix_params* p, uint8_t* out_iters, uint8_t* out_flags);
// pmv_detect_fast's contract (a cell may be as large as the frame): a request of the detector combiner
int engine_detect_fast(BatchEngine* E, int slot, const int* cells, int n_cells, int max_per_cell, int threshold, int nonmax, int* out_xy, float* out_response,
                       int* out_count, int ring_round = -1);
// pmv_knn_match's contract: a request of the LK combiners (the matcher role), served by one k_knn_round launch per round; counted under LK
int engine_knn(BatchEngine* E, int src_slot, int cmp_slot, const int* src_xy, int n, const int* cmp_xy, int m, int n_neighbours, int window, int* out_best,
               float* out_err, int ring_round = -1);
int engine_pnp(BatchEngine* E, int seq, const float* obj_xyz, const float* img_xy, int m, const double* K, double* rvec, double* tvec, int iterations,
               float reproj_err, double confidence, int* out_inliers, int* out_n_inliers);
int engine_ba(BatchEngine* E, int seq, double* cams, int nc, double* pts, int np, const double* obs_xy, const int* cam_idx, const int* pt_idx, int n_obs,
              const double* K, double huber, int max_iterations, pmv_ba_summary* summary = nullptr);
int engine_dlt(BatchEngine* E, int seq, const double* q1, const double* q2, int n, const double* P1x4, const uint8_t* mask_in, double* out_Q,
               uint8_t* out_mask, int* out_good);
// pmv_triangulate_tracks' contract: a request of the DLT combiner; a round serves all its requests of this kind with one k_tri_tracks_batch
// launch, next to the k_tri_dlt_batch launch of its two-view ones. An empty problem (np == 0 or n_obs == 0) enters no round.
int engine_tri_tracks(BatchEngine* E, int seq, const double* P3x4, int nc, const double* obs_xy, const int* cam_idx, const int* pt_idx, int n_obs, int np,
                      const pmv_tri_params* p_or_null, double* out_xyz, uint8_t* out_status, double* out_err_or_null, int* out_good);
int engine_fivepoint(BatchEngine* E, int seq, const double* q1, const double* q2, int n, const int* samples, int n_hyp, float thr, double* models,
                     int* n_models, int* counts);
// pmv_find_essential_mat's contract: one workgroup of the round's k_essential_ransac launch; returns when the request's own completion word is
// seen (or, after a failed launch, with the combiner's error), which may be before the round's launch ends
int engine_essential(BatchEngine* E, int seq, const double* p1_xy, const double* p2_xy, int n, const double* K, double prob, double threshold, double* E9,
                     uint8_t* mask, int* out_found, int* out_samples_drawn);
// pmv_find_fundamental_mat's contract, in the same form: one workgroup of the round's k_fundamental_ransac launch
int engine_fundamental(BatchEngine* E, int seq, const float* p1_xy, const float* p2_xy, int n, double threshold, double confidence, double* F9, uint8_t* mask,
                       int* out_found, int* out_samples_drawn);
// pmv_find_homography's contract, in the same form: one workgroup of the round's k_homography_ransac launch
int engine_homography(BatchEngine* E, int seq, const float* p1_xy, const float* p2_xy, int n, double threshold, double confidence, int max_iters, double* H9,
                      uint8_t* mask, int* out_found, int* out_samples_drawn);
}  // namespace pmv
