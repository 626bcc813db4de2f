// Back-end (PnP / BA) launch interfaces shared by backend*.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include "../../include/pmv_hip.h"
#include "pmv_mem.h"
#include "backend_layout.h"   // MAX_HYP, FP_MAX_HYP, PNP_HDR, ESS_HDR, the result-block headers and every staging block's layout

namespace pmv {

// Device / pinned buffers of ONE back-end problem slot (PnP, BA, two-view DLT workspaces and the single-copy staging blocks). The
// context owns one (the plain C-ABI calls); the batch engine owns one per concurrent sequence.

struct BackendBuffers {   // every buffer: one row of backend_alloc's table; freed with the set (backend_free)
    unsigned done_seq = 0;   // sequence number of the last call that signals its completion through the result block
    // BA problem
    Buf<double> d_cams, d_pts, d_obs, d_K;
    Buf<int> d_cam_idx, d_pt_idx, d_pobs_start, d_pobs_list, d_cobs_start, d_cobs_list;
    // BA workspaces
    Buf<double> d_x, d_cand, d_scale, d_diag, d_D2, d_step, d_res, d_J, d_Einv, d_gp, d_Yd, d_Wd, d_S, d_rhs, d_Gpart, d_summary;
    size_t ydwd_elems = 0, gpart_elems = 0;
    Buf<unsigned long long> d_stamps;
    Buf<void> d_bastate;
    Buf<double> d_bapart;
    Buf<char> d_tri_in, d_tri_out;
    Buf<char> d_fp_work;   // five-point round: [models FP_MAX_HYP x 90 doubles | n_models FP_MAX_HYP ints] (inputs share d_tri_in: fivepoint_layout)
    Buf<char> d_ess_in;    // whole findEssentialMat RANSAC: the in-block of essential_layout
    Buf<char> d_fund_in;   // whole findFundamentalMat RANSAC: the in-block of fundamental_layout; made by the set's first such call (fundamental_prepare)
    Buf<char> d_tt_in;     // N-view triangulation: the in-block of tri_tracks_layout
    // single-copy transfers: one mapped pinned staging block (result blocks are written straight into it through .dm()) and one device
    // block per direction
    Buf<char> h_stage;
    Buf<char> d_ba_io;     // ba_io_layout
    Buf<char> d_pnp_in;    // the in-block of pnp_layout
    Buf<char> d_pnp_out;   // [PnPResultHdr | inliers]
    // PnP
    Buf<float> d_obj, d_img;
    Buf<int> d_samples, d_counts, d_inliers, d_info;
    Buf<double> d_models, d_rt, d_Kp;
    Buf<uint8_t> d_masks;
};

struct BAArgs {
    // problem (device)
    double* cams; double* pts; const double* obs; const int* cam_idx; const int* pt_idx; const double* K;
    const int* pobs_start; const int* pobs_list; const int* cobs_start; const int* cobs_list;
    const int4* erec;  // per entry e of pobs_list: (observation index, camera, point, dup flag) in one 16-byte record; dup flag: 0 = only
                       // observation of its (point, camera), 1 = first of several, 2 = a later one
    int nc, np, nobs, max_iterations;
    double huber;
    // workspaces (device)
    double *x, *cand, *scale, *diag, *D2, *step, *res, *J, *Einv, *gp, *Yd, *Wd, *S, *rhs, *Gpart, *summary;
    int ldw, krows, tiles_r, tiles_c, kslices, kper, gp_rows;
    unsigned long long* stamps;   // optional (diagnostic): 32 accumulated shader-clock phase timers
    double* out;                  // optional: host-mapped result block [summary BA_SUM_SLOTS | cams 6*nc | pts 3*np] (multi-kernel LM)
    unsigned done_seq;            // != 0 (with `out`): the finish kernel stores it last into the low word of summary slot BA_SUM_DONE (the host spins on it)
};

hipError_t launch_ba_residuals(hipStream_t s, const double* cams, const double* pts, const double* obs, const int* cam_idx,
                               const int* pt_idx, int nobs, const double* K, double* out_r, double* out_J);
hipError_t launch_ba_lm(hipStream_t s, const BAArgs& A);
// multi-kernel LM (default); d_state: >= 512 + 4*BA_MAX_ITERATIONS B, d_part: >= (nobs/256 + 5*np/64 + 58*nc + 3*nobs + 16) doubles
constexpr int BA_MAX_ITERATIONS = 512;   // per-iteration flags of the multi-kernel LM
hipError_t launch_ba_multi(hipStream_t s, const BAArgs& A, void* d_state, double* d_part);
hipError_t launch_pnp(hipStream_t s, const float* d_obj, const float* d_img, int m, const double* d_K, const int* d_samples,
                      int n_hyp, float thr, double confidence, double* d_models, uint8_t* d_masks, int* d_counts,
                      double* d_rt_out, int* d_inliers, int* d_info, char* host_out /* mapped pinned [PnPResultHdr | inliers] */,
                      unsigned long long* d_stamps /* diagnostic, may be null */, unsigned done_seq = 0 /* see pnp_select_refit_body */);

// one problem of a batched multi-kernel LM launch chain: the arguments launch_ba_multi derives for a single solve, kept in device memory
struct BAProb {
    BAArgs A;
    void* st2[2];            // double-buffered BAGState
    int* chol_flags;
    double *part_cost, *part_gmax, *part4, *Ublk, *rhsblk, *candrot, *tmp3;
    int nbo, nbp, clear_blocks, tiles;
};
struct BABatchDims { int n_probs, max_eval_blocks, max_nc, max_nbp, max_tiles, max_m, max_iterations; };
// fills everything of `P` that launch_ba_multi computes from A / d_state / d_part (host side; the result is copied to the device)
void ba_fill_prob(BAProb& P, const BAArgs& A, void* d_state, double* d_part);
hipError_t launch_ba_multi_batch(hipStream_t s, const BAProb* d_probs, const BABatchDims& D);
// the one-workgroup-per-problem form (pmv_set_ba_mode(ctx, 1)): d_args[i] = problem i, max_m = largest 6 * nc of the batch
hipError_t launch_ba_lm_batch(hipStream_t s, const BAArgs* d_args, int n_probs, int max_m);
// one RANSAC problem of a batched PnP launch (device pointers)
struct PnPProblem {
    const float* obj; const float* img; const int* samples; const double* K;   // K: 9 doubles + 10^k table (see pmv_pnp_ransac)
    double* models; uint8_t* masks; int* counts; double* rt_out; int* inliers; int* info; char* host_out;
    int m, n_hyp; float thr; double confidence;
};
hipError_t launch_pnp_batch(hipStream_t s, const PnPProblem* d_probs, int n_probs, int max_hyp);
// one findEssentialMat RANSAC round of a batched five-point launch (backend_fivepoint.hip): n_hyp samples of 5 correspondences each
struct FivePointProblem {
    const int* samples; const double* q1; const double* q2;   // device inputs: 5 n_hyp indices, n normalised points each
    double* models_d; int* n_models_d;                        // device: n_hyp x 90 doubles, n_hyp ints (read by the scoring kernel)
    double* models_h; int* n_models_h; int* counts_h;         // mapped pinned results: models, model counts, n_hyp x 10 inlier counts
    int n, n_hyp; float thr;
};
hipError_t launch_fivepoint_batch(hipStream_t s, const FivePointProblem* d_probs, int n_probs, int max_hyp);
// one whole RANSAC request (pmv_ransac.h): one workgroup runs the adaptive loop of one cv::findEssentialMat (k_essential_ransac,
// backend_fivepoint.hip; Pt = double), cv::findFundamentalMat call (k_fundamental_ransac, backend_fundamental.hip; Pt = float) or
// cv::findHomography call (k_homography_ransac, backend_homography.hip; Pt = float, the blocks of the fundamental call)
template <class Pt> struct WholeProblem {
    const Pt* p1; const Pt* p2;           // device: n points (x, y) each - normalised for E, pixel positions for F
    const double* iters;                  // device: [log(1 - prob) | for g = 0..n inliers: log(1 - (1 - (n - g) / n)^S), -inf where RANSACUpdateNumIters returns 0], S = 5, 7 or 4
    char* out;                            // mapped pinned result block: [WholeResultHdr (E or F, found, samples drawn, best count, done_seq) | mask n bytes]
    int n, max_iters; float thr;
    unsigned done_seq;                    // != 0; the kernel's last store, into WholeResultHdr::done (the caller waits for it)
};
using EssentialProblem = WholeProblem<double>;
using FundamentalProblem = WholeProblem<float>;
static_assert(sizeof(WholeProblem<double>) <= ESS_HDR, "the record is the header of the input block");
// the record of a request of n points with the iteration cap (cv's 1000 for E and F, the caller's maxIters for H) and the threshold in the points' unit
constexpr int WHOLE_MAX_ITERS = 1000;
template <class Pt> inline WholeProblem<Pt> whole_problem(const Pt* p1, const Pt* p2, const double* iters, char* out, int n, double threshold, int max_iters, unsigned done_seq) {
    return WholeProblem<Pt>{p1, p2, iters, out, n, max_iters, (float)(threshold * threshold), done_seq};
}
constexpr int ESS_MAX_WAVES = 16;   // hypotheses per in-kernel round at most (wavefronts of the workgroup)
constexpr int ESS_DEFAULT_WAVES = 8;   // R of DESIGN.md §4: 8 x 6.2 KB = 49 KB of LDS, three workgroups per CU
int essential_round_width();        // hypotheses per in-kernel round (PMV_ESSENTIAL_R overrides the default, 1..ESS_MAX_WAVES)
hipError_t launch_essential_ransac(hipStream_t s, const EssentialProblem* d_probs, int n_probs);
constexpr int FUND_MAX_R = 64;       // hypotheses per in-kernel round at most (one lane of a wavefront each)
constexpr int FUND_DEFAULT_R = 64;   // R of DESIGN.md §4 (measured: the widest round is the fastest on eight of nine ubench rows)
int fundamental_round_width();       // hypotheses per in-kernel round (PMV_FUNDAMENTAL_R overrides the default, 1..FUND_MAX_R)
void fundamental_set_round_width(int r);   // pmv_debug_set_fundamental_r: r in 1..FUND_MAX_R from the next launch on, 0 = back to the above
hipError_t launch_fundamental_ransac(hipStream_t s, const FundamentalProblem* d_probs, int n_probs);
using HomographyProblem = WholeProblem<float>;   // (the record and the blocks of a fundamental request: fundamental_layout, d_fund_in)
constexpr int HG_R = 64;             // hypotheses per in-kernel round (one lane of a wavefront each)
constexpr int HG_MAX_ITERS = 10000;  // pmv_find_homography's max_iters at most
hipError_t launch_homography_ransac(hipStream_t s, const HomographyProblem* d_probs, int n_probs);
// one two-view problem of a batched DLT launch
struct DltProblem { const double* P1x4; const double* q1; const double* q2; const uint8_t* mask_in; double* Q; uint8_t* mask; int n; };
hipError_t launch_tri_dlt_batch(hipStream_t s, const DltProblem* d_probs, int n_probs, int max_n);
hipError_t launch_tri_dlt(hipStream_t s, const double* d_P1x4, const double* d_q1, const double* d_q2, const uint8_t* d_mask_in, int n,
                          double* d_Q, uint8_t* d_mask);
// one N-view triangulation request (k_tri_tracks / k_tri_tracks_batch, backend_tritracks.hip): one lane per landmark
struct TriTracksProblem {
    const double* P; const double* C;     // device: nc projection matrices (12 doubles each); nc camera centres (read with parallax_on only)
    const double* obs; const int* cam;    // device: the observations re-ordered into per-landmark runs - (x, y) and camera of each
    const int* start;                     // device: np + 1 run starts
    unsigned* counter;                    // device: workgroups of this request that are done (0 when the launch starts)
    char* out;                            // mapped pinned result block: [completion word, TT_OUT_HDR bytes | xyz 3 np | err np doubles | status np bytes]
    double min_depth, max_depth, max_reproj, cos_thr;   // cos_thr: cos(min_parallax_deg) from the host's libm
    int nc, np, min_views, refine_iters, parallax_on;
    unsigned done_seq;                    // != 0; the request's last store, into the result block's completion word
};
static_assert(sizeof(TriTracksProblem) <= TT_HDR, "the record is the header of the input block");
constexpr int TT_LDS_CAMS = 64;           // projection matrices and centres in LDS up to this many cameras (7.5 KB); beyond it through L2
constexpr int TT_MAX_REFINE = 20;         // pmv_tri_params::refine_iters at most
hipError_t launch_tri_tracks(hipStream_t s, const TriTracksProblem* d_rec, int np);
hipError_t launch_tri_tracks_batch(hipStream_t s, const TriTracksProblem* d_probs, int n_probs, int max_np);

// prepare / finish halves of the back-end entry points (backend.hip), shared by the single calls and the batch engine
struct PnPProblem; struct DltProblem;
}  // namespace pmv
struct pmv_ctx;
namespace pmv {
int backend_alloc(pmv_ctx* c, BackendBuffers** out);
void backend_free(BackendBuffers* b);
int pnp_check(pmv_ctx* ctx, const float* obj_xyz, const float* img_xy, int m, const double* K, double* rvec, double* tvec, int iterations,
              double confidence, int* out_inliers, int* out_n_inliers);
// Every *_prepare carves b's blocks by the call's layout (backend_layout.h), refuses with PMV_ERR_CAPACITY what does not fit them and hands
// the layout back; the stage-in copy, the completion word and *_finish use that same value.
int pnp_prepare(pmv_ctx* ctx, BackendBuffers* b, const float* obj_xyz, const float* img_xy, int m, const double* K, int iterations, float reproj_err,
                double confidence, PnPProblem* P, PnPLayout* L);
void pnp_finish(pmv_ctx* ctx, BackendBuffers* b, const float* obj_xyz, const float* img_xy, int m, const double* K, double* rvec, double* tvec,
                int iterations, float reproj_err, double confidence, const PnPLayout& L, int* out_inliers, int* out_n_inliers);
int ba_check(pmv_ctx* ctx, const double* cams, int nc, const double* pts, int np, const double* obs_xy, const int* cam_idx, const int* pt_idx,
             int n_obs, const double* K, double huber_delta, int max_iterations);
int ba_prepare(pmv_ctx* ctx, BackendBuffers* b, const double* cams, int nc, const double* pts, int np, const double* obs_xy, const int* cam_idx,
               const int* pt_idx, int n_obs, const double* K, double huber_delta, int max_iterations, bool multi, BAArgs* A, BaIoLayout* L);
void ba_finish(pmv_ctx* ctx, BackendBuffers* b, double* cams, int nc, double* pts, int np, const double* obs_xy, const int* cam_idx,
               const int* pt_idx, int n_obs, const double* K, double huber_delta, int max_iterations, const BaIoLayout& L, pmv_ba_summary* summary);
// five-point round: samples (5 n_hyp ints) of n normalised correspondences; thr = squared Sampson threshold as float
// (the outputs of pmv_fivepoint_hypotheses are checked by fivepoint_check, everything else by fivepoint_prepare)
int fivepoint_check(pmv_ctx* ctx, const double* models, const int* n_models, const int* counts);
int fivepoint_prepare(pmv_ctx* ctx, BackendBuffers* b, const double* q1, const double* q2, int n, const int* samples, int n_hyp, float thr,
                      FivePointProblem* P, FivePointLayout* L);
void fivepoint_finish(BackendBuffers* b, int n_hyp, const FivePointLayout& L, double* models, int* n_models, int* counts);
// whole findEssentialMat: argument rules of pmv_find_essential_mat (outputs untouched on error); prepare normalises the points into b's pinned
// block behind the problem record, builds the iteration table with the host's libm and clears the completion word; finish reads the result block
int essential_check(pmv_ctx* ctx, const char* who, const double* p1_xy, const double* p2_xy, int n, const double* K, double prob, double threshold,
                    double* E9, uint8_t* mask, int* out_found, int* out_samples_drawn);
int essential_prepare(pmv_ctx* ctx, BackendBuffers* b, const double* p1_xy, const double* p2_xy, int n, const double* K, double prob, double threshold,
                      EssentialProblem* P, WholeLayout* L);
volatile unsigned* whole_done_word(BackendBuffers* b, const WholeLayout& L);   // of either whole-RANSAC call: the result blocks share their header
void whole_finish(BackendBuffers* b, int n, const WholeLayout& L, double* M9, uint8_t* mask, int* out_found, int* out_samples_drawn);
// whole findFundamentalMat: argument rules of pmv_find_fundamental_mat (outputs untouched on error); prepare makes b's d_fund_in on first use,
// copies the points into b's pinned block behind the problem record, builds the iteration table with the host's libm and clears the completion word
int fundamental_check(pmv_ctx* ctx, const char* who, const float* p1_xy, const float* p2_xy, int n, double threshold, double confidence, double* F9,
                      uint8_t* mask, int* out_found, int* out_samples_drawn);
int fundamental_prepare(pmv_ctx* ctx, BackendBuffers* b, const float* p1_xy, const float* p2_xy, int n, double threshold, double confidence,
                        FundamentalProblem* P, WholeLayout* L);
// whole findHomography: argument rules of pmv_find_homography (outputs untouched on error; homography_args_check is their ctx-free statement,
// err: the message, 256 bytes); prepare is fundamental_prepare's with 4 model points and the caller's iteration cap
int homography_args_check(int max_tracks, const char* who, const float* p1_xy, const float* p2_xy, int n, double threshold, double confidence, int max_iters,
                          const double* H9, const uint8_t* mask, const int* out_found, const int* out_samples_drawn, char* err);
int homography_check(pmv_ctx* ctx, const char* who, const float* p1_xy, const float* p2_xy, int n, double threshold, double confidence, int max_iters, double* H9,
                     uint8_t* mask, int* out_found, int* out_samples_drawn);
int homography_prepare(pmv_ctx* ctx, BackendBuffers* b, const float* p1_xy, const float* p2_xy, int n, double threshold, double confidence, int max_iters,
                       HomographyProblem* P, WholeLayout* L);
// cv::recoverPose around a DLT launch: `dlt` is pmv_triangulate_candidates' contract on the caller's workspace set; PMV_OK or its error
int recover_pose_check(pmv_ctx* ctx, const char* who, const double* E9, const double* p1_xy, const double* p2_xy, int n, const double* K, double* R9,
                       double* t3, uint8_t* mask, double* tri4n, int* out_good);
// argument rules of pmv_triangulate_candidates and, under its own name, of the _ahead form (ctx is not null)
int dlt_check(pmv_ctx* ctx, const char* who, const double* q1, const double* q2, int n, const double* P1x4, const uint8_t* mask_in, const double* out_Q,
              const uint8_t* out_mask, const int* out_good);
int dlt_prepare(pmv_ctx* ctx, BackendBuffers* b, const double* q1, const double* q2, int n, const double* P1x4, const uint8_t* mask_in, DltProblem* P,
                DltLayout* L);
void dlt_finish(pmv_ctx* ctx, BackendBuffers* b, const double* q1, const double* q2, int n, const double* P1x4, const uint8_t* mask_in,
                const DltLayout& L, double* out_Q, uint8_t* out_mask, int* out_good);
// N-view triangulation of track landmarks: argument rules of pmv_triangulate_tracks (outputs untouched on error; tri_tracks_args_check is
// their ctx-free statement for a context of the given BA caps, err: the message, 256 bytes; p_or_null = null: the defaults). prepare groups
// the observations by landmark (stable counting sort), computes the camera centres if the parallax gate is on (PMV_ERR_INVALID for a camera
// with det M == 0), fills b's pinned block and the record and clears the completion word; finish reads the result block. A problem with
// np == 0 or n_obs == 0 is not prepared: tri_tracks_empty writes its outputs.
pmv_tri_params tri_tracks_defaults();
int tri_tracks_args_check(int max_cams, int max_points, int max_obs, const char* who, const double* P3x4, int nc, const double* obs_xy, const int* cam_idx,
                          const int* pt_idx, int n_obs, int np, const pmv_tri_params* p_or_null, const double* out_xyz, const uint8_t* out_status,
                          const int* out_good, char* err);
int tri_tracks_check(pmv_ctx* ctx, const char* who, const double* P3x4, int nc, const double* obs_xy, const int* cam_idx, const int* pt_idx, int n_obs, int np,
                     const pmv_tri_params* p_or_null, double* out_xyz, uint8_t* out_status, int* out_good);
int tri_tracks_prepare(pmv_ctx* ctx, BackendBuffers* b, const double* P3x4, int nc, const double* obs_xy, const int* cam_idx, const int* pt_idx, int n_obs,
                       int np, const pmv_tri_params* p_or_null, TriTracksProblem* P, TriTracksLayout* L);
void tri_tracks_finish(BackendBuffers* b, int np, const TriTracksLayout& L, double* out_xyz, uint8_t* out_status, double* out_err_or_null, int* out_good);
void tri_tracks_empty(int np, double* out_xyz, uint8_t* out_status, double* out_err_or_null, int* out_good);
}  // namespace pmv
