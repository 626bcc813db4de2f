/* pmv_hip.h — C ABI of the MI355X (gfx950) visual-odometry hot path.
 *
 * Drop-in boundary: each entry point replaces the third-party call that one of the
 * reference's plugin implementations makes behind its Base* interface.  Citations are into the
 * reference tree (JeanElsner/practical-multi-view):
 *
 *   pmv_frame_upload / pmv_frames_upload   Frame::Frame + cv::buildOpticalFlowPyramid   (Frame.cpp:31-42,
 *                                          implicit inside OpenCVLucasKanadeFM.cpp:15)
 *   pmv_detect_gftt                        cv::goodFeaturesToTrack per grid cell         (OpenCVGoodFeatureExtractor.cpp:7,
 *                                          called from OdometryPipeline.cpp:357 / :450)  -> BaseFeatureExtractor.h:21
 *   pmv_detect_gftt_frame                  cv::goodFeaturesToTrack on the whole frame or one region of any size, one call per frame
 *   pmv_detect_gftt_refill                 the same with the keep-away mask made on the device from the caller's track list (setMask)
 *   pmv_detect_gftt_ex                     cv::goodFeaturesToTrack with the caller's mask, blockSize, useHarrisDetector, k (a KLT front end
 *                                          of the caller's own; the reference passes cv::Mat(), 3, 3, false, 0.04)
 *   pmv_corner_subpix                      cv::cornerSubPix on level 0 of a slot (the step between the detector and LK in the caller's own
 *                                          KLT front end; the reference hands integer corners on, OpenCVGoodFeatureExtractor.cpp:7)
 *   pmv_frames_clahe                       cv::CLAHE::apply on level 0 of slots (the contrast equalisation a KLT front end of the caller's own runs
 *                                          in front of the pyramid; the reference tracks the plain gray image, Frame.cpp:40-41)
 *   pmv_frames_remap                       cv::remap(INTER_LINEAR, BORDER_CONSTANT) on level 0 of slots: the lens undistortion every camera but a
 *                                          rectified one needs in front of everything else (the reference takes K alone: a pinhole camera)
 *   pmv_undistort_points                   cv::undistortPoints(src, dst, K, dist): the lift of tracked pixels onto the normalised image plane
 *                                          (a VINS-style front end's liftProjective; also stage 9 of the tracker step, pmv_klt_set_observe)
 *   pmv_project_points                     cv::projectPoints without rvec / tvec: points of the camera frame onto the image (a VINS-style
 *                                          front end's spaceToPlane: where known landmarks should appear, as LK's initial flow)
 *   pmv_camera_create_fisheye              a camera of cv::fisheye's equidistant model (Kalibr "equidistant") for the two calls above and the
 *                                          tracker step; pmv_fisheye_map_build is cv::fisheye::initUndistortRectifyMap for pmv_frames_remap
 *   pmv_detect_shitomasi                   ShiTomasiFeatureExtractor::extractFeatures    (ShiTomasiFeatureExtractor.cpp:5-75,
 *                                          Frame.cpp:58-86,119-138)                      -> BaseFeatureExtractor.h:21
 *   pmv_lk_track                           cv::calcOpticalFlowPyrLK                      (OpenCVLucasKanadeFM.cpp:15) -> BaseFeatureMatcher.h:22
 *   pmv_knn_match                          kNNFeatureMatcher::matchFeatures' arithmetic   (kNNFeatureMatcher.cpp:13-31,63-122) -> BaseFeatureMatcher.h:22
 *   pmv_detect_fast                        cv::FAST                                      (OpenCVFASTFeatureExtractor.cpp:8) -> BaseFeatureExtractor.h:21
 *   pmv_pnp_ransac                         cv::solvePnPRansac                            (OpenCVEPnPSolver.cpp:35-36) -> BasePnPSolver.h:19
 *   pmv_fivepoint_hypotheses               cv::findEssentialMat (RANSAC hypotheses)      (OpenCVFivePointTri.cpp:24) -> BaseTriangulator.h
 *   pmv_triangulate_candidates             cv::recoverPose (triangulation + cheirality)  (OpenCVFivePointTri.cpp:27) -> BaseTriangulator.h
 *   pmv_find_essential_mat                 cv::findEssentialMat (the whole RANSAC)       (OpenCVFivePointTri.cpp:24) -> BaseTriangulator.h
 *   pmv_find_fundamental_mat               cv::findFundamentalMat, FM_RANSAC (a KLT loop's rejectWithF; not a call of the reference)
 *   pmv_find_homography                    cv::findHomography, RANSAC with its refit (planar scenes, pure rotations; not a call of the reference)
 *   pmv_triangulate_tracks                 N-view DLT + Gauss-Newton + gates per track landmark (FeatureManager::triangulate of a VINS-style caller; not a call of the reference)
 *   pmv_recover_pose                       cv::recoverPose (the whole call)              (OpenCVFivePointTri.cpp:27) -> BaseTriangulator.h
 *   pmv_ba_residuals / pmv_ba_solve        ProjectionResidual + ceres::Solve             (ProjectionResidual.h:38-58,
 *                                          CeresBundleAdjustment.cpp:50-61)              -> BaseOptimizer.h:15
 *
 * Conventions: plain pointers and sizes only; every in/out buffer is caller-allocated HOST memory
 * unless a parameter is documented as a device frame slot; the opaque context owns all device
 * memory and two HIP streams (front-end: detect/LK, back-end: PnP/BA — the reference's two threads,
 * OdometryPipeline.cpp:261-262).  All functions return 0 on success or a negative pmv_status;
 * pmv_last_error() gives the text.  Nothing throws across this boundary.  There is NO CPU fallback:
 * if no gfx950 device / code object is available pmv_ctx_create fails.
 */
#ifndef PMV_HIP_H
#define PMV_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct pmv_ctx pmv_ctx;

enum pmv_status {
    PMV_OK = 0,
    PMV_ERR_NO_DEVICE = -1,   /* no HIP device / wrong arch */
    PMV_ERR_INVALID = -2,     /* bad argument (null, size, slot out of range) */
    PMV_ERR_CAPACITY = -3,    /* exceeds the capacity given at pmv_ctx_create */
    PMV_ERR_HIP = -4,         /* HIP runtime error, see pmv_last_error */
    PMV_ERR_DEGENERATE = -5,  /* e.g. fewer than 5 PnP points (cv::Exception in the reference) */
    PMV_ERR_OVERFLOW = -6     /* more corners than PMV_GFTT_UNLIMITED_CAP in a cell of a no-limit goodFeaturesToTrack call */
};

/* ---- context ------------------------------------------------------------------------------- */
/* max_w/max_h: largest frame; n_slots: device frame slots (each holds a padded 8-bit pyramid);
 * max_tracks: largest N for lk_track / M for pnp; max_ba_cams / max_ba_points / max_ba_obs: BA caps. */
int pmv_ctx_create(pmv_ctx** out, int device, int max_w, int max_h, int n_slots, int max_tracks,
                   int max_ba_cams, int max_ba_points, int max_ba_obs);
void pmv_ctx_destroy(pmv_ctx* ctx);
const char* pmv_last_error(pmv_ctx* ctx); /* ctx may be NULL for create-time errors */
/* The text of the last failing call made on the CALLING thread (any context; "" if none): what a caller reads when several of its
 * threads use one context at once (the batch sessions below), where pmv_last_error may already hold another thread's message. */
const char* pmv_thread_error(void);
int pmv_sync(pmv_ctx* ctx);               /* waits for both streams */

/* ---- frames / pyramids ----------------------------------------------------------------------- */
/* Copy one 8-bit gray frame (host) into `slot` and build its LK pyramid (levels as cv::buildOpticalFlowPyramid
 * with winSize 32, maxLevel 4, or with the values of pmv_set_lk_params). */
int pmv_frame_upload(pmv_ctx* ctx, int slot, const uint8_t* gray, int w, int h, int stride);
/* The same from a colour image as Frame::Frame(file) reads it (Frame.cpp:33: imread(IMREAD_COLOR) = 8-bit BGR, `stride` bytes per row):
 * cv::cvtColor(BGR2GRAY) (Frame.cpp:40-41) runs on the device, then the pyramid as above. Identity for B = G = R (KITTI's gray PNGs). */
int pmv_frame_upload_bgr(pmv_ctx* ctx, int slot, const uint8_t* bgr, int w, int h, int stride);
/* The format of the host frames that the throughput paths take: pmv_frames_stage, pmv_frames_stream_begin, pmv_pipeline_run_streamed and
 * pmv_pipeline_run_batch_streamed (their `gray` / `host_frames` arguments). The reference never sees a gray image on input: Frame::Frame(file)
 * reads with imread(IMREAD_COLOR) and Frame::init runs cvtColor(BGR2GRAY) (Frame.cpp:33,40-41).
 *   PMV_FRAMES_GRAY  w * h bytes per frame (the default);
 *   PMV_FRAMES_BGR   tight 8-bit BGR, 3 * w bytes per row and 3 * w * h per frame, at any alignment. The conversion
 *                    gray = (B * 1868 + G * 9617 + R * 4899 + 8192) >> 14 runs on the device inside the kernel that writes level 0
 *                    (k_pad_level0_bgr), so a slot holds exactly what the gray path would have left for the converted image and every
 *                    result is bit-identical to the gray run on cv::cvtColor's output. Identity for B = G = R (KITTI's gray PNGs).
 * A context setting like pmv_set_ba_mode; pmv_frame_upload and pmv_frame_upload_bgr keep their own explicit formats, and
 * pmv_pipeline_params is not involved. Wherever the calls above speak of w * h gray bytes, a BGR context reads three times as many: staging
 * chunks, ingest rounds and landing buffers keep their byte sizes and hold a third as many frames, and pmv_batch_ingest_stats counts the
 * BGR bytes.
 * Lens undistortion and equalisation of the same host frames on their way in: pmv_set_frame_preproc, below the remap calls.
 *   Errors: a format other than the two above is PMV_ERR_INVALID; a call while a pmv_frames_stream_begin bracket or a batched run
 *   (pmv_pipeline_run_batch, pmv_pipeline_run_batch_streamed) is open on the context is PMV_ERR_INVALID, and the format stays as it was. */
enum pmv_frame_format { PMV_FRAMES_GRAY = 0, PMV_FRAMES_BGR = 1 };
int pmv_set_frame_format(pmv_ctx* ctx, int format);
/* Batch form: n frames, tightly packed (n*w*h bytes; BGR: n*3*w*h), into slots first_slot..first_slot+n-1. The gray data
 * is staged to HBM first (pmv_frames_stage: level 0 of each slot; a slot keeps no second copy of the frame), the pyramids are
 * built by pmv_frames_build (level 0's REFLECT_101 frame in place + the levels above) so that a benchmark can time the build with
 * inputs already resident in HBM. */
int pmv_frames_stage(pmv_ctx* ctx, int first_slot, int n, const uint8_t* gray, int w, int h);
int pmv_frames_build(pmv_ctx* ctx, int first_slot, int n);
/* Streamed ingest (Frame::Frame / Frame::init + the front-end's per-frame load, Frame.cpp:31-42, OdometryPipeline.cpp:212-220):
 * n tightly packed frames (gray, or BGR: pmv_set_frame_format; remapped / equalised on the way in: pmv_set_frame_preproc) in HOST memory (pageable, or pinned: then DMA'd straight from it) are moved into slots first_slot.. by the
 * context's feeder thread on its own HIP stream, round by round, each round's pyramids built as soon as its frames land.
 * pmv_frames_stream_begin returns at once; until pmv_frames_stream_end, pmv_lk_track / pmv_detect_* / pmv_knn_match on a slot of the
 * range first make the front-end stream wait for that slot's round (nothing else blocks), so tracking starts while later frames are
 * still on their way. pmv_frame_upload* / pmv_frames_stage into slots outside the range may be called meanwhile: they use a landing
 * area of their own. pmv_frame_num_levels / pmv_frame_get_level* do not wait: on a slot of the range they are meaningful only after a
 * tracking or detection call on that slot, or after pmv_frames_stream_end. `gray` must stay valid until pmv_frames_stream_end, which
 * joins the feeder thread. One stream per context. Memory: 4 pinned staging buffers of 16 frames and as many HBM landing buffers
 * (7.5 MB each at 1241x376), kept by the context. */
int pmv_frames_stream_begin(pmv_ctx* ctx, int first_slot, int n, const uint8_t* gray, int w, int h);
int pmv_frames_stream_end(pmv_ctx* ctx);
/* Debug/parity: copy pyramid level `level` of `slot` (unpadded, tightly packed) back to host. Returns level dims. */
int pmv_frame_get_level(pmv_ctx* ctx, int slot, int level, uint8_t* out, int* w, int* h);
int pmv_frame_num_levels(pmv_ctx* ctx, int slot); /* maxLevel actually built (>=0) or <0 */
/* Debug/parity: the same level WITH its 64-pixel BORDER_REFLECT_101 frame (what cv::buildOpticalFlowPyramid keeps around every level,
 * lkpyramid.cpp, here PMV_PYR_PAD wide): (w + 128) x (h + 128) bytes, tightly packed; returns the padded dims. */
#define PMV_PYR_PAD 64
int pmv_frame_get_level_padded(pmv_ctx* ctx, int slot, int level, uint8_t* out, int* pw, int* ph);

/* cv::createCLAHE(clip_limit, Size(tiles_x, tiles_y))->apply(level 0, level 0) on the slots first_slot .. first_slot + n - 1, then the
 * 64-pixel REFLECT_101 frame of level 0 and every level above rebuilt from the equalised image: the step a KLT front end of the caller's
 * own (VINS-style trackers by default) runs on every frame in front of the pyramid - so that such a front end never needs the frame in
 * host memory. The reference never equalises (Frame.cpp:40-41 hands the gray image on); the whole-sequence drivers do not call this.
 *   Slots: staged (pmv_frames_stage) or built (any upload, pmv_frames_build, a finished pmv_frames_stream_begin bracket); the slots of a
 *     range may differ in size. Afterwards every slot is built and holds byte for byte what pmv_frame_upload of the equalised image would
 *     have left, at every level with its border: pmv_frames_stage -> pmv_frames_clahe -> pmv_pipeline_run is the equalised run, whatever
 *     build_pyramids says. A second call equalises again, as cv would. The launches go on the front-end stream and the call returns after
 *     they complete. During a batch session the call stays legal under the caller's slot rule, like the other single calls.
 *   Arithmetic, for a w x h level 0 and histSize 256:
 *     1. Extended image: if w % tiles_x == 0 && h % tiles_y == 0 the image itself; otherwise the image extended on the right by
 *        tiles_x - w % tiles_x columns and at the bottom by tiles_y - h % tiles_y rows with REFLECT_101 - cv's quirk included: a dimension
 *        that DOES divide still gets a full extra tiles_x or tiles_y when the other one does not. tile size = (ext_w / tiles_x,
 *        ext_h / tiles_y), area = their product. The kernels take the extension from the INTERIOR of level 0, never from the slot's own
 *        border (a staged slot has none yet).
 *     2. Constants, computed once per frame on the host: lutScale = (float)255 / area (a float division); cl = clip_limit > 0 ?
 *        max((int)(clip_limit * area / 256), 1) : 0, evaluated in double and clamped to area before the cast (no bin can exceed area, so
 *        this changes no result); inv_tw = 1.0f / tile_w, inv_th = 1.0f / tile_h.
 *     3. Per tile: 256 int bins of the tile's area pixels. If cl > 0: clipped = sum of max(hist[i] - cl, 0), the bins are cut to cl,
 *        batch = clipped / 256, residual = clipped - 256 batch, every bin += batch, and if residual != 0: step = max(256 / residual, 1),
 *        for (i = 0; i < 256 && residual > 0; i += step, residual--) hist[i]++ (bin i gets the increment iff i % step == 0 &&
 *        i / step < residual).
 *     4. Per tile: lut[i] = saturate_u8(rint((float)sum * lutScale)) over the running int sum of the bins, rounding half to even (cvRound).
 *     5. Per pixel (x, y) of value v: txf = x * inv_tw - 0.5f, tx1 = floor(txf), tx2 = tx1 + 1, xa = txf - tx1, xa1 = 1.0f - xa, then
 *        tx1 = max(tx1, 0), tx2 = min(tx2, tiles_x - 1); the same for y; res = (lut[ty1][tx1][v] * xa1 + lut[ty1][tx2][v] * xa) * ya1 +
 *        (lut[ty2][tx1][v] * xa1 + lut[ty2][tx2][v] * xa) * ya in float, in this order, without contraction; dst = saturate_u8(rint(res)).
 *     Histograms are integer sums, so their order is free; nothing else needs one.
 *   Kernels: k_clahe_lut (one workgroup per tile and frame, a histogram per wavefront in LDS, one thread per bin for the rest) and
 *     k_clahe_apply (a pixel is read once and written once by the same thread, so it works in place), both driven by one record per frame:
 *     ONE pair of launches per 64 frames whatever their sizes, then pmv_frames_build's launches. The scratch (records and 64 x 64 KB of
 *     LUTs) is made by the first call on a context and is not sized by n. Booked under the level-0 profiling class.
 *   [mem: OpenCV 3.4 clahe.cpp; parity unpinned like the rest of the front end - tests/twin/clahe_twin.cpp is the CPU restatement that
 *   fixes the arithmetic, bit for bit.]
 * Errors (nothing is written, nothing is clamped): PMV_ERR_INVALID - a null ctx or p, tiles_x or tiles_y outside 1..16, clip_limit negative
 *   or not finite, an empty slot (the message names it), a call while a pmv_frames_stream_begin bracket or a batched run is open on the
 *   context; PMV_ERR_CAPACITY - a slot range outside n_slots, as for pmv_frames_build.
 * Out of scope: cv::equalizeHist, 16-bit images, more than 16 tiles in a direction. Host frames that enter through a feeder (the
 *   pmv_frames_stream_begin bracket and the two streamed runs) are equalised on their way in by pmv_set_frame_preproc; staged runs get it
 *   through pmv_frames_stage -> pmv_frames_clahe. pmv_frame_upload followed by pmv_frames_clahe builds the pyramid twice; the session form
 *   pmv_batch_frame_upload_clahe and the feeder form do not. */
typedef struct pmv_clahe_params {
    double clip_limit;   /* cv's clipLimit; 0 = no clipping; 0 <= clip_limit, finite */
    int tiles_x, tiles_y;/* cv's tileGridSize (width, height); 1 .. 16 each */
} pmv_clahe_params;
int pmv_frames_clahe(pmv_ctx* ctx, int first_slot, int n, const pmv_clahe_params* p);
/* diagnostic: {LUT + apply launch pairs of pmv_frames_clahe, session upload rounds that held at least one pmv_batch_frame_upload_clahe
 * request, launch pairs made for them} since the context was created. */
int pmv_debug_clahe_launches(pmv_ctx* ctx, long long* out3);

/* ---- lens undistortion: cv::remap of frame slots ------------------------------------------------ */
/* A remap map, created once per camera: map_x and map_y are the tight w x h CV_32FC1 maps of cv::remap, dst(x, y) = src(map_x(x, y),
 * map_y(x, y)) - from pmv_undistort_map_build, cv::initUndistortRectifyMap, cv::fisheye::initUndistortRectifyMap or the caller's own model.
 * The call converts them ONCE, on the host, into cv's fixed-point form and keeps the packed map in device memory; map_x and map_y may be
 * freed when it returns. At most 16 maps per context; a map's memory is sized by w h.
 *   Conversion per element (INTER_BITS 5): sx = cvRound(map_x * 32.0f) - a float product, which is exact, rounded half to even; a NaN or a
 *     value beyond int32 gives INT_MIN, as cvtss2si does; ix = saturate_s16(sx >> 5) with an arithmetic shift, fx = sx & 31. The same for y.
 *   Packing (private): two planes over the linear pixel index y w + x, each padded to a multiple of four entries - a dword (ix & 0xffff) |
 *     iy << 16 and a halfword fx | fy << 5: 6 bytes per pixel.
 *   [mem: OpenCV 3.4 imgwarp.cpp, remap with INTER_LINEAR, the CV_32FC1 pair converted as convertMaps does]
 * Errors: PMV_ERR_INVALID - a null argument, or w, h outside 1 .. the context's max_w, max_h; PMV_ERR_CAPACITY - a 17th map.
 * pmv_remap_map_destroy: PMV_ERR_INVALID for an unknown id, while a batch session is open on the context (its upload rounds read the
 * maps of their requests), and for a map that the current pmv_set_frame_preproc setting names (clear the setting first).
 * pmv_ctx_destroy frees the maps that are left. */
int pmv_remap_map_create(pmv_ctx* ctx, int w, int h, const float* map_x, const float* map_y, int* out_id);
int pmv_remap_map_destroy(pmv_ctx* ctx, int id);
/* cv::remap(level 0, level 0, map, INTER_LINEAR, BORDER_CONSTANT, Scalar(border_value)) on the slots first_slot .. first_slot + n - 1, then the
 * 64-pixel REFLECT_101 frame of level 0 and every level above rebuilt from the remapped image: with an undistortion map, cv::undistort on
 * the device, the first link of pmv_frames_remap -> pmv_frames_clahe -> pmv_detect_gftt_ex -> pmv_corner_subpix -> pmv_lk_track_fb. The
 * reference never undistorts (it takes K alone and KITTI's images are rectified); the whole-sequence drivers do not call this.
 *   Slots: the rules of pmv_frames_clahe - staged (pmv_frames_stage) or built; afterwards every slot is built and holds byte for byte what
 *     pmv_frame_upload of the remapped image would have left, at every level with its border, whatever build_pyramids says. A second call
 *     remaps again. The launches go on the front-end stream and the call returns after they complete. During a batch session the call
 *     stays legal under the caller's slot rule.
 *   Source and destination have the same size (cv::undistort's case): every slot's level-0 size must equal the map's size.
 *   Arithmetic per destination pixel, with (ix, iy, fx, fy) of the map: tap(x, y) = src(x, y) inside the w x h interior of level 0, else
 *     border_value - the taps are never read from the slot's own border (a staged slot has none yet);
 *     D = ((32 - fy)(32 - fx) tap(ix, iy) + (32 - fy) fx tap(ix + 1, iy) + fy (32 - fx) tap(ix, iy + 1) + fy fx tap(ix + 1, iy + 1) + 512) >> 10.
 *     This equals cv's (sum of w tap + 2^14) >> 15, because every weight of cv's table is 32 times the one above; it copies the source
 *     exactly where fx = fy = 0, and it covers cv's three branches (all taps inside, all outside, mixed) with one rule. Integer arithmetic:
 *     no order to fix.
 *   Kernel: k_remap, driven by one record per frame (slot, geometry entry, packed map, border value, scratch offset): ONE launch per 64
 *     frames. A gather cannot run in place: k_remap reads the raw interior of level 0 and writes a tight frame into a scratch area (made by
 *     the first call, 64 frames of the context's capacity, and is not sized by n); the list-form k_pad_level0 launch with that frame as its
 *     source writes level 0 and its border, the k_pyrdown launches the levels above. Booked under the level-0 profiling class.
 *   [mem: OpenCV 3.4 imgwarp.cpp, remapBilinear; parity with a real OpenCV is unpinned like the rest of the front end -
 *   tests/twin/remap_twin.cpp is the CPU restatement that fixes the bits.]
 * Errors (nothing is written, nothing is clamped): PMV_ERR_INVALID - a null ctx, an unknown map_id, border_value outside 0..255, an empty
 *   slot (the message names it), a slot whose level-0 size is not the map's (the message names the slot and both sizes), a call while a
 *   pmv_frames_stream_begin bracket or a batched run is open on the context; PMV_ERR_CAPACITY - a slot range outside n_slots, as for
 *   pmv_frames_build.
 * Out of scope: other interpolations and border modes, a destination size different from the source size, 16-bit images. Host frames that
 *   enter through a feeder (the pmv_frames_stream_begin bracket and the two streamed runs) are remapped on their way in by
 *   pmv_set_frame_preproc. pmv_frame_upload followed by pmv_frames_remap builds the pyramid twice; the session form
 *   pmv_batch_frame_upload_remap and the feeder form do not. */
int pmv_frames_remap(pmv_ctx* ctx, int first_slot, int n, int map_id, int border_value);
/* diagnostic: {k_remap launches of pmv_frames_remap, session upload rounds that held at least one pmv_batch_frame_upload_remap request,
 * k_remap launches made for them} since the context was created. */
int pmv_debug_remap_launches(pmv_ctx* ctx, long long* out3);
/* ---- remap and equalisation inside the feeder: real cameras on the streamed runs --------------------- */
/* Preprocessing of the host frames that the throughput paths take: a context setting next to pmv_set_frame_format, for callers whose camera
 * has a real lens and real exposure. It governs every frame that enters a slot from HOST memory through the feeder:
 *   the pmv_frames_stream_begin .. _end bracket, pmv_pipeline_run_streamed and pmv_pipeline_run_batch_streamed.
 * Per frame, in this order: BGR -> remap -> CLAHE -> border, that is
 *   1. cv::cvtColor(BGR2GRAY) if the context's format is PMV_FRAMES_BGR (pmv_set_frame_format);
 *   2. cv::remap(INTER_LINEAR, BORDER_CONSTANT, Scalar(border_value)) through the map whose size equals the frame's size (n_maps > 0);
 *   3. cv::CLAHE::apply with clahe_params (clahe != 0);
 *   4. the 64-pixel REFLECT_101 border of level 0 and the levels above.
 * Result: the slot holds, at every level with its border, byte for byte what pmv_frame_upload of the preprocessed gray image would have
 *   left - hence what pmv_frames_stage -> pmv_frames_remap -> pmv_frames_clahe leaves - and every pipeline result is bit-identical to the
 *   same run with the setting off on host frames preprocessed by tests/twin/remap_twin.cpp / clahe_twin.cpp. The caller passes the camera
 *   matrix that goes with the map (newK of pmv_undistort_map_build) as K9; the library does not touch K9.
 * Arithmetic: that of pmv_frames_remap and pmv_frames_clahe above, statement for statement (integer rule and float order included); a BGR
 *   tap is converted with (B * 1868 + G * 9617 + R * 4899 + 8192) >> 14 before the weights, the value k_pad_level0_bgr would have stored.
 * Staged feeds are untouched: frames already in slots - the staged feeds of pmv_pipeline_run_batch and of pmv_pipeline_run with
 *   build_pyramids, pmv_frames_stage, pmv_frames_build - are not preprocessed; the caller runs pmv_frames_remap / pmv_frames_clahe over
 *   them, as before. pmv_frame_upload* and the session uploads (pmv_batch_frame_upload_remap / _clahe) keep their own per-call forms.
 * Sizes: a feed may mix frame sizes; each sequence uses the map of its own size, so the maps of a setting have pairwise different sizes
 *   (a batch has one K9 per sequence, hence one camera per size). With n_maps > 0, a sequence with a host source and no map of its size is
 *   PMV_ERR_INVALID; the message names the sequence and the size, and it is raised before any thread starts or any slot changes.
 * Kernels and launches: a round of the feeder with preprocessing makes, after its copy, ONE k_remap_src launch in place of the level-0
 *   launch (remap on: the gather reads the round's tight source frames in the HBM landing buffer and writes the interior of level 0
 *   directly - one read of the taps, one write, no scratch frame; counted in pmv_debug_batch_launches where the level-0 launch it replaces
 *   is) or the level-0 launch as always (remap off); ONE k_clahe_lut + k_clahe_apply pair over the round's slots (CLAHE on; the LUT scratch
 *   is the feeder's, 256 bytes per tile and frame of a round, made by the first such feed); ONE in-place k_pad_level0 launch for the
 *   border; the k_pyrdown launches as always. One record per frame names its source, map, slot and geometry, so one launch serves a round
 *   of any sizes and maps. All are booked under the level-0 profiling class. k_remap_src keeps k_remap's map loads (16 + 8 bytes per four
 *   pixels, aligned); it stores one aligned dword where a thread's four pixels lie in one row at a column that is a multiple of 4 (always
 *   when w % 4 == 0) and bytes elsewhere.
 * No gather from host memory: a 2 x 2 byte gather across the host link is a link transaction per tap, so a feed with n_maps > 0 brings
 *   every host frame into HBM through the copy form first - whatever PMV_BATCH_INGEST says, and for a caller's pinned buffer as well
 *   (NBUF landing buffers in HBM, as PMV_BATCH_INGEST=copy). pmv_batch_ingest_stats keeps counting the bytes moved. A CLAHE-only feed keeps
 *   whichever form it would have had.
 * Off (the default; p_or_null == NULL, or n_maps == 0 && clahe == 0): the feeder makes exactly the launches it made before this setting
 *   existed and allocates nothing new.
 * Errors: PMV_ERR_INVALID - a null ctx; n_maps outside 0..PMV_PREPROC_MAX_MAPS; an unknown map id, or two maps of one size;
 *   border_value outside 0..255; with clahe != 0, parameters that pmv_frames_clahe would refuse; a call while a pmv_frames_stream_begin
 *   bracket or a batched run is open on the context. The setting then stays as it was, and nothing is clamped.
 * pmv_get_frame_preproc returns the setting in force (unused map_ids and, with clahe == 0, clahe_params are zero).
 * Out of scope: preprocessing of staged feeds; several maps of one size (per-sequence cameras of one size); other interpolations and border
 *   modes, 16-bit images, cv::equalizeHist; pmv_batch_frame_upload_remap and pmv_frames_remap keep their own launches. */
#define PMV_PREPROC_MAX_MAPS 8
typedef struct pmv_frame_preproc {
    int n_maps;                          /* 0 = no remap */
    int map_ids[PMV_PREPROC_MAX_MAPS];   /* ids of pmv_remap_map_create, pairwise different sizes */
    int border_value;                    /* 0..255, as pmv_frames_remap */
    int clahe;                           /* 0 = no equalisation */
    pmv_clahe_params clahe_params;       /* read only if clahe != 0; the ranges of pmv_frames_clahe */
} pmv_frame_preproc;
int pmv_set_frame_preproc(pmv_ctx* ctx, const pmv_frame_preproc* p_or_null);   /* null: off (the default) */
int pmv_get_frame_preproc(pmv_ctx* ctx, pmv_frame_preproc* out);
/* diagnostic: out4 = {feeder rounds that preprocessed, k_remap_src launches, k_clahe_lut + k_clahe_apply launch pairs, in-place
 * k_pad_level0 border launches made for them} since the context was created, over the bracket's and the batched runs' feeders. The border
 * launches are counted here only: pmv_debug_batch_launches keeps its meaning. */
int pmv_debug_preproc_launches(pmv_ctx* ctx, long long* out4);
/* diagnostic: bytes the library currently holds, over every context of the process: out2 = {device memory, pinned host memory}. Needs no
 * context. Every allocation has one owner that frees it, and these two counters are written where a block is made and where it is freed,
 * so the pair returns to its earlier value once everything made in between has been closed - whatever other processes do to the card. */
int pmv_debug_mem_live(long long* out2);
/* The map of cv::initUndistortRectifyMap(K, dist, R, newK, Size(w, h), CV_32FC1), on the host; needs no context (pmv_last_error(NULL) has
 * the message of a refusal). K9, R9, newK9: row-major 3 x 3; dist8 = (k1, k2, p1, p2, k3, k4, k5, k6); a null R is the identity, a null newK
 * is K. map_x, map_y: w h floats each, for pmv_remap_map_create.
 *   In double, for column j and row i: (X, Y, W) = (newK R)^-1 (j, i, 1), the inverse by adjugate and determinant; x = X / W, y = Y / W,
 *   r2 = x^2 + y^2; kr = (1 + ((k3 r2 + k2) r2 + k1) r2) / (1 + ((k6 r2 + k5) r2 + k4) r2); xd = x kr + p1 (2xy) + p2 (r2 + 2x^2);
 *   yd = y kr + p1 (r2 + 2y^2) + p2 (2xy); map_x = (float)(fx xd + cx), map_y = (float)(fy yd + cy) with K's fx, fy, cx, cy.
 *   cv walks the ray incrementally along a row, so its last double bits differ: this helper is held to a tolerance (one float ulp of the
 *   coordinate), not to bits; the bits that matter are those of pmv_frames_remap given the float maps. The maps of a cv::fisheye camera are
 *   pmv_fisheye_map_build's (below, with pmv_camera_create_fisheye).
 * Errors: PMV_ERR_INVALID - a null K9, dist8, map_x or map_y, a singular newK R, w or h < 1. */
int pmv_undistort_map_build(const double* K9, const double* dist8, const double* R9_or_null, const double* newK9_or_null, int w, int h, float* map_x,
                            float* map_y);

/* ---- cameras and cv::undistortPoints: tracked pixels onto the normalised image plane -----------------------------------------------------
 * A VINS-style tracker tracks in the raw image and lifts the few hundred points, not the frame. A camera object holds the intrinsics and the
 * distortion coefficients of pmv_undistort_map_build's model; pmv_undistort_points is cv::undistortPoints(src CV_32FC2, dst, K, dist) with
 * no R and no P, as a single call; the tracker step uses the same lift (pmv_klt_set_observe below).
 * Result definition: for point i < n, (u, v) = xy[2 i .. 2 i + 1]; all arithmetic in double, IEEE + - * / only, without contraction, operand
 *   order as written; ifx = 1.0 / fx and ify = 1.0 / fy are computed once on the host at pmv_camera_create and kept in the camera record:
 *     x0 = ((double)u - cx) * ifx;  y0 = ((double)v - cy) * ify;  x = x0;  y = y0;
 *     repeat iters times:
 *         r2     = x*x + y*y
 *         icdist = (1 + ((k6*r2 + k5)*r2 + k4)*r2) / (1 + ((k3*r2 + k2)*r2 + k1)*r2)
 *         dX     = 2*p1*x*y + p2*(r2 + 2*x*x)
 *         dY     = p1*(r2 + 2*y*y) + 2*p2*x*y
 *         x = (x0 - dX) * icdist;  y = (y0 - dY) * icdist
 *   out_ok[i] = 1 iff x and y are finite after the last iteration and still finite after rounding to float; then out_xy[2 i .. 2 i + 1] =
 *   ((float)x, (float)y). Otherwise out_ok[i] = 0 and out_xy = (0, 0): cv would return NaN, and the device's NaN bits are not the host's, so
 *   no NaN is ever written. This is the fixed-point inverse of the forward model pmv_undistort_map_build states, as OpenCV 3.4's
 *   undistortPoints iterates it (cv's default is iters = 5); parity with a real OpenCV is unpinned. The device equals the CPU restatement
 *   tests/twin/lift_twin.cpp bit for bit.
 * Device side: the cameras live in one small device table of the context, made by the first pmv_camera_create and released with the last
 *   camera. pmv_undistort_points is one launch on the front-end stream (one lane per point, FP64, the camera record read as uniform loads)
 *   and one wait; n == 0 is legal and launches nothing.
 * Errors (nothing is written, nothing is clamped): PMV_ERR_INVALID - a null argument; fx or fy zero or not finite; any parameter not finite;
 *   iters outside 1..50; an unknown camera id; a coordinate that is not finite or beyond 1e6 in magnitude (the message names the point);
 *   destroying a camera that a tracker's observation setting names. PMV_ERR_CAPACITY - a 17th camera; n < 0 or n above max_tracks.
 *   pmv_ctx_destroy frees the cameras that are left.
 * A camera of pmv_camera_create_fisheye (the equidistant model, below) is lifted by that model's own statement, given there.
 * Out of scope: camera models other than this one and cv::fisheye's equidistant one (skew and the omnidirectional model among them); the
 *   R / P arguments of undistortPoints; thin-prism and tilt coefficients (not built: a
 *   camera has the 8 coefficients below); the session form (pmv_batch_*); a forward distort_points call on normalised points (the forward
 *   model as a call is pmv_project_points below, from points of the camera frame). */
#define PMV_MAX_CAMERAS 16
typedef struct pmv_camera_params {
    double fx, fy, cx, cy;
    double dist[8];         /* k1, k2, p1, p2, k3, k4, k5, k6: the order of pmv_undistort_map_build */
    int    iters;           /* fixed-point iterations, 1 .. 50; cv's default is 5 */
} pmv_camera_params;
int pmv_camera_create(pmv_ctx* ctx, const pmv_camera_params* p, int* out_id);
int pmv_camera_destroy(pmv_ctx* ctx, int id);
int pmv_undistort_points(pmv_ctx* ctx, int cam_id, const float* xy, int n, float* out_xy, uint8_t* out_ok);
/* ---- cv::projectPoints without rvec and tvec: points of the camera frame onto the image ---------------------------------------------------
 * The forward direction of the lift above, through the same camera object: where a landmark the back end knows should appear in the next
 * frame (VINS: setPrediction / spaceToPlane). The pixels are meant as the initial flow of pmv_lk_track_ex / pmv_lk_track_fb_levels.
 * Result definition: for point i < n, (X, Y, Z) = xyz[3 i .. 3 i + 2] in the camera frame; all arithmetic in double, IEEE + - * / only, without
 *   contraction, operand order as written; fx and fy are the caller's own values (not 1 / ifx):
 *     x = X / Z;  y = Y / Z;  r2 = x*x + y*y
 *     kr = (1 + ((k3*r2 + k2)*r2 + k1)*r2) / (1 + ((k6*r2 + k5)*r2 + k4)*r2)
 *     xd = x*kr + (2*p1*x*y + p2*(r2 + 2*x*x));  yd = y*kr + (p1*(r2 + 2*y*y) + 2*p2*x*y)
 *     u = fx*xd + cx;  v = fy*yd + cy
 *   out_ok[i] = 1 iff X, Y and Z are finite, Z > 0, u and v are finite before and after their rounding to float, and |(float)u|, |(float)v| <=
 *   1e6 (the bound pmv_lk_track_ex puts on an initial flow); then out_xy[2 i .. 2 i + 1] = ((float)u, (float)v). Otherwise out_ok[i] = 0 and
 *   out_xy = (0, 0); no NaN is ever written. The pixel may lie outside the frame: that is the tracker's business. [mem: cv::projectPoints;
 *   parity with a real OpenCV is unpinned, like the lift.] The device equals the CPU restatement tests/twin/project_twin.cpp bit for bit.
 * Device side: one launch on the front-end stream (one lane per point, FP64, the camera record read as uniform loads) and one wait; n == 0 is
 *   legal and launches nothing. The call's block is made by the first call and released with the last camera.
 * Errors (nothing is written): PMV_ERR_INVALID - a null argument, an unknown camera id. PMV_ERR_CAPACITY - n < 0 or n above max_tracks. A
 *   coordinate of any value, NaN and infinities included, is no error: the point comes back with ok 0.
 * A camera of pmv_camera_create_fisheye (below) is projected by the equidistant model's forward statement, given there.
 * Out of scope: rvec / tvec (transform the points first), the Jacobian output, camera models other than this one and cv::fisheye's
 *   equidistant one, skew, thin-prism and tilt coefficients, the session form. */
int pmv_project_points(pmv_ctx* ctx, int cam_id, const double* xyz /* 3 n, camera frame */, int n, float* out_xy, uint8_t* out_ok);
/* ---- cv::fisheye cameras: the equidistant model (Kannala-Brandt, Kalibr "equidistant") ----------------------------------------------------
 * The wide-angle cameras of VIO rigs are calibrated with this model (VINS-Fusion and OpenVINS read it next to the radial-tangential one).
 * pmv_camera_create_fisheye makes a camera of it in the same table as pmv_camera_create; its id is a camera id wherever one is taken -
 * pmv_undistort_points, pmv_project_points, pmv_klt_set_observe (cam_id, right_cam_id, undistorted_f; every step form, single and group)
 * and pmv_klt_set_prediction - and pmv_camera_destroy frees it. A rig may mix models: a fisheye left and a radial-tangential right camera,
 * or a group of trackers with different cameras. No launch and no wait is added anywhere: the model is one field of the camera record, the
 * same for every lane of a launch, and a step with a fisheye camera is the same chain as a step with a radial-tangential one.
 * Arithmetic: double, IEEE + - * / only, without contraction, operand order as written, plus the correctly rounded double square root. The
 *   model needs atan (forward) and tan (inverse); no math library's are the same on the device and the host, so the library states its own
 *   in + - * /, comparisons and literal constants (pmv_atan, pmv_tan in csrc/pmv_lift.h; derived by scripts/derive_atan_tan.py):
 *     pmv_atan on [0, inf): the argument goes to |t| <= 7/16 by atan x = atan c + atan((x - c) / (1 + c x)), c = 0.5, 1, 1.5 (breakpoints
 *       7/16, 11/16, 19/16) and atan x = pi/2 - atan(1 / x) from 39/16; there atan t = t - t (z A(z)), z = t t, A of degree 13.
 *     pmv_tan on [0, pi/2], pi/2 the double 0x1.921fb54442d18p+0: up to pi/4 tan x = x + x (z T(z)), z = x x, T of degree 16; beyond pi/4
 *       the reciprocal of the tangent of the complement, the complement formed with a two-part pi/2.
 *   Both are within 2^-40 of the true function, relative, over the whole domain (tests/test_fisheye_twin.py holds them to that against
 *   mpmath at 50 digits; the measured maxima, far smaller, are in DESIGN.md section 4), so the float results are those of an exact atan /
 *   tan in all but about one case in 10^5.
 * Forward (pmv_project_points; cv::fisheye::projectPoints without rvec / tvec, skew 0), PI_2 = 0x1.921fb54442d18p+0:
 *     a = X / Z;  b = Y / Z;  r2 = a*a + b*b;  r = sqrt(r2);  t = pmv_atan(r)
 *     t2 = t*t;  t4 = t2*t2;  t6 = t4*t2;  t8 = t4*t4
 *     td = t * (1 + k1*t2 + k2*t4 + k3*t6 + k4*t8)          (sums left to right)
 *     s  = r > 1e-8 ? td / r : 1.0
 *     u  = fx*(a*s) + cx;  v = fy*(b*s) + cy
 *   out_ok and the refusal (0, 0) are pmv_project_points' own - X, Y, Z finite, Z > 0, u and v finite before and after their rounding to
 *   float and within 1e6 - and in addition r must be finite.
 * Inverse (pmv_undistort_points; cv::fisheye::undistortPoints without R / P):
 *     px = ((double)u - cx) * ifx;  py = ((double)v - cy) * ify
 *     td = sqrt(px*px + py*py);  if (td > PI_2) td = PI_2
 *     if (td > 1e-8):
 *         t = td;  converged = false
 *         repeat at most 10 times:
 *             t2 .. t8 as above
 *             fix = (t*(1 + k1*t2 + k2*t4 + k3*t6 + k4*t8) - td) / (1 + 3*k1*t2 + 5*k2*t4 + 7*k3*t6 + 9*k4*t8)
 *             t = t - fix
 *             if (fabs(fix) < 1e-8) { converged = true; break }
 *         good = converged && t >= 0 && t <= PI_2
 *         s = pmv_tan(t) / td                                 (evaluated only when good)
 *     else: s = 1.0, good = true
 *     x = px*s;  y = py*s
 *   out_ok = good and x, y finite, and still finite after rounding to float; a refused point is (0, 0) and no NaN is ever written.
 *   Differences from OpenCV: a point that did not converge, or whose angle left [0, pi/2], is refused with ok = 0 and (0, 0) - it is not
 *   returned as a sentinel, and a negative angle is not mirrored; skew is not taken. Parity with a real OpenCV is unpinned, as for the
 *   radial-tangential lift. The device equals the CPU restatement tests/twin/fisheye_twin.cpp bit for bit.
 * pmv_fisheye_map_build is cv::fisheye::initUndistortRectifyMap(K, k, R, newK, Size(w, h), CV_32FC1) on the host, in the shape of
 *   pmv_undistort_map_build: (X, Y, W) = (newK R)^-1 (j, i, 1) by adjugate and determinant, then the forward statement above on (X, Y, W)
 *   with K's fx, fy, cx, cy (the same function the kernels run, compiled for the host). A pixel the statement refuses gets (-1, -1), which
 *   is the border under pmv_frames_remap. The maps go to pmv_remap_map_create and through it to pmv_frames_remap,
 *   pmv_batch_frame_upload_remap and pmv_set_frame_preproc.
 * Errors (nothing is written): pmv_camera_create_fisheye - those of pmv_camera_create: PMV_ERR_INVALID for a null argument, fx or fy zero
 *   or not finite, any parameter not finite (the message names it, k[2]); PMV_ERR_CAPACITY for a 17th camera of either model.
 *   pmv_fisheye_map_build - PMV_ERR_INVALID for a null K9, k4, map_x or map_y, a singular newK R, w or h < 1.
 * Out of scope: skew; the R / P arguments of cv::fisheye::undistortPoints; a Jacobian output; the session form (pmv_batch_*); the
 *   omnidirectional (Mei) model. */
typedef struct pmv_fisheye_params {
    double fx, fy, cx, cy;
    double k[4];            /* k1, k2, k3, k4 of theta_d = theta (1 + k1 theta^2 + k2 theta^4 + k3 theta^6 + k4 theta^8) */
} pmv_fisheye_params;
int pmv_camera_create_fisheye(pmv_ctx* ctx, const pmv_fisheye_params* p, int* out_id);
int pmv_fisheye_map_build(const double* K9, const double* k4, const double* R9_or_null, const double* newK9_or_null, int w, int h, float* map_x,
                          float* map_y);

/* ---- feature extraction ------------------------------------------------------------------------ */
/* cells: n_cells * 4 ints (x0, y0, w, h), each <= 255x255, sub-views of the frame in `slot`.
 * out_xy: n_cells * max_per_cell * 2 ints, CELL-LOCAL (x, y) in descending-response order as OpenCV returns them;
 * out_count: n_cells ints. max_per_cell <= 0 means "no limit" as in cv::goodFeaturesToTrack: out_xy must then hold
 * n_cells * PMV_GFTT_UNLIMITED_CAP * 2 ints (cell stride PMV_GFTT_UNLIMITED_CAP corners); a cell with more corners than that
 * returns PMV_ERR_OVERFLOW. Status bits of one call never leak into the next. */
#define PMV_GFTT_UNLIMITED_CAP 4096
int pmv_detect_gftt(pmv_ctx* ctx, int slot, const int* cells, int n_cells, int max_per_cell, double quality,
                    double min_dist, int* out_xy, int* out_count);
/* cv::goodFeaturesToTrack with the caller's remaining arguments: mask, blockSize, useHarrisDetector, k. pmv_detect_gftt is this call
 * frozen at the reference's `cv::Mat(), 3, 3, false, 0.04` (OpenCVGoodFeatureExtractor.cpp:7); a KLT loop that refills its tracks calls
 * the detector with a mask that keeps new corners away from the tracks it has, often with a larger block or the Harris response.
 *   Cells, outputs and limits: exactly those of pmv_detect_gftt - sub-views of the frame in `slot`, at most 255x255 and at least 3x3,
 *     cell-local coordinates in cv's order, max_per_cell <= 0 = no limit with PMV_GFTT_UNLIMITED_CAP and PMV_ERR_OVERFLOW.
 *   mask: NULL = no mask. Otherwise host memory of the size of the slot's level-0 frame, mask_stride bytes per row; a non-zero byte
 *     allows the pixel. A cell sees the sub-view of the mask at its own rectangle: what cv::goodFeaturesToTrack(cell, ..., mask(cellRect),
 *     ...) sees. The mask cannot be applied afterwards: the quality threshold is quality x the maximum over the ALLOWED pixels (a cell
 *     without one has maximum 0 and returns nothing), the 3x3 non-maximum test still looks at every neighbour, masked-out ones included,
 *     and a pixel becomes a corner candidate only if its own byte is non-zero.
 *   block_size: the un-normalised block_size x block_size box over cov = (dx^2, dx dy, dy^2), anchor block_size / 2 (offsets -b/2 ..
 *     b-1-b/2: an even size leans to the upper left), REFLECT_101 on the CELL as often as needed; Sobel 3x3 with the scale
 *     1 / (4 block_size 255), its border the parent frame's as in pmv_detect_gftt.
 *   use_harris: the response is (float)(a c - b b - k (a + c)(a + c)) over the un-halved sums instead of the smaller eigenvalue. With
 *     quality in (0, 1] only responses above 0 can be selected, so a cell whose Harris response is nowhere positive returns nothing.
 *   Defaults: {q, d, 3, 0, any k} with a NULL mask returns the bytes of pmv_detect_gftt(q, d) and runs the tuned kernels (k_gftt_cand);
 *     everything else runs k_gftt_cand_general. Both feed the same k_gftt_pick, under the same two profiling classes.
 *   [mem: OpenCV 3.4 cornerEigenValsVecs, calcMinEigenVal, calcHarris, goodFeaturesToTrack; parity unpinned like the rest of the
 *   detector - tests/twin/gftt_twin.cpp is the CPU restatement that fixes the arithmetic, bit for bit.]
 * Errors (nothing is written on any of them): PMV_ERR_INVALID - null p or null outputs, block_size outside 1..15, quality outside (0, 1]
 *   or not finite, min_dist negative or not finite, k not finite while use_harris is set; PMV_ERR_CAPACITY - mask_stride below the frame
 *   width while a mask is given (as for the upload strides); the cell and slot errors of pmv_detect_gftt.
 * The device buffers of the mask are made by the first extended call with a mask on a context: the host packs the cells' mask sub-views
 *   tightly into pinned memory, so only the bytes under the cells cross the bus.
 * Out of scope: the Sobel aperture (gradientSize) stays 3. Corner sub-pixel refinement (cv::cornerSubPix) is pmv_corner_subpix below. */
typedef struct pmv_gftt_params {
    double quality;      /* qualityLevel, 0 < quality <= 1 */
    double min_dist;     /* minDistance, as pmv_detect_gftt */
    int    block_size;   /* blockSize, 1 .. 15; default 3 */
    int    use_harris;   /* useHarrisDetector */
    double k;            /* Harris k, finite; ignored without use_harris */
} pmv_gftt_params;
int pmv_detect_gftt_ex(pmv_ctx* ctx, int slot, const int* cells, int n_cells, int max_per_cell, const pmv_gftt_params* p, const uint8_t* mask,
                       int mask_stride, int* out_xy, int* out_count);
/* Debug/parity: the float32 response map of one cell for p's block_size, use_harris and k (quality and min_dist are checked, not used). */
int pmv_debug_gftt_response_ex(pmv_ctx* ctx, int slot, const int* cell, const pmv_gftt_params* p, float* out);
/* diagnostic: on != 0 sends the default arguments of pmv_detect_gftt_ex (block 3, no Harris, no mask) through the general kernels as
 * well, single and session calls alike, so that a test can compare the two code paths. It changes no result. */
int pmv_debug_gftt_general(pmv_ctx* ctx, int on);
/* cv::goodFeaturesToTrack(frame(roi), corners, max_corners, p->quality, p->min_dist, mask(roi), p->block_size, p->use_harris, p->k) on
 * level 0 of `slot`, for ONE region of any size up to the frame: what a KLT loop calls once per frame to refill its tracks. It is not the
 * union of per-cell calls: the quality threshold is quality x the maximum over the whole allowed region, the order and the max_corners cut
 * are global, and min_dist acts across what would be cell borders.
 *   roi4_or_null: (x0, y0, w, h), at least 3x3 and inside the frame; NULL = the whole frame.
 *   Arithmetic: exactly that of pmv_detect_gftt_ex with the region as its cell (see there) - the Sobel border is the parent frame's, the
 *     box border REFLECT_101 of the region, the maximum is taken over the allowed pixels, the 3x3 test runs on the raw response and looks at
 *     masked-out neighbours too, threshold (float)(max * quality), order (value, address) descending, greedy min_dist. The yardstick is the
 *     bytes of gftt_twin_cell (tests/twin/gftt_twin.cpp) with the region as its cell.
 *   mask: as for pmv_detect_gftt_ex - NULL, or host memory of the frame's size, mask_stride bytes per row, non-zero = allowed; the region
 *     sees its own rectangle. Only the bytes under the region cross the bus, packed tight into pinned memory.
 *   out_xy: out_cap * 2 ints, REGION-LOCAL (x, y) in cv's order; *out_count: the number of corners written.
 *   cap = max_corners > 0 ? max_corners : out_cap must satisfy 1 <= cap <= min(out_cap, PMV_GFTT_FRAME_MAX_CORNERS).
 *   No limit: max_corners <= 0 is cv's "no limit"; if more than out_cap corners would be selected the call returns PMV_ERR_OVERFLOW and
 *     writes nothing. Status bits of one call never leak into the next.
 *   Kernels: pass 1 is the per-tile work of k_gftt_cand - for (3, no Harris, no mask) unless pmv_debug_gftt_general is on - or of
 *     k_gftt_cand_general, over ceil(h / 32) x ceil(w / 32) tiles; pass 2 (k_gftt_pick_frame) makes the selection over the frame's records in
 *     one launch: up to PMV_GFTT_FRAME_MAX_CORNERS records above the threshold are sorted and walked on chip, more take the same steps in
 *     HBM (exact, slower). Both are booked under the profiling classes of pmv_detect_gftt (k_gftt_cand, k_gftt_pick).
 * Errors (nothing is written and nothing is clamped on any of them): the parameter errors of pmv_detect_gftt_ex with the same codes
 *   (PMV_ERR_INVALID: null p or null outputs, block_size, quality, min_dist, k; PMV_ERR_CAPACITY: mask_stride below the frame width);
 *   PMV_ERR_INVALID - a region smaller than 3x3 or not inside the frame (the message names the region and the frame size);
 *   PMV_ERR_CAPACITY - a bad cap, a slot out of range, a frame with a side above 32767; the slot-state and bracket rules of the other
 *   detectors.
 * The device buffers are made by the first frame call on a context, sized for max_w x max_h (a flat plateau makes every pixel a record).
 * pmv_detect_gftt and pmv_detect_gftt_ex keep their 255x255 cells and every refusal: this is a new entry point, not a lifted limit.
 * Out of scope: Sobel apertures other than 3; more than PMV_GFTT_FRAME_MAX_CORNERS corners; the whole-sequence drivers (pmv_pipeline_run*)
 *   and bench.py do not call this. Building the keep-away mask on the device from a track list (cv::circle's rasterisation) is
 *   pmv_detect_gftt_refill below. */
#define PMV_GFTT_FRAME_MAX_CORNERS 16384
int pmv_detect_gftt_frame(pmv_ctx* ctx, int slot, const int* roi4_or_null, int max_corners, const pmv_gftt_params* p,
                          const uint8_t* mask, int mask_stride, int* out_xy, int out_cap, int* out_count);
/* diagnostic: out6 = {frame calls served by the single entry point, session rounds that held at least one frame request, launch pairs
 * made for those rounds, records above the threshold in the last request served, of those the number kept off-chip, on-chip record
 * capacity of the selection kernel}. */
int pmv_debug_gftt_frame_stats(pmv_ctx* ctx, long long* out6);
/* The refill of a KLT loop in one call: FeatureTracker::setMask on the caller's tracks, then pmv_detect_gftt_frame with that mask. The
 * tracks are sorted, walked and thinned, the keep-away mask is painted in HBM and the detector reads it there: no w x h buffer is written
 * by the host or crosses the bus (unless the caller has a base mask of its own), and there is one wait.
 *   track_xy: n_tracks (x, y) float pairs, frame coordinates. The integer position of a track is (cvRound(x), cvRound(y)), round half to
 *     even, as cv's Point2f -> Point conversion.
 *   Order: priority descending, then index ascending - one of the orders setMask's std::sort may give among equal priorities.
 *     track_prio_or_null: any int32 per track (a track's age); NULL = all equal, the caller's order.
 *   Walk: track i is kept (out_keep[i] = 1, else 0) when the mask byte at its position is 255 - the base byte, exactly as setMask tests
 *     `== 255`; 255 everywhere without a base mask - and its position lies in no disc of a track kept earlier in the order.
 *   Disc: a kept track clears cv::circle(mask, pt, radius, 0, -1): the Circle() loop of OpenCV 3.4 (fill, LINE_8, shift 0), clipped to the
 *     frame; radius 0 is the centre pixel. It is NOT x^2 + y^2 <= r^2 by definition: the kernels test |dy| <= radius and |dx| <= hw[|dy|],
 *     hw = the widest span of that loop per row offset, computed on the host.
 *   Final mask: 0 inside any kept disc, else the base byte (255 without a base mask).
 *   out_keep depends on the track geometry and on the base bytes under the n positions only, not on the region: a track outside the
 *     region still suppresses tracks inside it. Only painting and detection are restricted to the region.
 *   Detection: exactly pmv_detect_gftt_frame with that mask (non-zero = allowed) - the same roi4_or_null, max_corners, p, out_xy, out_cap
 *     and out_count, region rule, cap rule, overflow rule and bytes. The yardstick is refill_twin_mask (tests/twin/refill_twin.cpp) for
 *     out_keep and the mask, and gftt_twin_cell with that mask and the region as its cell for the corners.
 *   base_mask_or_null: host memory of the frame's size, base_stride bytes per row. The host reads the n bytes under the tracks (n flag
 *     bytes go to the device) and packs the region's sub-view as pmv_detect_gftt_frame packs its mask. Without one nothing of the
 *     region's size is allocated in pinned memory, written by the host or copied.
 *   Kernels: k_track_select (one workgroup: keys and positions in LDS, the sorting network and the chunked walk of k_gftt_pick_frame),
 *     k_track_paint (every dword of the packed mask written once by its owner), then the general pass 1 and pass 2 of
 *     pmv_detect_gftt_frame; booked under k_gftt_pick and k_gftt_cand.
 * Errors (nothing is written and nothing is clamped on any of them): every refusal of pmv_detect_gftt_frame, with the same codes and in
 *   the same order (base_mask_or_null and base_stride in the place of mask and mask_stride); then
 *   PMV_ERR_INVALID - null out_keep, or null track_xy with n_tracks > 0; radius outside 0..PMV_REFILL_MAX_RADIUS; a coordinate that is
 *     not finite or beyond 1e6; a track whose rounded position lies outside the frame (cv reads out of bounds there; the message names the
 *     point and the frame size);
 *   PMV_ERR_CAPACITY - n_tracks < 0 or above min(max_tracks, PMV_REFILL_MAX_TRACKS).
 *   n_tracks == 0 is legal: the mask is the base mask, or all 255.
 * The buffers are made by the first refill call on a context. The call is not logged by pmv_record_enable.
 * Out of scope: non-filled or anti-aliased circles; a per-track radius; returning the mask outside pmv_debug_refill_mask; feeding the
 *   kept tracks onward on the device (that is pmv_klt_step below, which runs these kernels inside its chain); the whole-sequence drivers (pmv_pipeline_run*) and bench.py do not call this. */
#define PMV_REFILL_MAX_TRACKS 8192
#define PMV_REFILL_MAX_RADIUS 255
int pmv_detect_gftt_refill(pmv_ctx* ctx, int slot, const int* roi4_or_null, int max_corners, const pmv_gftt_params* p,
                           const float* track_xy, const int* track_prio_or_null, int n_tracks, int radius,
                           const uint8_t* base_mask_or_null, int base_stride,
                           uint8_t* out_keep, int* out_xy, int out_cap, int* out_count);
/* diagnostic: the packed mask of the region of the last pmv_detect_gftt_refill call on this context (not a session call), *w x *h tight
 * bytes into out (cap bytes; PMV_ERR_CAPACITY if too small, PMV_ERR_INVALID before the first refill call). */
int pmv_debug_refill_mask(pmv_ctx* ctx, uint8_t* out, long long cap, int* w, int* h);
/* diagnostic: out4 = {single refill calls, session rounds that held at least one refill request, select + paint launch pairs made for
 * those rounds, bytes of mask copied host -> device by refill calls since the context was created (0 unless a base mask was given)}. */
int pmv_debug_refill_stats(pmv_ctx* ctx, long long* out4);
/* Same geometry; out_score: n_cells * max_per_cell doubles (the reference fills Feature::score). max_per_cell <= 0 returns no
 * features (ShiTomasiFeatureExtractor.cpp:37-44). */
int pmv_detect_shitomasi(pmv_ctx* ctx, int slot, const int* cells, int n_cells, int max_per_cell, double quality,
                         int* out_xy, double* out_score, int* out_count);
/* Debug/parity: response map of one cell (GFTT: float32 min-eigenvalue map before thresholding). */
int pmv_debug_gftt_response(pmv_ctx* ctx, int slot, const int* cell, float* out);
int pmv_debug_shitomasi_response(pmv_ctx* ctx, int slot, const int* cell, double* out);

/* cv::cornerSubPix(level 0 of `slot`, corners, Size(win_w, win_h), Size(zero_w, zero_h), criteria): the step between pmv_detect_gftt[_ex],
 * which returns integer pixel corners, and pmv_lk_track*, which takes float positions - so that a KLT front end of the caller's own
 * (goodFeaturesToTrack -> cornerSubPix -> calcOpticalFlowPyrLK) never needs the frame in host memory. The reference itself never refines
 * (OpenCVGoodFeatureExtractor.cpp:7 hands integer corners on); the whole-sequence drivers do not call this.
 *   xy: n * 2 floats, in/out, FRAME coordinates of level 0 (the detectors return cell-local corners: add the cell origin). The call works
 *     on the whole frame; points may lie anywhere within the coordinate limit, outside the frame too (they take the general sampling path).
 *   Weight table: mask[i][j] = (float)(vy * expf(-x*x)) with x = (float)(j - win_w) / win_w and vy = expf(-y*y), y formed likewise from i and
 *     win_h. The zero zone is cleared only when zero_w >= 0 && zero_h >= 0 && 2 zero_w + 1 < 2 win_w + 1 && 2 zero_h + 1 < 2 win_h + 1;
 *     otherwise it is ignored and is not an error. The table is computed on the HOST with libm and handed to the kernel (a device expf does
 *     not have libm's bits).
 *   Patch, per iteration: getRectSubPix(src, (2 win_w + 3) x (2 win_h + 3), cI) from 8-bit to float, with both of cv's paths. ip =
 *     floor(cI - (win + 1)). Interior fast path, when 0 <= ip.x && ip.x + W < cols && 0 <= ip.y && ip.y + H < rows: a = max(a, 0.0001f),
 *     a12 = a (1 - b), a22 = a b, b1 = 1 - b, b2 = b, and along a row dst[j] = prev + t with t = a12 src[j+1] + a22 src[j+1+step] and the
 *     running prev = (float)(t * s), s = (1. - a) / a in double, starting from prev = (1 - a)(b1 src[0] + b2 src[step]); element j needs
 *     only t[j] and t[j-1]. General path otherwise: the four float weights a11..a22 (a not floored), added left to right, rows and columns
 *     with replicated borders; where both sample columns clamp to the same column (x0 < 0 or x0 >= cols - 1) the two-weight form
 *     src*b1 + src2*b2 applies. Level 0 of a slot is stored with a 64-pixel REFLECT_101 frame: the kernel does NOT sample it,
 *     out-of-image samples are replicate-clamped to the real w x h image.
 *   Normal equations: tgx, tgy are float differences of patch neighbours; gxx = tgx*tgx*m, gxy = tgx*tgy*m, gyy = tgy*tgy*m in double; the
 *     sums a, b, c, bb1, bb2 in double; stop without an update when fabs(det) <= DBL_EPSILON^2; otherwise cI2 = (float)(cI + ...) with
 *     scale = 1.0 / det, and err is the squared float step; stop when the new cI lies outside [0, cols) x [0, rows); loop
 *     while (++iter < max_iter && err > eps*eps), eps squared and compared in double. Afterwards the point returns to its input when
 *     |cI.x - cT.x| > win_w or |cI.y - cT.y| > win_h.
 *   Order of the five double sums: a wavefront cannot add in cv's raster order. ONE order is fixed, by tests/twin/subpix_twin.cpp, and the
 *     kernel follows it: lane l of 64 adds the window pixels k = l, l + 64, l + 128, ... (k = i (2 win_w + 1) + j, rows outer) in ascending
 *     k into accumulators that start at +0.0, then the 64 lane values are added as a binary tree of neighbours ((0,1), (2,3), ..., then
 *     pairs of pairs, up to the two halves). The order does not depend on n, on the point's position in the launch, or on single versus
 *     session form; the two orders differ by double rounding noise before the one rounding to float of an update.
 *   out_iters (n bytes, may be NULL): the number of position updates made, 0..100.
 *   out_flags (n bytes, may be NULL): bit 1 = stopped on the determinant test; 2 = left the frame; 4 = the iteration cap ended the loop with
 *     err > eps^2; 8 = reverted to the input position.
 *   Frames are at least 40x40 and win <= 15, so cv's own assertion cols >= 2 win_w + 5 (rows likewise) cannot fire.
 *   [mem: OpenCV 3.4 cornersubpix.cpp, samplers.cpp; parity unpinned like the rest of the front end - tests/twin/subpix_twin.cpp is the
 *   CPU restatement that fixes the arithmetic, bit for bit.]
 * Errors (nothing is written on any of them): PMV_ERR_INVALID - a null p, a null xy with n != 0, win_w or win_h outside 1..15, max_iter
 *   outside 1..100 (nothing is clamped, as for pmv_set_lk_params), eps negative or not finite, a coordinate that is not finite or beyond
 *   1e6 in magnitude (the message names the point, as for pmv_lk_track_ex); PMV_ERR_CAPACITY - n above max_tracks; the slot errors of
 *   pmv_lk_track. n == 0 is PMV_OK and launches nothing.
 * The device buffers are made by the first call on a context. Out of scope: ROI sub-views as the image, windows above 15, refinement on
 *   the levels above 0. */
typedef struct pmv_subpix_params {
    int win_w, win_h;     /* cv's `winSize` HALF sizes: the search window is (2 win_w + 1) x (2 win_h + 1); 1 .. 15 each */
    int zero_w, zero_h;   /* cv's `zeroZone` half sizes; (-1, -1) = none */
    int max_iter;         /* TermCriteria COUNT, 1 .. 100 (cv clamps to that range; a caller without COUNT passes 100) */
    double eps;           /* TermCriteria EPS, >= 0 and finite (compared squared, in double; no EPS criterion = 0) */
} pmv_subpix_params;
int pmv_corner_subpix(pmv_ctx* ctx, int slot, float* xy, int n, const pmv_subpix_params* p, uint8_t* out_iters, uint8_t* out_flags);
/* diagnostic: {launches of pmv_corner_subpix, session rounds that held at least one pmv_batch_corner_subpix request, launches made for
 * them} since the context was created. */
int pmv_debug_subpix_launches(pmv_ctx* ctx, long long* out3);

/* cv::FAST(cell, kp, threshold, nonmax) (OpenCVFASTFeatureExtractor.cpp:8; 9_16 pattern) on sub-views of the frame in `slot`; a
 * "cell" here may be as large as the frame (kNNFeatureMatcher.cpp:11 calls the extractor on the whole next frame). out_xy:
 * n_cells * max_per_cell * 2 ints, cell-local (x, y) in cv::FAST's raster order, first max_per_cell kept as the adapter does
 * (:10-18; max_per_cell <= 0 keeps nothing); out_response: n_cells * max_per_cell floats (the keypoint response = corner score,
 * 0 without non-maximum suppression). */
int pmv_detect_fast(pmv_ctx* ctx, int slot, const int* cells, int n_cells, int max_per_cell, int threshold, int nonmax, int* out_xy,
                    float* out_response, int* out_count);

/* ---- feature matching ----------------------------------------------------------------------------- */
/* The arithmetic of kNNFeatureMatcher::matchFeatures (kNNFeatureMatcher.cpp:13-31): for each of the n source features (x, y in
 * src_slot's frame) the n_neighbours nearest of the m candidates (x, y in cmp_slot's frame; getNearestNeighbors :63-101 incl. its
 * repeat-the-last-pick and default-(0,0) quirks) are compared through compareFeatures' pixel window (:103-122) and the best fit is
 * chosen by the sequential `_err < err || err == 0` rule. out_best: n indices into the candidates (-1 = the default Feature at
 * (0,0)); out_err: n floats. Thresholding, displacement statistics and the maps stay in the caller's adapter (:32-60).
 * The reference's constants: n_neighbours 7, window 15. Source and candidate coordinates may lie outside the frame: a pixel is read
 * only where both ends of a pair are inside both images (the reference skips the others, :109-112), so such a call is defined. */
int pmv_knn_match(pmv_ctx* ctx, int src_slot, int cmp_slot, const int* src_xy, int n, const int* cmp_xy, int m, int n_neighbours, int window,
                  int* out_best, float* out_err);
/* Pyramidal LK from frame slot `prev_slot` to `next_slot`. prev_xy: n*2 floats. out_xy n*2 floats,
 * out_status n bytes, out_err n floats (exactly the three outputs of cv::calcOpticalFlowPyrLK). */
int pmv_lk_track(pmv_ctx* ctx, int prev_slot, int next_slot, const float* prev_xy, int n, float* out_xy,
                 uint8_t* out_status, float* out_err);
/* The caller's cv::calcOpticalFlowPyrLK arguments (OpenCVLucasKanadeFM.h:9-10 `win_size`, `pyr_size`; OpenCV's own defaults are winSize
 * 21x21, maxLevel 3). A context setting like pmv_set_frame_format and pmv_set_ba_mode: no argument list changes, and a context that never
 * calls the setter tracks with the reference's Size(32,32), 4, {COUNT+EPS, 30, 0.01}, 1e-4 through the kernels built for them.
 *   What it governs:
 *     Pyramid depth, on every route that builds a pyramid from then on (pmv_frame_upload[_bgr], pmv_frames_stage / pmv_frames_build, the
 *       pmv_frames_stream_begin bracket, both batched runs, pmv_batch_frame_upload): cv::buildOpticalFlowPyramid's rule - after level k is
 *       kept, stop if level k + 1 would be <= win in either dimension; never beyond max_level. pmv_frame_num_levels reports the result.
 *     LK arithmetic of pmv_lk_track, pmv_batch_lk_track and the LK matcher inside pmv_pipeline_run, _run_streamed, _run_batch and
 *       _run_batch_streamed: half = (win - 1) / 2, the window tests, minEig / (2 win^2), err / (32 win^2), the iteration cap, eps^2 (compared
 *       in double with dx^2 + dy^2) and min_eig. Bit-exact against the CPU restatement for every accepted value. win = 32 runs the tuned
 *       kernels (k_lk, k_lk_batch), any other window the general ones (k_lk_general, k_lk_batch_general: same profiling class).
 *   Accepted ranges (anything else is PMV_ERR_INVALID, the setting stays as it was, nothing is clamped):
 *     3 <= win <= 63         the template tile reads one pixel beyond the window: with PMV_PYR_PAD = 64 a window of 63 stays inside the frame
 *     0 <= max_level <= 4    a pyramid has at most 5 levels (the 8-int record of pmv_batch_upload_rounds keeps its meaning)
 *     1 <= max_iter <= 100, 0 <= eps <= 10      cv::calcOpticalFlowPyrLK's own clamps [mem: lkpyramid.cpp]
 *     min_eig >= 0 and finite
 *   Refused (PMV_ERR_INVALID, the setting stays as it was) while a pmv_frames_stream_begin bracket, a batched run or a batch session is open
 *     on the context. Sessions: set the parameters before pmv_batch_open; all callers of a session share them.
 *   Frame slots: a call that changes win or max_level EMPTIES EVERY FRAME SLOT - the slots are what they were after pmv_ctx_create, their
 *     contents are lost, and their storage is laid out again (and reallocated if the new depth needs more room). pmv_lk_track and every
 *     other reader then fail on such a slot as on a slot that was never uploaded, until it is uploaded again. A call that changes only
 *     max_iter, eps or min_eig leaves the slots alone.
 *   Frame sizes: 40x40 .. max_w x max_h as before. Level 0 may be narrower than the window and upper levels narrower than the 64-pixel
 *     border (a 10x8 level at win = 5): the border is REFLECT_101 applied as often as needed.
 *   pmv_lk_counters: the general kernels count at most 255 iterations per track (the tuned ones cannot reach that).
 *   Out of scope: non-square windows. OPTFLOW_USE_INITIAL_FLOW and OPTFLOW_LK_GET_MIN_EIGENVALS are no context settings: they are the
 *     per-call `flags` argument of pmv_lk_track_ex (below), as in cv. */
typedef struct pmv_lk_params {
    int win;          /* square window side, cv::Size(win, win); default 32 */
    int max_level;    /* maxLevel of buildOpticalFlowPyramid / calcOpticalFlowPyrLK; default 4 */
    int max_iter;     /* TermCriteria COUNT; default 30 */
    double eps;       /* TermCriteria EPS (the kernel compares dx^2 + dy^2 with eps^2); default 0.01 */
    float min_eig;    /* minEigThreshold; default 1e-4f */
} pmv_lk_params;
int pmv_set_lk_params(pmv_ctx* ctx, const pmv_lk_params* p);
int pmv_get_lk_params(pmv_ctx* ctx, pmv_lk_params* out);
/* cv::calcOpticalFlowPyrLK with its `flags` argument (cv's values). Window, depth, criteria and minEigThreshold come from the context
 * (pmv_set_lk_params) as for pmv_lk_track; the flags are per call.
 *   next_xy: n*2 floats, in/out. With PMV_LK_USE_INITIAL_FLOW the top level's search of point i starts at next_xy[i] * 2^-level instead of
 *     prev_xy[i] * 2^-level; next_xy is read, then overwritten with the result. Without the flag it is output only. A guess may lie anywhere,
 *     outside the frame too (the point then ends with status 0 like a point that walks out of the frame).
 *   PMV_LK_GET_MIN_EIGENVALS: out_err[i] = the smaller eigenvalue of the point's 2x2 normal matrix divided by 2 win^2 - the value the
 *     minEigThreshold test looks at - instead of the L1 residual. It is stored at every level whose template window passes the bounds
 *     test, before the threshold test, and the final residual is not computed: out_err is level 0's value for every point whose level-0
 *     template is in range, points that end with status 0 included, and 0 otherwise. Positions and status are those of the call without
 *     the flag.
 *   flags = 0: the bytes of pmv_lk_track in all three outputs. An initial flow equal to prev_xy: the same bytes again.
 *   [mem: OpenCV 3.4 lkpyramid.cpp; parity unpinned like the rest of LK - tests/twin/lkx_twin.cpp is the CPU restatement that fixes it.]
 * Errors (nothing is written on any of them): PMV_ERR_INVALID - a null pointer, flag bits other than the two, with
 *   PMV_LK_USE_INITIAL_FLOW an initial coordinate that is not finite or beyond 1e6 in magnitude (the message names the point);
 *   PMV_ERR_CAPACITY - n above max_tracks; the slot errors of pmv_lk_track.
 * The device buffers of the extra inputs and outputs are made by the first extended call on a context. pmv_lk_counters: as pmv_lk_track
 * (a track counts once, at most 255 iterations per track). The launches run under the LK profiling class. */
enum { PMV_LK_USE_INITIAL_FLOW = 4, PMV_LK_GET_MIN_EIGENVALS = 8 };
int pmv_lk_track_ex(pmv_ctx* ctx, int prev_slot, int next_slot, const float* prev_xy, int n, float* next_xy /* in/out */, int flags,
                    uint8_t* out_status, float* out_err);
/* Forward-backward check (the outlier filter of a KLT front end) in ONE launch: the workgroup that tracked a point forward tracks the
 * result back into the first frame. Defined as a composition, bit for bit:
 *   1. forward: pmv_lk_track_ex(prev_slot, next_slot, prev_xy, next_xy, flags);
 *   2. backward, for the tracks with forward status 1: pmv_lk_track_ex(next_slot, prev_slot, points = the forward result, initial flow =
 *      prev_xy, flags = PMV_LK_USE_INITIAL_FLOW | (flags & PMV_LK_GET_MIN_EIGENVALS)) -> back_xy, back_status, back_err;
 *   3. a track whose forward status is 0 runs no backward pass: back_status 0, back_err 0, back_xy = the bits of its forward next_xy.
 * The library does not threshold |back_xy - prev_xy|: that is the caller's policy. Errors: those of pmv_lk_track_ex; the three back
 * outputs must not be null. pmv_lk_counters adds the iterations (saturating at 255 per track) and (track, level) passes of both directions;
 * a track counts once. */
int pmv_lk_track_fb(pmv_ctx* ctx, int prev_slot, int next_slot, const float* prev_xy, int n, float* next_xy /* in/out */, int flags,
                    uint8_t* out_status, float* out_err, float* back_xy, uint8_t* back_status, float* back_err);
/* cv's maxLevel as a per-call argument on pyramids that are already built: pmv_lk_track_fb, except that the forward pass starts at level
 * min(fwd_top_level, L - 1) and the backward pass at level min(back_top_level, L - 1), L = the slots' level count (pmv_frame_num_levels + 1).
 * Levels 0 .. top of a pyramid are the same images whatever depth was built, so a pass is cv::calcOpticalFlowPyrLK with maxLevel = min(top,
 * the context's max_level) on the same frames; max_level of pmv_set_lk_params stays the depth that is BUILT, and no slot is emptied. The use:
 * a guess that is already close (a landmark projected with pmv_project_points, a back check that starts at the known position) needs the
 * upper levels no more - VINS tracks predicted points and runs its reverse check on two levels (top = 1) instead of four.
 *   -1 means L - 1: with (-1, -1) every output holds the bytes of pmv_lk_track_fb.
 *   All three back outputs NULL: the call is forward only and returns the bytes of pmv_lk_track_ex at that level (back_top_level is
 *     checked, then ignored). One or two of them NULL: PMV_ERR_INVALID.
 *   Errors (nothing is written): those of pmv_lk_track_fb; PMV_ERR_INVALID - a level outside -1 .. 4. Nothing is clamped except by L.
 *   Device side: the same ONE launch of the extended kernels (k_lk_ex, both forms) and one wait; the level is a workgroup-uniform launch
 *     argument of the two device functions behind their EX template parameter, so k_lk, k_lk_batch and the two general plain kernels are
 *     the code they were. pmv_lk_counters counts the level passes that ran.
 *   The CPU yardstick is the existing twin, tests/twin/lkx_twin.cpp, with max_level = min(top, the context's max_level).
 *   Out of scope: the session form (pmv_batch_*), a per-track level. Inside the tracker step the levels are capped only by a pending
 *     prediction (pmv_klt_set_prediction); stereo stage 8 walks every level of the slot. */
int pmv_lk_track_fb_levels(pmv_ctx* ctx, int prev_slot, int next_slot, const float* prev_xy, int n, float* next_xy /* in/out */, int flags,
                           int fwd_top_level, int back_top_level, uint8_t* out_status, float* out_err,
                           float* back_xy_or_null, uint8_t* back_status_or_null, float* back_err_or_null);
/* diagnostic: on != 0 sends the default window (32) through the general kernels as well, so that a test can compare the two code paths.
 * It changes no result. */
int pmv_debug_lk_general(pmv_ctx* ctx, int on);

/* ---- PnP ------------------------------------------------------------------------------------------------ */
/* obj_xyz m*3 float32, img_xy m*2 float32, K 9 doubles row-major, rvec/tvec 3 doubles in/out
 * (useExtrinsicGuess=true semantics of the reference call), out_inliers: capacity m ints. */
int pmv_pnp_ransac(pmv_ctx* ctx, const float* obj_xyz, const float* img_xy, int m, const double* K, double* rvec,
                   double* tvec, int iterations, float reproj_err, double confidence, int* out_inliers,
                   int* out_n_inliers);

/* Debug/parity: models (n*6: rvec,tvec) and inlier counts of the first n hypotheses of the last pmv_pnp_ransac call. */
int pmv_debug_pnp_hypotheses(pmv_ctx* ctx, int n, double* models, int* counts);
/* diagnostic: 32 accumulated shader-clock phase timers of the back-end kernels (recorded only with PMV_BA_STAMPS=1) */
int pmv_debug_ba_stamps(pmv_ctx* ctx, unsigned long long* out32);
/* diagnostic: 16 phase timers of the LK kernel, track 0 (recorded only with PMV_LK_STAMPS=1) */
int pmv_debug_lk_stamps(pmv_ctx* ctx, unsigned long long* out16);

/* ---- bundle adjustment ------------------------------------------------------------------------------------- */
typedef struct pmv_ba_summary {
    double initial_cost, final_cost;
    int iterations;       /* LM iterations executed (successful + unsuccessful) */
    int successful_steps;
    int termination;      /* 0 = max iterations, 1 = function tol, 2 = gradient tol, 3 = parameter tol, 4 = failure */
} pmv_ba_summary;

/* Per-observation residuals (n_obs*2) and Jacobians (n_obs*2*9: d r / d cam[6], d r / d point[3]) of
 * ProjectionResidual (ProjectionResidual.h:38-58). cams nc*6 = [angle-axis(R^T), -t], pts np*3 doubles. */
int pmv_ba_residuals(pmv_ctx* ctx, const double* cams, int nc, const double* pts, int np, const double* obs_xy,
                     const int* cam_idx, const int* pt_idx, int n_obs, const double* K, double* out_r,
                     double* out_J);
/* Levenberg–Marquardt with Huber(huber_delta) loss and Schur elimination of the points; cams/pts updated in place. */
/* Which of the two LM implementations pmv_ba_solve / the pipeline's BA plugin use on this context (default 0):
 *   0  the multi-kernel launch chain: every phase of an LM iteration spread over many CUs - the shortest latency for ONE solve;
 *   1  the whole solve in one workgroup per problem: one launch per solve, and ONE launch per round of B solves in
 *      pmv_pipeline_run_batch - what a GPU shared by many sequences wants (a launch chain pays for wave slots 23 times).
 * Same algorithm, same parity bars against the CPU restatement; the floating-point sums are ordered differently, so two runs
 * are bitwise comparable only under the same mode. */
int pmv_set_ba_mode(pmv_ctx* ctx, int mode);
int pmv_ba_solve(pmv_ctx* ctx, double* cams, int nc, double* pts, int np, const double* obs_xy, const int* cam_idx,
                 const int* pt_idx, int n_obs, const double* K, double huber_delta, int max_iterations,
                 pmv_ba_summary* summary);

/* ---- five-point RANSAC round -----------------------------------------------------------------------------
 * The hypothesis half of cv::findEssentialMat(p1, p2, K, RANSAC, 0.99, 1.0) (OpenCVFivePointTri.cpp:24): for n_hyp (<= 64) samples of
 * five correspondence indices each (the caller draws them from cv::RNG as RANSACPointSetRegistrator::getSubset does), Nister's
 * solver gives up to 10 essential matrices per sample (models: n_hyp x 10 x 9 doubles, n_models: n_hyp) and every model is scored
 * on all n normalised correspondences q1, q2 (x, y each) by the float32 Sampson distance <= thr (counts: n_hyp x 10). The caller
 * replays the sequential bookkeeping (best so far, RANSACUpdateNumIters) in sample order. One thread per hypothesis: a latency
 * chain, slower than a host core for one sequence, useful when many sequences' rounds share a launch (pmv_pipeline_run_batch). */
int pmv_fivepoint_hypotheses(pmv_ctx* ctx, const double* q1, const double* q2, int n, const int* samples, int n_hyp, float thr, double* models,
                             int* n_models, int* counts);

/* ---- two-view triangulation ------------------------------------------------------------------ */
/* The per-point part of cv::recoverPose(E, p1, p2, K, R, t, HUGE_VAL, mask, tri) (OpenCVFivePointTri.cpp:27): for each of
 * the four (R, t) candidates of decomposeEssentialMat, DLT-triangulate every correspondence (cv::triangulatePoints) and apply
 * the cheirality tests. q1, q2: n normalised image points (x, y) each; P1x4: four row-major 3x4 matrices [R | t];
 * mask_in: n bytes (RANSAC inlier mask of findEssentialMat). out_Q: [4][4][n] homogeneous points, out_mask: [4][n],
 * out_good: [4] number of points passing all tests. n <= max_tracks. */
int pmv_triangulate_candidates(pmv_ctx* ctx, const double* q1, const double* q2, int n, const double* P1x4,
                               const uint8_t* mask_in, double* out_Q, uint8_t* out_mask, int* out_good);
/* The same call on an auxiliary lane of the context (own workspace and stream, created on first use, one call at a time): for a
 * helper thread that evaluates cv::recoverPose of a frame pair AHEAD of the back-end thread (the candidates depend on the 2-D
 * correspondences only), concurrently with pmv_pnp_ransac / pmv_ba_solve / pmv_triangulate_candidates on the main lane. */
int pmv_triangulate_candidates_ahead(pmv_ctx* ctx, const double* q1, const double* q2, int n, const double* P1x4, const uint8_t* mask_in,
                                     double* out_Q, uint8_t* out_mask, int* out_good);

/* ---- N-view triangulation of track landmarks: the link between the tracker's observations and pmv_klt_set_prediction / pmv_ba_solve ----------
 * What FeatureManager::triangulate of a VINS-style estimator or cv::sfm::triangulatePoints does on the host: every landmark of a sliding
 * window is triangulated from ALL its observations. obs_xy (n_obs x 2), cam_idx, pt_idx and n_obs are exactly the arrays of pmv_ba_solve: a
 * caller hands the same arrays to both calls. P3x4: one general row-major projection matrix per camera, nc x 12 doubles - [R|t] for
 * normalised observations, K[R|t] for pixels; its third row must give the depth, P[2].(X,1) (so a matrix scaled by -1, or pmv_ba_solve's own
 * camera form with pz = -p[2], is not one: the Python helper projections_from_ba_cams makes the matrices of that form). out_xyz np x 3,
 * out_status np bytes (PMV_TRI_* bits, 0 = accepted), out_err_or_null np doubles (the rms reprojection error over the landmark's views, in the
 * observations' unit), *out_good = landmarks with status 0. ONE launch per call (k_tri_tracks: one lane per landmark, 64-lane workgroups),
 * one copy in, results in a mapped pinned block behind a completion word, one wait; the result has the bits of
 * tests/twin/tri_tracks_twin.cpp, the CPU restatement that fixes them.
 *   Capacities: the context's BA caps - nc <= max_ba_cams, np <= max_ba_points, n_obs <= max_ba_obs, else PMV_ERR_CAPACITY (negative np or
 *     n_obs too). np == 0 or n_obs == 0 is valid: nothing is launched, every landmark is FEW_VIEWS, *out_good = 0.
 *   Lists: a landmark's observations are taken in order of appearance in the caller's arrays (a stable counting sort on the host during
 *     stage-in); pt_idx need not be sorted; a camera may occur twice. Fewer than min_views observations: PMV_TRI_FEW_VIEWS.
 *   DLT: per observation two rows, x P[8+k] - P[k] and y P[8+k] - P[4+k] (k = 0..3); AtA (4x4) accumulated row by row in list order from 0;
 *     the eigenvector Qh of its smallest eigenvalue by the cyclic Jacobi of pmv_triangulate_candidates - the statement and the operation
 *     order of that call's kernel, so a two-observation landmark whose first camera is [I|0] has its bits; X = Qh[0..2] / Qh[3].
 *     Qh[3] == 0 or a non-finite X: PMV_TRI_DEGENERATE.
 *   Refinement (refine_iters > 0): Gauss-Newton on sum |pi(P_i X) - obs_i|^2 over the three coordinates; JtJ and Jtr accumulated in list
 *     order; the 3x3 system solved by the explicit adjugate over the determinant; a step is taken only if the new cost is strictly smaller,
 *     and the first step that is not ends the refinement (the undamped step from the same X would be the same again). A zero or non-finite
 *     determinant or a non-finite cost ends the refinement with the X it had.
 *   Gates: all evaluated, no early exit, status bits OR-ed. FEW_VIEWS and DEGENERATE short-circuit: out_xyz = 0 and out_err = +inf for them.
 *     Depth of view i is P_i[2].(X,1); it must lie in [min_depth, max_depth] in every view, else PMV_TRI_DEPTH. The reprojection error of a
 *     view is the Euclidean distance in the observations' unit; a view whose error is not <= max_reproj: PMV_TRI_REPROJ (max_reproj = +inf:
 *     no gate). Parallax: the camera centres C = -M^-1 p4 by the adjugate, computed once per call on the host and only if the gate is on (a
 *     camera with det M == 0 is then PMV_ERR_INVALID; the message names the camera); the smallest cosine over pairs i < j of
 *     (C_i - X).(C_j - X) / sqrt(|.|^2 |.|^2) must be <= cos(min_parallax_deg pi / 180) from the host's libm, else PMV_TRI_PARALLAX; a
 *     non-finite cosine counts as no parallax. The device never evaluates a transcendental function.
 *   Errors, each with its code and its message, nothing is written: null pointers (out_err_or_null and p_or_null may be null), nc < 1:
 *     PMV_ERR_INVALID; cam_idx or pt_idx out of range (the message names the observation), non-finite P or obs, min_views < 2,
 *     refine_iters outside 0..20, min_depth not finite or max_depth < min_depth, max_reproj <= 0 or NaN, min_parallax_deg outside [0, 180):
 *     PMV_ERR_INVALID. Not logged by pmv_record_enable. */
enum { PMV_TRI_OK = 0, PMV_TRI_FEW_VIEWS = 1, PMV_TRI_DEGENERATE = 2, PMV_TRI_DEPTH = 4, PMV_TRI_REPROJ = 8, PMV_TRI_PARALLAX = 16 };
typedef struct pmv_tri_params {
    int    min_views;         /* >= 2 */
    int    refine_iters;      /* 0..20 Gauss-Newton iterations on the reprojection error behind the DLT; 0 = DLT only */
    double min_depth, max_depth;   /* accepted depth in EVERY observing view; max_depth may be +inf */
    double max_reproj;        /* largest accepted reprojection error of any view, in the observations' unit; +inf = no gate */
    double min_parallax_deg;  /* the largest angle between two viewing rays at X must reach it; 0 = no gate */
} pmv_tri_params;             /* NULL = {2, 0, 0.1, +inf, +inf, 0}: VINS-Mono's triangulate with its depth test */
int pmv_triangulate_tracks(pmv_ctx* ctx, const double* P3x4, int nc, const double* obs_xy, const int* cam_idx, const int* pt_idx, int n_obs, int np,
                           const pmv_tri_params* p_or_null, double* out_xyz, uint8_t* out_status, double* out_err_or_null, int* out_good);
/* diagnostic, ctx-free: the argument rules of pmv_triangulate_tracks for a context of the given BA caps, in its order and with its codes
 * (the singular camera of the parallax gate included); reads the inputs, writes nothing but err256 (optional: the message the call would
 * leave, 256 bytes). */
int pmv_debug_tri_tracks_check(int max_cams, int max_points, int max_obs, const double* P3x4, int nc, const double* obs_xy, const int* cam_idx,
                               const int* pt_idx, int n_obs, int np, const pmv_tri_params* p_or_null, const double* out_xyz, const uint8_t* out_status,
                               const double* out_err_or_null, const int* out_good, char* err256);
/* diagnostic: out2 = {k_tri_tracks and k_tri_tracks_batch launches, requests they served} since the context was created
 * (pmv_triangulate_tracks: one each, none for an empty problem; pmv_batch_triangulate_tracks: one launch per round of the DLT combiner that
 * holds such requests). */
int pmv_debug_tri_tracks_launches(pmv_ctx* ctx, long long* out2);

/* ---- the two calls of the triangulator, whole (OpenCVFivePointTri.cpp:24-27) ------------------------------------------------------------
 * cv::findEssentialMat(points1, points2, K, RANSAC, prob, threshold, mask) (OpenCVFivePointTri.cpp:24). p1_xy, p2_xy: n pixel coordinates
 * (x, y) as doubles; K: 9 doubles, row-major; E9 row-major; mask n bytes; *out_samples_drawn = RANSAC iterations made. *out_found 0 = no
 * model (cv returns an empty Mat): E9 untouched, mask all 0. The whole adaptive RANSAC - cv::RNG((uint64)-1) sample stream, Nister's
 * solver per sample, float32 Sampson scoring, best-so-far and RANSACUpdateNumIters, at most 1000 iterations - runs in ONE launch, one
 * workgroup per call (k_essential_ransac); the result has the bits of the host code behind pmv_pipeline_run (device_fivepoint = 0).
 *   n: 0 <= n <= max_tracks, else PMV_ERR_CAPACITY. n < 5: no model (nothing is launched); n == 5: one solve without RANSAC, the first
 *   model wins, mask all 1, 0 samples drawn. Null pointers, prob outside [0, 1], a non-positive or non-finite threshold: PMV_ERR_INVALID.
 *   On an error no output is written. Not logged by pmv_record_enable. */
int pmv_find_essential_mat(pmv_ctx* ctx, const double* p1_xy, const double* p2_xy, int n, const double* K, double prob, double threshold,
                           double* E9, uint8_t* mask, int* out_found, int* out_samples_drawn);
/* cv::recoverPose(E, points1, points2, K, R, t, HUGE_VAL, mask, triangulatedPoints) (OpenCVFivePointTri.cpp:27): decomposeEssentialMat on
 * the host, the four (R, t) candidates through the DLT kernel of pmv_triangulate_candidates (logged by pmv_record_enable as that call's DLT
 * record), the candidate choice of cv::recoverPose. mask is in/out: n bytes, the inlier mask of pmv_find_essential_mat going in, the
 * winning candidate's mask coming out; R9 row-major, t3 of unit length; tri4n: 4 x n homogeneous points, row-major (row k = coordinate k
 * of every point); *out_good: the winning candidate's count. n: 0 <= n <= max_tracks, else PMV_ERR_CAPACITY; null pointers:
 * PMV_ERR_INVALID; on an error no output is written. */
int pmv_recover_pose(pmv_ctx* ctx, const double* E9, const double* p1_xy, const double* p2_xy, int n, const double* K, double* R9, double* t3,
                     uint8_t* mask, double* tri4n, int* out_good);
/* diagnostic, ctx-free: how pmv_find_essential_mat splits RANSACUpdateNumIters(prob, (n - g) / n, 5, maxIters) between host and device for a
 * call with n points. The host's libm gives *out_num = log(1 - prob) and, per inlier count g = 0..n, out_denoms[g] = log(1 - (1 - (n - g) /
 * n)^5) (n + 1 doubles; -infinity where the function returns 0 before its logarithms); the kernel evaluates only the final expression
 * `denom >= 0 || -num >= maxIters * (-denom) ? maxIters : lrint(num / denom)`. n < 0 or a null pointer: PMV_ERR_INVALID. */
int pmv_debug_essential_iters_table(int n, double prob, double* out_denoms, double* out_num);

/* ---- fundamental-matrix RANSAC: the rejectWithF of a KLT loop ------------------------------------------------------------------------------
 * cv::findFundamentalMat(points1, points2, FM_RANSAC, threshold, confidence, mask) for n >= 15 correspondences, the step of a VINS-style
 * tracker between pmv_lk_track_fb and the masked re-detection: the tracks that survive the forward-backward check but violate the epipolar
 * geometry are masked out. p1_xy, p2_xy: n pixel positions (x, y) as float32 (cv converts its input to CV_32F; the LK calls return float32, so
 * the outputs of pmv_lk_track_fb go in directly); F9 row-major; mask n bytes; *out_samples_drawn = RANSAC iterations made. *out_found 0 = no
 * model (cv returns an empty Mat): F9 untouched, mask all 0. The whole adaptive RANSAC runs in ONE launch, one workgroup per call
 * (k_fundamental_ransac); the result has the bits of tests/twin/fundamental_twin.cpp.
 * [mem: OpenCV 3.4 fundam.cpp, ptsetreg.cpp; parity with a real OpenCV unpinned like the rest - tests/twin/fundamental_twin.cpp is the CPU
 * restatement that fixes the bits]
 *   Branch by n. cv runs the RANSAC only for n >= 15; at n = 7 it returns up to three stacked matrices, for 8..14 it switches to LMedS.
 *     Neither is built (nor FM_8POINT, FM_LMEDS or a normalised eight-point refit): n < 15 is PMV_ERR_DEGENERATE and the message says why - a
 *     KLT loop with that few tracks re-detects anyway. n < 0 or n > max_tracks: PMV_ERR_CAPACITY.
 *   Sampling: RANSACPointSetRegistrator::getSubset with 7 model points. rng = cv::RNG((uint64)-1) per call; a draw is rng % n; a duplicate is
 *     redrawn without counting an attempt; a full subset goes through FMEstimatorCallback::checkSubset and is refused if haveCollinearPoints
 *     holds for either image. haveCollinearPoints has cv's quirk: only the LAST point of the subset is tested, against every pair (j, k < j)
 *     of the earlier ones, fabs(dx2*dy1 - dy2*dx1) <= FLT_EPSILON*(fabs(dx1) + fabs(dy1) + fabs(dx2) + fabs(dy2)) with the differences taken as
 *     float subtractions widened to double. Attempts per subset: 10000 - getSubset's default is 1000, but RANSACPointSetRegistrator::run passes
 *     10000, and that is followed here. No subset at iteration 0: no model, 0 samples drawn; at a later iteration: the loop ends there.
 *   Seven-point solver (run7Point): no normalisation; row i of the 7x9 system is [x2 x1, x2 y1, x2, y2 x1, y2 y1, y2, x1, y1, 1]; f1, f2 a
 *     basis of its null space; the cubic is det(lambda f1 + (1 - lambda) f2) = 0. As in cv, f1 -= f2 comes first and everything after it is
 *     written in that difference: det(lambda f1 + f2) with cv's expressions for the four coefficients; per real root s = f1[8] lambda + f2[8]; fabs(s) > DBL_EPSILON:
 *     mu = 1 / s, lambda *= mu, F[8] = 1, else mu = 1 and F[8] = 0; F[i] = f1[i] lambda + f2[i] mu for i < 8. Up to three models.
 *     Two places cannot have cv's bits on a device, the twin fixes both. The null space: cv takes it from its SVD; here Gauss-Jordan with
 *     complete pivoting on the 7x9 system, then the two vectors of the free columns normalised to unit length (the construction of the
 *     five-point solver's 5x9 case). The cubic: cv's solveCubic calls acos, cos and pow, and the device's libm is not glibc's; its case
 *     analysis is kept exactly - leading coefficients that are zero (quadratic, linear, none), then Q, R and the sign of Q^3 - R^2 - because it
 *     decides HOW MANY roots there are; their VALUES come from IEEE + - * / sqrt only: one real root inside the Cauchy bound 1 + max |a_i| by
 *     Newton's iteration kept inside a shrinking bracket (bisection where it leaves; at most 200 steps, over when the iterate no longer
 *     changes), deflation to a quadratic solved in its stable form, two Newton steps per root on the undeflated cubic (a step is taken only
 *     where |f| does not grow). Order of three roots: smallest, largest, middle, which is the order of cv's cos(t), cos(t + 2 pi / 3),
 *     cos(t + 4 pi / 3), so that "the first model that beats the best wins" breaks ties as cv does. Q^3 - R^2 == 0: cv's pow(R, 1/3) is
 *     sign(R) sqrt(Q) there.
 *   Error and inliers (FMEstimatorCallback::computeError): err = (float)max(d1^2 s1, d2^2 s2), the two squared point-to-epipolar-line
 *     distances in double from the float points; inlier iff err <= (float)(threshold * threshold). A model becomes the best iff its count >
 *     max(maxGood, 6); then niters = RANSACUpdateNumIters(confidence, (n - count) / n, 7, niters), starting from 1000, with pow and log on
 *     the host (pmv_debug_fundamental_iters_table). No refit on the inliers: cv has none for F.
 *   Errors: null pointers, a threshold that is not positive and finite, a confidence outside (0, 1) or not finite (cv silently substitutes
 *     3 and 0.99 for such values; here they are refused), a coordinate that is not finite or beyond 1e6 in magnitude (the message names the
 *     point): PMV_ERR_INVALID. On an error nothing is written and nothing is clamped. Not logged by pmv_record_enable; the whole-sequence
 *     drivers do not call this. */
int pmv_find_fundamental_mat(pmv_ctx* ctx, const float* p1_xy, const float* p2_xy, int n, double threshold, double confidence, double* F9,
                             uint8_t* mask, int* out_found, int* out_samples_drawn);
/* diagnostic, ctx-free: pmv_debug_essential_iters_table for the 7 model points of pmv_find_fundamental_mat: *out_num = log(1 - confidence),
 * out_denoms[g] = log(1 - (1 - (n - g) / n)^7) for g = 0..n (n + 1 doubles; -infinity where RANSACUpdateNumIters returns 0 before its
 * logarithms). n < 0 or a null pointer: PMV_ERR_INVALID. */
int pmv_debug_fundamental_iters_table(int n, double confidence, double* out_denoms, double* out_num);
/* diagnostic, process-wide: hypotheses per in-kernel round of k_fundamental_ransac from the next launch on, 1..64; 0 = back to PMV_FUNDAMENTAL_R
 * or the default (64). The results do not depend on it. Outside 0..64: PMV_ERR_INVALID. */
int pmv_debug_set_fundamental_r(int r);
/* diagnostic, process-wide: the round width the next k_fundamental_ransac launch takes (the setter's value, else PMV_FUNDAMENTAL_R clamped to
 * 1..64, else 64). */
int pmv_debug_fundamental_r(void);
/* diagnostic: out3 = {k_fundamental_ransac launches, k_essential_ransac launches, rounds that made both} of the five-point combiner's
 * whole-RANSAC rounds (pmv_batch_find_fundamental_mat, pmv_batch_find_essential_mat, device_fivepoint = 2) since the context was created. */
int pmv_debug_whole_rounds(pmv_ctx* ctx, long long* out3);

/* ---- homography RANSAC with cv's refit: the planar / rotation-only counterpart of E and F -----------------------------------------------------
 * cv::findHomography(points1, points2, cv::RANSAC, threshold, mask, maxIters, confidence) for n >= 4 correspondences: what a caller estimates
 * beside E or F on a planar scene or a near-pure rotation, where those are degenerate, to compare the supports. p1_xy, p2_xy: n pixel positions
 * (x, y) as float32 (cv converts its input to CV_32F; the LK calls and the KLT step return float32); H9 row-major, maps image 1 to image 2, H9[8]
 * = 1; mask n bytes; *out_samples_drawn = RANSAC iterations made. *out_found 0 = no model (cv returns an empty Mat): H9 untouched, mask all 0.
 * The adaptive RANSAC and the refit run in ONE launch, one workgroup per call (k_homography_ransac); the result has the bits of
 * tests/twin/homography_twin.cpp.
 * [mem: OpenCV 3.4 fundam.cpp, ptsetreg.cpp, lmsolver.cpp; parity with a real OpenCV unpinned like the rest - tests/twin/homography_twin.cpp is
 * the CPU restatement that fixes the bits]
 *   Branch by n. n == 4: one runKernel on the four points without RANSAC; the mask is all 1, 0 samples drawn, no refit; no model from it:
 *     found 0. n < 4 is PMV_ERR_DEGENERATE (cv asserts); n < 0 or n > max_tracks: PMV_ERR_CAPACITY. LMEDS, RHO and method 0 are not built.
 *   Sampling: RANSACPointSetRegistrator::getSubset with 4 model points, rng = cv::RNG((uint64)-1) per call, a draw is rng % n, duplicates are
 *     redrawn, up to 10000 attempts per subset. checkSubset refuses a subset if haveCollinearPoints holds for either image (only the LAST point
 *     is tested, as for pmv_find_fundamental_mat) or if the four-point orientation test fails: for the triples {0,1,2}, {0,1,3}, {0,2,3},
 *     {1,2,3} the 3x3 determinants of the homogeneous points (doubles from the floats) of image 1 and image 2 must not have opposite signs.
 *     No subset at iteration 0: no model, 0 samples drawn; at a later iteration: the loop ends there.
 *   Four-point solver (runKernel): cv's normalisation - centroids, then count / (sum of absolute deviations) per axis, no model if a sum is
 *     < DBL_EPSILON - and its two rows per point [X, Y, 1, 0, 0, 0, -xX, -xY, -x], [0, 0, 0, X, Y, 1, -yX, -yY, -y]; the null vector of the 8x9
 *     system by Gauss-Jordan with complete pivoting, normalised to unit length (cv: the least eigenvector of LtL; the twin's first fixed
 *     choice); H = invHnorm H0 Hnorm2 scaled by 1 / H[8], H[8] = 1. H[8] == 0 or not a number: the model is dropped (cv divides unguarded).
 *   Error and inliers (computeError): float32 throughout - the nine entries cast to float, ww = 1.f / (H6 x + H7 y + 1.f), err = dx dx + dy dy;
 *     inlier iff err <= (float)(threshold * threshold). A model becomes the best iff its count > max(maxGood, 3); then niters =
 *     RANSACUpdateNumIters(confidence, (n - count) / n, 4, niters), starting from max_iters, with pow and log on the host
 *     (pmv_debug_homography_iters_table).
 *   Refit (only with a model and n > 4; the mask is the RANSAC model's and is not recomputed): runKernel on the inliers - the 9x9 LtL and the
 *     eigenvector of its smallest eigenvalue by cv's JacobiImpl_, with hypot written as |a| sqrt(1 + (b / a)^2) (the twin's second fixed
 *     choice); H stays the RANSAC model where that gives none - then LMSolver with at most 10 iterations on the 8 free entries with
 *     HomographyRefineCallback's residuals and Jacobian in double, cv's damping rule (Rlo 0.25, Rhi 0.75, the lambda / nu updates,
 *     invert(A, DECOMP_EIG) at lambda == 0), the step from solve(Ap, v, d, DECOMP_EIG) by the same Jacobi routine, over at |d|inf <
 *     FLT_EPSILON or |r|inf < FLT_EPSILON. Every sum over the inliers (centroids, deviations, LtL, JtJ, Jtr, S, Sd) is taken in the twin's
 *     order, its third fixed choice: 64 partial sums, point i in partial sum i mod 64 in increasing i, then the xor butterfly 32, 16, .. 1.
 *   Errors: null pointers, a threshold that is not positive and finite (cv substitutes 3; here it is refused), a confidence outside (0, 1),
 *     max_iters outside 1..10000, a coordinate that is not finite or beyond 1e6 in magnitude (the message names the point): PMV_ERR_INVALID.
 *     On an error nothing is written and nothing is clamped. Not logged by pmv_record_enable; the whole-sequence drivers and pmv_klt_step do
 *     not call this. The call shares the staging blocks of pmv_find_fundamental_mat. */
int pmv_find_homography(pmv_ctx* ctx, const float* p1_xy, const float* p2_xy, int n, double threshold, double confidence, int max_iters, double* H9,
                        uint8_t* mask, int* out_found, int* out_samples_drawn);
/* diagnostic, ctx-free: pmv_debug_essential_iters_table for the 4 model points of pmv_find_homography: *out_num = log(1 - confidence),
 * out_denoms[g] = log(1 - (1 - (n - g) / n)^4) for g = 0..n (n + 1 doubles; -infinity where RANSACUpdateNumIters returns 0 before its
 * logarithms). n < 0 or a null pointer: PMV_ERR_INVALID. */
int pmv_debug_homography_iters_table(int n, double confidence, double* out_denoms, double* out_num);
/* diagnostic, ctx-free: the argument rules of pmv_find_homography for a context of max_tracks, in its order and with its codes; reads the
 * points, writes nothing but out_message256 (optional: the message the call would leave, 256 bytes). */
int pmv_debug_homography_check(int max_tracks, const float* p1_xy, const float* p2_xy, int n, double threshold, double confidence, int max_iters,
                               const double* H9, const uint8_t* mask, const int* out_found, const int* out_samples_drawn, char* out_message256);
/* diagnostic: out2 = {k_homography_ransac launches, requests they served} since the context was created (pmv_find_homography: one each;
 * pmv_batch_find_homography: one launch per round of the five-point combiner that holds such requests). */
int pmv_debug_homography_launches(pmv_ctx* ctx, long long* out2);

/* ---- A device-resident KLT tracker: one call per frame, the tracks stay in HBM ------------------------------------------------------------
 * A tracker lives in the context and holds n <= target tracks, each an (id, age, xy) triple - xy float32 in the coordinates of the frame the
 * last step ran on - and next_id. A new tracker is empty with next_id = 0. pmv_klt_step runs the per-frame chain of a VINS-style front end
 * in ONE call; it is defined as a composition, bit for bit, of the single calls above plus the small policy stated here. No arithmetic of
 * LK, the F RANSAC, setMask, the detector or cornerSubPix changes; LK's parameters come from the context (pmv_set_lk_params).
 * The seven stages, n0 = the state's n ("=" means the same bytes):
 *   1. Track (skipped when n0 = 0; prev_slot is then ignored): fb_max_dist >= 0 - the outputs of pmv_lk_track_fb(prev_slot, cur_slot, state
 *      xy, flags 0); else those of pmv_lk_track_ex(.., flags 0). The launch uses the identity track order; the order changes no result.
 *   2. Filter: track i survives iff status[i] == 1, with fb on also back_status[i] == 1 and dx * dx + dy * dy <= thr2 (dx = back.x - prev.x,
 *      dy likewise; both products and the sum float32 operations without contraction; thr2 = (float)(fb_max_dist * fb_max_dist), computed
 *      on the host), and its forward position is inside the border: ix = lrintf(x), iy = lrintf(y) (round half to even),
 *      border <= ix < w - border and border <= iy < h - border. Stable compaction; survivors get age += 1; their count is n1.
 *   3. rejectWithF (only if reject_f and n1 >= 15): pmv_find_fundamental_mat(prev xy of the survivors, cur xy of the survivors, n1,
 *      f_threshold, f_confidence); tracks with mask 0 go. No model: cv's status is all zero, so ALL go, as the VINS loop does with cv's
 *      output. Otherwise nothing happens and counts[5] = -1. Stable compaction; the count is n2.
 *   4. Thin: out_keep of pmv_detect_gftt_refill(cur_slot, roi NULL, .., the n2 cur positions in list order, prio NULL, n2, radius, base
 *      NULL) - the list is age-descending by construction, so this is setMask's order. Tracks not kept go; the count is n3.
 *   5. Refill (only if target - n3 > 0): the corners of the same refill call with max_corners = target - n3 (out_keep does not depend on
 *      max_corners); m corners, positions (float)x, (float)y.
 *   6. Refine (only if subpix and m > 0): pmv_corner_subpix(cur_slot, the m corners, subpix_params).
 *   7. Append: the m new tracks come after the survivors, in detector order, with ids next_id .. next_id + m - 1 and age 1; next_id += m.
 * Outputs: *out_n = n3 + m <= target; the list in out_ids, out_ages, out_xy (2 floats a track); out_prev_xy (may be NULL): the position in
 *   the previous frame, for a new track its own xy; out_counts8 = {n0, n1, n2, n3, m, f_found (-1 not run / 0 / 1), f_samples_drawn, 0}.
 *   The state becomes the output.
 * pmv_klt_set_tracks replaces the state (n in 0..target, else PMV_ERR_CAPACITY; a null array with n > 0, next_id < 0 or a coordinate that
 *   is not finite or beyond 1e6 in magnitude: PMV_ERR_INVALID; the state is kept on an error); pmv_klt_get_tracks reads it (cap < n:
 *   PMV_ERR_CAPACITY).
 * Device side: the kernels hand the counts to each other through device memory, the host never learns the intermediate lists. With reject_f
 *   = 0 a step waits ONCE; with reject_f = 1 at most twice - the first wait reads the single word n1, because the F kernel's iteration
 *   table (libm's pow and log) depends on it. Only request records, that table and the result block cross the bus. The scratch of a step
 *   is the tracker's own or the context's and is rewritten by every step: single calls between two steps return their usual bytes and do
 *   not disturb the next step, and neither do other trackers of the context.
 * Errors (nothing is written, nothing is clamped, the state is unchanged): PMV_ERR_INVALID - a null argument, an unknown id; at
 *   pmv_klt_create target < 1, border outside 0..64, fb_max_dist not finite or above 1e3, reject_f or subpix other than 0 / 1, radius
 *   outside 0..PMV_REFILL_MAX_RADIUS, and the parameter errors of pmv_find_fundamental_mat (if reject_f), pmv_detect_gftt_frame and
 *   pmv_corner_subpix (if subpix), each with that call's code and wording; PMV_ERR_CAPACITY - target above min(max_tracks,
 *   PMV_REFILL_MAX_TRACKS), a 17th tracker, out_cap < target; the slot errors of pmv_lk_track and pmv_detect_gftt_frame (range, empty
 *   slot, differing sizes, open bracket). pmv_ctx_destroy frees the trackers that are left. Not logged by pmv_record_enable; legal during
 *   a batch session under the caller's slot rule, like the other single calls.
 * Out of scope: the session form (pmv_batch_klt_*), a region or base mask, an initial-flow prediction as a field of pmv_klt_params (it is a
 *   one-shot setting of its own: pmv_klt_set_prediction below), per-track radius, LMedS or 8-point
 *   for n1 < 15, undistorting points before F by a field of pmv_klt_params (the observation setting does it: undistorted_f of
 *   pmv_klt_set_observe below), id wrap-around. */
#define PMV_KLT_MAX_TRACKERS 16
typedef struct pmv_klt_params {
    int    target;          /* MAX_CNT: tracks wanted after a step; 1 .. min(ctx max_tracks, PMV_REFILL_MAX_TRACKS) */
    int    border;          /* BORDER_SIZE of inBorder; 0 .. 64 */
    double fb_max_dist;     /* < 0: no backward pass (pmv_lk_track_ex); else finite, 0 .. 1e3: forward-backward check */
    int    reject_f;        /* 0 / 1 */
    double f_threshold, f_confidence;   /* as pmv_find_fundamental_mat; read only if reject_f */
    int    radius;          /* setMask's circle radius, 0 .. PMV_REFILL_MAX_RADIUS */
    pmv_gftt_params gftt;   /* the detector's arguments, as pmv_detect_gftt_frame */
    int    subpix;          /* 0 / 1: refine the new corners */
    pmv_subpix_params subpix_params;    /* read only if subpix */
} pmv_klt_params;
int pmv_klt_create(pmv_ctx* ctx, const pmv_klt_params* p, int* out_id);
int pmv_klt_destroy(pmv_ctx* ctx, int id);
int pmv_klt_set_tracks(pmv_ctx* ctx, int id, const int* ids, const int* ages, const float* xy, int n, int next_id);
int pmv_klt_get_tracks(pmv_ctx* ctx, int id, int* ids, int* ages, float* xy, int cap, int* out_n);
int pmv_klt_step(pmv_ctx* ctx, int id, int prev_slot, int cur_slot, int* out_ids, int* out_ages, float* out_xy, float* out_prev_xy_or_null,
                 int out_cap, int* out_n, int* out_counts8);
/* diagnostic: out4 = {steps, host waits inside steps, kernel launches inside steps, trackers alive} since the context was created */
int pmv_debug_klt_stats(pmv_ctx* ctx, long long* out4);

/* ---- A group of trackers in one call: pmv_klt_step_many ------------------------------------------------------------------------------------
 * A step is 8-10 short, serially dependent launches and one or two host waits; a caller with several cameras (a rig, sequences replayed side by
 * side; left and right of a stereo rig share ONE list: pmv_klt_step_stereo below) pays that once per camera with pmv_klt_step. pmv_klt_step_many steps n_trk trackers of the context through ONE chain
 * of launches.
 * Result definition: tracker j of the call is ids[j]. Its lists start at track j * out_stride of out_ids / out_ages / out_xy / out_prev_xy
 *   (xy: 2 floats a track), its count is out_n[j] and its counts are out_counts8[8 j .. 8 j + 7]. For every j the outputs and the tracker's
 *   new state are, byte for byte, what pmv_klt_step(ctx, ids[j], prev_slots[j], cur_slots[j], ..) returns from the same state. Trackers are
 *   independent: the order within the group changes nothing, and two trackers may name the same slots. No arithmetic of any stage changes.
 * Per tracker: target, border, fb_max_dist (on or off), reject_f, f_threshold, f_confidence, radius and the length of the list may differ
 *   from tracker to tracker; an empty tracker may sit next to full ones.
 * Launch-wide: the five fields of gftt, subpix and (if subpix) subpix_params are arguments of the detector's and the refinement's one launch
 *   and must be equal over the group; all cur_slots must hold frames of one size (and so do the prev_slots of the trackers that track, by
 *   pmv_klt_step's own slot rule). A difference is PMV_ERR_INVALID; the message names the first tracker that differs from tracker 0 and the
 *   field. Every pmv_set_lk_params setting is served.
 * Errors (nothing is written, nothing is clamped, no tracker of the group changes its state): PMV_ERR_INVALID - a null argument
 *   (out_prev_xy may be NULL), n_trk < 1, an unknown id, an id named twice; PMV_ERR_CAPACITY - n_trk > PMV_KLT_MAX_TRACKERS, out_stride
 *   below the largest target of the group; the slot errors of pmv_klt_step for whichever tracker they hit (the message says which). The
 *   host updates n and next_id of the trackers only after the last wait, once every tracker's result block is complete; an incomplete
 *   block is PMV_ERR_HIP and updates nothing.
 * Device side: the launches and waits of a call do not depend on n_trk - at most 12 launches (a step's chain plus one kernel that writes
 *   LK's records in device memory from the trackers' states, so no position crosses the bus on the way in; one more, LK's gated second
 *   launch, in a call in which a tracker has a pending prediction: pmv_klt_set_prediction below) and at most two waits, one when no
 *   tracker of the group has reject_f = 1 and 15 tracks. The first wait reads the n_trk words n1; the F problems and iteration tables of
 *   the trackers with n1 >= 15 go up in one copy and run in one launch, the others pass their list through. The filter, the two
 *   compactions and the append run one workgroup per tracker on per-tracker argument records; the detector's record lists, the painted
 *   masks and the kept lists are per-tracker shares of the context's scratch, which the call grows as needed.
 * Mixing: a tracker may be stepped by pmv_klt_step and pmv_klt_step_many in any mixture; single calls between many-calls return their usual
 *   bytes. Legal during a batch session under the caller's slot rule; the call keeps a one-entry geometry table of its own and does not
 *   touch the session's. The first three counters of pmv_debug_klt_stats count pmv_klt_step only; many-calls are counted by
 *   pmv_debug_klt_many_stats; pmv_debug_refill_stats does not move.
 * Out of scope: the session form (pmv_batch_klt_*, which can be laid over this call), groups with mixed frame sizes, detector arguments or
 *   refinement arguments, more than PMV_KLT_MAX_TRACKERS trackers, and everything pmv_klt_step lists. */
int pmv_klt_step_many(pmv_ctx* ctx, int n_trk, const int* ids, const int* prev_slots, const int* cur_slots, int* out_ids, int* out_ages, float* out_xy,
                      float* out_prev_xy_or_null, int out_stride, int* out_n /* n_trk */, int* out_counts8 /* 8 * n_trk */);
/* diagnostic: out4 = {many-calls, trackers stepped by them, host waits inside them, kernel launches inside them} since the context was created */
int pmv_debug_klt_many_stats(pmv_ctx* ctx, long long* out4);

/* ---- Stereo matches in the tracker step: left-to-right LK as stage 8 ----------------------------------------------------------------------
 * A stereo front end of the VINS kind (FeatureTracker::trackImage with a second image) keeps ONE list, on the left camera; after the refill
 * it runs LK from the current left frame into the current right frame for every track of the list, new corners included, and LK back, and a
 * track gets a right observation iff both passes succeed and the round trip ends near its start. pmv_klt_step_stereo is pmv_klt_step with
 * that as a stage 8 behind the append, in the same call and with no additional wait; pmv_klt_step and pmv_klt_step_many are unchanged.
 * Result definition: let (ids, ages, xy, prev_xy, counts8, n) be what pmv_klt_step(ctx, id, prev_slot, cur_slot, ..) returns from the
 *   tracker's state. The stereo step returns exactly those bytes and leaves exactly that state (the right observations are not state),
 *   except counts8[7], and in addition, for i < n:
 *   Back check on (the stereo setting's fb_max_dist >= 0): (rxy, st, err, back, bst, berr) = the outputs of pmv_lk_track_fb(ctx, cur_slot,
 *     right_slot, xy, n, flags 0) under the context's pmv_set_lk_params; ok[i] = st[i] == 1 && bst[i] == 1 && dx * dx + dy * dy <= thr2 &&
 *     inBorder(rxy[i]), with dx = back.x - xy.x, dy likewise, both products and the sum float32 operations without contraction, thr2 =
 *     (float)(fb_max_dist * fb_max_dist) computed on the host, and inBorder stage 2's rule (lrintf, round half to even) with the stereo
 *     setting's border and the right frame's size. This is stage 2's arithmetic, run by stage 2's code.
 *   Back check off (fb_max_dist < 0): the outputs are those of pmv_lk_track_ex(.., flags 0); ok[i] = st[i] == 1 && inBorder(rxy[i]).
 *   out_right_xy[2 i .. 2 i + 1] = the bits of rxy[i] for every i < n, matched or not; out_right_status[i] = ok[i] as 0 or 1; counts8[7] =
 *     the number of matched tracks (0 in pmv_klt_step, which stays so). The arrays are aligned with the left list: a caller pairs by index.
 *   n == 0: nothing is written to the right arrays and counts8[7] = 0.
 * Two differences from the VINS loop: the backward pass of pmv_lk_track_fb starts at the left position (its initial-flow second trip),
 *   while the VINS stereo reverse pass starts at the right position; and VINS applies no border test when its back check is off, this stage
 *   applies one.
 * pmv_klt_set_stereo gives a tracker its stereo setting (NULL turns it off, which is the default; it may change between steps);
 *   pmv_klt_get_stereo reads it (*out_on = 0 / 1; *out = the last setting given, zeros if none).
 * pmv_klt_step_many_stereo: tracker j is byte for byte its own pmv_klt_step_stereo. right_slots[j] < 0 means tracker j has no right frame
 *   in this call (a mono camera in a rig next to a stereo pair): it gets the bytes of pmv_klt_step, right status all 0 and counts8[7] = 0,
 *   its right xy are not written and it needs no stereo setting. fb_max_dist and border may differ from tracker to tracker; the right
 *   frames have the size of the group's current frames. Tracker j's right arrays start at track j * out_stride, like its left lists.
 * Device side: no additional wait - a stereo step waits as often as pmv_klt_step from the same state (once, twice with reject_f), a stereo
 *   many-call at most twice; the launches of stage 8 are enqueued behind the append. The length of the list after the append is known only
 *   on the device: the LK launch of stage 8 is sized by the bound (target; in the many form the sum of the targets of the trackers with a
 *   right slot) and reads the count the append left in device memory; workgroups beyond it leave at once. Stage 8 adds at most 3 launches to
 *   a step and at most 3 to a many-call, whatever n_trk is. Its scratch is the LK result arrays of stage 1, free again by then: single
 *   calls between two steps return their usual bytes.
 * Errors (nothing is written, nothing is clamped, no tracker's state changes): PMV_ERR_INVALID - a null out_right_xy or out_right_status
 *   (or right_slots); a stereo step on a tracker without a stereo setting (the message says so); at pmv_klt_set_stereo fb_max_dist not
 *   finite (either infinity included) or above 1e3, border outside 0..64 (the old setting is kept). The slot errors of pmv_lk_track for the pair (cur_slot,
 *   right_slot) - range, empty slot, differing sizes, open bracket - with that call's code, checked before anything is launched, since n
 *   is unknown then; in the many form the message names the tracker. Everything pmv_klt_step and pmv_klt_step_many refuse is refused in the
 *   same words. The last kernel of the chain is the stereo one and writes the completion word the host checks: an incomplete result block
 *   is PMV_ERR_HIP and n and next_id are not updated.
 * Counters: stereo calls do not move pmv_debug_klt_stats or pmv_debug_klt_many_stats; pmv_debug_klt_stereo_stats counts them.
 * Out of scope: the session form, a backward pass without the initial guess, a right frame of another size or pyramid depth, an epipolar
 *   band or a disparity prior, compacted right lists, right positions as tracker state (normalised coordinates and velocities: the
 *   observation setting below). */
typedef struct pmv_klt_stereo_params {
    double fb_max_dist;     /* finite; < 0: no backward pass, else 0 .. 1e3 */
    int    border;          /* 0 .. 64 */
} pmv_klt_stereo_params;
int pmv_klt_set_stereo(pmv_ctx* ctx, int id, const pmv_klt_stereo_params* p_or_null);
int pmv_klt_get_stereo(pmv_ctx* ctx, int id, pmv_klt_stereo_params* out, int* out_on);
int pmv_klt_step_stereo(pmv_ctx* ctx, int id, int prev_slot, int cur_slot, int right_slot, int* out_ids, int* out_ages, float* out_xy,
                        float* out_prev_xy_or_null, float* out_right_xy, uint8_t* out_right_status, int out_cap, int* out_n, int* out_counts8);
int pmv_klt_step_many_stereo(pmv_ctx* ctx, int n_trk, const int* ids, const int* prev_slots, const int* cur_slots, const int* right_slots,
                             int* out_ids, int* out_ages, float* out_xy, float* out_prev_xy_or_null, float* out_right_xy,
                             uint8_t* out_right_status, int out_stride, int* out_n /* n_trk */, int* out_counts8 /* 8 * n_trk */);
/* diagnostic: out4 = {stereo steps, stereo many-calls, host waits inside both, kernel launches inside both} since the context was created */
int pmv_debug_klt_stereo_stats(pmv_ctx* ctx, long long* out4);

/* ---- Normalised observations and velocities from the tracker step: the lift as stage 9 -------------------------------------------------------
 * A VIO or VO back end consumes, per track, (id, x, y, 1, u, v, vx, vy): the position on the normalised image plane through the camera's
 * distortion model and its velocity there; a stereo back end also the normalised right observation. A tracker with an observation setting
 * returns them from the same step call, with at most one launch more and no additional wait, and can run stage 3 on undistorted points as
 * FeatureTracker::rejectWithF does. The setting is off by default; with it off every step form makes the launches, waits and bytes it
 * makes without this section. No step entry point gets a new signature: pmv_klt_step, pmv_klt_step_stereo, pmv_klt_step_many and
 * pmv_klt_step_many_stereo stay as they are, and the observations are read afterwards with pmv_klt_get_observations.
 * pmv_klt_set_observe gives a tracker its setting (NULL turns it off; it may change between steps, dt for example; a bad value keeps the old
 *   setting); pmv_klt_get_observe reads it (*out_on = 0 / 1; *out = the last setting given, zeros if none). In a group the cameras, dt and on /
 *   off may differ from tracker to tracker.
 * Result definition of stage 9: a pure function of what the step returns - (ages, xy, prev_xy, n) and in a stereo call (right_xy,
 *   right_status) - with lift = pmv_undistort_points' rule for one point (result (0, 0) and ok 0 where it refuses). For i < n:
 *     (un, ok) = lift(cam_id, xy[i]); (pun, pok) = lift(cam_id, prev_xy[i]); out_un_xy[i] = un; out_ok[i] = ok.
 *     ages[i] > 1 && ok && pok: vel.x = (float)((double)(un.x - pun.x) / dt), vel.y likewise - the subtraction is one float32 operation on
 *       the lifts already rounded to float32 (VINS keeps them as Point2f), the division is in double. Otherwise vel = (0, 0): a new track,
 *       whose prev_xy is its own xy, has no velocity. Lifting prev_xy again gives the bits of the previous step's un (the same function of
 *       the same float), so no per-track state is added.
 *     In a stereo call with right_cam_id >= 0 and, in the many form, right_slots[j] >= 0: (run, rok) = lift(right_cam_id, right_xy[i]);
 *       out_right_un_xy[i] = run; out_right_ok[i] = right_status[i] && rok - unmatched tracks are lifted too and get ok 0. Otherwise
 *       out_right_ok is all 0 and the right xy are not written.
 *   The step's own outputs and the tracker's state are byte for byte those of the same step with the setting off.
 * pmv_klt_get_observations copies the observations of the tracker's last step out of its result block - a host copy, no device work;
 *   *out_n = n of that step; the two right arrays may be NULL. PMV_ERR_INVALID if the tracker's last step ran with the setting off, or if it
 *   has not stepped since pmv_klt_create or pmv_klt_set_tracks (the message says which); PMV_ERR_CAPACITY for cap < n.
 * rejectWithF on undistorted points (undistorted_f = 1): stage 3, which still runs only for reject_f and n1 >= 15, takes as its two point
 *   sets the virtual-camera points of VINS instead of the pixels. For survivor i and both its previous and its current position, with
 *   (xd, yd) the double pair of the lift BEFORE its rounding to float and w, h the frame size:
 *     q = ((float)(f_focal * xd + w / 2.0), (float)(f_focal * yd + h / 2.0)), the product and the sum separate double operations.
 *   If either of the track's two lifts is not finite, both of its points are (0, 0); it goes or stays by F's mask like any other.
 *   pmv_find_fundamental_mat's arithmetic on those float points, f_threshold, the mask, the compaction and counts8[5..6] are unchanged.
 * Device side: the observe kernel is the last of the chain (behind the append, or behind stage 8) and writes its own completion word, which
 *   the host checks only for trackers with the setting on: an incomplete block is PMV_ERR_HIP and n and next_id are not updated. One
 *   workgroup per tracker; a many-call makes one observe launch whatever n_trk is, and a tracker of the group with the setting off leaves at
 *   once. The lift for stage 3 is one more launch, sized by n0 and enqueued before the host's wait for n1, so it runs under that wait; its
 *   scratch is the LK result arrays of stage 1, free by then. pmv_debug_klt_observe_stats counts; the other klt counters count these
 *   launches with the rest of the call's.
 * Errors (nothing is written, the old setting is kept): PMV_ERR_INVALID - a null argument, an unknown tracker, a cam_id that is no camera,
 *   a right_cam_id that is neither -1 nor a camera, dt not finite or not above 0, undistorted_f other than 0 / 1, with undistorted_f a
 *   f_focal not finite or not above 0. A camera named by a setting cannot be destroyed until the setting is cleared.
 * Out of scope: right-camera velocities (they need right positions as tracker state, which the stereo section excludes); the session form
 *   (pmv_batch_*); an undistorted_f that lifts through a camera other than cam_id; camera models other than the two of pmv_camera_create and
 *   pmv_camera_create_fisheye (cv::fisheye's skew among them), R / P, thin-prism and tilt coefficients and a forward distort_points call,
 *   as for pmv_undistort_points. */
typedef struct pmv_klt_observe_params {
    int    cam_id;          /* the left camera */
    int    right_cam_id;    /* the right camera, or -1: no normalised right observations */
    double dt;              /* seconds between the previous and this frame; finite, > 0 */
    int    undistorted_f;   /* 0 / 1: stage 3 runs on lifted points */
    double f_focal;         /* the virtual focal length of that stage (VINS: 460); finite, > 0; read only if undistorted_f */
} pmv_klt_observe_params;
int pmv_klt_set_observe(pmv_ctx* ctx, int id, const pmv_klt_observe_params* p_or_null);   /* NULL: off (the default) */
int pmv_klt_get_observe(pmv_ctx* ctx, int id, pmv_klt_observe_params* out, int* out_on);
int pmv_klt_get_observations(pmv_ctx* ctx, int id, float* out_un_xy, float* out_vel, uint8_t* out_ok, float* out_right_un_xy_or_null,
                             uint8_t* out_right_ok_or_null, int cap, int* out_n);
/* diagnostic: out4 = {step calls with the setting on, observe launches, lift-for-F launches, host waits inside those calls} since the context
 * was created */
int pmv_debug_klt_observe_stats(pmv_ctx* ctx, long long* out4);

/* ---- Predicted positions in the tracker step: projected guesses, capped LK levels ---------------------------------------------------------
 * When the back end has a pose and landmarks, a VINS-style front end projects them into the new image (setPrediction, spaceToPlane), runs
 * LK from those guesses on two pyramid levels instead of four, falls back to the full pyramid only if fewer than 10 points succeed, and
 * always runs its reverse check on two levels (FeatureTracker::trackImage, hasPrediction). pmv_klt_set_prediction gives a tracker such a
 * prediction: points in the camera frame of the NEW image, keyed by track id. It is one-shot: the tracker's next step that succeeds,
 * through any of the four step entry points, consumes it; a refused step leaves it pending; NULL or n = 0 clears it; pmv_klt_set_tracks
 * leaves it pending (the join is by id). No step entry point gets a new signature, and a tracker with no pending prediction makes the
 * launches, waits and bytes it makes without this section.
 * Result definition of a consuming step: only stage 1 changes; stages 2 to 9 are untouched. For track i of the state (n0 tracks, positions xy):
 *     guess[i] = pmv_project_points(cam_id, xyz[k]) if ids[k] equals the track's id and that projection is ok, else xy[i];
 *     joined   = the number of tracks of the first kind;
 *     A        = the outputs of pmv_lk_track_fb_levels(prev_slot, cur_slot, xy, next_xy = guess, PMV_LK_USE_INITIAL_FLOW, top_level,
 *                back_top_level, ..), forward only (three null back outputs) when the tracker's fb_max_dist < 0;
 *     succ     = the number of i with A's forward status equal to 1;
 *     succ < min_succ: A = the outputs of pmv_lk_track_fb_levels(.., flags 0, -1, back_top_level, ..) and fell_back = 1.
 *   Stage 2 filters A exactly as it filters stage 1's outputs in any other step. With n0 = 0 the prediction is consumed with {1, 0, 0, 0}.
 *   out_counts8 keeps its meaning, and all eight words are taken. pmv_klt_get_prediction_result returns {consumed, joined, succ, fell_back}
 *   of the tracker's last step - a host copy; {0, 0, 0, 0} after a step that had no prediction to consume and before the first step.
 *   Ids that no track has, and tracks without an entry, are no error; the order of the list changes nothing. A point of any value is
 *   legal: one that pmv_project_points refuses (not finite, Z <= 0, beyond 1e6) simply predicts nothing.
 * Device side: no additional wait; at most 2 more launches in a single step and at most 2 more in a many-call, whatever n_trk is (a single
 *   step makes 2 more, a many-call 1). The join and projection kernel runs one workgroup per tracker (k_klt_predict; in a group it is folded
 *   into the kernel that writes LK's records): a binary search per track in the prediction list, which the host sorts once at
 *   pmv_klt_set_prediction, project_point for a hit, the guess into the initial-flow array or the LK record, and the tracker's success word
 *   zeroed. The predicted LK launch counts its forward successes into that word - one integer atomic add by one lane of a workgroup, whose
 *   sum does not depend on the order of the workgroups, so the bytes are deterministic. The fall-back is a second LK launch of the same
 *   size, n0, whose workgroups read the word first and leave at once when succ >= min_succ - a workgroup-uniform decision; it never counts
 *   from the result arrays, which other workgroups of the same launch are overwriting. In a group, trackers with and without a pending
 *   prediction mix freely, and their settings may differ. pmv_debug_klt_stats and its siblings count the new launches with the call's.
 * Errors (the old state is kept - a pending prediction stays pending - and nothing is written): PMV_ERR_INVALID - a null argument with n >
 *   0, an unknown tracker, n < 0, an id named twice (the message names it), top_level outside 0..4, back_top_level outside -1..4, a cam_id
 *   that is no camera, min_succ < 0; PMV_ERR_CAPACITY - n above PMV_REFILL_MAX_TRACKS. A camera named by a pending prediction cannot be
 *   destroyed until the prediction is consumed or cleared.
 * Out of scope: the session form; camera models other than the two of pmv_camera_create and pmv_camera_create_fisheye; a level per track; back_top_level for steps without a
 *   prediction; stereo stage 8 at a capped level; rvec / tvec (the caller transforms the landmarks into the camera frame). */
typedef struct pmv_klt_predict_params {
    int cam_id;           /* the camera that projects the points */
    int top_level;        /* the predicted forward pass starts at min(top_level, L - 1); 0 .. 4 (VINS: 1) */
    int back_top_level;   /* the backward pass of the consuming step; -1: the pyramid's top, else 0 .. 4 (VINS: 1) */
    int min_succ;         /* fall back if fewer forward status-1 tracks; >= 0 (VINS: 10) */
} pmv_klt_predict_params;
int pmv_klt_set_prediction(pmv_ctx* ctx, int id, const pmv_klt_predict_params* p_or_null, const int* ids, const double* xyz /* 3 n */, int n);
int pmv_klt_get_prediction_result(pmv_ctx* ctx, int id, int* out4);   /* {consumed, joined, succ, fell_back} of the last step; a host copy */

/* ---- call log (parity tooling) -------------------------------------------------------------------------------------------
 * While recording is on, every pmv_pnp_ransac / pmv_ba_solve / pmv_triangulate_candidates call of this context (also those
 * made from inside pmv_pipeline_run) appends one blob holding its inputs and outputs, so that a test can replay the calls
 * of a whole run, one by one, through another implementation ("teacher forcing"). Little-endian, tightly packed:
 *   PnP:  int32 {0, m, iterations, n_inliers}; f32 obj[3m], img[2m]; f64 K[9], rvec_in[3], tvec_in[3], reproj_err, confidence;
 *         f64 rvec_out[3], tvec_out[3]; int32 inliers[n_inliers]
 *   BA:   int32 {1, nc, np, n_obs, max_iterations}; f64 cams_in[6nc], pts_in[3np], obs[2n_obs], K[9], huber;
 *         int32 cam_idx[n_obs], pt_idx[n_obs]; f64 cams_out[6nc], pts_out[3np], summary[5] (initial, final cost, iterations,
 *         successful steps, termination)
 *   DLT:  int32 {2, n}; f64 q1[2n], q2[2n], P1x4[48]; u8 mask_in[n]; f64 Q[16n]; u8 mask[4n]; int32 good[4]
 * pmv_record_enable(ctx, 1) clears the log and starts, (ctx, 0) stops (the log stays readable). Not thread-safe against a
 * running pipeline: read after the run. */
int pmv_record_enable(pmv_ctx* ctx, int on);
int pmv_record_count(pmv_ctx* ctx);
long long pmv_record_size(pmv_ctx* ctx, int i);
int pmv_record_get(pmv_ctx* ctx, int i, void* out, long long capacity);

/* ---- per-kernel timing (HIP events on the launching stream; used by bench.py for the roofline object) -------------- */
int pmv_prof_enable(pmv_ctx* ctx, int on);  /* on != 0: reset counters and start recording; 0: stop */
int pmv_prof_select(pmv_ctx* ctx, unsigned mask); /* after pmv_prof_enable(1): record only classes whose bit (= id) is set */
int pmv_prof_kernel_count(void);
/* k_lk / k_lk_batch work since context creation / last reset: out3 = {LK iterations, (track, level) passes, tracks}; summed on the
 * host from a 16-bit word per track that the kernels write next to their results (no device-side atomics) */
int pmv_lk_counters(pmv_ctx* ctx, unsigned long long* out3, int reset);
const char* pmv_prof_kernel_name(int id);
int pmv_prof_read(pmv_ctx* ctx, int id, int* launches, double* total_ms, double* max_ms);

/* ---- whole-sequence driver -------------------------------------------------------------------------------------- */
/* Runs the reference's OdometryPipeline schedule (initialise, addFrame per frame, estimatePose with lag 2, BA every
 * bundle_size/3*2 frames; OdometryPipeline.cpp:247-264, :329-426) with every plugin call served by the kernels above.
 * Frames 0..n_frames-1 must already be staged in slots 0..n_frames-1 (pmv_frames_stage); with build_pyramids != 0 the
 * pyramids of all frames are (re)built first, inside the call, so that a benchmark times HBM-resident gray frames ->
 * poses. gt_poses12: n_frames KITTI pose rows (only the translation column is used, for the monocular scale, quirk Q11). */
typedef struct pmv_pipeline_params {
    int n_frames, w, h;
    int min_tracked_features, tracked_features_tol, init_frames, bundle_size, ba_iterations;
    int extractor;      /* 0 = goodFeaturesToTrack (reference default), 1 = ShiTomasi, 2 = FAST (OpenCVFASTFeatureExtractor) */
    int threaded;       /* 0 = sequential schedule, 1 = front-end / back-end host threads (the reference's two threads) */
    int n_threads;      /* host threads that evaluate the triangulator's five-point RANSAC hypotheses side by side (>= 1; results do not depend on it) */
    int build_pyramids; /* rebuild the pyramids of slots 0..n_frames-1 inside the call */
    int matcher;        /* 0 = pyramidal LK (reference default), 1 = kNNFeatureMatcher over `extractor` */
    int device_fivepoint; /* 0 = five-point RANSAC on host threads, 1 = its hypotheses on the GPU, one launch per round of 32 (pmv_fivepoint_hypotheses),
                           * 2 = the whole RANSAC of a call in one launch (pmv_find_essential_mat); same results, [23] included */
} pmv_pipeline_params;
typedef struct pmv_pipeline_result pmv_pipeline_result;

int pmv_pipeline_run(pmv_ctx* ctx, const pmv_pipeline_params* params, const double* K9, const double* gt_poses12,
                     pmv_pipeline_result** out);
/* The same run from n_frames frames (gray, or BGR: pmv_set_frame_format; remapped / equalised on the way in: pmv_set_frame_preproc) in HOST memory: pmv_frames_stream_begin(ctx, 0, n_frames, host_frames, w, h), the run
 * (build_pyramids ignored), pmv_frames_stream_end. Identical results; copies and pyramid builds overlap the tracking. */
int pmv_pipeline_run_streamed(pmv_ctx* ctx, const pmv_pipeline_params* params, const double* K9, const double* gt_poses12,
                              const uint8_t* host_frames, pmv_pipeline_result** out);
/* B independent sequences through batched launches (SURVEY.md §8e "same kernels with a leading batch dimension"): sequence b =
 * frame slots first_slot[b] .. + params[b].n_frames - 1 (pmv_frames_stage; ranges may overlap, a shared slot is
 * built once), intrinsics K9 + 9 b, ground
 * truth gt_poses12[b].
 *   Frame sizes: per sequence, from params[b].w / params[b].h - the reference takes whatever cv::imread returns (Frame.cpp:31-42) and KITTI
 *     odometry comes in three sizes. Every size lies within the context's capacity (40 x 40 .. max_w x max_h, else PMV_ERR_CAPACITY); a batch
 *     may hold any mix of them and still makes one k_lk_batch / k_knn_round launch per round and one k_pad_level0 / k_pyrdown launch per
 *     feeder round and level (each track / request / frame record names its geometry in a small table in device memory). params[b].w / h must
 *     equal the size staged in every slot of sequence b's range, so overlapping ranges must agree on the size of every shared slot: otherwise
 *     PMV_ERR_INVALID, naming the sequence, before a sequence starts. Each sequence keeps the reference's front-end / back-end host threads; their plugin calls are merged into
 * one k_lk_batch / detector / k_pnp_*_batch / k_bamB_* / k_tri_dlt_batch launch per kernel class by that class's combiner
 * thread (one HIP stream each); the combiners are the only threads that talk to the HIP runtime. out[b] is bit-identical to the same sequence's own pmv_pipeline_run.
 *   Plugins: params[b] takes every pair pmv_pipeline_run takes - extractor 0, 1 or 2 with matcher 0 (LK), and matcher = 1 (kNN) with
 *     extractor = 2 (FAST): the kNN matcher calls the extractor on whole frames (kNNFeatureMatcher.cpp:11). Sequences with different pairs may
 *     share a batch: FAST requests go to the detector combiner (k_fast_score / k_fast_select over the cells of several frames), kNN requests
 *     to the LK combiners (one k_knn_round launch per round; counted under LK in pmv_batch_stats). Any other value or pair is
 *     PMV_ERR_INVALID before a sequence starts. */
int pmv_pipeline_run_batch(pmv_ctx* ctx, int B, const pmv_pipeline_params* params, const double* K9, const double* const* gt_poses12,
                           const int* first_slot, pmv_pipeline_result** out);
/* diagnostic: launches of the batched legs since the context was created: out4 = {k_lk_batch, k_knn_round (LK combiners), k_pad_level0 /
 * k_pad_level0_bgr, k_pyrdown (the feeder of the two batched entry points)}. Against the rounds of pmv_batch_stats / pmv_batch_ingest_stats
 * it shows that a round is one launch (per level) whatever frame sizes it holds. */
int pmv_debug_batch_launches(pmv_ctx* ctx, long long* out4);
/* The same B sequences streamed from HOST memory through recycled frame slots (the reference loads one image per front-end iteration,
 * Frame.cpp:31-42, OdometryPipeline.cpp:212-229, and tracking reads only frames k-1 and k), so that the batch size is not capped by frame
 * storage: B x ring slots instead of the sum of all n_frames.
 *   Frames: sequence b's params[b].n_frames tightly packed frames (gray, or BGR: pmv_set_frame_format; remapped / equalised on the way in: pmv_set_frame_preproc) at host_frames[b], pageable or pinned / registered; read only, several
 *     b may point at the same buffer; they stay valid until the call returns. A kernel never reads a pageable address: pinned memory
 *     mapped at its host address (hipHostMalloc, torch pin_memory) is read in place, anything else is copied into pinned staging first.
 *   Slots: sequence b owns slots first_slot[b] .. first_slot[b] + ring - 1 (disjoint ranges inside n_slots); frame f lives in slot
 *     first_slot[b] + f % ring. After the call each ring slot holds the last frame that went through it, pyramid built.
 *   Frame sizes: per sequence, from params[b].w / params[b].h (Frame.cpp:31-42: a run takes whatever size its images have), each within
 *     the context's capacity (else PMV_ERR_CAPACITY); host_frames[b] holds frames of that size, and every slot of sequence b's ring holds
 *     that size. Staging buffers are sized for the largest frame of the batch; pmv_batch_ingest_stats counts the bytes actually moved.
 *   Shared rules: build_pyramids is ignored (the feeder builds every frame as it lands); the
 *     parameters are validated as in pmv_pipeline_run_batch (bundle limits; the plugin pairs of pmv_pipeline_run: extractor 0, 1 or 2 with
 *     matcher 0, and matcher = 1 (kNN) with extractor = 2 (FAST), per sequence). The feeder needs nothing new for them: the kNN matcher reads
 *     frames k - 1 and k, FAST the whole frame k or the previous frame's cells, so the minimum ring and the release rule below hold as they are.
 *   Minimum ring: ring >= init_frames + 1. initialise() holds frames 0 .. init_frames - 1 (OdometryPipeline.cpp:428-482), and the first
 *     addFrame may need frame init_frames while frame init_offset is still live. A smaller ring is PMV_ERR_INVALID.
 *   Release rule: once addFrame(image i) (OdometryPipeline.cpp:329-374) has returned, every frame below i is dead - addFrame(i + 1) reads
 *     frames i (LK and the re-detection on the previous frame's cells) and i + 1 only - and its slot may be refilled. A sequence that
 *     finishes or fails frees its whole ring.
 *   Errors: a slot range outside n_slots is PMV_ERR_CAPACITY, overlapping ranges PMV_ERR_INVALID; a call while a pmv_frames_stream_begin
 *     bracket is open on the context is PMV_ERR_INVALID (the call owns the context until it returns, so the reverse cannot arise).
 *   Result: out[b] is bit-identical to the same sequence's pmv_pipeline_run_batch on staged frames and to its own pmv_pipeline_run: poses,
 *     per-frame features and landmark ids, and every count of the statistics.
 * Memory besides the rings: 4 pinned staging buffers of up to 64 frames (<= 32 MB) each; with PMV_BATCH_INGEST=copy as many HBM landing
 * buffers. These belong to the context's batch feeder: pmv_frames_stream_begin's landing area is not used. */
int pmv_pipeline_run_batch_streamed(pmv_ctx* ctx, int B, const pmv_pipeline_params* params, const double* K9, const double* const* gt_poses12,
                                    const uint8_t* const* host_frames, const int* first_slot, int ring, pmv_pipeline_result** out);
/* Ingest counters of the last pmv_pipeline_run_batch_streamed call: writes PMV_BATCH_INGEST_STATS (= 6) doubles to out and returns that
 * count (out = NULL: only the count, ctx may be NULL too): [0] ingest rounds [1] frames [2] bytes moved from host memory [3] seconds of host memcpy into the staging buffers
 * [4] seconds the ingest thread waited for ring room [5] seconds the sequence threads waited for frames (summed over the threads). */
#define PMV_BATCH_INGEST_STATS 6
int pmv_batch_ingest_stats(pmv_ctx* ctx, double* out);
/* diagnostic, per combiner in the order LK, detectors, PnP, BA, DLT: counts10 = {launch rounds, requests served} x 5; times15 (may
 * be NULL) = seconds spent {CPU time of the combiner thread, wall time processing batches, of that waiting for the GPU} x 5 */
int pmv_batch_stats(pmv_ctx* ctx, long long* counts10, double* times15);

/* ---- batch sessions: the batch engine for callers who bring their own pipeline --------------------------------------------------------
 * pmv_pipeline_run_batch[_streamed] run this library's own mirror of OdometryPipeline and need every frame of every sequence before the
 * call. A session opens the same machinery - the combiners of the five kernel classes and the list-form pyramid kernels - to plugin-level
 * callers: the reference's real OdometryPipeline behind the adapters of INTEGRATION.md, a live camera loop, a Python experiment. Frames
 * arrive one at a time, the length of a sequence is not known in advance, and B callers' requests share batched launches.
 *
 * pmv_batch_open: n_seq (1..256, else PMV_ERR_INVALID) back-end workspace sets; sizes_wh holds n_sizes (1..256) distinct (w, h) pairs:
 *   every frame that a session call will see has one of these sizes, each within 40x40 .. max_w x max_h (else PMV_ERR_CAPACITY; a pair named
 *   twice is PMV_ERR_INVALID). They become the geometry table of the batched launches. Memory: one pinned staging pool of min(64, max(4,
 *   2 n_seq)) blocks of the largest declared BGR frame (at most 256 MB), freed by pmv_batch_close.
 *   Ownership of the context: a session owns the batch engine and the geometry table. While one is open, pmv_pipeline_run_batch,
 *   pmv_pipeline_run_batch_streamed and a second pmv_batch_open return PMV_ERR_INVALID; pmv_batch_open during one of those runs returns
 *   PMV_ERR_INVALID. The single-sequence pmv_* calls stay legal on slots that no session call is using; pmv_set_frame_format is unaffected,
 *   because a session names the format per upload (a refused call changes nothing).
 * pmv_batch_close: PMV_ERR_INVALID while session calls are still outstanding, and without an open session. Afterwards the context serves
 *   batched runs again; the frame slots keep what they hold.
 * Any session call (every pmv_batch_* below) without an open session is PMV_ERR_INVALID.
 *
 * Threads: every session call may be made from any thread at any time, by any number of threads (n_seq does not limit the front-end calls:
 *   requests that do not fit a round's result blocks wait for the next round). Error text is per thread: read it with pmv_thread_error();
 *   pmv_last_error(ctx) is one buffer per context and holds the last message of ANY thread. The callers' threads launch nothing and wait for no HIP stream: requests go to the
 *   class's combiner thread, uploads to the upload thread. The four back-end calls (those that take `seq`) allow one outstanding call per
 *   seq and call; the calls of one seq share that seq's pinned block, so the library makes them take turns. seq outside 0 .. n_seq - 1 is
 *   PMV_ERR_INVALID.
 * Results: each call returns exactly the bits the single-sequence pmv_* call of the same name returns for the same inputs, with the same
 *   status codes raised in the same places (PMV_ERR_DEGENERATE of pmv_pnp_ransac, PMV_ERR_OVERFLOW of a no-limit pmv_detect_gftt, ...);
 *   pmv_batch_ba_solve matches pmv_ba_solve in the context's current pmv_set_ba_mode. The LK ordering hint of the batched runs stays
 *   internal: a session LK call uses the engine's default order, which changes no result.
 * Slots are the caller's to manage, as with pmv_frame_upload: a slot must not be uploaded into while a call that reads it is outstanding
 *   (for the reference's pipeline: frames k - 1 and k are live, so a ring of 3 slots per sequence is enough). This is the caller's rule;
 *   the library does not police it. Session calls must not name slots of an open pmv_frames_stream_begin bracket. */
int pmv_batch_open(pmv_ctx* ctx, int n_seq, const int* sizes_wh, int n_sizes);
int pmv_batch_close(pmv_ctx* ctx);
/* Like pmv_frame_upload / pmv_frame_upload_bgr (format: pmv_frame_format; anything else is PMV_ERR_INVALID), with `stride` bytes per source
 * row. Callable from any number of threads: the upload thread takes whatever requests accumulated while its previous round ran and builds
 * them in ONE round - at most one gray and one BGR level-0 launch and one k_pyrdown launch per level, whatever the number of requests and
 * the mix of sizes - on the upload stream.
 *   Sources: `pixels` may be pageable host memory, pinned mapped host memory, or device memory of the context's device. Pinned memory mapped
 *     at its host address (hipHostMalloc, torch pin_memory) and device memory are read IN PLACE by the kernel, at any base alignment and any
 *     stride (a camera buffer with aligned rows, an ROI view into a larger image, a hipMallocPitch surface): a row is fetched as the aligned
 *     dwords that hold its bytes and no others, so nothing past the last row's last byte is read. Anything else is copied by the calling
 *     thread, row by row and tight, into a block of the session's pinned staging pool (the call waits for a free block). Device memory of
 *     another device is PMV_ERR_INVALID, and so is a device frame that reaches past the end of its allocation.
 *     A source read in place is read by a kernel on the session's own stream, which waits for no other stream: whatever produced the
 *     pixels (a kernel or copy on the caller's stream, a decoder) must have COMPLETED before the call, e.g. by a stream synchronise.
 *   Return of an upload: when the call returns, the source may be reused and the slot is built (its size and state recorded); a session call
 *     on that slot from any thread needs no further ordering, because the request returned only after its round's completion word was seen.
 *   Upload errors: a size not declared at pmv_batch_open is PMV_ERR_INVALID and the message names the size; stride below w (gray) or 3 w
 *     (BGR) is PMV_ERR_CAPACITY; a slot outside n_slots is PMV_ERR_CAPACITY, as for pmv_frame_upload.
 *   Two uploads into one slot that meet in a round are built one after the other, in arrival order. */
int pmv_batch_frame_upload(pmv_ctx* ctx, int slot, const uint8_t* pixels, int w, int h, int stride, int format);
/* pmv_batch_frame_upload with the equalisation of pmv_frames_clahe inside the same upload round: the arguments, sources (pageable, pinned in
 * place, device in place, any stride), errors and return rule of pmv_batch_frame_upload, plus p (NULL is PMV_ERR_INVALID - the plain call
 * stays the way to upload without equalisation; the parameter errors of pmv_frames_clahe). The slot then holds the bytes of
 * pmv_frame_upload[_bgr] followed by pmv_frames_clahe with the same p, and the pyramid is built once.
 *   The upload thread serves these requests in the same round as plain uploads. A round with at least one of them runs, in this order: the
 *   level-0 launches it always makes; ONE k_clahe_lut launch and ONE k_clahe_apply launch for all its CLAHE requests, whatever their frame
 *   sizes and parameters (each record names its own); ONE in-place k_pad_level0 launch over those slots, which rebuilds their REFLECT_101
 *   frame and is counted as a level-0 launch of the round (pmv_batch_upload_stats out4[2], pmv_batch_upload_rounds [5]); the k_pyrdown
 *   launches it always makes. A round without CLAHE requests launches exactly what it launched before, and its records are what they were.
 *   The LUT scratch of a round (256 bytes per tile) is the session's own and grows to the largest round seen. */
int pmv_batch_frame_upload_clahe(pmv_ctx* ctx, int slot, const uint8_t* pixels, int w, int h, int stride, int format, const pmv_clahe_params* p);
/* pmv_batch_frame_upload with the remap of pmv_frames_remap inside the same upload round, and the equalisation of pmv_frames_clahe behind
 * it when clahe_or_null is set: the arguments, sources, errors and return rule of pmv_batch_frame_upload, plus the map and border errors of
 * pmv_frames_remap (w x h must be the map's size: PMV_ERR_INVALID, the message names the slot and both sizes) and, with clahe_or_null, the
 * parameter errors of pmv_frames_clahe. The slot then holds the bytes of pmv_frame_upload[_bgr], pmv_frames_remap, and with parameters
 * pmv_frames_clahe, in this order, and the pyramid is built once. A colour source is converted by the level-0 kernel first: the remap always
 * sees gray - conversion, then remap, then equalisation. A host source is never gathered over the bus: the gather reads HBM only.
 *   A round launches in this order: the level-0 launches it always makes; ONE k_remap launch for all remap requests of the round, from the
 *   slots into a session scratch (a tight frame per request; the scratch grows to the largest round seen); ONE list-form k_pad_level0
 *   launch from that scratch, counted as a level-0 launch of the round; the CLAHE stage of pmv_batch_frame_upload_clahe for the requests
 *   that carry parameters, of either call; the k_pyrdown launches, once. A round without remap requests launches and records exactly what
 *   it did before. */
int pmv_batch_frame_upload_remap(pmv_ctx* ctx, int slot, const uint8_t* pixels, int w, int h, int stride, int format, int map_id, int border_value,
                                 const pmv_clahe_params* clahe_or_null);
/* The contracts of the pmv_* calls of the same name, argument for argument and status code for status code, served by the class's combiner
 * in batched launches (LK and kNN: the LK combiners; the three detectors: the detector combiner). The slots must hold frames of a declared
 * size (else PMV_ERR_INVALID). */
int pmv_batch_lk_track(pmv_ctx* ctx, int prev_slot, int next_slot, const float* prev_xy, int n, float* out_xy, uint8_t* out_status, float* out_err);
/* pmv_lk_track_ex and pmv_lk_track_fb as session calls: same arguments, same checks, same bytes. A round of the LK combiner serves all its
 * extended requests with ONE launch on top of the k_lk_batch launch of its plain requests (counted in pmv_debug_batch_launches out4[0]); a
 * round without extended requests launches what it always did. An fb request counts n tracks against the round's capacity. The tracks go
 * in the engine's default order. */
int pmv_batch_lk_track_ex(pmv_ctx* ctx, int prev_slot, int next_slot, const float* prev_xy, int n, float* next_xy /* in/out */, int flags,
                          uint8_t* out_status, float* out_err);
int pmv_batch_lk_track_fb(pmv_ctx* ctx, int prev_slot, int next_slot, const float* prev_xy, int n, float* next_xy /* in/out */, int flags,
                          uint8_t* out_status, float* out_err, float* back_xy, uint8_t* back_status, float* back_err);
int pmv_batch_knn_match(pmv_ctx* ctx, int src_slot, int cmp_slot, const int* src_xy, int n, const int* cmp_xy, int m, int n_neighbours, int window,
                        int* out_best, float* out_err);
int pmv_batch_detect_gftt(pmv_ctx* ctx, int slot, const int* cells, int n_cells, int max_per_cell, double quality, double min_dist, int* out_xy,
                          int* out_count);
/* pmv_detect_gftt_ex as a session call: the same arguments, bits and status codes. Requests that agree in block_size, use_harris, k and
 * has-mask (and, as before, in quality, min_dist, max_per_cell and frame size) share a launch; a round without extended requests launches
 * what it launched before. The mask is read before the call returns. */
int pmv_batch_detect_gftt_ex(pmv_ctx* ctx, int slot, const int* cells, int n_cells, int max_per_cell, const pmv_gftt_params* p, const uint8_t* mask,
                             int mask_stride, int* out_xy, int* out_count);
/* pmv_detect_gftt_frame as a session call: the same arguments, bytes and status codes, served by the detector combiner. The frame requests
 * of a round share ONE pass-1 launch and ONE pass-2 launch if they agree in block_size, use_harris, k, has-mask, quality, min_dist, cap, the
 * no-limit flag and the frame layout (the grouping rules of pmv_batch_detect_gftt_ex): each request's records sit at their own offset and
 * pass 2 runs one workgroup per request. A round without frame requests launches exactly what it launched before. The mask is read before
 * the call returns; record space grows to the largest round seen. */
int pmv_batch_detect_gftt_frame(pmv_ctx* ctx, int slot, const int* roi4_or_null, int max_corners, const pmv_gftt_params* p,
                                const uint8_t* mask, int mask_stride, int* out_xy, int out_cap, int* out_count);
/* pmv_detect_gftt_refill as a session call: the same arguments, bytes and status codes. It is a frame request that carries a track list:
 * it joins the frame groups of its round under the rules above with has-mask = true, and the round makes ONE k_track_select and ONE
 * k_track_paint launch for all its refill requests, in front of the frame launches - each request names its own n, radius, half-width
 * table and mask offset. A round without refill requests launches and allocates exactly what it did before. The track list and the base
 * mask are read before the call returns. */
int pmv_batch_detect_gftt_refill(pmv_ctx* ctx, int slot, const int* roi4_or_null, int max_corners, const pmv_gftt_params* p,
                                 const float* track_xy, const int* track_prio_or_null, int n_tracks, int radius,
                                 const uint8_t* base_mask_or_null, int base_stride,
                                 uint8_t* out_keep, int* out_xy, int out_cap, int* out_count);
/* pmv_corner_subpix as a session call: the same arguments, bits and status codes. It is served by the detector combiner: requests of a
 * round that agree in the six parameters share ONE launch, whatever their slots and declared frame sizes (every point's record names its
 * geometry); a round without such requests launches exactly what it launched before. A round's result block holds at least
 * n_seq * max_tracks points, as for LK: requests that do not fit wait for the next round. */
int pmv_batch_corner_subpix(pmv_ctx* ctx, int slot, float* xy, int n, const pmv_subpix_params* p, uint8_t* out_iters, uint8_t* out_flags);
int pmv_batch_detect_shitomasi(pmv_ctx* ctx, int slot, const int* cells, int n_cells, int max_per_cell, double quality, int* out_xy, double* out_score,
                               int* out_count);
int pmv_batch_detect_fast(pmv_ctx* ctx, int slot, const int* cells, int n_cells, int max_per_cell, int threshold, int nonmax, int* out_xy,
                          float* out_response, int* out_count);
/* The same for the back-end: `seq` (0 .. n_seq - 1, else PMV_ERR_INVALID) selects the workspace set; one outstanding call per seq and call.
 * pmv_batch_ba_solve runs in the context's current pmv_set_ba_mode; the calls are logged by pmv_record_enable like the single ones. */
int pmv_batch_pnp_ransac(pmv_ctx* ctx, int seq, const float* obj_xyz, const float* img_xy, int m, const double* K, double* rvec, double* tvec,
                         int iterations, float reproj_err, double confidence, int* out_inliers, int* out_n_inliers);
int pmv_batch_ba_solve(pmv_ctx* ctx, int seq, double* cams, int nc, double* pts, int np, const double* obs_xy, const int* cam_idx, const int* pt_idx,
                       int n_obs, const double* K, double huber_delta, int max_iterations, pmv_ba_summary* summary);
int pmv_batch_triangulate_candidates(pmv_ctx* ctx, int seq, const double* q1, const double* q2, int n, const double* P1x4, const uint8_t* mask_in,
                                     double* out_Q, uint8_t* out_mask, int* out_good);
int pmv_batch_fivepoint_hypotheses(pmv_ctx* ctx, int seq, const double* q1, const double* q2, int n, const int* samples, int n_hyp, float thr,
                                   double* models, int* n_models, int* counts);
/* The triangulator's two calls for a seq, argument for argument (rules above: the no-model convention, 0 <= n <= max_tracks else
 * PMV_ERR_CAPACITY, mask in/out of pmv_recover_pose) with `seq` (0 .. n_seq - 1, else PMV_ERR_INVALID) after the context; the bits of the
 * single calls. The five-point combiner serves a round of pmv_batch_find_essential_mat requests with ONE k_essential_ransac launch, one
 * workgroup per request, and a call returns as soon as ITS request is complete (the workgroup's last store is the request's completion
 * word): it does not wait for the slowest request of its round. One outstanding call per seq and call: the seq's next call may come at
 * once, also while the round it left is still running - it waits inside the library until that round has released the seq's request
 * record. pmv_batch_recover_pose is a request of the DLT combiner. */
int pmv_batch_find_essential_mat(pmv_ctx* ctx, int seq, const double* p1_xy, const double* p2_xy, int n, const double* K, double prob, double threshold,
                                 double* E9, uint8_t* mask, int* out_found, int* out_samples_drawn);
int pmv_batch_recover_pose(pmv_ctx* ctx, int seq, const double* E9, const double* p1_xy, const double* p2_xy, int n, const double* K, double* R9, double* t3,
                           uint8_t* mask, double* tri4n, int* out_good);
/* pmv_find_fundamental_mat for a seq, argument for argument (its rules: n >= 15 else PMV_ERR_DEGENERATE, n <= max_tracks else
 * PMV_ERR_CAPACITY, the no-model convention) with `seq` (0 .. n_seq - 1, else PMV_ERR_INVALID) after the context; the bits of the single call.
 * A request of the five-point combiner: a round serves all its fundamental requests with ONE k_fundamental_ransac launch, one workgroup per
 * request, on top of the launch for the round's essential requests, and a call returns as soon as ITS request is complete. One outstanding
 * call per seq and call, as for pmv_batch_find_essential_mat. */
int pmv_batch_find_fundamental_mat(pmv_ctx* ctx, int seq, const float* p1_xy, const float* p2_xy, int n, double threshold, double confidence,
                                   double* F9, uint8_t* mask, int* out_found, int* out_samples_drawn);
/* pmv_find_homography for a seq, argument for argument (its rules: n >= 4 else PMV_ERR_DEGENERATE, n <= max_tracks else PMV_ERR_CAPACITY,
 * the no-model convention) with `seq` (0 .. n_seq - 1, else PMV_ERR_INVALID) after the context; the bits of the single call. A request of the
 * five-point combiner: a round serves all its homography requests with ONE k_homography_ransac launch, one workgroup per request, beside the
 * launches for the round's fundamental and essential requests (pmv_debug_whole_rounds does not count it: pmv_debug_homography_launches),
 * and a call returns as soon as ITS request is complete. One outstanding call per seq and call, as for pmv_batch_find_essential_mat; the
 * seq's fundamental and homography calls share their staging blocks, so one of the two at a time. */
int pmv_batch_find_homography(pmv_ctx* ctx, int seq, const float* p1_xy, const float* p2_xy, int n, double threshold, double confidence, int max_iters,
                              double* H9, uint8_t* mask, int* out_found, int* out_samples_drawn);
/* pmv_triangulate_tracks for a seq, argument for argument (its rules, its capacities, its empty problems, which launch nothing and enter no
 * round) with `seq` (0 .. n_seq - 1, else PMV_ERR_INVALID) after the context; the bits of the single call. A request of the DLT combiner:
 * a round serves all its requests of this kind with ONE k_tri_tracks_batch launch, one row of 64-landmark workgroups per request, beside
 * the launch for the round's pmv_batch_triangulate_candidates / pmv_batch_recover_pose requests; the requests are counted under the "dlt"
 * role of pmv_batch_stats and the launches by pmv_debug_tri_tracks_launches. One outstanding call per seq and call. */
int pmv_batch_triangulate_tracks(pmv_ctx* ctx, int seq, const double* P3x4, int nc, const double* obs_xy, const int* cam_idx, const int* pt_idx, int n_obs,
                                 int np, const pmv_tri_params* p_or_null, double* out_xyz, uint8_t* out_status, double* out_err_or_null, int* out_good);
/* out4 = {upload rounds, frames uploaded, level-0 launches, pyrDown launches} since pmv_batch_open: level-0 launches <= 2 x rounds (+ 1 for a
 * round with pmv_batch_frame_upload_clahe requests: the in-place launch behind the equalisation; + 1 for a round with
 * pmv_batch_frame_upload_remap requests: the launch from the remap scratch), and the
 * pyrDown launches are the sum over the rounds of the levels above 0 of each round's tallest pyramid. */
int pmv_batch_upload_stats(pmv_ctx* ctx, long long* out4);
/* diagnostic: one record of 8 ints per upload round since pmv_batch_open (the first 65536 rounds), in order:
 * [0..4] frames of the round whose pyramid has 1, 2, 3, 4, 5 levels; [5] level-0 launches and [6] pyrDown launches the round made, counted
 * where they are made; [7] frames of the round that were read in place (the others came through the staging pool). Writes the first
 * min(capacity, rounds) records to out8 and returns the number of rounds recorded (capacity 0: only the count). */
int pmv_batch_upload_rounds(pmv_ctx* ctx, int* out8, int capacity);

void pmv_pipeline_free(pmv_pipeline_result* r);
/* Same, but the (host-container) teardown runs on a background thread; pmv_pipeline_drain() joins all of them. */
void pmv_pipeline_release(pmv_pipeline_result* r);
void pmv_pipeline_drain(void);
int pmv_pipeline_num_poses(const pmv_pipeline_result* r);
void pmv_pipeline_get_poses(const pmv_pipeline_result* r, double* out12); /* per pose: R row-major (9) then t (3) */
int pmv_pipeline_num_frames(const pmv_pipeline_result* r);
int pmv_pipeline_frame_feature_count(const pmv_pipeline_result* r, int k);
void pmv_pipeline_get_frame_features(const pmv_pipeline_result* r, int k, int* out3); /* (column,row,landmark id|-1) */
/* Run statistics: pmv_pipeline_stats_count() (= 25) doubles, in this order:
 *   [0] lk_calls [1] lk_points [2] detect_calls [3] pnp_calls [4] pnp_points [5] tri_calls [6] ba_calls [7] ba_obs [8] ba_points
 *   [9] heuristic_motion (frames whose pose came from motionHeuristics' fallback branch) [10] run seconds [11] init_offset
 *   [12] live landmarks at the end [13] scale; wall seconds per stage as seen by the calling host threads: [14] t_lk [15] t_detect
 *   [16] t_pnp [17] t_tri [18] t_ba [19] t_pnp_kernel [20] t_ba_kernel [21] t_tri_essential [22] t_tri_pose; [23] five-point
 *   RANSAC samples drawn [24] tri_ahead: two-view calls whose findEssentialMat + recoverPose had been computed ahead of the back-end
 *   by a helper thread (two-thread pipeline). The caller's buffer must hold pmv_pipeline_stats_count() doubles. */
int pmv_pipeline_stats_count(void);
void pmv_pipeline_get_stats(const pmv_pipeline_result* r, double* out25);

#ifdef __cplusplus
}
#endif
#endif
