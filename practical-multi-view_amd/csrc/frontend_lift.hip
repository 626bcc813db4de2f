// pmv_camera_*, pmv_undistort_points and pmv_project_points (contract: include/pmv_hip.h): the cameras of the context - one small device
// table of LiftCam entries, made by the first pmv_camera_create and released with the last camera - and cv::undistortPoints as a single
// call: one launch of k_undistort_points on the front-end stream and one wait. The arithmetic is lift_point's (pmv_lift.h), which the
// tracker's stages 3 and 9 call too (frontend_klt.hip). pmv_project_points is the forward direction in the same shape: one launch of
// k_project_points (project_point, pmv_lift.h) and one wait. A camera is of the radial-tangential model (pmv_camera_create) or of
// cv::fisheye's equidistant one (pmv_camera_create_fisheye): one field of its LiftCam entry, which the two device functions branch on.
#include "pmv_ctx.h"
#include "pmv_lift.h"
#include <cmath>
#include <cstring>

namespace pmv {

namespace {
constexpr int LIFT_T = 256;
}

// one lane per point, FP64, no LDS; the camera entry is the launch's, so its loads are uniform
__global__ __launch_bounds__(LIFT_T) void k_undistort_points(const LiftCam* __restrict__ cam, const float* __restrict__ xy, int n, float* __restrict__ out_xy,
                                                             uint8_t* __restrict__ out_ok) {
    const int i = blockIdx.x * LIFT_T + threadIdx.x;
    if (i >= n) return;
    const LiftCam c = *cam;
    float x, y;
    const bool ok = lift_point_f(c, xy[2 * i], xy[2 * i + 1], &x, &y);
    out_xy[2 * i] = x; out_xy[2 * i + 1] = y;
    out_ok[i] = ok ? 1 : 0;
}

// one lane per point as above; the three doubles of a point are read as they lie (24 bytes a lane)
__global__ __launch_bounds__(LIFT_T) void k_project_points(const LiftCam* __restrict__ cam, const double* __restrict__ xyz, int n, float* __restrict__ out_xy,
                                                           uint8_t* __restrict__ out_ok) {
    const int i = blockIdx.x * LIFT_T + threadIdx.x;
    if (i >= n) return;
    const LiftCam c = *cam;
    float u, v;
    const bool ok = project_point(c, xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], &u, &v);
    out_xy[2 * i] = u; out_xy[2 * i + 1] = v;
    out_ok[i] = ok ? 1 : 0;
}

hipError_t launch_project_points(hipStream_t s, const LiftCam* cam, const double* d_xyz, int n, float* d_out_xy, uint8_t* d_ok) {
    if (!cam || !d_xyz || !d_out_xy || !d_ok || n < 1) return hipErrorInvalidValue;
    ProfScope ps(K_GFTT_PICK, s);
    hipLaunchKernelGGL(k_project_points, dim3((n + LIFT_T - 1) / LIFT_T), dim3(LIFT_T), 0, s, cam, d_xyz, n, d_out_xy, d_ok);
    return hipGetLastError();
}

hipError_t launch_undistort_points(hipStream_t s, const LiftCam* cam, const float* d_xy, int n, float* d_out_xy, uint8_t* d_ok) {
    if (!cam || !d_xy || !d_out_xy || !d_ok || n < 1) return hipErrorInvalidValue;
    ProfScope ps(K_GFTT_PICK, s);
    hipLaunchKernelGGL(k_undistort_points, dim3((n + LIFT_T - 1) / LIFT_T), dim3(LIFT_T), 0, s, cam, d_xy, n, d_out_xy, d_ok);
    return hipGetLastError();
}

const LiftCam* camera_entry(pmv_ctx* ctx, int id) {
    std::lock_guard<std::mutex> lk(ctx->cam_mu);
    if (id < 0 || id >= PMV_MAX_CAMERAS || !ctx->cam_used[id]) return nullptr;
    return ctx->d_cams.get() + id;
}

}  // namespace pmv

using namespace pmv;

#define CKC(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { set_err(ctx, "%s: %s", #x, hipGetErrorString(e_)); return PMV_ERR_HIP; } } while (0)
#define REQ(cond, code, ...) do { if (!(cond)) { set_err(ctx, __VA_ARGS__); return code; } } while (0)

// a validated camera record into the first free entry of the table (both constructors end here); `radtan` is what cam_params keeps for it
static int camera_place(pmv_ctx* ctx, const char* who, const LiftCam& c, const pmv_camera_params& radtan, int* out_id) {
    std::lock_guard<std::mutex> lk(ctx->cam_mu);
    int id = 0;
    while (id < PMV_MAX_CAMERAS && ctx->cam_used[id]) id++;
    REQ(id < PMV_MAX_CAMERAS, PMV_ERR_CAPACITY, "%s: the context holds %d cameras already (pmv_camera_destroy one)", who, PMV_MAX_CAMERAS);
    CKC(hipSetDevice(ctx->device));
    CKC(ctx->d_cams.ensure(PMV_MAX_CAMERAS * sizeof(LiftCam)));
    CKC(hipMemcpy(ctx->d_cams.get() + id, &c, sizeof(c), hipMemcpyHostToDevice));   // (no launch in flight reads a free entry)
    ctx->cam_used[id] = true;
    ctx->cam_params[id] = radtan;
    *out_id = id;
    return PMV_OK;
}

extern "C" {

int pmv_camera_create(pmv_ctx* ctx, const pmv_camera_params* p, int* out_id) {
    REQ(ctx, PMV_ERR_INVALID, "pmv_camera_create: null argument");
    REQ(p && out_id, PMV_ERR_INVALID, "pmv_camera_create: null argument");
    REQ(std::isfinite(p->fx) && std::isfinite(p->fy) && p->fx != 0.0 && p->fy != 0.0, PMV_ERR_INVALID, "pmv_camera_create: fx = %g, fy = %g: zero or not finite", p->fx, p->fy);
    REQ(std::isfinite(p->cx) && std::isfinite(p->cy), PMV_ERR_INVALID, "pmv_camera_create: cx = %g, cy = %g: not finite", p->cx, p->cy);
    for (int k = 0; k < 8; k++) REQ(std::isfinite(p->dist[k]), PMV_ERR_INVALID, "pmv_camera_create: dist[%d] = %g is not finite", k, p->dist[k]);
    REQ(p->iters >= 1 && p->iters <= 50, PMV_ERR_INVALID, "pmv_camera_create: iters = %d is outside 1..50", p->iters);
    LiftCam c{};
    c.cx = p->cx; c.cy = p->cy; c.ifx = 1.0 / p->fx; c.ify = 1.0 / p->fy; c.fx = p->fx; c.fy = p->fy;
    c.k1 = p->dist[0]; c.k2 = p->dist[1]; c.p1 = p->dist[2]; c.p2 = p->dist[3]; c.k3 = p->dist[4]; c.k4 = p->dist[5]; c.k5 = p->dist[6]; c.k6 = p->dist[7];
    c.iters = p->iters;
    REQ(std::isfinite(c.ifx) && std::isfinite(c.ify), PMV_ERR_INVALID, "pmv_camera_create: 1 / fx or 1 / fy is not finite (fx = %g, fy = %g)", p->fx, p->fy);
    return camera_place(ctx, "pmv_camera_create", c, *p, out_id);
}

int pmv_camera_create_fisheye(pmv_ctx* ctx, const pmv_fisheye_params* p, int* out_id) {
    REQ(ctx, PMV_ERR_INVALID, "pmv_camera_create_fisheye: null argument");
    REQ(p && out_id, PMV_ERR_INVALID, "pmv_camera_create_fisheye: null argument");
    REQ(std::isfinite(p->fx) && std::isfinite(p->fy) && p->fx != 0.0 && p->fy != 0.0, PMV_ERR_INVALID, "pmv_camera_create_fisheye: fx = %g, fy = %g: zero or not finite", p->fx, p->fy);
    REQ(std::isfinite(p->cx) && std::isfinite(p->cy), PMV_ERR_INVALID, "pmv_camera_create_fisheye: cx = %g, cy = %g: not finite", p->cx, p->cy);
    for (int k = 0; k < 4; k++) REQ(std::isfinite(p->k[k]), PMV_ERR_INVALID, "pmv_camera_create_fisheye: k[%d] = %g is not finite", k, p->k[k]);
    LiftCam c{};
    c.cx = p->cx; c.cy = p->cy; c.ifx = 1.0 / p->fx; c.ify = 1.0 / p->fy; c.fx = p->fx; c.fy = p->fy;
    c.k1 = p->k[0]; c.k2 = p->k[1]; c.k3 = p->k[2]; c.k4 = p->k[3];
    c.iters = 10; c.model = LIFT_FISHEYE;   // (the Newton loop's bound is fisheye_lift's own; iters is not read)
    REQ(std::isfinite(c.ifx) && std::isfinite(c.ify), PMV_ERR_INVALID, "pmv_camera_create_fisheye: 1 / fx or 1 / fy is not finite (fx = %g, fy = %g)", p->fx, p->fy);
    return camera_place(ctx, "pmv_camera_create_fisheye", c, pmv_camera_params{}, out_id);   // (no radial-tangential record goes with the entry)
}

int pmv_camera_destroy(pmv_ctx* ctx, int id) {
    REQ(ctx, PMV_ERR_INVALID, "pmv_camera_destroy: null argument");
    REQ(!klt_camera_in_use(ctx, id), PMV_ERR_INVALID, "pmv_camera_destroy: camera %d is named by a tracker's observation setting (clear it with pmv_klt_set_observe first)", id);
    REQ(!klt_camera_predicted(ctx, id), PMV_ERR_INVALID, "pmv_camera_destroy: camera %d is named by a tracker's pending prediction (step the tracker, or clear it with pmv_klt_set_prediction)", id);
    std::lock_guard<std::mutex> lk(ctx->cam_mu);
    REQ(id >= 0 && id < PMV_MAX_CAMERAS && ctx->cam_used[id], PMV_ERR_INVALID, "pmv_camera_destroy: camera %d does not exist", id);
    CKC(hipSetDevice(ctx->device));
    CKC(hipStreamSynchronize(ctx->s_front));
    ctx->cam_used[id] = false;
    bool any = false;
    for (int k = 0; k < PMV_MAX_CAMERAS; k++) any = any || ctx->cam_used[k];
    if (!any) { CKC(ctx->d_cams.release()); CKC(ctx->h_lift.release()); CKC(ctx->h_proj.release()); }   // the table and the single calls' blocks go with the last camera
    return PMV_OK;
}

int pmv_undistort_points(pmv_ctx* ctx, int cam_id, const float* xy, int n, float* out_xy, uint8_t* out_ok) {
    REQ(ctx, PMV_ERR_INVALID, "pmv_undistort_points: null argument");
    REQ(xy && out_xy && out_ok, PMV_ERR_INVALID, "pmv_undistort_points: null argument");
    REQ(n >= 0 && n <= ctx->max_tracks, PMV_ERR_CAPACITY, "pmv_undistort_points: n = %d is outside 0..%d (max_tracks)", n, ctx->max_tracks);
    const LiftCam* cam = camera_entry(ctx, cam_id);
    REQ(cam, PMV_ERR_INVALID, "pmv_undistort_points: camera %d does not exist (pmv_camera_create)", cam_id);
    for (int i = 0; i < 2 * n; i++)   // (a NaN fails the comparison too)
        REQ(fabsf(xy[i]) <= 1e6f, PMV_ERR_INVALID, "pmv_undistort_points: point %d (%g, %g) is not finite or beyond 1e6", i / 2, (double)xy[i & ~1], (double)xy[i | 1]);
    if (n == 0) return PMV_OK;
    tl_prof = &ctx->prof; CKC(hipSetDevice(ctx->device));
    // the call's block, mapped pinned, made by the first call: [points | lifted points | ok bytes], max_tracks of each
    const size_t nt = (size_t)ctx->max_tracks;
    Carve need;
    need.take<float>(2 * nt, 16); need.take<float>(2 * nt, 16); need.take<uint8_t>(nt, 16);
    CKC(ctx->h_lift.ensure(need.bytes()));
    Carve c = carve_of(ctx->h_lift);
    const Carved<float> in = c.take<float>(2 * nt, 16), out = c.take<float>(2 * nt, 16);
    const Carved<uint8_t> ok = c.take<uint8_t>(nt, 16);
    memcpy(in.h, xy, (size_t)n * 8);
    CKC(launch_undistort_points(ctx->s_front, cam, in.d, n, out.d, ok.d));
    CKC(hipStreamSynchronize(ctx->s_front));
    memcpy(out_xy, out.h, (size_t)n * 8);
    memcpy(out_ok, ok.h, (size_t)n);
    return PMV_OK;
}

int pmv_project_points(pmv_ctx* ctx, int cam_id, const double* xyz, int n, float* out_xy, uint8_t* out_ok) {
    REQ(ctx, PMV_ERR_INVALID, "pmv_project_points: null argument");
    REQ(xyz && out_xy && out_ok, PMV_ERR_INVALID, "pmv_project_points: null argument");
    REQ(n >= 0 && n <= ctx->max_tracks, PMV_ERR_CAPACITY, "pmv_project_points: n = %d is outside 0..%d (max_tracks)", n, ctx->max_tracks);
    const LiftCam* cam = camera_entry(ctx, cam_id);
    REQ(cam, PMV_ERR_INVALID, "pmv_project_points: camera %d does not exist (pmv_camera_create)", cam_id);
    if (n == 0) return PMV_OK;   // (a coordinate of any value is legal: a point that cannot be projected comes back with ok 0)
    tl_prof = &ctx->prof; CKC(hipSetDevice(ctx->device));
    // the call's block, mapped pinned, made by the first call: [camera-frame points | pixels | ok bytes], max_tracks of each
    const size_t nt = (size_t)ctx->max_tracks;
    Carve need;
    need.take<double>(3 * nt, 16); need.take<float>(2 * nt, 16); need.take<uint8_t>(nt, 16);
    CKC(ctx->h_proj.ensure(need.bytes()));
    Carve c = carve_of(ctx->h_proj);
    const Carved<double> in = c.take<double>(3 * nt, 16);
    const Carved<float> out = c.take<float>(2 * nt, 16);
    const Carved<uint8_t> ok = c.take<uint8_t>(nt, 16);
    memcpy(in.h, xyz, (size_t)n * 24);
    CKC(launch_project_points(ctx->s_front, cam, in.d, n, out.d, ok.d));
    CKC(hipStreamSynchronize(ctx->s_front));
    memcpy(out_xy, out.h, (size_t)n * 8);
    memcpy(out_ok, ok.h, (size_t)n);
    return PMV_OK;
}

}  // extern "C"
