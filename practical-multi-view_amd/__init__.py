"""practical-multi-view_amd — MI355X (gfx950) visual-odometry hot path behind the reference's plugin roles.

Python here is plumbing only: a ctypes binding of the C ABI in include/pmv_hip.h (the product is the HIP library
`libpmv_hip.so` built by build.py) plus thin mirrors of the reference's plugin roles used by tests and bench.py.
There is NO CPU fallback: creating a Context without a gfx950 device raises.
"""
import ctypes as C
import os

import numpy as np

from . import build as _build

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

_u8p = C.POINTER(C.c_uint8)
_i32p = C.POINTER(C.c_int)
_f32p = C.POINTER(C.c_float)
_f64p = C.POINTER(C.c_double)


class PmvError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"pmv error {code}: {msg}")
        self.code = code


class BaSummary(C.Structure):
    _fields_ = [("initial_cost", C.c_double), ("final_cost", C.c_double), ("iterations", C.c_int),
                ("successful_steps", C.c_int), ("termination", C.c_int)]


class LKParams(C.Structure):
    """pmv_lk_params of include/pmv_hip.h"""
    _fields_ = [("win", C.c_int), ("max_level", C.c_int), ("max_iter", C.c_int), ("eps", C.c_double), ("min_eig", C.c_float)]


class GfttParams(C.Structure):
    """pmv_gftt_params of include/pmv_hip.h"""
    _fields_ = [("quality", C.c_double), ("min_dist", C.c_double), ("block_size", C.c_int), ("use_harris", C.c_int), ("k", C.c_double)]


class SubpixParams(C.Structure):
    """pmv_subpix_params of include/pmv_hip.h"""
    _fields_ = [("win_w", C.c_int), ("win_h", C.c_int), ("zero_w", C.c_int), ("zero_h", C.c_int), ("max_iter", C.c_int), ("eps", C.c_double)]


class ClaheParams(C.Structure):
    """pmv_clahe_params of include/pmv_hip.h"""
    _fields_ = [("clip_limit", C.c_double), ("tiles_x", C.c_int), ("tiles_y", C.c_int)]


class TriParams(C.Structure):
    """pmv_tri_params of include/pmv_hip.h; the defaults are the call's (a null pointer): VINS-Mono's triangulate with its depth test"""
    _fields_ = [("min_views", C.c_int), ("refine_iters", C.c_int), ("min_depth", C.c_double), ("max_depth", C.c_double), ("max_reproj", C.c_double),
                ("min_parallax_deg", C.c_double)]

    def __init__(self, min_views=2, refine_iters=0, min_depth=0.1, max_depth=float("inf"), max_reproj=float("inf"), min_parallax_deg=0.0):
        super().__init__(int(min_views), int(refine_iters), float(min_depth), float(max_depth), float(max_reproj), float(min_parallax_deg))


# status bits of pmv_triangulate_tracks (PMV_TRI_* of include/pmv_hip.h); 0 = accepted
TRI_OK, TRI_FEW_VIEWS, TRI_DEGENERATE, TRI_DEPTH, TRI_REPROJ, TRI_PARALLAX = 0, 1, 2, 4, 8, 16


def projections_from_ba_cams(cams, K=None):
    """The projection matrices (nc, 3, 4) of pmv_triangulate_tracks for cameras in pmv_ba_solve's form, cam = [angle-axis w, c]: p = R(w) (X + c),
    depth pz = -p[2], u = fx p[0] / pz + cx, v = fy p[1] / pz + cy. Their projections have zero ProjectionResidual for that form and their third
    row gives pz. K (3, 3) for pixel observations; None for normalised ones (fx = fy = 1, cx = cy = 0)."""
    cams = np.ascontiguousarray(cams, np.float64).reshape(-1, 6)
    Kd = np.eye(3) if K is None else np.ascontiguousarray(K, np.float64).reshape(3, 3)
    Kn = np.array([[Kd[0, 0], 0.0, -Kd[0, 2]], [0.0, Kd[1, 1], -Kd[1, 2]], [0.0, 0.0, -1.0]])
    out = np.zeros((len(cams), 3, 4))
    for i, cam in enumerate(cams):
        w, th2 = cam[:3], float(cam[:3] @ cam[:3])
        Wx = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
        if th2 > np.finfo(np.float64).eps:
            th = np.sqrt(th2)
            R = np.eye(3) + np.sin(th) / th * Wx + (1.0 - np.cos(th)) / th2 * (Wx @ Wx)
        else:
            R = np.eye(3) + Wx   # (the first-order form ProjectionResidual's rotation takes near zero)
        out[i] = Kn @ np.c_[R, R @ cam[3:]]
    return out


KLT_MAX_TRACKERS = 16   # PMV_KLT_MAX_TRACKERS of include/pmv_hip.h


class KltParams(C.Structure):
    """pmv_klt_params of include/pmv_hip.h"""
    _fields_ = [("target", C.c_int), ("border", C.c_int), ("fb_max_dist", C.c_double), ("reject_f", C.c_int), ("f_threshold", C.c_double),
                ("f_confidence", C.c_double), ("radius", C.c_int), ("gftt", GfttParams), ("subpix", C.c_int), ("subpix_params", SubpixParams)]


def klt_params(target=150, border=1, fb_max_dist=0.5, reject_f=True, f_threshold=1.0, f_confidence=0.99, radius=10, quality=0.01, min_dist=10.0, block_size=3,
               use_harris=False, k=0.04, subpix=False, subpix_win=(5, 5), subpix_zero_zone=(-1, -1), subpix_max_iter=30, subpix_eps=0.01):
    """a KltParams from keywords; the defaults are a VINS-style front end's (MAX_CNT 150, BORDER_SIZE 1, F_THRESHOLD 1.0, MIN_DIST 10).
    fb_max_dist None or negative: no backward pass."""
    return KltParams(int(target), int(border), -1.0 if fb_max_dist is None else float(fb_max_dist), int(reject_f), float(f_threshold), float(f_confidence), int(radius),
                     GfttParams(float(quality), float(min_dist), int(block_size), 1 if use_harris else 0, float(k)), int(subpix),
                     SubpixParams(int(subpix_win[0]), int(subpix_win[1]), int(subpix_zero_zone[0]), int(subpix_zero_zone[1]), int(subpix_max_iter), float(subpix_eps)))


class KltStereoParams(C.Structure):
    """pmv_klt_stereo_params of include/pmv_hip.h"""
    _fields_ = [("fb_max_dist", C.c_double), ("border", C.c_int)]


class CameraParams(C.Structure):
    """pmv_camera_params of include/pmv_hip.h"""
    _fields_ = [("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double), ("dist", C.c_double * 8), ("iters", C.c_int)]


def camera_params(fx, fy, cx, cy, dist=(), iters=5):
    """a CameraParams from keywords; dist: up to 8 coefficients (k1, k2, p1, p2, k3, k4, k5, k6), the missing ones 0"""
    d = np.asarray(dist, np.float64).reshape(-1)
    if d.size > 8:
        raise ValueError(f"camera_params: at most 8 distortion coefficients (k1, k2, p1, p2, k3, k4, k5, k6), got {d.size}")
    p = CameraParams(float(fx), float(fy), float(cx), float(cy))
    for k, v in enumerate(d):
        p.dist[k] = float(v)
    p.iters = int(iters)
    return p


class FisheyeParams(C.Structure):
    """pmv_fisheye_params of include/pmv_hip.h"""
    _fields_ = [("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double), ("k", C.c_double * 4)]


def fisheye_params(fx, fy, cx, cy, k=()):
    """a FisheyeParams from keywords; k: up to 4 coefficients (k1, k2, k3, k4) of the equidistant model (cv::fisheye, Kalibr "equidistant"),
    the missing ones 0"""
    d = np.asarray(k, np.float64).reshape(-1)
    if d.size > 4:
        raise ValueError(f"fisheye_params: at most 4 distortion coefficients (k1, k2, k3, k4), got {d.size}")
    p = FisheyeParams(float(fx), float(fy), float(cx), float(cy))
    for i, v in enumerate(d):
        p.k[i] = float(v)
    return p


class KltObserveParams(C.Structure):
    """pmv_klt_observe_params of include/pmv_hip.h"""
    _fields_ = [("cam_id", C.c_int), ("right_cam_id", C.c_int), ("dt", C.c_double), ("undistorted_f", C.c_int), ("f_focal", C.c_double)]


class KltPredictParams(C.Structure):
    """pmv_klt_predict_params of include/pmv_hip.h"""
    _fields_ = [("cam_id", C.c_int), ("top_level", C.c_int), ("back_top_level", C.c_int), ("min_succ", C.c_int)]


class KltTracker:
    """A tracker of Context.klt_create. The state - ids, ages, positions - lives in device memory; step() returns the new list."""

    def __init__(self, ctx, tid, target):
        self.ctx, self.id, self.target = ctx, tid, target

    def step(self, prev_slot, cur_slot):
        """pmv_klt_step: (ids (n,) int32, ages (n,) int32, xy (n, 2) float32, prev_xy (n, 2) float32, counts (8,) int32 = n0, n1, n2, n3, m,
        f_found (-1: not run), f_samples_drawn, 0)"""
        ctx, cap = self.ctx, self.target
        ids, ages = np.zeros(cap, np.int32), np.zeros(cap, np.int32)
        xy, prev = np.zeros((cap, 2), np.float32), np.zeros((cap, 2), np.float32)
        counts = np.zeros(8, np.int32)
        n = C.c_int(0)
        fn = ctx.lib.pmv_klt_step
        fn.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, _i32p, _i32p, _f32p, _f32p, C.c_int, C.POINTER(C.c_int), _i32p]
        ctx._ck(fn(ctx.h, self.id, int(prev_slot), int(cur_slot), _p(ids, _i32p), _p(ages, _i32p), _p(xy, _f32p), _p(prev, _f32p), cap, C.byref(n), _p(counts, _i32p)))
        k = n.value
        return ids[:k].copy(), ages[:k].copy(), xy[:k].copy(), prev[:k].copy(), counts

    def set_stereo(self, fb_max_dist=0.5, border=1):
        """pmv_klt_set_stereo: the setting of step_stereo's stage 8 - the forward-backward distance of the left-to-right LK (negative: no
        backward pass) and the border of the right frame. fb_max_dist=None turns the setting off."""
        fn = self.ctx.lib.pmv_klt_set_stereo
        fn.argtypes = [C.c_void_p, C.c_int, C.POINTER(KltStereoParams)]
        if fb_max_dist is None:
            self.ctx._ck(fn(self.ctx.h, self.id, None))
            return
        p = KltStereoParams(float(fb_max_dist), int(border))
        self.ctx._ck(fn(self.ctx.h, self.id, C.byref(p)))

    def get_stereo(self):
        """pmv_klt_get_stereo: (fb_max_dist, border) of the stereo setting, or None when it is off"""
        p, on = KltStereoParams(), C.c_int(0)
        fn = self.ctx.lib.pmv_klt_get_stereo
        fn.argtypes = [C.c_void_p, C.c_int, C.POINTER(KltStereoParams), C.POINTER(C.c_int)]
        self.ctx._ck(fn(self.ctx.h, self.id, C.byref(p), C.byref(on)))
        return (p.fb_max_dist, p.border) if on.value else None

    def step_stereo(self, prev_slot, cur_slot, right_slot):
        """pmv_klt_step_stereo: step()'s 5-tuple (counts[7] = the number of matched tracks), then right_xy (n, 2) float32 - where LK from
        cur_slot into right_slot put every track of the list - and right_status (n,) uint8, 1 for the tracks that have a right observation"""
        ctx, cap = self.ctx, self.target
        ids, ages = np.zeros(cap, np.int32), np.zeros(cap, np.int32)
        xy, prev, rxy = np.zeros((cap, 2), np.float32), np.zeros((cap, 2), np.float32), np.zeros((cap, 2), np.float32)
        rst = np.zeros(cap, np.uint8)
        counts = np.zeros(8, np.int32)
        n = C.c_int(0)
        fn = ctx.lib.pmv_klt_step_stereo
        fn.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, _i32p, _i32p, _f32p, _f32p, _f32p, _u8p, C.c_int, C.POINTER(C.c_int), _i32p]
        ctx._ck(fn(ctx.h, self.id, int(prev_slot), int(cur_slot), int(right_slot), _p(ids, _i32p), _p(ages, _i32p), _p(xy, _f32p), _p(prev, _f32p), _p(rxy, _f32p),
                   _p(rst, _u8p), cap, C.byref(n), _p(counts, _i32p)))
        k = n.value
        return ids[:k].copy(), ages[:k].copy(), xy[:k].copy(), prev[:k].copy(), counts, rxy[:k].copy(), rst[:k].copy()

    def set_observe(self, cam_id, right_cam_id=-1, dt=1.0, undistorted_f=False, f_focal=460.0):
        """pmv_klt_set_observe: the setting of stage 9 - the left camera (Context.camera_create), the right camera or -1, the seconds between
        the previous and this frame - and of stage 3 on undistorted points (undistorted_f, f_focal). cam_id=None turns the setting off."""
        fn = self.ctx.lib.pmv_klt_set_observe
        fn.argtypes = [C.c_void_p, C.c_int, C.POINTER(KltObserveParams)]
        if cam_id is None:
            self.ctx._ck(fn(self.ctx.h, self.id, None))
            return
        p = KltObserveParams(int(cam_id), int(right_cam_id), float(dt), int(undistorted_f), float(f_focal))
        self.ctx._ck(fn(self.ctx.h, self.id, C.byref(p)))

    def get_observe(self):
        """pmv_klt_get_observe: dict(cam_id, right_cam_id, dt, undistorted_f, f_focal) of the observation setting, or None when it is off"""
        p, on = KltObserveParams(), C.c_int(0)
        fn = self.ctx.lib.pmv_klt_get_observe
        fn.argtypes = [C.c_void_p, C.c_int, C.POINTER(KltObserveParams), C.POINTER(C.c_int)]
        self.ctx._ck(fn(self.ctx.h, self.id, C.byref(p), C.byref(on)))
        return dict(cam_id=p.cam_id, right_cam_id=p.right_cam_id, dt=p.dt, undistorted_f=bool(p.undistorted_f), f_focal=p.f_focal) if on.value else None

    def get_observations(self):
        """pmv_klt_get_observations, after a step with the observation setting on: (un_xy (n, 2) float32 - the list's positions on the
        normalised image plane, vel (n, 2) float32 - their velocities there, ok (n,) uint8, right_un_xy (n, 2) float32, right_ok (n,) uint8);
        without right observations in that step right_ok is all 0 and right_un_xy zeros"""
        cap = self.target
        un, vel, run = np.zeros((cap, 2), np.float32), np.zeros((cap, 2), np.float32), np.zeros((cap, 2), np.float32)
        ok, rok = np.zeros(cap, np.uint8), np.zeros(cap, np.uint8)
        n = C.c_int(0)
        fn = self.ctx.lib.pmv_klt_get_observations
        fn.argtypes = [C.c_void_p, C.c_int, _f32p, _f32p, _u8p, _f32p, _u8p, C.c_int, C.POINTER(C.c_int)]
        self.ctx._ck(fn(self.ctx.h, self.id, _p(un, _f32p), _p(vel, _f32p), _p(ok, _u8p), _p(run, _f32p), _p(rok, _u8p), cap, C.byref(n)))
        k = n.value
        return un[:k].copy(), vel[:k].copy(), ok[:k].copy(), run[:k].copy(), rok[:k].copy()

    def set_prediction(self, cam_id, ids=None, xyz=None, top_level=1, back_top_level=1, min_succ=10):
        """pmv_klt_set_prediction: a one-shot prediction for the tracker's next step - xyz (n, 3) float64, the points with track ids `ids` in
        the frame of camera cam_id (Context.camera_create) at the NEW image. The step projects them, starts LK of the tracks they belong to
        there on pyramid levels 0 .. top_level, runs its backward pass on levels 0 .. back_top_level (-1: all) and falls back to the full
        pyramid if fewer than min_succ tracks succeed. cam_id=None (or no point) clears a pending prediction."""
        fn = self.ctx.lib.pmv_klt_set_prediction
        fn.argtypes = [C.c_void_p, C.c_int, C.POINTER(KltPredictParams), _i32p, C.POINTER(C.c_double), C.c_int]
        if cam_id is None:
            self.ctx._ck(fn(self.ctx.h, self.id, None, None, None, 0))
            return
        ids = np.ascontiguousarray(ids if ids is not None else [], np.int32).reshape(-1)
        xyz = np.ascontiguousarray(xyz if xyz is not None else np.zeros((0, 3)), np.float64)
        if xyz.size and (xyz.ndim != 2 or xyz.shape[1] != 3):
            raise ValueError("set_prediction: xyz must be an (n, 3) float64 array")
        n = xyz.size // 3
        if ids.size != n:
            raise ValueError("set_prediction: one id per point")
        p = KltPredictParams(int(cam_id), int(top_level), int(back_top_level), int(min_succ))
        self.ctx._ck(fn(self.ctx.h, self.id, C.byref(p), _p(ids, _i32p) if n else None, _p(xyz, C.POINTER(C.c_double)) if n else None, n))

    def get_prediction_result(self):
        """pmv_klt_get_prediction_result: dict(consumed, joined, succ, fell_back) of the tracker's last step"""
        out = (C.c_int * 4)()
        fn = self.ctx.lib.pmv_klt_get_prediction_result
        fn.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int)]
        self.ctx._ck(fn(self.ctx.h, self.id, out))
        return dict(consumed=int(out[0]), joined=int(out[1]), succ=int(out[2]), fell_back=int(out[3]))

    def set_tracks(self, ids, ages, xy, next_id):
        """pmv_klt_set_tracks: replace the state"""
        ids, ages = np.ascontiguousarray(ids, np.int32).reshape(-1), np.ascontiguousarray(ages, np.int32).reshape(-1)
        xy = np.ascontiguousarray(xy, np.float32)
        if xy.size and (xy.ndim != 2 or xy.shape[1] != 2):
            raise ValueError("set_tracks: xy must be an (n, 2) float32 array")
        n = xy.size // 2
        if ids.size != n or ages.size != n:
            raise ValueError("set_tracks: one id and one age per track")
        fn = self.ctx.lib.pmv_klt_set_tracks
        fn.argtypes = [C.c_void_p, C.c_int, _i32p, _i32p, _f32p, C.c_int, C.c_int]
        self.ctx._ck(fn(self.ctx.h, self.id, _p(ids, _i32p) if n else None, _p(ages, _i32p) if n else None, _p(xy, _f32p) if n else None, n, int(next_id)))

    def get_tracks(self):
        """pmv_klt_get_tracks: (ids, ages, xy) of the state"""
        cap = self.target
        ids, ages, xy = np.zeros(cap, np.int32), np.zeros(cap, np.int32), np.zeros((cap, 2), np.float32)
        n = C.c_int(0)
        fn = self.ctx.lib.pmv_klt_get_tracks
        fn.argtypes = [C.c_void_p, C.c_int, _i32p, _i32p, _f32p, C.c_int, C.POINTER(C.c_int)]
        self.ctx._ck(fn(self.ctx.h, self.id, _p(ids, _i32p), _p(ages, _i32p), _p(xy, _f32p), cap, C.byref(n)))
        return ids[: n.value].copy(), ages[: n.value].copy(), xy[: n.value].copy()

    def close(self):
        """pmv_klt_destroy"""
        if self.id is not None and self.ctx.h:
            self.ctx.lib.pmv_klt_destroy.argtypes = [C.c_void_p, C.c_int]
            self.ctx._ck(self.ctx.lib.pmv_klt_destroy(self.ctx.h, self.id))
        self.id = None


def _clahe_params(who, clip_limit, tiles):
    # refused before the library is touched: what the struct cannot hold as the caller meant it
    if isinstance(clip_limit, (bool, np.bool_)) or not isinstance(clip_limit, (int, float, np.integer, np.floating)):
        raise ValueError(f"{who}: clip_limit must be a number, got {clip_limit!r}")
    try:
        tx, ty = tiles
    except (TypeError, ValueError):
        raise ValueError(f"{who}: tiles is a (tiles_x, tiles_y) pair, got {tiles!r}") from None
    for t in (tx, ty):
        if isinstance(t, (bool, np.bool_)) or not isinstance(t, (int, np.integer)):
            raise ValueError(f"{who}: tiles is a pair of integers, got {tiles!r}")
    return ClaheParams(float(clip_limit), int(tx), int(ty))


PREPROC_MAX_MAPS = 8   # PMV_PREPROC_MAX_MAPS of include/pmv_hip.h


class FramePreproc(C.Structure):
    """pmv_frame_preproc of include/pmv_hip.h"""
    _fields_ = [("n_maps", C.c_int), ("map_ids", C.c_int * PREPROC_MAX_MAPS), ("border_value", C.c_int), ("clahe", C.c_int), ("clahe_params", ClaheParams)]


def _preproc_arg(who, remap, border_value, clahe):
    """set_frame_preproc's arguments as a FramePreproc, or None when everything is off; wrong types and ranges are refused here"""
    def is_int(v):
        return isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_))
    if remap is None:
        ids = []
    elif is_int(remap):
        ids = [int(remap)]
    else:
        try:
            ids = list(remap)
        except TypeError:
            raise ValueError(f"{who}: remap is a map id or a sequence of map ids, got {remap!r}") from None
        if isinstance(remap, (str, bytes)) or not all(is_int(i) for i in ids):
            raise ValueError(f"{who}: remap is a map id or a sequence of integer map ids, got {remap!r}")
        ids = [int(i) for i in ids]
    if len(ids) > PREPROC_MAX_MAPS:
        raise ValueError(f"{who}: at most {PREPROC_MAX_MAPS} maps, got {len(ids)}")
    if not is_int(border_value) or not 0 <= int(border_value) <= 255:
        raise ValueError(f"{who}: border_value is an integer in 0..255, got {border_value!r}")
    p = FramePreproc()
    p.n_maps = len(ids)
    for k, i in enumerate(ids):
        p.map_ids[k] = i
    p.border_value = int(border_value)
    if clahe is not None:
        try:
            clip, tiles = clahe
        except (TypeError, ValueError):
            raise ValueError(f"{who}: clahe is None or (clip_limit, (tiles_x, tiles_y)), got {clahe!r}") from None
        cp = _clahe_params(who, clip, tiles)
        if not (cp.clip_limit >= 0.0 and np.isfinite(cp.clip_limit)):
            raise ValueError(f"{who}: clip_limit is a finite number >= 0, got {clip!r}")
        if not (1 <= cp.tiles_x <= 16 and 1 <= cp.tiles_y <= 16):
            raise ValueError(f"{who}: tiles are in 1..16 each, got {tiles!r}")
        p.clahe = 1
        p.clahe_params = cp
    if not ids and clahe is None and int(border_value) == 0:
        return None
    return p


def _remap_arg(who, remap):
    """remap= of the session upload: a map id, or (map_id, border_value)"""
    def is_int(v):
        return isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_))
    if is_int(remap):
        return int(remap), 0
    try:
        map_id, border = remap
    except (TypeError, ValueError):
        raise ValueError(f"{who}: remap is a map id or (map_id, border_value), got {remap!r}") from None
    if not is_int(map_id) or not is_int(border):
        raise ValueError(f"{who}: remap is a map id or (map_id, border_value) of integers, got {remap!r}")
    return int(map_id), int(border)


def undistort_map(K, dist, size, R=None, new_K=None):
    """pmv_undistort_map_build: the (map_x, map_y) float32 (h, w) maps of cv::initUndistortRectifyMap(K, dist, R, new_K, size, CV_32FC1), on
    the host. dist: up to 8 coefficients (k1, k2, p1, p2, k3, k4, k5, k6), the missing ones 0; size = (w, h); R None = identity, new_K None = K."""
    def mat(m, name):
        a = np.ascontiguousarray(m, np.float64)
        if a.shape != (3, 3):
            raise ValueError(f"undistort_map: {name} is 3 x 3, got shape {a.shape}")
        return a
    Km = mat(K, "K")
    d = np.asarray(dist, np.float64).reshape(-1)
    if d.size > 8:
        raise ValueError(f"undistort_map: at most 8 distortion coefficients (k1, k2, p1, p2, k3, k4, k5, k6), got {d.size}")
    d8 = np.zeros(8, np.float64)
    d8[:d.size] = d
    try:
        w, h = size
    except (TypeError, ValueError):
        raise ValueError(f"undistort_map: size is (w, h), got {size!r}") from None
    w, h = int(w), int(h)
    if w < 1 or h < 1:
        raise ValueError(f"undistort_map: size {size!r}")
    Rm = None if R is None else mat(R, "R")
    Nm = None if new_K is None else mat(new_K, "new_K")
    mx, my = np.empty((h, w), np.float32), np.empty((h, w), np.float32)
    lib = load_library()
    _f32p = C.POINTER(C.c_float)
    lib.pmv_undistort_map_build.argtypes = [_f64p, _f64p, _f64p, _f64p, C.c_int, C.c_int, _f32p, _f32p]
    rc = lib.pmv_undistort_map_build(_p(Km, _f64p), _p(d8, _f64p), None if Rm is None else _p(Rm, _f64p), None if Nm is None else _p(Nm, _f64p), w, h,
                                     _p(mx, _f32p), _p(my, _f32p))
    if rc != 0:
        raise PmvError(rc, lib.pmv_last_error(None).decode())
    return mx, my


def fisheye_map_build(K, k, size, R=None, new_K=None):
    """pmv_fisheye_map_build: the (map_x, map_y) float32 (h, w) maps of cv::fisheye::initUndistortRectifyMap(K, k, R, new_K, size, CV_32FC1),
    on the host. k: up to 4 coefficients (k1, k2, k3, k4), the missing ones 0; size = (w, h); R None = identity, new_K None = K. A pixel whose
    ray the model refuses has (-1, -1)."""
    def mat(m, name):
        a = np.ascontiguousarray(m, np.float64)
        if a.shape != (3, 3):
            raise ValueError(f"fisheye_map_build: {name} is 3 x 3, got shape {a.shape}")
        return a
    Km = mat(K, "K")
    d = np.asarray(k, np.float64).reshape(-1)
    if d.size > 4:
        raise ValueError(f"fisheye_map_build: at most 4 distortion coefficients (k1, k2, k3, k4), got {d.size}")
    k4 = np.zeros(4, np.float64)
    k4[:d.size] = d
    try:
        w, h = size
    except (TypeError, ValueError):
        raise ValueError(f"fisheye_map_build: size is (w, h), got {size!r}") from None
    w, h = int(w), int(h)
    if w < 1 or h < 1:
        raise ValueError(f"fisheye_map_build: size {size!r}")
    Rm = None if R is None else mat(R, "R")
    Nm = None if new_K is None else mat(new_K, "new_K")
    mx, my = np.empty((h, w), np.float32), np.empty((h, w), np.float32)
    lib = load_library()
    _f32p = C.POINTER(C.c_float)
    lib.pmv_fisheye_map_build.argtypes = [_f64p, _f64p, _f64p, _f64p, C.c_int, C.c_int, _f32p, _f32p]
    rc = lib.pmv_fisheye_map_build(_p(Km, _f64p), _p(k4, _f64p), None if Rm is None else _p(Rm, _f64p), None if Nm is None else _p(Nm, _f64p), w, h,
                                   _p(mx, _f32p), _p(my, _f32p))
    if rc != 0:
        raise PmvError(rc, lib.pmv_last_error(None).decode())
    return mx, my


def mem_live():
    """pmv_debug_mem_live: (device bytes, pinned host bytes) the library holds right now, over every context of the process"""
    lib = load_library()
    out = (C.c_longlong * 2)()
    lib.pmv_debug_mem_live.argtypes = [C.POINTER(C.c_longlong)]
    rc = lib.pmv_debug_mem_live(out)
    if rc != 0:
        raise PmvError(rc, lib.pmv_last_error(None).decode())
    return int(out[0]), int(out[1])


# every symbol include/pmv_hip.h declares (tests check the library exports all of them)
# the `flags` of pmv_lk_track_ex / pmv_lk_track_fb (cv's values)
LK_USE_INITIAL_FLOW = 4
LK_GET_MIN_EIGENVALS = 8

ABI_SYMBOLS = [
    "pmv_ctx_create", "pmv_ctx_destroy", "pmv_last_error", "pmv_thread_error", "pmv_sync",
    "pmv_frame_upload", "pmv_frame_upload_bgr", "pmv_set_frame_format", "pmv_frames_stage", "pmv_frames_build", "pmv_frames_stream_begin", "pmv_frames_stream_end", "pmv_frame_get_level", "pmv_frame_get_level_padded", "pmv_frame_num_levels",
    "pmv_detect_gftt", "pmv_detect_shitomasi", "pmv_detect_fast", "pmv_knn_match", "pmv_debug_gftt_response", "pmv_debug_shitomasi_response",
    "pmv_detect_gftt_ex", "pmv_debug_gftt_response_ex", "pmv_debug_gftt_general", "pmv_batch_detect_gftt_ex",
    "pmv_detect_gftt_frame", "pmv_batch_detect_gftt_frame", "pmv_debug_gftt_frame_stats",
    "pmv_detect_gftt_refill", "pmv_batch_detect_gftt_refill", "pmv_debug_refill_mask", "pmv_debug_refill_stats",
    "pmv_corner_subpix", "pmv_batch_corner_subpix", "pmv_debug_subpix_launches",
    "pmv_frames_clahe", "pmv_batch_frame_upload_clahe", "pmv_debug_clahe_launches",
    "pmv_remap_map_create", "pmv_remap_map_destroy", "pmv_frames_remap", "pmv_debug_remap_launches", "pmv_batch_frame_upload_remap", "pmv_undistort_map_build",
    "pmv_set_frame_preproc", "pmv_get_frame_preproc", "pmv_debug_preproc_launches",
    "pmv_debug_mem_live",
    "pmv_lk_track", "pmv_lk_track_ex", "pmv_lk_track_fb", "pmv_lk_track_fb_levels", "pmv_set_lk_params", "pmv_get_lk_params", "pmv_debug_lk_general", "pmv_set_ba_mode", "pmv_pnp_ransac", "pmv_debug_pnp_hypotheses", "pmv_debug_ba_stamps", "pmv_debug_lk_stamps", "pmv_ba_residuals", "pmv_ba_solve", "pmv_triangulate_candidates", "pmv_triangulate_candidates_ahead", "pmv_fivepoint_hypotheses",
    "pmv_find_essential_mat", "pmv_recover_pose", "pmv_debug_essential_iters_table",
    "pmv_find_fundamental_mat", "pmv_debug_fundamental_iters_table", "pmv_debug_set_fundamental_r", "pmv_debug_fundamental_r", "pmv_debug_whole_rounds",
    "pmv_find_homography", "pmv_debug_homography_iters_table", "pmv_debug_homography_check", "pmv_debug_homography_launches",
    "pmv_triangulate_tracks", "pmv_batch_triangulate_tracks", "pmv_debug_tri_tracks_check", "pmv_debug_tri_tracks_launches",
    "pmv_klt_create", "pmv_klt_destroy", "pmv_klt_set_tracks", "pmv_klt_get_tracks", "pmv_klt_step", "pmv_debug_klt_stats",
    "pmv_klt_step_many", "pmv_debug_klt_many_stats",
    "pmv_klt_set_stereo", "pmv_klt_get_stereo", "pmv_klt_step_stereo", "pmv_klt_step_many_stereo", "pmv_debug_klt_stereo_stats",
    "pmv_camera_create", "pmv_camera_destroy", "pmv_undistort_points", "pmv_project_points",
    "pmv_camera_create_fisheye", "pmv_fisheye_map_build",
    "pmv_klt_set_observe", "pmv_klt_get_observe", "pmv_klt_get_observations", "pmv_debug_klt_observe_stats",
    "pmv_klt_set_prediction", "pmv_klt_get_prediction_result",
    "pmv_record_enable", "pmv_record_count", "pmv_record_size", "pmv_record_get",
    "pmv_prof_enable", "pmv_prof_select", "pmv_prof_kernel_count", "pmv_lk_counters", "pmv_prof_kernel_name", "pmv_prof_read",
    "pmv_pipeline_run", "pmv_pipeline_run_streamed", "pmv_pipeline_run_batch", "pmv_pipeline_run_batch_streamed", "pmv_batch_ingest_stats", "pmv_batch_stats", "pmv_debug_batch_launches", "pmv_pipeline_free", "pmv_pipeline_release", "pmv_pipeline_drain", "pmv_pipeline_num_poses", "pmv_pipeline_get_poses", "pmv_pipeline_num_frames",
    "pmv_pipeline_frame_feature_count", "pmv_pipeline_get_frame_features", "pmv_pipeline_stats_count", "pmv_pipeline_get_stats",
    "pmv_batch_open", "pmv_batch_close", "pmv_batch_frame_upload", "pmv_batch_upload_stats", "pmv_batch_upload_rounds",
    "pmv_batch_lk_track", "pmv_batch_lk_track_ex", "pmv_batch_lk_track_fb", "pmv_batch_knn_match", "pmv_batch_detect_gftt", "pmv_batch_detect_shitomasi", "pmv_batch_detect_fast",
    "pmv_batch_pnp_ransac", "pmv_batch_ba_solve", "pmv_batch_triangulate_candidates", "pmv_batch_fivepoint_hypotheses",
    "pmv_batch_find_essential_mat", "pmv_batch_recover_pose", "pmv_batch_find_fundamental_mat", "pmv_batch_find_homography",
]


GFTT_UNLIMITED_CAP = 4096   # PMV_GFTT_UNLIMITED_CAP of include/pmv_hip.h
GFTT_FRAME_MAX_CORNERS = 16384   # PMV_GFTT_FRAME_MAX_CORNERS of include/pmv_hip.h
REFILL_MAX_TRACKS = 8192   # PMV_REFILL_MAX_TRACKS of include/pmv_hip.h
REFILL_MAX_RADIUS = 255    # PMV_REFILL_MAX_RADIUS of include/pmv_hip.h


class PipelineParams(C.Structure):
    _fields_ = [("n_frames", C.c_int), ("w", C.c_int), ("h", C.c_int), ("min_tracked_features", C.c_int),
                ("tracked_features_tol", C.c_int), ("init_frames", C.c_int), ("bundle_size", C.c_int),
                ("ba_iterations", C.c_int), ("extractor", C.c_int), ("threaded", C.c_int), ("n_threads", C.c_int),
                ("build_pyramids", C.c_int), ("matcher", C.c_int), ("device_fivepoint", C.c_int)]


STAT_KEYS = ["lk_calls", "lk_points", "detect_calls", "pnp_calls", "pnp_points", "tri_calls", "ba_calls", "ba_obs",
             "ba_points", "heuristic_motion", "seconds", "init_offset", "n_landmarks", "scale", "t_lk", "t_detect", "t_pnp", "t_tri",
             "t_ba", "t_pnp_kernel", "t_ba_kernel", "t_tri_essential", "t_tri_pose", "tri_hypotheses", "tri_ahead"]


BATCH_INGEST_KEYS = ["rounds", "frames", "bytes", "memcpy_s", "ingest_wait_s", "seq_wait_s"]   # pmv_batch_ingest_stats, in order


FRAME_FORMATS = {"gray": 0, "bgr": 1}   # pmv_frame_format of include/pmv_hip.h


def _host_frames(frames, fmt, who, h=None, w=None, n=None):
    """the host frames of a staged / streamed call as the library reads them. "bgr" (Context.set_frame_format): (n, h, w, 3) uint8 or a
    ValueError before anything reaches the device; "gray": as before, converted to contiguous uint8."""
    if fmt != "bgr":
        f = np.ascontiguousarray(frames, np.uint8)
        if f.ndim != 3 or (h is not None and f.shape[1:] != (h, w)) or (n is not None and f.shape[0] != n):
            # (n, h, w, 3) on a gray context is a forgotten set_frame_format("bgr"): the library would read the interleaved bytes as gray frames
            want = f"({'n' if n is None else n}, {'h' if h is None else h}, {'w' if w is None else w})"
            raise ValueError(f"{who}: the context's frame format is gray: frames must be {want} uint8, got {f.shape} (set_frame_format(\"bgr\") for colour frames)")
        return f
    f = np.asarray(frames)
    ok = f.dtype == np.uint8 and f.ndim == 4 and f.shape[3] == 3 and f.shape[0] >= 1
    if ok and h is not None:
        ok = f.shape[1:3] == (h, w)
    if ok and n is not None:
        ok = f.shape[0] == n
    if not ok:
        want = f"({'n' if n is None else n}, {'h' if h is None else h}, {'w' if w is None else w}, 3)"
        raise ValueError(f"{who}: the context's frame format is BGR: frames must be {want} uint8, got {f.shape} {f.dtype}")
    return np.ascontiguousarray(f)   # (a contiguous array, pinned or not, is passed as it is)


def _batch_streamed_args(seqs, w, h, ring, first_slot, fmt="gray"):
    """shapes of pipeline_run_batch_streamed's arguments, checked before anything reaches the device: (frames, gt_poses, first_slot). w, h:
    one int for all sequences, one int per sequence, or None = each sequence's own array shape; the sizes the library is given are the arrays'
    own (frames[b].shape[2], frames[b].shape[1]), which a given w, h must match."""
    if len(seqs) < 1:
        raise ValueError("pipeline_run_batch_streamed: no sequences")
    if int(ring) != ring or ring < 1:
        raise ValueError(f"pipeline_run_batch_streamed: ring must be a positive integer, got {ring!r}")
    if (w is None) != (h is None):
        raise ValueError("pipeline_run_batch_streamed: w and h are given together, or both None (each sequence's own array shape)")
    ws = hs = [None] * len(seqs)
    if w is not None:
        ws = _per_sequence("pipeline_run_batch_streamed", "w", w, len(seqs))
        hs = _per_sequence("pipeline_run_batch_streamed", "h", h, len(seqs))
    frames, gts = [], []
    for b, seq in enumerate(seqs):
        if len(seq) != 2:
            raise ValueError(f"pipeline_run_batch_streamed: sequence {b} must be (frames, gt_poses)")
        f, gt = seq
        f = np.asarray(f)
        if fmt == "bgr":
            f = _host_frames(f, fmt, f"pipeline_run_batch_streamed: sequence {b}", hs[b], ws[b])
        elif f.dtype != np.uint8 or f.ndim != 3 or (ws[b] is not None and f.shape[1:] != (hs[b], ws[b])):
            want = f"(n, {hs[b]}, {ws[b]})" if ws[b] is not None else "(n, h, w)"
            raise ValueError(f"pipeline_run_batch_streamed: sequence {b}: frames must be {want} uint8, got {f.shape} {f.dtype}")
        f = np.ascontiguousarray(f)   # (a contiguous array, pinned or not, is passed as it is)
        g = np.ascontiguousarray(gt, np.float64)
        if g.size != 12 * f.shape[0]:
            raise ValueError(f"pipeline_run_batch_streamed: sequence {b}: {f.shape[0]} frames but {g.size / 12:g} pose rows")
        frames.append(f)
        gts.append(g.reshape(f.shape[0], 12))
    B = len(frames)
    first = [b * int(ring) for b in range(B)] if first_slot is None else [int(v) for v in first_slot]
    if len(first) != B:
        raise ValueError(f"pipeline_run_batch_streamed: {len(first)} first slots for {B} sequences")
    return frames, gts, first


BATCH_UPLOAD_KEYS = ["rounds", "frames", "level0_launches", "pyrdown_launches"]   # pmv_batch_upload_stats, in order


def _session_sizes(sizes):
    """the (w, h) pairs of batch_open as a flat int32 array, checked before anything reaches the library"""
    try:
        pairs = [tuple(p) for p in sizes]
    except TypeError:
        raise ValueError(f"batch_open: sizes must be a sequence of (w, h) integer pairs, got {sizes!r}") from None
    if not pairs:
        raise ValueError("batch_open: no sizes")
    for p in pairs:
        if len(p) != 2 or any(isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) for v in p):
            raise ValueError(f"batch_open: sizes must be (w, h) integer pairs, got {p!r}")
    return np.asarray(pairs, np.int32).reshape(-1)


def _upload_source(frame, fmt):
    """what batch_frame_upload hands to pmv_batch_frame_upload: (address, w, h, stride in bytes, format, the object that keeps the memory
    alive). frame: a uint8 numpy array - (h, w) for "gray", (h, w, 3) for "bgr" - whose pixel axis (gray: the columns; bgr: columns and
    channels) is contiguous, with ANY row stride: a view into a larger image is passed in place with its own address and stride, it is not
    copied tight. Or any object with data_ptr(), shape and stride() (a torch tensor, pageable, host-pinned or on the device; strides in
    elements). Everything is checked here, before the library is touched."""
    if not isinstance(fmt, str) or fmt not in FRAME_FORMATS:
        raise ValueError(f"batch_frame_upload: fmt must be one of {sorted(FRAME_FORMATS)}, got {fmt!r}")
    nd = 3 if fmt == "bgr" else 2
    if isinstance(frame, np.ndarray):
        if frame.dtype != np.uint8:
            raise ValueError(f"batch_frame_upload: frames are uint8, got {frame.dtype}")
        shape, strides, addr = tuple(frame.shape), tuple(frame.strides), frame.ctypes.data
    elif all(hasattr(frame, a) for a in ("data_ptr", "shape", "stride")):
        dt = str(getattr(frame, "dtype", "uint8"))
        if not dt.endswith("uint8"):
            raise ValueError(f"batch_frame_upload: frames are uint8, got {dt}")
        shape, strides, addr = tuple(int(v) for v in frame.shape), tuple(int(v) for v in frame.stride()), int(frame.data_ptr())
    else:
        raise ValueError(f"batch_frame_upload: a uint8 numpy array or an object with data_ptr(), shape and stride() is needed, got {type(frame).__name__}")
    if len(shape) != nd or (nd == 3 and shape[2] != 3):
        want = "(h, w, 3)" if nd == 3 else "(h, w)"
        raise ValueError(f"batch_frame_upload: a {fmt} frame is {want} uint8, got shape {shape}")
    h, w = shape[0], shape[1]
    if h < 1 or w < 1:
        raise ValueError(f"batch_frame_upload: empty frame {shape}")
    if (nd == 2 and strides[1] != 1) or (nd == 3 and (strides[2] != 1 or strides[1] != 3)):
        raise ValueError(f"batch_frame_upload: the pixels of a row must be contiguous (strides {strides} for shape {shape}); only the row stride is free")
    stride = strides[0] if h > 1 else max(strides[0], w * (nd == 3 and 3 or 1))
    if stride < w * (3 if nd == 3 else 1) or stride >= 2 ** 31:
        raise ValueError(f"batch_frame_upload: row stride {strides[0]} bytes for rows of {w * (3 if nd == 3 else 1)} bytes (overlapping or reversed rows)")
    return addr, w, h, stride, FRAME_FORMATS[fmt], frame


def _per_sequence(who, name, value, B):
    """a plugin option of a batched call: one int for all B sequences or a sequence of B ints (checked before anything reaches the device)"""
    if np.ndim(value) == 0:
        return [int(value)] * B
    v = [int(x) for x in value]
    if len(v) != B:
        raise ValueError(f"{who}: {name} has {len(v)} entries for {B} sequences")
    return v


class PipelineResult:
    """poses (n,12: R row-major then t), per-frame (column,row,landmark) triples in container order, run statistics"""

    def __init__(self, lib, handle, want_features=True):
        n = lib.pmv_pipeline_num_poses(handle)
        self.poses = np.zeros((n, 12), np.float64)
        if n:
            lib.pmv_pipeline_get_poses(handle, _p(self.poses, _f64p))
        self.features = []
        if want_features:
            for k in range(lib.pmv_pipeline_num_frames(handle)):
                c = lib.pmv_pipeline_frame_feature_count(handle, k)
                a = np.zeros((c, 3), np.int32)
                if c:
                    lib.pmv_pipeline_get_frame_features(handle, k, _p(a, _i32p))
                self.features.append(a)
        st = np.zeros(lib.pmv_pipeline_stats_count(), np.float64)   # the library says how many doubles it writes
        assert len(st) >= len(STAT_KEYS)
        lib.pmv_pipeline_get_stats(handle, _p(st, _f64p))
        self.stats = dict(zip(STAT_KEYS, [float(v) for v in st[:len(STAT_KEYS)]]))
        self._deferred = None   # (lib, handle) when the caller asked to free the native result later (defer_free)

    def free(self):
        """frees the native result of a pipeline_run(..., defer_free=True) call (idempotent)"""
        if self._deferred:
            lib, handle = self._deferred
            self._deferred = None
            lib.pmv_pipeline_free(handle)

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def parse_record(buf):
    """one blob of the call log (layout: include/pmv_hip.h, "call log")"""
    pos = [0]
    raw = buf.tobytes()

    def take(dtype, count):
        nb = np.dtype(dtype).itemsize * count
        a = np.frombuffer(raw[pos[0]:pos[0] + nb], dtype=dtype).copy()
        pos[0] += nb
        return a
    kind = int(take(np.int32, 1)[0])
    if kind == 0:
        m, iters, nin = [int(v) for v in take(np.int32, 3)]
        r = dict(kind="pnp", m=m, iterations=iters, obj=take(np.float32, 3 * m).reshape(m, 3), img=take(np.float32, 2 * m).reshape(m, 2),
                 K=take(np.float64, 9), rvec_in=take(np.float64, 3), tvec_in=take(np.float64, 3))
        opt = take(np.float64, 2)
        r.update(reproj_err=float(opt[0]), confidence=float(opt[1]), rvec=take(np.float64, 3), tvec=take(np.float64, 3), inliers=take(np.int32, nin))
    elif kind == 1:
        nc, npnt, nobs, iters = [int(v) for v in take(np.int32, 4)]
        r = dict(kind="ba", nc=nc, np=npnt, n_obs=nobs, max_iterations=iters, cams_in=take(np.float64, 6 * nc).reshape(nc, 6),
                 pts_in=take(np.float64, 3 * npnt).reshape(npnt, 3), obs=take(np.float64, 2 * nobs).reshape(nobs, 2), K=take(np.float64, 9),
                 huber=float(take(np.float64, 1)[0]), cam_idx=take(np.int32, nobs), pt_idx=take(np.int32, nobs))
        r.update(cams=take(np.float64, 6 * nc).reshape(nc, 6), pts=take(np.float64, 3 * npnt).reshape(npnt, 3))
        sm = take(np.float64, 5)
        r.update(initial_cost=float(sm[0]), final_cost=float(sm[1]), iterations=int(sm[2]), successful_steps=int(sm[3]), termination=int(sm[4]))
    elif kind == 2:
        n = int(take(np.int32, 1)[0])
        r = dict(kind="dlt", n=n, q1=take(np.float64, 2 * n).reshape(n, 2), q2=take(np.float64, 2 * n).reshape(n, 2), P1x4=take(np.float64, 48),
                 mask_in=take(np.uint8, n), Q=take(np.float64, 16 * n).reshape(4, 4, n), mask=take(np.uint8, 4 * n).reshape(4, n), good=take(np.int32, 4))
    else:
        raise ValueError(f"unknown record kind {kind}")
    assert pos[0] == len(buf), "record length does not match its header"
    return r


_lib = None
_synth = None


def lib_path():
    return os.path.join(HERE, "libpmv_hip.so")


def load_library():
    """dlopen the product library (must have been built: __graft_entry__.build() or build.build_hip())."""
    global _lib
    if _lib is None:
        p = lib_path()
        if not os.path.exists(p):
            raise PmvError(-1, f"{p} not built; run `python -c 'import __graft_entry__ as g; g.build()'`")
        _lib = C.CDLL(p, mode=C.RTLD_GLOBAL)
        _lib.pmv_last_error.restype = C.c_char_p
        _lib.pmv_last_error.argtypes = [C.c_void_p]
        if hasattr(_lib, "pmv_thread_error"):
            _lib.pmv_thread_error.restype = C.c_char_p
            _lib.pmv_thread_error.argtypes = []
        if hasattr(_lib, "pmv_pipeline_run"):
            _lib.pmv_pipeline_run.argtypes = [C.c_void_p, C.POINTER(PipelineParams), _f64p, _f64p, C.POINTER(C.c_void_p)]
            _lib.pmv_pipeline_run_streamed.argtypes = [C.c_void_p, C.POINTER(PipelineParams), _f64p, _f64p, _u8p, C.POINTER(C.c_void_p)]
            _lib.pmv_pipeline_free.argtypes = [C.c_void_p]
            _lib.pmv_pipeline_release.argtypes = [C.c_void_p]
            _lib.pmv_pipeline_release.restype = None
            _lib.pmv_pipeline_drain.argtypes = []
            _lib.pmv_pipeline_drain.restype = None
            _lib.pmv_pipeline_num_poses.argtypes = [C.c_void_p]
            _lib.pmv_pipeline_get_poses.argtypes = [C.c_void_p, _f64p]
            _lib.pmv_pipeline_num_frames.argtypes = [C.c_void_p]
            _lib.pmv_pipeline_frame_feature_count.argtypes = [C.c_void_p, C.c_int]
            _lib.pmv_pipeline_get_frame_features.argtypes = [C.c_void_p, C.c_int, _i32p]
            _lib.pmv_pipeline_get_stats.argtypes = [C.c_void_p, _f64p]
    return _lib


def load_synth():
    global _synth
    if _synth is None:
        _synth = C.CDLL(_build.build_synth())
    return _synth


def _p(a, t):
    return a.ctypes.data_as(t)


def synth_sequence(seed, first, n, w, h, fx, fy, cx, cy, nthreads=8):
    """n deterministic synthetic KITTI-like frames (n, h, w) uint8 + their KITTI pose rows (n, 12)."""
    s = load_synth()
    out = np.empty((n, h, w), np.uint8)
    s.pmv_synth_sequence(C.c_uint64(seed), first, n, w, h, C.c_double(fx), C.c_double(fy), C.c_double(cx),
                         C.c_double(cy), _p(out, _u8p), nthreads)
    poses = np.empty((n, 12), np.float64)
    for i in range(n):
        s.pmv_synth_pose(C.c_uint64(seed), first + i, _p(poses[i], _f64p))
    return out, poses


def grid_cells(w, h, gw=255, gh=255):
    """OdometryPipeline::getGridROI (reference OdometryPipeline.cpp:674-693): row-major cells (x0, y0, cw, ch)."""
    cells = []
    for r in range(0, h, gh):
        for c in range(0, w, gw):
            cells.append((c, r, min(gw, w - c), min(gh, h - r)))
    return np.asarray(cells, np.int32)


class Context:
    """Opaque device context (owns HBM frame slots, workspaces and the front-end/back-end HIP streams)."""

    def __init__(self, max_w, max_h, n_slots=2, max_tracks=4096, max_ba_cams=32, max_ba_points=8192,
                 max_ba_obs=65536, device=0):
        self.lib = load_library()
        self.h = C.c_void_p()
        rc = self.lib.pmv_ctx_create(C.byref(self.h), device, max_w, max_h, n_slots, max_tracks, max_ba_cams,
                                     max_ba_points, max_ba_obs)
        if rc != 0:
            raise PmvError(rc, self.lib.pmv_last_error(None).decode())
        self.max_pixels = int(max_w) * int(max_h)   # the largest region a diagnostic may hand back (debug_refill_mask)

    def close(self):
        if self.h:
            self.lib.pmv_ctx_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc):
        if rc != 0:
            raise PmvError(rc, self.lib.pmv_last_error(self.h).decode())

    def _ckt(self, rc):
        """_ck for calls that several threads make on one context at once: the calling thread's own error text (pmv_thread_error)"""
        if rc != 0:
            raise PmvError(rc, self.lib.pmv_thread_error().decode())

    def sync(self):
        self._ck(self.lib.pmv_sync(self.h))

    # ---- frames ----
    def frame_upload(self, slot, gray):
        g = np.ascontiguousarray(gray, np.uint8)
        self._ck(self.lib.pmv_frame_upload(self.h, slot, _p(g, _u8p), g.shape[1], g.shape[0], g.shape[1]))

    def frame_upload_bgr(self, slot, bgr):
        """(h, w, 3) uint8 BGR image as cv::imread(IMREAD_COLOR) gives it: BGR2GRAY on the device, then the pyramid"""
        b = np.ascontiguousarray(bgr, np.uint8)
        assert b.ndim == 3 and b.shape[2] == 3
        self._ck(self.lib.pmv_frame_upload_bgr(self.h, slot, _p(b, _u8p), b.shape[1], b.shape[0], 3 * b.shape[1]))

    def set_frame_format(self, fmt):
        """"gray" (default) or "bgr": what the host frames of frames_stage, frames_stream_begin, pipeline_run(host_frames=...) and
        pipeline_run_batch_streamed hold (pmv_set_frame_format). With "bgr" they take (n, h, w, 3) uint8 BGR frames, as cv::imread(IMREAD_COLOR)
        gives them, and the conversion to gray runs on the device inside the level-0 kernel; frame_upload / frame_upload_bgr are not affected."""
        if not isinstance(fmt, str) or fmt not in FRAME_FORMATS:
            raise ValueError(f"set_frame_format: format must be one of {sorted(FRAME_FORMATS)}, got {fmt!r}")
        self._ck(self.lib.pmv_set_frame_format(self.h, FRAME_FORMATS[fmt]))
        self._frame_format = fmt

    @property
    def frame_format(self):
        return getattr(self, "_frame_format", "gray")

    def set_frame_preproc(self, remap=None, border_value=0, clahe=None):
        """pmv_set_frame_preproc: lens undistortion and / or CLAHE of every HOST frame that enters a slot through the feeder - frames_stream_begin,
        pipeline_run(host_frames=...) and pipeline_run_batch_streamed - in the order BGR -> remap -> CLAHE -> border. remap: a map id of
        remap_map_create or a sequence of ids (at most 8, pairwise different sizes: each sequence uses the map of its own frame size);
        border_value: cv's borderValue, 0..255; clahe: None or (clip_limit, (tiles_x, tiles_y)). No arguments: off (the default). Frames
        already in slots (frames_stage, staged batches) are not touched. Pass the camera matrix that goes with the map as K."""
        p = _preproc_arg("set_frame_preproc", remap, border_value, clahe)
        self.lib.pmv_set_frame_preproc.argtypes = [C.c_void_p, C.POINTER(FramePreproc)]
        self._ck(self.lib.pmv_set_frame_preproc(self.h, None if p is None else C.byref(p)))

    def get_frame_preproc(self):
        """pmv_get_frame_preproc: dict(remap=[map ids], border_value=int, clahe=None or (clip_limit, (tiles_x, tiles_y)))"""
        p = FramePreproc()
        self.lib.pmv_get_frame_preproc.argtypes = [C.c_void_p, C.POINTER(FramePreproc)]
        self._ck(self.lib.pmv_get_frame_preproc(self.h, C.byref(p)))
        cp = p.clahe_params
        return dict(remap=[int(p.map_ids[k]) for k in range(p.n_maps)], border_value=int(p.border_value),
                    clahe=(float(cp.clip_limit), (int(cp.tiles_x), int(cp.tiles_y))) if p.clahe else None)

    def debug_preproc_launches(self):
        """pmv_debug_preproc_launches: [feeder rounds that preprocessed, gather launches, CLAHE launch pairs, in-place border launches]"""
        out = (C.c_longlong * 4)()
        self.lib.pmv_debug_preproc_launches.argtypes = [C.c_void_p, C.POINTER(C.c_longlong)]
        self._ck(self.lib.pmv_debug_preproc_launches(self.h, out))
        return [int(v) for v in out]

    def frames_stage(self, first_slot, frames):
        f = _host_frames(frames, self.frame_format, "frames_stage")
        self._ck(self.lib.pmv_frames_stage(self.h, first_slot, f.shape[0], _p(f, _u8p), f.shape[2], f.shape[1]))

    def frames_stream_begin(self, first_slot, frames):
        """start streaming host frames (n, h, w) uint8 ((n, h, w, 3) BGR after set_frame_format("bgr")) into slots first_slot..; `frames` must
        stay alive until frames_stream_end()"""
        f = _host_frames(frames, self.frame_format, "frames_stream_begin")
        self._stream_src = f
        self._ck(self.lib.pmv_frames_stream_begin(self.h, first_slot, f.shape[0], _p(f, _u8p), f.shape[2], f.shape[1]))

    def frames_stream_end(self):
        self._ck(self.lib.pmv_frames_stream_end(self.h))
        self._stream_src = None

    def frames_build(self, first_slot, n):
        self._ck(self.lib.pmv_frames_build(self.h, first_slot, n))

    def frames_clahe(self, first_slot, n, clip_limit=40.0, tiles=(8, 8)):
        """pmv_frames_clahe: cv::createCLAHE(clip_limit, tiles)->apply on level 0 of the staged or built slots first_slot .. first_slot + n - 1,
        in place, then the border and the levels above rebuilt; the defaults are cv's. tiles = (tiles_x, tiles_y), 1..16 each."""
        p = _clahe_params("frames_clahe", clip_limit, tiles)
        self.lib.pmv_frames_clahe.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(ClaheParams)]
        self._ck(self.lib.pmv_frames_clahe(self.h, int(first_slot), int(n), C.byref(p)))

    def debug_clahe_launches(self):
        """pmv_debug_clahe_launches: [launch pairs of frames_clahe, session upload rounds with a CLAHE request, launch pairs made for them]"""
        out = (C.c_longlong * 3)()
        self.lib.pmv_debug_clahe_launches.argtypes = [C.c_void_p, C.POINTER(C.c_longlong)]
        self._ck(self.lib.pmv_debug_clahe_launches(self.h, out))
        return [int(v) for v in out]

    def remap_map_create(self, map_x, map_y):
        """pmv_remap_map_create: the (h, w) float32 maps of cv::remap (undistort_map, or the caller's own), converted once into cv's fixed-point
        form and kept on the device; returns the map's id. At most 16 per context."""
        mx, my = np.ascontiguousarray(map_x, np.float32), np.ascontiguousarray(map_y, np.float32)
        if mx.ndim != 2 or mx.shape != my.shape:
            raise ValueError(f"remap_map_create: map_x and map_y are (h, w) float32 arrays of one shape, got {mx.shape} and {my.shape}")
        out = C.c_int(-1)
        f32p = C.POINTER(C.c_float)
        self.lib.pmv_remap_map_create.argtypes = [C.c_void_p, C.c_int, C.c_int, f32p, f32p, C.POINTER(C.c_int)]
        self._ck(self.lib.pmv_remap_map_create(self.h, mx.shape[1], mx.shape[0], _p(mx, f32p), _p(my, f32p), C.byref(out)))
        return int(out.value)

    def remap_map_destroy(self, map_id):
        self.lib.pmv_remap_map_destroy.argtypes = [C.c_void_p, C.c_int]
        self._ck(self.lib.pmv_remap_map_destroy(self.h, int(map_id)))

    def frames_remap(self, first_slot, n, map_id, border_value=0):
        """pmv_frames_remap: cv::remap(INTER_LINEAR, BORDER_CONSTANT, border_value) through map `map_id` on level 0 of the staged or built slots
        first_slot .. first_slot + n - 1, then the border and the levels above rebuilt"""
        self.lib.pmv_frames_remap.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int]
        self._ck(self.lib.pmv_frames_remap(self.h, int(first_slot), int(n), int(map_id), int(border_value)))

    def debug_remap_launches(self):
        """pmv_debug_remap_launches: [k_remap launches of frames_remap, session upload rounds with a remap request, k_remap launches made for them]"""
        out = (C.c_longlong * 3)()
        self.lib.pmv_debug_remap_launches.argtypes = [C.c_void_p, C.POINTER(C.c_longlong)]
        self._ck(self.lib.pmv_debug_remap_launches(self.h, out))
        return [int(v) for v in out]

    def num_levels(self, slot):
        return self.lib.pmv_frame_num_levels(self.h, slot)

    def get_level(self, slot, level, max_w, max_h):
        out = np.zeros(max_w * max_h, np.uint8)
        w, h = C.c_int(), C.c_int()
        self._ck(self.lib.pmv_frame_get_level(self.h, slot, level, _p(out, _u8p), C.byref(w), C.byref(h)))
        return out[: w.value * h.value].reshape(h.value, w.value).copy()

    def get_level_padded(self, slot, level, max_w, max_h):
        """the level with its 64-pixel BORDER_REFLECT_101 frame"""
        out = np.zeros((max_w + 128) * (max_h + 128), np.uint8)
        w, h = C.c_int(), C.c_int()
        self._ck(self.lib.pmv_frame_get_level_padded(self.h, slot, level, _p(out, _u8p), C.byref(w), C.byref(h)))
        return out[: w.value * h.value].reshape(h.value, w.value).copy()

    # ---- BaseFeatureExtractor role ----
    # Each plugin call is marshalled once, in a private method that takes the library function and the error check: the single call (pmv_*,
    # _ck) and the session call (pmv_batch_*, _ckt: the calling thread's own error text) share it. `head`: () or (seq,) of a back-end call.
    def _detect_gftt(self, fn, ck, slot, cells, max_per_cell, quality, min_dist):
        cells = np.ascontiguousarray(cells, np.int32).reshape(-1, 4)
        n = cells.shape[0]
        cap = max_per_cell if max_per_cell > 0 else GFTT_UNLIMITED_CAP   # max_per_cell <= 0: no limit (cv::goodFeaturesToTrack)
        xy = np.zeros((n, cap, 2), np.int32)
        cnt = np.zeros(n, np.int32)
        ck(fn(self.h, int(slot), _p(cells, _i32p), n, int(max_per_cell), C.c_double(quality), C.c_double(min_dist), _p(xy, _i32p), _p(cnt, _i32p)))
        return [xy[i, : cnt[i]].copy() for i in range(n)]

    def detect_gftt(self, slot, cells, max_per_cell, quality=0.01, min_dist=5.0):
        return self._detect_gftt(self.lib.pmv_detect_gftt, self._ck, slot, cells, max_per_cell, quality, min_dist)

    def _gftt_ex(self, fn, ck, slot, cells, max_per_cell, quality, min_dist, mask, block_size, use_harris, k):
        cells = np.ascontiguousarray(cells, np.int32).reshape(-1, 4)
        n = cells.shape[0]
        cap = max_per_cell if max_per_cell > 0 else GFTT_UNLIMITED_CAP
        xy = np.zeros((n, cap, 2), np.int32)
        cnt = np.zeros(n, np.int32)
        p = GfttParams(float(quality), float(min_dist), int(block_size), 1 if use_harris else 0, float(k))
        mptr, mstride = None, 0
        if mask is not None:
            # passed in place with its own row stride (a view into a larger array is not copied tight); the library checks it against the frame
            if not isinstance(mask, np.ndarray) or mask.dtype != np.uint8 or mask.ndim != 2 or (mask.shape[1] > 1 and mask.strides[1] != 1):
                raise ValueError("detect_gftt_ex: mask must be an (h, w) uint8 array whose rows are contiguous (any row stride)")
            # the library reads the mask under the cells only: a mask smaller than the frame must still cover every cell
            if n and ((cells[:, 0] + cells[:, 2]).max() > mask.shape[1] or (cells[:, 1] + cells[:, 3]).max() > mask.shape[0] or cells[:, :2].min() < 0):
                raise ValueError(f"detect_gftt_ex: a cell lies outside the {mask.shape[1]}x{mask.shape[0]} mask (the mask has the frame's size)")
            mptr, mstride = C.cast(C.c_void_p(mask.ctypes.data), _u8p), int(mask.strides[0]) if mask.shape[0] > 1 else max(int(mask.strides[0]), mask.shape[1])
        fn.argtypes = [C.c_void_p, C.c_int, _i32p, C.c_int, C.c_int, C.POINTER(GfttParams), _u8p, C.c_int, _i32p, _i32p]
        ck(fn(self.h, int(slot), _p(cells, _i32p), n, int(max_per_cell), C.byref(p), mptr, mstride, _p(xy, _i32p), _p(cnt, _i32p)))
        return [xy[i, : cnt[i]].copy() for i in range(n)]

    def detect_gftt_ex(self, slot, cells, max_per_cell, quality=0.01, min_dist=5.0, mask=None, block_size=3, use_harris=False, k=0.04):
        """pmv_detect_gftt_ex: detect_gftt with cv::goodFeaturesToTrack's remaining arguments. mask: None or an (h, w) uint8 array of the frame's
        size (non-zero = allowed; any row stride), each cell sees its own rectangle of it; block_size 1..15; use_harris with k. The defaults
        return detect_gftt's arrays."""
        return self._gftt_ex(self.lib.pmv_detect_gftt_ex, self._ck, slot, cells, max_per_cell, quality, min_dist, mask, block_size, use_harris, k)

    def _gftt_frame(self, fn, ck, slot, max_corners, quality, min_dist, mask, block_size, use_harris, k, roi, out_cap):
        if out_cap is None:
            out_cap = int(max_corners) if max_corners > 0 else GFTT_FRAME_MAX_CORNERS
        xy = np.zeros((max(int(out_cap), 1), 2), np.int32)
        cnt = C.c_int(0)
        p = GfttParams(float(quality), float(min_dist), int(block_size), 1 if use_harris else 0, float(k))
        rptr = None
        if roi is not None:
            roi = np.ascontiguousarray(roi, np.int32).reshape(-1)
            if roi.size != 4:
                raise ValueError("detect_gftt_frame: roi is (x0, y0, w, h)")
            rptr = _p(roi, _i32p)
        mptr, mstride = None, 0
        if mask is not None:
            # passed in place with its own row stride; the library reads the bytes under the region only, so the mask must cover it
            if not isinstance(mask, np.ndarray) or mask.dtype != np.uint8 or mask.ndim != 2 or (mask.shape[1] > 1 and mask.strides[1] != 1):
                raise ValueError("detect_gftt_frame: mask must be an (h, w) uint8 array whose rows are contiguous (any row stride)")
            if roi is not None and (roi[0] < 0 or roi[1] < 0 or roi[0] + roi[2] > mask.shape[1] or roi[1] + roi[3] > mask.shape[0]):
                raise ValueError(f"detect_gftt_frame: the region lies outside the {mask.shape[1]}x{mask.shape[0]} mask (the mask has the frame's size)")
            mptr, mstride = C.cast(C.c_void_p(mask.ctypes.data), _u8p), int(mask.strides[0]) if mask.shape[0] > 1 else max(int(mask.strides[0]), mask.shape[1])
        fn.argtypes = [C.c_void_p, C.c_int, _i32p, C.c_int, C.POINTER(GfttParams), _u8p, C.c_int, _i32p, C.c_int, C.POINTER(C.c_int)]
        ck(fn(self.h, int(slot), rptr, int(max_corners), C.byref(p), mptr, mstride, _p(xy, _i32p), int(out_cap), C.byref(cnt)))
        return xy[: cnt.value].copy()

    def detect_gftt_frame(self, slot, max_corners, quality=0.01, min_dist=5.0, mask=None, block_size=3, use_harris=False, k=0.04, roi=None, out_cap=None):
        """pmv_detect_gftt_frame: cv::goodFeaturesToTrack on the whole frame in `slot` (roi None) or on one region (x0, y0, w, h) of any size.
        Returns (n, 2) int32 region-local corners in cv's order. max_corners <= 0: no limit; out_cap (default max_corners, or
        GFTT_FRAME_MAX_CORNERS without a limit) is the list's capacity - more corners than that raise PmvError (PMV_ERR_OVERFLOW). With a
        mask of a frame that is smaller than the mask's array, pass roi."""
        return self._gftt_frame(self.lib.pmv_detect_gftt_frame, self._ck, slot, max_corners, quality, min_dist, mask, block_size, use_harris, k, roi, out_cap)

    def _gftt_refill(self, fn, ck, slot, max_corners, tracks, radius, priorities, base_mask, quality, min_dist, block_size, use_harris, k, roi, out_cap):
        if out_cap is None:
            out_cap = int(max_corners) if max_corners > 0 else GFTT_FRAME_MAX_CORNERS
        tracks = np.ascontiguousarray(tracks, np.float32)
        if tracks.size and (tracks.ndim != 2 or tracks.shape[1] != 2):
            raise ValueError("detect_gftt_refill: tracks must be an (n, 2) float32 array")
        n = tracks.size // 2
        pptr = None
        if priorities is not None:
            priorities = np.ascontiguousarray(priorities, np.int32).reshape(-1)
            if priorities.size != n:
                raise ValueError("detect_gftt_refill: one priority per track")
            pptr = _p(priorities, _i32p)
        keep = np.zeros(max(n, 1), np.uint8)
        xy = np.zeros((max(int(out_cap), 1), 2), np.int32)
        cnt = C.c_int(0)
        p = GfttParams(float(quality), float(min_dist), int(block_size), 1 if use_harris else 0, float(k))
        rptr = None
        if roi is not None:
            roi = np.ascontiguousarray(roi, np.int32).reshape(-1)
            if roi.size != 4:
                raise ValueError("detect_gftt_refill: roi is (x0, y0, w, h)")
            rptr = _p(roi, _i32p)
        mptr, mstride = None, 0
        if base_mask is not None:
            # passed in place with its own row stride: the library reads the bytes under the tracks and under the region
            if not isinstance(base_mask, np.ndarray) or base_mask.dtype != np.uint8 or base_mask.ndim != 2 or (base_mask.shape[1] > 1 and base_mask.strides[1] != 1):
                raise ValueError("detect_gftt_refill: base_mask must be an (h, w) uint8 array whose rows are contiguous (any row stride)")
            mptr = C.cast(C.c_void_p(base_mask.ctypes.data), _u8p)
            mstride = int(base_mask.strides[0]) if base_mask.shape[0] > 1 else max(int(base_mask.strides[0]), base_mask.shape[1])
        fn.argtypes = [C.c_void_p, C.c_int, _i32p, C.c_int, C.POINTER(GfttParams), _f32p, _i32p, C.c_int, C.c_int, _u8p, C.c_int, _u8p, _i32p, C.c_int, C.POINTER(C.c_int)]
        ck(fn(self.h, int(slot), rptr, int(max_corners), C.byref(p), _p(tracks, _f32p) if n else None, pptr, n, int(radius), mptr, mstride, _p(keep, _u8p), _p(xy, _i32p),
              int(out_cap), C.byref(cnt)))
        return keep[:n].copy(), xy[: cnt.value].copy()

    def detect_gftt_refill(self, slot, max_corners, tracks, radius, priorities=None, base_mask=None, quality=0.01, min_dist=5.0, block_size=3, use_harris=False, k=0.04,
                           roi=None, out_cap=None):
        """pmv_detect_gftt_refill: FeatureTracker::setMask on `tracks` ((n, 2) float32 frame coordinates; priorities: None or n int32, higher
        first) with cv::circle's `radius`, then detect_gftt_frame with that mask - the mask is made on the device. base_mask: None or an
        (h, w) uint8 array of the frame's size (a track on a byte other than 255 is dropped; 0 = not allowed for the detector).
        Returns (keep (n,) uint8, corners (m, 2) int32 region-local in cv's order)."""
        return self._gftt_refill(self.lib.pmv_detect_gftt_refill, self._ck, slot, max_corners, tracks, radius, priorities, base_mask, quality, min_dist, block_size,
                                 use_harris, k, roi, out_cap)

    def debug_refill_mask(self):
        """pmv_debug_refill_mask: the (h, w) uint8 mask of the region of the last detect_gftt_refill call of this context"""
        out = np.zeros(self.max_pixels, np.uint8)
        w, h = C.c_int(0), C.c_int(0)
        self.lib.pmv_debug_refill_mask.argtypes = [C.c_void_p, _u8p, C.c_longlong, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        self._ck(self.lib.pmv_debug_refill_mask(self.h, _p(out, _u8p), out.size, C.byref(w), C.byref(h)))
        return out[: w.value * h.value].reshape(h.value, w.value).copy()

    def debug_refill_stats(self):
        """pmv_debug_refill_stats: [single refill calls, session rounds with a refill request, select + paint launch pairs made for them, bytes
        of mask copied host -> device by refill calls]"""
        out = (C.c_longlong * 4)()
        self.lib.pmv_debug_refill_stats.argtypes = [C.c_void_p, C.POINTER(C.c_longlong)]
        self._ck(self.lib.pmv_debug_refill_stats(self.h, out))
        return [int(v) for v in out]

    def debug_gftt_frame_stats(self):
        """pmv_debug_gftt_frame_stats: [frame calls of the single entry point, session rounds with a frame request, launch pairs made for them,
        records above the threshold in the last request served, of those kept off-chip, on-chip record capacity of the selection kernel]"""
        out = (C.c_longlong * 6)()
        self.lib.pmv_debug_gftt_frame_stats.argtypes = [C.c_void_p, C.POINTER(C.c_longlong)]
        self._ck(self.lib.pmv_debug_gftt_frame_stats(self.h, out))
        return [int(v) for v in out]

    def gftt_response_ex(self, slot, cell, block_size=3, use_harris=False, k=0.04):
        """pmv_debug_gftt_response_ex: the float32 response map of one cell for this block size and response kind"""
        cell = np.ascontiguousarray(cell, np.int32)
        out = np.zeros((cell[3], cell[2]), np.float32)
        p = GfttParams(0.01, 5.0, int(block_size), 1 if use_harris else 0, float(k))
        self.lib.pmv_debug_gftt_response_ex.argtypes = [C.c_void_p, C.c_int, _i32p, C.POINTER(GfttParams), _f32p]
        self._ck(self.lib.pmv_debug_gftt_response_ex(self.h, int(slot), _p(cell, _i32p), C.byref(p), _p(out, _f32p)))
        return out

    def debug_gftt_general(self, on):
        """diagnostic: detect_gftt_ex's default arguments through the general kernels as well (pmv_debug_gftt_general); changes no result"""
        self._ck(self.lib.pmv_debug_gftt_general(self.h, 1 if on else 0))

    def _corner_subpix(self, fn, ck, slot, xy, win, zero_zone, max_iter, eps, return_info):
        # refused before the library is touched: the library takes n * 2 float32 values in place
        if not isinstance(xy, np.ndarray) or xy.dtype != np.float32 or xy.ndim != 2 or xy.shape[1] != 2:
            raise ValueError("corner_subpix: xy must be an (n, 2) float32 array")
        if len(win) != 2 or len(zero_zone) != 2:
            raise ValueError("corner_subpix: win and zero_zone are (w, h) pairs of half sizes")
        out = np.ascontiguousarray(xy).copy()
        n = out.shape[0]
        iters = np.zeros(n, np.uint8)
        flags = np.zeros(n, np.uint8)
        p = SubpixParams(int(win[0]), int(win[1]), int(zero_zone[0]), int(zero_zone[1]), int(max_iter), float(eps))
        fn.argtypes = [C.c_void_p, C.c_int, _f32p, C.c_int, C.POINTER(SubpixParams), _u8p, _u8p]
        ck(fn(self.h, int(slot), _p(out, _f32p), n, C.byref(p), _p(iters, _u8p) if return_info else None, _p(flags, _u8p) if return_info else None))
        return (out, iters, flags) if return_info else out

    def corner_subpix(self, slot, xy, win=(5, 5), zero_zone=(-1, -1), max_iter=30, eps=0.01, return_info=False):
        """pmv_corner_subpix: cv::cornerSubPix on level 0 of `slot`. xy: (n, 2) float32 FRAME coordinates (detect_gftt* returns cell-local
        corners: add the cell origin); win / zero_zone: cv's half sizes. Returns a new (n, 2) float32 array; with return_info also the
        position updates made per point and the flag bits (1 determinant, 2 left the frame, 4 iteration cap, 8 reverted)."""
        return self._corner_subpix(self.lib.pmv_corner_subpix, self._ck, slot, xy, win, zero_zone, max_iter, eps, return_info)

    def debug_subpix_launches(self):
        """pmv_debug_subpix_launches: [launches of corner_subpix, session rounds with a subpix request, launches made for them]"""
        out = (C.c_longlong * 3)()
        self.lib.pmv_debug_subpix_launches.argtypes = [C.c_void_p, C.POINTER(C.c_longlong)]
        self._ck(self.lib.pmv_debug_subpix_launches(self.h, out))
        return [int(v) for v in out]

    def _detect_shitomasi(self, fn, ck, slot, cells, max_per_cell, quality):
        cells = np.ascontiguousarray(cells, np.int32).reshape(-1, 4)
        n = cells.shape[0]
        xy = np.zeros((n, max(max_per_cell, 1), 2), np.int32)
        sc = np.zeros((n, max(max_per_cell, 1)), np.float64)
        cnt = np.zeros(n, np.int32)
        ck(fn(self.h, int(slot), _p(cells, _i32p), n, int(max_per_cell), C.c_double(quality), _p(xy, _i32p), _p(sc, _f64p), _p(cnt, _i32p)))
        return [(xy[i, : cnt[i]].copy(), sc[i, : cnt[i]].copy()) for i in range(n)]

    def detect_shitomasi(self, slot, cells, max_per_cell, quality=0.4):
        return self._detect_shitomasi(self.lib.pmv_detect_shitomasi, self._ck, slot, cells, max_per_cell, quality)

    def _detect_fast(self, fn, ck, slot, cells, max_per_cell, threshold, nonmax):
        cells = np.ascontiguousarray(cells, np.int32).reshape(-1, 4)
        n = cells.shape[0]
        cap = max(max_per_cell, 1)
        xy = np.zeros((n, cap, 2), np.int32)
        rs = np.zeros((n, cap), np.float32)
        cnt = np.zeros(n, np.int32)
        ck(fn(self.h, int(slot), _p(cells, _i32p), n, int(max_per_cell), int(threshold), 1 if nonmax else 0, _p(xy, _i32p), _p(rs, _f32p), _p(cnt, _i32p)))
        return [(xy[i, : cnt[i]].copy(), rs[i, : cnt[i]].copy()) for i in range(n)]

    def detect_fast(self, slot, cells, max_per_cell, threshold=10, nonmax=True):
        """cv::FAST per view (views may be as large as the frame): [(xy (k,2) int32, response (k,) float32)] per cell"""
        return self._detect_fast(self.lib.pmv_detect_fast, self._ck, slot, cells, max_per_cell, threshold, nonmax)

    def _knn_match(self, fn, ck, src_slot, cmp_slot, src_xy, cmp_xy, neighbours, window):
        s = np.ascontiguousarray(src_xy, np.int32).reshape(-1, 2)
        c = np.ascontiguousarray(cmp_xy, np.int32).reshape(-1, 2)
        best = np.zeros(max(len(s), 1), np.int32)
        err = np.zeros(max(len(s), 1), np.float32)
        ck(fn(self.h, int(src_slot), int(cmp_slot), _p(s, _i32p), len(s), _p(c, _i32p), len(c), int(neighbours), int(window), _p(best, _i32p), _p(err, _f32p)))
        return best[: len(s)].copy(), err[: len(s)].copy()

    def knn_match(self, src_slot, cmp_slot, src_xy, cmp_xy, neighbours=7, window=15):
        """kNNFeatureMatcher's arithmetic: (best candidate index or -1, window error) per source feature"""
        return self._knn_match(self.lib.pmv_knn_match, self._ck, src_slot, cmp_slot, src_xy, cmp_xy, neighbours, window)

    def gftt_response(self, slot, cell):
        cell = np.ascontiguousarray(cell, np.int32)
        out = np.zeros((cell[3], cell[2]), np.float32)
        self._ck(self.lib.pmv_debug_gftt_response(self.h, slot, _p(cell, _i32p), _p(out, _f32p)))
        return out

    def shitomasi_response(self, slot, cell):
        cell = np.ascontiguousarray(cell, np.int32)
        out = np.zeros((cell[3], cell[2]), np.float64)
        self._ck(self.lib.pmv_debug_shitomasi_response(self.h, slot, _p(cell, _i32p), _p(out, _f64p)))
        return out

    # ---- BaseFeatureMatcher role ----
    def _lk_track(self, fn, ck, prev_slot, next_slot, prev_xy):
        p = np.ascontiguousarray(prev_xy, np.float32).reshape(-1, 2)
        n = p.shape[0]
        out = np.zeros((n, 2), np.float32)
        st = np.zeros(n, np.uint8)
        err = np.zeros(n, np.float32)
        ck(fn(self.h, int(prev_slot), int(next_slot), _p(p, _f32p), n, _p(out, _f32p), _p(st, _u8p), _p(err, _f32p)))
        return out, st, err

    def lk_track(self, prev_slot, next_slot, prev_xy):
        return self._lk_track(self.lib.pmv_lk_track, self._ck, prev_slot, next_slot, prev_xy)

    def _lk_ex(self, fn, ck, fb, prev_slot, next_slot, prev_xy, init_xy, min_eigenvals, levels=None):
        p = np.ascontiguousarray(prev_xy, np.float32).reshape(-1, 2)
        n = p.shape[0]
        flags = (LK_USE_INITIAL_FLOW if init_xy is not None else 0) | (LK_GET_MIN_EIGENVALS if min_eigenvals else 0)
        # the in/out array of the call: the initial flow on the way in, the tracked positions on the way out
        nxt = np.zeros((n, 2), np.float32) if init_xy is None else np.array(init_xy, np.float32).reshape(-1, 2)
        if nxt.shape[0] != n:
            raise ValueError(f"init_xy has {nxt.shape[0]} points, prev_xy {n}")
        st = np.zeros(n, np.uint8)
        err = np.zeros(n, np.float32)
        args = [self.h, int(prev_slot), int(next_slot), _p(p, _f32p), n, _p(nxt, _f32p), flags, _p(st, _u8p), _p(err, _f32p)]
        if levels is not None:   # pmv_lk_track_fb_levels: the two top levels sit behind `flags`; forward only = three null back outputs
            args[7:7] = [int(levels[0]), int(levels[1])]
            if not fb:
                args += [None, None, None]
        if not fb:
            ck(fn(*args))
            return nxt, st, err
        bxy = np.zeros((n, 2), np.float32)
        bst = np.zeros(n, np.uint8)
        berr = np.zeros(n, np.float32)
        ck(fn(*args, _p(bxy, _f32p), _p(bst, _u8p), _p(berr, _f32p)))
        return nxt, st, err, bxy, bst, berr

    def lk_track_ex(self, prev_slot, next_slot, prev_xy, init_xy=None, min_eigenvals=False):
        """pmv_lk_track_ex: lk_track with cv's flags. init_xy (n x 2): OPTFLOW_USE_INITIAL_FLOW, the search of point i starts there;
        min_eigenvals: OPTFLOW_LK_GET_MIN_EIGENVALS, err is the minimum eigenvalue measure instead of the residual. Returns (xy, status, err)."""
        return self._lk_ex(self.lib.pmv_lk_track_ex, self._ck, False, prev_slot, next_slot, prev_xy, init_xy, min_eigenvals)

    def lk_track_fb(self, prev_slot, next_slot, prev_xy, init_xy=None, min_eigenvals=False):
        """pmv_lk_track_fb: lk_track_ex and, in the same launch, every tracked point back into the first frame. Returns
        (xy, status, err, back_xy, back_status, back_err); thresholding |back_xy - prev_xy| is the caller's policy."""
        return self._lk_ex(self.lib.pmv_lk_track_fb, self._ck, True, prev_slot, next_slot, prev_xy, init_xy, min_eigenvals)

    def lk_track_fb_levels(self, prev_slot, next_slot, prev_xy, init_xy=None, min_eigenvals=False, fwd_top_level=-1, back_top_level=-1, back=True):
        """pmv_lk_track_fb_levels: lk_track_fb whose forward / backward pass starts at pyramid level min(top, levels - 1) of the slots as
        they are built (cv's maxLevel per call); -1 = the top. back=False: forward only, (xy, status, err) as lk_track_ex."""
        fn = self.lib.pmv_lk_track_fb_levels
        fn.argtypes = [C.c_void_p, C.c_int, C.c_int, _f32p, C.c_int, _f32p, C.c_int, C.c_int, C.c_int, _u8p, _f32p, _f32p, _u8p, _f32p]
        return self._lk_ex(fn, self._ck, bool(back), prev_slot, next_slot, prev_xy, init_xy, min_eigenvals, levels=(fwd_top_level, back_top_level))

    def set_lk_params(self, win=32, max_level=4, max_iter=30, eps=0.01, min_eig=1e-4):
        """cv::calcOpticalFlowPyrLK's winSize (square), maxLevel, criteria and minEigThreshold for every pyramid built and every LK call
        made from now on (pmv_set_lk_params). A change of win or max_level empties every frame slot: upload the frames again."""
        p = LKParams(int(win), int(max_level), int(max_iter), float(eps), float(min_eig))
        self.lib.pmv_set_lk_params.argtypes = [C.c_void_p, C.POINTER(LKParams)]
        self._ck(self.lib.pmv_set_lk_params(self.h, C.byref(p)))

    def lk_params(self):
        """the context's LK setting as a dict with the keyword names of set_lk_params"""
        p = LKParams()
        self.lib.pmv_get_lk_params.argtypes = [C.c_void_p, C.POINTER(LKParams)]
        self._ck(self.lib.pmv_get_lk_params(self.h, C.byref(p)))
        return dict(win=p.win, max_level=p.max_level, max_iter=p.max_iter, eps=p.eps, min_eig=p.min_eig)

    def debug_lk_general(self, on):
        """diagnostic: the default window through the general LK kernels as well (pmv_debug_lk_general); changes no result"""
        self._ck(self.lib.pmv_debug_lk_general(self.h, 1 if on else 0))

    # ---- BasePnPSolver role ----
    def _pnp_ransac(self, fn, ck, head, obj_xyz, img_xy, K, rvec, tvec, iterations, reproj_err, confidence):
        o = np.ascontiguousarray(obj_xyz, np.float32).reshape(-1, 3)
        i2 = np.ascontiguousarray(img_xy, np.float32).reshape(-1, 2)
        m = o.shape[0]
        Kd = np.ascontiguousarray(K, np.float64).reshape(9)
        rv = np.array(rvec, np.float64).reshape(3).copy()
        tv = np.array(tvec, np.float64).reshape(3).copy()
        inl = np.zeros(max(m, 1), np.int32)
        nin = C.c_int()
        ck(fn(self.h, *head, _p(o, _f32p), _p(i2, _f32p), m, _p(Kd, _f64p), _p(rv, _f64p), _p(tv, _f64p), int(iterations), C.c_float(reproj_err),
              C.c_double(confidence), _p(inl, _i32p), C.byref(nin)))
        return rv, tv, inl[: nin.value].copy()

    def pnp_ransac(self, obj_xyz, img_xy, K, rvec, tvec, iterations=100, reproj_err=8.0, confidence=0.99):
        return self._pnp_ransac(self.lib.pmv_pnp_ransac, self._ck, (), obj_xyz, img_xy, K, rvec, tvec, iterations, reproj_err, confidence)

    def pnp_hypotheses(self, n=100):
        models = np.zeros((n, 6), np.float64)
        counts = np.zeros(n, np.int32)
        self._ck(self.lib.pmv_debug_pnp_hypotheses(self.h, n, _p(models, _f64p), _p(counts, _i32p)))
        return models, counts

    # ---- BaseOptimizer role ----
    def ba_residuals(self, cams, pts, obs_xy, cam_idx, pt_idx, K):
        cams = np.ascontiguousarray(cams, np.float64).reshape(-1, 6)
        pts = np.ascontiguousarray(pts, np.float64).reshape(-1, 3)
        obs = np.ascontiguousarray(obs_xy, np.float64).reshape(-1, 2)
        ci = np.ascontiguousarray(cam_idx, np.int32)
        pi = np.ascontiguousarray(pt_idx, np.int32)
        Kd = np.ascontiguousarray(K, np.float64).reshape(9)
        n = obs.shape[0]
        r = np.zeros((n, 2), np.float64)
        J = np.zeros((n, 2, 9), np.float64)
        self._ck(self.lib.pmv_ba_residuals(self.h, _p(cams, _f64p), cams.shape[0], _p(pts, _f64p), pts.shape[0],
                                           _p(obs, _f64p), _p(ci, _i32p), _p(pi, _i32p), n, _p(Kd, _f64p),
                                           _p(r, _f64p), _p(J, _f64p)))
        return r, J

    def set_ba_mode(self, mode):
        """0 = multi-kernel LM chain (default), 1 = one workgroup per solve / one launch per batched round"""
        self._ck(self.lib.pmv_set_ba_mode(self.h, int(mode)))

    def _ba_solve(self, fn, ck, head, cams, pts, obs_xy, cam_idx, pt_idx, K, huber, max_iterations):
        cams = np.array(cams, np.float64).reshape(-1, 6).copy()
        pts = np.array(pts, np.float64).reshape(-1, 3).copy()
        obs = np.ascontiguousarray(obs_xy, np.float64).reshape(-1, 2)
        ci = np.ascontiguousarray(cam_idx, np.int32)
        pi = np.ascontiguousarray(pt_idx, np.int32)
        Kd = np.ascontiguousarray(K, np.float64).reshape(9)
        s = BaSummary()
        ck(fn(self.h, *head, _p(cams, _f64p), cams.shape[0], _p(pts, _f64p), pts.shape[0], _p(obs, _f64p), _p(ci, _i32p), _p(pi, _i32p), obs.shape[0],
              _p(Kd, _f64p), C.c_double(huber), int(max_iterations), C.byref(s)))
        return cams, pts, s

    def ba_solve(self, cams, pts, obs_xy, cam_idx, pt_idx, K, huber=1.0, max_iterations=5):
        return self._ba_solve(self.lib.pmv_ba_solve, self._ck, (), cams, pts, obs_xy, cam_idx, pt_idx, K, huber, max_iterations)

    def _fivepoint_hypotheses(self, fn, ck, head, q1, q2, samples, thr):
        q1 = np.ascontiguousarray(q1, np.float64).reshape(-1, 2)
        q2 = np.ascontiguousarray(q2, np.float64).reshape(-1, 2)
        s = np.ascontiguousarray(samples, np.int32).reshape(-1, 5)
        nh = s.shape[0]
        models = np.zeros((nh, 10, 9), np.float64)
        nm = np.zeros(nh, np.int32)
        counts = np.zeros((nh, 10), np.int32)
        ck(fn(self.h, *head, _p(q1, _f64p), _p(q2, _f64p), q1.shape[0], _p(s, _i32p), nh, C.c_float(thr), _p(models, _f64p), _p(nm, _i32p), _p(counts, _i32p)))
        return models, nm, counts

    def fivepoint_hypotheses(self, q1, q2, samples, thr):
        """one RANSAC round of findEssentialMat on the GPU: models (n_hyp, 10, 9), n_models (n_hyp,), counts (n_hyp, 10)"""
        return self._fivepoint_hypotheses(self.lib.pmv_fivepoint_hypotheses, self._ck, (), q1, q2, samples, thr)

    def _triangulate_candidates(self, fn, ck, head, q1, q2, P1x4, mask_in):
        q1 = np.ascontiguousarray(q1, np.float64).reshape(-1, 2)
        q2 = np.ascontiguousarray(q2, np.float64).reshape(-1, 2)
        n = q1.shape[0]
        P = np.ascontiguousarray(P1x4, np.float64).reshape(48)
        mi = np.ascontiguousarray(mask_in, np.uint8).reshape(n)
        Q = np.zeros((4, 4, n), np.float64)
        mask = np.zeros((4, n), np.uint8)
        good = np.zeros(4, np.int32)
        ck(fn(self.h, *head, _p(q1, _f64p), _p(q2, _f64p), n, _p(P, _f64p), _p(mi, _u8p), _p(Q, _f64p), _p(mask, _u8p), _p(good, _i32p)))
        return Q, mask, good

    def triangulate_candidates(self, q1, q2, P1x4, mask_in):
        """DLT triangulation + cheirality of cv::recoverPose's four candidates: returns Q (4,4,n), mask (4,n), good (4,)"""
        return self._triangulate_candidates(self.lib.pmv_triangulate_candidates, self._ck, (), q1, q2, P1x4, mask_in)

    @staticmethod
    def _two_view_args(p1, p2, K):
        p1 = np.ascontiguousarray(p1, np.float64).reshape(-1, 2)
        p2 = np.ascontiguousarray(p2, np.float64).reshape(-1, 2)
        if p1.shape != p2.shape:
            raise ValueError(f"p1 {p1.shape} and p2 {p2.shape}: one (x, y) pair per correspondence in each")
        return p1, p2, np.ascontiguousarray(K, np.float64).reshape(9)

    def _find_essential(self, call, ck, head, p1, p2, K, prob, threshold):
        p1, p2, Kd = self._two_view_args(p1, p2, K)
        n = p1.shape[0]
        E = np.zeros(9, np.float64)
        mask = np.zeros(n, np.uint8)
        found, drawn = C.c_int(), C.c_int()
        ck(call(self.h, *head, _p(p1, _f64p), _p(p2, _f64p), n, _p(Kd, _f64p), C.c_double(prob), C.c_double(threshold), _p(E, _f64p), _p(mask, _u8p),
                C.byref(found), C.byref(drawn)))
        return bool(found.value), E.reshape(3, 3), mask, drawn.value

    def _recover_pose(self, call, ck, head, E, p1, p2, K, mask):
        p1, p2, Kd = self._two_view_args(p1, p2, K)
        n = p1.shape[0]
        Ed = np.ascontiguousarray(E, np.float64).reshape(9)
        m = np.array(mask, np.uint8).reshape(n).copy()
        R, t, tri = np.zeros(9, np.float64), np.zeros(3, np.float64), np.zeros((4, n), np.float64)
        good = C.c_int()
        ck(call(self.h, *head, _p(Ed, _f64p), _p(p1, _f64p), _p(p2, _f64p), n, _p(Kd, _f64p), _p(R, _f64p), _p(t, _f64p), _p(m, _u8p), _p(tri, _f64p),
                C.byref(good)))
        return R.reshape(3, 3), t, m, tri, good.value

    def find_essential_mat(self, p1, p2, K, prob=0.99, threshold=1.0):
        """cv::findEssentialMat(p1, p2, K, RANSAC, prob, threshold, mask), the whole RANSAC in one launch: (found, E (3, 3), mask (n,), samples drawn);
        found False = no model (E zeros, mask all 0)"""
        return self._find_essential(self.lib.pmv_find_essential_mat, self._ck, (), p1, p2, K, prob, threshold)

    def recover_pose(self, E, p1, p2, K, mask):
        """cv::recoverPose(E, p1, p2, K, R, t, HUGE_VAL, mask, tri): (R (3, 3), t (3,), mask out (n,), tri (4, n) homogeneous, good)"""
        return self._recover_pose(self.lib.pmv_recover_pose, self._ck, (), E, p1, p2, K, mask)

    def _find_fundamental(self, call, ck, head, p1, p2, threshold, confidence):
        p1 = np.ascontiguousarray(p1, np.float32).reshape(-1, 2)
        p2 = np.ascontiguousarray(p2, np.float32).reshape(-1, 2)
        if p1.shape != p2.shape:
            raise ValueError(f"p1 {p1.shape} and p2 {p2.shape}: one (x, y) pair per correspondence in each")
        n = p1.shape[0]
        F = np.zeros(9, np.float64)
        mask = np.zeros(n, np.uint8)
        found, drawn = C.c_int(), C.c_int()
        ck(call(self.h, *head, _p(p1, _f32p), _p(p2, _f32p), n, C.c_double(threshold), C.c_double(confidence), _p(F, _f64p), _p(mask, _u8p),
                C.byref(found), C.byref(drawn)))
        return bool(found.value), F.reshape(3, 3), mask, drawn.value

    def find_fundamental_mat(self, p1, p2, threshold=1.0, confidence=0.99):
        """cv::findFundamentalMat(p1, p2, FM_RANSAC, threshold, confidence, mask) for n >= 15 float32 correspondences, the whole RANSAC in one
        launch (a KLT loop's rejectWithF): (found, F (3, 3), mask (n,), samples drawn); found False = no model (F zeros, mask all 0)"""
        return self._find_fundamental(self.lib.pmv_find_fundamental_mat, self._ck, (), p1, p2, threshold, confidence)

    def _find_homography(self, call, ck, head, p1, p2, threshold, confidence, max_iters):
        p1 = np.ascontiguousarray(p1, np.float32).reshape(-1, 2)
        p2 = np.ascontiguousarray(p2, np.float32).reshape(-1, 2)
        if p1.shape != p2.shape:
            raise ValueError(f"p1 {p1.shape} and p2 {p2.shape}: one (x, y) pair per correspondence in each")
        n = p1.shape[0]
        H = np.zeros(9, np.float64)
        mask = np.zeros(n, np.uint8)
        found, drawn = C.c_int(), C.c_int()
        ck(call(self.h, *head, _p(p1, _f32p), _p(p2, _f32p), n, C.c_double(threshold), C.c_double(confidence), int(max_iters), _p(H, _f64p), _p(mask, _u8p),
                C.byref(found), C.byref(drawn)))
        return bool(found.value), H.reshape(3, 3), mask, drawn.value

    def find_homography(self, p1, p2, threshold=3.0, confidence=0.995, max_iters=2000):
        """cv::findHomography(p1, p2, cv::RANSAC, threshold, mask, max_iters, confidence) for n >= 4 float32 correspondences, the RANSAC and cv's
        refit on the inliers in one launch: (found, H (3, 3) image 1 -> image 2, mask (n,), samples drawn); found False = no model (H zeros,
        mask all 0). The defaults are cv's."""
        return self._find_homography(self.lib.pmv_find_homography, self._ck, (), p1, p2, threshold, confidence, max_iters)

    def homography_launches(self):
        """(k_homography_ransac launches, requests they served) since the context was created"""
        out = (C.c_longlong * 2)()
        self._ck(self.lib.pmv_debug_homography_launches(self.h, out))
        return int(out[0]), int(out[1])

    def _triangulate_tracks(self, call, ck, head, P3x4, obs_xy, cam_idx, pt_idx, n_points, params):
        P = np.ascontiguousarray(P3x4, np.float64).reshape(-1, 12)
        obs = np.ascontiguousarray(obs_xy, np.float64).reshape(-1, 2)
        ci = np.ascontiguousarray(cam_idx, np.int32).reshape(-1)
        pi = np.ascontiguousarray(pt_idx, np.int32).reshape(-1)
        if not (len(obs) == len(ci) == len(pi)):
            raise ValueError(f"obs_xy {obs.shape}, cam_idx {ci.shape} and pt_idx {pi.shape}: one entry per observation in each")
        n_obs, n_pts = len(obs), int(n_points)
        if params is not None and not isinstance(params, TriParams):
            params = TriParams(**params)
        xyz = np.zeros((max(n_pts, 0), 3), np.float64)
        status = np.zeros(max(n_pts, 0), np.uint8)
        err = np.zeros(max(n_pts, 0), np.float64)
        good = C.c_int()
        ck(call(self.h, *head, _p(P, _f64p), P.shape[0], _p(obs, _f64p), _p(ci, _i32p), _p(pi, _i32p), n_obs, n_pts, C.byref(params) if params is not None else None,
                _p(xyz, _f64p), _p(status, _u8p), _p(err, _f64p), C.byref(good)))
        return xyz, status, err, good.value

    def triangulate_tracks(self, P3x4, obs_xy, cam_idx, pt_idx, n_points, params=None):
        """pmv_triangulate_tracks: every landmark of a window from ALL its observations - N-view DLT, optional Gauss-Newton refinement, depth /
        reprojection / parallax gates - in one launch. P3x4 (nc, 3, 4) general projection matrices whose third row gives the depth
        (projections_from_ba_cams for pmv_ba_solve's cameras); obs_xy, cam_idx, pt_idx: the arrays of ba_solve; params: a TriParams, a dict of
        its fields, or None for the call's defaults. Returns (xyz (n_points, 3), status (n_points,) of TRI_* bits, err (n_points,), good)."""
        return self._triangulate_tracks(self.lib.pmv_triangulate_tracks, self._ck, (), P3x4, obs_xy, cam_idx, pt_idx, n_points, params)

    def tri_tracks_launches(self):
        """(k_tri_tracks / k_tri_tracks_batch launches, requests they served) since the context was created"""
        out = (C.c_longlong * 2)()
        self._ck(self.lib.pmv_debug_tri_tracks_launches(self.h, out))
        return int(out[0]), int(out[1])

    # ---- device-resident KLT tracker ----
    def klt_create(self, **params):
        """pmv_klt_create: a KltTracker whose track list stays on the device; one step() per frame runs LK (forward-backward), the filter,
        rejectWithF, setMask thinning, the masked detection, the optional sub-pixel refinement and the append. Keywords: klt_params()'s."""
        p = klt_params(**params)
        tid = C.c_int(-1)
        self.lib.pmv_klt_create.argtypes = [C.c_void_p, C.POINTER(KltParams), C.POINTER(C.c_int)]
        self._ck(self.lib.pmv_klt_create(self.h, C.byref(p), C.byref(tid)))
        return KltTracker(self, tid.value, p.target)

    def debug_klt_stats(self):
        """pmv_debug_klt_stats: [steps, host waits inside steps, kernel launches inside steps, trackers alive]"""
        out = (C.c_longlong * 4)()
        self.lib.pmv_debug_klt_stats.argtypes = [C.c_void_p, C.POINTER(C.c_longlong)]
        self._ck(self.lib.pmv_debug_klt_stats(self.h, out))
        return [int(v) for v in out]

    def klt_step_many(self, trackers, prev_slots, cur_slots):
        """pmv_klt_step_many: the trackers of this context stepped through one chain of launches; a list of KltTracker.step's 5-tuples, one per
        tracker, each byte for byte what its own step(prev_slots[j], cur_slots[j]) returns. The detector's and the refinement's arguments
        must be equal over the group and all frames of one size."""
        trackers = list(trackers)
        for t in trackers:
            if not isinstance(t, KltTracker) or t.ctx is not self or t.id is None:
                raise ValueError("klt_step_many: every tracker must be an open KltTracker of this context")
        k = len(trackers)
        prev_slots, cur_slots = np.ascontiguousarray(prev_slots, np.int32).reshape(-1), np.ascontiguousarray(cur_slots, np.int32).reshape(-1)
        if prev_slots.size != k or cur_slots.size != k:
            raise ValueError("klt_step_many: one prev_slot and one cur_slot per tracker")
        ids = np.asarray([t.id for t in trackers], np.int32)
        stride = max([t.target for t in trackers], default=1)
        o_ids, o_ages = np.zeros((max(k, 1), stride), np.int32), np.zeros((max(k, 1), stride), np.int32)
        o_xy, o_prev = np.zeros((max(k, 1), stride, 2), np.float32), np.zeros((max(k, 1), stride, 2), np.float32)
        o_n, counts = np.zeros(max(k, 1), np.int32), np.zeros((max(k, 1), 8), np.int32)
        fn = self.lib.pmv_klt_step_many
        fn.argtypes = [C.c_void_p, C.c_int, _i32p, _i32p, _i32p, _i32p, _i32p, _f32p, _f32p, C.c_int, _i32p, _i32p]
        self._ck(fn(self.h, k, _p(ids, _i32p), _p(prev_slots, _i32p), _p(cur_slots, _i32p), _p(o_ids, _i32p), _p(o_ages, _i32p), _p(o_xy, _f32p), _p(o_prev, _f32p), stride,
                    _p(o_n, _i32p), _p(counts, _i32p)))
        return [(o_ids[j, :o_n[j]].copy(), o_ages[j, :o_n[j]].copy(), o_xy[j, :o_n[j]].copy(), o_prev[j, :o_n[j]].copy(), counts[j].copy()) for j in range(k)]

    def klt_step_many_stereo(self, trackers, prev_slots, cur_slots, right_slots):
        """pmv_klt_step_many_stereo: klt_step_many with stage 8 - a list of KltTracker.step_stereo's 7-tuples, one per tracker, each byte for
        byte what its own step_stereo returns. right_slots[j] < 0: tracker j has no right frame in this call - step()'s bytes, right_status
        all 0 and right_xy zeros."""
        trackers = list(trackers)
        for t in trackers:
            if not isinstance(t, KltTracker) or t.ctx is not self or t.id is None:
                raise ValueError("klt_step_many_stereo: every tracker must be an open KltTracker of this context")
        k = len(trackers)
        prev_slots, cur_slots = np.ascontiguousarray(prev_slots, np.int32).reshape(-1), np.ascontiguousarray(cur_slots, np.int32).reshape(-1)
        right_slots = np.ascontiguousarray(right_slots, np.int32).reshape(-1)
        if prev_slots.size != k or cur_slots.size != k or right_slots.size != k:
            raise ValueError("klt_step_many_stereo: one prev_slot, one cur_slot and one right_slot per tracker")
        ids = np.asarray([t.id for t in trackers], np.int32)
        stride = max([t.target for t in trackers], default=1)
        o_ids, o_ages = np.zeros((max(k, 1), stride), np.int32), np.zeros((max(k, 1), stride), np.int32)
        o_xy, o_prev, o_rxy = (np.zeros((max(k, 1), stride, 2), np.float32) for _ in range(3))
        o_rst = np.zeros((max(k, 1), stride), np.uint8)
        o_n, counts = np.zeros(max(k, 1), np.int32), np.zeros((max(k, 1), 8), np.int32)
        fn = self.lib.pmv_klt_step_many_stereo
        fn.argtypes = [C.c_void_p, C.c_int, _i32p, _i32p, _i32p, _i32p, _i32p, _i32p, _f32p, _f32p, _f32p, _u8p, C.c_int, _i32p, _i32p]
        self._ck(fn(self.h, k, _p(ids, _i32p), _p(prev_slots, _i32p), _p(cur_slots, _i32p), _p(right_slots, _i32p), _p(o_ids, _i32p), _p(o_ages, _i32p), _p(o_xy, _f32p),
                    _p(o_prev, _f32p), _p(o_rxy, _f32p), _p(o_rst, _u8p), stride, _p(o_n, _i32p), _p(counts, _i32p)))
        return [(o_ids[j, :o_n[j]].copy(), o_ages[j, :o_n[j]].copy(), o_xy[j, :o_n[j]].copy(), o_prev[j, :o_n[j]].copy(), counts[j].copy(), o_rxy[j, :o_n[j]].copy(),
                 o_rst[j, :o_n[j]].copy()) for j in range(k)]

    def debug_klt_stereo_stats(self):
        """pmv_debug_klt_stereo_stats: [stereo steps, stereo many-calls, host waits inside both, kernel launches inside both]"""
        out = (C.c_longlong * 4)()
        self.lib.pmv_debug_klt_stereo_stats.argtypes = [C.c_void_p, C.POINTER(C.c_longlong)]
        self._ck(self.lib.pmv_debug_klt_stereo_stats(self.h, out))
        return [int(v) for v in out]

    def debug_klt_observe_stats(self):
        """pmv_debug_klt_observe_stats: [step calls with the observation setting on, observe launches, lift-for-F launches, host waits inside
        those calls]"""
        out = (C.c_longlong * 4)()
        self.lib.pmv_debug_klt_observe_stats.argtypes = [C.c_void_p, C.POINTER(C.c_longlong)]
        self._ck(self.lib.pmv_debug_klt_observe_stats(self.h, out))
        return [int(v) for v in out]

    def camera_create(self, **params):
        """pmv_camera_create: the id of a camera of this context. Keywords: camera_params()'s (fx, fy, cx, cy, dist, iters)."""
        p = camera_params(**params)
        out = C.c_int(-1)
        self.lib.pmv_camera_create.argtypes = [C.c_void_p, C.POINTER(CameraParams), C.POINTER(C.c_int)]
        self._ck(self.lib.pmv_camera_create(self.h, C.byref(p), C.byref(out)))
        return out.value

    def camera_create_fisheye(self, fx, fy, cx, cy, k=()):
        """pmv_camera_create_fisheye: the id of a camera of the equidistant model (cv::fisheye, Kalibr "equidistant"); it is a camera id like
        camera_create's wherever one is taken, and camera_destroy frees it."""
        p = fisheye_params(fx, fy, cx, cy, k)
        out = C.c_int(-1)
        self.lib.pmv_camera_create_fisheye.argtypes = [C.c_void_p, C.POINTER(FisheyeParams), C.POINTER(C.c_int)]
        self._ck(self.lib.pmv_camera_create_fisheye(self.h, C.byref(p), C.byref(out)))
        return out.value

    def camera_destroy(self, cam_id):
        self.lib.pmv_camera_destroy.argtypes = [C.c_void_p, C.c_int]
        self._ck(self.lib.pmv_camera_destroy(self.h, int(cam_id)))

    def undistort_points(self, cam_id, xy):
        """pmv_undistort_points: cv::undistortPoints(xy, K, dist) through camera cam_id - (un_xy (n, 2) float32 on the normalised image plane,
        ok (n,) uint8; a point whose lift is not finite has ok 0 and un_xy (0, 0))"""
        xy = np.ascontiguousarray(xy, np.float32)
        if xy.size and (xy.ndim != 2 or xy.shape[1] != 2):
            raise ValueError("undistort_points: xy must be an (n, 2) float32 array")
        n = xy.size // 2
        out, ok = np.zeros((max(n, 1), 2), np.float32), np.zeros(max(n, 1), np.uint8)
        src = xy if n else np.zeros((1, 2), np.float32)
        fn = self.lib.pmv_undistort_points
        fn.argtypes = [C.c_void_p, C.c_int, _f32p, C.c_int, _f32p, _u8p]
        self._ck(fn(self.h, int(cam_id), _p(src, _f32p), n, _p(out, _f32p), _p(ok, _u8p)))
        return out[:n].copy(), ok[:n].copy()

    def project_points(self, cam_id, xyz):
        """pmv_project_points: cv::projectPoints(xyz, rvec = tvec = 0, K, dist) through camera cam_id - (xy (n, 2) float32 pixels, ok (n,)
        uint8; a point that is not finite, not in front of the camera or lands beyond 1e6 has ok 0 and xy (0, 0))"""
        xyz = np.ascontiguousarray(xyz, np.float64)
        if xyz.size and (xyz.ndim != 2 or xyz.shape[1] != 3):
            raise ValueError("project_points: xyz must be an (n, 3) float64 array")
        n = xyz.size // 3
        out, ok = np.zeros((max(n, 1), 2), np.float32), np.zeros(max(n, 1), np.uint8)
        src = xyz if n else np.zeros((1, 3), np.float64)
        fn = self.lib.pmv_project_points
        fn.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_double), C.c_int, _f32p, _u8p]
        self._ck(fn(self.h, int(cam_id), _p(src, C.POINTER(C.c_double)), n, _p(out, _f32p), _p(ok, _u8p)))
        return out[:n].copy(), ok[:n].copy()

    def debug_klt_many_stats(self):
        """pmv_debug_klt_many_stats: [many-calls, trackers stepped by them, host waits inside them, kernel launches inside them]"""
        out = (C.c_longlong * 4)()
        self.lib.pmv_debug_klt_many_stats.argtypes = [C.c_void_p, C.POINTER(C.c_longlong)]
        self._ck(self.lib.pmv_debug_klt_many_stats(self.h, out))
        return [int(v) for v in out]

    # ---- call log (teacher-forced replay) ----
    def record_enable(self, on=True):
        self._ck(self.lib.pmv_record_enable(self.h, 1 if on else 0))

    def records(self):
        """the logged back-end calls as dicts (kind 'pnp' | 'ba' | 'dlt') with numpy views of inputs and outputs"""
        self.lib.pmv_record_size.restype = C.c_longlong
        self.lib.pmv_record_size.argtypes = [C.c_void_p, C.c_int]
        self.lib.pmv_record_get.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_longlong]
        out = []
        for i in range(self.lib.pmv_record_count(self.h)):
            nb = self.lib.pmv_record_size(self.h, i)
            buf = np.zeros(nb, np.uint8)
            self._ck(self.lib.pmv_record_get(self.h, i, buf.ctypes.data_as(C.c_void_p), nb))
            out.append(parse_record(buf))
        return out

    # ---- per-kernel HIP-event timing ----
    def prof_enable(self, on=True):
        self._ck(self.lib.pmv_prof_enable(self.h, 1 if on else 0))

    def lk_counters(self, reset=False):
        """(LK iterations, (track, level) passes, tracks) executed by k_lk since the last reset"""
        out = (C.c_ulonglong * 3)()
        self._ck(self.lib.pmv_lk_counters(self.h, out, 1 if reset else 0))
        return int(out[0]), int(out[1]), int(out[2])

    def prof_select(self, names):
        """after prof_enable(True): record only the named kernel classes"""
        self.lib.pmv_prof_kernel_name.restype = C.c_char_p
        mask = 0
        for i in range(self.lib.pmv_prof_kernel_count()):
            if self.lib.pmv_prof_kernel_name(i).decode() in names:
                mask |= 1 << i
        self._ck(self.lib.pmv_prof_select(self.h, C.c_uint(mask)))

    def prof_read(self):
        """{kernel: (launches, total_ms, max_ms)} for every kernel class launched since prof_enable(True)"""
        self.lib.pmv_prof_kernel_name.restype = C.c_char_p
        out = {}
        for i in range(self.lib.pmv_prof_kernel_count()):
            n, tot, mx = C.c_int(), C.c_double(), C.c_double()
            self._ck(self.lib.pmv_prof_read(self.h, i, C.byref(n), C.byref(tot), C.byref(mx)))
            if n.value:
                out[self.lib.pmv_prof_kernel_name(i).decode()] = (n.value, tot.value, mx.value)
        return out

    # ---- whole sequence (OdometryPipeline role) ----
    def pipeline_run(self, n_frames, w, h, K, gt_poses, min_tracked=400, tol=150, init_frames=5, bundle_size=5,
                     ba_iterations=5, extractor=0, threaded=0, build_pyramids=1, want_features=True, n_threads=1, async_free=False,
                     defer_free=False, host_frames=None, matcher=0, device_fivepoint=0):
        """frames 0..n_frames-1 must be staged in slots 0..n_frames-1 (frames_stage) unless host_frames (n, h, w) uint8 ((n, h, w, 3) BGR after
        set_frame_format("bgr")) is given:
        then they are streamed from host memory while the pipeline runs (pmv_pipeline_run_streamed). n_threads: host threads that
        evaluate the five-point RANSAC hypotheses of the triangulator side by side (the results do not depend on it)"""
        P = PipelineParams(n_frames, w, h, min_tracked, tol, init_frames, bundle_size, ba_iterations, extractor, threaded,
                           n_threads, build_pyramids, matcher, device_fivepoint)
        Kd = np.ascontiguousarray(K, np.float64).reshape(9)
        gt = np.ascontiguousarray(gt_poses, np.float64).reshape(n_frames, 12)
        out = C.c_void_p()
        if host_frames is not None:
            hf = _host_frames(host_frames, self.frame_format, "pipeline_run: host_frames", h, w, n_frames)
            self._ck(self.lib.pmv_pipeline_run_streamed(self.h, C.byref(P), _p(Kd, _f64p), _p(gt, _f64p), _p(hf, _u8p), C.byref(out)))
        else:
            self._ck(self.lib.pmv_pipeline_run(self.h, C.byref(P), _p(Kd, _f64p), _p(gt, _f64p), C.byref(out)))
        # Tearing down the ~10^6 host-container nodes of a long run takes ~40 ms and is not part of the path. defer_free: the
        # caller frees later (result.free()); async_free: a background thread does it (pipeline_drain() joins).
        ok = False
        try:
            r = PipelineResult(self.lib, out, want_features)
            ok = True
        finally:
            if not (ok and defer_free):
                if async_free:
                    self.lib.pmv_pipeline_release(out)
                else:
                    self.lib.pmv_pipeline_free(out)
        if defer_free:
            r._deferred = (self.lib, out)
        return r

    def pipeline_run_batch(self, seqs, w, h, K, min_tracked=400, tol=150, init_frames=5, bundle_size=5, ba_iterations=5, extractor=0,
                           build_pyramids=1, want_features=True, defer_free=False, threaded=1, device_fivepoint=0, matcher=0):
        """B independent sequences through batched launches (pmv_pipeline_run_batch). seqs: list of (first_slot, n_frames, gt_poses);
        the frames must be staged in slots first_slot..first_slot+n_frames-1. w, h: the frame size, one int for all sequences or B ints
        (sequences of different sizes may share a batch; each must name the size staged in its slots). K: 9 values shared by all, or (B, 9). extractor (0 GFTT,
        1 ShiTomasi, 2 FAST) and matcher (0 LK, 1 kNN, which needs extractor 2): one int for all sequences or B ints, every pair
        pipeline_run accepts; sequences with different pairs may share a batch. Returns one PipelineResult per sequence (bit-identical to
        pipeline_run on the same sequence)."""
        B = len(seqs)
        extractor = _per_sequence("pipeline_run_batch", "extractor", extractor, B)
        matcher = _per_sequence("pipeline_run_batch", "matcher", matcher, B)
        w = _per_sequence("pipeline_run_batch", "w", w, B)
        h = _per_sequence("pipeline_run_batch", "h", h, B)
        params = (PipelineParams * B)()
        gts = []
        gt_ptrs = (_f64p * B)()
        first = (C.c_int * B)()
        Kd = np.ascontiguousarray(np.broadcast_to(np.asarray(K, np.float64).reshape(-1, 9), (B, 9)))
        for b, (fs, n, gt) in enumerate(seqs):
            params[b] = PipelineParams(n, w[b], h[b], min_tracked, tol, init_frames, bundle_size, ba_iterations, extractor[b], threaded, 1, build_pyramids, matcher[b],
                                       device_fivepoint)
            g = np.ascontiguousarray(gt, np.float64).reshape(n, 12)
            gts.append(g)
            gt_ptrs[b] = _p(g, _f64p)
            first[b] = fs
        outs = (C.c_void_p * B)()
        self.lib.pmv_pipeline_run_batch.argtypes = [C.c_void_p, C.c_int, C.POINTER(PipelineParams), _f64p, C.POINTER(_f64p), _i32p, C.POINTER(C.c_void_p)]
        self._ck(self.lib.pmv_pipeline_run_batch(self.h, B, params, _p(Kd, _f64p), gt_ptrs, first, outs))
        res = []
        for b in range(B):
            hnd = C.c_void_p(outs[b])
            r = PipelineResult(self.lib, hnd, want_features)
            if defer_free:
                r._deferred = (self.lib, hnd)
            else:
                self.lib.pmv_pipeline_free(hnd)
            res.append(r)
        return res

    def pipeline_run_batch_streamed(self, seqs, w=None, h=None, K=None, ring=16, first_slot=None, min_tracked=400, tol=150, init_frames=5, bundle_size=5,
                                    ba_iterations=5, extractor=0, build_pyramids=1, want_features=True, defer_free=False, threaded=1,
                                    device_fivepoint=0, matcher=0):
        """B sequences streamed from host memory through rings of `ring` frame slots (pmv_pipeline_run_batch_streamed). seqs: list of
        (frames (n, h, w) uint8 - (n, h, w, 3) BGR after set_frame_format("bgr") -, gt_poses (n, 12)); the frames are read where they are (numpy arrays, also over pinned memory such as a
        torch pin_memory() tensor's .numpy(); several entries may share one array) and must stay alive during the call. w, h: one int for
        all sequences, B ints, or None = each sequence's own array shape (sequences of different sizes may share a batch); a given size
        that an array does not match is a ValueError. first_slot:
        sequence b's ring starts there (default b * ring). Other arguments as pipeline_run_batch; build_pyramids is ignored. Returns one
        PipelineResult per sequence, bit-identical to pipeline_run_batch on the same frames staged."""
        if K is None:
            raise ValueError("pipeline_run_batch_streamed: K (9 values, or (B, 9)) is required")
        frames, gts, first = _batch_streamed_args(seqs, w, h, ring, first_slot, self.frame_format)
        B = len(frames)
        extractor = _per_sequence("pipeline_run_batch_streamed", "extractor", extractor, B)
        matcher = _per_sequence("pipeline_run_batch_streamed", "matcher", matcher, B)
        params = (PipelineParams * B)()
        gt_ptrs = (_f64p * B)()
        src = (_u8p * B)()
        fs = (C.c_int * B)(*first)
        Kd = np.ascontiguousarray(np.broadcast_to(np.asarray(K, np.float64).reshape(-1, 9), (B, 9)))
        for b in range(B):
            params[b] = PipelineParams(frames[b].shape[0], frames[b].shape[2], frames[b].shape[1], min_tracked, tol, init_frames, bundle_size, ba_iterations, extractor[b], threaded, 1,
                                       build_pyramids, matcher[b], device_fivepoint)
            gt_ptrs[b] = _p(gts[b], _f64p)
            src[b] = _p(frames[b], _u8p)
        outs = (C.c_void_p * B)()
        self.lib.pmv_pipeline_run_batch_streamed.argtypes = [C.c_void_p, C.c_int, C.POINTER(PipelineParams), _f64p, C.POINTER(_f64p),
                                                             C.POINTER(_u8p), _i32p, C.c_int, C.POINTER(C.c_void_p)]
        self._ck(self.lib.pmv_pipeline_run_batch_streamed(self.h, B, params, _p(Kd, _f64p), gt_ptrs, src, fs, int(ring), outs))
        res = []
        for b in range(B):
            hnd = C.c_void_p(outs[b])
            r = PipelineResult(self.lib, hnd, want_features)
            if defer_free:
                r._deferred = (self.lib, hnd)
            else:
                self.lib.pmv_pipeline_free(hnd)
            res.append(r)
        return res

    def batch_ingest_stats(self):
        """ingest counters of the last pipeline_run_batch_streamed call (include/pmv_hip.h, pmv_batch_ingest_stats)"""
        self.lib.pmv_batch_ingest_stats.argtypes = [C.c_void_p, _f64p]
        n = self.lib.pmv_batch_ingest_stats(None, None)   # the count the library writes
        out = np.zeros(n, np.float64)
        self._ck(min(self.lib.pmv_batch_ingest_stats(self.h, _p(out, _f64p)), 0))
        return dict(zip(BATCH_INGEST_KEYS, [float(v) for v in out]))

    def batch_launches(self):
        """launches of the batched legs since the context was created (pmv_debug_batch_launches): k_lk_batch, k_knn_round, k_pad_level0
        (gray or BGR), k_pyrdown"""
        out = (C.c_longlong * 4)()
        self.lib.pmv_debug_batch_launches.argtypes = [C.c_void_p, C.POINTER(C.c_longlong)]
        self._ck(self.lib.pmv_debug_batch_launches(self.h, out))
        return dict(zip(("k_lk_batch", "k_knn_round", "k_pad_level0", "k_pyrdown"), [int(v) for v in out]))

    def batch_stats(self):
        """per combiner of the batch engine (lk, det, pnp, ba, dlt): launch rounds, requests served, CPU seconds of the thread, wall seconds processing batches / of that waiting for the GPU"""
        cnt = (C.c_longlong * 10)()
        t = (C.c_double * 15)()
        self.lib.pmv_batch_stats(self.h, cnt, t)
        out = {}
        for r, name in enumerate(("lk", "det", "pnp", "ba", "dlt")):
            out[name] = dict(launches=int(cnt[2 * r]), requests=int(cnt[2 * r + 1]), cpu_s=t[3 * r], work_s=t[3 * r + 1], sync_s=t[3 * r + 2])
        return out

    def pipeline_drain(self):
        self.lib.pmv_pipeline_drain()

    # ---- batch sessions: the batch engine for callers who bring their own pipeline (include/pmv_hip.h, "batch sessions") ----
    # Every batch_* call may be made from any Python thread: ctypes releases the GIL during a call, so the threads' requests do meet in
    # the combiners' launches. Each returns exactly what the call without the prefix returns.
    def batch_open(self, n_seq, sizes):
        """opens a session: n_seq back-end workspace sets (seq = 0 .. n_seq - 1), sizes = the (w, h) pairs of every frame the session will see"""
        if isinstance(n_seq, (bool, np.bool_)) or not isinstance(n_seq, (int, np.integer)) or n_seq < 1:
            raise ValueError(f"batch_open: n_seq must be a positive integer, got {n_seq!r}")
        wh = _session_sizes(sizes)
        self._ckt(self.lib.pmv_batch_open(self.h, int(n_seq), _p(wh, _i32p), len(wh) // 2))

    def batch_close(self):
        self._ckt(self.lib.pmv_batch_close(self.h))

    def batch_session(self, n_seq, sizes):
        """with ctx.batch_session(n_seq, sizes): ... - batch_open on entry, batch_close on exit"""
        import contextlib

        @contextlib.contextmanager
        def session():
            self.batch_open(n_seq, sizes)
            try:
                yield self
            finally:
                self.batch_close()
        return session()

    def batch_frame_upload(self, slot, frame, fmt="gray", clahe=None):
        """one frame into `slot` through the session's upload class (see _upload_source for what `frame` may be); returns when the slot's
        pyramid is built. A pinned or device source is read in place by a kernel on the session's own stream: the work that produced it (a
        torch op on torch's stream, say) must have completed - torch.cuda.synchronize() or a blocking copy - before this call.
        clahe: None, or (clip_limit, (tiles_x, tiles_y)) - level 0 is equalised inside the same upload round (pmv_batch_frame_upload_clahe)"""
        p = None
        if clahe is not None:
            try:
                clip_limit, tiles = clahe
            except (TypeError, ValueError):
                raise ValueError(f"batch_frame_upload: clahe is None or (clip_limit, (tiles_x, tiles_y)), got {clahe!r}") from None
            p = _clahe_params("batch_frame_upload", clip_limit, tiles)
        addr, w, h, stride, f, keep = _upload_source(frame, fmt)
        if p is None:
            self._ckt(self.lib.pmv_batch_frame_upload(self.h, int(slot), C.c_void_p(addr), w, h, stride, f))
        else:
            self.lib.pmv_batch_frame_upload_clahe.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(ClaheParams)]
            self._ckt(self.lib.pmv_batch_frame_upload_clahe(self.h, int(slot), C.c_void_p(addr), w, h, stride, f, C.byref(p)))
        del keep

    def batch_frame_upload_remap(self, slot, frame, remap, fmt="gray", clahe=None):
        """batch_frame_upload with the remap of frames_remap inside the same upload round (pmv_batch_frame_upload_remap). remap: a map id or
        (map_id, border_value). clahe: None, or (clip_limit, (tiles_x, tiles_y)) - equalised behind the remap, in the same round. A colour frame
        is converted first: conversion, remap, equalisation."""
        map_id, border = _remap_arg("batch_frame_upload_remap", remap)
        p = None
        if clahe is not None:
            try:
                clip_limit, tiles = clahe
            except (TypeError, ValueError):
                raise ValueError(f"batch_frame_upload_remap: clahe is None or (clip_limit, (tiles_x, tiles_y)), got {clahe!r}") from None
            p = _clahe_params("batch_frame_upload_remap", clip_limit, tiles)
        addr, w, h, stride, f, keep = _upload_source(frame, fmt)
        self.lib.pmv_batch_frame_upload_remap.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(ClaheParams)]
        self._ckt(self.lib.pmv_batch_frame_upload_remap(self.h, int(slot), C.c_void_p(addr), w, h, stride, f, map_id, border, None if p is None else C.byref(p)))
        del keep

    def batch_upload_stats(self):
        """{rounds, frames, level0_launches, pyrdown_launches} of the upload class since batch_open"""
        out = (C.c_longlong * 4)()
        self._ckt(self.lib.pmv_batch_upload_stats(self.h, out))
        return dict(zip(BATCH_UPLOAD_KEYS, [int(v) for v in out]))

    def batch_upload_rounds(self):
        """one dict per upload round since batch_open (pmv_batch_upload_rounds): frames_by_levels (frames whose pyramid has 1..5 levels),
        level0_launches, pyrdown_launches, in_place (frames read where the caller has them; the others came through the staging pool)"""
        n = self.lib.pmv_batch_upload_rounds(self.h, None, 0)
        self._ckt(min(n, 0))
        out = np.zeros((max(n, 1), 8), np.int32)
        self._ckt(min(self.lib.pmv_batch_upload_rounds(self.h, _p(out, _i32p), n), 0))
        return [dict(frames_by_levels=[int(v) for v in r[:5]], level0_launches=int(r[5]), pyrdown_launches=int(r[6]), in_place=int(r[7])) for r in out[:n]]

    # ---- the plugin calls as session calls: the single call's marshalling (same arguments, same arrays), the thread's own error text
    def batch_detect_gftt(self, slot, cells, max_per_cell, quality=0.01, min_dist=5.0):
        return self._detect_gftt(self.lib.pmv_batch_detect_gftt, self._ckt, slot, cells, max_per_cell, quality, min_dist)

    def batch_detect_gftt_ex(self, slot, cells, max_per_cell, quality=0.01, min_dist=5.0, mask=None, block_size=3, use_harris=False, k=0.04):
        """pmv_batch_detect_gftt_ex: detect_gftt_ex as a session call (same arguments, same arrays)"""
        return self._gftt_ex(self.lib.pmv_batch_detect_gftt_ex, self._ckt, slot, cells, max_per_cell, quality, min_dist, mask, block_size, use_harris, k)

    def batch_detect_gftt_frame(self, slot, max_corners, quality=0.01, min_dist=5.0, mask=None, block_size=3, use_harris=False, k=0.04, roi=None, out_cap=None):
        """pmv_batch_detect_gftt_frame: detect_gftt_frame as a session call (same arguments, same array)"""
        return self._gftt_frame(self.lib.pmv_batch_detect_gftt_frame, self._ckt, slot, max_corners, quality, min_dist, mask, block_size, use_harris, k, roi, out_cap)

    def batch_detect_gftt_refill(self, slot, max_corners, tracks, radius, priorities=None, base_mask=None, quality=0.01, min_dist=5.0, block_size=3, use_harris=False,
                                 k=0.04, roi=None, out_cap=None):
        """pmv_batch_detect_gftt_refill: detect_gftt_refill as a session call (same arguments, same arrays)"""
        return self._gftt_refill(self.lib.pmv_batch_detect_gftt_refill, self._ckt, slot, max_corners, tracks, radius, priorities, base_mask, quality, min_dist,
                                 block_size, use_harris, k, roi, out_cap)

    def batch_corner_subpix(self, slot, xy, win=(5, 5), zero_zone=(-1, -1), max_iter=30, eps=0.01, return_info=False):
        """pmv_batch_corner_subpix: corner_subpix as a session call (same arguments, same arrays)"""
        return self._corner_subpix(self.lib.pmv_batch_corner_subpix, self._ckt, slot, xy, win, zero_zone, max_iter, eps, return_info)

    def batch_detect_shitomasi(self, slot, cells, max_per_cell, quality=0.4):
        return self._detect_shitomasi(self.lib.pmv_batch_detect_shitomasi, self._ckt, slot, cells, max_per_cell, quality)

    def batch_detect_fast(self, slot, cells, max_per_cell, threshold=10, nonmax=True):
        return self._detect_fast(self.lib.pmv_batch_detect_fast, self._ckt, slot, cells, max_per_cell, threshold, nonmax)

    def batch_knn_match(self, src_slot, cmp_slot, src_xy, cmp_xy, neighbours=7, window=15):
        return self._knn_match(self.lib.pmv_batch_knn_match, self._ckt, src_slot, cmp_slot, src_xy, cmp_xy, neighbours, window)

    def batch_lk_track(self, prev_slot, next_slot, prev_xy):
        return self._lk_track(self.lib.pmv_batch_lk_track, self._ckt, prev_slot, next_slot, prev_xy)

    def batch_lk_track_ex(self, prev_slot, next_slot, prev_xy, init_xy=None, min_eigenvals=False):
        """lk_track_ex as a session call (pmv_batch_lk_track_ex)"""
        return self._lk_ex(self.lib.pmv_batch_lk_track_ex, self._ckt, False, prev_slot, next_slot, prev_xy, init_xy, min_eigenvals)

    def batch_lk_track_fb(self, prev_slot, next_slot, prev_xy, init_xy=None, min_eigenvals=False):
        """lk_track_fb as a session call (pmv_batch_lk_track_fb)"""
        return self._lk_ex(self.lib.pmv_batch_lk_track_fb, self._ckt, True, prev_slot, next_slot, prev_xy, init_xy, min_eigenvals)

    def batch_pnp_ransac(self, seq, obj_xyz, img_xy, K, rvec, tvec, iterations=100, reproj_err=8.0, confidence=0.99):
        return self._pnp_ransac(self.lib.pmv_batch_pnp_ransac, self._ckt, (int(seq),), obj_xyz, img_xy, K, rvec, tvec, iterations, reproj_err, confidence)

    def batch_ba_solve(self, seq, cams, pts, obs_xy, cam_idx, pt_idx, K, huber=1.0, max_iterations=5):
        return self._ba_solve(self.lib.pmv_batch_ba_solve, self._ckt, (int(seq),), cams, pts, obs_xy, cam_idx, pt_idx, K, huber, max_iterations)

    def batch_triangulate_candidates(self, seq, q1, q2, P1x4, mask_in):
        return self._triangulate_candidates(self.lib.pmv_batch_triangulate_candidates, self._ckt, (int(seq),), q1, q2, P1x4, mask_in)

    def batch_triangulate_tracks(self, seq, P3x4, obs_xy, cam_idx, pt_idx, n_points, params=None):
        """triangulate_tracks for sequence `seq` of the session: the round's requests of this kind share one launch"""
        return self._triangulate_tracks(self.lib.pmv_batch_triangulate_tracks, self._ckt, (int(seq),), P3x4, obs_xy, cam_idx, pt_idx, n_points, params)

    def batch_fivepoint_hypotheses(self, seq, q1, q2, samples, thr):
        return self._fivepoint_hypotheses(self.lib.pmv_batch_fivepoint_hypotheses, self._ckt, (int(seq),), q1, q2, samples, thr)

    def batch_find_essential_mat(self, seq, p1, p2, K, prob=0.99, threshold=1.0):
        """find_essential_mat for sequence `seq` of the session: returns when its own request is complete, not when its round's launch is"""
        return self._find_essential(self.lib.pmv_batch_find_essential_mat, self._ckt, (int(seq),), p1, p2, K, prob, threshold)

    def batch_find_fundamental_mat(self, seq, p1, p2, threshold=1.0, confidence=0.99):
        """find_fundamental_mat for sequence `seq` of the session: returns when its own request is complete, not when its round's launch is"""
        return self._find_fundamental(self.lib.pmv_batch_find_fundamental_mat, self._ckt, (int(seq),), p1, p2, threshold, confidence)

    def batch_find_homography(self, seq, p1, p2, threshold=3.0, confidence=0.995, max_iters=2000):
        """find_homography for sequence `seq` of the session: returns when its own request is complete, not when its round's launch is"""
        return self._find_homography(self.lib.pmv_batch_find_homography, self._ckt, (int(seq),), p1, p2, threshold, confidence, max_iters)

    def batch_recover_pose(self, seq, E, p1, p2, K, mask):
        return self._recover_pose(self.lib.pmv_batch_recover_pose, self._ckt, (int(seq),), E, p1, p2, K, mask)
