"""Shared by the tests of the equidistant (cv::fisheye) camera model (pmv_camera_create_fisheye, pmv_fisheye_map_build): the CPU twin
tests/twin/fisheye_twin.cpp, built on the fly, and the fixture cameras. A fisheye camera is a dict with model="fisheye" and the keywords of
Context.camera_create_fisheye (fx, fy, cx, cy, k); a dict without `model` is a radial-tangential camera of lift_common (pmv.camera_params'
keywords), which the twin restates too, so that a rig of mixed models has one yardstick."""
import ctypes as C
import os
import subprocess

import numpy as np

import gftt_common as gc
from lift_common import bits, same  # noqa: F401  (the comparison of the lift tests)

TW = os.path.join(os.path.dirname(os.path.abspath(__file__)), "twin")
_f32p, _f64p, _u8p, _i32p = C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_uint8), C.POINTER(C.c_int)

PI_2 = float.fromhex("0x1.921fb54442d18p+0")
PI_4 = float.fromhex("0x1.921fb54442d18p-1")

# TUM-VI-like: a 512 x 512 camera of about 190 degrees
TUMVI = dict(model="fisheye", fx=190.97, fy=190.97, cx=254.93, cy=256.90, k=(0.003482, 0.000715, -0.002053, 0.000202))
TUMVI_SIZE = (512, 512)
# every coefficient large enough to matter
ALL_K = dict(model="fisheye", fx=201.5, fy=197.25, cx=250.75, cy=261.5, k=(-0.05, 0.02, -0.01, 0.003))
# the refusing one: theta (1 - theta^2) <= 0.385, so theta_d = 1.0 has no root and the Newton loop cannot settle; fx = fy = 128 and integer
# cx, cy make theta_d of REFUSED_POINT exactly 1.0
REFUSING = dict(model="fisheye", fx=128.0, fy=128.0, cx=256.0, cy=256.0, k=(-1.0, 0.0, 0.0, 0.0))
REFUSED_POINT = (REFUSING["cx"] + 128.0, REFUSING["cy"])
CAMERAS = (("tumvi", TUMVI), ("all_k", ALL_K), ("refusing", REFUSING))


def scene_fisheye(w, h, k=(-0.02, 0.004, -0.001, 0.0002), **over):
    """a fisheye camera with the intrinsics of the tracker scenes (klt_common.scene's)"""
    return dict(dict(model="fisheye", fx=0.58 * w, fy=0.58 * w, cx=w / 2, cy=h / 2, k=k), **over)


def is_fisheye(cam):
    return cam.get("model") == "fisheye"


def cam14(cam):
    c = np.zeros(14)
    c[:4] = cam["fx"], cam["fy"], cam["cx"], cam["cy"]
    if is_fisheye(cam):
        c[4:4 + len(cam["k"])] = cam["k"]
        c[12], c[13] = 10, 1
    else:
        c[4:4 + len(cam["dist"])] = cam["dist"]
        c[12], c[13] = cam["iters"], 0
    return np.ascontiguousarray(c, np.float64)


def create(ctx, cam):
    """the camera on the device, through the constructor of its model"""
    if is_fisheye(cam):
        return ctx.camera_create_fisheye(cam["fx"], cam["fy"], cam["cx"], cam["cy"], k=cam["k"])
    return ctx.camera_create(**cam)


def _p(a, t):
    return None if a is None else a.ctypes.data_as(t)


class Twin:
    def __init__(self, lib):
        self.lib = lib
        for fn in (lib.fisheye_twin_atan, lib.fisheye_twin_tan):
            fn.argtypes, fn.restype = [_f64p, C.c_int, _f64p], None
        lib.fisheye_twin_points.argtypes = [_f64p, _f32p, C.c_int, _f32p, _u8p]
        lib.fisheye_twin_newton.argtypes = [_f64p, C.c_float, C.c_float, _f64p]
        lib.fisheye_twin_project.argtypes = [_f64p, _f64p, C.c_int, _f32p, _u8p]
        lib.fisheye_twin_map.argtypes = [_f64p, _f64p, _f64p, _f64p, C.c_int, C.c_int, _f32p, _f32p]
        lib.fisheye_twin_observe.argtypes = [_f64p, _f64p, C.c_double, _i32p, _f32p, _f32p, _f32p, _u8p, C.c_int, _f32p, _f32p, _u8p, _f32p, _u8p]
        lib.fisheye_twin_f_points.argtypes = [_f64p, C.c_double, C.c_int, C.c_int, _f32p, _f32p, C.c_int, _f32p, _f32p]

    def _fn(self, fn, x):
        x = np.ascontiguousarray(x, np.float64).reshape(-1)
        out = np.zeros_like(x)
        fn(_p(x, _f64p), len(x), _p(out, _f64p))
        return out

    def atan(self, x):
        return self._fn(self.lib.fisheye_twin_atan, x)

    def tan(self, x):
        return self._fn(self.lib.fisheye_twin_tan, x)

    def points(self, cam, xy):
        """pmv_undistort_points: (un_xy (n, 2) float32, ok (n,) uint8)"""
        xy = np.ascontiguousarray(xy, np.float32).reshape(-1, 2)
        n = len(xy)
        out, ok = np.zeros((n, 2), np.float32), np.zeros(n, np.uint8)
        assert self.lib.fisheye_twin_points(_p(cam14(cam), _f64p), _p(xy, _f32p), n, _p(out, _f32p), _p(ok, _u8p)) == 0
        return out, ok

    def newton(self, cam, u, v):
        """(the clamped theta_d of the pixel, theta after the Newton loop, converged)"""
        out = np.zeros(3)
        assert self.lib.fisheye_twin_newton(_p(cam14(cam), _f64p), float(u), float(v), _p(out, _f64p)) == 0
        return float(out[0]), float(out[1]), bool(out[2])

    def project(self, cam, xyz):
        """pmv_project_points: (xy (n, 2) float32, ok (n,) uint8)"""
        xyz = np.ascontiguousarray(xyz, np.float64).reshape(-1, 3)
        n = len(xyz)
        out, ok = np.zeros((n, 2), np.float32), np.zeros(n, np.uint8)
        assert self.lib.fisheye_twin_project(_p(cam14(cam), _f64p), _p(xyz, _f64p), n, _p(out, _f32p), _p(ok, _u8p)) == 0
        return out, ok

    def map_build(self, K, k, size, R=None, new_K=None, fill=None):
        """pmv_fisheye_map_build: (map_x, map_y) float32 (h, w), or None when newK R is singular; fill: the value the maps hold beforehand"""
        w, h = size
        Km, k4 = np.ascontiguousarray(K, np.float64), np.zeros(4)
        k4[:len(k)] = k
        Rm = None if R is None else np.ascontiguousarray(R, np.float64)
        Nm = None if new_K is None else np.ascontiguousarray(new_K, np.float64)
        mx, my = np.full((h, w), 0 if fill is None else fill, np.float32), np.full((h, w), 0 if fill is None else fill, np.float32)
        rc = self.lib.fisheye_twin_map(_p(Km, _f64p), _p(k4, _f64p), _p(Rm, _f64p), _p(Nm, _f64p), w, h, _p(mx, _f32p), _p(my, _f32p))
        return (mx, my) if rc == 0 else None

    def observe(self, cam, dt, ages, xy, prev_xy, right_cam=None, right_xy=None, right_status=None):
        """stage 9 on a step's outputs: (un_xy, vel, ok, right_un_xy, right_ok), as lift_common.Twin.observe, for cameras of either model"""
        ages = np.ascontiguousarray(ages, np.int32)
        xy, prev = np.ascontiguousarray(xy, np.float32).reshape(-1, 2), np.ascontiguousarray(prev_xy, np.float32).reshape(-1, 2)
        n = len(xy)
        has_right = right_cam is not None and right_xy is not None
        rxy = np.ascontiguousarray(right_xy, np.float32).reshape(-1, 2) if has_right else None
        rst = np.ascontiguousarray(right_status, np.uint8) if has_right else None
        un, vel, ok = np.zeros((n, 2), np.float32), np.zeros((n, 2), np.float32), np.zeros(n, np.uint8)
        run, rok = np.zeros((n, 2), np.float32), np.zeros(n, np.uint8)
        rc = self.lib.fisheye_twin_observe(_p(cam14(cam), _f64p), _p(cam14(right_cam), _f64p) if has_right else None, float(dt), _p(ages, _i32p), _p(xy, _f32p),
                                           _p(prev, _f32p), _p(rxy, _f32p), _p(rst, _u8p), n, _p(un, _f32p), _p(vel, _f32p), _p(ok, _u8p), _p(run, _f32p), _p(rok, _u8p))
        assert rc == 0
        return un, vel, ok, run, rok

    def f_points(self, cam, f_focal, w, h, prev_xy, cur_xy):
        """stage 3's two point sets with undistorted_f"""
        a, b = np.ascontiguousarray(prev_xy, np.float32).reshape(-1, 2), np.ascontiguousarray(cur_xy, np.float32).reshape(-1, 2)
        p1, p2 = np.zeros_like(a), np.zeros_like(b)
        assert self.lib.fisheye_twin_f_points(_p(cam14(cam), _f64p), float(f_focal), int(w), int(h), _p(a, _f32p), _p(b, _f32p), len(a), _p(p1, _f32p), _p(p2, _f32p)) == 0
        return p1, p2


def twin():
    def make():
        so, src = os.path.join(TW, "libfisheye_twin.so"), os.path.join(TW, "fisheye_twin.cpp")
        if not os.path.exists(so) or os.path.getmtime(so) < os.path.getmtime(src):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", "-Wall", src, "-o", so])
        return Twin(C.CDLL(so))
    return gc.cached("fisheye_twin", make)


def K_of(cam):
    return np.array([[cam["fx"], 0, cam["cx"]], [0, cam["fy"], cam["cy"]], [0, 0, 1]], np.float64)


def lift_points(cam, size, n, seed):
    """n pixels from -40 to size + 40, then the principal point, a pixel with theta_d just under and just over pi/2 (along +x), and - for
    every camera - the pixel at theta_d = 1.0, which the refusing camera refuses"""
    w, h = size
    rng = np.random.default_rng(seed)
    xy = np.stack([rng.uniform(-40, w + 40, n), rng.uniform(-40, h + 40, n)], axis=1)
    edge = PI_2 * cam["fx"]
    special = [(cam["cx"], cam["cy"]), (cam["cx"] + edge - 0.01, cam["cy"]), (cam["cx"] + edge + 0.01, cam["cy"]), (cam["cx"] + cam["fx"], cam["cy"])]
    return np.concatenate([xy, special]).astype(np.float32)


def project_points(n, seed):
    """n camera-frame points in front of the camera up to about 80 degrees off the axis, then Z = 0, Z < 0, NaN, an infinity, an on-axis point
    (r = 0), r = 1e-9, and a ray at 89.9 degrees"""
    rng = np.random.default_rng(seed)
    ang, az, depth = rng.uniform(0, np.radians(80), n), rng.uniform(0, 2 * np.pi, n), rng.uniform(0.5, 30, n)
    r = np.tan(ang)
    xyz = np.stack([depth * r * np.cos(az), depth * r * np.sin(az), depth], axis=1)
    t = np.tan(np.radians(89.9))
    special = [(0.3, 0.2, 0.0), (0.3, 0.2, -1.0), (np.nan, 0.0, 1.0), (0.0, np.inf, 2.0), (0.0, 0.0, 3.0), (1e-9, 0.0, 1.0), (t * 0.6, t * 0.8, 1.0)]
    return np.concatenate([xyz, special]).astype(np.float64)
