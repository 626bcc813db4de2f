"""Shared by the tests of the lift onto the normalised image plane (pmv_camera_*, pmv_undistort_points, stage 9 of the tracker step): the CPU
twin tests/twin/lift_twin.cpp, built on the fly, and the cameras the tests use. A camera is a dict of pmv.camera_params' keywords."""
import ctypes as C
import os
import subprocess

import numpy as np

import gftt_common as gc

TW = os.path.join(os.path.dirname(os.path.abspath(__file__)), "twin")
_f32p, _f64p, _u8p, _i32p = C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_uint8), C.POINTER(C.c_int)

# EuRoC-like: a 752 x 480 camera with a mild barrel distortion
EUROC = dict(fx=458.654, fy=457.296, cx=367.215, cy=248.375, dist=(-0.28340811, 0.07395907, 1.9359e-4, 1.76187e-5), iters=5)
# the singular case: r2 is exactly 1 at (cx + 512, cy) and the denominator 1 + k1 r2 exactly 0
SINGULAR = dict(fx=512.0, fy=512.0, cx=300.0, cy=200.0, dist=(-1.0,), iters=5)
SINGULAR_POINT = (SINGULAR["cx"] + 512.0, SINGULAR["cy"])


def scene_camera(w, h, k1=-0.3, iters=8, **over):
    """the camera of the tracker scenes (klt_common.scene's intrinsics) with a barrel distortion"""
    return dict(dict(fx=0.58 * w, fy=0.58 * w, cx=w / 2, cy=h / 2, dist=(k1,), iters=iters), **over)


def all_terms(w, h, iters=5):
    """every coefficient of the model non-zero"""
    return dict(fx=0.61 * w, fy=0.57 * w, cx=w / 2 + 3.25, cy=h / 2 - 1.5, dist=(-0.21, 0.05, 1.3e-3, -7e-4, -0.004, 0.012, -0.003, 0.0007), iters=iters)


def dist8(cam):
    d = np.zeros(8)
    d[:len(cam["dist"])] = cam["dist"]
    return d


def cam13(cam):
    return np.ascontiguousarray(np.concatenate([[cam["fx"], cam["fy"], cam["cx"], cam["cy"]], dist8(cam), [cam["iters"]]]), np.float64)


def _p(a, t):
    return None if a is None else a.ctypes.data_as(t)


class Twin:
    def __init__(self, lib):
        self.lib = lib
        lib.lift_twin_points.argtypes = [_f64p, _f32p, C.c_int, _f32p, _u8p]
        lib.lift_twin_observe.argtypes = [_f64p, _f64p, C.c_double, _i32p, _f32p, _f32p, _f32p, _u8p, C.c_int, _f32p, _f32p, _u8p, _f32p, _u8p]
        lib.lift_twin_f_points.argtypes = [_f64p, C.c_double, C.c_int, C.c_int, _f32p, _f32p, C.c_int, _f32p, _f32p]

    def points(self, cam, xy):
        """(un_xy (n, 2) float32, ok (n,) uint8)"""
        xy = np.ascontiguousarray(xy, np.float32).reshape(-1, 2)
        n = len(xy)
        out, ok = np.zeros((n, 2), np.float32), np.zeros(n, np.uint8)
        assert self.lib.lift_twin_points(_p(cam13(cam), _f64p), _p(xy, _f32p), n, _p(out, _f32p), _p(ok, _u8p)) == 0
        return out, ok

    def observe(self, cam, dt, ages, xy, prev_xy, right_cam=None, right_xy=None, right_status=None):
        """stage 9 on a step's outputs: (un_xy, vel, ok, right_un_xy, right_ok); without a right camera or right outputs the right ok bytes
        are 0 and the right xy stay zeros"""
        ages = np.ascontiguousarray(ages, np.int32)
        xy, prev = np.ascontiguousarray(xy, np.float32).reshape(-1, 2), np.ascontiguousarray(prev_xy, np.float32).reshape(-1, 2)
        n = len(xy)
        has_right = right_cam is not None and right_xy is not None
        rxy = np.ascontiguousarray(right_xy, np.float32).reshape(-1, 2) if has_right else None
        rst = np.ascontiguousarray(right_status, np.uint8) if has_right else None
        un, vel, ok = np.zeros((n, 2), np.float32), np.zeros((n, 2), np.float32), np.zeros(n, np.uint8)
        run, rok = np.zeros((n, 2), np.float32), np.zeros(n, np.uint8)
        rc = self.lib.lift_twin_observe(_p(cam13(cam), _f64p), _p(cam13(right_cam), _f64p) if has_right else None, float(dt), _p(ages, _i32p), _p(xy, _f32p), _p(prev, _f32p),
                                        _p(rxy, _f32p), _p(rst, _u8p), n, _p(un, _f32p), _p(vel, _f32p), _p(ok, _u8p), _p(run, _f32p), _p(rok, _u8p))
        assert rc == 0
        return un, vel, ok, run, rok

    def f_points(self, cam, f_focal, w, h, prev_xy, cur_xy):
        """stage 3's two point sets with undistorted_f"""
        a, b = np.ascontiguousarray(prev_xy, np.float32).reshape(-1, 2), np.ascontiguousarray(cur_xy, np.float32).reshape(-1, 2)
        p1, p2 = np.zeros_like(a), np.zeros_like(b)
        assert self.lib.lift_twin_f_points(_p(cam13(cam), _f64p), float(f_focal), int(w), int(h), _p(a, _f32p), _p(b, _f32p), len(a), _p(p1, _f32p), _p(p2, _f32p)) == 0
        return p1, p2


def twin():
    def make():
        so, src = os.path.join(TW, "liblift_twin.so"), os.path.join(TW, "lift_twin.cpp")
        if not os.path.exists(so) or os.path.getmtime(so) < os.path.getmtime(src):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", "-Wall", src, "-o", so])
        return Twin(C.CDLL(so))
    return gc.cached("lift_twin", make)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same(got, want, names):
    for name, g, x in zip(names, got, want):
        assert g.shape == x.shape and g.dtype == x.dtype, f"{name}: {g.dtype}{g.shape} != {x.dtype}{x.shape}"
        assert np.array_equal(bits(g), bits(x)), f"{name} differ"


def forward(cam, x, y):
    """the forward model of pmv_undistort_map_build in float64 numpy: normalised (x, y) -> pixels"""
    k1, k2, p1, p2, k3, k4, k5, k6 = dist8(cam)
    x2, y2, xy2 = x * x, y * y, 2 * x * y
    r2 = x2 + y2
    kr = (1 + ((k3 * r2 + k2) * r2 + k1) * r2) / (1 + ((k6 * r2 + k5) * r2 + k4) * r2)
    xd = x * kr + p1 * xy2 + p2 * (r2 + 2 * x2)
    yd = y * kr + p1 * (r2 + 2 * y2) + p2 * xy2
    return cam["fx"] * xd + cam["cx"], cam["fy"] * yd + cam["cy"]
