"""Shared by the tests of pmv_corner_subpix: the CPU twin (tests/twin/subpix_twin.cpp, compiled on first use) and the scenes.

Frames and caching come from gftt_common. Points: the corners of all grid cells of the 160x120 and 203x87 frames with no limit, in frame
coordinates, shifted by (+0.3, -0.2); an edge set per frame. Everything handed out is computed once and shared; callers must not modify it."""
import ctypes as C
import os
import subprocess

import numpy as np

import gftt_common as gc

TW = gc.TW
SIZES = gc.SIZES
KERNEL, SERIAL = 1, 0          # the `order` argument of the twin: the kernel's summation order, cv's raster order
DET, LEFT, CAP, REVERTED = 1, 2, 4, 8   # out_flags
_u8p, _f32p, _i32p = C.POINTER(C.c_uint8), C.POINTER(C.c_float), C.POINTER(C.c_int32)
# (win_w, win_h | zero_w, zero_h | max_iter | eps)
PARAMS = {
    "default": dict(win=(5, 5), zero_zone=(-1, -1), max_iter=30, eps=0.01),
    "win1": dict(win=(1, 1), zero_zone=(-1, -1), max_iter=30, eps=0.01),
    "win3x7_zero1": dict(win=(3, 7), zero_zone=(1, 1), max_iter=40, eps=0.001),
    "win15_full": dict(win=(15, 15), zero_zone=(-1, -1), max_iter=100, eps=0.0),
    "zero0": dict(win=(5, 5), zero_zone=(0, 0), max_iter=30, eps=0.01),
    "zero_ignored": dict(win=(5, 5), zero_zone=(5, 5), max_iter=30, eps=0.01),
    "one_iter": dict(win=(5, 5), zero_zone=(-1, -1), max_iter=1, eps=0.01),
}


def _p(a, t):
    return a.ctypes.data_as(t)


class Twin:
    def __init__(self, lib):
        self.lib = lib

    def table(self, win, zero_zone=(-1, -1)):
        out = np.zeros((2 * win[1] + 1, 2 * win[0] + 1), np.float32)
        self.lib.subpix_twin_table(int(win[0]), int(win[1]), int(zero_zone[0]), int(zero_zone[1]), _p(out, _f32p))
        return out

    def patch(self, img, cx, cy, win):
        """(the (2 win_h + 3) x (2 win_w + 3) float patch of getRectSubPix around (cx, cy), True when the interior fast path was taken)"""
        img = np.ascontiguousarray(img, np.uint8)
        h, w = img.shape
        out = np.zeros((2 * win[1] + 3, 2 * win[0] + 3), np.float32)
        self.lib.subpix_twin_patch.argtypes = [_u8p, C.c_int, C.c_int, C.c_float, C.c_float, C.c_int, C.c_int, _f32p]
        fast = self.lib.subpix_twin_patch(_p(img, _u8p), w, h, C.c_float(cx), C.c_float(cy), int(win[0]), int(win[1]), _p(out, _f32p))
        return out, bool(fast)

    def refine(self, img, xy, win=(5, 5), zero_zone=(-1, -1), max_iter=30, eps=0.01, order=KERNEL):
        """(positions (n, 2) float32, updates (n,) uint8, flags (n,) uint8, iterations on the interior path (n,) int32)"""
        img = np.ascontiguousarray(img, np.uint8)
        h, w = img.shape
        out = np.ascontiguousarray(xy, np.float32).reshape(-1, 2).copy()
        n = len(out)
        it, fl, fast = np.zeros(n, np.uint8), np.zeros(n, np.uint8), np.zeros(n, np.int32)
        self.lib.subpix_twin_refine.argtypes = [_u8p, C.c_int, C.c_int, _f32p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int,
                                                _u8p, _u8p, _i32p]
        self.lib.subpix_twin_refine(_p(img, _u8p), w, h, _p(out, _f32p), n, int(win[0]), int(win[1]), int(zero_zone[0]), int(zero_zone[1]), int(max_iter),
                                    C.c_double(eps), int(order), _p(it, _u8p), _p(fl, _u8p), _p(fast, _i32p))
        return out, it, fl, fast


def twin():
    def make():
        so, src = os.path.join(TW, "libsubpix_twin.so"), os.path.join(TW, "subpix_twin.cpp")
        if not os.path.exists(so) or os.path.getmtime(so) < os.path.getmtime(src):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", "-Wall", src, "-o", so])
        return Twin(C.CDLL(so))
    return gc.cached("subpix_twin", make)


def scene_points(pmv, w, h):
    """the corners of all grid cells (no limit, the detector's twin), frame coordinates, shifted by (+0.3, -0.2): (n, 2) float32"""
    def make():
        img = gc.frame(pmv, w, h)
        pts = [gc.twin().corners(img, c, 0) + np.asarray(c[:2]) for c in pmv.grid_cells(w, h)]
        return (np.concatenate(pts).astype(np.float32) + np.asarray([0.3, -0.2], np.float32)).astype(np.float32)
    return gc.cached(("subpix_points", w, h), make)


def edge_points(w, h, win=(5, 5)):
    """the frame's corners, points within win + 1 of each border (either side of where the interior path ends), two points outside"""
    ww, wh = win
    pts = [(0, 0), (w - 1, h - 1), (0, h - 1), (w - 1, 0), (-3.5, 10), (w + 2, h / 2)]
    for d in (0.0, 0.4, 1.0, ww + 0.9, ww + 1.0, ww + 1.1, ww + 2.0):
        pts += [(d, h / 2 + 0.25), (w - 1 - d, h / 2 - 0.25)]
    for d in (0.0, 0.4, 1.0, wh + 0.9, wh + 1.0, wh + 1.1, wh + 2.0):
        pts += [(w / 2 + 0.25, d), (w / 2 - 0.25, h - 1 - d)]
    pts += [(ww + 1.5, wh + 1.5), (w - ww - 2.5, h - wh - 2.5), (2.25, 3.75), (w - 2.25, h - 3.75)]
    return np.asarray(pts, np.float32)


def refined(pmv, w, h, name, order=KERNEL, edge=False):
    """the twin's result for a scene and a named parameter set, computed once"""
    kw = PARAMS[name]
    pts = edge_points(w, h, kw["win"]) if edge else scene_points(pmv, w, h)
    return gc.cached(("subpix_refined", w, h, name, order, edge), lambda: twin().refine(gc.frame(pmv, w, h), pts, order=order, **kw))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)
