"""Shared by the tests of pmv_frames_remap: the CPU twin (tests/twin/remap_twin.cpp, compiled on first use), the table of cases, their
images and their maps.

Frames and caching come from gftt_common, as in clahe_common. The 160x120 and 203x87 images are the synthetic frames of the LK tests, the
41x40 one is a crop of the noise frame. Everything handed out is computed once and shared; callers must not modify it."""
import ctypes as C
import os
import subprocess

import numpy as np

import gftt_common as gc

TW = gc.TW
_u8p, _i32p, _f32p = C.POINTER(C.c_uint8), C.POINTER(C.c_int32), C.POINTER(C.c_float)

DIST = (-0.35, 0.12, 0.001, -0.0005, -0.02, 0.0, 0.0, 0.0)   # (k1, k2, p1, p2, k3, k4, k5, k6) of the two undistortion rows
SIZES = [(160, 120), (203, 87), (41, 40)]                    # 203: an odd width; 41x40: w h = 1640, 203x87: w h % 4 = 1 (a byte tail)

# (map, w, h, border_value)
CASES = [("identity", 160, 120, 0),
         ("shift", 160, 120, 0), ("shift", 160, 120, 200),          # integer shift (+3, -2): border on two sides
         ("fraction", 160, 120, 0),                                 # (13/32, 27/32) everywhere: one weight set
         ("ties", 160, 120, 0),                                     # every product map * 32 ends in .5: half to even, both directions
         ("turn", 160, 120, 0),                                     # a quarter turn about the centre: worst locality
         ("special", 160, 120, 0)]                                  # NaN, +-inf, +-1e9: those pixels get the border value
CASES += [("undistort", w, h, 0) for w, h in SIZES]                 # new_K = K: everything inside
CASES += [("undistort06", w, h, b) for w, h in SIZES for b in (0, 200)]   # new_K focal lengths x 0.6: border taps on all four sides

# where the "special" map departs from the identity: (row, column, plane, value)
SPECIALS = [(5, 7, "x", np.nan), (5, 8, "y", np.nan), (17, 3, "x", np.inf), (17, 4, "y", np.inf), (40, 100, "x", -np.inf), (41, 100, "y", -np.inf),
            (60, 20, "x", 1e9), (60, 21, "y", 1e9), (90, 150, "x", -1e9), (90, 151, "y", -1e9), (119, 159, "x", np.nan), (0, 0, "y", 3e9)]


def case_id(case):
    name, w, h, border = case
    return f"{name}-{w}x{h}-b{border}"


def _p(a, t):
    return a.ctypes.data_as(t)


class Twin:
    def __init__(self, lib):
        self.lib = lib
        lib.remap_twin_apply.argtypes = [_u8p, C.c_int, C.c_int, _f32p, _f32p, C.c_int, _u8p, _i32p]

    def apply(self, img, map_x, map_y, border=0):
        """(the remapped image, statistics: inside / outside / mixed = pixels whose four taps are all inside the image, all outside, some of
        each; left, right, above, below = mixed pixels with a tap beyond that side; pairs = the set of (fy, fx) seen)"""
        img = np.ascontiguousarray(img, np.uint8)
        mx, my = np.ascontiguousarray(map_x, np.float32), np.ascontiguousarray(map_y, np.float32)
        h, w = img.shape
        assert mx.shape == my.shape == (h, w)
        out = np.zeros_like(img)
        st = np.zeros(8 + 1024, np.int32)
        assert self.lib.remap_twin_apply(_p(img, _u8p), w, h, _p(mx, _f32p), _p(my, _f32p), int(border), _p(out, _u8p), _p(st, _i32p)) == 0
        stats = dict(inside=int(st[0]), outside=int(st[1]), mixed=int(st[2]), left=int(st[3]), right=int(st[4]), above=int(st[5]), below=int(st[6]),
                     pairs={(int(k) // 32, int(k) % 32) for k in np.nonzero(st[8:])[0]})
        return out, stats


def twin():
    def make():
        so, src = os.path.join(TW, "libremap_twin.so"), os.path.join(TW, "remap_twin.cpp")
        if not os.path.exists(so) or os.path.getmtime(so) < os.path.getmtime(src):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", "-Wall", src, "-o", so])
        return Twin(C.CDLL(so))
    return gc.cached("remap_twin", make)


def image(pmv, w, h):
    """the image of the cases of size w x h"""
    def make():
        if (w, h) in gc.SIZES:
            return gc.frame(pmv, w, h)
        return gc.noise_frame()[11:11 + h, 7:7 + w].copy()
    return gc.cached(("remap_image", w, h), make)


def camera(w, h):
    """K of the two undistortion rows at size w x h"""
    f = 0.75 * w
    return np.array([[f, 0.0, (w - 1) / 2 + 1.3], [0.0, 1.02 * f, (h - 1) / 2 - 0.8], [0.0, 0.0, 1.0]])


def new_camera(w, h, scale):
    K = camera(w, h)
    K[0, 0] *= scale
    K[1, 1] *= scale
    return K


def maps(pmv, name, w, h):
    """(map_x, map_y) float32 (h, w) of a row of the table, computed once"""
    def make():
        f32 = np.float32
        j, i = np.meshgrid(np.arange(w, dtype=f32), np.arange(h, dtype=f32))
        if name == "identity":
            return j, i
        if name == "shift":
            return j + f32(3), i - f32(2)
        if name == "fraction":
            return j + f32(13 / 32), i + f32(27 / 32)
        if name == "ties":   # j + k / 64 with odd k: exact in float32, and 32 times it ends in .5
            return (j + ((2 * (np.arange(w) % 32) + 1) / 64).astype(f32)[None, :]).astype(f32), (i + ((2 * (np.arange(h) % 32) + 1) / 64).astype(f32)[:, None]).astype(f32)
        if name == "turn":
            cx, cy = f32((w - 1) / 2), f32((h - 1) / 2)
            return (cx + (i - cy)).astype(f32), (cy - (j - cx)).astype(f32)
        if name == "special":
            mx, my = j.copy(), i.copy()
            for r, c, plane, v in SPECIALS:
                (mx if plane == "x" else my)[r, c] = f32(v)
            return mx, my
        if name == "undistort":
            return pmv.undistort_map(camera(w, h), DIST, (w, h), new_K=camera(w, h))
        if name == "undistort06":
            return pmv.undistort_map(camera(w, h), DIST, (w, h), new_K=new_camera(w, h, 0.6))
        raise KeyError(name)
    return gc.cached(("remap_maps", name, w, h), make)


def remapped(pmv, case):
    """the twin's (image, statistics) for a case of the table, computed once"""
    name, w, h, border = case
    return gc.cached(("remapped", case), lambda: twin().apply(image(pmv, w, h), *maps(pmv, name, w, h), border))
