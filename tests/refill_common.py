"""Shared by the tests of pmv_detect_gftt_refill, next to tests/gftt_common.py and tests/gftt_frame_common.py: the CPU twin of the mask half
(tests/twin/refill_twin.cpp, compiled on first use), the track scenes, and an independent numpy setMask - a sequential walk that paints each
disc row by row from the half-width table, the table itself found by its own restatement of the midpoint recurrence. Everything handed out
is computed once and shared; callers must not modify it."""
import ctypes as C
import os
import subprocess

import numpy as np

import gftt_common as gc

W1, H1 = 517, 261
INVALID, CAPACITY, OVERFLOW = -2, -3, -6
MAX_TRACKS, MAX_RADIUS = 8192, 255
_u8p, _f32p, _i32p = C.POINTER(C.c_uint8), C.POINTER(C.c_float), C.POINTER(C.c_int32)


class Twin:
    def __init__(self, lib):
        self.lib = lib

    def mask(self, w, h, xy, radius, prio=None, base=None):
        """(keep (n,) uint8, mask (h, w) uint8) of setMask; base: None or an (h, w) uint8 view of any row stride"""
        xy = np.ascontiguousarray(xy, np.float32).reshape(-1, 2)
        n = len(xy)
        keep, out = np.zeros(max(n, 1), np.uint8), np.zeros((h, w), np.uint8)
        pp = None if prio is None else np.ascontiguousarray(prio, np.int32)
        bptr, bstride = None, 0
        if base is not None:
            assert base.dtype == np.uint8 and base.shape == (h, w) and base.strides[1] == 1
            bptr, bstride = C.cast(base.ctypes.data, _u8p), base.strides[0]
        rc = self.lib.refill_twin_mask(w, h, xy.ctypes.data_as(_f32p), None if pp is None else pp.ctypes.data_as(_i32p), n, int(radius), bptr, bstride,
                                       keep.ctypes.data_as(_u8p), out.ctypes.data_as(_u8p))
        assert rc >= 0, f"track {-1 - rc} lies outside the frame"
        assert rc == int(keep[:n].sum())
        return keep[:n].copy(), out

    def halfwidths(self, radius):
        out = np.zeros(radius + 1, np.int32)
        self.lib.refill_twin_halfwidths(int(radius), out.ctypes.data_as(_i32p))
        return out

    def circle(self, img, cx, cy, radius, color=0):
        """the literal Circle() painting on `img` ((h, w) uint8, C-contiguous), in place"""
        h, w = img.shape
        self.lib.refill_twin_circle(img.ctypes.data_as(_u8p), w, h, img.strides[0], int(cx), int(cy), int(radius), int(color))

    def positions(self, xy):
        xy = np.ascontiguousarray(xy, np.float32).reshape(-1, 2)
        out = np.zeros(xy.shape, np.int32)
        self.lib.refill_twin_positions(xy.ctypes.data_as(_f32p), len(xy), out.ctypes.data_as(_i32p))
        return out


def twin():
    def make():
        so, src = os.path.join(gc.TW, "librefill_twin.so"), os.path.join(gc.TW, "refill_twin.cpp")
        if not os.path.exists(so) or os.path.getmtime(so) < os.path.getmtime(src):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", "-Wall", src, "-o", so])
        lib = C.CDLL(so)
        lib.refill_twin_mask.restype = C.c_int
        lib.refill_twin_mask.argtypes = [C.c_int, C.c_int, _f32p, _i32p, C.c_int, C.c_int, _u8p, C.c_int, _u8p, _u8p]
        lib.refill_twin_halfwidths.argtypes = [C.c_int, _i32p]
        lib.refill_twin_circle.argtypes = [_u8p] + [C.c_int] * 7
        lib.refill_twin_positions.argtypes = [_f32p, C.c_int, _i32p]
        return Twin(lib)
    return gc.cached("refill-twin", make)


def tracks(w, h, n, seed=5):
    """n uniform random tracks inside a w x h frame, float32 with fractions (never within 0.5 of the right or bottom edge), and int32 ages"""
    def make():
        rng = np.random.default_rng(seed)
        xy = np.stack([rng.uniform(0, w - 1, n), rng.uniform(0, h - 1, n)], axis=1).astype(np.float32)
        xy = np.minimum(xy, np.asarray([w - 1, h - 1], np.float32))
        prio = rng.integers(-5, 40, n).astype(np.int32)   # many ties: the index decides among them
        return xy, prio
    return gc.cached(("refill-tracks", w, h, n, seed), make)


def np_halfwidths(radius):
    """the widest span per row offset of the midpoint circle that cv draws, restated: x runs down from the radius while y runs up, the
    decision variable adds 2y + 1 per step and takes 2x - 1 off when it turns positive; each step gives row y the half-width x and row x the
    half-width y"""
    hw = np.full(radius + 1, -1, np.int64)
    x, y, d = radius, 0, 0
    while x >= y:
        hw[y] = max(hw[y], x)
        hw[x] = max(hw[x], y)
        d += 2 * y + 1
        y += 1
        if d > 0:
            d -= 2 * x - 1
            x -= 1
    return hw


def np_round(xy):
    """round half to even of float32 coordinates"""
    return np.rint(np.asarray(xy, np.float32)).astype(np.int64).reshape(-1, 2)


def np_setmask(w, h, xy, radius, prio=None, base=None):
    """setMask, independently of the twin: (keep, mask)"""
    pts = np_round(xy)
    n = len(pts)
    m = np.full((h, w), 255, np.uint8) if base is None else np.array(base, np.uint8)
    order = np.arange(n) if prio is None else np.lexsort((np.arange(n), -np.asarray(prio, np.int64)))
    hw = np_halfwidths(radius)
    keep = np.zeros(n, np.uint8)
    for i in order:
        x, y = int(pts[i, 0]), int(pts[i, 1])
        if m[y, x] != 255:
            continue
        keep[i] = 1
        for d in range(-radius, radius + 1):
            yy = y + d
            if 0 <= yy < h:
                m[yy, max(x - hw[abs(d)], 0):min(x + hw[abs(d)], w - 1) + 1] = 0
    return keep, m


def base_mask(w, h):
    """a base mask with the bytes 0, 128 and 255 as a view into a larger array (stride above w): a band of 0 on the left, a band of 128
    on the right, 255 between"""
    def make():
        m = np.full((h, w), 255, np.uint8)
        m[:, : w // 5] = 0
        m[:, w - w // 4:] = 128
        m[h // 2: h // 2 + 9, w // 3: w // 3 + 40] = 0
        return gc.roi_mask(m)
    return gc.cached(("refill-base", w, h), make)


def twin_case(w, h, n, radius, with_prio=True, base=None, seed=5):
    """(xy, prio or None, keep, mask) of the twin for the random scene, computed once per case"""
    xy, prio = tracks(w, h, n, seed)
    if not with_prio:
        prio = None
    k, m = gc.cached(("refill-case", w, h, n, radius, with_prio, id(base), seed), lambda: twin().mask(w, h, xy, radius, prio, base))
    return xy, prio, k, m


def raw_refill_call(ctx, fn, slot, roi, max_corners, params, xy, prio, n, radius, base, stride, keep, out_xy, out_cap, cnt):
    fn.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                   C.c_void_p]
    fn.restype = C.c_int
    roi = None if roi is None else np.ascontiguousarray(roi, np.int32)
    d = lambda a: None if a is None else a.ctypes.data   # noqa: E731
    return fn(None if ctx is None else ctx.h, slot, d(roi), max_corners, None if params is None else C.cast(C.pointer(params), C.c_void_p), d(xy), d(prio), n, radius,
              d(base), stride, d(keep), d(out_xy), out_cap, d(cnt))
