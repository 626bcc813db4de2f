"""Shared by the tests of pmv_frames_clahe: the CPU twin (tests/twin/clahe_twin.cpp, compiled on first use), the table of cases and their
images.

Frames and caching come from gftt_common. The 160x120 and 203x87 images are the synthetic frames of the LK tests; the small sizes are crops
of the noise frame with a flat rectangle painted in, so that whole tiles hold one value and clipping occurs. Everything handed out is
computed once and shared; callers must not modify it."""
import ctypes as C
import os
import subprocess

import numpy as np

import gftt_common as gc

TW = gc.TW
_u8p, _i32p = C.POINTER(C.c_uint8), C.POINTER(C.c_int32)

# (w, h, clip_limit, (tiles_x, tiles_y)) and what the case reaches
CASES = [
    (160, 120, 2.0, (8, 8)),      # divisible, tile 20x15, cl 2
    (160, 120, 40.0, (8, 8)),     # cv's default
    (160, 120, 0.0, (8, 8)),      # no clipping
    (160, 120, 1000.0, (8, 8)),   # cl above every bin: nothing clipped
    (203, 87, 2.0, (8, 8)),       # extension (5, 1)
    (203, 87, 3.0, (4, 3)),       # extension (1, 3), non-square grid
    (41, 40, 2.0, (8, 8)),        # the width does not divide: the height gets a full extra row of tiles' worth (7, 8), cl = 1
    (40, 41, 2.0, (8, 8)),        # and the other way round: (8, 7)
    (64, 48, 4.0, (1, 1)),        # one tile: both interpolation clamps everywhere
    (75, 53, 0.5, (16, 16)),      # 5x4 tiles, cl = 1
]
CLIPPING = (0.5, 2.0, 3.0)        # cases with these clip limits must clip and redistribute a residual (asserted on the twin's statistics)


def case_id(case):
    w, h, clip, (tx, ty) = case
    return f"{w}x{h}-clip{clip:g}-{tx}x{ty}"


def _p(a, t):
    return a.ctypes.data_as(t)


class Twin:
    def __init__(self, lib):
        self.lib = lib
        lib.clahe_twin_apply.argtypes = [_u8p, C.c_int, C.c_int, C.c_double, C.c_int, C.c_int, _u8p, _i32p]

    def apply(self, img, clip_limit=40.0, tiles=(8, 8)):
        """(the equalised image, statistics: ext = columns and rows added, tile = tile size, cl, clipped = tiles with clipped > 0, residual =
        tiles with residual > 0, steps = the set of redistribution steps seen)"""
        img = np.ascontiguousarray(img, np.uint8)
        h, w = img.shape
        out = np.zeros_like(img)
        st = np.zeros(8 + 257, np.int32)
        assert self.lib.clahe_twin_apply(_p(img, _u8p), w, h, C.c_double(clip_limit), int(tiles[0]), int(tiles[1]), _p(out, _u8p), _p(st, _i32p)) == 0
        stats = dict(ext=(int(st[0]), int(st[1])), tile=(int(st[2]), int(st[3])), cl=int(st[4]), clipped=int(st[5]), residual=int(st[6]),
                     steps={int(s) for s in np.nonzero(st[8:])[0]})
        return out, stats


def twin():
    def make():
        so, src = os.path.join(TW, "libclahe_twin.so"), os.path.join(TW, "clahe_twin.cpp")
        if not os.path.exists(so) or os.path.getmtime(so) < os.path.getmtime(src):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", "-Wall", src, "-o", so])
        return Twin(C.CDLL(so))
    return gc.cached("clahe_twin", make)


def image(pmv, w, h):
    """the image of the cases of size w x h"""
    def make():
        if (w, h) in gc.SIZES:
            return gc.frame(pmv, w, h)
        img = gc.noise_frame()[11:11 + h, 7:7 + w].copy()
        img[h // 4:h // 4 + h // 2, w // 5:w // 5 + w // 2] = 93   # flat: whole tiles of one value
        return img
    return gc.cached(("clahe_image", w, h), make)


def equalised(pmv, case):
    """the twin's (image, statistics) for a case of the table, computed once"""
    w, h, clip, tiles = case
    return gc.cached(("clahe_equalised", w, h, clip, tiles), lambda: twin().apply(image(pmv, w, h), clip, tiles))
