"""Shared by the tests of pmv_detect_gftt_ex: the CPU twin (tests/twin/gftt_twin.cpp, compiled on first use) and the scenes.

Frames: the synthetic 160x120 and 203x87 frames of the LK tests, a gradient-only image (no corner anywhere) and a 320x256 noise frame.
Masks: 255 = allowed. Everything handed out is computed once and shared; callers must not modify it."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TW = os.path.join(ROOT, "tests", "twin")
SIZES = [(160, 120), (203, 87)]
GP_REG = 4096          # records k_gftt_pick keeps in registers (frontend.hip); a cell with more takes its list in HBM
UNLIMITED_CAP = 4096   # PMV_GFTT_UNLIMITED_CAP
_u8p, _f32p, _i32p, _f64p = C.POINTER(C.c_uint8), C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_double)
_cache = {}


def _p(a, t):
    return a.ctypes.data_as(t)


class Twin:
    def __init__(self, lib):
        self.lib = lib

    def response(self, img, cell, block_size=3, use_harris=False, k=0.04):
        img = np.ascontiguousarray(img, np.uint8)
        h, w = img.shape
        x0, y0, cw, ch = [int(v) for v in cell]
        out = np.zeros((ch, cw), np.float32)
        assert self.lib.gftt_twin_response(_p(img, _u8p), w, h, x0, y0, cw, ch, int(block_size), int(bool(use_harris)), C.c_double(k), _p(out, _f32p)) == 0
        return out

    def cell(self, img, cell, max_corners, quality=0.01, min_dist=5.0, mask=None, block_size=3, use_harris=False, k=0.04):
        """(corners (n, 2) int32, response map, masked maximum, records above the threshold); mask: None or an (h, w) uint8 view of any row stride"""
        img = np.ascontiguousarray(img, np.uint8)
        h, w = img.shape
        x0, y0, cw, ch = [int(v) for v in cell]
        cap = cw * ch
        xy = np.zeros((cap, 2), np.int32)
        resp = np.zeros((ch, cw), np.float32)
        info = np.zeros(2, np.float64)
        mptr, mstride = None, 0
        if mask is not None:
            assert mask.dtype == np.uint8 and mask.shape == (h, w) and mask.strides[1] == 1
            mptr, mstride = C.cast(mask.ctypes.data, _u8p), mask.strides[0]
        n = self.lib.gftt_twin_cell(_p(img, _u8p), w, h, x0, y0, cw, ch, int(max_corners), C.c_double(quality), C.c_double(min_dist), int(block_size),
                                    int(bool(use_harris)), C.c_double(k), mptr, mstride, _p(xy, _i32p), cap, _p(resp, _f32p), _p(info, _f64p))
        assert n != -2, "a selected value is not above 0: the invariant k_gftt_pick relies on"
        assert 0 <= n <= cap
        return xy[:n].copy(), resp, float(info[0]), int(info[1])

    def corners(self, *a, **kw):
        return self.cell(*a, **kw)[0]


def twin():
    if "twin" not in _cache:
        so, src = os.path.join(TW, "libgftt_twin.so"), os.path.join(TW, "gftt_twin.cpp")
        if not os.path.exists(so) or os.path.getmtime(so) < os.path.getmtime(src):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", "-Wall", src, "-o", so])
        _cache["twin"] = Twin(C.CDLL(so))
    return _cache["twin"]


def cached(key, fn):
    """a result computed once and shared; callers must not modify it"""
    if key not in _cache:
        _cache[key] = fn()
    return _cache[key]


def frame(pmv, w, h):
    return cached(("frame", w, h), lambda: pmv.synth_sequence(1007, 10, 1, w, h, 0.58 * w, 0.58 * w, w / 2, h / 2)[0][0])


def gradient_frame(w=96, h=80):
    """a horizontal ramp: one-dimensional structure, det(M) = 0 everywhere, so the Harris response is nowhere positive"""
    return cached(("ramp", w, h), lambda: np.ascontiguousarray(np.broadcast_to((np.arange(w) * 2 % 256).astype(np.uint8), (h, w))))


def noise_frame(w=320, h=256):
    return cached(("noise", w, h), lambda: np.random.default_rng(3).integers(0, 256, (h, w), dtype=np.uint8))


def corner_cells(w, h, cw=31, ch=29):
    """a cell at each corner of a w x h frame"""
    return np.asarray([(0, 0, cw, ch), (w - cw, 0, cw, ch), (0, h - ch, cw, ch), (w - cw, h - ch, cw, ch)], np.int32)


def sweep_cells(pmv, w, h):
    """the grid; 40x33, narrower than a tile; 97x70 = 4x3 tiles with ragged edges; the four frame corners; 5x4 and 3x3"""
    extra = [(50, 20, 40, 33), (60, 10, 97, 70), (100, 40, 5, 4), (7, 9, 3, 3)]
    return np.concatenate([pmv.grid_cells(w, h), np.asarray(extra, np.int32), corner_cells(w, h)]).astype(np.int32)


def disc_mask(w, h, points, radius):
    """255 everywhere but inside the discs of `radius` around `points` (x, y): what a KLT loop hands the detector on a refill"""
    yy, xx = np.mgrid[0:h, 0:w]
    m = np.full((h, w), 255, np.uint8)
    for x, y in np.asarray(points).reshape(-1, 2):
        m[(xx - x) ** 2 + (yy - y) ** 2 <= radius * radius] = 0
    return m


def track_points(w, h, n, seed=17):
    rng = np.random.default_rng(seed)
    return np.stack([rng.integers(0, w, n), rng.integers(0, h, n)], axis=1)


def checker_mask(w, h):
    yy, xx = np.mgrid[0:h, 0:w]
    return (((xx + yy) & 1) * 255).astype(np.uint8)


def roi_mask(mask, pad=(5, 9)):
    """the same mask as a view into a larger array: mask_stride > w"""
    h, w = mask.shape
    big = np.full((h + 2 * pad[0], w + 2 * pad[1] + 7), 77, np.uint8)
    view = big[pad[0]:pad[0] + h, pad[1]:pad[1] + w]
    view[:] = mask
    assert view.strides[0] > w
    return view


def masks(w, h):
    """name -> (h, w) uint8 mask of the GPU mask cases"""
    def make():
        discs = disc_mask(w, h, track_points(w, h, 60), 7)
        return {"discs": discs, "checker": checker_mask(w, h), "zero": np.zeros((h, w), np.uint8), "roi": roi_mask(discs)}
    return cached(("masks", w, h), make)


def blanked_strongest(pmv, w, h, cell, radius=9, **kw):
    """(mask that blanks a disc around the unmasked run's strongest corner, the unmasked list, the masked list), by the twin"""
    def make():
        img = frame(pmv, w, h)
        plain = twin().corners(img, cell, 0, **kw)
        m = disc_mask(w, h, [plain[0] + np.asarray(cell[:2])], radius)
        return m, plain, twin().corners(img, cell, 0, mask=m, **kw)
    return cached(("blanked", w, h, tuple(int(v) for v in cell), radius, tuple(sorted(kw.items()))), make)
