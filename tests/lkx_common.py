"""Shared by the tests of pmv_lk_track_ex / pmv_lk_track_fb: the CPU twin (tests/twin/lkx_twin.cpp, compiled on first use) and the two scenes.

Pair A: the frame pair and the 320 points of tests/test_lk_params_gpu.py::_pair. Crop: two windows of one larger synthetic frame, a true
flow of (34, -22) - more than the pyramid covers at the default window - with guesses within +-2 px of the truth."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TW = os.path.join(ROOT, "tests", "twin")
SIZES = [(160, 120), (203, 87)]
FLOW = np.array([34.0, -22.0])
INIT, EIG = 4, 8
_u8p, _f32p = C.POINTER(C.c_uint8), C.POINTER(C.c_float)
_cache = {}


def _p(a, t):
    return a.ctypes.data_as(t)


class Twin:
    def __init__(self, lib):
        self.lib = lib

    def _call(self, fb, prev, nxt, pts, init, flags, win, max_level, max_iter, eps, min_eig):
        prev, nxt = np.ascontiguousarray(prev, np.uint8), np.ascontiguousarray(nxt, np.uint8)
        p = np.ascontiguousarray(pts, np.float32).reshape(-1, 2)
        n, (h, w) = len(p), prev.shape
        xy = np.zeros((n, 2), np.float32) if init is None else np.array(init, np.float32).reshape(-1, 2)
        flags |= 0 if init is None else INIT
        st, err = np.zeros(n, np.uint8), np.zeros(n, np.float32)
        args = [_p(prev, _u8p), _p(nxt, _u8p), w, h, _p(p, _f32p), n, win, max_level, max_iter, C.c_double(eps), C.c_float(min_eig), flags, _p(xy, _f32p), _p(st, _u8p), _p(err, _f32p)]
        if not fb:
            assert self.lib.lkx_track(*args) >= 0
            return xy, st, err
        bxy, bst, berr = np.zeros((n, 2), np.float32), np.zeros(n, np.uint8), np.zeros(n, np.float32)
        assert self.lib.lkx_track_fb(*args, _p(bxy, _f32p), _p(bst, _u8p), _p(berr, _f32p)) >= 0
        return xy, st, err, bxy, bst, berr

    def track(self, prev, nxt, pts, init=None, flags=0, win=32, max_level=4, max_iter=30, eps=0.01, min_eig=1e-4):
        return self._call(False, prev, nxt, pts, init, flags, win, max_level, max_iter, eps, min_eig)

    def track_fb(self, prev, nxt, pts, init=None, flags=0, win=32, max_level=4, max_iter=30, eps=0.01, min_eig=1e-4):
        return self._call(True, prev, nxt, pts, init, flags, win, max_level, max_iter, eps, min_eig)


def twin():
    if "twin" not in _cache:
        so, src = os.path.join(TW, "liblkx_twin.so"), os.path.join(TW, "lkx_twin.cpp")
        if not os.path.exists(so) or os.path.getmtime(so) < os.path.getmtime(src):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", "-Wall", src, "-o", so])
        _cache["twin"] = Twin(C.CDLL(so))
    return _cache["twin"]


def twin_cached(key, fn):
    """a twin result computed once and shared; callers must not modify it"""
    if key not in _cache:
        _cache[key] = fn()
    return _cache[key]


def pair_a(pmv, w, h):
    if ("A", w, h) not in _cache:
        fr, _ = pmv.synth_sequence(1007, 10, 2, w, h, 0.58 * w, 0.58 * w, w / 2, h / 2)
        rng = np.random.default_rng(5)
        wide = np.stack([rng.uniform(-70, w + 70, 160), rng.uniform(-70, h + 70, 160)], axis=1)
        inside = np.stack([rng.uniform(8, w - 8, 160), rng.uniform(8, h - 8, 160)], axis=1)
        _cache["A", w, h] = (fr[0], fr[1], np.concatenate([wide, inside]).astype(np.float32))
    return _cache["A", w, h]


def crop(pmv, w, h):
    """(prev, next, points, init): next shows the content of prev displaced by FLOW"""
    if ("crop", w, h) not in _cache:
        big = pmv.synth_sequence(1007, 10, 1, 320, 200, 185.6, 185.6, 160, 100)[0][0]
        prev = np.ascontiguousarray(big[40:40 + h, 60:60 + w])
        nxt = np.ascontiguousarray(big[62:62 + h, 26:26 + w])
        rng = np.random.default_rng(7)
        pts = np.stack([rng.uniform(8, w - 8, 320), rng.uniform(8, h - 8, 320)], axis=1)
        init = (pts + FLOW + rng.uniform(-2, 2, (320, 2))).astype(np.float32)
        _cache["crop", w, h] = (prev, nxt, pts.astype(np.float32), init)
    return _cache["crop", w, h]


def wild_init(w, h, init):
    """the guesses of 40 points replaced by positions anywhere within 70 px of the frame, outside it included"""
    rng = np.random.default_rng(11)
    out = init.copy()
    idx = rng.choice(len(init), 40, replace=False)
    out[idx] = np.stack([rng.uniform(-70, w + 70, 40), rng.uniform(-70, h + 70, 40)], axis=1).astype(np.float32)
    return out, idx


def near_truth(pts, xy, st, tol=0.5):
    """how many tracked points lie within tol of points + FLOW"""
    d = np.linalg.norm(xy.astype(np.float64) - (pts.astype(np.float64) + FLOW), axis=1)
    return int(((d < tol) & (st > 0)).sum())


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a
