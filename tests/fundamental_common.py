"""Shared by the tests of pmv_find_fundamental_mat: the CPU twin (tests/twin/fundamental_twin.cpp, compiled on first use) and the scenes.

Scenes come from test_twoview_host._scene (noise_px=0.3, integer=True) cast to float32, plus: "noise" (no geometry in either image: the call
runs into the 1000-iteration cap), "col40" (40 % of the image-1 points on one row: checkSubset refuses some subsets) and "colall" (every
image-1 point on one line: getSubset fails at iteration 0). Everything handed out is computed once and shared; callers must not modify it."""
import ctypes as C
import os
import subprocess

import numpy as np

from test_twoview_host import _scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TW = os.path.join(ROOT, "tests", "twin")
_u8p, _f32p, _i32p, _f64p = C.POINTER(C.c_uint8), C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_double)
_cache = {}
DEFAULT_R = 64   # FUND_DEFAULT_R of csrc/backend.h


def _p(a, t):
    return a.ctypes.data_as(t)


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


class Twin:
    def __init__(self, lib):
        self.lib = lib
        lib.fund_twin_find.argtypes = [_f32p, _f32p, C.c_int, C.c_double, C.c_double, _f64p, _u8p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        lib.fund_twin_iters_table.argtypes = [C.c_int, C.c_double, C.c_int, _f64p, _f64p]

    def subsets(self, p1, p2, count):
        """(the subsets drawn before getSubset failed (k, 7), how many subsets checkSubset refused on the way)"""
        out = np.zeros((count, 7), np.int32)
        refused = C.c_int()
        k = self.lib.fund_twin_subsets(_p(p1, _f32p), _p(p2, _f32p), len(p1), count, _p(out, _i32p), C.byref(refused))
        return out[:k], refused.value

    def seven_point(self, s1, s2):
        s1, s2 = np.ascontiguousarray(s1, np.float32), np.ascontiguousarray(s2, np.float32)
        F = np.zeros(27)
        n = self.lib.fund_twin_seven_point(_p(s1, _f32p), _p(s2, _f32p), _p(F, _f64p))
        return F[: 9 * n].reshape(n, 3, 3)

    def cubic(self, c):
        c = np.ascontiguousarray(c, np.float64)
        r = np.zeros(3)
        n = self.lib.fund_twin_cubic(_p(c, _f64p), _p(r, _f64p))
        return n, r

    def errors(self, F, p1, p2):
        F = np.ascontiguousarray(F, np.float64).reshape(9)
        err = np.zeros(len(p1), np.float32)
        self.lib.fund_twin_errors(_p(F, _f64p), _p(p1, _f32p), _p(p2, _f32p), len(p1), _p(err, _f32p))
        return err

    def iters_table(self, n, confidence, model_points=7):
        den, num = np.zeros(n + 1), np.zeros(1)
        self.lib.fund_twin_iters_table(n, confidence, model_points, _p(den, _f64p), _p(num, _f64p))
        return den, num[0]

    def update_iters(self, den, num, good, max_iters):
        tab = np.concatenate([[num], den])
        return self.lib.fund_twin_update_iters(_p(tab, _f64p), good, max_iters)

    def find(self, p1, p2, threshold=1.0, confidence=0.99):
        """(found, F (3, 3), mask, samples drawn, how often a model became the best)"""
        n = len(p1)
        F, mask = np.zeros(9), np.zeros(n, np.uint8)
        drawn, upd = C.c_int(), C.c_int()
        found = self.lib.fund_twin_find(_p(p1, _f32p), _p(p2, _f32p), n, threshold, confidence, _p(F, _f64p), _p(mask, _u8p), C.byref(drawn), C.byref(upd))
        return bool(found), F.reshape(3, 3), mask, drawn.value, upd.value


def twin():
    def make():
        so, src = os.path.join(TW, "libfundamental_twin.so"), os.path.join(TW, "fundamental_twin.cpp")
        if not os.path.exists(so) or os.path.getmtime(so) < os.path.getmtime(src):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", "-Wall", src, "-o", so])
        return Twin(C.CDLL(so))
    return cached("twin", make)


def points(kind, seed, n, f):
    """(p1, p2) as contiguous float32 (n, 2)"""
    def make():
        rng = np.random.default_rng(seed)
        if kind == "noise":   # no geometry at all: integer points uniform in 1200 x 370
            p1, p2 = np.floor(rng.uniform(0, [1200, 370], (n, 2))), np.floor(rng.uniform(0, [1200, 370], (n, 2)))
        else:
            S = _scene(seed, n, noise_px=0.3, outlier_frac=f, integer=True)
            p1, p2 = S["p1"].copy(), S["p2"].copy()
            if kind == "col40":    # 40 % of the image-1 points on one row
                p1[rng.random(n) < 0.4, 1] = 100.0
            elif kind == "colall":  # every image-1 point on one line
                p1[:, 1] = 100.0
            else:
                assert kind == "scene"
        return np.ascontiguousarray(p1, np.float32), np.ascontiguousarray(p2, np.float32)
    return cached(("points", kind, seed, n, f), make)


def scene(seed, n, f):
    """the _scene dict behind points("scene", seed, n, f)"""
    return cached(("scene", seed, n, f), lambda: _scene(seed, n, noise_px=0.3, outlier_frac=f, integer=True))


def found(key, threshold=1.0, confidence=0.99):
    """the twin's result of a scene key (kind, seed, n, f), computed once: (found, F, mask, drawn, updates)"""
    return cached(("find", key, threshold, confidence), lambda: twin().find(*points(*key), threshold, confidence))


# The cases of the GPU tests (tests/test_fundamental_gpu.py) as (scene key, threshold); what each is there for is asserted on the twin in
# tests/test_fundamental_twin.py. At 1 px the 0.3 px noise plus the rounding to integer pixels leave a minimal-sample model with ~80 % of the
# true inliers, so an outlier fraction of 0.5 runs into the 1000-iteration cap whatever n is: the "several hundred samples" and "first few
# rounds" cases are the same scenes at 3 px. ("scene", 7, 63, 0.3) draws exactly 64 samples and ("scene", 4, 64, 0.3) exactly 256: calls that
# end at a round's last sample for every R the kernel is measured with.
SCENES = ([("scene", 1, 15, 0.0)] + [("scene", s, n, f) for n in (63, 64, 65) for s in (1, 2, 3) for f in (0.0, 0.3, 0.5)] +
          [("scene", 1, 300, 0.5), ("noise", 5, 40, 0.0), ("noise", 5, 200, 0.0), ("col40", 1, 100, 0.0), ("colall", 1, 100, 0.0),
           ("scene", 7, 63, 0.3), ("scene", 4, 64, 0.3)])
CASES = [(k, 1.0) for k in SCENES] + [(("scene", 1, 300, 0.5), 3.0), (("scene", 1, 65, 0.3), 3.0)]


def case_id(c):
    return "%s-thr%g" % (scene_id(c[0]), c[1])


def scene_id(k):
    return "%s-seed%d-n%d-f%g" % k


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)
