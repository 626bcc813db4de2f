"""Shared by the tests of pmv_find_homography: the CPU twin (tests/twin/homography_twin.cpp, compiled on first use) and the scenes.

Every scene is float32 from a seeded generator here; all but "tiny" are rounded to integer pixels in a 1200 x 370 image:
  plane   points on a 3-D plane seen from two poses, Gaussian noise (0.3 px unless said otherwise), a fraction f of outliers
  rot     a pure rotation of general 3-D points
  noise   no geometry in either image: the call runs into max_iters
  col40   40 % of the image-1 points on one row: checkSubset refuses some subsets as collinear
  colall  every image-1 point on one line: getSubset fails at iteration 0
  twist   half of the image-2 points mirrored: the four-point orientation test refuses most subsets
  tiny    every image-2 point within 1e-7 of one point (one float32): runKernel's deviation sums are 0, no model
Everything handed out is computed once and shared; callers must not modify it."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TW = os.path.join(ROOT, "tests", "twin")
_u8p, _f32p, _i32p, _f64p = C.POINTER(C.c_uint8), C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_double)
_cache = {}
W_IMG, H_IMG = 1200, 370
KMAT = np.array([[370.0, 0, 600.0], [0, 370.0, 185.0], [0, 0, 1]])
DEFAULT_MAX_ITERS, DEFAULT_CONFIDENCE = 2000, 0.995   # cv::findHomography's defaults
ROUND = 64   # hypotheses per in-kernel round (HG_R of csrc/backend_homography.hip)


def _p(a, t):
    return a.ctypes.data_as(t)


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


class Twin:
    def __init__(self, lib):
        self.lib = lib
        lib.hg_twin_find.argtypes = [_f32p, _f32p, C.c_int, C.c_double, C.c_double, C.c_int, _f64p, _u8p, C.POINTER(C.c_int), C.POINTER(C.c_int), _f64p, _f64p]
        lib.hg_twin_iters_table.argtypes = [C.c_int, C.c_double, _f64p, _f64p]
        lib.hg_twin_hypot.argtypes = [C.c_double, C.c_double]
        lib.hg_twin_hypot.restype = C.c_double
        lib.hg_twin_lm.argtypes = [_f32p, _f32p, C.c_int, _u8p, _f64p, C.c_int, _f64p]

    def subsets(self, p1, p2, count):
        """(the subsets drawn before getSubset failed (k, 4), subsets refused as collinear, subsets refused by the orientation test)"""
        out = np.zeros((count, 4), np.int32)
        refused = np.zeros(2, np.int32)
        k = self.lib.hg_twin_subsets(_p(p1, _f32p), _p(p2, _f32p), len(p1), count, _p(out, _i32p), _p(refused, _i32p))
        return out[:k], int(refused[0]), int(refused[1])

    def check_subset(self, s1, s2):
        """0 accepted, 1 collinear, 2 orientation"""
        s1, s2 = np.ascontiguousarray(s1, np.float32), np.ascontiguousarray(s2, np.float32)
        return self.lib.hg_twin_check_subset(_p(s1, _f32p), _p(s2, _f32p))

    def four_point(self, s1, s2):
        """H (3, 3) of the four correspondences, or None"""
        s1, s2 = np.ascontiguousarray(s1, np.float32), np.ascontiguousarray(s2, np.float32)
        H = np.zeros(9)
        return H.reshape(3, 3) if self.lib.hg_twin_four_point(_p(s1, _f32p), _p(s2, _f32p), _p(H, _f64p)) else None

    def errors(self, H, p1, p2):
        H = np.ascontiguousarray(H, np.float64).reshape(9)
        err = np.zeros(len(p1), np.float32)
        self.lib.hg_twin_errors(_p(H, _f64p), _p(p1, _f32p), _p(p2, _f32p), len(p1), _p(err, _f32p))
        return err

    def iters_table(self, n, confidence):
        den, num = np.zeros(n + 1), np.zeros(1)
        self.lib.hg_twin_iters_table(n, confidence, _p(den, _f64p), _p(num, _f64p))
        return den, num[0]

    def update_iters(self, den, num, good, max_iters):
        tab = np.concatenate([[num], den])
        return self.lib.hg_twin_update_iters(_p(tab, _f64p), good, max_iters)

    def jacobi(self, A):
        """(eigenvalues descending, eigenvectors as rows)"""
        A = np.ascontiguousarray(A, np.float64)
        n = len(A)
        w, V = np.zeros(n), np.zeros((n, n))
        self.lib.hg_twin_jacobi(_p(A, _f64p), n, _p(w, _f64p), _p(V, _f64p))
        return w, V

    def hypot(self, a, b):
        return self.lib.hg_twin_hypot(a, b)

    def refit_dlt(self, p1, p2, mask):
        mask = np.ascontiguousarray(mask, np.uint8)
        H = np.zeros(9)
        return H.reshape(3, 3) if self.lib.hg_twin_refit_dlt(_p(p1, _f32p), _p(p2, _f32p), len(p1), _p(mask, _u8p), _p(H, _f64p)) else None

    def lm(self, p1, p2, mask, H, max_iter=10):
        """(H after up to max_iter LM iterations, iterations made, |r|^2 before, after)"""
        mask = np.ascontiguousarray(mask, np.uint8)
        H = np.array(H, np.float64).reshape(9)
        S2 = np.zeros(2)
        it = self.lib.hg_twin_lm(_p(p1, _f32p), _p(p2, _f32p), len(p1), _p(mask, _u8p), _p(H, _f64p), max_iter, _p(S2, _f64p))
        return H.reshape(3, 3), it, S2[0], S2[1]

    def find(self, p1, p2, threshold=3.0, confidence=DEFAULT_CONFIDENCE, max_iters=DEFAULT_MAX_ITERS):
        """dict: found, H (3, 3), mask, drawn, updates (how often a model became the best), H_ransac (the model in front of the refit),
        S2 (the LM stage's |r|^2 before and after; NaN without a refit)"""
        n = len(p1)
        H, Hr, mask, S2 = np.zeros(9), np.zeros(9), np.zeros(n, np.uint8), np.full(2, np.nan)
        drawn, upd = C.c_int(), C.c_int()
        found = self.lib.hg_twin_find(_p(p1, _f32p), _p(p2, _f32p), n, threshold, confidence, max_iters, _p(H, _f64p), _p(mask, _u8p), C.byref(drawn),
                                      C.byref(upd), _p(Hr, _f64p), _p(S2, _f64p))
        return dict(found=bool(found), H=H.reshape(3, 3), mask=mask, drawn=drawn.value, updates=upd.value, H_ransac=Hr.reshape(3, 3), S2=S2)


def twin():
    def make():
        so, src = os.path.join(TW, "libhomography_twin.so"), os.path.join(TW, "homography_twin.cpp")
        if not os.path.exists(so) or os.path.getmtime(so) < os.path.getmtime(src):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", "-Wall", src, "-o", so])
        return Twin(C.CDLL(so))
    return cached("twin", make)


def _rodrigues(r):
    th = np.linalg.norm(r)
    k = r / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx


def _proj(H, p):
    q = np.c_[p, np.ones(len(p))] @ H.T
    return q[:, :2] / q[:, 2:]


def geometry(kind, seed):
    """the true H (3, 3, H[2, 2] = 1) of a "plane" or "rot" scene: K (R + t n^T / d) K^-1 for the plane n . X = d, K R K^-1 for the rotation"""
    rng = np.random.default_rng(1000 + seed)
    R = _rodrigues(rng.uniform(-0.06, 0.06, 3) + np.array([0, 0.04, 0]))
    if kind == "rot":
        H = KMAT @ R @ np.linalg.inv(KMAT)
    else:
        nrm = np.array([0.15, -0.2, -1.0]) + rng.uniform(-0.1, 0.1, 3)
        nrm /= np.linalg.norm(nrm)
        d = -rng.uniform(8, 12)   # the plane in front of camera 1: n . X = d with n_z < 0
        t = rng.uniform(-0.5, 0.5, 3)
        H = KMAT @ (R + np.outer(t, nrm) / d) @ np.linalg.inv(KMAT)
    return H / H[2, 2]


def points(kind, seed, n, f, noise_px=0.3):
    """(p1, p2) as contiguous float32 (n, 2)"""
    def make():
        rng = np.random.default_rng(seed)
        p1 = rng.uniform([20, 20], [W_IMG - 20, H_IMG - 20], (n, 2))
        if kind == "noise":
            p2 = rng.uniform(0, [W_IMG, H_IMG], (n, 2))
        elif kind == "tiny":
            p2 = 100.0 + 1e-7 * rng.uniform(-1, 1, (n, 2))
            return np.ascontiguousarray(np.floor(p1), np.float32), np.ascontiguousarray(p2, np.float32)
        else:
            p2 = _proj(geometry("rot" if kind == "rot" else "plane", seed), p1) + noise_px * rng.standard_normal((n, 2))
            p1 = p1 + noise_px * rng.standard_normal((n, 2))
            out = rng.random(n) < f
            p2[out] = rng.uniform(0, [W_IMG, H_IMG], (int(out.sum()), 2))
            if kind == "col40":
                p1[rng.random(n) < 0.4, 1] = 100.0
            elif kind == "colall":
                p1[:, 1] = 100.0
            elif kind == "twist":
                p2[::2, 0] = W_IMG - p2[::2, 0]
            else:
                assert kind in ("plane", "rot"), kind
        return np.ascontiguousarray(np.round(p1), np.float32), np.ascontiguousarray(np.round(p2), np.float32)
    return cached(("points", kind, seed, n, f, noise_px), make)


def found(key, threshold=3.0, confidence=DEFAULT_CONFIDENCE, max_iters=DEFAULT_MAX_ITERS):
    """the twin's result of a scene key (kind, seed, n, f), computed once"""
    return cached(("find", key, threshold, confidence, max_iters), lambda: twin().find(*points(*key), threshold, confidence, max_iters))


# The cases of the GPU tests (tests/test_homography_gpu.py) as (scene key, threshold); what each is there for is asserted on the twin in
# tests/test_homography_twin.py. n = 63, 64, 65 sit around the width of the lane-strided sums and of a round; n = 4 is cv's branch without RANSAC.
SCENES = ([("plane", 1, 4, 0.0), ("tiny", 1, 4, 0.0), ("tiny", 1, 5, 0.0)] +
          [("plane", s, n, f) for n, s in ((5, 1), (63, 1), (64, 2), (65, 3)) for f in (0.0, 0.3, 0.6)] +
          [("plane", 1, 300, 0.6), ("rot", 1, 64, 0.0), ("rot", 2, 65, 0.3), ("noise", 5, 40, 0.0), ("noise", 5, 300, 0.0), ("col40", 1, 100, 0.0),
           ("colall", 1, 100, 0.0), ("twist", 1, 64, 0.0)])
CASES = [(k, t) for k in SCENES for t in (1.0, 3.0)]


def case_id(c):
    return "%s-thr%g" % (scene_id(c[0]), c[1])


def scene_id(k):
    return "%s-seed%d-n%d-f%g" % k


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)
