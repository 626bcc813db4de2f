"""Shared by the tests of pmv_triangulate_tracks: the CPU twin (tests/twin/tri_tracks_twin.cpp, compiled on first use) and the scenes.

A scene is a seeded corridor: cameras 0.8 apart along z with small rotations and lateral offsets (camera 0 is exactly [I|0] when
first_identity is set), points at depth 3..40 in front of the last camera, normalised or pixel observations (K = 718, 718, 607, 185) with
Gaussian noise given in pixels, and per landmark a random subset of the cameras (0..nc views unless min_v says otherwise). The observation
arrays are shuffled as a whole, so pt_idx is not sorted. The gate scene is hand-made (see gate_scene). Everything handed out is computed
once and shared; callers must not modify it."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TW = os.path.join(ROOT, "tests", "twin")
_u8p, _i32p, _f64p = C.POINTER(C.c_uint8), C.POINTER(C.c_int32), C.POINTER(C.c_double)
_cache = {}
KMAT = np.array([[718.0, 0, 607.0], [0, 718.0, 185.0], [0, 0, 1]])
FEW_VIEWS, DEGENERATE, DEPTH, REPROJ, PARALLAX = 1, 2, 4, 8, 16
INF = float("inf")
DEFAULTS = dict(min_views=2, refine_iters=0, min_depth=0.1, max_depth=INF, max_reproj=INF, min_parallax_deg=0.0)   # the call's (a null pointer)
NO_GATES = dict(min_views=2, refine_iters=0, min_depth=-1e300, max_depth=INF, max_reproj=INF, min_parallax_deg=0.0)


def _p(a, t):
    return a.ctypes.data_as(t)


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def params(**kw):
    p = dict(DEFAULTS)
    p.update(kw)
    return p


def gates_on(pixel, **kw):
    """every gate on, in the observations' unit"""
    return params(min_depth=0.5, max_depth=30.0, max_reproj=1.5 if pixel else 1.5 / 718.0, min_parallax_deg=0.5, **kw)


class Twin:
    def __init__(self, lib):
        self.lib = lib
        lib.tt_twin_run.argtypes = [_f64p, C.c_int, _f64p, _i32p, _i32p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, C.c_double,
                                    _f64p, _u8p, _f64p, C.POINTER(C.c_int), _f64p, _f64p, _i32p]
        lib.tt_twin_centres.argtypes = [_f64p, C.c_int, _f64p]

    def centres(self, P):
        P = np.ascontiguousarray(P, np.float64).reshape(-1, 12)
        Cn = np.zeros((len(P), 3))
        return self.lib.tt_twin_centres(_p(P, _f64p), len(P), _p(Cn, _f64p)), Cn

    def run(self, P, obs, cam, pt, n_pts, p):
        """dict: rc (0, or -(1 + c) for the singular camera c of the parallax gate), xyz, status, err, good, Qh (the DLT's homogeneous
        vectors), costs (n_pts, refine_iters + 1: at the DLT's X and after every accepted step, NaN behind), steps (accepted steps)"""
        P = np.ascontiguousarray(P, np.float64).reshape(-1, 12)
        obs = np.ascontiguousarray(obs, np.float64).reshape(-1, 2)
        cam, pt = np.ascontiguousarray(cam, np.int32), np.ascontiguousarray(pt, np.int32)
        n = max(n_pts, 1)
        xyz, status, err, Qh = np.zeros((n, 3)), np.zeros(n, np.uint8), np.zeros(n), np.zeros((n, 4))
        costs, steps = np.zeros((n, p["refine_iters"] + 1)), np.zeros(n, np.int32)
        good = C.c_int()
        rc = self.lib.tt_twin_run(_p(P, _f64p), len(P), _p(obs, _f64p), _p(cam, _i32p), _p(pt, _i32p), len(obs), n_pts, p["min_views"], p["refine_iters"],
                                  p["min_depth"], p["max_depth"], p["max_reproj"], p["min_parallax_deg"], _p(xyz, _f64p), _p(status, _u8p), _p(err, _f64p),
                                  C.byref(good), _p(Qh, _f64p), _p(costs, _f64p), _p(steps, _i32p))
        return dict(rc=rc, xyz=xyz[:n_pts], status=status[:n_pts], err=err[:n_pts], good=good.value, Qh=Qh[:n_pts], costs=costs[:n_pts], steps=steps[:n_pts])


def twin():
    def make():
        so, src = os.path.join(TW, "libtri_tracks_twin.so"), os.path.join(TW, "tri_tracks_twin.cpp")
        if not os.path.exists(so) or os.path.getmtime(so) < os.path.getmtime(src):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", "-Wall", src, "-o", so])
        return Twin(C.CDLL(so))
    return cached("twin", make)


def _rodrigues(r):
    th = np.linalg.norm(r)
    if th == 0:
        return np.eye(3)
    k = r / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx


def project(P, X):
    """(u, v) of the points X (n, 3) through the matrices P (n, 3, 4), one each; depth = the third row"""
    q = np.einsum("nij,nj->ni", P, np.c_[X, np.ones(len(X))])
    return q[:, :2] / q[:, 2:], q[:, 2]


def scene(nc, n_pts, seed, noise_px=0.0, pixel=False, first_identity=False, min_v=0):
    """dict: P (nc, 3, 4), obs (n_obs, 2), cam, pt (n_obs,), n_pts, X (the true points), views (per landmark)"""
    def make():
        rng = np.random.default_rng(seed)
        P, Rs, cs = np.zeros((nc, 3, 4)), [], []
        for i in range(nc):
            ident = first_identity and i == 0
            R = np.eye(3) if ident else _rodrigues(rng.uniform(-0.03, 0.03, 3))
            c = np.zeros(3) if ident else np.array([rng.uniform(-0.3, 0.3), rng.uniform(-0.15, 0.15), 0.8 * i + rng.uniform(-0.05, 0.05)])
            Rt = np.c_[R, -R @ c]
            P[i] = KMAT @ Rt if pixel else Rt
            Rs.append(R)
            cs.append(c)
        z = rng.uniform(3, 40, n_pts)
        X = cs[-1] + (np.c_[rng.uniform(-0.45, 0.45, n_pts) * z, rng.uniform(-0.2, 0.2, n_pts) * z, z]) @ Rs[-1]   # rows: R^T (x, y, z)
        cam, pt, views = [], [], np.zeros(n_pts, np.int32)
        for j in range(n_pts):
            k = int(rng.integers(min_v, nc + 1))
            views[j] = k
            cam += list(rng.permutation(nc)[:k])
            pt += [j] * k
        cam, pt = np.array(cam, np.int32), np.array(pt, np.int32)
        if len(cam):
            uv, _ = project(P[cam], X[pt])
            uv = uv + (noise_px if pixel else noise_px / 718.0) * rng.standard_normal(uv.shape)
            perm = rng.permutation(len(cam))
            cam, pt, uv = cam[perm], pt[perm], uv[perm]
        else:
            uv = np.zeros((0, 2))
        return dict(P=P, obs=np.ascontiguousarray(uv), cam=np.ascontiguousarray(cam), pt=np.ascontiguousarray(pt), n_pts=n_pts, X=X, views=views, pixel=pixel)
    return cached(("scene", nc, n_pts, seed, noise_px, pixel, first_identity, min_v), make)


GATE_PARAMS = params(min_depth=0.1, max_depth=100.0, max_reproj=2.0 / 718.0, min_parallax_deg=1.0)
GATE_NAMES = ["good", "behind", "outlier", "baseline", "no-obs", "one-obs", "at-centre", "behind+outlier", "twice-degenerate"]


def gate_scene():
    """Normalised observations; cameras 0..3 at (0, 0, 0.8 i) looking along z (camera 0 is [I|0]), camera 4 at (0.01, 0, 0). Landmarks:
      0 good              seen by cameras 0..3, exact observations
      1 behind            in front of cameras 0 and 1, behind camera 3
      2 outlier           seen by cameras 0..3, the observation of camera 2 off by 50 px
      3 baseline          seen by cameras 0 and 4 only: 0.01 apart
      4 no-obs, 5 one-obs
      6 at-centre         the centre of camera 1, seen by cameras 0, 1, 2
      7 behind+outlier    landmark 1's geometry with the observation of camera 1 off by 50 px
      8 twice-degenerate  camera 0 listed twice with the observation (0, 0): AtA = diag(2, 2, 0, 0), the first null vector is a direction"""
    def make():
        cs = [np.array([0.0, 0.0, 0.8 * i]) for i in range(4)] + [np.array([0.01, 0.0, 0.0])]
        P = np.array([np.c_[np.eye(3), -c] for c in cs])
        X = np.array([[2.0, 1.0, 5.0], [0.3, 0.2, 1.5], [-1.5, 0.8, 6.0], [0.5, -0.3, 10.0], [1.0, 1.0, 8.0], [1.0, -1.0, 8.0], cs[1], [0.3, 0.2, 1.5], [0.0, 0.0, 1.0]])
        lists = {0: [0, 1, 2, 3], 1: [0, 1, 3], 2: [0, 1, 2, 3], 3: [0, 4], 4: [], 5: [2], 6: [0, 1, 2], 7: [0, 1, 3], 8: [0, 0]}
        cam, pt, uv = [], [], []
        for j, cl in lists.items():
            for c in cl:
                q = P[c] @ np.r_[X[j], 1.0]
                o = q[:2] / q[2] if q[2] != 0 else np.array([0.1, 0.1])
                if (j, c) in ((2, 2), (7, 1)):
                    o = o + np.array([50.0 / 718.0, 0.0])
                if j == 8:
                    o = np.zeros(2)
                cam.append(c), pt.append(j), uv.append(o)
        return dict(P=P, obs=np.ascontiguousarray(np.array(uv)), cam=np.array(cam, np.int32), pt=np.array(pt, np.int32), n_pts=len(X), X=X, pixel=False)
    return cached("gate_scene", make)


def run(sc, p):
    """the twin's result of a scene with the parameters p, computed once (keyed by the scene object and the parameters)"""
    return cached(("run", id(sc), tuple(sorted(p.items()))), lambda: twin().run(sc["P"], sc["obs"], sc["cam"], sc["pt"], sc["n_pts"], p))


def order_preserving_shuffle(sc, seed):
    """the observation arrays permuted so that every landmark's observations keep their relative order"""
    rng = np.random.default_rng(seed)
    n = len(sc["pt"])
    slots = rng.permutation(n)                      # slot i of the new arrays belongs to landmark pt[slots[i]] ...
    new_pt = sc["pt"][slots]
    src = np.zeros(n, np.int64)
    for j in np.unique(new_pt):                      # ... and takes that landmark's observations in their old order
        src[np.flatnonzero(new_pt == j)] = np.flatnonzero(sc["pt"] == j)
    return dict(sc, obs=np.ascontiguousarray(sc["obs"][src]), cam=np.ascontiguousarray(sc["cam"][src]), pt=np.ascontiguousarray(sc["pt"][src]))


def svd_points(sc):
    """per landmark with >= 2 observations: X from the smallest right singular vector of its 2m x 4 system (numpy, float64); NaN rows elsewhere"""
    def make():
        out = np.full((sc["n_pts"], 3), np.nan)
        for j in range(sc["n_pts"]):
            idx = np.flatnonzero(sc["pt"] == j)
            if len(idx) < 2:
                continue
            rows = []
            for i in idx:
                Pc, (x, y) = sc["P"][sc["cam"][i]], sc["obs"][i]
                rows += [x * Pc[2] - Pc[0], y * Pc[2] - Pc[1]]
            v = np.linalg.svd(np.array(rows))[2][-1]
            out[j] = v[:3] / v[3]
        return out
    return cached(("svd", id(sc)), make)


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)
