"""Shared by the tests of pmv_project_points and pmv_lk_track_fb_levels: the CPU twin of the projection (tests/twin/project_twin.cpp, built on
the fly), the points the projection tests use, and the composition that defines a level-capped forward-backward call over the existing LK
twin (tests/lkx_common.py): cv's maxLevel = min(top, the context's max_level) per pass."""
import ctypes as C
import os
import subprocess

import numpy as np

import gftt_common as gc
import lift_common as lf
import lkx_common as lx

TW = os.path.join(os.path.dirname(os.path.abspath(__file__)), "twin")
_f32p, _f64p, _u8p = C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_uint8)


class ProjectTwin:
    def __init__(self, lib):
        self.lib = lib
        lib.project_twin_points.argtypes = [_f64p, _f64p, C.c_int, _f32p, _u8p]

    def points(self, cam, xyz):
        """(xy (n, 2) float32, ok (n,) uint8)"""
        xyz = np.ascontiguousarray(xyz, np.float64).reshape(-1, 3)
        n = len(xyz)
        out, ok = np.zeros((n, 2), np.float32), np.zeros(n, np.uint8)
        c13 = lf.cam13(cam)
        assert self.lib.project_twin_points(c13.ctypes.data_as(_f64p), xyz.ctypes.data_as(_f64p), n, out.ctypes.data_as(_f32p), ok.ctypes.data_as(_u8p)) == 0
        return out, ok


def project_twin():
    def make():
        so, src = os.path.join(TW, "libproject_twin.so"), os.path.join(TW, "project_twin.cpp")
        if not os.path.exists(so) or os.path.getmtime(so) < os.path.getmtime(src):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", "-Wall", src, "-o", so])
        return ProjectTwin(C.CDLL(so))
    return gc.cached("project_twin", make)


def camera_points(n, seed=11, spread=0.9):
    """n points in front of the camera: normalised coordinates within +-spread (beyond the frame's edge too), depths 0.5 .. 40"""
    rng = np.random.default_rng(seed)
    z = rng.uniform(0.5, 40.0, n)
    x, y = rng.uniform(-spread, spread, n), rng.uniform(-spread, spread, n)
    return np.stack([x * z, y * z, z], axis=1)


# one of each reason to refuse a point, and their good neighbours: (xyz, ok)
REFUSED = [((0.1, 0.2, 0.0), 0), ((0.1, 0.2, -1.0), 0), ((0.1, 0.2, -0.0), 0), ((np.nan, 0.2, 1.0), 0), ((0.1, np.nan, 1.0), 0), ((0.1, 0.2, np.nan), 0),
           ((np.inf, 0.2, 1.0), 0), ((0.1, -np.inf, 1.0), 0), ((0.1, 0.2, np.inf), 0), ((0.1, 0.2, 1.0), 1), ((1e300, 0.0, 1e-300), 0),
           ((5e3, 0.0, 1.0), 0), ((0.0, -5e3, 1.0), 0), ((0.0, 0.0, 1e-300), 1), ((-0.3, 0.25, 7.0), 1)]


# the pole of the forward model: with k4 = -1 the denominator 1 + k4 r2 is exactly 0 at r2 = 1 (kr = 1 / 0), with k1 = -1 as well kr = 0 / 0
POLE = dict(fx=512.0, fy=512.0, cx=300.0, cy=200.0, dist=(0, 0, 0, 0, 0, -1.0), iters=5)
POLE_NAN = dict(POLE, dist=(-1.0, 0, 0, 0, 0, -1.0))
POLE_POINTS = [(2.0, 0.0, 2.0), (0.0, -3.0, 3.0), (0.6, 0.8, 1.0)]   # r2 = 1 exactly (0.36 + 0.64 rounds to 1.0 in double)


def ulp_distance(a, b):
    """float32 arrays of finite values: the distance in units of the last place, through the ordered-integer view"""
    def key(v):
        i = np.ascontiguousarray(v, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(a) - key(b))


def twin_fb_levels(prev, nxt, pts, init, flags, fwd_top, back_top, win, max_level, back=True, **kw):
    """pmv_lk_track_fb_levels as the header defines it, over the LK twin: forward at maxLevel min(fwd_top, max_level); backward, for the tracks
    with forward status 1, from the forward result with the points as initial flow at maxLevel min(back_top, max_level); a track whose
    forward status is 0 has back status 0, back err 0 and the bits of its forward position. -1 = max_level."""
    tw = lx.twin()
    lf_, lb_ = (max_level if t < 0 else min(t, max_level) for t in (fwd_top, back_top))
    xy, st, err = tw.track(prev, nxt, pts, init=init, flags=flags, win=win, max_level=lf_, **kw)
    if not back:
        return xy, st, err
    ok = st > 0
    bxy, bst, berr = xy.copy(), np.zeros(len(xy), np.uint8), np.zeros(len(xy), np.float32)
    if ok.any():
        bxy[ok], bst[ok], berr[ok] = tw.track(nxt, prev, xy[ok], init=np.ascontiguousarray(pts, np.float32).reshape(-1, 2)[ok], flags=flags & lx.EIG, win=win, max_level=lb_, **kw)
    return xy, st, err, bxy, bst, berr


# ---- the tracker step with a prediction (pmv_klt_set_prediction): stage 1 as include/pmv_hip.h defines it, on the CPU twins --------------
import klt_common as kc   # noqa: E402

VINS = dict(top_level=1, back_top_level=1, min_succ=10)


def prediction(cam, ids, xyz, **over):
    """a prediction as the tests hand it round: the camera (a dict of pmv.camera_params' keywords), the ids, their points, the setting"""
    return dict(dict(VINS, cam=cam, ids=np.ascontiguousarray(ids, np.int32), xyz=np.ascontiguousarray(xyz, np.float64).reshape(-1, 3)), **over)


def guesses_of(pred, ids, xy):
    """(guess (n0, 2) float32, joined): the projection of the prediction point with the track's id where it is ok, else the track's position"""
    guess = np.array(xy, np.float32).reshape(-1, 2)
    pxy, pok = project_twin().points(pred["cam"], pred["xyz"])
    where = {int(k): j for j, k in enumerate(pred["ids"])}
    joined = 0
    for i, k in enumerate(ids):
        j = where.get(int(k))
        if j is not None and pok[j]:
            guess[i] = pxy[j]
            joined += 1
    return guess, joined


class PredictOps(kc.TwinOps):
    """klt_common's twin stages under the LK setting lk = (win, max_level), with stage 1 from a prediction (or None: the plain stage 1);
    result: (consumed, joined, succ, fell_back) once track() ran - a step with n0 = 0 never calls it"""
    def __init__(self, prev, cur, ids, pred, lk=(32, 4)):
        super().__init__(prev, cur)
        self.ids, self.pred, self.lk = ids, pred, lk
        self.result = (1 if pred is not None else 0, 0, 0, 0)
        self.stage1 = None

    def track(self, xy, fb):
        win, ml = self.lk
        p = self.pred
        if p is None:
            a = twin_fb_levels(self.prev, self.cur, xy, None, 0, -1, -1, win, ml, back=fb)
        else:
            guess, joined = guesses_of(p, self.ids, xy)
            a = twin_fb_levels(self.prev, self.cur, xy, guess, 0, p["top_level"], p["back_top_level"], win, ml, back=fb)
            succ, fell = int((a[1] == 1).sum()), 0
            if succ < p["min_succ"]:
                a, fell = twin_fb_levels(self.prev, self.cur, xy, None, 0, -1, p["back_top_level"], win, ml, back=fb), 1
            self.result = (1, joined, succ, fell)
        self.stage1 = a
        return a if fb else a + (None, None, None)


def twin_predicted_step(state, prev, cur, p, pred, lk=(32, 4)):
    """(new state, (ids, ages, xy, prev_xy, counts), (consumed, joined, succ, fell_back), stage 1's outputs or None)"""
    ops = PredictOps(prev, cur, state["ids"], pred, lk)
    new, out = kc.compose(ops, state, p)
    return new, out, ops.result, ops.stage1


def points_for(cam, ids, target_xy, seed=0, jitter=1.5):
    """camera-frame points whose projection through `cam` lies within +-jitter px of target_xy: the pixel, displaced, is lifted by the twin
    lift and put at a depth of 2 .. 30"""
    rng = np.random.default_rng(seed)
    px = (np.asarray(target_xy, np.float64).reshape(-1, 2) + rng.uniform(-jitter, jitter, (len(ids), 2))).astype(np.float32)
    un, ok = lf.twin().points(cam, px)
    assert ok.all()
    z = rng.uniform(2.0, 30.0, len(ids))
    return np.stack([un[:, 0].astype(np.float64) * z, un[:, 1].astype(np.float64) * z, z], axis=1)


# ---- the scenes of the prediction tests: klt_common's tracker scene, state after the first (detecting) step, the step onto frame 1 --------
FAR = (3.0, 3.0, 1.0)   # a point whose projection through predict_camera lies some hundreds of px outside the frame, and is ok


def predict_camera(w, h):
    """a mild barrel distortion, and iterations enough for the lift to invert the projection to 1e-5 px over the whole frame"""
    return lf.scene_camera(w, h, k1=-0.1, iters=20)


def scene_case(pmv, w, h, **over):
    """a case = (key, frames, tracker params, camera): klt_common's tracker scene at w x h"""
    return (("scene", w, h, tuple(sorted(over.items()))), kc.scene(pmv, w, h), kc.params(**over), predict_camera(w, h))


def big_case(pmv):
    """klt_common's 1500-track case on the 517 x 261 frames: two 1024-chunks in the join kernel"""
    return (("big",), kc.big_pair(pmv), kc.params(**kc.BIG), predict_camera(kc.W_BIG, kc.H_BIG))


def state_of(case):
    """the twin's state after the step that only detects"""
    key, frames, p, _ = case
    return gc.cached(("predict-state", key), lambda: kc.twin_step(kc.empty_state(), frames[0], frames[0], p)[0])


def plain_step(case, lk=(32, 4)):
    """the twin's step onto frame 1 without a prediction under lk: twin_predicted_step's 4-tuple"""
    key, frames, p, _ = case
    return gc.cached(("predict-plain", key, lk), lambda: twin_predicted_step(state_of(case), frames[0], frames[1], p, None, lk))


def truth(case, lk=(32, 4)):
    """where the plain step's LK puts the state's tracks in frame 1 (a track it loses: its own position)"""
    a = plain_step(case, lk)[3]
    return np.where((a[1] == 1)[:, None], a[0], state_of(case)["xy"]).astype(np.float32)


def good_prediction(case, lk=(32, 4), seed=1, **setting):
    """every track predicted within 1.5 px of where the plain step's LK finds it"""
    s0, cam = state_of(case), case[3]
    return prediction(cam, s0["ids"], points_for(cam, s0["ids"], truth(case, lk), seed=seed), **setting)


def far_prediction(case, **setting):
    """every track predicted far outside the frame"""
    s0 = state_of(case)
    return prediction(case[3], s0["ids"], np.tile(FAR, (len(s0["ids"]), 1)), **setting)


def partial_prediction(case, lk, keep, **setting):
    """good_prediction for the tracks `keep` (indices into the state), far_prediction for the others"""
    good = good_prediction(case, lk, **setting)
    xyz = np.tile(FAR, (len(good["ids"]), 1)).astype(np.float64)
    xyz[keep] = good["xyz"][keep]
    return dict(good, xyz=xyz)


def predicted_step(case, pred, lk=(32, 4)):
    """twin_predicted_step onto frame 1 from the case's state"""
    _, frames, p, _ = case
    return twin_predicted_step(state_of(case), frames[0], frames[1], p, pred, lk)


def boundary_tracks(case, lk, min_succ):
    """state indices of tracks that the predicted pass of good_prediction tracks (status 1), min_succ + 2 of them spread over the list: a
    track's LK does not depend on the other tracks, so a prediction that is good for k of them and far for the rest has exactly k successes"""
    a = predicted_step(case, good_prediction(case, lk, min_succ=min_succ), lk)[3]
    tracked = np.flatnonzero(a[1] == 1)
    assert len(tracked) >= min_succ + 5
    return tracked[::max(1, len(tracked) // (min_succ + 2))]
