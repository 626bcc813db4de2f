"""Shared by the tests of the tracker's observation setting (pmv_klt_set_observe: stage 9, and stage 3 on undistorted points): the cameras of
the scenes, the stage-9 yardstick on a step's outputs, and the twin run whose stage 3 takes the virtual-camera points. Everything handed out
is computed once and shared; callers must not modify it."""
import numpy as np

import fundamental_common as fc
import gftt_common as gc
import klt_common as kc
import klt_stereo_common as ks   # noqa: F401  (the stereo scenes of the callers)
import lift_common as lf

INVALID, CAPACITY = -2, -3
DT = 0.05
F_FOCAL = 460.0
# the scene of the undistorted-F tests: klt_common.scene at SIZES[0], seen through a strong barrel distortion (k1 = -0.3). The frames are the
# pinhole scene's, so the lifted points obey the background's epipolar geometry less well than the pixels and F's mask changes.
F_SIZE = kc.SIZES[0]


def left_camera(w, h):
    return lf.scene_camera(w, h)


def right_camera(w, h):
    """another camera: all eight coefficients, other intrinsics, cv's default iteration count"""
    return lf.all_terms(w, h)


def f_camera():
    return lf.scene_camera(*F_SIZE, k1=-0.3, iters=8)


def expected(cam, dt, out5, right_cam=None, right=None):
    """stage 9 on a step's outputs (ids, ages, xy, prev_xy, counts) and, with `right` = (right_xy, right_status), a stereo step's"""
    _, ages, xy, prev, _ = out5[:5]
    if right_cam is not None and right is not None:
        return lf.twin().observe(cam, dt, ages, xy, prev, right_cam, right[0], right[1])
    return lf.twin().observe(cam, dt, ages, xy, prev)


NAMES = ("un_xy", "vel", "ok", "right_un_xy", "right_ok")


def same_observations(got, want):
    lf.same(got, want, NAMES)


class LiftedTwinOps(kc.TwinOps):
    """klt_common's twin stages with stage 3 on the virtual-camera points; log: per F call (lifted mask, pixel mask of the same survivors)"""
    def __init__(self, prev, cur, cam, f_focal, log):
        super().__init__(prev, cur)
        self.cam, self.f_focal, self.log = cam, f_focal, log

    def fundamental(self, p1, p2, thr, conf):
        q1, q2 = lf.twin().f_points(self.cam, self.f_focal, self.w, self.h, p1, p2)
        found, _, mask, drawn, _ = fc.twin().find(q1, q2, thr, conf)
        pixel = super().fundamental(p1, p2, thr, conf)[1]
        self.log.append((mask.copy(), pixel.copy()))
        return found, mask, drawn


def lifted_run(frames, p, cam, f_focal, key):
    """klt_common.twin_run with undistorted_f: (the list of (state, outputs) per step, the F log)"""
    def make():
        s, out, log = kc.empty_state(), [], []
        for i in range(len(frames)):
            s, o = kc.compose(LiftedTwinOps(frames[max(i - 1, 0)], frames[i], cam, f_focal, log), s, p)
            out.append((s, o))
        return out, log
    return gc.cached(("observe-lifted-run", key), make)


def f_scene_run(pmv, **over):
    w, h = F_SIZE
    p = kc.params(**over)
    run, log = lifted_run(kc.scene(pmv, w, h), p, f_camera(), F_FOCAL, ("f-scene", tuple(sorted(over.items()))))
    return p, run, log


def last_error(ctx):
    return ctx.lib.pmv_last_error(ctx.h).decode()


def counts(run):
    return np.stack([o[4] for _, o in run]).astype(np.int64)
