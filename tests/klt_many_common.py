"""Shared by the tests of pmv_klt_step_many: the yardstick is klt_common's CPU twin, one solo run per tracker (computed once per key and
shared; callers must not modify what they get). A group member is (params, twin run, slot rule): slot rule(i) = (prev_slot, cur_slot) of
the member's step i on a context whose slot k holds frame k of the scene."""
import ctypes as C

import numpy as np

import klt_common as kc

INVALID, CAPACITY = -2, -3
CANARY = -7


def forward(i):
    return max(i - 1, 0), i


def backward(i):
    """the scene's six frames in reversed order, on the slots of the forward upload"""
    return 5 - max(i - 1, 0), 5 - i


def forward_member(pmv, w, h, name="default", **over):
    p, run = kc.scene_run(pmv, w, h, name, **over)
    return p, run, forward


def reversed_run(pmv, w, h, name="default", **over):
    p = kc.params(**kc.SETTINGS[name], **over)
    return p, kc.twin_run(kc.scene(pmv, w, h)[::-1], p, ("many-rev", w, h, name, tuple(sorted(over.items()))))


def backward_member(pmv, w, h, name="default", **over):
    p, run = reversed_run(pmv, w, h, name, **over)
    return p, run, backward


def no_model_run(pmv, w, h):
    p = kc.params(f_threshold=kc.NO_MODEL_THRESHOLD)
    return p, kc.twin_run(kc.scene(pmv, w, h), p, ("many-no-model", w, h))


def late_run(pmv, w, h, name="default", **over):
    """a tracker that starts on frame 3 of the scene: three steps"""
    p = kc.params(**kc.SETTINGS[name], **over)
    return p, kc.twin_run(kc.scene(pmv, w, h)[3:], p, ("many-late", w, h, name, tuple(sorted(over.items()))))


def counts(run):
    return np.stack([o[4] for _, o in run]).astype(np.int64)


def make_ctx(factory, frames, max_tracks=2048, n_slots=None):
    h, w = frames[0].shape
    ctx = factory(w, h, n_slots=n_slots or len(frames), max_tracks=max_tracks)
    kc.upload(ctx, frames)
    return ctx


def step_group(ctx, trackers, members, i):
    """one many-call for step i of every member; every tracker equals its solo twin run byte for byte"""
    slots = [m[2](i) for m in members]
    got = ctx.klt_step_many(trackers, [s[0] for s in slots], [s[1] for s in slots])
    assert len(got) == len(members)
    for j, (g, m) in enumerate(zip(got, members)):
        try:
            kc.same(g, m[1][i][1])
        except AssertionError as e:
            raise AssertionError(f"tracker {j} of the group, step {i}: {e}") from None
    return got


def run_group(ctx, members, steps=kc.N_FRAMES):
    trackers = [ctx.klt_create(**m[0]) for m in members]
    outs = [step_group(ctx, trackers, members, i) for i in range(steps)]
    for t, last in zip(trackers, outs[-1]):
        kc.same(t.get_tracks(), last[:3])
        t.close()
    return outs


def last_error(ctx):
    return ctx.lib.pmv_last_error(ctx.h).decode()


def raw_many(ctx, ids, prev_slots, cur_slots, stride, n_trk=None, null=None):
    """the C call on canary-filled outputs: (return code, outputs untouched); null names one array to pass as NULL"""
    fn = ctx.lib.pmv_klt_step_many
    vp = C.c_void_p
    fn.argtypes = [vp, C.c_int, vp, vp, vp, vp, vp, vp, vp, C.c_int, vp, vp]
    k = max(len(ids), 1)
    a = dict(ids=np.asarray(ids, np.int32), prev_slots=np.asarray(prev_slots, np.int32), cur_slots=np.asarray(cur_slots, np.int32),
             out_ids=np.full(k * max(stride, 1), CANARY, np.int32), out_ages=np.full(k * max(stride, 1), CANARY, np.int32),
             out_xy=np.full(2 * k * max(stride, 1), CANARY, np.float32), out_prev=np.full(2 * k * max(stride, 1), CANARY, np.float32),
             out_n=np.full(k, CANARY, np.int32), out_counts=np.full(8 * k, CANARY, np.int32))
    ptr = {name: (None if name == null else v.ctypes.data) for name, v in a.items()}
    rc = fn(ctx.h, len(ids) if n_trk is None else n_trk, ptr["ids"], ptr["prev_slots"], ptr["cur_slots"], ptr["out_ids"], ptr["out_ages"], ptr["out_xy"], ptr["out_prev"],
            stride, ptr["out_n"], ptr["out_counts"])
    untouched = all((a[name] == CANARY).all() for name in ("out_ids", "out_ages", "out_xy", "out_prev", "out_n", "out_counts"))
    return rc, untouched
