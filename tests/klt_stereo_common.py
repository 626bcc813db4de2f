"""Shared by the tests of the stereo tracker step (pmv_klt_step_stereo, pmv_klt_step_many_stereo): the right frame of a left frame, the stereo
rule of include/pmv_hip.h in numpy, and its two yardsticks - twin_stereo (the CPU twin of LK) and calls_stereo (the Context's single LK calls
on the pair (cur_slot, right_slot)). Everything handed out is computed once and shared; callers must not modify it.

The right frame: the left frame shifted by two disparities - 4 px in the upper half, 9 px below (2 and 3 on the 40 x 40 pair) - with an
occluder of 4 x 4-block noise pasted over it, so that some tracks of the left list have nothing to match."""
import ctypes as C

import numpy as np

import gftt_common as gc
import klt_common as kc
import lkx_common as lc

INVALID, CAPACITY = -2, -3
CANARY = -7
STEREO = {"fb": dict(fb_max_dist=0.5, border=1), "fb_off": dict(fb_max_dist=-1.0, border=1)}
SMALL = dict(target=20, radius=3, min_dist=3.0, reject_f=False)   # the 40 x 40 pair's tracker


def right_of(left, d_top=4, d_bottom=9, occluder=True):
    """right[y, x] = left[y, min(x + d, w - 1)], d = d_top for y < h // 2 and d_bottom below; then the occluder at (w // 8, h // 8)"""
    h, w = left.shape
    x = np.arange(w)
    right = np.empty_like(left)
    right[:h // 2] = left[:h // 2][:, np.minimum(x + d_top, w - 1)]
    right[h // 2:] = left[h // 2:][:, np.minimum(x + d_bottom, w - 1)]
    if occluder:
        ow, oh = max(16, w // 5), max(12, h // 4)
        rng = np.random.default_rng(41)
        tex = np.kron(rng.integers(0, 256, ((oh + 3) // 4, (ow + 3) // 4)), np.ones((4, 4))).astype(np.uint8)[:oh, :ow]
        right[h // 8:h // 8 + oh, w // 8:w // 8 + ow] = tex
    return right


def rights(frames, key, **kw):
    """the right frames of a sequence of left frames, (n, h, w) uint8"""
    return gc.cached(("stereo-right", key), lambda: np.stack([right_of(f, **kw) for f in frames]))


def scene_rights(pmv, w, h):
    return rights(kc.scene(pmv, w, h), (w, h))


def small_pair(pmv):
    """(left frames, right frames) of the 40 x 40 pair: disparities 2 and 3, no occluder"""
    left = gc.cached("stereo-40", lambda: pmv.synth_sequence(1007, 10, 2, 40, 40, 23.2, 23.2, 20, 20)[0])
    return left, rights(left, "40x40", d_top=2, d_bottom=3, occluder=False)


def gray_pair(w, h):
    return np.full((2, h, w), 128, np.uint8)


# ---- the rule of stage 8 ---------------------------------------------------------------------------------------------------------------
def rule(xy, tracked, st, w, h):
    """(right xy (n, 2) float32, right status (n,) uint8) from the outputs of the LK call on the list xy; st: a STEREO setting"""
    xy = np.ascontiguousarray(xy, np.float32).reshape(-1, 2)
    if len(xy) == 0:
        return np.zeros((0, 2), np.float32), np.zeros(0, np.uint8)
    rxy, s, _, back, bst, _ = tracked
    ok = s == 1
    if st["fb_max_dist"] >= 0:
        ok &= (bst == 1) & kc.fb_ok(xy, back, st["fb_max_dist"])
    ok &= kc.in_border(rxy, st["border"], w, h)
    return np.ascontiguousarray(rxy, np.float32).reshape(-1, 2), ok.astype(np.uint8)


def twin_stereo(cur, right, xy, st):
    """the stereo outputs of the list xy on the CPU twin"""
    if len(xy) == 0:
        return rule(xy, None, st, 0, 0)
    fb = st["fb_max_dist"] >= 0
    t = lc.twin().track_fb(cur, right, xy) if fb else lc.twin().track(cur, right, xy) + (None, None, None)
    return rule(xy, t, st, cur.shape[1], cur.shape[0])


def calls_stereo(ctx, cur_slot, right_slot, xy, st):
    """the stereo outputs of the list xy through the Context's single LK calls"""
    if len(xy) == 0:
        return rule(xy, None, st, 0, 0)
    fb = st["fb_max_dist"] >= 0
    t = ctx.lk_track_fb(cur_slot, right_slot, xy) if fb else ctx.lk_track_ex(cur_slot, right_slot, xy) + (None, None, None)
    w, h = kc.ctx_frame_size(ctx, right_slot)
    return rule(xy, t, st, w, h)


def twin_stereo_run(lefts, rts, run, st, key):
    """twin_stereo for every step of a klt_common twin run over `lefts`: a list of (right xy, right status); computed once per key"""
    return gc.cached(("stereo-run", key), lambda: [twin_stereo(lefts[i], rts[i], run[i][1][2], st) for i in range(len(run))])


def with_matched(out5, rst):
    """a step's 5-tuple with counts[7] = the number of matched tracks, as the stereo step returns it"""
    c = out5[4].copy()
    c[7] = int(np.count_nonzero(rst))
    return out5[:4] + (c,)


def same_right(got, want):
    """right xy as uint32, right status as bytes"""
    for name, g, x in (("right_xy", got[0], want[0]), ("right_status", got[1], want[1])):
        assert g.shape == x.shape and g.dtype == x.dtype, f"{name}: {g.dtype}{g.shape} != {x.dtype}{x.shape}"
        assert np.array_equal(kc.bits(g), kc.bits(x)), f"{name} differ"


def same_stereo(got7, want5, want_right):
    """a stereo step's 7-tuple against a plain step's 5-tuple and the stereo outputs of its list"""
    kc.same(got7[:5], with_matched(want5, want_right[1]))
    same_right(got7[5:], want_right)


def upload_pair(ctx, lefts, rts):
    """left frame i in slot i, right frame i in slot len(lefts) + i"""
    kc.upload(ctx, lefts)
    kc.upload(ctx, rts, first_slot=len(lefts))


def make_ctx(factory, lefts, rts, max_tracks=2048, extra_slots=0):
    h, w = lefts[0].shape
    ctx = factory(w, h, n_slots=len(lefts) + len(rts) + extra_slots, max_tracks=max_tracks)
    upload_pair(ctx, lefts, rts)
    return ctx


def last_error(ctx):
    return ctx.lib.pmv_last_error(ctx.h).decode()


def _canaries(k, stride):
    s = max(stride, 1)
    return dict(out_ids=np.full(k * s, CANARY, np.int32), out_ages=np.full(k * s, CANARY, np.int32), out_xy=np.full(2 * k * s, CANARY, np.float32),
                out_prev=np.full(2 * k * s, CANARY, np.float32), out_rxy=np.full(2 * k * s, CANARY, np.float32), out_rst=np.full(k * s, 0xA5, np.uint8),
                out_n=np.full(k, CANARY, np.int32), out_counts=np.full(8 * k, CANARY, np.int32))


def _untouched(a):
    return all((a[name] == (0xA5 if name == "out_rst" else CANARY)).all() for name in a)


def raw_step(ctx_h, lib, tid, prev_slot, cur_slot, right_slot, cap, null=None):
    """the C call on pattern-filled outputs: (return code, outputs untouched, the outputs); null names one array to pass as NULL"""
    fn = lib.pmv_klt_step_stereo
    vp, ci = C.c_void_p, C.c_int
    fn.argtypes = [vp, ci, ci, ci, ci, vp, vp, vp, vp, vp, vp, ci, vp, vp]
    a = _canaries(1, cap)
    ptr = {name: (None if name == null else v.ctypes.data) for name, v in a.items()}
    rc = fn(ctx_h, tid, prev_slot, cur_slot, right_slot, ptr["out_ids"], ptr["out_ages"], ptr["out_xy"], ptr["out_prev"], ptr["out_rxy"], ptr["out_rst"], cap, ptr["out_n"],
            ptr["out_counts"])
    return rc, _untouched(a), a


def raw_many(ctx_h, lib, ids, prev_slots, cur_slots, right_slots, stride, null=None):
    """the same for pmv_klt_step_many_stereo"""
    fn = lib.pmv_klt_step_many_stereo
    vp, ci = C.c_void_p, C.c_int
    fn.argtypes = [vp, ci, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, ci, vp, vp]
    k = max(len(ids), 1)
    a = _canaries(k, stride)
    inp = dict(ids=np.asarray(ids, np.int32), prev_slots=np.asarray(prev_slots, np.int32), cur_slots=np.asarray(cur_slots, np.int32),
               right_slots=np.asarray(right_slots, np.int32))
    ptr = {name: (None if name == null else v.ctypes.data) for name, v in {**inp, **a}.items()}
    rc = fn(ctx_h, len(ids), ptr["ids"], ptr["prev_slots"], ptr["cur_slots"], ptr["right_slots"], ptr["out_ids"], ptr["out_ages"], ptr["out_xy"], ptr["out_prev"],
            ptr["out_rxy"], ptr["out_rst"], stride, ptr["out_n"], ptr["out_counts"])
    return rc, _untouched(a), a
