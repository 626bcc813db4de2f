"""Shared by the tests of the device-resident KLT tracker (pmv_klt_*): the scenes, the per-frame policy in numpy, and the two yardsticks that
pmv_klt_step is defined as a composition of - twin_step (the CPU twins of the single calls, through their Python wrappers) and calls_step
(the Context's single calls). Everything handed out is computed once and shared; callers must not modify it.

The scene: 6 consecutive frames of pmv.synth_sequence with a textured block pasted into each frame. The block moves against the
background's motion, so its tracks are LK-consistent but violate the epipolar geometry of the rest: rejectWithF has something to reject."""
import numpy as np

import fundamental_common as fc
import gftt_common as gc
import lkx_common as lc
import refill_common as rc
import subpix_common as sc

SIZES = [(320, 200), (203, 87)]
N_FRAMES = 6
W_BIG, H_BIG = rc.W1, rc.H1   # the 517 x 261 frame of the refill tests
# a VINS-style front end: MAX_CNT 150, BORDER_SIZE 1, forward-backward 0.5 px, F_THRESHOLD 1.0, MIN_DIST 10 (the keywords of pmv.klt_params)
DEFAULTS = dict(target=150, border=1, fb_max_dist=0.5, reject_f=True, f_threshold=1.0, f_confidence=0.99, radius=10, quality=0.01, min_dist=10.0, block_size=3,
                use_harris=False, k=0.04, subpix=False, subpix_win=(5, 5), subpix_zero_zone=(-1, -1), subpix_max_iter=30, subpix_eps=0.01)
# the defaults and their four single deviations
SETTINGS = {
    "default": {},
    "fb_off": dict(fb_max_dist=-1.0),
    "f_off": dict(reject_f=False),
    "subpix": dict(subpix=True),
    "block5_harris": dict(block_size=5, use_harris=True),
}
TARGETS = [1, 63, 64, 65, 257]
NO_MODEL_THRESHOLD = 1e-15  # an F threshold at which no seven-point model gathers 7 inliers: asserted on the twin (tests/test_klt_twin.py)
# the 517 x 261 case: radius and min_dist small enough for more than 1024 tracks (two chunks of the compaction)
BIG = dict(target=1500, radius=3, min_dist=3.0, quality=0.001)


def params(**over):
    p = dict(DEFAULTS)
    p.update(over)
    return p


def scene(pmv, w, h, n=N_FRAMES):
    """(n, h, w) uint8: the synthetic sequence with the moving block"""
    def make():
        fr = pmv.synth_sequence(1007, 10, n, w, h, 0.58 * w, 0.58 * w, w / 2, h / 2)[0].copy()
        bw, bh = max(24, w // 6) // 4 * 4, max(20, h // 5) // 4 * 4
        rng = np.random.default_rng(23)
        tex = np.kron(rng.integers(0, 256, (bh // 4, bw // 4)), np.ones((4, 4))).astype(np.uint8)   # 4 x 4 blocks of noise: strong corners
        for i in range(n):
            x0, y0 = w // 2 - bw // 2 - 6 + 3 * i, h // 2 - bh // 2 + 4 - 2 * i
            fr[i, y0:y0 + bh, x0:x0 + bw] = tex
        return fr
    return gc.cached(("klt-scene", w, h, n), make)


def empty_state():
    return dict(ids=np.zeros(0, np.int32), ages=np.zeros(0, np.int32), xy=np.zeros((0, 2), np.float32), next_id=0)


# ---- the policy between the calls (float32 arithmetic, round half to even) -------------------------------------------------------------
def in_border(xy, border, w, h):
    r = np.rint(np.asarray(xy, np.float32).reshape(-1, 2))
    return (r[:, 0] >= border) & (r[:, 0] < w - border) & (r[:, 1] >= border) & (r[:, 1] < h - border)


def fb_ok(prev, back, fb_max_dist):
    d = np.asarray(back, np.float32).reshape(-1, 2) - np.asarray(prev, np.float32).reshape(-1, 2)
    dx2, dy2 = d[:, 0] * d[:, 0], d[:, 1] * d[:, 1]
    assert dx2.dtype == np.float32
    return (dx2 + dy2) <= np.float32(float(fb_max_dist) * float(fb_max_dist))


class TwinOps:
    """the stages on the CPU twins; `prev`, `cur`: (h, w) uint8 frames"""
    def __init__(self, prev, cur):
        self.prev, self.cur = prev, cur
        self.h, self.w = cur.shape

    def track(self, xy, fb):
        if fb:
            return lc.twin().track_fb(self.prev, self.cur, xy)
        return lc.twin().track(self.prev, self.cur, xy) + (None, None, None)

    def fundamental(self, p1, p2, thr, conf):
        found, _, mask, drawn, _ = fc.twin().find(np.ascontiguousarray(p1, np.float32), np.ascontiguousarray(p2, np.float32), thr, conf)
        return found, mask, drawn

    def keep(self, xy, p):
        self._mask = rc.twin().mask(self.w, self.h, xy, p["radius"])
        return self._mask[0]

    def corners(self, xy, want, p):
        return gc.twin().corners(self.cur, (0, 0, self.w, self.h), want, quality=p["quality"], min_dist=p["min_dist"], mask=self._mask[1], block_size=p["block_size"],
                                 use_harris=p["use_harris"], k=p["k"])

    def refine(self, pts, p):
        return sc.twin().refine(self.cur, pts, win=p["subpix_win"], zero_zone=p["subpix_zero_zone"], max_iter=p["subpix_max_iter"], eps=p["subpix_eps"])[0]


class CallOps:
    """the stages on the Context's single calls"""
    def __init__(self, ctx, prev_slot, cur_slot, w, h):
        self.ctx, self.ps, self.cs, self.w, self.h = ctx, prev_slot, cur_slot, w, h

    def track(self, xy, fb):
        if fb:
            return self.ctx.lk_track_fb(self.ps, self.cs, xy)
        return self.ctx.lk_track_ex(self.ps, self.cs, xy) + (None, None, None)

    def fundamental(self, p1, p2, thr, conf):
        found, _, mask, drawn = self.ctx.find_fundamental_mat(p1, p2, thr, conf)
        return found, mask, drawn

    def _refill(self, xy, want, p):
        return self.ctx.detect_gftt_refill(self.cs, want, xy, p["radius"], quality=p["quality"], min_dist=p["min_dist"], block_size=p["block_size"],
                                           use_harris=p["use_harris"], k=p["k"])

    def keep(self, xy, p):
        return self._refill(xy, p["target"], p)[0]

    def corners(self, xy, want, p):
        return self._refill(xy, want, p)[1]   # (the yardstick calls refill twice: out_keep does not depend on max_corners)

    def refine(self, pts, p):
        return self.ctx.corner_subpix(self.cs, pts, win=p["subpix_win"], zero_zone=p["subpix_zero_zone"], max_iter=p["subpix_max_iter"], eps=p["subpix_eps"])


def compose(ops, state, p):
    """the seven stages of include/pmv_hip.h on `ops`: (new state, (ids, ages, xy, prev_xy, counts))"""
    ids, ages, prev = state["ids"], state["ages"], np.ascontiguousarray(state["xy"], np.float32).reshape(-1, 2)
    n0 = len(ids)
    fb = p["fb_max_dist"] is not None and p["fb_max_dist"] >= 0
    cur = prev
    if n0:
        cur, st, _, back, bst, _ = ops.track(prev, fb)
        ok = st == 1
        if fb:
            ok &= (bst == 1) & fb_ok(prev, back, p["fb_max_dist"])
        ok &= in_border(cur, p["border"], ops.w, ops.h)
        ids, ages, prev, cur = ids[ok], ages[ok] + 1, prev[ok], cur[ok]
    n1 = len(ids)
    f_found, f_drawn = -1, 0
    if p["reject_f"] and n1 >= 15:
        found, mask, f_drawn = ops.fundamental(prev, cur, p["f_threshold"], p["f_confidence"])
        f_found = int(found)
        ok = mask != 0   # no model: cv's status is all zero and every track goes
        ids, ages, prev, cur = ids[ok], ages[ok], prev[ok], cur[ok]
    n2 = len(ids)
    ok = ops.keep(cur, p) != 0
    ids, ages, prev, cur = ids[ok], ages[ok], prev[ok], cur[ok]
    n3 = len(ids)
    new = np.zeros((0, 2), np.float32)
    if p["target"] - n3 > 0:
        new = np.ascontiguousarray(ops.corners(cur, p["target"] - n3, p), np.int32).reshape(-1, 2).astype(np.float32)
        if p["subpix"] and len(new):
            new = ops.refine(new, p)
    m = len(new)
    nid = state["next_id"]
    out_ids = np.concatenate([ids, np.arange(nid, nid + m)]).astype(np.int32)
    out_ages = np.concatenate([ages, np.ones(m)]).astype(np.int32)
    out_xy = np.concatenate([cur.reshape(-1, 2), new]).astype(np.float32)
    out_prev = np.concatenate([prev.reshape(-1, 2), new]).astype(np.float32)
    counts = np.asarray([n0, n1, n2, n3, m, f_found, f_drawn, 0], np.int32)
    return dict(ids=out_ids, ages=out_ages, xy=out_xy, next_id=nid + m), (out_ids, out_ages, out_xy, out_prev, counts)


def twin_step(state, prev, cur, p):
    return compose(TwinOps(prev, cur), state, p)


def calls_step(ctx, state, prev_slot, cur_slot, p):
    w, h = ctx_frame_size(ctx, cur_slot)
    return compose(CallOps(ctx, prev_slot, cur_slot, w, h), state, p)


_sizes = {}


def note_frame_size(ctx, slot, w, h):
    """calls_step needs the size of the frame in a slot for inBorder: the uploader tells it here"""
    _sizes[id(ctx), slot] = (w, h)


def ctx_frame_size(ctx, slot):
    return _sizes[id(ctx), slot]


def upload(ctx, frames, first_slot=0):
    for i, f in enumerate(frames):
        ctx.frame_upload(first_slot + i, f)
        note_frame_size(ctx, first_slot + i, f.shape[1], f.shape[0])


def twin_run(frames, p, key, state=None):
    """the twin over consecutive frames from `state` (default: empty, so the first step only detects): the list of (state, outputs) per
    step, step 0 running on (frames[0], frames[0]); computed once per key"""
    def make():
        s, out = state or empty_state(), []
        for i in range(len(frames)):
            s, o = twin_step(s, frames[max(i - 1, 0)], frames[i], p)
            out.append((s, o))
        return out
    return gc.cached(("klt-run", key), make)


def scene_run(pmv, w, h, name="default", **over):
    p = params(**SETTINGS[name], **over)
    return p, twin_run(scene(pmv, w, h), p, (w, h, name, tuple(sorted(over.items()))))


def big_pair(pmv):
    return gc.cached("klt-big", lambda: pmv.synth_sequence(1007, 10, 3, W_BIG, H_BIG, 0.58 * W_BIG, 0.58 * W_BIG, W_BIG / 2, H_BIG / 2)[0])


def big_run(pmv):
    p = params(**BIG)
    return p, twin_run(big_pair(pmv), p, "big")


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same(got, want):
    """byte for byte: ids, ages, xy, prev_xy, counts"""
    names = ("ids", "ages", "xy", "prev_xy", "counts")
    for k, (g, x) in enumerate(zip(got, want)):
        assert g.shape == x.shape, f"{names[k]}: shape {g.shape} != {x.shape}"
        assert np.array_equal(bits(g), bits(x)), f"{names[k]} differ"
