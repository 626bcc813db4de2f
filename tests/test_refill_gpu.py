"""pmv_detect_gftt_refill on the GPU, bit for bit: the keep bytes and the painted mask against the CPU twin (tests/twin/refill_twin.cpp),
the corners against pmv_detect_gftt_frame given the twin's mask as a host mask and against gftt_twin_cell with that mask. One 768x512
context with max_tracks = 2048: slot 0 holds the 517x261 scene, slot 1 a 40x40 frame."""
import numpy as np
import pytest

import gftt_common as gc
import gftt_frame_common as gf
import refill_common as rc

pytestmark = pytest.mark.gpu

W, H = rc.W1, rc.H1
REGION = (13, 7, 301, 199)   # odd width, not at the origin
_state = {}


def _ctx(pmv, gpu_ctx_factory):
    if "ctx" not in _state:
        ctx = gpu_ctx_factory(gf.W2, gf.H2, n_slots=2, max_tracks=2048)
        ctx.frame_upload(0, gf.rect_frame(pmv, W, H))
        ctx.frame_upload(1, gc.noise_frame(40, 40))
        _state["ctx"] = ctx
    return _state["ctx"]


def _check(pmv, ctx, slot, img, xy, radius, prio=None, base=None, roi=None, max_corners=150, what="", **kw):
    """one refill call against the twin (keep, mask), the host-mask path and the corner twin; returns (keep, corners)"""
    h, w = img.shape
    want_keep, want_mask = rc.twin().mask(w, h, xy, radius, prio, base)
    r = gf.whole(img) if roi is None else np.asarray(roi, np.int32)
    before = ctx.debug_refill_stats()
    keep, corners = ctx.detect_gftt_refill(slot, max_corners, xy, radius, priorities=prio, base_mask=base, roi=roi, **kw)
    after = ctx.debug_refill_stats()
    painted = ctx.debug_refill_mask()
    print(f"{what}: kept {int(keep.sum())} of {len(keep)}, {len(corners)} corners, {int((painted == 0).sum())} bytes cleared")
    assert np.array_equal(keep, want_keep), f"{what}: keep bytes differ at {np.flatnonzero(keep != want_keep)[:6]}"
    sub = want_mask[r[1]:r[1] + r[3], r[0]:r[0] + r[2]]
    assert painted.shape == sub.shape and np.array_equal(painted, sub), f"{what}: {int((painted != sub).sum())} mask bytes differ"
    assert after[0] == before[0] + 1 and after[1:3] == before[1:3]
    assert after[3] - before[3] == (0 if base is None else int(r[2]) * int(r[3])), f"{what}: {after[3] - before[3]} mask bytes crossed the bus"
    host = ctx.detect_gftt_frame(slot, max_corners, mask=want_mask, roi=roi, **kw)
    assert np.array_equal(corners, host), f"{what}: the corners differ from pmv_detect_gftt_frame's with the twin's mask"
    twin = gc.twin().corners(img, r, max_corners, mask=want_mask, **kw)
    assert np.array_equal(corners, twin), f"{what}: the corners differ from gftt_twin_cell's with the twin's mask"
    return keep, corners


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 300, 1025, 2048])
def test_track_counts_on_the_whole_frame(pmv, gpu_ctx_factory, n):
    """1025 and 2048 tracks at radius 1: more than 64 and more than 1024 are kept, so the kept list crosses the lanes of the wavefront
    and the chunks of the walk"""
    ctx = _ctx(pmv, gpu_ctx_factory)
    img = gf.rect_frame(pmv, W, H)
    radius = 1 if n > 1000 else 7
    xy, prio = rc.tracks(W, H, max(n, 1))
    keep, corners = _check(pmv, ctx, 0, img, xy[:n], radius, prio[:n], what=f"n = {n}", min_dist=30.0)
    if n >= 300:
        assert 0 < keep.sum() < n
    if n == 1025:
        assert keep.sum() > 64
    if n == 2048:
        assert keep.sum() > 1024 + 64
    if n > 0:
        first = np.lexsort((np.arange(n), -prio[:n].astype(np.int64)))[0]
        assert keep[first] == 1, "the first in order is always kept without a base mask"


@pytest.mark.parametrize("radius", [0, 1, 7, 30, 255])
def test_radii_on_a_region(pmv, gpu_ctx_factory, radius):
    """no limit (max_corners 0), block size 5, the tracks all over the frame, painting and detection on the region only"""
    ctx = _ctx(pmv, gpu_ctx_factory)
    img = gf.rect_frame(pmv, W, H)
    xy, prio = rc.tracks(W, H, 300)
    keep, _ = _check(pmv, ctx, 0, img, xy, radius, prio, roi=REGION, max_corners=0, what=f"radius {radius}", min_dist=10.0, block_size=5)
    assert 0 < keep.sum() <= 300 and (radius < 7 or keep.sum() < 300)


@pytest.mark.parametrize("harris", [False, True])
@pytest.mark.parametrize("b", [3, 5])
def test_block_sizes_and_harris(pmv, gpu_ctx_factory, b, harris):
    ctx = _ctx(pmv, gpu_ctx_factory)
    img = gf.rect_frame(pmv, W, H)
    xy, _ = rc.tracks(W, H, 300)
    for mc, roi in ((150, None), (0, REGION)):
        _, corners = _check(pmv, ctx, 0, img, xy, 7, None, roi=roi, max_corners=mc, what=f"block {b}, harris {harris}, max_corners {mc}", min_dist=7.0, block_size=b,
                            use_harris=harris, k=0.04)
        assert len(corners) > 10


def test_a_40x40_frame(pmv, gpu_ctx_factory):
    ctx = _ctx(pmv, gpu_ctx_factory)
    img = gc.noise_frame(40, 40)
    xy, prio = rc.tracks(40, 40, 65)
    for radius in (0, 3, 30):
        keep, _ = _check(pmv, ctx, 1, img, xy, radius, prio, what=f"40x40, radius {radius}", min_dist=3.0)
        assert 0 < keep.sum() <= 65 and (radius == 0 or keep.sum() < 65)


def test_no_tracks_and_no_base_mask_is_the_unmasked_frame_call(pmv, gpu_ctx_factory):
    ctx = _ctx(pmv, gpu_ctx_factory)
    for roi in (None, REGION):
        keep, corners = ctx.detect_gftt_refill(0, 150, np.zeros((0, 2), np.float32), 30, roi=roi, min_dist=30.0)
        assert len(keep) == 0 and (ctx.debug_refill_mask() == 255).all()
        assert np.array_equal(corners, ctx.detect_gftt_frame(0, 150, roi=roi, min_dist=30.0)) and len(corners) > 20


def test_a_base_mask_with_a_stride_above_w(pmv, gpu_ctx_factory):
    ctx = _ctx(pmv, gpu_ctx_factory)
    img = gf.rect_frame(pmv, W, H)
    base = rc.base_mask(W, H)
    xy, prio = rc.tracks(W, H, 300)
    pts = rc.np_round(xy)
    under = base[pts[:, 1], pts[:, 0]]
    for roi in (None, REGION):
        keep, _ = _check(pmv, ctx, 0, img, xy, 10, prio, base=base, roi=roi, what=f"base mask, region {roi}", min_dist=10.0)
        assert (under == 0).any() and (under == 128).any() and not keep[under != 255].any(), "tracks on base bytes 0 and 128 are dropped"
        assert 0 < keep.sum() < (under == 255).sum()
    _check(pmv, ctx, 0, img, xy[:0], 10, None, base=base, what="base mask, no tracks", min_dist=10.0)


def test_tracks_outside_the_region_still_suppress_tracks_inside(pmv, gpu_ctx_factory):
    ctx = _ctx(pmv, gpu_ctx_factory)
    img = gf.rect_frame(pmv, W, H)
    x0, y0, cw, ch = REGION
    # pairs across the region's left and top border: the outer one is older, so the inner one goes; and a lone inner track stays
    xy = np.asarray([(x0 - 3, 100), (x0 + 2, 100), (200, y0 - 2), (200, y0 + 4), (150, 150)], np.float32)
    prio = np.asarray([9, 1, 9, 1, 0], np.int32)
    keep, _ = _check(pmv, ctx, 0, img, xy, 8, prio, roi=REGION, what="outside the region", min_dist=10.0)
    assert keep.tolist() == [1, 0, 1, 0, 1]
    whole, _ = ctx.detect_gftt_refill(0, 150, xy, 8, priorities=prio, min_dist=10.0)
    assert np.array_equal(whole, keep), "the keep bytes do not depend on the region"


def test_refusals_write_nothing(pmv, gpu_ctx_factory):
    ctx = _ctx(pmv, gpu_ctx_factory)
    P = pmv.GfttParams(0.01, 7.0, 3, 0, 0.04)
    good = np.asarray([(10, 10), (100, 50), (300, 200), (500, 250)], np.float32)
    small = np.zeros((H, W - 1), np.uint8)
    big = np.zeros((2049, 2), np.float32)

    def trk(i, x, y):
        t = good.copy()
        t[i] = (x, y)
        return t
    cases = [("null out_keep", rc.INVALID, dict(keep=None)), ("null track_xy", rc.INVALID, dict(xy=None)), ("radius -1", rc.INVALID, dict(radius=-1)),
             ("radius 256", rc.INVALID, dict(radius=256)), ("NaN", rc.INVALID, dict(xy=trk(2, np.nan, 5))), ("inf", rc.INVALID, dict(xy=trk(1, 5, np.inf))),
             ("beyond 1e6", rc.INVALID, dict(xy=trk(0, 2e6, 5))), ("right of the frame", rc.INVALID, dict(xy=trk(3, W - 0.4, 5))),
             ("below the frame", rc.INVALID, dict(xy=trk(3, 5, H - 0.5 + 0.01))), ("left of the frame", rc.INVALID, dict(xy=trk(0, -0.6, 5))),
             ("n = -1", rc.CAPACITY, dict(n=-1)), ("n above max_tracks", rc.CAPACITY, dict(xy=big, n=2049)),
             ("base_stride below w", rc.CAPACITY, dict(base=small, stride=W - 1)),
             ("region", rc.INVALID, dict(roi=(300, 0, 218, 100))), ("slot", rc.CAPACITY, dict(slot=9)), ("cap", rc.CAPACITY, dict(mc=51)),
             ("block size first, then n", rc.INVALID, dict(params=pmv.GfttParams(0.01, 7.0, 16, 0, 0.04), n=-1)),
             ("overflow", rc.OVERFLOW, dict(mc=0, cap=20))]
    fn = ctx.lib.pmv_detect_gftt_refill
    for what, code, a in cases:
        b = dict(slot=0, roi=None, mc=50, params=P, xy=good, prio=None, n=4, radius=5, base=None, stride=0, cap=50)
        b.update(a)
        keep = None if "keep" in a else np.full(2049, 9, np.uint8)
        out, cnt = np.full((50, 2), -7, np.int32), np.full(1, -7, np.int32)
        status = rc.raw_refill_call(ctx, fn, b["slot"], b["roi"], b["mc"], b["params"], b["xy"], b["prio"], b["n"], b["radius"], b["base"], b["stride"], keep, out, b["cap"], cnt)
        assert status == code, f"{what}: status {status}"
        assert (keep is None or (keep == 9).all()) and (out == -7).all() and (cnt == -7).all(), f"{what}: an output was written"
        if what == "right of the frame":
            msg = ctx.lib.pmv_last_error(ctx.h).decode()
            assert f"({W}, 5)" in msg and f"{W}x{H}" in msg, msg
    keep, corners = ctx.detect_gftt_refill(0, 50, good, 5, min_dist=7.0)
    assert keep.tolist() == [1, 1, 1, 1] and len(corners) == 50, "a good call after the refusals"


def test_a_second_call_never_sees_the_first_calls_mask(pmv, gpu_ctx_factory):
    ctx = _ctx(pmv, gpu_ctx_factory)
    img = gf.rect_frame(pmv, W, H)
    xy, prio = rc.tracks(W, H, 300)
    _check(pmv, ctx, 0, img, xy, 255, prio, what="radius 255 first", min_dist=10.0)
    keep, _ = _check(pmv, ctx, 0, img, xy, 0, prio, what="then radius 0", min_dist=10.0)
    assert int((ctx.debug_refill_mask() == 0).sum()) == int(keep.sum())
    _check(pmv, ctx, 0, img, xy, 30, prio, base=rc.base_mask(W, H), what="a base mask", min_dist=10.0)
    _check(pmv, ctx, 0, img, xy[:5], 2, None, what="then none", min_dist=10.0)
