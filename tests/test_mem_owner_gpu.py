"""Every device and pinned buffer has one owner that frees it: pmv_debug_mem_live, the library's own count of the bytes it holds, is above
its starting value while a context is open and back at EXACTLY that value after close() - after every lazily made block and every owner
(context, back-end workspaces, combiners, session, feeder) has been touched once, for a second context in the same process, and after the
batch engine was destroyed and rebuilt for a larger batch. The count is the library's, so other users of the card do not move it. The
contexts are this test's own (not the session-scoped factory's): it must close them itself."""
import gc

import numpy as np
import pytest

import scenes

pytestmark = pytest.mark.gpu

BIG, SMALL = (96, 64), (64, 48)   # (w, h); 96x64 is the context's capacity


def _ctx(pmv):
    return pmv.Context(96, 64, n_slots=4, max_tracks=64, max_ba_cams=4, max_ba_points=32, max_ba_obs=64)


def _frame(rng, wh, bgr=False):
    w, h = wh
    return rng.integers(0, 256, (h, w, 3) if bgr else (h, w), dtype=np.uint8)


def _identity_map(wh):
    w, h = wh
    mx, my = np.meshgrid(np.arange(w, dtype=np.float32) + 0.25, np.arange(h, dtype=np.float32) + 0.25)
    return mx, my


def _exercise(pmv, ctx):
    """every lazily made block and every owner once"""
    rng = np.random.default_rng(5)
    big, small = _frame(rng, BIG), _frame(rng, SMALL)
    cells = np.array([[0, 0, 96, 64]], np.int32)
    mask = np.full((64, 96), 255, np.uint8)
    mask[:, :8] = 0
    pts = np.stack([rng.uniform(20, 76, 24), rng.uniform(16, 48, 24)], 1).astype(np.float32)
    ipts = pts.astype(np.int32)
    # uploads: the landing area, the staged form, the feeder of a bracket
    ctx.frame_upload(0, big)
    ctx.frame_upload_bgr(1, _frame(rng, BIG, bgr=True))
    ctx.frames_stage(2, np.stack([small, small]))
    ctx.frames_build(2, 2)
    ctx.frames_stream_begin(2, np.stack([big, big]))
    ctx.lk_track(2, 3, pts)
    ctx.frames_stream_end()
    # CLAHE and remap blocks; the map stays: the context frees it
    ctx.frames_clahe(2, 2, 40.0, (4, 4))
    ctx.frames_remap(2, 2, ctx.remap_map_create(*_identity_map(BIG)))
    # detectors (the mask block), matcher, sub-pixel block
    ctx.detect_gftt(0, cells, 16)
    ctx.detect_gftt_ex(0, cells, 16, mask=mask, block_size=5)
    ctx.detect_shitomasi(0, cells, 16)
    ctx.detect_fast(0, cells, 16)
    ctx.knn_match(0, 1, ipts, ipts)
    ctx.corner_subpix(0, pts)
    # LK and the extended block
    ctx.lk_track(0, 1, pts)
    ctx.lk_track_fb(0, 1, pts)
    # a deeper pyramid: at 96x64 one level becomes four, the slot storage grows
    ctx.set_lk_params(win=5, max_level=4)
    ctx.frame_upload(0, big)
    assert ctx.num_levels(0) == 3
    # back-end workspaces
    P = scenes.pnp_problem(3, m=48, outlier_frac=0.0)
    ctx.pnp_ransac(P["obj"], P["img"], scenes.K, np.zeros(3), np.zeros(3))
    Q = scenes.ba_problem(4, nc=3, npts=10, vis=1.0, outlier_every=0)
    ctx.ba_solve(Q["cams"], Q["pts"], Q["obs"], Q["cam_idx"], Q["pt_idx"], scenes.K, 1.0, 2)
    # the engine, a session and its two scratches: a smaller round first, then a larger one, so both grow
    ids = {SMALL: ctx.remap_map_create(*_identity_map(SMALL)), BIG: ctx.remap_map_create(*_identity_map(BIG))}
    ctx.batch_open(2, [BIG, SMALL])
    for wh, tiles in ((SMALL, (2, 2)), (BIG, (4, 4))):
        ctx.batch_frame_upload(0, _frame(rng, wh), clahe=(40.0, tiles))
        ctx.batch_frame_upload_remap(1, _frame(rng, wh), ids[wh], clahe=(40.0, tiles))
    ctx.batch_lk_track_fb(0, 1, pts)
    ctx.batch_detect_gftt_ex(0, cells, 16, mask=mask, block_size=5)
    ctx.batch_corner_subpix(0, pts)
    ctx.batch_close()


def _above(live, start):
    return live[0] > start[0] and live[1] > start[1]


def test_every_buffer_goes_with_its_owner(pmv):
    gc.collect()   # (a context some earlier test dropped without close() must not go in the middle of this one)
    start = pmv.mem_live()
    for turn in ("first", "second"):   # the second context: statics, and the engine made again
        ctx = _ctx(pmv)
        try:
            created = pmv.mem_live()
            assert _above(created, start), f"{turn} context: {created} after create, {start} before"
            _exercise(pmv, ctx)
            used = pmv.mem_live()
            assert used[0] > created[0] and used[1] > created[1], f"{turn} context: the lazy blocks added nothing: {created} -> {used}"
        finally:
            ctx.close()
        assert pmv.mem_live() == start, f"{turn} context: {pmv.mem_live()} after close(), {start} before it was made"


def test_engine_rebuilt_for_a_larger_batch(pmv):
    gc.collect()
    start = pmv.mem_live()
    ctx = _ctx(pmv)
    try:
        ctx.batch_open(1, [BIG])
        ctx.batch_close()
        one = pmv.mem_live()
        ctx.batch_open(3, [BIG])   # more sequences than the engine has: it is destroyed and built again
        ctx.batch_close()
        three = pmv.mem_live()
        assert _above(one, start) and three[0] > one[0] and three[1] > one[1], f"{start} -> {one} -> {three}"
    finally:
        ctx.close()
    assert pmv.mem_live() == start, f"{pmv.mem_live()} after close(), {start} before the context was made"
