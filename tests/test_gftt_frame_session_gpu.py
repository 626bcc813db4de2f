"""pmv_batch_detect_gftt_frame: frame requests from six threads of one session return the twin's bytes (tests/twin/gftt_twin.cpp, the
region as its cell), requests that agree share one round with one launch pair, and a round that mixes them with cell and sub-pixel
requests serves each its own. One 768x512 context of its own: slots 0, 2 hold 517x261 frames, slots 1, 3 hold 768x512 ones.

As in tests/test_capacity_edge_gpu.py the rounds that must be full are made to form: the engine of this module's context is made with
PMV_BATCH_LINGER_US = 50 ms, and the threads of a case start together behind a barrier."""
import os
import threading

import numpy as np
import pytest

import gftt_common as gc
import gftt_frame_common as gf

pytestmark = pytest.mark.gpu

N = 6
SIZES = [(gf.W1, gf.H1), (gf.W2, gf.H2)]
_state = {}


@pytest.fixture(scope="module", autouse=True)
def _lingering_rounds():
    """read by the engine when it is made (the first batch_open of this module's context)"""
    old = os.environ.get("PMV_BATCH_LINGER_US")
    os.environ["PMV_BATCH_LINGER_US"] = "50000"
    yield
    if old is None:
        del os.environ["PMV_BATCH_LINGER_US"]
    else:
        os.environ["PMV_BATCH_LINGER_US"] = old


def _images(pmv):
    return [gf.rect_frame(pmv, gf.W1, gf.H1), gf.rect_frame(pmv, gf.W2, gf.H2), gf.plateau_frame(gf.W1, gf.H1), gf.noise(gf.W2, gf.H2)]


def _ctx(pmv, gpu_ctx_factory):
    if "ctx" not in _state:
        ctx = gpu_ctx_factory(gf.W2, gf.H2, n_slots=4, max_tracks=256)
        for slot, img in enumerate(_images(pmv)):
            ctx.frame_upload(slot, img)
        _state["ctx"] = ctx
    return _state["ctx"]


def _threads(n, fn):
    res, errors = [None] * n, []
    start = threading.Barrier(n)

    def run(j):
        try:
            start.wait()
            res[j] = fn(j)
        except Exception as e:   # noqa: BLE001 - reported by the main thread
            errors.append((j, repr(e)))
    th = [threading.Thread(target=run, args=(j,)) for j in range(n)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors, errors
    return res


def _delta(ctx, before):
    return [a - b for a, b in zip(ctx.debug_gftt_frame_stats()[:3], before[:3])]


def test_a_session_without_frame_requests_launches_what_it_did(pmv, gpu_ctx_factory):
    """(the first test of the module: no frame request has been made on this context)"""
    ctx = _ctx(pmv, gpu_ctx_factory)
    cells = pmv.grid_cells(gf.W1, gf.H1)
    want = ctx.detect_gftt_ex(0, cells, 20, block_size=5)
    with ctx.batch_session(2, SIZES):
        got = _threads(2, lambda j: ctx.batch_detect_gftt_ex(0, cells, 20, block_size=5))
    assert all(np.array_equal(a, b) for g in got for a, b in zip(g, want))
    assert ctx.debug_gftt_frame_stats()[:5] == [0, 0, 0, 0, 0]


def test_six_threads_share_one_round_and_one_launch_pair(pmv, gpu_ctx_factory):
    """requests that agree in every argument, on the two slots of one frame size, with regions of their own"""
    ctx = _ctx(pmv, gpu_ctx_factory)
    imgs = _images(pmv)
    rois = [None, (37, 11, 301, 200), (0, 0, 300, 140), None, (gf.W1 - 300, gf.H1 - 140, 300, 140), (411, 0, 5, 261)]
    slots = [0, 0, 0, 2, 2, 2]
    kw = dict(quality=0.01, min_dist=7.0, block_size=5)
    want = [gf.twin_region(imgs[s], gf.whole(imgs[s]) if r is None else np.asarray(r, np.int32), 500, **kw)[0] for s, r in zip(slots, rois)]
    before = ctx.debug_gftt_frame_stats()
    with ctx.batch_session(N, SIZES):
        got = _threads(N, lambda j: ctx.batch_detect_gftt_frame(slots[j], 500, roi=rois[j], **kw))
    for j in range(N):
        assert np.array_equal(got[j], want[j]), f"thread {j}"
    assert sum(len(w) for w in want) > 300
    assert _delta(ctx, before) == [0, 1, 1], "six agreeing requests: one round, one pass-1 and one pass-2 launch"


def test_two_frame_sizes_and_masks_in_one_round(pmv, gpu_ctx_factory):
    """slots of both declared sizes, half of the requests with a mask: one round, one launch pair per (layout, has-mask) group"""
    ctx = _ctx(pmv, gpu_ctx_factory)
    imgs = _images(pmv)
    slots = [0, 1, 2, 3, 0, 1]
    masks = [None, None, None, None, gc.masks(gf.W1, gf.H1)["roi"], gc.masks(gf.W2, gf.H2)["discs"]]
    kw = dict(quality=0.01, min_dist=10.0)
    want = [gf.twin_region(imgs[s], gf.whole(imgs[s]), 0, mask=m, **kw)[0] for s, m in zip(slots, masks)]
    before = ctx.debug_gftt_frame_stats()
    with ctx.batch_session(N, SIZES):
        got = _threads(N, lambda j: ctx.batch_detect_gftt_frame(slots[j], 0, mask=masks[j], **kw))
    for j in range(N):
        assert np.array_equal(got[j], want[j]), f"thread {j}"
    assert _delta(ctx, before) == [0, 1, 4]


def test_a_round_mixes_frame_cell_and_subpix_requests(pmv, gpu_ctx_factory):
    ctx = _ctx(pmv, gpu_ctx_factory)
    imgs = _images(pmv)
    cells = pmv.grid_cells(gf.W1, gf.H1)
    kw = dict(quality=0.01, min_dist=30.0)
    want_frame = [gf.twin_region(imgs[s], gf.whole(imgs[s]), 150, **kw)[0] for s in (0, 1)]
    want_cells = ctx.detect_gftt_ex(0, cells, 20, block_size=5)
    pts = (want_frame[0][:64] + 0.25).astype(np.float32)
    want_spx = ctx.corner_subpix(0, pts)
    calls = [lambda: ctx.batch_detect_gftt_frame(0, 150, **kw), lambda: ctx.batch_detect_gftt_frame(1, 150, **kw),
             lambda: ctx.batch_detect_gftt_ex(0, cells, 20, block_size=5), lambda: ctx.batch_detect_gftt_ex(0, cells, 20, block_size=5),
             lambda: ctx.batch_corner_subpix(0, pts), lambda: ctx.batch_corner_subpix(0, pts)]
    before = ctx.debug_gftt_frame_stats()
    with ctx.batch_session(N, SIZES):
        got = _threads(N, lambda j: calls[j]())
    assert np.array_equal(got[0], want_frame[0]) and np.array_equal(got[1], want_frame[1])
    for g in got[2:4]:
        assert all(np.array_equal(a, b) for a, b in zip(g, want_cells))
    for g in got[4:]:
        assert np.array_equal(g.view(np.uint32), want_spx.view(np.uint32))
    assert _delta(ctx, before) == [0, 1, 2]


def test_session_refusals_and_overflow(pmv, gpu_ctx_factory):
    """the session form refuses what the single call refuses, with its codes, and an overflowing no-limit request fails alone"""
    ctx = _ctx(pmv, gpu_ctx_factory)
    imgs = _images(pmv)
    want, _ = gf.twin_region(imgs[0], gf.whole(imgs[0]), 50, quality=0.01, min_dist=7.0)
    P = pmv.GfttParams(0.01, 7.0, 3, 0, 0.04)
    fn = ctx.lib.pmv_batch_detect_gftt_frame
    with ctx.batch_session(1, SIZES):
        for what, code, a in (("region", gf.INVALID, dict(roi=(300, 0, 218, 100))), ("block", gf.INVALID, dict(params=pmv.GfttParams(0.01, 7.0, 16, 0, 0.04))),
                              ("cap", gf.CAPACITY, dict(mc=51)), ("slot", gf.CAPACITY, dict(slot=9)), ("overflow", gf.OVERFLOW, dict(mc=0, cap=20))):
            b = dict(slot=0, roi=None, mc=50, params=P, cap=50)
            b.update(a)
            xy, cnt = np.full((50, 2), -7, np.int32), np.full(1, -7, np.int32)
            rc = gf.raw_frame_call(ctx, fn, b["slot"], b["roi"], b["mc"], b["params"], None, 0, xy, b["cap"], cnt)
            assert rc == code, f"{what}: status {rc}"
            assert (xy == -7).all() and (cnt == -7).all(), f"{what}: an output was written"
            assert np.array_equal(ctx.batch_detect_gftt_frame(0, 50, min_dist=7.0), want)
