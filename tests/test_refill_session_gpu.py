"""pmv_batch_detect_gftt_refill: refill requests from the threads of one session return the bytes of the single call, the refill requests
of a round share ONE select + paint launch pair, and a round that mixes them with plain frame requests serves each its own. One 768x512
context of its own: slots 0 and 2 hold 517x261 frames, slot 1 a 768x512 one.

As in tests/test_gftt_frame_session_gpu.py the rounds that must be full are made to form: the engine of this module's context is made with
PMV_BATCH_LINGER_US = 50 ms, and the threads of a case start together behind a barrier."""
import os
import threading

import numpy as np
import pytest

import gftt_common as gc
import gftt_frame_common as gf
import refill_common as rc

pytestmark = pytest.mark.gpu

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
    return [gf.rect_frame(pmv, gf.W1, gf.H1), gf.rect_frame(pmv, gf.W2, gf.H2), gf.plateau_frame(gf.W1, gf.H1)]


def _ctx(pmv, gpu_ctx_factory):
    if "ctx" not in _state:
        ctx = gpu_ctx_factory(gf.W2, gf.H2, n_slots=3, max_tracks=2048)
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


def _same(got, want, what):
    assert np.array_equal(got[0], want[0]), f"{what}: keep bytes differ"
    assert np.array_equal(got[1], want[1]), f"{what}: corners differ"


def test_a_session_without_refill_requests_leaves_the_counters_at_zero(pmv, gpu_ctx_factory):
    """(the first test of the module: no refill request has been made on this context)"""
    ctx = _ctx(pmv, gpu_ctx_factory)
    mask = gc.masks(gf.W1, gf.H1)["discs"]
    want = [ctx.detect_gftt_frame(0, 150, min_dist=30.0), ctx.detect_gftt_frame(0, 150, min_dist=30.0, mask=mask)]
    before = ctx.debug_gftt_frame_stats()
    with ctx.batch_session(2, SIZES):
        got = _threads(2, lambda j: ctx.batch_detect_gftt_frame(0, 150, min_dist=30.0, mask=mask if j else None))
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert ctx.debug_refill_stats() == [0, 0, 0, 0]
    assert [a - b for a, b in zip(ctx.debug_gftt_frame_stats()[:3], before[:3])] == [0, 1, 2]


def test_four_threads_with_their_own_n_radius_and_region(pmv, gpu_ctx_factory):
    ctx = _ctx(pmv, gpu_ctx_factory)
    xy1, prio1 = rc.tracks(gf.W1, gf.H1, 1025)
    xy2, prio2 = rc.tracks(gf.W2, gf.H2, 300)
    base = rc.base_mask(gf.W1, gf.H1)
    # (slot, tracks, priorities, radius, base mask, region): an odd-sized region, a base mask, another frame size, no tracks
    args = [(0, xy1[:300], prio1[:300], 30, None, (13, 7, 301, 199)), (2, xy1, prio1, 1, base, None), (1, xy2, None, 7, None, None),
            (0, xy1[:0], None, 10, None, (0, 0, 255, 131))]
    kw = dict(quality=0.01, min_dist=10.0)
    call = lambda f, a: f(a[0], 150, a[1], a[3], priorities=a[2], base_mask=a[4], roi=a[5], **kw)   # noqa: E731
    want = [call(ctx.detect_gftt_refill, a) for a in args]
    for a, w in zip(args, want):   # (the single call itself is held to the twin in tests/test_refill_gpu.py; here its keep bytes once more)
        img = _images(pmv)[a[0]]
        assert np.array_equal(w[0], rc.twin().mask(img.shape[1], img.shape[0], a[1], a[3], a[2], a[4])[0])
    before, fbefore = ctx.debug_refill_stats(), ctx.debug_gftt_frame_stats()
    with ctx.batch_session(4, SIZES):
        got = _threads(4, lambda j: call(ctx.batch_detect_gftt_refill, args[j]))
    for j in range(4):
        _same(got[j], want[j], f"thread {j}")
    after = ctx.debug_refill_stats()
    rounds, pairs = after[1] - before[1], after[2] - before[2]
    assert after[0] == before[0] and 1 <= rounds <= 4 and pairs <= rounds, "at most one select + paint pair per round that held a refill request"
    assert rounds == 1, "four requests that start together share the lingering round"
    assert after[3] - before[3] == gf.W1 * gf.H1, "only the base mask's region crossed the bus"
    fd = [a - b for a, b in zip(ctx.debug_gftt_frame_stats()[:3], fbefore[:3])]
    assert fd == [0, 1, 2], "one round; one launch pair per frame layout (the refill requests all count as masked)"


def test_a_round_mixes_refill_requests_with_plain_frame_requests(pmv, gpu_ctx_factory):
    ctx = _ctx(pmv, gpu_ctx_factory)
    xy, prio = rc.tracks(gf.W1, gf.H1, 300)
    mask = gc.masks(gf.W1, gf.H1)["roi"]
    kw = dict(quality=0.01, min_dist=10.0)
    want_refill = [ctx.detect_gftt_refill(0, 150, xy, 30, priorities=prio, **kw), ctx.detect_gftt_refill(2, 150, xy[:65], 7, roi=(5, 5, 99, 77), **kw)]
    want_masked, want_plain = ctx.detect_gftt_frame(0, 150, mask=mask, **kw), ctx.detect_gftt_frame(2, 150, **kw)
    calls = [lambda: ctx.batch_detect_gftt_refill(0, 150, xy, 30, priorities=prio, **kw), lambda: ctx.batch_detect_gftt_frame(0, 150, mask=mask, **kw),
             lambda: ctx.batch_detect_gftt_refill(2, 150, xy[:65], 7, roi=(5, 5, 99, 77), **kw), lambda: ctx.batch_detect_gftt_frame(2, 150, **kw)]
    before, fbefore = ctx.debug_refill_stats(), ctx.debug_gftt_frame_stats()
    with ctx.batch_session(4, SIZES):
        got = _threads(4, lambda j: calls[j]())
    _same(got[0], want_refill[0], "refill on slot 0")
    _same(got[2], want_refill[1], "refill on slot 2")
    assert np.array_equal(got[1], want_masked), "the masked frame request that shares the refill requests' group"
    assert np.array_equal(got[3], want_plain), "the unmasked frame request"
    after = ctx.debug_refill_stats()
    assert [a - b for a, b in zip(after, before)] == [0, 1, 1, 0]
    fd = [a - b for a, b in zip(ctx.debug_gftt_frame_stats()[:3], fbefore[:3])]
    assert fd == [0, 1, 2], "pmv_debug_gftt_frame_stats counts what it counted: one round, a masked group (three requests) and an unmasked one"


def test_session_refusals_write_nothing(pmv, gpu_ctx_factory):
    ctx = _ctx(pmv, gpu_ctx_factory)
    P = pmv.GfttParams(0.01, 7.0, 3, 0, 0.04)
    good = np.asarray([(10, 10), (100, 50), (300, 200), (500, 250)], np.float32)
    want = ctx.detect_gftt_refill(0, 50, good, 5, min_dist=7.0)
    fn = ctx.lib.pmv_batch_detect_gftt_refill
    with ctx.batch_session(1, SIZES):
        for what, code, a in (("radius", rc.INVALID, dict(radius=256)), ("outside", rc.INVALID, dict(xy=np.asarray([(10, 10), (517, 5), (1, 1), (2, 2)], np.float32))),
                              ("n", rc.CAPACITY, dict(n=-1)), ("slot", rc.CAPACITY, dict(slot=9)), ("region", rc.INVALID, dict(roi=(300, 0, 218, 100))),
                              ("overflow", rc.OVERFLOW, dict(mc=0, cap=20))):
            b = dict(slot=0, roi=None, mc=50, xy=good, n=4, radius=5, cap=50)
            b.update(a)
            keep, out, cnt = np.full(8, 9, np.uint8), np.full((50, 2), -7, np.int32), np.full(1, -7, np.int32)
            status = rc.raw_refill_call(ctx, fn, b["slot"], b["roi"], b["mc"], P, b["xy"], None, b["n"], b["radius"], None, 0, keep, out, b["cap"], cnt)
            assert status == code, f"{what}: status {status}"
            assert (keep == 9).all() and (out == -7).all() and (cnt == -7).all(), f"{what}: an output was written"
            _same(ctx.batch_detect_gftt_refill(0, 50, good, 5, min_dist=7.0), want, f"a good call after {what}")
