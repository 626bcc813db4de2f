"""pmv_frames_clahe and pmv_batch_frame_upload_clahe on the device: after the call a slot holds, at EVERY level with its border, the bytes
that pmv_frame_upload of the CPU twin's output (tests/twin/clahe_twin.cpp) leaves in another slot - from staged and from built slots, over
ranges of mixed sizes, across the LUT scratch's chunk, from colour uploads and through the session's upload rounds. Every comparison is
byte-exact. The cases and their images come from clahe_common; the statistics of the twin assert that each case reaches its branch."""
import ctypes as C
import threading

import numpy as np
import pytest

import clahe_common as cc

pytestmark = pytest.mark.gpu

CAP_W, CAP_H = 203, 120       # the largest width and height of the table
INVALID, CAPACITY = -2, -3    # PMV_ERR_INVALID, PMV_ERR_CAPACITY
CHUNK = 64                    # frames per pair of launches of pmv_frames_clahe (pmv_ctx::CLAHE_CHUNK)
REF = 7                       # the slot the twin's images are uploaded into

_cache = {}


def _ctx(gpu_ctx_factory):
    if "ctx" not in _cache:
        _cache["ctx"] = gpu_ctx_factory(CAP_W, CAP_H, n_slots=8, max_tracks=1024)
    return _cache["ctx"]


def _levels(ctx, slot):
    return [ctx.get_level_padded(slot, l, CAP_W, CAP_H) for l in range(ctx.num_levels(slot) + 1)]


def _same_levels(got, want, what):
    assert len(got) == len(want) >= 1, f"{what}: {len(got)} levels, expected {len(want)}"
    for l, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape and np.array_equal(a, b), f"{what}: level {l} differs in {int((a != b).sum())} bytes"


def _want(pmv, ctx, case):
    """every padded level of the twin's image through pmv_frame_upload, computed once per case"""
    key = ("want", case)
    if key not in _cache:
        ctx.frame_upload(REF, cc.equalised(pmv, case)[0])
        _cache[key] = _levels(ctx, REF)
    return _cache[key]


def _code(fn):
    with pytest.raises(Exception) as e:
        fn()
    return getattr(e.value, "code", None), str(e.value)


@pytest.mark.parametrize("case", cc.CASES, ids=cc.case_id)
def test_slot_contents_equal_the_twin(pmv, gpu_ctx_factory, case):
    """from a staged slot (no border, no upper levels yet) and from an uploaded one (whose border and upper levels are the plain image's)"""
    w, h, clip, tiles = case
    ctx = _ctx(gpu_ctx_factory)
    img = cc.image(pmv, w, h)
    stats = cc.equalised(pmv, case)[1]
    if clip in cc.CLIPPING:
        assert stats["clipped"] >= 1 and stats["residual"] >= 1, stats
    want = _want(pmv, ctx, case)
    assert want[0].shape == (h + 128, w + 128) and not np.array_equal(want[0][64:64 + h, 64:64 + w], img)
    before = ctx.debug_clahe_launches()
    ctx.frames_stage(0, img[None])
    ctx.frames_clahe(0, 1, clip, tiles)
    _same_levels(_levels(ctx, 0), want, "from a staged slot")
    ctx.frame_upload(1, img)
    ctx.frames_clahe(1, 1, clip, tiles)
    _same_levels(_levels(ctx, 1), want, "from an uploaded slot")
    after = ctx.debug_clahe_launches()
    assert after[0] - before[0] == 2 and after[1:] == before[1:]
    # a second call equalises again, as cv would
    ctx.frames_clahe(1, 1, clip, tiles)
    ctx.frame_upload(2, cc.twin().apply(cc.equalised(pmv, case)[0], clip, tiles)[0])
    _same_levels(_levels(ctx, 1), _levels(ctx, 2), "applied twice")


def test_the_table_reaches_both_redistribution_steps(pmv):
    steps = set().union(*(cc.equalised(pmv, c)[1]["steps"] for c in cc.CASES))
    assert 1 in steps and any(s > 1 for s in steps), steps


def test_one_call_over_a_range_of_mixed_sizes(pmv, gpu_ctx_factory):
    """four slots of three sizes, staged and built ones mixed: one call (one pair of launches) equals the per-slot results"""
    ctx = _ctx(gpu_ctx_factory)
    cases = [(160, 120, 2.0, (8, 8)), (203, 87, 2.0, (8, 8)), (203, 87, 2.0, (8, 8)), (41, 40, 2.0, (8, 8))]
    wants = [_want(pmv, ctx, c) for c in cases]
    for slot, (w, h, _, _) in enumerate(cases):
        if slot % 2:
            ctx.frames_stage(slot, cc.image(pmv, w, h)[None])
        else:
            ctx.frame_upload(slot, cc.image(pmv, w, h))
    before = ctx.debug_clahe_launches()[0]
    ctx.frames_clahe(0, 4, 2.0, (8, 8))
    assert ctx.debug_clahe_launches()[0] - before == 1
    for slot, want in enumerate(wants):
        _same_levels(_levels(ctx, slot), want, f"slot {slot} of the range")


def test_a_range_longer_than_the_lut_scratch_chunk(pmv, gpu_ctx_factory):
    """70 small frames of two sizes (the chunk's end falls inside the second size) in one call: the bytes of slot-by-slot calls, and of the twin"""
    n = CHUNK + 6
    ctx = gpu_ctx_factory(48, 48, n_slots=2 * n, max_tracks=64)
    noise = cc.gc.noise_frame()
    a = np.stack([noise[3 * k:3 * k + 40, 5 * k:5 * k + 41] for k in range(40)])               # 41x40
    b = np.stack([noise[2 * k:2 * k + 41, 100 + 3 * k:100 + 3 * k + 40] for k in range(n - 40)])   # 40x41
    for first in (0, n):
        ctx.frames_stage(first, a)
        ctx.frames_stage(first + 40, b)
    before = ctx.debug_clahe_launches()[0]
    ctx.frames_clahe(0, n, 2.0, (8, 8))
    assert ctx.debug_clahe_launches()[0] - before == 2          # 64 + 6 frames
    for k in range(n):
        ctx.frames_clahe(n + k, 1, 2.0, (8, 8))
    assert ctx.debug_clahe_launches()[0] - before == 2 + n
    for k in range(n):
        _same_levels([ctx.get_level_padded(k, 0, 48, 48)], [ctx.get_level_padded(n + k, 0, 48, 48)], f"slot {k}")
        assert ctx.num_levels(k) == 0
    for k, img in ((0, a[0]), (39, a[39]), (40, b[0]), (CHUNK - 1, b[CHUNK - 41]), (CHUNK, b[CHUNK - 40]), (n - 1, b[-1])):
        got = ctx.get_level(k, 0, 48, 48)
        assert np.array_equal(got, cc.twin().apply(img, 2.0, (8, 8))[0]), f"slot {k} against the twin"


def test_after_a_colour_upload(pmv, gpu_ctx_factory):
    """pmv_frame_upload_bgr, then the equalisation: the twin on the gray image that the gray path holds"""
    ctx = _ctx(gpu_ctx_factory)
    g = cc.image(pmv, 203, 87)
    bgr = np.ascontiguousarray(np.stack([g, np.roll(g, 3, axis=1), np.roll(g, 2, axis=0)], axis=2))
    ctx.frame_upload_bgr(0, bgr)
    gray = ctx.get_level(0, 0, CAP_W, CAP_H)
    assert gray.shape == g.shape and not np.array_equal(gray, g)
    ctx.frames_clahe(0, 1, 3.0, (4, 3))
    ctx.frame_upload(REF, cc.twin().apply(gray, 3.0, (4, 3))[0])
    _same_levels(_levels(ctx, 0), _levels(ctx, REF), "after a colour upload")


def _roi(img):
    h, w = img.shape[:2]
    big = np.random.default_rng(w * 31 + h).integers(0, 256, (h + 4, w + 7) + img.shape[2:], dtype=np.uint8)
    big[2:2 + h, 3:3 + w] = img
    return big


SESSION_SIZES = [(160, 120), (203, 87), (75, 53)]


def test_session_uploads_from_every_kind_of_source(pmv, gpu_ctx_factory):
    """pageable, an ROI view of a larger pageable image, the same view in pinned memory (read in place): the bytes of the single calls. One
    upload at a time, so every round holds one request: it makes its level-0 launch, one launch pair, the in-place level-0 launch"""
    import torch
    ctx = _ctx(gpu_ctx_factory)
    before = ctx.debug_clahe_launches()
    n = 0
    with ctx.batch_session(2, SESSION_SIZES):
        for case in ((160, 120, 2.0, (8, 8)), (203, 87, 3.0, (4, 3)), (75, 53, 0.5, (16, 16))):
            w, h, clip, tiles = case
            want = _want(pmv, ctx, case)
            big = _roi(cc.image(pmv, w, h))
            pinned = torch.empty(big.shape, dtype=torch.uint8).pin_memory()
            pinned.numpy()[...] = big
            sources = {"tight pageable": cc.image(pmv, w, h), "ROI view": big[2:2 + h, 3:3 + w], "pinned ROI view": pinned[2:2 + h, 3:3 + w]}
            for slot, (name, src) in enumerate(sources.items()):
                ctx.batch_frame_upload(slot, src, "gray", clahe=(clip, tiles))
                _same_levels(_levels(ctx, slot), want, f"{cc.case_id(case)} from a {name}")
                n += 1
        # the colour form: the bytes of pmv_frame_upload_bgr followed by pmv_frames_clahe
        g = cc.image(pmv, 203, 87)
        bgr = np.ascontiguousarray(np.stack([g, np.roll(g, 3, axis=1), np.roll(g, 2, axis=0)], axis=2))
        ctx.batch_frame_upload(3, _roi(bgr)[2:2 + 87, 3:3 + 203], "bgr", clahe=(3.0, (4, 3)))
        n += 1
        st = ctx.batch_upload_stats()
        rounds = ctx.batch_upload_rounds()
    ctx.frame_upload_bgr(4, bgr)
    ctx.frames_clahe(4, 1, 3.0, (4, 3))
    _same_levels(_levels(ctx, 3), _levels(ctx, 4), "colour session upload")
    after = ctx.debug_clahe_launches()
    assert after[1] - before[1] == n and after[2] - before[2] == n and after[0] - before[0] == 1
    assert st["rounds"] == st["frames"] == n == len(rounds) and st["level0_launches"] == 2 * n
    assert all(r["level0_launches"] == 2 for r in rounds)
    assert [r["in_place"] for r in rounds] == [0, 0, 1] * 3 + [0]


def test_session_threads_mix_clahe_and_plain_uploads(pmv, gpu_ctx_factory):
    """three threads released together: two CLAHE requests of different sizes and parameters and a plain upload. The right bytes in all
    three slots, and one launch pair per round that held a request, however the requests met"""
    ctx = _ctx(gpu_ctx_factory)
    jobs = [(0, (160, 120, 2.0, (8, 8))), (1, (75, 53, 0.5, (16, 16))), (2, None)]
    wants = [_want(pmv, ctx, case) for _, case in jobs[:2]]
    plain = cc.image(pmv, 203, 87)
    ctx.frame_upload(REF, plain)
    wants.append(_levels(ctx, REF))
    before = ctx.debug_clahe_launches()
    errors = []
    with ctx.batch_session(3, SESSION_SIZES):
        start = threading.Barrier(len(jobs))

        def run(slot, case):
            try:
                start.wait()
                if case is None:
                    ctx.batch_frame_upload(slot, plain)
                else:
                    ctx.batch_frame_upload(slot, cc.image(pmv, case[0], case[1]), "gray", clahe=(case[2], case[3]))
            except Exception as e:   # noqa: BLE001 - reported by the main thread
                errors.append(e)
        ts = [threading.Thread(target=run, args=j) for j in jobs]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        assert not errors, errors
        st = ctx.batch_upload_stats()
        rounds = ctx.batch_upload_rounds()
    for slot, want in enumerate(wants):
        _same_levels(_levels(ctx, slot), want, f"slot {slot}")
    after = ctx.debug_clahe_launches()
    with_requests = after[1] - before[1]
    print(f"three uploads, two with CLAHE: {st}; rounds {rounds}; rounds with requests {with_requests}")
    assert st["frames"] == 3 and 1 <= with_requests <= 2 and with_requests <= st["rounds"]
    assert after[2] - before[2] == with_requests and after[0] == before[0]
    # a round with requests makes one level-0 launch more than its plain launches (gray frames only here: one)
    assert st["level0_launches"] == st["rounds"] + with_requests
    assert sorted(r["level0_launches"] for r in rounds).count(2) == with_requests


def test_a_session_of_plain_uploads_launches_what_it_always_did(pmv, gpu_ctx_factory):
    """a fresh context: after plain uploads only, the three counters are 0 and the rounds' records are those of the plain upload class"""
    ctx = gpu_ctx_factory(CAP_W, CAP_H, n_slots=3, max_tracks=64)
    with ctx.batch_session(1, SESSION_SIZES):
        for slot, (w, h) in enumerate(SESSION_SIZES):
            ctx.batch_frame_upload(slot, cc.image(pmv, w, h))
        st = ctx.batch_upload_stats()
        rounds = ctx.batch_upload_rounds()
    assert ctx.debug_clahe_launches() == [0, 0, 0]
    # 160x120 and 203x87 build levels 0-1 (the next would be 40x30 / 51x22: not above the 32-pixel window), 75x53 level 0 only
    assert rounds == [dict(frames_by_levels=[0, 1, 0, 0, 0], level0_launches=1, pyrdown_launches=1, in_place=0),
                      dict(frames_by_levels=[0, 1, 0, 0, 0], level0_launches=1, pyrdown_launches=1, in_place=0),
                      dict(frames_by_levels=[1, 0, 0, 0, 0], level0_launches=1, pyrdown_launches=0, in_place=0)], rounds
    assert st == dict(rounds=3, frames=3, level0_launches=3, pyrdown_launches=2)
    for slot, (w, h) in enumerate(SESSION_SIZES):
        assert np.array_equal(ctx.get_level(slot, 0, CAP_W, CAP_H), cc.image(pmv, w, h))


def test_detector_and_lk_downstream(pmv, gpu_ctx_factory):
    """pmv_detect_gftt and pmv_lk_track between two equalised slots return the bytes they return on slots uploaded from the twin's images"""
    ctx = _ctx(gpu_ctx_factory)
    w, h = 160, 120
    frames = cc.gc.cached(("clahe_pair", w, h), lambda: pmv.synth_sequence(1007, 10, 2, w, h, 0.58 * w, 0.58 * w, w / 2, h / 2)[0])
    ctx.frames_stage(0, frames)
    ctx.frames_clahe(0, 2)                                 # cv's defaults
    for k in range(2):
        ctx.frame_upload(2 + k, cc.twin().apply(frames[k], 40.0, (8, 8))[0])
    cells = pmv.grid_cells(w, h)
    got, want = ctx.detect_gftt(0, cells, 50), ctx.detect_gftt(2, cells, 50)
    assert len(got) == len(want) and all(np.array_equal(a, b) for a, b in zip(got, want))
    pts = np.concatenate([d + c[:2] for c, d in zip(cells, want[:len(cells)])]).astype(np.float32)
    assert len(pts) >= 20
    a, b = ctx.lk_track(0, 1, pts), ctx.lk_track(2, 3, pts)
    for x, y in zip(a, b):
        assert np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8))
    assert int((a[1] > 0).sum()) >= 1   # (not vacuous: tracks survive)


def test_errors_leave_the_slots_as_they_were(pmv, gpu_ctx_factory):
    ctx = gpu_ctx_factory(CAP_W, CAP_H, n_slots=4, max_tracks=64)
    img = cc.image(pmv, 160, 120)
    ctx.frame_upload(0, img)
    ctx.frame_upload(1, img)
    keep = _levels(ctx, 0)
    for kw, what in ((dict(tiles=(0, 8)), "tiles"), (dict(tiles=(8, 17)), "tiles"), (dict(clip_limit=-0.5), "clip_limit"), (dict(clip_limit=float("nan")), "clip_limit"),
                     (dict(clip_limit=float("inf")), "clip_limit")):
        code, msg = _code(lambda: ctx.frames_clahe(0, 2, **kw))
        assert code == INVALID and what in msg, (kw, code, msg)
    ctx.lib.pmv_frames_clahe.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(pmv.ClaheParams)]
    assert ctx.lib.pmv_frames_clahe(ctx.h, 0, 2, None) == INVALID
    assert ctx.lib.pmv_frames_clahe(None, 0, 2, C.byref(pmv.ClaheParams(2.0, 8, 8))) == INVALID
    for first, n in ((-1, 1), (3, 2), (4, 1), (0, 5), (0, 0), (1, 2 ** 31 - 1)):
        code, msg = _code(lambda: ctx.frames_clahe(first, n))
        assert code == CAPACITY, (first, n, code, msg)
    # slot 2 was never staged: the range is refused as a whole and the message names the slot
    code, msg = _code(lambda: ctx.frames_clahe(0, 3))
    assert code == INVALID and "slot 2" in msg, msg
    # while a stream bracket is open; once it is closed its slots are built and may be equalised
    frames = np.stack([img, img[::-1].copy()])
    ctx.frames_stream_begin(2, frames)
    try:
        code, msg = _code(lambda: ctx.frames_clahe(0, 1))
        assert code == INVALID and "pmv_frames_stream_begin" in msg, msg
    finally:
        ctx.frames_stream_end()
    assert ctx.debug_clahe_launches() == [0, 0, 0]
    for slot in (0, 1):
        _same_levels(_levels(ctx, slot), keep, f"slot {slot} after the refused calls")
    ctx.frames_clahe(2, 1, 2.0, (8, 8))
    _same_levels(_levels(ctx, 2), _want(pmv, _ctx(gpu_ctx_factory), cc.CASES[0]), "a slot of a finished bracket")
    # the session call: a null p and bad parameters are refused, the slot keeps its bytes
    with ctx.batch_session(1, [(160, 120)]):
        ctx.lib.pmv_batch_frame_upload_clahe.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(pmv.ClaheParams)]
        assert ctx.lib.pmv_batch_frame_upload_clahe(ctx.h, 0, C.c_void_p(img.ctypes.data), 160, 120, 160, 0, None) == INVALID
        for clahe in ((2.0, (17, 8)), (-1.0, (8, 8))):
            code, msg = _code(lambda: ctx.batch_frame_upload(0, img, "gray", clahe=clahe))
            assert code == INVALID, (clahe, code, msg)
        code, msg = _code(lambda: ctx.batch_frame_upload(0, cc.image(pmv, 203, 87), "gray", clahe=(2.0, (8, 8))))
        assert code == INVALID and "203x87" in msg, msg     # a size that was not declared, as for the plain call
        assert ctx.batch_upload_stats()["rounds"] == 0
    assert ctx.debug_clahe_launches() == [1, 0, 0]
    _same_levels(_levels(ctx, 0), keep, "slot 0 after the refused session calls")
