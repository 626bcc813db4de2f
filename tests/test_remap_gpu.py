"""pmv_frames_remap and pmv_batch_frame_upload_remap on the device: after the call a slot holds, at EVERY level with its border, the bytes
that pmv_frame_upload of the CPU twin's output (tests/twin/remap_twin.cpp) leaves in another slot - from staged and from built slots, across
the scratch's chunk, with maps of different sizes, from colour uploads, in front of the equalisation and through the session's upload
rounds. Every comparison is byte-exact. The cases, images and maps come from remap_common."""
import ctypes as C
import threading

import numpy as np
import pytest

import clahe_common as cc
import remap_common as rc

pytestmark = pytest.mark.gpu

CAP_W, CAP_H = 203, 120       # the largest width and height of the table
INVALID, CAPACITY = -2, -3    # PMV_ERR_INVALID, PMV_ERR_CAPACITY
CHUNK = 64                    # frames per k_remap launch of pmv_frames_remap (pmv_ctx::REMAP_CHUNK)
REF = 7                       # the slot the twin's images are uploaded into
UPLOAD_REMAP = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]

_cache = {}


def _ctx(gpu_ctx_factory):
    if "ctx" not in _cache:
        _cache["ctx"] = gpu_ctx_factory(CAP_W, CAP_H, n_slots=8, max_tracks=1024)
    return _cache["ctx"]


def _map(pmv, ctx, name, w, h):
    """the id of a map of the table on the shared context, created once (the table has 12 maps: within the 16 of a context)"""
    key = ("map", name, w, h)
    if key not in _cache:
        _cache[key] = ctx.remap_map_create(*rc.maps(pmv, name, w, h))
    return _cache[key]


def _levels(ctx, slot):
    return [ctx.get_level_padded(slot, l, CAP_W, CAP_H) for l in range(ctx.num_levels(slot) + 1)]


def _same_levels(got, want, what):
    assert len(got) == len(want) >= 1, f"{what}: {len(got)} levels, expected {len(want)}"
    for l, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape and np.array_equal(a, b), f"{what}: level {l} differs in {int((a != b).sum())} bytes"


def _upload_levels(ctx, img):
    ctx.frame_upload(REF, img)
    return _levels(ctx, REF)


def _want(pmv, ctx, case):
    """every padded level of the twin's image through pmv_frame_upload, computed once per case"""
    key = ("want", case)
    if key not in _cache:
        _cache[key] = _upload_levels(ctx, rc.remapped(pmv, case)[0])
    return _cache[key]


def _code(fn):
    with pytest.raises(Exception) as e:
        fn()
    return getattr(e.value, "code", None), str(e.value)


def _bgr(g):
    return np.ascontiguousarray(np.stack([g, np.roll(g, 3, axis=1), np.roll(g, 2, axis=0)], axis=2))


def _roi(img):
    h, w = img.shape[:2]
    big = np.random.default_rng(w * 31 + h).integers(0, 256, (h + 4, w + 7) + img.shape[2:], dtype=np.uint8)
    big[2:2 + h, 3:3 + w] = img
    return big


@pytest.mark.parametrize("case", rc.CASES, ids=rc.case_id)
def test_slot_contents_equal_the_twin(pmv, gpu_ctx_factory, case):
    """from a staged slot (no border, no upper levels yet) and from an uploaded one (whose border and upper levels are the plain image's)"""
    name, w, h, border = case
    ctx = _ctx(gpu_ctx_factory)
    img = rc.image(pmv, w, h)
    mid = _map(pmv, ctx, name, w, h)
    want = _want(pmv, ctx, case)
    assert want[0].shape == (h + 128, w + 128) and np.array_equal(want[0][64:64 + h, 64:64 + w], rc.remapped(pmv, case)[0])
    before = ctx.debug_remap_launches()
    ctx.frames_stage(0, img[None])
    ctx.frames_remap(0, 1, mid, border)
    _same_levels(_levels(ctx, 0), want, "from a staged slot")
    ctx.frame_upload(1, img)
    ctx.frames_remap(1, 1, mid, border)
    _same_levels(_levels(ctx, 1), want, "from an uploaded slot")
    after = ctx.debug_remap_launches()
    assert after[0] - before[0] == 2 and after[1:] == before[1:]
    # a second call remaps the remapped image
    ctx.frames_remap(1, 1, mid, border)
    again = rc.twin().apply(rc.remapped(pmv, case)[0], *rc.maps(pmv, name, w, h), border)[0]
    _same_levels(_levels(ctx, 1), _upload_levels(ctx, again), "applied twice")


def test_after_a_colour_upload(pmv, gpu_ctx_factory):
    """pmv_frame_upload_bgr, then the remap: the twin on the gray image that the colour path holds"""
    ctx = _ctx(gpu_ctx_factory)
    w, h = 203, 87
    bgr = _bgr(rc.image(pmv, w, h))
    ctx.frame_upload_bgr(0, bgr)
    gray = ctx.get_level(0, 0, CAP_W, CAP_H)
    assert gray.shape == (h, w) and not np.array_equal(gray, rc.image(pmv, w, h))
    ctx.frames_remap(0, 1, _map(pmv, ctx, "undistort06", w, h), 200)
    want = rc.twin().apply(gray, *rc.maps(pmv, "undistort06", w, h), 200)[0]
    _same_levels(_levels(ctx, 0), _upload_levels(ctx, want), "after a colour upload")


def test_a_range_longer_than_the_scratch_chunk(pmv, gpu_ctx_factory):
    """70 frames of 41x40 in one call: two k_remap launches (64 + 6 frames), every slot against the twin"""
    n = CHUNK + 6
    w, h = 41, 40
    ctx = gpu_ctx_factory(48, 48, n_slots=n + 1, max_tracks=64)
    noise = rc.gc.noise_frame()
    frames = np.stack([noise[3 * (k % 40):3 * (k % 40) + h, 2 * k:2 * k + w] for k in range(n)])
    mx, my = rc.maps(pmv, "undistort06", w, h)
    mid = ctx.remap_map_create(mx, my)
    ctx.frames_stage(0, frames)
    ctx.frames_remap(0, n, mid, 200)
    assert ctx.debug_remap_launches() == [2, 0, 0]
    for k in range(n):
        assert ctx.num_levels(k) == 0
        assert np.array_equal(ctx.get_level(k, 0, 48, 48), rc.twin().apply(frames[k], mx, my, 200)[0]), f"slot {k} against the twin"
    for k in (0, CHUNK - 1, CHUNK, n - 1):   # the border too, on both sides of the chunk's end
        ctx.frame_upload(n, rc.twin().apply(frames[k], mx, my, 200)[0])
        assert np.array_equal(ctx.get_level_padded(k, 0, 48, 48), ctx.get_level_padded(n, 0, 48, 48)), f"slot {k} with its border"


def test_two_maps_of_different_sizes_in_consecutive_calls(pmv, gpu_ctx_factory):
    """one context, one scratch: a 203x87 range, a 41x40 range, the 203x87 range again"""
    ctx = _ctx(gpu_ctx_factory)
    big, small = ("undistort06", 203, 87, 0), ("undistort", 41, 40, 0)
    wants = {c: _want(pmv, ctx, c) for c in (big, small)}
    for rounds in range(2):
        for case, slots in ((big, (0, 1)), (small, (2, 3, 4))):
            name, w, h, border = case
            ctx.frames_stage(slots[0], np.stack([rc.image(pmv, w, h)] * len(slots)))
            ctx.frames_remap(slots[0], len(slots), _map(pmv, ctx, name, w, h), border)
        for case, slots in ((big, (0, 1)), (small, (2, 3, 4))):
            for s in slots:
                _same_levels(_levels(ctx, s), wants[case], f"slot {s}, pass {rounds}")


def test_remap_then_clahe(pmv, gpu_ctx_factory):
    """pmv_frames_remap followed by pmv_frames_clahe: the twin of the one, then the twin of the other"""
    ctx = _ctx(gpu_ctx_factory)
    case = ("undistort06", 203, 87, 200)
    ctx.frames_stage(0, rc.image(pmv, 203, 87)[None])
    ctx.frames_remap(0, 1, _map(pmv, ctx, "undistort06", 203, 87), 200)
    ctx.frames_clahe(0, 1, 3.0, (4, 3))
    want = cc.twin().apply(rc.remapped(pmv, case)[0], 3.0, (4, 3))[0]
    _same_levels(_levels(ctx, 0), _upload_levels(ctx, want), "remap, then CLAHE")


SESSION_SIZES = [(160, 120), (203, 87), (41, 40)]


def test_session_uploads_from_every_kind_of_source(pmv, gpu_ctx_factory):
    """pageable, an ROI view of a larger pageable image, the same view in pinned memory and in device memory (both read in place). One upload
    at a time, so every round holds one request: its level-0 launch, one k_remap launch, the level-0 launch from the scratch"""
    import torch
    ctx = _ctx(gpu_ctx_factory)
    before = ctx.debug_remap_launches()
    n = 0
    with ctx.batch_session(2, SESSION_SIZES):
        for case in (("undistort06", 160, 120, 0), ("undistort06", 203, 87, 200), ("undistort", 41, 40, 0)):
            name, w, h, border = case
            want = _want(pmv, ctx, case)
            mid = _map(pmv, ctx, name, w, h)
            big = _roi(rc.image(pmv, w, h))
            pinned = torch.empty(big.shape, dtype=torch.uint8).pin_memory()
            pinned.numpy()[...] = big
            dev = torch.from_numpy(big).to("cuda:0")
            torch.cuda.synchronize()
            sources = {"tight pageable": rc.image(pmv, w, h), "ROI view": big[2:2 + h, 3:3 + w], "pinned ROI view": pinned[2:2 + h, 3:3 + w],
                       "device ROI view": dev[2:2 + h, 3:3 + w]}
            for slot, (what, src) in enumerate(sources.items()):
                ctx.batch_frame_upload_remap(slot, src, (mid, border))
                _same_levels(_levels(ctx, slot), want, f"{rc.case_id(case)} from a {what}")
                n += 1
        # the colour form: conversion, then remap, then equalisation
        bgr = _bgr(rc.image(pmv, 203, 87))
        ctx.batch_frame_upload_remap(4, _roi(bgr)[2:2 + 87, 3:3 + 203], (_map(pmv, ctx, "undistort06", 203, 87), 200), "bgr", clahe=(3.0, (4, 3)))
        n += 1
        st = ctx.batch_upload_stats()
        rounds = ctx.batch_upload_rounds()
    ctx.frame_upload_bgr(5, bgr)
    ctx.frames_remap(5, 1, _map(pmv, ctx, "undistort06", 203, 87), 200)
    ctx.frames_clahe(5, 1, 3.0, (4, 3))
    _same_levels(_levels(ctx, 4), _levels(ctx, 5), "colour session upload with remap and CLAHE")
    after = ctx.debug_remap_launches()
    assert after[1] - before[1] == n and after[2] - before[2] == n and after[0] - before[0] == 1
    # level-0 launches: the upload's own and the one from the remap scratch; the last round adds CLAHE's in-place launch
    assert st["rounds"] == st["frames"] == n == len(rounds) and st["level0_launches"] == 2 * n + 1
    assert [r["level0_launches"] for r in rounds] == [2] * (n - 1) + [3]
    assert [r["in_place"] for r in rounds] == [0, 0, 1, 1] * 3 + [0]


def test_session_threads_mix_the_four_kinds_of_upload(pmv, gpu_ctx_factory):
    """eight threads released together: plain, CLAHE, remap and remap + CLAHE uploads, each at two sizes. The right bytes in all eight slots,
    and one k_remap launch per round that held a remap request, however the requests met"""
    ctx = _ctx(gpu_ctx_factory)
    clahe = (3.0, (4, 3))
    jobs, wants = [], []
    for w, h in ((160, 120), (203, 87)):
        img = rc.image(pmv, w, h)
        rm = rc.remapped(pmv, ("undistort06", w, h, 200))[0]
        mid = _map(pmv, ctx, "undistort06", w, h)
        for remap, cl, want in ((None, None, img), (None, clahe, cc.twin().apply(img, *clahe)[0]), ((mid, 200), None, rm), ((mid, 200), clahe, cc.twin().apply(rm, *clahe)[0])):
            jobs.append((len(jobs), img, remap, cl))
            wants.append(_upload_levels(ctx, want))
    before = ctx.debug_remap_launches(), ctx.debug_clahe_launches()
    errors = []
    with ctx.batch_session(len(jobs), SESSION_SIZES):
        start = threading.Barrier(len(jobs))

        def run(slot, img, remap, cl):
            try:
                start.wait()
                if remap is None:
                    ctx.batch_frame_upload(slot, img, "gray", clahe=cl)
                else:
                    ctx.batch_frame_upload_remap(slot, img, remap, clahe=cl)
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
    after = ctx.debug_remap_launches(), ctx.debug_clahe_launches()
    with_remap, with_clahe = after[0][1] - before[0][1], after[1][1] - before[1][1]
    print(f"eight uploads: {st}; rounds {rounds}; rounds with remap requests {with_remap}, with CLAHE requests {with_clahe}")
    assert st["frames"] == 8 and 1 <= with_remap <= 4 and 1 <= with_clahe <= 4 and max(with_remap, with_clahe) <= st["rounds"]
    assert after[0][2] - before[0][2] == with_remap and after[0][0] == before[0][0]
    # every round makes one gray level-0 launch, one more with remap requests, one more with CLAHE requests
    assert st["level0_launches"] == st["rounds"] + with_remap + with_clahe


def test_a_session_of_plain_uploads_launches_what_it_always_did(pmv, gpu_ctx_factory):
    """a fresh context: after plain uploads only, the counters are 0 and the rounds' records are those of the plain upload class"""
    ctx = gpu_ctx_factory(CAP_W, CAP_H, n_slots=3, max_tracks=64)
    sizes = [(160, 120), (203, 87), (75, 53)]
    with ctx.batch_session(1, sizes):
        for slot, (w, h) in enumerate(sizes):
            ctx.batch_frame_upload(slot, cc.image(pmv, w, h))
        st = ctx.batch_upload_stats()
        rounds = ctx.batch_upload_rounds()
    assert ctx.debug_remap_launches() == [0, 0, 0] and ctx.debug_clahe_launches() == [0, 0, 0]
    # what the code before this call existed records for these uploads (tests/test_clahe_gpu.py states the same): 160x120 and 203x87 build
    # levels 0-1, 75x53 level 0 only
    assert rounds == [dict(frames_by_levels=[0, 1, 0, 0, 0], level0_launches=1, pyrdown_launches=1, in_place=0),
                      dict(frames_by_levels=[0, 1, 0, 0, 0], level0_launches=1, pyrdown_launches=1, in_place=0),
                      dict(frames_by_levels=[1, 0, 0, 0, 0], level0_launches=1, pyrdown_launches=0, in_place=0)], rounds
    assert st == dict(rounds=3, frames=3, level0_launches=3, pyrdown_launches=2)
    for slot, (w, h) in enumerate(sizes):
        assert np.array_equal(ctx.get_level(slot, 0, CAP_W, CAP_H), cc.image(pmv, w, h))


def test_the_klt_chain_downstream(pmv, gpu_ctx_factory):
    """detect_gftt_ex -> corner_subpix -> lk_track_fb on remapped slots return the bits they return on uploads of the twin's images"""
    ctx = _ctx(gpu_ctx_factory)
    w, h = 160, 120
    frames = rc.gc.cached(("remap_pair", w, h), lambda: pmv.synth_sequence(1007, 10, 2, w, h, 0.58 * w, 0.58 * w, w / 2, h / 2)[0])
    mx, my = rc.maps(pmv, "undistort", w, h)
    ctx.frames_stage(0, frames)
    ctx.frames_remap(0, 2, _map(pmv, ctx, "undistort", w, h), 0)
    for k in range(2):
        ctx.frame_upload(2 + k, rc.twin().apply(frames[k], mx, my, 0)[0])
    cells = pmv.grid_cells(w, h)
    got, want = ctx.detect_gftt_ex(0, cells, 50, block_size=5), ctx.detect_gftt_ex(2, cells, 50, block_size=5)
    assert len(got) == len(want) and all(np.array_equal(a, b) for a, b in zip(got, want))
    pts = np.concatenate([d + c[:2] for c, d in zip(cells, want)]).astype(np.float32)
    assert len(pts) >= 20
    a, b = ctx.corner_subpix(0, pts), ctx.corner_subpix(2, pts)
    assert np.array_equal(a.view(np.uint8), b.view(np.uint8)) and not np.array_equal(a, pts)
    ta, tb = ctx.lk_track_fb(0, 1, a), ctx.lk_track_fb(2, 3, b)
    for x, y in zip(ta, tb):
        assert np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8))
    assert int((ta[1] > 0).sum()) >= 1 and int((ta[4] > 0).sum()) >= 1   # (not vacuous: tracks survive, forth and back)


def test_errors_leave_the_slots_and_the_map_table_as_they_were(pmv, gpu_ctx_factory):
    ctx = gpu_ctx_factory(CAP_W, CAP_H, n_slots=4, max_tracks=64)
    img = rc.image(pmv, 160, 120)
    mx, my = rc.maps(pmv, "undistort06", 160, 120)
    f32p = C.POINTER(C.c_float)
    # ---- maps
    ctx.lib.pmv_remap_map_create.argtypes = [C.c_void_p, C.c_int, C.c_int, f32p, f32p, C.POINTER(C.c_int)]
    out = C.c_int(-7)
    px, py = mx.ctypes.data_as(f32p), my.ctypes.data_as(f32p)
    for args in ((None, 160, 120, px, py, C.byref(out)), (ctx.h, 160, 120, None, py, C.byref(out)), (ctx.h, 160, 120, px, None, C.byref(out)),
                 (ctx.h, 160, 120, px, py, None), (ctx.h, 0, 120, px, py, C.byref(out)), (ctx.h, 160, -1, px, py, C.byref(out)),
                 (ctx.h, CAP_W + 1, 40, px, py, C.byref(out)), (ctx.h, 40, CAP_H + 1, px, py, C.byref(out))):
        assert ctx.lib.pmv_remap_map_create(*args) == INVALID, args[1:3]
    assert out.value == -7
    ids = [ctx.remap_map_create(mx, my) for _ in range(16)]
    assert sorted(ids) == list(range(16))
    code, msg = _code(lambda: ctx.remap_map_create(mx, my))
    assert code == CAPACITY and "16" in msg, msg
    for bad in (-1, 16, 99):
        code, msg = _code(lambda: ctx.remap_map_destroy(bad))
        assert code == INVALID, (bad, code, msg)
    ctx.remap_map_destroy(5)
    code, msg = _code(lambda: ctx.remap_map_destroy(5))      # destroyed already
    assert code == INVALID and "5" in msg, msg
    small = ctx.remap_map_create(*rc.maps(pmv, "undistort", 41, 40))
    assert small == 5                                         # the freed entry is used again
    # ---- the single call
    ctx.frame_upload(0, img)
    ctx.frame_upload(1, img)
    keep = _levels(ctx, 0)
    for kw, what in ((dict(map_id=-1), "map -1"), (dict(map_id=16), "map 16"), (dict(border_value=-1), "border_value"), (dict(border_value=256), "border_value")):
        args = dict(map_id=0, border_value=0)
        args.update(kw)
        code, msg = _code(lambda: ctx.frames_remap(0, 2, **args))
        assert code == INVALID and what in msg, (kw, code, msg)
    ctx.lib.pmv_frames_remap.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int]
    assert ctx.lib.pmv_frames_remap(None, 0, 2, 0, 0) == INVALID
    for first, n in ((-1, 1), (3, 2), (4, 1), (0, 5), (0, 0), (1, 2 ** 31 - 1)):
        code, msg = _code(lambda: ctx.frames_remap(first, n, 0))
        assert code == CAPACITY, (first, n, code, msg)
    # slot 2 was never staged: the range is refused as a whole and the message names the slot
    code, msg = _code(lambda: ctx.frames_remap(0, 3, 0))
    assert code == INVALID and "slot 2" in msg, msg
    # a map of another size: the message names the slot and both sizes
    code, msg = _code(lambda: ctx.frames_remap(0, 2, small))
    assert code == INVALID and "slot 0" in msg and "160x120" in msg and "41x40" in msg, msg
    ctx.frame_upload(2, rc.image(pmv, 203, 87))
    code, msg = _code(lambda: ctx.frames_remap(0, 3, 0))
    assert code == INVALID and "slot 2" in msg and "203x87" in msg and "160x120" in msg, msg
    # while a stream bracket is open; once it is closed its slots are built and may be remapped
    frames = np.stack([img, img[::-1].copy()])
    ctx.frames_stream_begin(2, frames)
    try:
        code, msg = _code(lambda: ctx.frames_remap(0, 1, 0))
        assert code == INVALID and "pmv_frames_stream_begin" in msg, msg
    finally:
        ctx.frames_stream_end()
    assert ctx.debug_remap_launches() == [0, 0, 0]
    for slot in (0, 1):
        _same_levels(_levels(ctx, slot), keep, f"slot {slot} after the refused calls")
    ctx.frames_remap(2, 1, 0, 200)
    ctx.frame_upload(3, rc.remapped(pmv, ("undistort06", 160, 120, 200))[0])
    _same_levels(_levels(ctx, 2), _levels(ctx, 3), "a slot of a finished bracket")
    # ---- the session call, and the map table while a session is open
    ctx.remap_map_destroy(7)
    with ctx.batch_session(1, [(160, 120)]):
        code, msg = _code(lambda: ctx.remap_map_destroy(0))
        assert code == INVALID and "session" in msg, msg
        for remap in ((16, 0), (-1, 0), (0, 256), (0, -1)):
            code, msg = _code(lambda: ctx.batch_frame_upload_remap(0, img, remap))
            assert code == INVALID, (remap, code, msg)
        for clahe in ((2.0, (17, 8)), (-1.0, (8, 8))):
            code, msg = _code(lambda: ctx.batch_frame_upload_remap(0, img, 0, clahe=clahe))
            assert code == INVALID, (clahe, code, msg)
        code, msg = _code(lambda: ctx.batch_frame_upload_remap(0, img, small))
        assert code == INVALID and "slot 0" in msg and "160x120" in msg and "41x40" in msg, msg
        code, msg = _code(lambda: ctx.batch_frame_upload_remap(0, rc.image(pmv, 41, 40), small))
        assert code == INVALID and "41x40" in msg and "not declared" in msg, msg
        ctx.lib.pmv_batch_frame_upload_remap.argtypes = UPLOAD_REMAP + [C.c_void_p]
        assert ctx.lib.pmv_batch_frame_upload_remap(None, 0, C.c_void_p(img.ctypes.data), 160, 120, 160, 0, 0, 0, None) == INVALID
        assert ctx.lib.pmv_batch_frame_upload_remap(ctx.h, 0, None, 160, 120, 160, 0, 0, 0, None) == INVALID
        assert ctx.batch_upload_stats()["rounds"] == 0
        fresh = ctx.remap_map_create(mx, my)                # creating stays legal during a session
        assert fresh == 7
        ctx.batch_frame_upload_remap(1, img, (fresh, 200))
    assert ctx.debug_remap_launches() == [1, 1, 1]
    _same_levels(_levels(ctx, 0), keep, "slot 0 after the refused session calls")
    _same_levels(_levels(ctx, 1), _levels(ctx, 3), "the session upload through a map made during the session")
    # the table is what the successful calls left: 16 maps again, none free, all usable
    code, msg = _code(lambda: ctx.remap_map_create(mx, my))
    assert code == CAPACITY, msg
    ctx.remap_map_destroy(small)
    ctx.frames_remap(0, 1, 15, 200)
    _same_levels(_levels(ctx, 0), _levels(ctx, 3), "map 15 after the refused calls")
