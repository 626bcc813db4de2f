"""pmv_lk_track_fb_levels on the GPU: cv's maxLevel per call on pyramids that are already built. The yardstick is the existing LK twin
(tests/twin/lkx_twin.cpp) with max_level = min(top, the context's max_level) per pass, composed in tests/predict_common.py - status
identical, positions and err bit for bit where the status is 1, as for the other extended calls (tests/test_lkx_gpu.py). Next to it the
library's own bytes: (-1, -1) is pmv_lk_track_fb, the forward-only form is pmv_lk_track_ex, and a capped call equals the plain call of a
context whose pyramids were BUILT no deeper than the cap. Scenes: Pair A and Crop of tests/lkx_common.py, and Pair A at 517 x 261, where the
tuned kernels have four levels to cap."""
import ctypes as C

import numpy as np
import pytest

import lkx_common as lx
import predict_common as pc

pytestmark = pytest.mark.gpu

MIN_TRACKED = 60
LEVELS = [(-1, -1), (0, 0), (1, 1), (1, -1), (4, 0)]
CASES = [(32, 4, False), (32, 4, True), (21, 3, False)]
CASE_IDS = ["32-tuned", "32-general", "21"]
SIZE_IDS = dict(ids=lambda s: f"{s[0]}x{s[1]}")
BIG = (517, 261)
_state = {}


def _ctx(pmv, gpu_ctx_factory, which, size, win, max_level, general=False):
    """one of two shared contexts ("main": the calls under test, "built": pyramids built no deeper than a cap) under (win, max_level) with
    Pair A in slots 0, 1 and - at the small sizes - Crop in slots 2, 3; uploads only when something changed"""
    if which not in _state:
        _state[which] = [gpu_ctx_factory(528, 264, n_slots=4, max_tracks=1024), None]
    ctx, key = _state[which]
    if key != (size, win, max_level):
        ctx.set_lk_params(win=win, max_level=max_level)
        imgs = list(lx.pair_a(pmv, *size)[:2]) + (list(lx.crop(pmv, *size)[:2]) if size != BIG else [])
        for slot, img in enumerate(imgs):
            ctx.frame_upload(slot, img)
        _state[which][1] = (size, win, max_level)
    ctx.debug_lk_general(general)
    return ctx


def _levels_of(size, win, max_level):
    """cv::buildOpticalFlowPyramid's rule (include/pmv_hip.h, pmv_set_lk_params)"""
    w, h, n = size[0], size[1], 1
    while n <= max_level and (w + 1) // 2 > win and (h + 1) // 2 > win:
        w, h, n = (w + 1) // 2, (h + 1) // 2, n + 1
    return n


def _same_bytes(got, want, what):
    assert len(got) == len(want), what
    for k, (g, r) in enumerate(zip(got, want)):
        assert g.dtype == r.dtype and np.array_equal(lx.bits(g), lx.bits(r)), f"{what}: output {k} differs at {np.flatnonzero((lx.bits(g) != lx.bits(r)).reshape(len(r), -1).any(axis=1))[:8]}"


def _same_as_twin(got, want, what, eig=False):
    """status identical; xy and err bit-exact where the status is 1 (err everywhere with the min-eigenvalue measure); the same for the back
    outputs, whose forward-failed tracks are defined in full"""
    st, rst = got[1], want[1]
    assert np.array_equal(st, rst), f"{what}: status differs at {np.flatnonzero(st != rst)[:8]}"
    ok = rst > 0
    assert int(ok.sum()) >= MIN_TRACKED, f"{what}: the twin tracks only {int(ok.sum())} points"
    assert np.array_equal(lx.bits(got[0])[ok], lx.bits(want[0])[ok]), f"{what}: positions differ at {np.flatnonzero((lx.bits(got[0]) != lx.bits(want[0])).any(axis=1) & ok)[:8]}"
    e = np.ones_like(ok) if eig else ok
    assert np.array_equal(lx.bits(got[2])[e], lx.bits(want[2])[e]), f"{what}: err differs"
    if len(want) == 3:
        return
    assert np.array_equal(got[4], want[4]), f"{what}: back status differs at {np.flatnonzero(got[4] != want[4])[:8]}"
    both = want[4] > 0
    assert int(both.sum()) >= MIN_TRACKED // 2, f"{what}: the twin takes only {int(both.sum())} points back"
    assert np.array_equal(lx.bits(got[3])[both], lx.bits(want[3])[both]) and np.array_equal(lx.bits(got[5])[both], lx.bits(want[5])[both]), f"{what}: back outputs differ"
    failed = ~ok
    assert np.array_equal(lx.bits(got[3])[failed], lx.bits(got[0])[failed]) and not got[5][failed].any(), f"{what}: the back outputs of forward-failed tracks"


def _scene(pmv, size, scene):
    """(prev, next, points, initial flow or None, first slot)"""
    if scene == "pairA":
        a, b, pts = lx.pair_a(pmv, *size)
        return a, b, pts, None, 0
    a, b, pts, init = lx.crop(pmv, *size)
    return a, b, pts, lx.wild_init(*size, init)[0], 2


def _twin(size, scene, win, max_level, levels, eig, pmv, back=True):
    a, b, pts, init, _ = _scene(pmv, size, scene)
    return lx.twin_cached(("levels", size, scene, win, max_level, levels, eig, back),
                          lambda: pc.twin_fb_levels(a, b, pts, init, lx.EIG if eig else 0, levels[0], levels[1], win, max_level, back=back))


@pytest.mark.parametrize("size", lx.SIZES, **SIZE_IDS)
@pytest.mark.parametrize("win, max_level, general", CASES, ids=CASE_IDS)
@pytest.mark.parametrize("scene", ["pairA", "crop-wild"])
def test_levels_match_the_twin(pmv, gpu_ctx_factory, size, win, max_level, general, scene):
    ctx = _ctx(pmv, gpu_ctx_factory, "main", size, win, max_level, general)
    L = _levels_of(size, win, max_level)
    assert ctx.num_levels(0) == L - 1
    _, _, pts, init, s0 = _scene(pmv, size, scene)
    full = _twin(size, scene, win, max_level, (-1, -1), False, pmv)
    differs = 0
    for levels in LEVELS:
        for eig in ((False, True) if levels == (1, -1) else (False,)):
            what = f"{scene} {size} win {win} L {L} levels {levels} eig {eig}"
            want = _twin(size, scene, win, max_level, levels, eig, pmv)
            got = ctx.lk_track_fb_levels(s0, s0 + 1, pts, init_xy=init, min_eigenvals=eig, fwd_top_level=levels[0], back_top_level=levels[1])
            _same_as_twin(got, want, what, eig)
            capped = min(levels[0] % 5, L - 1) < L - 1   # (-1 % 5 = 4: no cap)
            if not eig and capped:
                t = (want[1] > 0) & (full[1] > 0)
                assert (lx.bits(want[0])[t] != lx.bits(full[0])[t]).any(), f"{what}: the twin's capped pass equals its full pass - the case shows nothing"
                differs += 1
        if levels[0] == 4 or levels == (-1, -1):   # clamped by L: the forward half is the uncapped one
            _same_bytes(got[:3], ctx.lk_track_fb(s0, s0 + 1, pts, init_xy=init)[:3], f"{scene} {size} levels {levels}: forward half vs pmv_lk_track_fb")
    assert differs >= 1, "no level of LEVELS is a cap at this size"
    _same_bytes(ctx.lk_track_fb_levels(s0, s0 + 1, pts, init_xy=init), ctx.lk_track_fb(s0, s0 + 1, pts, init_xy=init), "(-1, -1) vs pmv_lk_track_fb")


@pytest.mark.parametrize("size", lx.SIZES, **SIZE_IDS)
@pytest.mark.parametrize("win, max_level, general", CASES, ids=CASE_IDS)
def test_forward_only(pmv, gpu_ctx_factory, size, win, max_level, general):
    """three null back outputs: the bytes of pmv_lk_track_ex at top -1, the twin's forward pass at a cap; the back level is ignored"""
    ctx = _ctx(pmv, gpu_ctx_factory, "main", size, win, max_level, general)
    for scene in ("pairA", "crop-wild"):
        _, _, pts, init, s0 = _scene(pmv, size, scene)
        _same_bytes(ctx.lk_track_fb_levels(s0, s0 + 1, pts, init_xy=init, back=False), ctx.lk_track_ex(s0, s0 + 1, pts, init_xy=init), f"{scene}: forward only, top -1")
        for top, eig in ((0, False), (1, True)):
            got = ctx.lk_track_fb_levels(s0, s0 + 1, pts, init_xy=init, min_eigenvals=eig, fwd_top_level=top, back_top_level=3, back=False)
            assert len(got) == 3
            _same_as_twin(got, _twin(size, scene, win, max_level, (top, -1), eig, pmv, back=False), f"{scene} {size} win {win} forward only, top {top}", eig)
            _same_bytes(got, ctx.lk_track_fb_levels(s0, s0 + 1, pts, init_xy=init, min_eigenvals=eig, fwd_top_level=top, back_top_level=0)[:3], "forward half of the fb form")


@pytest.mark.parametrize("size", lx.SIZES + [BIG], **SIZE_IDS)
@pytest.mark.parametrize("win, max_level, general", CASES, ids=CASE_IDS)
def test_a_cap_is_a_pyramid_built_no_deeper(pmv, gpu_ctx_factory, size, win, max_level, general):
    """all bytes, failed tracks included: top = (k, k) on the pyramids of (win, max_level) equals pmv_lk_track_fb of a context whose
    pyramids were built with max_level = k; at 517 x 261 the pyramid has four levels at both windows"""
    L = _levels_of(size, win, max_level)
    assert L == (4 if size == BIG else 2 if win == 32 else 3)
    scenes = ("pairA",) if size == BIG else ("pairA", "crop-wild")
    got = {}
    ctx = _ctx(pmv, gpu_ctx_factory, "main", size, win, max_level, general)
    for scene in scenes:
        _, _, pts, init, s0 = _scene(pmv, size, scene)
        for k in range(L):
            got[scene, k] = ctx.lk_track_fb_levels(s0, s0 + 1, pts, init_xy=init, fwd_top_level=k, back_top_level=k)
    for k in range(L):
        built = _ctx(pmv, gpu_ctx_factory, "built", size, win, k, general)
        assert built.num_levels(0) == k
        for scene in scenes:
            _, _, pts, init, s0 = _scene(pmv, size, scene)
            want = built.lk_track_fb(s0, s0 + 1, pts, init_xy=init)
            assert int(want[1].sum()) >= (MIN_TRACKED if k else 20)
            _same_bytes(got[scene, k], want, f"{scene} {size} win {win}: top {k} vs a pyramid of {k + 1} levels")
            if k:
                assert not np.array_equal(lx.bits(got[scene, k][0]), lx.bits(got[scene, k - 1][0])), "one level more changes nothing"
    if size == BIG:   # the twin at the size where the tuned kernels have levels to drop
        a, b, pts = lx.pair_a(pmv, *size)
        for levels in ((1, 1), (2, 0), (0, 3)):
            want = lx.twin_cached(("levels-big", win, levels), lambda: pc.twin_fb_levels(a, b, pts, None, 0, levels[0], levels[1], win, max_level))
            _same_as_twin(ctx.lk_track_fb_levels(0, 1, pts, fwd_top_level=levels[0], back_top_level=levels[1]), want, f"{size} win {win} levels {levels}")


def test_counters_show_the_levels_that_ran(pmv, gpu_ctx_factory):
    """pmv_lk_counters: (track, level) passes - at (0, 0) a track makes at most one pass per direction, at (-1, -1) the crop scene makes more"""
    size = lx.SIZES[0]
    ctx = _ctx(pmv, gpu_ctx_factory, "main", size, 21, 3)
    _, _, pts, init = lx.crop(pmv, *size)
    ctx.lk_counters(reset=True)
    full = ctx.lk_track_fb_levels(2, 3, pts, init_xy=init)
    c_full = ctx.lk_counters(reset=True)
    low = ctx.lk_track_fb_levels(2, 3, pts, init_xy=init, fwd_top_level=0, back_top_level=0)
    c_low = ctx.lk_counters(reset=True)
    mixed = ctx.lk_track_fb_levels(2, 3, pts, init_xy=init, fwd_top_level=-1, back_top_level=0)
    c_mixed = ctx.lk_counters(reset=True)
    print("full", c_full, "(0, 0)", c_low, "(-1, 0)", c_mixed)
    assert c_full[2] == c_low[2] == c_mixed[2] == len(pts)
    assert c_low[1] <= len(pts) + int(low[1].sum()) < c_full[1]
    _same_bytes(mixed[:3], full[:3], "the forward half does not depend on the back level")
    assert c_low[1] < c_mixed[1] < c_full[1]


_f32p, _u8p = C.POINTER(C.c_float), C.POINTER(C.c_uint8)


def _raw(ctx, pts, nxt, flags, fwd, back, n=None, null=(), prev_slot=0, next_slot=1):
    """the C call itself on sentinel-filled outputs: (status code, True if no output byte changed)"""
    fn = ctx.lib.pmv_lk_track_fb_levels
    fn.argtypes = [C.c_void_p, C.c_int, C.c_int, _f32p, C.c_int, _f32p, C.c_int, C.c_int, C.c_int, _u8p, _f32p, _f32p, _u8p, _f32p]
    n = len(pts) if n is None else n
    m = max(len(pts), 1)
    bufs = dict(next=np.array(nxt, np.float32), st=np.full(m, 0xAB, np.uint8), err=np.full(m, -7.5, np.float32), bxy=np.full((m, 2), -7.5, np.float32),
                bst=np.full(m, 0xAB, np.uint8), berr=np.full(m, -7.5, np.float32))
    before = {k: v.tobytes() for k, v in bufs.items()}

    def ptr(k, t):
        return None if k in null else bufs[k].ctypes.data_as(t)
    p = np.ascontiguousarray(pts, np.float32)
    rc = fn(ctx.h, prev_slot, next_slot, None if "prev" in null else p.ctypes.data_as(_f32p), n, ptr("next", _f32p), flags, fwd, back, ptr("st", _u8p), ptr("err", _f32p),
            ptr("bxy", _f32p), ptr("bst", _u8p), ptr("berr", _f32p))
    return rc, all(v.tobytes() == before[k] for k, v in bufs.items())


def test_refusals_write_nothing(pmv, gpu_ctx_factory):
    INVALID, CAPACITY = -2, -3
    size = lx.SIZES[0]
    a, b, pts = lx.pair_a(pmv, *size)
    ctx = gpu_ctx_factory(256, 128, n_slots=3, max_tracks=400)
    ctx.frame_upload(0, a)
    ctx.frame_upload(1, b)
    ctx.lib.pmv_thread_error.restype = C.c_char_p
    for fwd, back in ((-2, -1), (5, 0), (0, -2), (1, 5), (-3, 7), (1 << 30, 0), (0, -(1 << 31))):
        for null in ((), ("bxy", "bst", "berr")):
            assert _raw(ctx, pts, pts, 0, fwd, back, null=null) == (INVALID, True), (fwd, back, null)
            assert "top_level" in ctx.lib.pmv_thread_error().decode()
    for null in (("bxy",), ("bst",), ("berr",), ("bxy", "bst"), ("bxy", "berr"), ("bst", "berr")):
        assert _raw(ctx, pts, pts, 0, 1, 1, null=null) == (INVALID, True), null
        assert "back outputs" in ctx.lib.pmv_thread_error().decode()
    for null in (("prev",), ("next",), ("st",), ("err",), ("st", "bxy", "bst", "berr")):
        assert _raw(ctx, pts, pts, 0, 1, 1, null=null) == (INVALID, True), null
    for flags in (1, 2, 16, 4 | 1, 12 | 256, -1):
        assert _raw(ctx, pts, pts, flags, 0, 0) == (INVALID, True), flags
    nxt = pts.copy()
    nxt[37, 1] = np.nan
    assert _raw(ctx, pts, nxt, 4, 1, 1) == (INVALID, True) and "point 37" in ctx.lib.pmv_thread_error().decode()
    many = np.tile(pts, (2, 1))[:401]
    assert _raw(ctx, many, many, 0, 1, 1) == (CAPACITY, True)
    assert _raw(ctx, pts, pts, 0, 1, 1, next_slot=3) == (CAPACITY, True)      # slot out of range: as pmv_lk_track
    assert _raw(ctx, pts, pts, 0, 1, 1, next_slot=2) == (INVALID, True)       # slot never uploaded: as pmv_lk_track
    assert _raw(ctx, pts, pts, 12, 4, -1, n=0) == (0, True)
    # every legal level is accepted, whatever the pyramid's depth; good calls afterwards
    want = ctx.lk_track_fb(0, 1, pts)
    for fwd in range(-1, 5):
        got = ctx.lk_track_fb_levels(0, 1, pts, fwd_top_level=fwd, back_top_level=4 - max(fwd, 0))
        assert got[1].sum() >= MIN_TRACKED
    _same_bytes(ctx.lk_track_fb_levels(0, 1, pts, fwd_top_level=4, back_top_level=4), want, "levels above the pyramid's top are the top")
