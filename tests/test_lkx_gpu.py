"""pmv_lk_track_ex / pmv_lk_track_fb on the GPU: the bytes of pmv_lk_track where the flags ask for nothing, the CPU twin
(tests/twin/lkx_twin.cpp) bit for bit where they do, the fused back check against the library's own two-call composition, the session
forms, the contract. One 256x128 context with four slots: Pair A in slots 0 and 1, Crop in slots 2 and 3 (tests/lkx_common.py)."""
import ctypes as C
import threading

import numpy as np
import pytest

import lkx_common as lx

pytestmark = pytest.mark.gpu

MIN_TRACKED = 60     # of the 320 points, by the twin: a comparison "where status = 1" must not be empty
_state = {}
SIZE_IDS = dict(ids=lambda s: f"{s[0]}x{s[1]}")


def _ctx(pmv, gpu_ctx_factory, size, win=32, max_level=4, general=False):
    """the shared context under (win, max_level) with both scenes of `size` uploaded; uploads only when something changed"""
    if "ctx" not in _state:
        _state["ctx"] = gpu_ctx_factory(256, 128, n_slots=4, max_tracks=1024)
    ctx = _state["ctx"]
    key = (size, win, max_level)
    if _state.get("key") != key:
        ctx.set_lk_params(win=win, max_level=max_level)
        a, b, _ = lx.pair_a(pmv, *size)
        p, n, _, _ = lx.crop(pmv, *size)
        for slot, img in enumerate((a, b, p, n)):
            ctx.frame_upload(slot, img)
        _state["key"] = key
    ctx.debug_lk_general(general)
    return ctx


def _twin(key, fn):
    return lx.twin_cached(("gpu",) + key, fn)


def _same_bytes(got, want, what):
    for k, (g, r) in enumerate(zip(got, want)):
        assert np.array_equal(lx.bits(g), lx.bits(r)), f"{what}: output {k} differs at {np.flatnonzero((lx.bits(g) != lx.bits(r)).reshape(len(r), -1).any(axis=1))[:8]}"


def _same_where_tracked(got, want, what, err_everywhere=False):
    (xy, st, err), (rxy, rst, rerr) = got, want
    tracked = int(rst.sum())
    print(f"{what}: {tracked} of {len(rst)} tracked by the twin")
    assert tracked >= MIN_TRACKED, f"{what}: the twin tracks only {tracked} points"
    assert np.array_equal(st, rst), f"{what}: status differs at {np.flatnonzero(st != rst)[:8]}"
    ok = rst > 0
    assert np.array_equal(lx.bits(xy)[ok], lx.bits(rxy)[ok]), f"{what}: positions differ at {np.flatnonzero((lx.bits(xy) != lx.bits(rxy)).any(axis=1) & ok)[:8]}"
    e = np.ones_like(ok) if err_everywhere else ok
    assert np.array_equal(lx.bits(err)[e], lx.bits(rerr)[e]), f"{what}: err differs at {np.flatnonzero((lx.bits(err) != lx.bits(rerr)) & e)[:8]}"


@pytest.mark.parametrize("size", lx.SIZES, **SIZE_IDS)
@pytest.mark.parametrize("win, max_level, general", [(32, 4, False), (32, 4, True), (21, 3, False)], ids=["32-tuned", "32-general", "21"])
def test_without_flags_it_is_lk_track(pmv, gpu_ctx_factory, size, win, max_level, general):
    """1. flags 0, and an initial flow equal to the points: all bytes of all three outputs"""
    ctx = _ctx(pmv, gpu_ctx_factory, size, win, max_level, general)
    pts = lx.pair_a(pmv, *size)[2]
    want = ctx.lk_track(0, 1, pts)
    assert int(want[1].sum()) >= MIN_TRACKED
    _same_bytes(ctx.lk_track_ex(0, 1, pts), want, "flags 0")
    _same_bytes(ctx.lk_track_ex(0, 1, pts, init_xy=pts), want, "init = prev")


INIT_CASES = [(32, 4, False), (32, 4, True), (21, 1, False), (21, 0, False), (15, 4, False), (63, 4, False), (3, 4, False)]


@pytest.mark.parametrize("size", lx.SIZES, **SIZE_IDS)
@pytest.mark.parametrize("win, max_level, general", INIT_CASES, ids=lambda v: str(int(v)))
def test_initial_flow_matches_the_twin(pmv, gpu_ctx_factory, size, win, max_level, general):
    """2. Crop: status identical, xy and err bit-exact where status is 1; 40 of the guesses anywhere within 70 px of the frame"""
    ctx = _ctx(pmv, gpu_ctx_factory, size, win, max_level, general)
    a, b, pts, init = lx.crop(pmv, *size)
    wild, idx = lx.wild_init(*size, init)
    assert ((wild[idx] < 0).any(axis=1) | (wild[idx, 0] >= size[0]) | (wild[idx, 1] >= size[1])).sum() >= 5, "no guess outside the frame"
    want = _twin(("init", size, win, max_level), lambda: lx.twin().track(a, b, pts, init=wild, win=win, max_level=max_level))
    got = ctx.lk_track_ex(2, 3, pts, init_xy=wild)
    _same_where_tracked(got, want, f"{size} win {win} maxLevel {max_level}")
    print("status 1 among the 40 wild guesses:", int(want[1][idx].sum()))
    plain = ctx.lk_track_ex(2, 3, pts)
    assert not np.array_equal(lx.bits(plain[0]), lx.bits(got[0])), "the initial flow changes nothing"


@pytest.mark.parametrize("size", lx.SIZES, **SIZE_IDS)
@pytest.mark.parametrize("win, max_level, general", [(32, 4, False), (32, 4, True), (21, 3, False)], ids=["32-tuned", "32-general", "21"])
@pytest.mark.parametrize("scene", ["pairA", "crop-init"])
def test_min_eigenvalue_error(pmv, gpu_ctx_factory, size, win, max_level, general, scene):
    """3. err bit-exact against the twin at ALL points; xy and status those of the call without the flag"""
    ctx = _ctx(pmv, gpu_ctx_factory, size, win, max_level, general)
    if scene == "pairA":
        (a, b, pts), init, s0 = lx.pair_a(pmv, *size), None, 0
    else:
        a, b, pts, init = lx.crop(pmv, *size)
        s0 = 2
    want = _twin(("eig", scene, size, win, max_level), lambda: lx.twin().track(a, b, pts, init=init, flags=lx.EIG, win=win, max_level=max_level))
    got = ctx.lk_track_ex(s0, s0 + 1, pts, init_xy=init, min_eigenvals=True)
    _same_where_tracked(got, want, f"{scene} {size} win {win}", err_everywhere=True)
    failed_with_err = int(((got[1] == 0) & (got[2] != 0)).sum())
    print("status-0 points with a non-zero err:", failed_with_err)
    if scene == "pairA":
        assert failed_with_err >= 5
    plain = ctx.lk_track_ex(s0, s0 + 1, pts, init_xy=init)
    _same_bytes(got[:2], plain[:2], "xy / status with the flag vs without")
    assert not np.array_equal(lx.bits(got[2]), lx.bits(plain[2]))


@pytest.mark.parametrize("size", lx.SIZES, **SIZE_IDS)
@pytest.mark.parametrize("win, max_level", [(32, 4), (21, 3)])
@pytest.mark.parametrize("scene", ["pairA", "crop-init"])
@pytest.mark.parametrize("eig", [False, True], ids=["residual", "mineig"])
def test_back_check_is_the_two_call_composition(pmv, gpu_ctx_factory, size, win, max_level, scene, eig):
    """4. byte for byte the library's own two calls, the stated outputs of forward-failed tracks included; and the twin's composition"""
    ctx = _ctx(pmv, gpu_ctx_factory, size, win, max_level)
    if scene == "pairA":
        (a, b, pts), init, s0 = lx.pair_a(pmv, *size), None, 0
    else:
        a, b, pts, init = lx.crop(pmv, *size)
        s0 = 2
    got = ctx.lk_track_fb(s0, s0 + 1, pts, init_xy=init, min_eigenvals=eig)
    fwd = ctx.lk_track_ex(s0, s0 + 1, pts, init_xy=init, min_eigenvals=eig)
    ok = fwd[1] > 0
    assert MIN_TRACKED <= int(ok.sum()) < len(pts), "the scene needs tracked and failed points"
    back = ctx.lk_track_ex(s0 + 1, s0, fwd[0][ok], init_xy=pts[ok], min_eigenvals=eig)
    bxy, bst, berr = fwd[0].copy(), np.zeros(len(pts), np.uint8), np.zeros(len(pts), np.float32)
    bxy[ok], bst[ok], berr[ok] = back
    _same_bytes(got, fwd + (bxy, bst, berr), "lk_track_fb vs two lk_track_ex calls")
    want = _twin(("fb", scene, size, win, max_level, eig), lambda: lx.twin().track_fb(a, b, pts, init=init, flags=lx.EIG if eig else 0, win=win, max_level=max_level))
    _same_where_tracked(got[:3], want[:3], f"forward, {scene} {size} win {win}", err_everywhere=eig)
    assert np.array_equal(got[4], want[4]), "back status differs from the twin"
    both = want[4] > 0
    assert int(both.sum()) >= MIN_TRACKED
    assert np.array_equal(lx.bits(got[3])[both], lx.bits(want[3])[both]) and np.array_equal(lx.bits(got[5])[both], lx.bits(want[5])[both])
    if scene == "crop-init" and size == (160, 120):
        kept = both & (np.linalg.norm(got[3].astype(np.float64) - pts, axis=1) < 0.5)
        print("the back check keeps", int(kept.sum()), "tracks")
        assert int(kept.sum()) >= 100


def _threads(n, fn):
    res, errors = [None] * n, []
    start = threading.Barrier(n)

    def run(j):
        try:
            start.wait()
            res[j] = fn(j)
        except Exception as e:   # noqa: BLE001
            errors.append((j, repr(e)))
    th = [threading.Thread(target=run, args=(j,)) for j in range(n)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors, errors
    return res


@pytest.mark.parametrize("win, max_level, general", [(32, 4, False), (32, 4, True), (21, 3, False)], ids=["32-tuned", "32-general", "21"])
def test_session_forms(pmv, gpu_ctx_factory, win, max_level, general):
    """5. both sizes declared; three threads issue plain, ex and fb requests at once: the bytes of the single calls, at most two LK
    launches per round; plain requests alone: at most one"""
    ctx = gpu_ctx_factory(256, 128, n_slots=4, max_tracks=1024)
    ctx.set_lk_params(win=win, max_level=max_level)
    ctx.debug_lk_general(general)
    pa = lx.pair_a(pmv, *lx.SIZES[0])
    cr = lx.crop(pmv, *lx.SIZES[1])
    for slot, img in enumerate((pa[0], pa[1], cr[0], cr[1])):
        ctx.frame_upload(slot, img)
    calls = [("lk_track", (0, 1, pa[2]), {}),
             ("lk_track_ex", (2, 3, cr[2]), dict(init_xy=cr[3])),
             ("lk_track_fb", (2, 3, cr[2]), dict(init_xy=cr[3], min_eigenvals=True)),
             ("lk_track_ex", (0, 1, pa[2]), dict(min_eigenvals=True)),
             ("lk_track_fb", (0, 1, pa[2][:100]), {}),
             ("lk_track", (2, 3, cr[2]), {})]
    want = [getattr(ctx, m)(*a, **kw) for m, a, kw in calls]
    l0, s0 = ctx.batch_launches()["k_lk_batch"], ctx.batch_stats()["lk"]["launches"]
    with ctx.batch_session(1, lx.SIZES):
        got = _threads(3, lambda j: [getattr(ctx, "batch_" + calls[(j + i) % 6][0])(*calls[(j + i) % 6][1], **calls[(j + i) % 6][2]) for i in range(6)])
    launches, rounds = ctx.batch_launches()["k_lk_batch"] - l0, ctx.batch_stats()["lk"]["launches"] - s0
    print("mixed session: LK launches", launches, "rounds", rounds, "requests 18")
    assert 0 < rounds <= 18 and rounds <= launches <= 2 * rounds
    for j in range(3):
        for i in range(6):
            _same_bytes(got[j][i], want[(j + i) % 6], f"thread {j}, request {i} ({calls[(j + i) % 6][0]})")
    l0, s0 = ctx.batch_launches()["k_lk_batch"], ctx.batch_stats()["lk"]["launches"]
    with ctx.batch_session(1, lx.SIZES):
        got = _threads(3, lambda j: [ctx.batch_lk_track(*calls[0][1]), ctx.batch_lk_track(*calls[5][1])])
    launches, rounds = ctx.batch_launches()["k_lk_batch"] - l0, ctx.batch_stats()["lk"]["launches"] - s0
    print("plain session: LK launches", launches, "rounds", rounds)
    assert 0 < launches <= rounds <= 6
    for j in range(3):
        _same_bytes(got[j][0], want[0], "plain request in a plain session")
        _same_bytes(got[j][1], want[5], "plain request in a plain session")


_f32p, _u8p = C.POINTER(C.c_float), C.POINTER(C.c_uint8)


def _raw(ctx, fn, prev_slot, next_slot, pts, nxt, flags, n=None, null=None, fb=False):
    """the C call itself on sentinel-filled outputs: (status code, True if no output byte changed)"""
    n = len(pts) if n is None else n
    m = max(len(pts), 1)
    bufs = dict(next=np.array(nxt, np.float32), st=np.full(m, 0xAB, np.uint8), err=np.full(m, -7.5, np.float32), bxy=np.full((m, 2), -7.5, np.float32),
                bst=np.full(m, 0xAB, np.uint8), berr=np.full(m, -7.5, np.float32))
    before = {k: v.tobytes() for k, v in bufs.items()}

    def ptr(k, t):
        return None if k == null else bufs[k].ctypes.data_as(t)
    p = np.ascontiguousarray(pts, np.float32)
    args = [ctx.h, prev_slot, next_slot, None if null == "prev" else p.ctypes.data_as(_f32p), n, ptr("next", _f32p), flags, ptr("st", _u8p), ptr("err", _f32p)]
    if fb:
        args += [ptr("bxy", _f32p), ptr("bst", _u8p), ptr("berr", _f32p)]
    rc = fn(*args)
    return rc, all(v.tobytes() == before[k] for k, v in bufs.items())


def test_contract(pmv, gpu_ctx_factory):
    """6. every error returns its code with the outputs untouched; flags 0 on a context that never called the setter; the extended calls
    follow pmv_set_lk_params"""
    size = lx.SIZES[0]
    a, b, pts = lx.pair_a(pmv, *size)
    ctx = gpu_ctx_factory(256, 128, n_slots=3, max_tracks=400)
    ctx.frame_upload(0, a)
    ctx.frame_upload(1, b)
    never = ctx.lk_track(0, 1, pts)
    _same_bytes(ctx.lk_track_ex(0, 1, pts), never, "flags 0, no setter call")
    fbr = ctx.lk_track_fb(0, 1, pts)
    _same_bytes(fbr[:3], never, "forward half of lk_track_fb, no setter call")
    INVALID, CAPACITY = -2, -3
    lib = ctx.lib
    bad_init = {"nan": np.nan, "inf": np.inf, "-inf": -np.inf, "2e6": 2e6, "-1.5e6": -1.5e6}
    lib.pmv_thread_error.restype = C.c_char_p

    def errors(fn, fb, what):
        for flags in (1, 2, 16, 4 | 1, 12 | 256, -1):
            assert _raw(ctx, fn, 0, 1, pts, pts, flags, fb=fb) == (INVALID, True), (what, flags)
        for null in ("prev", "next", "st", "err") + (("bxy", "bst", "berr") if fb else ()):
            assert _raw(ctx, fn, 0, 1, pts, pts, 0, null=null, fb=fb) == (INVALID, True), (what, null)
        for name, v in bad_init.items():
            nxt = pts.copy()
            nxt[37, 1] = v
            assert _raw(ctx, fn, 0, 1, pts, nxt, 4, fb=fb) == (INVALID, True), (what, name)
            assert "point 37" in lib.pmv_thread_error().decode(), (what, name)
            # without the flag the array is output only: whatever it holds is no error
            assert _raw(ctx, fn, 0, 1, pts[:8], nxt[30:38], 0, fb=fb)[0] == 0, (what, name)
        many = np.tile(pts, (2, 1))[:401]
        assert _raw(ctx, fn, 0, 1, many, many, 0, fb=fb) == (CAPACITY, True), what
        assert _raw(ctx, fn, 0, 3, pts, pts, 0, fb=fb) == (CAPACITY, True), what      # slot out of range: as pmv_lk_track
        assert _raw(ctx, fn, 0, 2, pts, pts, 0, fb=fb) == (INVALID, True), what       # slot never uploaded: as pmv_lk_track
        assert _raw(ctx, fn, 0, 1, pts, pts, 12, n=0, fb=fb) == (0, True), what

    errors(lib.pmv_lk_track_ex, False, "pmv_lk_track_ex")
    errors(lib.pmv_lk_track_fb, True, "pmv_lk_track_fb")
    with ctx.batch_session(1, [size]):
        errors(lib.pmv_batch_lk_track_ex, False, "pmv_batch_lk_track_ex")
        errors(lib.pmv_batch_lk_track_fb, True, "pmv_batch_lk_track_fb")
    # the setter reaches the extended calls
    ctx.set_lk_params(win=21, max_level=3)
    ctx.frame_upload(0, a)
    ctx.frame_upload(1, b)
    want = ctx.lk_track(0, 1, pts)
    assert not np.array_equal(lx.bits(want[0]), lx.bits(never[0]))
    _same_bytes(ctx.lk_track_ex(0, 1, pts), want, "flags 0 after set_lk_params(21, 3)")
    _same_bytes(ctx.lk_track_fb(0, 1, pts)[:3], want, "lk_track_fb after set_lk_params(21, 3)")


def test_counters_add_both_directions(pmv, gpu_ctx_factory):
    """pmv_lk_counters: a forward-backward track counts once, with the iterations and level passes of both directions"""
    size = lx.SIZES[0]
    ctx = _ctx(pmv, gpu_ctx_factory, size)
    _, _, pts, init = lx.crop(pmv, *size)
    ctx.lk_counters(reset=True)
    fwd = ctx.lk_track_ex(2, 3, pts, init_xy=init)
    c_fwd = ctx.lk_counters(reset=True)
    ok = fwd[1] > 0
    ctx.lk_track_ex(3, 2, fwd[0][ok], init_xy=pts[ok])
    c_back = ctx.lk_counters(reset=True)
    ctx.lk_track_fb(2, 3, pts, init_xy=init)
    c_fb = ctx.lk_counters(reset=True)
    print("forward", c_fwd, "back", c_back, "fused", c_fb)
    assert c_fb[2] == len(pts) == c_fwd[2]
    assert c_fb[1] == c_fwd[1] + c_back[1]
    assert c_fb[0] == c_fwd[0] + c_back[0]   # (no track of this scene comes near 255 iterations)
