"""pmv_corner_subpix on the GPU: positions, update counts and flags against the kernel-order CPU twin (tests/twin/subpix_twin.cpp) bit
for bit, for every parameter set and point set of tests/subpix_common.py; sizes of n and a point's place in the call; the contract; the
chain detector -> refinement -> LK against the three twins composed; the session form. One 320x256 context, eight slots:
0 / 4 = the 203x87 frame, 1 / 5 = 160x120, 2 = the horizontal ramp (96x80), 3 = a flat 60x60 frame, 6 = the frame after 1, 7 stays empty."""
import ctypes as C
import threading

import numpy as np
import pytest

import gftt_common as gc
import lkx_common as lx
import subpix_common as sc

pytestmark = pytest.mark.gpu

INVALID, CAPACITY = -2, -3
MAX_TRACKS = 512
EMPTY_SLOT = 7
SLOT_OF = {(203, 87): 0, (160, 120): 1}
_state = {}
_u8p, _f32p = C.POINTER(C.c_uint8), C.POINTER(C.c_float)


def _flat():
    return gc.cached("flat60", lambda: np.full((60, 60), 93, np.uint8))


def _ctx(pmv, gpu_ctx_factory):
    if "ctx" not in _state:
        ctx = gpu_ctx_factory(320, 256, n_slots=8, max_tracks=MAX_TRACKS)
        frames = [gc.frame(pmv, 203, 87), gc.frame(pmv, 160, 120), gc.gradient_frame(), _flat(), gc.frame(pmv, 203, 87), gc.frame(pmv, 160, 120),
                  lx.pair_a(pmv, 160, 120)[1]]
        for slot, img in enumerate(frames):
            ctx.frame_upload(slot, img)
        _state["ctx"] = ctx
    return _state["ctx"]


def _same(got, want, what):
    """positions bit for bit, update counts, flags"""
    (xy, it, fl), (rxy, rit, rfl) = got, want[:3]
    bad = (sc.bits(xy) != sc.bits(rxy)).any(axis=1) | (it != rit) | (fl != rfl)
    assert not bad.any(), f"{what}: {bad.sum()} of {len(bad)} points differ, first {np.flatnonzero(bad)[:6]}: got {xy[bad][:3]}, {it[bad][:3]}, {fl[bad][:3]}; " \
                          f"the twin {rxy[bad][:3]}, {rit[bad][:3]}, {rfl[bad][:3]}"


@pytest.mark.parametrize("size", sc.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", list(sc.PARAMS))
def test_every_parameter_set_matches_the_twin(pmv, gpu_ctx_factory, size, name):
    ctx = _ctx(pmv, gpu_ctx_factory)
    w, h = size
    kw = sc.PARAMS[name]
    for edge in (False, True):
        pts = sc.edge_points(w, h, kw["win"]) if edge else sc.scene_points(pmv, w, h)
        want = sc.refined(pmv, w, h, name, sc.KERNEL, edge)
        for i in range(0, len(pts), MAX_TRACKS):
            got = ctx.corner_subpix(SLOT_OF[size], pts[i:i + MAX_TRACKS], return_info=True, **kw)
            _same(got, [a[i:i + MAX_TRACKS] for a in want], f"{name} {size} {'edge' if edge else 'scene'}")
        if not edge:
            moved = (sc.bits(want[0]) != sc.bits(pts)).any(axis=1)
            print(f"{name} {size}: {len(pts)} points, {moved.sum()} moved, updates max {want[1].max()}, flags {np.bincount(want[2], minlength=16).tolist()}")
            assert moved.sum() >= len(pts) // 8, "the scene moves too few points to compare anything"


def test_flat_and_ramp_frames_return_every_point_unchanged(pmv, gpu_ctx_factory):
    ctx = _ctx(pmv, gpu_ctx_factory)
    for slot, img in ((3, _flat()), (2, gc.gradient_frame())):
        h, w = img.shape
        rng = np.random.default_rng(5)
        pts = np.concatenate([sc.edge_points(w, h), (rng.random((40, 2)) * [w, h]).astype(np.float32)])
        for name in ("default", "win1", "win3x7_zero1", "win15_full"):
            xy, it, fl = ctx.corner_subpix(slot, pts, return_info=True, **sc.PARAMS[name])
            assert np.array_equal(sc.bits(xy), sc.bits(pts)) and (it == 0).all() and (fl == sc.DET).all(), (slot, name)


def test_sizes_of_n_and_the_place_of_a_point_in_the_call(pmv, gpu_ctx_factory):
    ctx = _ctx(pmv, gpu_ctx_factory)
    w, h = 160, 120
    pts = np.concatenate([sc.scene_points(pmv, w, h)[:60], sc.edge_points(w, h)])
    want = sc.twin().refine(gc.frame(pmv, w, h), pts)
    before = ctx.debug_subpix_launches()
    xy, it, fl = ctx.corner_subpix(1, np.zeros((0, 2), np.float32), return_info=True)
    assert xy.shape == (0, 2) and it.shape == fl.shape == (0,) and ctx.debug_subpix_launches() == before, "n = 0 launches nothing"
    for n in (1, 3, 4, 5, 257, MAX_TRACKS):
        idx = np.arange(n) % len(pts)
        _same(ctx.corner_subpix(1, pts[idx], return_info=True), [a[idx] for a in want], f"n = {n}")
    assert ctx.debug_subpix_launches() == [before[0] + 6, before[1], before[2]], "one launch per call"
    # a point's bytes are the same alone, first, last and in the middle of a call
    for k in (0, 7, 33, len(pts) - 3):
        others = [i for i in (2, 11, 40, 61) if i != k]
        for idx in ([k], [k] + others[:2], others[:2] + [k], others[:2] + [k] + others[2:], others[:3] + [k]):
            got = ctx.corner_subpix(1, pts[idx], return_info=True)
            _same(got, [a[idx] for a in want], f"point {k} in {idx}")


def _raw(ctx, fn, slot, xy, n, p, iters, flags):
    fn.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    return fn(ctx.h, slot, None if xy is None else xy.ctypes.data, n, None if p is None else C.cast(C.pointer(p), C.c_void_p),
              None if iters is None else iters.ctypes.data, None if flags is None else flags.ctypes.data)


def test_null_outputs_are_accepted(pmv, gpu_ctx_factory):
    ctx = _ctx(pmv, gpu_ctx_factory)
    pts = sc.scene_points(pmv, 160, 120)[:50]
    want = sc.twin().refine(gc.frame(pmv, 160, 120), pts)
    assert np.array_equal(sc.bits(ctx.corner_subpix(1, pts)), sc.bits(want[0]))
    p = pmv.SubpixParams(5, 5, -1, -1, 30, 0.01)
    for null_it, null_fl in ((True, False), (False, True)):
        xy, it, fl = pts.copy(), np.full(50, 77, np.uint8), np.full(50, 77, np.uint8)
        assert _raw(ctx, ctx.lib.pmv_corner_subpix, 1, xy, 50, p, None if null_it else it, None if null_fl else fl) == 0
        assert np.array_equal(sc.bits(xy), sc.bits(want[0]))
        assert (it == 77).all() if null_it else np.array_equal(it, want[1])
        assert (fl == 77).all() if null_fl else np.array_equal(fl, want[2])


def _error_cases(pmv, pts):
    P = pmv.SubpixParams
    nan, inf = float("nan"), float("inf")
    cases = [("null p", INVALID, dict(p=None)), ("null xy", INVALID, dict(null_xy=True))]
    cases += [(f"win {w}", INVALID, dict(p=P(w[0], w[1], -1, -1, 30, 0.01))) for w in ((0, 5), (5, 0), (16, 5), (5, 16), (-1, 5))]
    cases += [(f"max_iter {m}", INVALID, dict(p=P(5, 5, -1, -1, m, 0.01))) for m in (0, 101, -5)]
    cases += [(f"eps {e}", INVALID, dict(p=P(5, 5, -1, -1, 30, e))) for e in (-0.1, nan, inf, -inf)]
    for v in (nan, inf, -inf, 1.5e6, -1.5e6):
        for c in (0, 1):
            bad = pts.copy()
            bad[2, c] = v
            cases.append((f"coordinate {v}", INVALID, dict(xy=bad, names="point 2")))
    cases += [("n above max_tracks", CAPACITY, dict(xy=np.tile(pts, (MAX_TRACKS // len(pts) + 1, 1))[:MAX_TRACKS + 1].copy())),
              ("slot out of range", CAPACITY, dict(slot=8)), ("slot below 0", CAPACITY, dict(slot=-1)), ("a slot without a frame", INVALID, dict(slot=EMPTY_SLOT))]
    return cases


@pytest.mark.parametrize("session", [False, True], ids=["single", "session"])
def test_errors_write_nothing_and_a_valid_call_follows(pmv, gpu_ctx_factory, session):
    ctx = _ctx(pmv, gpu_ctx_factory)
    pts = sc.scene_points(pmv, 160, 120)[:9].copy()
    want = sc.twin().refine(gc.frame(pmv, 160, 120), pts)
    fn = ctx.lib.pmv_batch_corner_subpix if session else ctx.lib.pmv_corner_subpix
    call = ctx.batch_corner_subpix if session else ctx.corner_subpix
    good = pmv.SubpixParams(5, 5, -1, -1, 30, 0.01)
    if session:
        ctx.batch_open(1, [(160, 120)])
    try:
        for what, code, change in _error_cases(pmv, pts):
            xy = change.get("xy", pts).copy()
            keep = xy.copy()
            it, fl = np.full(len(xy), 77, np.uint8), np.full(len(xy), 77, np.uint8)
            rc = _raw(ctx, fn, change.get("slot", 1), None if change.get("null_xy") else xy, len(xy), change.get("p", good) if "p" in change else good, it, fl)
            assert rc == code, f"{what}: status {rc}, expected {code}"
            assert np.array_equal(sc.bits(xy), sc.bits(keep)) and (it == 77).all() and (fl == 77).all(), f"{what}: an output was written"
            if "names" in change:
                msg = (ctx.lib.pmv_thread_error() if session else ctx.lib.pmv_last_error(ctx.h)).decode()
                assert change["names"] in msg, msg
            _same(call(1, pts, return_info=True), want, f"the valid call after '{what}'")
        # a zero zone that is not strictly inside the window, and one that is larger than it, are no errors
        for zero in ((5, 5), (40, 40), (-1, 3), (-7, -7)):
            _same(call(1, pts, zero_zone=zero, return_info=True), want, f"zero zone {zero}")
    finally:
        if session:
            ctx.batch_close()


def test_the_chain_detector_refinement_lk_equals_the_three_twins(pmv, gpu_ctx_factory):
    ctx = _ctx(pmv, gpu_ctx_factory)
    prev, nxt, _ = lx.pair_a(pmv, 160, 120)
    assert np.array_equal(prev, gc.frame(pmv, 160, 120))   # (slot 1 holds `prev`, slot 6 `nxt`)
    cells = pmv.grid_cells(160, 120)
    det = dict(quality=0.02, min_dist=4.0, block_size=5)
    sub = dict(win=(4, 4), zero_zone=(-1, -1), max_iter=20, eps=0.03)
    corners = ctx.detect_gftt_ex(1, cells, 0, **det)   # (160x120 is one grid cell: no limit)
    pts = np.concatenate([d + c[:2] for c, d in zip(cells, corners)]).astype(np.float32)
    refined = ctx.corner_subpix(1, pts, **sub)
    got = ctx.lk_track_ex(1, 6, refined)
    t_pts = np.concatenate([gc.twin().corners(prev, c, 0, **det) + np.asarray(c[:2]) for c in cells]).astype(np.float32)
    t_ref = sc.twin().refine(prev, t_pts, **sub)[0]
    t_lk = lx.twin().track(prev, nxt, t_ref)
    assert np.array_equal(pts, t_pts) and len(pts) > 60
    assert np.array_equal(sc.bits(refined), sc.bits(t_ref)) and (sc.bits(refined) != sc.bits(pts)).any(axis=1).sum() > len(pts) // 4
    ok = t_lk[1] > 0
    assert ok.sum() > 40 and np.array_equal(got[1], t_lk[1])
    assert np.array_equal(sc.bits(got[0])[ok], sc.bits(t_lk[0])[ok]) and np.array_equal(sc.bits(got[2])[ok], sc.bits(t_lk[2])[ok])


def _threads(n, fn):
    errors, start = [], threading.Barrier(n)

    def run(j):
        try:
            start.wait()
            fn(j)
        except Exception as e:   # noqa: BLE001
            errors.append((j, repr(e)))
    th = [threading.Thread(target=run, args=(j,)) for j in range(n)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors, errors


def _session_jobs(pmv):
    """per caller thread: its own slot, its frame size and its points (scene and edge set)"""
    jobs = []
    for slot, size in ((0, (203, 87)), (1, (160, 120)), (4, (203, 87)), (5, (160, 120))):
        pts = np.concatenate([sc.scene_points(pmv, *size)[:100 + 7 * slot], sc.edge_points(*size)])
        jobs.append((slot, size, pts))
    return jobs


@pytest.mark.parametrize("sets", [("default",), ("default", "win3x7_zero1")], ids=["one-parameter-set", "two-parameter-sets"])
def test_sessions(pmv, gpu_ctx_factory, sets):
    """two declared sizes, four caller threads, each on its own slot: every result is the single call's bytes (and the twin's); requests
    that agree in the parameters share a launch whatever their slots and sizes"""
    ctx = _ctx(pmv, gpu_ctx_factory)
    jobs = _session_jobs(pmv)
    reps = 4
    want = {(j, name): ctx.corner_subpix(jobs[j][0], jobs[j][2], return_info=True, **sc.PARAMS[name]) for j in range(4) for name in sets}
    for (j, name), w in want.items():
        if name == "default":
            _same(w, sc.twin().refine(gc.frame(pmv, *jobs[j][1]), jobs[j][2]), f"single call, thread {j}'s points")
    results = [[] for _ in range(4)]
    batch_before = ctx.batch_launches()
    with ctx.batch_session(4, [(160, 120), (203, 87)]):
        c0, d0 = ctx.debug_subpix_launches(), ctx.batch_stats()["det"]

        def run(j):
            for rep in range(reps):
                name = sets[(j + rep) % len(sets)]
                results[j].append((name, ctx.batch_corner_subpix(jobs[j][0], jobs[j][2], return_info=True, **sc.PARAMS[name])))
        _threads(4, run)
        c1, d1 = ctx.debug_subpix_launches(), ctx.batch_stats()["det"]
    for j in range(4):
        assert len(results[j]) == reps
        for name, got in results[j]:
            _same(got, want[j, name], f"thread {j}, {name}")
    rounds, launches = c1[1] - c0[1], c1[2] - c0[2]
    print(f"{len(sets)} parameter set(s): {4 * reps} requests in {rounds} rounds, {launches} launches")
    assert c1[0] == c0[0], "the session form does not count as the single call"
    assert d1["requests"] - d0["requests"] == 4 * reps and rounds == d1["launches"] - d0["launches"], "every detector round of this session held a subpix request"
    assert 1 <= rounds <= 4 * reps
    if len(sets) == 1:
        assert launches == rounds, "requests that agree in the six parameters share ONE launch"
    else:
        assert rounds <= launches <= 2 * rounds
    assert ctx.batch_launches() == batch_before, "pmv_debug_batch_launches counts the LK, matcher and upload legs only, as before"


def test_session_requests_beyond_the_result_block_wait_for_the_next_round(pmv, gpu_ctx_factory):
    """a context of its own with n_seq = 1: a round's result block holds max_tracks = 300 points, so two requests of 300 never share a round"""
    ctx = gpu_ctx_factory(208, 120, n_slots=2, max_tracks=300)
    sizes = [(203, 87), (160, 120)]
    for slot, size in enumerate(sizes):
        ctx.frame_upload(slot, gc.frame(pmv, *size))
    pts = [np.tile(np.concatenate([sc.scene_points(pmv, *sizes[j % 2]), sc.edge_points(*sizes[j % 2])]), (3, 1))[37 * j:37 * j + 300].copy() for j in range(4)]
    want = [ctx.corner_subpix(j % 2, pts[j], return_info=True) for j in range(4)]
    _same(want[1], sc.twin().refine(gc.frame(pmv, 160, 120), pts[1]), "single call at n = max_tracks")
    got = [None] * 4
    with ctx.batch_session(1, sizes):
        c0 = ctx.debug_subpix_launches()

        def run(j):
            got[j] = ctx.batch_corner_subpix(j % 2, pts[j], return_info=True)
        _threads(4, run)
        c1 = ctx.debug_subpix_launches()
    for j in range(4):
        _same(got[j], want[j], f"thread {j}")
    assert (c1[1] - c0[1], c1[2] - c0[2]) == (4, 4)


def test_a_session_without_subpix_calls_leaves_the_counters_at_zero(pmv, gpu_ctx_factory):
    ctx = gpu_ctx_factory(160, 120, n_slots=1, max_tracks=64)
    img = gc.frame(pmv, 160, 120)
    ctx.frame_upload(0, img)
    cells = pmv.grid_cells(160, 120)
    want = ctx.detect_gftt(0, cells, 20)
    with ctx.batch_session(1, [(160, 120)]):
        d0 = ctx.batch_stats()["det"]
        for _ in range(3):
            got = ctx.batch_detect_gftt(0, cells, 20)
            assert all(np.array_equal(g, w) for g, w in zip(got, want))
        d1 = ctx.batch_stats()["det"]
        assert (d1["requests"] - d0["requests"], d1["launches"] - d0["launches"]) == (3, 3), "plain requests one at a time: a round each, as ever"
        assert ctx.debug_subpix_launches() == [0, 0, 0]
    assert ctx.debug_subpix_launches() == [0, 0, 0]
