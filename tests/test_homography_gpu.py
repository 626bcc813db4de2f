"""pmv_find_homography and its session form on the GPU against the CPU twin (tests/twin/homography_twin.cpp, pinned by
tests/test_homography_twin.py): found, the H bits, the mask bytes, the samples drawn and the best count are the twin's for every scene and
threshold of homography_common.CASES - cv's branch without RANSAC at n = 4, the no-model cases, sizes around the width of a round and of the
refit's partial sums, 300 points through 2000 iterations - for max_iters 1 and 2000; through a session round of three callers; and E and F keep
their bits on a context that has served H calls (the three share staging blocks)."""
import ctypes as C
import threading

import numpy as np
import pytest

import fundamental_common as fc
import homography_common as hc
from test_twoview_host import K

pytestmark = pytest.mark.gpu

_f32p, _f64p, _u8p = C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_uint8)
INVALID, CAPACITY, DEGENERATE = -2, -3, -5
MAX_TRACKS = 1024
_cache = {}


def _ctx(gpu_ctx_factory):
    if "ctx" not in _cache:
        _cache["ctx"] = gpu_ctx_factory(640, 200, n_slots=2, max_tracks=MAX_TRACKS)
    return _cache["ctx"]


def _same(got, want, what):
    found, H, mask, drawn = got
    print(f"{what}: twin found={want['found']} samples={want['drawn']} best count={int(want['mask'].sum())} | device found={found} samples={drawn} "
          f"best count={int(mask.sum())}")
    assert found == want["found"], what
    assert drawn == want["drawn"], what
    assert int(mask.sum()) == int(want["mask"].sum()), what
    assert np.array_equal(mask, want["mask"]), what
    if want["found"]:
        assert np.array_equal(hc.bits(H), hc.bits(want["H"])), (what, H, want["H"])
    else:
        assert not H.any() and not mask.any(), what   # (the binding's zeros: H9 untouched, mask all 0)


@pytest.mark.parametrize("case", hc.CASES, ids=[hc.case_id(c) for c in hc.CASES])
def test_find_homography_has_the_twins_bits(gpu_ctx_factory, case):
    key, thr = case
    _same(_ctx(gpu_ctx_factory).find_homography(*hc.points(*key), threshold=thr), hc.found(key, thr), hc.case_id(case))


def test_four_points_take_the_branch_without_ransac(gpu_ctx_factory):
    found, H, mask, drawn = _ctx(gpu_ctx_factory).find_homography(*hc.points("plane", 1, 4, 0.0))
    assert found and drawn == 0 and mask.tolist() == [1, 1, 1, 1] and H[2, 2] == 1.0
    p1, p2 = hc.points("plane", 1, 4, 0.0)
    assert np.array_equal(hc.bits(H), hc.bits(hc.twin().four_point(p1, p2)))   # no refit behind it


@pytest.mark.parametrize("key", [("tiny", 1, 4, 0.0), ("tiny", 1, 5, 0.0), ("colall", 1, 100, 0.0)], ids=hc.scene_id)
def test_no_model_leaves_h_untouched_and_the_mask_zero(gpu_ctx_factory, key):
    ctx = _ctx(gpu_ctx_factory)
    p1, p2 = hc.points(*key)
    n = len(p1)
    H, mask = np.full(9, 7.0), np.full(n, 9, np.uint8)
    found, drawn = C.c_int(-5), C.c_int(-6)
    rc = ctx.lib.pmv_find_homography(ctx.h, p1.ctypes.data_as(_f32p), p2.ctypes.data_as(_f32p), n, C.c_double(3.0), C.c_double(0.995), 2000, H.ctypes.data_as(_f64p),
                                     mask.ctypes.data_as(_u8p), C.byref(found), C.byref(drawn))
    assert rc == 0 and found.value == 0 and drawn.value == 0 and (H == 7.0).all() and not mask.any()
    assert not hc.found(key)["found"]


@pytest.mark.parametrize("max_iters", [1, 2000])
def test_the_callers_iteration_cap_is_the_loops(gpu_ctx_factory, max_iters):
    ctx = _ctx(gpu_ctx_factory)
    for key, thr in ((("plane", 2, 64, 0.3), 1.0), (("plane", 1, 300, 0.6), 1.0), (("noise", 5, 300, 0.0), 3.0), (("plane", 3, 65, 0.0), 3.0)):
        want = hc.found(key, thr, max_iters=max_iters)
        assert want["drawn"] <= max_iters
        _same(ctx.find_homography(*hc.points(*key), threshold=thr, max_iters=max_iters), want, f"max_iters={max_iters} {hc.scene_id(key)}")
    if max_iters == 2000:
        assert hc.found(("noise", 5, 300, 0.0), 3.0, max_iters=2000)["drawn"] == 2000


def _threads(n, fn):
    res, errors = [None] * n, []

    def run(j):
        try:
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


def _whole_rounds(ctx):
    out = (C.c_longlong * 3)()
    assert ctx.lib.pmv_debug_whole_rounds(ctx.h, out) == 0
    return list(out)


def test_session_callers_get_the_single_calls_bits_in_merged_launches(gpu_ctx_factory):
    """three sequences of 5 / 64 / 300 points issued from three threads, six calls each (the 300-point one runs into the 2000-iteration cap,
    so the others' later calls queue up behind its round): every call has the bits of the single call, the launches are fewer than the
    requests, and the counters of the E / F rounds do not move"""
    ctx = _ctx(gpu_ctx_factory)
    cases = [(("plane", 1, 5, 0.0), 3.0), (("plane", 2, 64, 0.3), 3.0), (("plane", 1, 300, 0.6), 1.0)]
    for key, thr in cases:
        _same(ctx.find_homography(*hc.points(*key), threshold=thr), hc.found(key, thr), f"single {key}")
    reps = 6
    start = threading.Barrier(3)
    before, rounds_before = ctx.homography_launches(), _whole_rounds(ctx)

    def chain(j):
        start.wait()
        key, thr = cases[j]
        return [ctx.batch_find_homography(j, *hc.points(*key), threshold=thr) for _ in range(reps)]
    with ctx.batch_session(3, [(640, 200)]):
        got = _threads(3, chain)
    launches, requests = (a - b for a, b in zip(ctx.homography_launches(), before))
    print(f"homography launches of the session: {launches} for {requests} requests")
    assert requests == 3 * reps and 1 <= launches < requests
    assert _whole_rounds(ctx) == rounds_before
    for j, (key, thr) in enumerate(cases):
        for rep in range(reps):
            _same(got[j][rep], hc.found(key, thr), f"seq {j} call {rep}")


def test_essential_and_fundamental_keep_their_bits_behind_a_homography_call(gpu_ctx_factory):
    ctx = _ctx(gpu_ctx_factory)
    fkey = ("scene", 1, 65, 0.0)
    p1, p2 = fc.points(*fkey)
    e1, e2 = (np.ascontiguousarray(p, np.float64) for p in (p1, p2))
    F_before, E_before = ctx.find_fundamental_mat(p1, p2), ctx.find_essential_mat(e1, e2, K)
    _same(ctx.find_homography(*hc.points("plane", 1, 300, 0.6), threshold=1.0), hc.found(("plane", 1, 300, 0.6), 1.0), "H in between")
    F_after, E_after = ctx.find_fundamental_mat(p1, p2), ctx.find_essential_mat(e1, e2, K)
    for a, b in ((F_before, F_after), (E_before, E_after)):
        assert a[0] and (a[0], a[3]) == (b[0], b[3]) and np.array_equal(a[2], b[2]) and np.array_equal(hc.bits(a[1]), hc.bits(b[1]))
    wfound, wF, wmask, wdrawn, _ = fc.found(fkey)
    assert F_after[0] == wfound and F_after[3] == wdrawn and np.array_equal(F_after[2], wmask) and np.array_equal(fc.bits(F_after[1]), fc.bits(wF))


def _refused(pmv, code, needles, call):
    with pytest.raises(pmv.PmvError) as e:
        call()
    assert e.value.code == code, e.value
    for s in needles:
        assert s in str(e.value), e.value


def test_bad_arguments_are_refused_with_their_reasons(pmv, gpu_ctx_factory):
    ctx = _ctx(gpu_ctx_factory)
    p1, p2 = hc.points("plane", 2, 64, 0.3)
    big = np.zeros((MAX_TRACKS + 1, 2), np.float32)
    bad = p1.copy()
    bad[3, 1] = np.nan
    _refused(pmv, DEGENERATE, ["3 correspondences", "cv asserts"], lambda: ctx.find_homography(p1[:3], p2[:3]))
    _refused(pmv, CAPACITY, ["max_tracks=%d" % MAX_TRACKS], lambda: ctx.find_homography(big, big))
    _refused(pmv, INVALID, ["point 3 of image 1", "not finite"], lambda: ctx.find_homography(bad, p2))
    _refused(pmv, INVALID, ["max_iters = 0"], lambda: ctx.find_homography(p1, p2, max_iters=0))
    _refused(pmv, INVALID, ["threshold"], lambda: ctx.find_homography(p1, p2, threshold=0.0))
    _refused(pmv, INVALID, ["confidence"], lambda: ctx.find_homography(p1, p2, confidence=1.0))
    _refused(pmv, INVALID, ["no batch session is open"], lambda: ctx.batch_find_homography(0, p1, p2))
    with ctx.batch_session(2, [(640, 200)]):
        _refused(pmv, INVALID, ["seq 2 outside 0..1"], lambda: ctx.batch_find_homography(2, p1, p2))
        _refused(pmv, DEGENERATE, ["3 correspondences"], lambda: ctx.batch_find_homography(1, p1[:3], p2[:3]))
        _same(ctx.batch_find_homography(1, p1, p2), hc.found(("plane", 2, 64, 0.3)), "after the refusals")
    # not logged by pmv_record_enable
    ctx.record_enable(True)
    ctx.find_homography(p1, p2)
    ctx.record_enable(False)
    assert ctx.records() == []
