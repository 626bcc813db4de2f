"""pmv_find_fundamental_mat and its session form on the GPU against the CPU twin (tests/twin/fundamental_twin.cpp, pinned by
tests/test_fundamental_twin.py): found, the F bits, the mask bytes and the samples drawn are the twin's, for every branch of the RANSAC - the
smallest n, the wave-size edges of the scoring loop, an exit inside the first in-kernel round, at a round's last sample and after dozens of
rounds, the 1000-iteration cap, and both getSubset failure branches - whatever the round width R; through a session round shared with
findEssentialMat requests; behind the detector and the forward-backward LK call on a synthetic frame pair."""
import ctypes as C
import threading

import numpy as np
import pytest

import fundamental_common as fc
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
    found, F, mask, drawn = got
    wfound, wF, wmask, wdrawn = want[:4]
    print(f"{what}: twin found={wfound} samples={wdrawn} inliers={int(wmask.sum())} | device found={found} samples={drawn} inliers={int(mask.sum())}")
    assert found == wfound, what
    assert drawn == wdrawn, what
    assert np.array_equal(mask, wmask), what
    if wfound:
        assert np.array_equal(fc.bits(F), fc.bits(wF)), what


@pytest.mark.parametrize("case", fc.CASES, ids=[fc.case_id(c) for c in fc.CASES])
def test_find_fundamental_mat_has_the_twins_bits(gpu_ctx_factory, case):
    key, thr = case
    p1, p2 = fc.points(*key)
    _same(_ctx(gpu_ctx_factory).find_fundamental_mat(p1, p2, threshold=thr), fc.found(key, thr), fc.case_id(case))


def test_every_round_boundary_is_crossed():
    """for the default round width: among the cases above are calls that end inside the first round, exactly at a round's last sample, in
    a later round, at the cap, and without a single sample"""
    R = fc.DEFAULT_R
    drawn = sorted({fc.found(k, t)[3] for k, t in fc.CASES})
    print("samples drawn by the twin over the cases:", drawn)
    assert any(0 < d < R for d in drawn) and any(d > R and d % R for d in drawn) and any(d and d % R == 0 and d < 1000 for d in drawn)
    assert 1000 in drawn and 0 in drawn and any(d > 10 * R for d in drawn)


@pytest.mark.parametrize("R", [1, 8, 32, 64])
def test_the_round_width_does_not_matter(gpu_ctx_factory, R):
    ctx = _ctx(gpu_ctx_factory)
    cases = [(("scene", 1, 15, 0.0), 1.0), (("scene", 2, 65, 0.3), 1.0), (("scene", 7, 63, 0.3), 1.0), (("col40", 1, 100, 0.0), 1.0),
             (("colall", 1, 100, 0.0), 1.0), (("scene", 1, 65, 0.3), 3.0)] + ([(("noise", 5, 40, 0.0), 1.0)] if R > 1 else [])
    assert ctx.lib.pmv_debug_set_fundamental_r(R) == 0
    try:
        for key, thr in cases:
            _same(ctx.find_fundamental_mat(*fc.points(*key), threshold=thr), fc.found(key, thr), f"R={R} {fc.scene_id(key)}")
    finally:
        assert ctx.lib.pmv_debug_set_fundamental_r(0) == 0
    assert ctx.lib.pmv_debug_set_fundamental_r(65) == INVALID and ctx.lib.pmv_debug_set_fundamental_r(-1) == INVALID


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


def test_session_callers_get_the_single_calls_bits_beside_essential_requests(gpu_ctx_factory):
    """four fundamental callers and three essential callers (one slow request of each kind: the 1000-iteration noise scene) start together,
    twice in a row per seq, so that rounds of the five-point combiner hold both kinds - asserted from the combiner's round counters; every
    caller gets its single-call bits"""
    ctx = _ctx(gpu_ctx_factory)
    keys = [("noise", 5, 40, 0.0), ("scene", 1, 65, 0.0), ("scene", 2, 64, 0.3), ("scene", 1, 300, 0.5)]
    for k in keys:
        _same(ctx.find_fundamental_mat(*fc.points(*k)), fc.found(k), f"single {k}")
    ekeys = [("scene", 1, 65, 0.0), ("scene", 2, 64, 0.3), ("noise", 5, 40, 0.0)]
    epts = [tuple(np.ascontiguousarray(p, np.float64) for p in fc.points(*k)) for k in ekeys]
    esingle = [ctx.find_essential_mat(p1, p2, K) for p1, p2 in epts]
    assert all(e[0] for e in esingle)
    start = threading.Barrier(7)

    def rounds():
        out = (C.c_longlong * 3)()
        assert ctx.lib.pmv_debug_whole_rounds(ctx.h, out) == 0
        return list(out)
    before = rounds()

    def chain(j):
        start.wait()
        if j < 4:
            return [ctx.batch_find_fundamental_mat(j, *fc.points(*keys[j])) for _ in range(2)]
        return [ctx.batch_find_essential_mat(j, *epts[j - 4], K) for _ in range(2)]
    with ctx.batch_session(7, [(640, 200)]):
        got = _threads(7, chain)
    fund, ess, both = (a - b for a, b in zip(rounds(), before))
    print(f"whole-RANSAC rounds of the session: {fund} with a fundamental launch, {ess} with an essential launch, {both} with both")
    assert 1 <= fund <= 8 and 1 <= ess <= 6 and both >= 1
    for j in range(4):
        for rep in range(2):
            _same(got[j][rep], fc.found(keys[j]), f"seq {j} call {rep}")
    for j in range(3):
        for rep in range(2):
            found, E, mask, drawn = got[4 + j][rep]
            wfound, wE, wmask, wdrawn = esingle[j]
            assert (found, drawn) == (wfound, wdrawn) and np.array_equal(mask, wmask) and np.array_equal(fc.bits(E), fc.bits(wE)), (j, rep)


def _refused(pmv, code, needles, call):
    with pytest.raises(pmv.PmvError) as e:
        call()
    assert e.value.code == code, e.value
    for s in needles:
        assert s in str(e.value), e.value


def test_session_error_paths(pmv, gpu_ctx_factory):
    ctx = _ctx(gpu_ctx_factory)
    p1, p2 = fc.points("scene", 1, 65, 0.0)
    _refused(pmv, INVALID, ["no batch session is open"], lambda: ctx.batch_find_fundamental_mat(0, p1, p2))
    big = np.zeros((MAX_TRACKS + 1, 2), np.float32)
    with ctx.batch_session(2, [(640, 200)]):
        for seq in (-1, 2):
            _refused(pmv, INVALID, ["seq %d outside 0..1" % seq], lambda: ctx.batch_find_fundamental_mat(seq, p1, p2))
        _refused(pmv, CAPACITY, ["max_tracks=%d" % MAX_TRACKS], lambda: ctx.batch_find_fundamental_mat(1, big, big))
        _refused(pmv, DEGENERATE, ["14 correspondences", "LMedS"], lambda: ctx.batch_find_fundamental_mat(1, p1[:14], p2[:14]))
        _refused(pmv, INVALID, ["confidence"], lambda: ctx.batch_find_fundamental_mat(1, p1, p2, confidence=1.0))
        _same(ctx.batch_find_fundamental_mat(1, p1, p2), fc.found(("scene", 1, 65, 0.0)), "after the refusals")


def test_bad_arguments_return_the_documented_codes_and_leave_the_outputs_untouched(pmv, gpu_ctx_factory):
    ctx = _ctx(gpu_ctx_factory)
    lib = ctx.lib
    n = 20
    p1, p2 = (np.ascontiguousarray(p[:n]) for p in fc.points("scene", 1, 65, 0.0))
    big = np.zeros((MAX_TRACKS + 1, 2), np.float32)

    def bad(i, j, v):
        q = p1.copy()
        q[i, j] = v
        return q

    def find(p1=p1, p2=p2, n=n, thr=1.0, conf=0.99, null=None):
        F, mask = np.full(9, 7.0), np.full(max(n, 1), 9, np.uint8)
        found, drawn = C.c_int(-5), C.c_int(-6)
        a = [ctx.h, p1.ctypes.data_as(_f32p), p2.ctypes.data_as(_f32p), n, C.c_double(thr), C.c_double(conf), F.ctypes.data_as(_f64p),
             mask.ctypes.data_as(_u8p), C.byref(found), C.byref(drawn)]
        if null is not None:
            a[null] = None
        rc = lib.pmv_find_fundamental_mat(*a)
        untouched = (null == 6 or (F == 7.0).all()) and (null == 7 or (mask == 9).all()) and (null == 8 or found.value == -5) and (null == 9 or drawn.value == -6)
        return rc, untouched
    nan, inf = float("nan"), float("inf")
    invalid = [dict(null=i) for i in (1, 2, 6, 7, 8, 9)] + [dict(thr=0.0), dict(thr=-1.0), dict(thr=inf), dict(thr=nan)] + \
              [dict(conf=c) for c in (0.0, 1.0, -0.1, 1.01, nan, inf)] + [dict(p1=bad(3, 1, nan)), dict(p2=bad(19, 0, inf)), dict(p1=bad(0, 0, 1.5e6)), dict(p2=bad(7, 1, -1.5e6))]
    for kw, code in (invalid, INVALID), ([dict(n=-1), dict(p1=big, p2=big, n=MAX_TRACKS + 1)], CAPACITY), ([dict(n=14), dict(n=7), dict(n=0)], DEGENERATE):
        for k in kw:
            assert find(**k) == (code, True), k
    assert find()[0] == 0
    assert lib.pmv_find_fundamental_mat(None, None, None, 0, C.c_double(1.0), C.c_double(0.99), None, None, None, None) == INVALID
    # the messages say why
    _refused(pmv, DEGENERATE, ["14 correspondences", "LMedS"], lambda: ctx.find_fundamental_mat(p1[:14], p2[:14]))
    _refused(pmv, INVALID, ["point 3 of image 1", "not finite"], lambda: ctx.find_fundamental_mat(bad(3, 1, nan), p2))
    _refused(pmv, INVALID, ["point 19 of image 2"], lambda: ctx.find_fundamental_mat(p1, bad(19, 0, inf)))
    # not logged by pmv_record_enable
    ctx.record_enable(True)
    ctx.find_fundamental_mat(p1, p2)
    ctx.record_enable(False)
    assert ctx.records() == []


def test_the_chain_detect_lk_fb_reject_with_f(pmv, gpu_ctx_factory):
    """pmv_detect_gftt -> pmv_lk_track_fb -> pmv_find_fundamental_mat on one synthetic frame pair: five tracks displaced by 20 px across
    their own flow are masked out, and the mask is the twin's on the same float points"""
    w, h = 640, 200
    frames, _ = pmv.synth_sequence(1007, 0, 2, w, h, 370.0, 370.0, 320.0, 100.0, nthreads=4)
    ctx = _ctx(gpu_ctx_factory)
    ctx.frame_upload(0, frames[0])
    ctx.frame_upload(1, frames[1])
    cells = pmv.grid_cells(w, h)
    prev = np.concatenate([d + c[:2] for c, d in zip(cells, ctx.detect_gftt(0, cells, 20))]).astype(np.float32)
    xy, st, _, back, bst, _ = ctx.lk_track_fb(0, 1, prev)
    keep = (st > 0) & (bst > 0) & (np.abs(back - prev).max(1) < 1.0)
    prev, cur = np.ascontiguousarray(prev[keep]), np.ascontiguousarray(xy[keep]).copy()
    n = len(prev)
    assert n >= 30, n
    flow = cur - prev
    moved = np.flatnonzero(np.hypot(flow[:, 0], flow[:, 1]) > 1.0)[:: max(1, n // 6)][:5]
    assert len(moved) == 5
    for i in moved:
        d = flow[i] / np.hypot(*flow[i])
        cur[i] += np.float32(20.0) * np.array([-d[1], d[0]], np.float32)
    found, F, mask, drawn = ctx.find_fundamental_mat(prev, cur)
    want = fc.twin().find(prev, cur)
    print(f"chain: n={n} inliers={int(mask.sum())} samples={drawn}; twin inliers={int(want[2].sum())} samples={want[3]}")
    assert found and not mask[moved].any() and mask.sum() > 0.5 * n
    _same((found, F, mask, drawn), want, "chain")
