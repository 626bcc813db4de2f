"""pmv_find_essential_mat / pmv_recover_pose, their session forms and device_fivepoint = 2 on the GPU, against the host code that the CPU
known-answer tests pin (tests/test_twoview_host.py): found, the E bits, the mask bytes and the sample count are the host's, for every branch
of the RANSAC - no model, the non-RANSAC branch, rejection sampling on tiny n, the wave-size edges of the scoring loop, hundreds of
in-kernel rounds with several niters updates, and the 1000-iteration cap."""
import ctypes as C
import threading

import numpy as np
import pytest

from test_twoview_host import K, _find_essential, _scene

pytestmark = pytest.mark.gpu

_f64p = C.POINTER(C.c_double)
_u8p = C.POINTER(C.c_uint8)
INVALID, CAPACITY = -2, -3
MAX_TRACKS = 1024
_cache = {}


def _ctx(gpu_ctx_factory):
    if "ctx" not in _cache:
        _cache["ctx"] = gpu_ctx_factory(640, 200, n_slots=2, max_tracks=MAX_TRACKS)
    return _cache["ctx"]


def _points(kind, seed, n, f):
    if kind == "noise":   # no geometry at all: integer points uniform in 1200 x 370
        rng = np.random.default_rng(seed)
        return np.floor(rng.uniform(0, [1200, 370], (n, 2))), np.floor(rng.uniform(0, [1200, 370], (n, 2)))
    S = _scene(seed, n, noise_px=0.3, outlier_frac=f, integer=True)
    return S["p1"], S["p2"]


def _host(orc, key):
    """the reference of a scene, computed once: (p1, p2, found, E, mask, drawn)"""
    if key not in _cache:
        p1, p2 = _points(*key)
        _cache[key] = (p1, p2) + _find_essential(orc, p1, p2)
    return _cache[key]


def _same(got, want, what):
    found, E, mask, drawn = got
    wfound, wE, wmask, wdrawn = want
    print(f"{what}: host found={wfound} samples={wdrawn} inliers={int(wmask.sum())} | device found={found} samples={drawn} inliers={int(mask.sum())}")
    assert found == wfound, what
    assert drawn == wdrawn, what
    assert np.array_equal(mask, wmask), what
    if wfound:
        assert np.array_equal(np.ascontiguousarray(E).view(np.uint64), np.ascontiguousarray(wE).view(np.uint64)), what


SCENES = ([("scene", 1, 4, 0.0)] + [("scene", 1, 5, f) for f in (0.0, 0.3, 0.6)] + [("scene", 1, n, f) for n in (6, 8) for f in (0.0, 0.3, 0.6)] +
          [("scene", s, n, f) for n in (63, 64, 65) for s in (1, 2, 3) for f in (0.0, 0.3, 0.6)] + [("scene", s, 300, 0.6) for s in (1, 2, 3)] +
          [("noise", 5, 40, 0.0), ("noise", 5, 200, 0.0)])


@pytest.mark.parametrize("key", SCENES, ids=["%s-seed%d-n%d-f%g" % k for k in SCENES])
def test_find_essential_mat_has_the_hosts_bits(orc, gpu_ctx_factory, key):
    p1, p2, *want = _host(orc, key)
    kind, _, n, f = key
    # the branch each scene is there for
    if n == 4:
        assert not want[0] and want[3] == 0
    elif n == 5:
        assert want[3] == 0 and (not want[0] or want[2].all())
    elif kind == "noise":
        assert want[3] == 1000, "the scene is meant to run into the iteration cap"
    elif f == 0.6 and n >= 63:
        assert want[3] > 200
    _same(_ctx(gpu_ctx_factory).find_essential_mat(p1, p2, K), want, str(key))


def test_every_round_boundary_is_crossed(orc):
    """the in-kernel round holds 8 hypotheses by default: among the scenes above are calls that end inside the first round, exactly at a
    round's last sample and in a later round"""
    drawn = sorted({_host(orc, k)[5] for k in SCENES})
    print("samples drawn by the host over the scenes:", drawn)
    assert any(0 < d < 8 for d in drawn) and any(d > 8 and d % 8 for d in drawn) and any(d and d % 8 == 0 for d in drawn)


def _host_pose(orc, E, p1, p2, mask):
    n = len(p1)
    R, t, tri, m = np.zeros(9), np.zeros(3), np.zeros(4 * n), mask.copy()
    good = orc.lib.orc_host_recover_pose(E.ctypes.data_as(_f64p), p1.ctypes.data_as(_f64p), p2.ctypes.data_as(_f64p), n, K.ctypes.data_as(_f64p),
                                         R.ctypes.data_as(_f64p), t.ctypes.data_as(_f64p), m.ctypes.data_as(_u8p), tri.ctypes.data_as(_f64p))
    return R.reshape(3, 3), t, m, tri.reshape(4, n), good


def _same_pose(got, want, what):
    for a, b, name in zip(got[:4], want[:4], ("R", "t", "mask", "tri")):
        assert a.shape == b.shape and a.tobytes() == b.tobytes(), f"{what}: {name}"
    assert got[4] == want[4], what


@pytest.mark.parametrize("key", [("scene", 1, 65, 0.3), ("scene", 1, 300, 0.6)], ids=["n65", "n300"])
def test_recover_pose_has_the_hosts_bits(orc, gpu_ctx_factory, key):
    ctx = _ctx(gpu_ctx_factory)
    p1, p2 = _points(*key)
    found, E, mask, _ = ctx.find_essential_mat(p1, p2, K)
    assert found
    mask = mask.copy(); mask[::7] = 0
    E = np.ascontiguousarray(E)
    want = _host_pose(orc, E, p1, p2, mask)
    assert want[4] > 0.3 * (1 - key[3]) * key[2]
    _same_pose(ctx.recover_pose(E, p1, p2, K, mask), want, str(key))
    # the DLT of the call is logged as a DLT record, the essential matrix call is not logged
    ctx.record_enable(True)
    ctx.find_essential_mat(p1, p2, K)
    ctx.recover_pose(E, p1, p2, K, mask)
    ctx.record_enable(False)
    recs = ctx.records()
    assert [r["kind"] for r in recs] == ["dlt"]


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


def test_four_threads_of_a_session_get_the_single_calls_bits(orc, gpu_ctx_factory):
    """a slow request (the noise scene: 1000 iterations) and fast ones meet in the rounds; every caller gets its own single-call bits, twice:
    the second call on each seq comes right after the first returned, possibly while the round it left is still running"""
    ctx = _ctx(gpu_ctx_factory)
    keys = [("noise", 5, 40, 0.0), ("scene", 1, 65, 0.0), ("scene", 2, 64, 0.3), ("scene", 1, 300, 0.6)]
    single = []
    for k in keys:
        p1, p2 = _points(*k)
        fe = ctx.find_essential_mat(p1, p2, K)
        _same(fe, _host(orc, k)[2:], f"single {k}")
        m = fe[2].copy(); m[::7] = 0
        single.append((fe, ctx.recover_pose(fe[1], p1, p2, K, m) if fe[0] else None))
    start = threading.Barrier(4)

    def chain(j):
        p1, p2 = _points(*keys[j])
        out = []
        start.wait()
        for _ in range(2):
            fe = ctx.batch_find_essential_mat(j, p1, p2, K)
            m = fe[2].copy(); m[::7] = 0
            out.append((fe, ctx.batch_recover_pose(j, fe[1], p1, p2, K, m) if fe[0] else None))
        return out
    with ctx.batch_session(4, [(640, 200)]):
        got = _threads(4, chain)
    for j in range(4):
        for rep in range(2):
            fe, pose = got[j][rep]
            _same(fe, single[j][0], f"seq {j} call {rep}")
            assert (pose is None) == (single[j][1] is None)
            if pose is not None:
                _same_pose(pose, single[j][1], f"seq {j} call {rep}")


def _refused(pmv, code, needles, call):
    with pytest.raises(pmv.PmvError) as e:
        call()
    assert e.value.code == code, e.value
    for s in needles:
        assert s in str(e.value), e.value


def test_session_error_paths(pmv, gpu_ctx_factory):
    ctx = _ctx(gpu_ctx_factory)
    p1, p2 = _points("scene", 1, 65, 0.0)
    E, m = np.eye(3), np.ones(65, np.uint8)
    for call in (lambda: ctx.batch_find_essential_mat(0, p1, p2, K), lambda: ctx.batch_recover_pose(0, E, p1, p2, K, m)):
        _refused(pmv, INVALID, ["no batch session is open"], call)
    big = np.zeros((MAX_TRACKS + 1, 2))
    with ctx.batch_session(2, [(640, 200)]):
        for seq in (-1, 2):
            _refused(pmv, INVALID, ["seq %d outside 0..1" % seq], lambda: ctx.batch_find_essential_mat(seq, p1, p2, K))
            _refused(pmv, INVALID, ["seq %d outside 0..1" % seq], lambda: ctx.batch_recover_pose(seq, E, p1, p2, K, m))
        _refused(pmv, CAPACITY, ["max_tracks=%d" % MAX_TRACKS], lambda: ctx.batch_find_essential_mat(1, big, big, K))
        _refused(pmv, CAPACITY, ["max_tracks=%d" % MAX_TRACKS], lambda: ctx.batch_recover_pose(1, E, big, big, K, np.ones(MAX_TRACKS + 1, np.uint8)))
        _refused(pmv, INVALID, ["prob"], lambda: ctx.batch_find_essential_mat(1, p1, p2, K, prob=1.5))


def test_bad_arguments_return_the_documented_codes_and_leave_the_outputs_untouched(pmv, gpu_ctx_factory):
    ctx = _ctx(gpu_ctx_factory)
    lib = ctx.lib
    n = 20
    p1, p2 = _points("scene", 1, n, 0.0)
    Kd = np.ascontiguousarray(K)
    big = np.zeros((MAX_TRACKS + 1, 2))

    def find(p1=p1, p2=p2, n=n, Kp=Kd, prob=0.99, thr=1.0, null=None):
        E, mask = np.full(9, 7.0), np.full(max(n, 1), 9, np.uint8)
        found, drawn = C.c_int(-5), C.c_int(-6)
        a = [ctx.h, p1.ctypes.data_as(_f64p), p2.ctypes.data_as(_f64p), n, Kp.ctypes.data_as(_f64p), C.c_double(prob), C.c_double(thr), E.ctypes.data_as(_f64p),
             mask.ctypes.data_as(_u8p), C.byref(found), C.byref(drawn)]
        if null is not None:
            a[null] = None
        rc = lib.pmv_find_essential_mat(*a)
        untouched = (null == 7 or (E == 7.0).all()) and (null == 8 or (mask == 9).all()) and (null == 9 or found.value == -5) and (null == 10 or drawn.value == -6)
        return rc, untouched
    invalid = [dict(null=i) for i in (1, 2, 4, 7, 8, 9, 10)] + [dict(prob=-0.1), dict(prob=1.01), dict(prob=float("nan")), dict(thr=0.0), dict(thr=-1.0),
                                                                dict(thr=float("inf")), dict(thr=float("nan"))]
    for kw, code in (invalid, INVALID), ([dict(n=-1), dict(p1=big, p2=big, n=MAX_TRACKS + 1)], CAPACITY):
        for k in kw:
            assert find(**k) == (code, True), k
    assert find()[0] == 0

    def pose(n=n, null=None, p1=p1, p2=p2):
        E = np.arange(9.0)
        R, t, mask, tri = np.full(9, 7.0), np.full(3, 7.0), np.full(max(n, 1), 9, np.uint8), np.full(4 * max(n, 1), 7.0)
        good = C.c_int(-5)
        a = [ctx.h, E.ctypes.data_as(_f64p), p1.ctypes.data_as(_f64p), p2.ctypes.data_as(_f64p), n, Kd.ctypes.data_as(_f64p), R.ctypes.data_as(_f64p),
             t.ctypes.data_as(_f64p), mask.ctypes.data_as(_u8p), tri.ctypes.data_as(_f64p), C.byref(good)]
        if null is not None:
            a[null] = None
        rc = lib.pmv_recover_pose(*a)
        untouched = (null == 6 or (R == 7.0).all()) and (null == 7 or (t == 7.0).all()) and (null == 8 or (mask == 9).all()) and (null == 9 or (tri == 7.0).all()) and \
            (null == 10 or good.value == -5)
        return rc, untouched
    for i in (1, 2, 3, 5, 6, 7, 8, 9, 10):
        assert pose(null=i) == (INVALID, True), i
    assert pose(n=-1) == (CAPACITY, True) and pose(n=MAX_TRACKS + 1, p1=big, p2=big) == (CAPACITY, True)
    assert lib.pmv_find_essential_mat(None, *([None] * 3), 0, None, C.c_double(0.99), C.c_double(1.0), *([None] * 4)) == INVALID


def test_pipelines_with_the_whole_ransac_on_the_device_equal_the_host_fivepoint(pmv, gpu_ctx_factory):
    """device_fivepoint = 2 against 0: poses, features and the samples drawn, for one sequence and for two through the batch engine"""
    cfg = dict(w=1241, h=376, fx=718.856, fy=718.856, cx=607.1928, cy=185.2157)
    n = 45
    frames, poses = pmv.synth_sequence(1002, 0, n, cfg["w"], cfg["h"], cfg["fx"], cfg["fy"], cfg["cx"], cfg["cy"], nthreads=16)
    Kc = np.array([cfg["fx"], 0, cfg["cx"], 0, cfg["fy"], cfg["cy"], 0, 0, 1.0])
    ctx = gpu_ctx_factory(cfg["w"], cfg["h"], n_slots=2 * n, max_tracks=4096)
    ctx.frames_stage(0, frames); ctx.frames_stage(n, frames)
    a = ctx.pipeline_run(n, cfg["w"], cfg["h"], Kc, poses, threaded=1, n_threads=4)
    assert a.stats["tri_calls"] >= 3

    def same(r, what):
        print(f"{what}: tri_calls={r.stats['tri_calls']} tri_hypotheses={r.stats['tri_hypotheses']} (host {a.stats['tri_hypotheses']})")
        assert np.array_equal(a.poses, r.poses), what
        assert len(a.features) == len(r.features), what
        for x, y in zip(a.features, r.features):
            assert np.array_equal(x, y), what
        assert r.stats["tri_hypotheses"] == a.stats["tri_hypotheses"] and r.stats["tri_calls"] == a.stats["tri_calls"], what
    same(ctx.pipeline_run(n, cfg["w"], cfg["h"], Kc, poses, threaded=1, device_fivepoint=2), "pipeline_run")
    same(ctx.pipeline_run(n, cfg["w"], cfg["h"], Kc, poses, threaded=1, n_threads=4, device_fivepoint=2), "pipeline_run, 4 host threads")
    for j, r in enumerate(ctx.pipeline_run_batch([(0, n, poses), (n, n, poses)], cfg["w"], cfg["h"], Kc, device_fivepoint=2)):
        same(r, f"pipeline_run_batch, sequence {j}")
