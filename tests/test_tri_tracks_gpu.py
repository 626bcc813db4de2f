"""pmv_triangulate_tracks and its session form on the GPU against the CPU twin (tests/twin/tri_tracks_twin.cpp, pinned by
tests/test_tri_tracks_twin.py): out_xyz, out_status, out_err and out_good are the twin's bit for bit - for landmark counts around one
64-lane workgroup and its tail, 2, 3 and 12 cameras with 0..nc views per landmark, with and without the refinement and the gates, the gate
scene, more cameras than the LDS holds (TT_LDS_CAMS = 64); the two-observation case has the bits of pmv_triangulate_candidates; a context
at its capacities; empty problems launch nothing; a session volley of eight different problems shares one launch, also mixed with
two-view requests; a small call behind a large one has its own bits.

A round is made to form as in tests/test_backend_rounds_gpu.py: the engine of this module's context is created under
PMV_BATCH_LINGER_US = 50 ms and the threads of a volley start behind a barrier."""
import ctypes as C
import os
import threading

import numpy as np
import pytest

import tri_tracks_common as tc

pytestmark = pytest.mark.gpu

_f64p, _u8p, _ip = C.POINTER(C.c_double), C.POINTER(C.c_uint8), C.POINTER(C.c_int)
INVALID, CAPACITY = -2, -3
SIZE = (64, 48)
N = 8


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


@pytest.fixture(scope="module")
def ctx(gpu_ctx_factory):
    return gpu_ctx_factory(*SIZE, n_slots=1, max_tracks=256, max_ba_cams=65, max_ba_points=130, max_ba_obs=2000)


@pytest.fixture(scope="module")
def edge_ctx(gpu_ctx_factory):
    return gpu_ctx_factory(*SIZE, n_slots=1, max_tracks=64, max_ba_cams=12, max_ba_points=130, max_ba_obs=700)


def _same(got, want, what):
    xyz, status, err, good = got
    print(f"{what}: twin good={want['good']} status counts={np.bincount(want['status'], minlength=1).tolist()[:4]} | device good={good}")
    assert want["rc"] == 0, what
    assert np.array_equal(status, want["status"]), (what, status, want["status"])
    assert np.array_equal(tc.bits(xyz), tc.bits(want["xyz"])), (what, np.abs(xyz - want["xyz"]).max())
    assert np.array_equal(tc.bits(err), tc.bits(want["err"])), what
    assert good == want["good"], what


def _single(ctx, sc, p):
    return ctx.triangulate_tracks(sc["P"], sc["obs"], sc["cam"], sc["pt"], sc["n_pts"], p)


def _shape_scene(n_pts, nc):
    return tc.scene(nc, n_pts, 1000 + 13 * nc + n_pts, noise_px=0.5, pixel=(nc == 3))


PARAM_SETS = [("dlt", lambda px: dict(tc.NO_GATES)), ("dlt-defaults", lambda px: None), ("refine5", lambda px: dict(tc.NO_GATES, refine_iters=5)),
              ("dlt-gates", lambda px: tc.gates_on(px)), ("refine5-gates", lambda px: tc.gates_on(px, refine_iters=5, min_views=3))]


@pytest.mark.parametrize("nc", [2, 3, 12])
@pytest.mark.parametrize("n_pts", [1, 63, 64, 65, 130])
def test_the_call_has_the_twins_bits(ctx, n_pts, nc):
    sc = _shape_scene(n_pts, nc)
    assert (sc["views"].min() == 0 and sc["views"].max() == nc) or n_pts == 1
    for name, make in PARAM_SETS:
        p = make(sc["pixel"])
        _same(_single(ctx, sc, p), tc.run(sc, p if p is not None else tc.DEFAULTS), f"np={n_pts} nc={nc} {name}")


def test_the_gate_scene_has_the_twins_bits(ctx):
    sc = tc.gate_scene()
    for it in (0, 5):
        p = dict(tc.GATE_PARAMS, refine_iters=it)
        got = _single(ctx, sc, p)
        _same(got, tc.run(sc, p), f"gate scene, refine_iters={it}")
        assert np.bitwise_or.reduce(got[1]) == 31 and got[3] == 1


def test_more_cameras_than_the_lds_holds_read_them_through_l2(ctx):
    """nc = 65 > TT_LDS_CAMS: the other path of the kernel, with the parallax gate (the centres too)"""
    for nc in (64, 65):
        sc = tc.scene(nc, 70, 4000 + nc, noise_px=0.5, min_v=2)
        keep = slice(0, 2000)   # (the context's max_ba_obs)
        sc = dict(sc, obs=np.ascontiguousarray(sc["obs"][keep]), cam=np.ascontiguousarray(sc["cam"][keep]), pt=np.ascontiguousarray(sc["pt"][keep]))
        assert sc["cam"].max() == nc - 1
        p = tc.gates_on(False, refine_iters=5)
        _same(_single(ctx, sc, p), tc.twin().run(sc["P"], sc["obs"], sc["cam"], sc["pt"], sc["n_pts"], p), f"nc={nc}")


def test_two_views_with_the_first_camera_at_the_origin_have_the_two_view_kernels_bits(ctx):
    n = 65
    scs = [tc.scene(2, n, 20 + k, noise_px=0.5, first_identity=True, min_v=2) for k in range(4)]
    q1, q2 = np.zeros((n, 2)), np.zeros((n, 2))
    for i in range(len(scs[0]["pt"])):
        (q1 if scs[0]["cam"][i] == 0 else q2)[scs[0]["pt"][i]] = scs[0]["obs"][i]
    P1x4 = np.array([s["P"][1] for s in scs])
    Q, _, _ = ctx.triangulate_candidates(q1, q2, P1x4, np.ones(n, np.uint8))
    pt, cam = np.repeat(np.arange(n, dtype=np.int32), 2), np.tile(np.array([0, 1], np.int32), n)
    obs = np.stack([q1, q2], axis=1).reshape(-1, 2)
    for c in range(4):
        P = np.array([np.c_[np.eye(3), np.zeros(3)], P1x4[c]])
        xyz, status, _, _ = ctx.triangulate_tracks(P, obs, cam, pt, n, tc.NO_GATES)
        ok = status == 0
        assert ok.sum() >= n - 2
        assert np.array_equal(tc.bits(xyz[ok]), tc.bits((Q[c][:3] / Q[c][3]).T[ok])), c


def _raw(ctx, sc, n_pts=None, n_obs=None):
    n_pts = sc["n_pts"] if n_pts is None else n_pts
    n_obs = len(sc["obs"]) if n_obs is None else n_obs
    P = np.ascontiguousarray(sc["P"], np.float64)
    xyz, st, err = np.full((n_pts + 1, 3), 7.0), np.full(n_pts + 1, 9, np.uint8), np.full(n_pts + 1, 5.0)
    good = C.c_int(-5)
    rc = ctx.lib.pmv_triangulate_tracks(ctx.h, P.ctypes.data_as(_f64p), len(P), sc["obs"].ctypes.data_as(_f64p), sc["cam"].ctypes.data_as(_ip), sc["pt"].ctypes.data_as(_ip),
                                        n_obs, n_pts, None, xyz.ctypes.data_as(_f64p), st.ctypes.data_as(_u8p), err.ctypes.data_as(_f64p), C.byref(good))
    untouched = (xyz == 7.0).all() and (st == 9).all() and (err == 5.0).all() and good.value == -5
    return rc, bool(untouched), (xyz[:n_pts], st[:n_pts], err[:n_pts], good.value)


def _last_error(ctx):
    return ctx.lib.pmv_last_error(ctx.h).decode()


def _edge_scene():
    sc = tc.scene(12, 130, 77, noise_px=0.5, min_v=3)
    n = len(sc["obs"])
    assert n >= 701
    big = dict(sc, obs=np.ascontiguousarray(sc["obs"][:701]), cam=np.ascontiguousarray(sc["cam"][:701]), pt=np.ascontiguousarray(sc["pt"][:701]))
    at = dict(sc, obs=np.ascontiguousarray(sc["obs"][:700]), cam=np.ascontiguousarray(sc["cam"][:700]), pt=np.ascontiguousarray(sc["pt"][:700]))
    return at, big


def test_a_context_is_served_at_its_capacities_and_refuses_one_more(edge_ctx):
    at, big = _edge_scene()
    assert at["n_pts"] == 130 and len(at["obs"]) == 700 and at["pt"].max() == 129
    for p in (tc.DEFAULTS, tc.gates_on(False, refine_iters=5)):
        _same(_single(edge_ctx, at, p), tc.twin().run(at["P"], at["obs"], at["cam"], at["pt"], 130, p), "np=130 n_obs=700 on caps (12, 130, 700)")
    rc, untouched, _ = _raw(edge_ctx, big)
    assert (rc, untouched) == (CAPACITY, True) and "n_obs=701" in _last_error(edge_ctx)
    rc, untouched, _ = _raw(edge_ctx, at, n_pts=131)
    assert (rc, untouched) == (CAPACITY, True) and "np=131" in _last_error(edge_ctx)
    P13 = dict(at, P=np.concatenate([at["P"], at["P"][:1]]))
    rc, untouched, _ = _raw(edge_ctx, P13)
    assert (rc, untouched) == (CAPACITY, True) and "nc=13" in _last_error(edge_ctx)
    rc, untouched, got = _raw(edge_ctx, at)   # and the context still serves
    assert rc == 0 and not untouched
    _same(got, tc.twin().run(at["P"], at["obs"], at["cam"], at["pt"], 130, tc.DEFAULTS), "after the refusals")


def test_empty_problems_launch_nothing(ctx):
    sc = _shape_scene(65, 3)
    before = ctx.tri_tracks_launches()
    xyz, status, err, good = ctx.triangulate_tracks(sc["P"], sc["obs"][:0], sc["cam"][:0], sc["pt"][:0], 5)
    assert not xyz.any() and (status == tc.FEW_VIEWS).all() and (err == np.inf).all() and good == 0 and len(status) == 5
    xyz, status, err, good = ctx.triangulate_tracks(sc["P"], sc["obs"][:0], sc["cam"][:0], sc["pt"][:0], 0)
    assert xyz.shape == (0, 3) and good == 0
    with ctx.batch_session(2, [SIZE]):
        xyz, status, err, good = ctx.batch_triangulate_tracks(1, sc["P"], sc["obs"][:0], sc["cam"][:0], sc["pt"][:0], 7)
        assert (status == tc.FEW_VIEWS).all() and (err == np.inf).all() and good == 0
    assert ctx.tri_tracks_launches() == before
    _same(_single(ctx, sc, None), tc.run(sc, tc.DEFAULTS), "behind the empty ones")
    assert ctx.tri_tracks_launches() == (before[0] + 1, before[1] + 1)


def _threads(fn, n=N):
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


def _volley_problems():
    shapes = [(1, 3), (63, 3), (64, 12), (65, 2), (130, 12), (130, 3), (64, 3), (65, 12)]
    out = []
    for j, (n_pts, nc) in enumerate(shapes):
        sc = _shape_scene(n_pts, nc)
        assert len(sc["obs"]) > 0   # (an empty problem enters no round)
        out.append((sc, [None, tc.gates_on(sc["pixel"], refine_iters=5), dict(tc.NO_GATES, refine_iters=5), tc.gates_on(sc["pixel"])][j % 4]))
    return out


def test_a_volley_of_session_callers_shares_one_launch_and_each_gets_its_single_calls_bits(ctx):
    probs = _volley_problems()
    singles = [_single(ctx, sc, p) for sc, p in probs]
    for (sc, p), s in zip(probs, singles):
        _same(s, tc.run(sc, p if p is not None else tc.DEFAULTS), "single")
    with ctx.batch_session(N, [SIZE]):
        before, stats = ctx.tri_tracks_launches(), ctx.batch_stats()["dlt"]
        got = _threads(lambda j: ctx.batch_triangulate_tracks(j, probs[j][0]["P"], probs[j][0]["obs"], probs[j][0]["cam"], probs[j][0]["pt"], probs[j][0]["n_pts"], probs[j][1]))
        after, stats2 = ctx.tri_tracks_launches(), ctx.batch_stats()["dlt"]
        launches, requests = after[0] - before[0], after[1] - before[1]
        print(f"k_tri_tracks_batch launches of the volley: {launches} for {requests} requests; dlt rounds {stats2['launches'] - stats['launches']}")
        assert requests == N and 1 <= launches < requests
        assert stats2["requests"] - stats["requests"] == N
        for j in range(N):
            for a, b in zip(got[j][:3], singles[j][:3]):
                assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), j
            assert got[j][3] == singles[j][3]
        # a round that mixes the new kind with two-view requests: each gets its own bits
        n = 65
        tv = tc.scene(2, n, 20, noise_px=0.5, first_identity=True, min_v=2)
        q1, q2 = np.zeros((n, 2)), np.zeros((n, 2))
        for i in range(len(tv["pt"])):
            (q1 if tv["cam"][i] == 0 else q2)[tv["pt"][i]] = tv["obs"][i]
        P1x4 = np.array([tc.scene(2, n, 20 + k, noise_px=0.5, first_identity=True, min_v=2)["P"][1] for k in range(4)])
        mask = np.ones(n, np.uint8)
        mask[::7] = 0

        def mixed(j):
            if j % 2:
                return ctx.batch_triangulate_candidates(j, q1, q2, P1x4, mask)
            return ctx.batch_triangulate_tracks(j, probs[j][0]["P"], probs[j][0]["obs"], probs[j][0]["cam"], probs[j][0]["pt"], probs[j][0]["n_pts"], probs[j][1])
        before, stats = ctx.tri_tracks_launches(), ctx.batch_stats()["dlt"]
        got = _threads(mixed)
        after, stats2 = ctx.tri_tracks_launches(), ctx.batch_stats()["dlt"]
        assert after[1] - before[1] == N // 2 and 1 <= after[0] - before[0] < N // 2
        assert stats2["requests"] - stats["requests"] == N
    Qs, ms, gs = ctx.triangulate_candidates(q1, q2, P1x4, mask)
    for j in range(N):
        if j % 2:
            assert np.array_equal(tc.bits(got[j][0]), tc.bits(Qs)) and np.array_equal(got[j][1], ms) and np.array_equal(got[j][2], gs), j
        else:
            for a, b in zip(got[j][:3], singles[j][:3]):
                assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), j
            assert got[j][3] == singles[j][3]


def test_a_small_call_behind_a_large_one_has_its_own_bits(ctx):
    big, small = _shape_scene(130, 12), _shape_scene(63, 2)
    p = tc.gates_on(False, refine_iters=5)
    _same(_single(ctx, big, p), tc.run(big, p), "the large call")
    _same(_single(ctx, small, p), tc.run(small, p), "the small call behind it")
    _same(_single(ctx, small, None), tc.run(small, tc.DEFAULTS), "and with the defaults")
    with ctx.batch_session(1, [SIZE]):
        _same(ctx.batch_triangulate_tracks(0, big["P"], big["obs"], big["cam"], big["pt"], 130, p), tc.run(big, p), "session, large")
        _same(ctx.batch_triangulate_tracks(0, small["P"], small["obs"], small["cam"], small["pt"], 63, p), tc.run(small, p), "session, small behind it")


def _refused(pmv, code, needles, call):
    with pytest.raises(pmv.PmvError) as e:
        call()
    assert e.value.code == code, e.value
    for s in needles:
        assert s in str(e.value), e.value


def test_bad_arguments_are_refused_with_their_reasons_and_the_call_is_not_logged(pmv, ctx):
    sc = _shape_scene(64, 3)
    bad_cam = sc["cam"].copy()
    bad_cam[5] = 3
    sing = sc["P"].copy()
    sing[1, :, :3] = [[1, 2, 3], [2, 4, 6], [0, 0, 1]]
    a = (sc["obs"], sc["cam"], sc["pt"], 64)
    _refused(pmv, INVALID, ["observation 5"], lambda: ctx.triangulate_tracks(sc["P"], sc["obs"], bad_cam, sc["pt"], 64))
    _refused(pmv, INVALID, ["min_views = 1"], lambda: ctx.triangulate_tracks(sc["P"], *a, dict(min_views=1)))
    _refused(pmv, INVALID, ["refine_iters = 21"], lambda: ctx.triangulate_tracks(sc["P"], *a, dict(refine_iters=21)))
    _refused(pmv, INVALID, ["camera 1 has a singular"], lambda: ctx.triangulate_tracks(sing, *a, dict(min_parallax_deg=1.0)))
    _refused(pmv, CAPACITY, ["np=131"], lambda: ctx.triangulate_tracks(sc["P"], *a[:3], 131))
    _refused(pmv, INVALID, ["no batch session is open"], lambda: ctx.batch_triangulate_tracks(0, sc["P"], *a))
    with ctx.batch_session(2, [SIZE]):
        _refused(pmv, INVALID, ["seq 2 outside 0..1"], lambda: ctx.batch_triangulate_tracks(2, sc["P"], *a))
        _refused(pmv, INVALID, ["observation 5"], lambda: ctx.batch_triangulate_tracks(1, sc["P"], sc["obs"], bad_cam, sc["pt"], 64))
        _same(ctx.batch_triangulate_tracks(1, sc["P"], *a), tc.run(sc, tc.DEFAULTS), "after the refusals")
    _same(ctx.triangulate_tracks(sing, *a), tc.twin().run(sing, sc["obs"], sc["cam"], sc["pt"], 64, tc.DEFAULTS), "a singular camera with the gate off")
    ctx.record_enable(True)
    ctx.triangulate_tracks(sc["P"], *a)
    ctx.record_enable(False)
    assert ctx.records() == []
