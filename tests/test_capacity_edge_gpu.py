"""Every staging block exactly full: a context of max_tracks = 64 with 160x120 frames and BA maxima equal to one problem's sizes, each call at
n = max_tracks (and at its smallest n), through the single call and through a session. A layout that disagrees between the code that carves a
block and the code that sized it shows here, where nothing is left over; every result is compared with the oracle or twin the way the
call's own test compares it, and the session's with the single call's bits.

The rounds that must be full are made to form: for this module the engine's combiners and the session's upload thread run with
PMV_BATCH_LINGER_US = 50 ms, so a round that finds fewer requests than the session has seqs waits that long for the rest, and the threads of a
case start together behind a barrier. That the requests did share a round is then asserted from the launch counters and the rounds' records."""
import ctypes as C
import os
import threading

import numpy as np
import pytest

import clahe_common as cc
import fundamental_common as fc
import gftt_common as gc
import lkx_common as lx
import orc_binding as ob
import remap_common as rc
import scenes
import subpix_common as sc
from test_twoview_host import K as K2, _find_essential, _scene

pytestmark = pytest.mark.gpu

MT, W, H = 64, 160, 120
MAX_HYP, FP_MAX_HYP = 1024, 64
N_SEQ = 2
REF = 7   # the slot reference images are uploaded into
_state = {}


@pytest.fixture(scope="module", autouse=True)
def _lingering_rounds():
    """read by the engine and the session when they are made (every batch_open of this module)"""
    old = os.environ.get("PMV_BATCH_LINGER_US")
    os.environ["PMV_BATCH_LINGER_US"] = "50000"
    yield
    if old is None:
        del os.environ["PMV_BATCH_LINGER_US"]
    else:
        os.environ["PMV_BATCH_LINGER_US"] = old


def _ba():
    if "ba" not in _state:
        P = scenes.ba_problem(3, nc=4, npts=32)
        assert len(P["pts"]) == 32
        _state["ba"] = P
    return _state["ba"]


def _ctx(pmv, gpu_ctx_factory):
    """slots 0, 1: the crop pair of lkx_common; 2: the detector frame; 3..6: the upload round; REF"""
    if "ctx" not in _state:
        P = _ba()
        ctx = gpu_ctx_factory(W, H, n_slots=8, max_tracks=MT, max_ba_cams=4, max_ba_points=32, max_ba_obs=len(P["obs"]))
        prev, nxt, _, _ = lx.crop(pmv, W, H)
        for slot, img in enumerate((prev, nxt, gc.frame(pmv, W, H))):
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


def _session_pair(ctx, call):
    """call(seq) from N_SEQ threads of one session"""
    with ctx.batch_session(N_SEQ, [(W, H)]):
        return _threads(N_SEQ, call)


def _same_bits(got, want, what):
    for k, (g, r) in enumerate(zip(got, want)):
        g, r = np.ascontiguousarray(g), np.ascontiguousarray(r)
        assert g.shape == r.shape and g.tobytes() == r.tobytes(), f"{what}: output {k} differs"


@pytest.mark.parametrize("m, iterations", [(MT, MAX_HYP), (6, MAX_HYP), (6, 1)], ids=["m64-it1024", "m6-it1024", "m6-it1"])
def test_pnp_ransac(pmv, gpu_ctx_factory, m, iterations):
    ctx = _ctx(pmv, gpu_ctx_factory)
    P = scenes.pnp_problem(5, m=m, outlier_frac=0.2 if m == MT else 0.0)
    guess_r, guess_t = np.array([0.3, -0.2, 0.1]), np.array([1.0, 2.0, -30.0])
    rv, tv, inl = ctx.pnp_ransac(P["obj"], P["img"], scenes.K, guess_r, guess_t, iterations=iterations)
    rr, rt, rinl, _ = ob.pnp_ransac(P["obj"], P["img"], scenes.K, guess_r, guess_t, iterations=iterations)
    print(f"m={m} iterations={iterations}: {len(rinl)} inliers in the oracle, {len(inl)} on the device")
    assert np.array_equal(inl, rinl), "inlier index list differs"
    np.testing.assert_allclose(rv, rr, rtol=1e-6, atol=1e-8)
    np.testing.assert_allclose(tv, rt, rtol=1e-6, atol=1e-8)
    for got in _session_pair(ctx, lambda j: ctx.batch_pnp_ransac(j, P["obj"], P["img"], scenes.K, guess_r, guess_t, iterations=iterations)):
        _same_bits(got, (rv, tv, inl), "session PnP")


@pytest.mark.parametrize("n", [MT, 1])
def test_triangulate_candidates(pmv, gpu_ctx_factory, n):
    ctx = _ctx(pmv, gpu_ctx_factory)
    P = scenes.two_view_problem(2, n=n)
    got = ctx.triangulate_candidates(P["q1"], P["q2"], P["P1x4"], P["mask"])
    want = ob.triangulate_candidates(P["q1"], P["q2"], P["P1x4"], P["mask"])
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
    for s in _session_pair(ctx, lambda j: ctx.batch_triangulate_candidates(j, P["q1"], P["q2"], P["P1x4"], P["mask"])):
        _same_bits(s, got, "session DLT")


@pytest.mark.parametrize("n, nh", [(MT, FP_MAX_HYP), (5, 1)], ids=["n64-h64", "n5-h1"])
def test_fivepoint_hypotheses(pmv, orc, gpu_ctx_factory, n, nh):
    """the scene and the comparison of tests/test_backend_gpu.py's five-point test"""
    ctx = _ctx(pmv, gpu_ctx_factory)
    rng = np.random.default_rng(12)
    X = np.stack([rng.uniform(-8, 8, n), rng.uniform(-3, 2, n), rng.uniform(5, 40, n)], 1)
    rv = rng.normal(0, 0.03, 3); th = np.linalg.norm(rv); k = rv / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    R = np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx
    t = np.array([0.08, -0.03, -1.0]); t /= np.linalg.norm(t)
    Xc = X @ R.T + t
    f = 718.856
    q1 = np.floor(X[:, :2] / X[:, 2:3] * f + rng.normal(0, 0.3, (n, 2))) / f
    q2 = np.floor(Xc[:, :2] / Xc[:, 2:3] * f + rng.normal(0, 0.3, (n, 2))) / f
    q2[::7] += rng.normal(0, 0.05, q2[::7].shape)
    samples = np.zeros((nh, 5), np.int32)
    orc.lib.orc_host_five_point_samples(n, nh, samples.ctypes.data_as(C.POINTER(C.c_int)))
    thr = np.float32((1.0 / f) ** 2)
    models, nm, counts = ctx.fivepoint_hypotheses(q1, q2, samples, thr)
    f64p = C.POINTER(C.c_double)
    x1 = np.concatenate([q1, np.ones((n, 1))], 1); x2 = np.concatenate([q2, np.ones((n, 1))], 1)
    total = 0
    for h in range(nh):
        Es = np.zeros(90)
        s1 = np.ascontiguousarray(q1[samples[h]]); s2 = np.ascontiguousarray(q2[samples[h]])
        want = orc.lib.orc_host_five_point(s1.ctypes.data_as(f64p), s2.ctypes.data_as(f64p), Es.ctypes.data_as(f64p))
        assert nm[h] == want, f"hypothesis {h}: {nm[h]} models on the device, {want} on the host"
        assert np.array_equal(models[h].reshape(90)[: 9 * want], Es[: 9 * want]), f"hypothesis {h}: models are not bit-exact"
        for mi in range(want):
            E = Es[9 * mi: 9 * mi + 9].reshape(3, 3)
            Ex1 = x1 @ E.T; Etx2 = x2 @ E
            err = ((x2 * Ex1).sum(1) ** 2 / (Ex1[:, 0] ** 2 + Ex1[:, 1] ** 2 + Etx2[:, 0] ** 2 + Etx2[:, 1] ** 2)).astype(np.float32)
            sure_in = int((err <= thr * np.float32(1 - 1e-6)).sum()); sure_out = int((err > thr * np.float32(1 + 1e-6)).sum())
            assert sure_in <= counts[h, mi] <= n - sure_out
        total += want
    print(f"n={n} n_hyp={nh}: {total} models")
    assert total >= 1
    for s in _session_pair(ctx, lambda j: ctx.batch_fivepoint_hypotheses(j, q1, q2, samples, thr)):
        _same_bits(s, (models, nm, counts), "session five-point round")


def _same_whole(got, want, what):
    found, M, mask, drawn = got
    wfound, wM, wmask, wdrawn = want[:4]
    print(f"{what}: reference found={wfound} samples={wdrawn} inliers={int(wmask.sum())} | device found={found} samples={drawn} inliers={int(mask.sum())}")
    assert found == wfound and drawn == wdrawn and np.array_equal(mask, wmask), what
    if wfound:
        assert np.array_equal(fc.bits(M), fc.bits(wM)), what


@pytest.mark.parametrize("n", [MT, 5])
def test_find_essential_mat(pmv, orc, gpu_ctx_factory, n):
    ctx = _ctx(pmv, gpu_ctx_factory)
    S = _scene(1, n, noise_px=0.3, outlier_frac=0.3 if n == MT else 0.0, integer=True)
    want = _find_essential(orc, S["p1"], S["p2"])
    got = ctx.find_essential_mat(S["p1"], S["p2"], K2)
    _same_whole(got, want, f"essential n={n}")
    for s in _session_pair(ctx, lambda j: ctx.batch_find_essential_mat(j, S["p1"], S["p2"], K2)):
        _same_whole(s, want, f"session essential n={n}")


@pytest.mark.parametrize("n", [MT, 15])
def test_find_fundamental_mat(pmv, gpu_ctx_factory, n):
    ctx = _ctx(pmv, gpu_ctx_factory)
    key = ("scene", 1, n, 0.3 if n == MT else 0.0)
    p1, p2 = fc.points(*key)
    want = fc.found(key)
    _same_whole(ctx.find_fundamental_mat(p1, p2), want, f"fundamental n={n}")
    for s in _session_pair(ctx, lambda j: ctx.batch_find_fundamental_mat(j, p1, p2)):
        _same_whole(s, want, f"session fundamental n={n}")


def test_corner_subpix(pmv, gpu_ctx_factory):
    ctx = _ctx(pmv, gpu_ctx_factory)
    pts = sc.scene_points(pmv, W, H)[:MT]
    assert len(pts) == MT
    rxy, rit, rfl, _ = sc.twin().refine(gc.frame(pmv, W, H), pts)
    assert (sc.bits(rxy) != sc.bits(pts)).any(axis=1).sum() >= MT // 8, "the scene moves too few points to compare anything"

    def same(got, what):
        xy, it, fl = got
        assert np.array_equal(sc.bits(xy), sc.bits(rxy)) and np.array_equal(it, rit) and np.array_equal(fl, rfl), what
    same(ctx.corner_subpix(2, pts, return_info=True), "single call")
    before = ctx.debug_subpix_launches()
    for s in _session_pair(ctx, lambda j: ctx.batch_corner_subpix(2, pts, return_info=True)):
        same(s, "session")
    after = ctx.debug_subpix_launches()
    # [single-call launches, session rounds with such requests, their launches]: ONE round of N_SEQ x 64 points in ONE launch - the block was full
    assert [a - b for a, b in zip(after, before)] == [0, 1, 1], (before, after)


def test_lk_track_fb(pmv, gpu_ctx_factory):
    """the comparison of tests/test_lkx_gpu.py's back check: status as the twin's, positions and errors bit for bit where the twin tracks"""
    ctx = _ctx(pmv, gpu_ctx_factory)
    prev, nxt, pts, init = lx.crop(pmv, W, H)
    pts, init = pts[:MT], init[:MT]
    want = lx.twin().track_fb(prev, nxt, pts, init=init)
    got = ctx.lk_track_fb(0, 1, pts, init_xy=init)
    ok, both = want[1] > 0, want[4] > 0
    print(f"{int(ok.sum())} of {MT} tracked forward by the twin, {int(both.sum())} back")
    assert int(both.sum()) >= MT // 4, "the scene tracks too few points to compare anything"
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[4], want[4]), "status differs from the twin"
    assert np.array_equal(lx.bits(got[0])[ok], lx.bits(want[0])[ok]) and np.array_equal(lx.bits(got[2])[ok], lx.bits(want[2])[ok])
    assert np.array_equal(lx.bits(got[3])[both], lx.bits(want[3])[both]) and np.array_equal(lx.bits(got[5])[both], lx.bits(want[5])[both])
    # a session round of N_SEQ x 64 forward-backward tracks: the round's back block is full
    l0 = ctx.batch_launches()["k_lk_batch"]
    for s in _session_pair(ctx, lambda j: ctx.batch_lk_track_fb(0, 1, pts, init_xy=init)):
        _same_bits(s, got, "session lk_track_fb")
    assert ctx.batch_launches()["k_lk_batch"] - l0 == 1, "the two requests did not share a launch: the back block was never full"


def _levels(ctx, slot):
    return [ctx.get_level_padded(slot, l, W, H) for l in range(ctx.num_levels(slot) + 1)]


def test_upload_round_with_all_four_kinds(pmv, gpu_ctx_factory):
    """a gray, a BGR, a CLAHE and a remap upload in ONE round - a round makes one level-0 launch per kind it holds, so its record shows four -
    and every slot holds the bytes of the single-call path"""
    ctx = _ctx(pmv, gpu_ctx_factory)
    img = rc.image(pmv, W, H)
    bgr = np.ascontiguousarray(np.stack([img, np.roll(img, 3, axis=1), np.roll(img, 2, axis=0)], axis=2))
    clahe = (3.0, (4, 3))
    mid = ctx.remap_map_create(*rc.maps(pmv, "undistort06", W, H))
    ctx.frame_upload_bgr(REF, bgr)
    wants = {1: _levels(ctx, REF)}   # by kind: 0 gray, 1 BGR, 2 CLAHE, 3 remap
    for k, ref in ((0, img), (2, cc.twin().apply(img, *clahe)[0]), (3, rc.remapped(pmv, ("undistort06", W, H, 200))[0])):
        ctx.frame_upload(REF, ref)
        wants[k] = _levels(ctx, REF)
    kinds = [lambda s: ctx.batch_frame_upload(s, img), lambda s: ctx.batch_frame_upload(s, bgr, "bgr"),
             lambda s: ctx.batch_frame_upload(s, img, "gray", clahe=clahe), lambda s: ctx.batch_frame_upload_remap(s, img, (mid, 200))]
    with ctx.batch_session(4, [(W, H)]):
        _threads(4, lambda j: kinds[j](3 + j))
        st, rounds = ctx.batch_upload_stats(), ctx.batch_upload_rounds()
    print(f"four uploads: {st}; rounds {rounds}")
    assert st["frames"] == 4
    assert any(sum(r["frames_by_levels"]) == 4 and r["level0_launches"] == 4 for r in rounds), "no round held all four kinds: not all seven tables were in use at once"
    for k in range(4):
        got = _levels(ctx, 3 + k)
        assert len(got) == len(wants[k])
        for l, (a, b) in enumerate(zip(got, wants[k])):
            assert a.shape == b.shape and np.array_equal(a, b), f"slot {3 + k} level {l} differs in {int((a != b).sum())} bytes"


def test_ba_solve_at_the_contexts_maxima(pmv, gpu_ctx_factory):
    """the comparison of tests/test_backend_gpu.py::test_ba_solve_matches_oracle at nc, np, n_obs = max_ba_cams, max_ba_points, max_ba_obs"""
    ctx = _ctx(pmv, gpu_ctx_factory)
    P = _ba()
    cams, pts, s = ctx.ba_solve(P["cams"], P["pts"], P["obs"], P["cam_idx"], P["pt_idx"], scenes.K, 1.0, 5)
    rc_, rp, rs = ob.ba_solve(P["cams"], P["pts"], P["obs"], P["cam_idx"], P["pt_idx"], scenes.K, 1.0, 5)
    print(f"nc=4 np=32 n_obs={len(P['obs'])}: cost {s.initial_cost} -> {s.final_cost} in {s.iterations} iterations (oracle {rs['final_cost']})")
    np.testing.assert_allclose(s.initial_cost, rs["initial_cost"], rtol=1e-12)
    assert s.iterations == rs["iterations"] and s.successful_steps == rs["successful_steps"] and s.termination == rs["termination"]
    np.testing.assert_allclose(s.final_cost, rs["final_cost"], rtol=1e-8)
    np.testing.assert_allclose(cams, rc_, rtol=1e-6, atol=1e-8)
    np.testing.assert_allclose(pts, rp, rtol=1e-6, atol=1e-6)
    for c2, p2, s2 in _session_pair(ctx, lambda j: ctx.batch_ba_solve(j, P["cams"], P["pts"], P["obs"], P["cam_idx"], P["pt_idx"], scenes.K, 1.0, 5)):
        _same_bits((c2, p2), (cams, pts), "session BA")
        assert (s2.initial_cost, s2.final_cost, s2.iterations, s2.successful_steps) == (s.initial_cost, s.final_cost, s.iterations, s.successful_steps)
