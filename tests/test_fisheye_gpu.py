"""The equidistant (cv::fisheye) camera model on the device: pmv_undistort_points and pmv_project_points through a fisheye camera equal the CPU
twin (tests/twin/fisheye_twin.cpp) bit for bit - xy as uint32, ok as bytes; sixteen cameras of mixed models share the one table; the tracker
step with a fisheye camera (observations, undistorted_f, a prediction) equals the composition of the single calls on the device and the
twin's stage-9 and stage-3 rules, at the launch counts of the same step with a radial-tangential camera; and the maps of
pmv_fisheye_map_build drive pmv_frames_remap."""
import ctypes as C

import numpy as np
import pytest

import fisheye_common as fc
import fundamental_common as fm
import gftt_common as gc
import klt_common as kc
import klt_observe_common as ko
import klt_stereo_common as ks
import lift_common as lf
import predict_common as pc
import remap_common as rm

pytestmark = pytest.mark.gpu
INVALID, CAPACITY = -2, -3
W, H = fc.TUMVI_SIZE
MAX_TRACKS = 2048
SIZES = (0, 1, 63, 64, 65, 257, 1025)   # the sizes of tests/test_undistort_points_gpu.py
STEREO = ks.STEREO["fb"]


@pytest.fixture(scope="module")
def ctx(gpu_ctx_factory):
    return gpu_ctx_factory(W, H, n_slots=2, max_tracks=MAX_TRACKS)


@pytest.mark.parametrize("name,cam", fc.CAMERAS, ids=[n for n, _ in fc.CAMERAS])
def test_the_lift_equals_the_twin(ctx, name, cam):
    cid = fc.create(ctx, cam)
    try:
        for n in SIZES:
            xy = fc.lift_points(cam, (W, H), n, seed=n + 1)[:n] if n < 5 else fc.lift_points(cam, (W, H), n - 4, seed=n + 1)
            got = ctx.undistort_points(cid, xy)
            assert got[0].shape == (n, 2) and got[1].shape == (n,)
            fc.same(got, fc.twin().points(cam, xy), ("un_xy", "ok"))
            assert not np.isnan(got[0]).any()
            if n >= 63:
                assert got[1][n - 4] == 1 and (name == "refusing" or got[1][:n - 4].sum() > (n - 4) // 2)
                if name != "tumvi":   # (cx and cy are float32 numbers: theta_d is 0)
                    assert not fc.bits(got[0])[n - 4].any(), "the principal point"
        un, ok = ctx.undistort_points(cid, np.asarray([fc.REFUSED_POINT], np.float32))
        if name == "refusing":
            assert ok[0] == 0 and not fc.bits(un).any(), "the refused point: ok 0 and (0, 0)"
    finally:
        ctx.camera_destroy(cid)


@pytest.mark.parametrize("name,cam", fc.CAMERAS, ids=[n for n, _ in fc.CAMERAS])
def test_the_projection_equals_the_twin(ctx, name, cam):
    cid = fc.create(ctx, cam)
    try:
        for n in SIZES:
            xyz = fc.project_points(n, seed=n + 3)[:n] if n < 8 else fc.project_points(n - 7, seed=n + 3)
            got = ctx.project_points(cid, xyz)
            assert got[0].shape == (n, 2) and got[1].shape == (n,)
            fc.same(got, fc.twin().project(cam, xyz), ("xy", "ok"))
            assert not np.isnan(got[0]).any()
            if n >= 63:
                assert got[1][n - 7:].tolist() == [0, 0, 0, 0, 1, 1, 1], "Z = 0, Z < 0, NaN, an infinity; on the axis, r = 1e-9, 89.9 degrees"
                assert got[0][n - 3].tolist() == [np.float32(cam["cx"]), np.float32(cam["cy"])]
    finally:
        ctx.camera_destroy(cid)


def test_the_constructor_refuses_and_writes_nothing(pmv, ctx):
    base = dict(fx=190.97, fy=190.97, cx=254.93, cy=256.90, k=(0.003482, 0.000715, -0.002053, 0.000202))
    nan, inf = float("nan"), float("inf")
    for kw, text in ((dict(fx=0.0), "fx"), (dict(fy=0.0), "fy"), (dict(fx=nan), "fx"), (dict(fy=inf), "fy"), (dict(cx=nan), "cx"), (dict(cy=-inf), "cy"),
                     (dict(k=(0.1, 0.0, nan)), "k[2]"), (dict(k=(0, 0, 0, inf)), "k[3]"), (dict(k=(-inf,)), "k[0]"), (dict(fx=5e-324), "1 / fx")):
        with pytest.raises(pmv.PmvError) as e:
            ctx.camera_create_fisheye(**dict(base, **kw))
        assert e.value.code == INVALID and text in str(e.value) and "pmv_camera_create_fisheye" in str(e.value), (kw, str(e.value))
    fn = ctx.lib.pmv_camera_create_fisheye
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    p, out = pmv.fisheye_params(**base), C.c_int(-7)
    assert fn(ctx.h, None, C.addressof(out)) == INVALID and out.value == -7
    assert fn(ctx.h, C.addressof(p), None) == INVALID


def test_sixteen_cameras_of_mixed_models(pmv, ctx):
    start = pmv.mem_live()
    cams = []
    for k in range(16):
        if k % 2:
            cams.append(dict(lf.all_terms(W, H), fx=300.0 + 7 * k, iters=1 + k))
        else:
            cams.append(dict(fc.ALL_K, fx=180.0 + 5 * k, k=(-0.05 + 0.004 * k, 0.02, -0.01, 0.003 - 0.0002 * k)))
    ids = [fc.create(ctx, c) for c in cams]
    assert sorted(ids) == list(range(16))
    assert pmv.mem_live()[0] > start[0], "the cameras live in a device table"
    for make in (lambda: fc.create(ctx, cams[0]), lambda: fc.create(ctx, cams[1])):
        with pytest.raises(pmv.PmvError) as e:
            make()
        assert e.value.code == CAPACITY and "16 cameras" in str(e.value)
    xy, xyz = fc.lift_points(fc.ALL_K, (W, H), 61, seed=5), fc.project_points(58, seed=6)
    for k in range(16):   # every entry of the table answers as its own twin
        fc.same(ctx.undistort_points(ids[k], xy), fc.twin().points(cams[k], xy), ("un_xy", "ok"))
        fc.same(ctx.project_points(ids[k], xyz), fc.twin().project(cams[k], xyz), ("xy", "ok"))
    # the twin's radial-tangential half is the yardstick of the older tests
    fc.same(fc.twin().points(cams[1], xy), lf.twin().points(cams[1], xy), ("un_xy", "ok"))
    fc.same(fc.twin().project(cams[1], xyz), pc.project_twin().points(cams[1], xyz), ("xy", "ok"))
    # a freed fisheye id is handed out again as a radial-tangential camera
    assert fc.is_fisheye(cams[4])
    ctx.camera_destroy(ids[4])
    again = ctx.camera_create(**lf.EUROC)
    assert again == ids[4]
    fc.same(ctx.undistort_points(again, xy), lf.twin().points(lf.EUROC, xy), ("un_xy", "ok"))
    fc.same(ctx.project_points(again, xyz), pc.project_twin().points(lf.EUROC, xyz), ("xy", "ok"))
    for i in ids:
        ctx.camera_destroy(i)
    assert pmv.mem_live() == start


# ---- the tracker --------------------------------------------------------------------------------------------------------------------------
def _expected(cams, o, out, right):
    rcam = o.get("rcam", -1)
    if right is not None and rcam >= 0:
        return fc.twin().observe(cams[o["cam"]], o["dt"], out[1], out[2], out[3], cams[rcam], right[0], right[1])
    return fc.twin().observe(cams[o["cam"]], o["dt"], out[1], out[2], out[3])


def _check_observations(ctx, trk, o, cams, out, right_on):
    """the twin's stage-9 rule on the step's outputs, and the composition of the single calls on the device: step, then pmv_undistort_points"""
    rcam = o.get("rcam", -1)
    right = (out[5], out[6]) if right_on and rcam >= 0 else None
    got = trk.get_observations()
    fc.same(got, _expected(cams, o, out, right), ko.NAMES)
    n = len(out[0])
    if n:
        un, ok = ctx.undistort_points(o["cam"], out[2])
        pun, pok = ctx.undistort_points(o["cam"], out[3])
        fc.same((got[0], got[2]), (un, ok), ("un_xy", "ok"))
        moving = (out[1] > 1) & (ok == 1) & (pok == 1)
        vel = np.zeros((n, 2), np.float32)
        vel[moving] = ((un[moving] - pun[moving]).astype(np.float64) / o["dt"]).astype(np.float32)
        assert np.array_equal(fc.bits(got[1]), fc.bits(vel)), "vel differ from the composition"
    if right is not None and n:
        run, rok = ctx.undistort_points(rcam, out[5])
        assert np.array_equal(fc.bits(got[3]), fc.bits(run)) and np.array_equal(got[4], rok & out[6])
    return got


def _drive(ctx, form, plist, olist, cams, n_steps, nl=kc.N_FRAMES):
    """trackers with the observation settings of olist and trackers without any over the same frames: the step's own outputs do not depend on
    the setting, and the observations are checked every step"""
    k = len(plist)
    on, off = [ctx.klt_create(**p) for p in plist], [ctx.klt_create(**p) for p in plist]
    for t, o in zip(on, olist):
        t.set_observe(o["cam"], o.get("rcam", -1), o["dt"])
    if "stereo" in form:
        for t in on + off:
            t.set_stereo(**STEREO)
    outs = []
    for i in range(n_steps):
        ps, cs = max(i - 1, 0), i

        def step(trks):
            if form == "single":
                return [trks[0].step(ps, cs)]
            if form == "stereo":
                return [trks[0].step_stereo(ps, cs, nl + i)]
            return ctx.klt_step_many(trks, [ps] * k, [cs] * k)

        got, want = step(on), step(off)
        for j in range(k):
            try:
                kc.same(got[j][:5], want[j][:5])
                if len(got[j]) > 5:
                    ks.same_right(got[j][5:], want[j][5:])
                _check_observations(ctx, on[j], olist[j], cams, got[j], form == "stereo")
            except AssertionError as e:
                raise AssertionError(f"step {i}, tracker {j}: {e}") from None
        outs.append(got)
    for t in on + off:
        t.close()
    return outs


def _make(gpu_ctx_factory, pmv, w, h, stereo, cam_list):
    lefts = kc.scene(pmv, w, h)
    if stereo:
        ctx = ks.make_ctx(gpu_ctx_factory, lefts, ks.scene_rights(pmv, w, h), max_tracks=MAX_TRACKS)
    else:
        ctx = gpu_ctx_factory(w, h, n_slots=len(lefts), max_tracks=MAX_TRACKS)
        kc.upload(ctx, lefts)
    cams = {}
    for cam in cam_list:
        cams[fc.create(ctx, cam)] = cam
    return ctx, cams


@pytest.mark.parametrize("size", kc.SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("form", ["single", "stereo", "many"])
def test_observations_through_a_fisheye_camera(pmv, gpu_ctx_factory, size, form):
    """a single step; the stereo form with a radial-tangential right camera; a group of three of which one has a radial-tangential camera and
    two have different fisheye cameras"""
    w, h = size
    fish, fish2, radtan = fc.scene_fisheye(w, h), fc.scene_fisheye(w, h, k=(0.05, -0.01, 0.002, 0.0), fx=0.5 * w), ko.right_camera(w, h)
    ctx, cams = _make(gpu_ctx_factory, pmv, w, h, form == "stereo", [fish, fish2, radtan])
    a, b, r = sorted(cams)
    p = kc.params()
    if form == "many":
        plist = [p, dict(p, target=64), dict(p, target=65)]
        olist = [dict(cam=a, dt=ko.DT), dict(cam=r, dt=ko.DT), dict(cam=b, dt=2 * ko.DT)]
    else:
        plist, olist = [p], [dict(cam=a, rcam=r, dt=ko.DT)]
    outs = _drive(ctx, form, plist, olist, cams, kc.N_FRAMES)
    assert all(len(o[0][0]) > 0 for o in outs) and any((o[0][1] > 1).any() for o in outs[1:]), "no survivor ever had a velocity to compute"
    if form == "stereo":
        assert all(o[0][6].any() for o in outs)


class _FisheyeLiftedOps(kc.TwinOps):
    """klt_common's twin stages with stage 3 on the virtual-camera points of a camera of either model (klt_observe_common.LiftedTwinOps' rule,
    through the fisheye twin)"""
    def __init__(self, prev, cur, cam, f_focal):
        super().__init__(prev, cur)
        self.cam, self.f_focal = cam, f_focal

    def fundamental(self, p1, p2, thr, conf):
        q1, q2 = fc.twin().f_points(self.cam, self.f_focal, self.w, self.h, p1, p2)
        found, _, mask, drawn, _ = fm.twin().find(q1, q2, thr, conf)
        return found, mask, drawn


def _lifted_run(frames, p, cam, f_focal, key):
    def make():
        s, out = kc.empty_state(), []
        for i in range(len(frames)):
            s, o = kc.compose(_FisheyeLiftedOps(frames[max(i - 1, 0)], frames[i], cam, f_focal), s, p)
            out.append((s, o))
        return out
    return gc.cached(("fisheye-lifted-run", key), make)


def _per_step(trk, n, stats):
    out = []
    for i in range(n):
        s0 = stats()
        trk.step(max(i - 1, 0), i)
        s1 = stats()
        out.append(tuple(b - a for a, b in zip(s0, s1)))
    return out


def test_undistorted_f_and_the_launch_counts(pmv, gpu_ctx_factory):
    """stage 3 on the virtual-camera points of a fisheye camera: every step's survivors, and so every output, equal the twin step with lifted
    stage-3 points, single and in a group next to a radial-tangential tracker; and a step with a fisheye camera makes the launches and the
    waits of the same step with a radial-tangential camera"""
    w, h = ko.F_SIZE
    lefts = kc.scene(pmv, w, h)
    n = len(lefts)
    fish, radtan = fc.scene_fisheye(w, h, k=(-0.3, 0.05, 0.0, 0.0)), ko.f_camera()
    ctx, cams = _make(gpu_ctx_factory, pmv, w, h, False, [fish, radtan])
    a, r = sorted(cams)
    p = kc.params()
    want = _lifted_run(lefts, p, fish, ko.F_FOCAL, ("f-scene", "fish"))
    _, want_r, _ = ko.f_scene_run(pmv)
    _, plain = kc.scene_run(pmv, w, h, "default")
    assert (ko.counts(want)[:, 5] >= 0).sum() >= 3 and not np.array_equal(ko.counts(want), ko.counts(plain)), "the lift changes what F rejects"

    def stats():   # klt: (waits, launches); observe: (calls, observe launches, lift launches, waits)
        return tuple(ctx.debug_klt_stats()[1:3]) + tuple(ctx.debug_klt_observe_stats())

    for cid, cam, run in ((a, fish, want), (r, radtan, want_r)):
        trk = ctx.klt_create(**p)
        trk.set_observe(cid, -1, ko.DT, undistorted_f=True, f_focal=ko.F_FOCAL)
        for i in range(n):
            got = trk.step(max(i - 1, 0), i)
            kc.same(got, run[i][1])
            fc.same(trk.get_observations(), fc.twin().observe(cam, ko.DT, got[1], got[2], got[3]), ko.NAMES)
        trk.close()
    # the same step - the plain run's state before frame i, stage 3 on lifted points - through either camera: (waits, launches, observe calls,
    # observe launches, lift launches, observe waits) do not depend on the model
    lift_launches = 0
    for i in range(1, n):
        cost = []
        for cid in (a, r):
            trk = ctx.klt_create(**p)
            trk.set_tracks(*plain[i - 1][0].values())
            trk.set_observe(cid, -1, ko.DT, undistorted_f=True, f_focal=ko.F_FOCAL)
            s0 = stats()
            trk.step(i - 1, i)
            cost.append(tuple(y - x for x, y in zip(s0, stats())))
            trk.close()
        assert cost[0] == cost[1], (i, cost)
        lift_launches += cost[0][4]
    assert lift_launches >= 3, "F ran, on lifted points"
    # stage 3 on pixels: the observe launch alone, with either camera
    plain_cost = []
    for cid in (a, r):
        trk = ctx.klt_create(**p)
        trk.set_observe(cid, -1, ko.DT)
        plain_cost.append(_per_step(trk, n, stats))
        trk.close()
    assert plain_cost[0] == plain_cost[1]
    # a group: a fisheye tracker and a radial-tangential one on lifted points, and one on pixels
    trks = [ctx.klt_create(**p) for _ in range(3)]
    trks[0].set_observe(a, -1, ko.DT, undistorted_f=True, f_focal=ko.F_FOCAL)
    trks[1].set_observe(r, -1, ko.DT, undistorted_f=True, f_focal=ko.F_FOCAL)
    trks[2].set_observe(a, -1, ko.DT)
    for i in range(n):
        got = ctx.klt_step_many(trks, [max(i - 1, 0)] * 3, [i] * 3)
        for j, (run, cam) in enumerate(((want, fish), (want_r, radtan), (plain, fish))):
            try:
                kc.same(got[j], run[i][1])
                fc.same(trks[j].get_observations(), fc.twin().observe(cam, ko.DT, got[j][1], got[j][2], got[j][3]), ko.NAMES)
            except AssertionError as e:
                raise AssertionError(f"step {i}, tracker {j}: {e}") from None
    for t in trks:
        t.close()


class _DeviceStage1(kc.TwinOps):
    """klt_common's twin stages with stage 1 composed of the single calls on the device: pmv_project_points for the guesses, then
    pmv_lk_track_fb_levels from them (include/pmv_hip.h, pmv_klt_set_prediction); the fall-back as the header states it"""
    def __init__(self, ctx, cam_id, prev, cur, ids, pred):
        super().__init__(prev, cur)
        self.ctx, self.cam_id, self.ids, self.pred = ctx, cam_id, ids, pred
        self.result, self.guess = None, None

    def track(self, xy, fb):
        p = self.pred
        pxy, pok = self.ctx.project_points(self.cam_id, p["xyz"])
        where = {int(k): j for j, k in enumerate(p["ids"])}
        guess, joined = np.array(xy, np.float32).reshape(-1, 2), 0
        for i, k in enumerate(self.ids):
            j = where.get(int(k))
            if j is not None and pok[j]:
                guess[i], joined = pxy[j], joined + 1
        a = self.ctx.lk_track_fb_levels(0, 1, xy, init_xy=guess, fwd_top_level=p["top_level"], back_top_level=p["back_top_level"], back=fb)
        succ, fell = int((a[1] == 1).sum()), 0
        if succ < p["min_succ"]:
            a, fell = self.ctx.lk_track_fb_levels(0, 1, xy, fwd_top_level=-1, back_top_level=p["back_top_level"], back=fb), 1
        self.result, self.guess = (1, joined, succ, fell), guess
        return a if fb else a + (None, None, None)


def _fisheye_points_for(cam, target_xy, seed, jitter=1.5):
    """camera-frame points whose projection through `cam` lies within +-jitter px of target_xy (predict_common.points_for through the
    fisheye twin)"""
    rng = np.random.default_rng(seed)
    px = (np.asarray(target_xy, np.float64).reshape(-1, 2) + rng.uniform(-jitter, jitter, (len(target_xy), 2))).astype(np.float32)
    un, ok = fc.twin().points(cam, px)
    assert ok.all()
    z = rng.uniform(2.0, 30.0, len(px))
    return np.stack([un[:, 0].astype(np.float64) * z, un[:, 1].astype(np.float64) * z, z], axis=1)


def test_a_predicted_step_through_a_fisheye_camera(pmv, gpu_ctx_factory):
    """the guesses, the joined count and the step's outputs are those of pmv_project_points + pmv_lk_track_fb_levels composed, and of the
    twins; some points of the list cannot be projected (behind the camera, NaN) and their tracks start from their own positions"""
    w, h = kc.SIZES[0]
    case = pc.scene_case(pmv, w, h)
    _, frames, p, _ = case
    cam = fc.scene_fisheye(w, h)
    ctx = gpu_ctx_factory(w, h, n_slots=len(frames), max_tracks=MAX_TRACKS)
    kc.upload(ctx, frames)
    cid = fc.create(ctx, cam)
    s0 = pc.state_of(case)
    xyz = _fisheye_points_for(cam, pc.truth(case), seed=2)
    xyz[3], xyz[10], xyz[11] = (0.1, 0.1, -2.0), (np.nan, 0.0, 1.0), pc.FAR
    pred = pc.prediction(cam, s0["ids"], xyz)
    # the twins: predict_common's stage 1 with the guesses of the fisheye twin's projection
    pxy, pok = fc.twin().project(cam, xyz)
    want_guess = np.where(pok[:, None] == 1, pxy, s0["xy"]).astype(np.float32)
    assert pok.sum() == len(pok) - 2 and np.abs(want_guess - pc.truth(case))[pok == 1].max() > 0
    trk = ctx.klt_create(**p)
    for setting in (dict(), dict(top_level=0, back_top_level=0, min_succ=0), dict(min_succ=10 ** 6)):
        q = dict(pred, **setting)
        trk.set_tracks(s0["ids"], s0["ages"], s0["xy"], s0["next_id"])
        ops = _DeviceStage1(ctx, cid, frames[0], frames[1], s0["ids"], q)
        _, want = kc.compose(ops, s0, p)
        trk.set_prediction(cid, q["ids"], q["xyz"], top_level=q["top_level"], back_top_level=q["back_top_level"], min_succ=q["min_succ"])
        got = trk.step(0, 1)
        kc.same(got, want)
        r = trk.get_prediction_result()
        assert (r["consumed"], r["joined"], r["succ"], r["fell_back"]) == ops.result, (r, ops.result)
        assert ops.result[1] == int(pok.sum()) and np.array_equal(fc.bits(ops.guess), fc.bits(want_guess))
        assert ops.result[3] == (1 if setting.get("min_succ", 0) > 10 ** 5 else 0)
    # the launches and waits of a predicted step do not depend on the camera's model
    rid = ctx.camera_create(**pc.predict_camera(w, h))
    cost = []
    for c in (cid, rid):
        trk.set_tracks(s0["ids"], s0["ages"], s0["xy"], s0["next_id"])
        trk.set_prediction(c, pred["ids"], pc.good_prediction(case)["xyz"] if c == rid else _fisheye_points_for(cam, pc.truth(case), seed=2))
        k0 = ctx.debug_klt_stats()
        trk.step(0, 1)
        k1 = ctx.debug_klt_stats()
        cost.append((k1[1] - k0[1], k1[2] - k0[2]))
    assert cost[0] == cost[1], cost
    trk.close()


def test_remap_through_the_fisheye_maps(pmv, gpu_ctx_factory):
    w, h = 64, 48
    img = gc.noise_frame()[5:5 + h, 9:9 + w].copy()
    K = np.array([[30.0, 0, 31.5], [0, 31.0, 23.25], [0, 0, 1.0]])
    new_K = np.array([[12.0, 0, 32.0], [0, 12.0, 24.0], [0, 0, 1.0]])   # a wide virtual camera: border taps on every side
    mx, my = pmv.fisheye_map_build(K, fc.ALL_K["k"], (w, h), new_K=new_K)
    fc.same((mx, my), fc.twin().map_build(K, fc.ALL_K["k"], (w, h), new_K=new_K), ("map_x", "map_y"))
    ctx = gpu_ctx_factory(w, h, n_slots=1, max_tracks=64)
    mid = ctx.remap_map_create(mx, my)
    for border in (0, 200):
        ctx.frame_upload(0, img)
        ctx.frames_remap(0, 1, mid, border)
        want, st = rm.twin().apply(img, mx, my, border)
        assert st["inside"] > 0 and st["outside"] > 0 and st["mixed"] > 0
        assert np.array_equal(ctx.get_level(0, 0, w, h), want)
    ctx.remap_map_destroy(mid)
