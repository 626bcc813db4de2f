"""The tracker's observation setting on the device (pmv_klt_set_observe): in every step form the step's own outputs are those of the same
run with the setting off, byte for byte; pmv_klt_get_observations equals the stage-9 rule of the CPU twin (tests/twin/lift_twin.cpp) applied
to that step's outputs, bit for bit; and with undistorted_f every step equals the twin step whose stage 3 takes the lifted points
(tests/klt_observe_common.py). Slots: left frame i in slot i, its right frame in slot len(lefts) + i."""
import ctypes as C

import numpy as np
import pytest

import klt_common as kc
import klt_observe_common as ko
import klt_stereo_common as ks
import lift_common as lf

pytestmark = pytest.mark.gpu
INVALID, CAPACITY = ko.INVALID, ko.CAPACITY
FORMS = ["single", "stereo", "many", "many_stereo"]
STEREO = ks.STEREO["fb"]


def _same_outputs(got, want):
    kc.same(got[:5], want[:5])
    if len(got) > 5:
        ks.same_right(got[5:], want[5:])


def _check_observations(pmv, ctx, trk, o, cams, out, right_on):
    """o: None (setting off) or dict(cam=, rcam=, dt=) of camera ids; cams: id -> the camera's parameters"""
    if o is None:
        with pytest.raises(pmv.PmvError) as e:
            trk.get_observations()
        assert e.value.code == INVALID and "setting off" in str(e.value)
        return
    rcam = o.get("rcam", -1)
    right = (out[5], out[6]) if right_on and rcam >= 0 else None
    got = trk.get_observations()
    ko.same_observations(got, ko.expected(cams[o["cam"]], o["dt"], out, cams[rcam] if rcam >= 0 else None, right))
    if len(out[0]):
        lf.same(got[::2][:2], ctx.undistort_points(o["cam"], out[2]), ("un_xy", "ok"))
    if right is not None and len(out[0]):
        run, rok = ctx.undistort_points(rcam, out[5])
        assert np.array_equal(lf.bits(got[3]), lf.bits(run)) and np.array_equal(got[4], rok & out[6])
    return got


def _drive(pmv, ctx, form, plist, olist, cams, n_steps, right_slot=None, nl=kc.N_FRAMES):
    """two sets of trackers over the same frames, one with the observation settings of olist and one without any: every step, every tracker"""
    k = len(plist)
    assert k == 1 or form.startswith("many")
    on, off = [ctx.klt_create(**p) for p in plist], [ctx.klt_create(**p) for p in plist]
    for t, o in zip(on, olist):
        if o is not None:
            t.set_observe(o["cam"], o.get("rcam", -1), o["dt"])
    if "stereo" in form:
        for t in on + off:
            t.set_stereo(**STEREO)
    right_slot = right_slot or (lambda i, j: nl + i)   # nl: the number of left frames in the context
    outs = []
    for i in range(n_steps):
        ps, cs = max(i - 1, 0), i
        rs = [right_slot(i, j) for j in range(k)]

        def step(trks):
            if form == "single":
                return [trks[0].step(ps, cs)]
            if form == "stereo":
                return [trks[0].step_stereo(ps, cs, rs[0])]
            if form == "many":
                return ctx.klt_step_many(trks, [ps] * k, [cs] * k)
            return ctx.klt_step_many_stereo(trks, [ps] * k, [cs] * k, rs)

        got, want = step(on), step(off)
        for j in range(k):
            try:
                _same_outputs(got[j], want[j])
                _check_observations(pmv, ctx, on[j], olist[j], cams, got[j], "stereo" in form and rs[j] >= 0)
            except AssertionError as e:
                raise AssertionError(f"step {i}, tracker {j}: {e}") from None
        outs.append(got)
    for t in on + off:
        t.close()
    return outs


def _make(gpu_ctx_factory, pmv, w, h, stereo, lefts=None, rts=None, max_tracks=2048):
    lefts = kc.scene(pmv, w, h) if lefts is None else lefts
    if stereo:
        rts = ks.scene_rights(pmv, w, h) if rts is None else rts
        ctx = ks.make_ctx(gpu_ctx_factory, lefts, rts, max_tracks=max_tracks)
    else:
        ctx = gpu_ctx_factory(w, h, n_slots=len(lefts), max_tracks=max_tracks)
        kc.upload(ctx, lefts)
    cams = {}
    for cam in (ko.left_camera(w, h), ko.right_camera(w, h)):
        cams[ctx.camera_create(**cam)] = cam
    return ctx, cams


@pytest.mark.parametrize("size", kc.SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("name", ["default", "subpix"])
@pytest.mark.parametrize("form", FORMS)
def test_sequences(pmv, gpu_ctx_factory, size, name, form):
    w, h = size
    ctx, cams = _make(gpu_ctx_factory, pmv, w, h, "stereo" in form)
    a, b = sorted(cams)
    p = kc.params(**kc.SETTINGS[name])
    if form.startswith("many"):
        plist = [p, dict(p, target=64), dict(p, target=65)]
        olist = [dict(cam=a, rcam=b, dt=ko.DT), dict(cam=a, rcam=b, dt=ko.DT), dict(cam=b, rcam=a, dt=2 * ko.DT)]
        right = (lambda i, j: -1 if j == 1 else kc.N_FRAMES + i)
    else:
        plist, olist, right = [p], [dict(cam=a, rcam=b, dt=ko.DT)], None
    outs = _drive(pmv, ctx, form, plist, olist, cams, kc.N_FRAMES, right)
    assert all(len(o[0][0]) > 0 for o in outs) and any((o[0][1] > 1).any() for o in outs[1:]), "no survivor ever had a velocity to compute"
    if form == "many_stereo":
        assert all(not o[1][6].any() for o in outs) and all(o[0][6].any() for o in outs)


def test_a_group_with_the_setting_off_on_and_on_with_another_camera(pmv, gpu_ctx_factory):
    w, h = kc.SIZES[0]
    ctx, cams = _make(gpu_ctx_factory, pmv, w, h, False)
    a, b = sorted(cams)
    p = kc.params()
    _drive(pmv, ctx, "many", [p, p, dict(p, target=63)], [None, dict(cam=a, dt=ko.DT), dict(cam=b, dt=0.31)], cams, 4)
    # ... and in a stereo group, where the second tracker has a right frame and no right camera
    ctx, cams = _make(gpu_ctx_factory, pmv, w, h, True)
    a, b = sorted(cams)
    _drive(pmv, ctx, "many_stereo", [p, p, p], [None, dict(cam=a, dt=ko.DT), dict(cam=b, rcam=a, dt=0.31)], cams, 3, lambda i, j: kc.N_FRAMES + i)


@pytest.mark.parametrize("target", kc.TARGETS)
def test_targets(pmv, gpu_ctx_factory, target):
    """a lane short of a wavefront, a wavefront, one more, and several: the chunks of the observe kernel"""
    w, h = kc.SIZES[0]
    ctx, cams = _make(gpu_ctx_factory, pmv, w, h, True)
    a, b = sorted(cams)
    outs = _drive(pmv, ctx, "stereo", [kc.params(target=target)], [dict(cam=a, rcam=b, dt=ko.DT)], cams, 3)
    assert len(outs[0][0][0]) == min(target, len(outs[0][0][0])) > 0


def test_more_than_1024_tracks(pmv, gpu_ctx_factory):
    lefts = kc.big_pair(pmv)
    rts = ks.rights(lefts, "big")
    ctx, cams = _make(gpu_ctx_factory, pmv, kc.W_BIG, kc.H_BIG, True, lefts, rts)
    a, b = sorted(cams)
    outs = _drive(pmv, ctx, "stereo", [kc.params(**kc.BIG)], [dict(cam=a, rcam=b, dt=ko.DT)], cams, len(lefts), nl=len(lefts))
    assert max(len(o[0][0]) for o in outs) > 1024 and (outs[-1][0][1] > 1).sum() > 512


def _raw_get(ctx, tid, cap, n_alloc):
    fn = ctx.lib.pmv_klt_get_observations
    vp = C.c_void_p
    fn.argtypes = [vp, C.c_int, vp, vp, vp, vp, vp, C.c_int, vp]
    a = dict(un=np.full(2 * n_alloc, -7, np.float32), vel=np.full(2 * n_alloc, -7, np.float32), ok=np.full(n_alloc, 0xA5, np.uint8),
             run=np.full(2 * n_alloc, -7, np.float32), rok=np.full(n_alloc, 0xA5, np.uint8), n=np.full(1, -7, np.int32))
    rc = fn(ctx.h, tid, *(a[k].ctypes.data for k in ("un", "vel", "ok", "run", "rok")), cap, a["n"].ctypes.data)
    untouched = all((v == (0xA5 if v.dtype == np.uint8 else -7)).all() for k, v in a.items() if k != "n")
    return rc, untouched, int(a["n"][0])


def test_a_constant_gray_pair_gives_no_observations(pmv, gpu_ctx_factory):
    w, h = 64, 48
    g = ks.gray_pair(w, h)
    ctx, cams = _make(gpu_ctx_factory, pmv, w, h, True, g, g)
    a, b = sorted(cams)
    p = kc.params()
    trk = ctx.klt_create(**p)
    trk.set_stereo(**STEREO)
    trk.set_observe(a, b, ko.DT)
    for i in range(2):
        out = trk.step_stereo(max(i - 1, 0), i, 2 + i) if i else trk.step(0, 0)
        assert len(out[0]) == 0
        rc, untouched, n = _raw_get(ctx, trk.id, p["target"], p["target"])
        assert rc == 0 and untouched and n == 0, ko.last_error(ctx)
    trk.close()


def test_the_getter_refuses_what_it_cannot_answer(pmv, gpu_ctx_factory):
    w, h = kc.SIZES[0]
    ctx, cams = _make(gpu_ctx_factory, pmv, w, h, False)
    a, _ = sorted(cams)
    p = kc.params()
    trk = ctx.klt_create(**p)
    trk.set_observe(a, -1, ko.DT)
    rc, untouched, n = _raw_get(ctx, trk.id, p["target"], p["target"])
    assert rc == INVALID and untouched and n == -7 and "has not stepped" in ko.last_error(ctx)
    out = trk.step(0, 0)
    k = len(out[0])
    assert k > 1
    rc, untouched, n = _raw_get(ctx, trk.id, k - 1, p["target"])
    assert rc == CAPACITY and untouched and n == -7 and "cap" in ko.last_error(ctx)
    rc, untouched, n = _raw_get(ctx, trk.id, k, p["target"])
    assert rc == 0 and n == k and not untouched
    # null right arrays are legal
    fn = ctx.lib.pmv_klt_get_observations
    un, vel, ok, cnt = np.zeros((k, 2), np.float32), np.zeros((k, 2), np.float32), np.zeros(k, np.uint8), C.c_int(0)
    assert fn(ctx.h, trk.id, un.ctypes.data, vel.ctypes.data, ok.ctypes.data, None, None, k, C.addressof(cnt)) == 0 and cnt.value == k
    ko.same_observations((un, vel, ok), ko.expected(cams[a], ko.DT, out)[:3])
    assert fn(ctx.h, trk.id, None, vel.ctypes.data, ok.ctypes.data, None, None, k, C.addressof(cnt)) == INVALID
    # replacing the state forgets the observations; a step with the setting off too
    ids, ages, xy = trk.get_tracks()
    trk.set_tracks(ids, ages, xy, int(ids.max()) + 1)
    rc, untouched, _ = _raw_get(ctx, trk.id, p["target"], p["target"])
    assert rc == INVALID and untouched and "has not stepped" in ko.last_error(ctx)
    trk.set_observe(None)
    assert trk.get_observe() is None
    trk.step(0, 1)
    rc, untouched, _ = _raw_get(ctx, trk.id, p["target"], p["target"])
    assert rc == INVALID and untouched and "setting off" in ko.last_error(ctx)
    trk.close()


def test_undistorted_f_single_and_group(pmv, gpu_ctx_factory):
    """stage 3 on the virtual-camera points: every step equals the twin step with lifted stage-3 points, counts included"""
    w, h = ko.F_SIZE
    lefts = kc.scene(pmv, w, h)
    ctx = gpu_ctx_factory(w, h, n_slots=len(lefts), max_tracks=2048)
    kc.upload(ctx, lefts)
    cam = ko.f_camera()
    cid = ctx.camera_create(**cam)
    p, want, _ = ko.f_scene_run(pmv)
    p64, want64, _ = ko.f_scene_run(pmv, target=64)
    _, plain = kc.scene_run(pmv, w, h, "default")
    assert (ko.counts(want)[:, 5] >= 0).sum() >= 3 and not np.array_equal(ko.counts(want), ko.counts(plain))
    trk = ctx.klt_create(**p)
    trk.set_observe(cid, -1, ko.DT, undistorted_f=True, f_focal=ko.F_FOCAL)
    assert trk.get_observe() == dict(cam_id=cid, right_cam_id=-1, dt=ko.DT, undistorted_f=True, f_focal=ko.F_FOCAL)
    for i in range(len(lefts)):
        got = trk.step(max(i - 1, 0), i)
        kc.same(got, want[i][1])
        ko.same_observations(trk.get_observations(), ko.expected(cam, ko.DT, got))
    trk.close()
    # a group: two trackers on lifted points and one on pixels, which keeps the plain run's bytes
    trks = [ctx.klt_create(**p), ctx.klt_create(**p64), ctx.klt_create(**p)]
    trks[0].set_observe(cid, -1, ko.DT, undistorted_f=True, f_focal=ko.F_FOCAL)
    trks[1].set_observe(cid, -1, ko.DT, undistorted_f=True, f_focal=ko.F_FOCAL)
    trks[2].set_observe(cid, -1, ko.DT, undistorted_f=False, f_focal=float("nan"))   # (f_focal is read only with undistorted_f)
    for i in range(len(lefts)):
        got = ctx.klt_step_many(trks, [max(i - 1, 0)] * 3, [i] * 3)
        for j, run in enumerate((want, want64, plain)):
            try:
                kc.same(got[j], run[i][1])
                ko.same_observations(trks[j].get_observations(), ko.expected(cam, ko.DT, got[j]))
            except AssertionError as e:
                raise AssertionError(f"step {i}, tracker {j}: {e}") from None
    for t in trks:
        t.close()


def _per_step(ctx, trk, n, stats):
    """(launches, waits) of every step of a fresh run of n steps, from the counter function `stats` -> (waits, launches)"""
    out = []
    for i in range(n):
        s0 = stats()
        trk.step(max(i - 1, 0), i)
        s1 = stats()
        out.append((s1[1] - s0[1], s1[0] - s0[0]))
    return out


def test_counters(pmv, gpu_ctx_factory):
    w, h = ko.F_SIZE
    lefts = kc.scene(pmv, w, h)
    n = len(lefts)
    ctx = gpu_ctx_factory(w, h, n_slots=n, max_tracks=2048)
    kc.upload(ctx, lefts)
    p, want, _ = ko.f_scene_run(pmv)
    f_ran = [int(c[5] >= 0) for c in ko.counts(want)]
    assert sum(f_ran) >= 3 and f_ran[0] == 0

    def klt():   # (waits, launches) of pmv_debug_klt_stats
        s = ctx.debug_klt_stats()
        return s[1], s[2]

    # before any camera exists
    t = ctx.klt_create(**p)
    before = _per_step(ctx, t, n, klt)
    t.close()
    assert ctx.debug_klt_observe_stats() == [0, 0, 0, 0]
    cid = ctx.camera_create(**ko.f_camera())
    # the setting on, stage 3 on pixels: one observe launch per step, no wait more
    t = ctx.klt_create(**p)
    t.set_observe(cid, -1, ko.DT)
    o0 = ctx.debug_klt_observe_stats()
    on = _per_step(ctx, t, n, klt)
    o1 = ctx.debug_klt_observe_stats()
    t.close()
    assert [o1[k] - o0[k] for k in range(4)] == [n, n, 0, sum(wt for _, wt in before)]
    assert [(la + 1, wt) for la, wt in before] == on
    # with undistorted_f: one lift launch more in the steps in which F ran (the run is the lifted twin's, so its lists differ from `before`)
    t = ctx.klt_create(**p)
    t.set_observe(cid, -1, ko.DT, undistorted_f=True, f_focal=ko.F_FOCAL)
    o0 = ctx.debug_klt_observe_stats()
    s0 = klt()
    for i in range(n):
        kc.same(t.step(max(i - 1, 0), i), want[i][1])
    s1 = klt()
    o1 = ctx.debug_klt_observe_stats()
    assert [o1[k] - o0[k] for k in range(4)] == [n, n, sum(f_ran), s1[0] - s0[0]]
    assert s1[0] - s0[0] == n + sum(f_ran), "a step waits once, twice when F may run"
    # the setting off again, with cameras in the context: the observe counters do not move and a step is what it was
    t.set_observe(None)
    t.set_tracks(*kc.empty_state().values())
    o0 = ctx.debug_klt_observe_stats()
    assert _per_step(ctx, t, n, klt) == before
    assert ctx.debug_klt_observe_stats() == o0
    t.close()
    # a many-call: one observe launch whatever n_trk is, and none when no tracker of the group has the setting
    for n_trk in (1, 3):
        trks = [ctx.klt_create(**p) for _ in range(n_trk)]
        m0 = ctx.debug_klt_many_stats()
        ctx.klt_step_many(trks, [0] * n_trk, [0] * n_trk)
        m1 = ctx.debug_klt_many_stats()
        assert ctx.debug_klt_observe_stats() == o0
        for tr in trks:
            tr.set_tracks(*kc.empty_state().values())
        trks[-1].set_observe(cid, -1, ko.DT)
        ctx.klt_step_many(trks, [0] * n_trk, [0] * n_trk)
        m2 = ctx.debug_klt_many_stats()
        o1 = ctx.debug_klt_observe_stats()
        assert (m2[3] - m1[3]) - (m1[3] - m0[3]) == 1 and m2[2] - m1[2] == m1[2] - m0[2]
        assert [o1[k] - o0[k] for k in range(4)] == [1, 1, 0, m2[2] - m1[2]]
        o0 = o1
        for tr in trks:
            tr.close()


def test_changing_dt_changes_only_the_velocities(pmv, gpu_ctx_factory):
    w, h = kc.SIZES[0]
    ctx, cams = _make(gpu_ctx_factory, pmv, w, h, False)
    a, _ = sorted(cams)
    trk = ctx.klt_create(**kc.params())
    trk.set_observe(a, -1, 0.05)
    trk.step(0, 0)
    trk.step(0, 1)
    ids, ages, xy = trk.get_tracks()
    nid = int(ids.max()) + 1
    res = []
    for dt in (0.05, 0.1, 1.0 / 3.0):
        trk.set_tracks(ids, ages, xy, nid)
        trk.set_observe(a, -1, dt)
        out = trk.step(1, 2)
        obs = trk.get_observations()
        ko.same_observations(obs, ko.expected(cams[a], dt, out))
        res.append((out, obs))
    for out, obs in res[1:]:
        kc.same(out, res[0][0])
        lf.same((obs[0], obs[2]), (res[0][1][0], res[0][1][2]), ("un_xy", "ok"))
        assert not np.array_equal(lf.bits(obs[1]), lf.bits(res[0][1][1]))
    assert res[0][1][1].any()
    trk.close()


def test_a_bad_setting_keeps_the_old_one_and_a_named_camera_stays(pmv, gpu_ctx_factory):
    w, h = kc.SIZES[0]
    ctx, cams = _make(gpu_ctx_factory, pmv, w, h, False)
    a, b = sorted(cams)
    spare = ctx.camera_create(**lf.EUROC)
    ctx.camera_destroy(spare)
    trk = ctx.klt_create(**kc.params())
    assert trk.get_observe() is None
    good = dict(cam_id=a, right_cam_id=b, dt=0.05, undistorted_f=True, f_focal=460.0)
    trk.set_observe(**good)
    assert trk.get_observe() == good
    nan, inf = float("nan"), float("inf")
    for kw, text in ((dict(cam_id=-1), "cam_id"), (dict(cam_id=16), "cam_id"), (dict(cam_id=spare), "cam_id"), (dict(right_cam_id=-2), "right_cam_id"),
                     (dict(right_cam_id=spare), "right_cam_id"), (dict(dt=0.0), "dt"), (dict(dt=-0.1), "dt"), (dict(dt=nan), "dt"), (dict(dt=inf), "dt"),
                     (dict(undistorted_f=2), "undistorted_f"), (dict(undistorted_f=-1), "undistorted_f"), (dict(f_focal=0.0), "f_focal"), (dict(f_focal=-460.0), "f_focal"),
                     (dict(f_focal=nan), "f_focal"), (dict(f_focal=inf), "f_focal")):
        with pytest.raises(pmv.PmvError) as e:
            trk.set_observe(**dict(good, **kw))
        assert e.value.code == INVALID and text in str(e.value) and "pmv_klt_set_observe" in str(e.value), (kw, str(e.value))
        assert trk.get_observe() == good
    # a camera named by a setting cannot be destroyed until the setting is cleared (or names another camera, or the tracker goes)
    for cid in (a, b):
        with pytest.raises(pmv.PmvError) as e:
            ctx.camera_destroy(cid)
        assert e.value.code == INVALID and "observation setting" in str(e.value)
    lf.same(ctx.undistort_points(b, np.asarray([(10, 20)], np.float32)), lf.twin().points(cams[b], [(10, 20)]), ("un_xy", "ok"))
    trk.set_observe(a, -1, 0.05)
    ctx.camera_destroy(b)
    with pytest.raises(pmv.PmvError):
        ctx.camera_destroy(a)
    trk.set_observe(None)
    ctx.camera_destroy(a)
    with pytest.raises(pmv.PmvError) as e:
        trk.set_observe(**good)
    assert e.value.code == INVALID and trk.get_observe() is None
    trk.close()
