"""pmv_camera_* and pmv_undistort_points on the device: the lifted points equal the CPU twin (tests/twin/lift_twin.cpp) bit for bit - xy as
uint32, ok as bytes; every refusal returns its code and writes nothing; the camera table has 16 entries and leaves no memory behind."""
import ctypes as C

import numpy as np
import pytest

import lift_common as lf

pytestmark = pytest.mark.gpu
INVALID, CAPACITY = -2, -3
CANARY = -7
W, H = 640, 480
MAX_TRACKS = 2048


@pytest.fixture(scope="module")
def ctx(gpu_ctx_factory):
    return gpu_ctx_factory(W, H, n_slots=2, max_tracks=MAX_TRACKS)


def _points(n, seed=11):
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(-40, W + 40, n), rng.uniform(-40, H + 40, n)], axis=1).astype(np.float32)


def _last_error(ctx):
    return ctx.lib.pmv_last_error(ctx.h).decode()


@pytest.mark.parametrize("iters", [1, 5, 50])
def test_device_equals_twin(ctx, iters):
    """a lane, a lane short of a wavefront, a wavefront, one more, more than a workgroup, and several workgroups with a tail"""
    cam = lf.all_terms(W, H, iters=iters)
    cid = ctx.camera_create(**cam)
    try:
        for n in (0, 1, 63, 64, 65, 257, 1025):
            xy = _points(n, seed=n + 1)
            got = ctx.undistort_points(cid, xy)
            assert got[0].shape == (n, 2) and got[1].shape == (n,)
            lf.same(got, lf.twin().points(cam, xy), ("un_xy", "ok"))
            assert got[1].all()
    finally:
        ctx.camera_destroy(cid)


def test_the_singular_point_and_points_far_outside_the_frame(ctx):
    cid = ctx.camera_create(**lf.SINGULAR)
    far = ctx.camera_create(**lf.EUROC)
    try:
        xy = np.asarray([(310.5, 207.25), lf.SINGULAR_POINT, (290.0, 180.0), lf.SINGULAR_POINT, (0, 0)], np.float32)
        un, ok = ctx.undistort_points(cid, xy)
        lf.same((un, ok), lf.twin().points(lf.SINGULAR, xy), ("un_xy", "ok"))
        assert ok.tolist() == [1, 0, 1, 0, 1] and not lf.bits(un)[1].any() and not lf.bits(un)[3].any() and not np.isnan(un).any()
        rng = np.random.default_rng(3)
        out = np.concatenate([rng.uniform(-1e6, 1e6, (300, 2)), [(1e6, 1e6), (-1e6, -1e6), (1e6, -1e6), (999999.94, 0.0)]]).astype(np.float32)
        for c, cam in ((far, lf.EUROC), (cid, lf.SINGULAR)):
            got = ctx.undistort_points(c, out)
            lf.same(got, lf.twin().points(cam, out), ("un_xy", "ok"))
            assert not np.isnan(got[0]).any()
    finally:
        ctx.camera_destroy(cid)
        ctx.camera_destroy(far)


def _raw_points(ctx, cam_id, xy, n, null=None):
    """the C call on canary-filled outputs: (return code, outputs untouched)"""
    fn = ctx.lib.pmv_undistort_points
    vp = C.c_void_p
    fn.argtypes = [vp, C.c_int, vp, C.c_int, vp, vp]
    k = max(abs(n), len(xy), 1)
    a = dict(xy=np.ascontiguousarray(xy, np.float32), out=np.full(2 * k, CANARY, np.float32), ok=np.full(k, 0xA5, np.uint8))
    ptr = {name: (None if name == null else v.ctypes.data) for name, v in a.items()}
    rc = fn(ctx.h, cam_id, ptr["xy"], n, ptr["out"], ptr["ok"])
    return rc, bool((a["out"] == CANARY).all() and (a["ok"] == 0xA5).all())


def test_refusals_write_nothing(pmv, ctx):
    cid = ctx.camera_create(**lf.EUROC)
    gone = ctx.camera_create(**lf.EUROC)
    ctx.camera_destroy(gone)
    good = _points(8)
    try:
        for what, args, code, text in (("null xy", dict(cam_id=cid, xy=good, n=8, null="xy"), INVALID, "null"), ("null out_xy", dict(cam_id=cid, xy=good, n=8, null="out"), INVALID, "null"),
                                       ("null out_ok", dict(cam_id=cid, xy=good, n=8, null="ok"), INVALID, "null"),
                                       ("camera -1", dict(cam_id=-1, xy=good, n=8), INVALID, "camera -1"), ("camera 16", dict(cam_id=16, xy=good, n=8), INVALID, "camera 16"),
                                       ("destroyed camera", dict(cam_id=gone, xy=good, n=8), INVALID, "does not exist"),
                                       ("n < 0", dict(cam_id=cid, xy=good, n=-1), CAPACITY, "n = -1"),
                                       ("n above max_tracks", dict(cam_id=cid, xy=_points(MAX_TRACKS + 1), n=MAX_TRACKS + 1), CAPACITY, "max_tracks")):
            rc, untouched = _raw_points(ctx, **args)
            assert rc == code and untouched and text in _last_error(ctx), (what, rc, untouched, _last_error(ctx))
        for k, bad in ((0, (np.nan, 1.0)), (3, (1.0, np.inf)), (7, (-np.inf, 2.0)), (5, (1.5e6, 0.0)), (2, (0.0, -1.0000001e6))):
            xy = good.copy()
            xy[k] = bad
            rc, untouched = _raw_points(ctx, cid, xy, 8)
            assert rc == INVALID and untouched and f"point {k} " in _last_error(ctx) and "beyond 1e6" in _last_error(ctx), (k, bad, rc, _last_error(ctx))
        # n == 0 is legal, launches nothing and writes nothing
        rc, untouched = _raw_points(ctx, cid, good, 0)
        assert rc == 0 and untouched
        # the camera's own parameters
        base = dict(lf.EUROC)
        for kw, text in ((dict(fx=0.0), "fx"), (dict(fy=0.0), "fy"), (dict(fx=float("nan")), "fx"), (dict(fy=float("inf")), "fy"), (dict(cx=float("nan")), "cx"),
                         (dict(cy=float("-inf")), "cy"), (dict(dist=(0.1, float("nan"))), "dist[1]"), (dict(dist=(0, 0, 0, 0, 0, 0, 0, float("inf"))), "dist[7]"),
                         (dict(iters=0), "iters"), (dict(iters=51), "iters"), (dict(iters=-3), "iters")):
            with pytest.raises(pmv.PmvError) as e:
                ctx.camera_create(**dict(base, **kw))
            assert e.value.code == INVALID and text in str(e.value) and "pmv_camera_create" in str(e.value), (kw, str(e.value))
        fn = ctx.lib.pmv_camera_create
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        p, out = pmv.camera_params(**lf.EUROC), C.c_int(CANARY)
        assert fn(ctx.h, None, C.addressof(out)) == INVALID and out.value == CANARY
        assert fn(ctx.h, C.addressof(p), None) == INVALID
        for bad_id in (-1, 16, gone):
            with pytest.raises(pmv.PmvError) as e:
                ctx.camera_destroy(bad_id)
            assert e.value.code == INVALID and "does not exist" in str(e.value)
        # good calls afterwards
        lf.same(ctx.undistort_points(cid, good), lf.twin().points(lf.EUROC, good), ("un_xy", "ok"))
    finally:
        ctx.camera_destroy(cid)


def test_sixteen_cameras_and_no_memory_left_behind(pmv, ctx):
    start = pmv.mem_live()
    cams = [dict(lf.all_terms(W, H), fx=300.0 + 7 * k, iters=1 + k) for k in range(16)]
    ids = [ctx.camera_create(**c) for c in cams]
    assert sorted(ids) == list(range(16))
    assert pmv.mem_live()[0] > start[0], "the cameras live in a device table"
    with pytest.raises(pmv.PmvError) as e:
        ctx.camera_create(**cams[0])
    assert e.value.code == CAPACITY and "16 cameras" in str(e.value)
    xy = _points(65)
    for k in (0, 7, 15):   # every entry of the table is its own camera
        lf.same(ctx.undistort_points(ids[k], xy), lf.twin().points(cams[k], xy), ("un_xy", "ok"))
    # a freed id is handed out again, with the new parameters
    ctx.camera_destroy(ids[5])
    again = ctx.camera_create(**lf.EUROC)
    assert again == ids[5]
    lf.same(ctx.undistort_points(again, xy), lf.twin().points(lf.EUROC, xy), ("un_xy", "ok"))
    for i in ids:
        ctx.camera_destroy(i)
    assert pmv.mem_live() == start
