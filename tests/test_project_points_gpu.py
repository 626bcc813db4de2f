"""pmv_project_points on the device: the pixels equal the CPU twin (tests/twin/project_twin.cpp) bit for bit - xy as uint32, ok as bytes -,
refused points included; every refusal of the call returns its code and writes nothing; the call's block leaves with the last camera."""
import ctypes as C

import numpy as np
import pytest

import lift_common as lf
import predict_common as pc

pytestmark = pytest.mark.gpu
INVALID, CAPACITY = -2, -3
CANARY = -7
W, H = 640, 480
MAX_TRACKS = 2048


@pytest.fixture(scope="module")
def ctx(gpu_ctx_factory):
    return gpu_ctx_factory(W, H, n_slots=2, max_tracks=MAX_TRACKS)


@pytest.mark.parametrize("name", ["EUROC", "all_terms", "pinhole"])
def test_device_equals_twin(ctx, name):
    """a lane, a lane short of a wavefront, one more than a wavefront, more than a workgroup, several workgroups with a tail, the most"""
    cam = dict(EUROC=lf.EUROC, all_terms=lf.all_terms(W, H), pinhole=dict(fx=371.2, fy=371.2, cx=320.0, cy=240.0, dist=(), iters=1))[name]
    cid = ctx.camera_create(**cam)
    try:
        for n in (0, 1, 63, 64, 65, 257, 1025, MAX_TRACKS):
            xyz = pc.camera_points(n, seed=n + 1, spread=1.2)
            got = ctx.project_points(cid, xyz)
            assert got[0].shape == (n, 2) and got[1].shape == (n,) and got[0].dtype == np.float32 and got[1].dtype == np.uint8
            lf.same(got, pc.project_twin().points(cam, xyz), ("xy", "ok"))
            assert got[1].all()
    finally:
        ctx.camera_destroy(cid)


def test_refused_points_are_zero_with_ok_0(ctx):
    xyz = np.array([p for p, _ in pc.REFUSED], np.float64)
    want_ok = [k for _, k in pc.REFUSED]
    unit = dict(fx=1.0, fy=1.0, cx=0.0, cy=0.0, dist=(), iters=1)
    edge = np.array([(1e6, 0, 1), (0, -1e6, 1), (1000000.03, 0, 1), (1000000.04, 0, 1), (0, 1000000.0625, 1), (-1000000.0625, 0, 1)], np.float64)
    poles = np.array(pc.POLE_POINTS + [(0.1, 0.2, 1.0)], np.float64)
    # refused points between good ones, across a wavefront boundary
    mixed = pc.camera_points(130, seed=4)
    mixed[[0, 63, 64, 65, 129]] = [(0, 0, 0), (np.nan, 1, 1), (1, 1, -2), (1, np.inf, 1), (0.5, 0.5, -0.0)]
    for cam, pts, ok_list in ((lf.EUROC, xyz, want_ok), (lf.all_terms(W, H), xyz, want_ok), (unit, edge, [1, 1, 1, 0, 0, 0]), (pc.POLE, poles, [0, 0, 0, 1]),
                              (pc.POLE_NAN, poles, [0, 0, 0, 1]), (lf.EUROC, mixed, None)):
        cid = ctx.camera_create(**cam)
        try:
            got = ctx.project_points(cid, pts)
        finally:
            ctx.camera_destroy(cid)
        want = pc.project_twin().points(cam, pts)
        lf.same(got, want, ("xy", "ok"))
        if ok_list is not None:
            assert want[1].tolist() == ok_list
        assert not lf.bits(got[0])[got[1] == 0].any() and not np.isnan(got[0]).any()
    assert np.flatnonzero(want[1] == 0).tolist() == [0, 63, 64, 65, 129]


def _raw(ctx, cam_id, xyz, n, null=None):
    """the C call on canary-filled outputs: (return code, outputs untouched)"""
    fn = ctx.lib.pmv_project_points
    vp = C.c_void_p
    fn.argtypes = [vp, C.c_int, vp, C.c_int, vp, vp]
    k = max(abs(n), len(xyz), 1)
    a = dict(xyz=np.ascontiguousarray(xyz, np.float64), out=np.full(2 * k, CANARY, np.float32), ok=np.full(k, 0xA5, np.uint8))
    ptr = {name: (None if name == null else v.ctypes.data) for name, v in a.items()}
    rc = fn(ctx.h, cam_id, ptr["xyz"], n, ptr["out"], ptr["ok"])
    return rc, bool((a["out"] == CANARY).all() and (a["ok"] == 0xA5).all())


def test_refusals_write_nothing_and_the_block_leaves_with_the_cameras(pmv, ctx):
    start = pmv.mem_live()
    cid = ctx.camera_create(**lf.EUROC)
    gone = ctx.camera_create(**lf.EUROC)
    ctx.camera_destroy(gone)
    good = pc.camera_points(8)
    for what, args, code, text in (("null xyz", dict(cam_id=cid, xyz=good, n=8, null="xyz"), INVALID, "null"), ("null out_xy", dict(cam_id=cid, xyz=good, n=8, null="out"), INVALID, "null"),
                                   ("null out_ok", dict(cam_id=cid, xyz=good, n=8, null="ok"), INVALID, "null"),
                                   ("camera -1", dict(cam_id=-1, xyz=good, n=8), INVALID, "camera -1"), ("camera 16", dict(cam_id=16, xyz=good, n=8), INVALID, "camera 16"),
                                   ("destroyed camera", dict(cam_id=gone, xyz=good, n=8), INVALID, "does not exist"),
                                   ("n < 0", dict(cam_id=cid, xyz=good, n=-1), CAPACITY, "n = -1"),
                                   ("n above max_tracks", dict(cam_id=cid, xyz=pc.camera_points(MAX_TRACKS + 1), n=MAX_TRACKS + 1), CAPACITY, "max_tracks")):
        rc, untouched = _raw(ctx, **args)
        err = ctx.lib.pmv_last_error(ctx.h).decode()
        assert rc == code and untouched and text in err and "pmv_project_points" in err, (what, rc, untouched, err)
    rc, untouched = _raw(ctx, cid, good, 0)   # n == 0 is legal, launches nothing and writes nothing
    assert rc == 0 and untouched
    lf.same(ctx.project_points(cid, good), pc.project_twin().points(lf.EUROC, good), ("xy", "ok"))
    # the lift of the same context is what it was next to the new call
    px = np.stack([np.linspace(5, W - 5, 65), np.linspace(5, H - 5, 65)], axis=1).astype(np.float32)
    lf.same(ctx.undistort_points(cid, px), lf.twin().points(lf.EUROC, px), ("un_xy", "ok"))
    assert pmv.mem_live()[1] > start[1], "the call's block is pinned host memory"
    ctx.camera_destroy(cid)
    assert pmv.mem_live() == start
