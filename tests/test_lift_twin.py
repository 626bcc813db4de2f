"""The CPU twin of the lift (tests/twin/lift_twin.cpp) without a GPU: against a float64 numpy restatement bit for bit, the closed cases, the
round trip through the forward model of pmv.undistort_map's arithmetic, the stage-9 rule on hand-made lists, and what the scene of the
undistorted-F GPU test is there for."""
import numpy as np

import klt_common as kc
import klt_observe_common as ko
import lift_common as lf


def restated(cam, xy):
    """the header's statements in their order, in float64 numpy (IEEE + - * /): (un_xy float32, ok uint8)"""
    xy = np.asarray(xy, np.float32).reshape(-1, 2)
    fx, fy, cx, cy = (np.float64(cam[k]) for k in ("fx", "fy", "cx", "cy"))
    k1, k2, p1, p2, k3, k4, k5, k6 = (np.float64(v) for v in lf.dist8(cam))
    ifx, ify = np.float64(1.0) / fx, np.float64(1.0) / fy
    with np.errstate(all="ignore"):
        x0 = (xy[:, 0].astype(np.float64) - cx) * ifx
        y0 = (xy[:, 1].astype(np.float64) - cy) * ify
        x, y = x0, y0
        for _ in range(cam["iters"]):
            r2 = x * x + y * y
            icdist = (1 + ((k6 * r2 + k5) * r2 + k4) * r2) / (1 + ((k3 * r2 + k2) * r2 + k1) * r2)
            dX = 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
            dY = p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
            x, y = (x0 - dX) * icdist, (y0 - dY) * icdist
        xf, yf = x.astype(np.float32), y.astype(np.float32)
    ok = np.isfinite(x) & np.isfinite(y) & np.isfinite(xf) & np.isfinite(yf)
    out = np.stack([np.where(ok, xf, np.float32(0)), np.where(ok, yf, np.float32(0))], axis=1).astype(np.float32)
    return out, ok.astype(np.uint8), (x, y)


def _draw(seed, n, w, h, margin=0.0):
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(-margin, w + margin, n), rng.uniform(-margin, h + margin, n)], axis=1).astype(np.float32)


def test_the_twin_equals_the_numpy_restatement_bit_for_bit():
    for cam, (w, h) in ((lf.EUROC, (752, 480)), (lf.all_terms(640, 480), (640, 480)), (lf.all_terms(640, 480, iters=50), (640, 480)),
                        (lf.scene_camera(320, 200), (320, 200)), (dict(lf.EUROC, iters=1), (752, 480)), (lf.SINGULAR, (600, 400))):
        xy = np.concatenate([_draw(5, 1500, w, h, margin=3 * w), np.asarray([lf.SINGULAR_POINT, (cam["cx"], cam["cy"]), (-1e6, 1e6), (1e6, -1e6)], np.float32)])
        got = lf.twin().points(cam, xy)
        want = restated(cam, xy)[:2]
        lf.same(got, want, ("un_xy", "ok"))
        assert not np.isnan(got[0]).any()


def test_zero_distortion_is_the_pinhole_lift_exactly():
    cam = dict(fx=458.654, fy=457.296, cx=367.215, cy=248.375, dist=(), iters=5)
    xy = _draw(7, 1000, 752, 480, margin=100)
    un, ok = lf.twin().points(cam, xy)
    ifx, ify = 1.0 / np.float64(cam["fx"]), 1.0 / np.float64(cam["fy"])
    want = np.stack([((xy[:, 0].astype(np.float64) - cam["cx"]) * ifx).astype(np.float32), ((xy[:, 1].astype(np.float64) - cam["cy"]) * ify).astype(np.float32)], axis=1)
    assert ok.all() and np.array_equal(lf.bits(un), lf.bits(want))


def test_the_singular_point_is_refused_and_no_nan_is_written():
    xy = np.asarray([(310.5, 207.25), lf.SINGULAR_POINT, (290.0, 180.0)], np.float32)
    x, y = restated(lf.SINGULAR, xy)[2]
    assert np.isnan(x[1]) and np.isnan(y[1]), "the plain iteration is expected to yield NaN at the singular point"
    un, ok = lf.twin().points(lf.SINGULAR, xy)
    assert ok.tolist() == [1, 0, 1] and lf.bits(un)[1].tolist() == [0, 0] and not np.isnan(un).any()
    assert un[0].any() and un[2].any()


def test_round_trip_through_the_forward_model():
    """the lift inverts the forward model of pmv_undistort_map_build: re-projecting the lifted points gives the pixels back, the better the
    more iterations. This pins the model, not bits."""
    xy = _draw(1, 4000, 752, 480)
    err, err_d = {}, {}
    for iters in (5, 8, 20):
        cam = dict(lf.EUROC, iters=iters)
        un, ok = lf.twin().points(cam, xy)
        assert ok.all()
        u, v = lf.forward(cam, un[:, 0].astype(np.float64), un[:, 1].astype(np.float64))
        err[iters] = float(np.hypot(u - xy[:, 0], v - xy[:, 1]).max())
        x, y = restated(cam, xy)[2]   # the doubles before their rounding to float
        u, v = lf.forward(cam, x, y)
        err_d[iters] = float(np.hypot(u - xy[:, 0], v - xy[:, 1]).max())
    print("re-projection error (px) by iters, float32 lifts:", err, " doubles:", err_d)
    assert err[5] > err[8] > err[20] and err_d[5] > err_d[8] > err_d[20]
    assert 0.05 < err[5] < 1.0 and err[8] < 0.05
    # measured with this draw (seed 1, 4000 points) at iters = 20: 3.0e-8 px on the doubles, 1.9e-5 px on the float32 lifts (the rounding of
    # a normalised coordinate to float32, times fx); the bounds are 10 x those
    assert err_d[20] < 3.0e-7
    assert err[20] < 1.9e-4


def test_the_stage_9_rule_on_hand_made_lists():
    cam, rcam = lf.SINGULAR, lf.all_terms(600, 400)
    bad = lf.SINGULAR_POINT
    ages = np.asarray([1, 5, 5, 5, 2, 0], np.int32)
    xy = np.asarray([(310, 210), (320.5, 190.25), bad, (280, 220), (305, 195), (300, 205)], np.float32)
    prev = np.asarray([(310, 210), (318.0, 191.0), (330, 200), bad, (304, 196), (299, 204)], np.float32)
    dt = 0.1
    un, vel, ok, run, rok = lf.twin().observe(cam, dt, ages, xy, prev)
    pun, pok = lf.twin().points(cam, prev)
    pts, pts_ok = lf.twin().points(cam, xy)
    assert np.array_equal(lf.bits(un), lf.bits(pts)) and np.array_equal(ok, pts_ok)
    assert ok.tolist() == [1, 1, 0, 1, 1, 1] and pok.tolist() == [1, 1, 1, 0, 1, 1]
    assert not vel[0].any(), "a new track (age 1, prev = xy) has velocity 0"
    assert not vel[2].any() and not vel[3].any(), "a track whose lift or previous lift is refused has velocity 0"
    assert not vel[5].any(), "age 0 is not above 1"
    for i in (1, 4):   # the subtraction in float32, the division in double
        d = (un[i] - pun[i]).astype(np.float32)
        want = (d.astype(np.float64) / np.float64(dt)).astype(np.float32)
        assert np.array_equal(lf.bits(vel[i]), lf.bits(want)) and vel[i].any()
        # ... which is not the float32 division, nor a multiplication by 1 / dt, for every operand: the rule is pinned by its own statement
    many = _draw(3, 2000, 600, 400)
    shifted = many + np.float32(1.5)
    _, v2, ok2, _, _ = lf.twin().observe(lf.all_terms(600, 400), 0.3, np.full(len(many), 3, np.int32), shifted, many)
    a, b = lf.twin().points(lf.all_terms(600, 400), shifted)[0], lf.twin().points(lf.all_terms(600, 400), many)[0]
    want = ((a - b).astype(np.float32).astype(np.float64) / np.float64(0.3)).astype(np.float32)
    assert ok2.all() and np.array_equal(lf.bits(v2), lf.bits(want))
    f32_div = ((a - b).astype(np.float32) / np.float32(0.3)).astype(np.float32)
    assert not np.array_equal(lf.bits(want), lf.bits(f32_div)), "dt enters as a double division: a float32 division gives other bits somewhere"
    assert not rok.any() and not run.any(), "no right camera: right ok all 0 and nothing written"
    # right ok = right status AND right lift ok; unmatched tracks are lifted too
    rxy = np.asarray([(300, 200), (310, 190), (0, 0), (280, 220), (np.nan, 0), (290, 210)], np.float32)
    rst = np.asarray([1, 0, 1, 1, 1, 1], np.uint8)
    sing_right = lf.twin().observe(rcam, dt, ages, xy, prev, lf.SINGULAR, np.where(np.arange(6)[:, None] == 3, np.asarray(bad, np.float32), rxy), rst)
    assert sing_right[4].tolist() == [1, 0, 1, 0, 0, 1]   # 1: unmatched; 3: the singular point; 4: LK left no number
    lifted = lf.twin().points(lf.SINGULAR, np.where(np.arange(6)[:, None] == 3, np.asarray(bad, np.float32), rxy))
    assert np.array_equal(lf.bits(sing_right[3]), lf.bits(lifted[0])) and sing_right[3][1].any() and not np.isnan(sing_right[3]).any()


def test_the_undistorted_f_scene_does_what_it_is_there_for(pmv):
    """k1 = -0.3, fx = fy = 0.58 w, centre (w / 2, h / 2), iters 8, f_focal 460 on klt_common's moving-block scene at 320 x 200: stage 3 runs,
    its mask differs from the pixel-F mask of the same survivors in at least one step, and it always keeps at least 15 tracks"""
    cam = ko.f_camera()
    w, h = ko.F_SIZE
    assert (cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["dist"], cam["iters"], ko.F_FOCAL) == (0.58 * w, 0.58 * w, w / 2, h / 2, (-0.3,), 8, 460.0)
    p, run, log = ko.f_scene_run(pmv)
    c = ko.counts(run)
    ran = c[:, 5] >= 0
    assert ran.sum() >= 3 and len(log) == ran.sum()
    assert (c[ran, 2] >= 15).all(), c
    assert any(not np.array_equal(lifted, pixel) for lifted, pixel in log), "the lifted points give the pixel-F mask in every step"
    # and the run is not the plain one
    plain = ko.counts(kc.scene_run(pmv, w, h, "default")[1])
    assert not np.array_equal(c, plain)
