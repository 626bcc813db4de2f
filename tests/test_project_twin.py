"""The CPU twin of pmv_project_points (tests/twin/project_twin.cpp) without a GPU: it agrees with the forward model in float64 numpy
(lift_common.forward) to one float32 ulp - both are double computations that differ only in operation order, so after the rounding to
float they can straddle at most one rounding boundary -, it inverts the twin lift, and its ok rule refuses what the header says it refuses."""
import numpy as np
import pytest

import lift_common as lf
import predict_common as pc

W, H = 752, 480
CAMS = {"EUROC": lf.EUROC, "all_terms": lf.all_terms(W, H)}


@pytest.mark.parametrize("name", sorted(CAMS))
def test_the_twin_agrees_with_the_numpy_forward_model(name):
    cam = CAMS[name]
    xyz = pc.camera_points(4000, seed=3, spread=1.2)
    xy, ok = pc.project_twin().points(cam, xyz)
    assert ok.all()
    u, v = lf.forward(cam, xyz[:, 0] / xyz[:, 2], xyz[:, 1] / xyz[:, 2])
    want = np.stack([u, v], axis=1).astype(np.float32)
    d = pc.ulp_distance(xy, want)
    print(name, "ulp distance: max", int(d.max()), "non-zero", int((d > 0).sum()), "of", d.size)
    assert d.max() <= 1
    outside = (xy[:, 0] < 0) | (xy[:, 0] >= W) | (xy[:, 1] < 0) | (xy[:, 1] >= H)
    print(name, "pixels outside the frame:", int(outside.sum()))
    assert outside.any() and not outside.all(), "points beyond the frame's edge are projected like the others"


@pytest.mark.parametrize("name", sorted(CAMS))
def test_it_inverts_the_lift(name):
    """pixels -> twin lift -> any depth -> twin projection: back at the pixel to the accuracy the fixed-point lift has"""
    cam = dict(CAMS[name], iters=50)
    rng = np.random.default_rng(5)
    px = np.stack([rng.uniform(40, W - 40, 500), rng.uniform(40, H - 40, 500)], axis=1).astype(np.float32)
    un, ok = lf.twin().points(cam, px)
    assert ok.all()
    z = rng.uniform(0.5, 30.0, 500)
    xyz = np.stack([un[:, 0].astype(np.float64) * z, un[:, 1].astype(np.float64) * z, z], axis=1)
    xy, ok = pc.project_twin().points(cam, xyz)
    err = np.abs(xy.astype(np.float64) - px).max()
    print(name, "round trip error", err, "px")
    # the lift is rounded to float (2^-24 relative on a coordinate of at most ~1, times fx < 500 px: 3e-5 px) and the pixel again (ulp of 752: 6e-5)
    assert ok.all() and err < 2e-4


def test_the_ok_rule():
    tw = pc.project_twin()
    xyz = np.array([p for p, _ in pc.REFUSED], np.float64)
    want = np.array([k for _, k in pc.REFUSED], np.uint8)
    for cam in (lf.EUROC, lf.all_terms(W, H)):
        xy, ok = tw.points(cam, xyz)
        assert ok.tolist() == want.tolist()
        assert not lf.bits(xy)[ok == 0].any(), "a refused point is (+0, +0)"
        assert not np.isnan(xy).any() and np.abs(xy).max() <= 1e6
    # Z <= 0 and NaN refuse whatever the rest is
    rng = np.random.default_rng(9)
    pts = pc.camera_points(64, seed=9)
    behind = pts * np.array([1, 1, -1.0])
    assert not tw.points(lf.EUROC, behind)[1].any()
    holes = pts.copy()
    holes[np.arange(64), rng.integers(0, 3, 64)] = np.nan
    xy, ok = tw.points(lf.EUROC, holes)
    assert not ok.any() and not lf.bits(xy).any()
    # the pole of the forward model: 1 / 0 and 0 / 0
    for cam in (pc.POLE, pc.POLE_NAN):
        xy, ok = tw.points(cam, np.array(pc.POLE_POINTS + [(0.1, 0.2, 1.0)], np.float64))
        assert ok.tolist() == [0, 0, 0, 1] and not lf.bits(xy)[:3].any() and not np.isnan(xy).any()
    # the 1e6 bound is on the rounded pixel, inclusive: fx = 1, cx = 0 -> u = x
    unit = dict(fx=1.0, fy=1.0, cx=0.0, cy=0.0, dist=(), iters=1)
    edge = np.array([(1e6, 0, 1), (0, -1e6, 1), (1000000.03, 0, 1), (1000000.04, 0, 1), (0, 1000000.0625, 1), (-1000000.0625, 0, 1)], np.float64)
    xy, ok = tw.points(unit, edge)
    # float32 has a spacing of 0.0625 at 1e6: 1000000.03 rounds down to 1e6 (accepted), 1000000.04 up to 1000000.0625 (refused)
    assert ok.tolist() == [1, 1, 1, 0, 0, 0]
    assert xy[2, 0] == np.float32(1e6)
