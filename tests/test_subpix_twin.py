"""The CPU twin of pmv_corner_subpix (tests/twin/subpix_twin.cpp) without a GPU: an independent numpy restatement written from the header
text equals its serial form bit for bit (weight table, one patch on each sampling path, one update step); the kernel's summation order
stays within one float ulp of cv's serial order after one update; properties of the refinement; the scenes give the GPU tests something
to compare."""
import ctypes as C
import ctypes.util

import numpy as np
import pytest

import gftt_common as gc
import subpix_common as sc

f32, f64 = np.float32, np.float64


# ---- the restatement: include/pmv_hip.h, "cv::cornerSubPix(level 0 of `slot`, ...", line by line ----------------------------------------
def _expf():
    def make():
        libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
        libm.expf.restype, libm.expf.argtypes = C.c_float, [C.c_float]
        return lambda v: f32(libm.expf(C.c_float(float(v))))   # "computed on the HOST with libm"
    return gc.cached("libm_expf", make)


def np_table(win, zero):
    expf = _expf()
    ww, wh = win
    m = np.zeros((2 * wh + 1, 2 * ww + 1), f32)
    for i in range(2 * wh + 1):
        y = f32(i - wh) / f32(wh)
        vy = expf(-y * y)
        for j in range(2 * ww + 1):
            x = f32(j - ww) / f32(ww)
            m[i, j] = f32(vy * expf(-x * x))
    zw, zh = zero
    if zw >= 0 and zh >= 0 and 2 * zw + 1 < 2 * ww + 1 and 2 * zh + 1 < 2 * wh + 1:
        m[wh - zh:wh + zh + 1, ww - zw:ww + zw + 1] = 0
    return m


def np_patch(img, cx, cy, win):
    rows, cols = img.shape
    W, H = 2 * win[0] + 3, 2 * win[1] + 3
    cx, cy = f32(cx) - f32(win[0] + 1), f32(cy) - f32(win[1] + 1)
    ipx, ipy = int(np.floor(cx)), int(np.floor(cy))
    a, b = f32(cx - f32(ipx)), f32(cy - f32(ipy))
    src = img.astype(f32)
    one = f32(1)
    out = np.zeros((H, W), f32)
    if 0 <= ipx and ipx + W < cols and 0 <= ipy and ipy + H < rows:
        a = max(a, f32(0.0001))
        a12, a22, b1, b2 = a * (one - b), a * b, one - b, b
        s = (f64(1) - f64(a)) / f64(a)
        top, bot = src[ipy:ipy + H, ipx:ipx + W + 1], src[ipy + 1:ipy + H + 1, ipx:ipx + W + 1]
        t = a12 * top[:, 1:] + a22 * bot[:, 1:]                 # t[j] = a12 src[j+1] + a22 src[j+1+step]
        prev = np.empty_like(t)
        prev[:, 0] = (one - a) * (b1 * top[:, 0] + b2 * bot[:, 0])
        prev[:, 1:] = (t[:, :-1].astype(f64) * s).astype(f32)   # element j needs only t[j] and t[j-1]
        return prev + t, True
    a11, a12, a21, a22, b1, b2 = (one - a) * (one - b), a * (one - b), (one - a) * b, a * b, one - b, b
    for i in range(H):
        r0, r1 = src[min(max(ipy + i, 0), rows - 1)], src[min(max(ipy + i + 1, 0), rows - 1)]
        for j in range(W):
            x0 = ipx + j
            if x0 < 0 or x0 >= cols - 1:                        # both sample columns clamp to the same column
                xc = 0 if x0 < 0 else cols - 1
                out[i, j] = r0[xc] * b1 + r1[xc] * b2
            else:
                out[i, j] = ((r0[x0] * a11 + r0[x0 + 1] * a12) + r1[x0] * a21) + r1[x0 + 1] * a22
    return out, False


def np_step(img, x, y, win, zero):
    """one pass of the loop body in cv's raster order: (x, y, updates, flag bits before the revert test)"""
    rows, cols = img.shape
    P, _ = np_patch(img, x, y, win)
    m = np_table(win, zero)
    ww, wh = win
    a = b = c = bb1 = bb2 = 0.0
    for i in range(2 * wh + 1):
        for j in range(2 * ww + 1):
            tgx, tgy = float(f32(P[i + 1, j + 2] - P[i + 1, j])), float(f32(P[i + 2, j + 1] - P[i, j + 1]))
            w = float(m[i, j])
            gxx, gxy, gyy = tgx * tgx * w, tgx * tgy * w, tgy * tgy * w
            px, py = float(j - ww), float(i - wh)
            a += gxx
            b += gxy
            c += gyy
            bb1 += gxx * px + gxy * py
            bb2 += gxy * px + gyy * py
    det = a * c - b * b
    eps = float(np.finfo(f64).eps)
    if abs(det) <= eps * eps:
        return f32(x), f32(y), 0, sc.DET
    scale = 1.0 / det
    nx = f32(float(f32(x)) + c * scale * bb1 - b * scale * bb2)
    ny = f32(float(f32(y)) - b * scale * bb1 + a * scale * bb2)
    flags = sc.LEFT if (nx < 0 or nx >= cols or ny < 0 or ny >= rows) else 0
    return nx, ny, 1, flags


# ---- restatement against the serial twin -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("win, zero", [((5, 5), (-1, -1)), ((1, 1), (-1, -1)), ((3, 7), (1, 1)), ((15, 15), (-1, -1)), ((5, 5), (0, 0)), ((5, 5), (5, 5)),
                                       ((7, 2), (6, 2)), ((4, 4), (3, -1))])
def test_weight_table(win, zero):
    got, want = sc.twin().table(win, zero), np_table(win, zero)
    assert np.array_equal(sc.bits(got), sc.bits(want))
    assert got[win[1], win[0]] == (1.0 if not (want == 0).any() else 0.0)


def test_a_zero_zone_that_is_not_strictly_inside_equals_none(pmv):
    t = sc.twin()
    for win, zero in [((5, 5), (5, 5)), ((5, 5), (7, 0)), ((3, 7), (3, 1)), ((3, 7), (1, 7)), ((5, 5), (-1, 2)), ((5, 5), (2, -1))]:
        assert np.array_equal(sc.bits(t.table(win, zero)), sc.bits(t.table(win))), (win, zero)
    assert (t.table((5, 5), (4, 4)) == 0).sum() == 81 and (t.table((5, 5), (0, 0)) == 0).sum() == 1
    img, pts = gc.frame(pmv, 160, 120), sc.scene_points(pmv, 160, 120)[:40]
    a, b = t.refine(img, pts, zero_zone=(5, 5)), t.refine(img, pts)
    assert all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(a[:3], b[:3]))
    c = t.refine(img, pts, zero_zone=(2, 2))
    assert not np.array_equal(sc.bits(c[0]), sc.bits(b[0])), "a zero zone inside the window changes nothing: the comparison compares nothing"


PATCH_CASES = [(80.3, 60.7, (5, 5), True), (17.0, 23.0, (5, 5), True), (40.00001, 30.5, (3, 7), True), (6.0, 60.2, (5, 5), True), (5.9, 60.2, (5, 5), False),
               (2.25, 3.75, (5, 5), False), (0.0, 0.0, (5, 5), False), (159.0, 119.0, (5, 5), False), (-3.5, 10.0, (5, 5), False), (162.0, 60.0, (5, 5), False),
               (80.4, 117.6, (1, 1), False), (80.4, 116.0, (1, 1), True), (-40.0, -40.0, (2, 2), False), (300.0, 60.0, (15, 15), False), (80.0, 60.0, (15, 15), True)]


@pytest.mark.parametrize("cx, cy, win, fast", PATCH_CASES)
def test_one_patch_on_each_sampling_path(pmv, cx, cy, win, fast):
    img = gc.frame(pmv, 160, 120)
    got, got_fast = sc.twin().patch(img, cx, cy, win)
    want, want_fast = np_patch(img, cx, cy, win)
    assert got_fast == want_fast == fast
    assert np.array_equal(sc.bits(got), sc.bits(want)), np.argwhere(sc.bits(got) != sc.bits(want))[:4]


@pytest.mark.parametrize("w, h", sc.SIZES)
def test_one_update_step(pmv, w, h):
    img = gc.frame(pmv, w, h)
    pts = np.concatenate([sc.scene_points(pmv, w, h)[:12], sc.edge_points(w, h)[:14]])
    for win, zero in [((5, 5), (-1, -1)), ((3, 7), (1, 1))]:
        xy, it, fl, _ = sc.twin().refine(img, pts, win=win, zero_zone=zero, max_iter=1, eps=0.0, order=sc.SERIAL)
        for k, (x, y) in enumerate(pts):
            nx, ny, upd, flags = np_step(img, x, y, win, zero)
            if upd and not flags and (nx != x or ny != y):
                flags |= sc.CAP   # max_iter = 1 ended the loop with err > 0
            if abs(float(nx) - float(x)) > win[0] or abs(float(ny) - float(y)) > win[1]:
                nx, ny, flags = x, y, flags | sc.REVERTED
            assert (sc.bits(f32(nx)), sc.bits(f32(ny)), upd, flags) == (sc.bits(xy[k, 0]), sc.bits(xy[k, 1]), it[k], fl[k]), (k, x, y, win)


# ---- the two summation orders -----------------------------------------------------------------------------------------------------------
def _ulps(a, b):
    """distance in float32 steps between finite values of one sign region (monotone integer keys)"""
    def key(v):
        i = np.ascontiguousarray(v, f32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7fffffff), i)
    return np.abs(key(a) - key(b))


@pytest.mark.parametrize("w, h", sc.SIZES)
def test_kernel_order_is_within_one_ulp_of_the_serial_order_after_one_update(pmv, w, h):
    """The double sums of the two orders differ by rounding noise (relative 1e-14 and below), the update adds them to the position in
    double and rounds to float ONCE: the float results are equal or neighbours. Every point of the scene and of the edge set, no
    exception. The full runs are reported, not asserted: the orders may part ways after many iterations."""
    img = gc.frame(pmv, w, h)
    for edge in (False, True):
        pts = sc.edge_points(w, h) if edge else sc.scene_points(pmv, w, h)
        k = sc.refined(pmv, w, h, "one_iter", sc.KERNEL, edge)
        s = sc.refined(pmv, w, h, "one_iter", sc.SERIAL, edge)
        assert np.isfinite(k[0]).all() and np.isfinite(s[0]).all()
        d = _ulps(k[0], s[0])
        print(f"{w}x{h} {'edge' if edge else 'scene'}: {len(pts)} points, one update: {(d > 0).any(axis=1).sum()} differ, max {d.max()} ulp")
        assert d.max() <= 1, f"point {np.argwhere(d > 1)[:4]}"
        assert np.array_equal(k[1], s[1])
    kf, sf = sc.refined(pmv, w, h, "default", sc.KERNEL), sc.refined(pmv, w, h, "default", sc.SERIAL)
    differ = (sc.bits(kf[0]) != sc.bits(sf[0])).any(axis=1) | (kf[1] != sf[1]) | (kf[2] != sf[2])
    print(f"{w}x{h}: full runs (5, 5 | 30 | 0.01): {differ.sum()} of {len(differ)} points differ in a byte between the two orders")


# ---- properties --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [sc.SERIAL, sc.KERNEL], ids=["serial", "kernel"])
def test_flat_and_ramp_frames_return_every_point_unchanged(order):
    flat = np.full((60, 60), 93, np.uint8)
    ramp = gc.gradient_frame()
    for img in (flat, ramp):
        h, w = img.shape
        rng = np.random.default_rng(5)
        pts = np.concatenate([sc.edge_points(w, h), (rng.random((40, 2)) * [w, h]).astype(f32)])
        for name in ("default", "win1", "win3x7_zero1", "win15_full"):
            xy, it, fl, _ = sc.twin().refine(img, pts, order=order, **sc.PARAMS[name])
            assert np.array_equal(sc.bits(xy), sc.bits(pts)) and (it == 0).all() and (fl == sc.DET).all(), name


@pytest.mark.parametrize("w, h", sc.SIZES)
def test_the_full_criteria_never_make_fewer_updates(pmv, w, h):
    img, pts = gc.frame(pmv, w, h), sc.scene_points(pmv, w, h)
    for order in (sc.SERIAL, sc.KERNEL):
        full = sc.twin().refine(img, pts, max_iter=100, eps=0.0, order=order)
        dflt = sc.refined(pmv, w, h, "default", order)
        assert (full[1] >= dflt[1]).all()
        assert (full[1] > dflt[1]).any()


@pytest.mark.parametrize("w, h, first", [(160, 120, 150), (203, 87, 125)])
def test_the_scenes_compare_something(pmv, w, h, first):
    """shifted detector corners at (5, 5 | 30 | 0.01): most move, some hit the cap, some revert; both sampling paths are taken"""
    pts = sc.scene_points(pmv, w, h)
    assert len(pts) >= first
    for order in (sc.SERIAL, sc.KERNEL):
        xy, it, fl, fast = sc.refined(pmv, w, h, "default", order)
        moved = np.hypot(*(xy[:first] - pts[:first]).T) > 0.05
        cap, rev = (fl[:first] & sc.CAP) != 0, (fl[:first] & sc.REVERTED) != 0
        print(f"{w}x{h} order {order}: of {first}: {moved.sum()} moved > 0.05 px, {cap.sum()} hit the cap, {rev.sum()} reverted; updates max {it.max()}")
        assert moved.sum() > first // 2 and cap.any() and rev.any()
        assert (fast > 0).any() and (fast < it.astype(np.int32) + ((fl & (sc.DET | sc.LEFT)) == sc.DET)).any(), "both sampling paths"
    e = sc.refined(pmv, w, h, "default", sc.KERNEL, edge=True)
    assert (e[2] & sc.LEFT).any() or (e[2] & sc.REVERTED).any()
