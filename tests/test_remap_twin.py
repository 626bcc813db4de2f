"""The CPU twin of pmv_frames_remap (tests/twin/remap_twin.cpp) and the host map builder without a GPU: the twin equals a second, independent
numpy restatement of the contract byte for byte on every case of the table; the table reaches what it is meant to reach (asserted on the
twin's own statistics, so that no case can silently miss its branch); pmv_undistort_map_build agrees with a float64 restatement of its
formula to one float ulp of the coordinate."""
import numpy as np
import pytest

import remap_common as rc

INT_MIN = -2 ** 31


def _fixed(m):
    """cv's conversion of a float map: (integer part saturated to int16, 5-bit fraction)"""
    v = np.asarray(m, np.float32) * np.float32(32.0)
    assert v.dtype == np.float32
    ok = np.isfinite(v) & (v >= np.float32(-2 ** 31)) & (v < np.float32(2 ** 31))
    s = np.full(v.shape, INT_MIN, np.int64)
    s[ok] = np.rint(v[ok].astype(np.float64)).astype(np.int64)   # rint: half to even; a float32 is exact in float64
    return np.clip(s >> 5, -32768, 32767), s & 31


def _restate(img, map_x, map_y, border):
    img = np.asarray(img, np.uint8)
    h, w = img.shape
    ix, fx = _fixed(map_x)
    iy, fy = _fixed(map_y)
    padded = np.full((h + 2, w + 2), border, np.int64)      # one ring of border pixels: every tap beyond it is the border value as well
    padded[1:-1, 1:-1] = img

    def tap(x, y):
        return padded[np.clip(y, -1, h) + 1, np.clip(x, -1, w) + 1]
    acc = (32 - fy) * (32 - fx) * tap(ix, iy) + (32 - fy) * fx * tap(ix + 1, iy) + fy * (32 - fx) * tap(ix, iy + 1) + fy * fx * tap(ix + 1, iy + 1)
    return ((acc + 512) >> 10).astype(np.uint8)


@pytest.mark.parametrize("case", rc.CASES, ids=rc.case_id)
def test_twin_equals_the_numpy_restatement(pmv, case):
    name, w, h, border = case
    got, _ = rc.remapped(pmv, case)
    want = _restate(rc.image(pmv, w, h), *rc.maps(pmv, name, w, h), border)
    assert got.shape == want.shape == (h, w) and np.array_equal(got, want), f"{int((got != want).sum())} of {w * h} bytes differ"
    if name != "identity":
        assert not np.array_equal(got, rc.image(pmv, w, h)), "the remapped image is the input"


def test_the_table_reaches_what_it_is_meant_to(pmv):
    stats = {rc.case_id(c): rc.remapped(pmv, c)[1] for c in rc.CASES}
    for c in rc.CASES:
        name, w, h, border = c
        s = stats[rc.case_id(c)]
        assert s["inside"] + s["outside"] + s["mixed"] == w * h
        if name == "undistort06":
            # all-inside pixels, all-outside pixels, and mixed pixels on each of the four sides, at all three sizes
            assert s["inside"] > 0 and s["outside"] > 0 and min(s["left"], s["right"], s["above"], s["below"]) > 0, (c, s)
            if (w, h) != (41, 40):
                assert len(s["pairs"]) == 1024, (c, len(s["pairs"]))
        if name == "undistort":
            assert s["outside"] == 0 and s["mixed"] == 0 and s["inside"] == w * h, (c, s)
    assert stats["identity-160x120-b0"]["pairs"] == {(0, 0)} and stats["identity-160x120-b0"]["mixed"] == 160 + 120 - 1
    s = stats["shift-160x120-b0"]
    assert s["pairs"] == {(0, 0)} and s["outside"] > 0 and s["right"] > 0 and s["above"] > 0 and s["left"] == s["below"] == 0, s
    assert stats["fraction-160x120-b0"]["pairs"] == {(27, 13)}
    # ties: 32 (j + k / 64) = 32 j + k / 2 with odd k rounds to the even neighbour: k = 1 -> 0, 3 -> 2, 5 -> 2, 7 -> 4, ..
    even = {int(np.rint(k / 2)) % 32 for k in range(1, 64, 2)}
    assert {fx for _, fx in stats["ties-160x120-b0"]["pairs"]} == even and {fy for fy, _ in stats["ties-160x120-b0"]["pairs"]} == even
    assert all(f % 2 == 0 for f in even)
    s = stats["turn-160x120-b0"]
    assert s["outside"] > 0 and s["inside"] > 0


def test_known_answers(pmv):
    tw = rc.twin()
    img = rc.image(pmv, 160, 120)
    ident = rc.maps(pmv, "identity", 160, 120)
    assert np.array_equal(tw.apply(img, *ident, 0)[0], img) and np.array_equal(tw.apply(img, *ident, 255)[0], img)
    # the integer shift: dst(x, y) = src(x + 3, y - 2), the border value where that leaves the image
    for border in (0, 200):
        got = rc.remapped(pmv, ("shift", 160, 120, border))[0]
        want = np.full_like(img, border)
        want[2:, :-3] = img[:-2, 3:]
        assert np.array_equal(got, want)
    # half to even: map 0.5 / 32 = 1 / 64 rounds to fraction 0 (a copy), 3 / 64 to fraction 2
    j, i = ident
    assert np.array_equal(tw.apply(img, j + np.float32(1 / 64), i, 0)[0], img)
    assert tw.apply(img, j + np.float32(3 / 64), i, 0)[1]["pairs"] == {(0, 2)}
    # negative coordinates: the shift is arithmetic (floor), -1 / 32 is ix = -1, fx = 31
    got, st = tw.apply(img, j - np.float32(1 / 32), i, 0)
    assert st["pairs"] == {(0, 31)} and st["left"] == 120
    assert np.array_equal(got[:, 0], (31 * img[:, 0].astype(np.int64) * 32 + 512) >> 10)
    # NaN, +-inf and +-1e9 give the border value; the pixels around them are the input's
    for border in (0, 77):
        got = tw.apply(img, *rc.maps(pmv, "special", 160, 120), border)[0]
        hit = np.zeros(img.shape, bool)
        for r, c, _, _ in rc.SPECIALS:
            hit[r, c] = True
            assert got[r, c] == border, (r, c, got[r, c])
        assert np.array_equal(got[~hit], img[~hit])
    # a constant image and a constant border of the same value stay constant whatever the map (the weights sum to 1024)
    flat = np.full((120, 160), 93, np.uint8)
    assert (tw.apply(flat, *rc.maps(pmv, "undistort06", 160, 120), 93)[0] == 93).all()


def _builder_restated(K, dist, R, new_K, w, h):
    """section 4 of the contract in numpy float64: whole-array operations, the inverse from cofactors"""
    K, dist = np.asarray(K, np.float64), np.asarray(dist, np.float64)
    A = np.asarray(new_K if new_K is not None else K, np.float64) @ (np.eye(3) if R is None else np.asarray(R, np.float64))
    cof = np.empty((3, 3))
    for r in range(3):
        for c in range(3):
            m = np.delete(np.delete(A, r, 0), c, 1)
            cof[r, c] = (-1) ** (r + c) * (m[0, 0] * m[1, 1] - m[0, 1] * m[1, 0])
    inv = cof.T / (A[0] @ cof[0])
    j, i = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    X, Y, W = (inv[r, 0] * j + inv[r, 1] * i + inv[r, 2] for r in range(3))
    x, y = X / W, Y / W
    r2 = x * x + y * y
    k1, k2, p1, p2, k3, k4, k5, k6 = dist
    kr = (1 + ((k3 * r2 + k2) * r2 + k1) * r2) / (1 + ((k6 * r2 + k5) * r2 + k4) * r2)
    xd = x * kr + p1 * (2 * x * y) + p2 * (r2 + 2 * x * x)
    yd = y * kr + p1 * (r2 + 2 * y * y) + p2 * (2 * x * y)
    return K[0, 0] * xd + K[0, 2], K[1, 1] * yd + K[1, 2]


def _rot(rx, ry, rz):
    def r(a, i, j):
        m = np.eye(3)
        m[i, i] = m[j, j] = np.cos(a)
        m[i, j], m[j, i] = -np.sin(a), np.sin(a)
        return m
    return r(rx, 1, 2) @ r(ry, 2, 0) @ r(rz, 0, 1)


@pytest.mark.parametrize("size", rc.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_builder_against_the_float64_restatement(pmv, size):
    w, h = size
    K = rc.camera(w, h)
    full = (-0.35, 0.12, 0.001, -0.0005, -0.02, 0.01, -0.003, 0.0007)
    for dist, R, new_K in ((rc.DIST, None, None), (rc.DIST, None, rc.new_camera(w, h, 0.6)), (full, _rot(0.02, -0.03, 0.01), rc.new_camera(w, h, 0.8)),
                           (rc.DIST[:5], _rot(-0.01, 0.02, 0.3), None)):
        mx, my = pmv.undistort_map(K, dist, (w, h), R=R, new_K=new_K)
        assert mx.dtype == my.dtype == np.float32 and mx.shape == my.shape == (h, w)
        d8 = np.zeros(8)
        d8[:len(dist)] = dist
        wx, wy = _builder_restated(K, d8, R, new_K, w, h)
        assert max(np.abs(wx).max(), np.abs(wy).max()) < 2048
        # a last-bit difference in double can move the float rounding by one ulp of the largest coordinate: 2^-13 px below 2048
        ex, ey = np.abs(mx.astype(np.float64) - wx).max(), np.abs(my.astype(np.float64) - wy).max()
        print(f"{w}x{h}: max |map_x - restated| = {ex:.3g}, max |map_y - restated| = {ey:.3g}")
        assert ex <= 2.0 ** -13 and ey <= 2.0 ** -13


def test_zero_distortion_reproduces_the_image(pmv):
    for w, h in rc.SIZES:
        K = rc.camera(w, h)
        mx, my = pmv.undistort_map(K, np.zeros(8), (w, h), new_K=K)
        got, st = rc.twin().apply(rc.image(pmv, w, h), mx, my, 0)
        assert np.array_equal(got, rc.image(pmv, w, h)) and st["pairs"] == {(0, 0)}


def test_builder_refusals(pmv):
    K = rc.camera(160, 120)
    singular = K.copy()
    singular[1] = 2 * singular[0]
    for kw in (dict(new_K=singular), dict(new_K=np.zeros((3, 3))), dict(R=np.ones((3, 3)))):
        with pytest.raises(pmv.PmvError) as e:
            pmv.undistort_map(K, rc.DIST, (160, 120), **kw)
        assert e.value.code == -2 and "singular" in str(e.value), str(e.value)
    lib = pmv.load_library()
    import ctypes as C
    f64, f32 = C.POINTER(C.c_double), C.POINTER(C.c_float)
    lib.pmv_undistort_map_build.argtypes = [f64, f64, f64, f64, C.c_int, C.c_int, f32, f32]
    k9, d8 = (C.c_double * 9)(*K.ravel()), (C.c_double * 8)(*rc.DIST)
    out = (C.c_float * 16)()
    assert lib.pmv_undistort_map_build(k9, d8, None, None, 4, 4, out, out) == 0
    for args in ((None, d8, None, None, 4, 4, out, out), (k9, None, None, None, 4, 4, out, out), (k9, d8, None, None, 4, 4, None, out),
                 (k9, d8, None, None, 4, 4, out, None), (k9, d8, None, None, 0, 4, out, out), (k9, d8, None, None, 4, -1, out, out)):
        assert lib.pmv_undistort_map_build(*args) == -2
    for bad in (dict(size=(0, 4)), dict(size=5), dict(dist=np.zeros(9)), dict(K=np.eye(4))):
        kw = dict(K=K, dist=rc.DIST, size=(8, 8))
        kw.update(bad)
        with pytest.raises(ValueError):
            pmv.undistort_map(**kw)
