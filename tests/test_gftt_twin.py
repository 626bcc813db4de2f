"""The CPU twin of pmv_detect_gftt_ex (tests/twin/gftt_twin.cpp) without a GPU: at the reference's arguments it is orc_gftt_cell byte for
byte; its response map equals an independent numpy restatement for every block size and both response kinds; the mask behaves as
cv::goodFeaturesToTrack's does - in particular the threshold follows the MASKED maximum, which post-filtering cannot reproduce."""
import numpy as np
import pytest

import gftt_common as gc

SIZE_IDS = dict(ids=lambda s: f"{s[0]}x{s[1]}")


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("size", gc.SIZES, **SIZE_IDS)
def test_at_the_reference_arguments_the_twin_is_the_oracle(pmv, orc, size):
    w, h = size
    img = gc.frame(pmv, w, h)
    cells = np.concatenate([pmv.grid_cells(w, h), gc.corner_cells(w, h)])
    total = 0
    for cell in cells:
        for max_corners in (20, 0):
            want_xy, want_eig = orc.gftt_cell(img, cell, max_corners, want_eig=True)
            xy, resp, _, _ = gc.twin().cell(img, cell, max_corners)
            assert np.array_equal(xy, want_xy), f"cell {cell}, max {max_corners}: corners differ"
            assert np.array_equal(_bits(resp), _bits(want_eig)), f"cell {cell}: eig map differs"
            total += len(xy)
    assert total > 50, "the scene has too few corners to compare anything"


def _mirror(idx, n):
    idx = np.asarray(idx).copy()
    if n == 1:
        return np.zeros_like(idx)
    while ((idx < 0) | (idx >= n)).any():
        idx = np.where(idx < 0, -idx, idx)
        idx = np.where(idx >= n, 2 * n - 2 - idx, idx)
    return idx


def _numpy_response(img, cell, b, harris, k):
    """float32 planes; the b*b shifted cov planes added in raster order into float64"""
    f32 = np.float32
    h, w = img.shape
    x0, y0, cw, ch = [int(v) for v in cell]
    ys = _mirror(np.arange(y0 - 1, y0 + ch + 1), h)
    xs = _mirror(np.arange(x0 - 1, x0 + cw + 1), w)
    P = img[np.ix_(ys, xs)].astype(f32)   # the cell with one pixel of the PARENT's border around it
    dscale = 1.0 / (4.0 * b * 255.0)
    k1, k2 = f32(1.0 * dscale), f32(2.0 * dscale)
    tl, tm, tr = P[:-2, :-2], P[:-2, 1:-1], P[:-2, 2:]
    ml, mr = P[1:-1, :-2], P[1:-1, 2:]
    bl, bm, br = P[2:, :-2], P[2:, 1:-1], P[2:, 2:]
    dx = ((tr - tl) + (br - bl)) * k1 + (mr - ml) * k2
    st = k1 * tl; st = st + k2 * tm; st = st + k1 * tr
    sb = k1 * bl; sb = sb + k2 * bm; sb = sb + k1 * br
    dy = sb - st
    assert dx.dtype == f32 and dy.dtype == f32
    cov = [dx * dx, dx * dy, dy * dy]
    an = b // 2
    s = [np.zeros((ch, cw), np.float64) for _ in range(3)]
    for j in range(-an, b - an):
        yy = _mirror(np.arange(ch) + j, ch)
        for i in range(-an, b - an):
            xx = _mirror(np.arange(cw) + i, cw)
            for q in range(3):
                s[q] = s[q] + cov[q][np.ix_(yy, xx)].astype(np.float64)
    s0, s1, s2 = [v.astype(f32) for v in s]
    if harris:
        det = s0 * s2 - s1 * s1
        tr_ = (s0 + s2).astype(np.float64)
        return (det.astype(np.float64) - (k * tr_) * tr_).astype(f32)
    a, c = s0 * f32(0.5), s2 * f32(0.5)
    return (a + c) - np.sqrt((a - c) * (a - c) + s1 * s1)


@pytest.mark.parametrize("cell", [(31, 20, 40, 33), (150, 60, 5, 4)], ids=["40x33", "5x4"])
@pytest.mark.parametrize("harris", [False, True], ids=["mineig", "harris"])
@pytest.mark.parametrize("b", [1, 2, 3, 4, 7, 15])
def test_response_map_equals_an_independent_numpy_restatement(pmv, b, harris, cell):
    img = gc.frame(pmv, 203, 87)
    want = _numpy_response(img, cell, b, harris, 0.04)
    got = gc.twin().response(img, cell, b, harris, 0.04)
    assert want.dtype == np.float32
    assert np.array_equal(_bits(got), _bits(want)), f"differs at {np.argwhere(_bits(got) != _bits(want))[:5]}"
    assert np.abs(got).max() > 0


@pytest.mark.parametrize("size", gc.SIZES, **SIZE_IDS)
@pytest.mark.parametrize("b, harris", [(3, False), (5, True)], ids=["3-mineig", "5-harris"])
def test_mask_properties(pmv, size, b, harris):
    w, h = size
    img = gc.frame(pmv, w, h)
    tw = gc.twin()
    kw = dict(block_size=b, use_harris=harris, k=0.04)
    for cell in pmv.grid_cells(w, h):
        plain = tw.corners(img, cell, 0, **kw)
        assert len(plain) > 10
        assert np.array_equal(tw.corners(img, cell, 0, mask=np.full((h, w), 255, np.uint8), **kw), plain), "an all-255 mask is no mask"
        assert np.array_equal(tw.corners(img, cell, 0, mask=np.full((h, w), 1, np.uint8), **kw), plain), "any non-zero byte allows"
        assert len(tw.corners(img, cell, 0, mask=np.zeros((h, w), np.uint8), **kw)) == 0, "an all-zero mask allows nothing"
        for name, m in gc.masks(w, h).items():
            xy = tw.corners(img, cell, 0, mask=m, **kw) + cell[:2]
            assert (m[xy[:, 1], xy[:, 0]] != 0).all(), f"{name}: a corner on a masked-out pixel"
        assert len(tw.corners(img, cell, 0, mask=gc.masks(w, h)["discs"], **kw)) > 5


@pytest.mark.parametrize("size", gc.SIZES, **SIZE_IDS)
def test_the_threshold_follows_the_masked_maximum(pmv, size):
    """blanking the strongest corner lowers the threshold: corners appear that the unmasked run had dropped, so filtering the unmasked list
    by the mask afterwards gives a different (shorter) list"""
    w, h = size
    cell = pmv.grid_cells(w, h)[0]
    img = gc.frame(pmv, w, h)
    m, plain, masked = gc.blanked_strongest(pmv, w, h, cell, quality=0.3)
    keep = m[plain[:, 1] + cell[1], plain[:, 0] + cell[0]] != 0
    post = plain[keep]
    assert not keep[0] and len(post) > 0
    _, _, max_plain, _ = gc.twin().cell(img, cell, 0, quality=0.3)
    _, _, max_masked, _ = gc.twin().cell(img, cell, 0, quality=0.3, mask=m)
    assert max_masked < max_plain
    assert not np.array_equal(masked, post), "the masked run equals post-filtering: the scene does not show the masked maximum at work"
    assert len(masked) > len(post)
