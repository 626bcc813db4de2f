"""The CPU twin of pmv_detect_gftt_refill's mask half (tests/twin/refill_twin.cpp) against an independent numpy setMask
(tests/refill_common.py), and the half-width table against the literal Circle() painting for every radius. No GPU."""
import numpy as np
import pytest

import refill_common as rc


def _same(w, h, xy, radius, prio=None, base=None, what=""):
    k, m = rc.twin().mask(w, h, xy, radius, prio, base)
    nk, nm = rc.np_setmask(w, h, xy, radius, prio, base)
    assert np.array_equal(k, nk), f"{what}: keep bytes differ at {np.flatnonzero(k != nk)[:6]}"
    assert np.array_equal(m, nm), f"{what}: {int((m != nm).sum())} mask bytes differ"
    return k, m


@pytest.mark.parametrize("radius", [10, 30])
@pytest.mark.parametrize("size", [(rc.W1, rc.H1), (96, 80)], ids=["517x261", "96x80"])
def test_random_tracks_against_numpy(size, radius):
    w, h = size
    n = 300 if w == rc.W1 else 120
    xy, prio = rc.tracks(w, h, n)
    for p in (prio, None):
        k, m = _same(w, h, xy, radius, p, None, (size, radius, p is not None))
        print(f"{w}x{h}, r = {radius}, priorities {p is not None}: kept {int(k.sum())} of {n}")
        assert 0 < k.sum() < n, "the case is empty: nothing or everything is kept"
        assert (m == 0).any() and (m == 255).any()


def test_discs_clipped_at_all_edges_and_corners():
    w, h, r = 96, 80, 13
    pts = [(0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1), (w // 2, 0), (w // 2, h - 1), (0, h // 2), (w - 1, h // 2), (3, 20), (w - 4, 60), (70, 77)]
    k, m = _same(w, h, np.asarray(pts, np.float32), r, None, None, "edges")
    assert k.all(), "the points are further apart than a disc"
    assert m[0, 0] == 0 and m[h - 1, w - 1] == 0 and m[0, w - 1] == 0 and m[h - 1, 0] == 0 and m[h // 2, w // 2] == 255


def test_duplicates_keep_the_first_in_order():
    w, h = 96, 80
    xy = np.asarray([(20, 20), (20, 20), (60, 50), (20, 20), (60, 50)], np.float32)
    k, _ = _same(w, h, xy, 0, None, None, "duplicates, radius 0")
    assert k.tolist() == [1, 0, 1, 0, 0]
    k, _ = _same(w, h, xy, 0, np.asarray([0, 5, 1, 9, 1], np.int32), None, "duplicates with priorities")
    assert k.tolist() == [0, 0, 1, 1, 0], "the highest priority of a position wins; among equals the lower index"


def test_equal_priorities_fall_back_to_the_index():
    w, h = 96, 80
    xy = np.asarray([(30, 30), (33, 30), (36, 30), (70, 60)], np.float32)
    same = np.full(4, 7, np.int32)
    k_none, m_none = _same(w, h, xy, 4, None, None, "no priorities")
    k_same, m_same = _same(w, h, xy, 4, same, None, "equal priorities")
    assert np.array_equal(k_none, k_same) and np.array_equal(m_none, m_same)
    assert k_same.tolist() == [1, 0, 1, 1]
    k, _ = _same(w, h, xy, 4, np.asarray([-2147483648, 2147483647, 0, 0], np.int32), None, "the int32 extremes")
    assert k.tolist() == [0, 1, 0, 1]


@pytest.mark.parametrize("radius", [0, 255])
def test_radius_0_and_255(radius):
    w, h = rc.W1, rc.H1
    xy, prio = rc.tracks(w, h, 300)
    k, m = _same(w, h, xy, radius, prio, None, f"radius {radius}")
    if radius == 0:
        pts = rc.np_round(xy)
        assert int((m == 0).sum()) == len({(int(x), int(y)) for x, y in pts}) == int(k.sum()), "radius 0 clears the centre pixel only"
    else:
        assert 0 < k.sum() < 300


def test_half_way_coordinates_round_to_even():
    got = rc.twin().positions(np.asarray([(2.5, 3.5), (-0.5, 0.5), (1.5, 4.4999), (7.5, 8.5)], np.float32))
    assert got.tolist() == [[2, 4], [0, 0], [2, 4], [8, 8]]
    assert np.array_equal(got, rc.np_round(np.asarray([(2.5, 3.5), (-0.5, 0.5), (1.5, 4.4999), (7.5, 8.5)], np.float32)))
    k, m = _same(40, 40, np.asarray([(2.5, 3.5), (-0.5, 0.5)], np.float32), 0, None, None, "half-way")
    assert k.tolist() == [1, 1] and m[4, 2] == 0 and m[0, 0] == 0 and int((m == 0).sum()) == 2


def test_a_base_mask_with_0_128_255_and_a_stride_above_w():
    w, h = rc.W1, rc.H1
    base = rc.base_mask(w, h)
    assert base.strides[0] > w and set(np.unique(base)) == {0, 128, 255}
    xy, prio = rc.tracks(w, h, 300)
    k, m = _same(w, h, xy, 10, prio, base, "base mask")
    pts = rc.np_round(xy)
    under = base[pts[:, 1], pts[:, 0]]
    assert (under == 0).any() and (under == 128).any() and (under == 255).any()
    assert not k[under != 255].any(), "a track on a base byte other than 255 is dropped"
    assert 0 < k.sum() < (under == 255).sum()
    assert np.array_equal(m[m != 0], np.asarray(base)[m != 0]) and (m[np.asarray(base) == 0] == 0).all()
    assert (m == 128).any()


def test_the_half_width_table_is_the_literal_painting_for_every_radius():
    euclid = []
    for r in range(0, 256):
        side = 2 * r + 5
        img = np.full((side, side), 255, np.uint8)
        c = r + 2
        rc.twin().circle(img, c, c, r)
        hw = rc.twin().halfwidths(r)
        assert np.array_equal(hw, rc.np_halfwidths(r)), f"radius {r}: the twin's table is not the numpy recurrence's"
        want = np.full((side, side), 255, np.uint8)
        for d in range(-r, r + 1):
            want[c + d, c - hw[abs(d)]: c + hw[abs(d)] + 1] = 0
        assert np.array_equal(img, want), f"radius {r}: the table is not what Circle() paints"
        yy, xx = np.mgrid[0:side, 0:side]
        euclid.append(bool(np.array_equal(img == 0, (xx - c) ** 2 + (yy - c) ** 2 <= r * r)))
    differ = [r for r, e in enumerate(euclid) if not e]
    print(f"Circle() equals the Euclidean disc x^2 + y^2 <= r^2 at {sum(euclid)} of 256 radii; it differs at {differ[:20]}{' ...' if len(differ) > 20 else ''}")


def test_a_clipped_literal_disc_is_the_unclipped_one_cut_to_the_image():
    """the clipped branch of Circle() paints what the table says, cut at the border - for centres on and next to every border"""
    w, h = 37, 29
    for r in (0, 1, 2, 5, 12, 40):
        hw = rc.twin().halfwidths(r)
        for cx, cy in [(0, 0), (w - 1, h - 1), (1, h - 2), (w - 2, 1), (r, r), (w - 1 - r if w - 1 - r >= 0 else 0, 5), (18, 14)]:
            img = np.full((h, w), 255, np.uint8)
            rc.twin().circle(img, cx, cy, r)
            want = np.full((h, w), 255, np.uint8)
            for d in range(-r, r + 1):
                if 0 <= cy + d < h:
                    want[cy + d, max(cx - hw[abs(d)], 0): min(cx + hw[abs(d)], w - 1) + 1] = 0
            assert np.array_equal(img, want), (r, cx, cy)
