"""The yardstick of pmv_detect_gftt_frame where it has never been used: tests/twin/gftt_twin.cpp with a whole 517x261 region as its cell
(x above 255, pixel indices above 65 535) against an independent numpy selection on the twin's own response map, and the reason the call
exists: the whole-frame answer is not the union of the 255-grid's."""
import numpy as np
import pytest

import gftt_common as gc
import gftt_frame_common as gf


def _scene(pmv, name):
    return gf.rect_frame(pmv) if name == "rectangles" else gf.plateau_frame()


@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("min_dist", [0.0, 7.0, 30.0])
@pytest.mark.parametrize("name", ["rectangles", "plateau"])
def test_the_twin_on_a_whole_frame_is_the_numpy_selection(pmv, name, min_dist, masked):
    img = _scene(pmv, name)
    h, w = img.shape
    mask = gc.masks(w, h)["discs"] if masked else None
    for max_corners in (150, 0):
        xy, resp, mx, records = gc.twin().cell(img, gf.whole(img), max_corners, quality=0.01, min_dist=min_dist, mask=mask)
        want, n = gf.numpy_selection(resp, max_corners, 0.01, min_dist, mask)
        assert records == n and n > 100
        assert np.array_equal(xy, want), f"differs from index {np.flatnonzero((xy != want).any(axis=1))[:4] if len(xy) == len(want) else (len(xy), len(want))}"
    if name == "plateau" and not masked:
        # 512 records of one value: the order is the address alone, descending
        xy = gc.twin().corners(img, gf.whole(img), 0, quality=0.01, min_dist=0.0)
        idx = xy[:, 1].astype(np.int64) * w + xy[:, 0]
        assert len(xy) == 512 and (np.diff(idx) < 0).all() and xy[:, 0].max() > 255 and idx.max() > 65535


def test_the_whole_frame_is_not_the_union_of_the_grid_cells(pmv):
    """(150, 0.01, 30) on the 517x261 scene: the threshold, the order, the cut and min_dist are global in the whole-frame call. The figures are
    the twin's on this repository's synthetic scene (the grid cells each with the frame's limit)."""
    img = gf.rect_frame(pmv)
    kw = dict(quality=0.01, min_dist=30.0)
    whole = gc.twin().corners(img, gf.whole(img), 150, **kw)
    grid = np.concatenate([gc.twin().corners(img, c, 150, **kw) + np.asarray(c[:2]) for c in pmv.grid_cells(gf.W1, gf.H1)])
    common = set(map(tuple, whole)) & set(map(tuple, grid))
    print(f"whole frame {len(whole)} corners, 255-grid {len(grid)}, common {len(common)}")
    assert (len(whole), len(grid), len(common)) == (92, 107, 87)
    assert len(common) < len(whole) < len(grid)
