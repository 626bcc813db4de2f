"""The CPU twin of pmv_frames_clahe (tests/twin/clahe_twin.cpp) without a GPU: it equals a second, independent numpy restatement of the five
steps of the contract byte for byte on every case of the table, it gives the known answers, and the table reaches the branches it is
meant to reach (asserted on the twin's own statistics, so that no case can silently miss its branch)."""
import numpy as np
import pytest

import clahe_common as cc


def _restate(img, clip_limit, tiles):
    """cv::CLAHE::apply, vectorised: the histogram of a tile by bincount, the redistribution in its closed form (bin i receives the residual
    increment iff i % step == 0 and i // step < residual), the interpolation over whole index planes. float32 throughout where cv uses float."""
    f32 = np.float32
    img = np.asarray(img, np.uint8)
    h, w = img.shape
    tx, ty = tiles
    ext = img
    if w % tx or h % ty:
        ext = np.pad(img, ((0, ty - h % ty), (0, tx - w % tx)), mode="reflect")   # numpy's "reflect" is cv's BORDER_REFLECT_101
    eh, ew = ext.shape
    tw, th = ew // tx, eh // ty
    area = tw * th
    lut_scale = f32(255) / f32(area)
    cl = max(int(min(clip_limit * area / 256, float(area))), 1) if clip_limit > 0 else 0
    luts = np.zeros((ty, tx, 256), np.uint8)
    bins = np.arange(256)
    for j in range(ty):
        for i in range(tx):
            hist = np.bincount(ext[j * th:(j + 1) * th, i * tw:(i + 1) * tw].ravel(), minlength=256).astype(np.int64)
            if cl > 0:
                clipped = int(np.maximum(hist - cl, 0).sum())
                hist = np.minimum(hist, cl)
                batch, residual = divmod(clipped, 256)
                hist = hist + batch
                if residual:
                    step = max(256 // residual, 1)
                    hist[(bins % step == 0) & (bins // step < residual)] += 1
            assert hist.sum() == area
            luts[j, i] = np.clip(np.rint(np.cumsum(hist).astype(f32) * lut_scale), 0, 255).astype(np.uint8)   # rint: half to even

    def axis(n, inv, tiles_n):
        t = np.arange(n).astype(f32) * inv - f32(0.5)
        t1 = np.floor(t).astype(np.int64)
        a = t - t1.astype(f32)
        return np.maximum(t1, 0), np.minimum(t1 + 1, tiles_n - 1), a, f32(1.0) - a
    tx1, tx2, xa, xa1 = axis(w, f32(1.0) / f32(tw), tx)
    ty1, ty2, ya, ya1 = axis(h, f32(1.0) / f32(th), ty)
    v = img.astype(np.int64)

    def look(tyi, txi):
        return luts[tyi[:, None], txi[None, :], v].astype(f32)
    top = look(ty1, tx1) * xa1[None, :] + look(ty1, tx2) * xa[None, :]
    bot = look(ty2, tx1) * xa1[None, :] + look(ty2, tx2) * xa[None, :]
    res = top * ya1[:, None] + bot * ya[:, None]
    assert res.dtype == np.float32
    return np.clip(np.rint(res), 0, 255).astype(np.uint8)


@pytest.mark.parametrize("case", cc.CASES, ids=cc.case_id)
def test_twin_equals_the_numpy_restatement(pmv, case):
    w, h, clip, tiles = case
    got, stats = cc.equalised(pmv, case)
    want = _restate(cc.image(pmv, w, h), clip, tiles)
    assert got.shape == want.shape == (h, w) and np.array_equal(got, want), f"{int((got != want).sum())} of {w * h} bytes differ"
    assert not np.array_equal(got, cc.image(pmv, w, h)), "the equalised image is the input"
    if clip in cc.CLIPPING:
        assert stats["clipped"] >= 1 and stats["residual"] >= 1, stats
    if clip in (0.0, 1000.0):
        assert stats["clipped"] == 0 and stats["residual"] == 0, stats


def test_the_table_reaches_what_it_is_meant_to(pmv):
    stats = {cc.case_id(c): cc.equalised(pmv, c)[1] for c in cc.CASES}
    s = stats["160x120-clip2-8x8"]
    assert s["ext"] == (0, 0) and s["tile"] == (20, 15) and s["cl"] == 2 and s["clipped"] == 64, s
    assert stats["160x120-clip0-8x8"]["cl"] == 0 and stats["160x120-clip40-8x8"]["cl"] == 46
    assert stats["203x87-clip2-8x8"]["ext"] == (5, 1) and stats["203x87-clip3-4x3"]["ext"] == (1, 3)
    assert stats["203x87-clip3-4x3"]["tile"] == (51, 30)
    assert stats["41x40-clip2-8x8"]["ext"] == (7, 8) and stats["41x40-clip2-8x8"]["tile"] == (6, 6) and stats["41x40-clip2-8x8"]["cl"] == 1
    assert stats["40x41-clip2-8x8"]["ext"] == (8, 7) and stats["40x41-clip2-8x8"]["tile"] == (6, 6)
    assert stats["64x48-clip4-1x1"]["tile"] == (64, 48)
    assert stats["75x53-clip0.5-16x16"]["ext"] == (5, 11) and stats["75x53-clip0.5-16x16"]["tile"] == (5, 4) and stats["75x53-clip0.5-16x16"]["cl"] == 1
    steps = set().union(*(s["steps"] for s in stats.values()))
    assert 1 in steps and any(s > 1 for s in steps), steps


def test_known_answers():
    tw = cc.twin()
    # a constant image without clipping: the one occupied bin's running sum is the whole area, every LUT entry from it on is 255
    for value in (0, 77, 255):
        out, stats = tw.apply(np.full((48, 56), value, np.uint8), 0.0, (8, 8))
        assert (out == 255).all() and stats["cl"] == 0 and stats["ext"] == (0, 0) and stats["tile"] == (7, 6)
    # each of the 256 values 16 times in one tile: lut[i] = rint((i + 1) * 16 * 255 / 4096), applied to every pixel (one tile: no interpolation)
    img = np.random.default_rng(1).permutation(np.repeat(np.arange(256, dtype=np.uint8), 16)).reshape(64, 64)
    out, stats = tw.apply(img, 0.0, (1, 1))
    lut = np.rint((np.arange(256) + 1).astype(np.float32) * np.float32(16) * (np.float32(255) / np.float32(4096))).astype(np.uint8)
    assert np.array_equal(lut, np.rint((np.arange(256) + 1) * 16 * 255 / 4096).astype(np.uint8))   # (exact in float32 as well)
    assert np.array_equal(out, lut[img]) and stats["tile"] == (64, 64)
    # the extension quirk and the clip constant
    rng = np.random.default_rng(2)
    assert tw.apply(rng.integers(0, 256, (40, 41), dtype=np.uint8), 2.0, (8, 8))[1]["ext"] == (7, 8)
    s = tw.apply(rng.integers(0, 256, (41, 40), dtype=np.uint8), 2.0, (8, 8))[1]
    assert s["ext"] == (8, 7) and s["tile"] == (6, 6) and s["cl"] == 1    # clip_limit 2.0 on a 6x6 tile: (int)(2 * 36 / 256) = 0 -> 1
    # a clip limit beyond every bin changes nothing against no clipping at all ... but is not the same as 0 = off for a flat image
    img = rng.integers(0, 256, (60, 80), dtype=np.uint8)
    assert np.array_equal(tw.apply(img, 1e300, (4, 4))[0], tw.apply(img, 0.0, (4, 4))[0])


def test_a_second_application_equalises_again(pmv):
    case = cc.CASES[0]
    once, _ = cc.equalised(pmv, case)
    twice, _ = cc.twin().apply(once, case[2], case[3])
    assert not np.array_equal(once, twice)
