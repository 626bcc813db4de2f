"""pmv_detect_gftt_frame on the GPU: every case against the CPU twin (tests/twin/gftt_twin.cpp) with the region as its cell, bit for bit -
the corner list, the count and the number of records above the threshold -, or against pmv_detect_gftt_ex where a region is a cell. One
768x512 context, four slots (tests/gftt_frame_common.py): the frames are loaded into the slots as the tests need them."""
import ctypes as C

import numpy as np
import pytest

import gftt_common as gc
import gftt_frame_common as gf

pytestmark = pytest.mark.gpu

INVALID, CAPACITY, OVERFLOW = gf.INVALID, gf.CAPACITY, gf.OVERFLOW
_state = {"slots": {}}
SETTINGS = [(150, 0.01, 30.0), (500, 0.01, 7.0), (0, 0.01, 10.0)]   # (max_corners, quality, min_dist); 0 = no limit


def _ctx(pmv, gpu_ctx_factory):
    if "ctx" not in _state:
        _state["ctx"] = gpu_ctx_factory(gf.W2, gf.H2, n_slots=4, max_tracks=256)
    _state["ctx"].debug_gftt_general(False)
    return _state["ctx"]


def _image(pmv, name):
    kind, w, h = name
    return {"rect": lambda: gf.rect_frame(pmv, w, h), "plateau": lambda: gf.plateau_frame(w, h), "noise": lambda: gf.noise(w, h)}[kind]()


def _load(pmv, ctx, slot, name):
    """the image `name` = (kind, w, h) in `slot` (uploaded when the slot holds another one)"""
    img = _image(pmv, name)
    if _state["slots"].get(slot) != name:
        ctx.frame_upload(slot, img)
        _state["slots"][slot] = name
    return img


def _against_the_twin(ctx, img, slot, roi, max_corners, what, **kw):
    want, records = gf.twin_region(img, gf.whole(img) if roi is None else roi, max_corners, **kw)
    got = ctx.detect_gftt_frame(slot, max_corners, roi=roi, **kw)
    stats = ctx.debug_gftt_frame_stats()
    print(f"{what}: {len(got)} corners, {records} records above the threshold, {stats[4]} off-chip")
    assert len(got) == len(want), f"{what}: {len(got)} corners, the twin has {len(want)}"
    assert np.array_equal(got, want), f"{what}: corners differ from index {np.flatnonzero((got != want).any(axis=1))[:4]}"
    assert stats[3] == records, f"{what}: {stats[3]} records above the threshold, the twin has {records}"
    return len(want), records, stats


@pytest.mark.parametrize("b", [1, 2, 3, 5, 15])
@pytest.mark.parametrize("size", [(gf.W1, gf.H1), (gf.W2, gf.H2)], ids=["517x261", "768x512"])
def test_sweep_of_block_sizes_against_the_twin(pmv, gpu_ctx_factory, size, b):
    ctx = _ctx(pmv, gpu_ctx_factory)
    slot = 0 if size == (gf.W1, gf.H1) else 1
    img = _load(pmv, ctx, slot, ("rect",) + size)
    total = 0
    for mc, q, d in SETTINGS:
        total += _against_the_twin(ctx, img, slot, None, mc, (size, b, mc, d), quality=q, min_dist=d, block_size=b)[0]
    assert total > 100, "the scene gives too few corners to compare anything"


@pytest.mark.parametrize("size", [(gf.W1, gf.H1), (gf.W2, gf.H2)], ids=["517x261", "768x512"])
def test_harris_against_the_twin(pmv, gpu_ctx_factory, size):
    ctx = _ctx(pmv, gpu_ctx_factory)
    slot = 0 if size == (gf.W1, gf.H1) else 1
    img = _load(pmv, ctx, slot, ("rect",) + size)
    total = 0
    for mc, q, d in SETTINGS:
        for b in (3, 5):
            total += _against_the_twin(ctx, img, slot, None, mc, (size, "harris", b, mc), quality=q, min_dist=d, block_size=b, use_harris=True, k=0.04)[0]
    assert total > 100


@pytest.mark.parametrize("b", [3, 5])
@pytest.mark.parametrize("name", ["discs", "checker", "zero", "roi"])
def test_masks(pmv, gpu_ctx_factory, name, b):
    """517x261: discs of radius 7 around 60 points, a checkerboard of single pixels, all-zero (nothing comes back) and the disc mask as a view
    into a larger array (mask_stride > w)"""
    ctx = _ctx(pmv, gpu_ctx_factory)
    img = _load(pmv, ctx, 0, ("rect", gf.W1, gf.H1))
    m = gc.masks(gf.W1, gf.H1)[name]
    assert m.shape == (gf.H1, gf.W1) and (name != "roi" or m.strides[0] > gf.W1)
    for mc, q, d in SETTINGS:
        n, _, _ = _against_the_twin(ctx, img, 0, None, mc, ("mask", name, b, mc), quality=q, min_dist=d, block_size=b, mask=m)
        assert (n == 0) == (name == "zero")
    # a region of the masked frame sees its own rectangle of the mask
    _against_the_twin(ctx, img, 0, np.asarray([37, 11, 301, 200], np.int32), 500, ("mask region", name, b), quality=0.01, min_dist=7.0, block_size=b, mask=m)


def test_both_pass_1_kernels_give_the_same_bytes(pmv, gpu_ctx_factory):
    """the defaults (3, no Harris, no mask) run the tuned tile code, with pmv_debug_gftt_general the general one; both are booked under the two
    existing profiling classes, one launch each"""
    ctx = _ctx(pmv, gpu_ctx_factory)
    for slot, size in ((0, (gf.W1, gf.H1)), (1, (gf.W2, gf.H2))):
        img = _load(pmv, ctx, slot, ("rect",) + size)
        for mc, q, d in SETTINGS:
            want, _ = gf.twin_region(img, gf.whole(img), mc, quality=q, min_dist=d)
            ctx.prof_enable(True)
            tuned = ctx.detect_gftt_frame(slot, mc, q, d, k=123.0)
            prof_tuned = ctx.prof_read()
            ctx.debug_gftt_general(True)
            ctx.prof_enable(True)
            general = ctx.detect_gftt_frame(slot, mc, q, d)
            prof_general = ctx.prof_read()
            ctx.prof_enable(False)
            ctx.debug_gftt_general(False)
            assert np.array_equal(tuned, want) and np.array_equal(general, want)
            for prof in (prof_tuned, prof_general):
                assert {k: v[0] for k, v in prof.items()} == {"k_gftt_cand": 1, "k_gftt_pick": 1}
    ctx.lib.pmv_prof_kernel_name.restype = C.c_char_p
    classes = [ctx.lib.pmv_prof_kernel_name(i).decode() for i in range(ctx.lib.pmv_prof_kernel_count())]
    assert [c for c in classes if "gftt" in c] == ["k_gftt_cand", "k_gftt_pick"], "no new profiling class"


def test_regions(pmv, gpu_ctx_factory):
    """an inner region, the four frame corners, 3x3, a strip narrower than a tile, the whole frame given explicitly and as NULL"""
    ctx = _ctx(pmv, gpu_ctx_factory)
    img = _load(pmv, ctx, 0, ("rect", gf.W1, gf.H1))
    w, h = gf.W1, gf.H1
    rois = [(37, 11, 301, 200), (0, 0, 300, 140), (w - 300, 0, 300, 140), (0, h - 140, 300, 140), (w - 300, h - 140, 300, 140), (100, 60, 3, 3), (411, 0, 5, 261), (0, 0, w, h)]
    for roi in rois:
        roi = np.asarray(roi, np.int32)
        for b in (3, 5):
            _against_the_twin(ctx, img, 0, roi, 500, ("roi", tuple(roi), b), quality=0.01, min_dist=7.0, block_size=b)
    for mc, q, d in SETTINGS:
        assert np.array_equal(ctx.detect_gftt_frame(0, mc, q, d), ctx.detect_gftt_frame(0, mc, q, d, roi=(0, 0, w, h)))


def test_a_region_that_is_a_cell_returns_the_bytes_of_the_cell_call(pmv, gpu_ctx_factory):
    ctx = _ctx(pmv, gpu_ctx_factory)
    _load(pmv, ctx, 0, ("rect", gf.W1, gf.H1))
    m = gc.masks(gf.W1, gf.H1)["discs"]
    total = 0
    for cell in ((0, 0, 255, 255), (255, 0, 255, 255), (262, 6, 255, 255), (300, 100, 97, 70), (510, 0, 7, 255)):
        for mc in (20, 0):
            for kw in (dict(), dict(block_size=5, use_harris=True, k=0.05, quality=0.02, min_dist=4.0), dict(mask=m, block_size=2)):
                want = ctx.detect_gftt_ex(0, [cell], mc, **kw)[0]
                got = ctx.detect_gftt_frame(0, mc, roi=cell, out_cap=None if mc else gc.UNLIMITED_CAP, **kw)
                assert np.array_equal(got, want), (cell, mc, sorted(kw))
                total += len(want)
    assert total > 200


@pytest.mark.parametrize("min_dist", [0.0, 20.0])
def test_ties_are_broken_by_address(pmv, gpu_ctx_factory, min_dist):
    """the plateau image: 512 records of one value, x above 255, pixel indices above 65 535"""
    ctx = _ctx(pmv, gpu_ctx_factory)
    img = _load(pmv, ctx, 2, ("plateau", gf.W1, gf.H1))
    for mc in (100, 0):
        n, records, _ = _against_the_twin(ctx, img, 2, None, mc, ("plateau", min_dist, mc), quality=0.01, min_dist=min_dist)
        assert records == 512 and n == (100 if mc else (512 if min_dist < 1 else n))


def test_more_records_than_fit_on_chip(pmv, gpu_ctx_factory):
    """768x512 noise at block size 1: more records above the threshold than the selection kernel holds on chip, so it takes its list in HBM -
    same bytes. Fewer records than that stay on chip."""
    ctx = _ctx(pmv, gpu_ctx_factory)
    img = _load(pmv, ctx, 3, ("noise", gf.W2, gf.H2))
    onchip = ctx.debug_gftt_frame_stats()[5]
    for d in (0.0, 3.0):
        n, records, stats = _against_the_twin(ctx, img, 3, None, 300, ("noise b1", d), quality=0.01, min_dist=d, block_size=1)
        assert n == 300 and records > onchip and stats[4] > 0
    n, records, stats = _against_the_twin(ctx, img, 3, None, 300, "noise b3", block_size=3)
    assert stats[4] == (0 if records <= onchip else stats[4]) and (records <= onchip or stats[4] > 0)
    small = _load(pmv, ctx, 2, ("noise", gf.W1, gf.H1))
    n, records, stats = _against_the_twin(ctx, small, 2, None, 300, "noise 517x261 b3", block_size=3)
    assert records == 8885 and records <= onchip and stats[4] == 0


def test_no_limit_and_overflow(pmv, gpu_ctx_factory):
    """517x261 noise at block size 1, min_dist 0, no limit: all 14 835 corners in order with out_cap 16384; with out_cap 1000 the call refuses
    with PMV_ERR_OVERFLOW, writes nothing, and leaves no trace in the next call"""
    ctx = _ctx(pmv, gpu_ctx_factory)
    img = _load(pmv, ctx, 2, ("noise", gf.W1, gf.H1))
    kw = dict(quality=0.01, min_dist=0.0, block_size=1)
    n, records, _ = _against_the_twin(ctx, img, 2, None, 0, "no limit", **kw)
    assert n == records == 14835
    P = pmv.GfttParams(0.01, 0.0, 1, 0, 0.04)
    xy, cnt = np.full((1000, 2), -7, np.int32), np.full(1, -7, np.int32)
    rc = gf.raw_frame_call(ctx, ctx.lib.pmv_detect_gftt_frame, 2, None, 0, P, None, 0, xy, 1000, cnt)
    assert rc == OVERFLOW and (xy == -7).all() and (cnt == -7).all()
    assert "no limit" in ctx.lib.pmv_last_error(ctx.h).decode()
    # the same with min_dist >= 1 (the walk looks for one corner more than fits)
    P3 = pmv.GfttParams(0.01, 3.0, 1, 0, 0.04)
    want3, _ = gf.twin_region(img, gf.whole(img), 0, quality=0.01, min_dist=3.0, block_size=1)
    assert len(want3) > 1000
    rc = gf.raw_frame_call(ctx, ctx.lib.pmv_detect_gftt_frame, 2, None, 0, P3, None, 0, xy, 1000, cnt)
    assert rc == OVERFLOW and (xy == -7).all() and (cnt == -7).all()
    got = ctx.detect_gftt_frame(2, 0, out_cap=len(want3), **dict(kw, min_dist=3.0))   # exactly as many as fit: no overflow
    assert np.array_equal(got, want3)
    _against_the_twin(ctx, img, 2, None, 1000, "the next ordinary call", **kw)


def test_refusals_write_nothing(pmv, gpu_ctx_factory):
    ctx = _ctx(pmv, gpu_ctx_factory)
    img = _load(pmv, ctx, 0, ("rect", gf.W1, gf.H1))
    P = pmv.GfttParams
    good = P(0.01, 7.0, 3, 0, 0.04)
    mask = np.full((gf.H1, gf.W1), 255, np.uint8)
    nan, inf = float("nan"), float("inf")
    cases = [("null p", INVALID, "null argument", dict(params=None)), ("null out_xy", INVALID, "null argument", dict(xy=None)),
             ("null out_count", INVALID, "null argument", dict(cnt=None))]
    cases += [(f"block_size {b}", INVALID, "block_size", dict(params=P(0.01, 5.0, b, 0, 0.04))) for b in (0, 16)]
    cases += [(f"quality {q}", INVALID, "quality", dict(params=P(q, 5.0, 3, 0, 0.04))) for q in (0.0, 1.5, nan)]
    cases += [(f"min_dist {d}", INVALID, "min_dist", dict(params=P(0.01, d, 3, 0, 0.04))) for d in (-1.0, inf)]
    cases += [("k", INVALID, "k =", dict(params=P(0.01, 5.0, 3, 1, nan)))]
    cases += [("mask_stride below the width", CAPACITY, "mask_stride", dict(mask=mask, stride=gf.W1 - 1))]
    cases += [("region outside the frame", INVALID, f"(300,0,218,100) is smaller than 3x3 or not inside the {gf.W1}x{gf.H1} frame", dict(roi=(300, 0, 218, 100))),
              ("region below 3x3", INVALID, "(5,5,2,3) is smaller than 3x3", dict(roi=(5, 5, 2, 3))),
              ("negative origin", INVALID, "not inside", dict(roi=(-1, 0, 50, 50))),
              ("slot out of range", CAPACITY, "slot out of range", dict(slot=9)),
              ("max_corners above out_cap", CAPACITY, "max_corners", dict(mc=51)),
              ("no limit without room", CAPACITY, "max_corners", dict(mc=0, cap=0)),
              ("out_cap above the maximum without a limit", CAPACITY, "max_corners", dict(mc=0, cap=gf.MAX_CORNERS + 1))]
    want, _ = gf.twin_region(img, gf.whole(img), 50, quality=0.01, min_dist=7.0)
    for what, code, text, change in cases:
        a = dict(slot=0, roi=None, mc=50, params=good, mask=None, stride=0, xy=1, cap=50, cnt=1)
        a.update(change)
        xy, cnt = np.full((gf.MAX_CORNERS + 1, 2), -7, np.int32), np.full(1, -7, np.int32)
        rc = gf.raw_frame_call(ctx, ctx.lib.pmv_detect_gftt_frame, a["slot"], a["roi"], a["mc"], a["params"], a["mask"], a["stride"], None if a["xy"] is None else xy,
                               a["cap"], None if a["cnt"] is None else cnt)
        assert rc == code, f"{what}: status {rc}, expected {code}"
        assert text in ctx.lib.pmv_last_error(ctx.h).decode(), f"{what}: message {ctx.lib.pmv_last_error(ctx.h).decode()!r}"
        assert (xy == -7).all() and (cnt == -7).all(), f"{what}: an output was written"
        assert np.array_equal(ctx.detect_gftt_frame(0, 50, min_dist=7.0), want), f"the valid call after '{what}'"
    # an empty slot
    with pytest.raises(pmv.PmvError) as e:
        gpu_ctx_factory(64, 64, n_slots=1, max_tracks=16).detect_gftt_frame(0, 10)
    assert e.value.code == INVALID
    # the cell calls keep their 255 limit
    for fn in (lambda c: ctx.detect_gftt(0, [c], 20), lambda c: ctx.detect_gftt_ex(0, [c], 20, block_size=5)):
        for cell in ((0, 0, 256, 80), (0, 0, 80, 256)):
            with pytest.raises(pmv.PmvError) as e:
                fn(cell)
            assert e.value.code == INVALID and "invalid for" in str(e.value)


def test_the_buffers_go_with_the_context(pmv):
    before = pmv.mem_live()
    ctx = pmv.Context(320, 256, n_slots=1, max_tracks=16)
    try:
        img = gc.noise_frame()
        ctx.frame_upload(0, img)
        mid = pmv.mem_live()
        got = ctx.detect_gftt_frame(0, 100, mask=gc.checker_mask(320, 256))
        assert np.array_equal(got, gc.twin().corners(img, gf.whole(img), 100, mask=gc.checker_mask(320, 256)))
        assert pmv.mem_live()[0] > mid[0] and pmv.mem_live()[1] > mid[1], "the first frame call makes its buffers"
    finally:
        ctx.close()
    assert pmv.mem_live() == before
