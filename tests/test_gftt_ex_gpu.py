"""pmv_detect_gftt_ex on the GPU: every case against the CPU twin (tests/twin/gftt_twin.cpp) bit for bit - corners, counts and the
response map of one cell per case -, the default arguments against pmv_detect_gftt through both kernel paths, the contract, the session
form. One 320x256 context, four slots (tests/gftt_common.py): 0 = the 203x87 frame, 1 = 160x120, 2 = the gradient image, 3 = noise."""
import ctypes as C
import threading

import numpy as np
import pytest

import gftt_common as gc

pytestmark = pytest.mark.gpu

INVALID, CAPACITY, OVERFLOW = -2, -3, -6
_state = {}
_i32p, _u8p = C.POINTER(C.c_int32), C.POINTER(C.c_uint8)


def _frames(pmv):
    return [gc.frame(pmv, 203, 87), gc.frame(pmv, 160, 120), gc.gradient_frame(), gc.noise_frame()]


def _ctx(pmv, gpu_ctx_factory):
    if "ctx" not in _state:
        ctx = gpu_ctx_factory(320, 256, n_slots=4, max_tracks=256)
        for slot, img in enumerate(_frames(pmv)):
            ctx.frame_upload(slot, img)
        _state["ctx"] = ctx
    _state["ctx"].debug_gftt_general(False)
    return _state["ctx"]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _against_the_twin(ctx, img, slot, cells, max_per_cell, resp_cell, what, detect=None, **kw):
    """one extended call over `cells` against one twin run per cell; the response map of cells[resp_cell]"""
    got = (detect or ctx.detect_gftt_ex)(slot, cells, max_per_cell, **kw)
    total = 0
    for i, cell in enumerate(cells):
        want = gc.cached((what, max_per_cell, tuple(int(v) for v in cell)), lambda: gc.twin().cell(img, cell, max_per_cell, **kw))
        assert len(got[i]) == len(want[0]), f"{what}: cell {cell}: {len(got[i])} corners, the twin has {len(want[0])}"
        assert np.array_equal(got[i], want[0]), f"{what}: cell {cell}: corners differ from index {np.flatnonzero((got[i] != want[0]).any(axis=1))[:4]}"
        total += len(want[0])
        if i == resp_cell:
            rkw = {k: v for k, v in kw.items() if k in ("block_size", "use_harris", "k")}
            resp = ctx.gftt_response_ex(slot, cell, **rkw)
            assert np.array_equal(_bits(resp), _bits(want[1])), f"{what}: cell {cell}: response differs at {np.argwhere(_bits(resp) != _bits(want[1]))[:4]}"
    return total


@pytest.mark.parametrize("max_per_cell", [20, 0], ids=["max20", "nolimit"])
@pytest.mark.parametrize("harris", [False, True], ids=["mineig", "harris"])
@pytest.mark.parametrize("b", [1, 2, 3, 5, 8, 15])
def test_sweep_of_block_sizes_and_response_kinds(pmv, gpu_ctx_factory, b, harris, max_per_cell):
    """203x87: the grid, 40x33 (narrower than a tile), 97x70 (4x3 ragged tiles), the four frame corners, 5x4 and 3x3"""
    ctx = _ctx(pmv, gpu_ctx_factory)
    cells = gc.sweep_cells(pmv, 203, 87)
    resp_cell = 2 if max_per_cell else len(cells) - 1   # 97x70; the cell at the frame's lower right corner
    total = _against_the_twin(ctx, _frames(pmv)[0], 0, cells, max_per_cell, resp_cell, ("sweep", b, harris), block_size=b, use_harris=harris, k=0.04)
    # (at b = 1 the Harris response is -k (dx^2 + dy^2)^2 up to rounding: nowhere positive, nothing selected - by the twin)
    assert total > 30 or (b == 1 and harris and total == 0), "the scene gives too few corners to compare anything"


def test_harris_with_nothing_positive(pmv, gpu_ctx_factory):
    """k = 0.25 on a gradient-only image: no response is positive, so nothing is selected"""
    ctx = _ctx(pmv, gpu_ctx_factory)
    img = _frames(pmv)[2]
    h, w = img.shape
    cells = np.concatenate([pmv.grid_cells(w, h), [(10, 10, 40, 33)]]).astype(np.int32)
    for b in (3, 5):
        for cell in cells:
            xy, resp, mx, _ = gc.twin().cell(img, cell, 0, block_size=b, use_harris=True, k=0.25)
            assert mx <= 0 and resp.max() <= 0 and resp.min() < 0 and len(xy) == 0
        for mpc in (20, 0):
            got = ctx.detect_gftt_ex(2, cells, mpc, block_size=b, use_harris=True, k=0.25)
            assert [len(g) for g in got] == [0] * len(cells)
        resp = ctx.gftt_response_ex(2, cells[0], block_size=b, use_harris=True, k=0.25)
        assert np.array_equal(_bits(resp), _bits(gc.twin().response(img, cells[0], b, True, 0.25)))


@pytest.mark.parametrize("b", [3, 5])
@pytest.mark.parametrize("name", ["discs", "checker", "zero", "roi"])
def test_masks(pmv, gpu_ctx_factory, name, b):
    """160x120: discs of radius 7 around 60 points, a checkerboard of single pixels, all-zero, and the disc mask as an ROI view of a larger
    array (mask_stride > w)"""
    ctx = _ctx(pmv, gpu_ctx_factory)
    w, h = 160, 120
    m = gc.masks(w, h)[name]
    assert m.shape == (h, w) and (name != "roi" or m.strides[0] > w)
    cells = np.concatenate([pmv.grid_cells(w, h), gc.corner_cells(w, h), [(50, 20, 40, 33), (60, 10, 97, 70)]]).astype(np.int32)
    for mpc in (20, 0):
        total = _against_the_twin(ctx, _frames(pmv)[1], 1, cells, mpc, 0, ("mask", name, b), mask=m, block_size=b)
        assert (total == 0) == (name == "zero")
    if name == "roi":   # the view and the tight copy are the same mask
        assert all(np.array_equal(a, c) for a, c in zip(ctx.detect_gftt_ex(1, cells, 0, mask=m, block_size=b),
                                                         ctx.detect_gftt_ex(1, cells, 0, mask=np.ascontiguousarray(m), block_size=b)))


def test_the_threshold_follows_the_masked_maximum_on_the_device(pmv, gpu_ctx_factory):
    """the mask of tests/test_gftt_twin.py that blanks the strongest corner: the device returns the twin's list, not the post-filtered one"""
    ctx = _ctx(pmv, gpu_ctx_factory)
    cell = pmv.grid_cells(160, 120)[0]
    m, plain, masked = gc.blanked_strongest(pmv, 160, 120, cell, quality=0.3)
    assert np.array_equal(ctx.detect_gftt_ex(1, [cell], 0, quality=0.3)[0], plain)
    assert np.array_equal(ctx.detect_gftt_ex(1, [cell], 0, quality=0.3, mask=m)[0], masked)
    assert len(masked) > int((m[plain[:, 1], plain[:, 0]] != 0).sum())


def test_more_records_than_the_register_capacity(pmv, gpu_ctx_factory):
    """a 255x255 noise cell at b = 1, min_dist 0: more than GP_REG records pass the threshold, so k_gftt_pick walks its list in HBM; the
    no-limit call overflows PMV_GFTT_UNLIMITED_CAP like pmv_detect_gftt in the same situation"""
    ctx = _ctx(pmv, gpu_ctx_factory)
    img = _frames(pmv)[3]
    cell = np.asarray([40, 1, 255, 255], np.int32)
    xy, _, _, records = gc.twin().cell(img, cell, 4000, min_dist=0.0, block_size=1)
    assert records > gc.GP_REG and len(xy) == 4000
    got = ctx.detect_gftt_ex(3, [cell], 4000, min_dist=0.0, block_size=1)[0]
    assert np.array_equal(got, xy), f"differs from index {np.flatnonzero((got != xy).any(axis=1))[:4]}"
    assert len(gc.twin().corners(img, cell, 0, min_dist=0.0, block_size=1)) > gc.UNLIMITED_CAP
    with pytest.raises(pmv.PmvError) as e:
        ctx.detect_gftt_ex(3, [cell], 0, min_dist=0.0, block_size=1)
    assert e.value.code == OVERFLOW
    # the overflow bit does not leak into the next call
    assert np.array_equal(ctx.detect_gftt_ex(3, [cell], 4000, min_dist=0.0, block_size=1)[0], xy)


def test_the_defaults_are_detect_gftt_through_either_path(pmv, gpu_ctx_factory):
    ctx = _ctx(pmv, gpu_ctx_factory)
    names = set()
    for slot, (w, h) in ((0, (203, 87)), (1, (160, 120))):
        cells = np.concatenate([pmv.grid_cells(w, h), gc.corner_cells(w, h), [(50, 20, 40, 33)]]).astype(np.int32)
        for mpc, q, d in ((20, 0.01, 5.0), (0, 0.05, 3.0), (50, 0.01, 0.0)):
            want = ctx.detect_gftt(slot, cells, mpc, q, d)
            assert sum(len(x) for x in want) > 30
            ctx.prof_enable(True)
            tuned = ctx.detect_gftt_ex(slot, cells, mpc, q, d, k=123.0)
            prof_tuned = ctx.prof_read()
            ctx.debug_gftt_general(True)
            ctx.prof_enable(True)
            general = ctx.detect_gftt_ex(slot, cells, mpc, q, d)
            prof_general = ctx.prof_read()
            ctx.prof_enable(False)
            ctx.debug_gftt_general(False)
            for what, got in (("tuned", tuned), ("general", general)):
                assert all(np.array_equal(a, b) for a, b in zip(got, want)) and len(got) == len(want), f"{what} path, slot {slot}, max {mpc}"
            # both paths are booked under the two existing classes, one launch each
            for prof in (prof_tuned, prof_general):
                assert {k: v[0] for k, v in prof.items()} == {"k_gftt_cand": 1, "k_gftt_pick": 1}
            names |= set(prof_general)
        # the general response map at the defaults is pmv_debug_gftt_response's
        assert np.array_equal(_bits(ctx.gftt_response_ex(slot, cells[0])), _bits(ctx.gftt_response(slot, cells[0])))
    ctx.lib.pmv_prof_kernel_name.restype = C.c_char_p
    classes = [ctx.lib.pmv_prof_kernel_name(i).decode() for i in range(ctx.lib.pmv_prof_kernel_count())]
    assert [c for c in classes if "gftt" in c] == ["k_gftt_cand", "k_gftt_pick"], "no new profiling class"


def _raw_call(ctx, fn, slot, cells, mpc, params, mask, stride, xy, cnt):
    fn.argtypes = [C.c_void_p, C.c_int, _i32p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    cells = None if cells is None else np.ascontiguousarray(cells, np.int32)
    return fn(ctx.h, slot, None if cells is None else cells.ctypes.data_as(_i32p), 0 if cells is None else len(cells), mpc,
              None if params is None else C.cast(C.pointer(params), C.c_void_p), None if mask is None else mask.ctypes.data, stride,
              None if xy is None else xy.ctypes.data, None if cnt is None else cnt.ctypes.data)


def _error_cases(pmv):
    P = pmv.GfttParams
    good = P(0.01, 5.0, 3, 0, 0.04)
    cells = [(0, 0, 100, 80), (100, 0, 60, 80)]
    mask = np.full((120, 160), 255, np.uint8)
    nan, inf = float("nan"), float("inf")
    cases = [("null p", INVALID, dict(params=None)), ("null out_xy", INVALID, dict(xy=None)), ("null out_count", INVALID, dict(cnt=None))]
    cases += [(f"block_size {b}", INVALID, dict(params=P(0.01, 5.0, b, 0, 0.04))) for b in (0, 16, -3)]
    cases += [(f"quality {q}", INVALID, dict(params=P(q, 5.0, 3, 0, 0.04))) for q in (0.0, -0.1, 1.5, nan, inf)]
    cases += [(f"min_dist {d}", INVALID, dict(params=P(0.01, d, 3, 0, 0.04))) for d in (-1.0, nan, inf)]
    cases += [(f"k {k}", INVALID, dict(params=P(0.01, 5.0, 3, 1, k))) for k in (nan, inf)]
    cases += [("mask_stride below the width", CAPACITY, dict(mask=mask, stride=159))]
    cases += [("cell outside the frame", INVALID, dict(cells=[(100, 0, 61, 80)])), ("cell below 3x3", INVALID, dict(cells=[(0, 0, 2, 3)])),
              ("cell above 255", INVALID, dict(cells=[(0, 0, 256, 80)])), ("slot out of range", CAPACITY, dict(slot=9)),
              ("max_per_cell above the capacity", CAPACITY, dict(mpc=5000))]
    return good, cells, mask, cases


@pytest.mark.parametrize("session", [False, True], ids=["single", "session"])
def test_errors_write_nothing_and_a_valid_call_follows(pmv, gpu_ctx_factory, session):
    ctx = _ctx(pmv, gpu_ctx_factory)
    good, cells, mask, cases = _error_cases(pmv)
    fn = ctx.lib.pmv_batch_detect_gftt_ex if session else ctx.lib.pmv_detect_gftt_ex
    detect = ctx.batch_detect_gftt_ex if session else ctx.detect_gftt_ex
    want = ctx.detect_gftt_ex(1, cells, 20, mask=mask, block_size=5)
    want_nan_k = ctx.detect_gftt(1, cells, 20)
    if session:
        ctx.batch_open(1, [(160, 120)])
    try:
        for what, code, change in cases:
            a = dict(slot=1, cells=cells, mpc=20, params=good, mask=None, stride=0, xy=np.full((2, 20, 2), -7, np.int32), cnt=np.full(2, -7, np.int32))
            a.update(change)
            xy, cnt = np.full((2, 20, 2), -7, np.int32), np.full(2, -7, np.int32)
            rc = _raw_call(ctx, fn, a["slot"], a["cells"], a["mpc"], a["params"], a["mask"], a["stride"], a["xy"] if a["xy"] is None else xy,
                           a["cnt"] if a["cnt"] is None else cnt)
            assert rc == code, f"{what}: status {rc}, expected {code}"
            assert (xy == -7).all() and (cnt == -7).all(), f"{what}: an output was written"
            got = detect(1, cells, 20, mask=mask, block_size=5)
            assert all(np.array_equal(g, w) for g, w in zip(got, want)), f"the valid call after '{what}'"
        # k is ignored without use_harris, whatever it holds
        got = detect(1, cells, 20, k=float("nan"))
        assert all(np.array_equal(g, w) for g, w in zip(got, want_nan_k))
    finally:
        if session:
            ctx.batch_close()


def test_sessions_mix_plain_and_extended_requests(pmv, gpu_ctx_factory):
    """four threads on one session, each a mix of batch_detect_gftt and batch_detect_gftt_ex with two extended parameter sets (one with a
    mask) on two frame sizes: every result is the single call's. Before that, a run of plain requests only: one round per request, as ever."""
    ctx = _ctx(pmv, gpu_ctx_factory)
    sizes = {0: (203, 87), 1: (160, 120)}
    cells = {s: np.concatenate([pmv.grid_cells(w, h), gc.corner_cells(w, h)]).astype(np.int32) for s, (w, h) in sizes.items()}
    masks = {s: gc.disc_mask(w, h, gc.track_points(w, h, 40, seed=23 + s), 6) for s, (w, h) in sizes.items()}
    ext_a = dict(block_size=5, use_harris=True, k=0.05, quality=0.02, min_dist=4.0)
    ext_b = dict(block_size=2, quality=0.01, min_dist=5.0)
    jobs = []   # (kind, slot, max_per_cell, kwargs)
    for s in sizes:
        for mpc in (20, 0):
            jobs += [("plain", s, mpc, {}), ("ex", s, mpc, ext_a), ("ex", s, mpc, dict(ext_b, mask=masks[s])), ("ex", s, mpc, {})]
    want = [(ctx.detect_gftt if kind == "plain" else ctx.detect_gftt_ex)(s, cells[s], mpc, **kw) for kind, s, mpc, kw in jobs]
    assert all(sum(len(x) for x in w) > 10 for w in want)
    plain20 = {s: ctx.detect_gftt(s, cells[s], 20) for s in sizes}
    with ctx.batch_session(1, list(sizes.values())):
        before = ctx.batch_stats()["det"]
        for s in sizes:
            for _ in range(3):
                got = ctx.batch_detect_gftt(s, cells[s], 20)
                assert all(np.array_equal(g, w) for g, w in zip(got, plain20[s]))
        mid = ctx.batch_stats()["det"]
        assert (mid["requests"] - before["requests"], mid["launches"] - before["launches"]) == (6, 6), "plain requests one at a time: a round each"
        errors, results = [], [None] * 4
        start = threading.Barrier(4)

        def run(j):
            try:
                start.wait()
                out = []
                for rep in range(3):
                    for i in range(len(jobs)):
                        kind, s, mpc, kw = jobs[(i + 5 * j) % len(jobs)]
                        fn = ctx.batch_detect_gftt if kind == "plain" else ctx.batch_detect_gftt_ex
                        out.append(((i + 5 * j) % len(jobs), fn(s, cells[s], mpc, **kw)))
                results[j] = out
            except Exception as e:   # noqa: BLE001
                errors.append((j, repr(e)))
        th = [threading.Thread(target=run, args=(j,)) for j in range(4)]
        for t in th:
            t.start()
        for t in th:
            t.join()
        after = ctx.batch_stats()["det"]
    assert not errors, errors
    for j in range(4):
        for i, got in results[j]:
            assert len(got) == len(want[i]) and all(np.array_equal(g, w) for g, w in zip(got, want[i])), f"thread {j}, job {jobs[i][:3]}"
    assert after["requests"] - mid["requests"] == 4 * 3 * len(jobs)
    print(f"session mix: {after['requests'] - mid['requests']} requests in {after['launches'] - mid['launches']} rounds")
