"""ShiTomasi (k_st_resp, k_st_select), FAST (k_fast_score, k_fast_select) and the kNN matcher (k_knn_round) off the reference's constants
and off the one frame size the other suites use: the candidate list in HBM instead of LDS, neighbour counts and windows other than 7 and 15
(window 63: totals above 2^24, the one-lane fallback as the normal path), duplicate candidates, points outside the frame; ShiTomasi cells
whose candidates spill past the LDS list, score ties across the LDS list and the spill list, cells that are no multiple of the 32x32 tile,
every quality; FAST at the ends of the threshold range, on a binary image, at the 256-column step of the selection and with MAX_CELLS cells;
session rounds whose requests differ in their parameters.

Every comparison is bitwise against the oracle (integers, or float64 / float32 in a fixed order). Inputs: tests/alt_common.py. Each test
asserts on the oracle's side that it reaches the path it is about."""
import threading

import numpy as np
import pytest

import alt_common as ac

pytestmark = pytest.mark.gpu

_cache = {}
IMAGES = {"noise": ac.noise, "shifted": ac.shifted, "binary": ac.binary, "flat": ac.flat, "periodic": ac.periodic}


def _ctx(gpu_ctx_factory, size):
    """one context per frame size (four slots); what a slot holds is remembered, so an image goes up once"""
    key = ("ctx", size)
    if key not in _cache:
        _cache[key] = (gpu_ctx_factory(size[0], size[1], n_slots=4, max_tracks=2048), {})
    return _cache[key]


def _slot(gpu_ctx_factory, size, kind):
    """(context, slot) with the image `kind` of that size in the slot: noise in 0, shifted in 1, the others take turns in 2"""
    ctx, held = _ctx(gpu_ctx_factory, size)
    slot = {"noise": 0, "shifted": 1}.get(kind, 2)
    if held.get(slot) != kind:
        ctx.frame_upload(slot, IMAGES[kind](*size))
        held[slot] = kind
    return ctx, slot


def _same(got, want, what):
    assert len(got) == len(want), what
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), f"{what}: array {i} differs"


# ---- kNN matcher, single calls ------------------------------------------------------------------------------------------------------
def _knn_pair(gpu_ctx_factory, size, second):
    ctx, s0 = _slot(gpu_ctx_factory, size, "noise")
    _, s1 = _slot(gpu_ctx_factory, size, second)
    return ctx, s0, s1, ac.noise(*size), IMAGES[second](*size)


def _knn_check(ctx, orc, s0, s1, a, b, src, cand, n_nn, window, what):
    gb, ge = ctx.knn_match(s0, s1, src, cand, neighbours=n_nn, window=window)
    ob_, oe = orc.knn_match(a, b, src, cand, neighbours=n_nn, window=window)
    assert np.array_equal(gb, ob_), (what, n_nn, window, len(cand), gb, ob_)
    assert np.array_equal(ge, oe), (what, n_nn, window, len(cand), ge, oe)
    return ob_, oe


@pytest.mark.parametrize("size", [ac.SMALL, ac.MID], ids=lambda s: f"{s[0]}x{s[1]}")
def test_knn_neighbour_counts_and_windows(orc, gpu_ctx_factory, size):
    """n_neighbours 1, 2, 7, 8 (the unrolled KNN_MAX_NN loops) times window 1, 2, 15, 16, 63 (side, pairs and p / side of knn_window_error;
    even windows: win = ceil(window / 2)), 9 sources with three at the border, 300 candidates with duplicated rows and one at a source's own
    coordinates; the shifted second frame, and the first frame against itself. At window 63 a compared window sums to more than 2^24 (the
    walk in the reference's order decides the bits), at window 15 one sums to less (the integer total does)."""
    src, cand = ac.knn_sweep_lists(*size)
    assert len(np.unique(cand, axis=0)) <= len(cand) - 6 and (cand == src[4]).all(1).any()
    for second in ("shifted", "noise"):
        ctx, s0, s1, a, b = _knn_pair(gpu_ctx_factory, size, second)
        for n_nn in (1, 2, 7, 8):
            for window in (1, 2, 15, 16, 63):
                best, err = _knn_check(ctx, orc, s0, s1, a, b, src, cand, n_nn, window, second)
                assert (best >= 0).all() and (err > 0).all()
                totals = ac.window_totals(a, b, src, cand, best, window)
                if window == 63:
                    assert totals.max() > 2 ** 24, totals
                if window == 15:
                    assert 0 < totals.min() < 2 ** 24, totals


@pytest.mark.parametrize("n_nn,window", [(7, 15), (8, 16)])
def test_knn_candidate_list_in_lds_and_in_hbm(orc, gpu_ctx_factory, n_nn, window):
    """list lengths 0, 1, 5 and on both sides of KNN_LDS_M = 1024: from 1025 on k_knn_round reads the list from HBM (the lds == false
    instantiation of knn_one). The last candidate of the two long lists is the best fit of one source (alt_common.knn_length_lists), so the
    results hold an index >= 1024: the tail of the list was read."""
    ctx, s0, s1, a, b = _knn_pair(gpu_ctx_factory, ac.MID, "shifted")
    for m in (0, 1, 5, 1023, 1024, 1025, 1500):
        src, cand = ac.knn_length_lists(*ac.MID, m, n_nn)
        assert len(cand) == m
        best, err = _knn_check(ctx, orc, s0, s1, a, b, src, cand, n_nn, window, "list length")
        if m == 0:
            assert (best == -1).all()
        if m >= 1023:
            assert len(np.unique(cand, axis=0)) < m, "the list was meant to hold duplicates"
        if m > ac.KNN_LDS_M:
            assert (best >= ac.KNN_LDS_M).any() and best[20] == m - 1 and err[20] == 0, best


def test_knn_source_counts_around_a_workgroup(orc, gpu_ctx_factory):
    """1, 3, 4 and 5 sources (KNN_WAVES = 4 per workgroup: a partial workgroup, a full one, a second one with one wavefront at work) against
    a list in HBM and a list in LDS"""
    ctx, s0, s1, a, b = _knn_pair(gpu_ctx_factory, ac.MID, "shifted")
    src, long_list = ac.knn_length_lists(*ac.MID, 1025, 7)
    src = src[[20, 0, 1, 2, 3]]                              # source 20 first: its best fit is the last candidate of the long list
    for n in (1, 3, ac.KNN_WAVES, ac.KNN_WAVES + 1):
        best, _ = _knn_check(ctx, orc, s0, s1, a, b, src[:n], long_list, 7, 15, f"{n} sources, list in HBM")
        assert best[0] == 1024
        best, _ = _knn_check(ctx, orc, s0, s1, a, b, src[:n], long_list[:40], 7, 15, f"{n} sources, list in LDS")
        assert (best >= 0).all()


def test_knn_every_candidate_at_the_source(orc, gpu_ctx_factory):
    """three candidates, all at the source's own coordinates: every pass finds nothing, the default Feature at (0, 0) is compared and the
    best index is -1"""
    ctx, s0, s1, a, b = _knn_pair(gpu_ctx_factory, ac.SMALL, "shifted")
    src = np.array([[40, 30]], np.int32)
    cand = np.repeat(src, 3, axis=0)
    for n_nn, window in ((7, 15), (1, 1), (8, 63)):
        best, err = _knn_check(ctx, orc, s0, s1, a, b, src, cand, n_nn, window, "all candidates at the source")
        assert best[0] == -1 and err[0] > 0


@pytest.mark.parametrize("size", [ac.SMALL, ac.MID], ids=lambda s: f"{s[0]}x{s[1]}")
def test_knn_points_outside_the_frame(orc, gpu_ctx_factory, size):
    """sources and candidates up to 10 pixels outside the frame on every side: a pixel is read only behind the bounds test on both
    coordinates (the reference skips such pairs), so the call is defined and equals the oracle"""
    w, h = size
    ctx, s0, s1, a, b = _knn_pair(gpu_ctx_factory, size, "shifted")
    src = np.concatenate([ac.points(31, w, h, 36, margin=10), [[-10, -10], [w + 9, h + 9], [-10, h + 9], [w + 9, -10]]]).astype(np.int32)
    cand = np.concatenate([ac.points(32, w, h, 196, margin=10), [[-10, -10], [w + 9, h + 9], [-9, h // 2], [w // 2, h + 9]]]).astype(np.int32)
    outside = lambda p: ((p[:, 0] < 0) | (p[:, 1] < 0) | (p[:, 0] >= w) | (p[:, 1] >= h)).sum()
    assert outside(src) >= 8 and outside(cand) >= 20
    for n_nn, window in ((7, 15), (8, 16), (2, 63), (3, 1)):
        best, err = _knn_check(ctx, orc, s0, s1, a, b, src, cand, n_nn, window, "outside the frame")
        assert (best >= 0).all()
    _knn_check(ctx, orc, s0, s1, a, b, src, cand[:0], 7, 15, "outside the frame, no candidate")


# ---- FAST, single calls -----------------------------------------------------------------------------------------------------------
def _fast_check(ctx, orc, slot, img, views, mx, t, nonmax):
    got = ctx.detect_fast(slot, views, mx, threshold=t, nonmax=nonmax)
    n = 0
    for c, (gxy, grs) in zip(views, got):
        rxy, rrs = orc.fast9_cell(img, c, mx, threshold=t, nonmax=nonmax)
        assert np.array_equal(gxy, rxy) and np.array_equal(grs, rrs), (t, nonmax, mx, tuple(c), len(gxy), len(rxy))
        n += len(rxy)
    return n


@pytest.mark.parametrize("kind", ["noise", "binary", "flat"])
@pytest.mark.parametrize("size", [ac.SMALL, ac.WIDE], ids=lambda s: f"{s[0]}x{s[1]}")
def test_fast_thresholds_at_the_ends_of_the_range(pmv, orc, gpu_ctx_factory, size, kind):
    """thresholds 0 (without and with non-max suppression), 1, 254, 255 and the clamped 300 and -5, on the whole frame and on the grid
    cells. Noise and the binary image give keypoints at 0 and none at 255; on the binary image every corner scores 254, so the strict `>` of
    the non-max rule is what thins them; the flat image gives nothing."""
    w, h = size
    ctx, slot = _slot(gpu_ctx_factory, size, kind)
    img = IMAGES[kind](w, h)
    whole = np.asarray([[0, 0, w, h]], np.int32)
    counts = {}
    for t, nonmax in ((0, False), (0, True), (1, True), (254, True), (254, False), (255, True), (300, False), (-5, True)):
        for views in (whole, pmv.grid_cells(w, h)):
            counts[t, nonmax] = _fast_check(ctx, orc, slot, img, views, 4096, t, nonmax)
    if kind == "flat":
        assert not any(counts.values())
        return
    assert counts[0, False] > counts[0, True] > 0 and counts[1, True] > 0 and counts[-5, True] == counts[0, True]
    assert counts[255, True] == 0 and counts[300, False] == 0
    if kind == "binary":
        assert counts[254, False] == counts[0, False] and counts[254, True] == counts[0, True]
        rs = np.concatenate([r for _, r in ctx.detect_fast(slot, whole, 4096, threshold=0, nonmax=True)])
        assert (rs == 254).all()


def test_fast_cell_geometry(orc, gpu_ctx_factory):
    """on 333x121: cell widths 255, 256, 257 and 333 (the x0 += 256 step of k_fast_select), 7x7 (one interior pixel, and it is a corner),
    6x9 and 9x6 (none), a cell flush with the right and bottom edge of a frame whose width is no multiple of 4, two overlapping cells, and
    MAX_CELLS = 64 cells of 20x15 in one call"""
    w, h = ac.WIDE
    wide = np.asarray([[0, 0, 255, h], [0, 0, 256, h], [0, 0, 257, h], [0, 0, w, h], [w - 257, 0, 257, h]], np.int32)
    tiny = np.asarray([[50, 40, 6, 9], [50, 40, 9, 6], [w - 6, h - 9, 6, 9]], np.int32)
    flush = np.asarray([[w - 41, h - 30, 41, 30], [w - 7, h - 7, 7, 7]], np.int32)
    overlap = np.asarray([[10, 10, 60, 50], [30, 25, 60, 50]], np.int32)
    tiles = np.asarray([[5 + 20 * i, 3 + 15 * j, 20, 15] for j in range(4) for i in range(16)], np.int32)
    assert len(tiles) == ac.MAX_CELLS and tiles[-1][0] + 20 <= w and tiles[-1][1] + 15 <= h
    for kind in ("noise", "binary"):
        ctx, slot = _slot(gpu_ctx_factory, ac.WIDE, kind)
        img = IMAGES[kind](w, h)
        # a 7x7 cell whose single interior pixel is a keypoint at every threshold used here: the first one the oracle finds at 30
        kp = orc.fast9_cell(img, (0, 0, w, h), 1, threshold=30, nonmax=False)[0][0]
        seven = np.asarray([[kp[0] - 3, kp[1] - 3, 7, 7]], np.int32)
        for t, nonmax in ((10, True), (0, False), (20, False)):
            for views, mx in ((wide, 4096), (wide, 300), (tiny, 50), (flush, 4096), (overlap, 4096), (tiles, 4096), (seven, 5)):
                n = _fast_check(ctx, orc, slot, img, views, mx, t, nonmax)
                assert n == 0 if views is tiny else n == 1 if views is seven else n > 0 if not nonmax or views is wide else True, (kind, t, nonmax, views[0], n)
        # columns on both sides of the 256-column step hold keypoints
        xs = orc.fast9_cell(img, (0, 0, w, h), 4096, threshold=10, nonmax=False)[0][:, 0]
        assert (xs < 253).any() and (xs >= 256).any() and ((xs >= 253) & (xs < 256)).any()


def test_fast_first_max_cut(orc, gpu_ctx_factory):
    """max_per_cell 1, k - 1, k and k + 1 around the cell's full count k: the first `max` in raster order"""
    ctx, slot = _slot(gpu_ctx_factory, ac.WIDE, "noise")
    img = ac.noise(*ac.WIDE)
    cell = np.asarray([[13, 7, 300, 60]], np.int32)             # wider than 256: the cut may fall in the second column block of a row
    for t, nonmax in ((10, True), (30, False)):
        k = len(orc.fast9_cell(img, cell[0], 100000, threshold=t, nonmax=nonmax)[0])
        assert 3 < k < 4096
        for mx in (1, k - 1, k, k + 1):
            assert _fast_check(ctx, orc, slot, img, cell, mx, t, nonmax) == min(mx, k)


# ---- ShiTomasi, single calls ------------------------------------------------------------------------------------------------------
def _st_check(ctx, orc, slot, img, cells, mx, quality, responses=True):
    """lists, float64 scores and (once per cell) the response map against the oracle; returns the oracle's (xy, scores, candidate count)"""
    out = []
    for c, (gxy, gsc) in zip(cells, ctx.detect_shitomasi(slot, cells, mx, quality=quality)):
        rxy, rsc, R = orc.shitomasi_cell(img, c, mx, quality=quality, want_resp=True)
        if responses:
            Rg = ctx.shitomasi_response(slot, c)
            assert np.array_equal(np.isnan(Rg), np.isnan(R)), tuple(c)
            assert np.array_equal(np.nan_to_num(Rg), np.nan_to_num(R)), f"response differs in cell {tuple(c)}"
        assert np.array_equal(gxy, rxy), (tuple(c), mx, quality, len(gxy), len(rxy))
        assert gsc.dtype == np.float64 and np.array_equal(gsc, rsc), (tuple(c), mx, quality)
        Rn = np.nan_to_num(R)
        out.append((rxy, rsc, int((Rn > Rn.max() * quality).sum())))
    return out


def test_shitomasi_candidates_beyond_the_lds_list(orc, gpu_ctx_factory):
    """noise at quality 0.05 and 0.0: more than ST_CAP = 8192 candidates in a cell, so k_st_select keeps the rest in its HBM spill list and
    marks the taken ones there; a cell that is the whole 224x131 frame, a 128x100 cell, both in one call, and a 255x255 cell"""
    for size, cells in ((ac.MID, [[0, 0, 224, 131], [3, 2, 128, 100]]), (ac.TALL, [[41, 3, 255, 255]])):
        ctx, slot = _slot(gpu_ctx_factory, size, "noise")
        img = ac.noise(*size)
        cells = np.asarray(cells, np.int32)
        for quality in (0.05, 0.0):
            for views in ([cells[:1], cells[1:], cells] if len(cells) > 1 else [cells]):
                for xy, _, n_cand in _st_check(ctx, orc, slot, img, views, 40, quality, responses=quality == 0.0):
                    assert n_cand > ac.ST_CAP and len(xy) == 40, n_cand


def test_shitomasi_ties_across_the_lds_and_the_spill_list(orc, gpu_ctx_factory):
    """a 16x16 tile repeated: more than 8192 candidates at quality 0.4 and every score many times over, so the 40 corners hold fewer distinct
    scores than corners and their order is the raster-index rule alone - across the LDS list and the spill list, whose order atomicAdd
    changes from run to run. Twice, with identical output."""
    ctx, slot = _slot(gpu_ctx_factory, ac.MID, "periodic")
    img = ac.periodic(*ac.MID)
    cells = np.asarray([[0, 0, 224, 131]], np.int32)
    (xy, sc, n_cand), = _st_check(ctx, orc, slot, img, cells, 40, 0.4)
    assert n_cand > ac.ST_CAP and len(xy) == 40 and len(np.unique(sc)) < len(sc), (n_cand, len(np.unique(sc)))
    same = sc == sc[0]
    assert same.sum() > 1 and (np.diff((xy[same, 1] * 224 + xy[same, 0]).astype(np.int64)) > 0).all(), "equal scores come in raster order"
    first = ctx.detect_shitomasi(slot, cells, 40)
    second = ctx.detect_shitomasi(slot, cells, 40)
    _same(list(first[0]), list(second[0]), "second run")
    for mx in (300, 4096):                                      # deeper into the tied runs
        (xy, sc, _), = _st_check(ctx, orc, slot, img, cells, mx, 0.4, responses=False)
        assert len(xy) == mx


def test_shitomasi_cell_geometry(orc, gpu_ctx_factory):
    """cells that are no multiple of the 32x32 tile of k_st_resp: 3x3, 3x255, 255x3, 33x33 and 35x34 at odd offsets, flush with the right
    and bottom edge, and MAX_CELLS = 64 cells in one call; max_per_cell 1 and 4096"""
    w, h = ac.TALL
    ctx, slot = _slot(gpu_ctx_factory, ac.TALL, "noise")
    img = ac.noise(w, h)
    odd = np.asarray([[7, 9, 3, 3], [11, 1, 3, 255], [1, 13, 255, 3], [5, 3, 33, 33], [5, 3, 35, 34], [w - 35, h - 34, 35, 34], [w - 3, h - 3, 3, 3],
                      [w - 65, h - 97, 65, 97]], np.int32)
    tiles = np.asarray([[3 + 37 * i, 1 + 31 * j, 33 + (i & 1), 29 + (j & 1)] for j in range(8) for i in range(8)], np.int32)
    assert len(tiles) == ac.MAX_CELLS and (tiles[:, 0] + tiles[:, 2]).max() <= w and (tiles[:, 1] + tiles[:, 3]).max() <= h
    for mx in (1, 4096):
        for quality in (0.4, 0.0):
            res = _st_check(ctx, orc, slot, img, odd, mx, quality, responses=mx == 1)
            assert all(len(xy) == min(mx, n) for xy, _, n in res)
            assert all(n > 0 for (_, _, n), c in zip(res, odd) if c[2] > 3 and c[3] > 3)
            res = _st_check(ctx, orc, slot, img, tiles, mx, quality, responses=False)
            assert all(len(xy) == min(mx, n) > 0 for xy, _, n in res)


@pytest.mark.parametrize("kind", ["noise", "binary", "flat"])
def test_shitomasi_qualities(pmv, orc, gpu_ctx_factory, kind):
    """quality 0.4, 0.05, 0.0 (every positive response) and 1.0 (nothing: the comparison with the maximum is strict); the flat image has no
    feature at any quality and its response map equals the oracle's"""
    w, h = ac.WIDE
    ctx, slot = _slot(gpu_ctx_factory, ac.WIDE, kind)
    img = IMAGES[kind](w, h)
    cells = np.concatenate([pmv.grid_cells(w, h), [[5, 3, 35, 34], [w - 100, h - 77, 100, 77]]]).astype(np.int32)
    seen = {}
    for quality in (0.4, 0.05, 0.0, 1.0):
        for mx in (40, 4096):
            seen[quality, mx] = [len(xy) for xy, _, _ in _st_check(ctx, orc, slot, img, cells, mx, quality, responses=(quality, mx) == (0.4, 40))]
    assert not any(seen[1.0, 40]) and not any(seen[1.0, 4096])
    if kind == "flat":
        assert not any(any(v) for v in seen.values())
    else:
        assert all(v == 40 for v in seen[0.05, 40]) and all(a >= b > 0 for a, b in zip(seen[0.0, 4096], seen[0.4, 4096]))
        assert sum(seen[0.0, 4096]) >= sum(seen[0.05, 4096]) >= sum(seen[0.4, 4096])
        assert kind == "binary" or sum(seen[0.0, 4096]) > sum(seen[0.05, 4096]) > sum(seen[0.4, 4096])   # (binary: bytes 0 and -1, a handful of response values)


# ---- session rounds whose requests differ in their parameters ----------------------------------------------------------------------------
SESSION_SIZES = [ac.SMALL, ac.MID]
SESSION_SLOTS = {(ac.SMALL, "noise"): 0, (ac.SMALL, "shifted"): 1, (ac.MID, "noise"): 2, (ac.MID, "shifted"): 3}
REPEATS = 10


def _session_ctx(gpu_ctx_factory):
    if "session" not in _cache:
        _cache["session"] = gpu_ctx_factory(ac.MID[0], ac.MID[1], n_slots=4, max_tracks=2048)
    return _cache["session"]


def _threads(n, fn):
    res, errors = [None] * n, []

    def run(j):
        try:
            res[j] = fn(j)
        except Exception as e:   # noqa: BLE001
            errors.append((j, repr(e)))
    th = [threading.Thread(target=run, args=(j,)) for j in range(n)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors, errors
    return res


def _run_session(ctx, role, jobs):
    """six threads start together and repeat their own session call; returns their results and the (requests, launches) the role's
    combiner counted meanwhile"""
    with ctx.batch_session(1, SESSION_SIZES):
        for (size, kind), slot in SESSION_SLOTS.items():       # the frames go up once
            ctx.batch_frame_upload(slot, IMAGES[kind](*size))
        before = ctx.batch_stats()[role]
        start = threading.Barrier(len(jobs))

        def run(j):
            start.wait()
            return [jobs[j](ctx) for _ in range(REPEATS)]
        got = _threads(len(jobs), run)
        after = ctx.batch_stats()[role]
    return got, (after["requests"] - before["requests"], after["launches"] - before["launches"])


def _flat(res):
    """the arrays of a detector result (a list per cell of an array or of a tuple of arrays) or of a matcher result, in order"""
    out = []
    for r in res:
        out += list(r) if isinstance(r, tuple) else [r]
    return out


def test_session_rounds_hold_detector_groups_of_different_parameters(pmv, orc, gpu_ctx_factory):
    """process_det groups the requests of a round by kind, max_per_cell, quality / threshold, non-max flag and geometry and lays the groups
    out one after another in the cell records, the result block and the FAST score maps. Six threads, each its own call ten times: three
    FAST parameter sets, ShiTomasi on one spilling cell at two qualities (requests that differ in the quality alone and return different
    counts), GFTT; two frame sizes. Every result equals the single call's,
    which equals the oracle's; 60 requests in fewer launch rounds, so - every thread being serial - some round held different parameter sets."""
    small = pmv.grid_cells(*ac.SMALL)
    whole_mid = np.asarray([[0, 0, *ac.MID]], np.int32)
    spill = np.asarray([[3, 2, 128, 100]], np.int32)
    S = SESSION_SLOTS
    # (size, single / session method, arguments after the slot, the oracle's result per cell)
    jobs = [
        (ac.SMALL, "detect_fast", (small, 50, 10, True), lambda img, c: orc.fast9_cell(img, c, 50, threshold=10, nonmax=True)),
        (ac.MID, "detect_fast", (whole_mid, 500, 0, False), lambda img, c: orc.fast9_cell(img, c, 500, threshold=0, nonmax=False)),
        (ac.SMALL, "detect_fast", (small, 7, 30, True), lambda img, c: orc.fast9_cell(img, c, 7, threshold=30, nonmax=True)),
        (ac.MID, "detect_shitomasi", (spill, 4096, 0.4), lambda img, c: orc.shitomasi_cell(img, c, 4096, quality=0.4)),
        (ac.MID, "detect_shitomasi", (spill, 4096, 0.05), lambda img, c: orc.shitomasi_cell(img, c, 4096, quality=0.05)),
        (ac.SMALL, "detect_gftt", (small, 20), lambda img, c: orc.gftt_cell(img, c, 20)),
    ]
    want = []
    for size, name, args, oracle in jobs:
        ref, slot = _slot(gpu_ctx_factory, size, "noise")
        single = getattr(ref, name)(slot, *args)
        _same(_flat(single), _flat([oracle(ac.noise(*size), c) for c in args[0]]), f"{name}{args[1:]} against the oracle")
        assert all(len(a) > 0 for a in _flat(single)), f"{name}{args[1:]} finds features in every cell"
        want.append(_flat(single))
    R = np.nan_to_num(orc.shitomasi_cell(ac.noise(*ac.MID), spill[0], 40, quality=0.05, want_resp=True)[2])
    assert (R > R.max() * 0.05).sum() > ac.ST_CAP
    # the two ShiTomasi requests differ in nothing but the quality, and it shows: a group that took one quality for both would be seen
    assert len(want[3][0]) < len(want[4][0]) == 4096, (len(want[3][0]), len(want[4][0]))
    ctx = _session_ctx(gpu_ctx_factory)
    calls = [lambda c, size=size, name=name, args=args: getattr(c, "batch_" + name)(S[size, "noise"], *args) for size, name, args, _ in jobs]
    got, (requests, launches) = _run_session(ctx, "det", calls)
    for j, (_, name, args, _) in enumerate(jobs):
        for k in range(REPEATS):
            _same(_flat(got[j][k]), want[j], f"thread {j} ({name}{args[1:]}), call {k}")
    print(f"detector requests {requests} in {launches} rounds")
    assert requests == 6 * REPEATS and 0 < launches < requests, "no round held two requests: the groups never met"


def test_session_rounds_hold_knn_requests_of_different_parameters(orc, gpu_ctx_factory):
    """process_lk packs the kNN requests of a round with their own (n_neighbours, window, m) and geometry index: six threads, six parameter
    sets - a list in HBM (m = 1025) beside lists in LDS, window 63 beside window 1 - over two frame sizes"""
    S = SESSION_SLOTS
    sw_src, sw_cand = ac.knn_sweep_lists(*ac.SMALL)
    params = [(ac.SMALL, 1, 1, 40), (ac.SMALL, 8, 63, 300), (ac.MID, 7, 15, 1025), (ac.MID, 7, 15, 1023), (ac.SMALL, 2, 16, 5), (ac.MID, 8, 2, 1500)]
    jobs, want = [], []
    for size, n_nn, window, m in params:
        src, cand = (sw_src, sw_cand[:m]) if size == ac.SMALL else ac.knn_length_lists(*ac.MID, m, n_nn)
        assert len(cand) == m
        ref, s0, s1, a, b = _knn_pair(gpu_ctx_factory, size, "shifted")
        best, err = _knn_check(ref, orc, s0, s1, a, b, src, cand, n_nn, window, "single call")
        assert (best >= 0).all() and (m <= ac.KNN_LDS_M or (best >= ac.KNN_LDS_M).any())
        want.append([best, err])
        jobs.append(lambda c, size=size, src=src, cand=cand, n_nn=n_nn, window=window:
                    c.batch_knn_match(S[size, "noise"], S[size, "shifted"], src, cand, neighbours=n_nn, window=window))
    got, (requests, launches) = _run_session(_session_ctx(gpu_ctx_factory), "lk", jobs)
    for j, p in enumerate(params):
        for k in range(REPEATS):
            _same(list(got[j][k]), want[j], f"thread {j} {p[1:]}, call {k}")
    print(f"kNN requests {requests} in {launches} rounds")
    assert requests == 6 * REPEATS and 0 < launches < requests, "no round held two requests: the parameter sets never met"
