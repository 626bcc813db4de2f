"""Colour (BGR) host frames on every staged, streamed and batched path (pmv_set_frame_format; Frame::Frame / Frame::init, Frame.cpp:33,40-41).
Every comparison is bitwise, and the expected side is always the existing GRAY path run on the oracle's cvtColor(BGR2GRAY) of the same frames
(orc.bgr2gray, pinned by a numpy twin in test_oracle_frontend.py), never the code under test."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

K00 = dict(w=1241, h=376, fx=718.856, fy=718.856, cx=607.1928, cy=185.2157)
K = np.array([K00["fx"], 0, K00["cx"], 0, K00["fy"], K00["cy"], 0, 0, 1.0])
W, H = K00["w"], K00["h"]
# (seed, first frame) of a synthetic sequence whose initialise() keeps a frame other than the first: init_offset = 2 (CPU oracle; also on
# the gray of its coloured frames)
SEED_INIT_OFFSET = (1001, 213)
RING = 8
COUNTS = ("lk_calls", "lk_points", "detect_calls", "pnp_calls", "pnp_points", "tri_calls", "ba_calls", "ba_obs", "ba_points", "heuristic_motion",
          "init_offset", "n_landmarks", "scale", "tri_hypotheses")


def _synth(pmv, n, seed, first=0):
    return pmv.synth_sequence(seed, first, n, W, H, K00["fx"], K00["fy"], K00["cx"], K00["cy"], nthreads=16)


def colourise(gray):
    """(n, h, w) gray -> (n, h, w, 3) BGR: the gray scene plus three different smooth, deterministic per-channel offset fields, clipped"""
    n, h, w = gray.shape
    yy, xx = np.mgrid[0:h, 0:w]
    fields = (25 + 20 * np.sin(2 * np.pi * xx / w * 1.5), -20 + 15 * np.cos(2 * np.pi * yy / h), 10 + 25 * np.sin(2 * np.pi * (xx + yy) / (w + h) * 2))
    return np.stack([np.clip(gray.astype(np.int32) + np.rint(f).astype(np.int32)[None], 0, 255).astype(np.uint8) for f in fields], -1)


def to_gray(orc, bgr):
    n, h, w, _ = bgr.shape
    return orc.bgr2gray(bgr.reshape(n * h, w, 3)).reshape(n, h, w)


def _assert_same(a, b, what):
    assert np.array_equal(a.poses, b.poses), f"{what}: poses differ"
    assert len(a.features) == len(b.features), f"{what}: frame counts differ"
    for k, (x, y) in enumerate(zip(a.features, b.features)):
        assert np.array_equal(x, y), f"{what}: features of frame {k} differ"
    for key in COUNTS:
        assert a.stats[key] == b.stats[key], (what, key, a.stats[key], b.stats[key])


def _staged(ctx, frames_and_gt, **kw):
    """the staged batched run: sequence b in slots [sum(n_<b), ...)"""
    seqs, first = [], 0
    for frames, gt in frames_and_gt:
        ctx.frames_stage(first, frames)
        seqs.append((first, len(frames), gt))
        first += len(frames)
    return ctx.pipeline_run_batch(seqs, W, H, K, **kw)


class Data:
    pass


@pytest.fixture(scope="module")
def data(pmv, orc, gpu_ctx_factory):
    """three distinct colour sequences (one with init_offset > 0), their oracle gray, and the GRAY path's results on that gray: the staged
    batch and, per sequence, its own pipeline_run. Checked here, so that no equality below is vacuous: the conversion changes most pixels
    against every channel, and the gray runs really track."""
    d = Data()
    lengths = [36, 31, 34]
    src = [_synth(pmv, lengths[0], *SEED_INIT_OFFSET), _synth(pmv, lengths[1], 1002), _synth(pmv, lengths[2], 1004)]
    d.gt = [s[1] for s in src]
    d.bgr = [colourise(s[0]) for s in src]
    d.gray = [to_gray(orc, b) for b in d.bgr]
    for b, (c, g) in enumerate(zip(d.bgr, d.gray)):
        for ch in range(3):
            frac = float((g != c[..., ch]).mean())
            print(f"sequence {b}: converted gray differs from channel {ch} on {frac:.3f} of the pixels")
            assert frac > 0.5, (b, ch, frac)
        assert float((c[..., 0] != c[..., 1]).mean()) > 0.5 and float((c[..., 1] != c[..., 2]).mean()) > 0.5 and float((c[..., 0] != c[..., 2]).mean()) > 0.5
    d.n_slots = sum(lengths)
    d.gray_ctx = gpu_ctx_factory(W, H, n_slots=d.n_slots, max_tracks=4096)
    d.ref = _staged(d.gray_ctx, list(zip(d.gray, d.gt)))
    d.single = []
    for g, gt in zip(d.gray, d.gt):
        d.gray_ctx.frames_stage(0, g)
        d.single.append(d.gray_ctx.pipeline_run(len(g), W, H, K, gt, threaded=1))
    for b, (r, s) in enumerate(zip(d.ref, d.single)):
        n = lengths[b]
        for res in (r, s):
            print(f"sequence {b}: gray run: " + ", ".join(f"{k}={res.stats[k]:g}" for k in ("pnp_calls", "ba_calls", "tri_calls", "init_offset")) + f", poses {len(res.poses)}")
            assert res.stats["pnp_calls"] > 0 and res.stats["ba_calls"] > 0 and res.stats["tri_calls"] > 0
            off = int(res.stats["init_offset"])
            # a feature list for every frame from the one initialise() kept, and a pose for each of them but the newest (estimatePose lags one frame)
            assert len(res.features) == n - off and len(res.poses) == n - off - 1 and np.isfinite(res.poses).all()
        _assert_same(r, s, f"gray staged batch vs gray single run, sequence {b}")
    assert d.ref[0].stats["init_offset"] > 0, "the tests need a sequence with init_offset > 0"
    return d


def _pinned(arr, lead=0):
    """a copy of `arr` in page-locked host memory that starts `lead` bytes into its allocation; returns (array, owner)"""
    import torch   # only to get page-locked host memory
    t = torch.empty(arr.size + lead, dtype=torch.uint8).pin_memory()
    a = t.numpy()[lead:].reshape(arr.shape)
    a[:] = arr
    return a, t


def _pageable(arr, lead):
    a = np.empty(arr.size + lead + 64, np.uint8)
    lead += (-a.ctypes.data) % 4   # `lead` bytes past a 4-byte boundary, wherever numpy put the buffer
    a = a[lead:lead + arr.size].reshape(arr.shape)
    a[:] = arr
    return a


# the frame sizes of test_frontend_gpu.py's pyramid tests: odd widths put the rows of a tight BGR frame on every residue mod 4, and both the
# wide and the narrow border paths of the row writer are covered; 23 frames are more than one landing chunk (64 gray / 21 BGR frames);
# 4301 pixels are too wide for four colour rows of LDS per workgroup (the one-row form of the kernel)
@pytest.mark.parametrize("w,h,n", [(1241, 376, 23), (1226, 370, 3), (321, 163, 4), (224, 131, 3), (113, 97, 5), (111, 80, 4), (100, 66, 3), (97, 67, 4), (4301, 131, 2)])
def test_colour_staging_equals_gray_upload(pmv, orc, gpu_ctx_factory, w, h, n):
    rng = np.random.default_rng(w * 1000 + h)
    bgr = rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    gray = to_gray(orc, bgr)
    assert all(float((gray != bgr[..., c]).mean()) > 0.5 for c in range(3))
    ctx = gpu_ctx_factory(w, h, n_slots=n + 1)
    ctx.set_frame_format("bgr")
    ctx.frames_stage(0, _pageable(bgr, 1))   # (the copy engine takes any source address)
    ctx.frames_build(0, n)
    for i in range(n):
        ctx.frame_upload(n, gray[i])         # its own explicit format, whatever the context's
        assert ctx.num_levels(i) == ctx.num_levels(n) >= 1
        for lv in range(ctx.num_levels(n) + 1):
            got, want = ctx.get_level_padded(i, lv, w, h), ctx.get_level_padded(n, lv, w, h)
            assert got.shape == want.shape and np.array_equal(got, want), f"frame {i} level {lv}: {np.argwhere(got != want)[:5]}"
    # the colour upload entry keeps its explicit format as well
    ctx.frame_upload_bgr(n, bgr[0])
    assert np.array_equal(ctx.get_level_padded(n, 0, w, h), ctx.get_level_padded(0, 0, w, h))


@pytest.mark.parametrize("w,h", [(1241, 376), (321, 163), (113, 97), (111, 80), (97, 67)])
@pytest.mark.parametrize("source", ["pinned", "pageable"])
def test_colour_bracket_builds_the_gray_pyramids(pmv, orc, gpu_ctx_factory, w, h, source):
    """the bracket's rounds (copy form by default: DMA straight from a pinned source, through staging from a pageable one) from sources that
    start at an odd byte: every padded level of every slot equals the gray upload's"""
    n = 19   # more than one bracket round (16 frames)
    rng = np.random.default_rng(w * 7 + h)
    bgr = rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    gray = to_gray(orc, bgr)
    src, owner = _pinned(bgr, 3) if source == "pinned" else (_pageable(bgr, 3), None)
    ctx = gpu_ctx_factory(w, h, n_slots=n + 1)
    ctx.set_frame_format("bgr")
    ctx.frames_stream_begin(0, src)
    ctx.frames_stream_end()
    for i in range(n):
        ctx.frame_upload(n, gray[i])
        for lv in range(ctx.num_levels(n) + 1):
            got, want = ctx.get_level_padded(i, lv, w, h), ctx.get_level_padded(n, lv, w, h)
            assert np.array_equal(got, want), f"frame {i} level {lv}: {np.argwhere(got != want)[:5]}"
    del owner


def test_colour_bracket_tracks_while_frames_are_on_their_way(pmv, orc, gpu_ctx_factory, data):
    """detection and LK on slots of an open colour bracket, the first ones at once and the last ones before anything else waited for them,
    equal the same calls on gray uploads"""
    bgr, gray = data.bgr[1], data.gray[1]
    n = len(bgr)
    ctx = gpu_ctx_factory(W, H, n_slots=n, max_tracks=4096)
    ref = gpu_ctx_factory(W, H, n_slots=2, max_tracks=4096)
    cells = pmv.grid_cells(W, H)
    ctx.set_frame_format("bgr")
    ctx.frames_stream_begin(0, bgr)
    try:
        for a, b in ((0, 1), (n - 2, n - 1), (7, 8)):
            ref.frame_upload(0, gray[a])
            ref.frame_upload(1, gray[b])
            det, want = ctx.detect_gftt(a, cells, 30), ref.detect_gftt(0, cells, 30)
            assert all(np.array_equal(x, y) for x, y in zip(det, want)), (a, "corners")
            pts = np.concatenate([d + c[:2] for c, d in zip(cells, want)]).astype(np.float32)
            assert len(pts) > 100
            got_lk, want_lk = ctx.lk_track(a, b, pts), ref.lk_track(0, 1, pts)
            assert int(want_lk[1].sum()) > 50, "LK must really track"
            for x, y in zip(got_lk, want_lk):
                assert np.array_equal(x, y), (a, b, "LK")
    finally:
        ctx.frames_stream_end()


def test_colour_single_streamed_run_equals_gray_run(pmv, gpu_ctx_factory, data):
    ctx = gpu_ctx_factory(W, H, n_slots=max(len(b) for b in data.bgr), max_tracks=4096)
    ctx.set_frame_format("bgr")
    ctx.prof_enable(True)
    for b, (bgr, gt) in enumerate(zip(data.bgr, data.gt)):
        got = ctx.pipeline_run(len(bgr), W, H, K, gt, threaded=1, host_frames=bgr)
        _assert_same(got, data.single[b], f"colour streamed run vs gray pipeline_run, sequence {b}")
    ctx.sync()
    prof = ctx.prof_read()
    ctx.prof_enable(False)
    # level 0 of every frame came from the colour kernel, booked under its own class; the levels above from the unchanged k_pyrdown
    assert "k_pad_level0_bgr" in prof and "k_pad_level0" not in prof and prof["k_pyrdown"][0] == ctx.num_levels(0) * prof["k_pad_level0_bgr"][0] > 0, prof
    got = ctx.pipeline_run(len(data.bgr[2]), W, H, K, data.gt[2], threaded=0, host_frames=_pageable(data.bgr[2], 1))
    _assert_same(got, data.single[2], "colour streamed run, sequential schedule, odd source address")


@pytest.mark.parametrize("mode", ["copy", "mapped"])
def test_colour_batched_streamed_run_equals_gray_batch(pmv, gpu_ctx_factory, data, mode):
    """three distinct sequences (one with init_offset > 0) on rings of 8 slots for 31..36 frames, so every ring wraps; pinned and pageable
    sources, each also sliced at an odd byte offset; PMV_BATCH_INGEST=copy | mapped (test_format_hygiene runs the default form)"""
    pin0, own0 = _pinned(data.bgr[0])
    pin2, own2 = _pinned(data.bgr[2], 1)
    pin1, own1 = _pinned(data.bgr[1], 3)
    seqs = [(pin0, data.gt[0]), (data.bgr[1], data.gt[1]), (pin2, data.gt[2]), (_pageable(data.bgr[0], 1), data.gt[0]), (pin1, data.gt[1]),
            (_pageable(data.bgr[2], 2), data.gt[2])]
    which = [0, 1, 2, 0, 1, 2]
    assert pin2.ctypes.data % 2 == 1 and pin1.ctypes.data % 4 == 3 and seqs[3][0].ctypes.data % 4 == 1
    assert all(len(s[0]) > RING for s in seqs)
    ctx = gpu_ctx_factory(W, H, n_slots=len(seqs) * RING, max_tracks=4096)
    ctx.set_frame_format("bgr")
    old = os.environ.get("PMV_BATCH_INGEST")
    os.environ["PMV_BATCH_INGEST"] = mode
    try:
        got = ctx.pipeline_run_batch_streamed(seqs, W, H, K, ring=RING)
    finally:
        if old is None:
            os.environ.pop("PMV_BATCH_INGEST", None)
        else:
            os.environ["PMV_BATCH_INGEST"] = old
    ing = ctx.batch_ingest_stats()
    print(f"{mode}: ingest counters:", ing)
    frames = sum(len(s[0]) for s in seqs)
    assert ing["frames"] == frames and ing["bytes"] == 3 * W * H * frames and 0 < ing["rounds"] <= frames
    for b, k in enumerate(which):
        _assert_same(got[b], data.ref[k], f"{mode}: colour streamed sequence {b} vs gray staged batch")
        _assert_same(got[b], data.single[k], f"{mode}: colour streamed sequence {b} vs gray single run")
    assert got[0].stats["init_offset"] > 0
    # after the run each ring slot holds the gray pyramid of the last frame that went through it
    other = gpu_ctx_factory(W, H, n_slots=1, max_tracks=1024)
    for b in (0, 4):
        n = len(seqs[b][0])
        for f in range(n - RING, n):
            other.frame_upload(0, data.gray[which[b]][f])
            for lv in range(other.num_levels(0) + 1):
                assert np.array_equal(ctx.get_level_padded(b * RING + f % RING, lv, W, H), other.get_level_padded(0, lv, W, H)), (b, f, lv)
    del own0, own1, own2


def test_colour_staged_batch_equals_gray_batch(pmv, gpu_ctx_factory, data):
    ctx = gpu_ctx_factory(W, H, n_slots=data.n_slots, max_tracks=4096)
    ctx.set_frame_format("bgr")
    got = _staged(ctx, list(zip(data.bgr, data.gt)))
    for b in range(3):
        _assert_same(got[b], data.ref[b], f"colour staged batch vs gray staged batch, sequence {b}")
    # staged slots hold gray: the single run over colour-staged slots as well
    ctx.frames_stage(0, data.bgr[0])
    _assert_same(ctx.pipeline_run(len(data.bgr[0]), W, H, K, data.gt[0], threaded=1), data.single[0], "pipeline_run over colour-staged slots")


def test_gray_sent_as_bgr_is_the_identity(pmv, gpu_ctx_factory):
    """quirk Q2: a gray sequence as B = G = R (what imread(IMREAD_COLOR) makes of KITTI's gray PNGs) gives the gray path's results"""
    frames, gt = _synth(pmv, 30, 1006)
    n = len(frames)
    gray_ctx = gpu_ctx_factory(W, H, n_slots=n, max_tracks=4096)
    gray_ctx.frames_stage(0, frames)
    want = gray_ctx.pipeline_run(n, W, H, K, gt, threaded=1)
    assert want.stats["pnp_calls"] > 0 and want.stats["ba_calls"] > 0 and len(want.poses) > 20
    bgr = np.repeat(frames[..., None], 3, axis=3)
    ctx = gpu_ctx_factory(W, H, n_slots=2 * RING + n, max_tracks=4096)
    ctx.set_frame_format("bgr")
    _assert_same(ctx.pipeline_run(n, W, H, K, gt, threaded=1, host_frames=bgr), want, "B = G = R, single streamed run")
    for r in ctx.pipeline_run_batch_streamed([(bgr, gt), (bgr, gt)], W, H, K, ring=RING):
        _assert_same(r, want, "B = G = R, streamed batch")
    ctx.frames_stage(2 * RING, bgr)
    ctx.frames_build(2 * RING, n)
    other = gpu_ctx_factory(W, H, n_slots=1, max_tracks=1024)
    other.frame_upload(0, frames[n - 1])
    assert np.array_equal(ctx.get_level_padded(2 * RING + n - 1, 0, W, H), other.get_level_padded(0, 0, W, H))


def test_format_hygiene(pmv, gpu_ctx_factory, data):
    """one context, one engine: colour, then gray again, then colour; unknown formats and a change under an open bracket are refused and
    leave the format as it was"""
    ctx = gpu_ctx_factory(W, H, n_slots=3 * RING + 4, max_tracks=4096)
    lib = pmv.load_library()
    frames = sum(len(b) for b in data.bgr)
    assert ctx.frame_format == "gray"
    ctx.set_frame_format("bgr")
    colour = ctx.pipeline_run_batch_streamed(list(zip(data.bgr, data.gt)), W, H, K, ring=RING)
    assert ctx.batch_ingest_stats()["bytes"] == 3 * W * H * frames
    for bad in (2, -1, 3, 255):
        assert lib.pmv_set_frame_format(ctx.h, bad) == -2
        assert b"format" in lib.pmv_last_error(ctx.h)
    with pytest.raises(ValueError):
        ctx.set_frame_format("rgb")
    # still BGR after the refused calls
    again = ctx.pipeline_run_batch_streamed(list(zip(data.bgr, data.gt)), W, H, K, ring=RING)
    ctx.set_frame_format("gray")
    gray = ctx.pipeline_run_batch_streamed(list(zip(data.gray, data.gt)), W, H, K, ring=RING)
    assert ctx.batch_ingest_stats()["bytes"] == W * H * frames
    for b in range(3):
        _assert_same(colour[b], data.ref[b], f"colour run, sequence {b}")
        _assert_same(again[b], data.ref[b], f"colour run after refused format changes, sequence {b}")
        _assert_same(gray[b], data.ref[b], f"gray run after a colour run on the same context and engine, sequence {b}")
    # gray staging and the gray bracket are back as well
    ctx.frames_stage(3 * RING, data.gray[1][:4])
    ctx.frames_build(3 * RING, 4)
    other = gpu_ctx_factory(W, H, n_slots=1, max_tracks=1024)
    other.frame_upload(0, data.gray[1][3])
    assert np.array_equal(ctx.get_level_padded(3 * RING + 3, 0, W, H), other.get_level_padded(0, 0, W, H))
    # a change while a bracket is open is refused, in both directions, and the bracket finishes in its own format
    ctx.frames_stream_begin(0, data.gray[2][:12])
    try:
        with pytest.raises(pmv.PmvError) as e:
            ctx.set_frame_format("bgr")
        assert e.value.code == -2 and ctx.frame_format == "gray"
        assert lib.pmv_set_frame_format(ctx.h, 0) == -2
    finally:
        ctx.frames_stream_end()
    other.frame_upload(0, data.gray[2][11])
    assert np.array_equal(ctx.get_level_padded(11, 0, W, H), other.get_level_padded(0, 0, W, H))
    ctx.set_frame_format("bgr")   # accepted once the bracket is closed
    ctx.frames_stream_begin(0, data.bgr[2][:12])
    try:
        with pytest.raises(pmv.PmvError) as e:
            ctx.set_frame_format("gray")
        assert e.value.code == -2 and ctx.frame_format == "bgr"
    finally:
        ctx.frames_stream_end()
    assert np.array_equal(ctx.get_level_padded(11, 0, W, H), other.get_level_padded(0, 0, W, H))
