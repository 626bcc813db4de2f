"""Sequences of different frame sizes in ONE batch (the reference takes whatever cv::imread returns, Frame.cpp:31-42; KITTI odometry comes in
three sizes): pmv_pipeline_run_batch / pmv_pipeline_run_batch_streamed on a mix of sizes must give, for every sequence, exactly the bits of
that sequence's own pmv_pipeline_run - through ONE k_lk_batch launch per LK round and one k_pad_level0 / k_pyrdown launch per feeder round and
level, whatever sizes the round holds. Sizes A, B, C are the three KITTI sizes (pyramid levels 0-3), D is 640 x 200 (levels 0-2)."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZES = {
    "A": dict(w=1241, h=376, f=718.856, cx=607.1928, cy=185.2157),
    "B": dict(w=1242, h=375, f=721.5377, cx=609.5593, cy=172.854),
    "C": dict(w=1226, h=370, f=707.0912, cx=601.8873, cy=183.1104),
    "D": dict(w=640, h=200, f=370.0, cx=320.0, cy=100.0),
}
CAP_W, CAP_H = 1242, 376
STAT_KEYS = ("lk_calls", "lk_points", "detect_calls", "pnp_calls", "pnp_points", "tri_calls", "ba_calls", "ba_obs", "ba_points", "init_offset")
# the six sequences of the staged and streamed cases: sizes A B C D A D, different lengths and seeds
MIX = [("A", 60, 1010), ("B", 41, 1011), ("C", 75, 1012), ("D", 33, 1013), ("A", 52, 1014), ("D", 60, 1015)]

_cache = {}


def _K(size):
    c = SIZES[size]
    return np.array([c["f"], 0, c["cx"], 0, c["f"], c["cy"], 0, 0, 1.0])


def _synth(pmv, size, n, seed):
    key = ("synth", size, n, seed)
    if key not in _cache:
        c = SIZES[size]
        _cache[key] = pmv.synth_sequence(seed, 0, n, c["w"], c["h"], c["f"], c["f"], c["cx"], c["cy"], nthreads=16)
    return _cache[key]


def _assert_same(a, b, what):
    assert np.array_equal(a.poses, b.poses), f"{what}: poses differ"
    assert len(a.features) == len(b.features), f"{what}: frame counts differ"
    for k, (x, y) in enumerate(zip(a.features, b.features)):
        assert np.array_equal(x, y), f"{what}: features of frame {k} differ"
    for key in STAT_KEYS:
        assert a.stats[key] == b.stats[key], (what, key, a.stats[key], b.stats[key])


def _stage(ctx, data):
    seqs, first = [], 0
    for frames, gt in data:
        ctx.frames_stage(first, frames)
        seqs.append((first, len(frames), gt))
        first += len(frames)
    return seqs


def _wh(mix):
    return [SIZES[s]["w"] for s, _, _ in mix], [SIZES[s]["h"] for s, _, _ in mix]


def _single_ctx(gpu_ctx_factory):
    if "single" not in _cache:
        _cache["single"] = gpu_ctx_factory(CAP_W, CAP_H, n_slots=80, max_tracks=4096)
    return _cache["single"]


def _single(pmv, gpu_ctx_factory, size, n, seed, **kw):
    """the sequence's own pmv_pipeline_run (two host threads, as the sequences of a batch), in a context of its own"""
    key = ("single", size, n, seed, tuple(sorted(kw.items())))
    if key not in _cache:
        frames, gt = _synth(pmv, size, n, seed)
        ctx = _single_ctx(gpu_ctx_factory)
        ctx.frames_stage(0, frames)
        _cache[key] = ctx.pipeline_run(n, SIZES[size]["w"], SIZES[size]["h"], _K(size), gt, threaded=1, **kw)
    return _cache[key]


def _staged_mix(pmv, gpu_ctx_factory):
    """the six sequences staged back to back, one pipeline_run_batch; with the engine's and the launch counters around it"""
    if "staged_mix" not in _cache:
        data = [_synth(pmv, s, n, seed) for s, n, seed in MIX]
        ctx = gpu_ctx_factory(CAP_W, CAP_H, n_slots=sum(n for _, n, _ in MIX), max_tracks=4096)
        seqs = _stage(ctx, data)
        w, h = _wh(MIX)
        ctx.lk_counters(reset=True)
        l0, s0 = ctx.batch_launches(), ctx.batch_stats()
        got = ctx.pipeline_run_batch(seqs, w, h, np.stack([_K(s) for s, _, _ in MIX]))
        _cache["staged_mix"] = dict(ctx=ctx, seqs=seqs, got=got, lk=ctx.lk_counters(), launches=(l0, ctx.batch_launches()), stats=(s0, ctx.batch_stats()))
    return _cache["staged_mix"]


def test_staged_mixed_sizes_equal_single_runs(pmv, gpu_ctx_factory):
    """1. sizes A B C D A D in one staged batch: every result is its own single run's, bit for bit; the LK work of the batch is the sum of
    the single runs'. (Before sizes per sequence this call returned PMV_ERR_INVALID.)"""
    run = _staged_mix(pmv, gpu_ctx_factory)
    single = _single_ctx(gpu_ctx_factory)
    work = np.zeros(3, np.int64)
    for b, (size, n, seed) in enumerate(MIX):
        key = ("single", size, n, seed, ())
        fresh = key not in _cache
        single.lk_counters(reset=True)
        ref = _single(pmv, gpu_ctx_factory, size, n, seed)
        assert fresh, "the single runs of this test are counted as they run"
        work += np.array(single.lk_counters(), np.int64)
        _assert_same(run["got"][b], ref, f"sequence {b} ({size}, {n} frames)")
        assert ref.stats["lk_calls"] == n - 1 and ref.stats["ba_calls"] > 0 and ref.stats["pnp_calls"] > 0, "the sequence runs to its end through every stage"
    assert tuple(int(v) for v in work) == run["lk"] and run["lk"][2] > 0
    # a second batch on the same engine, other order, other batch size, another mix
    ctx, seqs = run["ctx"], run["seqs"]
    pick = (3, 1, 4)
    again = ctx.pipeline_run_batch([seqs[b] for b in pick], [SIZES[MIX[b][0]]["w"] for b in pick], [SIZES[MIX[b][0]]["h"] for b in pick],
                                   np.stack([_K(MIX[b][0]) for b in pick]))
    for r, b in zip(again, pick):
        _assert_same(r, run["got"][b], f"re-run of sequence {b}")


def test_one_launch_per_round_whatever_the_sizes(pmv, gpu_ctx_factory):
    """2. LK sequences of four sizes: k_lk_batch launches <= LK combiner rounds < LK requests (sizes really share launches); streamed:
    k_pad_level0 launches <= ingest rounds, k_pyrdown launches <= 3 x ingest rounds (the largest pyramid has levels 0-3). Counted by
    pmv_debug_batch_launches: the profiler's per-class event pools are not made for the two LK lanes."""
    run = _staged_mix(pmv, gpu_ctx_factory)
    (l0, l1), (s0, s1) = run["launches"], run["stats"]
    lk_launches = l1["k_lk_batch"] - l0["k_lk_batch"]
    rounds = s1["lk"]["launches"] - s0["lk"]["launches"]
    requests = s1["lk"]["requests"] - s0["lk"]["requests"]
    print("staged mix: k_lk_batch launches", lk_launches, "LK rounds", rounds, "LK requests", requests)
    assert 0 < lk_launches <= rounds < requests
    assert l1["k_knn_round"] == l0["k_knn_round"]
    st = _streamed_mix(pmv, gpu_ctx_factory, "gray", None)
    l0, l1 = st["launches"]
    pad, pyr, ing = l1["k_pad_level0"] - l0["k_pad_level0"], l1["k_pyrdown"] - l0["k_pyrdown"], st["ingest"]
    print("streamed mix: k_pad_level0 launches", pad, "k_pyrdown launches", pyr, "ingest", ing)
    assert 0 < pad <= ing["rounds"] and 0 < pyr <= 3 * ing["rounds"]
    assert ing["rounds"] < ing["frames"] == sum(n for _, n, _ in MIX), "rounds hold frames of several sequences"


def _sources(pmv, fmt):
    """host frames of the six sequences: pinned memory for sequences 0, 3 and 4 (one of every level count), pageable for the others"""
    import torch   # only to get page-locked host memory
    key = ("sources", fmt)
    if key not in _cache:
        out, keep = [], []
        for b, (size, n, seed) in enumerate(MIX):
            frames, gt = _synth(pmv, size, n, seed)
            if fmt == "bgr":   # B = G = R: cv::cvtColor(BGR2GRAY) of it is the gray frame itself
                frames = np.ascontiguousarray(np.repeat(frames[..., None], 3, axis=3))
            if b in (0, 3, 4):
                pinned = torch.empty(frames.shape, dtype=torch.uint8).pin_memory()
                pinned.numpy()[:] = frames
                keep.append(pinned)
                frames = pinned.numpy()
            out.append((frames, gt))
        _cache[key] = (out, keep)
    return _cache[key][0]


def _streamed_mix(pmv, gpu_ctx_factory, fmt, mode):
    key = ("streamed_mix", fmt, mode)
    if key not in _cache:
        ring = 8
        ckey = ("streamed_ctx", fmt)
        if ckey not in _cache:
            _cache[ckey] = gpu_ctx_factory(CAP_W, CAP_H, n_slots=len(MIX) * ring, max_tracks=4096)
            if fmt == "bgr":
                _cache[ckey].set_frame_format("bgr")
        ctx = _cache[ckey]
        old = os.environ.get("PMV_BATCH_INGEST")
        if mode is not None:
            os.environ["PMV_BATCH_INGEST"] = mode
        try:
            l0 = ctx.batch_launches()
            got = ctx.pipeline_run_batch_streamed(_sources(pmv, fmt), K=np.stack([_K(s) for s, _, _ in MIX]), ring=ring)
        finally:
            if mode is not None:
                if old is None:
                    del os.environ["PMV_BATCH_INGEST"]
                else:
                    os.environ["PMV_BATCH_INGEST"] = old
        _cache[key] = dict(got=got, launches=(l0, ctx.batch_launches()), ingest=ctx.batch_ingest_stats())
    return _cache[key]


@pytest.mark.parametrize("fmt", ["gray", "bgr"])
@pytest.mark.parametrize("mode", ["mapped", "copy"])
def test_streamed_mixed_sizes_equal_staged(pmv, gpu_ctx_factory, fmt, mode):
    """3. the six sequences from host memory through rings of 8 slots (every sequence is longer than its ring), pinned and pageable sources
    in one batch, both ingest forms, gray and colour frames (B = G = R, whose gray conversion is the gray input): the bits of the staged mix"""
    ref = _staged_mix(pmv, gpu_ctx_factory)["got"]
    st = _streamed_mix(pmv, gpu_ctx_factory, fmt, mode)
    for b, (size, n, _) in enumerate(MIX):
        _assert_same(st["got"][b], ref[b], f"{fmt}, {mode}: sequence {b} ({size}, {n} frames)")
    ing = st["ingest"]
    bytes_moved = sum(n * SIZES[s]["w"] * SIZES[s]["h"] for s, n, _ in MIX) * (3 if fmt == "bgr" else 1)
    assert ing["frames"] == sum(n for _, n, _ in MIX) and ing["bytes"] == bytes_moved, ing


@pytest.mark.parametrize("name, pairs", [
    ("ShiTomasi on some", {"A": (1, 0), "B": (0, 0), "C": (1, 0), "D": (0, 0)}),
    ("kNN over FAST next to LK", {"A": (2, 1), "D": (2, 1), "B": (0, 0), "C": (0, 0)}),
])
def test_plugins_in_a_mixed_size_batch(pmv, gpu_ctx_factory, name, pairs):
    """4. every extractor (GFTT, ShiTomasi, FAST) and both matchers in batches of four sizes: each sequence equals its single run with
    the same plugins (the detectors make one launch group per (kind, parameters, layout), the kNN round one launch for all sizes)"""
    mix = [(s, 36, 1010 + i) for i, s in enumerate("ABCD")]
    data = [_synth(pmv, s, n, seed) for s, n, seed in mix]
    if "plugin_ctx" not in _cache:
        _cache["plugin_ctx"] = gpu_ctx_factory(CAP_W, CAP_H, n_slots=4 * 36, max_tracks=4096)
        _cache["plugin_seqs"] = _stage(_cache["plugin_ctx"], data)
    ctx, seqs = _cache["plugin_ctx"], _cache["plugin_seqs"]
    w, h = _wh(mix)
    l0 = ctx.batch_launches()
    got = ctx.pipeline_run_batch(seqs, w, h, np.stack([_K(s) for s, _, _ in mix]), extractor=[pairs[s][0] for s, _, _ in mix],
                                 matcher=[pairs[s][1] for s, _, _ in mix])
    l1 = ctx.batch_launches()
    for b, (size, n, seed) in enumerate(mix):
        ex, ma = pairs[size]
        kw = {k: v for k, v in (("extractor", ex), ("matcher", ma)) if v}
        _assert_same(got[b], _single(pmv, gpu_ctx_factory, size, n, seed, **kw), f"{name}: sequence {b} ({size}, extractor {ex}, matcher {ma})")
    if any(ma for _, ma in pairs.values()):
        assert l1["k_knn_round"] > l0["k_knn_round"] and l1["k_lk_batch"] > l0["k_lk_batch"]


def test_same_size_batches_are_untouched(pmv, gpu_ctx_factory):
    """5. the six same-size sequences of tests/test_batch_gpu.py's first case: w = [..] * B gives the bits of the scalar form"""
    c = SIZES["A"]
    lengths, seeds = [60, 41, 75, 33, 52, 60], [1000, 1001, 1002, 1003, 1004, 1000]
    ctx = gpu_ctx_factory(c["w"], c["h"], n_slots=sum(lengths), max_tracks=4096)
    data = [pmv.synth_sequence(seed, 0, n, c["w"], c["h"], c["f"], c["f"], c["cx"], c["cy"], nthreads=16) for n, seed in zip(lengths, seeds)]
    seqs = _stage(ctx, data)
    scalar = ctx.pipeline_run_batch(seqs, c["w"], c["h"], _K("A"))
    listed = ctx.pipeline_run_batch(seqs, [c["w"]] * 6, [c["h"]] * 6, _K("A"))
    for b in range(6):
        _assert_same(listed[b], scalar[b], f"sequence {b}")
    _assert_same(scalar[0], scalar[5], "same input in two batch slots")


def test_errors_are_refused_before_any_sequence_starts(pmv, gpu_ctx_factory):
    """6. a sequence larger than the capacity: PMV_ERR_CAPACITY (-3); two staged sequences of different sizes over one slot range, and a staged
    sequence whose w, h are not what was staged: PMV_ERR_INVALID (-2); nothing reaches a combiner, and a valid batch then succeeds"""
    n = 20
    d, a = _synth(pmv, "D", n, 1013), _synth(pmv, "A", n, 1010)
    ctx = gpu_ctx_factory(CAP_W, CAP_H, n_slots=2 * n, max_tracks=4096)
    ctx.frames_stage(0, d[0])
    ctx.frames_stage(n, a[0])
    Ks = np.stack([_K("D"), _K("A")])
    before = ctx.batch_stats()

    def refused(code, call):
        with pytest.raises(pmv.PmvError) as e:
            call()
        assert e.value.code == code, e.value
        assert ctx.batch_stats() == before, "a request reached a combiner"

    big = (np.zeros((n, CAP_H, CAP_W + 1), np.uint8), a[1])
    refused(-3, lambda: ctx.pipeline_run_batch_streamed([d, big], K=Ks, ring=8))
    refused(-3, lambda: ctx.pipeline_run_batch([(0, n, d[1]), (n, n, a[1])], [640, CAP_W + 1], [200, CAP_H], Ks))
    refused(-2, lambda: ctx.pipeline_run_batch([(0, n, d[1]), (0, n, d[1])], [640, 1241], [200, 376], Ks))   # one range, two sizes
    refused(-2, lambda: ctx.pipeline_run_batch([(0, n, d[1]), (n, n, a[1])], [640, 1242], [200, 376], Ks))   # sequence 1 was staged as 1241 x 376
    assert "sequence 1" in str(pytest.raises(pmv.PmvError, ctx.pipeline_run_batch, [(0, n, d[1]), (n, n, a[1])], [640, 1242], [200, 376], Ks).value)
    got = ctx.pipeline_run_batch([(0, n, d[1]), (n, n, a[1])], [640, 1241], [200, 376], Ks)
    _assert_same(got[0], _single(pmv, gpu_ctx_factory, "D", n, 1013), "after the refusals: sequence 0")
    _assert_same(got[1], _single(pmv, gpu_ctx_factory, "A", n, 1010), "after the refusals: sequence 1")
