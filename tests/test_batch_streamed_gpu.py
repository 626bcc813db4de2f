"""Streamed batched path: pmv_pipeline_run_batch_streamed moves B sequences' frames from host memory through per-sequence rings of recycled
frame slots while they track. Every sequence's result must equal, bit for bit, the staged pmv_pipeline_run_batch on the same frames and its
own pmv_pipeline_run, whatever the ring size, the kind of source memory or the ingest form."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

K00 = dict(w=1241, h=376, fx=718.856, fy=718.856, cx=607.1928, cy=185.2157)
K = np.array([K00["fx"], 0, K00["cx"], 0, K00["fy"], K00["cy"], 0, 0, 1.0])
W, H = K00["w"], K00["h"]
# (seed, first frame) of a synthetic sequence whose initialise() keeps a frame other than the first: init_offset = 2 (CPU oracle)
SEED_INIT_OFFSET = (1001, 213)


def _synth(pmv, n, seed, first=0):
    return pmv.synth_sequence(seed, first, n, W, H, K00["fx"], K00["fy"], K00["cx"], K00["cy"], nthreads=16)


def _staged(ctx, data, **kw):
    """the staged batched run on the same frames: sequence b in slots [sum(n_<b), ...)"""
    seqs, first = [], 0
    for frames, gt in data:
        ctx.frames_stage(first, frames)
        seqs.append((first, len(frames), gt))
        first += len(frames)
    return ctx.pipeline_run_batch(seqs, W, H, K, **kw)


def _assert_same(a, b, what):
    assert np.array_equal(a.poses, b.poses), f"{what}: poses differ"
    assert len(a.features) == len(b.features), f"{what}: frame counts differ"
    for k, (x, y) in enumerate(zip(a.features, b.features)):
        assert np.array_equal(x, y), f"{what}: features of frame {k} differ"
    for key in ("lk_calls", "lk_points", "detect_calls", "pnp_calls", "pnp_points", "tri_calls", "ba_calls", "ba_obs", "ba_points",
                "heuristic_motion", "init_offset", "n_landmarks", "scale", "tri_hypotheses"):
        assert a.stats[key] == b.stats[key], (what, key, a.stats[key], b.stats[key])


def test_six_sequences_on_rings_equal_staged_and_single(pmv, gpu_ctx_factory):
    """the staged batch test's six sequences on rings of 8 slots: 48 slots for 321 frames"""
    lengths = [60, 41, 75, 33, 52, 60]
    seeds = [1000, 1001, 1002, 1003, 1004, 1000]
    data = [_synth(pmv, n, s) for n, s in zip(lengths, seeds)]
    ctx = gpu_ctx_factory(W, H, n_slots=48, max_tracks=4096)
    ctx.lk_counters(reset=True)
    got = ctx.pipeline_run_batch_streamed(data, W, H, K, ring=8)
    lk_streamed = ctx.lk_counters()
    ing = ctx.batch_ingest_stats()
    print("ingest counters:", ing)
    assert ing["frames"] == sum(lengths) and ing["bytes"] == sum(lengths) * W * H and 0 < ing["rounds"] <= sum(lengths)
    staged_ctx = gpu_ctx_factory(W, H, n_slots=sum(lengths), max_tracks=4096)
    ref = _staged(staged_ctx, data)
    single = gpu_ctx_factory(W, H, n_slots=max(lengths), max_tracks=4096)
    single.lk_counters(reset=True)
    for b, (frames, gt) in enumerate(data):
        _assert_same(got[b], ref[b], f"sequence {b} vs staged batch")
        single.frames_stage(0, frames)
        _assert_same(got[b], single.pipeline_run(lengths[b], W, H, K, gt, threaded=1), f"sequence {b} vs single run")
    assert lk_streamed == single.lk_counters() and lk_streamed[2] > 0
    _assert_same(got[0], got[5], "same input in two batch slots")


def test_ring_sizes_give_identical_results(pmv, gpu_ctx_factory):
    """the smallest legal ring (init_frames + 1), 8, and a ring longer than every sequence (no recycling); one sequence keeps a frame other
    than the first in initialise(), so the release rule's index mapping (frames index + init_offset) is exercised"""
    lengths = [40, 47, 35]
    data = [_synth(pmv, 40, *SEED_INIT_OFFSET), _synth(pmv, 47, 1002), _synth(pmv, 35, 1004)]
    ctx = gpu_ctx_factory(W, H, n_slots=3 * max(lengths), max_tracks=4096)
    results = {ring: ctx.pipeline_run_batch_streamed(data, W, H, K, ring=ring) for ring in (6, 8, max(lengths))}
    assert results[6][0].stats["init_offset"] > 0, "the test needs a sequence with init_offset > 0"
    staged_ctx = gpu_ctx_factory(W, H, n_slots=sum(lengths), max_tracks=4096)
    ref = _staged(staged_ctx, data)
    for ring, got in results.items():
        for b in range(len(data)):
            _assert_same(got[b], ref[b], f"ring {ring}, sequence {b}")


def test_long_initialisation_window_on_its_minimal_ring(pmv, gpu_ctx_factory):
    """init_frames = 10 on a ring of 11: initialise() needs ten frames at once, more than an ingest round hands a sequence by default"""
    data = [_synth(pmv, 30, 1003), _synth(pmv, 26, 1005), _synth(pmv, 33, 1007)]
    ctx = gpu_ctx_factory(W, H, n_slots=3 * 11, max_tracks=4096)
    got = ctx.pipeline_run_batch_streamed(data, W, H, K, ring=11, init_frames=10)
    staged_ctx = gpu_ctx_factory(W, H, n_slots=89, max_tracks=4096)
    ref = _staged(staged_ctx, data, init_frames=10)
    for b in range(len(data)):
        _assert_same(got[b], ref[b], f"init_frames 10, sequence {b}")


def test_long_sequence_and_sixteen_sequences(pmv, gpu_ctx_factory):
    """320 frames on a ring of 8 (the ring wraps 40 times) next to 16 sequences of 120 frames"""
    data = [_synth(pmv, 320, 1003)] + [_synth(pmv, 120, 1000 + b % 8) for b in range(16)]
    ring = 8
    ctx = gpu_ctx_factory(W, H, n_slots=17 * ring, max_tracks=4096)
    got = ctx.pipeline_run_batch_streamed(data, W, H, K, ring=ring)
    staged_ctx = gpu_ctx_factory(W, H, n_slots=320 + 16 * 120, max_tracks=4096)
    ref = _staged(staged_ctx, data)
    for b in range(len(data)):
        _assert_same(got[b], ref[b], f"sequence {b} ({len(data[b][0])} frames)")


def test_source_kinds_and_modes(pmv, gpu_ctx_factory):
    """pinned (torch pin_memory) and pageable sources, two sequences aliasing one buffer of each kind, both front-end schedules, the
    ShiTomasi extractor and the 800-track / bundle-10 configuration"""
    import torch   # only to get page-locked host memory
    a, b_, c = _synth(pmv, 30, 1005), _synth(pmv, 26, 1006), _synth(pmv, 38, 1007)
    pinned = torch.empty(a[0].shape, dtype=torch.uint8).pin_memory()
    pinned.numpy()[:] = a[0]
    pin = (pinned.numpy(), a[1])
    seqs = [pin, pin, b_, c, c]
    data = [a, a, b_, c, c]
    ctx = gpu_ctx_factory(W, H, n_slots=5 * 8, max_tracks=4096)
    staged_ctx = gpu_ctx_factory(W, H, n_slots=sum(len(d[0]) for d in data), max_tracks=4096)
    for kw in (dict(), dict(threaded=0), dict(extractor=1), dict(min_tracked=800, tol=300, bundle_size=10)):
        got = ctx.pipeline_run_batch_streamed(seqs, W, H, K, ring=8, **kw)
        ref = _staged(staged_ctx, data, **kw)
        for b in range(len(seqs)):
            _assert_same(got[b], ref[b], f"{kw}: sequence {b}")


@pytest.mark.parametrize("mode", ["copy", "mapped"])
def test_ingest_forms_give_identical_results(pmv, gpu_ctx_factory, mode):
    """PMV_BATCH_INGEST=copy | mapped (read at every call) changes no result, for a pinned and a pageable source"""
    import torch
    a, b_ = _synth(pmv, 34, 1008), _synth(pmv, 29, 1002)
    pinned = torch.empty(a[0].shape, dtype=torch.uint8).pin_memory()
    pinned.numpy()[:] = a[0]
    ctx = gpu_ctx_factory(W, H, n_slots=2 * 7, max_tracks=4096)
    old = os.environ.get("PMV_BATCH_INGEST")
    os.environ["PMV_BATCH_INGEST"] = mode
    try:
        got = ctx.pipeline_run_batch_streamed([(pinned.numpy(), a[1]), b_], W, H, K, ring=7)
    finally:
        if old is None:
            del os.environ["PMV_BATCH_INGEST"]
        else:
            os.environ["PMV_BATCH_INGEST"] = old
    staged_ctx = gpu_ctx_factory(W, H, n_slots=63, max_tracks=4096)
    ref = _staged(staged_ctx, [a, b_])
    for b in range(2):
        _assert_same(got[b], ref[b], f"{mode}: sequence {b}")


def test_ring_slots_hold_the_pyramids_of_the_last_frames(pmv, gpu_ctx_factory):
    """after a streamed run, each ring slot holds the last frame that went through it: every padded level equals frame_upload's"""
    ring = 6
    data = [_synth(pmv, 20, 1004), _synth(pmv, 13, 1006)]
    ctx = gpu_ctx_factory(W, H, n_slots=2 * ring + 3, max_tracks=4096)
    ctx.pipeline_run_batch_streamed(data, W, H, K, ring=ring, first_slot=[ring + 3, 0])
    other = gpu_ctx_factory(W, H, n_slots=1, max_tracks=1024)
    for (frames, _), first in zip(data, (ring + 3, 0)):
        n = len(frames)
        for f in range(n - ring, n):
            other.frame_upload(0, frames[f])
            slot = first + f % ring
            assert ctx.num_levels(slot) == other.num_levels(0) >= 1
            for lv in range(other.num_levels(0) + 1):
                assert np.array_equal(ctx.get_level_padded(slot, lv, W, H), other.get_level_padded(0, lv, W, H)), (first, f, lv)


def test_engine_reuse_staged_streamed_staged(pmv, gpu_ctx_factory):
    """one context, one batch engine: staged batch, streamed batch, staged batch again - all unchanged"""
    data = [_synth(pmv, 31, 1000), _synth(pmv, 27, 1003), _synth(pmv, 36, 1005)]
    staged_slots = sum(len(d[0]) for d in data)
    ctx = gpu_ctx_factory(W, H, n_slots=staged_slots + 3 * 8, max_tracks=4096)
    first = _staged(ctx, data)
    streamed = ctx.pipeline_run_batch_streamed(data, W, H, K, ring=8, first_slot=[staged_slots + 8 * b for b in range(3)])
    again = _staged(ctx, data)
    for b in range(3):
        _assert_same(streamed[b], first[b], f"streamed vs staged, sequence {b}")
        _assert_same(again[b], first[b], f"staged after streamed, sequence {b}")


def test_argument_errors_leave_the_context_usable(pmv, gpu_ctx_factory):
    data = [_synth(pmv, 14, 1002), _synth(pmv, 12, 1004)]
    ctx = gpu_ctx_factory(W, H, n_slots=16, max_tracks=4096)
    ok = None

    def expect(codes, **kw):
        nonlocal ok
        with pytest.raises(pmv.PmvError) as e:
            ctx.pipeline_run_batch_streamed(data, W, H, K, **kw)
        assert e.value.code in codes, (kw, e.value)
        got = ctx.pipeline_run_batch_streamed(data, W, H, K, ring=8)   # a correct call on the same context still succeeds
        if ok is None:
            ok = got
        for b in range(2):
            _assert_same(got[b], ok[b], f"after {kw}: sequence {b}")

    expect((-2,), ring=5)                         # < init_frames + 1
    expect((-2, -3), ring=8, first_slot=[0, 4])   # overlapping rings
    expect((-3,), ring=8, first_slot=[0, 9])      # past n_slots
    expect((-3,), ring=8, first_slot=[-1, 8])
    ctx.frames_stream_begin(0, data[0][0][:4])
    try:
        with pytest.raises(pmv.PmvError) as e:
            ctx.pipeline_run_batch_streamed(data, W, H, K, ring=8)
        assert e.value.code == -2
    finally:
        ctx.frames_stream_end()
    got = ctx.pipeline_run_batch_streamed(data, W, H, K, ring=8)
    for b in range(2):
        _assert_same(got[b], ok[b], f"after an open stream bracket: sequence {b}")
    # and against the staged batch
    staged_ctx = gpu_ctx_factory(W, H, n_slots=26, max_tracks=4096)
    ref = _staged(staged_ctx, data)
    for b in range(2):
        _assert_same(ok[b], ref[b], f"sequence {b} vs staged")
