"""The reference's alternative plugins through the batch engine: OpenCVFASTFeatureExtractor (extractor = 2) and kNNFeatureMatcher over it
(matcher = 1) on pmv_pipeline_run_batch / pmv_pipeline_run_batch_streamed. Every sequence of a batch - also one whose neighbours run
other plugin pairs - must give exactly the bits of its own pmv_pipeline_run, and the feature coordinates of the oracle pipeline; the
batched kNN kernel body (shared with pmv_knn_match) is pinned where its whole-wavefront window sum must fall back to the reference's
summation order."""
import numpy as np
import pytest

import orc_binding as ob

pytestmark = pytest.mark.gpu

K00 = dict(w=1241, h=376, fx=718.856, fy=718.856, cx=607.1928, cy=185.2157)
K = np.array([K00["fx"], 0, K00["cx"], 0, K00["fy"], K00["cy"], 0, 0, 1.0])
W, H = K00["w"], K00["h"]
LENGTHS = [40, 33, 45, 30, 36, 40]
SEEDS = [1000, 1001, 1002, 1003, 1004, 1005]
STAT_KEYS = ("lk_calls", "lk_points", "detect_calls", "pnp_calls", "pnp_points", "tri_calls", "ba_calls", "ba_obs", "ba_points", "init_offset")

_data = {}


def _sequences(pmv):
    if not _data:
        _data["seqs"] = [pmv.synth_sequence(s, 0, n, W, H, K00["fx"], K00["fy"], K00["cx"], K00["cy"], nthreads=16) for n, s in zip(LENGTHS, SEEDS)]
    return _data["seqs"]


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


def _single_runs(gpu_ctx_factory, data, pairs):
    """every sequence's own pmv_pipeline_run (two host threads, as the sequences of a batch)"""
    ctx = _data.get("single")
    if ctx is None:
        ctx = _data["single"] = gpu_ctx_factory(W, H, n_slots=max(LENGTHS), max_tracks=4096)
    out = []
    for (frames, gt), (ex, ma) in zip(data, pairs):
        key = (id(frames), ex, ma)
        if key not in _data:
            ctx.frames_stage(0, frames)
            _data[key] = ctx.pipeline_run(len(frames), W, H, K, gt, threaded=1, extractor=ex, matcher=ma)
        out.append(_data[key])
    return out


def _assert_oracle_features(res, frames, gt, ex, ma, what):
    o = ob.run_pipeline(frames, K, gt, n_threads=8, extractor=ex, matcher=ma)
    assert len(res.features) == len(o.features), what
    for k, (a, b) in enumerate(zip(res.features, o.features)):
        assert np.array_equal(a[:, :2], b[:, :2]), f"{what}: feature coordinates of frame {k} differ from the oracle pipeline"


@pytest.fixture(scope="module")
def batch_ctx(gpu_ctx_factory):
    return gpu_ctx_factory(W, H, n_slots=sum(LENGTHS), max_tracks=4096)


def test_fast_extractor_batch_equals_single_runs_and_oracle(pmv, gpu_ctx_factory, batch_ctx):
    """FAST + LK (extractor = 2): six sequences in one staged batch"""
    data = _sequences(pmv)
    seqs = _stage(batch_ctx, data)
    got = batch_ctx.pipeline_run_batch(seqs, W, H, K, extractor=2)
    ref = _single_runs(gpu_ctx_factory, data, [(2, 0)] * 6)
    for b, (frames, gt) in enumerate(data):
        _assert_same(got[b], ref[b], f"FAST + LK, sequence {b}")
        assert len(got[b].poses) > 20
        _assert_oracle_features(got[b], frames, gt, 2, 0, f"FAST + LK, sequence {b}")


def test_knn_matcher_batch_equals_single_runs_and_oracle(pmv, gpu_ctx_factory, batch_ctx):
    """kNN over FAST (extractor = 2, matcher = 1): the kNN requests of a round share one k_knn_round launch, the whole-frame FAST
    requests one detector launch"""
    data = _sequences(pmv)
    seqs = _stage(batch_ctx, data)
    s0 = batch_ctx.batch_stats()
    got = batch_ctx.pipeline_run_batch(seqs, W, H, K, extractor=2, matcher=1)
    s1 = batch_ctx.batch_stats()
    for role in ("lk", "det"):
        req, launches = s1[role]["requests"] - s0[role]["requests"], s1[role]["launches"] - s0[role]["launches"]
        print(f"{role}: {req} requests in {launches} rounds")
        assert req > launches > 0, f"{role}: nothing was merged into a shared launch"
    ref = _single_runs(gpu_ctx_factory, data, [(2, 1)] * 6)
    nmax = 0
    for b, (frames, gt) in enumerate(data):
        _assert_same(got[b], ref[b], f"kNN over FAST, sequence {b}")
        assert len(got[b].poses) > 0
        nmax = max(nmax, max(len(f) for f in got[b].features))
        _assert_oracle_features(got[b], frames, gt, 2, 1, f"kNN over FAST, sequence {b}")
    print("largest feature count of a frame:", nmax)


def test_mixed_plugin_pairs_share_a_batch(pmv, gpu_ctx_factory, batch_ctx):
    data = _sequences(pmv)
    pairs = [(0, 0), (1, 0), (2, 0), (2, 1), (2, 1), (0, 0)]
    seqs = _stage(batch_ctx, data)
    ex, ma = [p[0] for p in pairs], [p[1] for p in pairs]
    got = batch_ctx.pipeline_run_batch(seqs, W, H, K, extractor=ex, matcher=ma)
    ref = _single_runs(gpu_ctx_factory, data, pairs)
    for b in range(6):
        _assert_same(got[b], ref[b], f"mixed batch, sequence {b} {pairs[b]}")
    # the same engine again: three of them in another order (other engine slots, other neighbours)
    order = (4, 0, 2)
    again = batch_ctx.pipeline_run_batch([seqs[b] for b in order], W, H, K, extractor=[ex[b] for b in order], matcher=[ma[b] for b in order])
    for r, b in zip(again, order):
        _assert_same(r, got[b], f"re-run of sequence {b}")
    # an engine that has served the new request kinds serves the default ones as before
    plain = batch_ctx.pipeline_run_batch([seqs[0], seqs[5]], W, H, K)
    _assert_same(plain[0], got[0], "default plugins after the alternative ones, sequence 0")
    _assert_same(plain[1], got[5], "default plugins after the alternative ones, sequence 5")


@pytest.mark.parametrize("fmt", ["gray", "bgr"])
def test_streamed_batch_with_alternative_plugins_equals_staged(pmv, gpu_ctx_factory, batch_ctx, fmt):
    """pairs (2,0) and (2,1) from pageable host memory through rings shorter than every sequence"""
    data = _sequences(pmv)[:4]
    pairs = [(2, 0), (2, 1), (2, 1), (2, 0)]
    ex, ma = [p[0] for p in pairs], [p[1] for p in pairs]
    seqs = _stage(batch_ctx, data)
    want = batch_ctx.pipeline_run_batch(seqs, W, H, K, extractor=ex, matcher=ma)
    if fmt == "bgr":   # gray in all three channels: BGR2GRAY ((B 1868 + G 9617 + R 4899 + 8192) >> 14, weights summing to 2^14) gives the gray frame back
        src = [(np.ascontiguousarray(np.repeat(f[..., None], 3, axis=3)), gt) for f, gt in data]
    else:
        src = [(f.copy(), gt) for f, gt in data]
    ctx = gpu_ctx_factory(W, H, n_slots=4 * 16, max_tracks=4096)
    ctx.set_frame_format(fmt)
    for ring in (6, 16):
        assert all(len(f) > ring for f, _ in src)
        got = ctx.pipeline_run_batch_streamed(src, W, H, K, ring=ring, extractor=ex, matcher=ma)
        for b in range(4):
            _assert_same(got[b], want[b], f"{fmt}, ring {ring}, sequence {b} {pairs[b]}")


def test_plugin_pairs_the_single_run_refuses_are_refused_by_name(pmv, gpu_ctx_factory, batch_ctx):
    data = _sequences(pmv)[:2]
    seqs = _stage(batch_ctx, data)
    before = batch_ctx.pipeline_run_batch(seqs, W, H, K, extractor=[2, 2], matcher=[0, 1])
    for kw, words in ((dict(matcher=1, extractor=0), ("matcher = 1", "extractor = 2")), (dict(matcher=[0, 1], extractor=[2, 1]), ("matcher = 1", "extractor = 2")),
                      (dict(extractor=3), ("extractor = 3", "FAST")), (dict(matcher=2, extractor=2), ("matcher = 2", "kNN"))):
        with pytest.raises(pmv.PmvError) as e:
            batch_ctx.pipeline_run_batch(seqs, W, H, K, **kw)
        assert e.value.code == -2, (kw, e.value.code)
        for word in words:
            assert word in str(e.value), (kw, str(e.value))
        with pytest.raises(pmv.PmvError) as e:
            batch_ctx.pipeline_run_batch_streamed([(f, gt) for f, gt in data], W, H, K, ring=8, first_slot=[0, 8], **kw)
        assert e.value.code == -2 and words[0] in str(e.value), (kw, str(e.value))
    after = batch_ctx.pipeline_run_batch(seqs, W, H, K, extractor=[2, 2], matcher=[0, 1])
    for b in range(2):
        _assert_same(after[b], before[b], f"after the refusals, sequence {b}")


def test_knn_window_error_is_exact_where_the_integer_sum_is_not(pmv, orc, gpu_ctx_factory):
    """compareFeatures accumulates a float through double additions, x outer / y inner. All terms are integers, so a window whose total
    stays <= 2^24 may be summed in any order; a larger one (frame A all 0 against B near 255: 289 pixel pairs, total 18 767 793) rounds
    on the way and must be summed in the reference's order: 19.254125595 there, 19.254137039 for an order-free integer sum. Border
    windows (fewer pairs, totals below 2^24) stay exact either way. Best indices and errors bit-exact against the oracle."""
    a = np.zeros((H, W), np.uint8)
    b = np.full((H, W), 255, np.uint8)
    b[::3, ::2] = 254
    ctx = gpu_ctx_factory(W, H, n_slots=4, max_tracks=2048)
    ctx.frame_upload(0, a); ctx.frame_upload(1, b)
    src = np.array([[600, 180], [20, 20], [0, 0], [1240, 375], [3, 374], [8, 8], [1232, 367], [300, 7]], np.int32)
    rng = np.random.default_rng(11)
    big = np.unique(np.stack([rng.integers(0, W, 1000), rng.integers(0, H, 1000)], 1), axis=0).astype(np.int32)
    rng.shuffle(big)
    sets = [big, big[:5].copy(), np.zeros((0, 2), np.int32)]
    for cmp_xy in sets:
        gb, ge = ctx.knn_match(0, 1, src, cmp_xy)
        ob_, oe = orc.knn_match(a, b, src, cmp_xy)
        assert np.array_equal(gb, ob_) and np.array_equal(ge, oe), len(cmp_xy)
    gb, ge = ctx.knn_match(0, 1, src[:1], np.array([[601, 182]], np.int32))
    ob_, oe = orc.knn_match(a, b, src[:1], np.array([[601, 182]], np.int32))
    assert np.array_equal(gb, ob_) and np.array_equal(ge, oe)
    # the window of 289 pairs sums to 18 767 793 > 2^24: the float of the reference's order, not of the integer total
    total = sum((255 - (1 if (182 + y) % 3 == 0 and (601 + x) % 2 == 0 else 0)) ** 2 for x in range(-8, 9) for y in range(-8, 9))
    assert total == 18767793 and total > 2 ** 24
    assert ge[0] != np.float32(np.sqrt(np.float64(np.float32(total))) / 225.0), "an order-free sum was reported for a window above 2^24"
    assert abs(float(ge[0]) - 19.254125595) < 1e-6
    # a textured frame pair: every total is small
    fr, _ = pmv.synth_sequence(1003, 0, 2, W, H, K00["fx"], K00["fy"], K00["cx"], K00["cy"], nthreads=16)
    ctx.frame_upload(2, fr[0]); ctx.frame_upload(3, fr[1])
    cells = pmv.grid_cells(W, H)
    tex = np.concatenate([orc.gftt_cell(fr[0], c, 40) + c[:2] for c in cells]).astype(np.int32)
    gb, ge = ctx.knn_match(2, 3, tex, big)
    ob_, oe = orc.knn_match(fr[0], fr[1], tex, big)
    assert np.array_equal(gb, ob_) and np.array_equal(ge, oe)
