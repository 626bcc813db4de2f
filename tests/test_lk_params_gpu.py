"""Lucas-Kanade with caller-chosen window, pyramid depth and stop criteria (pmv_set_lk_params): every accepted setting against the CPU
restatement (oracle/orc_lk.cpp), bit for bit; the general kernels against the tuned ones at the default window; the batched, session and
pipeline routes under a non-default setting; the setter's contract."""
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZES = [(160, 120), (203, 87)]            # the second: odd sizes, upper levels narrower than the 64-pixel border
WINDOWS = [3, 5, 15, 21, 31, 32, 33, 48, 63]
LEVELS_160x120 = {(3, 4): 4, (5, 4): 4, (15, 4): 2, (21, 4): 2, (31, 4): 1, (32, 4): 1, (33, 4): 1, (48, 4): 1, (63, 4): 0, (21, 0): 0, (21, 1): 1, (21, 3): 2}
MIN_TRACKED = 60                            # of the 320 points, by the oracle: the comparison where status = 1 must not be empty
K00 = dict(w=1241, h=376, fx=718.856, fy=718.856, cx=607.1928, cy=185.2157)
_cache = {}


def _pair(pmv, w, h):
    """two consecutive synthetic frames and 320 points: 160 anywhere within 70 pixels of the frame (outside, on the border, within a
    window of it) and 160 well inside"""
    if (w, h) not in _cache:
        fr, _ = pmv.synth_sequence(1007, 10, 2, w, h, 0.58 * w, 0.58 * w, w / 2, h / 2)
        rng = np.random.default_rng(5)
        wide = np.stack([rng.uniform(-70, w + 70, 160), rng.uniform(-70, h + 70, 160)], axis=1)
        inside = np.stack([rng.uniform(8, w - 8, 160), rng.uniform(8, h - 8, 160)], axis=1)
        _cache[(w, h)] = (fr[0], fr[1], np.concatenate([wide, inside]).astype(np.float32))
    return _cache[(w, h)]


def _oracle(pmv, orc, w, h, **kw):
    key = (w, h, tuple(sorted(kw.items())))
    if key not in _cache:
        a, b, pts = _pair(pmv, w, h)
        _cache[key] = orc.lk_track(a, b, pts, **kw)
    return _cache[key]


def _ctx(pmv, gpu_ctx_factory, name="main"):
    """one context of 256x128 capacity with four slots for all the small cases"""
    if name not in _cache:
        _cache[name] = gpu_ctx_factory(256, 128, n_slots=4, max_tracks=1024)
    return _cache[name]


def _upload_pair(pmv, ctx, w, h, first=0):
    a, b, pts = _pair(pmv, w, h)
    ctx.frame_upload(first, a)
    ctx.frame_upload(first + 1, b)
    return a, b, pts


def _same_where_tracked(got, want, what):
    (xy, st, err), (rxy, rst, rerr) = got, want[:3]
    tracked = int(rst.sum())
    print(f"{what}: {tracked} of {len(rst)} tracked by the oracle")
    assert tracked >= MIN_TRACKED, f"{what}: the oracle tracks only {tracked} points"
    assert np.array_equal(st, rst), f"{what}: status differs at {np.flatnonzero(st != rst)[:8]}"
    ok = rst > 0
    assert np.array_equal(xy[ok].view(np.uint32), rxy[ok].view(np.uint32)), f"{what}: positions differ at {np.flatnonzero((xy != rxy).any(axis=1) & ok)[:8]}"
    assert np.array_equal(err[ok].view(np.uint32), rerr[ok].view(np.uint32)), f"{what}: err differs at {np.flatnonzero((err != rerr) & ok)[:8]}"


CASES = [(w, 4) for w in WINDOWS] + [(21, m) for m in (0, 1, 3)]


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("win, max_level", CASES)
def test_window_and_depth_match_the_oracle(pmv, orc, gpu_ctx_factory, size, win, max_level):
    """1. status identical, xy and err bit-exact, the level count that of orc::build_pyramid, every level that of repeated orc.pyr_down"""
    w, h = size
    ctx = _ctx(pmv, gpu_ctx_factory)
    ctx.set_lk_params(win=win, max_level=max_level)
    a, b, pts = _upload_pair(pmv, ctx, w, h)
    want = _oracle(pmv, orc, w, h, win=win, max_level=max_level)
    levels = want[3]
    if size == (160, 120):
        assert levels == LEVELS_160x120[(win, max_level)]
    assert ctx.num_levels(0) == levels and ctx.num_levels(1) == levels
    for slot, img in ((0, a), (1, b)):
        ref = img
        for lv in range(levels + 1):
            if lv:
                ref = orc.pyr_down(ref)
            assert np.array_equal(ctx.get_level(slot, lv, w, h), ref), f"slot {slot}: level {lv} ({ref.shape[1]}x{ref.shape[0]}) differs"
            # the REFLECT_101 frame around it, reflected as often as the level is narrow
            assert np.array_equal(ctx.get_level_padded(slot, lv, w, h), np.pad(ref, 64, mode="reflect")), f"slot {slot}: border of level {lv}"
    _same_where_tracked(ctx.lk_track(0, 1, pts), want, f"{w}x{h} win {win} maxLevel {max_level}")


STOP = [dict(max_iter=1), dict(max_iter=3), dict(max_iter=100), dict(eps=0.0), dict(eps=0.3), dict(eps=10.0), dict(min_eig=0.0), dict(min_eig=1e-2)]


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("kw", STOP, ids=lambda k: "-".join(f"{a}={b}" for a, b in k.items()))
def test_stop_criteria_match_the_oracle(pmv, orc, gpu_ctx_factory, size, kw):
    """2. one field at a time at win 21, maxLevel 3; the oracle itself must tell the setting from (30, 0.01, 1e-4), so a kernel that
    ignores the field fails"""
    w, h = size
    base = _oracle(pmv, orc, w, h, win=21, max_level=3)
    want = _oracle(pmv, orc, w, h, win=21, max_level=3, **kw)
    both = (base[1] > 0) & (want[1] > 0)
    assert not np.array_equal(base[1], want[1]) or not np.array_equal(base[0][both], want[0][both]), f"{kw}: the oracle gives the default result"
    ctx = _ctx(pmv, gpu_ctx_factory)
    ctx.set_lk_params(win=21, max_level=3, **kw)
    _, _, pts = _upload_pair(pmv, ctx, w, h)
    _same_where_tracked(ctx.lk_track(0, 1, pts), want, f"{w}x{h} {kw}")


def _threads(n, fn):
    res, errors = [None] * n, []
    start = threading.Barrier(n)

    def run(j):
        try:
            start.wait()
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


def _bytes(r):
    return [np.asarray(x).tobytes() for x in r]


def test_general_and_tuned_kernels_agree_at_the_default_window(pmv, gpu_ctx_factory):
    """3. 320x200, about 300 detected corners, default parameters: pmv_debug_lk_general on and off give the same bytes, from lk_track and
    from batch_lk_track called by three threads"""
    w, h = 320, 200
    fr, _ = pmv.synth_sequence(1007, 10, 2, w, h, 0.58 * w, 0.58 * w, w / 2, h / 2)
    ctx = gpu_ctx_factory(w, h, n_slots=2, max_tracks=1024)
    ctx.frame_upload(0, fr[0])
    ctx.frame_upload(1, fr[1])
    cells = pmv.grid_cells(w, h)
    pts = np.concatenate([d + c[:2] for c, d in zip(cells, ctx.detect_gftt(0, cells, 150))]).astype(np.float32)
    print(len(pts), "corners")
    assert 200 <= len(pts) <= 400
    parts = [pts[j::3] for j in range(3)]
    got = {}
    for on in (0, 1):
        ctx.debug_lk_general(on)
        got[on, "single"] = ctx.lk_track(0, 1, pts)
        with ctx.batch_session(1, [(w, h)]):
            got[on, "batch"] = _threads(3, lambda j: ctx.batch_lk_track(0, 1, parts[j]))
    ctx.debug_lk_general(0)
    assert int(got[0, "single"][1].sum()) > 0.6 * len(pts)
    assert _bytes(got[0, "single"]) == _bytes(got[1, "single"]), "lk_track: the general kernel differs from the tuned one"
    for j in range(3):
        assert _bytes(got[0, "batch"][j]) == _bytes(got[1, "batch"][j]), f"batch_lk_track, thread {j}: the general kernel differs from the tuned one"


def test_batched_session_form_under_other_parameters(pmv, orc, gpu_ctx_factory):
    """4. (21, 3): batch_lk_track from three threads on slots of both sizes, declared together, equals lk_track on the same slots; one LK
    launch per round whatever the sizes"""
    ctx = _ctx(pmv, gpu_ctx_factory)
    ctx.set_lk_params(win=21, max_level=3)
    pts = {}
    for k, (w, h) in enumerate(SIZES):
        pts[k] = _upload_pair(pmv, ctx, w, h, first=2 * k)[2]
    want = [ctx.lk_track(2 * k, 2 * k + 1, pts[k]) for k in range(2)]
    for k, (w, h) in enumerate(SIZES):
        _same_where_tracked(want[k], _oracle(pmv, orc, w, h, win=21, max_level=3), f"slots {2 * k}, {2 * k + 1}")
    l0, s0 = ctx.batch_launches()["k_lk_batch"], ctx.batch_stats()["lk"]["launches"]
    with ctx.batch_session(1, SIZES):
        got = _threads(3, lambda j: [ctx.batch_lk_track(2 * (k % 2), 2 * (k % 2) + 1, pts[k % 2]) for k in range(j, j + 4)])
    launches, rounds = ctx.batch_launches()["k_lk_batch"] - l0, ctx.batch_stats()["lk"]["launches"] - s0
    print("LK launches", launches, "rounds", rounds, "requests 12")
    assert 0 < launches <= rounds <= 12
    for j in range(3):
        for i, k in enumerate(range(j, j + 4)):
            assert _bytes(got[j][i]) == _bytes(want[k % 2]), f"thread {j}, request {i}: batch_lk_track differs from lk_track"


def _assert_same(a, b, what):
    assert np.array_equal(a.poses, b.poses), f"{what}: poses differ"
    assert len(a.features) == len(b.features)
    for k, (x, y) in enumerate(zip(a.features, b.features)):
        assert np.array_equal(x, y), f"{what}: features of frame {k} differ"
    for key in ("lk_calls", "lk_points", "detect_calls", "pnp_calls", "pnp_points", "tri_calls", "ba_calls", "ba_obs", "ba_points", "init_offset"):
        assert a.stats[key] == b.stats[key], (what, key)


def test_pipelines_under_other_parameters(pmv, gpu_ctx_factory):
    """5. (21, 3) on the metric configuration: the four pipeline entry points give identical poses, features and counters, and the features
    differ from the default-parameter run of the same sequence (the setting reaches the LK plugin)"""
    cfg = K00
    lengths, seeds = [26, 30, 34], [1006, 1005, 1008]
    K = np.array([cfg["fx"], 0, cfg["cx"], 0, cfg["fy"], cfg["cy"], 0, 0, 1.0])
    data = [pmv.synth_sequence(seed, 0, n, cfg["w"], cfg["h"], cfg["fx"], cfg["fy"], cfg["cx"], cfg["cy"], nthreads=16) for n, seed in zip(lengths, seeds)]
    single = gpu_ctx_factory(cfg["w"], cfg["h"], n_slots=max(lengths), max_tracks=4096)
    single.frames_stage(0, data[0][0])
    default = single.pipeline_run(lengths[0], cfg["w"], cfg["h"], K, data[0][1], threaded=1)
    single.set_lk_params(win=21, max_level=3)
    ref = []
    for (frames, gt), n in zip(data, lengths):
        single.frames_stage(0, frames)
        ref.append(single.pipeline_run(n, cfg["w"], cfg["h"], K, gt, threaded=1))
        assert single.num_levels(0) == 3
    assert any(not np.array_equal(x, y) for x, y in zip(default.features, ref[0].features)), "the (21, 3) run has the default run's features"
    _assert_same(single.pipeline_run(lengths[0], cfg["w"], cfg["h"], K, data[0][1], threaded=1, host_frames=data[0][0]), ref[0], "pipeline_run_streamed")
    ctx = gpu_ctx_factory(cfg["w"], cfg["h"], n_slots=sum(lengths), max_tracks=4096)
    ctx.set_lk_params(win=21, max_level=3)
    seqs, first = [], 0
    for (frames, gt), n in zip(data, lengths):
        ctx.frames_stage(first, frames)
        seqs.append((first, n, gt))
        first += n
    for b, r in enumerate(ctx.pipeline_run_batch(seqs, cfg["w"], cfg["h"], K)):
        _assert_same(r, ref[b], f"pipeline_run_batch, sequence {b}")
    for b, r in enumerate(ctx.pipeline_run_batch_streamed(data, K=K, ring=8)):
        _assert_same(r, ref[b], f"pipeline_run_batch_streamed, sequence {b}")


DEFAULTS = dict(win=32, max_level=4, max_iter=30, eps=0.01, min_eig=1e-4)


def test_contract(pmv, gpu_ctx_factory):
    """6. ranges, refusals, the effect on the slots, and the defaults set explicitly"""
    w, h = SIZES[0]
    a, b, pts = _pair(pmv, w, h)
    fresh = gpu_ctx_factory(256, 128, n_slots=2, max_tracks=1024)
    fresh.frame_upload(0, a)
    fresh.frame_upload(1, b)
    never = fresh.lk_track(0, 1, pts)
    ctx = gpu_ctx_factory(256, 128, n_slots=2, max_tracks=1024)
    got = ctx.lk_params()
    assert got == dict(DEFAULTS, min_eig=float(np.float32(1e-4)))
    ctx.set_lk_params()
    ctx.frame_upload(0, a)
    ctx.frame_upload(1, b)
    assert _bytes(ctx.lk_track(0, 1, pts)) == _bytes(never), "set_lk_params() with the defaults changes the result"
    ctx.set_lk_params(win=21, max_level=3, max_iter=20, eps=0.03, min_eig=1e-3)
    held = ctx.lk_params()
    for bad in (dict(win=2), dict(win=64), dict(win=-21), dict(max_level=-1), dict(max_level=5), dict(max_iter=0), dict(max_iter=101), dict(eps=-1e-9), dict(eps=10.5),
                dict(eps=float("nan")), dict(min_eig=-1e-6), dict(min_eig=float("inf")), dict(min_eig=float("nan"))):
        with pytest.raises(pmv.PmvError) as e:
            ctx.set_lk_params(**dict(held, **bad))
        assert e.value.code == -2, bad
        assert ctx.lk_params() == held, f"{bad}: a refused call changed the setting"
    # a change of win empties the slots; a change of eps alone does not
    ctx.frame_upload(0, a)
    ctx.frame_upload(1, b)
    ctx.set_lk_params(**dict(held, eps=0.02))
    ctx.lk_track(0, 1, pts)
    ctx.set_lk_params(**dict(held, eps=0.02, win=15))
    with pytest.raises(pmv.PmvError) as e:
        ctx.lk_track(0, 1, pts)
    assert e.value.code == -2
    assert ctx.num_levels(0) < 0
    ctx.frame_upload(0, a)
    ctx.frame_upload(1, b)
    assert int(ctx.lk_track(0, 1, pts)[1].sum()) >= MIN_TRACKED
    # refused inside a stream bracket and inside an open session
    held = ctx.lk_params()
    frames = np.stack([a, b])
    ctx.frames_stream_begin(0, frames)
    try:
        with pytest.raises(pmv.PmvError) as e:
            ctx.set_lk_params(win=21)
        assert e.value.code == -2
    finally:
        ctx.frames_stream_end()
    with ctx.batch_session(1, [(w, h)]):
        with pytest.raises(pmv.PmvError) as e:
            ctx.set_lk_params(win=21)
        assert e.value.code == -2
    assert ctx.lk_params() == held
    assert int(ctx.lk_track(0, 1, pts)[1].sum()) >= MIN_TRACKED   # the bracket rebuilt the slots under the setting that stayed
