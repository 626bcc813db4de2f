"""Batch sessions (include/pmv_hip.h, pmv_batch_*): plugin-level callers reach the batch engine - uploads merged into rounds by the upload
class (pitched level-0 kernels reading strided sources in place), the nine plugin calls served by the combiners - and every call returns
exactly the bits of the single-sequence call of the same name.

Inputs: synth_sequence(seed, 0, 6, w, h, 0.58 w, 0.58 w, w / 2, h / 2) at 640x200 (seed 1007), 333x121 (seed 1008: odd sizes, levels 0-1
only) and 1241x376 (seed 1000: levels 0-3). The CPU oracle finds 20 GFTT corners in every grid cell of frame 0 (60 / 40 / 200 corners) and
tracks 54 / 35 / 124 of them over three frames with truncation, so every comparison also asserts that it is not vacuous: every cell
returns its 20 corners and at least half of them are still tracked after three frames."""
import ctypes as C
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZES = [(640, 200, 1007), (333, 121, 1008), (1241, 376, 1000)]
CAP_W, CAP_H = 1241, 376
LEVELS_ABOVE_0 = {(640, 200): 2, (333, 121): 1, (1241, 376): 3}   # cv::buildOpticalFlowPyramid(winSize 32, maxLevel 4) stops at <= 32
N_FRAMES = 6

_cache = {}


def _frames(pmv, w, h, seed):
    key = ("frames", w, h)
    if key not in _cache:
        _cache[key] = pmv.synth_sequence(seed, 0, N_FRAMES, w, h, 0.58 * w, 0.58 * w, w / 2, h / 2, nthreads=8)[0]
    return _cache[key]


def _bgr(gray):
    """a colour frame whose three channels differ (so that a wrong channel order or a wrong pitch cannot cancel out)"""
    return np.ascontiguousarray(np.stack([gray, np.roll(gray, 3, axis=1), np.roll(gray, 2, axis=0)], axis=2))


def _roi(img):
    """`img` as an ROI view at column offset 3, row offset 2 inside an image 7 pixels wider and 4 rows taller: an odd pitch and a base that
    is not dword aligned (BGR: pitch 3 W, neither 3 w nor a multiple of 4). The surroundings are noise."""
    h, w = img.shape[:2]
    big = np.random.default_rng(w * 31 + h).integers(0, 256, (h + 4, w + 7) + img.shape[2:], dtype=np.uint8)
    big[2:2 + h, 3:3 + w] = img
    return big


def _ctxs(gpu_ctx_factory):
    """the session context (36 frame slots) and the context of the single-sequence calls"""
    if "ctxs" not in _cache:
        _cache["ctxs"] = (gpu_ctx_factory(CAP_W, CAP_H, n_slots=36, max_tracks=1024), gpu_ctx_factory(CAP_W, CAP_H, n_slots=4, max_tracks=1024))
    return _cache["ctxs"]


def _levels(ctx, slot):
    return [ctx.get_level_padded(slot, l, CAP_W, CAP_H) for l in range(ctx.num_levels(slot) + 1)]


def _ref_levels(pmv, ref, w, h, seed, fmt, k):
    """every padded level of frame k through pmv_frame_upload / pmv_frame_upload_bgr, computed once"""
    key = ("ref", w, h, fmt, k)
    if key not in _cache:
        g = _frames(pmv, w, h, seed)[k]
        if fmt == "bgr":
            ref.frame_upload_bgr(0, _bgr(g))
        else:
            ref.frame_upload(0, g)
        _cache[key] = _levels(ref, 0)
        assert len(_cache[key]) == 1 + LEVELS_ABOVE_0[(w, h)]
    return _cache[key]


def _same_levels(got, want, what):
    assert len(got) == len(want), f"{what}: {len(got)} levels, expected {len(want)}"
    for l, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape and np.array_equal(a, b), f"{what}: level {l} differs"


def test_uploads_from_every_kind_of_source_equal_the_single_upload(pmv, gpu_ctx_factory):
    """each size, both formats; a tight pageable array, an ROI view of a larger pageable image, the same view in pinned memory and in device
    memory (both read in place through the pitched kernels): every padded level byte-equal to pmv_frame_upload[_bgr]. One upload at a time,
    so every round holds one frame: rounds = frames = level-0 launches, and the pyrDown launches are the sum of the frames' levels above 0."""
    import torch
    ctx, ref = _ctxs(gpu_ctx_factory)
    with ctx.batch_session(6, [(w, h) for w, h, _ in SIZES]):
        n = pyr = 0
        for w, h, seed in SIZES:
            for fmt in ("gray", "bgr"):
                img = _frames(pmv, w, h, seed)[1] if fmt == "gray" else _bgr(_frames(pmv, w, h, seed)[1])
                want = _ref_levels(pmv, ref, w, h, seed, fmt, 1)
                big = _roi(img)
                pinned = torch.empty(big.shape, dtype=torch.uint8).pin_memory()
                pinned.numpy()[...] = big
                dev = torch.from_numpy(big).to("cuda:0")
                sources = {"tight pageable": img, "ROI view": big[2:2 + h, 3:3 + w], "pinned ROI view": pinned[2:2 + h, 3:3 + w],
                           "device ROI view": dev[2:2 + h, 3:3 + w]}
                assert not sources["ROI view"].flags["C_CONTIGUOUS"] and sources["ROI view"].ctypes.data % 4 != 0
                for slot, (name, src) in enumerate(sources.items()):
                    ctx.batch_frame_upload(slot, src, fmt)
                    _same_levels(_levels(ctx, slot), want, f"{w}x{h} {fmt} from a {name}")
                    n += 1
                    pyr += LEVELS_ABOVE_0[(w, h)]
        st = ctx.batch_upload_stats()
        assert st == dict(rounds=n, frames=n, level0_launches=n, pyrdown_launches=pyr), st
        # the pinned and the device source were read where they are, the two pageable ones came through the staging pool
        assert [r["in_place"] for r in ctx.batch_upload_rounds()] == [0, 0, 1, 1] * (n // 4)


def test_one_row_per_workgroup_bgr_form(pmv, gpu_ctx_factory):
    """a 4200x40 BGR frame is too wide for four rows of LDS: the one-row instantiation of the pitched BGR kernel, tight and as an ROI view in
    device memory"""
    import torch
    w, h = 4200, 40
    ctx = gpu_ctx_factory(w, h, n_slots=3, max_tracks=64)
    img = np.random.default_rng(5).integers(0, 256, (h, w, 3), dtype=np.uint8)
    ctx.frame_upload_bgr(2, img)
    want = [ctx.get_level_padded(2, 0, w, h)]
    assert ctx.num_levels(2) == 0
    dev = torch.from_numpy(_roi(img)).to("cuda:0")
    with ctx.batch_session(1, [(w, h)]):
        ctx.batch_frame_upload(0, img, "bgr")
        ctx.batch_frame_upload(1, dev[2:2 + h, 3:3 + w], "bgr")
        for slot in (0, 1):
            assert ctx.num_levels(slot) == 0
            _same_levels([ctx.get_level_padded(slot, 0, w, h)], want, f"4200x40 BGR, slot {slot}")
        assert ctx.batch_upload_stats() == dict(rounds=2, frames=2, level0_launches=2, pyrdown_launches=0)


def test_six_threads_upload_six_sequences_at_once(pmv, gpu_ctx_factory):
    """six threads, two per size (one uploads gray frames from tight arrays, the other BGR frames from ROI views), six frames each into slots
    of their own: the same bytes as the single uploads. From the counters: 36 frames; level-0 launches <= 2 x rounds (one gray and one BGR
    launch per round at most, whatever its sizes); pyrDown launches = sum over the rounds of the levels above 0 of the round's tallest
    pyramid. Which frames met in a round is timing; the library's per-round record (pmv_batch_upload_rounds: the round's frames by pyramid
    height, and the launches it made, counted where they are made) tells it afterwards, so the equality is asserted round by round."""
    ctx, ref = _ctxs(gpu_ctx_factory)
    jobs = []   # (w, h, seed, fmt, first slot)
    for i, (w, h, seed) in enumerate(SIZES):
        jobs += [(w, h, seed, "gray", 12 * i), (w, h, seed, "bgr", 12 * i + 6)]
    srcs = []
    for w, h, seed, fmt, _ in jobs:
        f = _frames(pmv, w, h, seed)
        srcs.append([f[k] for k in range(N_FRAMES)] if fmt == "gray" else [_roi(_bgr(f[k]))[2:2 + h, 3:3 + w] for k in range(N_FRAMES)])
    with ctx.batch_session(6, [(w, h) for w, h, _ in SIZES]):
        start = threading.Barrier(len(jobs))

        def run(j):
            start.wait()
            for k in range(N_FRAMES):
                ctx.batch_frame_upload(jobs[j][4] + k, srcs[j][k], jobs[j][3])
        _threads(len(jobs), run)
        st = ctx.batch_upload_stats()
        rounds = ctx.batch_upload_rounds()
        for w, h, seed, fmt, first in jobs:
            for k in range(N_FRAMES):
                _same_levels(_levels(ctx, first + k), _ref_levels(pmv, ref, w, h, seed, fmt, k), f"{w}x{h} {fmt} frame {k}")
    print(f"36 uploads from six threads: {st}; frames per round {[sum(r['frames_by_levels']) for r in rounds]}")
    assert st["frames"] == 36 and len(rounds) == st["rounds"]
    assert st["level0_launches"] <= 2 * st["rounds"]
    # every frame is in exactly one round: 12 frames each with 2 (333x121), 3 (640x200) and 4 (1241x376) levels, none read in place
    assert [sum(r["frames_by_levels"][i] for r in rounds) for i in range(5)] == [0, 12, 12, 12, 0]
    assert all(r["in_place"] == 0 for r in rounds)
    mixed = 0
    for r in rounds:
        tallest = max(i + 1 for i, c in enumerate(r["frames_by_levels"]) if c)
        assert r["pyrdown_launches"] == tallest - 1, r          # one launch per level above 0 of the round's tallest pyramid
        assert 1 <= r["level0_launches"] <= 2, r
        mixed += sum(1 for c in r["frames_by_levels"] if c) > 1
    assert st["pyrdown_launches"] == sum(r["pyrdown_launches"] for r in rounds) and st["level0_launches"] == sum(r["level0_launches"] for r in rounds)
    # not vacuous: uploads did meet, and at least one round held pyramids of different heights and still made one launch per level
    assert st["rounds"] < 36 and mixed >= 1, (st, rounds)


class _Api:
    """the front-end calls of one context, by their single-sequence names: through the session (batch_*) or directly"""

    def __init__(self, ctx, session):
        pre = "batch_" if session else ""
        for name in ("lk_track", "detect_gftt", "detect_shitomasi", "detect_fast", "knn_match"):
            setattr(self, name, getattr(ctx, pre + name))
        if session:
            self.upload = lambda slot, frame: ctx.batch_frame_upload(slot, frame, "gray")
        else:
            self.upload = ctx.frame_upload


def _chain_lk(pmv, api, frames, ring):
    """GFTT on frame 0, LK from k - 1 to k on the truncated survivors, once more GFTT on the middle frame without a limit: every array"""
    h, w = frames[0].shape
    cells = pmv.grid_cells(w, h)
    out = []
    pts = None
    for k in range(len(frames)):
        api.upload(ring[k % 3], frames[k])
        if k == 0:
            det = api.detect_gftt(ring[0], cells, 20)
            out += det
            pts = np.concatenate([d + c[:2] for c, d in zip(cells, det)]).astype(np.float32)
            continue
        xy, st, err = api.lk_track(ring[(k - 1) % 3], ring[k % 3], pts)
        out += [xy, st, err]
        pts = np.trunc(xy[st > 0])
        if k == len(frames) // 2:
            out += api.detect_gftt(ring[k % 3], cells, 0)
    return out


def _chain_alt(pmv, api, frames, ring):
    """ShiTomasi with scores on frame 0; FAST on every frame and the kNN matcher from the previous frame's keypoints to this frame's"""
    h, w = frames[0].shape
    cells = pmv.grid_cells(w, h)
    out = []
    prev = None
    for k in range(len(frames)):
        api.upload(ring[k % 3], frames[k])
        if k == 0:
            for xy, sc in api.detect_shitomasi(ring[0], cells, 20):
                out += [xy, sc]
        det = api.detect_fast(ring[k % 3], cells, 50, 20, True)
        for xy, rs in det:
            out += [xy, rs]
        cur = np.concatenate([xy + c[:2] for c, (xy, _) in zip(cells, det)]).astype(np.int32)
        if prev is not None:
            out += list(api.knn_match(ring[(k - 1) % 3], ring[k % 3], prev, cur))
        prev = cur
    return out


def _same_arrays(got, want, what):
    assert len(got) == len(want), f"{what}: {len(got)} arrays, expected {len(want)}"
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), f"{what}: array {i} differs"


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


def test_front_end_chain_from_six_threads_equals_the_single_calls(pmv, gpu_ctx_factory):
    """six Python threads, two per size, run their sequence through session calls only, each in a ring of 3 slots of its own; the same loop
    through frame_upload, lk_track and detect_gftt, sequentially on a second context, gives identical arrays at every step"""
    ctx, ref = _ctxs(gpu_ctx_factory)
    seqs = [s for s in SIZES for _ in range(2)]
    before = ctx.batch_stats()
    with ctx.batch_session(6, [(w, h) for w, h, _ in SIZES]):
        api = _Api(ctx, True)
        got = _threads(6, lambda j: _chain_lk(pmv, api, _frames(pmv, *seqs[j]), [3 * j, 3 * j + 1, 3 * j + 2]))
        up = ctx.batch_upload_stats()
    after = ctx.batch_stats()
    single = _Api(ref, False)
    for j, (w, h, seed) in enumerate(seqs):
        if j % 2 == 0:
            want = _chain_lk(pmv, single, _frames(pmv, w, h, seed), [0, 1, 2])
            n_cells = len(pmv.grid_cells(w, h))
            assert all(len(d) == 20 for d in want[:n_cells]), f"{w}x{h}: every cell returns its 20 corners"
            st3 = want[n_cells + 3 * 2 + 1]   # status of the third LK step
            assert 2 * int((st3 > 0).sum()) >= 20 * n_cells, f"{w}x{h}: at least half of the corners are still tracked after three frames"
            unlimited = want[n_cells + 3 * 3: n_cells + 3 * 3 + n_cells]
            assert all(len(u) > 20 for u in unlimited), "the no-limit call returns more than the limited one"
        _same_arrays(got[j], want, f"thread {j} ({w}x{h})")
    lk = after["lk"]["requests"] - before["lk"]["requests"], after["lk"]["launches"] - before["lk"]["launches"]
    det = after["det"]["requests"] - before["det"]["requests"]
    print(f"front-end chain: uploads {up}; LK requests / rounds {lk}; detector requests {det}")
    assert up["frames"] == 36 and lk[0] == 30 and det == 12, "every call went through the upload class and the combiners"


def test_more_front_end_callers_than_n_seq(pmv, gpu_ctx_factory):
    """n_seq counts back-end workspace sets, not callers: six threads on a session of n_seq = 1 each track 200 points in a context of
    max_tracks = 256, so two of their requests do not fit one round's result blocks (1 x 256 tracks). Requests that do not fit wait for the
    next round; every call returns the single call's bits and none fails (before the split, a round that overflowed failed all its
    requests with PMV_ERR_CAPACITY, which pmv_lk_track never raises for n <= max_tracks). The same for the kNN matcher."""
    w, h, seed = SIZES[1]
    frames = _frames(pmv, w, h, seed)
    ctx = gpu_ctx_factory(w, h, n_slots=2, max_tracks=256)
    ctx.frame_upload(0, frames[0]); ctx.frame_upload(1, frames[1])
    gx, gy = np.meshgrid(np.linspace(20, w - 20, 20), np.linspace(20, h - 20, 10))
    pts = [np.stack([gx.ravel() + 0.25 * j, gy.ravel() + 0.5 * j], 1).astype(np.float32) for j in range(6)]
    ipts = [p.astype(np.int32) for p in pts]
    want_lk = [ctx.lk_track(0, 1, p) for p in pts]
    want_knn = [ctx.knn_match(0, 1, p, ipts[0]) for p in ipts]
    assert all(len(p) == 200 and int(st.sum()) >= 100 for p, (_, st, _) in zip(pts, want_lk)), "the points are tracked"
    before = ctx.batch_stats()["lk"]
    with ctx.batch_session(1, [(w, h)]):
        start = threading.Barrier(6)

        def run(j):
            start.wait()
            return [(ctx.batch_lk_track(0, 1, pts[j]), ctx.batch_knn_match(0, 1, ipts[j], ipts[0])) for _ in range(10)]
        got = _threads(6, run)
    after = ctx.batch_stats()["lk"]
    for j in range(6):
        for lk, knn in got[j]:
            _same_arrays(list(lk), list(want_lk[j]), f"thread {j}: LK")
            _same_arrays(list(knn), list(want_knn[j]), f"thread {j}: kNN")
    assert after["requests"] - before["requests"] == 120 and after["launches"] - before["launches"] >= 120, "200 + 200 > 256: one request per round"


def test_shitomasi_fast_and_knn_chain_equals_the_single_calls(pmv, gpu_ctx_factory):
    """the same scheme with batch_detect_shitomasi (scores included), batch_detect_fast and batch_knn_match: four threads, two sizes"""
    ctx, ref = _ctxs(gpu_ctx_factory)
    seqs = [s for s in SIZES[1:] for _ in range(2)]
    with ctx.batch_session(4, [(w, h) for w, h, _ in SIZES[1:]]):
        api = _Api(ctx, True)
        got = _threads(4, lambda j: _chain_alt(pmv, api, _frames(pmv, *seqs[j]), [3 * j, 3 * j + 1, 3 * j + 2]))
    single = _Api(ref, False)
    for j, (w, h, seed) in enumerate(seqs):
        if j % 2 == 0:
            want = _chain_alt(pmv, single, _frames(pmv, w, h, seed), [0, 1, 2])
            n_cells = len(pmv.grid_cells(w, h))
            assert all(len(want[2 * i]) == 20 and want[2 * i + 1].dtype == np.float64 for i in range(n_cells)), "ShiTomasi: 20 corners with scores per cell"
            assert sum(len(a) for a in want[2 * n_cells: 4 * n_cells: 2]) >= 10 * n_cells, "FAST finds keypoints"
            best = want[-2]
            assert len(best) >= 10 * n_cells and (best >= 0).sum() * 2 >= len(best), "the kNN matcher matches"
        _same_arrays(got[j], want, f"thread {j} ({w}x{h})")


def _recorded_run(pmv, gpu_ctx_factory, ba_mode):
    key = ("run", ba_mode)
    if key not in _cache:
        if "back" not in _cache:
            w, h, n = 640, 200, 40
            frames, poses = pmv.synth_sequence(1007, 0, n, w, h, 0.58 * w, 0.58 * w, w / 2, h / 2, nthreads=8)
            ctx = gpu_ctx_factory(w, h, n_slots=n, max_tracks=4096)
            ctx.frames_stage(0, frames)
            _cache["back"] = (ctx, poses, np.array([0.58 * w, 0, w / 2, 0, 0.58 * w, h / 2, 0, 0, 1.0]))
        ctx, poses, K = _cache["back"]
        ctx.set_ba_mode(ba_mode)
        ctx.record_enable(True)
        ctx.pipeline_run(40, 640, 200, K, poses, threaded=1, want_features=False)
        ctx.record_enable(False)
        _cache[key] = ctx.records()
        ctx.record_enable(True); ctx.record_enable(False)   # drop the log
    return _cache["back"][0], _cache[key]


@pytest.mark.parametrize("ba_mode", [0, 1])
def test_back_end_calls_replayed_from_four_threads_are_bit_exact(pmv, gpu_ctx_factory, ba_mode):
    """the PnP, BA and two-view DLT calls that a 40-frame pipeline_run recorded, replayed through batch_pnp_ransac, batch_ba_solve and
    batch_triangulate_candidates from four threads (each its own seq, the calls dealt round-robin): every output equals the recorded one bit
    for bit - in both BA modes, each against a run recorded in that mode"""
    ctx, recs = _recorded_run(pmv, gpu_ctx_factory, ba_mode)
    kinds = [r["kind"] for r in recs]
    assert kinds.count("pnp") >= 10 and kinds.count("ba") >= 5 and kinds.count("dlt") >= 1, kinds

    def replay(t):
        n = 0
        for r in recs[t::4]:
            if r["kind"] == "pnp":
                rv, tv, inl = ctx.batch_pnp_ransac(t, r["obj"], r["img"], r["K"], r["rvec_in"], r["tvec_in"], r["iterations"], r["reproj_err"], r["confidence"])
                assert np.array_equal(inl, r["inliers"]) and np.array_equal(rv, r["rvec"]) and np.array_equal(tv, r["tvec"]), "PnP"
            elif r["kind"] == "ba":
                cams, pts, s = ctx.batch_ba_solve(t, r["cams_in"], r["pts_in"], r["obs"], r["cam_idx"], r["pt_idx"], r["K"], r["huber"], r["max_iterations"])
                assert np.array_equal(cams, r["cams"]) and np.array_equal(pts, r["pts"]), "BA parameters"
                assert (s.initial_cost, s.final_cost, s.iterations, s.successful_steps, s.termination) == \
                    (r["initial_cost"], r["final_cost"], r["iterations"], r["successful_steps"], r["termination"]), "BA summary"
            else:
                Q, mask, good = ctx.batch_triangulate_candidates(t, r["q1"], r["q2"], r["P1x4"], r["mask_in"])
                assert np.array_equal(Q, r["Q"]) and np.array_equal(mask, r["mask"]) and np.array_equal(good, r["good"]), "DLT"
            n += 1
        return n
    with ctx.batch_session(4, [(640, 200)]):
        done = _threads(4, replay)
        with pytest.raises(pmv.PmvError) as e:   # PMV_ERR_DEGENERATE arises where pmv_pnp_ransac raises it
            r = next(r for r in recs if r["kind"] == "pnp")
            ctx.batch_pnp_ransac(0, r["obj"][:5], r["img"][:5], r["K"], r["rvec_in"], r["tvec_in"])
        assert e.value.code == -5
    assert sum(done) == len(recs)
    ctx.set_ba_mode(0)


def test_fivepoint_round_from_four_threads_equals_the_single_call(pmv, orc, gpu_ctx_factory):
    """batch_fivepoint_hypotheses on the inputs of tests/test_backend_gpu.py's five-point test"""
    rng = np.random.default_rng(12)
    n = 400
    X = np.stack([rng.uniform(-8, 8, n), rng.uniform(-3, 2, n), rng.uniform(5, 40, n)], 1)
    rv = rng.normal(0, 0.03, 3); th = np.linalg.norm(rv); k = rv / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    R = np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx
    t = np.array([0.08, -0.03, -1.0]); t /= np.linalg.norm(t)
    Xc = X @ R.T + t
    f = 718.856
    q1 = np.floor(X[:, :2] / X[:, 2:3] * f + rng.normal(0, 0.3, (n, 2))) / f
    q2 = np.floor(Xc[:, :2] / Xc[:, 2:3] * f + rng.normal(0, 0.3, (n, 2))) / f
    q2[::7] += rng.normal(0, 0.05, q2[::7].shape)
    nh = 32
    samples = np.zeros((nh, 5), np.int32)
    orc.lib.orc_host_five_point_samples(n, nh, samples.ctypes.data_as(C.POINTER(C.c_int)))
    samples[5] = samples[5][[0, 0, 1, 2, 3]]
    thr = np.float32((1.0 / f) ** 2)
    ctx, _ = _ctxs(gpu_ctx_factory)
    want = ctx.fivepoint_hypotheses(q1, q2, samples, thr)
    assert want[1].sum() > 40 and want[1][5] == 0 and want[2].max() > 0.7 * n
    with ctx.batch_session(4, [(640, 200)]):
        got = _threads(4, lambda j: ctx.batch_fivepoint_hypotheses(j, q1, q2, samples, thr))
    for j in range(4):
        _same_arrays(list(got[j]), list(want), f"thread {j}")


def _refused(pmv, code, needles, call):
    with pytest.raises(pmv.PmvError) as e:
        call()
    assert e.value.code == code, e.value
    for s in needles:
        assert s in str(e.value), e.value


def test_the_rules_of_a_session_are_enforced(pmv, gpu_ctx_factory):
    """every refusal returns the stated status code and pmv_last_error names the cause; a refused call changes nothing; after batch_close a
    plain pipeline_run_batch on the same context gives its single-run bits"""
    import torch
    INVALID, CAPACITY = -2, -3
    w, h, n = 640, 200, 30
    frames, poses = pmv.synth_sequence(1007, 0, n, w, h, 0.58 * w, 0.58 * w, w / 2, h / 2, nthreads=8)
    K = np.array([0.58 * w, 0, w / 2, 0, 0.58 * w, h / 2, 0, 0, 1.0])
    ctx = gpu_ctx_factory(w, h, n_slots=2 * n, max_tracks=4096)
    ctx.frames_stage(0, frames); ctx.frames_stage(n, frames)
    single = ctx.pipeline_run(n, w, h, K, poses, threaded=1)
    pts = np.array([[100.0, 100.0]], np.float32)
    # no session
    for call in (lambda: ctx.batch_frame_upload(0, frames[0]), lambda: ctx.batch_lk_track(0, 1, pts), lambda: ctx.batch_detect_gftt(0, pmv.grid_cells(w, h), 20),
                 lambda: ctx.batch_pnp_ransac(0, np.zeros((8, 3)), np.zeros((8, 2)), K, np.zeros(3), np.zeros(3)), ctx.batch_upload_stats, ctx.batch_close):
        _refused(pmv, INVALID, ("no batch session is open",), call)
    _refused(pmv, CAPACITY, ("1241x376",), lambda: ctx.batch_open(2, [(w, h), (1241, 376)]))
    ctx.batch_open(2, [(w, h), (320, 100)])
    try:
        _refused(pmv, INVALID, ("already open",), lambda: ctx.batch_open(2, [(w, h)]))
        _refused(pmv, INVALID, ("batch session is open",), lambda: ctx.pipeline_run_batch([(0, n, poses), (n, n, poses)], w, h, K))
        _refused(pmv, INVALID, ("batch session is open",), lambda: ctx.pipeline_run_batch_streamed([(frames, poses)], K=K, ring=8))
        _refused(pmv, INVALID, ("600x200", "not declared"), lambda: ctx.batch_frame_upload(0, frames[0][:, :600]))
        _refused(pmv, INVALID, ("200x100", "not declared"), lambda: ctx.batch_frame_upload(0, torch.zeros((100, 200), dtype=torch.uint8, device="cuda:0")))
        g = np.ascontiguousarray(frames[0])
        rc = ctx.lib.pmv_batch_frame_upload(ctx.h, 0, g.ctypes.data_as(C.c_void_p), w, h, w - 1, 0)
        assert rc == CAPACITY and b"stride" in ctx.lib.pmv_last_error(ctx.h)
        rc = ctx.lib.pmv_batch_frame_upload(ctx.h, 0, g.ctypes.data_as(C.c_void_p), 320, 100, 3 * 320 - 1, 1)
        assert rc == CAPACITY and b"stride" in ctx.lib.pmv_last_error(ctx.h)
        _refused(pmv, CAPACITY, ("slot",), lambda: ctx.batch_frame_upload(2 * n, frames[0]))
        q = np.zeros((8, 2))
        for seq in (-1, 2):
            for call in (lambda: ctx.batch_pnp_ransac(seq, np.zeros((8, 3)), np.zeros((8, 2)), K, np.zeros(3), np.zeros(3)),
                         lambda: ctx.batch_ba_solve(seq, np.zeros((2, 6)), np.zeros((4, 3)), np.zeros((8, 2)), np.zeros(8, np.int32), np.zeros(8, np.int32), K),
                         lambda: ctx.batch_triangulate_candidates(seq, q, q, np.zeros(48), np.ones(8, np.uint8)),
                         lambda: ctx.batch_fivepoint_hypotheses(seq, q, q, np.arange(5, dtype=np.int32), 1e-6)):
                _refused(pmv, INVALID, (f"seq {seq}",), call)
        # nothing has changed: the session still serves, and its results are the single calls'
        ctx.batch_frame_upload(0, frames[0]); ctx.batch_frame_upload(1, frames[1])
        cells = pmv.grid_cells(w, h)
        det = ctx.batch_detect_gftt(0, cells, 20)
        p0 = np.concatenate([d + c[:2] for c, d in zip(cells, det)]).astype(np.float32)
        got = ctx.batch_lk_track(0, 1, p0)
        assert ctx.batch_upload_stats()["frames"] == 2
    finally:
        ctx.batch_close()
    want = ctx.lk_track(0, 1, p0)
    assert len(p0) == 60 and all(np.array_equal(a, b) for a, b in zip(got, want))
    # the context serves batched runs again, with its single-run bits (slots 0 and 1 hold frames 0 and 1 again, built)
    for r in ctx.pipeline_run_batch([(0, n, poses), (n, n, poses)], w, h, K):
        assert np.array_equal(r.poses, single.poses) and len(r.poses) > 0
        for x, y in zip(r.features, single.features):
            assert np.array_equal(x, y)
