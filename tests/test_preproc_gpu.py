"""pmv_set_frame_preproc on the device: host frames that enter a slot through the feeder - the pmv_frames_stream_begin bracket,
pmv_pipeline_run_streamed, pmv_pipeline_run_batch_streamed - are remapped and / or equalised on their way in. A slot then holds, at EVERY
level with its border, the bytes that pmv_frame_upload of the CPU twins' output (tests/twin/remap_twin.cpp, clahe_twin.cpp) leaves in another
slot, and every pipeline result equals, bit for bit, the same run with the setting off on host frames that the twins preprocessed."""
import ctypes as C
import os

import numpy as np
import pytest

import clahe_common as cc
import remap_common as rc

pytestmark = pytest.mark.gpu

INVALID = -2                  # PMV_ERR_INVALID
CAP_W, CAP_H = 203, 120       # the bracket cases' largest width and height
N_BRACKET = 20                # frames per bracket case: more than BRACKET_CHUNK = 16, so two feeder rounds
ROUNDS = 2
REF = N_BRACKET               # the slot the twins' images are uploaded into

_cache = {}


# ---- 1. the bracket: slot contents -----------------------------------------------------------------------------------------------------

def _bracket_cases():
    """(w, h, map or None, border, (clip, tiles) or None, format). Remap alone: every map of the issue at every size, gray, and two of them
    from colour frames; CLAHE alone: clip 2.0 and 0.0, tiles (8, 8) and the non-divisible (3, 5); both stages, gray and colour."""
    cases = []
    for w, h in rc.SIZES:
        maps = [("identity", 0), ("ties", 0), ("turn", 0), ("undistort06", 0), ("undistort06", 200)]
        if (w, h) == (160, 120):
            maps.append(("special", 0))
        cases += [(w, h, m, b, None, "gray") for m, b in maps]
        cases += [(w, h, "ties", 0, None, "bgr"), (w, h, "undistort06", 200, None, "bgr")]
        cases += [(w, h, None, 0, cl, "gray") for cl in ((2.0, (8, 8)), (0.0, (8, 8)), (2.0, (3, 5)))]
        cases += [(w, h, None, 0, (2.0, (8, 8)), "bgr")]
        cases += [(w, h, "undistort06", 200, (2.0, (3, 5)), "gray"), (w, h, "undistort06", 200, (2.0, (3, 5)), "bgr"), (w, h, "ties", 0, (0.0, (8, 8)), "gray")]
    return cases


def _bracket_id(case):
    w, h, m, b, cl, fmt = case
    return f"{w}x{h}-{m or 'nomap'}-b{b}-" + (f"clahe{cl[0]:g}-{cl[1][0]}x{cl[1][1]}" if cl else "noclahe") + f"-{fmt}"


def _bracket_ctx(gpu_ctx_factory):
    if "bracket_ctx" not in _cache:
        _cache["bracket_ctx"] = gpu_ctx_factory(CAP_W, CAP_H, n_slots=N_BRACKET + 1, max_tracks=1024)
    return _cache["bracket_ctx"]


def _map(pmv, ctx, name, w, h):
    """the id of a map on the bracket context, created once (13 maps: within the 16 of a context)"""
    key = ("map", name, w, h)
    if key not in _cache:
        _cache[key] = ctx.remap_map_create(*rc.maps(pmv, name, w, h))
    return _cache[key]


def _bgr(g):
    """three different planes, so that the conversion is not the identity"""
    return np.ascontiguousarray(np.stack([g, np.roll(g, 3, axis=1), np.roll(g, 2, axis=0)], axis=2))


def _gray(bgr):
    """cv::cvtColor(BGR2GRAY) for 8-bit images"""
    b, g, r = (bgr[..., k].astype(np.int64) for k in range(3))
    return ((b * 1868 + g * 9617 + r * 4899 + 8192) >> 14).astype(np.uint8)


def _twins(pmv, gray, name, w, h, border, clahe):
    out = gray
    if name is not None:
        out = rc.twin().apply(out, *rc.maps(pmv, name, w, h), border)[0]
    if clahe is not None:
        out = cc.twin().apply(out, clahe[0], clahe[1])[0]
    return out


def _levels(ctx, slot, cap_w=CAP_W, cap_h=CAP_H):
    return [ctx.get_level_padded(slot, l, cap_w, cap_h) for l in range(ctx.num_levels(slot) + 1)]


def _same_levels(got, want, what):
    assert len(got) == len(want) >= 1, f"{what}: {len(got)} levels, expected {len(want)}"
    for l, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape and np.array_equal(a, b), f"{what}: level {l} differs in {int((a != b).sum())} bytes"


def _run_bracket(pmv, gpu_ctx_factory, case, pinned=False):
    w, h, name, border, clahe, fmt = case
    ctx = _bracket_ctx(gpu_ctx_factory)
    img = rc.image(pmv, w, h)
    grays = [np.roll(img, k, axis=1) for k in range(N_BRACKET)]
    if fmt == "bgr":
        frames = np.stack([_bgr(g) for g in grays])
        grays = [_gray(f) for f in frames]
        assert not np.array_equal(grays[0], img), "the conversion is not the identity"
    else:
        frames = np.stack(grays)
    if pinned:
        import torch   # only to get page-locked host memory
        keep = torch.empty(frames.shape, dtype=torch.uint8).pin_memory()
        keep.numpy()[:] = frames
        frames = keep.numpy()
    want = [_twins(pmv, g, name, w, h, border, clahe) for g in grays]
    if name == "undistort06":   # taps beyond all four sides
        st = rc.twin().apply(grays[0], *rc.maps(pmv, name, w, h), border)[1]
        assert min(st["left"], st["right"], st["above"], st["below"]) > 0
    ctx.set_frame_format(fmt)
    try:
        ctx.set_frame_preproc(remap=None if name is None else _map(pmv, ctx, name, w, h), border_value=border, clahe=clahe)
        before = ctx.debug_preproc_launches()
        ctx.frames_stream_begin(0, frames)
        ctx.frames_stream_end()
        after = ctx.debug_preproc_launches()
    finally:
        ctx.set_frame_preproc()
        ctx.set_frame_format("gray")
    assert [a - b for a, b in zip(after, before)] == [ROUNDS, ROUNDS if name is not None else 0, ROUNDS if clahe is not None else 0, ROUNDS]
    for k in range(N_BRACKET):
        ctx.frame_upload(REF, want[k])
        _same_levels(_levels(ctx, k), _levels(ctx, REF), f"slot {k}")


@pytest.mark.parametrize("case", _bracket_cases(), ids=_bracket_id)
def test_bracket_slot_contents_equal_the_twins(pmv, gpu_ctx_factory, case):
    """twenty distinct frames (the case's image rolled by the frame index) through a bracket of two rounds: after pmv_frames_stream_end every
    slot equals pmv_frame_upload of the twins' image at every level with its border; one gather launch, at most one CLAHE pair and one
    border launch per round"""
    _run_bracket(pmv, gpu_ctx_factory, case)


@pytest.mark.parametrize("fmt", ["gray", "bgr"])
def test_bracket_from_pinned_memory_and_in_the_mapped_form(pmv, gpu_ctx_factory, fmt):
    """a pinned source is DMA'd straight into the landing buffer, so the round's tables travel in a copy of their own; and with
    PMV_BATCH_INGEST=mapped a CLAHE-only bracket reads its tables and frames across the link while a remap still lands its frames in HBM"""
    _run_bracket(pmv, gpu_ctx_factory, (203, 87, "undistort06", 200, (2.0, (3, 5)), fmt), pinned=True)
    _run_bracket(pmv, gpu_ctx_factory, (203, 87, None, 0, (2.0, (8, 8)), fmt), pinned=True)
    old = os.environ.get("PMV_BATCH_INGEST")
    os.environ["PMV_BATCH_INGEST"] = "mapped"
    try:
        for pinned in (False, True):
            _run_bracket(pmv, gpu_ctx_factory, (203, 87, None, 0, (2.0, (3, 5)), fmt), pinned=pinned)
            _run_bracket(pmv, gpu_ctx_factory, (41, 40, "turn", 0, None, fmt), pinned=pinned)
    finally:
        if old is None:
            del os.environ["PMV_BATCH_INGEST"]
        else:
            os.environ["PMV_BATCH_INGEST"] = old


# ---- 2. / 3. the streamed batch ---------------------------------------------------------------------------------------------------------

A = dict(w=1241, h=376, f=718.856, cx=607.1928, cy=185.2157)
B = dict(w=1226, h=370, f=707.0912, cx=601.8873, cy=183.1104)
# (size, seed, frames): poses and pnp_calls of the oracle's pipeline on the twins' frames (remap, remap + CLAHE), computed on the CPU:
#   1005 / 30 / A: 29 poses, 21 and 22;  1002 / 26 / B: 25 poses, 19 and 17;  1003 / 30 / A: 29 poses, 23 and 22
SEQS = [(A, 1005, 30), (B, 1002, 26), (A, 1003, 30), (A, 1005, 30)]   # the first sequence again in a fourth batch slot
DIST = (-0.05, 0.01)          # k1, k2 with new_K = K: every tap inside the frame (border taps are the bracket test's business)
CLAHE = (2.0, (8, 8))
RING = 6
STAT_KEYS = ("lk_calls", "lk_points", "detect_calls", "pnp_calls", "pnp_points", "tri_calls", "ba_calls", "ba_obs", "ba_points",
             "heuristic_motion", "init_offset", "n_landmarks", "scale", "tri_hypotheses")


def _K(c):
    return np.array([c["f"], 0, c["cx"], 0, c["f"], c["cy"], 0, 0, 1.0])


def _assert_same(a, b, what):
    assert np.array_equal(a.poses, b.poses), f"{what}: poses differ"
    assert len(a.features) == len(b.features), f"{what}: frame counts differ"
    for k, (x, y) in enumerate(zip(a.features, b.features)):
        assert np.array_equal(x, y), f"{what}: features of frame {k} differ"
    for key in STAT_KEYS:
        assert a.stats[key] == b.stats[key], (what, key, a.stats[key], b.stats[key])


def _camera_maps(pmv, c):
    key = ("camera_maps", c["w"], c["h"])
    if key not in _cache:
        _cache[key] = pmv.undistort_map(_K(c).reshape(3, 3), DIST, (c["w"], c["h"]), new_K=_K(c).reshape(3, 3))
    return _cache[key]


def _sequence(pmv, c, seed, n):
    """(raw frames, ground truth, the twins' frames: remapped then equalised), computed once"""
    key = ("sequence", c["w"], seed, n)
    if key not in _cache:
        frames, gt = pmv.synth_sequence(seed, 0, n, c["w"], c["h"], c["f"], c["f"], c["cx"], c["cy"], nthreads=16)
        mx, my = _camera_maps(pmv, c)
        pre = np.stack([cc.twin().apply(rc.twin().apply(f, mx, my, 0)[0], *CLAHE)[0] for f in frames])
        _cache[key] = (frames, gt, pre)
    return _cache[key]


def _batch_ctx(pmv, gpu_ctx_factory):
    """the context of the streamed batches, with the two cameras' maps"""
    if "batch_ctx" not in _cache:
        ctx = gpu_ctx_factory(A["w"], A["h"], n_slots=len(SEQS) * RING, max_tracks=4096)
        _cache["batch_ctx"] = (ctx, [ctx.remap_map_create(*_camera_maps(pmv, c)) for c in (A, B)])
    return _cache["batch_ctx"]


def _streamed(ctx, data, Ks, preproc):
    """one pipeline_run_batch_streamed under a setting that is cleared again; (results, ingest counters, preprocessing launches made)"""
    before = ctx.debug_preproc_launches()
    if preproc is not None:
        ctx.set_frame_preproc(**preproc)
    try:
        got = ctx.pipeline_run_batch_streamed(data, K=np.stack(Ks), ring=RING)
    finally:
        ctx.set_frame_preproc()
    return got, ctx.batch_ingest_stats(), [a - b for a, b in zip(ctx.debug_preproc_launches(), before)]


def _reference(pmv, gpu_ctx_factory):
    """the four sequences with the setting OFF on the twins' frames, once"""
    if "reference" not in _cache:
        ctx, _ = _batch_ctx(pmv, gpu_ctx_factory)
        seqs = [_sequence(pmv, *s) for s in SEQS]
        ref, _, launches = _streamed(ctx, [(pre, gt) for _, gt, pre in seqs], [_K(s[0]) for s in SEQS], None)
        assert launches == [0, 0, 0, 0]
        _cache["reference"] = ref
    return _cache["reference"]


def test_streamed_batch_of_mixed_sizes_on_recycled_rings(pmv, gpu_ctx_factory):
    """four sequences of two sizes (one of them in two batch slots) on rings of 6 slots, two maps, CLAHE behind them: every result equals
    the run with the setting off on the twins' frames, and one sequence also equals stage -> remap -> clahe -> run on a context of its own"""
    ctx, maps = _batch_ctx(pmv, gpu_ctx_factory)
    seqs = [_sequence(pmv, *s) for s in SEQS]
    ref = _reference(pmv, gpu_ctx_factory)
    got, ing, launches = _streamed(ctx, [(raw, gt) for raw, gt, _ in seqs], [_K(s[0]) for s in SEQS], dict(remap=maps, clahe=CLAHE))
    _cache["streamed"] = got
    print("ingest:", ing, "preprocessing launches:", launches)
    for b, (c, seed, n) in enumerate(SEQS):
        # what keeps this from comparing two empty runs: every sequence yields all its poses and solves PnP
        assert len(ref[b].poses) == n - 1 and ref[b].stats["pnp_calls"] > 0, (b, len(ref[b].poses), ref[b].stats["pnp_calls"])
        _assert_same(got[b], ref[b], f"sequence {b} (seed {seed}, {c['w']}x{c['h']})")
    _assert_same(got[0], got[3], "the same input in two batch slots")
    total = sum(n for _, _, n in SEQS)
    assert ing["frames"] == total and ing["bytes"] == sum(c["w"] * c["h"] * n for c, _, n in SEQS)
    assert launches[0] == ing["rounds"] and launches == [launches[0]] * 4, "one gather, one CLAHE pair and one border launch per round"
    assert RING < ing["rounds"] < total, "the rings are recycled and rounds hold several frames"
    # sequence 1 (1226 x 370) the way a caller had to do it before: every frame staged, remapped and equalised in its slot
    c, seed, n = SEQS[1]
    raw, gt, _ = seqs[1]
    own = gpu_ctx_factory(c["w"], c["h"], n_slots=n, max_tracks=4096)
    own.frames_stage(0, raw)
    mid = own.remap_map_create(*_camera_maps(pmv, c))
    own.frames_remap(0, n, mid, 0)
    own.frames_clahe(0, n, *CLAHE)
    _assert_same(got[1], own.pipeline_run(n, c["w"], c["h"], _K(c), gt, threaded=1), "sequence 1 vs stage -> remap -> clahe -> run")
    # and through pmv_pipeline_run_streamed (a bracket under the run) with the setting on
    own.set_frame_preproc(remap=mid, clahe=CLAHE)
    try:
        _assert_same(got[1], own.pipeline_run(n, c["w"], c["h"], _K(c), gt, threaded=1, host_frames=raw), "sequence 1 vs pmv_pipeline_run_streamed")
    finally:
        own.set_frame_preproc()


@pytest.mark.parametrize("source", ["pageable", "pinned"])
@pytest.mark.parametrize("mode", ["copy", "mapped"])
def test_ingest_forms_and_sources(pmv, gpu_ctx_factory, mode, source):
    """the first two sequences under both values of PMV_BATCH_INGEST, from pageable and from pinned memory: the results of the test above,
    and - a remap never gathers across the host link - the frames' bytes moved in both forms"""
    ctx, maps = _batch_ctx(pmv, gpu_ctx_factory)
    ref = _reference(pmv, gpu_ctx_factory)
    seqs = [_sequence(pmv, *s) for s in SEQS[:2]]
    data, keep = [], []
    for raw, gt, _ in seqs:
        if source == "pinned":
            import torch   # only to get page-locked host memory
            pinned = torch.empty(raw.shape, dtype=torch.uint8).pin_memory()
            pinned.numpy()[:] = raw
            keep.append(pinned)
            raw = pinned.numpy()
        data.append((raw, gt))
    old = os.environ.get("PMV_BATCH_INGEST")
    os.environ["PMV_BATCH_INGEST"] = mode
    try:
        got, ing, launches = _streamed(ctx, data, [_K(s[0]) for s in SEQS[:2]], dict(remap=maps, clahe=CLAHE))
    finally:
        if old is None:
            del os.environ["PMV_BATCH_INGEST"]
        else:
            os.environ["PMV_BATCH_INGEST"] = old
    for b in range(2):
        _assert_same(got[b], ref[b], f"{mode}, {source}: sequence {b}")
    assert ing["frames"] == sum(n for _, _, n in SEQS[:2]) and ing["bytes"] == sum(c["w"] * c["h"] * n for c, _, n in SEQS[:2]), ing
    assert launches[0] == ing["rounds"] and launches == [launches[0]] * 4


# ---- 4. off means off -------------------------------------------------------------------------------------------------------------------

def test_off_means_off(pmv):
    """a streamed batch before any setter call and after a setting was made and cleared: the same results, the same feeder launches, no
    preprocessing launch, and the memory counters back where they were once the context is closed.
    pmv_debug_batch_launches: the feeder's two entries (level 0, pyrDown) are compared exactly - every ring holds its whole sequence, so
    the rounds do not depend on timing. The k_lk_batch entry counts rounds of the LK combiner, which merges whatever requests have arrived
    when it looks: between the longer sequence's LK calls and the sum of both, in either run."""
    w, h, f, cx, cy = 640, 200, 370.0, 320.0, 100.0
    K = np.array([f, 0, cx, 0, f, cy, 0, 0, 1.0])
    lengths = (14, 12)
    data = [pmv.synth_sequence(1013 + i, 0, n, w, h, f, f, cx, cy, nthreads=8) for i, n in enumerate(lengths)]
    live0 = pmv.mem_live()
    ctx = pmv.Context(w, h, n_slots=32, max_tracks=4096)
    try:
        def run():
            l0 = ctx.batch_launches()
            got = ctx.pipeline_run_batch_streamed(data, K=K, ring=16)
            l1 = ctx.batch_launches()
            return got, {k: l1[k] - l0[k] for k in l0}
        assert ctx.get_frame_preproc() == dict(remap=[], border_value=0, clahe=None) and ctx.debug_preproc_launches() == [0, 0, 0, 0]
        first, d1 = run()
        j, i = np.meshgrid(np.arange(w, dtype=np.float32), np.arange(h, dtype=np.float32))
        mid = ctx.remap_map_create(j, i)
        ctx.set_frame_preproc(remap=mid, border_value=7, clahe=(2.0, (8, 8)))
        assert ctx.get_frame_preproc() == dict(remap=[mid], border_value=7, clahe=(2.0, (8, 8)))
        ctx.set_frame_preproc()
        assert ctx.get_frame_preproc() == dict(remap=[], border_value=0, clahe=None)
        second, d2 = run()
        for b in range(2):
            assert first[b].stats["pnp_calls"] > 0 and len(first[b].poses) == lengths[b] - 1
            _assert_same(second[b], first[b], f"sequence {b}")
        print("launches:", d1, d2)
        assert d1["k_pad_level0"] == d2["k_pad_level0"] > 0 and d1["k_pyrdown"] == d2["k_pyrdown"] > 0 and d1["k_knn_round"] == d2["k_knn_round"] == 0
        for d in (d1, d2):
            assert max(lengths) - 1 <= d["k_lk_batch"] <= sum(lengths) - 2
        assert ctx.debug_preproc_launches() == [0, 0, 0, 0]
    finally:
        ctx.close()
    assert pmv.mem_live() == live0


# ---- 5. errors --------------------------------------------------------------------------------------------------------------------------

def _refused(fn):
    with pytest.raises(Exception) as e:
        fn()
    return getattr(e.value, "code", None), str(e.value)


def test_errors(pmv, gpu_ctx_factory):
    ctx = _bracket_ctx(gpu_ctx_factory)
    big, small = rc.image(pmv, 160, 120), rc.image(pmv, 41, 40)
    m_big = _map(pmv, ctx, "identity", 160, 120)
    m_big2 = _map(pmv, ctx, "ties", 160, 120)
    m_small = _map(pmv, ctx, "identity", 41, 40)
    off = dict(remap=[], border_value=0, clahe=None)
    assert ctx.get_frame_preproc() == off
    # two maps of one size; an unknown id; too many; the library's own range checks (the binding refuses these before the library)
    code, msg = _refused(lambda: ctx.set_frame_preproc(remap=[m_big, m_small, m_big2]))
    assert code == INVALID and f"maps {m_big} and {m_big2} are both 160x120" in msg, msg
    code, msg = _refused(lambda: ctx.set_frame_preproc(remap=[m_small, 15]))
    assert code == INVALID and "map 15 does not exist" in msg, msg
    assert ctx.get_frame_preproc() == off

    def raw(n_maps=0, ids=(), border=0, clahe=0, clip=2.0, tiles=(8, 8)):
        p = pmv.FramePreproc()
        p.n_maps, p.border_value, p.clahe = n_maps, border, clahe
        for k, i in enumerate(ids):
            p.map_ids[k] = i
        p.clahe_params = pmv.ClaheParams(clip, *tiles)
        ctx.lib.pmv_set_frame_preproc.argtypes = [C.c_void_p, C.POINTER(pmv.FramePreproc)]
        rc_ = ctx.lib.pmv_set_frame_preproc(ctx.h, C.byref(p))
        return rc_, ctx.lib.pmv_last_error(ctx.h).decode()
    for args, text in ((dict(n_maps=1, ids=(m_big,), border=-1), "border_value = -1 is outside 0..255"),
                       (dict(border=256), "border_value = 256 is outside 0..255"),
                       (dict(n_maps=9), "n_maps = 9 is outside 0..8"), (dict(n_maps=-1), "n_maps = -1 is outside 0..8"),
                       (dict(clahe=1, tiles=(17, 8)), "tiles = (17, 8) is outside 1..16"), (dict(clahe=1, clip=-1.0), "clip_limit = -1 is negative or not finite")):
        code, msg = raw(**args)
        assert code == INVALID and "pmv_set_frame_preproc" in msg and text in msg, (args, code, msg)
        assert ctx.get_frame_preproc() == off
    ctx.lib.pmv_set_frame_preproc.argtypes = [C.c_void_p, C.POINTER(pmv.FramePreproc)]
    assert ctx.lib.pmv_set_frame_preproc(None, None) == INVALID

    # a sequence whose size has no map: refused before a slot changes - in a bracket ...
    ctx.frame_upload(0, big)
    state = [ctx.num_levels(s) for s in range(N_BRACKET + 1)]
    slot0 = _levels(ctx, 0)
    ctx.set_frame_preproc(remap=m_small, clahe=(2.0, (8, 8)))
    try:
        code, msg = _refused(lambda: ctx.frames_stream_begin(0, np.stack([big] * 3)))
        assert code == INVALID and "sequence 0" in msg and "160x120" in msg and "no remap map of that size" in msg, msg
        ctx.frames_stream_end()
        # ... and in a streamed batch of two sizes with a map for one of them
        gt = np.tile(np.eye(3, 4).reshape(12), (8, 1))
        seqs = [(np.stack([small] * 8), gt), (np.stack([big] * 8), gt)]
        code, msg = _refused(lambda: ctx.pipeline_run_batch_streamed(seqs, K=np.array([100.0, 0, 20, 0, 100.0, 20, 0, 0, 1]), ring=8))
        assert code == INVALID and "sequence 1" in msg and "160x120" in msg and "no remap map of that size" in msg, msg
        assert [ctx.num_levels(s) for s in range(N_BRACKET + 1)] == state
        _same_levels(_levels(ctx, 0), slot0, "slot 0 after the refused feeds")
        # a map that the setting names cannot be destroyed
        code, msg = _refused(lambda: ctx.remap_map_destroy(m_small))
        assert code == INVALID and f"map {m_small} is named by the frame preprocessing setting" in msg, msg
        assert ctx.get_frame_preproc() == dict(remap=[m_small], border_value=0, clahe=(2.0, (8, 8)))
    finally:
        ctx.set_frame_preproc()
    # the setter during an open bracket: the setting is unchanged
    ctx.set_frame_preproc(clahe=(0.0, (3, 5)))
    try:
        ctx.frames_stream_begin(0, np.stack([small] * 3))
        try:
            for kw in (dict(remap=m_small), dict()):
                code, msg = _refused(lambda: ctx.set_frame_preproc(**kw))
                assert code == INVALID and "a pmv_frames_stream_begin bracket is open" in msg, msg
                assert ctx.get_frame_preproc() == dict(remap=[], border_value=0, clahe=(0.0, (3, 5)))
        finally:
            ctx.frames_stream_end()
        ctx.frame_upload(REF, cc.twin().apply(small, 0.0, (3, 5))[0])
        _same_levels(_levels(ctx, 2), _levels(ctx, REF), "the bracket under which the setter was refused")
    finally:
        ctx.set_frame_preproc()
    assert ctx.get_frame_preproc() == off
    # cleared: the map goes (and is made again for the tests that share the context)
    ctx.remap_map_destroy(m_small)
    del _cache[("map", "identity", 41, 40)]
