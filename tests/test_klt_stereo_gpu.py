"""pmv_klt_step_stereo and pmv_klt_step_many_stereo on the device, byte for byte: the left outputs against pmv_klt_step's two yardsticks
(tests/klt_common.py; counts[7] = the number of matched tracks), the right outputs - xy as uint32, status as bytes - against the stereo rule
on the CPU twin of LK and on the Context's single LK calls for the pair (cur_slot, right_slot) (tests/klt_stereo_common.py). What the scene
is there for is asserted on the twin alone in tests/test_klt_stereo_twin.py. Slots: left frame i in slot i, its right frame in slot
len(lefts) + i."""
import numpy as np
import pytest

import klt_common as kc
import klt_stereo_common as ks

pytestmark = pytest.mark.gpu
INVALID, CAPACITY = ks.INVALID, ks.CAPACITY


def _run(ctx, lefts, rts, p, st, want, key, calls=True, twin=True, right=None):
    """stereo steps over the frames from an empty tracker: step 0 matches corners born in the same call. right(i): the right slot of step
    i (default: len(lefts) + i)"""
    nl = len(lefts)
    right = right or (lambda i: nl + i)
    trk = ctx.klt_create(**p)
    trk.set_stereo(**st)
    assert trk.get_stereo() == (st["fb_max_dist"], st["border"])
    wr = ks.twin_stereo_run(lefts, rts, want, st, key) if twin else None
    state, outs = kc.empty_state(), []
    for i in range(nl):
        got = trk.step_stereo(max(i - 1, 0), i, right(i))
        if twin:
            ks.same_stereo(got, want[i][1], wr[i])
        if calls:
            state, ref = kc.calls_step(ctx, state, max(i - 1, 0), i, p)
            ks.same_stereo(got, ref, ks.calls_stereo(ctx, i, right(i), ref[2], st))
        assert got[4][7] == got[6].sum() and set(np.unique(got[6])) <= {0, 1}
        outs.append(got)
    kc.same(trk.get_tracks(), outs[-1][:3])
    trk.close()
    return outs


@pytest.mark.parametrize("size", kc.SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("name", ["default", "subpix"])
@pytest.mark.parametrize("stereo", list(ks.STEREO))
def test_sequences(pmv, gpu_ctx_factory, size, name, stereo):
    """203 x 87 keeps n far below the target: the void workgroups of the bound-sized launch are there in every step"""
    w, h = size
    lefts, rts = kc.scene(pmv, w, h), ks.scene_rights(pmv, w, h)
    p, want = kc.scene_run(pmv, w, h, name)
    outs = _run(ks.make_ctx(gpu_ctx_factory, lefts, rts), lefts, rts, p, ks.STEREO[stereo], want, (w, h, name, stereo))
    assert outs[0][4][0] == 0 and outs[0][4][7] > 0, "step 0 matched no corner born in the same call"
    assert all(0 < o[4][7] <= len(o[0]) for o in outs)
    if size == kc.SIZES[1]:
        assert all(len(o[0]) < p["target"] for o in outs)


@pytest.mark.parametrize("target", kc.TARGETS)
def test_targets(pmv, gpu_ctx_factory, target):
    """a lane short of a wavefront, a wavefront, one more, and several: the launch bound and the chunks of the rule's kernel"""
    w, h = kc.SIZES[0]
    lefts, rts = kc.scene(pmv, w, h), ks.scene_rights(pmv, w, h)
    p, want = kc.scene_run(pmv, w, h, "default", target=target)
    _run(ks.make_ctx(gpu_ctx_factory, lefts, rts), lefts, rts, p, ks.STEREO["fb"], want, (w, h, "default", "fb", target), calls=False)


def test_more_than_1024_tracks(pmv, gpu_ctx_factory):
    lefts = kc.big_pair(pmv)
    rts = ks.rights(lefts, "big")
    p, want = kc.big_run(pmv)
    outs = _run(ks.make_ctx(gpu_ctx_factory, lefts, rts, max_tracks=2048), lefts, rts, p, ks.STEREO["fb"], want, "big", calls=False)
    assert max(len(o[0]) for o in outs) > 1024 and all(o[4][7] > 512 for o in outs)


def test_a_constant_gray_pair_gives_no_tracks_and_writes_nothing_to_the_right(pmv, gpu_ctx_factory):
    """the device's count is zero under a full-size grid"""
    w, h = 64, 48
    g = ks.gray_pair(w, h)
    ctx = ks.make_ctx(gpu_ctx_factory, g, g)
    p = kc.params()
    trk = ctx.klt_create(**p)
    trk.set_stereo(**ks.STEREO["fb"])
    for i in range(2):
        rc, _, a = ks.raw_step(ctx.h, ctx.lib, trk.id, max(i - 1, 0), i, 2 + i, p["target"])
        assert rc == 0, ks.last_error(ctx)
        assert a["out_n"][0] == 0 and a["out_counts"].tolist() == [0, 0, 0, 0, 0, -1, 0, 0]
        assert (a["out_rxy"] == ks.CANARY).all() and (a["out_rst"] == 0xA5).all() and (a["out_xy"] == ks.CANARY).all()
    assert len(trk.get_tracks()[0]) == 0
    trk.close()


def test_a_40x40_frame_pair(pmv, gpu_ctx_factory):
    lefts, rts = ks.small_pair(pmv)
    p = kc.params(**ks.SMALL)
    want = kc.twin_run(lefts, p, "40x40")
    outs = _run(ks.make_ctx(gpu_ctx_factory, lefts, rts), lefts, rts, p, ks.STEREO["fb"], want, "40x40")
    assert outs[0][4][4] > 0 and outs[0][4][7] > 0


@pytest.mark.parametrize("stereo", list(ks.STEREO))
def test_right_slot_equal_to_cur_slot(pmv, gpu_ctx_factory, stereo):
    """the same slot index as current and as right frame, single and many form: the composition's bytes, and every track inside the stereo
    border is matched"""
    w, h = kc.SIZES[0]
    lefts = kc.scene(pmv, w, h)[:3]
    p, want = kc.scene_run(pmv, w, h, "default")
    st = dict(ks.STEREO[stereo], border=8)
    ctx = gpu_ctx_factory(w, h, n_slots=3, max_tracks=2048)
    kc.upload(ctx, lefts)
    outs = _run(ctx, lefts, lefts, p, st, want[:3], (w, h, "self", stereo), right=lambda i: i)
    for o in outs:
        inside = kc.in_border(o[2], 8, w, h)
        assert np.array_equal(o[6] == 1, inside) and 0 < inside.sum() < len(inside)
    a, b = ctx.klt_create(**p), ctx.klt_create(**p)
    a.set_stereo(**st)
    b.set_stereo(**ks.STEREO[stereo])
    wide = ks.twin_stereo_run(lefts, lefts, want[:3], ks.STEREO[stereo], (w, h, "self-border-1", stereo))
    for i in range(3):
        cur = [i, i]
        got = ctx.klt_step_many_stereo([a, b], [max(i - 1, 0)] * 2, cur, cur)
        kc.same(got[0][:5], outs[i][:5])
        ks.same_right(got[0][5:], outs[i][5:])
        ks.same_stereo(got[1], want[i][1], wide[i])
        ks.same_right(got[1][5:], ks.calls_stereo(ctx, i, i, got[1][2], ks.STEREO[stereo]))
    a.close()
    b.close()


def test_steps_inside_an_open_stream_bracket(pmv, gpu_ctx_factory):
    """left and right frames on their way in through pmv_frames_stream_begin: the step's slot checks, the pair (cur, right) included, wait
    for the slots' rounds on the front-end stream, and the step returns what it returns on uploaded frames"""
    w, h = kc.SIZES[1]
    lefts, rts = kc.scene(pmv, w, h), ks.scene_rights(pmv, w, h)
    p, want = kc.scene_run(pmv, w, h, "default")
    st = ks.STEREO["fb"]
    wr = ks.twin_stereo_run(lefts, rts, want, st, (w, h, "default", "fb"))
    nl = len(lefts)
    ctx = gpu_ctx_factory(w, h, n_slots=2 * nl, max_tracks=2048)
    both = np.ascontiguousarray(np.concatenate([lefts, rts]))
    trk = ctx.klt_create(**p)
    trk.set_stereo(**st)
    ctx.frames_stream_begin(0, both)
    try:
        for i in range(nl):
            ks.same_stereo(trk.step_stereo(max(i - 1, 0), i, nl + i), want[i][1], wr[i])
    finally:
        ctx.frames_stream_end()
    trk.close()


def test_window_21_and_three_levels(pmv, gpu_ctx_factory):
    """the general LK kernel through the device-counted entry; the yardstick is the composition of the Context's own single calls"""
    w, h = kc.SIZES[0]
    lefts, rts = kc.scene(pmv, w, h)[:3], ks.scene_rights(pmv, w, h)[:3]
    ctx = gpu_ctx_factory(w, h, n_slots=6, max_tracks=2048)
    ctx.set_lk_params(win=21, max_level=3)
    ks.upload_pair(ctx, lefts, rts)
    for stereo in ks.STEREO:
        outs = _run(ctx, lefts, rts, kc.params(), ks.STEREO[stereo], None, None, twin=False)
        assert all(0 < o[4][7] <= len(o[0]) for o in outs)


def test_mixing_with_plain_steps_and_single_calls(pmv, gpu_ctx_factory):
    w, h = kc.SIZES[0]
    lefts, rts = kc.scene(pmv, w, h), ks.scene_rights(pmv, w, h)
    p, want = kc.scene_run(pmv, w, h, "subpix")
    st = ks.STEREO["fb"]
    wr = ks.twin_stereo_run(lefts, rts, want, st, (w, h, "subpix", "fb"))
    ctx = ks.make_ctx(gpu_ctx_factory, lefts, rts)
    rng = np.random.default_rng(9)
    pts = np.stack([rng.uniform(8, w - 8, 90), rng.uniform(8, h - 8, 90)], axis=1).astype(np.float32)

    def singles():
        keep, corners = ctx.detect_gftt_refill(5, 40, pts, 7, quality=0.02, min_dist=6.0)
        return [keep, corners, *ctx.lk_track_fb(4, 11, pts)]

    usual = singles()
    trk = ctx.klt_create(**p)
    trk.set_stereo(**st)
    base = ctx.debug_klt_stats()[0]
    for i in range(len(lefts)):
        if i % 2:
            kc.same(trk.step(i - 1, i), want[i][1])
        else:
            ks.same_stereo(trk.step_stereo(max(i - 1, 0), i, 6 + i), want[i][1], wr[i])
        for g, x in zip(singles(), usual):
            assert g.shape == x.shape and g.tobytes() == x.tobytes()
    assert ctx.debug_klt_stats()[0] - base == 3 and ctx.debug_klt_stereo_stats()[0] == 3
    # the setting turned off: the stereo step is refused and the state stays
    held = trk.get_tracks()
    trk.set_stereo(None)
    assert trk.get_stereo() is None
    rc, untouched, _ = ks.raw_step(ctx.h, ctx.lib, trk.id, 4, 5, 11, p["target"])
    assert rc == INVALID and untouched and "no stereo setting" in ks.last_error(ctx)
    kc.same(trk.get_tracks(), held)
    kc.same(trk.step(5, 5)[:3], trk.get_tracks())
    trk.close()


# ---- the many form --------------------------------------------------------------------------------------------------------------------
def _known_states(pmv, w, h):
    """four trackers on frame 1 of the scene, to be stepped onto frame 2: (params, state or None for an empty tracker, stereo setting or
    None for a tracker without a right frame)"""
    out = []
    for target, empty, st in ((1, False, ks.STEREO["fb"]), (64, True, ks.STEREO["fb"]), (150, False, ks.STEREO["fb_off"]), (257, False, None)):
        p, run = kc.scene_run(pmv, w, h, "default", target=target)
        out.append((p, kc.empty_state() if empty else run[1][0], st))
    return out


def _reset(trk, s):
    trk.set_tracks(s["ids"], s["ages"], s["xy"], s["next_id"])


def test_many_equals_the_single_steps_in_either_order(pmv, gpu_ctx_factory):
    w, h = kc.SIZES[0]
    lefts, rts = kc.scene(pmv, w, h), ks.scene_rights(pmv, w, h)
    ctx = ks.make_ctx(gpu_ctx_factory, lefts, rts)
    cases = _known_states(pmv, w, h)
    trks, solo = [], []
    for p, s, st in cases:
        t = ctx.klt_create(**p)
        _reset(t, s)
        if st is None:
            o = t.step(1, 2)
            solo.append(o + (np.zeros((len(o[0]), 2), np.float32), np.zeros(len(o[0]), np.uint8)))
        else:
            t.set_stereo(**st)
            solo.append(t.step_stereo(1, 2, 8))
            ks.same_right(solo[-1][5:], ks.calls_stereo(ctx, 2, 8, solo[-1][2], st))
        trks.append(t)
    assert [int(o[4][0]) for o in solo] == [len(c[1]["ids"]) for c in cases] and solo[1][4][0] == 0 and solo[0][4][0] == 1
    assert all(o[4][7] > 0 for o in solo[:3]) and solo[3][4][7] == 0
    order = list(range(4))
    for perm in (order, order[::-1]):
        for j in perm:
            _reset(trks[j], cases[j][1])
        got = ctx.klt_step_many_stereo([trks[j] for j in perm], [1] * 4, [2] * 4, [8 if cases[j][2] else -1 for j in perm])
        for g, j in zip(got, perm):
            try:
                kc.same(g[:5], solo[j][:5])
                ks.same_right(g[5:], solo[j][5:])
            except AssertionError as e:
                raise AssertionError(f"tracker {j}: {e}") from None
            kc.same(trks[j].get_tracks(), solo[j][:3])
    for t in trks:
        t.close()


def test_many_launches_and_waits_do_not_depend_on_the_group(pmv, gpu_ctx_factory):
    w, h = kc.SIZES[1]
    lefts, rts = kc.scene(pmv, w, h), ks.scene_rights(pmv, w, h)
    ctx = ks.make_ctx(gpu_ctx_factory, lefts, rts)
    p, run = kc.scene_run(pmv, w, h, "f_off", target=20)
    state = run[1][0]
    per_call = {}
    for n_trk in (1, 16):
        trks = [ctx.klt_create(**p) for _ in range(n_trk)]
        for t in trks:
            t.set_stereo(**ks.STEREO["fb"])
            _reset(t, state)
        klt0, many0 = ctx.debug_klt_stats(), ctx.debug_klt_many_stats()
        s0 = ctx.debug_klt_stereo_stats()
        got = ctx.klt_step_many_stereo(trks, [1] * n_trk, [2] * n_trk, [8] * n_trk)
        s1 = ctx.debug_klt_stereo_stats()
        assert ctx.debug_klt_stats()[:3] == klt0[:3] and ctx.debug_klt_many_stats() == many0
        per_call[n_trk] = [s1[k] - s0[k] for k in range(4)]
        for g in got:
            kc.same(g[:4], run[2][1][:4])
            ks.same_right(g[5:], got[0][5:])
        assert got[0][4][7] > 0
        # the same states through the plain many-call: stage 8 is at most 3 launches and no wait
        for t in trks:
            _reset(t, state)
        m0 = ctx.debug_klt_many_stats()
        ctx.klt_step_many(trks, [1] * n_trk, [2] * n_trk)
        m1 = ctx.debug_klt_many_stats()
        assert 0 < per_call[n_trk][3] - (m1[3] - m0[3]) <= 3 and per_call[n_trk][2] == m1[2] - m0[2] == 1
        for t in trks:
            t.close()
    assert per_call[1] == per_call[16] and per_call[1][:2] == [0, 1], per_call
    # and a single stereo step: at most 3 launches over the plain step, the same waits
    t = ctx.klt_create(**p)
    t.set_stereo(**ks.STEREO["fb"])
    _reset(t, state)
    k0 = ctx.debug_klt_stats()
    t.step(1, 2)
    k1 = ctx.debug_klt_stats()
    _reset(t, state)
    s0 = ctx.debug_klt_stereo_stats()
    t.step_stereo(1, 2, 8)
    s1 = ctx.debug_klt_stereo_stats()
    assert s1[0] - s0[0] == 1 and s1[2] - s0[2] == k1[1] - k0[1] == 1 and 0 < (s1[3] - s0[3]) - (k1[2] - k0[2]) <= 3
    assert ctx.debug_klt_stats()[:3] == k1[:3]
    t.close()


def test_refusals_write_nothing_and_keep_the_state(pmv, gpu_ctx_factory):
    w, h = kc.SIZES[0]
    lefts, rts = kc.scene(pmv, w, h)[:2], ks.scene_rights(pmv, w, h)[:2]
    ctx = ks.make_ctx(gpu_ctx_factory, lefts, rts, max_tracks=300, extra_slots=2)   # slots 0, 1 left; 2, 3 right; 4 another size; 5 empty
    small = pmv.synth_sequence(1007, 10, 1, 203, 87, 117.7, 117.7, 101.5, 43.5)[0][0]
    ctx.frame_upload(4, small)
    p, want = kc.scene_run(pmv, w, h, "default")
    a, b = ctx.klt_create(**p), ctx.klt_create(**p)
    for t in (a, b):
        t.set_stereo(**ks.STEREO["fb"])
        t.step(0, 0)
    plain = ctx.klt_create(**p)   # no stereo setting
    plain.step(0, 0)
    held = [t.get_tracks() for t in (a, b, plain)]
    cap = p["target"]

    def unchanged():
        for t, was in zip((a, b, plain), held):
            kc.same(t.get_tracks(), was)

    for what, kw, code, text in (("null right xy", dict(right_slot=3, null="out_rxy"), INVALID, "null"), ("null right status", dict(right_slot=3, null="out_rst"), INVALID, "null"),
                                 ("out of range", dict(right_slot=6), CAPACITY, "slot out of range"), ("negative", dict(right_slot=-1), CAPACITY, "slot out of range"),
                                 ("empty", dict(right_slot=5), INVALID, ""), ("another size", dict(right_slot=4), INVALID, "frame sizes differ")):
        rc, untouched, _ = ks.raw_step(ctx.h, ctx.lib, a.id, 0, 1, cap=cap, **kw)
        assert rc == code and untouched and text in ks.last_error(ctx), (what, rc, untouched, ks.last_error(ctx))
        unchanged()
    rc, untouched, _ = ks.raw_step(ctx.h, ctx.lib, plain.id, 0, 1, 3, cap)
    assert rc == INVALID and untouched and "no stereo setting" in ks.last_error(ctx)
    unchanged()
    ids = [a.id, b.id]
    for what, kw, code, text in (("null right xy", dict(right_slots=[3, 3], null="out_rxy"), INVALID, "null"), ("null right status", dict(right_slots=[3, 3], null="out_rst"), INVALID, "null"),
                                 ("null right slots", dict(right_slots=[3, 3], null="right_slots"), INVALID, "null"),
                                 ("out of range", dict(right_slots=[3, 6]), CAPACITY, "tracker 1 of the group"), ("empty", dict(right_slots=[3, 5]), INVALID, "tracker 1 of the group"),
                                 ("another size", dict(right_slots=[4, 3]), INVALID, "tracker 0 of the group")):
        rc, untouched, _ = ks.raw_many(ctx.h, ctx.lib, ids, [0, 0], [1, 1], stride=cap, **kw)
        assert rc == code and untouched and text in ks.last_error(ctx), (what, rc, untouched, ks.last_error(ctx))
        unchanged()
    rc, untouched, _ = ks.raw_many(ctx.h, ctx.lib, [a.id, plain.id], [0, 0], [1, 1], [3, 3], cap)
    assert rc == INVALID and untouched and "no stereo setting" in ks.last_error(ctx) and "tracker 1 of the group" in ks.last_error(ctx)
    unchanged()
    # the setting: refused values keep the old one
    for kw, text in ((dict(fb_max_dist=2e3), "fb_max_dist"), (dict(fb_max_dist=float("nan")), "fb_max_dist"), (dict(fb_max_dist=float("inf")), "fb_max_dist"),
                     (dict(fb_max_dist=float("-inf")), "fb_max_dist"), (dict(border=65), "border"), (dict(border=-1), "border")):
        with pytest.raises(pmv.PmvError) as e:
            a.set_stereo(**dict(ks.STEREO["fb"], **kw))
        assert e.value.code == INVALID and text in str(e.value) and "pmv_klt_set_stereo" in str(e.value)
        assert a.get_stereo() == (0.5, 1)
    # good calls afterwards: the mono tracker of the group needs no setting
    wr = ks.twin_stereo(lefts[1], rts[1], want[1][1][2], ks.STEREO["fb"])
    ks.same_stereo(a.step_stereo(0, 1, 3), want[1][1], wr)
    got = ctx.klt_step_many_stereo([b, plain], [0, 0], [1, 1], [3, -1])
    ks.same_stereo(got[0], want[1][1], wr)
    kc.same(got[1][:5], want[1][1])
    assert not got[1][6].any()
    for t in (a, b, plain):
        t.close()
