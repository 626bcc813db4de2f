"""pmv_klt_step on the device against its two yardsticks, byte for byte (ids, ages, xy and prev_xy as uint32, counts): calls_step - the
Context's single calls with the policy in numpy - and twin_step - the CPU twins (tests/klt_common.py). What the scenes are there for is
asserted on the twin alone in tests/test_klt_twin.py."""
import ctypes as C

import numpy as np
import pytest

import klt_common as kc

pytestmark = pytest.mark.gpu
INVALID, CAPACITY = -2, -3


def _ctx(pmv, factory, frames, max_tracks=2048):
    h, w = frames[0].shape
    ctx = factory(w, h, n_slots=len(frames), max_tracks=max_tracks)
    kc.upload(ctx, frames)
    return ctx


def _run(ctx, frames, p, want, calls=True):
    """steps over the frames from an empty tracker: each equals the twin's and, composed from the single calls, the yardstick's"""
    trk = ctx.klt_create(**p)
    state = kc.empty_state()
    outs = []
    for i in range(len(frames)):
        got = trk.step(max(i - 1, 0), i)
        kc.same(got, want[i][1])
        if calls:
            state, ref = kc.calls_step(ctx, state, max(i - 1, 0), i, p)
            kc.same(got, ref)
        outs.append(got)
    ids, ages, xy = trk.get_tracks()
    kc.same((ids, ages, xy), outs[-1][:3])
    trk.close()
    return outs


@pytest.mark.parametrize("size", kc.SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("name", list(kc.SETTINGS))
def test_sequences(pmv, gpu_ctx_factory, size, name):
    w, h = size
    frames = kc.scene(pmv, w, h)
    p, want = kc.scene_run(pmv, w, h, name)
    _run(_ctx(pmv, gpu_ctx_factory, frames), frames, p, want)


@pytest.mark.parametrize("target", kc.TARGETS)
def test_targets(pmv, gpu_ctx_factory, target):
    """a lane short of a wavefront, a wavefront, one more, and several"""
    w, h = kc.SIZES[0]
    frames = kc.scene(pmv, w, h)
    p, want = kc.scene_run(pmv, w, h, "default", target=target)
    outs = _run(_ctx(pmv, gpu_ctx_factory, frames), frames, p, want)
    if target == 1:
        assert any(o[4][3] == target and o[4][4] == 0 for o in outs), "no step with target - n3 == 0"


def test_more_than_1024_tracks(pmv, gpu_ctx_factory):
    """two chunks of the compaction, on the 517 x 261 frames with a small radius and min_dist"""
    frames = kc.big_pair(pmv)
    p, want = kc.big_run(pmv)
    outs = _run(_ctx(pmv, gpu_ctx_factory, frames), frames, p, want)
    assert max(o[4][0] for o in outs) > 1024


def test_fewer_than_15_survivors_skip_the_f_stage(pmv, gpu_ctx_factory):
    w, h = kc.SIZES[0]
    frames = kc.scene(pmv, w, h)
    p, want = kc.scene_run(pmv, w, h, "default", target=14)
    outs = _run(_ctx(pmv, gpu_ctx_factory, frames), frames, p, want)
    for o in outs:
        assert o[4][5] == -1 and o[4][6] == 0 and o[4][2] == o[4][1]
    assert outs[-1][4][0] > 0


def test_no_model_empties_and_refills_the_list(pmv, gpu_ctx_factory):
    w, h = kc.SIZES[0]
    frames = kc.scene(pmv, w, h)[:3]
    p = kc.params(f_threshold=kc.NO_MODEL_THRESHOLD)
    want = kc.twin_run(frames, p, ("no-model", w, h))
    outs = _run(_ctx(pmv, gpu_ctx_factory, frames), frames, p, want)
    for o in outs[1:]:
        c = o[4]
        assert c[1] >= 15 and c[5] == 0 and c[2] == 0 and c[3] == 0 and c[4] > 0
        assert (o[1] == 1).all() and np.array_equal(kc.bits(o[2]), kc.bits(o[3]))


def test_set_and_get_tracks(pmv, gpu_ctx_factory):
    w, h = kc.SIZES[0]
    frames = kc.scene(pmv, w, h)
    p, want = kc.scene_run(pmv, w, h, "default")
    ctx = _ctx(pmv, gpu_ctx_factory, frames)
    trk = ctx.klt_create(**p)
    s = want[1][0]   # the twin's state after the step onto frame 1
    xy = s["xy"].copy()
    rng = np.random.default_rng(3)
    moved = rng.choice(len(xy), 40, replace=False)
    xy[moved] += rng.choice([-20.0, 20.0], (40, 2)).astype(np.float32)
    xy = np.clip(xy, 0, [w - 1, h - 1]).astype(np.float32)
    ages = (s["ages"] + 3).astype(np.int32)
    trk.set_tracks(s["ids"], ages, xy, 1000)
    kc.same(trk.get_tracks(), (s["ids"], ages, xy))
    state = dict(ids=s["ids"], ages=ages, xy=xy, next_id=1000)
    _, ref = kc.twin_step(state, frames[1], frames[2], p)
    got = trk.step(1, 2)
    kc.same(got, ref)
    assert got[4][1] < got[4][0] and not set(s["ids"][moved]) <= set(got[0]), "none of the moved tracks was dropped"
    assert got[0][got[4][3]:].tolist() == list(range(1000, 1000 + got[4][4]))
    trk.close()


def test_a_40x40_frame_pair(pmv, gpu_ctx_factory):
    frames = pmv.synth_sequence(1007, 10, 2, 40, 40, 23.2, 23.2, 20, 20)[0]
    p = kc.params(target=20, radius=3, min_dist=3.0, reject_f=False)
    want = kc.twin_run(frames, p, "40x40")
    outs = _run(_ctx(pmv, gpu_ctx_factory, frames), frames, p, want)
    assert outs[0][4][4] > 0


def test_two_trackers_interleaved_equal_their_solo_runs(pmv, gpu_ctx_factory):
    w, h = kc.SIZES[0]
    frames = kc.scene(pmv, w, h)
    pa, wa = kc.scene_run(pmv, w, h, "default")
    pb, wb = kc.scene_run(pmv, w, h, "default", target=63)
    ctx = _ctx(pmv, gpu_ctx_factory, frames)
    a, b = ctx.klt_create(**pa), ctx.klt_create(**pb)
    assert ctx.debug_klt_stats()[3] == 2
    for i in range(len(frames)):
        kc.same(a.step(max(i - 1, 0), i), wa[i][1])
        kc.same(b.step(max(i - 1, 0), i), wb[i][1])
    a.close()
    b.close()
    assert ctx.debug_klt_stats()[3] == 0


def test_single_calls_between_steps(pmv, gpu_ctx_factory):
    """the refill, LK, F and sub-pixel calls on other inputs return their usual bytes between two steps, and the next step is unchanged"""
    import fundamental_common as fc
    w, h = kc.SIZES[0]
    frames = kc.scene(pmv, w, h)
    p, want = kc.scene_run(pmv, w, h, "subpix")
    ctx = _ctx(pmv, gpu_ctx_factory, frames)
    rng = np.random.default_rng(9)
    pts = np.stack([rng.uniform(8, w - 8, 90), rng.uniform(8, h - 8, 90)], axis=1).astype(np.float32)
    p1, p2 = fc.points("scene", 1, 64, 0.3)

    def singles():
        keep, corners = ctx.detect_gftt_refill(5, 40, pts, 7, quality=0.02, min_dist=6.0)
        lk = ctx.lk_track_fb(4, 5, pts)
        found, F, mask, drawn = ctx.find_fundamental_mat(p1, p2, 1.0, 0.99)
        sp = ctx.corner_subpix(5, pts, win=(3, 3), max_iter=20, eps=0.001)
        return [keep, corners, *lk, np.asarray([found, drawn]), F, mask, sp]

    usual = singles()
    trk = ctx.klt_create(**p)
    for i in range(len(frames)):
        kc.same(trk.step(max(i - 1, 0), i), want[i][1])
        for g, x in zip(singles(), usual):
            assert g.shape == x.shape and g.tobytes() == x.tobytes()
    trk.close()


def test_waits_launches_and_the_bus(pmv, gpu_ctx_factory):
    w, h = kc.SIZES[0]
    frames = kc.scene(pmv, w, h)
    ctx = _ctx(pmv, gpu_ctx_factory, frames)
    for name, most in (("f_off", 1), ("default", 2)):
        p, want = kc.scene_run(pmv, w, h, name)
        s0 = ctx.debug_klt_stats()
        _run(ctx, frames, p, want, calls=False)
        s1 = ctx.debug_klt_stats()
        steps, waits, launches = (s1[k] - s0[k] for k in range(3))
        assert steps == len(frames)
        assert waits == steps if most == 1 else steps <= waits <= 2 * steps
        assert 0 < launches <= 12 * steps
    assert ctx.debug_refill_stats()[3] == 0   # no mask byte crossed the bus
    assert ctx.debug_refill_stats()[0] == 0   # and no single refill call was made on the way


def test_destroy_returns_every_byte(pmv, gpu_ctx_factory):
    w, h = kc.SIZES[1]
    frames = kc.scene(pmv, w, h)[:2]
    ctx = _ctx(pmv, gpu_ctx_factory, frames)
    p = kc.params(subpix=True)
    for k in range(2):   # (the first round also makes the context's own scratch, which stays with the context)
        base = pmv.mem_live()
        trk = ctx.klt_create(**p)
        trk.step(0, 0)
        trk.step(0, 1)
        assert pmv.mem_live()[0] > base[0] and pmv.mem_live()[1] > base[1]
        trk.close()
    assert pmv.mem_live() == base


def _raw_step(ctx, tid, prev_slot, cur_slot, cap, out_cap=None, null=False):
    fn = ctx.lib.pmv_klt_step
    fn.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    ids, ages, xy, prev = np.full(cap, -7, np.int32), np.full(cap, -7, np.int32), np.full((cap, 2), -7, np.float32), np.full((cap, 2), -7, np.float32)
    n, counts = np.full(1, -7, np.int32), np.full(8, -7, np.int32)
    rc = fn(ctx.h, tid, prev_slot, cur_slot, None if null else ids.ctypes.data, ages.ctypes.data, xy.ctypes.data, prev.ctypes.data, cap if out_cap is None else out_cap,
            n.ctypes.data, counts.ctypes.data)
    untouched = all((a == -7).all() for a in (ids, ages, xy, prev, n, counts))
    return rc, untouched


def test_refusals_write_nothing_and_keep_the_state(pmv, gpu_ctx_factory):
    w, h = kc.SIZES[0]
    frames = kc.scene(pmv, w, h)[:3]
    ctx = gpu_ctx_factory(w, h, n_slots=5, max_tracks=300)
    kc.upload(ctx, frames)
    small = pmv.synth_sequence(1007, 10, 1, 203, 87, 117.7, 117.7, 101.5, 43.5)[0][0]
    ctx.frame_upload(3, small)   # slot 3: another size; slot 4: empty
    p, want = kc.scene_run(pmv, w, h, "default")
    trk = ctx.klt_create(**p)
    kc.same(trk.step(0, 0), want[0][1])
    held = trk.get_tracks()
    cap = p["target"]
    for args, code in (((trk.id + 1, 0, 1, cap), INVALID), ((-1, 0, 1, cap), INVALID), ((trk.id, 0, 1, cap, cap - 1), CAPACITY), ((trk.id, 0, 4, cap), INVALID),
                       ((trk.id, 4, 1, cap), INVALID), ((trk.id, 0, 3, cap), INVALID), ((trk.id, 0, 5, cap), CAPACITY), ((trk.id, -1, 1, cap), CAPACITY)):
        rc, untouched = _raw_step(ctx, *args)
        assert rc == code and untouched, (args, rc)
        kc.same(trk.get_tracks(), held)
    rc, untouched = _raw_step(ctx, trk.id, 0, 1, cap, null=True)
    assert rc == INVALID and untouched
    # set_tracks: n above the target, a NaN coordinate
    ids, ages, xy = held
    big = np.zeros(cap + 1, np.int32)
    with pytest.raises(pmv.PmvError) as e:
        trk.set_tracks(big, big, np.zeros((cap + 1, 2), np.float32), 0)
    assert e.value.code == CAPACITY
    bad = xy.copy()
    bad[3, 1] = np.nan
    with pytest.raises(pmv.PmvError) as e:
        trk.set_tracks(ids, ages, bad, 0)
    assert e.value.code == INVALID and "track 3" in str(e.value)
    kc.same(trk.get_tracks(), held)
    # create: one bad field per borrowed check, the tracker's own fields, a target beyond the context
    for over, code, text in ((dict(f_threshold=0.0), INVALID, "threshold"), (dict(f_confidence=1.0), INVALID, "confidence"), (dict(quality=0.0), INVALID, "quality"),
                             (dict(block_size=16), INVALID, "block_size"), (dict(subpix=True, subpix_win=(0, 5)), INVALID, "win"),
                             (dict(subpix=True, subpix_max_iter=0), INVALID, "max_iter"), (dict(radius=256), INVALID, "radius"), (dict(border=65), INVALID, "border"),
                             (dict(fb_max_dist=float("nan")), INVALID, "fb_max_dist"), (dict(target=0), INVALID, "target"), (dict(target=301), CAPACITY, "target")):
        with pytest.raises(pmv.PmvError) as e:
            ctx.klt_create(**kc.params(**over))
        assert e.value.code == code and text in str(e.value) and "pmv_klt_create" in str(e.value), (over, str(e.value))
    # a 17th tracker
    more = [ctx.klt_create(**kc.params(target=8)) for _ in range(pmv.KLT_MAX_TRACKERS - 1)]
    with pytest.raises(pmv.PmvError) as e:
        ctx.klt_create(**kc.params(target=8))
    assert e.value.code == CAPACITY
    gone = more[0].id
    for t in more:
        t.close()
    fn = ctx.lib.pmv_klt_destroy
    fn.argtypes = [C.c_void_p, C.c_int]
    assert fn(ctx.h, gone) == INVALID and fn(ctx.h, 99) == INVALID
    # a good step afterwards works
    kc.same(trk.get_tracks(), held)
    kc.same(trk.step(0, 1), want[1][1])
    kc.same(trk.step(1, 2), want[2][1])
    trk.close()
