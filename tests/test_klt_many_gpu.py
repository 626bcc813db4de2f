"""pmv_klt_step_many on the device: every tracker of every many-call equals its solo run on the CPU twin byte for byte (ids, ages, xy and
prev_xy as uint32, counts). What the groups are there for is asserted on the twin alone in tests/test_klt_many_twin.py."""
import numpy as np
import pytest

import klt_common as kc
import klt_many_common as mc

pytestmark = pytest.mark.gpu
SIZE_IDS = dict(ids=lambda s: "%dx%d" % s)


@pytest.mark.parametrize("size", kc.SIZES, **SIZE_IDS)
def test_mixed_targets(pmv, gpu_ctx_factory, size):
    """F skipped for two trackers and run for two in the same call; one tracker has nothing to refill"""
    w, h = size
    members = [mc.forward_member(pmv, w, h, "default", target=t) for t in (1, 14, 63, 150)]
    outs = mc.run_group(mc.make_ctx(gpu_ctx_factory, kc.scene(pmv, w, h)), members)
    if size == kc.SIZES[0]:
        for got in outs[1:]:
            assert [int(g[4][5]) for g in got] == [-1, -1, 1, 1]
            assert got[0][4][3] == 1 and got[0][4][4] == 0


@pytest.mark.parametrize("size", kc.SIZES, **SIZE_IDS)
def test_per_tracker_policy(pmv, gpu_ctx_factory, size):
    """forward and reversed frames, the backward pass and F on and off, another border and radius: one call per frame"""
    w, h = size
    members = [mc.forward_member(pmv, w, h, "default"), mc.backward_member(pmv, w, h, "fb_off"), mc.backward_member(pmv, w, h, "f_off"),
               mc.forward_member(pmv, w, h, "default", border=8, radius=5)]
    mc.run_group(mc.make_ctx(gpu_ctx_factory, kc.scene(pmv, w, h)), members)


@pytest.mark.parametrize("size", kc.SIZES, **SIZE_IDS)
def test_no_model_next_to_a_model(pmv, gpu_ctx_factory, size):
    w, h = size
    members = [mc.no_model_run(pmv, w, h) + (mc.forward,), mc.forward_member(pmv, w, h, "default")]
    outs = mc.run_group(mc.make_ctx(gpu_ctx_factory, kc.scene(pmv, w, h)), members)
    for got in outs[1:]:
        c = got[0][4]
        assert c[5] == 0 and c[2] == 0 and c[3] == 0 and c[4] > 0 and (got[0][1] == 1).all()
        assert got[1][4][5] == 1


def test_late_joiner_and_alternation(pmv, gpu_ctx_factory):
    """A from frame 0, stepped by step and klt_step_many in turn; B is created before frame 3, an empty list next to a full one; the single
    calls between the steps return their usual bytes"""
    import fundamental_common as fc
    w, h = kc.SIZES[0]
    frames = kc.scene(pmv, w, h)
    pa, wa = kc.scene_run(pmv, w, h, "subpix")
    pb, wb = mc.late_run(pmv, w, h, "subpix")
    ctx = mc.make_ctx(gpu_ctx_factory, frames)
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
    a, b = ctx.klt_create(**pa), None
    for i in range(len(frames)):
        if i == 3:
            b = ctx.klt_create(**pb)
        ps, cs = mc.forward(i)
        if i % 2 == 0:
            kc.same(a.step(ps, cs), wa[i][1])
            if b is not None:
                kc.same(b.step(max(ps, 3), cs), wb[i - 3][1])
        else:
            group = [a] if b is None else [a, b]
            got = ctx.klt_step_many(group, [ps, max(ps, 3)][:len(group)], [cs] * len(group))
            kc.same(got[0], wa[i][1])
            if b is not None:
                if i == 3:
                    assert got[1][4][0] == 0 and got[0][4][0] > 0
                kc.same(got[1], wb[i - 3][1])
        for g, x in zip(singles(), usual):
            assert g.shape == x.shape and g.tobytes() == x.tobytes()
    a.close()
    b.close()


@pytest.mark.parametrize("name,size", [("subpix", kc.SIZES[0]), ("block5_harris", kc.SIZES[0]), ("subpix", kc.SIZES[1])],
                         ids=lambda v: v if isinstance(v, str) else "%dx%d" % v)
def test_launch_wide_settings(pmv, gpu_ctx_factory, name, size):
    w, h = size
    members = [mc.forward_member(pmv, w, h, name), mc.forward_member(pmv, w, h, name, target=63)]
    outs = mc.run_group(mc.make_ctx(gpu_ctx_factory, kc.scene(pmv, w, h)), members)
    assert all(g[4][4] > 0 for g in outs[0])


def test_more_than_1024_tracks_next_to_150(pmv, gpu_ctx_factory):
    """two chunks of the compaction in one workgroup and a short list in the next"""
    frames = kc.big_pair(pmv)
    pa, wa = kc.big_run(pmv)
    pb = kc.params(**dict(kc.BIG, target=150))
    wb = kc.twin_run(frames, pb, "many-big-150")
    outs = mc.run_group(mc.make_ctx(gpu_ctx_factory, frames, max_tracks=2048), [(pa, wa, mc.forward), (pb, wb, mc.forward)], steps=len(frames))
    assert max(got[0][4][0] for got in outs) > 1024 and max(got[1][4][0] for got in outs) == 150


def test_sixteen_trackers(pmv, gpu_ctx_factory):
    w, h = kc.SIZES[1]
    sets = [mc.forward_member(pmv, w, h, "default"), mc.forward_member(pmv, w, h, "default", target=63), mc.forward_member(pmv, w, h, "fb_off"),
            mc.forward_member(pmv, w, h, "f_off")]
    members = [sets[j % 4] for j in range(16)]
    outs = mc.run_group(mc.make_ctx(gpu_ctx_factory, kc.scene(pmv, w, h)), members)
    for got in outs:
        for j in range(4, 16):
            kc.same(got[j], got[j % 4])


@pytest.mark.parametrize("n_trk", [1, 3, 16])
def test_launches_waits_and_the_bus(pmv, gpu_ctx_factory, n_trk):
    w, h = kc.SIZES[1]
    ctx = mc.make_ctx(gpu_ctx_factory, kc.scene(pmv, w, h))
    calls = trackers_stepped = 0
    for names, f_anywhere in ((["f_off"], False), (["default", "f_off", "fb_off"], True)):
        members = [mc.forward_member(pmv, w, h, names[j % len(names)]) for j in range(n_trk)]
        trackers = [ctx.klt_create(**m[0]) for m in members]
        base_klt, base_refill = ctx.debug_klt_stats(), ctx.debug_refill_stats()
        for i in range(kc.N_FRAMES):
            s0 = ctx.debug_klt_many_stats()
            mc.step_group(ctx, trackers, members, i)
            s1 = ctx.debug_klt_many_stats()
            d = [s1[k] - s0[k] for k in range(4)]
            assert d[0] == 1 and d[1] == n_trk
            assert 0 < d[3] <= 12, d
            assert d[2] == 1 if not f_anywhere else 1 <= d[2] <= 2, d
            if f_anywhere and i > 0:
                assert d[2] == 2   # (some tracker has reject_f and 15 tracks)
            calls += 1
            trackers_stepped += n_trk
        assert ctx.debug_klt_stats()[0:3] == base_klt[0:3]
        assert ctx.debug_refill_stats() == base_refill
        for t in trackers:
            t.close()
    assert ctx.debug_klt_many_stats()[0:2] == [calls, trackers_stepped]
    assert ctx.debug_refill_stats()[0] == 0 and ctx.debug_refill_stats()[3] == 0


def test_refusals_are_all_or_nothing(pmv, gpu_ctx_factory):
    w, h = kc.SIZES[0]
    frames = kc.scene(pmv, w, h)[:3]
    ctx = gpu_ctx_factory(w, h, n_slots=5, max_tracks=300)
    kc.upload(ctx, frames)
    small = pmv.synth_sequence(1007, 10, 1, 203, 87, 117.7, 117.7, 101.5, 43.5)[0][0]
    ctx.frame_upload(3, small)   # slot 3: another size; slot 4: empty
    members = [mc.forward_member(pmv, w, h, "default"), mc.forward_member(pmv, w, h, "default", target=63), mc.forward_member(pmv, w, h, "f_off")]
    trk = [ctx.klt_create(**m[0]) for m in members]
    odd = {"min_dist": ctx.klt_create(**kc.params(min_dist=9.0)), "subpix": ctx.klt_create(**kc.params(subpix=True))}
    sp = [ctx.klt_create(**kc.params(subpix=True)), ctx.klt_create(**kc.params(subpix=True, subpix_win=(4, 4)))]
    mc.step_group(ctx, trk, members, 0)
    for t in list(odd.values()) + sp:
        t.step(0, 0)
    everyone = trk + list(odd.values()) + sp
    held = [t.get_tracks() for t in everyone]
    ids = [t.id for t in trk]
    free_id = next(k for k in range(pmv.KLT_MAX_TRACKERS) if k not in [t.id for t in everyone])
    cases = [
        ("a duplicate id", dict(ids=[ids[0], ids[1], ids[0]], prev_slots=[0] * 3, cur_slots=[1] * 3, stride=150), mc.INVALID, "twice"),
        ("an unknown id", dict(ids=[ids[0], free_id], prev_slots=[0] * 2, cur_slots=[1] * 2, stride=150), mc.INVALID, "does not exist"),
        ("n_trk 0", dict(ids=ids, prev_slots=[0] * 3, cur_slots=[1] * 3, stride=150, n_trk=0), mc.INVALID, "n_trk"),
        ("n_trk 17", dict(ids=ids, prev_slots=[0] * 3, cur_slots=[1] * 3, stride=150, n_trk=17), mc.CAPACITY, "n_trk"),
        ("a null array", dict(ids=ids, prev_slots=[0] * 3, cur_slots=[1] * 3, stride=150, null="out_xy"), mc.INVALID, "null"),
        ("null ids", dict(ids=ids, prev_slots=[0] * 3, cur_slots=[1] * 3, stride=150, null="ids"), mc.INVALID, "null"),
        ("out_stride", dict(ids=ids, prev_slots=[0] * 3, cur_slots=[1] * 3, stride=149), mc.CAPACITY, "out_stride"),
        ("min_dist", dict(ids=[ids[0], ids[1], odd["min_dist"].id], prev_slots=[0] * 3, cur_slots=[1] * 3, stride=150), mc.INVALID, "tracker 2 of the group"),
        ("subpix", dict(ids=[ids[0], odd["subpix"].id, ids[1]], prev_slots=[0] * 3, cur_slots=[1] * 3, stride=150), mc.INVALID, "tracker 1 of the group"),
        ("subpix_params", dict(ids=[sp[0].id, sp[1].id], prev_slots=[0] * 2, cur_slots=[1] * 2, stride=150), mc.INVALID, "subpix_params"),
        ("another frame size", dict(ids=ids, prev_slots=[0, 0, 3], cur_slots=[1, 1, 3], stride=150), mc.INVALID, "tracker 2 of the group"),
        ("an empty slot", dict(ids=ids, prev_slots=[0] * 3, cur_slots=[1, 1, 4], stride=150), mc.INVALID, "tracker 2 of the group"),
    ]
    for what, kw, code, text in cases:
        rc, untouched = mc.raw_many(ctx, **kw)
        assert rc == code and untouched, (what, rc, untouched)
        assert text in mc.last_error(ctx), (what, mc.last_error(ctx))
        if what in ("min_dist", "subpix"):
            assert ("gftt.min_dist" if what == "min_dist" else "subpix") in mc.last_error(ctx)
        for t, was in zip(everyone, held):
            kc.same(t.get_tracks(), was)
    # out_prev_xy may be null, and the following many-calls equal the twin
    rc, _ = mc.raw_many(ctx, ids=ids, prev_slots=[0] * 3, cur_slots=[1] * 3, stride=150, null="out_prev")
    assert rc == 0
    for t, m in zip(trk, members):
        kc.same(t.get_tracks(), m[1][1][1][:3])
    mc.step_group(ctx, trk, members, 2)
    for t in everyone:
        t.close()


def test_closing_a_round_returns_every_byte(pmv, gpu_ctx_factory):
    w, h = kc.SIZES[1]
    ctx = mc.make_ctx(gpu_ctx_factory, kc.scene(pmv, w, h)[:2])
    ps = [kc.params(subpix=True), kc.params(subpix=True, target=63, reject_f=False)]
    for k in range(2):   # (the first round also makes the context's scratch and the group's blocks, which stay with the context)
        base = pmv.mem_live()
        trackers = [ctx.klt_create(**p) for p in ps]
        ctx.klt_step_many(trackers, [0, 0], [0, 0])
        ctx.klt_step_many(trackers, [0, 0], [1, 1])
        assert pmv.mem_live()[0] > base[0] and pmv.mem_live()[1] > base[1]
        for t in trackers:
            t.close()
    assert pmv.mem_live() == base
