"""The tracker step with a prediction (pmv_klt_set_prediction) on the device, byte for byte against the twin composition of
tests/predict_common.py (ids, ages, xy and prev_xy as uint32, counts) and its {consumed, joined, succ, fell_back}: every step form, the
fall-back and its boundary, lists that are unsorted, partial and partly unprojectable, one lane to two 1024-chunks of tracks, the life of a
prediction, and the launches and waits it may cost. What the scenes are there for is asserted on the twin in tests/test_klt_predict_twin.py."""
import numpy as np
import pytest

import klt_common as kc
import klt_observe_common as ko
import klt_stereo_common as ks
import predict_common as pc

pytestmark = pytest.mark.gpu
INVALID, CAPACITY = -2, -3
MIN_SUCC = 10
_ctxs = {}


def _ctx(factory, case, lk=(32, 4), extra=()):
    """a context with the case's frames in slots 0 .., then `extra` frames, under the LK setting lk; shared per (case, lk, number of extras)"""
    key, frames = case[0], case[1]
    k = (key, lk, len(extra))
    if k not in _ctxs:
        h, w = frames[0].shape
        ctx = factory(w, h, n_slots=len(frames) + len(extra), max_tracks=2048)
        if lk != (32, 4):
            ctx.set_lk_params(win=lk[0], max_level=lk[1])
        kc.upload(ctx, frames)
        if len(extra):
            kc.upload(ctx, extra, first_slot=len(frames))
        _ctxs[k] = (ctx, ctx.camera_create(**case[3]))
    return _ctxs[k]


def _tracker(ctx, case):
    """a tracker of the case's parameters holding the case's state"""
    s0 = pc.state_of(case)
    trk = ctx.klt_create(**case[2])
    trk.set_tracks(s0["ids"], s0["ages"], s0["xy"], s0["next_id"])
    return trk


def _predict(trk, cam_id, pred):
    trk.set_prediction(cam_id, pred["ids"], pred["xyz"], top_level=pred["top_level"], back_top_level=pred["back_top_level"], min_succ=pred["min_succ"])


def _result(trk):
    r = trk.get_prediction_result()
    return (r["consumed"], r["joined"], r["succ"], r["fell_back"])


def _step_and_check(trk, cam_id, case, pred, lk=(32, 4)):
    """one consuming step onto frame 1: the twin's bytes and result; returns (the twin's new state, the outputs)"""
    if pred is not None:
        _predict(trk, cam_id, pred)
    new, want, res, _ = pc.predicted_step(case, pred, lk)
    got = trk.step(0, 1)
    kc.same(got, want)
    assert _result(trk) == res, (_result(trk), res)
    return new, got


@pytest.mark.parametrize("size", kc.SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("lk", [(32, 4), (21, 3)], ids=lambda v: "win%d-level%d" % v)
@pytest.mark.parametrize("name", ["default", "fb_off"])
def test_a_predicted_step_and_the_plain_step_after_it(pmv, gpu_ctx_factory, size, lk, name):
    """the consuming step, then one-shot: the next step is the plain one, and get_prediction_result says consumed = 0"""
    case = pc.scene_case(pmv, *size, **kc.SETTINGS[name])
    ctx, cam = _ctx(gpu_ctx_factory, case, lk)
    trk = _tracker(ctx, case)
    assert _result(trk) == (0, 0, 0, 0)
    pred = pc.good_prediction(case, lk)
    new, got = _step_and_check(trk, cam, case, pred, lk)
    plain = pc.plain_step(case, lk)[1]
    assert not all(np.array_equal(kc.bits(g), kc.bits(x)) for g, x in zip(got, plain)), "the prediction changed nothing"
    _, frames, p, _ = case
    _, want2, res2, _ = pc.twin_predicted_step(new, frames[1], frames[2], p, None, lk)
    kc.same(trk.step(1, 2), want2)
    assert _result(trk) == res2 == (0, 0, 0, 0)
    # other settings of the prediction, from the same state
    s0 = pc.state_of(case)
    for setting in (dict(top_level=0, back_top_level=0), dict(top_level=4, back_top_level=-1), dict(top_level=2, back_top_level=1, min_succ=0)):
        trk.set_tracks(s0["ids"], s0["ages"], s0["xy"], s0["next_id"])
        _step_and_check(trk, cam, case, dict(pred, **setting), lk)
    trk.close()


@pytest.mark.parametrize("size", kc.SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("lk", [(32, 4), (21, 3)], ids=lambda v: "win%d-level%d" % v)
def test_the_fall_back_and_its_boundary(pmv, gpu_ctx_factory, size, lk):
    case = pc.scene_case(pmv, *size)
    ctx, cam = _ctx(gpu_ctx_factory, case, lk)
    s0 = pc.state_of(case)
    trk = _tracker(ctx, case)
    # every guess out of the frame, the backward pass on every level: the plain step's bytes
    _, got = _step_and_check(trk, cam, case, pc.far_prediction(case, back_top_level=-1), lk)
    kc.same(got, pc.plain_step(case, lk)[1])
    assert _result(trk) == (1, len(s0["ids"]), 0, 1)
    # ... with the backward pass capped, and with min_succ = 0, which never falls back
    for setting in (dict(back_top_level=0), dict(min_succ=0)):
        trk.set_tracks(s0["ids"], s0["ages"], s0["xy"], s0["next_id"])
        _step_and_check(trk, cam, case, pc.far_prediction(case, **setting), lk)
    # exactly min_succ - 1 and exactly min_succ successes
    pick = pc.boundary_tracks(case, lk, MIN_SUCC)
    for k, fell in ((MIN_SUCC - 1, 1), (MIN_SUCC, 0)):
        trk.set_tracks(s0["ids"], s0["ages"], s0["xy"], s0["next_id"])
        _step_and_check(trk, cam, case, pc.partial_prediction(case, lk, pick[:k], min_succ=MIN_SUCC), lk)
        assert _result(trk) == (1, len(s0["ids"]), k, fell)
    trk.close()


def test_lists_unsorted_partial_and_partly_unprojectable(pmv, gpu_ctx_factory):
    case = pc.scene_case(pmv, *kc.SIZES[0])
    ctx, cam = _ctx(gpu_ctx_factory, case)
    s0 = pc.state_of(case)
    n0 = len(s0["ids"])
    good = pc.good_prediction(case)
    rng = np.random.default_rng(17)
    keep = rng.permutation(n0)[: 2 * n0 // 3]                       # a third of the tracks has no entry, the rest in any order
    ids, xyz = good["ids"][keep].copy(), good["xyz"][keep].copy()
    bad = {0: (0.1, 0.2, 0.0), 1: (0.1, 0.2, -3.0), 2: (np.nan, 0.0, 1.0), 3: (0.0, np.inf, 1.0), 4: (1e300, 0.0, 1e-300), 5: (9e3, 0.0, 1.0)}
    for j, v in bad.items():
        xyz[j] = v
    strangers = np.arange(5000, 5040, dtype=np.int32)                # ids that no track has, below and above the tracks' own, and a negative one
    ids = np.concatenate([ids, strangers, [-3]]).astype(np.int32)
    xyz = np.concatenate([xyz, pc.camera_points(41, seed=2)])
    order = rng.permutation(len(ids))
    pred = dict(good, ids=ids[order], xyz=xyz[order])
    trk = _tracker(ctx, case)
    _step_and_check(trk, cam, case, pred)
    assert _result(trk)[1] == len(keep) - len(bad)
    # the order of the list changes nothing, and neither does a list of one entry or of strangers only
    for sub in (dict(pred, ids=ids, xyz=xyz), dict(good, ids=good["ids"][7:8], xyz=good["xyz"][7:8]), dict(good, ids=strangers, xyz=xyz[-41:-1])):
        trk.set_tracks(s0["ids"], s0["ages"], s0["xy"], s0["next_id"])
        _step_and_check(trk, cam, case, sub)
    assert _result(trk)[:2] == (1, 0)
    trk.close()


@pytest.mark.parametrize("target", [1, 65, "BIG"])
def test_targets(pmv, gpu_ctx_factory, target):
    """one track, a lane more than a wavefront, and the 1500-track case that takes two 1024-chunks in the join kernel"""
    case = pc.big_case(pmv) if target == "BIG" else pc.scene_case(pmv, *kc.SIZES[0], target=target)
    ctx, cam = _ctx(gpu_ctx_factory, case)
    s0 = pc.state_of(case)
    assert len(s0["ids"]) > 1024 if target == "BIG" else len(s0["ids"]) == target
    trk = _tracker(ctx, case)
    pred = pc.good_prediction(case, min_succ=1)
    _step_and_check(trk, cam, case, pred)
    assert _result(trk)[1] == len(s0["ids"]) and _result(trk)[3] == 0
    trk.set_tracks(s0["ids"], s0["ages"], s0["xy"], s0["next_id"])
    _, got = _step_and_check(trk, cam, case, pc.far_prediction(case, back_top_level=-1, min_succ=1))
    kc.same(got, pc.plain_step(case)[1])
    trk.close()


def test_an_empty_tracker_consumes_its_prediction(pmv, gpu_ctx_factory):
    case = pc.scene_case(pmv, *kc.SIZES[0])
    ctx, cam = _ctx(gpu_ctx_factory, case)
    trk = ctx.klt_create(**case[2])
    _predict(trk, cam, pc.good_prediction(case))
    _, frames, p, _ = case
    _, want = kc.twin_step(kc.empty_state(), frames[0], frames[0], p)
    kc.same(trk.step(0, 0), want)
    assert _result(trk) == (1, 0, 0, 0)
    kc.same(trk.step(0, 1), pc.plain_step(case)[1])
    assert _result(trk) == (0, 0, 0, 0)
    trk.close()


def test_stereo_and_observing_steps(pmv, gpu_ctx_factory):
    """stages 8 and 9 are functions of the list the step returns: with a prediction they see the predicted step's list"""
    size = kc.SIZES[0]
    case = pc.scene_case(pmv, *size)
    _, frames, p, camera = case
    rts = ks.scene_rights(pmv, *size)
    ctx, cam = _ctx(gpu_ctx_factory, case, extra=rts[:2])
    right_slot = len(frames) + 1
    s0 = pc.state_of(case)
    pred = pc.good_prediction(case)
    _, want, res, _ = pc.predicted_step(case, pred)
    trk = _tracker(ctx, case)
    st = ks.STEREO["fb"]
    trk.set_stereo(**st)
    trk.set_observe(cam, dt=ko.DT)
    _predict(trk, cam, pred)
    got = trk.step_stereo(0, 1, right_slot)
    want_right = ks.twin_stereo(frames[1], rts[1], want[2], st)
    ks.same_stereo(got, want, want_right)
    assert _result(trk) == res and int(want_right[1].sum()) > 0
    ko.same_observations(trk.get_observations(), ko.expected(camera, ko.DT, want))
    # the observing single step, and the plain stereo step after a consumed prediction
    trk.set_tracks(s0["ids"], s0["ages"], s0["xy"], s0["next_id"])
    _step_and_check(trk, cam, case, pred)
    ko.same_observations(trk.get_observations(), ko.expected(camera, ko.DT, want))
    trk.set_tracks(s0["ids"], s0["ages"], s0["xy"], s0["next_id"])
    plain = pc.plain_step(case)[1]
    ks.same_stereo(trk.step_stereo(0, 1, right_slot), plain, ks.twin_stereo(frames[1], rts[1], plain[2], st))
    assert _result(trk) == (0, 0, 0, 0)
    trk.close()


def _group(ctx, cam, case, preds):
    """trackers holding the case's state (None in `preds`: no prediction; "empty": an empty tracker with a prediction it consumes)"""
    trks = []
    for pr in preds:
        if isinstance(pr, str):
            t = ctx.klt_create(**case[2])
            _predict(t, cam, pc.good_prediction(case))
        else:
            t = _tracker(ctx, case)
            if pr is not None:
                _predict(t, cam, pr)
        trks.append(t)
    return trks


def test_a_group_of_four(pmv, gpu_ctx_factory):
    """one predicted, one falling back, one without a prediction, one empty - and the same mixed with stereo; every tracker its own twin step"""
    size = kc.SIZES[0]
    case = pc.scene_case(pmv, *size)
    _, frames, p, _ = case
    rts = ks.scene_rights(pmv, *size)
    ctx, cam = _ctx(gpu_ctx_factory, case, extra=rts[:2])
    preds = [pc.good_prediction(case), pc.far_prediction(case), None, "empty"]
    wants = [pc.predicted_step(case, preds[0]), pc.predicted_step(case, preds[1]), pc.plain_step(case)]
    empty = kc.twin_step(kc.empty_state(), frames[1], frames[1], p)[1]
    for order in ((0, 1, 2, 3), (3, 2, 1, 0)):
        trks = _group(ctx, cam, case, [preds[k] for k in order])
        got = ctx.klt_step_many(trks, [0] * 4, [1] * 4)
        for j, k in enumerate(order):
            kc.same(got[j], empty if k == 3 else wants[k][1])
            assert _result(trks[j]) == ((1, 0, 0, 0) if k == 3 else wants[k][2]), (order, j, _result(trks[j]))
        assert wants[0][2][3] == 0 and wants[1][2][3] == 1
        # the next many-call has nothing to consume
        got = ctx.klt_step_many(trks, [1] * 4, [1] * 4)
        assert all(_result(t) == (0, 0, 0, 0) for t in trks)
        for t in trks:
            t.close()
    # settings that differ from tracker to tracker, and stage 8 behind them
    settings = [dict(top_level=0, back_top_level=0), dict(top_level=2, back_top_level=-1, min_succ=200), dict(top_level=1, back_top_level=1, min_succ=0)]
    gp = [dict(pc.good_prediction(case, seed=3 + k), **s) for k, s in enumerate(settings)]
    trks = _group(ctx, cam, case, gp)
    st = ks.STEREO["fb"]
    for t in trks:
        t.set_stereo(**st)
    got = ctx.klt_step_many_stereo(trks, [0] * 3, [1] * 3, [len(frames) + 1, -1, len(frames) + 1])
    for j in range(3):
        _, want, res, _ = pc.predicted_step(case, gp[j])
        assert _result(trks[j]) == res
        if j == 1:
            assert res[3] == 1, "min_succ = 200 of 150 tracks always falls back"
            kc.same(got[j][:5], want)
            assert not got[j][6].any()
        else:
            ks.same_stereo(got[j], want, ks.twin_stereo(frames[1], rts[1], want[2], st))
    for t in trks:
        t.close()


def test_refusals_keep_what_is_pending(pmv, gpu_ctx_factory):
    """a refused step and a refused pmv_klt_set_prediction leave the pending prediction as it is; set_tracks leaves it pending; NULL clears
    it; its camera cannot be destroyed while it is pending"""
    case = pc.scene_case(pmv, *kc.SIZES[0])
    ctx, cam = _ctx(gpu_ctx_factory, case)
    s0 = pc.state_of(case)
    n_slots = len(case[1])
    pred = pc.good_prediction(case)
    other = ctx.camera_create(**case[3])
    trk = ctx.klt_create(**case[2])
    _predict(trk, other, pred)                                        # set before the tracks: the join is by id
    trk.set_tracks(s0["ids"], s0["ages"], s0["xy"], s0["next_id"])
    for bad_step in (lambda: trk.step(0, n_slots), lambda: trk.step(n_slots, 1), lambda: trk.step_stereo(0, 1, 1)):
        with pytest.raises(pmv.PmvError):
            bad_step()
    ids, xyz = pred["ids"], pred["xyz"]
    dup = ids.copy()
    dup[5] = dup[90]
    for what, kw, code, text in (("a duplicate id", dict(ids=dup), INVALID, "named twice"), ("top_level 5", dict(top_level=5), INVALID, "top_level"),
                                 ("top_level -1", dict(top_level=-1), INVALID, "top_level"), ("back_top_level -2", dict(back_top_level=-2), INVALID, "back_top_level"),
                                 ("back_top_level 5", dict(back_top_level=5), INVALID, "back_top_level"), ("min_succ -1", dict(min_succ=-1), INVALID, "min_succ"),
                                 ("camera 15", dict(cam_id=15), INVALID, "camera"), ("camera -1", dict(cam_id=-1), INVALID, "camera")):
        a = dict(cam_id=other, ids=ids, xyz=np.zeros_like(xyz), top_level=0, back_top_level=0, min_succ=0)
        a.update(kw)
        with pytest.raises(pmv.PmvError) as e:
            trk.set_prediction(**a)
        assert e.value.code == code and text in str(e.value) and "pmv_klt_set_prediction" in str(e.value), (what, str(e.value))
    many = np.arange(8193, dtype=np.int32)
    with pytest.raises(pmv.PmvError) as e:
        trk.set_prediction(other, many, np.ones((8193, 3)))
    assert e.value.code == CAPACITY and "PMV_REFILL_MAX_TRACKS" in str(e.value)
    with pytest.raises(pmv.PmvError) as e:
        ctx.camera_destroy(other)
    assert e.value.code == INVALID and "pending prediction" in str(e.value)
    # the prediction given first is still the pending one
    _, want, res, _ = pc.predicted_step(case, pred)
    kc.same(trk.step(0, 1), want)
    assert _result(trk) == res
    ctx.camera_destroy(other)                                          # consumed: the camera is free
    # NULL clears; a second prediction replaces the first
    trk.set_tracks(s0["ids"], s0["ages"], s0["xy"], s0["next_id"])
    _predict(trk, cam, pc.far_prediction(case))
    trk.set_prediction(None)
    kc.same(trk.step(0, 1), pc.plain_step(case)[1])
    assert _result(trk) == (0, 0, 0, 0)
    trk.set_tracks(s0["ids"], s0["ages"], s0["xy"], s0["next_id"])
    _predict(trk, cam, pc.far_prediction(case))
    _step_and_check(trk, cam, case, pred)
    trk.close()


def test_launches_and_waits(pmv, gpu_ctx_factory):
    """pmv_debug_klt_stats / _many_stats: with a prediction at most 2 launches more than the same plain call and no wait more, for a single
    step and for groups of 1 and 4; without one exactly the plain call's"""
    case = pc.scene_case(pmv, *kc.SIZES[0])
    ctx, cam = _ctx(gpu_ctx_factory, case)
    s0 = pc.state_of(case)
    pred = pc.good_prediction(case)

    def single(with_pred):
        trk = _tracker(ctx, case)
        if with_pred:
            _predict(trk, cam, pred)
        a = ctx.debug_klt_stats()
        trk.step(0, 1)
        b = ctx.debug_klt_stats()
        trk.close()
        return b[0] - a[0], b[1] - a[1], b[2] - a[2]

    plain, again, predicted = single(False), single(False), single(True)
    print("single step (steps, waits, launches): plain", plain, "predicted", predicted)
    assert plain == again and plain[0] == 1
    assert predicted[1] == plain[1] and plain[2] < predicted[2] <= plain[2] + 2
    for n_trk in (1, 4):
        def many(preds):
            trks = _group(ctx, cam, case, preds)
            a = ctx.debug_klt_many_stats()
            ctx.klt_step_many(trks, [0] * n_trk, [1] * n_trk)
            b = ctx.debug_klt_many_stats()
            for t in trks:
                t.close()
            return b[0] - a[0], b[2] - a[2], b[3] - a[3]
        plain, again = many([None] * n_trk), many([None] * n_trk)
        predicted = many([pred] + [None, pc.far_prediction(case), pred][: n_trk - 1])
        print("group of", n_trk, "(calls, waits, launches): plain", plain, "predicted", predicted)
        assert plain == again and plain[0] == 1
        assert predicted[1] == plain[1] and plain[2] < predicted[2] <= plain[2] + 2
