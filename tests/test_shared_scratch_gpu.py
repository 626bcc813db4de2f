"""The calls that share the context's frame-detector scratch and its sub-pixel weight table, interleaved on ONE context: the whole-frame
detector, the masked refill, the sub-pixel refinement and the KLT steps in their single, many and stereo forms. Every output of every call is
compared, byte for byte, with the same call made on a fresh context whose trackers were brought to the same state with set_tracks: what an
earlier call left in the shared buffers (their sizes, the painted mask, the cached weight table) must not show in a later one. The
sequence is built so that the scratch grows after single calls have used it (three full-frame regions need more list entries than
max_w * max_h) and so that the weight table's key changes with every refinement: (5,5), (3,3), (4,4), (5,5), (4,4)."""
import numpy as np
import pytest

import klt_common as kc

pytestmark = pytest.mark.gpu
W, H, MAX_TRACKS, N_SLOTS = 192, 144, 256, 6
SINGLE = dict(target=40, subpix=True, subpix_win=(5, 5))      # the tracker of the single steps
GROUP = dict(subpix=True, subpix_win=(4, 4))                  # the three trackers of the many-calls (targets below)
GROUP_TARGETS = (40, 33, 64)
STEREO = dict(fb_max_dist=0.5, border=1)


def _same(name, got, want):
    got, want = (got, want) if isinstance(got, (tuple, list)) else ((got,), (want,))
    assert len(got) == len(want), f"{name}: {len(got)} outputs, not {len(want)}"
    for k, (g, x) in enumerate(zip(got, want)):
        if isinstance(g, (tuple, list)):
            _same(f"{name}[{k}]", g, x)
            continue
        assert g.dtype == x.dtype and g.shape == x.shape, f"{name}, output {k}: {g.dtype}{g.shape} != {x.dtype}{x.shape}"
        assert g.tobytes() == x.tobytes(), f"{name}, output {k} differs from the fresh context's"


def _base_mask():
    m = np.full((H, W), 255, np.uint8)
    m[30:70, 50:120] = 0
    m[100:, :40] = 0
    return m


def _state_of(ids_xy, n, first_id):
    """a tracker state of the first n of the corners `ids_xy` ((k, 2) int32 frame coordinates)"""
    xy = ids_xy[:n].astype(np.float32)
    return np.arange(first_id, first_id + len(xy), dtype=np.int32), np.ones(len(xy), np.int32), xy, first_id + len(xy)


def run_sequence(pmv, note=None):
    """The eight calls on the shared context, each also made on a fresh one. note(label): called after every call on the shared context
    (while no fresh context is alive). Returns the list of (label, outputs on the shared context, outputs on the fresh one)."""
    frames = kc.scene(pmv, W, H)
    mask = _base_mask()
    calls = []

    def make_ctx():
        c = pmv.Context(W, H, n_slots=N_SLOTS, max_tracks=MAX_TRACKS)
        for i, f in enumerate(frames):
            c.frame_upload(i, f)
        return c

    def both(label, call, trackers=(), stereo=False):
        """call(ctx, trackers of that ctx): first on a fresh context whose trackers are copies of `trackers` (parameters, state, next id as
        the shared ones have them NOW), then on the shared one"""
        states = [(t.params, t.get_tracks(), t.next_id) for t in trackers]
        fresh = make_ctx()
        try:
            twins = []
            for p, (ids, ages, xy), next_id in states:
                t = fresh.klt_create(**p)
                t.set_tracks(ids, ages, xy, next_id)
                if stereo:
                    t.set_stereo(**STEREO)
                twins.append(t)
            want = call(fresh, twins)
        finally:
            fresh.close()
        got = call(shared, list(trackers))
        # next_id is the tracker's own: follow it through the step (counts[4] = the m new tracks of a step)
        for t, o in zip(trackers, got if trackers and isinstance(got, list) else [got]):
            t.next_id += int(o[4][4])
        calls.append((label, got, want))
        if note:
            note(label)

    def create(ctx, p, state):
        t = ctx.klt_create(**p)
        t.params = p
        t.set_tracks(*state)
        t.next_id = state[3]
        return t

    shared = make_ctx()
    try:
        # 1. the whole-frame detector on slot 0
        both("1 detect_gftt_frame", lambda c, _: c.detect_gftt_frame(0, 100, min_dist=6.0))
        c0 = calls[-1][1]
        assert len(c0) >= 64, "the scene gives too few corners for the trackers' states"
        # 2. a single step with refinement, window (5, 5), from 30 of those corners
        a = create(shared, kc.params(**SINGLE), _state_of(c0, 30, 0))
        both("2 klt_step", lambda c, t: t[0].step(0, 1), [a])
        assert calls[-1][1][4][0] == 30 and calls[-1][1][4][3] > 0 and calls[-1][1][4][4] > 0, "the step neither tracked nor refilled"
        # 3. the masked refill with a base mask, around the tracker's list
        trk_xy = a.get_tracks()[2]
        both("3 detect_gftt_refill", lambda c, _: c.detect_gftt_refill(1, 60, trk_xy, 10, base_mask=mask, min_dist=8.0))
        keep, c1 = calls[-1][1]
        assert 0 < keep.sum() and len(c1) >= 33
        # 4. the refinement alone, window (3, 3): another weight table
        both("4 corner_subpix", lambda c, _: c.corner_subpix(1, c1.astype(np.float32), win=(3, 3), return_info=True))
        # 5. three trackers with full-frame regions: 3 * W * H list entries and mask bytes, more than the single calls made
        group = [create(shared, kc.params(target=GROUP_TARGETS[0], **GROUP), _state_of(c1, 33, 100)),
                 create(shared, kc.params(target=GROUP_TARGETS[1], **GROUP), _state_of(c0, 20, 200)),
                 create(shared, kc.params(target=GROUP_TARGETS[2], **GROUP), _state_of(c1[::-1].copy(), 15, 300))]
        both("5 klt_step_many", lambda c, t: c.klt_step_many(t, [1, 0, 1], [2, 1, 2]), group)
        assert all(o[4][0] > 0 and o[4][3] > 0 and o[4][4] > 0 for o in calls[-1][1]), "a tracker of the group neither tracked nor refilled"
        # 6. the single step again: its table is no longer the cached one
        both("6 klt_step", lambda c, t: t[0].step(1, 2), [a])
        # 7. the whole-frame detector with a mask
        both("7 detect_gftt_frame", lambda c, _: c.detect_gftt_frame(3, 80, mask=mask))
        # 8. the stereo many-call on two of the group
        for t in group[:2]:
            t.set_stereo(**STEREO)
        both("8 klt_step_many_stereo", lambda c, t: c.klt_step_many_stereo(t, [2, 1], [3, 2], [4, 5]), group[:2], stereo=True)
        assert all(o[4][7] > 0 for o in calls[-1][1]), "no track of a tracker was matched in its right frame"
    finally:
        shared.close()
    return calls


def test_interleaved_calls_equal_fresh_contexts_and_free_their_memory(pmv):
    base = pmv.mem_live()
    live = []
    calls = run_sequence(pmv, lambda label: live.append((label, pmv.mem_live())))
    for label, m in live:
        print(f"mem_live after {label}: device {m[0] - base[0]}, pinned {m[1] - base[1]}")
    assert [c[0][0] for c in calls] == list("12345678")
    for label, got, want in calls:
        _same(label, got, want)
    assert pmv.mem_live() == base, "a buffer outlived its context"
