"""The KLT tracker's yardstick on the CPU twins alone (klt_common.twin_step): what the scenes of tests/test_klt_gpu.py are there for, and the
policy between the calls at its edges."""
import numpy as np
import pytest

import klt_common as kc


@pytest.mark.parametrize("size", kc.SIZES, ids=lambda s: "%dx%d" % s)
def test_every_stage_drops_and_the_refill_adds(pmv, size):
    w, h = size
    _, run = kc.scene_run(pmv, w, h, "default")
    c = np.stack([o[4] for _, o in run]).astype(np.int64)
    assert (c[0, :4] == 0).all() and c[0, 4] > 0                       # the first step only detects
    assert (c[1:, 0] - c[1:, 1] > 0).any(), "stage 2 drops nothing"
    assert (c[1:, 1] - c[1:, 2] > 0).any() and (c[1:, 5] == 1).all(), "stage 3 drops nothing"
    assert (c[1:, 2] - c[1:, 3] > 0).any(), "stage 4 drops nothing"
    assert (c[1:, 4] > 0).any(), "stage 5 adds nothing"
    made = 0
    for s, o in run:
        made += int(o[4][4])
        assert len(o[0]) == o[4][3] + o[4][4] <= kc.DEFAULTS["target"]
        assert len(set(o[0].tolist())) == len(o[0]) and s["next_id"] == made


@pytest.mark.parametrize("size", kc.SIZES, ids=lambda s: "%dx%d" % s)
def test_the_moving_block_is_what_rejectwithf_rejects(pmv, size):
    """with F off the block's tracks live on; with F on tracks are dropped at stage 3 in every step"""
    w, h = size
    _, on = kc.scene_run(pmv, w, h, "default")
    _, off = kc.scene_run(pmv, w, h, "f_off")
    assert sum(int(o[4][1] - o[4][2]) for _, o in on) >= 5
    assert all(o[4][5] == -1 and o[4][1] == o[4][2] for _, o in off)


def test_some_step_has_nothing_to_refill(pmv):
    w, h = kc.SIZES[0]
    _, run = kc.scene_run(pmv, w, h, "default", target=1)
    assert any(o[4][3] == 1 and o[4][4] == 0 for _, o in run)


@pytest.mark.parametrize("size", kc.SIZES, ids=lambda s: "%dx%d" % s)
def test_a_tiny_threshold_finds_no_model(pmv, size):
    w, h = size
    p = kc.params(f_threshold=kc.NO_MODEL_THRESHOLD)
    run = kc.twin_run(kc.scene(pmv, w, h)[:3], p, ("no-model", w, h))
    for _, o in run[1:]:
        c = o[4]
        assert c[1] >= 15 and c[5] == 0 and c[2] == 0 and c[3] == 0, "the twin found a model"
        assert c[4] > 0 and (o[1] == 1).all(), "stage 5 did not refill from nothing"


@pytest.mark.parametrize("name", list(kc.SETTINGS))
def test_ages_never_increase_along_the_list(pmv, name):
    for w, h in kc.SIZES:
        _, run = kc.scene_run(pmv, w, h, name)
        for _, o in run:
            assert (np.diff(o[1]) <= 0).all()
        assert max(int(o[1].max()) for _, o in run) >= 4


def test_more_than_1024_tracks_on_the_large_frames(pmv):
    _, run = kc.big_run(pmv)
    c = np.stack([o[4] for _, o in run])
    assert c[:, 0].max() > 1024 and c[1:, 3].min() > 0 and c[1:, 4].min() > 0


def test_the_border_test_rounds_half_to_even():
    w, h, b = 100, 80, 3
    x = np.asarray([b - 0.5, b + 0.5, b - 0.49, b - 1.5, w - b - 0.5, w - b - 1.5, w - b - 0.51, w - b - 1], np.float32)
    # 2.5 -> 2 (out), 3.5 -> 4 (in), 2.51 -> 3 (in), 1.5 -> 2 (out); 96.5 -> 96 (in: 96 < 97), 95.5 -> 96 (in), 96.49 -> 96 (in), 96 (in)
    pts = np.stack([x, np.full(len(x), 40, np.float32)], axis=1)
    assert kc.in_border(pts, b, w, h).tolist() == [False, True, True, False, True, True, True, True]
    assert kc.in_border(pts[:, ::-1], b, h + 20, w).tolist() == [False, True, True, False, True, True, True, True]
    even = np.asarray([[4.5, 40], [w - 4 - 0.5, 40], [w - 4 + 0.5, 40]], np.float32)   # 4.5 -> 4 (in at border 4), 95.5 -> 96 (out: 96 >= 96), 96.5 -> 96 (out)
    assert kc.in_border(even, 4, w, h).tolist() == [True, False, False]
    assert not kc.in_border(np.asarray([[np.nan, 40.0]], np.float32), 0, w, h)[0]


def test_the_forward_backward_comparison_at_equality():
    prev = np.zeros((4, 2), np.float32)   # (at the origin, so that back - prev is the offset itself)
    back = prev + np.asarray([[0.3, 0.4], [0.5, 0.0], [np.nextafter(np.float32(0.5), np.float32(1)), 0], [0.0, -0.5]], np.float32)
    # 0.3f^2 + 0.4f^2 in float32 against (float)(0.5 * 0.5): whatever float32 gives, computed here step by step
    d = back - prev
    want = [bool(np.float32(np.float32(a * a) + np.float32(b * b)) <= np.float32(0.25)) for a, b in d]
    assert kc.fb_ok(prev, back, 0.5).tolist() == want
    assert want[1] and want[3] and not want[2]
    assert kc.fb_ok(prev, prev, 0.0).all()   # a threshold of 0 keeps the exact returns
